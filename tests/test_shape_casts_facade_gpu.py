"""The facade's castShapes (tests/cpp/shape_casts.cpp): a hull lowered onto a pile until it rests, a platform's box swept up to a wall, and the rail that
passes between a capsule's two end spheres but not the capsule."""
import subprocess

import pytest

from test_facade_gpu import build_facade_exe


def test_shape_casts_compiles(tmp_path):
    assert build_facade_exe(tmp_path, "shape_casts.cpp")


@pytest.mark.gpu
def test_shape_casts_place_stop_and_catch_the_rail(tmp_path):
    exe = build_facade_exe(tmp_path, "shape_casts.cpp")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout + r.stderr
