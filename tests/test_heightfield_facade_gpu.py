"""The facade's createJoltHeightFieldShape (a native height field) against createMeshShape of the same triangles: identical transforms,
ray hits and player positions (tests/cpp/heightfield_facade.cpp)."""
import subprocess

import pytest

from test_facade_gpu import build_facade_exe


def test_heightfield_facade_compiles(tmp_path):
    assert build_facade_exe(tmp_path, "heightfield_facade.cpp")


@pytest.mark.gpu
def test_heightfield_facade_matches_mesh(tmp_path):
    exe = build_facade_exe(tmp_path, "heightfield_facade.cpp")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
