"""The facade's collideShapes / getObjectsInBox (tests/cpp/parcel_triggers.cpp): objects dropped inside and outside a parcel's box; the box's contents
must be exactly the inside objects and the ground it reaches."""
import subprocess

import pytest

from test_facade_gpu import build_facade_exe


def test_parcel_triggers_compiles(tmp_path):
    assert build_facade_exe(tmp_path, "parcel_triggers.cpp")


@pytest.mark.gpu
def test_parcel_triggers_finds_exactly_the_inside_objects(tmp_path):
    exe = build_facade_exe(tmp_path, "parcel_triggers.cpp")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout + r.stderr
