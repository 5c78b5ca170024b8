"""PhysicsWorld::checkpoint / rollback / saveState of the facade (tests/cpp/checkpoint_facade.cpp): a rolled-back facade world -- ground, boxes,
a mesh object, a car -- replays the same object transforms, activated_obs membership and contact callbacks."""
import subprocess

import pytest

from test_facade_gpu import build_facade_exe


def test_checkpoint_facade_compiles(tmp_path):
    assert build_facade_exe(tmp_path, "checkpoint_facade.cpp")


@pytest.mark.gpu
def test_checkpoint_facade_rollback_replays(tmp_path):
    exe = build_facade_exe(tmp_path, "checkpoint_facade.cpp")
    r = subprocess.run([exe, str(tmp_path / "world.ckpt")], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "identical 1" in r.stdout and "refused 1, world untouched 1" in r.stdout
