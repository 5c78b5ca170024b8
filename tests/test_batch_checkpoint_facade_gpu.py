"""saveState / restoreState of the facade's batches (tests/cpp/batch_checkpoint_facade.cpp): a MoverBatch with a follower that is waiting for its leader at
the capture, a CraftBatch and its ParticleBatch are saved next to PhysicsWorld::checkpoint, run on, restored and run again: the same bytes."""
import subprocess

import pytest

from test_facade_gpu import build_facade_exe


def test_batch_checkpoint_facade_compiles(tmp_path):
    assert build_facade_exe(tmp_path, "batch_checkpoint_facade.cpp")


@pytest.mark.gpu
def test_batch_checkpoint_facade_restore_replays(tmp_path):
    exe = build_facade_exe(tmp_path, "batch_checkpoint_facade.cpp")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "identical 1" in r.stdout and "carriage waiting again 1, same handles 1" in r.stdout and "in place 1, movers alive 3" in r.stdout
