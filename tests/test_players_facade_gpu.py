"""shim/PlayerBatch.h through a caller program (tests/cpp/players_facade.cpp): four players at once over the route of tests/cpp/player_controller.cpp's parts 1-5
and 9 -- fall and land, walk, the 0.3 m step, the wall, the jump, swimming -- with no readBack inside a part; that file's position checks are applied at the end
of each part, by the program itself."""
import subprocess

import pytest

from test_facade_gpu import build_facade_exe

pytestmark = pytest.mark.gpu


def test_four_players_walk_the_player_controller_route_without_reading_back(tmp_path):
    exe = build_facade_exe(tmp_path, "players_facade.cpp")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0 and "players: ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
