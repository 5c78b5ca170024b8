"""Checkpoint and rollback of a driven character batch (sgp_characters_checkpoint / _rollback take the drive records and the device's drive states along): world and
batch are captured while a jump is PENDING -- pressed and not yet fired --, run on, rolled back and run again: states, drive states and drained contacts of the
second pass are the first pass's, byte for byte.  A removed and re-added slot starts with num_jumps = 0 and no pending jump."""
import ctypes as C

import numpy as np
import pytest

from substrata_amd import abi, build
from test_players_gpu import player_desc, drives, extended, ON_GROUND, IN_AIR

pytestmark = pytest.mark.gpu
DT = 1.0 / 60.0


@pytest.fixture()
def world():
    from substrata_amd.world import CWorld
    lib = C.CDLL(build.build())
    abi.bind(lib, "sgp_")
    assert lib.sgp_init() >= 1
    w = CWorld(lib, "sgp_", max_bodies=64)
    d = w.default_body_desc()
    d.shape[:] = (20.0, 20.0, 0.5, 0.0); d.pos[:] = (0.0, 0.0, -0.5)
    w.add(d)
    d = w.default_body_desc()      # a box in the walker's way: a contact-added record behind the capture
    d.shape[:] = (0.5, 2.0, 1.0, 0.0); d.pos[:] = (2.0, 0.0, 1.0)
    w.add(d)
    yield w
    w.close()


def run_on(world, cs, first_frame, n):
    """n frames from first_frame on: the walker changes its mind half way; what every frame leaves, as bytes"""
    out = []
    for k in range(first_frame, first_frame + n):
        if k == first_frame + n // 2:
            cs.set_drive(0, drives(cs, 1, move=(0.0, 1.5, 0.0)))
        cs.update_at(DT, k * DT)
        world.step(DT)
        out.append((cs.states(0, 4).tobytes(), cs.drive_states(0, 4).tobytes(), cs.drain_contacts().tobytes()))
    return out


def test_rollback_with_a_jump_pending_replays_bit_for_bit(world):
    cs = world.characters(4)
    cs.add(player_desc(cs), (0.0, 0.0, 0.0))           # 0 walks into the box
    cs.add(player_desc(cs), (0.0, 3.0, 0.6))           # 1 is dropped from 0.6 m: it lands in the 20th update or so
    cs.add(player_desc(cs), (0.0, -3.0, 0.0))          # 2 stands, undriven
    cs.set_inputs(0, extended(3))
    d = drives(cs, 2); d["move_desired_vel"][0] = (3.0, 0.0, 0.0)
    cs.set_drive(0, d)
    for k in range(17):
        cs.update_at(DT, k * DT)
        world.step(DT)
    cs.jump([1], 17 * DT)                              # pressed in the air ...
    cs.update_at(DT, 17 * DT)
    world.step(DT)
    s, ds = cs.states(0, 3), cs.drive_states(0, 3)
    assert s["ground_state"][1] == IN_AIR and ds["num_jumps"][1] == 0 and s["ground_state"][0] == ON_GROUND      # ... and not fired yet: pending at the capture
    wcp, bcp = world.checkpoint(), cs.checkpoint()
    first = run_on(world, cs, 18, 40)
    ds = cs.drive_states(0, 3)
    assert ds["num_jumps"].tolist() == [0, 1, 0]       # the pending jump fired on landing, within its 0.1 s
    assert any(np.frombuffer(f[2], dtype=abi.character_contact_dtype).size for f in first)      # the walker met the box behind the capture
    # a foreign history before the rollback: another jump, another drive
    cs.jump([0, 1], 58 * DT); cs.set_drive(0, drives(cs, 2, move=(-2.0, 0.0, 0.0), flags=abi.DRIVE_ON | abi.DRIVE_FLY))
    for k in range(58, 63):
        cs.update_at(DT, k * DT)
        world.step(DT)
    cs.rollback(bcp); world.rollback(wcp)
    second = run_on(world, cs, 18, 40)
    assert second == first
    bcp.close(); wcp.close()
    cs.close()


def test_removed_slot_leaves_nothing_of_its_drive(world):
    cs = world.characters(2)
    a = cs.add(player_desc(cs), (0.0, 0.0, 0.0))
    cs.set_inputs(0, extended(1)); cs.set_drive(0, drives(cs, 1, move=(1.0, 0.0, 0.0)))
    for k in range(4):
        cs.update_at(DT, k * DT)
    cs.jump([a], 4 * DT)
    cs.update_at(DT, 4 * DT)
    assert cs.drive_states(0, 1)["num_jumps"][0] == 1
    cs.jump([a], 5 * DT)                               # pressed again, in the air: pending when the character goes
    cs.remove(a)
    b = cs.add(player_desc(cs), (5.0, 5.0, 0.0))
    assert b == a
    ds = cs.drive_states(0, 1)
    assert ds["num_jumps"][0] == 0 and ds["jumped"][0] == 0 and ds["on_ground"][0] == 0 and ds["campos_z_delta"][0] == 0.0
    cs.set_inputs(0, extended(1))
    for k in range(5, 9):                              # the slot's new character is not driven (the old drive is gone: it does not walk) ...
        cs.update_at(DT, k * DT)
    s = cs.states(0, 1)
    assert s["pos"][0][0] == 5.0 and cs.drive_states(0, 1)["num_jumps"][0] == 0
    cs.set_drive(0, drives(cs, 1))                     # ... and driven, it does not jump: the old character's press went with it
    for k in range(9, 14):
        cs.update_at(DT, k * DT)
    ds = cs.drive_states(0, 1)
    assert ds["num_jumps"][0] == 0 and ds["on_ground"][0] == 1 and cs.states(0, 1)["ground_state"][0] == ON_GROUND
    cs.close()
