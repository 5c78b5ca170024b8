"""The batched character controller on the device (sgp_characters_*, shim/CharacterBatch.h) against the host class it restates (shim/Jolt/JoltCharacterLite.h).

tests/cpp/characters_batch.cpp sets up one small scene per branch of CharacterVirtual::Update / ExtendedUpdate, walks it with JPH::CharacterVirtual objects one
after the other (PlayerPhysics' listener attached) and then with ONE batch from the same starting states, and prints both records.  Discrete results -- ground
state, ground body, the contact-added records and their order, the overflow bit -- must be equal at every update; positions and velocities must agree to the
project's parity tolerance (tests/test_parity_gpu.py: 1e-4 m, 1e-3 m/s).  Both sides evaluate the same fp32 expressions without contraction, so bit equality is
the expectation; every scene prints how many of its values are bit-equal."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

from substrata_amd import abi, build
from test_facade_gpu import build_facade_exe

pytestmark = pytest.mark.gpu

POS_TOL, VEL_TOL = 1.0e-4, 1.0e-3          # tests/test_parity_gpu.py:16-17
ON_GROUND, ON_STEEP, NOT_SUPPORTED, IN_AIR = 0, 1, 2, 3
INVALID = 0xFFFFFFFF


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return build_facade_exe(tmp_path_factory.mktemp("characters"), "characters_batch.cpp")


_runs = {}


def run(exe, *args):
    """One run of the program per argument list, shared by the tests that read it (never modified)."""
    if args not in _runs:
        r = subprocess.run([exe, *args], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        _runs[args] = json.loads(r.stdout)
    return _runs[args]


def f32(a):
    return np.asarray(a, dtype=np.uint32).view(np.float32)


def frames(rec):
    """{(frame, character): dict} of one walk."""
    out = {}
    for row in rec["frames"]:
        out[(row[0], row[1])] = dict(gs=row[2], gbody=row[3], overflow=row[4], pos=f32(row[5:8]), vel=f32(row[8:11]), gn=f32(row[11:14]), gv=f32(row[14:17]), bits=row[5:17])
    return out


def contacts(rec):
    return [(row[0], row[1], row[2], row[3]) for row in rec["contacts"]]


def compare(name, host, batch):
    """The assertions every scene shares; returns the batch's frames."""
    hf, bf = frames(host), frames(batch)
    assert hf.keys() == bf.keys() and len(hf) > 0
    equal = total = 0
    worst_p = worst_v = 0.0
    for key in sorted(hf):
        h, b = hf[key], bf[key]
        assert (h["gs"], h["gbody"]) == (b["gs"], b["gbody"]), (name, key, h, b)
        assert b["overflow"] == 0, (name, key)
        worst_p = max(worst_p, float(np.abs(h["pos"] - b["pos"]).max()))
        worst_v = max(worst_v, float(np.abs(h["vel"] - b["vel"]).max()), float(np.abs(h["gv"] - b["gv"]).max()))
        assert np.abs(h["pos"] - b["pos"]).max() <= POS_TOL, (name, key, h["pos"], b["pos"])
        assert np.abs(h["vel"] - b["vel"]).max() <= VEL_TOL and np.abs(h["gv"] - b["gv"]).max() <= VEL_TOL, (name, key)
        assert np.abs(h["gn"] - b["gn"]).max() <= POS_TOL, (name, key, h["gn"], b["gn"])
        equal += sum(int(x == y) for x, y in zip(h["bits"], b["bits"])); total += len(h["bits"])
    print(f"{name}: {equal} of {total} values bit-equal; worst position difference {worst_p:.3g} m, velocity {worst_v:.3g} m/s; host walk met at most {host['max_contacts']} contacts")
    assert host["max_contacts"] < abi.CHAR_MAX_CONTACTS
    assert contacts(host) == contacts(batch), name            # the set and the order of the contact-added records
    for hrow, brow in zip(host["contacts"], batch["contacts"]):
        assert np.abs(f32(hrow[4:7]) - f32(brow[4:7])).max() <= POS_TOL and np.abs(f32(hrow[7:10]) - f32(brow[7:10])).max() <= POS_TOL, name
    return bf


def states(bf, ch=0):
    return [bf[k]["gs"] for k in sorted(bf) if k[1] == ch]


def test_flat_floor_fall_land_walk_stop(exe):
    d = run(exe, "flat")
    bf = compare("flat", d["host"], d["batch"])
    gs = states(bf)
    assert gs[0] == IN_AIR and gs[-1] == ON_GROUND and ON_GROUND in gs[:30]
    assert bf[(44, 0)]["pos"][0] > 0.4                                              # it walked
    assert np.array_equal(bf[(59, 0)]["pos"][:2], bf[(50, 0)]["pos"][:2]) and abs(bf[(59, 0)]["pos"][2] - bf[(50, 0)]["pos"][2]) < 1.0e-6      # ... and stands still once stopped (no-slide at rest)
    assert len(d["batch"]["contacts"]) == 1                                         # the floor, once


def test_staircase_is_climbed_and_a_block_is_not(exe):
    d = run(exe, "stairs")
    bf = compare("stairs", d["host"], d["batch"])
    assert bf[(59, 0)]["pos"][2] > 0.55 and bf[(59, 0)]["pos"][0] > 2.0             # on the third step (0.6 m)
    # the 0.6 m block: the 0.4 m step up does not clear it, the step comes down on the block's edge (the rounded nose: the second cast of WalkStairs finds the
    # top further ahead) and the character stands on that edge as OnSteepGround -- the updates that START there run CancelVelocityTowardsSteepSlopes
    d = run(exe, "block")
    bf = compare("block", d["host"], d["batch"])
    gs = states(bf)
    assert ON_STEEP in gs[:-1] and gs[-1] != ON_STEEP and max(bf[k]["pos"][2] for k in bf) > 0.6
    # a 1 m block stops both
    d = run(exe, "block10")
    bf = compare("block10", d["host"], d["batch"])
    assert max(bf[k]["pos"][2] for k in bf) < 0.05 and bf[(59, 0)]["pos"][0] < 0.8 - 0.3 + 0.05      # WalkStairs refused in every update: never off the floor


def test_steep_ramp_is_not_climbed(exe):
    """Walking against the 60 degree ramp from the floor: the vertical wall constraint of the steep contact stops the character at the ramp's foot."""
    d = run(exe, "ramp60")
    bf = compare("ramp60", d["host"], d["batch"])
    assert max(bf[k]["pos"][2] for k in bf) < 0.05 and set(states(bf)) == {ON_GROUND}
    assert abs(bf[(59, 0)]["pos"][0] - bf[(30, 0)]["pos"][0]) < 2.0e-3 and bf[(59, 0)]["pos"][0] < -1.0      # held where it met the ramp


def test_steep_ground_cancels_the_velocity_towards_the_slope(exe):
    """Dropped onto the 60 degree ramp while pushing into it: OnSteepGround, and the updates that start in that state run CancelVelocityTowardsSteepSlopes."""
    d = run(exe, "steep_drop")
    bf = compare("steep_drop", d["host"], d["batch"])
    gs = states(bf)
    first = gs.index(ON_STEEP)
    assert first < 58 and gs[first + 1] in (ON_STEEP, NOT_SUPPORTED, ON_GROUND, IN_AIR)
    # the update after it started on steep ground: what it asked for (3 m/s along +x, into the slope) was cut down
    assert bf[(first + 1, 0)]["vel"][0] < 3.0 - 1.0e-3


def test_plain_update_neither_climbs_nor_sticks(exe):
    """SGP_CHAR_EXTENDED unset: CharacterVirtual::Update alone; the 0.2 m step that ExtendedUpdate climbs (the stairs scene) stops it."""
    d = run(exe, "plain")
    bf = compare("plain", d["host"], d["batch"])
    assert states(bf)[0] == IN_AIR and ON_GROUND in states(bf)
    assert max(bf[k]["pos"][2] for k in bf if k[0] > 30) < 0.15 and bf[(59, 0)]["pos"][0] < 0.8


def test_down_a_slope_at_speed_sticks_to_the_floor(exe):
    """StickToFloor taken: past the crest the slope falls away faster than gravity brings the character down, and every update puts it back on the ground."""
    d = run(exe, "downslope")
    bf = compare("downslope", d["host"], d["batch"])
    gs = states(bf)
    over = [k[0] for k in sorted(bf) if 0.1 < bf[k]["pos"][0] < 1.6]      # the updates that end over the slope
    assert len(over) >= 15 and all(gs[f] == ON_GROUND for f in over)       # never in the air on the way down ...
    drops = [bf[(f, 0)]["pos"][2] - bf[(f + 1, 0)]["pos"][2] for f in over[:-1]]
    assert min(drops) > 0.03                                                # ... and 3.8 cm lower each update: ten times what gravity alone gives (0.27 cm)


@pytest.mark.parametrize("scene", ["ramp35_noslide", "ramp35_slide"])
def test_walkable_ramp_standing_still(exe, scene):
    d = run(exe, scene)
    bf = compare(scene, d["host"], d["batch"])
    assert states(bf)[-1] == ON_GROUND
    moved = float(np.abs(bf[(59, 0)]["pos"] - bf[(40, 0)]["pos"]).max())
    assert (moved == 0.0) if scene == "ramp35_noslide" else (moved > 1.0e-3)


def test_inside_corner_stops(exe):
    d = run(exe, "corner")
    bf = compare("corner", d["host"], d["batch"])
    p = bf[(59, 0)]["pos"]
    assert p[0] < 1.0 - 0.3 + 0.05 and p[1] < 1.1 - 0.3 + 0.05 and float(np.abs(p - bf[(55, 0)]["pos"]).max()) < 1.0e-3


def test_ledges_stick_to_floor_or_fall(exe):
    d = run(exe, "ledge03")
    bf = compare("ledge03", d["host"], d["batch"])
    # (StickToFloor's cast is made as the character leaves the edge; while the capsule's round bottom still touches the box's edge the cast reports that
    # edge, too steep to stand on, and the host class lets go: both sides then fall the 0.3 m)
    assert bf[(59, 0)]["pos"][2] < 0.05 and states(bf)[-1] == ON_GROUND and bf[(59, 0)]["gbody"] == 0
    d = run(exe, "ledge10")
    bf = compare("ledge10", d["host"], d["batch"])
    assert states(bf).count(IN_AIR) > states(frames(run(exe, "ledge03")["batch"])).count(IN_AIR) and states(bf)[-1] == ON_GROUND


@pytest.mark.parametrize("scene", ["mesh", "field"])
def test_mesh_floor_and_height_field(exe, scene):
    d = run(exe, scene)
    bf = compare(scene, d["host"], d["batch"])
    assert states(bf)[-1] == ON_GROUND and bf[(59, 0)]["pos"][0] - bf[(0, 0)]["pos"][0] > 1.0      # walked on, across the seam / over the cells


def test_kinematic_platform_carries_the_character(exe):
    d = run(exe, "platform")
    bf = compare("platform", d["host"], d["batch"])
    assert abs(bf[(59, 0)]["gv"][1] - 1.0) < 0.05 and bf[(59, 0)]["pos"][1] - bf[(20, 0)]["pos"][1] > 0.5      # ground velocity; no-slide did not hold it back


def test_sensor_is_reported_and_walked_through(exe):
    d = run(exe, "sensor")
    bf = compare("sensor", d["host"], d["batch"])
    assert bf[(59, 0)]["pos"][0] > 2.5 and len({c[2] for c in contacts(d["batch"])}) == 2      # floor and sensor, one record each
    assert len(contacts(d["batch"])) == 2


def test_ignored_body_is_walked_through(exe):
    d = run(exe, "ignored")
    bf = compare("ignored", d["host"], d["batch"])
    assert bf[(59, 0)]["pos"][0] > 2.5 and len(contacts(d["batch"])) == 1


def test_dynamic_box_is_pushed_alike(exe):
    d = run(exe, "push")
    compare("push", d["host"], d["batch"])
    hb, bb = f32(d["host"]["box"]), f32(d["batch"]["box"])
    print("box, host walk :", hb, "\nbox, batch     :", bb, "\nbit-equal:", int((np.asarray(d["host"]["box"]) == np.asarray(d["batch"]["box"])).sum()), "of 13")
    assert hb[0] > 1.0 + 1.0e-3                                                     # it moved
    assert np.abs(hb[:3] - bb[:3]).max() <= POS_TOL and np.abs(hb[7:] - bb[7:]).max() <= VEL_TOL and np.abs(hb[3:7] - bb[3:7]).max() <= POS_TOL


def test_two_characters_one_box_same_bits_every_run(exe):
    d = run(exe, "two_push")
    assert d["batch"]["frames"] == d["batch2"]["frames"] and d["batch"]["contacts"] == d["batch2"]["contacts"] and d["batch"]["box"] == d["batch2"]["box"]
    assert abs(f32(d["batch"]["box"])[:2]).max() > 1.0e-4 or abs(f32(d["batch"]["box"])[7:]).max() > 1.0e-4      # both pushed: it did not stay put


def test_seventy_characters_each_as_alone_in_any_order(exe):
    """More characters than a wave has lanes: each equals its own single-character batch bit for bit, and the order of adding them changes nothing."""
    together, alone, rev = run(exe, "many", "all")["batch"], run(exe, "many", "single")["batch"], run(exe, "many", "reversed")["batch"]
    key = lambda rows: sorted(map(tuple, rows))
    assert len(together["frames"]) == 70 * 60
    assert key(together["frames"]) == key(alone["frames"])
    assert key(together["frames"]) == key(rev["frames"])
    by_char = lambda rec: {c: [r for r in rec["contacts"] if r[1] == c] for c in range(70)}
    assert by_char(together) == by_char(alone) == by_char(rev)
    assert [r[1] for r in together["contacts"] if r[0] == 0] == sorted(r[1] for r in together["contacts"] if r[0] == 0)      # ascending character within a drain
    z = [f32(r[5:8])[2] for r in together["frames"] if r[0] == 59]
    assert max(z) > 0.55 and all(r[4] == 0 for r in together["frames"])            # some climbed the stairs; nobody overflowed


# ---- lifecycle, through the Python wrapper ------------------------------------------------------------------------------------------------------

@pytest.fixture()
def world():
    from substrata_amd.world import CWorld
    lib = C.CDLL(build.build())
    abi.bind(lib, "sgp_")
    assert lib.sgp_init() >= 1
    w = CWorld(lib, "sgp_", max_bodies=256)
    d = w.default_body_desc()
    d.shape[:] = (20.0, 20.0, 0.5, 0.0); d.pos[:] = (0.0, 0.0, -0.5)
    w.add(d)
    yield w
    w.close()


def char_desc(cs):
    d = cs.default_desc()
    d.up[:] = (0.0, 0.0, 1.0); d.shape_offset[:] = (0.0, 0.0, 0.95); d.supporting_plane[:] = (0.0, 0.0, 1.0, -0.3)
    d.stick_to_floor_step_down[:] = (0.0, 0.0, -0.5); d.walk_stairs_step_up[:] = (0.0, 0.0, 0.4)
    return d


def inputs(n, vel=(0.0, 0.0, -0.1635), flags=abi.CHAR_EXTENDED):
    a = np.zeros(n, dtype=abi.character_input_dtype)
    a["velocity"] = vel; a["ignore_id"] = INVALID; a["flags"] = flags
    return a


def test_states_without_an_update_are_the_set_values(world):
    cs = world.characters(4)
    a, b = cs.add(char_desc(cs), (1.0, 2.0, 3.0)), cs.add(char_desc(cs), (4.0, 5.0, 6.0))
    assert (a, b) == (0, 1)
    i = inputs(2); i["velocity"][1] = (0.5, 0.25, -1.0)
    cs.set_inputs(0, i)
    s = cs.states(0, 3)
    assert s["pos"].tolist() == [[1, 2, 3], [4, 5, 6], [0, 0, 0]] and s["lin_vel"][1].tolist() == [0.5, 0.25, -1.0]
    assert s["ground_state"].tolist() == [IN_AIR] * 3 and s["ground_body"].tolist() == [INVALID] * 3
    cs.set_pose([1], [(7.0, 8.0, 9.0)])
    assert cs.states(1, 1)["pos"].tolist() == [[7, 8, 9]]
    cs.close()


def test_removed_slot_is_reused_and_carries_nothing_over(world):
    cs = world.characters(2)
    a = cs.add(char_desc(cs), (0.0, 0.0, 0.0))
    cs.set_inputs(0, inputs(1))
    for _ in range(3):
        cs.update()
    s = cs.states(0, 1)
    assert s["ground_state"][0] == ON_GROUND and s["ground_body"][0] == 0 and len(cs.drain_contacts()) == 1
    cs.remove(a)
    b = cs.add(char_desc(cs), (0.0, 0.0, 5.0))      # high above the floor
    assert b == a
    s = cs.states(0, 1)
    assert s["ground_state"][0] == IN_AIR and s["ground_body"][0] == INVALID and s["pos"][0].tolist() == [0, 0, 5] and not s["ground_normal"].any()
    cs.set_inputs(0, inputs(1))
    cs.update()
    assert cs.states(0, 1)["ground_state"][0] == IN_AIR and len(cs.drain_contacts()) == 0
    cs.set_pose([b], [(0.0, 0.0, 0.0)])
    cs.update()
    assert cs.states(0, 1)["ground_state"][0] == ON_GROUND and len(cs.drain_contacts()) == 1      # the floor is new to the new character
    cs.close()


def test_disabled_characters_do_not_move_and_emit_nothing(world):
    cs = world.characters(2)
    cs.add(char_desc(cs), (0.0, 0.0, 0.0)); cs.add(char_desc(cs), (2.0, 0.0, 0.0))
    i = inputs(2, vel=(1.0, 0.0, -0.1635)); i["flags"][1] |= abi.CHAR_DISABLED
    cs.set_inputs(0, i)
    for _ in range(5):
        cs.update()
    s = cs.states(0, 2)
    assert s["pos"][0][0] > 0.05 and s["pos"][1].tolist() == [2, 0, 0] and s["ground_state"][1] == IN_AIR
    assert set(cs.drain_contacts()["character"].tolist()) == {0}
    cs.close()


def test_degenerate_characters_and_bad_ranges_are_refused(world):
    from substrata_amd.world import SgpError
    cs = world.characters(2)
    d = char_desc(cs); d.radius = 0.0
    with pytest.raises(SgpError):
        cs.add(d, (0.0, 0.0, 0.0))
    cs.add(char_desc(cs), (0.0, 0.0, 0.0))
    with pytest.raises(SgpError):
        cs.set_inputs(0, inputs(1, vel=(float("nan"), 0.0, 0.0)))
    with pytest.raises(SgpError):
        cs.set_inputs(1, inputs(1))            # beyond the last character
    with pytest.raises(SgpError):
        cs.remove(1)
    with pytest.raises(SgpError):
        cs.states(0, 3)                        # beyond the capacity
    with pytest.raises(SgpError):
        cs.update(0.0)
    cs.close()


def test_destroy_after_the_world_is_safe():
    """sgp_characters_destroy after sgp_world_destroy frees the batch; anything else on such a batch is refused."""
    from substrata_amd.world import CWorld
    lib = C.CDLL(build.build())
    abi.bind(lib, "sgp_")
    assert lib.sgp_init() >= 1
    w = CWorld(lib, "sgp_", max_bodies=64)
    cs = w.characters(2)
    cs.add(char_desc(cs), (0.0, 0.0, 1.0))
    cs.update()
    h = cs._h
    w.close()
    assert lib.sgp_characters_update(h, 1.0 / 60.0) == abi.ERR_INVALID
    assert lib.sgp_characters_destroy(h) == abi.OK
    cs._h = C.c_void_p()


def test_set_shape_switches_to_the_sitting_capsule(world):
    """PlayerPhysics.cpp:71-79: a shorter capsule at a lower offset; a beam the standing capsule touches is out of the sitting one's reach."""
    d = world.default_body_desc()
    d.shape[:] = (1.0, 1.0, 0.1, 0.0); d.pos[:] = (0.0, 0.0, 2.05)      # underside at z = 1.95: 0.05 m above the standing capsule's top (1.9), inside its 0.12 m reach
    beam = world.add(d)
    cs = world.characters(1)
    c = cs.add(char_desc(cs), (0.0, 0.0, 0.0))
    cs.set_inputs(0, inputs(1))
    cs.update()
    assert sorted(cs.drain_contacts()["body"].tolist()) == [0, beam]
    cs.remove(c)
    c = cs.add(char_desc(cs), (0.0, 0.0, 0.0))
    cs.set_shape(c, 0.3, 0.3, (0.0, 0.0, 0.6))      # top at z = 1.2
    cs.set_inputs(0, inputs(1))
    cs.update()
    assert cs.drain_contacts()["body"].tolist() == [0] and cs.states(0, 1)["ground_state"][0] == ON_GROUND
    cs.close()


def test_a_push_from_beyond_the_first_64_characters_wakes_a_sleeping_box(world):
    """k_characters_push finds pushers 64 at a time; waking is done on the device, and the step after the update is not skipped as idle."""
    d = world.default_body_desc()
    d.motion_type = abi.MOTION_DYNAMIC; d.layer = abi.LAYER_MOVING; d.mass = 10.0
    d.shape[:] = (0.3, 0.3, 0.3, 0.0); d.pos[:] = (0.0, 10.0, 0.3); d.activate = 1
    box = world.add(d)
    for _ in range(120):
        world.step(1.0 / 60.0)
    before = world.get_state([box])[0]
    assert before["active"] == 0                                            # asleep on the floor
    cs = world.characters(80)
    for i in range(70):
        cs.add(char_desc(cs), (-15.0 + 0.7 * i, -5.0, 0.0) if i != 69 else (-0.75, 10.0, 0.0))
    i = inputs(70, vel=(0.0, 0.0, -0.1635)); i["velocity"][69] = (1.5, 0.0, -0.1635)
    cs.set_inputs(0, i)
    for _ in range(20):
        cs.update()
        world.step(1.0 / 60.0)
    after = world.get_state([box])[0]
    assert after["active"] == 1 and after["pos"][0] > before["pos"][0] + 1.0e-3
    assert not cs.states(0, 70)["overflow"].any()
    cs.close()
