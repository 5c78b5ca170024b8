"""Known answers of the crafts' restatement (tests/craft_reference.py, written from docs/CONTRACT.md "Crafts") against closed forms, the generator's stated
values, and the branch margins of the seeded table the device parity test runs (tests/craft_scenes.py).  No device."""
import numpy as np
import pytest

import craft_reference as cr
import craft_scenes as cs
from helpers import DT, dyn

F = np.float32
LEVEL = dict(pos=(0, 0, 5), rot=(0, 0, 0, 1), lin_vel=(0, 0, 0), ang_vel=(0, 0, 0), submerged=0.0)
NO_INPUT = dict(forward=0.0, right=0.0, up=0.0, hand_brake=0.0, flags=cr.IN_DRIVER)
NO_WATER = (False, 0.0)


def vec(v):
    return np.array([float(x) for x in v])


def test_level_hover_car_gets_exactly_its_weight():
    d = cr.default_desc(cr.HOVERCAR, mass=1234.5)
    r = cr.craft_update(d, NO_INPUT, LEVEL, (-1, -1), NO_WATER, None, 0, DT)
    assert r["branches"] == cr.BR["HOVER"] and r["unflip"] == F(-1) and not r["particles"]
    forces = [op[1] for op in r["ops"] if op[0] == "force"]
    assert forces[0][0] == 0 and forces[0][1] == 0 and forces[0][2] == F(1234.5) * F(9.81) and forces[0][2].dtype == np.float32
    assert all(float(np.abs(vec(op[1])).max()) == 0.0 for op in r["ops"][1:])      # the control forces and torques of no input, the correction of a level car
    assert [op[0] for op in r["ops"]] == ["force", "force", "force", "torque", "torque", "torque", "torque"]
    # ... plus drag once it moves: straight down at 3 m/s only the top area sees the flow, 0.5 rho v^2 C_d A = 0.5 * 1.293 * 9 * 0.75 * 8 upwards
    r = cr.craft_update(d, NO_INPUT, dict(LEVEL, lin_vel=(0, 0, -3)), (-1, -1), NO_WATER, None, 0, DT)
    assert r["branches"] == cr.BR["HOVER"] | cr.BR["DRAG"]      # (no lift: the flow is along the up axis, the lift direction has no length)
    drag = [op[1] for op in r["ops"] if op[0] == "force"][3]
    assert drag[0] == 0 and drag[1] == 0 and abs(float(drag[2]) - 0.5 * 1.293 * 9 * 0.75 * 8) < 1e-4


def test_hovering_car_keeps_its_height_over_120_steps(oracle):
    """The up force is mass * 9.81f and the world's gravity is -9.81f: what is left is the rounding of their cancellation, a few ulp of 9.81 times (2 s)^2."""
    w = oracle.OracleWorld(max_bodies=16)
    b = dyn(w, shape=(0.9, 2.0, 0.4, 0.0), pos=(0, 0, 5), mass=1000.0, allow_sleeping=0)
    d = cr.default_desc(cr.HOVERCAR, mass=1000.0)
    timers = (-1.0, -1.0)
    z0 = float(w.read_states(b, 1)["pos"][0][2])
    for step in range(120):
        s = w.read_states(b, 1)[0]
        r = cr.craft_update(d, NO_INPUT, dict(pos=s["pos"], rot=s["rot"], lin_vel=s["lin_vel"], ang_vel=s["ang_vel"], submerged=0.0), timers, NO_WATER, None, step, DT)
        timers = (r["unflip"], r["righting"])
        for op in r["ops"]:
            if op[0] == "force":
                w.add_force(b, vec(op[1]))
            elif op[0] == "torque":
                w.add_torque(b, vec(op[1]))
        w.step(DT)
    dz = abs(float(w.read_states(b, 1)["pos"][0][2]) - z0)
    print(f"height change after 120 steps: {dz:.3e} m")
    assert dz < 1.0e-4
    w.close()


def test_level_boat_drag_is_the_closed_form():
    a_front, volume, submerged = 1.5, 6.0, 2.4
    d = cr.default_desc(cr.BOAT, a_front=a_front, volume=volume)
    r = cr.craft_update(d, dict(NO_INPUT, flags=0), dict(LEVEL, lin_vel=(0, 10, 0), submerged=submerged), (-1, -1), (True, 0.0), None, 0, DT)
    assert r["branches"] == cr.BR["DRAG"] and len(r["ops"]) == 1 and r["ops"][0][0] == "force"
    drag = vec(r["ops"][0][1])
    want = -0.5 * 1020 * 100 * 0.1 * a_front * (submerged / volume)
    assert drag[0] == 0 and drag[2] == 0 and abs(drag[1] - want) <= 4e-7 * abs(want), (drag, want)
    # the top drag is 0: the flow is along the deck.  Evaluated alone: straight down, only the top area and the smooth step of the volume count
    r = cr.craft_update(d, dict(NO_INPUT, flags=0), dict(LEVEL, lin_vel=(0, 0, -2), submerged=0.5), (-1, -1), (True, 0.0), None, 0, DT)
    want = 0.5 * 1020 * 4 * 0.75 * 8.0 * (0.5 * 0.5 * (3 - 2 * 0.5))
    assert abs(vec(r["ops"][0][1])[2] - want) <= 4e-7 * want


def test_upside_down_hover_car_unflips_for_a_second():
    d = cr.default_desc(cr.HOVERCAR, mass=500.0)
    flipped = dict(LEVEL, rot=tuple(cs.quat((0, 1, 0), np.pi - 0.2)))      # up.z = cos(pi - 0.2) = -0.98 < -0.9
    r = cr.craft_update(d, NO_INPUT, flipped, (-1, -1), NO_WATER, None, 0, DT)
    assert r["unflip"] == F(1) and not r["branches"] & (cr.BR["HOVER"] | cr.BR["UNFLIP"])
    r = cr.craft_update(d, NO_INPUT, flipped, (r["unflip"], -1), NO_WATER, None, 1, DT)
    assert r["branches"] & cr.BR["UNFLIP"] and r["unflip"] == F(1) - F(DT)
    up = [op[1] for op in r["ops"] if op[0] == "force"][0]
    assert up[0] == 0 and up[1] == 0 and up[2] == F(500.0) * F(9.81)
    # on its side (up.z = cos(1.45) = 0.12 <= 0.2) the force stays on; past 0.2 it ends
    r = cr.craft_update(d, NO_INPUT, dict(LEVEL, rot=tuple(cs.quat((0, 1, 0), 1.45))), (0.5, -1), NO_WATER, None, 2, DT)
    assert r["branches"] & cr.BR["UNFLIP"] and r["branches"] & cr.BR["HOVER"] and r["unflip"] == F(0.5) - F(DT)
    r = cr.craft_update(d, NO_INPUT, dict(LEVEL, rot=tuple(cs.quat((0, 1, 0), 1.3))), (0.5, -1), NO_WATER, None, 3, DT)      # cos(1.3) = 0.27
    assert not r["branches"] & cr.BR["UNFLIP"] and r["unflip"] == F(-1)
    # without a driver nothing happens at all
    r = cr.craft_update(d, dict(NO_INPUT, flags=0), flipped, (-1, -1), NO_WATER, None, 0, DT)
    assert not r["ops"] and r["branches"] == 0 and r["unflip"] == F(-1)


def test_righting_counts_down_from_two_seconds():
    d = cr.default_desc(cr.BOAT, mass=2000.0)
    capsized = dict(LEVEL, rot=tuple(cs.quat((0, 1, 0), 3.0)))
    t, n = F(2.0), 0
    while t > 0:
        r = cr.craft_update(d, dict(NO_INPUT, flags=0), capsized, (-1, t), NO_WATER, None, n, DT)
        assert r["branches"] == cr.BR["RIGHTING"] and r["righting"] == t - F(DT) and [op[0] for op in r["ops"]] == ["torque"]
        t, n = r["righting"], n + 1
    assert n == 120 or n == 121
    tq = vec(r["ops"][0][1])
    assert abs(tq[1]) > 1000.0 and abs(tq[0]) < 1e-2 * abs(tq[1])      # about the axis the boat is rolled around, towards upright
    r = cr.craft_update(d, dict(NO_INPUT, flags=0), capsized, (-1, t), NO_WATER, None, n, DT)
    assert r["branches"] == 0 and not r["ops"] and r["righting"] == t
    # entering the driver seat cancels it: the library sets the timer to -1 when SGP_CRAFT_IN_DRIVER appears (sgp_crafts_set_inputs); from then on nothing
    r = cr.craft_update(d, NO_INPUT, capsized, (-1, -1), NO_WATER, None, 0, DT)
    assert not r["branches"] & cr.BR["RIGHTING"] and r["righting"] == F(-1)


def test_generator_values_worked_by_hand():
    """h0 = seed ^ update * 0x9E3779B9 ^ draw * 0x85EBCA6B; h ^= h >> 16; h *= 0x7FEB352D; h ^= h >> 15; h *= 0x846CA68B; h ^= h >> 16; u = (h >> 8) / 2^24.
    (1, 0, 0): 0x1, 0x1, 0x7FEB352D, 0x7FEBCAFB, 0x6889F849, 0x688990C0 -> 0x688990 / 2^24
    (0x12345678, 3, 7): 0x61E0B3BE, 0x61E0D25E, 0x7E5C7086, 0x7E5C8C3E, 0xC15859AA, 0xC15898F2 -> 0xC15898 / 2^24
    (0xDEADBEEF, 100, 23): 0x1B291D36, 0x1B29061F, 0x43EF7E73, 0x43EFF9AD, 0x082EBEEF, 0x082EB6C1 -> 0x082EB6 / 2^24"""
    assert cr.craft_rand(0, 0, 0) == 0.0
    assert cr.craft_rand(1, 0, 0) == 0x688990 / 2.0 ** 24 == 0.40834903717041016
    assert cr.craft_rand(0x12345678, 3, 7) == 0xC15898 / 2.0 ** 24 == 0.7552580833435059
    assert cr.craft_rand(0xDEADBEEF, 100, 23) == 0x082EB6 / 2.0 ** 24 == 0.03196275234222412
    assert all(0.0 <= cr.craft_rand(9, u, k) < 1.0 and F(cr.craft_rand(9, u, k)) == cr.craft_rand(9, u, k) for u in range(8) for k in range(66))


def test_emission_order_kinds_and_tags():
    d = cr.default_desc(cr.BOAT, craft=5, splash=[(-1, 2, -0.3, -1), (1, 2, -0.3, 1)], prop_os=(0, -3, -0.3))
    body = dict(LEVEL, pos=(0, 0, 0), lin_vel=(0, 8, 0), submerged=2.0)
    r = cr.craft_update(d, dict(NO_INPUT, forward=1.0), body, (-1, -1), (True, 0.0), None, 4, DT, counter=10)
    assert [p["kind"] for p in r["particles"]] == [cr.PK_JET] * 6 + [cr.PK_SPLASH] * 4
    assert [p["tag"] for p in r["particles"]] == [(5 << 32) | (p["kind"] << 28) | (10 + i) for i, p in enumerate(r["particles"])]
    assert r["counter"] == 20 and r["branches"] & (cr.BR["SPLASH0"] | cr.BR["SPLASH0"] << 1) == cr.BR["SPLASH0"] * 3
    # water disabled: every "below the water level" test is false
    r = cr.craft_update(d, dict(NO_INPUT, forward=1.0), body, (-1, -1), NO_WATER, None, 4, DT)
    assert not r["particles"] and not r["branches"] & cr.BR["THRUST"]
    # a hover car: four spray particles over water, one dust particle over ground
    h = cr.default_desc(cr.HOVERCAR, craft=2, trace_os=(0, 0, -0.5))
    r = cr.craft_update(h, NO_INPUT, LEVEL, (-1, -1), (True, 0.0), lambda o, dd: (None, 0.0), 0, DT)
    assert [p["kind"] for p in r["particles"]] == [cr.PK_SPRAY] * 4 and r["branches"] & cr.BR["RAY_WATER"] and all(p["flags"] == cr.DIE_ON_HIT for p in r["particles"])
    r = cr.craft_update(h, NO_INPUT, LEVEL, (-1, -1), (True, 0.0), lambda o, dd: (7, 2.0), 0, DT)
    assert [p["kind"] for p in r["particles"]] == [cr.PK_DUST] and r["branches"] & cr.BR["RAY_BODY"] and r["particles"][0]["flags"] == 0 and r["trace_body"] == 7


def test_float64_switch_runs_the_same_formulas():
    descs, table = cs.parity_table()
    worst = 0.0
    for k in range(0, len(descs), 7):
        e = table[3][k]
        body = dict(pos=e["pos"], rot=e["rot"], lin_vel=e["lin_vel"], ang_vel=e["ang_vel"], submerged=1.0)
        a = cr.craft_update(descs[k], dict(e["inp"], flags=cr.IN_DRIVER), body, (0.5, 0.5), (True, cs.WATER_Z), None, 3, DT)
        b = cr.craft_update(descs[k], dict(e["inp"], flags=cr.IN_DRIVER), body, (0.5, 0.5), (True, cs.WATER_Z), None, 3, DT, dtype=np.float64)
        assert a["branches"] == b["branches"] and a["force"][0].dtype == np.float32 and b["force"][0].dtype == np.float64
        if b["force_scale"] > 0:
            worst = max(worst, float(np.abs(vec(a["force"]) - vec(b["force"])).max()) / b["force_scale"])
    assert 0.0 < worst < 1.0e-5


def test_twin_horizon_survives_one_ulp_of_the_transcendentals(oracle):
    """The horizon of the free-running twin test (tests/test_crafts_gpu.py: 30 updates): the restatement drives the twin scene over the CPU oracle twice, as it is
    and with every acos / atan2 / sin / cos result moved by one ulp in a seeded direction.  What that moves the bodies by at the horizon must stay within a
    quarter of the parity tolerance (1e-4 m, 1e-3 m/s), or the device's own transcendental functions could fail the twin test on their own."""
    horizon = 30
    runs = []
    for seed in (None, 77):
        w = oracle.OracleWorld(max_bodies=64)
        _, hist = cs.run_twin_reference(w, horizon, trans_seed=seed)
        runs.append(hist)
        w.close()
    drift = {f: max(float(np.abs(a[f] - b[f]).max()) for a, b in zip(*runs)) for f in ("pos", "rot", "lin_vel", "ang_vel")}
    print(f"drift after {horizon} updates with the transcendentals moved by one ulp: {drift}")
    assert float(np.abs(runs[0][-1]["pos"] - runs[0][0]["pos"]).max()) > 0.05      # (the crafts moved)
    assert drift["pos"] <= 0.25e-4 and drift["rot"] <= 0.25e-4 and drift["lin_vel"] <= 0.25e-3 and drift["ang_vel"] <= 0.25e-3


def test_branch_margins_of_the_parity_table():
    """In float64 every pose-dependent branch condition of the seeded table (the 25 degree lift threshold, up.z against 0 / 0.2 / -0.9, v_mag against 1e-3 and 5,
    the propeller and splash points against the water level, the -0.5 dot test) is at least 1e-4 (relative) away from its threshold, with the timers running or not."""
    descs, table = cs.parity_table()
    assert len(descs) == 65 and len(table) == 20
    worst, names = np.inf, set()
    for u, row in enumerate(table):
        for k, e in enumerate(row):
            body = dict(pos=e["pos"], rot=e["rot"], lin_vel=e["lin_vel"], ang_vel=e["ang_vel"], submerged=1.0)
            for timers in ((-1.0, -1.0), (0.5, 0.5)):
                r = cr.craft_update(descs[k], e["inp"], body, timers, (True, cs.WATER_Z), None, u, DT, dtype=np.float64)
                worst = min(worst, cr.min_margin(r, ("pose",)))
                names |= {n.split(" 25")[0] for kk, n, _ in r["margins"] if kk == "pose"}
    print(f"smallest pose margin of the table: {worst:.3e}")
    assert worst >= 1.0e-4
    for n in ("up.z > 0", "up.z > 0.2", "up.z < -0.9", "v_mag > 1e-3", "v_mag > 5", "propellor under water", "top lift", "right lift"):
        assert n in names, n
    assert any(n.startswith("splash") and n.endswith("dot > -0.5") for n in names) and any(n.endswith("under water") and n.startswith("splash") for n in names)
