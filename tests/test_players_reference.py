"""The velocity rule of the driven characters (substrata_amd/csrc/sgp_player_rule.h, compiled for the host by tests/cpp/player_rule_host_check.cpp) against
tests/player_reference.py, an independent numpy float32 restatement of PlayerPhysics::update: a seeded table that crosses supported and not, flying and not,
gravity on and off, the submerged fractions {0, 0.29, 0.3, 0.31, 1}, zero / small / over-cap moves and a jump due and not, plus the edges of every comparison
the rule makes.  Bit equality on every row.  No device."""
import os
import struct
import subprocess

import numpy as np
import pytest

import player_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def bits(x):
    return struct.unpack("<I", struct.pack("<f", float(x)))[0]


def dbits(x):
    return struct.unpack("<Q", struct.pack("<d", float(x)))[0]


def nxt(x, up):
    return np.nextafter(F(x), F(np.inf) if up else F(-np.inf))


def row(vel=(0, 0, 0), move=(0, 0, 0), move_up=0, flags=ref.DRIVE_GRAVITY, supported=0, gv=(0, 0, 0), gn=(0, 0, 1), feet_z=0, water=0, water_z=0, dt=1 / 60, jump_speed=4.5,
        max_air_speed=8, eye_height=1.67, campos=0, cur_time=100.0, last_jump=-1.0, px=1.5, py=-2.5, supported_after=1, dz=0):
    return dict(vel=[F(v) for v in vel], move=[F(v) for v in move], move_up=F(move_up), flags=int(flags), supported=int(supported), gv=[F(v) for v in gv], gn=[F(v) for v in gn],
                feet_z=F(feet_z), water=int(water), water_z=F(water_z), dt=F(dt), jump_speed=F(jump_speed), max_air_speed=F(max_air_speed), eye_height=F(eye_height), campos=F(campos),
                cur_time=float(cur_time), last_jump=float(last_jump), px=F(px), py=F(py), supported_after=int(supported_after), dz=F(dz))


def table():
    rows = []
    rng = np.random.default_rng(20240607)
    u = lambda lo, hi: F(rng.uniform(lo, hi))
    for seed in range(12):
        for supported in (0, 1):
            for fly in (0, 1):
                for gravity in (0, 1):
                    for frac in (0.0, 0.29, 0.3, 0.31, 1.0):
                        for move_kind in range(3):
                            for due in (0, 1):
                                exact = seed == 0      # feet at 0 and an eye height of 1: the fraction is the water level, to the bit
                                feet = F(0) if exact else u(-3, 3)
                                eye = F(1) if exact else F(1.67)
                                water_z = feet + F(frac) * eye
                                move = [(0, 0, 0), (u(-3, 3), u(-3, 3), u(-1, 1)), (u(9, 15), u(-15, -9), u(-2, 2))][move_kind]
                                theta = u(0, 0.6)
                                gn = (np.sin(theta) * np.cos(u(0, 6.28)), np.sin(theta) * np.sin(u(0, 6.28)), np.cos(theta))
                                flags = ref.DRIVE_ON | (ref.DRIVE_FLY if fly else 0) | (ref.DRIVE_GRAVITY if gravity else 0) | (ref.DRIVE_FREE_CAMERA if seed % 5 == 4 else 0)
                                rows.append(row(vel=(u(-6, 6), u(-6, 6), u(-12, 3)), move=move, move_up=u(-3, 3) if seed % 2 else 0, flags=flags, supported=supported,
                                                gv=(u(-1, 1), u(-1, 1), u(-0.5, 0.5)) if seed % 3 else (0, 0, 0), gn=gn, feet_z=feet, water=int(frac > 0 or seed % 4 == 1), water_z=water_z,
                                                dt=[1 / 60, 1 / 30, 1 / 144, 0.1][seed % 4], eye_height=eye, campos=u(-0.3, 0.3) if seed % 3 == 2 else 0,
                                                cur_time=50.0 + seed, last_jump=50.0 + seed - (0.05 if due else 0.2), px=u(-9, 9), py=u(-9, 9), supported_after=int(rng.integers(0, 2)),
                                                dz=u(-0.4, 0.4) if seed % 3 == 1 else 0))
    # vel.z - ground_vel.z at 0.1 and one float either side (on the ground or not; on_ground alike)
    for z in (nxt(0.1, False), F(0.1), nxt(0.1, True)):
        rows.append(row(vel=(1, 2, z), move=(2, 0, 0), supported=1))
        rows.append(row(vel=(1, 2, z + F(0.25)), move=(2, 0, 0), supported=1, gv=(0.5, 0, 0.25)))
    # the jump age at 0.1f (as a double) and one double either side
    period = float(F(0.1))
    for age in (np.nextafter(period, -np.inf), period, np.nextafter(period, np.inf)):
        rows.append(row(move=(2, 1, 0), supported=1, cur_time=age, last_jump=0.0))
        rows.append(row(move=(2, 1, 0), supported=1, flags=ref.DRIVE_FLY, vel=(1, 0, 0), cur_time=age, last_jump=0.0))
        rows.append(row(move=(2, 1, 0), supported=0, cur_time=age, last_jump=0.0))
    # |move| at 1e-4f when flying
    for m in (nxt(1.0e-4, False), F(1.0e-4), nxt(1.0e-4, True)):
        rows.append(row(vel=(3, 1, -2), move=(m, 0, 0), flags=ref.DRIVE_FLY))
        rows.append(row(vel=(3, 1, -2), move=(0, 0, m), flags=ref.DRIVE_FLY | ref.DRIVE_GRAVITY))
    # vel.z at -100
    for z in (nxt(-100, False), F(-100), nxt(-100, True), F(-120)):
        rows.append(row(vel=(0, 0, z), flags=0))
        rows.append(row(vel=(0, 0, z), flags=ref.DRIVE_GRAVITY))
    # campos_z_delta at 1e-5f: with dt = 0 the decay leaves it as it is
    for c in (nxt(1.0e-5, False), F(1.0e-5), nxt(1.0e-5, True)):
        for sign in (1, -1):
            rows.append(row(campos=sign * c, dt=0.0))
            rows.append(row(campos=sign * c / (F(1) - F(20) * F(1 / 60))))
    # the camera's clamp at +-0.3
    for c, dz in ((0.25, 0.05), (0.25, 0.1), (-0.25, -0.05), (-0.25, -0.1), (0.0, 0.3), (0.0, 0.31)):
        rows.append(row(campos=c, dz=dz, dt=0.0))
    # a -0 in the velocity and in the move: x + 0 * dt
    rows.append(row(vel=(-0.0, -0.0, -0.0), move=(-0.0, -0.0, -0.0), flags=ref.DRIVE_GRAVITY))
    rows.append(row(vel=(-0.0, -0.0, -0.0), move=(-0.0, 0.0, -0.0), flags=0, supported=1))
    rows.append(row(vel=(-0.0, -0.0, -0.0), move=(1, 0, 0), move_up=-2, flags=ref.DRIVE_FLY))
    return rows


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("player_rule") / "player_rule_host_check")
    cmd = ["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-I", os.path.join(ROOT, "substrata_amd", "csrc"),
           os.path.join(ROOT, "tests", "cpp", "player_rule_host_check.cpp"), "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return out


def test_rule_header_matches_the_numpy_restatement_bit_for_bit(exe, tmp_path):
    rows = table()
    assert 2500 < len(rows) < 4000
    path = tmp_path / "table.txt"
    with open(path, "w") as f:
        for r in rows:
            cols = [bits(v) for v in r["vel"] + r["move"]] + [bits(r["move_up"]), r["flags"], r["supported"]] + [bits(v) for v in r["gv"] + r["gn"]]
            cols += [bits(r["feet_z"]), r["water"], bits(r["water_z"]), bits(r["dt"]), bits(r["jump_speed"]), bits(r["max_air_speed"]), bits(r["eye_height"]), bits(r["campos"])]
            cols += [dbits(r["cur_time"]), dbits(r["last_jump"]), bits(r["px"]), bits(r["py"]), r["supported_after"], bits(r["dz"])]
            f.write(" ".join("%x" % c for c in cols) + "\n")
    out = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.strip().split("\n")
    assert len(lines) == len(rows)
    seen = dict(jumped=0, ground_set=0, capped=0, fell_cap=0, fly=0, swam=0, decayed_to_zero=0, clamped=0)
    for i, (r, line) in enumerate(zip(rows, lines)):
        got = line.split()
        due = ref.jump_due(r["cur_time"], r["last_jump"])
        o = ref.update(r["vel"], r["move"], r["move_up"], r["flags"], r["supported"], r["gv"], r["gn"], r["feet_z"], r["water"], r["water_z"], r["dt"], due, r["jump_speed"],
                       r["max_air_speed"], r["eye_height"], r["campos"])
        k = ref.camera([r["px"], r["py"], r["feet_z"]], o["vel"], r["supported_after"], r["gv"], r["dz"], r["eye_height"], o["campos_z_delta"])
        want = ["%x" % bits(v) for v in o["vel"] + o["move"]] + ["%x" % bits(o["fraction_submerged"])]
        want += [str(int(o["on_ground"])), str(int(o["jumped"])), str(int(o["allow_sliding"])), str(int(due)), "%x" % bits(o["campos_z_delta"])]
        want += ["%x" % bits(k["campos_z_delta"])] + ["%x" % bits(v) for v in k["last_xy"] + k["cam_pos"]]
        assert got == want, (i, r, got, want)
        seen["jumped"] += o["jumped"]; seen["fly"] += bool(r["flags"] & ref.DRIVE_FLY); seen["swam"] += bool(o["fraction_submerged"] > F(0.3))
        seen["fell_cap"] += bool(o["vel"][2] == F(-100)); seen["decayed_to_zero"] += bool(r["campos"] != 0 and o["campos_z_delta"] == 0)
        seen["clamped"] += bool(abs(k["campos_z_delta"]) == F(0.3))
        seen["ground_set"] += bool(o["on_ground"]); seen["capped"] += bool(not (r["flags"] & ref.DRIVE_FLY) and ref.length(r["move"]) > r["max_air_speed"] and not o["on_ground"])
    assert all(v > 0 for v in seen.values()), seen      # every branch was taken by some row


def test_the_edges_fall_on_the_side_the_reference_puts_them():
    """The comparisons are strict where the reference's are: 0.1 is not `< 0.1f`, an age of exactly JUMP_PERIOD is no jump, -100 is not capped again, 0.3 is not `< 0.3f`."""
    g = dict(move_up=F(0), flags=ref.DRIVE_GRAVITY, ground_vel=ref.vec(0, 0, 0), ground_normal=ref.vec(0, 0, 1), feet_z=F(0), water_enabled=0, water_z=F(0), dt=F(1 / 60),
             jump_speed=F(4.5), max_air_speed=F(8), eye_height=F(1.67), campos_z_delta=F(0))
    on = lambda z: ref.update(ref.vec(0, 0, z), ref.vec(1, 0, 0), supported=1, due=False, **g)["on_ground"]
    assert on(nxt(0.1, False)) and not on(F(0.1)) and not on(nxt(0.1, True))
    period = float(F(0.1))
    assert ref.jump_due(np.nextafter(period, -np.inf), 0.0) and not ref.jump_due(period, 0.0) and period != 0.1
    assert ref.jump_due(5.0, 4.95) and not ref.jump_due(5.0, 4.8) and not ref.jump_due(5.0, -1.0)
    assert not ref.jump_due(float("inf"), 1.0e300)      # sgp_characters_update's clock: no window is open
    # an idle character on the ground keeps the ground's velocity plus one step of gravity; its jump goes through the ground normal
    o = ref.update(ref.vec(0, 0, 0), ref.vec(3, 0, 0), supported=1, due=True, **{**g, "ground_normal": ref.vec(-0.5, 0, 0.8660254)})
    assert o["jumped"] and not o["on_ground"] and o["vel"][2] > F(4.5) and o["vel"][0] < F(3)
    w = dict(g, water_enabled=1, water_z=F(0.3), eye_height=F(1))
    assert ref.update(ref.vec(0, 0, 0), ref.vec(0, 0, 1), supported=0, due=False, **w)["fraction_submerged"] == F(0.3)
    assert ref.update(ref.vec(0, 0, 0), ref.vec(0, 0, 1), supported=1, due=False, **w)["vel"][2] > 0.5      # 0.3 is not below 0.3: the vertical wish is kept
