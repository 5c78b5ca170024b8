"""The batched path and move-to controllers on the device (sgp_movers_*) against the numpy restatement of tests/mover_reference.py (written from
docs/CONTRACT.md 4j), which is fed the library's prepared segments and the bodies' poses as the world reports them, and never reads what the mover kernels wrote.

Everything discrete and every state value (waypoint index, distances, clocks, status bits, update index) must be EQUAL to the float32 restatement; targets and
the bodies' velocities are held against the float64 evaluation of the same formulas from the float32 state of the same update, with the float32 restatement's own
error as the yardstick."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

from substrata_amd import abi, build, scenes
import mover_reference as mr
import mover_scenes as ms

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
DT = 1.0 / 60.0
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOG = os.environ.get("SGP_MOVERS_LOG")      # where test_twin_worlds also writes what it measured (profiles/movers_cost.log was assembled from it)
SEEN = set()
# every branch the table must reach (tests/mover_scenes.py), by the names the restatement gives them
BRANCHES = {"entry", "arc", "exit", "equal_dirs", "curve_out", "station", "paused", "no_end", "one_end", "several_ends", "overrun", "back_0", "back_1", "back_many",
            "back_overrun", "ease_0", "ease_1", "track_done", "elapsed_beyond_duration", "slerp_neg", "moveto_finished"}


def new_world(**kw):
    from substrata_amd.lib import World
    return World(**kw)


@pytest.fixture(scope="module")
def paths():
    """name -> (waypoint array, the library's prepared segments, its traversal time): sgp_path_prepare needs no device."""
    lib = C.CDLL(build.build())
    abi.bind(lib, "sgp_")
    out = {}
    for name, wps in ms.PATHS.items():
        a = np.zeros(len(wps), dtype=abi.path_waypoint_dtype)
        for k, (pos, typ, pause, speed) in enumerate(wps):
            a[k]["pos"] = pos; a[k]["type"] = typ; a[k]["pause_time"] = pause; a[k]["speed"] = speed
        segs = np.zeros(len(a), dtype=abi.path_segment_dtype)
        total = C.c_double(0.0)
        assert lib.sgp_path_prepare(a.ctypes.data, len(a), segs.ctypes.data, C.byref(total)) == abi.OK
        out[name] = (a, segs, total.value)
    return out


# where the parity bodies start: tilted, so that no target is exactly a half turn away (there the rotation axis has two equally good signs, and the angular
# velocities of two correct implementations differ by 2 pi / dt)
TILT = tuple(float(x) for x in np.float32((0.05, 0.1, 0.15, 0.98)) / np.linalg.norm(np.float32((0.05, 0.1, 0.15, 0.98))))


def kinematic_box(w, pos, half=(1.0, 1.0, 0.2), friction=0.8, rot=(0.0, 0.0, 0.0, 1.0)):
    d = scenes._blank(1)
    d["motion_type"] = abi.MOTION_KINEMATIC; d["layer"] = abi.LAYER_MOVING; d["activate"] = 1; d["friction"] = friction
    d["shape"][0, :3] = half; d["pos"][0] = pos; d["rot"][0] = rot
    return int(w.add_batch(d)[0])


def vec(v):
    return np.array([float(x) for x in v])


def bits(x):
    return np.float32(x).tobytes()


class Rig:
    """A world with one kinematic box per mover of a mix, the batch over it and the restatement next to it."""

    def __init__(self, paths, specs, w=None, home=None, pos_tracks=ms.POS_TRACKS, half=(1.0, 1.0, 0.2), rot=(0.0, 0.0, 0.0, 1.0)):
        self.w = w if w is not None else new_world(max_bodies=max(256, 2 * len(specs) + 16))
        self.movers = self.w.movers(max(len(specs), 1), len(paths))
        self.path_id = {}
        for name, (a, segs, total) in paths.items():
            self.path_id[name] = self.movers.add_path(a)
            got = self.movers.path_segments(self.path_id[name])
            assert got.tobytes() == segs.tobytes()
        self.sim = mr.Sim({name: (segs, total) for name, (a, segs, total) in paths.items()})
        self.extent = {name: max(float(np.linalg.norm(a["pos"] - a["pos"][0], axis=1).max()), 1.0) for name, (a, segs, total) in paths.items()}
        self.specs, self.bodies, self.ids, self.scale, self.pos_tracks = list(specs), [], [], [], pos_tracks
        for k, s in enumerate(specs):
            at = home(k) if home else (3.0 * (k % 8), 3.0 * (k // 8), 50.0)
            self.bodies.append(kinematic_box(self.w, at, half=half, rot=rot))
            self.add(k, s)

    def add(self, k, s):
        if s[0] == "path":
            _, name, t0, leader, follow, flags, base = s
            i = self.movers.add_path_mover(self.bodies[k], self.path_id[name], t0, None if leader is None else self.ids[leader], follow, base, bool(flags & mr.ORIENT_ALONG_PATH), tag=k)
            self.scale.append(self.extent[name])
        else:
            _, pi, ri, hold_pos, hold_rot = s
            i = self.movers.add_moveto_mover(self.bodies[k], hold_pos, hold_rot, tag=k)
            if pi is not None:
                self.movers.set_position_track(i, *self.pos_tracks[pi])
            if ri is not None:
                self.movers.set_rotation_track(i, *ms.ROT_TRACKS[ri])
            self.scale.append(max([1.0] + [float(np.linalg.norm(np.subtract(t[0], t[1]))) for t in ([self.pos_tracks[pi]] if pi is not None else [])]))
        self.ids.append(i)
        assert self.sim.add(s, self.pos_tracks, ms.ROT_TRACKS) == k
        return i

    def close(self):
        self.movers.close()
        self.w.close()


def check_states(rig, got, u):
    """Everything discrete and every state value of every mover against the float32 restatement: equal, none left out."""
    n = 0
    for k, m in enumerate(rig.sim.m):
        g = got[rig.ids[k]]
        want = m["status"]
        if m["kind"] == mr.MOVETO and m["ran"]:
            want |= (mr.ST_POS_ACTIVE if m["pos_track"] and m["pos_track"].active else 0) | (mr.ST_ROT_ACTIVE if m["rot_track"] and m["rot_track"].active else 0)
        if not m["ran"] and m["update_index"] == 0:
            continue      # (never ran: the record of the add)
        assert int(g["status"]) == (want if m["ran"] else 0), (u, k, int(g["status"]), want)
        assert int(g["update_index"]) == m["update_index"], (u, k)
        if m["kind"] == mr.PATH:
            assert int(g["waypoint_index"]) == m["idx"] and bits(g["dist_along_segment"]) == bits(m["dist"]) and bits(g["time_along_segment"]) == bits(m["time"]), (u, k, g, m["idx"], m["dist"], m["time"])
        else:
            for f, t in (("pos_elapsed", m["pos_track"]), ("rot_elapsed", m["rot_track"])):
                assert bits(g[f]) == bits(t.elapsed if t else 0.0), (u, k, f)
        n += 1
    return n


def run_parity(paths, n, updates):
    rig = Rig(paths, ms.mix(n), rot=TILT)
    w, movers = rig.w, rig.movers
    err = {"dev": dict(pos=0.0, rot=0.0, dir=0.0, lin=0.0, ang=0.0), "f32": dict(pos=0.0, rot=0.0, dir=0.0, lin=0.0, ang=0.0)}
    compared = values = equal = 0
    for u in range(updates):
        before = w.get_state(rig.bodies)
        movers.update(DT)
        got = movers.states(0, n)
        after = w.get_state(rig.bodies)                     # velocities as the update left them, before the step
        rig.sim.update(DT, SEEN)
        compared += check_states(rig, got, u)
        t32, t64 = rig.sim.targets(F32, SEEN), rig.sim.targets(F64)
        for k in range(n):
            if t64[k] is None:
                assert np.array_equal(after["lin_vel"][k], before["lin_vel"][k]) and np.array_equal(after["ang_vel"][k], before["ang_vel"][k])      # the body is not touched
                continue
            g, s = got[rig.ids[k]], rig.scale[k]
            pose = (before["pos"][k], before["rot"][k])
            v32 = mr.move_kinematic(tuple(F32(x) for x in pose[0]), tuple(F32(x) for x in pose[1]), t32[k][0], t32[k][1], F32(DT))
            v64 = mr.move_kinematic(tuple(F64(x) for x in pose[0]), tuple(F64(x) for x in pose[1]), t64[k][0], t64[k][1], F64(F32(DT)))
            for name, dev, a, b, norm in (("pos", g["pos"], t32[k][0], t64[k][0], s), ("rot", g["rot"], t32[k][1], t64[k][1], 1.0), ("dir", g["dir"], t32[k][2], t64[k][2], 1.0),
                                          ("lin", after["lin_vel"][k], v32[0], v64[0], s / DT), ("ang", after["ang_vel"][k], v32[1], v64[1], 1.0 / DT)):
                err["dev"][name] = max(err["dev"][name], float(np.abs(dev.astype(F64) - vec(b)).max()) / norm)
                err["f32"][name] = max(err["f32"][name], float(np.abs(vec(a) - vec(b)).max()) / norm)
                eq = np.ascontiguousarray(dev, dtype=F32).view(np.uint32) == np.float32(vec(a)).view(np.uint32)
                values += eq.size
                equal += int(eq.sum())
        w.step(DT)
    rig.close()
    return compared, err, values, equal


@pytest.mark.parametrize("n", [1, 64, 65])
def test_per_update_parity(paths, n):
    updates = 40
    compared, err, values, equal = run_parity(paths, n, updates)
    print("movers parity n=%d: %d mover-updates compared, none left out; bit-equal share of targets and velocities %.1f %% (%d of %d)" % (n, compared, 100.0 * equal / values, equal, values))
    for name in ("pos", "rot", "dir", "lin", "ang"):
        print("  %-3s device error %.3e, float32 restatement %.3e (normalised; the bound is four times the latter)" % (name, err["dev"][name], err["f32"][name]))
    assert compared == updates * n      # none left out: a finished move-to mover is still held against its last record
    for name in ("pos", "rot", "dir", "lin", "ang"):
        assert err["dev"][name] <= 4.0 * err["f32"][name], (name, err)


def test_every_branch_was_seen(paths):
    """Runs after the parity tests of this module (pytest keeps file order): the table reaches every branch it promises."""
    if "overrun" not in SEEN:      # (this test run on its own)
        run_parity(paths, 65, 40)
    assert BRANCHES <= SEEN, sorted(BRANCHES - SEEN)


def test_mesh_body_alias_slots_follow(paths):
    w = new_world(max_bodies=64)
    V = np.array([(-2, -2, 0), (2, -2, 0), (2, 2, 0), (-2, 2, 0)], np.float32)
    T = np.array([(0, 1, 2), (0, 2, 3)], np.uint32)
    info = w.mesh_create(V, T)
    d = scenes._blank(1)
    d["shape_type"] = abi.SHAPE_MESH; d["shape"][0] = 0; d["shape"][0, 0] = float(info.mesh_id); d["pos"][0] = (0, 0, 1)
    d["motion_type"] = abi.MOTION_KINEMATIC; d["layer"] = abi.LAYER_MOVING; d["activate"] = 1
    body = int(w.add_batch(d)[0])
    movers = w.movers(4, 2)
    p = movers.add_path(paths["loop"][0])
    with pytest.raises(Exception):
        movers.add_path_mover(body + 1, p)                   # an alias slot carries no mover
    m = movers.add_path_mover(body, p, 2.0, orient_along_path=True)
    for u in range(5):
        movers.update(DT)
        st = w.read_states(body, 3)
        assert np.any(st["lin_vel"][0] != 0)
        for k in (1, 2):
            assert np.array_equal(st["lin_vel"][k], st["lin_vel"][0]) and np.array_equal(st["ang_vel"][k], st["ang_vel"][0]), (u, k)
        w.step(DT)
        st = w.read_states(body, 3)
        for k in (1, 2):
            assert np.array_equal(st["pos"][k], st["pos"][0]) and np.array_equal(st["rot"][k], st["rot"][0]), (u, k)
    target = movers.states(m, 1)[0]
    assert np.abs(w.read_states(body, 1)[0]["pos"] - target["pos"]).max() < 1e-4      # the body is where the last update sent it
    movers.close(); w.close()


ID_ROT = (0.0, 0.0, 0.0, 1.0)
LIFT_HOME = (30.0, 0.0, 1.0)
LIFT_TRACK = [((LIFT_HOME[0], LIFT_HOME[1], 1.0), (LIFT_HOME[0], LIFT_HOME[1], 2.0), 0.9, mr.EASE_SMOOTHSTEP, 0.0)]      # (6 h / T^2 = 7.4 m/s^2 at most: the box stays down)
TRAIN = [("path", "loop", 1.0, None, 0.0, mr.ORIENT_ALONG_PATH, ID_ROT), ("path", "loop", 0.0, 0, 5.0, mr.ORIENT_ALONG_PATH, ID_ROT),
         ("path", "loop", 0.0, 0, 10.0, mr.ORIENT_ALONG_PATH, ID_ROT), ("moveto", 0, None, LIFT_HOME, ID_ROT)]
HALF = (2.0, 2.0, 0.2)


def twin_world(paths, drive):
    """The train of TRAIN on the loop, a lift, a dynamic box riding each; 60 free-running steps.  drive: "batch", or the dtype of a host loop over move_kinematic."""
    w = new_world(max_bodies=64)
    w.add_batch(scenes.ground())
    # the platforms start where the first update will put them, so that no box is thrown off by a jump
    probe = mr.Sim({name: (segs, total) for name, (a, segs, total) in paths.items()})
    for s in TRAIN:
        probe.add(s, LIFT_TRACK, ms.ROT_TRACKS)
    probe.update(DT)
    start = [vec(t[0]) for t in probe.targets(F32)]
    start[3] = np.array(LIFT_HOME)
    rig = Rig(paths, TRAIN, w=w, home=lambda k: tuple(start[k]), pos_tracks=LIFT_TRACK, half=HALF)
    boxes = scenes.dynamic_bodies(4, mass=10.0, friction=0.9)
    boxes["shape"][:, :3] = 0.25
    boxes["pos"] = np.array([s + (0.0, 0.0, 0.2 + 0.25 + 0.01) for s in start])
    box_ids = [int(i) for i in w.add_batch(boxes)]
    for step in range(60):
        if drive == "batch":
            rig.movers.update(DT)
        else:
            rig.sim.update(DT)
            for k, t in enumerate(rig.sim.targets(drive)):
                if t is not None:
                    w.move_kinematic(rig.bodies[k], [float(F32(x)) for x in t[0]], [float(F32(x)) for x in t[1]], DT)
        w.step(DT)
    st = w.get_state(rig.bodies + box_ids)
    rig.close()
    return st


def test_twin_worlds(paths):
    a, b, b64 = twin_world(paths, "batch"), twin_world(paths, F32), twin_world(paths, F64)
    lines = []
    for f in ("pos", "rot", "lin_vel", "ang_vel"):
        dab = float(np.abs(a[f].astype(F64) - b[f]).max())
        dbb = float(np.abs(b[f].astype(F64) - b64[f]).max())
        size = float(np.abs(b64[f]).max())
        bound = 4.0 * dbb + float(np.spacing(F32(size)))
        lines.append("twin worlds, 60 steps, %-7s |A - B| %.3e  |B - B'| %.3e  bound %.3e" % (f, dab, dbb, bound))
        print(lines[-1])
    if LOG:
        with open(LOG, "a") as fh:
            fh.write("\n".join(lines) + "\n")
    for f in ("pos", "rot", "lin_vel", "ang_vel"):
        dab = float(np.abs(a[f].astype(F64) - b[f]).max())
        dbb = float(np.abs(b[f].astype(F64) - b64[f]).max())
        assert dab <= 4.0 * dbb + float(np.spacing(F32(np.abs(b64[f]).max()))), (f, dab, dbb)
    # the boxes are still on their platforms
    for st in (a, b):
        for k in range(4):
            off = st["pos"][4 + k] - st["pos"][k]
            assert float(np.hypot(off[0], off[1])) < HALF[0] and 0.3 < off[2] < 0.6, (k, off)
    assert a["pos"][3][2] > 1.9      # the lift went up


def test_lifecycle(paths):
    specs = [("path", "loop", 0.5, None, 0.0, 0, (0.0, 0.0, 0.0, 1.0)), ("path", "loop", 0.0, 0, 3.0, 0, (0.0, 0.0, 0.0, 1.0)),
             ("moveto", 2, None, (0, 0, 0), (0.0, 0.0, 0.0, 1.0)), ("path", "two", 0.0, None, 0.0, 0, (0.0, 0.0, 0.0, 1.0))]
    rig = Rig(paths, specs)
    w, movers = rig.w, rig.movers
    with pytest.raises(Exception):
        movers.add_path_mover(rig.bodies[0], rig.path_id["loop"])                             # the body carries a mover already
    with pytest.raises(Exception):
        movers.remove_path(rig.path_id["loop"])                                              # a path in use stays
    spare = kinematic_box(w, (0, 0, 80))
    with pytest.raises(Exception):
        movers.add_path_mover(spare, rig.path_id["loop"], leader=rig.ids[1], follow_dist=1.0)      # a follower cannot lead
    with pytest.raises(Exception):
        movers.add_path_mover(spare, rig.path_id["two"], leader=rig.ids[0], follow_dist=1.0)       # the leader walks another path
    with pytest.raises(Exception):
        movers.update(-1.0)
    movers.update(0.0)                                                                       # no launch: nothing has run
    assert int(movers.states(0, 4)["update_index"].max()) == 0
    movers.update(DT); w.step(DT)
    st = movers.states(0, 4)
    assert [int(x) for x in st["update_index"]] == [1, 1, 1, 1] and not st["status"][:2].any()
    # the move-to mover's track had cur_elapsed > duration: it reached its target at once and is finished -- it no longer writes its body
    assert np.allclose(st["pos"][2], ms.POS_TRACKS[2][1]) and int(st["status"][2]) == 0
    w.set_pose_vel_batch([rig.bodies[2]], np.array([((5, 5, 5), (0, 0, 0, 1), (1, 2, 3), (0, 0, 0))], dtype=abi.pose_vel_dtype))
    movers.update(DT)
    assert tuple(w.get_state([rig.bodies[2]])[0]["lin_vel"]) == (1.0, 2.0, 3.0)
    assert int(movers.states(2, 1)[0]["update_index"]) == 1
    # set_position_track mid-run replaces the track
    movers.set_position_track(rig.ids[2], (5, 5, 5), (5, 5, 9), 1.0, mr.EASE_LINEAR, 0.0)
    movers.update(0.25)
    movers.set_position_track(rig.ids[2], (0, 0, 0), (8, 0, 0), 2.0, mr.EASE_LINEAR, 0.5)
    movers.update(0.5)
    s2 = movers.states(2, 1)[0]
    assert np.allclose(s2["pos"], (4.0, 0, 0), atol=1e-6) and int(s2["status"]) == mr.ST_POS_ACTIVE and float(s2["pos_elapsed"]) == 1.0
    # body removed and its slot re-used: BODY_GONE, and the new body is untouched
    w.remove(rig.bodies[3])
    w.step(DT)
    newcomer = kinematic_box(w, (0, 0, 90))
    assert newcomer == rig.bodies[3]
    movers.update(DT)
    assert int(movers.states(3, 1)[0]["status"]) & mr.ST_BODY_GONE
    ns = w.get_state([newcomer])[0]
    assert not ns["lin_vel"].any() and tuple(ns["pos"]) == (0.0, 0.0, 90.0)
    # leader removed: the follower is at waypoint 0 with LEADER_GONE
    movers.remove(rig.ids[0])
    movers.update(DT)
    f = movers.states(1, 1)[0]
    assert int(f["status"]) == mr.ST_LEADER_GONE and int(f["waypoint_index"]) == 0 and tuple(f["pos"]) == tuple(paths["loop"][0]["pos"][0]) and tuple(f["dir"]) == (1.0, 0.0, 0.0)
    movers.remove(rig.ids[1])
    movers.remove_path(rig.path_id["loop"])                                                  # no longer in use
    rig.close()


def test_updates_without_waits_give_the_same_states(paths):
    specs = ms.mix(16)
    out = []
    for read_back in (True, False):
        rig = Rig(paths, specs)
        for u in range(12):
            rig.movers.update(DT)
            if read_back:
                rig.movers.states(0, 16)
            rig.w.step(DT)
        out.append((rig.movers.states(0, 16).tobytes(), rig.w.get_state(rig.bodies).tobytes()))
        rig.close()
    assert out[0] == out[1]


def test_idle_batch_leaves_the_world_bit_identical(paths):
    """A world whose movers are all finished or removed steps as a world without the batch."""
    finals = []
    for with_batch in (True, False):
        w = new_world(max_bodies=64)
        w.add_batch(scenes.ground())
        plat = kinematic_box(w, (0, 0, 1.0), half=(2.0, 2.0, 0.2))
        other = kinematic_box(w, (10, 0, 1.0))
        d = scenes.dynamic_bodies(6, mass=5.0)
        d["shape"][:, :3] = 0.2
        d["pos"] = [(0.5 * k - 1.2, 0.1 * k, 1.6 + 0.5 * k) for k in range(6)]
        ids = [int(i) for i in w.add_batch(d)]
        movers = None
        if with_batch:
            movers = w.movers(4, 2)
            m0 = movers.add_moveto_mover(plat, (0, 0, 1.0))                                   # never given a track: finished from the start
            m1 = movers.add_path_mover(other, movers.add_path(paths["two"][0]))
            movers.remove(m1)
        for s in range(40):
            if movers:
                movers.update(DT)
            w.step(DT)
        finals.append(w.get_state([plat, other] + ids).tobytes())
        if movers:
            movers.close()
        w.close()
    assert finals[0] == finals[1]


def test_caller_program_agrees_with_its_host_loop(tmp_path):
    from test_facade_gpu import build_facade_exe
    exe = build_facade_exe(tmp_path, "movers_batch.cpp")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    out = json.loads(r.stdout.strip().splitlines()[-1])
    print(out)
    assert out["leader_updates"] == 90 and out["carriage_status"] == 0 and out["moved"] > 1.0
    assert out["max_pos_diff"] <= 1.0e-4 and out["max_vel_diff"] <= 1.0e-3      # the project's parity tolerance (tests/test_parity_gpu.py:16-17)
    assert 2.3 < out["box_z"] < 2.6                                                    # the box rode the lift up
