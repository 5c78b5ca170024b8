"""The batched hover cars and boats on the device (sgp_crafts_*) against the numpy restatement of tests/craft_reference.py (written from docs/CONTRACT.md,
"Crafts"), which is fed by the bodies' states as the world reports them and by CWorld.raycast on the same world, and never reads what the craft kernels wrote.

Discrete results (branch words, timers, emission counts, kinds, tags) must be EQUAL; forces and torques are held against the float64 evaluation of the same
formulas, with the float32 restatement's own error as the yardstick; body states of free-running twins within the project's parity tolerance
(tests/test_parity_gpu.py:16-17)."""
import json
import subprocess

import numpy as np
import pytest

from substrata_amd import abi
import craft_reference as cr
import craft_scenes as cs

pytestmark = pytest.mark.gpu

POS_TOL, VEL_TOL = 1.0e-4, 1.0e-3          # tests/test_parity_gpu.py:16-17
DT = cs.DT
TWIN_HORIZON = 30
STATE_FIELDS = ("pos", "rot", "lin_vel", "ang_vel")


def new_world(**kw):
    from substrata_amd.lib import World
    return World(**kw)


def to_abi(crafts, d, body):
    a = crafts.default_desc(d["kind"], body)
    a.mass, a.seed, a.tag = d["mass"], d["seed"], 1000 + d["craft"]
    a.model_to_y_forwards_rot_1[:] = [float(x) for x in d["q1"]]
    a.model_to_y_forwards_rot_2[:] = [float(x) for x in d["q2"]]
    a.trace_origin_os[:] = d["trace_os"]
    a.thrust_force, a.propellor_sideways_offset, a.rudder_deflection_force_factor = d["thrust"], d["prop_off"], d["rudder"]
    a.propellor_point_os[:] = d["prop_os"]
    a.thrust_vector_lateral_amount, a.jet_particle_initial_width = d["lateral"], d["jet_w"]
    a.front_cross_sectional_area, a.side_cross_sectional_area, a.top_cross_sectional_area = d["a_front"], d["a_side"], d["a_top"]
    a.n_splash_points = len(d["splash"])
    for p, sp in enumerate(d["splash"]):
        a.splash_points[4 * p:4 * p + 4] = sp
    return a


def inputs_array(inps):
    a = np.zeros(len(inps), dtype=abi.craft_input_dtype)
    for i, e in enumerate(inps):
        a[i] = (e["forward"], e["right"], e["up"], e["hand_brake"], e["flags"])
    return a


def raycast(w, rays):
    """CWorld.raycast through the batched kernel (a single ray would go to the resident ray server)."""
    if len(rays) == 0:
        return np.zeros(0, dtype=abi.hit_dtype)
    if len(rays) == 1:
        return w.raycast(np.concatenate([rays, rays]))[:1]
    return w.raycast(rays)


def vec(v):
    return np.array([float(x) for x in v])


def bits_equal(a, b):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32) == np.ascontiguousarray(b, dtype=np.float32).view(np.uint32)


def restate(w, descs, inps, st, timers, counters, u):
    """The restatement of one update of every craft, in float32 and float64, over the body states `st` and CWorld.raycast on `w`."""
    n = len(descs)
    bodies = [dict(pos=st["pos"][i], rot=st["rot"][i], lin_vel=st["lin_vel"][i], ang_vel=st["ang_vel"][i], submerged=st["submerged_volume"][i]) for i in range(n)]
    casting = [i for i in range(n) if descs[i]["kind"] == cr.HOVERCAR and inps[i]["flags"] & cr.IN_DRIVER]
    rays = np.zeros(len(casting), dtype=abi.ray_dtype)
    for j, i in enumerate(casting):      # a first pass without a ray oracle: where the ray starts and where it points
        r = cr.craft_update(descs[i], inps[i], bodies[i], timers[i], (True, cs.WATER_Z), None, u, DT, counter=counters[i])
        rays[j] = (tuple(r["trace_origin"]), tuple(r["trace_dir"]), cr.MAX_TRACE_DIST, abi.INVALID_ID, 0)
    hits = raycast(w, rays)
    oracle = {i: (lambda o, d, h=hits[j]: ((int(h["id"]), h["t"]) if h["id"] != abi.INVALID_ID else (None, 0.0))) for j, i in enumerate(casting)}
    out32 = [cr.craft_update(descs[i], inps[i], bodies[i], timers[i], (True, cs.WATER_Z), oracle.get(i), u, DT, counter=counters[i]) for i in range(n)]
    out64 = [cr.craft_update(descs[i], inps[i], bodies[i], timers[i], (True, cs.WATER_Z), oracle.get(i), u, DT, counter=counters[i], dtype=np.float64) for i in range(n)]
    return out32, out64


def check_particles(read, results, skip):
    """The batch's new particles against the restatement's: order, tags, flags, pos, vel, width.  Returns (values compared, bit-equal)."""
    want = [(i, p) for i, r in enumerate(results) for p in r["particles"]]
    if skip:      # (a craft left out of the discrete comparison: only the others' particles are held, by tag)
        keep = [k for k, (i, _) in enumerate(want) if i not in skip]
        read = read[[k for k in range(len(read)) if (int(read["tag"][k]) >> 32) not in skip]]
        want = [want[k] for k in keep]
    assert len(read) == len(want), (len(read), len(want))
    total = equal = 0
    for got, (i, p) in zip(read, want):
        assert int(got["tag"]) == p["tag"] and int(got["flags"]) == p["flags"], (i, hex(int(got["tag"])), hex(p["tag"]))
        assert float(np.abs(got["pos"] - vec(p["pos"])).max()) <= POS_TOL and float(np.abs(got["vel"] - vec(p["vel"])).max()) <= VEL_TOL, (i, got, p)
        assert abs(float(got["width"]) - float(p["width"])) <= POS_TOL and abs(float(got["opacity"]) - float(p["opacity"])) <= POS_TOL
        eq = np.concatenate([bits_equal(got["pos"], np.float32(vec(p["pos"]))), bits_equal(got["vel"], np.float32(vec(p["vel"]))), bits_equal([got["width"]], [p["width"]])])
        total += eq.size
        equal += int(eq.sum())
    return total, equal


def run_parity(n, updates):
    descs, table = cs.parity_table()
    descs = descs[:n]
    w = new_world(max_bodies=256)
    w.set_water(True, cs.WATER_Z)
    cs.add_ground_box(w, n)
    bodies = [cs.add_craft_body(w, d["kind"], cs.home(k)) for k, d in enumerate(descs)]
    crafts = w.crafts(n)
    ps = w.particles(n * abi.CRAFT_MAX_EMIT, event_capacity=64)
    crafts.attach(ps)
    for k, d in enumerate(descs):
        assert crafts.add(to_abi(crafts, d, bodies[k])) == k
    timers = [[-1.0, -1.0] for _ in range(n)]
    counters = [0] * n
    prev_flags = [0] * n
    tainted = set()
    compared = left_out = 0
    err_dev = err_f32 = 0.0
    seen = 0
    p_total = p_equal = 0
    for u in range(updates):
        row = table[u][:n]
        recs = np.zeros(n, dtype=abi.pose_vel_dtype)
        for k, e in enumerate(row):
            recs[k] = (e["pos"], e["rot"], e["lin_vel"], e["ang_vel"])
        w.set_pose_vel_batch(bodies, recs)                                   # 1. every body's pose and velocity from the table
        inps = [e["inp"] for e in row]
        crafts.set_inputs(0, inputs_array(inps))
        started = [k for k in range(n) if cs.righting_started(k, u)]
        crafts.start_righting(started)
        for k in range(n):      # what those two calls mean for a boat's righting timer (include/sgp.h)
            if descs[k]["kind"] == cr.BOAT and inps[k]["flags"] & cr.IN_DRIVER and not prev_flags[k] & cr.IN_DRIVER:
                timers[k][1] = -1.0
            if k in started:
                timers[k][1] = 2.0
            prev_flags[k] = inps[k]["flags"]
        st = w.get_state(bodies)                                             # 2. the body states
        assert np.array_equal(st["pos"], recs["pos"]) and np.array_equal(st["lin_vel"], recs["lin_vel"])
        ps.clear()
        crafts.update(DT)                                                    # 3.
        got = crafts.states(0, n)                                            # 4.
        out32, out64 = restate(w, descs, inps, st, timers, counters, u)      # 5.
        for k in range(n):
            if cr.min_margin(out64[k], ("dyn",)) < 1.0e-4:
                tainted.add(k)
            if k in tainted:
                left_out += 1
                continue
            compared += 1
            a, g = out32[k], got[k]
            assert int(g["status"]) == 0 and int(g["update_index"]) == u + 1
            assert int(g["branches"]) == a["branches"] == out64[k]["branches"], (u, k, hex(int(g["branches"])), hex(a["branches"]))
            assert bits_equal([g["unflip_time_remaining"], g["righting_time_remaining"]], [a["unflip"], a["righting"]]).all(), (u, k, g, a["unflip"], a["righting"])
            assert int(g["n_emitted"]) == len(a["particles"]), (u, k)
            assert int(g["trace_body"]) == (abi.INVALID_ID if a["trace_body"] is None else a["trace_body"]), (u, k)
            seen |= a["branches"]
            timers[k], counters[k] = [float(a["unflip"]), float(a["righting"])], a["counter"]
            b = out64[k]
            for name, scale in (("force", b["force_scale"]), ("torque", b["torque_scale"])):
                if scale > 0.0:
                    err_dev = max(err_dev, float(np.abs(g[name].astype(np.float64) - vec(b[name])).max()) / scale)
                    err_f32 = max(err_f32, float(np.abs(vec(a[name]) - vec(b[name])).max()) / scale)
                else:
                    assert not np.any(g[name])
        t, e = check_particles(ps.read(), out32, tainted)
        p_total, p_equal = p_total + t, p_equal + e
        w.step(DT)                                                           # 6.
    share = left_out / float(compared + left_out)
    print(f"crafts {n}: {compared} craft-updates compared, {left_out} left out ({100 * share:.2f} %); force / torque error against float64, normalised: "
          f"device {err_dev:.3e}, float32 restatement {err_f32:.3e}; particle values bit-equal {p_equal} of {p_total}")
    assert share <= 0.02
    assert err_dev <= 4.0 * err_f32, (err_dev, err_f32)
    crafts.close(); ps.close(); w.close()
    return seen


def test_per_update_parity_65_crafts():
    seen = run_parity(65, 20)
    for name in ("HOVER", "UNFLIP", "DRAG", "LIFT_TOP", "LIFT_BOTTOM", "LIFT_RIGHT", "LIFT_LEFT", "THRUST", "RUDDER", "RIGHTING", "RAY_BODY", "RAY_WATER", "ACTIVATE", "SPLASH0"):
        assert seen & cr.BR[name], name


@pytest.mark.parametrize("n", [1, 64])
def test_per_update_parity_other_sizes(n):
    run_parity(n, 6)


def make_twin_batch(w, attach=None, capacity=4):
    descs, poses, inputs, righting = cs.twin_scene()
    w.set_water(True, cs.WATER_Z)
    cs.add_ground_box(w, 8)
    bodies = [cs.add_craft_body(w, d["kind"], p, r) for d, (p, r) in zip(descs, poses)]
    crafts = w.crafts(capacity)
    if attach is not None:
        crafts.attach(attach)
    for i, d in enumerate(descs):
        assert crafts.add(to_abi(crafts, d, bodies[i])) == i
    crafts.set_inputs(0, inputs_array(inputs))
    crafts.start_righting(righting)
    return bodies, crafts


def test_twin_worlds_free_running():
    a, b = new_world(max_bodies=64), new_world(max_bodies=64)
    bodies, crafts = make_twin_batch(a)
    hist_a = []
    for u in range(TWIN_HORIZON):
        crafts.update(DT)
        a.step(DT)
        hist_a.append(a.get_state(bodies).copy())
    bodies_b, hist_b = cs.run_twin_reference(b, TWIN_HORIZON)
    assert list(bodies_b) == list(bodies)
    total = equal = 0
    worst = dict.fromkeys(STATE_FIELDS, 0.0)
    for sa, sb in zip(hist_a, hist_b):
        for f in STATE_FIELDS:
            worst[f] = max(worst[f], float(np.abs(sa[f] - sb[f]).max()))
            eq = bits_equal(sa[f], sb[f])
            total, equal = total + eq.size, equal + int(eq.sum())
    print(f"twin worlds, {TWIN_HORIZON} updates: worst differences {worst}; bit-equal {equal} of {total} ({100.0 * equal / total:.1f} %)")
    st = crafts.states(0, 4)
    assert st["branches"][0] & cr.BR["RAY_BODY"] and st["branches"][1] & cr.BR["RAY_WATER"] and st["branches"][2] & cr.BR["THRUST"] and st["branches"][3] & cr.BR["RIGHTING"]
    assert np.abs(hist_a[-1]["pos"] - hist_a[0]["pos"]).max() > 0.05      # (they moved)
    assert worst["pos"] <= POS_TOL and worst["rot"] <= POS_TOL and worst["lin_vel"] <= VEL_TOL and worst["ang_vel"] <= VEL_TOL, worst
    crafts.close(); a.close(); b.close()


def test_emission_into_a_full_batch_and_detached():
    w = new_world(max_bodies=64)
    ps = w.particles(4 * abi.CRAFT_MAX_EMIT, event_capacity=256)
    bodies, crafts = make_twin_batch(w, attach=ps)
    descs, _, inputs, righting = cs.twin_scene()
    # fill the batch to the brim with particles that stay (no update of the particle batch in this test)
    filler = ps.defaults(ps.capacity)
    filler["tag"] = 7000 + np.arange(ps.capacity)
    filler["pos"][:, 0] = np.arange(ps.capacity)
    ps.add(filler)
    assert len(ps.read()) == ps.capacity and len(ps.drain_events()[0]) == 0
    st = w.get_state(bodies)
    crafts.update(DT)
    got = crafts.states(0, 4)
    timers = [[-1.0, 2.0 if i in righting else -1.0] for i in range(4)]
    out32, _ = restate(w, descs, inputs, st, timers, [0] * 4, 0)
    new = [p for r in out32 for p in r["particles"]]
    assert [int(g) for g in got["n_emitted"]] == [len(r["particles"]) for r in out32] and len(new) >= 1 + 4 + 6
    # what sgp_particles_add of the same records would have raised: newcomer j replaces slot j (the cursor starts at 0) and reports the filler that was there
    ev, dropped = ps.drain_events()
    assert dropped == 0 and len(ev) == len(new)
    assert [int(t) for t in ev["tag"]] == [7000 + j for j in range(len(new))] and np.all(ev["kind"] == abi.PARTICLE_EV_REPLACED)
    assert np.array_equal(ev["pos"][:, 0], np.arange(len(new), dtype=np.float32))
    live = ps.read()
    assert len(live) == ps.capacity and [int(t) for t in live["tag"][:len(new)]] == [p["tag"] for p in new] and int(live["tag"][len(new)]) == 7000 + len(new)
    # ... and a twin batch fed through sgp_particles_add says the same
    twin = w.particles(ps.capacity, event_capacity=256)
    twin.add(filler)
    recs = twin.defaults(len(new))
    for j, p in enumerate(new):
        recs[j] = (vec(p["pos"]), vec(p["vel"]), p["area"], p["mass"], p["restitution"], p["width"], p["dwidth_dt"], p["opacity"], p["dopacity_dt"], p["flags"], p["tag"])
    twin.add(recs)
    ev2, _ = twin.drain_events()
    assert np.array_equal(ev2["tag"], ev["tag"]) and np.array_equal(ev2["kind"], ev["kind"]) and np.array_equal(ev2["pos"], ev["pos"])
    assert np.array_equal(twin.read()["tag"], live["tag"])
    # detached: nothing is appended, n_emitted still counts
    crafts.attach(None)
    w.step(DT)
    crafts.update(DT)
    assert crafts.states(0, 4)["n_emitted"].sum() > 0
    assert np.array_equal(ps.read()["tag"], live["tag"]) and len(ps.drain_events()[0]) == 0
    # a batch that is too small, or of another world, is refused
    from substrata_amd.world import SgpError
    small = w.particles(4 * abi.CRAFT_MAX_EMIT - 1)
    other = new_world(max_bodies=16)
    foreign = other.particles(4 * abi.CRAFT_MAX_EMIT)
    for bad in (small, foreign):
        with pytest.raises(SgpError):
            crafts.attach(bad)
    for x in (crafts, small, foreign, twin, ps, other, w):
        x.close()


def test_no_wait_gives_the_same_states():
    finals = []
    for read_back in (False, True):
        w = new_world(max_bodies=64)
        ps = w.particles(4 * abi.CRAFT_MAX_EMIT)
        bodies, crafts = make_twin_batch(w, attach=ps)
        for u in range(12):
            crafts.update(DT)
            if read_back:
                crafts.states(0, 4); ps.read()
            ps.update(DT)
            w.step(DT)
            if read_back:
                w.get_state(bodies)
        finals.append((w.get_state(bodies).copy(), crafts.states(0, 4).copy(), ps.read().copy()))
        crafts.close(); ps.close(); w.close()
    for x, y in zip(finals[0], finals[1]):
        assert x.tobytes() == y.tobytes()
    assert len(finals[0][2]) > 0


def falling_boxes(w):
    from helpers import add_ground, dyn
    add_ground(w)
    return [dyn(w, pos=(2.0 * i, 0.3 * i, 1.0 + 0.7 * i), rot=cs.quat((1, 2, 3), 0.3 * i), allow_sleeping=1) for i in range(6)]


def test_a_world_whose_crafts_do_nothing_steps_as_without_them():
    runs = []
    for mode in ("none", "empty", "idle"):
        w = new_world(max_bodies=64)
        boxes = falling_boxes(w)
        ids = list(boxes)
        # (the bodies the idle crafts ride on exist in every variant: only the batch differs)
        ids += [cs.add_craft_body(w, k % 2, (40.0 + 8 * k, 0.0, 5.0), gravity_factor=0.0) for k in range(3)]
        crafts = None
        if mode != "none":
            crafts = w.crafts(8)
        if mode == "idle":      # no driver, zero velocity, no righting
            for k in range(3):
                crafts.add(to_abi(crafts, cs.craft_desc(k, 5), ids[len(boxes) + k]))
        states = []
        for s in range(60):
            if crafts is not None:
                crafts.update(DT)
            w.step(DT)
            states.append(w.get_state(ids).tobytes())
        if mode == "idle":
            st = crafts.states(0, 3)
            assert not st["branches"].any() and not st["force"].any() and not st["torque"].any() and np.all(st["update_index"] == 60)
        runs.append(states)
        if crafts is not None:
            crafts.close()
        w.close()
    assert runs[0] == runs[1] and runs[0] == runs[2]


def test_body_gone_is_reported_and_its_slot_left_alone():
    from helpers import dyn
    from substrata_amd.world import SgpError
    worlds = [new_world(max_bodies=64), new_world(max_bodies=64)]
    newcomers = []
    for which, w in enumerate(worlds):
        falling_boxes(w)
        body = cs.add_craft_body(w, cr.HOVERCAR, (30.0, 0.0, 5.0))
        if which == 0:
            crafts = w.crafts(4)
            d = cs.craft_desc(0, 5)
            cid = crafts.add(to_abi(crafts, d, body))
            with pytest.raises(SgpError):      # a second craft on the same body
                crafts.add(to_abi(crafts, d, body))
            crafts.set_inputs(0, inputs_array([dict(forward=1.0, right=1.0, up=1.0, hand_brake=0.0, flags=cr.IN_DRIVER)]))
            crafts.update(DT)
        w.step(DT)
        if which == 0:
            assert crafts.states(0, 1)["force"][0][2] > 0 and crafts.states(0, 1)["status"][0] == 0
        w.remove(body)
        new = dyn(w, pos=(30.0, 0.0, 6.0), mass=10.0)
        assert new == body      # the newcomer takes the slot
        newcomers.append(new)
        for s in range(3):
            if which == 0:
                crafts.update(DT)
            w.step(DT)
    st = crafts.states(0, 1)[0]
    assert st["status"] == abi.CRAFT_ST_BODY_GONE and not st["force"].any() and not st["torque"].any() and st["branches"] == 0 and st["n_emitted"] == 0
    a, b = worlds[0].get_state(newcomers[:1]), worlds[1].get_state(newcomers[1:])
    assert a.tobytes() == b.tobytes()
    # the body is free for another craft
    assert crafts.add(to_abi(crafts, cs.craft_desc(2, 5), newcomers[0])) == 1
    crafts.close()
    for w in worlds:
        w.close()


def test_caller_program_agrees_with_its_host_loop(tmp_path):
    from test_facade_gpu import build_facade_exe
    exe = build_facade_exe(tmp_path, "crafts_batch.cpp")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    out = json.loads(r.stdout.strip().splitlines()[-1])
    print(out)
    assert out["crafts"] == 4 and out["updates"] >= 10 and out["moved"] > 0.05
    assert out["max_pos_diff"] <= POS_TOL and out["max_rot_diff"] <= POS_TOL and out["max_vel_diff"] <= VEL_TOL
    assert out["particles_batch"] == out["particles_host"] > 0
