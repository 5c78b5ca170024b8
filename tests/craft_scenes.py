"""The seeded scene and table of the craft parity tests (tests/test_crafts_reference.py checks its branch margins on the CPU, tests/test_crafts_gpu.py
runs it on the device) -- a helper, not a test.

parity_table(n, updates, seed): n crafts, hover cars (even) and boats (odd), seats taken and empty, and for every (update, craft) a pose, velocities and
an input.  Hover cars with id % 4 == 0 fly over a ground box (top at z = 1), those with id % 4 == 2 over open water (level 0.5); boats float around the
water level.  Poses include flipped cars and capsized boats.  Every entry was drawn until the float64 evaluation of the restatement keeps every
pose-dependent branch condition at least 1e-3 (relative) from its threshold, with either state of the timers -- ten times what the tests require."""
import functools

import numpy as np

import craft_reference as cr

WATER_Z = 0.5
GROUND_TOP = 1.0
SPACING = 8.0
DT = 1.0 / 60.0
HOVER_SHAPE, BOAT_SHAPE = (0.9, 2.0, 0.4), (1.0, 3.0, 0.5)
HOVER_MASS, BOAT_MASS = 1000.0, 2000.0
HOVER_VOLUME = 8.0 * 0.9 * 2.0 * 0.4
BOAT_VOLUME = 8.0 * 1.0 * 3.0 * 0.5
MARGIN_DRAWN = 1.0e-3
SPLASH = [(-0.9, 2.5, -0.3, -1.0), (0.9, 2.5, -0.3, 1.0), (-1.0, 0.0, -0.35, -3.0)]      # (the third right_sign is clamped to -1)


def quat(axis, angle):
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.linalg.norm(a)
    s = np.sin(angle / 2)
    return np.array([a[0] * s, a[1] * s, a[2] * s, np.cos(angle / 2)])


def q_mul(a, b):
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw, aw * bw - ax * bx - ay * by - az * bz])


def craft_desc(k, seed):
    """The description of craft k (craft_reference.default_desc keys; body and volume are filled by the caller's scene)."""
    kind = cr.BOAT if k % 2 else cr.HOVERCAR
    d = cr.default_desc(kind, craft=k, seed=(seed * 7919 + k * 104729) & 0xFFFFFFFF, mass=BOAT_MASS if kind == cr.BOAT else HOVER_MASS)
    if k % 5 == 3:      # a model whose y-forward frame is not the object frame
        d["q1"] = tuple(np.float32(quat((0, 0, 1), 0.5)))
        d["q2"] = tuple(np.float32(quat((1, 0, 0), 0.1)))
    if kind == cr.HOVERCAR:
        d["trace_os"] = (0.0, 0.0, -0.408)
        d["volume"] = HOVER_VOLUME
    else:
        d.update(prop_os=(0.0, -2.8, -0.3), prop_off=0.6, thrust=30000.0, rudder=400.0, lateral=0.3 if k % 3 == 0 else 0.0, jet_w=3.0 if k % 7 == 1 else 0.7,
                 a_front=1.5, a_side=3.0, a_top=6.0, volume=BOAT_VOLUME, splash=list(SPLASH[:1 + (k // 2) % 3]))
    return d


def home(k):
    kind = k % 2
    x = SPACING * (k // 2)
    if kind:
        return np.array([x, 40.0, WATER_Z])
    return np.array([x, -20.0 if k % 4 == 0 else 20.0, 4.0])


def _draw(rng, k, kind):
    """One candidate (pos, rot, lin_vel, ang_vel, input)."""
    mode = rng.integers(10)
    yaw = quat((0, 0, 1), rng.uniform(-np.pi, np.pi))
    axis = (np.cos(a := rng.uniform(0, 2 * np.pi)), np.sin(a), 0.0)
    tilt = rng.uniform(2.7, 3.1) if mode == 0 else (rng.uniform(1.0, 2.2) if mode == 1 else rng.uniform(0.0, 0.5))      # flipped / on its side / nearly level
    rot = q_mul(yaw, quat(axis, tilt))
    rot = np.float32(rot / np.linalg.norm(rot))
    pos = home(k) + np.array([rng.uniform(-1, 1), rng.uniform(-1, 1), rng.uniform(-0.25, 0.25) if kind else rng.uniform(-1.0, 3.0)])
    speed = 0.0 if mode == 2 else rng.choice([0.5, 3.0, 8.0, 14.0]) * rng.uniform(0.7, 1.3)
    v = rng.normal(size=3) * np.array([1.0, 1.0, 0.3])
    lin_vel = v / np.linalg.norm(v) * speed
    ang_vel = rng.uniform(-1.5, 1.5, 3)
    inp = dict(forward=float(np.float32(rng.choice([0.0, 1.0, -1.0, -0.2, 2.0, rng.uniform(-1, 1)]))), right=float(np.float32(rng.choice([0.0, 1.0, -1.0, rng.uniform(-1, 1)]))),
               up=float(np.float32(rng.choice([0.0, 1.0, -1.0, rng.uniform(-1, 1)]))) if not kind else 0.0, hand_brake=float(rng.integers(2)) if not kind else 0.0)
    return np.float32(pos), rot, np.float32(lin_vel), np.float32(ang_vel), inp


def driver_flags(k, update):
    """Seats: a third of the crafts never has a driver (crafts 4, 5, 10, 11, ...); the boats with k % 6 == 1 take theirs at update 8 (which stops a righting in
    progress); the boats with k % 4 == 1 boost."""
    if (k // 2) % 3 == 2:
        return 0
    if k % 6 == 1 and update < 8:
        return 0
    return cr.IN_DRIVER | (cr.IN_BOOST if k % 4 == 1 else 0)


def righting_started(k, update):
    """sgp_crafts_start_righting calls: boats with k % 4 == 1 at update 0 and 12 (made after that update's inputs are set)."""
    return k % 2 == 1 and k % 4 == 1 and update in (0, 12)


def add_ground_box(w, n_crafts):
    """The static box under the hover cars with id % 4 == 0: top at z = GROUND_TOP, y in [-30, -10]."""
    from substrata_amd import abi
    d = w.default_body_desc()
    half = SPACING * (n_crafts // 2 + 2) / 2 + 10.0
    d.shape_type = abi.SHAPE_BOX
    d.shape[:] = (half, 10.0, 0.5, 0.0)
    d.pos[:] = (half - 10.0 - SPACING, -20.0, GROUND_TOP - 0.5)
    d.motion_type, d.layer = abi.MOTION_STATIC, abi.LAYER_NON_MOVING
    return w.add(d)


def add_craft_body(w, kind, pos, rot=(0, 0, 0, 1), gravity_factor=1.0):
    """The dynamic box a craft rides on; a boat's with use_zero_linear_drag = 1 (BoatPhysics.cpp:36)."""
    from substrata_amd import abi
    d = w.default_body_desc()
    d.shape_type = abi.SHAPE_BOX
    d.shape[:] = (BOAT_SHAPE if kind == cr.BOAT else HOVER_SHAPE) + (0.0,)
    d.pos[:] = tuple(float(x) for x in pos)
    d.rot[:] = tuple(float(x) for x in rot)
    d.mass = BOAT_MASS if kind == cr.BOAT else HOVER_MASS
    d.motion_type, d.layer = abi.MOTION_DYNAMIC, abi.LAYER_MOVING
    d.allow_sleeping, d.activate, d.gravity_factor = 0, 1, gravity_factor
    d.use_zero_linear_drag = 1 if kind == cr.BOAT else 0
    return w.add(d)


def twin_scene():
    """Four crafts that run free: a hover car over ground raising dust, a hover car over water, a driven boat, and a capsized boat being righted.
    Returns (descriptions, start poses, inputs, ids of the boats that start righting)."""
    descs = [craft_desc(0, 11), craft_desc(2, 11), craft_desc(1, 11), craft_desc(5, 11)]
    for i, d in enumerate(descs):
        d["craft"] = i
    poses = [(home(0) + (0, 0, -0.5), (0, 0, 0, 1)), (home(2), tuple(quat((0, 0, 1), 0.4))), (home(1) + (0, 0, 0.1), (0, 0, 0, 1)), (home(5) + (0, 0, 0.1), tuple(quat((0, 1, 0), 2.9)))]
    inputs = [dict(forward=0.5, right=0.3, up=0.2, hand_brake=0.0, flags=cr.IN_DRIVER), dict(forward=1.0, right=0.0, up=0.0, hand_brake=0.0, flags=cr.IN_DRIVER),
              dict(forward=1.0, right=0.5, up=0.0, hand_brake=0.0, flags=cr.IN_DRIVER | cr.IN_BOOST), dict(forward=0.0, right=0.0, up=0.0, hand_brake=0.0, flags=0)]
    return descs, poses, inputs, [3]


def apply_ops(w, body, ops):
    """The operations of one restated update through the body entry points, in order."""
    for op in ops:
        if op[0] == "activate":
            w.activate(body)
        elif op[0] == "force":
            w.add_force(body, [float(x) for x in op[1]])
        elif op[0] == "torque":
            w.add_torque(body, [float(x) for x in op[1]])
        else:
            w.add_force_at(body, [float(x) for x in op[1]], [float(x) for x in op[2]])


def run_twin_reference(w, horizon, trans_seed=None, dtype=np.float32):
    """The twin scene on world `w` (any CWorld) driven by the restatement through the body entry points; returns the bodies' states after every update + step."""
    descs, poses, inputs, righting = twin_scene()
    w.set_water(True, WATER_Z)
    add_ground_box(w, 8)
    bodies = [add_craft_body(w, d["kind"], p, r) for d, (p, r) in zip(descs, poses)]
    timers = [[-1.0, 2.0 if i in righting else -1.0] for i in range(len(descs))]
    counters = [0] * len(descs)
    tr = cr.Trans(dtype, trans_seed)
    history = []
    for u in range(horizon):
        st = w.get_state(bodies)
        for i, d in enumerate(descs):
            body = dict(pos=st["pos"][i], rot=st["rot"][i], lin_vel=st["lin_vel"][i], ang_vel=st["ang_vel"][i], submerged=st["submerged_volume"][i])
            r = cr.craft_update(d, inputs[i], body, timers[i], (True, WATER_Z), None, u, DT, counter=counters[i], dtype=dtype, trans=tr)
            timers[i], counters[i] = [r["unflip"], r["righting"]], r["counter"]
            apply_ops(w, bodies[i], r["ops"])
        w.step(DT)
        history.append(w.get_state(bodies).copy())
    return bodies, history


@functools.lru_cache(maxsize=None)
def parity_table(n=65, updates=20, seed=2024):
    rng = np.random.default_rng(seed)
    descs = [craft_desc(k, seed) for k in range(n)]
    table = []
    for u in range(updates):
        row = []
        for k in range(n):
            kind = k % 2
            while True:
                pos, rot, lv, av, inp = _draw(rng, k, kind)
                inp["flags"] = driver_flags(k, u)
                body = dict(pos=pos, rot=rot, lin_vel=lv, ang_vel=av, submerged=1.0)
                ok = True
                for timers in ((-1.0, -1.0), (0.5, 0.5)):
                    for fl in (inp["flags"], cr.IN_DRIVER):      # (with the seat taken too: every pose-dependent branch of the entry is looked at)
                        r = cr.craft_update(descs[k], dict(inp, flags=fl), body, timers, (True, WATER_Z), None, u, DT, dtype=np.float64)
                        ok = ok and cr.min_margin(r, ("pose",)) >= MARGIN_DRAWN
                if ok:
                    break
            row.append(dict(pos=pos, rot=rot, lin_vel=lv, ang_vel=av, inp=inp))
        table.append(row)
    return descs, table
