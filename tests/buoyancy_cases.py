"""The case table of the buoyancy tests and the run that compares a world (the CPU oracle or the product) with tests/buoyancy_reference.py.

Two worlds hold the same bodies, one with water at z = 0 and one without; both take one step.  Buoyancy is the last stage of a step and changes
velocities only, so the dry world's velocities are, bit for bit, those the sweep started from, and the wet world's pose is the pose it saw.  The
reference is evaluated at that pose with those velocities: no model of the integrator is needed.  A dry calibration world goes first: it tells by how
much a step moves and turns each body, so that the bodies can be started where the step takes them to the wanted depth and rotation.
"""
import numpy as np

from substrata_amd import abi
from buoyancy_reference import Shape, evaluate, quat_to_mat

EPS32 = float(np.finfo(np.float32).eps)
DT = float(np.float32(1.0 / 60.0))
WATER_Z = 0.0
SPACING = 3.0
COLUMNS = 20
FRACTIONS = (1.0e-4, 1.0e-3, 0.3, 0.5, 0.999, 1.05, 1.5, -0.2)      # water plane as a fraction of the body's vertical extent, from its lowest point
MASSES = (1.0, 80.0, 2000.0)
GRAVITY_FACTORS = (1.0, 0.0, 0.5, 2.0)
COM_OFFSET = (0.1, -0.05, 0.2)


def _q_mul(a, b):
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw, aw * bw - ax * bx - ay * by - az * bz])


def _q_conj(q):
    return np.array([-q[0], -q[1], -q[2], q[3]])


def _q_axis_angle(axis, angle):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    return np.append(a * np.sin(0.5 * angle), np.cos(0.5 * angle))


def _q_from_to(a, b):
    """The shortest turn that takes direction a to direction b."""
    a, b = np.asarray(a, np.float64) / np.linalg.norm(a), np.asarray(b, np.float64) / np.linalg.norm(b)
    return _q_axis_angle(np.cross(a, b), np.arccos(np.clip(np.dot(a, b), -1.0, 1.0)))


def _box_points(h):
    return np.array([(sx * h[0], sy * h[1], sz * h[2]) for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)], np.float32)


def shape_specs():
    """(name, kind, parameters): boxes, a sphere, two capsules (the thin one for the angular clamp), four hulls."""
    rng = np.random.default_rng(11)
    cloud = (rng.uniform(-1.0, 1.0, size=(16, 3)) * (0.35, 0.3, 0.25)).astype(np.float32)
    # a wedge with a long thin nose: its bounds about the centre of mass are far from symmetric, which the drag's `size` is sensitive to
    lop = np.array([(-0.2, -0.25, -0.15), (-0.2, 0.25, -0.15), (-0.2, -0.25, 0.15), (-0.2, 0.25, 0.15), (0.1, -0.2, -0.1), (0.1, 0.2, -0.1), (0.1, 0.0, 0.12), (0.5, 0.02, 0.0)], np.float32)
    return [("box", abi.SHAPE_BOX, dict(h=(0.35, 0.3, 0.25))),
            ("sphere", abi.SHAPE_SPHERE, dict(r=0.35)),
            ("capsule", abi.SHAPE_CAPSULE, dict(r=0.2, hh=0.4)),
            ("thin capsule", abi.SHAPE_CAPSULE, dict(r=0.1, hh=1.0)),
            ("hull of 8 (box)", abi.SHAPE_HULL, dict(points=_box_points((0.3, 0.25, 0.2)), offset=None)),
            ("lopsided hull", abi.SHAPE_HULL, dict(points=lop, offset=None)),
            ("hull of 16", abi.SHAPE_HULL, dict(points=cloud, offset=None)),
            ("hull of 16, offset", abi.SHAPE_HULL, dict(points=cloud, offset=COM_OFFSET)),
            ("cube", abi.SHAPE_BOX, dict(h=(0.25, 0.25, 0.25)))]


def build_cases():
    """The table: dicts of shape (index into shape_specs), rot (target rotation after the step), frac, mass, gravity_factor, zero_lin_drag, lin_vel, ang_vel."""
    rng = np.random.default_rng(2024)
    specs = shape_specs()
    cases = []

    def add(si, rot, frac, **kw):
        thin = specs[si][0] == "thin capsule"
        moving = kw.pop("moving", rng.random() < 0.5)
        lin, ang = np.zeros(3), np.zeros(3)
        if moving:
            lin, ang = rng.uniform(-3.0, 3.0, 3), rng.uniform(-4.0, 4.0, 3)
            if thin:      # spinning about its long axis, where its inertia is small: angular drag would reverse the spin
                ang = quat_to_mat(rot)[:, 2] * 3.5 + rng.uniform(-0.5, 0.5, 3)
            if frac < 0.0:
                lin[2] = abs(lin[2])      # (a body above the water does not dive in during the second step either)
        # A light body under water gains tens of m/s in a step: 167 m/s per m^3 of water displaced and kg.  What the float32 sum of the submerged volume can be
        # off by, about eps32 * V_total, is then a velocity of 167 * eps32 * V_total / m: for 1 kg and a sliver under water, where neither the body's own
        # velocity nor the change gives the bound anything to scale with, more than the bound (measured on the CPU oracle: up to 10 times).  The light bodies
        # are there for the drag clamp, which needs depth anyway, and take the cases from 0.3 up.
        masses = MASSES if frac >= 0.3 else MASSES[1:]
        c = dict(shape=si, rot=np.asarray(rot, np.float64), frac=float(frac), mass=float(kw.pop("mass", rng.choice(masses))),
                 gravity_factor=float(kw.pop("gravity_factor", rng.choice(GRAVITY_FACTORS))), zero_lin_drag=int(kw.pop("zero_lin_drag", rng.random() < 0.3)),
                 lin_vel=lin, ang_vel=ang, exact=False)
        assert not kw
        cases.append(c)
        return c

    for si, (name, kind, p) in enumerate(specs[:-1]):
        diag = np.asarray(p["h"], np.float64) if kind == abi.SHAPE_BOX else np.ones(3)
        rots = [np.array([0.0, 0.0, 0.0, 1.0]), _q_axis_angle((1, 0, 0), 0.5 * np.pi), _q_axis_angle((0, 1, 0), 0.5 * np.pi),
                _q_axis_angle(rng.normal(size=3), 1.0e-4), _q_from_to(diag, (0, 0, 1)), _q_axis_angle(rng.normal(size=3), rng.uniform(0.3, 3.0))]
        for rot in rots:
            for frac in FRACTIONS:
                add(si, rot, frac)
    # a cube on its corner: the plane through the three corners next to the lowest one, the hexagon through the middle, the three next to the highest
    cube = len(specs) - 1
    for frac in (1.0 / 3.0, 0.5, 2.0 / 3.0):
        for moving in (False, True):
            add(cube, _q_from_to((1, 1, 1), (0, 0, 1)), frac, moving=moving)
    # at rest and weightless, the lower face ends exactly in the plane: nothing under water, no flag, no event
    c = add(0, (0.0, 0.0, 0.0, 1.0), 0.0, moving=False, gravity_factor=0.0, mass=80.0, zero_lin_drag=0)
    c["exact"] = True
    return cases


def make_shapes(world):
    """Creates the hulls in `world`; returns the shape records for the body descs and the reference's Shape of every spec."""
    recs, shapes = [], []
    for name, kind, p in shape_specs():
        if kind == abi.SHAPE_BOX:
            recs.append(tuple(p["h"]) + (0.0,)); shapes.append(Shape.box(np.asarray(p["h"], np.float32)))
        elif kind == abi.SHAPE_SPHERE:
            recs.append((p["r"], 0.0, 0.0, 0.0)); shapes.append(Shape.sphere(float(np.float32(p["r"]))))
        elif kind == abi.SHAPE_CAPSULE:
            recs.append((p["r"], p["hh"], 0.0, 0.0)); shapes.append(Shape.capsule(float(np.float32(p["r"])), float(np.float32(p["hh"]))))
        else:
            info = world.hull_create(p["points"], com_offset=p["offset"])
            recs.append((float(info.hull_id), 0.0, 0.0, 0.0)); shapes.append(Shape.hull(p["points"], info, p["offset"]))
    return recs, shapes


def populate(world, cases, recs, z, rot):
    specs = shape_specs()
    for k, c in enumerate(cases):
        d = world.default_body_desc()
        d.shape_type = specs[c["shape"]][1]
        d.shape[:] = recs[c["shape"]]
        d.pos[:] = (SPACING * (k % COLUMNS), SPACING * (k // COLUMNS), z[k])
        d.rot[:] = tuple(rot[k])
        d.lin_vel[:], d.ang_vel[:] = tuple(c["lin_vel"]), tuple(c["ang_vel"])
        d.mass, d.gravity_factor, d.use_zero_linear_drag = c["mass"], c["gravity_factor"], c["zero_lin_drag"]
        d.motion_type, d.layer, d.allow_sleeping, d.activate = abi.MOTION_DYNAMIC, abi.LAYER_MOVING, 0, 1
        assert world.add(d) == k


class Run:
    pass


def run_table(make_world):
    """make_world(max_bodies) -> a CWorld.  Returns a Run: cases, shapes, the wet and the dry world's states after one step, the reference's results, the
    wet world (still open, for the event and flag checks) and the figures compare() needs."""
    cases = build_cases()
    n = len(cases)
    r = Run()
    # how far one step moves and turns each body
    cal = make_world(1024)
    recs, shapes = make_shapes(cal)
    rot0 = np.array([c["rot"] for c in cases])
    populate(cal, cases, recs, np.zeros(n), rot0)
    cal.step(DT)
    s = cal.read_states(0, n)
    cal.close()
    z, rot = np.zeros(n), rot0.copy()
    for k, c in enumerate(cases):
        if c["exact"]:
            z[k] = float(np.float32(shape_specs()[c["shape"]][2]["h"][2]))
            continue
        turn = _q_mul(s["rot"][k].astype(np.float64), _q_conj(rot0[k]))
        rot[k] = _q_mul(_q_conj(turn), rot0[k])
        lo, hi = shapes[c["shape"]].vertical_extent(quat_to_mat(rot0[k]))
        z[k] = (WATER_Z - lo - c["frac"] * (hi - lo)) - float(s["pos"][k][2])
    r.wet, r.dry = make_world(1024), make_world(1024)
    for w in (r.wet, r.dry):
        recs, _ = make_shapes(w)
        populate(w, cases, recs, z, rot)
    r.wet.set_water(True, WATER_Z)
    r.wet.step(DT); r.dry.step(DT)
    r.on, r.off = r.wet.read_states(0, n), r.dry.read_states(0, n)
    r.dry.close()
    r.cases, r.shapes, r.n = cases, shapes, n
    r.ref = [evaluate(shapes[c["shape"]], c["mass"], c["gravity_factor"], c["zero_lin_drag"], r.on["pos"][k], r.on["rot"][k], r.off["lin_vel"][k], r.off["ang_vel"][k], WATER_Z, DT)
             for k, c in enumerate(cases)]
    return r


def table_conditions(r):
    """What the table promises, by the reference's own count."""
    specs = shape_specs()
    ref, cases = r.ref, r.cases
    assert sum(x.lin_clamped for x in ref) >= 5 and sum(x.ang_clamped for x in ref) >= 5, (sum(x.lin_clamped for x in ref), sum(x.ang_clamped for x in ref))
    assert sum(x.fully_submerged and specs[c["shape"]][2].get("offset") is not None for x, c in zip(ref, cases)) >= 10
    assert sum(x.underwater and x.fraction <= 1.0e-3 for x in ref) >= 20
    for x, c in zip(ref, cases):
        if c["exact"]:
            assert x.bottom == WATER_Z and not x.underwater
        else:
            assert abs(x.bottom - WATER_Z) > 1.0e-5, (c, x.bottom)      # the gate is the exact case's business
            assert x.underwater == (c["frac"] > 0.0)
    assert np.array_equal(r.on["pos"], r.off["pos"]) and np.array_equal(r.on["rot"], r.off["rot"])


def expect_underwater(r, k):
    """The flag says "some volume is under water".  Where the reference's volume is positive but within the bound on the volume itself, 16 eps32 V_total -- a
    corner dipping 1e-4 of the body's height in is 1e-12 of its volume --, the float32 sum may come out as zero and the body then counts as dry, flag, event
    and all; there the flag has to agree with the volume the world reports.  Everywhere else the reference decides."""
    x, total = r.ref[k], r.shapes[r.cases[k]["shape"]].total
    if x.volume == 0.0 or x.volume > 16.0 * EPS32 * total:
        return x.volume > 0.0
    return float(r.on["submerged_volume"][k]) > 0.0


def compare(r):
    """Per case: the error of the submerged volume in units of eps32 * V_total, and of the linear and the angular velocity change in units of the bound
    8 eps32 max|v| + 2e-5 max|dv_ref| (so: <= 16 and <= 1 pass).  Both maxima run over all of the body's velocity components, linear and angular, before
    and after: the torque is the lever arm of the centre of buoyancy times the linear impulse, so the rounding of that arm (eps32 of the body's size, whatever
    the arm's length) puts an error on the angular change that scales with the linear one -- also where the angular change itself is zero by symmetry and
    the body has no spin, where a bound from the angular components alone would be zero.  The flag: expect_underwater()."""
    vol_err, lin_err, ang_err, flags_ok = np.zeros(r.n), np.zeros(r.n), np.zeros(r.n), np.zeros(r.n, bool)
    for k, (c, x) in enumerate(zip(r.cases, r.ref)):
        sh = r.shapes[c["shape"]]
        vol_err[k] = abs(float(r.on["submerged_volume"][k]) - x.volume) / (EPS32 * sh.total)
        flags_ok[k] = int(r.on["underwater"][k]) == int(expect_underwater(r, k)) and int(r.off["underwater"][k]) == 0
        vmax = max(float(np.max(np.abs(s[f][k]))) for s in (r.on, r.off) for f in ("lin_vel", "ang_vel"))
        bound = 8.0 * EPS32 * vmax + 2.0e-5 * max(float(np.max(np.abs(x.dlin))), float(np.max(np.abs(x.dang))))
        for f, dref, out in (("lin_vel", x.dlin, lin_err), ("ang_vel", x.dang, ang_err)):
            err = float(np.max(np.abs((r.on[f][k].astype(np.float64) - r.off[f][k].astype(np.float64)) - dref)))
            out[k] = err / bound if bound > 0.0 else (0.0 if err == 0.0 else np.inf)
    return vol_err, lin_err, ang_err, flags_ok


def describe(r, k):
    c = r.cases[k]
    return f"case {k}: {shape_specs()[c['shape']][0]}, frac {c['frac']:g}, mass {c['mass']:g}, gf {c['gravity_factor']:g}, zero drag {c['zero_lin_drag']}, rot {np.round(c['rot'], 4)}, v {np.round(c['lin_vel'], 2)}, w {np.round(c['ang_vel'], 2)}"


def check_events_and_flags(r):
    """EVENT_ENTERED_WATER exactly for the bodies with volume under water, once; none on a second step; lifted out of the water, flag and volume go."""
    w = r.wet
    ev = w.drain_events(abi.EVENT_ENTERED_WATER)
    want = [k for k in range(r.n) if expect_underwater(r, k)]
    assert sorted(ev["id"].tolist()) == want
    w.step(DT)
    again = w.drain_events(abi.EVENT_ENTERED_WATER)["id"].tolist()
    s = w.read_states(0, r.n)
    # nobody enters twice (a body that was dry after the first step and moving down may enter now: once, and it is flagged)
    assert not set(again) & set(want) and len(set(again)) == len(again) and all(s["underwater"][k] == 1 and r.cases[k]["frac"] <= 1.0e-3 for k in again)
    for k in range(r.n):
        w.set_pos(k, (float(s["pos"][k][0]), float(s["pos"][k][1]), WATER_Z + 5.0))
    w.step(DT)
    s = w.read_states(0, r.n)
    assert not s["underwater"].any() and not s["submerged_volume"].any()
    assert len(w.drain_events(abi.EVENT_ENTERED_WATER)) == 0


def check_sleeper(make_world):
    """A body that falls asleep under water keeps its flag and its volume, and the sweep leaves it alone."""
    from helpers import add_ground, dyn
    w = make_world(16)
    add_ground(w)
    w.set_water(True, 3.0)
    i = dyn(w, shape=(0.5, 0.5, 0.5, 0.0), pos=(0, 0, 0.5), mass=2000.0, restitution=0.0)      # twice as dense as the water: stays down
    s = None
    for _ in range(600):
        w.step(DT)
        s = w.get_state([i])[0]
        if not s["active"]:
            break
    assert not s["active"] and s["underwater"] == 1 and s["submerged_volume"] > 0.99
    vol = float(s["submerged_volume"])
    w.step(DT)
    s = w.get_state([i])[0]
    assert not s["active"] and s["underwater"] == 1 and float(s["submerged_volume"]) == vol
    assert not s["lin_vel"].any() and not s["ang_vel"].any()
    assert len(w.drain_events(abi.EVENT_ENTERED_WATER)) == 1
    w.close()
