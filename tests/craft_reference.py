"""A numpy restatement of one craft update (sgp_crafts_update), written from docs/CONTRACT.md, "Crafts" -- a helper, not a test.

craft_update() is a pure function: (description, input, body state, timers, water, a ray oracle, update index) -> the ordered list of force / torque
operations, the new timers, the branch word, the emitted particles, and the margin of every branch condition.  Every value is a numpy scalar of `dtype`
(float32: the contract's arithmetic, one rounding per operation, in the contract's order; float64: the same formulas with the same fp32 constants and
inputs, as the yardstick of the fp32 rounding).  It never reads anything the craft kernels wrote.

`Trans` supplies acos / atan2 / sin / cos; with a seed it moves every result by one ulp (of dtype) in a seeded direction: how far a free-running
craft drifts when the transcendental functions of two implementations differ in the last place."""
import math

import numpy as np

HOVERCAR, BOAT = 0, 1
IN_DRIVER, IN_BOOST = 1, 2
BR = {"HOVER": 1 << 0, "UNFLIP": 1 << 1, "DRAG": 1 << 2, "LIFT_TOP": 1 << 3, "LIFT_BOTTOM": 1 << 4, "LIFT_RIGHT": 1 << 5, "LIFT_LEFT": 1 << 6,
      "THRUST": 1 << 7, "RUDDER": 1 << 8, "RIGHTING": 1 << 9, "RAY_BODY": 1 << 10, "RAY_WATER": 1 << 11, "ACTIVATE": 1 << 12, "SPLASH0": 1 << 16}
PK_SPRAY, PK_DUST, PK_JET, PK_SPLASH = 0, 1, 2, 3
DIE_ON_HIT = 1
MAX_TRACE_DIST = 12.0
FLT_MIN = 1.17549435e-38


def craft_rand(seed, update_index, draw):
    """The generator of the crafts: a function of (seed, update index, draw index) alone; a multiple of 2^-24 in [0, 1)."""
    m = 0xFFFFFFFF
    h = (seed ^ ((update_index * 0x9E3779B9) & m) ^ ((draw * 0x85EBCA6B) & m)) & m
    h ^= h >> 16
    h = (h * 0x7FEB352D) & m
    h ^= h >> 15
    h = (h * 0x846CA68B) & m
    h ^= h >> 16
    return (h >> 8) * 2.0 ** -24


class Trans:
    """acos, atan2, sin, cos in `dtype`; seed != None: every result moved by one ulp in a seeded direction."""

    def __init__(self, dtype, seed=None):
        self.T = dtype
        self.rng = np.random.default_rng(seed) if seed is not None else None

    def _out(self, v):
        v = self.T(v)
        if self.rng is None or not np.isfinite(v):
            return v
        return np.nextafter(v, self.T(np.inf if self.rng.integers(2) else -np.inf))

    def acos(self, x):
        with np.errstate(invalid="ignore"):
            return self._out(np.arccos(self.T(x)))

    def atan2(self, y, x):
        return self._out(np.arctan2(self.T(y), self.T(x)))

    def sin(self, x):
        return self._out(np.sin(self.T(x)))

    def cos(self, x):
        return self._out(np.cos(self.T(x)))


# ---- vectors as tuples of scalars of one dtype: every operation below rounds once, in the order it is written --------------------------------------
def v_add(a, b): return (a[0] + b[0], a[1] + b[1], a[2] + b[2])
def v_sub(a, b): return (a[0] - b[0], a[1] - b[1], a[2] - b[2])
def v_scale(a, s): return (a[0] * s, a[1] * s, a[2] * s)
def v_div(a, s): return (a[0] / s, a[1] / s, a[2] / s)
def v_neg(a): return (-a[0], -a[1], -a[2])
def v_dot(a, b): return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]
def v_cross(a, b): return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])
def v_len(a): return np.sqrt(v_dot(a, a))


def v_normalise(a):
    with np.errstate(invalid="ignore", divide="ignore"):
        return v_div(a, v_len(a))


def q_mul(a, b):
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return (aw * bx + ax * bw + ay * bz - az * by,
            aw * by - ax * bz + ay * bw + az * bx,
            aw * bz + ax * by - ay * bx + az * bw,
            aw * bw - ax * bx - ay * by - az * bz)


def q_conj(q): return (-q[0], -q[1], -q[2], q[3])


def q_to_m33(q, one):
    """Columns (c0, c1, c2) of the rotation matrix of q."""
    x, y, z, w = q
    x2, y2, z2 = x + x, y + y, z + z
    xx, yy, zz = x * x2, y * y2, z * z2
    xy, xz, yz = x * y2, x * z2, y * z2
    wx, wy, wz = w * x2, w * y2, w * z2
    return ((one - (yy + zz), xy + wz, xz - wy), (xy - wz, one - (xx + zz), yz + wx), (xz + wy, yz - wx, one - (xx + yy)))


def m_mul(m, v):
    c0, c1, c2 = m
    return (c0[0] * v[0] + c1[0] * v[1] + c2[0] * v[2], c0[1] * v[0] + c1[1] * v[1] + c2[1] * v[2], c0[2] * v[0] + c1[2] * v[1] + c2[2] * v[2])


def default_desc(kind, **kw):
    d = dict(kind=kind, craft=0, mass=1000.0, q1=(0, 0, 0, 1), q2=(0, 0, 0, 1), seed=0, trace_os=(0, 0, 0), thrust=40000.0, prop_os=(0, 0.2, -6.2),
             prop_off=1.0, rudder=500.0, lateral=0.0, jet_w=1.0, a_front=2.0, a_side=4.0, a_top=8.0, volume=1.0, splash=[])
    d.update(kw)
    return d


def _margin(value, threshold, scale=None):
    value, threshold = float(value), float(threshold)
    s = abs(threshold) if scale is None else scale
    return abs(value - threshold) / s if np.isfinite(value) else np.inf


def craft_update(desc, inp, body, timers, water, ray, update_index, dt, counter=0, dtype=np.float32, trans=None):
    """One update of one craft.
    desc: default_desc() keys; inp: dict(forward, right, up, hand_brake, flags); body: dict(pos, rot, lin_vel, ang_vel, submerged);
    timers: (unflip, righting); water: (enabled, z); ray: callable(origin xyz, dir xyz) -> (hit id or None, t), asked at most once;
    returns dict(ops, unflip, righting, branches, particles, counter, margins, trace_origin, trace_t, trace_body, force, torque, force_scale, torque_scale).
    ops: ("activate",) | ("force", F) | ("force_at", F, P) | ("torque", T) in the order of the reference's calls.
    margins: (kind, name, relative distance of the deciding value from its threshold), kind "pose" or "dyn" (submerged volume, ray)."""
    T = dtype
    tr = trans if trans is not None else Trans(T)
    c = lambda x: T(np.float32(x))                      # an fp32 constant of the reference
    f = lambda x: T(np.float32(x))                      # an fp32 input
    vec = lambda a: tuple(f(x) for x in a)
    one, zero = T(1), T(0)
    kind, mass = desc["kind"], f(desc["mass"])
    seed = int(desc["seed"]) & 0xFFFFFFFF
    rnd = lambda k: T(craft_rand(seed, update_index, k))
    forward, right, up_in, hand_brake, flags = f(inp["forward"]), f(inp["right"]), f(inp["up"]), f(inp["hand_brake"]), int(inp["flags"])
    pos, q, lin_vel, ang_vel = vec(body["pos"]), vec(body["rot"]), vec(body["lin_vel"]), vec(body["ang_vel"])
    submerged = f(body["submerged"])
    unflip, righting = f(timers[0]), f(timers[1])
    water_on, water_z = bool(water[0]), f(water[1])
    dt = f(dt)
    ops, particles, margins = [], [], []
    out = dict(branches=0, trace_origin=(zero, zero, zero), trace_t=zero, trace_body=None)

    # the frame
    r_quat = q_mul(vec(desc["q2"]), vec(desc["q1"]))
    ri = q_to_m33(q_conj(r_quat), one)
    right_os, fwd_os = ri[0], ri[1]
    up_os = v_cross(right_os, fwd_os)
    R = q_to_m33(q, one)
    right_ws, fwd_ws, up_ws = m_mul(R, right_os), m_mul(R, fwd_os), m_mul(R, up_os)
    point = lambda p_os: v_add(m_mul(R, vec(p_os)), pos)

    def lift_coeff(cos_theta, name):
        theta = tr.acos(cos_theta)
        alpha = c(1.5707964) - theta
        thr = c(25.0) * c(0.017453292)
        margins.append(("pose", name, _margin(alpha, thr)))
        return c(2.0) if alpha < thr else zero

    def axis_times_angle(d):
        if d[3] < zero:
            d = (-d[0], -d[1], -d[2], -d[3])
        if d[3] >= one:
            return (zero, zero, zero)
        angle = c(2.0) * tr.acos(d[3])
        len_sq = d[0] * d[0] + d[1] * d[1] + d[2] * d[2]
        if len_sq <= T(FLT_MIN):
            return (zero, zero, zero)
        ln = np.sqrt(len_sq)
        return v_scale((d[0] / ln, d[1] / ln, d[2] / ln), angle)

    def correction_torque(yaw, gain):
        yq = (zero, zero, tr.sin(c(0.5) * yaw), tr.cos(c(0.5) * yaw))
        desired = q_mul(yq, r_quat)
        dav = v_scale(axis_times_angle(q_mul(desired, q_conj(q))), c(3.0))
        return v_scale(v_scale(v_sub(dav, ang_vel), mass), gain)

    def emit(pk, p, v, area, width, opacity, dopacity, fl):
        nonlocal counter
        particles.append(dict(pos=p, vel=v, area=c(area), mass=c(1.0e-6), restitution=c(0.5), width=width, dwidth_dt=c(1.0), opacity=c(opacity), dopacity_dt=c(dopacity),
                              flags=fl, kind=pk, tag=(int(desc["craft"]) << 32) | (pk << 28) | (counter & 0x0FFFFFFF)))
        counter += 1

    def drag(rho, cds, areas, fractions):
        v_mag = v_len(lin_vel)
        nv = v_div(lin_vel, v_mag)
        fd = []
        for axis, cd, area, frac in zip((fwd_ws, right_ws, up_ws), cds, areas, fractions):
            x = c(0.5) * rho * v_mag * v_mag * cd * (abs(v_dot(nv, axis)) * area)
            fd.append(x if frac is None else x * frac)
        total = fd[0] + fd[1] + fd[2]
        ops.append(("force", v_scale(nv, -total)))
        out["branches"] |= BR["DRAG"]
        return v_mag, nv

    if kind == HOVERCAR:
        if flags & IN_DRIVER:
            if right != zero or forward != zero or hand_brake != zero:
                ops.append(("activate",))
                out["branches"] |= BR["ACTIVATE"]
            margins.append(("pose", "up.z > 0", _margin(up_ws[2], 0.0, 1.0)))
            if up_ws[2] > zero:
                factor = one / max(c(0.7), up_ws[2])
                ops.append(("force", v_scale(v_scale(v_scale(v_scale(up_ws, one + up_in * c(0.6)), factor), mass), c(9.81))))
                out["branches"] |= BR["HOVER"]
            if unflip > zero:
                margins.append(("pose", "up.z > 0.2", _margin(up_ws[2], 0.2)))
                if np.float64(up_ws[2]) > 0.2:
                    unflip = -one
                else:
                    ops.append(("force", v_scale(v_scale(v_scale((zero, zero, one), one), mass), c(9.81))))
                    unflip = unflip - dt
                    out["branches"] |= BR["UNFLIP"]
            else:
                margins.append(("pose", "up.z < -0.9", _margin(up_ws[2], -0.9)))
                if np.float64(up_ws[2]) < -0.9:
                    unflip = one
            fcf = v_scale(v_scale(v_scale(fwd_ws, mass), c(10.0)), forward)
            ops.append(("force", fcf))
            ops.append(("force", v_scale(up_ws, -fcf[2])))
            ops.append(("torque", v_scale(v_scale(v_scale(right_ws, mass), c(-0.5)), forward)))
            ops.append(("torque", v_scale(v_scale(v_scale(up_ws, mass), c(-3.0)), right)))
            ops.append(("torque", v_scale(v_scale(v_scale(fwd_ws, mass), c(2.0)), right)))
            ops.append(("torque", correction_torque(tr.atan2(right_ws[1], right_ws[0]), c(1.5))))

            v_mag = v_len(lin_vel)
            margins.append(("pose", "v_mag > 1e-3", _margin(v_mag, 1.0e-3)))
            if v_mag > c(1.0e-3):
                rho = c(1.293)
                v_mag, nv = drag(rho, (c(0.2), c(0.5), c(0.75)), (c(2.0), c(4.0), c(8.0)), (None, None, None))
                up_dir = v_sub(up_ws, v_scale(nv, v_dot(up_ws, nv)))
                margins.append(("pose", "up lift dir", _margin(v_len(up_dir), 1.0e-3)))
                if v_len(up_dir) > c(1.0e-3):
                    top_dot = v_dot(nv, up_ws)
                    margins.append(("pose", "top_dot sign", _margin(top_dot, 0.0, 1.0)))
                    top_cl = lift_coeff(top_dot, "top lift 25 deg")
                    top_area = top_dot * c(8.0)
                    if top_cl > zero and top_area > zero:
                        top_l = c(0.5) * rho * v_mag * v_mag * top_area * top_cl
                        ops.append(("force", v_scale(v_neg(v_normalise(up_dir)), top_l)))
                        out["branches"] |= BR["LIFT_TOP"]
                    bottom_area = -top_area
                    bottom_cl = lift_coeff(-top_dot, "bottom lift 25 deg")
                    if bottom_cl > zero and bottom_area > zero:
                        bottom_l = c(0.5) * rho * v_mag * v_mag * bottom_area * bottom_cl
                        ops.append(("force", v_scale(v_normalise(up_dir), bottom_l)))
                        out["branches"] |= BR["LIFT_BOTTOM"]
                right_dir = v_sub(right_ws, v_scale(nv, v_dot(right_ws, nv)))
                margins.append(("pose", "right lift dir", _margin(v_len(right_dir), 1.0e-3)))
                if v_len(right_dir) > c(1.0e-3):
                    right_dot = v_dot(nv, right_ws)
                    margins.append(("pose", "right_dot sign", _margin(right_dot, 0.0, 1.0)))
                    right_cl = lift_coeff(right_dot, "right lift 25 deg")
                    right_area = v_dot(nv, right_ws) * c(4.0)
                    if right_area > zero:
                        right_l = c(0.5) * rho * v_mag * v_mag * right_area * right_cl
                        ops.append(("force", v_scale(v_neg(v_normalise(right_dir)), right_l)))
                        out["branches"] |= BR["LIFT_RIGHT"]
                    left_area = -right_area
                    left_cl = lift_coeff(-right_dot, "left lift 25 deg")
                    if left_area > zero:
                        left_l = c(0.5) * rho * v_mag * v_mag * left_area * left_cl
                        ops.append(("force", v_scale(v_normalise(right_dir), left_l)))
                        out["branches"] |= BR["LIFT_LEFT"]

            origin = point(desc["trace_os"])
            out["trace_origin"] = origin
            side_vec = v_add(v_scale(right_ws, c(-0.5) + rnd(0)), v_scale(fwd_ws, c(-0.5) + rnd(1)))
            trace_dir = v_normalise(v_add(v_neg(up_ws), v_scale(side_vec, c(0.8))))
            out["trace_dir"] = trace_dir
            hit_id, hit_t = ray(origin, trace_dir) if ray is not None else (None, 0.0)
            hit_t = f(hit_t)
            out["trace_body"], out["trace_t"] = hit_id, (hit_t if hit_id is not None else zero)
            mtd = c(MAX_TRACE_DIST)
            with np.errstate(divide="ignore", invalid="ignore"):
                whd = (water_z - origin[2]) / trace_dir[2]
            water_hit = False
            if water_on:
                margins.append(("dyn", "water_hit_dist >= 0", _margin(whd, 0.0, 1.0)))
                margins.append(("dyn", "water_hit_dist < 12", _margin(whd, MAX_TRACE_DIST)))
                if hit_id is not None:
                    margins.append(("dyn", "hit_t > water_hit_dist", _margin(hit_t, float(whd), max(abs(float(whd)), 1.0e-30)) if np.isfinite(whd) else np.inf))
                water_hit = bool(whd >= zero and whd < mtd and (hit_id is None or hit_t > whd))
            if water_hit:
                hitpos = v_add(origin, v_scale(trace_dir, whd))
                t = whd / mtd
                vel = c(20.0) * (one - t) + c(6.0) * t
                for z in range(4):
                    rx, ry, rz = rnd(2 + 3 * z), rnd(3 + 3 * z), rnd(4 + 3 * z)
                    pv = v_scale(v_add(side_vec, (one * (c(-0.5) + rx), one * (c(-0.5) + ry), rz * c(0.2))), vel)
                    emit(PK_SPRAY, hitpos, pv, 0.000001, c(2.0), 0.5, -0.06, DIE_ON_HIT)
                out["branches"] |= BR["RAY_WATER"]
            elif hit_id is not None:
                hitpos = v_add(origin, v_scale(trace_dir, hit_t))
                t = hit_t / mtd
                vel = c(20.0) * (one - t) + c(6.0) * t
                rx, ry, rz = rnd(2), rnd(3), rnd(4)
                pv = v_scale(v_add(side_vec, (zero * (c(-0.5) + rx), zero * (c(-0.5) + ry), rz * c(0.2))), vel)
                emit(PK_DUST, hitpos, pv, 0.00001, c(2.0), 0.5, -0.06, 0)
                out["branches"] |= BR["RAY_BODY"]
    else:
        forwards_vel = v_dot(lin_vel, fwd_ws)
        if flags & IN_DRIVER:
            if right != zero or forward != zero:
                ops.append(("activate",))
                out["branches"] |= BR["ACTIVATE"]
            prop = point(desc["prop_os"])
            if forward != zero:
                if water_on:
                    margins.append(("pose", "propellor under water", _margin(prop[2], water_z, max(abs(float(water_z)), 1.0))))
                if water_on and prop[2] <= water_z:
                    lateral = f(desc["lateral"])
                    d = v_normalise(v_sub(v_sub(fwd_ws, v_scale(up_ws, c(0.2))), v_scale(v_scale(right_ws, right), lateral)))
                    ops.append(("force_at", v_scale(v_scale(d, f(desc["thrust"])), forward), prop))
                    out["branches"] |= BR["THRUST"]
                    off = f(desc["prop_off"])
                    positions = (v_sub(prop, v_scale(right_ws, off)), v_add(prop, v_scale(right_ws, off)))
                    vel = c(2.0) if flags & IN_BOOST else c(1.0)
                    xy = vel * c(0.5)
                    width = min(max(f(desc["jet_w"]), c(0.01)), c(2.0))
                    for i in range(2):
                        for z in range(3):
                            base = 3 * (3 * i + z)
                            rx, ry, rz = rnd(base), rnd(base + 1), rnd(base + 2)
                            a = v_scale(fwd_ws, forward * -vel)
                            b = v_scale(v_scale(v_scale(right_ws, right), c(3.0)), lateral)
                            cc = v_scale((xy * (c(-0.5) + rx), xy * (c(-0.5) + ry), c(2.0) + rz * c(4.0)), vel)
                            emit(PK_JET, positions[i], v_add(v_sub(a, b), cc), 0.000001, width, 1.0, -0.3, DIE_ON_HIT)
            if right != zero:
                ops.append(("force_at", v_scale(v_scale(v_scale(right_ws, -right), forwards_vel), f(desc["rudder"])), prop))
                out["branches"] |= BR["RUDDER"]

        volume = f(desc["volume"])
        frac = submerged / volume
        ss = min(max((submerged - zero) / (one - zero), zero), one)
        top_frac = ss * ss * (c(3.0) - c(2.0) * ss)
        v_mag = v_len(lin_vel)
        margins.append(("pose", "v_mag > 1e-3", _margin(v_mag, 1.0e-3)))
        # (submerged > 0 compares an input with zero: nothing is rounded on the way, so it has no margin to state)
        if submerged > zero and v_mag > c(1.0e-3):
            drag(c(1020.0), (c(0.1), c(0.5), c(0.75)), (f(desc["a_front"]), f(desc["a_side"]), f(desc["a_top"])), (frac, frac, top_frac))
            # (the lift block of BoatPhysics.cpp:272-318 is disabled in the reference and stays disabled)
        if desc["splash"]:
            margins.append(("pose", "v_mag > 5", _margin(v_mag, 5.0)))
        for p, sp in enumerate(desc["splash"]):
            if not v_mag > c(5.0):
                continue
            sign = min(max(f(sp[3]), -one), one)
            pt = point(sp[:3])
            if water_on:
                margins.append(("pose", "splash point %d under water" % p, _margin(pt[2], water_z, max(abs(float(water_z)), 1.0))))
            immersed = water_on and pt[2] < water_z
            rvd = v_cross(lin_vel, (zero, zero, one))
            svd = v_scale(rvd, sign)
            side_dir = v_scale(right_ws, sign)
            dotv = v_dot(v_normalise(lin_vel), side_dir)
            margins.append(("pose", "splash %d dot > -0.5" % p, _margin(dotv, -0.5)))
            if immersed and dotv > c(-0.5):
                for z in range(2):
                    base = 18 + 3 * (2 * p + z)
                    r0, r1, r2 = rnd(base), rnd(base + 1), rnd(base + 2)
                    a = v_scale(lin_vel, c(0.6) + (c(-0.5) + r0) * c(0.1))
                    b = v_scale(svd, c(0.3) + (c(-0.5) + r1) * c(0.1))
                    cc = v_scale(v_scale((zero, zero, one), v_mag), c(0.1) + (c(-0.5) + r2) * c(0.08))
                    emit(PK_SPLASH, pt, v_add(v_add(a, b), cc), 0.01, c(0.4), 1.0, -0.3, DIE_ON_HIT)
                out["branches"] |= BR["SPLASH0"] << p
        if righting > zero:
            nrr = v_normalise(v_cross(fwd_ws, (zero, zero, one)))
            ops.append(("torque", correction_torque(tr.atan2(nrr[1], nrr[0]), c(3.5))))
            righting = righting - dt
            out["branches"] |= BR["RIGHTING"]

    # the totals as the device keeps them: sums in op order, a force at a point adding cross(point - pos, F) to the torque
    F, Tq = (zero, zero, zero), (zero, zero, zero)
    fs, ts = 0.0, 0.0
    for op in ops:
        if op[0] == "force":
            F = v_add(F, op[1]); fs += float(v_len(op[1]))
        elif op[0] == "torque":
            Tq = v_add(Tq, op[1]); ts += float(v_len(op[1]))
        elif op[0] == "force_at":
            t = v_cross(v_sub(op[2], pos), op[1])
            F = v_add(F, op[1]); Tq = v_add(Tq, t); fs += float(v_len(op[1])); ts += float(v_len(t))
    out.update(ops=ops, unflip=unflip, righting=righting, particles=particles, counter=counter, margins=margins, force=F, torque=Tq, force_scale=fs, torque_scale=ts)
    return out


def min_margin(result, kinds=("pose", "dyn")):
    ms = [m for k, _, m in result["margins"] if k in kinds]
    return min(ms) if ms else math.inf
