"""A numpy restatement of the movers (sgp_path_prepare / sgp_path_advance / sgp_movers_update), written from docs/CONTRACT.md 4j -- a helper, not a test.

Every value is a numpy scalar of `T` (float32: the contract's arithmetic, one rounding per operation, in the contract's order; float64: the same formulas
with the same fp32 inputs, as the yardstick of the fp32 rounding).  Nothing here reads what the library wrote, except where a test hands it over
(the prepared segments for advance(), the state of an update for the float64 evaluation of that update's targets)."""
import numpy as np

PATH, MOVETO = 0, 1
CURVE_IN, CURVE_OUT, STATION = 0, 1, 2
EASE_LINEAR, EASE_SMOOTHSTEP = 0, 1
ORIENT_ALONG_PATH = 1
MAX_WAYPOINTS, MAX_SEGMENTS_PER_UPDATE = 128, 64
ST_BODY_GONE, ST_LEADER_GONE, ST_OVERRUN, ST_POS_ACTIVE, ST_ROT_ACTIVE = 1, 2, 4, 8, 16
INVALID = 0xFFFFFFFF
DERIVED = ("segment_len", "just_curve_len", "entry_segment_len", "curve_angle", "curve_r")


# ---- vectors as tuples of scalars of one dtype: every operation below rounds once, in the order it is written ------------------------------------------
def v_add(a, b): return tuple(x + y for x, y in zip(a, b))
def v_sub(a, b): return tuple(x - y for x, y in zip(a, b))
def v_scale(a, s): return tuple(x * s for x in a)
def v_dot(a, b): return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]
def v_len(a): return np.sqrt(v_dot(a, a))
def v_dist(a, b): return v_len(v_sub(a, b))


def v_normalise(a):
    with np.errstate(invalid="ignore", divide="ignore"):
        l = v_len(a)
        return tuple(x / l for x in a)


def cmin(a, b): return a if a < b else b                              # myMin / myMax as the library writes them (a NaN takes the same side)
def cmax(a, b): return a if a > b else b
def clamp(x, lo, hi): return cmax(lo, cmin(x, hi))                    # myClamp
def lerp(a, b, t): return a * (type(t)(1) - t) + b * t                # Maths::lerp / uncheckedLerp
def v_lerp(a, b, t): return tuple(lerp(x, y, t) for x, y in zip(a, b))


def smoothstep01(x):
    T = type(x)
    s = clamp((x - T(0)) / (T(1) - T(0)), T(0), T(1))
    return (s * s) * (T(3) - T(2) * s)


def q_mul(p, q):
    px, py, pz, pw = p
    qx, qy, qz, qw = q
    return (((pw * qx + px * qw) + py * qz) - pz * qy, ((pw * qy - px * qz) + py * qw) + pz * qx,
            ((pw * qz + px * qy) - py * qx) + pz * qw, ((pw * qw - px * qx) - py * qy) - pz * qz)


class Seg:
    """One sgp_path_segment in dtype T."""
    __slots__ = ("pos", "type", "pause_time", "speed", "segment_len", "just_curve_len", "entry_segment_len", "curve_angle", "curve_r", "exit_dir")


def segs_from_array(arr, T):
    """abi.path_segment_dtype records -> Seg objects of dtype T (fp32 values are exact in float64)."""
    out = []
    for r in arr:
        s = Seg()
        s.pos = tuple(T(x) for x in r["pos"]); s.type = int(r["type"]); s.pause_time = T(r["pause_time"]); s.speed = T(r["speed"])
        for k in DERIVED:
            setattr(s, k, T(r[k]))
        s.exit_dir = tuple(T(x) for x in r["exit_segment_unit_dir"])
        out.append(s)
    return out


def wp(segs, i): return segs[i % len(segs)].pos                       # waypointPos (Python's % is the non-negative remainder)


def prepare(waypoints, T):
    """waypoints: [(pos, type, pause_time, speed)] in fp32 values.  -> (segs, total_time as a Python float) or None where the library refuses."""
    n = len(waypoints)
    if n < 2 or n > MAX_WAYPOINTS:
        return None
    segs = []
    for pos, typ, pause, speed in waypoints:
        vals = [np.float32(x) for x in pos] + [np.float32(pause), np.float32(speed)]
        if not all(np.isfinite(v) for v in vals) or not np.float32(speed) > 0 or not np.float32(pause) >= 0 or typ not in (CURVE_IN, CURVE_OUT, STATION):
            return None
        s = Seg()
        s.pos = tuple(T(np.float32(x)) for x in pos); s.type = typ; s.pause_time = T(np.float32(pause)); s.speed = T(np.float32(speed))
        for k in DERIVED:
            setattr(s, k, T(0))
        s.exit_dir = (T(0), T(0), T(0))
        segs.append(s)
    if any(v_dist(wp(segs, i), wp(segs, i + 1)) < T(np.float32(1.0e-5)) for i in range(n)):
        return None
    total = 0.0
    for i, w in enumerate(segs):
        entry_pos, exit_pos = wp(segs, i), wp(segs, i + 1)
        entry_dir = v_normalise(v_sub(entry_pos, wp(segs, i - 1)))
        exit_dir = v_normalise(v_sub(wp(segs, i + 2), exit_pos))
        if w.type == CURVE_IN:
            angle = np.arccos(clamp(v_dot(entry_dir, exit_dir), T(-1), T(1)))
            if angle < T(np.float32(1.0e-6)):
                w.segment_len = v_dist(entry_pos, exit_pos); w.just_curve_len = T(0); w.entry_segment_len = v_dist(entry_pos, exit_pos)
                w.curve_angle = T(0); w.curve_r = T(1000)
                w.exit_dir = v_normalise(v_sub(exit_pos, entry_pos))
            else:
                a, b, c, d = entry_pos, entry_dir, exit_pos, exit_dir
                bd = v_dot(b, d)
                with np.errstate(invalid="ignore", divide="ignore"):
                    t = (v_dot(v_sub(c, a), b) + v_dot(v_sub(a, c), d) * bd) / (T(1) - bd * bd)
                    p = v_add(a, v_scale(b, t))
                    entry_to_p, exit_to_p = v_dist(p, entry_pos), v_dist(p, exit_pos)
                    dd = cmin(entry_to_p, exit_to_p)
                    curve_r = dd / np.tan(angle / T(2))
                    curve_len = angle * curve_r
                    entry_len, exit_len = cmax(entry_to_p - dd, T(0)), cmax(exit_to_p - dd, T(0))
                    w.segment_len = (curve_len + entry_len) + exit_len; w.just_curve_len = curve_len; w.entry_segment_len = entry_len
                    w.curve_angle = angle; w.curve_r = curve_r
                    w.exit_dir = v_normalise(v_sub(exit_pos, p))
        else:
            w.segment_len = v_dist(entry_pos, exit_pos)
        vals = [getattr(w, k) for k in DERIVED] + list(w.exit_dir)
        if not all(np.isfinite(v) for v in vals) or w.segment_len < T(np.float32(1.0e-5)):
            return None
        total += float(w.segment_len / w.speed)
        if w.type == STATION:
            total += float(w.pause_time)
    return segs, total


def advance(segs, state, dt, max_ends=MAX_SEGMENTS_PER_UPDATE):
    """walkAlongPathForTime's state change.  state = (index, dist, time) -> (index, dist, time, status)."""
    idx, dist, time = state
    T = type(dist)
    rem = T(dt)
    n, ends, status = len(segs), 0, 0
    while rem > 0:
        w = segs[idx]
        vel = w.speed
        travelled = time
        if w.type == STATION:
            if time < w.pause_time:
                stop = w.pause_time - time
                if rem < stop:
                    time = time + rem
                    break
                rem = rem - stop
                time = time + stop
            travelled = time - w.pause_time
        seg_rem = w.segment_len / vel - travelled
        if rem < seg_rem:
            dist = dist + rem * vel
            time = time + rem
            break
        rem = rem - seg_rem
        dist, time = T(0), T(0)
        idx = (idx + 1) % n
        ends += 1
        if ends >= max_ends:
            status |= ST_OVERRUN
            break
    return idx, dist, time, status


def eval_state(segs, idx, dist, seen=None):
    """Position and direction at `dist` along segment `idx`.  seen: a set that collects the branch taken."""
    T = type(dist)
    w = segs[idx]
    entry_pos, exit_pos = wp(segs, idx), wp(segs, idx + 1)
    entry_dir = v_normalise(v_sub(entry_pos, wp(segs, idx - 1)))
    note = seen.add if seen is not None else (lambda b: None)
    if w.type == CURVE_IN:
        ex = w.exit_dir
        if dist < w.entry_segment_len:
            note("equal_dirs" if w.curve_angle == 0 else "entry")
            return v_add(entry_pos, v_scale(entry_dir, dist)), entry_dir
        if dist < w.entry_segment_len + w.just_curve_len:
            note("arc")
            frac = (dist - w.entry_segment_len) / w.just_curve_len
            comp = v_sub(ex, v_scale(entry_dir, v_dot(ex, entry_dir)))      # removeComponentInDir
            orthog = v_normalise(comp)
            angle = frac * w.curve_angle
            sn, cs = np.sin(angle), np.cos(angle)
            pos = v_add(v_add(entry_pos, v_scale(entry_dir, w.entry_segment_len)),
                        v_add(v_scale(v_scale(entry_dir, w.curve_r), sn), v_scale(v_scale(orthog, w.curve_r), T(1) - cs)))
            return pos, v_add(v_scale(entry_dir, cs), v_scale(orthog, sn))
        note("exit")
        return v_sub(exit_pos, v_scale(ex, w.segment_len - dist)), ex
    frac = dist / w.segment_len
    pos = v_lerp(entry_pos, exit_pos, frac)
    end_dir = v_normalise(v_sub(exit_pos, entry_pos))
    if w.type == CURVE_OUT:
        note("curve_out")
        return pos, end_dir
    note("station")
    return pos, v_lerp(entry_dir, end_dir, smoothstep01(frac + T(0.5)) * T(2) - T(1))


def eval_backwards(segs, idx, dist, delta, max_starts=MAX_SEGMENTS_PER_UPDATE, seen=None):
    """evalAlongPathDistBackwards -> (pos, dir, index, dist, status)."""
    T = type(dist)
    delta = T(delta)
    starts = 0
    while True:
        if delta < dist:
            dist = dist - delta
            break
        delta = delta - dist
        idx = (idx - 1) % len(segs)
        dist = segs[idx].segment_len
        starts += 1
        if starts >= max_starts:
            entry_pos = wp(segs, idx)
            if seen is not None:
                seen.add("back_overrun")
            return entry_pos, v_normalise(v_sub(entry_pos, wp(segs, idx - 1))), idx, T(0), ST_OVERRUN
    if seen is not None:
        seen.add("back_%s" % ("0" if starts == 0 else "1" if starts == 1 else "many"))
    pos, d = eval_state(segs, idx, dist, seen)
    return pos, d, idx, dist, 0


def path_rotation(base_rot, flags, d):
    T = type(d[0])
    if not flags & ORIENT_ALONG_PATH:
        return base_rot
    a = np.arctan2(d[1], d[0])
    return q_mul((T(0), T(0), np.sin(T(0.5) * a), np.cos(T(0.5) * a)), base_rot)


def slerp(a, b, t, seen=None):
    T = type(t)
    c = ((a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]) + a[3] * b[3]
    if c < 0:
        b = tuple(-x for x in b)
        c = -c
        if seen is not None:
            seen.add("slerp_neg")
    if c > T(np.float32(0.9995)):
        r = tuple(lerp(x, y, t) for x, y in zip(a, b))
        l = np.sqrt(((r[0] * r[0] + r[1] * r[1]) + r[2] * r[2]) + r[3] * r[3])
        return tuple(x / l for x in r)
    theta = np.arccos(clamp(c, T(-1), T(1)))
    tp = theta * t
    p = tuple(y - x * c for x, y in zip(a, b))
    pl = np.sqrt(((p[0] * p[0] + p[1] * p[1]) + p[2] * p[2]) + p[3] * p[3])
    p = tuple(x / pl for x in p)
    cs, sn = np.cos(tp), np.sin(tp)
    return tuple(x * cs + y * sn for x, y in zip(a, p))


def easing(frac, kind): return smoothstep01(frac) if kind == EASE_SMOOTHSTEP else frac


class Track:
    """One track of a move-to mover.  The clock is float32 (the contract's state); value() evaluates in any dtype from that clock."""

    def __init__(self, start, target, duration, ease, cur_elapsed):
        F = np.float32
        self.start, self.target = tuple(F(x) for x in start), tuple(F(x) for x in target)
        self.duration = cmax(F(duration), F(1.0e-4))
        self.ease, self.elapsed, self.active = ease, cmax(F(cur_elapsed), F(0)), True

    def advance(self, dt, seen=None):
        self.elapsed = self.elapsed + np.float32(dt)
        if self.elapsed >= self.duration:
            self.active = False
            if seen is not None:
                seen.add("track_done")
                if self.elapsed - np.float32(dt) > self.duration:
                    seen.add("elapsed_beyond_duration")

    def value(self, T, rotation, seen=None):
        frac = clamp(T(self.elapsed) / T(self.duration), T(0), T(1))
        e = easing(frac, self.ease)
        if seen is not None:
            seen.add("ease_%d" % self.ease)
        a, b = tuple(T(x) for x in self.start), tuple(T(x) for x in self.target)
        return slerp(a, b, e, seen) if rotation else v_lerp(a, b, e)


class Sim:
    """A batch restated.  States are float32 (the contract's); targets() evaluates position, rotation and direction of the last update in float32 or
    float64 from that float32 state.  paths: name -> (abi.path_segment_dtype array as the library prepared it, its traversal time)."""

    def __init__(self, paths):
        self.paths = {k: {np.float32: segs_from_array(a, np.float32), np.float64: segs_from_array(a, np.float64), "total": t} for k, (a, t) in paths.items()}
        self.m = []

    def add(self, spec, pos_tracks=(), rot_tracks=()):
        import math
        F = np.float32
        m = dict(update_index=0, status=0, ran=False, removed=False, body_gone=False, leader_gone=False, idx=0, dist=F(0), time=F(0), pos_track=None, rot_track=None)
        if spec[0] == "path":
            _, name, t0, leader, follow, flags, base = spec
            m.update(kind=PATH, path=name, leader=leader, follow=F(follow), flags=flags, base=tuple(F(x) for x in base))
            if leader is None:
                total = self.paths[name]["total"]
                t = math.fmod(t0, total)
                if t < 0:
                    t += total
                segs = self.paths[name][F]
                m["idx"], m["dist"], m["time"], _ = advance(segs, (0, F(0), F(0)), F(t), max_ends=len(segs) + 1)
        else:
            _, pi, ri, hold_pos, hold_rot = spec
            m.update(kind=MOVETO, leader=None, held={T: [tuple(T(F(x)) for x in hold_pos), tuple(T(F(x)) for x in hold_rot)] for T in (np.float32, np.float64)})
            if pi is not None:
                m["pos_track"] = Track(*pos_tracks[pi])
            if ri is not None:
                m["rot_track"] = Track(*rot_tracks[ri])
        self.m.append(m)
        return len(self.m) - 1

    def remove(self, k):
        self.m[k]["removed"] = True
        for f in self.m:
            if f["leader"] == k:
                f["leader_gone"] = True

    def update(self, dt, seen=None):
        """The states after one update, in float32.  m["ran"]: whether the mover wrote its body."""
        F = np.float32
        for m in self.m:      # walkers and move-to movers
            m["ran"] = False
            if m["removed"] or m["body_gone"] or (m["kind"] == PATH and m["leader"] is not None):
                continue
            m["status"] = 0
            if m["kind"] == PATH:
                before = m["idx"]
                segs = self.paths[m["path"]][F]
                m["idx"], m["dist"], m["time"], m["status"] = advance(segs, (m["idx"], m["dist"], m["time"]), F(dt))
                if seen is not None:
                    ends = (m["idx"] - before) % len(segs)
                    seen.add("overrun" if m["status"] & ST_OVERRUN else "several_ends" if ends > 1 else "one_end" if ends == 1 else "no_end")
                    if segs[m["idx"]].type == STATION and m["time"] < segs[m["idx"]].pause_time:
                        seen.add("paused")
            else:
                tp, tr = m["pos_track"], m["rot_track"]
                m["ran_pos"], m["ran_rot"] = bool(tp and tp.active), bool(tr and tr.active)
                if not m["ran_pos"] and not m["ran_rot"]:
                    if seen is not None:
                        seen.add("moveto_finished")
                    continue
                if m["ran_pos"]:
                    tp.advance(dt, seen)
                if m["ran_rot"]:
                    tr.advance(dt, seen)
            m["ran"] = True
            m["update_index"] += 1
        for m in self.m:      # followers, from what their leaders published in this update
            if m["removed"] or m["body_gone"] or m["kind"] != PATH or m["leader"] is None:
                continue
            m["ran"] = True
            m["update_index"] += 1
            m["time"] = F(0)
            if m["leader_gone"] or self.m[m["leader"]]["body_gone"]:
                m["idx"], m["dist"], m["status"] = 0, F(0), ST_LEADER_GONE
            else:
                lead = self.m[m["leader"]]
                m["lead"] = (lead["idx"], lead["dist"])
                _, _, m["idx"], m["dist"], m["status"] = eval_backwards(self.paths[m["path"]][F], lead["idx"], lead["dist"], m["follow"], seen=seen)

    def targets(self, T, seen=None):
        """[(pos, rot, dir) or None] of the last update, evaluated in T."""
        out = []
        for m in self.m:
            if not m["ran"]:
                out.append(None)
                continue
            if m["kind"] == MOVETO:
                held = m["held"][T]
                if m["ran_pos"]:
                    held[0] = m["pos_track"].value(T, False, seen)
                if m["ran_rot"]:
                    held[1] = m["rot_track"].value(T, True, seen)
                out.append((held[0], held[1], (T(0), T(0), T(0))))
                continue
            segs = self.paths[m["path"]][T]
            if m["leader"] is None:
                pos, d = eval_state(segs, m["idx"], T(m["dist"]), seen)
            elif m["status"] & ST_LEADER_GONE:
                pos, d = wp(segs, 0), (T(1), T(0), T(0))
            else:
                pos, d, _, _, _ = eval_backwards(segs, m["lead"][0], T(m["lead"][1]), T(m["follow"]), seen=seen)
            out.append((pos, path_rotation(tuple(T(x) for x in m["base"]), m["flags"], d), d))
        return out


# ---- MotionProperties::MoveKinematic as CMD_MOVE_KINEMATIC has it (sgp_dev_edits.h) ---------------------------------------------------------------------
def _acos01(x):
    T = type(x)
    xc = clamp(x, T(0), T(1))
    p = T(np.float32(-0.0187293))
    p = p * xc + T(np.float32(0.0742610))
    p = p * xc - T(np.float32(0.2121144))
    p = p * xc + T(np.float32(1.5707288))
    return p * np.sqrt(T(1) - xc)


def _quat_angle(sl, w):
    T = type(sl)
    if sl < T(0.25):
        x2 = sl * sl
        c = [T(np.float32(v)) for v in (0.16666667, 0.075, 0.044642857, 0.030381944)]
        return T(2) * (sl * (T(1) + x2 * (c[0] + x2 * (c[1] + x2 * (c[2] + x2 * c[3])))))
    w = clamp(w, T(-1), T(1))
    return T(2) * (_acos01(w) if w >= 0 else T(np.float32(3.14159265358979)) - _acos01(-w))


def move_kinematic(pos, rot, tpos, trot, dt):
    """-> (linear velocity, angular velocity) that take (pos, rot) to (tpos, trot) in dt."""
    T = type(pos[0])
    dt = T(dt)
    lv = v_scale(v_sub(tpos, pos), T(1) / dt)
    dq = q_mul(trot, (-rot[0], -rot[1], -rot[2], rot[3]))
    if dq[3] < 0:
        dq = tuple(-x for x in dq)
    sl = np.sqrt(dq[0] * dq[0] + dq[1] * dq[1] + dq[2] * dq[2])
    av = (T(0), T(0), T(0))
    if sl > T(np.float32(1.0e-12)):
        av = v_scale((dq[0] / sl, dq[1] / sl, dq[2] / sl), _quat_angle(sl, dq[3]) / dt)
    return lv, av
