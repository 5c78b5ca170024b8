"""docs/CONTRACT.md 4m restated in numpy: what one update of an audibility batch computes for every (source, listener) pair.  Written from the contract,
not from the C++: float32 arrays keep every fp32 operation in fp32 and in the contract's order, the ramp's times are float64.  The functions are
elementwise over arrays of one shape; AudibilityModel keeps the pair table of a batch and replays whole updates, asking the caller for the rays' answers."""
import numpy as np

F = np.float32
INVALID = 0xFFFFFFFF
ONE_SHOT, WANT_RANGE, WANT_OCCLUSION, WANT_VOLUME = 1, 2, 4, 8
EV_IN_RANGE, EV_OUT_OF_RANGE, EV_OCCLUDED, EV_UNOCCLUDED, EV_VOLUME = 1, 2, 3, 4, 5


def geometry(ps, pl, volume):
    """step 1: (dx, dy, dz, d2, maxd, max2), all float32.  ps, pl: (..., 3); volume: (...)."""
    ps, pl, volume = np.asarray(ps, F), np.asarray(pl, F), np.asarray(volume, F)
    dx, dy, dz = ps[..., 0] - pl[..., 0], ps[..., 1] - pl[..., 1], ps[..., 2] - pl[..., 2]
    d2 = (dx * dx + dy * dy) + dz * dz
    maxd = F(60.0) * volume
    max2 = maxd * maxd
    return dx, dy, dz, d2, maxd, max2


def range_step(in_range, d2, max2):
    """step 2: the pair leaves beyond max2, enters at or inside it."""
    leaves = in_range & (d2 > max2)
    enters = ~in_range & (d2 <= max2)
    return (in_range & ~leaves) | enters


def traced(in_range_now, d2, maxd):
    """step 3's test: (traced, dist); dist is 0 where the pair is not in range."""
    dist = np.where(in_range_now, np.sqrt(d2, dtype=F), F(0.0)).astype(F)
    return in_range_now & (dist < maxd), dist


def pair_ray(dx, dy, dz, dist):
    """the ray of a traced pair: unit direction (division by dist; (1, 0, 0) at dist == 0) and trace length min(max(dist - 1, 0), 60)."""
    zero = dist == 0
    safe = np.where(zero, F(1.0), dist).astype(F)
    d = np.stack([np.where(zero, F(1.0), dx / safe), np.where(zero, F(0.0), dy / safe), np.where(zero, F(0.0), dz / safe)], axis=-1).astype(F)
    trace = np.minimum(np.maximum(dist - F(1.0), F(0.0)), F(60.0)).astype(F)
    return d, trace


def fresh_ramp(shape):
    """the five ramp variables as AudioSource's constructor leaves them: factor, start time, end time, start factor, end factor"""
    return {"factor": np.ones(shape, F), "start": np.full(shape, -2.0), "end": np.full(shape, -1.0), "fac_start": np.ones(shape, F), "fac_end": np.ones(shape, F)}


def ramp_step(r, mute, cur_time, transition, sel=None):
    """startMuting where `mute`, startUnmuting elsewhere, then updateCurrentMuteVolumeFactor, on the elements `sel` of the ramp arrays `r` (in place).
    Returns factor != old (False outside sel)."""
    mute = np.asarray(mute, bool)
    sel = np.ones(mute.shape, bool) if sel is None else np.asarray(sel, bool)
    cur_time, transition = np.float64(cur_time), np.float64(transition)
    old = r["factor"].copy()
    m = sel & mute & (r["fac_end"] != 0)
    u = sel & ~mute & (r["fac_end"] != 1)
    end_m = cur_time + transition * r["factor"].astype(np.float64)
    end_u = cur_time + transition * (F(1.0) - r["factor"]).astype(np.float64)
    r["start"] = np.where(m | u, cur_time, r["start"])
    r["end"] = np.where(m, end_m, np.where(u, end_u, r["end"]))
    r["fac_start"] = np.where(m | u, r["factor"], r["fac_start"]).astype(F)
    r["fac_end"] = np.where(m, F(0.0), np.where(u, F(1.0), r["fac_end"])).astype(F)
    span = r["end"] - r["start"]
    ramping = (cur_time < r["end"]) & (span > 1.0e-4)
    with np.errstate(divide="ignore", invalid="ignore"):
        frac = (cur_time - r["start"]) / np.where(ramping, span, 1.0)
    mid = (r["fac_start"] + frac.astype(F) * (r["fac_end"] - r["fac_start"])).astype(F)
    r["factor"] = np.where(sel, np.where(ramping, mid, r["fac_end"]), r["factor"]).astype(F)
    return sel & (r["factor"] != old), {"muting_started": m, "unmuting_started": u, "ramping": sel & ramping}


class AudibilityModel:
    """The pair table of a batch of n source slots and L listener slots, and one update of it."""

    def __init__(self, n, L):
        self.n, self.L = n, L
        self.in_range = np.zeros((n, L), bool)
        self.occluded = np.zeros((n, L), bool)
        self.ramp = fresh_ramp((n, L))
        self.dist = np.zeros((n, L), F)
        self.update_index = 0
        self.stats = {"rays": 0, "dist_below_1": 0, "clamped_60": 0, "reversed": 0}

    def reset_source(self, s):
        self.in_range[s] = False; self.occluded[s] = False; self.dist[s] = 0
        f = fresh_ramp((self.L,))
        for k in f:
            self.ramp[k][s] = f[k]

    def reset_listener(self, l):
        self.in_range[:, l] = False; self.occluded[:, l] = False; self.dist[:, l] = 0
        f = fresh_ramp((self.n,))
        for k in f:
            self.ramp[k][:, l] = f[k]

    def update(self, src_pos, src_live, volume, src_key, flags, lst_pos, lst_live, lst_key, lst_mute, cur_time, transition, any_hit):
        """src_*: per source slot; lst_*: per listener slot; any_hit(origins, dirs, max_ts, listeners) -> bool per ray.  Returns the events of the update
        in their order as (kind, source, listener, factor bits)."""
        n, L = self.n, self.L
        live = np.asarray(src_live, bool)[:, None] & np.asarray(lst_live, bool)[None, :]
        ps = np.broadcast_to(np.asarray(src_pos, F)[:, None, :], (n, L, 3))
        pl = np.broadcast_to(np.asarray(lst_pos, F)[None, :, :], (n, L, 3))
        vol = np.broadcast_to(np.asarray(volume, F)[:, None], (n, L))
        dx, dy, dz, d2, maxd, max2 = geometry(ps, pl, vol)
        now = np.where(live, range_step(self.in_range, d2, max2), self.in_range)
        range_changed = now != self.in_range
        self.in_range = now
        tr, dist = traced(now & live, d2, maxd)
        idx = np.argwhere(tr)                                                   # source-major, then listener: the ray list's order
        occ_changed = np.zeros((n, L), bool)
        vol_changed = np.zeros((n, L), bool)
        if len(idx):
            s, l = idx[:, 0], idx[:, 1]
            dirs, trace = pair_ray(dx[s, l], dy[s, l], dz[s, l], dist[s, l])
            hit = np.asarray(any_hit(np.asarray(lst_pos, F)[l], dirs, trace, l), bool)
            occ_changed[s, l] = hit != self.occluded[s, l]
            self.occluded[s, l] = hit
            self.dist[s, l] = dist[s, l]
            ramped = tr & ((np.asarray(flags)[:, None] & ONE_SHOT) == 0)
            mute = np.asarray(lst_mute, bool)[None, :] & (np.asarray(src_key, np.uint32)[:, None] != np.asarray(lst_key, np.uint32)[None, :])
            before_end = self.ramp["fac_end"].copy(); before_factor = self.ramp["factor"].copy()
            vol_changed, what = ramp_step(self.ramp, mute, cur_time, transition, ramped)
            started = what["muting_started"] | what["unmuting_started"]
            self.stats["reversed"] += int((started & (before_factor != before_end)).sum())      # a flip while the factor was still on its way
            self.stats["rays"] += len(idx)
            self.stats["dist_below_1"] += int((dist[s, l] < 1).sum())
            self.stats["clamped_60"] += int((dist[s, l] - F(1.0) > 60).sum())
        fl = np.asarray(flags)[:, None]
        ev_r = range_changed & ((fl & WANT_RANGE) != 0)
        ev_o = occ_changed & ((fl & WANT_OCCLUSION) != 0)
        ev_v = vol_changed & ((fl & WANT_VOLUME) != 0)
        events = []
        for s, l in np.argwhere(ev_r | ev_o | ev_v):
            if ev_r[s, l]:
                events.append((EV_IN_RANGE if self.in_range[s, l] else EV_OUT_OF_RANGE, int(s), int(l), 0))
            if ev_o[s, l]:
                events.append((EV_OCCLUDED if self.occluded[s, l] else EV_UNOCCLUDED, int(s), int(l), 0))
            if ev_v[s, l]:
                events.append((EV_VOLUME, int(s), int(l), int(self.ramp["factor"][s, l].view(np.uint32))))
        self.update_index += 1
        return events
