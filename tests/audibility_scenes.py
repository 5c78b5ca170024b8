"""Scenes for the audio sources' GPU tests: a row of walls, behind it a field of sources -- POINT sources, sources on static spheres and boxes, on kinematic
boxes that sgp_movers slide over the field and on falling dynamic spheres --, listeners on a scripted polyline on both sides of the walls.  The sources'
positions are computed HERE from the bodies' reported poses and the shapes (spheres and identity-rotation boxes: centre -+ extent, exact in float32, then
the centroid of those bounds), the occlusion answers are sgp_raycast's to the rays the restatement built itself.  Rig drives a batch and the restatement of
tests/audibility_reference.py side by side and compares masks, distances, factors and events."""
import numpy as np

from substrata_amd import abi, scenes
import audibility_reference as ar

F32 = np.float32
DT = 1.0 / 60.0
SPACING = 3.0
SPARE = 4            # source slots a rig has beyond its field
MAX_MOVING = 16      # kinematic boxes, and as many dynamic spheres, whatever the size of the field
N_WALLS = 10
ALL_WANTS = abi.AUD_WANT_RANGE | abi.AUD_WANT_OCCLUSION | abi.AUD_WANT_VOLUME


def new_world(**kw):
    from substrata_amd.lib import World
    return World(**kw)


def walls():
    """A row of wall segments with 2 m gaps along y = 7, between the first leg of the walk and the field, and one wall across the field."""
    d = scenes._blank(N_WALLS + 1)
    d["pos"][:N_WALLS, 0] = -20.0 + 6.0 * np.arange(N_WALLS); d["pos"][:N_WALLS, 1] = 7.0; d["pos"][:N_WALLS, 2] = 2.5
    d["shape"][:N_WALLS, :3] = (2.0, 0.2, 2.5)
    d["pos"][N_WALLS] = (13.5, 16.5, 2.5); d["shape"][N_WALLS, :3] = (0.2, 6.0, 2.5)
    return d


def field(n):
    """(what every source slot is, the body descs of the BODY sources): slot j is a POINT source where j % 4 == 0, else it sits on a body."""
    j = np.arange(n)
    side = int(np.ceil(np.sqrt(n)))
    pos = np.zeros((n, 3), F32)
    pos[:, 0] = (j % side) * SPACING; pos[:, 1] = 9.0 + (j // side) * SPACING; pos[:, 2] = 1.0 + 0.5 * (j % 3)
    is_body = j % 4 != 0
    kin = np.nonzero(j % 16 == 7)[0][:MAX_MOVING]
    dyn = np.nonzero(j % 16 == 10)[0][:MAX_MOVING]
    sphere = (j % 4 == 1) | np.isin(j, dyn)      # (the falling ones are spheres: their bounds are exact whatever they do)
    d = scenes._blank(n)
    d["pos"] = pos
    d["shape_type"] = np.where(sphere, abi.SHAPE_SPHERE, abi.SHAPE_BOX)
    d["shape"][:] = 0
    d["shape"][:, :3] = np.where(sphere[:, None], np.stack([0.3 + 0.1 * (j % 3)] * 3, 1), np.array([(0.4, 0.5, 0.3)]))
    d["shape"][sphere, 1:3] = 0.0
    d["motion_type"][kin] = abi.MOTION_KINEMATIC
    d["motion_type"][dyn] = abi.MOTION_DYNAMIC
    for m in (kin, dyn):
        d["layer"][m] = abi.LAYER_MOVING
        d["activate"][m] = 1
    d["pos"][dyn, 2] = 3.0
    d["pos"][kin, 2] = 4.0      # above the field: they slide over it
    half = np.where(sphere[:, None], np.repeat(d["shape"][:, :1], 3, 1), d["shape"][:, :3]).astype(F32)
    return pos, is_body, d, half, kin, dyn


def walk(k, u):
    """Listener k's position at update u: a polyline in front of the walls, round their end and over the field, each listener on a line of its own."""
    t = 2.5 * u + 3.0 * (k % 8)
    legs = [((-25.0, 4.0), (1.0, 0.0), 50.0), ((25.0, 4.0), (0.0, 1.0), 30.0), ((25.0, 34.0), (-0.6, 0.8), 1e9)]
    for (x0, y0), (dx, dy), length in legs:
        if t <= length:
            return np.array((x0 + dx * t, y0 + dy * t + 2.0 * (k // 8), 2.75), F32)      # (above the static sources, below the sliding boxes)
        t -= length
    raise AssertionError


def times(n_updates, seed=3):
    """cur_time of every update: irregular steps"""
    rng = np.random.default_rng(seed)
    return 100.0 + np.cumsum(rng.choice([0.016, 0.033, 0.1, 0.25], n_updates) * rng.uniform(0.7, 1.3, n_updates))


def records(ev):
    """Drained events as the tuples the restatement makes, with the tag and the update index."""
    return [(int(e["kind"]), int(e["source"]), int(e["listener"]), int(e["factor"].view(np.uint32)), int(e["tag"]), int(e["update_index"])) for e in ev]


class Rig:
    """A world with the walls and the field, the batch over it, movers for the kinematic boxes, and the restatement next to it."""

    def __init__(self, n, n_listeners, event_capacity=1 << 16, listener_capacity=None):
        self.n, self.L = n, n_listeners
        self.lcap = n_listeners if listener_capacity is None else listener_capacity
        self.w = new_world(max_bodies=n + 64)
        self.w.add_batch(scenes.ground())
        self.w.add_batch(walls())
        self.pos, self.is_body, d, self.half, self.kin, self.dyn = field(n)
        self.capacity = n + SPARE
        self.body = np.full(self.capacity, abi.INVALID_ID, np.uint32)      # the body a source slot sits on
        self.body_half = np.zeros((self.capacity, 3), F32)
        slots = np.flatnonzero(self.is_body)
        if len(slots):
            self.body[slots] = self.w.add_batch(d[slots])
            self.body_half[slots] = self.half[slots]
        self.movers = None
        if len(self.kin):
            self.movers = self.w.movers(len(self.kin), 1)
            for s in self.kin:
                p = d["pos"][s]
                m = self.movers.add_moveto_mover(int(self.body[s]), p)
                self.movers.set_position_track(m, p, p + np.array((12.0, 6.0, 0.0), F32), 0.5, abi.MOVER_EASE_LINEAR, 0.0)
        self.ab = self.w.audibility(self.capacity, self.lcap, event_capacity)
        self.model = ar.AudibilityModel(self.capacity, self.lcap)
        j = np.arange(n)
        self.point = np.zeros((self.capacity, 3), F32); self.point[:n] = self.pos
        self.volume = np.zeros(self.capacity, F32); self.volume[:n] = np.array((0.1, 0.2, 0.35, 0.5), F32)[j % 4]
        self.key = np.full(self.capacity, abi.INVALID_ID, np.uint32); self.key[:n] = np.where(j % 5 == 0, abi.INVALID_ID, np.where(self.pos[:, 0] < 15, 40, 20))
        self.flags = np.zeros(self.capacity, np.uint32); self.flags[:n] = ALL_WANTS
        self.flags[:n][j % 8 == 6] |= abi.AUD_ONE_SHOT
        self.flags[:n][j % 32 == 9] = 0
        self.flags[:n][j % 32 == 11] = abi.AUD_WANT_VOLUME
        self.tags = np.zeros(self.capacity, np.uint64); self.tags[:n] = 5000 + j
        if n > 4:
            self.point[4] = walk(0, 10) + np.array((0.25, 0.0, 0.0), F32)      # POINT: a quarter of a metre from listener 0 at update 10
        if n >= 63:
            self.point[8] = (95.0, 4.0, 2.75); self.volume[8] = 2.0             # POINT: in range from more than 61 m away
        if n > 1000:                                                            # the far end of a large field reaches the walk
            for s in (n - 1, n - 2, n - 3, AUD_FAR):
                self.volume[s] = F32(np.linalg.norm(self.pos[s] - walk(0, 20)) / 60.0 * 1.25)
                self.flags[s] = ALL_WANTS
        self.alive = np.zeros(self.capacity, bool); self.alive[:n] = True
        desc = np.zeros(n, dtype=abi.audibility_source_dtype)
        desc["kind"] = np.where(self.is_body, abi.AUD_SRC_BODY, abi.AUD_SRC_POINT); desc["body"] = np.where(self.is_body, self.body[:n], 0)
        desc["pos"] = self.point[:n]; desc["volume"] = self.volume[:n]; desc["zone_key"] = self.key[:n]; desc["flags"] = self.flags[:n]; desc["tag"] = self.tags[:n]
        ids = self.ab.add(desc)
        assert np.array_equal(ids, j)
        # listeners: 1 rides the first kinematic box (and ignores it); the others walk
        self.rider = None
        self.lst_key = np.full(self.lcap, abi.INVALID_ID, np.uint32); self.lst_mute = np.zeros(self.lcap, bool); self.lst_live = np.zeros(self.lcap, bool)
        self.lst_ignore = np.full(self.lcap, abi.INVALID_ID, np.uint32)
        for k in range(n_listeners):
            key, mute = (40, True) if k == 2 else ((20, False) if k else (abi.INVALID_ID, False))
            if k == 1 and len(self.kin):
                self.rider = (int(self.body[self.kin[0]]), np.array((0.0, 0.0, 1.5), F32))
                self.ab.set_listener(k, body=self.rider[0], offset=self.rider[1], ignore_body=self.rider[0], zone_key=key, mute_outside=mute)
                self.lst_ignore[k] = self.rider[0]
            else:
                self.ab.set_listener(k, pos=walk(k, 0), zone_key=key, mute_outside=mute)
            self.lst_key[k], self.lst_mute[k], self.lst_live[k] = key, mute, True
        self.u = 0
        self.body_there = self.body != abi.INVALID_ID
        self.max_near_miss = 0.0

    def source_positions(self):
        """Every slot's position: the POINT sources' own, and for a BODY source the centroid of the bounds the device has for the body."""
        out = self.point.copy()
        slots = np.flatnonzero(self.body_there)
        if len(slots):
            st = self.w.get_state(self.body[slots])
            boxes = self.body_half[slots, 1] != self.body_half[slots, 0]
            assert np.array_equal(st["rot"][boxes], np.tile(np.array((0, 0, 0, 1), F32), (int(boxes.sum()), 1)))      # the boxes' bounds are exact only unrotated
            mn, mx = st["pos"] - self.body_half[slots], st["pos"] + self.body_half[slots]
            out[slots] = (mn + mx) * F32(0.5)
        return out

    def listener_positions(self):
        out = np.zeros((self.lcap, 3), F32)
        for k in range(self.lcap):
            if not self.lst_live[k]:
                continue
            if k == 1 and self.rider is not None:
                out[k] = self.w.get_state([self.rider[0]])[0]["pos"] + self.rider[1]
            else:
                out[k] = walk(k, self.u)
        return out

    def any_hit(self, origins, dirs, max_ts, listeners):
        """sgp_raycast's answer to the restatement's rays; also the condition that no closest hit lies within 1e-3 of a ray's end."""
        rays = np.zeros(len(origins), dtype=abi.ray_dtype)
        rays["origin"], rays["dir"], rays["max_t"] = origins, dirs, max_ts
        rays["ignore_id"] = self.lst_ignore[listeners]
        hit = self.w.raycast(rays)["id"] != abi.INVALID_ID
        longer = rays.copy(); longer["max_t"] = max_ts + F32(2e-3)
        h = self.w.raycast(longer)
        near = (h["id"] != abi.INVALID_ID) & (np.abs(h["t"] - max_ts) <= 1e-3)
        assert not near.any(), (self.u, np.flatnonzero(near)[:4], h["t"][near][:4], max_ts[near][:4])
        return hit

    def frame(self, cur_time, transition=1.0, check=True):
        """Movers, a step, the listeners moved, one update on both sides; returns the restatement's events of the update with tag and update index."""
        if self.movers is not None:
            self.movers.update(DT)
        self.w.step(DT)
        pl = self.listener_positions()
        for k in range(self.lcap):
            if self.lst_live[k] and not (k == 1 and self.rider is not None):
                self.ab.set_listener_points(k, pl[k])
        self.ab.update(cur_time)
        src_live = self.alive & ((self.body == abi.INVALID_ID) | self.body_there)
        u = self.model.update_index
        ev = self.model.update(self.source_positions(), src_live, self.volume, self.key, self.flags, pl, self.lst_live, self.lst_key, self.lst_mute, cur_time, transition, self.any_hit)
        self.u += 1
        if check:
            self.check_states()
        return [(k, s, l, f, int(self.tags[s]), u) for k, s, l, f in ev]

    def set_listener_zone(self, k, key, mute):
        self.ab.set_listener_zone(k, key, mute)
        self.lst_key[k], self.lst_mute[k] = key, mute

    def check_states(self):
        st = self.ab.states(0, self.capacity)
        pr = self.ab.pair_states(0, self.capacity)
        m = self.model
        live = self.alive[:, None] & self.lst_live[None, :]
        bit = (1 << np.arange(self.lcap, dtype=np.uint64)).astype(np.uint32)
        want_in = (np.where(m.in_range & live, bit[None, :], 0).sum(axis=1)).astype(np.uint32)
        want_occ = (np.where(m.occluded & live, bit[None, :], 0).sum(axis=1)).astype(np.uint32)
        assert np.array_equal(st["in_range_mask"], want_in), (self.u, np.flatnonzero(st["in_range_mask"] != want_in)[:8])
        assert np.array_equal(st["occluded_mask"], want_occ), (self.u, np.flatnonzero(st["occluded_mask"] != want_occ)[:8])
        want_dist = np.where(live, m.dist, F32(0)).astype(F32); want_fac = np.where(live, m.ramp["factor"], F32(1)).astype(F32)
        assert np.array_equal(pr["dist"].view(np.uint32), want_dist.view(np.uint32)), (self.u, np.argwhere(pr["dist"] != want_dist)[:8])
        assert np.array_equal(pr["mute_volume_factor"].view(np.uint32), want_fac.view(np.uint32)), (self.u, np.argwhere(pr["mute_volume_factor"] != want_fac)[:8])
        bits = np.where(m.in_range & live, abi.AUD_PAIR_IN_RANGE, 0) | np.where(m.occluded & live, abi.AUD_PAIR_OCCLUDED, 0)
        assert np.array_equal(pr["bits"], bits.astype(np.uint32)), self.u
        return st, pr

    def check_drain(self, want):
        ev, dropped = self.ab.drain_events()
        got = records(ev)
        assert dropped == 0 and len(got) == len(want), (self.u, len(got), len(want), dropped)
        for i, (g, x) in enumerate(zip(got, want)):
            assert g == x, (self.u, i, g, x)
        return got

    def close(self):
        self.ab.close()
        if self.movers is not None:
            self.movers.close()
        self.w.close()


AUD_FAR = 8191      # a slot in the middle of a large field, with the last three: far from the walk, their volume reaches it
