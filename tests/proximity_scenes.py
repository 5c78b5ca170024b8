"""Scenes for the proximity watchers' GPU tests: a field of static spheres and boxes, kinematic boxes on sgp_movers tracks and falling dynamic spheres, with the
bodies' bounds computed HERE from the shapes (spheres and identity-rotation boxes: centre -+ extent, exact in float32); observers on a scripted polyline; three
overlapping zones.  Rig drives a batch and the restatement of tests/proximity_reference.py side by side and compares masks and events after every update."""
import numpy as np

from substrata_amd import abi, scenes
import proximity_reference as pr

F32 = np.float32
DT = 1.0 / 60.0
SPACING = 3.0
SPARE = 8            # object slots a rig has beyond its field
MAX_MOVING = 48      # kinematic boxes, and as many dynamic spheres, whatever the size of the field


def new_world(**kw):
    from substrata_amd.lib import World
    return World(**kw)


def field(n):
    """n body descs on a grid in the plane, SPACING apart, and for each its half extent (3,) as the device's bounds have it."""
    d = scenes._blank(n)
    side = int(np.ceil(np.sqrt(n)))
    j = np.arange(n)
    d["pos"][:, 0] = (j % side) * SPACING
    d["pos"][:, 1] = (j // side) * SPACING
    d["pos"][:, 2] = 1.0
    sphere = j % 2 == 0
    d["shape_type"] = np.where(sphere, abi.SHAPE_SPHERE, abi.SHAPE_BOX)
    d["shape"][:, :3] = np.where(sphere[:, None], np.stack([0.5 + 0.25 * (j % 3)] * 3, 1), np.array([(0.5, 1.0, 0.75)]))
    d["shape"][sphere, 1:3] = 0.0
    kin = np.nonzero(j % 16 == 5)[0][:MAX_MOVING]
    dyn = np.nonzero(j % 16 == 10)[0][:MAX_MOVING]      # (even: spheres -- their bounds are exact whatever they do)
    d["motion_type"][kin] = abi.MOTION_KINEMATIC
    d["motion_type"][dyn] = abi.MOTION_DYNAMIC
    for m in (kin, dyn):
        d["layer"][m] = abi.LAYER_MOVING
        d["activate"][m] = 1
    d["pos"][dyn, 2] = 3.0
    d["pos"][kin, 2] = 4.0      # above the field: they slide over it
    half = np.where(sphere[:, None], np.repeat(d["shape"][:, :1], 3, 1), d["shape"][:, :3]).astype(F32)
    return d, half, kin, dyn


def walk(k, u):
    """Observer k's position at update u: a polyline over the near corner of the field, each observer on a line of its own."""
    t = 2.5 * u + 3.0 * (k % 8)
    legs = [((-25.0, 4.0), (1.0, 0.0), 50.0), ((25.0, 4.0), (0.0, 1.0), 30.0), ((25.0, 34.0), (-0.6, 0.8), 1e9)]
    for (x0, y0), (dx, dy), length in legs:
        if t <= length:
            return np.array((x0 + dx * t, y0 + dy * t + 2.0 * (k // 8), 1.7), F32)
        t -= length
    raise AssertionError


# three overlapping zones over the near corner, and a strip along the field's first column that runs its whole length: the observers start in it, and its
# objects (one per row, so one in nearly every workgroup of a large field) raise ENTERED and EXITED when they enter and leave it
ZONES = [((-10.0, -5.0, -1.0), (20.0, 30.0, 8.0), 40), ((10.0, -5.0, -1.0), (40.0, 30.0, 8.0), 20), ((15.0, 20.0, -1.0), (45.0, 60.0, 8.0), 30),
         ((-30.0, -5.0, -1.0), (1.6, 1000.0, 8.0), 50)]
FAR_SLOTS = (16384, 16385, 32768, 32769, 49152, 65535)      # with the last three slots of the field: objects far from the walk whose radius reaches it


def far_slots(n):
    """Slots of a large field that get a radius as long as their distance to the middle of the walk: the observers cross it one after the other, so NEAR and
    AWAY are raised from workgroups all over the grid of the test launch, the last one included."""
    return sorted({j for j in FAR_SLOTS + (n - 3, n - 2, n - 1) if 1000 <= j < n})


def records(ev):
    """Drained events as the tuples the restatement makes."""
    return [(int(e["kind"]), int(e["object"]), int(e["observer"]), int(e["zone_key"]), int(e["tag"]), int(e["update_index"])) for e in ev]


class Rig:
    """A world with the field, the batch over it, movers for the kinematic boxes, and the restatement next to it."""

    def __init__(self, n, n_observers, event_capacity=1 << 16, rider=True, radius=None):
        self.n, self.K = n, n_observers
        self.w = new_world(max_bodies=n + 64)
        self.w.add_batch(scenes.ground())
        d, self.half, self.kin, self.dyn = field(n)
        self.bodies = np.asarray(self.w.add_batch(d), dtype=np.uint32)
        self.first = int(self.bodies[0])
        assert np.array_equal(self.bodies, self.first + np.arange(n))      # (read_states below takes them as one range)
        self.is_box = d["shape_type"] == abi.SHAPE_BOX
        self.movers = None
        if len(self.kin):
            self.movers = self.w.movers(len(self.kin), 1)
            for b in self.kin:
                p = d["pos"][b]
                m = self.movers.add_moveto_mover(int(self.bodies[b]), p)
                self.movers.set_position_track(m, p, p + np.array((12.0, 6.0, 0.0), F32), 0.5, abi.MOVER_EASE_LINEAR, 0.0)
        self.capacity = n + SPARE
        self.px = self.w.proximity(self.capacity, 8, event_capacity)
        self.sim = pr.Sim(self.capacity, event_capacity)
        self.extra = {}      # object slot beyond the field -> (body, half extent): what a test adds later
        j = np.arange(n)
        self.radius = (np.array((5.0, 20.0, 35.0), F32)[j % 3] if radius is None else np.full(n, radius, F32))
        self.flags = np.array((abi.PROX_WANT_NEAR, abi.PROX_WANT_ZONE, 3, 3), np.uint32)[j % 4]
        self.flags[j % 32 == 7] = 0
        if radius is None:
            for f in far_slots(n):
                self.radius[f] = F32(np.linalg.norm(d["pos"][f] - walk(0, 20)))
                self.flags[f] = 3
        self.tags = (1000 + j).astype(np.uint64)
        self.ids = self.px.add(self.bodies, self.radius, self.flags, self.tags)
        assert np.array_equal(self.ids, j)
        self.sim.add(self.ids, self.radius, self.flags, self.tags)
        self.zone_slot = []
        for mn, mx, key in ZONES:
            z = self.px.add_zone(mn, mx, key)
            self.sim.add_zone(z, mn, mx, key)
            self.zone_slot.append(z)
        self.rider = None
        for k in range(n_observers):
            if k == 1 and rider and len(self.kin):      # observer 1 rides the first kinematic box
                self.rider = (int(self.bodies[self.kin[0]]), np.array((0.0, 0.0, 1.5), F32))
                self.px.set_observer(k, body=self.rider[0], offset=self.rider[1])
            else:
                self.px.set_observer(k, pos=walk(k, 0))
            self.sim.set_observer(k)
        self.u = 0
        self.there = np.zeros(self.capacity, bool)
        self.there[:n] = True

    def bounds(self):
        """The objects' bounds from the bodies' poses as the world reports them and the shapes: what k_finalize / the edit flush left on the device."""
        st = self.w.read_states(self.first, self.n)
        boxes = self.is_box & self.there[:self.n]
        assert np.array_equal(st["rot"][boxes], np.tile(np.array((0, 0, 0, 1), F32), (int(boxes.sum()), 1)))      # the boxes' bounds are exact only unrotated
        pos = np.zeros((self.capacity, 3), F32)
        half = np.zeros((self.capacity, 3), F32)
        pos[:self.n], half[:self.n] = st["pos"], self.half
        for slot, (body, h) in self.extra.items():
            pos[slot], half[slot] = self.w.get_state([body])[0]["pos"], h
        return pos - half, pos + half, pos

    def positions(self, pos):
        out = {}
        for k in self.sim.obs:
            if k == 1 and self.rider is not None:
                out[k] = None if self.rider[0] is None else pos[self.rider[0] - self.first] + self.rider[1]
            else:
                out[k] = walk(k, self.u)
        return out

    def frame(self, check=True):
        """Movers, a step, the observers moved, one update on both sides; returns the restatement's events of the update."""
        if self.movers is not None:
            self.movers.update(DT)
        self.w.step(DT)
        mn, mx, pos = self.bounds()
        p = self.positions(pos)
        for k, v in p.items():
            if not (k == 1 and self.rider is not None):
                self.px.set_points(k, v)
        self.px.update()
        ev = self.sim.update(mn, mx, self.there, p)
        self.u += 1
        if check:
            self.check_masks()
        return ev

    def check_masks(self):
        st = self.px.states(0, self.capacity)
        assert np.array_equal(st["near_mask"], self.sim.mask), (self.u, np.nonzero(st["near_mask"] != self.sim.mask)[0][:8])

    def check_drain(self):
        ev, dropped = self.px.drain_events()
        want, want_dropped = self.sim.drain()
        got = records(ev)
        self.last_dropped = dropped
        assert len(got) == len(want) and dropped == want_dropped, (self.u, len(got), len(want), dropped, want_dropped)
        for i, (g, x) in enumerate(zip(got, want)):
            assert g == x, (self.u, i, g, x)
        return got

    def close(self):
        self.px.close()
        if self.movers is not None:
            self.movers.close()
        self.w.close()
