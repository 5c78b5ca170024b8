"""The proximity and zone watchers restated in numpy float32 from docs/CONTRACT.md 4l (not from the header): the near test, the zone of an observer, and a whole
batch -- masks, observers' zones, the events of every update in their order, the event buffer with its drops.  The tests feed it the bodies' bounds as THEY compute
them from the shapes and the observers' positions; it never reads what the proximity kernels wrote."""
import numpy as np

F32 = np.float32
INVALID = 0xFFFFFFFF
WANT_NEAR, WANT_ZONE = 1, 2
NEAR, AWAY, EXITED, ENTERED = 1, 2, 3, 4
MAX_OBSERVERS = 32


def dist2(mn, mx, p):
    """mn, mx: (..., 3) float32 bounds; p: (3,) float32.  The squared distance from p to the closest point of the box, as 4l writes it."""
    mn, mx, p = np.asarray(mn, F32), np.asarray(mx, F32), np.asarray(p, F32)
    c = np.minimum(np.maximum(p, mn), mx)
    d = p - c
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def near(mn, mx, p, radius):
    radius = np.asarray(radius, F32)
    return dist2(mn, mx, p) < radius * radius


def contains(zmn, zmx, q):
    zmn, zmx, q = np.asarray(zmn, F32), np.asarray(zmx, F32), np.asarray(q, F32)
    return np.all((q >= zmn) & (q <= zmx), axis=-1)


def centroid(mn, mx):
    return (np.asarray(mn, F32) + np.asarray(mx, F32)) * F32(0.5)


def pick_zone(mins, maxs, keys, live, current, p):
    """Index of the zone an observer at p stands in, or INVALID: `current` if it is live and contains p, else the live zone of the lowest key that contains p."""
    n = len(keys)
    if current != INVALID and current < n and live[current] and contains(mins[current], maxs[current], p):
        return int(current)
    inside = [z for z in range(n) if live[z] and contains(mins[z], maxs[z], p)]
    return min(inside, key=lambda z: int(keys[z])) if inside else INVALID


class Sim:
    def __init__(self, capacity, event_capacity):
        self.radius = np.zeros(capacity, F32)
        self.flags = np.zeros(capacity, np.uint32)
        self.tag = np.zeros(capacity, np.uint64)
        self.alive = np.zeros(capacity, bool)
        self.mask = np.zeros(capacity, np.uint32)
        self.obs = {}        # k -> dict(zone=(slot, gen) or None, key, updates)
        self.zones = {}      # slot -> dict(mn, mx, key, gen, live)
        self.updates = 0
        self.event_capacity = event_capacity
        self.events, self.raised = [], 0      # held records (kind, object, observer, zone_key, tag, update_index); raised since the last drain

    # ---- the host's edits
    def add(self, ids, radius, flags, tags):
        ids = np.asarray(ids)
        self.radius[ids], self.flags[ids], self.tag[ids] = radius, flags, tags
        self.alive[ids], self.mask[ids] = True, 0

    def remove(self, i):
        self.alive[i], self.mask[i] = False, 0

    def set_observer(self, k):
        if k not in self.obs:
            self.obs[k] = dict(zone=None, key=INVALID, updates=0)

    def remove_observer(self, k):
        del self.obs[k]
        self.mask &= np.uint32(~(1 << k) & 0xFFFFFFFF)

    def add_zone(self, slot, mn, mx, key):
        gen = self.zones[slot]["gen"] + 1 if slot in self.zones else 1
        self.zones[slot] = dict(mn=np.asarray(mn, F32), mx=np.asarray(mx, F32), key=int(key), gen=gen, live=True)

    def remove_zone(self, slot):
        self.zones[slot]["live"] = False

    # ---- one update
    def _zone_live(self, z):
        return z is not None and self.zones[z[0]]["live"] and self.zones[z[0]]["gen"] == z[1]

    def update(self, mn, mx, there, positions):
        """mn, mx: (capacity, 3) float32 bounds of the objects' bodies; there: (capacity,) the body is still the one the object was added on; positions: observer ->
        (3,) float32, or None for an observer whose body has gone.  Returns the events of this update, in order (all of them, kept or dropped)."""
        if not self.alive.any() or not self.obs:
            return []
        mn, mx = np.asarray(mn, F32), np.asarray(mx, F32)
        run = np.asarray(self.alive & there)
        n = len(self.alive)
        out = []
        changed = np.zeros((n, MAX_OBSERVERS, 3), bool)      # [object][observer][NEAR or AWAY, EXITED, ENTERED]
        kinds = np.zeros((n, MAX_OBSERVERS), np.uint32)
        zkeys = {}
        q = centroid(mn, mx)
        for k in sorted(self.obs):
            o, p = self.obs[k], positions.get(k)
            if p is None:
                continue
            p = np.asarray(p, F32)
            old = o["zone"]
            old_live = self._zone_live(old)
            zone_changed = False
            if not (old_live and contains(self.zones[old[0]]["mn"], self.zones[old[0]]["mx"], p)):
                slots = sorted(self.zones)
                z = pick_zone([self.zones[s]["mn"] for s in slots], [self.zones[s]["mx"] for s in slots], [self.zones[s]["key"] for s in slots],
                              [self.zones[s]["live"] for s in slots], INVALID, p)
                new = None if z == INVALID else (slots[z], self.zones[slots[z]]["gen"])
                zone_changed = old is not None or new is not None
                if zone_changed:
                    want = run & ((self.flags & WANT_ZONE) != 0)
                    if old_live:
                        out.append((EXITED, INVALID, k, o["key"], 0, self.updates))
                        changed[:, k, 1] = want & contains(self.zones[old[0]]["mn"], self.zones[old[0]]["mx"], q)
                    if new is not None:
                        out.append((ENTERED, INVALID, k, self.zones[new[0]]["key"], 0, self.updates))
                        changed[:, k, 2] = want & contains(self.zones[new[0]]["mn"], self.zones[new[0]]["mx"], q)
                    zkeys[k] = (o["key"], self.zones[new[0]]["key"] if new is not None else INVALID)
                o["zone"], o["key"] = new, (self.zones[new[0]]["key"] if new is not None else INVALID)
            o["updates"] += 1
            o["pos"] = p
            bit = np.uint32(1 << k)
            was = (self.mask & bit) != 0
            now = near(mn, mx, p, self.radius)
            flip = run & (was != now)
            changed[:, k, 0] = flip & ((self.flags & WANT_NEAR) != 0)
            kinds[:, k] = np.where(now, NEAR, AWAY)
            self.mask = np.where(run, np.where(now, self.mask | bit, self.mask & ~bit), self.mask).astype(np.uint32)
        for j, k, r in zip(*np.nonzero(changed)):      # C order: object, observer, kind
            j, k, r = int(j), int(k), int(r)
            if r == 0:
                out.append((int(kinds[j, k]), j, k, INVALID, int(self.tag[j]), self.updates))
            else:
                out.append((EXITED if r == 1 else ENTERED, j, k, zkeys[k][r - 1], int(self.tag[j]), self.updates))
        room = max(self.event_capacity - self.raised, 0)
        self.events += out[:room]
        self.raised += len(out)
        self.updates += 1
        return out

    def drain(self):
        """(held records, dropped count) since the last drain."""
        ev, dropped = self.events, self.raised - len(self.events)
        self.events, self.raised = [], 0
        return ev, dropped
