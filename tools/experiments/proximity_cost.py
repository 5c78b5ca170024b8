"""What an update of the proximity watchers costs: 1 k, 100 k and 2^20 watched objects (static boxes on a grid, radius 20) against 1 and 32 observers, in two
regimes -- steady (the observers stand still: no transition, no event; also with one object's record edited before every update, which uploads the whole
record mirror again) and flipping (the observers jump between the field and far away: every near bit in range
changes every update) -- next to the algorithmic bytes per object of docs/KERNELS.md and the bandwidth they imply, and next to the host loop the batch replaces:
ScriptedObjectProximityChecker::think restated over the bodies' bounds READ BACK from the device every frame (the read-back is part of it: the bounds live on the
device), vectorised with numpy -- a C++ loop over the same arrays would be faster than numpy for small n and slower for none of the sizes that matter.
One process, wall clock around work that ends in a wait, medians after a warm-up.
PYTHONPATH=. python tools/experiments/proximity_cost.py [updates = 30] [markdown file to append to]"""
import ctypes as C
import json
import sys
import time

import numpy as np

from substrata_amd import abi, scenes
from substrata_amd.lib import World

F32 = np.float32
# docs/KERNELS.md, "Batched proximity": steady state, per object slot
BYTES_STEADY = 16 + 8 + 4 + 32 + 4.0 / 256      # record, state, body flags, two bounds; one count per workgroup
# every bit flips: the state is written back (8), the event words are written and read again (16 + 16), the tag is read (8), an event record per wanted transition and observer (32)
def bytes_flipping(k):
    return BYTES_STEADY + 8 + 32 + 8 + 32.0 * k


def scene(n):
    w = World(max_bodies=n + 16)
    d = scenes._blank(n)
    side = int(np.ceil(np.sqrt(n)))
    j = np.arange(n)
    d["pos"] = np.column_stack([3.0 * (j % side), 3.0 * (j // side), np.full(n, 1.0)])
    bodies = np.asarray(w.add_batch(d), dtype=np.uint32)
    w.step(1.0 / 60.0)
    return w, bodies, 3.0 * side


def observers(k, side, inside):
    """k observers spread over the field's diagonal, or all far away from it."""
    t = (np.arange(k) + 0.5) / k
    p = np.column_stack([t * side, t * side, np.full(k, 1.7)]).astype(F32)
    return p if inside else p + F32(1.0e5)


def raised_events(w, px):
    """Events raised since the last drain (held + dropped), nothing copied."""
    n, dropped = C.c_uint32(0), C.c_uint32(0)
    w._check(w._fn("proximity_drain_events")(px._h, None, 0, C.byref(n), C.byref(dropped)), "proximity_drain_events")
    return int(n.value) + int(dropped.value)


def batch_times(w, bodies, side, k, updates, flipping, edit=False):
    n = len(bodies)
    px = w.proximity(n, 4, n * k + 64 if flipping else 1024)
    # flipping: the radius spans the field, so every object is in range of every observer standing in it and of none that is away
    px.add(bodies, 4.0 * side if flipping else 20.0, abi.PROX_WANT_NEAR)
    for o in range(k):
        px.set_observer(o, pos=observers(k, side, True)[o])
    px.update()
    raised_events(w, px)             # (the first update's NEAR events are not part of either regime)
    enqueue, done, events = [], [], 0
    for u in range(updates + 5):
        if flipping:
            px.set_points(0, observers(k, side, u % 2 == 1))
        if edit:
            px.set_flags(0, abi.PROX_WANT_NEAR)      # one record changes: the next update uploads the whole record mirror again (16 B per object slot)
        px.states(0, 1)
        t0 = time.perf_counter()
        px.update()
        t1 = time.perf_counter()
        px.states(0, 1)              # (a wait: the update has run)
        t2 = time.perf_counter()
        enqueue.append(t1 - t0); done.append(t2 - t0)
        events = max(events, raised_events(w, px))
    px.close()
    med = lambda a: float(np.median(a[5:]))
    return med(enqueue), med(done), events


def host_loop_times(w, bodies, side, k, updates):
    """think() on the host over bounds pulled back from the device: read the body states, centre -+ half extent, the near test per observer, compare with the stored bits."""
    n = len(bodies)
    obs = observers(k, side, True)
    half = np.full((n, 3), 0.5, F32)
    in_proximity = np.zeros((k, n), bool)
    r2 = F32(20.0) * F32(20.0)
    read, total = [], []
    for u in range(updates + 3):
        t0 = time.perf_counter()
        pos = w.read_states(int(bodies[0]), n)["pos"]
        t1 = time.perf_counter()
        mn, mx = pos - half, pos + half
        fired = 0
        for o in range(k):
            d = obs[o] - np.minimum(np.maximum(obs[o], mn), mx)
            near = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2] < r2
            fired += int(np.count_nonzero(near != in_proximity[o]))
            in_proximity[o] = near
        t2 = time.perf_counter()
        read.append(t1 - t0); total.append(t2 - t0)
    med = lambda a: float(np.median(a[3:]))
    return med(read), med(total)


if __name__ == "__main__":
    updates = int(sys.argv[1]) if len(sys.argv) > 1 else 30
    out = open(sys.argv[2], "a") if len(sys.argv) > 2 else None
    rows = []
    for n in (1000, 100000, 1 << 20):
        w, bodies, side = scene(n)
        for k in (1, 32):
            se, sd, sev = batch_times(w, bodies, side, k, updates, False)
            assert sev == 0, sev
            ee, ed, _ = batch_times(w, bodies, side, k, updates, False, edit=True)
            fe, fd, fev = batch_times(w, bodies, side, k, updates, True)
            assert fev == n * k, (fev, n * k)
            hr, ht = host_loop_times(w, bodies, side, k, updates if n < (1 << 20) else 6)
            row = {"objects": n, "observers": k, "steady_enqueue_ms": round(se * 1e3, 4), "steady_until_done_ms": round(sd * 1e3, 4),
                   "steady_bytes_per_object": round(BYTES_STEADY, 2), "steady_implied_GBps": round(n * BYTES_STEADY / sd / 1e9, 1),
                   "edited_enqueue_ms": round(ee * 1e3, 4), "edited_until_done_ms": round(ed * 1e3, 4),
                   "flipping_until_done_ms": round(fd * 1e3, 4), "flipping_events_per_update": fev, "flipping_bytes_per_object": round(bytes_flipping(k), 1),
                   "flipping_implied_GBps": round(n * bytes_flipping(k) / fd / 1e9, 1), "host_loop_readback_ms": round(hr * 1e3, 4), "host_loop_total_ms": round(ht * 1e3, 4)}
            rows.append(row)
            print(json.dumps(row), flush=True)
        w.close()
    if out:
        out.write("| objects | observers | steady: call returns | steady: until done | B/object | implied GB/s | one record edited: call returns | until done | flipping: until done | events/update | B/object | implied GB/s | host loop: read-back | host loop: total |\n")
        out.write("|---|---|---|---|---|---|---|---|---|---|---|---|---|---|\n")
        for r in rows:
            out.write("| %d | %d | %.3f ms | %.3f ms | %.1f | %.1f | %.3f ms | %.3f ms | %.3f ms | %d | %.0f | %.1f | %.3f ms | %.3f ms |\n" % (
                r["objects"], r["observers"], r["steady_enqueue_ms"], r["steady_until_done_ms"], r["steady_bytes_per_object"], r["steady_implied_GBps"], r["edited_enqueue_ms"], r["edited_until_done_ms"], r["flipping_until_done_ms"],
                r["flipping_events_per_update"], r["flipping_bytes_per_object"], r["flipping_implied_GBps"], r["host_loop_readback_ms"], r["host_loop_total_ms"]))
        out.close()
