"""What an update of the audio sources' batch costs: 256, 4 096 and 100 000 POINT sources on a 3 m grid crossed by rows of walls, against 1 and 32 listeners
standing on the field's diagonal, the sources' volume chosen so that about a tenth of the pairs are in range (every one of them is traced in every update, as
the reference traces every source in range every frame; nothing moves, so no event is raised) -- next to the algorithmic bytes per source of docs/KERNELS.md,
and next to the route the library had before: the host loop of GUIClient.cpp:6973-7034 with ONE sgp_raycast of n = 1 per traced pair (the resident ray
server answers them), the pairs' geometry vectorised with numpy and the mute ramps left out (both in the host loop's favour), the calls made through ctypes
on addresses computed beforehand.  Then sgp_raycast_any against sgp_raycast on the same 4 096 rays, in the walled half of a scene (hit-heavy) and in its open
half (miss-heavy).  One process, the two sides of every comparison alternating, wall clock around work that ends in a wait, medians of 30 repetitions after a
warm-up, in 5 blocks: the spread of a median is the range of its 5 block medians.
PYTHONPATH=. python tools/experiments/audibility_cost.py [repetitions = 30] [markdown file to append to]"""
import ctypes as C
import json
import sys
import time

import numpy as np

from substrata_amd import abi, scenes
from substrata_amd.lib import World

F32 = np.float32
BLOCKS = 5
# docs/KERNELS.md, "Batched audio sources": steady state.  Per source slot: record 32 + state 16 in, scratch 8 + position 16 out (k_aud_range), scratch 8 in
# (k_aud_list), scratch 8 in (k_aud_fold), four counts and offsets per 64 sources; a source with a traced pair adds record 32 + state 16 in and 16 out + position 16 in
# (k_aud_fold); a traced pair adds 4 (list, written) + 4 + 16 + 32 (list, position, record: k_aud_rays) + 4 (answer, written) + 4 (answer, read) + 32 + 32 (pair, read and written)
BYTES_SOURCE, BYTES_TRACED_SOURCE, BYTES_PAIR = 32 + 16 + 8 + 16 + 8 + 8 + 16.0 / 64, 32 + 16 + 16 + 16, 4 + 4 + 16 + 32 + 4 + 4 + 32 + 32


def scene(n):
    """n POINT sources on a 3 m grid, a row of wall segments (8 m long, 2 m gaps) every 12 m."""
    side = int(np.ceil(np.sqrt(n)))
    length = 3.0 * side
    rows = np.arange(4.5, length, 12.0)
    cols = np.arange(4.0, length + 8.0, 10.0)
    w = World(max_bodies=len(rows) * len(cols) + 64)
    w.add_batch(scenes.ground())
    d = scenes._blank(len(rows) * len(cols))
    gx, gy = np.meshgrid(cols, rows, indexing="ij")
    d["pos"][:, 0], d["pos"][:, 1], d["pos"][:, 2] = gx.ravel(), gy.ravel(), 2.5
    d["shape"][:, :3] = (4.0, 0.2, 2.5)
    w.add_batch(d)
    w.step(1.0 / 60.0)
    j = np.arange(n)
    pos = np.column_stack([3.0 * (j % side), 3.0 * (j // side), np.full(n, 1.5)]).astype(F32)
    return w, pos, length


def listeners(k, length):
    t = (np.arange(k) + 0.5) / k
    return np.column_stack([0.2 * length + 0.6 * t * length, 0.25 * length + 0.5 * t * length + 1.0, np.full(k, 1.7)]).astype(F32)


def traced_pairs(pos, lst, volume):
    """(source, listener) of the pairs an update traces, and their rays (CONTRACT 4m steps 1 and 3), source-major."""
    d = pos[:, None, :] - lst[None, :, :]
    d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    maxd = F32(60.0) * F32(volume)
    dist = np.sqrt(d2, dtype=F32)
    s, l = np.nonzero((d2 <= maxd * maxd) & (dist < maxd))
    rays = np.zeros(len(s), dtype=abi.ray_dtype)
    rays["origin"] = lst[l]
    rays["dir"] = d[s, l] / dist[s, l, None]
    rays["max_t"] = np.minimum(np.maximum(dist[s, l] - F32(1.0), F32(0.0)), F32(60.0))
    rays["ignore_id"] = abi.INVALID_ID
    return s, l, rays


def median_and_spread(samples, reps):
    """samples: BLOCKS * reps values -> (median of the block medians, their range)"""
    m = [float(np.median(samples[b * reps:(b + 1) * reps])) for b in range(BLOCKS)]
    return float(np.median(m)), max(m) - min(m)


def update_cost(n, k, reps, compare_host):
    w, pos, length = scene(n)
    volume = 0.178 * length / 60.0                      # pi r^2 = a tenth of the field
    lst = listeners(k, length)
    ab = w.audibility(n, k, 1 << 20)
    ab.add_points(pos, volume=volume)
    for i in range(k):
        ab.set_listener(i, pos=lst[i])
    s, l, rays = traced_pairs(pos, lst, volume)
    fn, hits = w._fn("raycast"), np.zeros(1, dtype=abi.hit_dtype)
    addr = [rays.ctypes.data + i * rays.itemsize for i in range(len(rays))]
    hit_addr = hits.ctypes.data

    def host_loop():
        """the walk of :6973-7034 for the same pairs: the geometry (numpy), then one blocking ray per traced pair"""
        traced_pairs(pos, lst, volume)
        occluded = 0
        for a in addr:
            fn(w._h, a, 1, hit_addr)
            occluded += hits["id"][0] != abi.INVALID_ID
        return occluded

    for u in range(5):                                   # warm-up: the first update raises the IN_RANGE and OCCLUDED events
        ab.update(1.0 + 0.016 * u); ab.states(0, 1)
        if compare_host:
            host_occluded = host_loop()
    ev, dropped = ab.drain_events()
    occluded = int(np.count_nonzero(ev["kind"] == abi.AUD_EV["OCCLUDED"]))
    if compare_host:
        assert occluded == host_occluded, (occluded, host_occluded)
    enqueue, done, host = [], [], []
    for u in range(BLOCKS * reps):
        t0 = time.perf_counter()
        ab.update(2.0 + 0.016 * u)
        t1 = time.perf_counter()
        ab.states(0, 1)                                  # (a wait: the update has run)
        t2 = time.perf_counter()
        enqueue.append(t1 - t0); done.append(t2 - t0)
        if compare_host:
            t3 = time.perf_counter()
            host_loop()
            host.append(time.perf_counter() - t3)
    steady_events = len(ab.drain_events()[0])
    assert steady_events == 0, steady_events
    sources_traced = len(np.unique(s))
    row = {"sources": n, "listeners": k, "pairs_in_range_share": round(len(rays) / (n * k), 3), "rays_traced": len(rays), "occluded": occluded,
           "call_returns_ms": round(median_and_spread(enqueue, reps)[0] * 1e3, 4), "until_done_ms": round(median_and_spread(done, reps)[0] * 1e3, 4),
           "until_done_spread_ms": round(median_and_spread(done, reps)[1] * 1e3, 4),
           "bytes_per_source": round(BYTES_SOURCE + BYTES_TRACED_SOURCE * sources_traced / n + BYTES_PAIR * len(rays) / n, 1)}
    if compare_host:
        row["host_loop_ms"] = round(median_and_spread(host, reps)[0] * 1e3, 4)
        row["host_loop_spread_ms"] = round(median_and_spread(host, reps)[1] * 1e3, 4)
        row["host_us_per_ray"] = round(row["host_loop_ms"] * 1e3 / max(len(rays), 1), 2)
    ab.close(); w.close()
    return row


def any_against_closest(reps):
    """4 096 rays in the walled half of a 192 m field and 4 096 in its open half, each set given to both entry points in turn."""
    rng = np.random.default_rng(5)
    w, pos, length = scene(4096)
    w.close()
    rows, cols = np.arange(4.5, length, 12.0), np.arange(4.0, length + 8.0, 10.0)
    w = World(max_bodies=len(rows) * len(cols) + 1600)
    w.add_batch(scenes.ground())
    d = scenes._blank(len(rows) * len(cols))
    gx, gy = np.meshgrid(cols, rows, indexing="ij")
    d["pos"][:, 0], d["pos"][:, 1], d["pos"][:, 2] = gx.ravel(), gy.ravel(), 2.5
    d["shape"][:, :3] = (4.0, 0.2, 2.5)
    small = scenes._blank(1500)                          # small bodies over both halves: the cell walk has something to look at
    small["pos"] = rng.uniform([0, 0, 0.5], [2 * length, length, 4.0], size=(1500, 3)); small["shape"][:, :3] = 0.3
    w.add_batch(d); w.add_batch(small); w.step(1.0 / 60.0)
    out = []
    for name, x0 in (("walled half (hit-heavy)", 0.0), ("open half (miss-heavy)", length + 10.0)):
        a = rng.uniform([x0, 0, 0.5], [x0 + length - 10.0, length, 3.5], size=(4096, 3)).astype(F32)
        v = rng.normal(size=(4096, 3)) * (1, 1, 0.05); v /= np.linalg.norm(v, axis=1, keepdims=True)
        rays = np.zeros(4096, dtype=abi.ray_dtype)
        rays["origin"], rays["dir"], rays["max_t"], rays["ignore_id"] = a, v.astype(F32), rng.uniform(20, 60, 4096), abi.INVALID_ID
        closest, anyhit = w.raycast(rays), w.raycast_any(rays)
        assert np.array_equal(anyhit, closest["id"] != abi.INVALID_ID)
        tc, ta = [], []
        for u in range(5 + BLOCKS * reps):
            t0 = time.perf_counter(); w.raycast(rays); t1 = time.perf_counter(); w.raycast_any(rays); t2 = time.perf_counter()
            if u >= 5:
                tc.append(t1 - t0); ta.append(t2 - t1)
        out.append({"rays": name, "hit_share": round(float(anyhit.mean()), 3), "closest_hit_ms": round(median_and_spread(tc, reps)[0] * 1e3, 4),
                    "closest_hit_spread_ms": round(median_and_spread(tc, reps)[1] * 1e3, 4), "any_hit_ms": round(median_and_spread(ta, reps)[0] * 1e3, 4),
                    "any_hit_spread_ms": round(median_and_spread(ta, reps)[1] * 1e3, 4)})
    w.close()
    return out


if __name__ == "__main__":
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 30
    out = open(sys.argv[2], "a") if len(sys.argv) > 2 else None
    rows = []
    for n in (256, 4096, 100000):
        for k in (1, 32):
            row = update_cost(n, k, reps, compare_host=(n * k <= 4096 * 32 and (n <= 4096)))
            rows.append(row)
            print(json.dumps(row), flush=True)
    first = rows[0]
    margin = first["host_loop_ms"] - first["until_done_ms"]
    verdict = margin > first["host_loop_spread_ms"] + first["until_done_spread_ms"]
    print(json.dumps({"required": "batch until done below the host loop at 256 x 1 by more than the two spreads", "margin_ms": round(margin, 4), "holds": bool(verdict)}), flush=True)
    rays = any_against_closest(reps)
    for r in rays:
        print(json.dumps(r), flush=True)
    if out:
        out.write("| sources | listeners | pairs in range | rays traced | occluded | call returns | until done (spread) | B/source | host loop (spread) | host us/ray |\n|---|---|---|---|---|---|---|---|---|---|\n")
        for r in rows:
            host = "%.3f ms (%.3f)" % (r["host_loop_ms"], r["host_loop_spread_ms"]) if "host_loop_ms" in r else "not run"
            out.write("| %d | %d | %.1f %% | %d | %d | %.3f ms | %.3f ms (%.3f) | %.0f | %s | %s |\n" % (
                r["sources"], r["listeners"], 100 * r["pairs_in_range_share"], r["rays_traced"], r["occluded"], r["call_returns_ms"], r["until_done_ms"], r["until_done_spread_ms"],
                r["bytes_per_source"], host, ("%.2f" % r["host_us_per_ray"]) if "host_us_per_ray" in r else "-"))
        out.write("\nRequired: at 256 x 1 the batch's time until done is below the host loop's by more than the two spreads: margin %.3f ms, %s.\n\n" % (margin, "holds" if verdict else "DOES NOT HOLD"))
        out.write("| 4 096 rays | hit share | sgp_raycast (spread) | sgp_raycast_any (spread) |\n|---|---|---|---|\n")
        for r in rays:
            out.write("| %s | %.1f %% | %.3f ms (%.3f) | %.3f ms (%.3f) |\n" % (r["rays"], 100 * r["hit_share"], r["closest_hit_ms"], r["closest_hit_spread_ms"], r["any_hit_ms"], r["any_hit_spread_ms"]))
        out.close()
    sys.exit(0 if verdict else 1)
