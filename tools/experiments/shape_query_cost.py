"""What sgp_collide_shapes costs, and where its two organisations cross over (profiles/shape_queries.md is this script's output).
The config 3 pile, settled; box queries of 0.5 m half extent at random poses inside the pile; n = 1 .. 65536 under SGP_QUERY_PATH=wave, =pairs and
unset (the library's own choice); host wall time per call, median of 20 calls after 3 warm-ups, with the spread.  One more row: 4096 capsule
queries through sgp_collide_capsules and the same through sgp_collide_shapes.
    python tools/experiments/shape_query_cost.py [settle_steps] [calls] > profiles/shape_queries.md"""
import os
import sys
import time

import numpy as np

from substrata_amd import abi, scenes
from substrata_amd.lib import World

DT = 1.0 / 60.0
NS = (1, 64, 1024, 16384, 65536)
PATHS = ("wave", "pairs", None)


def settled_world(path, settle):
    os.environ.pop("SGP_QUERY_PATH", None)
    if path:
        os.environ["SGP_QUERY_PATH"] = path
    w = World(max_bodies=131072)
    os.environ.pop("SGP_QUERY_PATH", None)
    w.add_batch(scenes.config3_100k_mixed())
    for _ in range(settle):
        w.step(DT)
    return w


def quats(rng, n):
    q = rng.normal(size=(n, 4)); q /= np.linalg.norm(q, axis=1, keepdims=True)
    return q.astype(np.float32)


def box_queries(rng, n, lo, hi):
    q = np.zeros(n, dtype=abi.shape_query_dtype)
    q["pos"] = rng.uniform(lo, hi, size=(n, 3)); q["rot"] = quats(rng, n)
    q["shape_type"] = abi.SHAPE_BOX; q["shape"][:, :3] = 0.5; q["ignore_id"] = abi.INVALID_ID
    return q


def timed(fn, calls, warm=3):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(calls):
        t0 = time.perf_counter(); fn(); ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), min(ts), max(ts)


def main():
    settle = int(sys.argv[1]) if len(sys.argv) > 1 else 240
    calls = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    rows = {}; caps_row = {}; lo = hi = None
    for path in PATHS:
        w = settled_world(path, settle)
        if lo is None:
            st = w.read_states(1, 100000)
            p = st["pos"][st["id"] != abi.INVALID_ID]
            lo = np.percentile(p, 2, axis=0); hi = np.percentile(p, 98, axis=0)      # inside the pile
        rng = np.random.default_rng(1)
        for n in NS:
            q = box_queries(rng, n, lo, hi)
            cap = 1 << 21
            out = np.zeros(cap, dtype=abi.query_contact_dtype)
            import ctypes as C
            cnt = C.c_uint32(0)
            fn = lambda: w._check(w._fn("collide_shapes")(w._h, q.ctypes.data, n, out.ctypes.data, cap, C.byref(cnt)), "collide_shapes")
            med, mn, mx = timed(fn, calls)
            rows[(n, path)] = (med, mn, mx, cnt.value)
        # 4096 capsules: the existing entry point against the new one, in the same world
        n = 4096
        cq = np.zeros(n, dtype=abi.capsule_query_dtype)
        cq["pos"] = rng.uniform(lo, hi, size=(n, 3)); cq["rot"] = quats(rng, n); cq["radius"] = 0.3; cq["half_height"] = 0.65
        cq["max_separation"] = 0.05; cq["ignore_id"] = abi.INVALID_ID; cq["collidable_only"] = 1
        sq = np.zeros(n, dtype=abi.shape_query_dtype)
        for f in ("pos", "rot", "max_separation", "ignore_id"):
            sq[f] = cq[f]
        sq["shape_type"] = abi.SHAPE_CAPSULE; sq["shape"][:, 0] = 0.3; sq["shape"][:, 1] = 0.65; sq["layer_mask"] = 0x3
        cap = 1 << 18
        a = timed(lambda: w.collide_capsules(cq, cap=cap), calls)
        na = len(w.collide_capsules(cq, cap=cap))
        b = timed(lambda: w.collide_shapes(sq, cap=cap), calls)
        nb = w.collide_shapes(sq, cap=cap)[1]
        caps_row[path] = (a, na, b, nb)
        w.close()

    name = lambda p: p or "unset"
    print("## Box queries (half extent 0.5 m, random poses inside the settled config 3 pile)\n")
    print(f"Host wall time per call in ms: median of {calls} calls after 3 warm-ups (min - max).\n")
    print("| n | " + " | ".join(f"SGP_QUERY_PATH={name(p)}" for p in PATHS) + " | contacts | unset vs faster forced |")
    print("|---|" + "---|" * (len(PATHS) + 2))
    for n in NS:
        cells = [f"{rows[(n, p)][0]:.3f} ({rows[(n, p)][1]:.3f} - {rows[(n, p)][2]:.3f})" for p in PATHS]
        counts = {rows[(n, p)][3] for p in PATHS}
        best = min(("wave", "pairs"), key=lambda p: rows[(n, p)][0])
        u, f = rows[(n, None)], rows[(n, best)]
        verdict = "within the spread" if u[1] <= f[2] else "SLOWER beyond the spread"
        print(f"| {n} | " + " | ".join(cells) + f" | {'/'.join(map(str, sorted(counts)))} | {verdict} (faster: {best}) |")
    print("\n## 4096 capsule queries: sgp_collide_capsules against sgp_collide_shapes (same queries, same world)\n")
    print("| world | sgp_collide_capsules | sgp_collide_shapes | contacts |")
    print("|---|---|---|---|")
    for p in PATHS:
        a, na, b, nb = caps_row[p]
        print(f"| SGP_QUERY_PATH={name(p)} | {a[0]:.3f} ({a[1]:.3f} - {a[2]:.3f}) | {b[0]:.3f} ({b[1]:.3f} - {b[2]:.3f}) | {na} / {nb} |")


if __name__ == "__main__":
    main()
