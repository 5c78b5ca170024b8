"""What sgp_cast_shapes costs (profiles/shape_casts.md is this script's output).  The config 3 pile, settled; 1, 256 and 4096 casts of each shape type along the
same paths -- from 3 m above the pile's bounds down and sideways into it, 1 to 4 m long --; host wall time per call, median of 20 calls after 3 warm-ups, with
the spread.  The yardstick is sgp_spherecast on the same paths with the radii of the sphere-typed casts.
    PYTHONPATH=. python tools/experiments/shape_cast_cost.py [settle_steps] [calls] > profiles/shape_casts.md"""
import sys
import time

import numpy as np

from substrata_amd import abi, scenes
from substrata_amd.lib import World

DT = 1.0 / 60.0
NS = (1, 256, 4096)
KINDS = (("sphere", abi.SHAPE_SPHERE), ("box", abi.SHAPE_BOX), ("capsule", abi.SHAPE_CAPSULE), ("hull", abi.SHAPE_HULL))


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
    w = World(max_bodies=131072)
    hull = w.hull_create(np.random.default_rng(8).normal(size=(10, 3)) * 0.45).hull_id
    w.add_batch(scenes.config3_100k_mixed())
    for _ in range(settle):
        w.step(DT)
    st = w.read_states(1, 100000)
    p = st["pos"][st["id"] != abi.INVALID_ID]
    lo = np.percentile(p, 2, axis=0); hi = np.percentile(p, 98, axis=0)
    rng = np.random.default_rng(1)
    rows = []
    for n in NS:
        start = rng.uniform(lo, hi, size=(n, 3)); start[:, 2] = hi[2] + 3.0
        d = np.column_stack([rng.uniform(-0.6, 0.6, n), rng.uniform(-0.6, 0.6, n), -np.ones(n)])
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        max_t = rng.uniform(1.0, 4.0, n) + 3.0
        q = rng.normal(size=(n, 4)); q /= np.linalg.norm(q, axis=1, keepdims=True)
        radii = rng.uniform(0.3, 0.6, n).astype(np.float32)
        rays = np.zeros(n, dtype=abi.ray_dtype)
        rays["origin"] = start; rays["dir"] = d; rays["max_t"] = max_t; rays["ignore_id"] = abi.INVALID_ID
        base = timed(lambda: w.spherecast(rays, radii), calls)
        base_hits = int((w.spherecast(rays, radii)["id"] != abi.INVALID_ID).sum())
        for name, kind in KINDS:
            c = np.zeros(n, dtype=abi.shape_cast_dtype)
            c["pos"] = start; c["rot"] = q; c["dir"] = d; c["max_t"] = max_t; c["ignore_id"] = abi.INVALID_ID; c["shape_type"] = kind
            if kind == abi.SHAPE_SPHERE:
                c["shape"][:, 0] = radii
            elif kind == abi.SHAPE_BOX:
                c["shape"][:, :3] = rng.uniform(0.25, 0.6, size=(n, 3))
            elif kind == abi.SHAPE_CAPSULE:
                c["shape"][:, 0] = 0.3; c["shape"][:, 1] = 0.65
            else:
                c["shape"][:, 0] = hull
            t = timed(lambda: w.cast_shapes(c), calls)
            hits = int((w.cast_shapes(c)["id"] != abi.INVALID_ID).sum())
            rows.append((n, name, t, hits, base, base_hits))
    capped, reruns = w.cast_shapes_counters()
    w.close()
    print("## Shape casts into the settled config 3 pile\n")
    print(f"Host wall time per call in ms: median of {calls} calls after 3 warm-ups (min - max).  Yardstick: sgp_spherecast on the same paths with the sphere casts' radii.\n")
    print("| n | shape | sgp_cast_shapes | hits | sgp_spherecast | hits | ratio of medians |")
    print("|---|---|---|---|---|---|---|")
    for n, name, t, hits, base, base_hits in rows:
        print(f"| {n} | {name} | {t[0]:.3f} ({t[1]:.3f} - {t[2]:.3f}) | {hits} | {base[0]:.3f} ({base[1]:.3f} - {base[2]:.3f}) | {base_hits} | {t[0] / base[0]:.2f} |")
    print(f"\nPairs that ran into the iteration cap: {capped}; runs repeated for a larger candidate list: {reruns}.")


if __name__ == "__main__":
    main()
