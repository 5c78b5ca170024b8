"""Height field (F) against the triangle mesh of the same samples (M), in one process, rounds alternating F and M: host create time, device bytes,
step and narrow-phase time on a terrain scene, batched rays, sphere casts, capsule queries and a step with cars (wheel casts).  Prints one markdown table.

    python tools/experiments/heightfield_bench.py [--mesh-only] [--rounds 5]

--mesh-only: M alone, for A/B runs of the triangle-mesh path against another build of the library (SGP_LIB_PATH)."""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from substrata_amd import abi, scenes                                             # noqa: E402
from substrata_amd.lib import World                                               # noqa: E402
from heightfield_scenes import heightfield_triangulation, chunk_params, mesh_body, ROT_X90   # noqa: E402
from helpers import add_car                                                       # noqa: E402

DT = 1.0 / 60.0
NARROWPHASE_STAGE = abi.STAGE_NAMES.index("narrowphase")


def heights(w, seed=1):
    z, x = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    return (1.5 * np.sin(0.05 * x) * np.cos(0.043 * z) + 0.3 * np.sin(0.31 * x + 0.2 * z)).astype(np.float32)


def make_shape(w, kind, h, quad_w):
    off, sp = chunk_params(h.shape[0], quad_w)
    t0 = time.perf_counter()
    if kind == "F":
        info = w.heightfield_create(h, off, sp)
    else:
        V, T, _ = heightfield_triangulation(h, off, sp)
        t0 = time.perf_counter()
        info = w.mesh_create(V, T)
    return info, time.perf_counter() - t0


def shape_bytes(w):
    c = abi.BodyCounts()
    w._check(w._fn("world_body_counts")(w._h, C.byref(c)), "world_body_counts")
    return int(c.shape_bytes)


def timed(fn, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter(); fn(); ts.append(time.perf_counter() - t0)
    return float(np.median(ts)) * 1e3


def scene_round(kind, n_bodies=5000, W=257, quad_w=1.0, steps=40):
    w = World(max_bodies=n_bodies + 512)
    h = heights(W)
    info, _ = make_shape(w, kind, h, quad_w)
    w.add_batch(mesh_body(info.mesh_id))
    rng = np.random.default_rng(3)
    d = scenes.dynamic_bodies(n_bodies)
    k = rng.integers(0, 3, n_bodies)
    d["shape_type"] = k; d["shape"][:, :3] = 0.3; d["shape"][k == 2, 1] = 0.3; d["shape"][k == 2, 0] = 0.2
    span = quad_w * (W - 1)
    d["pos"] = np.column_stack([rng.uniform(2, span - 2, n_bodies), rng.uniform(2, span - 2, n_bodies), rng.uniform(2.5, 4.0, n_bodies)])
    w.add_batch(d)
    for _ in range(60):
        w.step(DT)
    t_step = timed(lambda: w.step(DT), steps)
    np_ms = float(np.median([w.step_profiled(DT).stage_ms[NARROWPHASE_STAGE] for _ in range(10)]))
    rays = np.zeros(2048, dtype=abi.ray_dtype)
    rays["origin"] = np.column_stack([rng.uniform(0, span, 2048), rng.uniform(0, span, 2048), rng.uniform(6, 12, 2048)])
    dd = rng.normal(size=(2048, 3)) * (0.5, 0.5, 0.2) + (0, 0, -1.0)
    rays["dir"] = dd / np.linalg.norm(dd, axis=1, keepdims=True); rays["max_t"] = 60.0; rays["ignore_id"] = abi.INVALID_ID
    t_ray = timed(lambda: w.raycast(rays), 20)
    t_ray1 = timed(lambda: w.raycast(rays[:1]), 50)
    radii = np.full(2048, 0.3, np.float32)
    t_sc = timed(lambda: w.spherecast(rays, radii), 20)
    qy = np.zeros(64, dtype=abi.capsule_query_dtype)
    qy["pos"] = np.column_stack([rng.uniform(2, span - 2, 64), rng.uniform(2, span - 2, 64), np.full(64, 2.5)])
    qy["rot"] = (0, 0, 0, 1); qy["radius"] = 0.3; qy["half_height"] = 0.6; qy["max_separation"] = 0.1; qy["ignore_id"] = abi.INVALID_ID; qy["collidable_only"] = 1
    t_cap = timed(lambda: w.collide_capsules(qy), 20)
    w.close()
    # cars: 64 vehicles (four wheel casts each per step) on the same terrain
    w = World(max_bodies=1024)
    info, _ = make_shape(w, kind, h, quad_w)
    w.add_batch(mesh_body(info.mesh_id))
    for i in range(64):
        _, vid = add_car(w, pos=(10.0 + 28.0 * (i % 8), 10.0 + 28.0 * (i // 8), 4.0))
        w.vehicle_set_input(vid, 0.5, 0.0, 0.0, 0.0)
    for _ in range(60):
        w.step(DT)
    t_car = timed(lambda: w.step(DT), steps)
    w.close()
    return dict(step=t_step, narrowphase=np_ms, rays=t_ray, ray1=t_ray1, spherecast=t_sc, capsules=t_cap, cars=t_car)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mesh-only", action="store_true")
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    kinds = ["M"] if a.mesh_only else ["F", "M"]
    res = {k: [] for k in kinds}
    for r in range(a.rounds):
        for k in (kinds if r % 2 == 0 else kinds[::-1]):
            res[k].append(scene_round(k))
    print("| kind | metric | median ms | min ms |")
    print("|---|---|---|---|")
    for k in kinds:
        for m in res[k][0]:
            v = np.array([x[m] for x in res[k]])
            print(f"| {k} | {m} | {np.median(v):.4f} | {v.min():.4f} |")
    # host create time and device bytes, W = 128 (the reference's chunk) and 512
    if not a.mesh_only:
        print()
        print("| W | F create ms | M create ms | F shape bytes | M shape bytes |")
        print("|---|---|---|---|---|")
        for W in (128, 512):
            h = heights(W)
            out = {}
            for k in ("F", "M"):
                ts = []
                for _ in range(3):
                    w = World(max_bodies=64)
                    _, t = make_shape(w, k, h, 1.0)
                    ts.append(t * 1e3)
                    out[k + "b"] = shape_bytes(w)
                    w.close()
                out[k] = min(ts)
            print(f"| {W} | {out['F']:.2f} | {out['M']:.2f} | {out['Fb']} | {out['Mb']} |")


if __name__ == "__main__":
    main()
