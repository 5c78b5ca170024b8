"""What a world checkpoint costs: capture and rollback time of the lean path (the segmented copy of what the next step reads) against
SGP_CHECKPOINT_FULL=1 (every device allocation, whole), next to the same world's step time, on BASELINE config 3 (100k bodies) and
config 5 (1k cars + 50k debris); plus sgp_checkpoint_write + sgp_world_restore wall time and blob size.

    python tools/experiments/checkpoint_bench.py OUTDIR [--repeats 40] [--configs 3,5] [--small]

Device time is measured with HIP events recorded on the world's stream around each call (so it includes the stream's wait for the host where
the host is the slower side), after warm-up, lean and full alternating in the same process (two worlds of one scene, one created with the
switch set).  Median and spread (min, max, inter-quartile range) of REPEATS calls.  Writes OUTDIR/checkpoint_bench.json and prints a table.
The copy kernel alone is timed by 50 back-to-back launches between two events (sgp_debug_time_checkpoint_copy).
`--kernel-only N`: N lean captures and rollbacks and nothing else, for a separate run under a kernel trace."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from substrata_amd import scenes      # noqa: E402
from substrata_amd.lib import World, init      # noqa: E402

DT = 1.0 / 60.0
SETTLE = 240


class Events:
    """hipEvent pairs on a world's stream (the runtime libsgp.so already loaded)."""

    def __init__(self, world):
        self.hip = C.CDLL("libamdhip64.so")
        s = C.c_void_p()
        world._check(world._fn("world_stream")(world._h, C.byref(s)), "world_stream")
        self.stream = s
        self.a, self.b = C.c_void_p(), C.c_void_p()
        assert self.hip.hipEventCreate(C.byref(self.a)) == 0 and self.hip.hipEventCreate(C.byref(self.b)) == 0

    def time_ms(self, fn):
        t0 = time.perf_counter()
        self.hip.hipEventRecord(self.a, self.stream)
        fn()
        self.hip.hipEventRecord(self.b, self.stream)
        self.hip.hipEventSynchronize(self.b)
        wall = 1e3 * (time.perf_counter() - t0)
        ms = C.c_float(0.0)
        self.hip.hipEventElapsedTime(C.byref(ms), self.a, self.b)
        return float(ms.value), wall


def build(config, small, full):
    if full:
        os.environ["SGP_CHECKPOINT_FULL"] = "1"
    else:
        os.environ.pop("SGP_CHECKPOINT_FULL", None)
    try:
        if config == 3:
            descs = scenes.config3_100k_mixed(30, 30, 10) if small else scenes.config3_100k_mixed()
            w = World(max_bodies=len(descs) + 32768)
            w.add_batch(descs)
            n_cars = 0
        else:
            descs, car_ids = scenes.config5_cars_debris(8, 3000) if small else scenes.config5_cars_debris()
            w = World(max_bodies=len(descs) + 32768)
            scenes.use_car_hull(w, descs, car_ids)
            w.add_batch(descs)
            for b in car_ids:
                w.vehicle_create(w.default_vehicle_desc(int(b)))
            n_cars = len(car_ids)
    finally:
        os.environ.pop("SGP_CHECKPOINT_FULL", None)
    return w, n_cars


def stepper(w, n_cars):
    k = [0]

    def step():
        if n_cars:
            w.vehicle_set_inputs(0, scenes.config5_inputs(n_cars, k[0] * DT))
        k[0] += 1
        w.step(DT)
    return step


def summary(xs):
    a = np.sort(np.asarray(xs, dtype=np.float64))
    return {"median": float(np.median(a)), "min": float(a[0]), "max": float(a[-1]), "iqr": float(np.percentile(a, 75) - np.percentile(a, 25)), "n": int(len(a))}


def measure(config, repeats, small):
    worlds = {}
    for mode in ("lean", "full"):
        w, n_cars = build(config, small, mode == "full")
        step = stepper(w, n_cars)
        for _ in range(SETTLE if not small else 60):
            step()
        worlds[mode] = {"w": w, "step": step, "ev": Events(w), "cp": None, "capture": [], "rollback": [], "step_ms": [], "capture_wall": [], "rollback_wall": []}
    # warm-up: sizes the checkpoints, loads the kernels
    for m in worlds.values():
        m["cp"] = m["w"].checkpoint()
        for _ in range(3):
            m["step"](); m["w"].checkpoint(m["cp"]); m["step"](); m["w"].rollback(m["cp"])
    for _ in range(repeats):
        for mode in ("lean", "full"):      # alternating
            m = worlds[mode]
            w, cp, ev = m["w"], m["cp"], m["ev"]
            d, wall = ev.time_ms(m["step"]); m["step_ms"].append(d)
            d, wall = ev.time_ms(lambda: w.checkpoint(cp)); m["capture"].append(d); m["capture_wall"].append(wall)
            m["step"]()
            d, wall = ev.time_ms(lambda: w.rollback(cp)); m["rollback"].append(d); m["rollback_wall"].append(wall)
    out = {"config": config, "small": bool(small), "repeats": repeats}
    for mode, m in worlds.items():
        info = m["cp"].info()
        st = m["w"].stats()
        out[mode] = {"capture_ms": summary(m["capture"]), "rollback_ms": summary(m["rollback"]), "step_ms": summary(m["step_ms"]),
                     "capture_wall_ms": summary(m["capture_wall"]), "rollback_wall_ms": summary(m["rollback_wall"]),
                     "info": info, "bodies": int(st.num_bodies), "constraints": int(st.num_manifolds)}
    # the copy kernel alone: 50 launches back to back between two events (sgp_debug_time_checkpoint_copy), lean world
    m = worlds["lean"]
    m["step"](); m["w"].checkpoint(m["cp"])
    us, nbytes = C.c_float(0.0), C.c_uint64(0)
    fn = m["w"]._lib.sgp_debug_time_checkpoint_copy
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_uint64)]
    m["w"]._check(fn(m["w"]._h, m["cp"]._h, 50, C.byref(us), C.byref(nbytes)), "debug_time_checkpoint_copy")
    out["kernel"] = {"us_per_launch": float(us.value), "bytes_read": int(nbytes.value), "launches": 50,
                     "TB_per_s_read_plus_write": 2.0 * nbytes.value / (us.value * 1e-6) / 1e12}
    # the blob: host-bound, reported without a target (lean world)
    m = worlds["lean"]
    t0 = time.perf_counter(); blob = m["cp"].to_bytes(); t_write = time.perf_counter() - t0
    fresh = World(max_bodies=m["w"].max_bodies)
    t0 = time.perf_counter(); fresh.restore(blob); t_restore = time.perf_counter() - t0
    out["blob"] = {"bytes": len(blob), "write_ms": 1e3 * t_write, "restore_ms": 1e3 * t_restore}
    fresh.close()
    for m in worlds.values():
        m["cp"].close(); m["w"].close()
    return out


def kernel_only(config, n, small):
    w, n_cars = build(config, small, False)
    step = stepper(w, n_cars)
    for _ in range(SETTLE if not small else 60):
        step()
    cp = w.checkpoint()
    for _ in range(n):
        step(); w.checkpoint(cp); step(); w.rollback(cp)
    print(json.dumps({"kernel_only": n, "info": cp.info()}))
    cp.close(); w.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("outdir")
    ap.add_argument("--repeats", type=int, default=40)
    ap.add_argument("--configs", default="3,5")
    ap.add_argument("--small", action="store_true", help="a tenth of the scenes (a quick check of the script)")
    ap.add_argument("--kernel-only", type=int, default=0)
    a = ap.parse_args()
    os.makedirs(a.outdir, exist_ok=True)
    init()
    configs = [int(c) for c in a.configs.split(",")]
    if a.kernel_only:
        kernel_only(configs[0], a.kernel_only, a.small)
        return
    results = []
    for c in configs:
        r = measure(c, a.repeats, a.small)
        results.append(r)
        for mode in ("lean", "full"):
            x = r[mode]
            print(f"config {c} {mode:4s}: capture {x['capture_ms']['median']:.3f} ms (min {x['capture_ms']['min']:.3f}, max {x['capture_ms']['max']:.3f}, iqr {x['capture_ms']['iqr']:.3f})  "
                  f"rollback {x['rollback_ms']['median']:.3f} ms (min {x['rollback_ms']['min']:.3f}, max {x['rollback_ms']['max']:.3f}, iqr {x['rollback_ms']['iqr']:.3f})  "
                  f"step {x['step_ms']['median']:.3f} ms  device bytes {x['info']['device_bytes']} of {x['info']['world_device_bytes']}", flush=True)
        print(f"config {c} copy kernel alone: {r['kernel']['us_per_launch']:.1f} us per launch for {r['kernel']['bytes_read']} bytes read and as many written = {r['kernel']['TB_per_s_read_plus_write']:.2f} TB/s", flush=True)
        print(f"config {c} blob: {r['blob']['bytes']} bytes, write {r['blob']['write_ms']:.1f} ms, restore {r['blob']['restore_ms']:.1f} ms", flush=True)
        json.dump(results, open(os.path.join(a.outdir, "checkpoint_bench.json"), "w"), indent=1)


if __name__ == "__main__":
    main()
