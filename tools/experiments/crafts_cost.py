"""What a frame of scripted craft costs: update + step per frame for 1, 64 and 4096 crafts (hover cars and boats alternating, every seat taken, water on),
through a sgp_crafts batch and through the host loop the controllers imply -- read the bodies' states (a wait), evaluate, send the force calls -- in one
process, wall clock.  The host loop's arithmetic here is the numpy restatement of tests/craft_reference.py, which is far slower than the reference's C++;
it is timed on its own, and "host loop without arithmetic" (the read-back and the force calls alone) is the floor no host implementation gets under.
PYTHONPATH=.:tests python tools/experiments/crafts_cost.py [frames = 30]"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "tests"))
import craft_reference as cr      # noqa: E402
import craft_scenes as cs         # noqa: E402
from substrata_amd import abi     # noqa: E402
from substrata_amd.lib import World      # noqa: E402

DT = 1.0 / 60.0


def scene(n):
    w = World(max_bodies=max(64, 2 * n + 16))
    w.set_water(True, cs.WATER_Z)
    cs.add_ground_box(w, n)
    descs = [cs.craft_desc(k, 3) for k in range(n)]
    bodies = [cs.add_craft_body(w, d["kind"], cs.home(k)) for k, d in enumerate(descs)]
    inputs = [dict(forward=1.0, right=0.3, up=0.1, hand_brake=0.0, flags=cr.IN_DRIVER) for _ in range(n)]
    return w, descs, bodies, inputs


def batch_frames(n, frames):
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "tests"))
    from test_crafts_gpu import to_abi, inputs_array
    w, descs, bodies, inputs = scene(n)
    crafts = w.crafts(n)
    ps = w.particles(n * abi.CRAFT_MAX_EMIT)
    crafts.attach(ps)
    for k, d in enumerate(descs):
        crafts.add(to_abi(crafts, d, bodies[k]))
    crafts.set_inputs(0, inputs_array(inputs))
    times = []
    for f in range(frames + 5):
        t0 = time.perf_counter()
        crafts.update(DT)
        ps.update(DT)
        w.step(DT)
        w.get_state(bodies[:1])      # (the frame ends when the step has: one wait)
        times.append(time.perf_counter() - t0)
    crafts.close(); ps.close(); w.close()
    return float(np.median(times[5:]))


def host_frames(n, frames, arithmetic_frames):
    w, descs, bodies, inputs = scene(n)
    timers = [(-1.0, -1.0)] * n
    read_t, math_t, call_t, step_t = [], [], [], []
    ops_cache = None
    for f in range(frames + 2):
        t0 = time.perf_counter()
        st = w.get_state(bodies)
        t1 = time.perf_counter()
        if ops_cache is None or f < arithmetic_frames:
            ops_cache = []
            for i, d in enumerate(descs):
                body = dict(pos=st["pos"][i], rot=st["rot"][i], lin_vel=st["lin_vel"][i], ang_vel=st["ang_vel"][i], submerged=st["submerged_volume"][i])
                ops_cache.append(cr.craft_update(d, inputs[i], body, timers[i], (True, cs.WATER_Z), None, f, DT)["ops"])
            math_t.append(time.perf_counter() - t1)
        t2 = time.perf_counter()
        for i, ops in enumerate(ops_cache):
            cs.apply_ops(w, bodies[i], ops)
        t3 = time.perf_counter()
        w.step(DT)
        w.get_state(bodies[:1])
        t4 = time.perf_counter()
        read_t.append(t1 - t0); call_t.append(t3 - t2); step_t.append(t4 - t3)
    w.close()
    med = lambda a: float(np.median(a[2:] if len(a) > 2 else a))
    return med(read_t), float(np.median(math_t)), med(call_t), med(step_t)


if __name__ == "__main__":
    frames = int(sys.argv[1]) if len(sys.argv) > 1 else 30
    for n in (1, 64, 4096):
        b = batch_frames(n, frames)
        r, m, c, s = host_frames(n, frames if n < 4096 else 6, 3 if n < 4096 else 1)
        print(json.dumps({"crafts": n, "batch_frame_ms": round(b * 1e3, 4), "host_read_ms": round(r * 1e3, 4), "host_force_calls_ms": round(c * 1e3, 4), "host_step_ms": round(s * 1e3, 4),
                          "host_frame_without_arithmetic_ms": round((r + c + s) * 1e3, 4), "host_numpy_arithmetic_ms": round(m * 1e3, 3)}), flush=True)
