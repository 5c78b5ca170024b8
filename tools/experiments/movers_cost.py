"""What a frame of scripted movers costs: update + step per frame for 256, 4096 and 65 536 movers -- a train-heavy mix: of every eight, one leader and five
carriages on a loop and two move-to platforms whose tracks keep running -- through a sgp_movers batch and through what the parent commit offers for the same:
a host loop of sgp_body_move_kinematic calls, whose commands the step uploads.  One process, wall clock around work that ends in a wait, medians of the
frames after a warm-up.  The host loop's own arithmetic (the path evaluation) is NOT counted: its targets are computed once, outside the clock, so the figure is
the floor no host implementation gets under; the calls go through ctypes with prebuilt arguments (about a microsecond each; a C++ caller pays less).
PYTHONPATH=.:tests python tools/experiments/movers_cost.py [frames = 40] [log file to append to]"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "tests"))
import mover_reference as mr      # noqa: E402
import mover_scenes as ms         # noqa: E402
from substrata_amd import abi, scenes      # noqa: E402
from substrata_amd.lib import World        # noqa: E402

DT = 1.0 / 60.0


def scene(n, trains=False):
    w = World(max_bodies=n + 64)
    d = scenes._blank(n)
    d["motion_type"] = abi.MOTION_KINEMATIC; d["layer"] = abi.LAYER_MOVING; d["activate"] = 1
    d["shape"][:, :3] = (1.0, 1.0, 0.2)
    k = np.arange(n)
    d["pos"] = np.column_stack([40.0 * (k % 256), 40.0 * (k // 256), np.full(n, 30.0)])      # apart: the step has no pairs to find, its cost is the sweep
    if trains:      # the bodies of a train start on their loop (tools: loop_waypoints), so that the first update is no leap across the world
        on_loop = k % 8 < 6
        d["pos"][on_loop] = np.column_stack([60.0 * ((k // 16) % 64) + 1.5 * (k % 8), 60.0 * ((k // 16) // 64), np.full(n, 1.0)])[on_loop]
    return w, [int(i) for i in w.add_batch(d)]


def loop_waypoints(j):
    """The loop of the test table, the j-th copy of it: 60 m apart, so that the trains of different loops never meet."""
    a = np.zeros(len(ms.PATHS["loop"]), dtype=abi.path_waypoint_dtype)
    for k, (pos, typ, pause, speed) in enumerate(ms.PATHS["loop"]):
        a[k]["pos"] = (pos[0] + 60.0 * (j % 64), pos[1] + 60.0 * (j // 64), 1.0); a[k]["type"] = typ; a[k]["pause_time"] = pause; a[k]["speed"] = speed
    return a


def batch_frames(n, frames):
    w, bodies = scene(n, trains=True)
    movers = w.movers(n, (n + 15) // 16)
    leader = p = None
    for k, b in enumerate(bodies):
        if k % 16 == 0:
            p = movers.add_path(loop_waypoints(k // 16))      # two trains to a loop, half a lap apart: they keep their distance
        if k % 8 == 0:
            leader = movers.add_path_mover(b, p, 8.58 * ((k // 8) % 2), orient_along_path=True)
        elif k % 8 < 6:
            movers.add_path_mover(b, p, leader=leader, follow_dist=2.5 * (k % 8), orient_along_path=True)
        else:
            at = (40.0 * (k % 256), 40.0 * (k // 256), 30.0)
            i = movers.add_moveto_mover(b, at)
            movers.set_position_track(i, at, (at[0], at[1], 38.0), 1.0e3, mr.EASE_SMOOTHSTEP, 0.0)
            movers.set_rotation_track(i, (0, 0, 0, 1), (0, 0, 1, 0), 1.0e3, mr.EASE_LINEAR, 0.0)
    frame, update, enqueue = [], [], []
    for f in range(frames + 5):
        w.get_state(bodies[:1])
        t0 = time.perf_counter()
        movers.update(DT)
        t1 = time.perf_counter()
        w.get_state(bodies[:1])              # (a wait: the update has run)
        t2 = time.perf_counter()
        movers.update(DT)
        w.step(DT)
        w.get_state(bodies[:1])              # (the frame ends when the step has)
        t3 = time.perf_counter()
        enqueue.append(t1 - t0); update.append(t2 - t0); frame.append(t3 - t2)
    assert int(movers.states(0, 1)[0]["update_index"]) == 2 * (frames + 5)
    movers.close(); w.close()
    med = lambda a: float(np.median(a[5:]))
    return med(enqueue), med(update), med(frame)


def host_frames(n, frames):
    w, bodies = scene(n)
    fn = w._fn("body_move_kinematic")
    pos = [(C.c_float * 3)(40.0 * (k % 256) + 0.01, 40.0 * (k // 256), 30.0) for k in range(n)]
    rot = (C.c_float * 4)(0.0, 0.0, 0.0, 1.0)
    dt = C.c_float(DT)
    h = w._h
    calls, frame = [], []
    for f in range(frames + 5):
        w.get_state(bodies[:1])
        t0 = time.perf_counter()
        for k in range(n):
            fn(h, bodies[k], pos[k], rot, dt)
        t1 = time.perf_counter()
        w.step(DT)                           # (uploads and applies the commands, then steps)
        w.get_state(bodies[:1])
        t2 = time.perf_counter()
        calls.append(t1 - t0); frame.append(t2 - t0)
    w.close()
    med = lambda a: float(np.median(a[5:]))
    return med(calls), med(frame)


if __name__ == "__main__":
    frames = int(sys.argv[1]) if len(sys.argv) > 1 else 40
    log = open(sys.argv[2], "a") if len(sys.argv) > 2 else None
    for n in (256, 4096, 65536):
        e, u, b = batch_frames(n, frames)
        c, hf = host_frames(n, frames if n < 65536 else 8)
        line = json.dumps({"movers": n, "batch_update_enqueue_ms": round(e * 1e3, 4), "batch_update_until_done_ms": round(u * 1e3, 4), "batch_frame_ms": round(b * 1e3, 4),
                           "host_move_kinematic_calls_ms": round(c * 1e3, 4), "host_frame_without_arithmetic_ms": round(hf * 1e3, 4)})
        print(line, flush=True)
        if log:
            log.write(line + "\n"); log.flush()
