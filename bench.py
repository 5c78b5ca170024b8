#!/usr/bin/env python3
"""bench.py -- physics steps/sec at fixed dt = 1/60 s, 100k bodies (BASELINE.json metric).

    python bench.py --gpus N --steps K --warmup W
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P bench.py --gpus N ...

Called directly with --gpus N > 1 (no WORLD_SIZE in the environment) it launches itself through torch.distributed.run with N ranks on 127.0.0.1
and hands the ranks' output through, rank 0's JSON line last.  SGP_BENCH_SHARE_GPU=1 (a test switch, tests/test_bench_selflaunch_gpu.py) puts every
rank on cuda:0 with gloo between the processes and the test-only collective library behind SGP_RCCL_LIBRARY: the line then says
"transport": "test stand-in" and is never a scaling number.

A "step" is one PhysicsWorld::think(1/60) (/root/reference/gui_client/PhysicsWorld.cpp:1356-1443).  All state is resident in HBM
before the timed region; every step blocks until the device has finished it, like think().

N = 1 (the bench line): BASELINE config 3, 100k mixed box / sphere / capsule bodies (100x100x10 lattice, seed 3,
substrata_amd/scenes.py) dropped on the ground quad.  The measured state is PINNED, independent of --steps / --warmup:

    settle   SETTLE_STEPS (240) untimed steps from the lattice -> the settled pile (~300k contact constraints); its body states are
             read back once: the SNAPSHOT
    each leg starts from a fresh world built from the snapshot + PRIME_STEPS (24) untimed steps that rebuild the contact cache and
             let the launch plan settle, then the same W warm-up steps:
      timed      K steps, barrier + synchronize on both sides                           -> value, ms_per_step
    with --full, after the timed leg:
      read-back  the application's real loop, every step followed by the active-pose read-back (reported next to the headline)
      profiled   P steps with HIP events around every launch on the world's stream      -> roofline, kernel_ms_per_step
      cpu        the CPU oracle (a port, NOT Jolt) built from the same snapshot, 1 untimed + C timed steps -> cpu_baseline
    The simulation is deterministic, so every GPU leg walks through the very same states; `checks` in the JSON asserts it.

A plain run (no --full) sets up, warms up, times the K steps and prints the headline line; the other legs (and, at N > 1 or config 4, the
profiled steps and the CPU baseline) run only with --full.  --dump-outputs DIR writes the body states the timed world holds after its last
timed step (pos, rot, lin_vel, ang_vel, active; float32, one DIR/<field>.npy each; at most 64 MB, beyond that a fixed seeded sample of the
bodies whose indices are in DIR/sample_index.npy).  Tiles of N > 1 ranks write DIR/<field>_rank<r>.npy.

N > 1: BASELINE config 4, the 1M-box lattice (100^3, spacing 1.25 m, seed 4) STRONG-scaled over N spatial tiles of the 3-D grid
2x1x1 / 2x2x1 / 2x2x2 (substrata_amd/tiles.py), one process per GPU, ghost bodies exchanged once per step by sgp_tiles_exchange (RCCL
all-gather of the counts + grouped send / recv of the records, issued inside libsgp.so; the run fails if that cannot be set up -- there is
no second transport); value = steps/s of the whole 1M-body world.  (`--workload config3` at N > 1 keeps the round-1
weak-scaling layout, one 100k tile per GPU side by side; `--workload config4` at N = 1 runs the whole 1M world on one GPU.)

Prints ONE JSON line (rank 0).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

DT = 1.0 / 60.0
HBM_PEAK_GBS = 8000.0          # MI355X HBM3E spec peak (MI355X_MICROARCH.md)
HBM_ACHIEVABLE_GBS = 6300.0    # what a streaming kernel reaches on this part (same guide)
SWEEP_BYTES_PER_BODY = 188     # integrate + AABB body-array sweep, 112 B read + 76 B written
# per contact point per velocity iteration (no rows, the default from 65k constraints on since the end of round 5: the lanes rebuild r x axis and I (r x axis) from
# the lever arms): two lever-arm records (float4: r1 | bias, r2 | effective mass of the normal row), the friction rows' effective masses (float2), lambdas read, lambdas written
SOLVE_BYTES_PER_POINT = 2 * 16 + 8 + 16 + 16
# the other two layouts (sgp_step_profile::row_layout): 1 = r x axis stored (worlds below 65 536 constraints): 3 axes x 2 x 16 B of rows + lambdas read and written;
# 0 = full rows (worlds of <= 2048 body slots): 3 axes x 4 x 16 B + lambdas
SOLVE_BYTES_PER_POINT_BY_LAYOUT = {2: SOLVE_BYTES_PER_POINT, 1: 96 + 16 + 16, 0: 192 + 16 + 16}
# per manifold: ab 8 + normal/friction 16 + np 4; the velocity records of two bodies read and written; their world-inverse-inertia records (DV::iw) read
SOLVE_BYTES_PER_MANIFOLD = 28 + 2 * 32 + 2 * 32 + 2 * 32
SETTLE_STEPS = 240             # lattice -> settled pile, untimed, independent of the command line
SETTLE_STEPS_TILED = 120       # N > 1 (config 4): untimed steps before the warm-up
PRIME_STEPS = 24               # after a world is rebuilt from the snapshot: contact cache + launch plan + graph capture
PMC_FILE = os.path.join(ROOT, "profiles", "pmc_traffic.json")   # per-launch HBM traffic from the rocprofv3 --pmc passes (tools/collect_pmc.sh)


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=600)      # >= 600 timed steps after 120 warm-up steps
    ap.add_argument("--warmup", type=int, default=120)
    ap.add_argument("--bodies", type=int, default=100000, help="config3: bodies per tile (BASELINE: 100k)")
    ap.add_argument("--workload", default="auto", choices=["auto", "config3", "config4", "config5"],
                    help="auto = config3 at N = 1 (the bench line), config4 (1M boxes, strong scaling over 3-D tiles) at N > 1; "
                         "config5 = 1k cars + 50k debris (extra measurement, N = 1 only)")
    ap.add_argument("--lattice", type=int, default=100, help="config4: boxes per lattice edge (BASELINE: 100 -> 1M)")
    ap.add_argument("--cpu-steps", type=int, default=16, help="oracle steps timed for cpu_baseline (0 = skip)")
    ap.add_argument("--cpu-threads", type=int, default=0, help="OpenMP threads of the oracle (0 = sweep 16 / 32 / 64 / 128 / 256 up to the host's cpus and time the sample with the best)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-readback-leg", action="store_true")
    ap.add_argument("--profile-steps", type=int, default=8)
    ap.add_argument("--retile-every", type=int, default=16, help="config4 on N > 1 GPUs: move the tiles' split planes to the quantiles of bodies + contacts every this many steps (0: static split)")
    ap.add_argument("--force-comm", action="store_true", help="N = 1 with --workload config4: build the process group and the RCCL communicator anyway "
                    "(one rank), so that a one-GPU box runs the very code path of N > 1")
    ap.add_argument("--full", action="store_true", help="also run the legs beyond the headline: active-pose read-back, profiled steps (roofline, "
                    "kernel_ms_per_step), the CPU baseline and the bit-exact check against the oracle")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None, help="write the body states after the last timed step as DIR/<field>.npy (float32)")
    return ap.parse_args()


DUMP_BYTES = 64 << 20
DUMP_FIELDS = ("pos", "rot", "lin_vel", "ang_vel", "active")


def dump_outputs(dirname, states, suffix="", budget=DUMP_BYTES):
    """--dump-outputs: what a caller reads back after the timed path's last step, the body states, one float32 .npy per field.  Beyond
    `budget` bytes a fixed seeded sample of the bodies is written, its indices (float64) in sample_index<suffix>.npy."""
    os.makedirs(dirname, exist_ok=True)
    per_body = 4 * sum(int(np.prod(states.dtype[f].shape)) for f in DUMP_FIELDS)
    if len(states) * per_body > budget:
        k = (budget - 1024) // (per_body + 8)        # (1024: the .npy headers)
        idx = np.sort(np.random.default_rng(20260101).choice(len(states), size=k, replace=False))
        np.save(os.path.join(dirname, f"sample_index{suffix}.npy"), idx.astype(np.float64))
        states = states[idx]
    for f in DUMP_FIELDS:
        np.save(os.path.join(dirname, f"{f}{suffix}.npy"), np.ascontiguousarray(states[f], dtype=np.float32))


def single_gpu_reference(workload, lattice):
    """The same workload on ONE GPU, from the committed log (strong scaling is measured against this, not against the N = 1 bench line,
    which is config 3)."""
    if workload != "config4" or lattice != 100:
        return None
    try:
        with open(os.path.join(ROOT, "profiles", "r06y_bench_config4_1gpu.log")) as f:
            j = json.loads([l for l in f if l.startswith("{")][-1])
        return {"value": j["value"], "unit": j["unit"], "ms_per_step": j["ms_per_step"], "source": "profiles/r06y_bench_config4_1gpu.log (bench.py --workload config4, one MI355X, this round's final tree)"}
    except (OSError, ValueError, IndexError, KeyError):
        return None


def emit_line(out):
    """Rank 0's ONE JSON line, as the last line of stdout: RCCL writes its version banner through C stdio, which (stdout being a pipe or a file) sits in
    libc's buffer until exit and would land AFTER a Python print -- so libc's buffers are flushed first."""
    try:
        import ctypes
        ctypes.CDLL(None).fflush(None)
    except Exception:
        pass
    sys.stdout.flush()
    print(json.dumps(out), flush=True)


def load_pmc():
    try:
        with open(PMC_FILE) as f:
            return json.load(f)
    except (OSError, ValueError):
        return {}


KERNEL_TIME_FILE = os.path.join(ROOT, "profiles", "kernel_time.json")   # average kernel durations from the committed rocprofv3 --kernel-trace run


def load_kernel_times():
    try:
        with open(KERNEL_TIME_FILE) as f:
            return json.load(f)
    except (OSError, ValueError):
        return None


def profile_leg(w, n_prof, exchange=None):
    """P profiled steps: per-kernel-class HIP-event time, launches, contact counts."""
    names = w.kernel_class_names()
    ksum = np.zeros(len(names)); klaunch = np.zeros(len(names))
    pts = cons = 0
    total_ms = 0.0
    sweep_bodies = 0
    row_layout = 2
    for _ in range(n_prof):
        if exchange is not None:
            exchange()
        p = w.step_profiled(DT)
        ksum += np.array([p.kernel_ms[k] for k in range(len(names))])
        klaunch += np.array([p.kernel_launches[k] for k in range(len(names))])
        pts += p.num_contact_points; cons += p.num_constraints
        total_ms += p.total_ms
        sweep_bodies = p.sweep_bodies
        row_layout = int(p.row_layout)
    return dict(row_layout=row_layout, names=names, ksum=ksum, klaunch=klaunch, pts=pts / n_prof, cons=cons / n_prof, sweep_bodies=sweep_bodies,
                total_ms=total_ms / n_prof)


def rooflines(prof, n_prof, vel_iters, pmc, same_workload_as_profiles=True):
    names, ksum, klaunch = prof["names"], prof["ksum"], prof["klaunch"]
    k = {nm: i for i, nm in enumerate(names)}
    sweep_classes = [c for c in ("apply_forces", "integrate_pose", "finalize", "sweep") if c in k]
    sweep_ms = sum(ksum[k[c]] for c in sweep_classes) / n_prof
    sweep_launches = sum(klaunch[k[c]] for c in sweep_classes) / n_prof
    sweep_bytes = SWEEP_BYTES_PER_BODY * prof["sweep_bodies"]
    sweep_gbs = sweep_bytes / (sweep_ms * 1e-3) / 1e9 if sweep_ms > 0 else 0.0
    sv = k["solve_velocity"]
    launches = max(klaunch[sv] / n_prof, 1)
    solve_launch_ms = ksum[sv] / max(klaunch[sv], 1)
    solve_bytes_per_launch = (SOLVE_BYTES_PER_POINT_BY_LAYOUT[prof["row_layout"]] * prof["pts"] + SOLVE_BYTES_PER_MANIFOLD * prof["cons"]) * vel_iters / launches
    solve_gbs = solve_bytes_per_launch / (solve_launch_ms * 1e-3) / 1e9 if solve_launch_ms > 0 else 0.0
    sweep_traffic = pmc.get("sweep_bytes_per_body")
    # a pass = one launch per planned colour + (when the plan solves the high colours by component) one launch for all of those
    solve_traffic = pmc.get("solve_velocity_bytes_per_launch")
    comp_traffic = pmc.get("solve_components_bytes_per_launch")
    if solve_traffic and comp_traffic and launches > vel_iters:
        solve_traffic = (solve_traffic * (launches - vel_iters) + comp_traffic * vel_iters) / launches
    roof = {
        "bound": "hbm", "kernel": "body-array sweep (K8 integrate + K1 AABB + sleep test): kernel classes " + " + ".join(sweep_classes),
        "achieved": sweep_gbs, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": sweep_gbs / HBM_PEAK_GBS,
        "algorithmic_bytes_per_launch": sweep_bytes, "launch_ms": sweep_ms, "launches_per_step": sweep_launches,
        "traffic": (sweep_traffic * prof["sweep_bodies"]) if sweep_traffic else None,
        "traffic_source": pmc.get("source", "none: run tools/collect_pmc.sh on the GPU box"),
    }
    # the same fraction by KERNEL time: HIP events around a launch also contain the dispatch gap in front of it (3 launches x ~1.5 us here); the
    # committed rocprofv3 --kernel-trace summary of the same command holds the kernels' own durations (profiles/kernel_time.json, written by
    # tools/rocpd_summary.py --json from the run that produced profiles/*kernel_stats_config3.md), so this figure reproduces from profiles/.
    # (both committed files were measured on the default workload, config 3 on one GPU: another workload gets the per-body sweep traffic only, marked as such)
    kt = load_kernel_times() if same_workload_as_profiles else None
    if not same_workload_as_profiles:
        solve_traffic = None
        if roof["traffic"] is not None:
            roof["traffic_source"] = "per-body figure measured at config 3 (100k bodies), scaled by this workload's body slots: " + roof["traffic_source"]
    if kt and prof["sweep_bodies"]:
        us = sum(kt["avg_us"].get(kn, 0.0) for kn in ("k_pre_solve", "k_integrate_pose", "k_finalize"))
        if us > 0:
            roof["kernel_time_us"] = us
            roof["achieved_kernel_time"] = sweep_bytes / (us * 1e-6) / 1e9
            roof["frac_kernel_time"] = roof["achieved_kernel_time"] / HBM_PEAK_GBS
            roof["kernel_time_source"] = kt.get("source")
    roof_solver = {
        "bound": "hbm", "kernel": "velocity iterations (dominant by time): k_solve_colour<1> per planned colour + k_solve_hc<1> for the rest, averaged per launch",
        "achieved": solve_gbs, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": solve_gbs / HBM_PEAK_GBS,
        "algorithmic_bytes_per_launch": solve_bytes_per_launch, "launch_ms": solve_launch_ms,
        "launches_per_step": klaunch[sv] / n_prof, "traffic": solve_traffic,
        "row_layout": {0: "full rows (192 B per point)", 1: "r x axis rows (96 B per point)", 2: "no rows (40 B per point and lane)"}[prof["row_layout"]],
        "traffic_kernel": pmc.get("solve_velocity_kernel"),
    }
    kernel_ms = {names[i]: round(ksum[i] / n_prof, 4) for i in range(len(names)) if klaunch[i]}
    return roof, roof_solver, kernel_ms


def self_launch(args):
    """`python bench.py --gpus N` as the driver calls it, N > 1 and no launcher around it: run the same command line through torch.distributed.run
    (one rank per GPU, rendezvous on 127.0.0.1 at a free port) and hand its output through -- rank 0's JSON line last, whatever the launcher or
    a library's exit handlers printed after it."""
    import socket
    import subprocess
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        port = so.getsockname()[1]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")      # dmabuf IPC (RCCL / tensor sharing across processes on this driver)
    env.setdefault("OMP_NUM_THREADS", "8")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}", "--master-addr", "127.0.0.1", "--master-port", str(port),
           os.path.abspath(__file__)] + sys.argv[1:]
    r = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, text=True)
    lines = r.stdout.splitlines()
    result = [l for l in lines if l.startswith('{"metric"')]
    for l in lines:
        if not result or l is not result[-1]:
            print(l)
    sys.stdout.flush()
    if result:
        print(result[-1], flush=True)
    raise SystemExit(r.returncode if r.returncode or result else 1)


def main():
    args = parse()
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        self_launch(args)
    import torch
    from substrata_amd import abi, scenes, tiles
    from substrata_amd.lib import World, init

    world_size = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    n_gpus = args.gpus
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU: the product has no CPU path")
    dist = None
    # test switch: every rank on cuda:0, gloo between the processes, the exchange's collectives through the library SGP_RCCL_LIBRARY names (the test-only
    # stand-in: real RCCL wants one GPU per rank).  Proves the launch path on a one-GPU box; its numbers are labelled and mean nothing.
    share_gpu = os.environ.get("SGP_BENCH_SHARE_GPU", "0") == "1"
    if share_gpu and world_size > 1:
        if not os.environ.get("SGP_RCCL_LIBRARY"):
            raise SystemExit("SGP_BENCH_SHARE_GPU=1 needs SGP_RCCL_LIBRARY (tests/rccl_standin/librccl_standin.so): RCCL itself refuses two ranks on one GPU")
        local_rank = 0
    if world_size > 1 or args.force_comm:
        import torch.distributed as dist
        if args.force_comm and world_size == 1:
            os.environ.setdefault("MASTER_ADDR", "127.0.0.1"); os.environ.setdefault("MASTER_PORT", "29533")
            os.environ.setdefault("RANK", "0"); os.environ.setdefault("WORLD_SIZE", "1")
        torch.cuda.set_device(local_rank)
        if share_gpu:
            dist.init_process_group(backend="gloo")
        else:
            dist.init_process_group(backend="nccl", device_id=torch.device("cuda", local_rank))      # "nccl" IS RCCL on ROCm
        assert world_size == n_gpus, "launch with --nproc-per-node equal to --gpus"
    elif n_gpus != 1:
        raise SystemExit("--gpus N > 1 needs N ranks (WORLD_SIZE is set but 1?)")
    init()
    workload = args.workload
    if workload == "auto":
        workload = "config3" if n_gpus == 1 else "config4"
    if workload == "config5" and n_gpus != 1:
        raise SystemExit("--workload config5 is a single-GPU measurement")
    xdev = torch.device("cpu") if (share_gpu and world_size > 1) else torch.device("cuda", local_rank)      # where the tensors of the torch.distributed calls live
    pmc = load_pmc()

    def barrier():
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()

    # ================================================================================================================
    # N > 1, or the whole config 4 world on one GPU: tiles
    if n_gpus > 1 or workload == "config4":
        if workload == "config4":
            descs, lo, hi = scenes.config4_tile_descs(rank, n_gpus, n=args.lattice)
            total_bodies = args.lattice ** 3
            scaling = "strong"
            workload_text = (f"BASELINE config 4: {total_bodies} unit boxes, {args.lattice}^3 lattice spacing 1.25 m, seed 4, ground quad 2000 m, dt 1/60, "
                             f"split into {n_gpus} spatial tile(s) {'x'.join(str(g) for g in tiles.tile_grid(n_gpus))} (x, y, z), ghost margin 2 m")
            value_definition = "steps/s of the whole world (all tiles advance together)"
        else:
            nx = ny = 100
            nz = max(1, args.bodies // (nx * ny))
            spacing = 1.5
            tile_w, tile_d = nx * spacing, ny * spacing
            flat = {1: (1, 1, 1), 2: (2, 1, 1), 4: (2, 2, 1), 8: (4, 2, 1)}.get(n_gpus)
            lo, hi, origin = tiles.tile_bounds(rank, n_gpus, tile_w, tile_d, grid=flat)
            descs = scenes.config3_100k_mixed(nx, ny, nz, seed=3 + rank)
            descs["pos"][1:, 0] += origin[0] + tile_w / 2 - spacing / 2
            descs["pos"][1:, 1] += origin[1] + tile_d / 2 - spacing / 2
            total_bodies = (len(descs) - 1) * n_gpus
            scaling = "weak"
            workload_text = (f"BASELINE config 3 tiles side by side: {len(descs) - 1} mixed bodies per GPU (100x100x{nz} lattice spacing 1.5 m, seed 3 + rank), "
                             f"{n_gpus} tiles, dt 1/60")
            value_definition = "n_gpus x world steps/s (one tile per GPU, all advancing together)"
        n_own = len(descs) - 1
        # room for the bodies that migrate in (config 4: the upper tiles fall into the lower ones) and for the ghosts
        cap = (2 * total_bodies // max(1, min(n_gpus, 4)) if workload == "config4" and n_gpus > 1 else n_own) + 65536
        w = World(max_bodies=cap, device=local_rank)
        w.add_batch(descs)
        ex = None
        exchange_kind = "none (one tile)"
        if n_gpus > 1 or args.force_comm:
            # the native exchange (sgp_tiles_*: device routing + RCCL send / recv from inside libsgp.so); torch.distributed only carries the
            # communicator's unique id to the other ranks and runs the barriers around the timed region.  There is no other transport: a
            # rank that cannot set the exchange up says so, every rank learns of it (so nobody is left waiting in ncclCommInitRank's peers'
            # collectives), and the run ends with an error instead of a number measured on something else.
            boxes_t = torch.zeros(n_gpus * 6, dtype=torch.float32, device=xdev)
            dist.all_gather_into_tensor(boxes_t, torch.from_numpy(np.concatenate([lo, hi]).astype(np.float32)).to(xdev))
            uid = torch.zeros(128, dtype=torch.uint8, device=xdev)
            err = ""
            if rank == 0:
                try:
                    uid.copy_(torch.frombuffer(bytearray(tiles.NativeTiles.unique_id()), dtype=torch.uint8))
                except Exception as e:      # noqa: BLE001
                    err = f"ncclGetUniqueId: {e}"
            dist.broadcast(uid, src=0)
            if not err:
                try:
                    ex = tiles.NativeTiles(w, rank, n_gpus, boxes_t.cpu().numpy().reshape(n_gpus, 6), 2.0, unique_id=bytes(uid.cpu().numpy().tobytes()))
                except Exception as e:      # noqa: BLE001
                    err = str(e)
            okt = torch.tensor([0 if err else 1], dtype=torch.int32, device=xdev)
            dist.all_reduce(okt, op=dist.ReduceOp.MIN)
            if int(okt.item()) == 0:
                print(f"[bench rank {rank}] native tile exchange (sgp_tiles_create over RCCL) failed: {err or 'on another rank'}", file=sys.stderr, flush=True)
                raise SystemExit(f"bench.py --gpus {n_gpus}: the sgp_tiles_* exchange could not be set up on every rank; there is no fallback transport")
            exchange_kind = "sgp_tiles_exchange: device routing + RCCL all-gather of counts + grouped send/recv inside libsgp.so"
            if os.environ.get("SGP_RCCL_LIBRARY"):
                exchange_kind += f" -- collective library overridden by SGP_RCCL_LIBRARY={os.environ['SGP_RCCL_LIBRARY']}"


        # config 4 over several tiles: the regions follow the bodies (sgp_tiles_rebalance every --retile-every steps; 0 = the static split, whose upper
        # tiles run empty when the tower has fallen: profiles/r04_config4_tiles_projection.md)
        retile_grid = tiles.tile_grid(n_gpus) if (workload == "config4" and (n_gpus > 1 or args.force_comm) and args.retile_every > 0) else None
        step_no = [0]

        def one_step():
            if ex is not None:
                if retile_grid is not None and step_no[0] % args.retile_every == 0:
                    ex.rebalance(retile_grid, by_contacts=True)
                ex.exchange()
            w.step(DT)
            step_no[0] += 1

        # config 4 is a tower that never comes to rest: after step ~250 of the collapse it outgrows the world's default capacities (8 N manifolds, 63
        # colours) on any layout (profiles/r04_config4_tiles_projection.md).  The untimed settle steps shrink so that the timed window ends before that;
        # a window that cannot (more than 240 warm-up + timed steps) is flagged, and what was dropped is in `dropped_pairs_or_manifolds` either way.
        settle_tiled = SETTLE_STEPS_TILED
        if workload == "config4":
            settle_tiled = max(0, min(SETTLE_STEPS_TILED, 240 - args.warmup - args.steps))
        for _ in range(settle_tiled):
            one_step()
        for _ in range(args.warmup):
            one_step()
        ex_before = ex.stats() if ex is not None else None
        barrier()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            one_step()
        barrier()
        elapsed = time.perf_counter() - t0
        ex_after = ex.stats() if ex is not None else None
        if dist is not None:
            t = torch.tensor([elapsed], dtype=torch.float64, device=xdev)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            elapsed = float(t.item())
        st = w.stats()
        if args.dump_outputs:
            dump_outputs(args.dump_outputs, w.read_states(0, w.num_bodies()), suffix=(f"_rank{rank}" if world_size > 1 else ""),
                         budget=DUMP_BYTES // max(1, world_size))
        if args.full:
            n_prof = max(1, args.profile_steps)
            prof = profile_leg(w, n_prof, exchange=(ex.exchange if ex is not None else None))
            roof, roof_solver, kernel_ms = rooflines(prof, n_prof, w.desc.settings.num_velocity_steps, pmc, same_workload_as_profiles=False)
        ex_ms = ((ex_after.total_exchange_ms - ex_before.total_exchange_ms) / max(1, ex_after.exchanges - ex_before.exchanges)) if ex is not None else 0.0
        local = np.array([w.num_bodies() - 1 - (ex.last_imported if ex else 0), st.num_manifolds, st.num_active,
                          ex.last_exported if ex else 0, ex.last_imported if ex else 0, st.pairs_dropped + st.manifolds_dropped,
                          ex_ms, ex_after.comm_ranks if ex else 0, ex_after.comm_init_ms if ex else 0.0,
                          (ex_after.route_retries if ex else 0), (ex_after.slow_imports - ex_before.slow_imports) if ex else 0], dtype=np.float64)
        if dist is not None:
            allv = torch.zeros(n_gpus * len(local), dtype=torch.float64, device=xdev)
            dist.all_gather_into_tensor(allv, torch.from_numpy(local).to(xdev))
            allv = allv.cpu().numpy().reshape(n_gpus, -1)
        else:
            allv = local[None, :]
        cpu_base = None
        if args.full and n_gpus == 1 and ex is None and not args.no_cpu_baseline and args.cpu_steps > 0:
            # B2 beside config 4 on one GPU: the CPU port (oracle, NOT Jolt) on the state after the timed and profiled steps -- one untimed step
            # (contact cache) + two timed ones with 64 threads (a step of the collapsing 1M tower is several seconds of CPU work)
            from oracle import oracle
            S = w.read_states(0, len(descs))
            snap4 = descs.copy()
            snap4["pos"] = S["pos"]; snap4["rot"] = S["rot"]; snap4["lin_vel"] = S["lin_vel"]; snap4["ang_vel"] = S["ang_vel"]
            snap4["activate"] = (S["active"] != 0).astype(np.int32)
            threads = oracle.set_threads(args.cpu_threads or min(64, os.cpu_count() or 1))
            cw = oracle.OracleWorld(max_bodies=len(snap4) + 8)
            cw.add_batch(snap4)
            cw.step(DT)
            n_cpu = min(args.cpu_steps, 2)
            tc = time.perf_counter()
            for _ in range(n_cpu):
                cw.step(DT)
            cpu_el = time.perf_counter() - tc
            cst = cw.stats()
            cpu_base = {"value": n_cpu / cpu_el, "unit": "steps/s", "cores": threads, "kind": "port",
                        "sample": f"{n_cpu} steps of the same {total_bodies}-body world from the state after the timed and profiled steps ({cst.num_manifolds} contact constraints); "
                                  f"oracle/sgo_oracle.c with {threads} OpenMP threads; this repo's CPU restatement, not JoltPhysics",
                        "contact_constraints": int(cst.num_manifolds), "host_cpus": os.cpu_count()}
            cw.close(); oracle.set_threads(1)
        # (every rank empties libc's stdout buffer -- RCCL's version banner -- before rank 0 writes the line, so that nothing follows it at exit)
        try:
            import ctypes
            ctypes.CDLL(None).fflush(None)
        except Exception:
            pass
        sys.stdout.flush()
        barrier()
        if rank == 0:
            steps_per_s = args.steps / elapsed
            out = {
                "metric": "physics steps/sec at fixed dt, 1M boxes over 3-D spatial tiles" if workload == "config4" else "physics steps/sec at fixed dt, 100k bodies per GPU",
                "value": steps_per_s * (n_gpus if scaling == "weak" else 1),
                "unit": "steps/s", "n_gpus": n_gpus, "steps": args.steps, "warmup": args.warmup,
                "ms_per_step": 1000.0 * elapsed / args.steps, "higher_is_better": True, "scaling": scaling, "vs_baseline": None,
                "dtype": "f32", "data": "synthetic",
                "config": {
                    "workload": workload_text, "total_bodies": total_bodies, "tiles": n_gpus, "value_definition": value_definition,
                    "untimed_settle_steps": settle_tiled, "timed_window_steps_of_the_scene": [settle_tiled + args.warmup + 1, settle_tiled + args.warmup + args.steps],
                    "window_beyond_capacity_horizon": bool(workload == "config4" and settle_tiled + args.warmup + args.steps > 240), "exchange": exchange_kind,
                    "single_gpu_reference": single_gpu_reference(workload, args.lattice),
                    "owned_bodies_per_tile": [int(v) for v in allv[:, 0]], "contact_constraints_per_tile": [int(v) for v in allv[:, 1]],
                    "active_bodies_per_tile": [int(v) for v in allv[:, 2]],
                    "ghosts_exported_per_tile": [int(v) for v in allv[:, 3]], "ghosts_imported_per_tile": [int(v) for v in allv[:, 4]],
                    "dropped_pairs_or_manifolds": int(allv[:, 5].sum()),
                    "exchange_ms_per_step_per_tile": [round(float(v), 4) for v in allv[:, 6]],
                    "rccl_ranks_seen_per_tile": [int(v) for v in allv[:, 7]], "nccl_comm_init_ms_per_tile": [round(float(v), 1) for v in allv[:, 8]],
                    "route_retries_per_tile": [int(v) for v in allv[:, 9]], "host_side_imports_in_timed_steps_per_tile": [int(v) for v in allv[:, 10]],
                    "body_steps_per_s": steps_per_s * total_bodies,
                },
            }
            if args.full:
                out.update({"roofline": roof, "roofline_solver": roof_solver, "kernel_ms_per_step": kernel_ms, "cpu_baseline": cpu_base})
            if share_gpu and world_size > 1:
                out["transport"] = "test stand-in"
                out["note"] = "SGP_BENCH_SHARE_GPU=1: every rank ran on cuda:0 behind a test-only collective library -- a launch-path check, NOT a scaling number"
            emit_line(out)
        w.close()
        if dist is not None:
            dist.destroy_process_group()
        return

    # ================================================================================================================
    # N = 1: config 3 (the bench line) or config 5, pinned state
    car_ids = []
    if workload == "config5":
        descs, car_ids = scenes.config5_cars_debris()
    else:
        nx = ny = 100
        nz = max(1, args.bodies // (nx * ny))
        descs = scenes.config3_100k_mixed(nx, ny, nz, seed=3)
    n_bodies = len(descs) - 1
    sim_step = [0]

    def build(d, step0):
        w = World(max_bodies=len(d) + 32768, device=local_rank)
        if len(car_ids):                # the snapshot's chassis descs name hull 1: the same hull, created first, gets that id again
            w.hull_create(scenes.CAR_HULL_POINTS, com_offset=scenes.CAR_COM_OFFSET)
        w.add_batch(d)
        for b in car_ids:
            w.vehicle_create(w.default_vehicle_desc(int(b)))
        sim_step[0] = step0
        return w

    def one_step(w):
        if len(car_ids):                 # driver input arrives every frame (CarPhysics::update -> SetDriverInput)
            w.vehicle_set_inputs(0, scenes.config5_inputs(len(car_ids), sim_step[0] * DT))
        sim_step[0] += 1
        w.step(DT)

    # ---- settle -> snapshot ----------------------------------------------------------------------------------------
    d0 = descs.copy()
    w = World(max_bodies=len(d0) + 32768, device=local_rank)
    if len(car_ids):
        scenes.use_car_hull(w, d0, car_ids)       # chassis = the reference's 12-point convex hull with a lowered centre of mass
    w.add_batch(d0)
    for b in car_ids:
        w.vehicle_create(w.default_vehicle_desc(int(b)))
    for _ in range(SETTLE_STEPS):
        one_step(w)
    S = w.read_states(0, len(d0))
    snap = d0.copy()
    snap["pos"] = S["pos"]; snap["rot"] = S["rot"]; snap["lin_vel"] = S["lin_vel"]; snap["ang_vel"] = S["ang_vel"]
    snap["activate"] = (S["active"] != 0).astype(np.int32)
    settle_stats = w.stats()
    w.close()

    def leg_world():
        """A fresh world holding the snapshot, primed (contact cache, launch plan, graph) and warmed up: the same state for every leg."""
        lw = build(snap, SETTLE_STEPS)
        for _ in range(PRIME_STEPS + args.warmup):
            one_step(lw)
        return lw

    # ---- timed leg ---------------------------------------------------------------------------------------------------
    w = leg_world()
    st_start = w.stats()
    barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        one_step(w)
    barrier()
    elapsed = time.perf_counter() - t0
    st = w.stats()
    graph_replays, eager_steps, idle_steps = w.launch_counts()
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, w.read_states(0, len(snap)))
    w.close()

    steps_per_s = args.steps / elapsed
    ms_per_step = 1000.0 * elapsed / args.steps
    out = {
        "metric": "physics steps/sec at fixed dt, 100k bodies" if workload == "config3" else "physics steps/sec at fixed dt, 1k cars + 50k debris",
        "value": steps_per_s, "unit": "steps/s", "n_gpus": 1, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": ms_per_step, "higher_is_better": True,
        # one GPU: nothing is scaled on this line.  `--gpus N` > 1 runs BASELINE config 4 (1M boxes) STRONG-scaled over N tiles and says "strong" on its own line.
        "scaling": None, "vs_baseline": None, "dtype": "f32", "data": "synthetic",
        "config": {
            "workload": (f"BASELINE config 3: {n_bodies} mixed box/sphere/capsule bodies, 100x100x{max(1, args.bodies // 10000)} lattice spacing 1.5 m, seed 3, "
                         "ground quad 2000 m, dt 1/60, Jolt default settings (10 velocity / 2 position iterations), sleeping enabled")
                        if workload == "config3" else
                        ("BASELINE config 5: 1024 cars (32x32 grid, spacing 8 m; chassis = the 12-point convex hull of the car script, centre of mass lowered 0.2 m, 1200 kg, 4 wheels, "
                         "FWD, Scripting.cpp defaults; input forward=1, steer=sin(0.5t+id) refreshed every step) + 50k unit-box debris, seed 5, dt 1/60"),
            "state": f"pinned: {SETTLE_STEPS} untimed settle steps -> snapshot; every leg = fresh world from the snapshot + {PRIME_STEPS} priming steps + warm-up",
            "bodies_per_gpu": n_bodies, "tiles": 1, "value_definition": "world steps/s",
            "active_bodies_end": st.num_active, "contact_constraints_start": st_start.num_manifolds, "contact_constraints_end": st.num_manifolds,
            "contact_points_end": st.num_contact_points, "colours_end": st.num_colours,
            "contact_constraints_after_settle": settle_stats.num_manifolds,
            "dropped_pairs_or_manifolds": st.pairs_dropped + st.manifolds_dropped,
            "graph_replays_timed_world": graph_replays, "eager_steps_timed_world": eager_steps,
        },
    }
    if not args.full:
        emit_line(out)
        return

    # ---- the application's real loop: every step followed by the read-back of the active bodies' poses ------
    # (GUIClient walks activated_obs after think(), GUIClient.cpp:6581-6723).  Reported next to the headline, never as `value`.
    readback_steps_per_s, n_read_back, st_rb = 0.0, 0, None
    if not args.no_readback_leg:
        n_rb = max(1, min(args.steps, 60))
        w = leg_world()
        # (sgp_world_read_active_poses_view: id + position + rotation per active body -- all GUIClient's loop reads, GetPositionAndRotation at
        # GUIClient.cpp:6586-6588 -- in the library's pinned host buffer, which a caller's loop reads once: no second copy)
        barrier()
        t1 = time.perf_counter()
        for _ in range(n_rb):
            one_step(w)
            active_states = w.read_active_poses_view()
        barrier()
        readback_steps_per_s = n_rb / (time.perf_counter() - t1)
        n_read_back = len(active_states)
        st_rb = w.stats()
        w.close()
    out["config"]["steps_per_s_with_active_pose_readback"] = readback_steps_per_s
    out["config"]["bodies_read_back_per_step"] = n_read_back

    # ---- roofline: HIP events around every launch ------------------------------------------------------------------------
    n_prof = max(1, args.profile_steps)
    w = leg_world()
    prof = profile_leg(w, n_prof)
    vel_iters = w.desc.settings.num_velocity_steps
    pos_iters = w.desc.settings.num_position_steps
    st_prof = w.stats()
    w.close()
    roof, roof_solver, kernel_ms = rooflines(prof, n_prof, vel_iters, pmc, same_workload_as_profiles=(workload == "config3" and args.bodies == 100000))

    sum_kernel_ms = float(sum(kernel_ms.values()))
    profiled_step_ms = float(prof["total_ms"])      # first to last launch of a PROFILED step (eager launches, an event pair around each)
    out.update({"roofline": roof, "roofline_solver": roof_solver, "kernel_ms_per_step": kernel_ms})

    # ---- the whole step against the roofline (SURVEY 8d's B_step with this step's own counts) ------------------------
    # B_step = 188 N (sweep) + 40 N (cell key + index, sorted read) + 96 P (pair gather 2 x 44 + pair id) + 132 M (manifold) + I_v C 192 + I_p C 104
    n_, p_, m_, c_ = float(prof["sweep_bodies"]), float(st.num_pairs), float(st.num_manifolds), float(st.num_contact_points)
    step_bytes = 188.0 * n_ + 40.0 * n_ + 96.0 * p_ + 132.0 * m_ + vel_iters * c_ * 192.0 + pos_iters * c_ * 104.0      # (SURVEY's model, kept as it is for comparability across rounds: 192 B per point and velocity iteration)
    step_gbs = step_bytes / (ms_per_step * 1e-3) / 1e9
    out["roofline_step"] = {
        "bound": "hbm", "kernel": "the whole step (all launches; SURVEY 8d whole-step model B_step)", "achieved": step_gbs, "peak": HBM_PEAK_GBS, "unit": "GB/s",
        "frac": step_gbs / HBM_PEAK_GBS, "frac_of_achievable": step_gbs / HBM_ACHIEVABLE_GBS, "achievable": HBM_ACHIEVABLE_GBS,
        "algorithmic_bytes_per_step": step_bytes, "ms_per_step": ms_per_step,
        "counts": {"N_body_slots": int(n_), "P_pairs": int(p_), "M_manifolds": int(m_), "C_contact_points": int(c_), "I_v": int(vel_iters), "I_p": int(pos_iters)},
        "launches_per_step": float(sum(prof["klaunch"])) / n_prof,
        "note": "latency-bound at 100k bodies: ~13 us per dependent launch, not bytes, is what a step is made of (DESIGN.md 3, 8)",
    }
    out["roofline"]["frac_of_achievable"] = out["roofline"]["achieved"] / HBM_ACHIEVABLE_GBS

    # ---- CPU baseline: the oracle (a port of the same step, NOT Jolt) on a bounded sample of the SAME state ------------------
    cpu_constraints = None
    bench_parity = None
    if not args.no_cpu_baseline and args.cpu_steps > 0:
        from oracle import oracle
        host_cpus = os.cpu_count() or 1

        def oracle_world():
            cw_ = oracle.OracleWorld(max_bodies=len(snap) + 8)
            if len(car_ids):
                cw_.hull_create(scenes.CAR_HULL_POINTS, com_offset=scenes.CAR_COM_OFFSET)     # same hull id as on the device
            cw_.add_batch(snap)
            for b_ in car_ids:               # (drivetrain state starts fresh on both sides after the snapshot)
                cw_.vehicle_create(cw_.default_vehicle_desc(int(b_)))
            return cw_

        def oracle_step(cw_, k):
            if len(car_ids):                 # the same driver input the GPU legs get at this step of the simulation
                cw_.vehicle_set_inputs(0, scenes.config5_inputs(len(car_ids), (SETTLE_STEPS + k) * DT))
            cw_.step(DT)

        cw = oracle_world()
        oracle.set_threads(min(32, host_cpus))
        oracle_step(cw, 0)                   # builds the contact cache so the timed steps are warm-started like the device's
        # thread sweep (the host has more cores than 32): two steps per candidate, the best count then times the sample.  The
        # OpenMP loops are order independent, so the thread count changes no result.
        sweep = {}
        k_step = 1
        cands = [args.cpu_threads] if args.cpu_threads else sorted({min(t, host_cpus) for t in (16, 32, 64, 128, 256)})
        for t in cands:
            got = oracle.set_threads(t)
            ts = time.perf_counter()
            for _ in range(2):
                oracle_step(cw, k_step); k_step += 1
            sweep[got] = 2 / (time.perf_counter() - ts)
        threads = max(sweep, key=sweep.get)
        oracle.set_threads(threads)
        t1 = time.perf_counter()
        for _ in range(args.cpu_steps):
            oracle_step(cw, k_step); k_step += 1
        cpu_el = time.perf_counter() - t1
        cst = cw.stats()
        cpu_constraints = cst.num_manifolds
        # parity on the TIMED state: a GPU world built from the same snapshot takes the same k_step steps; every body's pose and
        # velocities must equal the oracle's bit for bit.  Outside every timed region; the oracle is the checker here, never the thing measured.
        S_cpu = cw.read_states(0, len(snap))
        gw = build(snap, SETTLE_STEPS)
        for _ in range(k_step):
            one_step(gw)
        S_gpu = gw.read_states(0, len(snap))
        gst = gw.stats()
        gw.close()
        diff = {f: int(np.count_nonzero(np.any(S_cpu[f] != S_gpu[f], axis=-1) if S_cpu[f].ndim > 1 else (S_cpu[f] != S_gpu[f]))) for f in ("pos", "rot", "lin_vel", "ang_vel", "active")}
        bench_parity = {"steps_from_snapshot": k_step, "bodies": int(len(snap)), "bodies_differing": diff,
                        "max_abs_dpos": float(np.max(np.abs(S_cpu["pos"] - S_gpu["pos"]))), "constraints_gpu": int(gst.num_manifolds), "constraints_cpu": int(cst.num_manifolds),
                        "bit_exact": all(v == 0 for v in diff.values()) and int(gst.num_manifolds) == int(cst.num_manifolds)}
        oracle.set_threads(1)
        t2 = time.perf_counter()
        for _ in range(2):
            oracle_step(cw, k_step); k_step += 1
        cpu1 = 2 / (time.perf_counter() - t2)
        out["cpu_baseline"] = {
            "value": args.cpu_steps / cpu_el, "unit": "steps/s", "cores": threads, "kind": "port",
            "sample": f"{args.cpu_steps} steps of the same {n_bodies}-body world built from the same snapshot as the GPU legs "
                      f"({cst.num_manifolds} contact constraints, {cst.num_active} active bodies); oracle/sgo_oracle.c with {threads} OpenMP "
                      f"threads = the best of the sweep {{{', '.join(f'{t}: {v:.2f}' for t, v in sorted(sweep.items()))}}} steps/s over 2 steps each "
                      f"(single thread: {cpu1:.2f} steps/s); this is this repo's CPU restatement, not JoltPhysics (absent from the reference tree)",
            "contact_constraints": cst.num_manifolds, "host_cpus": host_cpus, "thread_sweep_steps_per_s": {str(t): round(v, 3) for t, v in sorted(sweep.items())},
        }
        cw.close()
        # B1: real JoltPhysics v5.3.0 through oracle/_ref/oracle_jolt, only where a maintainer has built it (SGP_JOLT_DIR=...
        # make -C oracle jolt_ref); the same snapshot, primitives only.  When present it becomes cpu_baseline (kind "reference") and the port
        # is kept next to it.
        jolt_bin = os.path.join(ROOT, "oracle", "_ref", "oracle_jolt")
        if os.path.exists(jolt_bin) and not len(car_ids):
            import subprocess
            import tempfile
            sys.path.insert(0, os.path.join(ROOT, "tests"))
            import jolt_ref_io
            with tempfile.TemporaryDirectory() as td:
                scene, dump = os.path.join(td, "s.bin"), os.path.join(td, "d.bin")
                jolt_ref_io.write_scene(scene, snap)
                n_j = max(args.cpu_steps, 16)
                r = subprocess.run([jolt_bin, scene, dump, "--steps", str(n_j), "--dt", repr(DT), "--checkpoints", str(n_j)], capture_output=True, text=True)
                if r.returncode == 0:
                    t = json.loads(r.stdout.strip().splitlines()[-1])
                    out["cpu_baseline_port"] = out["cpu_baseline"]
                    out["cpu_baseline"] = {"value": t["steps_per_s"], "unit": "steps/s", "cores": t["threads"], "kind": "reference",
                                           "sample": f"{n_j} steps of the same snapshot through JoltPhysics {t.get('jolt')} (oracle/jolt_ref/oracle_jolt.cpp: PhysicsWorld's "
                                                     f"constructor / addObject / think over the real Jolt API, JobSystemThreadPool with {t['threads']} threads)",
                                           "host_cpus": os.cpu_count()}
    else:
        out["cpu_baseline"] = None
    if not (out.get("cpu_baseline") or {}).get("kind") == "reference":
        # the north star's ">= 10x host-CPU Jolt" is a claim against B1 (real JoltPhysics on these cores); what is printed above is this repo's port
        out["b1"] = "blocked: JoltPhysics v5.3.0 source absent (oracle/jolt_ref/oracle_jolt.cpp needs SGP_JOLT_DIR); cpu_baseline is the repo's own CPU port, not Jolt"

    def within(a, b, tol=0.05):
        return abs(float(a) - float(b)) <= tol * max(float(b), 1.0)
    out["checks"] = {
        "constraints_profiled_vs_timed_within_5pct": within(st_prof.num_manifolds, st.num_manifolds),
        "constraints_readback_vs_timed_within_5pct": (within(st_rb.num_manifolds, st.num_manifolds) if st_rb is not None else None),
        "constraints_cpu_vs_timed_within_5pct": (within(cpu_constraints, st.num_manifolds) if cpu_constraints is not None else None),
        # the per-kernel breakdown comes from profiled steps (eager launches bracketed by event pairs), which run slower than the timed,
        # graph-replayed ones: it must reconcile with the profiled step's own device time; the slow-down is reported, not hidden
        "profiled_step_ms": profiled_step_ms, "sum_kernel_ms": sum_kernel_ms,
        "sum_kernel_ms_le_1p05_profiled_step_ms": sum_kernel_ms <= 1.05 * profiled_step_ms,
        "profiled_step_ms_over_ms_per_step": profiled_step_ms / ms_per_step if ms_per_step > 0 else None,
        "nothing_dropped": (st.pairs_dropped + st.manifolds_dropped) == 0,
        # the GPU against the oracle on the bench's own pile: same snapshot, same number of steps, every body compared bit for bit (None: leg skipped)
        "bench_state_bit_exact_vs_oracle": (bench_parity["bit_exact"] if bench_parity else None),
        "bench_state_parity": bench_parity,
    }
    emit_line(out)


if __name__ == "__main__":
    main()
