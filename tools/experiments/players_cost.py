"""What a driven character batch costs and saves (profiles/players_cost.md), on characters_bench.py's scene: N = 1, 64, 1024 characters walking on the ground
around the settled config-3 pile.
  (a) per-frame host wall time: today's caller loop (readBack, host rule, SetLinearVelocity, update) against the driven batch (sgp_characters_update_at only)
  (b) device time of k_characters_update, driven against undriven with host-supplied velocities, from rocprofv3 --kernel-trace --stats runs of their own
  (c) with --parent-lib: the undriven kernel of this tree against an earlier build of libsgp.so, alternating, --rounds times each (the spread of each side
      against itself is what the difference has to stay within)
PYTHONPATH=. python tools/experiments/players_cost.py [--frames 30] [--rounds 3] [--parent-lib path/to/libsgp.so] [--skip-table]"""
import argparse
import csv
import glob
import os
import shutil
import subprocess
import sys
import tempfile

from substrata_amd import build, build_shim, scenes

HERE = os.path.dirname(os.path.abspath(__file__))


def kernel_ns(exe, args, lib_dir, tmp, tag):
    """(calls, average ns) of k_characters_update in a kernel trace of one run"""
    out = os.path.join(tmp, "prof_" + tag)
    env = dict(os.environ, LD_LIBRARY_PATH=lib_dir + os.pathsep + os.environ.get("LD_LIBRARY_PATH", ""))
    r = subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "-o", "kt", "--", exe] + args, env=env, capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        sys.exit("rocprofv3 failed: " + r.stdout[-1000:] + r.stderr[-1000:])
    for path in glob.glob(os.path.join(out, "**", "*kernel_stats.csv"), recursive=True):
        for row in csv.DictReader(open(path)):
            if "k_characters_update" in row["Name"]:
                return int(row["Calls"]), float(row["AverageNs"])
    sys.exit("no k_characters_update in the kernel stats of " + out)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", default="30")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--parent-lib")
    ap.add_argument("--skip-table", action="store_true")
    a = ap.parse_args()
    lib_dir = os.path.dirname(build.build())
    build_shim.build()
    with tempfile.TemporaryDirectory() as tmp:
        descs = os.path.join(tmp, "config3.bin")
        scenes.config3_100k_mixed().tofile(descs)
        exe, exe_old = os.path.join(tmp, "players_cost"), os.path.join(tmp, "players_cost_undriven")
        for out, extra in ((exe, []), (exe_old, ["-DNO_DRIVE"])):
            subprocess.run(["g++", "-O2", "-std=c++17", "-I", os.path.join(lib_dir, "shim"), os.path.join(HERE, "players_cost.cpp"), "-o", out,
                            "-L", lib_dir, "-lsgp_shim", "-lsgp"] + extra, check=True)
        env = dict(os.environ, LD_LIBRARY_PATH=lib_dir + os.pathsep + os.environ.get("LD_LIBRARY_PATH", ""))
        if not a.skip_table:
            print("(a) host wall time per frame, median of %s frames" % a.frames, flush=True)
            subprocess.run([exe, descs, a.frames, "table"], env=env, check=True)
        print("\n(b) k_characters_update, average device time per launch (rocprofv3 --kernel-trace --stats, one run per cell)\n| N | undriven, us | driven, us | difference, us |\n|---|---|---|---|", flush=True)
        for n in ("1", "64", "1024"):
            cu, u = kernel_ns(exe, [descs, a.frames, "kernel", "undriven", n], lib_dir, tmp, "u" + n)
            cd, d = kernel_ns(exe, [descs, a.frames, "kernel", "driven", n], lib_dir, tmp, "d" + n)
            print("| %s | %.1f (%d launches) | %.1f (%d launches) | %+.1f |" % (n, u / 1e3, cu, d / 1e3, cd, (d - u) / 1e3), flush=True)
        if a.parent_lib:
            parent_dir = os.path.join(tmp, "parent")
            os.makedirs(parent_dir)
            shutil.copy(a.parent_lib, os.path.join(parent_dir, "libsgp.so")); shutil.copy(os.path.join(lib_dir, "libsgp_shim.so"), parent_dir)
            print("\n(c) the undriven k_characters_update, N = 1024, this tree against the parent build, alternating; average us per launch\n| round | parent | tree |\n|---|---|---|", flush=True)
            p, t = [], []
            for r in range(a.rounds):
                p.append(kernel_ns(exe_old, [descs, a.frames, "kernel", "undriven", "1024"], parent_dir, tmp, "p%d" % r)[1] / 1e3)
                t.append(kernel_ns(exe_old, [descs, a.frames, "kernel", "undriven", "1024"], lib_dir, tmp, "t%d" % r)[1] / 1e3)
                print("| %d | %.1f | %.1f |" % (r + 1, p[-1], t[-1]), flush=True)
            print("parent: mean %.1f, spread %.1f (max - min); tree: mean %.1f, spread %.1f; tree - parent: %+.1f us" % (sum(p) / len(p), max(p) - min(p), sum(t) / len(t), max(t) - min(t), sum(t) / len(t) - sum(p) / len(p)))


if __name__ == "__main__":
    main()
