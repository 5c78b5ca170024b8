"""Builds substrata_amd/libsgp.so (HIP, gfx950 only) in-tree with hipcc.  Cross-compiles without a GPU.

One object per stage file of csrc/ (sgp_k_*.hip: the kernels; sgp_world*.hip: the host side of the C ABI), compiled side by side and
linked; an object is rebuilt only when its source, a header or this script is newer (objects live in csrc/.obj/, git-ignored).

-ffp-contract=off: fp32 expressions round exactly as written (no FMA contraction), the contract that lets the parity
tests compare the device path with the CPU oracle to rounding.  Correctly rounded fp32 divide/sqrt is hipcc's default.

SOURCE_FLAGS: extra flags per source file.  Four stage files of the world step (sgp_k_solve, sgp_k_narrowphase, sgp_k_sweep,
sgp_k_vehicle) are built with -fno-slp-vectorize: under plain -O3 the SLP vectorizer pairs neighbouring scalar f32 multiplies and adds
of the v3 arithmetic into v_pk_mul_f32 / v_pk_add_f32 and pays for the aligned register pairs with v_mov_b32 and registers
(docs/KERNELS.md, "f32 pairing"; tools/kernel_resources.py prints the table).  Each packed instruction becomes the two IEEE
operations it stood for: results do not change.  The load/store vectorizer is another pass and is not touched.  A file has the
flag only where its kernels measured no slower without the pairing (profiles/scalar_f32_step_kernels.md): sgp_k_constraints.hip
(k_setup) and sgp_k_solve_hc.hip (k_solve_hc, a stage file of its own for this reason) measured slower and keep the pairing.  The
query, character, particle, craft, mover, cast, mesh, tile, checkpoint and edit files have not been measured and stay as they were.
"""
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
OBJ = os.path.join(CSRC, ".obj")
LIB = os.path.join(HERE, "libsgp.so")
KERNEL_SOURCES = sorted(f for f in os.listdir(CSRC) if f.startswith("sgp_k_") and f.endswith(".hip"))
HOST_SOURCES = sorted(f for f in os.listdir(CSRC) if f.startswith("sgp_world") and f.endswith(".hip"))
HEADERS = sorted(f for f in os.listdir(CSRC) if f.endswith(".h")) + [os.path.join("..", "..", "include", "sgp.h")]      # every header: several are generated
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-fPIC",
         "-fvisibility=hidden", "-mllvm", "-amdgpu-kernarg-preload-count=16", "-Wall", "-Wno-unused-function", "-Wno-unused-result", "-Wno-unused-value"]
NO_F32_PAIRING = ["-fno-slp-vectorize"]
SOURCE_FLAGS = {
    "sgp_k_solve.hip": NO_F32_PAIRING,
    "sgp_k_narrowphase.hip": NO_F32_PAIRING,
    "sgp_k_sweep.hip": NO_F32_PAIRING,
    "sgp_k_vehicle.hip": NO_F32_PAIRING,
}


def source_flags(src):
    """The whole flag list build() compiles `src` (a file name in csrc/) with, without the -c / -o part."""
    return FLAGS + list(SOURCE_FLAGS.get(src, ()))


def hipcc():
    for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", "hipcc"):
        if c and (os.path.isabs(c) and os.path.exists(c) or not os.path.isabs(c)):
            return c
    return "hipcc"


def _newer(deps, target):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps)


def _common_deps():
    return [os.path.join(CSRC, h) for h in HEADERS] + [os.path.abspath(__file__)]


def _sources():
    return KERNEL_SOURCES + HOST_SOURCES


def _obj(src):
    return os.path.join(OBJ, src[:-4] + ".o")


def needs_build():
    return _newer(_common_deps() + [os.path.join(CSRC, s) for s in _sources()], LIB)


def build(force=False, verbose=False, extra=()):
    if not force and not needs_build():
        return LIB
    os.makedirs(OBJ, exist_ok=True)
    common = _common_deps()
    todo = [s for s in _sources() if force or _newer(common + [os.path.join(CSRC, s)], _obj(s))]

    def compile_one(src):
        cmd = [hipcc()] + source_flags(src) + list(extra) + ["-c", os.path.join(CSRC, src), "-o", _obj(src)]
        if verbose:
            print(" ".join(cmd), flush=True)
        return src, subprocess.run(cmd, capture_output=True, text=True)

    with ThreadPoolExecutor(max_workers=min(len(todo), os.cpu_count() or 4) or 1) as pool:
        results = list(pool.map(compile_one, todo))
    failed = [(s, r) for s, r in results if r.returncode != 0]
    for s, r in results:
        if r.returncode != 0 or (verbose and (r.stdout or r.stderr)):
            sys.stderr.write(f"---- {s}\n{r.stdout}{r.stderr}")
    if failed:
        raise RuntimeError("hipcc failed building " + ", ".join(s for s, _ in failed))
    cmd = [hipcc(), "--offload-arch=gfx950", "-shared", "-fPIC", "-fvisibility=hidden"] + [_obj(s) for s in _sources()] + ["-o", LIB]
    if verbose:
        print(" ".join(cmd), flush=True)
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        sys.stderr.write(r.stdout + r.stderr)
        raise RuntimeError("hipcc failed linking libsgp.so")
    return LIB


if __name__ == "__main__":
    build(force="--force" in sys.argv, verbose=True)
