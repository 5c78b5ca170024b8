"""Register pressure of the solver kernels of the bench's path, from the compiler alone (no GPU): sgp_k_solve.hip and sgp_k_solve_hc.hip are each compiled
once to gfx950 assembly through tools/kernel_resources.py with the flags substrata_amd/build.py gives that file (two hipcc -S runs, the only slow CPU test
of this kind).  No kernel of the config 3 step may use scratch, and none may fall below the waves per SIMD of the table in docs/KERNELS.md ("f32 pairing")
for the build it ships with: the colour kernels are built without the pairing of f32 operations (5 and 7 waves), k_solve_hc measured slower that way and
keeps the pairing in a stage file of its own (2 and 4 waves, the table's left-hand figures).  A later flag or source change that brings the register
pressure back fails here, not in a profile nobody takes."""
import os
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

# kernel -> (stage file, waves per SIMD it must at least reach)
MIN_WAVES = {"k_solve_colour<1,2,1>": ("sgp_k_solve.hip", 5), "k_solve_colour<2,-1,1>": ("sgp_k_solve.hip", 7),
             "k_solve_hc<1,2>": ("sgp_k_solve_hc.hip", 2), "k_solve_hc<2,-1>": ("sgp_k_solve_hc.hip", 4)}


@pytest.fixture(scope="module")
def rows():
    from substrata_amd import build as b
    cc = b.hipcc()
    if not (os.path.exists(cc) if os.path.isabs(cc) else shutil.which(cc)):
        pytest.skip("no hipcc")
    import kernel_resources as kr
    return {src: kr.resources(src) for src in sorted({s for s, _ in MIN_WAVES.values()})}


def test_the_colour_kernels_are_built_without_f32_pairing_and_the_component_launch_with_it():
    from substrata_amd import build as b
    assert "-fno-slp-vectorize" in b.source_flags("sgp_k_solve.hip")
    assert "-fno-slp-vectorize" not in b.source_flags("sgp_k_solve_hc.hip")


@pytest.mark.parametrize("kernel", sorted(MIN_WAVES))
def test_solver_kernel_has_no_scratch_and_keeps_its_occupancy(rows, kernel):
    src, waves = MIN_WAVES[kernel]
    assert kernel in rows[src], sorted(rows[src])
    row = rows[src][kernel]
    print(kernel, row)
    assert row["scratch"] == 0
    assert row["waves_per_simd"] >= waves
    if src == "sgp_k_solve.hip":
        assert row["packed_f32"] == 0
