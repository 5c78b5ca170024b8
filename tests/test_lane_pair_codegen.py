"""Roots and divisions of the lane-pair solver kernels, from the compiler alone (no GPU): lanes 2k and 2k + 1 of a wave are body 1 and body 2 of one
constraint, so a branch on `side` runs both ways in every wave and every root and division under it is paid twice.  half_apply, pos_half_solve_rec
and v3_normalized_perpendicular fold the difference into an operand (docs/KERNELS.md, "One path for both lanes"); this test keeps a later change from
bringing a twin back.  sgp_k_solve.hip and sgp_k_solve_hc.hip are each compiled once to gfx950 assembly through tools/kernel_resources.py with the
flags substrata_amd/build.py gives that file (slow in the way test_step_codegen.py is slow), and v_sqrt_f32 / v_rcp_f32 -- one per IEEE root /
division -- are counted per kernel.  The bounds follow from the source:

* a position solve of one contact point has 2 roots and 6 divisions: 1 / inv, |w| and s / len of quat_add_rotation_step, and the root and four
  divisions of quat_normalized.  k_solve_colour<2,-1,1> inlines four points: 8 and 24.  k_solve_hc<2,-1> inlines seven position solves: 56 and 168.
* a velocity iteration on the layout without rows has the perpendicular once (1 root, 2 divisions) and the friction clamp of four points
  (max_f / sqrtf(tot_sq)): 5 and 6.

Scratch stays 0 and the waves per SIMD stay at the figures of test_step_codegen.py."""
import os
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

OPS = ("v_sqrt_f32", "v_rcp_f32")
# kernel -> (stage file, most v_sqrt_f32, most v_rcp_f32, fewest waves per SIMD)
BOUNDS = {"k_solve_colour<2,-1,1>": ("sgp_k_solve.hip", 8, 24, 7),
          "k_solve_colour<1,2,1>": ("sgp_k_solve.hip", 5, 6, 5),
          "k_solve_hc<2,-1>": ("sgp_k_solve_hc.hip", 56, 168, 4),
          "k_solve_hc<1,2>": ("sgp_k_solve_hc.hip", None, None, 2)}      # (no bound from the source written down for the 13 phases of the velocity component launch)


@pytest.fixture(scope="module")
def rows():
    from substrata_amd import build as b
    cc = b.hipcc()
    if not (os.path.exists(cc) if os.path.isabs(cc) else shutil.which(cc)):
        pytest.skip("no hipcc")
    import kernel_resources as kr
    return {src: kr.resources(src, ops=OPS) for src in sorted({v[0] for v in BOUNDS.values()})}


@pytest.mark.parametrize("kernel", sorted(BOUNDS))
def test_roots_and_divisions_are_compiled_once(rows, kernel):
    src, roots, divisions, waves = BOUNDS[kernel]
    assert kernel in rows[src], sorted(rows[src])
    row = rows[src][kernel]
    print(kernel, row)
    if roots is not None:
        assert row["v_sqrt_f32"] <= roots
        assert row["v_rcp_f32"] <= divisions
    assert row["scratch"] == 0
    assert row["waves_per_simd"] >= waves


def test_the_counter_names_whole_mnemonics():
    """(no compiler) every encoding of the named instruction counts, and nothing that merely begins like it"""
    import kernel_resources as kr
    listing = "\n".join(["k:", "\tv_rcp_f32_e32 v0, v1", "\tv_rcp_f32_e64 v0, -v1", "\tv_rcp_f64_e32 v[0:1], v[2:3]", "\tv_rcp_iflag_f32_e32 v0, v1",
                         "\tv_sqrt_f32_sdwa v0, v1 dst_sel:DWORD", "\tv_sqrt_f32_e64_dpp v0, v1 quad_perm:[1,0,3,2]", "\tv_sqrt_f64_e32 v[0:1], v[2:3]", "\ts_endpgm",
                         "\t.amdhsa_kernel k", "\t.end_amdhsa_kernel", ".Lfunc_end0:", "helper:", "\tv_rcp_f32_e32 v0, v1", ".Lfunc_end1:"])
    assert kr.count_ops(listing, OPS) == {"k": {"v_sqrt_f32": 2, "v_rcp_f32": 2}}
    assert kr.parse_listing(listing)["k"]["instructions"] == 8
