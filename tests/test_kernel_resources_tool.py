"""tools/kernel_resources.py (pure Python, no compiler, no GPU): its parser on a short canned listing and the resource remarks that go with it.
Two kernels, one with packed f32 and register moves and one without; every column of the table is checked."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources as kr  # noqa: E402

LISTING = """\
	.amdgcn_target "amdgcn-amd-amdhsa--gfx950"
	.text
	.p2align	2
	.type	_ZL6helperf,@function
_ZL6helperf:                            ; @_ZL6helperf
; %bb.0:
	s_waitcnt vmcnt(0) expcnt(0) lgkmcnt(0)
	v_mul_f32_e32 v0, v0, v0
	s_setpc_b64 s[30:31]
.Lfunc_end0:
	.size	_ZL6helperf, .Lfunc_end0-_ZL6helperf
	.protected	_Z8k_pairedILi1ELi2EEvPKfPf ; -- Begin function _Z8k_pairedILi1ELi2EEvPKfPf
	.globl	_Z8k_pairedILi1ELi2EEvPKfPf
	.p2align	8
	.type	_Z8k_pairedILi1ELi2EEvPKfPf,@function
_Z8k_pairedILi1ELi2EEvPKfPf:            ; @_Z8k_pairedILi1ELi2EEvPKfPf
; %bb.0:
	s_load_dwordx4 s[0:3], s[4:5], 0x0
	v_lshlrev_b32_e32 v4, 3, v0
	s_waitcnt lgkmcnt(0)
	global_load_dwordx2 v[0:1], v4, s[0:1]
	s_waitcnt vmcnt(0)
	v_mov_b32_e32 v2, v1
	v_mov_b32_e32 v3, v0
	v_pk_mul_f32 v[0:1], v[0:1], v[2:3]
	v_pk_add_f32 v[0:1], v[0:1], v[2:3] op_sel_hi:[1,0]
	s_nop 0
	v_mov_b32_dpp v5, v0 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf bound_ctrl:1
	v_sub_f32_e32 v0, v0, v5
	v_pk_fma_f32 v[0:1], v[0:1], v[2:3], v[0:1]
	v_pk_mov_b32 v[2:3], v[0:1], v[0:1]
.LBB1_1:                                ; =>This Inner Loop Header: Depth=1
	scratch_store_dword off, v0, off offset:4
	global_store_dwordx2 v4, v[0:1], s[2:3]
	s_endpgm
	.section	.rodata,"a",@progbits
	.p2align	6, 0x0
	.amdhsa_kernel _Z8k_pairedILi1ELi2EEvPKfPf
		.amdhsa_group_segment_fixed_size 0
		.amdhsa_next_free_vgpr 110
	.end_amdhsa_kernel
	.text
.Lfunc_end1:
	.size	_Z8k_pairedILi1ELi2EEvPKfPf, .Lfunc_end1-_Z8k_pairedILi1ELi2EEvPKfPf
                                        ; -- End function
	.protected	_Z7k_plainPf           ; -- Begin function _Z7k_plainPf
	.globl	_Z7k_plainPf
	.p2align	8
	.type	_Z7k_plainPf,@function
_Z7k_plainPf:                           ; @_Z7k_plainPf
; %bb.0:
	s_load_dwordx2 s[0:1], s[4:5], 0x0
	v_lshlrev_b32_e32 v0, 2, v0
	s_waitcnt lgkmcnt(0)
	global_load_dword v1, v0, s[0:1]
	s_waitcnt vmcnt(0)
	v_mul_f32_e32 v1, v1, v1
	v_sub_f32_dpp v1, v1, v1 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf bound_ctrl:1
	v_cvt_pk_bf16_f32 v2, v1, v1
	global_store_dword v0, v1, s[0:1]
	s_endpgm
	.section	.rodata,"a",@progbits
	.p2align	6, 0x0
	.amdhsa_kernel _Z7k_plainPf
		.amdhsa_next_free_vgpr 3
	.end_amdhsa_kernel
	.text
.Lfunc_end2:
	.size	_Z7k_plainPf, .Lfunc_end2-_Z7k_plainPf
"""

REMARKS = """\
canned.hip:9:1: remark: Function Name: _ZL6helperf [-Rpass-analysis=kernel-resource-usage]
canned.hip:9:1: remark:     VGPRs: 1 [-Rpass-analysis=kernel-resource-usage]
canned.hip:9:1: remark:     ScratchSize [bytes/lane]: 0 [-Rpass-analysis=kernel-resource-usage]
canned.hip:9:1: remark:     Occupancy [waves/SIMD]: 8 [-Rpass-analysis=kernel-resource-usage]
canned.hip:17:1: remark: Function Name: _Z8k_pairedILi1ELi2EEvPKfPf [-Rpass-analysis=kernel-resource-usage]
canned.hip:17:1: remark:     TotalSGPRs: 12 [-Rpass-analysis=kernel-resource-usage]
canned.hip:17:1: remark:     VGPRs: 110 [-Rpass-analysis=kernel-resource-usage]
canned.hip:17:1: remark:     AGPRs: 0 [-Rpass-analysis=kernel-resource-usage]
canned.hip:17:1: remark:     ScratchSize [bytes/lane]: 16 [-Rpass-analysis=kernel-resource-usage]
canned.hip:17:1: remark:     Dynamic Stack: False [-Rpass-analysis=kernel-resource-usage]
canned.hip:17:1: remark:     Occupancy [waves/SIMD]: 4 [-Rpass-analysis=kernel-resource-usage]
canned.hip:17:1: remark:     SGPRs Spill: 0 [-Rpass-analysis=kernel-resource-usage]
canned.hip:17:1: remark:     VGPRs Spill: 4 [-Rpass-analysis=kernel-resource-usage]
canned.hip:17:1: remark:     LDS Size [bytes/block]: 0 [-Rpass-analysis=kernel-resource-usage]
canned.hip:40:1: remark: Function Name: _Z7k_plainPf [-Rpass-analysis=kernel-resource-usage]
canned.hip:40:1: remark:     TotalSGPRs: 8 [-Rpass-analysis=kernel-resource-usage]
canned.hip:40:1: remark:     VGPRs: 3 [-Rpass-analysis=kernel-resource-usage]
canned.hip:40:1: remark:     AGPRs: 0 [-Rpass-analysis=kernel-resource-usage]
canned.hip:40:1: remark:     ScratchSize [bytes/lane]: 0 [-Rpass-analysis=kernel-resource-usage]
canned.hip:40:1: remark:     Dynamic Stack: False [-Rpass-analysis=kernel-resource-usage]
canned.hip:40:1: remark:     Occupancy [waves/SIMD]: 8 [-Rpass-analysis=kernel-resource-usage]
canned.hip:40:1: remark:     SGPRs Spill: 0 [-Rpass-analysis=kernel-resource-usage]
canned.hip:40:1: remark:     VGPRs Spill: 0 [-Rpass-analysis=kernel-resource-usage]
canned.hip:40:1: remark:     LDS Size [bytes/block]: 0 [-Rpass-analysis=kernel-resource-usage]
"""

NAMES = {"_Z8k_pairedILi1ELi2EEvPKfPf": "void k_paired<1, 2>(float const*, float*)", "_Z7k_plainPf": "k_plain(float*)"}


def _parse():
    return kr.parse(LISTING, REMARKS, demangle=lambda syms: {s: NAMES[s] for s in syms})


def test_only_kernels_are_listed_under_their_short_names():
    assert list(_parse()) == ["k_paired<1,2>", "k_plain"]      # the helper function is no kernel; listing order kept


def test_every_column_of_the_kernel_with_packed_f32():
    row = _parse()["k_paired<1,2>"]
    assert set(row) == set(kr.COLUMNS)
    assert row == dict(instructions=17, valu=9, packed_f32=3, v_mov=4, vgprs=110, scratch=16, waves_per_simd=4)      # v_mov: two plain, one dpp, one v_pk_mov_b32 (no packed f32 arithmetic)


def test_every_column_of_the_kernel_without():
    row = _parse()["k_plain"]
    assert row == dict(instructions=10, valu=4, packed_f32=0, v_mov=0, vgprs=3, scratch=0, waves_per_simd=8)      # v_cvt_pk_bf16_f32 is no packed f32 arithmetic


def test_table_prints_before_and_after():
    rows = _parse()
    before = {"k_paired<1,2>": dict(rows["k_paired<1,2>"], vgprs=120, waves_per_simd=3)}
    lines = kr.table(rows, before).splitlines()
    assert lines[0] == "| kernel | instructions | VALU | packed f32 | `v_mov` | VGPRs | scratch B | waves/SIMD |"
    assert lines[2] == "| `k_paired<1,2>` | 17 | 9 | 3 | 4 | 120 → 110 | 16 | 3 → 4 |"
    assert lines[3] == "| `k_plain` | 10 | 4 | 0 | 0 | 3 | 0 | 8 |"


def test_a_kernel_without_remarks_is_an_error():
    import pytest
    with pytest.raises(ValueError):
        kr.parse(LISTING, REMARKS.replace("_Z7k_plainPf", "_Z7k_otherPf"))
