"""The store policy of the solver kernels, from the compiler alone (no GPU).  A launch that solves ONE colour and the pass of the component launch
store records and impulses that no lane of the same launch reads again, so they write them THROUGH the L2 (store_rec<ST_WT>,
store_rec2, sgp_dev_common.h; the rule and the audit: docs/KERNELS.md, "Write-through stores"): the kernel boundary behind them then has no dirty
lines to write back (config 3 +2.8 %, profiles/write_through_stores.md).  The kernels in which a workgroup walks several colours through global
memory -- k_solve_tail, k_solve_tail_vel, the small-world kernels and the catch-all at the end of k_solve_hc -- keep plain stores: a later phase
of the same launch reads those lines again.  So do k_warm_bodies, which measured no gain, the warm start by constraint, k_solve_colour<0>, where a
lane has no partner for store_rec2 (argued from the two-store build's loss, NOT measured: the benchmark's world never runs it), and the instances for
colours of more than SOLVE_MANY_MIN constraints (k_solve_colour<*,*,3>), with which config 4 measured slower.

This test holds the product and its plain twin (-DSGP_SOLVER_STORES=0, the build for another measurement): sgp_k_solve.hip and sgp_k_solve_hc.hip
are compiled to gfx950 assembly with the flags substrata_amd/build.py gives each file, once as they are and once with that flag (four compilations
side by side; slow in the way test_lane_pair_codegen.py is slow), and the vector stores to memory are counted per kernel by mnemonic and by the
write-through bit (`sc1` among the store's operands).

* The product: in the kernels that write through, records and impulses are ONE `buffer_store_dwordx4 ... sc1` each (the raw buffer builtin) -- a
  16-byte record is neither four dword stores nor two 8-byte halves --, every other store is plain, and per kernel there are as many store
  instructions as in the twin (which has the stores the kernels had before the policy existed).  One width differs, and on purpose nothing is
  done about it: where a body's first record is stored as F4(linear velocity, inverse mass) with the inverse mass it was loaded with, the compiler
  narrows a plain store to the 12 bytes that change (`global_store_dwordx3`); the builtin stores the 16 bytes it is given.
* The two halves of a 32-byte record must leave in one store instruction, on two neighbouring lanes (store_rec2): as two stores of one lane they
  left the L2 as two partial writes and the policy lost 1.6 %.  The listing cannot show which lane stores what; the count can show that the
  pairing added no store, and tests/test_store_policy_gpu.py that every byte lands where it belongs.
* k_solve_hc: 6 (velocity: four impulses, two halves of the record) and 2 (position) of its stores are the pass's and written through; the rest
  are the catch-all's (six inlined solves) and the ticket's, and stay plain.
* The twin: no store of any solver kernel carries the bit.

The counts are read off the listings once."""
import collections
import os
import re
import shutil
import sys
from concurrent.futures import ThreadPoolExecutor

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

TWIN_FLAG = "-DSGP_SOLVER_STORES=0"
WT = "buffer_store_dwordx4+sc1"
X4, X3, X1 = "global_store_dwordx4", "global_store_dwordx3", "global_store_dword"
SOLVE, HC = "sgp_k_solve.hip", "sgp_k_solve_hc.hip"
# kernel -> (stage file, stores of the plain twin {mnemonic: count}, stores of the product {mnemonic (+sc1: with the write-through bit): count};
#            None: the twin's, no store written through)
EXPECT = {
    "k_solve_colour<1,2,1>": (SOLVE, {X4: 5, X3: 1}, {WT: 6}),                 # two halves of the record, four impulses
    "k_solve_colour<1,1,1>": (SOLVE, {X4: 5, X3: 1}, {WT: 6}),
    "k_solve_colour<1,0,1>": (SOLVE, {X4: 5, X3: 1}, {WT: 6}),
    "k_solve_colour<2,-1,1>": (SOLVE, {X4: 1, X3: 1}, {WT: 2}),                # position and rotation
    "k_solve_hc<1,2>": (HC, {X4: 36, X3: 6, X1: 1}, {WT: 6, X4: 30, X3: 6, X1: 1}),
    "k_solve_hc<1,1>": (HC, {X4: 36, X3: 6, X1: 1}, {WT: 6, X4: 30, X3: 6, X1: 1}),
    "k_solve_hc<1,0>": (HC, {X4: 36, X3: 6, X1: 1}, {WT: 6, X4: 30, X3: 6, X1: 1}),
    "k_solve_hc<2,-1>": (HC, {X4: 8, X3: 6, X1: 1}, {WT: 2, X4: 6, X3: 6, X1: 1}),
    # plain stores in both builds: the warm start by body (measured: no gain) and by constraint (no partner lane); several colours per launch through global memory
    "k_warm_bodies": (SOLVE, {X4: 3, X3: 3}, None),
    "k_solve_colour<0,-1,1>": (SOLVE, {X4: 2, X3: 2}, None),
    # plain stores in both builds: the instances for colours of more than SOLVE_MANY_MIN constraints (OCC != 1), which run in rounds and evict their lines by
    # capacity anyway -- config 4 measured 1.3 % slower with write-through there (profiles/write_through_stores.md)
    "k_solve_colour<1,2,3>": (SOLVE, {X4: 5, X3: 1}, None),
    "k_solve_colour<1,1,3>": (SOLVE, {X4: 5, X3: 1}, None),
    "k_solve_colour<2,-1,3>": (SOLVE, {X4: 1, X3: 1}, None),
    "k_solve_tail": (SOLVE, {X4: 10, X3: 6}, None),
    "k_solve_tail_vel<0>": (SOLVE, {X4: 15, X3: 3}, None),
    "k_solve_tail_vel<1>": (SOLVE, {X4: 15, X3: 3}, None),
    "k_solve_tail_vel<2>": (SOLVE, {X4: 15, X3: 3}, None),
    "k_solve_small": (SOLVE, {X4: 13}, None),
    "k_solve_small_single": (SOLVE, {X4: 20}, None),
}
WRITE_THROUGH = tuple(k for k, v in EXPECT.items() if v[2] is not None)
PLAIN = tuple(k for k, v in EXPECT.items() if v[2] is None)

_LABEL = re.compile(r"^([A-Za-z_.$][\w.$]*):")
_STORE = re.compile(r"^\s+((?:global|buffer|flat)_store_[a-z0-9_]+)\s+(.*)$")      # vector stores to memory (spills to scratch are not records)


def memory_stores(listing):
    """{kernel symbol: Counter of 'mnemonic' / 'mnemonic+sc1'} over each kernel's own function body (label to end-of-function mark)"""
    kernels = set(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", listing, re.M))
    out, seen, cur = {}, set(), None
    for line in listing.splitlines():
        m = _LABEL.match(line)
        if m:
            name = m.group(1)
            if name in kernels and name not in seen:
                seen.add(name)
                cur = name
                out[cur] = collections.Counter()
            elif name.startswith(".Lfunc_end"):
                cur = None
            continue
        if cur is None:
            continue
        m = _STORE.match(line)
        if m:
            operands = m.group(2).split(";")[0]
            out[cur][m.group(1) + ("+sc1" if re.search(r"\bsc1\b", operands) else "")] += 1
    return out


@pytest.fixture(scope="module")
def stores():
    """{(stage file, build): {kernel: Counter}}, build = 'product' | 'twin'"""
    from substrata_amd import build as b
    cc = b.hipcc()
    if not (os.path.exists(cc) if os.path.isabs(cc) else shutil.which(cc)):
        pytest.skip("no hipcc")
    import kernel_resources as kr
    jobs = [(src, build) for src in (SOLVE, HC) for build in ("product", "twin")]

    def one(job):
        src, build = job
        flags = b.source_flags(src) + ([TWIN_FLAG] if build == "twin" else [])
        by_symbol = memory_stores(kr.compile_file(src, flags)[0])
        names = kr.demangler()(sorted(by_symbol))
        return job, {kr.short_name(names[sym]): c for sym, c in by_symbol.items()}
    with ThreadPoolExecutor(max_workers=len(jobs)) as pool:
        return dict(pool.map(one, jobs))


@pytest.mark.parametrize("kernel", WRITE_THROUGH)
def test_records_and_impulses_are_written_through(stores, kernel):
    src, twin, product = EXPECT[kernel]
    assert kernel in stores[src, "product"], sorted(stores[src, "product"])
    got = stores[src, "product"][kernel]
    print(kernel, dict(got))
    assert got[WT] == product[WT] and got[WT] > 0
    assert [k for k in got if k.endswith("+sc1")] == [WT]      # every write-through store is one whole 16-byte record
    assert dict(got) == product
    assert sum(got.values()) == sum(twin.values())             # as many store instructions as with plain stores: no record was split


@pytest.mark.parametrize("kernel", PLAIN)
def test_kernels_that_read_their_lines_again_keep_plain_stores(stores, kernel):
    src, twin, _ = EXPECT[kernel]
    assert kernel in stores[src, "product"], sorted(stores[src, "product"])
    got = stores[src, "product"][kernel]
    print(kernel, dict(got))
    assert not [k for k in got if k.endswith("+sc1")]
    assert dict(got) == twin


@pytest.mark.parametrize("kernel", sorted(EXPECT))
def test_the_twin_stores_plain(stores, kernel):
    src, twin, _ = EXPECT[kernel]
    got = stores[src, "twin"][kernel]
    print(kernel, dict(got))
    assert not [k for k in got if k.endswith("+sc1")]
    assert dict(got) == twin


def test_the_counter_reads_the_bit_and_the_kernel():
    """(no compiler) the bit counts only among a store's operands, in the kernel's own body, and scratch traffic is left out"""
    listing = "\n".join(["k:", "\tbuffer_store_dwordx4 v[0:3], v6, s[0:3], 0 offen sc1", "\tglobal_store_dwordx4 v[0:1], v[2:5], off ; not sc1",
                         "\tglobal_store_dwordx2 v[0:1], v[2:3], off offset:8 sc0 sc1", "\tscratch_store_dwordx2 off, v[0:1], off", "\tbuffer_wbl2 sc1",
                         "\tglobal_load_dwordx4 v[0:3], v[4:5], off sc1", "\ts_endpgm", "\t.amdhsa_kernel k", "\t.end_amdhsa_kernel", ".Lfunc_end0:",
                         "helper:", "\tglobal_store_dword v[0:1], v2, off sc1", ".Lfunc_end1:"])
    assert memory_stores(listing) == {"k": {"buffer_store_dwordx4+sc1": 1, "global_store_dwordx4": 1, "global_store_dwordx2+sc1": 1}}
