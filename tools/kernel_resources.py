#!/usr/bin/env python
"""Per-kernel instruction and register table of the stage files, from the compiler alone (no GPU).

Compiles the named files of substrata_amd/csrc/ to gfx950 assembly with the flags substrata_amd/build.py gives each file (or with another
flag set) and prints, per kernel: instructions, VALU instructions, packed f32 instructions (v_pk_mul/add/fma_f32), register moves (v_mov_b32, v_pk_mov_b32), VGPRs,
scratch bytes per lane and waves per SIMD.  Registers, scratch and occupancy come from -Rpass-analysis=kernel-resource-usage, the rest
is counted from the listing (the kernel's own function body: label to end-of-function mark).

  python tools/kernel_resources.py sgp_k_solve.hip sgp_k_constraints.hip            # build.py's flags
  python tools/kernel_resources.py sgp_k_solve.hip --without=-fno-slp-vectorize     # before -> after: build.py's flags less one, against build.py's
  python tools/kernel_resources.py sgp_k_solve.hip --flags="--offload-arch=gfx950 -O2"      # any flag set
  python tools/kernel_resources.py sgp_k_solve.hip --kernels='k_solve_(colour|hc)<'  # only kernels whose name matches
  python tools/kernel_resources.py sgp_k_solve.hip --ops=v_sqrt_f32,v_rcp_f32        # two more columns: how often these mnemonics occur (roots and divisions)
"""
import argparse
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

COLUMNS = ("instructions", "valu", "packed_f32", "v_mov", "vgprs", "scratch", "waves_per_simd")
HEADINGS = ("instructions", "VALU", "packed f32", "`v_mov`", "VGPRs", "scratch B", "waves/SIMD")

_LABEL = re.compile(r"^([A-Za-z_.$][\w.$]*):")
_INSTR = re.compile(r"^\s+([a-z][a-z0-9_]*)\b")
_PACKED_F32 = re.compile(r"^v_pk_(mul|add|fma)_f32")
_ENCODING = re.compile(r"(_e32|_e64|_dpp|_sdwa)+$")
_REMARK = re.compile(r"remark: (?:[^:\[]*:\d+:\d+: )?\s*([A-Za-z][A-Za-z /]*?)(?: \[[^\]]*\])?: (\S+)")


def _kernel_mnemonics(text):
    """(kernel symbol, mnemonic) of every instruction in the own function body of every symbol the listing declares with .amdhsa_kernel, in listing order"""
    kernels = set(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, re.M))
    seen, cur = set(), None
    for line in text.splitlines():
        m = _LABEL.match(line)
        if m:
            name = m.group(1)
            if name in kernels and name not in seen:
                seen.add(name)
                cur = name
                yield cur, None      # (a kernel without instructions is still a row)
            elif name.startswith(".Lfunc_end"):
                cur = None
            continue
        if cur is None:
            continue
        m = _INSTR.match(line)
        if m:      # else: directives (.p2align ...), comments, blank lines
            yield cur, m.group(1)


def parse_listing(text):
    """{kernel symbol: {instructions, valu, packed_f32, v_mov}} for every symbol the listing declares with .amdhsa_kernel."""
    out = {}
    for name, op in _kernel_mnemonics(text):
        cur = out.setdefault(name, dict(instructions=0, valu=0, packed_f32=0, v_mov=0))
        if op is None:
            continue
        cur["instructions"] += 1
        if op.startswith("v_"):
            cur["valu"] += 1
            if _PACKED_F32.match(op):
                cur["packed_f32"] += 1
            elif op.startswith("v_mov_b32") or op.startswith("v_pk_mov_b32"):      # plain, dpp and sdwa forms, and the pair move
                cur["v_mov"] += 1
    return out


def count_ops(text, ops):
    """{kernel symbol: {mnemonic: count}} for the named mnemonics (say v_sqrt_f32, v_rcp_f32: one per IEEE root / division).  A name counts every
    encoding of the instruction (v_rcp_f32_e32, _e64, _dpp, _sdwa) and nothing else (v_rcp_f32 is not v_rcp_f64 or v_rcp_iflag_f32)."""
    ops = tuple(ops)
    out = {}
    for name, op in _kernel_mnemonics(text):
        cur = out.setdefault(name, dict.fromkeys(ops, 0))
        base = _ENCODING.sub("", op) if op else None
        if base in cur:
            cur[base] += 1
    return out


def parse_remarks(text):
    """{kernel symbol: {vgprs, scratch, waves_per_simd}} from the remarks of -Rpass-analysis=kernel-resource-usage."""
    out, cur = {}, None
    for line in text.splitlines():
        m = _REMARK.search(line)
        if not m:
            continue
        key, val = m.group(1).strip(), m.group(2)
        if key == "Function Name":
            cur = out.setdefault(val, {})
        elif cur is not None:
            if key == "VGPRs":
                cur["vgprs"] = int(val)
            elif key == "ScratchSize":
                cur["scratch"] = int(val)
            elif key == "Occupancy":
                cur["waves_per_simd"] = int(val)
    return out


def short_name(demangled):
    """'void k_solve_colour<1, 2, 1>(unsigned int const*, ...)' -> 'k_solve_colour<1,2,1>'"""
    s = demangled.strip()
    depth, end = 0, len(s)
    for i, ch in enumerate(s):      # cut the argument list: the first '(' outside template brackets
        if ch == "<":
            depth += 1
        elif ch == ">":
            depth -= 1
        elif ch == "(" and depth == 0:
            end = i
            break
    s = s[:end]
    if s.startswith("void "):
        s = s[5:]
    return s.replace(", ", ",")


def demangler():
    """symbol -> readable name through llvm-cxxfilt / c++filt when there is one, else the symbol itself"""
    tool = next((t for t in ("/opt/rocm/llvm/bin/llvm-cxxfilt", shutil.which("llvm-cxxfilt"), shutil.which("c++filt")) if t and os.path.exists(t)), None)

    def run(symbols):
        if not tool or not symbols:
            return {s: s for s in symbols}
        r = subprocess.run([tool] + list(symbols), capture_output=True, text=True)
        names = r.stdout.splitlines()
        return dict(zip(symbols, names)) if r.returncode == 0 and len(names) == len(symbols) else {s: s for s in symbols}
    return run


def parse(listing, remarks, demangle=None, ops=()):
    """{kernel name: {column: value}} with every column of COLUMNS, for the kernels of one listing and its remarks; with `ops` (mnemonics) each row
    also carries the count of each of them under its own name."""
    counts, regs = parse_listing(listing), parse_remarks(remarks)
    named = count_ops(listing, ops) if ops else {}
    names = (demangle or (lambda syms: {s: s for s in syms}))(sorted(counts))
    out = {}
    for sym, row in counts.items():
        if sym not in regs:
            raise ValueError(f"no resource remarks for kernel {sym}")
        out[short_name(names[sym])] = {**row, **regs[sym], **named.get(sym, {})}
    return out


def compile_file(src, flags=None, hipcc=None):
    """(listing, remarks) of substrata_amd/csrc/<src>, device side only, with `flags` (default: what build.py compiles the file with)."""
    from substrata_amd import build as b
    flags = list(b.source_flags(src) if flags is None else flags)
    with tempfile.TemporaryDirectory() as tmp:
        asm = os.path.join(tmp, "out.s")
        cmd = [hipcc or b.hipcc()] + flags + ["--cuda-device-only", "-S", "-Rpass-analysis=kernel-resource-usage", os.path.join(b.CSRC, src), "-o", asm]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError("hipcc failed: " + " ".join(cmd) + "\n" + r.stderr)
        with open(asm) as f:
            return f.read(), r.stderr


def resources(src, flags=None, ops=()):
    """the rows of one stage file; `ops`: mnemonics to count per kernel besides (resources(src, ops=("v_sqrt_f32", "v_rcp_f32"))[kernel]["v_sqrt_f32"])"""
    listing, remarks = compile_file(src, flags)
    return parse(listing, remarks, demangler(), ops)


def table(rows, before=None, ops=()):
    """markdown; with `before` (same shape) every cell reads 'before -> after' where the two differ; `ops`: one more column per counted mnemonic"""
    columns, headings = COLUMNS + tuple(ops), HEADINGS + tuple(f"`{o}`" for o in ops)
    lines = ["| kernel | " + " | ".join(headings) + " |", "|---|" + "---|" * len(headings)]
    for name, row in rows.items():
        cells = []
        for c in columns:
            old = before.get(name, {}).get(c) if before else None
            cells.append(f"{old} → {row[c]}" if old is not None and old != row[c] else str(row[c]))
        lines.append(f"| `{name}` | " + " | ".join(cells) + " |")
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("sources", nargs="+", help="stage files of substrata_amd/csrc/ (file names)")
    ap.add_argument("--flags", help="compile with this flag set instead of build.py's")
    ap.add_argument("--without", action="append", default=[], help="also compile with build.py's flags less this one and print before -> after")
    ap.add_argument("--kernels", help="regular expression: only kernels whose name matches")
    ap.add_argument("--ops", default="", help="comma-separated mnemonics to count per kernel in columns of their own, e.g. v_sqrt_f32,v_rcp_f32 (one per IEEE root / division)")
    a = ap.parse_args()
    from substrata_amd import build as b
    ops = tuple(o for o in a.ops.split(",") if o)
    for src in a.sources:
        flags = a.flags.split() if a.flags else b.source_flags(src)
        rows = resources(src, flags, ops)
        before = resources(src, [f for f in flags if f not in a.without], ops) if a.without else None
        if a.kernels:
            rows = {k: v for k, v in rows.items() if re.search(a.kernels, k)}
        print(f"\n{src}: {' '.join(flags)}" + (f"   (before: without {' '.join(a.without)})" if before else ""))
        print(table(rows, before, ops))


if __name__ == "__main__":
    main()
