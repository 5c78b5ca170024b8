"""CPU-side checks of the batched path and move-to controllers' entry points (include/sgp.h, "batched path and move-to controllers"): declared, exported and
prototyped, the five structs have the library's sizes under NEW indices of sgp_abi_sizeof and their fields sit where the header puts them, NULL handles and bad
capacities are refused, there is no batch without a device, and the facade header and the caller program compile.  No device."""
import ctypes as C
import os
import re
import subprocess

import pytest

from substrata_amd import abi, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STRUCTS = [("sgp_path_waypoint", abi.PathWaypoint, 24), ("sgp_path_segment", abi.PathSegment, 56), ("sgp_path_progress", abi.PathProgress, 12),
           ("sgp_mover_desc", abi.MoverDesc, 88), ("sgp_mover_state", abi.MoverState, 68)]
FUNCTIONS = ["path_prepare", "path_advance", "movers_create", "movers_destroy", "movers_path_add", "movers_path_remove", "movers_path_get", "mover_add", "mover_remove",
             "movers_set_position_track", "movers_set_rotation_track", "movers_update", "movers_get_states"]
SIZES = {"float": 4, "int32_t": 4, "uint32_t": 4, "uint64_t": 8, "double": 8}


@pytest.fixture(scope="module")
def lib():
    lib = C.CDLL(build.build())
    abi.bind(lib, "sgp_")
    return lib


def header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sgp.h")).read(), flags=re.S)


def header_fields(struct):
    """(name, C type, array length) of the members of `typedef struct <struct> { ... }`, in order."""
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), header(), flags=re.S).group(1)
    out = []
    for ctype, names in re.findall(r"(float|double|int32_t|uint32_t|uint64_t)\s+([^;]+);", body):
        for nm in names.split(","):
            m = re.match(r"\s*(\w+)(?:\[(\d+)\])?\s*$", nm)
            out.append((m.group(1), ctype, int(m.group(2) or 1)))
    return out


@pytest.mark.parametrize("struct, mirror, size", STRUCTS)
def test_field_offsets_follow_the_header(struct, mirror, size):
    fields = header_fields(struct)
    assert [f[0] for f in fields] == [n for n, _ in mirror._fields_]
    off = 0
    for name, ctype, count in fields:
        a = SIZES[ctype]
        off = (off + a - 1) // a * a
        assert getattr(mirror, name).offset == off and getattr(mirror, name).size == a * count, name
        off += a * count
    align = max(SIZES[f[1]] for f in fields)
    assert C.sizeof(mirror) == (off + align - 1) // align * align == size


def test_declared_exported_and_prototyped(lib):
    h = header()
    for name in FUNCTIONS:
        assert re.search(r"\bsgp_%s\s*\(" % name, h), name
        assert hasattr(lib, "sgp_" + name) and name in abi.PROTOTYPES, name
    for macro, value in (("SGP_MOVER_PATH", abi.MOVER_PATH), ("SGP_MOVER_MOVETO", abi.MOVER_MOVETO), ("SGP_WAYPOINT_CURVE_IN", abi.WAYPOINT_CURVE_IN),
                         ("SGP_WAYPOINT_CURVE_OUT", abi.WAYPOINT_CURVE_OUT), ("SGP_WAYPOINT_STATION", abi.WAYPOINT_STATION), ("SGP_MOVER_EASE_LINEAR", abi.MOVER_EASE_LINEAR),
                         ("SGP_MOVER_EASE_SMOOTHSTEP", abi.MOVER_EASE_SMOOTHSTEP), ("SGP_MOVER_ORIENT_ALONG_PATH", abi.MOVER_ORIENT_ALONG_PATH)):
        assert re.search(r"#define %s\s+%du" % (macro, value), h), macro
    for name, bit in abi.MOVER_ST.items():
        assert re.search(r"#define SGP_MOVER_ST_%s\s+%du" % (name, bit), h), name
    assert re.search(r"#define SGP_MOVER_MAX_WAYPOINTS\s+128\b", h) and abi.MOVER_MAX_WAYPOINTS == 128
    assert re.search(r"#define SGP_MOVER_MAX_SEGMENTS_PER_UPDATE\s+64\b", h) and abi.MOVER_MAX_SEGMENTS_PER_UPDATE == 64
    assert re.search(r"#define SGP_MOVERS_MAX_CAPACITY\s+\(1u << 16\)", h) and abi.MOVERS_MAX_CAPACITY == 1 << 16
    assert re.search(r"#define SGP_MOVERS_MAX_PATHS\s+\(1u << 12\)", h) and abi.MOVERS_MAX_PATHS == 1 << 12


def test_structs_have_the_library_sizes_under_new_indices(lib):
    idx = [abi.ABI_SIZEOF_ALL.index(s) for s, _, _ in STRUCTS]
    assert idx == [38, 39, 40, 41, 42]             # (37 answers -1 for good, as 21, 24, 29 and 33 do)
    assert lib.sgp_abi_sizeof(37) == -1 and abi.ABI_SIZEOF_ALL[37] is None
    for (struct, mirror, size), i in zip(STRUCTS, idx):
        assert lib.sgp_abi_sizeof(i) == C.sizeof(mirror) == C.sizeof(abi.STRUCTS[struct]) == size, struct
    for k, name in enumerate(abi.ABI_SIZEOF_ALL):      # nothing that was there before moved
        assert lib.sgp_abi_sizeof(k) == (C.sizeof(abi.STRUCTS[name]) if name is not None else -1), (k, name)
    assert abi.ABI_SIZEOF_ALL[33:37] == [None, "sgp_craft_desc", "sgp_craft_input", "sgp_craft_state"]
    assert lib.sgp_abi_version() == 1 == abi.ABI_VERSION
    assert (abi.path_waypoint_dtype.itemsize, abi.path_segment_dtype.itemsize, abi.mover_state_dtype.itemsize) == (24, 56, 68)


def test_null_handles_and_bad_capacities_are_refused(lib):
    h = C.c_void_p()
    i = C.c_uint32(0)
    d = abi.MoverDesc()
    st = abi.MoverState()
    wp = (abi.PathWaypoint * 2)()
    seg = (abi.PathSegment * 2)()
    total = C.c_double(0.0)
    prog = abi.PathProgress()
    v = (C.c_float * 4)(0, 0, 0, 1)
    fake_world = C.c_void_p(0)
    assert lib.sgp_movers_create(fake_world, 16, 4, C.byref(h)) == abi.ERR_INVALID and not h.value
    assert b"sgp_movers_create" in lib.sgp_last_error()
    assert lib.sgp_movers_destroy(None) == abi.ERR_INVALID
    assert lib.sgp_movers_path_add(None, wp, 2, C.byref(i)) == abi.ERR_INVALID
    assert lib.sgp_movers_path_remove(None, 0) == abi.ERR_INVALID
    assert lib.sgp_movers_path_get(None, 0, seg, 2, C.byref(i)) == abi.ERR_INVALID
    assert lib.sgp_mover_add(None, C.byref(d), C.byref(i)) == abi.ERR_INVALID
    assert lib.sgp_mover_remove(None, 0) == abi.ERR_INVALID
    assert lib.sgp_movers_set_position_track(None, 0, v, v, 1.0, 0, 0.0) == abi.ERR_INVALID
    assert lib.sgp_movers_set_rotation_track(None, 0, v, v, 1.0, 0, 0.0) == abi.ERR_INVALID
    assert lib.sgp_movers_update(None, 1.0 / 60.0) == abi.ERR_INVALID
    assert b"sgp_movers_update" in lib.sgp_last_error()
    assert lib.sgp_movers_get_states(None, 0, 1, C.byref(st)) == abi.ERR_INVALID
    assert lib.sgp_path_prepare(None, 2, seg, C.byref(total)) == abi.ERR_INVALID
    assert lib.sgp_path_prepare(wp, 2, None, C.byref(total)) == abi.ERR_INVALID
    assert lib.sgp_path_advance(None, 2, C.byref(prog), 0.1, C.byref(i)) == abi.ERR_INVALID
    # capacities of 0 and beyond the limits are refused before the world is looked at (the argument check is one condition: sgp_world_movers.hip)
    src = open(os.path.join(ROOT, "substrata_amd", "csrc", "sgp_world_movers.hip")).read()
    assert "if (!w || !out || capacity == 0 || capacity > SGP_MOVERS_MAX_CAPACITY || path_capacity == 0 || path_capacity > SGP_MOVERS_MAX_PATHS) return fail(SGP_ERR_INVALID" in src
    for cap, paths in ((0, 4), ((1 << 16) + 1, 4), (16, 0), (16, (1 << 12) + 1)):
        assert lib.sgp_movers_create(fake_world, cap, paths, C.byref(h)) == abi.ERR_INVALID and not h.value


def test_no_batch_without_a_device(lib):
    """Without a GPU there is no world to own a batch: sgp_world_create says SGP_ERR_NO_DEVICE, and the Python wrapper raises."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    from substrata_amd import lib as product
    from substrata_amd.world import SgpError
    with pytest.raises(SgpError):
        product.World(max_bodies=16).movers(16, 4)


def test_facade_header_compiles():
    """shim/MoverBatch.h on its own, as a caller would include it."""
    shim = os.path.join(ROOT, "substrata_amd", "shim")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-fsyntax-only", "-I", shim, "-x", "c++", os.path.join(shim, "MoverBatch.h")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_caller_program_compiles(tmp_path):
    from test_facade_gpu import build_facade_exe
    assert os.path.exists(build_facade_exe(tmp_path, "movers_batch.cpp"))
