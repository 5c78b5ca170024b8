"""CPU-side checks of the shape-cast entry point (include/sgp.h, "shape casts with any convex shape"): declared, exported and prototyped, the two structs have
the library's sizes under NEW indices of sgp_abi_sizeof, their fields sit where the header puts them, and nothing that was there before moved.  No device."""
import ctypes as C
import os
import re

import pytest

from substrata_amd import abi, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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
    for ctype, names in re.findall(r"(float|int32_t|uint32_t|uint64_t)\s+([^;]+);", body):
        for nm in names.split(","):
            m = re.match(r"\s*(\w+)(?:\[(\d+)\])?\s*$", nm)
            out.append((m.group(1), ctype, int(m.group(2) or 1)))
    return out


SIZES = {"float": 4, "int32_t": 4, "uint32_t": 4, "uint64_t": 8}


@pytest.mark.parametrize("struct, mirror, size", [("sgp_shape_cast", abi.ShapeCast, 76), ("sgp_cast_hit", abi.CastHit, 56)])
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
    assert C.sizeof(mirror) == (off + align - 1) // align * align == size == np_itemsize(struct)


def np_itemsize(struct):
    return {"sgp_shape_cast": abi.shape_cast_dtype, "sgp_cast_hit": abi.cast_hit_dtype}[struct].itemsize


def test_declared_exported_and_prototyped(lib):
    h = header()
    assert re.search(r"int\s+sgp_cast_shapes\s*\(\s*sgp_world\s*\*\s*\w+\s*,\s*const\s+sgp_shape_cast\s*\*\s*\w+\s*,\s*uint32_t\s+\w+\s*,\s*sgp_cast_hit\s*\*", h)
    assert "#define SGP_CAST_TOLERANCE 1.0e-4f" in h and abi.CAST_TOLERANCE == 1.0e-4
    for name in ("cast_shapes", "cast_shapes_counters"):
        assert hasattr(lib, "sgp_" + name) and name in abi.PROTOTYPES


def test_structs_have_the_library_sizes_under_new_indices(lib):
    i, j = abi.ABI_SIZEOF_ALL.index("sgp_shape_cast"), abi.ABI_SIZEOF_ALL.index("sgp_cast_hit")
    assert (i, j) == (22, 23)                      # (21 answers -1 for good: the end of the list as bindings of the 21 earlier structs probe it)
    assert lib.sgp_abi_sizeof(21) == -1 and lib.sgp_abi_sizeof(24) == -1
    assert lib.sgp_abi_sizeof(i) == C.sizeof(abi.ShapeCast) == C.sizeof(abi.STRUCTS["sgp_shape_cast"])
    assert lib.sgp_abi_sizeof(j) == C.sizeof(abi.CastHit) == C.sizeof(abi.STRUCTS["sgp_cast_hit"])
    for k, name in enumerate(abi.ABI_SIZEOF_ALL):
        if name is not None:
            assert lib.sgp_abi_sizeof(k) == C.sizeof(abi.STRUCTS[name]), name
    assert lib.sgp_abi_version() == 1 == abi.ABI_VERSION


def test_null_arguments_are_invalid_without_a_device(lib):
    assert lib.sgp_cast_shapes(None, None, 0, None) == abi.ERR_INVALID
    assert b"sgp_cast_shapes" in lib.sgp_last_error()
