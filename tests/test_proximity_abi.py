"""CPU-side checks of the proximity and zone watchers' entry points (include/sgp.h, "batched proximity and zone watchers"): declared, exported and prototyped,
the five structs have the library's sizes under NEW indices of sgp_abi_sizeof and their fields sit where the header puts them, NULL handles and bad capacities
are refused, there is no batch without a device, and the facade header and the caller program compile.  No device."""
import ctypes as C
import os
import re
import subprocess

import pytest

from substrata_amd import abi, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STRUCTS = [("sgp_proximity_object", abi.ProximityObject, 24), ("sgp_proximity_observer", abi.ProximityObserver, 32), ("sgp_proximity_event", abi.ProximityEvent, 32),
           ("sgp_proximity_state", abi.ProximityState, 8), ("sgp_proximity_observer_state", abi.ProximityObserverState, 24)]
FUNCTIONS = ["proximity_create", "proximity_destroy", "proximity_add", "proximity_remove", "proximity_set_flags", "proximity_set_observer", "proximity_set_points",
             "proximity_remove_observer", "proximity_zone_add", "proximity_zone_remove", "proximity_update", "proximity_drain_events", "proximity_get_states",
             "proximity_get_observers", "proximity_checkpoint", "proximity_rollback", "proximity_test_point", "proximity_pick_zone"]
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
    for macro, value in (("SGP_PROX_WANT_NEAR", abi.PROX_WANT_NEAR), ("SGP_PROX_WANT_ZONE", abi.PROX_WANT_ZONE), ("SGP_PROX_OBS_POINT", abi.PROX_OBS_POINT),
                         ("SGP_PROX_OBS_BODY", abi.PROX_OBS_BODY), ("SGP_PROX_ST_BODY_GONE", abi.PROX_ST_BODY_GONE), ("SGP_PROX_OBS_ST_BODY_GONE", abi.PROX_OBS_ST_BODY_GONE),
                         ("SGP_BATCH_PROXIMITY", abi.BATCH_PROXIMITY)):
        assert re.search(r"#define %s\s+%du" % (macro, value), h), macro
    for name, kind in abi.PROX_EV.items():
        assert re.search(r"#define SGP_PROX_EV_%s\s+%du" % (name, kind), h), name
    assert re.search(r"#define SGP_PROX_MAX_OBSERVERS\s+32\b", h) and abi.PROX_MAX_OBSERVERS == 32
    assert re.search(r"#define SGP_PROXIMITY_MAX_OBJECTS\s+\(1u << 20\)", h) and abi.PROXIMITY_MAX_OBJECTS == 1 << 20
    assert re.search(r"#define SGP_PROXIMITY_MAX_ZONES\s+\(1u << 12\)", h) and abi.PROXIMITY_MAX_ZONES == 1 << 12


def test_structs_have_the_library_sizes_under_new_indices(lib):
    idx = [abi.ABI_SIZEOF_ALL.index(s) for s, _, _ in STRUCTS]
    assert idx == [46, 47, 48, 49, 50]             # (45 answers -1 for good, as 21, 24, 29, 33, 37 and 43 do)
    assert lib.sgp_abi_sizeof(45) == -1 and abi.ABI_SIZEOF_ALL[45] is None and lib.sgp_abi_sizeof(51) == -1
    for (struct, mirror, size), i in zip(STRUCTS, idx):
        assert lib.sgp_abi_sizeof(i) == C.sizeof(mirror) == C.sizeof(abi.STRUCTS[struct]) == size, struct
    for k, name in enumerate(abi.ABI_SIZEOF_ALL):      # nothing that was there before moved
        assert lib.sgp_abi_sizeof(k) == (C.sizeof(abi.STRUCTS[name]) if name is not None else -1), (k, name)
    assert abi.ABI_SIZEOF_ALL[43:45] == [None, "sgp_batch_checkpoint_info"]
    assert lib.sgp_abi_version() == 1 == abi.ABI_VERSION
    assert (abi.proximity_object_dtype.itemsize, abi.proximity_event_dtype.itemsize, abi.proximity_state_dtype.itemsize, abi.proximity_observer_state_dtype.itemsize) == (24, 32, 8, 24)


def test_null_handles_and_bad_capacities_are_refused(lib):
    h = C.c_void_p()
    i = C.c_uint32(0)
    d = abi.ProximityObject(body=0, radius=20.0)
    o = abi.ProximityObserver()
    st = abi.ProximityState()
    os_ = abi.ProximityObserverState()
    ev = abi.ProximityEvent()
    v = (C.c_float * 3)(0, 0, 0)
    f = C.c_float(0)
    fake_world = C.c_void_p(0)
    assert lib.sgp_proximity_create(fake_world, 16, 4, 64, C.byref(h)) == abi.ERR_INVALID and not h.value
    assert b"sgp_proximity_create" in lib.sgp_last_error()
    assert lib.sgp_proximity_destroy(None) == abi.ERR_INVALID
    assert lib.sgp_proximity_add(None, C.addressof(d), 1, C.addressof(i)) == abi.ERR_INVALID
    assert lib.sgp_proximity_remove(None, 0) == abi.ERR_INVALID
    assert lib.sgp_proximity_set_flags(None, 0, 1) == abi.ERR_INVALID
    assert lib.sgp_proximity_set_observer(None, 0, C.byref(o)) == abi.ERR_INVALID
    assert lib.sgp_proximity_set_points(None, 0, 1, C.addressof(v)) == abi.ERR_INVALID
    assert lib.sgp_proximity_remove_observer(None, 0) == abi.ERR_INVALID
    assert lib.sgp_proximity_zone_add(None, v, v, 1, C.byref(i)) == abi.ERR_INVALID
    assert lib.sgp_proximity_zone_remove(None, 0) == abi.ERR_INVALID
    assert lib.sgp_proximity_update(None) == abi.ERR_INVALID
    assert b"sgp_proximity_update" in lib.sgp_last_error()
    assert lib.sgp_proximity_drain_events(None, C.addressof(ev), 1, C.byref(i), C.byref(i)) == abi.ERR_INVALID
    assert lib.sgp_proximity_get_states(None, 0, 1, C.addressof(st)) == abi.ERR_INVALID
    assert lib.sgp_proximity_get_observers(None, 0, 1, C.addressof(os_)) == abi.ERR_INVALID
    assert lib.sgp_proximity_checkpoint(None, C.byref(h)) == abi.ERR_INVALID and not h.value
    assert lib.sgp_proximity_rollback(None, None) == abi.ERR_INVALID
    assert lib.sgp_proximity_test_point(None, v, v, 1.0, C.byref(i), C.byref(f)) == abi.ERR_INVALID
    assert lib.sgp_proximity_test_point(v, v, v, 1.0, None, C.byref(f)) == abi.ERR_INVALID
    assert lib.sgp_proximity_pick_zone(C.addressof(v), C.addressof(v), None, C.addressof(i), 1, 0, v, C.byref(i)) == abi.ERR_INVALID
    assert lib.sgp_proximity_pick_zone(None, None, None, None, 0, abi.INVALID_ID, v, C.byref(i)) == abi.OK and i.value == abi.INVALID_ID      # no zones: none
    # capacities of 0 and beyond the limits are refused before the world is looked at (the argument check is one condition: sgp_world_proximity.hip)
    src = open(os.path.join(ROOT, "substrata_amd", "csrc", "sgp_world_proximity.hip")).read()
    assert ("if (!w || !out || object_capacity == 0 || object_capacity > SGP_PROXIMITY_MAX_OBJECTS || zone_capacity == 0 || zone_capacity > SGP_PROXIMITY_MAX_ZONES || "
            "event_capacity == 0) return fail(SGP_ERR_INVALID") in src
    for objects, zones, events in ((0, 4, 64), ((1 << 20) + 1, 4, 64), (16, 0, 64), (16, (1 << 12) + 1, 64), (16, 4, 0)):
        assert lib.sgp_proximity_create(fake_world, objects, zones, events, C.byref(h)) == abi.ERR_INVALID and not h.value


def test_no_batch_without_a_device(lib):
    """Without a GPU there is no world to own a batch: sgp_world_create says SGP_ERR_NO_DEVICE, and the Python wrapper raises."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    from substrata_amd import lib as product
    from substrata_amd.world import SgpError
    with pytest.raises(SgpError):
        product.World(max_bodies=16).proximity(16, 4, 64)


def test_facade_header_compiles():
    """shim/ProximityBatch.h on its own, as a caller would include it."""
    shim = os.path.join(ROOT, "substrata_amd", "shim")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-fsyntax-only", "-I", shim, "-x", "c++", os.path.join(shim, "ProximityBatch.h")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_caller_program_compiles(tmp_path):
    from test_facade_gpu import build_facade_exe
    assert os.path.exists(build_facade_exe(tmp_path, "proximity_batch.cpp"))
