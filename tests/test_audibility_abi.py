"""CPU-side checks of the audio sources' entry points (include/sgp.h, "batched audio sources") and of sgp_raycast_any: declared, exported and prototyped, the
seven structs have the library's sizes under NEW indices of sgp_abi_sizeof and their fields sit where the header puts them, NULL handles and bad capacities
are refused with a message, there is no batch without a device, and the facade header and the caller program compile.  No device."""
import ctypes as C
import os
import re
import subprocess

import pytest

from substrata_amd import abi, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STRUCTS = [("sgp_audibility_source", abi.AudibilitySource, 40), ("sgp_audibility_listener", abi.AudibilityListener, 48), ("sgp_audibility_event", abi.AudibilityEvent, 32),
           ("sgp_audibility_state", abi.AudibilityState, 24), ("sgp_audibility_pair_state", abi.AudibilityPairState, 12),
           ("sgp_audibility_listener_state", abi.AudibilityListenerState, 28), ("sgp_audibility_ramp", abi.AudibilityRamp, 32)]
FUNCTIONS = ["audibility_create", "audibility_destroy", "audibility_add", "audibility_remove", "audibility_set_points", "audibility_set_volume", "audibility_set_flags",
             "audibility_set_listener", "audibility_remove_listener", "audibility_set_listener_points", "audibility_set_listener_zone", "audibility_set_transition",
             "audibility_attach_proximity", "audibility_set_muting_keys", "audibility_update", "audibility_drain_events", "audibility_get_states",
             "audibility_get_pair_states", "audibility_get_listeners", "audibility_checkpoint", "audibility_rollback", "audibility_pair_ray", "audibility_ramp_step",
             "raycast_any"]
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
    for macro, value in (("SGP_AUD_SRC_POINT", abi.AUD_SRC_POINT), ("SGP_AUD_SRC_BODY", abi.AUD_SRC_BODY), ("SGP_AUD_LST_POINT", abi.AUD_LST_POINT),
                         ("SGP_AUD_LST_BODY", abi.AUD_LST_BODY), ("SGP_AUD_ONE_SHOT", abi.AUD_ONE_SHOT), ("SGP_AUD_WANT_RANGE", abi.AUD_WANT_RANGE),
                         ("SGP_AUD_WANT_OCCLUSION", abi.AUD_WANT_OCCLUSION), ("SGP_AUD_WANT_VOLUME", abi.AUD_WANT_VOLUME), ("SGP_AUD_ST_BODY_GONE", abi.AUD_ST_BODY_GONE),
                         ("SGP_AUD_LST_ST_BODY_GONE", abi.AUD_LST_ST_BODY_GONE), ("SGP_AUD_PAIR_IN_RANGE", abi.AUD_PAIR_IN_RANGE),
                         ("SGP_AUD_PAIR_OCCLUDED", abi.AUD_PAIR_OCCLUDED), ("SGP_BATCH_AUDIBILITY", abi.BATCH_AUDIBILITY)):
        assert re.search(r"#define %s\s+%du" % (macro, value), h), macro
    assert abi.BATCH_AUDIBILITY == 6
    for name, kind in abi.AUD_EV.items():
        assert re.search(r"#define SGP_AUD_EV_%s\s+%du" % (name, kind), h), name
    assert re.search(r"#define SGP_AUD_MAX_LISTENERS\s+32\b", h) and abi.AUD_MAX_LISTENERS == 32
    assert re.search(r"#define SGP_AUDIBILITY_MAX_SOURCES\s+\(1u << 20\)", h) and abi.AUDIBILITY_MAX_SOURCES == 1 << 20
    assert re.search(r"#define SGP_AUDIBILITY_MAX_PAIRS\s+\(1u << 22\)", h) and abi.AUDIBILITY_MAX_PAIRS == 1 << 22


def test_structs_have_the_library_sizes_under_new_indices(lib):
    idx = [abi.ABI_SIZEOF_ALL.index(s) for s, _, _ in STRUCTS]
    assert idx == [52, 53, 54, 55, 56, 57, 58]             # (51 answers -1 for good, as 21, 24, 29, 33, 37, 43 and 45 do)
    assert lib.sgp_abi_sizeof(51) == -1 and abi.ABI_SIZEOF_ALL[51] is None and lib.sgp_abi_sizeof(59) == -1
    for (struct, mirror, size), i in zip(STRUCTS, idx):
        assert lib.sgp_abi_sizeof(i) == C.sizeof(mirror) == C.sizeof(abi.STRUCTS[struct]) == size, struct
    for k, name in enumerate(abi.ABI_SIZEOF_ALL):      # nothing that was there before moved
        assert lib.sgp_abi_sizeof(k) == (C.sizeof(abi.STRUCTS[name]) if name is not None else -1), (k, name)
    assert abi.ABI_SIZEOF_ALL[45:51] == [None, "sgp_proximity_object", "sgp_proximity_observer", "sgp_proximity_event", "sgp_proximity_state", "sgp_proximity_observer_state"]
    assert lib.sgp_abi_version() == 1 == abi.ABI_VERSION
    assert (abi.audibility_source_dtype.itemsize, abi.audibility_event_dtype.itemsize, abi.audibility_state_dtype.itemsize, abi.audibility_pair_state_dtype.itemsize,
            abi.audibility_listener_state_dtype.itemsize) == (40, 32, 24, 12, 28)


def test_null_handles_and_bad_capacities_are_refused(lib):
    h = C.c_void_p()
    i = C.c_uint32(0)
    d = abi.AudibilitySource(volume=1.0)
    o = abi.AudibilityListener()
    st = abi.AudibilityState()
    ps = abi.AudibilityPairState()
    ls = abi.AudibilityListenerState()
    ev = abi.AudibilityEvent()
    v = (C.c_float * 3)(0, 0, 0)
    fake_world = C.c_void_p(0)
    assert lib.sgp_audibility_create(fake_world, 16, 4, 64, C.byref(h)) == abi.ERR_INVALID and not h.value
    assert b"sgp_audibility_create" in lib.sgp_last_error()
    assert lib.sgp_audibility_destroy(None) == abi.ERR_INVALID
    assert lib.sgp_audibility_add(None, C.addressof(d), 1, C.addressof(i)) == abi.ERR_INVALID
    assert b"sgp_audibility_add" in lib.sgp_last_error()
    assert lib.sgp_audibility_remove(None, 0) == abi.ERR_INVALID
    assert lib.sgp_audibility_set_points(None, 0, 1, C.addressof(v)) == abi.ERR_INVALID
    assert lib.sgp_audibility_set_volume(None, 0, 1.0) == abi.ERR_INVALID
    assert lib.sgp_audibility_set_flags(None, 0, 1) == abi.ERR_INVALID
    assert lib.sgp_audibility_set_listener(None, 0, C.byref(o)) == abi.ERR_INVALID
    assert lib.sgp_audibility_remove_listener(None, 0) == abi.ERR_INVALID
    assert lib.sgp_audibility_set_listener_points(None, 0, 1, C.addressof(v)) == abi.ERR_INVALID
    assert lib.sgp_audibility_set_listener_zone(None, 0, 1, 1) == abi.ERR_INVALID
    assert lib.sgp_audibility_set_transition(None, 1.0) == abi.ERR_INVALID
    assert lib.sgp_audibility_attach_proximity(None, None) == abi.ERR_INVALID
    assert lib.sgp_audibility_set_muting_keys(None, C.addressof(i), 1) == abi.ERR_INVALID
    assert lib.sgp_audibility_update(None, 0.0) == abi.ERR_INVALID
    assert b"sgp_audibility_update" in lib.sgp_last_error()
    assert lib.sgp_audibility_drain_events(None, C.addressof(ev), 1, C.byref(i), C.byref(i)) == abi.ERR_INVALID
    assert lib.sgp_audibility_get_states(None, 0, 1, C.addressof(st)) == abi.ERR_INVALID
    assert lib.sgp_audibility_get_pair_states(None, 0, 1, C.addressof(ps)) == abi.ERR_INVALID
    assert lib.sgp_audibility_get_listeners(None, 0, 1, C.addressof(ls)) == abi.ERR_INVALID
    assert lib.sgp_audibility_checkpoint(None, C.byref(h)) == abi.ERR_INVALID and not h.value
    assert lib.sgp_audibility_rollback(None, None) == abi.ERR_INVALID
    assert lib.sgp_raycast_any(None, None, 0, None) == abi.ERR_INVALID
    assert b"sgp_raycast_any" in lib.sgp_last_error()
    # capacities of 0 and beyond the limits -- the pair cap and the listener cap among them -- are refused before the world is looked at: the argument check
    # is one condition (sgp_world_audibility.hip) over aud_capacities_ok (sgp_audibility_host.h, exercised by tests/test_audibility_host.py)
    src = open(os.path.join(ROOT, "substrata_amd", "csrc", "sgp_world_audibility.hip")).read()
    assert "if (!w || !out || !aud_capacities_ok(source_capacity, listener_capacity, event_capacity)) return fail(SGP_ERR_INVALID" in src
    for sources, listeners, events in ((0, 4, 64), ((1 << 20) + 1, 1, 64), (16, 0, 64), (16, 33, 64), (16, 4, 0), (1 << 20, 5, 64), ((1 << 17) + 1, 32, 64)):
        assert lib.sgp_audibility_create(fake_world, sources, listeners, events, C.byref(h)) == abi.ERR_INVALID and not h.value
        assert b"2^22 pairs" in lib.sgp_last_error() and b"beyond 32" in lib.sgp_last_error()


def test_no_batch_without_a_device(lib):
    """Without a GPU there is no world to own a batch: sgp_world_create says SGP_ERR_NO_DEVICE, and the Python wrapper raises."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    from substrata_amd import lib as product
    from substrata_amd.world import SgpError
    with pytest.raises(SgpError):
        product.World(max_bodies=16).audibility(16, 4, 64)


def test_facade_header_compiles():
    """shim/AudibilityBatch.h on its own, as a caller would include it."""
    shim = os.path.join(ROOT, "substrata_amd", "shim")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-fsyntax-only", "-I", shim, "-x", "c++", os.path.join(shim, "AudibilityBatch.h")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_caller_program_compiles(tmp_path):
    from test_facade_gpu import build_facade_exe
    assert os.path.exists(build_facade_exe(tmp_path, "audibility_batch.cpp"))
