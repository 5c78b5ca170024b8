"""CPU-side checks of the batched hover cars' and boats' entry points (include/sgp.h, "batched hover cars and boats"): declared, exported and prototyped,
the three structs have the library's sizes under NEW indices of sgp_abi_sizeof and their fields sit where the header puts them, the defaults are those of
the reference's script settings, NULL handles and bad capacities are refused, there is no batch without a device, and the facade header and the caller
program compile.  No device."""
import ctypes as C
import os
import re
import subprocess

import pytest

from substrata_amd import abi, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STRUCTS = [("sgp_craft_desc", abi.CraftDesc, 248), ("sgp_craft_input", abi.CraftInput, 20), ("sgp_craft_state", abi.CraftState, 72)]
FUNCTIONS = ["default_craft_desc", "crafts_create", "crafts_destroy", "craft_add", "craft_remove", "crafts_set_inputs", "crafts_start_righting",
             "crafts_attach_particles", "crafts_update", "crafts_get_states"]
SIZES = {"float": 4, "int32_t": 4, "uint32_t": 4, "uint64_t": 8}


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
    for macro, value in (("SGP_CRAFT_HOVERCAR", abi.CRAFT_HOVERCAR), ("SGP_CRAFT_BOAT", abi.CRAFT_BOAT), ("SGP_CRAFT_IN_DRIVER", abi.CRAFT_IN_DRIVER),
                         ("SGP_CRAFT_IN_BOOST", abi.CRAFT_IN_BOOST), ("SGP_CRAFT_ST_BODY_GONE", abi.CRAFT_ST_BODY_GONE), ("SGP_CRAFT_PK_SPRAY", abi.CRAFT_PK_SPRAY),
                         ("SGP_CRAFT_PK_DUST", abi.CRAFT_PK_DUST), ("SGP_CRAFT_PK_JET", abi.CRAFT_PK_JET), ("SGP_CRAFT_PK_SPLASH", abi.CRAFT_PK_SPLASH)):
        assert re.search(r"#define %s\s+%du" % (macro, value), h), macro
    for name, bit in abi.CRAFT_BR.items():
        assert re.search(r"#define SGP_CRAFT_BR_%s\s+\(1u << %d\)" % (name, bit.bit_length() - 1), h), name
    assert re.search(r"#define SGP_CRAFT_MAX_SPLASH_POINTS\s+8\b", h) and abi.CRAFT_MAX_SPLASH_POINTS == 8
    assert re.search(r"#define SGP_CRAFT_MAX_EMIT\s+22\b", h) and abi.CRAFT_MAX_EMIT == 22 == 6 + 2 * abi.CRAFT_MAX_SPLASH_POINTS
    assert re.search(r"#define SGP_CRAFTS_MAX_CAPACITY\s+\(1u << 16\)", h) and abi.CRAFTS_MAX_CAPACITY == 1 << 16
    assert "use_zero_linear_drag = 1" in open(os.path.join(ROOT, "include", "sgp.h")).read()      # (the header tells the caller how to create a boat's body)


def test_structs_have_the_library_sizes_under_new_indices(lib):
    idx = [abi.ABI_SIZEOF_ALL.index(s) for s, _, _ in STRUCTS]
    assert idx == [34, 35, 36]                     # (33 answers -1 for good, as 21, 24 and 29 do)
    assert lib.sgp_abi_sizeof(33) == -1 and lib.sgp_abi_sizeof(37) == -1
    for (struct, mirror, size), i in zip(STRUCTS, idx):
        assert lib.sgp_abi_sizeof(i) == C.sizeof(mirror) == C.sizeof(abi.STRUCTS[struct]) == size, struct
    for k, name in enumerate(abi.ABI_SIZEOF_ALL):      # nothing that was there before moved
        assert lib.sgp_abi_sizeof(k) == (C.sizeof(abi.STRUCTS[name]) if name is not None else -1), (k, name)
    assert abi.ABI_SIZEOF_ALL[:33] == abi.ABI_SIZEOF_ORDER + ["sgp_shape_query", None, "sgp_shape_cast", "sgp_cast_hit", None, "sgp_character_desc", "sgp_character_input",
                                                               "sgp_character_state", "sgp_character_contact", None, "sgp_particle", "sgp_particle_state", "sgp_particle_event"]
    assert lib.sgp_abi_version() == 1 == abi.ABI_VERSION
    assert (abi.craft_desc_dtype.itemsize, abi.craft_input_dtype.itemsize, abi.craft_state_dtype.itemsize) == (248, 20, 72)


def test_defaults_are_those_of_the_script_settings(lib):
    """Scripting.cpp:229-239: thrust 40000, propellor (0, 0.2, -6.2), offset 1, rudder factor 500, lateral 0, jet width 1, areas 2 / 4 / 8."""
    f32 = lambda x: C.c_float(x).value
    for kind in (abi.CRAFT_HOVERCAR, abi.CRAFT_BOAT):
        d = abi.CraftDesc()
        C.memset(C.byref(d), 0xFF, C.sizeof(d))
        lib.sgp_default_craft_desc(kind, C.byref(d))
        lib.sgp_default_craft_desc(kind, None)      # (returns)
        assert d.kind == kind and d.body == abi.INVALID_ID and d.mass == 1000.0 and d.seed == 0 and d.tag == 0 and d.n_splash_points == 0
        assert tuple(d.model_to_y_forwards_rot_1) == tuple(d.model_to_y_forwards_rot_2) == (0.0, 0.0, 0.0, 1.0)
        assert tuple(d.trace_origin_os) == (0.0, 0.0, 0.0) and not any(d.splash_points) and d.shape_volume == 0.0
        if kind == abi.CRAFT_BOAT:
            assert (d.thrust_force, d.propellor_sideways_offset, d.rudder_deflection_force_factor, d.thrust_vector_lateral_amount, d.jet_particle_initial_width) == (40000.0, 1.0, 500.0, 0.0, 1.0)
            assert tuple(d.propellor_point_os) == (0.0, f32(0.2), f32(-6.2))
            assert (d.front_cross_sectional_area, d.side_cross_sectional_area, d.top_cross_sectional_area) == (2.0, 4.0, 8.0)
        else:
            assert d.thrust_force == 0.0 and d.top_cross_sectional_area == 0.0


def test_null_handles_and_bad_capacities_are_refused(lib):
    h = C.c_void_p()
    i = C.c_uint32(0)
    d = abi.CraftDesc()
    lib.sgp_default_craft_desc(abi.CRAFT_BOAT, C.byref(d))
    inp = abi.CraftInput()
    st = abi.CraftState()
    fake_world = C.c_void_p(0)
    assert lib.sgp_crafts_create(fake_world, 16, C.byref(h)) == abi.ERR_INVALID and not h.value
    assert b"sgp_crafts_create" in lib.sgp_last_error()
    assert lib.sgp_crafts_destroy(None) == abi.ERR_INVALID
    assert lib.sgp_craft_add(None, C.byref(d), C.byref(i)) == abi.ERR_INVALID
    assert lib.sgp_craft_remove(None, 0) == abi.ERR_INVALID
    assert lib.sgp_crafts_set_inputs(None, 0, 1, C.byref(inp)) == abi.ERR_INVALID
    assert lib.sgp_crafts_start_righting(None, C.byref(i), 1) == abi.ERR_INVALID
    assert lib.sgp_crafts_attach_particles(None, None) == abi.ERR_INVALID
    assert lib.sgp_crafts_update(None, 1.0 / 60.0) == abi.ERR_INVALID
    assert b"sgp_crafts_update" in lib.sgp_last_error()
    assert lib.sgp_crafts_get_states(None, 0, 1, C.byref(st)) == abi.ERR_INVALID
    # capacity 0 and capacity beyond 2^16 are refused before the world is looked at (the argument check is one condition: sgp_world_crafts.hip)
    src = open(os.path.join(ROOT, "substrata_amd", "csrc", "sgp_world_crafts.hip")).read()
    assert "if (!w || !out || capacity == 0 || capacity > SGP_CRAFTS_MAX_CAPACITY) return fail(SGP_ERR_INVALID" in src
    for cap in (0, (1 << 16) + 1):
        assert lib.sgp_crafts_create(fake_world, cap, C.byref(h)) == abi.ERR_INVALID and not h.value


def test_no_batch_without_a_device(lib):
    """Without a GPU there is no world to own a batch: sgp_world_create says SGP_ERR_NO_DEVICE, and the Python wrapper raises."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    d = abi.WorldDesc()
    lib.sgp_default_world_desc(C.byref(d))
    w = C.c_void_p()
    assert lib.sgp_world_create(C.byref(d), C.byref(w)) == abi.ERR_NO_DEVICE and not w.value
    assert b"no CPU fallback" in lib.sgp_last_error()
    from substrata_amd import lib as product
    from substrata_amd.world import SgpError
    with pytest.raises(SgpError):
        product.World(max_bodies=16).crafts(16)


def test_facade_header_compiles():
    """shim/CraftBatch.h on its own, as a caller would include it."""
    shim = os.path.join(ROOT, "substrata_amd", "shim")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-fsyntax-only", "-I", shim, "-x", "c++", os.path.join(shim, "CraftBatch.h")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_caller_program_compiles(tmp_path):
    from test_facade_gpu import build_facade_exe
    assert os.path.exists(build_facade_exe(tmp_path, "crafts_batch.cpp"))
