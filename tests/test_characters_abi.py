"""CPU-side checks of the batched character controller's entry points (include/sgp.h, "batched virtual characters"): declared, exported and prototyped, the four
structs have the library's sizes under NEW indices of sgp_abi_sizeof and their fields sit where the header puts them, the defaults are those of
shim/Jolt/JoltCharacterLite.h, NULL handles are refused, and the facade header compiles.  No device."""
import ctypes as C
import math
import os
import re
import subprocess

import pytest

from substrata_amd import abi, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STRUCTS = [("sgp_character_desc", abi.CharacterDesc, 136), ("sgp_character_input", abi.CharacterInput, 20),
           ("sgp_character_state", abi.CharacterState, 88), ("sgp_character_contact", abi.CharacterContact, 48)]
FUNCTIONS = ["default_character_desc", "characters_create", "characters_destroy", "character_add", "character_remove", "characters_set_pose",
             "characters_set_shape", "characters_set_inputs", "characters_update", "characters_get_states", "characters_drain_contacts"]


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
    for macro, value in (("SGP_CHAR_EXTENDED", abi.CHAR_EXTENDED), ("SGP_CHAR_NO_SLIDE", abi.CHAR_NO_SLIDE), ("SGP_CHAR_DISABLED", abi.CHAR_DISABLED)):
        assert re.search(r"#define %s\s+%du" % (macro, value), h), macro
    # the four values of CharacterBase::EGroundState, in its order
    order = re.search(r"enum class EGroundState \{([^}]*)\}", open(os.path.join(ROOT, "substrata_amd", "shim", "Jolt", "JoltCharacterLite.h")).read()).group(1)
    assert [s.strip() for s in order.split(",")] == ["OnGround", "OnSteepGround", "NotSupported", "InAir"]
    assert (abi.GROUND_ON_GROUND, abi.GROUND_ON_STEEP_GROUND, abi.GROUND_NOT_SUPPORTED, abi.GROUND_IN_AIR) == (0, 1, 2, 3)
    for macro, value in (("SGP_GROUND_ON_GROUND", 0), ("SGP_GROUND_ON_STEEP_GROUND", 1), ("SGP_GROUND_NOT_SUPPORTED", 2), ("SGP_GROUND_IN_AIR", 3)):
        assert re.search(r"#define %s\s+%d\b" % (macro, value), h), macro


def test_structs_have_the_library_sizes_under_new_indices(lib):
    idx = [abi.ABI_SIZEOF_ALL.index(s) for s, _, _ in STRUCTS]
    assert idx == [25, 26, 27, 28]                 # (24 answers -1 for good, as 21 does: the end of the list as earlier bindings probe it)
    assert lib.sgp_abi_sizeof(24) == -1 and lib.sgp_abi_sizeof(21) == -1 and lib.sgp_abi_sizeof(29) == -1
    for (struct, mirror, size), i in zip(STRUCTS, idx):
        assert lib.sgp_abi_sizeof(i) == C.sizeof(mirror) == C.sizeof(abi.STRUCTS[struct]) == size, struct
    for k, name in enumerate(abi.ABI_SIZEOF_ALL):      # nothing that was there before moved
        if name is not None:
            assert lib.sgp_abi_sizeof(k) == C.sizeof(abi.STRUCTS[name]), name
    assert lib.sgp_abi_version() == 1 == abi.ABI_VERSION
    assert abi.character_state_dtype.itemsize == 88 and abi.character_input_dtype.itemsize == 20 and abi.character_contact_dtype.itemsize == 48


def test_defaults_are_those_of_the_host_character(lib):
    """JoltCharacterLite.h:33 (CharacterShape), :67-78 (CharacterVirtualSettings), :89-94 (ExtendedUpdateSettings)."""
    f32 = lambda x: C.c_float(x).value
    d = abi.CharacterDesc()
    lib.sgp_default_character_desc(C.byref(d))
    assert (d.radius, d.half_height, tuple(d.shape_offset)) == (f32(0.3), f32(0.65), (0.0, 0.0, 0.0))
    assert tuple(d.up) == (0.0, 1.0, 0.0)
    assert tuple(d.supporting_plane) == (0.0, 0.0, 1.0, f32(1.0e10))
    assert d.max_slope_angle == f32(f32(f32(50.0) * f32(3.14159265)) / 180.0) and abs(math.degrees(d.max_slope_angle) - 50.0) < 1e-4
    assert (d.mass, d.max_strength) == (70.0, 100.0)
    assert (d.predictive_contact_distance, d.character_padding, d.penetration_recovery_speed, d.collision_tolerance) == (f32(0.1), f32(0.02), 1.0, f32(1.0e-3))
    assert (d.max_collision_iterations, d.max_constraint_iterations, d.min_time_remaining) == (5, 15, f32(1.0e-4))
    assert tuple(d.stick_to_floor_step_down) == (0.0, -0.5, 0.0) and tuple(d.walk_stairs_step_up) == (0.0, f32(0.4), 0.0)
    assert (d.walk_stairs_min_step_forward, d.walk_stairs_step_forward_test, d.walk_stairs_cos_angle_forward_contact) == (f32(0.02), f32(0.15), f32(0.2588))
    assert tuple(d.walk_stairs_step_down_extra) == (0.0, 0.0, 0.0)
    # ... and the header they are taken from still says so
    src = open(os.path.join(ROOT, "substrata_amd", "shim", "Jolt", "JoltCharacterLite.h")).read()
    for text in ("radius = 0.3f, half_height = 0.65f", "mUp = Vec3(0, 1, 0)", "n(0, 0, 1), c(1.0e10f)", "mMaxSlopeAngle = 50.0f * 3.14159265f / 180.0f", "mMass = 70.0f, mMaxStrength = 100.0f",
                 "mPredictiveContactDistance = 0.1f, mCharacterPadding = 0.02f, mPenetrationRecoverySpeed = 1.0f, mCollisionTolerance = 1.0e-3f",
                 "mMaxCollisionIterations = 5, mMaxConstraintIterations = 15", "mMinTimeRemaining = 1.0e-4f", "mStickToFloorStepDown = Vec3(0, -0.5f, 0), mWalkStairsStepUp = Vec3(0, 0.4f, 0)",
                 "mWalkStairsMinStepForward = 0.02f, mWalkStairsStepForwardTest = 0.15f, mWalkStairsCosAngleForwardContact = 0.2588f", "mWalkStairsStepDownExtra = Vec3(0, 0, 0)"):
        assert text in src, text


def test_null_arguments_are_invalid_without_a_device(lib):
    h = C.c_void_p()
    d = abi.CharacterDesc()
    lib.sgp_default_character_desc(C.byref(d))
    lib.sgp_default_character_desc(None)      # (returns)
    pos = (C.c_float * 3)(0, 0, 0)
    i = C.c_uint32(0)
    n = C.c_uint32(0)
    assert lib.sgp_characters_create(None, 16, C.byref(h)) == abi.ERR_INVALID and not h.value
    assert b"sgp_characters_create" in lib.sgp_last_error()
    assert lib.sgp_characters_destroy(None) == abi.ERR_INVALID
    assert lib.sgp_character_add(None, C.byref(d), pos, C.byref(i)) == abi.ERR_INVALID
    assert lib.sgp_character_remove(None, 0) == abi.ERR_INVALID
    assert lib.sgp_characters_set_pose(None, None, None, 0) == abi.ERR_INVALID
    assert lib.sgp_characters_set_shape(None, 0, 0.3, 0.65, pos) == abi.ERR_INVALID
    assert lib.sgp_characters_set_inputs(None, 0, 0, None) == abi.ERR_INVALID
    assert lib.sgp_characters_update(None, 1.0 / 60.0) == abi.ERR_INVALID
    assert b"sgp_characters_update" in lib.sgp_last_error()
    assert lib.sgp_characters_get_states(None, 0, 0, None) == abi.ERR_INVALID
    assert lib.sgp_characters_drain_contacts(None, None, 0, C.byref(n)) == abi.ERR_INVALID


def test_facade_header_compiles():
    """shim/CharacterBatch.h on its own, as a caller would include it."""
    shim = os.path.join(ROOT, "substrata_amd", "shim")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-fsyntax-only", "-I", shim, "-x", "c++", os.path.join(shim, "CharacterBatch.h")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_caller_program_compiles(tmp_path):
    from test_facade_gpu import build_facade_exe
    assert os.path.exists(build_facade_exe(tmp_path, "characters_batch.cpp"))
