"""CPU-side checks of the driven characters' entry points (include/sgp.h, "driven characters"): declared, exported and prototyped, the two structs have the
library's sizes under NEW indices of sgp_abi_sizeof and their fields sit where the header puts them, the defaults are PlayerPhysics' constants, NULL handles and
bad values are refused, and the facade header and the caller programs compile.  No device."""
import ctypes as C
import math
import os
import re
import subprocess

import pytest

from substrata_amd import abi, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STRUCTS = [("sgp_character_drive", abi.CharacterDrive, 32), ("sgp_character_drive_state", abi.CharacterDriveState, 48)]
FUNCTIONS = ["default_character_drive", "characters_set_drive", "characters_jump", "characters_update_at", "characters_get_drive_states"]
SIZES = {"float": 4, "int32_t": 4, "uint32_t": 4, "uint64_t": 8, "double": 8}
# sgp_abi_sizeof as it stood before the two structs were appended (index: struct name, None where the index answers -1 for good)
BEFORE = ["sgp_settings", "sgp_world_desc", "sgp_body_desc", "sgp_body_state", "sgp_body_event", "sgp_contact_event", "sgp_ray", "sgp_hit", "sgp_step_stats",
          "sgp_step_profile", "sgp_ghost_record", "sgp_vehicle_desc", "sgp_vehicle_input", "sgp_vehicle_state", "sgp_hull_info", "sgp_capsule_query",
          "sgp_query_contact", "sgp_mesh_info", "sgp_heightfield_desc", "sgp_checkpoint_info", "sgp_shape_query", None, "sgp_shape_cast", "sgp_cast_hit",
          None, "sgp_character_desc", "sgp_character_input", "sgp_character_state", "sgp_character_contact", None, "sgp_particle", "sgp_particle_state",
          "sgp_particle_event", None, "sgp_craft_desc", "sgp_craft_input", "sgp_craft_state", None, "sgp_path_waypoint", "sgp_path_segment",
          "sgp_path_progress", "sgp_mover_desc", "sgp_mover_state", None, "sgp_batch_checkpoint_info", None, "sgp_proximity_object", "sgp_proximity_observer",
          "sgp_proximity_event", "sgp_proximity_state", "sgp_proximity_observer_state", None, "sgp_audibility_source", "sgp_audibility_listener",
          "sgp_audibility_event", "sgp_audibility_state", "sgp_audibility_pair_state", "sgp_audibility_listener_state", "sgp_audibility_ramp"]
BEFORE_SIZES = {"sgp_character_desc": 136, "sgp_character_input": 20, "sgp_character_state": 88, "sgp_character_contact": 48, "sgp_batch_checkpoint_info": 40,
                "sgp_audibility_source": 40, "sgp_audibility_ramp": 32, "sgp_shape_query": 80, "sgp_checkpoint_info": 72}


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
    for macro, value in (("SGP_DRIVE_ON", abi.DRIVE_ON), ("SGP_DRIVE_FLY", abi.DRIVE_FLY), ("SGP_DRIVE_GRAVITY", abi.DRIVE_GRAVITY),
                         ("SGP_DRIVE_FREE_CAMERA", abi.DRIVE_FREE_CAMERA), ("SGP_DRIVE_SMOOTH_STAIRS", abi.DRIVE_SMOOTH_STAIRS)):
        assert re.search(r"#define %s\s+%du" % (macro, value), h), macro
    assert (abi.DRIVE_ON, abi.DRIVE_FLY, abi.DRIVE_GRAVITY, abi.DRIVE_FREE_CAMERA, abi.DRIVE_SMOOTH_STAIRS) == (1, 2, 4, 8, 16)
    # sgp_characters_update keeps its signature; the header says what it means for a driven character
    assert re.search(r"int\s+sgp_characters_update\(sgp_characters\* cs, float dt\);", h)
    assert "no jump window is open" in open(os.path.join(ROOT, "include", "sgp.h")).read()


def test_structs_have_the_library_sizes_under_new_indices(lib):
    idx = [abi.ABI_SIZEOF_ALL.index(s) for s, _, _ in STRUCTS]
    assert idx == [60, 61]                     # (59 answers -1 for good, as 21, 24, 29, 33, 37, 43, 45 and 51 do)
    assert lib.sgp_abi_sizeof(59) == -1 and abi.ABI_SIZEOF_ALL[59] is None and lib.sgp_abi_sizeof(62) == -1 and len(abi.ABI_SIZEOF_ALL) == 62
    for (struct, mirror, size), i in zip(STRUCTS, idx):
        assert lib.sgp_abi_sizeof(i) == C.sizeof(mirror) == C.sizeof(abi.STRUCTS[struct]) == size, struct
    assert abi.ABI_SIZEOF_ALL[:59] == BEFORE                      # every earlier index is unchanged ...
    for k, name in enumerate(BEFORE):
        assert lib.sgp_abi_sizeof(k) == (C.sizeof(abi.STRUCTS[name]) if name is not None else -1), (k, name)
    for name, size in BEFORE_SIZES.items():                       # ... and so are the sizes behind them
        assert lib.sgp_abi_sizeof(BEFORE.index(name)) == size, name
    assert lib.sgp_abi_version() == 1 == abi.ABI_VERSION
    assert abi.character_drive_dtype.itemsize == 32 and abi.character_drive_state_dtype.itemsize == 48


def test_defaults_are_player_physics_constants(lib):
    f32 = lambda x: C.c_float(x).value
    d = abi.CharacterDrive()
    d.move_up = 5.0; d.move_desired_vel[0] = 1.0
    lib.sgp_default_character_drive(C.byref(d))
    lib.sgp_default_character_drive(None)      # (returns)
    assert tuple(d.move_desired_vel) == (0.0, 0.0, 0.0) and d.move_up == 0.0 and d.flags == abi.DRIVE_GRAVITY
    assert (d.jump_speed, d.max_air_speed, d.eye_height) == (4.5, 8.0, f32(1.67))
    # the literals of the rule are the reference's
    src = open(os.path.join(ROOT, "substrata_amd", "csrc", "sgp_player_rule.h")).read()
    for lit in ("9.81f", "1.1f", "0.2f", "2.0f", "0.3f", "0.1f", "3.f", "2.f", "1.e-4f", "-100", "20.f", "1.0e-5f", "-0.3f, 0.3f"):
        assert lit in src, lit
    assert "__global__" not in src and "hip_runtime" not in src and "threadIdx" not in src      # plain inline functions, no HIP


def test_null_handles_and_bad_values_are_refused(lib):
    d = abi.CharacterDrive()
    lib.sgp_default_character_drive(C.byref(d))
    st = abi.CharacterDriveState()
    i = C.c_uint32(0)
    assert lib.sgp_characters_set_drive(None, 0, 1, C.addressof(d)) == abi.ERR_INVALID
    assert b"sgp_characters_set_drive" in lib.sgp_last_error()
    assert lib.sgp_characters_set_drive(None, 0, 0, None) == abi.ERR_INVALID
    assert lib.sgp_characters_jump(None, C.addressof(i), 1, 0.0) == abi.ERR_INVALID
    assert b"sgp_characters_jump" in lib.sgp_last_error()
    assert lib.sgp_characters_update_at(None, 1.0 / 60.0, 0.0) == abi.ERR_INVALID
    assert b"sgp_characters_update_at" in lib.sgp_last_error()
    assert lib.sgp_characters_update_at(None, 1.0 / 60.0, math.nan) == abi.ERR_INVALID and b"non-finite time" in lib.sgp_last_error()
    assert lib.sgp_characters_update_at(None, 1.0 / 60.0, math.inf) == abi.ERR_INVALID
    assert lib.sgp_characters_get_drive_states(None, 0, 1, C.addressof(st)) == abi.ERR_INVALID
    assert b"sgp_characters_get_drive_states" in lib.sgp_last_error()
    # the value checks of sgp_characters_set_drive and sgp_characters_jump sit behind the handle check: what they refuse is read from the source (the GPU suite
    # exercises them on a live batch, tests/test_players_gpu.py::test_bad_drives_are_refused_all_or_nothing)
    src = open(os.path.join(ROOT, "substrata_amd", "csrc", "sgp_world_characters.hip")).read()
    for text in ("sgp_characters_set_drive: a non-finite value", "sgp_characters_set_drive: unknown flag", "d.jump_speed < 0.0f || d.max_air_speed < 0.0f || !(d.eye_height > 0.0f)",
                 "sgp_characters_set_drive: range beyond the last character", "sgp_characters_jump: non-finite time", "sgp_characters_jump: no such character"):
        assert text in src, text


def test_facade_header_compiles():
    """shim/PlayerBatch.h on its own, as a caller would include it."""
    shim = os.path.join(ROOT, "substrata_amd", "shim")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-fsyntax-only", "-I", shim, "-x", "c++", os.path.join(shim, "PlayerBatch.h")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_caller_programs_compile(tmp_path):
    from test_facade_gpu import build_facade_exe
    assert os.path.exists(build_facade_exe(tmp_path, "players_batch.cpp"))
    assert os.path.exists(build_facade_exe(tmp_path, "players_facade.cpp"))
