"""CPU-side checks of the overlap-query entry point (include/sgp.h, "overlap queries with any convex shape"): declared, exported and prototyped, the
query struct has the library's size under a NEW index of sgp_abi_sizeof, and nothing that was there before moved.  No world exists here (no device)."""
import ctypes as C
import os
import re

import pytest

from substrata_amd import abi, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the indices of sgp_abi_sizeof as they stood before sgp_shape_query was appended
EARLIER = ["sgp_settings", "sgp_world_desc", "sgp_body_desc", "sgp_body_state", "sgp_body_event", "sgp_contact_event", "sgp_ray", "sgp_hit",
           "sgp_step_stats", "sgp_step_profile", "sgp_ghost_record", "sgp_vehicle_desc", "sgp_vehicle_input", "sgp_vehicle_state", "sgp_hull_info",
           "sgp_capsule_query", "sgp_query_contact", "sgp_mesh_info", "sgp_heightfield_desc", "sgp_checkpoint_info"]


@pytest.fixture(scope="module")
def lib():
    lib = C.CDLL(build.build())
    abi.bind(lib, "sgp_")
    return lib


def test_declared_exported_and_prototyped(lib):
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sgp.h")).read(), flags=re.S)
    assert re.search(r"int\s+sgp_collide_shapes\s*\(\s*sgp_world\s*\*\s*\w+\s*,\s*const\s+sgp_shape_query\s*\*", header)
    assert "typedef struct sgp_shape_query" in header and "SGP_QUERY_DEEPEST_ONLY" in header
    assert hasattr(lib, "sgp_collide_shapes")
    assert "collide_shapes" in abi.PROTOTYPES and lib.sgp_collide_shapes.argtypes is not None


def test_query_struct_has_the_library_size_under_a_new_index(lib):
    i = abi.ABI_SIZEOF_ALL.index("sgp_shape_query")
    assert i == len(EARLIER) == 20
    assert lib.sgp_abi_sizeof(i) == C.sizeof(abi.ShapeQuery) == C.sizeof(abi.STRUCTS["sgp_shape_query"]) == abi.shape_query_dtype.itemsize == 80
    assert lib.sgp_abi_sizeof(i + 1) == -1
    # the fields of the header, in its order
    assert [n for n, _ in abi.ShapeQuery._fields_] == ["pos", "rot", "shape_type", "shape", "max_separation", "ignore_id", "layer_mask", "flags", "movement", "active_edges"]
    assert abi.ShapeQuery.shape_type.offset == 28 and abi.ShapeQuery.max_separation.offset == 48 and abi.ShapeQuery.movement.offset == 64
    assert abi.QUERY_DEEPEST_ONLY == 1


def test_version_and_earlier_indices_are_unchanged(lib):
    assert lib.sgp_abi_version() == 1 == abi.ABI_VERSION
    assert abi.ABI_SIZEOF_ALL[:len(EARLIER)] == EARLIER == abi.ABI_SIZEOF_ORDER
    for i, name in enumerate(EARLIER):
        assert lib.sgp_abi_sizeof(i) == C.sizeof(abi.STRUCTS[name]), name
    # the capsule query and the record both queries share keep their layouts
    assert C.sizeof(abi.CapsuleQuery) == 64 and C.sizeof(abi.QueryContact) == 72


def test_null_arguments_are_invalid_without_a_device(lib):
    n = C.c_uint32(7)
    assert lib.sgp_collide_shapes(None, None, 0, None, 0, C.byref(n)) == abi.ERR_INVALID
    assert b"sgp_collide_shapes" in lib.sgp_last_error()
