"""CPU-side checks of the height-field ABI: the header declares sgp_heightfield_create and the library exports it, the ctypes mirror of
sgp_heightfield_desc has the library's size, and the test triangulation reproduces the facade's grid (PhysicsWorld.cpp
createJoltHeightFieldShape + meshInstance) in order and bit for bit."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from substrata_amd import abi, build
from heightfield_scenes import heightfield_triangulation, chunk_params

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    return C.CDLL(build.build())


def test_header_declares_and_library_exports(lib):
    src = open(os.path.join(ROOT, "include", "sgp.h")).read()
    assert re.search(r"int\s+sgp_heightfield_create\s*\(\s*sgp_world\s*\*\s*\w+\s*,\s*const\s+sgp_heightfield_desc\s*\*", src)
    assert "typedef struct sgp_heightfield_desc" in src
    assert hasattr(lib, "sgp_heightfield_create")
    assert "heightfield_create" in abi.PROTOTYPES


def test_desc_size_matches(lib):
    lib.sgp_abi_sizeof.restype = C.c_int
    assert abi.ABI_SIZEOF_ORDER[18] == "sgp_heightfield_desc"
    assert lib.sgp_abi_sizeof(18) == C.sizeof(abi.HeightfieldDesc) == C.sizeof(abi.STRUCTS["sgp_heightfield_desc"])
    assert lib.sgp_abi_version() == 1


def facade_triangulation(heights, quad_w, scale):
    """The facade's current chunk mesh, written out as its loops are (createJoltHeightFieldShape, then meshInstance's scale)."""
    w = heights.shape[0]
    f32 = np.float32
    z_offset = f32(-f32(quad_w) * f32(w - 1))
    V, T = [], []
    for z in range(w):
        for x in range(w):
            v = (f32(quad_w) * f32(x), heights[z, x], f32(quad_w) * f32(z) + z_offset)
            V.append([f32(v[0]) * f32(scale[0]), f32(v[1]) * f32(scale[1]), f32(v[2]) * f32(scale[2])])
    for z in range(w - 1):
        for x in range(w - 1):
            a = z * w + x; b = a + 1; c = a + w; d = c + 1
            T += [(a, c, d), (a, d, b)]
    return np.array(V, np.float32), np.array(T, np.uint32)


@pytest.mark.parametrize("w", [2, 3, 5, 8, 13, 64, 128])
@pytest.mark.parametrize("quad_w,scale", [(1.0, (1.0, 1.0, 1.0)), (0.5, (1.0, 1.0, 1.0)), (0.37, (1.3, 0.7, 2.1))])
def test_triangulation_is_the_facades(w, quad_w, scale):
    rng = np.random.default_rng(w)
    h = rng.uniform(-3, 3, size=(w, w)).astype(np.float32)
    h[0, 0] = 0.0                                                         # (not -0.0: the field's expression makes that +0.0)
    offset, spacing = chunk_params(w, quad_w)
    V, T, M = heightfield_triangulation(h, offset, spacing, scale)
    Vf, Tf = facade_triangulation(h, quad_w, scale)
    assert np.array_equal(T, Tf)
    assert np.array_equal(V.view(np.uint32), Vf.view(np.uint32))
    assert len(T) == 2 * (w - 1) ** 2 and len(V) == w * w and not M.any()
    # both triangles of a quad face +y
    n = np.cross(V[T[:, 1]] - V[T[:, 0]], V[T[:, 2]] - V[T[:, 0]])
    assert (n[:, 1] > 0).all()
    mats = np.arange((w - 1) ** 2, dtype=np.uint32) + 7
    assert np.array_equal(heightfield_triangulation(h, offset, spacing, scale, mats)[2], np.repeat(mats, 2))
