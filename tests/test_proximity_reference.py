"""The two host exports of the proximity watchers (sgp_proximity_test_point, sgp_proximity_pick_zone: sgp_proximity_math.h compiled for the host, the code the
device runs) against the numpy float32 restatement of docs/CONTRACT.md 4l (tests/proximity_reference.py): 10 000 seeded cases each, equal to the bit, and the
exact boundary cases.  No device."""
import ctypes as C

import numpy as np
import pytest

from substrata_amd import abi, build
import proximity_reference as pr

F32 = np.float32


@pytest.fixture(scope="module")
def lib():
    lib = C.CDLL(build.build())
    abi.bind(lib, "sgp_")
    return lib


def f3(v):
    return (C.c_float * 3)(*[float(x) for x in v])


def host_point(lib, mn, mx, p, radius):
    near, d2 = C.c_uint32(7), C.c_float(-1.0)
    assert lib.sgp_proximity_test_point(f3(mn), f3(mx), f3(p), float(radius), C.byref(near), C.byref(d2)) == abi.OK
    return bool(near.value), F32(d2.value)


def pick(lib, mins, maxs, keys, live, current, p):
    mins, maxs = np.ascontiguousarray(mins, F32).reshape(-1, 3), np.ascontiguousarray(maxs, F32).reshape(-1, 3)
    keys, live = np.ascontiguousarray(keys, np.uint32), np.ascontiguousarray(live, np.uint32)
    z = C.c_uint32(12345)
    assert lib.sgp_proximity_pick_zone(mins.ctypes.data, maxs.ctypes.data, keys.ctypes.data, live.ctypes.data, len(keys), int(current), f3(p), C.byref(z)) == abi.OK
    return int(z.value)


def test_near_test_equals_the_restatement_on_seeded_cases(lib):
    rng = np.random.default_rng(20)
    n = 10000
    c = rng.uniform(-200, 200, (n, 3)).astype(F32)
    h = rng.uniform(0.0, 30, (n, 3)).astype(F32)
    mn, mx = c - h, c + h
    p = (c + rng.normal(0, 40, (n, 3))).astype(F32)
    radius = rng.uniform(0.1, 60, n).astype(F32)
    # a third of the cases sit on the boundary as closely as float32 lets them: the radius is the distance itself, or its neighbours
    d = np.sqrt(np.array([pr.dist2(mn[i], mx[i], p[i]) for i in range(n)], dtype=F32))
    edge = np.arange(n) % 3 == 0
    radius[edge] = np.where(np.arange(n)[edge] % 2 == 0, d[edge], np.nextafter(d[edge], F32(np.inf)))
    radius = np.maximum(radius, F32(1e-3))
    nears = 0
    for i in range(n):
        got_near, got_d2 = host_point(lib, mn[i], mx[i], p[i], radius[i])
        want_d2 = pr.dist2(mn[i], mx[i], p[i])
        assert got_d2.tobytes() == F32(want_d2).tobytes(), (i, got_d2, want_d2)
        assert got_near == bool(pr.near(mn[i], mx[i], p[i], radius[i])), i
        nears += got_near
    assert n // 10 < nears < 9 * n // 10      # both answers are well represented


def test_zone_choice_equals_the_restatement_on_seeded_cases(lib):
    rng = np.random.default_rng(21)
    outcomes = {"stays": 0, "moves": 0, "none": 0}
    for case in range(10000):
        nz = int(rng.integers(1, 9))
        c = rng.integers(-4, 5, (nz, 3)).astype(F32)
        h = rng.integers(2, 8, (nz, 3)).astype(F32)      # zones a few units wide around a few centres: they overlap, and most points are in one
        mins, maxs = c - h, c + h
        keys = rng.permutation(100)[:nz].astype(np.uint32)
        live = (rng.random(nz) < 0.8).astype(np.uint32)
        p = rng.integers(-8, 9, 3).astype(F32) if case % 2 else rng.uniform(-8, 8, 3).astype(F32)      # integer points land on faces
        current = int(rng.integers(0, nz)) if case % 3 else abi.INVALID_ID
        got = pick(lib, mins, maxs, keys, live, current, p)
        want = pr.pick_zone(mins, maxs, keys, live, current, p)
        assert got == want, (case, got, want)
        outcomes["none" if got == abi.INVALID_ID else "stays" if got == current else "moves"] += 1
    assert min(outcomes.values()) > 500, outcomes


def test_exact_boundary_cases(lib):
    o = (0.0, 0.0, 0.0)
    # a box face at x = 20, the observer at the origin, radius 20: dist2 = 400, NOT near (the comparison is strict)
    near, d2 = host_point(lib, (20.0, -1.0, -1.0), (22.0, 1.0, 1.0), o, 20.0)
    assert d2 == F32(400.0) and not near and not pr.near((20.0, -1.0, -1.0), (22.0, 1.0, 1.0), o, 20.0)
    # the face one float32 nearer: 399.99994, near
    x = np.nextafter(F32(20.0), F32(0.0))
    near, d2 = host_point(lib, (x, -1.0, -1.0), (22.0, 1.0, 1.0), o, 20.0)
    assert d2 == F32(399.99994) and d2 == x * x and near and pr.near((x, -1.0, -1.0), (22.0, 1.0, 1.0), o, 20.0)
    # the closest point (12, 16, 0): 144 + 256 = 400, not near
    near, d2 = host_point(lib, (12.0, 16.0, -1.0), (14.0, 18.0, 1.0), o, 20.0)
    assert d2 == F32(400.0) and not near
    # inside the box: distance 0, near for any radius > 0
    near, d2 = host_point(lib, (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0), o, 1e-3)
    assert d2 == F32(0.0) and near
    # an observer exactly on a zone's max face is inside; so is a centroid (3 + 5) * 0.5 = 4 on a min face at 4
    mins, maxs = [(0.0, 0.0, 0.0)], [(10.0, 10.0, 10.0)]
    assert pick(lib, mins, maxs, [5], [1], abi.INVALID_ID, (10.0, 5.0, 5.0)) == 0 == pr.pick_zone(np.array(mins, F32), np.array(maxs, F32), [5], [1], abi.INVALID_ID, (10.0, 5.0, 5.0))
    assert pick(lib, mins, maxs, [5], [1], abi.INVALID_ID, (np.nextafter(F32(10.0), F32(11.0)), 5.0, 5.0)) == abi.INVALID_ID
    q = pr.centroid((3.0, 3.0, 3.0), (5.0, 5.0, 5.0))
    assert tuple(q) == (4.0, 4.0, 4.0) and pr.contains((4.0, 4.0, 4.0), (9.0, 9.0, 9.0), q)
    assert pick(lib, [(4.0, 4.0, 4.0)], [(9.0, 9.0, 9.0)], [1], [1], abi.INVALID_ID, q) == 0
    # overlapping zones: an observer already in the higher key stays in it, a fresh one at the same point gets the lower key
    mins, maxs, keys = [(0.0, 0.0, 0.0), (5.0, 0.0, 0.0)], [(10.0, 10.0, 10.0), (15.0, 10.0, 10.0)], [9, 3]
    p = (7.0, 5.0, 5.0)
    assert pick(lib, mins, maxs, keys, [1, 1], 0, p) == 0
    assert pick(lib, mins, maxs, keys, [1, 1], abi.INVALID_ID, p) == 1
    assert pick(lib, mins, maxs, keys, [0, 1], 0, p) == 1      # the zone it was in is no longer live
    assert pick(lib, mins, maxs, keys, [1, 1], 0, (12.0, 5.0, 5.0)) == 1      # it left the zone it was in
