"""Any-hit rays (sgp_raycast_any, what PhysicsWorld::doesRayHitAnything keeps of a ray) against the closest-hit search: for every ray
hit_out[i] == (sgp_raycast's hit.id != SGP_INVALID_ID) -- with every layer and with collidable_only, with ignore_id set to the body the closest-hit search
reported, and at the boundary (max_t equal to the closest hit's t, and one float below it), where only the equality of the two answers is asserted."""
import numpy as np
import pytest

from substrata_amd import abi
from substrata_amd.lib import World
import raycast_any_scene as scene

pytestmark = pytest.mark.gpu

N_RAYS = 257
RAY_SEED = 11


@pytest.fixture(scope="module")
def world():
    w = World(max_bodies=256)
    ids = scene.build(w)
    yield w, ids
    w.close()


def both(w, rays):
    hits = w.raycast(rays)
    anyh = w.raycast_any(rays)
    assert anyh.dtype == bool and anyh.shape == (len(rays),)
    return hits, anyh


def test_the_scene_is_what_the_test_needs(world):
    """Conditions of the test, not measurements: about 60 bodies over several broad-phase cells, at least a quarter of the seeded rays hit and at least a
    quarter miss, and every shape kind is some ray's closest hit."""
    w, ids = world
    n_bodies = sum(len(v) for v in ids.values())
    assert 55 <= n_bodies <= 65
    rays = scene.segments(N_RAYS, RAY_SEED)
    hits = w.raycast(rays)
    hit = hits["id"] != abi.INVALID_ID
    assert hit.sum() * 4 >= N_RAYS and (~hit).sum() * 4 >= N_RAYS, (hit.sum(), N_RAYS)
    kind_of = scene.kind_of(ids)
    seen = {kind_of[int(i)] for i in hits["id"][hit]}
    assert seen == set(scene.KINDS), set(scene.KINDS) - seen
    assert set(np.unique(hits["sub_shape"][hits["id"] == ids["compound"][0]])) == {0, 1}      # the compound's mesh and its box


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_any_hit_equals_closest_hit_found_something(world, n):
    w, ids = world
    for collidable_only in (0, 1):
        rays = scene.segments(N_RAYS, RAY_SEED, collidable_only)[:n]
        hits, anyh = both(w, rays)
        hit = hits["id"] != abi.INVALID_ID
        assert np.array_equal(anyh, hit), np.flatnonzero(anyh != hit)
        if collidable_only:
            assert not np.isin(hits["id"], ids["non_collidable"]).any()
        # the same rays ignoring the body the closest-hit search reported
        rays2 = rays.copy()
        rays2["ignore_id"] = hits["id"]
        hits2, any2 = both(w, rays2)
        hit2 = hits2["id"] != abi.INVALID_ID
        assert np.array_equal(any2, hit2), np.flatnonzero(any2 != hit2)
        assert not (hit2 & ~hit).any()
        if n >= 63:
            assert (hit & ~hit2).any() and (hit & hit2).any()                   # ignoring it flips some answers and leaves others


def test_collidable_only_changes_some_answers(world):
    w, ids = world
    r0, r1 = scene.segments(N_RAYS, RAY_SEED, 0), scene.segments(N_RAYS, RAY_SEED, 1)
    a0, a1 = w.raycast_any(r0), w.raycast_any(r1)
    assert not (a1 & ~a0).any() and (a0 & ~a1).any()


def test_boundary_rays_get_one_answer_from_both(world):
    """max_t = the closest hit's t, and max_t one float below it: whichever way each test rounds, both entry points give the same answer."""
    w, ids = world
    rays = scene.segments(N_RAYS, RAY_SEED)
    hits = w.raycast(rays)
    sel = (hits["id"] != abi.INVALID_ID) & (hits["t"] > 0)
    assert sel.sum() >= 40
    kinds = {scene.kind_of(ids)[int(i)] for i in hits["id"][sel]}
    assert {"sphere", "box", "capsule", "hull", "mesh", "field", "compound", "ground"} <= kinds
    at = rays[sel].copy(); at["max_t"] = hits["t"][sel]
    below = rays[sel].copy(); below["max_t"] = np.nextafter(hits["t"][sel], np.float32(0.0))
    for name, r in (("max_t = t", at), ("max_t just below t", below)):
        h, a = both(w, r)
        hit = h["id"] != abi.INVALID_ID
        assert np.array_equal(a, hit), (name, np.flatnonzero(a != hit))
        print(name, "hits:", int(hit.sum()), "of", len(r))


def test_no_rays_and_null_arguments(world):
    w, ids = world
    assert len(w.raycast_any(np.zeros(0, dtype=abi.ray_dtype))) == 0
    assert w._fn("raycast_any")(w._h, None, 3, None) == abi.ERR_INVALID
    assert w._fn("raycast_any")(None, None, 0, None) == abi.ERR_INVALID
