"""The rays' cell walks (CellWalk, sgp_dev_broadphase.h, and its written-out twin in raycast_world) and the world walks (raycast_world, sgp_dev_raycast.h; raycast_wave, sgp_k_queries.hip) on the
rays the seeded segments of the other ray tests never produce: axis-parallel directions, origins outside the grids, origins in the border cells, max_t ending
inside the first cell (tests/ray_walk_rays.py).  Closest hit against the oracle twin, any hit against closest hit, and each ray sent alone (n = 1, the
route that hands a lone ray to the resident server) against its batched answer, bit for bit.  Nothing a world reports says that the server answered rather than
the launch the host falls back to; tests/test_queries_gpu.py's server test stands on the same ground.

The terrain mesh, the height field, the portal and the sensor are meant to sit in the static large bodies' grid.  Nothing a world reports says whether they
do, so the test cannot observe it.  It follows from the host's rule (sgp_world.hip: at least 32 static large bodies; the cell edge is twice their median
extent; a body filling more than 256 cells stays on the list), whose arithmetic the first test repeats from the sizes the scene is built with: it checks the
premises, not the grid.  A post among the hits shows that the grid is walked."""
import numpy as np
import pytest

from substrata_amd import abi
from substrata_amd.lib import World
import ray_walk_rays as rw

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def worlds(oracle):
    g = World(max_bodies=256, large_body_radius=rw.LARGE_BODY_RADIUS)
    c = oracle.OracleWorld(max_bodies=256, large_body_radius=rw.LARGE_BODY_RADIUS)
    ids = rw.build(g)
    assert rw.build(c, field_as_mesh=True) == ids
    rays = rw.rays()
    yield g, ids, rays, c.raycast(rays)
    g.close()
    c.close()


def test_the_world_and_the_rays_are_what_the_test_needs(worlds):
    """Conditions of the test, from the oracle alone: at least a quarter of the rays hit and at least a quarter miss, bodies of all three stages are among
    the hits, and at least 32 static bodies are above the large-body radius."""
    g, ids, rays, want = worlds
    n = len(rays)
    hit = want["id"] != abi.INVALID_ID
    print("hits", int(hit.sum()), "misses", int((~hit).sum()))
    assert hit.sum() * 4 >= n and (~hit).sum() * 4 >= n
    kind_of = rw.scene.kind_of(ids)
    seen = {kind_of[int(i)] for i in want["id"][hit]}
    assert {"ground", "post", "field", "compound", "sphere", "box", "capsule"} <= seen, seen      # the list, the large bodies' grid, the cells
    assert np.linalg.norm(rw.POST_HALF) > rw.LARGE_BODY_RADIUS and len(ids["post"]) >= 32
    # the host's rule from the sizes: posts are the majority of the static large bodies, so the median extent is a post's and the cell edge twice that; the
    # terrain (8 m), the field (16 quads of 0.5 m), the portal and the sensor are at most 8.5 m wide with their bounds' slack: (floor(extent / cell) + 2)^3 cells at most
    n_other_static_large = 5                                                    # ground, terrain, field, portal, sensor
    assert len(ids["post"]) > n_other_static_large
    cell = 2.0 * 2.0 * max(rw.POST_HALF)
    assert (np.floor(8.5 / cell) + 2.0) ** 3 <= 256
    zero = (rays["dir"] == 0).sum(axis=1)
    assert (zero == 2).sum() >= 12 and (zero == 1).sum() >= 24
    for a in range(3):
        for s in (-1.0, 1.0):
            assert ((zero == 2) & (rays["dir"][:, a] == s)).any()
            assert ((zero == 1) & (np.sign(rays["dir"][:, a]) == s)).any()


@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_closest_hit_any_hit_and_the_resident_server_agree(worlds, n):
    g, ids, rays, want = worlds
    rays, want = rays[:n], want[:n]
    got = g.raycast(rays) if n > 1 else g.raycast(np.concatenate([rays, rays]))[:1]      # (a lone ray would go to the resident server: k_raycast gets it twice)
    assert np.array_equal(got["id"], want["id"]), np.flatnonzero(got["id"] != want["id"])
    print("max |dt|", float(np.max(np.abs(got["t"] - want["t"]))), "max |dn|", float(np.max(np.abs(got["normal"] - want["normal"]))))
    assert np.allclose(got["t"], want["t"], atol=1e-4) and np.allclose(got["normal"], want["normal"], atol=1e-4)
    anyh = g.raycast_any(rays)
    hit = got["id"] != abi.INVALID_ID
    assert np.array_equal(anyh, hit), np.flatnonzero(anyh != hit)
    single = np.concatenate([g.raycast(rays[k:k + 1]) for k in range(n)])
    assert single.tobytes() == got.tobytes(), [k for k in range(n) if single[k].tobytes() != got[k].tobytes()]
