"""The scene of tests/test_raycast_any_gpu.py: about 60 bodies holding every kind ray_body knows (sgp_dev_raycast.h) -- spheres, boxes, capsules and hulls
spread over the broad-phase cells, a terrain mesh whose tree is several levels deep, a height field, a portal compound (mesh + box), the ground quad (a large
body), a sensor and a non-collidable body.  Never stepped: the bodies hang where they are put.  `build(w)` works on the product's world and on the oracle's
(field_as_mesh: the oracle keeps a field as its triangulation), so the shares of hits and misses can be looked at without a device."""
import numpy as np

from substrata_amd import abi, scenes
from compound_scene import add_portal
from heightfield_scenes import bumpy_heights, chunk_params, heightfield_triangulation, mesh_body

LO, HI = np.float32([-12.0, -12.0, -0.8]), np.float32([12.0, 12.0, 5.0])      # the scene's box: rays are segments between points of it
KINDS = ("ground", "sphere", "box", "capsule", "hull", "mesh", "field", "compound", "sensor", "non_collidable")
SEED = 5


def terrain_mesh(n=17, size=4.0):
    xs = np.linspace(-size, size, n)
    V = np.array([(x, y, 1.0 + 0.6 * np.sin(0.9 * x) * np.cos(0.7 * y)) for y in xs for x in xs], np.float32)
    T = []
    for j in range(n - 1):
        for i in range(n - 1):
            a = j * n + i; b = a + 1; c = a + n; d = c + 1
            T += [(a, b, d), (a, d, c)]
    return V, np.array(T, np.uint32)


def build(w, field_as_mesh=False):
    """Adds the scene to the empty world `w`.  Returns {kind: ids}."""
    rng = np.random.default_rng(SEED)
    ids = {}
    ids["ground"] = [int(w.add_batch(scenes.ground())[0])]
    V, T = terrain_mesh()
    assert len(T) == 512                                                        # (a leaf holds a handful of triangles: several levels)
    ids["mesh"] = [int(w.add_batch(mesh_body(w.mesh_create(V, T).mesh_id, pos=(-7.5, -7.5, 0.0), rot=(0, 0, 0, 1)))[0])]
    h = bumpy_heights(16)
    offset, spacing = chunk_params(16, 0.5)
    if field_as_mesh:
        fV, fT, fM = heightfield_triangulation(h, offset, spacing)
        fi = w.mesh_create(fV, fT, materials=fM)
    else:
        fi = w.heightfield_create(h, offset, spacing)
    ids["field"] = [int(w.add_batch(mesh_body(fi.mesh_id, pos=(4.0, -11.5, 1.2)))[0])]
    ids["compound"] = [int(add_portal(w, (0.0, 7.0, 0.0))[0])]
    hull = w.hull_create(rng.normal(size=(14, 3)) * 0.7)
    n = 52
    d = scenes.dynamic_bodies(n)
    d["pos"] = rng.uniform([-11, -11, 0.8], [11, 11, 4.5], size=(n, 3))
    d["rot"] = scenes._random_unit_quats(rng, n)
    kind = np.arange(n) % 4
    s = rng.uniform(0.5, 1.3, size=n).astype(np.float32)
    d["shape"][:] = 0
    d["shape_type"][kind == 0] = abi.SHAPE_SPHERE; d["shape"][kind == 0, 0] = 0.8 * s[kind == 0]
    d["shape_type"][kind == 1] = abi.SHAPE_BOX; d["shape"][kind == 1, :3] = rng.uniform(0.3, 1.0, size=((kind == 1).sum(), 3))
    d["shape_type"][kind == 2] = abi.SHAPE_CAPSULE; d["shape"][kind == 2, 0] = 0.4 * s[kind == 2]; d["shape"][kind == 2, 1] = 0.9 * s[kind == 2]
    d["shape_type"][kind == 3] = abi.SHAPE_HULL; d["shape"][kind == 3, 0] = float(hull.hull_id)
    small = w.add_batch(d)
    for k, name in enumerate(("sphere", "box", "capsule", "hull")):
        ids[name] = [int(i) for i in small[kind == k]]
    sens = scenes._blank(1); sens["is_sensor"] = 1; sens["pos"][0] = (6.0, 6.0, 2.0); sens["shape"][0, :3] = (1.5, 1.5, 1.5)
    ids["sensor"] = [int(w.add_batch(sens)[0])]
    ghost = scenes.dynamic_bodies(1); ghost["layer"] = abi.LAYER_MOVING_NON_COLLIDABLE; ghost["pos"][0] = (-6.0, 6.0, 2.0); ghost["shape"][0, :3] = (1.5, 1.5, 1.5)
    ids["non_collidable"] = [int(w.add_batch(ghost)[0])]
    assert set(ids) == set(KINDS)
    return ids


def segments(n, seed, collidable_only=0):
    """n rays of abi.ray_dtype: seeded segments between two points of the scene's box (unit direction, max_t = the segment's length)."""
    rng = np.random.default_rng(seed)
    a = rng.uniform(LO, HI, size=(n, 3)).astype(np.float32)
    b = rng.uniform(LO, HI, size=(n, 3)).astype(np.float32)
    rays = np.zeros(n, dtype=abi.ray_dtype)
    length = np.linalg.norm((b - a).astype(np.float64), axis=1)
    rays["origin"] = a
    rays["dir"] = ((b - a) / length[:, None]).astype(np.float32)
    rays["max_t"] = length.astype(np.float32)
    rays["ignore_id"] = abi.INVALID_ID
    rays["collidable_only"] = collidable_only
    return rays


def kind_of(ids):
    """{body id: kind}"""
    return {i: k for k, v in ids.items() for i in v}
