"""sgp_collide_shapes (NarrowPhaseQuery::CollideShape with a sphere, box, capsule or convex hull, batched): capsule-typed queries against the existing
capsule query bit for bit, the other shapes against the oracle's narrow phase by brute force, both kernel organisations against each other, known
answers, rejections and the absence of side effects.  The scene is the settled pile of tests/test_queries_gpu.py plus a layer-2 box inside it, and --
far from it -- a one-quad mesh floor and a static compound."""
import os

import numpy as np
import pytest

from substrata_amd import abi, scenes
from substrata_amd.world import SgpError
from helpers import DT

pytestmark = pytest.mark.gpu

FLOOR_X, COMPOUND_X = 40.0, -40.0      # where the mesh floor and the compound stand: nowhere near the pile (ground box aside, which spans everything)


def make_world(path=None, **kw):
    """A world whose sgp_collide_shapes takes the given organisation (SGP_QUERY_PATH is read at world creation)."""
    from substrata_amd.lib import World
    old = os.environ.pop("SGP_QUERY_PATH", None)
    if path:
        os.environ["SGP_QUERY_PATH"] = path
    try:
        return World(**kw)
    finally:
        os.environ.pop("SGP_QUERY_PATH", None)
        if old is not None:
            os.environ["SGP_QUERY_PATH"] = old


HULL_RNG_SEED = 8


def hull_points():
    rng = np.random.default_rng(HULL_RNG_SEED)
    return rng.normal(size=(14, 3)) * 0.6, rng.normal(size=(10, 3)) * 0.45      # the pile's hull, and one only queries use (a placement test)


class Pile:
    """The settled pile in a world of the given organisation, with what the tests need to know about its bodies."""

    def __init__(self, path):
        rng = np.random.default_rng(8)
        self.w = w = make_world(path, max_bodies=1024)
        pts_pile, pts_query = hull_points()
        self.hull_pile = w.hull_create(pts_pile).hull_id
        self.hull_query = w.hull_create(pts_query).hull_id
        descs = scenes.small_mixed(8, 3, seed=12)
        hd = scenes.dynamic_bodies(20)
        hd["shape_type"] = abi.SHAPE_HULL; hd["shape"][:, 0] = float(self.hull_pile); hd["shape"][:, 1:] = 0
        hd["pos"] = rng.uniform([-4, -4, 1], [4, 4, 5], size=(20, 3))
        sens = scenes.dynamic_bodies(1); sens["is_sensor"] = 1; sens["motion_type"] = abi.MOTION_STATIC; sens["pos"][0] = (0, 0, 1.0); sens["shape"][0, :3] = 1.0
        ghost = scenes._blank(1); ghost["layer"] = abi.LAYER_NON_MOVING_NON_COLLIDABLE; ghost["pos"][0] = (1.0, 1.0, 1.0); ghost["shape"][0, :3] = 1.5      # collides with nothing
        allb = np.concatenate([descs, hd, sens, ghost])
        ids = w.add_batch(allb)
        assert np.array_equal(ids, np.arange(len(allb)))
        self.descs = allb
        self.ghost_id = int(ids[-1])
        # the one-quad mesh floor
        V = np.array([(-2, -2, 0), (2, -2, 0), (2, 2, 0), (-2, 2, 0)], np.float32)
        mi = w.mesh_create(V, np.array([(0, 1, 2), (0, 2, 3)], np.uint32))
        md = scenes._blank(1); md["shape_type"] = abi.SHAPE_MESH; md["shape"][0] = (float(mi.mesh_id), 0, 0, 0); md["pos"][0] = (FLOOR_X, 0, 0)
        self.floor_id = int(w.add_batch(md)[0])
        # the compound: two boxes side by side with a gap of 0.2 m between them
        ch = np.zeros(2, dtype=abi.compound_child_dtype)
        ch["shape_type"] = abi.SHAPE_BOX; ch["shape"][:, :3] = 0.5; ch["rot"][:, 3] = 1.0
        ch["pos"][0] = (-0.6, 0, 0); ch["pos"][1] = (0.6, 0, 0)
        base = scenes._blank(1); base["pos"][0] = (COMPOUND_X, 0, 0.5)
        self.compound_id = w.add_compound(base, ch)
        for _ in range(200):
            w.step(DT)
        self.n_bodies = len(allb)
        self.states = w.read_states(0, self.n_bodies)

    def close(self):
        self.w.close()


@pytest.fixture(scope="module")
def piles():
    made = {}

    def get(path):
        if path not in made:
            made[path] = Pile(path)
        return made[path]
    yield get
    for p in made.values():
        p.close()


def rand_quats(rng, n):
    q = rng.normal(size=(n, 4)); q /= np.linalg.norm(q, axis=1, keepdims=True)
    return q.astype(np.float32)


def shape_queries(rng, n, kind, pile, max_sep=0.12):
    q = np.zeros(n, dtype=abi.shape_query_dtype)
    q["pos"] = rng.uniform([-5, -5, 0.2], [5, 5, 3.0], size=(n, 3))
    q["rot"] = rand_quats(rng, n)
    q["shape_type"] = kind
    if kind == abi.SHAPE_SPHERE:
        q["shape"][:, 0] = rng.uniform(0.3, 0.8, n)
    elif kind == abi.SHAPE_BOX:
        q["shape"][:, :3] = rng.uniform(0.25, 0.8, size=(n, 3))
    elif kind == abi.SHAPE_CAPSULE:
        q["shape"][:, 0] = 0.3; q["shape"][:, 1] = 0.65
    else:
        q["shape"][:, 0] = np.where(np.arange(n) % 2 == 0, pile.hull_pile, pile.hull_query)
    q["max_separation"] = max_sep
    q["ignore_id"] = abi.INVALID_ID
    return q


def mixed_queries(rng, pile, n=257):
    parts = [shape_queries(rng, n - 3 * (n // 4), abi.SHAPE_BOX, pile)] + [shape_queries(rng, n // 4, k, pile) for k in (abi.SHAPE_SPHERE, abi.SHAPE_CAPSULE, abi.SHAPE_HULL)]
    q = np.concatenate(parts)
    q = q[rng.permutation(len(q))]
    q["max_separation"][::2] = 0.0
    q["ignore_id"][::7] = 5
    q["layer_mask"][::5] = 0x3
    q["flags"][::11] = abi.QUERY_DEEPEST_ONLY
    return q


def capsule_as_shape(q):
    s = np.zeros(len(q), dtype=abi.shape_query_dtype)
    for f in ("pos", "rot", "max_separation", "ignore_id", "movement", "active_edges"):
        s[f] = q[f]
    s["shape_type"] = abi.SHAPE_CAPSULE
    s["shape"][:, 0] = q["radius"]; s["shape"][:, 1] = q["half_height"]
    s["layer_mask"] = np.where(q["collidable_only"] != 0, 0x3, 0)
    return s


def assert_records_equal_bitwise(a, b):
    assert len(a) == len(b)
    for f in abi.query_contact_dtype.names:
        assert a[f].tobytes() == b[f].tobytes(), f


# 1 ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("path", [None, "wave", "pairs"])
def test_capsule_typed_queries_equal_the_capsule_query(piles, path):
    p = piles(path)
    rng = np.random.default_rng(8)
    n = 257
    q = np.zeros(n, dtype=abi.capsule_query_dtype)
    q["pos"] = rng.uniform([-5, -5, 0.2], [5, 5, 3.0], size=(n, 3))
    q["rot"] = rand_quats(rng, n); q["rot"][: n // 2] = (0, 0, 0, 1)
    q["radius"] = 0.3; q["half_height"] = 0.65; q["max_separation"] = 0.12
    q["ignore_id"] = abi.INVALID_ID; q["ignore_id"][::7] = 5
    q["collidable_only"] = 1
    ref = p.w.collide_capsules(q, cap=16384)
    got, total = p.w.collide_shapes(capsule_as_shape(q), cap=16384)
    assert 100 < len(ref) < 16384 and total == len(ref)
    assert not (ref["body"] == p.ghost_id).any()          # (collidable_only means something here: the layer-2 box stands in the pile)
    assert_records_equal_bitwise(got, ref)


@pytest.mark.parametrize("path", ["wave", "pairs"])
def test_capsule_typed_queries_on_a_mesh_equal_the_capsule_query(path):
    from test_mesh_parity_gpu import grid_mesh, mesh_body
    rng = np.random.default_rng(4)
    w = make_world(path, max_bodies=64)
    height = lambda x, y: 0.0 if abs(x) < 4 and abs(y) < 4 else 0.35 * np.sin(0.9 * x) * np.cos(0.8 * y)
    V, T = grid_mesh(25, 12.0, height)
    w.add_batch(mesh_body(w.mesh_create(V, T)))
    n = 257
    q = np.zeros(n, dtype=abi.capsule_query_dtype)
    xy = rng.uniform(-10, 10, size=(n, 2))
    h = np.where((np.abs(xy[:, 0]) < 4) & (np.abs(xy[:, 1]) < 4), 0.0, 0.35 * np.sin(0.9 * xy[:, 0]) * np.cos(0.8 * xy[:, 1]))
    q["pos"] = np.column_stack([xy, h + 0.3 + 0.65 + rng.uniform(-0.05, 0.04, n)])
    q["rot"] = (0, 0, 0, 1)
    q["radius"] = 0.3; q["half_height"] = 0.65; q["max_separation"] = 0.08; q["ignore_id"] = abi.INVALID_ID; q["collidable_only"] = 1
    mv = rng.normal(size=(n, 3)) * (1, 1, 0.2); mv /= np.linalg.norm(mv, axis=1, keepdims=True)
    q["movement"] = mv
    for edges in (1, 0):
        q["active_edges"] = edges
        ref = w.collide_capsules(q, cap=16384)
        got, total = w.collide_shapes(capsule_as_shape(q), cap=16384)
        assert 150 < len(ref) < 16384 and total == len(ref)
        assert_records_equal_bitwise(got, ref)
    w.close()


# 2 ---------------------------------------------------------------------------------------------------------------

def body_desc(pile, j):
    d = abi.BodyDesc.from_buffer_copy(pile.descs[j:j + 1].tobytes())
    d.pos[:] = pile.states["pos"][j]; d.rot[:] = pile.states["rot"][j]
    return d


def query_desc(q):
    d = abi.BodyDesc()
    d.pos[:] = q["pos"]; d.rot[:] = q["rot"]; d.shape_type = int(q["shape_type"]); d.shape[:] = q["shape"]
    return d


def bound_radius(shape_type, shape, hull_r):
    if shape_type == abi.SHAPE_SPHERE:
        return float(shape[0])
    if shape_type == abi.SHAPE_BOX:
        return float(np.linalg.norm(shape[:3]))
    if shape_type == abi.SHAPE_CAPSULE:
        return float(shape[0] + shape[1])
    return hull_r[int(shape[0])]


@pytest.fixture(scope="module")
def oracle_hulls(oracle):
    """An oracle world that holds the pile's hulls under the pile's ids (no bodies: only its narrow phase is asked)."""
    ow = oracle.OracleWorld(max_bodies=16)
    pts_pile, pts_query = hull_points()
    ids = (ow.hull_create(pts_pile).hull_id, ow.hull_create(pts_query).hull_id)
    yield ow, ids, {ids[0]: float(np.linalg.norm(pts_pile, axis=1).max()) * 2.0, ids[1]: float(np.linalg.norm(pts_query, axis=1).max()) * 2.0}      # (generous: the hull's frame sits at its centre of mass)
    ow.close()


@pytest.mark.parametrize("kind", [abi.SHAPE_SPHERE, abi.SHAPE_BOX, abi.SHAPE_HULL])
def test_sphere_box_and_hull_queries_match_the_oracle_narrow_phase(piles, oracle, oracle_hulls, kind):
    p = piles(None)
    ow, hull_ids, hull_r = oracle_hulls
    assert hull_ids == (p.hull_pile, p.hull_query)
    rng = np.random.default_rng(100 + kind)
    n = 64
    q = shape_queries(rng, n, kind, p)
    q["max_separation"][n // 2:] = 0.0
    q["ignore_id"][::7] = 5
    q["layer_mask"][::5] = 0x3
    got, total = p.w.collide_shapes(q, cap=16384)
    assert total == len(got)
    # brute force: every query against every live body that passes the filters, no broad phase (pairs whose bounding spheres are apart are not asked)
    layers = p.descs["layer"]
    rb = np.array([bound_radius(int(p.descs["shape_type"][j]), p.descs["shape"][j], hull_r) for j in range(p.n_bodies)])
    exp = []
    for k in range(n):
        mask = int(q["layer_mask"][k]) or 0xF
        rq = bound_radius(kind, q["shape"][k], hull_r)
        near = np.linalg.norm(p.states["pos"] - q["pos"][k], axis=1) <= rb + rq + float(q["max_separation"][k]) + 0.05
        near[0] = True                                  # the ground box
        qd = query_desc(q[k])
        for j in np.nonzero(near)[0]:
            if j == int(q["ignore_id"][k]) or not (mask >> int(layers[j])) & 1:
                continue
            r = oracle.world_collide_pair(ow, body_desc(p, j), qd, float(q["max_separation"][k]))
            if r is None:
                continue
            nrm, p1, p2 = r
            for i in range(len(p1)):
                exp.append((k, int(j), p1[i], nrm, float(np.dot((p2[i] - p1[i]).astype(np.float32), nrm))))
    assert [(int(a), int(b)) for a, b in zip(got["query"], got["body"])] == [(e[0], e[1]) for e in exp]      # the same pairs, the same number of points each
    dp = np.max(np.abs(got["point"] - np.array([e[2] for e in exp])))
    dn = np.max(np.abs(got["normal"] - np.array([e[3] for e in exp])))
    dd = np.max(np.abs(got["distance"] - np.array([e[4] for e in exp], np.float32)))
    print(f"kind {kind}: {len(got)} contacts, max |point| {dp:.3g} |normal| {dn:.3g} |distance| {dd:.3g}")
    assert dp <= 1e-5 and dn <= 1e-5 and dd <= 1e-5
    assert len(got) > 50 and (got["distance"] < 0).any()
    assert (got["distance"] <= q["max_separation"][got["query"]] + 1e-5).all()
    assert (got["is_sensor"] == 1).any() or kind != abi.SHAPE_BOX      # (sensors are reported)


# 3 ---------------------------------------------------------------------------------------------------------------

def test_both_organisations_give_one_answer(piles):
    pw, pp, pa = piles("wave"), piles("pairs"), piles(None)
    assert pw.states.tobytes() == pp.states.tobytes() == pa.states.tobytes()
    rng = np.random.default_rng(33)
    q = mixed_queries(rng, pw, 257)
    big = np.zeros(1, dtype=abi.shape_query_dtype)
    big["pos"][0] = (0, 0, 2.0); big["rot"][0] = (0, 0, 0, 1); big["shape_type"] = abi.SHAPE_BOX; big["shape"][0, :3] = 12.0; big["ignore_id"] = abi.INVALID_ID
    q = np.concatenate([q, big])
    rw, nw = pw.w.collide_shapes(q, cap=65536)
    rp, np_ = pp.w.collide_shapes(q, cap=65536)
    ra, na = pa.w.collide_shapes(q, cap=65536)
    assert nw == np_ == na == len(rw) and len(rw) > 1000
    assert rw.tobytes() == rp.tobytes() == ra.tobytes()
    in_big = rw[rw["query"] == 257]
    assert len(np.unique(in_big["body"])) > 64          # more candidates in one query than a wave has lanes, and more than the first guess of the pair list holds
    # a second call (the capacities now follow the first) says the same
    assert pp.w.collide_shapes(q, cap=65536)[0].tobytes() == rp.tobytes()
    # overflow: the first cap records of the sorted whole, and the exact count
    for pile in (pw, pp):
        few, total = pile.w.collide_shapes(q, cap=100)
        assert total == nw > 100 and len(few) == 100
        assert few.tobytes() == rw[:100].tobytes()
    # sorted by (query, body) as documented
    key = rw["query"].astype(np.uint64) << np.uint64(32) | rw["body"].astype(np.uint64)
    assert (np.diff(key.astype(np.int64)) >= 0).all()


# 4 ---------------------------------------------------------------------------------------------------------------

def one_query(kind, pos, shape, max_sep=0.0, rot=(0, 0, 0, 1), **kw):
    q = np.zeros(1, dtype=abi.shape_query_dtype)
    q["pos"][0] = pos; q["rot"][0] = rot; q["shape_type"] = kind; q["shape"][0, :len(shape)] = shape; q["max_separation"] = max_sep; q["ignore_id"] = abi.INVALID_ID
    for k, v in kw.items():
        q[k] = v
    return q


@pytest.mark.parametrize("path", ["wave", "pairs"])
def test_known_answers(piles, path):
    p = piles(path)
    w = p.w
    # a box 0.01 m above the mesh floor (the ground box under it is ignored: the mesh is the subject)
    box = one_query(abi.SHAPE_BOX, (FLOOR_X, 0, 0.51), (0.5, 0.5, 0.5), 0.02, ignore_id=0)
    r, n = w.collide_shapes(box)
    assert n == 4 and (r["body"] == p.floor_id).all() and (r["query"] == 0).all()
    assert np.array_equal(r["normal"], np.tile(np.float32((0, 0, 1)), (4, 1)))
    assert np.max(np.abs(r["distance"] - 0.01)) <= 1e-6
    assert np.max(np.abs(r["point"][:, 2])) <= 1e-6 and sorted(map(tuple, np.round(r["point"][:, :2] - (FLOOR_X, 0), 4))) == [(-0.5, -0.5), (-0.5, 0.5), (0.5, -0.5), (0.5, 0.5)]
    box["max_separation"] = 0.0
    assert w.collide_shapes(box)[1] == 0
    # a sphere in the gap of the compound touches both children
    r, n = w.collide_shapes(one_query(abi.SHAPE_SPHERE, (COMPOUND_X, 0, 0.5), (0.3,), ignore_id=0))
    assert n == 2 and (r["body"] == p.compound_id).all() and sorted(r["sub_shape"]) == [0, 1]
    assert np.max(np.abs(r["distance"] + 0.2)) <= 1e-5
    # deepest only: one record per (query, body), the minimum-distance record of the whole answer
    rng = np.random.default_rng(5)
    q = shape_queries(rng, 64, abi.SHAPE_BOX, p)
    full, _ = w.collide_shapes(q, cap=16384)
    q["flags"] = abi.QUERY_DEEPEST_ONLY
    deep, nd = w.collide_shapes(q, cap=16384)
    keys = full["query"].astype(np.int64) << 32 | full["body"]
    uniq, first = np.unique(keys, return_index=True)
    assert nd == len(deep) == len(uniq) and len(uniq) < len(full)
    pick = [s + int(np.argmin(full["distance"][s:e])) for s, e in zip(first, list(first[1:]) + [len(full)])]
    assert deep.tobytes() == full[pick].tobytes()
    # layers and ignore_id
    # (bit l of layer_mask stands for layer l, as sgp_shape_query says and as 0x3 = collidable_only requires: NON_MOVING_NON_COLLIDABLE is layer 2, so its
    # mask is 1 << 2; 0x2 is bit 1, the MOVING layer -- both are checked)
    big = one_query(abi.SHAPE_BOX, (0, 0, 2.0), (12.0, 12.0, 12.0), layer_mask=0x2)
    r, n = w.collide_shapes(big, cap=16384)
    assert n > 200 and (p.descs["layer"][r["body"]] == abi.LAYER_MOVING).all()
    big["layer_mask"] = 1 << abi.LAYER_NON_MOVING_NON_COLLIDABLE
    r, n = w.collide_shapes(big)
    assert n > 0 and (r["body"] == p.ghost_id).all()
    big["ignore_id"] = p.ghost_id
    assert w.collide_shapes(big)[1] == 0
    big["layer_mask"] = 0
    r, n = w.collide_shapes(big, cap=16384)
    assert n > 200 and not (r["body"] == p.ghost_id).any() and (r["body"] == 0).any()


# 5 ---------------------------------------------------------------------------------------------------------------

def test_rejections_leave_the_world_answering(piles):
    p = piles(None)
    rng = np.random.default_rng(9)
    good = mixed_queries(rng, p, 40)
    before, nb = p.w.collide_shapes(good, cap=16384)
    assert nb > 20

    def spoiled(edit):
        q = good.copy()
        edit(q[17:18])
        return q
    bad = {
        "unknown hull": spoiled(lambda q: (q.__setitem__("shape_type", abi.SHAPE_HULL), q["shape"].__setitem__((0, 0), 77.0))),
        "mesh type": spoiled(lambda q: q.__setitem__("shape_type", abi.SHAPE_MESH)),
        "nan position": spoiled(lambda q: q["pos"].__setitem__((0, 1), np.nan)),
        "zero radius": spoiled(lambda q: (q.__setitem__("shape_type", abi.SHAPE_SPHERE), q["shape"].__setitem__((0, 0), 0.0))),
    }
    for what, q in bad.items():
        with pytest.raises(SgpError, match=r"rc=-1 .*query 17"):
            p.w.collide_shapes(q)
        after, na = p.w.collide_shapes(good, cap=16384)
        assert na == nb and after.tobytes() == before.tobytes(), what
    empty, n0 = p.w.collide_shapes(good[:0])
    assert n0 == 0 and len(empty) == 0


# 6 ---------------------------------------------------------------------------------------------------------------

def test_queries_leave_no_trace_in_the_simulation():
    def world():
        w = make_world(None, max_bodies=512)
        w.add_batch(scenes.small_mixed(5, 3, seed=3))
        return w
    a, b = world(), world()
    for _ in range(10):
        a.step(DT)
    rng = np.random.default_rng(2)
    n = 96
    q = np.zeros(n, dtype=abi.shape_query_dtype)
    q["pos"] = rng.uniform([-4, -4, 0.2], [4, 4, 4.0], size=(n, 3)); q["rot"] = rand_quats(rng, n)
    q["shape_type"] = abi.SHAPE_BOX; q["shape"][:, :3] = 0.5; q["max_separation"] = 0.05; q["ignore_id"] = abi.INVALID_ID
    assert a.collide_shapes(q)[1] > 0 and a.collide_shapes(q[:3])[1] >= 0
    for _ in range(10):
        a.step(DT)
    for _ in range(20):
        b.step(DT)
    assert a.read_states(0, 76).tobytes() == b.read_states(0, 76).tobytes()
    a.close(); b.close()
