"""The two batched world queries of the character controller (sgp_collide_capsules, sgp_spherecast; what JPH::CharacterVirtual asks
the world, /root/reference/gui_client/PlayerPhysics.cpp:258-353,477-481): GPU against the oracle on a settled mixed pile with hulls."""
import numpy as np
import pytest

from substrata_amd import abi, scenes
from helpers import DT
import parity

pytestmark = pytest.mark.gpu


def test_capsule_contacts_and_sphere_casts_match_oracle(oracle):
    rng = np.random.default_rng(8)
    tw = parity.make_twin(oracle, max_bodies=1024)
    descs = scenes.small_mixed(8, 3, seed=12)
    tw.add_batch(descs)
    ig, ic = tw.hull_create(rng.normal(size=(14, 3)) * 0.6)
    hd = scenes.dynamic_bodies(20)
    hd["shape_type"] = abi.SHAPE_HULL; hd["shape"][:, 0] = float(ig.hull_id); hd["shape"][:, 1:] = 0
    hd["pos"] = rng.uniform([-4, -4, 1], [4, 4, 5], size=(20, 3))
    tw.add_batch(hd)
    sens = scenes.dynamic_bodies(1); sens["is_sensor"] = 1; sens["motion_type"] = abi.MOTION_STATIC; sens["pos"][0] = (0, 0, 1.0); sens["shape"][0, :3] = 1.0
    tw.add_batch(sens)
    for _ in range(200):
        tw.step(DT)
    n = 256
    q = np.zeros(n, dtype=abi.capsule_query_dtype)
    q["pos"] = rng.uniform([-5, -5, 0.2], [5, 5, 3.0], size=(n, 3))
    quat = rng.normal(size=(n, 4)); quat /= np.linalg.norm(quat, axis=1, keepdims=True)
    q["rot"] = quat; q["rot"][: n // 2] = (0, 0, 0, 1)                       # half of them upright like a player
    q["radius"] = 0.3; q["half_height"] = 0.65; q["max_separation"] = 0.12
    q["ignore_id"] = abi.INVALID_ID; q["ignore_id"][::7] = 5
    q["collidable_only"] = 1
    cg, cc = tw.collide_capsules(q)
    assert len(cg) == len(cc) and len(cg) > 100
    assert np.array_equal(cg["query"], cc["query"]) and np.array_equal(cg["body"], cc["body"])
    for f in ("point", "normal", "distance", "point_velocity", "inv_mass"):
        assert np.max(np.abs(cg[f] - cc[f])) <= 1e-5, f
    assert np.array_equal(cg["motion_type"], cc["motion_type"]) and np.array_equal(cg["is_sensor"], cc["is_sensor"])
    assert (cg["distance"] <= 0.12 + 1e-5).all() and (cg["is_sensor"] == 1).any() and (cg["distance"] < 0).any()
    assert not ((cg["body"] == 5) & (q["ignore_id"][cg["query"]] == 5)).any()
    # sphere casts: downwards from above the pile, sideways through it
    rays = np.zeros(n, dtype=abi.ray_dtype)
    rays["origin"] = rng.uniform([-5, -5, 3.0], [5, 5, 6.0], size=(n, 3))
    d = rng.normal(size=(n, 3)) * (0.5, 0.5, 0.2) + (0, 0, -1.0); d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays["dir"] = d; rays["max_t"] = rng.uniform(0.5, 8.0, size=n); rays["ignore_id"] = abi.INVALID_ID; rays["collidable_only"] = 1
    radii = rng.choice([0.0, 0.1, 0.3], size=n).astype(np.float32)
    hg, hc = tw.spherecast(rays, radii)
    assert np.array_equal(hg["id"], hc["id"]) and (hg["id"] != abi.INVALID_ID).sum() > 100
    assert np.max(np.abs(hg["t"] - hc["t"])) <= 1e-5 and np.max(np.abs(hg["normal"] - hc["normal"])) <= 1e-5
    # a thicker cast never travels further than a thinner one along the same ray
    h0, _ = tw.spherecast(rays, np.zeros(n, np.float32)); h3, _ = tw.spherecast(rays, np.full(n, 0.3, np.float32))
    both = (h0["id"] != abi.INVALID_ID) & (h3["id"] != abi.INVALID_ID)
    assert (h3["t"][both] <= h0["t"][both] + 1e-4).all()
    tw.close()


def test_capsule_queries_on_a_mesh_with_active_edges_match_oracle(oracle):
    """what CharacterVirtual::GetContactsAtPosition asks (CollideOnlyWithActive + the direction of travel), on a terrain mesh: the same contacts on both sides,
    and a query standing beside a seam of a flat stretch gets the flat normal with the flag and a leaning one without"""
    from test_mesh_parity_gpu import grid_mesh, mesh_body
    rng = np.random.default_rng(4)
    tw = parity.make_twin(oracle, max_bodies=64)
    V, T = grid_mesh(25, 12.0, lambda x, y: 0.0 if abs(x) < 4 and abs(y) < 4 else 0.35 * np.sin(0.9 * x) * np.cos(0.8 * y))
    ig, ic = tw.mesh_create(V, T)
    tw.add_batch(mesh_body(ig))
    n = 512
    q = np.zeros(n, dtype=abi.capsule_query_dtype)
    xy = rng.uniform(-10, 10, size=(n, 2))
    h = np.where((np.abs(xy[:, 0]) < 4) & (np.abs(xy[:, 1]) < 4), 0.0, 0.35 * np.sin(0.9 * xy[:, 0]) * np.cos(0.8 * xy[:, 1]))
    q["pos"] = np.column_stack([xy, h + 0.3 + 0.65 + rng.uniform(-0.05, 0.04, n)])
    q["rot"] = (0, 0, 0, 1)
    q["radius"] = 0.3; q["half_height"] = 0.65; q["max_separation"] = 0.08; q["ignore_id"] = abi.INVALID_ID; q["collidable_only"] = 1
    mv = rng.normal(size=(n, 3)) * (1, 1, 0.2); mv /= np.linalg.norm(mv, axis=1, keepdims=True)
    q["movement"] = mv; q["active_edges"] = 1
    q["active_edges"][::5] = 0
    cg, cc = tw.collide_capsules(q)
    assert len(cg) == len(cc) and len(cg) > 300
    assert np.array_equal(cg["query"], cc["query"]) and np.array_equal(cg["body"], cc["body"])
    for f in ("point", "normal", "distance"):
        assert np.array_equal(cg[f].view(np.uint32), cc[f].view(np.uint32)), f
    # on the flat middle (vertices at whole metres: the triangles between 3 and 4 m already slope): without the flag some queries beside a seam see a
    # leaning normal -- a slope that is not there; walking INTO that slope with the flag set, the contact carries the floor's normal
    flat = (np.abs(q["pos"][cg["query"], 0]) < 2.5) & (np.abs(q["pos"][cg["query"], 1]) < 2.5)
    q2 = q.copy(); q2["active_edges"] = 0
    pg, pc = tw.collide_capsules(q2)
    flat2 = (np.abs(q2["pos"][pg["query"], 0]) < 2.5) & (np.abs(q2["pos"][pg["query"], 1]) < 2.5)
    leaning = flat2 & (pg["normal"][:, 2] < 0.99)
    assert flat.sum() > 30 and leaning.sum() >= 5
    q3 = q2[pg["query"][leaning]].copy()
    nxy = pg["normal"][leaning].copy(); nxy[:, 2] = 0; nxy /= np.linalg.norm(nxy, axis=1, keepdims=True)
    q3["movement"] = -nxy; q3["active_edges"] = 1
    fg, fc = tw.collide_capsules(q3)
    assert np.array_equal(fg["normal"].view(np.uint32), fc["normal"].view(np.uint32))
    # (other seams around the same capsule may still answer with their own normals when the walk does not run into them: what must be gone is every normal
    # that leans AGAINST the direction of travel -- the floor is flat)
    against = np.einsum("ij,ij->i", fg["normal"][:, :2], q3["movement"][fg["query"], :2])
    assert (against > -1e-4).all(), against.min()
    before = np.einsum("ij,ij->i", pg["normal"][leaning][:, :2], -nxy[:, :2])
    assert (before < -0.1).all()
    tw.close()


def _walk_scene(w):
    """All three sources of candidates of the queries' walk (sq_walk) in one small scene: 36 static large tiles (at least 32 of them: the static large bodies'
    grid), one moving large body (the linear list of large bodies) and 40 small bodies (the cell rows).  Never stepped: the bodies hang where they are put."""
    rng = np.random.default_rng(17)
    tiles = scenes._blank(36)
    gx, gy = np.meshgrid(np.arange(6), np.arange(6), indexing="ij")
    tiles["pos"][:, 0] = -5.0 + 2.0 * gx.ravel(); tiles["pos"][:, 1] = -5.0 + 2.0 * gy.ravel(); tiles["pos"][:, 2] = 0.25 + 0.05 * (np.arange(36) % 4)
    tiles["shape"][:, :3] = (0.95, 0.95, 0.25)
    mover = scenes.dynamic_bodies(1)
    mover["motion_type"] = abi.MOTION_KINEMATIC; mover["shape"][0, :3] = (1.2, 0.4, 0.8); mover["pos"][0] = (0.3, 0.2, 1.6); mover["lin_vel"][0] = (0.5, 0.0, 0.0)
    small = scenes.dynamic_bodies(40)
    small["pos"] = rng.uniform([-5, -5, 0.8], [5, 5, 2.2], size=(40, 3)); small["shape"][:, :3] = rng.uniform(0.15, 0.3, size=(40, 3))
    small["shape_type"][::2] = abi.SHAPE_SPHERE
    ids = w.add_batch(np.concatenate([tiles, mover, small]))
    assert np.array_equal(ids, np.arange(77))
    return range(0, 36), 36, range(37, 77)


def test_the_walk_agrees_between_its_one_lane_and_wave_instances_and_between_capsule_entry_points():
    """sq_walk's instances against each other, bit for bit, where all three sources of candidates answer.  (1) Its two-bounds form: sgp_spherecast (one lane takes
    every candidate) against the sweep of a character of a batch (the candidates dealt to 64 lanes) along the same segment.  A character with no contact at its
    start, one collision iteration and a capsule of half height 0 moves by velocity * dt * min(len, max(0, t - padding)) / len, t being the sphere cast's answer
    over len + padding when that hit faces the motion (char_sweep_fraction): the expected position is evaluated here in fp32 from sgp_spherecast's hit.
    (2) Its one-bounds form: sgp_collide_capsules for one capsule against the capsule-typed sgp_collide_shapes in both organisations."""
    from test_shape_queries_gpu import make_world, capsule_as_shape, assert_records_equal_bitwise
    f = np.float32
    worlds = {path: make_world(path, max_bodies=256, large_body_radius=1.0) for path in ("wave", "pairs")}
    for w in worlds.values():
        tile_ids, mover_id, small_ids = _walk_scene(w)
    w = worlds["wave"]
    rng = np.random.default_rng(3)

    # (1) the starts: free of contacts within the character's reach (so that no constraint touches the velocity)
    radius, padding, predictive, dt = f(0.3), f(0.02), f(0.1), f(0.05)
    n = 160
    start = rng.uniform([-5, -5, 1.0], [5, 5, 3.0], size=(n, 3))
    start[:48] = rng.uniform([-1.8, -1.4, 1.0], [2.4, 1.8, 3.3], size=(48, 3))      # (a good share of them around the moving large body)
    start = start.astype(f)
    vel = (rng.normal(size=(n, 3)) * (0.6, 0.6, 0.3) + (0, 0, -0.8)); vel = (vel / np.linalg.norm(vel, axis=1, keepdims=True) * rng.uniform(10.0, 30.0, size=(n, 1))).astype(f)
    q = np.zeros(n, dtype=abi.capsule_query_dtype)
    q["pos"] = start; q["rot"] = (0, 0, 0, 1); q["radius"] = radius; q["half_height"] = 0.0; q["max_separation"] = 0.13; q["ignore_id"] = abi.INVALID_ID; q["collidable_only"] = 1
    touched = np.unique(w.collide_capsules(q, cap=16384)["query"])
    free = np.setdiff1d(np.arange(n), touched)[:64]
    assert len(free) == 64
    start, vel = start[free], vel[free]
    disp = vel * dt                                                                   # solveConstraints without constraints: 0 + velocity * time
    length = np.sqrt(disp[:, 0] * disp[:, 0] + disp[:, 1] * disp[:, 1] + disp[:, 2] * disp[:, 2])
    direction = disp * (f(1.0) / length)[:, None]
    rays = np.zeros(64, dtype=abi.ray_dtype)
    rays["origin"] = start; rays["dir"] = direction; rays["max_t"] = length + padding; rays["ignore_id"] = abi.INVALID_ID; rays["collidable_only"] = 1
    hits = w.spherecast(rays, np.full(64, radius, f))
    hit = hits["id"] != abi.INVALID_ID
    hn = hits["normal"]
    facing = (hn[:, 0] * direction[:, 0] + hn[:, 1] * direction[:, 1] + hn[:, 2] * direction[:, 2]) < f(-0.05)
    stops = hit & (hits["t"] > f(1.0e-5)) & facing
    travel = np.where(stops, np.minimum(length, np.maximum(f(0.0), hits["t"] - padding)), length)
    expected = start + disp * (travel / length)[:, None]
    assert expected.dtype == np.float32
    # every source of candidates stopped somebody, and somebody went the whole way
    stoppers = set(hits["id"][stops].tolist())
    assert stoppers & set(tile_ids) and mover_id in stoppers and stoppers & set(small_ids) and (~hit).any(), sorted(stoppers)

    cs = w.characters(64)
    d = cs.default_desc()
    d.radius = float(radius); d.half_height = 0.0; d.up[:] = (0.0, 0.0, 1.0); d.character_padding = float(padding); d.predictive_contact_distance = float(predictive)
    d.max_collision_iterations = 1
    for p in start:
        cs.add(d, p)
    inp = np.zeros(64, dtype=abi.character_input_dtype)
    inp["velocity"] = vel; inp["ignore_id"] = abi.INVALID_ID; inp["flags"] = 0      # CharacterVirtual::Update: no stick-to-floor, no stairs
    cs.set_inputs(0, inp)
    cs.update(float(dt))
    got = cs.states(0, 64)
    cs.close()
    assert not got["overflow"].any()
    assert got["pos"].tobytes() == expected.tobytes(), np.abs(got["pos"] - expected).max()

    # (2) one capsule at a time, where the mover, tiles and small bodies are within reach
    c = np.zeros(12, dtype=abi.capsule_query_dtype)
    c["pos"] = rng.uniform([-2.0, -1.5, 0.9], [2.5, 1.5, 1.8], size=(12, 3))
    quat = rng.normal(size=(12, 4)); quat /= np.linalg.norm(quat, axis=1, keepdims=True)
    c["rot"] = quat; c["rot"][:6] = (0, 0, 0, 1)
    c["radius"] = 0.4; c["half_height"] = 0.8; c["max_separation"] = 0.3; c["ignore_id"] = abi.INVALID_ID; c["ignore_id"][::5] = mover_id; c["collidable_only"] = 1
    bodies = set()
    for k in range(12):
        ref = w.collide_capsules(c[k:k + 1], cap=1024)
        bodies |= set(ref["body"].tolist())
        for path, wp in worlds.items():
            got, total = wp.collide_shapes(capsule_as_shape(c[k:k + 1]), cap=1024)
            assert total == len(ref) < 1024, (k, path)
            assert_records_equal_bitwise(got, ref)
    assert bodies & set(tile_ids) and mover_id in bodies and bodies & set(small_ids), sorted(bodies)
    for wp in worlds.values():
        wp.close()


def test_single_rays_through_the_resident_server_equal_the_batched_answers():
    """PhysicsWorld::traceRay is called one ray at a time by unchanged callers (ParticleManager.cpp:164, HoverCarPhysics.cpp:348): such rays go to a
    resident wave through a host-mapped mailbox (round 5) that traces each with all 64 lanes.  The answers must be those of the batched kernel, bit for
    bit, on a pile with hulls over a terrain mesh -- also when the world is edited or stepped between two rays (the server is told to leave, the next
    ray starts another)."""
    from substrata_amd.lib import World
    rng = np.random.default_rng(21)
    w = World(max_bodies=2048)
    descs = scenes.small_mixed(8, 3, seed=5)
    w.add_batch(descs)
    # a bumpy terrain under and around the pile (rays that miss the bodies hit its triangles: triangle index, material, barycentrics travel too)
    gx = np.linspace(-12, 12, 25); gy = np.linspace(-12, 12, 25)
    vx, vy = np.meshgrid(gx, gy, indexing="ij")
    verts = np.stack([vx.ravel(), vy.ravel(), 0.25 + 0.15 * np.sin(vx.ravel()) * np.cos(0.7 * vy.ravel())], axis=1).astype(np.float32)
    tris = []
    for i in range(24):
        for j in range(24):
            a = i * 25 + j; tris += [(a, a + 25, a + 1), (a + 1, a + 25, a + 26)]
    mi = w.mesh_create(verts, np.array(tris, np.uint32), materials=np.arange(len(tris)) % 7)
    md = scenes.dynamic_bodies(1); md["motion_type"] = abi.MOTION_STATIC; md["layer"] = abi.LAYER_NON_MOVING
    md["shape_type"] = abi.SHAPE_MESH; md["shape"][0] = (float(mi.mesh_id), 0, 0, 0); md["pos"][0] = (0, 0, 0)
    w.add_batch(md)
    hi = w.hull_create(rng.normal(size=(16, 3)) * 0.5)
    hd = scenes.dynamic_bodies(24)
    hd["shape_type"] = abi.SHAPE_HULL; hd["shape"][:, 0] = float(hi.hull_id); hd["shape"][:, 1:] = 0
    hd["pos"] = rng.uniform([-4, -4, 1], [4, 4, 5], size=(24, 3))
    w.add_batch(hd)
    for _ in range(120):
        w.step(DT)
    n = 600
    rays = np.zeros(n, dtype=abi.ray_dtype)
    rays["origin"] = rng.uniform([-6, -6, 0.2], [6, 6, 6.0], size=(n, 3))
    d = rng.normal(size=(n, 3)) + (0, 0, -0.8); d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays["dir"] = d; rays["max_t"] = rng.uniform(0.05, 9.0, size=n); rays["ignore_id"] = abi.INVALID_ID; rays["ignore_id"][::9] = 7
    rays["collidable_only"] = rng.integers(0, 2, size=n)
    batched = w.raycast(rays)
    assert (batched["id"] != abi.INVALID_ID).sum() > 200 and (batched["triangle"] != abi.INVALID_ID).sum() > 20
    single = np.concatenate([w.raycast(rays[k:k + 1]) for k in range(n)])
    assert single.tobytes() == batched.tobytes()
    # edits and a step between single rays: each answer equals the batched answer in the state it was asked in
    for k in range(0, 120, 3):
        if k % 2 == 0:
            w.set_pos(1 + (k % 40), (float(rng.uniform(-3, 3)), float(rng.uniform(-3, 3)), 2.5))
        else:
            w.step(DT)
        one = w.raycast(rays[k:k + 1]); two = w.raycast(rays[k + 1:k + 2])
        ref = w.raycast(rays[k:k + 2])
        assert one.tobytes() == ref[:1].tobytes() and two.tobytes() == ref[1:].tobytes(), k
    w.close()
