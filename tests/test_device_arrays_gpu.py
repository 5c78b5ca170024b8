"""The device arrays of a world that grow after it was created -- the item list of the static large bodies' grid, the vehicle arrays, the
shape tables -- each grown while the step's graphs are already captured, and sgp_step_stats::device_bytes across such growth."""
import numpy as np
import pytest

from substrata_amd import abi, scenes
from substrata_amd.lib import World
from helpers import DT, add_car
import parity
import checkpoint_scenes as cs

pytestmark = pytest.mark.gpu

# ---- the large bodies' grid: more items than its list has room for ----------------------------------------------------------------------------
MAXB, LARGE_R = 8192, 0.3
HALF, NX, NY = 0.25, 50, 50                  # half-metre boxes (bounding radius 0.43 > LARGE_R: large), laid edge to edge as two floors of 50 x 50
BALL_R, N_BALLS = 0.25, 4                    # per floor; small bodies
LG_ITEMS_AT_CREATE = 4096


def _floor(x0):
    d = scenes._blank(NX * NY)
    d["shape_type"] = abi.SHAPE_BOX; d["shape"][:, :3] = HALF
    d["motion_type"] = abi.MOTION_STATIC; d["layer"] = abi.LAYER_NON_MOVING
    d["pos"] = [(x0 + 2 * HALF * i + HALF, 2 * HALF * j + HALF, HALF) for j in range(NY) for i in range(NX)]
    return d


def _balls(x0):
    d = scenes.dynamic_bodies(N_BALLS)
    d["shape_type"] = abi.SHAPE_SPHERE; d["shape"][:, 0] = BALL_R
    d["pos"] = [(x0 + 2 * HALF * (7 + 11 * k) + HALF, 2 * HALF * (5 + 9 * k) + HALF, 3.0) for k in range(N_BALLS)]      # each over the middle of a box
    return d


def _wave(k):
    x0 = 2 * HALF * NX * k
    return np.concatenate([_floor(x0), _balls(x0)])


def _new_world():
    w = World(max_bodies=MAXB, large_body_radius=LARGE_R)
    # Every state read, edit flush and grid rebuild goes through the stage buffer, which grows to one and a half times the largest request so far and counts
    # in device_bytes.  This read asks for more (68 B x 8192) than anything below (a flush: 140 B per new body; a rebuild: 36 B per large static body), so
    # the buffer has its final size from here on, whatever the order of the flushes.
    w.read_states(0, MAXB)
    return w


@pytest.fixture(scope="module")
def lg_growth():
    """World A gets the two floors in two waves with steps after each: its grid is rebuilt twice, and each rebuild finds more items than the list holds.
    World B gets the same bodies in one flush: one rebuild, one growth.  Both end with the same bodies, so with the same arrays."""
    n = 2 * (NX * NY + N_BALLS)
    out = {"slots": n}
    A, B = _new_world(), _new_world()
    out["bytes_fresh"] = (A.stats().device_bytes, B.stats().device_bytes)
    A.add_batch(_wave(0))
    for _ in range(12):
        A.step(DT)
    out["replays_before_second_wave"] = A.launch_counts()[0]
    out["bytes_a_first"] = A.stats().device_bytes
    A.add_batch(_wave(1))
    B.add_batch(_wave(0)); B.add_batch(_wave(1))
    for _ in range(150):
        A.step(DT)
    B.step(DT); B.step(DT)
    out["bytes_final"] = (A.stats().device_bytes, B.stats().device_bytes)
    out["states"] = A.read_states(0, n)
    cp = A.checkpoint()
    out["blob"] = cp.to_bytes()
    cp.close()
    ctx = {"slots": n}
    out["continuation"] = [_step_and_record(A, ctx) for _ in range(20)]
    A.close(); B.close()
    return out


def _step_and_record(w, ctx):
    w.step(DT)
    return cs.record(w, ctx)


def test_lg_items_grow_under_captured_graphs_and_device_bytes_does_not_drift(lg_growth):
    g = lg_growth
    fresh, first, (final_a, final_b) = g["bytes_fresh"][0], g["bytes_a_first"], g["bytes_final"]
    print("device_bytes: fresh", g["bytes_fresh"], "A after the first wave", first, "final (A, B)", g["bytes_final"], "graph replays before the second wave", g["replays_before_second_wave"])
    assert g["bytes_fresh"][0] == g["bytes_fresh"][1]
    assert g["replays_before_second_wave"] > 0                       # the second growth invalidates graphs that are replaying
    # each list is half as large again as the items it was grown for, so a growth adds at least that to the 4096 entries it replaces
    assert first - fresh > 4 * LG_ITEMS_AT_CREATE // 2               # the first wave alone outgrew the list ...
    assert final_a - first > (first - fresh) // 2                    # ... and both waves outgrew the list made for the first
    assert final_a == final_b                                        # the same arrays: the same figure, however often the list was re-made
    st = g["states"]
    balls = np.concatenate([st[NX * NY:NX * NY + N_BALLS], st[-N_BALLS:]])
    assert np.all(balls["id"] != abi.INVALID_ID)
    for f in ("pos", "rot", "lin_vel", "ang_vel"):
        assert np.all(np.isfinite(st[f])), f
    assert np.all(balls["pos"][:, 2] > 2 * HALF) and np.all(balls["pos"][:, 2] < 2 * HALF + 2 * BALL_R), balls["pos"]      # on the boxes: above their tops, no higher than a ball lying there
    assert np.max(np.abs(balls["lin_vel"])) < 0.05, balls["lin_vel"]                                                         # ... and at rest


def test_restore_grows_lg_items(lg_growth):
    """A fresh world has the list it was created with; the blob's is larger."""
    g = lg_growth
    F = _new_world()
    before = F.stats().device_bytes
    F.restore(g["blob"])
    assert F.stats().device_bytes == g["bytes_final"][0] > before      # (same arrays as the world the blob came from, stage buffer included)
    ctx = {"slots": g["slots"]}
    got = [_step_and_record(F, ctx) for _ in range(len(g["continuation"]))]
    assert cs.same(g["continuation"], got), f"a world restored from a blob: {cs.first_difference(g['continuation'], got)}"
    F.close()


# ---- the vehicle arrays past their first capacity ---------------------------------------------------------------------------------------------
VEH_CAP_AT_FIRST = 64


def test_a_65th_vehicle_mid_drive_matches_oracle(oracle):
    """64 cars fill the vehicle arrays as first allocated; the 65th is created while the others drive and a graph replays.  Twin, comparison and tolerances
    of test_vehicle_parity_gpu.test_cars_and_debris_match_oracle."""
    from test_vehicle_parity_gpu import vehicle_diff, drive
    tw = parity.make_twin(oracle, max_bodies=128)
    tw.add_batch(scenes.ground())
    spots = [(-80.0 + 20.0 * (k % 9), -70.0 + 20.0 * (k // 9), 0.75) for k in range(VEH_CAP_AT_FIRST + 1)]      # 20 m apart: nobody meets anybody
    for k in range(VEH_CAP_AT_FIRST):
        ids = [add_car(w, pos=spots[k]) for w in (tw.gpu, tw.cpu)]
        assert ids[0] == ids[1] == (1 + k, k)
    ncars = VEH_CAP_AT_FIRST
    bytes_before = tw.gpu.stats().device_bytes

    def check(s):
        n = 1 + ncars
        d = parity.compare(tw, n)
        assert d["active_mismatch"] == 0, (s, d)
        assert d["pos"] <= 2e-4 and d["rot"] <= 2e-4 and d["lin_vel"] <= 2e-3 and d["ang_vel"] <= 2e-3, (s, d)
        sg, sc = tw.vehicle_get_states(0, ncars)
        vd = vehicle_diff(sg, sc)
        assert vd["engine_rpm"] <= 0.5 and vd["angular_velocity"] <= 1e-2 and vd["suspension_length"] <= 1e-4, (s, vd)
        return d, vd

    for s in range(90):
        if s == 30:
            assert tw.gpu.launch_counts()[0] > 0                      # a graph is replaying
            check(s)
            ids = [add_car(w, pos=spots[ncars]) for w in (tw.gpu, tw.cpu)]
            assert ids[0] == ids[1] == (1 + ncars, ncars)
            ncars += 1
            assert tw.gpu.stats().device_bytes > bytes_before          # the arrays were re-made
        if s % 15 == 0:
            drive(tw, ncars, s)
        tw.step(DT)
        if s in (31, 45, 89):
            d, vd = check(s)
    assert vd["bit_exact"] and d["bit_exact"], (d, vd)
    sg, _ = tw.vehicle_get_states(0, ncars)
    assert np.all(sg["active"] == 1) and (np.abs(sg["wheels"]["angular_velocity"]) > 1.0).any()
    assert np.all(sg["wheels"]["has_contact"][-1][:4] == 1)           # the newcomer stands on its wheels
    tw.close()


# ---- the shape tables past their first capacities ---------------------------------------------------------------------------------------------
MESH_TABLE_AT_CREATE, HULL_TABLE_AT_CREATE = 256, 64      # entries, entry 0 of each taken by the library


def test_shape_tables_grow_after_steps_have_run(oracle):
    """A 257th mesh and a 65th hull, created after steps have run.  A ball on the first mesh and one on the last, a body of the first hull and one of the
    last, none allowed to sleep, collide all the way; device and oracle agree bit for bit."""
    from test_mesh_parity_gpu import mesh_body
    tw = parity.make_twin(oracle, max_bodies=64)
    tw.add_batch(scenes.ground())
    rng = np.random.default_rng(5)

    def quad(k):      # two triangles (one for every third mesh), level and facing up
        z = 0.01 * (k % 4)
        V = np.array([(-2, -2, z), (2, -2, z), (2, 2, z), (-2, 2, z)], np.float32)
        return V, np.array([(0, 1, 2), (0, 2, 3)] if k % 3 else [(0, 1, 2)], np.uint32)

    def tetra(k):
        return (np.array([(1, 1, 1), (1, -1, -1), (-1, 1, -1), (-1, -1, 1)], np.float32) * (0.3 + 0.002 * k) + rng.normal(size=(4, 3)) * 0.02).astype(np.float32)

    def ball_on(x):
        b = scenes.dynamic_bodies(1); b["shape_type"] = abi.SHAPE_SPHERE; b["shape"][0, 0] = 0.3
        b["pos"][0] = (x + 0.5, -1.0, 2.0); b["allow_sleeping"] = 0
        return b

    def hull_body(info, x):
        b = scenes.dynamic_bodies(1); b["shape_type"] = abi.SHAPE_HULL; b["shape"][0] = 0; b["shape"][0, 0] = float(info.hull_id)
        b["pos"][0] = (x, 8.0, 1.0); b["ang_vel"][0] = (0.5, 0.3, 0.0); b["allow_sleeping"] = 0
        return b

    def create(kind, k):
        ig, ic = tw.mesh_create(*quad(k)) if kind == "mesh" else tw.hull_create(tetra(k))
        key = "mesh_id" if kind == "mesh" else "hull_id"
        assert getattr(ig, key) == getattr(ic, key) == k
        return ig

    def add(descs):
        ig, ic = tw.add_batch(descs)
        assert np.array_equal(ig, ic)

    def exact(what):
        d = parity.compare(tw, 64)
        assert d["bit_exact"] and d["active_mismatch"] == 0, (what, d)
        sg, sc = tw.gpu.stats(), tw.cpu.stats()
        assert (sg.num_pairs, sg.num_manifolds, sg.num_contact_points) == (sc.num_pairs, sc.num_manifolds, sc.num_contact_points), what
        return sg

    add(mesh_body(create("mesh", 1), pos=(-10.0, 0.0, 1.0))); add(ball_on(-10.0))
    add(hull_body(create("hull", 1), -10.0))
    for _ in range(40):
        tw.step(DT)
    exact("the first shapes")
    assert tw.gpu.launch_counts()[0] > 0
    bytes_before = tw.gpu.stats().device_bytes
    for k in range(2, MESH_TABLE_AT_CREATE + 2):      # ids up to 257: the table of 256 entries is re-made at id 256
        last_mesh = create("mesh", k)
        if k % 64 == 0:
            tw.step(DT)
    for k in range(2, HULL_TABLE_AT_CREATE + 2):      # ids up to 65: the table of 64 entries is re-made at id 64
        last_hull = create("hull", k)
        if k % 16 == 0:
            tw.step(DT)
    assert tw.gpu.stats().device_bytes > bytes_before
    exact("both tables re-made")
    add(mesh_body(last_mesh, pos=(10.0, 0.0, 1.0))); add(ball_on(10.0))
    add(hull_body(last_hull, 10.0))
    for s in range(90):
        tw.step(DT)
        if s % 30 == 29:
            st = exact(s)
    assert st.num_manifolds >= 4                                   # two balls on their meshes, two hulls on the ground
    z = tw.gpu.read_states(0, 64)["pos"][:, 2]
    balls, hulls = z[[4, 9]], z[[5, 10]]                           # (ground 0, mesh 1-3, ball 4, hull 5; mesh 6-8, ball 9, hull 10)
    assert np.all(balls > 1.25) and np.all(balls < 1.4), balls     # on the quads at z = 1.01 (radius 0.3), not on the ground
    assert np.all(hulls > 0.05) and np.all(hulls < 0.6), hulls
    tw.close()
