"""World checkpoints (sgp_world_checkpoint / rollback / restore): a world that is rolled back, or restored into a fresh world or a fresh
process, continues BIT FOR BIT as the world that was never interrupted.  Everything here compares raw bits (np.array_equal on integer
views); there are no tolerances in this file except in the comparison with the CPU oracle, which is tests/test_parity_gpu.py's."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from substrata_amd import abi, scenes
from substrata_amd.lib import World
from substrata_amd.world import SgpError
from helpers import DT, dyn
import parity
import checkpoint_scenes as cs

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def assert_same(a, b, what):
    assert cs.same(a, b), f"{what}: {cs.first_difference(a, b)}"


def settle(scene, worlds, ctxs, cap=400, quiet=15):
    """Steps the worlds together until the constraint count has stopped rising (no new maximum for `quiet` steps): the pile is in full contact."""
    best, since, k = 0, 0, 0
    while k < cap and since < quiet:
        for w, c in zip(worlds, ctxs):
            scene.drive(w, c, k)
            w.step(DT)
            cs.drain_all(w)
        n = worlds[0].stats().num_manifolds
        best, since = (n, 0) if n > best else (best, since + 1)
        k += 1
    return k


def resume_matches(scene, n1, n2, settle_first=False):
    U, Cw = scene.world(World), scene.world(World)
    cu, cc = scene.make(U), scene.make(Cw)
    if settle_first:
        n1 = settle(scene, [U, Cw], [cu, cc])
        assert U.stats().num_manifolds > 0
    else:
        cs.run(U, scene, cu, 0, n1, rec=False)
        cs.run(Cw, scene, cc, 0, n1, rec=False)
    cp = Cw.checkpoint()
    ru = cs.run(U, scene, cu, n1, n2)
    r1 = cs.run(Cw, scene, cc, n1, n2)
    Cw.rollback(cp)
    r2 = cs.run(Cw, scene, cc, n1, n2)
    assert_same(ru, r1, "a captured world against an uninterrupted one")
    assert_same(ru, r2, "a rolled-back world against an uninterrupted one")
    info = cp.info()
    cp.close(); U.close(); Cw.close()
    return info, n1


def test_mixed_pile_small():
    info, n1 = resume_matches(cs.MixedPile(), 0, 40, settle_first=True)
    assert info["num_cached_contacts"] > 50 and info["steps_taken"] == n1


def test_mixed_pile_20k():
    info, _ = resume_matches(cs.MixedPile20k(), 0, 12, settle_first=True)
    assert info["num_bodies"] > 20000 and info["num_cached_contacts"] > 20000


def test_sleep_and_wake_captured_after_an_idle_step():
    """The whole pile is asleep at the capture (the steps before it were idle: nobody awake, nothing edited); a ball wakes it afterwards."""
    scene = cs.SleepWake(drop_at=215, walker=False)
    U = scene.world(World); cu = scene.make(U)
    cs.run(U, scene, cu, 0, 200, rec=False)
    assert U.stats().num_active == 0 and U.launch_counts()[2] > 0, "the pile should be asleep and the last steps idle"
    U.close()
    resume_matches(scene, 200, 80)


def test_sleep_and_wake_while_somebody_else_is_awake():
    """The pile sleeps, a body elsewhere does not: the contacts of the sleeping pairs are carried in the cache from step to step."""
    scene = cs.SleepWake(drop_at=215, walker=True)
    U = scene.world(World); cu = scene.make(U)
    cs.run(U, scene, cu, 0, 200, rec=False)
    assert U.stats().num_active == 1
    U.close()
    info, _ = resume_matches(scene, 200, 80)
    assert info["num_cached_contacts"] >= 8, "the sleeping pile's contacts should be in the cache"


def test_shapes():
    info, _ = resume_matches(cs.Shapes(), 45, 60)
    assert info["num_hulls"] == 2 and info["num_meshes"] == 4 and info["num_compounds"] == 1


def test_vehicles_mid_drive():
    scene = cs.Vehicles()
    w = scene.world(World); ctx = scene.make(w)
    assert (ctx["car"], ctx["bike"]) == (scene.IDS["car"], scene.IDS["bike"])
    # the capture step: the first one (mid-drive, gears engaged) at which a wheel of the car stands on one of the loose plates in its way -- found in
    # a scout world; every world of the scene takes the same steps, so it is that step in all of them
    n1 = None
    for k in range(300):
        cs.run(w, scene, ctx, k, 1, rec=False)
        vs = w.vehicle_get_states(0, 2)
        wheels = vs["wheels"][0][:4]
        on_plate = (wheels["has_contact"] != 0) & np.isin(wheels["contact_body"], ctx["plates"])
        if k >= 60 and on_plate.any() and (vs["current_gear"] != 0).all():
            n1 = k + 1
            break
    assert n1 is not None, "no wheel of the car came to stand on a dynamic body"
    st = w.read_states(0, scene.max_bodies)
    assert (st["active"][ctx["plates"]] != 0).any()
    w.close()
    info, _ = resume_matches(scene, n1, 90)
    assert info["num_vehicles"] == 2 and info["steps_taken"] == n1


def test_queries_right_after_rollback():
    scene = cs.Shapes()
    w = scene.world(World); ctx = scene.make(w)
    cs.run(w, scene, ctx, 0, 50, rec=False)
    cp = w.checkpoint()
    q0 = cs.query_answers(w)
    cs.run(w, scene, ctx, 50, 40, rec=False)
    q_later = cs.query_answers(w)
    w.rollback(cp)
    q1 = cs.query_answers(w)
    assert not np.array_equal(q0, q_later), "the scene should have moved"
    assert np.array_equal(q0, q1)
    cp.close(); w.close()


def _next_ids(w, scene_ctx):
    """The ids the next ten add / hull_create / mesh_create hand out."""
    out = []
    for k in range(10):
        out.append(dyn(w, pos=(20.0 + k, 20.0, 5.0)))
    for k in range(10):
        out.append(w.hull_create(cs._hull_points(8 + k, 100 + k, (0.3, 0.3, 0.3))).hull_id)
    V, T = cs.box_mesh((-1, -1, 0), (1, 1, 1))
    for k in range(10):
        out.append(w.mesh_create(V * (1.0 + 0.1 * k), T).mesh_id)
    return out


def test_rollback_over_edits():
    scene = cs.Shapes()
    U, Cw = scene.world(World), scene.world(World)
    cu, cc = scene.make(U), scene.make(Cw)
    # a sleeping island next to the scene: two stacked boxes far away, asleep by the capture
    for w in (U, Cw):
        a = dyn(w, pos=(30.0, 30.0, 5.5)); b = dyn(w, pos=(30.0, 30.0, 6.6))
    n1, n2 = 140, 40
    cs.run(U, scene, cu, 0, n1, rec=False)
    cs.run(Cw, scene, cc, 0, n1, rec=False)
    st = Cw.read_states(0, scene.max_bodies)
    cp = Cw.checkpoint()
    cp0 = Cw.checkpoint()
    Cw.rollback(cp0)
    assert cp0.info()["shape_bytes_copied"] == 0, "a rollback with no shape created or destroyed since moves no shape-pool bytes"
    Cw.checkpoint(cp0)
    assert cp0.info()["shape_bytes_copied"] == 0, "a capture into an existing checkpoint with no shape change moves no shape-pool bytes"
    # -- the other history
    added = [dyn(Cw, pos=(-20.0 + 0.1 * k, 15.0, 3.0 + k)) for k in range(50)]
    live = [int(i) for i in np.nonzero(st["id"] != abi.INVALID_ID)[0]]
    dynamic = [i for i in live if st["active"][i] or i >= scene.IDS["paddle"] + 3][:49]      # (dynamic bodies: whatever is awake, and the bodies added last)
    dynamic = [i for i in dynamic if i not in (a, b) and i != scene.IDS["paddle"]]
    for i in dynamic + [a]:      # a: the lower box of the sleeping pair (the root of its island is one of the two)
        Cw.remove(i)
    Cw.remove(b)
    h = Cw.hull_create(cs._hull_points(20, 9, (0.4, 0.4, 0.4))); Cw.hull_destroy(h.hull_id)
    V, T = cs.box_mesh((-1, -1, 0), (1, 1, 1))
    m = Cw.mesh_create(V, T); Cw.mesh_destroy(m.mesh_id)
    Cw.hull_create(cs._hull_points(40, 10, (0.4, 0.4, 0.4)))
    Cw.mesh_create(V * 2.0, T)
    Cw.vehicle_create(Cw.default_vehicle_desc(added[0]))
    Cw.set_water(False, 0.0)
    cs.run(Cw, scene, cc, n1, 7, rec=False)
    Cw.set_water(True, 3.0)
    Cw.set_pos(added[3], (0.0, 0.0, 9.0)); Cw.add_force(added[4], (0.0, 0.0, 9000.0))      # queued, never stepped
    # -- back
    Cw.rollback(cp)
    assert cp.info()["shape_bytes_copied"] > 0, "shapes were created and destroyed since the capture: tables and pools come back"
    ru = cs.run(U, scene, cu, n1, n2)
    rc = cs.run(Cw, scene, cc, n1, n2)
    assert_same(ru, rc, "rollback over edits")
    assert _next_ids(U, cu) == _next_ids(Cw, cc), "ids handed out after a rollback are those of the uninterrupted world"
    ru = cs.run(U, scene, cu, n1 + n2, 10)
    rc = cs.run(Cw, scene, cc, n1 + n2, 10)
    assert_same(ru, rc, "after the new bodies and shapes")
    cp.close(); cp0.close(); U.close(); Cw.close()


def test_pending_events_and_queued_edits():
    scene = cs.MixedPile()
    U, Cw = scene.world(World), scene.world(World)
    cu, cc = scene.make(U), scene.make(Cw)
    for w in (U, Cw):
        for k in range(30):
            w.step(DT)                        # events pile up: nothing is drained
        w.add_force(5, (0.0, 0.0, 40000.0))    # queued, not flushed
        w.set_vel(9, (0.0, 3.0, 0.0), (0.0, 0.0, 0.0))
    assert sum(Cw.event_counts()) > 0
    cp = Cw.checkpoint()
    ru = cs.run(U, scene, cu, 30, 20, sort_first=True)      # (the first drain returns the events of 31 steps)
    r1 = cs.run(Cw, scene, cc, 30, 20, sort_first=True)
    Cw.rollback(cp)
    r2 = cs.run(Cw, scene, cc, 30, 20, sort_first=True)
    assert_same(ru, r1, "capture with pending events and queued edits")
    assert_same(ru, r2, "rollback: the same events are drained again, the edits took effect exactly once")
    cp.close(); U.close(); Cw.close()


def test_foreign_scratch():
    """Between capture and rollback the world lives 200 steps of another history: nothing of it may survive in an array that counts as scratch."""
    scene = cs.MixedPile20k()
    U, Cw = scene.world(World), scene.world(World)
    cu, cc = scene.make(U), scene.make(Cw)
    n1 = settle(scene, [U, Cw], [cu, cc])
    cp = Cw.checkpoint()
    st = Cw.read_states(0, scene.max_bodies)
    ids = np.nonzero((st["id"] != abi.INVALID_ID))[0]
    ids = ids[ids >= 1]
    recs = np.zeros(len(ids[::2]), dtype=abi.pose_vel_dtype)
    recs["pos"] = st["pos"][ids[::2]]; recs["rot"] = st["rot"][ids[::2]]; recs["lin_vel"] = (0.5, -0.5, 14.0); recs["ang_vel"] = (1.0, 2.0, 3.0)
    Cw.set_pose_vel_batch(ids[::2].astype(np.uint32), recs)      # half the bodies thrown upward
    for i in ids[1::8]:
        Cw.remove(int(i))
    for k in range(200):
        Cw.step(DT)
    Cw.rollback(cp)
    ru = cs.run(U, scene, cu, n1, 8)
    rc = cs.run(Cw, scene, cc, n1, 8)
    assert_same(ru, rc, "rollback after a foreign history")
    cp.close(); U.close(); Cw.close()


def test_reuse_and_two_checkpoints():
    scene = cs.MixedPile()
    U, Cw = scene.world(World), scene.world(World)
    cu, cc = scene.make(U), scene.make(Cw)
    cs.run(U, scene, cu, 0, 60, rec=False); cs.run(Cw, scene, cc, 0, 60, rec=False)
    cp = Cw.checkpoint()
    sizes = []
    for k in range(10):
        cs.run(U, scene, cu, 60 + k, 1, rec=False); cs.run(Cw, scene, cc, 60 + k, 1, rec=False)
        assert Cw.checkpoint(cp) is cp
        sizes.append(cp.info()["device_bytes"])
    assert len(set(sizes[5:])) == 1, sizes
    cp.close()
    # two checkpoints at different steps, rolled back in either order
    a = Cw.checkpoint()                                   # step 70
    ra = cs.run(U, scene, cu, 70, 15)
    assert_same(ra, cs.run(Cw, scene, cc, 70, 15), "captured")
    b = Cw.checkpoint()                                   # step 85
    rb = cs.run(U, scene, cu, 85, 15)
    assert_same(rb, cs.run(Cw, scene, cc, 85, 15), "captured twice")
    Cw.rollback(a); assert_same(ra, cs.run(Cw, scene, cc, 70, 15), "first checkpoint")
    Cw.rollback(b); assert_same(rb, cs.run(Cw, scene, cc, 85, 15), "second checkpoint after the first")
    Cw.rollback(b); assert_same(rb, cs.run(Cw, scene, cc, 85, 15), "second checkpoint again")
    Cw.rollback(a); assert_same(ra + rb, cs.run(Cw, scene, cc, 70, 30), "first checkpoint after the second")
    a.close(); b.close(); U.close(); Cw.close()


def _blob_and_reference(scene, n1, n2):
    U, Cw = scene.world(World), scene.world(World)
    cu, cc = scene.make(U), scene.make(Cw)
    cs.run(U, scene, cu, 0, n1, rec=False); cs.run(Cw, scene, cc, 0, n1, rec=False)
    cp = Cw.checkpoint()
    blob = cp.to_bytes()
    assert abi.blob_info(blob) == cp.info()
    ru = cs.run(U, scene, cu, n1, n2)
    cp.close(); U.close(); Cw.close()
    return blob, ru, cc


@pytest.mark.parametrize("name", ["mixed", "shapes", "vehicles"])
def test_restore_into_a_fresh_world(name):
    scene = {"mixed": cs.MixedPile, "shapes": cs.Shapes, "vehicles": cs.Vehicles}[name]()
    blob, ru, ctx = _blob_and_reference(scene, 70, 40)
    for k, v in scene.IDS.items():
        assert ctx[k] == v
    F = scene.world(World)
    F.restore(blob)
    assert_same(ru, cs.run(F, scene, ctx, 70, 40), "a world restored from a blob")
    F.close()


def _run_child(args, env=None):
    e = dict(os.environ)
    e.update(env or {})
    p = subprocess.run([sys.executable, os.path.join(HERE, "checkpoint_child.py")] + [str(a) for a in args], env=e, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, f"child failed ({p.returncode}):\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}"      # (checked before anything else uses the GPU)


def _load(prefix):
    data, lens = np.load(prefix + ".npy"), np.load(prefix + ".len.npy")
    offs = np.concatenate([[0], np.cumsum(lens)])
    return [data[offs[i]:offs[i + 1]] for i in range(len(lens))]


@pytest.mark.parametrize("name", ["shapes", "vehicles"])
def test_restore_in_a_fresh_process(name):
    scene = {"shapes": cs.Shapes, "vehicles": cs.Vehicles}[name]()
    blob, ru, _ = _blob_and_reference(scene, 70, 40)
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "world.ckpt")
        open(path, "wb").write(blob)
        _run_child(["restore", name, path, 70, 40, os.path.join(tmp, "out")])
        assert_same(ru, _load(os.path.join(tmp, "out")), "a world restored in a fresh process")


def test_restore_refusals_leave_the_world_untouched():
    scene = cs.MixedPile()
    blob, _, _ = _blob_and_reference(scene, 40, 1)
    U = scene.world(World); cu = scene.make(U)
    ru = cs.run(U, scene, cu, 0, 30)
    U.close()

    def refused(w, b, built):
        with pytest.raises(SgpError) as e:
            w.restore(b)
        assert "rc=-1" in str(e.value), str(e.value)
        ctx = built if built is not None else scene.make(w)
        return ctx

    # a world of another capacity
    w = World(max_bodies=scene.max_bodies * 2)
    ctx = refused(w, blob, None)
    assert_same(ru, cs.run(w, scene, ctx, 0, 30), "a world that refused a blob of another description")
    w.close()
    # a world that is not fresh
    w = scene.world(World); ctx = scene.make(w)
    refused(w, blob, ctx)
    assert_same(ru, cs.run(w, scene, ctx, 0, 30), "a non-fresh world that refused a blob")
    w.close()
    # truncated blobs, and one with a byte of its sizes changed
    w = scene.world(World)
    for cut in (0, 7, 100, len(blob) // 2, len(blob) - 16, len(blob) - 1):
        refused(w, blob[:cut], {})
    bad = bytearray(blob); bad[40] ^= 0x10
    refused(w, bytes(bad), {})
    refused(w, blob + b"\0" * 16, {})
    ctx = scene.make(w)
    assert_same(ru, cs.run(w, scene, ctx, 0, 30), "a fresh world that refused malformed blobs")
    w.close()


@pytest.mark.parametrize("name", ["mixed", "shapes", "vehicles"])
def test_full_copy_gives_the_same_bits(name):
    """SGP_CHECKPOINT_FULL=1 (every device allocation copied whole) in a child process against the lean path here."""
    scene = {"mixed": cs.MixedPile, "shapes": cs.Shapes, "vehicles": cs.Vehicles}[name]()      # (vehicles: the full copy includes the vehicle rows and heads)
    n1, n2 = 70, 40
    w = scene.world(World); ctx = scene.make(w)
    cs.run(w, scene, ctx, 0, n1, rec=False)
    cp = w.checkpoint()
    a = cs.run(w, scene, ctx, n1, n2)
    w.rollback(cp)
    b = cs.run(w, scene, ctx, n1, n2)
    lean_device_bytes = cp.info()["device_bytes"]
    cp.close(); w.close()
    with tempfile.TemporaryDirectory() as tmp:
        _run_child(["record", name, n1, n2, os.path.join(tmp, "full")], env={"SGP_CHECKPOINT_FULL": "1"})
        full = _load(os.path.join(tmp, "full"))
    assert_same(a + b, full, "full copy against lean copy")
    assert lean_device_bytes > 0


def test_rolled_back_world_is_the_world_the_oracle_describes(oracle):
    from test_parity_gpu import POS_TOL, VEL_TOL
    descs = scenes.small_mixed()
    tw = parity.make_twin(oracle, max_bodies=max(64, len(descs) + 8))
    tw.add_batch(descs)
    n1, n2 = 60, 60
    for _ in range(n1):
        tw.step(DT)
    cp = tw.gpu.checkpoint()
    for _ in range(n2):
        tw.step(DT)
    first = tw.gpu.read_states(0, len(descs))
    tw.gpu.rollback(cp)
    for _ in range(n2):
        tw.gpu.step(DT)
    assert np.array_equal(cs.bits(first), cs.bits(tw.gpu.read_states(0, len(descs))))
    d = parity.compare(tw, len(descs))
    assert d["active_mismatch"] == 0
    assert d["pos"] <= POS_TOL and d["rot"] <= POS_TOL and d["lin_vel"] <= VEL_TOL and d["ang_vel"] <= VEL_TOL, d
    cp.close(); tw.close()


def size_bound(info):
    """What a lean checkpoint may hold at most, from the layout (docs/KERNELS.md, sgp_world_checkpoint.hip), not from what it happens to hold:
    per body slot up to the high-water slot the per-body arrays, 430 B today, 512 B allowed; per cached contact one slot of one constraint buffer
    (480 B) and its share of the hash table (the table is the power of two below 4 x the contacts of this step and the last, 16 B an entry: at most
    128 B per cached contact); 3 MB for what does not scale (the 1 MB start table of the large-body grid, a 16 KB minimum hash table, scalars, 256-byte
    alignment of a hundred pieces); and the quarter of room plus 4 KB the buffer is allocated with."""
    return 1.25 * (512 * info["high_slot"] + (480 + 128) * info["num_cached_contacts"] + 3 * (1 << 20)) + 4096 + 256


def test_size_follows_the_scene_not_the_capacity():
    infos = []
    for n in (1000, 30000):
        w = World(max_bodies=65536)
        side = int(np.ceil((n / 10) ** 0.5))
        d = scenes.config3_100k_mixed(nx=side, ny=side, nz=10)[:n + 1]
        w.add_batch(d)
        for _ in range(20):
            w.step(DT)
        cp = w.checkpoint()
        i = cp.info()
        assert abi.blob_info(cp.to_bytes()) == i
        assert i["num_bodies"] == len(d) and i["high_slot"] == len(d) and i["steps_taken"] == 20
        infos.append(i)
        cp.close(); w.close()
    assert infos[0]["device_bytes"] < infos[1]["device_bytes"] < infos[1]["world_device_bytes"], infos
    for i in infos:      # it follows the scene: bodies and contacts, not the world's capacity (65536 slots, 525k manifolds, 1.3 GB)
        assert i["device_bytes"] <= size_bound(i), (i, size_bound(i))
        assert i["device_bytes"] < 0.05 * i["world_device_bytes"], i
    print("checkpoint / world device bytes:", [(i["device_bytes"], i["world_device_bytes"]) for i in infos])


def test_refusals():
    A, B = World(max_bodies=64), World(max_bodies=64)
    for w in (A, B):
        w.add_batch(scenes.ground()); dyn(w)
        w.step(DT)
    cp = A.checkpoint()
    before = cs.bits(B.read_states(0, 64))
    with pytest.raises(SgpError) as e:
        B.rollback(cp)
    assert "rc=-1" in str(e.value) and "another world" in str(e.value)
    with pytest.raises(SgpError):
        B.checkpoint(cp)
    assert np.array_equal(before, cs.bits(B.read_states(0, 64)))
    # a world that holds a ghost record refuses to be captured
    recs = A.export_boundary((-100, -100, -100), (0.3, 100, 100), 2.0)      # the box at the origin lies within the margin of the region's x face
    assert len(recs) >= 1
    B.import_ghosts(recs)
    with pytest.raises(SgpError) as e:
        B.checkpoint()
    assert "rc=-1" in str(e.value) and "ghost" in str(e.value)
    cp.close(); A.close(); B.close()


def test_checkpoint_outlives_its_world_and_closed_handles():
    w = World(max_bodies=64)
    w.add_batch(scenes.ground()); dyn(w)
    w.step(DT)
    cp = w.checkpoint()
    before = cp.info()
    blob = cp.to_bytes()
    assert abi.blob_info(blob) == before
    closed = w.checkpoint(); closed.close()
    with pytest.raises(SgpError):
        w.checkpoint(closed)           # a closed Checkpoint is refused (the library would otherwise make a new one nobody owns)
    with pytest.raises(SgpError):
        w.rollback(closed)
    lib, h = w._lib, cp._h
    w.close()
    assert cp.info() == before         # the counts are the checkpoint's own
    n = __import__("ctypes").c_uint64(0)
    assert lib.sgp_checkpoint_write(h, None, 0, __import__("ctypes").byref(n)) == abi.ERR_INVALID      # writing needs the world
    assert b"destroyed" in lib.sgp_last_error()
    cp.close()
