"""Batch checkpoints (sgp_<batch>_checkpoint / _rollback for characters, particles, crafts and movers): after sgp_world_rollback and one rollback per batch,
the whole scene continues BIT FOR BIT as a scene that was never interrupted, and capturing changes nothing.  Everything here compares raw bytes: what
*_get_states / read, every drain and sgp_world_read_states return, frame by frame.  A frame is: the drains, the inputs, the batch updates, one world step.

Each scene is a part that populates a world and knows its frame; `resume_matches` runs the parts of one world through
  U    n1 + n2 frames, never interrupted, nothing captured;
  C    n1 frames, a capture of the world and of every batch, a FOREIGN history (other inputs, removals, additions: what the part's `foreign` does, then n2 frames
       driven differently), the rollbacks -- the batches first, in reverse order, then the world --, and the n2 frames again, with a capture of everything into a
       second set of checkpoints in every one of them.
The bytes of C's last n2 frames must be U's."""
import ctypes as C
import math

import numpy as np
import pytest

from substrata_amd import abi, scenes
from substrata_amd.lib import World
from substrata_amd.world import SgpError
from helpers import DT, dyn
import craft_reference as cr
import craft_scenes
from test_crafts_gpu import to_abi, inputs_array

pytestmark = pytest.mark.gpu
FALL = -0.1635      # the characters' downward input velocity (tests/test_characters_gpu.py)


# ---- the parts ---------------------------------------------------------------------------------------------------------------------------------------------
class CharactersPart:
    """3 characters on the ground, one pushable box in the way of the first, one stair in the way of the second.  Two more were added and removed again, so
    that the free list has an order.  Contacts are drained in recorded frames only: what the first frames raised is undrained at the capture."""

    def __init__(self, w, at=(0.0, 0.0)):
        self.w, (x, y) = w, at
        self.box = dyn(w, pos=(x + 1.5, y, 0.5), mass=10.0, allow_sleeping=0)
        self.stair = dyn(w, shape=(0.6, 1.0, 0.15), pos=(x - 1.5, y + 3.0, 0.15), motion=abi.MOTION_STATIC, layer=abi.LAYER_NON_MOVING)
        self.cs = cs = w.characters(8)
        self.home = [(x, y, 0.0), (x, y + 3.0, 0.0), (x, y - 3.0, 0.3), (x + 5.0, y, 0.0), (x + 6.0, y, 0.0)]
        ids = [cs.add(self.desc(), p) for p in self.home]
        assert ids == [0, 1, 2, 3, 4]
        cs.remove(4); cs.remove(3)      # the next ids are 3, then 4
        self.batches = [cs]

    def desc(self):
        d = self.cs.default_desc()
        d.up[:] = (0.0, 0.0, 1.0); d.shape_offset[:] = (0.0, 0.0, 0.95); d.supporting_plane[:] = (0.0, 0.0, 1.0, -0.3)
        d.stick_to_floor_step_down[:] = (0.0, 0.0, -0.5); d.walk_stairs_step_up[:] = (0.0, 0.0, 0.4)
        return d

    def drive(self, k, foreign):
        a = np.zeros(3, dtype=abi.character_input_dtype)
        s = -0.5 if foreign else 1.0
        a["velocity"] = [(s * (1.2 + 0.3 * math.sin(0.2 * k)), 0.0, FALL), (-1.0 * s, 0.1 * math.cos(0.3 * k), FALL), (0.0, 0.5 * s, FALL)]
        a["ignore_id"] = abi.INVALID_ID; a["flags"] = abi.CHAR_EXTENDED
        self.cs.set_inputs(0, a)

    def update(self):
        self.cs.update(DT)

    def drains(self):
        return [self.cs.drain_contacts().tobytes()]

    def states(self):
        return [self.cs.states(0, 8).tobytes()]

    def foreign(self):
        """after the capture: character 1 goes, a new one takes its slot and another the next, a third is moved"""
        self.cs.remove(1)
        assert self.cs.add(self.desc(), (50.0, 50.0, 0.0)) == 1 and self.cs.add(self.desc(), (52.0, 50.0, 0.0)) == 3
        self.cs.set_pose([0], [(9.0, 9.0, 0.0)])

    def probe(self):
        """at the end of a run: the ids the next two adds get"""
        return [self.cs.add(self.desc(), (70.0, 70.0, 0.0)), self.cs.add(self.desc(), (72.0, 70.0, 0.0))]


class ParticlesPart:
    """capacity + 44 particles added at once into a batch of `capacity` with room for 8 events: the replacement cursor wraps and events are dropped.  The
    survivors are short-lived -- they fade out in frame 8, raising more events than fit -- but for `live` - 1 of them; one more long-lived particle is added
    behind the last frame before the capture and not updated yet, so `live` particles are live at the capture while the host's bound is the capacity: nothing
    has been read.  From frame 12 on -- behind the capture -- every frame adds three."""

    def __init__(self, w, live, at=(0.0, 0.0)):
        self.w, self.live, self.at = w, live, at
        self.cap = cap = 256 if live <= 200 else 1024
        self.ps = ps = w.particles(cap, 8)
        n = cap + 44
        p = self.plain(n, 1000)
        p["dopacity_dt"] = -7.7                                   # opacity 1 - 7.7 k / 60 <= 0 from frame 8 on
        p["dopacity_dt"][44:44 + max(live - 1, 0)] = -0.01        # (newcomer cap + j replaces slot j: particles 44 .. n - 1 are the survivors)
        ps.add(p[:cap]); ps.add(p[cap:])
        self.batches = [ps]

    def plain(self, n, first_tag):
        p = self.ps.defaults(n)
        p["pos"][:, 0] = self.at[0] + 0.01 * np.arange(n); p["pos"][:, 1] = self.at[1]; p["pos"][:, 2] = 60.0
        p["dopacity_dt"] = -0.01
        p["tag"] = first_tag + np.arange(n)
        return p

    def before_capture(self):
        if self.live:
            self.ps.add(self.plain(1, 5000))

    def drive(self, k, foreign):
        if k >= 12:
            self.ps.add(self.plain(3 if not foreign else 5, (900000 if foreign else 10000) + 10 * k))

    def update(self):
        self.ps.update(DT)

    def drains(self):
        ev, dropped = self.ps.drain_events()
        return [ev.tobytes(), bytes([dropped & 255, dropped >> 8 & 255])]

    def states(self):
        return [self.ps.read().tobytes()]

    def foreign(self):
        self.ps.clear()
        self.ps.add(self.plain(40, 800000))

    def probe(self):
        return []


class CraftsPart:
    """One hover car over the ground box, raising dust, and one capsized boat that starts righting at frame 0 (the timer runs for 2 s: the capture is mid-righting),
    with a particle batch attached."""

    def __init__(self, w):
        self.w = w
        descs, poses, inputs, _ = craft_scenes.twin_scene()
        pick = [0, 3]
        w.set_water(True, craft_scenes.WATER_Z)
        craft_scenes.add_ground_box(w, 8)
        self.bodies = [craft_scenes.add_craft_body(w, descs[i]["kind"], poses[i][0], poses[i][1]) for i in pick]
        self.ps = w.particles(128, 64)
        self.crafts = crafts = w.crafts(4)
        crafts.attach(self.ps)
        for k, i in enumerate(pick):
            assert crafts.add(to_abi(crafts, descs[i], self.bodies[k])) == k
        self.inputs = [inputs[i] for i in pick]
        crafts.set_inputs(0, inputs_array(self.inputs))
        crafts.start_righting([1])
        self.batches = [crafts, self.ps]

    def drive(self, k, foreign):
        inp = [dict(e) for e in self.inputs]
        inp[0]["forward"] = 0.5 + 0.25 * math.sin(0.3 * k) if not foreign else -1.0
        inp[0]["right"] = 0.3 if not foreign else -0.7
        self.crafts.set_inputs(0, inputs_array(inp))

    def update(self):
        self.crafts.update(DT)
        self.ps.update(DT)

    def drains(self):
        ev, dropped = self.ps.drain_events()
        return [ev.tobytes(), bytes([dropped & 255])]

    def states(self):
        return [self.crafts.states(0, 4).tobytes(), self.ps.read().tobytes()]

    def foreign(self):
        """after the capture: the car's body goes, and the next update finds the craft without it"""
        self.w.remove(self.bodies[0])
        self.crafts.update(DT)
        st = self.crafts.states(0, 2)
        assert st["status"][0] == abi.CRAFT_ST_BODY_GONE and st["status"][1] == 0

    def probe(self):
        return [int(s) for s in self.crafts.states(0, 2)["status"]]


def waypoints(rows):
    a = np.zeros(len(rows), dtype=abi.path_waypoint_dtype)
    for k, (pos, typ, pause, speed) in enumerate(rows):
        a[k]["pos"] = pos; a[k]["type"] = typ; a[k]["pause_time"] = pause; a[k]["speed"] = speed
    return a


def kinematic_box(w, pos):
    d = scenes._blank(1)
    d["motion_type"] = abi.MOTION_KINEMATIC; d["layer"] = abi.LAYER_MOVING; d["activate"] = 1
    d["shape"][0, :3] = (1.0, 1.0, 0.2); d["pos"][0] = pos
    return int(w.add_batch(d)[0])


class MoversPart:
    """A walker with one follower on a loop of 4 waypoints -- a straight of 10 at speed 4 behind a station's pause of 0.1 s, then a quarter circle: started at
    3.0 s, the walker is inside the curve from the first frame to beyond the capture -- and one move-to mover on a smoothstep track of 1 s."""
    Z = 8.0

    def loop(self, z):
        return waypoints([((0, 0, z), abi.WAYPOINT_STATION, 0.1, 4.0), ((10, 0, z), abi.WAYPOINT_CURVE_IN, 0.0, 3.0), ((14, 4, z), abi.WAYPOINT_CURVE_OUT, 0.0, 5.0),
                          ((14, 12, z), abi.WAYPOINT_STATION, 0.0, 4.0)])

    def __init__(self, w):
        self.w = w
        self.bodies = [kinematic_box(w, (12.0, 1.0, self.Z)), kinematic_box(w, (11.0, 0.0, self.Z)), kinematic_box(w, (0.0, -8.0, self.Z))]
        self.movers = ms = w.movers(8, 4)
        self.path = ms.add_path(self.loop(self.Z))
        self.leader = ms.add_path_mover(self.bodies[0], self.path, initial_time=3.0, tag=71)
        self.follower = ms.add_path_mover(self.bodies[1], self.path, leader=self.leader, follow_dist=1.0, tag=72)
        self.lift = ms.add_moveto_mover(self.bodies[2], (0.0, -8.0, self.Z), tag=73)
        assert (self.path, self.leader, self.follower, self.lift) == (0, 0, 1, 2)
        ms.set_position_track(self.lift, (0.0, -8.0, self.Z), (4.0, -8.0, self.Z + 2.0), 1.0, abi.MOVER_EASE_SMOOTHSTEP, 0.0)
        self.batches = [ms]

    def drive(self, k, foreign):
        if foreign and k % 4 == 0:
            self.movers.set_position_track(self.lift, (0.0, 0.0, 1.0), (1.0, 1.0, 1.0), 0.5, abi.MOVER_EASE_LINEAR, 0.0)

    def update(self):
        self.movers.update(DT)

    def drains(self):
        return []

    def states(self):
        return [self.movers.states(0, 8).tobytes(), self.movers.path_segments(self.path).tobytes()]

    def foreign(self):
        """after the capture: the follower goes, then (with the walker) its path, and another path takes the slot"""
        ms = self.movers
        ms.remove(self.follower)
        with pytest.raises(SgpError):
            ms.remove_path(self.path)      # the walker still uses it
        ms.remove(self.leader)
        ms.remove_path(self.path)
        assert ms.add_path(self.loop(20.0)) == self.path
        assert ms.add_path_mover(self.bodies[1], self.path, initial_time=1.0) == self.leader      # (the slot freed last)

    def probe(self):
        """at the end of a run: the reference counts let the path go exactly once, when its two walkers are gone"""
        ms, seen = self.movers, []
        for step in (lambda: ms.remove_path(self.path), lambda: ms.remove(self.follower), lambda: ms.remove_path(self.path), lambda: ms.remove(self.leader),
                     lambda: ms.remove_path(self.path), lambda: ms.remove_path(self.path)):
            try:
                step(); seen.append(True)
            except SgpError:
                seen.append(False)
        return seen


# ---- the helper --------------------------------------------------------------------------------------------------------------------------------------------
def frame(w, parts, k, rec=True, foreign=False):
    out = []
    if rec:
        for p in parts:
            out += p.drains()
    for p in parts:
        p.drive(k, foreign)
    for p in parts:
        p.update()
    w.step(DT)
    if rec:
        for p in parts:
            out += p.states()
        out.append(w.read_states().tobytes())
    return out


def run(w, parts, k0, n, **kw):
    return [frame(w, parts, k, **kw) for k in range(k0, k0 + n)]


def batches_of(parts):
    return [b for p in parts for b in p.batches]


def capture(w, parts, into=None):
    """the world's checkpoint and one per batch; into: a set to overwrite in place"""
    bs = batches_of(parts)
    if into is None:
        return [w.checkpoint()] + [b.checkpoint() for b in bs]
    assert w.checkpoint(into[0]) is into[0]
    for b, cp in zip(bs, into[1:]):
        assert b.checkpoint(cp) is cp
    return into


def rollback(w, parts, cps, world_first=False):
    if world_first:
        w.rollback(cps[0])
    for b, cp in reversed(list(zip(batches_of(parts), cps[1:]))):
        b.rollback(cp)
    if not world_first:
        w.rollback(cps[0])


def assert_same(a, b, what):
    assert len(a) == len(b)
    for k, (fa, fb) in enumerate(zip(a, b)):
        assert len(fa) == len(fb)
        for i, (x, y) in enumerate(zip(fa, fb)):
            assert x == y, f"{what}: frame {k}, record {i} differs ({len(x)} and {len(y)} bytes)"


def make(build, max_bodies=96):
    w = World(max_bodies=max_bodies)
    w.add_batch(scenes.ground())
    return w, build(w)


def close(w, parts, *cp_sets):
    for cps in cp_sets:
        for cp in cps:
            cp.close()
    for b in batches_of(parts):
        b.close()
    w.close()


def resume_matches(build, n1, n2, world_first=False):
    (U, pu), (Cw, pc) = make(build), make(build)
    for w, parts in ((U, pu), (Cw, pc)):
        run(w, parts, 0, n1, rec=False)
        for p in parts:
            if hasattr(p, "before_capture"):
                p.before_capture()
    cps = capture(Cw, pc)
    infos = [cp.info() for cp in cps]
    ru = run(U, pu, n1, n2)
    for p in pc:
        p.foreign()
    run(Cw, pc, n1, n2, foreign=True)
    rollback(Cw, pc, cps, world_first)
    spare, rc = None, []
    for k in range(n1, n1 + n2):
        spare = capture(Cw, pc, spare)      # a capture in every frame changes nothing
        rc.append(frame(Cw, pc, k))
    assert_same(ru, rc, "a rolled-back scene against an uninterrupted one")
    assert any(len(x) for f in ru for x in f[:-1])
    probes = [(a.probe(), b.probe()) for a, b in zip(pu, pc)]
    for a, b in probes:
        assert a == b
    close(U, pu); close(Cw, pc, cps, spare)
    return infos, ru, [a for a, _ in probes]


# ---- the scenes --------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world_first", [False, True])
def test_characters(world_first):
    infos, ru, probes = resume_matches(lambda w: [CharactersPart(w)], 20, 30, world_first)
    i = infos[1]
    assert (i["kind"], i["capacity"], i["high_slot"], i["num_alive"], i["world_steps_taken"]) == (abi.BATCH_CHARACTERS, 8, 5, 3, 20) and infos[0]["steps_taken"] == 20
    assert len(ru[0][0]) > 0, "contact records raised before the capture should have been left for the first drain after it"
    assert probes[0] == [3, 4]


@pytest.mark.parametrize("live", [0, 1, 63, 64, 65, 511, 512, 513])
def test_particles(live):
    infos, ru, _ = resume_matches(lambda w: [ParticlesPart(w, live)], 12, 10)
    cap = 256 if live <= 200 else 1024
    i = infos[1]
    # the host's bound at the capture is the capacity (nothing was read), far above the live count; the checkpoint's buffer is sized by the bound
    assert (i["kind"], i["capacity"], i["high_slot"]) == (abi.BATCH_PARTICLES, cap, cap) and i["device_bytes"] >= 64 * cap
    states = abi.particle_state_dtype.itemsize
    assert len(ru[0][2]) == states * (live + 3), "the live count at the capture"      # (+ the three of the first frame after it)
    ev = np.frombuffer(ru[0][0], dtype=abi.particle_event_dtype)
    assert len(ev) == 8 and ru[0][1] != b"\0\0", "undrained events and a dropped count at the capture"


def test_crafts():
    infos, ru, probes = resume_matches(lambda w: [CraftsPart(w)], 20, 20)
    assert [i["kind"] for i in infos[1:]] == [abi.BATCH_CRAFTS, abi.BATCH_PARTICLES] and infos[1]["num_alive"] == 2
    assert probes[0] == [0, 0], "the car is attached to its body again"
    st = np.frombuffer(ru[0][2], dtype=abi.craft_state_dtype)
    assert st["branches"][1] & cr.BR["RIGHTING"], "the capture should be mid-righting"
    assert sum(len(f[3]) for f in ru) > 0, "the crafts should have raised particles"


def test_movers():
    infos, ru, probes = resume_matches(lambda w: [MoversPart(w)], 20, 20)
    assert infos[1]["kind"] == abi.BATCH_MOVERS and infos[1]["num_alive"] == 3
    st = np.frombuffer(ru[0][0], dtype=abi.mover_state_dtype)
    assert st["waypoint_index"][0] == 1 and st["status"][2] & abi.MOVER_ST["POS_ACTIVE"], "captured inside the curve and mid-ease"
    assert probes[0] == [False, True, False, True, True, False]


def everything(w):
    return [CharactersPart(w, at=(40.0, -60.0)), ParticlesPart(w, 65, at=(-40.0, -60.0)), CraftsPart(w), MoversPart(w)]


def test_everything_together():
    resume_matches(everything, 16, 12)


def test_two_checkpoints_alternated():
    (U, pu), (Cw, pc) = make(everything), make(everything)
    run(U, pu, 0, 10, rec=False); run(Cw, pc, 0, 10, rec=False)
    ru = run(U, pu, 10, 16)
    A = capture(Cw, pc)
    run(Cw, pc, 10, 6)      # (recorded like U's, for the drains are part of the history)
    B = capture(Cw, pc)
    run(Cw, pc, 16, 3, foreign=True)
    rollback(Cw, pc, A)
    assert_same(ru[:8], run(Cw, pc, 10, 8), "back to A")
    rollback(Cw, pc, B, world_first=True)
    assert_same(ru[6:], run(Cw, pc, 16, 10), "on to B")
    rollback(Cw, pc, A)
    capture(Cw, pc, B)      # B overwritten with A's moment
    run(Cw, pc, 10, 2, foreign=True)
    rollback(Cw, pc, B)
    assert_same(ru[:4], run(Cw, pc, 10, 4), "back to B, which is A's moment now")
    close(U, pu); close(Cw, pc, A, B)


# ---- refusals and lifetime ---------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_batch_untouched():
    (U, pu), (Cw, pc) = make(everything), make(everything)
    run(U, pu, 0, 6, rec=False); run(Cw, pc, 0, 6, rec=False)
    chars, parts_, crafts, craft_ps, movers = batches_of(pc)
    other_world, other_parts = make(lambda w: [CharactersPart(w)])
    foreign_cp = other_parts[0].cs.checkpoint()
    own = {b: b.checkpoint() for b in (chars, parts_, crafts, movers)}
    refused = 0
    for b in (chars, parts_, crafts, craft_ps, movers):
        fn = Cw._fn(b._stem + "_rollback")
        assert fn(b._h, None) == abi.ERR_INVALID                                     # NULL
        assert Cw._fn(b._stem + "_checkpoint")(b._h, None) == abi.ERR_INVALID
        for cp in [foreign_cp] + [c for o, c in own.items() if o is not b]:            # another batch of the kind, another kind, the other particle batch
            with pytest.raises(SgpError):
                b.rollback(cp)
            with pytest.raises(SgpError):
                b.checkpoint(cp)
            refused += 2
    assert refused == 42
    assert_same(run(U, pu, 6, 3), run(Cw, pc, 6, 3), "after the refusals")
    # a closed BatchCheckpoint is refused by the wrapper
    closed = chars.checkpoint(); closed.close()
    with pytest.raises(SgpError):
        chars.checkpoint(closed)
    with pytest.raises(SgpError):
        chars.rollback(closed)
    # a world that holds ghost bodies, as the updates refuse
    before = [x for p in pc for x in p.states()]
    bx = float(U.get_state([pu[0].box])["pos"][0][0])      # the characters' box lies within the margin of the region's x face
    recs = U.export_boundary((-1000, -1000, -1000), (bx + 0.3, 1000, 1000), 2.0)
    assert len(recs) >= 1
    Cw.import_ghosts(recs)
    for b in (chars, parts_, crafts, movers):
        with pytest.raises(SgpError) as e:
            b.checkpoint()
        assert "ghost" in str(e.value)
        with pytest.raises(SgpError) as e:
            b.rollback(own[b])
        assert "ghost" in str(e.value)
    assert before == [x for p in pc for x in p.states()]
    foreign_cp.close()
    close(other_world, other_parts); close(U, pu); close(Cw, pc, list(own.values()))


def test_reuse_keeps_device_bytes_and_a_checkpoint_outlives_its_world():
    w, parts = make(everything)
    run(w, parts, 0, 4, rec=False)
    cps = capture(w, parts)
    first = [cp.info() for cp in cps[1:]]
    handles = [cp._h.value for cp in cps]
    run(w, parts, 4, 4, rec=False)
    capture(w, parts, cps)
    again = [cp.info() for cp in cps[1:]]
    assert handles == [cp._h.value for cp in cps]
    for a, b in zip(first, again):
        assert a["device_bytes"] == b["device_bytes"] > 0 and a["kind"] == b["kind"] and b["world_steps_taken"] == a["world_steps_taken"] + 4 == 8
    # a batch whose world is gone refuses; the checkpoints still answer and go
    bs = batches_of(parts)
    w.close()
    for b, cp in zip(bs, cps[1:]):
        lib_fn = w._fn(b._stem + "_rollback")
        assert lib_fn(b._h, cp._h) == abi.ERR_INVALID
        h = C.c_void_p()
        assert w._fn(b._stem + "_checkpoint")(b._h, C.byref(h)) == abi.ERR_INVALID and h.value is None
    for cp, info in zip(cps[1:], again):
        got = abi.BatchCheckpointInfo()
        assert w._fn("batch_checkpoint_get_info")(cp._h, C.byref(got)) == abi.OK and got.as_dict() == info
        assert w._fn("batch_checkpoint_destroy")(cp._h) == abi.OK
        cp._h = C.c_void_p()
    for b in bs:
        b.close()
    cps[0].close()
