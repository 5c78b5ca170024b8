"""The batched particle system on the device (sgp_particles_*, shim/ParticleBatch.h) against a restatement of ParticleManager::think
(gui_client/ParticleManager.cpp:145-274) in this file: vectorised numpy in float32, every step in the reference's order as docs/CONTRACT.md ("Particles") writes
it out, over CWorld.raycast -- the batched ray path the query tests already trust.  The restatement keeps its own list of live particles (stable order: the
batch's documented departure from the reference's swap-with-last) and its own event list, and never reads anything the particle kernels wrote.

After every update the live tags in order, the removals and the event list (tags, kinds, order) must be EQUAL; positions and velocities must agree within the
project's parity tolerance (tests/test_parity_gpu.py:16-17: 1e-4 m, 1e-3 m/s).  Both sides evaluate the same uncontracted fp32 expressions, so bit equality is
the expectation; every comparison prints how many values are bit-equal."""
import json
import subprocess

import numpy as np
import pytest

from substrata_amd import abi, scenes
from substrata_amd.world import SgpError
from test_facade_gpu import build_facade_exe

pytestmark = pytest.mark.gpu

POS_TOL, VEL_TOL = 1.0e-4, 1.0e-3          # tests/test_parity_gpu.py:16-17
DT = 1.0 / 60.0
F = np.float32
DIED, FOAM, REPLACED = abi.PARTICLE_EV_DIED, abi.PARTICLE_EV_FOAM, abi.PARTICLE_EV_REPLACED
DIE_ON_HIT = abi.PARTICLE_DIE_ON_HIT


def new_world(**kw):
    from substrata_amd.lib import World
    return World(**kw)


class Reference:
    """ParticleManager with a stable removal and the batch's round-robin replacement, over CWorld.raycast."""

    def __init__(self, world, capacity, water=(False, 0.0)):
        self.w, self.cap, self.cursor = world, int(capacity), 0
        self.live = np.zeros(0, dtype=abi.particle_dtype)
        self.events = []           # (tag, kind, pos, width, foam_width) since the last take_events()
        self.water_enabled, self.water_z = bool(water[0]), F(water[1])
        self.hit_ids = []          # body id of every hit, in order
        self.deaths_by_fading = self.deaths_by_hit = 0

    def add(self, recs):
        for r in np.asarray(recs, dtype=abi.particle_dtype).reshape(-1):
            if len(self.live) < self.cap:
                self.live = np.append(self.live, r)
            else:
                slot = self.cursor % self.cap
                self.cursor = (self.cursor + 1) % self.cap
                old = self.live[slot]
                self.events.append((int(old["tag"]), REPLACED, old["pos"].copy(), F(old["width"]), F(0)))
                self.live[slot] = r

    def clear(self):
        self.live = self.live[:0]
        self.cursor = 0

    def take_events(self):
        ev, self.events = self.events, []
        return ev

    def update(self, dt):
        p = self.live
        n = len(p)
        if n == 0:
            return
        dt = F(dt)
        pos, vel = p["pos"].astype(F), p["vel"].astype(F)
        width, opacity = p["width"].copy(), p["opacity"].copy()
        die = (p["flags"] & DIE_ON_HIT) != 0
        rays = np.zeros(n, dtype=abi.ray_dtype)
        rays["origin"], rays["dir"], rays["max_t"], rays["ignore_id"], rays["collidable_only"] = pos, vel, dt, abi.INVALID_ID, 0
        if n == 1:      # (a single ray would go to the resident ray server: keep to the batched kernel)
            hits = self.w.raycast(np.concatenate([rays, rays]))[:1]
        else:
            hits = self.w.raycast(rays)
        hit = hits["id"] != abi.INVALID_ID
        self.hit_ids += [int(i) for i in hits["id"][hit]]
        with np.errstate(all="ignore"):
            # :167-191 on a hit
            t, nrm = hits["t"].astype(F), hits["normal"].astype(F)
            hitpos = pos + vel * t[:, None]
            s = F(2) * ((nrm[:, 0] * vel[:, 0] + nrm[:, 1] * vel[:, 1]) + nrm[:, 2] * vel[:, 2])
            vel_h = vel - nrm * s[:, None]
            vel_h = vel_h * p["restitution"][:, None]
            rem = dt - t
            pos_h = (hitpos + nrm * F(1.0e-3)) + vel_h * rem[:, None]
            # :194-212 on a miss
            pos_m = pos + vel * dt
            under = self.water_enabled & (pos_m[:, 2] < self.water_z)
            foam = ~hit & under & die & (vel[:, 2] < 0)
            vel_m = vel.copy()
            vel_m[:, 2] = np.where(under, np.maximum(vel[:, 2], F(0.5)), vel[:, 2] - F(9.81) * dt)
            pos = np.where(hit[:, None], pos_h, pos_m).astype(F)
            vel = np.where(hit[:, None], vel_h, vel_m).astype(F)
            opacity = np.where((hit & die) | foam, F(-1), opacity).astype(F)
            # :218-242 drag
            v2 = (vel[:, 0] * vel[:, 0] + vel[:, 1] * vel[:, 1]) + vel[:, 2] * vel[:, 2]
            gate = v2 > F(1.0e-3) * F(1.0e-3)
            force = (((F(0.5) * F(1.293)) * v2) * F(0.5)) * p["area"]
            a = np.minimum(F(10), force / p["mass"])
            f = np.maximum(F(0), F(1) - (a * dt) / np.sqrt(v2))
            vel = np.where(gate[:, None], vel * f[:, None], vel).astype(F)
            foam_width = width.copy()
            opacity = (opacity + p["dopacity_dt"] * dt).astype(F)
            width = (width + p["dwidth_dt"] * dt).astype(F)
        assert pos.dtype == vel.dtype == width.dtype == opacity.dtype == np.float32
        dead = opacity <= 0
        self.deaths_by_hit += int((dead & hit & die).sum())
        self.deaths_by_fading += int((dead & ~(hit & die) & ~foam).sum())
        for i in np.nonzero(dead | foam)[0]:
            kind = (DIED if dead[i] else 0) | (FOAM if foam[i] else 0)
            self.events.append((int(p["tag"][i]), kind, pos[i].copy(), F(width[i]), F(foam_width[i]) if foam[i] else F(0)))
        p = p.copy()
        p["pos"], p["vel"], p["width"], p["opacity"] = pos, vel, width, opacity
        self.live = p[~dead]


class Tally:
    def __init__(self):
        self.equal = self.total = 0
        self.worst_p = self.worst_v = 0.0

    def count(self, a, b):
        a, b = np.ascontiguousarray(a, dtype=F), np.ascontiguousarray(b, dtype=F)
        self.equal += int((a.view(np.uint32) == b.view(np.uint32)).sum()); self.total += a.size

    def report(self, name):
        print(f"{name}: {self.equal} of {self.total} values bit-equal; worst position difference {self.worst_p:.3g} m, velocity {self.worst_v:.3g} m/s")


def compare_state(ref, got, tally, where):
    """The live particles: tags in order equal, the moving state within tolerance."""
    assert [int(t) for t in ref.live["tag"]] == [int(t) for t in got["tag"]], where
    if not len(got):
        return
    dp, dv = np.abs(ref.live["pos"] - got["pos"]).max(), np.abs(ref.live["vel"] - got["vel"]).max()
    tally.worst_p, tally.worst_v = max(tally.worst_p, float(dp)), max(tally.worst_v, float(dv))
    assert dp <= POS_TOL and dv <= VEL_TOL, (where, dp, dv)
    assert np.abs(ref.live["width"] - got["width"]).max() <= POS_TOL and np.abs(ref.live["opacity"] - got["opacity"]).max() <= POS_TOL, where
    assert np.array_equal(ref.live["flags"], got["flags"]), where
    for f in ("pos", "vel", "width", "opacity"):
        tally.count(ref.live[f], got[f])


def compare_events(ref_events, got, tally, where):
    assert [(e[0], e[1]) for e in ref_events] == [(int(t), int(k)) for t, k in zip(got["tag"], got["kind"])], where
    for e, g in zip(ref_events, got):
        assert np.abs(e[2] - g["pos"]).max() <= POS_TOL and abs(e[3] - g["width"]) <= POS_TOL, (where, e, g)
        assert e[4] == g["foam_width"], (where, e, g)      # the width before the update's growth: a value that was stored, not computed
        tally.count(e[2], g["pos"]); tally.count([e[3]], [g["width"]])


# ---- the main scene ---------------------------------------------------------------------------------------------------------------------------

def quat_x90():
    s = float(np.sqrt(0.5))
    return (s, 0.0, 0.0, s)      # local +y -> world +z (a height field's heights run along local +y)


def build_main_scene(w):
    """A ground quad and one each of box, sphere, capsule, hull, two-triangle mesh, compound and small height field, at rest, in a row along x.
    Returns {name: body id}."""
    ids = {}
    ids["ground"] = int(w.add_batch(scenes.ground())[0])
    rng = np.random.default_rng(5)
    hull = w.hull_create(rng.normal(size=(14, 3)) * 0.6)
    d = scenes.dynamic_bodies(4)      # (never activated, never stepped: small bodies of the cell grid)
    d["activate"] = 0
    d["shape_type"] = [abi.SHAPE_BOX, abi.SHAPE_SPHERE, abi.SHAPE_CAPSULE, abi.SHAPE_HULL]
    d["shape"][0] = (0.9, 0.7, 0.5, 0); d["shape"][1] = (0.8, 0, 0, 0); d["shape"][2] = (0.5, 0.6, 0, 0); d["shape"][3] = (float(hull.hull_id), 0, 0, 0)
    d["pos"] = [(0, 0, 0.9), (4, 0, 1.0), (8, 0, 1.3), (12, 0, 1.0)]
    d["rot"][0] = (0.0, 0.1736482, 0.0, 0.9848078)      # the box tilted by 20 degrees about y
    d["rot"][2] = (0.3826834, 0.0, 0.0, 0.9238795)      # the capsule by 45 degrees about x
    for name, i in zip(("box", "sphere", "capsule", "hull"), w.add_batch(d)):
        ids[name] = int(i)
    V = np.array([(-1.2, -1.2, 0.0), (1.2, -1.2, 0.4), (1.2, 1.2, 0.8), (-1.2, 1.2, 0.4)], dtype=np.float32)
    mi = w.mesh_create(V, np.array([(0, 1, 2), (0, 2, 3)], np.uint32))
    md = scenes._blank(1); md["shape_type"] = abi.SHAPE_MESH; md["shape"][0] = (float(mi.mesh_id), 0, 0, 0); md["pos"][0] = (16, 0, 0.8)
    ids["mesh"] = int(w.add_batch(md)[0])
    ch = np.zeros(2, dtype=abi.compound_child_dtype)
    ch["rot"][:, 3] = 1.0
    ch["shape_type"] = abi.SHAPE_BOX; ch["shape"][0, :3] = (1.0, 0.8, 0.2); ch["shape"][1, :3] = (0.3, 0.3, 0.6); ch["pos"][0] = (0, 0, 0.2); ch["pos"][1] = (0.2, 0, 1.0)
    base = scenes._blank(1); base["pos"][0] = (20, 0, 0.3)
    ids["compound"] = int(w.add_compound(base, ch))
    W = 9
    gx, gz = np.meshgrid(np.arange(W), np.arange(W), indexing="xy")
    heights = (0.6 + 0.25 * np.sin(0.9 * gx) * np.cos(0.7 * gz)).astype(np.float32)
    fi = w.heightfield_create(heights, (0.0, 0.0, 0.0), 0.75)
    fd = scenes._blank(1); fd["shape_type"] = abi.SHAPE_MESH; fd["shape"][0] = (float(fi.mesh_id), 0, 0, 0); fd["pos"][0] = (23.0, 3.0, 0.0); fd["rot"][0] = quat_x90()
    ids["field"] = int(w.add_batch(fd)[0])
    return ids


def main_particles(ps, n=1000, seed=11):
    """n particles over the row of bodies, falling: varied restitution, area, mass, dopacity_dt (-0.3 .. -4: deaths in every wave and most frames), a fifth die on a hit."""
    rng = np.random.default_rng(seed)
    p = ps.defaults(n)
    p["pos"] = rng.uniform([-2.5, -3.0, 0.3], [30.0, 3.0, 4.0], size=(n, 3))
    p["vel"] = rng.uniform([-2.0, -2.0, -8.0], [2.0, 2.0, 0.0], size=(n, 3))
    p["restitution"] = rng.uniform(0.1, 0.9, size=n)
    p["area"] = 1.0e-6 * rng.uniform(0.5, 6.0, size=n)
    p["mass"] = 1.0e-6 * rng.uniform(0.5, 3.0, size=n)
    p["dopacity_dt"] = -rng.uniform(0.3, 4.0, size=n)
    p["dwidth_dt"] = rng.uniform(0.0, 1.0, size=n)
    p["flags"] = np.where(rng.integers(0, 5, size=n) == 0, DIE_ON_HIT, 0)
    p["tag"] = 1000 + np.arange(n)
    return p


def run_main_scene(with_reference, updates=40, event_capacity=4096):
    """The batch's records of the main scene: per update (state bytes, event bytes), with the comparison against the restatement when asked for."""
    w = new_world(max_bodies=256)
    ids = build_main_scene(w)
    ps = w.particles(1024, event_capacity)
    recs = main_particles(ps)
    ps.add(recs)
    ref, tally = None, Tally()
    if with_reference:
        ref = Reference(w, 1024)
        ref.add(recs)
    out = []
    for k in range(updates):
        ps.update(DT)
        got = ps.read()
        ev, dropped = ps.drain_events()
        assert dropped == 0
        out.append((got.tobytes(), ev.tobytes()))
        if ref is not None:
            before = [int(t) for t in ref.live["tag"]]
            ref.update(DT)
            rev = ref.take_events()
            compare_state(ref, got, tally, f"update {k}")
            compare_events(rev, ev, tally, f"update {k}")
            removed = [t for t in before if t not in set(int(x) for x in got["tag"])]
            assert removed == [e[0] for e in rev if e[1] & DIED], f"update {k}"       # the removals are the opacity <= 0 ones, in slot order
            assert (got["opacity"] > 0).all()
    ps.close()
    w.close()
    return out, ref, ids, tally


_main = {}


def main_run():
    if "run" not in _main:
        _main["run"] = run_main_scene(True)
    return _main["run"]


def test_main_scene_equals_the_restatement_at_every_update():
    out, ref, ids, tally = main_run()
    tally.report("main scene, 1000 particles x 40 updates")
    # the restatement met what the test is about (conditions on the reference side)
    hits = np.array(ref.hit_ids)
    assert len(hits) >= 100
    for name, i in ids.items():
        assert (hits == i).sum() >= 1, f"no particle of the restatement hit the {name}"
    assert ref.deaths_by_fading >= 1 and ref.deaths_by_hit >= 1
    print(f"   restatement: {len(hits)} hits ({ {n: int((hits == i).sum()) for n, i in ids.items()} }), {ref.deaths_by_fading} deaths by fading, {ref.deaths_by_hit} by DIE_ON_HIT, {len(ref.live)} alive at the end")
    assert tally.equal == tally.total, "values differ in their bits: find out why before leaning on the tolerance"


def test_main_scene_twice_gives_identical_bytes():
    out, _, _, _ = main_run()
    again, _, _, _ = run_main_scene(False)
    assert again == out


# ---- water --------------------------------------------------------------------------------------------------------------------------------------

def test_water_foam_clamp_and_no_foam_on_the_way_up():
    w = new_world(max_bodies=16)
    g = scenes.ground(); g["pos"][0] = (0.0, 0.0, -20.5)      # (far below: nobody reaches it)
    w.add_batch(g)
    w.set_water(True, 0.5)
    ps = w.particles(256, 1024)
    rng = np.random.default_rng(3)
    n = 200
    p = ps.defaults(n)
    p["pos"] = rng.uniform([-3, -3, 0.55], [3, 3, 1.6], size=(n, 3))
    p["vel"] = rng.uniform([-1, -1, -6.0], [1, 1, -0.5], size=(n, 3))
    p["flags"] = np.where(np.arange(n) % 2 == 0, DIE_ON_HIT, 0)
    p["dopacity_dt"] = -0.3
    p["dwidth_dt"] = rng.uniform(0.2, 1.0, size=n)
    p["width"] = rng.uniform(0.5, 2.0, size=n)
    p["tag"] = 1 + np.arange(n)
    # the last 20 start under water and move up: no foam for them, whatever their flag
    p["pos"][-20:, 2] = 0.2; p["vel"][-20:, 2] = rng.uniform(0.6, 3.0, size=20)
    ps.add(p)
    ref, tally = Reference(w, 256, water=(True, 0.5)), Tally()
    ref.add(p)
    width_of = {int(t): F(x) for t, x in zip(p["tag"], p["width"])}
    foams, clamped = [], 0
    for k in range(15):
        prev = ps.read()
        ps.update(DT)
        got = ps.read()
        ev, _ = ps.drain_events()
        ref.update(DT)
        rev = ref.take_events()
        compare_state(ref, got, tally, f"update {k}")
        compare_events(rev, ev, tally, f"update {k}")
        before = {int(t): r for t, r in zip(prev["tag"], prev)}
        for e in ev:
            if e["kind"] & FOAM:
                b = before[int(e["tag"])]
                assert e["kind"] == (DIED | FOAM) and (b["flags"] & DIE_ON_HIT) and b["vel"][2] < 0
                assert e["foam_width"] == b["width"] and e["width"] > e["foam_width"]      # the decal takes the width before this update's growth
                foams.append(int(e["tag"]))
            else:
                assert e["foam_width"] == 0
        for g in got:      # under water after the move (nothing to hit here): vel.z was clamped to at least 0.5 (drag then shrinks it by a factor close to 1)
            b = before[int(g["tag"])]
            if g["pos"][2] < 0.5 and b["vel"][2] < 0.5:
                clamped += 1
                assert g["vel"][2] > 0.45
    tally.report("water")
    assert len(foams) >= 50 and clamped >= 20
    assert not (set(foams) & set(int(t) for t in p["tag"][-20:])), "foam for a particle that moved up"
    assert all(t % 2 == 1 for t in foams)      # tags 1, 3, ... carry DIE_ON_HIT (index even)
    assert tally.equal == tally.total
    ps.close(); w.close()


# ---- drag edges ---------------------------------------------------------------------------------------------------------------------------------

def test_drag_gate_cap_and_clamp():
    w = new_world(max_bodies=16)
    w.add_batch(scenes.ground())
    ps = w.particles(8, 8)
    dt = F(DT)
    g = F(9.81) * dt                   # a vel.z that the gravity term cancels exactly
    p = ps.defaults(3)
    p["pos"] = [(0, 0, 50), (2, 0, 50), (4, 0, 50)]
    p["dopacity_dt"] = -0.01
    p["tag"] = [1, 2, 3]
    p["vel"][0] = (5.0e-4, 0, g)                                        # below the 1e-3 gate after gravity: untouched by drag
    p["vel"][1] = (30.0, 0, g); p["area"][1] = 1.0e-4                   # F / mass = 2.9e4: capped at 10
    p["vel"][2] = (0.05, 0, g); p["area"][2] = 1.0                      # capped at 10, and 10 dt / 0.05 > 1: the factor clamps to 0
    ps.add(p)
    ref, tally = Reference(w, 8), Tally()
    ref.add(p)
    ps.update(DT); ref.update(DT)
    got = ps.read()
    compare_state(ref, got, tally, "drag")
    assert tuple(got["vel"][0]) == (F(5.0e-4), 0.0, 0.0)
    assert got["vel"][1][0] == F(30.0) * (F(1) - (F(10) * dt) / F(30.0)) and got["vel"][1][0] < 30.0
    assert tuple(got["vel"][2]) == (0.0, 0.0, 0.0)
    assert tally.equal == tally.total
    ps.close(); w.close()


# ---- capacity -----------------------------------------------------------------------------------------------------------------------------------

def plain(ps, n, first_tag, z=50.0):
    p = ps.defaults(n)
    p["pos"][:, 0] = np.arange(n); p["pos"][:, 2] = z
    p["dopacity_dt"] = -0.01
    p["tag"] = first_tag + np.arange(n)
    return p


def test_a_full_batch_replaces_round_robin():
    w = new_world(max_bodies=16)
    w.add_batch(scenes.ground())
    ps = w.particles(128, 1024)
    ref, tally = Reference(w, 128), Tally()
    a, b, c = plain(ps, 100, 1000), plain(ps, 100, 2000), plain(ps, 10, 3000)
    ps.add(a); ref.add(a)
    ps.update(DT); ref.update(DT)
    ps.add(b); ref.add(b)
    got = ps.read()
    ev, dropped = ps.drain_events()
    compare_state(ref, got, tally, "second add")
    compare_events(ref.take_events(), ev, tally, "second add")
    assert dropped == 0 and len(ev) == 72 and (ev["kind"] == REPLACED).all()
    assert [int(t) for t in ev["tag"]] == [1000 + k for k in range(72)]                     # slots 0 .. 71, in order
    assert [int(t) for t in got["tag"]] == [2028 + k for k in range(72)] + [1072 + k for k in range(28)] + [2000 + k for k in range(28)]
    ps.add(c); ref.add(c)                                                                   # the cursor goes on at slot 72
    got = ps.read()
    ev, _ = ps.drain_events()
    compare_state(ref, got, tally, "third add")
    compare_events(ref.take_events(), ev, tally, "third add")
    assert [int(t) for t in ev["tag"]] == [1072 + k for k in range(10)]
    assert [int(t) for t in got["tag"][72:82]] == [3000 + k for k in range(10)]
    # a cursor that has wrapped into the slots the same call fills: newcomers replace newcomers of their own call, as adding one by one would
    ps.clear(); ref.clear()
    d = plain(ps, 120, 4000)
    ps.add(d); ref.add(d)
    e = plain(ps, 128, 5000)
    ps.add(plain(ps, 120, 6000)); ref.add(plain(ps, 120, 6000))      # 8 fit, 112 replace slots 0 .. 111; cursor 112
    ps.add(e); ref.add(e)                                              # none fit: slots 112 .. 127, 0 .. 111
    got = ps.read()
    ev, _ = ps.drain_events()
    compare_state(ref, got, tally, "wrapped")
    compare_events(ref.take_events(), ev, tally, "wrapped")
    assert len(ev) == 112 + 128
    with pytest.raises(SgpError):
        ps.add(plain(ps, 129, 7000))      # SGP_ERR_CAPACITY
    bad = plain(ps, 2, 8000); bad["mass"][1] = 0.0
    with pytest.raises(SgpError):
        ps.add(bad)
    bad = plain(ps, 2, 8000); bad["vel"][0, 1] = np.inf
    with pytest.raises(SgpError):
        ps.add(bad)
    assert ps.read().tobytes() == got.tobytes()      # nothing was added
    ps.close(); w.close()


def test_a_newcomer_replaced_by_its_own_call():
    """capacity 8: after 8 + 6 adds and an update in which two fade out, 6 are live and the cursor stands at 6.  8 at once: 2 fit into slots 6, 7 and the
    other 6 replace slots 6, 7, 0 .. 3 -- the first two of them newcomers of this very call, as adding one by one would have it."""
    w = new_world(max_bodies=16)
    w.add_batch(scenes.ground())
    ps = w.particles(8, 64)
    ref, tally = Reference(w, 8), Tally()
    first = plain(ps, 8, 100); first["opacity"][6:] = 1.0e-4; first["dopacity_dt"][6:] = -1.0      # the last two fade out in the first update
    six = plain(ps, 6, 200)
    for recs in (first, six):
        ps.add(recs); ref.add(recs)
    ps.update(DT); ref.update(DT)
    assert len(ref.live) == 6 and ref.cursor == 6
    eight = plain(ps, 8, 300)
    ps.add(eight); ref.add(eight)
    got = ps.read()
    ev, _ = ps.drain_events()
    compare_state(ref, got, tally, "own call")
    compare_events(ref.take_events(), ev, tally, "own call")
    assert [(int(t), int(k)) for t, k in zip(ev["tag"], ev["kind"])][-6:] == [(t, REPLACED) for t in (300, 301, 200, 201, 202, 203)]
    assert [int(t) for t in got["tag"]] == [304, 305, 306, 307, 204, 205, 302, 303]
    ps.close(); w.close()


# ---- no wait between calls ----------------------------------------------------------------------------------------------------------------------

def test_enqueued_calls_equal_the_same_calls_with_reads_between():
    results = []
    for reads in (False, True):
        w = new_world(max_bodies=256)
        build_main_scene(w)
        ps = w.particles(512, 4096)
        steps = [("add", main_particles(ps, 300, seed=1)), ("update", None), ("add", main_particles(ps, 300, seed=2)), ("update", None), ("update", None)]
        for what, recs in steps:
            ps.add(recs) if what == "add" else ps.update(DT)
            if reads:
                ps.read()
        state = ps.read()
        ev, dropped = ps.drain_events()
        results.append((state.tobytes(), ev.tobytes(), dropped))
        assert len(state) > 100 and (ev["kind"] == REPLACED).sum() > 50      # (the second add's newcomers did not all fit)
        ps.close(); w.close()
    assert results[0] == results[1]


# ---- the world is untouched ---------------------------------------------------------------------------------------------------------------------

def test_body_states_are_bit_identical_with_and_without_particles():
    finals = []
    for with_particles in (False, True):
        w = new_world(max_bodies=512)
        descs = scenes.config3_100k_mixed(10, 10, 2, seed=9)      # the ground and 200 mixed bodies falling onto it
        w.add_batch(descs)
        ps = None
        if with_particles:
            ps = w.particles(512, 4096)
            p = main_particles(ps, 500, seed=4)
            p["pos"][:, :2] *= 0.3      # over the pile
            ps.add(p)
        for k in range(30):
            w.step(DT)
            if ps is not None:
                ps.update(DT)
                ps.add(main_particles(ps, 8, seed=100 + k))
        finals.append(w.read_states(0, len(descs)).tobytes())
        if ps is not None:
            assert len(ps.read()) > 50
            ev, _ = ps.drain_events()
            assert len(ev) > 50
            ps.close()
        w.close()
    assert finals[0] == finals[1]


# ---- edge cases ---------------------------------------------------------------------------------------------------------------------------------

def test_empty_batch_zero_dt_and_clear_then_add():
    w = new_world(max_bodies=256)
    build_main_scene(w)
    ps = w.particles(300, 1024)
    ref, tally = Reference(w, 300), Tally()
    ps.update(DT)                                   # nothing to update
    assert len(ps.read()) == 0 and len(ps.drain_events()[0]) == 0
    with pytest.raises(SgpError):
        ps.update(-1.0)
    with pytest.raises(SgpError):
        ps.update(float("nan"))
    recs = main_particles(ps, 200, seed=6)
    ps.add(recs); ref.add(recs)
    ps.update(0.0); ref.update(0.0)                 # dt = 0: nobody moves, nobody fades; a particle that starts inside a body still hits it at t = 0
    got = ps.read()
    compare_state(ref, got, tally, "dt = 0")
    compare_events(ref.take_events(), ps.drain_events()[0], tally, "dt = 0")
    for k in range(5):
        ps.update(DT); ref.update(DT)
    compare_state(ref, ps.read(), tally, "five updates")
    ps.clear(); ref.clear()
    assert len(ps.read()) == 0
    again = main_particles(ps, 130, seed=7)
    ps.add(again); ref.add(again)
    ps.update(DT); ref.update(DT)
    compare_state(ref, ps.read(), tally, "clear then add")
    compare_events(ref.take_events(), ps.drain_events()[0], tally, "clear then add")      # the deaths before the clear are still reported, in order
    tally.report("edge cases")
    assert tally.equal == tally.total
    ps.close(); w.close()


def test_event_overflow_is_counted():
    w = new_world(max_bodies=256)
    build_main_scene(w)
    ps = w.particles(1024, 16)
    ref, tally = Reference(w, 1024), Tally()
    recs = main_particles(ps)
    ps.add(recs); ref.add(recs)
    for k in range(16):
        ps.update(DT); ref.update(DT)
    rev = ref.take_events()
    assert len(rev) > 16 + 20
    ev, dropped = ps.drain_events()
    assert len(ev) == 16 and dropped == len(rev) - 16
    compare_events(rev[:16], ev, tally, "overflow")
    compare_state(ref, ps.read(), tally, "overflow")
    # the list is empty again and takes the next events from its start
    ps.update(DT); ref.update(DT)
    rev = ref.take_events()
    ev, dropped = ps.drain_events()
    assert dropped == max(0, len(rev) - 16)
    compare_events(rev[:16], ev, tally, "after the drain")
    ps.close(); w.close()


def test_a_batch_outlives_its_world_only_to_be_freed():
    w = new_world(max_bodies=16)
    w.add_batch(scenes.ground())
    ps = w.particles(64, 64)
    ps.add(plain(ps, 10, 1))
    ps.update(DT)
    w.close()
    for call in (lambda: ps.update(DT), lambda: ps.add(plain(ps, 1, 1)), ps.read, ps.drain_events, ps.clear):
        with pytest.raises(SgpError):
            call()
    assert w._fn("particles_destroy")(ps._h) == abi.OK
    ps._h = None


# ---- the facade ---------------------------------------------------------------------------------------------------------------------------------

def test_particle_batch_equals_a_particle_manager_loop(tmp_path):
    """tests/cpp/particles_batch.cpp: ParticleManager's host loop over traceRays() and a ParticleBatch from the same 300 particles, 20 frames."""
    exe = build_facade_exe(tmp_path, "particles_batch.cpp")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    rec = json.loads(r.stdout)
    tally = Tally()
    deaths = 0
    assert len(rec["frames"]) == 20 and rec["events_dropped"] == 0
    for k, fr in enumerate(rec["frames"]):
        h, b = fr["host"], fr["batch"]
        assert h["tags"] == b["tags"], k
        assert h["events"] == b["events"], k
        deaths += len(h["events"])
        if not h["tags"]:
            continue
        hs, bs = np.array(h["state"], dtype=F), np.array(b["state"], dtype=F)      # (%.9g round-trips an fp32 value)
        dp, dv = np.abs(hs[:, 0:3] - bs[:, 0:3]).max(), np.abs(hs[:, 3:6] - bs[:, 3:6]).max()
        tally.worst_p, tally.worst_v = max(tally.worst_p, float(dp)), max(tally.worst_v, float(dv))
        assert dp <= POS_TOL and dv <= VEL_TOL and np.abs(hs[:, 6:8] - bs[:, 6:8]).max() <= POS_TOL, k
        tally.count(hs, bs)
    tally.report("facade, 300 particles x 20 frames")
    assert rec["hits"] >= 100 and deaths >= 20
    assert tally.equal == tally.total
