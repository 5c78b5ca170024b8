"""The proximity and zone watchers on the device (sgp_proximity_*) against the numpy float32 restatement of tests/proximity_reference.py (written from
docs/CONTRACT.md 4l), which is fed the bodies' bounds as tests/proximity_scenes.py computes them from the shapes and the poses the world reports, and never reads
what the proximity kernels wrote.  Everything is discrete: near masks after every update and the drained events WITH THEIR ORDER must be equal."""
import json
import os
import re
import subprocess

import numpy as np
import pytest

from substrata_amd import abi, scenes
import proximity_reference as pr
import proximity_scenes as ps

pytestmark = pytest.mark.gpu

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = abi.INVALID_ID
EV = abi.PROX_EV


def kernel_constant(name):
    """A #define of csrc/sgp_kernels.h, resolved through other #defines."""
    src = open(os.path.join(ROOT, "substrata_amd", "csrc", "sgp_kernels.h")).read()
    v = re.search(r"#define %s\s+(\w+)" % name, src).group(1)
    return int(v) if v.isdigit() else kernel_constant(v)


WG = kernel_constant("PROX_WG")                      # lanes of a workgroup: objects per count
SCAN_PASS = kernel_constant("PROX_SCAN_PASS")        # counts the scan's single workgroup takes in one pass
BEYOND_ONE_PASS = WG * SCAN_PASS + 1                 # the first size whose counts need a second pass
SIZES = [1, 63, 64, 65, 255, 256, 257, BEYOND_ONE_PASS]      # the wave, workgroup and scan-pass edges


def test_sizes_follow_the_kernels_constants():
    assert (WG, SCAN_PASS, BEYOND_ONE_PASS) == (256, 256, 65537)


@pytest.mark.parametrize("observers", [1, 2, 32])
@pytest.mark.parametrize("n", SIZES)
def test_transitions_along_a_walk(n, observers):
    """Observers walk a polyline through static, kinematic (on sgp_movers) and falling bodies; a zone is removed on the way and its slot refilled."""
    rig = ps.Rig(n, observers)
    updates = 40
    total, kinds, groups = 0, set(), {}      # groups: update -> workgroups of the test launch whose objects raised events
    for u in range(updates):
        if u == 6:
            rig.px.remove_zone(rig.zone_slot[1]); rig.sim.remove_zone(rig.zone_slot[1])
        if u == 9:
            z = rig.px.add_zone((5.0, -5.0, -1.0), (30.0, 12.0, 8.0), 10)
            assert z == rig.zone_slot[1]                                  # the slot freed last comes back
            rig.sim.add_zone(z, (5.0, -5.0, -1.0), (30.0, 12.0, 8.0), 10)
        rig.frame()
        if u % 3 == 2 or u == updates - 1:
            got = rig.check_drain()
            total += len(got)
            kinds |= {g[0] for g in got}
            for g in got:
                if g[1] != INVALID:
                    groups.setdefault(g[5], set()).add(g[1] // WG)
    if n == BEYOND_ONE_PASS:
        # the scene reaches what the size is there for: counts that are not zero in every wave of the scan's workgroup and in its second pass, in several updates
        # (the strip zone's objects and the far objects of tests/proximity_scenes.py), so that every event's place depends on the carry between waves and passes
        last = (n - 1) // WG
        assert last == SCAN_PASS and any(last in g for g in groups.values())
        wide = [u for u, g in groups.items() if len(g) > 64 * 2 and max(g) >= SCAN_PASS - 1]
        assert len(wide) >= 2 and max(wide) > 0, sorted((u, len(g), max(g)) for u, g in groups.items())
        assert len([u for u, g in groups.items() if max(g) >= 64]) >= 3
    obs = rig.px.observers(0, observers)
    for k in range(observers):
        assert int(obs[k]["update_index"]) == updates and int(obs[k]["zone_key"]) == rig.sim.obs[k]["key"], k
        assert np.array_equal(obs[k]["pos"], rig.sim.obs[k]["pos"]), k
    print("proximity walk n=%d observers=%d: %d updates, %d events, kinds %s" % (n, observers, updates, total, sorted(kinds)))
    assert total > 0 and EV["ENTERED"] in kinds
    if n >= 63:
        assert {EV["NEAR"], EV["AWAY"], EV["EXITED"], EV["ENTERED"]} <= kinds
    rig.close()


def static_boxes(w, centres, half=(1.0, 1.0, 1.0)):
    d = scenes._blank(len(centres))
    d["pos"] = np.asarray(centres, F32)
    d["shape"][:, :3] = half
    return np.asarray(w.add_batch(d), dtype=np.uint32)


def test_exact_boundary_cases():
    w = ps.new_world(max_bodies=64)
    x = np.nextafter(F32(21.0), F32(0.0))
    # faces at x = 20 and one float32 nearer; the closest point (12, 16, 0); a box [3, 5]^3 whose centroid lies on the zone's min face at 4
    bodies = static_boxes(w, [(21.0, 0.0, 0.0), (x, 50.0, 0.0), (13.0, 17.0, 0.0), (4.0, 4.0, 4.0)])
    px = w.proximity(8, 4, 256)
    ids = px.add(bodies, 20.0)
    px.add_zone((4.0, 4.0, 4.0), (9.0, 9.0, 9.0), 77)
    px.set_observer(0, pos=(0.0, 0.0, 0.0))
    px.set_observer(1, pos=(0.0, 50.0, 0.0))
    px.set_observer(2, pos=(9.0, 5.0, 5.0))      # exactly on the zone's max face: inside
    px.update()
    st = px.states(0, 4)
    assert int(st["near_mask"][0]) & 1 == 0      # dist2 = 400: NOT near, the comparison is strict
    assert int(st["near_mask"][1]) & 2 == 2      # dist2 = 399.99994: near
    assert int(st["near_mask"][2]) & 1 == 0      # 144 + 256 = 400: not near
    obs = px.observers(0, 3)
    assert [int(o["zone_key"]) for o in obs] == [INVALID, INVALID, 77]
    got = ps.records(px.drain_events()[0])
    assert got[0] == (EV["ENTERED"], INVALID, 2, 77, 0, 0)      # the observer-level record comes first
    assert (EV["ENTERED"], int(ids[3]), 2, 77, 0, 0) in got       # centroid (3 + 5) * 0.5 = 4 on the min face: inside
    assert not [g for g in got if g[0] == EV["ENTERED"] and g[1] in (int(ids[0]), int(ids[1]), int(ids[2]))]
    assert (EV["NEAR"], int(ids[1]), 1, INVALID, 0, 0) in got and not [g for g in got if g[0] == EV["NEAR"] and g[1] == int(ids[0]) and g[2] == 0]
    px.close(); w.close()


def test_want_flags():
    w = ps.new_world(max_bodies=64)
    bodies = static_boxes(w, [(0.0, 0.0, 0.0), (3.0, 0.0, 0.0)])
    px = w.proximity(8, 4, 256)
    ids = px.add(bodies, 5.0, flags=np.array((0, abi.PROX_WANT_NEAR), np.uint32), tags=np.array((11, 12), np.uint64))
    px.set_observer(0, pos=(0.0, 0.0, 0.0))
    px.update()
    assert [int(m) for m in px.states(0, 2)["near_mask"]] == [1, 1]      # the mask takes the bit whether or not the event is wanted
    assert ps.records(px.drain_events()[0]) == [(EV["NEAR"], int(ids[1]), 0, INVALID, 12, 0)]
    px.set_flags(int(ids[0]), abi.PROX_WANT_NEAR)                        # setting the flag later replays nothing
    px.update()
    assert ps.records(px.drain_events()[0]) == []
    px.set_points(0, (100.0, 0.0, 0.0))
    px.update()
    assert ps.records(px.drain_events()[0]) == [(EV["AWAY"], int(ids[0]), 0, INVALID, 11, 2), (EV["AWAY"], int(ids[1]), 0, INVALID, 12, 2)]
    assert [int(m) for m in px.states(0, 2)["near_mask"]] == [0, 0]
    px.close(); w.close()


def test_zones_enter_exit_remove_and_refill():
    w = ps.new_world(max_bodies=64)
    bodies = static_boxes(w, [(2.0, 0.0, 0.0), (12.0, 0.0, 0.0), (30.0, 0.0, 0.0)], half=(0.5, 0.5, 0.5))
    px = w.proximity(8, 4, 256)
    ids = [int(i) for i in px.add(bodies, 1.0, flags=abi.PROX_WANT_ZONE, tags=np.array((1, 2, 3), np.uint64))]
    za = px.add_zone((0.0, -5.0, -5.0), (15.0, 5.0, 5.0), 9)       # holds objects 0 and 1
    zb = px.add_zone((10.0, -5.0, -5.0), (25.0, 5.0, 5.0), 4)      # holds object 1; overlaps A on [10, 15]
    px.set_observer(0, pos=(-50.0, 0.0, 0.0))
    px.set_observer(5, pos=(12.0, 1.0, 0.0))      # in both from the start: the lower key
    events = []

    def step(pos):
        px.set_points(0, pos)
        px.update()
        got = ps.records(px.drain_events()[0])
        events.append(got)
        return [(g[0], g[1], g[2], g[3]) for g in got]

    X, E = EV["EXITED"], EV["ENTERED"]
    assert step((-50.0, 0.0, 0.0)) == [(E, INVALID, 5, 4), (E, ids[1], 5, 4)]                            # observer 0 is nowhere; observer 5 gets key 4, not 9
    assert step((5.0, 0.0, 0.0)) == [(E, INVALID, 0, 9), (E, ids[0], 0, 9), (E, ids[1], 0, 9)]           # enter A
    assert step((12.0, 0.0, 0.0)) == []                                                                  # in the overlap: it stays in A, the higher key
    assert step((20.0, 0.0, 0.0)) == [(X, INVALID, 0, 9), (E, INVALID, 0, 4), (X, ids[0], 0, 9), (X, ids[1], 0, 9), (E, ids[1], 0, 4)]      # A -> B; object 1 lies in both
    assert step((12.0, 0.0, 0.0)) == []                                                                  # back in the overlap: it stays in B now
    px.remove_zone(zb)                                                                                   # the zone it stands in goes: no EXITED, ENTERED for the next containing zone
    assert step((12.0, 0.0, 0.0)) == [(E, INVALID, 0, 9), (E, INVALID, 5, 9), (E, ids[0], 0, 9), (E, ids[0], 5, 9), (E, ids[1], 0, 9), (E, ids[1], 5, 9)]
    px.remove_zone(za)
    z2 = px.add_zone((0.0, -5.0, -5.0), (15.0, 5.0, 5.0), 2)                                             # the slot refilled between two updates: another zone, no EXITED for the old one
    assert z2 == za
    assert step((12.0, 0.0, 0.0)) == [(E, INVALID, 0, 2), (E, INVALID, 5, 2), (E, ids[0], 0, 2), (E, ids[0], 5, 2), (E, ids[1], 0, 2), (E, ids[1], 5, 2)]
    assert step((40.0, 0.0, 0.0)) == [(X, INVALID, 0, 2), (X, ids[0], 0, 2), (X, ids[1], 0, 2)]          # out of every zone
    assert [int(o["zone_key"]) for o in px.observers(0, 6)] == [INVALID] * 5 + [2]
    with pytest.raises(Exception):
        px.add_zone((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), 2)                                                 # keys are unique among live zones
    assert [g[5] for got in events for g in got] == sorted(g[5] for got in events for g in got)          # update indices only grow
    px.close(); w.close()


def test_many_zones_the_lowest_key_wins_wherever_its_slot_is():
    """More zones than the observers' workgroup has lanes: the containing zone of the lowest key sits in a later wave's lane, or in a later trip of the lanes'
    loop over the table, and the zone an observer stands in is found beyond the first 256 slots."""
    w = ps.new_world(max_bodies=16)
    bodies = static_boxes(w, [(0.0, 0.0, 0.0)])
    px = w.proximity(4, 700, 256)
    obj = int(px.add(bodies, 1.0, flags=abi.PROX_WANT_ZONE)[0])
    around = {70: 2900, 130: 2800, 300: 2700, 450: 2600, 255: 2650, 256: 2640, 699: 2950}      # slot -> key of the zones around the origin (lanes 70, 130, 44, 194, 255, 0, 187)
    slots, mins, maxs, keys = [], [], [], []
    for z in range(700):
        mn, mx = ((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0)) if z in around else ((10.0 + z, 0.0, 0.0), (10.5 + z, 1.0, 1.0))
        key = around.get(z, z + 1)                            # the far zones' keys are all lower than the near ones': only `contains` keeps them out
        slots.append(px.add_zone(mn, mx, key)); mins.append(mn); maxs.append(mx); keys.append(key)
    assert slots == list(range(700))
    live = [1] * 700
    px.set_observer(0, pos=(0.0, 0.0, 0.0))
    px.set_observer(3, pos=(10.25 + 600, 0.5, 0.5))           # stands in the zone of slot 600 alone
    X, E = EV["EXITED"], EV["ENTERED"]
    want_key = None
    for step in range(len(around) + 1):
        px.update()
        z = pr.pick_zone(np.array(mins, F32), np.array(maxs, F32), keys, live, INVALID, (0.0, 0.0, 0.0))      # (the zone it was in has just been removed: a fresh choice)
        prev_key, want_key = want_key, (keys[z] if z != INVALID else INVALID)
        obs = px.observers(0, 4)
        assert int(obs[0]["zone_key"]) == want_key and int(obs[3]["zone_key"]) == 600 + 1, step
        got = [g[:4] for g in ps.records(px.drain_events()[0]) if g[2] == 0]
        assert got == ([(E, INVALID, 0, want_key), (E, obj, 0, want_key)] if z != INVALID else []), (step, got, prev_key)
        if z != INVALID:
            px.remove_zone(z); live[z] = 0                    # the next update finds the next lowest key: 2600 (slot 450), 2640 (256), 2650 (255), 2700 (300), 2800, 2900, 2950
    assert want_key == INVALID and step == len(around)
    px.close(); w.close()


def test_overflow_keeps_the_head_of_the_order():
    n, cap = 300, 37
    full = ps.Rig(n, 2, event_capacity=1 << 16, radius=35.0)
    small = ps.Rig(n, 2, event_capacity=cap, radius=35.0)
    a, b = full.frame(), small.frame()
    assert a == b and len(a) > 4 * cap                    # one update raises far more than the small batch holds
    all_events = full.check_drain()
    kept = small.check_drain()                            # (against the restatement, which keeps the head and counts the rest)
    assert kept == all_events[:cap] and small.last_dropped == len(all_events) - cap      # exactly the head of the order, and the count is exact
    # the next update's events follow after the drain
    a, b = full.frame(), small.frame()
    assert a == b and len(a) > 0
    got_full, got_small = full.check_drain(), small.check_drain()
    assert got_small == got_full[:cap] and all(g[5] == 1 for g in got_small) and small.last_dropped == max(len(got_full) - cap, 0)
    # without a drain in between the buffer fills once and every later event is dropped and counted
    for _ in range(12):
        full.frame(); small.frame()
    got_full, got_small = full.check_drain(), small.check_drain()
    assert len(got_full) > cap and got_small == got_full[:cap] and small.last_dropped == len(got_full) - cap
    full.close(); small.close()


def test_lifetimes():
    rig = ps.Rig(40, 3, radius=20.0)
    w, px = rig.w, rig.px
    for _ in range(3):
        rig.frame()
    rig.check_drain()
    # a body is removed and its slot refilled: BODY_GONE, and no events for the newcomer
    victim = 7
    w.remove(int(rig.bodies[victim]))
    w.step(ps.DT)
    newcomer = int(w.add_batch(_one_box((4.0, 4.0, 1.0)))[0])
    assert newcomer == int(rig.bodies[victim])
    rig.there[victim] = False
    mask_before = int(rig.sim.mask[victim])
    for _ in range(3):
        rig.frame()
    got = rig.check_drain()
    assert not [g for g in got if g[1] == victim]
    st = px.states(victim, 1)[0]
    assert int(st["status"]) == abi.PROX_ST_BODY_GONE and int(st["near_mask"]) == mask_before
    with pytest.raises(Exception):
        px.add([int(rig.bodies[0])])                      # one object of the batch per body
    fresh = int(px.add([newcomer], 20.0, tags=[5])[0])    # the gone object has let go of the body: a new object may watch the newcomer
    assert fresh == 40
    rig.sim.add([fresh], 20.0, 3, [5]); rig.there[fresh] = True; rig.extra[fresh] = (newcomer, np.array((0.5, 0.5, 0.5), F32))
    rig.frame()
    got = rig.check_drain()
    assert [g for g in got if g[1] == fresh and g[4] == 5]      # it starts near nobody, so whoever is in range fires
    # an observer is removed and re-added: everything in range fires NEAR again
    rig.px.remove_observer(0); rig.sim.remove_observer(0)
    assert not (px.states(0, rig.capacity)["near_mask"] & 1).any()      # its bit has left every mask at once
    rig.px.set_observer(0, pos=ps.walk(0, rig.u)); rig.sim.set_observer(0)
    ev = rig.frame()
    assert len([e for e in ev if e[0] == EV["NEAR"] and e[2] == 0]) > 5
    rig.check_drain()
    assert int(px.observers(0, 1)[0]["update_index"]) == 1
    # a body-sourced observer's body is removed: the observer stops updating, and a status bit says so
    assert rig.rider is not None
    before = px.observers(1, 1)[0]
    w.remove(rig.rider[0])
    rig.there[rig.rider[0] - rig.first] = False
    rig.rider = (None, rig.rider[1])
    ev = rig.frame()
    assert not [e for e in ev if e[2] == 1]
    after = px.observers(1, 1)[0]
    assert int(after["status"]) & abi.PROX_OBS_ST_BODY_GONE and int(after["update_index"]) == int(before["update_index"]) and np.array_equal(after["pos"], before["pos"])
    assert not [g for g in rig.check_drain() if g[2] == 1]
    # calls after the world is destroyed are refused; destroy still frees
    w.close()
    for call in (px.update, lambda: px.states(0, 1), px.drain_events, lambda: px.add([1]), lambda: px.set_points(0, (0, 0, 0)), lambda: px.observers(0, 1), px.checkpoint):
        with pytest.raises(Exception):
            call()
    px.close()
    rig.movers.close()


def _one_box(pos):
    d = scenes._blank(1)
    d["pos"][0] = pos
    return d


def test_refusals():
    w = ps.new_world(max_bodies=64)
    bodies = static_boxes(w, [(0.0, 0.0, 0.0), (3.0, 0.0, 0.0)])
    for objects, zones, events in ((0, 4, 64), ((1 << 20) + 1, 4, 64), (16, 0, 64), (16, (1 << 12) + 1, 64), (16, 4, 0)):
        with pytest.raises(Exception):
            w.proximity(objects, zones, events)            # a capacity of 0 or beyond its maximum, with a real world
    px = w.proximity(2, 1, 16)
    for bad in (dict(radius=0.0), dict(radius=float("nan")), dict(flags=4)):
        with pytest.raises(Exception):
            px.add(bodies[:1], **bad)
    with pytest.raises(Exception):
        px.add([bodies[0], bodies[0]])                    # named twice
    with pytest.raises(Exception):
        px.add([63])                                      # not a live body
    assert px.states(0, 2)["near_mask"].tolist() == [0, 0] and len(px.add(bodies)) == 2      # nothing was taken by the refused calls
    with pytest.raises(Exception):
        px.add(static_boxes(w, [(9.0, 0.0, 0.0)]))        # full
    with pytest.raises(Exception):
        px.set_observer(32, pos=(0, 0, 0))
    with pytest.raises(Exception):
        px.set_observer(0, pos=(float("inf"), 0, 0))
    with pytest.raises(Exception):
        px.set_observer(0, body=63)
    with pytest.raises(Exception):
        px.set_points(0, (0, 0, 0))                       # no such observer
    with pytest.raises(Exception):
        px.remove_observer(0)
    px.update()                                           # no live observer: nothing is launched, nothing counts
    px.set_observer(0, pos=(0, 0, 0))
    px.update()
    assert ps.records(px.drain_events()[0])[0][5] == 0
    px.close(); w.close()


def test_updates_without_waits_give_the_same_events():
    """update() enqueues and returns: a run that never reads anything back between the calls ends with the same bytes as one that reads after every update."""
    out = []
    for read_back in (True, False):
        rig = ps.Rig(257, 2, rider=False)
        for u in range(12):
            rig.movers.update(ps.DT)
            rig.w.step(ps.DT)
            for k in range(2):
                rig.px.set_points(k, ps.walk(k, u))
            rig.px.update()
            if read_back:
                rig.px.states(0, 257); rig.px.observers()
        ev, dropped = rig.px.drain_events()
        out.append((ev.tobytes(), dropped, rig.px.states(0, 257).tobytes(), rig.px.observers().tobytes()))
        assert len(ev) > 20
        rig.close()
    assert out[0] == out[1]


def test_caller_program_agrees_with_its_host_loop(tmp_path):
    from test_facade_gpu import build_facade_exe
    exe = build_facade_exe(tmp_path, "proximity_batch.cpp")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    out = json.loads(r.stdout.strip().splitlines()[-1])
    print(out)
    assert out["mismatches"] == 0 and out["events"] == out["expected"] > 20
    assert min(out["near"], out["away"], out["exited"], out["entered"]) > 0
    assert out["replay_equal"] and out["replay_events"] > 3 and out["dropped"] == 0
    assert out["touches"] == 2 and out["in_proximity_last"]
