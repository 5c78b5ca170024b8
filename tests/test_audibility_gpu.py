"""The batched audio sources (sgp_audibility_*) against the numpy restatement of docs/CONTRACT.md 4m (tests/audibility_reference.py).  The restatement is fed
from two places and never from what the audibility kernels wrote: the sources' positions come from the bodies' reported poses and shapes
(tests/audibility_scenes.py), the occlusion answers are sgp_raycast's to the rays the restatement built itself.  After every update the two masks, every
pair's dist bits and factor bits are equal; at every drain the events are, in their order."""
import json
import subprocess

import numpy as np
import pytest

from substrata_amd import abi
import audibility_reference as ar
import audibility_scenes as sc

pytestmark = pytest.mark.gpu

N_UPDATES = 40


def kernel_constants():
    """AUD_WG and AUD_SCAN_PASS from sgp_kernels.h: sources per workgroup of the per-source launches, counts per pass of the single-workgroup scans."""
    import os
    import re
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "substrata_amd", "csrc", "sgp_kernels.h")).read()
    val = {m.group(1): m.group(2) for m in re.finditer(r"#define (AUD_WG|AUD_SCAN_WG|AUD_SCAN_PASS)\s+(\w+)", src)}
    wg, scan_wg = int(val["AUD_WG"]), int(val["AUD_SCAN_WG"])
    return wg, scan_wg if val["AUD_SCAN_PASS"] == "AUD_SCAN_WG" else int(val["AUD_SCAN_PASS"])


AUD_WG, AUD_SCAN_PASS = kernel_constants()
SECOND_PASS = AUD_WG * AUD_SCAN_PASS + 1      # the first size whose workgroup counts need a second pass of the scans
SIZES = [(n, L) for n in (1, 63, 64, 65, 255, 256, 257, SECOND_PASS) for L in (1, 2, 32)]


def run_sequence(rig, n_updates=N_UPDATES, drain_every=5):
    """The scripted sequence: irregular times, listener 0 into a muting zone and out again while the ramps are on their way, a body removed on the way and
    its source's slot reused.  Returns every event of the run."""
    t = sc.times(n_updates)
    pending, all_events = [], []
    removed = None
    for u in range(n_updates):
        if u == 12:
            rig.set_listener_zone(0, 40, True)
        if u == 15:
            rig.set_listener_zone(0, abi.INVALID_ID, False)
        if u == 25:
            rig.set_listener_zone(0, 20, True)
        if u == 33:
            rig.set_listener_zone(0, 20, False)
        if u == 18 and rig.n > 1:      # a body goes: its source is frozen and flagged ...
            removed = 1
            rig.w.remove(int(rig.body[removed]))
            rig.body_there[removed] = False
        if u == 22 and removed is not None:      # ... then removed, and its slot taken by a POINT source next to the walk
            rig.ab.remove(removed)
            p = np.array((20.0, 5.0, 1.5), sc.F32)
            new = rig.ab.add_points([p], volume=0.3, zone_key=40, flags=sc.ALL_WANTS, tags=[777])
            assert int(new[0]) == removed
            rig.model.reset_source(removed)
            rig.body[removed] = abi.INVALID_ID; rig.point[removed] = p; rig.volume[removed] = 0.3; rig.key[removed] = 40
            rig.flags[removed] = sc.ALL_WANTS; rig.tags[removed] = 777
        pending += rig.frame(float(t[u]))
        if u == 19 and removed is not None:
            assert rig.ab.states(removed, 1)[0]["status"] == abi.AUD_ST_BODY_GONE
        if (u + 1) % drain_every == 0 or u == n_updates - 1:
            all_events += rig.check_drain(pending)
            pending = []
    return all_events


@pytest.mark.parametrize("n, n_listeners", SIZES)
def test_masks_distances_factors_and_events_equal_the_restatement(n, n_listeners):
    rig = sc.Rig(n, n_listeners)
    try:
        events = run_sequence(rig)
        st = rig.model.stats
        kinds = {e[0] for e in events}
        print(f"n={n} L={n_listeners}: {len(events)} events, kinds {sorted(kinds)}, {st}")
        assert rig.model.update_index == N_UPDATES
        assert (rig.ab.listeners()["update_index"][:n_listeners] == N_UPDATES).all()
        if n >= 63:      # coverage: all five event kinds, a pair nearer than 1 m, a trace clamped at 60 m, a ramp reversed in mid-flight
            assert kinds == {ar.EV_IN_RANGE, ar.EV_OUT_OF_RANGE, ar.EV_OCCLUDED, ar.EV_UNOCCLUDED, ar.EV_VOLUME}, kinds
            assert st["rays"] > 100 and st["dist_below_1"] >= 1 and st["clamped_60"] >= 1 and st["reversed"] >= 1, st
        if n == SECOND_PASS:      # events and rays from workgroups of both passes of the scans
            wgs = {e[1] // AUD_WG for e in events}
            assert min(wgs) < AUD_SCAN_PASS <= max(wgs), (min(wgs), max(wgs))
    finally:
        rig.close()


def test_an_update_with_nothing_live_launches_nothing_and_does_not_count():
    rig = sc.Rig(5, 1)
    try:
        rig.ab.remove_listener(0)
        rig.ab.update(1.0)
        ev, dropped = rig.ab.drain_events()
        assert len(ev) == 0 and dropped == 0
        rig.ab.set_listener(0, pos=sc.walk(0, 0))
        rig.lst_live[0] = True
        ev = rig.frame(2.0)
        assert all(e[5] == 0 for e in ev) and len(ev) > 0      # the first update that ran stamps index 0
        rig.check_drain(ev)
        assert rig.ab.listeners()["update_index"][0] == 1
    finally:
        rig.close()


def test_a_removed_listener_takes_its_pairs_along_and_a_new_one_starts_fresh():
    rig = sc.Rig(65, 2)
    try:
        t = sc.times(12)
        pending = []
        for u in range(6):
            pending += rig.frame(float(t[u]))
        rig.check_drain(pending)
        assert rig.model.in_range[:, 0].any()
        rig.ab.remove_listener(0)
        rig.lst_live[0] = False
        rig.model.reset_listener(0)
        st = rig.ab.states(0, rig.capacity)
        assert not (st["in_range_mask"] & 1).any()      # at once in what the getters report
        rig.ab.set_listener(0, pos=sc.walk(0, rig.u))
        rig.lst_live[0] = True; rig.lst_key[0] = abi.INVALID_ID; rig.lst_mute[0] = False
        pending = []
        for u in range(6, 12):
            pending += rig.frame(float(t[u]))
        got = rig.check_drain(pending)
        assert any(e[0] == ar.EV_IN_RANGE and e[2] == 0 for e in got)      # in range again: reported again for the new listener
    finally:
        rig.close()


def test_refusals_need_a_world():
    w = sc.new_world(max_bodies=16)
    try:
        from substrata_amd.world import SgpError
        for caps in ((0, 1, 1), ((1 << 20) + 1, 1, 1), (4, 0, 1), (4, 33, 1), (1 << 20, 5, 1), (4, 1, 0)):
            with pytest.raises(SgpError):
                w.audibility(*caps)
        ab = w.audibility(4, 2, 16)
        with pytest.raises(SgpError):
            ab.set_listener(2, pos=(0, 0, 0))      # beyond the listener capacity
        with pytest.raises(SgpError):
            ab.add_bodies([7])                      # not a live body
        with pytest.raises(SgpError):
            ab.set_muting_keys([5, 3])
        with pytest.raises(SgpError):
            ab.update(float("nan"))
        ab.set_muting_keys([3, 5])
        ab.set_transition(0.5)
        ab.close()
    finally:
        w.close()


def test_listener_zones_from_an_attached_proximity_batch_equal_the_keys_set_by_hand():
    """Two batches over one world and one set of sources: A takes its listeners' zone keys on the device from the attached proximity batch's observers and
    looks them up in the muting keys; B gets the same keys from the host, which reads the observers back after the proximity update.  Masks, factors and
    events are equal."""
    n, L = 65, 2
    rig = sc.Rig(n, L)
    px = rig.w.proximity(8, 8, 256)
    other = rig.w.audibility(rig.capacity, L, 1 << 16)
    try:
        # zones over the walk; 40 mutes outside audio
        px.add_zone((-10.0, -5.0, -1.0), (20.0, 30.0, 8.0), 40)
        px.add_zone((10.0, -5.0, -1.0), (40.0, 30.0, 8.0), 20)
        muting = [40]
        px.add([int(rig.body[1])])      # (a proximity batch without an object launches nothing)
        desc = np.zeros(n, dtype=abi.audibility_source_dtype)
        desc["kind"] = np.where(rig.is_body, abi.AUD_SRC_BODY, abi.AUD_SRC_POINT); desc["body"] = np.where(rig.is_body, rig.body[:n], 0)
        desc["pos"] = rig.point[:n]; desc["volume"] = rig.volume[:n]; desc["zone_key"] = rig.key[:n]; desc["flags"] = rig.flags[:n]; desc["tag"] = rig.tags[:n]
        assert np.array_equal(other.add(desc), np.arange(n))
        for k in range(L):
            px.set_observer(k, pos=sc.walk(k, 0))
            other.set_listener(k, pos=sc.walk(k, 0))
        rig.ab.set_listener(1, pos=sc.walk(1, 0)); rig.rider = None; rig.lst_ignore[1] = abi.INVALID_ID      # (both listeners walk in this test)
        other.attach_proximity(px)
        other.set_muting_keys(muting)
        t = sc.times(N_UPDATES)
        seen_keys, volume_events = set(), 0
        for u in range(N_UPDATES):
            for k in range(L):
                px.set_points(k, sc.walk(k, u))
                other.set_listener_points(k, sc.walk(k, u))
            if rig.movers is not None:
                rig.movers.update(sc.DT)
            rig.w.step(sc.DT)
            px.update()
            other.update(float(t[u]))                      # A: the keys stay on the device
            keys = px.observers(0, L)["zone_key"]          # B: read back, set by hand
            for k in range(L):
                rig.set_listener_zone(k, int(keys[k]), int(keys[k]) in muting)
                rig.ab.set_listener_points(k, sc.walk(k, u))
                seen_keys.add(int(keys[k]))
            rig.ab.update(float(t[u]))
            sa, sb = other.states(0, n), rig.ab.states(0, n)
            pa, pb = other.pair_states(0, n), rig.ab.pair_states(0, n)
            assert np.array_equal(sa["in_range_mask"], sb["in_range_mask"]) and np.array_equal(sa["occluded_mask"], sb["occluded_mask"]), u
            assert np.array_equal(pa.view(np.uint32), pb.view(np.uint32)), u
            la, lb = other.listeners(), rig.ab.listeners()
            assert np.array_equal(la["zone_key"], lb["zone_key"]) and np.array_equal(la["mute_outside"], lb["mute_outside"]), u
            ea, eb = other.drain_events(), rig.ab.drain_events()
            assert sc.records(ea[0]) == sc.records(eb[0]) and ea[1] == eb[1] == 0, u
            volume_events += sum(1 for e in ea[0] if e["kind"] == ar.EV_VOLUME)
        assert {40, 20, abi.INVALID_ID} <= seen_keys and volume_events > 10
        other.attach_proximity(None)
    finally:
        other.close(); px.close(); rig.close()


def test_caller_program_runs(tmp_path):
    from test_facade_gpu import build_facade_exe
    exe = build_facade_exe(tmp_path, "audibility_batch.cpp")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    out = json.loads(r.stdout.strip().splitlines()[-1])
    print(out)
    assert out["mismatches"] == 0 and out["occlusion_callbacks"] > 0 and out["volume_callbacks"] > 0
    assert out["replay_equal"] and out["occluded_behind_wall"] and not out["occluded_in_the_open"]
