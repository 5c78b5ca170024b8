"""Body events reach the host through the window the step's last launch fills in host-mapped memory (the counters and the first ids of each list);
a list longer than the window is fetched with a copy of its own, as every list was before.  SGP_EVENT_WINDOW=0 (read when a world is created)
switches the window off, which is the earlier path: the same scene must deliver the same events, step by step, with the window off, at its
default size and at a size of four ids."""
import os

import numpy as np
import pytest

from substrata_amd import abi, scenes
from substrata_amd.lib import World
from helpers import DT, add_ground, dyn

pytestmark = pytest.mark.gpu

WINDOW = 256      # SGP_EVENT_WINDOW of csrc/sgp_kernels.h


def world_with_window(window, **kw):
    old = os.environ.get("SGP_EVENT_WINDOW")
    try:
        if window is None:
            os.environ.pop("SGP_EVENT_WINDOW", None)
        else:
            os.environ["SGP_EVENT_WINDOW"] = str(window)
        return World(**kw)
    finally:
        if old is None:
            os.environ.pop("SGP_EVENT_WINDOW", None)
        else:
            os.environ["SGP_EVENT_WINDOW"] = old


def brick_wall(w, width=40, height=16):
    """one island: every brick rests on two of the row below and touches its neighbours"""
    add_ground(w)
    # (odd rows are shifted by half a brick and hold one brick fewer: no brick hangs over the end of the row below)
    xz = [(i + 0.5 * (r % 2), 0.25 + 0.5 * r) for r in range(height) for i in range(width - r % 2)]
    d = scenes.dynamic_bodies(len(xz))
    d["shape"][:, :3] = (0.5, 0.3, 0.25)
    d["pos"][:, 0] = [x for x, z in xz]; d["pos"][:, 1] = 0.0; d["pos"][:, 2] = [z for x, z in xz]
    d["userdata"] = 1000 + np.arange(len(xz))
    return [int(x) for x in w.add_batch(d)]


def step_events(w):
    w.step(DT)
    st = w.stats()
    ev = tuple(w.drain_events(k) for k in (abi.EVENT_ACTIVATED, abi.EVENT_DEACTIVATED, abi.EVENT_ENTERED_WATER))
    assert (st.num_activated, st.num_deactivated) == (len(ev[0]), len(ev[1]))
    return tuple((tuple(int(x) for x in e["id"]), tuple(int(x) for x in e["userdata"])) for e in ev)


def test_same_events_with_and_without_the_window():
    ws = [world_with_window(win, max_bodies=1024) for win in (0, None, 4)]
    ids = [brick_wall(w) for w in ws]
    assert ids[0] == ids[1] == ids[2]
    n = len(ids[0])
    most = [0, 0, 0]
    in_window = 0
    log = []

    def run(steps, what):
        nonlocal in_window
        for s in range(steps):
            ev = [step_events(w) for w in ws]
            assert ev[0] == ev[1] == ev[2], (what, s, [[len(k[0]) for k in e] for e in ev])
            for k in range(3):
                most[k] = max(most[k], len(ev[0][k][0]))
                in_window += 0 < len(ev[0][k][0]) <= WINDOW
            log.append(tuple(len(k[0]) for k in ev[0]))

    run(3, "creation")             # (every brick is activated by its creation)
    assert most[0] == n > WINDOW
    run(500, "falling asleep")
    assert most[1] > WINDOW, ("the wall did not fall asleep as one island", most)
    assert not any(s["active"] for s in ws[1].get_state(ids[1]))
    # a mass wake-up: a heavy ball lands on the sleeping wall
    most[0] = 0
    for w in ws:
        dyn(w, abi.SHAPE_SPHERE, (0.5,), pos=(20.0, 0.0, 11.0), mass=400.0, lin_vel=(0, 0, -8.0))
    run(120, "wake-up")
    assert most[0] > WINDOW, ("the ball did not wake the wall at once", most)
    # water: bodies enter it a few at a time
    for w in ws:
        w.set_water(True, 1.1)
    run(200, "water")
    assert most[2] > 0
    assert in_window > 0           # some lists came through the window, some (above) through the copy
    for w in ws:
        w.close()


def test_step_n_delivers_the_union_of_its_steps():
    wa, wb = world_with_window(None, max_bodies=1024), world_with_window(None, max_bodies=1024)
    for w in (wa, wb):
        brick_wall(w, 20, 8)
        for k in range(12):       # loose boxes that come to rest at different times
            dyn(w, pos=(2.0 * k, 3.0, 0.5 + 0.4 * k), lin_vel=(0.3 * k, 0, 0))
    n_bodies = wa.num_bodies() - 1
    seen = 0
    for chunk in range(60):
        k = 1 + chunk % 8
        for _ in range(k):
            wa.step(DT)
        wb.step_n(DT, k)
        for kind in range(3):
            ea, eb = wa.drain_events(kind), wb.drain_events(kind)
            assert np.array_equal(ea["id"], eb["id"]) and np.array_equal(ea["userdata"], eb["userdata"]), (chunk, kind, len(ea), len(eb))
            seen += len(ea)
    assert seen > n_bodies        # every body was activated at its creation; more than that happened
    wa.close(); wb.close()


def test_an_edit_that_activates_a_body_between_steps_is_reported_once():
    for window in (None, 0):
        w = world_with_window(window, max_bodies=64)
        add_ground(w)
        ids = [dyn(w, pos=(3.0 * k, 0, 0.5)) for k in range(6)]
        for s in range(300):
            w.step(DT)
        assert not any(s["active"] for s in w.get_state(ids))
        for k in range(3):
            w.drain_events(k)
        # between two steps, events pulled by the step before
        w.activate(ids[2])
        w.step(DT)
        assert w.stats().num_activated == 1
        w.step(DT); w.step(DT)
        assert [int(x) for x in w.drain_events(abi.EVENT_ACTIVATED)["id"]] == [ids[2]]
        # read before the next step, then stepped: still once
        w.activate(ids[4])
        assert w.event_counts()[abi.EVENT_ACTIVATED] == 1
        w.step(DT); w.step(DT)
        assert [int(x) for x in w.drain_events(abi.EVENT_ACTIVATED)["id"]] == [ids[4]]
        # two edits with a read between them and no step
        w.activate(ids[0])
        assert w.event_counts()[abi.EVENT_ACTIVATED] == 1
        w.activate(ids[1])
        assert w.event_counts()[abi.EVENT_ACTIVATED] == 2
        w.step_n(DT, 3)
        assert sorted(int(x) for x in w.drain_events(abi.EVENT_ACTIVATED)["id"]) == sorted([ids[0], ids[1]])
        assert len(w.drain_events(abi.EVENT_DEACTIVATED)) == 0
        w.close()
