"""sgp_proximity_checkpoint / _rollback (SGP_BATCH_PROXIMITY): a batch rolled back with its world -- and with the movers that carry some of its bodies --
continues with the identical event stream: the near masks after every update and the drained bytes, pending undrained events included, are the same the
second time.  Between capture and rollback the scene is edited on every table a checkpoint holds: zones, objects, observers, and a watched body is removed
(the relink rule brings its object back with it)."""
import numpy as np
import pytest

from substrata_amd import abi
import proximity_scenes as ps

pytestmark = pytest.mark.gpu

N, OBSERVERS = 257, 3


def run(rig, first, count, edits):
    """`count` frames from update `first` on, with the edits of `edits` (frame -> callable); returns what a caller can see: masks and observers per frame."""
    seen = []
    for u in range(first, first + count):
        if u in edits:
            seen.append(repr(edits[u]()).encode())
        rig.movers.update(ps.DT)
        rig.w.step(ps.DT)
        for k in (0, 2):                                  # (observer 1 rides a kinematic box)
            if k not in rig.absent:
                rig.px.set_points(k, ps.walk(k, u))
        rig.px.update()
        seen.append(rig.px.states(0, rig.capacity).tobytes())
        seen.append(rig.px.observers().tobytes())
    return seen


def make_edits(rig, spare_body):
    w, px = rig.w, rig.px
    rig.absent = set()                                    # observers that are away between their removal and their return

    def observer_leaves():
        px.remove_observer(2); rig.absent.add(2)

    def observer_returns():
        px.set_observer(2, pos=ps.walk(2, 23)); rig.absent.discard(2)

    return {
        14: lambda: px.remove_zone(rig.zone_slot[0]),
        16: lambda: px.add_zone((0.0, 0.0, -1.0), (50.0, 50.0, 8.0), 5),                    # the freed slot, a new generation
        17: lambda: (px.remove(3), [int(i) for i in px.add([spare_body], 20.0, tags=[77])]),   # the freed object slot comes back first
        19: observer_leaves,
        21: lambda: w.remove(int(rig.bodies[9])),                                            # a watched body goes: BODY_GONE from the next update on
        23: observer_returns,                                                                # a new observer: everything in range fires again
        25: lambda: px.set_flags(12, 0),
    }


def test_rollback_continues_with_the_identical_event_stream():
    rig = ps.Rig(N, OBSERVERS, radius=20.0)
    w, px = rig.w, rig.px
    spare_body = int(w.add_batch(ps.scenes._blank(1))[0])
    for u in range(10):
        rig.frame()
        if u == 6:
            rig.check_drain()
    pending = rig.sim.raised
    assert pending > 0                                    # events of updates 7 .. 9 are still undrained at the capture
    wcp, pcp, mcp = w.checkpoint(), px.checkpoint(), rig.movers.checkpoint()
    info = pcp.info()
    assert info["kind"] == abi.BATCH_PROXIMITY and info["capacity"] == rig.capacity and info["high_slot"] == N and info["num_alive"] == N
    assert info["world_steps_taken"] == wcp.info()["steps_taken"] and info["device_bytes"] > 0 and info["host_bytes"] > 0
    edits = make_edits(rig, spare_body)
    first = run(rig, 10, 20, edits)
    ev1, dropped1 = px.drain_events()
    assert int(px.states(9, 1)[0]["status"]) == abi.PROX_ST_BODY_GONE
    # the batch first, while the removed body is still missing; then the movers and the world
    px.rollback(pcp); rig.movers.rollback(mcp); w.rollback(wcp)
    second = run(rig, 10, 20, edits)
    ev2, dropped2 = px.drain_events()
    assert len(first) == len(second)
    for i, (a, b) in enumerate(zip(first, second)):
        assert a == b, i
    assert ev1.tobytes() == ev2.tobytes() and dropped1 == dropped2 == 0
    assert len(ev1) > pending + 20 and int(ev1["update_index"][0]) < 10 and 23 <= int(ev1["update_index"].max()) <= 29      # the pending ones came back, then the 20 updates'
    assert {abi.PROX_EV["NEAR"], abi.PROX_EV["AWAY"], abi.PROX_EV["ENTERED"]} <= {int(k) for k in ev1["kind"]}
    # overwriting a checkpoint in place, and rolling back to it again
    px.checkpoint(pcp); rig.movers.checkpoint(mcp); w.checkpoint(wcp)
    third = run(rig, 30, 5, {})
    ev3 = px.drain_events()[0]
    w.rollback(wcp); rig.movers.rollback(mcp); px.rollback(pcp)
    assert run(rig, 30, 5, {}) == third and px.drain_events()[0].tobytes() == ev3.tobytes()
    for cp in (wcp, pcp, mcp):
        cp.close()
    rig.close()


def test_relink_after_rollback_and_refusals():
    rig = ps.Rig(40, 2, radius=20.0)
    other = ps.Rig(40, 2, radius=20.0)
    w, px = rig.w, rig.px
    for _ in range(3):
        rig.frame(); other.frame()
    rig.check_drain()
    wcp, pcp, mcp = w.checkpoint(), px.checkpoint(), rig.movers.checkpoint()
    sim_mask = rig.sim.mask.copy()
    # the rider's body and a watched body are removed after the capture
    w.remove(rig.rider[0]); w.remove(int(rig.bodies[8]))
    w.step(ps.DT)
    px.update()
    assert int(px.states(8, 1)[0]["status"]) == abi.PROX_ST_BODY_GONE and int(px.observers(1, 1)[0]["status"]) == abi.PROX_OBS_ST_BODY_GONE
    w.rollback(wcp); px.rollback(pcp); rig.movers.rollback(mcp)
    assert np.array_equal(px.states(0, rig.capacity)["near_mask"], sim_mask)
    for _ in range(3):
        rig.frame()                                       # masks equal the restatement's, which never saw the removal
    rig.check_drain()
    assert int(px.states(8, 1)[0]["status"]) == 0 and int(px.observers(1, 1)[0]["status"]) == 0 and int(px.observers(1, 1)[0]["update_index"]) == 6
    # a foreign batch's checkpoint, and another kind's, are refused with the batch untouched
    before = (px.states(0, rig.capacity).tobytes(), px.observers().tobytes())
    ocp = other.px.checkpoint()
    for foreign in (ocp, mcp):
        with pytest.raises(Exception):
            px.rollback(foreign)
        with pytest.raises(Exception):
            px.checkpoint(foreign)
    assert (px.states(0, rig.capacity).tobytes(), px.observers().tobytes()) == before
    # a checkpoint outlives its batch and its world
    other.close()
    assert ocp.info()["kind"] == abi.BATCH_PROXIMITY
    for cp in (wcp, pcp, mcp, ocp):
        cp.close()
    rig.close()
