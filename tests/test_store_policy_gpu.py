"""Every global store of a body record or an impulse in the solver launches goes through store_rec, whose policy -- plain, or written through the L2 --
the launch picks (sgp_dev_common.h; docs/KERNELS.md, "Write-through stores"; the product writes through in the colour launches and in the pass of the
component launch, its plain twin is built with -DSGP_SOLVER_STORES=0, and both passed these cases: profiles/write_through_stores.md).  A store policy
changes no value -- so every bit must stay where it was, whichever
build the library is: a small mixed pile (a 6 x 6 x 4 lattice of boxes, spheres and
capsules dropped on the ground, with a static sensor box inside it: 146 bodies, manifolds of 0, 1, 2, 3 and 4 points) is stepped against the
oracle and compared bit for bit, poses and velocities, at every one of 90 steps -- on every row layout, with and without the components' launch,
replayed from the graph and launched eagerly, with an even and an odd number of steps in front of the compared window (the window then starts on
the other constraint buffer), and across a checkpoint and rollback.  What would show here: a record stored narrower or wider than it is, a store
that went to the wrong array's descriptor or past a 32-bit offset, a launch that read a line another launch had not yet written through.
The oracle's run is made once and shared; nothing writes to it."""
import numpy as np
import pytest

from substrata_amd import scenes
from helpers import DT
import parity
from test_components_gpu import pile_scene
from test_solver_buffers_gpu import LAYOUT, gpu_world

WINDOW = 90          # compared steps
MAX_BEFORE = 1       # steps in front of the window: 0 (even) or 1 (odd)


def sensor_pile():
    """pile_scene's column four layers high (144 bodies on the ground) with a static sensor box where the second layer comes to rest: its pairs
    stay in the contact list as manifolds without points."""
    s = scenes.ground()
    s["shape"][0, :3] = 0.3
    s["pos"][0] = (0.36, 0.36, 0.9)
    s["is_sensor"] = 1
    return np.concatenate([pile_scene(6, 4), s])


@pytest.fixture(scope="module")
def reference(oracle):
    descs = sensor_pile()
    w = oracle.OracleWorld(max_bodies=1024)
    w.add_batch(descs)
    steps = []
    for _ in range(MAX_BEFORE + WINDOW):
        w.step(DT)
        st = w.stats()
        steps.append({"states": w.read_states(0, len(descs)).copy(), "counts": (st.num_manifolds, st.num_contact_points, st.num_colours),
                      "np": np.bincount(w.dump_constraints()["np"], minlength=5)})
    w.close()
    for s in steps:
        s["states"].flags.writeable = False
    return descs, steps


def test_pile_holds_every_manifold_size_by_step_30(reference):
    """(no GPU) From the oracle's contact counts: at step 30 and at the end of either window the pile holds manifolds of no, one, two, three and
    four points at once, so a case cannot pass on a pile that lost its four-point manifolds (or its sensor pairs)."""
    descs, steps = reference
    assert len(descs) == 6 * 6 * 4 + 2
    for s in (30, WINDOW, MAX_BEFORE + WINDOW):
        hist = steps[s - 1]["np"]
        print(s, hist, steps[s - 1]["counts"])
        assert len(hist) == 5 and all(hist[k] > 0 for k in range(5)), (s, hist)
        assert steps[s - 1]["counts"][1] == int(np.dot(hist, np.arange(5))), (s, steps[s - 1]["counts"], hist)
    assert steps[29]["counts"][2] >= 4, steps[29]["counts"]          # several colours: several colour launches per pass


def step_and_check(w, reference, first, last, tag, seen):
    descs, steps = reference
    for s in range(first, last + 1):
        w.step(DT)
        ref = steps[s - 1]
        st = w.stats()
        assert (st.num_manifolds, st.num_contact_points, st.num_colours) == ref["counts"], (tag, s)
        d = parity.state_diff(w.read_states(0, len(descs)), ref["states"])
        assert d["bit_exact"] and d["active_mismatch"] == 0, (tag, s, d)
        seen["colours"] = max(seen["colours"], st.num_colours)
        seen["by_component"] = max(seen["by_component"], st.num_component_constraints)


def check_plan(seen, budget):
    """several colour launches per pass, and the component launch (whose pass writes through) ran exactly where the case says it does"""
    assert seen["colours"] >= 4, seen
    if budget == "0":
        assert seen["by_component"] == 0, seen
    else:
        assert seen["by_component"] > 0, seen


def run_case(reference, layout, budget, no_graph, before):
    env = dict(LAYOUT[layout], SGP_NO_GRAPH=no_graph)
    if budget is not None:
        env["SGP_HC_BUDGET"] = budget
    w = gpu_world(env)
    w.add_batch(reference[0])
    seen = {"colours": 0, "by_component": 0}
    for _ in range(before):
        w.step(DT)
    step_and_check(w, reference, before + 1, before + WINDOW, (layout, budget, no_graph, before), seen)
    check_plan(seen, budget)
    assert w.step_profiled(DT).row_layout == layout          # (one more step, not compared: the layout the switches ask for is the one that ran)
    hist = np.bincount(w.dump_constraints()["np"], minlength=5)
    assert all(hist[k] > 0 for k in range(5)), hist
    w.close()
    return seen


@pytest.mark.gpu
@pytest.mark.parametrize("no_graph", ["0", "1"])
@pytest.mark.parametrize("budget", ["0", None])
@pytest.mark.parametrize("layout", [0, 1, 2])
def test_every_step_is_the_oracles(reference, layout, budget, no_graph):
    run_case(reference, layout, budget, no_graph, 0)


@pytest.mark.gpu
@pytest.mark.parametrize("layout", [0, 1, 2])
def test_window_on_the_other_buffer(reference, layout):
    """one step in front of the window: every compared step reads and writes the constraint buffer the even case used for its neighbour"""
    run_case(reference, layout, None, "0", 1)


@pytest.mark.gpu
def test_across_a_rollback(reference):
    """Checkpoint at step 20, on to 45, back, and on to 90: the replayed steps must land on the oracle's bits again (the layout the benchmark's world solves on)."""
    w = gpu_world(LAYOUT[2])
    w.add_batch(reference[0])
    seen = {"colours": 0, "by_component": 0}
    step_and_check(w, reference, 1, 20, "before", seen)
    cp = w.checkpoint()
    step_and_check(w, reference, 21, 45, "first pass", seen)
    w.rollback(cp)
    step_and_check(w, reference, 21, WINDOW, "after rollback", seen)
    check_plan(seen, None)
    cp.close()
    w.close()
