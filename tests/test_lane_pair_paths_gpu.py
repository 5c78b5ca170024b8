"""The lane-pair solver (sgp_dev_solve.h) corrects both bodies of a constraint on ONE path: lane `side` applies sl = side ? lambda : -lambda
(half_apply, pos_half_solve_rec), and the perpendicular of the normal selects its operand before the one root and two divisions
(v3_normalized_perpendicular).  In the other test scenes the only body that cannot move is the ground, which is always body `a` (id 0): the lane of
side 1 always moves there.  This scene is the 504-body pile of test_components_gpu plus a solid static WALL AS THE LAST BODY, so that the lane of
side 1 is the one that stays where it is in some constraints and the lane of side 0 in others, with normals of both perpendicular forms, ties
included.  Every one of 41 steps is compared bit for bit against the oracle, on row layouts 2 (the benchmark's) and 0, with the components' launch
and without it.  The oracle's run is made once and shared."""
import os

import numpy as np
import pytest

from substrata_amd import scenes
from helpers import DT
import parity
from test_components_gpu import pile_scene

STEPS = 41
ENV = ("SGP_NO_SMALL_WORLD", "SGP_TAIL_THRESHOLD", "SGP_HC_BUDGET", "SGP_HC_MIN_COLOURS", "SGP_NO_GRAPH", "SGP_ROWS_IN_SMALL_WORLDS",
       "SGP_ROWS_MODE_DEFAULT", "SGP_ROWS_MODE2_MIN", "SGP_COMPACT_ROWS_MIN", "SGP_ROWS_MODE")
BASE = {"SGP_NO_SMALL_WORLD": "1", "SGP_TAIL_THRESHOLD": "24"}      # the switches of test_solver_buffers_gpu: the colour launches do the work
LAYOUT = {0: {"SGP_ROWS_IN_SMALL_WORLDS": "1", "SGP_ROWS_MODE_DEFAULT": "0"},
          2: {"SGP_ROWS_IN_SMALL_WORLDS": "1", "SGP_COMPACT_ROWS_MIN": "0", "SGP_ROWS_MODE": "2"}}


def walled_pile():
    """pile_scene() (ground = body 0, 504 dynamic bodies) and a static wall, the LAST body, whose face touches the pile's +x side over its whole height"""
    wall = scenes.ground()
    wall["shape"][0, :3] = (0.1, 2.6, 6.0)
    wall["pos"][0] = (2.3, 0.0, 6.0)
    return np.concatenate([pile_scene(), wall])


@pytest.fixture(scope="module")
def reference(oracle):
    """The oracle's 41 steps, made once and shared (nothing writes to it): per step the body states, the counts and the constraints' ids, point counts,
    colours and normals."""
    descs = walled_pile()
    w = oracle.OracleWorld(max_bodies=1024)
    w.add_batch(descs)
    steps = []
    for _ in range(STEPS):
        w.step(DT)
        st = w.stats()
        cons = w.dump_constraints()
        steps.append({"states": w.read_states(0, len(descs)).copy(), "counts": (st.num_manifolds, st.num_contact_points, st.num_colours),
                      "dropped": (st.pairs_dropped, st.manifolds_dropped),
                      "a": cons["a"].copy(), "b": cons["b"].copy(), "np": cons["np"].copy(), "n": cons["n"].copy()})
    w.close()
    for s in steps:
        s["states"].flags.writeable = False
    return descs, steps


def test_scene_puts_a_static_body_on_either_side_and_splits_the_normals(reference):
    """(no GPU) What the GPU cases need of the scene, at every step from 10 to 41: constraints whose body b cannot move (the wall) and constraints whose
    body a cannot (the ground), normals of both forms of the perpendicular, every manifold size, many colours, nothing dropped."""
    descs, steps = reference
    wall = len(descs) - 1
    assert wall == 6 * 6 * 14 + 1
    ties = 0
    for k in range(10, STEPS + 1):
        s = steps[k - 1]
        on_wall = s["np"][s["b"] == wall]
        assert len(on_wall) >= 30, (k, len(on_wall))                      # 37 was the fewest seen
        assert (on_wall == 1).any() and (on_wall == 4).any(), (k, np.bincount(on_wall, minlength=5))
        assert not (s["a"] == wall).any()                                  # the last id is never body a: the static lane is the lane of side 1 there
        assert int((s["a"] == 0).sum()) >= 10, k                           # 12 seen
        nx, ny = np.abs(s["n"][:, 0]), np.abs(s["n"][:, 1])
        assert int((nx > ny).sum()) >= 300 and int((nx <= ny).sum()) >= 300, (k, int((nx > ny).sum()), int((nx <= ny).sum()))      # 408 and 491 seen
        ties += int((nx == ny).sum())
        sizes = np.bincount(s["np"], minlength=5)
        assert all(sizes[1:5] > 0), (k, sizes)
        assert s["counts"][2] >= 10, (k, s["counts"])                      # 12 colours seen
        assert s["dropped"] == (0, 0), (k, s["dropped"])
    assert ties >= 1
    assert all(s["dropped"] == (0, 0) for s in steps)


def gpu_world(env):
    from substrata_amd.lib import World
    old = {k: os.environ.get(k) for k in ENV}
    try:
        for k in ENV:
            os.environ.pop(k, None)
        os.environ.update(BASE)
        os.environ.update(env)
        return World(max_bodies=1024)      # (the product reads the switches when the world is created)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@pytest.mark.gpu
@pytest.mark.parametrize("budget", ["0", None])
@pytest.mark.parametrize("layout", [2, 0])
def test_every_step_matches_oracle_with_a_static_body_on_either_side(reference, layout, budget):
    descs, steps = reference
    env = dict(LAYOUT[layout])
    if budget is not None:
        env["SGP_HC_BUDGET"] = budget
    w = gpu_world(env)
    w.add_batch(descs)
    by_component = 0
    for s in range(1, STEPS + 1):
        w.step(DT)
        ref = steps[s - 1]
        st = w.stats()
        assert (st.num_manifolds, st.num_contact_points, st.num_colours) == ref["counts"], (layout, budget, s)
        assert (st.pairs_dropped, st.manifolds_dropped) == (0, 0), (layout, budget, s)
        d = parity.state_diff(w.read_states(0, len(descs)), ref["states"])
        assert d["bit_exact"] and d["active_mismatch"] == 0, (layout, budget, s, d)
        by_component = max(by_component, st.num_component_constraints)
    if budget == "0":
        assert by_component == 0
    else:
        assert by_component > 0          # the components' launch ran where it is planned
    assert w.step_profiled(DT).row_layout == layout          # (one more step, not compared: the layout the switches ask for is the one that ran)
    w.close()
