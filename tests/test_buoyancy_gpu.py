"""k_buoyancy (sgp_k_sweep.hip) against the float64 reference of tests/buoyancy_reference.py, on the case table of tests/buoyancy_cases.py: submerged
volume, the underwater flag, the change of the linear and of the angular velocity, the entered-water events.  The bounds and what was measured are in
tests/test_buoyancy_reference.py, which runs the same table on the CPU oracle; the GPU equals the oracle bit for bit (test_parity_gpu.py::test_buoyancy)."""
import numpy as np
import pytest

import buoyancy_cases as bc

pytestmark = pytest.mark.gpu


def _world(max_bodies):
    from substrata_amd.lib import World
    return World(max_bodies=max_bodies)


@pytest.fixture(scope="module")
def run():
    r = bc.run_table(_world)
    r.errors = bc.compare(r)
    yield r
    r.wet.close()


def test_table_keeps_its_promises(run):
    bc.table_conditions(run)


def test_submerged_volume(run):
    vol_err = run.errors[0]
    k = int(np.argmax(vol_err))
    print(f"worst volume error {vol_err[k]:.3g} eps32 V_total, {bc.describe(run, k)}")
    assert vol_err[k] <= 16.0, bc.describe(run, k)


def test_underwater_flag(run):
    bad = np.nonzero(~run.errors[3])[0]
    assert len(bad) == 0, [bc.describe(run, int(k)) for k in bad[:5]]


@pytest.mark.parametrize("which", ["linear", "angular"])
def test_velocity_change(run, which):
    err = run.errors[1 if which == "linear" else 2]
    k = int(np.argmax(err))
    print(f"worst {which} velocity change error {err[k]:.3g} of the bound, {bc.describe(run, k)}")
    assert err[k] <= 1.0, bc.describe(run, k)


def test_events_and_flags(run):
    """(last: steps the wet world on)"""
    bc.check_events_and_flags(run)


def test_sleeper_under_water():
    bc.check_sleeper(_world)
