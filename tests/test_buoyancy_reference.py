"""tests/buoyancy_reference.py against closed forms, then the CPU oracle's buoyancy sweep against it on the case table of tests/buoyancy_cases.py.

Bounds (float32 rounding units, not tuned):
  volume                 |got - ref| <= 16 eps32 V_total       (V_total: the box, the capsule's stand-in box, the hull, the sphere)
  velocity change, each  |got - ref| <= 8 eps32 max|v| + 2e-5 max|dv_ref|, the maxima over all the body's velocity components (buoyancy_cases.compare)
Measured on the CPU oracle, 391 cases: volume 1.7 eps32 V_total; linear change 0.13 of its bound, angular change 0.42 of its bound.
Before the fully submerged hull reported its own centroid as the centre of buoyancy, 9 of the table's 12 fully submerged offset hulls failed here (the
other three are weightless and at rest: no impulse), by 550 to 49000 times the bound on the angular change -- 1 % to 100 % of that change, and up to 40 %
of the linear one -- and nothing else did.
"""
import numpy as np
import pytest

import buoyancy_cases as bc
from buoyancy_reference import Polytope, Shape, evaluate, quat_to_mat, sphere_cap


def _rot(axis, angle):
    return quat_to_mat(bc._q_axis_angle(axis, angle))


# ---- the reference against closed forms ------------------------------------------------------------------------------------------------------------

def test_axis_aligned_box_is_face_area_times_depth():
    h = np.array([0.35, 0.3, 0.25])
    box = Shape.box(h)
    for R, up in ((np.eye(3), 2), (_rot((1, 0, 0), 0.5 * np.pi), 1), (_rot((0, 1, 0), 0.5 * np.pi), 0)):
        area = 8.0 * h[0] * h[1] * h[2] / (2.0 * h[up])
        for depth in (-h[up] + 1.0e-5, -0.1, 0.0, 0.17, h[up] - 1.0e-6):
            vol, cen = box.submerged(R, depth)
            assert abs(vol - area * (depth + h[up])) <= 1.0e-14
            assert np.allclose(cen, (0.0, 0.0, 0.5 * (depth - h[up])), atol=1.0e-11)      # (a turn by pi / 2 is one to 1e-16, which tilts the centroid of a 1e-5 slab by 1e-13)
    assert box.submerged(np.eye(3), -0.25)[0] == 0.0 and abs(box.submerged(np.eye(3), 0.25)[0] - box.total) <= 1.0e-15


def test_apex_down_tetrahedron_is_a_similar_solid():
    a = 1.0
    height = a * np.sqrt(2.0 / 3.0)
    tet = Polytope([(0, 0, height), (a, 0, height), (a / 2, a * np.sqrt(3) / 2, height), (a / 2, a * np.sqrt(3) / 6, 0.0)])
    vol = a ** 3 / (6.0 * np.sqrt(2.0))
    assert abs(tet.volume - vol) <= 1.0e-15 and np.allclose(tet.centroid, (a / 2, a * np.sqrt(3) / 6, 0.75 * height), atol=1.0e-15)
    for t in (1.0e-3, 0.2, 0.5, 0.999):
        v, c = tet.below(np.array([0.0, 0.0, 1.0]), t * height)
        assert abs(v - vol * t ** 3) <= 1.0e-15
        assert np.allclose(c, (a / 2, a * np.sqrt(3) / 6, 0.75 * t * height), atol=1.0e-13)


def test_sphere_cap_against_a_numerical_integral():
    r = 0.35
    for depth in (-0.3, -0.05, 0.0, 0.2, 0.349):
        zz = np.linspace(-r, depth, 200001)
        a = np.pi * (r * r - zz * zz)
        vol = np.sum(0.5 * (a[1:] + a[:-1]) * np.diff(zz))
        mom = np.sum(0.5 * (a[1:] * zz[1:] + a[:-1] * zz[:-1]) * np.diff(zz))
        v, cz = sphere_cap(r, depth)
        assert abs(v - vol) <= 1.0e-5 * vol and abs(cz - mom / vol) <= 1.0e-5 * r
    assert sphere_cap(r, -r)[0] == 0.0 and abs(sphere_cap(r, r)[0] - 4.0 / 3.0 * np.pi * r ** 3) <= 1.0e-15


def test_centroid_symmetry_and_complement():
    """A cut through the centre of a box halves it, whatever the tilt, and the two parts of any cut put the centroid of the whole back together."""
    rng = np.random.default_rng(3)
    box = Shape.box((0.35, 0.3, 0.25))
    cloud = Polytope(rng.uniform(-1.0, 1.0, size=(16, 3)) * (0.35, 0.3, 0.25))
    for _ in range(8):
        R = _rot(rng.normal(size=3), rng.uniform(0.0, 3.0))
        vol, cen = box.submerged(R, 0.0)
        assert abs(vol - 0.5 * box.total) <= 1.0e-14
        up_vol, up_cen = box.submerged(np.diag([1.0, -1.0, -1.0]) @ R, 0.0)      # turned upside down about the world's x: the other half, the mirror image through the centre
        assert abs(up_vol - vol) <= 1.0e-14 and np.allclose(up_cen, (-cen[0], cen[1], cen[2]), atol=1.0e-13)
        n, d = R[2], rng.uniform(-0.1, 0.1)
        v1, c1 = cloud.below(n, d)
        v2, c2 = cloud.below(-n, -d)
        assert abs(v1 + v2 - cloud.volume) <= 1.0e-14
        assert np.allclose(v1 * c1 + v2 * c2, cloud.volume * cloud.centroid, atol=1.0e-14)


def test_hull_volume_against_scipy():
    spatial = pytest.importorskip("scipy.spatial")
    rng = np.random.default_rng(4)
    for n in (4, 8, 16, 24):
        pts = rng.uniform(-1.0, 1.0, size=(n, 3)) * (0.35, 0.3, 0.25)
        p = Polytope(pts)
        hull = spatial.ConvexHull(pts)
        assert abs(p.volume - hull.volume) <= 1.0e-12 and len(p.verts) == len(hull.vertices)
    cube = Polytope(bc._box_points((0.3, 0.25, 0.2)))
    assert len(cube.edges) == 12 and abs(cube.volume - 8 * 0.3 * 0.25 * 0.2) <= 1.0e-7      # (float32 corners) quads are one face: no diagonal is an edge


def test_capsule_inertia_and_clamps_of_the_sweep():
    """The thin capsule's transverse inertia against a numerical integral over its length; a drag impulse never reverses the body in the water."""
    r, hh = 0.1, 1.0
    cap = Shape.capsule(r, hh)
    z = np.linspace(-(hh + r), hh + r, 200001)
    rad2 = np.where(np.abs(z) <= hh, r * r, np.maximum(r * r - (np.abs(z) - hh) ** 2, 0.0))
    f = np.pi * rad2 * (0.25 * rad2 + z * z)                      # a disc about a diameter, moved to the capsule's centre
    ix = np.sum(0.5 * (f[1:] + f[:-1]) * np.diff(z)) / cap.real_volume
    assert abs(ix - cap.unit_mass_inertia[0]) <= 1.0e-8 * ix
    res = evaluate(Shape.box((0.35, 0.3, 0.25)), 1.0, 0.0, 0, (0, 0, -2.0), (0, 0, 0, 1), (5.0, 0, 0), (0, 0, 0), 0.0, bc.DT)
    assert res.lin_clamped and np.allclose(res.dlin, (-5.0, 0.0, 0.0), atol=1.0e-12)
    res = evaluate(cap, 80.0, 0.0, 0, (0, 0, -2.0), (0, 0, 0, 1), (0, 0, 0), (0, 0, 3.0), 0.0, bc.DT)
    assert res.ang_clamped and np.allclose(res.dang, (0.0, 0.0, -3.0), atol=1.0e-12)


# ---- the CPU oracle against the reference ------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def run(oracle):
    r = bc.run_table(lambda n: oracle.OracleWorld(max_bodies=n))
    r.errors = bc.compare(r)
    yield r
    r.wet.close()


def test_table_keeps_its_promises(run):
    bc.table_conditions(run)


def test_oracle_submerged_volume(run):
    vol_err = run.errors[0]
    k = int(np.argmax(vol_err))
    print(f"worst volume error {vol_err[k]:.3g} eps32 V_total, {bc.describe(run, k)}")
    assert vol_err[k] <= 16.0, bc.describe(run, k)


def test_oracle_underwater_flag(run):
    bad = np.nonzero(~run.errors[3])[0]
    assert len(bad) == 0, [bc.describe(run, int(k)) for k in bad[:5]]


@pytest.mark.parametrize("which", ["linear", "angular"])
def test_oracle_velocity_change(run, which):
    err = run.errors[1 if which == "linear" else 2]
    k = int(np.argmax(err))
    print(f"worst {which} velocity change error {err[k]:.3g} of the bound, {bc.describe(run, k)}")
    bad = np.nonzero(err > 1.0)[0]
    assert len(bad) == 0, (len(bad), [bc.describe(run, int(j)) for j in bad[:5]])


def test_oracle_events_and_flags(run):
    """(last: steps the wet world on)"""
    bc.check_events_and_flags(run)


def test_oracle_sleeper_under_water(oracle):
    bc.check_sleeper(lambda n: oracle.OracleWorld(max_bodies=n))
