"""The yardstick of the shape-cast tests is checked before it is used: the float64 reference of tests/shape_cast_ref.py against the oracle's narrow
phase on the field of boxes both the CPU and the GPU tests use.  For every hit the oracle finds no contact 1 mm before the reference's entry time and a
contact 1 mm after it.  No GPU."""
import numpy as np
import pytest

from substrata_amd import abi
import shape_cast_ref as ref


@pytest.fixture(scope="module")
def hits():
    f = ref.field()
    return f, ref.field_box_hits(f)


def box_desc(pos, rot, half):
    d = abi.BodyDesc()
    d.pos[:] = [float(x) for x in pos]; d.rot[:] = [float(x) for x in rot]; d.shape_type = abi.SHAPE_BOX
    d.shape[:] = [float(half[0]), float(half[1]), float(half[2]), 0.0]
    return d


def test_the_field_is_what_the_issue_counted(hits):
    f, h = hits
    found = [x for x in h if x is not None]
    assert len(found) == 90 and len(h) == 96
    assert all(x[1] > 0 for x in found)                  # none starts overlapping
    grazing = [k for k, x in enumerate(h) if x is not None and abs(np.dot(x[2], f["dirs"][k].astype(np.float64))) < ref.GRAZING]
    assert len(grazing) == 3


def test_normals_are_unit_and_oppose_the_motion(hits):
    f, h = hits
    for k, x in enumerate(h):
        if x is None:
            continue
        assert abs(np.linalg.norm(x[2]) - 1) < 1e-12 and np.dot(x[2], f["dirs"][k].astype(np.float64)) < 0


def test_reference_brackets_the_oracle_narrow_phase(hits, oracle):
    f, h = hits
    ow = oracle.OracleWorld(max_bodies=16)
    try:
        for k, x in enumerate(h):
            if x is None:
                continue
            j, t, _ = x
            body = box_desc(f["centres"][j], f["rots"][j], f["halves"][j])
            for dt, expect in ((-1e-3, False), (1e-3, True)):
                pos = f["starts"][k].astype(np.float64) + (t + dt) * f["dirs"][k].astype(np.float64)
                r = oracle.world_collide_pair(ow, body, box_desc(pos, f["cast_rots"][k], f["cast_halves"][k]), 0.0)
                assert (r is not None) == expect, (k, j, t, dt)
    finally:
        ow.close()


def test_hull_polytope_of_a_cube_is_the_box():
    pts = np.array([[sx, sy, sz] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)], np.float64) * (0.5, 0.3, 0.2)
    loc = ref.hull_local_polytope(pts)
    rot = np.array([0.1, -0.3, 0.2, 0.9]); rot /= np.linalg.norm(rot)
    body = ref.box_polytope((0, 0, 0), (0, 0, 0, 1), (1, 1, 1))
    a = ref.cast(body, ref.hull_polytope(loc, (0.2, 5, 0.1), rot), (0, -1, 0), 10.0)
    b = ref.cast(body, ref.box_polytope((0.2, 5, 0.1), rot, (0.5, 0.3, 0.2)), (0, -1, 0), 10.0)
    assert a is not None and abs(a[0] - b[0]) < 1e-12 and np.allclose(a[1], b[1], atol=1e-12)
