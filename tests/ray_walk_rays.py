"""The world and the rays of tests/test_ray_walk_gpu.py.

The world is the scene of raycast_any_scene.py with 36 static posts added, built with large_body_radius = 1.5.  The host sorts static large bodies into
their grid only when there are at least 32 of them (fewer stay on the list every ray tests directly), and the scene has five: the posts (bounding radius
1.61) make up the number, so that the terrain mesh, the height field, the portal and the sensor are reached through the grid's walk.  The scene's small
dynamic bodies stay in the broad phase's cells (a few boxes and capsules above 1.5 go on the list), and the ground, which would fill too many cells,
stays on the list too: all three stages of the world walk have bodies to find.

The rays are those that seeded segments between points of a box do not produce: directions with two and with one component exactly zero, in both
signs along every axis; origins outside both grids pointing in, pointing away and running along a face with the perpendicular axis's rule deciding
(origin inside, on the edge of, and outside the box on an axis the ray does not move along); origins in the border cells, one cell outside the cells
that hold bodies; and max_t ending inside the first cell."""
import numpy as np

from substrata_amd import abi, scenes
import raycast_any_scene as scene

LARGE_BODY_RADIUS = 1.5
POST_HALF = (0.1, 0.1, 1.6)
POST_XY = (-20.0, -12.0, -4.0, 4.0, 12.0, 20.0)
AXES = [np.float32(v) for v in ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1))]
DIAGONALS = [np.float32(v) / np.float32(np.sqrt(2.0)) for v in ((1, 1, 0), (1, -1, 0), (-1, 1, 0), (-1, -1, 0), (1, 0, 1), (1, 0, -1), (-1, 0, 1), (-1, 0, -1),
                                                                (0, 1, 1), (0, 1, -1), (0, -1, 1), (0, -1, -1))]
P0, P1 = np.float32([0.5, -0.5, 2.0]), np.float32([-3.0, 4.0, 1.5])      # two points among the bodies
FAR = np.float32(35.0)                                                    # from there: outside both grids (the posts end at 20, the cells' bodies at 11)


def build(w, field_as_mesh=False):
    """The scene and the posts in the empty world `w` (created with large_body_radius=LARGE_BODY_RADIUS).  Returns {kind: ids}."""
    ids = scene.build(w, field_as_mesh)
    posts = scenes._blank(len(POST_XY) ** 2)
    posts["shape"][:, :3] = POST_HALF
    posts["pos"] = [(x, y, 1.6 if (i + j) % 2 == 0 else 8.0) for j, y in enumerate(POST_XY) for i, x in enumerate(POST_XY)]      # (two levels: the grid is more than one cell high)
    ids["post"] = [int(i) for i in w.add_batch(posts)]
    return ids


def rays():
    """65 rays of abi.ray_dtype (unit directions)."""
    out = []

    def ray(origin, direction, max_t):
        out.append((np.float32(origin), np.float32(direction), np.float32(max_t)))
    for d in AXES + DIAGONALS:                       # from among the bodies: two zero components, then one
        ray(P0, d, 40.0)
    for d in AXES:                                   # from outside both grids, pointing in
        ray(P0 - FAR * d, d, 80.0)
    for d in DIAGONALS:
        ray(P1 - FAR * d, d, 80.0)
    for d in AXES:                                   # from outside, pointing away
        ray(P0 + FAR * d, d, 80.0)
    for y in (11.0, 12.0, 12.5, 13.5, 20.05, 26.0, 27.5, 40.0):      # along +x at rest on the y axis: inside the cells, at their edge, in the border cells, among the last posts, beyond everything
        ray((-30.0, y, 2.0), AXES[0], 80.0)
    # origins in the border cells (the cells of the small bodies: their centres lie within +-11 and 0.8 .. 4.5; the posts' grid ends at +-20.1)
    ray((-12.0, 3.0, 0.3), AXES[0], 40.0); ray((12.0, -3.0, 0.3), AXES[1], 40.0); ray((2.0, -12.0, 2.0), AXES[2], 40.0); ray((-2.0, 12.0, 2.0), AXES[3], 40.0)
    ray((1.0, 1.0, 5.2), AXES[5], 40.0); ray((-23.0, 0.4, 1.0), AXES[0], 60.0); ray((23.0, -4.05, 1.0), AXES[1], 60.0); ray((4.05, -23.0, 1.0), AXES[2], 60.0)
    # max_t ending inside the first cell
    ray(P0, AXES[0], 0.3); ray(P0, AXES[2], 0.3); ray(P0, AXES[4], 0.3)      # (the second one ends inside a box)
    ray((-12.4, 2.0, 2.0), AXES[0], 0.5); ray((0.5, 12.4, 3.0), AXES[3], 0.6); ray((-26.0, 0.4, 1.0), AXES[0], 1.0); ray((3.0, 3.0, 5.4), AXES[5], 0.7)
    r = np.zeros(len(out), dtype=abi.ray_dtype)
    r["origin"] = [o for o, _, _ in out]; r["dir"] = [d for _, d, _ in out]; r["max_t"] = [t for _, _, t in out]
    r["ignore_id"] = abi.INVALID_ID
    assert len(r) == 65
    return r
