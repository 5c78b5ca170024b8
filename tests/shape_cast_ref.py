"""A float64 reference for shape casts of convex polytopes under pure translation, and the random field of boxes the shape-cast tests share.

For every candidate separating axis (the face normals of both polytopes and the cross products of their edge directions; a superset is fine) the
projections of the two polytopes overlap during an interval of t; the polytopes overlap exactly while all of those intervals do, so the
intersection of the intervals is [t_enter, t_exit] and the contact normal at the first touch is the axis that gave t_enter.  Boxes take their
15 axes; convex hulls take their face normals by brute force over vertex triples and their edge directions from all vertex pairs."""
import numpy as np

GRAZING = 0.2          # |n . dir| below this: the entry time moves by more than 5 tolerances per tolerance of separation


def quat_to_mat(q):
    x, y, z, w = (float(v) for v in q)
    n = x * x + y * y + z * z + w * w
    s = 2.0 / n
    return np.array([[1 - s * (y * y + z * z), s * (x * y - z * w), s * (x * z + y * w)],
                     [s * (x * y + z * w), 1 - s * (x * x + z * z), s * (y * z - x * w)],
                     [s * (x * z - y * w), s * (y * z + x * w), 1 - s * (x * x + y * y)]], dtype=np.float64)


class Polytope:
    """Vertices (world, float64), unit face normals and edge directions of a convex polytope."""

    def __init__(self, verts, normals, edges):
        self.verts, self.normals, self.edges = np.asarray(verts, np.float64), np.asarray(normals, np.float64), np.asarray(edges, np.float64)


def box_polytope(pos, rot, half):
    R = quat_to_mat(rot)
    h = np.asarray(half, np.float64)
    signs = np.array([[sx, sy, sz] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)], np.float64)
    return Polytope(np.asarray(pos, np.float64) + (signs * h) @ R.T, R.T.copy(), R.T.copy())


def hull_local_polytope(points):
    """Face normals by brute force over vertex triples, edge directions from all vertex pairs (a superset of the hull's edges), in the points' frame."""
    P = np.asarray(points, np.float64)
    n = len(P)
    normals = []
    for i in range(n):
        for j in range(i + 1, n):
            for k in range(j + 1, n):
                c = np.cross(P[j] - P[i], P[k] - P[i])
                l = np.linalg.norm(c)
                if l < 1e-12:
                    continue
                c = c / l
                d = (P - P[i]) @ c
                if d.max() <= 1e-9:
                    normals.append(c)
                elif d.min() >= -1e-9:
                    normals.append(-c)
    edges = []
    for i in range(n):
        for j in range(i + 1, n):
            e = P[j] - P[i]
            edges.append(e / np.linalg.norm(e))
    return Polytope(P, np.array(normals), np.array(edges))


def hull_polytope(local, pos, rot):
    """A polytope given in its body frame (hull_local_polytope of the body-frame vertices) at a pose."""
    R = quat_to_mat(rot)
    return Polytope(np.asarray(pos, np.float64) + local.verts @ R.T, local.normals @ R.T, local.edges @ R.T)


def body_frame_points(points, info):
    """The points of a hull in the body frame sgp_hull_create stores it in (input point = com + rot * body point)."""
    R = quat_to_mat(info.rot[:])
    return (np.asarray(points, np.float32).astype(np.float64) - np.array(info.com[:], np.float64)) @ R


def cast(body, shape, direction, max_t):
    """The moving polytope `shape` (at t = 0) against the resting `body`.  Returns None (no overlap within [0, max_t]) or (t_enter, normal, t_exit);
    t_enter < 0 means the two overlap at t = 0.  normal: unit, from the body towards the shape, the axis that gave t_enter."""
    d = np.asarray(direction, np.float64)
    axes = [body.normals, shape.normals]
    cr = np.cross(body.edges[:, None, :], shape.edges[None, :, :]).reshape(-1, 3)
    l = np.linalg.norm(cr, axis=1)
    axes.append(cr[l > 1e-9] / l[l > 1e-9, None])
    A = np.concatenate(axes)
    pa = body.verts @ A.T
    pb = shape.verts @ A.T
    a0, a1, b0, b1 = pa.min(0), pa.max(0), pb.min(0), pb.max(0)
    v = A @ d
    still = np.abs(v) < 1e-14
    if np.any(still & ((b0 > a1) | (b1 < a0))):
        return None                                # an axis the motion does not change keeps them apart
    m = ~still
    ta, tb = (a1[m] - b0[m]) / v[m], (a0[m] - b1[m]) / v[m]      # the shape leaves / reaches the body's far / near side along each axis
    lo, hi = np.minimum(ta, tb), np.maximum(ta, tb)
    i = int(np.argmax(lo))
    t_enter, t_exit = float(lo[i]), float(hi.min())
    normal = -A[m][i] * np.sign(v[m][i])           # the shape comes in against the normal
    if t_enter > t_exit or t_exit < 0 or t_enter > max_t:
        return None
    return t_enter, normal, t_exit


# ---- the field --------------------------------------------------------------------------------------------------

N_BODIES, N_CASTS = 48, 96


def field():
    """48 static boxes and 96 box casts through them; everything rounded to float32 (what both sides are given)."""
    rng = np.random.default_rng(21)
    f32 = lambda a: np.asarray(a, np.float64).astype(np.float32)
    centres = f32(rng.uniform(-4, 4, (N_BODIES, 3)))
    halves = f32(rng.uniform(0.2, 0.6, (N_BODIES, 3)))
    q = rng.normal(size=(N_BODIES, 4)); rots = f32(q / np.linalg.norm(q, axis=1, keepdims=True))
    s = rng.normal(size=(N_CASTS, 3)); starts = f32(s / np.linalg.norm(s, axis=1, keepdims=True) * 7)
    targets = rng.uniform(-3, 3, (N_CASTS, 3))
    delta = targets - starts.astype(np.float64)
    dist = np.linalg.norm(delta, axis=1)
    dirs = f32(delta / dist[:, None])
    max_t = f32(dist + 4)
    cast_halves = f32(rng.uniform(0.25, 0.6, (N_CASTS, 3)))
    q = rng.normal(size=(N_CASTS, 4)); cast_rots = f32(q / np.linalg.norm(q, axis=1, keepdims=True))
    return dict(centres=centres, halves=halves, rots=rots, starts=starts, dirs=dirs, max_t=max_t, cast_halves=cast_halves, cast_rots=cast_rots)


def first_hits(bodies, shapes, dirs, max_t):
    """Per cast: None, or (body index, t, normal) of the body touched first -- t = max(t_enter, 0): bodies the shape overlaps at the start all count as t = 0 --,
    ties: the lower index.  Bodies whose bounding sphere the swept bounding sphere of the shape cannot reach are not asked."""
    out = []
    cb = [(b.verts.mean(0), np.linalg.norm(b.verts - b.verts.mean(0), axis=1).max()) for b in bodies]
    for k, shape in enumerate(shapes):
        best = None
        c0 = shape.verts.mean(0); r0 = np.linalg.norm(shape.verts - c0, axis=1).max()
        d = np.asarray(dirs[k], np.float64)
        for j, body in enumerate(bodies):
            rel = cb[j][0] - c0
            along = np.clip(rel @ d, 0.0, float(max_t[k]))
            if np.linalg.norm(rel - along * d) > cb[j][1] + r0 + 1e-6:
                continue
            r = cast(body, shape, d, float(max_t[k]))
            if r is not None and (best is None or max(r[0], 0.0) < best[1]):
                best = (j, max(r[0], 0.0), r[1])
        out.append(best)
    return out


def field_box_hits(f):
    bodies = [box_polytope(f["centres"][j], f["rots"][j], f["halves"][j]) for j in range(N_BODIES)]
    shapes = [box_polytope(f["starts"][k], f["cast_rots"][k], f["cast_halves"][k]) for k in range(N_CASTS)]
    return first_hits(bodies, shapes, f["dirs"].astype(np.float64), f["max_t"])
