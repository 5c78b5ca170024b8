"""Float64 restatement of the water buoyancy sweep (docs/CONTRACT.md, "Buoyancy sweep"), numpy only.

Written from the statement of what the sweep computes, not from the kernel (k_buoyancy, sgp_k_sweep.hip) or the oracle (buoyancy_sweep,
sgo_oracle.c), whose method -- every face clipped to the half space and fanned into signed tetrahedra, the cut closed by an angle-sorted cap
polygon -- it does not share.  Here the part of a convex body under the water plane is taken for what it is, a convex body of its own: its
corners are the body's corners under the plane and the points where the body's edges cross it; its faces are found by brute force (every plane
through three of those points that has all the others on one side; coplanar triples make one face); its volume and centroid are sums over the
tetrahedra (interior point, face centre, edge of the face), all of them positive.

    shape = Shape.box(h) | Shape.sphere(r) | Shape.capsule(r, hh) | Shape.hull(points, info, offset)
    res = evaluate(shape, mass, gravity_factor, zero_lin_drag, pos, rot, lin_vel, ang_vel, water_z, dt)
"""
import itertools

import numpy as np

FLUID_DENSITY = 1020.0                       # kg / m^3, hard-wired
GRAVITY = np.array([0.0, 0.0, -9.81])        # hard-wired, whatever the world's gravity
LINEAR_DRAG, ANGULAR_DRAG = 0.1, 3.0


def quat_to_mat(q):
    """Rotation matrix of a quaternion (x, y, z, w)."""
    x, y, z, w = (float(c) for c in q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


# ---------------------------------------------------------------------------------------------------------------------
# convex bodies by brute force

def _dedupe(pts, tol):
    keep = []
    for p in pts:
        if all(np.max(np.abs(p - q)) > tol for q in keep):
            keep.append(p)
    return np.array(keep)


def convex_faces(pts, tol):
    """Faces of the convex hull of pts (n x 3) by brute force: [(unit outward normal, sorted point indices)].  Every plane through three points that has
    no point more than tol in front of it supports the hull; all points within tol of it form the face, so a quad or a hexagon is one face."""
    n = len(pts)
    tri = np.array(list(itertools.combinations(range(n), 3)))
    if len(tri) == 0:
        return []
    a, b, c = pts[tri[:, 0]], pts[tri[:, 1]], pts[tri[:, 2]]
    nrm = np.cross(b - a, c - a)
    ln = np.linalg.norm(nrm, axis=1)
    # (a triple that spans no area to speak of names no plane: longest edge squared times 1e-7)
    span = np.maximum(np.maximum(np.sum((b - a) ** 2, 1), np.sum((c - a) ** 2, 1)), np.sum((c - b) ** 2, 1))
    ok = ln > 1.0e-7 * span
    tri, a, nrm = tri[ok], a[ok], nrm[ok] / ln[ok, None]
    s = nrm @ pts.T - np.sum(nrm * a, axis=1)[:, None]            # signed distance of every point from every candidate plane
    hi, lo = s.max(axis=1), s.min(axis=1)
    faces = {}
    for k in np.nonzero((hi <= tol) | (lo >= -tol))[0]:
        if hi[k] <= tol and lo[k] >= -tol:
            continue                                               # every point in one plane: no body
        sign = 1.0 if hi[k] <= tol else -1.0
        key = tuple(np.nonzero(np.abs(s[k]) <= tol)[0])
        if key not in faces:
            faces[key] = sign * nrm[k]
    return [(nv, list(key)) for key, nv in faces.items()]


def face_edges(pts, normal, idx, tol):
    """The sides of a convex face: the pairs of its points that have all its other points on one side of their line (in the face's plane) and none between them."""
    out = []
    for i, j in itertools.combinations(idx, 2):
        e = pts[j] - pts[i]
        le = np.linalg.norm(e)
        side = np.cross(normal, e / le)
        s = [(float(np.dot(pts[k] - pts[i], side)), float(np.dot(pts[k] - pts[i], e) / (le * le))) for k in idx if k != i and k != j]
        if not (all(d <= tol for d, _ in s) or all(d >= -tol for d, _ in s)):
            continue
        if any(abs(d) <= tol and 0.0 < t < 1.0 for d, t in s):
            continue                                               # a point of the face lies on this stretch: its two halves are the sides
        out.append((i, j))
    return out


def convex_volume_centroid(pts, tol):
    """Volume and centroid of the convex hull of pts.  Also returns (faces, edges) with edges the set of index pairs that are sides of a face."""
    faces = convex_faces(pts, tol)
    if len(faces) < 4:
        return 0.0, np.zeros(3), faces, set()
    inner = pts.mean(axis=0)
    vol, mom, edges = 0.0, np.zeros(3), set()
    closed = np.zeros(3); area_sum = 0.0
    for normal, idx in faces:
        centre = pts[idx].mean(axis=0)
        for i, j in face_edges(pts, normal, idx, tol):
            edges.add((min(i, j), max(i, j)))
            tv = abs(np.dot(centre - inner, np.cross(pts[i] - inner, pts[j] - inner))) / 6.0
            vol += tv
            mom += tv * (inner + centre + pts[i] + pts[j]) / 4.0
            ta = 0.5 * np.linalg.norm(np.cross(pts[i] - centre, pts[j] - centre))
            closed += ta * normal; area_sum += ta
    # a closed surface: the area vectors of its faces cancel (a face counted twice or missed would show here)
    assert np.linalg.norm(closed) <= 1.0e-9 * area_sum + 1.0e-18, (closed, area_sum)
    return vol, (mom / vol if vol > 0.0 else np.zeros(3)), faces, edges


class Polytope:
    """A convex body given by points (body frame): its corners and edges, found once."""

    def __init__(self, points):
        pts = np.asarray(points, np.float64).reshape(-1, 3)
        self.extent = float(np.max(np.abs(pts)))
        self.tol = 1.0e-9 * self.extent
        self.volume, self.centroid, faces, edges = convex_volume_centroid(pts, self.tol)
        used = sorted({i for e in edges for i in e})
        self.verts = pts[used]
        remap = {i: k for k, i in enumerate(used)}
        self.edges = np.array([(remap[i], remap[j]) for i, j in sorted(edges)])
        self.aabb_min, self.aabb_max = self.verts.min(axis=0), self.verts.max(axis=0)

    def heights(self, R):
        """World z of every corner relative to the body origin."""
        return self.verts @ R[2]

    def below(self, n, d):
        """Volume and centroid (body frame) of the part with n . x <= d."""
        s = self.verts @ n - d
        if np.all(s >= 0.0):
            return 0.0, np.zeros(3)
        if np.all(s <= 0.0):
            return self.volume, self.centroid
        pts = [self.verts[i] for i in np.nonzero(s <= 0.0)[0]]
        for i, j in self.edges:
            if (s[i] < 0.0 < s[j]) or (s[j] < 0.0 < s[i]):
                t = s[i] / (s[i] - s[j])
                pts.append(self.verts[i] + t * (self.verts[j] - self.verts[i]))
        pts = _dedupe(pts, self.tol)
        vol, cen, _, _ = convex_volume_centroid(pts, self.tol)
        return vol, cen


def sphere_cap(r, depth):
    """Volume of the part of a sphere of radius r under a plane `depth` above its centre, and the z of that part's centroid relative to the centre."""
    h = min(max(depth + r, 0.0), 2.0 * r)                          # height of the cap, from the sphere's lowest point
    vol = np.pi * h * h * (3.0 * r - h) / 3.0
    cz = -3.0 * (2.0 * r - h) ** 2 / (4.0 * (3.0 * r - h)) if h > 0.0 else 0.0
    return vol, cz


# ---------------------------------------------------------------------------------------------------------------------
# shapes

class Shape:
    """What the sweep needs to know of a shape: kind, real volume, the volume the submerged part is measured against (`total`), the box the drag takes
    for it (`size`), principal moments of inertia per unit mass, and its polytope (box, hull; for a capsule the stand-in box)."""

    def __init__(self, kind, params, real_volume, total, size, unit_mass_inertia, poly=None):
        self.kind, self.params, self.real_volume, self.total = kind, params, float(real_volume), float(total)
        self.size, self.unit_mass_inertia, self.poly = np.asarray(size, np.float64), np.asarray(unit_mass_inertia, np.float64), poly

    @staticmethod
    def _box_poly(h):
        return Polytope([(sx * h[0], sy * h[1], sz * h[2]) for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)])

    @classmethod
    def box(cls, h):
        h = np.asarray(h, np.float64)
        s = 2.0 * h
        v = s[0] * s[1] * s[2]
        return cls("box", h, v, v, s, [(s[1] ** 2 + s[2] ** 2) / 12.0, (s[0] ** 2 + s[2] ** 2) / 12.0, (s[0] ** 2 + s[1] ** 2) / 12.0], cls._box_poly(h))

    @classmethod
    def sphere(cls, r):
        v = 4.0 / 3.0 * np.pi * r ** 3
        return cls("sphere", (float(r),), v, v, [2.0 * r] * 3, [0.4 * r * r] * 3)

    @classmethod
    def capsule(cls, r, hh):
        """Along z: a cylinder of half height hh and two hemispheres of radius r, uniform density."""
        vc, vs = np.pi * r * r * 2.0 * hh, 4.0 / 3.0 * np.pi * r ** 3
        mc, ms = vc / (vc + vs), vs / (vc + vs)                    # mass shares of the cylinder and of the two hemispheres
        iz = 0.5 * mc * r * r + 0.4 * ms * r * r
        # a hemisphere about a transverse axis through its own centre of mass: (2/5 - 9/64) m r^2; that centre lies hh + 3 r / 8 from the capsule's
        ix = mc * (3.0 * r * r + (2.0 * hh) ** 2) / 12.0 + ms * ((0.4 - 9.0 / 64.0) * r * r + (hh + 0.375 * r) ** 2)
        hb = np.array([r, r, hh + r])                              # the oriented box that stands in for the submerged part
        return cls("capsule", (float(r), float(hh)), vc + vs, 8.0 * hb[0] * hb[1] * hb[2], 2.0 * hb, [ix, ix, iz], cls._box_poly(hb))

    @classmethod
    def hull(cls, points, info, offset=None):
        """points: the float32 cloud handed to hull_create; info: the HullInfo it returned (com, rot: the body frame in the frame of the points;
        volume, unit_inertia: principal moments for density 1)."""
        p32 = np.asarray(points, np.float32).reshape(-1, 3)
        com, R0 = np.array(info.com[:], np.float64), quat_to_mat(info.rot[:])
        poly = Polytope((p32.astype(np.float64) - com) @ R0)      # body = R0^T (p - com)
        # the body origin is the hull's centroid moved by the offset, and nothing else
        cloud = Polytope(p32.astype(np.float64))
        o = np.zeros(3) if offset is None else np.asarray(offset, np.float64)
        assert np.max(np.abs(com - o - cloud.centroid)) <= 4.0e-7 * cloud.extent, (com, o, cloud.centroid)      # (com is a float32 triple)
        vol = float(info.volume)
        assert abs(vol - poly.volume) <= 1.0e-6 * poly.volume, (vol, poly.volume)
        size = 2.0 * np.maximum(np.abs(poly.aabb_min), np.abs(poly.aabb_max))      # a box symmetric about the origin, NOT aabb_max - aabb_min
        return cls("hull", None, vol, vol, size, np.array(info.unit_inertia[:], np.float64) / vol, poly)

    def vertical_extent(self, R):
        """(lowest, highest) world z of the body itself relative to its origin -- what its world AABB spans."""
        if self.kind == "sphere":
            return -self.params[0], self.params[0]
        if self.kind == "capsule":
            r, hh = self.params
            e = abs(R[2, 2]) * hh + r
            return -e, e
        z = self.poly.heights(R)
        return float(z.min()), float(z.max())

    def submerged(self, R, depth):
        """Volume under the plane `depth` above the body origin and that part's centroid relative to the origin, world axes."""
        if self.kind == "sphere":
            vol, cz = sphere_cap(self.params[0], depth)
            return vol, np.array([0.0, 0.0, cz])
        vol, cen = self.poly.below(R[2], depth)                    # the plane's normal in the body frame is R^T z = the third row of R
        return vol, R @ cen


# ---------------------------------------------------------------------------------------------------------------------
# the sweep for one body

class Result:
    def __init__(self, **kw):
        self.__dict__.update(kw)


def evaluate(shape, mass, gravity_factor, zero_lin_drag, pos, rot, lin_vel, ang_vel, water_z, dt):
    """One active dynamic body: submerged volume, the underwater flag and the change of its velocities."""
    pos, v, w = (np.asarray(a, np.float64) for a in (pos, lin_vel, ang_vel))
    R = quat_to_mat(rot)
    lo, hi = shape.vertical_extent(R)
    res = Result(volume=0.0, underwater=False, dlin=np.zeros(3), dang=np.zeros(3), lin_clamped=False, ang_clamped=False, fraction=0.0,
                 fully_submerged=False, bottom=float(pos[2] + lo), cob=np.zeros(3))
    if not (pos[2] + lo < water_z):                                # the gate: the body's own bounds reach under the plane
        return res
    sub, rc = shape.submerged(R, water_z - pos[2])
    if not (sub > 0.0):
        return res
    frac = sub / shape.total
    inv_mass = 1.0 / mass
    rho = FLUID_DENSITY * shape.real_volume / shape.total         # fluid density as the stand-in volume sees it
    buoy_imp = -GRAVITY * rho * sub * gravity_factor * dt
    rel = -(v + np.cross(w, rc))                                   # still water, seen from the centre of buoyancy
    lrel = R.T @ rel
    rl = float(np.linalg.norm(lrel))
    drag_imp = np.zeros(3)
    if rl * rl > 1.0e-12:
        d = np.abs(lrel) / rl
        s = shape.size
        area = frac * (d[0] * s[1] * s[2] + d[1] * s[0] * s[2] + d[2] * s[0] * s[1])
        dv = 0.5 * rho * rl * rl * (0.0 if zero_lin_drag else LINEAR_DRAG) * area * dt * inv_mass
        if dv > rl:
            dv, res.lin_clamped = rl, True                         # drag stops the body in the water at the most
        drag_imp = rel * (dv / rl) * mass
    inv_I = R @ np.diag(1.0 / (shape.unit_mass_inertia * mass)) @ R.T
    length = float(np.sum(shape.size)) / 3.0
    ddrag = inv_I @ (-ANGULAR_DRAG * frac * dt * length * length * mass * w)
    if np.dot(ddrag, ddrag) > np.dot(w, w):
        ddrag, res.ang_clamped = -w, True                          # nor does it turn it round
    res.volume, res.underwater, res.fraction, res.cob = sub, True, frac, rc
    res.fully_submerged = bool(pos[2] + hi <= water_z)
    res.dlin = (drag_imp + buoy_imp) * inv_mass
    res.dang = ddrag + inv_I @ np.cross(rc, buoy_imp + drag_imp)
    return res
