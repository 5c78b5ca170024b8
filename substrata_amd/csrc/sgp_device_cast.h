// sgp_device_cast.h -- gfx950 shape casts: conservative advancement of ONE (moving shape, resting body or triangle) pair over the pairwise separation
// functions of sgp_device_collide.h / sgp_device_hull.h (device code only; the kernels that deal pairs to lanes: sgp_k_shapecast.hip; the contract:
// docs/CONTRACT.md 4f).  Included after sgp_device_collide.h.
#pragma once
#include "../../include/sgp.h"       // SGP_CAST_TOLERANCE
#include "sgp_device_collide.h"

#define SC_MAX_ITERS 32

struct ScHit { float t; uint32_t tri, mat; v3 n, p; float pen; };

// separation along the normal of a finished manifold (at most four points): the deepest point's, and which point that is
SGP_DEV float sc_manifold_sep(const sgd_manifold& m, int* which)
{
	float s = 3.4e38f; int w = 0;
#pragma unroll
	for (int i = 0; i < 4; ++i) if (i < m.np) { const float di = v3_dot(v3_sub(m.p2[i], m.p1[i]), m.n); if (di < s) { s = di; w = i; } }
	*which = w;
	return s;
}
SGP_DEV v3 sc_manifold_p1(const sgd_manifold& m, int w) { return w == 0 ? m.p1[0] : (w == 1 ? m.p1[1] : (w == 2 ? m.p1[2] : m.p1[3])); }
// how far X reaches from its centre against the direction n (the fallback for `point` when no manifold can be had at the touch)
SGP_DEV float sc_extent(const sgd_shape& X, v3 n)
{
	if (X.type == SGD_SHAPE_SPHERE) return X.p0;
	if (X.type == SGD_SHAPE_CAPSULE) return X.p0 + fabsf(v3_dot(n, m33_col(X.R, 2))) * X.p1;
	const sgd_hview hv = sgd_hull_view(&X);
	return v3_dot(n, X.pos) - sgd_hv_proj_min(&hv, n);
}

// The 15 separating axes of two boxes -- the search of sgd_box_box before its clip -- with the largest separation and ITS axis (A -> B) as the result: what the
// advancement needs, where the manifold of sgd_box_box can come back empty (a face axis whose incident face does not lie over the reference face).  An edge
// axis is normalised first and both boxes are then projected on the vector that came out: a valid separation along a valid direction however nearly parallel the
// two edges are (the closed form divides a rounded difference by the sine of their angle).  0: some axis separates the boxes by more than max_sep.
SGP_DEV int sc_box_box_axis(const sgd_shape* A, const sgd_shape* B, float max_sep, float* s_out, v3* n_out)
{
	const v3 hA = V3(A->p0, A->p1, A->p2), hB = V3(B->p0, B->p1, B->p2);
	const v3 T = v3_sub(B->pos, A->pos);
	float best = -3.4e38f; v3 bn = V3(0.0f, 0.0f, 1.0f);
#pragma unroll
	for (int side = 0; side < 2; ++side) {
		const sgd_shape* X = side ? B : A; const sgd_shape* Y = side ? A : B;
		const v3 hX = side ? hB : hA, hY = side ? hA : hB;
#pragma unroll
		for (int i = 0; i < 3; ++i) {
			const v3 ax = m33_col(X->R, i);
			const float tp = v3_dot(T, ax);
			const float s = fabsf(tp) - (v3_get(hX, i) + (hY.x * fabsf(v3_dot(ax, m33_col(Y->R, 0))) + hY.y * fabsf(v3_dot(ax, m33_col(Y->R, 1))) + hY.z * fabsf(v3_dot(ax, m33_col(Y->R, 2)))));
			if (s > max_sep) return 0;
			if (s > best) { best = s; bn = tp < 0.0f ? v3_neg(ax) : ax; }
		}
	}
#pragma unroll
	for (int i = 0; i < 3; ++i) {
#pragma unroll
		for (int j = 0; j < 3; ++j) {
			v3 ax = v3_cross(m33_col(A->R, i), m33_col(B->R, j));
			const float l2 = v3_len_sq(ax);
			if (l2 < 1.0e-8f) continue;
			ax = v3_scale(ax, 1.0f / sqrtf(l2));
			const float tp = v3_dot(T, ax);
			const float ra = hA.x * fabsf(v3_dot(ax, m33_col(A->R, 0))) + hA.y * fabsf(v3_dot(ax, m33_col(A->R, 1))) + hA.z * fabsf(v3_dot(ax, m33_col(A->R, 2)));
			const float rb = hB.x * fabsf(v3_dot(ax, m33_col(B->R, 0))) + hB.y * fabsf(v3_dot(ax, m33_col(B->R, 1))) + hB.z * fabsf(v3_dot(ax, m33_col(B->R, 2)));
			const float s = fabsf(tp) - (ra + rb);
			if (s > max_sep) return 0;
			if (s > best) { best = s; bn = tp < 0.0f ? v3_neg(ax) : ax; }
		}
	}
	*s_out = best; *n_out = bn;
	return 1;
}
// the deepest axis of a separating-axis search over two polytopes (A -> B), faces before edges on equal separation
template <class HA, class HB> SGP_DEV void sc_sat_axis(const HA* A, const HB* B, const sgd_hull_sat& r, float* s_out, v3* n_out)
{
	if (r.eA >= 0 && r.sE > fmaxf(r.sA, r.sB)) { *s_out = r.sE; *n_out = r.nE; }
	else if (r.sA >= r.sB) { *s_out = r.sA; *n_out = sgd_hv_normal(A, r.fA); }
	else { *s_out = r.sB; *n_out = v3_neg(sgd_hv_normal(B, r.fB)); }
}

// The separation along the normal that a step aims for, c = -n . dir being the rate at which the motion closes it: half the tolerance ALONG THE PATH (so the
// reported t is about tolerance / 2 short of the touch however obliquely the surface is met, where half the tolerance along the normal would be tolerance / 2c
// short), but no less than 1e-5 m -- ten times what rounding does to a separation between shapes metres from the origin.  A pair is a hit once its separation is
// at most twice that: never more than the tolerance, and the landing point sits in the middle of what is accepted.
SGP_DEV float sc_landing(float c) { return fmaxf(0.5f * SGP_CAST_TOLERANCE * fminf(c, 1.0f), 1.0e-5f); }

// One (cast, body or triangle) pair.  axis(pos, max_sep, &s, &n): 0 = separated by more than max_sep, 1 = the separation s along n (body -> shape) of the shape
// at pos, 2 = this pair has no axis search of its own, ask the manifold.  manifold(pos, max_sep, &m): the pairwise function (normal body -> shape, p1 on the body).
// ONE call site of each, whatever the pair: the manifold is a true distance for the pairs that advance on it (2) and gives `point` and `penetration` at the
// final t for the others.  limit: the travel allowed (max_t, or less where the caller already holds a hit that close).
// Returns 0 = miss, 1 = hit (h filled in), 2 = hit at the iteration cap.
template <class AX, class MF> SGP_DEV int sc_advance(const sgd_shape& X, v3 dir, float limit, AX axis, MF manifold, ScHit& h)
{
	float t = 0.0f;
	for (int it = 0; it <= SC_MAX_ITERS; ++it) {
		const v3 pos = v3_add(X.pos, v3_scale(dir, t));
		float s = 0.0f; v3 n = V3(0.0f, 0.0f, 0.0f);
		const int a = axis(pos, (limit - t) + SGP_CAST_TOLERANCE, &s, &n);
		if (a == 0) return 0;
		sgd_manifold m; m.np = 0;
		bool ok = false; int w = 0; float sm = 0.0f;
		// (the final t of a pair with an axis search of its own is known before the manifold is asked: s against the landing separation below)
		float land = sc_landing(-v3_dot(n, dir));
		bool done = a == 1 && (s <= 2.0f * land || it == SC_MAX_ITERS);
		if (a == 2 || done) {
			ok = manifold(pos, a == 2 ? (limit - t) + SGP_CAST_TOLERANCE : 4.0f * SGP_CAST_TOLERANCE, &m) && m.np > 0;
			if (ok) sm = sc_manifold_sep(m, &w);
			if (a == 2) {
				if (!ok) return 0;
				s = sm; n = m.n;
				land = sc_landing(-v3_dot(n, dir));
				done = s <= 2.0f * land || it == SC_MAX_ITERS;
			}
		}
		if (done) {
			h.t = t; h.n = n; h.pen = 0.0f;
			if (ok) {
				h.p = sc_manifold_p1(m, w);
				if (t == 0.0f && sm < 0.0f) { h.n = m.n; h.pen = -sm; }      // starts overlapping: the contact sgp_collide_shapes reports here
			} else {
				sgd_shape Y = X; Y.pos = pos;
				h.p = v3_sub(pos, v3_scale(n, sc_extent(Y, n) + s));
			}
			return s <= 2.0f * land ? 1 : 2;
		}
		const float c = -v3_dot(n, dir);
		if (!(c > 0.0f)) return 0;
		t += (s - land) / c;
		if (!(t <= limit)) return 0;
	}
	return 0;
}

