// sgp_k_shapecast.hip -- A7 -- shape casts with a sphere, box, capsule or convex hull (sgp_cast_shapes; JPH::NarrowPhaseQuery::CastShape).
// One of the stage files of the step kernels (stage map: sgp_kernels.h).  Kernels first, their launch wrapper at the end.
//
// The sweep is CONSERVATIVE ADVANCEMENT over the pairwise separation functions the library already has.  At parameter t the shape at pos + t dir is collided
// with the body with a maximum separation of the travel left (plus the tolerance); that gives a separating normal n (body -> shape) and the separation s along
// it.  No answer: miss.  s within the landing band (sc_landing: at most the tolerance): hit at t.  n . dir >= 0: miss -- a separating axis the motion does not
// close stays one under pure translation.  Otherwise t += (s - landing separation) / (-n . dir).  ANY valid separating axis makes the step safe, so the deepest axis of a separating-axis search serves as well
// as a true distance, and polytope pairs end after a few steps; pairs with a rounded shape at an edge or corner converge geometrically and are capped
// (SC_MAX_ITERS; a pair that gets there reports the t it reached -- never past the true hit -- and is counted).
//
// Organisation: that of sgp_k_shapequery.hip's candidate pairs.  A wave per cast walks the broad-phase structures under the SWEPT bounds (the union of the shape's
// bounds at 0 and at max_t) and deals the bodies to three lists; a thread per pair advances sphere / box / capsule pairs (box - box clip polygons of the final
// manifold in LDS) and, in a kernel of their own, pairs with a convex hull on either side; a wave per (cast, mesh or height field) pair culls the triangles with
// the swept bounds, a lane advances the shape against a triangle, and the wave keeps the least (t, triangle).  Every pair that hits appends one record; the host
// keeps per cast the least by (t, id, triangle).  Nothing drops silently: a list that is too small is counted past its capacity and the call runs again.
#include "sgp_dev_all.h"
#include "sgp_device_cast.h"

#define SC_TRI_CHUNK 512      // candidate triangles of a mesh tree the wave takes per round of its walk

// the cast's shape as an overlap query at t = 0 (the record sq_shape and sq_passes read)
SGP_DEV sgp_shape_query sc_as_query(const sgp_shape_cast& c)
{
	sgp_shape_query q;
	q.pos[0] = c.pos[0]; q.pos[1] = c.pos[1]; q.pos[2] = c.pos[2]; q.movement[0] = q.movement[1] = q.movement[2] = 0.0f;
	q.rot[0] = c.rot[0]; q.rot[1] = c.rot[1]; q.rot[2] = c.rot[2]; q.rot[3] = c.rot[3];
	q.shape[0] = c.shape[0]; q.shape[1] = c.shape[1]; q.shape[2] = c.shape[2]; q.shape[3] = c.shape[3];
	q.shape_type = c.shape_type; q.max_separation = 2.0f * SGP_CAST_TOLERANCE; q.ignore_id = c.ignore_id; q.layer_mask = c.layer_mask; q.flags = 0u; q.active_edges = 0u;
	return q;
}
// [lo, hi] at t = 0 -> the bounds of the whole sweep (a little generous: the end point is rounded)
SGP_DEV void sc_swept(const sgp_shape_cast& c, v3& lo, v3& hi)
{
	const v3 mv = v3_scale(V3(c.dir[0], c.dir[1], c.dir[2]), c.max_t);
	const float g = 1.0e-6f * (c.max_t + fabsf(c.pos[0]) + fabsf(c.pos[1]) + fabsf(c.pos[2]));
	lo = v3_sub(v3_min(lo, v3_add(lo, mv)), V3(g, g, g)); hi = v3_add(v3_max(hi, v3_add(hi, mv)), V3(g, g, g));
}
SGP_DEV void sc_emit(const ScBufs& b, uint32_t k, uint32_t j, const ScHit& h, int rc)
{
	if (rc == 2) atomicAdd(&b.ctr[SC_N_CAPPED], 1u);
	sgp_cast_hit o;
	o.id = j; o.t = h.t;
	o.normal[0] = h.n.x; o.normal[1] = h.n.y; o.normal[2] = h.n.z;
	o.point[0] = h.p.x; o.point[1] = h.p.y; o.point[2] = h.p.z;
	o.penetration = h.pen; o.sub_shape = 0u; o.triangle = h.tri; o.material = h.mat; o.userdata = (uint64_t)k;      // (the cast's index: the host keeps the least record per cast)
	b.out[atomicAdd(&b.ctr[SC_N_OUT], 1u)] = o;      // (a record per pair at most: `out` holds 3 pcap)
}

// ---------------------------------------------------------------------------------------------------------------
// a wave per cast finds the candidates under the swept bounds ...

__global__ void __launch_bounds__(64) k_sc_candidates(DV d, ScBufs b)
{
	const uint32_t lane = threadIdx.x;
	for (uint32_t k = blockIdx.x; k < b.n; k += gridDim.x) {
		const sgp_shape_cast c = b.cs[k];
		const sgp_shape_query q = sc_as_query(c);
		sgd_shape X; v3 lo, hi;
		sq_shape<true>(d, q, X, lo, hi);
		sc_swept(c, lo, hi);
		sq_walk<64>(d, lo, hi, lane, [&](uint32_t j) {
			uint32_t f;
			if (!sq_passes(d, q, lo, hi, j, &f) || (f & BF_SENSOR)) return;      // (sensors never answer a cast, as for rays and sphere casts)
			const uint32_t st = f_shape(f);
			if (st == SGP_SHAPE_MESH) pair_append(b.lists, &b.ctr[SC_N_MESH], b.lists.mesh, k, j);
			else if (st == SGP_SHAPE_HULL || c.shape_type == SGP_SHAPE_HULL) pair_append(b.lists, &b.ctr[SC_N_HULL], b.lists.hull, k, j);
			else pair_append(b.lists, &b.ctr[SC_N_PRIM], b.lists.prim, k, j);
		});
	}
}

// ... a thread per pair advances them: spheres, boxes and capsules on both sides (the clip polygons of the box - box manifold at the final t in LDS: no scratch) ...
__global__ void __launch_bounds__(64) k_sc_pairs_prim(DV d, ScBufs b)
{
	__shared__ float s_clip[2 * SGD_LPOLY_FLOATS];
	const uint32_t n = min(b.ctr[SC_N_PRIM], b.lists.pcap);
	float* clip = &s_clip[threadIdx.x];
	for (uint32_t p = blockIdx.x * 64u + threadIdx.x; p < n; p += gridDim.x * 64u) {
		const uint2 kj = b.lists.prim[p];
		const sgp_shape_cast c = b.cs[kj.x];
		const sgp_shape_query q = sc_as_query(c);
		sgd_shape X; v3 lo, hi;
		sq_shape<false>(d, q, X, lo, hi);
		const sgd_shape sb = load_shape(d, kj.y, d.flags[kj.y]);
		const bool boxes = sb.type == SGD_SHAPE_BOX && X.type == SGD_SHAPE_BOX;
		sgd_shape Y = X;
		ScHit h; h.tri = SGP_INVALID_ID; h.mat = 0u;
		const int rc = sc_advance(X, V3(c.dir[0], c.dir[1], c.dir[2]), c.max_t,
			[&](v3 pos, float max_sep, float* s, v3* nn) { if (!boxes) return 2; Y.pos = pos; return sc_box_box_axis(&sb, &Y, max_sep, s, nn); },
			[&](v3 pos, float max_sep, sgd_manifold* m) { Y.pos = pos; return sgd_collide<true>(&sb, &Y, max_sep, m, clip) != 0; }, h);
		if (rc) sc_emit(b, kj.x, kj.y, h, rc);
	}
}
// ... and the pairs with a convex hull on either side (the sequential separating-axis search: its long loops and clip buffers stay out of the kernel above)
__global__ void __launch_bounds__(64) k_sc_pairs_hull(DV d, ScBufs b)
{
	const uint32_t n = min(b.ctr[SC_N_HULL], b.lists.pcap);
	for (uint32_t p = blockIdx.x * 64u + threadIdx.x; p < n; p += gridDim.x * 64u) {
		const uint2 kj = b.lists.hull[p];
		const sgp_shape_cast c = b.cs[kj.x];
		const sgp_shape_query q = sc_as_query(c);
		sgd_shape X; v3 lo, hi;
		sq_shape<false>(d, q, X, lo, hi);
		const sgd_shape sb = load_shape(d, kj.y, d.flags[kj.y]);
		const bool polytopes = (sb.type == SGD_SHAPE_BOX || sb.type == SGD_SHAPE_HULL) && (X.type == SGD_SHAPE_BOX || X.type == SGD_SHAPE_HULL);
		sgd_shape Y = X;
		ScHit h; h.tri = SGP_INVALID_ID; h.mat = 0u;
		const int rc = sc_advance(X, V3(c.dir[0], c.dir[1], c.dir[2]), c.max_t,
			[&](v3 pos, float max_sep, float* s, v3* nn) {
				if (!polytopes) return 2;      // (a sphere or capsule against a hull: sgd_hull_sphere / sgd_hull_capsule are true distances)
				Y.pos = pos;
				const sgd_hview ha = sgd_hull_view(&sb), hb = sgd_hull_view(&Y);
				sgd_hull_sat r;
				if (!sgd_hull_sat_search(&ha, &hb, max_sep, &r)) return 0;
				sc_sat_axis(&ha, &hb, r, s, nn);
				return 1; },
			[&](v3 pos, float max_sep, sgd_manifold* m) { Y.pos = pos; return sgd_collide_hull(&sb, &Y, max_sep, m) != 0; }, h);
		if (rc) sc_emit(b, kj.x, kj.y, h, rc);
	}
}

// ---------------------------------------------------------------------------------------------------------------
// (cast, mesh or height field) pairs: a wave per pair.  The triangles under the swept bounds -- a mesh: lane 0 walks the tree and hands the wave SC_TRI_CHUNK
// candidates at a time, as often as it takes; a height field: the quads under the bounds, blocks whose height range misses them skipped -- are dealt to the lanes,
// a lane advances the shape against its triangle (front side only, every edge with its own normal), and the wave keeps the least (t, triangle index).

struct ScMeshLds { uint32_t tri[SC_TRI_CHUNK]; uint32_t stack[48]; int sp; uint32_t n; uint32_t deep; };

__global__ void __launch_bounds__(64) k_sc_mesh(DV d, ScBufs b)
{
	__shared__ float s_lpoly[3 * SGD_LPOLY_FLOATS];
	__shared__ ScMeshLds L;
	const uint32_t n = min(b.ctr[SC_N_MESH], b.lists.pcap);
	const uint32_t lane = threadIdx.x;
	const sgd_box_code box_code = sgd_box_code_of(&d.hulls[0]);
	for (uint32_t p = blockIdx.x; p < n; p += gridDim.x) {
		const uint2 kj = b.lists.mesh[p];
		const uint32_t mid = kj.y;
		const sgp_shape_cast c = b.cs[kj.x];
		const sgp_shape_query q = sc_as_query(c);
		const v3 dir = V3(c.dir[0], c.dir[1], c.dir[2]);
		sgd_shape X; v3 lo, hi;
		sq_shape<true>(d, q, X, lo, hi);
		sc_swept(c, lo, hi);
		const MeshHeader mh = d.meshes[(uint32_t)d.pose[POSE_F4 * (size_t)mid + 3].x];
		const v3 mpos = V3(d.pose[POSE_F4 * (size_t)mid]); const m33 R = quat_to_m33(Q4(d.pose[POSE_F4 * (size_t)mid + 1]));
		// the swept bounds in the mesh frame: bounds of the box's 8 corners, a little generous (mesh_pair_groups)
		v3 llo = V3(3.4e38f, 3.4e38f, 3.4e38f), lhi = V3(-3.4e38f, -3.4e38f, -3.4e38f);
		for (int i = 0; i < 8; ++i) {
			const v3 cw = V3((i & 1) ? hi.x : lo.x, (i & 2) ? hi.y : lo.y, (i & 4) ? hi.z : lo.z);
			const v3 l = m33_tmul(R, v3_sub(cw, mpos));
			llo = v3_min(llo, l); lhi = v3_max(lhi, l);
		}
		const float pad = 1.0e-4f * (1.0f + fabsf(llo.x) + fabsf(llo.y) + fabsf(llo.z) + fabsf(lhi.x) + fabsf(lhi.y) + fabsf(lhi.z));
		llo = v3_sub(llo, V3(pad, pad, pad)); lhi = v3_add(lhi, V3(pad, pad, pad));

		ScHit best; best.t = 3.4e38f; best.tri = SGP_INVALID_ID; best.mat = 0u; best.n = V3(0.0f, 0.0f, 0.0f); best.p = best.n; best.pen = 0.0f;
		int best_rc = 0;
		sgd_shape Y = X;
		auto test = [&](uint32_t pos_in_mesh) {
			const MeshTri tr = mesh_tri(d, mh, pos_in_mesh);
			if (!mesh_tri_overlaps(tr, llo, lhi)) return;
			sgd_tri_hull_t th; v3 cen, nrm;
			sgd_tri_hull(tr.a, tr.b, tr.c, &th, &cen, &nrm);
			sgd_tri_view T; T.pos = v3_add(mpos, m33_mul(R, cen)); T.R = R; T.scale = V3(1.0f, 1.0f, 1.0f); T.h = &th;
			const v3 nt = m33_mul(R, nrm);
			ScHit h; h.tri = tr.index; h.mat = tr.mat;
			// (during the approach any separating axis serves, whichever side of the triangle it leaves: the front-side rule is asked of the normal AT THE TOUCH, below)
			int rc = sc_advance(X, dir, best_rc ? best.t : c.max_t,
				[&](v3 pos, float max_sep, float* s, v3* nn) {
					Y.pos = pos;
					if (X.type == SGD_SHAPE_SPHERE || X.type == SGD_SHAPE_CAPSULE) {      // (sgd_hull_sphere / sgd_hull_capsule against the thin hull: true distances)
						sgd_manifold m; int hit;
						if (X.type == SGD_SHAPE_SPHERE) hit = sgd_hull_sphere(&T, pos, X.p0, max_sep, &m);
						else { const v3 ax = v3_scale(m33_col(X.R, 2), X.p1); hit = sgd_hull_capsule(&T, v3_sub(pos, ax), v3_add(pos, ax), X.p0, max_sep, &m); }
						if (!hit) return 0;
						int w; *s = sc_manifold_sep(m, &w); *nn = m.n;
						return 1;
					}
					const sgd_hview hx = sgd_hull_view(&Y);
					sgd_hull_sat r;
					if (X.type == SGD_SHAPE_BOX) { if (!sgd_tri_box_sat(&T, &hx, box_code, max_sep, &r)) return 0; }
					else if (!sgd_hull_sat_search<false>(&T, &hx, max_sep, &r)) return 0;
					sc_sat_axis(&T, &hx, r, s, nn);
					return 1; },
				[&](v3 pos, float max_sep, sgd_manifold* m) {      // (a box: its clip polygons in LDS, sgd_tri_box_manifold; a hull: the instance without the box's code)
					Y.pos = pos;
					if (X.type == SGD_SHAPE_HULL) return sgd_collide_tri<8>(&Y, &T, nt, max_sep, m, 7u, V3(0.0f, 0.0f, 0.0f)) != 0;
					return sgd_collide_tri<SGD_KINDS_PRIMITIVES>(&Y, &T, nt, max_sep, m, 7u, V3(0.0f, 0.0f, 0.0f), &box_code, s_lpoly + lane) != 0; }, h);
			if (rc && v3_dot(h.n, nt) < 0.0f) rc = 0;      // touched from behind: a triangle answers on its front side only
			if (rc && (!best_rc || h.t < best.t || (h.t == best.t && h.tri < best.tri))) { best = h; best_rc = rc; }
		};

		if (mh.kind == MESH_KIND_FIELD) {
			int x0 = 0, x1 = -1, z0 = 0, z1 = -1;
			if (!(field_quad_span(mh, 0, llo.x, lhi.x, x0, x1) && field_quad_span(mh, 2, llo.z, lhi.z, z0, z1))) { x1 = -1; z1 = -1; }
			const uint32_t nxq = (uint32_t)(x1 - x0 + 1), nq = (x1 >= x0 && z1 >= z0) ? nxq * (uint32_t)(z1 - z0 + 1) : 0u;
			for (uint32_t i = lane; i < nq; i += 64u) {
				const uint32_t x = (uint32_t)x0 + i % nxq, z = (uint32_t)z0 + i / nxq;
				const uint32_t blk = mh.field_off + mh.blk_off + 2u * ((z / FIELD_BLOCK) * mh.nb + (x / FIELD_BLOCK));
				if (__uint_as_float(d.mesh_field[blk + 1u]) < llo.y || __uint_as_float(d.mesh_field[blk]) > lhi.y) continue;
				const uint32_t qd = z * (mh.fw - 1u) + x;
				test(2u * qd); test(2u * qd + 1u);
			}
		} else {
			if (lane == 0) { L.sp = 1; L.stack[0] = 0u; L.deep = 0u; }
			for (;;) {
				__syncthreads();
				if (lane == 0) {
					uint32_t m = 0; int sp = L.sp;
					while (sp > 0) {
						const uint32_t ni = L.stack[sp - 1];
						const MeshNode nd = d.mesh_nodes[mh.node_off + ni];
						if (nd.count != 0 && m + nd.count > (uint32_t)SC_TRI_CHUNK) { if (m == 0) { L.deep = 1u; --sp; } break; }      // (the leaf waits for the next round; one that no round can hold is counted)
						--sp;
						if (nd.mxx < llo.x || nd.mnx > lhi.x || nd.mxy < llo.y || nd.mny > lhi.y || nd.mxz < llo.z || nd.mnz > lhi.z) continue;
						if (nd.count == 0) { if (sp + 2 <= 48) { L.stack[sp++] = nd.left; L.stack[sp++] = nd.right; } else L.deep = 1u; continue; }
						for (uint32_t i = 0; i < nd.count; ++i) L.tri[m++] = nd.left + i;
					}
					L.sp = sp; L.n = m;
				}
				__syncthreads();
				const uint32_t m = L.n; const bool more = L.sp > 0;
				for (uint32_t i = lane; i < m; i += 64u) test(L.tri[i]);
				if (!more) break;
			}
			if (lane == 0 && L.deep) atomicAdd(&b.ctr[SC_N_DROPPED], 1u);
		}
		// the wave's least (t, triangle); the lane that holds it writes the pair's record
		float wt = best_rc ? best.t : 3.4e38f; uint32_t wtri = best_rc ? best.tri : 0xFFFFFFFFu; int who = (int)lane;
#pragma unroll
		for (int off = 32; off >= 1; off >>= 1) {
			const float ot = __shfl_xor(wt, off, 64); const uint32_t otri = (uint32_t)__shfl_xor((int)wtri, off, 64); const int ow = __shfl_xor(who, off, 64);
			if (ot < wt || (ot == wt && (otri < wtri || (otri == wtri && ow < who)))) { wt = ot; wtri = otri; who = ow; }
		}
		if (best_rc && who == (int)lane) sc_emit(b, kj.x, mid, best, best_rc);
		__syncthreads();      // (the tables are reused by the next pair)
	}
}

// ---------------------------------------------------------------------------------------------------------------
// launch wrapper (the grids of the list kernels: list_blocks, sgp_kernels.h)

void launch_shape_casts(const DV& d, const ScBufs& b, hipStream_t s)
{
	if (!b.n) return;
	hipLaunchKernelGGL(k_sc_candidates, dim3(std::min(b.n, 65536u)), dim3(64), 0, s, d, b);
	hipLaunchKernelGGL(k_sc_pairs_prim, dim3(list_blocks(b.lists.pcap, 64u, 4096u)), dim3(64), 0, s, d, b);
	hipLaunchKernelGGL(k_sc_pairs_hull, dim3(list_blocks(b.lists.pcap, 64u, 4096u)), dim3(64), 0, s, d, b);
	hipLaunchKernelGGL(k_sc_mesh, dim3(list_blocks(std::min(b.lists.pcap, 4u * b.n), 1u, 4096u)), dim3(64), 0, s, d, b);
}
