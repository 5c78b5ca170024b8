// sgp_k_shapequery.hip -- A7 -- overlap queries with a sphere, box, capsule or convex hull (sgp_collide_shapes; JPH::NarrowPhaseQuery::CollideShape).
// One of the stage files of the step kernels (stage map: sgp_kernels.h).  Kernels first, their launch wrappers at the end.
//
// Two organisations, one answer.  A WAVE PER QUERY (k_sq_wave: k_collide_capsules with the query shape built from sgp_shape_query) for the one or few
// volumes somebody waits for, and for a volume with hundreds of candidates: the candidates are dealt to the 64 lanes.  CANDIDATE PAIRS for thousands of
// small volumes that touch a handful of bodies each (60 of a wave's 64 lanes would idle): k_sq_candidates, a thread per query, walks the broad-phase
// structures under the query's bounds and appends (query, body) to one of three lists; then a thread per pair (k_sq_pairs_prim: sphere / box / capsule on
// both sides, nothing of the hull search in it; k_sq_pairs_hull: a convex hull on either side) and a wave per pair whose body is a mesh (k_sq_mesh, which
// the wave-per-query organisation uses too).  Every record is a function of its (query, body) pair alone -- the same device functions collide it in either
// organisation -- and the host sorts the records by (query, body, point): the answer depends neither on the organisation nor on the order of the atomics.
// Nothing here drops silently: a list or the output that is too small is counted past its capacity, and the host runs the call again with more room.
#include "sgp_dev_all.h"

// one (body j, query shape X) pair of convex shapes: the manifold with its normal from the body to the query shape
// (clip: the lane's two polygon columns of the box - box clip, sgd_box_box<true>)
SGP_DEV bool sq_collide_prim(const DV& d, const sgd_shape& X, float max_sep, uint32_t j, uint32_t f, float* clip, sgd_manifold* m)
{
	const sgd_shape sb = load_shape(d, j, f);
	return sgd_collide<true>(&sb, &X, max_sep, m, clip) != 0;
}
SGP_DEV bool sq_collide_hull(const DV& d, const sgd_shape& X, float max_sep, uint32_t j, uint32_t f, sgd_manifold* m)
{
	const sgd_shape sb = load_shape(d, j, f);
	return sgd_collide_hull(&sb, &X, max_sep, m) != 0;
}

// how many records manifold g of a (query, body) pair gives, and the records (contact_record: the capsule query's) from slot `base` on
SGP_DEV int sq_num_records(const sgp_shape_query& q, int g, const sgd_manifold& m)
{
	if (q.flags & SGP_QUERY_DEEPEST_ONLY) return (g == 0 && m.np > 0) ? 1 : 0;
	return m.np;
}
SGP_DEV void sq_emit_at(const DV& d, const SqBufs& b, const sgp_shape_query& q, uint32_t k, uint32_t j, uint32_t f, int g, const sgd_manifold& m, uint32_t base)
{
	if (q.flags & SGP_QUERY_DEEPEST_ONLY) {
		if (g != 0 || m.np <= 0) return;
		int best = 0; float bd = v3_dot(v3_sub(m.p2[0], m.p1[0]), m.n);
#pragma unroll
		for (int i = 1; i < 4; ++i) if (i < m.np) { const float di = v3_dot(v3_sub(m.p2[i], m.p1[i]), m.n); if (di < bd) { bd = di; best = i; } }      // (ties: the lower point index)
		if (base < b.cap) {
#pragma unroll
			for (int i = 0; i < 4; ++i) if (i == best) b.out[base] = contact_record(d, k, j, f, g, m, i);      // (static slots: the manifold stays in registers)
		}
		return;
	}
#pragma unroll
	for (int i = 0; i < 4; ++i) if (i < m.np && base + (uint32_t)i < b.cap) b.out[base + (uint32_t)i] = contact_record(d, k, j, f, g, m, i);
}
// ... with the slots taken by this lane alone (divergent callers)
SGP_DEV void sq_emit(const DV& d, const SqBufs& b, const sgp_shape_query& q, uint32_t k, uint32_t j, uint32_t f, int g, const sgd_manifold& m)
{
	const int nr = sq_num_records(q, g, m);
	if (nr > 0) sq_emit_at(d, b, q, k, j, f, g, m, atomicAdd(&b.ctr[SQ_N_OUT], (uint32_t)nr));
}
// Slots for every lane of a wave with ONE atomic (whole wave: every lane calls this, nr = 0 for a lane with nothing to write)
SGP_DEV uint32_t sq_wave_slots(uint32_t* counter, int nr)
{
	const int lane = (int)(threadIdx.x & 63u);
	int incl = nr;
#pragma unroll
	for (int off = 1; off < 64; off <<= 1) { const int o = __shfl_up(incl, off, 64); if (lane >= off) incl += o; }
	const int total = __shfl(incl, 63, 64);
	uint32_t base = 0;
	if (lane == 0 && total > 0) base = atomicAdd(counter, (uint32_t)total);
	base = (uint32_t)__shfl((int)base, 0, 64);
	return base + (uint32_t)(incl - nr);
}

// ---------------------------------------------------------------------------------------------------------------
// a wave per query

__global__ void __launch_bounds__(64) k_sq_wave(DV d, SqBufs b)
{
	__shared__ float s_clip[2 * SGD_LPOLY_FLOATS];
	const uint32_t lane = threadIdx.x;
	for (uint32_t k = blockIdx.x; k < b.n; k += gridDim.x) {
		const sgp_shape_query q = b.qs[k];
		sgd_shape X; v3 lo, hi;
		sq_shape<true>(d, q, X, lo, hi);
		sq_walk<64>(d, lo, hi, lane, [&](uint32_t j) {
			uint32_t f;
			if (!sq_passes(d, q, lo, hi, j, &f)) return;
			const uint32_t st = f_shape(f);
			if (st == SGP_SHAPE_MESH) { pair_append(b.lists, &b.ctr[SQ_N_MESH], b.lists.mesh, k, j); return; }      // (its triangles are a whole wave's work: k_sq_mesh)
			sgd_manifold m;
			const bool hit = (st == SGP_SHAPE_HULL || q.shape_type == SGP_SHAPE_HULL) ? sq_collide_hull(d, X, q.max_separation, j, f, &m) : sq_collide_prim(d, X, q.max_separation, j, f, &s_clip[lane], &m);
			if (hit) sq_emit(d, b, q, k, j, f, 0, m);
		});
	}
}

// ---------------------------------------------------------------------------------------------------------------
// candidate pairs: a thread per query finds them ...

__global__ void __launch_bounds__(64) k_sq_candidates(DV d, SqBufs b)
{
	const uint32_t k = blockIdx.x * 64 + threadIdx.x;
	if (k >= b.n) return;
	const sgp_shape_query q = b.qs[k];
	sgd_shape X; v3 lo, hi;
	sq_shape<true>(d, q, X, lo, hi);
	sq_walk<1>(d, lo, hi, 0u, [&](uint32_t j) {
		uint32_t f;
		if (!sq_passes(d, q, lo, hi, j, &f)) return;
		const uint32_t st = f_shape(f);
		if (st == SGP_SHAPE_MESH) pair_append(b.lists, &b.ctr[SQ_N_MESH], b.lists.mesh, k, j);
		else if (st == SGP_SHAPE_HULL || q.shape_type == SGP_SHAPE_HULL) pair_append(b.lists, &b.ctr[SQ_N_HULL], b.lists.hull, k, j);
		else pair_append(b.lists, &b.ctr[SQ_N_PRIM], b.lists.prim, k, j);
	});
}

// ... a thread per pair collides them: spheres, boxes and capsules on both sides (the box - box clip polygons in LDS: no scratch) ...
__global__ void __launch_bounds__(64) k_sq_pairs_prim(DV d, SqBufs b)
{
	__shared__ float s_clip[2 * SGD_LPOLY_FLOATS];
	const uint32_t n = min(b.ctr[SQ_N_PRIM], b.lists.pcap);
	const uint32_t lane = threadIdx.x;
	for (uint32_t p0 = blockIdx.x * 64u; p0 < n; p0 += gridDim.x * 64u) {
		const uint32_t p = p0 + lane;
		sgd_manifold m; m.np = 0;
		uint2 kj = make_uint2(0u, 0u); uint32_t f = 0; int nr = 0;
		sgp_shape_query q;
		if (p < n) {
			kj = b.lists.prim[p];
			q = b.qs[kj.x];
			sgd_shape X; v3 lo, hi;
			sq_shape<false>(d, q, X, lo, hi);
			f = d.flags[kj.y];
			if (sq_collide_prim(d, X, q.max_separation, kj.y, f, &s_clip[lane], &m)) nr = sq_num_records(q, 0, m);
		}
		const uint32_t base = sq_wave_slots(&b.ctr[SQ_N_OUT], nr);
		if (nr > 0) sq_emit_at(d, b, q, kj.x, kj.y, f, 0, m, base);
	}
}
// ... and the pairs with a convex hull on either side (the sequential separating-axis search: its clip buffers and long loops stay out of the kernel above)
__global__ void __launch_bounds__(64) k_sq_pairs_hull(DV d, SqBufs b)
{
	const uint32_t n = min(b.ctr[SQ_N_HULL], b.lists.pcap);
	for (uint32_t p = blockIdx.x * 64u + threadIdx.x; p < n; p += gridDim.x * 64u) {
		const uint2 kj = b.lists.hull[p];
		const sgp_shape_query q = b.qs[kj.x];
		sgd_shape X; v3 lo, hi;
		sq_shape<false>(d, q, X, lo, hi);
		const uint32_t f = d.flags[kj.y];
		sgd_manifold m;
		if (sq_collide_hull(d, X, q.max_separation, kj.y, f, &m)) sq_emit(d, b, q, kj.x, kj.y, f, 0, m);
	}
}

// ---------------------------------------------------------------------------------------------------------------
// (query, mesh body) pairs of either organisation: a wave per pair, 64 candidate triangles per round (mesh_pair_groups, as k_collide_capsules takes them)

__global__ void __launch_bounds__(64) k_sq_mesh(DV d, SqBufs b)
{
	__shared__ MeshPairLds<64> L;
	const uint32_t n = min(b.ctr[SQ_N_MESH], b.lists.pcap);
	const uint32_t lane = threadIdx.x;
	for (uint32_t p = blockIdx.x; p < n; p += gridDim.x) {
		const uint2 kj = b.lists.mesh[p];
		const sgp_shape_query q = b.qs[kj.x];
		const uint32_t mid = kj.y;
		sgd_shape X; v3 lo, hi;
		sq_shape<true>(d, q, X, lo, hi);
		const v3 es = V3(q.max_separation, q.max_separation, q.max_separation);
		const v3 mv = V3(q.movement[0], q.movement[1], q.movement[2]);
		bool valid = true, dropped = false;
		// (a capsule: the instance k_collide_capsules uses, nothing of the polytope search in it)
		if (q.shape_type == SGP_SHAPE_CAPSULE) mesh_pair_groups<64, 4>(d, L, valid, X, mid, v3_sub(lo, es), v3_add(hi, es), q.max_separation, 0, (int)lane, 0u, dropped, mv, q.active_edges != 0u);
		else mesh_pair_groups<64, SGD_KINDS_ALL>(d, L, valid, X, mid, v3_sub(lo, es), v3_add(hi, es), q.max_separation, 0, (int)lane, 0u, dropped, mv, q.active_edges != 0u);
		if ((int)lane < L.mc.ng) {
			const sgd_mesh_group& grp = L.mc.g[lane];
			sgd_manifold mm;
			sgd_hull_reduce(grp.n, grp.p_mesh, grp.p_body, grp.np, &mm);
			sq_emit(d, b, q, kj.x, mid, d.flags[mid], (int)lane, mm);
		}
		__syncthreads();          // (the tables are reused by the next pair)
	}
}

// ---------------------------------------------------------------------------------------------------------------
// launch wrappers (the grids of the list kernels: list_blocks, sgp_kernels.h)

void launch_shape_queries_wave(const DV& d, const SqBufs& b, hipStream_t s)
{
	if (!b.n) return;
	hipLaunchKernelGGL(k_sq_wave, dim3(std::min(b.n, 65536u)), dim3(64), 0, s, d, b);
	hipLaunchKernelGGL(k_sq_mesh, dim3(list_blocks(std::min(b.lists.pcap, 4u * b.n), 1u, 4096u)), dim3(64), 0, s, d, b);
}
void launch_shape_queries_pairs(const DV& d, const SqBufs& b, hipStream_t s)
{
	if (!b.n) return;
	hipLaunchKernelGGL(k_sq_candidates, dim3((b.n + 63u) / 64u), dim3(64), 0, s, d, b);
	hipLaunchKernelGGL(k_sq_pairs_prim, dim3(list_blocks(b.lists.pcap, 64u, 4096u)), dim3(64), 0, s, d, b);
	hipLaunchKernelGGL(k_sq_pairs_hull, dim3(list_blocks(b.lists.pcap, 64u, 4096u)), dim3(64), 0, s, d, b);
	hipLaunchKernelGGL(k_sq_mesh, dim3(list_blocks(std::min(b.lists.pcap, 4u * b.n), 1u, 4096u)), dim3(64), 0, s, d, b);
}
