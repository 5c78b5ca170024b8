// sgp_k_queries.hip -- A7 -- rays, the character's capsule queries, sphere casts.
// One of the stage files of the step kernels (stage map: sgp_kernels.h).  Kernels first, their launch wrappers at the end.
#include "sgp_dev_all.h"
#include "sgp_dev_raycast.h"

// traceRay (PhysicsWorld.cpp:1668-1725), batched: one thread per ray (raycast_one, sgp_dev_raycast.h)
__global__ void __launch_bounds__(64) k_raycast(DV d, const sgp_ray* rays, uint32_t n, sgp_hit* hits)
{
	const uint32_t k = blockIdx.x * 64 + threadIdx.x;
	if (k >= n) return;
	hits[k] = raycast_one(d, rays[k]);
}

// doesRayHitAnything (PhysicsWorld.cpp:1668-1725 with the plain CastRay), batched: one thread per ray, one byte per answer (raycast_any_one, sgp_dev_raycast.h)
__global__ void __launch_bounds__(64) k_raycast_any(DV d, const sgp_ray* rays, uint32_t n, uint8_t* hit)
{
	const uint32_t k = blockIdx.x * 64 + threadIdx.x;
	if (k >= n) return;
	hit[k] = raycast_any_one(d, rays[k]) ? (uint8_t)1 : (uint8_t)0;
}

// The same ray by all 64 lanes of a wave together (the resident server's form of raycast_one): the candidates are dealt to the lanes -- the large bodies
// by index, the bodies of the static large bodies' grid in the order it yields them, the nine neighbour rows of a visited cell one row per lane -- and
// every lane keeps its own closest hit.  The answer is the lexicographic minimum of (t, body id) over the lanes: ray_test breaks ties by body id
// precisely so that the result does not depend on the order of the tests, so this is raycast_one's answer bit for bit.  `tmin` (the wave's closest t so
// far, refreshed after every cell) bounds the walk for all lanes alike, which keeps the control flow -- and the dealing -- uniform.
SGP_DEV float wave_min_f(float x) { for (int off = 32; off >= 1; off >>= 1) x = fminf(x, __shfl_xor(x, off, 64)); return x; }
SGP_DEV void ray_share_bound(RayBest& best, float& tmin)
{
	tmin = wave_min_f(best.t);
	if (best.t > tmin) { best.t = tmin; best.id = SGP_INVALID_ID; }      // (somebody is closer: this lane's hit cannot win; it keeps pruning with the wave's bound)
}
// What the resident server keeps of the world between rays (LDS): the server is told to leave before anything touches the world (RayMailbox::stop_gen), so the
// grid headers and the large bodies' records it read when it started are those of every ray it answers.
#define RAY_CACHE_LARGE 16
struct RayServerCache {
	BpGrid g; LargeGrid lg; uint32_t n_large;
	uint32_t id[RAY_CACHE_LARGE], f[RAY_CACHE_LARGE]; float4 amin[RAY_CACHE_LARGE], amax[RAY_CACHE_LARGE], prop1[RAY_CACHE_LARGE], pose0[RAY_CACHE_LARGE], pose1[RAY_CACHE_LARGE];
};
SGP_DEV void ray_cache_fill(const DV& d, RayServerCache& C)
{
	const int lane = (int)(threadIdx.x & 63u);
	if (lane == 0) { C.g = *d.grid; C.lg = *d.lgrid; C.n_large = d.sp->n_large; }
	__syncthreads();
	if (lane < RAY_CACHE_LARGE && (uint32_t)lane < C.n_large) {
		const uint32_t i = d.large_ids[lane];
		C.id[lane] = i; C.f[lane] = d.flags[i]; C.amin[lane] = d.aabb_min[i]; C.amax[lane] = d.aabb_max[i];
		C.prop1[lane] = d.pose[POSE_F4 * (size_t)i + 3]; C.pose0[lane] = d.pose[POSE_F4 * (size_t)i]; C.pose1[lane] = d.pose[POSE_F4 * (size_t)i + 1];
	}
	__syncthreads();
}
#define RAY_WAVE_AHEAD 7      // cells of the walk looked at together: 7 x 9 neighbour rows = 63 lanes
SGP_DEV sgp_hit raycast_wave(const DV& d, const sgp_ray& ry, const RayServerCache& C)
{
	const int lane = (int)(threadIdx.x & 63u);
	const v3 o = V3(ry.origin[0], ry.origin[1], ry.origin[2]), dir = V3(ry.dir[0], ry.dir[1], ry.dir[2]);
	RayBest best = ray_best_none(ry.max_t);
	float tmin = ry.max_t;
	if (C.n_large <= RAY_CACHE_LARGE) { if ((uint32_t)lane < C.n_large) ray_test_loaded(d, ry, o, dir, C.id[lane], C.f[lane], C.amin[lane], C.amax[lane], C.prop1[lane], C.pose0[lane], C.pose1[lane], best); }
	else for (uint32_t l = (uint32_t)lane; l < C.n_large; l += 64u) ray_test_body<false>(d, ry, o, dir, d.large_ids[l], best);
	ray_share_bound(best, tmin);
	if (C.lg.n_items) {
		uint32_t dealt = 0;
		const float bound = tmin;      // (fixed for the walk: every lane walks the same cells and counts the same candidates)
		large_grid_ray(d, o, dir, &bound, [&](uint32_t i) { if ((int)(dealt++ & 63u) == lane) ray_test_body_eager(d, ry, o, dir, i, best); return false; });
		ray_share_bound(best, tmin);
	}
	const BpGrid g = C.g;
	if (g.n_cells > 0 && g.min_x <= g.max_x) {
		const float c = g.cell;
		const v3 lo = V3(g.ox - c, g.oy - c, g.oz - c);
		const v3 hi = V3(g.ox + ((float)g.nx + 1.0f) * c, g.oy + ((float)g.ny + 1.0f) * c, g.oz + ((float)g.nz + 1.0f) * c);
		CellWalk w;
		if (w.start(g, o, dir, lo, hi, tmin)) {
			// The walk, RAY_WAVE_AHEAD cells at a time: the cells of the walk follow from arithmetic alone, so the wave works out the next seven, lane l takes
			// neighbour row l % 9 of cell l / 9 of them, and the fetches of seven cells (page table -> cell table -> body records) are in flight together where the
			// cell-by-cell walk paid them one after the other (a 20 m ray: 23 -> see profiles/NOTES_r05.md section 2).  A cell beyond the one where raycast_one stops
			// can only hold bodies farther than the hit that stopped it (that is what stops it), so looking at it changes nothing.
			const int my_step = lane / 9, row = lane % 9, dy = row % 3 - 1, dz = row / 3 - 1;
			bool done = false;
			for (int iter = 0; iter < 100000 && !done; ++iter) {
				if (w.t_enter - 2.0f * c > tmin) break;
				int mx = 0, my = 0, mz = 0; bool mine = false;
#pragma unroll
				for (int k = 0; k < RAY_WAVE_AHEAD; ++k) {
					if (!done) {
						if (k == my_step && !(w.t_enter - 2.0f * c > tmin)) { mx = w.cx; my = w.cy; mz = w.cz; mine = true; }
						done = !w.advance();
					}
				}
				if (mine && lane < 9 * RAY_WAVE_AHEAD) {
					const int y = my + dy, z = mz + dz;
					const int xa = max(mx - 1, 0), xb = min(mx + 1, g.nx - 1);
					if (y >= 0 && y < g.ny && z >= 0 && z < g.nz && xa <= xb)
						grid_row_runs(d, g, xa, xb, y, z, [&](uint32_t q0, uint32_t q1) { for (uint32_t q = q0; q < q1; ++q) ray_test_body_eager(d, ry, o, dir, __float_as_uint(d.sorted_max[q].w), best); });
				}
				ray_share_bound(best, tmin);
			}
		}
	}
	// the wave's answer: lowest (t, id) among the lanes that hold a hit
	float wt = best.id != SGP_INVALID_ID ? best.t : 3.0e38f; uint32_t wid = best.id;
	for (int off = 32; off >= 1; off >>= 1) {
		const float ot = __shfl_xor(wt, off, 64); const uint32_t oid = (uint32_t)__shfl_xor((int)wid, off, 64);
		if (oid != SGP_INVALID_ID && (wid == SGP_INVALID_ID || ot < wt || (ot == wt && oid < wid))) { wt = ot; wid = oid; }
	}
	sgp_hit h;
	h.id = wid; h.t = 0.0f; h.normal[0] = h.normal[1] = h.normal[2] = 0.0f; h.triangle = SGP_INVALID_ID; h.material = 0; h.bary[0] = h.bary[1] = 0.0f; h.sub_shape = 0; h.userdata = 0;
	if (wid != SGP_INVALID_ID) {
		const unsigned long long owners = __ballot(best.id == wid && best.t == wt);
		const int src = __ffsll((long long)owners) - 1;
		h.t = wt;
		h.normal[0] = __shfl(best.n.x, src, 64); h.normal[1] = __shfl(best.n.y, src, 64); h.normal[2] = __shfl(best.n.z, src, 64);
		h.triangle = (uint32_t)__shfl((int)best.sub.tri, src, 64); h.material = (uint32_t)__shfl((int)best.sub.mat, src, 64);
		h.bary[0] = __shfl(best.sub.u, src, 64); h.bary[1] = __shfl(best.sub.v, src, 64);
	}
	return h;
}

// The resident ray server (RayMailbox, sgp_kernels.h): one wave.  Its 64 lanes trace the ray together (raycast_wave); the mailbox lines are read and written by lanes 0..15, one word each, as single 64-byte transactions over the host link.
__global__ void __launch_bounds__(64) k_ray_server(DV d, RayMailbox* mb, uint32_t first_seq, uint32_t generation, uint64_t idle_ticks, uint64_t max_ticks)
{
	const int lane = (int)threadIdx.x;
	__shared__ RayServerCache cache;
	ray_cache_fill(d, cache);
	uint32_t* req_line = (uint32_t*)mb;
	uint32_t* res_line = req_line + 16;
	uint32_t seen = first_seq;
	const uint64_t t_start = wall_clock64();
	uint64_t t_last = t_start;
	for (uint32_t poll = 0;; ++poll) {
		const uint32_t wv = lane < 16 ? __hip_atomic_load(&req_line[lane], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) : 0u;
		const uint32_t req = (uint32_t)__shfl((int)wv, 0, 64), stop_gen = (uint32_t)__shfl((int)wv, 1, 64);
		// told to leave (the host writes that BEFORE anything it does to the world and before any later request; the line is read as a whole, so a request
		// seen here without the order to leave was made while this server's view of the world was current)
		if ((int32_t)(stop_gen - generation) >= 0) break;
		if (req != seen) {
			sgp_ray ry;
			uint32_t* dst = (uint32_t*)&ry;
#pragma unroll
			for (int i = 0; i < (int)(sizeof(sgp_ray) / 4); ++i) dst[i] = (uint32_t)__shfl((int)wv, 2 + i, 64);
			const sgp_hit h = raycast_wave(d, ry, cache);
			const uint32_t* hs = (const uint32_t*)&h;
			uint32_t out = 0u;
			if (lane == 0 || lane == 15) out = req; else if (lane == 1) out = generation - 1u;      // (exited_gen: not this one)
#pragma unroll
			for (int i = 0; i < (int)(sizeof(sgp_hit) / 4); ++i) if (lane == 2 + i) out = hs[i];
			if (lane < 16) __hip_atomic_store(&res_line[lane], out, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
			seen = req;
			t_last = wall_clock64();
			continue;
		}
		if ((poll & 15u) == 15u) { const uint64_t now = wall_clock64(); if (now - t_last > idle_ticks || now - t_start > max_ticks) break; }
	}
	// a request that arrived while this wave was deciding to leave is answered by the next server: the host sees exited_gen == this generation with its request open
	if (lane == 1) __hip_atomic_store(&res_line[1], generation, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);      // exited_gen
}

// ---------------------------------------------------------------------------------------------------------------
// Shape queries of the character controller (JPH::CharacterVirtual: CollideShape with a maximum separation, swept test).

// where the answers of one query capsule go: the records into the caller's buffer (a slot per point from the global counter), mesh bodies onto the wave's list
#define QUERY_MESH_LIST 32
struct CapsuleSink {
	const DV& d; uint32_t k; sgp_query_contact* out; uint32_t cap; uint32_t* count; uint32_t* mesh_list; uint32_t* n_mesh;
	SGP_DEV bool list_mesh(uint32_t j) const { const uint32_t at = atomicAdd(n_mesh, 1u); if (at < QUERY_MESH_LIST) mesh_list[at] = j; return at < QUERY_MESH_LIST; }
	// the points of one manifold (normal: body -> capsule) as contacts of query k with body j
	SGP_DEV void emit(uint32_t j, uint32_t f, int g, const sgd_manifold& m) const
	{
		for (int i = 0; i < m.np; ++i) {
			const uint32_t slot = atomicAdd(count, 1u);
			if (slot < cap) out[slot] = contact_record(d, k, j, f, g, m, i);
		}
	}
};

// ONE WAVE PER QUERY CAPSULE (the character controller asks for one or a few per update, and waits for the answer): the candidate bodies -- the
// large ones, and those of the broad-phase cells its bounds reach -- dealt to the 64 lanes; the mesh bodies among them (a player stands on one and
// next to others all the time) are then taken one after the other by the whole wave, 64 candidate triangles per round (mesh_pair_groups).
__global__ void __launch_bounds__(64) k_collide_capsules(DV d, const sgp_capsule_query* qs, uint32_t n, sgp_query_contact* out, uint32_t cap, uint32_t* count)
{
	__shared__ MeshPairLds<64> L;
	__shared__ uint32_t mesh_list[QUERY_MESH_LIST];
	__shared__ uint32_t n_mesh;
	const uint32_t k = blockIdx.x;
	if (k >= n) return;
	const uint32_t lane = threadIdx.x;
	const sgp_capsule_query q = qs[k];
	quat qq; qq.x = q.rot[0]; qq.y = q.rot[1]; qq.z = q.rot[2]; qq.w = q.rot[3];
	sgd_shape sc; v3 lo, hi;
	capsule_shape(V3(q.pos[0], q.pos[1], q.pos[2]), qq, q.radius, q.half_height, q.max_separation, sc, lo, hi);
	const CapsuleSink sink = { d, k, out, cap, count, mesh_list, &n_mesh };
	if (lane == 0) n_mesh = 0;
	__syncthreads();
	sq_walk<64>(d, lo, hi, lane, [&](uint32_t j) { capsule_query_body(d, q.ignore_id, q.collidable_only != 0u, q.max_separation, sc, lo, hi, j, sink); });
	__syncthreads();
	const uint32_t nm = min(n_mesh, (uint32_t)QUERY_MESH_LIST);
	const v3 es = V3(q.max_separation, q.max_separation, q.max_separation);
	for (uint32_t mi = 0; mi < nm; ++mi) {
		const uint32_t mid = mesh_list[mi];
		bool valid = true, dropped = false;
		sgd_shape X = sc;
		mesh_pair_groups<64, 4>(d, L, valid, X, mid, v3_sub(lo, es), v3_add(hi, es), q.max_separation, 0, (int)lane, 0u, dropped, V3(q.movement[0], q.movement[1], q.movement[2]), q.active_edges != 0u);      // (CharacterVirtual::GetContactsAtPosition: CollideOnlyWithActive + its direction of travel; 0: every edge with its own normal)
		if ((int)lane < L.mc.ng) {
			const sgd_mesh_group& grp = L.mc.g[lane];
			sgd_manifold mm;
			sgd_hull_reduce(grp.n, grp.p_mesh, grp.p_body, grp.np, &mm);
			sink.emit(mid, d.flags[mid], (int)lane, mm);
		}
		__syncthreads();
	}
}

// one thread per cast (spherecast_walk, spherecast_body: sgp_dev_queries.h)
__global__ void __launch_bounds__(64) k_spherecast(DV d, const sgp_ray* rays, const float* radii, uint32_t n, sgp_hit* hits)
{
	const uint32_t k = blockIdx.x * 64 + threadIdx.x;
	if (k >= n) return;
	const sgp_ray ry = rays[k];
	const float rs = radii[k];
	const v3 o = V3(ry.origin[0], ry.origin[1], ry.origin[2]), dir = V3(ry.dir[0], ry.dir[1], ry.dir[2]);
	SphereHit best; best.t = ry.max_t; best.id = SGP_INVALID_ID; best.n = V3(0.0f, 0.0f, 0.0f);
	spherecast_walk<1>(d, o, dir, ry.max_t, rs, 0u, [&](uint32_t j) { spherecast_body(d, ry.ignore_id, ry.collidable_only != 0u, ry.max_t, rs, o, dir, j, best); });
	sgp_hit h;
	h.id = best.id; h.t = best.id == SGP_INVALID_ID ? 0.0f : best.t;
	h.normal[0] = best.n.x; h.normal[1] = best.n.y; h.normal[2] = best.n.z;
	h.triangle = SGP_INVALID_ID; h.material = 0; h.bary[0] = h.bary[1] = 0.0f; h.sub_shape = 0;
	h.userdata = 0;
	hits[k] = h;
}
void launch_ray_server(const DV& d, RayMailbox* mb, uint32_t first_seq, uint32_t generation, uint64_t idle_ticks, uint64_t max_ticks, hipStream_t s) { hipLaunchKernelGGL(k_ray_server, dim3(1), dim3(64), 0, s, d, mb, first_seq, generation, idle_ticks, max_ticks); }
void launch_raycast(const DV& d, const sgp_ray* rays, uint32_t n, sgp_hit* hits, hipStream_t s) { if (n) hipLaunchKernelGGL(k_raycast, dim3((n + 63) / 64), dim3(64), 0, s, d, rays, n, hits); }
void launch_raycast_any(const DV& d, const sgp_ray* rays, uint32_t n, uint8_t* hit, hipStream_t s) { if (n) hipLaunchKernelGGL(k_raycast_any, dim3((n + 63) / 64), dim3(64), 0, s, d, rays, n, hit); }
void launch_collide_capsules(const DV& d, const sgp_capsule_query* q, uint32_t n, sgp_query_contact* out, uint32_t cap, uint32_t* count, hipStream_t s) { if (n) hipLaunchKernelGGL(k_collide_capsules, dim3(n), dim3(64), 0, s, d, q, n, out, cap, count); }      // a wave per query
void launch_spherecast(const DV& d, const sgp_ray* rays, const float* radii, uint32_t n, sgp_hit* hits, hipStream_t s) { if (n) hipLaunchKernelGGL(k_spherecast, dim3((n + 63) / 64), dim3(64), 0, s, d, rays, radii, n, hits); }
