// sgp_world_queries.hip -- ray queries (PhysicsWorld::traceRay, PhysicsWorld.cpp:1668-1725), the character controller's capsule queries and sphere casts, overlap
// queries and shape casts with any convex shape.  Every entry point goes through query_prelude before it launches and lays its buffers out with StageCarve.
#include "sgp_world_internal.h"

// ---------------------------------------------------------------------------------------------------------------
// ray queries, PhysicsWorld.cpp:1668-1725

static void finish_hit(sgp_world* w, sgp_hit* h)
{
	h->userdata = h->id != SGP_INVALID_ID ? w->hb[h->id].userdata : 0;
	h->sub_shape = 0;
	if (h->id != SGP_INVALID_ID) h->id = compound_id_of(w, h->id, &h->sub_shape);
}

// One ray through the resident server (RayMailbox, sgp_kernels.h).  Returns 1 when the ray was answered, 0 when the caller should take the launch path
// (server disabled or it could not be reached), < 0 on error.
#define SGP_RAY_SERVER_IDLE_TICKS 30000ull          // 300 us at the 100 MHz wall clock: a caller tracing rays one after the other never lets it idle that long
#define SGP_RAY_SERVER_MAX_TICKS 20000000ull        // 200 ms: a server older than that leaves and is started again (nothing lives on the stream for ever)
static int ray_through_server(sgp_world* w, const sgp_ray* ray, sgp_hit* hit)
{
	if (!w->ray_server_enabled) return 0;
	if (!w->ray_mb) {
		if (hipHostMalloc((void**)&w->ray_mb, sizeof(RayMailbox), hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess) { w->ray_server_enabled = false; (void)hipGetLastError(); return 0; }
		memset(w->ray_mb, 0, sizeof(RayMailbox));      // (generation 0 = nobody: the first server is generation 1)
	}
	RayMailbox* mb = w->ray_mb;
	for (int attempt = 0; attempt < 3; ++attempt) {
		if (!w->ray_server_on) {
			// (the previous server, if any, was told to stop or left on its own; the new one queues behind it on the stream)
			++w->ray_gen;      // (servers of older generations have been told to leave, or have left; what they still write names their generation, not this one)
			RayMailbox* dmb = nullptr;
			if (hipHostGetDevicePointer((void**)&dmb, mb, 0) != hipSuccess) { w->ray_server_enabled = false; (void)hipGetLastError(); return 0; }
			launch_ray_server(w->dv, dmb, w->ray_seq, w->ray_gen, SGP_RAY_SERVER_IDLE_TICKS, SGP_RAY_SERVER_MAX_TICKS, w->stream);
			w->ray_server_on = true; w->ray_server_launches++;
		}
		mb->ray = *ray;
		const uint32_t seq = ++w->ray_seq;
		__atomic_store_n(&mb->req_seq, seq, __ATOMIC_RELEASE);
		const auto t0 = std::chrono::steady_clock::now();
		for (uint32_t spin = 0;; ++spin) {
			if (__atomic_load_n(&mb->done_seq, __ATOMIC_ACQUIRE) == seq && __atomic_load_n(&mb->done_seq2, __ATOMIC_ACQUIRE) == seq) { *hit = mb->hit; w->ray_server_rays++; return 1; }
			if ((spin & 1023u) == 1023u) {
				if (__atomic_load_n(&mb->exited_gen, __ATOMIC_ACQUIRE) == w->ray_gen) break;      // this generation's server left (idle / age) before it saw the request: start another
				if (std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > 2.0) {      // (never observed: the launch path still answers)
					ray_server_stop(w); HIP_TRY(hipStreamSynchronize(w->stream)); w->ray_server_enabled = false; return 0;
				}
			}
		}
		// the wave is gone; it may still have answered just before leaving
		if (__atomic_load_n(&mb->done_seq, __ATOMIC_ACQUIRE) == seq && __atomic_load_n(&mb->done_seq2, __ATOMIC_ACQUIRE) == seq) { *hit = mb->hit; w->ray_server_on = false; w->ray_server_rays++; return 1; }
		w->ray_server_on = false;
	}
	return 0;
}

SGP_API int sgp_raycast(sgp_world* w, const sgp_ray* rays, uint32_t n, sgp_hit* hits)
{
	if (!w || (!rays && n) || (!hits && n)) return fail(SGP_ERR_INVALID, "sgp_raycast: NULL");
	hipSetDevice(w->device);
	if (n == 1 && w->ray_server_on && w->cmds.empty() && w->ghost_refresh.empty() && !w->large_dirty && !w->large_list_dirty && w->grid_valid) {
		// the caller is tracing rays one by one (PhysicsWorld::traceRay in a loop) and nothing touched the world since the last one: hand it to the resident wave
		const int r = ray_through_server(w, rays, hits);
		if (r < 0) return r;
		if (r == 1) { finish_hit(w, hits); return SGP_OK; }
	}
	if (!n) { int r = flush_cmds(w); return r; }
	{ int r = query_prelude(w); if (r != SGP_OK) return r; }
	if (n == 1 && w->high) {
		// a single ray: start (or reach) the resident server behind the grid kernels just queued; the next single rays find it running
		const int r = ray_through_server(w, rays, hits);
		if (r < 0) return r;
		if (r == 1) { finish_hit(w, hits); return SGP_OK; }
	}
	StageCarve c;
	const size_t rays_off = c.add(sizeof(sgp_ray) * n), hits_off = c.add(sizeof(sgp_hit) * n);
	{ int r = ensure_stage(w, c.total); if (r != SGP_OK) return r; }
	sgp_hit* hh = stage_h<sgp_hit>(w, hits_off);
	memcpy(stage_h<sgp_ray>(w, rays_off), rays, sizeof(sgp_ray) * n);
	if (n <= 64) {
		// a handful of rays (the facade's traceRay is n = 1): the kernel reads them from, and writes the hits to, the pinned host buffer
		// directly -- one launch and one sync instead of two copies around it
		launch_raycast(w->dv, stage_h<sgp_ray>(w, rays_off), n, hh, w->stream);
		HIP_TRY(hipStreamSynchronize(w->stream));
	} else {
		HIP_TRY(hipMemcpyAsync(stage_d<sgp_ray>(w, rays_off), stage_h<sgp_ray>(w, rays_off), sizeof(sgp_ray) * n, hipMemcpyHostToDevice, w->stream));
		sgp_hit* dh = stage_d<sgp_hit>(w, hits_off);
		launch_raycast(w->dv, stage_d<sgp_ray>(w, rays_off), n, dh, w->stream);
		HIP_TRY(hipMemcpyAsync(hh, dh, sizeof(sgp_hit) * n, hipMemcpyDeviceToHost, w->stream));
		HIP_TRY(hipStreamSynchronize(w->stream));
	}
	memcpy(hits, hh, sizeof(sgp_hit) * n);
	for (uint32_t k = 0; k < n; ++k) finish_hit(w, &hits[k]);
	return SGP_OK;
}

// doesRayHitAnything, batched (k_raycast_any): one byte per ray.  Always the launch path, n = 1 included: query_prelude tells a resident ray server to leave
SGP_API int sgp_raycast_any(sgp_world* w, const sgp_ray* rays, uint32_t n, uint8_t* hit_out)
{
	if (!w || (!rays && n) || (!hit_out && n)) return fail(SGP_ERR_INVALID, "sgp_raycast_any: NULL");
	if (!n) { hipSetDevice(w->device); int r = flush_cmds(w); return r; }
	{ int r = query_prelude(w); if (r != SGP_OK) return r; }
	StageCarve c;
	const size_t rays_off = c.add(sizeof(sgp_ray) * n), hit_off = c.add(n);
	{ int r = ensure_stage(w, c.total); if (r != SGP_OK) return r; }
	uint8_t* hh = stage_h<uint8_t>(w, hit_off);
	memcpy(stage_h<sgp_ray>(w, rays_off), rays, sizeof(sgp_ray) * n);
	if (n <= 64) {
		// (as sgp_raycast: a handful of rays are read from, and answered into, the pinned host buffer directly)
		launch_raycast_any(w->dv, stage_h<sgp_ray>(w, rays_off), n, hh, w->stream);
		HIP_TRY(hipStreamSynchronize(w->stream));
	} else {
		HIP_TRY(hipMemcpyAsync(stage_d<sgp_ray>(w, rays_off), stage_h<sgp_ray>(w, rays_off), sizeof(sgp_ray) * n, hipMemcpyHostToDevice, w->stream));
		uint8_t* dh = stage_d<uint8_t>(w, hit_off);
		launch_raycast_any(w->dv, stage_d<sgp_ray>(w, rays_off), n, dh, w->stream);
		HIP_TRY(hipMemcpyAsync(hh, dh, n, hipMemcpyDeviceToHost, w->stream));
		HIP_TRY(hipStreamSynchronize(w->stream));
	}
	memcpy(hit_out, hh, n);
	return SGP_OK;
}

// What every query needs before its launch (all entry points of this file, sgp_characters_update, sgp_particles_update): pending body edits flushed -- which also tells
// a resident ray server to leave --, and the broad-phase grid valid for the poses as they are.  Nothing waits unless an edit was pending.
int query_prelude(sgp_world* w)
{
	hipSetDevice(w->device);
	{ int r = flush_cmds(w); if (r != SGP_OK) return r; }
	return ensure_query_grid(w);
}

int ensure_query_grid(sgp_world* w)
{
	if (!w->grid_valid && w->high) {
		// poses changed since the grid was built (a step integrates after its broad phase; edits move bodies): re-bin
		const DV& d = w->dv; hipStream_t s = w->stream; const uint32_t nb = w->high;
		launch_step_begin(d, *w->h_sp, nb, false, false, s); w->sp_uploaded = *w->h_sp; w->sp_uploaded_valid = true;
		launch_bp_bounds(d, nb, s); launch_bp_cell(d, nb, s); launch_bp_scan(d, s); launch_bp_scatter(d, nb, s);
		w->grid_valid = true;
	}
	return SGP_OK;
}

// The contact records of a call as the ABI reports them: the first n_sorted records sorted by (query, body, point) -- the kernels leave the contact's point
// index in sub_shape --, then userdata and the compound's id and child index in the first n_filled of them
static void finish_contacts(sgp_world* w, sgp_query_contact* h, uint32_t n_sorted, uint32_t n_filled)
{
	std::sort(h, h + n_sorted, [](const sgp_query_contact& a, const sgp_query_contact& b) {
		if (a.query != b.query) return a.query < b.query;
		if (a.body != b.body) return a.body < b.body;
		return a.sub_shape < b.sub_shape; });
	for (uint32_t i = 0; i < n_filled; ++i) { h[i].userdata = w->hb[h[i].body].userdata; h[i].body = compound_id_of(w, h[i].body, &h[i].sub_shape); }
}

// CharacterVirtual's CollideShape (PlayerPhysics.cpp:258-353): contacts of capsules with everything within max_separation
SGP_API int sgp_collide_capsules(sgp_world* w, const sgp_capsule_query* qs, uint32_t n, sgp_query_contact* out, uint32_t cap, uint32_t* n_out)
{
	if (!w || (!qs && n) || (!out && cap) || !n_out) return fail(SGP_ERR_INVALID, "sgp_collide_capsules: NULL");
	{ int r = n ? query_prelude(w) : flush_cmds(w); if (r != SGP_OK) return r; }
	*n_out = 0;
	if (!n) return SGP_OK;
	StageCarve c;
	const size_t q_off = c.add(sizeof(sgp_capsule_query) * n), out_off = c.add(sizeof(sgp_query_contact) * std::max(cap, 1u)), count_off = c.add(16);
	{ int r = ensure_stage(w, c.total); if (r != SGP_OK) return r; }
	memcpy(stage_h<char>(w, q_off), qs, sizeof(sgp_capsule_query) * n);
	HIP_TRY(hipMemcpyAsync(stage_d<char>(w, q_off), stage_h<char>(w, q_off), sizeof(sgp_capsule_query) * n, hipMemcpyHostToDevice, w->stream));
	HIP_TRY(hipMemsetAsync(stage_d<uint32_t>(w, count_off), 0, sizeof(uint32_t), w->stream));
	launch_collide_capsules(w->dv, stage_d<sgp_capsule_query>(w, q_off), n, stage_d<sgp_query_contact>(w, out_off), cap, stage_d<uint32_t>(w, count_off), w->stream);
	HIP_TRY(hipMemcpyAsync(stage_h<char>(w, out_off), stage_d<char>(w, out_off), c.total - out_off, hipMemcpyDeviceToHost, w->stream));      // (the records and the count behind them)
	HIP_TRY(hipStreamSynchronize(w->stream));
	const uint32_t cnt = *stage_h<uint32_t>(w, count_off);
	const uint32_t m = std::min(cnt, cap);
	sgp_query_contact* h = stage_h<sgp_query_contact>(w, out_off);
	finish_contacts(w, h, m, m);
	memcpy(out, h, sizeof(sgp_query_contact) * m);
	*n_out = cnt;
	return SGP_OK;
}

// NarrowPhaseQuery::CollideShape with a sphere, box, capsule or convex hull, batched (kernels and their two organisations: sgp_k_shapequery.hip)
static const char* shape_query_fault(const sgp_world* w, const sgp_shape_query& q)
{
	if (!finite3(q.pos) || !finite4(q.rot) || !finite3(q.movement) || !std::isfinite(q.max_separation)) return "non-finite pose, movement or max_separation";
	if (!(q.rot[0] * q.rot[0] + q.rot[1] * q.rot[1] + q.rot[2] * q.rot[2] + q.rot[3] * q.rot[3] > 0.0f)) return "zero rotation quaternion";
	if (q.max_separation < 0.0f) return "negative max_separation";
	if (!finite4(q.shape)) return "non-finite shape";
	switch (q.shape_type) {
	case SGP_SHAPE_SPHERE: return q.shape[0] > 0.0f ? nullptr : "non-positive sphere radius";
	case SGP_SHAPE_BOX: return (q.shape[0] > 0.0f && q.shape[1] > 0.0f && q.shape[2] > 0.0f) ? nullptr : "non-positive box half extent";
	case SGP_SHAPE_CAPSULE: return (q.shape[0] > 0.0f && q.shape[1] >= 0.0f) ? nullptr : "non-positive capsule size";
	case SGP_SHAPE_HULL: {
		const float h = q.shape[0];
		if (!(h >= 1.0f) || h != floorf(h) || h >= (float)w->hulls.size() || w->hulls[(size_t)h].nv == 0) return "no such hull";
		return nullptr; }
	case SGP_SHAPE_MESH: return "a mesh cannot be a query shape";
	default: return "unknown shape type";
	}
}

// One run of a call with candidate lists (sgp_collide_shapes, sgp_cast_shapes): the stage buffer carved into [records][counters][out][three lists of pcap pairs],
// the records uploaded, the counters zeroed, launch(records, counters, out, lists) on the device's regions, the counters read back into ctr (the call's one wait).
// Returns through *most the longest list the kernels counted -- above pcap the caller grows pcap and runs the call again, by its own rule -- and through *out_off
// where `out` lies in both buffers.
template <class Launch> static int run_list_call(sgp_world* w, const void* recs, size_t rec_bytes, uint32_t* ctr, size_t ctr_bytes, size_t out_bytes, uint64_t pcap, size_t* out_off, uint32_t* most, Launch launch)
{
	StageCarve c;
	const size_t rec_off = c.add(rec_bytes), ctr_off = c.add(ctr_bytes);
	*out_off = c.add(out_bytes);
	const size_t lists_off = c.add(3 * sizeof(uint2) * (size_t)pcap);
	{ int r = ensure_stage(w, c.total); if (r != SGP_OK) return r; }
	memcpy(stage_h<char>(w, rec_off), recs, rec_bytes);
	HIP_TRY(hipMemcpyAsync(stage_d<char>(w, rec_off), stage_h<char>(w, rec_off), rec_bytes, hipMemcpyHostToDevice, w->stream));
	PairLists lists;
	lists.prim = stage_d<uint2>(w, lists_off); lists.hull = lists.prim + pcap; lists.mesh = lists.hull + pcap; lists.pcap = (uint32_t)pcap;
	HIP_TRY(hipMemsetAsync(stage_d<char>(w, ctr_off), 0, ctr_bytes, w->stream));
	launch(stage_d<char>(w, rec_off), stage_d<uint32_t>(w, ctr_off), stage_d<char>(w, *out_off), lists);
	HIP_TRY(hipMemcpyAsync(stage_h<char>(w, ctr_off), stage_d<char>(w, ctr_off), ctr_bytes, hipMemcpyDeviceToHost, w->stream));
	HIP_TRY(hipStreamSynchronize(w->stream));
	memcpy(ctr, stage_h<char>(w, ctr_off), ctr_bytes);
	*most = std::max(ctr[SQ_N_PRIM], std::max(ctr[SQ_N_HULL], ctr[SQ_N_MESH]));
	return SGP_OK;
}
static_assert(SQ_N_PRIM == SC_N_PRIM && SQ_N_HULL == SC_N_HULL && SQ_N_MESH == SC_N_MESH, "run_list_call reads the list counters of either call");

SGP_API int sgp_collide_shapes(sgp_world* w, const sgp_shape_query* qs, uint32_t n, sgp_query_contact* out, uint32_t cap, uint32_t* n_out)
{
	if (!w || (!qs && n) || (!out && cap) || !n_out) return fail(SGP_ERR_INVALID, "sgp_collide_shapes: NULL");
	for (uint32_t k = 0; k < n; ++k) if (const char* what = shape_query_fault(w, qs[k])) {      // (before anything is launched: a call is answered whole or not at all)
		char msg[160]; snprintf(msg, sizeof(msg), "sgp_collide_shapes: query %u: %s", k, what);
		return fail(SGP_ERR_INVALID, msg);
	}
	{ int r = n ? query_prelude(w) : flush_cmds(w); if (r != SGP_OK) return r; }
	*n_out = 0;
	if (!n) return SGP_OK;
	const bool by_wave = w->query_path == 1 || (w->query_path == 0 && n <= w->sq_wave_max_n);
	// Capacities: a first guess from what the last call needed per query.  The kernels count everything they find, also what did not fit; a call that overflowed
	// a list or the output runs again with room for what was counted (a list that overflowed hid some of the output: that run may be followed by one more).
	uint64_t ocap = std::max<uint64_t>(64, (uint64_t)((double)w->sq_out_per_query * n) + 1), pcap = std::max<uint64_t>(64, (uint64_t)((double)w->sq_pairs_per_query * n) + 1);
	if (n == w->sq_last_n) { ocap = std::max<uint64_t>(ocap, w->sq_last_out + w->sq_last_out / 4); pcap = std::max<uint64_t>(pcap, w->sq_last_pairs + w->sq_last_pairs / 4); }      // (the same batch again, as every frame: what it needed last time)
	uint32_t ctr[4] = { 0, 0, 0, 0 }, most = 0;
	size_t out_off = 0;
	for (int attempt = 0;; ++attempt) {
		if (attempt == 6) return fail(SGP_ERR_CAPACITY, "sgp_collide_shapes: the answer kept outgrowing its buffers");      // (cannot happen while the world stands still: the counts are exact)
		if (ocap > 0x7FFFFFFFull || pcap > 0x7FFFFFFFull) return fail(SGP_ERR_CAPACITY, "sgp_collide_shapes: more than 2^31 contacts or candidate pairs");
		const int r = run_list_call(w, qs, sizeof(sgp_shape_query) * n, ctr, sizeof(ctr), sizeof(sgp_query_contact) * (size_t)ocap, pcap, &out_off, &most, [&](char* recs, uint32_t* dctr, char* dout, const PairLists& lists) {
			SqBufs b;
			b.qs = (const sgp_shape_query*)recs; b.n = n; b.out = (sgp_query_contact*)dout; b.cap = (uint32_t)ocap; b.ctr = dctr; b.lists = lists;
			if (by_wave) launch_shape_queries_wave(w->dv, b, w->stream); else launch_shape_queries_pairs(w->dv, b, w->stream);
		});
		if (r != SGP_OK) return r;
		if (ctr[SQ_N_OUT] <= ocap && most <= pcap) break;
		if (most > pcap) { ocap = std::max<uint64_t>(ocap, (uint64_t)ctr[SQ_N_OUT] * 2u); pcap = most; }
		else ocap = ctr[SQ_N_OUT];
	}
	const uint32_t cnt = ctr[SQ_N_OUT];
	// (per query at most 8: one huge volume must not size the buffers of the next call's thousands of small ones)
	w->sq_out_per_query = std::min(8.0f, 1.25f * (float)cnt / (float)n + 1.0f); w->sq_pairs_per_query = std::min(8.0f, 1.25f * (float)most / (float)n + 1.0f);
	w->sq_last_n = n; w->sq_last_out = cnt; w->sq_last_pairs = most;
	sgp_query_contact* h = stage_h<sgp_query_contact>(w, out_off);
	if (cnt) {
		HIP_TRY(hipMemcpyAsync(h, stage_d<char>(w, out_off), sizeof(sgp_query_contact) * (size_t)cnt, hipMemcpyDeviceToHost, w->stream));
		HIP_TRY(hipStreamSynchronize(w->stream));
	}
	const uint32_t m = std::min(cnt, cap);      // the FIRST cap records of the whole sorted answer
	finish_contacts(w, h, cnt, m);
	if (m) memcpy(out, h, sizeof(sgp_query_contact) * m);
	*n_out = cnt;
	return SGP_OK;
}

// NarrowPhaseQuery::CastShape with a sphere, box, capsule or convex hull, batched (kernels: sgp_k_shapecast.hip)
static const char* shape_cast_fault(const sgp_world* w, const sgp_shape_cast& c)
{
	sgp_shape_query q;
	memset(&q, 0, sizeof(q));
	memcpy(q.pos, c.pos, sizeof(q.pos)); memcpy(q.rot, c.rot, sizeof(q.rot)); memcpy(q.shape, c.shape, sizeof(q.shape)); q.shape_type = c.shape_type;
	if (const char* what = shape_query_fault(w, q)) return what;
	if (!finite3(c.dir)) return "non-finite dir";
	if (fabsf(sqrtf(c.dir[0] * c.dir[0] + c.dir[1] * c.dir[1] + c.dir[2] * c.dir[2]) - 1.0f) > 1.0e-3f) return "dir is not a unit vector";
	if (!std::isfinite(c.max_t) || c.max_t < 0.0f) return "negative or non-finite max_t";
	return nullptr;
}

SGP_API int sgp_cast_shapes(sgp_world* w, const sgp_shape_cast* cs, uint32_t n, sgp_cast_hit* hits)
{
	if (!w || (n && (!cs || !hits))) return fail(SGP_ERR_INVALID, "sgp_cast_shapes: NULL");
	for (uint32_t k = 0; k < n; ++k) if (const char* what = shape_cast_fault(w, cs[k])) {      // (before anything is launched: a call is answered whole or not at all)
		char msg[160]; snprintf(msg, sizeof(msg), "sgp_cast_shapes: cast %u: %s", k, what);
		return fail(SGP_ERR_INVALID, msg);
	}
	{ int r = n ? query_prelude(w) : flush_cmds(w); if (r != SGP_OK) return r; }
	if (!n) return SGP_OK;
	// Capacity of the three candidate lists: a first guess from what the last call needed per cast.  The kernels count every candidate they find, also what did not
	// fit; a call that overflowed a list runs again with room for what was counted (the counts are exact while the world stands still: one more run at most).
	uint64_t pcap = std::max<uint64_t>(64, (uint64_t)((double)w->sc_pairs_per_cast * n) + 1);
	uint32_t ctr[SC_N_CTR], most = 0;
	size_t out_off = 0;
	for (int attempt = 0;; ++attempt) {
		if (attempt == 4) return fail(SGP_ERR_CAPACITY, "sgp_cast_shapes: the candidate lists kept outgrowing their buffers");
		if (pcap > 0x3FFFFFFFull) return fail(SGP_ERR_CAPACITY, "sgp_cast_shapes: more than 2^30 candidate pairs");
		const int r = run_list_call(w, cs, sizeof(sgp_shape_cast) * n, ctr, sizeof(ctr), sizeof(sgp_cast_hit) * 3 * (size_t)pcap, pcap, &out_off, &most, [&](char* recs, uint32_t* dctr, char* dout, const PairLists& lists) {
			ScBufs b;
			b.cs = (const sgp_shape_cast*)recs; b.n = n; b.out = (sgp_cast_hit*)dout; b.ctr = dctr; b.lists = lists;
			launch_shape_casts(w->dv, b, w->stream);
		});
		if (r != SGP_OK) return r;
		if (most <= pcap) break;
		w->sc_reruns++;
		pcap = most;
	}
	if (ctr[SC_N_DROPPED]) return fail(SGP_ERR_CAPACITY, "sgp_cast_shapes: a mesh tree is deeper than the walk's stack");
	w->sc_capped += ctr[SC_N_CAPPED];
	w->sc_pairs_per_cast = std::min(16.0f, 1.25f * (float)most / (float)n + 1.0f);
	const uint32_t cnt = ctr[SC_N_OUT];
	sgp_cast_hit* h = stage_h<sgp_cast_hit>(w, out_off);
	if (cnt) {
		HIP_TRY(hipMemcpyAsync(h, stage_d<char>(w, out_off), sizeof(sgp_cast_hit) * (size_t)cnt, hipMemcpyDeviceToHost, w->stream));
		HIP_TRY(hipStreamSynchronize(w->stream));
	}
	// per cast the least record by (t, id, triangle): whatever order the records arrived in
	for (uint32_t k = 0; k < n; ++k) { memset(&hits[k], 0, sizeof(sgp_cast_hit)); hits[k].id = SGP_INVALID_ID; hits[k].triangle = SGP_INVALID_ID; }
	for (uint32_t i = 0; i < cnt; ++i) {
		const sgp_cast_hit& r = h[i];
		sgp_cast_hit& o = hits[(uint32_t)r.userdata];
		if (o.id == SGP_INVALID_ID || r.t < o.t || (r.t == o.t && (r.id < o.id || (r.id == o.id && r.triangle < o.triangle)))) o = r;
	}
	for (uint32_t k = 0; k < n; ++k) {
		sgp_cast_hit& o = hits[k];
		o.userdata = 0;
		if (o.id == SGP_INVALID_ID) continue;
		o.userdata = w->hb[o.id].userdata;
		o.id = compound_id_of(w, o.id, &o.sub_shape);
	}
	return SGP_OK;
}

SGP_API int sgp_cast_shapes_counters(sgp_world* w, uint32_t counters_out[2])
{
	if (!w || !counters_out) return fail(SGP_ERR_INVALID, "sgp_cast_shapes_counters: NULL");
	counters_out[0] = w->sc_capped; counters_out[1] = w->sc_reruns;
	return SGP_OK;
}

SGP_API int sgp_spherecast(sgp_world* w, const sgp_ray* rays, const float* radii, uint32_t n, sgp_hit* hits)
{
	if (!w || (n && (!rays || !radii || !hits))) return fail(SGP_ERR_INVALID, "sgp_spherecast: NULL");
	{ int r = n ? query_prelude(w) : flush_cmds(w); if (r != SGP_OK) return r; }
	if (!n) return SGP_OK;
	StageCarve c;
	const size_t rays_off = c.add(sizeof(sgp_ray) * n), radii_off = c.add(sizeof(float) * n), hits_off = c.add(sizeof(sgp_hit) * n);
	{ int r = ensure_stage(w, c.total); if (r != SGP_OK) return r; }
	memcpy(stage_h<char>(w, rays_off), rays, sizeof(sgp_ray) * n);
	memcpy(stage_h<char>(w, radii_off), radii, sizeof(float) * n);
	HIP_TRY(hipMemcpyAsync(stage_d<char>(w, rays_off), stage_h<char>(w, rays_off), radii_off + sizeof(float) * n - rays_off, hipMemcpyHostToDevice, w->stream));      // (the rays and the radii behind them)
	launch_spherecast(w->dv, stage_d<sgp_ray>(w, rays_off), stage_d<float>(w, radii_off), n, stage_d<sgp_hit>(w, hits_off), w->stream);
	HIP_TRY(hipMemcpyAsync(stage_h<char>(w, hits_off), stage_d<char>(w, hits_off), sizeof(sgp_hit) * n, hipMemcpyDeviceToHost, w->stream));
	HIP_TRY(hipStreamSynchronize(w->stream));
	memcpy(hits, stage_h<char>(w, hits_off), sizeof(sgp_hit) * n);
	for (uint32_t k = 0; k < n; ++k) finish_hit(w, &hits[k]);
	return SGP_OK;
}
