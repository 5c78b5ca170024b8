// sgp_world_particles.hip -- the batched point particles (ParticleManager for 10^3 .. 10^6 particles): the host side of sgp_particles_*.
// The particles, their count, the event list and the replacement cursor live on the device and are touched by the kernels of sgp_k_particles.hip alone; the
// host keeps an upper bound of the live count (what the grids cover) and learns the counts when it reads.  add, update and clear enqueue and return.
#include "sgp_world_internal.h"

struct sgp_particles : WorldBatch {
	uint32_t cap = 0, ev_cap = 0;
	uint32_t cur = 0;        // which copy of the arrays holds the live particles (every update compacts into the other one)
	uint32_t upper = 0;      // the live count is at most this: grows with every add, exact after a read
	PsBufs b;
	// what the device counts said at the last read, while nothing has been enqueued since (a drain right after a read needs no wait of its own for them)
	PsState st_host; bool st_known = false;
	PsState* h_st = nullptr;      // pinned
	// the device copy of the newcomers' pinned staging (WorldBatch::h_up): up_cap records each, both grown by add
	sgp_particle* d_up = nullptr; uint32_t up_cap = 0;
	~sgp_particles() { if (d_up) hipFree(d_up); if (h_st) hipHostFree(h_st); }      // (behind WorldBatch::release, which has waited for the stream)
	// what a checkpoint holds: the counts, and as much of the current copy and of the event list as the counts say -- the host knows neither without a read
	void ckpt_layout(BatchCkptLayout& l)
	{
		l.device_whole(b.st, 1u);
		l.counted(b.hot[cur], 2, upper, 0, offsetof(PsState, n_live)); l.counted(b.cold[cur], 2, upper, 0, offsetof(PsState, n_live));
		l.counted(b.events, 1, ev_cap, 0, offsetof(PsState, n_events));
		l.scalar(cur); l.scalar(upper);
		l.capacity = cap; l.high = upper; l.n_alive = upper;
	}
};

SGP_API void sgp_default_particle(sgp_particle* p)
{
	if (!p) return;
	memset(p, 0, sizeof(*p));
	// Particle() (ParticleManager.h:35-36)
	p->restitution = 0.5f; p->width = 1.0f; p->dwidth_dt = 0.5f; p->opacity = 1.0f; p->dopacity_dt = -0.3f; p->mass = 1.0e-6f; p->area = 1.0e-6f;
}

SGP_API int sgp_particles_destroy(sgp_particles* ps) { return batch_destroy(ps, "sgp_particles_destroy"); }

SGP_API int sgp_particles_create(sgp_world* w, uint32_t capacity, uint32_t event_capacity, sgp_particles** out)
{
	if (!w || !out || capacity == 0 || capacity > SGP_PARTICLES_MAX_CAPACITY) return fail(SGP_ERR_INVALID, "sgp_particles_create: NULL world or out, or a capacity of 0 or beyond 2^20");
	hipSetDevice(w->device);
	sgp_particles* ps = new sgp_particles();
	ps->cap = capacity; ps->ev_cap = event_capacity;
	memset(&ps->b, 0, sizeof(ps->b)); memset(&ps->st_host, 0, sizeof(ps->st_host));
	ps->b.cap = capacity; ps->b.ev_cap = event_capacity;
	const size_t n = capacity, blocks = (n + 63) / 64;
	bool ok = ps->adopt(w);
	ok = ok && ps->alloc(ps->b.hot[0], 2 * n) && ps->alloc(ps->b.hot[1], 2 * n) && ps->alloc(ps->b.cold[0], 2 * n) && ps->alloc(ps->b.cold[1], 2 * n)
	        && ps->alloc(ps->b.evw, n) && ps->alloc(ps->b.wg_counts, blocks) && ps->alloc(ps->b.wg_off, blocks) && ps->alloc(ps->b.st, 1)
	        && ps->alloc(ps->b.events, event_capacity);
	ok = ok && hipHostMalloc((void**)&ps->h_st, sizeof(PsState), hipHostMallocDefault) == hipSuccess;
	return batch_created(ps, ok, out, "sgp_particles_create");
}

static const char* particle_fault(const sgp_particle& p)
{
	if (!finite3(p.pos) || !finite3(p.vel) || !std::isfinite(p.area) || !std::isfinite(p.mass) || !std::isfinite(p.restitution) || !std::isfinite(p.width)
	    || !std::isfinite(p.dwidth_dt) || !std::isfinite(p.opacity) || !std::isfinite(p.dopacity_dt)) return "a non-finite value";
	if (!(p.mass > 0.0f)) return "a non-positive mass";
	if (p.flags & ~SGP_PARTICLE_DIE_ON_HIT) return "an unknown flag";
	return nullptr;
}

// room for n newcomers in the staging buffers (add may allocate; update never does)
static int particles_ensure_staging(sgp_particles* ps, uint32_t n)
{
	if (n <= ps->up_cap) return SGP_OK;
	HIP_TRY(hipStreamSynchronize(ps->w->stream));      // (an append in flight reads the buffers about to go)
	ps->upload_in_flight = false;
	if (ps->d_up) { hipFree(ps->d_up); ps->d_up = nullptr; }
	ps->up_cap = 0;
	const uint32_t want = std::min<uint64_t>(ps->cap, std::max<uint64_t>(256, (uint64_t)n + n / 2));
	if (!ps->pin(sizeof(sgp_particle) * (size_t)want)) return fail(SGP_ERR_HIP, "hipHostMalloc", hipGetLastError());
	HIP_TRY(hipMalloc((void**)&ps->d_up, sizeof(sgp_particle) * (size_t)want));
	ps->up_cap = want;
	return SGP_OK;
}

SGP_API int sgp_particles_add(sgp_particles* ps, const sgp_particle* recs, uint32_t n)
{
	if (!batch_usable(ps) || (n && !recs)) return fail(SGP_ERR_INVALID, "sgp_particles_add: NULL, or the batch's world is gone");
	if (n > ps->cap) return fail(SGP_ERR_CAPACITY, "sgp_particles_add: more particles than the batch's capacity");
	for (uint32_t k = 0; k < n; ++k) if (const char* what = particle_fault(recs[k])) {      // (all or nothing)
		char msg[160]; snprintf(msg, sizeof(msg), "sgp_particles_add: particle %u: %s", k, what);
		return fail(SGP_ERR_INVALID, msg);
	}
	if (!n) return SGP_OK;
	sgp_world* w = ps->w;
	hipSetDevice(w->device);
	ray_server_stop(w);      // (a resident ray server must not keep this call's stream work waiting)
	{ int r = particles_ensure_staging(ps, n); if (r != SGP_OK) return r; }
	{ int r = ps->upload_begin(); if (r != SGP_OK) return r; }
	memcpy(ps->h_up, recs, sizeof(sgp_particle) * (size_t)n);
	HIP_TRY(hipMemcpyAsync(ps->d_up, ps->h_up, sizeof(sgp_particle) * (size_t)n, hipMemcpyHostToDevice, w->stream));
	{ int r = ps->upload_end(); if (r != SGP_OK) return r; }
	launch_particles_append(ps->b, ps->cur, ps->d_up, n, w->stream);
	ps->upper = (uint32_t)std::min<uint64_t>(ps->cap, (uint64_t)ps->upper + n);
	ps->st_known = false;
	HIP_TRY(hipGetLastError());
	return SGP_OK;
}

// Internal (sgp_world_crafts.hip): newcomers the device made -- `d_recs` and their count `d_count` are device memory of the same stream, bound >= the count.
// Enqueues the append and raises the host's upper bound of the live count by `bound`; no wait, no copy, no allocation.
uint32_t particles_capacity(const sgp_particles* ps) { return ps->cap; }
bool particles_of_world(const sgp_particles* ps, const sgp_world* w) { return batch_usable(ps) && ps->w == w; }
int particles_append_device(sgp_particles* ps, const sgp_particle* d_recs, const uint32_t* d_count, uint32_t bound)
{
	if (!batch_usable(ps) || bound > ps->cap) return fail(SGP_ERR_INVALID, "particles_append_device: the batch's world is gone, or more records than its capacity");
	if (!bound) return SGP_OK;
	launch_particles_append_device(ps->b, ps->cur, d_recs, d_count, bound, ps->w->stream);
	ps->upper = (uint32_t)std::min<uint64_t>(ps->cap, (uint64_t)ps->upper + bound);
	ps->st_known = false;
	HIP_TRY(hipGetLastError());
	return SGP_OK;
}

SGP_API int sgp_particles_update(sgp_particles* ps, float dt)
{
	if (!batch_usable(ps)) return fail(SGP_ERR_INVALID, "sgp_particles_update: NULL, or the batch's world is gone");
	if (!std::isfinite(dt) || !(dt >= 0.0f)) return fail(SGP_ERR_INVALID, "sgp_particles_update: dt must be finite and not negative");
	sgp_world* w = ps->w;
	{ int r = query_prelude(w); if (r != SGP_OK) return r; }
	if (!ps->upper) return SGP_OK;
	launch_particles_update(w->dv, ps->b, ps->cur, ps->upper, dt, w->h_sp->water_enabled, w->h_sp->water_z, w->stream);
	ps->cur ^= 1u;
	ps->st_known = false;
	HIP_TRY(hipGetLastError());
	return SGP_OK;
}

SGP_API int sgp_particles_clear(sgp_particles* ps)
{
	if (!batch_usable(ps)) return fail(SGP_ERR_INVALID, "sgp_particles_clear: NULL, or the batch's world is gone");
	sgp_world* w = ps->w;
	hipSetDevice(w->device);
	ray_server_stop(w);
	HIP_TRY(hipMemsetAsync(ps->b.st, 0, 2 * sizeof(uint32_t), w->stream));      // n_live, cursor
	ps->upper = 0; ps->st_known = false;
	return SGP_OK;
}

SGP_API int sgp_particles_checkpoint(sgp_particles* ps, sgp_batch_checkpoint** io) { return batch_checkpoint(ps, SGP_BATCH_PARTICLES, "sgp_particles_checkpoint", io); }
SGP_API int sgp_particles_rollback(sgp_particles* ps, const sgp_batch_checkpoint* cp)
{
	const int r = batch_rollback(ps, SGP_BATCH_PARTICLES, "sgp_particles_rollback", cp);
	if (r == SGP_OK) ps->st_known = false;      // (what the last read learned of the counts is of the abandoned history)
	return r;
}

SGP_API int sgp_particles_read(sgp_particles* ps, sgp_particle_state* out, uint32_t cap, uint32_t* n_out)
{
	if (!batch_usable(ps) || (cap && !out) || !n_out) return fail(SGP_ERR_INVALID, "sgp_particles_read: NULL, or the batch's world is gone");
	*n_out = 0;
	sgp_world* w = ps->w;
	hipSetDevice(w->device);
	ray_server_stop(w);
	const uint32_t upper = ps->upper;
	{ int r = ensure_stage(w, sizeof(sgp_particle_state) * (size_t)std::max(upper, 1u)); if (r != SGP_OK) return r; }
	launch_particles_pack(ps->b, ps->cur, upper, (sgp_particle_state*)w->stage_dev, w->stream);
	HIP_TRY(hipMemcpyAsync(ps->h_st, ps->b.st, sizeof(PsState), hipMemcpyDeviceToHost, w->stream));
	if (upper) HIP_TRY(hipMemcpyAsync(w->stage_host, w->stage_dev, sizeof(sgp_particle_state) * (size_t)upper, hipMemcpyDeviceToHost, w->stream));
	HIP_TRY(hipStreamSynchronize(w->stream));      // the call's one wait
	ps->st_host = *ps->h_st; ps->st_known = true;
	const uint32_t n = std::min(ps->st_host.n_live, upper);
	ps->upper = n;
	if (std::min(n, cap)) memcpy(out, w->stage_host, sizeof(sgp_particle_state) * (size_t)std::min(n, cap));
	*n_out = n;
	return SGP_OK;
}

SGP_API int sgp_particles_drain_events(sgp_particles* ps, sgp_particle_event* out, uint32_t cap, uint32_t* n_out, uint32_t* n_dropped)
{
	if (!batch_usable(ps) || (cap && !out) || !n_out || !n_dropped) return fail(SGP_ERR_INVALID, "sgp_particles_drain_events: NULL, or the batch's world is gone");
	*n_out = 0; *n_dropped = 0;
	sgp_world* w = ps->w;
	hipSetDevice(w->device);
	ray_server_stop(w);
	if (!ps->st_known) {
		HIP_TRY(hipMemcpyAsync(ps->h_st, ps->b.st, sizeof(PsState), hipMemcpyDeviceToHost, w->stream));
		HIP_TRY(hipStreamSynchronize(w->stream));
		ps->st_host = *ps->h_st; ps->st_known = true;
		ps->upper = std::min(ps->upper, ps->st_host.n_live);
	}
	const uint32_t raised = ps->st_host.n_events, held = std::min(raised, ps->ev_cap);
	if (!raised) return SGP_OK;
	if (held) {
		{ int r = ensure_stage(w, sizeof(sgp_particle_event) * (size_t)held); if (r != SGP_OK) return r; }
		HIP_TRY(hipMemcpyAsync(w->stage_host, ps->b.events, sizeof(sgp_particle_event) * (size_t)held, hipMemcpyDeviceToHost, w->stream));
	}
	HIP_TRY(hipMemsetAsync(&ps->b.st->n_events, 0, sizeof(uint32_t), w->stream));
	if (held) HIP_TRY(hipStreamSynchronize(w->stream));
	ps->st_host.n_events = 0;
	if (std::min(held, cap)) memcpy(out, w->stage_host, sizeof(sgp_particle_event) * (size_t)std::min(held, cap));
	*n_out = held; *n_dropped = raised - held;
	return SGP_OK;
}
