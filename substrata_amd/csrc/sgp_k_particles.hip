// sgp_k_particles.hip -- A7 -- the batched point particles of sgp_particles_* (ParticleManager::think for a whole batch, on the device).
// One of the stage files (stage map: sgp_kernels.h).  Kernels first, their launch wrappers at the end.
//
// One update is three launches: k_particles_update (a lane per particle: the ray, the arithmetic, an event word per slot and the survivors / events of every
// 64-slot block), k_particles_scan (one workgroup: the exclusive scan of those block counts, and the new counts) and k_particles_scatter (the survivors to the
// other copy of the arrays in their old order, the event records to n_events + rank).  No atomics and no workgroup that waits for another: the order of the
// particles and of the events is a function of the slots alone.  The live count, the event count and the replacement cursor stay on the device (PsState).
#include "sgp_dev_all.h"
#include "sgp_dev_raycast.h"
#include "sgp_dev_particles.h"

__global__ void __launch_bounds__(64) k_particles_update(DV d, PsBufs b, uint32_t cur, float dt, int water_enabled, float water_z)
{
	const uint32_t n = min(b.st->n_live, b.cap);
	if (blockIdx.x * 64u >= n) return;      // (the grid covers the host's upper bound of the live count)
	const uint32_t i = blockIdx.x * 64u + threadIdx.x;
	const bool valid = i < n;
	uint32_t word = 0u;
	if (valid) {
		float4* hot = b.hot[cur] + 2 * (size_t)i;
		const uint4* cold = b.cold[cur] + 2 * (size_t)i;
		float4 A = hot[0], B = hot[1];
		const uint4 c0 = cold[0], c1 = cold[1];
		float foam_w;
		word = particle_think(d, A, B, make_float4(__uint_as_float(c0.x), __uint_as_float(c0.y), __uint_as_float(c0.z), __uint_as_float(c0.w)), __uint_as_float(c1.x), c1.y, dt, water_enabled, water_z, &foam_w);
		hot[0] = A; hot[1] = B;
		b.evw[i] = make_uint2(word, __float_as_uint(foam_w));
	}
	const unsigned long long alive = __ballot(valid && !(word & SGP_PARTICLE_EV_DIED)), ev = __ballot(valid && word != 0u);
	if (threadIdx.x == 0) b.wg_counts[blockIdx.x] = make_uint2((uint32_t)__popcll(alive), (uint32_t)__popcll(ev));
}

// exclusive scan of the block counts by one workgroup (every thread a run of consecutive blocks), then the counts of the batch after this update
__global__ void __launch_bounds__(PS_SCAN_THREADS) k_particles_scan(PsBufs b)
{
	__shared__ uint2 part[PS_SCAN_THREADS];
	const uint32_t n = min(b.st->n_live, b.cap), nb = (n + 63u) / 64u, t = threadIdx.x;
	const uint32_t per = (nb + PS_SCAN_THREADS - 1u) / PS_SCAN_THREADS, lo = min(t * per, nb), hi = min(lo + per, nb);
	uint2 sum = make_uint2(0u, 0u);
	for (uint32_t k = lo; k < hi; ++k) { const uint2 c = b.wg_counts[k]; sum.x += c.x; sum.y += c.y; }
	part[t] = sum;
	__syncthreads();
	for (uint32_t off = 1; off < PS_SCAN_THREADS; off <<= 1) {
		uint2 v = part[t];
		if (t >= off) { const uint2 u = part[t - off]; v.x += u.x; v.y += u.y; }
		__syncthreads();
		part[t] = v;
		__syncthreads();
	}
	uint2 run = t ? part[t - 1] : make_uint2(0u, 0u);
	for (uint32_t k = lo; k < hi; ++k) { const uint2 c = b.wg_counts[k]; b.wg_off[k] = run; run.x += c.x; run.y += c.y; }
	if (t == PS_SCAN_THREADS - 1u) {
		const uint2 total = part[t];
		const uint32_t ne = b.st->n_events;
		b.st->n_prev = n; b.st->ev_base = ne;
		b.st->n_live = total.x;
		b.st->n_events = ne + min(total.y, 0xFFFFFFFFu - ne);
	}
}

SGP_DEV sgp_particle_event particle_event(uint4 c1, uint32_t kind, float4 A, float foam_w)
{
	sgp_particle_event e;
	e.tag = (uint64_t)c1.z | ((uint64_t)c1.w << 32); e.kind = kind;
	e.pos[0] = A.x; e.pos[1] = A.y; e.pos[2] = A.z; e.width = A.w; e.foam_width = foam_w;
	return e;
}

__global__ void __launch_bounds__(64) k_particles_scatter(PsBufs b, uint32_t cur)
{
	const uint32_t n = min(b.st->n_prev, b.cap);
	if (blockIdx.x * 64u >= n) return;
	const uint32_t i = blockIdx.x * 64u + threadIdx.x;
	const bool valid = i < n;
	const uint2 w = valid ? b.evw[i] : make_uint2(0u, 0u);
	const bool alive = valid && !(w.x & SGP_PARTICLE_EV_DIED), ev = valid && w.x != 0u;
	const unsigned long long ma = __ballot(alive), me = __ballot(ev), below = (1ull << threadIdx.x) - 1ull;
	const uint2 off = b.wg_off[blockIdx.x];
	if (!alive && !ev) return;
	const float4 A = b.hot[cur][2 * (size_t)i], B = b.hot[cur][2 * (size_t)i + 1];
	const uint4 c0 = b.cold[cur][2 * (size_t)i], c1 = b.cold[cur][2 * (size_t)i + 1];
	if (alive) {
		const size_t dst = (size_t)off.x + (uint32_t)__popcll(ma & below);      // (<= i: the compaction only moves towards the front)
		b.hot[cur ^ 1u][2 * dst] = A; b.hot[cur ^ 1u][2 * dst + 1] = B;
		b.cold[cur ^ 1u][2 * dst] = c0; b.cold[cur ^ 1u][2 * dst + 1] = c1;
	}
	if (ev) {
		const uint64_t e = (uint64_t)b.st->ev_base + off.y + (uint32_t)__popcll(me & below);
		if (e < b.ev_cap) b.events[e] = particle_event(c1, w.x, A, __uint_as_float(w.y));      // (what does not fit is counted in n_events, not written)
	}
}

SGP_DEV void particle_store(const PsBufs& b, uint32_t cur, uint32_t slot, const sgp_particle& p)
{
	b.hot[cur][2 * (size_t)slot] = make_float4(p.pos[0], p.pos[1], p.pos[2], p.width);
	b.hot[cur][2 * (size_t)slot + 1] = make_float4(p.vel[0], p.vel[1], p.vel[2], p.opacity);
	b.cold[cur][2 * (size_t)slot] = make_uint4(__float_as_uint(p.area), __float_as_uint(p.mass), __float_as_uint(p.restitution), __float_as_uint(p.dwidth_dt));
	b.cold[cur][2 * (size_t)slot + 1] = make_uint4(__float_as_uint(p.dopacity_dt), p.flags, (uint32_t)p.tag, (uint32_t)(p.tag >> 32));
}

// addParticle, n at a time.  Newcomer k < fit goes behind the live particles; the other m = n - fit replace the slots (cursor + j) % capacity, j = k - fit,
// each raising a REPLACED event at n_events + j.  Every lane works from the counts the launch found (k_particles_append_commit moves them afterwards), and no
// slot is written by two lanes: a newcomer whose slot a later newcomer of the same call replaces leaves the write to that one, which reports it from the
// staged record -- what adding them one after the other would have done.
__global__ void __launch_bounds__(256) k_particles_append(PsBufs b, uint32_t cur, const sgp_particle* recs, uint32_t n)
{
	const uint32_t k = blockIdx.x * 256u + threadIdx.x;
	if (k >= n) return;
	const uint32_t cap = b.cap, n_old = min(b.st->n_live, cap), cursor = b.st->cursor % cap;
	const uint32_t fit = min(n, cap - n_old), m = n - fit;
	if (k < fit) {
		const uint32_t slot = n_old + k;
		const uint32_t rel = slot >= cursor ? slot - cursor : slot + (cap - cursor);
		if (rel < m) return;
		particle_store(b, cur, slot, recs[k]);
		return;
	}
	const uint32_t j = k - fit, slot = (cursor + j) % cap;      // (n <= cap: the m slots are distinct)
	sgp_particle_event e;
	if (slot >= n_old) {
		const sgp_particle& o = recs[slot - n_old];
		e.tag = o.tag; e.pos[0] = o.pos[0]; e.pos[1] = o.pos[1]; e.pos[2] = o.pos[2]; e.width = o.width;
		e.kind = SGP_PARTICLE_EV_REPLACED; e.foam_width = 0.0f;
	}
	else e = particle_event(b.cold[cur][2 * (size_t)slot + 1], SGP_PARTICLE_EV_REPLACED, b.hot[cur][2 * (size_t)slot], 0.0f);
	const uint64_t at = (uint64_t)b.st->n_events + j;
	if (at < b.ev_cap) b.events[at] = e;
	particle_store(b, cur, slot, recs[k]);
}
__global__ void k_particles_append_commit(PsBufs b, uint32_t n)
{
	const uint32_t cap = b.cap, n_old = min(b.st->n_live, cap), cursor = b.st->cursor % cap;
	const uint32_t fit = min(n, cap - n_old), m = n - fit, ne = b.st->n_events;
	b.st->n_live = n_old + fit;
	b.st->cursor = (cursor + m) % cap;
	b.st->n_events = ne + min(m, 0xFFFFFFFFu - ne);
}

// The same append for records the device made (sgp_crafts_update): their count comes from device memory, the grid covers the host's upper bound of it.  Lane for
// lane what k_particles_append / k_particles_append_commit do with that count.
__global__ void __launch_bounds__(256) k_particles_append_device(PsBufs b, uint32_t cur, const sgp_particle* recs, const uint32_t* n_dev)
{
	const uint32_t k = blockIdx.x * 256u + threadIdx.x;
	const uint32_t cap = b.cap, n = min(*n_dev, cap);
	if (k >= n) return;
	const uint32_t n_old = min(b.st->n_live, cap), cursor = b.st->cursor % cap;
	const uint32_t fit = min(n, cap - n_old), m = n - fit;
	if (k < fit) {
		const uint32_t slot = n_old + k;
		const uint32_t rel = slot >= cursor ? slot - cursor : slot + (cap - cursor);
		if (rel < m) return;
		particle_store(b, cur, slot, recs[k]);
		return;
	}
	const uint32_t j = k - fit, slot = (cursor + j) % cap;
	sgp_particle_event e;
	if (slot >= n_old) {
		const sgp_particle& o = recs[slot - n_old];
		e.tag = o.tag; e.pos[0] = o.pos[0]; e.pos[1] = o.pos[1]; e.pos[2] = o.pos[2]; e.width = o.width;
		e.kind = SGP_PARTICLE_EV_REPLACED; e.foam_width = 0.0f;
	}
	else e = particle_event(b.cold[cur][2 * (size_t)slot + 1], SGP_PARTICLE_EV_REPLACED, b.hot[cur][2 * (size_t)slot], 0.0f);
	const uint64_t at = (uint64_t)b.st->n_events + j;
	if (at < b.ev_cap) b.events[at] = e;
	particle_store(b, cur, slot, recs[k]);
}
__global__ void k_particles_append_device_commit(PsBufs b, const uint32_t* n_dev)
{
	const uint32_t cap = b.cap, n = min(*n_dev, cap), n_old = min(b.st->n_live, cap), cursor = b.st->cursor % cap;
	const uint32_t fit = min(n, cap - n_old), m = n - fit, ne = b.st->n_events;
	b.st->n_live = n_old + fit;
	b.st->cursor = (cursor + m) % cap;
	b.st->n_events = ne + min(m, 0xFFFFFFFFu - ne);
}

__global__ void __launch_bounds__(256) k_particles_pack(PsBufs b, uint32_t cur, uint32_t upper, sgp_particle_state* out)
{
	const uint32_t i = blockIdx.x * 256u + threadIdx.x;
	if (i >= min(min(b.st->n_live, b.cap), upper)) return;
	const float4 A = b.hot[cur][2 * (size_t)i], B = b.hot[cur][2 * (size_t)i + 1];
	const uint4 c1 = b.cold[cur][2 * (size_t)i + 1];
	sgp_particle_state s;
	s.pos[0] = A.x; s.pos[1] = A.y; s.pos[2] = A.z; s.width = A.w;
	s.vel[0] = B.x; s.vel[1] = B.y; s.vel[2] = B.z; s.opacity = B.w;
	s.tag = (uint64_t)c1.z | ((uint64_t)c1.w << 32); s.flags = c1.y; s.reserved_ = 0u;
	out[i] = s;
}

void launch_particles_update(const DV& d, const PsBufs& b, uint32_t cur, uint32_t upper, float dt, int water_enabled, float water_z, hipStream_t s)
{
	if (!upper) return;
	const uint32_t blocks = (upper + 63u) / 64u;
	hipLaunchKernelGGL(k_particles_update, dim3(blocks), dim3(64), 0, s, d, b, cur, dt, water_enabled, water_z);
	hipLaunchKernelGGL(k_particles_scan, dim3(1), dim3(PS_SCAN_THREADS), 0, s, b);
	hipLaunchKernelGGL(k_particles_scatter, dim3(blocks), dim3(64), 0, s, b, cur);
}
void launch_particles_append(const PsBufs& b, uint32_t cur, const sgp_particle* recs, uint32_t n, hipStream_t s)
{
	if (!n) return;
	hipLaunchKernelGGL(k_particles_append, dim3((n + 255u) / 256u), dim3(256), 0, s, b, cur, recs, n);
	hipLaunchKernelGGL(k_particles_append_commit, dim3(1), dim3(1), 0, s, b, n);
}
void launch_particles_append_device(const PsBufs& b, uint32_t cur, const sgp_particle* recs, const uint32_t* n_dev, uint32_t bound, hipStream_t s)
{
	if (!bound) return;
	hipLaunchKernelGGL(k_particles_append_device, dim3((bound + 255u) / 256u), dim3(256), 0, s, b, cur, recs, n_dev);
	hipLaunchKernelGGL(k_particles_append_device_commit, dim3(1), dim3(1), 0, s, b, n_dev);
}
void launch_particles_pack(const PsBufs& b, uint32_t cur, uint32_t upper, sgp_particle_state* out, hipStream_t s)
{
	if (upper) hipLaunchKernelGGL(k_particles_pack, dim3((upper + 255u) / 256u), dim3(256), 0, s, b, cur, upper, out);
}
