// sgp_k_proximity.hip -- A7 -- the batched proximity and zone watchers of sgp_proximity_* (ScriptedObjectProximityChecker::think and the parcel enter / exit
// walks of GUIClient.cpp:6874-6968, for up to 32 observers against a whole batch of watched objects, on the device).  One of the stage files (stage map:
// sgp_kernels.h).  Kernels first, their launch wrapper at the end.
//
// k_prox_observers: a workgroup per observer slot -- where the observer is (a host point, or a body's position plus an offset) and which zone it stands in:
//   the zone it was in if that is live and still contains it, else the live zone of the lowest key that contains it (the lanes share the zone table; one
//   minimum over the workgroup).  Leaves a ProxObsRun for the other three launches.
// k_prox_test: a lane per object slot -- the record and the state in one load each, then the body's flags and its two bounds requested together; the
//   observers' 3 KB table sits in LDS (every lane reads the same entry: a broadcast).  The near mask takes the new bits; what is to be reported is counted,
//   and only a workgroup that has something to report writes its lanes' event words.
// k_prox_scan: ONE workgroup -- writes the observer-level zone records, then turns the workgroups' counts into places in the event buffer, PROX_SCAN_PASS
//   counts per pass of its loop, and advances the batch's event count and update index.
// k_prox_emit: the workgroups that counted something write their events, each at its place: a prefix sum over the lanes' counts through wave ballots.
// No atomics, and no workgroup waits for another: the order of the events is the order of the slots, whatever the order the workgroups run in.
// Steady state (no transition) moves per object 16 (record) + 8 (state) + 4 (flags) + 32 (bounds) bytes in and 4 / PROX_WG out; k_prox_emit then ends after
// one 4-byte load per workgroup.  docs/KERNELS.md has the table.
#include "sgp_dev_all.h"
#include "sgp_dev_proximity.h"

__global__ void __launch_bounds__(PROX_WG) k_prox_observers(DV d, ProxBufs b)
{
	__shared__ unsigned long long s_best[PROX_WAVES];
	const uint32_t o = blockIdx.x;
	const ProxObsRec rc = b.obs[o];
	if (!rc.alive) { if (threadIdx.x == 0u) b.run[o].live = 0u; return; }
	ProxObsDyn dy = b.obs_dyn[o];
	if (dy.serial != rc.serial) {      // a new observer in the slot: near nothing (the host has cleared its bit), in no zone
		dy.pos[0] = dy.pos[1] = dy.pos[2] = 0.0f;
		dy.zone = SGP_INVALID_ID; dy.zone_gen = 0u; dy.zone_key = SGP_INVALID_ID; dy.update_index = 0u; dy.status = 0u; dy.serial = rc.serial;
	}
	px3 p = PX3(rc.pos);
	if (rc.source == SGP_PROX_OBS_BODY) {
		const uint32_t f = (rc.gone || rc.body >= d.cap_bodies) ? 0u : d.flags[rc.body];
		if (!prox_body_ok(f)) {      // the body has gone: the observer stays where it was and is not tested any more
			if (threadIdx.x == 0u) { dy.status |= SGP_PROX_OBS_ST_BODY_GONE; b.obs_dyn[o] = dy; b.run[o].live = 0u; }
			return;
		}
		const float4 bp = d.pose[(size_t)rc.body * POSE_F4];
		p = PX3(bp.x + rc.off[0], bp.y + rc.off[1], bp.z + rc.off[2]);
	}
	// the zone it was in: still live (the slot's generation is the one it remembers), still around it?
	const bool had = dy.zone != SGP_INVALID_ID;
	ProxZone pz; memset(&pz, 0, sizeof(pz));
	if (had && dy.zone < b.n_zones) pz = b.zones[dy.zone];
	const bool prev_live = had && dy.zone < b.n_zones && pz.gen_live == ((dy.zone_gen << 1) | 1u);
	const bool stays = prev_live && px_contains(PX3(pz.mn), PX3(pz.mx), p);
	uint32_t nz = dy.zone;
	if (!stays) {      // (uniform: every lane holds the same record)
		unsigned long long best = ~0ull;      // key << 32 | slot: keys are unique among live zones
		for (uint32_t z = threadIdx.x; z < b.n_zones; z += PROX_WG) {
			const ProxZone c = b.zones[z];
			if ((c.gen_live & 1u) && px_contains(PX3(c.mn), PX3(c.mx), p)) { const unsigned long long v = ((unsigned long long)c.key << 32) | z; best = v < best ? v : best; }
		}
		for (int m = 32; m >= 1; m >>= 1) { const unsigned long long v = __shfl_xor(best, m); best = v < best ? v : best; }
		if (prox_lane() == 0u) s_best[prox_wave()] = best;
		__syncthreads();
		best = s_best[0];
		for (uint32_t w = 1; w < PROX_WAVES; ++w) best = s_best[w] < best ? s_best[w] : best;
		nz = best == ~0ull ? SGP_INVALID_ID : (uint32_t)best;
	}
	if (threadIdx.x != 0u) return;
	ProxObsRun r; memset(&r, 0, sizeof(r));
	r.p[0] = p.x; r.p[1] = p.y; r.p[2] = p.z; r.live = 1u;
	r.changed = (!stays && (had || nz != SGP_INVALID_ID)) ? 1u : 0u;
	r.prev_ok = prev_live ? 1u : 0u; r.prev_key = dy.zone_key;
	for (int c = 0; c < 3; ++c) { r.pmn[c] = pz.mn[c]; r.pmx[c] = pz.mx[c]; }
	r.cur_key = SGP_INVALID_ID;
	if (!stays) {
		dy.zone = nz; dy.zone_gen = 0u; dy.zone_key = SGP_INVALID_ID;
		if (nz != SGP_INVALID_ID) {
			const ProxZone c = b.zones[nz];
			r.cur_ok = 1u; r.cur_key = c.key;
			for (int k = 0; k < 3; ++k) { r.cmn[k] = c.mn[k]; r.cmx[k] = c.mx[k]; }
			dy.zone_gen = c.gen_live >> 1; dy.zone_key = c.key;
		}
	}
	dy.pos[0] = p.x; dy.pos[1] = p.y; dy.pos[2] = p.z; dy.update_index++;
	b.run[o] = r;
	b.obs_dyn[o] = dy;
}

__global__ void __launch_bounds__(PROX_WG) k_prox_test(DV d, ProxBufs b)
{
	__shared__ ProxObsRun s_run[SGP_PROX_MAX_OBSERVERS];
	__shared__ uint32_t s_sum[PROX_WAVES];
	{
		// the entries up to the highest live observer: 96 bytes per workgroup for a lone observer 0, 3 KB for 32
		const uint32_t* src = (const uint32_t*)b.run; uint32_t* dst = (uint32_t*)s_run;
		const uint32_t words = (32u - (uint32_t)__clz((int)b.live_obs)) * (uint32_t)(sizeof(ProxObsRun) / 4);
		for (uint32_t i = threadIdx.x; i < words; i += PROX_WG) dst[i] = src[i];
	}
	const uint32_t k = blockIdx.x * PROX_WG + threadIdx.x;
	uint32_t changed = 0u, exited = 0u, entered = 0u, mask = 0u;
	uint4 rq = make_uint4(0u, 0u, 0u, 0u); uint2 st = make_uint2(0u, 0u);
	if (k < b.n) { rq = *(const uint4*)(b.rec + k); st = b.st[k]; }
	__syncthreads();
	if (k < b.n) {
		const uint32_t body = rq.x, flags = rq.z, serial = rq.w & 0xFFFFu;
		const float radius = __uint_as_float(rq.y);
		uint32_t status = st.x & 0xFFu;
		mask = st.y;
		if (((st.x >> PROX_ST_SERIAL_SHIFT) & 0xFFFFu) != serial) { status = 0u; mask = 0u; }      // a new object in the slot: near nobody
		mask &= ~b.clear_obs;
		if (flags & PROX_ALIVE) {
			// the flags and the two bounds: three independent gathers, in flight together
			const uint32_t bi = body < d.cap_bodies ? body : 0u;
			const uint32_t f = d.flags[bi];
			const float4 a_mn = d.aabb_min[bi], a_mx = d.aabb_max[bi];
			if (!(flags & PROX_GONE) && body < d.cap_bodies && prox_body_ok(f)) {
				const px3 mn = prox_f4(a_mn), mx = prox_f4(a_mx);
				const px3 c = px_centroid(mn, mx);
				uint32_t now = mask;
				for (uint32_t live = b.live_obs; live; live &= live - 1u) {      // (a kernel argument: the loop is the same for every lane)
					const uint32_t o = (uint32_t)__ffs((int)live) - 1u, bit = 1u << o;
					const ProxObsRun& r = s_run[o];
					if (!r.live) continue;
					const bool near = px_near(px_dist2(mn, mx, PX3(r.p)), radius);
					now = near ? (now | bit) : (now & ~bit);
					if (r.changed && (flags & SGP_PROX_WANT_ZONE)) {
						if (r.prev_ok && px_contains(PX3(r.pmn), PX3(r.pmx), c)) exited |= bit;
						if (r.cur_ok && px_contains(PX3(r.cmn), PX3(r.cmx), c)) entered |= bit;
					}
				}
				if (flags & SGP_PROX_WANT_NEAR) changed = mask ^ now;
				mask = now;      // the mask takes the new bits whether or not the events are wanted (in_script_proximity is set before the handlers are looked at)
				status = 0u;
			} else status = SGP_PROX_ST_BODY_GONE;
		} else { status = 0u; mask = 0u; }
		const uint2 out = make_uint2(status | (serial << PROX_ST_SERIAL_SHIFT), mask);
		if (out.x != st.x || out.y != st.y) b.st[k] = out;
	}
	const uint32_t total = prox_block_sum((uint32_t)(__popc(changed) + __popc(exited) + __popc(entered)), s_sum);
	if (threadIdx.x == 0u) b.wg_counts[blockIdx.x] = total;
	if (total && k < b.n) b.evw[k] = make_uint4(changed, mask, exited, entered);
}

__global__ void __launch_bounds__(PROX_WG) k_prox_scan(ProxBufs b, uint32_t n_wg)
{
	__shared__ uint32_t s_sum[PROX_WAVES];
	const ProxState st = *b.state;
	// the observer-level zone records: by ascending observer, EXITED before ENTERED
	uint32_t ne = 0u;
	ProxObsRun r; r.live = 0u;
	if (threadIdx.x < SGP_PROX_MAX_OBSERVERS && ((b.live_obs >> threadIdx.x) & 1u)) {
		r = b.run[threadIdx.x];
		if (r.live && r.changed) ne = (r.prev_ok ? 1u : 0u) + (r.cur_ok ? 1u : 0u);
	}
	uint32_t n_obs_ev = 0u;
	const uint32_t at_obs = prox_block_prefix(ne, s_sum, &n_obs_ev);
	if (ne) {
		uint64_t at = (uint64_t)st.n_events + at_obs;
		if (r.prev_ok) prox_store_event(b, at++, SGP_PROX_EV_EXITED, SGP_INVALID_ID, threadIdx.x, r.prev_key, 0ull, st.update_index);
		if (r.cur_ok) prox_store_event(b, at, SGP_PROX_EV_ENTERED, SGP_INVALID_ID, threadIdx.x, r.cur_key, 0ull, st.update_index);
	}
	// the objects' events behind them: where each workgroup of k_prox_test starts (saturating: what lies beyond the buffer is dropped anyway)
	uint64_t running = (uint64_t)st.n_events + n_obs_ev;
	for (uint32_t base = 0; base < n_wg; base += PROX_SCAN_PASS) {
		const uint32_t i = base + threadIdx.x;
		const uint32_t c = i < n_wg ? b.wg_counts[i] : 0u;
		uint32_t total = 0u;
		const uint32_t pre = prox_block_prefix(c, s_sum, &total);
		const uint64_t at = running + pre;
		if (i < n_wg) b.wg_off[i] = at > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)at;
		running += total;
	}
	if (threadIdx.x == 0u) {
		ProxState out = st;
		out.n_events = running > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)running;
		out.cur_update = st.update_index; out.update_index = st.update_index + 1u;
		*b.state = out;
	}
}

__global__ void __launch_bounds__(PROX_WG) k_prox_emit(ProxBufs b)
{
	__shared__ uint32_t s_sum[PROX_WAVES];
	if (!b.wg_counts[blockIdx.x]) return;      // (the whole workgroup)
	const uint32_t off = b.wg_off[blockIdx.x];
	const uint32_t k = blockIdx.x * PROX_WG + threadIdx.x;
	const uint4 e = k < b.n ? b.evw[k] : make_uint4(0u, 0u, 0u, 0u);
	const uint32_t c = (uint32_t)(__popc(e.x) + __popc(e.z) + __popc(e.w));      // <= 3 * 32: seven bits
	const uint32_t pre = prox_block_prefix_ballot(c, 7, s_sum);
	if (!c) return;
	uint64_t at = (uint64_t)off + pre;
	if (at >= (uint64_t)b.ev_cap) return;
	const uint64_t tag = b.tag[k];
	const uint32_t update = b.state->cur_update;
	// by ascending observer, then NEAR or AWAY, EXITED, ENTERED
	for (uint32_t bits = e.x | e.z | e.w; bits; bits &= bits - 1u) {
		const uint32_t o = (uint32_t)__ffs((int)bits) - 1u, bit = 1u << o;
		if (e.x & bit) prox_store_event(b, at++, (e.y & bit) ? SGP_PROX_EV_NEAR : SGP_PROX_EV_AWAY, k, o, SGP_INVALID_ID, tag, update);
		if (e.z & bit) prox_store_event(b, at++, SGP_PROX_EV_EXITED, k, o, b.run[o].prev_key, tag, update);
		if (e.w & bit) prox_store_event(b, at++, SGP_PROX_EV_ENTERED, k, o, b.run[o].cur_key, tag, update);
	}
}

void launch_proximity_update(const DV& d, const ProxBufs& b, hipStream_t s)
{
	if (!b.n) return;
	const uint32_t n_wg = (b.n + PROX_WG - 1u) / PROX_WG;
	hipLaunchKernelGGL(k_prox_observers, dim3(SGP_PROX_MAX_OBSERVERS), dim3(PROX_WG), 0, s, d, b);
	hipLaunchKernelGGL(k_prox_test, dim3(n_wg), dim3(PROX_WG), 0, s, d, b);
	hipLaunchKernelGGL(k_prox_scan, dim3(1), dim3(PROX_WG), 0, s, b, n_wg);
	hipLaunchKernelGGL(k_prox_emit, dim3(n_wg), dim3(PROX_WG), 0, s, b);
}
