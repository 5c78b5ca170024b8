// sgp_k_audibility.hip -- A7 -- the batched audio sources of sgp_audibility_* (the range walk of GUIClient.cpp:4512-4543 and the occlusion and muting walk of
// GUIClient.cpp:6973-7034, for up to 32 listeners against a whole batch of sources, on the device).  One of the stage files (stage map: sgp_kernels.h).
// Kernels first, their launch wrapper at the end.
//
// k_aud_listeners: a lane per listener slot -- where the listener is (a host point, or a body's position plus an offset), its zone key (the host's, or the
//   attached proximity batch's observer's) and whether that zone mutes outside audio.  Leaves an AudLstRun for the other launches.
// k_aud_range: a lane per source slot -- the record and the state, then where the source is (a body's flags and two bounds requested together); the
//   listeners' table sits in LDS.  The in-range mask takes the new bits; the bits that changed and the pairs to trace go to a scratch word pair, the
//   pairs to trace are counted per workgroup.
// k_aud_scan_rays: ONE workgroup -- the workgroups' counts become places in the ray list; the update's ray count.
// k_aud_list: a lane per source slot writes its pairs to trace into the ray list, in slot order, then listener order (a ballot prefix over the wave).
// k_aud_rays: a lane per listed pair (striding over the list) builds the pair's ray with the expressions k_aud_range tested it with and runs
//   raycast_any_one; one word out.
// k_aud_fold: a lane per source slot folds its pairs' answers into the occluded mask, runs the mute ramps on the pair table and counts what is to be
//   reported; only a workgroup that has something to report writes its lanes' event words.
// k_aud_scan_events: ONE workgroup -- the counts become places in the event buffer; the batch's event count and update index advance.
// k_aud_emit: the workgroups that counted something write their events, each at its place.
// No atomics, and no workgroup waits for another: the ray list and the events are in slot order whatever the order the workgroups run in.
// docs/KERNELS.md has the traffic per source.
#include "sgp_dev_all.h"
#include "sgp_dev_raycast.h"
#include "sgp_dev_audibility.h"

__global__ void __launch_bounds__(64) k_aud_listeners(DV d, AudBufs b)
{
	const uint32_t l = threadIdx.x;
	if (l >= b.lcap) return;
	const AudLstRec rc = b.lst[l];
	AudLstRun r; memset(&r, 0, sizeof(r));
	if (!rc.alive) { b.run[l] = r; return; }
	AudLstDyn dy = b.lst_dyn[l];
	if (dy.serial != rc.serial) {      // a new listener in the slot
		dy.pos[0] = dy.pos[1] = dy.pos[2] = 0.0f;
		dy.zone_key = SGP_INVALID_ID; dy.mute_outside = 0u; dy.update_index = 0u; dy.status = 0u; dy.serial = rc.serial;
	}
	float p[3] = { rc.pos[0], rc.pos[1], rc.pos[2] };
	if (rc.source == SGP_AUD_LST_BODY) {
		const uint32_t f = (rc.gone || rc.body >= d.cap_bodies) ? 0u : d.flags[rc.body];
		if (!aud_body_ok(f)) {      // the body has gone: the listener stays where it was and its pairs are frozen
			dy.status |= SGP_AUD_LST_ST_BODY_GONE; b.lst_dyn[l] = dy; b.run[l] = r;
			return;
		}
		const float4 bp = d.pose[(size_t)rc.body * POSE_F4];
		p[0] = bp.x + rc.off[0]; p[1] = bp.y + rc.off[1]; p[2] = bp.z + rc.off[2];
	}
	uint32_t key = rc.zone_key, mute = rc.mute_outside ? 1u : 0u;
	if (b.prox_dyn) {      // the key the proximity batch's last launched update left for observer l; in a muting zone?
		const ProxObsDyn pd = b.prox_dyn[l];
		key = pd.serial != 0u ? pd.zone_key : SGP_INVALID_ID;
		mute = (key != SGP_INVALID_ID && aud_key_mutes(b.mute_keys, b.n_mute_keys, key)) ? 1u : 0u;
	}
	r.p[0] = p[0]; r.p[1] = p[1]; r.p[2] = p[2]; r.live = 1u; r.zone_key = key; r.mute_outside = mute; r.ignore_body = rc.ignore_body;
	dy.pos[0] = p[0]; dy.pos[1] = p[1]; dy.pos[2] = p[2]; dy.zone_key = key; dy.mute_outside = mute; dy.update_index++;
	b.run[l] = r;
	b.lst_dyn[l] = dy;
}

__global__ void __launch_bounds__(AUD_WG) k_aud_range(DV d, AudBufs b)
{
	__shared__ AudLstRun s_run[SGP_AUD_MAX_LISTENERS];
	aud_load_listeners(b, s_run);
	const uint32_t k = blockIdx.x * AUD_WG + threadIdx.x;
	AudRec rc; memset(&rc, 0, sizeof(rc));
	uint4 st = make_uint4(0u, 0u, 0u, 0u);
	if (k < b.n) { rc = b.rec[k]; st = b.st[k]; }
	__syncthreads();
	uint32_t trace = 0u;
	if (k < b.n) {
		const uint32_t serial = rc.serial & 0xFFFFu;
		uint32_t status = st.x & 0xFFu, inr = st.y, occ = st.z, valid = st.w, changed = 0u;
		if (((st.x >> AUD_ST_SERIAL_SHIFT) & 0xFFFFu) != serial) { status = 0u; inr = 0u; occ = 0u; valid = 0u; }      // a new source in the slot: as the constructor leaves it
		inr &= ~b.clear_lst; occ &= ~b.clear_lst; valid &= ~b.clear_lst;
		if (rc.flags & AUD_ALIVE) {
			float p[3];
			if (aud_source_pos(d, rc, p)) {
				for (uint32_t live = b.live_lst; live; live &= live - 1u) {      // (a kernel argument: the loop is the same for every lane)
					const uint32_t l = (uint32_t)__ffs((int)live) - 1u, bit = 1u << l;
					const AudLstRun& r = s_run[l];
					if (!r.live) continue;
					const AxGeom g = ax_geom(p[0], p[1], p[2], r.p[0], r.p[1], r.p[2], rc.volume);
					const bool was = (inr & bit) != 0u, now = ax_range(was, g);
					if (now != was) { changed |= bit; inr ^= bit; }
					float dist;
					if (ax_traced(now, g, &dist)) trace |= bit;
				}
				status = 0u;
				b.pos[k] = make_float4(p[0], p[1], p[2], 0.0f);
			} else status = SGP_AUD_ST_BODY_GONE;
		} else { status = 0u; inr = 0u; occ = 0u; valid = 0u; }
		const uint4 out = make_uint4(status | (serial << AUD_ST_SERIAL_SHIFT), inr, occ, valid);
		if (out.x != st.x || out.y != st.y || out.z != st.z || out.w != st.w) b.st[k] = out;
		b.scr[k] = make_uint2(changed, trace);
	}
	const uint32_t total = aud_wave_sum((uint32_t)__popc(trace));
	if (threadIdx.x == 0u) b.wg_rays[blockIdx.x] = total;
}

__global__ void __launch_bounds__(AUD_SCAN_WG) k_aud_scan_rays(AudBufs b, uint32_t n_wg)
{
	__shared__ uint32_t s_sum[AUD_SCAN_WAVES];
	const uint64_t total = aud_scan_counts(b.wg_rays, b.wg_ray_off, n_wg, 0ull, s_sum);
	if (threadIdx.x == 0u) b.state->n_rays = total > (uint64_t)b.ray_cap ? b.ray_cap : (uint32_t)total;      // (never more than the pair table has pairs)
}

__global__ void __launch_bounds__(AUD_WG) k_aud_list(AudBufs b)
{
	if (!b.wg_rays[blockIdx.x]) return;      // (the whole workgroup)
	const uint32_t k = blockIdx.x * AUD_WG + threadIdx.x;
	const uint32_t trace = k < b.n ? b.scr[k].y : 0u;
	const uint32_t pre = aud_wave_prefix((uint32_t)__popc(trace), 6);      // <= 32 per lane: six bits
	uint64_t at = (uint64_t)b.wg_ray_off[blockIdx.x] + pre;
	for (uint32_t bits = trace; bits; bits &= bits - 1u) {
		const uint32_t l = (uint32_t)__ffs((int)bits) - 1u;
		if (at < (uint64_t)b.ray_cap) b.ray_list[at] = (k << 5) | l;
		++at;
	}
}

__global__ void __launch_bounds__(AUD_WG) k_aud_rays(DV d, AudBufs b)
{
	const uint32_t n_rays = b.state->n_rays, stride = gridDim.x * AUD_WG;
	for (uint32_t r = blockIdx.x * AUD_WG + threadIdx.x; r < n_rays; r += stride) {
		const uint32_t e = b.ray_list[r], k = e >> 5, l = e & 31u;
		const float4 p = b.pos[k];
		const AudLstRun ln = b.run[l];
		const AxGeom g = ax_geom(p.x, p.y, p.z, ln.p[0], ln.p[1], ln.p[2], b.rec[k].volume);
		float dist;
		ax_traced(true, g, &dist);
		sgp_ray ry;
		ry.origin[0] = ln.p[0]; ry.origin[1] = ln.p[1]; ry.origin[2] = ln.p[2];
		ax_ray(g, dist, ry.dir, &ry.max_t);
		ry.ignore_id = ln.ignore_body; ry.collidable_only = 0u;
		b.ray_hit[r] = raycast_any_one(d, ry) ? 1u : 0u;
	}
}

__global__ void __launch_bounds__(AUD_WG) k_aud_fold(AudBufs b)
{
	__shared__ AudLstRun s_run[SGP_AUD_MAX_LISTENERS];
	aud_load_listeners(b, s_run);
	const uint32_t k = blockIdx.x * AUD_WG + threadIdx.x;
	const uint2 sc = k < b.n ? b.scr[k] : make_uint2(0u, 0u);
	const uint32_t changed = sc.x, trace = sc.y;
	const uint32_t pre = aud_wave_prefix((uint32_t)__popc(trace), 6);
	__syncthreads();
	uint32_t ev_r = 0u, ev_o = 0u, ev_v = 0u;
	if (changed | trace) {
		const AudRec rc = b.rec[k];
		uint32_t occ_ch = 0u, vol_ch = 0u;
		if (trace) {
			uint4 st = b.st[k];
			const float4 p = b.pos[k];
			uint64_t at = (uint64_t)b.wg_ray_off[blockIdx.x] + pre;
			for (uint32_t bits = trace; bits; bits &= bits - 1u, ++at) {
				const uint32_t l = (uint32_t)__ffs((int)bits) - 1u, bit = 1u << l;
				const AudLstRun& ln = s_run[l];
				const bool hit = at < (uint64_t)b.ray_cap && b.ray_hit[at] != 0u;
				if (hit != ((st.z & bit) != 0u)) { st.z ^= bit; occ_ch |= bit; }
				AudPair* pp = b.pairs + (size_t)k * b.lcap + l;
				AudPair pr;
				AxRamp rm = ax_ramp_fresh();
				if (st.w & bit) { pr = *pp; rm.start = pr.start; rm.end = pr.end; rm.factor = pr.factor; rm.fac_start = pr.fac_start; rm.fac_end = pr.fac_end; }
				const AxGeom g = ax_geom(p.x, p.y, p.z, ln.p[0], ln.p[1], ln.p[2], rc.volume);
				float dist;
				ax_traced(true, g, &dist);
				if (!(rc.flags & SGP_AUD_ONE_SHOT) && ax_ramp_step(rm, ax_mute(ln.mute_outside, rc.zone_key, ln.zone_key), b.cur_time, b.transition)) vol_ch |= bit;
				pr.start = rm.start; pr.end = rm.end; pr.factor = rm.factor; pr.fac_start = rm.fac_start; pr.fac_end = rm.fac_end; pr.dist = dist;
				*pp = pr;
				st.w |= bit;
			}
			b.st[k] = st;
		}
		if (rc.flags & SGP_AUD_WANT_RANGE) ev_r = changed;
		if (rc.flags & SGP_AUD_WANT_OCCLUSION) ev_o = occ_ch;
		if (rc.flags & SGP_AUD_WANT_VOLUME) ev_v = vol_ch;
	}
	const uint32_t total = aud_wave_sum((uint32_t)(__popc(ev_r) + __popc(ev_o) + __popc(ev_v)));
	if (threadIdx.x == 0u) b.wg_counts[blockIdx.x] = total;
	if (total && k < b.n) b.evw[k] = make_uint4(ev_r, ev_o, ev_v, 0u);
}

__global__ void __launch_bounds__(AUD_SCAN_WG) k_aud_scan_events(AudBufs b, uint32_t n_wg)
{
	__shared__ uint32_t s_sum[AUD_SCAN_WAVES];
	const AudState st = *b.state;
	const uint64_t running = aud_scan_counts(b.wg_counts, b.wg_off, n_wg, (uint64_t)st.n_events, s_sum);
	if (threadIdx.x == 0u) {
		AudState out = st;
		out.n_events = running > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)running;
		out.cur_update = st.update_index; out.update_index = st.update_index + 1u;
		*b.state = out;
	}
}

__global__ void __launch_bounds__(AUD_WG) k_aud_emit(AudBufs b)
{
	if (!b.wg_counts[blockIdx.x]) return;      // (the whole workgroup)
	const uint32_t k = blockIdx.x * AUD_WG + threadIdx.x;
	const uint4 e = k < b.n ? b.evw[k] : make_uint4(0u, 0u, 0u, 0u);
	const uint32_t c = (uint32_t)(__popc(e.x) + __popc(e.y) + __popc(e.z));      // <= 3 * 32: seven bits
	const uint32_t pre = aud_wave_prefix(c, 7);
	if (!c) return;
	uint64_t at = (uint64_t)b.wg_off[blockIdx.x] + pre;
	if (at >= (uint64_t)b.ev_cap) return;
	const uint64_t tag = b.tag[k];
	const uint32_t update = b.state->cur_update;
	const uint4 st = b.st[k];
	// by ascending listener, then IN_RANGE or OUT_OF_RANGE, OCCLUDED or UNOCCLUDED, VOLUME
	for (uint32_t bits = e.x | e.y | e.z; bits; bits &= bits - 1u) {
		const uint32_t l = (uint32_t)__ffs((int)bits) - 1u, bit = 1u << l;
		if (e.x & bit) aud_store_event(b, at++, (st.y & bit) ? SGP_AUD_EV_IN_RANGE : SGP_AUD_EV_OUT_OF_RANGE, k, l, 0.0f, tag, update);
		if (e.y & bit) aud_store_event(b, at++, (st.z & bit) ? SGP_AUD_EV_OCCLUDED : SGP_AUD_EV_UNOCCLUDED, k, l, 0.0f, tag, update);
		if (e.z & bit) aud_store_event(b, at++, SGP_AUD_EV_VOLUME, k, l, b.pairs[(size_t)k * b.lcap + l].factor, tag, update);
	}
}

void launch_audibility_update(const DV& d, const AudBufs& b, hipStream_t s)
{
	if (!b.n) return;
	const uint32_t n_wg = (b.n + AUD_WG - 1u) / AUD_WG;
	const uint64_t pairs = (uint64_t)b.n * (uint64_t)__builtin_popcount(b.live_lst);
	const uint32_t ray_wgs = (uint32_t)std::min<uint64_t>((pairs + AUD_WG - 1u) / AUD_WG, (uint64_t)AUD_RAY_WGS);
	hipLaunchKernelGGL(k_aud_listeners, dim3(1), dim3(64), 0, s, d, b);
	hipLaunchKernelGGL(k_aud_range, dim3(n_wg), dim3(AUD_WG), 0, s, d, b);
	hipLaunchKernelGGL(k_aud_scan_rays, dim3(1), dim3(AUD_SCAN_WG), 0, s, b, n_wg);
	hipLaunchKernelGGL(k_aud_list, dim3(n_wg), dim3(AUD_WG), 0, s, b);
	hipLaunchKernelGGL(k_aud_rays, dim3(std::max(ray_wgs, 1u)), dim3(AUD_WG), 0, s, d, b);
	hipLaunchKernelGGL(k_aud_fold, dim3(n_wg), dim3(AUD_WG), 0, s, b);
	hipLaunchKernelGGL(k_aud_scan_events, dim3(1), dim3(AUD_SCAN_WG), 0, s, b, n_wg);
	hipLaunchKernelGGL(k_aud_emit, dim3(n_wg), dim3(AUD_WG), 0, s, b);
}
