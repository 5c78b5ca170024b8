// sgp_dev_audibility.h -- the pieces of the audibility launches (sgp_k_audibility.hip; included after sgp_dev_all.h and sgp_dev_raycast.h): sums and prefix
// sums of a wave, the prefix sum of the scans' workgroup, the listeners' table in LDS, the muting-key lookup and the 32-byte event store.  The arithmetic is
// sgp_audibility_math.h, shared with the host; every expression is written out in docs/CONTRACT.md 4m, from which tests/audibility_reference.py restates it.
#pragma once
#include "sgp_audibility_math.h"

#define AUD_SCAN_WAVES (AUD_SCAN_WG / 64)

// a body a source or a listener may sit on: alive and no alias slot (the host has refused compound children and ghosts)
SGP_DEV bool aud_body_ok(uint32_t f) { return (f & BF_ALIVE) && !(f & BF_ALIAS); }

// the sum of `v` over the wave (a workgroup of AUD_WG lanes is one wave), in every lane
SGP_DEV uint32_t aud_wave_sum(uint32_t v)
{
	for (int m = 32; m >= 1; m >>= 1) v += (uint32_t)__shfl_xor((int)v, m);
	return v;
}
// exclusive prefix sum over the wave of a per-lane count below 2^bits, one ballot per bit of the count
SGP_DEV uint32_t aud_wave_prefix(uint32_t c, int bits)
{
	const uint64_t below = (1ull << (threadIdx.x & 63u)) - 1ull;
	uint32_t pre = 0u;
	for (int b = 0; b < bits; ++b) pre += (uint32_t)__popcll(__ballot((c >> b) & 1u) & below) << b;
	return pre;
}
// exclusive prefix sum over the scans' workgroup of any 32-bit count, by shuffles inside a wave and one pass over LDS; *total: the sum over the workgroup
SGP_DEV uint32_t aud_scan_prefix(uint32_t c, uint32_t* s, uint32_t* total)
{
	const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
	uint32_t inc = c;
	for (int d = 1; d < 64; d <<= 1) {
		const uint32_t up = (uint32_t)__shfl_up((int)inc, d);
		if (lane >= (uint32_t)d) inc += up;
	}
	__syncthreads();
	if (lane == 63u) s[wave] = inc;
	__syncthreads();
	uint32_t pre = inc - c, t = 0u;
	for (uint32_t w = 0; w < AUD_SCAN_WAVES; ++w) { if (w < wave) pre += s[w]; t += s[w]; }
	*total = t;
	return pre;
}
// the workgroups' counts -> where each starts, AUD_SCAN_PASS counts per pass (saturating: what lies beyond 2^32 - 1 is dropped anyway); returns first + the sum
SGP_DEV uint64_t aud_scan_counts(const uint32_t* counts, uint32_t* offsets, uint32_t n_wg, uint64_t first, uint32_t* s)
{
	uint64_t running = first;
	for (uint32_t base = 0; base < n_wg; base += AUD_SCAN_PASS) {
		const uint32_t i = base + threadIdx.x;
		const uint32_t c = i < n_wg ? counts[i] : 0u;
		uint32_t total = 0u;
		const uint32_t pre = aud_scan_prefix(c, s, &total);
		const uint64_t at = running + pre;
		if (i < n_wg) offsets[i] = at > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)at;
		running += total;
	}
	return running;
}

// the listeners' run records up to the batch's listener capacity into LDS (32 bytes each: 1 KB for 32)
SGP_DEV void aud_load_listeners(const AudBufs& b, AudLstRun* s_run)
{
	const uint32_t* src = (const uint32_t*)b.run; uint32_t* dst = (uint32_t*)s_run;
	const uint32_t words = b.lcap * (uint32_t)(sizeof(AudLstRun) / 4);
	for (uint32_t i = threadIdx.x; i < words; i += AUD_WG) dst[i] = src[i];
}

// is `key` one of the ascending muting keys?
SGP_DEV bool aud_key_mutes(const uint32_t* keys, uint32_t n, uint32_t key)
{
	uint32_t lo = 0u, hi = n;
	while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if (keys[mid] < key) lo = mid + 1u; else hi = mid; }
	return lo < n && keys[lo] == key;
}

// where source k is: a POINT source's record, or the centroid of its body's world AABB as k_prox_test reads it; false: the body has gone
SGP_DEV bool aud_source_pos(const DV& d, const AudRec& rc, float p[3])
{
	if (!(rc.flags & AUD_BODY)) { p[0] = rc.pos[0]; p[1] = rc.pos[1]; p[2] = rc.pos[2]; return true; }
	const uint32_t bi = rc.body < d.cap_bodies ? rc.body : 0u;
	const uint32_t f = d.flags[bi];
	const float4 mn = d.aabb_min[bi], mx = d.aabb_max[bi];
	if ((rc.flags & AUD_GONE) || rc.body >= d.cap_bodies || !aud_body_ok(f)) return false;
	p[0] = (mn.x + mx.x) * 0.5f; p[1] = (mn.y + mx.y) * 0.5f; p[2] = (mn.z + mx.z) * 0.5f;
	return true;
}

// one event record at place `at` of the batch's event buffer -- two 16-byte stores --, or nothing where it does not fit: the dropped ones are the last of the order
SGP_DEV void aud_store_event(const AudBufs& b, uint64_t at, uint32_t kind, uint32_t source, uint32_t listener, float factor, uint64_t tag, uint32_t update)
{
	if (at >= (uint64_t)b.ev_cap) return;
	uint4* q = (uint4*)(b.events + at);
	q[0] = make_uint4(kind, source, listener, __float_as_uint(factor));
	q[1] = make_uint4((uint32_t)tag, (uint32_t)(tag >> 32), update, 0u);
}
