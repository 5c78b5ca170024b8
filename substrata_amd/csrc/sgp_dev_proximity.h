// sgp_dev_proximity.h -- the pieces of the proximity launches (sgp_k_proximity.hip; included after sgp_dev_all.h): the body checks, sums and prefix sums of
// a workgroup of PROX_WG lanes, and the 32-byte event store.  The arithmetic is sgp_proximity_math.h, shared with the host; every expression is written out in
// docs/CONTRACT.md 4l, from which tests/proximity_reference.py restates it.
#pragma once
#include "sgp_proximity_math.h"

#define PROX_WAVES (PROX_WG / 64)

SGP_DEV px3 prox_f4(float4 v) { return PX3(v.x, v.y, v.z); }
// a body an object or an observer may sit on: alive and no alias slot (the host has refused compound children and ghosts)
SGP_DEV bool prox_body_ok(uint32_t f) { return (f & BF_ALIVE) && !(f & BF_ALIAS); }
SGP_DEV uint32_t prox_lane() { return threadIdx.x & 63u; }
SGP_DEV uint32_t prox_wave() { return threadIdx.x >> 6; }

// the sum of `v` over the workgroup, in every lane (s: PROX_WAVES words of LDS, free again after the call)
SGP_DEV uint32_t prox_block_sum(uint32_t v, uint32_t* s)
{
	for (int m = 32; m >= 1; m >>= 1) v += (uint32_t)__shfl_xor((int)v, m);
	__syncthreads();
	if (prox_lane() == 0u) s[prox_wave()] = v;
	__syncthreads();
	uint32_t t = 0u;
	for (uint32_t w = 0; w < PROX_WAVES; ++w) t += s[w];
	return t;
}

// Exclusive prefix sum over the workgroup of a per-lane count below 2^bits, through wave ballots (one per bit of the count) and one pass over LDS:
// returns the lane's offset in the workgroup.
SGP_DEV uint32_t prox_block_prefix_ballot(uint32_t c, int bits, uint32_t* s)
{
	const uint64_t below = (1ull << prox_lane()) - 1ull;
	uint32_t pre = 0u, total = 0u;
	for (int b = 0; b < bits; ++b) {
		const uint64_t bal = __ballot((c >> b) & 1u);
		pre += (uint32_t)__popcll(bal & below) << b;
		total += (uint32_t)__popcll(bal) << b;
	}
	__syncthreads();
	if (prox_lane() == 0u) s[prox_wave()] = total;
	__syncthreads();
	for (uint32_t w = 0; w < prox_wave(); ++w) pre += s[w];
	return pre;
}

// Exclusive prefix sum over the workgroup of any 32-bit count (k_prox_scan: a workgroup's events), by shuffles inside a wave and one pass over LDS;
// *total: the sum over the workgroup.
SGP_DEV uint32_t prox_block_prefix(uint32_t c, uint32_t* s, uint32_t* total)
{
	uint32_t inc = c;
	for (int d = 1; d < 64; d <<= 1) {
		const uint32_t up = (uint32_t)__shfl_up((int)inc, d);
		if (prox_lane() >= (uint32_t)d) inc += up;
	}
	__syncthreads();
	if (prox_lane() == 63u) s[prox_wave()] = inc;
	__syncthreads();
	uint32_t pre = inc - c, t = 0u;
	for (uint32_t w = 0; w < PROX_WAVES; ++w) { if (w < prox_wave()) pre += s[w]; t += s[w]; }
	*total = t;
	return pre;
}

// one event record at place `at` of the batch's event buffer -- two 16-byte stores --, or nothing where it does not fit: the dropped ones are the last of the order
SGP_DEV void prox_store_event(const ProxBufs& b, uint64_t at, uint32_t kind, uint32_t object, uint32_t observer, uint32_t zone_key, uint64_t tag, uint32_t update)
{
	if (at >= (uint64_t)b.ev_cap) return;
	uint4* q = (uint4*)(b.events + at);
	q[0] = make_uint4(kind, object, observer, zone_key);
	q[1] = make_uint4((uint32_t)tag, (uint32_t)(tag >> 32), update, 0u);
}
