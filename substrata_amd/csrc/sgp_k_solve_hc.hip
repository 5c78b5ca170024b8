// sgp_k_solve_hc.hip -- K7 -- the high colours by connected component: the launch that solves the components laid out by the k_hc_* kernels of sgp_k_solve.hip.
// One of the stage files of the step kernels (stage map: sgp_kernels.h).  A file of its own because it keeps the compiler's pairing of f32 operations,
// which sgp_k_solve.hip is built without (substrata_amd/build.py, SOURCE_FLAGS; docs/KERNELS.md, "f32 pairing").
#include "sgp_dev_all.h"

// A workgroup's components own their movable bodies, so their solver records live in LDS for the whole pass (read once, written once; a
// colour phase is an LDS gather, the arithmetic and an LDS scatter): HC_TABLE hash slots keyed by body id, filled by the lanes themselves.
#define HC_TABLE 1024                 // >= 2 x the bodies a workgroup can meet (one per lane)
template <int MODE, int ROWS = -1> __global__ void __launch_bounds__(HC_TPB) k_solve_hc(const StepCounters* ctr_pre, const uint4* hc_entry_pre, const StepParams* sp_pre, int first_colour, DV d)      // (leading arguments: preloaded with the wave, k_solve_colour; `d` itself stays as passed -- the catch-all below takes it by reference, and a modified copy would live in scratch)
{
	constexpr int RS = MODE == 1 ? 2 : 3;      // float4 per body: velocity half (lin + inverse mass, ang) / pose half (pos + inverse mass, rot, inertia)
	__shared__ float4 s_rec[HC_TABLE * RS];
	__shared__ uint32_t s_key[HC_TABLE];
	__shared__ unsigned long long s_present;
	__shared__ uint32_t s_ticket;
	const int side = (int)(threadIdx.x & 1u);
	const uint32_t pair = threadIdx.x >> 1;
	const uint32_t parity = sp_pre->parity;
	const uint32_t entries = ctr_pre->hc_entries;
	const int n_colours = (int)ctr_pre->n_colours;
	// (k_solve_colour: the buffer resolved once, before the first barrier and any store, under one wait -- except on the layouts with rows, where a constraint half
	// already fills the register file: the resolved pointers cost scalar registers for the whole pass, and the spills of these instances grew with them)
	constexpr bool RESOLVE = MODE == 2 || ROWS == 2;
	if constexpr (RESOLVE) keep_head<MODE == 2 ? CA_LOC : CA_ARMS>(d, parity, entries, (uint32_t)n_colours, MODE == 2 ? d.pose : d.vel, gridDim.x);
	ConstraintArrays resolved;
	if constexpr (RESOLVE) resolved = cur_arrays(d, parity);
	const auto ca = [&]() -> const ConstraintArrays& { if constexpr (RESOLVE) return resolved; else return CUR(d); };
	for (uint32_t e0 = blockIdx.x * HC_WG_PAIRS; e0 < entries; e0 += gridDim.x * HC_WG_PAIRS) {
		__syncthreads();      // (everyone is done with the previous round's table and mask)
		for (uint32_t i = threadIdx.x; i < HC_TABLE; i += HC_TPB) s_key[i] = HC_NONE;
		if (threadIdx.x == 0) s_present = 0ull;
		__syncthreads();
		const uint4 entry = hc_entry_pre[e0 + pair];
		const uint32_t slot = entry.x;
		const bool mine = slot != HC_NONE;
		ConHalf h; PosHalf ph; int my_col = -1;
		uint32_t body = HC_NONE, at = 0; bool owner = false;
		if (mine) {
			my_col = ((int)entry.y >> 8) & 0xFF;
			body = side ? entry.w : entry.z;
			if (MODE == 1) half_load_known<ROWS>(d, ca(), slot, side, (int)entry.y, body, h); else pos_half_load(ca(), slot, side, (int)entry.y, ph);
			if (side == 0) atomicOr(&s_present, 1ull << my_col);
			// this body's LDS slot; the lane that claims it brings the record in
			at = uf_prio(body) & (HC_TABLE - 1);
			for (;;) {
				const uint32_t old = atomicCAS(&s_key[at], HC_NONE, body);
				if (old == HC_NONE) { owner = true; break; }
				if (old == body) break;
				at = (at + 1) & (HC_TABLE - 1);
			}
			if (owner) {
				const float4* g = (MODE == 1 ? d.vel + VEL_F4 * (size_t)body : d.pose + POSE_F4 * (size_t)body);
				s_rec[RS * at] = g[0]; s_rec[RS * at + 1] = g[1];
				if (MODE != 1) s_rec[RS * at + 2] = d.pose[POSE_F4 * (size_t)body + 2];
			}
			if (MODE == 1) h.body = at;
		}
		__syncthreads();
		const unsigned long long present = s_present;
		for (int c = first_colour; c < n_colours; ++c) {
			if (!((present >> c) & 1ull)) continue;
			if (my_col == c) { if (MODE == 1) half_solve<2>(h, side, s_rec, d.dbg_flags); else pos_half_solve(d, ph, side, s_rec + RS * at, V3(s_rec[RS * at + 2])); }
			__syncthreads();
		}
		// the pass's only global stores: impulses and records were read once, above, and are written once, here, through to memory (store_rec, store_rec2;
		// SGP_SOLVER_STORES); the catch-all below walks colours through global memory and keeps plain stores (it comes behind two fences, and a component is
		// solved here or there, never both)
		constexpr int ST = SGP_SOLVER_STORES;
		if (MODE == 1 && mine) half_store<ST>(ca(), slot, side, h);
		float4* const recs = MODE == 1 ? d.vel : d.pose;
		const size_t g = (MODE == 1 ? VEL_F4 : POSE_F4) * (size_t)body;
		if constexpr (ST == ST_WT) {
			const float4 ra = s_rec[RS * at], rb = s_rec[RS * at + 1];      // (every lane comes along, store_rec2: one that owns nothing reads slot 0 and stores nothing)
			store_rec2<ST>(recs, g, ra, rb, owner && ra.w > 0.0f);
		} else if (owner && s_rec[RS * at].w > 0.0f) { recs[g] = s_rec[RS * at]; recs[g + 1] = s_rec[RS * at + 1]; }
	}
	// catch-all: components too large for a workgroup and the overflow colour, by the last workgroup to finish (nothing to do: no ticket either)
	const uint32_t n_big = d.ctr->hc_n_big;
	const uint32_t ofirst = d.cstarts[SGP_OVERFLOW_COLOUR], ocount = d.cstarts[SGP_OVERFLOW_COLOUR + 1] - ofirst;
	if (n_big == 0u && ocount == 0u) return;
	__syncthreads();
	if (threadIdx.x == 0) { __threadfence(); s_ticket = atomicAdd(&d.ctr->hc_done, 1u); }
	__syncthreads();
	if (s_ticket != gridDim.x - 1u) return;
	if (threadIdx.x == 0) d.ctr->hc_done = 0u;      // for the next launch
	__threadfence();          // what the other workgroups wrote (and this compute unit may still hold older copies of)
	// (the rare path below looks the buffer up at each use, CUR(d): resolved pointers kept alive to here spill scalar registers in the pass above)
	if (n_big != 0u && n_big <= (uint32_t)HC_BIG_LIST) {
		// the constraints of the oversized components from their list, up to four per lane pair, colour by colour (constraints of one colour share no
		// movable body: any order).  Searching every colour's whole range for the flag instead cost 140 us per pass for 288 constraints -- a step of
		// 3.7 instead of 2.0 ms whenever one component of the pile outgrew a workgroup.
		uint32_t mine[4]; int mcol[4]; int cnt = 0;
		for (uint32_t e = pair; e < n_big; e += HC_WG_PAIRS) { const uint32_t k = d.hc_big_list[e]; mine[cnt] = k; mcol[cnt] = (int)((con_npc(CUR(d), k) >> 8) & 0xFF); ++cnt; }
		for (int c = first_colour; c < n_colours; ++c) {
#pragma unroll
			for (int j = 0; j < 4; ++j) if (j < cnt && mcol[j] == c) { if (MODE == 1) solve_velocity_pair_t<VEL_F4, ROWS>(d, CUR(d), mine[j], side, d.vel); else solve_position_pair(d, CUR(d), mine[j], side); }
			__syncthreads();
		}
	} else
	for (int c = first_colour; c < n_colours && n_big != 0u; ++c) {
		const uint32_t cb = d.cstarts[c], ce = d.cstarts[c + 1];
		for (uint32_t k = cb + pair; k < ce; k += HC_WG_PAIRS) {
			if (!(con_npc(CUR(d), k) & NPCOL_CATCH_ALL)) continue;
			if (MODE == 1) solve_velocity_pair_t<VEL_F4, ROWS>(d, CUR(d), k, side, d.vel); else solve_position_pair(d, CUR(d), k, side);
		}
		__syncthreads();
	}
	if (ocount == 0u || threadIdx.x >= 2u) return;               // lanes 0 and 1: the two sides of one constraint at a time
	overflow_walk(CUR(d), ofirst, ocount, [&](uint32_t slot) { if (MODE == 1) solve_velocity_pair_t<VEL_F4, ROWS>(d, CUR(d), slot, side, d.vel); else solve_position_pair(d, CUR(d), slot, side); });
}

void launch_solve_hc(const DV& d, int first_colour, uint32_t est, int mode, hipStream_t s, int compact_rows)
{
	// list entries: a component of n constraints takes the next power of two (< 2 n), plus the padding of the classes
	const uint32_t blocks = std::max(1u, std::min(2048u, (2u * est + HC_CLASSES * HC_WG_PAIRS) / HC_WG_PAIRS));
	if (mode == 1) {
		if (compact_rows == 2) hipLaunchKernelGGL((k_solve_hc<1, 2>), dim3(blocks), dim3(HC_TPB), 0, s, (const StepCounters*)d.ctr, (const uint4*)d.hc_entry, (const StepParams*)d.sp, first_colour, d);
		else if (compact_rows) hipLaunchKernelGGL((k_solve_hc<1, 1>), dim3(blocks), dim3(HC_TPB), 0, s, (const StepCounters*)d.ctr, (const uint4*)d.hc_entry, (const StepParams*)d.sp, first_colour, d);
		else hipLaunchKernelGGL((k_solve_hc<1, 0>), dim3(blocks), dim3(HC_TPB), 0, s, (const StepCounters*)d.ctr, (const uint4*)d.hc_entry, (const StepParams*)d.sp, first_colour, d);
	}
	else hipLaunchKernelGGL((k_solve_hc<2, -1>), dim3(blocks), dim3(HC_TPB), 0, s, (const StepCounters*)d.ctr, (const uint4*)d.hc_entry, (const StepParams*)d.sp, first_colour, d);
}
