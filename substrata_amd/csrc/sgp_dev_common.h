// sgp_dev_common.h -- flag accessors, layer table, shape bounds / sleep points, event lists, wave- and block-level slot allocation: what every stage uses.
// Device-inline functions only (no kernels), shared between stage files; included through sgp_dev_all.h, whose order is the dependency order.
#pragma once
#include "sgp_kernels.h"
#include <algorithm>
#include "sgp_device_collide.h"
#include "sgp_device_vehicle.h"
#include "sgp_device_mesh.h"

#define TPB 256

// ---------------------------------------------------------------------------------------------------------------
// small helpers

SGP_DEV const ConstraintArrays& CUR(const DV& d) { return d.ca[d.sp->parity & 1]; }
SGP_DEV const ConstraintArrays& PRV(const DV& d) { return d.ca[(d.sp->parity & 1) ^ 1]; }
// The same buffers resolved ONCE, by value: a kernel calls this at entry, before any store, with the parity it read through its preloaded StepParams pointer
// (one scalar load), and hands the result to the device functions of the solver.  The pointers then live in scalar registers for the whole kernel; CUR(d)
// at every use re-read the parity (after a store the compiler can neither hoist nor scalarise that load) and fetched each pointer from the argument segment
// at an address computed from it -- dependent memory round trips on the chain of every solver launch.  The parity stays a device-side value.
SGP_DEV ConstraintArrays cur_arrays(const DV& d, uint32_t parity)
{
	// member by member, a select between two VALUES: both buffers' pointers are fetched from the argument segment at fixed addresses, beside the parity
	// and everything else the kernel's head asks for, and picked with scalar selects when they are in -- one wait.  (`parity ? d.ca[1] : d.ca[0]` as a struct
	// copy compiles to a select between the two ADDRESSES: the pointer fetch then waits for the parity, a dependent level more.)  Members a kernel
	// does not use cost nothing.
	const bool odd = (parity & 1u) != 0u;
	const ConstraintArrays &a = d.ca[0], &b = d.ca[1];
	const auto pick = [odd](auto pa, auto pb) { return odd ? pb : pa; };      // (by value: `odd ? b.hdr : a.hdr` on the members themselves is a select between two addresses again)
	ConstraintArrays c;
	c.hdr = pick(a.hdr, b.hdr); c.n_fric = pick(a.n_fric, b.n_fric); c.prec = pick(a.prec, b.prec);
#pragma unroll
	for (int i = 0; i < 4; ++i) {
		c.r1b[i] = pick(a.r1b[i], b.r1b[i]); c.r2e[i] = pick(a.r2e[i], b.r2e[i]); c.lam[i] = pick(a.lam[i], b.lam[i]);
		c.efft[i] = pick(a.efft[i], b.efft[i]); c.loc1[i] = pick(a.loc1[i], b.loc1[i]); c.loc2[i] = pick(a.loc2[i], b.loc2[i]);
	}
	return c;
}
// The head of a solver kernel: names, as operands of ONE empty instruction, every scalar the first data loads need -- the resolved pointers the kernel reads, the
// colour's slot range, the base of the body records, the grid size.  The loads and selects that produce them cannot be moved below it; left alone, the compiler moves
// each argument fetch behind the range check, next to its first use, and the head becomes a chain of scalar fetches with a wait each.  Here nothing of it depends on
// anything else of it, so all is requested together, under one wait.
// WHAT: the lever arms, effective masses and impulses (velocity iterations on the layout without rows, the warm start); the impulses alone (velocity iterations on
// rows); the contact points in the bodies' frames (position iterations) -- always with the header and the normal.
enum { CA_ARMS = 1, CA_LAM = 2, CA_LOC = 4 };
#define SGP_KEEP4(a) "s"((a)[0]), "s"((a)[1]), "s"((a)[2]), "s"((a)[3])
template <int WHAT> SGP_DEV void keep_buffer(const ConstraintArrays& c)
{
	if constexpr (WHAT == CA_ARMS) asm volatile("" :: "s"(c.hdr), "s"(c.n_fric), SGP_KEEP4(c.r1b), SGP_KEEP4(c.r2e), SGP_KEEP4(c.efft), SGP_KEEP4(c.lam));
	else if constexpr (WHAT == CA_LAM) asm volatile("" :: "s"(c.hdr), "s"(c.n_fric), SGP_KEEP4(c.lam));
	else asm volatile("" :: "s"(c.hdr), "s"(c.n_fric), SGP_KEEP4(c.loc1), SGP_KEEP4(c.loc2));
}
template <int WHAT> SGP_DEV void keep_head(const DV& d, uint32_t parity, uint32_t first, uint32_t end, const void* records, uint32_t grid)
{
	asm volatile("" :: "s"(parity), "s"(first), "s"(end), "s"(records), "s"(grid));
	if constexpr (WHAT == CA_LAM) asm volatile("" :: "s"(d.rows), "s"(d.cap_manifolds));      // (the rows' base and stride)
	keep_buffer<WHAT>(d.ca[0]);
	keep_buffer<WHAT>(d.ca[1]);
}
// STORE POLICY of a record a LATER launch reads and the storing launch itself never does (docs/KERNELS.md, "Write-through stores": the rule and the audit).
// A plain store leaves the line dirty in the XCD's L2 and the kernel boundary writes it back before the next launch may start; a write-through store (sc1)
// sends the same bytes on while the launch's other waves are still working.  ST_WT is for such records only: the line does not stay in L2, so a lane
// of the same launch that read it again would fetch it from memory.  Kernels that walk several colours in one workgroup keep ST_PLAIN; a device function
// shared between both kinds takes the policy from its caller (template flag, one body for both).
// store_rec<ST>(base, index, v) is base[index] = v.  ST_WT: ONE buffer store of the record's own width (16, 8 or 4 bytes, a vector store) through the compiler's
// raw buffer builtin with the sc1 cache-policy bit -- compiler-visible, so counters and hazards stay the compiler's business, no inline assembly.  `base` must be
// uniform over the wave (an array's base out of the kernel arguments or cur_arrays: it becomes the descriptor in scalar registers; a per-lane pointer would be
// looped over lane by lane) and the record's byte offset must fit 32 bits: every record array does (sgp_world_create: max_bodies < 2^25 records of 64 bytes,
// max_manifolds < 2^28 - 1 records of 16 bytes).  The descriptor is the plain one (stride 0, 2^32 - 1 bytes, raw dword format): its range check never drops a store.
enum { ST_PLAIN = 0, ST_WT = 1 };
// What the solver launches whose stores qualify AND gain run with: the velocity and position instances of k_solve_colour, the pass of k_solve_hc.
// Measured on config 3 (profiles/write_through_stores.md): +2.8 %, a velocity colour launch 6.8 -> 6.4 us -- with a record's two halves in ONE store instruction
// (store_rec2 below); as two stores of one lane the same policy LOST 1.6 %.  -DSGP_SOLVER_STORES=0 builds the plain twin for another measurement
// (tests/test_store_policy_codegen.py holds both).
#ifndef SGP_SOLVER_STORES
#define SGP_SOLVER_STORES ST_WT
#endif
#define SGP_AUX_SC1 16      // cache-policy operand of the buffer builtins: bit 4 = sc1
template <int ST, class T> SGP_DEV void store_rec(T* base, size_t index, const T& v)
{
	static_assert(sizeof(T) == 16 || sizeof(T) == 8 || sizeof(T) == 4, "store_rec: one store instruction per record");
	if constexpr (ST == ST_WT) {
		typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
		typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
		const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc((void*)base, 0, 0xFFFFFFFF, 0x00020000);
		const uint32_t off = (uint32_t)(index * sizeof(T));
		if constexpr (sizeof(T) == 16) { u32x4 x; __builtin_memcpy(&x, &v, 16); __builtin_amdgcn_raw_buffer_store_b128(x, rsrc, off, 0, SGP_AUX_SC1); }
		else if constexpr (sizeof(T) == 8) { u32x2 x; __builtin_memcpy(&x, &v, 8); __builtin_amdgcn_raw_buffer_store_b64(x, rsrc, off, 0, SGP_AUX_SC1); }
		else { uint32_t x; __builtin_memcpy(&x, &v, 4); __builtin_amdgcn_raw_buffer_store_b32(x, rsrc, off, 0, SGP_AUX_SC1); }
	} else base[index] = v;
}
// A record of TWO float4 (base[at], base[at + 1]: 32 contiguous bytes; the velocity half of a solver record, position + rotation of a pose record), stored by a
// lane PAIR (lanes 2k and 2k + 1, each with a record of its own and whether it is to be stored; BOTH lanes must be at the call).  Written through as two 16-byte
// stores of one lane, the halves leave the L2 as two partial writes of 32 bytes each -- WRITE_SIZE per launch doubled (profiles/write_through_stores.md) --, so the
// pair shares the work the other way round: first the even lane's record, its first half by the even lane and its second by the odd lane, then the odd lane's
// record likewise.  One store instruction then carries the 32 contiguous bytes of a record in two neighbouring lanes.  ST_PLAIN: each lane stores its own.
SGP_DEV uint32_t lane_swap1_u(uint32_t x) { return (uint32_t)__builtin_amdgcn_mov_dpp((int)x, 0xB1, 0xF, 0xF, true); }      // (the value lane ^ 1 holds: lane_swap1, sgp_dev_solve.h)
SGP_DEV float4 lane_swap1_f4(float4 v)
{
	return make_float4(__uint_as_float(lane_swap1_u(__float_as_uint(v.x))), __uint_as_float(lane_swap1_u(__float_as_uint(v.y))),
	                   __uint_as_float(lane_swap1_u(__float_as_uint(v.z))), __uint_as_float(lane_swap1_u(__float_as_uint(v.w))));
}
template <int ST> SGP_DEV void store_rec2(float4* base, size_t at, float4 a, float4 b, bool store)
{
	if constexpr (ST == ST_WT) {
		const bool odd = (threadIdx.x & 1u) != 0u;
		const uint32_t mine = (uint32_t)at, other = lane_swap1_u(mine);
		const bool ostore = lane_swap1_u(store ? 1u : 0u) != 0u;
		const float4 oa = lane_swap1_f4(a), ob = lane_swap1_f4(b);
		if (odd ? ostore : store) store_rec<ST_WT>(base, odd ? other + 1u : mine, odd ? ob : a);
		if (odd ? store : ostore) store_rec<ST_WT>(base, odd ? mine + 1u : other, odd ? b : oa);
	} else if (store) { base[at] = a; base[at + 1] = b; }
}
// a constraint's header: the two body ids (8 bytes), np_col, or all of it in one 16-byte load
SGP_DEV uint2 con_ab(const ConstraintArrays& c, size_t k) { return *(const uint2*)(c.hdr + k); }
SGP_DEV int& con_npc(const ConstraintArrays& c, size_t k) { return ((int*)(c.hdr + k))[2]; }
SGP_DEV uint4 con_hdr(const ConstraintArrays& c, size_t k) { return c.hdr[k]; }

SGP_DEV uint32_t f_motion(uint32_t f) { return f & BF_MOTION_MASK; }
SGP_DEV uint32_t f_layer(uint32_t f) { return (f & BF_LAYER_MASK) >> BF_LAYER_SHIFT; }
SGP_DEV uint32_t f_shape(uint32_t f) { return (f & BF_SHAPE_MASK) >> BF_SHAPE_SHIFT; }
SGP_DEV bool f_movable(uint32_t f) { return (f & (BF_ALIVE | BF_ACTIVE)) == (BF_ALIVE | BF_ACTIVE) && f_motion(f) == SGP_MOTION_DYNAMIC; }
// Workgroups are dealt to the eight XCDs in turn (each with an L2 of its own).  For a kernel that walks a list whose neighbours share data -- pairs in
// broad-phase tile order, manifolds, a colour's slots -- workgroup b takes chunk xcd_block() instead of b: one XCD then works through a contiguous
// eighth of the list.  The grid must be a multiple of eight.  (Pays in the colour launches, +2 % on config 3; the streaming kernels k_narrowphase and
// k_setup got SLOWER with it -- 85 -> 93 us, 157 -> 188 us -- and keep the plain order.)
SGP_DEV uint32_t xcd_block() { return (blockIdx.x & 7u) * (gridDim.x >> 3) + (blockIdx.x >> 3); }
SGP_DEV bool f_active_for_pairs(uint32_t f) { return (f & (BF_ALIVE | BF_ACTIVE)) == (BF_ALIVE | BF_ACTIVE) && f_motion(f) != SGP_MOTION_STATIC; }

// MyObjectLayerPairFilter, PhysicsWorld.cpp:160-189
SGP_DEV bool layers_collide(uint32_t l1, uint32_t l2)
{
	if (l1 == SGP_LAYER_NON_MOVING) return l2 == SGP_LAYER_MOVING;
	if (l1 == SGP_LAYER_MOVING) return l2 != SGP_LAYER_NON_MOVING_NON_COLLIDABLE && l2 != SGP_LAYER_MOVING_NON_COLLIDABLE;
	return false;
}

SGP_DEV const sgd_hull* body_hull(const DV& d, float4 sh) { return &d.hulls[(uint32_t)sh.x]; }

SGP_DEV v3 shape_local_half(const DV& d, uint32_t type, float4 sh)
{
	if (type == SGP_SHAPE_MESH) return V3(1.0f, 1.0f, 1.0f);        // (static: never asked for sleep points)
	if (type == SGP_SHAPE_HULL) {
		const sgd_hull* h = body_hull(d, sh);
		return V3(fmaxf(fabsf(h->aabb_min.x), fabsf(h->aabb_max.x)), fmaxf(fabsf(h->aabb_min.y), fabsf(h->aabb_max.y)), fmaxf(fabsf(h->aabb_min.z), fabsf(h->aabb_max.z)));
	}
	if (type == SGP_SHAPE_SPHERE) return V3(sh.x, sh.x, sh.x);
	if (type == SGP_SHAPE_BOX) return V3(sh.x, sh.y, sh.z);
	return V3(sh.x, sh.x, sh.y + sh.x);
}

SGP_DEV float shape_volume(const DV& d, uint32_t type, float4 sh)
{
	if (type == SGP_SHAPE_MESH) return 0.0f;
	if (type == SGP_SHAPE_HULL) return body_hull(d, sh)->volume;
	if (type == SGP_SHAPE_SPHERE) return (4.0f / 3.0f) * 3.14159265358979323846f * sh.x * sh.x * sh.x;
	if (type == SGP_SHAPE_BOX) return 8.0f * sh.x * sh.y * sh.z;
	return 3.14159265358979323846f * sh.x * sh.x * (2.0f * sh.y) + (4.0f / 3.0f) * 3.14159265358979323846f * sh.x * sh.x * sh.x;
}

SGP_DEV void compute_aabb(const DV& d, uint32_t type, float4 sh, v3 pos, quat q, v3& mn, v3& mx)
{
	v3 e;
	if (type == SGP_SHAPE_MESH) {
		const MeshHeader mh = d.meshes[(uint32_t)sh.x];
		const m33 R = quat_to_m33(q);
		v3 lo = V3(3.4e38f, 3.4e38f, 3.4e38f), hi = V3(-3.4e38f, -3.4e38f, -3.4e38f);
		for (int k = 0; k < 8; ++k) {
			const v3 c = V3((k & 1) ? mh.mxx : mh.mnx, (k & 2) ? mh.mxy : mh.mny, (k & 4) ? mh.mxz : mh.mnz);
			const v3 p = m33_mul(R, c);
			lo = V3(fminf(lo.x, p.x), fminf(lo.y, p.y), fminf(lo.z, p.z)); hi = V3(fmaxf(hi.x, p.x), fmaxf(hi.y, p.y), fmaxf(hi.z, p.z));
		}
		mn = v3_add(pos, lo); mx = v3_add(pos, hi);
		return;
	}
	if (type == SGP_SHAPE_HULL) {
		const sgd_hull* h = body_hull(d, sh);
		const m33 R = quat_to_m33(q);
		v3 lo = V3(3.4e38f, 3.4e38f, 3.4e38f), hi = V3(-3.4e38f, -3.4e38f, -3.4e38f);
		for (int i = 0; i < h->nv; ++i) {
			const v3 p = m33_mul(R, h->verts[i]);
			lo = V3(fminf(lo.x, p.x), fminf(lo.y, p.y), fminf(lo.z, p.z)); hi = V3(fmaxf(hi.x, p.x), fmaxf(hi.y, p.y), fmaxf(hi.z, p.z));
		}
		mn = v3_add(pos, lo); mx = v3_add(pos, hi);
		return;
	}
	if (type == SGP_SHAPE_SPHERE) e = V3(sh.x, sh.x, sh.x);
	else {
		const m33 R = quat_to_m33(q);
		if (type == SGP_SHAPE_BOX) {
			e = V3(fabsf(R.c0.x) * sh.x + fabsf(R.c1.x) * sh.y + fabsf(R.c2.x) * sh.z,
			       fabsf(R.c0.y) * sh.x + fabsf(R.c1.y) * sh.y + fabsf(R.c2.y) * sh.z,
			       fabsf(R.c0.z) * sh.x + fabsf(R.c1.z) * sh.y + fabsf(R.c2.z) * sh.z);
		} else {
			e = V3(fabsf(R.c2.x) * sh.y + sh.x, fabsf(R.c2.y) * sh.y + sh.x, fabsf(R.c2.z) * sh.y + sh.x);
		}
	}
	mn = v3_sub(pos, e);
	mx = v3_add(pos, e);
}

// Body::GetSleepTestPoints
SGP_DEV void sleep_points(const DV& d, uint32_t type, float4 sh, v3 pos, quat q, v3 out[3])
{
	const v3 ext = shape_local_half(d, type, sh);
	const m33 R = quat_to_m33(q);
	int lowest = 0;
	if (ext.y < v3_get(ext, lowest)) lowest = 1;
	if (ext.z < v3_get(ext, lowest)) lowest = 2;
	const int i1 = lowest == 0 ? 1 : 0;
	const int i2 = lowest == 2 ? 1 : 2;
	out[0] = pos;
	out[1] = v3_add(pos, v3_scale(m33_col(R, i1), v3_get(ext, i1)));
	out[2] = v3_add(pos, v3_scale(m33_col(R, i2), v3_get(ext, i2)));
}

SGP_DEV void reset_sleep(const DV& d, uint32_t i, uint32_t type, float4 sh, v3 pos, quat q)
{
	v3 p[3];
	sleep_points(d, type, sh, pos, q, p);
	d.sleep_s[0][i] = F4(p[0], 0.0f);
	d.sleep_s[1][i] = F4(p[1], 0.0f);
	d.sleep_s[2][i] = F4(p[2], 0.0f);
	d.sleep_timer[i] = 0.0f;
}

SGP_DEV void push_event(uint32_t* list, uint32_t* counter, uint32_t cap, uint32_t id)
{
	const uint32_t k = atomicAdd(counter, 1u);
	if (k < cap) list[k] = id;
}

// One workgroup of the step's last launch: the step's counters, the event counters and the head of each body-event list go to host-mapped memory,
// where the host finds them after its wait.  All of it was final before that launch started.
SGP_DEV void step_end_block(const DV& d, StepCounters* host_mapped, EventWindow* host_events)
{
	const uint32_t* src = (const uint32_t*)d.ctr;
	uint32_t* dst = (uint32_t*)host_mapped;
	for (uint32_t i = threadIdx.x; i < sizeof(StepCounters) / 4; i += blockDim.x) dst[i] = src[i];
	__syncthreads();
	if (threadIdx.x < sizeof(EventCounters) / 4) ((uint32_t*)&host_events->c)[threadIdx.x] = ((const uint32_t*)d.evc)[threadIdx.x];
	const uint32_t win = min(min(d.ev_window, SGP_EVENT_WINDOW), d.cap_bodies);
	const uint32_t* lists[3] = { d.ev_activated, d.ev_deactivated, d.ev_water };
	const uint32_t counts[3] = { d.evc->n_activated, d.evc->n_deactivated, d.evc->n_water };
	for (int l = 0; l < 3; ++l) {
		if (counts[l] > win) continue;      // (the host fetches a longer list itself)
		for (uint32_t i = threadIdx.x; i < counts[l]; i += blockDim.x) host_events->ids[l][i] = lists[l][i];
	}
}

// "The last workgroup to finish does what needs everybody's results": every thread of the workgroup calls this at the end of the kernel's parallel part;
// true (for the whole workgroup) in the workgroup that took the last ticket.  The tickets live in StepCounters (zeroed by the step's first launch) and
// are used once per step each.  A dependent kernel boundary costs ~4.5 us at the launch floor; this costs a fence and an atomic.
SGP_DEV bool last_block(uint32_t* ticket)
{
	__shared__ uint32_t s_last_ticket;
	__syncthreads();
	if (threadIdx.x == 0) { __threadfence(); s_last_ticket = atomicAdd(ticket, 1u); }
	__syncthreads();
	const bool last = s_last_ticket == gridDim.x - 1u;
	if (last) __threadfence();          // what the other workgroups wrote (and this compute unit may still hold older copies of)
	return last;
}

SGP_DEV int float_to_ordered(float f) { const int i = __float_as_int(f); return i >= 0 ? i : i ^ 0x7FFFFFFF; }
SGP_DEV float ordered_to_float(int i) { return __int_as_float(i >= 0 ? i : i ^ 0x7FFFFFFF); }

// ---------------------------------------------------------------------------------------------------------------
// launch wrappers

static inline uint32_t blocks_for(uint32_t n) { return n ? (n + TPB - 1) / TPB : 1; }
static inline uint32_t stride_grid(uint32_t estimate) { uint32_t b = blocks_for(estimate); if (b < 64) b = 64; if (b > 4096) b = 4096; return (b + 7u) & ~7u; }      // (a multiple of eight: xcd_block)
