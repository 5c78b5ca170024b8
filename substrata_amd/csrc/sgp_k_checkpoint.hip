// sgp_k_checkpoint.hip -- the segmented copy behind sgp_world_checkpoint / sgp_world_rollback, and the reset of what the broad phase keeps from step to step.
// One of the stage files (stage map: sgp_kernels.h).  Kernels first, their launch wrappers at the end.
//
// A checkpoint holds the part of the world's device arrays the next step can read: the body arrays up to the high-water slot, ONE constraint buffer up to
// the contact cache's size, the used part of the hash table, the vehicle records and a few dozen scalars -- some ninety pieces of very different length.
// k_ckpt_copy moves all of them in one launch: the pieces are laid end to end in a space of 16-byte units, the launch grid-strides over that space, and a
// lane finds the piece its unit lies in from a prefix table.  The table comes in as a kernel argument (no upload, nothing whose lifetime the host has to
// watch) and is copied to LDS once per workgroup; a lane's units only ever move forward, so it walks the table forward and never searches.
// 16 bytes per lane (global_load_dwordx4 / global_store_dwordx4 through global-address-space pointers), the four loads of a lane's tile issued back to back
// before the first store, the values kept in registers: no atomics, no LDS staging of data (LDS holds the piece table only, 3.2 KB).  The same kernel runs in
// both directions: the host swaps the two pointer columns.  k_ckpt_copy_counted is the same copy behind a table the workgroup builds from device words.
#include "sgp_dev_all.h"

#define CKPT_TPB 256
#define CKPT_UNROLL 4

typedef uint32_t ckpt_u4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(1))) const ckpt_u4* ckpt_src_t;      // global address space: the compiler emits global_*, not flat_*, accesses
typedef __attribute__((address_space(1))) ckpt_u4* ckpt_dst_t;

// The copy itself, behind the barrier that made the piece table in LDS visible: n pieces, piece i the units [s_start[i], s_start[i + 1]).
static __device__ __forceinline__ void ckpt_copy_units(const uint32_t* s_start, const uint64_t* s_src, const uint64_t* s_dst, const uint32_t n)
{
	const uint32_t total = s_start[n];
	if (!total) return;
	const uint32_t tile = CKPT_TPB * CKPT_UNROLL;
	uint32_t seg = 0;
	// (64-bit loop variable: base + tile must not wrap when the unit space is close to 2^32)
	for (uint64_t base = (uint64_t)blockIdx.x * tile; base < total; base += (uint64_t)gridDim.x * tile) {
		// 1. where the lane's four units come from and go to.  A unit beyond the end (the last tile only) is clamped to the last unit: its load is
		//    harmless and unconditional, its store is skipped -- so the four loads below need no branch and their values stay in registers.
		ckpt_src_t sp[CKPT_UNROLL]; ckpt_dst_t dp[CKPT_UNROLL]; bool live[CKPT_UNROLL];
#pragma unroll
		for (int k = 0; k < CKPT_UNROLL; ++k) {
			const uint64_t u64 = base + (uint64_t)k * CKPT_TPB + threadIdx.x;
			live[k] = u64 < total;
			const uint32_t u = live[k] ? (uint32_t)u64 : total - 1u;
			while (u >= s_start[seg + 1]) ++seg;      // (u < total = s_start[n]: stops at seg < n; empty pieces are stepped over; u never goes back)
			const uint32_t off = u - s_start[seg];
			sp[k] = (ckpt_src_t)s_src[seg] + off;
			dp[k] = (ckpt_dst_t)s_dst[seg] + off;
		}
		// 2. four independent 16-byte loads in flight
		ckpt_u4 v0 = *sp[0], v1 = *sp[1], v2 = *sp[2], v3 = *sp[3];
		asm volatile("" : "+v"(v0), "+v"(v1), "+v"(v2), "+v"(v3));      // (all four are issued here: without it the compiler sinks a load into the branch of its store)
		// 3. the stores
		if (live[0]) *dp[0] = v0;
		if (live[1]) *dp[1] = v1;
		if (live[2]) *dp[2] = v2;
		if (live[3]) *dp[3] = v3;
	}
}

__global__ void __launch_bounds__(CKPT_TPB) k_ckpt_copy(const CkptTable t)
{
	__shared__ uint32_t s_start[SGP_CKPT_MAX_SEGS + 1];
	__shared__ uint64_t s_src[SGP_CKPT_MAX_SEGS];
	__shared__ uint64_t s_dst[SGP_CKPT_MAX_SEGS];
	const uint32_t n = min(t.n, (uint32_t)SGP_CKPT_MAX_SEGS);
	for (uint32_t i = threadIdx.x; i <= n; i += CKPT_TPB) s_start[i] = t.start[i];
	for (uint32_t i = threadIdx.x; i < n; i += CKPT_TPB) { s_src[i] = (uint64_t)t.src[i]; s_dst[i] = (uint64_t)t.dst[i]; }
	__syncthreads();
	ckpt_copy_units(s_start, s_src, s_dst, n);
}

// The counted variant (batch checkpoints): a piece's length may be a word of device memory -- the particles' live count, their event count -- that the host
// does not know without a read-back it must not wait for.  Every workgroup resolves the lengths while it fills LDS: lane i < n loads piece i's word (one
// global load per piece, L2 hits for all workgroups but the first) and clamps it to the host's bound, lane 0 turns the n <= 24 lengths into the prefix table
// (a serial walk over LDS: a scan would cost more barriers than it saves adds), and the copy is the one above.  The grid was sized from the bounds: a
// workgroup whose first tile lies beyond the resolved total finds its loop empty and returns.  No atomics, nothing written but the destinations.
__global__ void __launch_bounds__(CKPT_TPB) k_ckpt_copy_counted(const CkptCountedTable t)
{
	__shared__ uint32_t s_start[SGP_CKPT_MAX_COUNTED + 1];
	__shared__ uint64_t s_src[SGP_CKPT_MAX_COUNTED];
	__shared__ uint64_t s_dst[SGP_CKPT_MAX_COUNTED];
	const uint32_t n = min(t.n, (uint32_t)SGP_CKPT_MAX_COUNTED), i = threadIdx.x;
	if (i < n) {
		uint32_t len = t.bound[i];
		if (t.count[i]) len = (uint32_t)min(((uint64_t)*t.count[i] * t.per[i] + 15u) / 16u, (uint64_t)len);
		s_start[i + 1] = len; s_src[i] = (uint64_t)t.src[i]; s_dst[i] = (uint64_t)t.dst[i];
	}
	__syncthreads();
	if (i == 0) { uint32_t at = 0; s_start[0] = 0; for (uint32_t k = 1; k <= n; ++k) { at += s_start[k]; s_start[k] = at; } }
	__syncthreads();
	ckpt_copy_units(s_start, s_src, s_dst, n);
}

// What the broad phase carries from one step to the next is "what the next grid has to clear" (k_step_begin: the cell tables up to grid_cells_used, the page
// table entries of the tiles that held a slot).  A rollback does not bring those tables back: it clears what the CURRENT state has dirtied -- exactly what the
// next k_step_begin would have cleared -- and afterwards says "nothing to clear" (k_ckpt_grid_done, a launch of its own: every lane above reads the count).
__global__ void __launch_bounds__(CKPT_TPB) k_ckpt_grid_clear(DV d)
{
	const uint32_t tid = blockIdx.x * CKPT_TPB + threadIdx.x, stride = gridDim.x * CKPT_TPB;
	const uint32_t used = min(*d.grid_cells_used, d.table_size) + 4u;
	for (uint32_t i = tid; i < used; i += stride) { d.cell_count[i] = 0; d.cell_fill[i] = 0; }
	for (uint32_t sl = tid; sl < (used - 4u) / 64u; sl += stride) { const uint32_t tl = d.tile_of_slot[sl]; if (tl < d.tile_table_size) d.tile_slot[tl] = BP_TILE_NONE; }
}
__global__ void k_ckpt_grid_done(DV d)
{
	const uint32_t i = threadIdx.x;
	if (i == 0) *d.grid_cells_used = 0u;
	if (i < 6u) d.bounds_acc[i] = i < 3u ? 0x7FFFFFFF : (int)0x80000000;
}

// ---- launch wrappers ----------------------------------------------------------------------------------------------------------------------------------
void launch_ckpt_copy(const CkptTable& t, uint32_t n_cus, hipStream_t s)
{
	if (!t.n || !t.start[t.n]) return;
	const uint32_t tile = CKPT_TPB * CKPT_UNROLL;
	const uint32_t want = (t.start[t.n] + tile - 1u) / tile;
	// a fixed grid of eight workgroups per compute unit (32 waves, each lane with four 16-byte loads in flight: 128 KB requested per CU, well over the ~32-72 KB that
	// cover an HBM miss; measured 5.6 TB/s read + write at config 3, profiles/r08_checkpoint.md); short tables get fewer
	const uint32_t grid = std::min(want, std::max(n_cus, 1u) * 8u);
	hipLaunchKernelGGL(k_ckpt_copy, dim3(grid), dim3(CKPT_TPB), 0, s, t);
}
void launch_ckpt_copy_counted(const CkptCountedTable& t, uint32_t n_cus, hipStream_t s)
{
	uint64_t bound = 0;
	for (uint32_t i = 0; i < t.n; ++i) bound += t.bound[i];
	if (!t.n || !bound) return;
	const uint32_t tile = CKPT_TPB * CKPT_UNROLL;
	// the grid launch_ckpt_copy would take for the bounds: what the device finds may be far less, and then the surplus workgroups return behind their table
	const uint32_t grid = (uint32_t)std::min<uint64_t>((bound + tile - 1u) / tile, std::max(n_cus, 1u) * 8u);
	hipLaunchKernelGGL(k_ckpt_copy_counted, dim3(grid), dim3(CKPT_TPB), 0, s, t);
}
void launch_ckpt_grid_reset(const DV& d, hipStream_t s)
{
	hipLaunchKernelGGL(k_ckpt_grid_clear, dim3(512), dim3(CKPT_TPB), 0, s, d);
	hipLaunchKernelGGL(k_ckpt_grid_done, dim3(1), dim3(64), 0, s, d);
}
