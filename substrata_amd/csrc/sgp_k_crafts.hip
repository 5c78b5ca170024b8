// sgp_k_crafts.hip -- A7 -- the batched hover cars and boats of sgp_crafts_* (HoverCarPhysics::update / BoatPhysics::update for a whole batch, on the device).
// One of the stage files (stage map: sgp_kernels.h).  Kernels first, their launch wrappers at the end.
//
// k_crafts_update: a lane per craft -- the body's records, the reference's arithmetic (sgp_dev_crafts.h), the forces into the body's accumulators, the state
// record, the particles the update makes into the craft's own staging slots.  No two crafts share a body (the host refuses it), so no atomics.
// k_crafts_scan (one workgroup) + k_crafts_compact lay those particles end to end in ascending craft order; the particles' own append takes them from there
// with their count in device memory (launch_particles_append_device).
#include "sgp_dev_all.h"
#include "sgp_dev_raycast.h"
#include "sgp_dev_crafts.h"

SGP_DEV void craft_state_store(sgp_craft_state* out, const CraftDyn& dy, const CraftAcc* acc, const CraftOut& o, uint32_t n_emit, uint32_t status)
{
	sgp_craft_state s;
	s.force[0] = acc ? acc->sumF.x : 0.0f; s.force[1] = acc ? acc->sumF.y : 0.0f; s.force[2] = acc ? acc->sumF.z : 0.0f;
	s.torque[0] = acc ? acc->sumT.x : 0.0f; s.torque[1] = acc ? acc->sumT.y : 0.0f; s.torque[2] = acc ? acc->sumT.z : 0.0f;
	s.branches = o.branches; s.unflip_time_remaining = dy.unflip; s.righting_time_remaining = dy.righting;
	s.trace_origin[0] = o.trace_origin.x; s.trace_origin[1] = o.trace_origin.y; s.trace_origin[2] = o.trace_origin.z;
	s.trace_t = o.trace_t; s.trace_body = o.trace_body; s.n_emitted = n_emit; s.status = status; s.update_index = dy.update_index; s.reserved_ = 0u;
	*out = s;
}

__global__ void __launch_bounds__(64) k_crafts_update(DV d, CraftBufs b, float dt, int water_enabled, float water_z)
{
	const uint32_t k = blockIdx.x * 64u + threadIdx.x;
	if (k >= b.n) return;
	const CraftRec* rc = &b.rec[k];
	if (!rc->alive) { b.n_emit[k] = 0u; return; }
	CraftDyn dy = b.dyn[k];
	craft_apply_host(rc, dy);
	CraftOut o; o.branches = 0u; o.wake = false; o.trace_origin = V3(0.0f, 0.0f, 0.0f); o.trace_t = 0.0f; o.trace_body = SGP_INVALID_ID;
	const uint32_t i = rc->body;
	uint32_t f = (rc->gone || i >= d.cap_bodies) ? 0u : d.flags[i];
	if (!(f & BF_ALIVE) || (f & BF_ALIAS) || f_motion(f) != SGP_MOTION_DYNAMIC) {
		// the body has gone: nothing of it, or of whatever lives in its slot now, is touched
		b.dyn[k] = dy; b.n_emit[k] = 0u;
		craft_state_store(&b.st[k], dy, nullptr, o, 0u, SGP_CRAFT_ST_BODY_GONE);
		return;
	}
	const CraftIn in = b.in[k];
	const float4 p0 = d.pose[POSE_F4 * (size_t)i], p1 = d.pose[POSE_F4 * (size_t)i + 1];
	const v3 lin_vel = V3(d.vel[VEL_F4 * (size_t)i]), ang_vel = V3(d.vel[VEL_F4 * (size_t)i + 1]);
	const quat q = Q4(p1);
	const CraftFrame fr = craft_frame(rc, V3(p0), q);
	const float4 F0 = d.force[i], T0 = d.torque[i];
	CraftAcc acc; acc.F = V3(F0); acc.T = V3(T0); acc.sumF = V3(0.0f, 0.0f, 0.0f); acc.sumT = V3(0.0f, 0.0f, 0.0f); acc.pos = V3(p0); acc.any = false;
	sgp_particle* slots = b.emit + (size_t)k * SGP_CRAFT_MAX_EMIT;
	uint32_t n_emit = 0u;
	if (rc->kind == SGP_CRAFT_BOAT) craft_boat(d, rc, in, dy, fr, q, lin_vel, ang_vel, d.submerged[i], dt, water_enabled, water_z, k, acc, o, slots, n_emit);
	else if (in.flags & SGP_CRAFT_IN_DRIVER) craft_hovercar(d, rc, in, dy, fr, q, lin_vel, ang_vel, dt, water_enabled, water_z, k, acc, o, slots, n_emit);
	dy.update_index++;

	if (o.wake) f = activate_body(d, i, f);                        // ActivateBody
	if (acc.any) {
		d.force[i] = F4(acc.F, F0.w); d.torque[i] = F4(acc.T, T0.w);
		f = activate_body(d, i, f) | BF_HAS_FORCE;
	}
	if (o.wake || acc.any) d.flags[i] = f;
	b.dyn[k] = dy; b.n_emit[k] = n_emit;
	craft_state_store(&b.st[k], dy, &acc, o, n_emit, 0u);
}

// exclusive scan of the per-craft counts by one workgroup (every thread a run of consecutive crafts), laid out like k_particles_scan; the total at emit_off[n]
__global__ void __launch_bounds__(CRAFT_SCAN_THREADS) k_crafts_scan(CraftBufs b)
{
	__shared__ uint32_t part[CRAFT_SCAN_THREADS];
	const uint32_t n = b.n, t = threadIdx.x;
	const uint32_t per = (n + CRAFT_SCAN_THREADS - 1u) / CRAFT_SCAN_THREADS, lo = min(t * per, n), hi = min(lo + per, n);
	uint32_t sum = 0u;
	for (uint32_t k = lo; k < hi; ++k) sum += min(b.n_emit[k], (uint32_t)SGP_CRAFT_MAX_EMIT);
	part[t] = sum;
	__syncthreads();
	for (uint32_t off = 1; off < CRAFT_SCAN_THREADS; off <<= 1) {
		uint32_t v = part[t];
		if (t >= off) v += part[t - off];
		__syncthreads();
		part[t] = v;
		__syncthreads();
	}
	uint32_t run = t ? part[t - 1] : 0u;
	for (uint32_t k = lo; k < hi; ++k) { b.emit_off[k] = run; run += min(b.n_emit[k], (uint32_t)SGP_CRAFT_MAX_EMIT); }
	if (t == CRAFT_SCAN_THREADS - 1u) b.emit_off[n] = part[t];
}

__global__ void __launch_bounds__(256) k_crafts_compact(CraftBufs b)
{
	const uint32_t g = blockIdx.x * 256u + threadIdx.x;
	const uint32_t k = g / SGP_CRAFT_MAX_EMIT, e = g % SGP_CRAFT_MAX_EMIT;
	if (k >= b.n || e >= min(b.n_emit[k], (uint32_t)SGP_CRAFT_MAX_EMIT)) return;
	b.dense[(size_t)b.emit_off[k] + e] = b.emit[(size_t)k * SGP_CRAFT_MAX_EMIT + e];      // (emit_off[k] + e < n * SGP_CRAFT_MAX_EMIT: the size of dense)
}

__global__ void __launch_bounds__(TPB) k_crafts_sync(CraftBufs b)
{
	const uint32_t k = blockIdx.x * TPB + threadIdx.x;
	if (k >= b.n) return;
	const CraftRec* rc = &b.rec[k];
	if (!rc->alive) return;
	CraftDyn dy = b.dyn[k];
	const uint32_t seen = dy.reset_serial;
	craft_apply_host(rc, dy);
	b.dyn[k] = dy;
	if (seen != dy.reset_serial) {      // a new craft in the slot: the state of the previous one is not its own
		CraftOut o; o.branches = 0u; o.wake = false; o.trace_origin = V3(0.0f, 0.0f, 0.0f); o.trace_t = 0.0f; o.trace_body = SGP_INVALID_ID;
		craft_state_store(&b.st[k], dy, nullptr, o, 0u, 0u);
	}
	else { b.st[k].unflip_time_remaining = dy.unflip; b.st[k].righting_time_remaining = dy.righting; }
}

void launch_crafts_update(const DV& d, const CraftBufs& b, float dt, int water_enabled, float water_z, hipStream_t s)
{
	if (b.n) hipLaunchKernelGGL(k_crafts_update, dim3((b.n + 63u) / 64u), dim3(64), 0, s, d, b, dt, water_enabled, water_z);
}
void launch_crafts_gather(const CraftBufs& b, hipStream_t s)
{
	if (!b.n) return;
	hipLaunchKernelGGL(k_crafts_scan, dim3(1), dim3(CRAFT_SCAN_THREADS), 0, s, b);
	hipLaunchKernelGGL(k_crafts_compact, dim3((b.n * SGP_CRAFT_MAX_EMIT + 255u) / 256u), dim3(256), 0, s, b);
}
void launch_crafts_sync(const CraftBufs& b, hipStream_t s) { if (b.n) hipLaunchKernelGGL(k_crafts_sync, dim3(blocks_for(b.n)), dim3(TPB), 0, s, b); }
