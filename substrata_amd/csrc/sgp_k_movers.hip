// sgp_k_movers.hip -- A5 -- the batched path and move-to controllers of sgp_movers_* (ObjectPathController::update / ObjectMoveToController::update for a whole
// batch, on the device).  One of the stage files (stage map: sgp_kernels.h).  Kernels first, their launch wrappers at the end.
//
// k_movers_update: a lane per mover slot -- a walker advances along its path and publishes (waypoint_index, dist_along_segment), a move-to mover advances its
// two tracks; the target goes to the body as CMD_MOVE_KINEMATIC of k_apply_cmds gives it (move_kinematic_velocities, sgp_dev_edits.h).
// k_movers_follow: a second launch for the carriages, which walk back from what their leader published in the first -- the reference's topological order.
// No two movers share a body (the host refuses it), no lane reads what another lane of its launch writes: no atomics, no waits.  A few thousand lanes at most,
// a few hundred flops each: the launches are latency-bound and there is nothing here to tune.
#include "sgp_dev_all.h"
#include "sgp_dev_movers.h"

__global__ void __launch_bounds__(64) k_movers_update(DV d, MoverBufs b, float dt)
{
	const uint32_t k = blockIdx.x * 64u + threadIdx.x;
	if (k >= b.n) return;
	const MoverRec* rc = &b.rec[k];
	if (!rc->alive) return;
	if (rc->kind == SGP_MOVER_PATH && rc->leader != SGP_INVALID_ID) return;      // a follower: k_movers_follow
	MoverDyn dy = b.dyn[k];
	if (dy.reset_serial != rc->reset_serial) { mover_apply_host(rc, dy); mover_state_fresh(&b.st[k], rc, dy); }      // a new mover in the slot: the record of the previous one is not its own
	else mover_apply_host(rc, dy);
	uint32_t f;
	if (!mover_body(d, rc, f)) {
		// the body has gone: nothing of it, or of whatever lives in its slot now, is touched
		b.dyn[k] = dy;
		b.st[k].status = SGP_MOVER_ST_BODY_GONE | (dy.pos_active ? SGP_MOVER_ST_POS_ACTIVE : 0u) | (dy.rot_active ? SGP_MOVER_ST_ROT_ACTIVE : 0u);
		return;
	}
	v3 pos, dir = V3(0.0f, 0.0f, 0.0f); quat rot;
	uint32_t status = 0u;
	if (rc->kind == SGP_MOVER_PATH) {
		const uint32_t n = rc->path < b.n_paths ? b.path_n[rc->path] : 0u;
		if (n < 2u || n > (uint32_t)SGP_MOVER_MAX_WAYPOINTS || dy.index >= n) { b.dyn[k] = dy; return; }      // (cannot happen: a path in use is not removed)
		const sgp_path_segment* segs = b.segs + (size_t)rc->path * SGP_MOVER_MAX_WAYPOINTS;
		sgp_path_progress p; p.waypoint_index = dy.index; p.dist_along_segment = dy.dist; p.time_along_segment = dy.time;
		mp_advance(segs, n, &p, dt, SGP_MOVER_MAX_SEGMENTS_PER_UPDATE, &status);
		dy.index = p.waypoint_index; dy.dist = p.dist_along_segment; dy.time = p.time_along_segment;
		mp3 mpos, mdir;
		mp_eval(segs, n, dy.index, dy.dist, &mpos, &mdir);
		pos = mover_v3(mpos); dir = mover_v3(mdir);
		b.pub[k] = make_uint2(dy.index, __float_as_uint(dy.dist));                // controlled_ob->waypoint_index / dist_along_segment
		rot = mover_path_rotation(rc, dir);
	} else {
		if (!dy.pos_active && !dy.rot_active) {      // finished: the reference has dropped it from its active set
			b.dyn[k] = dy;
			b.st[k].status = 0u;
			return;
		}
		mover_moveto(rc, dy, dt, pos, rot);
	}
	dy.update_index++;
	mover_move_body(d, rc->body, f, pos, rot, dt);
	b.dyn[k] = dy;
	mover_state_store(&b.st[k], dy, status, dy.index, dy.dist, dy.time, pos, rot, dir);
}

__global__ void __launch_bounds__(64) k_movers_follow(DV d, MoverBufs b, float dt)
{
	const uint32_t k = blockIdx.x * 64u + threadIdx.x;
	if (k >= b.n) return;
	const MoverRec* rc = &b.rec[k];
	if (!rc->alive || rc->kind != SGP_MOVER_PATH || rc->leader == SGP_INVALID_ID) return;
	MoverDyn dy = b.dyn[k];
	if (dy.reset_serial != rc->reset_serial) { mover_apply_host(rc, dy); mover_state_fresh(&b.st[k], rc, dy); }
	else mover_apply_host(rc, dy);
	uint32_t f;
	if (!mover_body(d, rc, f)) { b.dyn[k] = dy; b.st[k].status = SGP_MOVER_ST_BODY_GONE; return; }
	const uint32_t n = rc->path < b.n_paths ? b.path_n[rc->path] : 0u;
	if (n < 2u || n > (uint32_t)SGP_MOVER_MAX_WAYPOINTS) { b.dyn[k] = dy; return; }      // (cannot happen)
	const sgp_path_segment* segs = b.segs + (size_t)rc->path * SGP_MOVER_MAX_WAYPOINTS;
	uint32_t status = 0u, index = 0u; float dist = 0.0f;
	mp3 mpos, mdir;
	const uint2 lead = rc->leader < b.n ? b.pub[rc->leader] : make_uint2(0u, 0u);
	if (rc->leader_gone || rc->leader >= b.n || lead.x >= n) {      // the object we follow does not exist: waypoint 0 (:468-473)
		status = SGP_MOVER_ST_LEADER_GONE;
		mpos = mp_wp(segs, n, 0); mdir = MP3(1.0f, 0.0f, 0.0f);
	} else {
		index = lead.x; dist = __uint_as_float(lead.y);
		mp_eval_backwards(segs, n, &index, &dist, rc->follow_dist, SGP_MOVER_MAX_SEGMENTS_PER_UPDATE, &status, &mpos, &mdir);
	}
	const v3 pos = mover_v3(mpos), dir = mover_v3(mdir);
	const quat rot = mover_path_rotation(rc, dir);
	dy.update_index++;
	mover_move_body(d, rc->body, f, pos, rot, dt);
	b.dyn[k] = dy;
	mover_state_store(&b.st[k], dy, status, index, dist, 0.0f, pos, rot, dir);
}

void launch_movers_update(const DV& d, const MoverBufs& b, float dt, hipStream_t s) { if (b.n) hipLaunchKernelGGL(k_movers_update, dim3((b.n + 63u) / 64u), dim3(64), 0, s, d, b, dt); }
void launch_movers_follow(const DV& d, const MoverBufs& b, float dt, hipStream_t s) { if (b.n) hipLaunchKernelGGL(k_movers_follow, dim3((b.n + 63u) / 64u), dim3(64), 0, s, d, b, dt); }
