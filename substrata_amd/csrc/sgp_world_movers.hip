// sgp_world_movers.hip -- the batched path and move-to controllers (ObjectPathController / ObjectMoveToController for many objects): the host side of sgp_movers_*.
// The host keeps the descriptions, the track commands and the prepared paths (uploaded when they change), the slot bookkeeping and which body each mover was
// added on; the walkers' progress, the tracks' clocks and the held poses live on the device and are touched by the kernels of sgp_k_movers.hip alone.  An
// update enqueues and returns.  sgp_path_prepare / sgp_path_advance are sgp_mover_path.h compiled for the host: they need no world and no device.
#include "sgp_world_internal.h"
#include "sgp_mover_path.h"

struct MoverPath { uint32_t n = 0, refs = 0; bool alive = false; double total_time = 0.0; };
struct sgp_movers : WorldBatch {
	BatchSlots slots, path_slots; BodyLinks links;      // (a body carries one mover)
	uint32_t n_followers = 0;
	Mirror<MoverRec> rec; std::vector<uint32_t> leader_serial; std::vector<uint64_t> tag; std::vector<uint8_t> fresh;
	std::vector<MoverPath> paths; Mirror<sgp_path_segment> segs; Mirror<uint32_t> path_n;      // (segs and path_n change together)
	// device
	MoverDyn* d_dyn = nullptr; sgp_mover_state* d_st = nullptr; uint2* d_pub = nullptr;
	// what a checkpoint holds beyond the segs, path_n and rec mirrors
	void ckpt_layout(BatchCkptLayout& l)
	{
		const uint32_t* n = &slots.high;
		l.device(d_dyn, n); l.device(d_st, n); l.device(d_pub, n);
		l.host_array(leader_serial, n); l.host_array(tag, n); l.host_array(fresh, n); l.host_array(paths, &path_slots.high);
		l.scalar(n_followers);
		l.table(slots); l.table(path_slots); l.body_links(links, n);
		l.capacity = slots.cap; l.high = slots.high; l.n_alive = slots.n_alive;
	}
};

static MoverBufs movers_bufs(const sgp_movers* ms)
{
	MoverBufs b;
	b.rec = ms->rec.d(); b.dyn = ms->d_dyn; b.st = ms->d_st; b.pub = ms->d_pub; b.segs = ms->segs.d(); b.path_n = ms->path_n.d(); b.n = ms->slots.high; b.n_paths = ms->path_slots.high;
	return b;
}

SGP_API int sgp_path_prepare(const sgp_path_waypoint* in, uint32_t n, sgp_path_segment* out, double* total_time_out)
{
	if (!in || !out || !total_time_out) return fail(SGP_ERR_INVALID, "sgp_path_prepare: NULL");
	static const char* const what[] = { "", "fewer than 2 or more than SGP_MOVER_MAX_WAYPOINTS waypoints", "a speed that is not finite and > 0, or a pause_time that is not finite and >= 0",
	                                    "an unknown waypoint type", "a near zero length or non-finite segment" };
	const int r = mp_prepare(in, n, out, total_time_out);
	if (r) { char msg[200]; snprintf(msg, sizeof(msg), "sgp_path_prepare: invalid path, %s", what[r]); return fail(SGP_ERR_INVALID, msg); }
	return SGP_OK;
}

SGP_API int sgp_path_advance(const sgp_path_segment* segs, uint32_t n, sgp_path_progress* io, float dt, uint32_t* status_io)
{
	if (!segs || !io || !status_io || n < 2u || io->waypoint_index >= n || !std::isfinite(dt)) return fail(SGP_ERR_INVALID, "sgp_path_advance: NULL, fewer than 2 segments, an index beyond them or a dt that is not finite");
	mp_advance(segs, n, io, dt, SGP_MOVER_MAX_SEGMENTS_PER_UPDATE, status_io);
	return SGP_OK;
}

SGP_API int sgp_movers_destroy(sgp_movers* ms) { return batch_destroy(ms, "sgp_movers_destroy"); }

SGP_API int sgp_movers_create(sgp_world* w, uint32_t capacity, uint32_t path_capacity, sgp_movers** out)
{
	if (!w || !out || capacity == 0 || capacity > SGP_MOVERS_MAX_CAPACITY || path_capacity == 0 || path_capacity > SGP_MOVERS_MAX_PATHS) return fail(SGP_ERR_INVALID, "sgp_movers_create: NULL world or out, a capacity of 0 or beyond 2^16, or a path capacity of 0 or beyond 2^12");
	if (world_holds_ghosts(w)) return fail_ghosts("sgp_movers_create", "movers");
	hipSetDevice(w->device);
	sgp_movers* ms = new sgp_movers();
	const size_t n = capacity;
	ms->slots.cap = capacity; ms->path_slots.cap = path_capacity; ms->links.resize(capacity);
	ms->leader_serial.assign(n, 0u); ms->tag.assign(n, 0ull); ms->fresh.assign(n, 0); ms->paths.resize(path_capacity);
	ms->segs.shape(path_capacity, &ms->path_slots.high, SGP_MOVER_MAX_WAYPOINTS); ms->path_n.shape(path_capacity, &ms->path_slots.high); ms->rec.shape(n, &ms->slots.high);
	bool ok = ms->adopt(w) && ms->create_mirrors({ &ms->segs, &ms->path_n, &ms->rec });      // (the paths go up before the records that name them)
	ok = ok && ms->alloc(ms->d_dyn, n) && ms->alloc(ms->d_st, n) && ms->alloc(ms->d_pub, n);
	return batch_created(ms, ok, out, "sgp_movers_create");
}

static bool path_live(const sgp_movers* ms, uint32_t p) { return p < ms->path_slots.high && ms->paths[p].alive; }

SGP_API int sgp_movers_path_add(sgp_movers* ms, const sgp_path_waypoint* waypoints, uint32_t n, uint32_t* path_id_out)
{
	if (!batch_usable(ms) || !waypoints || !path_id_out) return fail(SGP_ERR_INVALID, "sgp_movers_path_add: NULL, or the batch's world is gone");
	sgp_path_segment prepared[SGP_MOVER_MAX_WAYPOINTS];
	double total = 0.0;
	if (sgp_path_prepare(waypoints, n, prepared, &total) != SGP_OK) return SGP_ERR_INVALID;      // (the message is sgp_path_prepare's)
	if (!(total > 0.0) || !std::isfinite(total)) return fail(SGP_ERR_INVALID, "sgp_movers_path_add: the path's traversal time is not finite and > 0");
	const uint32_t p = ms->path_slots.take();
	if (p == BatchSlots::none) return fail(SGP_ERR_CAPACITY, "sgp_movers_path_add: no free path slot");
	memcpy(&ms->segs[(size_t)p * SGP_MOVER_MAX_WAYPOINTS], prepared, sizeof(sgp_path_segment) * n);
	ms->path_n[p] = n;
	MoverPath& mp = ms->paths[p]; mp.n = n; mp.refs = 0; mp.alive = true; mp.total_time = total;
	ms->segs.dirty = ms->path_n.dirty = true;
	*path_id_out = p;
	return SGP_OK;
}

SGP_API int sgp_movers_path_remove(sgp_movers* ms, uint32_t p)
{
	if (!batch_usable(ms) || !path_live(ms, p)) return fail(SGP_ERR_INVALID, "sgp_movers_path_remove: no such path");
	if (ms->paths[p].refs) return fail(SGP_ERR_INVALID, "sgp_movers_path_remove: the path is in use");
	ms->paths[p].alive = false; ms->path_n[p] = 0u; ms->path_slots.give_back(p);
	ms->segs.dirty = ms->path_n.dirty = true;
	return SGP_OK;
}

SGP_API int sgp_movers_path_get(sgp_movers* ms, uint32_t p, sgp_path_segment* out, uint32_t cap, uint32_t* n_out)
{
	if (!batch_usable(ms) || !path_live(ms, p) || !n_out || (cap && !out)) return fail(SGP_ERR_INVALID, "sgp_movers_path_get: NULL, or no such path");
	*n_out = ms->paths[p].n;
	if (cap) memcpy(out, &ms->segs[(size_t)p * SGP_MOVER_MAX_WAYPOINTS], sizeof(sgp_path_segment) * std::min(cap, ms->paths[p].n));
	return SGP_OK;
}

static bool mover_live(const sgp_movers* ms, uint32_t id) { return id < ms->slots.high && ms->rec[id].alive; }
static bool is_follower(const MoverRec& r) { return r.kind == SGP_MOVER_PATH && r.leader != SGP_INVALID_ID; }
// the bodies that have gone since the last look (the host hands out the slots, so it knows): their movers are marked, the body is free for another mover, and the
// followers of a walker that lost its body lose their leader
static void movers_mark_gone(sgp_movers* ms)
{
	const sgp_world* w = ms->w;
	ms->links.mark_gone(ms->slots.high, [w](uint32_t body) { return body_carries(w, body, SGP_MOTION_KINEMATIC); }, [w](uint32_t body) { return body_born_of(w, body); },
	                    [ms](uint32_t k) { ms->rec[k].gone = 1u; ms->rec.dirty = true; });
	if (!ms->n_followers) return;
	for (uint32_t k = 0; k < ms->slots.high; ++k) {
		MoverRec& r = ms->rec[k];
		if (!r.alive || !is_follower(r) || r.leader_gone) continue;
		const MoverRec& l = ms->rec[r.leader];
		if (l.alive && !l.gone && l.reset_serial == ms->leader_serial[k]) continue;
		r.leader_gone = 1u; ms->rec.dirty = true;
	}
}

static const char* mover_desc_fault(const sgp_movers* ms, const sgp_mover_desc& d)
{
	if (d.kind != SGP_MOVER_PATH && d.kind != SGP_MOVER_MOVETO) return "an unknown kind";
	if (d.flags & ~SGP_MOVER_ORIENT_ALONG_PATH) return "an unknown flag";
	if (d.kind == SGP_MOVER_MOVETO) return (finite3(d.hold_pos) && finite4(d.hold_rot)) ? nullptr : "a non-finite value";
	if (!finite4(d.base_rot) || !std::isfinite(d.initial_time)) return "a non-finite value";
	if (!path_live(ms, d.path)) return "no such path";
	if (d.leader == SGP_INVALID_ID) return nullptr;
	if (!std::isfinite(d.follow_dist) || !(d.follow_dist >= 0.0f)) return "follow_dist must be finite and >= 0";
	if (!mover_live(ms, d.leader) || ms->rec[d.leader].kind != SGP_MOVER_PATH || is_follower(ms->rec[d.leader])) return "the leader is not a live walker of this batch (a follower cannot lead)";
	if (ms->rec[d.leader].path != d.path) return "the leader walks another path";
	return nullptr;
}

SGP_API int sgp_mover_add(sgp_movers* ms, const sgp_mover_desc* desc, uint32_t* id_out)
{
	if (!batch_usable(ms) || !desc || !id_out) return fail(SGP_ERR_INVALID, "sgp_mover_add: NULL, or the batch's world is gone");
	if (const char* what = mover_desc_fault(ms, *desc)) { char msg[160]; snprintf(msg, sizeof(msg), "sgp_mover_add: %s", what); return fail(SGP_ERR_INVALID, msg); }
	sgp_world* w = ms->w;
	if (!body_carries(w, desc->body, SGP_MOTION_KINEMATIC)) return fail(SGP_ERR_INVALID, "sgp_mover_add: the body is not a live kinematic body (no compound, ghost or alias slot)");
	movers_mark_gone(ms);
	if (ms->links.carried(desc->body)) return fail(SGP_ERR_INVALID, "sgp_mover_add: the body already carries a mover of this batch");
	const uint32_t id = ms->slots.take();
	if (id == BatchSlots::none) return fail(SGP_ERR_CAPACITY, "sgp_mover_add: the batch is full");
	MoverRec& r = ms->rec[id];
	const uint32_t reset = r.reset_serial + 1u;
	memset(&r, 0, sizeof(r));
	r.alive = 1u; r.reset_serial = reset; r.kind = desc->kind; r.body = desc->body; r.flags = desc->flags; r.path = 0u; r.leader = SGP_INVALID_ID;
	r.base_rot[3] = 1.0f; r.hold_rot[3] = 1.0f; r.pos_duration = 1.0f; r.rot_duration = 1.0f; r.rot_start[3] = 1.0f; r.rot_target[3] = 1.0f;
	if (desc->kind == SGP_MOVER_PATH) {
		r.path = desc->path; r.leader = desc->leader; memcpy(r.base_rot, desc->base_rot, 16);
		MoverPath& mp = ms->paths[desc->path];
		mp.refs++;
		if (desc->leader == SGP_INVALID_ID) {
			// the constructor (:126-131): walk to the initial time modulo the loop's traversal time
			double t = fmod(desc->initial_time, mp.total_time);      // Maths::doubleMod: the non-negative remainder
			if (t < 0.0) t += mp.total_time;
			sgp_path_progress p = { 0u, 0.0f, 0.0f };
			uint32_t status = 0u;
			mp_advance(&ms->segs[(size_t)desc->path * SGP_MOVER_MAX_WAYPOINTS], mp.n, &p, (float)t, mp.n + 1u, &status);      // (less than one loop: the cap of an update does not apply)
			r.init_index = p.waypoint_index; r.init_dist = p.dist_along_segment; r.init_time = p.time_along_segment;
		} else {
			r.follow_dist = desc->follow_dist; ms->leader_serial[id] = ms->rec[desc->leader].reset_serial; ms->n_followers++;
		}
	} else { memcpy(r.hold_pos, desc->hold_pos, 12); memcpy(r.hold_rot, desc->hold_rot, 16); }
	ms->links.attach(id, desc->body, body_born_of(w, desc->body)); ms->tag[id] = desc->tag; ms->fresh[id] = 1;
	ms->rec.dirty = true;
	*id_out = id;
	return SGP_OK;
}

SGP_API int sgp_mover_remove(sgp_movers* ms, uint32_t id)
{
	if (!batch_usable(ms) || !mover_live(ms, id)) return fail(SGP_ERR_INVALID, "sgp_mover_remove: no such mover");
	MoverRec& r = ms->rec[id];
	ms->links.detach(id);
	if (r.kind == SGP_MOVER_PATH) { ms->paths[r.path].refs--; if (is_follower(r)) ms->n_followers--; }
	r.alive = 0u; ms->rec.dirty = true;
	ms->slots.give_back(id);
	if (ms->n_followers) for (uint32_t k = 0; k < ms->slots.high; ++k) if (ms->rec[k].alive && is_follower(ms->rec[k]) && ms->rec[k].leader == id) ms->rec[k].leader_gone = 1u;
	return SGP_OK;
}

static int set_track(sgp_movers* ms, uint32_t id, const float* start, const float* target, float duration, uint32_t easing, float cur_elapsed, bool rotation, const char* fn)
{
	char msg[160];
	const uint32_t nv = rotation ? 4u : 3u;
	bool ok = batch_usable(ms) && start && target;
	for (uint32_t c = 0; ok && c < nv; ++c) ok = std::isfinite(start[c]) && std::isfinite(target[c]);
	if (!ok || !std::isfinite(duration) || !std::isfinite(cur_elapsed)) { snprintf(msg, sizeof(msg), "%s: NULL, a non-finite value, or the batch's world is gone", fn); return fail(SGP_ERR_INVALID, msg); }
	if (!mover_live(ms, id) || ms->rec[id].kind != SGP_MOVER_MOVETO) { snprintf(msg, sizeof(msg), "%s: no such move-to mover", fn); return fail(SGP_ERR_INVALID, msg); }
	if (easing != SGP_MOVER_EASE_LINEAR && easing != SGP_MOVER_EASE_SMOOTHSTEP) { snprintf(msg, sizeof(msg), "%s: unknown easing", fn); return fail(SGP_ERR_INVALID, msg); }
	MoverRec& r = ms->rec[id];
	// ObjectMoveToController.cpp:36-55
	if (rotation) { memcpy(r.rot_start, start, 16); memcpy(r.rot_target, target, 16); r.rot_duration = std::max(duration, 1.0e-4f); r.rot_easing = easing; r.rot_elapsed = std::max(cur_elapsed, 0.0f); r.rot_serial++; }
	else { memcpy(r.pos_start, start, 12); memcpy(r.pos_target, target, 12); r.pos_duration = std::max(duration, 1.0e-4f); r.pos_easing = easing; r.pos_elapsed = std::max(cur_elapsed, 0.0f); r.pos_serial++; }
	ms->rec.dirty = true;
	return SGP_OK;
}
SGP_API int sgp_movers_set_position_track(sgp_movers* ms, uint32_t id, const float start[3], const float target[3], float duration, uint32_t easing, float cur_elapsed)
{
	return set_track(ms, id, start, target, duration, easing, cur_elapsed, false, "sgp_movers_set_position_track");
}
SGP_API int sgp_movers_set_rotation_track(sgp_movers* ms, uint32_t id, const float start[4], const float target[4], float duration, uint32_t easing, float cur_elapsed)
{
	return set_track(ms, id, start, target, duration, easing, cur_elapsed, true, "sgp_movers_set_rotation_track");
}

SGP_API int sgp_movers_update(sgp_movers* ms, float dt)
{
	{ int r = batch_update_admit(ms, "sgp_movers_update", "movers", std::isfinite(dt) && dt >= 0.0f, "not negative"); if (r != SGP_OK) return r; }
	sgp_world* w = ms->w;
	if (dt == 0.0f) return SGP_OK;      // (the reference would move nothing and leave its target unset)
	{ int r = query_prelude(w); if (r != SGP_OK) return r; }
	if (ms->slots.empty()) return SGP_OK;
	movers_mark_gone(ms);
	{ int r = ms->update_stage(); if (r != SGP_OK) return r; }
	const MoverBufs b = movers_bufs(ms);
	launch_movers_update(w->dv, b, dt, w->stream);
	if (ms->n_followers) launch_movers_follow(w->dv, b, dt, w->stream);
	std::fill(ms->fresh.begin(), ms->fresh.begin() + ms->slots.high, (uint8_t)0);
	return ms->update_end();
}

SGP_API int sgp_movers_checkpoint(sgp_movers* ms, sgp_batch_checkpoint** io) { return batch_checkpoint(ms, SGP_BATCH_MOVERS, "sgp_movers_checkpoint", io); }
SGP_API int sgp_movers_rollback(sgp_movers* ms, const sgp_batch_checkpoint* cp) { return batch_rollback(ms, SGP_BATCH_MOVERS, "sgp_movers_rollback", cp); }

SGP_API int sgp_movers_get_states(sgp_movers* ms, uint32_t first, uint32_t n, sgp_mover_state* out)
{
	const sgp_mover_state* hs;
	const int rc = batch_read_states(ms, "sgp_movers_get_states", &sgp_movers::d_st, first, n, out, &hs, [] { return (int)SGP_OK; });      // (nothing to bring up to date: see `fresh`)
	if (rc != SGP_OK || !hs) return rc;
	for (uint32_t i = 0; i < n; ++i) {
		const uint32_t k = first + i;
		if (mover_live(ms, k) && !ms->fresh[k]) { out[i] = hs[i]; continue; }
		memset(&out[i], 0, sizeof(out[i]));
		if (!mover_live(ms, k)) continue;
		// added and not updated since: what the first update will start from
		const MoverRec& r = ms->rec[k];
		out[i].waypoint_index = r.init_index; out[i].dist_along_segment = r.init_dist; out[i].time_along_segment = r.init_time;
		memcpy(out[i].pos, r.hold_pos, 12); memcpy(out[i].rot, r.kind == SGP_MOVER_PATH ? r.base_rot : r.hold_rot, 16);
		out[i].status = (r.pos_serial ? SGP_MOVER_ST_POS_ACTIVE : 0u) | (r.rot_serial ? SGP_MOVER_ST_ROT_ACTIVE : 0u);
	}
	return SGP_OK;
}
