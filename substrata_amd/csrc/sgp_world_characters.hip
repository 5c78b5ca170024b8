// sgp_world_characters.hip -- the batched character controller (JPH::CharacterVirtual for many avatars): the host side of sgp_characters_*.
// The host keeps the descriptions and inputs (uploaded when they change) and the slot bookkeeping; positions, ground states, active contacts and the bodies
// already reported live on the device and are touched by the kernels of sgp_k_characters.hip alone.  An update enqueues and returns.
#include "sgp_world_internal.h"
#include <limits>

struct sgp_characters : WorldBatch {
	BatchSlots slots;
	// the copy of the world's DV the update kernel reads through a pointer: a mirror of `one` record, brought up to date by every update (dv_valid: it has been the world's once)
	Mirror<DV> dv; bool dv_valid = false; const uint32_t one = 1;
	Mirror<CharRec> rec; Mirror<CharIn> in; Mirror<CharDrive> drive;
	uint32_t n_driven = 0;      // slots whose drive has SGP_DRIVE_ON (sgp_character_remove clears it): 0 picks the update kernel without the drive
	void count_driven() { n_driven = 0; for (uint32_t i = 0; i < slots.high; ++i) if (drive[i].flags & SGP_DRIVE_ON) ++n_driven; }
	// device
	CharState* d_st = nullptr; CharDriveState* d_dst = nullptr; CharContact* d_active = nullptr; uint32_t* d_seen = nullptr;
	CharPush* d_push = nullptr; uint32_t* d_n_push = nullptr; CharAdded* d_added = nullptr; uint32_t* d_n_added = nullptr;
	// what a checkpoint holds beyond the rec, in and drive mirrors (d_n_push whole: the push_any word sits behind its last slot)
	void ckpt_layout(BatchCkptLayout& l)
	{
		const uint32_t* n = &slots.high;
		l.device(d_st, n); l.device(d_dst, n); l.device(d_active, n, SGP_CHAR_MAX_CONTACTS); l.device(d_seen, n, SGP_CHAR_MAX_CONTACTS);
		l.device(d_push, n, SGP_CHAR_MAX_PUSHES); l.device_whole(d_n_push, slots.cap + 1u); l.device(d_added, n, SGP_CHAR_MAX_ADDED); l.device(d_n_added, n);
		l.table(slots);
		l.capacity = slots.cap; l.high = slots.high; l.n_alive = slots.n_alive;
	}
};

static CharBufs chars_bufs(const sgp_characters* cs)
{
	CharBufs b;
	b.rec = cs->rec.d(); b.in = cs->in.d(); b.st = cs->d_st; b.active = cs->d_active; b.seen = cs->d_seen;
	b.push = cs->d_push; b.n_push = cs->d_n_push; b.push_any = cs->d_n_push + cs->slots.cap; b.added = cs->d_added; b.n_added = cs->d_n_added; b.n = cs->slots.high;
	return b;
}

SGP_API void sgp_default_character_desc(sgp_character_desc* d)
{
	if (!d) return;
	memset(d, 0, sizeof(*d));
	// CharacterShape, CharacterVirtualSettings and ExtendedUpdateSettings of shim/Jolt/JoltCharacterLite.h (Jolt's defaults)
	d->radius = 0.3f; d->half_height = 0.65f;
	d->up[1] = 1.0f;
	d->supporting_plane[2] = 1.0f; d->supporting_plane[3] = 1.0e10f;
	d->max_slope_angle = 50.0f * 3.14159265f / 180.0f;
	d->mass = 70.0f; d->max_strength = 100.0f;
	d->predictive_contact_distance = 0.1f; d->character_padding = 0.02f; d->penetration_recovery_speed = 1.0f; d->collision_tolerance = 1.0e-3f;
	d->max_collision_iterations = 5; d->max_constraint_iterations = 15;
	d->min_time_remaining = 1.0e-4f;
	d->stick_to_floor_step_down[1] = -0.5f;
	d->walk_stairs_step_up[1] = 0.4f;
	d->walk_stairs_min_step_forward = 0.02f; d->walk_stairs_step_forward_test = 0.15f; d->walk_stairs_cos_angle_forward_contact = 0.2588f;
}

SGP_API int sgp_characters_destroy(sgp_characters* cs) { return batch_destroy(cs, "sgp_characters_destroy"); }

SGP_API int sgp_characters_create(sgp_world* w, uint32_t capacity, sgp_characters** out)
{
	if (!w || !out || capacity == 0 || capacity > (1u << 20)) return fail(SGP_ERR_INVALID, "sgp_characters_create: NULL world or out, or a capacity of 0 or beyond 2^20");
	if (world_holds_ghosts(w)) return fail_ghosts("sgp_characters_create", "characters");
	hipSetDevice(w->device);
	sgp_characters* cs = new sgp_characters();
	const size_t n = capacity;
	cs->slots.cap = capacity;
	cs->dv.shape(1, &cs->one); cs->dv.state = false; cs->rec.shape(n, &cs->slots.high); cs->in.shape(n, &cs->slots.high); cs->drive.shape(n, &cs->slots.high);
	for (uint32_t i = 0; i < capacity; ++i) cs->in[i].ignore = SGP_INVALID_ID;
	bool ok = cs->adopt(w) && cs->create_mirrors({ &cs->dv, &cs->rec, &cs->in, &cs->drive });
	ok = ok && cs->alloc(cs->d_st, n) && cs->alloc(cs->d_dst, n)
	        && cs->alloc(cs->d_active, n * SGP_CHAR_MAX_CONTACTS) && cs->alloc(cs->d_seen, n * SGP_CHAR_MAX_CONTACTS)
	        && cs->alloc(cs->d_push, n * SGP_CHAR_MAX_PUSHES) && cs->alloc(cs->d_n_push, n + 1) && cs->alloc(cs->d_added, n * SGP_CHAR_MAX_ADDED) && cs->alloc(cs->d_n_added, n);
	return batch_created(cs, ok, out, "sgp_characters_create");
}

static const char* character_desc_fault(const sgp_character_desc& d)
{
	if (!std::isfinite(d.radius) || !std::isfinite(d.half_height) || !finite3(d.shape_offset) || !finite3(d.up) || !finite4(d.supporting_plane) || !std::isfinite(d.max_slope_angle)
	    || !std::isfinite(d.mass) || !std::isfinite(d.max_strength) || !std::isfinite(d.predictive_contact_distance) || !std::isfinite(d.character_padding)
	    || !std::isfinite(d.penetration_recovery_speed) || !std::isfinite(d.collision_tolerance)) return "a non-finite value";
	if (!std::isfinite(d.min_time_remaining) || !finite3(d.stick_to_floor_step_down) || !finite3(d.walk_stairs_step_up) || !finite3(d.walk_stairs_step_down_extra)
	    || !std::isfinite(d.walk_stairs_min_step_forward) || !std::isfinite(d.walk_stairs_step_forward_test) || !std::isfinite(d.walk_stairs_cos_angle_forward_contact)) return "a non-finite value";
	if (!(d.radius > 0.0f) || !(d.half_height >= 0.0f)) return "a non-positive capsule size";
	if (!(d.up[0] * d.up[0] + d.up[1] * d.up[1] + d.up[2] * d.up[2] > 0.0f)) return "a zero up vector";
	if (!(d.mass > 0.0f) || d.max_strength < 0.0f) return "a non-positive mass or a negative strength";
	if (d.predictive_contact_distance < 0.0f || d.character_padding < 0.0f || d.collision_tolerance < 0.0f || d.penetration_recovery_speed < 0.0f) return "a negative distance";
	if (d.max_collision_iterations == 0 || d.max_collision_iterations > 16 || d.max_constraint_iterations == 0 || d.max_constraint_iterations > 64) return "iteration limits outside 1..16 / 1..64";
	if (!(d.min_time_remaining > 0.0f)) return "a non-positive minimum time remaining";      // (bounds the collision iterations' time)
	return nullptr;
}

SGP_API int sgp_character_add(sgp_characters* cs, const sgp_character_desc* desc, const float pos[3], uint32_t* id_out)
{
	if (!batch_usable(cs) || !desc || !pos || !id_out) return fail(SGP_ERR_INVALID, "sgp_character_add: NULL, or the batch's world is gone");
	if (!finite3(pos)) return fail(SGP_ERR_INVALID, "sgp_character_add: non-finite position");
	if (const char* what = character_desc_fault(*desc)) { char msg[160]; snprintf(msg, sizeof(msg), "sgp_character_add: %s", what); return fail(SGP_ERR_INVALID, msg); }
	const uint32_t id = cs->slots.take();
	if (id == BatchSlots::none) return fail(SGP_ERR_CAPACITY, "sgp_character_add: the batch is full");
	CharRec& r = cs->rec[id];
	const uint32_t reset = r.reset_serial + 1u, pose = r.pose_serial + 1u;
	memset(&r, 0, sizeof(r));
	r.alive = 1; r.reset_serial = reset; r.pose_serial = pose;
	memcpy(r.pose, pos, 12);
	r.radius = desc->radius; r.half_height = desc->half_height; memcpy(r.offset, desc->shape_offset, 12); memcpy(r.up, desc->up, 12);
	memcpy(r.sv_n, desc->supporting_plane, 12); r.sv_c = desc->supporting_plane[3];
	r.cos_max_slope = std::cos(desc->max_slope_angle);      // (once, here: as CharacterVirtual's constructor)
	r.mass = desc->mass; r.max_strength = desc->max_strength; r.predictive = desc->predictive_contact_distance; r.padding = desc->character_padding;
	r.recovery = desc->penetration_recovery_speed; r.tolerance = desc->collision_tolerance;
	r.max_coll_it = desc->max_collision_iterations; r.max_cons_it = desc->max_constraint_iterations; r.min_time = desc->min_time_remaining;
	memcpy(r.stick, desc->stick_to_floor_step_down, 12); memcpy(r.stairs_up, desc->walk_stairs_step_up, 12);
	r.min_step_fwd = desc->walk_stairs_min_step_forward; r.step_fwd_test = desc->walk_stairs_step_forward_test; r.cos_fwd = desc->walk_stairs_cos_angle_forward_contact;
	memcpy(r.down_extra, desc->walk_stairs_step_down_extra, 12);
	CharIn& in = cs->in[id];
	const uint32_t in_serial = in.serial + 1u;
	memset(&in, 0, sizeof(in)); in.ignore = SGP_INVALID_ID; in.serial = in_serial;
	// nothing of the slot's previous character is driven on: the default drive with SGP_DRIVE_ON unset, and no jump pending
	CharDrive& dr = cs->drive[id];
	const uint32_t drive_serial = dr.serial + 1u, jump_serial = dr.jump_serial + 1u;
	sgp_character_drive dd; sgp_default_character_drive(&dd);
	if (dr.flags & SGP_DRIVE_ON) cs->n_driven--;
	memset(&dr, 0, sizeof(dr));
	dr.flags = dd.flags; dr.jump_speed = dd.jump_speed; dr.max_air_speed = dd.max_air_speed; dr.eye_height = dd.eye_height;
	dr.serial = drive_serial; dr.jump_serial = jump_serial; dr.jump_time = -1.0;
	cs->rec.dirty = cs->in.dirty = cs->drive.dirty = true;
	*id_out = id;
	return SGP_OK;
}

static bool char_live(const sgp_characters* cs, uint32_t id) { return id < cs->slots.high && cs->rec[id].alive; }

SGP_API int sgp_character_remove(sgp_characters* cs, uint32_t id)
{
	if (!batch_usable(cs) || !char_live(cs, id)) return fail(SGP_ERR_INVALID, "sgp_character_remove: no such character");
	hipSetDevice(cs->w->device);
	HIP_TRY(hipMemsetAsync(cs->d_n_added + id, 0, sizeof(uint32_t), cs->w->stream));      // (its pending contact records go with it: the slot's next character starts with none)
	cs->rec[id].alive = 0; cs->rec.dirty = true;
	if (cs->drive[id].flags & SGP_DRIVE_ON) { cs->drive[id].flags &= ~SGP_DRIVE_ON; cs->n_driven--; cs->drive.dirty = true; }      // (a batch whose last driven character goes is an undriven batch again)
	cs->slots.give_back(id);
	return SGP_OK;
}

SGP_API int sgp_characters_set_pose(sgp_characters* cs, const uint32_t* ids, const float* pos, uint32_t n)
{
	if (!batch_usable(cs) || (n && (!ids || !pos))) return fail(SGP_ERR_INVALID, "sgp_characters_set_pose: NULL");
	for (uint32_t i = 0; i < n; ++i) if (!char_live(cs, ids[i]) || !finite3(pos + 3 * i)) return fail(SGP_ERR_INVALID, "sgp_characters_set_pose: no such character, or a non-finite position");      // (all or nothing)
	for (uint32_t i = 0; i < n; ++i) { CharRec& r = cs->rec[ids[i]]; memcpy(r.pose, pos + 3 * i, 12); r.pose_serial++; }
	if (n) cs->rec.dirty = true;
	return SGP_OK;
}

SGP_API int sgp_characters_set_shape(sgp_characters* cs, uint32_t id, float radius, float half_height, const float offset[3])
{
	if (!batch_usable(cs) || !char_live(cs, id) || !offset) return fail(SGP_ERR_INVALID, "sgp_characters_set_shape: no such character");
	if (!std::isfinite(radius) || !std::isfinite(half_height) || !finite3(offset) || !(radius > 0.0f) || !(half_height >= 0.0f)) return fail(SGP_ERR_INVALID, "sgp_characters_set_shape: a non-finite or non-positive capsule size");
	CharRec& r = cs->rec[id];
	r.radius = radius; r.half_height = half_height; memcpy(r.offset, offset, 12);
	cs->rec.dirty = true;
	return SGP_OK;
}

SGP_API int sgp_characters_set_inputs(sgp_characters* cs, uint32_t first, uint32_t n, const sgp_character_input* inputs)
{
	if (!batch_usable(cs) || (n && !inputs)) return fail(SGP_ERR_INVALID, "sgp_characters_set_inputs: NULL");
	if ((uint64_t)first + n > cs->slots.high) return fail(SGP_ERR_INVALID, "sgp_characters_set_inputs: range beyond the last character");
	for (uint32_t i = 0; i < n; ++i) {
		if (!finite3(inputs[i].velocity)) return fail(SGP_ERR_INVALID, "sgp_characters_set_inputs: non-finite velocity");
		if (inputs[i].flags & ~(SGP_CHAR_EXTENDED | SGP_CHAR_NO_SLIDE | SGP_CHAR_DISABLED)) return fail(SGP_ERR_INVALID, "sgp_characters_set_inputs: unknown flag");
	}
	for (uint32_t i = 0; i < n; ++i) {
		CharIn& in = cs->in[first + i];
		memcpy(in.vel, inputs[i].velocity, 12); in.ignore = inputs[i].ignore_id; in.flags = inputs[i].flags; in.serial++;
	}
	if (n) cs->in.dirty = true;
	return SGP_OK;
}

SGP_API void sgp_default_character_drive(sgp_character_drive* d)
{
	if (!d) return;
	memset(d, 0, sizeof(*d));
	// PlayerPhysics.cpp:29-41: jump_speed, max_air_speed, EYE_HEIGHT; gravity is on once the player has moved
	d->flags = SGP_DRIVE_GRAVITY; d->jump_speed = 4.5f; d->max_air_speed = 8.0f; d->eye_height = 1.67f;
}

static const uint32_t k_drive_flags = SGP_DRIVE_ON | SGP_DRIVE_FLY | SGP_DRIVE_GRAVITY | SGP_DRIVE_FREE_CAMERA | SGP_DRIVE_SMOOTH_STAIRS;

SGP_API int sgp_characters_set_drive(sgp_characters* cs, uint32_t first, uint32_t n, const sgp_character_drive* drives)
{
	if (!batch_usable(cs) || (n && !drives)) return fail(SGP_ERR_INVALID, "sgp_characters_set_drive: NULL, or the batch's world is gone");
	if ((uint64_t)first + n > cs->slots.high) return fail(SGP_ERR_INVALID, "sgp_characters_set_drive: range beyond the last character");
	for (uint32_t i = 0; i < n; ++i) {      // (all or nothing)
		const sgp_character_drive& d = drives[i];
		if (!finite3(d.move_desired_vel) || !std::isfinite(d.move_up) || !std::isfinite(d.jump_speed) || !std::isfinite(d.max_air_speed) || !std::isfinite(d.eye_height))
			return fail(SGP_ERR_INVALID, "sgp_characters_set_drive: a non-finite value");
		if (d.flags & ~k_drive_flags) return fail(SGP_ERR_INVALID, "sgp_characters_set_drive: unknown flag");
		if (d.jump_speed < 0.0f || d.max_air_speed < 0.0f || !(d.eye_height > 0.0f)) return fail(SGP_ERR_INVALID, "sgp_characters_set_drive: a negative jump_speed or max_air_speed, or an eye_height that is not positive");
	}
	for (uint32_t i = 0; i < n; ++i) {
		CharDrive& dr = cs->drive[first + i];
		cs->n_driven += ((drives[i].flags & SGP_DRIVE_ON) ? 1u : 0u) - ((dr.flags & SGP_DRIVE_ON) ? 1u : 0u);
		memcpy(dr.move, drives[i].move_desired_vel, 12); dr.move_up = drives[i].move_up; dr.flags = drives[i].flags;
		dr.jump_speed = drives[i].jump_speed; dr.max_air_speed = drives[i].max_air_speed; dr.eye_height = drives[i].eye_height; dr.serial++;
	}
	if (n) cs->drive.dirty = true;
	return SGP_OK;
}

SGP_API int sgp_characters_jump(sgp_characters* cs, const uint32_t* ids, uint32_t n, double cur_time)
{
	if (!batch_usable(cs) || (n && !ids)) return fail(SGP_ERR_INVALID, "sgp_characters_jump: NULL, or the batch's world is gone");
	if (!std::isfinite(cur_time)) return fail(SGP_ERR_INVALID, "sgp_characters_jump: non-finite time");
	for (uint32_t i = 0; i < n; ++i) if (!char_live(cs, ids[i])) return fail(SGP_ERR_INVALID, "sgp_characters_jump: no such character");      // (all or nothing)
	for (uint32_t i = 0; i < n; ++i) { CharDrive& dr = cs->drive[ids[i]]; dr.jump_time = cur_time; dr.jump_serial++; }
	if (n) cs->drive.dirty = true;
	return SGP_OK;
}

static int characters_update(sgp_characters* cs, const char* fn, float dt, double cur_time)
{
	{ int r = batch_update_admit(cs, fn, "characters", std::isfinite(dt) && dt > 0.0f, "positive"); if (r != SGP_OK) return r; }
	sgp_world* w = cs->w;
	{ int r = cs->slots.empty() ? flush_cmds(w) : query_prelude(w); if (r != SGP_OK) return r; }      // (an empty batch applies the edits and leaves the grid alone)
	if (cs->slots.empty()) return SGP_OK;
	if (!cs->dv_valid || memcmp(&cs->dv[0], &w->dv, sizeof(DV)) != 0) { memcpy(&cs->dv[0], &w->dv, sizeof(DV)); cs->dv.dirty = cs->dv_valid = true; }
	{ int r = cs->update_stage(); if (r != SGP_OK) return r; }
	const CharBufs b = chars_bufs(cs);
	const CharDriveArgs drive = { cs->drive.d(), cs->d_dst, cur_time, w->h_sp->water_enabled, w->h_sp->water_z };
	launch_characters_update(cs->dv.d(), b, dt, cs->n_driven ? &drive : nullptr, w->stream);
	launch_characters_push(w->dv, b, w->stream);
	return cs->update_end();
}

// (no clock: one for which no jump window is open -- infinitely late)
SGP_API int sgp_characters_update(sgp_characters* cs, float dt) { return characters_update(cs, "sgp_characters_update", dt, std::numeric_limits<double>::infinity()); }
SGP_API int sgp_characters_update_at(sgp_characters* cs, float dt, double cur_time)
{
	if (!std::isfinite(cur_time)) return fail(SGP_ERR_INVALID, "sgp_characters_update_at: non-finite time");
	return characters_update(cs, "sgp_characters_update_at", dt, cur_time);
}

SGP_API int sgp_characters_checkpoint(sgp_characters* cs, sgp_batch_checkpoint** io) { return batch_checkpoint(cs, SGP_BATCH_CHARACTERS, "sgp_characters_checkpoint", io); }
SGP_API int sgp_characters_rollback(sgp_characters* cs, const sgp_batch_checkpoint* cp)
{
	const int r = batch_rollback(cs, SGP_BATCH_CHARACTERS, "sgp_characters_rollback", cp);
	if (r == SGP_OK) cs->count_driven();      // (the drive records are the capture's again)
	return r;
}

// host edits pending and no update to carry them: they reach the device's states
static int chars_sync(sgp_characters* cs)
{
	if (!cs->rec.dirty && !cs->in.dirty && !cs->drive.dirty) return (int)SGP_OK;
	{ int r = cs->upload(); if (r != SGP_OK) return r; }
	launch_characters_sync(chars_bufs(cs), cs->drive.d(), cs->d_dst, cs->w->stream);
	return (int)SGP_OK;
}

SGP_API int sgp_characters_get_drive_states(sgp_characters* cs, uint32_t first, uint32_t n, sgp_character_drive_state* out)
{
	const CharDriveState* hs;
	const int rc = batch_read_states(cs, "sgp_characters_get_drive_states", &sgp_characters::d_dst, first, n, out, &hs, [cs] { return chars_sync(cs); });
	if (rc != SGP_OK || !hs) return rc;
	for (uint32_t i = 0; i < n; ++i) {
		sgp_character_drive_state& o = out[i];
		memset(&o, 0, sizeof(o));
		if (!char_live(cs, first + i)) continue;
		const CharDriveState& s = hs[i];
		memcpy(o.cam_pos, s.cam_pos, 12); o.campos_z_delta = s.campos_z_delta; memcpy(o.last_xy_plane_vel_rel_ground, s.last_xy, 12);
		o.fraction_submerged = s.fraction_submerged; o.on_ground = s.on_ground; o.jumped = s.jumped; o.num_jumps = s.num_jumps;
	}
	return SGP_OK;
}

SGP_API int sgp_characters_get_states(sgp_characters* cs, uint32_t first, uint32_t n, sgp_character_state* out)
{
	const CharState* hs;
	const int rc = batch_read_states(cs, "sgp_characters_get_states", &sgp_characters::d_st, first, n, out, &hs, [cs] { return chars_sync(cs); });
	if (rc != SGP_OK || !hs) return rc;
	const sgp_world* w = cs->w;
	for (uint32_t i = 0; i < n; ++i) {
		sgp_character_state& o = out[i];
		memset(&o, 0, sizeof(o));
		o.ground_state = SGP_GROUND_IN_AIR; o.ground_body = SGP_INVALID_ID;
		if (!char_live(cs, first + i)) continue;
		const CharState& s = hs[i];
		memcpy(o.pos, s.pos, 12); memcpy(o.lin_vel, s.vel, 12);
		o.ground_state = s.ground_state;
		memcpy(o.ground_normal, s.gn, 12); memcpy(o.ground_velocity, s.gv, 12); memcpy(o.ground_position, s.gp, 12);
		o.overflow = s.overflow;
		if (s.ground_body != SGP_INVALID_ID && s.ground_body < w->hb.size()) {
			o.ground_userdata = w->hb[s.ground_body].userdata;
			o.ground_body = compound_id_of(w, s.ground_body, &o.ground_sub_shape);
		}
	}
	return SGP_OK;
}

SGP_API int sgp_characters_drain_contacts(sgp_characters* cs, sgp_character_contact* out, uint32_t cap, uint32_t* n_out)
{
	if (!batch_usable(cs) || (cap && !out) || !n_out) return fail(SGP_ERR_INVALID, "sgp_characters_drain_contacts: NULL, or the batch's world is gone");
	*n_out = 0;
	if (!cs->slots.high) return SGP_OK;
	sgp_world* w = cs->w;
	hipSetDevice(w->device);
	ray_server_stop(w);
	const size_t cb = (sizeof(uint32_t) * cs->slots.high + 15) & ~size_t(15);
	{ int r = ensure_stage(w, cb + sizeof(CharAdded) * SGP_CHAR_MAX_ADDED * (size_t)cs->slots.high); if (r != SGP_OK) return r; }
	HIP_TRY(hipMemcpyAsync(w->stage_host, cs->d_n_added, sizeof(uint32_t) * cs->slots.high, hipMemcpyDeviceToHost, w->stream));
	HIP_TRY(hipStreamSynchronize(w->stream));
	const uint32_t* counts = (const uint32_t*)w->stage_host;
	uint32_t last = 0, total = 0;
	for (uint32_t k = 0; k < cs->slots.high; ++k) if (counts[k]) { last = k + 1; total += std::min(counts[k], (uint32_t)SGP_CHAR_MAX_ADDED); }
	if (!total) return SGP_OK;
	HIP_TRY(hipMemcpyAsync((char*)w->stage_host + cb, cs->d_added, sizeof(CharAdded) * SGP_CHAR_MAX_ADDED * (size_t)last, hipMemcpyDeviceToHost, w->stream));
	HIP_TRY(hipMemsetAsync(cs->d_n_added, 0, sizeof(uint32_t) * cs->slots.high, w->stream));
	HIP_TRY(hipStreamSynchronize(w->stream));
	const CharAdded* recs = (const CharAdded*)((char*)w->stage_host + cb);
	uint32_t m = 0;
	for (uint32_t k = 0; k < last; ++k) for (uint32_t r = 0; r < std::min(counts[k], (uint32_t)SGP_CHAR_MAX_ADDED); ++r) {
		const CharAdded& a = recs[(size_t)k * SGP_CHAR_MAX_ADDED + r];
		if (a.body >= w->hb.size()) continue;      // (cannot happen: the device reports slots it found alive)
		if (m < cap) {
			sgp_character_contact& o = out[m];
			memset(&o, 0, sizeof(o));
			o.character = k; o.userdata = w->hb[a.body].userdata; o.body = compound_id_of(w, a.body, &o.sub_shape);
			memcpy(o.point, a.p, 12); memcpy(o.normal, a.n, 12);
		}
		++m;
	}
	*n_out = m;
	return SGP_OK;
}
