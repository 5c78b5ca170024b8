// sgp_world_crafts.hip -- the batched hover cars and boats (HoverCarPhysics / BoatPhysics for many craft): the host side of sgp_crafts_*.
// The host keeps the descriptions and inputs (uploaded when they change), the slot bookkeeping and which body each craft was added on; the timers, the update
// index and the particle counter live on the device and are touched by the kernels of sgp_k_crafts.hip alone.  An update enqueues and returns.
#include "sgp_world_internal.h"

struct sgp_crafts : WorldBatch {
	uint32_t cap = 0, high = 0, n_alive = 0;
	std::vector<CraftRec> rec; std::vector<CraftIn> in; std::vector<uint32_t> born; std::vector<uint64_t> tag; std::vector<uint32_t> free_list;
	std::unordered_map<uint32_t, uint32_t> craft_of_body;      // body -> the live craft on it (a body carries one craft)
	bool rec_dirty = false, in_dirty = false;
	sgp_particles* ps = nullptr;                               // where the particles go (sgp_crafts_attach_particles)
	// device
	CraftRec* d_rec = nullptr; CraftIn* d_in = nullptr; CraftDyn* d_dyn = nullptr; sgp_craft_state* d_st = nullptr;
	sgp_particle* d_emit = nullptr; sgp_particle* d_dense = nullptr; uint32_t* d_n_emit = nullptr; uint32_t* d_emit_off = nullptr;
	size_t up_rec = 0, up_in = 0;      // the pinned staging of the uploads (WorldBatch::h_up): [records at up_rec][inputs at up_in]
};

static CraftBufs crafts_bufs(const sgp_crafts* cs)
{
	CraftBufs b;
	b.rec = cs->d_rec; b.in = cs->d_in; b.dyn = cs->d_dyn; b.st = cs->d_st; b.emit = cs->d_emit; b.n_emit = cs->d_n_emit; b.emit_off = cs->d_emit_off; b.dense = cs->d_dense; b.n = cs->high;
	return b;
}

SGP_API void sgp_default_craft_desc(uint32_t kind, sgp_craft_desc* d)
{
	if (!d) return;
	memset(d, 0, sizeof(*d));
	d->kind = kind; d->body = SGP_INVALID_ID; d->mass = 1000.0f;
	d->model_to_y_forwards_rot_1[3] = 1.0f; d->model_to_y_forwards_rot_2[3] = 1.0f;
	if (kind == SGP_CRAFT_BOAT) {
		// Scripting.cpp:229-239
		d->thrust_force = 40000.0f; d->propellor_point_os[1] = 0.2f; d->propellor_point_os[2] = -6.2f; d->propellor_sideways_offset = 1.0f;
		d->rudder_deflection_force_factor = 500.0f; d->thrust_vector_lateral_amount = 0.0f; d->jet_particle_initial_width = 1.0f;
		d->front_cross_sectional_area = 2.0f; d->side_cross_sectional_area = 4.0f; d->top_cross_sectional_area = 8.0f;
	}
}

SGP_API int sgp_crafts_destroy(sgp_crafts* cs)
{
	if (!cs) return fail(SGP_ERR_INVALID, "sgp_crafts_destroy: NULL");
	cs->release();
	delete cs;
	return SGP_OK;
}

SGP_API int sgp_crafts_create(sgp_world* w, uint32_t capacity, sgp_crafts** out)
{
	if (!w || !out || capacity == 0 || capacity > SGP_CRAFTS_MAX_CAPACITY) return fail(SGP_ERR_INVALID, "sgp_crafts_create: NULL world or out, or a capacity of 0 or beyond 2^16");
	if (world_holds_ghosts(w)) return fail(SGP_ERR_INVALID, "sgp_crafts_create: the world holds ghost bodies (crafts of tiled worlds are not supported)");
	hipSetDevice(w->device);
	sgp_crafts* cs = new sgp_crafts();
	cs->cap = capacity;
	cs->rec.resize(capacity); cs->in.resize(capacity); cs->born.assign(capacity, 0u); cs->tag.assign(capacity, 0ull);
	memset(cs->rec.data(), 0, sizeof(CraftRec) * capacity); memset(cs->in.data(), 0, sizeof(CraftIn) * capacity);
	const size_t n = capacity;
	StageCarve up;
	cs->up_rec = up.add(sizeof(CraftRec) * n); cs->up_in = up.add(sizeof(CraftIn) * n);
	bool ok = cs->adopt(w);
	ok = ok && cs->alloc(cs->d_rec, n) && cs->alloc(cs->d_in, n) && cs->alloc(cs->d_dyn, n) && cs->alloc(cs->d_st, n)
	        && cs->alloc(cs->d_emit, n * SGP_CRAFT_MAX_EMIT) && cs->alloc(cs->d_dense, n * SGP_CRAFT_MAX_EMIT) && cs->alloc(cs->d_n_emit, n) && cs->alloc(cs->d_emit_off, n + 1);
	ok = ok && cs->pin(up.total);
	if (!ok) { (void)hipGetLastError(); sgp_crafts_destroy(cs); return fail(SGP_ERR_HIP, "sgp_crafts_create: allocation"); }
	*out = cs;
	return SGP_OK;
}

static const char* craft_desc_fault(const sgp_craft_desc& d)
{
	if (d.kind != SGP_CRAFT_HOVERCAR && d.kind != SGP_CRAFT_BOAT) return "an unknown kind";
	if (d.n_splash_points > SGP_CRAFT_MAX_SPLASH_POINTS) return "more than SGP_CRAFT_MAX_SPLASH_POINTS splash points";
	if (!std::isfinite(d.mass) || !finite4(d.model_to_y_forwards_rot_1) || !finite4(d.model_to_y_forwards_rot_2) || !finite3(d.trace_origin_os) || !std::isfinite(d.thrust_force)
	    || !finite3(d.propellor_point_os) || !std::isfinite(d.propellor_sideways_offset) || !std::isfinite(d.rudder_deflection_force_factor) || !std::isfinite(d.thrust_vector_lateral_amount)
	    || !std::isfinite(d.jet_particle_initial_width) || !std::isfinite(d.front_cross_sectional_area) || !std::isfinite(d.side_cross_sectional_area) || !std::isfinite(d.top_cross_sectional_area))
		return "a non-finite value";
	for (uint32_t p = 0; p < d.n_splash_points; ++p) if (!finite4(d.splash_points + 4 * p)) return "a non-finite splash point";
	if (!(d.mass > 0.0f)) return "a non-positive mass";
	return nullptr;
}

static bool craft_live(const sgp_crafts* cs, uint32_t id) { return id < cs->high && cs->rec[id].alive; }
static bool body_carries_craft(const sgp_world* w, uint32_t body)
{
	if (!live(w, body)) return false;
	const HostBody& b = w->hb[body];
	return (b.flags & BF_MOTION_MASK) == SGP_MOTION_DYNAMIC && !(b.flags & BF_ALIAS) && b.comp_root == SGP_INVALID_ID && !b.ghost;
}
static uint32_t born_of(const sgp_world* w, uint32_t body) { return body < w->body_born.size() ? w->body_born[body] : 0u; }
// the bodies that have gone since the last look (the host hands out the slots, so it knows): their crafts are marked, and the body is free for another craft
static void crafts_mark_gone(sgp_crafts* cs)
{
	const sgp_world* w = cs->w;
	for (uint32_t k = 0; k < cs->high; ++k) {
		CraftRec& r = cs->rec[k];
		if (!r.alive || r.gone) continue;
		if (body_carries_craft(w, r.body) && born_of(w, r.body) == cs->born[k]) continue;
		r.gone = 1u; cs->rec_dirty = true;
		const auto it = cs->craft_of_body.find(r.body);
		if (it != cs->craft_of_body.end() && it->second == k) cs->craft_of_body.erase(it);
	}
}

SGP_API int sgp_craft_add(sgp_crafts* cs, const sgp_craft_desc* desc, uint32_t* id_out)
{
	if (!batch_usable(cs) || !desc || !id_out) return fail(SGP_ERR_INVALID, "sgp_craft_add: NULL, or the batch's world is gone");
	if (const char* what = craft_desc_fault(*desc)) { char msg[160]; snprintf(msg, sizeof(msg), "sgp_craft_add: %s", what); return fail(SGP_ERR_INVALID, msg); }
	sgp_world* w = cs->w;
	if (!body_carries_craft(w, desc->body)) return fail(SGP_ERR_INVALID, "sgp_craft_add: the body is not a live dynamic body");
	crafts_mark_gone(cs);
	if (cs->craft_of_body.count(desc->body)) return fail(SGP_ERR_INVALID, "sgp_craft_add: the body already carries a craft of this batch");
	uint32_t id;
	if (!cs->free_list.empty()) { id = cs->free_list.back(); cs->free_list.pop_back(); }
	else if (cs->high < cs->cap) id = cs->high++;
	else return fail(SGP_ERR_CAPACITY, "sgp_craft_add: the batch is full");
	CraftRec& r = cs->rec[id];
	const uint32_t reset = r.reset_serial + 1u, cmd = r.cmd_serial;
	memset(&r, 0, sizeof(r));
	r.alive = 1u; r.reset_serial = reset; r.cmd_serial = cmd; r.cmd_value = -1.0f;
	r.kind = desc->kind; r.body = desc->body; r.seed = desc->seed; r.mass = desc->mass;
	memcpy(r.q1, desc->model_to_y_forwards_rot_1, 16); memcpy(r.q2, desc->model_to_y_forwards_rot_2, 16); memcpy(r.trace_os, desc->trace_origin_os, 12);
	r.thrust = desc->thrust_force; memcpy(r.prop_os, desc->propellor_point_os, 12); r.prop_off = desc->propellor_sideways_offset; r.rudder = desc->rudder_deflection_force_factor;
	r.lateral = desc->thrust_vector_lateral_amount; r.jet_w = desc->jet_particle_initial_width;
	r.a_front = desc->front_cross_sectional_area; r.a_side = desc->side_cross_sectional_area; r.a_top = desc->top_cross_sectional_area;
	r.volume = w->hb[desc->body].volume;
	if (r.volume == 0.0f) r.volume = 1.0f;      // BoatPhysics.cpp:43-45
	r.n_splash = desc->n_splash_points;
	for (uint32_t p = 0; p < r.n_splash; ++p) {
		memcpy(r.splash + 4 * p, desc->splash_points + 4 * p, 12);
		r.splash[4 * p + 3] = std::min(std::max(desc->splash_points[4 * p + 3], -1.0f), 1.0f);      // myClamp, BoatPhysics.cpp:55
	}
	memset(&cs->in[id], 0, sizeof(CraftIn));
	cs->born[id] = born_of(w, desc->body); cs->tag[id] = desc->tag;
	cs->craft_of_body[desc->body] = id;
	cs->rec_dirty = cs->in_dirty = true;
	cs->n_alive++;
	*id_out = id;
	return SGP_OK;
}

SGP_API int sgp_craft_remove(sgp_crafts* cs, uint32_t id)
{
	if (!batch_usable(cs) || !craft_live(cs, id)) return fail(SGP_ERR_INVALID, "sgp_craft_remove: no such craft");
	CraftRec& r = cs->rec[id];
	const auto it = cs->craft_of_body.find(r.body);
	if (it != cs->craft_of_body.end() && it->second == id) cs->craft_of_body.erase(it);
	r.alive = 0u; cs->rec_dirty = true;
	cs->free_list.push_back(id); cs->n_alive--;
	return SGP_OK;
}

SGP_API int sgp_crafts_set_inputs(sgp_crafts* cs, uint32_t first, uint32_t n, const sgp_craft_input* inputs)
{
	if (!batch_usable(cs) || (n && !inputs)) return fail(SGP_ERR_INVALID, "sgp_crafts_set_inputs: NULL, or the batch's world is gone");
	if ((uint64_t)first + n > cs->high) return fail(SGP_ERR_INVALID, "sgp_crafts_set_inputs: range beyond the last craft");
	for (uint32_t i = 0; i < n; ++i) {
		if (!std::isfinite(inputs[i].forward) || !std::isfinite(inputs[i].right) || !std::isfinite(inputs[i].up) || !std::isfinite(inputs[i].hand_brake)) return fail(SGP_ERR_INVALID, "sgp_crafts_set_inputs: non-finite value");
		if (inputs[i].flags & ~(SGP_CRAFT_IN_DRIVER | SGP_CRAFT_IN_BOOST)) return fail(SGP_ERR_INVALID, "sgp_crafts_set_inputs: unknown flag");
	}
	for (uint32_t i = 0; i < n; ++i) {
		CraftIn& in = cs->in[first + i];
		CraftRec& r = cs->rec[first + i];
		// userEnteredVehicle stops a boat's righting (BoatPhysics.cpp:80)
		if (r.alive && r.kind == SGP_CRAFT_BOAT && (inputs[i].flags & SGP_CRAFT_IN_DRIVER) && !(in.flags & SGP_CRAFT_IN_DRIVER)) { r.cmd_value = -1.0f; r.cmd_serial++; cs->rec_dirty = true; }
		in.forward = inputs[i].forward; in.right = inputs[i].right; in.up = inputs[i].up; in.hand_brake = inputs[i].hand_brake; in.flags = inputs[i].flags;
	}
	if (n) cs->in_dirty = true;
	return SGP_OK;
}

SGP_API int sgp_crafts_start_righting(sgp_crafts* cs, const uint32_t* ids, uint32_t n)
{
	if (!batch_usable(cs) || (n && !ids)) return fail(SGP_ERR_INVALID, "sgp_crafts_start_righting: NULL, or the batch's world is gone");
	for (uint32_t i = 0; i < n; ++i) if (!craft_live(cs, ids[i])) return fail(SGP_ERR_INVALID, "sgp_crafts_start_righting: no such craft");      // (all or nothing)
	for (uint32_t i = 0; i < n; ++i) {
		CraftRec& r = cs->rec[ids[i]];
		if (r.kind != SGP_CRAFT_BOAT) continue;      // HoverCarPhysics::startRightingVehicle is empty
		r.cmd_value = 2.0f; r.cmd_serial++; cs->rec_dirty = true;
	}
	return SGP_OK;
}

SGP_API int sgp_crafts_attach_particles(sgp_crafts* cs, sgp_particles* ps)
{
	if (!batch_usable(cs)) return fail(SGP_ERR_INVALID, "sgp_crafts_attach_particles: NULL, or the batch's world is gone");
	if (ps) {
		if (!particles_of_world(ps, cs->w)) return fail(SGP_ERR_INVALID, "sgp_crafts_attach_particles: the particle batch belongs to another world, or its world is gone");
		if ((uint64_t)particles_capacity(ps) < (uint64_t)cs->cap * SGP_CRAFT_MAX_EMIT) return fail(SGP_ERR_CAPACITY, "sgp_crafts_attach_particles: the particle batch holds fewer than capacity x SGP_CRAFT_MAX_EMIT particles");
	}
	cs->ps = ps;
	return SGP_OK;
}

// what changed on the host -> the device, behind whatever the stream holds (no wait for the stream; only for the previous upload to have left the staging buffer)
static int crafts_upload(sgp_crafts* cs)
{
	sgp_world* w = cs->w;
	if (!cs->rec_dirty && !cs->in_dirty) return SGP_OK;
	{ int r = cs->upload_begin(); if (r != SGP_OK) return r; }
	if (cs->rec_dirty && cs->high) {
		memcpy(cs->h_up + cs->up_rec, cs->rec.data(), sizeof(CraftRec) * cs->high);
		HIP_TRY(hipMemcpyAsync(cs->d_rec, cs->h_up + cs->up_rec, sizeof(CraftRec) * cs->high, hipMemcpyHostToDevice, w->stream));
	}
	if (cs->in_dirty && cs->high) {
		memcpy(cs->h_up + cs->up_in, cs->in.data(), sizeof(CraftIn) * cs->high);
		HIP_TRY(hipMemcpyAsync(cs->d_in, cs->h_up + cs->up_in, sizeof(CraftIn) * cs->high, hipMemcpyHostToDevice, w->stream));
	}
	cs->rec_dirty = cs->in_dirty = false;
	return cs->upload_end();
}

SGP_API int sgp_crafts_update(sgp_crafts* cs, float dt)
{
	if (!batch_usable(cs)) return fail(SGP_ERR_INVALID, "sgp_crafts_update: NULL, or the batch's world is gone");
	if (!std::isfinite(dt) || !(dt >= 0.0f)) return fail(SGP_ERR_INVALID, "sgp_crafts_update: dt must be finite and not negative");
	sgp_world* w = cs->w;
	if (world_holds_ghosts(w)) return fail(SGP_ERR_INVALID, "sgp_crafts_update: the world holds ghost bodies (crafts of tiled worlds are not supported)");
	{ int r = query_prelude(w); if (r != SGP_OK) return r; }
	if (!cs->high || !cs->n_alive) return SGP_OK;
	crafts_mark_gone(cs);
	{ int r = crafts_upload(cs); if (r != SGP_OK) return r; }
	{ int r = flush_event_reset(w); if (r != SGP_OK) return r; }      // (a force may wake a body: an activation event)
	const CraftBufs b = crafts_bufs(cs);
	launch_crafts_update(w->dv, b, dt, w->h_sp->water_enabled, w->h_sp->water_z, w->stream);
	if (cs->ps) {
		if (!particles_of_world(cs->ps, w)) return fail(SGP_ERR_INVALID, "sgp_crafts_update: the attached particle batch's world is gone");
		launch_crafts_gather(b, w->stream);
		{ int r = particles_append_device(cs->ps, cs->d_dense, cs->d_emit_off + cs->high, cs->high * SGP_CRAFT_MAX_EMIT); if (r != SGP_OK) return r; }
	}
	// an update leaves forces on bodies, and may have woken them, without the host hearing of it: the next step is not skipped as idle, and the event lists may hold something
	w->dirty_since_step = true; w->events_on_device = true;
	HIP_TRY(hipGetLastError());
	return SGP_OK;
}

SGP_API int sgp_crafts_get_states(sgp_crafts* cs, uint32_t first, uint32_t n, sgp_craft_state* out)
{
	if (!batch_usable(cs) || (n && !out)) return fail(SGP_ERR_INVALID, "sgp_crafts_get_states: NULL, or the batch's world is gone");
	if ((uint64_t)first + n > cs->cap) return fail(SGP_ERR_INVALID, "sgp_crafts_get_states: range beyond the batch's capacity");
	if (!n) return SGP_OK;
	sgp_world* w = cs->w;
	hipSetDevice(w->device);
	ray_server_stop(w);
	if (cs->rec_dirty || cs->in_dirty) {
		{ int r = crafts_upload(cs); if (r != SGP_OK) return r; }
		launch_crafts_sync(crafts_bufs(cs), w->stream);
	}
	{ int r = ensure_stage(w, sizeof(sgp_craft_state) * (size_t)n); if (r != SGP_OK) return r; }
	HIP_TRY(hipMemcpyAsync(w->stage_host, cs->d_st + first, sizeof(sgp_craft_state) * (size_t)n, hipMemcpyDeviceToHost, w->stream));
	HIP_TRY(hipStreamSynchronize(w->stream));
	const sgp_craft_state* hs = (const sgp_craft_state*)w->stage_host;
	for (uint32_t i = 0; i < n; ++i) {
		if (craft_live(cs, first + i)) { out[i] = hs[i]; continue; }
		memset(&out[i], 0, sizeof(out[i]));
		out[i].trace_body = SGP_INVALID_ID;
	}
	return SGP_OK;
}
