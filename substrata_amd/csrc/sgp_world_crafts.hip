// sgp_world_crafts.hip -- the batched hover cars and boats (HoverCarPhysics / BoatPhysics for many craft): the host side of sgp_crafts_*.
// The host keeps the descriptions and inputs (uploaded when they change), the slot bookkeeping and which body each craft was added on; the timers, the update
// index and the particle counter live on the device and are touched by the kernels of sgp_k_crafts.hip alone.  An update enqueues and returns.
#include "sgp_world_internal.h"

struct sgp_crafts : WorldBatch {
	BatchSlots slots; BodyLinks links;      // (a body carries one craft)
	Mirror<CraftRec> rec; Mirror<CraftIn> in; std::vector<uint64_t> tag;
	sgp_particles* ps = nullptr;                               // where the particles go (sgp_crafts_attach_particles)
	// device
	CraftDyn* d_dyn = nullptr; sgp_craft_state* d_st = nullptr;
	sgp_particle* d_emit = nullptr; sgp_particle* d_dense = nullptr; uint32_t* d_n_emit = nullptr; uint32_t* d_emit_off = nullptr;
	// what a checkpoint holds beyond the rec and in mirrors (the emit buffers are scratch of one update; `ps` is wiring)
	void ckpt_layout(BatchCkptLayout& l)
	{
		const uint32_t* n = &slots.high;
		l.device(d_dyn, n); l.device(d_st, n);
		l.host_array(tag, n);
		l.table(slots); l.body_links(links, n);
		l.capacity = slots.cap; l.high = slots.high; l.n_alive = slots.n_alive;
	}
};

static CraftBufs crafts_bufs(const sgp_crafts* cs)
{
	CraftBufs b;
	b.rec = cs->rec.d(); b.in = cs->in.d(); b.dyn = cs->d_dyn; b.st = cs->d_st; b.emit = cs->d_emit; b.n_emit = cs->d_n_emit; b.emit_off = cs->d_emit_off; b.dense = cs->d_dense; b.n = cs->slots.high;
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

SGP_API int sgp_crafts_destroy(sgp_crafts* cs) { return batch_destroy(cs, "sgp_crafts_destroy"); }

SGP_API int sgp_crafts_create(sgp_world* w, uint32_t capacity, sgp_crafts** out)
{
	if (!w || !out || capacity == 0 || capacity > SGP_CRAFTS_MAX_CAPACITY) return fail(SGP_ERR_INVALID, "sgp_crafts_create: NULL world or out, or a capacity of 0 or beyond 2^16");
	if (world_holds_ghosts(w)) return fail_ghosts("sgp_crafts_create", "crafts");
	hipSetDevice(w->device);
	sgp_crafts* cs = new sgp_crafts();
	const size_t n = capacity;
	cs->slots.cap = capacity; cs->links.resize(capacity); cs->tag.assign(n, 0ull);
	cs->rec.shape(n, &cs->slots.high); cs->in.shape(n, &cs->slots.high);
	bool ok = cs->adopt(w) && cs->create_mirrors({ &cs->rec, &cs->in });
	ok = ok && cs->alloc(cs->d_dyn, n) && cs->alloc(cs->d_st, n)
	        && cs->alloc(cs->d_emit, n * SGP_CRAFT_MAX_EMIT) && cs->alloc(cs->d_dense, n * SGP_CRAFT_MAX_EMIT) && cs->alloc(cs->d_n_emit, n) && cs->alloc(cs->d_emit_off, n + 1);
	return batch_created(cs, ok, out, "sgp_crafts_create");
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

static bool craft_live(const sgp_crafts* cs, uint32_t id) { return id < cs->slots.high && cs->rec[id].alive; }
// the bodies that have gone since the last look (the host hands out the slots, so it knows): their crafts are marked, and the body is free for another craft
static void crafts_mark_gone(sgp_crafts* cs)
{
	const sgp_world* w = cs->w;
	cs->links.mark_gone(cs->slots.high, [w](uint32_t body) { return body_carries(w, body, SGP_MOTION_DYNAMIC); }, [w](uint32_t body) { return body_born_of(w, body); },
	                    [cs](uint32_t k) { cs->rec[k].gone = 1u; cs->rec.dirty = true; });
}

SGP_API int sgp_craft_add(sgp_crafts* cs, const sgp_craft_desc* desc, uint32_t* id_out)
{
	if (!batch_usable(cs) || !desc || !id_out) return fail(SGP_ERR_INVALID, "sgp_craft_add: NULL, or the batch's world is gone");
	if (const char* what = craft_desc_fault(*desc)) { char msg[160]; snprintf(msg, sizeof(msg), "sgp_craft_add: %s", what); return fail(SGP_ERR_INVALID, msg); }
	sgp_world* w = cs->w;
	if (!body_carries(w, desc->body, SGP_MOTION_DYNAMIC)) return fail(SGP_ERR_INVALID, "sgp_craft_add: the body is not a live dynamic body");
	crafts_mark_gone(cs);
	if (cs->links.carried(desc->body)) return fail(SGP_ERR_INVALID, "sgp_craft_add: the body already carries a craft of this batch");
	const uint32_t id = cs->slots.take();
	if (id == BatchSlots::none) return fail(SGP_ERR_CAPACITY, "sgp_craft_add: the batch is full");
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
	cs->links.attach(id, desc->body, body_born_of(w, desc->body)); cs->tag[id] = desc->tag;
	cs->rec.dirty = cs->in.dirty = true;
	*id_out = id;
	return SGP_OK;
}

SGP_API int sgp_craft_remove(sgp_crafts* cs, uint32_t id)
{
	if (!batch_usable(cs) || !craft_live(cs, id)) return fail(SGP_ERR_INVALID, "sgp_craft_remove: no such craft");
	cs->links.detach(id);
	cs->rec[id].alive = 0u; cs->rec.dirty = true;
	cs->slots.give_back(id);
	return SGP_OK;
}

SGP_API int sgp_crafts_set_inputs(sgp_crafts* cs, uint32_t first, uint32_t n, const sgp_craft_input* inputs)
{
	if (!batch_usable(cs) || (n && !inputs)) return fail(SGP_ERR_INVALID, "sgp_crafts_set_inputs: NULL, or the batch's world is gone");
	if ((uint64_t)first + n > cs->slots.high) return fail(SGP_ERR_INVALID, "sgp_crafts_set_inputs: range beyond the last craft");
	for (uint32_t i = 0; i < n; ++i) {
		if (!std::isfinite(inputs[i].forward) || !std::isfinite(inputs[i].right) || !std::isfinite(inputs[i].up) || !std::isfinite(inputs[i].hand_brake)) return fail(SGP_ERR_INVALID, "sgp_crafts_set_inputs: non-finite value");
		if (inputs[i].flags & ~(SGP_CRAFT_IN_DRIVER | SGP_CRAFT_IN_BOOST)) return fail(SGP_ERR_INVALID, "sgp_crafts_set_inputs: unknown flag");
	}
	for (uint32_t i = 0; i < n; ++i) {
		CraftIn& in = cs->in[first + i];
		CraftRec& r = cs->rec[first + i];
		// userEnteredVehicle stops a boat's righting (BoatPhysics.cpp:80)
		if (r.alive && r.kind == SGP_CRAFT_BOAT && (inputs[i].flags & SGP_CRAFT_IN_DRIVER) && !(in.flags & SGP_CRAFT_IN_DRIVER)) { r.cmd_value = -1.0f; r.cmd_serial++; cs->rec.dirty = true; }
		in.forward = inputs[i].forward; in.right = inputs[i].right; in.up = inputs[i].up; in.hand_brake = inputs[i].hand_brake; in.flags = inputs[i].flags;
	}
	if (n) cs->in.dirty = true;
	return SGP_OK;
}

SGP_API int sgp_crafts_start_righting(sgp_crafts* cs, const uint32_t* ids, uint32_t n)
{
	if (!batch_usable(cs) || (n && !ids)) return fail(SGP_ERR_INVALID, "sgp_crafts_start_righting: NULL, or the batch's world is gone");
	for (uint32_t i = 0; i < n; ++i) if (!craft_live(cs, ids[i])) return fail(SGP_ERR_INVALID, "sgp_crafts_start_righting: no such craft");      // (all or nothing)
	for (uint32_t i = 0; i < n; ++i) {
		CraftRec& r = cs->rec[ids[i]];
		if (r.kind != SGP_CRAFT_BOAT) continue;      // HoverCarPhysics::startRightingVehicle is empty
		r.cmd_value = 2.0f; r.cmd_serial++; cs->rec.dirty = true;
	}
	return SGP_OK;
}

SGP_API int sgp_crafts_attach_particles(sgp_crafts* cs, sgp_particles* ps)
{
	if (!batch_usable(cs)) return fail(SGP_ERR_INVALID, "sgp_crafts_attach_particles: NULL, or the batch's world is gone");
	if (ps) {
		if (!particles_of_world(ps, cs->w)) return fail(SGP_ERR_INVALID, "sgp_crafts_attach_particles: the particle batch belongs to another world, or its world is gone");
		if ((uint64_t)particles_capacity(ps) < (uint64_t)cs->slots.cap * SGP_CRAFT_MAX_EMIT) return fail(SGP_ERR_CAPACITY, "sgp_crafts_attach_particles: the particle batch holds fewer than capacity x SGP_CRAFT_MAX_EMIT particles");
	}
	cs->ps = ps;
	return SGP_OK;
}

SGP_API int sgp_crafts_update(sgp_crafts* cs, float dt)
{
	{ int r = batch_update_admit(cs, "sgp_crafts_update", "crafts", std::isfinite(dt) && dt >= 0.0f, "not negative"); if (r != SGP_OK) return r; }
	sgp_world* w = cs->w;
	{ int r = query_prelude(w); if (r != SGP_OK) return r; }
	if (cs->slots.empty()) return SGP_OK;
	crafts_mark_gone(cs);
	{ int r = cs->update_stage(); if (r != SGP_OK) return r; }
	const CraftBufs b = crafts_bufs(cs);
	launch_crafts_update(w->dv, b, dt, w->h_sp->water_enabled, w->h_sp->water_z, w->stream);
	if (cs->ps) {
		if (!particles_of_world(cs->ps, w)) return fail(SGP_ERR_INVALID, "sgp_crafts_update: the attached particle batch's world is gone");
		launch_crafts_gather(b, w->stream);
		{ int r = particles_append_device(cs->ps, cs->d_dense, cs->d_emit_off + cs->slots.high, cs->slots.high * SGP_CRAFT_MAX_EMIT); if (r != SGP_OK) return r; }
	}
	return cs->update_end();
}

SGP_API int sgp_crafts_checkpoint(sgp_crafts* cs, sgp_batch_checkpoint** io) { return batch_checkpoint(cs, SGP_BATCH_CRAFTS, "sgp_crafts_checkpoint", io); }
SGP_API int sgp_crafts_rollback(sgp_crafts* cs, const sgp_batch_checkpoint* cp) { return batch_rollback(cs, SGP_BATCH_CRAFTS, "sgp_crafts_rollback", cp); }

SGP_API int sgp_crafts_get_states(sgp_crafts* cs, uint32_t first, uint32_t n, sgp_craft_state* out)
{
	const sgp_craft_state* hs;
	const int rc = batch_read_states(cs, "sgp_crafts_get_states", &sgp_crafts::d_st, first, n, out, &hs, [cs] {
		if (!cs->rec.dirty && !cs->in.dirty) return (int)SGP_OK;
		{ int r = cs->upload(); if (r != SGP_OK) return r; }
		launch_crafts_sync(crafts_bufs(cs), cs->w->stream);      // (host edits pending and no update to carry them)
		return (int)SGP_OK;
	});
	if (rc != SGP_OK || !hs) return rc;
	for (uint32_t i = 0; i < n; ++i) {
		if (craft_live(cs, first + i)) { out[i] = hs[i]; continue; }
		memset(&out[i], 0, sizeof(out[i]));
		out[i].trace_body = SGP_INVALID_ID;
	}
	return SGP_OK;
}
