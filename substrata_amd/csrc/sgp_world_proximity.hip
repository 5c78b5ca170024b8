// sgp_world_proximity.hip -- the batched proximity and zone watchers (ScriptedObjectProximityChecker and the parcel enter / exit events of GUIClient for many
// observers and objects): the host side of sgp_proximity_*.  The host keeps the objects' records and tags, the observers' sources and the zones (uploaded when
// they change), the slot bookkeeping and which body each object was added on; the near masks, the observers' zones and the pending events live on the device
// and are touched by the kernels of sgp_k_proximity.hip alone.  An update enqueues and returns.  sgp_proximity_test_point / sgp_proximity_pick_zone are
// sgp_proximity_math.h compiled for the host: they need no world and no device.
#include "sgp_world_internal.h"
#include "sgp_proximity_math.h"
#include "sgp_proximity_host.h"
#include <stddef.h>

static const uint32_t k_prox_obs_slots = SGP_PROX_MAX_OBSERVERS;
struct sgp_proximity : WorldBatch {
	BatchSlots slots; BodyLinks links;      // (a body carries one object)
	ProxZoneBook zb;
	Mirror<ProxZone> zones; Mirror<ProxObsRec> obs; Mirror<ProxRec> rec; Mirror<uint64_t> tag;
	std::vector<uint32_t> obs_born;          // [observer]: the birth number of a body-sourced observer's body
	uint32_t live_obs = 0, clear_obs = 0;    // observers that are alive; observers removed since the last launch
	uint32_t ev_cap = 0;
	// not part of a checkpoint: when the links were last walked (a walk is due when the world's bodies changed since, or after a rollback)
	uint32_t seen_births = 0, seen_alive = 0, seen_high = 0; bool walk_due = true, obs_relink = false;
	// device
	uint2* d_st = nullptr; uint4* d_evw = nullptr; uint32_t* d_wg_counts = nullptr; uint32_t* d_wg_off = nullptr;
	ProxObsDyn* d_obs_dyn = nullptr; ProxObsRun* d_run = nullptr; ProxState* d_state = nullptr; sgp_proximity_event* d_events = nullptr;
	// what a checkpoint holds beyond the zones, obs, rec and tag mirrors (the event words, counts, offsets and the observers' run records live for one update)
	void ckpt_layout(BatchCkptLayout& l)
	{
		const uint32_t* n = &slots.high;
		l.device(d_st, n); l.device_whole(d_obs_dyn, k_prox_obs_slots); l.device_whole(d_state, 1u);
		l.counted(d_events, 1, ev_cap, /*word_piece=*/2, (uint32_t)offsetof(ProxState, n_events));      // the pending events: as many as the device's count says (piece 2 is d_state)
		l.host_array(obs_born, &k_prox_obs_slots); l.host_array(zb.gen, &zb.slots.high); l.host_array(zb.key, &zb.slots.high); l.host_array(zb.alive, &zb.slots.high);
		l.scalar(live_obs); l.scalar(clear_obs);
		l.table(slots); l.table(zb.slots); l.body_links(links, n);
		l.capacity = slots.cap; l.high = slots.high; l.n_alive = slots.n_alive;
	}
};

static ProxBufs proximity_bufs(const sgp_proximity* pb)
{
	ProxBufs b;
	b.rec = pb->rec.d(); b.tag = pb->tag.d(); b.st = pb->d_st; b.evw = pb->d_evw; b.wg_counts = pb->d_wg_counts; b.wg_off = pb->d_wg_off;
	b.zones = pb->zones.d(); b.obs = pb->obs.d(); b.obs_dyn = pb->d_obs_dyn; b.run = pb->d_run; b.state = pb->d_state; b.events = pb->d_events;
	b.n = pb->slots.high; b.n_zones = pb->zb.slots.high; b.ev_cap = pb->ev_cap; b.live_obs = pb->live_obs; b.clear_obs = pb->clear_obs;
	return b;
}

bool proximity_of_world(const sgp_proximity* pb, const sgp_world* w) { return batch_usable(pb) && pb->w == w; }
const ProxObsDyn* proximity_obs_dyn(const sgp_proximity* pb) { return pb->d_obs_dyn; }

SGP_API int sgp_proximity_test_point(const float mn[3], const float mx[3], const float p[3], float radius, uint32_t* near_out, float* dist2_out)
{
	if (!mn || !mx || !p || !near_out || !dist2_out) return fail(SGP_ERR_INVALID, "sgp_proximity_test_point: NULL");
	const float d2 = px_dist2(PX3(mn), PX3(mx), PX3(p));
	*dist2_out = d2; *near_out = px_near(d2, radius) ? 1u : 0u;
	return SGP_OK;
}

SGP_API int sgp_proximity_pick_zone(const float* mins, const float* maxs, const uint32_t* keys, const uint32_t* live, uint32_t n, uint32_t current, const float p[3], uint32_t* zone_out)
{
	if (!p || !zone_out || (n && (!mins || !maxs || !keys || !live))) return fail(SGP_ERR_INVALID, "sgp_proximity_pick_zone: NULL");
	*zone_out = px_pick_zone(mins, maxs, keys, live, n, current, PX3(p));
	return SGP_OK;
}

SGP_API int sgp_proximity_destroy(sgp_proximity* pb) { return batch_destroy(pb, "sgp_proximity_destroy"); }

SGP_API int sgp_proximity_create(sgp_world* w, uint32_t object_capacity, uint32_t zone_capacity, uint32_t event_capacity, sgp_proximity** out)
{
	if (!w || !out || object_capacity == 0 || object_capacity > SGP_PROXIMITY_MAX_OBJECTS || zone_capacity == 0 || zone_capacity > SGP_PROXIMITY_MAX_ZONES || event_capacity == 0) return fail(SGP_ERR_INVALID, "sgp_proximity_create: NULL world or out, an object capacity of 0 or beyond 2^20, a zone capacity of 0 or beyond 2^12, or an event capacity of 0");
	if (world_holds_ghosts(w)) return fail_ghosts("sgp_proximity_create", "proximity watchers");
	hipSetDevice(w->device);
	sgp_proximity* pb = new sgp_proximity();
	const size_t n = object_capacity, n_wg = (n + PROX_WG - 1) / PROX_WG;
	pb->slots.cap = object_capacity; pb->links.resize(object_capacity); pb->zb.resize(zone_capacity); pb->ev_cap = event_capacity;
	pb->obs_born.assign(k_prox_obs_slots, 0u);
	pb->zones.shape(zone_capacity, &pb->zb.slots.high); pb->obs.shape(k_prox_obs_slots, &k_prox_obs_slots); pb->rec.shape(n, &pb->slots.high); pb->tag.shape(n, &pb->slots.high);
	bool ok = pb->adopt(w) && pb->create_mirrors({ &pb->zones, &pb->obs, &pb->rec, &pb->tag });
	ok = ok && pb->alloc(pb->d_st, n) && pb->alloc(pb->d_evw, n) && pb->alloc(pb->d_wg_counts, n_wg) && pb->alloc(pb->d_wg_off, n_wg);
	ok = ok && pb->alloc(pb->d_obs_dyn, k_prox_obs_slots) && pb->alloc(pb->d_run, k_prox_obs_slots) && pb->alloc(pb->d_state, 1) && pb->alloc(pb->d_events, event_capacity);
	return batch_created(pb, ok, out, "sgp_proximity_create");
}

// the bodies an object or a body-sourced observer sits on: a live body of any motion type that is no compound child, ghost or alias slot
static bool prox_body_carries(const sgp_world* w, uint32_t body)
{
	if (!live(w, body)) return false;
	const HostBody& b = w->hb[body];
	return !(b.flags & BF_ALIAS) && b.comp_root == SGP_INVALID_ID && !b.ghost;
}
static bool object_live(const sgp_proximity* pb, uint32_t id) { return id < pb->slots.high && (pb->rec[id].flags & PROX_ALIVE); }

// The bodies that have gone since the last look: their objects and observers are marked and skipped from then on.  The walk over the objects is the one of
// the other batches, but a batch of 2^20 objects cannot afford it in every update: it runs when the world has created or lost a body since the last walk
// (births only grows, the live count goes down with every removal) or a rollback has left slots to relink.  A world rollback that brings the live count
// back to what the last walk saw while other bodies went is not noticed here -- the device checks every body's flags itself, so such an object is skipped
// all the same, and the next birth in the world brings the walk.
static void proximity_mark_gone(sgp_proximity* pb)
{
	const sgp_world* w = pb->w;
	if (!pb->walk_due && pb->seen_births == w->births && pb->seen_alive == w->n_alive && pb->seen_high == w->high) return;
	pb->links.mark_gone(pb->slots.high, [w](uint32_t body) { return prox_body_carries(w, body); }, [w](uint32_t body) { return body_born_of(w, body); },
	                    [pb](uint32_t k) { pb->rec[k].flags |= PROX_GONE; pb->rec.dirty = true; });
	for (uint32_t k = 0; k < k_prox_obs_slots; ++k) {
		ProxObsRec& o = pb->obs[k];
		if (!o.alive || o.source != SGP_PROX_OBS_BODY || o.gone) continue;
		const bool there = prox_body_carries(w, o.body);
		if (there && pb->obs_relink) { pb->obs_born[k] = body_born_of(w, o.body); continue; }      // (restored from a checkpoint: the body is back under the number it has now)
		if (there && body_born_of(w, o.body) == pb->obs_born[k]) continue;
		o.gone = 1u; pb->obs.dirty = true;
	}
	pb->walk_due = false; pb->obs_relink = false;
	pb->seen_births = w->births; pb->seen_alive = w->n_alive; pb->seen_high = w->high;
}

SGP_API int sgp_proximity_add(sgp_proximity* pb, const sgp_proximity_object* descs, uint32_t n, uint32_t* ids_out)
{
	if (!batch_usable(pb) || (n && (!descs || !ids_out))) return fail(SGP_ERR_INVALID, "sgp_proximity_add: NULL, or the batch's world is gone");
	for (uint32_t i = 0; i < n; ++i) {
		if (!std::isfinite(descs[i].radius) || !(descs[i].radius > 0.0f)) return fail(SGP_ERR_INVALID, "sgp_proximity_add: a radius that is not finite and > 0");
		if (descs[i].flags & ~(SGP_PROX_WANT_NEAR | SGP_PROX_WANT_ZONE)) return fail(SGP_ERR_INVALID, "sgp_proximity_add: an unknown flag");
	}
	const sgp_world* w = pb->w;
	const int why = prox_add(pb->slots, pb->links, descs, n, [w](uint32_t body) { return prox_body_carries(w, body); }, [w](uint32_t body) { return body_born_of(w, body); },
	                         [pb](uint32_t k) { pb->rec[k].flags |= PROX_GONE; pb->rec.dirty = true; },
	                         [pb](uint32_t id, const sgp_proximity_object& d) {
		                         ProxRec& r = pb->rec[id];
		                         r.body = d.body; r.radius = d.radius; r.flags = d.flags | PROX_ALIVE; r.serial++;
		                         pb->tag[id] = d.tag;
	                         }, ids_out);
	if (why) {
		static const char* const what[] = { "", "a body that is not live (or a compound, ghost or alias slot)", "a body that already carries an object of this batch", "a body named twice", "the objects do not all fit" };
		return fail_in(why == 4 ? SGP_ERR_CAPACITY : SGP_ERR_INVALID, "sgp_proximity_add", what[why]);
	}
	if (n) pb->rec.dirty = pb->tag.dirty = true;
	return SGP_OK;
}

SGP_API int sgp_proximity_remove(sgp_proximity* pb, uint32_t id)
{
	if (!batch_usable(pb) || !object_live(pb, id)) return fail(SGP_ERR_INVALID, "sgp_proximity_remove: no such object");
	pb->links.detach(id);
	pb->rec[id].flags = 0u; pb->rec.dirty = true;
	pb->slots.give_back(id);
	return SGP_OK;
}

SGP_API int sgp_proximity_set_flags(sgp_proximity* pb, uint32_t id, uint32_t flags)
{
	if (!batch_usable(pb) || !object_live(pb, id)) return fail(SGP_ERR_INVALID, "sgp_proximity_set_flags: no such object");
	if (flags & ~(SGP_PROX_WANT_NEAR | SGP_PROX_WANT_ZONE)) return fail(SGP_ERR_INVALID, "sgp_proximity_set_flags: an unknown flag");
	ProxRec& r = pb->rec[id];
	r.flags = (r.flags & (PROX_ALIVE | PROX_GONE)) | flags; pb->rec.dirty = true;
	return SGP_OK;
}

SGP_API int sgp_proximity_set_observer(sgp_proximity* pb, uint32_t k, const sgp_proximity_observer* in)
{
	if (!batch_usable(pb) || !in || k >= k_prox_obs_slots) return fail(SGP_ERR_INVALID, "sgp_proximity_set_observer: NULL, an observer beyond SGP_PROX_MAX_OBSERVERS, or the batch's world is gone");
	if (in->source != SGP_PROX_OBS_POINT && in->source != SGP_PROX_OBS_BODY) return fail(SGP_ERR_INVALID, "sgp_proximity_set_observer: an unknown source");
	if (!finite3(in->pos) || !finite3(in->offset)) return fail(SGP_ERR_INVALID, "sgp_proximity_set_observer: a non-finite value");
	if (in->source == SGP_PROX_OBS_BODY && !prox_body_carries(pb->w, in->body)) return fail(SGP_ERR_INVALID, "sgp_proximity_set_observer: the body is not live (or a compound, ghost or alias slot)");
	ProxObsRec& o = pb->obs[k];
	if (!o.alive) { o.alive = 1u; o.serial++; pb->live_obs |= 1u << k; }      // a new observer: the device forgets what the slot's last one knew
	o.source = in->source; o.body = in->source == SGP_PROX_OBS_BODY ? in->body : 0u; o.gone = 0u;
	memcpy(o.pos, in->pos, 12); memcpy(o.off, in->offset, 12);
	pb->obs_born[k] = in->source == SGP_PROX_OBS_BODY ? body_born_of(pb->w, in->body) : 0u;
	pb->obs.dirty = true;
	return SGP_OK;
}

SGP_API int sgp_proximity_set_points(sgp_proximity* pb, uint32_t first, uint32_t n, const float* xyz)
{
	if (!batch_usable(pb) || (n && !xyz) || (uint64_t)first + n > k_prox_obs_slots) return fail(SGP_ERR_INVALID, "sgp_proximity_set_points: NULL, a range beyond SGP_PROX_MAX_OBSERVERS, or the batch's world is gone");
	for (uint32_t i = 0; i < n; ++i) {
		const ProxObsRec& o = pb->obs[first + i];
		if (!o.alive || o.source != SGP_PROX_OBS_POINT) return fail(SGP_ERR_INVALID, "sgp_proximity_set_points: not a live POINT observer");
		if (!finite3(xyz + 3 * (size_t)i)) return fail(SGP_ERR_INVALID, "sgp_proximity_set_points: a non-finite value");
	}
	for (uint32_t i = 0; i < n; ++i) memcpy(pb->obs[first + i].pos, xyz + 3 * (size_t)i, 12);
	if (n) pb->obs.dirty = true;
	return SGP_OK;
}

SGP_API int sgp_proximity_remove_observer(sgp_proximity* pb, uint32_t k)
{
	if (!batch_usable(pb) || k >= k_prox_obs_slots || !pb->obs[k].alive) return fail(SGP_ERR_INVALID, "sgp_proximity_remove_observer: no such observer");
	pb->obs[k].alive = 0u; pb->obs.dirty = true;
	pb->live_obs &= ~(1u << k); pb->clear_obs |= 1u << k;      // its bit leaves every mask with the next launch (and what get_states reports at once)
	return SGP_OK;
}

SGP_API int sgp_proximity_zone_add(sgp_proximity* pb, const float mn[3], const float mx[3], uint32_t key, uint32_t* zone_id_out)
{
	if (!batch_usable(pb) || !mn || !mx || !zone_id_out) return fail(SGP_ERR_INVALID, "sgp_proximity_zone_add: NULL, or the batch's world is gone");
	if (!finite3(mn) || !finite3(mx) || mn[0] > mx[0] || mn[1] > mx[1] || mn[2] > mx[2]) return fail(SGP_ERR_INVALID, "sgp_proximity_zone_add: bounds that are not finite, or mn > mx");
	const uint32_t z = pb->zb.add(key);
	if (z == ProxZoneBook::duplicate) return fail(SGP_ERR_INVALID, "sgp_proximity_zone_add: a live zone has the key");
	if (z == ProxZoneBook::none) return fail(SGP_ERR_CAPACITY, "sgp_proximity_zone_add: no free zone slot");
	ProxZone& r = pb->zones[z];
	memcpy(r.mn, mn, 12); memcpy(r.mx, mx, 12); r.key = key; r.gen_live = (pb->zb.gen[z] << 1) | 1u;
	pb->zones.dirty = true;
	*zone_id_out = z;
	return SGP_OK;
}

SGP_API int sgp_proximity_zone_remove(sgp_proximity* pb, uint32_t z)
{
	if (!batch_usable(pb) || !pb->zb.remove(z)) return fail(SGP_ERR_INVALID, "sgp_proximity_zone_remove: no such zone");
	pb->zones[z].gen_live &= ~1u; pb->zones.dirty = true;
	return SGP_OK;
}

SGP_API int sgp_proximity_update(sgp_proximity* pb)
{
	{ int r = batch_update_admit(pb, "sgp_proximity_update", "proximity watchers", true, ""); if (r != SGP_OK) return r; }
	sgp_world* w = pb->w;
	hipSetDevice(w->device);
	{ int r = flush_cmds(w); if (r != SGP_OK) return r; }      // pending edits reach the bodies' bounds first
	if (pb->slots.empty() || !pb->live_obs) return SGP_OK;
	proximity_mark_gone(pb);
	{ int r = pb->upload(); if (r != SGP_OK) return r; }
	launch_proximity_update(w->dv, proximity_bufs(pb), w->stream);
	pb->clear_obs = 0u;
	HIP_TRY(hipGetLastError());
	return SGP_OK;
}

SGP_API int sgp_proximity_checkpoint(sgp_proximity* pb, sgp_batch_checkpoint** io) { return batch_checkpoint(pb, SGP_BATCH_PROXIMITY, "sgp_proximity_checkpoint", io); }
SGP_API int sgp_proximity_rollback(sgp_proximity* pb, const sgp_batch_checkpoint* cp)
{
	const int r = batch_rollback(pb, SGP_BATCH_PROXIMITY, "sgp_proximity_rollback", cp);
	if (r != SGP_OK) return r;
	pb->zb.rebuild();
	pb->walk_due = true; pb->obs_relink = true;      // the relink rule: the next walk attaches every slot to the body its id names now, objects and observers alike
	return SGP_OK;
}

SGP_API int sgp_proximity_drain_events(sgp_proximity* pb, sgp_proximity_event* out, uint32_t cap, uint32_t* n_out, uint32_t* n_dropped)
{
	if (!batch_usable(pb) || (cap && !out) || !n_out || !n_dropped) return fail(SGP_ERR_INVALID, "sgp_proximity_drain_events: NULL, or the batch's world is gone");
	*n_out = 0; *n_dropped = 0;
	sgp_world* w = pb->w;
	hipSetDevice(w->device);
	ray_server_stop(w);
	{ int r = ensure_stage(w, sizeof(ProxState)); if (r != SGP_OK) return r; }
	HIP_TRY(hipMemcpyAsync(w->stage_host, pb->d_state, sizeof(ProxState), hipMemcpyDeviceToHost, w->stream));
	HIP_TRY(hipStreamSynchronize(w->stream));
	const uint32_t raised = ((const ProxState*)w->stage_host)->n_events, held = std::min(raised, pb->ev_cap), taken = std::min(held, cap);
	if (!raised) return SGP_OK;
	if (taken) {
		{ int r = ensure_stage(w, sizeof(sgp_proximity_event) * (size_t)taken); if (r != SGP_OK) return r; }
		HIP_TRY(hipMemcpyAsync(w->stage_host, pb->d_events, sizeof(sgp_proximity_event) * (size_t)taken, hipMemcpyDeviceToHost, w->stream));
	}
	HIP_TRY(hipMemsetAsync(&pb->d_state->n_events, 0, sizeof(uint32_t), w->stream));
	if (taken) { HIP_TRY(hipStreamSynchronize(w->stream)); memcpy(out, w->stage_host, sizeof(sgp_proximity_event) * (size_t)taken); }
	*n_out = held; *n_dropped = raised - held;
	return SGP_OK;
}

SGP_API int sgp_proximity_get_states(sgp_proximity* pb, uint32_t first, uint32_t n, sgp_proximity_state* out)
{
	const uint2* hs;
	const int rc = batch_read_states(pb, "sgp_proximity_get_states", &sgp_proximity::d_st, first, n, out, &hs, [] { return (int)SGP_OK; });
	if (rc != SGP_OK || !hs) return rc;
	for (uint32_t i = 0; i < n; ++i) {
		const uint32_t k = first + i;
		out[i].status = 0u; out[i].near_mask = 0u;
		if (!object_live(pb, k)) continue;
		const ProxRec& r = pb->rec[k];
		if (((hs[i].x >> PROX_ST_SERIAL_SHIFT) & 0xFFFFu) == (r.serial & 0xFFFFu)) { out[i].status = hs[i].x & 0xFFu; out[i].near_mask = hs[i].y & ~pb->clear_obs; }      // (else: added and not updated since)
		if (r.flags & PROX_GONE) out[i].status |= SGP_PROX_ST_BODY_GONE;
	}
	return SGP_OK;
}

SGP_API int sgp_proximity_get_observers(sgp_proximity* pb, uint32_t first, uint32_t n, sgp_proximity_observer_state* out)
{
	if (!batch_usable(pb) || (n && !out) || (uint64_t)first + n > k_prox_obs_slots) return fail(SGP_ERR_INVALID, "sgp_proximity_get_observers: NULL, a range beyond SGP_PROX_MAX_OBSERVERS, or the batch's world is gone");
	if (!n) return SGP_OK;
	sgp_world* w = pb->w;
	hipSetDevice(w->device);
	ray_server_stop(w);
	{ int r = ensure_stage(w, sizeof(ProxObsDyn) * (size_t)n); if (r != SGP_OK) return r; }
	HIP_TRY(hipMemcpyAsync(w->stage_host, pb->d_obs_dyn + first, sizeof(ProxObsDyn) * (size_t)n, hipMemcpyDeviceToHost, w->stream));
	HIP_TRY(hipStreamSynchronize(w->stream));
	const ProxObsDyn* hd = (const ProxObsDyn*)w->stage_host;
	for (uint32_t i = 0; i < n; ++i) {
		const ProxObsRec& o = pb->obs[first + i];
		memset(&out[i], 0, sizeof(out[i]));
		out[i].zone_key = SGP_INVALID_ID;
		if (!o.alive) continue;
		if (hd[i].serial == o.serial) { memcpy(out[i].pos, hd[i].pos, 12); out[i].zone_key = hd[i].zone_key; out[i].update_index = hd[i].update_index; out[i].status = hd[i].status; }
		else if (o.source == SGP_PROX_OBS_POINT) memcpy(out[i].pos, o.pos, 12);      // set and not updated since: where the first update will find it
		if (o.gone) out[i].status |= SGP_PROX_OBS_ST_BODY_GONE;
	}
	return SGP_OK;
}
