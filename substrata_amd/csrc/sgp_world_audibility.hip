// sgp_world_audibility.hip -- the batched audio sources (the range walk and the occlusion and muting walk of GUIClient for many listeners and sources): the
// host side of sgp_audibility_*.  The host keeps the sources' records and tags, the listeners' records and the muting keys (uploaded when they change), the
// slot bookkeeping and which body each BODY source was added on; the masks, the pair table, the listeners' last positions and the pending events live on the
// device and are touched by the kernels of sgp_k_audibility.hip alone.  An update enqueues and returns.  sgp_audibility_pair_ray / sgp_audibility_ramp_step
// are sgp_audibility_math.h compiled for the host: they need no world and no device.
#include "sgp_world_internal.h"
#include "sgp_audibility_math.h"
#include "sgp_audibility_host.h"
#include <stddef.h>

static const uint32_t k_aud_lst_slots = SGP_AUD_MAX_LISTENERS;
struct sgp_audibility : WorldBatch {
	BatchSlots slots; BodyLinks links;      // (a body carries one source)
	AudMutingKeys muting;
	Mirror<AudLstRec> lst; Mirror<AudRec> rec; Mirror<uint64_t> tag; Mirror<uint32_t> keys;
	std::vector<uint32_t> lst_born;          // [listener]: the birth number of a body-sourced listener's body
	uint32_t lcap = 0, n_keys = 0, live_lst = 0, clear_lst = 0;
	uint32_t ev_cap = 0, ray_cap = 0;
	double transition = 1.0;
	sgp_proximity* prox = nullptr;           // configuration, like the muting keys: not part of a checkpoint
	// not part of a checkpoint: when the links were last walked
	uint32_t seen_births = 0, seen_alive = 0, seen_high = 0; bool walk_due = true, lst_relink = false;
	// device
	uint4* d_st = nullptr; float4* d_pos = nullptr; uint2* d_scr = nullptr; uint4* d_evw = nullptr;
	uint32_t* d_wg_rays = nullptr; uint32_t* d_wg_ray_off = nullptr; uint32_t* d_wg_counts = nullptr; uint32_t* d_wg_off = nullptr;
	uint32_t* d_ray_list = nullptr; uint32_t* d_ray_hit = nullptr;
	AudLstDyn* d_lst_dyn = nullptr; AudLstRun* d_run = nullptr; AudPair* d_pairs = nullptr; AudState* d_state = nullptr; sgp_audibility_event* d_events = nullptr;
	// what a checkpoint holds beyond the lst, rec and tag mirrors (the scratch words, counts, offsets, the ray list and the listeners' run records live for one update)
	void ckpt_layout(BatchCkptLayout& l)
	{
		const uint32_t* n = &slots.high;
		l.device(d_st, n); l.device(d_pos, n); l.device_whole(d_state, 1u); l.device(d_pairs, n, lcap); l.device_whole(d_lst_dyn, k_aud_lst_slots);
		l.counted(d_events, 1, ev_cap, /*word_piece=*/2, (uint32_t)offsetof(AudState, n_events));      // the pending events: as many as the device's count says (piece 2 is d_state)
		l.host_array(lst_born, &k_aud_lst_slots);
		l.scalar(live_lst); l.scalar(clear_lst);
		l.table(slots); l.body_links(links, n);
		l.capacity = slots.cap; l.high = slots.high; l.n_alive = slots.n_alive;
	}
};

static AudBufs audibility_bufs(const sgp_audibility* ab, double cur_time)
{
	AudBufs b;
	b.rec = ab->rec.d(); b.tag = ab->tag.d(); b.st = ab->d_st; b.pos = ab->d_pos; b.scr = ab->d_scr; b.evw = ab->d_evw;
	b.wg_rays = ab->d_wg_rays; b.wg_ray_off = ab->d_wg_ray_off; b.wg_counts = ab->d_wg_counts; b.wg_off = ab->d_wg_off;
	b.ray_list = ab->d_ray_list; b.ray_hit = ab->d_ray_hit;
	b.lst = ab->lst.d(); b.lst_dyn = ab->d_lst_dyn; b.run = ab->d_run; b.pairs = ab->d_pairs; b.state = ab->d_state; b.events = ab->d_events;
	b.prox_dyn = ab->prox ? proximity_obs_dyn(ab->prox) : nullptr;
	b.mute_keys = ab->keys.d(); b.n_mute_keys = ab->n_keys;
	b.n = ab->slots.high; b.lcap = ab->lcap; b.ev_cap = ab->ev_cap; b.ray_cap = ab->ray_cap;
	b.live_lst = ab->live_lst; b.clear_lst = ab->clear_lst;
	b.cur_time = cur_time; b.transition = ab->transition;
	return b;
}

SGP_API int sgp_audibility_pair_ray(const float sp[3], const float lp[3], float volume, uint32_t in_range_before, uint32_t* in_range_out, uint32_t* traced_out, float* dist_out, float dir_out[3], float* trace_out)
{
	if (!sp || !lp || !in_range_out || !traced_out || !dist_out || !dir_out || !trace_out) return fail(SGP_ERR_INVALID, "sgp_audibility_pair_ray: NULL");
	const AxGeom g = ax_geom(sp[0], sp[1], sp[2], lp[0], lp[1], lp[2], volume);
	const bool now = ax_range(in_range_before != 0u, g);
	float dist;
	const bool traced = ax_traced(now, g, &dist);
	*in_range_out = now ? 1u : 0u; *traced_out = traced ? 1u : 0u;
	*dist_out = 0.0f; dir_out[0] = dir_out[1] = dir_out[2] = 0.0f; *trace_out = 0.0f;
	if (traced) { *dist_out = dist; ax_ray(g, dist, dir_out, trace_out); }
	return SGP_OK;
}

SGP_API int sgp_audibility_ramp_step(sgp_audibility_ramp* io, uint32_t mute, double cur_time, double transition, uint32_t* changed_out)
{
	if (!io || !changed_out) return fail(SGP_ERR_INVALID, "sgp_audibility_ramp_step: NULL");
	AxRamp r;
	r.start = io->mute_change_start_time; r.end = io->mute_change_end_time; r.factor = io->mute_volume_factor; r.fac_start = io->mute_vol_fac_start; r.fac_end = io->mute_vol_fac_end;
	*changed_out = ax_ramp_step(r, mute != 0u, cur_time, transition) ? 1u : 0u;
	io->mute_change_start_time = r.start; io->mute_change_end_time = r.end; io->mute_volume_factor = r.factor; io->mute_vol_fac_start = r.fac_start; io->mute_vol_fac_end = r.fac_end;
	return SGP_OK;
}

SGP_API int sgp_audibility_destroy(sgp_audibility* ab) { return batch_destroy(ab, "sgp_audibility_destroy"); }

SGP_API int sgp_audibility_create(sgp_world* w, uint32_t source_capacity, uint32_t listener_capacity, uint32_t event_capacity, sgp_audibility** out)
{
	if (!w || !out || !aud_capacities_ok(source_capacity, listener_capacity, event_capacity)) return fail(SGP_ERR_INVALID, "sgp_audibility_create: NULL world or out, a source capacity of 0 or beyond 2^20, a listener capacity of 0 or beyond 32, more than 2^22 pairs, or an event capacity of 0");
	if (world_holds_ghosts(w)) return fail_ghosts("sgp_audibility_create", "audio sources");
	hipSetDevice(w->device);
	sgp_audibility* ab = new sgp_audibility();
	const size_t n = source_capacity, n_wg = (n + AUD_WG - 1) / AUD_WG, n_pairs = n * listener_capacity;
	static const uint32_t k_max_keys = SGP_PROXIMITY_MAX_ZONES;
	ab->slots.cap = source_capacity; ab->links.resize(source_capacity); ab->lcap = listener_capacity; ab->ev_cap = event_capacity; ab->ray_cap = (uint32_t)n_pairs;
	ab->lst_born.assign(k_aud_lst_slots, 0u);
	ab->lst.shape(k_aud_lst_slots, &k_aud_lst_slots); ab->rec.shape(n, &ab->slots.high); ab->tag.shape(n, &ab->slots.high); ab->keys.shape(k_max_keys, &ab->n_keys);
	ab->keys.state = false;
	bool ok = ab->adopt(w) && ab->create_mirrors({ &ab->lst, &ab->rec, &ab->tag, &ab->keys });
	ok = ok && ab->alloc(ab->d_st, n) && ab->alloc(ab->d_pos, n) && ab->alloc(ab->d_scr, n) && ab->alloc(ab->d_evw, n);
	ok = ok && ab->alloc(ab->d_wg_rays, n_wg) && ab->alloc(ab->d_wg_ray_off, n_wg) && ab->alloc(ab->d_wg_counts, n_wg) && ab->alloc(ab->d_wg_off, n_wg);
	ok = ok && ab->alloc(ab->d_ray_list, n_pairs) && ab->alloc(ab->d_ray_hit, n_pairs) && ab->alloc(ab->d_pairs, n_pairs);
	ok = ok && ab->alloc(ab->d_lst_dyn, k_aud_lst_slots) && ab->alloc(ab->d_run, k_aud_lst_slots) && ab->alloc(ab->d_state, 1) && ab->alloc(ab->d_events, event_capacity);
	return batch_created(ab, ok, out, "sgp_audibility_create");
}

// the bodies a source or a body-sourced listener sits on: a live body of any motion type that is no compound child, ghost or alias slot
static bool aud_body_carries(const sgp_world* w, uint32_t body)
{
	if (!live(w, body)) return false;
	const HostBody& b = w->hb[body];
	return !(b.flags & BF_ALIAS) && b.comp_root == SGP_INVALID_ID && !b.ghost;
}
static bool source_live(const sgp_audibility* ab, uint32_t id) { return id < ab->slots.high && (ab->rec[id].flags & AUD_ALIVE); }
static const uint32_t k_aud_user_flags = SGP_AUD_ONE_SHOT | SGP_AUD_WANT_RANGE | SGP_AUD_WANT_OCCLUSION | SGP_AUD_WANT_VOLUME;

// The bodies that have gone since the last look: their sources and listeners are marked and frozen from then on (the walk and its rule: sgp_world_proximity.hip)
static void audibility_mark_gone(sgp_audibility* ab)
{
	const sgp_world* w = ab->w;
	if (!ab->walk_due && ab->seen_births == w->births && ab->seen_alive == w->n_alive && ab->seen_high == w->high) return;
	ab->links.mark_gone(ab->slots.high, [w](uint32_t body) { return aud_body_carries(w, body); }, [w](uint32_t body) { return body_born_of(w, body); },
	                    [ab](uint32_t k) { ab->rec[k].flags |= AUD_GONE; ab->rec.dirty = true; });
	for (uint32_t k = 0; k < k_aud_lst_slots; ++k) {
		AudLstRec& o = ab->lst[k];
		if (!o.alive || o.source != SGP_AUD_LST_BODY || o.gone) continue;
		const bool there = aud_body_carries(w, o.body);
		if (there && ab->lst_relink) { ab->lst_born[k] = body_born_of(w, o.body); continue; }      // (restored from a checkpoint: the body is back under the number it has now)
		if (there && body_born_of(w, o.body) == ab->lst_born[k]) continue;
		o.gone = 1u; ab->lst.dirty = true;
	}
	ab->walk_due = false; ab->lst_relink = false;
	ab->seen_births = w->births; ab->seen_alive = w->n_alive; ab->seen_high = w->high;
}

SGP_API int sgp_audibility_add(sgp_audibility* ab, const sgp_audibility_source* descs, uint32_t n, uint32_t* ids_out)
{
	if (!batch_usable(ab) || (n && (!descs || !ids_out))) return fail(SGP_ERR_INVALID, "sgp_audibility_add: NULL, or the batch's world is gone");
	for (uint32_t i = 0; i < n; ++i) {
		if (descs[i].kind != SGP_AUD_SRC_POINT && descs[i].kind != SGP_AUD_SRC_BODY) return fail(SGP_ERR_INVALID, "sgp_audibility_add: an unknown kind");
		if (!std::isfinite(descs[i].volume) || descs[i].volume < 0.0f || !finite3(descs[i].pos)) return fail(SGP_ERR_INVALID, "sgp_audibility_add: a volume that is not finite and >= 0, or a non-finite position");
		if (descs[i].flags & ~k_aud_user_flags) return fail(SGP_ERR_INVALID, "sgp_audibility_add: an unknown flag");
	}
	const sgp_world* w = ab->w;
	const int why = aud_add(ab->slots, ab->links, descs, n, [w](uint32_t body) { return aud_body_carries(w, body); }, [w](uint32_t body) { return body_born_of(w, body); },
	                        [ab](uint32_t k) { ab->rec[k].flags |= AUD_GONE; ab->rec.dirty = true; },
	                        [ab](uint32_t id, const sgp_audibility_source& d) {
		                        AudRec& r = ab->rec[id];
		                        const bool body = d.kind == SGP_AUD_SRC_BODY;
		                        r.body = body ? d.body : 0u; memcpy(r.pos, d.pos, 12); r.volume = d.volume; r.zone_key = d.zone_key;
		                        r.flags = d.flags | AUD_ALIVE | (body ? AUD_BODY : 0u); r.serial++;
		                        ab->tag[id] = d.tag;
	                        }, ids_out);
	if (why) {
		static const char* const what[] = { "", "a body that is not live (or a compound, ghost or alias slot)", "a body that already carries a source of this batch", "a body named twice", "the sources do not all fit" };
		return fail_in(why == 4 ? SGP_ERR_CAPACITY : SGP_ERR_INVALID, "sgp_audibility_add", what[why]);
	}
	if (n) ab->rec.dirty = ab->tag.dirty = true;
	return SGP_OK;
}

SGP_API int sgp_audibility_remove(sgp_audibility* ab, uint32_t id)
{
	if (!batch_usable(ab) || !source_live(ab, id)) return fail(SGP_ERR_INVALID, "sgp_audibility_remove: no such source");
	if (ab->rec[id].flags & AUD_BODY) ab->links.detach(id);
	ab->rec[id].flags = 0u; ab->rec.dirty = true;
	ab->slots.give_back(id);
	return SGP_OK;
}

SGP_API int sgp_audibility_set_points(sgp_audibility* ab, uint32_t first, uint32_t n, const float* xyz)
{
	if (!batch_usable(ab) || (n && !xyz) || (uint64_t)first + n > ab->slots.high) return fail(SGP_ERR_INVALID, "sgp_audibility_set_points: NULL, a range beyond the sources, or the batch's world is gone");
	for (uint32_t i = 0; i < n; ++i) {
		if (!source_live(ab, first + i) || (ab->rec[first + i].flags & AUD_BODY)) return fail(SGP_ERR_INVALID, "sgp_audibility_set_points: not a live POINT source");
		if (!finite3(xyz + 3 * (size_t)i)) return fail(SGP_ERR_INVALID, "sgp_audibility_set_points: a non-finite value");
	}
	for (uint32_t i = 0; i < n; ++i) memcpy(ab->rec[first + i].pos, xyz + 3 * (size_t)i, 12);
	if (n) ab->rec.dirty = true;
	return SGP_OK;
}

SGP_API int sgp_audibility_set_volume(sgp_audibility* ab, uint32_t id, float volume)
{
	if (!batch_usable(ab) || !source_live(ab, id)) return fail(SGP_ERR_INVALID, "sgp_audibility_set_volume: no such source");
	if (!std::isfinite(volume) || volume < 0.0f) return fail(SGP_ERR_INVALID, "sgp_audibility_set_volume: a volume that is not finite and >= 0");
	ab->rec[id].volume = volume; ab->rec.dirty = true;
	return SGP_OK;
}

SGP_API int sgp_audibility_set_flags(sgp_audibility* ab, uint32_t id, uint32_t flags)
{
	if (!batch_usable(ab) || !source_live(ab, id)) return fail(SGP_ERR_INVALID, "sgp_audibility_set_flags: no such source");
	if (flags & ~k_aud_user_flags) return fail(SGP_ERR_INVALID, "sgp_audibility_set_flags: an unknown flag");
	AudRec& r = ab->rec[id];
	r.flags = (r.flags & (AUD_ALIVE | AUD_GONE | AUD_BODY)) | flags; ab->rec.dirty = true;
	return SGP_OK;
}

SGP_API int sgp_audibility_set_listener(sgp_audibility* ab, uint32_t k, const sgp_audibility_listener* in)
{
	if (!batch_usable(ab) || !in || k >= ab->lcap) return fail(SGP_ERR_INVALID, "sgp_audibility_set_listener: NULL, a listener beyond the batch's listener capacity, or the batch's world is gone");
	if (in->source != SGP_AUD_LST_POINT && in->source != SGP_AUD_LST_BODY) return fail(SGP_ERR_INVALID, "sgp_audibility_set_listener: an unknown source");
	if (!finite3(in->pos) || !finite3(in->offset)) return fail(SGP_ERR_INVALID, "sgp_audibility_set_listener: a non-finite value");
	if (in->source == SGP_AUD_LST_BODY && !aud_body_carries(ab->w, in->body)) return fail(SGP_ERR_INVALID, "sgp_audibility_set_listener: the body is not live (or a compound, ghost or alias slot)");
	AudLstRec& o = ab->lst[k];
	if (!o.alive) { o.alive = 1u; o.serial++; ab->live_lst |= 1u << k; }      // a new listener: its pairs start as the constructor leaves them (the slot's bits were cleared when its last one left)
	o.source = in->source; o.body = in->source == SGP_AUD_LST_BODY ? in->body : 0u; o.gone = 0u;
	memcpy(o.pos, in->pos, 12); memcpy(o.off, in->offset, 12);
	o.ignore_body = in->ignore_body; o.zone_key = in->zone_key; o.mute_outside = in->mute_outside ? 1u : 0u;
	ab->lst_born[k] = in->source == SGP_AUD_LST_BODY ? body_born_of(ab->w, in->body) : 0u;
	ab->lst.dirty = true;
	return SGP_OK;
}

SGP_API int sgp_audibility_remove_listener(sgp_audibility* ab, uint32_t k)
{
	if (!batch_usable(ab) || k >= ab->lcap || !ab->lst[k].alive) return fail(SGP_ERR_INVALID, "sgp_audibility_remove_listener: no such listener");
	ab->lst[k].alive = 0u; ab->lst.dirty = true;
	ab->live_lst &= ~(1u << k); ab->clear_lst |= 1u << k;      // its bit leaves every mask with the next launch (and what the getters report at once)
	return SGP_OK;
}

SGP_API int sgp_audibility_set_listener_points(sgp_audibility* ab, uint32_t first, uint32_t n, const float* xyz)
{
	if (!batch_usable(ab) || (n && !xyz) || (uint64_t)first + n > ab->lcap) return fail(SGP_ERR_INVALID, "sgp_audibility_set_listener_points: NULL, a range beyond the batch's listener capacity, or the batch's world is gone");
	for (uint32_t i = 0; i < n; ++i) {
		const AudLstRec& o = ab->lst[first + i];
		if (!o.alive || o.source != SGP_AUD_LST_POINT) return fail(SGP_ERR_INVALID, "sgp_audibility_set_listener_points: not a live POINT listener");
		if (!finite3(xyz + 3 * (size_t)i)) return fail(SGP_ERR_INVALID, "sgp_audibility_set_listener_points: a non-finite value");
	}
	for (uint32_t i = 0; i < n; ++i) memcpy(ab->lst[first + i].pos, xyz + 3 * (size_t)i, 12);
	if (n) ab->lst.dirty = true;
	return SGP_OK;
}

SGP_API int sgp_audibility_set_listener_zone(sgp_audibility* ab, uint32_t k, uint32_t zone_key, uint32_t mute_outside)
{
	if (!batch_usable(ab) || k >= ab->lcap || !ab->lst[k].alive) return fail(SGP_ERR_INVALID, "sgp_audibility_set_listener_zone: no such listener");
	ab->lst[k].zone_key = zone_key; ab->lst[k].mute_outside = mute_outside ? 1u : 0u; ab->lst.dirty = true;
	return SGP_OK;
}

SGP_API int sgp_audibility_set_transition(sgp_audibility* ab, double seconds)
{
	if (!batch_usable(ab) || !std::isfinite(seconds) || seconds < 0.0) return fail(SGP_ERR_INVALID, "sgp_audibility_set_transition: NULL, the batch's world is gone, or a period that is not finite and >= 0");
	ab->transition = seconds;
	return SGP_OK;
}

SGP_API int sgp_audibility_attach_proximity(sgp_audibility* ab, sgp_proximity* pb)
{
	if (!batch_usable(ab)) return fail(SGP_ERR_INVALID, "sgp_audibility_attach_proximity: NULL, or the batch's world is gone");
	if (pb && !proximity_of_world(pb, ab->w)) return fail(SGP_ERR_INVALID, "sgp_audibility_attach_proximity: the proximity batch is not one of this world");
	ab->prox = pb;
	return SGP_OK;
}

SGP_API int sgp_audibility_set_muting_keys(sgp_audibility* ab, const uint32_t* keys, uint32_t n)
{
	if (!batch_usable(ab) || (n && !keys)) return fail(SGP_ERR_INVALID, "sgp_audibility_set_muting_keys: NULL, or the batch's world is gone");
	if (!ab->muting.set(keys, n)) return fail(SGP_ERR_INVALID, "sgp_audibility_set_muting_keys: more than SGP_PROXIMITY_MAX_ZONES keys, a key of SGP_INVALID_ID, or keys that are not strictly ascending");
	// (a host write: the next update uploads the list, and its launches carry the count)
	for (uint32_t i = 0; i < n; ++i) ab->keys[i] = keys[i];
	ab->n_keys = n; ab->keys.dirty = true;
	return SGP_OK;
}

SGP_API int sgp_audibility_update(sgp_audibility* ab, double cur_time)
{
	{ int r = batch_update_admit(ab, "sgp_audibility_update", "audio sources", true, ""); if (r != SGP_OK) return r; }
	if (!std::isfinite(cur_time)) return fail(SGP_ERR_INVALID, "sgp_audibility_update: cur_time must be finite");
	sgp_world* w = ab->w;
	{ int r = query_prelude(w); if (r != SGP_OK) return r; }      // pending edits reach the bodies first, the resident ray server leaves, the rays' grid is valid
	if (ab->slots.empty() || !ab->live_lst) return SGP_OK;
	audibility_mark_gone(ab);
	{ int r = ab->upload(); if (r != SGP_OK) return r; }
	launch_audibility_update(w->dv, audibility_bufs(ab, cur_time), w->stream);
	ab->clear_lst = 0u;
	HIP_TRY(hipGetLastError());
	return SGP_OK;
}

SGP_API int sgp_audibility_checkpoint(sgp_audibility* ab, sgp_batch_checkpoint** io) { return batch_checkpoint(ab, SGP_BATCH_AUDIBILITY, "sgp_audibility_checkpoint", io); }
SGP_API int sgp_audibility_rollback(sgp_audibility* ab, const sgp_batch_checkpoint* cp)
{
	const int r = batch_rollback(ab, SGP_BATCH_AUDIBILITY, "sgp_audibility_rollback", cp);
	if (r != SGP_OK) return r;
	ab->walk_due = true; ab->lst_relink = true;      // the relink rule: the next walk attaches every slot to the body its id names now, sources and listeners alike
	return SGP_OK;
}

SGP_API int sgp_audibility_drain_events(sgp_audibility* ab, sgp_audibility_event* out, uint32_t cap, uint32_t* n_out, uint32_t* n_dropped)
{
	if (!batch_usable(ab) || (cap && !out) || !n_out || !n_dropped) return fail(SGP_ERR_INVALID, "sgp_audibility_drain_events: NULL, or the batch's world is gone");
	*n_out = 0; *n_dropped = 0;
	sgp_world* w = ab->w;
	hipSetDevice(w->device);
	ray_server_stop(w);
	{ int r = ensure_stage(w, sizeof(AudState)); if (r != SGP_OK) return r; }
	HIP_TRY(hipMemcpyAsync(w->stage_host, ab->d_state, sizeof(AudState), hipMemcpyDeviceToHost, w->stream));
	HIP_TRY(hipStreamSynchronize(w->stream));
	const uint32_t raised = ((const AudState*)w->stage_host)->n_events, held = std::min(raised, ab->ev_cap), taken = std::min(held, cap);
	if (!raised) return SGP_OK;
	if (taken) {
		{ int r = ensure_stage(w, sizeof(sgp_audibility_event) * (size_t)taken); if (r != SGP_OK) return r; }
		HIP_TRY(hipMemcpyAsync(w->stage_host, ab->d_events, sizeof(sgp_audibility_event) * (size_t)taken, hipMemcpyDeviceToHost, w->stream));
	}
	HIP_TRY(hipMemsetAsync(&ab->d_state->n_events, 0, sizeof(uint32_t), w->stream));
	if (taken) { HIP_TRY(hipStreamSynchronize(w->stream)); memcpy(out, w->stage_host, sizeof(sgp_audibility_event) * (size_t)taken); }
	*n_out = held; *n_dropped = raised - held;
	return SGP_OK;
}

// the state words of a source as the getters see them: live, and written by an update since the source was added
static bool source_state_valid(const sgp_audibility* ab, uint32_t k, const uint4& st) { return ((st.x >> AUD_ST_SERIAL_SHIFT) & 0xFFFFu) == (ab->rec[k].serial & 0xFFFFu); }

SGP_API int sgp_audibility_get_states(sgp_audibility* ab, uint32_t first, uint32_t n, sgp_audibility_state* out)
{
	if (!batch_usable(ab) || (n && !out)) return fail(SGP_ERR_INVALID, "sgp_audibility_get_states: NULL, or the batch's world is gone");
	if ((uint64_t)first + n > ab->slots.cap) return fail(SGP_ERR_INVALID, "sgp_audibility_get_states: range beyond the batch's capacity");
	if (!n) return SGP_OK;
	sgp_world* w = ab->w;
	hipSetDevice(w->device);
	ray_server_stop(w);
	StageCarve c;
	const size_t st_off = c.add(sizeof(uint4) * (size_t)n), pos_off = c.add(sizeof(float4) * (size_t)n);
	{ int r = ensure_stage(w, c.total); if (r != SGP_OK) return r; }
	HIP_TRY(hipMemcpyAsync(stage_h<uint4>(w, st_off), ab->d_st + first, sizeof(uint4) * (size_t)n, hipMemcpyDeviceToHost, w->stream));
	HIP_TRY(hipMemcpyAsync(stage_h<float4>(w, pos_off), ab->d_pos + first, sizeof(float4) * (size_t)n, hipMemcpyDeviceToHost, w->stream));
	HIP_TRY(hipStreamSynchronize(w->stream));
	const uint4* hs = stage_h<uint4>(w, st_off); const float4* hp = stage_h<float4>(w, pos_off);
	for (uint32_t i = 0; i < n; ++i) {
		const uint32_t k = first + i;
		memset(&out[i], 0, sizeof(out[i]));
		if (!source_live(ab, k)) continue;
		const AudRec& r = ab->rec[k];
		if (source_state_valid(ab, k, hs[i])) {
			out[i].status = hs[i].x & 0xFFu; out[i].in_range_mask = hs[i].y & ~ab->clear_lst; out[i].occluded_mask = hs[i].z & ~ab->clear_lst;
			out[i].pos[0] = hp[i].x; out[i].pos[1] = hp[i].y; out[i].pos[2] = hp[i].z;
		} else if (!(r.flags & AUD_BODY)) memcpy(out[i].pos, r.pos, 12);      // added and not updated since: where the first update will find it
		if (r.flags & AUD_GONE) out[i].status |= SGP_AUD_ST_BODY_GONE;
	}
	return SGP_OK;
}

SGP_API int sgp_audibility_get_pair_states(sgp_audibility* ab, uint32_t first, uint32_t n, sgp_audibility_pair_state* out)
{
	if (!batch_usable(ab) || (n && !out)) return fail(SGP_ERR_INVALID, "sgp_audibility_get_pair_states: NULL, or the batch's world is gone");
	if ((uint64_t)first + n > ab->slots.cap) return fail(SGP_ERR_INVALID, "sgp_audibility_get_pair_states: range beyond the batch's capacity");
	if (!n) return SGP_OK;
	sgp_world* w = ab->w;
	hipSetDevice(w->device);
	ray_server_stop(w);
	const size_t lc = ab->lcap;
	StageCarve c;
	const size_t st_off = c.add(sizeof(uint4) * (size_t)n), pr_off = c.add(sizeof(AudPair) * (size_t)n * lc);
	{ int r = ensure_stage(w, c.total); if (r != SGP_OK) return r; }
	HIP_TRY(hipMemcpyAsync(stage_h<uint4>(w, st_off), ab->d_st + first, sizeof(uint4) * (size_t)n, hipMemcpyDeviceToHost, w->stream));
	HIP_TRY(hipMemcpyAsync(stage_h<AudPair>(w, pr_off), ab->d_pairs + aud_pair_index(first, 0, ab->lcap), sizeof(AudPair) * (size_t)n * lc, hipMemcpyDeviceToHost, w->stream));
	HIP_TRY(hipStreamSynchronize(w->stream));
	const uint4* hs = stage_h<uint4>(w, st_off); const AudPair* hp = stage_h<AudPair>(w, pr_off);
	for (uint32_t i = 0; i < n; ++i) {
		const uint32_t k = first + i;
		const bool valid = source_live(ab, k) && source_state_valid(ab, k, hs[i]);
		for (uint32_t l = 0; l < ab->lcap; ++l) {
			sgp_audibility_pair_state& o = out[aud_pair_index(i, l, ab->lcap)];
			o.bits = 0u; o.mute_volume_factor = 1.0f; o.dist = 0.0f;
			const uint32_t bit = 1u << l;
			if (!valid || !(ab->live_lst & bit) || (ab->clear_lst & bit)) continue;
			if (hs[i].y & bit) o.bits |= SGP_AUD_PAIR_IN_RANGE;
			if (hs[i].z & bit) o.bits |= SGP_AUD_PAIR_OCCLUDED;
			if (hs[i].w & bit) { const AudPair& p = hp[aud_pair_index(i, l, ab->lcap)]; o.mute_volume_factor = p.factor; o.dist = p.dist; }
		}
	}
	return SGP_OK;
}

SGP_API int sgp_audibility_get_listeners(sgp_audibility* ab, uint32_t first, uint32_t n, sgp_audibility_listener_state* out)
{
	if (!batch_usable(ab) || (n && !out) || (uint64_t)first + n > ab->lcap) return fail(SGP_ERR_INVALID, "sgp_audibility_get_listeners: NULL, a range beyond the batch's listener capacity, or the batch's world is gone");
	if (!n) return SGP_OK;
	sgp_world* w = ab->w;
	hipSetDevice(w->device);
	ray_server_stop(w);
	{ int r = ensure_stage(w, sizeof(AudLstDyn) * (size_t)n); if (r != SGP_OK) return r; }
	HIP_TRY(hipMemcpyAsync(w->stage_host, ab->d_lst_dyn + first, sizeof(AudLstDyn) * (size_t)n, hipMemcpyDeviceToHost, w->stream));
	HIP_TRY(hipStreamSynchronize(w->stream));
	const AudLstDyn* hd = (const AudLstDyn*)w->stage_host;
	for (uint32_t i = 0; i < n; ++i) {
		const AudLstRec& o = ab->lst[first + i];
		memset(&out[i], 0, sizeof(out[i]));
		out[i].zone_key = SGP_INVALID_ID;
		if (!o.alive) continue;
		if (hd[i].serial == o.serial) { memcpy(out[i].pos, hd[i].pos, 12); out[i].zone_key = hd[i].zone_key; out[i].mute_outside = hd[i].mute_outside; out[i].update_index = hd[i].update_index; out[i].status = hd[i].status; }
		else if (o.source == SGP_AUD_LST_POINT) memcpy(out[i].pos, o.pos, 12);      // set and not updated since: where the first update will find it
		if (o.gone) out[i].status |= SGP_AUD_LST_ST_BODY_GONE;
	}
	return SGP_OK;
}
