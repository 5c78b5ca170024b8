// sgp_world_checkpoint.hip -- world checkpoints: capture, rollback, the blob and restore (JPH::PhysicsSystem::SaveState / RestoreState).
//
// STATE is everything the next step, query or getter can observe (docs/CONTRACT.md, "Checkpoints").  On the device that is a small part of what a world
// allocates: every device array says so where it is allocated (its ArrayKind and stride, sgp_world_internal.h), and for_each_array() below turns that into bytes.
// What is scratch was decided by reading the kernels, and is checked by the tests that restore into a fresh world and that roll back over a foreign history.
// The broad phase's "what the next step has to clear" is not copied either: rollback clears what the current grid dirtied and says so (launch_ckpt_grid_reset).
// SGP_CHECKPOINT_FULL=1 copies every array whole (scratch included; not the stage buffer) with the runtime's copies: the obviously correct statement the lean
// path is measured and tested against.
// On the host the state is the mirrors of sgp_world (CkptHost) and, shared between the checkpoints of one shape epoch, the shape tables and pools (CkptShapes).
#include "sgp_world_internal.h"

#define CKPT_MAGIC "SGPCKPT"      // 7 characters + NUL
#define CKPT_FORMAT_VERSION 2u      // 2: sgd_hull carries the hull's own centroid
#define CKPT_MAX_VEHICLES (1u << 20)

// ---- host state -----------------------------------------------------------------------------------------------------------------------------------------
struct CkptScalars {      // plain data, written to the blob as it is
	uint32_t high, n_alive, lg_pending, lg_tombs, lg_static, last_active, last_pairs, last_manifolds, n_con, plan_rounds, n_vehicles, steps_taken;
	uint32_t plan_round_n[32], plan_colour_count[SGP_MAX_COLOURS];
	uint32_t hc_bump, hc_since_bump, hc_probe_in, hc_probe_gap; int32_t hc_k;
	uint32_t large_dirty, large_list_dirty, dirty_since_step, sp_uploaded_valid, plan_seen, bp_dense_last, last_step_idle, veh_cylinder_seen;
	float max_small_radius; uint32_t pad_;
	StepParams h_sp, sp_uploaded; StepCounters h_ctr; EventCounters h_evc; sgp_step_stats stats;
};
struct CkptCompound { uint32_t id; std::vector<uint32_t> ids; std::vector<sgp_compound_child> children; float pos[3]; float rot[4]; };
struct CkptHost {
	CkptScalars s;
	std::vector<HostBody> hb;      // [0, high)
	std::vector<uint32_t> free_list, large_ids, large_linear, free_triples, mesh_refs, hull_refs, veh_body;
	std::vector<uint8_t> veh_alive; std::vector<sgp_vehicle_input> veh_inputs;
	std::vector<CkptCompound> compounds;
	std::vector<sgp_body_event> ev_act, ev_deact, ev_water; std::vector<sgp_contact_event> ev_added, ev_pers;
	size_t bytes() const
	{
		size_t b = sizeof(s) + hb.size() * sizeof(HostBody) + 4 * (free_list.size() + large_ids.size() + large_linear.size() + free_triples.size() + mesh_refs.size() + hull_refs.size() + veh_body.size());
		b += veh_alive.size() + veh_inputs.size() * sizeof(sgp_vehicle_input) + (ev_act.size() + ev_deact.size() + ev_water.size()) * sizeof(sgp_body_event) + (ev_added.size() + ev_pers.size()) * sizeof(sgp_contact_event);
		for (const CkptCompound& c : compounds) b += sizeof(CkptCompound) + c.ids.size() * 4 + c.children.size() * sizeof(sgp_compound_child);
		return b;
	}
};
struct CkptShapes {
	uint64_t epoch = 0; uint32_t n_big_hulls = 0;
	std::vector<MeshHeader> meshes; std::vector<float4> mesh_verts; std::vector<uint4> mesh_tris; std::vector<uint32_t> mesh_tri_mat; std::vector<MeshNode> mesh_nodes; std::vector<uint32_t> mesh_field;
	std::vector<sgd_hull> hulls; std::vector<uint32_t> free_mesh_ids, free_hull_ids;
	std::vector<std::pair<uint32_t, uint32_t>> free_vert_ranges, free_tri_ranges, free_node_ranges, free_field_ranges;
	size_t bytes() const
	{
		return meshes.size() * sizeof(MeshHeader) + mesh_verts.size() * 16 + mesh_tris.size() * 16 + mesh_tri_mat.size() * 4 + mesh_nodes.size() * sizeof(MeshNode) + mesh_field.size() * 4 + hulls.size() * sizeof(sgd_hull) +
		       4 * (free_mesh_ids.size() + free_hull_ids.size()) + 8 * (free_vert_ranges.size() + free_tri_ranges.size() + free_node_ranges.size() + free_field_ranges.size());
	}
};

// ---- device state ---------------------------------------------------------------------------------------------------------------------------------------
struct CkptCounts { uint32_t high, cache_n, ht_n, n_vehicles, cache_buf; };
struct CkptArray { uint32_t id; void* ptr; size_t alloc, lean; };      // one device array of the world: what it holds in all, and how much of that is state
struct CkptSeg { uint32_t id; uint32_t pad_; uint64_t bytes, lean, offset; };      // one piece a checkpoint holds (offset into its device buffer); the blob's piece table is this record

struct sgp_checkpoint {
	sgp_world* owner = nullptr; uint64_t owner_serial = 0; int device = 0; hipStream_t stream = nullptr;      // owner / stream: used only while world_alive(owner_serial)
	sgp_world_desc desc{};      // the owner's, kept here: a checkpoint may outlive its world
	bool full = false;
	void* dev = nullptr; size_t dev_cap = 0, dev_used = 0;
	std::vector<CkptSeg> segs; std::vector<void*> seg_ptr;      // seg_ptr: where the piece came from (sgp_debug_time_checkpoint_copy copies it again)
	CkptHost host;
	std::shared_ptr<const CkptShapes> shapes;
	CkptCounts counts{};
	mutable uint64_t shape_bytes_copied = 0;
	uint64_t world_device_bytes = 0;
};

static inline size_t up16(size_t b) { return (b + 15) & ~size_t(15); }
static inline size_t up256(size_t b) { return (b + 255) & ~size_t(255); }

// Every device array of the world in the order of the ids (a blob names arrays by id), and how much of each is state under the counts `c`
static void for_each_array(sgp_world* w, const CkptCounts& c, std::vector<CkptArray>& out)
{
	out.clear();
	for (const auto& kv : w->arrays.recs) {
		const uint32_t id = kv.first; const DevArray& a = kv.second;
		if (a.kind == AK_NEVER) continue;
		const size_t alloc = a.bytes;
		size_t lean = 0;
		switch (a.kind) {
		case AK_BODY: lean = (size_t)c.high * a.stride; break;
		case AK_CACHE: lean = (id >= A_CA + CA_IDS ? 1u : 0u) == c.cache_buf ? (size_t)c.cache_n * a.stride : 0; break;      // (the other buffer is where the next step writes its constraints)
		case AK_TABLE: lean = (size_t)c.ht_n * a.stride; break;
		case AK_VEHICLES: lean = (size_t)c.n_vehicles * a.stride; break;
		case AK_WHOLE: lean = alloc; break;
		default: break;
		}
		lean = std::min(up16(lean), alloc & ~size_t(15));      // (every array is allocated in whole 16-byte units or is copied up to its last whole one: hipMalloc aligns to 256)
		if (a.kind == AK_WHOLE && (alloc & 15)) lean = alloc;  // a whole array of odd size: the runtime copies it (never the kernel)
		out.push_back(CkptArray{ id, a.ptr, alloc, lean });
	}
}

// one launch (or a few, for more pieces than a table holds) of the segmented copy; to_checkpoint: world -> buffer, else back
static void copy_pieces_kernel(sgp_world* w, const std::vector<CkptSeg>& segs, const std::vector<void*>& world_ptr, const std::vector<uint64_t>& bytes, char* buf, bool to_checkpoint)
{
	CkptTable t; t.n = 0; t.start[0] = 0;
	auto flush = [&]() { if (t.n) launch_ckpt_copy(t, w->n_cus, w->stream); t.n = 0; t.start[0] = 0; };
	for (size_t i = 0; i < segs.size(); ++i) {
		if (!world_ptr[i] || !bytes[i]) continue;
		uint64_t done = 0;
		while (done < bytes[i]) {      // (a piece of more than 2^32 units is split)
			const uint64_t room = (uint64_t)0xFFFFFF00u - t.start[t.n];
			const uint64_t units = std::min((bytes[i] - done) / 16, room);
			if (t.n == SGP_CKPT_MAX_SEGS || units == 0) { flush(); continue; }
			char* a = (char*)world_ptr[i] + done; char* b = buf + segs[i].offset + done;
			t.src[t.n] = to_checkpoint ? a : b; t.dst[t.n] = to_checkpoint ? b : a;
			t.start[t.n + 1] = t.start[t.n] + (uint32_t)units; t.n++;
			done += units * 16;
		}
	}
	flush();
}

static int read_device_counts(sgp_world* w, CkptCounts& c)
{
	const DV& d = w->dv;
	{ int r = ensure_stage(w, 64); if (r != SGP_OK) return r; }
	uint32_t* h = (uint32_t*)w->stage_host;
	HIP_TRY(hipMemcpyAsync(h, d.cache_total, 8, hipMemcpyDeviceToHost, w->stream));
	HIP_TRY(hipMemcpyAsync(h + 2, d.ht_cur, 4, hipMemcpyDeviceToHost, w->stream));
	HIP_TRY(hipStreamSynchronize(w->stream));
	c.high = w->high;
	c.cache_buf = (w->h_sp->parity & 1u) ^ 1u;      // the buffer the last step solved = the contact cache of the next
	c.cache_n = std::min(h[c.cache_buf], d.cap_manifolds);
	c.ht_n = std::min(h[2], d.ht_size);
	c.n_vehicles = w->n_vehicles;
	return SGP_OK;
}

static void grab_host(const sgp_world* w, CkptHost& h)
{
	CkptScalars& s = h.s; memset(&s, 0, sizeof(s));
	s.high = w->high; s.n_alive = w->n_alive; s.lg_pending = w->lg_pending; s.lg_tombs = w->lg_tombs; s.lg_static = w->lg_static; s.last_active = w->last_active;
	s.last_pairs = w->last_pairs; s.last_manifolds = w->last_manifolds; s.n_con = w->n_con; s.plan_rounds = w->plan_rounds; s.n_vehicles = w->n_vehicles; s.steps_taken = w->steps_taken;
	memcpy(s.plan_round_n, w->plan_round_n, sizeof(s.plan_round_n)); memcpy(s.plan_colour_count, w->plan_colour_count, sizeof(s.plan_colour_count));
	s.hc_bump = w->hc_bump; s.hc_since_bump = w->hc_since_bump; s.hc_probe_in = w->hc_probe_in; s.hc_probe_gap = w->hc_probe_gap; s.hc_k = w->hc_k;
	s.large_dirty = w->large_dirty; s.large_list_dirty = w->large_list_dirty; s.dirty_since_step = w->dirty_since_step; s.sp_uploaded_valid = w->sp_uploaded_valid;
	s.plan_seen = w->plan_seen; s.bp_dense_last = w->bp_dense_last; s.last_step_idle = w->last_step_idle; s.veh_cylinder_seen = w->veh_cylinder_seen;
	s.max_small_radius = w->max_small_radius;
	s.h_sp = *w->h_sp; s.sp_uploaded = w->sp_uploaded; s.h_ctr = *w->h_ctr; s.h_evc = *w->h_evc; s.stats = w->stats;
	h.hb.assign(w->hb.begin(), w->hb.begin() + w->high);
	h.free_list = w->free_list; h.large_ids = w->large_ids; h.large_linear = w->large_linear; h.free_triples = w->free_triples; h.mesh_refs = w->mesh_refs; h.hull_refs = w->hull_refs;
	h.veh_body = w->veh_body; h.veh_alive = w->veh_alive; h.veh_inputs = w->veh_inputs;
	h.compounds.clear();
	for (const auto& kv : w->compounds) { CkptCompound c; c.id = kv.first; c.ids = kv.second.ids; c.children = kv.second.children; memcpy(c.pos, kv.second.pos, sizeof(c.pos)); memcpy(c.rot, kv.second.rot, sizeof(c.rot)); h.compounds.push_back(std::move(c)); }
	std::sort(h.compounds.begin(), h.compounds.end(), [](const CkptCompound& a, const CkptCompound& b) { return a.id < b.id; });
	h.ev_act = w->ev_act; h.ev_deact = w->ev_deact; h.ev_water = w->ev_water; h.ev_added = w->ev_added; h.ev_pers = w->ev_pers;
}

static void apply_host(sgp_world* w, const CkptHost& h)
{
	const CkptScalars& s = h.s;
	for (uint32_t i = s.high; i < w->high; ++i) w->hb[i] = HostBody{};      // slots first used after the capture
	std::copy(h.hb.begin(), h.hb.end(), w->hb.begin());
	w->high = s.high; w->n_alive = s.n_alive; w->lg_pending = s.lg_pending; w->lg_tombs = s.lg_tombs; w->lg_static = s.lg_static; w->last_active = s.last_active;
	w->last_pairs = s.last_pairs; w->last_manifolds = s.last_manifolds; w->n_con = s.n_con; w->plan_rounds = s.plan_rounds; w->n_vehicles = s.n_vehicles; w->steps_taken = s.steps_taken;
	memcpy(w->plan_round_n, s.plan_round_n, sizeof(s.plan_round_n)); memcpy(w->plan_colour_count, s.plan_colour_count, sizeof(s.plan_colour_count));
	w->hc_bump = s.hc_bump; w->hc_since_bump = s.hc_since_bump; w->hc_probe_in = s.hc_probe_in; w->hc_probe_gap = s.hc_probe_gap; w->hc_k = s.hc_k;
	w->large_dirty = s.large_dirty != 0; w->large_list_dirty = s.large_list_dirty != 0; w->dirty_since_step = s.dirty_since_step != 0; w->sp_uploaded_valid = s.sp_uploaded_valid != 0;
	w->plan_seen = s.plan_seen != 0; w->bp_dense_last = s.bp_dense_last != 0; w->last_step_idle = s.last_step_idle != 0; w->veh_cylinder_seen = s.veh_cylinder_seen != 0;
	w->max_small_radius = s.max_small_radius;
	*w->h_sp = s.h_sp; w->sp_uploaded = s.sp_uploaded; *w->h_ctr = s.h_ctr; *w->h_evc = s.h_evc; w->stats = s.stats;
	w->free_list = h.free_list; w->large_ids = h.large_ids; w->large_linear = h.large_linear; w->free_triples = h.free_triples; w->mesh_refs = h.mesh_refs; w->hull_refs = h.hull_refs;
	w->veh_body = h.veh_body; w->veh_alive = h.veh_alive; w->veh_inputs = h.veh_inputs; w->veh_inputs_dirty = true;      // (the device's copy of the inputs is uploaded again by the next step)
	w->compounds.clear();
	for (const CkptCompound& c : h.compounds) { CompoundRec r; r.ids = c.ids; r.children = c.children; memcpy(r.pos, c.pos, sizeof(r.pos)); memcpy(r.rot, c.rot, sizeof(r.rot)); w->compounds.emplace(c.id, std::move(r)); }
	w->ev_act = h.ev_act; w->ev_deact = h.ev_deact; w->ev_water = h.ev_water; w->ev_added = h.ev_added; w->ev_pers = h.ev_pers;
	w->cmds.clear(); w->ghost_refresh.clear();      // edits queued after the capture belong to the history that is being abandoned
	w->events_on_device = false; w->ev_reset_pending = false;      // (a capture leaves the device's event lists empty)
	recount_layers(w);
	w->grid_valid = false;
}

static std::shared_ptr<const CkptShapes> grab_shapes(const sgp_world* w)
{
	auto p = std::make_shared<CkptShapes>();
	p->epoch = w->shape_epoch; p->n_big_hulls = w->n_big_hulls;
	p->meshes = w->meshes; p->mesh_verts = w->mesh_verts; p->mesh_tris = w->mesh_tris; p->mesh_tri_mat = w->mesh_tri_mat; p->mesh_nodes = w->mesh_nodes; p->mesh_field = w->mesh_field;
	p->hulls = w->hulls; p->free_mesh_ids = w->free_mesh_ids; p->free_hull_ids = w->free_hull_ids;
	p->free_vert_ranges = w->free_vert_ranges; p->free_tri_ranges = w->free_tri_ranges; p->free_node_ranges = w->free_node_ranges; p->free_field_ranges = w->free_field_ranges;
	return p;
}
static int apply_shapes(sgp_world* w, const CkptShapes& p)
{
	w->n_big_hulls = p.n_big_hulls;
	w->meshes = p.meshes; w->mesh_verts = p.mesh_verts; w->mesh_tris = p.mesh_tris; w->mesh_tri_mat = p.mesh_tri_mat; w->mesh_nodes = p.mesh_nodes; w->mesh_field = p.mesh_field;
	w->hulls = p.hulls; w->free_mesh_ids = p.free_mesh_ids; w->free_hull_ids = p.free_hull_ids;
	w->free_vert_ranges = p.free_vert_ranges; w->free_tri_ranges = p.free_tri_ranges; w->free_node_ranges = p.free_node_ranges; w->free_field_ranges = p.free_field_ranges;
	return shapes_upload_all(w);
}

static bool holds_ghosts(const sgp_world* w)
{
	if (!w->ghost_map.empty() || !w->ghost_seq.empty() || !w->ghost_refresh.empty() || !w->rec_creates.empty()) return true;
	for (uint32_t i = 0; i < w->high; ++i) if (w->hb[i].ghost) return true;
	return false;
}

static void fill_info(const sgp_checkpoint* cp, sgp_checkpoint_info* o);
static uint64_t blob_size(const sgp_checkpoint* cp);

// ---- capture --------------------------------------------------------------------------------------------------------------------------------------------
SGP_API int sgp_world_checkpoint(sgp_world* w, sgp_checkpoint** io)
{
	if (!w || !io) return fail(SGP_ERR_INVALID, "sgp_world_checkpoint: NULL");
	if (*io && ((*io)->owner != w || (*io)->owner_serial != w->serial)) return fail(SGP_ERR_INVALID, "sgp_world_checkpoint: the checkpoint belongs to another world");
	if (holds_ghosts(w)) return fail(SGP_ERR_INVALID, "sgp_world_checkpoint: the world holds ghost bodies (a tiled world keeps state in sgp_tiles and on other ranks: not supported)");
	hipSetDevice(w->device);
	{ int r = flush_cmds(w); if (r != SGP_OK) return r; }      // (stops a resident ray server too)
	{ int r = collect_events(w); if (r != SGP_OK) return r; }   // raised but not drained: into the host's lists, in order -- what a drain would do first
	{ int r = flush_event_reset(w); if (r != SGP_OK) return r; }   // ... and the device's counters say so before they are copied
	CkptCounts c;
	{ int r = read_device_counts(w, c); if (r != SGP_OK) return r; }
	std::vector<CkptArray> arrays;
	for_each_array(w, c, arrays);
	const bool full = w->checkpoint_full;
	std::vector<CkptSeg> segs; std::vector<void*> ptrs; std::vector<uint64_t> bytes;
	size_t total = 0;
	for (const CkptArray& a : arrays) {
		const size_t b = full ? a.alloc : a.lean;
		if (!b) continue;
		segs.push_back(CkptSeg{ a.id, 0u, (uint64_t)b, (uint64_t)a.lean, (uint64_t)total }); ptrs.push_back(a.ptr); bytes.push_back(b);
		total += up256(b);
	}
	sgp_checkpoint* cp = *io;
	const bool created = cp == nullptr;
	if (!cp) { cp = new sgp_checkpoint(); cp->owner = w; cp->owner_serial = w->serial; cp->device = w->device; cp->stream = w->stream; cp->desc = w->desc; }
	if (total > cp->dev_cap) {
		// (the stream is idle: read_device_counts waited for it, and every earlier use of the old buffer was on this stream)
		if (cp->dev) { hipFree(cp->dev); cp->dev = nullptr; cp->dev_cap = 0; }
		const size_t nc = up256(total + total / 4 + 4096);      // some room: the next capture of a scene that is still settling fits
		void* q = nullptr;
		const hipError_t e = hipMalloc(&q, nc);
		if (e != hipSuccess) { if (created) delete cp; else cp->segs.clear(); return fail(SGP_ERR_HIP, "sgp_world_checkpoint: hipMalloc", e); }
		cp->dev = q; cp->dev_cap = nc;
	}
	*io = cp;
	cp->full = full; cp->dev_used = total; cp->segs = segs; cp->seg_ptr = ptrs; cp->counts = c; cp->world_device_bytes = w->arrays.bytes;
	if (full) {
		for (size_t i = 0; i < segs.size(); ++i) HIP_TRY(hipMemcpyAsync((char*)cp->dev + segs[i].offset, ptrs[i], bytes[i], hipMemcpyDeviceToDevice, w->stream));
	} else {
		// pieces of odd size (none today) go through the runtime, everything else through ONE launch
		std::vector<void*> kp(ptrs);
		for (size_t i = 0; i < segs.size(); ++i) if (bytes[i] & 15) { HIP_TRY(hipMemcpyAsync((char*)cp->dev + segs[i].offset, ptrs[i], bytes[i], hipMemcpyDeviceToDevice, w->stream)); kp[i] = nullptr; }
		copy_pieces_kernel(w, segs, kp, bytes, (char*)cp->dev, true);
	}
	grab_host(w, cp->host);
	if (cp->shapes && cp->shapes->epoch == w->shape_epoch) cp->shape_bytes_copied = 0;
	else {
		if (!w->shape_snapshot || w->shape_snapshot->epoch != w->shape_epoch) w->shape_snapshot = grab_shapes(w);
		cp->shapes = w->shape_snapshot;
		cp->shape_bytes_copied = cp->shapes->bytes();
	}
	return SGP_OK;
}

// ---- rollback -------------------------------------------------------------------------------------------------------------------------------------------
SGP_API int sgp_world_rollback(sgp_world* w, const sgp_checkpoint* cp)
{
	if (!w || !cp) return fail(SGP_ERR_INVALID, "sgp_world_rollback: NULL");
	if (cp->owner != w || cp->owner_serial != w->serial) return fail(SGP_ERR_INVALID, "sgp_world_rollback: the checkpoint was made by another world");
	if (cp->segs.empty() || !cp->dev) return fail(SGP_ERR_INVALID, "sgp_world_rollback: the checkpoint holds nothing");
	hipSetDevice(w->device);
	ray_server_stop(w);
	// where every piece goes NOW (an array may have been re-allocated larger since the capture: lg_items, the vehicle records)
	std::vector<CkptArray> arrays;
	for_each_array(w, cp->counts, arrays);
	std::unordered_map<uint32_t, const CkptArray*> by_id;
	for (const CkptArray& a : arrays) by_id[a.id] = &a;
	std::vector<void*> ptrs(cp->segs.size(), nullptr); std::vector<uint64_t> bytes(cp->segs.size(), 0);
	for (size_t i = 0; i < cp->segs.size(); ++i) {
		auto it = by_id.find(cp->segs[i].id);
		if (it == by_id.end()) continue;
		if (!cp->segs[i].lean && cp->segs[i].bytes != it->second->alloc) continue;      // scratch (full checkpoints only) of an array that has been re-made since
		ptrs[i] = it->second->ptr; bytes[i] = std::min<uint64_t>(cp->segs[i].bytes, it->second->alloc);
	}
	const bool lean = !cp->full;
	if (lean) launch_ckpt_grid_reset(w->dv, w->stream);      // what the CURRENT grid dirtied is cleared, and the count says so: the state every step begins its grid from
	if (cp->full) {
		for (size_t i = 0; i < cp->segs.size(); ++i) if (ptrs[i]) HIP_TRY(hipMemcpyAsync(ptrs[i], (const char*)cp->dev + cp->segs[i].offset, bytes[i], hipMemcpyDeviceToDevice, w->stream));
	} else {
		std::vector<void*> kp(ptrs);
		for (size_t i = 0; i < cp->segs.size(); ++i) if (ptrs[i] && (bytes[i] & 15)) { HIP_TRY(hipMemcpyAsync(ptrs[i], (const char*)cp->dev + cp->segs[i].offset, bytes[i], hipMemcpyDeviceToDevice, w->stream)); kp[i] = nullptr; }
		copy_pieces_kernel(w, cp->segs, kp, bytes, (char*)cp->dev, false);
	}
	if (lean && w->high > cp->counts.high) {
		// body slots first used after the capture: back to what a slot nobody has used holds (zeroes, as allocated), so that a getter that looks beyond the
		// high-water slot, and the body that is created there next, find what they find in the world that was never interrupted
		CkptCounts now = cp->counts; now.high = w->high;
		std::vector<CkptArray> later;
		for_each_array(w, now, later);
		for (const CkptArray& a : later) {
			auto it = by_id.find(a.id);
			if (it != by_id.end() && a.lean > it->second->lean) HIP_TRY(hipMemsetAsync((char*)a.ptr + it->second->lean, 0, a.lean - it->second->lean, w->stream));
		}
	}
	const uint32_t veh_before = w->dv.n_vehicles;
	apply_host(w, cp->host);
	w->dv.n_vehicles = w->n_vehicles;
	cp->shape_bytes_copied = 0;
	if (cp->shapes && cp->shapes->epoch != w->shape_epoch) {
		{ int r = apply_shapes(w, *cp->shapes); if (r != SGP_OK) return r; }
		w->shape_epoch = cp->shapes->epoch; w->shape_snapshot = cp->shapes;
		cp->shape_bytes_copied = cp->shapes->bytes();
	}
	if (veh_before != w->dv.n_vehicles) invalidate_graphs(w);      // (DV travels by value in the captured launches)
	return SGP_OK;
}

// Timing aid (tools/experiments/checkpoint_bench.py; not declared in include/sgp.h): the copy kernel alone, `reps` launches back to back
// between two events on the world's stream, each moving the pieces of `cp` from the world into the checkpoint's buffer again (call it right after the capture,
// before anything re-allocates an array: it captures the same state `reps` more times).  us_out: device time per launch; bytes_out: bytes one launch reads.
SGP_API int sgp_debug_time_checkpoint_copy(sgp_world* w, sgp_checkpoint* cp, int reps, float* us_out, uint64_t* bytes_out)
{
	if (!w || !cp || !us_out || reps < 1 || cp->owner != w || cp->owner_serial != w->serial || cp->full || !cp->dev) return fail(SGP_ERR_INVALID, "sgp_debug_time_checkpoint_copy: needs a lean checkpoint of this world");
	hipSetDevice(w->device);
	std::vector<uint64_t> bytes(cp->segs.size()); uint64_t total = 0;
	std::vector<void*> kp(cp->seg_ptr);
	for (size_t i = 0; i < cp->segs.size(); ++i) { bytes[i] = cp->segs[i].bytes; if (bytes[i] & 15) kp[i] = nullptr; else total += bytes[i]; }
	hipEvent_t e0, e1; HIP_TRY(hipEventCreate(&e0)); HIP_TRY(hipEventCreate(&e1));
	for (int r = 0; r < 3; ++r) copy_pieces_kernel(w, cp->segs, kp, bytes, (char*)cp->dev, true);
	HIP_TRY(hipEventRecord(e0, w->stream));
	for (int r = 0; r < reps; ++r) copy_pieces_kernel(w, cp->segs, kp, bytes, (char*)cp->dev, true);
	HIP_TRY(hipEventRecord(e1, w->stream));
	HIP_TRY(hipStreamSynchronize(w->stream));
	float ms = 0.0f; HIP_TRY(hipEventElapsedTime(&ms, e0, e1));
	hipEventDestroy(e0); hipEventDestroy(e1);
	*us_out = 1000.0f * ms / (float)reps;
	if (bytes_out) *bytes_out = total;
	return SGP_OK;
}

SGP_API int sgp_checkpoint_destroy(sgp_checkpoint* cp)
{
	if (!cp) return SGP_OK;
	if (cp->dev) { hipSetDevice(cp->device); hipFree(cp->dev); }      // (hipFree waits for the device: the world -- and its stream -- may be gone already)
	delete cp;
	return SGP_OK;
}

static void fill_info(const sgp_checkpoint* cp, sgp_checkpoint_info* o)
{
	memset(o, 0, sizeof(*o));
	o->device_bytes = cp->dev_cap; o->host_bytes = cp->host.bytes() + (cp->shapes ? cp->shapes->bytes() : 0);
	o->blob_bytes = blob_size(cp); o->world_device_bytes = cp->world_device_bytes; o->shape_bytes_copied = cp->shape_bytes_copied;
	o->num_bodies = cp->host.s.n_alive; o->high_slot = cp->host.s.high; o->num_cached_contacts = cp->counts.cache_n; o->num_vehicles = 0;
	for (uint8_t a : cp->host.veh_alive) o->num_vehicles += a ? 1u : 0u;
	if (cp->shapes) {
		for (size_t i = 1; i < cp->shapes->meshes.size(); ++i) o->num_meshes += cp->shapes->meshes[i].nt ? 1u : 0u;
		for (size_t i = 1; i < cp->shapes->hulls.size(); ++i) o->num_hulls += cp->shapes->hulls[i].nv ? 1u : 0u;
	}
	o->num_compounds = (uint32_t)cp->host.compounds.size();
	o->steps_taken = cp->host.s.steps_taken;
}
SGP_API int sgp_checkpoint_get_info(const sgp_checkpoint* cp, sgp_checkpoint_info* out)
{
	if (!cp || !out) return fail(SGP_ERR_INVALID, "sgp_checkpoint_get_info: NULL");
	fill_info(cp, out);
	return SGP_OK;
}

// ---- the blob -------------------------------------------------------------------------------------------------------------------------------------------
// header | host section | shape section | piece table (CkptSeg records) | piece data (each piece at its offset, 16-byte aligned).  Little-endian, the records
// of this build (SGP_ABI_VERSION and the format version say which); pointer-free; userdata travels as the 64-bit numbers it is.
struct CkptBlobHeader {
	char magic[8]; uint32_t abi_version, format_version, header_bytes, desc_bytes;
	uint64_t total_bytes, host_bytes, shape_bytes, table_bytes, data_bytes;
	CkptCounts counts; uint32_t pad_[3];
	sgp_checkpoint_info info;
	sgp_world_desc desc;
};

struct Writer {
	std::vector<uint8_t> b;
	void raw(const void* p, size_t n) { const uint8_t* q = (const uint8_t*)p; b.insert(b.end(), q, q + n); while (b.size() & 7) b.push_back(0); }
	template <typename T> void pod(const T& v) { raw(&v, sizeof(T)); }
	template <typename T> void vec(const std::vector<T>& v) { const uint64_t n = v.size(); pod(n); if (n) raw(v.data(), sizeof(T) * v.size()); }
};
struct Reader {
	const uint8_t* p; uint64_t left; bool ok = true;
	bool raw(void* out, uint64_t n) { const uint64_t padded = (n + 7) & ~uint64_t(7); if (!ok || n > left || padded > left) { ok = false; return false; } memcpy(out, p, n); p += padded; left -= padded; return true; }      // (a section is a whole number of 8-byte words)
	template <typename T> bool pod(T& v) { return raw(&v, sizeof(T)); }
	template <typename T> bool vec(std::vector<T>& v, uint64_t max_n)
	{
		uint64_t n = 0; if (!pod(n)) return false;
		if (n > max_n || n > left / sizeof(T)) { ok = false; return false; }      // (no length from the blob is trusted: it must fit what is left, and the bound its meaning sets)
		v.resize((size_t)n); return n ? raw(v.data(), sizeof(T) * n) : true;
	}
};

static void write_host(Writer& wr, const CkptHost& h)
{
	wr.pod(h.s); wr.vec(h.hb); wr.vec(h.free_list); wr.vec(h.large_ids); wr.vec(h.large_linear); wr.vec(h.free_triples); wr.vec(h.mesh_refs); wr.vec(h.hull_refs);
	wr.vec(h.veh_body); wr.vec(h.veh_alive); wr.vec(h.veh_inputs);
	const uint64_t nc = h.compounds.size(); wr.pod(nc);
	for (const CkptCompound& c : h.compounds) { wr.pod(c.id); wr.vec(c.ids); wr.vec(c.children); wr.raw(c.pos, sizeof(c.pos)); wr.raw(c.rot, sizeof(c.rot)); }
	wr.vec(h.ev_act); wr.vec(h.ev_deact); wr.vec(h.ev_water); wr.vec(h.ev_added); wr.vec(h.ev_pers);
}
static bool read_host(Reader& rd, CkptHost& h, const sgp_world_desc& desc)
{
	const uint64_t N = desc.max_bodies, M = desc.max_manifolds;
	if (!rd.pod(h.s)) return false;
	const CkptScalars& s = h.s;
	if (s.high > N || s.n_alive > s.high || s.n_vehicles > CKPT_MAX_VEHICLES || (s.h_sp.parity & ~1u) || s.h_sp.n_slots > N) return false;
	if (!rd.vec(h.hb, N) || h.hb.size() != s.high) return false;
	if (!rd.vec(h.free_list, N) || !rd.vec(h.large_ids, 4 * N) || !rd.vec(h.large_linear, N) || !rd.vec(h.free_triples, N) || !rd.vec(h.mesh_refs, 1u << 24) || !rd.vec(h.hull_refs, 1u << 24)) return false;
	if (!rd.vec(h.veh_body, CKPT_MAX_VEHICLES) || !rd.vec(h.veh_alive, CKPT_MAX_VEHICLES) || !rd.vec(h.veh_inputs, CKPT_MAX_VEHICLES)) return false;
	if (h.veh_body.size() != s.n_vehicles || h.veh_alive.size() != s.n_vehicles || h.veh_inputs.size() != s.n_vehicles) return false;
	for (HostBody& b : h.hb) { b.ghost = false; if (b.comp_root != SGP_INVALID_ID && b.comp_root >= s.high) return false; }
	for (uint32_t v : h.free_list) if (v >= s.high) return false;
	for (uint32_t v : h.large_ids) if (v >= s.high) return false;
	for (uint32_t v : h.large_linear) if (v >= s.high) return false;
	for (uint32_t v : h.free_triples) if (v >= s.high) return false;
	for (uint32_t v : h.veh_body) if (v != SGP_INVALID_ID && v >= s.high) return false;
	uint64_t nc = 0; if (!rd.pod(nc) || nc > N) return false;
	h.compounds.resize((size_t)nc);
	for (CkptCompound& c : h.compounds) {
		if (!rd.pod(c.id) || !rd.vec(c.ids, SGP_MAX_COMPOUND_CHILDREN) || !rd.vec(c.children, SGP_MAX_COMPOUND_CHILDREN) || !rd.raw(c.pos, sizeof(c.pos)) || !rd.raw(c.rot, sizeof(c.rot))) return false;
		if (c.id >= s.high) return false;
		for (uint32_t v : c.ids) if (v >= s.high) return false;
	}
	if (!rd.vec(h.ev_act, 64 * N) || !rd.vec(h.ev_deact, 64 * N) || !rd.vec(h.ev_water, 64 * N) || !rd.vec(h.ev_added, 64 * M) || !rd.vec(h.ev_pers, 64 * M)) return false;
	return rd.ok;
}
static void write_shapes(Writer& wr, const CkptShapes& p)
{
	wr.pod(p.n_big_hulls); wr.vec(p.meshes); wr.vec(p.mesh_verts); wr.vec(p.mesh_tris); wr.vec(p.mesh_tri_mat); wr.vec(p.mesh_nodes); wr.vec(p.mesh_field); wr.vec(p.hulls);
	wr.vec(p.free_mesh_ids); wr.vec(p.free_hull_ids); wr.vec(p.free_vert_ranges); wr.vec(p.free_tri_ranges); wr.vec(p.free_node_ranges); wr.vec(p.free_field_ranges);
}
static bool read_shapes(Reader& rd, CkptShapes& p)
{
	const uint64_t big = 1ull << 31;
	if (!rd.pod(p.n_big_hulls) || !rd.vec(p.meshes, 1u << 24) || !rd.vec(p.mesh_verts, big) || !rd.vec(p.mesh_tris, big) || !rd.vec(p.mesh_tri_mat, big) || !rd.vec(p.mesh_nodes, big) || !rd.vec(p.mesh_field, big) || !rd.vec(p.hulls, 1u << 24)) return false;
	if (!rd.vec(p.free_mesh_ids, 1u << 24) || !rd.vec(p.free_hull_ids, 1u << 24) || !rd.vec(p.free_vert_ranges, big) || !rd.vec(p.free_tri_ranges, big) || !rd.vec(p.free_node_ranges, big) || !rd.vec(p.free_field_ranges, big)) return false;
	if (p.meshes.empty() || p.hulls.empty() || p.mesh_tri_mat.size() != p.mesh_tris.size()) return false;      // (entry 0 of both tables always exists)
	// every range a header names lies inside its pool: the kernels index the pools with them
	for (const MeshHeader& m : p.meshes) {
		if (!m.nt) continue;
		if (m.kind == MESH_KIND_FIELD) {
			if ((uint64_t)m.field_off + m.field_words > p.mesh_field.size() || m.edge_off > m.field_words || m.mat_off > m.field_words || m.blk_off > m.field_words || (uint64_t)m.fw * m.fw > m.field_words) return false;
		} else if (m.kind == MESH_KIND_TRIS) {
			if ((uint64_t)m.vert_off + m.nv > p.mesh_verts.size() || (uint64_t)m.tri_off + m.nt > p.mesh_tris.size() || (uint64_t)m.node_off + m.n_nodes > p.mesh_nodes.size() || !m.n_nodes) return false;
			for (uint32_t t = 0; t < m.nt; ++t) { const uint4 tr = p.mesh_tris[m.tri_off + t]; if (tr.x >= m.nv || tr.y >= m.nv || tr.z >= m.nv) return false; }
			for (uint32_t k = 0; k < m.n_nodes; ++k) { const MeshNode& nd = p.mesh_nodes[m.node_off + k]; if (nd.count ? ((uint64_t)nd.left + nd.count > m.nt) : (nd.left >= m.n_nodes || nd.right >= m.n_nodes)) return false; }
		} else return false;
	}
	for (uint32_t v : p.free_mesh_ids) if (v >= p.meshes.size()) return false;
	for (uint32_t v : p.free_hull_ids) if (v >= p.hulls.size()) return false;
	return rd.ok;
}

static uint64_t blob_size(const sgp_checkpoint* cp)
{
	Writer a, b; write_host(a, cp->host); if (cp->shapes) write_shapes(b, *cp->shapes);
	uint64_t data = 0; uint64_t n = 0;
	for (const CkptSeg& s : cp->segs) if (s.lean) { data += up16(s.lean); ++n; }
	return up16(sizeof(CkptBlobHeader)) + a.b.size() + b.b.size() + n * sizeof(CkptSeg) + data;
}

SGP_API int sgp_checkpoint_write(const sgp_checkpoint* cp, void* out, uint64_t cap, uint64_t* bytes_out)
{
	if (!cp || !bytes_out) return fail(SGP_ERR_INVALID, "sgp_checkpoint_write: NULL");
	if (!cp->shapes || !cp->dev) return fail(SGP_ERR_INVALID, "sgp_checkpoint_write: the checkpoint holds nothing");
	if (!world_alive(cp->owner_serial)) return fail(SGP_ERR_INVALID, "sgp_checkpoint_write: the world that made the checkpoint has been destroyed (write the blob while it exists)");
	Writer hs, ss; write_host(hs, cp->host); write_shapes(ss, *cp->shapes);
	// the pieces that are state, each cut to the part that is (a full checkpoint holds whole arrays: their beginnings are what a lean one holds)
	std::vector<CkptSeg> table; uint64_t data = 0;
	for (const CkptSeg& s : cp->segs) if (s.lean) { table.push_back(CkptSeg{ s.id, 0u, s.lean, s.lean, data }); data += up16(s.lean); }
	CkptBlobHeader h; memset(&h, 0, sizeof(h));
	memcpy(h.magic, CKPT_MAGIC, 8); h.abi_version = SGP_ABI_VERSION; h.format_version = CKPT_FORMAT_VERSION; h.header_bytes = (uint32_t)up16(sizeof(h)); h.desc_bytes = (uint32_t)sizeof(sgp_world_desc);
	h.host_bytes = hs.b.size(); h.shape_bytes = ss.b.size(); h.table_bytes = table.size() * sizeof(CkptSeg); h.data_bytes = data;
	h.total_bytes = h.header_bytes + h.host_bytes + h.shape_bytes + h.table_bytes + h.data_bytes;
	h.counts = cp->counts; fill_info(cp, &h.info); h.desc = cp->desc; h.desc.device = 0;
	*bytes_out = h.total_bytes;
	if (!out) return SGP_OK;
	if (cap < h.total_bytes) return fail(SGP_ERR_CAPACITY, "sgp_checkpoint_write: buffer too small");
	uint8_t* o = (uint8_t*)out;
	memset(o, 0, h.header_bytes); memcpy(o, &h, sizeof(h)); o += h.header_bytes;
	memcpy(o, hs.b.data(), hs.b.size()); o += hs.b.size();
	memcpy(o, ss.b.data(), ss.b.size()); o += ss.b.size();
	if (!table.empty()) memcpy(o, table.data(), h.table_bytes);
	o += h.table_bytes;
	hipSetDevice(cp->device);
	HIP_TRY(hipStreamSynchronize(cp->stream));      // the capture's copy ran on the world's stream
	size_t k = 0;
	for (const CkptSeg& s : cp->segs) {
		if (!s.lean) continue;
		HIP_TRY(hipMemcpy(o + table[k].offset, (const char*)cp->dev + s.offset, s.lean, hipMemcpyDeviceToHost));
		if (up16(s.lean) != s.lean) memset(o + table[k].offset + s.lean, 0, up16(s.lean) - s.lean);
		++k;
	}
	return SGP_OK;
}

// Everything of a blob that can be checked without a device: the header, that the sections add up to `bytes`, and that every piece lies inside the data.
static int parse_blob(const void* blob, uint64_t bytes, CkptBlobHeader& h, const char* who)
{
	char msg[160];
	auto bad = [&](const char* what) { snprintf(msg, sizeof(msg), "%s: %s", who, what); return fail(SGP_ERR_INVALID, msg); };
	if (!blob) return bad("NULL");
	if (bytes < sizeof(CkptBlobHeader)) return bad("truncated blob (shorter than a header)");
	memcpy(&h, blob, sizeof(h));
	if (memcmp(h.magic, CKPT_MAGIC, 8) != 0) return bad("not a checkpoint blob (wrong magic)");
	if (h.abi_version != SGP_ABI_VERSION || h.format_version != CKPT_FORMAT_VERSION) return bad("blob of another ABI or format version");
	if (h.header_bytes != up16(sizeof(CkptBlobHeader)) || h.desc_bytes != sizeof(sgp_world_desc)) return bad("header of another build");
	if (h.total_bytes != bytes) return bad(h.total_bytes > bytes ? "truncated blob" : "blob size does not match its header");
	// (each section is at most `bytes`, so the sum cannot wrap)
	if (h.host_bytes > bytes || h.shape_bytes > bytes || h.table_bytes > bytes || h.data_bytes > bytes) return bad("section sizes exceed the blob");
	if ((uint64_t)h.header_bytes + h.host_bytes + h.shape_bytes + h.table_bytes + h.data_bytes != bytes) return bad("section sizes do not add up to the blob's size");
	if (h.table_bytes % sizeof(CkptSeg) != 0 || (h.host_bytes & 7) || (h.shape_bytes & 7) || (h.data_bytes & 15)) return bad("misaligned section");
	const uint8_t* tab = (const uint8_t*)blob + h.header_bytes + h.host_bytes + h.shape_bytes;
	for (uint64_t i = 0; i < h.table_bytes / sizeof(CkptSeg); ++i) {
		CkptSeg s; memcpy(&s, tab + i * sizeof(CkptSeg), sizeof(s));
		if ((s.offset & 15) || s.bytes > h.data_bytes || s.offset > h.data_bytes - s.bytes || s.lean != s.bytes || !s.bytes) return bad("a piece lies outside the data section");
	}
	if (h.desc.max_bodies == 0 || h.desc.max_bodies >= (1u << 25) || h.counts.high > h.desc.max_bodies || h.counts.cache_n > h.desc.max_manifolds || h.counts.cache_buf > 1u) return bad("counts exceed the world description");
	return SGP_OK;
}

SGP_API int sgp_checkpoint_blob_info(const void* blob, uint64_t bytes, sgp_checkpoint_info* out)
{
	if (!blob || !out) return fail(SGP_ERR_INVALID, "sgp_checkpoint_blob_info: NULL");
	CkptBlobHeader h;
	{ int r = parse_blob(blob, bytes, h, "sgp_checkpoint_blob_info"); if (r != SGP_OK) return r; }
	// the host and shape sections must parse too (a device is not needed for that)
	CkptHost host; CkptShapes shapes;
	Reader r1{ (const uint8_t*)blob + h.header_bytes, h.host_bytes }; Reader r2{ (const uint8_t*)blob + h.header_bytes + h.host_bytes, h.shape_bytes };
	if (!read_host(r1, host, h.desc) || r1.left != 0 || !read_shapes(r2, shapes) || r2.left != 0) return fail(SGP_ERR_INVALID, "sgp_checkpoint_blob_info: malformed host or shape section");
	*out = h.info;      // (as sgp_checkpoint_get_info reported it when the blob was written)
	return SGP_OK;
}

static bool same_desc(sgp_world_desc a, sgp_world_desc b) { a.device = 0; b.device = 0; return memcmp(&a, &b, sizeof(a)) == 0; }

static int ensure_lg_items(sgp_world* w, size_t bytes)
{
	if (bytes <= sizeof(uint32_t) * (size_t)w->cap_lg_items) return SGP_OK;
	return grow_lg_items(w, (uint32_t)(bytes / sizeof(uint32_t)));
}

SGP_API int sgp_world_set_contact_events(sgp_world* w, int enabled);

SGP_API int sgp_world_restore(sgp_world* w, const void* blob, uint64_t bytes)
{
	if (!w || !blob) return fail(SGP_ERR_INVALID, "sgp_world_restore: NULL");
	if (w->high != 0 || w->shape_epoch_counter != 0 || w->n_vehicles != 0 || !w->cmds.empty() || w->steps_taken != 0 || holds_ghosts(w))
		return fail(SGP_ERR_INVALID, "sgp_world_restore: the world is not fresh (a body or shape has been created in it)");
	CkptBlobHeader h;
	{ int r = parse_blob(blob, bytes, h, "sgp_world_restore"); if (r != SGP_OK) return r; }
	if (!same_desc(h.desc, w->desc)) return fail(SGP_ERR_INVALID, "sgp_world_restore: the world's sgp_world_desc (capacities, gravity, settings) differs from the blob's");
	CkptHost host; auto shapes = std::make_shared<CkptShapes>();
	const uint8_t* base = (const uint8_t*)blob;
	Reader r1{ base + h.header_bytes, h.host_bytes }; Reader r2{ base + h.header_bytes + h.host_bytes, h.shape_bytes };
	if (!read_host(r1, host, h.desc) || r1.left != 0 || !read_shapes(r2, *shapes) || r2.left != 0) return fail(SGP_ERR_INVALID, "sgp_world_restore: malformed host or shape section");
	if (host.s.high != h.counts.high || host.s.n_vehicles != h.counts.n_vehicles || host.mesh_refs.size() != shapes->meshes.size() || host.hull_refs.size() != shapes->hulls.size())
		return fail(SGP_ERR_INVALID, "sgp_world_restore: the blob's sections disagree");
	hipSetDevice(w->device);
	ray_server_stop(w);
	// what may have to exist before the pieces have somewhere to go.  (None of this is physics: a refusal below leaves a world that steps as a fresh one does.)
	const size_t n_seg = h.table_bytes / sizeof(CkptSeg);
	std::vector<CkptSeg> table(n_seg);
	if (n_seg) memcpy(table.data(), base + h.header_bytes + h.host_bytes + h.shape_bytes, h.table_bytes);
	// first pass over the pieces against the arrays as they are: everything but the growable ones must fit NOW, or the world stays untouched
	std::vector<CkptArray> arrays;
	CkptCounts c = h.counts;
	for_each_array(w, c, arrays);
	std::unordered_map<uint32_t, const CkptArray*> by_id;
	for (const CkptArray& a : arrays) by_id[a.id] = &a;
	size_t lg_bytes = 0; bool want_events = host.s.h_sp.contact_events != 0;
	for (const CkptSeg& s : table) {
		if (s.id == A_LG_ITEMS) { lg_bytes = (size_t)s.bytes; if (s.bytes > (1ull << 32)) return fail(SGP_ERR_INVALID, "sgp_world_restore: a piece is larger than its array can be"); continue; }
		if (s.id == A_VEHICLES) { if (s.bytes > up16(sizeof(sgd_vehicle) * (uint64_t)host.s.n_vehicles)) return fail(SGP_ERR_INVALID, "sgp_world_restore: a piece is larger than its array"); continue; }
		auto it = by_id.find(s.id);
		if (it == by_id.end()) return fail(SGP_ERR_INVALID, "sgp_world_restore: the blob names a device array this world does not have");
		if (s.bytes > it->second->alloc) return fail(SGP_ERR_INVALID, "sgp_world_restore: a piece is larger than its array");
	}
	// from here on the world changes
	{ int r = ensure_lg_items(w, lg_bytes); if (r != SGP_OK) return r; }
	if (host.s.n_vehicles) { int r = ensure_vehicle_capacity(w, host.s.n_vehicles); if (r != SGP_OK) return r; }
	if (want_events) { int r = sgp_world_set_contact_events(w, 1); if (r != SGP_OK) return r; }
	{ int r = apply_shapes(w, *shapes); if (r != SGP_OK) return r; }
	w->shape_epoch = ++w->shape_epoch_counter; shapes->epoch = w->shape_epoch; w->shape_snapshot = shapes;
	c.n_vehicles = host.s.n_vehicles;
	w->n_vehicles = host.s.n_vehicles;
	for_each_array(w, c, arrays);
	by_id.clear(); for (const CkptArray& a : arrays) by_id[a.id] = &a;
	launch_ckpt_grid_reset(w->dv, w->stream);
	const uint8_t* data = base + h.header_bytes + h.host_bytes + h.shape_bytes + h.table_bytes;
	for (const CkptSeg& s : table) {
		auto it = by_id.find(s.id);
		if (it == by_id.end() || s.bytes > it->second->alloc) continue;      // (checked above; the growable arrays have grown)
		HIP_TRY(hipMemcpyAsync(it->second->ptr, data + s.offset, s.bytes, hipMemcpyHostToDevice, w->stream));
	}
	HIP_TRY(hipStreamSynchronize(w->stream));      // (the blob is the caller's memory)
	apply_host(w, host);
	w->dv.n_vehicles = w->n_vehicles;
	invalidate_graphs(w);
	return SGP_OK;
}
