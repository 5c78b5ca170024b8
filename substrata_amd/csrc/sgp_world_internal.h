// sgp_world_internal.h -- what the host-side files of libsgp.so share: the world record (sgp_world), error reporting, device allocation helpers and
// the handful of functions one file defines and another calls.  Not part of the ABI (include/sgp.h is); nothing here is exported.
//   sgp_world.hip            defaults, world construction, the launch plan and the step (think), command flush, events
//   sgp_world_bodies.hip     body lifecycle, setters, forces, read-back (addObject / setters / getters of PhysicsWorld)
//   sgp_world_shapes.hip     meshes, convex hulls, vehicles
//   sgp_world_queries.hip    rays, capsule queries, sphere casts, shape queries (sgp_collide_shapes), shape casts (sgp_cast_shapes); the query prologue
//   sgp_world_characters.hip the batched character controller (sgp_characters_*)
//   sgp_world_particles.hip  the batched point particles (sgp_particles_*)
//   sgp_world_crafts.hip     the batched hover cars and boats (sgp_crafts_*)
//   sgp_world_movers.hip     the batched path and move-to controllers (sgp_movers_*), sgp_path_prepare / sgp_path_advance
//                            (what the four batches share on the host -- owner, device arrays, uploaded mirrors, the skeletons of create, destroy, update
//                            and get_states: WorldBatch, below; their slots and body links: sgp_batch_slots.h)
//   sgp_stage_carve.h        the regions of one call in the stage buffer (host only, no HIP types)
//   sgp_batch_slots.h        a batch's slot table and the bodies its slots are attached to (host only, no HIP types)
//   sgp_world_tiles.hip      ghost import / export, the tile exchange over RCCL, re-tiling
//   sgp_world_snapshots.hip  the network snapshot codec and the de-jitter queue (host only)
//   sgp_world_checkpoint.hip capture, rollback, the checkpoint blob and restore
#pragma once
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include <unordered_map>
#include <map>
#include <chrono>
#include <memory>
#include <mutex>
#include <set>
#include "sgp_kernels.h"
#include "sgp_device_vehicle.h"
#include "sgp_hull_build.h"
#include "sgp_stage_carve.h"
#include "sgp_batch_slots.h"

#define SGP_API extern "C" __attribute__((visibility("default")))

extern thread_local std::string g_last_error;      // (defined in sgp_world.hip)
extern int g_device_count;

inline int fail(int code, const char* what, hipError_t e = hipSuccess)
{
	char buf[512];
	if (e != hipSuccess) snprintf(buf, sizeof(buf), "%s: %s", what, hipGetErrorString(e));
	else snprintf(buf, sizeof(buf), "%s", what);
	g_last_error = buf;
	return code;
}
#define HIP_TRY(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) return fail(SGP_ERR_HIP, #expr, e_); } while (0)

inline const char* const k_class_names[KC_COUNT] = {
	"apply_forces", "bp_cell", "bp_scan", "bp_scatter", "bp_pairs", "bp_large", "narrowphase", "wake",
	"colour_claim", "colour_commit", "colour_count", "setup", "warm_start", "solve_velocity",
	"integrate_pose", "solve_position", "finalize", "island_hook", "island_flag", "sleep_apply", "buoyancy",
	"cache_build", "misc", "edit", "gather", "prep_bodies", "vehicle" };

// ---------------------------------------------------------------------------------------------------------------

struct HostBody {
	uint32_t flags = 0;          // mirror of the static part of the device flags (alive, motion, layer, shape, large)
	uint64_t userdata = 0;
	float bound_radius = 0.0f;
	float volume = 0.0f;         // Shape::GetVolume of the current shape
	bool ghost = false;
	uint32_t shape_ref = 0;                // the mesh / hull id the body references (0 = none): keeps sgp_mesh_destroy / sgp_hull_destroy honest
	uint32_t comp_root = SGP_INVALID_ID;   // child of a static compound body: slot of the compound (= its first child), else invalid
	uint32_t comp_child = 0;               // index among the compound's children
	uint8_t in_large_ids = 0;              // listed in sgp_world::large_ids (no search needed to know)
	uint8_t lg_state = 0;                  // the static large bodies' grid: 0 not in it, 1 in the device grid, 2 waiting on the linear list for the next rebuild
	uint8_t lg_tomb = 0;                   // this id still has a (dead) entry in the device grid: giving the slot to a new body forces the rebuild
};

// A static compound body (sgp_body_add_compound): the slots of its children and their poses in the compound's frame
struct CompoundRec { std::vector<uint32_t> ids; std::vector<sgp_compound_child> children; float pos[3]; float rot[4]; };

struct ProfEvent { int kc; hipEvent_t a, b; };

// ---- the device arrays of a world ---------------------------------------------------------------------------------------------------------------------------
// Every device allocation of a sgp_world has one record in sgp_world::arrays, made at the line that allocates the array (DEV_ALLOC, dev_array_grow below): its
// checkpoint id, what of it is state, where it is and how large.  Allocating, growing, freeing and sgp_step_stats::device_bytes all go through the records,
// and sgp_world_checkpoint.hip walks them (for_each_array) -- a new array is an id here and the line that allocates it.
// What of an array is state, by kind (`stride`: bytes per counted record; the counts: CkptCounts):
//   body      one record per body slot: the first `high` records
//   cache     a constraint buffer; the one the LAST step solved is the contact cache (its first cache_total[buffer] slots are state), the other one scratch
//   table     the contact cache's hash table: the first *ht_cur entries (look-ups mask with it; k_island_mark clears what a larger table adds before anything reads it)
//   vehicles  the first n_vehicles records
//   whole     scalars and small tables, copied whole
//   scratch   rewritten by every step before it is read, or re-made from a host mirror that is the truth: nothing of it in a lean checkpoint (a full one copies it whole)
//   never     no part of any checkpoint (the stage buffer)
enum ArrayKind : char { AK_BODY = 'B', AK_CACHE = 'C', AK_TABLE = 'T', AK_VEHICLES = 'V', AK_WHOLE = 'W', AK_SCRATCH = 'S', AK_NEVER = 'N' };
// The ids: a checkpoint blob names arrays by them, so a number is never changed or used again, and a new array takes the next free one.
// (Arrays a world does not have -- the contact-event lists before they are asked for, the vehicle arrays before the first vehicle -- leave their ids unused.)
enum ArrayId : uint32_t {
	A_POSE = 1, A_VEL = 2, A_DYN = 3, A_FORCE = 4, A_TORQUE = 5, A_FLAGS = 6, A_AABB_MIN = 7, A_AABB_MAX = 8,
	A_SLEEP_S = 9,      // + k, k < 3
	A_SLEEP_TIMER = 12, A_SUBMERGED = 13, A_USERDATA = 14, A_COLOUR_MASK = 15, A_WARM = 16,
	A_CLAIM = 17,       // + k, k < 2
	A_VEH_CLAIM = 19, A_VEH_EPOCH = 20, A_ISLAND = 21, A_ISLAND_AWAKE = 22, A_AWAKE_MARK = 23, A_EXPORT_COUNTS = 24, A_CELL_HASH = 25,
	A_CELL_COUNT = 26, A_CELL_START = 27, A_CELL_FILL = 28, A_TILE_SLOT = 29, A_TILE_OF_SLOT = 30,
	A_LARGE = 31, A_LGRID = 32, A_LG_START = 33, A_LG_ITEMS = 34,
	A_MESH_PAIRS = 35, A_MESH_BIG = 36, A_HULL_PAIRS = 37, A_HULL_WORK = 38, A_SORTED_MIN = 39, A_SORTED_MAX = 40,
	A_GRID = 41, A_GRID_CELLS_USED = 42, A_BOUNDS_ACC = 43, A_SCAN_BLOCK_SUMS = 44, A_PAIRS = 45, A_WAKE_PAIRS = 46,
	A_SLEEP_LABEL = 47, A_LABEL_WAKE = 48, A_SLOT_GEN = 49,
	A_MAN_AB = 50, A_MAN_N = 51, A_MAN_COLOUR = 52, A_MAN_PRIO = 53, A_MAN_PREV = 54, A_MAN_SLOT = 55,
	A_HC_ROOT = 56, A_HC_COUNT = 57, A_HC_BASE = 58, A_HC_RANK = 59, A_HC_LIST = 60, A_HC_ENTRY = 61, A_HC_BIG_LIST = 62,
	A_ULIST = 63,       // + k, k < 2
	A_MAN_P1 = 65, A_MAN_P2 = 66,      // + 2 k, k < 4
	A_ROWS = 73,
	A_CA = 74,          // + CA_IDS * buffer + one of the offsets below (alloc_constraints)
	CA_HDR = 0, CA_N_FRIC = 1, CA_PREC = 2, CA_R1B = 3, CA_R2E = 4, CA_LAM = 5, CA_EFFT = 6, CA_LOC1 = 7, CA_LOC2 = 8,      // the last six: + 6 k, k < 4
	CA_IDS = 27,
	A_HT = 128, A_HT_CUR = 129, A_CACHE_TOTAL = 130, A_CSTARTS = 131, A_CTR = 132, A_EVC = 133,
	A_EV_ACTIVATED = 134, A_EV_DEACTIVATED = 135, A_EV_WATER = 136, A_EV_CONTACTS_ADDED = 137, A_EV_CONTACTS_PERSISTED = 138, A_SP = 139,
	A_VEHICLES = 140, A_VEH_INPUTS = 141, A_VEH_ROWS = 142, A_VEH_HEAD = 143,
	A_MESHES = 144, A_HULLS = 145, A_MESH_VERTS = 146, A_MESH_TRIS = 147, A_MESH_TRI_MAT = 148, A_MESH_NODES = 149, A_MESH_FIELD = 150,
	A_STAGE = 151,
};
struct DevArray { void* ptr; size_t bytes, counted; char kind; size_t stride; };      // counted: its share of DevArrays::bytes (what it holds, but for the vehicle heads)
struct DevArrays {
	std::map<uint32_t, DevArray> recs;      // by id: a walk meets them in the order of their ids, which is the order of a checkpoint's pieces
	uint64_t bytes = 0;                     // sgp_step_stats::device_bytes
};

struct sgp_world {
	sgp_world_desc desc;
	int device = 0;
	hipStream_t stream = nullptr;
	hipStream_t capture_stream = nullptr;      // launch plans are captured here while the step they belong to already runs, issued eagerly, on `stream`
	DV dv;
	DevArrays arrays;                                    // every device allocation of the world (checkpoints: a record's size is what a full copy moves, and the bound of its lean piece)
	bool checkpoint_full = false;                        // SGP_CHECKPOINT_FULL=1
	uint64_t serial = 0;                                 // which world of this process this is (a checkpoint names the world that made it)
	uint64_t shape_epoch = 0, shape_epoch_counter = 0;   // every shape create / destroy gives the shape tables a new epoch (a number never used before in this world): a rollback
	                                                     //   to a checkpoint of the current epoch leaves the shape pools alone; a rollback sets the epoch back, never the counter
	std::shared_ptr<const struct CkptShapes> shape_snapshot;      // host copy of the shape tables and pools of `shape_epoch`, shared by the checkpoints of that epoch (made by the first of them)
	uint32_t steps_taken = 0;
	// host mirrors
	std::vector<HostBody> hb;
	std::vector<uint32_t> free_list;
	uint32_t high = 0, n_alive = 0;
	std::vector<uint32_t> body_born; uint32_t births = 0;      // [slot]: the birth number of the body that lives there (set_body_flags); not part of a checkpoint
	std::vector<uint32_t> large_ids; bool large_dirty = false;      // every large body (host order; may hold ids that have gone: rebuild_large_grid compacts it)
	// round 4: the grid of the static large bodies is rebuilt in full only now and then -- a newcomer waits on the linear list every body walks (lg_pending
	// of them at most), a removed one stays behind as a dead entry (lg_tombs; a query skips what is not alive): streaming one parcel object in or out is
	// a 64-entry list upload or nothing at all, not a read-back and re-sort of 65k bounds (advisor r03)
	uint32_t lg_pending = 0, lg_tombs = 0; bool large_list_dirty = false;
	// what the device sees of them: the static ones in a grid of their own (LargeGrid, rebuilt when the set or a pose in it changes), the rest --
	// moving large bodies, static ones that would fill too many cells -- on the linear list the kernels walk
	std::vector<uint32_t> large_linear;
	LargeGrid* d_lgrid = nullptr; uint32_t* d_lg_start = nullptr; uint32_t* d_lg_items = nullptr; uint32_t cap_lg_items = 0; uint32_t lg_static = 0;
	uint32_t* d_large = nullptr; uint32_t cap_large = 0;
	float max_small_radius = 0.0f;
	uint32_t last_export = 0;                              // records the previous sgp_world_export_boundary produced
	std::unordered_map<uint64_t, uint64_t> ghost_map;      // global id of a ghost -> generation << 32 | local body id (stable across steps)
	std::vector<uint4> rec_creates;      // bodies the device is to create from received records: (record index, body slot, flags, -), launched by the import that queued them
	uint32_t ghost_gen = 0; bool ghost_map_stale = false; uint64_t ghost_seq_version = 1;      // version: bumped whenever ghost_seq changes (a device copy of the ids knows whether it is current)
	//      // ghost_map is rebuilt from ghost_seq when the general import path needs it
	std::vector<GhostRefresh> ghost_refresh;               // pose refreshes of existing ghosts queued by the last import (uploaded by flush_cmds)
	std::vector<std::pair<uint64_t, uint32_t>> ghost_seq;   // (global id, local id) of the previous import, in its order (fast path of the next one)
	std::unordered_map<uint32_t, CompoundRec> compounds;    // compound id (= first child's slot) -> record
	// pending edits
	std::vector<BodyCmd> cmds;
	// staging
	void* stage_dev = nullptr; size_t stage_dev_bytes = 0;
	void* stage_host = nullptr; size_t stage_host_bytes = 0;
	void* view_host = nullptr; size_t view_host_bytes = 0;       // pinned buffer of sgp_world_read_active[_poses]_view only
	StepCounters* h_ctr = nullptr; StepCounters* h_ctr_dev = nullptr;
	EventWindow* h_evw = nullptr; EventWindow* h_evw_dev = nullptr; EventCounters* h_evc = nullptr;      // host-mapped: what the step's last launch reports (h_evc = &h_evw->c)
	bool ev_reset_pending = false;                             // the host has pulled the device's event lists; their counters are emptied by the next step's first launch (or by
	                                                           //   flush_event_reset before anything else that can raise an event)
	uint32_t layer_counts[SGP_NUM_LAYERS] = { 0 };             // live, non-alias slots per layer: kept as HostBody::flags change (set_body_flags), reported by every step
	bool dirty_since_step = true;                              // an edit was flushed since the last step (or no step yet)
	bool events_on_device = true;                              // the device event lists may hold something the host vectors do not (a step without read-back, applied edits)
	StepParams sp_uploaded; bool sp_uploaded_valid = false;    // what d_sp holds (upload_sp skips the launch when nothing changed)
	uint32_t last_active = 0xFFFFFFFFu;
	StepParams* h_sp = nullptr; StepParams* d_sp = nullptr;      // pinned host copy / device copy of the per-step scalars
	std::map<std::string, hipGraphExec_t> graphs;              // replayable launch sequences keyed by launch plan
	std::string last_plan_key[2]; uint32_t plan_repeats[2] = { 0, 0 };   // per buffer parity: StepParams (by value in the first launch) flips parity every step
	bool use_graphs = true; bool use_small_world = true; bool use_wake_round = true; uint32_t tail_threshold = 256;
	uint32_t rows_mode_default = 2;        // SGP_ROWS_MODE_DEFAULT: the layout below compact_rows_min constraints -- 1 compact rows: r x axis stored (96 B per point), I (r x axis) rebuilt by the lane from the
	                                       // step's world-inverse-inertia record (DV::iw, round 5): config 3 496 -> 509, config 5 626 -> 652, config 2 915 -> 939 steps/s against 0 = full rows (192 B per point)
	bool rows_in_small_worlds = false;     // SGP_ROWS_IN_SMALL_WORLDS=1 with SGP_NO_SMALL_WORLD=1 (tools/fuzz_parity.py): worlds of up to 2048 bodies, which otherwise keep full rows, take the layouts below
	uint32_t rows_mode2_min = 65536;       // ... and below this many constraints compact rows (1) where the default says none (2): a world of 20k constraints spends its passes in the component and tail kernels, which keep a constraint for ten iterations and have the rows' use ten times (config 2: 942 against 934 steps/s)
	uint32_t rows_mode_large = 2;          // SGP_ROWS_MODE: the layout worlds of at least compact_rows_min constraints use -- 2 no rows (the lanes rebuild them from the lever arms), 1 compact rows (r x axis only)
	uint32_t compact_rows_min = 1000000;   // SGP_COMPACT_ROWS_MIN: from this many contact constraints on, the velocity rows are stored compact (96 B per point)
	// high colours by component: share of the constraints they may hold (per mille; SGP_HC_BUDGET, 0 = off), and the plan's correction of it
	// hc_k: the first colour that goes to the components (-1: not chosen yet -> the budget rule).  One colour fewer after a step that left a
	// component to the catch-all; one more after a probe (component sizes computed for hc_k - 1 without using them) found that it fits.
	bool use_components = true; uint32_t hc_budget = 160; uint32_t n_cus = 256; uint32_t hc_min_colours = 4; int hc_k = -1; uint32_t hc_bump = 1, hc_since_bump = 0xFFFFu; uint32_t hc_probe_in = 8, hc_probe_gap = 16;
	bool bp_dense_last = false;     // the previous step's broad phase met a halo too large for the small instance of k_bp_pairs
	bool plan_seen = false;         // a step has run: plan_colour_count etc. describe the previous step
	uint32_t graph_launches = 0, eager_steps = 0, idle_steps = 0;
	// single-query mailbox (sgp_raycast with n = 1): host-mapped block + whether a server wave is (believed to be) resident on the stream
	RayMailbox* ray_mb = nullptr; bool ray_server_on = false; bool ray_server_enabled = true; uint32_t ray_seq = 0, ray_gen = 0;
	uint32_t ray_server_launches = 0, ray_server_rays = 0;
	// sgp_collide_shapes: which organisation answers (SGP_QUERY_PATH: 0 by the number of queries, 1 a wave per query, 2 candidate pairs), and what the last call
	// needed per query -- the first guess of the next call's list and output capacities (a guess only: a call that overflows them grows them and runs again)
	int query_path = 0; uint32_t sq_wave_max_n = 32; float sq_pairs_per_query = 2.0f, sq_out_per_query = 4.0f; uint32_t sq_last_n = 0, sq_last_out = 0, sq_last_pairs = 0;
	// sgp_cast_shapes: what the last call needed per cast (the first guess of the next call's list capacity), runs repeated because a list was too small, pairs that ran into the iteration cap
	float sc_pairs_per_cast = 2.0f; uint32_t sc_reruns = 0, sc_capped = 0;
	bool last_step_idle = false;       // the last step was skipped (every body asleep, nothing edited): no vehicle took part in it, whatever its record says
	bool grid_valid = false;                                   // the broad-phase grid matches the current poses (ray queries reuse it)
	// static triangle meshes: host-side headers + pools mirrored on the device (grown on demand)
	std::vector<MeshHeader> meshes; std::vector<float4> mesh_verts; std::vector<uint4> mesh_tris; std::vector<uint32_t> mesh_tri_mat; std::vector<MeshNode> mesh_nodes;
	MeshHeader* d_meshes = nullptr; float4* d_mesh_verts = nullptr; uint4* d_mesh_tris = nullptr; uint32_t* d_mesh_tri_mat = nullptr; MeshNode* d_mesh_nodes = nullptr;
	size_t cap_mesh_verts = 0, cap_mesh_tris = 0, cap_mesh_tri_mat = 0, cap_mesh_nodes = 0;
	std::vector<uint32_t> mesh_field; uint32_t* d_mesh_field = nullptr; size_t cap_mesh_field = 0;      // height fields: samples, edge bytes, materials, block ranges (MeshHeader)
	// shape lifecycle: bodies referencing each mesh / hull, ids and pool ranges of destroyed shapes waiting for reuse, table capacities (grown on demand)
	std::vector<uint32_t> mesh_refs, hull_refs, free_mesh_ids, free_hull_ids;
	uint32_t n_big_hulls = 0;      // live hulls of more than SGD_HULL_SMALL_VERTS vertices: their pairs go through k_narrowphase_hull_big (part of the step plan)
	std::vector<std::pair<uint32_t, uint32_t>> free_vert_ranges, free_tri_ranges, free_node_ranges, free_field_ranges;      // (offset, length)
	size_t cap_mesh_table = 0, cap_hull_table = 0;
	std::vector<uint32_t> free_triples;                   // first slot of freed (mesh body + 2 alias) slot triples
	// convex hull shapes: host copies of the device table (mass properties, radii) -- hull 0 is the +-1 cube template
	std::vector<sgd_hull> hulls; sgd_hull* d_hulls = nullptr;
	// wheeled vehicles: device records (AoS) + host mirror of what the ABI needs without a read-back
	sgd_vehicle* d_vehicles = nullptr; sgp_vehicle_input* d_veh_inputs = nullptr; uint32_t cap_vehicles = 0, n_vehicles = 0;
	float4* d_veh_rows = nullptr; float4* d_veh_head = nullptr;      // the step's rows in the solver's lane-major layout (DV::veh_rows)
	bool fuse_vehicle_solve = true;                                  // SGP_VEHICLE_FUSED=0: the vehicles' rows in launches of their own
	std::vector<uint8_t> veh_alive; std::vector<uint32_t> veh_body; std::vector<sgp_vehicle_input> veh_inputs; bool veh_inputs_dirty = false;
	bool veh_cylinder_seen = false;                            // some vehicle casts its wheels as cylinders (SGP_VEHICLE_TESTER_CYLINDER): k_vehicle_cast's instance with that search in it
	// events collected on the host until drained
	std::vector<sgp_body_event> ev_act, ev_deact, ev_water;
	std::vector<sgp_contact_event> ev_added, ev_pers;
	// last step
	sgp_step_stats stats;
	uint32_t last_pairs = 0, last_manifolds = 0, n_con = 0;
	uint32_t plan_rounds = 12;                               // launch plan for the next step (from the last step's counters)
	uint32_t plan_round_n[32] = { 0, ~0u, ~0u, ~0u, ~0u, ~0u, ~0u, ~0u };      // uncoloured manifolds at the start of each round of the last step (no history yet: eight wide rounds)
	uint32_t plan_colour_count[SGP_MAX_COLOURS] = { 0 };
	uint32_t table_alloc = 0, ht_alloc = 0;
	// profiling
	bool profiling = false;
	std::vector<ProfEvent> prof;
	std::vector<hipEvent_t> event_pool; size_t event_next = 0;
	hipEvent_t stage_ev[SGP_NUM_STAGES + 1];
	bool stage_ev_ok = false;
};

// Array `id` of the world gets `bytes` bytes of its own: the new array is allocated, zeroed if asked, given the first `keep` bytes of the one it replaces, and
// once the stream has finished with the old one that is freed and the record and `p` name the new one.  (A first allocation has nothing to wait for.)  How large,
// how much to keep and whether to zero is the caller's; so is telling whoever holds the old pointer -- DV, and through it the captured graphs.
// uncounted: bytes at the array's end that sgp_step_stats::device_bytes has never reported (the defer bits behind the vehicle heads).  A failure leaves the old array in place.
template <typename T> inline int dev_array_grow(sgp_world* w, uint32_t id, char kind, size_t stride, T*& p, size_t bytes, size_t keep, bool zero, size_t uncounted = 0)
{
	auto it = w->arrays.recs.find(id);
	void* old = it != w->arrays.recs.end() ? it->second.ptr : nullptr;
	void* q = nullptr;
	hipError_t e = hipMalloc(&q, bytes);
	if (e != hipSuccess) return fail(SGP_ERR_HIP, "hipMalloc", e);
	if (zero) e = hipMemsetAsync(q, 0, bytes, w->stream);
	if (e == hipSuccess && old && keep) e = hipMemcpyAsync(q, old, keep, hipMemcpyDeviceToDevice, w->stream);
	if (e == hipSuccess && old) e = hipStreamSynchronize(w->stream);
	if (e != hipSuccess || old) hipFree(e != hipSuccess ? q : old);
	if (e != hipSuccess) return fail(SGP_ERR_HIP, "device array", e);
	if (old) w->arrays.bytes -= it->second.counted;
	w->arrays.recs[id] = DevArray{ q, bytes, bytes - uncounted, kind, stride };
	w->arrays.bytes += bytes - uncounted;
	p = (T*)q;
	return SGP_OK;
}
// ... and the arrays that never grow: `n` records, in whole 16-byte units (the checkpoint copy moves 16 bytes per lane), zeroed on the world's stream
template <typename T> inline int dev_alloc(sgp_world* w, uint32_t id, char kind, size_t stride, T*& p, size_t n, size_t record = sizeof(T))
{
	return dev_array_grow(w, id, kind, stride, p, (std::max<size_t>(n, 1) * record + 15) & ~size_t(15), 0, true);
}
#define DEV_ALLOC(id, kind, stride, ptr, n) do { int r_ = dev_alloc(w, id, kind, stride, ptr, n); if (r_ != SGP_OK) return r_; } while (0)
// what sgp_world_destroy does with them (the stream has been waited for)
inline void dev_arrays_release(sgp_world* w)
{
	for (auto& kv : w->arrays.recs) hipFree(kv.second.ptr);
	w->arrays.recs.clear(); w->arrays.bytes = 0;
}

inline int ensure_stage(sgp_world* w, size_t bytes)
{
	if (bytes > w->stage_dev_bytes) {
		size_t nb = std::max<size_t>(bytes, 1 << 16); nb = nb + nb / 2;
		{ int r = dev_array_grow(w, A_STAGE, AK_NEVER, 0, w->stage_dev, nb, 0, false); if (r != SGP_OK) return r; }
		w->stage_dev_bytes = nb;
	}
	if (bytes > w->stage_host_bytes) {
		if (w->stage_host) { hipStreamSynchronize(w->stream); hipHostFree(w->stage_host); }
		size_t nb = std::max<size_t>(bytes, 1 << 16); nb = nb + nb / 2;
		HIP_TRY(hipHostMalloc(&w->stage_host, nb, hipHostMallocDefault));
		w->stage_host_bytes = nb;
	}
	return SGP_OK;
}

// a region of the stage buffer (offsets: StageCarve) on the host and on the device
template <class T> inline T* stage_h(sgp_world* w, size_t off) { return StageCarve::at<T>(w->stage_host, off); }
template <class T> inline T* stage_d(sgp_world* w, size_t off) { return StageCarve::at<T>(w->stage_dev, off); }

inline uint32_t next_pow2(uint32_t v) { uint32_t p = 1; while (p < v) p <<= 1; return p; }

bool world_alive(uint64_t serial);      // (defined in sgp_world.hip)

// a tile's world: ghosts imported, or queued for import (the characters and the crafts refuse it)
static inline bool world_holds_ghosts(const sgp_world* w) { return !w->ghost_map.empty() || !w->ghost_seq.empty() || !w->ghost_refresh.empty() || !w->rec_creates.empty(); }


// ---- helpers used by several files -----------------------------------------------------------------------------------------------------------
static inline bool finite3(const float* v) { return std::isfinite(v[0]) && std::isfinite(v[1]) && std::isfinite(v[2]); }
static inline bool finite4(const float* v) { return finite3(v) && std::isfinite(v[3]); }
// The reference only asserts finite inputs in debug builds (PhysicsWorld.cpp:548-556,625,710); a NaN that gets into one body spreads through
// every contact it touches, so the setters refuse it outright.
#define REQUIRE_FINITE(cond, what) do { if (!(cond)) return fail(SGP_ERR_INVALID, what ": non-finite argument"); } while (0)
// every write of HostBody::flags goes through here: sgp_step_stats::layer_counts counts the slots that are alive and no alias slot of a mesh body, under their layer
static inline bool counts_in_layer(uint32_t f) { return (f & (BF_ALIVE | BF_ALIAS)) == BF_ALIVE; }
static inline void set_body_flags(sgp_world* w, HostBody& b, uint32_t f)
{
	if (counts_in_layer(b.flags)) w->layer_counts[(b.flags & BF_LAYER_MASK) >> BF_LAYER_SHIFT]--;
	if (counts_in_layer(f)) w->layer_counts[(f & BF_LAYER_MASK) >> BF_LAYER_SHIFT]++;
	if (!(b.flags & BF_ALIVE) && (f & BF_ALIVE)) {      // a slot is given to a new body: it gets a birth number no body of this world had before (sgp_crafts: "is this still my body?")
		const size_t id = (size_t)(&b - w->hb.data());
		if (w->body_born.size() < w->hb.size()) w->body_born.resize(w->hb.size(), 0u);
		if (id < w->body_born.size()) w->body_born[id] = ++w->births;
	}
	b.flags = f;
}
// ... and after the mirror was replaced wholesale (a rollback)
static inline void recount_layers(sgp_world* w)
{
	memset(w->layer_counts, 0, sizeof(w->layer_counts));
	for (uint32_t i = 0; i < w->high; ++i) if (counts_in_layer(w->hb[i].flags)) w->layer_counts[(w->hb[i].flags & BF_LAYER_MASK) >> BF_LAYER_SHIFT]++;
}
static inline bool live(const sgp_world* w, uint32_t id) { return w && id < w->high && (w->hb[id].flags & BF_ALIVE); }

static BodyCmd blank_cmd(uint32_t id, uint32_t ops) { BodyCmd c; memset(&c, 0, sizeof(c)); c.id = id; c.ops = ops; return c; }
// compound ids reported by queries and events: a child's slot -> the compound's id (+ the child index)
static inline uint32_t compound_id_of(const sgp_world* w, uint32_t id, uint32_t* sub_out)
{
	const HostBody& b = w->hb[id];
	if (b.comp_root == SGP_INVALID_ID) { if (sub_out) *sub_out = 0; return id; }
	if (sub_out) *sub_out = b.comp_child;
	return b.comp_root;
}

// defined in sgp_world.hip
void ray_server_stop(sgp_world* w);      // tells a resident ray server to leave (no wait: what is launched next runs after it); called by flush_cmds
void invalidate_graphs(sgp_world* w);
int grow_lg_items(sgp_world* w, uint32_t cap);      // a larger item list for the static large bodies' grid (empty; graphs invalidated)
int flush_cmds(sgp_world* w);
int collect_events(sgp_world* w, bool counters_fresh = false);
int flush_event_reset(sgp_world* w);      // empties the device's event counters now if the host has pulled the lists (before edits are applied, before a checkpoint)
int read_counters(sgp_world* w);
// defined in sgp_world.hip: the worlds of this process that exist, by serial
uint64_t world_register(); void world_unregister(uint64_t serial); bool world_alive(uint64_t serial);
// defined in sgp_world_shapes.hip
int ensure_vehicle_capacity(sgp_world* w, uint32_t need);      // grows the vehicle arrays (device pointers change: graphs are invalidated by the caller)
int shapes_upload_all(sgp_world* w);                           // the host mirrors of the shape tables and pools -> the device (pools grow through the usual path), DV updated, graphs invalidated
// defined in sgp_world_queries.hip
int query_prelude(sgp_world* w);          // flush_cmds (edits applied, the resident ray server told to leave) + ensure_query_grid: what precedes the launch of every query, characters' and particles' update
int ensure_query_grid(sgp_world* w);      // re-bins the bodies when poses changed since the broad-phase grid was built (every query's first step after flush_cmds)
// defined in sgp_world_particles.hip (struct sgp_particles is private to it): what sgp_world_crafts.hip needs of a particle batch
struct sgp_particles;
uint32_t particles_capacity(const sgp_particles* ps);
bool particles_of_world(const sgp_particles* ps, const sgp_world* w);      // usable, and of this world
int particles_append_device(sgp_particles* ps, const sgp_particle* d_recs, const uint32_t* d_count, uint32_t bound);
// defined in sgp_world_proximity.hip (struct sgp_proximity is private to it): what sgp_world_audibility.hip needs of a proximity batch
struct sgp_proximity;
bool proximity_of_world(const sgp_proximity* pb, const sgp_world* w);      // usable, and of this world
const ProxObsDyn* proximity_obs_dyn(const sgp_proximity* pb);               // the observers' device records (SGP_PROX_MAX_OBSERVERS of them)
// defined in sgp_world_bodies.hip
int add_one(sgp_world* w, const sgp_body_desc* d, uint32_t* id_out, bool ghost);
int book_record_body(sgp_world* w, uint32_t* flags_io, uint64_t userdata, float radius, float volume, bool ghost, uint32_t* id_out);      // (the host's share of add_one for a body created on the device from a record)

// ---- the host side the device-resident batches of a world share (sgp_characters, sgp_particles, sgp_crafts, sgp_movers, sgp_proximity) ------------------------
static inline int fail_in(int code, const char* fn, const char* what) { char msg[256]; snprintf(msg, sizeof(msg), "%s: %s", fn, what); return fail(code, msg); }
static inline int fail_ghosts(const char* fn, const char* whose)
{
	char msg[256]; snprintf(msg, sizeof(msg), "%s: the world holds ghost bodies (%s of tiled worlds are not supported)", fn, whose);
	return fail(SGP_ERR_INVALID, msg);
}
// the bodies a batch attaches its slots to (BodyLinks): a live body of the given motion type that is no compound child, ghost or alias slot, and the birth number it has
static inline bool body_carries(const sgp_world* w, uint32_t body, uint32_t motion)
{
	if (!live(w, body)) return false;
	const HostBody& b = w->hb[body];
	return (b.flags & BF_MOTION_MASK) == motion && !(b.flags & BF_ALIAS) && b.comp_root == SGP_INVALID_ID && !b.ghost;
}
static inline uint32_t body_born_of(const sgp_world* w, uint32_t body) { return body < w->body_born.size() ? w->body_born[body] : 0u; }

// One array the host keeps and the device gets when it changed: the host's copy, the device's, where the copy is staged in WorldBatch::h_up, and whether the
// two differ.  An upload moves the first *count units of `stride` bytes (the records up to the batch's high-water mark, the segments of the paths up to theirs).
// `state`: a batch checkpoint holds the array (not the characters' copy of the world's DV, which every update brings up to date).
struct BatchMirror { const void* host = nullptr; void* dev = nullptr; size_t stride = 0, bytes = 0, off = 0; const uint32_t* count = nullptr; bool dirty = false, state = true; };
template <class T> struct Mirror : BatchMirror {
	std::vector<T> h;
	void shape(size_t units, const uint32_t* count_, size_t per = 1)      // `units` zeroed units of `per` records each
	{
		h.resize(units * per); memset((void*)h.data(), 0, sizeof(T) * h.size());
		host = h.data(); stride = sizeof(T) * per; bytes = stride * units; count = count_;
	}
	T* d() const { return (T*)dev; }
	T& operator[](size_t i) { return h[i]; }
	const T& operator[](size_t i) const { return h[i]; }
};

// Who owns the batch; device arrays zeroed on the world's stream; the uploaded mirrors and their pinned upload buffer with its fence -- `uploaded` is recorded
// behind the copies that read the buffer and waited for before the buffer is written again, so that add, update and clear never wait for the stream --; the
// two ends of an update; the release sequence.  (batch_created, batch_destroy, batch_update_admit and batch_read_states, below, are the rest of the skeletons.)
uint64_t batch_next_serial();      // defined in sgp_world_batch_checkpoint.hip
struct WorldBatch {
	sgp_world* w = nullptr; uint64_t world_serial = 0; int device = 0;
	std::vector<void*> dev;      // the device arrays of alloc(), freed by release()
	std::vector<BatchMirror*> mirrors;      // in the order they are uploaded
	char* h_up = nullptr; hipEvent_t uploaded = nullptr; bool upload_in_flight = false;

	uint64_t serial = 0;         // no other batch of this process has it: what a batch checkpoint knows its batch by (an address may be handed out again)

	bool usable() const { return w && world_alive(world_serial); }
	bool adopt(sgp_world* world)
	{
		w = world; world_serial = world->serial; device = world->device; serial = batch_next_serial();
		return hipEventCreateWithFlags(&uploaded, hipEventDisableTiming) == hipSuccess;
	}
	bool alloc_bytes(void** p, size_t bytes)
	{
		bytes = (bytes + 15) & ~size_t(15);      // (whole 16-byte units: a checkpoint copies an array's used part rounded up to one)
		if (hipMalloc(p, bytes) != hipSuccess) { *p = nullptr; return false; }
		dev.push_back(*p);
		return hipMemsetAsync(*p, 0, bytes, w->stream) == hipSuccess;
	}
	template <typename T> bool alloc(T*& p, size_t n) { return alloc_bytes((void**)&p, std::max<size_t>(n, 1) * sizeof(T)); }
	bool pin(size_t bytes)      // a new upload buffer (the caller has seen to it that nothing reads the old one)
	{
		if (h_up) { hipHostFree(h_up); h_up = nullptr; }
		return hipHostMalloc((void**)&h_up, bytes, hipHostMallocDefault) == hipSuccess;
	}
	// the mirrors of the batch (shaped already), in upload order: their device arrays, their regions of the upload buffer, the buffer
	bool create_mirrors(std::initializer_list<BatchMirror*> list)
	{
		StageCarve up;
		for (BatchMirror* m : list) {
			m->off = up.add(m->bytes);
			if (!alloc_bytes(&m->dev, std::max<size_t>(m->bytes, 1))) return false;
			mirrors.push_back(m);
		}
		return pin(up.total);
	}
	int upload_begin() { if (upload_in_flight) { HIP_TRY(hipEventSynchronize(uploaded)); upload_in_flight = false; } return SGP_OK; }      // before h_up is written
	int upload_end() { HIP_TRY(hipEventRecord(uploaded, w->stream)); upload_in_flight = true; return SGP_OK; }                              // behind the copies that read it
	// what changed on the host -> the device, behind whatever the stream holds (no wait for the stream; only for the previous upload to have left the staging buffer)
	// (keep_dirty: a capture's upload -- the device has the host's records, and whoever looks at the flags later finds them as they were)
	int upload(bool keep_dirty = false)
	{
		bool any = false;
		for (const BatchMirror* m : mirrors) any = any || m->dirty;
		if (!any) return SGP_OK;
		{ int r = upload_begin(); if (r != SGP_OK) return r; }
		for (const BatchMirror* m : mirrors) {
			const size_t n = m->stride * *m->count;
			if (!m->dirty || !n) continue;
			memcpy(h_up + m->off, m->host, n);
			HIP_TRY(hipMemcpyAsync(m->dev, h_up + m->off, n, hipMemcpyHostToDevice, w->stream));
		}
		if (!keep_dirty) for (BatchMirror* m : mirrors) m->dirty = false;
		return upload_end();
	}
	// an update of characters, crafts or movers that has something to launch: the mirrors go up, and the event counters are emptied if the host has pulled the
	// lists (a push, a force or a move may wake a body: an activation event) ...
	int update_stage()
	{
		{ int r = upload(); if (r != SGP_OK) return r; }
		return flush_event_reset(w);
	}
	// ... and behind its launches: the update has left forces or velocities on bodies, and may have woken them, without the host hearing of it -- the next step is
	// not skipped as idle, and the event lists may hold something
	int update_end()
	{
		w->dirty_since_step = true; w->events_on_device = true;
		HIP_TRY(hipGetLastError());
		return SGP_OK;
	}
	void release()
	{
		hipSetDevice(device);
		if (usable()) hipStreamSynchronize(w->stream);      // (a destroyed world has waited for its stream already)
		for (void* p : dev) hipFree(p);
		if (h_up) hipHostFree(h_up);
		if (uploaded) hipEventDestroy(uploaded);
	}
};
static inline bool batch_usable(const WorldBatch* b) { return b && b->usable(); }

// ---- batch checkpoints (sgp_world_batch_checkpoint.hip; docs/CONTRACT.md, "Batch checkpoints") ---------------------------------------------------------------
// What a batch says of itself for a capture or a rollback: its state beyond the mirrors, which WorldBatch knows already.  Every sgp_world_<batch>.hip has one
// ckpt_layout() that lists
//   device   an array of the device, `*count` records of `stride` bytes of it in use (count == NULL: `n` records, as many at every capture)
//   counted  an array whose used part is a word of device memory: at most `bound` records of `per` bytes, and the word sits `word_off` bytes into the device
//            piece listed as number `word_piece` (the particles' PsState) -- in the batch at a capture, in the checkpoint's own copy at a rollback
//   host     an array of the host, `*count` records of it in use
//   scalar   a plain value of the host
//   slots, links   the tables of sgp_batch_slots.h
// and the counts sgp_batch_checkpoint_get_info reports.  Records beyond a count hold zeroes (as allocated), and a rollback over a count that has grown since
// the capture makes them so again, on the device and on the host.
struct BatchCkptLayout {
	struct Dev { void* p; size_t stride; const uint32_t* count; uint32_t n; int word_piece; uint32_t word_off; };
	struct Host { void* p; size_t stride; const uint32_t* count; };
	std::vector<Dev> dev; std::vector<Host> host; std::vector<std::pair<void*, size_t>> scalars;
	std::vector<BatchSlots*> slots; BodyLinks* links = nullptr; const uint32_t* links_high = nullptr;
	uint32_t capacity = 0, high = 0, n_alive = 0;
	template <class T> void device(T* p, const uint32_t* count, size_t per = 1) { dev.push_back(Dev{ (void*)p, sizeof(T) * per, count, 0u, -1, 0u }); }
	template <class T> void device_whole(T* p, uint32_t n) { dev.push_back(Dev{ (void*)p, sizeof(T), nullptr, n, -1, 0u }); }
	template <class T> void counted(T* p, size_t per, uint32_t bound, int word_piece, uint32_t word_off) { dev.push_back(Dev{ (void*)p, sizeof(T) * per, nullptr, bound, word_piece, word_off }); }
	template <class T> void host_array(std::vector<T>& v, const uint32_t* count) { host.push_back(Host{ (void*)v.data(), sizeof(T), count }); }
	template <class T> void scalar(T& v) { scalars.push_back({ (void*)&v, sizeof(T) }); }
	void table(BatchSlots& s) { slots.push_back(&s); }
	void body_links(BodyLinks& l, const uint32_t* high_) { links = &l; links_high = high_; }
};
typedef void (*BatchLayoutFn)(WorldBatch*, BatchCkptLayout&);
int batch_checkpoint_capture(WorldBatch* b, uint32_t kind, const char* fn, BatchLayoutFn layout, sgp_batch_checkpoint** io);
int batch_checkpoint_rollback(WorldBatch* b, uint32_t kind, const char* fn, BatchLayoutFn layout, const sgp_batch_checkpoint* cp);
template <class B> inline int batch_checkpoint(B* b, uint32_t kind, const char* fn, sgp_batch_checkpoint** io)
{
	return batch_checkpoint_capture(b, kind, fn, [](WorldBatch* wb, BatchCkptLayout& l) { static_cast<B*>(wb)->ckpt_layout(l); }, io);
}
template <class B> inline int batch_rollback(B* b, uint32_t kind, const char* fn, const sgp_batch_checkpoint* cp)
{
	return batch_checkpoint_rollback(b, kind, fn, [](WorldBatch* wb, BatchCkptLayout& l) { static_cast<B*>(wb)->ckpt_layout(l); }, cp);
}

// the end of every *_create (`ok`: adopt, the allocations and the pinning all succeeded) and the whole of every *_destroy
template <class B> inline int batch_created(B* b, bool ok, B** out, const char* fn)
{
	if (!ok) { (void)hipGetLastError(); b->release(); delete b; return fail_in(SGP_ERR_HIP, fn, "allocation"); }
	*out = b;
	return SGP_OK;
}
template <class B> inline int batch_destroy(B* b, const char* fn)
{
	if (!b) return fail_in(SGP_ERR_INVALID, fn, "NULL");
	b->release();
	delete b;
	return SGP_OK;
}
// what an update of characters, crafts or movers refuses (`whose`: "crafts"; `dt_rule`: what `dt_ok` asked of a finite dt -- "positive", "not negative")
static inline int batch_update_admit(const WorldBatch* b, const char* fn, const char* whose, bool dt_ok, const char* dt_rule)
{
	if (!batch_usable(b)) return fail_in(SGP_ERR_INVALID, fn, "NULL, or the batch's world is gone");
	if (!dt_ok) { char msg[256]; snprintf(msg, sizeof(msg), "%s: dt must be finite and %s", fn, dt_rule); return fail(SGP_ERR_INVALID, msg); }
	if (world_holds_ghosts(b->w)) return fail_ghosts(fn, whose);
	return SGP_OK;
}
// The opening of every *_get_states: the argument checks, the resident ray server told to leave, `before_copy()` (what the batch has to bring up to date on the
// device first), then `n` records of the device's states from `first` on copied to the stage buffer and waited for.  *staged: the records, or NULL where n == 0
// (nothing to fill).  The fill loop is the batch's own.
template <class B, class S, class F> inline int batch_read_states(B* b, const char* fn, S* B::* d_st, uint32_t first, uint32_t n, const void* out, const S** staged, F&& before_copy)
{
	*staged = nullptr;
	if (!batch_usable(b) || (n && !out)) return fail_in(SGP_ERR_INVALID, fn, "NULL, or the batch's world is gone");
	if ((uint64_t)first + n > b->slots.cap) return fail_in(SGP_ERR_INVALID, fn, "range beyond the batch's capacity");
	if (!n) return SGP_OK;
	sgp_world* w = b->w;
	hipSetDevice(w->device);
	ray_server_stop(w);
	{ int r = before_copy(); if (r != SGP_OK) return r; }
	{ int r = ensure_stage(w, sizeof(S) * (size_t)n); if (r != SGP_OK) return r; }
	HIP_TRY(hipMemcpyAsync(w->stage_host, b->*d_st + first, sizeof(S) * (size_t)n, hipMemcpyDeviceToHost, w->stream));
	HIP_TRY(hipStreamSynchronize(w->stream));
	*staged = (const S*)w->stage_host;
	return SGP_OK;
}
