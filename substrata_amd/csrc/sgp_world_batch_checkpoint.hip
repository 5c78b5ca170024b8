// sgp_world_batch_checkpoint.hip -- capture and rollback of a device-resident batch (sgp_characters, sgp_particles, sgp_crafts, sgp_movers, sgp_proximity): the part they
// share, which is all of it but the list each batch gives of its state (BatchCkptLayout, sgp_world_internal.h; docs/CONTRACT.md, "Batch checkpoints").
//
// A checkpoint holds, on the device, one buffer with a piece per listed array -- the mirrors' device copies first, then the batch's own arrays --, and on the
// host the mirrors' records, the listed arrays and scalars and the slot and link tables.  Capture and rollback are one launch each: launch_ckpt_copy where the
// host knows every length, launch_ckpt_copy_counted where a length is a word of device memory (the particles).  Neither waits for the stream; a capture whose
// buffer has to grow frees the old one, which does.
#include "sgp_world_internal.h"
#include <atomic>

struct sgp_batch_checkpoint {
	uint32_t kind = 0; uint64_t batch_serial = 0; int device = 0;
	void* dev = nullptr; size_t dev_cap = 0;
	struct Piece { size_t offset; uint32_t n; };      // where the piece lies in `dev`, and how many records it holds (a counted piece: at most)
	std::vector<Piece> pieces;
	std::vector<std::vector<char>> host; std::vector<uint32_t> host_n;      // the mirrors first, then the listed arrays
	std::vector<uint8_t> dirty;                                             // the mirrors' flags
	std::vector<char> scalars;
	std::vector<BatchSlots::Snapshot> slots; BodyLinks::Snapshot links;
	sgp_batch_checkpoint_info info{};
};

uint64_t batch_next_serial() { static std::atomic<uint64_t> last{ 0 }; return ++last; }

static inline size_t up16(size_t b) { return (b + 15) & ~size_t(15); }
static inline size_t up256(size_t b) { return (b + 255) & ~size_t(255); }

// the pieces of the device, in the checkpoint's order: the mirrors that are state, then what the batch lists (its word_piece numbers count from there)
static uint32_t device_pieces(const WorldBatch* b, const BatchCkptLayout& l, std::vector<BatchCkptLayout::Dev>& out)
{
	out.clear();
	for (const BatchMirror* m : b->mirrors) if (m->state) out.push_back(BatchCkptLayout::Dev{ m->dev, m->stride, m->count, 0u, -1, 0u });
	const uint32_t own = (uint32_t)out.size();
	out.insert(out.end(), l.dev.begin(), l.dev.end());
	for (BatchCkptLayout::Dev& d : out) if (d.count) d.n = *d.count;
	return own;
}

// one launch: `n[i]` records (at most, where counted) of every piece between the batch and the checkpoint's buffer
static int copy_pieces(const WorldBatch* b, const std::vector<BatchCkptLayout::Dev>& dev, uint32_t own, const sgp_batch_checkpoint* cp, bool to_checkpoint, const char* fn)
{
	bool counted = false;
	for (const BatchCkptLayout::Dev& d : dev) counted = counted || d.word_piece >= 0;
	if (dev.size() > (counted ? (size_t)SGP_CKPT_MAX_COUNTED : (size_t)SGP_CKPT_MAX_SEGS)) return fail_in(SGP_ERR_CAPACITY, fn, "more pieces than one launch of the copy takes");
	CkptTable t; CkptCountedTable c;
	t.n = 0; t.start[0] = 0; c.n = 0;
	uint64_t total = 0;
	for (size_t i = 0; i < dev.size(); ++i) {
		const uint32_t units = (uint32_t)(up16(dev[i].stride * (size_t)cp->pieces[i].n) / 16);
		char* a = (char*)dev[i].p; char* q = (char*)cp->dev + cp->pieces[i].offset;
		total += units;
		if (counted) {
			c.bound[c.n] = units; c.per[c.n] = (uint32_t)dev[i].stride; c.count[c.n] = nullptr;
			if (dev[i].word_piece >= 0) {
				const size_t wp = own + (size_t)dev[i].word_piece;      // the word: in the batch's array at a capture, in the checkpoint's copy of it at a rollback
				c.count[c.n] = (const uint32_t*)((to_checkpoint ? (char*)dev[wp].p : (char*)cp->dev + cp->pieces[wp].offset) + dev[i].word_off);
			}
			c.src[c.n] = to_checkpoint ? a : q; c.dst[c.n] = to_checkpoint ? q : a; c.n++;
		} else {
			t.src[t.n] = to_checkpoint ? a : q; t.dst[t.n] = to_checkpoint ? q : a;
			t.start[t.n + 1] = t.start[t.n] + units; t.n++;
		}
	}
	if (total >= 0xFFFFFF00ull) return fail_in(SGP_ERR_CAPACITY, fn, "more than 2^32 units in one launch of the copy");
	if (counted) launch_ckpt_copy_counted(c, b->w->n_cus, b->w->stream);
	else launch_ckpt_copy(t, b->w->n_cus, b->w->stream);
	HIP_TRY(hipGetLastError());
	return SGP_OK;
}

static int admit(const WorldBatch* b, uint32_t kind, const char* fn, const sgp_batch_checkpoint* cp, bool cp_needed)
{
	if (!batch_usable(b) || (cp_needed && !cp)) return fail_in(SGP_ERR_INVALID, fn, "NULL, or the batch's world is gone");
	if (cp && (cp->kind != kind || cp->batch_serial != b->serial)) return fail_in(SGP_ERR_INVALID, fn, "the checkpoint belongs to another batch");
	if (world_holds_ghosts(b->w)) return fail_ghosts(fn, "batch checkpoints");
	return SGP_OK;
}

int batch_checkpoint_capture(WorldBatch* b, uint32_t kind, const char* fn, BatchLayoutFn layout, sgp_batch_checkpoint** io)
{
	if (!io) return fail_in(SGP_ERR_INVALID, fn, "NULL");
	{ int r = admit(b, kind, fn, *io, false); if (r != SGP_OK) return r; }
	sgp_world* w = b->w;
	hipSetDevice(w->device);
	ray_server_stop(w);      // (a resident ray server must not keep this call's stream work waiting)
	{ int r = b->upload(true); if (r != SGP_OK) return r; }      // the device's copies of the mirrors are what the checkpoint holds of them
	BatchCkptLayout l;
	layout(b, l);
	std::vector<BatchCkptLayout::Dev> dev;
	const uint32_t own = device_pieces(b, l, dev);
	std::vector<sgp_batch_checkpoint::Piece> pieces;
	size_t total = 0;
	for (const BatchCkptLayout::Dev& d : dev) { pieces.push_back({ total, d.n }); total += up256(up16(d.stride * (size_t)d.n)); }
	sgp_batch_checkpoint* cp = *io;
	const bool created = cp == nullptr;
	if (!cp) { cp = new sgp_batch_checkpoint(); cp->kind = kind; cp->batch_serial = b->serial; cp->device = w->device; }
	if (total > cp->dev_cap) {
		if (cp->dev) { hipFree(cp->dev); cp->dev = nullptr; cp->dev_cap = 0; cp->pieces.clear(); }      // (waits for the copies that still use it)
		void* q = nullptr;
		const hipError_t e = hipMalloc(&q, total);
		if (e != hipSuccess) { if (created) delete cp; return fail(SGP_ERR_HIP, "batch checkpoint: hipMalloc", e); }
		cp->dev = q; cp->dev_cap = total;
	}
	*io = cp;
	cp->pieces = pieces;
	{ int r = copy_pieces(b, dev, own, cp, true, fn); if (r != SGP_OK) return r; }
	// the host's share
	size_t host_bytes = 0;
	cp->host.clear(); cp->host_n.clear(); cp->dirty.clear(); cp->scalars.clear();
	auto keep = [&](const void* p, size_t stride, uint32_t n) {
		cp->host.emplace_back((const char*)p, (const char*)p + stride * (size_t)n); cp->host_n.push_back(n); host_bytes += stride * (size_t)n;
	};
	for (const BatchMirror* m : b->mirrors) if (m->state) { keep(m->host, m->stride, *m->count); cp->dirty.push_back(m->dirty); }
	for (const BatchCkptLayout::Host& h : l.host) keep(h.p, h.stride, *h.count);
	for (const auto& s : l.scalars) cp->scalars.insert(cp->scalars.end(), (const char*)s.first, (const char*)s.first + s.second);
	cp->slots.resize(l.slots.size());
	for (size_t i = 0; i < l.slots.size(); ++i) { l.slots[i]->snapshot(cp->slots[i]); host_bytes += 4 * cp->slots[i].free_list.size(); }
	cp->links = BodyLinks::Snapshot();
	if (l.links) { l.links->snapshot(cp->links, *l.links_high); host_bytes += 5 * cp->links.state.size(); }
	sgp_batch_checkpoint_info& o = cp->info;
	memset(&o, 0, sizeof(o));
	o.device_bytes = cp->dev_cap; o.host_bytes = host_bytes + cp->scalars.size(); o.kind = kind;
	o.capacity = l.capacity; o.high_slot = l.high; o.num_alive = l.n_alive; o.world_steps_taken = w->steps_taken;
	return SGP_OK;
}

int batch_checkpoint_rollback(WorldBatch* b, uint32_t kind, const char* fn, BatchLayoutFn layout, const sgp_batch_checkpoint* cp)
{
	{ int r = admit(b, kind, fn, cp, true); if (r != SGP_OK) return r; }
	sgp_world* w = b->w;
	hipSetDevice(w->device);
	ray_server_stop(w);
	// what the batch uses NOW: records first used since the capture go back to zeroes, on both sides
	BatchCkptLayout now;
	layout(b, now);
	std::vector<BatchCkptLayout::Dev> dev;
	uint32_t own = device_pieces(b, now, dev);
	if (dev.size() != cp->pieces.size()) return fail_in(SGP_ERR_INVALID, fn, "the checkpoint holds nothing of this batch");
	for (size_t i = 0; i < dev.size(); ++i) {
		if (!dev[i].count || dev[i].n <= cp->pieces[i].n) continue;
		HIP_TRY(hipMemsetAsync((char*)dev[i].p + dev[i].stride * (size_t)cp->pieces[i].n, 0, dev[i].stride * (size_t)(dev[i].n - cp->pieces[i].n), w->stream));
	}
	size_t hi = 0;
	auto put_back = [&](void* p, size_t stride, uint32_t n_now) {
		const uint32_t n = cp->host_n[hi];
		if (n_now > n) memset((char*)p + stride * (size_t)n, 0, stride * (size_t)(n_now - n));
		if (n) memcpy(p, cp->host[hi].data(), stride * (size_t)n);
		++hi;
	};
	size_t mi = 0;
	for (BatchMirror* m : b->mirrors) if (m->state) { put_back(const_cast<void*>(m->host), m->stride, *m->count); m->dirty = cp->dirty[mi++] != 0; }
	for (const BatchCkptLayout::Host& h : now.host) put_back(h.p, h.stride, *h.count);
	size_t at = 0;
	for (const auto& s : now.scalars) { memcpy(s.first, cp->scalars.data() + at, s.second); at += s.second; }
	if (now.links) now.links->restore(cp->links, *now.links_high);      // (before the table's `high` goes back: the slots in between are free again)
	for (size_t i = 0; i < now.slots.size(); ++i) now.slots[i]->restore(cp->slots[i]);
	// the arrays as the restored scalars name them (which copy of the particles is the current one), filled from the checkpoint
	BatchCkptLayout then;
	layout(b, then);
	own = device_pieces(b, then, dev);
	return copy_pieces(b, dev, own, cp, false, fn);
}

SGP_API int sgp_batch_checkpoint_destroy(sgp_batch_checkpoint* cp)
{
	if (!cp) return SGP_OK;
	if (cp->dev) { hipSetDevice(cp->device); hipFree(cp->dev); }
	delete cp;
	return SGP_OK;
}

SGP_API int sgp_batch_checkpoint_get_info(const sgp_batch_checkpoint* cp, sgp_batch_checkpoint_info* out)
{
	if (!cp || !out) return fail(SGP_ERR_INVALID, "sgp_batch_checkpoint_get_info: NULL");
	*out = cp->info;
	return SGP_OK;
}
