// sgp_audibility_host.h -- the host bookkeeping of sgp_audibility that is its own (the source slots and their body links are sgp_batch_slots.h): the
// capacities a batch may have, where a pair sits in the pair table, the muting-key list, and the batched add over the body links (a POINT source has no
// body).  Host only and free of HIP types, so that tests/cpp/audibility_host_check.cpp can exercise it under a sanitizer without a GPU.
#pragma once
#include <stdint.h>
#include <unordered_map>
#include <vector>
#include "sgp_batch_slots.h"
#include "../../include/sgp.h"

// what sgp_audibility_create accepts
inline bool aud_capacities_ok(uint32_t source_capacity, uint32_t listener_capacity, uint32_t event_capacity)
{
	if (source_capacity == 0 || source_capacity > SGP_AUDIBILITY_MAX_SOURCES || listener_capacity == 0 || listener_capacity > SGP_AUD_MAX_LISTENERS || event_capacity == 0) return false;
	return (uint64_t)source_capacity * listener_capacity <= (uint64_t)SGP_AUDIBILITY_MAX_PAIRS;
}
// the pair table is source-major: a row of listener_capacity pairs per source slot
inline size_t aud_pair_index(uint32_t source, uint32_t listener, uint32_t listener_capacity) { return (size_t)source * listener_capacity + listener; }

// The zone keys whose parcel mutes outside audio: strictly ascending (the device looks a key up by bisection), none SGP_INVALID_ID.
struct AudMutingKeys {
	std::vector<uint32_t> keys;
	static bool valid(const uint32_t* k, uint32_t n)
	{
		if (n > SGP_PROXIMITY_MAX_ZONES) return false;
		for (uint32_t i = 0; i < n; ++i) { if (k[i] == SGP_INVALID_ID) return false; if (i && k[i] <= k[i - 1]) return false; }
		return true;
	}
	bool set(const uint32_t* k, uint32_t n) { if (!valid(k, n)) return false; keys.assign(k, k + n); return true; }
	bool contains(uint32_t key) const      // the device's bisection (aud_key_mutes)
	{
		size_t lo = 0, hi = keys.size();
		while (lo < hi) { const size_t mid = (lo + hi) >> 1; if (keys[mid] < key) lo = mid + 1; else hi = mid; }
		return lo < keys.size() && keys[lo] == key;
	}
};

// The host side of sgp_audibility_add, n sources at once, all or none: ONE walk of the body links for the whole call, then the BODY descs are checked
// against the links and against each other, then every slot is taken, attached (BODY) and filled.  Returns 0, or why nothing was added: 1 a body does not
// qualify, 2 it is carried already, 3 it is named twice in the call, 4 the n do not all fit.
template <class Q, class B, class G, class F>
inline int aud_add(BatchSlots& slots, BodyLinks& links, const sgp_audibility_source* descs, uint32_t n, Q&& qualifies, B&& born_of, G&& gone, F&& fill, uint32_t* ids_out)
{
	links.mark_gone(slots.high, qualifies, born_of, gone);
	std::unordered_map<uint32_t, uint32_t> seen;
	seen.reserve(n);
	for (uint32_t i = 0; i < n; ++i) {
		if (descs[i].kind != SGP_AUD_SRC_BODY) continue;
		const uint32_t b = descs[i].body;
		if (!qualifies(b)) return 1;
		if (links.carried(b)) return 2;
		if (!seen.emplace(b, i).second) return 3;
	}
	if (slots.cap - slots.n_alive < n) return 4;
	for (uint32_t i = 0; i < n; ++i) {
		const uint32_t id = slots.take();
		if (descs[i].kind == SGP_AUD_SRC_BODY) links.attach(id, descs[i].body, born_of(descs[i].body));
		else links.state[id] = BodyLinks::FREE;
		fill(id, descs[i]);
		ids_out[i] = id;
	}
	return 0;
}
