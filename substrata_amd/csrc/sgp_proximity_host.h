// sgp_proximity_host.h -- the host bookkeeping of sgp_proximity that is its own (the object slots and their body links are sgp_batch_slots.h): the zone
// table with its unique keys and the generation every slot carries, and the batched add over the body links.  Host only and free of HIP types, so that
// tests/cpp/proximity_host_check.cpp can exercise it under a sanitizer without a GPU.
#pragma once
#include <stdint.h>
#include <unordered_map>
#include <vector>
#include "sgp_batch_slots.h"
#include "../../include/sgp.h"

// Zone slots: a key is unique among the live zones; gen[z] counts how often slot z was filled, so that whoever remembers (z, gen) knows a refilled slot
// from the zone it stood in.  slot_of_key is derived: rebuild() makes it from the arrays again (after a checkpoint's arrays came back).
struct ProxZoneBook {
	static constexpr uint32_t none = 0xFFFFFFFFu, duplicate = 0xFFFFFFFEu;
	BatchSlots slots;
	std::vector<uint32_t> gen, key; std::vector<uint8_t> alive;
	std::unordered_map<uint32_t, uint32_t> slot_of_key;

	void resize(uint32_t cap) { slots.cap = cap; gen.assign(cap, 0u); key.assign(cap, 0u); alive.assign(cap, (uint8_t)0); }
	bool live(uint32_t z) const { return z < slots.high && alive[z]; }
	uint32_t add(uint32_t k)      // the slot, `duplicate` (a live zone has the key) or `none` (the table is full)
	{
		if (slot_of_key.count(k)) return duplicate;
		const uint32_t z = slots.take();
		if (z == BatchSlots::none) return none;
		gen[z]++; key[z] = k; alive[z] = 1; slot_of_key[k] = z;
		return z;
	}
	bool remove(uint32_t z)
	{
		if (!live(z)) return false;
		alive[z] = 0; slot_of_key.erase(key[z]); slots.give_back(z);
		return true;
	}
	void rebuild()
	{
		slot_of_key.clear();
		for (uint32_t z = 0; z < slots.high; ++z) if (alive[z]) slot_of_key[key[z]] = z;
	}
};

// The host side of sgp_proximity_add, n objects at once, all or none: ONE walk of the body links for the whole call (a body that was reborn lets go of its
// old object first), then the descs are checked against the links and against each other, then every slot is taken, attached and filled.  `qualifies(body)`:
// what the batch asks of a body; `born_of(body)`: its birth number; `gone(slot)`: a slot the walk found without its body; `fill(slot, desc)`: the batch's
// record of the newcomer.  Returns 0, or why nothing was added: 1 a body does not qualify, 2 it is carried already, 3 it is named twice in the call, 4 the n
// do not all fit.
template <class Q, class B, class G, class F>
inline int prox_add(BatchSlots& slots, BodyLinks& links, const sgp_proximity_object* descs, uint32_t n, Q&& qualifies, B&& born_of, G&& gone, F&& fill, uint32_t* ids_out)
{
	links.mark_gone(slots.high, qualifies, born_of, gone);
	std::unordered_map<uint32_t, uint32_t> seen;
	seen.reserve(n);
	for (uint32_t i = 0; i < n; ++i) {
		const uint32_t b = descs[i].body;
		if (!qualifies(b)) return 1;
		if (links.carried(b)) return 2;
		if (!seen.emplace(b, i).second) return 3;
	}
	if (slots.cap - slots.n_alive < n) return 4;
	for (uint32_t i = 0; i < n; ++i) {
		const uint32_t id = slots.take();
		links.attach(id, descs[i].body, born_of(descs[i].body));
		fill(id, descs[i]);
		ids_out[i] = id;
	}
	return 0;
}
