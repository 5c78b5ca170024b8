// sgp_batch_slots.h -- the host bookkeeping the device-resident batches share (sgp_characters, sgp_crafts, sgp_movers and the movers' paths, sgp_proximity and its zones): which slots are
// handed out, and which body each slot was attached to.  Host only and free of HIP types, so that tests/cpp/batch_slots_check.cpp can exercise it under a
// sanitizer without a GPU.
#pragma once
#include <stdint.h>
#include <unordered_map>
#include <vector>

// Slots 0 .. cap - 1: `high` is one past the highest slot ever handed out (what the kernels cover; it never shrinks), `n_alive` how many are out now.
// The ids are seen through the ABI, so is their order: the slot freed last is reused first, and only then a slot never used.
struct BatchSlots {
	static constexpr uint32_t none = 0xFFFFFFFFu;
	uint32_t cap = 0, high = 0, n_alive = 0;
	std::vector<uint32_t> free_list;

	bool empty() const { return !high || !n_alive; }      // nothing for a kernel to do
	uint32_t take()                                        // a slot's id, or `none`: the table is full
	{
		uint32_t id;
		if (!free_list.empty()) { id = free_list.back(); free_list.pop_back(); }
		else if (high < cap) id = high++;
		else return none;
		n_alive++;
		return id;
	}
	void give_back(uint32_t id) { free_list.push_back(id); n_alive--; }      // (the caller knows `id` to be out)

	// What a batch checkpoint keeps of the table, and the way back: the free list in its order, so that the next take() hands out the id it would have.  `high`
	// goes back too (the table may have grown since: the owner blanks what the slots in between hold, they count as never used again); `cap` is the table's own.
	struct Snapshot { uint32_t high = 0, n_alive = 0; std::vector<uint32_t> free_list; };
	void snapshot(Snapshot& s) const { s.high = high; s.n_alive = n_alive; s.free_list = free_list; }
	void restore(const Snapshot& s) { high = s.high; n_alive = s.n_alive; free_list = s.free_list; }
};

// Which body each slot was attached to, and under which birth number (a world gives every body it creates a number no body of it had before: a body slot
// that was freed and given to a new body has another), and for every body the slot on it: a body carries one slot of a batch.  A slot whose body has gone,
// found by mark_gone, stays out -- its owner removes it -- but gives the body up for another slot.
struct BodyLinks {
	enum : uint8_t { FREE = 0, ATTACHED = 1, GONE = 2, RELINK = 3 };      // RELINK: attached in the checkpoint the table was restored from, birth number not taken yet (restore, below)
	std::vector<uint32_t> body, born;
	std::vector<uint8_t> state;
	std::unordered_map<uint32_t, uint32_t> slot_of_body;

	void resize(uint32_t cap) { body.assign(cap, 0u); born.assign(cap, 0u); state.assign(cap, (uint8_t)FREE); }
	bool carried(uint32_t b) const { return slot_of_body.count(b) != 0; }
	void attach(uint32_t slot, uint32_t b, uint32_t birth) { body[slot] = b; born[slot] = birth; state[slot] = ATTACHED; slot_of_body[b] = slot; }
	// the slot lets go of its body; a slot that was marked gone may find the body taken over by another slot, whose entry stays
	void detach(uint32_t slot)
	{
		const auto it = slot_of_body.find(body[slot]);
		if (it != slot_of_body.end() && it->second == slot) slot_of_body.erase(it);
		state[slot] = FREE;
	}
	// Walks the attached slots below `high` that are not marked yet: where `qualifies(body)` no longer holds or `born_of(body)` is not the birth number the slot
	// was attached under, the slot is marked, the body is free for another slot and `gone(slot)` is called -- once per slot, not again by a later walk.
	template <class Q, class B, class G> void mark_gone(uint32_t high, Q&& qualifies, B&& born_of, G&& gone)
	{
		for (uint32_t k = 0; k < high; ++k) {
			if (state[k] == RELINK) {
				if (qualifies(body[k])) { born[k] = born_of(body[k]); state[k] = ATTACHED; continue; }
			} else {
				if (state[k] != ATTACHED) continue;
				if (qualifies(body[k]) && born_of(body[k]) == born[k]) continue;
			}
			state[k] = GONE;
			const auto it = slot_of_body.find(body[k]);
			if (it != slot_of_body.end() && it->second == k) slot_of_body.erase(it);
			gone(k);
		}
	}

	// What a batch checkpoint keeps of the links -- the body and the state of the slots below the table's `high`, no birth numbers: a world checkpoint does not
	// hold the world's, so a body that was removed after the capture and is back after the world's rollback has the number its slot has NOW -- and the way back.
	// After restore a slot that was FREE or GONE at the capture is so again (a slot first used since is FREE), and a slot that was attached is RELINK: it holds
	// its body against other slots, and the next mark_gone -- every add and every update begins with one -- attaches it under the birth number the body slot has
	// then if `qualifies(body)` holds, and marks it gone otherwise, as it marks any other slot.  The rule waits for that walk so that the batch may be rolled back
	// ahead of its world, while the body is still missing.
	struct Snapshot { std::vector<uint32_t> body; std::vector<uint8_t> state; };
	void snapshot(Snapshot& s, uint32_t high) const { s.body.assign(body.begin(), body.begin() + high); s.state.assign(state.begin(), state.begin() + high); }
	void restore(const Snapshot& s, uint32_t high_now)
	{
		slot_of_body.clear();
		for (uint32_t k = 0; k < high_now && k < state.size(); ++k) state[k] = FREE;
		for (uint32_t k = 0; k < s.state.size() && k < state.size(); ++k) {
			body[k] = s.body[k]; born[k] = 0u;
			state[k] = s.state[k] == ATTACHED ? (uint8_t)RELINK : s.state[k];
			if (state[k] == RELINK) slot_of_body[body[k]] = k;
		}
	}
};
