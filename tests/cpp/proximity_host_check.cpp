// The host-only bookkeeping of sgp_proximity (substrata_amd/csrc/sgp_proximity_host.h over sgp_batch_slots.h): the zone table with its unique keys and the
// generation a slot carries through a refill and through a snapshot's way back, a batched add through the function the library calls, with ONE walk of the body links for the call.
// Host only; built with -fsanitize=address,undefined by tests/test_proximity_host.py.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <vector>
#include "../../substrata_amd/csrc/sgp_proximity_host.h"

static int g_bad = 0;
#define CHECK(cond) do { if (!(cond)) { printf("FAILED line %d: %s\n", __LINE__, #cond); ++g_bad; } } while (0)

static void zone_table()
{
	const int bad_before = g_bad;
	ProxZoneBook zb; zb.resize(3);
	CHECK(!zb.live(0) && zb.slots.empty());
	const uint32_t a = zb.add(70), b = zb.add(30), c = zb.add(50);
	CHECK(a == 0 && b == 1 && c == 2 && zb.gen[a] == 1 && zb.gen[b] == 1 && zb.gen[c] == 1);
	CHECK(zb.add(30) == ProxZoneBook::duplicate && zb.slots.n_alive == 3);      // a key is unique among the live zones: nothing is taken
	CHECK(zb.add(31) == ProxZoneBook::none && zb.slots.n_alive == 3);           // full
	CHECK(zb.live(b) && zb.remove(b) && !zb.live(b) && !zb.remove(b) && !zb.remove(9));
	CHECK(zb.gen[b] == 1);                                                        // a removal leaves the generation: whoever remembers (b, 1) sees "not live"
	const uint32_t d = zb.add(30);                                                // the key is free again, and the slot freed last comes back
	CHECK(d == b && zb.gen[d] == 2 && zb.live(d) && zb.slot_of_key.at(30) == d);  // refilled: another generation, so (b, 1) is still not this zone
	// what a checkpoint keeps (the arrays and the slot table) and the way back: the map is made from them again
	BatchSlots::Snapshot snap; zb.slots.snapshot(snap);
	const std::vector<uint32_t> gen = zb.gen, key = zb.key; const std::vector<uint8_t> alive = zb.alive;
	CHECK(zb.remove(a) && zb.add(99) == a && zb.gen[a] == 2 && zb.remove(c));
	zb.gen = gen; zb.key = key; zb.alive = alive; zb.slots.restore(snap); zb.rebuild();
	CHECK(zb.live(a) && zb.live(c) && zb.live(d) && zb.gen[a] == 1 && zb.key[a] == 70 && zb.slot_of_key.size() == 3 && zb.slot_of_key.at(70) == a && !zb.slot_of_key.count(99));
	CHECK(zb.add(70) == ProxZoneBook::duplicate);
	CHECK(zb.remove(a) && zb.add(99) == a && zb.gen[a] == 2);                     // the same refill gives the same generation again
	if (g_bad == bad_before) printf("zone table: ok\n");
}

// a world's bodies as far as the links care; `asked`: how often the last add asked for a birth number -- once per attached slot in ONE walk, once per newcomer
struct Bodies {
	std::vector<uint8_t> ok; std::vector<uint32_t> born;
	uint32_t asked = 0; std::vector<uint32_t> reported;
	bool qualifies(uint32_t b) const { return b < ok.size() && ok[b] != 0; }
};

// sgp_proximity_add through the function the library calls (prox_add, sgp_proximity_host.h)
static int add_many(Bodies& w, BatchSlots& s, BodyLinks& l, const std::vector<uint32_t>& bodies, std::vector<uint32_t>& ids)
{
	std::vector<sgp_proximity_object> d(bodies.size());
	for (size_t i = 0; i < bodies.size(); ++i) { d[i] = sgp_proximity_object{}; d[i].body = bodies[i]; d[i].radius = 20.0f; }
	std::vector<uint32_t> out(bodies.size()), filled;
	w.reported.clear(); w.asked = 0;
	const int why = prox_add(s, l, d.data(), (uint32_t)d.size(), [&w](uint32_t b) { return w.qualifies(b); },
	                         [&w](uint32_t b) { ++w.asked; return b < w.born.size() ? w.born[b] : 0u; }, [&w](uint32_t k) { w.reported.push_back(k); },
	                         [&filled](uint32_t id, const sgp_proximity_object&) { filled.push_back(id); }, out.data());
	if (!why) { ids = out; CHECK(filled == out); }
	else CHECK(filled.empty());
	return why;
}

static void batched_add()
{
	const int bad_before = g_bad;
	Bodies w; w.ok.assign(8, 1); w.born = { 1, 2, 3, 4, 5, 6, 7, 8 };
	BatchSlots s; s.cap = 6;
	BodyLinks l; l.resize(6);
	std::vector<uint32_t> ids;
	CHECK(add_many(w, s, l, { 0, 1, 2, 3 }, ids) == 0 && ids == std::vector<uint32_t>({ 0, 1, 2, 3 }) && w.asked == 4);      // (nothing was attached yet: the walk had nothing to ask, the four newcomers one question each)
	CHECK(add_many(w, s, l, { 4, 2 }, ids) == 2 && s.n_alive == 4 && !l.carried(4) && w.asked == 4);      // ONE walk over the four attached slots;       // body 2 is carried: nothing of the call is taken
	CHECK(add_many(w, s, l, { 4, 5, 4 }, ids) == 3 && s.n_alive == 4 && !l.carried(4));    // named twice
	w.ok[6] = 0;
	CHECK(add_many(w, s, l, { 6 }, ids) == 1 && s.n_alive == 4);                            // does not qualify
	CHECK(add_many(w, s, l, { 4, 5, 7 }, ids) == 4 && s.n_alive == 4);                      // three do not fit two free slots: none is taken
	// body 1 is reborn: the call's walk lets its old object go, and the newcomer is taken in the same call
	w.born[1] = 9;
	CHECK(add_many(w, s, l, { 1, 4 }, ids) == 0 && ids == std::vector<uint32_t>({ 4, 5 }) && w.reported == std::vector<uint32_t>({ 1 }) && w.asked == 4 + 2);
	CHECK(l.slot_of_body.at(1) == 4 && l.state[1] == BodyLinks::GONE && s.n_alive == 6);
	l.detach(1); s.give_back(1);      // the gone object's removal leaves its successor's entry
	CHECK(l.carried(1) && l.slot_of_body.at(1) == 4);
	CHECK(add_many(w, s, l, {}, ids) == 0 && ids.empty());
	if (g_bad == bad_before) printf("batched add: ok\n");
}

int main()
{
	zone_table();
	batched_add();
	if (g_bad) printf("%d checks failed\n", g_bad);
	return g_bad ? 1 : 0;
}
