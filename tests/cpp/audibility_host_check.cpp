// The host-only bookkeeping of sgp_audibility (substrata_amd/csrc/sgp_audibility_host.h over sgp_batch_slots.h): the capacities a batch may have, the pair
// table's indexing at a listener capacity of 1 and of 32, the muting-key list, a batched add of POINT and BODY sources through the function the library
// calls, and the slot and link tables through a snapshot and back.  Host only; built with -fsanitize=address,undefined by tests/test_audibility_host.py.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <vector>
#include "../../substrata_amd/csrc/sgp_audibility_host.h"

static int g_bad = 0;
#define CHECK(cond) do { if (!(cond)) { printf("FAILED line %d: %s\n", __LINE__, #cond); ++g_bad; } } while (0)

static void capacities_and_pairs()
{
	const int bad_before = g_bad;
	CHECK(aud_capacities_ok(1, 1, 1) && aud_capacities_ok(1u << 20, 4, 1) && aud_capacities_ok(1u << 17, 32, 64));
	CHECK(!aud_capacities_ok(0, 1, 1) && !aud_capacities_ok(1, 0, 1) && !aud_capacities_ok(1, 1, 0));
	CHECK(!aud_capacities_ok((1u << 20) + 1, 1, 1) && !aud_capacities_ok(16, 33, 1));
	CHECK(!aud_capacities_ok((1u << 17) + 1, 32, 1) && !aud_capacities_ok(1u << 20, 5, 1));      // more than 2^22 pairs
	CHECK(!aud_capacities_ok(0xFFFFFFFFu, 0xFFFFFFFFu, 1));                                        // (the product is formed in 64 bits)
	// a pair table as the batch lays it out: every pair has its own record, rows do not overlap, the last pair is the last record
	for (uint32_t lcap : { 1u, 32u }) {
		const uint32_t n = 1000;
		std::vector<uint8_t> table((size_t)n * lcap, 0);
		for (uint32_t s = 0; s < n; ++s) for (uint32_t l = 0; l < lcap; ++l) table[aud_pair_index(s, l, lcap)]++;
		CHECK(std::all_of(table.begin(), table.end(), [](uint8_t c) { return c == 1; }));
		CHECK(aud_pair_index(n - 1, lcap - 1, lcap) == table.size() - 1 && aud_pair_index(7, 0, lcap) == 7u * lcap);
	}
	CHECK(aud_pair_index((1u << 17) - 1, 31, 32) == ((size_t)1 << 22) - 1);
	if (g_bad == bad_before) printf("capacities and pairs: ok\n");
}

static void muting_keys()
{
	const int bad_before = g_bad;
	AudMutingKeys m;
	CHECK(!m.contains(0) && !m.contains(SGP_INVALID_ID));
	const uint32_t a[] = { 3, 8, 9, 200, 4000000000u };
	CHECK(m.set(a, 5) && m.keys.size() == 5);
	for (uint32_t k : a) CHECK(m.contains(k));
	CHECK(!m.contains(0) && !m.contains(4) && !m.contains(10) && !m.contains(4000000001u) && !m.contains(SGP_INVALID_ID));
	const uint32_t unsorted[] = { 3, 9, 8 }, twice[] = { 3, 3 }, invalid[] = { 3, SGP_INVALID_ID };
	CHECK(!m.set(unsorted, 3) && !m.set(twice, 2) && !m.set(invalid, 2) && m.keys.size() == 5 && m.contains(200));      // a refused list leaves the old one
	std::vector<uint32_t> many(SGP_PROXIMITY_MAX_ZONES + 1);
	for (size_t i = 0; i < many.size(); ++i) many[i] = (uint32_t)(2 * i);
	CHECK(!m.set(many.data(), (uint32_t)many.size()) && m.set(many.data(), SGP_PROXIMITY_MAX_ZONES));
	CHECK(m.contains(0) && m.contains(2 * (SGP_PROXIMITY_MAX_ZONES - 1)) && !m.contains(2 * SGP_PROXIMITY_MAX_ZONES) && !m.contains(1) && !m.contains(200 + 1));
	CHECK(m.set(many.data(), 0) && m.keys.empty() && !m.contains(0));
	if (g_bad == bad_before) printf("muting keys: ok\n");
}

struct Bodies {
	std::vector<uint8_t> ok; std::vector<uint32_t> born; std::vector<uint32_t> reported;
	bool qualifies(uint32_t b) const { return b < ok.size() && ok[b] != 0; }
};
static const uint32_t POINT = 0xFFFFFFFFu;      // (in the lists below: a POINT source)

// sgp_audibility_add through the function the library calls (aud_add, sgp_audibility_host.h)
static int add_many(Bodies& w, BatchSlots& s, BodyLinks& l, const std::vector<uint32_t>& bodies, std::vector<uint32_t>& ids)
{
	std::vector<sgp_audibility_source> d(bodies.size());
	for (size_t i = 0; i < bodies.size(); ++i) { d[i] = sgp_audibility_source{}; d[i].kind = bodies[i] == POINT ? SGP_AUD_SRC_POINT : SGP_AUD_SRC_BODY; d[i].body = bodies[i] == POINT ? 77u : bodies[i]; d[i].volume = 1.0f; }
	std::vector<uint32_t> out(bodies.size()), filled;
	w.reported.clear();
	const int why = aud_add(s, l, d.data(), (uint32_t)d.size(), [&w](uint32_t b) { return w.qualifies(b); }, [&w](uint32_t b) { return b < w.born.size() ? w.born[b] : 0u; },
	                        [&w](uint32_t k) { w.reported.push_back(k); }, [&filled](uint32_t id, const sgp_audibility_source&) { filled.push_back(id); }, out.data());
	if (!why) { ids = out; CHECK(filled == out); }
	else CHECK(filled.empty());
	return why;
}

static void slots_and_links()
{
	const int bad_before = g_bad;
	Bodies w; w.ok.assign(8, 1); w.born = { 1, 2, 3, 4, 5, 6, 7, 8 };
	BatchSlots s; s.cap = 6;
	BodyLinks l; l.resize(6);
	std::vector<uint32_t> ids;
	CHECK(add_many(w, s, l, { 0, POINT, 2, POINT }, ids) == 0 && ids == std::vector<uint32_t>({ 0, 1, 2, 3 }));
	CHECK(l.carried(0) && l.carried(2) && !l.carried(77) && l.state[1] == BodyLinks::FREE && l.state[3] == BodyLinks::FREE && l.state[0] == BodyLinks::ATTACHED);
	CHECK(add_many(w, s, l, { POINT, 2 }, ids) == 2 && s.n_alive == 4);                    // body 2 is carried: nothing of the call is taken, not its POINT source either
	CHECK(add_many(w, s, l, { 4, POINT, 4 }, ids) == 3 && s.n_alive == 4 && !l.carried(4));   // named twice
	w.ok[6] = 0;
	CHECK(add_many(w, s, l, { 6 }, ids) == 1 && s.n_alive == 4);                            // does not qualify
	CHECK(add_many(w, s, l, { POINT, POINT, POINT }, ids) == 4 && s.n_alive == 4);          // three do not fit two free slots
	// any number of POINT sources: they share no body
	CHECK(add_many(w, s, l, { POINT, POINT }, ids) == 0 && ids == std::vector<uint32_t>({ 4, 5 }) && s.n_alive == 6 && s.take() == BatchSlots::none);
	// a POINT source's removal frees its slot and touches no link; the slot freed last comes back first, for a BODY source this time
	s.give_back(3); s.give_back(1);
	CHECK(add_many(w, s, l, { 5 }, ids) == 0 && ids[0] == 1 && l.slot_of_body.at(5) == 1 && l.state[1] == BodyLinks::ATTACHED);
	// body 0 is reborn: the next call's walk reports its source gone, and the body may carry a new one
	w.born[0] = 9;
	CHECK(add_many(w, s, l, { 0 }, ids) == 0 && ids[0] == 3 && w.reported == std::vector<uint32_t>({ 0 }) && l.state[0] == BodyLinks::GONE && l.slot_of_body.at(0) == 3);
	// what a checkpoint keeps of the tables, and the way back
	BatchSlots::Snapshot ss; s.snapshot(ss);
	BodyLinks::Snapshot ls; l.snapshot(ls, s.high);
	l.detach(1); s.give_back(1); l.detach(3); s.give_back(3);
	CHECK(add_many(w, s, l, { POINT }, ids) == 0 && ids[0] == 3 && !l.carried(0) && !l.carried(5));
	l.restore(ls, s.high); s.restore(ss);
	CHECK(s.n_alive == 6 && s.high == 6 && s.free_list.empty());
	CHECK(l.state[0] == BodyLinks::GONE && l.state[1] == BodyLinks::RELINK && l.state[2] == BodyLinks::RELINK && l.state[3] == BodyLinks::RELINK && l.state[4] == BodyLinks::FREE && l.state[5] == BodyLinks::FREE);
	CHECK(l.carried(5) && l.carried(2) && l.carried(0) && l.slot_of_body.at(0) == 3);
	w.ok[2] = 0;      // body 2 did not come back: the next walk attaches the others under the numbers they have now and reports slot 2
	CHECK(add_many(w, s, l, {}, ids) == 0 && w.reported == std::vector<uint32_t>({ 2 }) && l.state[1] == BodyLinks::ATTACHED && l.born[3] == 9 && l.state[2] == BodyLinks::GONE);
	if (g_bad == bad_before) printf("slots and links: ok\n");
}

int main()
{
	capacities_and_pairs();
	muting_keys();
	slots_and_links();
	if (g_bad) printf("%d checks failed\n", g_bad);
	return g_bad ? 1 : 0;
}
