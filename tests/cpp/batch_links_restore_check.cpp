// What a batch checkpoint keeps of BatchSlots and BodyLinks (substrata_amd/csrc/sgp_batch_slots.h) and the way back: the free list's order and the next id;
// the relink rule -- a slot attached at the capture is attached to the same body id under the birth number the body has NOW if the body qualifies, gone otherwise,
// decided by the first walk after the restore --; a body another slot took over since the capture; a slot that was gone at the capture; a table that grew since.
// Host only; built with -fsanitize=address,undefined by tests/test_batch_links_restore.py.
#include <cstdint>
#include <cstdio>
#include <vector>
#include "../../substrata_amd/csrc/sgp_batch_slots.h"

static int g_bad = 0;
#define CHECK(cond) do { if (!(cond)) { printf("FAILED line %d: %s\n", __LINE__, #cond); ++g_bad; } } while (0)

struct Bodies {
	std::vector<uint8_t> ok; std::vector<uint32_t> born;
	std::vector<uint32_t> reported;
	void walk(BodyLinks& l, uint32_t high)
	{
		reported.clear();
		l.mark_gone(high, [this](uint32_t b) { return b < ok.size() && ok[b] != 0; }, [this](uint32_t b) { return b < born.size() ? born[b] : 0u; },
		            [this](uint32_t k) { reported.push_back(k); });
	}
};

// the ids a table hands out until it is full
static std::vector<uint32_t> drain(BatchSlots s)
{
	std::vector<uint32_t> ids;
	for (uint32_t id = s.take(); id != BatchSlots::none; id = s.take()) ids.push_back(id);
	return ids;
}

static void slots_snapshot()
{
	const int bad_before = g_bad;
	BatchSlots s; s.cap = 6;
	for (int k = 0; k < 4; ++k) s.take();
	s.give_back(1); s.give_back(3); s.give_back(0);      // free list 1, 3, 0: the next ids are 0, 3, 1, then the unused 4, 5
	BatchSlots::Snapshot snap; s.snapshot(snap);
	const std::vector<uint32_t> expected = drain(s);
	CHECK((expected == std::vector<uint32_t>{ 0, 3, 1, 4, 5 }));
	// another history: slots taken, freed in another order, the table grown to its capacity
	CHECK(s.take() == 0 && s.take() == 3);
	s.give_back(2); s.give_back(0);
	CHECK(s.take() == 0 && s.take() == 2 && s.take() == 1 && s.take() == 4 && s.take() == 5 && s.high == 6);
	s.give_back(5);
	s.restore(snap);
	CHECK(s.high == 4 && s.n_alive == 1 && s.cap == 6 && s.free_list.size() == 3);
	CHECK(drain(s) == expected);
	// a snapshot of an empty table, restored over a used one
	BatchSlots e; e.cap = 2;
	BatchSlots::Snapshot none; e.snapshot(none);
	e.take(); e.take(); e.give_back(0);
	e.restore(none);
	CHECK(e.empty() && e.high == 0 && e.n_alive == 0 && e.take() == 0 && e.take() == 1 && e.take() == BatchSlots::none);
	if (g_bad == bad_before) printf("slots snapshot: ok\n");
}

static void relink_rule()
{
	const int bad_before = g_bad;
	Bodies w; w.ok = { 1, 1, 1, 1, 1, 1 }; w.born = { 1, 2, 3, 4, 5, 6 };
	BatchSlots s; s.cap = 6;
	BodyLinks l; l.resize(6);
	// the capture: slot 0 on body 2, slot 1 on body 0, slot 2 on body 3 and gone already (its body was reborn), slot 3 on body 4
	for (int k = 0; k < 4; ++k) s.take();
	l.attach(0, 2, w.born[2]); l.attach(1, 0, w.born[0]); l.attach(2, 3, w.born[3]); l.attach(3, 4, w.born[4]);
	w.born[3] = 7;
	w.walk(l, s.high);
	CHECK(w.reported.size() == 1 && w.reported[0] == 2 && l.state[2] == BodyLinks::GONE);
	BatchSlots::Snapshot ss; s.snapshot(ss);
	BodyLinks::Snapshot ls; l.snapshot(ls, s.high);
	CHECK(ls.body.size() == 4 && ls.state.size() == 4);
	// afterwards: body 2 is removed and made again (another birth number), body 0 goes for good, slot 3 is removed and body 4 taken over by the new slot 4,
	// slot 5 is taken on body 5: the table has grown
	w.born[2] = 8; w.ok[0] = 0;
	w.walk(l, s.high);
	CHECK(w.reported.size() == 2 && l.state[0] == BodyLinks::GONE && l.state[1] == BodyLinks::GONE);
	l.detach(3); s.give_back(3);
	CHECK(s.take() == 3);
	const uint32_t n4 = s.take(), n5 = s.take();
	CHECK(n4 == 4 && n5 == 5 && s.high == 6);
	l.attach(n4, 4, w.born[4]); l.attach(n5, 5, w.born[5]);
	CHECK(l.slot_of_body.at(4) == 4);
	// the way back, into the grown table
	l.restore(ls, s.high);
	s.restore(ss);
	CHECK(s.high == 4 && s.n_alive == 4);
	CHECK(l.state[4] == BodyLinks::FREE && l.state[5] == BodyLinks::FREE && !l.carried(5));      // slots first used since the capture are free again
	CHECK(l.state[2] == BodyLinks::GONE && l.body[2] == 3 && !l.carried(3));                     // gone at the capture: gone
	CHECK(l.state[0] == BodyLinks::RELINK && l.state[1] == BodyLinks::RELINK && l.state[3] == BodyLinks::RELINK);
	CHECK(l.carried(2) && l.carried(0) && l.carried(4) && l.slot_of_body.at(4) == 3);            // the body another slot took over is the old slot's again
	// the first walk decides: body 2 qualifies -> attached under the birth number it has now; body 0 does not -> gone, reported once; body 4 -> attached
	w.walk(l, s.high);
	CHECK(w.reported.size() == 1 && w.reported[0] == 1);
	CHECK(l.state[0] == BodyLinks::ATTACHED && l.born[0] == 8 && l.slot_of_body.at(2) == 0);
	CHECK(l.state[1] == BodyLinks::GONE && !l.carried(0));
	CHECK(l.state[3] == BodyLinks::ATTACHED && l.born[3] == w.born[4] && l.slot_of_body.at(4) == 3);
	CHECK(l.state[2] == BodyLinks::GONE);
	w.walk(l, s.high); CHECK(w.reported.empty());
	// from here on the slot is like any other: its body reborn again is noticed
	w.born[2] = 9;
	w.walk(l, s.high);
	CHECK(w.reported.size() == 1 && w.reported[0] == 0 && !l.carried(2));
	// restored a second time from the same snapshot, with the bodies as the world's rollback leaves them: everything qualifies
	w.ok[0] = 1;
	l.restore(ls, s.high);
	w.walk(l, s.high);
	CHECK(w.reported.empty() && l.state[0] == BodyLinks::ATTACHED && l.born[0] == 9 && l.state[1] == BodyLinks::ATTACHED && l.state[3] == BodyLinks::ATTACHED && l.state[2] == BodyLinks::GONE);
	// a slot waiting for its walk can be removed: its body is free at once
	l.restore(ls, s.high);
	l.detach(1);
	CHECK(!l.carried(0) && l.state[1] == BodyLinks::FREE);
	// a snapshot taken while slots wait for their walk holds them as attached
	BodyLinks::Snapshot again; l.snapshot(again, s.high);
	l.restore(again, s.high);
	CHECK(l.state[0] == BodyLinks::RELINK && l.state[3] == BodyLinks::RELINK && l.state[1] == BodyLinks::FREE);
	if (g_bad == bad_before) printf("relink rule: ok\n");
}

int main()
{
	slots_snapshot();
	relink_rule();
	if (g_bad) printf("%d checks failed\n", g_bad);
	return g_bad ? 1 : 0;
}
