// BatchSlots and BodyLinks (substrata_amd/csrc/sgp_batch_slots.h), the host bookkeeping of the device-resident batches: the order in which slots are reused, the
// high-water mark and the live count; attaching slots to bodies, refusing a carried body, finding the bodies that were reborn or stopped qualifying, and a gone
// slot's detach leaving its successor's entry alone.  Host only; built with -fsanitize=address,undefined by tests/test_batch_slots.py.
#include <cstdint>
#include <cstdio>
#include <vector>
#include "../../substrata_amd/csrc/sgp_batch_slots.h"

static int g_bad = 0;
#define CHECK(cond) do { if (!(cond)) { printf("FAILED line %d: %s\n", __LINE__, #cond); ++g_bad; } } while (0)

// fill, refuse, free in `order`, reuse: the slot freed last comes back first
static void slot_table(uint32_t cap, const std::vector<uint32_t>& order)
{
	const int bad_before = g_bad;
	BatchSlots s; s.cap = cap;
	CHECK(s.empty() && s.high == 0 && s.n_alive == 0);
	for (uint32_t k = 0; k < cap; ++k) { CHECK(s.take() == k); CHECK(s.high == k + 1 && s.n_alive == k + 1 && !s.empty()); }
	CHECK(s.take() == BatchSlots::none);
	CHECK(s.high == cap && s.n_alive == cap);      // (a refusal changes nothing)
	uint32_t alive = cap;
	for (uint32_t id : order) { s.give_back(id); CHECK(s.n_alive == --alive && s.high == cap); }
	CHECK(s.empty() == (alive == 0));
	for (size_t k = order.size(); k-- > 0;) { CHECK(s.take() == order[k]); CHECK(s.n_alive == ++alive && s.high == cap); }
	CHECK(alive == cap && s.take() == BatchSlots::none && s.n_alive == cap && s.high == cap);
	// freed and taken in turns: always the one just freed, never a new slot
	for (uint32_t id : order) { s.give_back(id); CHECK(s.take() == id); CHECK(s.n_alive == cap && s.high == cap); }
	if (g_bad == bad_before) printf("slot table of %u: %zu freed and reused\n", cap, order.size());
}

// a world's bodies as far as the links care: does the body qualify, and under which birth number does it live
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

static void body_links()
{
	const int bad_before = g_bad;
	Bodies w; w.ok = { 1, 1, 1, 1 }; w.born = { 1, 2, 3, 4 };
	BatchSlots s; s.cap = 3;
	BodyLinks l; l.resize(3);
	// two slots on two bodies
	const uint32_t a = s.take(), b = s.take();
	l.attach(a, 2, w.born[2]); l.attach(b, 0, w.born[0]);
	CHECK(l.slot_of_body.at(2) == a && l.slot_of_body.at(0) == b && l.slot_of_body.size() == 2);
	// a second slot on a carried body is refused: carried() is what *_add asks before it takes a slot
	CHECK(l.carried(2) && l.carried(0) && !l.carried(1) && !l.carried(3));
	CHECK(s.n_alive == 2 && s.high == 2);
	w.walk(l, s.high); CHECK(w.reported.empty());      // nothing has changed: nothing is reported
	// body 2 is removed and its slot given to a new body: another birth number
	w.born[2] = 5;
	w.walk(l, s.high);
	CHECK(w.reported.size() == 1 && w.reported[0] == a);
	CHECK(!l.carried(2) && l.carried(0));
	w.walk(l, s.high); CHECK(w.reported.empty());      // ... exactly once
	// the body is free for a new attach, while the gone slot is still out
	const uint32_t c = s.take();
	CHECK(c == 2 && s.n_alive == 3);
	l.attach(c, 2, w.born[2]);
	CHECK(l.carried(2) && l.slot_of_body.at(2) == c);
	// the gone slot's detach leaves the entry of the slot that took the body over
	l.detach(a); s.give_back(a);
	CHECK(l.carried(2) && l.slot_of_body.at(2) == c && s.n_alive == 2);
	w.walk(l, s.high); CHECK(w.reported.empty());
	// a body that stops qualifying is reported like a reborn one
	w.ok[0] = 0;
	w.walk(l, s.high);
	CHECK(w.reported.size() == 1 && w.reported[0] == b);
	CHECK(!l.carried(0) && l.carried(2));
	w.walk(l, s.high); CHECK(w.reported.empty());
	// a live slot's detach erases its own entry; the freed slot comes back first and attaches anew
	l.detach(c); s.give_back(c);
	CHECK(!l.carried(2) && s.n_alive == 1);
	w.ok[0] = 1;
	const uint32_t d = s.take();
	CHECK(d == c);
	l.attach(d, 0, w.born[0]);      // (body 0 qualifies again: free since slot b was marked)
	CHECK(l.slot_of_body.at(0) == d);
	l.detach(b); s.give_back(b);    // the gone slot b lets go of body 0, which slot d holds now
	CHECK(l.carried(0) && l.slot_of_body.at(0) == d);
	w.walk(l, s.high); CHECK(w.reported.empty());
	// a body beyond the world's tables does not qualify
	const uint32_t e = s.take();
	CHECK(e == b);
	l.attach(e, 9, 0u);
	w.walk(l, s.high);
	CHECK(w.reported.size() == 1 && w.reported[0] == e && !l.carried(9));
	// the walk stops at `high`
	BodyLinks m; m.resize(3);
	m.attach(2, 1, 77u);
	w.walk(m, 2); CHECK(w.reported.empty() && m.carried(1));
	w.walk(m, 3); CHECK(w.reported.size() == 1 && w.reported[0] == 2 && !m.carried(1));
	if (g_bad == bad_before) printf("body links: ok\n");
}

int main()
{
	slot_table(1, { 0 });
	slot_table(3, { 1, 0, 2 });
	slot_table(3, { 2, 0 });
	body_links();
	if (g_bad) printf("%d checks failed\n", g_bad);
	return g_bad ? 1 : 0;
}
