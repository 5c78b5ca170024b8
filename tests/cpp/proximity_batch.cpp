// A caller with scripted objects twice over: a row of static cubes and a kinematic platform are watched through a ProximityBatch (shim/ProximityBatch.h) while
// the camera walks past them and through two overlapping parcels, and next to it the host does what ScriptedObjectProximityChecker::think and the parcel walks
// of GUIClient do -- one object at a time, on bounds it computes itself from the cubes' positions (identity rotations: centre -+ half extent, exact) -- with every
// expression written as docs/CONTRACT.md 4l writes it.  Half way the batch and the world are saved with events still undrained, run on, rolled back and run
// again.  Prints one JSON line: how the two event streams compare.
#include "PhysicsWorld.h"
#include "ProximityBatch.h"
#include <utils/Exception.h>
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <vector>

struct Box3 { float mn[3], mx[3]; };
static bool contains(const Box3& b, const float* q) { return q[0] >= b.mn[0] && q[0] <= b.mx[0] && q[1] >= b.mn[1] && q[1] <= b.mx[1] && q[2] >= b.mn[2] && q[2] <= b.mx[2]; }
static bool nearTo(const Box3& b, const float* p, float radius)
{
	float d[3];
	for (int c = 0; c < 3; ++c) d[c] = p[c] - std::fmin(std::fmax(p[c], b.mn[c]), b.mx[c]);
	const float dist2 = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2];
	return dist2 < radius * radius;
}

struct Ev { int kind; PhysicsObject* object; uint32_t parcel; uint32_t update; };
static bool operator==(const Ev& a, const Ev& b) { return a.kind == b.kind && a.object == b.object && a.parcel == b.parcel && a.update == b.update; }

struct Watched { Reference<PhysicsObject> ob; float half[3]; bool in_proximity = false; };
struct Parcel { uint32_t id; Box3 box; };

// the host's own checker: in_script_proximity per object, cur_in_parcel_id for the camera
struct HostChecker
{
	std::vector<Watched>* objects; std::vector<Parcel> parcels; int cur_parcel = -1; uint32_t updates = 0;
	Box3 boundsOf(PhysicsWorld& w, Watched& o)
	{
		JPH::RVec3 p; JPH::Quat q;
		w.physics_system->GetBodyInterface().GetPositionAndRotation(o.ob->jolt_body_id, p, q);
		const float c[3] = { (float)p.GetX(), (float)p.GetY(), (float)p.GetZ() };
		Box3 b;
		for (int k = 0; k < 3; ++k) { b.mn[k] = c[k] - o.half[k]; b.mx[k] = c[k] + o.half[k]; }
		return b;
	}
	void think(PhysicsWorld& w, const float* campos, std::vector<Ev>& out)
	{
		// the parcel the camera is in: the guess first, then the lowest id
		int now = -1;
		if (cur_parcel >= 0 && contains(parcels[cur_parcel].box, campos)) now = cur_parcel;
		else for (size_t i = 0; i < parcels.size(); ++i) if (contains(parcels[i].box, campos) && (now < 0 || parcels[i].id < parcels[now].id)) now = (int)i;
		const bool changed = now != cur_parcel;
		if (changed && cur_parcel >= 0) out.push_back(Ev{ ProximityBatch::UserExitedParcel, nullptr, parcels[cur_parcel].id, updates });
		if (changed && now >= 0) out.push_back(Ev{ ProximityBatch::UserEnteredParcel, nullptr, parcels[now].id, updates });
		for (Watched& o : *objects) {
			const Box3 b = boundsOf(w, o);
			const bool n = nearTo(b, campos, 20.f);
			if (n != o.in_proximity) { o.in_proximity = n; out.push_back(Ev{ n ? ProximityBatch::UserMovedNearToObject : ProximityBatch::UserMovedAwayFromObject, o.ob.ptr(), SGP_INVALID_ID, updates }); }
			if (changed) {
				const float q[3] = { (b.mn[0] + b.mx[0]) * 0.5f, (b.mn[1] + b.mx[1]) * 0.5f, (b.mn[2] + b.mx[2]) * 0.5f };
				if (cur_parcel >= 0 && contains(parcels[cur_parcel].box, q)) out.push_back(Ev{ ProximityBatch::UserExitedParcel, o.ob.ptr(), parcels[cur_parcel].id, updates });
				if (now >= 0 && contains(parcels[now].box, q)) out.push_back(Ev{ ProximityBatch::UserEnteredParcel, o.ob.ptr(), parcels[now].id, updates });
			}
		}
		cur_parcel = now; ++updates;
	}
};

static Reference<PhysicsObject> cube(PhysicsWorld& w, Vec4f pos, Vec3f scale, PhysicsObject::MotionType motion)
{
	Reference<PhysicsObject> ob = new PhysicsObject(true);
	ob->is_cube = true; ob->scale = scale; ob->pos = pos; ob->motion_type = motion; ob->mass = 50.f;
	w.addObject(ob);
	if (motion != PhysicsObject::MotionType_static) w.activateObject(ob);
	return ob;
}

static void campos(int frame, float* p) { p[0] = -60.f + 1.25f * (float)frame; p[1] = 0.5f * std::sin(0.1f * (float)frame); p[2] = 1.7f; }

int main()
{
	try {
		PhysicsWorld::init();
		Reference<PhysicsWorld> world = new PhysicsWorld(nullptr, nullptr);
		cube(*world, Vec4f(0, 0, -0.5f, 1), Vec3f(400.f, 400.f, 1.f), PhysicsObject::MotionType_static);
		std::vector<Watched> objects;
		for (int i = 0; i < 12; ++i) {
			Watched o; o.ob = cube(*world, Vec4f(-50.f + 9.f * (float)i, (i % 3 - 1) * 6.f, 1.f, 1), Vec3f(2.f, 2.f, 2.f), PhysicsObject::MotionType_static);
			o.half[0] = o.half[1] = o.half[2] = 1.f; objects.push_back(o);
		}
		Watched plat; plat.ob = cube(*world, Vec4f(0.f, 30.f, 2.f, 1), Vec3f(4.f, 4.f, 0.5f), PhysicsObject::MotionType_kinematic);
		plat.half[0] = plat.half[1] = 2.f; plat.half[2] = 0.25f; objects.push_back(plat);

		ProximityBatch batch(world.ptr(), 32, 4, 4096);
		std::vector<PhysicsObject*> ptrs;
		for (Watched& o : objects) ptrs.push_back(o.ob.ptr());
		batch.addObjects(ptrs);
		HostChecker host; host.objects = &objects;
		const Parcel parcels[2] = { { 7u, { { -30.f, -20.f, -1.f }, { 10.f, 20.f, 10.f } } }, { 3u, { { 0.f, -20.f, -1.f }, { 40.f, 20.f, 10.f } } } };
		for (const Parcel& p : parcels) { host.parcels.push_back(p); batch.addParcel(p.id, Vec4f(p.box.mn[0], p.box.mn[1], p.box.mn[2], 1), Vec4f(p.box.mx[0], p.box.mx[1], p.box.mx[2], 1)); }

		const float dt = 1.f / 60.f;
		const int frames = 100, save_at = 45, replay = 20;
		std::vector<Ev> got, want;
		auto frame = [&](int f, std::vector<Ev>& host_out) {
			// the platform slides towards the camera's line, identity rotation
			world->moveKinematicObject(*objects.back().ob, Vec4f(0.f, 30.f - 0.25f * (float)f, 2.f, 1), Quatf::identity(), dt);
			world->think(dt);
			float p[3]; campos(f, p);
			batch.think(Vec4f(p[0], p[1], p[2], 1));
			host.think(*world, p, host_out);
		};
		auto drain = [&](std::vector<Ev>& out) { return batch.drain([&](const ProximityBatch::Event& e) { out.push_back(Ev{ (int)e.kind, e.object, e.parcel_id, e.update_index }); }); };

		uint32_t dropped = 0;
		for (int f = 0; f < save_at; ++f) { frame(f, want); if (f % 7 == 6) dropped += drain(got); }      // (frames 42 .. 44 stay undrained)
		// save with events pending, run on, come back, run again: the same events, drained as one stream
		ProximityBatch::SavedState saved;
		batch.saveState(saved);
		Reference<PhysicsWorldCheckpoint> cp = world->checkpoint();
		const HostChecker host_saved = host; const std::vector<Watched> objects_saved = objects; const size_t want_saved = want.size();
		std::vector<Ev> first_run, second_run, scratch;
		for (int f = save_at; f < save_at + replay; ++f) frame(f, scratch);
		dropped += drain(first_run);
		batch.restoreState(saved);
		if (!world->rollback(*cp)) return 4;
		host = host_saved; objects = objects_saved; host.objects = &objects; want.resize(want_saved);
		for (int f = save_at; f < save_at + replay; ++f) frame(f, want);
		dropped += drain(second_run);
		const bool replay_equal = first_run == second_run && !first_run.empty();
		got.insert(got.end(), second_run.begin(), second_run.end());
		for (int f = save_at + replay; f < frames; ++f) frame(f, want);
		dropped += drain(got);

		size_t mismatches = got.size() > want.size() ? got.size() - want.size() : want.size() - got.size();
		for (size_t i = 0; i < std::min(got.size(), want.size()); ++i) if (!(got[i] == want[i])) ++mismatches;
		int kinds[5] = { 0, 0, 0, 0, 0 };
		for (const Ev& e : got) kinds[e.kind]++;

		// the touch throttle: contacts of one watched object at 0, 0.3 and 0.6 s fire twice; an object that is not watched never fires
		std::vector<sgp_character_contact> contacts(2);
		memset(contacts.data(), 0, sizeof(sgp_character_contact) * 2);
		contacts[0].userdata = (uint64_t)objects[0].ob.ptr(); contacts[1].userdata = 0;
		int touches = 0;
		for (double t : { 0.0, 0.3, 0.6 }) batch.touchEvents(contacts, t, [&](PhysicsObject&, uint32_t) { ++touches; });

		printf("{\"objects\": %u, \"frames\": %d, \"events\": %zu, \"expected\": %zu, \"mismatches\": %zu, \"near\": %d, \"away\": %d, \"exited\": %d, \"entered\": %d, \"replay_equal\": %s, \"replay_events\": %zu, \"dropped\": %u, \"touches\": %d, \"in_proximity_last\": %s}\n",
		       batch.numObjects(), frames, got.size(), want.size(), mismatches, kinds[1], kinds[2], kinds[3], kinds[4], replay_equal ? "true" : "false", first_run.size(), dropped, touches,
		       batch.inProximity(*objects[11].ob) == objects[11].in_proximity ? "true" : "false");
		return 0;
	} catch (glare::Exception& e) { fprintf(stderr, "glare::Exception: %s\n", e.what().c_str()); return 2; }
	catch (std::exception& e) { fprintf(stderr, "exception: %s\n", e.what()); return 3; }
}
