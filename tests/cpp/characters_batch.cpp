// A server-shaped caller of the batched character controller (shim/CharacterBatch.h): a scene set up through the facade is walked by N JPH::CharacterVirtual
// objects of Jolt/JoltCharacterLite.h, one after the other -- with PlayerPhysics' contact listener (PlayerPhysics.cpp:519-545) -- and then by ONE batch from the
// same starting states.  Both records go out as JSON (floats as their bit patterns) for tests/test_characters_gpu.py to compare.
//   characters_batch <scene>            one of the scenes below
//   characters_batch many <mode>        70 characters over the staircase and ramp scene: mode all | reversed | single (each alone in a batch of its own)
#include "PhysicsWorld.h"
#include "CharacterBatch.h"
#include <utils/Exception.h>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <functional>
#include <memory>
#include <string>
#include <vector>

static const float RADIUS = 0.3f, CYL_HEIGHT = 1.3f, DT = 1.f / 60.f;

static uint32_t bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
static void put3(std::string& s, const JPH::Vec3& v) { char b[64]; snprintf(b, sizeof(b), "%u,%u,%u", bits(v.x), bits(v.y), bits(v.z)); s += b; }

struct Start { JPH::Vec3 pos; };
struct Wish { JPH::Vec3 desired; bool no_slide; uint32_t ignore; bool extended = true; };      // extended = false: the plain Update of updateForInVehicle      // what the "player" asks for this frame
struct Scene {
	Reference<PhysicsWorld> world;
	std::vector<Reference<PhysicsObject>> obs;
	Reference<PhysicsObject> platform, box;
	std::vector<Start> starts;
	std::function<Wish(int frame, int ch)> wish;
	int frames = 60;
	bool steps = false;          // the world moves: a world step after every update (then the two walks run in worlds of their own)
};

static Reference<PhysicsObject> addBox(Scene& sc, const Vec3f& size, const Vec4f& centre, PhysicsObject::MotionType mt = PhysicsObject::MotionType_static, float mass = 100.f, const Quatf& rot = Quatf::identity(), bool sensor = false)
{
	Reference<PhysicsObject> ob = new PhysicsObject(true);
	ob->is_cube = true; ob->scale = size; ob->pos = centre; ob->rot = rot; ob->mass = mass; ob->motion_type = mt; ob->is_sensor = sensor;
	sc.world->addObject(ob);
	if (mt != PhysicsObject::MotionType_static) sc.world->activateObject(ob);
	sc.obs.push_back(ob);
	return ob;
}
static void addFloor(Scene& sc) { addBox(sc, Vec3f(40, 40, 1), Vec4f(0, 0, -0.5f, 1)); }
static void addStairsAndRamp(Scene& sc)
{
	addFloor(sc);
	for (int i = 0; i < 3; ++i) addBox(sc, Vec3f(0.6f, 6, 0.2f * (float)(i + 1)), Vec4f(1.1f + 0.6f * (float)i, 0, 0.1f * (float)(i + 1), 1));      // fronts at x = 0.8, 1.4, 2.0; 0.2 m rise each
	addBox(sc, Vec3f(4, 6, 0.2f), Vec4f(0, 8, 1.5f, 1), PhysicsObject::MotionType_static, 100.f, Quatf::fromAxisAndAngle(Vec4f(0, 1, 0, 0), -1.0471976f));   // a 60 degree ramp at y = 8
}

static bool buildScene(Scene& sc, const std::string& name)
{
	sc.world = new PhysicsWorld(nullptr, nullptr);
	const uint32_t none = SGP_INVALID_ID;
	auto walk = [&](const JPH::Vec3& v) { sc.wish = [v, none](int, int) { return Wish{ v, false, none }; }; };
	if (name == "flat") {
		addFloor(sc); sc.starts = { { JPH::Vec3(0, 0, 0.5f) } };
		sc.wish = [none](int f, int) { const bool go = f >= 30 && f < 45; return Wish{ go ? JPH::Vec3(2, 0, 0) : JPH::Vec3(0, 0, 0), !go, none }; };
	} else if (name == "plain") {
		// the plain Update (no stick-to-floor, no stairs): fall, land, walk into a 0.2 m step that only ExtendedUpdate would climb
		addStairsAndRamp(sc); sc.starts = { { JPH::Vec3(0, 0, 0.3f) } };
		sc.wish = [none](int, int) { Wish w{ JPH::Vec3(2.5f, 0, 0), false, none }; w.extended = false; return w; };
	} else if (name == "downslope") {
		// a platform with its top at z = 1, then a 30 degree slope down to the floor, walked at 4 m/s: past the crest the ground falls away 3.8 cm per update, more
		// than counts as touching, and StickToFloor brings the character back down onto the slope
		addFloor(sc); addBox(sc, Vec3f(4, 4, 1), Vec4f(-2, 0, 0.5f, 1));
		addBox(sc, Vec3f(4, 4, 0.2f), Vec4f(1.6820508f, 0, -0.0866025f, 1), PhysicsObject::MotionType_static, 100.f, Quatf::fromAxisAndAngle(Vec4f(0, 1, 0, 0), 0.5235988f));
		sc.starts = { { JPH::Vec3(-1.0f, 0, 1.0f) } }; walk(JPH::Vec3(4, 0, 0));
	} else if (name == "steep_drop") {
		// dropped onto the 60 degree ramp while pushing into it: OnSteepGround, and every update that starts there runs CancelVelocityTowardsSteepSlopes
		addStairsAndRamp(sc); sc.starts = { { JPH::Vec3(-0.3f, 8, 1.5f) } }; walk(JPH::Vec3(3, 0, 0));
	} else if (name == "stairs") {
		addStairsAndRamp(sc); sc.starts = { { JPH::Vec3(0, 0, 0) } }; walk(JPH::Vec3(2.5f, 0, 0));
	} else if (name == "block") {
		addFloor(sc); addBox(sc, Vec3f(1, 6, 0.6f), Vec4f(1.3f, 0, 0.3f, 1)); sc.starts = { { JPH::Vec3(0, 0, 0) } }; walk(JPH::Vec3(2.5f, 0, 0));
	} else if (name == "block10") {
		addFloor(sc); addBox(sc, Vec3f(1, 6, 1.0f), Vec4f(1.3f, 0, 0.5f, 1)); sc.starts = { { JPH::Vec3(0, 0, 0) } }; walk(JPH::Vec3(2.5f, 0, 0));
	} else if (name == "ramp60") {
		addStairsAndRamp(sc); sc.starts = { { JPH::Vec3(-2.2f, 8, 0) } }; walk(JPH::Vec3(3, 0, 0));
	} else if (name == "ramp35_noslide" || name == "ramp35_slide") {
		addFloor(sc);
		addBox(sc, Vec3f(4, 4, 0.2f), Vec4f(0, 0, 1.0f, 1), PhysicsObject::MotionType_static, 100.f, Quatf::fromAxisAndAngle(Vec4f(0, 1, 0, 0), -0.6108652f));
		sc.starts = { { JPH::Vec3(0, 0, 1.3f) } };
		const bool ns = name == "ramp35_noslide";
		sc.wish = [ns, none](int, int) { return Wish{ JPH::Vec3(0, 0, 0), ns, none }; };
	} else if (name == "corner") {
		addFloor(sc); addBox(sc, Vec3f(0.2f, 4, 2), Vec4f(1.1f, 0, 1, 1)); addBox(sc, Vec3f(4, 0.2f, 2), Vec4f(0, 1.2f, 1, 1));
		sc.starts = { { JPH::Vec3(0, 0, 0) } }; walk(JPH::Vec3(2.0f, 1.5f, 0));
	} else if (name == "ledge03" || name == "ledge10") {
		const float h = name == "ledge03" ? 0.3f : 1.0f;
		addFloor(sc); addBox(sc, Vec3f(2, 4, h), Vec4f(0, 0, 0.5f * h, 1));
		sc.starts = { { JPH::Vec3(0.3f, 0, h) } }; walk(JPH::Vec3(2, 0, 0));
	} else if (name == "mesh") {
		std::vector<Vec3f> v = { Vec3f(-4, -4, 0), Vec3f(4, -4, 0), Vec3f(4, 4, 0), Vec3f(-4, 4, 0) };
		std::vector<uint32> t = { 0, 1, 2, 0, 2, 3 };      // the seam is the diagonal x = y
		Reference<PhysicsObject> ob = new PhysicsObject(true, PhysicsWorld::createMeshShape(v, t), nullptr, 0);
		ob->pos = Vec4f(0, 0, 0, 1); sc.world->addObject(ob); sc.obs.push_back(ob);
		sc.starts = { { JPH::Vec3(-1.0f, 0.25f, 0.1f) } }; walk(JPH::Vec3(2.5f, 0.3f, 0));
	} else if (name == "field") {
		const int W = 8; std::vector<float> h((size_t)W * W);
		for (int z = 0; z < W; ++z) for (int x = 0; x < W; ++x) h[(size_t)z * W + x] = 0.15f * std::sin(0.9f * (float)x) + 0.1f * std::cos(0.7f * (float)z);
		Reference<PhysicsObject> ob = new PhysicsObject(true, PhysicsWorld::createJoltHeightFieldShape(W, h, W, 1.0f), nullptr, 0);
		ob->rot = Quatf::fromAxisAndAngle(Vec4f(1, 0, 0, 0), 1.5707963f); ob->pos = Vec4f(-3.5f, -3.5f, 0, 1);
		sc.world->addObject(ob); sc.obs.push_back(ob);
		sc.starts = { { JPH::Vec3(-1.6f, -0.7f, 0.6f) } }; walk(JPH::Vec3(2.0f, 0.7f, 0));
	} else if (name == "platform") {
		addFloor(sc); sc.platform = addBox(sc, Vec3f(3, 3, 0.4f), Vec4f(0, 0, 0.2f, 1), PhysicsObject::MotionType_kinematic);
		sc.starts = { { JPH::Vec3(0, 0, 0.45f) } }; sc.steps = true;
		sc.wish = [none](int, int) { return Wish{ JPH::Vec3(0, 0, 0), true, none }; };
	} else if (name == "sensor") {
		addFloor(sc); addBox(sc, Vec3f(1, 2, 2), Vec4f(1.5f, 0, 1, 1), PhysicsObject::MotionType_static, 100.f, Quatf::identity(), true);
		sc.starts = { { JPH::Vec3(0, 0, 0) } }; walk(JPH::Vec3(3, 0, 0));
	} else if (name == "ignored") {
		addFloor(sc); Reference<PhysicsObject> wall = addBox(sc, Vec3f(0.5f, 2, 2), Vec4f(1.5f, 0, 1, 1));
		const uint32_t ig = wall->jolt_body_id.GetIndex();
		sc.starts = { { JPH::Vec3(0, 0, 0) } };
		sc.wish = [ig](int, int) { return Wish{ JPH::Vec3(3, 0, 0), false, ig }; };
	} else if (name == "push") {
		addFloor(sc); sc.box = addBox(sc, Vec3f(0.6f, 0.6f, 0.6f), Vec4f(1.0f, 0, 0.3f, 1), PhysicsObject::MotionType_dynamic, 10.f);
		sc.starts = { { JPH::Vec3(0, 0, 0) } }; sc.steps = true; sc.frames = 30; walk(JPH::Vec3(1.5f, 0, 0));
	} else if (name == "two_push") {
		addFloor(sc); sc.box = addBox(sc, Vec3f(0.8f, 0.8f, 0.8f), Vec4f(0, 0, 0.4f, 1), PhysicsObject::MotionType_dynamic, 10.f);
		sc.starts = { { JPH::Vec3(-1.0f, 0.1f, 0) }, { JPH::Vec3(1.0f, -0.15f, 0) } }; sc.steps = true; sc.frames = 30;
		sc.wish = [none](int, int ch) { return Wish{ JPH::Vec3(ch ? -1.5f : 1.5f, ch ? 0.2f : 0.0f, 0), false, none }; };
	} else if (name == "many") {
		addStairsAndRamp(sc);
		for (int i = 0; i < 70; ++i) {
			// 40 in front of the stairs, 30 in front of the ramp, a few centimetres apart from row to row so that no two do the same thing
			if (i < 40) sc.starts.push_back({ JPH::Vec3(-0.9f + 0.17f * (float)(i % 8), -2.4f + 1.1f * (float)(i / 8) + 0.013f * (float)i, 0.0f) });
			else sc.starts.push_back({ JPH::Vec3(-3.4f + 0.21f * (float)((i - 40) % 6), 6.0f + 0.9f * (float)((i - 40) / 6) + 0.011f * (float)i, 0.0f) });
		}
		sc.wish = [none](int, int ch) { return Wish{ JPH::Vec3(2.0f + 0.01f * (float)(ch % 7), 0.05f * (float)(ch % 3), 0), false, none }; };
	} else return false;
	return true;
}

static JPH::CharRef<JPH::CharacterVirtualSettings> makeSettings()
{
	JPH::CharRef<JPH::CharacterShape> shape = JPH::RotatedTranslatedShapeSettings(JPH::Vec3(0, 0, 0.5f * CYL_HEIGHT + RADIUS), JPH::Quat(0.7071068f, 0, 0, 0.7071068f),
		new JPH::CapsuleShape(0.5f * CYL_HEIGHT, RADIUS)).Create().Get();
	JPH::CharRef<JPH::CharacterVirtualSettings> s = new JPH::CharacterVirtualSettings();
	s->mShape = shape; s->mUp = JPH::Vec3(0, 0, 1); s->mSupportingVolume = JPH::Plane(JPH::Vec3(0, 0, 1), -RADIUS); s->mMaxStrength = 1000;
	return s;
}
static JPH::CharacterVirtual::ExtendedUpdateSettings makeExt()
{
	JPH::CharacterVirtual::ExtendedUpdateSettings e;
	e.mStickToFloorStepDown = JPH::Vec3(0, 0, -0.5f); e.mWalkStairsStepUp = JPH::Vec3(0, 0, 0.4f);
	return e;
}

// the velocity a PlayerPhysics-style caller sets before the update (PlayerPhysics.cpp:296-330 without flying, jumping and swimming), from the state of its own side
static JPH::Vec3 velocityFor(const Wish& w, const JPH::Vec3& vel, bool supported, const JPH::Vec3& ground_vel)
{
	JPH::Vec3 v = supported ? w.desired + ground_vel : vel;
	return v + JPH::Vec3(0, 0, -9.81f) * DT;
}

struct Record { std::string frames, contacts; size_t max_contacts = 0; };
static void putFrame(Record& r, int frame, int ch, const JPH::Vec3& p, const JPH::Vec3& v, int gs, uint32_t gbody, const JPH::Vec3& gn, const JPH::Vec3& gv, uint32_t overflow)
{
	char b[96];
	if (!r.frames.empty()) r.frames += ",";
	snprintf(b, sizeof(b), "[%d,%d,%d,%u,%u,", frame, ch, gs, gbody, overflow); r.frames += b;
	put3(r.frames, p); r.frames += ","; put3(r.frames, v); r.frames += ","; put3(r.frames, gn); r.frames += ","; put3(r.frames, gv); r.frames += "]";
}
static void putContact(Record& r, int frame, int ch, uint32_t body, uint32_t sub, const JPH::Vec3& p, const JPH::Vec3& n)
{
	char b[96];
	if (!r.contacts.empty()) r.contacts += ",";
	snprintf(b, sizeof(b), "[%d,%d,%u,%u,", frame, ch, body, sub); r.contacts += b;
	put3(r.contacts, p); r.contacts += ","; put3(r.contacts, n); r.contacts += "]";
}
static void putBox(std::string& out, Scene& sc)
{
	if (sc.box.isNull()) { out += "null"; return; }
	sgp_body_state st; uint32_t id = sc.box->jolt_body_id.GetIndex();
	sgp_body_get_state(sc.world->world, &id, 1, &st);
	char b[400]; snprintf(b, sizeof(b), "[%u,%u,%u,%u,%u,%u,%u,%u,%u,%u,%u,%u,%u]", bits(st.pos[0]), bits(st.pos[1]), bits(st.pos[2]), bits(st.rot[0]), bits(st.rot[1]), bits(st.rot[2]), bits(st.rot[3]),
		bits(st.lin_vel[0]), bits(st.lin_vel[1]), bits(st.lin_vel[2]), bits(st.ang_vel[0]), bits(st.ang_vel[1]), bits(st.ang_vel[2]));
	out += b;
}
static void worldFrame(Scene& sc, int frame, bool before)
{
	if (!sc.steps) return;
	if (before) { if (!sc.platform.isNull()) sc.world->moveKinematicObject(*sc.platform, Vec4f(0, 1.0f * DT * (float)(frame + 1), 0.2f, 1), Quatf::identity(), DT); }
	else sc.world->think(DT);
}

// PlayerPhysics' listener (PlayerPhysics.cpp:519-545)
struct Listener : public JPH::CharacterContactListener
{
	Record* rec = nullptr; int frame = 0, ch = 0; bool allow_sliding = true;
	void OnContactAdded(const JPH::CharacterVirtual*, const JPH::BodyID& body, const JPH::SubShapeID& sub, JPH::RVec3Arg p, JPH::Vec3Arg n, JPH::CharacterContactSettings&) override { putContact(*rec, frame, ch, body.GetIndex(), sub.GetValue() == 0xFFFFFFFFu ? 0u : sub.GetValue(), p, n); }
	void OnContactSolve(const JPH::CharacterVirtual* c, const JPH::BodyID&, const JPH::SubShapeID&, JPH::RVec3Arg, JPH::Vec3Arg n, JPH::Vec3Arg contact_velocity, const JPH::PhysicsMaterial*, JPH::Vec3Arg, JPH::Vec3& new_velocity) override
	{
		if (!allow_sliding && contact_velocity.IsNearZero() && !c->IsSlopeTooSteep(n)) new_velocity = JPH::Vec3(0, 0, 0);
	}
};

static void hostWalk(Scene& sc, const std::vector<int>& who, Record& rec)
{
	JPH::CharRef<JPH::CharacterVirtualSettings> settings = makeSettings();
	const JPH::CharacterVirtual::ExtendedUpdateSettings ext = makeExt();
	std::vector<std::unique_ptr<JPH::CharacterVirtual>> chars; std::vector<Listener> listeners(who.size());
	for (size_t i = 0; i < who.size(); ++i) {
		chars.emplace_back(new JPH::CharacterVirtual(settings, sc.starts[who[i]].pos, JPH::Quat(), sc.world->physics_system));
		listeners[i].rec = &rec; listeners[i].ch = who[i]; chars[i]->SetListener(&listeners[i]);
	}
	JPH::TempAllocator ta; const JPH::ShapeFilter sf;
	const JPH::BroadPhaseLayerFilter& bp = sc.world->physics_system->GetDefaultBroadPhaseLayerFilter(1); const JPH::ObjectLayerFilter& ol = sc.world->physics_system->GetDefaultLayerFilter(1);
	for (int f = 0; f < sc.frames; ++f) {
		worldFrame(sc, f, true);
		for (size_t i = 0; i < who.size(); ++i) {
			JPH::CharacterVirtual& c = *chars[i];
			const Wish w = sc.wish(f, who[i]);
			listeners[i].frame = f; listeners[i].allow_sliding = !w.no_slide;
			c.SetLinearVelocity(velocityFor(w, c.GetLinearVelocity(), c.IsSupported(), c.GetGroundVelocity()));
			if (!w.extended) c.Update(DT, sc.world->physics_system->GetGravity(), bp, ol, JPH::BodyFilter(), sf, ta);
			else if (w.ignore != SGP_INVALID_ID) c.ExtendedUpdate(DT, sc.world->physics_system->GetGravity(), ext, bp, ol, JPH::IgnoreSingleBodyFilter(JPH::BodyID(w.ignore)), sf, ta);
			else c.ExtendedUpdate(DT, sc.world->physics_system->GetGravity(), ext, bp, ol, JPH::BodyFilter(), sf, ta);
			rec.max_contacts = std::max(rec.max_contacts, c.GetActiveContacts().size());
		}
		worldFrame(sc, f, false);
		for (size_t i = 0; i < who.size(); ++i) {
			const JPH::CharacterVirtual& c = *chars[i];
			putFrame(rec, f, who[i], c.GetPosition(), c.GetLinearVelocity(), (int)c.GetGroundState(), c.GetGroundBodyID().IsInvalid() ? SGP_INVALID_ID : c.GetGroundBodyID().GetIndex(), c.GetGroundNormal(), c.GetGroundVelocity(), 0u);
		}
	}
}

static void batchWalk(Scene& sc, const std::vector<int>& who, Record& rec)
{
	JPH::CharRef<JPH::CharacterVirtualSettings> settings = makeSettings();
	const JPH::CharacterVirtual::ExtendedUpdateSettings ext = makeExt();
	CharacterBatch batch(sc.world->physics_system, (uint32_t)who.size());
	std::vector<uint32_t> ids(who.size());
	for (size_t i = 0; i < who.size(); ++i) ids[i] = batch.add(*settings.GetPtr(), ext, sc.starts[who[i]].pos);
	std::vector<sgp_character_contact> added;
	for (int f = 0; f < sc.frames; ++f) {
		worldFrame(sc, f, true);
		for (size_t i = 0; i < who.size(); ++i) {
			const Wish w = sc.wish(f, who[i]);
			batch.setAllowSliding(ids[i], !w.no_slide);
			batch.setExtendedUpdate(ids[i], w.extended);
			batch.setIgnoredBody(ids[i], w.ignore == SGP_INVALID_ID ? JPH::BodyID() : JPH::BodyID(w.ignore));
			batch.SetLinearVelocity(ids[i], velocityFor(w, batch.GetLinearVelocity(ids[i]), batch.IsSupported(ids[i]), batch.GetGroundVelocity(ids[i])));
		}
		batch.update(DT);
		worldFrame(sc, f, false);
		batch.readBack();
		batch.drainContacts(added);
		for (const sgp_character_contact& a : added) {
			int ch = -1; for (size_t i = 0; i < who.size(); ++i) if (ids[i] == a.character) ch = who[i];
			putContact(rec, f, ch, a.body, a.sub_shape, JPH::Vec3(a.point[0], a.point[1], a.point[2]), JPH::Vec3(a.normal[0], a.normal[1], a.normal[2]));
		}
		for (size_t i = 0; i < who.size(); ++i) {
			const uint32_t id = ids[i];
			putFrame(rec, f, who[i], batch.GetPosition(id), batch.GetLinearVelocity(id), (int)batch.GetGroundState(id), batch.GetGroundBodyID(id).IsInvalid() ? SGP_INVALID_ID : batch.GetGroundBodyID(id).GetIndex(),
				batch.GetGroundNormal(id), batch.GetGroundVelocity(id), batch.state(id).overflow);
		}
	}
}

static void emit(const char* key, const Record& r, const std::string& box, bool last = false)
{
	printf("\"%s\":{\"frames\":[%s],\"contacts\":[%s],\"max_contacts\":%zu,\"box\":%s}%s\n", key, r.frames.c_str(), r.contacts.c_str(), r.max_contacts, box.c_str(), last ? "" : ",");
}

int main(int argc, char** argv)
{
	const std::string name = argc > 1 ? argv[1] : "flat", mode = argc > 2 ? argv[2] : "all";
	try {
		PhysicsWorld::init();
		Scene sc;
		if (!buildScene(sc, name)) { fprintf(stderr, "unknown scene %s\n", name.c_str()); return 2; }
		std::vector<int> everyone; for (size_t i = 0; i < sc.starts.size(); ++i) everyone.push_back((int)i);
		printf("{\"scene\":\"%s\",\n", name.c_str());
		if (name == "many") {
			// batch runs only: all 70 together, the same added in reverse order, or each alone in a batch of its own
			Record r;
			if (mode == "all") batchWalk(sc, everyone, r);
			else if (mode == "reversed") { std::vector<int> rev(everyone.rbegin(), everyone.rend()); batchWalk(sc, rev, r); }
			else for (int c : everyone) batchWalk(sc, std::vector<int>{ c }, r);
			emit("batch", r, "null", true);
		} else if (name == "two_push") {
			// the batch twice, in two worlds built alike: two characters pushing one box must give the same bits on every run
			Record a, b; std::string box_a, box_b;
			batchWalk(sc, everyone, a); putBox(box_a, sc);
			Scene again; buildScene(again, name);
			batchWalk(again, everyone, b); putBox(box_b, again);
			emit("batch", a, box_a); emit("batch2", b, box_b, true);
		} else {
			Record host, batch; std::string box_h, box_b;
			hostWalk(sc, everyone, host); putBox(box_h, sc);
			if (sc.steps) { Scene other; buildScene(other, name); batchWalk(other, everyone, batch); putBox(box_b, other); }      // the world moved: the batch walks a world of its own, built and stepped alike
			else { batchWalk(sc, everyone, batch); putBox(box_b, sc); }
			emit("host", host, box_h); emit("batch", batch, box_b, true);
		}
		printf("}\n");
		return 0;
	} catch (glare::Exception& e) { fprintf(stderr, "glare::Exception: %s\n", e.what().c_str()); return 2; }
	catch (std::exception& e) { fprintf(stderr, "exception: %s\n", e.what()); return 2; }
}
