// A server-shaped caller of the DRIVEN character batch (sgp_characters_set_drive / _jump / _update_at, include/sgp.h): a scene set up through the facade is walked
// by N JPH::CharacterVirtual objects of Jolt/JoltCharacterLite.h, one after the other, each moved by PlayerPhysics::update's velocity rule written out here in this
// program's own words (gui_client/PlayerPhysics.cpp:256-342, 450-461; tests/cpp/player_controller.cpp has the same loop for one character) -- and then by ONE
// driven batch from the same starting states, which gets what the players ask for and never a state back.  Both records go out as JSON (floats as their bit
// patterns) for tests/test_players_gpu.py to compare.
//   players_batch <scene>              host walk + batch walk
//   players_batch <scene> twice        the batch walk twice, in two worlds built alike
//   players_batch <scene> noread       the batch walk with the states read every frame, and again with no read before the last frame: the final states of both
//   players_batch <scene> smooth       the batch walk alone, every driven character with SGP_DRIVE_SMOOTH_STAIRS
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
static const float JUMP_SPEED = 4.5f, MAX_AIR_SPEED = 8.f, EYE_HEIGHT = 1.67f, JUMP_PERIOD = 0.1f;
static double timeOf(int frame) { return (double)frame * (1.0 / 60.0); }

static uint32_t bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
static void put3(std::string& s, const JPH::Vec3& v) { char b[64]; snprintf(b, sizeof(b), "%u,%u,%u", bits(v.x), bits(v.y), bits(v.z)); s += b; }

enum Kind { DRIVEN, UNDRIVEN, DISABLED };
struct Start { JPH::Vec3 pos; Kind kind = DRIVEN; };
// what the player asks for this frame
struct Wish {
	JPH::Vec3 move = JPH::Vec3(0, 0, 0); float move_up = 0; bool fly = false, gravity = true, free_camera = false;
	bool jump = false;                                    // processJump this frame
	bool kick = false; JPH::Vec3 kick_vel = JPH::Vec3(0, 0, 0);      // SetLinearVelocity before the update (a bounce pad, addToLinearVel)
};
struct Water { bool enabled = false; float z = 0; };
struct Scene {
	Reference<PhysicsWorld> world;
	std::vector<Reference<PhysicsObject>> obs;
	Reference<PhysicsObject> platform;
	std::vector<Start> starts;
	std::function<Wish(int frame, int ch)> wish;
	std::function<Water(int frame)> water;
	std::function<float(int frame)> platform_y;      // where the platform is at the START of frame f
	int frames = 60;
	bool steps = false;          // the world moves: a world step after every update (then the two walks run in worlds of their own)
};

static Reference<PhysicsObject> addBox(Scene& sc, const Vec3f& size, const Vec4f& centre, PhysicsObject::MotionType mt = PhysicsObject::MotionType_static, const Quatf& rot = Quatf::identity())
{
	Reference<PhysicsObject> ob = new PhysicsObject(true);
	ob->is_cube = true; ob->scale = size; ob->pos = centre; ob->rot = rot; ob->mass = 100.f; ob->motion_type = mt;
	sc.world->addObject(ob);
	if (mt != PhysicsObject::MotionType_static) sc.world->activateObject(ob);
	sc.obs.push_back(ob);
	return ob;
}
static void addFloor(Scene& sc) { addBox(sc, Vec3f(40, 40, 1), Vec4f(0, 0, -0.5f, 1)); }
// a 30 degree slope rising towards +x; its surface is at z = 2.615 + 0.577 x
static void addSlope30(Scene& sc) { addBox(sc, Vec3f(8, 4, 0.2f), Vec4f(0, 0, 2.5f, 1), PhysicsObject::MotionType_static, Quatf::fromAxisAndAngle(Vec4f(0, 1, 0, 0), -0.5235988f)); }

// the platform of the `platform` scene: 1 m/s along y, the direction reversed every 30 frames
static float platformY(int frame) { const int k = frame % 60; return DT * (float)(k < 30 ? k : 60 - k); }

static bool buildScene(Scene& sc, const std::string& name)
{
	sc.world = new PhysicsWorld(nullptr, nullptr);
	sc.water = [](int) { return Water(); };
	if (name == "walk_jump") {
		// three fall 1 m (the first update that STARTS supported is the 28th or so), walk from frame 40, jump while walking at frame 95, land.  Character 0 presses jump
		// at frame 24 (0.05 s before it lands: fires on landing), character 1 at frame 15 (0.2 s before: does not fire), character 2 not at all.
		addFloor(sc); sc.frames = 160;
		sc.starts = { { JPH::Vec3(0, 0, 1.0f) }, { JPH::Vec3(0, 3, 1.0f) }, { JPH::Vec3(0, -3, 1.0f) } };
		sc.wish = [](int f, int ch) { Wish w; if (f >= 40) w.move = JPH::Vec3(3, 0.5f * (float)ch, 0); w.jump = (f == 95) || (ch == 0 && f == 24) || (ch == 1 && f == 15); return w; };
	} else if (name == "platform") {
		addFloor(sc); sc.platform = addBox(sc, Vec3f(3, 3, 0.4f), Vec4f(0, 0, 0.2f, 1), PhysicsObject::MotionType_kinematic);
		sc.starts = { { JPH::Vec3(0, 0, 0.45f) } }; sc.steps = true; sc.frames = 100; sc.platform_y = platformY;
		sc.wish = [](int, int) { return Wish(); };
	} else if (name == "uphill_jump") {
		addFloor(sc); addSlope30(sc); sc.frames = 90;
		sc.starts = { { JPH::Vec3(-2.5f, 0, 1.5f) } };
		sc.wish = [](int f, int) { Wish w; if (f >= 25) w.move = JPH::Vec3(4, 0, 0); w.jump = f == 40; return w; };
	} else if (name == "rest_on_slope") {
		addFloor(sc); addSlope30(sc); sc.frames = 100;
		sc.starts = { { JPH::Vec3(-1.0f, 0, 2.3f) } };
		sc.wish = [](int f, int) { Wish w; if (f >= 70) w.move = JPH::Vec3(2, 0, 0); return w; };
	} else if (name == "air") {
		addFloor(sc); sc.frames = 20;
		sc.starts = { { JPH::Vec3(0, 0, 30.0f) } };
		sc.wish = [](int, int) { Wish w; w.move = JPH::Vec3(15, 0, 0); return w; };
	} else if (name == "fall_cap") {
		addFloor(sc); sc.frames = 10;
		sc.starts = { { JPH::Vec3(0, 0, 60.0f) } };
		sc.wish = [](int f, int) { Wish w; w.kick = f == 0; w.kick_vel = JPH::Vec3(0, 0, -120.f); return w; };
	} else if (name == "swim") {
		// water at z = 3 over the floor: dropped in a little above where it floats, settles; dives; swims along; the water is switched off and the wish to go up means nothing
		addFloor(sc); sc.frames = 330;
		sc.starts = { { JPH::Vec3(0, 0, 1.6f) } };
		sc.water = [](int f) { Water w; w.enabled = f < 270; w.z = 3.0f; return w; };
		sc.wish = [](int f, int) { Wish w; if (f >= 150 && f < 210) w.move_up = -1.5f; else if (f >= 210 && f < 270) w.move = JPH::Vec3(1, 0, 0); else if (f >= 270) w.move_up = 1.5f; return w; };
	} else if (name == "fly") {
		// fly mode on the floor: idle, then a wish along x and a jump while supported (adds jump_speed, keeps the sideways part), accelerate, release: decay
		addFloor(sc); sc.frames = 90;
		sc.starts = { { JPH::Vec3(0, 0, 0) } };
		sc.wish = [](int f, int) { Wish w; w.fly = true; if (f >= 5 && f < 45) w.move = JPH::Vec3(3, 0, 0); w.jump = f == 5; return w; };
	} else if (name == "kick") {
		addFloor(sc); sc.frames = 70;
		sc.starts = { { JPH::Vec3(0, 0, 0) } };
		sc.wish = [](int f, int) { Wish w; w.move = JPH::Vec3(3, 0, 0); w.kick = f == 30; w.kick_vel = JPH::Vec3(0, 5, 3); return w; };
	} else if (name == "step03") {
		// a 0.3 m step across the path: WalkStairs takes it in one update
		addFloor(sc); addBox(sc, Vec3f(2, 4, 0.3f), Vec4f(1.5f, 0, 0.15f, 1)); sc.frames = 45;
		sc.starts = { { JPH::Vec3(-0.3f, 0, 0) } };
		sc.wish = [](int, int) { Wish w; w.move = JPH::Vec3(3, 0, 0); return w; };
	} else if (name == "mixed") {
		// one batch with driven, undriven and disabled characters: 0 driven walks, 1 undriven walks, 2 disabled, 3 driven jumps, 4 undriven walks and stops, 5 driven flies
		addFloor(sc); sc.frames = 60;
		sc.starts = { { JPH::Vec3(0, -5, 0.5f), DRIVEN }, { JPH::Vec3(0, -3, 0.5f), UNDRIVEN }, { JPH::Vec3(0, -1, 0.5f), DISABLED }, { JPH::Vec3(0, 1, 0.5f), DRIVEN },
		              { JPH::Vec3(0, 3, 0.5f), UNDRIVEN }, { JPH::Vec3(0, 5, 0.5f), DRIVEN } };
		sc.wish = [](int f, int ch) {
			Wish w;
			if (ch == 0 || ch == 1) { if (f >= 25) w.move = JPH::Vec3(2.5f, 0.25f, 0); }
			else if (ch == 2) w.move = JPH::Vec3(3, 0, 0);
			else if (ch == 3) w.jump = f == 35;
			else if (ch == 4) { if (f >= 25 && f < 40) w.move = JPH::Vec3(-2, 0, 0); w.jump = f == 30; }
			else { w.fly = true; if (f >= 20) { w.move = JPH::Vec3(1, 1, 0); w.move_up = 2.f; } }
			return w;
		};
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

struct Record { std::string frames, contacts, finals; size_t max_contacts = 0; };
struct Extras { uint32_t on_ground = 0, jumped = 0, num_jumps = 0; JPH::Vec3 cam = JPH::Vec3(0, 0, 0), last_xy = JPH::Vec3(0, 0, 0); float campos_z_delta = 0, fraction = 0; };
static void putRow(std::string& out, int frame, int ch, const JPH::Vec3& p, const JPH::Vec3& v, int gs, uint32_t gbody, const JPH::Vec3& gn, const JPH::Vec3& gv, uint32_t overflow, const Extras& x)
{
	char b[160];
	if (!out.empty()) out += ",";
	snprintf(b, sizeof(b), "[%d,%d,%d,%u,%u,%u,%u,%u,", frame, ch, gs, gbody, overflow, x.on_ground, x.jumped, x.num_jumps); out += b;
	put3(out, p); out += ","; put3(out, v); out += ","; put3(out, gn); out += ","; put3(out, gv); out += ","; put3(out, x.cam); out += ","; put3(out, x.last_xy);
	snprintf(b, sizeof(b), ",%u,%u]", bits(x.campos_z_delta), bits(x.fraction)); out += b;
}
static void putContact(Record& r, int frame, int ch, uint32_t body, uint32_t sub, const JPH::Vec3& p, const JPH::Vec3& n)
{
	char b[96];
	if (!r.contacts.empty()) r.contacts += ",";
	snprintf(b, sizeof(b), "[%d,%d,%u,%u,", frame, ch, body, sub); r.contacts += b;
	put3(r.contacts, p); r.contacts += ","; put3(r.contacts, n); r.contacts += "]";
}
static void worldFrame(Scene& sc, int frame, bool before)
{
	if (before) {
		const Water w = sc.water(frame);
		sc.world->setWaterBuoyancyEnabled(w.enabled); sc.world->setWaterZ(w.z);
		if (!sc.platform.isNull()) sc.world->moveKinematicObject(*sc.platform, Vec4f(0, sc.platform_y(frame + 1), 0.2f, 1), Quatf::identity(), DT);
	} else if (sc.steps) sc.world->think(DT);
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

static float len3(const JPH::Vec3& v) { return std::sqrt((v.x * v.x + v.y * v.y) + v.z * v.z); }

// One player of the host walk: PlayerPhysics' members and its update, in this program's words.
struct HostPlayer {
	std::unique_ptr<JPH::CharacterVirtual> c; Listener listener;
	double last_jump_time = -1; float campos_z_delta = 0; Extras x;
	JPH::Vec3 velocity_set = JPH::Vec3(0, 0, 0);      // what this frame's rule handed to SetLinearVelocity (the undriven characters of the batch get exactly this)

	void update(Scene& sc, const Wish& w, double cur_time, const JPH::CharacterVirtual::ExtendedUpdateSettings& ext)
	{
		PhysicsWorld& pw = *sc.world;
		JPH::CharacterVirtual& ch = *c;
		if (w.jump) last_jump_time = cur_time;                                        // processJump
		if (w.kick) ch.SetLinearVelocity(w.kick_vel);
		const float feet_z = ch.GetPosition().z;
		float wet = 0.f;
		if (pw.getWaterBuoyancyEnabled()) { const float under = pw.getWaterZ() - feet_z; wet = std::fmax(0.f, std::fmin(under / EYE_HEIGHT, 1.f)); }
		JPH::Vec3 wish = w.move;
		if (w.fly || w.free_camera || wet > 0.3f) wish = wish + JPH::Vec3(0.f * w.move_up, 0.f * w.move_up, 1.f * w.move_up);      // processMoveUp
		listener.allow_sliding = !(wish.x == 0.f && wish.y == 0.f && wish.z == 0.f);
		JPH::Vec3 vel = ch.GetLinearVelocity();
		const float vel_z_before = vel.z;
		if (!w.fly) {
			JPH::Vec3 par = wish;
			if (wet < 0.3f) par.z = 0;
			ch.UpdateGroundVelocity();
			if (ch.IsSupported() && (vel.z - ch.GetGroundVelocity().z) < 0.1f) { vel = par; vel = vel + ch.GetGroundVelocity(); }
			else {
				if (len3(par) > MAX_AIR_SPEED) par = par * (MAX_AIR_SPEED / len3(par));
				vel = vel + par * DT;
			}
			if (w.gravity) {
				vel = vel + JPH::Vec3(0, 0, -9.81f) * DT;
				vel = vel + JPH::Vec3(0, 0, 9.81f * 1.1f * wet) * DT;
				const float drag = 2.0f * wet * DT;
				vel = vel * (1.f - (0.2f < drag ? 0.2f : drag));
			}
			if (vel.z < -100) vel.z = -100;
		} else {
			const float speed = len3(vel), wl = len3(wish);
			const JPH::Vec3 desired = (wl < 1.e-4f) ? JPH::Vec3(0, 0, 0) : JPH::Vec3(wish.x / wl, wish.y / wl, wish.z / wl) * speed;
			const JPH::Vec3 accel = wish * 3.f + (desired - vel) * 2.f;
			vel = vel + accel * DT;
		}
		campos_z_delta = campos_z_delta - 20.f * DT * campos_z_delta;
		if (std::fabs(campos_z_delta) < 1.0e-5f) campos_z_delta = 0;
		x.on_ground = (ch.IsSupported() && (vel_z_before - ch.GetGroundVelocity().z) < 0.1f) ? 1u : 0u;
		x.jumped = 0;
		if ((cur_time - last_jump_time) < (double)JUMP_PERIOD && ch.IsSupported()) {
			x.on_ground = 0;
			const JPH::Vec3 gn = ch.GetGroundNormal();
			if (w.fly) vel = vel + JPH::Vec3(0, 0, JUMP_SPEED);
			else {
				const float along = (wish.x * gn.x + wish.y * gn.y) + wish.z * gn.z;
				vel = ((wish - gn * along) + ch.GetGroundVelocity()) + JPH::Vec3(0, 0, JUMP_SPEED);
			}
			last_jump_time = -1; x.jumped = 1; x.num_jumps++;
		}
		x.fraction = wet;
		velocity_set = vel;
		ch.SetLinearVelocity(vel);
		ch.ExtendedUpdate(DT, pw.physics_system->GetGravity(), ext, pw.physics_system->GetDefaultBroadPhaseLayerFilter(1), pw.physics_system->GetDefaultLayerFilter(1), JPH::BodyFilter(), JPH::ShapeFilter(), ta);
		// (the reference reads pre_stair_walk_position after ExtendedUpdate: dz = 0)
		const float dz = ch.GetPosition().z - ch.GetPosition().z;
		const float sum = campos_z_delta + dz;
		campos_z_delta = std::fmax(-0.3f, std::fmin(sum, 0.3f));
		x.last_xy = ch.IsSupported() ? ch.GetLinearVelocity() - ch.GetGroundVelocity() : ch.GetLinearVelocity();
		x.last_xy.z = 0;
		const JPH::Vec3 p = ch.GetPosition();
		x.cam = JPH::Vec3(p.x, p.y, p.z + EYE_HEIGHT - campos_z_delta);
		x.campos_z_delta = campos_z_delta;
	}
	JPH::TempAllocator ta;
};

struct HostTrace { std::vector<std::vector<JPH::Vec3>> velocity_set; std::vector<std::vector<uint8_t>> no_slide; };      // [frame][character]

static void hostWalk(Scene& sc, Record& rec, HostTrace& trace)
{
	JPH::CharRef<JPH::CharacterVirtualSettings> settings = makeSettings();
	const JPH::CharacterVirtual::ExtendedUpdateSettings ext = makeExt();
	const size_t n = sc.starts.size();
	std::vector<HostPlayer> players(n);
	for (size_t i = 0; i < n; ++i) {
		players[i].c.reset(new JPH::CharacterVirtual(settings, sc.starts[i].pos, JPH::Quat(), sc.world->physics_system));
		players[i].listener.rec = &rec; players[i].listener.ch = (int)i; players[i].c->SetListener(&players[i].listener);
	}
	trace.velocity_set.assign(sc.frames, std::vector<JPH::Vec3>(n, JPH::Vec3(0, 0, 0))); trace.no_slide.assign(sc.frames, std::vector<uint8_t>(n, 0));
	for (int f = 0; f < sc.frames; ++f) {
		worldFrame(sc, f, true);
		for (size_t i = 0; i < n; ++i) {
			if (sc.starts[i].kind == DISABLED) continue;
			players[i].listener.frame = f;
			players[i].update(sc, sc.wish(f, (int)i), timeOf(f), ext);
			trace.velocity_set[f][i] = players[i].velocity_set; trace.no_slide[f][i] = players[i].listener.allow_sliding ? 0 : 1;
			rec.max_contacts = std::max(rec.max_contacts, players[i].c->GetActiveContacts().size());
		}
		worldFrame(sc, f, false);
		for (size_t i = 0; i < n; ++i) {
			const JPH::CharacterVirtual& c = *players[i].c;
			putRow(rec.frames, f, (int)i, c.GetPosition(), c.GetLinearVelocity(), (int)c.GetGroundState(), c.GetGroundBodyID().IsInvalid() ? SGP_INVALID_ID : c.GetGroundBodyID().GetIndex(), c.GetGroundNormal(),
			       c.GetGroundVelocity(), 0u, sc.starts[i].kind == DRIVEN ? players[i].x : Extras());
		}
	}
}

static void check(int rc, const char* what) { if (rc != SGP_OK) throw std::runtime_error(std::string(what) + ": " + sgp_last_error()); }

// ONE batch: the driven characters get their wishes (set_drive, jump) and the clock; the undriven ones the velocities the host walk computed.  read_every: the states
// are fetched after every update (for the record); otherwise nothing is read before the last frame.
static void batchWalk(Scene& sc, Record& rec, const HostTrace* trace, bool read_every, bool smooth)
{
	JPH::CharRef<JPH::CharacterVirtualSettings> settings = makeSettings();
	const sgp_character_desc desc = CharacterBatch::makeDesc(*settings.GetPtr(), makeExt());
	const uint32_t n = (uint32_t)sc.starts.size();
	sgp_characters* cs = nullptr;
	check(sgp_characters_create(sc.world->world, n, &cs), "sgp_characters_create");
	std::vector<sgp_character_input> in(n); std::vector<sgp_character_drive> drive(n), sent(n);
	for (uint32_t i = 0; i < n; ++i) {
		uint32_t id = 0; const float p[3] = { sc.starts[i].pos.x, sc.starts[i].pos.y, sc.starts[i].pos.z };
		check(sgp_character_add(cs, &desc, p, &id), "sgp_character_add");
		if (id != i) throw std::runtime_error("ids are handed out in order");
		in[i].velocity[0] = in[i].velocity[1] = in[i].velocity[2] = 0; in[i].ignore_id = SGP_INVALID_ID; in[i].flags = SGP_CHAR_EXTENDED | (sc.starts[i].kind == DISABLED ? SGP_CHAR_DISABLED : 0u);
		sgp_default_character_drive(&drive[i]); sent[i] = drive[i];
	}
	check(sgp_characters_set_inputs(cs, 0, n, in.data()), "sgp_characters_set_inputs");
	std::vector<sgp_character_state> st(n); std::vector<sgp_character_drive_state> ds(n);
	std::vector<sgp_character_contact> added(n * 32u);
	for (int f = 0; f < sc.frames; ++f) {
		worldFrame(sc, f, true);
		for (uint32_t i = 0; i < n; ++i) {
			const Wish w = sc.wish(f, (int)i);
			if (sc.starts[i].kind == UNDRIVEN) {
				// as CharacterBatch's callers do today: the velocity from the host (here: the host walk's), the no-slide flag with it
				const JPH::Vec3 v = trace->velocity_set[f][i];
				in[i].velocity[0] = v.x; in[i].velocity[1] = v.y; in[i].velocity[2] = v.z; in[i].flags = SGP_CHAR_EXTENDED | (trace->no_slide[f][i] ? SGP_CHAR_NO_SLIDE : 0u);
				check(sgp_characters_set_inputs(cs, i, 1, &in[i]), "sgp_characters_set_inputs");
				continue;
			}
			sgp_character_drive& d = drive[i];
			d.move_desired_vel[0] = w.move.x; d.move_desired_vel[1] = w.move.y; d.move_desired_vel[2] = w.move.z; d.move_up = w.move_up;
			d.flags = SGP_DRIVE_ON | (w.fly ? SGP_DRIVE_FLY : 0u) | (w.gravity ? SGP_DRIVE_GRAVITY : 0u) | (w.free_camera ? SGP_DRIVE_FREE_CAMERA : 0u) | (smooth ? SGP_DRIVE_SMOOTH_STAIRS : 0u);
			if (memcmp(&d, &sent[i], sizeof(d)) != 0) { check(sgp_characters_set_drive(cs, i, 1, &d), "sgp_characters_set_drive"); sent[i] = d; }      // (only what changed)
			if (w.jump) check(sgp_characters_jump(cs, &i, 1, timeOf(f)), "sgp_characters_jump");
			if (w.kick) { in[i].velocity[0] = w.kick_vel.x; in[i].velocity[1] = w.kick_vel.y; in[i].velocity[2] = w.kick_vel.z; check(sgp_characters_set_inputs(cs, i, 1, &in[i]), "sgp_characters_set_inputs"); }
		}
		check(sgp_characters_update_at(cs, DT, timeOf(f)), "sgp_characters_update_at");
		worldFrame(sc, f, false);
		if (!read_every && f + 1 < sc.frames) continue;
		check(sgp_characters_get_states(cs, 0, n, st.data()), "sgp_characters_get_states");
		check(sgp_characters_get_drive_states(cs, 0, n, ds.data()), "sgp_characters_get_drive_states");
		uint32_t na = 0;
		check(sgp_characters_drain_contacts(cs, added.data(), (uint32_t)added.size(), &na), "sgp_characters_drain_contacts");
		if (read_every) for (uint32_t a = 0; a < std::min<uint32_t>(na, (uint32_t)added.size()); ++a)
			putContact(rec, f, (int)added[a].character, added[a].body, added[a].sub_shape, JPH::Vec3(added[a].point[0], added[a].point[1], added[a].point[2]), JPH::Vec3(added[a].normal[0], added[a].normal[1], added[a].normal[2]));
		for (uint32_t i = 0; i < n; ++i) {
			Extras x;
			x.on_ground = ds[i].on_ground; x.jumped = ds[i].jumped; x.num_jumps = ds[i].num_jumps; x.cam = JPH::Vec3(ds[i].cam_pos[0], ds[i].cam_pos[1], ds[i].cam_pos[2]);
			x.last_xy = JPH::Vec3(ds[i].last_xy_plane_vel_rel_ground[0], ds[i].last_xy_plane_vel_rel_ground[1], ds[i].last_xy_plane_vel_rel_ground[2]);
			x.campos_z_delta = ds[i].campos_z_delta; x.fraction = ds[i].fraction_submerged;
			if (sc.starts[i].kind != DRIVEN) x = Extras();      // (never driven: the library answers zeros, but for the camera at the eye height -- not compared)
			std::string row;
			putRow(row, f, (int)i, JPH::Vec3(st[i].pos[0], st[i].pos[1], st[i].pos[2]), JPH::Vec3(st[i].lin_vel[0], st[i].lin_vel[1], st[i].lin_vel[2]), (int)st[i].ground_state, st[i].ground_body,
			       JPH::Vec3(st[i].ground_normal[0], st[i].ground_normal[1], st[i].ground_normal[2]), JPH::Vec3(st[i].ground_velocity[0], st[i].ground_velocity[1], st[i].ground_velocity[2]), st[i].overflow, x);
			if (read_every) { if (!rec.frames.empty()) rec.frames += ","; rec.frames += row; }
			if (f + 1 == sc.frames) { if (!rec.finals.empty()) rec.finals += ","; rec.finals += row; }
		}
	}
	check(sgp_characters_destroy(cs), "sgp_characters_destroy");
}

static void emit(const char* key, const Record& r, bool last = false)
{
	printf("\"%s\":{\"frames\":[%s],\"contacts\":[%s],\"finals\":[%s],\"max_contacts\":%zu}%s\n", key, r.frames.c_str(), r.contacts.c_str(), r.finals.c_str(), r.max_contacts, last ? "" : ",");
}

int main(int argc, char** argv)
{
	const std::string name = argc > 1 ? argv[1] : "walk_jump", mode = argc > 2 ? argv[2] : "both";
	try {
		PhysicsWorld::init();
		Scene sc;
		if (!buildScene(sc, name)) { fprintf(stderr, "unknown scene %s\n", name.c_str()); return 2; }
		printf("{\"scene\":\"%s\",\n", name.c_str());
		Record host; HostTrace trace;
		if (mode == "both") {
			hostWalk(sc, host, trace);
			Record batch;
			if (sc.steps) { Scene other; buildScene(other, name); batchWalk(other, batch, &trace, true, false); }      // the world moved: the batch walks a world of its own, built and stepped alike
			else batchWalk(sc, batch, &trace, true, false);
			emit("host", host); emit("batch", batch, true);
		} else {
			// batch walks only; a scene with undriven characters still needs the host's velocities
			bool undriven = false; for (const Start& s : sc.starts) undriven = undriven || s.kind == UNDRIVEN;
			if (undriven) { Scene first; buildScene(first, name); hostWalk(first, host, trace); }
			Scene other; buildScene(other, name);
			Record a, b;
			if (mode == "smooth") { batchWalk(sc, a, &trace, true, true); emit("batch", a, true); }
			else if (mode == "twice") { batchWalk(sc, a, &trace, true, false); batchWalk(other, b, &trace, true, false); emit("batch", a); emit("batch2", b, true); }
			else if (mode == "noread") { batchWalk(sc, a, &trace, true, false); batchWalk(other, b, &trace, false, false); emit("batch", a); emit("batch2", b, true); }
			else { fprintf(stderr, "unknown mode %s\n", mode.c_str()); return 2; }
		}
		printf("}\n");
		return 0;
	} catch (glare::Exception& e) { fprintf(stderr, "glare::Exception: %s\n", e.what().c_str()); return 2; }
	catch (std::exception& e) { fprintf(stderr, "exception: %s\n", e.what()); return 2; }
}
