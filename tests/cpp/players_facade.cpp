// Four players at once through shim/PlayerBatch.h, over the route of tests/cpp/player_controller.cpp's parts 1-5 and 9 (fall and land, walk, the 0.3 m step, the wall,
// the jump, swimming), with that file's position checks at the end of each part.  Inside a part nothing is read back: a frame is what the players ask for, update(),
// the world's think(), and zeroMoveDesiredVel() -- the loop of a server that owns many avatars.
#include "PhysicsWorld.h"
#include "PlayerBatch.h"
#include <utils/Exception.h>
#include <cmath>
#include <cstdio>
#include <string>

static const int N = 4;

static Reference<PhysicsObject> addBox(PhysicsWorld& w, const Vec3f& size, const Vec4f& pos)
{
	Reference<PhysicsObject> ob = new PhysicsObject(true);
	ob->is_cube = true; ob->scale = size; ob->pos = pos; ob->rot = Quatf::identity(); ob->mass = 100.f; ob->motion_type = PhysicsObject::MotionType_static;
	w.addObject(ob);
	return ob;
}

#define CHECK(cond) do { if (!(cond)) { printf("FAILED in part %d, player %d: %s  (pos %.3f %.3f %.3f)\n", part, i, #cond, p.x, p.y, p.z); return 1; } } while (0)

int main()
{
	try {
		PhysicsWorld::init();
		Reference<PhysicsWorld> world = new PhysicsWorld(nullptr, nullptr);
		Reference<PhysicsObject> ground = new PhysicsObject(true, PhysicsWorld::createGroundQuadShape(2000.f), nullptr, 0);
		ground->pos = Vec4f(0, 0, -0.5f, 1);
		world->addObject(ground);
		addBox(*world, Vec3f(2, 6, 0.3f), Vec4f(6, 0, 0.15f, 1));                 // a 0.3 m step across the paths (x in [5,7])
		addBox(*world, Vec3f(1, 8, 4), Vec4f(12.5f, 0, 2, 1));                    // a wall at x = 12

		PlayerBatch players(world->physics_system, N);
		const float lane_y[N] = { -1.8f, -0.6f, 0.6f, 1.8f };
		uint32_t id[N];
		for (int i = 0; i < N; ++i) id[i] = players.add(JPH::Vec3(0, lane_y[i], 2.0f));
		const float dt = 1.f / 60.f;
		int step = 0, part = 0;
		// forwards: the factor of processMoveForwards along +x (1 = move_speed = 3 m/s); up: the factor of processMoveUp
		auto frame = [&](float forwards, float up = 0.f, bool jump = false) {
			const double cur_time = (double)step * (1.0 / 60.0);
			for (int i = 0; i < N; ++i) {
				if (forwards != 0.f) players.processMoveForwards(id[i], forwards, false, JPH::Vec3(1, 0, 0));
				if (up != 0.f) players.processMoveUp(id[i], up, false);
				if (jump) players.processJump(id[i], cur_time);
			}
			players.update(dt, cur_time);
			world->think(dt);
			players.zeroMoveDesiredVel();      // (the reference's caller zeroes move_desired_vel itself)
			++step;
		};
		JPH::Vec3 p;
		// 1. fall and land
		part = 1;
		for (int k = 0; k < 90; ++k) frame(0.f);
		players.readBack();
		for (int i = 0; i < N; ++i) {
			p = players.getCapsuleBottomPosition(id[i]);
			CHECK(players.isSupported(id[i]) && std::fabs(p.z) < 0.05f && std::fabs(p.x) < 1e-3f);
			CHECK(players.state(id[i]).ground_state == SGP_GROUND_ON_GROUND && players.state(id[i]).ground_normal[2] > 0.99f && players.onGround(id[i]));
		}
		// 2. walk +x at 3 m/s for a second
		part = 2;
		for (int k = 0; k < 60; ++k) frame(1.f);
		players.readBack();
		for (int i = 0; i < N; ++i) { p = players.getCapsuleBottomPosition(id[i]); CHECK(std::fabs(p.x - 3.0f) < 0.15f && std::fabs(p.z) < 0.05f && std::fabs(p.y - lane_y[i]) < 1e-3f); }
		// 3. on to the 0.3 m step (stairs), across it, and down the other side (stick to floor)
		part = 3;
		for (int k = 0; k < 60; ++k) frame(1.f);
		players.readBack();
		for (int i = 0; i < N; ++i) { p = players.getCapsuleBottomPosition(id[i]); CHECK(p.x > 5.6f && p.x < 6.4f && std::fabs(p.z - 0.3f) < 0.06f && players.isSupported(id[i])); }      // (a second on: on the step)
		for (int k = 0; k < 110; ++k) frame(1.f);
		players.readBack();
		for (int i = 0; i < N; ++i) {
			p = players.getCapsuleBottomPosition(id[i]);
			CHECK(p.x > 7.5f && std::fabs(p.z) < 0.05f && players.isSupported(id[i]));
			const JPH::Vec3 cam = players.camPos(id[i]);
			CHECK(cam.z == p.z + PlayerBatch::EYE_HEIGHT && cam.x == p.x);      // the reference's camera: an eye height above the feet
		}
		// 4. into the wall: stops a radius (+ padding) in front of it
		part = 4;
		for (int k = 0; k < 120; ++k) frame(1.f);
		players.readBack();
		for (int i = 0; i < N; ++i) { p = players.getCapsuleBottomPosition(id[i]); CHECK(std::fabs(p.x - (12.0f - PlayerBatch::SPHERE_RAD)) < 0.06f && std::fabs(p.z) < 0.05f); }
		// 5. jump: leaves the ground, comes back
		part = 5;
		frame(0.f, 0.f, true);
		for (int k = 0; k < 20; ++k) frame(0.f);
		players.readBack();
		for (int i = 0; i < N; ++i) { p = players.getCapsuleBottomPosition(id[i]); CHECK(!players.isSupported(id[i]) && p.z > 0.6f && p.z < 1.3f && players.numJumps(id[i]) == 1 && !players.onGround(id[i])); }
		for (int k = 0; k < 60; ++k) frame(0.f);
		players.readBack();
		for (int i = 0; i < N; ++i) { p = players.getCapsuleBottomPosition(id[i]); CHECK(players.isSupported(id[i]) && std::fabs(p.z) < 0.05f && players.numJumps(id[i]) == 1 && !players.jumped(id[i])); }
		// 9. swimming: the water rises to z = 3 far from everything else
		part = 9;
		world->setWaterBuoyancyEnabled(true); world->setWaterZ(3.0f);
		for (int i = 0; i < N; ++i) players.setCapsuleBottomPosition(id[i], JPH::Vec3(40.f + 2.f * (float)i, 40, 2.6f), JPH::Vec3(0, 0, 0));
		for (int k = 0; k < 600; ++k) frame(0.f);
		const float float_z = 3.0f - PlayerBatch::EYE_HEIGHT / 1.1f;
		players.readBack();
		for (int i = 0; i < N; ++i) { p = players.getCapsuleBottomPosition(id[i]); CHECK(!players.isSupported(id[i]) && std::fabs(p.z - float_z) < 0.05f && std::fabs(players.getLinearVel(id[i]).z) < 0.05f); }
		for (int k = 0; k < 90; ++k) frame(0.f, -0.5f);            // dive: -1.5 m/s wished
		players.readBack();
		float dived_z[N];
		for (int i = 0; i < N; ++i) { p = players.getCapsuleBottomPosition(id[i]); CHECK(p.z < float_z - 0.4f && p.z > 0.05f); dived_z[i] = p.z; }
		for (int k = 0; k < 240; ++k) frame(1.f / 3.f);            // swim along at 1 m/s wished: comes back up while it moves
		players.readBack();
		for (int i = 0; i < N; ++i) { p = players.getCapsuleBottomPosition(id[i]); CHECK(p.z > dived_z[i] + 0.2f && p.x > 41.0f + 2.f * (float)i); }
		world->setWaterBuoyancyEnabled(false);
		for (int k = 0; k < 120; ++k) frame(0.f, 0.5f);            // no water: the wish to go up means nothing, the players fall and stand
		players.readBack();
		for (int i = 0; i < N; ++i) { p = players.getCapsuleBottomPosition(id[i]); CHECK(players.isSupported(id[i]) && std::fabs(p.z) < 0.05f); }
		std::vector<sgp_character_contact> added;
		players.drainContacts(added);
		printf("players: ok (%d frames, %zu contact records pending at the end)\n", step, added.size());
		return 0;
	} catch (glare::Exception& e) { fprintf(stderr, "glare::Exception: %s\n", e.what().c_str()); return 2; }
	catch (std::exception& e) { fprintf(stderr, "exception: %s\n", e.what()); return 2; }
}
