// saveState / restoreState of the facade's batches (shim/MoverBatch.h, CraftBatch.h, ParticleBatch.h over sgp_<batch>_checkpoint / _rollback, include/sgp.h)
// next to PhysicsWorld::checkpoint / rollback.  A caller with a train and a lift (MoverBatch) and a hover car and a capsized boat that raise particles
// (CraftBatch with a ParticleBatch attached) runs 10 frames and saves everything -- while the carriage, added before its leader, still waits for it in the
// facade's own list --, runs 20 more frames in which the leader arrives (frame 12) and the car's keys change (frame 15), recording what the batches and the
// world report, restores everything and runs the same 20 frames again: the two recordings must be identical, bit for bit.  Without the facade's host state
// in the pair the second run would find the leader's controller already there and the car's keys already changed.
#include "MoverBatch.h"
#include "CraftBatch.h"
#include <utils/Exception.h>
#include <cstdio>
#include <cstring>
#include <cmath>
#include <vector>
#include <algorithm>

typedef std::vector<uint32_t> Recording;

template <class T> static void words(Recording& out, const T* p, size_t n)
{
	const size_t at = out.size(), bytes = sizeof(T) * n;
	out.resize(at + (bytes + 3) / 4, 0u);
	if (bytes) memcpy(out.data() + at, p, bytes);
}

static Reference<PhysicsObject> cube(PhysicsWorld& w, Vec4f pos, Vec3f scale, PhysicsObject::MotionType motion, float mass = 50.f, bool zero_drag = false)
{
	Reference<PhysicsObject> ob = new PhysicsObject(true);
	ob->is_cube = true; ob->scale = scale; ob->pos = pos; ob->motion_type = motion; ob->mass = mass; ob->use_zero_linear_drag = zero_drag;
	return ob;
}

int main()
{
	try {
		PhysicsWorld::init();
		Reference<PhysicsWorld> world = new PhysicsWorld(nullptr, nullptr);
		world->setWaterBuoyancyEnabled(true); world->setWaterZ(0.5f);
		std::vector<Reference<PhysicsObject>> obs;
		obs.push_back(cube(*world, Vec4f(0, -20.f, 0.5f, 1), Vec3f(60.f, 20.f, 1.f), PhysicsObject::MotionType_static));                 // the slab under the car
		obs.push_back(cube(*world, Vec4f(0, 0, 8.f, 1), Vec3f(3.f, 1.5f, 0.4f), PhysicsObject::MotionType_kinematic));                     // 1: the leader
		obs.push_back(cube(*world, Vec4f(-4.f, 0, 8.f, 1), Vec3f(3.f, 1.5f, 0.4f), PhysicsObject::MotionType_kinematic));                  // 2: the carriage
		obs.push_back(cube(*world, Vec4f(20.f, 20.f, 8.f, 1), Vec3f(2.f, 2.f, 0.4f), PhysicsObject::MotionType_kinematic));                // 3: the lift
		obs.push_back(cube(*world, Vec4f(0, -20.f, 3.5f, 1), Vec3f(1.8f, 4.f, 0.8f), PhysicsObject::MotionType_dynamic, 1000.f));          // 4: the hover car
		obs.push_back(cube(*world, Vec4f(10.f, 40.f, 0.6f, 1), Vec3f(2.f, 6.f, 1.f), PhysicsObject::MotionType_dynamic, 2000.f, true));    // 5: the boat, capsized
		obs[5]->rot = Quatf(); obs[5]->rot.v = Vec4f(0, std::sin(1.45f), 0, std::cos(1.45f));
		for (Reference<PhysicsObject>& ob : obs) { world->addObject(ob); if (ob->motion_type != PhysicsObject::MotionType_static) world->activateObject(ob); }

		std::vector<PathWaypointIn> wps;
		const float at[6][3] = { { 0, 0, 8 }, { 10, 0, 8 }, { 14, 4, 8 }, { 14, 12, 8 }, { 0, 14, 8 }, { -6, 6, 8 } };
		const PathWaypointIn::WaypointType types[6] = { PathWaypointIn::Station, PathWaypointIn::CurveIn, PathWaypointIn::CurveOut, PathWaypointIn::CurveOut, PathWaypointIn::Station, PathWaypointIn::CurveOut };
		for (int i = 0; i < 6; ++i) { PathWaypointIn w(Vec4f(at[i][0], at[i][1], at[i][2], 1), types[i]); w.pause_time = i == 0 ? 0.1f : 0.f; w.speed = 6.f + i; wps.push_back(w); }

		MoverBatch movers(world.ptr(), 8, 2);
		const uint32_t carriage = movers.addPathController(*obs[2], 2, wps, 0.0, /*follow_uid=*/1, 4.f, true);      // waits for its leader
		const uint32_t lift = movers.addMoveToController(*obs[3]);
		movers.setPositionTrack(lift, Vec4f(20.f, 20.f, 8.f, 1), Vec4f(20.f, 20.f, 10.f, 1), 0.9f, MoverBatch::MoveTo_EasingSmoothstep, 0.f);
		if (movers.moverOf(carriage) != SGP_INVALID_ID) { printf("the carriage should be waiting for its leader\n"); return 1; }

		CraftBatch crafts(world->physics_system, 4);
		ParticleBatch particles(world->physics_system, 4 * SGP_CRAFT_MAX_EMIT, 256);
		crafts.attachParticles(&particles);
		HoverCarPhysicsSettings hs; hs.hovercar_mass = 1000.f; hs.trace_origin_os = Vec4f(0, 0, -0.408f, 1);
		BoatPhysicsSettings bs; bs.boat_mass = 2000.f;
		bs.script_settings.propellor_point_os = Vec4f(0, -2.8f, -0.3f, 1); bs.script_settings.propellor_sideways_offset = 0.6f; bs.script_settings.thrust_force = 30000.f;
		bs.script_settings.splash_points.push_back(BoatScriptSettings::SplashPoint{ Vec4f(-0.9f, 2.5f, -0.3f, 1), -1.f });
		const uint32_t car = crafts.addHoverCar(obs[4]->jolt_body_id, hs, 100u), boat = crafts.addBoat(obs[5]->jolt_body_id, bs, 103u);
		crafts.userEnteredVehicle(car, 0);
		crafts.startRightingVehicle(boat);

		uint32_t leader = SGP_INVALID_ID;
		const float dt = 1.f / 60.f;
		auto frame = [&](int s, Recording* out) {
			if (s == 12) leader = movers.addPathController(*obs[1], 1, wps, 0.5, MoverBatch::invalid_uid, 0.f, true);
			PlayerPhysicsInput keys;
			keys.W_down = true; keys.right_trigger = 0.2f; keys.D_down = s >= 15;
			if (s % 3 == 0) crafts.setInput(car, keys);      // (kept until set again: between two sets the facade's copy is what counts)
			movers.update(dt);
			crafts.update(dt);
			particles.think(dt);
			world->think(dt);
			if (!out) return;
			const std::vector<sgp_mover_state>& ms = movers.readBack();
			words(*out, ms.data(), ms.size());
			out->push_back(movers.moverOf(carriage)); out->push_back(leader == SGP_INVALID_ID ? SGP_INVALID_ID : movers.moverOf(leader)); out->push_back(movers.numPaths());
			const std::vector<sgp_craft_state>& cs = crafts.readBack();
			words(*out, cs.data(), cs.size());
			particles.readBack();
			out->push_back((uint32_t)particles.live().size()); words(*out, particles.live().data(), particles.live().size());
			out->push_back((uint32_t)particles.events().size()); words(*out, particles.events().data(), particles.events().size());
			out->push_back(particles.eventsDropped());
			std::vector<sgp_body_state> bodies(16);
			sgp_world_read_states(world->world, 0, 16, bodies.data());
			words(*out, bodies.data(), bodies.size());
		};

		Recording first, second;
		for (int s = 0; s < 10; ++s) frame(s, nullptr);
		MoverBatch::SavedState saved_movers; CraftBatch::SavedState saved_crafts; ParticleBatch::SavedState saved_particles;
		movers.saveState(saved_movers); crafts.saveState(saved_crafts); particles.saveState(saved_particles);
		Reference<PhysicsWorldCheckpoint> cp = world->checkpoint();
		const sgp_batch_checkpoint_info mi = saved_movers.lib.info(), ci = saved_crafts.lib.info();
		if (mi.kind != SGP_BATCH_MOVERS || mi.num_alive != 1 || ci.kind != SGP_BATCH_CRAFTS || ci.num_alive != 2) { printf("unexpected checkpoint info\n"); return 1; }
		for (int s = 10; s < 30; ++s) frame(s, &first);
		const uint32_t carriage_mover = movers.moverOf(carriage), leader_handle = leader;
		if (carriage_mover == SGP_INVALID_ID || leader == SGP_INVALID_ID) { printf("the leader should have arrived and the carriage followed\n"); return 1; }

		// back: the batches ahead of the world
		movers.restoreState(saved_movers); crafts.restoreState(saved_crafts); particles.restoreState(saved_particles);
		if (!world->rollback(*cp)) { printf("rollback returned false\n"); return 1; }
		leader = SGP_INVALID_ID;
		const bool waiting = movers.moverOf(carriage) == SGP_INVALID_ID;
		for (int s = 10; s < 30; ++s) frame(s, &second);
		const bool same = first.size() == second.size() && std::equal(first.begin(), first.end(), second.begin());
		size_t diff = 0; while (diff < first.size() && diff < second.size() && first[diff] == second[diff]) ++diff;
		printf("recordings: %zu and %zu words, identical %d (first difference at %zu); carriage waiting again %d, same handles %d\n", first.size(), second.size(), (int)same, diff,
		       (int)waiting, (int)(leader == leader_handle && movers.moverOf(carriage) == carriage_mover));
		if (!same || !waiting || leader != leader_handle || movers.moverOf(carriage) != carriage_mover || first.size() < 20 * 16 * sizeof(sgp_body_state) / 4) return 1;

		// saved into again: the library's checkpoints are overwritten in place
		const sgp_batch_checkpoint* before = saved_movers.lib.cp;
		movers.saveState(saved_movers);
		printf("saved again: in place %d, movers alive %u\n", (int)(saved_movers.lib.cp == before), saved_movers.lib.info().num_alive);
		if (saved_movers.lib.cp != before || saved_movers.lib.info().num_alive != 3) return 1;
		return 0;
	} catch (glare::Exception& e) { fprintf(stderr, "glare::Exception: %s\n", e.what().c_str()); return 2; }
	catch (std::exception& e) { fprintf(stderr, "exception: %s\n", e.what()); return 3; }
}
