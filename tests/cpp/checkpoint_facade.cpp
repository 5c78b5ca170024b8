// PhysicsWorld::checkpoint / rollback / saveState (extensions of the facade over sgp_world_checkpoint, include/sgp.h): a facade world with a ground, boxes,
// a mesh object and a car thinks 60 times, is captured, thinks 60 more times while every object's pos / rot, its activated_obs membership and the
// listener's contact callbacks are recorded, is rolled back and thinks the same 60 steps again: the two recordings must be identical, bit for bit.
#include "PhysicsWorld.h"
#include "JoltUtils.h"
#include <utils/Exception.h>
#include <Jolt/Jolt.h>
#include <Jolt/Physics/Collision/ObjectLayer.h>
#include <Jolt/Physics/Vehicle/VehicleConstraint.h>
#include <Jolt/Physics/PhysicsSystem.h>
#include <Jolt/Physics/Vehicle/WheeledVehicleController.h>
#include "../../include/sgp.h"
#include <cstdio>
#include <cstring>
#include <cmath>
#include <vector>
#include <algorithm>

struct Listener : public PhysicsWorldEventListener
{
	std::vector<uint32_t> log;      // per callback: kind, the two body ids, the bits of the manifold
	static uint32_t bitsOf(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
	void note(uint32_t kind, const JPH::Body& a, const JPH::Body& b, const JPH::ContactManifold& m)
	{
		log.push_back(kind); log.push_back(a.id.GetIndex()); log.push_back(b.id.GetIndex());
		log.push_back(bitsOf(m.mPenetrationDepth)); log.push_back(bitsOf(m.mWorldSpaceNormal.x)); log.push_back(bitsOf(m.mBaseOffset.z)); log.push_back((uint32_t)m.mRelativeContactPointsOn1.size());
	}
	void contactAdded(const JPH::Body& a, const JPH::Body& b, const JPH::ContactManifold& m) override { note(1, a, b, m); }
	void contactPersisted(const JPH::Body& a, const JPH::Body& b, const JPH::ContactManifold& m) override { note(2, a, b, m); }
};

typedef std::vector<uint32_t> Recording;

static void record(PhysicsWorld& world, const std::vector<Reference<PhysicsObject>>& obs, Listener& listener, Recording& out)
{
	world.readBackActivatedObjectTransforms();
	Lock lock(world.activated_obs_mutex);
	for (const Reference<PhysicsObject>& ob : obs) {
		for (int k = 0; k < 3; ++k) out.push_back(Listener::bitsOf(ob->pos[k]));
		for (int k = 0; k < 4; ++k) out.push_back(Listener::bitsOf(ob->rot.v[k]));
		out.push_back(world.activated_obs.count(ob.ptr()) ? 1u : 0u);
	}
	out.push_back((uint32_t)world.activated_obs.size());
	// (the callbacks of one step arrive in the library's sorted order)
	out.push_back((uint32_t)listener.log.size());
	out.insert(out.end(), listener.log.begin(), listener.log.end());
	listener.log.clear();
}

int main(int argc, char** argv)
{
	const char* blob_path = argc > 1 ? argv[1] : "checkpoint_facade.ckpt";
	try {
		PhysicsWorld::init();
		Reference<PhysicsWorld> world = new PhysicsWorld(nullptr, nullptr);
		Listener listener;
		world->event_listener = &listener;
		std::vector<Reference<PhysicsObject>> obs;
		Reference<PhysicsObject> ground = new PhysicsObject(true, PhysicsWorld::createGroundQuadShape(2000.f), nullptr, 0);
		ground->pos = Vec4f(0, 0, -0.5f, 1);
		world->addObject(ground); obs.push_back(ground);
		for (int i = 0; i < 24; ++i) {
			Reference<PhysicsObject> ob = new PhysicsObject(true);
			if (i % 3 == 0) ob->is_sphere = true; else ob->is_cube = true;
			ob->scale = Vec3f(0.6f + 0.05f * (float)(i % 5)); ob->mass = 20.f; ob->motion_type = PhysicsObject::MotionType_dynamic;
			ob->pos = Vec4f(-6.f + 1.7f * (float)(i % 6), 6.f + 1.9f * (float)(i / 6), 0.6f + 0.9f * (float)(i % 4), 1);
			world->addObject(ob); world->activateObject(ob); obs.push_back(ob);
		}
		{      // a static mesh object: a ramp
			std::vector<Vec3f> v = { Vec3f(-3, 0, 0), Vec3f(3, 0, 0), Vec3f(3, 6, 1.5f), Vec3f(-3, 6, 1.5f), Vec3f(-3, 6, 0), Vec3f(3, 6, 0) };
			std::vector<uint32> t = { 0, 1, 2, 0, 2, 3, 3, 2, 5, 3, 5, 4, 0, 3, 4, 1, 5, 2 };
			Reference<PhysicsObject> ramp = new PhysicsObject(true, PhysicsWorld::createMeshShape(v, t), nullptr, 0);
			ramp->pos = Vec4f(0, 5, 0, 1);
			world->addObject(ramp); obs.push_back(ramp);
		}
		// a car (the CarPhysics set-up of tests/cpp/car_controller.cpp, box chassis)
		Reference<PhysicsObject> car = new PhysicsObject(true);
		car->is_cube = true; car->scale = Vec3f(1.8f, 4.0f, 0.5f); car->pos = Vec4f(0, -4, 0.8f, 1); car->mass = 1200.f; car->restitution = 0.f;
		car->motion_type = PhysicsObject::MotionType_dynamic;
		world->addObject(car); world->activateObject(car); obs.push_back(car);
		const float wheel_radius = 0.42f, wheel_width = 0.16f, sus_min = 0.2f, sus_max = 0.5f;
		JPH::Ref<JPH::VehicleCollisionTester> tester = new JPH::VehicleCollisionTesterCastSphere(1, 0.5f * wheel_width, JPH::Vec3(0, 0, 1));
		JPH::VehicleConstraintSettings vehicle;
		vehicle.mUp = JPH::Vec3(0, 0, 1); vehicle.mForward = JPH::Vec3(0, 1, 0);
		const JPH::Vec3 joint[4] = { JPH::Vec3(-0.8f, 1.3f, -0.25f), JPH::Vec3(0.8f, 1.3f, -0.25f), JPH::Vec3(-0.8f, -1.3f, -0.25f), JPH::Vec3(0.8f, -1.3f, -0.25f) };
		for (int i = 0; i < 4; ++i) {
			JPH::WheelSettingsWV* w = new JPH::WheelSettingsWV;
			w->mPosition = joint[i] + JPH::Vec3(0, 0, sus_min + 0.2f);
			w->mSuspensionDirection = JPH::Vec3(0, 0, -1); w->mSteeringAxis = JPH::Vec3(0, 0, 1); w->mWheelUp = JPH::Vec3(0, 0, 1); w->mWheelForward = JPH::Vec3(0, 1, 0);
			w->mWidth = wheel_width; w->mRadius = wheel_radius; w->mSuspensionMinLength = sus_min; w->mSuspensionMaxLength = sus_max;
			w->mSuspensionSpring.mFrequency = 2.0f; w->mSuspensionSpring.mDamping = 0.5f;
			w->mMaxSteerAngle = (i < 2) ? 0.78525f : 0.0f; w->mMaxBrakeTorque = 1500.f; w->mMaxHandBrakeTorque = (i < 2) ? 0.0f : 4000.f;
			vehicle.mWheels.push_back(w);
		}
		JPH::WheeledVehicleControllerSettings* controller_settings = new JPH::WheeledVehicleControllerSettings;
		vehicle.mController = controller_settings;
		controller_settings->mDifferentials.resize(1);
		controller_settings->mDifferentials[0].mLeftWheel = 0; controller_settings->mDifferentials[0].mRightWheel = 1;
		controller_settings->mEngine.mMaxTorque = 500.f; controller_settings->mEngine.mMaxRPM = 6000.f;
		const JPH::Body chassis_body = world->getJoltBody(*car);
		JPH::Ref<JPH::VehicleConstraint> vehicle_constraint = new JPH::VehicleConstraint(chassis_body, vehicle);
		vehicle_constraint->SetVehicleCollisionTester(tester);
		world->physics_system->AddConstraint(vehicle_constraint);
		world->physics_system->AddStepListener(vehicle_constraint.GetPtr());
		JPH::BodyInterface& body_interface = world->physics_system->GetBodyInterface();
		JPH::WheeledVehicleController* controller = static_cast<JPH::WheeledVehicleController*>(vehicle_constraint->GetController());

		auto think = [&](int s) {
			body_interface.ActivateBody(car->jolt_body_id);
			controller->SetDriverInput(1.f, 0.3f * std::sin(0.05f * (float)s), 0.f, 0.f);
			world->think(1.0 / 60.0);
		};
		Recording scratch, first, second;
		// 1. think 60 times
		for (int s = 0; s < 60; ++s) { think(s); record(*world, obs, listener, scratch); }
		// 2. checkpoint
		Reference<PhysicsWorldCheckpoint> cp = world->checkpoint();
		// 3. think 60 times, recording
		for (int s = 60; s < 120; ++s) { think(s); record(*world, obs, listener, first); }
		const Vec4f car_after = car->pos;
		// 4. rollback
		if (!world->rollback(*cp)) { printf("rollback returned false\n"); return 1; }
		{ Lock lock(world->activated_obs_mutex); if (world->newly_activated_obs.size() != 0) { printf("newly_activated_obs not cleared\n"); return 1; } }
		if (car->pos[1] == car_after[1]) { printf("the car's cached position was not rewritten by rollback\n"); return 1; }
		// 5. the same 60 steps again
		for (int s = 60; s < 120; ++s) { think(s); record(*world, obs, listener, second); }
		const bool same = first.size() == second.size() && std::equal(first.begin(), first.end(), second.begin());
		size_t diff = 0; while (diff < first.size() && diff < second.size() && first[diff] == second[diff]) ++diff;
		printf("recordings: %zu and %zu words, identical %d (first difference at %zu); car y %.3f\n", first.size(), second.size(), (int)same, diff, car->pos[1]);
		if (!same || first.size() < 60 * 8 * obs.size()) return 1;

		// after an addObject, rollback to the old checkpoint returns false and changes nothing
		Reference<PhysicsObject> extra = new PhysicsObject(true);
		extra->is_cube = true; extra->scale = Vec3f(0.5f); extra->mass = 5.f; extra->motion_type = PhysicsObject::MotionType_dynamic; extra->pos = Vec4f(20, 20, 3, 1);
		world->addObject(extra); world->activateObject(extra);
		const Vec4f car_before = car->pos;
		std::vector<sgp_body_state> before(64), after(64);
		sgp_world_read_states(world->world, 0, 64, before.data());
		const bool refused = !world->rollback(*cp);
		sgp_world_read_states(world->world, 0, 64, after.data());
		const bool untouched = memcmp(before.data(), after.data(), sizeof(sgp_body_state) * 64) == 0 && car->pos[1] == car_before[1];
		printf("rollback after addObject: refused %d, world untouched %d\n", (int)refused, (int)untouched);
		if (!refused || !untouched) return 1;

		// saveState writes a blob sgp_checkpoint_blob_info accepts, with the object count the facade reports
		if (!world->saveState(blob_path)) { printf("saveState failed\n"); return 1; }
		FILE* f = fopen(blob_path, "rb");
		if (!f) return 1;
		fseek(f, 0, SEEK_END); const long n = ftell(f); fseek(f, 0, SEEK_SET);
		std::vector<unsigned char> blob((size_t)n);
		const bool read_ok = fread(blob.data(), 1, (size_t)n, f) == (size_t)n;
		fclose(f); remove(blob_path);
		sgp_checkpoint_info info; memset(&info, 0, sizeof(info));
		const int rc = sgp_checkpoint_blob_info(blob.data(), (uint64_t)n, &info);
		// (a mesh object is one body of three slots: its two alias slots are counted as bodies by the world)
		sgp_step_stats st; sgp_world_stats(world->world, &st);
		printf("saveState: %ld bytes, blob_info rc %d, bodies %u (world %u), objects %zu, vehicles %u\n", n, rc, info.num_bodies, st.num_bodies, world->getNumObjects(), info.num_vehicles);
		if (!read_ok || rc != SGP_OK || info.num_bodies != st.num_bodies || info.blob_bytes != (uint64_t)n || info.num_vehicles != 1 || info.num_meshes != 1) return 1;
		if (world->getNumObjects() != obs.size() + 1) return 1;
		world->physics_system->RemoveConstraint(vehicle_constraint);
		world->physics_system->RemoveStepListener(vehicle_constraint.GetPtr());
		return 0;
	} catch (glare::Exception& e) { fprintf(stderr, "glare::Exception: %s\n", e.what().c_str()); return 2; }
}
