// One terrain chunk through createJoltHeightFieldShape (a native height field behind the facade) and the same chunk through createMeshShape
// of its triangulation (the facade's former path), in two worlds: the same objects, steps, rays and walking player give identical transforms,
// hits and positions, and the field's shape is several times smaller.
#include "PhysicsWorld.h"
#include "JoltUtils.h"
#include <utils/Exception.h>
#include <Jolt/Jolt.h>
#include <Jolt/Physics/Character/CharacterVirtual.h>
#include <Jolt/Physics/PhysicsSystem.h>
#include <Jolt/Physics/Collision/Shape/CapsuleShape.h>
#include <Jolt/Physics/Collision/Shape/RotatedTranslatedShape.h>
#include <cstdio>
#include <cmath>
#include <cstring>
#include <vector>

static float terrainHeight(int x, int z) { return 0.9f * std::sin(0.21f * (float)x) * std::cos(0.17f * (float)z) + 0.03f * (float)x - 0.02f * (float)z; }

struct Scene
{
	Reference<PhysicsWorld> world;
	Reference<PhysicsObject> terrain;
	std::vector<Reference<PhysicsObject>> obs;
	size_t terrain_size_B = 0;
};

static void build(Scene& sc, bool field, int W, float quad_w)
{
	sc.world = new PhysicsWorld(nullptr, nullptr);
	std::vector<float> h((size_t)W * W);
	for (int z = 0; z < W; ++z) for (int x = 0; x < W; ++x) h[(size_t)z * W + x] = terrainHeight(x, z);
	PhysicsShape shape;
	if (field) shape = PhysicsWorld::createJoltHeightFieldShape(W, h, W, quad_w);
	else {      // the triangulation the facade used to build (shape space: x, height, z - quad_w (W - 1))
		const float z_offset = -quad_w * (float)(W - 1);
		std::vector<Vec3f> v; std::vector<uint32> t;
		for (int z = 0; z < W; ++z) for (int x = 0; x < W; ++x) v.push_back(Vec3f(quad_w * (float)x, h[(size_t)z * W + x], quad_w * (float)z + z_offset));
		for (int z = 0; z + 1 < W; ++z) for (int x = 0; x + 1 < W; ++x) {
			const uint32 a = (uint32)(z * W + x), b = a + 1, c = a + (uint32)W, d = c + 1;
			t.push_back(a); t.push_back(c); t.push_back(d); t.push_back(a); t.push_back(d); t.push_back(b);
		}
		shape = PhysicsWorld::createMeshShape(v, t);
	}
	sc.terrain_size_B = shape.size_B;
	sc.terrain = new PhysicsObject(true, shape, nullptr, 0);
	sc.terrain->rot = Quatf::fromAxisAndAngle(Vec4f(1, 0, 0, 0), 1.5707963f);      // TerrainSystem.cpp:1742-1749: +90 degrees about x
	sc.terrain->pos = Vec4f(-20.f, -20.f, 0.f, 1);
	sc.world->addObject(sc.terrain);
	for (int i = 0; i < 40; ++i) {
		Reference<PhysicsObject> ob = new PhysicsObject(true);
		if (i % 3 == 0) ob->is_sphere = true; else ob->is_cube = true;
		ob->scale = Vec3f(0.6f + 0.05f * (float)(i % 5)); ob->mass = 20.f; ob->motion_type = PhysicsObject::MotionType_dynamic;
		ob->pos = Vec4f(-15.f + 3.1f * (float)(i % 8), -15.f + 5.3f * (float)(i / 8), 4.f + 0.4f * (float)i, 1);
		sc.world->addObject(ob); sc.world->activateObject(ob); sc.obs.push_back(ob);
	}
}

int main()
{
	try {
		PhysicsWorld::init();
		const int W = 96; const float quad_w = 0.5f;
		Scene F, M;
		build(F, true, W, quad_w); build(M, false, W, quad_w);
		bool ok = true;
		for (int s = 0; s < 300; ++s) { F.world->think(1.0 / 60.0); M.world->think(1.0 / 60.0); }
		F.world->readBackActivatedObjectTransforms(); M.world->readBackActivatedObjectTransforms();
		int same_pos = 0;
		for (size_t i = 0; i < F.obs.size(); ++i) {
			const Vec4f a = F.world->getPosInJolt(F.obs[i]), b = M.world->getPosInJolt(M.obs[i]);
			if (memcmp(&a, &b, sizeof(Vec4f)) == 0) ++same_pos;
			const bool over_terrain = a[0] > -19.f && a[0] < 26.5f && a[1] > -19.f && a[1] < 26.5f;
			if (over_terrain && !(a[2] > -3.f)) { printf("object %d fell through at %.2f %.2f %.2f\n", (int)i, a[0], a[1], a[2]); ok = false; }      // (one may roll off the chunk's edge)
		}
		printf("objects: %d of %d transforms identical\n", same_pos, (int)F.obs.size());
		ok = ok && same_pos == (int)F.obs.size();
		// rays: down onto the terrain and the objects, and slanted
		int hits = 0, same_hits = 0;
		for (int i = 0; i < 400; ++i) {
			const float x = -19.f + 0.093f * (float)i, y = -19.f + 0.0871f * (float)((i * 37) % 400);
			const Vec4f dir = (i % 2) ? Vec4f(0, 0, -1, 0) : normalise(Vec4f(0.3f, -0.2f, -1.f, 0));
			RayTraceResult rf, rm;
			F.world->traceRay(Vec4f(x, y, 15.f, 1), dir, 100.f, JPH::BodyID(), rf);
			M.world->traceRay(Vec4f(x, y, 15.f, 1), dir, 100.f, JPH::BodyID(), rm);
			const bool hf = rf.hit_object != nullptr, hm = rm.hit_object != nullptr;
			if (hf) ++hits;
			const bool same_obj = (!hf && !hm) || (hf && hm && ((rf.hit_object == F.terrain.ptr()) == (rm.hit_object == M.terrain.ptr())));
			if (same_obj && (!hf || (rf.hit_t == rm.hit_t && memcmp(&rf.hit_normal_ws, &rm.hit_normal_ws, sizeof(Vec4f)) == 0 && rf.hit_mat_index == rm.hit_mat_index))) ++same_hits;
		}
		printf("rays: %d hits, %d of 400 answers identical\n", hits, same_hits);
		ok = ok && hits > 300 && same_hits == 400;
		// the player walks across the terrain in both worlds
		float max_d = 0.f;
		{
			struct P : public JPH::CharacterContactListener {} lf, lm;
			JPH::CharRef<JPH::CharacterShape> shape = JPH::RotatedTranslatedShapeSettings(JPH::Vec3(0, 0, 0.65f + 0.3f), JPH::Quat(), new JPH::CapsuleShape(0.65f, 0.3f)).Create().Get();
			JPH::CharRef<JPH::CharacterVirtualSettings> cs = new JPH::CharacterVirtualSettings();
			cs->mShape = shape; cs->mUp = JPH::Vec3(0, 0, 1); cs->mSupportingVolume = JPH::Plane(JPH::Vec3(0, 0, 1), -0.3f); cs->mMaxStrength = 1000;
			JPH::CharacterVirtual pf(cs, JPH::Vec3(-17.f, 3.f, 4.f), JPH::Quat(), F.world->physics_system), pm(cs, JPH::Vec3(-17.f, 3.f, 4.f), JPH::Quat(), M.world->physics_system);
			pf.SetListener(&lf); pm.SetListener(&lm);
			JPH::TempAllocator ta; JPH::CharacterVirtual::ExtendedUpdateSettings ext; ext.mStickToFloorStepDown = JPH::Vec3(0, 0, -0.5f); ext.mWalkStairsStepUp = JPH::Vec3(0, 0, 0.4f);
			for (int s = 0; s < 360; ++s) {
				for (int k = 0; k < 2; ++k) {
					JPH::CharacterVirtual& p = k ? pm : pf; PhysicsWorld* w = k ? M.world.ptr() : F.world.ptr();
					JPH::Vec3 vel = p.GetLinearVelocity();
					if (p.IsSupported()) vel = JPH::Vec3(3, 0.5f, 0) + p.GetGroundVelocity(); else vel = vel + JPH::Vec3(3, 0.5f, 0) * (1.f / 60.f);
					vel = vel + JPH::Vec3(0, 0, -9.81f / 60.f);
					p.SetLinearVelocity(vel);
					p.ExtendedUpdate(1.f / 60.f, w->physics_system->GetGravity(), ext, w->physics_system->GetDefaultBroadPhaseLayerFilter(1), w->physics_system->GetDefaultLayerFilter(1), JPH::BodyFilter(), JPH::ShapeFilter(), ta);
					w->think(1.0 / 60.0);
				}
				const JPH::Vec3 a = pf.GetPosition(), b = pm.GetPosition();
				max_d = std::fmax(max_d, std::fmax(std::fabs(a.x - b.x), std::fmax(std::fabs(a.y - b.y), std::fabs(a.z - b.z))));
			}
			const JPH::Vec3 a = pf.GetPosition();
			printf("player at %.2f %.2f %.2f, max |field - mesh| %.3g, supported %d\n", a.x, a.y, a.z, max_d, (int)pf.IsSupported());
			ok = ok && max_d == 0.f && a.x > -5.f && pf.IsSupported();
		}
		// the shape: samples instead of vertices and triangles
		printf("size_B: field %zu, mesh %zu (%.1fx)\n", F.terrain_size_B, M.terrain_size_B, (double)M.terrain_size_B / (double)F.terrain_size_B);
		ok = ok && F.terrain_size_B * 8 < M.terrain_size_B;
		return ok ? 0 : 1;
	} catch (glare::Exception& e) { fprintf(stderr, "glare::Exception: %s\n", e.what().c_str()); return 2; }
}
