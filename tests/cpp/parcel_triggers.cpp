// A parcel-trigger-shaped caller: "which objects are inside parcel X?" is a box.  A few objects are dropped onto the ground quad, some inside a parcel's
// box and some outside; the world thinks until they rest; getObjectsInBox must then return exactly the inside objects -- and the ground, which the box
// reaches.  A second parcel high above the ground holds nothing; collideShapes answers both parcels and a sphere (an audio radius) in one call.
#include "PhysicsWorld.h"
#include <utils/Exception.h>
#include <algorithm>
#include <cstdio>
#include <set>
#include <vector>

int main()
{
	try {
		PhysicsWorld::init();
		Reference<PhysicsWorld> world = new PhysicsWorld(nullptr, nullptr);
		Reference<PhysicsObject> ground = new PhysicsObject(true, PhysicsWorld::createGroundQuadShape(2000.f), nullptr, 0);
		ground->pos = Vec4f(0, 0, -0.5f, 1);
		world->addObject(ground);
		// the parcel: x, y in [10, 30], z in [-0.1, 6]
		const Vec4f pmin(10.f, 10.f, -0.1f, 1.f), pmax(30.f, 30.f, 6.f, 1.f);
		const float inside_xy[5][2] = { { 12.f, 12.f }, { 20.f, 20.f }, { 28.f, 13.f }, { 15.f, 27.f }, { 20.f, 20.2f } };      // (the last one lands on the second)
		const float outside_xy[4][2] = { { 5.f, 20.f }, { 33.f, 20.f }, { 20.f, 36.f }, { -20.f, -20.f } };
		std::vector<Reference<PhysicsObject>> inside, outside;
		for (int i = 0; i < 9; ++i) {
			Reference<PhysicsObject> ob = new PhysicsObject(true);
			if (i % 2) ob->is_sphere = true; else ob->is_cube = true;
			ob->scale = Vec3f(1.f); ob->mass = 10.f; ob->motion_type = PhysicsObject::MotionType_dynamic;
			const float* xy = i < 5 ? inside_xy[i] : outside_xy[i - 5];
			ob->pos = Vec4f(xy[0], xy[1], i == 4 ? 2.6f : 1.0f, 1);
			world->addObject(ob); world->activateObject(ob);
			(i < 5 ? inside : outside).push_back(ob);
		}
		for (int s = 0; s < 240; ++s) world->think(1.0 / 60.0);

		std::vector<PhysicsObject*> found;
		world->getObjectsInBox(pmin, pmax, 0, found);
		std::set<PhysicsObject*> got(found.begin(), found.end()), want;
		want.insert(ground.ptr());
		for (auto& ob : inside) want.insert(ob.ptr());
		bool ok = got == want && got.size() == found.size();      // exactly the inside objects and the ground, each once
		printf("parcel: %zu objects found, %zu expected\n", found.size(), want.size());
		for (auto& ob : outside) if (got.count(ob.ptr())) { printf("an outside object was reported\n"); ok = false; }

		// moving objects only (Layers::MOVING = 1): the ground is not among them
		world->getObjectsInBox(pmin, pmax, 1u << 1, found);
		ok = ok && found.size() == inside.size() && std::find(found.begin(), found.end(), ground.ptr()) == found.end();

		// an empty parcel above, the parcel itself and an audio radius around the first outside object, in one call
		std::vector<PhysicsWorld::ShapeQuery> qs(3);
		qs[0].pos = Vec4f(20.f, 20.f, 50.f, 1.f); qs[0].size = Vec3f(10.f, 10.f, 5.f);
		qs[1].pos = (pmin + pmax) * 0.5f; qs[1].pos[3] = 1.f; qs[1].size = Vec3f(10.f, 10.f, 3.05f); qs[1].deepest_only = true;
		qs[2].kind = PhysicsWorld::ShapeQuery::Kind_Sphere; qs[2].pos = outside[0]->pos; qs[2].size = Vec3f(3.f); qs[2].deepest_only = true; qs[2].layer_mask = 1u << 1;
		world->readBackActivatedObjectTransforms();
		qs[2].pos = outside[0]->pos;
		std::vector<PhysicsWorld::ShapeContact> cs;
		world->collideShapes(qs, cs);
		size_t per_query[3] = { 0, 0, 0 };
		for (const auto& c : cs) { if (c.query > 2 || !c.hit_object) { ok = false; break; } per_query[c.query]++; if (c.query == 2 && c.hit_object != outside[0].ptr()) ok = false; }
		printf("one call, three volumes: %zu / %zu / %zu contacts\n", per_query[0], per_query[1], per_query[2]);
		ok = ok && per_query[0] == 0 && per_query[1] == want.size() && per_query[2] == 1;
		for (size_t i = 1; i < cs.size(); ++i) if (cs[i].query < cs[i - 1].query) ok = false;

		printf(ok ? "OK\n" : "FAILED\n");
		return ok ? 0 : 1;
	} catch (glare::Exception& e) { fprintf(stderr, "glare::Exception: %s\n", e.what().c_str()); return 2; }
}
