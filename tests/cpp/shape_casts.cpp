// Three callers of castShapes.  (1) Placing an object: the convex hull of a new object is lowered onto a settled pile of cubes, the object is put where
// the cast stopped, and it rests there.  (2) A kinematic platform's box is swept sideways up to a wall and stops at it.  (3) The rail: a thin bar at the
// height of a capsule's middle passes between the two end spheres of the capsule (two sphere casts miss it), the capsule's own cast stops at it.
#include "PhysicsWorld.h"
#include <utils/Exception.h>
#include <cmath>
#include <cstdio>
#include <vector>

static Reference<PhysicsObject> addBox(PhysicsWorld& world, const Vec4f& pos, const Vec3f& scale, bool dynamic)
{
	Reference<PhysicsObject> ob = new PhysicsObject(true);
	ob->is_cube = true; ob->scale = scale; ob->mass = 20.f; ob->pos = pos;
	ob->motion_type = dynamic ? PhysicsObject::MotionType_dynamic : PhysicsObject::MotionType_static;
	world.addObject(ob);
	if (dynamic) world.activateObject(ob);
	return ob;
}

int main()
{
	try {
		PhysicsWorld::init();
		Reference<PhysicsWorld> world = new PhysicsWorld(nullptr, nullptr);
		Reference<PhysicsObject> ground = new PhysicsObject(true, PhysicsWorld::createGroundQuadShape(2000.f), nullptr, 0);
		ground->pos = Vec4f(0, 0, -0.5f, 1);
		world->addObject(ground);
		bool ok = true;

		// (1) a pile: two cubes side by side and one across them; then the hull of a new object lowered onto it
		addBox(*world, Vec4f(-0.52f, 0, 0.5f, 1), Vec3f(1.f), true);
		addBox(*world, Vec4f(0.52f, 0, 0.5f, 1), Vec3f(1.f), true);
		Reference<PhysicsObject> top = addBox(*world, Vec4f(0, 0, 1.52f, 1), Vec3f(1.f), true);
		for (int s = 0; s < 180; ++s) world->think(1.0 / 60.0);
		world->readBackActivatedObjectTransforms();
		// an octahedron, one face down (any signed permutation of its axes maps it onto itself: its body frame is its points' frame)
		const float a = 0.5f;
		std::vector<Vec3f> pts = { Vec3f(a, 0, 0), Vec3f(-a, 0, 0), Vec3f(0, a, 0), Vec3f(0, -a, 0), Vec3f(0, 0, a), Vec3f(0, 0, -a) };
		Reference<PhysicsObject> placed = new PhysicsObject(true, PhysicsWorld::createConvexHullShape(pts), nullptr, 0);
		placed->mass = 20.f; placed->motion_type = PhysicsObject::MotionType_dynamic;
		const float inv = 1.f / std::sqrt(2.f);
		placed->rot = Quatf::fromAxisAndAngle(Vec4f(-inv, inv, 0, 0), std::acos(-1.f / std::sqrt(3.f)));      // turns (1, 1, 1) / sqrt 3 onto (0, 0, -1)
		placed->pos = Vec4f(0.05f, -0.03f, 6.f, 1);
		world->addObject(placed);                      // (the first hull of this world: id 1)
		std::vector<PhysicsWorld::ShapeCast> casts(1);
		casts[0].kind = PhysicsWorld::ShapeQuery::Kind_Hull; casts[0].hull_id = 1;
		casts[0].pos = placed->pos; casts[0].rot = placed->rot; casts[0].dir = Vec4f(0, 0, -1, 0); casts[0].max_t = 10.f;
		casts[0].ignore_body_id = placed->jolt_body_id;
		std::vector<PhysicsWorld::ShapeCastResult> res;
		world->castShapes(casts, res);
		const float face_h = a / std::sqrt(3.f);       // distance of a face of the octahedron from its centre
		const float expect_t = 6.f - res[0].hit_pos_ws[2] - face_h;      // (the touched point lies on the top cube's upper face, about 2 m up)
		printf("placing: hit %s at t = %.5f (the top cube's face: %.5f), normal (%.3f %.3f %.3f)\n", res[0].hit_object == top.ptr() ? "the top cube" : "something else",
			res[0].hit_t, expect_t, res[0].hit_normal_ws[0], res[0].hit_normal_ws[1], res[0].hit_normal_ws[2]);
		ok = ok && res.size() == 1 && res[0].hit_object == top.ptr() && std::fabs(res[0].hit_t - expect_t) < 1.0e-3f && std::fabs(res[0].hit_pos_ws[2] - 2.f) < 0.05f && res[0].hit_normal_ws[2] > 0.999f && res[0].penetration == 0.f;
		const Vec4f rest_pos = placed->pos + casts[0].dir * res[0].hit_t;
		world->setNewObToWorldTransform(*placed, rest_pos, placed->rot, Vec4f(0, 0, 0, 0), Vec4f(0, 0, 0, 0));
		world->activateObject(placed);
		for (int s = 0; s < 120; ++s) world->think(1.0 / 60.0);
		world->readBackActivatedObjectTransforms();
		const Vec4f moved = placed->pos - rest_pos;
		printf("placing: after two seconds the object is (%.4f %.4f %.4f) from where the cast put it\n", moved[0], moved[1], moved[2]);
		ok = ok && std::fabs(moved[0]) < 0.03f && std::fabs(moved[1]) < 0.03f && std::fabs(moved[2]) < 0.03f;

		// (2) a platform's box swept along +x up to a wall whose near face is at x = 60
		Reference<PhysicsObject> wall = addBox(*world, Vec4f(60.5f, 0, 2.f, 1), Vec3f(1.f, 8.f, 4.f), false);
		casts.assign(3, PhysicsWorld::ShapeCast());
		casts[0].pos = Vec4f(50.f, 1.f, 1.5f, 1); casts[0].size = Vec3f(2.f, 1.5f, 0.25f); casts[0].dir = Vec4f(1, 0, 0, 0); casts[0].max_t = 20.f;
		casts[1] = casts[0]; casts[1].max_t = 7.9f;                                   // stops short of the wall: nothing
		casts[2] = casts[0]; casts[2].pos = Vec4f(50.f, 1.f, 6.f, 1);                 // passes over the wall
		world->castShapes(casts, res);
		printf("platform: t = %.5f (8 expected)\n", res[0].hit_t);
		ok = ok && res[0].hit_object == wall.ptr() && res[0].hit_t <= 8.f && res[0].hit_t >= 8.f - 2.0e-4f && res[0].hit_normal_ws[0] < -0.999f;
		ok = ok && res[1].hit_object == nullptr && res[2].hit_object == nullptr;

		// (3) the rail, 1 m ahead of a capsule of radius 0.3 and half height 0.65 at the height of its middle
		Reference<PhysicsObject> rail = addBox(*world, Vec4f(100.f, 0, 2.f, 1), Vec3f(4.f, 0.04f, 0.04f), false);
		std::vector<PhysicsWorld::ShapeCast> ends(2);
		for (int e = 0; e < 2; ++e) {
			ends[e].kind = PhysicsWorld::ShapeQuery::Kind_Sphere; ends[e].size = Vec3f(0.3f);
			ends[e].pos = Vec4f(100.f, -1.f, 2.f + (e ? 0.65f : -0.65f), 1); ends[e].dir = Vec4f(0, 1, 0, 0); ends[e].max_t = 3.f; ends[e].collidable_only = true;
		}
		world->castShapes(ends, res);
		ok = ok && res[0].hit_object == nullptr && res[1].hit_object == nullptr;
		casts.assign(1, PhysicsWorld::ShapeCast());
		casts[0].kind = PhysicsWorld::ShapeQuery::Kind_Capsule; casts[0].size = Vec3f(0.3f, 0.65f, 0.f);
		casts[0].pos = Vec4f(100.f, -1.f, 2.f, 1); casts[0].dir = Vec4f(0, 1, 0, 0); casts[0].max_t = 3.f; casts[0].collidable_only = true;
		world->castShapes(casts, res);
		printf("rail: the end spheres pass, the capsule stops at t = %.5f (0.68 expected)\n", res[0].hit_t);
		ok = ok && res[0].hit_object == rail.ptr() && res[0].hit_t <= 0.68f + 2.0e-5f && res[0].hit_t >= 0.68f - 2.0e-4f;

		printf(ok ? "OK\n" : "FAILED\n");
		return ok ? 0 : 1;
	} catch (glare::Exception& e) { fprintf(stderr, "glare::Exception: %s\n", e.what().c_str()); return 2; }
}
