// A caller with scripted movers twice over: world A drives a train (a leader and a carriage on a loop with an arc and a station) and a lift through a MoverBatch
// (shim/MoverBatch.h), world B drives the same bodies the way ObjectPathController::update / ObjectMoveToController::update do -- evaluate on the host,
// PhysicsWorld::moveKinematicObject, one controller and one sub-step at a time -- with every expression written as docs/CONTRACT.md 4j writes it (the walk
// itself through sgp_path_prepare / sgp_path_advance, which need no device).  Prints one JSON line: how far the two worlds are apart.
#include "PhysicsWorld.h"
#include "MoverBatch.h"
#include <utils/Exception.h>
#include <cmath>
#include <cstdio>
#include <vector>

struct V { float x, y, z; };
static V operator+(V a, V b) { return V{ a.x + b.x, a.y + b.y, a.z + b.z }; }
static V operator-(V a, V b) { return V{ a.x - b.x, a.y - b.y, a.z - b.z }; }
static V operator*(V a, float s) { return V{ a.x * s, a.y * s, a.z * s }; }
static float dotv(V a, V b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
static V norm(V a) { const float l = std::sqrt(dotv(a, a)); return V{ a.x / l, a.y / l, a.z / l }; }
static float lerpf(float a, float b, float t) { return a * (1.0f - t) + b * t; }
static V lerpv(V a, V b, float t) { return V{ lerpf(a.x, b.x, t), lerpf(a.y, b.y, t), lerpf(a.z, b.z, t) }; }
static float smooth01(float x) { const float s = std::fmax(0.0f, std::fmin((x - 0.0f) / (1.0f - 0.0f), 1.0f)); return (s * s) * (3.0f - 2.0f * s); }

struct HostPath
{
	std::vector<sgp_path_segment> segs;
	V wp(int i) const { const int n = (int)segs.size(); const sgp_path_segment& s = segs[((i % n) + n) % n]; return V{ s.pos[0], s.pos[1], s.pos[2] }; }
	void eval(int idx, float dist, V& pos, V& dir) const
	{
		const sgp_path_segment& w = segs[idx];
		const V entry_pos = wp(idx), exit_pos = wp(idx + 1), entry_dir = norm(entry_pos - wp(idx - 1));
		if (w.type == SGP_WAYPOINT_CURVE_IN) {
			const V ex{ w.exit_segment_unit_dir[0], w.exit_segment_unit_dir[1], w.exit_segment_unit_dir[2] };
			if (dist < w.entry_segment_len) { pos = entry_pos + entry_dir * dist; dir = entry_dir; }
			else if (dist < w.entry_segment_len + w.just_curve_len) {
				const float frac = (dist - w.entry_segment_len) / w.just_curve_len;
				const V orthog = norm(ex - entry_dir * dotv(ex, entry_dir));
				const float angle = frac * w.curve_angle, sn = std::sin(angle), cs = std::cos(angle);
				pos = (entry_pos + entry_dir * w.entry_segment_len) + ((entry_dir * w.curve_r) * sn + (orthog * w.curve_r) * (1.0f - cs));
				dir = entry_dir * cs + orthog * sn;
			}
			else { pos = exit_pos - ex * (w.segment_len - dist); dir = ex; }
			return;
		}
		const float frac = dist / w.segment_len;
		pos = lerpv(entry_pos, exit_pos, frac);
		const V end_dir = norm(exit_pos - entry_pos);
		dir = w.type == SGP_WAYPOINT_CURVE_OUT ? end_dir : lerpv(entry_dir, end_dir, smooth01(frac + 0.5f) * 2.0f - 1.0f);
	}
	void evalBackwards(int idx, float dist, float delta, V& pos, V& dir) const
	{
		for (;;) {
			if (delta < dist) { dist -= delta; break; }
			delta -= dist;
			idx = (idx + (int)segs.size() - 1) % (int)segs.size();
			dist = segs[idx].segment_len;
		}
		eval(idx, dist, pos, dir);
	}
};

static Quatf alongPath(V dir)
{
	const float a = std::atan2(dir.y, dir.x);
	Quatf q; q.v = Vec4f(0, 0, std::sin(0.5f * a), std::cos(0.5f * a));      // track_rot * identity
	return q;
}

struct Scene { Reference<PhysicsWorld> world; Reference<PhysicsObject> leader, carriage, lift, box; };
static Reference<PhysicsObject> cube(PhysicsWorld& w, Vec4f pos, Vec3f scale, PhysicsObject::MotionType motion)
{
	Reference<PhysicsObject> ob = new PhysicsObject(true);
	ob->is_cube = true; ob->scale = scale; ob->pos = pos; ob->motion_type = motion; ob->mass = 50.f;
	w.addObject(ob);
	if (motion != PhysicsObject::MotionType_static) w.activateObject(ob);
	return ob;
}
static Scene makeScene()
{
	Scene sc;
	sc.world = new PhysicsWorld(nullptr, nullptr);
	cube(*sc.world, Vec4f(0, 0, -0.5f, 1), Vec3f(80.f, 80.f, 1.f), PhysicsObject::MotionType_static);
	sc.leader = cube(*sc.world, Vec4f(0, 0, 1.f, 1), Vec3f(3.f, 1.5f, 0.4f), PhysicsObject::MotionType_kinematic);
	sc.carriage = cube(*sc.world, Vec4f(-4.f, 0, 1.f, 1), Vec3f(3.f, 1.5f, 0.4f), PhysicsObject::MotionType_kinematic);
	sc.lift = cube(*sc.world, Vec4f(20.f, 20.f, 1.f, 1), Vec3f(2.f, 2.f, 0.4f), PhysicsObject::MotionType_kinematic);
	sc.box = cube(*sc.world, Vec4f(20.f, 20.f, 1.75f, 1), Vec3f(0.5f, 0.5f, 0.5f), PhysicsObject::MotionType_dynamic);
	return sc;
}

int main()
{
	try {
		PhysicsWorld::init();
		Scene a = makeScene(), b = makeScene();
		std::vector<PathWaypointIn> wps;
		const float at[6][3] = { { 0, 0, 1 }, { 10, 0, 1 }, { 14, 4, 1 }, { 14, 12, 1 }, { 0, 14, 1 }, { -6, 6, 1 } };
		const PathWaypointIn::WaypointType types[6] = { PathWaypointIn::Station, PathWaypointIn::CurveIn, PathWaypointIn::CurveOut, PathWaypointIn::CurveOut, PathWaypointIn::Station, PathWaypointIn::CurveOut };
		for (int i = 0; i < 6; ++i) { PathWaypointIn w(Vec4f(at[i][0], at[i][1], at[i][2], 1), types[i]); w.pause_time = i == 0 ? 0.2f : 0.f; w.speed = 6.f + i; wps.push_back(w); }
		const float follow_dist = 4.f, dt = 1.f / 60.f;
		const Vec4f lift_from(20.f, 20.f, 1.f, 1), lift_to(20.f, 20.f, 2.f, 1);

		MoverBatch batch(a.world.ptr(), 8, 2);
		// the carriage first: it waits for its leader
		const uint32_t hc = batch.addPathController(*a.carriage, 2, wps, 0.0, /*follow_uid=*/1, follow_dist, true);
		const uint32_t hl = batch.addPathController(*a.leader, 1, wps, 0.0, MoverBatch::invalid_uid, 0.f, true);
		const uint32_t hm = batch.addMoveToController(*a.lift);
		batch.setPositionTrack(hm, lift_from, lift_to, 0.9f, MoverBatch::MoveTo_EasingSmoothstep, 0.f);
		if (batch.numPaths() != 1 || batch.moverOf(hl) == SGP_INVALID_ID || batch.moverOf(hc) == SGP_INVALID_ID) return 4;
		const Vec4f drawn = batch.evalSegmentCurvePos(hl, 1, 0.5f);

		// the host's own controllers
		HostPath path; path.segs.resize(wps.size());
		std::vector<sgp_path_waypoint> in(wps.size());
		for (size_t i = 0; i < wps.size(); ++i) { in[i] = sgp_path_waypoint{ { wps[i].pos[0], wps[i].pos[1], wps[i].pos[2] }, (uint32_t)wps[i].waypoint_type, wps[i].pause_time, wps[i].speed }; }
		double total = 0;
		if (sgp_path_prepare(in.data(), (uint32_t)in.size(), path.segs.data(), &total) != SGP_OK) return 5;
		sgp_path_progress prog = { 0u, 0.f, 0.f };
		float lift_elapsed = 0.f; bool lift_active = true;

		const int updates = 90;
		float max_pos = 0.f, max_vel = 0.f, moved = 0.f, lifted = 0.f;
		for (int s = 0; s < updates; ++s) {
			batch.update(dt);
			a.world->think(dt);

			uint32_t status = 0;
			sgp_path_advance(path.segs.data(), (uint32_t)path.segs.size(), &prog, dt, &status);
			V pos, dir;
			path.eval((int)prog.waypoint_index, prog.dist_along_segment, pos, dir);
			b.world->moveKinematicObject(*b.leader, Vec4f(pos.x, pos.y, pos.z, 1), alongPath(dir), dt);
			path.evalBackwards((int)prog.waypoint_index, prog.dist_along_segment, follow_dist, pos, dir);
			b.world->moveKinematicObject(*b.carriage, Vec4f(pos.x, pos.y, pos.z, 1), alongPath(dir), dt);
			if (lift_active) {
				lift_elapsed += dt;
				const float e = smooth01(std::fmax(0.f, std::fmin(lift_elapsed / 0.9f, 1.f)));
				if (lift_elapsed >= 0.9f) lift_active = false;
				b.world->moveKinematicObject(*b.lift, Vec4f(lerpf(lift_from[0], lift_to[0], e), lerpf(lift_from[1], lift_to[1], e), lerpf(lift_from[2], lift_to[2], e), 1), Quatf::identity(), dt);
			}
			b.world->think(dt);

			JPH::BodyInterface& ba = a.world->physics_system->GetBodyInterface(); JPH::BodyInterface& bb = b.world->physics_system->GetBodyInterface();
			PhysicsObject* oa[4] = { a.leader.ptr(), a.carriage.ptr(), a.lift.ptr(), a.box.ptr() }; PhysicsObject* ob[4] = { b.leader.ptr(), b.carriage.ptr(), b.lift.ptr(), b.box.ptr() };
			for (int i = 0; i < 4; ++i) {
				JPH::RVec3 pa, pb; JPH::Quat qa, qb; JPH::Vec3 la, lb, wa, wb;
				ba.GetPositionAndRotation(oa[i]->jolt_body_id, pa, qa); bb.GetPositionAndRotation(ob[i]->jolt_body_id, pb, qb);
				ba.GetLinearAndAngularVelocity(oa[i]->jolt_body_id, la, wa); bb.GetLinearAndAngularVelocity(ob[i]->jolt_body_id, lb, wb);
				max_pos = std::fmax(max_pos, std::fmax(std::fabs(pa.GetX() - pb.GetX()), std::fmax(std::fabs(pa.GetY() - pb.GetY()), std::fabs(pa.GetZ() - pb.GetZ()))));
				max_vel = std::fmax(max_vel, std::fmax(std::fabs(la.GetX() - lb.GetX()), std::fmax(std::fabs(la.GetY() - lb.GetY()), std::fabs(la.GetZ() - lb.GetZ()))));
				max_vel = std::fmax(max_vel, std::fmax(std::fabs(wa.GetX() - wb.GetX()), std::fmax(std::fabs(wa.GetY() - wb.GetY()), std::fabs(wa.GetZ() - wb.GetZ()))));
				if (s == updates - 1 && i == 0) moved = std::fabs(pa.GetX() - at[0][0]) + std::fabs(pa.GetY() - at[0][1]);
				if (s == updates - 1 && i == 3) lifted = pa.GetZ();
			}
		}
		const std::vector<sgp_mover_state>& st = batch.readBack();
		printf("{\"movers\": 3, \"updates\": %d, \"max_pos_diff\": %.9g, \"max_vel_diff\": %.9g, \"moved\": %.9g, \"box_z\": %.9g, \"leader_updates\": %u, \"carriage_status\": %u, \"drawn_x\": %.9g}\n",
		       updates, max_pos, max_vel, moved, lifted, st[batch.moverOf(hl)].update_index, st[batch.moverOf(hc)].status, drawn[0]);
		return 0;
	} catch (glare::Exception& e) { fprintf(stderr, "glare::Exception: %s\n", e.what().c_str()); return 2; }
	catch (std::exception& e) { fprintf(stderr, "exception: %s\n", e.what()); return 3; }
}
