// MoverBatch: ObjectPathController and ObjectMoveToController (gui_client/ObjectPathController.h/.cpp, ObjectMoveToController.h/.cpp) for many objects on the
// device (sgp_movers_*, include/sgp.h).  A controller evaluates its path or its tracks on the host every sub-step and ends in
// PhysicsWorld::moveKinematicObject; with a batch the controllers live on the device and update(dt) enqueues all of them on the world's stream and returns.
// What stays here: byte-identical waypoint lists share one path; a follower added before its leader waits until the leader is there (in place of
// sortPathControllers: the library takes leaders before followers; until then the follower is not moved); evalSegmentCurvePos for drawing, on the host from
// the prepared segments; and a move-to controller on a STATIC body, which stays on PhysicsWorld::setNewObToWorldTransform as the reference has it -- static
// large bodies have host bookkeeping that the device does not see, so this header evaluates those few on the host itself.  A dynamic body under move-to is
// left to the simulation, as in the reference.  Departures: docs/GAPS.md ("Movers").
#pragma once
#include "../../include/sgp.h"
#include "PhysicsWorld.h"
#include "BatchCheckpoint.h"
#include "maths/Quat.h"
#include "maths/Vec4f.h"
#include <algorithm>
#include <cmath>
#include <cstring>
#include <map>
#include <stdexcept>
#include <string>
#include <vector>

struct PathWaypointIn
{
	enum WaypointType { CurveIn, CurveOut, Station };
	PathWaypointIn() : pos(0.f), waypoint_type(Station), pause_time(10.f), speed(10.f) {}
	PathWaypointIn(const Vec4f& pos_, WaypointType waypoint_type_) : pos(pos_), waypoint_type(waypoint_type_), pause_time(10.f), speed(10.f) {}
	Vec4f pos;
	WaypointType waypoint_type;
	float pause_time;
	float speed;      // speed to next waypoint
};

class MoverBatch
{
public:
	static const uint64_t invalid_uid = ~0ull;
	static const uint32_t MoveTo_EasingLinear = SGP_MOVER_EASE_LINEAR, MoveTo_EasingSmoothstep = SGP_MOVER_EASE_SMOOTHSTEP;      // Protocol.h

	MoverBatch(PhysicsWorld* world_, uint32_t capacity, uint32_t path_capacity) : world(world_), batch(nullptr), cap(capacity) { check(sgp_movers_create(world->world, capacity, path_capacity, &batch), "sgp_movers_create"); }
	~MoverBatch() { if (batch) sgp_movers_destroy(batch); }
	MoverBatch(const MoverBatch&) = delete;
	MoverBatch& operator=(const MoverBatch&) = delete;

	// ObjectPathController(controlled_ob, waypoints_in, initial_time, follow_ob_uid, follow_dist, orient_along_path).  uid: the controlled object's, for
	// others to follow.  Returns a handle of this batch.
	uint32_t addPathController(PhysicsObject& object, uint64_t uid, const std::vector<PathWaypointIn>& waypoints, double initial_time, uint64_t follow_uid, float follow_dist, bool orient_along_path)
	{
		if (follow_dist < 0.f) throw std::runtime_error("follow_dist must be >= 0");
		Controller c;
		c.kind = OnDevice; c.object = &object; c.uid = uid; c.follow_uid = follow_uid; c.path = pathFor(waypoints);
		memset(&c.desc, 0, sizeof(c.desc));
		c.desc.kind = SGP_MOVER_PATH; c.desc.body = object.jolt_body_id.GetIndex(); c.desc.flags = orient_along_path ? SGP_MOVER_ORIENT_ALONG_PATH : 0u; c.desc.path = c.path;
		c.desc.initial_time = initial_time; c.desc.tag = (uint64_t)&object; c.desc.leader = SGP_INVALID_ID; c.desc.follow_dist = follow_dist;
		for (int k = 0; k < 4; ++k) c.desc.base_rot[k] = object.rot.v[k];
		c.desc.hold_rot[3] = 1.f;
		controllers.push_back(c);
		resolvePending();
		return (uint32_t)controllers.size() - 1u;
	}

	// ObjectMoveToController(controlled_ob)
	uint32_t addMoveToController(PhysicsObject& object)
	{
		Controller c;
		c.object = &object; c.uid = invalid_uid; c.follow_uid = invalid_uid; c.path = SGP_INVALID_ID;
		memset(&c.desc, 0, sizeof(c.desc));
		if (object.isKinematic()) {
			c.kind = OnDevice;
			c.desc.kind = SGP_MOVER_MOVETO; c.desc.body = object.jolt_body_id.GetIndex(); c.desc.leader = SGP_INVALID_ID; c.desc.tag = (uint64_t)&object; c.desc.base_rot[3] = 1.f;
			for (int k = 0; k < 3; ++k) c.desc.hold_pos[k] = object.pos[k];
			for (int k = 0; k < 4; ++k) c.desc.hold_rot[k] = object.rot.v[k];
			check(sgp_mover_add(batch, &c.desc, &c.mover), "sgp_mover_add");
			c.added = true;
		}
		else c.kind = object.isDynamic() ? LeftAlone : OnHost;
		controllers.push_back(c);
		return (uint32_t)controllers.size() - 1u;
	}

	void setPositionTrack(uint32_t handle, const Vec4f& start_pos, const Vec4f& target_pos, float duration, uint32_t easing, float cur_elapsed)
	{
		Controller& c = controllers.at(handle);
		if (c.kind == OnDevice) { check(sgp_movers_set_position_track(batch, c.mover, start_pos.x, target_pos.x, duration, easing, cur_elapsed), "sgp_movers_set_position_track"); return; }
		c.pos.set(start_pos.x, target_pos.x, 3, duration, easing, cur_elapsed);
	}
	void setRotationTrack(uint32_t handle, const Quatf& start_rot, const Quatf& target_rot, float duration, uint32_t easing, float cur_elapsed)
	{
		Controller& c = controllers.at(handle);
		if (c.kind == OnDevice) { check(sgp_movers_set_rotation_track(batch, c.mover, start_rot.v.x, target_rot.v.x, duration, easing, cur_elapsed), "sgp_movers_set_rotation_track"); return; }
		c.rot.set(start_rot.v.x, target_rot.v.x, 4, duration, easing, cur_elapsed);
	}

	// update(world_state, physics_world, opengl_engine, dtime) of every controller: enqueued, not waited for.  Call it once per sub-step, before PhysicsWorld::think(dtime).
	void update(float dtime)
	{
		resolvePending();
		check(sgp_movers_update(batch, dtime), "sgp_movers_update");
		for (Controller& c : controllers) if (c.kind == OnHost && (c.pos.active || c.rot.active)) hostMoveTo(c, dtime);
	}

	// evalSegmentCurvePos(waypoint_index, frac) of a path controller (ObjectPathController.cpp:396-438), on the host
	Vec4f evalSegmentCurvePos(uint32_t handle, int waypoint_index, float frac)
	{
		const Controller& c = controllers.at(handle);
		sgp_path_segment s[SGP_MOVER_MAX_WAYPOINTS]; uint32_t n = 0;
		check(sgp_movers_path_get(batch, c.path, s, SGP_MOVER_MAX_WAYPOINTS, &n), "sgp_movers_path_get");
		const sgp_path_segment& w = s[waypoint_index];
		const float* entry_pos = w.pos; const float* exit_pos = s[(waypoint_index + 1) % (int)n].pos; const float* prev = s[(waypoint_index + (int)n - 1) % (int)n].pos;
		float begin_dir[3] = { entry_pos[0] - prev[0], entry_pos[1] - prev[1], entry_pos[2] - prev[2] };
		normalise3(begin_dir);
		const float vel = w.speed, t = frac * (w.segment_len / vel), dist = t * vel;
		float p[3];
		if (t < w.entry_segment_len / vel) { for (int k = 0; k < 3; ++k) p[k] = entry_pos[k] + begin_dir[k] * dist; }
		else if (t < (w.entry_segment_len + w.just_curve_len) / vel) {
			const float curve_frac = (dist - w.entry_segment_len) / w.just_curve_len;
			const float d = w.exit_segment_unit_dir[0] * begin_dir[0] + w.exit_segment_unit_dir[1] * begin_dir[1] + w.exit_segment_unit_dir[2] * begin_dir[2];
			float orthog[3] = { w.exit_segment_unit_dir[0] - begin_dir[0] * d, w.exit_segment_unit_dir[1] - begin_dir[1] * d, w.exit_segment_unit_dir[2] - begin_dir[2] * d };
			normalise3(orthog);
			const float angle = curve_frac * w.curve_angle;
			for (int k = 0; k < 3; ++k) p[k] = entry_pos[k] + begin_dir[k] * w.entry_segment_len + (begin_dir[k] * w.curve_r * std::sin(angle) + orthog[k] * w.curve_r * (1 - std::cos(angle)));
		}
		else { for (int k = 0; k < 3; ++k) p[k] = exit_pos[k] - w.exit_segment_unit_dir[k] * (w.segment_len - dist); }
		return Vec4f(p[0], p[1], p[2], 1);
	}

	// waits for what is in flight; the record of a controller that is on the device: states[moverOf(handle)]
	const std::vector<sgp_mover_state>& readBack()
	{
		states.resize(cap);
		check(sgp_movers_get_states(batch, 0, cap, states.data()), "sgp_movers_get_states");
		return states;
	}
	uint32_t moverOf(uint32_t handle) const { const Controller& c = controllers.at(handle); return c.added ? c.mover : SGP_INVALID_ID; }
	uint32_t numPaths() const { return (uint32_t)paths.size(); }
	sgp_movers* handle() const { return batch; }

private:
	enum Kind { OnDevice, OnHost, LeftAlone };
	struct HostTrack
	{
		bool active = false; float start[4] = { 0, 0, 0, 1 }, target[4] = { 0, 0, 0, 1 }, duration = 1.f, elapsed = 0.f; uint32_t easing = 0;
		void set(const float* s, const float* t, int n, float duration_, uint32_t easing_, float cur_elapsed)
		{
			for (int k = 0; k < n; ++k) { start[k] = s[k]; target[k] = t[k]; }
			duration = std::max(duration_, 1.0e-4f); easing = easing_; elapsed = std::max(cur_elapsed, 0.f); active = true;
		}
		float advance(float dtime)      // the eased fraction
		{
			elapsed += dtime;
			float frac = std::max(0.f, std::min(elapsed / duration, 1.f));
			if (easing == SGP_MOVER_EASE_SMOOTHSTEP) frac = (frac * frac) * (3.f - 2.f * frac);
			if (elapsed >= duration) active = false;
			return frac;
		}
	};
	struct Controller
	{
		Kind kind = LeftAlone; PhysicsObject* object = nullptr; uint64_t uid = ~0ull, follow_uid = ~0ull; uint32_t path = SGP_INVALID_ID, mover = SGP_INVALID_ID; bool added = false;
		sgp_mover_desc desc; HostTrack pos, rot;
	};

	static void check(int rc, const char* what) { if (rc != SGP_OK) throw std::runtime_error(std::string(what) + ": " + sgp_last_error()); }
	static void normalise3(float* v) { const float l = std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]); v[0] /= l; v[1] /= l; v[2] /= l; }

	uint32_t pathFor(const std::vector<PathWaypointIn>& waypoints)
	{
		std::vector<sgp_path_waypoint> in(waypoints.size());
		for (size_t i = 0; i < waypoints.size(); ++i) {
			memset(&in[i], 0, sizeof(in[i]));
			for (int k = 0; k < 3; ++k) in[i].pos[k] = waypoints[i].pos[k];
			in[i].type = (uint32_t)waypoints[i].waypoint_type; in[i].pause_time = waypoints[i].pause_time; in[i].speed = waypoints[i].speed;
		}
		const std::string key(in.empty() ? "" : (const char*)in.data(), in.size() * sizeof(sgp_path_waypoint));
		const auto it = paths.find(key);
		if (it != paths.end()) return it->second;
		uint32_t p = 0;
		check(sgp_movers_path_add(batch, in.data(), (uint32_t)in.size(), &p), "sgp_movers_path_add");
		paths[key] = p;
		return p;
	}
	// leaders before followers: a follower is added once the controller of the object it follows is on the device
	void resolvePending()
	{
		for (bool progress = true; progress;) {
			progress = false;
			for (Controller& c : controllers) {
				if (c.added || c.kind != OnDevice || c.desc.kind != SGP_MOVER_PATH) continue;
				if (c.follow_uid != invalid_uid) {
					const Controller* leader = nullptr;
					for (const Controller& l : controllers) if (l.added && l.uid == c.follow_uid && l.desc.kind == SGP_MOVER_PATH) leader = &l;
					if (!leader) continue;
					c.desc.leader = leader->mover;
				}
				check(sgp_mover_add(batch, &c.desc, &c.mover), "sgp_mover_add");
				c.added = true; progress = true;
			}
		}
	}
	// ObjectMoveToController::update for a static body (ObjectMoveToController.cpp:58-103)
	void hostMoveTo(Controller& c, float dtime)
	{
		PhysicsObject& ob = *c.object;
		Vec4f new_pos = ob.pos; Quatf new_rot = ob.rot;
		if (c.pos.active) { const float e = c.pos.advance(dtime); for (int k = 0; k < 3; ++k) new_pos.x[k] = c.pos.start[k] * (1.f - e) + c.pos.target[k] * e; }
		if (c.rot.active) {
			const float e = c.rot.advance(dtime);
			float b[4] = { c.rot.target[0], c.rot.target[1], c.rot.target[2], c.rot.target[3] }; const float* a = c.rot.start;
			float cs = a[0] * b[0] + a[1] * b[1] + a[2] * b[2] + a[3] * b[3], r[4];
			if (cs < 0.f) { for (int k = 0; k < 4; ++k) b[k] = -b[k]; cs = -cs; }
			if (cs > 0.9995f) { for (int k = 0; k < 4; ++k) r[k] = a[k] * (1.f - e) + b[k] * e; }
			else {
				const float theta = std::acos(std::min(cs, 1.f)) * e;
				float p[4]; float pl = 0.f;
				for (int k = 0; k < 4; ++k) { p[k] = b[k] - a[k] * cs; pl += p[k] * p[k]; }
				pl = std::sqrt(pl);
				for (int k = 0; k < 4; ++k) r[k] = a[k] * std::cos(theta) + (p[k] / pl) * std::sin(theta);
			}
			const float l = std::sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2] + r[3] * r[3]);
			new_rot.v = Vec4f(r[0] / l, r[1] / l, r[2] / l, r[3] / l);
		}
		world->setNewObToWorldTransform(ob, new_pos, new_rot, /*linear vel=*/Vec4f(0.f), /*angular vel=*/Vec4f(0.f));
	}

public:
	// Extensions (not in the reference): the batch as it is now, to come back to after PhysicsWorld's rollback to the checkpoint of the same moment -- the
	// library's state and, with it, what this header keeps on the host: the controllers (a follower that still waits for its leader waits again, one that was
	// added since is forgotten; the tracks of the move-to controllers of static bodies with their clocks) and the table of shared paths.
	struct SavedState { BatchCheckpoint lib; std::vector<Controller> controllers; std::map<std::string, uint32_t> paths; std::vector<sgp_mover_state> states; };
	void saveState(SavedState& s)
	{
		check(sgp_movers_checkpoint(batch, &s.lib.cp), "sgp_movers_checkpoint");
		s.controllers = controllers; s.paths = paths; s.states = states;
	}
	void restoreState(const SavedState& s)
	{
		check(sgp_movers_rollback(batch, s.lib.cp), "sgp_movers_rollback");
		controllers = s.controllers; paths = s.paths; states = s.states;
	}

private:

	PhysicsWorld* world;
	sgp_movers* batch;
	uint32_t cap;
	std::vector<Controller> controllers;
	std::map<std::string, uint32_t> paths;
	std::vector<sgp_mover_state> states;
};
