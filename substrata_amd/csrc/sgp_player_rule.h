// sgp_player_rule.h -- the velocity rule of PlayerPhysics::update (gui_client/PlayerPhysics.cpp:256-342) and what follows its ExtendedUpdate (:450-461), written
// once for the host and the device.  pr_update restates the rule -- walking, air control, swimming, flying, gravity, the falling cap, the jump --, pr_jump_due the
// jump window, pr_camera the camera height, last_xy_plane_vel_rel_ground and the camera position.  Every expression is fp32 in the reference's order with the
// reference's literals (docs/CONTRACT.md 4n writes them out); the build does not contract a * b + c, so both sides round alike.  A Vec3f operation is written for
// all three components, the zero ones too: x + 0 * dt turns a -0 into +0 as the reference's does.  Plain inline functions: the device compiles them for
// k_characters_update (sgp_k_characters.hip), the host for tests/cpp/player_rule_host_check.cpp.
// UNVERIFIED (glare-core is absent: docs/GAPS.md): Vec3f::length as sqrtf((x * x + y * y) + z * z), normalise as v / length, setLength(l) as v * (l / length),
// myMin(a, b) as a < b ? a : b, myClamp as max(lo, min(x, hi)), removeComponentInDir(v, dir) as v - dir * dot(v, dir) (the movers' form, CONTRACT 4j).
#pragma once
#include <math.h>
#include <stdint.h>
#include "../../include/sgp.h"

#if defined(__HIPCC__)
#define SGP_PR __host__ __device__ inline
#else
#define SGP_PR inline
#endif

struct pr3 { float x, y, z; };
SGP_PR pr3 PR3(float x, float y, float z) { pr3 r; r.x = x; r.y = y; r.z = z; return r; }
SGP_PR pr3 pr_add(pr3 a, pr3 b) { return PR3(a.x + b.x, a.y + b.y, a.z + b.z); }
SGP_PR pr3 pr_sub(pr3 a, pr3 b) { return PR3(a.x - b.x, a.y - b.y, a.z - b.z); }
SGP_PR pr3 pr_scale(pr3 a, float s) { return PR3(a.x * s, a.y * s, a.z * s); }
SGP_PR float pr_dot(pr3 a, pr3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
SGP_PR float pr_length(pr3 a) { return sqrtf(pr_dot(a, a)); }                                                   // Vec3f::length
SGP_PR pr3 pr_normalise(pr3 a) { const float l = pr_length(a); return PR3(a.x / l, a.y / l, a.z / l); }         // normalise
SGP_PR pr3 pr_set_length(pr3 a, float len) { return pr_scale(a, len / pr_length(a)); }                          // Vec3f::setLength
SGP_PR float pr_min(float a, float b) { return a < b ? a : b; }                                                 // myMin
SGP_PR float pr_max(float a, float b) { return a > b ? a : b; }
SGP_PR float pr_clamp(float x, float lo, float hi) { return pr_max(lo, pr_min(x, hi)); }                        // myClamp
SGP_PR pr3 pr_remove_component(pr3 v, pr3 dir) { return pr_sub(v, pr_scale(dir, pr_dot(v, dir))); }             // removeComponentInDir

struct pr_rule_in {
	pr3 vel;                 // GetLinearVelocity
	pr3 move;                // move_desired_vel as processMoveForwards / processStrafeRight summed it
	float move_up;           // processMoveUp's term
	uint32_t flags;          // SGP_DRIVE_*
	uint32_t supported;      // IsSupported, after UpdateGroundVelocity
	pr3 ground_vel, ground_normal;
	float feet_z;            // GetPosition().z
	uint32_t water_enabled; float water_z;
	float dt;
	uint32_t jump_due;       // pr_jump_due
	float jump_speed, max_air_speed, eye_height;
	float campos_z_delta;
};
struct pr_rule_out {
	pr3 vel;                 // what SetLinearVelocity gets
	pr3 move;                // move_desired_vel with processMoveUp's term where it counts
	uint32_t on_ground, jumped, allow_sliding;
	float fraction_submerged;
	float campos_z_delta;    // after the decay of :313-315
};

// computeSubmergedFraction (:180-190)
SGP_PR float pr_submerged_fraction(uint32_t water_enabled, float water_z, float feet_z, float eye_height)
{
	if (!water_enabled) return 0.f;
	const float dist_foot_under_water = water_z - feet_z;
	return pr_clamp(dist_foot_under_water / eye_height, 0.f, 1.f);
}

// the jump window of :321-322: in doubles, JUMP_PERIOD the float 0.1f promoted
SGP_PR bool pr_jump_due(double cur_time, double last_jump_time)
{
	const double time_since_jump_pressed = cur_time - last_jump_time;
	return time_since_jump_pressed < (double)0.1f;
}

// PlayerPhysics::update :256-342
SGP_PR pr_rule_out pr_update(const pr_rule_in& in)
{
	pr_rule_out o;
	const bool fly_mode = (in.flags & SGP_DRIVE_FLY) != 0u, gravity_enabled = (in.flags & SGP_DRIVE_GRAVITY) != 0u;
	const float dtime = in.dt;
	const float fraction_submerged = pr_submerged_fraction(in.water_enabled, in.water_z, in.feet_z, in.eye_height);
	// processMoveUp (:199-209): honoured when flying, with the free camera, or under water
	pr3 move_desired_vel = in.move;
	if (fly_mode || (in.flags & SGP_DRIVE_FREE_CAMERA) || fraction_submerged > 0.3f) move_desired_vel = pr_add(move_desired_vel, PR3(0.f * in.move_up, 0.f * in.move_up, 1.f * in.move_up));
	o.move = move_desired_vel;
	o.allow_sliding = (move_desired_vel.x != 0.f || move_desired_vel.y != 0.f || move_desired_vel.z != 0.f) ? 1u : 0u;
	o.fraction_submerged = fraction_submerged;

	pr3 vel = in.vel;
	if (!fly_mode) {
		pr3 parallel_vel = move_desired_vel;
		if (fraction_submerged < 0.3f) parallel_vel.z = 0;
		if (in.supported && ((vel.z - in.ground_vel.z) < 0.1f)) {
			vel = parallel_vel;
			vel = pr_add(vel, in.ground_vel);
		} else {
			if (pr_length(parallel_vel) > in.max_air_speed) parallel_vel = pr_set_length(parallel_vel, in.max_air_speed);
			vel = pr_add(vel, pr_scale(parallel_vel, dtime));
		}
		if (gravity_enabled) {
			const pr3 gravity_accel = PR3(0, 0, -9.81f);
			vel = pr_add(vel, pr_scale(gravity_accel, dtime));
			const pr3 buoyancy_accel = PR3(0, 0, 9.81f * 1.1f * fraction_submerged);
			vel = pr_add(vel, pr_scale(buoyancy_accel, dtime));
			vel = pr_scale(vel, 1.f - pr_min(0.2f, 2.0f * fraction_submerged * dtime));
		}
		if (vel.z < -100) vel.z = -100;
	} else {
		const float speed = pr_length(vel);
		const pr3 desired_vel = (pr_length(move_desired_vel) < 1.e-4f) ? PR3(0.f, 0.f, 0.f) : pr_scale(pr_normalise(move_desired_vel), speed);
		const pr3 accel = pr_add(pr_scale(move_desired_vel, 3.f), pr_scale(pr_sub(desired_vel, vel), 2.f));
		vel = pr_add(vel, pr_scale(accel, dtime));
	}

	float campos_z_delta = in.campos_z_delta;
	campos_z_delta = campos_z_delta - 20.f * dtime * campos_z_delta;
	if (fabsf(campos_z_delta) < 1.0e-5f) campos_z_delta = 0;
	o.campos_z_delta = campos_z_delta;

	o.on_ground = (in.supported && ((in.vel.z - in.ground_vel.z) < 0.1f)) ? 1u : 0u;
	o.jumped = 0u;
	if (in.jump_due && in.supported) {
		o.on_ground = 0u;
		if (fly_mode) vel = pr_add(vel, PR3(0, 0, in.jump_speed));
		else vel = pr_add(pr_add(pr_remove_component(move_desired_vel, in.ground_normal), in.ground_vel), PR3(0, 0, in.jump_speed));
		o.jumped = 1u;      // (the caller sets last_jump_time = -1)
	}
	o.vel = vel;
	return o;
}

struct pr_camera_out { float campos_z_delta; pr3 last_xy_plane_vel_rel_ground, cam_pos; };
// PlayerPhysics::update :450-461, after ExtendedUpdate.  dz: GetPosition().z - pre_stair_walk_position.z
SGP_PR pr_camera_out pr_camera(pr3 pos, pr3 vel, uint32_t supported, pr3 ground_vel, float dz, float eye_height, float campos_z_delta)
{
	pr_camera_out o;
	o.campos_z_delta = pr_clamp(campos_z_delta + dz, -0.3f, 0.3f);
	o.last_xy_plane_vel_rel_ground = supported ? pr_sub(vel, ground_vel) : vel;
	o.last_xy_plane_vel_rel_ground.z = 0;
	o.cam_pos = PR3(pos.x, pos.y, pos.z + eye_height - o.campos_z_delta);
	return o;
}
