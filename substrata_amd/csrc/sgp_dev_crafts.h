// sgp_dev_crafts.h -- one craft through HoverCarPhysics::update (gui_client/HoverCarPhysics.cpp:76-407) or BoatPhysics::update (gui_client/BoatPhysics.cpp:105-391),
// for k_crafts_update.  Included by sgp_k_crafts.hip after sgp_dev_all.h and sgp_dev_raycast.h.  Every expression is written out in docs/CONTRACT.md ("Crafts"),
// from which tests/craft_reference.py restates it in numpy; the build does not contract a * b + c, so each line rounds as it reads.
#pragma once

// the generator of the crafts (docs/CONTRACT.md): a function of (seed, update index, draw index) alone
SGP_DEV float craft_rand(uint32_t seed, uint32_t update_index, uint32_t draw)
{
	uint32_t h = seed ^ (update_index * 0x9E3779B9u) ^ (draw * 0x85EBCA6Bu);
	h ^= h >> 16; h *= 0x7FEB352Du;
	h ^= h >> 15; h *= 0x846CA68Bu;
	h ^= h >> 16;
	return (float)(h >> 8) * 5.9604644775390625e-8f;      // 2^-24
}

// the body's accumulators in registers: every operation adds to them as k_apply_cmds adds the command of the same name, in the order of the calls
struct CraftAcc { v3 F, T, sumF, sumT, pos; bool any; };
SGP_DEV void craft_add_force(CraftAcc& a, v3 f) { a.F = v3_add(a.F, f); a.sumF = v3_add(a.sumF, f); a.any = true; }
SGP_DEV void craft_add_torque(CraftAcc& a, v3 t) { a.T = v3_add(a.T, t); a.sumT = v3_add(a.sumT, t); a.any = true; }
SGP_DEV void craft_add_force_at(CraftAcc& a, v3 f, v3 p)
{
	const v3 t = v3_cross(v3_sub(p, a.pos), f);
	a.F = v3_add(a.F, f); a.T = v3_add(a.T, t); a.sumF = v3_add(a.sumF, f); a.sumT = v3_add(a.sumT, t); a.any = true;
}

struct CraftFrame { m33 R; v3 pos, right, fwd, up; quat r_quat; };
SGP_DEV v3 craft_point(const CraftFrame& fr, v3 p_os) { return v3_add(m33_mul(fr.R, p_os), fr.pos); }      // to_world * point
SGP_DEV v3 craft_normalise(v3 v) { const float l = v3_len(v); return V3(v.x / l, v.y / l, v.z / l); }
SGP_DEV v3 craft_div(v3 v, float s) { return V3(v.x / s, v.y / s, v.z / s); }

SGP_DEV CraftFrame craft_frame(const CraftRec* rc, v3 pos, quat q)
{
	CraftFrame fr;
	quat r1, r2; r1.x = rc->q1[0]; r1.y = rc->q1[1]; r1.z = rc->q1[2]; r1.w = rc->q1[3]; r2.x = rc->q2[0]; r2.y = rc->q2[1]; r2.z = rc->q2[2]; r2.w = rc->q2[3];
	fr.r_quat = quat_mul(r2, r1);                                  // R_quat = rot_2 * rot_1
	quat cj; cj.x = -fr.r_quat.x; cj.y = -fr.r_quat.y; cj.z = -fr.r_quat.z; cj.w = fr.r_quat.w;
	const m33 Ri = quat_to_m33(cj);                                // R_inv
	const v3 right_os = Ri.c0, fwd_os = Ri.c1;                     // R_inv * (1,0,0,0), R_inv * (0,1,0,0): the columns
	const v3 up_os = v3_cross(right_os, fwd_os);
	fr.R = quat_to_m33(q); fr.pos = pos;
	fr.right = m33_mul(fr.R, right_os); fr.fwd = m33_mul(fr.R, fwd_os); fr.up = m33_mul(fr.R, up_os);
	return fr;
}

// https://en.wikipedia.org/wiki/Lift_coefficient as HoverCarPhysics.cpp:63-73 has it
SGP_DEV float craft_lift_coeff(float cos_theta)
{
	const float theta = acosf(cos_theta);
	const float alpha = 1.5707964f - theta;
	return alpha < 25.0f * 0.017453292f ? 2.0f : 0.0f;
}

// (axis * angle) of JPH::Quat::GetAxisAngle
SGP_DEV v3 craft_axis_times_angle(quat d)
{
	if (d.w < 0.0f) { d.x = -d.x; d.y = -d.y; d.z = -d.z; d.w = -d.w; }      // EnsureWPositive
	if (d.w >= 1.0f) return V3(0.0f, 0.0f, 0.0f);
	const float angle = 2.0f * acosf(d.w);
	const float len_sq = d.x * d.x + d.y * d.y + d.z * d.z;
	if (len_sq <= 1.17549435e-38f) return V3(0.0f, 0.0f, 0.0f);              // NormalizedOr(zero)
	const float len = sqrtf(len_sq);
	return v3_scale(V3(d.x / len, d.y / len, d.z / len), angle);
}

// the torque towards "current yaw, no pitch or roll" (HoverCarPhysics.cpp:214-234, BoatPhysics.cpp:367-385)
SGP_DEV v3 craft_correction_torque(const CraftFrame& fr, quat q, float yaw, v3 ang_vel, float mass, float gain)
{
	quat yq; yq.x = 0.0f; yq.y = 0.0f; yq.z = sinf(0.5f * yaw); yq.w = cosf(0.5f * yaw);      // Quat::sRotation((0,0,1), yaw)
	const quat desired = quat_mul(yq, fr.r_quat);
	quat cj; cj.x = -q.x; cj.y = -q.y; cj.z = -q.z; cj.w = q.w;
	const v3 desired_ang_vel = v3_scale(craft_axis_times_angle(quat_mul(desired, cj)), 3.0f);
	return v3_scale(v3_scale(v3_sub(desired_ang_vel, ang_vel), mass), gain);
}

SGP_DEV void craft_emit(sgp_particle* slots, uint32_t& n, uint32_t craft, uint32_t kind, uint32_t& counter, v3 pos, v3 vel, float area, float width, float opacity, float dopacity_dt, uint32_t flags)
{
	if (n >= SGP_CRAFT_MAX_EMIT) return;      // (cannot happen: 6 + 2 x 8)
	sgp_particle p;
	p.pos[0] = pos.x; p.pos[1] = pos.y; p.pos[2] = pos.z; p.vel[0] = vel.x; p.vel[1] = vel.y; p.vel[2] = vel.z;
	p.area = area; p.mass = 1.0e-6f; p.restitution = 0.5f; p.width = width; p.dwidth_dt = 1.0f; p.opacity = opacity; p.dopacity_dt = dopacity_dt; p.flags = flags;
	p.tag = ((uint64_t)craft << 32) | ((uint64_t)kind << 28) | (uint64_t)(counter & 0x0FFFFFFFu);
	counter++;
	slots[n++] = p;
}

struct CraftOut { uint32_t branches; bool wake; v3 trace_origin; float trace_t; uint32_t trace_body; };

// HoverCarPhysics::update with user_in_driver_seat (without a driver the reference does nothing)
SGP_DEV void craft_hovercar(const DV& d, const CraftRec* rc, const CraftIn& in, CraftDyn& dy, const CraftFrame& fr, quat q, v3 lin_vel, v3 ang_vel, float dt,
                            int water_enabled, float water_z, uint32_t craft, CraftAcc& acc, CraftOut& o, sgp_particle* slots, uint32_t& n_emit)
{
	const float mass = rc->mass, forward = in.forward, right = in.right, up = in.up;
	if (right != 0.0f || forward != 0.0f || in.hand_brake != 0.0f) { o.wake = true; o.branches |= SGP_CRAFT_BR_ACTIVATE; }
	if (fr.up.z > 0.0f) {
		const float up_force_factor = 1.0f / fmaxf(0.7f, fr.up.z);
		craft_add_force(acc, v3_scale(v3_scale(v3_scale(v3_scale(fr.up, 1.0f + up * 0.6f), up_force_factor), mass), 9.81f));
		o.branches |= SGP_CRAFT_BR_HOVER;
	}
	if (dy.unflip > 0.0f) {
		if ((double)fr.up.z > 0.2) dy.unflip = -1.0f;
		else {
			craft_add_force(acc, v3_scale(v3_scale(v3_scale(V3(0.0f, 0.0f, 1.0f), 1.0f), mass), 9.81f));
			dy.unflip -= dt;
			o.branches |= SGP_CRAFT_BR_UNFLIP;
		}
	}
	else if ((double)fr.up.z < -0.9) dy.unflip = 1.0f;

	const v3 forwards_control_force = v3_scale(v3_scale(v3_scale(fr.fwd, mass), 10.0f), forward);
	craft_add_force(acc, forwards_control_force);
	craft_add_force(acc, v3_scale(fr.up, -forwards_control_force.z));
	craft_add_torque(acc, v3_scale(v3_scale(v3_scale(fr.right, mass), -0.5f), forward));
	craft_add_torque(acc, v3_scale(v3_scale(v3_scale(fr.up, mass), -3.0f), right));
	craft_add_torque(acc, v3_scale(v3_scale(v3_scale(fr.fwd, mass), 2.0f), right));
	craft_add_torque(acc, craft_correction_torque(fr, q, atan2f(fr.right.y, fr.right.x), ang_vel, mass, 1.5f));

	const float v_mag = v3_len(lin_vel);
	if (v_mag > 1.0e-3f) {
		const v3 nv = craft_div(lin_vel, v_mag);
		const float rho = 1.293f;
		const float forwards_F_d = 0.5f * rho * v_mag * v_mag * 0.2f * (fabsf(v3_dot(nv, fr.fwd)) * 2.0f);
		const float side_F_d = 0.5f * rho * v_mag * v_mag * 0.5f * (fabsf(v3_dot(nv, fr.right)) * 4.0f);
		const float top_F_d = 0.5f * rho * v_mag * v_mag * 0.75f * (fabsf(v3_dot(nv, fr.up)) * 8.0f);
		const float total_F_d = forwards_F_d + side_F_d + top_F_d;
		craft_add_force(acc, v3_scale(nv, -total_F_d));
		o.branches |= SGP_CRAFT_BR_DRAG;

		const v3 up_lift_dir = v3_sub(fr.up, v3_scale(nv, v3_dot(fr.up, nv)));      // removeComponentInDir
		if (v3_len(up_lift_dir) > 1.0e-3f) {
			const float top_dot = v3_dot(nv, fr.up);
			const float top_C_L = craft_lift_coeff(top_dot);
			const float projected_top_area = top_dot * 8.0f;
			if (top_C_L > 0.0f && projected_top_area > 0.0f) {
				const float top_L = 0.5f * rho * v_mag * v_mag * projected_top_area * top_C_L;
				craft_add_force(acc, v3_scale(v3_neg(craft_normalise(up_lift_dir)), top_L));
				o.branches |= SGP_CRAFT_BR_LIFT_TOP;
			}
			const float projected_bottom_area = -projected_top_area;
			const float bottom_C_L = craft_lift_coeff(-top_dot);
			if (bottom_C_L > 0.0f && projected_bottom_area > 0.0f) {
				const float bottom_L = 0.5f * rho * v_mag * v_mag * projected_bottom_area * bottom_C_L;
				craft_add_force(acc, v3_scale(craft_normalise(up_lift_dir), bottom_L));
				o.branches |= SGP_CRAFT_BR_LIFT_BOTTOM;
			}
		}
		const v3 right_lift_dir = v3_sub(fr.right, v3_scale(nv, v3_dot(fr.right, nv)));
		if (v3_len(right_lift_dir) > 1.0e-3f) {
			const float right_dot = v3_dot(nv, fr.right);
			const float right_C_L = craft_lift_coeff(right_dot);
			const float projected_right_area = v3_dot(nv, fr.right) * 4.0f;
			if (projected_right_area > 0.0f) {      // (no test of the coefficient on this side: a force of zero is still added)
				const float right_L = 0.5f * rho * v_mag * v_mag * projected_right_area * right_C_L;
				craft_add_force(acc, v3_scale(v3_neg(craft_normalise(right_lift_dir)), right_L));
				o.branches |= SGP_CRAFT_BR_LIFT_RIGHT;
			}
			const float projected_left_area = -projected_right_area;
			const float left_C_L = craft_lift_coeff(-right_dot);
			if (projected_left_area > 0.0f) {
				const float left_L = 0.5f * rho * v_mag * v_mag * projected_left_area * left_C_L;
				craft_add_force(acc, v3_scale(craft_normalise(right_lift_dir), left_L));
				o.branches |= SGP_CRAFT_BR_LIFT_LEFT;
			}
		}
	}

	// the ray under the car, and what it raises
	const v3 origin = craft_point(fr, V3(rc->trace_os[0], rc->trace_os[1], rc->trace_os[2]));
	o.trace_origin = origin;
	const float u0 = craft_rand(rc->seed, dy.update_index, 0u), u1 = craft_rand(rc->seed, dy.update_index, 1u);
	const v3 side_vec = v3_add(v3_scale(fr.right, -0.5f + u0), v3_scale(fr.fwd, -0.5f + u1));
	const v3 trace_dir = craft_normalise(v3_add(v3_neg(fr.up), v3_scale(side_vec, 0.8f)));
	const float max_trace_dist = 12.0f;
	sgp_ray ry;
	ry.origin[0] = origin.x; ry.origin[1] = origin.y; ry.origin[2] = origin.z; ry.dir[0] = trace_dir.x; ry.dir[1] = trace_dir.y; ry.dir[2] = trace_dir.z;
	ry.max_t = max_trace_dist; ry.ignore_id = SGP_INVALID_ID; ry.collidable_only = 0u;
	const sgp_hit hit = raycast_one(d, ry);
	const bool hit_object = hit.id != SGP_INVALID_ID;
	o.trace_body = hit.id; o.trace_t = hit.t;
	const float water_hit_dist = (water_z - origin.z) / trace_dir.z;
	if (water_enabled && water_hit_dist >= 0.0f && water_hit_dist < max_trace_dist && (!hit_object || hit.t > water_hit_dist)) {
		const v3 hitpos = v3_add(origin, v3_scale(trace_dir, water_hit_dist));
		const float t = water_hit_dist / max_trace_dist;
		const float vel = 20.0f * (1.0f - t) + 6.0f * t;
		for (uint32_t z = 0; z < 4u; ++z) {
			const float rx = craft_rand(rc->seed, dy.update_index, 2u + 3u * z), ry_ = craft_rand(rc->seed, dy.update_index, 3u + 3u * z), rz = craft_rand(rc->seed, dy.update_index, 4u + 3u * z);
			const v3 pv = v3_scale(v3_add(side_vec, V3(1.0f * (-0.5f + rx), 1.0f * (-0.5f + ry_), rz * 0.2f)), vel);
			craft_emit(slots, n_emit, craft, SGP_CRAFT_PK_SPRAY, dy.counter, hitpos, pv, 0.000001f, 2.0f, 0.5f, -0.06f, SGP_PARTICLE_DIE_ON_HIT);
		}
		o.branches |= SGP_CRAFT_BR_RAY_WATER;
	}
	else if (hit_object) {
		const v3 hitpos = v3_add(origin, v3_scale(trace_dir, hit.t));
		const float t = hit.t / max_trace_dist;
		const float vel = 20.0f * (1.0f - t) + 6.0f * t;
		const float rx = craft_rand(rc->seed, dy.update_index, 2u), ry_ = craft_rand(rc->seed, dy.update_index, 3u), rz = craft_rand(rc->seed, dy.update_index, 4u);
		const v3 pv = v3_scale(v3_add(side_vec, V3(0.0f * (-0.5f + rx), 0.0f * (-0.5f + ry_), rz * 0.2f)), vel);
		craft_emit(slots, n_emit, craft, SGP_CRAFT_PK_DUST, dy.counter, hitpos, pv, 0.00001f, 2.0f, 0.5f, -0.06f, 0u);
		o.branches |= SGP_CRAFT_BR_RAY_BODY;
	}
}

// BoatPhysics::update
SGP_DEV void craft_boat(const DV& d, const CraftRec* rc, const CraftIn& in, CraftDyn& dy, const CraftFrame& fr, quat q, v3 lin_vel, v3 ang_vel, float submerged, float dt,
                        int water_enabled, float water_z, uint32_t craft, CraftAcc& acc, CraftOut& o, sgp_particle* slots, uint32_t& n_emit)
{
	const float forward = in.forward, right = in.right;
	const float forwards_vel = v3_dot(lin_vel, fr.fwd);
	if (in.flags & SGP_CRAFT_IN_DRIVER) {
		if (right != 0.0f || forward != 0.0f) { o.wake = true; o.branches |= SGP_CRAFT_BR_ACTIVATE; }
		const v3 prop = craft_point(fr, V3(rc->prop_os[0], rc->prop_os[1], rc->prop_os[2]));
		if (forward != 0.0f && water_enabled && prop.z <= water_z) {
			const v3 dir = craft_normalise(v3_sub(v3_sub(fr.fwd, v3_scale(fr.up, 0.2f)), v3_scale(v3_scale(fr.right, right), rc->lateral)));
			craft_add_force_at(acc, v3_scale(v3_scale(dir, rc->thrust), forward), prop);
			o.branches |= SGP_CRAFT_BR_THRUST;
			const v3 positions[2] = { v3_sub(prop, v3_scale(fr.right, rc->prop_off)), v3_add(prop, v3_scale(fr.right, rc->prop_off)) };
			const float vel = (in.flags & SGP_CRAFT_IN_BOOST) ? 2.0f : 1.0f;
			const float xy_spread = vel * 0.5f;
			const float width = clampf(rc->jet_w, 0.01f, 2.0f);
			for (uint32_t i = 0; i < 2u; ++i) for (uint32_t z = 0; z < 3u; ++z) {
				const uint32_t base = 3u * (3u * i + z);
				const float rx = craft_rand(rc->seed, dy.update_index, base), ry_ = craft_rand(rc->seed, dy.update_index, base + 1u), rz = craft_rand(rc->seed, dy.update_index, base + 2u);
				const v3 a = v3_scale(fr.fwd, forward * -vel);
				const v3 bterm = v3_scale(v3_scale(v3_scale(fr.right, right), 3.0f), rc->lateral);
				const v3 c = v3_scale(V3(xy_spread * (-0.5f + rx), xy_spread * (-0.5f + ry_), 2.0f + rz * 4.0f), vel);
				craft_emit(slots, n_emit, craft, SGP_CRAFT_PK_JET, dy.counter, positions[i], v3_add(v3_sub(a, bterm), c), 0.000001f, width, 1.0f, -0.3f, SGP_PARTICLE_DIE_ON_HIT);
			}
		}
		if (right != 0.0f) {
			craft_add_force_at(acc, v3_scale(v3_scale(v3_scale(fr.right, -right), forwards_vel), rc->rudder), prop);
			o.branches |= SGP_CRAFT_BR_RUDDER;
		}
	}

	const float forwards_submerged_fraction = submerged / rc->volume, side_submerged_fraction = submerged / rc->volume;
	const float ss = clampf((submerged - 0.0f) / (1.0f - 0.0f), 0.0f, 1.0f);
	const float top_submerged_fraction = ss * ss * (3.0f - 2.0f * ss);      // Maths::smoothStep(0, 1, x)
	const float v_mag = v3_len(lin_vel);
	if (submerged > 0.0f && v_mag > 1.0e-3f) {
		const v3 nv = craft_div(lin_vel, v_mag);
		const float rho = 1020.0f;
		const float forwards_F_d = 0.5f * rho * v_mag * v_mag * 0.1f * (fabsf(v3_dot(nv, fr.fwd)) * rc->a_front) * forwards_submerged_fraction;
		const float side_F_d = 0.5f * rho * v_mag * v_mag * 0.5f * (fabsf(v3_dot(nv, fr.right)) * rc->a_side) * side_submerged_fraction;
		const float top_F_d = 0.5f * rho * v_mag * v_mag * 0.75f * (fabsf(v3_dot(nv, fr.up)) * rc->a_top) * top_submerged_fraction;
		const float total_F_d = forwards_F_d + side_F_d + top_F_d;
		craft_add_force(acc, v3_scale(nv, -total_F_d));
		o.branches |= SGP_CRAFT_BR_DRAG;
		// (the lift block of BoatPhysics.cpp:272-318 is disabled in the reference -- if(0) -- and stays disabled)
	}

	const uint32_t n_splash = min(rc->n_splash, (uint32_t)SGP_CRAFT_MAX_SPLASH_POINTS);
	for (uint32_t p = 0; p < n_splash; ++p) {
		if (!(v_mag > 5.0f)) continue;
		const float sign = rc->splash[4 * p + 3];
		const v3 point = craft_point(fr, V3(rc->splash[4 * p], rc->splash[4 * p + 1], rc->splash[4 * p + 2]));
		const bool immersed = water_enabled && point.z < water_z;
		const v3 right_vel_dir = v3_cross(lin_vel, V3(0.0f, 0.0f, 1.0f));
		const v3 side_vel_dir = v3_scale(right_vel_dir, sign);
		const v3 side_dir = v3_scale(fr.right, sign);
		if (immersed && v3_dot(craft_normalise(lin_vel), side_dir) > -0.5f) {
			for (uint32_t z = 0; z < 2u; ++z) {
				const uint32_t base = 18u + 3u * (2u * p + z);
				const float r0 = craft_rand(rc->seed, dy.update_index, base), r1 = craft_rand(rc->seed, dy.update_index, base + 1u), r2 = craft_rand(rc->seed, dy.update_index, base + 2u);
				const v3 a = v3_scale(lin_vel, 0.6f + (-0.5f + r0) * 0.1f);
				const v3 bterm = v3_scale(side_vel_dir, 0.3f + (-0.5f + r1) * 0.1f);
				const v3 c = v3_scale(v3_scale(V3(0.0f, 0.0f, 1.0f), v_mag), 0.1f + (-0.5f + r2) * 0.08f);
				craft_emit(slots, n_emit, craft, SGP_CRAFT_PK_SPLASH, dy.counter, point, v3_add(v3_add(a, bterm), c), 0.01f, 0.4f, 1.0f, -0.3f, SGP_PARTICLE_DIE_ON_HIT);
			}
			o.branches |= SGP_CRAFT_BR_SPLASH0 << p;
		}
	}

	if (dy.righting > 0.0f) {
		const v3 no_roll_right = craft_normalise(v3_cross(fr.fwd, V3(0.0f, 0.0f, 1.0f)));
		craft_add_torque(acc, craft_correction_torque(fr, q, atan2f(no_roll_right.y, no_roll_right.x), ang_vel, rc->mass, 3.5f));
		dy.righting -= dt;
		o.branches |= SGP_CRAFT_BR_RIGHTING;
	}
}

// what the host changed since the device state last saw the record
SGP_DEV void craft_apply_host(const CraftRec* rc, CraftDyn& dy)
{
	if (dy.reset_serial != rc->reset_serial) {
		dy.unflip = -1.0f; dy.righting = rc->cmd_value; dy.update_index = 0u; dy.counter = 0u;      // (cmd_value: -1 from sgp_craft_add, unless a command came since)
		dy.reset_serial = rc->reset_serial; dy.cmd_serial = rc->cmd_serial;
		return;
	}
	if (dy.cmd_serial != rc->cmd_serial) { dy.righting = rc->cmd_value; dy.cmd_serial = rc->cmd_serial; }
}
