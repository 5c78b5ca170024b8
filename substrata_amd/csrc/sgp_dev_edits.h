// sgp_dev_edits.h -- AABB refresh and activation of an edited body.
// Device-inline functions only (no kernels), shared between stage files; included through sgp_dev_all.h, whose order is the dependency order.
#pragma once

// ---------------------------------------------------------------------------------------------------------------
// host edits: one thread per body, its commands applied in submission order

SGP_DEV void refresh_aabb(const DV& d, uint32_t i, uint32_t f)
{
	v3 mn, mx;
	compute_aabb(d, f_shape(f), d.pose[POSE_F4 * (size_t)i + 3], V3(d.pose[POSE_F4 * (size_t)i]), Q4(d.pose[POSE_F4 * (size_t)i + 1]), mn, mx);
	d.aabb_min[i] = F4(mn, 0.0f); d.aabb_max[i] = F4(mx, 0.0f);
}

SGP_DEV uint32_t activate_body(const DV& d, uint32_t i, uint32_t f)
{
	if (!(f & BF_ALIVE) || f_motion(f) == SGP_MOTION_STATIC) return f;
	if (!(f & BF_ACTIVE)) { f |= BF_ACTIVE; push_event(d.ev_activated, &d.evc->n_activated, d.cap_bodies, i); }
	reset_sleep(d, i, f_shape(f), d.pose[POSE_F4 * (size_t)i + 3], V3(d.pose[POSE_F4 * (size_t)i]), Q4(d.pose[POSE_F4 * (size_t)i + 1]));
	return f;
}

// MotionProperties::MoveKinematic: the velocities that take body i from the pose it has to (tp, t) in dt (> 0).  What CMD_MOVE_KINEMATIC and the movers give a body.
SGP_DEV void move_kinematic_velocities(const DV& d, uint32_t i, v3 tp, quat t, float dt, v3& lv, v3& av)
{
	const v3 pos = V3(d.pose[POSE_F4 * (size_t)i]);
	const quat q = Q4(d.pose[POSE_F4 * (size_t)i + 1]);
	lv = v3_scale(v3_sub(tp, pos), 1.0f / dt);
	quat cj; cj.x = -q.x; cj.y = -q.y; cj.z = -q.z; cj.w = q.w;
	quat dq = quat_mul(t, cj);
	if (dq.w < 0.0f) { dq.x = -dq.x; dq.y = -dq.y; dq.z = -dq.z; dq.w = -dq.w; }
	const float sl = sqrtf(dq.x * dq.x + dq.y * dq.y + dq.z * dq.z);
	av = V3(0.0f, 0.0f, 0.0f);
	if (sl > 1.0e-12f) { const float angle = sgd_quat_angle(sl, dq.w); av = v3_scale(V3(dq.x / sl, dq.y / sl, dq.z / sl), angle / dt); }
}
SGP_DEV void store_velocities(const DV& d, uint32_t i, v3 lv, v3 av)
{
	d.vel[VEL_F4 * (size_t)i] = F4(lv, d.vel[VEL_F4 * (size_t)i].w);
	d.vel[VEL_F4 * (size_t)i + 1] = F4(av, d.vel[VEL_F4 * (size_t)i + 1].w);
}
