// sgp_dev_movers.h -- one mover through ObjectPathController::update (gui_client/ObjectPathController.cpp:441-526) or ObjectMoveToController::update
// (gui_client/ObjectMoveToController.cpp:58-114), for k_movers_update and k_movers_follow.  Included by sgp_k_movers.hip after sgp_dev_all.h.  The path
// arithmetic is sgp_mover_path.h, shared with the host; every expression is written out in docs/CONTRACT.md 4j, from which tests/mover_reference.py restates it.
#pragma once
#include "sgp_mover_path.h"

SGP_DEV v3 mover_v3(mp3 a) { return V3(a.x, a.y, a.z); }
SGP_DEV quat mover_quat(const float* p) { quat q; q.x = p[0]; q.y = p[1]; q.z = p[2]; q.w = p[3]; return q; }

// what the host changed since the last update: a new mover in the slot, a new track
SGP_DEV void mover_apply_host(const MoverRec* rc, MoverDyn& dy)
{
	if (dy.reset_serial != rc->reset_serial) {
		dy.reset_serial = rc->reset_serial; dy.pos_serial = 0u; dy.rot_serial = 0u; dy.update_index = 0u;
		dy.index = rc->init_index; dy.dist = rc->init_dist; dy.time = rc->init_time;
		dy.pos_active = 0u; dy.rot_active = 0u; dy.pos_elapsed = 0.0f; dy.rot_elapsed = 0.0f;
		dy.last_pos[0] = rc->hold_pos[0]; dy.last_pos[1] = rc->hold_pos[1]; dy.last_pos[2] = rc->hold_pos[2];
		dy.last_rot[0] = rc->hold_rot[0]; dy.last_rot[1] = rc->hold_rot[1]; dy.last_rot[2] = rc->hold_rot[2]; dy.last_rot[3] = rc->hold_rot[3];
	}
	if (dy.pos_serial != rc->pos_serial) { dy.pos_serial = rc->pos_serial; dy.pos_active = 1u; dy.pos_elapsed = rc->pos_elapsed; }      // setPositionTrack
	if (dy.rot_serial != rc->rot_serial) { dy.rot_serial = rc->rot_serial; dy.rot_active = 1u; dy.rot_elapsed = rc->rot_elapsed; }      // setRotationTrack
}

// the body of a mover, if it still is the live kinematic body the mover was added on (the host clears nothing on the device: rc->gone says the slot changed hands)
SGP_DEV bool mover_body(const DV& d, const MoverRec* rc, uint32_t& f)
{
	const uint32_t i = rc->body;
	f = (rc->gone || i >= d.cap_bodies) ? 0u : d.flags[i];
	return (f & BF_ALIVE) && !(f & BF_ALIAS) && f_motion(f) == SGP_MOTION_KINEMATIC;
}

// PhysicsWorld::moveKinematicObject: as CMD_MOVE_KINEMATIC of k_apply_cmds does it for the body and for the alias slots of a mesh body
SGP_DEV void mover_move_body(const DV& d, uint32_t i, uint32_t f, v3 pos, quat rot, float dt)
{
	v3 lv, av;
	move_kinematic_velocities(d, i, pos, rot, dt, lv, av);
	store_velocities(d, i, lv, av);
	if (f_shape(f) == SGP_SHAPE_MESH && i + 2u < d.cap_bodies)      // (the alias slots share the body's pose: the same velocities; they are never awake themselves)
		for (uint32_t k = 1u; k <= 2u; ++k) if ((d.flags[i + k] & (BF_ALIVE | BF_ALIAS)) == (BF_ALIVE | BF_ALIAS)) store_velocities(d, i + k, lv, av);
	d.flags[i] = activate_body(d, i, f);
}

SGP_DEV void mover_state_store(sgp_mover_state* out, const MoverDyn& dy, uint32_t status, uint32_t index, float dist, float time, v3 pos, quat rot, v3 dir)
{
	sgp_mover_state s;
	s.status = status | (dy.pos_active ? SGP_MOVER_ST_POS_ACTIVE : 0u) | (dy.rot_active ? SGP_MOVER_ST_ROT_ACTIVE : 0u);
	s.waypoint_index = index; s.dist_along_segment = dist; s.time_along_segment = time;
	s.pos[0] = pos.x; s.pos[1] = pos.y; s.pos[2] = pos.z; s.rot[0] = rot.x; s.rot[1] = rot.y; s.rot[2] = rot.z; s.rot[3] = rot.w;
	s.dir[0] = dir.x; s.dir[1] = dir.y; s.dir[2] = dir.z;
	s.pos_elapsed = dy.pos_elapsed; s.rot_elapsed = dy.rot_elapsed; s.update_index = dy.update_index;
	*out = s;
}

// the record of a mover that has not run yet: where it starts (what sgp_movers_get_states reports before the first update)
SGP_DEV void mover_state_fresh(sgp_mover_state* out, const MoverRec* rc, const MoverDyn& dy)
{
	mover_state_store(out, dy, 0u, dy.index, dy.dist, dy.time, V3(rc->hold_pos[0], rc->hold_pos[1], rc->hold_pos[2]), mover_quat(rc->kind == SGP_MOVER_PATH ? rc->base_rot : rc->hold_rot), V3(0.0f, 0.0f, 0.0f));
}

// ObjectPathController.cpp:486-498
SGP_DEV quat mover_path_rotation(const MoverRec* rc, v3 dir)
{
	const quat base = mover_quat(rc->base_rot);
	if (!(rc->flags & SGP_MOVER_ORIENT_ALONG_PATH)) return base;
	const float track_angle = atan2f(dir.y, dir.x);
	quat track; track.x = 0.0f; track.y = 0.0f; track.z = sinf(0.5f * track_angle); track.w = cosf(0.5f * track_angle);      // Quatf::fromAxisAndAngle((0,0,1), track_angle)
	return quat_mul(track, base);
}

SGP_DEV float mover_easing(float frac, uint32_t easing) { return easing == SGP_MOVER_EASE_SMOOTHSTEP ? mp_smoothstep01(frac) : frac; }      // applyEasing

// Quatf::slerp (UNVERIFIED: docs/CONTRACT.md 4j)
SGP_DEV quat mover_slerp(quat a, quat b, float t)
{
	float c = ((a.x * b.x + a.y * b.y) + a.z * b.z) + a.w * b.w;
	if (c < 0.0f) { b.x = -b.x; b.y = -b.y; b.z = -b.z; b.w = -b.w; c = -c; }
	quat r;
	if (c > 0.9995f) {      // nearly parallel: the normalised lerp
		r.x = mp_lerp(a.x, b.x, t); r.y = mp_lerp(a.y, b.y, t); r.z = mp_lerp(a.z, b.z, t); r.w = mp_lerp(a.w, b.w, t);
	} else {
		const float theta = acosf(mp_clamp(c, -1.0f, 1.0f));
		const float tp = theta * t;
		quat p; p.x = b.x - a.x * c; p.y = b.y - a.y * c; p.z = b.z - a.z * c; p.w = b.w - a.w * c;
		const float pl = sqrtf(((p.x * p.x + p.y * p.y) + p.z * p.z) + p.w * p.w);
		p.x = p.x / pl; p.y = p.y / pl; p.z = p.z / pl; p.w = p.w / pl;
		const float cs = cosf(tp), sn = sinf(tp);
		r.x = a.x * cs + p.x * sn; r.y = a.y * cs + p.y * sn; r.z = a.z * cs + p.z * sn; r.w = a.w * cs + p.w * sn;
		return r;
	}
	const float l = sqrtf(((r.x * r.x + r.y * r.y) + r.z * r.z) + r.w * r.w);
	r.x = r.x / l; r.y = r.y / l; r.z = r.z / l; r.w = r.w / l;
	return r;
}

// ObjectMoveToController::update (:58-84): the two tracks for dt; an inactive track holds what it wrote last
SGP_DEV void mover_moveto(const MoverRec* rc, MoverDyn& dy, float dt, v3& pos, quat& rot)
{
	if (dy.pos_active) {
		dy.pos_elapsed += dt;
		const float frac = mp_clamp(dy.pos_elapsed / rc->pos_duration, 0.0f, 1.0f);
		const mp3 p = mp_lerp3(MP3(rc->pos_start), MP3(rc->pos_target), mover_easing(frac, rc->pos_easing));
		if (dy.pos_elapsed >= rc->pos_duration) dy.pos_active = 0u;
		dy.last_pos[0] = p.x; dy.last_pos[1] = p.y; dy.last_pos[2] = p.z;
	}
	if (dy.rot_active) {
		dy.rot_elapsed += dt;
		const float frac = mp_clamp(dy.rot_elapsed / rc->rot_duration, 0.0f, 1.0f);
		const quat q = mover_slerp(mover_quat(rc->rot_start), mover_quat(rc->rot_target), mover_easing(frac, rc->rot_easing));
		if (dy.rot_elapsed >= rc->rot_duration) dy.rot_active = 0u;
		dy.last_rot[0] = q.x; dy.last_rot[1] = q.y; dy.last_rot[2] = q.z; dy.last_rot[3] = q.w;
	}
	pos = V3(dy.last_pos[0], dy.last_pos[1], dy.last_pos[2]);
	rot = mover_quat(dy.last_rot);
}
