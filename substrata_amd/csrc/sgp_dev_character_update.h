// sgp_dev_character_update.h -- the body of the character update, for the two stage files that make a kernel of it: sgp_k_characters.hip (k_characters_update<false>, a
// batch without driven characters) and sgp_k_characters_driven.hip (k_characters_update<true>).  The phases it calls: sgp_dev_character.h.
#pragma once
#include "sgp_dev_all.h"
#include "sgp_dev_character.h"
#include "sgp_player_rule.h"

// what the host changed since the state last saw the character's record (every lane alike; the caller stores the state)
SGP_DEV void char_apply_host(const CharRec* rc, const CharIn& in, CharState& s)
{
	if (s.reset_serial != rc->reset_serial) {
		// a new character in this slot: nothing of the previous one is carried over
		for (int i = 0; i < 3; ++i) { s.pos[i] = rc->pose[i]; s.vel[i] = in.vel[i]; s.gn[i] = 0.0f; s.gv[i] = 0.0f; s.gp[i] = 0.0f; }
		s.ground_state = SGP_GROUND_IN_AIR; s.ground_body = SGP_INVALID_ID; s.overflow = 0; s.n_active = 0; s.n_seen = 0;
		s.reset_serial = rc->reset_serial; s.pose_serial = rc->pose_serial; s.in_serial = in.serial;
		return;
	}
	if (s.pose_serial != rc->pose_serial) { for (int i = 0; i < 3; ++i) s.pos[i] = rc->pose[i]; s.pose_serial = rc->pose_serial; }
	if (s.in_serial != in.serial) { for (int i = 0; i < 3; ++i) s.vel[i] = in.vel[i]; s.in_serial = in.serial; }      // (SetLinearVelocity)
}

SGP_DEV bool char_supported(uint32_t ground_state) { return ground_state == SGP_GROUND_ON_GROUND || ground_state == SGP_GROUND_ON_STEEP_GROUND; }

// what a new character in the slot, or a newer jump, makes of the drive state (every lane alike; the caller stores it)
SGP_DEV void char_apply_drive(const CharRec* rc, const CharDrive& dr, CharDriveState& ds)
{
	if (ds.reset_serial != rc->reset_serial) {
		// nothing of the previous character: no jump pending (the host left jump_time = -1 when it added this one, and a jump pressed since is taken below)
		ds.last_jump_time = dr.jump_time; ds.jump_serial = dr.jump_serial; ds.reset_serial = rc->reset_serial;
		ds.campos_z_delta = 0.0f; ds.fraction_submerged = 0.0f; ds.on_ground = 0u; ds.jumped = 0u; ds.num_jumps = 0u; ds.pre_stairs_z = rc->pose[2];
		for (int i = 0; i < 3; ++i) { ds.cam_pos[i] = rc->pose[i]; ds.last_xy[i] = 0.0f; }
		ds.cam_pos[2] = rc->pose[2] + dr.eye_height;
		return;
	}
	if (ds.jump_serial != dr.jump_serial) { ds.last_jump_time = dr.jump_time; ds.jump_serial = dr.jump_serial; }      // (processJump)
}

SGP_DEV pr3 ch_pr3(const float* p) { return PR3(p[0], p[1], p[2]); }

// PlayerPhysics::update in front of a driven character's update (PlayerPhysics.cpp:256-342): UpdateGroundVelocity as the host class makes it -- the contacts at
// the current position with nothing ignored, the supporting contact chosen WITHOUT storing them as active -- where the reference makes it (not flying) and the
// host class does anything (a ground body is set); then the rule of sgp_player_rule.h from the state the previous update left.  The velocity and the ground
// in *sp become what SetLinearVelocity and UpdateGroundVelocity leave; lane 0 stores the drive state.  Returns char_move_shape's flags: notify, and the
// no-slide rule from the rule's own allow_sliding.  Whole wave, every lane alike.  A function of its own: the undriven kernel keeps its registers.
__device__ __noinline__ uint32_t char_drive_before(const DV& d, MeshPairLds<64>& L, CharLds& S, const CharRec* rc, const CharDriveArgs& a, uint32_t k, float dt, CharState* sp)
{
	CharState& s = *sp;
	const CharDrive dr = a.drive[k];
	CharDriveState ds = a.dst[k];
	char_apply_drive(rc, dr, ds);
	if (!(dr.flags & SGP_DRIVE_FLY) && s.ground_body != SGP_INVALID_ID) {
		const v3 position = ch_v3(s.pos);
		char_contacts(d, L, S, rc, SGP_INVALID_ID, position, ch_v3(s.vel));
		const CharGround g = char_supporting_contact(S, rc, position, ch_v3(s.gp), false);
		s.ground_state = g.state; s.ground_body = g.body;
		s.gn[0] = g.n.x; s.gn[1] = g.n.y; s.gn[2] = g.n.z; s.gv[0] = g.v.x; s.gv[1] = g.v.y; s.gv[2] = g.v.z; s.gp[0] = g.p.x; s.gp[1] = g.p.y; s.gp[2] = g.p.z;
	}
	pr_rule_in in;
	in.vel = ch_pr3(s.vel); in.move = ch_pr3(dr.move); in.move_up = dr.move_up; in.flags = dr.flags;
	in.supported = char_supported(s.ground_state) ? 1u : 0u; in.ground_vel = ch_pr3(s.gv); in.ground_normal = ch_pr3(s.gn);
	in.feet_z = s.pos[2]; in.water_enabled = a.water_enabled ? 1u : 0u; in.water_z = a.water_z; in.dt = dt;
	in.jump_due = pr_jump_due(a.cur_time, ds.last_jump_time) ? 1u : 0u;
	in.jump_speed = dr.jump_speed; in.max_air_speed = dr.max_air_speed; in.eye_height = dr.eye_height; in.campos_z_delta = ds.campos_z_delta;
	const pr_rule_out o = pr_update(in);
	s.vel[0] = o.vel.x; s.vel[1] = o.vel.y; s.vel[2] = o.vel.z;
	if (o.jumped) { ds.last_jump_time = -1.0; ds.num_jumps++; }
	ds.campos_z_delta = o.campos_z_delta; ds.fraction_submerged = o.fraction_submerged; ds.on_ground = o.on_ground; ds.jumped = o.jumped; ds.pre_stairs_z = s.pos[2];
	if (threadIdx.x == 0) a.dst[k] = ds;
	return 1u | (o.allow_sliding ? 0u : 2u);
}

// ... and behind it (PlayerPhysics.cpp:450-461): the camera height, last_xy_plane_vel_rel_ground, the camera position.  One lane.
SGP_DEV void char_drive_after(const CharDriveArgs& a, uint32_t k, uint32_t extended, const CharState& s)
{
	const CharDrive& dr = a.drive[k];
	CharDriveState& ds = a.dst[k];
	const float dz = ((dr.flags & SGP_DRIVE_SMOOTH_STAIRS) && extended) ? s.pos[2] - ds.pre_stairs_z : 0.0f;
	const pr_camera_out c = pr_camera(ch_pr3(s.pos), ch_pr3(s.vel), char_supported(s.ground_state) ? 1u : 0u, ch_pr3(s.gv), dz, dr.eye_height, ds.campos_z_delta);
	ds.campos_z_delta = c.campos_z_delta;
	ds.last_xy[0] = c.last_xy_plane_vel_rel_ground.x; ds.last_xy[1] = c.last_xy_plane_vel_rel_ground.y; ds.last_xy[2] = c.last_xy_plane_vel_rel_ground.z;
	ds.cam_pos[0] = c.cam_pos.x; ds.cam_pos[1] = c.cam_pos.y; ds.cam_pos[2] = c.cam_pos.z;
}

SGP_DEV bool char_touching(const CharRec* rc, const CharContact& c) { return c.dist <= rc->tolerance + 0.01f; }

// ONE WAVE PER CHARACTER, the whole update inside it (the phases: sgp_dev_character.h).  Every loop is bounded by the description's iteration limits (checked by
// the host) or by a count of at most 128; nothing waits for another workgroup.
// A driven character (SGP_DRIVE_ON) runs char_drive_before in front of the update and char_drive_after behind it; the branch is the same for the whole workgroup.
// DRIVEN = false is instantiated in sgp_k_characters.hip and updates a batch without any driven slot; DRIVEN = true in a stage file of its own,
// sgp_k_characters_driven.hip.  Two translation units, not two kernels in one: the phases are functions of their own that the compiler specialises for their
// callers (the addresses of the two LDS blocks, the by-value CharBufs), so a second kernel next to the first changes the code of both.  Alone in its file the
// undriven kernel is, instruction for instruction, what it was before there were driven characters (profiles/players_cost.md, (c)).
template <bool DRIVEN> __global__ void __launch_bounds__(64) k_characters_update(const DV* __restrict__ dp, CharBufs b, float dt, CharDriveArgs a)
{
	__shared__ MeshPairLds<64> L;
	__shared__ CharLds S;
	const uint32_t k = blockIdx.x, lane = threadIdx.x;
	if (k >= b.n) return;
	const CharRec* rc = &b.rec[k];
	if (!rc->alive) return;
	const DV& d = *dp;
	const CharIn in = b.in[k];
	CharState s = b.st[k];
	char_apply_host(rc, in, s);
	if (in.flags & SGP_CHAR_DISABLED) { if (lane == 0) b.st[k] = s; return; }
	const uint32_t n_act0 = min(s.n_active, (uint32_t)SGP_CHAR_MAX_CONTACTS), n_seen0 = min(s.n_seen, (uint32_t)SGP_CHAR_MAX_CONTACTS);
	if (lane < n_act0) S.act[lane] = b.active[(size_t)k * SGP_CHAR_MAX_CONTACTS + lane];
	if (lane < n_seen0) S.seen[lane] = b.seen[(size_t)k * SGP_CHAR_MAX_CONTACTS + lane];
	if (lane == 0) { S.n_act = n_act0; S.n_seen = n_seen0; S.n_cur = 0; S.n_k = 0; S.overflow = 0; S.n_push = min(b.n_push[k], (uint32_t)SGP_CHAR_MAX_PUSHES); S.n_added = min(b.n_added[k], (uint32_t)SGP_CHAR_MAX_ADDED); }
	__syncthreads();

	const uint32_t ignore = in.ignore;
	uint32_t move_flags = 1u | ((in.flags & SGP_CHAR_NO_SLIDE) ? 2u : 0u);
	const bool driven = DRIVEN && (a.drive[k].flags & SGP_DRIVE_ON) != 0u;
	if (driven) { CharState t = s; move_flags = char_drive_before(d, L, S, rc, a, k, dt, &t); s = t; }
	const v3 up = ch_v3(rc->up);
	v3 position = ch_v3(s.pos), linear_velocity = ch_v3(s.vel);
	CharGround g; g.state = s.ground_state; g.body = s.ground_body; g.n = ch_v3(s.gn); g.v = ch_v3(s.gv); g.p = ch_v3(s.gp);

	if (!(in.flags & SGP_CHAR_EXTENDED)) {
		// CharacterVirtual::Update
		position = char_move_shape(d, L, S, rc, b, k, position, linear_velocity, dt, ignore, move_flags);
		char_contacts(d, L, S, rc, ignore, position, linear_velocity);
		g = char_supporting_contact(S, rc, position, g.p);
	} else do {
		// CharacterVirtual::ExtendedUpdate
		const v3 wanted = linear_velocity;
		if (!(g.state == SGP_GROUND_ON_GROUND || g.state == SGP_GROUND_IN_AIR)) {
			// CancelVelocityTowardsSteepSlopes
			v3 v = wanted;
			for (uint32_t i = 0; i < S.n_act; ++i) {
				const CharContact& c = S.act[i];
				if ((c.bits & 1u) || !char_touching(rc, c) || !char_too_steep(rc, ch_v3(c.n))) continue;
				const v3 h = v3_sub(ch_v3(c.n), v3_scale(up, v3_dot(ch_v3(c.n), up)));
				const float towards = v3_dot(h, v), l2 = v3_len_sq(h);
				if (towards < 0.0f && l2 > 1.0e-12f) v = v3_sub(v, v3_scale(h, towards / l2));
			}
			linear_velocity = v;
		}
		const v3 before = position;
		bool left_the_ground = char_supported(g.state);
		position = char_move_shape(d, L, S, rc, b, k, position, linear_velocity, dt, ignore, move_flags);
		char_contacts(d, L, S, rc, ignore, position, linear_velocity);
		g = char_supporting_contact(S, rc, position, g.p);
		if (char_supported(g.state)) left_the_ground = false;
		const v3 stick = ch_v3(rc->stick);
		if (left_the_ground && v3_len_sq(stick) > 0.0f && v3_dot(v3_sub(position, before), up) / dt <= 1.0e-6f) {
			// StickToFloor
			v3 n = V3(0.0f, 0.0f, 0.0f);
			const float t = char_cast_down(d, rc, position, stick, ignore, &n);
			if (!(t < 0.0f || char_too_steep(rc, n))) {
				const float len = sqrtf(v3_len_sq(stick));
				position = v3_add(position, v3_scale(stick, ch_max(0.0f, t - rc->padding) / len));
				char_contacts(d, L, S, rc, ignore, position, linear_velocity);
				g = char_supporting_contact(S, rc, position, g.p);
			}
		}
		if (driven && lane == 0) a.dst[k].pre_stairs_z = position.z;      // (pre_stair_walk_position, for SGP_DRIVE_SMOOTH_STAIRS)
		const v3 step_up = ch_v3(rc->stairs_up);
		if (!(v3_len_sq(step_up) > 0.0f)) break;
		v3 want_h = v3_scale(wanted, dt); want_h = v3_sub(want_h, v3_scale(up, v3_dot(want_h, up)));
		const float want_len = sqrtf(v3_len_sq(want_h));
		if (!(want_len > 0.0f)) break;
		const v3 ahead = v3_scale(want_h, 1.0f / want_len);
		v3 got = v3_sub(position, before); got = v3_sub(got, v3_scale(up, v3_dot(got, up)));
		const float got_len = ch_max(0.0f, v3_dot(got, ahead));
		if (!(got_len + 1.0e-4f < want_len)) break;
		{
			// CanWalkStairs(wanted)
			if (!char_supported(g.state)) break;
			const v3 hv = v3_sub(wanted, v3_scale(up, v3_dot(wanted, up)));
			if (v3_len_sq(hv) < 1.0e-12f) break;
			bool can = false;
			for (uint32_t i = 0; i < S.n_act && !can; ++i) {
				const CharContact& c = S.act[i];
				if (!(c.bits & 1u) && char_touching(rc, c) && v3_dot(ch_v3(c.n), v3_sub(hv, ch_v3(c.v))) < 0.0f && char_too_steep(rc, ch_v3(c.n))) can = true;
			}
			if (!can) break;
		}
		const v3 step_forward = v3_scale(ahead, ch_max(rc->min_step_fwd, want_len - got_len));
		v3 test = v3_scale(g.n, -1.0f); test = v3_sub(test, v3_scale(up, v3_dot(test, up)));
		const float tl = sqrtf(v3_len_sq(test));
		test = tl > 1.0e-6f ? v3_scale(test, 1.0f / tl) : ahead;
		if (v3_dot(test, ahead) < rc->cos_fwd) test = ahead;
		const v3 step_forward_test = v3_scale(test, rc->step_fwd_test), step_down_extra = ch_v3(rc->down_extra);
		// WalkStairs
		const v3 start = position;
		const v3 up_pos = v3_add(position, v3_scale(step_up, char_sweep_fraction(d, rc, position, step_up, ignore)));
		const float risen = sqrtf(v3_len_sq(v3_sub(up_pos, position)));
		if (risen < 1.0e-3f) break;
		if (v3_len_sq(step_forward) < 1.0e-10f || !(dt > 0.0f)) break;
		const v3 fwd_pos = char_move_shape(d, L, S, rc, b, k, up_pos, v3_scale(step_forward, 1.0f / dt), dt, ignore, move_flags & 2u);
		const v3 moved = v3_sub(fwd_pos, up_pos);
		if (v3_len_sq(moved) < 1.0e-8f) break;
		const v3 down = v3_add(v3_scale(up, -(risen + 1.0e-3f)), step_down_extra);
		v3 n = V3(0.0f, 0.0f, 0.0f);
		const float t = char_cast_down(d, rc, fwd_pos, down, ignore, &n);
		if (t < 0.0f) break;
		if (char_too_steep(rc, n)) {
			v3 n2 = V3(0.0f, 0.0f, 0.0f);
			const float t2 = char_cast_down(d, rc, v3_add(fwd_pos, step_forward_test), down, ignore, &n2);
			if (t2 < 0.0f || char_too_steep(rc, n2)) break;
		}
		const float len = sqrtf(v3_len_sq(down));
		const v3 new_pos = v3_add(fwd_pos, v3_scale(down, ch_max(0.0f, t - rc->padding) / len));
		if (v3_dot(v3_sub(new_pos, start), up) < 1.0e-3f && v3_len_sq(v3_sub(new_pos, start)) < 1.0e-6f) break;
		position = new_pos;
		char_contacts(d, L, S, rc, ignore, position, linear_velocity);
		g = char_supporting_contact(S, rc, position, g.p);
	} while (false);

	__syncthreads();
	const uint32_t n_act = S.n_act, n_seen = min(S.n_seen, (uint32_t)SGP_CHAR_MAX_CONTACTS);
	if (lane < n_act) b.active[(size_t)k * SGP_CHAR_MAX_CONTACTS + lane] = S.act[lane];
	if (lane < n_seen) b.seen[(size_t)k * SGP_CHAR_MAX_CONTACTS + lane] = S.seen[lane];
	if (lane == 0) {
		s.pos[0] = position.x; s.pos[1] = position.y; s.pos[2] = position.z;
		s.vel[0] = linear_velocity.x; s.vel[1] = linear_velocity.y; s.vel[2] = linear_velocity.z;
		s.ground_state = g.state; s.ground_body = g.body;
		s.gn[0] = g.n.x; s.gn[1] = g.n.y; s.gn[2] = g.n.z; s.gv[0] = g.v.x; s.gv[1] = g.v.y; s.gv[2] = g.v.z; s.gp[0] = g.p.x; s.gp[1] = g.p.y; s.gp[2] = g.p.z;
		s.overflow = S.overflow; s.n_active = n_act; s.n_seen = n_seen;
		b.st[k] = s;
		if (driven) char_drive_after(a, k, in.flags & SGP_CHAR_EXTENDED, s);
		b.n_push[k] = S.n_push; b.n_added[k] = S.n_added;
		if (S.n_push) *b.push_any = 1u;
	}
}
