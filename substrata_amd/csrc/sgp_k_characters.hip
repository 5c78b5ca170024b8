// sgp_k_characters.hip -- A7 -- the batched character controller: JPH::CharacterVirtual::Update / ExtendedUpdate for every character of a batch in one launch.
// One of the stage files of the step kernels (stage map: sgp_kernels.h).  Kernels first, their launch wrappers at the end.
#include "sgp_dev_all.h"
#include "sgp_dev_character.h"

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
SGP_DEV bool char_touching(const CharRec* rc, const CharContact& c) { return c.dist <= rc->tolerance + 0.01f; }

// ONE WAVE PER CHARACTER, the whole update inside it (the phases: sgp_dev_character.h).  Every loop is bounded by the description's iteration limits (checked by
// the host) or by a count of at most 128; nothing waits for another workgroup.
__global__ void __launch_bounds__(64) k_characters_update(const DV* __restrict__ dp, CharBufs b, float dt)
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
	const uint32_t move_flags = 1u | ((in.flags & SGP_CHAR_NO_SLIDE) ? 2u : 0u);
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
		b.n_push[k] = S.n_push; b.n_added[k] = S.n_added;
		if (S.n_push) *b.push_any = 1u;
	}
}

// The push records reach the bodies: one wave; lane 0 applies them in ascending character order, then in order of occurrence -- what sgp_body_activate +
// sgp_body_add_force_at in that order would leave (k_apply_cmds), whatever order the update's workgroups ran in.  Pushes are rare (a character against a
// dynamic body); finding them is the 64-wide part.
__global__ void __launch_bounds__(64) k_characters_push(DV d, CharBufs b)
{
	const uint32_t lane = threadIdx.x;
	if (*b.push_any == 0u) return;      // (the same word for every lane: nobody pushed in this update)
	for (uint32_t base = 0; base < b.n; base += 64) {
		const uint32_t k = base + lane;
		const uint32_t cnt = k < b.n ? b.n_push[k] : 0u;
		const unsigned long long pushers = __ballot(cnt > 0u);      // (every lane is here: the serial part below is a branch of lane 0's that ends before the next round)
		if (lane == 0) {
			unsigned long long todo = pushers;
			while (todo) {
				const uint32_t c = base + (uint32_t)(__ffsll((long long)todo) - 1);
				todo &= todo - 1ull;
				const uint32_t nc = min(b.n_push[c], (uint32_t)SGP_CHAR_MAX_PUSHES);
				for (uint32_t r = 0; r < nc; ++r) {
					const CharPush p = b.push[(size_t)c * SGP_CHAR_MAX_PUSHES + r];
					const uint32_t i = p.body;
					if (i >= d.cap_bodies) continue;
					uint32_t f = d.flags[i];
					if (!(f & BF_ALIVE)) continue;
					f = activate_body(d, i, f);      // sgp_body_activate
					if (f_motion(f) == SGP_MOTION_DYNAMIC) {
						// sgp_body_add_force_at
						const v3 Fv = V3(p.f[0], p.f[1], p.f[2]);
						const float4 F = d.force[i], T = d.torque[i];
						d.force[i] = F4(v3_add(V3(F), Fv), F.w);
						d.torque[i] = F4(v3_add(V3(T), v3_cross(v3_sub(V3(p.p[0], p.p[1], p.p[2]), V3(d.pose[POSE_F4 * (size_t)i])), Fv)), T.w);
						f = activate_body(d, i, f) | BF_HAS_FORCE;
					}
					d.flags[i] = f;
				}
				b.n_push[c] = 0u;
			}
		}
	}
	if (lane == 0) *b.push_any = 0u;
}

// sgp_characters_get_states with edits pending and no update to carry them: what the host changed reaches the state
__global__ void __launch_bounds__(TPB) k_characters_sync(CharBufs b)
{
	const uint32_t k = blockIdx.x * TPB + threadIdx.x;
	if (k >= b.n) return;
	const CharRec* rc = &b.rec[k];
	if (!rc->alive) return;
	CharState s = b.st[k];
	char_apply_host(rc, b.in[k], s);
	b.st[k] = s;
}

void launch_characters_update(const DV* d_dev, const CharBufs& b, float dt, hipStream_t s) { if (b.n) hipLaunchKernelGGL(k_characters_update, dim3(b.n), dim3(64), 0, s, d_dev, b, dt); }      // a wave per character
void launch_characters_push(const DV& d, const CharBufs& b, hipStream_t s) { if (b.n) hipLaunchKernelGGL(k_characters_push, dim3(1), dim3(64), 0, s, d, b); }
void launch_characters_sync(const CharBufs& b, hipStream_t s) { if (b.n) hipLaunchKernelGGL(k_characters_sync, dim3(blocks_for(b.n)), dim3(TPB), 0, s, b); }
