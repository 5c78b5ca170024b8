// sgp_dev_character.h -- the phases of the batched character controller (sgp_k_characters.hip): the contacts of a capsule, the swept sphere, MoveShape with its
// constraint solver, the supporting contact.  One wave per character; the algorithm and every fp32 expression are those of shim/Jolt/JoltCharacterLite.h, which the
// host compiles without contraction -- same expressions in the same order here, so a character of a batch moves bit for bit as the host class moves it.
// The geometry (candidate bodies, collision tests, mesh triangles, sphere casts) is spread over the 64 lanes exactly as k_collide_capsules and k_spherecast's
// callers would have it answered; what follows from it (constraints, sliding, ground state) is a few dozen scalar steps that all lanes take alike, so that
// control flow stays uniform and nothing has to be broadcast.  The large phases are functions of their own (__noinline__): inlined at each of their call
// sites the kernel would carry five copies of the collision code.
#pragma once

// std::max / std::min as the host evaluates them (fmaxf / fminf may pick the other zero)
SGP_DEV float ch_max(float a, float b) { return (a < b) ? b : a; }
SGP_DEV float ch_min(float a, float b) { return (b < a) ? b : a; }
SGP_DEV v3 ch_v3(const float* p) { return V3(p[0], p[1], p[2]); }

struct CharCons { v3 n, vel; float dist; int contact; int steep; };
struct CharLds {
	CharContact cur[SGP_CHAR_MAX_CONTACTS];      // the contacts of the last query, in the host's order (raw body slot, point index)
	CharContact act[SGP_CHAR_MAX_CONTACTS];      // CharacterVirtual::active
	CharCons k[2 * SGP_CHAR_MAX_CONTACTS];
	uint32_t seen[SGP_CHAR_MAX_SEEN];
	uint32_t mesh_list[SGP_CHAR_MESH_LIST];
	uint32_t n_raw, n_cur, n_act, n_k, n_seen, n_mesh, overflow, n_push, n_added;
};
struct CharGround { uint32_t state, body; v3 n, v, p; };

// ---------------------------------------------------------------------------------------------------------------
// CharacterVirtual::getContacts: k_collide_capsules for one capsule (the same capsule_shape, sq_walk, capsule_query_body and contact_record), its records into
// LDS instead of the caller's buffer

struct CharSink {
	const DV& d; CharLds& S; float padding;
	SGP_DEV bool list_mesh(uint32_t j) const { const uint32_t at = atomicAdd(&S.n_mesh, 1u); if (at < SGP_CHAR_MESH_LIST) S.mesh_list[at] = j; return at < SGP_CHAR_MESH_LIST; }
	SGP_DEV void emit(uint32_t j, uint32_t f, int g, const sgd_manifold& m) const
	{
		for (int i = 0; i < m.np; ++i) {
			const uint32_t slot = atomicAdd(&S.n_raw, 1u);
			if (slot >= SGP_CHAR_MAX_CONTACTS) continue;
			const sgp_query_contact q = contact_record(d, 0u, j, f, g, m, i);
			CharContact c;
			c.body = j; c.idx = q.sub_shape;
			for (int a = 0; a < 3; ++a) { c.p[a] = q.point[a]; c.n[a] = q.normal[a]; c.v[a] = q.point_velocity[a]; }
			c.dist = q.distance - padding;
			c.bits = q.is_sensor | (q.motion_type == SGP_MOTION_DYNAMIC ? 2u : 0u);
			c.inv_mass = q.inv_mass;
			S.cur[slot] = c;
		}
	}
};

// the contacts of the capsule at `pos` into S.cur / S.n_cur, sorted; whole wave
__device__ __noinline__ void char_contacts(const DV& d, MeshPairLds<64>& L, CharLds& S, const CharRec* rc, uint32_t ignore, v3 pos, v3 movement)
{
	const uint32_t lane = threadIdx.x;
	const float ml = sqrtf(v3_len_sq(movement));
	const v3 mv = V3(ml > 0.0f ? movement.x / ml : 0.0f, ml > 0.0f ? movement.y / ml : 0.0f, ml > 0.0f ? movement.z / ml : 0.0f);
	const float max_sep = rc->predictive + rc->padding;
	quat qq; qq.x = 0.0f; qq.y = 0.0f; qq.z = 0.0f; qq.w = 1.0f;
	sgd_shape sc; v3 lo, hi;
	capsule_shape(v3_add(pos, ch_v3(rc->offset)), qq, rc->radius, rc->half_height, max_sep, sc, lo, hi);
	const CharSink sink = { d, S, rc->padding };
	__syncthreads();      // (everybody is done with the previous S.cur)
	if (lane == 0) { S.n_mesh = 0; S.n_raw = 0; }
	__syncthreads();
	sq_walk<64>(d, lo, hi, lane, [&](uint32_t j) { capsule_query_body(d, ignore, true, max_sep, sc, lo, hi, j, sink); });      // (collidable only: PlayerPhysicsObjectLayerFilter)
	__syncthreads();
	const uint32_t nm = min(S.n_mesh, (uint32_t)SGP_CHAR_MESH_LIST);
	const v3 es = V3(max_sep, max_sep, max_sep);
	for (uint32_t mi = 0; mi < nm; ++mi) {
		const uint32_t mid = S.mesh_list[mi];
		bool valid = true, dropped = false;
		sgd_shape X = sc;
		mesh_pair_groups<64, 4>(d, L, valid, X, mid, v3_sub(lo, es), v3_add(hi, es), max_sep, 0, (int)lane, 0u, dropped, mv, true);      // (CollideOnlyWithActive + the direction of travel)
		if ((int)lane < L.mc.ng) {
			const sgd_mesh_group& grp = L.mc.g[lane];
			sgd_manifold mm;
			sgd_hull_reduce(grp.n, grp.p_mesh, grp.p_body, grp.np, &mm);
			sink.emit(mid, d.flags[mid], (int)lane, mm);
		}
		__syncthreads();
	}
	// the order of the host's sort: raw body slot, then point index (the keys are unique: a lane's rank is the number of smaller ones)
	const uint32_t n_raw = S.n_raw, n = min(n_raw, (uint32_t)SGP_CHAR_MAX_CONTACTS);
	CharContact mine; uint32_t rank = 0;
	if (lane < n) {
		mine = S.cur[lane];
		const uint64_t key = ((uint64_t)mine.body << 8) | mine.idx;
		for (uint32_t i = 0; i < n; ++i) { const uint64_t other = ((uint64_t)S.cur[i].body << 8) | S.cur[i].idx; if (other < key) ++rank; }
	}
	__syncthreads();
	if (lane < n) S.cur[rank] = mine;
	if (lane == 0) { S.n_cur = n; if (n_raw > SGP_CHAR_MAX_CONTACTS) S.overflow |= 1u; }
	__syncthreads();
}

// ---------------------------------------------------------------------------------------------------------------
// sgp_spherecast for one sphere by the wave: k_spherecast's walk and candidate test (spherecast_walk, spherecast_body), the candidates dealt to the lanes, each lane
// keeping its closest hit, the answer the least (t, body id) of the lanes -- k_spherecast's, whose tie rule makes the result independent of the order of the tests

// returns sgp_hit's id, t (0 without a hit) and normal, the same in every lane
__device__ __noinline__ SphereHit char_spherecast(const DV& d, v3 o, v3 dir, float max_t, float rs, uint32_t ignore)
{
	const uint32_t lane = threadIdx.x;
	SphereHit best; best.t = max_t; best.id = SGP_INVALID_ID; best.n = V3(0.0f, 0.0f, 0.0f);
	spherecast_walk<64>(d, o, dir, max_t, rs, lane, [&](uint32_t j) { spherecast_body(d, ignore, true, max_t, rs, o, dir, j, best); });
	float wt = best.id != SGP_INVALID_ID ? best.t : 3.0e38f; uint32_t wid = best.id;
	for (int off = 32; off >= 1; off >>= 1) {
		const float ot = __shfl_xor(wt, off, 64); const uint32_t oid = (uint32_t)__shfl_xor((int)wid, off, 64);
		if (oid != SGP_INVALID_ID && (wid == SGP_INVALID_ID || ot < wt || (ot == wt && oid < wid))) { wt = ot; wid = oid; }
	}
	SphereHit h; h.id = wid; h.t = 0.0f; h.n = V3(0.0f, 0.0f, 0.0f);
	if (wid != SGP_INVALID_ID) {
		const unsigned long long owners = __ballot(best.id == wid && best.t == wt);
		const int src = __ffsll((long long)owners) - 1;
		h.t = wt;
		h.n = V3(__shfl(best.n.x, src, 64), __shfl(best.n.y, src, 64), __shfl(best.n.z, src, 64));
	}
	return h;
}

// CharacterVirtual::sweepFraction: the two end spheres
SGP_DEV float char_sweep_fraction(const DV& d, const CharRec* rc, v3 pos, v3 displacement, uint32_t ignore)
{
	const float len = sqrtf(v3_len_sq(displacement));
	if (len < 1.0e-6f) return 1.0f;
	const v3 dir = v3_scale(displacement, 1.0f / len);
	const v3 c = v3_add(pos, ch_v3(rc->offset)), up = ch_v3(rc->up);
	float travel = len;
	for (int k = 0; k < 2; ++k) {
		const v3 o = v3_add(c, v3_scale(up, (k ? 1.0f : -1.0f) * rc->half_height));
		const SphereHit h = char_spherecast(d, o, dir, len + rc->padding, rc->radius, ignore);
		if (h.id != SGP_INVALID_ID && h.t > 1.0e-5f) {
			if (h.n.x * dir.x + h.n.y * dir.y + h.n.z * dir.z < -0.05f) travel = ch_min(travel, ch_max(0.0f, h.t - rc->padding));
		}
	}
	return travel / len;
}

// CharacterVirtual::castDown: the lower sphere; travel distance or -1
SGP_DEV float char_cast_down(const DV& d, const CharRec* rc, v3 pos, v3 step, uint32_t ignore, v3* normal_out)
{
	const float len = sqrtf(v3_len_sq(step));
	if (len < 1.0e-6f) return -1.0f;
	const v3 dir = v3_scale(step, 1.0f / len), o = v3_sub(v3_add(pos, ch_v3(rc->offset)), v3_scale(ch_v3(rc->up), rc->half_height));
	const SphereHit h = char_spherecast(d, o, dir, len, rc->radius, ignore);
	if (h.id == SGP_INVALID_ID) return -1.0f;
	*normal_out = h.n;
	return h.t;
}

SGP_DEV bool char_too_steep(const CharRec* rc, v3 n) { return v3_dot(n, ch_v3(rc->up)) < rc->cos_max_slope; }

// ---------------------------------------------------------------------------------------------------------------
// CharacterVirtual::moveShape with solveConstraints and pushBody.  flags: bit 0 notify (contact-added records, the seen list), bit 1 the no-slide rule

__device__ __noinline__ v3 char_move_shape(const DV& d, MeshPairLds<64>& L, CharLds& S, const CharRec* rc, const CharBufs& b, uint32_t k, v3 pos, v3 velocity, float dt, uint32_t ignore, uint32_t flags)
{
	const uint32_t lane = threadIdx.x;
	const bool notify = (flags & 1u) != 0u, no_slide = (flags & 2u) != 0u;
	const v3 up = ch_v3(rc->up);
	const float cos_max_slope = rc->cos_max_slope;
	float time_remaining = dt;
	bool ran = false;
	for (uint32_t it = 0; it < rc->max_coll_it && time_remaining >= rc->min_time; ++it) {
		char_contacts(d, L, S, rc, ignore, pos, velocity);
		ran = true;
		if (lane == 0) {
			uint32_t nk = 0, ns = S.n_seen, na = S.n_added;
			for (uint32_t i = 0; i < S.n_cur; ++i) {
				const CharContact& c = S.cur[i];
				if (notify) {
					bool found = false;
					for (uint32_t j = 0; j < ns; ++j) if (S.seen[j] == c.body) found = true;
					if (!found) {
						if (ns < SGP_CHAR_MAX_SEEN) S.seen[ns++] = c.body; else S.overflow |= 2u;
						if (na < SGP_CHAR_MAX_ADDED) {
							CharAdded a; a.body = c.body; a.pad_ = 0; a.p[0] = c.p[0]; a.p[1] = c.p[1]; a.p[2] = c.p[2]; a.n[0] = c.n[0]; a.n[1] = c.n[1]; a.n[2] = c.n[2];
							b.added[(size_t)k * SGP_CHAR_MAX_ADDED + na++] = a;
						} else S.overflow |= 2u;
					}
				}
				if (c.bits & 1u) continue;      // sensor
				const v3 cn = ch_v3(c.n), cv = ch_v3(c.v);
				CharCons q; q.n = cn; q.vel = cv; q.dist = c.dist; q.contact = (int)i; q.steep = 0;
				if (c.dist < 0.0f) q.vel = v3_add(q.vel, v3_scale(cn, -c.dist * rc->recovery / dt));      // push out of penetration
				const float nu = v3_dot(cn, up);
				q.steep = (nu > 1.0e-3f && nu < cos_max_slope) ? 1 : 0;
				S.k[nk++] = q;
				if (q.steep) {
					const v3 h = v3_sub(cn, v3_scale(up, nu));
					const float hl = sqrtf(v3_len_sq(h));
					if (hl > 1.0e-6f) { CharCons w; w.n = v3_scale(h, 1.0f / hl); w.vel = v3_scale(w.n, v3_dot(cv, w.n)); w.dist = c.dist / hl; w.contact = (int)i; w.steep = 0; S.k[nk++] = w; }
				}
			}
			S.n_k = nk; S.n_seen = ns; S.n_added = na;
		}
		__syncthreads();
		// solveConstraints(velocity, time_remaining): every lane alike
		const float time = time_remaining;
		const uint32_t nk = S.n_k;
		v3 vel = velocity, displacement = V3(0.0f, 0.0f, 0.0f);
		float t_left = time;
		int previous = -1;
		for (uint32_t ci = 0; ci < rc->max_cons_it && t_left > 0.0f; ++ci) {
			float best_toi = t_left; int hit = -1;
			for (uint32_t i = 0; i < nk; ++i) {
				const v3 cn = S.k[i].n, cvel = S.k[i].vel;
				const float vn = v3_dot(v3_sub(vel, cvel), cn);
				if (vn >= -1.0e-6f) continue;
				const float dist = S.k[i].dist + v3_dot(displacement, cn) - v3_dot(cvel, cn) * (time - t_left);
				const float toi = ch_max(0.0f, dist) / -vn;
				if (toi < best_toi) { best_toi = toi; hit = (int)i; }
			}
			displacement = v3_add(displacement, v3_scale(vel, best_toi));
			t_left -= best_toi;
			if (hit < 0) break;
			const v3 hn = S.k[hit].n, hv = S.k[hit].vel;
			if (S.k[hit].steep) {
				const v3 vpn = v3_sub(hn, v3_scale(up, v3_dot(hn, up)));
				const float towards = ch_min(0.0f, v3_dot(v3_sub(vel, hv), vpn));
				vel = v3_sub(vel, v3_scale(vpn, towards / v3_len_sq(vpn)));
			}
			const v3 rel = v3_sub(vel, hv);
			v3 new_vel = v3_sub(vel, v3_scale(hn, v3_dot(rel, hn)));
			{
				// pushBody(contact, rel, time)
				const CharContact& c = S.cur[S.k[hit].contact];
				if ((c.bits & 2u) && !(c.inv_mass <= 0.0f) && !(time <= 0.0f)) {
					const v3 cn = ch_v3(c.n);
					const float vn = -v3_dot(rel, cn);
					if (!(vn <= 0.0f)) {
						const float impulse = ch_min(rc->mass * vn, rc->max_strength * time);
						const v3 f = v3_scale(cn, -impulse / time);
						const uint32_t np = S.n_push;
						// (these barriers sit inside conditions: safe only because every condition up to here is computed by all 64 lanes from the same LDS and
						// record values -- wave-uniform by construction.  Nothing lane-dependent may ever decide a branch that holds a barrier: the workgroup would hang.)
						__syncthreads();
						if (lane == 0) {
							if (np < SGP_CHAR_MAX_PUSHES) {
								CharPush p; p.body = c.body; p.f[0] = f.x; p.f[1] = f.y; p.f[2] = f.z; p.p[0] = c.p[0]; p.p[1] = c.p[1]; p.p[2] = c.p[2]; p.pad_ = 0;
								b.push[(size_t)k * SGP_CHAR_MAX_PUSHES + np] = p; S.n_push = np + 1;
							} else S.overflow |= 2u;
						}
						__syncthreads();
					}
				}
				// OnContactSolve: PlayerPhysics' anti-sliding rule
				if (no_slide && v3_len_sq(hv) <= 1.0e-12f && !char_too_steep(rc, hn)) new_vel = V3(0.0f, 0.0f, 0.0f);
			}
			if (previous >= 0 && previous != hit && v3_dot(v3_sub(new_vel, S.k[previous].vel), S.k[previous].n) < -1.0e-6f) {
				v3 dir = v3_cross(hn, S.k[previous].n);
				const float l2 = v3_len_sq(dir);
				if (l2 > 1.0e-8f) { dir = v3_scale(dir, 1.0f / sqrtf(l2)); new_vel = v3_scale(dir, v3_dot(vel, dir)); }
				else new_vel = V3(0.0f, 0.0f, 0.0f);
				for (uint32_t i = 0; i < nk; ++i) if ((int)i != hit && (int)i != previous && S.k[i].dist + v3_dot(displacement, S.k[i].n) < 1.0e-3f && v3_dot(v3_sub(new_vel, S.k[i].vel), S.k[i].n) < -1.0e-6f) { new_vel = V3(0.0f, 0.0f, 0.0f); break; }
			}
			previous = hit;
			vel = new_vel;
			if (v3_len_sq(vel) < 1.0e-12f) break;
		}
		float time_simulated = time - ch_max(0.0f, t_left);
		if (v3_len_sq(vel) < 1.0e-12f) time_simulated = time;
		displacement = v3_scale(displacement, char_sweep_fraction(d, rc, pos, displacement, ignore));
		pos = v3_add(pos, displacement);
		time_remaining -= ch_max(time_simulated, rc->min_time);
		if (v3_len_sq(displacement) < 1.0e-10f) break;
	}
	if (notify) {
		// the pairs already reported are those of the last contacts
		__syncthreads();
		if (lane == 0) {
			uint32_t ns = 0;
			const uint32_t n = ran ? S.n_cur : 0u;
			for (uint32_t i = 0; i < n; ++i) { bool found = false; for (uint32_t j = 0; j < ns; ++j) if (S.seen[j] == S.cur[i].body) found = true; if (!found) S.seen[ns++] = S.cur[i].body; }
			S.n_seen = ns;
		}
		__syncthreads();
	}
	return pos;
}

// CharacterVirtual::updateSupportingContact(S.cur, store): the ground of the character at `position`.  store = false is UpdateGroundVelocity's call: the active
// contacts stay those of the previous update, which CancelVelocityTowardsSteepSlopes and CanWalkStairs of the update that follows read.
SGP_DEV CharGround char_supporting_contact(CharLds& S, const CharRec* rc, v3 position, v3 previous_ground_position, bool store = true)
{
	const uint32_t lane = threadIdx.x;
	const v3 up = ch_v3(rc->up), svn = ch_v3(rc->sv_n);
	const uint32_t n = S.n_cur;
	if (store) {
		__syncthreads();
		if (lane < n) S.act[lane] = S.cur[lane];
		if (lane == 0) S.n_act = n;
		__syncthreads();
	}
	int best = -1; bool best_steep = true; float best_up = -2.0f; bool touching = false;
	for (uint32_t i = 0; i < n; ++i) {
		const CharContact& c = S.cur[i];
		if ((c.bits & 1u) || c.dist > rc->tolerance + 0.01f) continue;
		touching = true;
		const float nu = v3_dot(ch_v3(c.n), up);
		if (nu <= 0.0f) continue;
		const v3 rel = v3_sub(ch_v3(c.p), position);
		if (svn.x * rel.x + svn.y * rel.y + svn.z * rel.z + rc->sv_c > 0.0f) continue;
		const bool steep = nu < rc->cos_max_slope;
		if (best < 0 || (best_steep && !steep) || (steep == best_steep && nu > best_up)) { best = (int)i; best_steep = steep; best_up = nu; }
	}
	CharGround g;
	if (best >= 0) {
		const CharContact& c = S.cur[best];
		g.state = best_steep ? SGP_GROUND_ON_STEEP_GROUND : SGP_GROUND_ON_GROUND;
		g.n = ch_v3(c.n); g.v = ch_v3(c.v); g.p = ch_v3(c.p); g.body = c.body;
	} else {
		g.state = touching ? SGP_GROUND_NOT_SUPPORTED : SGP_GROUND_IN_AIR;
		g.n = V3(0.0f, 0.0f, 0.0f); g.v = V3(0.0f, 0.0f, 0.0f); g.p = previous_ground_position; g.body = SGP_INVALID_ID;      // (the host class leaves the ground position as it was)
	}
	return g;
}
