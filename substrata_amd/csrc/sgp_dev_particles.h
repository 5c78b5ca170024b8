// sgp_dev_particles.h -- one particle through ParticleManager::think (gui_client/ParticleManager.cpp:145-274), for k_particles_update.
// Needs sgp_dev_all.h and sgp_dev_raycast.h in front of it.  The expressions are the reference's, in fp32, in its order, term by term as docs/CONTRACT.md
// ("Particles") writes them out; the build does not contract a * b + c, so the host restatement of the tests computes the same bits.
#pragma once

// A: pos xyz, width.  B: vel xyz, opacity.  c0: area, mass, restitution, dwidth_dt.  Returns the event word (SGP_PARTICLE_EV_DIED | _FOAM), *foam_w = the decal's width.
SGP_DEV uint32_t particle_think(const DV& d, float4& A, float4& B, float4 c0, float dopacity_dt, uint32_t flags, float dt, int water_enabled, float water_z, float* foam_w)
{
	v3 pos = V3(A.x, A.y, A.z), vel = V3(B.x, B.y, B.z);
	float width = A.w, opacity = B.w;
	const float area = c0.x, mass = c0.y, restitution = c0.z, dwidth_dt = c0.w;
	const bool die_on_hit = (flags & SGP_PARTICLE_DIE_ON_HIT) != 0u;
	uint32_t word = 0u;
	*foam_w = 0.0f;
	// :164 traceRay(pos, vel, dt, no ignored body): the direction is the velocity as it is, so t is a time
	sgp_ray ry;
	ry.origin[0] = pos.x; ry.origin[1] = pos.y; ry.origin[2] = pos.z;
	ry.dir[0] = vel.x; ry.dir[1] = vel.y; ry.dir[2] = vel.z;
	ry.max_t = dt; ry.ignore_id = SGP_INVALID_ID; ry.collidable_only = 0u;
	const sgp_hit h = raycast_one(d, ry);
	if (h.id != SGP_INVALID_ID) {
		// :167-191
		const float to_hit = h.t;
		const v3 n = V3(h.normal[0], h.normal[1], h.normal[2]);
		const v3 hitpos = V3(pos.x + vel.x * to_hit, pos.y + vel.y * to_hit, pos.z + vel.z * to_hit);
		const float s = 2.0f * ((n.x * vel.x + n.y * vel.y) + n.z * vel.z);
		vel = V3(vel.x - n.x * s, vel.y - n.y * s, vel.z - n.z * s);
		vel = V3(vel.x * restitution, vel.y * restitution, vel.z * restitution);
		const float rem = dt - to_hit;
		pos = V3((hitpos.x + n.x * 1.0e-3f) + vel.x * rem, (hitpos.y + n.y * 1.0e-3f) + vel.y * rem, (hitpos.z + n.z * 1.0e-3f) + vel.z * rem);
		if (die_on_hit) opacity = -1.0f;
	} else {
		// :194-212
		pos = V3(pos.x + vel.x * dt, pos.y + vel.y * dt, pos.z + vel.z * dt);
		if (water_enabled && pos.z < water_z) {
			if (die_on_hit && vel.z < 0.0f) { opacity = -1.0f; word |= SGP_PARTICLE_EV_FOAM; *foam_w = width; }
			vel.z = fmaxf(vel.z, 0.5f);
		}
		else vel.z = vel.z - 9.81f * dt;
	}
	// :218-242 wind resistance
	const float v2 = (vel.x * vel.x + vel.y * vel.y) + vel.z * vel.z;
	if (v2 > 1.0e-3f * 1.0e-3f) {
		const float F = (((0.5f * 1.293f) * v2) * 0.5f) * area;
		const float a = fminf(10.0f, F / mass);
		const float f = fmaxf(0.0f, 1.0f - (a * dt) / sqrtf(v2));
		vel = V3(vel.x * f, vel.y * f, vel.z * f);
	}
	// :247-248, :259
	opacity = opacity + dopacity_dt * dt;
	width = width + dwidth_dt * dt;
	if (opacity <= 0.0f) word |= SGP_PARTICLE_EV_DIED;
	A = make_float4(pos.x, pos.y, pos.z, width);
	B = make_float4(vel.x, vel.y, vel.z, opacity);
	return word;
}
