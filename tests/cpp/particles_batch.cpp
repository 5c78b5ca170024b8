// A ParticleManager-shaped caller twice over: the manager's host loop (ParticleManager.cpp:145-274) over the batched facade extension traceRays(), and a
// ParticleBatch (shim/ParticleBatch.h) fed the same 300 particles, on the scene of particle_rays.cpp, for 20 frames.  Both sides are printed as one JSON
// document -- per frame the live tags in order, positions, velocities, widths, opacities and the events -- for tests/test_particles_gpu.py to compare.  The
// host loop removes its dead in order (the batch's stable compaction; docs/GAPS.md) and writes every expression as docs/CONTRACT.md ("Particles") does.
#include "PhysicsWorld.h"
#include "ParticleBatch.h"
#include <utils/Exception.h>
#include <cmath>
#include <cstdio>
#include <string>
#include <vector>

static uint32_t rng_state = 12345u;
static float unitRandom() { rng_state = rng_state * 1664525u + 1013904223u; return (float)(rng_state >> 8) * (1.f / 16777216.f); }

struct Event { uint64_t tag; uint32_t kind; };

static void hostThink(PhysicsWorld& world, std::vector<Particle>& particles, float dt, std::vector<Event>& events, size_t& hits)
{
	const size_t n = particles.size();
	std::vector<PhysicsWorld::RayQuery> qs(n); std::vector<RayTraceResult> rs;
	for (size_t i = 0; i < n; ++i) { qs[i].origin = particles[i].pos; qs[i].dir = particles[i].vel; qs[i].max_t = dt; qs[i].ignore_body_id = JPH::BodyID(); qs[i].collidable_only = false; }
	if (n) world.traceRays(qs, rs);
	std::vector<Particle> kept;
	for (size_t i = 0; i < n; ++i) {
		Particle p = particles[i];
		float pos[3] = { p.pos[0], p.pos[1], p.pos[2] }, vel[3] = { p.vel[0], p.vel[1], p.vel[2] };
		if (rs[i].hit_object) {
			++hits;
			const float t = rs[i].hit_t;
			const float nn[3] = { rs[i].hit_normal_ws[0], rs[i].hit_normal_ws[1], rs[i].hit_normal_ws[2] };
			float hitpos[3];
			for (int k = 0; k < 3; ++k) hitpos[k] = pos[k] + vel[k] * t;
			const float s = 2.f * ((nn[0] * vel[0] + nn[1] * vel[1]) + nn[2] * vel[2]);
			for (int k = 0; k < 3; ++k) vel[k] = vel[k] - nn[k] * s;
			for (int k = 0; k < 3; ++k) vel[k] = vel[k] * p.restitution;
			const float rem = dt - t;
			for (int k = 0; k < 3; ++k) pos[k] = (hitpos[k] + nn[k] * 1.0e-3f) + vel[k] * rem;
			if (p.die_when_hit_surface) p.cur_opacity = -1.f;
		} else {
			for (int k = 0; k < 3; ++k) pos[k] = pos[k] + vel[k] * dt;
			vel[2] = vel[2] - 9.81f * dt;      // (no water in this scene)
		}
		const float v2 = (vel[0] * vel[0] + vel[1] * vel[1]) + vel[2] * vel[2];
		if (v2 > 1.0e-3f * 1.0e-3f) {
			const float F = (((0.5f * 1.293f) * v2) * 0.5f) * p.area;
			const float a = std::fmin(10.f, F / p.mass);
			const float f = std::fmax(0.f, 1.f - (a * dt) / std::sqrt(v2));
			for (int k = 0; k < 3; ++k) vel[k] = vel[k] * f;
		}
		p.cur_opacity = p.cur_opacity + p.dopacity_dt * dt;
		p.width = p.width + p.dwidth_dt * dt;
		p.pos = Vec4f(pos[0], pos[1], pos[2], 1); p.vel = Vec4f(vel[0], vel[1], vel[2], 0);
		if (p.cur_opacity <= 0) events.push_back(Event{ p.tag, SGP_PARTICLE_EV_DIED });
		else kept.push_back(p);
	}
	particles.swap(kept);
}

template <typename T, typename F> static void printList(const char* name, const std::vector<T>& v, F one, const char* tail)
{
	printf("\"%s\": [", name);
	for (size_t i = 0; i < v.size(); ++i) { if (i) printf(", "); one(v[i]); }
	printf("]%s", tail);
}

int main()
{
	try {
		PhysicsWorld::init();
		Reference<PhysicsWorld> world = new PhysicsWorld(nullptr, nullptr);
		Reference<PhysicsObject> ground = new PhysicsObject(true, PhysicsWorld::createGroundQuadShape(2000.f), nullptr, 0);
		ground->pos = Vec4f(0, 0, -0.5f, 1);
		world->addObject(ground);
		std::vector<Reference<PhysicsObject>> obs;
		for (int i = 0; i < 200; ++i) {      // things for the particles to hit (particle_rays.cpp)
			Reference<PhysicsObject> ob = new PhysicsObject(true);
			if (i % 2) ob->is_sphere = true; else ob->is_cube = true;
			ob->scale = Vec3f(0.5f + unitRandom()); ob->mass = 10.f; ob->motion_type = PhysicsObject::MotionType_dynamic;
			ob->pos = Vec4f(-15.f + 30.f * unitRandom(), -15.f + 30.f * unitRandom(), 0.6f + 2.f * unitRandom(), 1);
			world->addObject(ob); world->activateObject(ob); obs.push_back(ob);
		}
		for (int s = 0; s < 120; ++s) world->think(1.0 / 60.0);

		const size_t N = 300;
		std::vector<Particle> host(N);
		for (size_t i = 0; i < N; ++i) {
			Particle& p = host[i];
			p.pos = Vec4f(-15.f + 30.f * unitRandom(), -15.f + 30.f * unitRandom(), 0.3f + 4.f * unitRandom(), 1);
			p.vel = Vec4f(-6.f + 12.f * unitRandom(), -6.f + 12.f * unitRandom(), -8.f * unitRandom(), 0);
			p.tag = 1000 + i;
			p.restitution = 0.2f + 0.7f * unitRandom();
			p.area = 1.0e-6f * (0.5f + 4.f * unitRandom()); p.mass = 1.0e-6f * (0.5f + 2.f * unitRandom());
			p.dopacity_dt = -0.3f - 3.7f * unitRandom();
			p.die_when_hit_surface = (i % 5) == 0;
		}
		ParticleBatch batch(world->physics_system, 512, 4096);
		for (const Particle& p : host) batch.addParticle(p);

		const float dt = 1.f / 60.f;
		size_t hits = 0;
		printf("{\"frames\": [\n");
		for (int frame = 0; frame < 20; ++frame) {
			std::vector<Event> host_events;
			hostThink(*world, host, dt, host_events, hits);
			batch.think(dt);
			batch.readBack();
			printf("{\"host\": {");
			printList("tags", host, [](const Particle& p) { printf("%llu", (unsigned long long)p.tag); }, ", ");
			printList("state", host, [](const Particle& p) { printf("[%.9g, %.9g, %.9g, %.9g, %.9g, %.9g, %.9g, %.9g]", p.pos[0], p.pos[1], p.pos[2], p.vel[0], p.vel[1], p.vel[2], p.width, p.cur_opacity); }, ", ");
			printList("events", host_events, [](const Event& e) { printf("[%llu, %u]", (unsigned long long)e.tag, e.kind); }, "}, ");
			printf("\"batch\": {");
			printList("tags", batch.live(), [](const sgp_particle_state& s) { printf("%llu", (unsigned long long)s.tag); }, ", ");
			printList("state", batch.live(), [](const sgp_particle_state& s) { printf("[%.9g, %.9g, %.9g, %.9g, %.9g, %.9g, %.9g, %.9g]", s.pos[0], s.pos[1], s.pos[2], s.vel[0], s.vel[1], s.vel[2], s.width, s.opacity); }, ", ");
			printList("events", batch.events(), [](const sgp_particle_event& e) { printf("[%llu, %u]", (unsigned long long)e.tag, e.kind); }, "}}");
			printf(frame + 1 < 20 ? ",\n" : "\n");
		}
		printf("], \"hits\": %zu, \"events_dropped\": %u}\n", hits, batch.eventsDropped());
		return 0;
	} catch (glare::Exception& e) { fprintf(stderr, "glare::Exception: %s\n", e.what().c_str()); return 2; }
	catch (std::exception& e) { fprintf(stderr, "exception: %s\n", e.what()); return 3; }
}
