// What a frame of particles costs, two ways, in one process on one device (driven by particles_cost.py, which writes config 3's body descriptions to argv[1]):
//  1. on the scene of tests/cpp/particle_rays.cpp, 2048 particles: ParticleManager's host loop over the batched facade extension traceRays() (one upload of the
//     rays, one launch, one download of the hits, a wait, the arithmetic on the host) against ParticleBatch (think + readBack: three launches, one download of the
//     live states, one wait).  The particles neither fade nor die on a hit, so both sides carry 2048 through every frame.  Per frame: wall clock around the whole
//     frame, and HIP events on the world's stream around what the frame puts on it.
//  2. over config 3's settled pile, through the C ABI: sgp_particles_update for 65 536 and 1 048 576 particles (HIP events), and the world's steps per second
//     with and without a 65 536-particle update behind every step.
// Medians after a warm-up; nothing is tuned for either side.
#include "PhysicsWorld.h"
#include "ParticleBatch.h"
#include <utils/Exception.h>
#include <hip/hip_runtime_api.h>
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

static uint32_t rng_state = 12345u;
static float unitRandom() { rng_state = rng_state * 1664525u + 1013904223u; return (float)(rng_state >> 8) * (1.f / 16777216.f); }
static double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
static double median(std::vector<double> v) { std::sort(v.begin(), v.end()); return v.empty() ? 0.0 : v[v.size() / 2]; }
#define HIP_OK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); exit(4); } } while (0)
#define SGP_OK_(x) do { if ((x) != SGP_OK) { fprintf(stderr, "%s: %s\n", #x, sgp_last_error()); exit(5); } } while (0)

// ParticleManager::think (ParticleManager.cpp:145-274) over traceRays(); no water in these scenes, nobody dies
static void hostThink(PhysicsWorld& world, std::vector<Particle>& particles, float dt)
{
	const size_t n = particles.size();
	std::vector<PhysicsWorld::RayQuery> qs(n); std::vector<RayTraceResult> rs;
	for (size_t i = 0; i < n; ++i) { qs[i].origin = particles[i].pos; qs[i].dir = particles[i].vel; qs[i].max_t = dt; qs[i].ignore_body_id = JPH::BodyID(); qs[i].collidable_only = false; }
	world.traceRays(qs, rs);
	size_t kept = 0;
	for (size_t i = 0; i < n; ++i) {
		Particle p = particles[i];
		float pos[3] = { p.pos[0], p.pos[1], p.pos[2] }, vel[3] = { p.vel[0], p.vel[1], p.vel[2] };
		if (rs[i].hit_object) {
			const float t = rs[i].hit_t;
			const float nn[3] = { rs[i].hit_normal_ws[0], rs[i].hit_normal_ws[1], rs[i].hit_normal_ws[2] };
			float hitpos[3];
			for (int k = 0; k < 3; ++k) hitpos[k] = pos[k] + vel[k] * t;
			const float s = 2.f * ((nn[0] * vel[0] + nn[1] * vel[1]) + nn[2] * vel[2]);
			for (int k = 0; k < 3; ++k) vel[k] = (vel[k] - nn[k] * s) * p.restitution;
			const float rem = dt - t;
			for (int k = 0; k < 3; ++k) pos[k] = (hitpos[k] + nn[k] * 1.0e-3f) + vel[k] * rem;
			if (p.die_when_hit_surface) p.cur_opacity = -1.f;
		} else {
			for (int k = 0; k < 3; ++k) pos[k] = pos[k] + vel[k] * dt;
			vel[2] = vel[2] - 9.81f * dt;
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
		if (!(p.cur_opacity <= 0)) particles[kept++] = p;      // (in order)
	}
	particles.resize(kept);
}

struct Timer {
	hipStream_t s; hipEvent_t a, b;
	explicit Timer(sgp_world* w) { void* p = nullptr; SGP_OK_(sgp_world_stream(w, &p)); s = (hipStream_t)p; HIP_OK(hipEventCreate(&a)); HIP_OK(hipEventCreate(&b)); }
	~Timer() { (void)hipEventDestroy(a); (void)hipEventDestroy(b); }
	void begin() { HIP_OK(hipEventRecord(a, s)); }
	void end() { HIP_OK(hipEventRecord(b, s)); }
	double ms() { HIP_OK(hipEventSynchronize(b)); float t = 0; HIP_OK(hipEventElapsedTime(&t, a, b)); return (double)t; }
};

static void frameCost(int frames)
{
	Reference<PhysicsWorld> world = new PhysicsWorld(nullptr, nullptr);
	Reference<PhysicsObject> ground = new PhysicsObject(true, PhysicsWorld::createGroundQuadShape(2000.f), nullptr, 0);
	ground->pos = Vec4f(0, 0, -0.5f, 1);
	world->addObject(ground);
	std::vector<Reference<PhysicsObject>> obs;
	for (int i = 0; i < 200; ++i) {
		Reference<PhysicsObject> ob = new PhysicsObject(true);
		if (i % 2) ob->is_sphere = true; else ob->is_cube = true;
		ob->scale = Vec3f(0.5f + unitRandom()); ob->mass = 10.f; ob->motion_type = PhysicsObject::MotionType_dynamic;
		ob->pos = Vec4f(-15.f + 30.f * unitRandom(), -15.f + 30.f * unitRandom(), 0.6f + 2.f * unitRandom(), 1);
		world->addObject(ob); world->activateObject(ob); obs.push_back(ob);
	}
	for (int s = 0; s < 120; ++s) world->think(1.0 / 60.0);
	const size_t N = 2048;
	std::vector<Particle> host(N);
	for (size_t i = 0; i < N; ++i) {
		Particle& p = host[i];
		p.pos = Vec4f(-15.f + 30.f * unitRandom(), -15.f + 30.f * unitRandom(), 0.3f + 4.f * unitRandom(), 1);
		p.vel = Vec4f(-6.f + 12.f * unitRandom(), -6.f + 12.f * unitRandom(), -8.f * unitRandom(), 0);
		p.tag = i; p.dopacity_dt = 0.f; p.dwidth_dt = 0.f;
	}
	ParticleBatch batch(world->physics_system, (uint32_t)N, 64);
	for (const Particle& p : host) batch.addParticle(p);
	batch.flush();
	Timer tm(world->world);
	const float dt = 1.f / 60.f;
	const int warm = 10;
	std::vector<double> wall_h, dev_h, wall_b, dev_b;
	for (int fr = 0; fr < warm + frames; ++fr) {
		double t0 = now_ms();
		tm.begin(); hostThink(*world, host, dt); tm.end();
		double t1 = now_ms();
		const double dh = tm.ms();
		double t2 = now_ms();
		tm.begin(); batch.think(dt); tm.end(); batch.readBack();
		double t3 = now_ms();
		const double db = tm.ms();
		if (fr >= warm) { wall_h.push_back(t1 - t0); dev_h.push_back(dh); wall_b.push_back(t3 - t2); dev_b.push_back(db); }
	}
	bool same = host.size() == batch.live().size();
	for (size_t i = 0; i < host.size() && same; ++i) for (int k = 0; k < 3; ++k) same = same && host[i].pos[k] == batch.live()[i].pos[k] && host[i].vel[k] == batch.live()[i].vel[k];
	printf("## 2048 particles on the scene of particle_rays.cpp, %d frames (median per frame; both sides end with identical particles: %d)\n", frames, (int)same);
	printf("| path | wall clock, ms per frame | device time between the events, ms per frame |\n|---|---|---|\n");
	printf("| host loop over batched traceRays (upload, launch, download, wait, arithmetic on the host) | %.3f | %.3f |\n", median(wall_h), median(dev_h));
	printf("| ParticleBatch: think + readBack (events around think: update, scan, scatter) | %.3f | %.3f |\n", median(wall_b), median(dev_b));
	fflush(stdout);
}

static void fill(std::vector<sgp_particle>& p, size_t n)
{
	p.resize(n);
	for (size_t i = 0; i < n; ++i) {
		sgp_default_particle(&p[i]);
		p[i].pos[0] = -75.f + 150.f * unitRandom(); p[i].pos[1] = -75.f + 150.f * unitRandom(); p[i].pos[2] = 0.2f + 12.f * unitRandom();
		p[i].vel[0] = -6.f + 12.f * unitRandom(); p[i].vel[1] = -6.f + 12.f * unitRandom(); p[i].vel[2] = -8.f * unitRandom();
		p[i].dopacity_dt = 0.f; p[i].dwidth_dt = 0.f; p[i].tag = i;
	}
}

static void pileCost(const char* descs_path, int frames)
{
	FILE* f = fopen(descs_path, "rb"); if (!f) exit(2);
	fseek(f, 0, SEEK_END); const size_t bytes = (size_t)ftell(f); fseek(f, 0, SEEK_SET);
	std::vector<sgp_body_desc> descs(bytes / sizeof(sgp_body_desc));
	if (fread(descs.data(), sizeof(sgp_body_desc), descs.size(), f) != descs.size()) exit(2);
	fclose(f);
	sgp_world_desc wd; sgp_default_world_desc(&wd); wd.max_bodies = (uint32_t)descs.size() + 1024;
	sgp_world* world = nullptr;
	SGP_OK_(sgp_world_create(&wd, &world));
	std::vector<uint32_t> ids(descs.size());
	SGP_OK_(sgp_body_add_batch(world, descs.data(), (uint32_t)descs.size(), ids.data()));
	for (int s = 0; s < 240; ++s) sgp_world_step(world, 1.f / 60.f);      // let the pile settle a little (tools/experiments/characters_bench.cpp)
	const float dt = 1.f / 60.f;
	const int warm = 5;
	printf("## over config 3's pile after 240 steps (median of %d updates)\n| particles | sgp_particles_update, ms (HIP events) | particles per second |\n|---|---|---|\n", frames);
	const size_t Ns[2] = { 65536, 1048576 };
	for (size_t N : Ns) {
		sgp_particles* ps = nullptr;
		SGP_OK_(sgp_particles_create(world, (uint32_t)N, 64, &ps));
		std::vector<sgp_particle> p; fill(p, N);
		SGP_OK_(sgp_particles_add(ps, p.data(), (uint32_t)N));
		Timer tm(world);
		std::vector<double> t;
		for (int fr = 0; fr < warm + frames; ++fr) {
			tm.begin(); SGP_OK_(sgp_particles_update(ps, dt)); tm.end();
			const double ms = tm.ms();
			if (fr >= warm) t.push_back(ms);
		}
		uint32_t live = 0;
		SGP_OK_(sgp_particles_read(ps, nullptr, 0, &live));
		printf("| %zu (%u live at the end) | %.3f | %.3g |\n", N, live, median(t), (double)N / (median(t) * 1.0e-3));
		fflush(stdout);
		SGP_OK_(sgp_particles_destroy(ps));
	}
	// the step with and without particles behind it (the update is enqueued behind the step and the next step queues behind it: one stream)
	sgp_particles* ps = nullptr;
	SGP_OK_(sgp_particles_create(world, 65536, 64, &ps));
	std::vector<sgp_particle> p; fill(p, 65536);
	SGP_OK_(sgp_particles_add(ps, p.data(), 65536));
	const int steps = 200;
	double rate[2] = { 0, 0 };
	for (int pass = 0; pass < 4; ++pass) {      // without, with, without, with: the later pair is reported
		const bool with = pass & 1;
		for (int s = 0; s < 20; ++s) { sgp_world_step(world, dt); if (with) SGP_OK_(sgp_particles_update(ps, dt)); }
		const double t0 = now_ms();
		for (int s = 0; s < steps; ++s) { sgp_world_step(world, dt); if (with) SGP_OK_(sgp_particles_update(ps, dt)); }
		uint32_t live = 0;
		if (with) SGP_OK_(sgp_particles_read(ps, nullptr, 0, &live));      // (waits for the last update)
		rate[with] = steps / ((now_ms() - t0) * 1.0e-3);
	}
	printf("## config 3, %d steps: %.1f steps/s alone, %.1f steps/s with a 65 536-particle update behind every step\n", steps, rate[0], rate[1]);
	SGP_OK_(sgp_particles_destroy(ps));
	sgp_world_destroy(world);
}

int main(int argc, char** argv)
{
	if (argc < 2) return 2;
	const int frames = argc > 2 ? atoi(argv[2]) : 200;
	try {
		PhysicsWorld::init();
		frameCost(frames);
		pileCost(argv[1], std::min(frames, 50));
		return 0;
	} catch (glare::Exception& e) { fprintf(stderr, "glare::Exception: %s\n", e.what().c_str()); return 2; }
	catch (std::exception& e) { fprintf(stderr, "exception: %s\n", e.what()); return 3; }
}
