// Time per frame of N characters walking on the ground around the settled config-3 pile: the batch (CharacterBatch: update + read-back) against the host walk
// (N JPH::CharacterVirtual of Jolt/JoltCharacterLite.h, one after the other through sgp_collide_capsules / sgp_spherecast).  Driven by characters_bench.py, which
// writes the pile's body descriptions to the file named in argv[1].
#include "../../include/sgp.h"
static unsigned long g_round_trips = 0;      // blocking queries of the host walk
static int counted_collide_capsules(sgp_world* w, const sgp_capsule_query* q, uint32_t n, sgp_query_contact* out, uint32_t cap, uint32_t* n_out) { ++g_round_trips; return sgp_collide_capsules(w, q, n, out, cap, n_out); }
static int counted_spherecast(sgp_world* w, const sgp_ray* rays, const float* radii, uint32_t n, sgp_hit* hits) { ++g_round_trips; return sgp_spherecast(w, rays, radii, n, hits); }
#define sgp_collide_capsules counted_collide_capsules
#define sgp_spherecast counted_spherecast
#include "CharacterBatch.h"
#undef sgp_collide_capsules
#undef sgp_spherecast
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

static const float DT = 1.f / 60.f;
static double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
static double median(std::vector<double> v) { std::sort(v.begin(), v.end()); return v[v.size() / 2]; }

static JPH::Vec3 startOf(int i)
{
	const float along = -74.f + 0.58f * (float)(i / 4), off = 76.3f;      // a ring just outside the pile's footprint (+-75 m)
	switch (i % 4) { case 0: return JPH::Vec3(along, -off, 0.02f); case 1: return JPH::Vec3(off, along, 0.02f); case 2: return JPH::Vec3(-along, off, 0.02f); default: return JPH::Vec3(-off, -along, 0.02f); }
}
static JPH::Vec3 wishOf(int i) { switch (i % 4) { case 0: return JPH::Vec3(2, 0, 0); case 1: return JPH::Vec3(0, 2, 0); case 2: return JPH::Vec3(-2, 0, 0); default: return JPH::Vec3(0, -2, 0); } }
static JPH::Vec3 velocityFor(const JPH::Vec3& desired, const JPH::Vec3& vel, bool supported, const JPH::Vec3& ground_vel) { return (supported ? desired + ground_vel : vel) + JPH::Vec3(0, 0, -9.81f) * DT; }

int main(int argc, char** argv)
{
	if (argc < 2) return 2;
	FILE* f = fopen(argv[1], "rb"); if (!f) return 2;
	fseek(f, 0, SEEK_END); const size_t bytes = (size_t)ftell(f); fseek(f, 0, SEEK_SET);
	std::vector<sgp_body_desc> descs(bytes / sizeof(sgp_body_desc));
	if (fread(descs.data(), sizeof(sgp_body_desc), descs.size(), f) != descs.size()) return 2;
	fclose(f);
	const int frames = argc > 2 ? atoi(argv[2]) : 30, warm = 5;
	if (sgp_init() < 1) { fprintf(stderr, "%s\n", sgp_last_error()); return 3; }
	sgp_world_desc wd; sgp_default_world_desc(&wd); wd.max_bodies = (uint32_t)descs.size() + 1024;
	sgp_world* world = nullptr;
	if (sgp_world_create(&wd, &world) != SGP_OK) { fprintf(stderr, "%s\n", sgp_last_error()); return 3; }
	std::vector<uint32_t> ids(descs.size());
	if (sgp_body_add_batch(world, descs.data(), (uint32_t)descs.size(), ids.data()) != SGP_OK) { fprintf(stderr, "%s\n", sgp_last_error()); return 3; }
	for (int s = 0; s < 240; ++s) sgp_world_step(world, DT);      // let the pile settle a little
	JPH::PhysicsSystem system(world);
	JPH::CharRef<JPH::CharacterShape> shape = JPH::RotatedTranslatedShapeSettings(JPH::Vec3(0, 0, 0.95f), JPH::Quat(0.7071068f, 0, 0, 0.7071068f), new JPH::CapsuleShape(0.65f, 0.3f)).Create().Get();
	JPH::CharRef<JPH::CharacterVirtualSettings> settings = new JPH::CharacterVirtualSettings();
	settings->mShape = shape; settings->mUp = JPH::Vec3(0, 0, 1); settings->mSupportingVolume = JPH::Plane(JPH::Vec3(0, 0, 1), -0.3f); settings->mMaxStrength = 1000;
	JPH::CharacterVirtual::ExtendedUpdateSettings ext; ext.mStickToFloorStepDown = JPH::Vec3(0, 0, -0.5f); ext.mWalkStairsStepUp = JPH::Vec3(0, 0, 0.4f);
	printf("| N | host walk, ms per frame | round trips per update | batch (update + get_states), ms per frame | ratio |\n|---|---|---|---|---|\n");
	const int Ns[3] = { 1, 64, 1024 };
	for (int N : Ns) {
		// host walk
		std::vector<std::unique_ptr<JPH::CharacterVirtual>> chars;
		for (int i = 0; i < N; ++i) chars.emplace_back(new JPH::CharacterVirtual(settings, startOf(i), JPH::Quat(), &system));
		JPH::TempAllocator ta; const JPH::ShapeFilter sf; const JPH::BodyFilter bf; const JPH::DefaultBroadPhaseLayerFilter bp; const JPH::DefaultObjectLayerFilter ol;
		std::vector<double> th; unsigned long trips = 0;
		for (int fr = 0; fr < warm + frames; ++fr) {
			const unsigned long t_before = g_round_trips;
			const double t0 = now_ms();
			for (int i = 0; i < N; ++i) {
				JPH::CharacterVirtual& c = *chars[i];
				c.SetLinearVelocity(velocityFor(wishOf(i), c.GetLinearVelocity(), c.IsSupported(), c.GetGroundVelocity()));
				c.ExtendedUpdate(DT, system.GetGravity(), ext, bp, ol, bf, sf, ta);
			}
			if (fr >= warm) { th.push_back(now_ms() - t0); trips += g_round_trips - t_before; }
		}
		// the batch
		std::vector<double> tb;
		{
			CharacterBatch batch(&system, (uint32_t)N);
			std::vector<uint32_t> cid(N);
			for (int i = 0; i < N; ++i) cid[i] = batch.add(*settings.GetPtr(), ext, startOf(i));
			for (int fr = 0; fr < warm + frames; ++fr) {
				const double t0 = now_ms();
				for (int i = 0; i < N; ++i) batch.SetLinearVelocity(cid[i], velocityFor(wishOf(i), batch.GetLinearVelocity(cid[i]), batch.IsSupported(cid[i]), batch.GetGroundVelocity(cid[i])));
				batch.update(DT);
				batch.readBack();
				if (fr >= warm) tb.push_back(now_ms() - t0);
			}
		}
		const double mh = median(th), mb = median(tb);
		printf("| %d | %.3f | %.1f | %.3f | %.1f |\n", N, mh, (double)trips / ((double)frames * N), mb, mh / mb);
		fflush(stdout);
	}
	sgp_world_destroy(world);
	return 0;
}
