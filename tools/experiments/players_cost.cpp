// What a driven character batch costs and saves, on characters_bench's scene (N characters walking on the ground around the settled config-3 pile).
//   players_cost <descs> <frames> table                    per-frame host wall time, N = 1, 64, 1024: today's caller loop (readBack, host rule, SetLinearVelocity,
//                                                          update) against the driven batch (sgp_characters_update_at only); median of <frames> after 5 of warm-up
//   players_cost <descs> <frames> kernel undriven|driven N  the same walk of N characters for <frames> frames, for a kernel trace of k_characters_update
// Built with -DNO_DRIVE the program has the undriven walk only and calls nothing a library without the driven entry points lacks (the A/B against an earlier build).
// Driven by players_cost.py, which writes the pile's body descriptions to the file named in argv[1].
#include "../../include/sgp.h"
#include "CharacterBatch.h"
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
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

struct Setup { JPH::CharRef<JPH::CharacterVirtualSettings> settings; JPH::CharacterVirtual::ExtendedUpdateSettings ext; };

// today's caller loop: the states come back, the host computes every velocity, the inputs go up, the update is enqueued
static void callerLoop(JPH::PhysicsSystem& system, const Setup& su, int N, int warm, int frames, std::vector<double>* ms)
{
	CharacterBatch batch(&system, (uint32_t)N);
	std::vector<uint32_t> cid(N);
	for (int i = 0; i < N; ++i) cid[i] = batch.add(*su.settings.GetPtr(), su.ext, startOf(i));
	for (int fr = 0; fr < warm + frames; ++fr) {
		const double t0 = now_ms();
		batch.readBack();
		for (int i = 0; i < N; ++i) batch.SetLinearVelocity(cid[i], velocityFor(wishOf(i), batch.GetLinearVelocity(cid[i]), batch.IsSupported(cid[i]), batch.GetGroundVelocity(cid[i])));
		batch.update(DT);
		if (ms && fr >= warm) ms->push_back(now_ms() - t0);
	}
	batch.readBack();
}

#ifndef NO_DRIVE
static void check(int rc) { if (rc != SGP_OK) { fprintf(stderr, "%s\n", sgp_last_error()); exit(3); } }
// the driven batch: the wishes go up once (they stay in force), a frame is sgp_characters_update_at
static void drivenLoop(sgp_world* world, const Setup& su, int N, int warm, int frames, std::vector<double>* ms)
{
	const sgp_character_desc desc = CharacterBatch::makeDesc(*su.settings.GetPtr(), su.ext);
	sgp_characters* cs = nullptr;
	check(sgp_characters_create(world, (uint32_t)N, &cs));
	std::vector<sgp_character_input> in(N); std::vector<sgp_character_drive> dr(N);
	for (int i = 0; i < N; ++i) {
		const JPH::Vec3 p = startOf(i), w = wishOf(i); const float pos[3] = { p.x, p.y, p.z }; uint32_t id = 0;
		check(sgp_character_add(cs, &desc, pos, &id));
		in[i].velocity[0] = in[i].velocity[1] = in[i].velocity[2] = 0; in[i].ignore_id = SGP_INVALID_ID; in[i].flags = SGP_CHAR_EXTENDED;
		sgp_default_character_drive(&dr[i]); dr[i].flags |= SGP_DRIVE_ON; dr[i].move_desired_vel[0] = w.x; dr[i].move_desired_vel[1] = w.y; dr[i].move_desired_vel[2] = w.z;
	}
	check(sgp_characters_set_inputs(cs, 0, (uint32_t)N, in.data())); check(sgp_characters_set_drive(cs, 0, (uint32_t)N, dr.data()));
	for (int fr = 0; fr < warm + frames; ++fr) {
		const double t0 = now_ms();
		check(sgp_characters_update_at(cs, DT, (double)fr * (1.0 / 60.0)));
		if (ms && fr >= warm) ms->push_back(now_ms() - t0);
	}
	std::vector<sgp_character_state> st(N);
	check(sgp_characters_get_states(cs, 0, (uint32_t)N, st.data()));      // (waits for the stream: the trace is complete)
	check(sgp_characters_destroy(cs));
}
#endif

int main(int argc, char** argv)
{
	if (argc < 4) { fprintf(stderr, "usage: players_cost <descs> <frames> table | kernel undriven|driven N\n"); return 2; }
	FILE* f = fopen(argv[1], "rb"); if (!f) return 2;
	fseek(f, 0, SEEK_END); const size_t bytes = (size_t)ftell(f); fseek(f, 0, SEEK_SET);
	std::vector<sgp_body_desc> descs(bytes / sizeof(sgp_body_desc));
	if (fread(descs.data(), sizeof(sgp_body_desc), descs.size(), f) != descs.size()) return 2;
	fclose(f);
	const int frames = atoi(argv[2]), warm = 5;
	const std::string mode = argv[3];
	if (sgp_init() < 1) { fprintf(stderr, "%s\n", sgp_last_error()); return 3; }
	sgp_world_desc wd; sgp_default_world_desc(&wd); wd.max_bodies = (uint32_t)descs.size() + 1024;
	sgp_world* world = nullptr;
	if (sgp_world_create(&wd, &world) != SGP_OK) { fprintf(stderr, "%s\n", sgp_last_error()); return 3; }
	std::vector<uint32_t> ids(descs.size());
	if (sgp_body_add_batch(world, descs.data(), (uint32_t)descs.size(), ids.data()) != SGP_OK) { fprintf(stderr, "%s\n", sgp_last_error()); return 3; }
	for (int s = 0; s < 240; ++s) sgp_world_step(world, DT);      // let the pile settle a little
	JPH::PhysicsSystem system(world);
	Setup su;
	JPH::CharRef<JPH::CharacterShape> shape = JPH::RotatedTranslatedShapeSettings(JPH::Vec3(0, 0, 0.95f), JPH::Quat(0.7071068f, 0, 0, 0.7071068f), new JPH::CapsuleShape(0.65f, 0.3f)).Create().Get();
	su.settings = new JPH::CharacterVirtualSettings();
	su.settings->mShape = shape; su.settings->mUp = JPH::Vec3(0, 0, 1); su.settings->mSupportingVolume = JPH::Plane(JPH::Vec3(0, 0, 1), -0.3f); su.settings->mMaxStrength = 1000;
	su.ext.mStickToFloorStepDown = JPH::Vec3(0, 0, -0.5f); su.ext.mWalkStairsStepUp = JPH::Vec3(0, 0, 0.4f);
	if (mode == "kernel") {
		if (argc < 6) return 2;
		const std::string which = argv[4]; const int N = atoi(argv[5]);
		if (which == "undriven") callerLoop(system, su, N, warm, frames, nullptr);
#ifndef NO_DRIVE
		else if (which == "driven") drivenLoop(world, su, N, warm, frames, nullptr);
#endif
		else return 2;
		printf("%s walk of %d characters: %d frames\n", which.c_str(), N, warm + frames);
	}
#ifndef NO_DRIVE
	else if (mode == "table") {
		printf("| N | caller loop (readBack, host rule, SetLinearVelocity, update), ms per frame | driven batch (update_at only), ms per frame | ratio |\n|---|---|---|---|\n");
		const int Ns[3] = { 1, 64, 1024 };
		for (int N : Ns) {
			std::vector<double> tc, td;
			callerLoop(system, su, N, warm, frames, &tc);
			drivenLoop(world, su, N, warm, frames, &td);
			const double mc = median(tc), md = median(td);
			printf("| %d | %.4f | %.4f | %.1f |\n", N, mc, md, mc / md);
			fflush(stdout);
		}
	}
#endif
	else return 2;
	sgp_world_destroy(world);
	return 0;
}
