// A caller with audio sources twice over: sources at points and on cubes behind a wall are held by an AudibilityBatch (shim/AudibilityBatch.h) while the
// camera walks along the wall, past its end and through a parcel that mutes outside audio, and next to it the host does what checkForAudioRangeChanges
// (GUIClient.cpp:4512-4543) and the audio-occlusion walk (GUIClient.cpp:6973-7034) do -- one source at a time, one blocking doesRayHitAnything per source in
// range, the mute ramp of AudioSource with its own expressions -- as docs/CONTRACT.md 4m writes them.  Half way the batch and the world are saved with events
// still undrained, run on, rolled back and run again.  Also asks doRaysHitAnything (one launch) what doesRayHitAnything answers ray by ray.  Prints one JSON
// line: how the two event streams compare.
#include "PhysicsWorld.h"
#include "AudibilityBatch.h"
#include <utils/Exception.h>
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

struct Ev { int kind; void* source; uint32_t value; uint32_t update; };      // value: num_occlusions, or the factor's bits
static bool operator==(const Ev& a, const Ev& b) { return a.kind == b.kind && a.source == b.source && a.value == b.value && a.update == b.update; }
static uint32_t bitsOf(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }

// glare::AudioSource as far as the two walks touch it (AudioEngine.h:136-140, AudioEngine.cpp:69-121)
struct HostSource
{
	Reference<PhysicsObject> ob; float half[3]; float pos[3]; float volume; uint32_t parcel; bool one_shot;
	bool in_audio_proximity = false; uint32_t num_occlusions = 0;
	float mute_volume_factor = 1.f; double mute_change_start_time = -2, mute_change_end_time = -1; float mute_vol_fac_start = 1.f, mute_vol_fac_end = 1.f;
	void startMuting(double cur_time, double transition_period)
	{
		if (mute_vol_fac_end != 0) { mute_change_start_time = cur_time; mute_change_end_time = cur_time + transition_period * mute_volume_factor; mute_vol_fac_start = mute_volume_factor; mute_vol_fac_end = 0; }
	}
	void startUnmuting(double cur_time, double transition_period)
	{
		if (mute_vol_fac_end != 1) { mute_change_start_time = cur_time; mute_change_end_time = cur_time + transition_period * (1.f - mute_volume_factor); mute_vol_fac_start = mute_volume_factor; mute_vol_fac_end = 1; }
	}
	void updateCurrentMuteVolumeFactor(double cur_time)
	{
		if ((cur_time < mute_change_end_time) && ((mute_change_end_time - mute_change_start_time) > 1.0e-4)) {
			const double frac = (cur_time - mute_change_start_time) / (mute_change_end_time - mute_change_start_time);
			mute_volume_factor = mute_vol_fac_start + (float)frac * (mute_vol_fac_end - mute_vol_fac_start);
		} else mute_volume_factor = mute_vol_fac_end;
	}
};

static Reference<PhysicsObject> cube(PhysicsWorld& w, Vec4f pos, Vec3f scale, PhysicsObject::MotionType motion)
{
	Reference<PhysicsObject> ob = new PhysicsObject(true);
	ob->is_cube = true; ob->scale = scale; ob->pos = pos; ob->motion_type = motion; ob->mass = 50.f;
	w.addObject(ob);
	if (motion != PhysicsObject::MotionType_static) w.activateObject(ob);
	return ob;
}

static void campos(int frame, float* p) { p[0] = -40.f + 1.0f * (float)frame; p[1] = -6.f + 0.5f * std::sin(0.1f * (float)frame); p[2] = 1.7f; }
// the parcel the camera stands in: parcel 9 (x in [-5, 25]) mutes outside audio
static void camParcel(const float* p, uint32_t* id, bool* mute) { const bool in = p[0] >= -5.f && p[0] <= 25.f; *id = in ? 9u : SGP_INVALID_ID; *mute = in; }

int main()
{
	try {
		PhysicsWorld::init();
		Reference<PhysicsWorld> world = new PhysicsWorld(nullptr, nullptr);
		cube(*world, Vec4f(0, 0, -0.5f, 1), Vec3f(400.f, 400.f, 1.f), PhysicsObject::MotionType_static);
		cube(*world, Vec4f(-10.f, 0.f, 2.5f, 1), Vec3f(50.f, 0.4f, 5.f), PhysicsObject::MotionType_static);      // the wall: x in [-35, 15], y = 0
		std::vector<HostSource> sources(14);
		for (int i = 0; i < 14; ++i) {
			HostSource& s = sources[i];
			s.volume = 0.2f + 0.05f * (float)(i % 4); s.parcel = (i % 3 == 0) ? 9u : ((i % 3 == 1) ? 4u : SGP_INVALID_ID); s.one_shot = i == 5;
			const float x = -38.f + 6.f * (float)i, y = 5.f + (float)(i % 2) * 3.f;
			if (i % 2) { s.ob = cube(*world, Vec4f(x, y, 1.f, 1), Vec3f(0.8f, 0.8f, 0.8f), PhysicsObject::MotionType_static); s.half[0] = s.half[1] = s.half[2] = 0.4f; }
			else { s.pos[0] = x; s.pos[1] = y; s.pos[2] = 1.5f; }
		}
		AudibilityBatch batch(world.ptr(), 32, 1, 4096);
		for (HostSource& s : sources) {
			if (!s.ob.isNull()) batch.addSourceOnObject(&s, *s.ob, s.volume, s.parcel, s.one_shot);
			else batch.addSourceAtPoint(&s, Vec4f(s.pos[0], s.pos[1], s.pos[2], 1), s.volume, s.parcel, s.one_shot);
		}
		{ float p[3]; campos(0, p); batch.setListener(0, Vec4f(p[0], p[1], p[2], 1)); }

		const float dt = 1.f / 60.f;
		const int frames = 90, save_at = 40, replay = 20;
		uint32_t host_updates = 0; int rays_any_mismatch = 0; size_t rays_asked = 0;
		// the host's two walks for the camera at p
		auto hostWalks = [&](const float* p, double cur_time, std::vector<Ev>& out) {
			uint32_t in_parcel; bool mute_outside_audio; camParcel(p, &in_parcel, &mute_outside_audio);
			std::vector<Vec4f> origins, dirs; std::vector<float> max_ts; std::vector<uint8_t> single;
			for (HostSource& s : sources) {
				if (!s.ob.isNull()) {      // getCentroidWS of the object's world AABB (identity rotation: centre -+ half extent)
					JPH::RVec3 c; JPH::Quat q;
					world->physics_system->GetBodyInterface().GetPositionAndRotation(s.ob->jolt_body_id, c, q);
					const float cc[3] = { (float)c.GetX(), (float)c.GetY(), (float)c.GetZ() };
					for (int k = 0; k < 3; ++k) s.pos[k] = ((cc[k] - s.half[k]) + (cc[k] + s.half[k])) * 0.5f;
				}
				const float dx = s.pos[0] - p[0], dy = s.pos[1] - p[1], dz = s.pos[2] - p[2];
				const float dist2 = (dx * dx + dy * dy) + dz * dz;
				const float max_dist = 60.f * s.volume, max_dist2 = max_dist * max_dist;
				if (s.in_audio_proximity && dist2 > max_dist2) { s.in_audio_proximity = false; out.push_back(Ev{ AudibilityBatch::MovedOutOfAudioRange, &s, 0u, host_updates }); }
				else if (!s.in_audio_proximity && dist2 <= max_dist2) { s.in_audio_proximity = true; out.push_back(Ev{ AudibilityBatch::MovedIntoAudioRange, &s, 0u, host_updates }); }
				if (!s.in_audio_proximity) continue;
				const float dist = std::sqrt(dist2);
				if (!(dist < max_dist)) continue;
				const Vec4f trace_dir = (dist == 0) ? Vec4f(1, 0, 0, 0) : Vec4f(dx / dist, dy / dist, dz / dist, 0);
				const float trace_dist = std::fmin(std::fmax(dist - 1.f, 0.f), 60.f);
				const Vec4f trace_start(p[0], p[1], p[2], 1);
				const bool hit_object = world->doesRayHitAnything(trace_start, trace_dir, trace_dist);
				origins.push_back(trace_start); dirs.push_back(trace_dir); max_ts.push_back(trace_dist); single.push_back(hit_object ? 1 : 0);
				const uint32_t now = hit_object ? 1u : 0u;
				if (now != s.num_occlusions) { s.num_occlusions = now; out.push_back(Ev{ now ? AudibilityBatch::BecameOccluded : AudibilityBatch::BecameUnoccluded, &s, now, host_updates }); }
				if (!s.one_shot) {
					const float old_mute_volume_factor = s.mute_volume_factor;
					if (mute_outside_audio) { if (s.parcel != in_parcel) s.startMuting(cur_time, 1); else s.startUnmuting(cur_time, 1); }
					else s.startUnmuting(cur_time, 1);
					s.updateCurrentMuteVolumeFactor(cur_time);
					if (old_mute_volume_factor != s.mute_volume_factor) out.push_back(Ev{ AudibilityBatch::VolumeUpdated, &s, bitsOf(s.mute_volume_factor), host_updates });
				}
			}
			// the same rays in one launch
			std::vector<uint8_t> many;
			world->doRaysHitAnything(origins, dirs, max_ts, many);
			rays_asked += origins.size();
			for (size_t i = 0; i < single.size(); ++i) if (many.size() != single.size() || (many[i] != 0) != (single[i] != 0)) ++rays_any_mismatch;
			++host_updates;
		};
		auto frame = [&](int f, std::vector<Ev>& host_out) {
			world->think(dt);
			float p[3]; campos(f, p);
			const double cur_time = 10.0 + 0.05 * (double)f + 0.01 * (double)(f % 3);
			uint32_t in_parcel; bool mute; camParcel(p, &in_parcel, &mute);
			batch.setListenerParcel(0, in_parcel, mute);
			batch.think(Vec4f(p[0], p[1], p[2], 1), cur_time);
			hostWalks(p, cur_time, host_out);
		};
		int occlusion_callbacks = 0, volume_callbacks = 0, range_callbacks = 0;
		auto drain = [&](std::vector<Ev>& out) {
			// (the named callbacks carry no update index: the comparison takes the events through the plain drain and counts what each callback would get)
			return batch.drain([&](const AudibilityBatch::Event& e) {
				const bool range = e.kind == AudibilityBatch::MovedIntoAudioRange || e.kind == AudibilityBatch::MovedOutOfAudioRange;
				if (range) ++range_callbacks; else if (e.kind == AudibilityBatch::VolumeUpdated) ++volume_callbacks; else ++occlusion_callbacks;
				out.push_back(Ev{ (int)e.kind, e.source, range ? 0u : (e.kind == AudibilityBatch::VolumeUpdated ? bitsOf(e.mute_volume_factor) : e.num_occlusions), e.update_index });
			});
		};

		std::vector<Ev> got, want;
		uint32_t dropped = 0;
		for (int f = 0; f < save_at; ++f) { frame(f, want); if (f % 7 == 6) dropped += drain(got); }
		// a source behind the wall and one past its end, seen from the camera at frame save_at - 1 (x = -1)
		const bool occluded_behind_wall = batch.numOcclusions(&sources[6]) == 1 && sources[6].num_occlusions == 1;
		// save with events pending, run on, come back, run again: the same events, drained as one stream
		AudibilityBatch::SavedState saved;
		batch.saveState(saved);
		Reference<PhysicsWorldCheckpoint> cp = world->checkpoint();
		const std::vector<HostSource> sources_saved = sources; const size_t want_saved = want.size(); const uint32_t updates_saved = host_updates;
		std::vector<Ev> first_run, second_run, scratch;
		for (int f = save_at; f < save_at + replay; ++f) frame(f, scratch);
		dropped += drain(first_run);
		batch.restoreState(saved);
		if (!world->rollback(*cp)) return 4;
		for (size_t i = 0; i < sources.size(); ++i) { const Reference<PhysicsObject> ob = sources[i].ob; sources[i] = sources_saved[i]; sources[i].ob = ob; }
		want.resize(want_saved); host_updates = updates_saved;
		for (int f = save_at; f < save_at + replay; ++f) frame(f, want);
		dropped += drain(second_run);
		const bool replay_equal = first_run == second_run && !first_run.empty();
		got.insert(got.end(), second_run.begin(), second_run.end());
		for (int f = save_at + replay; f < frames; ++f) frame(f, want);
		dropped += drain(got);
		// at the last frame the camera is at x = 49, past the wall's end: source 13 (x = 40) is in the open
		const bool occluded_in_the_open = batch.numOcclusions(&sources[13]) == 1 || sources[13].num_occlusions == 1;

		size_t mismatches = got.size() > want.size() ? got.size() - want.size() : want.size() - got.size();
		for (size_t i = 0; i < std::min(got.size(), want.size()); ++i) if (!(got[i] == want[i])) ++mismatches;
		bool state_equal = true;
		for (HostSource& s : sources) state_equal = state_equal && batch.inAudioProximity(&s) == s.in_audio_proximity && batch.numOcclusions(&s) == s.num_occlusions && bitsOf(batch.muteVolumeFactor(&s, 0, 1)) == bitsOf(s.mute_volume_factor);
		printf("{\"sources\": %u, \"frames\": %d, \"events\": %zu, \"expected\": %zu, \"mismatches\": %zu, \"range_callbacks\": %d, \"occlusion_callbacks\": %d, \"volume_callbacks\": %d, \"replay_equal\": %s, \"replay_events\": %zu, \"dropped\": %u, \"state_equal\": %s, \"occluded_behind_wall\": %s, \"occluded_in_the_open\": %s, \"rays_asked\": %zu, \"rays_any_mismatch\": %d}\n",
		       batch.numSources(), frames, got.size(), want.size(), mismatches, range_callbacks, occlusion_callbacks, volume_callbacks, replay_equal ? "true" : "false", first_run.size(), dropped,
		       state_equal ? "true" : "false", occluded_behind_wall ? "true" : "false", occluded_in_the_open ? "true" : "false", rays_asked, rays_any_mismatch);
		return 0;
	} catch (glare::Exception& e) { fprintf(stderr, "glare::Exception: %s\n", e.what().c_str()); return 2; }
	catch (std::exception& e) { fprintf(stderr, "exception: %s\n", e.what()); return 3; }
}
