// AudibilityBatch: the two audio walks of GUIClient -- checkForAudioRangeChanges (GUIClient.cpp:4512-4543) and "audio occlusions"
// (GUIClient.cpp:6973-7034) -- for many sources on the device (sgp_audibility_*, include/sgp.h).  The reference walks every audio source twice per
// frame on the host and traces one blocking ray per source in range; with a batch the range bit, num_occlusions and the mute ramp of every
// (source, listener) pair live on the device, think(cur_time) enqueues the update on the world's stream and returns, and drain() calls the caller back
// once per transition, in the library's order: where the reference calls sourceNumOcclusionsUpdated, sourceVolumeUpdated, and where it creates or drops
// the audio source at the edge of the range.  What stays here: which source holds which slot.  Departures: docs/GAPS.md ("Audio sources").
#pragma once
#include "../../include/sgp.h"
#include "PhysicsWorld.h"
#include "BatchCheckpoint.h"
#include "ProximityBatch.h"
#include "maths/Vec4f.h"
#include <cstring>
#include <functional>
#include <stdexcept>
#include <string>
#include <unordered_map>
#include <vector>

class AudibilityBatch
{
public:
	enum EventKind { MovedIntoAudioRange = SGP_AUD_EV_IN_RANGE, MovedOutOfAudioRange = SGP_AUD_EV_OUT_OF_RANGE, BecameOccluded = SGP_AUD_EV_OCCLUDED,
		BecameUnoccluded = SGP_AUD_EV_UNOCCLUDED, VolumeUpdated = SGP_AUD_EV_VOLUME };
	// source: what the caller added (its glare::AudioSource* or WorldObject*); num_occlusions: 1 or 0 after an occlusion event; mute_volume_factor: after a volume event
	struct Event { EventKind kind; void* source; uint32_t listener; uint32_t num_occlusions; float mute_volume_factor; uint32_t update_index; };
	struct Callbacks {
		std::function<void(void* source, uint32_t listener, bool in_range)> audioRangeChanged;                   // loadAudioForObject / removeSource at :4519-4542
		std::function<void(void* source, uint32_t listener, uint32_t num_occlusions)> sourceNumOcclusionsUpdated; // AudioEngine::sourceNumOcclusionsUpdated, where the number changed
		std::function<void(void* source, uint32_t listener, float mute_volume_factor)> sourceVolumeUpdated;       // AudioEngine::sourceVolumeUpdated
	};

	AudibilityBatch(PhysicsWorld* world_, uint32_t source_capacity, uint32_t listener_capacity, uint32_t event_capacity) : world(world_), batch(nullptr), ev_cap(event_capacity), dropped(0)
	{
		check(sgp_audibility_create(world->world, source_capacity, listener_capacity, event_capacity, &batch), "sgp_audibility_create");
	}
	~AudibilityBatch() { if (batch) sgp_audibility_destroy(batch); }
	AudibilityBatch(const AudibilityBatch&) = delete;
	AudibilityBatch& operator=(const AudibilityBatch&) = delete;

	// a source at a point the caller moves (audio_source->pos = ...), or on a physics object (its world AABB's centroid, getCentroidWS, read on the device).
	// parcel_id: AudioSource::userdata_1; one_shot: SourceType_NonStreaming && !looping.
	void addSourceAtPoint(void* source, const Vec4f& pos, float volume, uint32_t parcel_id = SGP_INVALID_ID, bool one_shot = false)
	{
		sgp_audibility_source d = desc(source, volume, parcel_id, one_shot);
		d.kind = SGP_AUD_SRC_POINT; d.pos[0] = pos[0]; d.pos[1] = pos[1]; d.pos[2] = pos[2];
		add(source, d);
	}
	void addSourceOnObject(void* source, PhysicsObject& object, float volume, uint32_t parcel_id = SGP_INVALID_ID, bool one_shot = false)
	{
		sgp_audibility_source d = desc(source, volume, parcel_id, one_shot);
		d.kind = SGP_AUD_SRC_BODY; d.body = object.jolt_body_id.GetIndex();
		add(source, d);
	}
	void removeSource(void* source)
	{
		const auto it = slot_of.find(source);
		if (it == slot_of.end()) return;
		check(sgp_audibility_remove(batch, it->second), "sgp_audibility_remove");
		slot_of.erase(it);
	}
	void setSourcePos(void* source, const Vec4f& pos)
	{
		const float p[3] = { pos[0], pos[1], pos[2] };
		check(sgp_audibility_set_points(batch, slot_of.at(source), 1, p), "sgp_audibility_set_points");
	}
	void setSourceVolume(void* source, float volume) { check(sgp_audibility_set_volume(batch, slot_of.at(source), volume), "sgp_audibility_set_volume"); }

	// listener 0 is the camera of think(); further listeners are other avatars this process hosts
	void setListener(uint32_t k, const Vec4f& pos, uint32_t in_parcel_id = SGP_INVALID_ID, bool mute_outside_audio = false)
	{
		sgp_audibility_listener o; memset(&o, 0, sizeof(o));
		o.source = SGP_AUD_LST_POINT; o.pos[0] = pos[0]; o.pos[1] = pos[1]; o.pos[2] = pos[2];
		o.ignore_body = SGP_INVALID_ID; o.zone_key = in_parcel_id; o.mute_outside = mute_outside_audio ? 1u : 0u;
		check(sgp_audibility_set_listener(batch, k, &o), "sgp_audibility_set_listener");
	}
	void setListenerOnObject(uint32_t k, PhysicsObject& object, const Vec4f& offset, uint32_t in_parcel_id = SGP_INVALID_ID, bool mute_outside_audio = false)
	{
		sgp_audibility_listener o; memset(&o, 0, sizeof(o));
		o.source = SGP_AUD_LST_BODY; o.body = object.jolt_body_id.GetIndex(); o.offset[0] = offset[0]; o.offset[1] = offset[1]; o.offset[2] = offset[2];
		o.ignore_body = o.body; o.zone_key = in_parcel_id; o.mute_outside = mute_outside_audio ? 1u : 0u;      // (a listener that is a body would otherwise always be inside its own shape)
		check(sgp_audibility_set_listener(batch, k, &o), "sgp_audibility_set_listener");
	}
	void setListenerParcel(uint32_t k, uint32_t in_parcel_id, bool mute_outside_audio) { check(sgp_audibility_set_listener_zone(batch, k, in_parcel_id, mute_outside_audio ? 1u : 0u), "sgp_audibility_set_listener_zone"); }
	void removeListener(uint32_t k) { check(sgp_audibility_remove_listener(batch, k), "sgp_audibility_remove_listener"); }

	// The listeners' parcels from a ProximityBatch's observers, on the device: listener k stands in the parcel observer k stands in; muting_parcel_ids
	// (ascending): the parcels with MUTE_OUTSIDE_AUDIO_FLAG.  NULL detaches (do so before the ProximityBatch goes).
	void attachProximity(ProximityBatch* proximity, const std::vector<uint32_t>& muting_parcel_ids = std::vector<uint32_t>())
	{
		check(sgp_audibility_set_muting_keys(batch, muting_parcel_ids.data(), (uint32_t)muting_parcel_ids.size()), "sgp_audibility_set_muting_keys");
		check(sgp_audibility_attach_proximity(batch, proximity ? proximity->handle() : nullptr), "sgp_audibility_attach_proximity");
	}

	// both walks for every listener: enqueued, not waited for.  Call it once per frame, after PhysicsWorld::think (and after ProximityBatch::think where attached).
	void think(double cur_time) { check(sgp_audibility_update(batch, cur_time), "sgp_audibility_update"); }
	void think(const Vec4f& campos, double cur_time)
	{
		const float p[3] = { campos[0], campos[1], campos[2] };
		check(sgp_audibility_set_listener_points(batch, 0, 1, p), "sgp_audibility_set_listener_points");
		think(cur_time);
	}

	// waits for what is in flight; one call per event since the last drain, in the library's order.  Returns how many events the batch had to drop.
	uint32_t drain(const std::function<void(const Event&)>& callback)
	{
		events.resize(ev_cap);
		uint32_t n = 0, n_dropped = 0;
		check(sgp_audibility_drain_events(batch, events.data(), ev_cap, &n, &n_dropped), "sgp_audibility_drain_events");
		for (uint32_t i = 0; i < n; ++i) {
			const sgp_audibility_event& e = events[i];
			callback(Event{ (EventKind)e.kind, (void*)e.tag, e.listener, e.kind == SGP_AUD_EV_OCCLUDED ? 1u : 0u, e.factor, e.update_index });
		}
		dropped += n_dropped;
		return n_dropped;
	}
	// ... through the reference's names
	uint32_t drain(const Callbacks& cb)
	{
		return drain([&cb](const Event& e) {
			if (e.kind == MovedIntoAudioRange || e.kind == MovedOutOfAudioRange) { if (cb.audioRangeChanged) cb.audioRangeChanged(e.source, e.listener, e.kind == MovedIntoAudioRange); }
			else if (e.kind == VolumeUpdated) { if (cb.sourceVolumeUpdated) cb.sourceVolumeUpdated(e.source, e.listener, e.mute_volume_factor); }
			else if (cb.sourceNumOcclusionsUpdated) cb.sourceNumOcclusionsUpdated(e.source, e.listener, e.num_occlusions);
		});
	}

	// in_audio_proximity, num_occlusions and getMuteVolumeFactor() of a source for listener k, as the last update left them (wait)
	bool inAudioProximity(void* source, uint32_t k = 0) { return (state(source).in_range_mask >> k & 1u) != 0; }
	uint32_t numOcclusions(void* source, uint32_t k = 0) { return state(source).occluded_mask >> k & 1u; }
	float muteVolumeFactor(void* source, uint32_t k, uint32_t listener_capacity)
	{
		std::vector<sgp_audibility_pair_state> p(listener_capacity);
		check(sgp_audibility_get_pair_states(batch, slot_of.at(source), 1, p.data()), "sgp_audibility_get_pair_states");
		return p.at(k).mute_volume_factor;
	}

	uint32_t numSources() const { return (uint32_t)slot_of.size(); }
	uint64_t numDropped() const { return dropped; }
	sgp_audibility* handle() const { return batch; }

	// Extensions (not in the reference): the batch as it is now, to come back to after PhysicsWorld's rollback to the checkpoint of the same moment -- the
	// library's state (the pairs, undrained events) and what this header keeps on the host: the sources' slots.
	struct SavedState { BatchCheckpoint lib; std::unordered_map<void*, uint32_t> slot_of; uint64_t dropped = 0; };
	void saveState(SavedState& s)
	{
		check(sgp_audibility_checkpoint(batch, &s.lib.cp), "sgp_audibility_checkpoint");
		s.slot_of = slot_of; s.dropped = dropped;
	}
	void restoreState(const SavedState& s)
	{
		check(sgp_audibility_rollback(batch, s.lib.cp), "sgp_audibility_rollback");
		slot_of = s.slot_of; dropped = s.dropped;
	}

private:
	static void check(int rc, const char* what) { if (rc != SGP_OK) throw std::runtime_error(std::string(what) + ": " + sgp_last_error()); }
	static sgp_audibility_source desc(void* source, float volume, uint32_t parcel_id, bool one_shot)
	{
		sgp_audibility_source d; memset(&d, 0, sizeof(d));
		d.volume = volume; d.zone_key = parcel_id; d.tag = (uint64_t)source;
		d.flags = SGP_AUD_WANT_RANGE | SGP_AUD_WANT_OCCLUSION | SGP_AUD_WANT_VOLUME | (one_shot ? SGP_AUD_ONE_SHOT : 0u);
		return d;
	}
	void add(void* source, const sgp_audibility_source& d)
	{
		if (slot_of.count(source)) return;      // (a set: inserting twice changes nothing)
		uint32_t id = 0;
		check(sgp_audibility_add(batch, &d, 1, &id), "sgp_audibility_add");
		slot_of[source] = id;
	}
	sgp_audibility_state state(void* source)
	{
		sgp_audibility_state s; memset(&s, 0, sizeof(s));
		check(sgp_audibility_get_states(batch, slot_of.at(source), 1, &s), "sgp_audibility_get_states");
		return s;
	}

	PhysicsWorld* world;
	sgp_audibility* batch;
	uint32_t ev_cap;
	uint64_t dropped;
	std::unordered_map<void*, uint32_t> slot_of;
	std::vector<sgp_audibility_event> events;
};
