// ProximityBatch: ScriptedObjectProximityChecker (gui_client/ScriptedObjectProximityChecker.h/.cpp) and the parcel enter / exit walks of GUIClient
// (GUIClient.cpp:6874-6968) for many objects on the device (sgp_proximity_*, include/sgp.h).  The reference tests every scripted object's AABB against the
// camera on the host every frame; with a batch the near bits and the observer's parcel live on the device, think(campos) moves observer 0, enqueues the
// update on the world's stream and returns, and drain() calls the caller back once per event, in the library's order.  What stays here: which object holds
// which slot (addObject / removeObject / clear carry the reference's names), the parcels by their id, and the 0.5 s throttle of onUserTouchedObject
// (GUIClient.cpp:6464-6469), a host-side helper keyed by the object and fed from the character batch's drained contacts.  Departures: docs/GAPS.md
// ("Proximity watchers").
#pragma once
#include "../../include/sgp.h"
#include "PhysicsWorld.h"
#include "BatchCheckpoint.h"
#include "maths/Vec4f.h"
#include <cstring>
#include <functional>
#include <map>
#include <stdexcept>
#include <string>
#include <unordered_map>
#include <vector>

class ProximityBatch
{
public:
	enum EventKind { UserMovedNearToObject = SGP_PROX_EV_NEAR, UserMovedAwayFromObject = SGP_PROX_EV_AWAY, UserExitedParcel = SGP_PROX_EV_EXITED, UserEnteredParcel = SGP_PROX_EV_ENTERED };
	// object: NULL in the observer-level parcel records (the reference's UserEnteredParcelMessage carries no object)
	struct Event { EventKind kind; PhysicsObject* object; uint32_t observer; uint32_t parcel_id; uint32_t update_index; };

	ProximityBatch(PhysicsWorld* world_, uint32_t object_capacity, uint32_t parcel_capacity, uint32_t event_capacity) : world(world_), batch(nullptr), ev_cap(event_capacity), dropped(0)
	{
		check(sgp_proximity_create(world->world, object_capacity, parcel_capacity, event_capacity, &batch), "sgp_proximity_create");
	}
	~ProximityBatch() { if (batch) sgp_proximity_destroy(batch); }
	ProximityBatch(const ProximityBatch&) = delete;
	ProximityBatch& operator=(const ProximityBatch&) = delete;

	// addObject(ob): the reference adds every scripted object ("TEMP: just add in all cases"); has_near_handlers / has_parcel_handlers say which events the
	// object's scripts listen for (event_handlers->onUserMovedNearToObject_handlers.nonEmpty() and its kin).
	void addObject(PhysicsObject& object, bool has_near_handlers = true, bool has_parcel_handlers = true, float radius = 20.f)
	{
		if (slot_of.count(&object)) return;      // (a set: inserting twice changes nothing)
		sgp_proximity_object d; memset(&d, 0, sizeof(d));
		d.body = object.jolt_body_id.GetIndex(); d.radius = radius; d.tag = (uint64_t)&object;
		d.flags = (has_near_handlers ? SGP_PROX_WANT_NEAR : 0u) | (has_parcel_handlers ? SGP_PROX_WANT_ZONE : 0u);
		uint32_t id = 0;
		check(sgp_proximity_add(batch, &d, 1, &id), "sgp_proximity_add");
		slot_of[&object] = id;
	}
	// many at once: one walk over the batch's links for the whole call
	void addObjects(const std::vector<PhysicsObject*>& objects, float radius = 20.f)
	{
		std::vector<sgp_proximity_object> d; std::vector<PhysicsObject*> fresh;
		for (PhysicsObject* ob : objects) {
			if (slot_of.count(ob)) continue;
			sgp_proximity_object o; memset(&o, 0, sizeof(o));
			o.body = ob->jolt_body_id.GetIndex(); o.radius = radius; o.flags = SGP_PROX_WANT_NEAR | SGP_PROX_WANT_ZONE; o.tag = (uint64_t)ob;
			d.push_back(o); fresh.push_back(ob);
		}
		std::vector<uint32_t> ids(d.size());
		check(sgp_proximity_add(batch, d.data(), (uint32_t)d.size(), ids.data()), "sgp_proximity_add");
		for (size_t i = 0; i < fresh.size(); ++i) slot_of[fresh[i]] = ids[i];
	}
	void removeObject(PhysicsObject& object)
	{
		const auto it = slot_of.find(&object);
		if (it == slot_of.end()) return;
		check(sgp_proximity_remove(batch, it->second), "sgp_proximity_remove");
		slot_of.erase(it); last_touch.erase(&object);
	}
	void clear()
	{
		for (const auto& kv : slot_of) check(sgp_proximity_remove(batch, kv.second), "sgp_proximity_remove");
		slot_of.clear(); last_touch.clear();
	}

	// world_state->parcels: an axis-aligned parcel by its id (among the parcels around a point the lowest id wins, as std::map order gives it)
	void addParcel(uint32_t parcel_id, const Vec4f& aabb_min, const Vec4f& aabb_max)
	{
		uint32_t z = 0;
		check(sgp_proximity_zone_add(batch, aabb_min.x, aabb_max.x, parcel_id, &z), "sgp_proximity_zone_add");
		zone_of[parcel_id] = z;
	}
	void removeParcel(uint32_t parcel_id)
	{
		const auto it = zone_of.find(parcel_id);
		if (it == zone_of.end()) return;
		check(sgp_proximity_zone_remove(batch, it->second), "sgp_proximity_zone_remove");
		zone_of.erase(it);
	}

	// further observers (other avatars this process hosts); observer 0 is the camera of think()
	void setObserver(uint32_t k, const Vec4f& pos)
	{
		sgp_proximity_observer o; memset(&o, 0, sizeof(o));
		o.source = SGP_PROX_OBS_POINT; o.pos[0] = pos[0]; o.pos[1] = pos[1]; o.pos[2] = pos[2];
		check(sgp_proximity_set_observer(batch, k, &o), "sgp_proximity_set_observer");
	}
	void setObserverOnBody(uint32_t k, PhysicsObject& object, const Vec4f& offset)
	{
		sgp_proximity_observer o; memset(&o, 0, sizeof(o));
		o.source = SGP_PROX_OBS_BODY; o.body = object.jolt_body_id.GetIndex(); o.offset[0] = offset[0]; o.offset[1] = offset[1]; o.offset[2] = offset[2];
		check(sgp_proximity_set_observer(batch, k, &o), "sgp_proximity_set_observer");
	}
	void removeObserver(uint32_t k) { check(sgp_proximity_remove_observer(batch, k), "sgp_proximity_remove_observer"); }

	// think(campos, world_state_lock): enqueued, not waited for.  Call it once per frame, after PhysicsWorld::think.
	void think(const Vec4f& campos)
	{
		setObserver(0, campos);
		check(sgp_proximity_update(batch), "sgp_proximity_update");
	}

	// waits for what is in flight; one call per event since the last drain, in the library's order.  Returns how many events the batch had to drop.
	uint32_t drain(const std::function<void(const Event&)>& callback)
	{
		events.resize(ev_cap);
		uint32_t n = 0, n_dropped = 0;
		check(sgp_proximity_drain_events(batch, events.data(), ev_cap, &n, &n_dropped), "sgp_proximity_drain_events");
		for (uint32_t i = 0; i < n; ++i) {
			const sgp_proximity_event& e = events[i];
			callback(Event{ (EventKind)e.kind, e.object == SGP_INVALID_ID ? nullptr : (PhysicsObject*)e.tag, e.observer, e.zone_key, e.update_index });
		}
		dropped += n_dropped;
		return n_dropped;
	}

	// in_script_proximity of an object for observer k, as the last update left it (waits)
	bool inProximity(PhysicsObject& object, uint32_t k = 0)
	{
		sgp_proximity_state s; memset(&s, 0, sizeof(s));
		check(sgp_proximity_get_states(batch, slot_of.at(&object), 1, &s), "sgp_proximity_get_states");
		return ((s.near_mask >> k) & 1u) != 0;
	}

	// The throttle of onUserTouchedObject (GUIClient.cpp:6464-6469): Jolt -- and the character batch -- raise contact-added records very fast; a watched object's
	// handler runs at most once per 0.5 s.  Feed it the userdata of a drained character contact (the PhysicsObject*); true: run the handler now.
	bool shouldFireTouchEvent(PhysicsObject* object, double cur_time)
	{
		if (!object || !slot_of.count(object)) return false;
		const auto it = last_touch.find(object);
		if (it != last_touch.end() && !(cur_time - it->second > 0.5)) return false;
		last_touch[object] = cur_time;
		return true;
	}
	template <class Contacts, class F> void touchEvents(const Contacts& contacts, double cur_time, F&& on_touched)
	{
		for (const auto& c : contacts) { PhysicsObject* ob = (PhysicsObject*)c.userdata; if (shouldFireTouchEvent(ob, cur_time)) on_touched(*ob, c.character); }
	}

	uint32_t numObjects() const { return (uint32_t)slot_of.size(); }
	uint64_t numDropped() const { return dropped; }
	sgp_proximity* handle() const { return batch; }

	// Extensions (not in the reference): the batch as it is now, to come back to after PhysicsWorld's rollback to the checkpoint of the same moment -- the
	// library's state (near bits, the observers' parcels, undrained events) and what this header keeps on the host: the objects' slots, the parcels' and the
	// touch clocks.
	struct SavedState { BatchCheckpoint lib; std::unordered_map<PhysicsObject*, uint32_t> slot_of; std::map<uint32_t, uint32_t> zone_of; std::unordered_map<PhysicsObject*, double> last_touch; uint64_t dropped = 0; };
	void saveState(SavedState& s)
	{
		check(sgp_proximity_checkpoint(batch, &s.lib.cp), "sgp_proximity_checkpoint");
		s.slot_of = slot_of; s.zone_of = zone_of; s.last_touch = last_touch; s.dropped = dropped;
	}
	void restoreState(const SavedState& s)
	{
		check(sgp_proximity_rollback(batch, s.lib.cp), "sgp_proximity_rollback");
		slot_of = s.slot_of; zone_of = s.zone_of; last_touch = s.last_touch; dropped = s.dropped;
	}

private:
	static void check(int rc, const char* what) { if (rc != SGP_OK) throw std::runtime_error(std::string(what) + ": " + sgp_last_error()); }

	PhysicsWorld* world;
	sgp_proximity* batch;
	uint32_t ev_cap;
	uint64_t dropped;
	std::unordered_map<PhysicsObject*, uint32_t> slot_of;
	std::map<uint32_t, uint32_t> zone_of;
	std::unordered_map<PhysicsObject*, double> last_touch;
	std::vector<sgp_proximity_event> events;
};
