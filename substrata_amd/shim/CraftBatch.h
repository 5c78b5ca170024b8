// CraftBatch: HoverCarPhysics and BoatPhysics (gui_client/HoverCarPhysics.h/.cpp, BoatPhysics.h/.cpp) for many craft on the device (sgp_crafts_*, include/sgp.h).
// A HoverCarPhysics or BoatPhysics reads its body back every sub-step, evaluates its control, drag and lift on the host and sends the forces one call at a
// time; with a batch the crafts live on the device, update(dt) enqueues HoverCarPhysics::update / BoatPhysics::update for all of them on the world's stream
// and returns, and the dust, spray and foam they raise go to an attached ParticleBatch without leaving the device.  What the controllers did with key states
// stays here: setInput() maps a PlayerPhysicsInput to the resolved values the library takes (HoverCarPhysics.cpp:82-110, BoatPhysics.cpp:110-131).
// Colour and sprite type of a particle follow from the kind in its tag (SGP_CRAFT_PK_*): bits 28..31 of the low word.
// Departures from the controllers (docs/GAPS.md): the random numbers are the library's counter-based generator, and PhysicsWorld::think must be called one
// sub-step at a time between updates (the reference updates its vehicles per sub-step).
#pragma once
#include "../../include/sgp.h"
#include "Jolt/JoltLite.h"
#include "ParticleBatch.h"
#include "maths/Quat.h"
#include "maths/Vec4f.h"
#include <algorithm>
#include <stdexcept>
#include <string>
#include <vector>

// gui_client/PlayerPhysicsInput.h: the key and pad state a vehicle controller is updated with
struct PlayerPhysicsInput
{
	PlayerPhysicsInput() { clear(); }
	void clear()
	{
		SHIFT_down = CTRL_down = A_down = W_down = S_down = D_down = space_down = B_down = C_down = left_down = right_down = up_down = down_down = false;
		left_trigger = right_trigger = axis_left_x = axis_left_y = 0;
	}
	bool SHIFT_down, CTRL_down, A_down, W_down, S_down, D_down, space_down, B_down, C_down, left_down, right_down, up_down, down_down;
	float left_trigger, right_trigger, axis_left_x, axis_left_y;
};

// Scripting::VehicleScriptedSettings, the part both controllers read
struct CraftScriptSettings
{
	CraftScriptSettings() { model_to_y_forwards_rot_1.v = Vec4f(0, 0, 0, 1); model_to_y_forwards_rot_2.v = Vec4f(0, 0, 0, 1); }
	Quatf model_to_y_forwards_rot_1, model_to_y_forwards_rot_2;
};
// HoverCarPhysics.h:29-35
struct HoverCarPhysicsSettings
{
	HoverCarPhysicsSettings() : hovercar_mass(1000.f), trace_origin_os(0, 0, 0, 1) {}
	CraftScriptSettings script_settings;
	float hovercar_mass;
	Vec4f trace_origin_os;      // HoverCarPhysics.cpp:331-337 computes it from the mesh's AABB and the object's scale every update; here the caller does, once
};
// Scripting.h:97-122
struct BoatScriptSettings : CraftScriptSettings
{
	struct SplashPoint { Vec4f point_os; float right_sign; };
	BoatScriptSettings() : thrust_force(40000.f), propellor_point_os(0, 0.2f, -6.2f, 1), propellor_sideways_offset(1.f), rudder_deflection_force_factor(500.f), thrust_vector_lateral_amount(0.f),
		jet_particle_initial_width(1.f), front_cross_sectional_area(2.f), side_cross_sectional_area(4.f), top_cross_sectional_area(8.f) {}
	float thrust_force;
	Vec4f propellor_point_os;
	float propellor_sideways_offset, rudder_deflection_force_factor, thrust_vector_lateral_amount, jet_particle_initial_width;
	float front_cross_sectional_area, side_cross_sectional_area, top_cross_sectional_area;
	std::vector<SplashPoint> splash_points;
};
// BoatPhysics.h:28-34
struct BoatPhysicsSettings
{
	BoatPhysicsSettings() : boat_mass(1000.f) {}
	BoatScriptSettings script_settings;
	float boat_mass;
};

class CraftBatch
{
public:
	CraftBatch(JPH::PhysicsSystem* system, uint32_t capacity) : batch(nullptr), cap(capacity) { check(sgp_crafts_create(system->world, capacity, &batch), "sgp_crafts_create"); inputs.resize(capacity); kinds.resize(capacity); }
	~CraftBatch() { if (batch) sgp_crafts_destroy(batch); }
	CraftBatch(const CraftBatch&) = delete;
	CraftBatch& operator=(const CraftBatch&) = delete;

	// HoverCarPhysics(object, car_body_id, settings, physics_world, particle_manager)
	uint32_t addHoverCar(JPH::BodyID car_body_id, const HoverCarPhysicsSettings& settings, uint32_t seed = 0, uint64_t tag = 0)
	{
		sgp_craft_desc d;
		sgp_default_craft_desc(SGP_CRAFT_HOVERCAR, &d);
		d.body = car_body_id.GetIndex(); d.mass = settings.hovercar_mass; d.seed = seed; d.tag = tag;
		setRotations(d, settings.script_settings);
		for (int k = 0; k < 3; ++k) d.trace_origin_os[k] = settings.trace_origin_os[k];
		return add(d);
	}
	// BoatPhysics(object, body_id, settings, physics_world, particle_manager, terrain_decal_manager).  The object's body must have been created with
	// PhysicsObject::use_zero_linear_drag = true (BoatPhysics.cpp:36 sets it afterwards; the library reads it when the body is added).
	uint32_t addBoat(JPH::BodyID body_id, const BoatPhysicsSettings& settings, uint32_t seed = 0, uint64_t tag = 0)
	{
		const BoatScriptSettings& s = settings.script_settings;
		if (s.splash_points.size() > SGP_CRAFT_MAX_SPLASH_POINTS) throw std::runtime_error("CraftBatch::addBoat: more than SGP_CRAFT_MAX_SPLASH_POINTS splash points");
		sgp_craft_desc d;
		sgp_default_craft_desc(SGP_CRAFT_BOAT, &d);
		d.body = body_id.GetIndex(); d.mass = settings.boat_mass; d.seed = seed; d.tag = tag;
		setRotations(d, s);
		d.thrust_force = s.thrust_force;
		for (int k = 0; k < 3; ++k) d.propellor_point_os[k] = s.propellor_point_os[k];
		d.propellor_sideways_offset = s.propellor_sideways_offset; d.rudder_deflection_force_factor = s.rudder_deflection_force_factor;
		d.thrust_vector_lateral_amount = s.thrust_vector_lateral_amount; d.jet_particle_initial_width = s.jet_particle_initial_width;
		d.front_cross_sectional_area = s.front_cross_sectional_area; d.side_cross_sectional_area = s.side_cross_sectional_area; d.top_cross_sectional_area = s.top_cross_sectional_area;
		d.n_splash_points = (uint32_t)s.splash_points.size();
		for (size_t p = 0; p < s.splash_points.size(); ++p) {
			for (int k = 0; k < 3; ++k) d.splash_points[4 * p + k] = s.splash_points[p].point_os[k];
			d.splash_points[4 * p + 3] = s.splash_points[p].right_sign;
		}
		return add(d);
	}
	void remove(uint32_t craft) { check(sgp_craft_remove(batch, craft), "sgp_craft_remove"); }

	// userEnteredVehicle / userExitedVehicle: seat 0 is the driver's (entering a boat stops its righting, BoatPhysics.cpp:80)
	void userEnteredVehicle(uint32_t craft, int seat_index) { if (seat_index == 0) { inputs.at(craft).flags |= SGP_CRAFT_IN_DRIVER; dirty = true; } }
	void userExitedVehicle(uint32_t craft, int old_seat_index) { if (old_seat_index == 0) { inputs.at(craft).flags &= ~SGP_CRAFT_IN_DRIVER; dirty = true; } }
	void startRightingVehicle(uint32_t craft) { flushInputs(); check(sgp_crafts_start_righting(batch, &craft, 1), "sgp_crafts_start_righting"); }

	// the physics_input argument of update(): kept until set again
	void setInput(uint32_t craft, const PlayerPhysicsInput& in)
	{
		sgp_craft_input& o = inputs.at(craft);
		float forward = 0.f, right = 0.f, up = 0.f, hand_brake = 0.f;
		if (kinds[craft] == SGP_CRAFT_HOVERCAR) {
			// HoverCarPhysics.cpp:82-110
			forward = -in.axis_left_y;
			if (in.W_down || in.up_down) forward = 1.f;
			else if (in.S_down || in.down_down) forward = -1.f;
			up = in.right_trigger - in.left_trigger;
			if (in.space_down) { hand_brake = 1.f; up = 1.f; }
			if (in.C_down) up = -1.f;
			right = in.axis_left_x;
			if (in.A_down) right = -1.f;
			else if (in.D_down) right = 1.f;
		} else {
			// BoatPhysics.cpp:110-131
			if (in.W_down || in.up_down) forward = 1.f;
			else if (in.S_down || in.down_down) forward = -1.f;
			if (in.SHIFT_down) forward *= 2.f;
			if (forward == 0.f) forward = std::max(in.left_trigger, in.right_trigger) * 2.f;
			if (forward < 0.f) forward *= 0.2f;
			right = in.axis_left_x;
			if (in.A_down) right = -1.f;
			else if (in.D_down) right = 1.f;
		}
		o.forward = forward; o.right = right; o.up = up; o.hand_brake = hand_brake;
		o.flags = (o.flags & SGP_CRAFT_IN_DRIVER) | (in.SHIFT_down ? SGP_CRAFT_IN_BOOST : 0u);
		dirty = true;
	}

	// particle_manager of the controllers: where the dust, spray and foam go (nullptr: nowhere).  Its capacity must be at least capacity() * SGP_CRAFT_MAX_EMIT.
	void attachParticles(ParticleBatch* particles) { check(sgp_crafts_attach_particles(batch, particles ? particles->handle() : nullptr), "sgp_crafts_attach_particles"); }

	// update(physics_world, physics_input, dtime) of every craft: enqueued, not waited for.  Call it once per sub-step, before PhysicsWorld::think(dtime).
	void update(float dtime) { flushInputs(); check(sgp_crafts_update(batch, dtime), "sgp_crafts_update"); }

	// waits for what is in flight
	const std::vector<sgp_craft_state>& readBack()
	{
		flushInputs();
		states.resize(cap);
		check(sgp_crafts_get_states(batch, 0, cap, states.data()), "sgp_crafts_get_states");
		return states;
	}
	Vec4f getLastTraceOrigin(uint32_t craft) const { const sgp_craft_state& s = states.at(craft); return Vec4f(s.trace_origin[0], s.trace_origin[1], s.trace_origin[2], 1); }      // last_trace_origin_ws, as of the last readBack()
	uint32_t capacity() const { return cap; }
	sgp_crafts* handle() const { return batch; }

	// Extensions (not in the reference): the batch as it is now, to come back to after PhysicsWorld's rollback to the checkpoint of the same moment -- the
	// library's state and, with it, the inputs set here and not sent yet and what the last readBack() fetched.  The attached ParticleBatch is saved and restored
	// by its own pair; which one is attached is not state.
	struct SavedState { BatchCheckpoint lib; std::vector<sgp_craft_input> inputs; std::vector<uint32_t> kinds; std::vector<sgp_craft_state> states; uint32_t high = 0; bool dirty = false; };
	void saveState(SavedState& s)
	{
		check(sgp_crafts_checkpoint(batch, &s.lib.cp), "sgp_crafts_checkpoint");
		s.inputs = inputs; s.kinds = kinds; s.states = states; s.high = high; s.dirty = dirty;
	}
	void restoreState(const SavedState& s)
	{
		check(sgp_crafts_rollback(batch, s.lib.cp), "sgp_crafts_rollback");
		inputs = s.inputs; kinds = s.kinds; states = s.states; high = s.high; dirty = s.dirty;
	}

private:
	static void check(int rc, const char* what) { if (rc != SGP_OK) throw std::runtime_error(std::string(what) + ": " + sgp_last_error()); }
	static void setRotations(sgp_craft_desc& d, const CraftScriptSettings& s)
	{
		for (int k = 0; k < 4; ++k) { d.model_to_y_forwards_rot_1[k] = s.model_to_y_forwards_rot_1.v[k]; d.model_to_y_forwards_rot_2[k] = s.model_to_y_forwards_rot_2.v[k]; }
	}
	uint32_t add(const sgp_craft_desc& d)
	{
		uint32_t id = 0;
		check(sgp_craft_add(batch, &d, &id), "sgp_craft_add");
		inputs[id] = sgp_craft_input(); kinds[id] = d.kind; high = std::max(high, id + 1u);
		return id;
	}
	void flushInputs()
	{
		if (dirty && high) check(sgp_crafts_set_inputs(batch, 0, high, inputs.data()), "sgp_crafts_set_inputs");
		dirty = false;
	}

	sgp_crafts* batch;
	uint32_t cap, high = 0;
	bool dirty = false;
	std::vector<sgp_craft_input> inputs;
	std::vector<uint32_t> kinds;
	std::vector<sgp_craft_state> states;
};
