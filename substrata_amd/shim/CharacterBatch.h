// CharacterBatch: many JPH::CharacterVirtual-style characters advanced by one call (sgp_characters_*, include/sgp.h).
// Code that keeps a vector of PlayerPhysics-style characters -- a server that owns many avatars or NPCs -- moves to this: the settings are
// JPH::CharacterVirtualSettings and CharacterVirtual::ExtendedUpdateSettings, the answers EGroundState and BodyID, and a character of the batch moves as
// the JPH::CharacterVirtual of Jolt/JoltCharacterLite.h with the same settings moves.  What a CharacterContactListener did:
//   OnContactAdded  -> drainContacts(): one record per (body, sub shape) a character newly touches
//   OnContactSolve  -> PlayerPhysics' anti-sliding rule is built in: setAllowSliding(id, false)      (PlayerPhysics.cpp:536-545)
//   IgnoreSingleBodyFilter -> setIgnoredBody(id, body)                                             (PlayerPhysics.cpp:477)
// update() enqueues the work on the world's stream and returns; readBack() waits and fetches the states the getters then answer from.
#pragma once
#include "Jolt/JoltCharacterLite.h"
#include "BatchCheckpoint.h"
#include <stdexcept>
#include <string>
#include <vector>

class CharacterBatch
{
public:
	typedef JPH::CharacterBase::EGroundState EGroundState;

	CharacterBatch(JPH::PhysicsSystem* system, uint32_t capacity) : physics_system(system), batch(nullptr)
	{
		check(sgp_characters_create(system->world, capacity, &batch), "sgp_characters_create");
		inputs.resize(capacity); states.resize(capacity); dirty.assign(capacity, 0); used = 0; inputs_dirty = false;
		for (sgp_character_input& in : inputs) { in.velocity[0] = in.velocity[1] = in.velocity[2] = 0.0f; in.ignore_id = SGP_INVALID_ID; in.flags = SGP_CHAR_EXTENDED; }
		for (sgp_character_state& s : states) { s = sgp_character_state(); s.ground_state = SGP_GROUND_IN_AIR; s.ground_body = SGP_INVALID_ID; }
	}
	~CharacterBatch() { if (batch) sgp_characters_destroy(batch); }
	CharacterBatch(const CharacterBatch&) = delete;
	CharacterBatch& operator=(const CharacterBatch&) = delete;

	static sgp_character_desc makeDesc(const JPH::CharacterVirtualSettings& s, const JPH::CharacterVirtual::ExtendedUpdateSettings& ext)
	{
		sgp_character_desc d;
		sgp_default_character_desc(&d);
		if (s.mShape.GetPtr()) { d.radius = s.mShape->radius; d.half_height = s.mShape->half_height; set3(d.shape_offset, s.mShape->offset); }
		set3(d.up, s.mUp);
		set3(d.supporting_plane, s.mSupportingVolume.n); d.supporting_plane[3] = s.mSupportingVolume.c;
		d.max_slope_angle = s.mMaxSlopeAngle; d.mass = s.mMass; d.max_strength = s.mMaxStrength;
		d.predictive_contact_distance = s.mPredictiveContactDistance; d.character_padding = s.mCharacterPadding;
		d.penetration_recovery_speed = s.mPenetrationRecoverySpeed; d.collision_tolerance = s.mCollisionTolerance;
		d.max_collision_iterations = s.mMaxCollisionIterations; d.max_constraint_iterations = s.mMaxConstraintIterations; d.min_time_remaining = s.mMinTimeRemaining;
		set3(d.stick_to_floor_step_down, ext.mStickToFloorStepDown); set3(d.walk_stairs_step_up, ext.mWalkStairsStepUp);
		d.walk_stairs_min_step_forward = ext.mWalkStairsMinStepForward; d.walk_stairs_step_forward_test = ext.mWalkStairsStepForwardTest;
		d.walk_stairs_cos_angle_forward_contact = ext.mWalkStairsCosAngleForwardContact; set3(d.walk_stairs_step_down_extra, ext.mWalkStairsStepDownExtra);
		return d;
	}

	uint32_t add(const JPH::CharacterVirtualSettings& s, const JPH::CharacterVirtual::ExtendedUpdateSettings& ext, JPH::RVec3Arg position)
	{
		const sgp_character_desc d = makeDesc(s, ext);
		const float p[3] = { position.x, position.y, position.z };
		uint32_t id = 0;
		check(sgp_character_add(batch, &d, p, &id), "sgp_character_add");
		if (id + 1 > used) used = id + 1;
		sgp_character_input& in = inputs[id];
		in.velocity[0] = in.velocity[1] = in.velocity[2] = 0.0f; in.ignore_id = SGP_INVALID_ID; in.flags = SGP_CHAR_EXTENDED; touch(id);
		sgp_character_state& st = states[id];
		st = sgp_character_state(); st.pos[0] = p[0]; st.pos[1] = p[1]; st.pos[2] = p[2]; st.ground_state = SGP_GROUND_IN_AIR; st.ground_body = SGP_INVALID_ID;
		return id;
	}
	void remove(uint32_t id) { check(sgp_character_remove(batch, id), "sgp_character_remove"); }

	// what the caller sets per frame (they stay in force until set again)
	void SetLinearVelocity(uint32_t id, JPH::Vec3Arg v) { set3(inputs.at(id).velocity, v); touch(id); }
	void SetPosition(uint32_t id, JPH::RVec3Arg p) { const float q[3] = { p.x, p.y, p.z }; check(sgp_characters_set_pose(batch, &id, q, 1), "sgp_characters_set_pose"); }
	void SetShape(uint32_t id, const JPH::CharacterShape& shape) { const float o[3] = { shape.offset.x, shape.offset.y, shape.offset.z }; check(sgp_characters_set_shape(batch, id, shape.radius, shape.half_height, o), "sgp_characters_set_shape"); }
	void setIgnoredBody(uint32_t id, const JPH::BodyID& body) { inputs.at(id).ignore_id = body.IsInvalid() ? SGP_INVALID_ID : body.GetIndex(); touch(id); }
	void setAllowSliding(uint32_t id, bool allow) { setFlag(id, SGP_CHAR_NO_SLIDE, !allow); }
	void setExtendedUpdate(uint32_t id, bool extended) { setFlag(id, SGP_CHAR_EXTENDED, extended); }      // false: the plain Update of PlayerPhysics::updateForInVehicle
	void setEnabled(uint32_t id, bool enabled) { setFlag(id, SGP_CHAR_DISABLED, !enabled); }

	// CharacterVirtual::Update / ExtendedUpdate for every character: enqueued, not waited for
	void update(float dt)
	{
		sendInputs();
		check(sgp_characters_update(batch, dt), "sgp_characters_update");
	}
	// waits for the updates in flight; the getters below answer from what this fetched
	void readBack()
	{
		sendInputs();
		if (used) check(sgp_characters_get_states(batch, 0, used, states.data()), "sgp_characters_get_states");
	}
	JPH::RVec3 GetPosition(uint32_t id) const { return vec(states.at(id).pos); }
	JPH::Vec3 GetLinearVelocity(uint32_t id) const { return vec(states.at(id).lin_vel); }
	EGroundState GetGroundState(uint32_t id) const { return (EGroundState)states.at(id).ground_state; }
	bool IsSupported(uint32_t id) const { const EGroundState s = GetGroundState(id); return s == EGroundState::OnGround || s == EGroundState::OnSteepGround; }
	JPH::Vec3 GetGroundNormal(uint32_t id) const { return vec(states.at(id).ground_normal); }
	JPH::Vec3 GetGroundVelocity(uint32_t id) const { return vec(states.at(id).ground_velocity); }
	JPH::RVec3 GetGroundPosition(uint32_t id) const { return vec(states.at(id).ground_position); }
	JPH::BodyID GetGroundBodyID(uint32_t id) const { const uint32_t b = states.at(id).ground_body; return b == SGP_INVALID_ID ? JPH::BodyID() : JPH::BodyID(b); }
	JPH::SubShapeID GetGroundSubShapeID(uint32_t id) const { return physics_system->subShapeID(GetGroundBodyID(id), states.at(id).ground_sub_shape); }
	uint64_t GetGroundUserData(uint32_t id) const { return states.at(id).ground_userdata; }
	bool overflowed(uint32_t id) const { return states.at(id).overflow != 0; }
	const sgp_character_state& state(uint32_t id) const { return states.at(id); }

	// OnContactAdded since the last call: ascending character, then order of discovery
	void drainContacts(std::vector<sgp_character_contact>& out)
	{
		out.resize((size_t)std::max<uint32_t>(used, 1u) * 32u);      // (a character holds at most 32 records between drains)
		uint32_t n = 0;
		check(sgp_characters_drain_contacts(batch, out.data(), (uint32_t)out.size(), &n), "sgp_characters_drain_contacts");
		out.resize(std::min<size_t>(n, out.size()));
	}
	sgp_characters* handle() const { return batch; }

	// Extensions (not in the reference): the batch as it is now, to come back to after PhysicsWorld's rollback to the checkpoint of the same moment -- the
	// library's state and, with it, the inputs set here and not sent yet and what the last readBack() fetched.
	struct SavedState { BatchCheckpoint lib; std::vector<sgp_character_input> inputs; std::vector<sgp_character_state> states; std::vector<uint8_t> dirty; uint32_t used = 0; bool inputs_dirty = false; };
	void saveState(SavedState& s)
	{
		check(sgp_characters_checkpoint(batch, &s.lib.cp), "sgp_characters_checkpoint");
		s.inputs = inputs; s.states = states; s.dirty = dirty; s.used = used; s.inputs_dirty = inputs_dirty;
	}
	void restoreState(const SavedState& s)
	{
		check(sgp_characters_rollback(batch, s.lib.cp), "sgp_characters_rollback");
		inputs = s.inputs; states = s.states; dirty = s.dirty; used = s.used; inputs_dirty = s.inputs_dirty;
	}

private:
	static void set3(float* d, const JPH::Vec3& v) { d[0] = v.x; d[1] = v.y; d[2] = v.z; }
	static JPH::Vec3 vec(const float* p) { return JPH::Vec3(p[0], p[1], p[2]); }
	void setFlag(uint32_t id, uint32_t flag, bool on) { uint32_t& f = inputs.at(id).flags; f = on ? (f | flag) : (f & ~flag); touch(id); }
	void touch(uint32_t id) { dirty.at(id) = 1; inputs_dirty = true; }
	// the inputs that were set since the last call, in runs of consecutive ids: a character whose caller set nothing keeps the velocity it has (as
	// CharacterVirtual keeps what CancelVelocityTowardsSteepSlopes left of it)
	void sendInputs()
	{
		if (!inputs_dirty) return;
		for (uint32_t i = 0; i < used;) {
			if (!dirty[i]) { ++i; continue; }
			uint32_t j = i; while (j < used && dirty[j]) dirty[j++] = 0;
			check(sgp_characters_set_inputs(batch, i, j - i, inputs.data() + i), "sgp_characters_set_inputs");
			i = j;
		}
		inputs_dirty = false;
	}
	static void check(int rc, const char* what) { if (rc != SGP_OK) throw std::runtime_error(std::string(what) + ": " + sgp_last_error()); }

	JPH::PhysicsSystem* physics_system;
	sgp_characters* batch;
	std::vector<sgp_character_input> inputs; std::vector<sgp_character_state> states; std::vector<uint8_t> dirty;
	uint32_t used; bool inputs_dirty;
};
