// PlayerBatch: many PlayerPhysics-style players advanced by one call, with PlayerPhysics' names (gui_client/PlayerPhysics.h).  Code that keeps a vector of
// PlayerPhysics objects -- a server that owns many avatars or NPCs -- moves to this: every member takes the player's id first.  The velocity rule of
// PlayerPhysics::update runs on the device, in front of the character's ExtendedUpdate (sgp_characters_set_drive / _jump / _update_at, include/sgp.h,
// "driven characters"); the host sends what the players ask for and nothing else:
//   add(position)                          PlayerPhysics::init: capsule 0.3 / 1.3, up = z, supporting volume = lower sphere, max strength 1000, stick 0.5, stairs 0.4
//   processMoveForwards / StrafeRight / MoveUp / Jump, setFlyModeEnabled ...      summed on the host, where the reference sums them (move_speed 3, run factor 5)
//   update(dt, cur_time)                   sends what changed and enqueues the update: no read, no wait.  As in the reference, the CALLER zeroes move_desired_vel
//                                          (zeroMoveDesiredVel) once the frame's updates are done
//   readBack()                             waits and fetches; the getters answer from what it fetched
// What is left out against PlayerPhysics: docs/GAPS.md, "Driven characters against PlayerPhysics".
#pragma once
#include "Jolt/JoltCharacterLite.h"
#include "BatchCheckpoint.h"
#include <algorithm>
#include <stdexcept>
#include <string>
#include <vector>

class PlayerBatch
{
public:
	static constexpr float run_factor = 5, move_speed = 3, jump_speed = 4.5f, max_air_speed = 8;
	static constexpr float SPHERE_RAD = 0.3f, CYLINDER_HEIGHT = 1.3f, SITTING_HEIGHT = 0.3f, EYE_HEIGHT = 1.67f;

	PlayerBatch(JPH::PhysicsSystem* system, uint32_t capacity) : batch(nullptr), used(0)
	{
		check(sgp_characters_create(system->world, capacity, &batch), "sgp_characters_create");
		drives.resize(capacity); drive_dirty.assign(capacity, 0); inputs.resize(capacity); input_dirty.assign(capacity, 0); states.resize(capacity); drive_states.resize(capacity);
		for (uint32_t i = 0; i < capacity; ++i) resetSlot(i);
	}
	~PlayerBatch() { if (batch) sgp_characters_destroy(batch); }
	PlayerBatch(const PlayerBatch&) = delete;
	PlayerBatch& operator=(const PlayerBatch&) = delete;

	// PlayerPhysics::init; position: the capsule's bottom (the eye position less EYE_HEIGHT)
	uint32_t add(JPH::RVec3Arg bottom_position)
	{
		sgp_character_desc d;
		sgp_default_character_desc(&d);
		d.radius = SPHERE_RAD; d.half_height = 0.5f * CYLINDER_HEIGHT;
		d.shape_offset[0] = 0; d.shape_offset[1] = 0; d.shape_offset[2] = 0.5f * CYLINDER_HEIGHT + SPHERE_RAD;
		d.up[0] = 0; d.up[1] = 0; d.up[2] = 1;
		d.supporting_plane[0] = 0; d.supporting_plane[1] = 0; d.supporting_plane[2] = 1; d.supporting_plane[3] = -SPHERE_RAD;
		d.max_strength = 1000;
		d.stick_to_floor_step_down[0] = 0; d.stick_to_floor_step_down[1] = 0; d.stick_to_floor_step_down[2] = -0.5f;
		d.walk_stairs_step_up[0] = 0; d.walk_stairs_step_up[1] = 0; d.walk_stairs_step_up[2] = 0.4f;
		const float p[3] = { bottom_position.x, bottom_position.y, bottom_position.z };
		uint32_t id = 0;
		check(sgp_character_add(batch, &d, p, &id), "sgp_character_add");
		if (id + 1 > used) used = id + 1;
		resetSlot(id);
		drives[id].flags |= SGP_DRIVE_ON; drive_dirty[id] = 1; input_dirty[id] = 1;
		states[id].pos[0] = p[0]; states[id].pos[1] = p[1]; states[id].pos[2] = p[2];
		drive_states[id].cam_pos[0] = p[0]; drive_states[id].cam_pos[1] = p[1]; drive_states[id].cam_pos[2] = p[2] + EYE_HEIGHT;
		return id;
	}
	void remove(uint32_t id) { check(sgp_character_remove(batch, id), "sgp_character_remove"); }

	// ---- per-frame inputs (summed into move_desired_vel as the reference sums them) ----
	void processMoveForwards(uint32_t id, float factor, bool runpressed, const JPH::Vec3& forwards_vec) { addMove(id, forwards_vec * factor * move_speed * doRunFactor(runpressed)); setFlag(id, SGP_DRIVE_GRAVITY, true); }
	void processStrafeRight(uint32_t id, float factor, bool runpressed, const JPH::Vec3& right_vec) { addMove(id, right_vec * factor * move_speed * doRunFactor(runpressed)); setFlag(id, SGP_DRIVE_GRAVITY, true); }
	// (whether it counts -- flying, free camera, under water -- is decided on the device, where the feet's depth is known)
	void processMoveUp(uint32_t id, float factor, bool runpressed) { drives.at(id).move_up += factor * move_speed * doRunFactor(runpressed); drive_dirty[id] = 1; setFlag(id, SGP_DRIVE_GRAVITY, true); }
	void processJump(uint32_t id, double cur_time) { check(sgp_characters_jump(batch, &id, 1, cur_time), "sgp_characters_jump"); setFlag(id, SGP_DRIVE_GRAVITY, true); }
	void setFlyModeEnabled(uint32_t id, bool enabled) { setFlag(id, SGP_DRIVE_FLY, enabled); }
	bool flyModeEnabled(uint32_t id) const { return (drives.at(id).flags & SGP_DRIVE_FLY) != 0; }
	void setFreeCamera(uint32_t id, bool enabled) { setFlag(id, SGP_DRIVE_FREE_CAMERA, enabled); }
	void setGravityEnabled(uint32_t id, bool enabled) { setFlag(id, SGP_DRIVE_GRAVITY, enabled); }
	void setSmoothStairs(uint32_t id, bool enabled) { setFlag(id, SGP_DRIVE_SMOOTH_STAIRS, enabled); }      // (extension: SGP_DRIVE_SMOOTH_STAIRS)
	void setStandingShape(uint32_t id) { const float o[3] = { 0, 0, 0.5f * CYLINDER_HEIGHT + SPHERE_RAD }; check(sgp_characters_set_shape(batch, id, SPHERE_RAD, 0.5f * CYLINDER_HEIGHT, o), "sgp_characters_set_shape"); }
	void setSittingShape(uint32_t id) { const float o[3] = { 0, 0, 0.5f * SITTING_HEIGHT + SPHERE_RAD }; check(sgp_characters_set_shape(batch, id, SPHERE_RAD, 0.5f * SITTING_HEIGHT, o), "sgp_characters_set_shape"); }
	void setEyePosition(uint32_t id, JPH::RVec3Arg eye_pos, JPH::Vec3Arg linear_vel = JPH::Vec3(0, 0, 0)) { setCapsuleBottomPosition(id, eye_pos - JPH::Vec3(0, 0, EYE_HEIGHT), linear_vel); }
	void setCapsuleBottomPosition(uint32_t id, JPH::RVec3Arg pos, JPH::Vec3Arg linear_vel)
	{
		const float q[3] = { pos.x, pos.y, pos.z };
		check(sgp_characters_set_pose(batch, &id, q, 1), "sgp_characters_set_pose");
		setLinearVel(id, linear_vel);
	}
	// SetLinearVelocity: the next update's rule starts from it (a bounce pad; addToLinearVel is this with getLinearVel(id) + delta after a readBack)
	void setLinearVel(uint32_t id, JPH::Vec3Arg v) { sgp_character_input& in = inputs.at(id); in.velocity[0] = v.x; in.velocity[1] = v.y; in.velocity[2] = v.z; input_dirty[id] = 1; }
	void zeroMoveDesiredVel(uint32_t id) { sgp_character_drive& d = drives.at(id); if (d.move_desired_vel[0] != 0 || d.move_desired_vel[1] != 0 || d.move_desired_vel[2] != 0 || d.move_up != 0) drive_dirty[id] = 1; d.move_desired_vel[0] = d.move_desired_vel[1] = d.move_desired_vel[2] = 0; d.move_up = 0; }
	void zeroMoveDesiredVel() { for (uint32_t i = 0; i < used; ++i) zeroMoveDesiredVel(i); }
	bool isMoveDesiredVelNonZero(uint32_t id) const { const sgp_character_drive& d = drives.at(id); return d.move_desired_vel[0] != 0 || d.move_desired_vel[1] != 0 || d.move_desired_vel[2] != 0 || d.move_up != 0; }
	static float getEyeHeight() { return EYE_HEIGHT; }

	// PlayerPhysics::update for every player: what changed goes to the library, the update is enqueued.  No read, no wait.
	void update(float dt, double cur_time)
	{
		send();
		check(sgp_characters_update_at(batch, dt, cur_time), "sgp_characters_update_at");
	}

	// waits for the updates in flight; the getters below answer from what this fetched
	void readBack()
	{
		send();
		if (!used) return;
		check(sgp_characters_get_states(batch, 0, used, states.data()), "sgp_characters_get_states");
		check(sgp_characters_get_drive_states(batch, 0, used, drive_states.data()), "sgp_characters_get_drive_states");
	}
	JPH::RVec3 getCapsuleBottomPosition(uint32_t id) const { return vec(states.at(id).pos); }
	JPH::Vec3 getLinearVel(uint32_t id) const { return vec(states.at(id).lin_vel); }
	bool onGround(uint32_t id) const { return drive_states.at(id).on_ground != 0; }
	bool jumped(uint32_t id) const { return drive_states.at(id).jumped != 0; }      // UpdateEvents::jumped of the last update
	uint32_t numJumps(uint32_t id) const { return drive_states.at(id).num_jumps; }
	JPH::Vec3 camPos(uint32_t id) const { return vec(drive_states.at(id).cam_pos); }
	JPH::Vec3 getLastXYPlaneVelRelGround(uint32_t id) const { return vec(drive_states.at(id).last_xy_plane_vel_rel_ground); }
	bool isSupported(uint32_t id) const { const uint32_t s = states.at(id).ground_state; return s == SGP_GROUND_ON_GROUND || s == SGP_GROUND_ON_STEEP_GROUND; }
	const sgp_character_state& state(uint32_t id) const { return states.at(id); }
	const sgp_character_drive_state& driveState(uint32_t id) const { return drive_states.at(id); }
	// contacted_events' source (OnContactAdded) since the last call: ascending player, then order of discovery
	void drainContacts(std::vector<sgp_character_contact>& out)
	{
		out.resize((size_t)std::max<uint32_t>(used, 1u) * 32u);
		uint32_t n = 0;
		check(sgp_characters_drain_contacts(batch, out.data(), (uint32_t)out.size(), &n), "sgp_characters_drain_contacts");
		out.resize(std::min<size_t>(n, out.size()));
	}
	sgp_characters* handle() const { return batch; }

	// Extensions (not in the reference): the batch as it is now, to come back to after PhysicsWorld's rollback to the checkpoint of the same moment
	struct SavedState {
		BatchCheckpoint lib; std::vector<sgp_character_drive> drives; std::vector<sgp_character_input> inputs; std::vector<uint8_t> drive_dirty, input_dirty;
		std::vector<sgp_character_state> states; std::vector<sgp_character_drive_state> drive_states; uint32_t used = 0;
	};
	void saveState(SavedState& s)
	{
		check(sgp_characters_checkpoint(batch, &s.lib.cp), "sgp_characters_checkpoint");
		s.drives = drives; s.inputs = inputs; s.drive_dirty = drive_dirty; s.input_dirty = input_dirty; s.states = states; s.drive_states = drive_states; s.used = used;
	}
	void restoreState(const SavedState& s)
	{
		check(sgp_characters_rollback(batch, s.lib.cp), "sgp_characters_rollback");
		drives = s.drives; inputs = s.inputs; drive_dirty = s.drive_dirty; input_dirty = s.input_dirty; states = s.states; drive_states = s.drive_states; used = s.used;
	}

private:
	static float doRunFactor(bool runpressed) { return runpressed ? run_factor : 1.0f; }
	static JPH::Vec3 vec(const float* p) { return JPH::Vec3(p[0], p[1], p[2]); }
	void addMove(uint32_t id, const JPH::Vec3& v) { sgp_character_drive& d = drives.at(id); d.move_desired_vel[0] += v.x; d.move_desired_vel[1] += v.y; d.move_desired_vel[2] += v.z; drive_dirty[id] = 1; }
	void setFlag(uint32_t id, uint32_t flag, bool on) { uint32_t& f = drives.at(id).flags; const uint32_t nf = on ? (f | flag) : (f & ~flag); if (nf != f) { f = nf; drive_dirty[id] = 1; } }
	void resetSlot(uint32_t i)
	{
		sgp_default_character_drive(&drives[i]); drive_dirty[i] = 0;
		sgp_character_input& in = inputs[i]; in.velocity[0] = in.velocity[1] = in.velocity[2] = 0.0f; in.ignore_id = SGP_INVALID_ID; in.flags = SGP_CHAR_EXTENDED; input_dirty[i] = 0;
		states[i] = sgp_character_state(); states[i].ground_state = SGP_GROUND_IN_AIR; states[i].ground_body = SGP_INVALID_ID;
		drive_states[i] = sgp_character_drive_state();
	}
	// what was set since the last call, in runs of consecutive ids
	template <class T, class F> void sendRuns(std::vector<uint8_t>& dirty, const std::vector<T>& recs, F&& call)
	{
		for (uint32_t i = 0; i < used;) {
			if (!dirty[i]) { ++i; continue; }
			uint32_t j = i; while (j < used && dirty[j]) dirty[j++] = 0;
			call(i, j - i, recs.data() + i);
			i = j;
		}
	}
	void send()
	{
		sendRuns(input_dirty, inputs, [this](uint32_t first, uint32_t n, const sgp_character_input* p) { check(sgp_characters_set_inputs(batch, first, n, p), "sgp_characters_set_inputs"); });
		sendRuns(drive_dirty, drives, [this](uint32_t first, uint32_t n, const sgp_character_drive* p) { check(sgp_characters_set_drive(batch, first, n, p), "sgp_characters_set_drive"); });
	}
	static void check(int rc, const char* what) { if (rc != SGP_OK) throw std::runtime_error(std::string(what) + ": " + sgp_last_error()); }

	sgp_characters* batch;
	std::vector<sgp_character_drive> drives; std::vector<uint8_t> drive_dirty;
	std::vector<sgp_character_input> inputs; std::vector<uint8_t> input_dirty;
	std::vector<sgp_character_state> states; std::vector<sgp_character_drive_state> drive_states;
	uint32_t used;
};
