// ParticleBatch: the simulation half of ParticleManager (gui_client/ParticleManager.h/.cpp) on the device (sgp_particles_*, include/sgp.h).
// A ParticleManager keeps a std::vector<Particle> and walks it every frame with one traceRay per particle; with a batch the particles live on the
// device, think(dt) enqueues ParticleManager::think for all of them on the world's stream and returns, and readBack() waits and fetches what the
// renderer needs.  What the manager did with its OpenGLEngine and TerrainDecalManager stays with the caller, keyed by Particle::tag (in place of gl_ob):
//   opengl_engine->updateObjectTransformData  -> for every record of live():    translation = pos, uniform scale = width        (ParticleManager.cpp:250-253)
//   opengl_engine->removeObject               -> for every event with SGP_PARTICLE_EV_DIED or _REPLACED                         (:96, :262)
//   terrain_decal_manager->addFoamDecal       -> for every event with SGP_PARTICLE_EV_FOAM: (pos.x, pos.y, water_z), foam_width (:203-205)
// Departures from the manager (docs/GAPS.md): survivors keep their order when the dead are removed, and a full batch replaces its particles in
// round-robin slot order instead of at random.  The capacity is the caller's (the manager's 2048 came from its host loop).
#pragma once
#include "../../include/sgp.h"
#include "Jolt/JoltLite.h"
#include "BatchCheckpoint.h"
#include "maths/Vec4f.h"
#include <algorithm>
#include <stdexcept>
#include <string>
#include <vector>

// ParticleManager.h:25-60, with `tag` in place of gl_ob
struct Particle
{
	enum ParticleType { ParticleType_Smoke, ParticleType_Foam };

	Particle() : pos(0, 0, 0, 1), vel(0, 0, 0, 0), tag(0), area(1.0e-6f), mass(1.0e-6f), restitution(0.5f), width(1.f), dwidth_dt(0.5f), cur_opacity(1.f), dopacity_dt(-0.3f), theta(0.f),
		die_when_hit_surface(false), particle_type(ParticleType_Smoke) { colour[0] = colour[1] = colour[2] = 0.8f; }

	Vec4f pos;
	Vec4f vel;
	uint64_t tag;        // the caller's handle of the sprite (the reference's GLObjectRef gl_ob)
	float colour[3];     // render-only: stays with the caller
	float area;
	float mass;
	float restitution;
	float width;
	float dwidth_dt;
	float cur_opacity;
	float dopacity_dt;
	float theta;         // render-only
	bool die_when_hit_surface;
	ParticleType particle_type;      // render-only
};

class ParticleBatch
{
public:
	ParticleBatch(JPH::PhysicsSystem* system, uint32_t capacity, uint32_t event_capacity = 4096) : batch(nullptr), cap(capacity), ev_cap(event_capacity)
	{
		check(sgp_particles_create(system->world, capacity, event_capacity, &batch), "sgp_particles_create");
	}
	~ParticleBatch() { if (batch) sgp_particles_destroy(batch); }
	ParticleBatch(const ParticleBatch&) = delete;
	ParticleBatch& operator=(const ParticleBatch&) = delete;

	static sgp_particle makeRecord(const Particle& p)
	{
		sgp_particle r;
		sgp_default_particle(&r);
		for (int k = 0; k < 3; ++k) { r.pos[k] = p.pos[k]; r.vel[k] = p.vel[k]; }
		r.area = p.area; r.mass = p.mass; r.restitution = p.restitution; r.width = p.width; r.dwidth_dt = p.dwidth_dt;
		r.opacity = p.cur_opacity; r.dopacity_dt = p.dopacity_dt; r.flags = p.die_when_hit_surface ? SGP_PARTICLE_DIE_ON_HIT : 0u; r.tag = p.tag;
		return r;
	}

	// addParticle (ParticleManager.cpp:84-142): queued here, sent with the next think() / readBack() / flush() in one call
	void addParticle(const Particle& particle) { pending.push_back(makeRecord(particle)); }
	void flush()
	{
		for (size_t i = 0; i < pending.size(); i += cap) check(sgp_particles_add(batch, pending.data() + i, (uint32_t)std::min<size_t>(cap, pending.size() - i)), "sgp_particles_add");
		pending.clear();
	}
	// think (ParticleManager.cpp:145-274) for every particle: enqueued, not waited for
	void think(float dt) { flush(); check(sgp_particles_update(batch, dt), "sgp_particles_update"); }
	void clearParticles() { pending.clear(); check(sgp_particles_clear(batch), "sgp_particles_clear"); }
	// waits for what is in flight; live() and events() answer from what this fetched
	void readBack()
	{
		flush();
		states.resize(cap);
		uint32_t n = 0;
		check(sgp_particles_read(batch, states.data(), cap, &n), "sgp_particles_read");
		states.resize(std::min(n, cap));
		evs.resize(ev_cap);
		uint32_t ne = 0, nd = 0;
		check(sgp_particles_drain_events(batch, evs.data(), ev_cap, &ne, &nd), "sgp_particles_drain_events");
		evs.resize(std::min(ne, ev_cap)); dropped = nd;
	}
	const std::vector<sgp_particle_state>& live() const { return states; }        // (tag, pos, width) of every live particle, in slot order
	const std::vector<sgp_particle_event>& events() const { return evs; }         // since the previous readBack(), in order
	uint32_t eventsDropped() const { return dropped; }                            // ... and how many did not fit event_capacity
	sgp_particles* handle() const { return batch; }

	// Extensions (not in the reference): the batch as it is now, to come back to after PhysicsWorld's rollback to the checkpoint of the same moment -- the
	// library's state and, with it, the particles queued here and not sent yet and what the last readBack() fetched.  Nothing is sent or waited for.
	struct SavedState { BatchCheckpoint lib; std::vector<sgp_particle> pending; std::vector<sgp_particle_state> states; std::vector<sgp_particle_event> evs; uint32_t dropped = 0; };
	void saveState(SavedState& s)
	{
		check(sgp_particles_checkpoint(batch, &s.lib.cp), "sgp_particles_checkpoint");
		s.pending = pending; s.states = states; s.evs = evs; s.dropped = dropped;
	}
	void restoreState(const SavedState& s)
	{
		check(sgp_particles_rollback(batch, s.lib.cp), "sgp_particles_rollback");
		pending = s.pending; states = s.states; evs = s.evs; dropped = s.dropped;
	}

private:
	static void check(int rc, const char* what) { if (rc != SGP_OK) throw std::runtime_error(std::string(what) + ": " + sgp_last_error()); }

	sgp_particles* batch;
	uint32_t cap, ev_cap, dropped = 0;
	std::vector<sgp_particle> pending;
	std::vector<sgp_particle_state> states;
	std::vector<sgp_particle_event> evs;
};
