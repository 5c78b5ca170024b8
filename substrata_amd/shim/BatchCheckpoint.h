// BatchCheckpoint: the library's checkpoint of one batch (sgp_batch_checkpoint, include/sgp.h) as an object the SavedState of CharacterBatch, ParticleBatch,
// CraftBatch and MoverBatch keeps next to the facade's own host state.  saveState overwrites it in place, so a SavedState that is kept and saved into every
// frame allocates once.  It may outlive its batch and its world.
#pragma once
#include "../../include/sgp.h"

struct BatchCheckpoint
{
	BatchCheckpoint() : cp(nullptr) {}
	~BatchCheckpoint() { sgp_batch_checkpoint_destroy(cp); }
	BatchCheckpoint(const BatchCheckpoint&) = delete;
	BatchCheckpoint& operator=(const BatchCheckpoint&) = delete;
	sgp_batch_checkpoint_info info() const { sgp_batch_checkpoint_info i = sgp_batch_checkpoint_info(); if (cp) sgp_batch_checkpoint_get_info(cp, &i); return i; }
	sgp_batch_checkpoint* cp;
};
