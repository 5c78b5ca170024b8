// sgp_k_characters_driven.hip -- A7 -- the character update of a batch that has driven characters (SGP_DRIVE_ON: PlayerPhysics::update's velocity rule in front of
// CharacterVirtual::Update / ExtendedUpdate).  A stage file of its own, so that k_characters_update of sgp_k_characters.hip stays the code it was: see
// sgp_dev_character_update.h.
#include "sgp_dev_character_update.h"

void launch_characters_update_driven(const DV* d_dev, const CharBufs& b, float dt, const CharDriveArgs& drive, hipStream_t s) { hipLaunchKernelGGL(k_characters_update<true>, dim3(b.n), dim3(64), 0, s, d_dev, b, dt, drive); }      // a wave per character
