// sgp_k_characters.hip -- A7 -- the batched character controller: JPH::CharacterVirtual::Update / ExtendedUpdate for every character of a batch in one launch.
// One of the stage files of the step kernels (stage map: sgp_kernels.h).  Kernels first, their launch wrappers at the end.
#include "sgp_dev_character_update.h"

// The push records reach the bodies: one wave; lane 0 applies them in ascending character order, then in order of occurrence -- what sgp_body_activate +
// sgp_body_add_force_at in that order would leave (k_apply_cmds), whatever order the update's workgroups ran in.  Pushes are rare (a character against a
// dynamic body); finding them is the 64-wide part.
__global__ void __launch_bounds__(64) k_characters_push(DV d, CharBufs b)
{
	const uint32_t lane = threadIdx.x;
	if (*b.push_any == 0u) return;      // (the same word for every lane: nobody pushed in this update)
	for (uint32_t base = 0; base < b.n; base += 64) {
		const uint32_t k = base + lane;
		const uint32_t cnt = k < b.n ? b.n_push[k] : 0u;
		const unsigned long long pushers = __ballot(cnt > 0u);      // (every lane is here: the serial part below is a branch of lane 0's that ends before the next round)
		if (lane == 0) {
			unsigned long long todo = pushers;
			while (todo) {
				const uint32_t c = base + (uint32_t)(__ffsll((long long)todo) - 1);
				todo &= todo - 1ull;
				const uint32_t nc = min(b.n_push[c], (uint32_t)SGP_CHAR_MAX_PUSHES);
				for (uint32_t r = 0; r < nc; ++r) {
					const CharPush p = b.push[(size_t)c * SGP_CHAR_MAX_PUSHES + r];
					const uint32_t i = p.body;
					if (i >= d.cap_bodies) continue;
					uint32_t f = d.flags[i];
					if (!(f & BF_ALIVE)) continue;
					f = activate_body(d, i, f);      // sgp_body_activate
					if (f_motion(f) == SGP_MOTION_DYNAMIC) {
						// sgp_body_add_force_at
						const v3 Fv = V3(p.f[0], p.f[1], p.f[2]);
						const float4 F = d.force[i], T = d.torque[i];
						d.force[i] = F4(v3_add(V3(F), Fv), F.w);
						d.torque[i] = F4(v3_add(V3(T), v3_cross(v3_sub(V3(p.p[0], p.p[1], p.p[2]), V3(d.pose[POSE_F4 * (size_t)i])), Fv)), T.w);
						f = activate_body(d, i, f) | BF_HAS_FORCE;
					}
					d.flags[i] = f;
				}
				b.n_push[c] = 0u;
			}
		}
	}
	if (lane == 0) *b.push_any = 0u;
}

// sgp_characters_get_states with edits pending and no update to carry them: what the host changed reaches the state
__global__ void __launch_bounds__(TPB) k_characters_sync(CharBufs b, const CharDrive* drive, CharDriveState* dst)
{
	const uint32_t k = blockIdx.x * TPB + threadIdx.x;
	if (k >= b.n) return;
	const CharRec* rc = &b.rec[k];
	if (!rc->alive) return;
	CharState s = b.st[k];
	char_apply_host(rc, b.in[k], s);
	b.st[k] = s;
	CharDriveState ds = dst[k];
	char_apply_drive(rc, drive[k], ds);      // (a pending jump, a new character: sgp_characters_get_drive_states answers as the next update would find it)
	dst[k] = ds;
}

// a wave per character
void launch_characters_update(const DV* d_dev, const CharBufs& b, float dt, const CharDriveArgs* drive, hipStream_t s)
{
	if (!b.n) return;
	if (drive) launch_characters_update_driven(d_dev, b, dt, *drive, s);
	else hipLaunchKernelGGL(k_characters_update<false>, dim3(b.n), dim3(64), 0, s, d_dev, b, dt, CharDriveArgs());
}
void launch_characters_push(const DV& d, const CharBufs& b, hipStream_t s) { if (b.n) hipLaunchKernelGGL(k_characters_push, dim3(1), dim3(64), 0, s, d, b); }
void launch_characters_sync(const CharBufs& b, const CharDrive* drive, CharDriveState* dst, hipStream_t s) { if (b.n) hipLaunchKernelGGL(k_characters_sync, dim3(blocks_for(b.n)), dim3(TPB), 0, s, b, drive, dst); }
