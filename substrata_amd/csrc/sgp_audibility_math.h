// sgp_audibility_math.h -- the arithmetic of the audio sources' batch (the range walk of GUIClient.cpp:4512-4543, the occlusion and muting walk of
// GUIClient.cpp:6973-7034 and the mute ramp of audio/AudioEngine.cpp:79-121), written once for the host and the device.  Every expression is fp32 or fp64
// exactly as docs/CONTRACT.md 4m writes it out; the build does not contract a * b + c, so both sides round the same.  Plain inline functions: the host
// compiles them for sgp_audibility_pair_ray / sgp_audibility_ramp_step, the device for k_aud_range / k_aud_rays / k_aud_fold (sgp_dev_audibility.h).
#pragma once
#include <math.h>
#include <stdint.h>
#include "../../include/sgp.h"

#if defined(__HIPCC__)
#define SGP_AX __host__ __device__ inline
#else
#define SGP_AX inline
#endif

// step 1: source minus listener, the squared distance (getDist2: UNVERIFIED summation order, docs/CONTRACT.md 4m) and maxAudioDistForSourceVolFactor (:1507-1510)
struct AxGeom { float dx, dy, dz, d2, maxd, max2; };
SGP_AX AxGeom ax_geom(float sx, float sy, float sz, float lx, float ly, float lz, float volume)
{
	AxGeom g;
	g.dx = sx - lx; g.dy = sy - ly; g.dz = sz - lz;
	g.d2 = (g.dx * g.dx + g.dy * g.dy) + g.dz * g.dz;
	g.maxd = 60.0f * volume;
	g.max2 = g.maxd * g.maxd;
	return g;
}
// step 2 (:4519-4542): leaves beyond the range, enters at or inside it
SGP_AX bool ax_range(bool in_range, const AxGeom& g)
{
	if (in_range && g.d2 > g.max2) return false;
	if (!in_range && g.d2 <= g.max2) return true;
	return in_range;
}
// step 3's test (:6984-6985): in range, and strictly nearer than maxd; *dist = sqrtf(d2) where the pair is in range
SGP_AX bool ax_traced(bool in_range_now, const AxGeom& g, float* dist)
{
	if (!in_range_now) { *dist = 0.0f; return false; }
	*dist = sqrtf(g.d2);
	return *dist < g.maxd;
}
// the ray of a traced pair (:6987-6992): from the listener towards the source, a division by dist; myClamp(dist - 1, 0, 60) (UNVERIFIED: min(max(x, lo), hi))
SGP_AX void ax_ray(const AxGeom& g, float dist, float dir[3], float* trace)
{
	if (dist == 0.0f) { dir[0] = 1.0f; dir[1] = 0.0f; dir[2] = 0.0f; }
	else { dir[0] = g.dx / dist; dir[1] = g.dy / dist; dir[2] = g.dz / dist; }
	const float a = dist - 1.0f;
	const float b = a > 0.0f ? a : 0.0f;
	*trace = b < 60.0f ? b : 60.0f;
}

// the five ramp variables of AudioSource (AudioEngine.h:136-140); as the constructor leaves them (AudioEngine.cpp:70-71)
struct AxRamp { double start, end; float factor, fac_start, fac_end; };
SGP_AX AxRamp ax_ramp_fresh() { AxRamp r; r.start = -2.0; r.end = -1.0; r.factor = 1.0f; r.fac_start = 1.0f; r.fac_end = 1.0f; return r; }
// AudioSource::startMuting (:79-90): transition * factor is formed in double
SGP_AX void ax_start_muting(AxRamp& r, double cur_time, double transition)
{
	if (r.fac_end != 0.0f) {
		r.start = cur_time;
		r.end = cur_time + transition * (double)r.factor;
		r.fac_start = r.factor;
		r.fac_end = 0.0f;
	}
}
// AudioSource::startUnmuting (:93-104): 1.f - factor in float, the product in double
SGP_AX void ax_start_unmuting(AxRamp& r, double cur_time, double transition)
{
	if (r.fac_end != 1.0f) {
		r.start = cur_time;
		r.end = cur_time + transition * (double)(1.0f - r.factor);
		r.fac_start = r.factor;
		r.fac_end = 1.0f;
	}
}
// AudioSource::updateCurrentMuteVolumeFactor (:107-121)
SGP_AX void ax_update_factor(AxRamp& r, double cur_time)
{
	if ((cur_time < r.end) && ((r.end - r.start) > 1.0e-4)) {
		const double frac = (cur_time - r.start) / (r.end - r.start);
		r.factor = r.fac_start + (float)frac * (r.fac_end - r.fac_start);
	} else r.factor = r.fac_end;
}
// one pass of :7013-7027 for a pair that is not one-shot; returns factor != old
SGP_AX bool ax_ramp_step(AxRamp& r, bool mute, double cur_time, double transition)
{
	const float old = r.factor;
	if (mute) ax_start_muting(r, cur_time, transition); else ax_start_unmuting(r, cur_time, transition);
	ax_update_factor(r, cur_time);
	return r.factor != old;
}
// the mute decision (:7014-7022)
SGP_AX bool ax_mute(uint32_t listener_mute_outside, uint32_t source_key, uint32_t listener_key) { return listener_mute_outside && source_key != listener_key; }
