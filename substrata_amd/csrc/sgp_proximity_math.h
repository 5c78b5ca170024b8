// sgp_proximity_math.h -- the arithmetic of the proximity and zone watchers (ScriptedObjectProximityChecker::think, gui_client/ScriptedObjectProximityChecker.cpp:40-90;
// Parcel::pointInParcel and WorldState::getParcelPointIsIn as GUIClient.cpp:6874-6968 uses them), written once for the host and the device.  Every expression is
// fp32 in the order docs/CONTRACT.md 4l writes out; the build does not contract a * b + c, so both sides round the same.  Plain inline functions: the host
// compiles them for sgp_proximity_test_point / sgp_proximity_pick_zone, the device for k_prox_observers / k_prox_test (sgp_dev_proximity.h).
#pragma once
#include <math.h>
#include <stdint.h>
#include "../../include/sgp.h"

#if defined(__HIPCC__)
#define SGP_PX __host__ __device__ inline
#else
#define SGP_PX inline
#endif

struct px3 { float x, y, z; };
SGP_PX px3 PX3(float x, float y, float z) { px3 r; r.x = x; r.y = y; r.z = z; return r; }
SGP_PX px3 PX3(const float* p) { return PX3(p[0], p[1], p[2]); }
SGP_PX float px_min(float a, float b) { return a < b ? a : b; }
SGP_PX float px_max(float a, float b) { return a > b ? a : b; }

// getClosestPointInAABB (UNVERIFIED: docs/GAPS.md): per axis min(max(p, mn), mx)
SGP_PX px3 px_closest(px3 mn, px3 mx, px3 p) { return PX3(px_min(px_max(p.x, mn.x), mx.x), px_min(px_max(p.y, mn.y), mx.y), px_min(px_max(p.z, mn.z), mx.z)); }
// campos.getDist2(closest point)
SGP_PX float px_dist2(px3 mn, px3 mx, px3 p)
{
	const px3 c = px_closest(mn, mx, p);
	const float dx = p.x - c.x, dy = p.y - c.y, dz = p.z - c.z;
	return (dx * dx + dy * dy) + dz * dz;
}
// in_proximity (:60): strictly inside the radius
SGP_PX bool px_near(float dist2, float radius) { return dist2 < radius * radius; }
// AABBox::contains / Parcel::pointInParcel for an axis-aligned parcel (UNVERIFIED: docs/GAPS.md): inclusive on all six faces
SGP_PX bool px_contains(px3 mn, px3 mx, px3 p) { return p.x >= mn.x && p.x <= mx.x && p.y >= mn.y && p.y <= mx.y && p.z >= mn.z && p.z <= mx.z; }
// the AABB's centroid
SGP_PX px3 px_centroid(px3 mn, px3 mx) { return PX3((mn.x + mx.x) * 0.5f, (mn.y + mx.y) * 0.5f, (mn.z + mx.z) * 0.5f); }

// The zone an observer at p stands in (GUIClient.cpp:6874-6890: the guess first, then std::map order): `current` stays if it is live and still contains p;
// else the live zone of the lowest key that contains p; else none.  The device finds the same zone with a workgroup (k_prox_observers): keys are unique
// among live zones, so the least key names one zone whatever the order of the search.
SGP_PX uint32_t px_pick_zone(const float* mins, const float* maxs, const uint32_t* keys, const uint32_t* live, uint32_t n, uint32_t current, px3 p)
{
	if (current < n && live[current] && px_contains(PX3(mins + 3 * (size_t)current), PX3(maxs + 3 * (size_t)current), p)) return current;
	uint32_t best = SGP_INVALID_ID, best_key = 0u;
	for (uint32_t z = 0; z < n; ++z) {
		if (!live[z] || !px_contains(PX3(mins + 3 * (size_t)z), PX3(maxs + 3 * (size_t)z), p)) continue;
		if (best == SGP_INVALID_ID || keys[z] < best_key) { best = z; best_key = keys[z]; }
	}
	return best;
}
