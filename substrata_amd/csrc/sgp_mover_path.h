// sgp_mover_path.h -- the path arithmetic of ObjectPathController (gui_client/ObjectPathController.cpp), written once for the host and the device.
// mp_prepare restates the constructor's segment loop (:60-124), mp_advance the state change of walkAlongPathForTime (:233-393), mp_eval the position and
// direction of a state (the bodies of its branches, and of evalAlongPathDistBackwards'), mp_eval_backwards the walk of evalAlongPathDistBackwards (:147-229).
// Every expression is fp32 in the order docs/CONTRACT.md 4j writes out; the build does not contract a * b + c, so mp_advance -- which has only + - * / and
// comparisons in it -- rounds the same on both sides.  Plain inline functions; the host compiles them for sgp_path_prepare / sgp_path_advance and for the
// initial state of a walker, the device for k_movers_update / k_movers_follow (sgp_dev_movers.h).
#pragma once
#include <math.h>
#include <stdint.h>
#include "../../include/sgp.h"

#if defined(__HIPCC__)
#define SGP_MP __host__ __device__ inline
#else
#define SGP_MP inline
#endif

struct mp3 { float x, y, z; };
SGP_MP mp3 MP3(float x, float y, float z) { mp3 r; r.x = x; r.y = y; r.z = z; return r; }
SGP_MP mp3 MP3(const float* p) { return MP3(p[0], p[1], p[2]); }
SGP_MP mp3 mp_add(mp3 a, mp3 b) { return MP3(a.x + b.x, a.y + b.y, a.z + b.z); }
SGP_MP mp3 mp_sub(mp3 a, mp3 b) { return MP3(a.x - b.x, a.y - b.y, a.z - b.z); }
SGP_MP mp3 mp_scale(mp3 a, float s) { return MP3(a.x * s, a.y * s, a.z * s); }
SGP_MP float mp_dot(mp3 a, mp3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
SGP_MP float mp_len(mp3 a) { return sqrtf(mp_dot(a, a)); }
SGP_MP mp3 mp_normalise(mp3 a) { const float l = mp_len(a); return MP3(a.x / l, a.y / l, a.z / l); }
SGP_MP float mp_dist(mp3 a, mp3 b) { return mp_len(mp_sub(a, b)); }
SGP_MP float mp_min(float a, float b) { return a < b ? a : b; }
SGP_MP float mp_max(float a, float b) { return a > b ? a : b; }
SGP_MP float mp_clamp(float x, float lo, float hi) { return mp_max(lo, mp_min(x, hi)); }                        // myClamp
SGP_MP float mp_lerp(float a, float b, float t) { return a * (1.0f - t) + b * t; }                              // Maths::lerp / uncheckedLerp (term order: CONTRACT 4i)
SGP_MP mp3 mp_lerp3(mp3 a, mp3 b, float t) { return MP3(mp_lerp(a.x, b.x, t), mp_lerp(a.y, b.y, t), mp_lerp(a.z, b.z, t)); }
SGP_MP float mp_smoothstep01(float x) { const float s = mp_clamp((x - 0.0f) / (1.0f - 0.0f), 0.0f, 1.0f); return (s * s) * (3.0f - 2.0f * s); }      // Maths::smoothStep(0, 1, x)
SGP_MP mp3 mp_remove_component(mp3 v, mp3 dir) { return mp_sub(v, mp_scale(dir, mp_dot(v, dir))); }             // removeComponentInDir (UNVERIFIED)
SGP_MP uint32_t mp_wrap(int32_t i, uint32_t n) { const int32_t m = i % (int32_t)n; return (uint32_t)(m < 0 ? m + (int32_t)n : m); }      // Maths::intMod: the non-negative remainder
SGP_MP bool mp_finite(float x) { return x - x == 0.0f; }
SGP_MP mp3 mp_wp(const sgp_path_segment* s, uint32_t n, int32_t i) { return MP3(s[mp_wrap(i, n)].pos); }       // waypointPos

// closestPointOnLineToRay (:20-31)
SGP_MP mp3 mp_closest_point_on_line_to_ray(mp3 a, mp3 b, mp3 c, mp3 d)
{
	const float bd = mp_dot(b, d);
	const float t = (mp_dot(mp_sub(c, a), b) + mp_dot(mp_sub(a, c), d) * bd) / (1.0f - bd * bd);
	return mp_add(a, mp_scale(b, t));
}

// The constructor's segment loop.  0: prepared (out[0..n), *total_time_out); otherwise what is wrong (1 count, 2 a value, 3 a type, 4 a segment).
SGP_MP int mp_prepare(const sgp_path_waypoint* in, uint32_t n, sgp_path_segment* out, double* total_time_out)
{
	if (n < 2u || n > (uint32_t)SGP_MOVER_MAX_WAYPOINTS) return 1;
	for (uint32_t i = 0; i < n; ++i) {
		if (!mp_finite(in[i].pos[0]) || !mp_finite(in[i].pos[1]) || !mp_finite(in[i].pos[2])) return 4;
		if (!mp_finite(in[i].speed) || !(in[i].speed > 0.0f) || !mp_finite(in[i].pause_time) || !(in[i].pause_time >= 0.0f)) return 2;
		if (in[i].type != SGP_WAYPOINT_CURVE_IN && in[i].type != SGP_WAYPOINT_CURVE_OUT && in[i].type != SGP_WAYPOINT_STATION) return 3;
		sgp_path_segment s;
		s.pos[0] = in[i].pos[0]; s.pos[1] = in[i].pos[1]; s.pos[2] = in[i].pos[2]; s.type = in[i].type; s.pause_time = in[i].pause_time; s.speed = in[i].speed;
		s.segment_len = 0.0f; s.just_curve_len = 0.0f; s.entry_segment_len = 0.0f; s.curve_angle = 0.0f; s.curve_r = 0.0f;
		s.exit_segment_unit_dir[0] = 0.0f; s.exit_segment_unit_dir[1] = 0.0f; s.exit_segment_unit_dir[2] = 0.0f;
		out[i] = s;
	}
	for (uint32_t i = 0; i < n; ++i) if (mp_dist(mp_wp(out, n, (int32_t)i), mp_wp(out, n, (int32_t)i + 1)) < 1.0e-5f) return 4;      // (before any direction is formed from it)
	double total_time = 0.0;
	for (uint32_t i = 0; i < n; ++i) {
		sgp_path_segment& w = out[i];
		const mp3 entry_pos = mp_wp(out, n, (int32_t)i), exit_pos = mp_wp(out, n, (int32_t)i + 1);
		const mp3 entry_dir = mp_normalise(mp_sub(entry_pos, mp_wp(out, n, (int32_t)i - 1)));
		const mp3 exit_dir = mp_normalise(mp_sub(mp_wp(out, n, (int32_t)i + 2), exit_pos));
		if (w.type == SGP_WAYPOINT_CURVE_IN) {
			const float angle = acosf(mp_clamp(mp_dot(entry_dir, exit_dir), -1.0f, 1.0f));
			mp3 ex;
			if (angle < 1.0e-6f) {      // entry and exit direction are equal: an entry segment and no arc
				w.segment_len = mp_dist(entry_pos, exit_pos); w.just_curve_len = 0.0f; w.entry_segment_len = mp_dist(entry_pos, exit_pos);
				w.curve_angle = 0.0f; w.curve_r = 1000.0f;
				ex = mp_normalise(mp_sub(exit_pos, entry_pos));
			} else {
				const mp3 p = mp_closest_point_on_line_to_ray(entry_pos, entry_dir, exit_pos, exit_dir);
				const float entry_to_p = mp_dist(p, entry_pos), exit_to_p = mp_dist(p, exit_pos);
				const float d = mp_min(entry_to_p, exit_to_p);
				const float curve_r = d / tanf(angle / 2.0f);
				const float curve_len = angle * curve_r;
				const float entry_segment_len = mp_max(entry_to_p - d, 0.0f), exit_segment_len = mp_max(exit_to_p - d, 0.0f);
				w.segment_len = (curve_len + entry_segment_len) + exit_segment_len; w.just_curve_len = curve_len; w.entry_segment_len = entry_segment_len;
				w.curve_angle = angle; w.curve_r = curve_r;
				ex = mp_normalise(mp_sub(exit_pos, p));
			}
			w.exit_segment_unit_dir[0] = ex.x; w.exit_segment_unit_dir[1] = ex.y; w.exit_segment_unit_dir[2] = ex.z;
		}
		else w.segment_len = mp_dist(entry_pos, exit_pos);
		if (!mp_finite(w.segment_len) || w.segment_len < 1.0e-5f) return 4;
		if (!mp_finite(w.just_curve_len) || !mp_finite(w.entry_segment_len) || !mp_finite(w.curve_r) || !mp_finite(w.exit_segment_unit_dir[0]) || !mp_finite(w.exit_segment_unit_dir[1])
		    || !mp_finite(w.exit_segment_unit_dir[2])) return 4;
		total_time += (double)(w.segment_len / w.speed);
		if (w.type == SGP_WAYPOINT_STATION) total_time += (double)w.pause_time;
	}
	*total_time_out = total_time;
	return 0;
}

// walkAlongPathForTime's state change for dt; at most max_ends segment ends are passed (the reference's loop has no bound).
SGP_MP void mp_advance(const sgp_path_segment* segs, uint32_t n, sgp_path_progress* io, float dt, uint32_t max_ends, uint32_t* status_io)
{
	uint32_t idx = io->waypoint_index; float dist = io->dist_along_segment, time = io->time_along_segment;
	float dtime_remaining = dt;
	uint32_t ends = 0u;
	while (dtime_remaining > 0.0f) {
		const sgp_path_segment& w = segs[idx];
		const float vel = w.speed;
		float travelled = time;      // time spent travelling on this segment so far
		if (w.type == SGP_WAYPOINT_STATION) {
			if (time < w.pause_time) {      // still stopped at the station
				const float stop_time_remaining = w.pause_time - time;
				if (dtime_remaining < stop_time_remaining) { time += dtime_remaining; break; }
				dtime_remaining -= stop_time_remaining;
				time += stop_time_remaining;
			}
			travelled = time - w.pause_time;
		}
		const float segment_time_remaining = w.segment_len / vel - travelled;
		if (dtime_remaining < segment_time_remaining) {      // the end of the segment is not reached
			dist += dtime_remaining * vel;
			time += dtime_remaining;
			break;
		}
		dtime_remaining -= segment_time_remaining;
		dist = 0.0f; time = 0.0f;
		idx = mp_wrap((int32_t)idx + 1, n);
		if (++ends >= max_ends) { *status_io |= SGP_MOVER_ST_OVERRUN; break; }
	}
	io->waypoint_index = idx; io->dist_along_segment = dist; io->time_along_segment = time;
}

// Position and direction at `dist` along segment `idx`: the branch bodies of walkAlongPathForTime and evalAlongPathDistBackwards, the branch chosen by distance
// as the latter does.  (A walker still paused at a station has dist = 0, where the travelling expressions give entry_pos and begin_dir: no branch of its own.)
SGP_MP void mp_eval(const sgp_path_segment* segs, uint32_t n, uint32_t idx, float dist, mp3* pos_out, mp3* dir_out)
{
	const sgp_path_segment& w = segs[idx];
	const mp3 entry_pos = mp_wp(segs, n, (int32_t)idx), exit_pos = mp_wp(segs, n, (int32_t)idx + 1);
	const mp3 entry_dir = mp_normalise(mp_sub(entry_pos, mp_wp(segs, n, (int32_t)idx - 1)));
	if (w.type == SGP_WAYPOINT_CURVE_IN) {
		const mp3 ex = MP3(w.exit_segment_unit_dir);
		if (dist < w.entry_segment_len) {
			*pos_out = mp_add(entry_pos, mp_scale(entry_dir, dist));
			*dir_out = entry_dir;
		}
		else if (dist < w.entry_segment_len + w.just_curve_len) {
			const float curve_frac = (dist - w.entry_segment_len) / w.just_curve_len;
			const mp3 orthog = mp_normalise(mp_remove_component(ex, entry_dir));
			const float angle = curve_frac * w.curve_angle;
			const float sn = sinf(angle), cs = cosf(angle);
			*pos_out = mp_add(mp_add(entry_pos, mp_scale(entry_dir, w.entry_segment_len)),
			                  mp_add(mp_scale(mp_scale(entry_dir, w.curve_r), sn), mp_scale(mp_scale(orthog, w.curve_r), 1.0f - cs)));
			*dir_out = mp_add(mp_scale(entry_dir, cs), mp_scale(orthog, sn));
		}
		else {
			const float dist_uncovered = w.segment_len - dist;
			*pos_out = mp_sub(exit_pos, mp_scale(ex, dist_uncovered));
			*dir_out = ex;
		}
		return;
	}
	const float frac = dist / w.segment_len;
	*pos_out = mp_lerp3(entry_pos, exit_pos, frac);
	const mp3 end_dir = mp_normalise(mp_sub(exit_pos, entry_pos));
	if (w.type == SGP_WAYPOINT_CURVE_OUT) *dir_out = end_dir;
	else *dir_out = mp_lerp3(entry_dir, end_dir, mp_smoothstep01(frac + 0.5f) * 2.0f - 1.0f);
}

// evalAlongPathDistBackwards: from `dist` along segment `idx`, back by delta (>= 0).  io: where it ends (the segment and the distance along it).
SGP_MP void mp_eval_backwards(const sgp_path_segment* segs, uint32_t n, uint32_t* idx_io, float* dist_io, float delta, uint32_t max_starts, uint32_t* status_io, mp3* pos_out, mp3* dir_out)
{
	uint32_t idx = *idx_io; float dist = *dist_io;
	uint32_t starts = 0u;
	for (;;) {
		if (delta < dist) { dist -= delta; break; }      // the start of the segment is not reached
		delta -= dist;
		idx = mp_wrap((int32_t)idx - 1, n);
		dist = segs[idx].segment_len;                     // at the end of the previous segment
		if (++starts >= max_starts) {                     // the cap: entry_pos and entry_dir of the segment reached
			*status_io |= SGP_MOVER_ST_OVERRUN;
			const mp3 entry_pos = mp_wp(segs, n, (int32_t)idx);
			*pos_out = entry_pos; *dir_out = mp_normalise(mp_sub(entry_pos, mp_wp(segs, n, (int32_t)idx - 1)));
			*idx_io = idx; *dist_io = 0.0f;
			return;
		}
	}
	mp_eval(segs, n, idx, dist, pos_out, dir_out);
	*idx_io = idx; *dist_io = dist;
}
