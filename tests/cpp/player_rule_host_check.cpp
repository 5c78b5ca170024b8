// The rule of substrata_amd/csrc/sgp_player_rule.h as the host compiles it: reads rows of inputs (hexadecimal bit patterns, one row per line; the columns are
// those tests/test_players_reference.py writes) and prints the outputs of pr_jump_due, pr_update and pr_camera as bit patterns, for the test to compare with
// tests/player_reference.py.
//   player_rule_host_check <table file>
#include "sgp_player_rule.h"
#include <cinttypes>
#include <cstdio>
#include <cstring>

static float f(uint64_t u) { const uint32_t w = (uint32_t)u; float x; memcpy(&x, &w, 4); return x; }
static double d(uint64_t u) { double x; memcpy(&x, &u, 8); return x; }
static uint32_t b(float x) { uint32_t u; memcpy(&u, &x, 4); return u; }

int main(int argc, char** argv)
{
	if (argc < 2) { fprintf(stderr, "usage: player_rule_host_check <table file>\n"); return 2; }
	FILE* in = fopen(argv[1], "r");
	if (!in) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
	enum { COLS = 29 };
	uint64_t c[COLS];
	for (;;) {
		int got = 0;
		for (; got < COLS; ++got) if (fscanf(in, "%" SCNx64, &c[got]) != 1) break;
		if (got == 0) break;
		if (got != COLS) { fprintf(stderr, "short row\n"); return 2; }
		pr_rule_in r;
		r.vel = PR3(f(c[0]), f(c[1]), f(c[2])); r.move = PR3(f(c[3]), f(c[4]), f(c[5])); r.move_up = f(c[6]); r.flags = (uint32_t)c[7]; r.supported = (uint32_t)c[8];
		r.ground_vel = PR3(f(c[9]), f(c[10]), f(c[11])); r.ground_normal = PR3(f(c[12]), f(c[13]), f(c[14])); r.feet_z = f(c[15]);
		r.water_enabled = (uint32_t)c[16]; r.water_z = f(c[17]); r.dt = f(c[18]); r.jump_speed = f(c[19]); r.max_air_speed = f(c[20]); r.eye_height = f(c[21]);
		r.campos_z_delta = f(c[22]);
		const bool due = pr_jump_due(d(c[23]), d(c[24]));
		r.jump_due = due ? 1u : 0u;
		const pr_rule_out o = pr_update(r);
		// the camera function from what an update would have left: position (c25, c26, feet_z), the rule's velocity, supported-after c27, the same ground velocity, dz c28
		const pr_camera_out k = pr_camera(PR3(f(c[25]), f(c[26]), r.feet_z), o.vel, (uint32_t)c[27], r.ground_vel, f(c[28]), r.eye_height, o.campos_z_delta);
		printf("%x %x %x %x %x %x %x %u %u %u %u %x %x %x %x %x %x %x %x\n", b(o.vel.x), b(o.vel.y), b(o.vel.z), b(o.move.x), b(o.move.y), b(o.move.z), b(o.fraction_submerged),
		       o.on_ground, o.jumped, o.allow_sliding, due ? 1u : 0u, b(o.campos_z_delta),
		       b(k.campos_z_delta), b(k.last_xy_plane_vel_rel_ground.x), b(k.last_xy_plane_vel_rel_ground.y), b(k.last_xy_plane_vel_rel_ground.z), b(k.cam_pos.x), b(k.cam_pos.y), b(k.cam_pos.z));
	}
	fclose(in);
	return 0;
}
