// A caller with hover cars and boats twice over: world A drives four crafts through a CraftBatch (shim/CraftBatch.h), world B drives the same four bodies the
// way HoverCarPhysics::update / BoatPhysics::update do -- read the body back, evaluate, AddForce / AddTorque, one craft and one sub-step at a time -- with every
// expression written as docs/CONTRACT.md ("Crafts") writes it.  Prints one JSON line: how far the two worlds are apart, and the particles each side made.
#include "PhysicsWorld.h"
#include "CraftBatch.h"
#include <utils/Exception.h>
#include <cmath>
#include <cstdio>
#include <vector>

struct V { float x, y, z; };
static V operator+(V a, V b) { return V{ a.x + b.x, a.y + b.y, a.z + b.z }; }
static V operator-(V a, V b) { return V{ a.x - b.x, a.y - b.y, a.z - b.z }; }
static V operator*(V a, float s) { return V{ a.x * s, a.y * s, a.z * s }; }
static V operator-(V a) { return V{ -a.x, -a.y, -a.z }; }
static float dotv(V a, V b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
static V crossv(V a, V b) { return V{ a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x }; }
static float lenv(V a) { return std::sqrt(dotv(a, a)); }
static V divv(V a, float s) { return V{ a.x / s, a.y / s, a.z / s }; }
static V norm(V a) { return divv(a, lenv(a)); }
struct Q { float x, y, z, w; };
static Q qmul(Q a, Q b)
{
	return Q{ a.w * b.x + a.x * b.w + a.y * b.z - a.z * b.y, a.w * b.y - a.x * b.z + a.y * b.w + a.z * b.x, a.w * b.z + a.x * b.y - a.y * b.x + a.z * b.w, a.w * b.w - a.x * b.x - a.y * b.y - a.z * b.z };
}
static Q conj(Q q) { return Q{ -q.x, -q.y, -q.z, q.w }; }
struct M { V c0, c1, c2; };
static M toMatrix(Q q)
{
	const float x2 = q.x + q.x, y2 = q.y + q.y, z2 = q.z + q.z;
	const float xx = q.x * x2, yy = q.y * y2, zz = q.z * z2, xy = q.x * y2, xz = q.x * z2, yz = q.y * z2, wx = q.w * x2, wy = q.w * y2, wz = q.w * z2;
	return M{ V{ 1.0f - (yy + zz), xy + wz, xz - wy }, V{ xy - wz, 1.0f - (xx + zz), yz + wx }, V{ xz + wy, yz - wx, 1.0f - (xx + yy) } };
}
static V mulv(const M& m, V v) { return V{ m.c0.x * v.x + m.c1.x * v.y + m.c2.x * v.z, m.c0.y * v.x + m.c1.y * v.y + m.c2.y * v.z, m.c0.z * v.x + m.c1.z * v.y + m.c2.z * v.z }; }

static float craftRand(uint32_t seed, uint32_t update_index, uint32_t draw)
{
	uint32_t h = seed ^ (update_index * 0x9E3779B9u) ^ (draw * 0x85EBCA6Bu);
	h ^= h >> 16; h *= 0x7FEB352Du; h ^= h >> 15; h *= 0x846CA68Bu; h ^= h >> 16;
	return (float)(h >> 8) * 5.9604644775390625e-8f;
}
static float liftCoeff(float cos_theta) { const float theta = std::acos(cos_theta); const float alpha = 1.5707964f - theta; return alpha < 25.0f * 0.017453292f ? 2.0f : 0.0f; }
static V axisTimesAngle(Q d)
{
	if (d.w < 0.0f) d = Q{ -d.x, -d.y, -d.z, -d.w };
	if (d.w >= 1.0f) return V{ 0, 0, 0 };
	const float angle = 2.0f * std::acos(d.w);
	const float len_sq = d.x * d.x + d.y * d.y + d.z * d.z;
	if (len_sq <= 1.17549435e-38f) return V{ 0, 0, 0 };
	const float len = std::sqrt(len_sq);
	return V{ d.x / len, d.y / len, d.z / len } * angle;
}
static V correctionTorque(Q r_quat, Q q, float yaw, V ang_vel, float mass, float gain)
{
	const Q yq{ 0.0f, 0.0f, std::sin(0.5f * yaw), std::cos(0.5f * yaw) };
	const V desired_ang_vel = axisTimesAngle(qmul(qmul(yq, r_quat), conj(q))) * 3.0f;
	return ((desired_ang_vel - ang_vel) * mass) * gain;
}
static JPH::Vec3 J(V v) { return JPH::Vec3(v.x, v.y, v.z); }

struct HostCraft {
	bool boat; Reference<PhysicsObject> ob; float mass; uint32_t seed; bool driver, boost; float forward, right, up;
	float unflip = -1.f, righting = -1.f; uint32_t update_index = 0; size_t particles = 0;
	V trace_os{ 0, 0, -0.408f }; BoatScriptSettings boat_settings; float shape_volume = 1.f;
};

static void hostUpdate(PhysicsWorld& world, HostCraft& c, float dt)
{
	JPH::BodyInterface& bi = world.physics_system->GetBodyInterface();
	const JPH::BodyID id = c.ob->jolt_body_id;
	JPH::RVec3 p; JPH::Quat jq; JPH::Vec3 lv, av;
	bi.GetPositionAndRotation(id, p, jq);
	bi.GetLinearAndAngularVelocity(id, lv, av);
	const V pos{ p.GetX(), p.GetY(), p.GetZ() }, lin_vel{ lv.GetX(), lv.GetY(), lv.GetZ() }, ang_vel{ av.GetX(), av.GetY(), av.GetZ() };
	const Q q{ jq.GetX(), jq.GetY(), jq.GetZ(), jq.GetW() };
	const Q r_quat = qmul(Q{ 0, 0, 0, 1 }, Q{ 0, 0, 0, 1 });
	const M Ri = toMatrix(conj(r_quat)), R = toMatrix(q);
	const V right_os = Ri.c0, fwd_os = Ri.c1, up_os = crossv(right_os, fwd_os);
	const V right_ws = mulv(R, right_os), fwd_ws = mulv(R, fwd_os), up_ws = mulv(R, up_os);
	const bool water = world.getWaterBuoyancyEnabled(); const float water_z = world.getWaterZ();
	const float mass = c.mass, forward = c.forward, right = c.right;
	const uint32_t u = c.update_index++;
	if (!c.boat) {
		if (!c.driver) return;
		if (right != 0.f || forward != 0.f) bi.ActivateBody(id);
		if (up_ws.z > 0.f) bi.AddForce(id, J((((up_ws * (1.0f + c.up * 0.6f)) * (1.0f / std::fmax(0.7f, up_ws.z))) * mass) * 9.81f));
		if (c.unflip > 0.f) {
			if ((double)up_ws.z > 0.2) c.unflip = -1.f;
			else { bi.AddForce(id, J(((V{ 0, 0, 1 } * 1.0f) * mass) * 9.81f)); c.unflip -= dt; }
		} else if ((double)up_ws.z < -0.9) c.unflip = 1.f;
		const V fcf = ((fwd_ws * mass) * 10.0f) * forward;
		bi.AddForce(id, J(fcf));
		bi.AddForce(id, J(up_ws * -fcf.z));
		bi.AddTorque(id, J(((right_ws * mass) * -0.5f) * forward));
		bi.AddTorque(id, J(((up_ws * mass) * -3.0f) * right));
		bi.AddTorque(id, J(((fwd_ws * mass) * 2.0f) * right));
		bi.AddTorque(id, J(correctionTorque(r_quat, q, std::atan2(right_ws.y, right_ws.x), ang_vel, mass, 1.5f)));
		const float v_mag = lenv(lin_vel);
		if (v_mag > 1.0e-3f) {
			const V nv = divv(lin_vel, v_mag);
			const float rho = 1.293f;
			const float f_d = 0.5f * rho * v_mag * v_mag * 0.2f * (std::fabs(dotv(nv, fwd_ws)) * 2.0f);
			const float s_d = 0.5f * rho * v_mag * v_mag * 0.5f * (std::fabs(dotv(nv, right_ws)) * 4.0f);
			const float t_d = 0.5f * rho * v_mag * v_mag * 0.75f * (std::fabs(dotv(nv, up_ws)) * 8.0f);
			bi.AddForce(id, J(nv * -(f_d + s_d + t_d)));
			const V up_dir = up_ws - nv * dotv(up_ws, nv);
			if (lenv(up_dir) > 1.0e-3f) {
				const float top_dot = dotv(nv, up_ws), top_C_L = liftCoeff(top_dot), top_area = top_dot * 8.0f;
				if (top_C_L > 0 && top_area > 0) bi.AddForce(id, J((-norm(up_dir)) * (0.5f * rho * v_mag * v_mag * top_area * top_C_L)));
				const float bottom_area = -top_area, bottom_C_L = liftCoeff(-top_dot);
				if (bottom_C_L > 0 && bottom_area > 0) bi.AddForce(id, J(norm(up_dir) * (0.5f * rho * v_mag * v_mag * bottom_area * bottom_C_L)));
			}
			const V right_dir = right_ws - nv * dotv(right_ws, nv);
			if (lenv(right_dir) > 1.0e-3f) {
				const float right_dot = dotv(nv, right_ws), right_C_L = liftCoeff(right_dot), right_area = dotv(nv, right_ws) * 4.0f;
				if (right_area > 0) bi.AddForce(id, J((-norm(right_dir)) * (0.5f * rho * v_mag * v_mag * right_area * right_C_L)));
				const float left_area = -right_area, left_C_L = liftCoeff(-right_dot);
				if (left_area > 0) bi.AddForce(id, J(norm(right_dir) * (0.5f * rho * v_mag * v_mag * left_area * left_C_L)));
			}
		}
		const V origin = mulv(R, c.trace_os) + pos;
		const V side_vec = right_ws * (-0.5f + craftRand(c.seed, u, 0)) + fwd_ws * (-0.5f + craftRand(c.seed, u, 1));
		const V dir = norm(-up_ws + side_vec * 0.8f);
		RayTraceResult res;
		world.traceRay(Vec4f(origin.x, origin.y, origin.z, 1), Vec4f(dir.x, dir.y, dir.z, 0), 12.f, JPH::BodyID(), res);
		const float whd = (water_z - origin.z) / dir.z;
		if (water && whd >= 0 && whd < 12.f && (!res.hit_object || res.hit_t > whd)) c.particles += 4;
		else if (res.hit_object) c.particles += 1;
		return;
	}
	const BoatScriptSettings& s = c.boat_settings;
	const float forwards_vel = dotv(lin_vel, fwd_ws);
	if (c.driver) {
		if (right != 0.f || forward != 0.f) bi.ActivateBody(id);
		const V prop = mulv(R, V{ s.propellor_point_os[0], s.propellor_point_os[1], s.propellor_point_os[2] }) + pos;
		if (forward != 0.f && water && prop.z <= water_z) {
			const V d = norm((fwd_ws - up_ws * 0.2f) - (right_ws * right) * s.thrust_vector_lateral_amount);
			bi.AddForce(id, J((d * s.thrust_force) * forward), JPH::RVec3(prop.x, prop.y, prop.z));
			c.particles += 6;
		}
		if (right != 0.f) bi.AddForce(id, J(((right_ws * -right) * forwards_vel) * s.rudder_deflection_force_factor), JPH::RVec3(prop.x, prop.y, prop.z));
	}
	const float sub = c.ob->last_submerged_volume;
	const float frac = sub / c.shape_volume;
	const float ss = std::fmin(std::fmax((sub - 0.0f) / (1.0f - 0.0f), 0.0f), 1.0f);
	const float top_frac = ss * ss * (3.0f - 2.0f * ss);
	const float v_mag = lenv(lin_vel);
	if (sub > 0 && v_mag > 1.0e-3f) {
		const V nv = divv(lin_vel, v_mag);
		const float rho = 1020.0f;
		const float f_d = 0.5f * rho * v_mag * v_mag * 0.1f * (std::fabs(dotv(nv, fwd_ws)) * s.front_cross_sectional_area) * frac;
		const float s_d = 0.5f * rho * v_mag * v_mag * 0.5f * (std::fabs(dotv(nv, right_ws)) * s.side_cross_sectional_area) * frac;
		const float t_d = 0.5f * rho * v_mag * v_mag * 0.75f * (std::fabs(dotv(nv, up_ws)) * s.top_cross_sectional_area) * top_frac;
		bi.AddForce(id, J(nv * -(f_d + s_d + t_d)));
	}
	for (size_t i = 0; i < s.splash_points.size(); ++i) {
		if (!(v_mag > 5.f)) continue;
		const float sign = std::fmin(std::fmax(s.splash_points[i].right_sign, -1.f), 1.f);
		const V pt = mulv(R, V{ s.splash_points[i].point_os[0], s.splash_points[i].point_os[1], s.splash_points[i].point_os[2] }) + pos;
		if (water && pt.z < water_z && dotv(norm(lin_vel), right_ws * sign) > -0.5f) c.particles += 2;
	}
	if (c.righting > 0.f) {
		const V nrr = norm(crossv(fwd_ws, V{ 0, 0, 1 }));
		bi.AddTorque(id, J(correctionTorque(r_quat, q, std::atan2(nrr.y, nrr.x), ang_vel, mass, 3.5f)));
		c.righting -= dt;
	}
}

struct Scene { Reference<PhysicsWorld> world; std::vector<Reference<PhysicsObject>> obs; };
static Scene makeScene()
{
	Scene sc;
	sc.world = new PhysicsWorld(nullptr, nullptr);
	sc.world->setWaterBuoyancyEnabled(true); sc.world->setWaterZ(0.5f);
	Reference<PhysicsObject> ground = new PhysicsObject(true);
	ground->is_cube = true; ground->scale = Vec3f(60.f, 20.f, 1.f); ground->pos = Vec4f(0, -20.f, 0.5f, 1);
	sc.world->addObject(ground);
	const float at[4][3] = { { 0, -20.f, 3.5f }, { 0, 20.f, 4.f }, { 0, 40.f, 0.6f }, { 10.f, 40.f, 0.6f } };
	for (int i = 0; i < 4; ++i) {
		Reference<PhysicsObject> ob = new PhysicsObject(true);
		const bool boat = i >= 2;
		ob->is_cube = true; ob->scale = boat ? Vec3f(2.f, 6.f, 1.f) : Vec3f(1.8f, 4.f, 0.8f); ob->mass = boat ? 2000.f : 1000.f;
		ob->motion_type = PhysicsObject::MotionType_dynamic; ob->use_zero_linear_drag = boat;
		ob->pos = Vec4f(at[i][0], at[i][1], at[i][2], 1);
		if (i == 3) { ob->rot = Quatf(); ob->rot.v = Vec4f(0, std::sin(1.45f), 0, std::cos(1.45f)); }      // capsized: 2.9 rad about y
		sc.world->addObject(ob); sc.world->activateObject(ob); sc.obs.push_back(ob);
	}
	return sc;
}

int main()
{
	try {
		PhysicsWorld::init();
		Scene a = makeScene(), b = makeScene();
		BoatScriptSettings bs;
		bs.propellor_point_os = Vec4f(0, -2.8f, -0.3f, 1); bs.propellor_sideways_offset = 0.6f; bs.thrust_force = 30000.f; bs.rudder_deflection_force_factor = 400.f;
		bs.front_cross_sectional_area = 1.5f; bs.side_cross_sectional_area = 3.f; bs.top_cross_sectional_area = 6.f;
		bs.splash_points.push_back(BoatScriptSettings::SplashPoint{ Vec4f(-0.9f, 2.5f, -0.3f, 1), -1.f });
		bs.splash_points.push_back(BoatScriptSettings::SplashPoint{ Vec4f(0.9f, 2.5f, -0.3f, 1), 1.f });

		CraftBatch batch(a.world->physics_system, 4);
		ParticleBatch particles(a.world->physics_system, 4 * SGP_CRAFT_MAX_EMIT);
		batch.attachParticles(&particles);
		std::vector<HostCraft> host(4);
		PlayerPhysicsInput keys[4];
		keys[0].W_down = true; keys[0].D_down = true; keys[0].right_trigger = 0.2f;
		keys[1].W_down = true;
		keys[2].W_down = true; keys[2].SHIFT_down = true; keys[2].axis_left_x = 0.5f;
		for (uint32_t i = 0; i < 4; ++i) {
			HostCraft& h = host[i];
			h.boat = i >= 2; h.ob = b.obs[i]; h.mass = h.boat ? 2000.f : 1000.f; h.seed = 100u + i; h.driver = i < 3; h.boost = keys[i].SHIFT_down;
			if (h.boat) {
				BoatPhysicsSettings st; st.script_settings = bs; st.boat_mass = h.mass;
				if (batch.addBoat(a.obs[i]->jolt_body_id, st, h.seed) != i) return 4;
				h.boat_settings = bs;
				const JPH::Body* locked = b.world->physics_system->GetBodyLockInterface().TryGetBody(h.ob->jolt_body_id);
				h.shape_volume = locked ? locked->GetShape()->GetVolume() : 1.f;
				if (h.shape_volume == 0.f) h.shape_volume = 1.f;
				h.forward = keys[i].W_down ? (keys[i].SHIFT_down ? 2.f : 1.f) : 0.f; h.right = keys[i].axis_left_x; h.up = 0.f;
			} else {
				HoverCarPhysicsSettings st; st.hovercar_mass = h.mass; st.trace_origin_os = Vec4f(h.trace_os.x, h.trace_os.y, h.trace_os.z, 1);
				if (batch.addHoverCar(a.obs[i]->jolt_body_id, st, h.seed) != i) return 4;
				h.forward = keys[i].W_down ? 1.f : 0.f; h.right = keys[i].D_down ? 1.f : keys[i].axis_left_x; h.up = keys[i].right_trigger - keys[i].left_trigger;
			}
			if (h.driver) batch.userEnteredVehicle(i, 0);
			batch.setInput(i, keys[i]);
		}
		batch.startRightingVehicle(3); host[3].righting = 2.f;

		const int updates = 20;
		const float dt = 1.f / 60.f;
		size_t batch_particles = 0;
		float max_pos = 0.f, max_rot = 0.f, max_vel = 0.f, moved = 0.f;
		for (int s = 0; s < updates; ++s) {
			batch.update(dt);
			a.world->think(dt);
			for (HostCraft& h : host) hostUpdate(*b.world, h, dt);
			b.world->think(dt);
			for (const sgp_craft_state& st : batch.readBack()) batch_particles += st.n_emitted;
			JPH::BodyInterface& ba = a.world->physics_system->GetBodyInterface(); JPH::BodyInterface& bb = b.world->physics_system->GetBodyInterface();
			for (int i = 0; i < 4; ++i) {
				JPH::RVec3 pa, pb; JPH::Quat qa, qb; JPH::Vec3 la, lb, wa, wb;
				ba.GetPositionAndRotation(a.obs[i]->jolt_body_id, pa, qa); bb.GetPositionAndRotation(b.obs[i]->jolt_body_id, pb, qb);
				ba.GetLinearAndAngularVelocity(a.obs[i]->jolt_body_id, la, wa); bb.GetLinearAndAngularVelocity(b.obs[i]->jolt_body_id, lb, wb);
				max_pos = std::fmax(max_pos, std::fmax(std::fabs(pa.GetX() - pb.GetX()), std::fmax(std::fabs(pa.GetY() - pb.GetY()), std::fabs(pa.GetZ() - pb.GetZ()))));
				max_rot = std::fmax(max_rot, std::fmax(std::fmax(std::fabs(qa.GetX() - qb.GetX()), std::fabs(qa.GetY() - qb.GetY())), std::fmax(std::fabs(qa.GetZ() - qb.GetZ()), std::fabs(qa.GetW() - qb.GetW()))));
				max_vel = std::fmax(max_vel, std::fmax(std::fabs(la.GetX() - lb.GetX()), std::fmax(std::fabs(la.GetY() - lb.GetY()), std::fabs(la.GetZ() - lb.GetZ()))));
				max_vel = std::fmax(max_vel, std::fmax(std::fabs(wa.GetX() - wb.GetX()), std::fmax(std::fabs(wa.GetY() - wb.GetY()), std::fabs(wa.GetZ() - wb.GetZ()))));
				if (s == updates - 1) moved = std::fmax(moved, std::fabs(pa.GetY() - a.obs[i]->pos[1]) + std::fabs(pa.GetZ() - a.obs[i]->pos[2]));
			}
		}
		size_t host_particles = 0;
		for (const HostCraft& h : host) host_particles += h.particles;
		particles.readBack();
		printf("{\"crafts\": 4, \"updates\": %d, \"max_pos_diff\": %.9g, \"max_rot_diff\": %.9g, \"max_vel_diff\": %.9g, \"moved\": %.9g, \"particles_batch\": %zu, \"particles_host\": %zu, \"particles_live\": %zu}\n",
		       updates, max_pos, max_rot, max_vel, moved, batch_particles, host_particles, particles.live().size());
		return 0;
	} catch (glare::Exception& e) { fprintf(stderr, "glare::Exception: %s\n", e.what().c_str()); return 2; }
	catch (std::exception& e) { fprintf(stderr, "exception: %s\n", e.what()); return 3; }
}
