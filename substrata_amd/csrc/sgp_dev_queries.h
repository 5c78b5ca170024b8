// sgp_dev_queries.h -- ray against a box; the broad-phase walk, the capsule and sphere-cast candidate tests, the contact record, the query shape and the
// filters that the capsule queries, the sphere casts, the characters, the overlap queries and the shape casts share.
// Device-inline functions only (no kernels), shared between stage files; included through sgp_dev_all.h, whose order is the dependency order.
#pragma once

SGP_DEV bool ray_aabb(v3 o, v3 dir, float4 mn, float4 mx, float tmax)
{
	float t0 = 0.0f, t1 = tmax;
	const float oo[3] = { o.x, o.y, o.z }, dd[3] = { dir.x, dir.y, dir.z };
	const float lo[3] = { mn.x, mn.y, mn.z }, hi[3] = { mx.x, mx.y, mx.z };
#pragma unroll
	for (int a = 0; a < 3; ++a) {
		if (fabsf(dd[a]) < 1.0e-12f) { if (oo[a] < lo[a] - 1.0e-4f || oo[a] > hi[a] + 1.0e-4f) return false; }
		else {
			float ta = (lo[a] - 1.0e-4f - oo[a]) / dd[a], tb = (hi[a] + 1.0e-4f - oo[a]) / dd[a];
			if (ta > tb) { const float tmp = ta; ta = tb; tb = tmp; }
			t0 = fmaxf(t0, ta); t1 = fminf(t1, tb);
			if (t0 > t1) return false;
		}
	}
	return true;
}

// ---- what the capsule queries (sgp_k_queries.hip), the characters (sgp_dev_character.h), sgp_collide_shapes (sgp_k_shapequery.hip) and sgp_cast_shapes
// (sgp_k_shapecast.hip) share: each of the following is stated once, so that what is bit-equal between them is so by construction ----

// a capsule's shape record and its world bounds grown by max_sep
SGP_DEV void capsule_shape(v3 pos, quat rot, float radius, float half_height, float max_sep, sgd_shape& X, v3& lo, v3& hi)
{
	X.pos = pos; X.R = quat_to_m33(rot); X.type = SGP_SHAPE_CAPSULE; X.p0 = radius; X.p1 = half_height; X.p2 = 0.0f; X.hull = nullptr;
	const v3 ax = v3_scale(X.R.c2, half_height);
	const float e = radius + max_sep;
	const v3 ext = V3(fabsf(ax.x) + e, fabsf(ax.y) + e, fabsf(ax.z) + e);
	lo = v3_sub(X.pos, ext); hi = v3_add(X.pos, ext);
}

// the query's shape record and its world bounds grown by max_separation (BOUNDS = false: the caller does not read lo and hi)
template <bool BOUNDS> SGP_DEV void sq_shape(const DV& d, const sgp_shape_query& q, sgd_shape& X, v3& lo, v3& hi)
{
	quat qq; qq.x = q.rot[0]; qq.y = q.rot[1]; qq.z = q.rot[2]; qq.w = q.rot[3];
	if (q.shape_type == SGP_SHAPE_CAPSULE) { capsule_shape(V3(q.pos[0], q.pos[1], q.pos[2]), qq, q.shape[0], q.shape[1], q.max_separation, X, lo, hi); return; }
	X.pos = V3(q.pos[0], q.pos[1], q.pos[2]);
	X.R = quat_to_m33(qq); X.type = (int)q.shape_type; X.hull = nullptr;
	X.p0 = q.shape[0]; X.p1 = q.shape[1]; X.p2 = q.shape[2];
	if (q.shape_type == SGP_SHAPE_SPHERE) { X.p1 = 0.0f; X.p2 = 0.0f; }
	else if (q.shape_type == SGP_SHAPE_BOX) X.hull = &d.hulls[0];
	else X.hull = &d.hulls[(uint32_t)q.shape[0]];      // (the host has checked the id)
	if (BOUNDS) {
		v3 mn, mx;
		compute_aabb(d, (uint32_t)q.shape_type, make_float4(q.shape[0], q.shape[1], q.shape[2], q.shape[3]), X.pos, qq, mn, mx);
		const v3 e = V3(q.max_separation, q.max_separation, q.max_separation);
		lo = v3_sub(mn, e); hi = v3_add(mx, e);
	}
}

// the filters every candidate passes before anything is computed for it: ignore_id, alive and no alias slot, the layer mask, the bounds
SGP_DEV bool sq_passes(const DV& d, const sgp_shape_query& q, v3 lo, v3 hi, uint32_t j, uint32_t* f_out)
{
	if (j == q.ignore_id) return false;
	const uint32_t f = d.flags[j];
	if (!(f & BF_ALIVE) || (f & BF_ALIAS)) return false;
	const uint32_t mask = q.layer_mask ? q.layer_mask : 0xFu;
	if (!((mask >> f_layer(f)) & 1u)) return false;
	const float4 mn = d.aabb_min[j], mx = d.aabb_max[j];
	if (mx.x < lo.x || mn.x > hi.x || mx.y < lo.y || mn.y > hi.y || mx.z < lo.z || mn.z > hi.z) return false;
	*f_out = f;
	return true;
}

// fn(body) for the candidates of the bounds [lo, hi] -- the large bodies, those of the static large bodies' grid under [glo, ghi], those of the cell rows under
// [lo, hi] -- dealt to W lanes (W = 64: the lanes of a wave walk together; W = 1: one lane takes them all).  THE statement of "candidates under these bounds" of
// the queries and the characters (k_vehicle_cast's walk deals to 16-lane groups inside the step; the rays walk the cells along the ray: both stay their own).
template <int W, class F> SGP_DEV void sq_walk(const DV& d, v3 glo, v3 ghi, v3 lo, v3 hi, uint32_t lane, F fn)
{
	for (uint32_t l = lane; l < d.sp->n_large; l += W) fn(d.large_ids[l]);
	{
		uint32_t seen = 0;      // (dealt in the order the grid yields them)
		large_grid_query(d, glo, ghi, [&](uint32_t i) { if (W == 1 || (seen++ & (uint32_t)(W - 1)) == lane) fn(i); });
	}
	const BpGrid g = *d.grid;
	if (g.n_cells > 0 && g.min_x <= g.max_x) {
		const int x0 = max((int)floorf((lo.x - g.ox) * g.inv_cell) - 1, 0), x1 = min((int)floorf((hi.x - g.ox) * g.inv_cell) + 1, g.nx - 1);
		const int y0 = max((int)floorf((lo.y - g.oy) * g.inv_cell) - 1, 0), y1 = min((int)floorf((hi.y - g.oy) * g.inv_cell) + 1, g.ny - 1);
		const int z0 = max((int)floorf((lo.z - g.oz) * g.inv_cell) - 1, 0), z1 = min((int)floorf((hi.z - g.oz) * g.inv_cell) + 1, g.nz - 1);
		if (x0 <= x1) for (int z = z0; z <= z1; ++z) for (int y = y0; y <= y1; ++y) {
			grid_row_runs(d, g, x0, x1, y, z, [&](uint32_t c0, uint32_t c1) { for (uint32_t c = c0 + lane; c < c1; c += W) fn(__float_as_uint(d.sorted_max[c].w)); });
		}
	}
}
template <int W, class F> SGP_DEV void sq_walk(const DV& d, v3 lo, v3 hi, uint32_t lane, F fn) { sq_walk<W>(d, lo, hi, lo, hi, lane, fn); }

// a candidate on one of a call's pair lists (the lanes of the wave that append to the same list at the same time share one atomic)
SGP_DEV void pair_append(const PairLists& L, uint32_t* counter, uint2* list, uint32_t k, uint32_t j)
{
	const uint32_t at = wave_alloc(counter);
	if (at < L.pcap) list[at] = make_uint2(k, j);
}

// ---- capsule queries: one candidate body, one contact record ----

// point i of manifold g (normal: body -> query shape) as a contact of query k with body j
SGP_DEV sgp_query_contact contact_record(const DV& d, uint32_t k, uint32_t j, uint32_t f, int g, const sgd_manifold& m, int i)
{
	sgp_query_contact c;
	c.query = k; c.body = j; c.sub_shape = (uint32_t)(4 * g + i);      // point index for the host's sort; the host then stores the compound child index here
	c.point[0] = m.p1[i].x; c.point[1] = m.p1[i].y; c.point[2] = m.p1[i].z;
	c.normal[0] = m.n.x; c.normal[1] = m.n.y; c.normal[2] = m.n.z;
	c.distance = v3_dot(v3_sub(m.p2[i], m.p1[i]), m.n);
	v3 pv = V3(0.0f, 0.0f, 0.0f);
	if (f_motion(f) != SGP_MOTION_STATIC) pv = v3_add(V3(d.vel[VEL_F4 * (size_t)j]), v3_cross(V3(d.vel[VEL_F4 * (size_t)j + 1]), v3_sub(m.p1[i], V3(d.pose[POSE_F4 * (size_t)j]))));
	c.point_velocity[0] = pv.x; c.point_velocity[1] = pv.y; c.point_velocity[2] = pv.z;
	c.motion_type = f_motion(f); c.is_sensor = (f & BF_SENSOR) ? 1u : 0u; c.inv_mass = d.pose[POSE_F4 * (size_t)j].w; c.userdata = 0;
	return c;
}

// One candidate body of a capsule query, by one lane: the filters, then the collision test -- except for mesh bodies, which go on the wave's list (their
// triangles are the whole wave's work).  The sink says where things go: list_mesh(j) puts a mesh on the wave's list (false: the list is full), emit(j, f, g, m)
// takes manifold g of body j.
template <class Sink> SGP_DEV void capsule_query_body(const DV& d, uint32_t ignore, bool collidable_only, float max_sep, const sgd_shape& sc, v3 lo, v3 hi, uint32_t j, Sink& sink)
{
	if (j == ignore) return;
	const uint32_t f = d.flags[j];
	if (!(f & BF_ALIVE) || (f & BF_ALIAS)) return;
	const uint32_t layer = f_layer(f);
	if (collidable_only && !(layer == SGP_LAYER_NON_MOVING || layer == SGP_LAYER_MOVING)) return;      // (PlayerPhysicsObjectLayerFilter)
	const float4 mn = d.aabb_min[j], mx = d.aabb_max[j];
	if (mx.x < lo.x || mn.x > hi.x || mx.y < lo.y || mn.y > hi.y || mx.z < lo.z || mn.z > hi.z) return;
	const sgd_shape sb = load_shape(d, j, f);
	sgd_manifold mm[SGD_MESH_MAX_GROUPS]; int ng; bool dropped = false;
	if (sb.type == SGP_SHAPE_MESH) {
		if (sink.list_mesh(j)) return;
		ng = collide_with_mesh(d, j, sc, lo, hi, max_sep, mm, &dropped);      // (more meshes around one capsule than the list holds: this lane walks the rest)
	}
	else ng = (sb.type == SGP_SHAPE_HULL ? sgd_collide_hull(&sb, &sc, max_sep, &mm[0]) : sgd_collide(&sb, &sc, max_sep, &mm[0])) ? 1 : 0;   // normal: body -> capsule
	for (int g = 0; g < ng; ++g) sink.emit(j, f, g, mm[g]);
}

// ---- sphere casts: one candidate body, the walk under the swept sphere ----

struct SphereHit { float t; uint32_t id; v3 n; };      // the closest hit so far; ties go to the lower body id, so the answer does not depend on the order of the tests

SGP_DEV void spherecast_body(const DV& d, uint32_t ignore, bool collidable_only, float max_t, float rs, v3 o, v3 dir, uint32_t j, SphereHit& best)
{
	if (j == ignore) return;
	const uint32_t f = d.flags[j];
	if (!(f & BF_ALIVE) || (f & (BF_SENSOR | BF_ALIAS))) return;
	const uint32_t layer = f_layer(f);
	if (collidable_only && !(layer == SGP_LAYER_NON_MOVING || layer == SGP_LAYER_MOVING)) return;
	const float4 mn = d.aabb_min[j], mx = d.aabb_max[j];
	const float e = rs + 1.0e-3f;
	if (!ray_aabb(o, dir, make_float4(mn.x - e, mn.y - e, mn.z - e, 0.0f), make_float4(mx.x + e, mx.y + e, mx.z + e, 0.0f), max_t)) return;      // full length: see veh_cast_test
	const float4 sh = d.pose[POSE_F4 * (size_t)j + 3];
	const float prm[3] = { sh.x, sh.y, sh.z };
	v3 n, p;
	const float t = f_shape(f) == SGP_SHAPE_MESH ? cast_sphere_mesh(d, j, o, dir, best.t, rs, &n, &p)
	              : sgd_cast_sphere_body((int)f_shape(f), prm, f_shape(f) == SGP_SHAPE_HULL ? body_hull(d, sh) : nullptr, V3(d.pose[POSE_F4 * (size_t)j]), quat_to_m33(Q4(d.pose[POSE_F4 * (size_t)j + 1])), o, dir, best.t, rs, &n, &p);
	if (t >= 0.0f && t <= best.t && (t < best.t || best.id == SGP_INVALID_ID || j < best.id)) { best.t = t; best.id = j; best.n = n; }
}

// the candidates of a sphere cast: those under the swept sphere's bounds (casts are short: a character's step), the static large bodies' grid padded by
// rs + 2e-3, the cell rows by rs + 1e-3
template <int W, class F> SGP_DEV void spherecast_walk(const DV& d, v3 o, v3 dir, float max_t, float rs, uint32_t lane, F fn)
{
	const v3 e = v3_add(o, v3_scale(dir, max_t));
	const v3 mn = V3(fminf(o.x, e.x), fminf(o.y, e.y), fminf(o.z, e.z)), mx = V3(fmaxf(o.x, e.x), fmaxf(o.y, e.y), fmaxf(o.z, e.z));
	const float mg = rs + 2.0e-3f, mr = rs + 1.0e-3f;
	sq_walk<W>(d, V3(mn.x - mg, mn.y - mg, mn.z - mg), V3(mx.x + mg, mx.y + mg, mx.z + mg), V3(mn.x - mr, mn.y - mr, mn.z - mr), V3(mx.x + mr, mx.y + mr, mx.z + mr), lane, fn);
}
