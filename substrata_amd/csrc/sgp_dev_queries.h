// sgp_dev_queries.h -- ray against a box; the query shape, filters and broad-phase walk that the overlap queries and the shape casts share.
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

// ---- what sgp_collide_shapes (sgp_k_shapequery.hip) and sgp_cast_shapes (sgp_k_shapecast.hip) share ----
// the query's shape record and, BOUNDS: its world bounds grown by max_separation (a capsule: the expressions of k_collide_capsules, bit for bit)
template <bool BOUNDS> SGP_DEV void sq_shape(const DV& d, const sgp_shape_query& q, sgd_shape& X, v3& lo, v3& hi)
{
	X.pos = V3(q.pos[0], q.pos[1], q.pos[2]);
	quat qq; qq.x = q.rot[0]; qq.y = q.rot[1]; qq.z = q.rot[2]; qq.w = q.rot[3];
	X.R = quat_to_m33(qq); X.type = (int)q.shape_type; X.hull = nullptr;
	if (q.shape_type == SGP_SHAPE_CAPSULE) {
		X.p0 = q.shape[0]; X.p1 = q.shape[1]; X.p2 = 0.0f;
		if (BOUNDS) {
			const v3 ax = v3_scale(X.R.c2, q.shape[1]);
			const float e = q.shape[0] + q.max_separation;
			const v3 ext = V3(fabsf(ax.x) + e, fabsf(ax.y) + e, fabsf(ax.z) + e);
			lo = v3_sub(X.pos, ext); hi = v3_add(X.pos, ext);
		}
		return;
	}
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

// fn(body) for the candidates of the bounds [lo, hi] -- the large bodies, those of the static large bodies' grid, those of the cell rows under the bounds --
// dealt to W lanes (W = 64: the lanes of a wave walk together, as k_collide_capsules does; W = 1: one lane takes them all)
template <int W, class F> SGP_DEV void sq_walk(const DV& d, v3 lo, v3 hi, uint32_t lane, F fn)
{
	for (uint32_t l = lane; l < d.sp->n_large; l += W) fn(d.large_ids[l]);
	{
		uint32_t seen = 0;
		large_grid_query(d, lo, hi, [&](uint32_t i) { if (W == 1 || (seen++ & (uint32_t)(W - 1)) == lane) fn(i); });
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
