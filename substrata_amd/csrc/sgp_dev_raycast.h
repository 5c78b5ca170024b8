// sgp_dev_raycast.h -- one ray against the world (traceRay and doesRayHitAnything, PhysicsWorld.cpp:1668-1725), closest hit and any hit from one text: the
// per-shape test (ray_body), the per-body test (ray_test and its three fetch orders) and the world walk (raycast_world; raycast_one and raycast_any_one are
// its two instantiations).  The walk of the static large bodies' grid and the resident server's raycast_wave step their cells with CellWalk
// (sgp_dev_broadphase.h); raycast_world keeps that text written out for its cells, for the measured reason given there.
// Included after sgp_dev_all.h by sgp_k_queries.hip (k_raycast, k_raycast_any, the resident ray server), sgp_k_particles.hip (k_particles_update),
// sgp_k_crafts.hip (through sgp_dev_crafts.h) and sgp_k_audibility.hip (k_aud_rays): every one of them compiles this text, so a particle's, a craft's or an
// audio source's ray is answered with the bits k_raycast / k_raycast_any give the same ray.
//
// ANY, the compile-time flag all three carry: leave at the first accepted hit.  The closest-hit search runs every test under a cut-off it shrinks from
// max_t; the any form leaves before it could shrink one, so its cut-off is max_t throughout.  Each test accepts under a larger cut-off what it accepts under
// a smaller one (docs/GAPS.md), hence raycast_any_one(d, ry) == (raycast_one(d, ry).id != SGP_INVALID_ID).  The any form uses no normal, RaySub or
// barycentrics: what only they need is dead code in its instantiation.
#pragma once

struct RaySub { uint32_t tri, mat; float u, v; };      // which triangle of a mesh a ray hit, its user data, barycentrics

// t of the ray's hit on one shape within max_t, or -1 (ANY: of the first hit found, not the closest)
template <bool ANY> SGP_DEV float ray_body(const DV& d, uint32_t type, float4 sh, v3 pos, quat q, v3 o, v3 dir, float max_t, v3* n_out, RaySub* sub)
{
	const m33 R = quat_to_m33(q);
	const v3 ol = m33_tmul(R, v3_sub(o, pos)), dl = m33_tmul(R, dir);
	sub->tri = SGP_INVALID_ID; sub->mat = 0; sub->u = 0.0f; sub->v = 0.0f;
	if (type == SGP_SHAPE_MESH) {
		const MeshHeader mh = d.meshes[(uint32_t)sh.x];
		// a height field: the blocks and cells under the path (field_cast, out of line), no stack (its walk keeps a closest hit under ANY too)
		if (mh.kind == MESH_KIND_FIELD) {
			const FieldCastHit h = field_cast(d.mesh_field, mh, ol, dl, 0.0f, max_t, true);
			if (h.tri == 0xFFFFFFFFu) return -1.0f;
			sub->tri = h.tri; sub->mat = h.mat; sub->u = h.u; sub->v = h.v;
			*n_out = m33_mul(R, h.n);
			return h.t;
		}
		// closest front-facing triangle; on equal distance the lower triangle index (caller's order) wins
		float best = max_t; uint32_t best_idx = 0xFFFFFFFFu; v3 bn = V3(0.0f, 0.0f, 0.0f);
		const v3 inv = V3(fabsf(dl.x) > 1.0e-12f ? 1.0f / dl.x : 3.0e38f, fabsf(dl.y) > 1.0e-12f ? 1.0f / dl.y : 3.0e38f, fabsf(dl.z) > 1.0e-12f ? 1.0f / dl.z : 3.0e38f);
		uint32_t stack[48]; int sp = 0;
		stack[sp++] = 0;
		while (sp > 0) {
			const MeshNode nd = d.mesh_nodes[mh.node_off + stack[--sp]];
			// slab test against the node box grown a little (never rejects a triangle the exact test would accept)
			const float g = 1.0e-4f * (1.0f + fabsf(nd.mxx) + fabsf(nd.mxy) + fabsf(nd.mxz) + fabsf(nd.mnx) + fabsf(nd.mny) + fabsf(nd.mnz));
			float t0 = 0.0f, t1 = best; bool miss = false;
			const float lo3[3] = { nd.mnx - g, nd.mny - g, nd.mnz - g }, hi3[3] = { nd.mxx + g, nd.mxy + g, nd.mxz + g };
			const float o3[3] = { ol.x, ol.y, ol.z }, d3[3] = { dl.x, dl.y, dl.z }, i3[3] = { inv.x, inv.y, inv.z };
			for (int a = 0; a < 3 && !miss; ++a) {
				if (fabsf(d3[a]) <= 1.0e-12f) { if (o3[a] < lo3[a] || o3[a] > hi3[a]) miss = true; }
				else { float ta = (lo3[a] - o3[a]) * i3[a], tb = (hi3[a] - o3[a]) * i3[a]; if (ta > tb) { const float tmp = ta; ta = tb; tb = tmp; } t0 = fmaxf(t0, ta - g); t1 = fminf(t1, tb + g); if (t0 > t1) miss = true; }
			}
			if (miss) continue;
			if (nd.count == 0) { if (sp + 2 <= 48) { stack[sp++] = nd.left; stack[sp++] = nd.right; } continue; }
			for (uint32_t k = 0; k < nd.count; ++k) {
				const MeshTri tr = mesh_tri(d, mh, nd.left + k);
				float uv[2];
				const float tt = sgd_ray_tri_uv(ol, dl, tr.a, tr.b, tr.c, best, ANY ? (float*)0 : uv);
				if (ANY && tt >= 0.0f) return tt;      // the first triangle that answers
				if (tt >= 0.0f && (tt < best || best_idx == 0xFFFFFFFFu || (tt == best && tr.index < best_idx))) {
					best = tt; best_idx = tr.index;
					const v3 nn = v3_cross(v3_sub(tr.b, tr.a), v3_sub(tr.c, tr.a)); bn = v3_scale(nn, 1.0f / v3_len(nn));
					sub->tri = tr.index; sub->mat = tr.mat; sub->u = uv[0]; sub->v = uv[1];
				}
			}
		}
		if (best_idx == 0xFFFFFFFFu) return -1.0f;
		*n_out = m33_mul(R, bn);
		return best;
	}
	if (type == SGP_SHAPE_HULL) {
		v3 nl;
		const float t = sgd_ray_hull(body_hull(d, sh), ol, dl, max_t, 0.0f, &nl);
		if (t < 0.0f) return -1.0f;
		*n_out = m33_mul(R, nl);
		return t;
	}
	if (type == SGP_SHAPE_SPHERE) {
		const float r = sh.x;
		const float B = v3_dot(ol, dl), C = v3_len_sq(ol) - r * r;
		if (C <= 0.0f) { *n_out = v3_neg(dir); return 0.0f; }
		const float disc = B * B - C;
		if (disc < 0.0f) return -1.0f;
		const float t = -B - sqrtf(disc);
		if (t < 0.0f || t > max_t) return -1.0f;
		*n_out = m33_mul(R, v3_scale(v3_add(ol, v3_scale(dl, t)), 1.0f / r));
		return t;
	}
	if (type == SGP_SHAPE_BOX) {
		const v3 h = V3(sh.x, sh.y, sh.z);
		float t0 = 0.0f, t1 = max_t; int ax = -1; float sg = 0.0f;
		for (int k = 0; k < 3; ++k) {
			const float ok = v3_get(ol, k), dk = v3_get(dl, k), hk = v3_get(h, k);
			if (fabsf(dk) < 1.0e-12f) { if (ok < -hk || ok > hk) return -1.0f; continue; }
			float ta = (-hk - ok) / dk, tb = (hk - ok) / dk; float s = -1.0f;
			if (ta > tb) { const float tmp = ta; ta = tb; tb = tmp; s = 1.0f; }
			if (ta > t0) { t0 = ta; ax = k; sg = s; }
			if (tb < t1) t1 = tb;
			if (t0 > t1) return -1.0f;
		}
		if (ax < 0) { *n_out = v3_neg(dir); return 0.0f; }
		v3 nl = V3(0.0f, 0.0f, 0.0f); v3_set(nl, ax, sg);
		*n_out = m33_mul(R, nl);
		return t0;
	}
	{
		const float r = sh.x, hh = sh.y;
		{      // starting inside comes first (else an interior cap-sphere entry can win, depending on max_t; see sgd_ray_capsule_z)
			const v3 qq = sgd_closest_on_segment(V3(0.0f, 0.0f, -hh), V3(0.0f, 0.0f, hh), ol);
			if (v3_len_sq(v3_sub(ol, qq)) <= r * r) { *n_out = v3_neg(dir); return 0.0f; }
		}
		float best = -1.0f; v3 bn = V3(0.0f, 0.0f, 0.0f);
		const float a = dl.x * dl.x + dl.y * dl.y;
		const float bq = ol.x * dl.x + ol.y * dl.y, c = ol.x * ol.x + ol.y * ol.y - r * r;
		if (a > 1.0e-12f) {
			const float disc = bq * bq - a * c;
			if (disc >= 0.0f) {
				const float t = (-bq - sqrtf(disc)) / a;
				const float z = ol.z + dl.z * t;
				if (t >= 0.0f && t <= max_t && fabsf(z) <= hh) { if (ANY) return t; best = t; bn = V3((ol.x + dl.x * t) / r, (ol.y + dl.y * t) / r, 0.0f); }
			}
		}
		for (int sgn = -1; sgn <= 1; sgn += 2) {
			const v3 oc = V3(ol.x, ol.y, ol.z - (float)sgn * hh);
			const float B = v3_dot(oc, dl), C = v3_len_sq(oc) - r * r;
			const float disc = B * B - C;
			if (disc < 0.0f) continue;
			const float t = -B - sqrtf(disc);
			if (t < 0.0f || t > max_t) continue;
			if (ANY) return t;
			if (best < 0.0f || t < best) { best = t; bn = v3_scale(v3_add(oc, v3_scale(dl, t)), 1.0f / r); }
		}
		if (best < 0.0f) return -1.0f;
		*n_out = m33_mul(R, bn);
		return best;
	}
}

struct RayBest { float t; uint32_t id; v3 n; RaySub sub; };
SGP_DEV RayBest ray_best_none(float max_t)
{
	RayBest best; best.t = max_t; best.id = SGP_INVALID_ID; best.n = V3(0.0f, 0.0f, 0.0f);
	best.sub.tri = SGP_INVALID_ID; best.sub.mat = 0; best.sub.u = best.sub.v = 0.0f;
	return best;
}

// Body i against the ray: the filters, the bounds, the shape, the best hit kept in `best`; true: the search is over (ANY, at its first accepted hit).  The
// body's records are read through the pointers where the test gets to them, so the caller decides the order of the fetches: see the three forms below.
template <bool ANY> SGP_DEV bool ray_test(const DV& d, const sgp_ray& ry, v3 o, v3 dir, uint32_t i, const uint32_t* flags, const float4* amin, const float4* amax, const float4* prop1, const float4* pose0, const float4* pose1, RayBest& best)
{
	if (i == ry.ignore_id) return false;
	const uint32_t f = *flags;
	if (!(f & BF_ALIVE) || (f & BF_ALIAS)) return false;
	const uint32_t layer = f_layer(f);
	if (ry.collidable_only && !(layer == SGP_LAYER_NON_MOVING || layer == SGP_LAYER_MOVING)) return false;
	if (!ray_aabb(o, dir, *amin, *amax, best.t)) return false;
	v3 nn; RaySub sub;
	const float t = ray_body<ANY>(d, f_shape(f), *prop1, V3(*pose0), Q4(*pose1), o, dir, best.t, &nn, &sub);
	// closest hit; ties go to the lower body id so the result does not depend on the traversal order
	if (!(t >= 0.0f && t <= best.t && (t < best.t || best.id == SGP_INVALID_ID || i < best.id))) return false;
	best.t = t; best.id = i;
	if (!ANY) { best.n = nn; best.sub = sub; }
	return ANY;
}
// ... fetched as the test needs them (the batched kernels, bound by throughput, keep the tests between the fetches: flags, then bounds, then pose and shape)
template <bool ANY> SGP_DEV bool ray_test_body(const DV& d, const sgp_ray& ry, v3 o, v3 dir, uint32_t i, RayBest& best)
{
	return ray_test<ANY>(d, ry, o, dir, i, &d.flags[i], &d.aabb_min[i], &d.aabb_max[i], &d.pose[POSE_F4 * (size_t)i + 3], &d.pose[POSE_F4 * (size_t)i], &d.pose[POSE_F4 * (size_t)i + 1], best);
}
// ... already at hand (the resident server's large bodies, cached in LDS)
SGP_DEV void ray_test_loaded(const DV& d, const sgp_ray& ry, v3 o, v3 dir, uint32_t i, uint32_t f, float4 amin, float4 amax, float4 prop1, float4 pose0, float4 pose1, RayBest& best)
{
	ray_test<false>(d, ry, o, dir, i, &f, &amin, &amax, &prop1, &pose0, &pose1, best);
}
// ... all fetched at once (the resident server: a lone wave waits for every dependent fetch in full -- flags, then bounds, then pose and shape is three
// round trips to memory where this is one)
SGP_DEV void ray_test_body_eager(const DV& d, const sgp_ray& ry, v3 o, v3 dir, uint32_t i, RayBest& best)
{
	const uint32_t f = d.flags[i];
	const float4 amin = d.aabb_min[i], amax = d.aabb_max[i], prop1 = d.pose[POSE_F4 * (size_t)i + 3], pose0 = d.pose[POSE_F4 * (size_t)i], pose1 = d.pose[POSE_F4 * (size_t)i + 1];
	ray_test<false>(d, ry, o, dir, i, &f, &amin, &amax, &prop1, &pose0, &pose1, best);
}

// One ray against the world, one thread per ray.  Large bodies (ground quad ...) are tested directly, the static large bodies through their grid, small
// bodies through a 3D-DDA walk of the broad-phase cell grid (bodies are binned by centre and reach at most one cell beyond it, so every visited cell also
// looks at its 26 neighbours), stopping once the cell entry distance passes the best hit.  ANY: back with the first accepted hit.
template <bool ANY> SGP_DEV RayBest raycast_world(const DV& d, const sgp_ray& ry)
{
	const v3 o = V3(ry.origin[0], ry.origin[1], ry.origin[2]), dir = V3(ry.dir[0], ry.dir[1], ry.dir[2]);
	RayBest best = ray_best_none(ry.max_t);
	for (uint32_t l = 0; l < d.sp->n_large; ++l) if (ray_test_body<ANY>(d, ry, o, dir, d.large_ids[l], best)) return best;
	if (large_grid_ray(d, o, dir, &best.t, [&](uint32_t i) { return ray_test_body<ANY>(d, ry, o, dir, i, best); })) return best;
	const BpGrid g = *d.grid;
	if (g.n_cells > 0 && g.min_x <= g.max_x) {
		// Clip to the grid box inflated by one cell and walk the cells: the text of CellWalk (sgp_dev_broadphase.h) written out, with a miss flag and nested
		// blocks where CellWalk leaves by return.  Over CellWalk k_raycast measured 20 to 25 % slower on incoherent rays (profiles/ray_walk_fold.md): the
		// two must be edited together.
		const float c = g.cell;
		const v3 lo = V3(g.ox - c, g.oy - c, g.oz - c);
		const v3 hi = V3(g.ox + ((float)g.nx + 1.0f) * c, g.oy + ((float)g.ny + 1.0f) * c, g.oz + ((float)g.nz + 1.0f) * c);
		float t0 = 0.0f, t1 = best.t; bool miss = false;
		const float oo[3] = { o.x, o.y, o.z }, dd[3] = { dir.x, dir.y, dir.z };
		const float bl[3] = { lo.x, lo.y, lo.z }, bh[3] = { hi.x, hi.y, hi.z };
		for (int a = 0; a < 3 && !miss; ++a) {
			if (fabsf(dd[a]) < 1.0e-12f) { if (oo[a] < bl[a] || oo[a] > bh[a]) miss = true; }
			else {
				float ta = (bl[a] - oo[a]) / dd[a], tb = (bh[a] - oo[a]) / dd[a];
				if (ta > tb) { const float tmp = ta; ta = tb; tb = tmp; }
				t0 = fmaxf(t0, ta); t1 = fminf(t1, tb);
				if (t0 > t1) miss = true;
			}
		}
		if (!miss) {
			const v3 p0 = v3_add(o, v3_scale(dir, t0));
			int cx = (int)floorf((p0.x - g.ox) * g.inv_cell), cy = (int)floorf((p0.y - g.oy) * g.inv_cell), cz = (int)floorf((p0.z - g.oz) * g.inv_cell);
			cx = min(max(cx, -1), g.nx); cy = min(max(cy, -1), g.ny); cz = min(max(cz, -1), g.nz);
			const int sx = dir.x > 0.0f ? 1 : -1, sy = dir.y > 0.0f ? 1 : -1, sz = dir.z > 0.0f ? 1 : -1;
			const float inf = 3.0e38f;
			const float tdx = fabsf(dir.x) > 1.0e-12f ? c / fabsf(dir.x) : inf, tdy = fabsf(dir.y) > 1.0e-12f ? c / fabsf(dir.y) : inf, tdz = fabsf(dir.z) > 1.0e-12f ? c / fabsf(dir.z) : inf;
			float tmx = fabsf(dir.x) > 1.0e-12f ? ((g.ox + (float)(cx + (sx > 0 ? 1 : 0)) * c) - o.x) / dir.x : inf;
			float tmy = fabsf(dir.y) > 1.0e-12f ? ((g.oy + (float)(cy + (sy > 0 ? 1 : 0)) * c) - o.y) / dir.y : inf;
			float tmz = fabsf(dir.z) > 1.0e-12f ? ((g.oz + (float)(cz + (sz > 0 ? 1 : 0)) * c) - o.z) / dir.z : inf;
			float t_enter = t0;
			for (int iter = 0; iter < 100000; ++iter) {
				if (t_enter - 2.0f * c > best.t) break;           // nothing nearer can come from cells this far along the ray
				for (int dz = -1; dz <= 1; ++dz) for (int dy = -1; dy <= 1; ++dy) {
					const int y = cy + dy, z = cz + dz;
					if (y < 0 || y >= g.ny || z < 0 || z >= g.nz) continue;
					const int xa = max(cx - 1, 0), xb = min(cx + 1, g.nx - 1);
					if (xa > xb) continue;
					bool over = false;
					grid_row_runs(d, g, xa, xb, y, z, [&](uint32_t q0, uint32_t q1) { for (uint32_t q = q0; q < q1 && !over; ++q) over = ray_test_body<ANY>(d, ry, o, dir, __float_as_uint(d.sorted_max[q].w), best); });
					if (over) return best;
				}
				if (tmx <= tmy && tmx <= tmz) { t_enter = tmx; tmx += tdx; cx += sx; if (cx < -1 || cx > g.nx) break; }
				else if (tmy <= tmz) { t_enter = tmy; tmy += tdy; cy += sy; if (cy < -1 || cy > g.ny) break; }
				else { t_enter = tmz; tmz += tdz; cz += sz; if (cz < -1 || cz > g.nz) break; }
				if (t_enter > t1) break;
			}
		}
	}
	return best;
}

// traceRay (PhysicsWorld.cpp:1668-1725)
SGP_DEV sgp_hit raycast_one(const DV& d, const sgp_ray& ry)
{
	const RayBest best = raycast_world<false>(d, ry);
	sgp_hit h;
	h.id = best.id; h.t = best.id == SGP_INVALID_ID ? 0.0f : best.t;
	h.normal[0] = best.n.x; h.normal[1] = best.n.y; h.normal[2] = best.n.z;
	h.triangle = best.sub.tri; h.material = best.sub.mat; h.bary[0] = best.sub.u; h.bary[1] = best.sub.v; h.sub_shape = 0;
	h.userdata = 0;
	return h;
}
// "does this ray hit anything within max_t" (JPH::NarrowPhaseQuery::CastRay with the plain result, which PhysicsWorld::doesRayHitAnything calls)
SGP_DEV bool raycast_any_one(const DV& d, const sgp_ray& ry) { return raycast_world<true>(d, ry).id != SGP_INVALID_ID; }
