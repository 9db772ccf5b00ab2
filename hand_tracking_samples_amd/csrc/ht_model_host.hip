// ht_model_host.hip -- host-only view of a built hand model behind the C-ABI (ht_model_*): what an application needs from a PhysModel object
// that is NOT being tracked -- the reference's synthetic-tracker keeps such a "fake hand" to pose, draw and ray-cast its input frames
// (synthetic-hand-tracker/synthetic-tracker.cpp:94-96,139,69-76).  No device call is made here.
//
// Reference interfaces: PhysModel::PhysModel(const char*) + LoadHandModel() (include/physmodel.h:444-475, include/handtrack.h:347-366) through the
// same host builder ht_create uses; PhysModel::HitCheck (physmodel.h:287-294) = ConvexHitCheck of every body's hull planes
// (third_party/geometric.h:275-302); RigidBody::PositionUser (third_party/physics.h:142).
#include <string.h>
#include <string>
#include <vector>
#include "ht_device.hpp"
#include "ht_model_build.hpp"
#include "ht_launch.hpp"
#include "ht_raster.hpp"

struct ht_model
{
	int nb = 0, nj = 0;
	std::vector<std::vector<float>> verts, planes;      // per body: [n][3] com-centred vertices, [n][4] local half-space planes
	std::vector<std::vector<int>> tris;                 // per body: [n][3] hull triangles over verts
	std::vector<std::vector<float>> sdverts;            // per body: [3 t][3] the subdivision surface's triangles corner by corner, in the bone's rig frame (GetMeshes(true), physmodel.h:258)
	std::vector<std::vector<float>> sdrows;             // per body: [t][16] corners and PolyPlane of every sdverts triangle (ht_mesh_rows), what the mesh ray cast reads
	std::vector<float> com, rest;                       // [nb][3], [nb][7]
	std::vector<float> jointc;                          // [nj][HT_JC] the joint table as a context keeps it
	bool mirrored = false;                              // ht_model_mirror was applied an odd number of times (ht_model_scale makes the mesh rows from the unmirrored corners)
	std::string err;
};

extern "C" int ht_model_open(const char *path, int hand_tweaks, ht_model **out)
{
	if (!path || !out) return HT_ERR_ARG;
	ht_model *m = new ht_model();
	*out = m;
	fx_map fx;
	char magic[8] = { 0 };
	{ FILE *fp = fopen(path, "rb"); if (!fp) { m->err = std::string("cannot open model ") + path; return HT_ERR_IO; } size_t n = fread(magic, 1, 8, fp); (void)n; fclose(fp); }
	if (!memcmp(magic, "HTFX0001", 8)) { if (!fx_load(path, fx)) { m->err = std::string("cannot read baked model ") + path; return HT_ERR_IO; } }
	else if (!ht_build_model(path, hand_tweaks ? HT_BUILD_HAND_TWEAKS : 0, fx, m->err)) return HT_ERR_IO;
	auto get = [&](const std::string &n) -> const fx_arr * { auto it = fx.find(n); return it == fx.end() ? nullptr : &it->second; };
	const fx_arr *nb = get("nb"), *nj = get("nj"), *bf = get("body_f");
	if (!nb || !nj || !bf) { m->err = "model entries missing"; return HT_ERR_IO; }
	m->nb = nb->i()[0]; m->nj = nj->i()[0];
	for (int b = 0; b < m->nb; b++)
	{
		const std::string k = "b" + std::to_string(b);
		const fx_arr *v = get(k + "/verts"), *p = get(k + "/planes"), *t = get(k + "/tris");
		if (!v || !p || !t) { m->err = "model body arrays missing"; return HT_ERR_IO; }
		m->verts.emplace_back(v->f(), v->f() + (size_t)v->dims[0] * 3);
		m->planes.emplace_back(p->f(), p->f() + (size_t)p->dims[0] * 4);
		m->tris.emplace_back(t->i(), t->i() + (size_t)t->dims[0] * 3);
		const fx_arr *sv = get(k + "/sdverts");
		if (sv) m->sdverts.emplace_back(sv->f(), sv->f() + (size_t)sv->dims[0] * 3); else m->sdverts.emplace_back();
		m->sdrows.emplace_back((m->sdverts.back().size() / 9) * 16);
		ht_mesh_rows(m->sdverts.back().data(), m->sdverts.back().size() / 9, m->sdrows.back().data());
		const float *r = bf->f() + 26 * b;      // mass massinv radius radius_inner damping friction gravscale com3 pos_start3 quat_start4 tensorinv9
		m->com.insert(m->com.end(), r + 7, r + 10);
		m->rest.insert(m->rest.end(), r + 10, r + 17);
	}
	const fx_arr *ji = get("joint_i"), *jf = get("joint_f");
	if (m->nj > 0 && (!ji || !jf)) { m->err = "model joint arrays missing"; return HT_ERR_IO; }
	m->jointc.assign((size_t)m->nj * HT_JC, 0.0f);
	for (int j = 0; j < m->nj; j++)
	{
		float *c = &m->jointc[(size_t)j * HT_JC]; const float *r = jf->f() + 16 * j;      // p0 p1 rangemin rangemax jointframe
		c[HT_JC_RB0] = (float)ji->i()[2 * j]; c[HT_JC_RB1] = (float)ji->i()[2 * j + 1];
		for (int i = 0; i < 3; i++) { c[HT_JC_P0 + i] = r[i]; c[HT_JC_P1 + i] = r[3 + i]; c[HT_JC_RMIN + i] = r[6 + i]; c[HT_JC_RMAX + i] = r[9 + i]; }
		for (int i = 0; i < 4; i++) c[HT_JC_FRAME + i] = r[12 + i];
	}
	return HT_OK;
}
// the limits of the joint coordinates c = (s.x, s.y, t.z) (ConstrainAngularRangeW physics.h:351-393), as a context computes them at model load
extern "C" int ht_model_joint_limits(const ht_model *m, float *lo, float *hi, int *swapped)
{
	if (!m || m->jointc.size() != (size_t)m->nj * HT_JC) return HT_ERR_ARG;
	std::vector<float> jl((size_t)m->nj * HT_JL, 0.0f);
	ht_joint_limits(m->jointc.data(), m->nj, jl.data());
	ht_joint_limits_public(jl.data(), m->nj, lo, hi, swapped);
	return HT_OK;
}
extern "C" int ht_model_close(ht_model *m) { if (!m) return HT_ERR_ARG; delete m; return HT_OK; }
extern "C" const char *ht_model_error(const ht_model *m) { return m ? m->err.c_str() : "null model"; }
extern "C" int ht_model_counts(const ht_model *m, int *nb, int *nj) { if (!m) return HT_ERR_ARG; if (nb) *nb = m->nb; if (nj) *nj = m->nj; return HT_OK; }
extern "C" int ht_model_body(const ht_model *m, int body, int *nverts, int *ntris, int *nplanes, float *com3, float *rest_pose7)
{
	if (!m || body < 0 || body >= m->nb) return HT_ERR_ARG;
	if (nverts) *nverts = (int)m->verts[body].size() / 3;
	if (ntris) *ntris = (int)m->tris[body].size() / 3;
	if (nplanes) *nplanes = (int)m->planes[body].size() / 4;
	if (com3) memcpy(com3, &m->com[3 * body], 3 * sizeof(float));
	if (rest_pose7) memcpy(rest_pose7, &m->rest[7 * body], 7 * sizeof(float));
	return HT_OK;
}
extern "C" int ht_model_body_mesh(const ht_model *m, int body, float *verts, int *tris)
{
	if (!m || body < 0 || body >= m->nb) return HT_ERR_ARG;
	if (verts) memcpy(verts, m->verts[body].data(), m->verts[body].size() * sizeof(float));
	if (tris) memcpy(tris, m->tris[body].data(), m->tris[body].size() * sizeof(int));
	return HT_OK;
}
// the subdivision surface of a body (PhysModel::sdmeshes, physmodel.h:258: MeshFlatShadeTex of the twice-subdivided control cage): *nverts corner positions, three per
// triangle in order, in the bone's rig frame -- drawn at Pose{PositionUser, orientation} (physmodel.h:297-298).  verts may be NULL to ask for the count.
extern "C" int ht_model_body_sdmesh(const ht_model *m, int body, int *nverts, float *verts)
{
	if (!m || body < 0 || body >= m->nb) return HT_ERR_ARG;
	if (nverts) *nverts = (int)m->sdverts[body].size() / 3;
	if (verts) memcpy(verts, m->sdverts[body].data(), m->sdverts[body].size() * sizeof(float));
	return HT_OK;
}
// PhysModel::HitCheck(v0, v1): the segment is clipped against the hull of every body in turn, each body starting from the impact the previous
// ones left (physmodel.h:291), so the nearest hit along the segment wins.  poses [nb][7] = the bodies' poses (centre-of-mass frames).
extern "C" int ht_model_hitcheck(const ht_model *m, const float *poses, const float *v0_, const float *v1_, float *impact3, float *normal3, int *body_out)
{
	if (!m || !poses || !v0_ || !v1_) return HT_ERR_ARG;
	const v3 v0w = V3(v0_[0], v0_[1], v0_[2]);
	v3 impact = V3(v1_[0], v1_[1], v1_[2]), normal = V3(0, 0, 0);
	int who = -1;
	for (int b = 0; b < m->nb; b++)
	{
		const float *p = poses + 7 * b;
		const xf pose = XF(V3(p[0], p[1], p[2]), V4(p[3], p[4], p[5], p[6])), inv = inverse(pose);
		v3 a = apply(inv, v0w), c = apply(inv, impact), n = V3(0, 0, 0);
		bool hit = true;
		const std::vector<float> &pl = m->planes[b];
		for (size_t k = 0; k + 3 < pl.size(); k += 4)      // ConvexHitCheck geometric.h:275-297
		{
			const v4 plane = V4(pl[k], pl[k + 1], pl[k + 2], pl[k + 3]);
			const float d0 = dot_plane(plane, a), d1 = dot_plane(plane, c);
			if (d0 >= 0 && d1 >= 0) { hit = false; break; }
			if (d0 <= 0 && d1 <= 0) continue;
			const v3 x = a + ((c - a) * d0) / (d0 - d1);
			if (d0 >= 0) { n = xyz(plane); a = x; } else c = x;
		}
		if (hit) { impact = apply(pose, a); normal = qrot(pose.q, n); who = b; }
	}
	if (impact3) { impact3[0] = impact.x; impact3[1] = impact.y; impact3[2] = impact.z; }
	if (normal3) { normal3[0] = normal.x; normal3[1] = normal.y; normal3[2] = normal.z; }
	if (body_out) *body_out = who;
	return HT_OK;
}

// PhysModel::scale (physmodel.h:196-219,304-319) for what this view holds: hull vertices and plane offsets, the subdivision meshes and the centres of mass times s,
// the operations ht_scale applies to a context's model, so a scaled host model and a scaled context stay bit-equal.  The mesh planes are made again from the scaled corners.
static void model_mirror_arrays(ht_model *m);
extern "C" int ht_model_scale(ht_model *m, float s)
{
	if (!m || !(s > 0.0f)) return HT_ERR_ARG;
	if (m->mirrored) { model_mirror_arrays(m); const int r = ht_model_scale(m, s); model_mirror_arrays(m); return r; }      // PolyPlane's sums depend on the corner order: scaled as the right hand, so that scale and mirror commute to the bit
	for (int b = 0; b < m->nb; b++)
	{
		for (auto &v : m->verts[b]) v *= s;
		for (size_t k = 3; k < m->planes[b].size(); k += 4) m->planes[b][k] *= s;
		for (auto &v : m->sdverts[b]) v *= s;
		ht_mesh_rows(m->sdverts[b].data(), m->sdverts[b].size() / 9, m->sdrows[b].data());
	}
	for (auto &v : m->com) v *= s;
	return HT_OK;
}

// The left hand of this model: the mirror x -> -x of what is drawn and ray-cast, by sign flips and swaps of the stored arrays alone -- nothing is
// computed again, so twice is the identity byte for byte.  Vertices, corners and centres of mass: x negated.  Planes (hull planes, the meshes' PolyPlanes): x of the
// normal negated, the offset kept.  Rest poses: (-px,py,pz, qx,-qy,-qz,qw).  Triangles keep their first corner and swap the other two, which keeps them facing outwards.
// The joint table is left alone: the joint coordinates of a left hand are those of its mirror image.
static inline void flip_sign(float &v) { unsigned u; memcpy(&u, &v, 4); u ^= 0x80000000u; memcpy(&v, &u, 4); }
static void model_mirror_arrays(ht_model *m)
{
	for (int b = 0; b < m->nb; b++)
	{
		for (size_t k = 0; k < m->verts[b].size(); k += 3) flip_sign(m->verts[b][k]);
		for (size_t k = 0; k < m->planes[b].size(); k += 4) flip_sign(m->planes[b][k]);
		for (size_t k = 0; k + 2 < m->tris[b].size(); k += 3) std::swap(m->tris[b][k + 1], m->tris[b][k + 2]);
		std::vector<float> &sv = m->sdverts[b], &sr = m->sdrows[b];
		for (size_t t = 0; t < sv.size() / 9; t++)
		{
			float *c = &sv[9 * t], *r = &sr[16 * t];
			for (int i = 0; i < 3; i++) { std::swap(c[3 + i], c[6 + i]); std::swap(r[4 + i], r[8 + i]); }
			for (int i = 0; i < 3; i++) { flip_sign(c[3 * i]); flip_sign(r[4 * i]); }
			flip_sign(r[12]);
		}
		flip_sign(m->com[3 * b]);
		float *p = &m->rest[7 * b];
		flip_sign(p[0]); flip_sign(p[4]); flip_sign(p[5]);
	}
	m->mirrored = !m->mirrored;
}
// the stored planes of a body: its hull's [nplanes][4] and the PolyPlane [t][4] of every triangle of its subdivision mesh (what the two ray casts read); either may be null
extern "C" int ht_model_body_planes(const ht_model *m, int body, float *hull_planes, float *mesh_planes)
{
	if (!m || body < 0 || body >= m->nb) return HT_ERR_ARG;
	if (hull_planes) memcpy(hull_planes, m->planes[body].data(), m->planes[body].size() * sizeof(float));
	if (mesh_planes) for (size_t t = 0; t < m->sdrows[body].size() / 16; t++) memcpy(mesh_planes + 4 * t, &m->sdrows[body][16 * t + 12], 4 * sizeof(float));
	return HT_OK;
}
extern "C" int ht_model_mirror(ht_model *m)
{
	if (!m) return HT_ERR_ARG;
	model_mirror_arrays(m);
	return HT_OK;
}

// The ray cast against the subdivision surface GetMeshes(true) hands to a renderer (physmodel.h:295-303): the software statement of the application's default depth
// source (synthetic-tracker.cpp:164-165), built from PolyHitCheck (geometric.h:263-273) alone.  Every triangle of every body is tested on the whole segment, in the
// frame of its mesh pose U_b = {pos_b - qrot(q_b, com_b), q_b}; the candidate with the smallest d0 / (d0 - d1) wins, the first in (body, triangle) order on a tie.
// No culling of any kind: this is the definition ht_render_mesh_depth is held to.
struct mesh_hit { int body, tri; v3 impact, normal; };
static mesh_hit mesh_hitcheck(const ht_model *m, const float *poses, v3 v0, v3 v1)
{
	mesh_hit h; h.body = -1; h.tri = -1; h.impact = v1; h.normal = V3(0, 0, 0);
	float best = INFINITY;
	for (int b = 0; b < m->nb; b++)
	{
		const float *p = poses + 7 * b;
		const v4 q = V4(p[3], p[4], p[5], p[6]);
		const xf U = XF(V3(p[0], p[1], p[2]) - qrot(q, V3(m->com[3 * b], m->com[3 * b + 1], m->com[3 * b + 2])), q), inv = inverse(U);
		const v3 a = apply(inv, v0), c = apply(inv, v1);
		const std::vector<float> &R = m->sdrows[b];
		for (size_t k = 0; 16 * k < R.size(); k++)
		{
			const float *r = &R[16 * k];
			const v4 P = V4(r[12], r[13], r[14], r[15]);
			const float d0 = dot_plane(P, a), d1 = dot_plane(P, c);
			if (!(d0 > 0 && d1 < 0)) continue;
			const v3 t[3] = { V3(r[0], r[1], r[2]), V3(r[4], r[5], r[6]), V3(r[8], r[9], r[10]) };
			bool hit = true;
			for (int i = 0; hit && i < 3; i++) { m3 M; M.x = t[(i + 1) % 3] - a; M.y = t[i] - a; M.z = c - a; hit = determinant(M) >= 0; }
			if (!hit) continue;
			const float tt = d0 / (d0 - d1);
			if (!(tt < best)) continue;
			best = tt; h.body = b; h.tri = (int)k;
			h.impact = apply(U, a + ((c - a) * d0) / (d0 - d1));
			h.normal = qrot(q, xyz(P));
		}
	}
	return h;
}
extern "C" int ht_model_hitcheck_mesh(const ht_model *m, const float *poses, const float *v0, const float *v1, float *impact3, float *normal3, int *body, int *tri)
{
	if (!m || !poses || !v0 || !v1) return HT_ERR_ARG;
	const mesh_hit h = mesh_hitcheck(m, poses, V3(v0[0], v0[1], v0[2]), V3(v1[0], v1[1], v1[2]));
	if (impact3) { impact3[0] = h.impact.x; impact3[1] = h.impact.y; impact3[2] = h.impact.z; }
	if (normal3) { normal3[0] = h.normal.x; normal3[1] = h.normal.y; normal3[2] = h.normal.z; }
	if (body) *body = h.body;
	if (tri) *tri = h.tri;
	return HT_OK;
}
// One frame: pixel (x, y) = (uint16)(impact.z / depth_scale) of the segment from the origin to deprojectz((x + pixel_offset, y + pixel_offset), far) (misc_image.h:48).
// A plain loop over pixels, bodies and triangles.  cam12: focal, principal point and depth_scale are used, the camera's pose is not.
extern "C" int ht_model_render_mesh(const ht_model *m, const float *poses, const float *cam12, int w, int h, float far, float pixel_offset, uint16_t *depth, int8_t *body)
{
	if (!m || !poses || !cam12 || !depth || w < 1 || h < 1 || w > 4096 || h > 4096 || !(far > 0.0f) || !(pixel_offset >= 0.0f && pixel_offset <= 1.0f)) return HT_ERR_ARG;
	const float fx = cam12[0], fy = cam12[1], px = cam12[2], py = cam12[3], ds = cam12[4];
	for (int y = 0; y < h; y++) for (int x = 0; x < w; x++)
	{
		const v3 v1 = V3((((float)x + pixel_offset) - px) / fx * far, (((float)y + pixel_offset) - py) / fy * far, far);
		const mesh_hit hit = mesh_hitcheck(m, poses, V3(0.0f, 0.0f, 0.0f), v1);
		depth[(size_t)y * w + x] = (unsigned short)(hit.impact.z / ds);
		if (body) body[(size_t)y * w + x] = (int8_t)hit.body;
	}
	return HT_OK;
}

// The forward z-buffer rasteriser of the same meshes (the definition is in include/ht_mi355x.h and, per triangle and pixel, in ht_raster.hpp):
// a plain loop over bodies, triangles and the pixels of each triangle's own rectangle.  The smallest count wins a pixel, the first in (body, triangle) order on equal
// counts.  This is the definition ht_raster_mesh_depth is held to.
extern "C" int ht_model_raster_mesh(const ht_model *m, const float *poses, const float *cam12, int w, int h, float far, float pixel_offset, uint16_t *depth, int8_t *body)
{
	if (!m || !poses || !cam12 || !depth || w < 1 || h < 1 || w > 4096 || h > 4096 || !(far > 0.0f) || !(pixel_offset >= 0.0f && pixel_offset <= 1.0f)) return HT_ERR_ARG;
	const float fx = cam12[0], fy = cam12[1], px = cam12[2], py = cam12[3], ds = cam12[4];
	std::vector<int> best((size_t)w * h, 65536), who((size_t)w * h, -1);
	for (int b = 0; b < m->nb; b++)
	{
		const float *p = poses + 7 * b;
		const m3 R = qmat(V4(p[3], p[4], p[5], p[6]));
		const v3 up = V3(p[0], p[1], p[2]) - mul(R, V3(m->com[3 * b], m->com[3 * b + 1], m->com[3 * b + 2]));
		const std::vector<float> &C = m->sdverts[b];
		for (size_t k = 0; 9 * k < C.size(); k++)
		{
			const float *c = &C[9 * k];
			rz_tri T;
			if (!rz_setup(R, up, V3(c[0], c[1], c[2]), V3(c[3], c[4], c[5]), V3(c[6], c[7], c[8]), fx, fy, px, py, pixel_offset, T)) continue;
			int x0, x1, y0, y1;
			rz_rect(T, x0, x1, y0, y1);
			x0 = x0 < 0 ? 0 : x0; y0 = y0 < 0 ? 0 : y0; x1 = x1 > w - 1 ? w - 1 : x1; y1 = y1 > h - 1 ? h - 1 : y1;
			for (int y = y0; y <= y1; y++) for (int x = x0; x <= x1; x++)
			{
				if (!rz_inside(T, x, y)) continue;
				const int n = rz_count(T, rz_ray(x, pixel_offset, px, fx), rz_ray(y, pixel_offset, py, fy), far, ds);
				const size_t o = (size_t)y * w + x;
				if (n >= 0 && n < best[o]) { best[o] = n; who[o] = b; }
			}
		}
	}
	const unsigned short bg = (unsigned short)(far / ds);
	for (size_t o = 0; o < best.size(); o++)
	{
		depth[o] = who[o] >= 0 ? (unsigned short)best[o] : bg;
		if (body) body[o] = (int8_t)who[o];
	}
	return HT_OK;
}
