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

// ------------------------------------------------------------------------------------------------- the record (ht_model_build.hpp)
static float body_diam(const ht_model_rec &rec, int b)      // HT_BC_DIAM: the largest distance between two of body b's vertices (the exact contact-patch shortcut uses it)
{
	float diam2 = 0.0f;
	for (int i = rec.vert_off[b]; i < rec.vert_off[b + 1]; i++) for (int j = i + 1; j < rec.vert_off[b + 1]; j++)
	{
		const float *p = &rec.verts[3 * (size_t)i], *q = &rec.verts[3 * (size_t)j], dx = p[0] - q[0], dy = p[1] - q[1], dz = p[2] - q[2];
		const float d2 = dx * dx + dy * dy + dz * dz; if (d2 > diam2) diam2 = d2;
	}
	return sqrtf(diam2);
}
bool ht_model_read(const char *path, int flags, ht_model_rec &rec, std::string &err)
{
	// `path` is either the reference's model JSON (built here, a33) or a model baked earlier with ht_model_bake
	fx_map fx;
	char magic[8] = { 0 };
	{ FILE *fp = fopen(path, "rb"); if (!fp) { err = std::string("cannot open model ") + path; return false; } size_t n = fread(magic, 1, 8, fp); (void)n; fclose(fp); }
	if (!memcmp(magic, "HTFX0001", 8)) { if (!fx_load(path, fx)) { err = std::string("cannot read baked model ") + path; return false; } }
	else if (!ht_build_model(path, flags, fx, err)) return false;
	rec = ht_model_rec();
	auto get = [&](const std::string &n) -> const fx_arr * { auto it = fx.find(n); if (it == fx.end()) { rec.missing.push_back(n); return nullptr; } return &it->second; };
	auto floats = [&](const fx_arr *a) { return a ? std::vector<float>(a->f(), a->f() + a->data.size() / 4) : std::vector<float>(); };
	auto ints = [&](const fx_arr *a) { return a ? std::vector<int>(a->i(), a->i() + a->data.size() / 4) : std::vector<int>(); };
	const fx_arr *nb = get("nb"), *nj = get("nj");
	if (!nb || !nj) return true;
	rec.nb = nb->i()[0]; rec.nj = nj->i()[0];
	const fx_arr *bf = get("body_f");
	rec.collide = ints(get("body_collide")); rec.ignore = ints(get("ignore"));
	const fx_arr *ji = get("joint_i"), *jf = get("joint_f");
	rec.physics = floats(get("physics")); rec.ub_verts = floats(get("unibody/verts")); rec.ub_f = floats(get("unibody/f"));
	{ auto it = fx.find("ignore_count"); if (it != fx.end()) rec.ignore_count = ints(&it->second); }
	for (int b = 0; bf && b < rec.nb; b++)
	{
		const std::string k = "b" + std::to_string(b);
		const fx_arr *v = get(k + "/verts"), *p = get(k + "/planes"), *t = get(k + "/tris");
		if (!v || !p) break;
		rec.verts.insert(rec.verts.end(), v->f(), v->f() + (size_t)v->dims[0] * 3);
		rec.planes.insert(rec.planes.end(), p->f(), p->f() + (size_t)p->dims[0] * 4);
		if (t) rec.tris.insert(rec.tris.end(), t->i(), t->i() + (size_t)t->dims[0] * 3);
		// the subdivision meshes (GetMeshes(true)); a baked model from before they were stored has none, and the mesh renderers then refuse
		auto sv = fx.find(k + "/sdverts");
		if (sv != fx.end()) rec.corners.insert(rec.corners.end(), sv->second.f(), sv->second.f() + (size_t)(sv->second.dims[0] / 3) * 9);
		rec.vert_off.push_back((int)(rec.verts.size() / 3)); rec.plane_off.push_back((int)(rec.planes.size() / 4));
		rec.tri_off.push_back((int)(rec.tris.size() / 3)); rec.mesh_off.push_back((int)(rec.corners.size() / 9));
		const float *r = bf->f() + 26 * b;     // mass massinv radius radius_inner damping friction gravscale com3 pos_start3 quat_start4 tensorinv9
		rec.bodyc.resize((size_t)(b + 1) * HT_BC, 0.0f); rec.damping.push_back(r[4]);
		float *c = &rec.bodyc[(size_t)b * HT_BC];
		c[HT_BC_MASS] = r[0]; c[HT_BC_MASSINV] = r[1]; c[HT_BC_RADIUS] = r[2]; c[HT_BC_RINNER] = r[3]; c[HT_BC_FRICTION] = r[5]; c[HT_BC_DIAM] = body_diam(rec, b);
		for (int i = 0; i < 3; i++) { c[HT_BC_COM + i] = r[7 + i]; c[HT_BC_POS0 + i] = r[10 + i]; }
		for (int i = 0; i < 4; i++) c[HT_BC_Q0 + i] = r[13 + i];
		for (int i = 0; i < 9; i++) c[HT_BC_TINV + i] = r[17 + i];
	}
	rec.rows.resize(rec.corners.size() / 9 * 16); ht_mesh_rows(rec.corners.data(), rec.corners.size() / 9, rec.rows.data());
	if (ji && jf && rec.nj > 0) rec.jointc.assign((size_t)rec.nj * HT_JC, 0.0f);
	for (size_t j = 0; j < rec.jointc.size() / HT_JC; j++)
	{
		float *c = &rec.jointc[j * HT_JC]; const float *r = jf->f() + 16 * j;      // p0 p1 rangemin rangemax jointframe
		c[HT_JC_RB0] = (float)ji->i()[2 * j]; c[HT_JC_RB1] = (float)ji->i()[2 * j + 1];
		for (int i = 0; i < 3; i++) { c[HT_JC_P0 + i] = r[i]; c[HT_JC_P1 + i] = r[3 + i]; c[HT_JC_RMIN + i] = r[6 + i]; c[HT_JC_RMAX + i] = r[9 + i]; }
		for (int i = 0; i < 4; i++) c[HT_JC_FRAME + i] = r[12 + i];
	}
	return true;
}
void ht_model_rec_scale(ht_model_rec &rec, float s)
{
	const float ss = s * s;
	for (float &v : rec.verts) v *= s;
	for (size_t k = 3; k < rec.planes.size(); k += 4) rec.planes[k] *= s;
	for (float &v : rec.corners) v *= s;      // scale(Mesh&) on the sdmeshes (physmodel.h:215-219,308-309)
	for (size_t b = 0; b < rec.bodyc.size() / HT_BC; b++)
	{
		float *c = &rec.bodyc[b * HT_BC];
		for (int i = 0; i < 3; i++) c[HT_BC_COM + i] *= s;
		c[HT_BC_RADIUS] *= s; c[HT_BC_RINNER] *= s;
		for (int i = 0; i < 9; i++) c[HT_BC_TINV + i] /= ss;
		c[HT_BC_DIAM] = body_diam(rec, (int)b);
	}
	for (size_t j = 0; j < rec.jointc.size() / HT_JC; j++) { float *c = &rec.jointc[j * HT_JC]; for (int i = 0; i < 3; i++) { c[HT_JC_P0 + i] *= s; c[HT_JC_P1 + i] *= s; } }
	ht_mesh_rows(rec.corners.data(), rec.corners.size() / 9, rec.rows.data());      // PolyPlane of the scaled corners
	rec.gen++;
}

// ------------------------------------------------------------------------------------------------- the host view
struct ht_model
{
	ht_model_rec rec;
	bool mirrored = false;      // ht_model_mirror was applied an odd number of times (ht_model_scale makes the mesh rows from the unmirrored corners)
	std::string err;
	int bodies() const { return (int)rec.vert_off.size() - 1; }      // the bodies held: nb of a model that opened
	bool has(int body) const { return body >= 0 && body < bodies(); }
	const float *com(int b) const { return &rec.bodyc[(size_t)b * HT_BC + HT_BC_COM]; }
};

extern "C" int ht_model_open(const char *path, int hand_tweaks, ht_model **out)
{
	if (!path || !out) return HT_ERR_ARG;
	ht_model *m = *out = new ht_model();
	const ht_model_rec &rec = m->rec;
	if (!ht_model_read(path, hand_tweaks ? HT_BUILD_HAND_TWEAKS : 0, m->rec, m->err)) return HT_ERR_IO;
	// this view needs the bodies whole (hull triangles included) and the joint table; the physics constants, collision lists and unibody proxy it can do without
	if (rec.lacks("nb") || rec.lacks("nj") || rec.lacks("body_f")) { m->err = "model entries missing"; return HT_ERR_IO; }
	for (const std::string &n : rec.missing) if (n[0] == 'b' && n[1] >= '0' && n[1] <= '9') { m->err = "model body arrays missing"; return HT_ERR_IO; }
	if (rec.nj > 0 && (rec.lacks("joint_i") || rec.lacks("joint_f"))) { m->err = "model joint arrays missing"; return HT_ERR_IO; }
	return HT_OK;
}
// the limits of the joint coordinates c = (s.x, s.y, t.z) (ConstrainAngularRangeW physics.h:351-393), as a context computes them at model load
extern "C" int ht_model_joint_limits(const ht_model *m, float *lo, float *hi, int *swapped)
{
	if (!m || m->rec.jointc.size() != (size_t)m->rec.nj * HT_JC) return HT_ERR_ARG;
	std::vector<float> jl((size_t)m->rec.nj * HT_JL, 0.0f);
	ht_joint_limits(m->rec.jointc.data(), m->rec.nj, jl.data());
	ht_joint_limits_public(jl.data(), m->rec.nj, lo, hi, swapped);
	return HT_OK;
}
extern "C" int ht_model_close(ht_model *m) { if (!m) return HT_ERR_ARG; delete m; return HT_OK; }
extern "C" const char *ht_model_error(const ht_model *m) { return m ? m->err.c_str() : "null model"; }
extern "C" int ht_model_counts(const ht_model *m, int *nb, int *nj) { if (!m) return HT_ERR_ARG; if (nb) *nb = m->rec.nb; if (nj) *nj = m->rec.nj; return HT_OK; }
extern "C" int ht_model_body(const ht_model *m, int body, int *nverts, int *ntris, int *nplanes, float *com3, float *rest_pose7)
{
	if (!m || !m->has(body)) return HT_ERR_ARG;
	const ht_model_rec &r = m->rec;
	if (nverts) *nverts = r.vert_off[body + 1] - r.vert_off[body];
	if (ntris) *ntris = r.tri_off[body + 1] - r.tri_off[body];
	if (nplanes) *nplanes = r.plane_off[body + 1] - r.plane_off[body];
	if (com3) memcpy(com3, m->com(body), 3 * sizeof(float));
	if (rest_pose7)      // position_start, orientation_start
	{
		memcpy(rest_pose7, &r.bodyc[(size_t)body * HT_BC + HT_BC_POS0], 3 * sizeof(float));
		memcpy(rest_pose7 + 3, &r.bodyc[(size_t)body * HT_BC + HT_BC_Q0], 4 * sizeof(float));
	}
	return HT_OK;
}
extern "C" int ht_model_body_mesh(const ht_model *m, int body, float *verts, int *tris)
{
	if (!m || !m->has(body)) return HT_ERR_ARG;
	const ht_model_rec &r = m->rec;
	if (verts) memcpy(verts, r.verts.data() + (size_t)3 * r.vert_off[body], (size_t)3 * (r.vert_off[body + 1] - r.vert_off[body]) * sizeof(float));
	if (tris) memcpy(tris, r.tris.data() + (size_t)3 * r.tri_off[body], (size_t)3 * (r.tri_off[body + 1] - r.tri_off[body]) * sizeof(int));
	return HT_OK;
}
// the subdivision surface of a body (PhysModel::sdmeshes, physmodel.h:258: MeshFlatShadeTex of the twice-subdivided control cage): *nverts corner positions, three per
// triangle in order, in the bone's rig frame -- drawn at Pose{PositionUser, orientation} (physmodel.h:297-298).  verts may be NULL to ask for the count.
extern "C" int ht_model_body_sdmesh(const ht_model *m, int body, int *nverts, float *verts)
{
	if (!m || !m->has(body)) return HT_ERR_ARG;
	const int t0 = m->rec.mesh_off[body], nt = m->rec.mesh_off[body + 1] - t0;
	if (nverts) *nverts = 3 * nt;
	if (verts) memcpy(verts, m->rec.corners.data() + (size_t)9 * t0, (size_t)9 * nt * sizeof(float));
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
	for (int b = 0; b < m->bodies(); b++)
	{
		const float *p = poses + 7 * b;
		const xf pose = XF(V3(p[0], p[1], p[2]), V4(p[3], p[4], p[5], p[6])), inv = inverse(pose);
		v3 a = apply(inv, v0w), c = apply(inv, impact), n = V3(0, 0, 0);
		bool hit = true;
		const float *pl = m->rec.planes.data();
		for (size_t k = (size_t)4 * m->rec.plane_off[b]; k < (size_t)4 * m->rec.plane_off[b + 1]; k += 4)      // ConvexHitCheck geometric.h:275-297
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

// PhysModel::scale (physmodel.h:196-219,304-319): ht_model_rec_scale, the statement ht_scale applies to a context's record, so a scaled host model and a scaled
// context are bit-equal.
static void model_mirror_arrays(ht_model *m);
extern "C" int ht_model_scale(ht_model *m, float s)
{
	if (!m || !(s > 0.0f)) return HT_ERR_ARG;
	if (m->mirrored) { model_mirror_arrays(m); const int r = ht_model_scale(m, s); model_mirror_arrays(m); return r; }      // PolyPlane's sums depend on the corner order: scaled as the right hand, so that scale and mirror commute to the bit
	ht_model_rec_scale(m->rec, s);
	return HT_OK;
}

// The left hand of this model: the mirror x -> -x of what is drawn and ray-cast, by sign flips and swaps of the stored arrays alone -- nothing is
// computed again, so twice is the identity byte for byte.  Vertices, corners and centres of mass: x negated.  Planes (hull planes, the meshes' PolyPlanes): x of the
// normal negated, the offset kept.  Rest poses: (-px,py,pz, qx,-qy,-qz,qw).  Triangles keep their first corner and swap the other two, which keeps them facing outwards.
// The joint table is left alone: the joint coordinates of a left hand are those of its mirror image.
static inline void flip_sign(float &v) { unsigned u; memcpy(&u, &v, 4); u ^= 0x80000000u; memcpy(&v, &u, 4); }
static void model_mirror_arrays(ht_model *m)
{
	ht_model_rec &R = m->rec;
	for (size_t k = 0; k < R.verts.size(); k += 3) flip_sign(R.verts[k]);
	for (size_t k = 0; k < R.planes.size(); k += 4) flip_sign(R.planes[k]);
	for (size_t k = 0; k + 2 < R.tris.size(); k += 3) std::swap(R.tris[k + 1], R.tris[k + 2]);
	for (size_t t = 0; t < R.corners.size() / 9; t++)
	{
		float *c = &R.corners[9 * t], *r = &R.rows[16 * t];
		for (int i = 0; i < 3; i++) { std::swap(c[3 + i], c[6 + i]); std::swap(r[4 + i], r[8 + i]); }
		for (int i = 0; i < 3; i++) { flip_sign(c[3 * i]); flip_sign(r[4 * i]); }
		flip_sign(r[12]);
	}
	for (size_t b = 0; b < R.bodyc.size() / HT_BC; b++)
	{
		float *c = &R.bodyc[b * HT_BC];
		flip_sign(c[HT_BC_COM]); flip_sign(c[HT_BC_POS0]); flip_sign(c[HT_BC_Q0 + 1]); flip_sign(c[HT_BC_Q0 + 2]);
	}
	m->mirrored = !m->mirrored;
}
// the stored planes of a body: its hull's [nplanes][4] and the PolyPlane [t][4] of every triangle of its subdivision mesh (what the two ray casts read); either may be null
extern "C" int ht_model_body_planes(const ht_model *m, int body, float *hull_planes, float *mesh_planes)
{
	if (!m || !m->has(body)) return HT_ERR_ARG;
	const ht_model_rec &r = m->rec;
	if (hull_planes) memcpy(hull_planes, r.planes.data() + (size_t)4 * r.plane_off[body], (size_t)4 * (r.plane_off[body + 1] - r.plane_off[body]) * sizeof(float));
	if (mesh_planes) for (int t = r.mesh_off[body]; t < r.mesh_off[body + 1]; t++) memcpy(mesh_planes + 4 * (t - r.mesh_off[body]), &r.rows[(size_t)16 * t + 12], 4 * sizeof(float));
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
	for (int b = 0; b < m->bodies(); b++)
	{
		const float *p = poses + 7 * b, *com = m->com(b);
		const v4 q = V4(p[3], p[4], p[5], p[6]);
		const xf U = XF(V3(p[0], p[1], p[2]) - qrot(q, V3(com[0], com[1], com[2])), q), inv = inverse(U);
		const v3 a = apply(inv, v0), c = apply(inv, v1);
		for (size_t k = 0; k < (size_t)(m->rec.mesh_off[b + 1] - m->rec.mesh_off[b]); k++)      // k: the triangle within the body
		{
			const float *r = &m->rec.rows[16 * (m->rec.mesh_off[b] + k)];
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
// one hand's layer: best [h][w] the winning counts (65536: not covered), who [h][w] the winning bodies (-1), through the principal point (px, py)
static void raster_layer(const ht_model *m, const float *poses, float fx, float fy, float px, float py, float ds, int w, int h, float far, float pixel_offset, std::vector<int> &best, std::vector<int> &who)
{
	best.assign((size_t)w * h, 65536); who.assign((size_t)w * h, -1);
	for (int b = 0; b < m->bodies(); b++)
	{
		const float *p = poses + 7 * b, *com = m->com(b);
		const m3 R = qmat(V4(p[3], p[4], p[5], p[6]));
		const v3 up = V3(p[0], p[1], p[2]) - mul(R, V3(com[0], com[1], com[2]));
		for (int k = m->rec.mesh_off[b]; k < m->rec.mesh_off[b + 1]; k++)
		{
			const float *c = &m->rec.corners[(size_t)9 * k];
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
}
static bool raster_args_ok(const void *m, const void *poses, const void *cam12, const void *depth, int w, int h, float far, float pixel_offset)
{
	return m && poses && cam12 && depth && w >= 1 && h >= 1 && w <= 4096 && h <= 4096 && far > 0.0f && pixel_offset >= 0.0f && pixel_offset <= 1.0f;
}
extern "C" int ht_model_raster_mesh(const ht_model *m, const float *poses, const float *cam12, int w, int h, float far, float pixel_offset, uint16_t *depth, int8_t *body)
{
	if (!raster_args_ok(m, poses, cam12, depth, w, h, far, pixel_offset)) return HT_ERR_ARG;
	const float ds = cam12[4];
	std::vector<int> best, who;
	raster_layer(m, poses, cam12[0], cam12[1], cam12[2], cam12[3], ds, w, h, far, pixel_offset, best, who);
	const unsigned short bg = (unsigned short)(far / ds);
	for (size_t o = 0; o < best.size(); o++)
	{
		depth[o] = who[o] >= 0 ? (unsigned short)best[o] : bg;
		if (body) body[o] = (int8_t)who[o];
	}
	return HT_OK;
}

// A scene of H hands in one z-buffer (the definition is in include/ht_mi355x.h): the layer of every instance that is present, a left one from its
// mirrored pose through the mirrored principal point and read at the flipped column (ht_raster.hpp), then the smallest count per pixel, the lowest instance on equal
// counts, over the background frame.  This is the definition ht_raster_scene_depth is held to.
extern "C" int ht_model_raster_scene(const ht_model *m, const float *poses, const uint8_t *hands, int H, const float *cam12, int w, int h, float far, float pixel_offset,
                                     const uint16_t *bg, uint16_t *depth, int8_t *hand, int8_t *body, int32_t *visible)
{
	if (!raster_args_ok(m, poses, cam12, depth, w, h, far, pixel_offset) || H < 1 || H > HT_SCENE_MAX_HANDS) return HT_ERR_ARG;
	const int nb = m->bodies();
	if (!rz_scene_fits(H, m->rec.mesh_off[nb])) { const_cast<ht_model *>(m)->err = "ht_model_raster_scene: instances times mesh triangles exceed 65535"; return HT_ERR_STATE; }
	const size_t npx = (size_t)w * h, db = npx * sizeof(uint16_t);
	// bg == depth exactly composes in place (a pixel is read, then written); any other overlap of an output with a buffer of the call is refused
	const struct { const void *p; size_t n; } buf[7] = { { depth, db }, { hand, npx }, { body, npx }, { visible, (size_t)H * sizeof(int32_t) }, { bg == depth ? nullptr : bg, db },
	                                                     { poses, (size_t)H * nb * 7 * sizeof(float) }, { cam12, 12 * sizeof(float) } };
	for (int i = 0; i < 4; i++) for (int j = i + 1; j < 7; j++)
		if (buf[i].p && buf[j].p && (uintptr_t)buf[i].p < (uintptr_t)buf[j].p + buf[j].n && (uintptr_t)buf[j].p < (uintptr_t)buf[i].p + buf[i].n) return HT_ERR_ARG;
	const float fx = cam12[0], fy = cam12[1], px = cam12[2], py = cam12[3], ds = cam12[4];
	std::vector<int> cnt(npx, 65536), inst(npx, -1), bod(npx, -1), best, who;
	std::vector<float> mp((size_t)nb * 7);
	for (int i = 0; i < H; i++)
	{
		const unsigned char flag = hands ? hands[i] : 0;
		if (rz_scene_absent(flag)) continue;
		const bool left = rz_scene_left(flag);
		const float *p = poses + (size_t)i * nb * 7;
		if (left) { for (int b = 0; b < nb; b++) rz_mirror_pose(p + 7 * b, &mp[(size_t)7 * b]); p = mp.data(); }
		raster_layer(m, p, fx, fy, left ? rz_mirror_px(px, w, pixel_offset) : px, py, ds, w, h, far, pixel_offset, best, who);
		for (int y = 0; y < h; y++) for (int x = 0; x < w; x++)
		{
			const size_t o = (size_t)y * w + x, l = (size_t)y * w + rz_scene_column(x, w, left);      // the layer is read at the flipped column
			if (who[l] >= 0 && best[l] < cnt[o]) { cnt[o] = best[l]; inst[o] = i; bod[o] = who[l]; }
		}
	}
	const unsigned short none = (unsigned short)(far / ds);
	if (visible) for (int i = 0; i < H; i++) visible[i] = 0;
	for (size_t o = 0; o < npx; o++)
	{
		const unsigned short bgv = bg ? bg[o] : none;
		const bool on = inst[o] >= 0 && rz_scene_wins(cnt[o], bg != nullptr, bgv);
		depth[o] = on ? (unsigned short)cnt[o] : bgv;
		if (hand) hand[o] = (int8_t)(on ? inst[o] : -1);
		if (body) body[o] = (int8_t)(on ? bod[o] : -1);
		if (on && visible) visible[inst[o]]++;
	}
	return HT_OK;
}
