// ht_model_build.hpp -- init-time model build: model JSON -> the named arrays the context loader consumes.
#pragma once
#include <stdint.h>
#include <map>
#include <string>
#include <vector>

// one named array of the HTFX container (dtype 0 = f32, 1 = i32, 2 = u16, 3 = u8)
struct fx_arr
{
	uint32_t dtype = 0, ndim = 0, dims[4] = { 0, 0, 0, 0 };
	std::vector<unsigned char> data;
	const float *f() const { return (const float *)data.data(); }
	const int *i() const { return (const int *)data.data(); }
};
typedef std::map<std::string, fx_arr> fx_map;

bool fx_load(const char *path, fx_map &out);
bool fx_save(const char *path, const fx_map &in);

// flags for ht_build_model
enum { HT_BUILD_HAND_TWEAKS = 1 };      // LoadHandModel()'s post-processing (handtrack.h:347-366)

// Parses a PhysModel JSON ("controlcages", "joints") and builds bodies, joints, physics constants and the UnibodyFit proxy.
bool ht_build_model(const char *json_path, int flags, fx_map &out, std::string &err);

// numeric top-level members of a JSON object file, as text
bool ht_json_top_level(const char *path, std::map<std::string, std::string> &numbers, std::string &err);

// The subdivision surface as the mesh ray cast reads it (ht_model_hitcheck_mesh, ht_render_mesh_depth): per triangle 16 floats,
// corners p0 p1 p2 (each padded to four floats) and PolyPlane({p0, p1, p2}) (geometric.h:247-260) in float, in that function's operation order.
// corners: [ntri][3][3] as ht_model_body_sdmesh hands them out.  ht_model_read and ht_model_rec_scale make a record's rows here.
void ht_mesh_rows(const float *corners, size_t ntri, float *rows16);

// The one host record of a model: what a context (ht_create) and the host view (ht_model_open) both keep, read by one reader and scaled by one statement of
// PhysModel::scale, so a scaled host model and a scaled context are bit-equal because they are the same code.  Geometry of all bodies back to back, body b's
// part from its offset to the next one's.
struct ht_model_rec
{
	int nb = 0, nj = 0;
	std::vector<int> vert_off{ 0 }, plane_off{ 0 }, tri_off{ 0 }, mesh_off{ 0 };      // [nb + 1]: first vertex, hull plane, hull triangle and mesh triangle of every body
	std::vector<float> verts, planes;                             // [..][3] com-centred hull vertices, [..][4] local half-space planes
	std::vector<int> tris;                                        // [..][3] hull triangles over a body's own vertices
	std::vector<float> corners, rows;                             // [t][9] the subdivision surface corner by corner, in the bone's rig frame (GetMeshes(true), physmodel.h:258); [t][16] ht_mesh_rows of them
	std::vector<float> bodyc, jointc;                             // [nb][HT_BC], [nj][HT_JC] as the device takes them; HT_BC_DAMPLEFT is the context's to fill (it needs the time step)
	std::vector<float> damping;                                   // [nb] the bodies' own damping, what HT_BC_DAMPLEFT is made from
	std::vector<int> collide, ignore, ignore_count;               // "body_collide" [nb], "ignore" [nb][nb], "ignore_count" [nb] (empty: a file from before it was stored) as the file has them
	std::vector<float> physics, ub_verts, ub_f;                   // "physics" [18], the unibody proxy "unibody/verts" [8][3] and "unibody/f" [18] as the file has them
	std::vector<std::string> missing;                             // entries the reader looked for in vain, in the order it looked; what to refuse over, and in which words, is the caller's
	unsigned gen = 0;                                             // counts the scalings: what was derived from the geometry (ht_render_depth's cull radii) is stale when it differs
	bool lacks(const char *name) const { for (const std::string &n : missing) if (n == name) return true; return false; }
};
// path (a model JSON, built with `flags`, or a model baked by ht_model_bake) -> record.  False with `err` set when the file cannot be opened, read or built; true
// otherwise, with rec.missing saying what the file lacks: without "nb" or "nj" nothing else is read, the bodies end at the first one without vertices or planes,
// a body without "tris" has no hull triangles, one without "sdverts" no mesh, the joint table is read when both joint arrays are there.
bool ht_model_read(const char *path, int flags, ht_model_rec &rec, std::string &err);
// PhysModel::scale (physmodel.h:196-219,304-319): vertices, plane offsets, mesh corners, centres of mass, radii and joint anchors times s, the inverse inertia over
// s * s; HT_BC_DIAM and the mesh rows made again from the scaled geometry
void ht_model_rec_scale(ht_model_rec &rec, float s);
