// ht_handtrack.hpp -- C++ wrappers over the C-ABI (ht_mi355x.h) that keep the reference's own names and signatures, so that
// code written against include/handtrack.h / third_party/cnn.h of IntelRealSense/hand_tracking_samples keeps compiling:
//
//     HandTracker htk;                                   // handtrack.h:830 (paths are constructor arguments here)
//     htk.microforce = 3.0f; htk.mainthreadpasses = 3;   // synthetic-tracker.cpp:91-93
//     std::vector<Pose> pose = htk.update(std::move(dimage));      // handtrack.h:748
//     std::vector<float> y = htk.cnn.Eval(x);                        // cnn.h:550
//
// Provided: the members the per-frame path and synthetic-tracker.cpp touch: HandTracker {update, update_cnn_model, kickstart, slowfit,
// scale, load_config, handmodel / othermodel facades, cnn, cnn_input, cnn_output, cnn_output_analysis}, CNN {Eval, Train, loadb, saveb},
// PoseInitializerCNN, PhysModel / LoadHandModel (a host-side model that is posed, drawn and ray-cast, never tracked), HandSegmentVR, camsub,
// GatherHandExpectedCNN, Pose / Image<T> / DCamera / Mesh.  Define HT_MI355X_GLOBAL_NAMES before including to have these names in the global
// namespace, as the reference's headers put them.  Caller-built constraint rows cross the boundary too: LimitLinear / LimitAngular (physics.h:239-308) hold
// RigidBody pointers into a tracked model's `rigidbodies`, handmodel.FitPointCloud(points, linears, angulars, microforce) (physmodel.h:345) and the free
// PhysicsUpdate(Addresses(model.rigidbodies), linears, angulars) (physics.h:543) keep the reference's signatures.  Documented deviation: update()
// runs the CNN job synchronously every frame (the reference polls a background std::async job for 1 ms, which makes its output
// timing dependent, handtrack.h:755-768); this is HandTracker::update_cnn_model followed by the main-thread passes.
// Errors are reported the way the reference's apps expect them: by throwing std::runtime_error (synthetic-tracker.cpp:255-264).
#pragma once
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <fstream>
#include <limits>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>
#include "ht_mi355x.h"

namespace ht_mi355x
{
struct float2 { float x, y; };
struct int2 { int x, y; };
struct int3 { int x, y, z; };
struct float3 { float x, y, z; };
struct float4 { float x, y, z, w; };
struct Pose { float3 position{ 0, 0, 0 }; float4 orientation{ 0, 0, 0, 1 }; };            // geometric.h:111-125

class DCamera                                                                                // misc_image.h:30-55
{
	int2 dim_{ 64, 64 }; float2 focal_{ 164.f, 164.f }; float2 principal_{ 32.f, 32.f };
public:
	float depth_scale = 0.001f; Pose pose;
	DCamera() {}
	DCamera(int2 dim, float2 focal, float2 principal, float depth_scale, Pose pose = Pose()) : dim_(dim), focal_(focal), principal_(principal), depth_scale(depth_scale), pose(pose) {}
	int2 &dim() { return dim_; } const int2 &dim() const { return dim_; }
	float2 &focal() { return focal_; } const float2 &focal() const { return focal_; }
	float2 &principal() { return principal_; } const float2 &principal() const { return principal_; }
};
template <class T> struct Image                                                              // misc_image.h:109-129
{
	DCamera cam; std::vector<T> raster;
	Image() {}
	Image(DCamera cam) : cam(cam), raster((size_t)cam.dim().x * cam.dim().y, T()) {}
	Image(DCamera cam, std::vector<T> data) : cam(cam), raster(std::move(data)) {}
	const int2 dim() const { return cam.dim(); }
	T &pixel(int2 p) { return raster[(size_t)p.y * dim().x + p.x]; }
};

// ---- constraint rows a caller builds (physics.h:239-308).  A RigidBody here is a handle to body `index` of one of a tracker's two models: rows hold
//      RigidBody pointers exactly like the reference's (NULL = the world) and only live as long as the HandTracker they point into.
struct RigidBody { ht_ctx *ctx = nullptr; int which = 0, index = 0; };
struct LimitAngular
{
	RigidBody *rb0 = nullptr, *rb1 = nullptr; float3 axis{ 0, 0, 1 }; float torque = 0, targetspin = 0, mintorque = -FLT_MAX, maxtorque = FLT_MAX;
	LimitAngular() {}
	LimitAngular(RigidBody *rb0, RigidBody *rb1, const float3 &axis, float targetspin = 0, float mintorque = -FLT_MAX, float maxtorque = FLT_MAX)
		: rb0(rb0), rb1(rb1), axis(axis), targetspin(targetspin), mintorque(mintorque), maxtorque(maxtorque) {}                                 // physics.h:248-249
};
struct LimitLinear
{
	RigidBody *rb0 = nullptr, *rb1 = nullptr; float3 position0{ 0, 0, 0 }, position1{ 0, 0, 0 }, normal{ 0, 0, 1 };
	float targetdist = 0, targetspeednobias = 0; float2 forcelimit{ -FLT_MAX, FLT_MAX }; int friction_master = 0; float targetspeed = 0, impulsesum = 0;
	LimitLinear() {}
	LimitLinear(RigidBody *rb0, RigidBody *rb1, const float3 &position0, const float3 &position1, const float3 &normal = float3{ 0, 0, 1 }, float targetdist = 0.0f,
	            float targetspeednobias = 0.0f, const float2 forcelimit = { -FLT_MAX, FLT_MAX })
		: rb0(rb0), rb1(rb1), position0(position0), position1(position1), normal(normal), targetdist(targetdist), targetspeednobias(targetspeednobias),
		  forcelimit{ forcelimit.x < forcelimit.y ? forcelimit.x : forcelimit.y, forcelimit.x < forcelimit.y ? forcelimit.y : forcelimit.x } {}   // physics.h:283-287
};
template <class T> std::vector<T *> Addresses(std::vector<T> &v) { std::vector<T *> a; for (auto &e : v) a.push_back(&e); return a; }             // misc.h
namespace detail
{
	inline void pack_rows(const std::vector<LimitLinear> &L, const std::vector<LimitAngular> &A, std::vector<float> &l, std::vector<float> &a)
	{
		for (auto &c : L)
		{
			const float r[16] = { c.rb0 ? (float)c.rb0->index : -1.0f, c.rb1 ? (float)c.rb1->index : -1.0f, c.position0.x, c.position0.y, c.position0.z, c.position1.x, c.position1.y, c.position1.z,
			                      c.normal.x, c.normal.y, c.normal.z, c.targetdist, c.targetspeednobias, c.forcelimit.x, c.forcelimit.y, (float)c.friction_master };
			l.insert(l.end(), r, r + 16);
		}
		for (auto &c : A)
		{
			const float r[8] = { c.rb0 ? (float)c.rb0->index : -1.0f, c.rb1 ? (float)c.rb1->index : -1.0f, c.axis.x, c.axis.y, c.axis.z, c.targetspin, c.mintorque, c.maxtorque };
			a.insert(a.end(), r, r + 8);
		}
	}
}
// void PhysicsUpdate(const std::vector<RigidBody*> &rigidbodies, std::vector<LimitLinear> &Linears, std::vector<LimitAngular> &Angulars, wgeom) (physics.h:543-587):
// one solver step of the model the bodies belong to under the caller's rows (plus the collision rows); `rigidbodies` must be all bodies of one tracked model
inline void PhysicsUpdate(const std::vector<RigidBody *> &rigidbodies, std::vector<LimitLinear> &Linears, std::vector<LimitAngular> &Angulars, const std::vector<std::vector<float3> *> &wgeom = {})
{
	if (rigidbodies.empty() || !rigidbodies[0]) throw std::runtime_error("PhysicsUpdate: no bodies");
	if (!wgeom.empty()) throw std::runtime_error("PhysicsUpdate: world geometry is not supported (every call site of the reference passes none)");
	for (size_t i = 0; i < rigidbodies.size(); i++) if (!rigidbodies[i] || rigidbodies[i]->ctx != rigidbodies[0]->ctx || rigidbodies[i]->which != rigidbodies[0]->which || rigidbodies[i]->index != (int)i) throw std::runtime_error("PhysicsUpdate: pass Addresses(model.rigidbodies) of one tracked model");
	std::vector<float> l, a; detail::pack_rows(Linears, Angulars, l, a);
	const int nl = (int)Linears.size(), na = (int)Angulars.size();
	if (ht_physics_update(rigidbodies[0]->ctx, rigidbodies[0]->which, 1, l.data(), nl, &nl, a.data(), na, &na) != HT_OK) throw std::runtime_error(std::string("PhysicsUpdate: ") + ht_last_error(rigidbodies[0]->ctx));
}

// std::vector<float3> PointCloud(const Image<T> &dimage, float2 filter_range) (misc_image.h:409-417): the in-range pixels of a depth image as camera-space
// points, in row-major order (what synthetic-tracker.cpp:233 draws; the tracker's own cloud is made on the device, k_prepare).  Same expressions as the
// reference: d = pixel * depth_scale, kept when filter_range.x <= d < filter_range.y, point = ((x - cx) / fx, (y - cy) / fy, 1) * d.
template <class T> std::vector<float3> PointCloud(const Image<T> &dimage, float2 filter_range)
{
	std::vector<float3> pointcloud;
	const DCamera &c = dimage.cam;
	for (int y = 0; y < dimage.dim().y; y++) for (int x = 0; x < dimage.dim().x; x++)
	{
		const float d = dimage.raster[(size_t)y * dimage.dim().x + x] * c.depth_scale;
		if (d >= filter_range.x && d < filter_range.y) pointcloud.push_back({ ((float)x - c.principal().x) / c.focal().x * d, ((float)y - c.principal().y) / c.focal().y * d, 1.0f * d });
	}
	return pointcloud;
}
inline DCamera camsub(const DCamera &c, int s)                                               // misc_image.h:60
{
	return DCamera({ c.dim().x / s, c.dim().y / s }, { c.focal().x / (float)s, c.focal().y / (float)s }, { c.principal().x / (float)s, c.principal().y / (float)s }, c.depth_scale, c.pose);
}
// Addition (left hands, include/ht_mi355x.h "left hands"): a pose under the mirror x -> -x, (px,py,pz, qx,qy,qz,qw) -> (-px,py,pz, qx,-qy,-qz,qw)
inline Pose mirrored(const Pose &p) { Pose q = p; q.position.x = -p.position.x; q.orientation.y = -p.orientation.y; q.orientation.z = -p.orientation.z; return q; }
inline std::vector<Pose> mirrored(std::vector<Pose> v) { for (auto &p : v) p = mirrored(p); return v; }
struct Mesh { std::vector<float3> verts; std::vector<int3> tris; Pose pose; float4 hack{ 1, 1, 1, 1 }; std::string material; };      // mesh.h (what GetMeshes hands to a renderer)
namespace detail
{
// PhysModel::sdmeshes[body] (physmodel.h:258): the twice-subdivided control cage, flat-shaded -- three fresh vertices per triangle, as MeshFlatShadeTex lays them out
// (mesh.h:154-177; positions only: the tangent frames and texture coordinates a renderer derives from them are not part of this surface)
inline Mesh subdivision_mesh(const ht_model *m, int body)
{
	Mesh mesh; int nv = 0;
	ht_model_body_sdmesh(m, body, &nv, nullptr);
	std::vector<float> v((size_t)nv * 3);
	ht_model_body_sdmesh(m, body, nullptr, v.data());
	for (int i = 0; i < nv; i++) mesh.verts.push_back({ v[3 * i], v[3 * i + 1], v[3 * i + 2] });
	for (int i = 0; i + 2 < nv; i += 3) mesh.tris.push_back({ i, i + 1, i + 2 });
	return mesh;
}
// PhysModel::meshes[body]: the collision hull in the centre-of-mass frame (ht_model_body_mesh)
inline Mesh hull_mesh(const ht_model *m, int body)
{
	Mesh mesh; int nv = 0, nt = 0;
	ht_model_body(m, body, &nv, &nt, nullptr, nullptr, nullptr);
	std::vector<float> v((size_t)nv * 3); std::vector<int> t((size_t)nt * 3);
	ht_model_body_mesh(m, body, v.data(), t.data());
	for (int i = 0; i < nv; i++) mesh.verts.push_back({ v[3 * i], v[3 * i + 1], v[3 * i + 2] });
	for (int i = 0; i < nt; i++) mesh.tris.push_back({ t[3 * i], t[3 * i + 1], t[3 * i + 2] });
	return mesh;
}
}

// ---- the host-side image helpers the applications draw with (synthetic-tracker.cpp:191,206,208-209,218,221-222): plain loops over small rasters, no device work.
//      Same names and results as the reference's templates; written for this Image / DCamera.
struct byte3 { unsigned char x, y, z; byte3() : x(0), y(0), z(0) {} byte3(unsigned char a, unsigned char b, unsigned char c) : x(a), y(b), z(c) {} explicit byte3(int v) : x((unsigned char)v), y((unsigned char)v), z((unsigned char)v) {} };      // linalg.h:355
inline bool operator==(const byte3 &a, const byte3 &b) { return a.x == b.x && a.y == b.y && a.z == b.z; }
// Transform(image, f) (misc_image.h:165): f over every pixel, the camera kept
template <typename F, typename S> auto Transform(const Image<S> &src, F f) -> Image<decltype(f(S()))>
{
	Image<decltype(f(S()))> dst; dst.cam = src.cam; dst.raster.reserve(src.raster.size());
	for (const S &v : src.raster) dst.raster.push_back(f(v));
	return dst;
}
inline unsigned char ToGrayScale(float x) { const float v = x * 255.0f; return (unsigned char)(v < 0.0f ? 0.0f : (v > 255.0f ? 255.0f : v)); }      // misc_image.h:169 (truncating, clamp first)
inline unsigned char ToGrayScale(unsigned char x) { return x; }
template <class T> Image<unsigned char> ToGrayScale(const Image<T> &src) { return Transform(src, [](T x) { return ToGrayScale(x); }); }                   // misc_image.h:172
inline Image<byte3> ToRGB(const Image<unsigned char> &src) { return Transform(src, [](unsigned char p) { return byte3(p, p, p); }); }                    // misc_image.h:173
inline Image<byte3> ToRGB(const Image<float> &src) { return ToRGB(ToGrayScale(src)); }
// UpSample (misc_image.h:96-102,135): every pixel becomes a 2x2 block; the camera's dimensions, focal lengths and principal point double (operator*, :61)
template <class T> Image<T> UpSample(const Image<T> &src)
{
	const int w = src.dim().x, h = src.dim().y;
	Image<T> dst; dst.cam = DCamera({ w * 2, h * 2 }, { src.cam.focal().x * 2.0f, src.cam.focal().y * 2.0f }, { src.cam.principal().x * 2.0f, src.cam.principal().y * 2.0f }, src.cam.depth_scale, src.cam.pose);
	dst.raster.resize(src.raster.size() * 4);
	for (int y = 0; y < 2 * h; y++) for (int x = 0; x < 2 * w; x++) dst.raster[(size_t)y * 2 * w + x] = src.raster[(size_t)(y / 2) * w + x / 2];
	return dst;
}
// ImageConcat (misc_image.h:225-238): the images stacked top to bottom in a canvas as wide as the widest, each row copied to the left edge
template <class T> Image<T> ImageConcat(const std::vector<Image<T>> &images)
{
	int w = 0, h = 0;
	for (auto &im : images) { w = im.dim().x > w ? im.dim().x : w; h += im.dim().y; }
	Image<T> dst; dst.cam = DCamera({ w, h }, { (float)w, (float)h }, { (float)w / 2.0f, (float)h / 2.0f }, 0.001f); dst.cam.depth_scale = DCamera().depth_scale;      // DCamera(int2 dim), misc_image.h:47
	dst.raster.assign((size_t)w * h, T());
	size_t row = 0;
	for (auto &im : images) for (int y = 0; y < im.dim().y; y++, row++) for (int x = 0; x < im.dim().x; x++) dst.raster[row * w + x] = im.raster[(size_t)y * im.dim().x + x];
	return dst;
}
// ImageOverlayYellowBlue (handtrack.h:249-254): red = green = the heat-map, blue = the background image as grey
template <class T> Image<byte3> ImageOverlayYellowBlue(const Image<unsigned char> &image_rg, const Image<T> &image_b)
{
	Image<byte3> o; o.cam = image_rg.cam; o.raster.resize(image_rg.raster.size());
	for (size_t i = 0; i < image_rg.raster.size(); i++) o.raster[i] = byte3(image_rg.raster[i], image_rg.raster[i], ToGrayScale(image_b.raster[i]));
	return o;
}
// VisualizeHMaps (handtrack.h:256-267): every heat-map blown up to the background's size, laid over it, doubled once more, the eight stacked (synthetic-tracker.cpp:208,221)
template <class T> Image<byte3> VisualizeHMaps(const std::vector<Image<unsigned char>> &hmaps, Image<T> &dmap_d)
{
	std::vector<Image<byte3>> vmaps;
	for (auto hmap : hmaps)
	{
		while ((long)hmap.dim().x * hmap.dim().y < (long)dmap_d.dim().x * dmap_d.dim().y) hmap = UpSample(hmap);
		vmaps.push_back(UpSample(ImageOverlayYellowBlue(hmap, dmap_d)));
	}
	return ImageConcat(vmaps);
}
// DepthMesh (misc_image.h:419-450; synthetic-tracker.cpp:191): a triangle mesh over the in-range pixels, one vertex per skip x skip cell (the first in-range pixel of the
// cell, scanned towards cells that already have a vertex), two triangles per 2x2 block of vertices whose depth steps stay under gaplimit
template <class T> std::pair<std::vector<float3>, std::vector<int3>> DepthMesh(const Image<T> &dimage, float2 filter_range, float gaplimit = FLT_MAX, int skip = 1)
{
	std::vector<float3> verts; std::vector<int3> tris;
	const int W = dimage.dim().x, H = dimage.dim().y, w = W / skip, h = H / skip;
	std::vector<int> vmap((size_t)w * h, -1);
	const DCamera &c = dimage.cam;
	for (int py = 0; py < h; py++) for (int px = 0; px < w; px++)
	{
		const int rvx = (px && vmap[(size_t)py * w + px - 1] != -1) ? 1 : 0, rvy = (py && vmap[(size_t)(py - 1) * w + px] != -1) ? 1 : 0;
		bool placed = false;
		for (int sy = 0; sy < skip && !placed; sy++) for (int sx = 0; sx < skip && !placed; sx++)
		{
			const int x = px * skip + sx + rvx * ((skip - 1) - sx * 2), y = py * skip + sy + rvy * ((skip - 1) - sy * 2);
			const float d = dimage.raster[(size_t)y * W + x] * c.depth_scale;
			if (d >= filter_range.x && d < filter_range.y)
			{
				vmap[(size_t)py * w + px] = (int)verts.size();
				verts.push_back({ ((float)x - c.principal().x) / c.focal().x * d, ((float)y - c.principal().y) / c.focal().y * d, 1.0f * d });
				placed = true;
			}
		}
	}
	auto step = [&](int a, int b) { const float dz = verts[a].z - verts[b].z; return (dz < 0 ? -dz : dz) > gaplimit; };
	auto ok = [&](int a, int b, int cc) { return !(step(a, b) || step(b, cc) || step(cc, a)); };
	for (int py = 0; py + 1 < h; py++) for (int px = 0; px + 1 < w; px++)
	{
		const int a = vmap[(size_t)py * w + px], b = vmap[(size_t)(py + 1) * w + px], cc = vmap[(size_t)(py + 1) * w + px + 1], d = vmap[(size_t)py * w + px + 1];      // counter-clockwise
		if (a >= 0 && cc >= 0 && ((b >= 0 && ok(a, b, cc)) || (d >= 0 && ok(cc, d, a))))
		{
			if (b >= 0 && ok(a, b, cc)) tris.push_back({ a, b, cc });
			if (d >= 0 && ok(cc, d, a)) tris.push_back({ cc, d, a });
		}
		else if (b >= 0 && d >= 0)
		{
			if (a >= 0 && ok(d, a, b)) tris.push_back({ d, a, b });
			if (cc >= 0 && ok(b, cc, d)) tris.push_back({ b, cc, d });
		}
	}
	return { verts, tris };
}
inline float3 qrot_(const float4 &q, const float3 &v)                                       // linalg.h:288
{
	const float3 X{ q.w * q.w + q.x * q.x - q.y * q.y - q.z * q.z, (q.x * q.y + q.z * q.w) * 2, (q.z * q.x - q.y * q.w) * 2 };
	const float3 Y{ (q.x * q.y - q.z * q.w) * 2, q.w * q.w - q.x * q.x + q.y * q.y - q.z * q.z, (q.y * q.z + q.x * q.w) * 2 };
	const float3 Z{ (q.z * q.x + q.y * q.w) * 2, (q.y * q.z - q.x * q.w) * 2, q.w * q.w - q.x * q.x - q.y * q.y + q.z * q.z };
	return { (X.x * v.x + Y.x * v.y) + Z.x * v.z, (X.y * v.x + Y.y * v.y) + Z.y * v.z, (X.z * v.x + Y.z * v.y) + Z.z * v.z };
}
inline float3 operator*(const Pose &p, const float3 &v) { const float3 r = qrot_(p.orientation, v); return { p.position.x + r.x, p.position.y + r.y, p.position.z + r.z }; }      // geometric.h:119

namespace detail { inline ht_ctx *&live_ctx() { static ht_ctx *c = nullptr; return c; } }      // a context the free functions below can run on
inline void check(ht_ctx *ctx, int rc) { if (rc != HT_OK) throw std::runtime_error(std::string("ht_mi355x: ") + (ctx ? ht_last_error(ctx) : "no context")); }

// Model points in space and in the image (handtrack.h:76-96).  Additions to the reference's ModelFeaturePoint: `rel` says whose frame the offset is in (1, the default and
// the reference's only case: the body's centre-of-mass frame, the frame of GetPose; 0: its rig frame, the frame of GetPoseUser), see ht_mi355x.h "tracking accuracy".
// Skin and ImageFeaturePoints take one pose set as GetPose() returns it and run on the device of the first live HandTracker (ht_keypoints, the host form).
struct ModelFeaturePoint { int bone; float3 offset; int rel = 1; ModelFeaturePoint(int b = 0, float3 o = { 0, 0, 0 }, int r = 1) : bone(b), offset(o), rel(r) {} };
static const std::vector<ModelFeaturePoint> handmodelfeaturepoints =                             // handtrack.h:77-81
{
	{ 1, { 0, 0.0f, 0.0f } }, { 1, { -0.03f, 0, -0.03f } }, { 1, { 0.03f, 0, -0.03f } },
	{ 4, { 0, 0, 0 } }, { 7, { 0, 0, 0 } }, { 10, { 0, 0, 0 } }, { 13, { 0, 0, 0 } }, { 16, { 0, 0, 0 } },
};
namespace detail
{
// ht_keypoints (host form) for one set of centre-of-mass poses and a caller table; cam / depth may be null
inline void keypoints_on(ht_ctx *ctx, const std::vector<Pose> &pose, const std::vector<ModelFeaturePoint> &pts, bool left, const float *cam, const unsigned short *depth, int w, int h, float near_tol, float far_tol,
                         std::vector<float3> *xyz, std::vector<float2> *pix, std::vector<unsigned char> *vis)
{
	if (!ctx) throw std::runtime_error("Skin / ImageFeaturePoints need a live HandTracker (they run on its device)");
	const int K = (int)pts.size();
	std::vector<float> p7; for (auto &q : pose) { const float r[7] = { q.position.x, q.position.y, q.position.z, q.orientation.x, q.orientation.y, q.orientation.z, q.orientation.w }; p7.insert(p7.end(), r, r + 7); }
	int nb = 0; ht_model_info(ctx, &nb, nullptr, nullptr);
	if ((int)pose.size() != nb) throw std::runtime_error("Skin: one pose per body of the model");
	std::vector<int> bones(K), rel(K); std::vector<float> off((size_t)K * 3);
	for (int k = 0; k < K; k++) { bones[k] = pts[k].bone; rel[k] = pts[k].rel; off[3 * k] = pts[k].offset.x; off[3 * k + 1] = pts[k].offset.y; off[3 * k + 2] = pts[k].offset.z; }
	if (xyz) xyz->assign(K, float3{ 0, 0, 0 });
	if (pix) pix->assign(K, float2{ 0, 0 });
	if (vis) vis->assign(K, 0);
	const unsigned char hand = left ? 1 : 0;
	if (K) check(ctx, ht_keypoints(ctx, p7.data(), 1, HT_KP_COM_POSES, HT_KP_CALLER, K, bones.data(), off.data(), rel.data(), &hand, cam, depth, w, h, near_tol, far_tol,
	                               xyz ? &(*xyz)[0].x : nullptr, pix ? &(*pix)[0].x : nullptr, nullptr, vis ? vis->data() : nullptr));
}
}
inline std::vector<float3> Skin(const std::vector<Pose> &pose, const std::vector<ModelFeaturePoint> &pts)                                                     // handtrack.h:83-84
{
	std::vector<float3> x; detail::keypoints_on(detail::live_ctx(), pose, pts, false, nullptr, nullptr, 0, 0, 0.0f, 0.0f, &x, nullptr, nullptr); return x;
}
inline std::vector<float2> ImageFeaturePoints(const std::vector<Pose> &pose, const std::vector<ModelFeaturePoint> &modelfeaturepoints, const DCamera &hcam)      // handtrack.h:92-96
{
	const float cam[HT_CAM] = { hcam.focal().x, hcam.focal().y, hcam.principal().x, hcam.principal().y, hcam.depth_scale, hcam.pose.position.x, hcam.pose.position.y, hcam.pose.position.z,
	                            hcam.pose.orientation.x, hcam.pose.orientation.y, hcam.pose.orientation.z, hcam.pose.orientation.w };
	std::vector<float2> u; detail::keypoints_on(detail::live_ctx(), pose, modelfeaturepoints, false, cam, nullptr, 0, 0, 0.0f, 0.0f, nullptr, &u, nullptr); return u;
}

// Addition: the optimiser CNN::Step and CNN::TrainOpt apply: an ht_opt with ht_opt_default's values for its kind (HT_OPT_SGD, _MOMENTUM, _NESTEROV, _ADAM); set the fields on .opt
struct Optimizer
{
	ht_opt opt;
	explicit Optimizer(int kind = HT_OPT_SGD) { if (ht_opt_default(kind, &opt) != HT_OK) throw std::runtime_error("Optimizer: unknown kind"); }
};
class CNN;
CNN PoseInitializerCNN(std::string filename, int device);
class CNN                                                                                    // third_party/cnn.h:100-605 (Eval / Train / loadb / saveb)
{
	ht_ctx *ctx_ = nullptr;
	std::shared_ptr<ht_ctx> own_;      // set when the object owns its (CNN-only) context: PoseInitializerCNN
	friend struct HandTracker;
	friend struct TwoHandTracker;
	friend CNN PoseInitializerCNN(std::string, int);
public:
	std::vector<float> Eval(const std::vector<float> &x)                                     // cnn.h:550
	{
		if (x.size() != HT_CNN_IN) throw std::runtime_error("CNN::Eval expects 64*64 inputs");
		std::vector<float> y(HT_CNN_OUT);
		check(ctx_, ht_cnn_eval(ctx_, x.data(), y.data(), 1));
		return y;
	}
	void loadb(std::istream &s)                                                              // cnn.h:590
	{
		std::vector<float> w(HT_CNNB_COUNT);
		s.read((char *)w.data(), (std::streamsize)(w.size() * sizeof(float)));
		if ((size_t)s.gcount() != w.size() * sizeof(float)) throw std::runtime_error("CNN::loadb: short .cnnb stream");
		check(ctx_, ht_cnn_load_weights(ctx_, w.data(), w.size()));
	}
	// one SGD step; returns the mean squared error of the forward pass, as cnn.h:558 does
	float Train(const std::vector<float> &x, const std::vector<float> &expected, float alpha = 0.01f)
	{
		if (x.size() != HT_CNN_IN || expected.size() != HT_CNN_OUT) throw std::runtime_error("CNN::Train expects 64*64 inputs and 2304 labels");
		float mse = 0;
		check(ctx_, ht_cnn_train(ctx_, x.data(), expected.data(), 1, alpha, &mse));
		return mse;
	}
	// Addition: Train (cnn.h:558-580) for a pool on the device, d_inputs [n_pool][4096] and d_targets [n_pool][2304]: step k on sample order[k], in turn
	// (ht_cnn_train_dev; asynchronous on `stream`, the indices checked first).  d_mse [order.size()] (device, optional) takes what each step returns.
	void Train(const float *d_inputs, const float *d_targets, int n_pool, const std::vector<int> &order, float alpha = 0.01f, float *d_mse = nullptr, void *stream = nullptr)
	{
		check(ctx_, ht_cnn_train_dev(ctx_, d_inputs, d_targets, n_pool, order.data(), (int)order.size(), alpha, d_mse, stream));
	}
	// Addition: mini-batch steps on the same pools (ht_cnn_train_batch_dev): step k trains on samples order[k*batch .. (k+1)*batch), all at the step's
	// starting weights, w' = w - alpha * SUM_b g_b(w) -- a sum, not a mean (pass alpha / batch for the mean).  order.size() must be a multiple of batch.
	// d_mse [order.size()] (device, optional) takes every sample's loss.
	void TrainBatch(const float *d_inputs, const float *d_targets, int n_pool, const std::vector<int> &order, int batch, float alpha = 0.01f, float *d_mse = nullptr, void *stream = nullptr)
	{
		if (batch < 1 || order.size() % (size_t)batch) throw std::runtime_error("CNN::TrainBatch expects a positive batch that divides order.size()");
		check(ctx_, ht_cnn_train_batch_dev(ctx_, d_inputs, d_targets, n_pool, order.data(), (int)(order.size() / (size_t)batch), batch, alpha, d_mse, stream));
	}
	// Addition: the mini-batch gradient as a buffer and optimiser steps over it (ht_cnn_grad_batch_sized, ht_cnn_opt_step_sized_dev, ht_cnn_train_opt_sized_dev at
	// side 64; their contract is in ht_mi355x.h).  GradBatch: G = (accumulate ? G : 0) + SUM_b g_b(w) over up to HT_TRAIN_MAX_BATCH host samples x [n][4096],
	// expected [n][2304], the weights untouched; returns the samples' losses.  Step: one step of the optimiser over all weights from G.  TrainOpt: on device pools,
	// order.size() / (accum * batch) steps, each after `accum` gradient calls of `batch` samples -- exactly that sequence of the two calls.
	std::vector<float> GradBatch(const std::vector<float> &x, const std::vector<float> &expected, bool accumulate = false)
	{
		const size_t n = x.size() / HT_CNN_IN;
		if (!n || x.size() != n * HT_CNN_IN || expected.size() != n * HT_CNN_OUT) throw std::runtime_error("CNN::GradBatch expects n x 64*64 inputs and n x 2304 labels");
		std::vector<float> mse(n);
		check(ctx_, ht_cnn_grad_batch_sized(ctx_, 64, x.data(), expected.data(), (int)n, accumulate ? 1 : 0, mse.data()));
		return mse;
	}
	void Step(const Optimizer &o, void *stream = nullptr) { check(ctx_, ht_cnn_opt_step_sized_dev(ctx_, 64, &o.opt, stream)); }
	void TrainOpt(const float *d_inputs, const float *d_targets, int n_pool, const std::vector<int> &order, int batch, int accum, const Optimizer &o, float *d_mse = nullptr, void *stream = nullptr)
	{
		if (batch < 1 || accum < 1 || order.size() % ((size_t)batch * (size_t)accum)) throw std::runtime_error("CNN::TrainOpt expects positive batch and accum whose product divides order.size()");
		check(ctx_, ht_cnn_train_opt_sized_dev(ctx_, 64, d_inputs, d_targets, n_pool, order.data(), (int)(order.size() / ((size_t)batch * (size_t)accum)), batch, accum, &o.opt, d_mse, stream));
	}
	void saveb(std::ostream &s)                                                              // cnn.h:591
	{
		std::vector<float> w(HT_CNNB_COUNT);
		check(ctx_, ht_cnn_get_weights(ctx_, w.data(), w.size()));
		s.write((const char *)w.data(), (std::streamsize)(w.size() * sizeof(float)));
	}
	void saveb(std::string fname) { std::ofstream os(fname, std::ios_base::binary | std::ios_base::out); if (!os.is_open()) throw std::runtime_error("cannot open " + fname); saveb(os); }   // cnn.h:593
	void loadb(std::string fname) { std::ifstream is(fname, std::ios_base::binary | std::ios_base::in); if (!is.is_open()) throw std::runtime_error("cannot open " + fname); loadb(is); }   // cnn.h:592
};

struct ExpectedCNN;
struct HandTracker                                                                            // include/handtrack.h:513-846
{
	// tunables with the reference's names and defaults (handtrack.h:523-547); pushed to the device context before every update
	float segment_scale = 0.17f;
	float full_reset_on_error = 0.6f; bool angles_only = false; bool always_take_cnn = false; float drangey = 0.7f; int boundary_planes = 1;
	float microforce = 1.0f; float cloudforce_max_point = 15.0f; float cloudforce_max_sum = 3000.0f; int mainthreadpasses = 1; int subsample_fraction = 4;
	int subsample_voxel = 0; float subsample_size = 0.0f;                     // handtrack.h:535-536: voxel sub-sampling of the main-thread cloud
	size_t min_point_num = 400; float accum_error_threshold = 0.0f; float min_cray_prob = 0.0f;
	int steps = 5, steps_keypoints = 3, steps_keyangles = 2, steps_palmangle = 2, steps_cloudstart = 1, steps_unibody = 3;
	CNN cnn;
	// The reference's update() overlaps the CNN job with the caller's passes (std::async, handtrack.h:755-768) and is therefore timing dependent; the default here is the
	// deterministic synchronous sum (what every parity statement is made on).  overlapped_update = true gives the reference's structure: the job of frame k runs
	// on a second device context beside the caller's passes and is collected by a later call, when it is through (the 1 ms wait_for = one poll); the caller's latency is
	// the passes alone.  overlapped_wait = true (tests) waits for the job before the passes: the same sequence of operations as the synchronous call.
	bool overlapped_update = false, overlapped_wait = false;
	// Addition (the reference tracks right hands only; its README lists left / right as open work): the hand in front of the camera is a LEFT hand.  update,
	// update_cnn_model, kickstart and SetPose, and handmodel / othermodel's GetPose, GetPoseUser, SetPose and GetMeshes then speak the left hand's space.  Inside, the
	// tracker stays a right hand's on the mirror image (include/ht_mi355x.h "left hands"): cnn_input, cnn_output, the heat maps and cnn_output_analysis stay CANONICAL,
	// they show the mirrored frame the net saw.  Set it before the first frame; changing it on a running tracker wants a new SetPose.
	bool left_hand = false;
	// PhysModel facade of the two tracked models (handtrack.h:517-518): the members the applications use on them (physmodel.h:295-303,345,433-435)
	struct TrackedModel
	{
		// (Addition: with HandTracker::left_hand set, GetPose, GetPoseUser, SetPose and GetMeshes speak the left hand's space -- the mirror image of the slot's canonical
		// state, which stays a right hand's; the joint coordinates are those of the mirror image, the same numbers for both hands.)
		std::vector<Pose> GetPose() const { return left() ? mirrored(read(false)) : read(false); }                   // body poses (centre-of-mass frames)
		std::vector<Pose> GetPoseUser() const { return left() ? mirrored(read(true)) : read(true); }                 // rig space: RigidBody::PositionUser physics.h:142
		TrackedModel &SetPose(const std::vector<Pose> &poses) { return left() ? set(mirrored(poses)) : set(poses); } // poses only, momenta untouched (physmodel.h:435)
	private:
		TrackedModel &set(const std::vector<Pose> &poses)
		{
			std::vector<float> st((size_t)nb_ * HT_STATE);
			check(ctx_, ht_get_state(ctx_, which_, 0, 1, st.data()));
			for (size_t b = 0; b < poses.size() && (int)b < nb_; b++) { float *s = &st[b * HT_STATE]; s[0] = poses[b].position.x; s[1] = poses[b].position.y; s[2] = poses[b].position.z; s[3] = poses[b].orientation.x; s[4] = poses[b].orientation.y; s[5] = poses[b].orientation.z; s[6] = poses[b].orientation.w; }
			check(ctx_, ht_set_state(ctx_, which_, 0, 1, st.data()));
			return *this;
		}
	public:
		// physmodel.h:295-303: the subdivision meshes live in rig space (pose = PositionUser, orientation), the hull meshes in the centre-of-mass frames
		std::vector<Mesh> &GetMeshes(int show_subdiv = 0)
		{
			const std::vector<Pose> p = GetPose(), u = GetPoseUser();
			std::vector<Mesh> &sd = left() ? sdmeshes_left_ : sdmeshes_, &hull = left() ? meshes_left_ : meshes_;      // (addition: a left hand draws the mirrored meshes, ht_model_mirror)
			for (size_t b = 0; b < sd.size() && b < u.size(); b++) sd[b].pose = u[b];
			for (size_t b = 0; b < hull.size() && b < p.size(); b++) hull[b].pose = p[b];
			return show_subdiv ? sd : hull;
		}
		// void FitPointCloud(const std::vector<float3> &points, std::vector<LimitLinear> linears = {}, std::vector<LimitAngular> angulars = {}, float microforce = 1.0f)
		// (physmodel.h:345-356): one fit step of this model against a point cloud under the caller's rows, the cloud rows, the joint rows and the collision rows
		std::vector<RigidBody> rigidbodies;                                                                          // handles for the rows (physmodel.h:253)
		void FitPointCloud(const std::vector<float3> &points, std::vector<LimitLinear> linears = {}, std::vector<LimitAngular> angulars = {}, float microforce = 1.0f)
		{
			std::vector<float> l, a; detail::pack_rows(linears, angulars, l, a);
			const int n = (int)points.size(), nl = (int)linears.size(), na = (int)angulars.size();
			check(ctx_, ht_fit_rows(ctx_, which_, 1, n ? &points[0].x : nullptr, n, &n, l.data(), nl, &nl, a.data(), na, &na, microforce));
		}
		void FitPointCloud(const std::vector<float3> &points, float microforce) { FitPointCloud(points, {}, {}, microforce); }      // round-1 shorthand
		// Additions (the reference's PhysModel has no such members; its solver computes these on every pass and keeps them, physics.h:351-393): the model in its
		// joints' own coordinates c = (s.x, s.y, t.z) per joint (ht_joint_coords), the same as angles in the reference's degrees (2 asin(c) 180 / 3.14), how far every
		// joint's two anchors are apart (what FixPositions closes, physmodel.h:404-408), and the way back (ht_joint_pose: FixOrientations / FixPositions top down
		// from body 0, which stays where it is; momenta untouched).  SetJointCoords(GetJointCoords()) closes the joints and keeps the orientations.
		// (Addition) a built-in keypoint table of the model as scale() left it: HT_KP_FEATURE8 (handmodelfeaturepoints) or HT_KP_SKELETON (the wrist, every joint, every fingertip)
		std::vector<ModelFeaturePoint> GetKeypoints(int which = HT_KP_FEATURE8) const
		{
			int K = 0; check(ctx_, ht_keypoint_table(ctx_, which, &K, nullptr, nullptr, nullptr));
			std::vector<int> bones(K), rel(K); std::vector<float> off((size_t)K * 3);
			check(ctx_, ht_keypoint_table(ctx_, which, nullptr, bones.data(), off.data(), rel.data()));
			std::vector<ModelFeaturePoint> t;
			for (int k = 0; k < K; k++) t.push_back(ModelFeaturePoint(bones[k], float3{ off[3 * k], off[3 * k + 1], off[3 * k + 2] }, rel[k]));
			return t;
		}
		std::vector<float3> GetJointCoords() const { std::vector<float3> c; joints(&c, nullptr); return c; }
		std::vector<float> GetJointGaps() const { std::vector<float> g; joints(nullptr, &g); return g; }
		std::vector<float3> JointAngles() const
		{
			std::vector<float3> c = GetJointCoords();
			for (auto &a : c) a = { 2.0f * std::asin(a.x) * 180.0f / 3.14f, 2.0f * std::asin(a.y) * 180.0f / 3.14f, 2.0f * std::asin(a.z) * 180.0f / 3.14f };
			return c;
		}
		TrackedModel &SetJointCoords(const std::vector<float3> &coords)
		{
			int nj = 0; ht_model_info(ctx_, nullptr, &nj, nullptr);
			if ((int)coords.size() != nj) throw std::runtime_error("SetJointCoords expects one coordinate triple per joint");
			const std::vector<Pose> now = read(false);
			const float root[7] = { now[0].position.x, now[0].position.y, now[0].position.z, now[0].orientation.x, now[0].orientation.y, now[0].orientation.z, now[0].orientation.w };
			std::vector<float> p((size_t)nb_ * HT_POSE);
			check(ctx_, ht_joint_pose(ctx_, root, nj ? &coords[0].x : root, 1, HT_JOINTS_COM_POSES, p.data()));
			std::vector<Pose> poses(nb_);
			for (int b = 0; b < nb_; b++) { const float *s = &p[(size_t)b * HT_POSE]; poses[b].position = { s[0], s[1], s[2] }; poses[b].orientation = { s[3], s[4], s[5], s[6] }; }
			poses[0] = now[0];      // to the bit (the walk takes the root through the rig frame and back)
			return set(poses);
		}
	private:
		void joints(std::vector<float3> *c, std::vector<float> *g) const
		{
			int nj = 0; ht_model_info(ctx_, nullptr, &nj, nullptr);
			const std::vector<Pose> now = read(false);
			std::vector<float> p; for (auto &q : now) { const float r[7] = { q.position.x, q.position.y, q.position.z, q.orientation.x, q.orientation.y, q.orientation.z, q.orientation.w }; p.insert(p.end(), r, r + 7); }
			std::vector<float3> cc((size_t)nj); std::vector<float> gg((size_t)nj);
			if (nj) check(ctx_, ht_joint_coords(ctx_, p.data(), 1, HT_JOINTS_COM_POSES, &cc[0].x, gg.data()));
			if (c) *c = cc;
			if (g) *g = gg;
		}
		friend struct HandTracker;
		ht_ctx *ctx_ = nullptr; int which_ = 0, nb_ = 0; std::vector<float3> com_; std::vector<Mesh> meshes_, sdmeshes_;
		const bool *left_ = nullptr; std::vector<Mesh> meshes_left_, sdmeshes_left_;      // (addition) HandTracker::left_hand, and the meshes of the mirrored model
		bool left() const { return left_ && *left_; }
		std::vector<Pose> read(bool user) const
		{
			std::vector<float> st((size_t)nb_ * HT_STATE);
			check(ctx_, ht_get_state(ctx_, which_, 0, 1, st.data()));
			std::vector<Pose> out(nb_);
			for (int b = 0; b < nb_; b++)
			{
				const float *s = &st[(size_t)b * HT_STATE];
				out[b].position = { s[0], s[1], s[2] }; out[b].orientation = { s[3], s[4], s[5], s[6] };
				if (user && (size_t)b < com_.size()) out[b].position = out[b] * float3{ -com_[b].x, -com_[b].y, -com_[b].z };
			}
			return out;
		}
	} handmodel, othermodel;
	Image<float> cnn_input; std::vector<float> cnn_output;
	// the parts of CNNOutputAnalysis that synthetic-tracker.cpp draws (handtrack.h:186,188; synthetic-tracker.cpp:221-222)
	struct { std::vector<Image<unsigned char>> hmaps; Image<float> vmap; } cnn_output_analysis;

	// Defaults are the reference's hard-coded asset paths (handtrack.h:349,831): the model JSON is built on the host at
	// construction like PhysModel + LoadHandModel do; a model baked with ht_model_bake is accepted too.  Like the reference
	// (handtrack.h:123-126) a missing weight file is not an error at construction, but update() then fails loudly instead
	// of running on random weights.
	explicit HandTracker(const std::string &model_path = "../assets/model_hand.json", const std::string &cnnb_path = "../assets/handposedd.cnnb", int device = 0)
	{
		int rc = ht_create(model_path.c_str(), 1, device, &ctx_);
		if (rc != HT_OK) { std::string msg = ctx_ ? ht_last_error(ctx_) : "ht_create failed"; if (ctx_) ht_destroy(ctx_); ctx_ = nullptr; throw std::runtime_error("HandTracker: " + msg); }
		model_path_ = model_path; device_ = device;
		cnn.ctx_ = ctx_;
		if (!detail::live_ctx()) detail::live_ctx() = ctx_;
		ht_model_info(ctx_, &nb_, nullptr, nullptr);
		{
			// geometry for the facades (GetPoseUser needs the centres of mass, GetMeshes the hulls): the same host build, no device involved
			ht_model *m = nullptr;
			if (ht_model_open(model_path.c_str(), 1, &m) == HT_OK)
				for (int b = 0; b < nb_; b++)
				{
					float com[3] = { 0, 0, 0 };
					ht_model_body(m, b, nullptr, nullptr, nullptr, com, nullptr);
					handmodel.com_.push_back({ com[0], com[1], com[2] }); handmodel.meshes_.push_back(detail::hull_mesh(m, b)); handmodel.sdmeshes_.push_back(detail::subdivision_mesh(m, b));
				}
			if (m && !handmodel.meshes_.empty() && ht_model_mirror(m) == HT_OK)      // (addition) the left hand's meshes: the same model mirrored
				for (int b = 0; b < nb_; b++) { handmodel.meshes_left_.push_back(detail::hull_mesh(m, b)); handmodel.sdmeshes_left_.push_back(detail::subdivision_mesh(m, b)); }
			if (m) ht_model_close(m);
			othermodel.com_ = handmodel.com_; othermodel.meshes_ = handmodel.meshes_; othermodel.sdmeshes_ = handmodel.sdmeshes_;
			othermodel.meshes_left_ = handmodel.meshes_left_; othermodel.sdmeshes_left_ = handmodel.sdmeshes_left_; handmodel.left_ = othermodel.left_ = &left_hand;
			handmodel.ctx_ = othermodel.ctx_ = ctx_; handmodel.nb_ = othermodel.nb_ = nb_; handmodel.which_ = 0; othermodel.which_ = 1;
			for (int b = 0; b < nb_; b++) { handmodel.rigidbodies.push_back(RigidBody{ ctx_, 0, b }); othermodel.rigidbodies.push_back(RigidBody{ ctx_, 1, b }); }
		}
		if (!cnnb_path.empty()) { std::ifstream is(cnnb_path, std::ios_base::in | std::ios_base::binary); if (is.is_open()) cnn.loadb(is); }
		cnn_output.assign(HT_CNN_OUT, 0.01f);
	}
	~HandTracker() { if (job_) { ht_job_wait(job_); ht_destroy(job_); } if (detail::live_ctx() == ctx_) detail::live_ctx() = nullptr; if (ctx_) ht_destroy(ctx_); }      // the reference's destructor joins the job too (handtrack.h:841-844)
	HandTracker(const HandTracker &) = delete; HandTracker &operator=(const HandTracker &) = delete;

	void load_config(const std::string &jsonfile)                                            // handtrack.h:822-828
	{
		ht_params p; pull_params(p);
		float pfe = 0.0f; float seg = segment_scale; int ini = 0;
		check(ctx_, ht_get_tracker_flags(ctx_, 0, 1, &pfe, &ini));
		const float pfe0 = pfe;
		const int rc = ht_config_read(jsonfile.c_str(), &p, &seg, &pfe);
		if (rc != HT_OK) throw std::runtime_error("json parse error - " + jsonfile);
		segment_scale = seg;
		full_reset_on_error = p.full_reset_on_error; angles_only = p.angles_only != 0; always_take_cnn = p.always_take_cnn != 0; drangey = p.drangey; boundary_planes = p.boundary_planes;
		microforce = p.microforce; cloudforce_max_point = p.cloudforce_max_point; cloudforce_max_sum = p.cloudforce_max_sum; mainthreadpasses = p.mainthreadpasses;
		subsample_fraction = p.subsample_fraction; min_point_num = p.min_point_num; accum_error_threshold = p.accum_error_threshold; min_cray_prob = p.min_cray_prob;
		subsample_voxel = p.subsample_voxel; subsample_size = p.subsample_size;
		steps = p.steps; steps_keypoints = p.steps_keypoints; steps_keyangles = p.steps_keyangles; steps_palmangle = p.steps_palmangle; steps_cloudstart = p.steps_cloudstart; steps_unibody = p.steps_unibody;
		check(ctx_, ht_set_params(ctx_, &p));      // also carries physics_iterations(_post), physics_use_collision, physics_weak_force, bone_sum_error_scale, unibody_force
		if (pfe != pfe0) check(ctx_, ht_set_tracker_flags(ctx_, 0, 1, &pfe, &ini));
	}
	void SetPose(const std::vector<Pose> &pose) { check(ctx_, ht_tracker_reset(ctx_, 0, 1, flat(left_hand ? mirrored(pose) : pose).data())); }          // handmodel/othermodel.SetPose

	std::vector<Pose> update(Image<unsigned short> dimage)                                   // handtrack.h:748
	{
		// A frame that is not 64x64 goes through ht_update_frames_sync, which does what update() does with it (handtrack.h:693-785): the CNN
		// sees HandSegmentVR(dimage, 0xF, {0.1, drangey}, segment_scale), the cloud and FitError come from the full frame.  The segment is
		// fetched once more below, only for the visualisation members (cnn_input and the heat-map camera).
		push_params();
		const bool full = dimage.dim().x != 64 || dimage.dim().y != 64;
		std::vector<float> out((size_t)nb_ * HT_POSE);
		// Addition: a left hand.  The synchronous call hands the frame over with one flag (ht_update_hands_sync mirrors on the device); everything else below -- the
		// overlapped arrangement, the segment for the visualisation members -- takes the canonical frame, mirrored here with the host calls, and the poses are mirrored after.
		const Image<unsigned short> given = (left_hand && !overlapped_update) ? dimage : Image<unsigned short>();
		if (left_hand) dimage = mirror_image(dimage);
		const DCamera &fc = dimage.cam;
		const float fcam[HT_CAM] = { fc.focal().x, fc.focal().y, fc.principal().x, fc.principal().y, fc.depth_scale, fc.pose.position.x, fc.pose.position.y, fc.pose.position.z,
		                             fc.pose.orientation.x, fc.pose.orientation.y, fc.pose.orientation.z, fc.pose.orientation.w };
		if (overlapped_update)
		{
			// handtrack.h:755-768 on two device contexts (include/ht_mi355x.h: ht_job_start / ht_job_poll / ht_job_collect / ht_update_passes_sync)
			ensure_job_context();
			if (!job_in_flight_)
			{
				check(job_, ht_job_start(job_, ctx_, dimage.raster.data(), fcam, dimage.dim().x, dimage.dim().y, segment_scale, 1));
				job_in_flight_ = true; job_image_ = dimage;
			}
			int ready = 0;
			if (overlapped_wait) { check(job_, ht_job_wait(job_)); ready = 1; } else check(job_, ht_job_poll(job_, &ready));
			if (ready)
			{
				check(job_, ht_job_collect(job_, ctx_, 1, nullptr));
				check(job_, ht_get_cnn_results(job_, 0, 1, nullptr, cnn_output.data(), nullptr));
				Image<unsigned short> seen = (job_image_.dim().x != 64 || job_image_.dim().y != 64) ? segment(job_image_, 0xF, { 0.1f, drangey }, segment_scale) : job_image_;
				fill_visualisation(seen);      // cnn_input / cnn_output / the heat-maps of the frame the job saw
				job_in_flight_ = false;
			}
			check(ctx_, ht_update_passes_sync(ctx_, dimage.raster.data(), fcam, dimage.dim().x, dimage.dim().y, 1, out.data()));
			if (left_hand) check(ctx_, ht_mirror_poses(ctx_, out.data(), nb_, 1, nullptr, out.data()));
		}
		else if (left_hand)
		{
			const uint8_t left = 1; float gcam[HT_CAM]; cam12(given.cam, gcam);
			check(ctx_, ht_update_hands_sync(ctx_, 64, given.raster.data(), gcam, given.dim().x, given.dim().y, segment_scale, &left, 1, out.data(), cnn_output.data()));
			if (full) dimage = segment(dimage, 0xF, { 0.1f, drangey }, segment_scale);
			fill_visualisation(dimage);      // canonical: the mirrored frame's segment, as the net saw it
		}
		else
		{
			check(ctx_, ht_update_frames_sync(ctx_, dimage.raster.data(), fcam, dimage.dim().x, dimage.dim().y, segment_scale, 1, out.data(), cnn_output.data()));
			if (full) dimage = segment(dimage, 0xF, { 0.1f, drangey }, segment_scale);
			fill_visualisation(dimage);
		}
		std::vector<Pose> pose(nb_);
		for (int b = 0; b < nb_; b++) { const float *p = &out[(size_t)b * HT_POSE]; pose[b].position = { p[0], p[1], p[2] }; pose[b].orientation = { p[3], p[4], p[5], p[6] }; }
		return pose;
	}
	// slowfit (handtrack.h:786-821); the selected bone is given by index (-1: none) instead of a RigidBody pointer
	void slowfit(const std::vector<float3> &points, int hold, const std::vector<Pose> &refpose, int steps_ = 6, int selectrb = -1, float3 spoint = { 0, 0, 0 }, float3 rbpoint = { 0, 0, 0 },
	             const std::vector<float4> &crays = std::vector<float4>())
	{
		push_params();
		const int n = (int)points.size();
		check(ctx_, ht_set_points(ctx_, 1, n ? &points[0].x : &spoint.x, n > 0 ? n : 1, &n));
		std::vector<float> ref = flat(refpose), cr(32, 0.0f);
		const int ncray = crays.size() < 8 ? (int)crays.size() : 8;
		for (int i = 0; i < ncray; i++) { cr[4 * i] = crays[i].x; cr[4 * i + 1] = crays[i].y; cr[4 * i + 2] = crays[i].z; cr[4 * i + 3] = crays[i].w; }
		check(ctx_, ht_slowfit(ctx_, 1, refpose.empty() ? 0 : hold, refpose.empty() ? nullptr : ref.data(), steps_, selectrb, &spoint.x, &rbpoint.x, ncray ? cr.data() : nullptr, ncray));
	}
	float scale(float s) { check(ctx_, ht_scale(ctx_, s)); segment_scale *= s; return segment_scale; }                     // handtrack.h:591
	// update_cnn_model (handtrack.h:734-741): the CNN job alone, synchronously -- othermodel is not re-seeded from handmodel, no main-thread pass;
	// returns othermodel.GetPose() when the tracker would take it over (:720-722) and an empty vector otherwise
	std::vector<Pose> update_cnn_model(Image<unsigned short> dimage) { return cnn_job(std::move(dimage), false); }
	// kickstart (handtrack.h:743-746): handmodel.SetPose(update_cnn_model(dimage))
	void kickstart(Image<unsigned short> dimage) { cnn_job(std::move(dimage), true); }
	// HandSegmentVR (handtrack.h:280-344) on this tracker's device
	Image<unsigned short> segment(const Image<unsigned short> &depth, int entry_options = 0xF, float2 wrange = { 0.1f, 0.65f }, float diam = 0.17f) const { return segment_on(ctx_, depth, entry_options, wrange, diam); }
	static Image<unsigned short> segment_on(ht_ctx *ctx, const Image<unsigned short> &depth, int entry_options, float2 wrange, float diam)
	{
		const DCamera &c = depth.cam;
		float cam[HT_CAM] = { c.focal().x, c.focal().y, c.principal().x, c.principal().y, c.depth_scale, c.pose.position.x, c.pose.position.y, c.pose.position.z,
		                      c.pose.orientation.x, c.pose.orientation.y, c.pose.orientation.z, c.pose.orientation.w };
		float co[HT_CAM]; std::vector<unsigned short> tile(4096);
		check(ctx, ht_segment_vr(ctx, depth.raster.data(), cam, depth.dim().x, depth.dim().y, 1, entry_options, wrange.x, wrange.y, diam, tile.data(), co));
		Pose pose; pose.position = { co[5], co[6], co[7] }; pose.orientation = { co[8], co[9], co[10], co[11] };
		return Image<unsigned short>(DCamera({ 64, 64 }, { co[0], co[1] }, { co[2], co[3] }, co[4], pose), std::move(tile));
	}
	// Addition, not a reference name: the application's FakeDepth (synthetic-tracker.cpp:69-76, the software_rasterizer branch of :182) on this tracker's
	// device, for a batch of hands at centre-of-mass poses (PhysModel::SetPose) seen through `cam` (its pose is not used: the rays start at the origin)
	std::vector<Image<unsigned short>> render_depth(const std::vector<std::vector<Pose>> &poses, const DCamera &cam, float far = 4.0f) const
	{
		const int B = (int)poses.size(), w = cam.dim().x, h = cam.dim().y;
		std::vector<float> p7; p7.reserve((size_t)B * nb_ * HT_POSE);
		for (auto &fr : poses) { if ((int)fr.size() != nb_) throw std::runtime_error("render_depth: one pose per body"); const std::vector<float> f = flat(fr); p7.insert(p7.end(), f.begin(), f.end()); }
		const float c[HT_CAM] = { cam.focal().x, cam.focal().y, cam.principal().x, cam.principal().y, cam.depth_scale, cam.pose.position.x, cam.pose.position.y, cam.pose.position.z,
		                          cam.pose.orientation.x, cam.pose.orientation.y, cam.pose.orientation.z, cam.pose.orientation.w };
		std::vector<float> cams; for (int b = 0; b < B; b++) cams.insert(cams.end(), c, c + HT_CAM);
		std::vector<unsigned short> d((size_t)B * w * h);
		check(ctx_, ht_render_depth(ctx_, p7.data(), cams.data(), w, h, far, B, d.data(), nullptr));
		std::vector<Image<unsigned short>> out;
		for (int b = 0; b < B; b++) out.emplace_back(cam, std::vector<unsigned short>(d.begin() + (size_t)b * w * h, d.begin() + (size_t)(b + 1) * w * h));
		return out;
	}
	Image<unsigned short> render_depth(const std::vector<Pose> &poses, const DCamera &cam, float far = 4.0f) const { return render_depth(std::vector<std::vector<Pose>>{ poses }, cam, far)[0]; }
	// Addition, not a reference name: the hand's subdivision surface (GetMeshes(true), what the application draws with OpenGL, synthetic-tracker.cpp:164-182) through the
	// device's z-buffer rasteriser (ht_raster_mesh_depth), shaped like render_depth.  pixel_offset 0 / far 4 gives frames interchangeable with render_depth's, 0.5 / 0.85
	// the application's GL convention
	std::vector<Image<unsigned short>> render_mesh_raster(const std::vector<std::vector<Pose>> &poses, const DCamera &cam, float far = 4.0f, float pixel_offset = 0.0f) const
	{
		const int B = (int)poses.size(), w = cam.dim().x, h = cam.dim().y;
		std::vector<float> p7; p7.reserve((size_t)B * nb_ * HT_POSE);
		for (auto &fr : poses) { if ((int)fr.size() != nb_) throw std::runtime_error("render_mesh_raster: one pose per body"); const std::vector<float> f = flat(fr); p7.insert(p7.end(), f.begin(), f.end()); }
		const float c[HT_CAM] = { cam.focal().x, cam.focal().y, cam.principal().x, cam.principal().y, cam.depth_scale, cam.pose.position.x, cam.pose.position.y, cam.pose.position.z,
		                          cam.pose.orientation.x, cam.pose.orientation.y, cam.pose.orientation.z, cam.pose.orientation.w };
		std::vector<float> cams; for (int b = 0; b < B; b++) cams.insert(cams.end(), c, c + HT_CAM);
		std::vector<unsigned short> d((size_t)B * w * h);
		check(ctx_, ht_raster_mesh_depth(ctx_, p7.data(), cams.data(), w, h, far, pixel_offset, B, d.data(), nullptr));
		std::vector<Image<unsigned short>> out;
		for (int b = 0; b < B; b++) out.emplace_back(cam, std::vector<unsigned short>(d.begin() + (size_t)b * w * h, d.begin() + (size_t)(b + 1) * w * h));
		return out;
	}
	Image<unsigned short> render_mesh_raster(const std::vector<Pose> &poses, const DCamera &cam, float far = 4.0f, float pixel_offset = 0.0f) const
	{ return render_mesh_raster(std::vector<std::vector<Pose>>{ poses }, cam, far, pixel_offset)[0]; }
	// Addition, not a reference name: one frame of up to HT_SCENE_MAX_HANDS hands, each right or left, in one z-buffer pass over an optional background frame
	// (ht_raster_scene_depth).  hands: (centre-of-mass poses, left?) per instance, a left hand's poses as the camera sees them (what GetPose returns with left_hand
	// set).  background: an image of cam's dimensions, or one without a raster for none.  hand and body are -1 where no hand is written.
	struct Scene { Image<unsigned short> depth; std::vector<signed char> hand, body; std::vector<int> visible; };
	Scene render_scene(const std::vector<std::pair<std::vector<Pose>, bool>> &hands, const DCamera &cam, float far = 4.0f, float pixel_offset = 0.0f,
	                   const Image<unsigned short> &background = Image<unsigned short>()) const
	{
		const int H = (int)hands.size(), w = cam.dim().x, h = cam.dim().y;
		const size_t n = (size_t)w * h;
		if (!background.raster.empty() && background.raster.size() != n) throw std::runtime_error("render_scene: the background does not match the camera's dimensions");
		std::vector<float> p7; p7.reserve((size_t)H * nb_ * HT_POSE);
		std::vector<uint8_t> flags;
		for (auto &hd : hands)
		{
			if ((int)hd.first.size() != nb_) throw std::runtime_error("render_scene: one pose per body");
			const std::vector<float> f = flat(hd.first); p7.insert(p7.end(), f.begin(), f.end());
			flags.push_back(hd.second ? 1 : HT_SCENE_RIGHT);
		}
		float c[HT_CAM]; cam12(cam, c);
		Scene s; s.depth = Image<unsigned short>(cam); s.hand.resize(n); s.body.resize(n); s.visible.assign((size_t)(H > 0 ? H : 0), 0);
		check(ctx_, ht_raster_scene_depth(ctx_, p7.data(), flags.data(), H, c, w, h, far, pixel_offset, 1, background.raster.empty() ? nullptr : background.raster.data(), s.depth.raster.data(),
		                                  (int8_t *)s.hand.data(), (int8_t *)s.body.data(), (int32_t *)s.visible.data()));
		return s;
	}
	// Additions, not reference names (ht_mi355x.h "tracking accuracy").  keypoints: where the hand of the latest update is in `image` -- the points of a built-in table in
	// the poses' frame, in pixels of image.cam, and their visibility against the frame (0 visible, 1 occluded, 2 nothing there, 3 outside the image, 4 behind the camera;
	// the tolerances in metres).  What the reference's overlay computes per point (handtrack.h:632-634).  With left_hand set the points are the left hand's.
	struct Keypoints { std::vector<float3> xyz; std::vector<float2> pixels; std::vector<unsigned char> visibility; };
	Keypoints keypoints(const Image<unsigned short> &image, int which = HT_KP_FEATURE8, float near_tol = 0.03f, float far_tol = 0.02f) const
	{
		if (image.raster.size() != (size_t)image.dim().x * image.dim().y) throw std::runtime_error("HandTracker: the raster does not match the camera's dimensions");
		float cam[HT_CAM]; cam12(image.cam, cam);
		Keypoints k;
		detail::keypoints_on(ctx_, handmodel.GetPose(), handmodel.GetKeypoints(which), left_hand, cam, image.raster.data(), image.dim().x, image.dim().y, near_tol, far_tol, &k.xyz, &k.pixels, &k.visibility);
		return k;
	}
	// depth_residual: how well the posed model explains `image` -- the hull model of the latest update rendered through image.cam (ht_render_depth) and compared with the
	// frame over the pixels inside wrange (metres, half open as HandSegmentVR's): pixel counts, silhouette overlap, and the depth residual over the overlap in metres.
	// A left hand is compared in the mirrored frame, where its slot's state lives.
	struct DepthResidual { long long n_observed, n_rendered, n_both, n_close; double iou, mean_abs, rms, max_abs; };
	DepthResidual depth_residual(const Image<unsigned short> &image, float2 wrange = { 0.1f, 0.65f }, float close_tol = 0.01f) const
	{
		const Image<unsigned short> im = left_hand ? mirror_image(image) : image;
		const int w = im.dim().x, h = im.dim().y;
		if (im.raster.size() != (size_t)w * h) throw std::runtime_error("HandTracker: the raster does not match the camera's dimensions");
		float cam[HT_CAM]; cam12(im.cam, cam);
		const float ds = im.cam.depth_scale;
		const std::vector<float> p7 = flat(handmodel.read(false));
		long long info[8];
		check(ctx_, ht_pose_depth_residual(ctx_, p7.data(), cam, im.raster.data(), w, h, 1, HT_KP_COM_POSES, 4.0f, (int)(wrange.x / ds), (int)(wrange.y / ds), (int)(close_tol / ds), (int64_t *)info, nullptr));
		DepthResidual r = { info[0], info[1], info[2], info[3], 0.0, 0.0, 0.0, (double)info[6] * ds };
		const long long uni = info[0] + info[1] - info[2];
		r.iou = uni ? (double)info[2] / (double)uni : 0.0;
		if (info[2]) { r.mean_abs = (double)info[4] / (double)info[2] * ds; r.rms = std::sqrt((double)info[5] / (double)info[2]) * ds; }
		return r;
	}
	// Addition, not a reference name (ht_mi355x.h "keypoint fit"): handmodel goes from its current pose to keypoint targets -- 3-D points (kind 0, three nailed rows a
	// keypoint, physics.h:342-346) and pixels of targets.cam (kind 1, a dead-zone pair on each axis across the pixel's ray, physics.h:332-340) -- in options.steps solver
	// steps that stay on the device.  table: handmodel.GetKeypoints(...) or the caller's own points; targets.kind empty: all points; targets.weights empty: all 1; a weight
	// of 0 or a NaN target: not annotated.  Returns the user poses as update() does and every keypoint's residual before and after (-1: absent).  With left_hand set the
	// point targets and the poses are the left hand's (mirrored on the way in and out); pixel targets of a left hand are refused: mirror the frame first.
	struct KeypointFit : ht_kpfit { KeypointFit() { ht_kpfit_default(this); } };      // steps 6, max_force FLT_MAX, ray_radius 0.01, ray_force 100000, flags 0 (HT_KPFIT_KEEP_MOMENTA)
	struct KeypointTargets { std::vector<float3> xyz; std::vector<float2> pixels; std::vector<int> kind; std::vector<float> weights; DCamera cam; };
	struct KeypointFitResult { std::vector<Pose> pose; std::vector<float> before, after; };
	KeypointFitResult fit_keypoints(const std::vector<ModelFeaturePoint> &table, const KeypointTargets &targets, const KeypointFit &options = KeypointFit())
	{
		const int K = (int)table.size();
		std::vector<int> bones(K), rel(K); std::vector<float> off((size_t)K * 3);
		for (int k = 0; k < K; k++) { bones[k] = table[k].bone; rel[k] = table[k].rel; off[3 * k] = table[k].offset.x; off[3 * k + 1] = table[k].offset.y; off[3 * k + 2] = table[k].offset.z; }
		bool rays = false; for (int k : targets.kind) rays = rays || k != 0;
		if ((!targets.kind.empty() && (int)targets.kind.size() != K) || (!targets.weights.empty() && (int)targets.weights.size() != K) || (!targets.xyz.empty() && (int)targets.xyz.size() != K) ||
		    (!targets.pixels.empty() && (int)targets.pixels.size() != K))
			throw std::runtime_error("fit_keypoints: one target, kind and weight per table entry");
		if (rays && left_hand) throw std::runtime_error("fit_keypoints: pixel targets of a left hand: mirror the frame and its pixels first");
		std::vector<float3> xyz = targets.xyz;
		if (left_hand) for (auto &p : xyz) p.x = -p.x;
		float cam[HT_CAM]; cam12(targets.cam, cam);
		std::vector<float> poses((size_t)nb_ * HT_POSE), resid((size_t)2 * (K > 0 ? K : 1));
		check(ctx_, ht_fit_keypoints(ctx_, 0, 1, HT_KP_CALLER, K, bones.data(), off.data(), rel.data(), targets.kind.empty() ? nullptr : targets.kind.data(), xyz.empty() ? nullptr : &xyz[0].x,
		                             targets.pixels.empty() ? nullptr : &targets.pixels[0].x, targets.weights.empty() ? nullptr : targets.weights.data(), rays ? cam : nullptr, &options, poses.data(), resid.data()));
		KeypointFitResult r;
		r.pose.resize(nb_);
		for (int b = 0; b < nb_; b++) { const float *p = &poses[(size_t)b * HT_POSE]; r.pose[b].position = { p[0], p[1], p[2] }; r.pose[b].orientation = { p[3], p[4], p[5], p[6] }; }
		if (left_hand) r.pose = mirrored(r.pose);
		r.before.assign(resid.begin(), resid.begin() + K); r.after.assign(resid.begin() + K, resid.begin() + 2 * K);
		return r;
	}
	// Additions, not reference names (ht_mi355x.h "several views").  The reference keeps the pieces -- PlaneSplit, Mirror, MirrorPlaneSplit "to get some view of the back of
	// an object" (misc_image.h:401-485), a mirror plane in every data set header (dataset.h:24,45) -- and tracks from one camera.  views: up to HT_VIEWS_MAX frames of one
	// size whose cameras' poses are expressed in one tracking space; mirrors: a plane per view in that view's camera space, empty or (0,0,0,FLT_MAX) for none.
	// FuseViews: the views' clouds as one, every point with the ray source that saw it (2 v: view v directly, 2 v + 1: through its mirror) and the sources' origins; the
	// cloud stays on the device for the fit.  update_views: update() on views[0] (whose camera pose must be identity: the reference's PointCloud is camera-local,
	// handtrack.h:703), then `passes` fits of handmodel against the fused cloud, each point's ray from its own source's origin (CloudConstraint, physmodel.h:164-174).
	// Right hands only: mirror the inputs first.
	struct ViewOptions : ht_views { explicit ViewOptions(const HandTracker &t) { ht_views_default(t.ctx_, this); } };      // range {0.1, drangey}, fraction = subsample_fraction, mirror_eps 0.02
	struct FusedCloud { std::vector<float3> points; std::vector<int> source, per_source; std::vector<float3> origins; bool cut; };
	FusedCloud FuseViews(const std::vector<Image<unsigned short>> &views, const std::vector<float4> &mirrors = std::vector<float4>(), const ht_views *options = nullptr)
	{
		push_params();
		view_arrays a = pack_views(views, mirrors);
		const ViewOptions dflt(*this);
		const ht_views &o = options ? *options : dflt;
		const int cap = a.V * ((a.w * a.h + (o.fraction > 0 ? o.fraction : 1) - 1) / (o.fraction > 0 ? o.fraction : 1));
		std::vector<float> pts((size_t)(cap > 0 ? cap : 1) * 4), org((size_t)a.V * 6);
		int n = 0, cut = 0;
		FusedCloud f; f.per_source.assign((size_t)2 * a.V, 0);
		check(ctx_, ht_fuse_views(ctx_, a.depth.data(), a.cams.data(), a.planes.empty() ? nullptr : a.planes.data(), a.w, a.h, a.V, 1, &o, pts.data(), cap > 0 ? cap : 1, &n, f.per_source.data(), org.data(), &cut));
		for (int i = 0; i < n; i++) { f.points.push_back({ pts[4 * (size_t)i], pts[4 * (size_t)i + 1], pts[4 * (size_t)i + 2] }); f.source.push_back((int)pts[4 * (size_t)i + 3]); }
		for (int s = 0; s < 2 * a.V; s++) f.origins.push_back({ org[3 * (size_t)s], org[3 * (size_t)s + 1], org[3 * (size_t)s + 2] });
		f.cut = cut != 0;
		return f;
	}
	std::vector<Pose> update_views(const std::vector<Image<unsigned short>> &views, const std::vector<float4> &mirrors = std::vector<float4>(), int passes = 3, const ht_views *options = nullptr)
	{
		if (left_hand) throw std::runtime_error("update_views: right hands only: mirror the frames, cameras and planes first");
		push_params();
		view_arrays a = pack_views(views, mirrors);
		std::vector<float> out((size_t)nb_ * HT_POSE);
		check(ctx_, ht_update_views_sync(ctx_, 64, a.depth.data(), a.cams.data(), a.planes.empty() ? nullptr : a.planes.data(), a.w, a.h, a.V, segment_scale, 1, options, passes, out.data(), cnn_output.data()));
		const bool full = a.w != 64 || a.h != 64;
		fill_visualisation(full ? segment(views[0], 0xF, { 0.1f, drangey }, segment_scale) : views[0]);      // what the net saw: view 0's segment
		std::vector<Pose> pose(nb_);
		for (int b = 0; b < nb_; b++) { const float *p = &out[(size_t)b * HT_POSE]; pose[b].position = { p[0], p[1], p[2] }; pose[b].orientation = { p[3], p[4], p[5], p[6] }; }
		return pose;
	}
	// Addition, not a reference name (ht_mi355x.h "a view's extrinsics"; the reference never calibrates anything).  CalibrateView: where another depth camera stands, from
	// the tracked hand alone.  frames: that camera's frames, one per tracked frame (one size; their cameras' intrinsics are read, their poses are not); poses: per frame the
	// tracked model's centre-of-mass poses in tracking space (handmodel.GetPose() after the update of that frame); guess: the camera's pose as far as it is known.
	// T maps the camera's space to tracking space (a point p of the view lies at T.position + qrot(T.orientation, p)): write it into that view's DCamera::pose for
	// update_views.  One T for the batch (HT_CALIB_RIG); the batch is not bounded by the tracker's one slot, as SplitHandsByModel's is not.  stats: the
	// (iterations + 1) records of HT_CALIB_STATS doubles the C call documents; degenerate: some record carries a flag (too few inliers, a pivot that is not positive).
	struct CalibOptions : ht_calib { explicit CalibOptions(const HandTracker &t) { ht_calib_default(t.ctx_, this); } };
	struct ViewCalibration { Pose T; std::vector<double> stats; bool degenerate; };
	ViewCalibration CalibrateView(const std::vector<Image<unsigned short>> &frames, const std::vector<std::vector<Pose>> &poses, const Pose &guess, const ht_calib *options = nullptr)
	{
		const int B = (int)frames.size();
		if (B < 1 || poses.size() != frames.size()) throw std::runtime_error("CalibrateView: one set of poses per frame, at least one frame");
		const CalibOptions dflt(*this);
		ht_calib o = options ? *options : dflt;
		if (o.mode != HT_CALIB_RIG) throw std::runtime_error("CalibrateView: one transform for the batch (HT_CALIB_RIG); the per-slot mode is the C call's");
		const int w = frames[0].dim().x, h = frames[0].dim().y;
		std::vector<unsigned short> depth; std::vector<float> cams((size_t)B * HT_CAM), p7;
		for (int b = 0; b < B; b++)
		{
			if (frames[b].dim().x != w || frames[b].dim().y != h || frames[b].raster.size() != (size_t)w * h) throw std::runtime_error("CalibrateView: the frames of a call have one size");
			if ((int)poses[b].size() != nb_) throw std::runtime_error("CalibrateView: one pose per body of the tracker's model for every frame");
			depth.insert(depth.end(), frames[b].raster.begin(), frames[b].raster.end());
			DCamera c = frames[b].cam; c.pose = guess;
			cam12(c, &cams[(size_t)b * HT_CAM]);
			const std::vector<float> f = flat(poses[b]);
			p7.insert(p7.end(), f.begin(), f.end());
		}
		ViewCalibration r;
		r.stats.assign((size_t)(o.iterations > 0 ? o.iterations + 1 : 1) * HT_CALIB_STATS, 0.0);
		float T[7];
		check(ctx_, ht_calibrate_view(ctx_, 0, p7.data(), depth.data(), cams.data(), w, h, B, &o, T, r.stats.data()));
		r.T.position = { T[0], T[1], T[2] }; r.T.orientation = { T[3], T[4], T[5], T[6] };
		r.degenerate = false;
		for (size_t i = 5; i < r.stats.size(); i += HT_CALIB_STATS) r.degenerate = r.degenerate || r.stats[i] != 0.0;
		return r;
	}
	// Addition, not a reference name (ht_mi355x.h "the hand's size"; the reference's applications ask the user: "hand size %f cm (use +/- to scale)").  EstimateHandSize:
	// the factor by which this tracker's model should grow to explain the frames of one view.  frames: one per tracked frame (one size; each frame's DCamera is read whole,
	// its pose places the view in tracking space); poses: per frame the tracked model's centre-of-mass poses (handmodel.GetPose() after the update of that frame).  One
	// scale for the batch (HT_SIZE_SHARED); the batch is not bounded by the tracker's one slot.  scale is relative to the model as it is now: apply it with scale(r.scale).
	// T: per frame the view's pose after the rigid shifts free_pose allows (the cameras' own when free_pose is 0); stats: the (iterations + 1) rows of
	// HT_SIZE_ROW(1, frames) doubles the C call documents; degenerate: the scale's record of some row carries a flag (no usable frame, no positive pivot, a clamped step).
	struct SizeOptions : ht_size { explicit SizeOptions(const HandTracker &t) { ht_size_default(t.ctx_, this); } };
	struct HandSize { float scale; std::vector<Pose> T; std::vector<double> stats; bool degenerate; };
	HandSize EstimateHandSize(const std::vector<Image<unsigned short>> &frames, const std::vector<std::vector<Pose>> &poses, const ht_size *options = nullptr)
	{
		const int B = (int)frames.size();
		if (B < 1 || poses.size() != frames.size()) throw std::runtime_error("EstimateHandSize: one set of poses per frame, at least one frame");
		const SizeOptions dflt(*this);
		ht_size o = options ? *options : dflt;
		if (o.mode != HT_SIZE_SHARED) throw std::runtime_error("EstimateHandSize: one scale for the batch (HT_SIZE_SHARED); the per-slot mode is the C call's");
		const int w = frames[0].dim().x, h = frames[0].dim().y;
		std::vector<unsigned short> depth; std::vector<float> cams((size_t)B * HT_CAM), p7;
		for (int b = 0; b < B; b++)
		{
			if (frames[b].dim().x != w || frames[b].dim().y != h || frames[b].raster.size() != (size_t)w * h) throw std::runtime_error("EstimateHandSize: the frames of a call have one size");
			if ((int)poses[b].size() != nb_) throw std::runtime_error("EstimateHandSize: one pose per body of the tracker's model for every frame");
			depth.insert(depth.end(), frames[b].raster.begin(), frames[b].raster.end());
			cam12(frames[b].cam, &cams[(size_t)b * HT_CAM]);
			const std::vector<float> f = flat(poses[b]);
			p7.insert(p7.end(), f.begin(), f.end());
		}
		HandSize r;
		const size_t row = (size_t)HT_SIZE_ROW(1, B);
		r.stats.assign((size_t)(o.iterations > 0 ? o.iterations + 1 : 1) * row, 0.0);
		std::vector<float> T((size_t)B * 7);
		check(ctx_, ht_estimate_scale(ctx_, 0, p7.data(), depth.data(), cams.data(), w, h, B, &o, &r.scale, T.data(), r.stats.data()));
		r.T.resize(B);
		for (int b = 0; b < B; b++) { const float *t = &T[(size_t)b * 7]; r.T[b].position = { t[0], t[1], t[2] }; r.T[b].orientation = { t[3], t[4], t[5], t[6] }; }
		r.degenerate = false;
		for (size_t i = 5; i < r.stats.size(); i += row) r.degenerate = r.degenerate || r.stats[i] != 0.0;
		return r;
	}
	// Addition, not a reference name: GatherHandExpectedCNN (handtrack.h:160-173) for a batch of pose sets on this tracker's device, frame b seen by the
	// heat-map camera hcams[b] (as the single-frame form takes it); segment_frame: train-cnn's compress first (train-cnn.cpp:31-50: the poses in the
	// camera's frame, the camera at the identity).  The same ExpectedCNN sets as the single-frame form, bit for bit (ht_expected_cnn_batch).
	std::vector<ExpectedCNN> GatherHandExpectedCNN(const std::vector<std::vector<Pose>> &poses, const std::vector<DCamera> &hcams, bool segment_frame = false) const;
private:
	ht_ctx *ctx_ = nullptr; int nb_ = 0;
	ht_ctx *job_ = nullptr; bool job_in_flight_ = false; Image<unsigned short> job_image_; std::string model_path_; int device_ = 0;      // the overlapped mode's second context
	void ensure_job_context()
	{
		if (!job_)
		{
			int rc = ht_create(model_path_.c_str(), 1, device_, &job_);
			if (rc != HT_OK) { std::string msg = job_ ? ht_last_error(job_) : "ht_create failed"; if (job_) ht_destroy(job_); job_ = nullptr; throw std::runtime_error("HandTracker (job context): " + msg); }
			std::vector<float> w(HT_CNNB_COUNT);
			check(ctx_, ht_cnn_get_weights(ctx_, w.data(), w.size()));      // the net the tracker carries (fails loudly when none was loaded)
			check(job_, ht_cnn_load_weights(job_, w.data(), w.size()));
		}
		if (!job_in_flight_) { ht_params p; pull_params(p); check(job_, ht_set_params(job_, &p)); }      // the job runs with the tunables as they stood when it was started
	}
	std::vector<Pose> cnn_job(Image<unsigned short> dimage, bool apply)
	{
		push_params();
		if (left_hand) dimage = mirror_image(dimage);      // (addition) the job runs on the canonical frame; its pose is mirrored on the way out
		const DCamera &fc = dimage.cam;
		const float fcam[HT_CAM] = { fc.focal().x, fc.focal().y, fc.principal().x, fc.principal().y, fc.depth_scale, fc.pose.position.x, fc.pose.position.y, fc.pose.position.z,
		                             fc.pose.orientation.x, fc.pose.orientation.y, fc.pose.orientation.z, fc.pose.orientation.w };
		std::vector<float> out((size_t)nb_ * HT_POSE); int accepted = 0;
		check(ctx_, ht_update_cnn_model_sync(ctx_, dimage.raster.data(), fcam, dimage.dim().x, dimage.dim().y, segment_scale, 1, apply ? 1 : 0, out.data(), &accepted, cnn_output.data()));
		if (dimage.dim().x != 64 || dimage.dim().y != 64) dimage = segment(dimage, 0xF, { 0.1f, drangey }, segment_scale);
		fill_visualisation(dimage);
		std::vector<Pose> pose;
		if (accepted) { pose.resize(nb_); for (int b = 0; b < nb_; b++) { const float *p = &out[(size_t)b * HT_POSE]; pose[b].position = { p[0], p[1], p[2] }; pose[b].orientation = { p[3], p[4], p[5], p[6] }; } }
		return left_hand ? mirrored(pose) : pose;
	}
	// (addition) the frame and its camera under the mirror, by the host mirror calls (ht_mirror_frames, ht_mirror_cams)
	// the arrays the several-views calls take for one slot: frames [V][h][w], cameras [V][12], planes [V][4] (empty: none)
	struct view_arrays { int V, w, h; std::vector<unsigned short> depth; std::vector<float> cams, planes; };
	static view_arrays pack_views(const std::vector<Image<unsigned short>> &views, const std::vector<float4> &mirrors)
	{
		view_arrays a;
		a.V = (int)views.size();
		if (a.V < 1 || a.V > HT_VIEWS_MAX) throw std::runtime_error("HandTracker: between 1 and HT_VIEWS_MAX views");
		if (!mirrors.empty() && (int)mirrors.size() != a.V) throw std::runtime_error("HandTracker: one mirror plane per view, or none");
		a.w = views[0].dim().x; a.h = views[0].dim().y;
		a.cams.resize((size_t)a.V * HT_CAM);
		for (int v = 0; v < a.V; v++)
		{
			if (views[v].dim().x != a.w || views[v].dim().y != a.h || views[v].raster.size() != (size_t)a.w * a.h) throw std::runtime_error("HandTracker: the views of a call have one size");
			a.depth.insert(a.depth.end(), views[v].raster.begin(), views[v].raster.end());
			cam12(views[v].cam, &a.cams[(size_t)v * HT_CAM]);
		}
		for (const float4 &m : mirrors) { a.planes.push_back(m.x); a.planes.push_back(m.y); a.planes.push_back(m.z); a.planes.push_back(m.w); }
		return a;
	}
	static void cam12(const DCamera &c, float *cam)
	{
		const float v[HT_CAM] = { c.focal().x, c.focal().y, c.principal().x, c.principal().y, c.depth_scale, c.pose.position.x, c.pose.position.y, c.pose.position.z,
		                          c.pose.orientation.x, c.pose.orientation.y, c.pose.orientation.z, c.pose.orientation.w };
		for (int i = 0; i < HT_CAM; i++) cam[i] = v[i];
	}
	Image<unsigned short> mirror_image(const Image<unsigned short> &im) const
	{
		const int w = im.dim().x, h = im.dim().y;
		float cam[HT_CAM], co[HT_CAM]; cam12(im.cam, cam);
		std::vector<unsigned short> flipped(im.raster.size());
		if (im.raster.size() != (size_t)w * h) throw std::runtime_error("HandTracker: the raster does not match the camera's dimensions");
		check(ctx_, ht_mirror_frames(ctx_, im.raster.data(), w, h, 1, nullptr, flipped.data()));
		check(ctx_, ht_mirror_cams(ctx_, cam, w, 1, nullptr, co));
		Pose pose; pose.position = { co[5], co[6], co[7] }; pose.orientation = { co[8], co[9], co[10], co[11] };
		return Image<unsigned short>(DCamera({ w, h }, { co[0], co[1] }, { co[2], co[3] }, co[4], pose), std::move(flipped));
	}
	// cnn_input and the drawn parts of cnn_output_analysis, filled on the host from what the device returned (handtrack.h:700, 225, 236-238)
	void fill_visualisation(const Image<unsigned short> &tile)
	{
		const DCamera &c = tile.cam;
		const float dr = drangey - 0.1f;
		cnn_input = Image<float>(c);
		for (size_t i = 0; i < tile.raster.size(); i++) { float v = 1.0f - (tile.raster[i] * c.depth_scale - 0.1f) / dr; cnn_input.raster[i] = v < 0.0f ? 0.0f : (v > 1.0f ? 1.0f : v); }
		const DCamera hcam = camsub(c, 4);
		cnn_output_analysis.hmaps.clear();
		for (int m = 0; m < 8; m++)
		{
			Image<unsigned char> h(hcam);
			for (int i = 0; i < 256; i++) { float y = cnn_output[(size_t)256 * m + i] * 255.0f; h.raster[i] = (unsigned char)(y < 0.0f ? 0.0f : (y > 255.0f ? 255.0f : y)); }      // ToGrayScale misc_image.h:169
			cnn_output_analysis.hmaps.push_back(h);
		}
		cnn_output_analysis.vmap = Image<float>(DCamera({ 16, 16 }, { 16.f, 16.f }, { 8.f, 8.f }, c.depth_scale), std::vector<float>(cnn_output.begin() + 2048, cnn_output.end()));
	}
	std::vector<float> flat(const std::vector<Pose> &pose) const
	{
		std::vector<float> f((size_t)nb_ * HT_POSE, 0.f);
		for (int b = 0; b < nb_ && b < (int)pose.size(); b++) { float *p = &f[(size_t)b * HT_POSE]; p[0] = pose[b].position.x; p[1] = pose[b].position.y; p[2] = pose[b].position.z; p[3] = pose[b].orientation.x; p[4] = pose[b].orientation.y; p[5] = pose[b].orientation.z; p[6] = pose[b].orientation.w; }
		return f;
	}
	void pull_params(ht_params &p)
	{
		check(ctx_, ht_get_params(ctx_, &p));
		p.full_reset_on_error = full_reset_on_error; p.angles_only = angles_only; p.always_take_cnn = always_take_cnn; p.drangey = drangey; p.boundary_planes = boundary_planes;
		p.microforce = microforce; p.cloudforce_max_point = cloudforce_max_point; p.cloudforce_max_sum = cloudforce_max_sum; p.mainthreadpasses = mainthreadpasses;
		p.subsample_fraction = subsample_fraction; p.min_point_num = (int)min_point_num; p.accum_error_threshold = accum_error_threshold; p.min_cray_prob = min_cray_prob;
		p.subsample_voxel = subsample_voxel; p.subsample_size = subsample_size;
		p.steps = steps; p.steps_keypoints = steps_keypoints; p.steps_keyangles = steps_keyangles; p.steps_palmangle = steps_palmangle; p.steps_cloudstart = steps_cloudstart; p.steps_unibody = steps_unibody;
	}
	void push_params()
	{
		ht_params p; pull_params(p);
		check(ctx_, ht_set_params(ctx_, &p));
	}
};
// Free function with the reference's signature (handtrack.h:280); it runs on the device of the first live HandTracker.
inline Image<unsigned short> HandSegmentVR(const Image<unsigned short> &depth, int entry_options = 0xF, float2 wrange = { 0.1f, 0.65f }, float diam = 0.17f)
{
	if (!detail::live_ctx()) throw std::runtime_error("HandSegmentVR: construct a HandTracker first (the segmentation runs on its device)");
	return HandTracker::segment_on(detail::live_ctx(), depth, entry_options, wrange, diam);
}

// Additions (two hands in one frame, include/ht_mi355x.h "two hands in one frame"; the reference segments one hand per frame).
// SplitHands cuts a frame into one masked frame per hand on the device of the first live HandTracker or TwoHandTracker: the blobs of the quarter-size image in
// [range_lo, range_hi) raw depth units, the two largest, the right hand the one at higher x (lower x with HT_SPLIT_RIGHT_IS_LOW_X).  With HT_SPLIT_MIRROR_LEFT the left
// frame and its camera come mirrored, ready for a right-hand tracker.  present[k] says whether hand k (0 right, 1 left) was found; info is ht_split_hands' record.
struct SplitResult { Image<unsigned short> right, left; bool present[2]; int info[2][8]; int n_components; };
inline SplitResult SplitHandsOn(ht_ctx *ctx, const Image<unsigned short> &depth, unsigned short range_lo, unsigned short range_hi, unsigned short far, unsigned short max_step = 65535, int min_pixels = 1, int flags = 0)
{
	const int w = depth.dim().x, h = depth.dim().y;
	if (depth.raster.size() != (size_t)w * h) throw std::runtime_error("SplitHands: the raster does not match the camera's dimensions");
	const DCamera &c = depth.cam;
	const float cam[HT_CAM] = { c.focal().x, c.focal().y, c.principal().x, c.principal().y, c.depth_scale, c.pose.position.x, c.pose.position.y, c.pose.position.z,
	                            c.pose.orientation.x, c.pose.orientation.y, c.pose.orientation.z, c.pose.orientation.w };
	std::vector<unsigned short> out((size_t)2 * w * h); float co[2][HT_CAM];
	SplitResult r;
	check(ctx, ht_split_hands(ctx, depth.raster.data(), cam, w, h, 1, range_lo, range_hi, max_step, min_pixels, far, flags, out.data(), &co[0][0], &r.info[0][0], &r.n_components, nullptr));
	Image<unsigned short> *im[2] = { &r.right, &r.left };
	for (int k = 0; k < 2; k++)
	{
		Pose pose; pose.position = { co[k][5], co[k][6], co[k][7] }; pose.orientation = { co[k][8], co[k][9], co[k][10], co[k][11] };
		*im[k] = Image<unsigned short>(DCamera({ w, h }, { co[k][0], co[k][1] }, { co[k][2], co[k][3] }, co[k][4], pose), std::vector<unsigned short>(out.begin() + (size_t)k * w * h, out.begin() + (size_t)(k + 1) * w * h));
		r.present[k] = r.info[k][0] > 0;
	}
	return r;
}
inline SplitResult SplitHands(const Image<unsigned short> &depth, unsigned short range_lo, unsigned short range_hi, unsigned short far, unsigned short max_step = 65535, int min_pixels = 1, int flags = 0)
{
	if (!detail::live_ctx()) throw std::runtime_error("SplitHands: construct a HandTracker or a TwoHandTracker first (the split runs on its device)");
	return SplitHandsOn(detail::live_ctx(), depth, range_lo, range_hi, far, max_step, min_pixels, flags);
}
// SplitHandsByModel (include/ht_mi355x.h "two hands that touch or cross"): the same cut by the tracked models and not by blobs -- every foreground cell goes to the hand
// whose bodies, at the given centre-of-mass poses in the camera's own space (HT_SPLIT_USER_POSES: rig-space poses, what update() returns), are nearer by the tracker's
// closest().  `left` is the left hand's own (unmirrored) pose.  mode HT_SPLIT_MODEL_ALWAYS or HT_SPLIT_MODEL_MERGED (only where the blobs have merged and both hands come
// out present); max_dist in metres drops cells far from both hands.  source: 1 the models decided, 0 the blob split's result stands.
struct SplitModelResult : SplitResult { int source; };
inline SplitModelResult SplitHandsByModelOn(ht_ctx *ctx, const Image<unsigned short> &depth, const std::vector<Pose> &right, const std::vector<Pose> &left, unsigned short range_lo, unsigned short range_hi,
                                            unsigned short far, float max_dist = std::numeric_limits<float>::infinity(), int mode = HT_SPLIT_MODEL_ALWAYS, unsigned short max_step = 65535, int min_pixels = 1, int flags = 0)
{
	const int w = depth.dim().x, h = depth.dim().y;
	if (depth.raster.size() != (size_t)w * h) throw std::runtime_error("SplitHandsByModel: the raster does not match the camera's dimensions");
	int nb = 0; ht_model_info(ctx, &nb, nullptr, nullptr);
	if ((int)right.size() != nb || (int)left.size() != nb) throw std::runtime_error("SplitHandsByModel: one pose per body of the tracker's model for either hand");
	const DCamera &c = depth.cam;
	const float cam[HT_CAM] = { c.focal().x, c.focal().y, c.principal().x, c.principal().y, c.depth_scale, c.pose.position.x, c.pose.position.y, c.pose.position.z,
	                            c.pose.orientation.x, c.pose.orientation.y, c.pose.orientation.z, c.pose.orientation.w };
	std::vector<float> poses((size_t)2 * nb * HT_POSE);
	for (int k = 0; k < 2; k++) for (int b = 0; b < nb; b++)
	{
		const Pose &q = (k ? left : right)[b]; float *p = &poses[((size_t)k * nb + b) * HT_POSE];
		p[0] = q.position.x; p[1] = q.position.y; p[2] = q.position.z; p[3] = q.orientation.x; p[4] = q.orientation.y; p[5] = q.orientation.z; p[6] = q.orientation.w;
	}
	std::vector<unsigned short> out((size_t)2 * w * h); float co[2][HT_CAM];
	SplitModelResult r;
	check(ctx, ht_split_hands_model(ctx, depth.raster.data(), cam, poses.data(), w, h, 1, range_lo, range_hi, max_step, min_pixels, far, max_dist, mode, flags, out.data(), &co[0][0], &r.info[0][0], &r.n_components,
	                                &r.source, nullptr, nullptr));
	Image<unsigned short> *im[2] = { &r.right, &r.left };
	for (int k = 0; k < 2; k++)
	{
		Pose pose; pose.position = { co[k][5], co[k][6], co[k][7] }; pose.orientation = { co[k][8], co[k][9], co[k][10], co[k][11] };
		*im[k] = Image<unsigned short>(DCamera({ w, h }, { co[k][0], co[k][1] }, { co[k][2], co[k][3] }, co[k][4], pose), std::vector<unsigned short>(out.begin() + (size_t)k * w * h, out.begin() + (size_t)(k + 1) * w * h));
		r.present[k] = r.info[k][0] > 0;
	}
	return r;
}
inline SplitModelResult SplitHandsByModel(const Image<unsigned short> &depth, const std::vector<Pose> &right, const std::vector<Pose> &left, unsigned short range_lo, unsigned short range_hi, unsigned short far,
                                          float max_dist = std::numeric_limits<float>::infinity(), int mode = HT_SPLIT_MODEL_ALWAYS, unsigned short max_step = 65535, int min_pixels = 1, int flags = 0)
{
	if (!detail::live_ctx()) throw std::runtime_error("SplitHandsByModel: construct a HandTracker or a TwoHandTracker first (the split runs on its device and its model)");
	return SplitHandsByModelOn(detail::live_ctx(), depth, right, left, range_lo, range_hi, far, max_dist, mode, max_step, min_pixels, flags);
}
// Both hands of one camera: one context of two tracker slots, slot 0 the right hand, slot 1 the left hand in canonical (mirrored) space.  update() splits the frame on the
// device, tracks both slots with ht_update_two_hands_sync and returns both hands' rig-space poses (what handmodel.GetPoseUser() is for a HandTracker) in the camera's own
// space, with the presence flags: the poses of an absent hand mean nothing.  Synchronous only (no overlapped arrangement).  The range is in metres like HandSegmentVR's
// wrange; everything nearer than wrange.y and not nearer than wrange.x is foreground, and `far` metres is written where a hand's frame is masked.
struct TwoHandTracker
{
	struct Hands { std::vector<Pose> right, left; bool present[2]; int info[2][8]; int source; };      // source: 1 the tracked models split the frame, 0 the blobs
	// how update() splits the frame: by blobs (the default; hands that touch are one blob and one of them is lost), by the slots' tracked models where the blobs have
	// merged, or always by the models; max_dist (metres): with the models, cells farther than this from both hands are dropped (a forearm, a torso in range)
	enum split_mode_t { Blobs, ModelWhenMerged, ModelAlways };
	split_mode_t split_mode = Blobs; float max_dist = std::numeric_limits<float>::infinity();
	float segment_scale = 0.17f; float2 wrange{ 0.1f, 0.65f }; float far = 4.0f; float max_step = 0.0f;      // max_step in metres between neighbouring quarter-size pixels of one blob; 0: no depth test
	int min_pixels = 16; bool right_is_low_x = false;      // right_is_low_x: a camera facing the user
	int side = 64; CNN cnn;
	explicit TwoHandTracker(const std::string &model_path = "../assets/model_hand.json", const std::string &cnnb_path = "../assets/handposedd.cnnb", int device = 0)
	{
		const int rc = ht_create(model_path.c_str(), 2, device, &ctx_);
		if (rc != HT_OK) { std::string msg = ctx_ ? ht_last_error(ctx_) : "ht_create failed"; if (ctx_) ht_destroy(ctx_); ctx_ = nullptr; throw std::runtime_error("TwoHandTracker: " + msg); }
		cnn.ctx_ = ctx_;
		if (!detail::live_ctx()) detail::live_ctx() = ctx_;
		ht_model_info(ctx_, &nb_, nullptr, nullptr);
		if (!cnnb_path.empty()) { std::ifstream is(cnnb_path, std::ios_base::in | std::ios_base::binary); if (is.is_open()) cnn.loadb(is); }
	}
	~TwoHandTracker() { if (detail::live_ctx() == ctx_) detail::live_ctx() = nullptr; if (ctx_) ht_destroy(ctx_); }
	TwoHandTracker(const TwoHandTracker &) = delete; TwoHandTracker &operator=(const TwoHandTracker &) = delete;
	ht_ctx *context() const { return ctx_; }
	// both hands' starting poses in the camera's space (centre-of-mass poses, as HandTracker::SetPose takes them): the left hand's are mirrored into its slot
	void SetPose(const std::vector<Pose> &right, const std::vector<Pose> &left)
	{
		std::vector<float> f = flat(right); const std::vector<float> l = flat(mirrored(left));
		f.insert(f.end(), l.begin(), l.end());
		check(ctx_, ht_tracker_reset(ctx_, 0, 2, f.data()));
	}
	Hands update(const Image<unsigned short> &dimage)
	{
		const DCamera &c = dimage.cam;
		const int w = dimage.dim().x, h = dimage.dim().y;
		if (dimage.raster.size() != (size_t)w * h) throw std::runtime_error("TwoHandTracker: the raster does not match the camera's dimensions");
		const float cam[HT_CAM] = { c.focal().x, c.focal().y, c.principal().x, c.principal().y, c.depth_scale, c.pose.position.x, c.pose.position.y, c.pose.position.z,
		                            c.pose.orientation.x, c.pose.orientation.y, c.pose.orientation.z, c.pose.orientation.w };
		const auto units = [&](float metres) { const float u = metres / c.depth_scale; return (unsigned short)(u < 0.0f ? 0.0f : (u > 65535.0f ? 65535.0f : u)); };
		std::vector<float> out((size_t)2 * nb_ * HT_POSE);
		Hands r;
		const unsigned short step = max_step > 0.0f ? units(max_step) : (unsigned short)65535;
		r.source = 0;
		if (split_mode == Blobs)
			check(ctx_, ht_update_two_hands_sync(ctx_, side, dimage.raster.data(), cam, w, h, segment_scale, units(wrange.x), units(wrange.y), step, min_pixels, units(far), right_is_low_x ? HT_SPLIT_RIGHT_IS_LOW_X : 0, 1,
			                                     out.data(), &r.info[0][0], nullptr));
		else      // (the position rule names no hand in ModelAlways: right_is_low_x bears on the blob split of ModelWhenMerged only)
			check(ctx_, ht_update_two_hands_model_sync(ctx_, side, dimage.raster.data(), cam, w, h, segment_scale, units(wrange.x), units(wrange.y), step, min_pixels, units(far), max_dist,
			                                           split_mode == ModelAlways ? HT_SPLIT_MODEL_ALWAYS : HT_SPLIT_MODEL_MERGED, split_mode == ModelWhenMerged && right_is_low_x ? HT_SPLIT_RIGHT_IS_LOW_X : 0, 1,
			                                           out.data(), &r.info[0][0], &r.source, nullptr));
		std::vector<Pose> *hand[2] = { &r.right, &r.left };
		for (int k = 0; k < 2; k++)
		{
			hand[k]->resize(nb_);
			for (int b = 0; b < nb_; b++) { const float *p = &out[((size_t)k * nb_ + b) * HT_POSE]; (*hand[k])[b].position = { p[0], p[1], p[2] }; (*hand[k])[b].orientation = { p[3], p[4], p[5], p[6] }; }
			r.present[k] = r.info[k][0] > 0;
		}
		return r;
	}
private:
	std::vector<float> flat(const std::vector<Pose> &pose) const
	{
		std::vector<float> f((size_t)nb_ * HT_POSE, 0.f);
		for (int b = 0; b < nb_ && b < (int)pose.size(); b++) { float *p = &f[(size_t)b * HT_POSE]; p[0] = pose[b].position.x; p[1] = pose[b].position.y; p[2] = pose[b].position.z; p[3] = pose[b].orientation.x; p[4] = pose[b].orientation.y; p[5] = pose[b].orientation.z; p[6] = pose[b].orientation.w; }
		return f;
	}
	ht_ctx *ctx_ = nullptr; int nb_ = 0;
};

// The noise set of ht_sensor_simulate (ht_mi355x.h) as a value: SensorNoise(HT_SENSOR_DS4, cam.depth_scale) holds ht_sensor_noise_default's figures -- reasoned
// from data sheets, never measured against a camera -- and every field can be changed afterwards (n.seed = ..., n.p_hole = 0).
struct SensorNoise : ht_sensor_noise
{
	SensorNoise() : ht_sensor_noise() { far_count = 3999; fly_bg_count = 3999; edge_step = 20; slope_step = 15; ir_floor = 16; }      // everything off, millimetre counts, 4 m
	SensorNoise(int kind, float depth_scale = 0.001f, float far = 4.0f)
	{
		if (ht_sensor_noise_default(kind, depth_scale, far, this) != HT_OK) throw std::runtime_error("SensorNoise: kind, depth_scale or far refused (ht_sensor_noise_default)");
	}
};

// RSCam's depth filters (include/dcam.h:144-244): what dcam.GetDepth() does to the sensor's frame before htk.update() sees it, on the device of the first live
// HandTracker.  No librealsense and no device handle: the caller hands over the raw frame (and, for an R200, the IR image of the same size) it got from its camera.
//     auto dimage = cam.FilterIvy(raw);  auto pose = htk.update(std::move(dimage));      // replaces htk.update(dcam.GetDepth()), realtime-tracker.cpp:56
struct RSCam
{
	int image_width_max_allowed = 320;                                                         // dcam.h:153
	Image<unsigned char> cache_ir;                                                             // dcam.h:163: the IR image that goes with the latest depth frame; SimulateDS4 writes it
	// Raw frames from rendered ones (ht_sensor_simulate; an addition): what a camera of either kind would have handed over instead of the clean frame `image`.
	// One frame is one stream: the frame is stream noise.first_index.  SimulateDS4 also gives the IR image (in *ir if asked for, and in cache_ir), so that
	//     auto raw = cam.SimulateDS4(rendered, noise);  auto dimage = cam.FilterDS4(raw, cam.cache_ir);
	Image<unsigned short> SimulateIvy(const Image<unsigned short> &image, const SensorNoise &noise) { return simulate(HT_SENSOR_IVY, image, noise, nullptr); }
	Image<unsigned short> SimulateDS4(const Image<unsigned short> &image, const SensorNoise &noise, Image<unsigned char> *ir = nullptr)
	{
		cache_ir = Image<unsigned char>(image.cam);
		Image<unsigned short> out = simulate(HT_SENSOR_DS4, image, noise, cache_ir.raster.data());
		if (ir) *ir = cache_ir;
		return out;
	}
	std::vector<uint16_t> background;                                                          // dcam.h:156: empty until addbackground is called
	void addbackground(const Image<unsigned short> &dp, unsigned short fudge = 3)              // dcam.h:157-162
	{
		const bool init = background.size() != dp.raster.size();
		if (init) background.resize(dp.raster.size());
		detail_check(ht_sensor_background(ctx(), dp.raster.data(), dp.dim().x, dp.dim().y, 1, fudge, init ? 1 : 0, background.data()));
	}
	Image<unsigned short> FilterDS4(const Image<unsigned short> &dp, const Image<unsigned char> &ir) { return filter(HT_SENSOR_DS4, dp, ir.raster.data(), ir.raster.size()); }      // dcam.h:174-208
	Image<unsigned short> FilterIvy(const Image<unsigned short> &dp) { return filter(HT_SENSOR_IVY, dp, nullptr, 0); }                                                             // dcam.h:209-226
private:
	static ht_ctx *ctx() { if (!detail::live_ctx()) throw std::runtime_error("RSCam: construct a HandTracker first (the filters run on its device)"); return detail::live_ctx(); }
	static void detail_check(int rc) { check(detail::live_ctx(), rc); }
	Image<unsigned short> simulate(int kind, const Image<unsigned short> &image, const SensorNoise &noise, unsigned char *ir)
	{
		const int w = image.dim().x, h = image.dim().y;
		if (w < 1 || h < 1 || image.raster.size() != (size_t)w * h) throw std::runtime_error("RSCam: a frame of this size cannot be simulated");
		Image<unsigned short> out(image.cam);
		detail_check(ht_sensor_simulate(ctx(), kind, image.raster.data(), w, h, 1, &noise, out.raster.data(), ir));
		return out;
	}
	Image<unsigned short> filter(int kind, const Image<unsigned short> &dp, const unsigned char *ir, size_t nir)
	{
		const int w = dp.dim().x, h = dp.dim().y;
		int wo = 0, ho = 0;
		if (dp.raster.size() != (size_t)w * h || (kind == HT_SENSOR_DS4 && nir != dp.raster.size()) || ht_sensor_out_dims(kind, w, h, image_width_max_allowed, &wo, &ho) != HT_OK)
			throw std::runtime_error("RSCam: a frame of this size cannot be filtered");
		float cam[HT_CAM] = { dp.cam.focal().x, dp.cam.focal().y, dp.cam.principal().x, dp.cam.principal().y, dp.cam.depth_scale, dp.cam.pose.position.x, dp.cam.pose.position.y, dp.cam.pose.position.z,
		                      dp.cam.pose.orientation.x, dp.cam.pose.orientation.y, dp.cam.pose.orientation.z, dp.cam.pose.orientation.w }, co[HT_CAM];
		Image<unsigned short> out(DCamera({ wo, ho }, { 0, 0 }, { 0, 0 }, dp.cam.depth_scale, dp.cam.pose));
		const bool bg = kind == HT_SENSOR_DS4 && background.size() == dp.raster.size();      // dcam.h:201
		detail_check(ht_sensor_filter(ctx(), kind, dp.raster.data(), ir, cam, w, h, 1, image_width_max_allowed, bg ? background.data() : nullptr, out.raster.data(), co));
		out.cam.focal() = { co[0], co[1] }; out.cam.principal() = { co[2], co[3] };
		return out;
	}
};

// CNN PoseInitializerCNN(std::string filename) (handtrack.h:103-130): the pose net as an object of its own (own CNN-only device context); like the
// reference, a missing weight file is not an error here -- Eval then fails loudly instead of running on random weights.
inline CNN PoseInitializerCNN(std::string filename, int device = 0)
{
	ht_ctx *ctx = nullptr;
	const int rc = ht_create(nullptr, 1, device, &ctx);
	if (rc != HT_OK) { const std::string msg = ctx ? ht_last_error(ctx) : "ht_create failed"; if (ctx) ht_destroy(ctx); throw std::runtime_error("PoseInitializerCNN: " + msg); }
	CNN cnn; cnn.ctx_ = ctx; cnn.own_ = std::shared_ptr<ht_ctx>(ctx, [](ht_ctx *c) { ht_destroy(c); });
	std::ifstream is(filename, std::ios_base::in | std::ios_base::binary);
	if (is.is_open()) cnn.loadb(is);
	return cnn;
}

// GatherHandExpectedCNN(pose, hcam) (handtrack.h:160-173): the labels the net is trained to produce for a hand pose seen by the 16x16 heat-map camera
struct ExpectedCNN { std::vector<float> cnn_expected; std::vector<float2> image_points; std::vector<Image<unsigned char>> hmaps; Image<unsigned char> vmap; std::vector<float> vals; };
namespace detail
{
// the C-ABI takes the 64x64 tile camera and forms camsub(cam, 4) itself; scaling by 4 and back is exact in binary floating point
inline void tile_cam_of(const DCamera &hcam, float *cam)
{
	const float c[HT_CAM] = { hcam.focal().x * 4.0f, hcam.focal().y * 4.0f, hcam.principal().x * 4.0f, hcam.principal().y * 4.0f, hcam.depth_scale,
	                          hcam.pose.position.x, hcam.pose.position.y, hcam.pose.position.z, hcam.pose.orientation.x, hcam.pose.orientation.y, hcam.pose.orientation.z, hcam.pose.orientation.w };
	for (int i = 0; i < HT_CAM; i++) cam[i] = c[i];
}
inline void flat_poses(const std::vector<Pose> &pose, float *p7)
{
	for (size_t b = 0; b < pose.size(); b++) { float *p = &p7[b * HT_POSE]; p[0] = pose[b].position.x; p[1] = pose[b].position.y; p[2] = pose[b].position.z; p[3] = pose[b].orientation.x; p[4] = pose[b].orientation.y; p[5] = pose[b].orientation.z; p[6] = pose[b].orientation.w; }
}
inline void fill_expected(ExpectedCNN &e, const float *ip, const DCamera &hcam);
}
inline ExpectedCNN GatherHandExpectedCNN(const std::vector<Pose> &pose, const DCamera &hcam)
{
	if (pose.size() < 17) throw std::runtime_error("GatherHandExpectedCNN: the landmark table names bones up to 16 (handtrack.h:77-81)");
	std::vector<float> p7(pose.size() * HT_POSE);
	detail::flat_poses(pose, p7.data());
	float cam[HT_CAM];
	detail::tile_cam_of(hcam, cam);
	ExpectedCNN e; e.cnn_expected.resize(HT_CNN_OUT); e.vals.resize(16);
	float ip[16];
	if (ht_expected_cnn_full(p7.data(), cam, e.cnn_expected.data(), ip, e.vals.data()) != HT_OK) throw std::runtime_error("GatherHandExpectedCNN failed");
	detail::fill_expected(e, ip, hcam);
	return e;
}
// the members of the Set the C-ABI does not return, made from the labels: image points, the eight 16x16 landmark maps and the key-angle map as bytes
inline void detail::fill_expected(ExpectedCNN &e, const float *ip, const DCamera &hcam)
{
	for (int k = 0; k < 8; k++) e.image_points.push_back({ ip[2 * k], ip[2 * k + 1] });
	auto gray = [](float v) { v *= 255.0f; return (unsigned char)(v < 0.0f ? 0.0f : v > 255.0f ? 255.0f : v + 0.5f); };      // the labels are bytes / 255: this recovers the byte
	for (int m = 0; m < 8; m++) { Image<unsigned char> h(hcam); for (int i = 0; i < 256; i++) h.raster[i] = gray(e.cnn_expected[(size_t)256 * m + i]); e.hmaps.push_back(h); }
	e.vmap = Image<unsigned char>(DCamera({ 16, 16 }, { 16.f, 16.f }, { 8.f, 8.f }, hcam.depth_scale));
	for (int i = 0; i < 256; i++) e.vmap.raster[i] = gray(e.cnn_expected[2048 + i]);
}
inline std::vector<ExpectedCNN> HandTracker::GatherHandExpectedCNN(const std::vector<std::vector<Pose>> &poses, const std::vector<DCamera> &hcams, bool segment_frame) const
{
	const int B = (int)poses.size();
	if (hcams.size() != poses.size()) throw std::runtime_error("GatherHandExpectedCNN: one camera per pose set");
	std::vector<float> p7((size_t)B * nb_ * HT_POSE), cams((size_t)B * HT_CAM), ex((size_t)B * HT_CNN_OUT), ip((size_t)B * 16), vals((size_t)B * 16);
	for (int b = 0; b < B; b++)
	{
		if ((int)poses[b].size() != nb_) throw std::runtime_error("GatherHandExpectedCNN: one pose per body");
		detail::flat_poses(poses[b], &p7[(size_t)b * nb_ * HT_POSE]);
		detail::tile_cam_of(hcams[b], &cams[(size_t)b * HT_CAM]);
	}
	check(ctx_, ht_expected_cnn_batch(ctx_, p7.data(), cams.data(), B, segment_frame ? HT_LABELS_SEGMENT_FRAME : 0, ex.data(), ip.data(), vals.data()));
	std::vector<ExpectedCNN> out((size_t)B);
	for (int b = 0; b < B; b++)
	{
		ExpectedCNN &e = out[(size_t)b];
		e.cnn_expected.assign(ex.begin() + (size_t)b * HT_CNN_OUT, ex.begin() + (size_t)(b + 1) * HT_CNN_OUT);
		e.vals.assign(vals.begin() + (size_t)b * 16, vals.begin() + (size_t)(b + 1) * 16);
		DCamera hc = hcams[(size_t)b];
		if (segment_frame) hc.pose = Pose();      // compress: the maps belong to the camera at the identity
		detail::fill_expected(e, &ip[(size_t)b * 16], hc);
	}
	return out;
}

// A hand model that is posed, drawn and ray-cast but not tracked (host only): `PhysModel fakehand = LoadHandModel();` (synthetic-tracker.cpp:94)
class PhysModel                                                                               // include/physmodel.h:236-477, the members the applications use
{
	std::shared_ptr<ht_model> m_;
public:
	struct Body { float3 position{ 0, 0, 0 }; float4 orientation{ 0, 0, 0, 1 }; float3 com{ 0, 0, 0 };
		Pose pose() const { Pose p; p.position = position; p.orientation = orientation; return p; }
		float3 PositionUser() const { return pose() * float3{ -com.x, -com.y, -com.z }; } };                          // physics.h:142
	struct ModelHitInfo { bool hit = false; float3 impact{ 0, 0, 0 }, normal{ 0, 0, 0 }; int rb = -1; operator bool() const { return hit; } };      // physmodel.h:280-286
	std::vector<Body> rigidbodies;
	std::vector<Mesh> sdmeshes, meshes;      // physmodel.h:251-252: the subdivision surfaces (rig space) and the collision hulls (centre-of-mass frames)
	explicit PhysModel(const char *jsonfile, bool hand_tweaks = false)
	{
		ht_model *m = nullptr;
		const int rc = ht_model_open(jsonfile, hand_tweaks ? 1 : 0, &m);
		if (rc != HT_OK) { const std::string msg = m ? ht_model_error(m) : "ht_model_open failed"; if (m) ht_model_close(m); throw std::runtime_error("PhysModel: " + msg); }
		m_ = std::shared_ptr<ht_model>(m, [](ht_model *x) { ht_model_close(x); });
		int nb = 0; ht_model_counts(m, &nb, nullptr);
		for (int b = 0; b < nb; b++)
		{
			float com[3], rest[7];
			ht_model_body(m, b, nullptr, nullptr, nullptr, com, rest);
			Body rb; rb.position = { rest[0], rest[1], rest[2] }; rb.orientation = { rest[3], rest[4], rest[5], rest[6] }; rb.com = { com[0], com[1], com[2] };
			rigidbodies.push_back(rb);
			meshes.push_back(detail::hull_mesh(m, b));
			sdmeshes.push_back(detail::subdivision_mesh(m, b));
		}
	}
	// Addition: this model becomes its own mirror image (ht_model_mirror: the left hand of a right-hand model, and back): hulls, subdivision meshes, centres of
	// mass and what HitCheck reads, and the bodies' current poses with them, so a posed model stays the same hand seen in a mirror.
	PhysModel &Mirror()
	{
		if (ht_model_mirror(m_.get()) != HT_OK) throw std::runtime_error("PhysModel::Mirror failed");
		for (size_t b = 0; b < rigidbodies.size(); b++)
		{
			float com[3] = { 0, 0, 0 };
			ht_model_body(m_.get(), (int)b, nullptr, nullptr, nullptr, com, nullptr);
			const Pose p = mirrored(rigidbodies[b].pose());
			rigidbodies[b].position = p.position; rigidbodies[b].orientation = p.orientation; rigidbodies[b].com = { com[0], com[1], com[2] };
			meshes[b] = detail::hull_mesh(m_.get(), (int)b); sdmeshes[b] = detail::subdivision_mesh(m_.get(), (int)b);
		}
		return *this;
	}
	std::vector<Pose> GetPose() const { std::vector<Pose> p; for (auto &rb : rigidbodies) p.push_back(rb.pose()); return p; }                                            // physmodel.h:433
	std::vector<Pose> GetPoseUser() const { std::vector<Pose> p; for (auto &rb : rigidbodies) { Pose q = rb.pose(); q.position = rb.PositionUser(); p.push_back(q); } return p; }      // :434
	PhysModel &SetPose(const std::vector<Pose> &poses) { for (size_t i = 0; i < poses.size() && i < rigidbodies.size(); i++) { rigidbodies[i].position = poses[i].position; rigidbodies[i].orientation = poses[i].orientation; } return *this; }      // :435
	std::vector<Mesh> &GetMeshes(int show_subdiv = 0)                                                                                                                    // :295-303
	{
		for (size_t i = 0; i < rigidbodies.size(); i++) { Pose u = rigidbodies[i].pose(); u.position = rigidbodies[i].PositionUser(); sdmeshes[i].pose = u; }      // the subdivision meshes are in rig space
		for (size_t i = 0; i < rigidbodies.size(); i++) meshes[i].pose = rigidbodies[i].pose();                                                                   // the hulls in the centre-of-mass frames
		return show_subdiv ? sdmeshes : meshes;
	}
	ModelHitInfo HitCheck(const float3 &v0, const float3 &v1) const                                                                                                      // :287-294
	{
		std::vector<float> p7(rigidbodies.size() * HT_POSE);
		for (size_t b = 0; b < rigidbodies.size(); b++) { const Body &rb = rigidbodies[b]; float *p = &p7[b * HT_POSE]; p[0] = rb.position.x; p[1] = rb.position.y; p[2] = rb.position.z; p[3] = rb.orientation.x; p[4] = rb.orientation.y; p[5] = rb.orientation.z; p[6] = rb.orientation.w; }
		ModelHitInfo h;
		ht_model_hitcheck(m_.get(), p7.data(), &v0.x, &v1.x, &h.impact.x, &h.normal.x, &h.rb);
		h.hit = h.rb >= 0;
		return h;
	}
};
inline PhysModel LoadHandModel(const char *jsonfile = "../assets/model_hand.json") { return PhysModel(jsonfile, true); }                                                    // handtrack.h:347-366
}  // namespace ht_mi355x

#ifdef HT_MI355X_GLOBAL_NAMES      // the reference's headers declare these names at global scope
using ht_mi355x::float2; using ht_mi355x::float3; using ht_mi355x::float4; using ht_mi355x::int2; using ht_mi355x::int3;
using ht_mi355x::Pose; using ht_mi355x::mirrored; using ht_mi355x::DCamera; using ht_mi355x::Image; using ht_mi355x::Mesh; using ht_mi355x::CNN; using ht_mi355x::HandTracker; using ht_mi355x::PhysModel;
using ht_mi355x::RigidBody; using ht_mi355x::LimitLinear; using ht_mi355x::LimitAngular; using ht_mi355x::PhysicsUpdate; using ht_mi355x::Addresses;
using ht_mi355x::HandSegmentVR; using ht_mi355x::RSCam; using ht_mi355x::PointCloud; using ht_mi355x::camsub; using ht_mi355x::GatherHandExpectedCNN; using ht_mi355x::PoseInitializerCNN; using ht_mi355x::LoadHandModel;
#endif
