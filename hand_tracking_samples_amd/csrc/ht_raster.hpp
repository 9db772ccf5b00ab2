// ht_raster.hpp -- the mesh rasteriser's definition, one triangle and one pixel at a time (include/ht_mi355x.h: ht_model_raster_mesh).  The host's plain loop
// (ht_model_host.hip) and the kernel (ht_raster_mesh.hip) both call these, so each evaluates the same float expressions in the same order and the same exact
// integers; tests/mesh_raster_ref.py restates them in numpy.  The scene call (ht_model_raster_scene, ht_raster_scene.hip) adds the pieces at the end: a left
// instance's pose, principal point and column, the limits and the composite rule (tests/scene_raster_ref.py).
//
// Screen coordinates are snapped to 1/256 pixel: |sx|, |sy| < 2^20 gives |X|, |Y| < 2^28, every difference below fits 32 bits and every product 64.
#pragma once
#include "ht_math.hpp"

struct rz_tri
{
	int X[3], Y[3];             // the corners on the screen, in 1/256 pixel, pixel (x, y)'s sample at (256 x, 256 y)
	v3 N; float k;              // the plane in camera space: dot(N, p) = k
};

HT_HD bool rz_finite(float v) { return fabsf(v) < INFINITY; }      // false for NaN

// One corner: camera space, then the screen.  false: the triangle is dropped (behind the near distance, not finite, or off the snapping range)
HT_HD bool rz_corner(const m3 &R, v3 up, v3 v, float fx, float fy, float px, float py, float off, v3 &w, int &X, int &Y)
{
	w = up + mul(R, v);
	if (!(w.z >= HT_RASTER_NEAR) || !rz_finite(w.x) || !rz_finite(w.y) || !rz_finite(w.z)) return false;
	const float sx = (fx * (w.x / w.z) + px) - off, sy = (fy * (w.y / w.z) + py) - off;
	if (!(fabsf(sx) < 1048576.0f) || !(fabsf(sy) < 1048576.0f)) return false;
	X = (int)rintf(sx * 256.0f); Y = (int)rintf(sy * 256.0f);      // round-half-even; the product is exact
	return true;
}

// A triangle of the mesh at the body's frame {up, R}: false when it is dropped or faces away (A2 >= 0)
HT_HD bool rz_setup(const m3 &R, v3 up, v3 v0, v3 v1, v3 v2, float fx, float fy, float px, float py, float off, rz_tri &T)
{
	v3 w0, w1, w2;
	if (!rz_corner(R, up, v0, fx, fy, px, py, off, w0, T.X[0], T.Y[0])) return false;
	if (!rz_corner(R, up, v1, fx, fy, px, py, off, w1, T.X[1], T.Y[1])) return false;
	if (!rz_corner(R, up, v2, fx, fy, px, py, off, w2, T.X[2], T.Y[2])) return false;
	const long long A2 = (long long)(T.X[1] - T.X[0]) * (long long)(T.Y[2] - T.Y[0]) - (long long)(T.X[2] - T.X[0]) * (long long)(T.Y[1] - T.Y[0]);
	if (!(A2 < 0)) return false;
	T.N = cross(w1 - w0, w2 - w0);
	T.k = dot(T.N, w0);
	return true;
}

// the pixels whose samples lie in the corners' rectangle (the only ones an inclusive edge test can pass)
HT_HD int rz_min3(int a, int b, int c) { return a < b ? (a < c ? a : c) : (b < c ? b : c); }
HT_HD int rz_max3(int a, int b, int c) { return a > b ? (a > c ? a : c) : (b > c ? b : c); }
HT_HD void rz_rect(const rz_tri &T, int &x0, int &x1, int &y0, int &y1)
{
	x0 = (rz_min3(T.X[0], T.X[1], T.X[2]) + 255) >> 8; x1 = rz_max3(T.X[0], T.X[1], T.X[2]) >> 8;
	y0 = (rz_min3(T.Y[0], T.Y[1], T.Y[2]) + 255) >> 8; y1 = rz_max3(T.Y[0], T.Y[1], T.Y[2]) >> 8;
}

HT_HD bool rz_edge(int Xi, int Yi, int Xj, int Yj, int qx, int qy) { return (long long)(Xj - Xi) * (long long)(qy - Yi) - (long long)(Yj - Yi) * (long long)(qx - Xi) <= 0; }
// pixel (x, y), 0 <= x, y < 4096, inside the triangle: all three edges, inclusive
HT_HD bool rz_inside(const rz_tri &T, int x, int y)
{
	const int qx = 256 * x, qy = 256 * y;
	return rz_edge(T.X[0], T.Y[0], T.X[1], T.Y[1], qx, qy) && rz_edge(T.X[1], T.Y[1], T.X[2], T.Y[2], qx, qy) && rz_edge(T.X[2], T.Y[2], T.X[0], T.Y[0], qx, qy);
}

HT_HD float rz_ray(int x, float off, float p, float f) { return (((float)x + off) - p) / f; }
// the depth count of the triangle's plane on the ray (rx, ry, 1), or -1 when the pixel is no candidate
HT_HD int rz_count(const rz_tri &T, float rx, float ry, float far, float ds)
{
	const float den = (T.N.x * rx + T.N.y * ry) + T.N.z;
	const float z = T.k / den, c = z / ds;
	if (!rz_finite(c) || !(z >= HT_RASTER_NEAR && z < far) || !(c >= 0.0f && c < 65536.0f)) return -1;
	return (int)(unsigned short)c;
}

// ---- scenes of several hands (ht_model_raster_scene) ----
HT_HD bool rz_scene_absent(unsigned char flag) { return flag == HT_SCENE_ABSENT; }
HT_HD bool rz_scene_left(unsigned char flag) { return flag != 0 && flag != HT_SCENE_ABSENT; }
// H instances of a model with T mesh triangles: the winner's index i * T + triangle must stay below 65535 (0xffff is "nothing yet" beside the count 0xffff)
HT_HD bool rz_scene_fits(int H, int T) { return H >= 1 && H <= HT_SCENE_MAX_HANDS && T >= 0 && (long long)H * T <= 65535; }
// a left instance's pose as the definition takes it: the sign bits of px, qy, qz flipped (ht_mirror_poses); negation is the sign bit's flip, for -0 and NaN too
HT_HD void rz_mirror_pose(const float *p, float *o) { o[0] = -p[0]; o[1] = p[1]; o[2] = p[2]; o[3] = p[3]; o[4] = -p[4]; o[5] = -p[5]; o[6] = p[6]; }
// its principal point: pixel x samples x + off and its mirror pixel w-1-x samples w-1-x + off, so cx' = (w-1) + 2 off - cx; at off 0 the bits of ht_mirror_cams
HT_HD float rz_mirror_px(float cx, int w, float off)
{
	const float m = (float)(w - 1) - cx;
	return off == 0.0f ? m : m + (off + off);
}
// column x of an instance's layer is this column of the scene
HT_HD int rz_scene_column(int x, int w, bool left) { return left ? w - 1 - x : x; }
// the composite: is the winner's count written over the background count bgv?  (has_bg false: no background frame was given)
HT_HD bool rz_scene_wins(int count, bool has_bg, unsigned short bgv) { return !has_bg || bgv == 0 || count <= (int)bgv; }
