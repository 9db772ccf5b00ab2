// ht_api.hip -- the C-ABI layer (include/ht_mi355x.h): context, device memory, launch sequencing.
// Host code stays C++ and only sequences hand-written HIP kernels; there is no CPU fallback: every entry point fails with
// HT_ERR_HIP when no gfx950 device is usable.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <limits.h>
#include <cmath>
#include <string>
#include <vector>
#include <map>
#include "ht_device.hpp"
#include "ht_host.hpp"
#include "ht_launch.hpp"
#include "ht_model_build.hpp"
#include "ht_train_shared.hpp"      // the packed conv2 index

// ------------------------------------------------------------------------------------------------- context
static void default_params(ht_params &p)     // handtrack.h:523-547, physics.h:45-47, physmodel.h:234, handtrack.h:369,450
{
	p.full_reset_on_error = 0.6f; p.angles_only = 0; p.always_take_cnn = 0; p.drangey = 0.7f; p.boundary_planes = 1; p.microforce = 1.0f;
	p.cloudforce_max_point = 15.0f; p.cloudforce_max_sum = 3000.0f; p.mainthreadpasses = 1; p.subsample_fraction = 4; p.min_point_num = 400; p.subsample_voxel = 0; p.subsample_size = 0.0f;
	p.accum_error_threshold = 0.0f; p.min_cray_prob = 0.0f; p.steps = 5; p.steps_keypoints = 3; p.steps_keyangles = 2; p.steps_palmangle = 2; p.steps_cloudstart = 1; p.steps_unibody = 3;
	p.physics_iterations = 16; p.physics_iterations_post = 4; p.physics_use_collision = 1; p.physics_weak_force = 0.4f; p.bone_sum_error_scale = 4.0f; p.unibody_force = 0.1f;
}

// The contact kernel's image of the collision vertices: every body padded to whole rows of 16 with copies of its vertex 0 (index 0), built from
// the model's vertices as the device takes them (again after ht_scale).
static int upload_padded_verts(ht_ctx *ctx, const std::vector<float4> &verts)
{
	ht_model_dev &m = ctx->model;
	std::vector<float4> pv;
	for (int b = 0; b < m.nb; b++)
	{
		m.cvert_off[b] = (int)pv.size();
		const int n = m.vert_off[b + 1] - m.vert_off[b], np = (n + 15) & ~15;
		for (int k = 0; k < np; k++) { const int src = k < n ? k : 0; float4 q = verts[(size_t)m.vert_off[b] + src]; memcpy(&q.w, &src, 4); pv.push_back(q); }
	}
	m.cvert_off[m.nb] = (int)pv.size();
	if (!ctx->d_cverts_rw) { int r = dev_alloc(ctx, &ctx->d_cverts_rw, pv.size() ? pv.size() : 1); if (r) return r; }
	if (pv.size()) HIPCHK(ctx, hipMemcpy(ctx->d_cverts_rw, pv.data(), pv.size() * sizeof(float4), hipMemcpyHostToDevice));
	m.cverts = ctx->d_cverts_rw;
	return HT_OK;
}
// a model array on the device: allocated by the first call (load_model), written again by the later ones (ht_scale; the sizes do not change)
template <class T> static int dev_put(ht_ctx *ctx, T **p, const T *h, size_t n)
{
	if (!*p) { const int r = dev_alloc(ctx, p, n ? n : 1); if (r) return r; }
	if (n) HIPCHK(ctx, hipMemcpy(*p, h, n * sizeof(T), hipMemcpyHostToDevice));
	return HT_OK;
}
// The record laid out for the device, at load and again after ht_scale: vertices as float4 with the index within the body in w (bit pattern, used by the support
// scans), the padded collision vertices, the mesh rows and radii, planes, body and joint tables.  It waits for the context's stream first and, before the mesh rows
// go, for a render of the old meshes on the caller's stream.
static int model_to_device(ht_ctx *ctx)
{
	const ht_model_rec &rec = ctx->rec;
	ht_model_dev &m = ctx->model;
	std::vector<float4> verts(rec.verts.size() / 3);
	for (int b = 0; b < m.nb; b++) for (int i = m.vert_off[b], k = 0; i < m.vert_off[b + 1]; i++, k++)
	{ verts[i] = make_float4(rec.verts[3 * (size_t)i], rec.verts[3 * (size_t)i + 1], rec.verts[3 * (size_t)i + 2], 0.0f); memcpy(&verts[i].w, &k, 4); }
	int r;
	HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
	if ((r = dev_put(ctx, &ctx->d_verts_rw, verts.data(), verts.size())) || (r = upload_padded_verts(ctx, verts))) return r;
	if (ctx->last_user_stream && ctx->last_user_stream != ctx->stream) HIPCHK(ctx, hipStreamSynchronize(ctx->last_user_stream));
	if ((r = ht_mesh_upload(ctx))) return r;
	if ((r = dev_put(ctx, &ctx->d_planes_rw, (const float4 *)rec.planes.data(), rec.planes.size() / 4)) || (r = dev_put(ctx, &ctx->d_bodyc_rw, rec.bodyc.data(), rec.bodyc.size())) ||
	    (r = dev_put(ctx, &ctx->d_jointc_rw, rec.jointc.data(), rec.jointc.size()))) return r;
	m.verts = ctx->d_verts_rw; m.planes = ctx->d_planes_rw; m.bodyc = ctx->d_bodyc_rw; m.jointc = ctx->d_jointc_rw;
	return HT_OK;
}

static int load_model(ht_ctx *ctx, const char *path)
{
	ht_model_rec &rec = ctx->rec;
	if (!ht_model_read(path, HT_BUILD_HAND_TWEAKS, rec, ctx->err)) return HT_ERR_IO;
	auto lacks = [&](const char *n) { if (!rec.lacks(n)) return false; ctx->err = std::string("model entry missing: ") + n; return true; };
	if (lacks("nb") || lacks("nj")) return HT_ERR_IO;
	const int nb = rec.nb, nj = rec.nj;
	// body slot HT_MAXNB-1 is the solver's idle body; 26 joints: the most whose angular rows a solve can always keep (13 CNN-driven + 6 range rows + slowfit's 3 relative
	// rows per joint = 247 of 252: csrc/ht_solver.hip), so that no model this accepts can run into that capacity
	if (nb < 1 || nb >= HT_MAXNB || nj > 26) { ctx->err = "model too large (at most 31 bodies and 26 joints)"; return HT_ERR_IO; }
	// a context needs the physics constants, collision lists and unibody proxy and can do without the hull triangles; of several absent entries the last one is named
	bool absent = false;
	for (const char *n : { "body_f", "body_collide", "ignore", "joint_i", "joint_f", "physics", "unibody/verts", "unibody/f" }) absent = lacks(n) || absent;
	for (const std::string &n : rec.missing) if (!absent && (n.size() < 5 || n.compare(n.size() - 5, 5, "/tris"))) absent = lacks(n.c_str());
	if (absent) return HT_ERR_IO;
	ht_model_dev &m = ctx->model;
	memset(&m, 0, sizeof m); m.nb = nb; m.nj = nj;
	const float *P = rec.physics.data();
	ht_physics_dev &phys = ctx->phys;
	phys.deltaT = P[0]; phys.restitution = P[1]; phys.gravity_len = sqrtf((P[2] * P[2] + P[3] * P[3]) + P[4] * P[4]); phys.coloumb = P[5]; phys.biasfactorjoint = P[6]; phys.biasfactorpositive = P[7];
	phys.falltime_to_ballistic = P[9]; phys.driftmax = P[10];
	phys.cos40d = cos((double)(40.0f * 3.14f / 180.0f));      // handtrack.h:437 (cos resolves to the double overload there)
	phys.cos40 = (float)phys.cos40d;
	phys.jiggle_sin = sinf(3.14f / 180.0f * (4.0f) / 2.0f);    // gjk.h:626-628
	const float physics_damping = P[11];
	for (int b = 0; b < nb; b++)
	{
		m.vert_off[b] = rec.vert_off[b]; m.plane_off[b] = rec.plane_off[b];
		rec.bodyc[(size_t)b * HT_BC + HT_BC_DAMPLEFT] = powf((1.0f - (rec.damping[b] < physics_damping ? physics_damping : rec.damping[b])), phys.deltaT);      // physics.h:506
		m.collide[b] = rec.collide[b];
		unsigned mask = 0; for (int j = 0; j < nb; j++) if (rec.ignore[b * nb + j]) mask |= 1u << j;
		m.ignore[b] = mask;
	}
	m.vert_off[nb] = rec.vert_off[nb]; m.plane_off[nb] = rec.plane_off[nb];
	// HandModelEnhancements' one-time rewrite (handtrack.h:408-416): a model whose bone 2 (the thumb base) ignores fewer than 10 bodies gets that
	// bone out of every collision pair.  The reference does it on the first call, which precedes every solve with collisions (:684-685, :773-779,
	// :798), so doing it at load gives the same pairs.  The list length counts duplicates there; a baked file without "ignore_count" falls back
	// to the number of distinct bodies.
	if (nb > 2)
	{
		int n2 = 0;
		if (!rec.ignore_count.empty()) n2 = rec.ignore_count[2]; else for (int j = 0; j < nb; j++) n2 += (m.ignore[2] >> j) & 1u;
		if (n2 < 10)
		{
			m.ignore[2] = 0;
			for (int j = 0; j < nb; j++) if (j != 2) { m.ignore[2] |= 1u << j; m.ignore[j] |= 1u << 2; }
		}
	}
	{   // unibody cube: f = mass massinv radius damping friction gravscale com3 tensorinv9
		const float *u = rec.ub_f.data();
		m.ub_massinv = u[1];
		m.ub_dampleft = powf((1.0f - (u[3] < physics_damping ? physics_damping : u[3])), phys.deltaT);
		for (int i = 0; i < 3; i++) m.ub_com[i] = u[6 + i];
		for (int i = 0; i < 9; i++) m.ub_tinv[i] = u[9 + i];
	}
	{ const int r = model_to_device(ctx); if (r) return r; }
	// the limits of the joint coordinates, with the host's sinf, once (ht_joints.hip)
	std::vector<float> jl((size_t)nj * HT_JL, 0.0f);
	ht_joint_limits(rec.jointc.data(), nj, jl.data());
	return dev_put(ctx, &ctx->d_jointl, jl.data(), jl.size());
}

static void sync_params(ht_ctx *ctx)
{
	ctx->phys.iterations = ctx->par.physics_iterations; ctx->phys.iterations_post = ctx->par.physics_iterations_post; ctx->phys.use_collision = ctx->par.physics_use_collision;
	ctx->phys.weak_force = ctx->par.physics_weak_force; ctx->phys.bone_sum_error_scale = ctx->par.bone_sum_error_scale; ctx->phys.unibody_force = ctx->par.unibody_force;
}

extern "C" int ht_create(const char *model_path, int max_batch, int device, ht_ctx **out)
{
	if (!out || max_batch < 1) return HT_ERR_ARG;
	ht_ctx *ctx = new ht_ctx();
	*out = ctx;      // returned even on failure so that ht_last_error can be read; caller destroys it
	ctx->B = max_batch; ctx->device = device;
	default_params(ctx->par);
	int ndev = 0;
	if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) { ctx->err = "no HIP device: the MI355X hot path has no CPU fallback"; return HT_ERR_HIP; }
	if (device < 0 || device >= ndev) { ctx->err = "no such HIP device"; return HT_ERR_ARG; }
	ht_device_guard dev_guard_(device);      // the caller's current device is restored on return
	hipDeviceProp_t prop;
	HIPCHK(ctx, hipGetDeviceProperties(&prop, device));
	if (!strstr(prop.gcnArchName, "gfx950")) { ctx->err = std::string("device is ") + prop.gcnArchName + ", kernels are built for gfx950 only"; return HT_ERR_HIP; }
	HIPCHK(ctx, hipStreamCreate(&ctx->stream));
	for (int i = 0; i < 2; i++) { HIPCHK(ctx, hipStreamCreateWithFlags(&ctx->side[i], hipStreamNonBlocking)); HIPCHK(ctx, ht_edge_event(ctx, &ctx->ev_join[i])); }
	HIPCHK(ctx, ht_edge_event(ctx, &ctx->ev_fork));
	HIPCHK(ctx, ht_edge_event(ctx, &ctx->ev_lap));
	// model_path == NULL: a context that only evaluates / trains the CNN (what a stand-alone CNN object of the reference is, cnn.h:100-605)
	int r = model_path ? load_model(ctx, model_path) : HT_OK;
	if (r) return r;
	ctx->cnn_only = model_path == nullptr;
	sync_params(ctx);
	r = ht_alloc_buffers(ctx);
	if (r) return r;
	ctx->ready = true;
	return HT_OK;
}
extern "C" int ht_model_bake(const char *json_path, const char *out_path, int flags)
{
	if (!json_path || !out_path) return HT_ERR_ARG;
	fx_map fx; std::string err;
	if (!ht_build_model(json_path, flags, fx, err)) { fprintf(stderr, "ht_model_bake: %s\n", err.c_str()); return HT_ERR_IO; }
	return fx_save(out_path, fx) ? HT_OK : HT_ERR_IO;
}
// HandTracker::load_config (handtrack.h:822-828) = from_json over visit_fields (:549-581).  The reference's decoder assigns every listed
// field from the file, and a member that is missing (or is not a number) reads as 0 (json.h:104,140,145); a missing file changes nothing.
extern "C" int ht_config_read(const char *jsonfile, ht_params *p, float *segment_scale, float *prev_frame_error)
{
	if (!jsonfile || !p) return HT_ERR_ARG;
	{ FILE *fp = fopen(jsonfile, "rb"); if (!fp) return HT_OK; fclose(fp); }
	std::map<std::string, std::string> num; std::string err;
	if (!ht_json_top_level(jsonfile, num, err)) { fprintf(stderr, "ht_config_read: %s\n", err.c_str()); return HT_ERR_IO; }
	auto F = [&](const char *k) -> float { auto it = num.find(k); return it == num.end() ? 0.0f : strtof(it->second.c_str(), nullptr); };       // istringstream >> float
	auto I = [&](const char *k) -> int { auto it = num.find(k); return it == num.end() ? 0 : (int)strtol(it->second.c_str(), nullptr, 10); };    // istringstream >> int
	p->subsample_voxel = I("subsample_voxel"); p->subsample_size = F("subsample_size");
	if (segment_scale) *segment_scale = F("segment_scale");
	p->full_reset_on_error = F("full_reset_on_error"); p->angles_only = I("angles_only") != 0; p->always_take_cnn = I("always_take_cnn"); p->drangey = F("drangey");
	p->boundary_planes = I("boundary_planes"); p->microforce = F("microforce"); p->mainthreadpasses = I("mainthreadpasses"); p->subsample_fraction = I("subsample_fraction");
	p->min_point_num = I("min_point_num"); p->accum_error_threshold = F("accum_error_threshold"); p->cloudforce_max_point = F("cloudforce_max_point"); p->cloudforce_max_sum = F("cloudforce_max_sum");
	p->steps = I("steps"); p->steps_keypoints = I("steps_keypoints"); p->steps_keyangles = I("steps_keyangles"); p->steps_palmangle = I("steps_palmangle"); p->steps_cloudstart = I("steps_cloudstart");
	if (prev_frame_error) *prev_frame_error = F("prev_frame_error");
	p->physics_iterations = I("physics_iterations"); p->physics_iterations_post = I("physics_iterations_post"); p->physics_use_collision = I("physics_use_collision");
	p->physics_weak_force = F("physics_weak_force"); p->steps_unibody = I("steps_unibody"); p->bone_sum_error_scale = F("bone_sum_error_scale"); p->min_cray_prob = F("min_cray_prob");
	p->unibody_force = F("unibody_force");
	return HT_OK;
}
// HandTracker::scale (handtrack.h:591) = PhysModel::scale on both models (physmodel.h:196-219,304-319): geometry, centres of mass, radii and
// joint anchors times s, inverse inertia over s*s, body positions stretched about the wrist.  The caller keeps segment_scale.
extern "C" int ht_scale(ht_ctx *ctx, float s)
{
	CHECK_READY(ctx); CHECK_MODEL(ctx);
	ht_model_rec_scale(ctx->rec, s);
	for (float &o : ctx->kp_feature8) o *= s;      // the built-in keypoint tables follow the model (HT_KP_SKELETON is read off the record's anchors and centres of mass)
	{ const int r = model_to_device(ctx); if (r) return r; }
	for (int w = 0; w < 2; w++) ht_launch_scale_state(ctx->d_state[w], ctx->model.nb, ctx->B, s, ctx->stream);
	return ht_sync_check(ctx, ctx->stream);
}
// Training on the weights held by the context; ht_cnn_get_weights reads them back in .cnnb order (CNN::saveb cnn.h:591-593).  Two step implementations, chosen by
// the entry point: CNN::Train (cnn.h:558-580), one SGD step per sample in the order given (train-cnn.cpp:156-162 calls it with alpha = 0.001; ht_train.hip), and
// mini-batch steps w' = w - alpha * sum_b g_b(w) (ht_train_batch.hip).  `batched` says which; the per-sample forms are checked as steps of batch = 1.  The mini-batch
// step trains either net (the *_sized entry points: ht_net_of), the per-sample step the 64x64-input net only.  Every implementation below takes the net and refuses
// a null one (ht_net_of has said why).  The arguments are checked completely before an arena or the staging buffer grows or anything is launched.
static int cnn_train_check(ht_ctx *ctx, const char *fn, bool batched, const ht_net *net, const void *in, const void *tg, int n_pool, const int *order, int n_steps, int batch)
{
	const std::string f(fn);
	if (!net) return HT_ERR_ARG;
	if (!net->have && !batched) { ctx->err = net->missing; return HT_ERR_STATE; }
	if (!net->have) { ctx->err = f + net->train_missing; return HT_ERR_ARG; }
	if (batch < 1 || batch > HT_TRAIN_MAX_BATCH) { ctx->err = f + ": batch must be in [1, HT_TRAIN_MAX_BATCH = " + std::to_string(HT_TRAIN_MAX_BATCH) + "]"; return HT_ERR_ARG; }
	if (!in || !tg) { ctx->err = f + ": inputs and targets must not be NULL"; return HT_ERR_ARG; }
	if (n_pool < 1) { ctx->err = f + ": n_pool must be positive"; return HT_ERR_ARG; }
	if (n_steps < 0) { ctx->err = f + ": n_steps must not be negative"; return HT_ERR_ARG; }
	if (!order && (long long)n_steps * batch > n_pool) { ctx->err = f + ": without an order, n_steps * batch must not exceed n_pool"; return HT_ERR_ARG; }
	if (order) for (long long k = 0; k < (long long)n_steps * batch; k++) if (order[k] < 0 || order[k] >= n_pool) { ctx->err = f + ": order[" + std::to_string(k) + "] is outside [0, n_pool)"; return HT_ERR_ARG; }
	return HT_OK;
}
// The steps on device pools over n_samples indices (order, or 0, 1, ...), checked by the caller.  Per sample: step k trains on index k; the training arena ends with
// a sink for the per-step MSE when the caller asks for none.  Batched: steps of `batch` indices, the last step takes what is left.  Then, once, the forward
// kernels' packed copy of the trained net's last layer follows the trained weights.
static int cnn_train_steps(ht_ctx *ctx, bool batched, ht_net &net, const float *d_x, const float *d_t, const int *order, int n_samples, int batch, float alpha, float *d_mse, hipStream_t s)
{
	float *w = net.d_weights, *W2p = w + net.dims.count;
	if (!batched)
	{
		const size_t na = ht_train_act_floats(), ne = ht_train_err_floats(), np = ht_train_part_floats();
		if (!ctx->d_train) { int r = dev_alloc(ctx, &ctx->d_train, na + ne + np + 16); if (r) return r; }
		float *sink = ctx->d_train + na + ne + np;
		for (int k = 0; k < n_samples; k++)
		{
			const size_t i = order ? (size_t)order[k] : (size_t)k;
			ht_launch_train_step(w, W2p, d_x + i * net.dims.in, d_t + i * HT_CNN_OUT, alpha, ctx->d_train, ctx->d_train + na, ctx->d_train + na + ne, d_mse ? d_mse + k : sink, s);
		}
	}
	else
	{
		const int cap = (batch + 31) & ~31;
		{ const int r = dev_grow(ctx, &net.train.buf, &net.train.cap, (size_t)cap, ht_train_batch_floats(cap, net.dims) / (size_t)cap + 1); if (r) return r; }
		int index[HT_TRAIN_MAX_BATCH];
		for (int k = 0; k < n_samples; k += batch)
		{
			const int n = n_samples - k < batch ? n_samples - k : batch;
			for (int b = 0; b < n; b++) index[b] = order ? order[k + b] : k + b;
			ht_launch_train_batch_step(w, W2p, d_x, d_t, index, n, alpha, net.train.buf, net.train.cap, d_mse ? d_mse + k : nullptr, s, net.dims);
			net.train.last = n;
		}
	}
	ht_launch_pack_w4(net.w.W4, W2p + 16384, s);
	HIPCHK(ctx, hipGetLastError());
	return HT_OK;
}
// the device-pool forms: asynchronous on the caller's stream
static int cnn_train_dev(ht_ctx *ctx, const char *fn, bool batched, ht_net *net, const float *d_inputs, const float *d_targets, int n_pool, const int *order, int n_steps, int batch, float alpha, float *d_mse, void *stream)
{
	{ const int r = cnn_train_check(ctx, fn, batched, net, d_inputs, d_targets, n_pool, order, n_steps, batch); if (r) return r; }
	if (n_steps == 0) return HT_OK;
	return cnn_train_steps(ctx, batched, *net, d_inputs, d_targets, order, n_steps * batch, batch, alpha, d_mse, ht_user_stream(ctx, stream));
}
// the host-array forms: the n samples staged through the context's buffer (ht_staged_call), then the same steps in order on the context's stream
static int cnn_train_host(ht_ctx *ctx, const char *fn, bool batched, ht_net *net, const float *inputs, const float *targets, int n, int batch, float alpha, float *mse_out)
{
	{ const int r = cnn_train_check(ctx, fn, batched, net, inputs, targets, n, nullptr, 0, batch); if (r) return r; }
	ht_seg seg[3] = { { (void *)inputs, (size_t)n * net->dims.in * sizeof(float), false }, { (void *)targets, (size_t)n * HT_CNN_OUT * sizeof(float), false }, { mse_out, (size_t)n * sizeof(float), true } };
	return ht_staged_call(ctx, seg, 3, [&](hipStream_t s)
	                      { return cnn_train_steps(ctx, batched, *net, (const float *)seg[0].dev, (const float *)seg[1].dev, nullptr, n, batch, alpha, (float *)seg[2].dev, s); });
}
// Test aid: the per-sample tensors of the latest mini-batch step of a net (layout: ht_train_batch_views, csrc/ht_train_batch.hip)
static int cnn_train_batch_buffers(ht_ctx *ctx, const char *fn, ht_net *net, int n, float *a3, float *a6, float *a8, float *e9, float *e7, float *e6, float *e3)
{
	const std::string f(fn);
	float *const out[7] = { a3, a6, a8, e9, e7, e6, e3 };
	if (!net) return HT_ERR_ARG;
	for (int i = 0; i < 7; i++) if (!out[i]) { ctx->err = f + ": NULL output"; return HT_ERR_ARG; }
	if (!net->train.buf || net->train.last < 1) { ctx->err = f + ": no mini-batch step has run"; return HT_ERR_STATE; }
	if (n != net->train.last) { ctx->err = f + ": n must be the latest step's sample count, " + std::to_string(net->train.last); return HT_ERR_ARG; }
	HIPCHK(ctx, ht_sync_all(ctx));
	const float *view[7]; size_t per[7];
	ht_train_batch_views(net->train.buf, net->train.cap, view, per, net->dims);
	for (int i = 0; i < 7; i++) HIPCHK(ctx, hipMemcpy(out[i], view[i], (size_t)n * per[i] * sizeof(float), hipMemcpyDeviceToHost));
	return HT_OK;
}
static int cnn_get_weights(ht_ctx *ctx, const ht_net *net, float *w, size_t n)
{
	if (!net || !w) return HT_ERR_ARG;
	if (!net->have) { ctx->err = "no weights to read"; return HT_ERR_STATE; }
	if (n != net->dims.count) { ctx->err = net->bad_count; return HT_ERR_ARG; }
	HIPCHK(ctx, ht_sync_all(ctx));      // also a ht_cnn_train_dev on a caller's stream
	HIPCHK(ctx, hipMemcpy(w, net->d_weights, n * sizeof(float), hipMemcpyDeviceToHost));
	return HT_OK;
}
// The exports.  The unsized forms are the 64x64-input net's; a sized form takes the net of its side (side = 128: the larger net's weights, pools of [..][16384] inputs
// and an arena of its own) and at side 64 is the unsized form, whose name its messages then carry (ht_form_name).
extern "C" int ht_cnn_train_dev(ht_ctx *ctx, const float *d_inputs, const float *d_targets, int n_pool, const int *order, int n_steps, float alpha, float *d_mse, void *stream)
{
	CHECK_READY(ctx);
	return cnn_train_dev(ctx, "ht_cnn_train_dev", false, ht_net_of(ctx, 64), d_inputs, d_targets, n_pool, order, n_steps, 1, alpha, d_mse, stream);
}
extern "C" int ht_cnn_train(ht_ctx *ctx, const float *inputs, const float *targets, int n, float alpha, float *mse_out)
{
	CHECK_READY(ctx);
	return cnn_train_host(ctx, "ht_cnn_train", false, ht_net_of(ctx, 64), inputs, targets, n, 1, alpha, mse_out);
}
extern "C" int ht_cnn_train_batch_dev(ht_ctx *ctx, const float *d_inputs, const float *d_targets, int n_pool, const int *order, int n_steps, int batch, float alpha, float *d_mse, void *stream)
{
	CHECK_READY(ctx);
	return cnn_train_dev(ctx, "ht_cnn_train_batch_dev", true, ht_net_of(ctx, 64), d_inputs, d_targets, n_pool, order, n_steps, batch, alpha, d_mse, stream);
}
extern "C" int ht_cnn_train_batch(ht_ctx *ctx, const float *inputs, const float *targets, int n, int batch, float alpha, float *mse_out)
{
	CHECK_READY(ctx);
	return cnn_train_host(ctx, "ht_cnn_train_batch", true, ht_net_of(ctx, 64), inputs, targets, n, batch, alpha, mse_out);
}
extern "C" int ht_debug_train_batch_buffers(ht_ctx *ctx, int n, float *a3, float *a6, float *a8, float *e9, float *e7, float *e6, float *e3)
{
	CHECK_READY(ctx);
	return cnn_train_batch_buffers(ctx, "ht_debug_train_batch_buffers", ht_net_of(ctx, 64), n, a3, a6, a8, e9, e7, e6, e3);
}
extern "C" int ht_cnn_get_weights(ht_ctx *ctx, float *w, size_t n) { CHECK_READY(ctx); return cnn_get_weights(ctx, ht_net_of(ctx, 64), w, n); }
extern "C" int ht_cnn_train_batch_sized_dev(ht_ctx *ctx, int side, const float *d_inputs, const float *d_targets, int n_pool, const int *order, int n_steps, int batch, float alpha, float *d_mse, void *stream)
{
	CHECK_READY(ctx);
	ht_net *net = ht_net_of(ctx, side);
	return cnn_train_dev(ctx, ht_form_name(ctx, net, "ht_cnn_train_batch_dev", "ht_cnn_train_batch_sized_dev"), true, net, d_inputs, d_targets, n_pool, order, n_steps, batch, alpha, d_mse, stream);
}
extern "C" int ht_cnn_train_batch_sized(ht_ctx *ctx, int side, const float *inputs, const float *targets, int n, int batch, float alpha, float *mse_out)
{
	CHECK_READY(ctx);
	ht_net *net = ht_net_of(ctx, side);
	return cnn_train_host(ctx, ht_form_name(ctx, net, "ht_cnn_train_batch", "ht_cnn_train_batch_sized"), true, net, inputs, targets, n, batch, alpha, mse_out);
}
extern "C" int ht_debug_train_batch_buffers_sized(ht_ctx *ctx, int side, int n, float *a3, float *a6, float *a8, float *e9, float *e7, float *e6, float *e3)
{
	CHECK_READY(ctx);
	ht_net *net = ht_net_of(ctx, side);
	return cnn_train_batch_buffers(ctx, ht_form_name(ctx, net, "ht_debug_train_batch_buffers", "ht_debug_train_batch_buffers_sized"), net, n, a3, a6, a8, e9, e7, e6, e3);
}
extern "C" int ht_cnn_get_weights_sized(ht_ctx *ctx, int side, float *w, size_t n) { CHECK_READY(ctx); return cnn_get_weights(ctx, ht_net_of(ctx, side), w, n); }

// ---- the gradient as a buffer, and the optimiser steps over it (ht_optim.hip) ----
// G = (accumulate ? G : 0) + SUM_b g_b(w) of the samples index[0..n) (null: 0, 1, ...) of the pools; the arguments have been checked (cnn_grad_check).  G comes with the
// first call, the arena grows as it does for a step.
static int cnn_grad_check(ht_ctx *ctx, const char *fn, const ht_net *net, const void *in, const void *tg, int n_pool, const int *order, int calls, int batch, int accumulate)
{
	{ const int r = cnn_train_check(ctx, fn, true, net, in, tg, n_pool, order, calls, batch); if (r) return r; }
	if (accumulate && !net->opt.G) { ctx->err = std::string(fn) + ": accumulate needs a gradient buffer, which the first call without it makes"; return HT_ERR_STATE; }
	return HT_OK;
}
static int cnn_grad_launch(ht_ctx *ctx, ht_net &net, const float *d_x, const float *d_t, const int *order, int n, int accumulate, float *d_mse, hipStream_t s)
{
	if (!net.opt.G) { const int r = dev_alloc(ctx, &net.opt.G, net.dims.count); if (r) return r; }
	const int cap = (n + 31) & ~31;
	{ const int r = dev_grow(ctx, &net.train.buf, &net.train.cap, (size_t)cap, ht_train_batch_floats(cap, net.dims) / (size_t)cap + 1); if (r) return r; }
	int index[HT_TRAIN_MAX_BATCH];
	for (int b = 0; b < n; b++) index[b] = order ? order[b] : b;
	ht_launch_train_batch_grad(net.d_weights, net.opt.G, accumulate ? 1 : 0, d_x, d_t, index, n, net.train.buf, net.train.cap, d_mse, s, net.dims);
	net.train.last = n;
	HIPCHK(ctx, hipGetLastError());
	return HT_OK;
}
extern "C" int ht_cnn_grad_batch_sized_dev(ht_ctx *ctx, int side, const float *d_inputs, const float *d_targets, int n_pool, const int *order, int batch, int accumulate, float *d_mse, void *stream)
{
	CHECK_READY(ctx);
	ht_net *net = ht_net_of(ctx, side);
	{ const int r = cnn_grad_check(ctx, "ht_cnn_grad_batch_sized_dev", net, d_inputs, d_targets, n_pool, order, 1, batch, accumulate); if (r) return r; }
	return cnn_grad_launch(ctx, *net, d_inputs, d_targets, order, batch, accumulate, d_mse, ht_user_stream(ctx, stream));
}
extern "C" int ht_cnn_grad_batch_sized(ht_ctx *ctx, int side, const float *inputs, const float *targets, int n, int accumulate, float *mse_out)
{
	CHECK_READY(ctx);
	ht_net *net = ht_net_of(ctx, side);
	{ const int r = cnn_grad_check(ctx, "ht_cnn_grad_batch_sized", net, inputs, targets, n, nullptr, 1, n, accumulate); if (r) return r; }
	ht_seg seg[3] = { { (void *)inputs, (size_t)n * net->dims.in * sizeof(float), false }, { (void *)targets, (size_t)n * HT_CNN_OUT * sizeof(float), false }, { mse_out, (size_t)n * sizeof(float), true } };
	return ht_staged_call(ctx, seg, 3, [&](hipStream_t s)
	                      { return cnn_grad_launch(ctx, *net, (const float *)seg[0].dev, (const float *)seg[1].dev, nullptr, n, accumulate, (float *)seg[2].dev, s); });
}
// a float array of the net's size on the device (G, m or v), host <-> device: the length every such call checks, and the upload
static int opt_array_check(ht_ctx *ctx, const char *fn, const ht_net *net, size_t n)
{
	if (!net) return HT_ERR_ARG;
	if (n != net->dims.count) { ctx->err = std::string(fn) + ": n must be the net's value count (HT_CNNB_COUNT / HT_CNNB128_COUNT)"; return HT_ERR_ARG; }
	return HT_OK;
}
static int opt_array_set(ht_ctx *ctx, const ht_net &net, float **d, const float *host)      // allocates on first need; host null: zeros
{
	float *fresh = nullptr;
	if (!*d) { const int r = dev_alloc(ctx, &fresh, net.dims.count); if (r) return r; }
	float *p = *d ? *d : fresh;
	const hipError_t e = host ? hipMemcpy(p, host, net.dims.count * sizeof(float), hipMemcpyHostToDevice) : hipMemset(p, 0, net.dims.count * sizeof(float));
	if (e != hipSuccess) { if (fresh) drop_alloc(ctx, fresh); ctx->err = std::string("optimiser state upload: ") + hipGetErrorString(e); return HT_ERR_HIP; }
	*d = p;
	return HT_OK;
}
extern "C" int ht_cnn_grad_get_sized(ht_ctx *ctx, int side, float *g, size_t n)
{
	CHECK_READY(ctx);
	ht_net *net = ht_net_of(ctx, side);
	if (!net || !g) return HT_ERR_ARG;
	{ const int r = opt_array_check(ctx, "ht_cnn_grad_get_sized", net, n); if (r) return r; }
	if (!net->opt.G) { ctx->err = "ht_cnn_grad_get_sized: no gradient buffer yet (ht_cnn_grad_batch_sized, ht_cnn_grad_set_sized)"; return HT_ERR_STATE; }
	HIPCHK(ctx, ht_sync_all(ctx));
	HIPCHK(ctx, hipMemcpy(g, net->opt.G, n * sizeof(float), hipMemcpyDeviceToHost));
	return HT_OK;
}
extern "C" int ht_cnn_grad_set_sized(ht_ctx *ctx, int side, const float *g, size_t n)
{
	CHECK_READY(ctx);
	ht_net *net = ht_net_of(ctx, side);
	if (!net || !g) return HT_ERR_ARG;
	{ const int r = opt_array_check(ctx, "ht_cnn_grad_set_sized", net, n); if (r) return r; }
	HIPCHK(ctx, ht_sync_all(ctx));
	return opt_array_set(ctx, *net, &net->opt.G, g);
}
extern "C" int ht_cnn_grad_ptr_sized(ht_ctx *ctx, int side, float **d_g, size_t *n)
{
	CHECK_READY(ctx);
	ht_net *net = ht_net_of(ctx, side);
	if (!net || !d_g) return HT_ERR_ARG;
	if (!net->opt.G) { ctx->err = "ht_cnn_grad_ptr_sized: no gradient buffer yet (ht_cnn_grad_batch_sized, ht_cnn_grad_set_sized)"; return HT_ERR_STATE; }
	*d_g = net->opt.G;
	if (n) *n = net->dims.count;
	return HT_OK;
}
extern "C" int ht_opt_default(int kind, ht_opt *o)
{
	if (!o || kind < HT_OPT_SGD || kind > HT_OPT_ADAM) return HT_ERR_ARG;
	o->kind = kind; o->lr = 0.001f; o->momentum = 0.9f; o->beta1 = 0.9f; o->beta2 = 0.999f; o->eps = 1e-8f; o->weight_decay = 0.0f; o->decoupled_decay = 0;
	o->grad_scale = 1.0f; o->clip_norm = 0.0f;
	return HT_OK;
}
// every field of an ht_opt, before anything is allocated or launched; the message names the field
static int opt_check(ht_ctx *ctx, const char *fn, const ht_opt *o)
{
	const char *bad = nullptr;
	auto unit = [](float x) { return x >= 0.0f && x < 1.0f; };      // false for NaN
	if (!o) bad = "the options must not be NULL";
	else if (o->kind < HT_OPT_SGD || o->kind > HT_OPT_ADAM) bad = "kind must be HT_OPT_SGD, _MOMENTUM, _NESTEROV or _ADAM";
	else if (!(std::isfinite(o->lr) && o->lr >= 0.0f)) bad = "lr must be finite and not negative";
	else if (!unit(o->momentum)) bad = "momentum must be in [0, 1)";
	else if (!unit(o->beta1)) bad = "beta1 must be in [0, 1)";
	else if (!unit(o->beta2)) bad = "beta2 must be in [0, 1)";
	else if (!std::isfinite(o->eps) || (o->kind == HT_OPT_ADAM && !(o->eps > 0.0f))) bad = "eps must be finite, and positive for HT_OPT_ADAM";
	else if (!std::isfinite(o->weight_decay)) bad = "weight_decay must be finite";
	else if (o->decoupled_decay != 0 && o->decoupled_decay != 1) bad = "decoupled_decay must be 0 or 1";
	else if (o->decoupled_decay && o->kind != HT_OPT_ADAM) bad = "decoupled_decay is HT_OPT_ADAM's; the other kinds take weight_decay coupled";
	else if (!std::isfinite(o->grad_scale)) bad = "grad_scale must be finite";
	else if (!(std::isfinite(o->clip_norm) && o->clip_norm >= 0.0f)) bad = "clip_norm must be finite and not negative (0 = off)";
	if (bad) { ctx->err = std::string(fn) + ": " + bad; return HT_ERR_ARG; }
	return HT_OK;
}
static int opt_net_check(ht_ctx *ctx, const char *fn, const ht_net *net)
{
	if (!net) return HT_ERR_ARG;
	if (!net->have) { ctx->err = std::string(fn) + net->train_missing; return HT_ERR_ARG; }
	return HT_OK;
}
// One step of the optimiser o (checked: opt_check) over all weights of the net from its G: the norm and the factor when clipping, the step, the packed copies
static int cnn_opt_launch(ht_ctx *ctx, ht_net &net, const ht_opt &o, hipStream_t s)
{
	const size_t n = net.dims.count;
	if (o.kind != HT_OPT_SGD && !net.opt.m) { const int r = opt_array_set(ctx, net, &net.opt.m, nullptr); if (r) return r; }
	if (o.kind == HT_OPT_ADAM && !net.opt.v) { const int r = opt_array_set(ctx, net, &net.opt.v, nullptr); if (r) return r; }
	if (!net.opt.stat) { const int r = dev_alloc(ctx, &net.opt.stat, ht_opt_stat_doubles()); if (r) return r; }
	ht_opt_args a = {};
	a.lr = o.lr; a.momentum = o.momentum; a.beta1 = o.beta1; a.beta2 = o.beta2; a.eps = o.eps; a.wd = o.weight_decay; a.gs = o.grad_scale;
	a.omb1 = 1.0f - o.beta1; a.omb2 = 1.0f - o.beta2; a.bc1 = a.bc2 = 1.0f;
	a.coupled = !o.decoupled_decay && o.weight_decay != 0.0f; a.decoupled = o.decoupled_decay != 0;
	if (o.kind == HT_OPT_ADAM)
	{
		const int t = ++net.opt.t;
		a.bc1 = (float)(1.0 - pow((double)o.beta1, (double)t)); a.bc2 = (float)(1.0 - pow((double)o.beta2, (double)t));
	}
	{
		const cnnb_layout<float> L = cnnb_layout_of(net.d_weights, net.dims.act2);
		float *const at[8] = { L.W1, L.B1, L.W2, L.B2, L.W3, L.B3, L.W4, L.B4 };
		for (int k = 0; k < 8; k++) a.r[k] = (unsigned)(at[k] - net.d_weights);
	}
	const bool clip = o.clip_norm > 0.0f;
	if (clip) ht_launch_opt_norm(net.opt.G, n, o.grad_scale, o.clip_norm, net.opt.stat, s);
	ht_launch_opt_step(o.kind, net.d_weights, net.opt.G, net.opt.m, net.opt.v, n, clip ? reinterpret_cast<const float *>(net.opt.stat + 1) : nullptr, a, s);
	ht_launch_opt_pack_w2(cnnb_layout_of(net.d_weights, net.dims.act2).W2, net.d_weights + n, s);
	ht_launch_pack_w4(net.w.W4, net.d_weights + n + 16384, s);
	net.opt.clipped = clip; net.opt.steps++;
	HIPCHK(ctx, hipGetLastError());
	return HT_OK;
}
extern "C" int ht_cnn_opt_step_sized_dev(ht_ctx *ctx, int side, const ht_opt *o, void *stream)
{
	CHECK_READY(ctx);
	ht_net *net = ht_net_of(ctx, side);
	{ int r = opt_net_check(ctx, "ht_cnn_opt_step_sized_dev", net); if (r || (r = opt_check(ctx, "ht_cnn_opt_step_sized_dev", o))) return r; }
	if (!net->opt.G) { ctx->err = "ht_cnn_opt_step_sized_dev: no gradient buffer yet (ht_cnn_grad_batch_sized, ht_cnn_grad_set_sized)"; return HT_ERR_STATE; }
	return cnn_opt_launch(ctx, *net, *o, ht_user_stream(ctx, stream));
}
extern "C" int ht_cnn_opt_reset_sized(ht_ctx *ctx, int side)
{
	CHECK_READY(ctx);
	ht_net *net = ht_net_of(ctx, side);
	if (!net) return HT_ERR_ARG;
	HIPCHK(ctx, ht_sync_all(ctx));
	if (net->opt.m) HIPCHK(ctx, hipMemset(net->opt.m, 0, net->dims.count * sizeof(float)));
	if (net->opt.v) HIPCHK(ctx, hipMemset(net->opt.v, 0, net->dims.count * sizeof(float)));
	net->opt.t = 0;
	return HT_OK;
}
extern "C" int ht_cnn_opt_state_get_sized(ht_ctx *ctx, int side, float *m, float *v, size_t n, int *t)
{
	CHECK_READY(ctx);
	ht_net *net = ht_net_of(ctx, side);
	if (!net) return HT_ERR_ARG;
	if (m || v) { const int r = opt_array_check(ctx, "ht_cnn_opt_state_get_sized", net, n); if (r) return r; }
	HIPCHK(ctx, ht_sync_all(ctx));
	float *const host[2] = { m, v }, *const dev[2] = { net->opt.m, net->opt.v };
	for (int k = 0; k < 2; k++)      // a moment no step has needed yet is all zeros
		if (host[k]) { if (dev[k]) HIPCHK(ctx, hipMemcpy(host[k], dev[k], n * sizeof(float), hipMemcpyDeviceToHost)); else memset(host[k], 0, n * sizeof(float)); }
	if (t) *t = net->opt.t;
	return HT_OK;
}
extern "C" int ht_cnn_opt_state_set_sized(ht_ctx *ctx, int side, const float *m, const float *v, size_t n, int t)
{
	CHECK_READY(ctx);
	ht_net *net = ht_net_of(ctx, side);
	if (!net) return HT_ERR_ARG;
	if (m || v) { const int r = opt_array_check(ctx, "ht_cnn_opt_state_set_sized", net, n); if (r) return r; }
	if (t < 0) { ctx->err = "ht_cnn_opt_state_set_sized: t must not be negative"; return HT_ERR_ARG; }
	HIPCHK(ctx, ht_sync_all(ctx));
	if (m) { const int r = opt_array_set(ctx, *net, &net->opt.m, m); if (r) return r; }
	if (v) { const int r = opt_array_set(ctx, *net, &net->opt.v, v); if (r) return r; }
	net->opt.t = t;
	return HT_OK;
}
extern "C" int ht_cnn_opt_last_sized(ht_ctx *ctx, int side, double *grad_norm, float *clip_factor)
{
	CHECK_READY(ctx);
	ht_net *net = ht_net_of(ctx, side);
	if (!net) return HT_ERR_ARG;
	if (!net->opt.steps) { ctx->err = "ht_cnn_opt_last_sized: no optimiser step has run on this net"; return HT_ERR_STATE; }
	HIPCHK(ctx, ht_sync_all(ctx));
	double st[2] = { -1.0, 0.0 }; float c = 1.0f;      // a step that did not clip formed no norm: -1 and 1.0f
	if (net->opt.clipped) { HIPCHK(ctx, hipMemcpy(st, net->opt.stat, sizeof st, hipMemcpyDeviceToHost)); memcpy(&c, &st[1], sizeof c); }
	if (grad_norm) *grad_norm = st[0];
	if (clip_factor) *clip_factor = c;
	return HT_OK;
}
// n_steps optimiser steps, each after accum gradient calls of `batch` samples (the first with accumulate = 0): the calls above in that order, nothing else
extern "C" int ht_cnn_train_opt_sized_dev(ht_ctx *ctx, int side, const float *d_inputs, const float *d_targets, int n_pool, const int *order, int n_steps, int batch, int accum, const ht_opt *o, float *d_mse, void *stream)
{
	CHECK_READY(ctx);
	const char *fn = "ht_cnn_train_opt_sized_dev";
	ht_net *net = ht_net_of(ctx, side);
	if (!net) return HT_ERR_ARG;
	if (accum < 1) { ctx->err = std::string(fn) + ": accum must be at least 1"; return HT_ERR_ARG; }
	if (n_steps < 0 || (long long)n_steps * accum > INT_MAX / HT_TRAIN_MAX_BATCH) { ctx->err = std::string(fn) + ": n_steps must not be negative, n_steps * accum * batch must fit an int"; return HT_ERR_ARG; }
	{ int r = cnn_grad_check(ctx, fn, net, d_inputs, d_targets, n_pool, order, n_steps * accum, batch, 0); if (r || (r = opt_check(ctx, fn, o))) return r; }
	hipStream_t s = ht_user_stream(ctx, stream);
	size_t k = 0;
	for (int i = 0; i < n_steps; i++)
	{
		for (int j = 0; j < accum; j++, k += (size_t)batch)
		{
			int index[HT_TRAIN_MAX_BATCH];
			for (int b = 0; b < batch; b++) index[b] = order ? order[k + b] : (int)k + b;
			const int r = cnn_grad_launch(ctx, *net, d_inputs, d_targets, index, batch, j > 0, d_mse ? d_mse + k : nullptr, s);
			if (r) return r;
		}
		const int r = cnn_opt_launch(ctx, *net, *o, s);
		if (r) return r;
	}
	return HT_OK;
}
// Test aid: the layer outputs and the errors of the training arena as the latest step left them (layout: ht_launch_train_step, csrc/ht_train.hip)
extern "C" int ht_debug_train_buffers(ht_ctx *ctx, float *act, size_t n_act, float *err, size_t n_err)
{
	CHECK_READY(ctx);
	if (!act || !err) return HT_ERR_ARG;
	if (n_act != ht_train_act_floats() || n_err != ht_train_err_floats()) { ctx->err = "ht_debug_train_buffers: expected ht_train_act_floats() / ht_train_err_floats() values (74768 / 64272)"; return HT_ERR_ARG; }
	if (!ctx->d_train) { ctx->err = "ht_debug_train_buffers: no training step has run"; return HT_ERR_STATE; }
	HIPCHK(ctx, ht_sync_all(ctx));      // also a ht_cnn_train_dev on a caller's stream
	HIPCHK(ctx, hipMemcpy(act, ctx->d_train, n_act * sizeof(float), hipMemcpyDeviceToHost));
	HIPCHK(ctx, hipMemcpy(err, ctx->d_train + n_act, n_err * sizeof(float), hipMemcpyDeviceToHost));
	return HT_OK;
}
// Label synthesis, host only.  GatherHandExpectedCNN (handtrack.h:160-173): 8 landmark heat-maps (ImageFeaturePoints :92-96, RenderHeatMap /
// NormalizeHeatMap misc_image.h:246-272) and 16 one-dimensional maps of the key angles (HandPoseToKeyAngleSet handtrack.h:132-151,
// Render1DHeatMaps misc_image.h:281-295), as bytes scaled by 1/255.  atan2 / asin / acos / exp / pow without std:: are the C double functions there.
static unsigned char gray_of(float x) { float v = x * 255.0f; v = fmin_std(fmax_std(v, 0.0f), 255.0f); return (unsigned char)v; }
extern "C" int ht_expected_cnn_full(const float *pose, const float *cam, float *expected, float *image_points, float *vals_out);
extern "C" int ht_expected_cnn(const float *pose, const float *cam, float *expected) { return ht_expected_cnn_full(pose, cam, expected, nullptr, nullptr); }
// the same with the other members of the Set the reference returns: image_points [8][2] (ImageFeaturePoints handtrack.h:92-96) and vals [16]
extern "C" int ht_expected_cnn_full(const float *pose, const float *cam, float *expected, float *image_points, float *vals_out)
{
	if (!pose || !cam || !expected) return HT_ERR_ARG;
	static const int fbone[8] = { 1, 1, 1, 4, 7, 10, 13, 16 };
	static const float foff[8][3] = { { 0, 0, 0 }, { -0.03f, 0, -0.03f }, { 0.03f, 0, -0.03f }, { 0, 0, 0 }, { 0, 0, 0 }, { 0, 0, 0 }, { 0, 0, 0 }, { 0, 0, 0 } };
	const float fx = cam[0] / 4.0f, fy = cam[1] / 4.0f, px = cam[2] / 4.0f, py = cam[3] / 4.0f;      // hcam = camsub(cam, 4), 16 x 16
	const xf campose = XF(V3(cam[5], cam[6], cam[7]), V4(cam[8], cam[9], cam[10], cam[11])), ci = inverse(campose);
	auto P = [&](int b) { return XF(V3(pose[7 * b], pose[7 * b + 1], pose[7 * b + 2]), V4(pose[7 * b + 3], pose[7 * b + 4], pose[7 * b + 5], pose[7 * b + 6])); };
	unsigned char img[HT_CNN_OUT];
	memset(img, 0, sizeof img);
	for (int k = 0; k < 8; k++)
	{
		const v3 v = apply(ci, apply(P(fbone[k]), V3(foff[k][0], foff[k][1], foff[k][2])));
		const float ux = v.x / v.z * fx + px, uy = v.y / v.z * fy + py;
		if (image_points) { image_points[2 * k] = ux; image_points[2 * k + 1] = uy; }
		unsigned char *h = img + 256 * k;
		const int hx = (int)ux, hy = (int)uy;
		for (int y = (hy - 2 > 0 ? hy - 2 : 0); y < (hy + 3 < 16 ? hy + 3 : 16); y++) for (int x = (hx - 2 > 0 ? hx - 2 : 0); x < (hx + 3 < 16 ? hx + 3 : 16); x++)
		{
			const float dx = ux - (float)x, dy = uy - (float)y;
			h[y * 16 + x] = gray_of(expf(-(dx * dx + dy * dy) / (2.0f * 0.33f)));
		}
		int sum = 0; for (int i = 0; i < 256; i++) sum += h[i];
		if (sum) for (int i = 0; i < 256; i++) h[i] = (unsigned char)(h[i] * 255 / sum);
	}
	float vals[16]; int nv = 0;
	const v4 q1 = P(1).q, palmq = qmul(ci.q, q1);
	vals[nv++] = (float)(atan2((double)qxdir(palmq).x, (double)-qxdir(palmq).z) / (double)(3.14159f * 2.0f) + (double)0.5f);
	vals[nv++] = (float)(asin((double)clamp_std(qzdir(palmq).z, -1.0f, 1.0f)) / (double)3.14159f + (double)0.5f);
	vals[nv++] = (float)(asin((double)clamp_std(qzdir(palmq).x, -1.0f, 1.0f)) / (double)3.14159f + (double)0.5f);
	vals[nv++] = (float)(acos((double)dot(qxdir(q1), qzdir(P(4).q))) / (double)3.14159f);
	for (int b : { 6, 9, 12, 15 }) vals[nv++] = (float)(acos((double)clamp_std(dot(qydir(q1), qydir(P(b).q)), -1.0f, 1.0f)) / (double)3.14159f);
	{ const v3 pz = qzdir(palmq); vals[nv++] = (float)((double)0.5f + atan2((double)-pz.x, (double)-pz.y) / (double)(3.14159f * 2.0f)); }
	while (nv < 16) vals[nv++] = 0.0f;
	if (vals_out) memcpy(vals_out, vals, sizeof vals);
	unsigned char *vm = img + 2048;
	for (int y = 0; y < 16; y++)
	{
		const float v = vals[y] * (float)(16 - 1);
		const int x0 = ((int)v - 2 > 0 ? (int)v - 2 : 0), x1 = ((int)v + 3 < 16 ? (int)v + 3 : 16);
		int sum = 0;
		for (int x = x0; x < x1; x++) { const float d2 = (float)pow((double)((float)x - v), (double)2.0f); sum += vm[y * 16 + x] = gray_of((float)exp((double)(-d2 / (2.0f * 0.5f)))); }
		for (int x = x0; sum && x < x1; x++) vm[y * 16 + x] = (unsigned char)(vm[y * 16 + x] * 255 / sum);
	}
	for (int i = 0; i < HT_CNN_OUT; i++) expected[i] = img[i] / 255.0f;
	return HT_OK;
}
extern "C" int ht_destroy(ht_ctx *ctx)
{
	if (!ctx) return HT_ERR_ARG;
	ht_device_guard dev_guard_(ctx->device);
	if (ctx->ready) (void)hipDeviceSynchronize();      // nothing of this context may still run when its buffers go
	if (ctx->comm) (void)ht_comm_destroy(ctx);
	for (void *p : ctx->allocs) (void)hipFree(p);
	if (ctx->h_nreset) (void)hipHostFree(const_cast<unsigned *>(ctx->h_nreset));
	for (auto &kv : ctx->prof) for (hipEvent_t e : kv.second.ev) (void)hipEventDestroy(e);
	for (int i = 0; i < 2; i++) { if (ctx->side[i]) (void)hipStreamDestroy(ctx->side[i]); if (ctx->ev_join[i]) (void)hipEventDestroy(ctx->ev_join[i]); }
	if (ctx->ev_fork) (void)hipEventDestroy(ctx->ev_fork);
	if (ctx->ev_lap) (void)hipEventDestroy(ctx->ev_lap);
	if (ctx->ev_job) (void)hipEventDestroy(ctx->ev_job);
	if (ctx->ev_seed) (void)hipEventDestroy(ctx->ev_seed);
	if (ctx->h_job_in) (void)hipHostFree(ctx->h_job_in);
	if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
	delete ctx;
	return HT_OK;
}
extern "C" const char *ht_last_error(const ht_ctx *ctx) { return ctx ? ctx->err.c_str() : "null context"; }
extern "C" int ht_get_params(const ht_ctx *ctx, ht_params *p) { if (!ctx || !p) return HT_ERR_ARG; *p = ctx->par; return HT_OK; }
// The reference takes any value (load_config writes 0 into every field its file omits, handtrack.h:822-828) and then divides by subsample_fraction
// (physmodel.h:58-64) or loops forever; here a configuration the kernels cannot run is refused with a message instead.
extern "C" int ht_set_params(ht_ctx *ctx, const ht_params *p)
{
	if (!ctx || !p) return HT_ERR_ARG;
	const char *bad = nullptr;
	if (p->subsample_fraction < 1) bad = "subsample_fraction must be >= 1";
	else if (!(p->drangey > 0.1f)) bad = "drangey must exceed the near limit 0.1";
	else if (p->steps < 0 || p->steps_keypoints < 0 || p->steps_keyangles < 0 || p->steps_palmangle < 0 || p->steps_cloudstart < 0 || p->steps_unibody < 0) bad = "step counts must be >= 0";
	else if (p->physics_iterations < 0 || p->physics_iterations_post < 0) bad = "physics iteration counts must be >= 0";
	else if (p->mainthreadpasses < 0) bad = "mainthreadpasses must be >= 0";
	else if (p->min_point_num < 0) bad = "min_point_num must be >= 0";
	else if (p->subsample_voxel && !(p->subsample_size > 0.0f)) bad = "subsample_voxel needs a positive subsample_size (the voxel edge in metres)";
	if (bad) { ctx->err = std::string("ht_set_params: ") + bad; return HT_ERR_ARG; }
	ctx->par = *p; sync_params(ctx);
	return HT_OK;
}
extern "C" int ht_model_info(const ht_ctx *ctx, int *nb, int *nj, int *mb) { if (!ctx) return HT_ERR_ARG; if (nb) *nb = ctx->model.nb; if (nj) *nj = ctx->model.nj; if (mb) *mb = ctx->B; return HT_OK; }


// ------------------------------------------------------------------------------------------------- CNN
// The net comes in two input sizes with the same layer list: 64x64 (conv5 -> 60, pool -> 30 -> 15, conv4 -> 12, pool -> 6, FC 2304 -> 2048 -> 2304, chunked softmax) and
// 128x128 (BASELINE configs[4] / SURVEY 8d "config 5 (ii)": conv5 -> 124, pool -> 62 -> 31, conv4 -> 28, pool -> 14, FC 12544 -> 2048 -> 2304).  Each is one ht_net of the
// context (ht_host.hpp); the loader and the forward pass take the net and refuse a null one (ht_net_of has said why).
static int net_alloc_frames(ht_ctx *ctx, ht_net &net)      // the net's input and convolution buffers, for the context's capacity
{
	const size_t B = (size_t)ctx->B;
	int r;
	if ((r = dev_alloc(ctx, &net.d_in, B * net.dims.in)) || (r = dev_alloc(ctx, &net.d_act1, B * net.dims.act1)) || (r = dev_alloc(ctx, &net.d_act2, B * net.dims.act2))) return r;
	return HT_OK;
}
static int cnn_load_weights(ht_ctx *ctx, ht_net *net, const float *w, size_t n)
{
	if (!net) return HT_ERR_ARG;
	if (!w || n != net->dims.count) { ctx->err = net->bad_count; return HT_ERR_ARG; }
	const size_t count = net->dims.count;
	if (!net->d_weights)
	{
		int r;
		if (!net->d_in && (r = net_alloc_frames(ctx, *net))) return r;      // (the larger net's: the 64x64-input net's came with the context)
		if ((r = dev_alloc(ctx, &net->d_weights, count + 16384 + HT_W4_COUNT))) return r;
	}
	float *d = net->d_weights;
	HIPCHK(ctx, hipMemcpy(d, w, n * sizeof(float), hipMemcpyHostToDevice));
	// conv2 weights repacked for the matrix kernel (cnn_w2p_index)
	const float *W2 = cnnb_layout_of(w, net->dims.act2).W2;
	std::vector<float> w2p(16384);
	for (int oc = 0; oc < 64; oc++) for (int ic = 0; ic < 16; ic++) for (int ky = 0; ky < 4; ky++) for (int kx = 0; kx < 4; kx++)
		w2p[cnn_w2p_index(oc, ic, ky, kx)] = W2[kx + 4 * (ky + 4 * (ic + 16 * oc))];
	HIPCHK(ctx, hipMemcpy(d + count, w2p.data(), 16384 * sizeof(float), hipMemcpyHostToDevice));
	ht_cnn_weights &cw = net->w;
	const cnnb_layout<float> L = cnnb_layout_of(d, net->dims.act2);
	cw.W1 = L.W1; cw.B1 = L.B1; cw.W2p = d + count; cw.B2 = L.B2; cw.W3 = L.W3; cw.B3 = L.B3; cw.W4 = L.W4; cw.B4 = L.B4;
	cw.W4p = d + count + 16384;
	ht_launch_pack_w4(cw.W4, d + count + 16384, ctx->stream);
	HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
	net->have = true;
	return HT_OK;
}
static int cnn_forward(ht_ctx *ctx, const ht_net &net, const float *d_in, float *d_out, int B, hipStream_t s)
{
	if (!net.have) { ctx->err = net.missing; return HT_ERR_STATE; }      // (the larger net's buffers come with its weights)
	ht_prof_scope p0(ctx, net.prof, s, true);
	ht_launch_cnn(net, d_in, ctx->d_act3, ctx->d_logits, B, s);
	ht_launch_softmax_decode(ctx->d_logits, d_out, nullptr, nullptr, 1, B, s);
	return HT_OK;
}
static int cnn_eval_dev(ht_ctx *ctx, const ht_net *net, const float *d_in, float *d_out, int B, void *stream)
{
	if (!net || !d_in || !d_out) return HT_ERR_ARG;
	int r = cnn_forward(ctx, *net, d_in, d_out, B, ht_user_stream(ctx, stream));
	if (r) return r;
	HIPCHK(ctx, hipGetLastError());
	return HT_OK;
}
static int cnn_eval(ht_ctx *ctx, const ht_net *net, const float *in, float *out, int B)
{
	if (!net || !in || !out) return HT_ERR_ARG;
	if (!net->have) { ctx->err = net->missing; return HT_ERR_STATE; }
	HIPCHK(ctx, hipMemcpyAsync(net->d_in, in, (size_t)B * net->dims.in * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
	int r = cnn_forward(ctx, *net, net->d_in, ctx->d_cnn_out, B, ctx->stream);
	if (r) return r;
	HIPCHK(ctx, hipMemcpyAsync(out, ctx->d_cnn_out, (size_t)B * HT_CNN_OUT * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
	return ht_sync_check(ctx, ctx->stream);
}
extern "C" int ht_cnn_load_weights(ht_ctx *ctx, const float *w, size_t n) { CHECK_READY(ctx); return cnn_load_weights(ctx, ht_net_of(ctx, 64), w, n); }
extern "C" int ht_cnn_load_weights_sized(ht_ctx *ctx, int side, const float *w, size_t n) { CHECK_READY(ctx); return cnn_load_weights(ctx, ht_net_of(ctx, side), w, n); }
extern "C" int ht_cnn_eval_dev(ht_ctx *ctx, const float *d_in, float *d_out, int B, void *stream) { CHECK_READY(ctx); CHECK_BATCH(ctx, B); return cnn_eval_dev(ctx, ht_net_of(ctx, 64), d_in, d_out, B, stream); }
extern "C" int ht_cnn_eval(ht_ctx *ctx, const float *in, float *out, int B) { CHECK_READY(ctx); CHECK_BATCH(ctx, B); return cnn_eval(ctx, ht_net_of(ctx, 64), in, out, B); }
extern "C" int ht_cnn_eval_sized_dev(ht_ctx *ctx, int side, const float *d_in, float *d_out, int B, void *stream) { CHECK_READY(ctx); CHECK_BATCH(ctx, B); return cnn_eval_dev(ctx, ht_net_of(ctx, side), d_in, d_out, B, stream); }
extern "C" int ht_cnn_eval_sized(ht_ctx *ctx, int side, const float *in, float *out, int B) { CHECK_READY(ctx); CHECK_BATCH(ctx, B); return cnn_eval(ctx, ht_net_of(ctx, side), in, out, B); }

// ------------------------------------------------------------------------------------------------- stage: prepare / decode
extern "C" int ht_stage_prepare(ht_ctx *ctx, const uint16_t *depth, const float *cams, int B, float *cnn_in, float *points, int *npoints)
{
	CHECK_READY(ctx); CHECK_MODEL(ctx); CHECK_BATCH(ctx, B);
	if (!depth || !cams) return HT_ERR_ARG;
	hipStream_t s = ctx->stream; const ht_net &tile = *ht_net_of(ctx, 64);
	HIPCHK(ctx, hipMemcpyAsync(ctx->d_depth, depth, (size_t)B * 4096 * sizeof(uint16_t), hipMemcpyHostToDevice, s));
	HIPCHK(ctx, hipMemcpyAsync(ctx->d_cams, cams, (size_t)B * HT_CAM * sizeof(float), hipMemcpyHostToDevice, s));
	ht_launch_prepare(ctx->d_depth, ctx->d_cams, ctx->par.drangey, ctx->par.subsample_fraction, tile.d_in, ctx->d_pts, ctx->d_npts, ctx->model.pts_cap, B, s);
	ctx->model.pts_bound = 0;      // stage calls: no assumption about the cloud size
	if (cnn_in) HIPCHK(ctx, hipMemcpyAsync(cnn_in, tile.d_in, (size_t)B * tile.dims.in * sizeof(float), hipMemcpyDeviceToHost, s));
	if (points) HIPCHK(ctx, hipMemcpy2DAsync(points, HT_MAXPTS * sizeof(float4), ctx->d_pts, (size_t)ctx->model.pts_cap * sizeof(float4), HT_MAXPTS * sizeof(float4), B, hipMemcpyDeviceToHost, s));
	if (npoints) HIPCHK(ctx, hipMemcpyAsync(npoints, ctx->d_npts, (size_t)B * sizeof(int), hipMemcpyDeviceToHost, s));
	return ht_sync_check(ctx, s);
}
extern "C" int ht_stage_decode(ht_ctx *ctx, const float *cnn_out, const float *cams, int B, float *analysis)
{
	CHECK_READY(ctx); CHECK_BATCH(ctx, B);
	if (!cnn_out || !cams || !analysis) return HT_ERR_ARG;
	hipStream_t s = ctx->stream;
	HIPCHK(ctx, hipMemcpyAsync(ctx->d_cnn_out, cnn_out, (size_t)B * HT_CNN_OUT * sizeof(float), hipMemcpyHostToDevice, s));
	HIPCHK(ctx, hipMemcpyAsync(ctx->d_cams, cams, (size_t)B * HT_CAM * sizeof(float), hipMemcpyHostToDevice, s));
	ht_launch_softmax_decode(nullptr, ctx->d_cnn_out, ctx->d_cams, ctx->d_analysis, 0, B, s);
	HIPCHK(ctx, hipMemcpyAsync(analysis, ctx->d_analysis, (size_t)B * HT_ANALYSIS * sizeof(float), hipMemcpyDeviceToHost, s));
	return ht_sync_check(ctx, s);
}

// ------------------------------------------------------------------------------------------------- profiling hooks
// Each named phase records a pair of HIP events on the stream the kernels run on; pairs are pooled and only resolved in
// ht_profile_read, so enabling the profile adds no host synchronisation to the launch sequence.
ht_prof_scope::ht_prof_scope(ht_ctx *c, const char *name, hipStream_t s, bool minor_phase) : ctx(c), ent(nullptr), stream(s), slot(0)
{
	if (!name || !c->profile || (minor_phase && !c->profile_phases)) return;      // a null name: this scope is not recorded
	auto it = c->prof.find(name);
	if (it == c->prof.end()) { ht_prof_entry e; e.used = 0; e.total_ms = 0; e.launches = 0; it = c->prof.emplace(name, e).first; }
	ht_prof_entry *e = &it->second;
	if (e->used + 2 > e->ev.size())
	{
		hipEvent_t a, b;
		if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) return;
		e->ev.push_back(a); e->ev.push_back(b);
	}
	ent = e; slot = e->used; e->used += 2;
	(void)hipEventRecord(e->ev[slot], s);
}
ht_prof_scope::~ht_prof_scope()
{
	if (!ent) return;
	(void)hipEventRecord(ent->ev[slot + 1], stream);
	ent->launches++;
}
static void prof_resolve(ht_prof_entry &e)
{
	for (size_t i = 0; i + 1 < e.used; i += 2)
	{
		float ms = 0;
		if (hipEventSynchronize(e.ev[i + 1]) == hipSuccess && hipEventElapsedTime(&ms, e.ev[i], e.ev[i + 1]) == hipSuccess) e.total_ms += ms;
	}
	e.used = 0;
}
extern "C" int ht_profile_enable(ht_ctx *ctx, int on) { if (!ctx) return HT_ERR_ARG; ctx->profile = on != 0; ctx->profile_phases = on > 1; return HT_OK; }
extern "C" int ht_profile_read(ht_ctx *ctx, int reset, int max_entries, char *names, int name_stride, float *total_ms, int *launches, int *n_entries)
{
	if (!ctx || !n_entries) return HT_ERR_ARG;
	ht_device_guard dev_guard_(ctx->device);
	int k = 0;
	for (auto &kv : ctx->prof)
	{
		ht_prof_entry &e = kv.second;
		prof_resolve(e);
		if (k < max_entries)
		{
			if (names && name_stride > 0) { strncpy(names + (size_t)k * name_stride, kv.first.c_str(), name_stride - 1); names[(size_t)k * name_stride + name_stride - 1] = 0; }
			if (total_ms) total_ms[k] = e.total_ms;
			if (launches) launches[k] = e.launches;
			k++;
		}
		if (reset) { e.total_ms = 0; e.launches = 0; }
	}
	*n_entries = k;
	return HT_OK;
}

// ------------------------------------------------------------------------------------------------- buffers
// The per-point arrays (points, cloud rows, the solver's row records) hold `pts_cap` points per frame.  A context starts with HT_MAXPTS and grows
// when a call brings frames that can carry more (w*h / subsample_fraction), so that no cloud is ever cut: handtrack.h:751 takes any count.
// Growing waits for the context's streams, frees the three arrays and allocates them again (their contents are per-call scratch).
int ht_reserve_points_locked(ht_ctx *ctx, int points)
{
	const int want = (points + 63) & ~63;
	if (ctx->d_pts && want <= ctx->model.pts_cap) return HT_OK;
	const size_t B = (size_t)ctx->B, nb = (size_t)ctx->model.nb, cap = (size_t)want;
	HIPCHK(ctx, ht_sync_all(ctx));
	const bool had_voxel = ctx->d_ptsv != nullptr;
	void *old[5] = { ctx->d_pts, ctx->d_rows, ctx->d_scratch, ctx->d_ptsv, ctx->d_rowbody };
	for (void *o : old) drop_alloc(ctx, o);
	ctx->d_pts = nullptr; ctx->d_rows = nullptr; ctx->d_scratch = nullptr; ctx->d_ptsv = nullptr; ctx->d_rowbody = nullptr; ctx->model.pts_cap = 0;
	int r;
	if ((r = dev_alloc(ctx, &ctx->d_pts, B * cap))) return r;
	if ((r = dev_alloc(ctx, &ctx->d_rows, B * cap * HT_ROW))) return r;
	if ((r = dev_alloc(ctx, &ctx->d_rowbody, B * cap))) return r;
	if ((r = dev_alloc(ctx, &ctx->d_scratch, B * ht_scratch_rows(cap, nb) * (HT_CREC + 6)))) return r;      // a row record + 1 float for the impulse sum, 1 word for the chain entry (frames that do not fit k_solve's LDS) and 4 floats of couplings per chain entry (ht_quad.hpp: quad_blocks_run); was: k_solve's LDS
	if (had_voxel && (r = dev_alloc(ctx, &ctx->d_ptsv, B * cap))) return r;
	ctx->model.pts_cap = want;
	return HT_OK;
}
extern "C" int ht_reserve_points(ht_ctx *ctx, int points)
{
	CHECK_READY(ctx); CHECK_MODEL(ctx);
	if (points < 1 || points > HT_POINTS_LIMIT) { ctx->err = "ht_reserve_points: between 1 and 76800 points (a 320x240 frame with every pixel in range)"; return HT_ERR_ARG; }
	return ht_reserve_points_locked(ctx, points < HT_MAXPTS ? HT_MAXPTS : points);
}
extern "C" int ht_point_capacity(ht_ctx *ctx, int *points)
{
	CHECK_READY(ctx); CHECK_MODEL(ctx);
	if (!points) return HT_ERR_ARG;
	*points = ctx->model.pts_cap;
	return HT_OK;
}
// the buffer of the solve tables (k_solve_prep's output, ht_solve_shared.hpp): only a context that switches the path on has it
int ht_alloc_solve_tables(ht_ctx *ctx)
{
	if (ctx->d_tables) return HT_OK;
	const size_t B = (size_t)ctx->B;
	int r;
	if ((r = dev_alloc(ctx, &ctx->d_tables, B * TB_WORDS))) return r;
	return HT_OK;
}
int ht_alloc_buffers(ht_ctx *ctx)
{
	const size_t B = (size_t)ctx->B, nb = (size_t)ctx->model.nb;
	int r;
#define A(ptr, n) if ((r = dev_alloc(ctx, &ctx->ptr, (n)))) return r
	A(d_depth, B * 4096); A(d_cams, B * HT_CAM);
	if ((r = net_alloc_frames(ctx, *ht_net_of(ctx, 64)))) return r;      // the larger net's come with its first weights (cnn_load_weights)
	A(d_act3, B * 2048);
	A(d_logits, B * HT_CNN_OUT); A(d_cnn_out, B * HT_CNN_OUT); A(d_analysis, B * HT_ANALYSIS);
	if (ctx->cnn_only) return HT_OK;
	A(d_npts, B);
	A(d_state[0], B * nb * HT_STATE_STRIDE); A(d_state[1], B * nb * HT_STATE_STRIDE);
	A(d_prev_err, B); A(d_initializing, B); A(d_err_old, B); A(d_err_new, B); A(d_flags, B); A(d_nflags, B);
	A(d_nreset, 2); HIPCHK(ctx, hipMemset(ctx->d_nreset, 0, 2 * sizeof(unsigned)));
	A(d_flist, B); A(d_nflist, 1); HIPCHK(ctx, hipMemset(ctx->d_nflist, 0, sizeof(int)));
	{
		void *h = nullptr;
		HIPCHK(ctx, hipHostMalloc(&h, 2 * sizeof(unsigned), hipHostMallocDefault));
		ctx->h_nreset = static_cast<volatile unsigned *>(h); ctx->h_nreset[0] = ctx->h_nreset[1] = 0;
		hipDeviceProp_t prop;
		if (hipGetDeviceProperties(&prop, ctx->device) == hipSuccess && prop.multiProcessorCount > 0) ctx->n_cu = prop.multiProcessorCount;
	}
	A(d_nrows, B);
	A(d_chamber, B * 5 * nb * HT_ROW); A(d_nchamber, B); A(d_accepted, B); A(d_chplanes, B * 20); A(d_chon, B);
	if (ht_tuning_int("HT_TABLES", 0) > 0) { if ((r = ht_alloc_solve_tables(ctx))) return r; }      // measurement builds (tools/exp_tables.sh); otherwise on ht_debug_solve_tables(ctx, 1)
	A(d_contacts, B * HT_MAXCONTACT * HT_CONTACT); A(d_ncontacts, B); A(d_epa_ws, ht_contacts_workspace_bytes((int)B)); HIPCHK(ctx, hipMemset(ctx->d_epa_ws, 0, ht_contacts_workspace_bytes((int)B)));
	if ((r = ht_history_alloc(ctx, ctx->contact_hist))) return r;
	A(d_porder, B);
	if ((r = ht_history_alloc(ctx, ctx->solve_hist))) return r;
	if ((r = ht_reserve_points_locked(ctx, HT_MAXPTS))) return r;
	A(d_poses_out, B * nb * HT_POSE); A(d_start, B * nb * HT_POSE);
	A(d_stage, B * nb * HT_STATE_STRIDE);
#undef A
	HIPCHK(ctx, hipMemset(ctx->d_state[0], 0, B * nb * HT_STATE_STRIDE * sizeof(float)));
	HIPCHK(ctx, hipMemset(ctx->d_state[1], 0, B * nb * HT_STATE_STRIDE * sizeof(float)));
	HIPCHK(ctx, hipMemset(ctx->d_prev_err, 0, B * sizeof(float)));
	HIPCHK(ctx, hipMemset(ctx->d_initializing, 0, B * sizeof(int)));
	HIPCHK(ctx, hipMemset(ctx->d_npts, 0, B * sizeof(int)));
	HIPCHK(ctx, hipMemset(ctx->d_nrows, 0, B * sizeof(int)));
	HIPCHK(ctx, hipMemset(ctx->d_ncontacts, 0, B * sizeof(int)));
	return HT_OK;
}
