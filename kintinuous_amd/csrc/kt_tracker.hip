// kt_tracker.hip -- KintinuousTracker::processFrame (src/frontend/KintinuousTracker.cpp:444-915) as a
// device-resident pipeline on one HIP stream: pyramid build -> odometry (all Gauss-Newton iterations
// enqueued back to back, solved on the device) -> ONE host sync for the pose -> cyclical-volume shift
// (slab extract + clear) -> integrate -> raycast -> predicted-map pyramid.  The reference performs 19
// blocking host round trips per frame (reduce.cu:398-401); this path performs one.
// Host-side state (pose lists, shift decision, dense pose graph) restates
// KintinuousTracker.cpp:71-182, 262-382, 575-667, 1003-1048, 1075-1085.
// This unit is the frame pipeline only: create / reset / destroy, the frame entry points, odometry, the set-up kernel, fusion, the
// shift, planning ahead, read-ahead, finalise.  struct kt_tracker is in kt_tracker.hpp; the slabs a shift extracts go to its
// kt_slice_store (kt_tracker_slices.hip, with the kt_tracker_slice_* / kt_tracker_enable_* calls), which this unit reaches only
// through fetch / back / join / clear / shutdown; the getters and debug hooks are in kt_tracker_api.hip.
#include "kt_tracker.hpp"
#include "kt_setup.hpp"

#include <limits.h>
#include <stdlib.h>
#include <string.h>

#include <atomic>
#include <chrono>

#ifndef KT_SIDE_GATE_DEFAULT
#define KT_SIDE_GATE_DEFAULT 2
#endif

static std::atomic<int> kt_live_trackers{0};   // live trackers of this process: the level form of the ICP chain needs to be alone (kt_tracker_create)

static int plan_frame(kt_tracker* t, const struct Pending& frame, long long ordinal);
static int lvl_cols(const kt_tracker* t, int l) { return t->cfg.cols >> l; }
static int lvl_rows(const kt_tracker* t, int l) { return t->cfg.rows >> l; }
static kt_intr lvl_intr(kt_intr k, int l)  // Intr::operator() internal.h:255-259
{
    const int div = 1 << l;
    kt_intr r = {k.fx / div, k.fy / div, k.cx / div, k.cy / div};
    return r;
}

// make sets[q] the current frame's set
static void select_set(kt_tracker* t, int q)
{
    for (int l = 0; l < KT_LEVELS; ++l) {
        t->depths_curr[l] = t->sets[q].depths[l];
        t->vmaps_curr[l] = t->sets[q].vmaps[l];
        t->nmaps_curr[l] = t->sets[q].nmaps[l];
    }
    t->depth_raw_scaled = t->sets[q].scaled;
    t->rec_curr = t->sets[q].rec;
}

// next set in rotation that is neither the previous frame's (its fusion may still run; RGB-D "last" of the coming frame) nor owned
// by an outstanding read-ahead; -1 if there is none
static int pick_free_set(kt_tracker* t)
{
    for (int k = 1; k <= KT_NSETS; ++k) {
        const int q = (t->last_assigned + k) % KT_NSETS;
        bool taken = q == t->prev_set;
        for (const Pending& p : t->pending) taken = taken || p.set == q;
        if (!taken) return q;
    }
    return -1;
}

// Events that only order one stream of this device behind another: no timing, no system-scope fence (the cache write-back of the
// default record is a 6 us bubble on the main stream; kernel boundaries already order device memory between streams of one agent).
#ifndef KT_EV_DEVICE
#define KT_EV_DEVICE (hipEventDisableTiming | hipEventDisableSystemFence)
#endif

// `stream` may overwrite what frame `u` consumed (its frame set, its staging slot) only after fusion(u) and the RGB-D "last" reads of
// odometry(u + 1).  Three ways to know, cheapest first:
//   1. the host has seen the pose of frame u + 1 in the mirror: the set-up kernel that posted it runs behind odometry(u + 1), which
//      runs behind fusion(u) -- the normal case (kt_tracker_prefetch_frame observes the frame in flight first), no stream operation;
//   2. -p mode, where the host never waits for a pose: odo_ev[u + 1], recorded between fusion(u) and fusion(u + 1);
//   3. otherwise order against everything enqueued so far.
// (A record per frame in every mode is a 5 us bubble on the main stream, rocprofv3 kernel trace: a marker packet between two kernels.)
static int wait_frame_consumed(kt_tracker* t, hipStream_t stream, long long u)
{
    if (u < 0 || stream == t->ctx->stream) return KT_OK;   // the main stream is ordered by itself
    if (u + 2 <= t->frames_observed) return KT_OK;
    if (t->has_trajectory && u + 1 < t->frames_started) {
        // a slot of the ring that has since been re-recorded by frame u + 1 + k * KT_NODO only waits longer, never less
        KT_HIP(hipStreamWaitEvent(stream, t->odo_ev[(u + 1) % KT_NODO], 0));
    } else {
        KT_HIP(hipEventRecord(t->guard_ev, t->ctx->stream));
        KT_HIP(hipStreamWaitEvent(stream, t->guard_ev, 0));
    }
    return KT_OK;
}

// minimumGradientMagnitudes / sobelScale of RGBDOdometry (RGBDOdometry.cpp:64-70, 236): the squared-gradient threshold of level l
static float rgbd_min_scale(int l)
{
    const float min_grad[KT_LEVELS] = {12, 5, 3, 1};
    const double SOBEL_SCALE = 1.0 / pow(2.0, 3);
    return (float)(pow(min_grad[l], 2.0) / pow(SOBEL_SCALE, 2.0));
}

// [A] of processFrame (KintinuousTracker.cpp:465-479) plus the pose-independent half of integrate, into sets[q] on cx's stream
static int build_frame_set(kt_tracker* t, kt_ctx* cx, int q, const uint16_t* depth_raw, const uint8_t* colors)
{
    const int cols = t->cfg.cols, rows = t->cfg.rows;
    FrameSet& fs = t->sets[q];
    // the odometry provider objects of the ctor (KintinuousTracker.cpp:128-178): ground truth wins over the RGB-D flags
    const bool icp = !t->has_trajectory && !(t->cfg.use_rgbd || t->cfg.use_rgbd_icp);
    const bool rgbd = !t->has_trajectory && !icp;
    static const bool fused_prepare = []() { const char* e = getenv("KT_PREPARE_FUSED"); return e ? atoi(e) != 0 : true; }();
    if (icp || t->cfg.use_rgbd_icp || !t->cfg.disable_color_angle) {
        KT_TRY(kt_bilateral_filter(cx, depth_raw, fs.depths[0], cols, rows));
        uint16_t* dl[3] = {fs.depths[1], fs.depths[2], fs.depths[3]};
        if (fused_prepare)   // pyramid + scaleDepth + pixel records in three launches (kt_volume.hip)
            KT_TRY(kt_frame_prepare(cx, &t->intr, fs.depths[0], dl, fs.vmaps, fs.nmaps, depth_raw, colors, cols, rows, !t->cfg.disable_color_angle, fs.scaled, fs.rec, fs.dpmax));
        else {
            KT_TRY(kt_build_pyramid(cx, &t->intr, fs.depths[0], cols, rows, dl, fs.vmaps, fs.nmaps));
            KT_TRY(kt_integrate_prepare(cx, depth_raw, colors, fs.nmaps[0], cols, rows, &t->intr, !t->cfg.disable_color_angle, fs.scaled, fs.rec, fs.dpmax));
        }
    } else
        KT_TRY(kt_integrate_prepare(cx, depth_raw, colors, fs.nmaps[0], cols, rows, &t->intr, !t->cfg.disable_color_angle, fs.scaled, fs.rec, fs.dpmax));
    if (rgbd) {
        // RGBDOdometry::populateRGBDData (RGBDOdometry.cpp:140-158), the derivative images of the frame as "next" (:296-300) and its
        // point clouds as "last" (:186): all functions of the frame alone
        KT_TRY(kt_depth_to_metres(cx, depth_raw, fs.depth_m[0], cols, rows, (int)(6.0 * 1000)));
        for (int l = 0; l + 1 < KT_LEVELS; ++l) KT_TRY(kt_pyr_down_gauss_f32(cx, fs.depth_m[l], lvl_cols(t, l), lvl_rows(t, l), fs.depth_m[l + 1]));
        KT_TRY(kt_bgr_to_intensity(cx, colors, fs.image[0], cols, rows));
        for (int l = 0; l + 1 < KT_LEVELS; ++l) KT_TRY(kt_pyr_down_gauss_u8(cx, fs.image[l], lvl_cols(t, l), lvl_rows(t, l), fs.image[l + 1]));
        const double ifx = t->intr.fx, ify = t->intr.fy, icx = t->intr.cx, icy = t->intr.cy;  // RGBDOdometry.cpp:72-75
        for (int l = 0; l < KT_LEVELS; ++l) {
            KT_TRY(kt_derivative_images(cx, fs.image[l], lvl_cols(t, l), lvl_rows(t, l), fs.dIdx[l], fs.dIdy[l]));
            KT_TRY(kt_rgb_residual_candidates(cx, rgbd_min_scale(l), fs.dIdx[l], fs.dIdy[l], fs.depth_m[l], fs.image[l], lvl_cols(t, l),
                                              lvl_rows(t, l), fs.cand[l]));
            KT_TRY(kt_project_to_cloud(cx, fs.depth_m[l], lvl_cols(t, l), lvl_rows(t, l), fs.cloud[l], ifx, ify, icx, icy, l));
        }
    }
    return KT_OK;
}

static void compute_global_camera(kt_tracker* t, const float* tcurr)
{
    // KintinuousTracker.cpp:581-595 (and :274-287 in reset())
    for (int k = 0; k < 3; ++k) {
        const float initial_trans = (float)((double)t->volume_basis[k] - (double)t->cfg.volume_size * 0.5);
        t->current_global_camera[k] = initial_trans;
        t->current_global_camera[k] += (float)t->voxel_wrap[k] * t->voxel_size[k];
        if (tcurr) t->current_global_camera[k] += tcurr[k] - t->volume_basis[k];
    }
}

static void v_wrap_copy_update(kt_tracker* t)
{
    // vWrapCopyUpdate KintinuousTracker.cpp:1075-1085
    for (int k = 0; k < 3; ++k) {
        t->v_wrap_copy[k] = t->voxel_wrap[k];
        if (t->v_wrap_copy[k] < 0) t->v_wrap_copy[k] = t->N - ((-t->v_wrap_copy[k]) % t->N);
    }
}

static void push_pose(kt_tracker* t, uint64_t ts, const float* R, int is_loop)
{
    DensePose p;
    p.ts = ts;
    p.is_loop = is_loop;
    for (int i = 0; i < 16; ++i) p.pose[i] = (i % 5 == 0) ? 1.f : 0.f;
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) p.pose[i * 4 + j] = R[i * 3 + j];
        p.pose[i * 4 + 3] = t->current_global_camera[i];
    }
    t->poses.push_back(p);
}

// ---- profiling helpers ---------------------------------------------------------------------------
// profiling modes: 0 off; 1 the tsdf23 event pair on every 8th frame (long timed regions: the timing stays off the other 7);
// 2 every stage of every frame (serial breakdown pass); 4 the tsdf23 pair on EVERY frame (short timed regions)
static bool prof_all(const kt_tracker* t) { return t->profiling == 2 || t->profiling == 3; }
static bool prof_tsdf(const kt_tracker* t) { return t->profiling == 1 || t->profiling == 4 || t->profiling == 5 || t->profiling == 6; }
static int ev_begin(kt_tracker* t, int st)
{
    if (prof_all(t) || (prof_tsdf(t) && st == ST_TSDF23)) {
        KT_HIP(hipEventRecord(t->ev[t->ev_par][st][0], t->ctx->stream));
    }
    return KT_OK;
}
static int ev_end(kt_tracker* t, int st)
{
    if (prof_all(t) || (prof_tsdf(t) && st == ST_TSDF23)) {
        KT_HIP(hipEventRecord(t->ev[t->ev_par][st][1], t->ctx->stream));
        t->ev_rec[t->ev_par][st] = true;
    }
    return KT_OK;
}
static void tsdf23_hook_arm(kt_tracker* t)
{
    // 4: every frame; 1 / 5: every 8th / 4th (an event pair costs two marker packets = ~10 us of bubbles on the main stream)
    kt_tsdf23_hook.on = prof_all(t) || t->profiling == 4 || (t->profiling == 1 && (t->prof_frames++ % 8) == 0) || (t->profiling == 5 && (t->prof_frames++ % 4) == 0) ||
                        (t->profiling == 6 && (t->prof_frames++ % 2) == 0);   // 6: every second frame (the driver's 20-frame region: 10 samples)
    kt_tsdf23_hook.ev[0] = t->ev[t->ev_par][ST_TSDF23][0];
    kt_tsdf23_hook.ev[1] = t->ev[t->ev_par][ST_TSDF23][1];
    if (kt_tsdf23_hook.on) t->ev_rec[t->ev_par][ST_TSDF23] = true;
}
// harvest every recorded pair whose end event has completed (pairs still in flight stay armed)
void ev_collect(kt_tracker* t)
{
    if (!t->profiling) return;
    for (int par = 0; par < 2; ++par)
        for (int st = 0; st < ST_COUNT; ++st)
            if (t->ev_rec[par][st] && hipEventQuery(t->ev[par][st][1]) == hipSuccess) {
                float ms = 0.f;
                if (hipEventElapsedTime(&ms, t->ev[par][st][0], t->ev[par][st][1]) == hipSuccess) {
                    t->stage_ms_sum[st] += ms;
                    t->stage_n[st] += 1;
                    t->stage_ms_last[st] = ms;
                }
                t->ev_rec[par][st] = false;
            }
}

extern "C" {

static int tracker_create_impl(kt_tracker* t, kt_ctx* ctx, const kt_tracker_config* cfg);

int kt_tracker_create(kt_ctx* ctx, const kt_tracker_config* cfg, kt_tracker** out)
{
    KT_ARG(ctx && cfg && out);
    KT_ARG(cfg->cols > 0 && cfg->rows > 0 && cfg->N > 0 && cfg->volume_size > 0);
    KT_ARG((cfg->cols % 8) == 0 && (cfg->rows % 8) == 0);  // 4 pyramid levels
    KT_ARG(cfg->N <= 1536);                                 // 32-bit voxel offsets (kt_volume.hip)
    KT_HIP(hipSetDevice(ctx->device));
    kt_tracker* t = new kt_tracker();   // value-initialised, then the in-class defaults: what a failed create took is in t->mem, which destroy releases
    const int s = tracker_create_impl(t, ctx, cfg);
    if (s != KT_OK) {
        t->ctx = ctx;
        (void)kt_tracker_destroy(t);   // kt_last_error() keeps the message of the failure
        return s;
    }
    *out = t;
    return KT_OK;
}

static int tracker_create_impl(kt_tracker* t, kt_ctx* ctx, const kt_tracker_config* cfg)
{
    t->ctx = ctx;
    kt_mem& m = t->mem;
    const hipStream_t st = ctx->stream;   // zero-fill goes on the context's stream
    t->cfg = *cfg;
    t->N = cfg->N;
    // KintinuousTracker ctor, KintinuousTracker.cpp:71-182
    t->intr.fx = cfg->fx; t->intr.fy = cfg->fy; t->intr.cx = cfg->cx; t->intr.cy = cfg->cy;
    for (int k = 0; k < 3; ++k) {
        t->volume_size[k] = cfg->volume_size;
        t->voxel_size[k] = cfg->volume_size / (float)cfg->N;
    }
    for (int k = 0; k < 9; ++k) t->initial_rotation[k] = (k % 4 == 0) ? 1.f : 0.f;
    for (int k = 0; k < 3; ++k) t->volume_basis[k] = t->volume_size[k] * 0.5f;
    if (cfg->static_mode || cfg->dynamic_cube)  // :101-110
        t->volume_basis[2] = t->volume_size[2] * 0.5f - (float)(((double)t->volume_size[2] * 0.5) + (cfg->static_mode ? 0.45 : 0));
    const float default_tranc = fmaxf(0.01f, t->volume_size[0] / 100.0f);               // :112
    const float mc = fmaxf(t->voxel_size[0], fmaxf(t->voxel_size[1], t->voxel_size[2]));
    t->tranc_dist = fmaxf(default_tranc, 2.1f * mc);                                    // TSDFVolume.cpp:89-97

    const size_t nvox = (size_t)cfg->N * cfg->N * cfg->N;
    const size_t P = (size_t)cfg->cols * cfg->rows;
    KT_TRY(m.device(&t->tsdf, nvox));
    KT_TRY(m.device(&t->color, nvox * 4));
    for (int l = 0; l < KT_LEVELS; ++l) {  // allocateBuffers :356-382; zero-filled so "stale" planes are defined
        const size_t p = (size_t)lvl_cols(t, l) * lvl_rows(t, l);
        const size_t q = cfg->use_rgbd || cfg->use_rgbd_icp ? p : 0;
        for (FrameSet& fs : t->sets) {
            KT_TRY(m.device_zero(&fs.depths[l], p, st));
            KT_TRY(m.device_zero(&fs.vmaps[l], 3 * p, st));
            KT_TRY(m.device_zero(&fs.nmaps[l], 3 * p, st));
            KT_TRY(m.device_zero(&fs.depth_m[l], q, st));
            KT_TRY(m.device_zero(&fs.image[l], q, st));
            KT_TRY(m.device_zero(&fs.dIdx[l], q, st));
            KT_TRY(m.device_zero(&fs.dIdy[l], q, st));
            KT_TRY(m.device_zero(&fs.cand[l], q, st));
            KT_TRY(m.device_zero(&fs.cloud[l], 3 * q, st));
        }
        KT_TRY(m.device_zero(&t->vmaps_g_prev[l], 3 * p, st));
        KT_TRY(m.device_zero(&t->nmaps_g_prev[l], 3 * p, st));
        KT_TRY(m.device_zero(&t->corres[l], q, st));
    }
    KT_TRY(m.device_zero(&t->vmap_curr_color, P * 4, st));
    for (FrameSet& fs : t->sets) {
        KT_TRY(m.device_zero(&fs.scaled, P, st));
        KT_TRY(m.device_zero((unsigned char**)&fs.rec, kt_integrate_rec_bytes(cfg->cols, cfg->rows), st));
        KT_TRY(m.device_zero((unsigned char**)&fs.dpmax, kt_integrate_dpmax_bytes(cfg->cols, cfg->rows), st));
        KT_TRY(m.event(&fs.ready, KT_EV_DEVICE));
    }
    KT_TRY(m.event(&t->guard_ev, KT_EV_DEVICE));
    for (int k = 0; k < KT_NODO; ++k) KT_TRY(m.event(&t->odo_ev[k], KT_EV_DEVICE));
    KT_TRY(m.stream(&t->pre_stream));
    KT_TRY(kt_bilateral_lut_ensure(ctx));   // before the context is cloned: both streams share the table
    t->pre_ctx = *ctx;
    t->pre_ctx.stream = t->pre_stream;
    t->pre_ctx.own_stream = false;
    select_set(t, 0);
    KT_TRY(t->slice.create(ctx, &m, cfg->N, cfg->max_slice_points > 0 ? (size_t)cfg->max_slice_points : P * 3,  // cloud_device_(numPixels * 3) :77
                           fmaxf(t->voxel_size[0], fmaxf(t->voxel_size[1], t->voxel_size[2]))));
    KT_TRY(m.device_zero(&t->state_dev, 1, st));
    KT_TRY(m.pinned(&t->state_host, 1));
    for (int k = 0; k < KT_NSLOTS; ++k) {
        KT_TRY(m.device_zero(&t->depth_stage[k], P, st));
        KT_TRY(m.device_zero(&t->rgb_stage[k], P * 3, st));
        KT_TRY(m.pinned(&t->depth_stage_host[k], P));
        KT_TRY(m.pinned(&t->rgb_stage_host[k], P * 3));
        KT_TRY(m.event(&t->slot_uploaded[k], hipEventDisableTiming));
    }
    KT_TRY(m.device_zero(&t->upd_dev, 16, st));
    KT_TRY(m.device_zero(&t->steps_dev, 4, st));
    for (int par = 0; par < 2; ++par)
        for (int s = 0; s < ST_COUNT; ++s) {
            KT_TRY(m.event(&t->ev[par][s][0], hipEventDefault));
            KT_TRY(m.event(&t->ev[par][s][1], hipEventDefault));
        }
    KT_TRY(m.device_zero(&t->fp_dev, 1, st));
    KT_TRY(m.stream(&t->plan_stream));
    // The level form is used only while this is the ONLY live tracker of the process (decided per frame, icp_odometry): its workgroups wait for
    // each other inside a launch and need the whole machine, so anything that keeps compute units busy next to it for long -- a second tracker
    // fed from the same host (scripts/multistream_one_gpu.py) -- can keep its last workgroup out until the bounded waits give up.  The
    // tracker's own side streams are finite per frame and its main-stream kernels are ordered behind the launch.  What this process cannot
    // see -- another process on the same GPU -- is handled per frame: a launch whose waits give up (50 ms) aborts, complete_frame re-runs the
    // frame's odometry in the stepwise form and keeps the level form off for a while (icp_demote).
    t->icp_levels = kt_icp_levels_selected(ctx->device);
    kt_live_trackers.fetch_add(1);
    t->counted = true;
    for (kt_tracker::PlanSlot& pl : t->plans) {
        KT_TRY(kt_tsdf_plan_alloc(&pl.plan, cfg->N));
        KT_TRY(m.event(&pl.done, KT_EV_DEVICE));
    }
    KT_TRY(m.event(&t->gate_ev, KT_EV_DEVICE));
    {
        // KT_SIDE_GATE: 0 never, 1 always, 2 (default) on dense views only -- the rule that picks 32 x 2 wave-columns (more than 1.5 pixels per
        // voxel column: the voxel kernel is the frame's longest and its launch is dense)
        const char* e = getenv("KT_SIDE_GATE");
        const int mode = e ? atoi(e) : KT_SIDE_GATE_DEFAULT;
        int wcx = 0, wcy = 0, xg = 0, yg = 0;
        kt_tsdf_plan_shape(nullptr, cfg->cols, cfg->rows, cfg->N, &wcx, &wcy, &xg, &yg);
        // "dense view": the voxel pass's rule for 32 x 2 wave-columns AND an image beyond 640x480 -- the case where the voxel kernel is the frame's
        // longest and the read-ahead is heavy (1280x960 into 768^3).  640x480 into 256^3 is dense by the first rule alone, but its voxel kernel is
        // 21 us and its frame is the orbit's: gated and stepwise it ran at 3770 frames/s against 4100 (profiles/r06_experiments.md, call 12)
        const bool dense = wcx == 32 && (long long)cfg->cols * cfg->rows > 640LL * 480LL;
        t->side_gate = mode == 1 || (mode == 2 && dense) ? 1 : 0;
        // A level launch takes every compute unit's whole register file: whatever the side streams have not finished when the odometry starts
        // waits for it to end and then runs beside the voxel kernel after all.  On a dense view (1280x960: the pixel loops are long, the
        // hand-over a level launch saves is 1.4 % of the frame) the odometry therefore stays one launch per iteration -- 48 VGPRs: read-ahead
        // and plan run UNDER it -- and the plan's completion event, which the set-up kernel already waits for, keeps both out of the voxel kernel.
        // (KT_ICP_LEVELS=1 keeps the level form on a dense view too.)
        if (mode == 2 && dense && !kt_icp_levels_forced()) t->icp_levels = false;
    }
    t->plan_enabled = getenv("KT_NO_PLAN") == nullptr;   // (A/B switch: every frame through the in-stream pre-pass)
    t->plan_margin_scale = getenv("KT_PLAN_MARGIN_SCALE") ? (float)atof(getenv("KT_PLAN_MARGIN_SCALE")) : 1.0f;   // (tests: 0 makes every plan miss)
    KT_TRY(m.device_zero(&t->bricks, kt_brick_count(cfg->N) + 16, st));
    for (int k = 0; k < 2; ++k) KT_TRY(m.device_zero(&t->wrkc_carry[k], P, st));  // zero: the oracle's calloc'ed normal map
    KT_TRY(kt_integrate_tables(ctx, cfg->cols, cfg->rows, cfg->N, &t->vgz_dev, &t->zs_dev));
    KT_TRY(m.pinned(&t->mirror, 1, hipHostMallocMapped | hipHostMallocCoherent));
    memset(t->mirror, 0, sizeof(PoseMirror));
    KT_TRY(kt_tracker_reset(t));
    // The kernels of the shift path run for the first time HERE, on the empty volume (a one-voxel extraction, one plane of zeros
    // cleared to zero), not in the middle of the first shift frame: a kernel's first launch pays the runtime's lazy set-up for it.
    KT_TRY(t->slice.warm_up(t->tsdf, t->color, t->volume_size));
    KT_TRY(kt_clear_volume(ctx, t->tsdf, 2, t->N, 0, 0, 0, 0));
    KT_TRY(kt_clear_volume(ctx, t->color, 4, t->N, 0, 0, 0, 0));
    KT_HIP(hipStreamSynchronize(ctx->stream));
    return KT_OK;
}

int kt_tracker_destroy(kt_tracker* t)
{
    if (!t) return KT_OK;
    if (t->counted) kt_live_trackers.fetch_sub(1);   // (a create that failed before it was counted is not)
    for (hipStream_t st : {t->ctx->stream, t->pre_stream, t->plan_stream})   // (a failed create: a stream it never made reads as the null stream)
        (void)hipStreamSynchronize(st);
    t->slice.shutdown();   // its downloads read pinned memory of t->mem
    for (kt_tracker::PlanSlot& pl : t->plans) kt_tsdf_plan_free(&pl.plan);
    t->mem.release();
    delete t;
    return KT_OK;
}

int kt_tracker_reset(kt_tracker* t)
{
    // KintinuousTracker::reset :262-354
    KT_ARG(t);
    t->outstanding = false;
    KT_TRY(kt_refill_granules(t->ctx));   // whatever a failed or abandoned frame left in the hand-off buffer
    KT_HIP(hipStreamSynchronize(t->ctx->stream));
    t->global_time = 0;
    memcpy(t->Rlast, t->initial_rotation, sizeof(t->Rlast));
    memcpy(t->tlast, t->volume_basis, sizeof(t->tlast));
    compute_global_camera(t, nullptr);
    t->voxel_wrap[0] = t->voxel_wrap[1] = t->voxel_wrap[2] = 0;
    t->poses.clear();
    (void)t->slice.join();
    t->slice.clear();
    t->pr_samples.clear();
    memcpy(t->pr_trans, t->current_global_camera, sizeof(t->pr_trans));   // :290-291
    memcpy(t->pr_rot, t->initial_rotation, sizeof(t->pr_rot));
    KT_HIP(hipStreamSynchronize(t->pre_stream));
    t->pending.clear();
    KT_HIP(hipStreamSynchronize(t->plan_stream));
    t->plan_sel = -1;
    for (int k = 0; k < 3; ++k) { t->plans[k].ordinal = -1; t->plans[k].set = -1; }
    t->hist_n = 0;
    t->pred_err_t = t->pred_err_r = 0.0f;
    t->prev_set = -1;
    t->parked = t->cfg.static_mode != 0;
    t->v_wrap_copy[0] = t->v_wrap_copy[1] = t->v_wrap_copy[2] = 0;
    t->gt_utime = 0;
    t->current_ts = 0;
    // the colour-weight carry of pixels without a normal starts from zero, like the freshly allocated nmaps_curr_ it stands for
    for (int k = 0; k < 2; ++k) KT_HIP(hipMemsetAsync(t->wrkc_carry[k], 0, sizeof(float) * (size_t)t->cfg.cols * t->cfg.rows, t->ctx->stream));
    KT_TRY(kt_init_volume(t->ctx, t->tsdf, t->N));
    KT_TRY(kt_init_color_volume(t->ctx, t->color, t->N));
    KT_HIP(hipMemsetAsync(t->bricks, 0, kt_brick_count(t->N), t->ctx->stream));
    memset(t->stage_ms_sum, 0, sizeof(t->stage_ms_sum));
    memset(t->stage_n, 0, sizeof(t->stage_n));
    memset(t->stage_ms_last, 0, sizeof(t->stage_ms_last));
    t->last_U = t->last_S = 0;
    KT_HIP(hipStreamSynchronize(t->ctx->stream));
    return KT_OK;
}

}  // extern "C"

// ---- odometry set-up shared by ICP and RGB-D ------------------------------------------------------
static int odometry_begin(kt_tracker* t, const kt_level_k* first_k)
{
    kt_track_state* s = t->state_host;
    memset(s, 0, sizeof(*s));
    memcpy(s->Rprev, t->Rlast, sizeof(s->Rprev));
    memcpy(s->tprev, t->tlast, sizeof(s->tprev));
    memcpy(s->Rcurr, t->Rlast, sizeof(s->Rcurr));
    memcpy(s->tcurr, t->tlast, sizeof(s->tcurr));
    kt_mat33_inverse(s->Rprev, s->Rprev_inv);  // ICPOdometry.cpp:81
    for (int k = 0; k < 16; ++k) s->resultRt[k] = (k % 5 == 0) ? 1.0 : 0.0;
    if (first_k) kt_compute_krk(s->resultRt, *first_k, s->krkinv, s->kt);
    KT_HIP(hipMemcpyAsync(t->state_dev, s, sizeof(*s), hipMemcpyHostToDevice, t->ctx->stream));
    return KT_OK;
}

static int odometry_end(kt_tracker* t)
{
    return ev_end(t, ST_ODOMETRY);  // the pose stays on the device; complete_frame() reads it one frame later
}

// ICPOdometry::getIncrementalTransformation, ICPOdometry.cpp:68-186
static int icp_odometry(kt_tracker* t, bool stepwise_only = false)
{
    int iters[KT_LEVELS] = {10, 5, 4, 0};
    if (t->cfg.fast_odometry) { iters[0] = 0; iters[1] = 10; iters[2] = 5; iters[3] = 0; }
    const float dist_thres = 0.10f;
    const float angle_thres = (float)sin(20.f * 3.14159254f / 180.f);  // ICPOdometry.h:35-36
    // ICPOdometry.cpp:70-85: the starting state travels in the arguments of the first iteration (no per-frame upload)
    kt_track_state init;
    memset(&init, 0, sizeof(init));
    memcpy(init.Rprev, t->Rlast, sizeof(init.Rprev));
    memcpy(init.tprev, t->tlast, sizeof(init.tprev));
    memcpy(init.Rcurr, t->Rlast, sizeof(init.Rcurr));
    memcpy(init.tcurr, t->tlast, sizeof(init.tcurr));
    kt_mat33_inverse(init.Rprev, init.Rprev_inv);  // ICPOdometry.cpp:81
    bool first = true;
    t->last_icp_levels = !stepwise_only && t->icp_levels && t->icp_demote == 0 && kt_live_trackers.load() == 1;
    if (!stepwise_only && t->icp_demote > 0) --t->icp_demote;
    if (t->last_icp_levels) {
        // ONE launch for the frame (round 6; round 5: one per level): the iterations of all levels hand the pose over inside the kernel
        // (kt_track.hip: kt_icp_level_kernel)
        const float* vc[KT_LEVELS]; const float* nc[KT_LEVELS]; const float* vg[KT_LEVELS]; const float* ng[KT_LEVELS];
        kt_intr li[KT_LEVELS]; int cs[KT_LEVELS], rs[KT_LEVELS], its[KT_LEVELS], nl = 0;
        for (int l = KT_LEVELS - 1; l >= 0; --l) {
            if (iters[l] <= 0) continue;
            vc[nl] = t->vmaps_curr[l]; nc[nl] = t->nmaps_curr[l]; vg[nl] = t->vmaps_g_prev[l]; ng[nl] = t->nmaps_g_prev[l];
            li[nl] = lvl_intr(t->intr, l); cs[nl] = lvl_cols(t, l); rs[nl] = lvl_rows(t, l); its[nl] = iters[l];
            ++nl;
        }
        if (nl) KT_TRY(kt_icp_levels_device(t->ctx, t->state_dev, nl, vc, nc, li, vg, ng, cs, rs, its, dist_thres, angle_thres, &init, 1));
        return odometry_end(t);
    }
    for (int l = KT_LEVELS - 1; l >= 0; --l) {
        const kt_intr li = lvl_intr(t->intr, l);
        for (int it = 0; it < iters[l]; ++it) {
            KT_TRY(kt_icp_step_device(t->ctx, t->state_dev, t->vmaps_curr[l], t->nmaps_curr[l], &li, t->vmaps_g_prev[l],
                                      t->nmaps_g_prev[l], lvl_cols(t, l), lvl_rows(t, l), dist_thres, angle_thres, KT_MODE_ICP_SOLVE,
                                      first ? &init : nullptr));
            first = false;
        }
    }
    return odometry_end(t);
}

// RGBDOdometry::getIncrementalTransformation, RGBDOdometry.cpp:165-393
static int rgbd_odometry(kt_tracker* t, int set, int last_set, bool stepwise_only = false)
{
    int iters[KT_LEVELS];
    if (!t->cfg.use_rgbd_icp) {
        iters[0] = 10; iters[1] = 7; iters[2] = 7; iters[3] = 7;
        if (t->cfg.fast_odometry) { iters[0] = 0; iters[1] = 10; iters[2] = 7; iters[3] = 0; }
    } else {
        iters[0] = 10; iters[1] = 5; iters[2] = 4; iters[3] = 0;
        if (t->cfg.fast_odometry) { iters[0] = 0; iters[1] = 10; iters[2] = 7; iters[3] = 0; }
    }
    const double SOBEL_SCALE = 1.0 / pow(2.0, 3), MAX_DEPTH_DELTA = 0.07;
    const float dist_thres = 0.10f;
    const float angle_thres = (float)sin(20.f * 3.14159254f / 180.f);
    // populateRGBDData, the derivative images and the point clouds were built with the frame sets (build_frame_set)
    KT_ARG(last_set >= 0);
    const FrameSet& next = t->sets[set];
    const FrameSet& last = t->sets[last_set];

    const double ifx = t->intr.fx, ify = t->intr.fy, icx = t->intr.cx, icy = t->intr.cy;  // RGBDOdometry.cpp:72-75
    kt_level_k lk[KT_LEVELS];
    for (int l = 0; l < KT_LEVELS; ++l) {
        const int div = 1 << l;
        lk[l].fx = ifx / div; lk[l].fy = ify / div; lk[l].cx = icx / div; lk[l].cy = icy / div;
    }
    // flatten the (level, iteration) schedule so each solve epilogue knows the NEXT iteration's level
    int sched[64], ns = 0;
    for (int l = KT_LEVELS - 1; l >= 0; --l)
        for (int j = 0; j < iters[l]; ++j) sched[ns++] = l;
    KT_TRY(odometry_begin(t, ns ? &lk[sched[0]] : nullptr));
    t->last_icp_levels = false;   // (the RGB-D modes have no level form: two launches per iteration)
    for (int q = 0; q < ns; ++q) {
        const int l = sched[q];
        const int cols = lvl_cols(t, l), rows = lvl_rows(t, l);
        const int first_at_level = q == 0 || sched[q - 1] != l;   // writes every DataTerm; later iterations only the candidates
        KT_TRY(kt_rgb_residual_device(t->ctx, t->state_dev, rgbd_min_scale(l), next.dIdx[l], next.dIdy[l], last.depth_m[l], next.depth_m[l],
                                      last.image[l], next.image[l], cols, rows, t->corres[l], (float)MAX_DEPTH_DELTA, next.cand[l],
                                      first_at_level));
        const kt_intr li = lvl_intr(t->intr, l);
        const kt_level_k* nk = &lk[q + 1 < ns ? sched[q + 1] : l];
        if (t->cfg.use_rgbd_icp)   // ICP sums + RGB-D sums + joint solve in one launch
            KT_TRY(kt_joint_step_device(t->ctx, t->state_dev, t->vmaps_curr[l], t->nmaps_curr[l], &li, t->vmaps_g_prev[l], t->nmaps_g_prev[l],
                                        dist_thres, angle_thres, t->corres[l], last.cloud[l], next.dIdx[l], next.dIdy[l], (float)SOBEL_SCALE,
                                        cols, rows, nk));
        else
            KT_TRY(kt_rgb_step_device(t->ctx, t->state_dev, t->corres[l], last.cloud[l], li.fx, li.fy, next.dIdx[l], next.dIdy[l],
                                      (float)SOBEL_SCALE, cols, rows, KT_MODE_RGB_SOLVE, nk));
    }
    // swap last/next (:377-381) = the frame sets rotate; the > 0.3 m jump guard (:383-387) runs in kt_frame_setup_kernel
    return odometry_end(t);
}

// ---- frame set-up on the device ---------------------------------------------------------------------------------------
// Runs after the last odometry iteration (csrc/kt_setup.hpp: what it does).  A frame that must shift the volume first is parked (skip = 1) and
// redone by the host's shift path in complete_frame().
// Workgroup 0 (two waves) is the set-up proper; workgroups 1.. are the carry and checkpoint blocks.
__global__ __launch_bounds__(256) void kt_frame_setup_kernel(const kt_setup_args a)
{
    if (blockIdx.x > 0) {
        float R[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, tv[3] = {0, 0, 0};
        if ((int)blockIdx.x > a.carry_groups) kt_setup_final_pose(a, R, tv);   // (the checkpoint blocks of a planned frame: mode 0)
        kt_setup_side_block(a, (int)blockIdx.x, (int)threadIdx.x, R, tv);
        return;
    }
    if (threadIdx.x >= 128 || a.mode == 2) return;
    float R[9], tv[3];
    if (a.mode == 0) kt_setup_final_pose(a, R, tv);
    else {
        for (int k = 0; k < 9; ++k) R[k] = a.R[k];
        for (int k = 0; k < 3; ++k) tv[k] = a.t[k];
    }
    kt_setup_block0(a, R, tv, a.mode == 0 ? a.st->handoff_timeout : 0, (int)(threadIdx.x >> 6), (int)(threadIdx.x & 63));
}

// the arguments of kt_frame_setup_kernel (kt_setup.hpp) as the tracker stands
static int fill_setup_args(kt_tracker* t, int mode, const float* R, const float* tv, kt_setup_args& a)
{
    KT_TRY(kt_integrate_tables(t->ctx, t->cfg.cols, t->cfg.rows, t->N, &t->vgz_dev, &t->zs_dev));  // may have been regrown by another user of the context
    a.st = t->state_dev; a.fp = t->fp_dev; a.vgz = t->vgz_dev; a.zs = t->zs_dev; a.N = t->N;
    a.mirror = t->mirror; a.seq = t->frame_seq;
    a.cell_z = t->volume_size[2] / t->N;
    a.mode = mode;
    a.rgbd_guard = (t->cfg.use_rgbd || t->cfg.use_rgbd_icp) ? 1 : 0;
    for (int k = 0; k < 9; ++k) a.R[k] = R ? R[k] : 0.f;
    for (int k = 0; k < 3; ++k) a.t[k] = tv ? tv[k] : 0.f;
    for (int k = 0; k < 3; ++k) { a.basis[k] = t->volume_basis[k]; a.voxel[k] = t->voxel_size[k]; }
    a.thresh = t->parked ? INT_MAX : t->cfg.voxel_shift;
    a.rec = (kt_pixrec*)t->sets[t->out_set].rec;
    a.carry_cur = t->wrkc_carry[t->carry_sel];
    a.carry_next = t->wrkc_carry[t->carry_sel ^ 1];
    a.npix = t->cfg.cols * t->cfg.rows;
    a.carry_groups = t->cfg.disable_color_angle ? 0 : (a.npix + 1023) / 1024;   // without the angle weight wrkc is 2 everywhere
    a.plan_wrange = nullptr; a.plan_walk0 = nullptr;
    a.walk_groups = 0;
    a.wx = a.wy = a.wcx = a.wcy = a.XG = a.YG = 0; a.cell_x = a.cell_y = a.fx = a.fy = 0.0f; a.plan_theta = a.plan_tau = 0.0f;
    memset(a.plan_R, 0, sizeof(a.plan_R)); memset(a.plan_t, 0, sizeof(a.plan_t));
    if (mode == 0 && t->plan_sel >= 0) {
        const kt_tracker::PlanSlot& pl = t->plans[t->plan_sel];
        a.plan_wrange = pl.plan.wrange; a.plan_walk0 = pl.plan.walk0;
        memcpy(a.plan_R, pl.R, sizeof(a.plan_R)); memcpy(a.plan_t, pl.t, sizeof(a.plan_t));
        a.plan_theta = pl.theta; a.plan_tau = pl.tau;
        kt_tsdf_plan_shape(&pl.plan, t->cfg.cols, t->cfg.rows, t->N, &a.wcx, &a.wcy, &a.XG, &a.YG);
        a.wx = t->v_wrap_copy[0] % t->N; a.wy = t->v_wrap_copy[1] % t->N;
        a.cell_x = t->volume_size[0] / t->N; a.cell_y = t->volume_size[1] / t->N;
        a.fx = t->intr.fx; a.fy = t->intr.fy;
        a.walk_groups = (a.XG * a.YG + 3) / 4;
    }
    return KT_OK;
}

static int launch_setup(kt_tracker* t, int mode, const float* R, const float* tv)
{
    kt_setup_args a;
    KT_TRY(fill_setup_args(t, mode, R, tv, a));
    hipLaunchKernelGGL(kt_frame_setup_kernel, dim3(1 + a.carry_groups + a.walk_groups), dim3(256), 0, t->ctx->stream, a);
    KT_LAUNCH_CHECK();
    return KT_OK;
}

// the integrate call of frame set `set` as the tracker stands; the caller adds the pose and the wrap
static kt_integrate_job integrate_job(kt_tracker* t, int set, const uint16_t* depth_raw, const uint8_t* colors)
{
    const FrameSet& fs = t->sets[set];
    kt_integrate_job j;
    j.depth_raw = depth_raw; j.cols = t->cfg.cols; j.rows = t->cfg.rows; j.intr = &t->intr; j.volume_size = t->volume_size; j.tranc_dist = t->tranc_dist;
    j.volume = t->tsdf; j.depth_raw_scaled = fs.scaled; j.color_volume = t->color; j.colors = colors; j.nmap_curr = fs.nmaps[0];
    j.angle_color = !t->cfg.disable_color_angle; j.N = t->N; j.updated_dev = t->counting ? t->upd_dev : nullptr;
    j.prepared_rec = fs.rec; j.prepared_dpmax = fs.dpmax; j.bricks = t->bricks;
    return j;
}

// [H] integrate (:864-876) + [I] raycast (:880-890) + [J] predicted-map pyramid (:892-899, fused into the raycast epilogue), with
// the pose taken from fp_dev; wrap = the tracker's current v_wrap_copy
static int enqueue_fusion(kt_tracker* t, int set, const uint16_t* depth_raw, const uint8_t* colors, const kt_tsdf_plan* plan)
{
    kt_ctx* c = t->ctx;
    const int cols = t->cfg.cols, rows = t->cfg.rows, N = t->N;
    const bool icp = !t->has_trajectory && !(t->cfg.use_rgbd || t->cfg.use_rgbd_icp);
    const kt_mat33 dummy_R = {{1, 0, 0, 0, 1, 0, 0, 0, 1}};
    const float dummy_t[3] = {0, 0, 0};
    if (t->counting) {
        KT_HIP(hipMemsetAsync(t->upd_dev, 0, 16 * sizeof(unsigned int), c->stream));
        KT_HIP(hipMemsetAsync(t->steps_dev, 0, 4 * sizeof(unsigned long long), c->stream));
    }
    KT_TRY(ev_begin(t, ST_INTEGRATE));
    tsdf23_hook_arm(t);
    kt_integrate_job j = integrate_job(t, set, depth_raw, colors);
    j.Rcurr_inv = &dummy_R; j.tcurr = dummy_t; j.voxel_wrap = t->v_wrap_copy; j.fp = t->fp_dev; j.plan = plan;
    KT_TRY(kt_integrate_tsdf_impl(c, j));
    KT_TRY(ev_end(t, ST_INTEGRATE));
    if (t->side_gate) { KT_HIP(hipEventRecord(t->gate_ev, c->stream)); t->gate_armed = true; }   // the voxel kernel has drained: the side streams may run
    KT_TRY(ev_begin(t, ST_RAYCAST));
    const bool pyr = icp || t->cfg.use_rgbd_icp;
    float* vp[3] = {t->vmaps_g_prev[1], t->vmaps_g_prev[2], t->vmaps_g_prev[3]};
    float* np_[3] = {t->nmaps_g_prev[1], t->nmaps_g_prev[2], t->nmaps_g_prev[3]};
    KT_TRY(kt_raycast_impl(c, &t->intr, &dummy_R, dummy_t, t->tranc_dist, t->volume_size, t->tsdf, t->vmaps_g_prev[0], t->nmaps_g_prev[0], cols, rows,
                           t->v_wrap_copy, t->vmap_curr_color, t->color, N, t->counting ? t->steps_dev : nullptr, pyr ? vp : nullptr,
                           pyr ? np_ : nullptr, t->fp_dev, t->bricks));
    KT_TRY(ev_end(t, ST_RAYCAST));
    return KT_OK;
}

// the slab of voxels [lo, hi) (mesh: cells [mlo, mhi)) leaves the volume as the tracker stands: extraction and stages are enqueued, nothing waits
static int fetch_slice(kt_tracker* t, const int lo[3], const int hi[3], int dim, const int mlo[3], const int mhi[3])
{
    const kt_slice_request q = {lo, hi, mlo, mhi, dim, t->tsdf, t->color, t->volume_size, t->v_wrap_copy, t->voxel_wrap,
                                t->Rlast, t->current_global_camera, t->current_ts};
    return t->slice.fetch(q);
}

static int read_counts(kt_tracker* t)
{
    if (!t->counting) return KT_OK;
    kt_ctx* c = t->ctx;
    unsigned int u = 0;
    unsigned long long sdev = 0;
    KT_HIP(hipMemcpyAsync(&u, t->upd_dev, sizeof(u), hipMemcpyDeviceToHost, c->stream));
    KT_HIP(hipMemcpyAsync(&sdev, t->steps_dev, sizeof(sdev), hipMemcpyDeviceToHost, c->stream));
    KT_HIP(hipStreamSynchronize(c->stream));
    t->last_U = u;
    t->last_S = sdev;
    return KT_OK;
}

// GroundTruthOdometry::getIncrementalTransformation (GroundTruthOdometry.cpp:42-74): the pose of the frame stamped `timestamp` from
// the loaded trajectory, composed in the volume's frame.  Every product is float, in Eigen's evaluation order: delta =
// Ta^-1 * Tb as Isometry3f (3x3 products, translation = linear * t + t), then currentTsdf * M^-1 * delta * M left to right as
// 4x4 products.  M permutes and negates axes, so the first and last product are exact column moves; the middle one rounds, with
// its sums running over the moved columns.
static void ground_truth_pose(kt_tracker* t, uint64_t timestamp, float Rcurr[9], float tcurr[3])
{
    memcpy(Rcurr, t->Rlast, 9 * sizeof(float));
    memcpy(tcurr, t->tlast, 3 * sizeof(float));
    if (t->gt_utime == 0 || t->trajectory.empty()) return;   // :50 -- a previous stamp of 0 reads as "no previous frame"
    const std::array<float, 12>& A = t->trajectory[(int)(uint32_t)t->gt_utime];   // operator[], as the reference
    const std::array<float, 12>& B = t->trajectory[(int)(uint32_t)timestamp];
    kt_host_ground_truth_pose(A.data(), B.data(), t->Rlast, t->tlast, Rcurr, tcurr);
}

// KintinuousTracker::addToPlaceRecognition :917-958: the sample carries lastPlaceRecognitionTrans / Rot (set by the caller just before)
static int add_pr_sample(kt_tracker* t)
{
    PrSample ps;
    ps.utime = t->current_ts;
    memcpy(ps.trans, t->pr_trans, sizeof(ps.trans));
    memcpy(ps.rot, t->pr_rot, sizeof(ps.rot));
    ps.pose_index = (int)t->poses.size();   // the dense pose of the frame being processed is pushed after this
    t->pr_samples.push_back(ps);
    return (int)t->pr_samples.size() - 1;
}

// Host half of a frame once its pose is known: the pose bookkeeping of KintinuousTracker.cpp:574-595, 903-909 and, when the volume
// has to shift (:627-833), the shift.  speculated = the fusion kernels were already enqueued against the device-side shift decision
// (they ran unless the device parked them); otherwise (pose supplied by the host) they are enqueued here, after any shift.
static int finish_pose(kt_tracker* t, float Rcurr[9], float tcurr[3], bool speculated)
{
    kt_ctx* c = t->ctx;
    const int N = t->N;
    t->current_ts = t->out_ts;

    // [D] rmats_/tvecs_ push, currentGlobalCamera :574-595
    memcpy(t->Rlast, Rcurr, 9 * sizeof(float));
    memcpy(t->tlast, tcurr, 3 * sizeof(float));
    compute_global_camera(t, tcurr);
    if (t->cfg.dynamic_cube)  // :597-600; while parked its threshold is VOLUME_X (x 3 with -sm), :403
        kt_host_reposition_cube(Rcurr, t->tlast, t->cfg.volume_size, t->voxel_size,
                                t->parked ? (t->cfg.static_mode ? t->N * 3 : t->N) : t->cfg.voxel_shift, t->volume_basis);

    // place-recognition tap :601-624: sample now if the camera has moved enough since the last sample, else at the next shift
    bool shift_send = false;
    int is_loop = 0;
    if (t->cfg.place_recognition) {
        const float place_recognition_movement = 0.15f;   // KintinuousTracker.cpp:76
        if (kt_host_place_recognition_movement(Rcurr, t->current_global_camera, t->pr_rot, t->pr_trans) >= place_recognition_movement) {
            memcpy(t->pr_rot, Rcurr, sizeof(t->pr_rot));
            memcpy(t->pr_trans, t->current_global_camera, sizeof(t->pr_trans));
            add_pr_sample(t);
            is_loop = 1;
        } else {
            shift_send = true;
        }
    }

    // [F] shift decision :627-667 and the three axis blocks :669-833
    float current_translation[3];
    for (int k = 0; k < 3; ++k) current_translation[k] = t->tlast[k] - t->volume_basis[k];
    const int thresh = t->out_thresh;
    int vt[3];
    bool need_shift = false;
    for (int k = 0; k < 3; ++k) {
        vt[k] = voxel_trans(current_translation[k], t->voxel_size[k], thresh);
        need_shift = need_shift || vt[k] >= thresh || vt[k] <= -thresh;
    }
    if (speculated && need_shift != (t->mirror->skip == 1)) {
        kt_set_error("tracker: host and device disagree on the shift decision");
        return KT_ERR_STATE;
    }
    // skip == 2: the pose fell outside the margins the frame's task plan was made with -- the device parked the fusion kernels, the
    // frame is fused below through the in-stream pre-pass
    const bool plan_missed = speculated && t->mirror->skip == 2;
    if (speculated && t->plan_sel >= 0) {
        float dr = 0.0f, dt = 0.0f;
        const kt_tracker::PlanSlot& pl = t->plans[t->plan_sel];
        for (int k = 0; k < 9; ++k) dr += (Rcurr[k] - pl.R[k]) * (Rcurr[k] - pl.R[k]);
        for (int k = 0; k < 3; ++k) dt += (tcurr[k] - pl.t[k]) * (tcurr[k] - pl.t[k]);
        t->pred_err_r = sqrtf(dr) * 0.70710678f;   // |R - R^|_F ~ sqrt(2) angle
        t->pred_err_t = sqrtf(dt);
        if (plan_missed) ++t->plan_misses; else if (!need_shift) ++t->plan_hits;
    }
    t->plan_sel = -1;   // whatever is enqueued from here on for this frame runs its own pre-pass
    if (need_shift) {
        const int ov = t->cfg.overlap;
        KT_TRY(ev_begin(t, ST_SHIFT));
        for (int axis = 0; axis < 3; ++axis) {
            v_wrap_copy_update(t);
            bool cycled = false;
            int lo[3] = {0, 0, 0}, hi[3] = {N, N, N};
            int mlo[3] = {0, 0, 0}, mhi[3] = {N - 1, N - 1, N - 1};
            int dim = 0;
            if (vt[axis] >= thresh) {
                lo[axis] = 0; hi[axis] = vt[axis] + 1 + ov;
                dim = axis * 2;  // XPlus / YPlus / ZPlus, CloudSlice.h:33-36
                mlo[axis] = 0; mhi[axis] = vt[axis];   // the mesh: every cell with a corner in the planes that leave
                KT_TRY(fetch_slice(t, lo, hi, dim, mlo, mhi));
                KT_TRY(kt_clear_volume(c, t->tsdf, 2, N, axis, 0, t->voxel_wrap[axis], t->voxel_wrap[axis] + vt[axis]));
                KT_TRY(kt_clear_volume(c, t->color, 4, N, axis, 0, t->voxel_wrap[axis], t->voxel_wrap[axis] + vt[axis]));
                cycled = true;
            } else if (vt[axis] <= -thresh) {
                if (axis == 2) { lo[2] = N + (vt[2] - ov) - 1; hi[2] = N - 1; }  // z-minus off by one :805
                else { lo[axis] = N + (vt[axis] - ov); hi[axis] = N; }
                dim = axis * 2 + 1;
                mlo[axis] = N + vt[axis] - 1; mhi[axis] = N - 1;
                KT_TRY(fetch_slice(t, lo, hi, dim, mlo, mhi));
                KT_TRY(kt_clear_volume(c, t->tsdf, 2, N, axis, 1, t->voxel_wrap[axis], t->voxel_wrap[axis] + vt[axis]));
                KT_TRY(kt_clear_volume(c, t->color, 4, N, axis, 1, t->voxel_wrap[axis], t->voxel_wrap[axis] + vt[axis]));
                cycled = true;
            }
            if (cycled) {
                if (shift_send) {   // :706-717, :762-771, :816-825: the slab leaving the volume takes a sample with it
                    memcpy(t->pr_rot, Rcurr, sizeof(t->pr_rot));
                    memcpy(t->pr_trans, t->current_global_camera, sizeof(t->pr_trans));
                    t->slice.back().pr_id = add_pr_sample(t);
                    is_loop = 1;
                    shift_send = false;
                }
                // mutexOutCloudBuffer :1156-1208
                const float shift = t->voxel_size[axis] * (float)vt[axis];
                t->tlast[axis] -= shift;
                t->voxel_wrap[axis] += vt[axis];
                tcurr[axis] -= shift;
            }
        }
        v_wrap_copy_update(t);
        KT_TRY(ev_end(t, ST_SHIFT));
    }
    if (need_shift || !speculated || plan_missed) {
        // the fusion the device parked (or that was never enqueued), with the final pose and wrap
        v_wrap_copy_update(t);
        KT_TRY(launch_setup(t, 1, Rcurr, tcurr));
        KT_TRY(enqueue_fusion(t, t->out_set, t->out_depth, t->out_rgb, nullptr));
    }
    v_wrap_copy_update(t);
    ++t->global_time;
    push_pose(t, t->out_ts, Rcurr, is_loop);  // [K] :903-909
    // pose history for the next prediction (rotation and the shift-invariant global camera)
    memcpy(t->hist_R[0], t->hist_R[1], sizeof(t->hist_R[0])); memcpy(t->hist_gc[0], t->hist_gc[1], sizeof(t->hist_gc[0]));
    memcpy(t->hist_R[1], Rcurr, sizeof(t->hist_R[1])); memcpy(t->hist_gc[1], t->current_global_camera, sizeof(t->hist_gc[1]));
    if (t->hist_n < 2) ++t->hist_n;
    return KT_OK;
}

// Planning ahead.  Called in process_frame(f), before f's odometry is enqueued, for the frame f + 1 that has been read ahead: the host
// knows the poses of frames f - 1 and f - 2, predicts the pose of f + 1 by repeating the last motion increment twice
// (body-frame rotation increment, global-camera translation increment), and enqueues the voxel kernel's pre-pass for that prediction
// on plan_stream behind the frame's read-ahead -- where it runs next to the fusion kernels of frame f - 1.  Margins: three times the
// error of the previous prediction on top of a floor, within caps.  The set-up kernel of frame f + 1 checks its pose against them;
// a volume shift in between invalidates the plan (its storage wrap no longer matches).
// A frame set that leaves the pending list WITHOUT being processed (a skipped or dropped read-ahead) takes its plan with it: the slot is
// invalidated, and whatever recycles the set -- the main stream or the read-ahead stream -- first waits for the plan's kernels, which read
// the set's pixel records and tile maxima on plan_stream.
static int drop_plans_of_set(kt_tracker* t, int set)
{
    for (int k = 0; k < 3; ++k) {
        kt_tracker::PlanSlot& pl = t->plans[k];
        if (pl.ordinal < 0 || pl.set != set) continue;
        KT_HIP(hipStreamWaitEvent(t->ctx->stream, pl.done, 0));
        KT_HIP(hipStreamWaitEvent(t->pre_stream, pl.done, 0));
        pl.ordinal = -1; pl.set = -1;
    }
    return KT_OK;
}

// read-aheads [first, last) of the pending list will not be processed: their sets return to the pool once written, their plans go with them
static int retire_pending(kt_tracker* t, size_t first, size_t last)
{
    for (size_t i = first; i < last; ++i) {
        KT_HIP(hipStreamWaitEvent(t->ctx->stream, t->sets[t->pending[i].set].ready, 0));
        KT_TRY(drop_plans_of_set(t, t->pending[i].set));
    }
    t->pending.erase(t->pending.begin() + first, t->pending.begin() + last);
    return KT_OK;
}

static float plan_rand(kt_tracker* t)   // uniform in (-1, 1), deterministic per tracker
{
    t->plan_rng = t->plan_rng * 1664525u + 1013904223u;
    return (float)((t->plan_rng >> 8) & 0xffffffu) * (2.0f / 16777216.0f) - 1.0f;
}
static void plan_rand_unit(kt_tracker* t, float v[3])
{
    for (;;) {
        v[0] = plan_rand(t); v[1] = plan_rand(t); v[2] = plan_rand(t);
        const float n2 = v[0] * v[0] + v[1] * v[1] + v[2] * v[2];
        if (n2 > 0.01f && n2 <= 1.0f) { const float s = 1.0f / sqrtf(n2); v[0] *= s; v[1] *= s; v[2] *= s; return; }
    }
}

static int plan_ahead(kt_tracker* t, const Pending& next, long long ordinal)
{
    const int set = next.set;
    kt_tracker::PlanSlot& pl = t->plans[ordinal % 3];
    pl.ordinal = -1; pl.set = -1;
    float D[9], Rp[9], tp[3];
    for (int i = 0; i < 3; ++i)       // D = R(f-2)^T R(f-1)
        for (int j = 0; j < 3; ++j) D[i * 3 + j] = t->hist_R[0][0 * 3 + i] * t->hist_R[1][0 * 3 + j] + t->hist_R[0][1 * 3 + i] * t->hist_R[1][1 * 3 + j] + t->hist_R[0][2 * 3 + i] * t->hist_R[1][2 * 3 + j];
    for (int i = 0; i < 3; ++i)       // R^ = R(f-1) D
        for (int j = 0; j < 3; ++j) Rp[i * 3 + j] = t->Rlast[i * 3 + 0] * D[0 * 3 + j] + t->Rlast[i * 3 + 1] * D[1 * 3 + j] + t->Rlast[i * 3 + 2] * D[2 * 3 + j];
    float step = 0.0f, turn = 0.0f;
    for (int k = 0; k < 3; ++k) {
        const float d = t->hist_gc[1][k] - t->hist_gc[0][k];
        tp[k] = t->tlast[k] + d;
        step += d * d;
    }
    for (int k = 0; k < 9; ++k) turn += (D[k] - ((k % 4 == 0) ? 1.0f : 0.0f)) * (D[k] - ((k % 4 == 0) ? 1.0f : 0.0f));
    step = sqrtf(step); turn = sqrtf(turn) * 0.70710678f;
    if (t->plan_hits + t->plan_misses == 0) { t->pred_err_t = 0.5f * step; t->pred_err_r = 0.5f * turn; }   // nothing observed yet
    pl.tau = t->plan_margin_scale * fminf(0.020f, 0.0015f + 3.0f * t->pred_err_t);
    pl.theta = t->plan_margin_scale * fminf(0.02f, 3.0e-4f + 3.0f * t->pred_err_r);
    // ---- test hooks: where a plan can actually fail is a pose that lands just inside its margins
    if (t->plan_theta_fixed > 0.0f) pl.theta = t->plan_theta_fixed;
    if (t->plan_tau_fixed > 0.0f) pl.tau = t->plan_tau_fixed;
    if ((size_t)(ordinal + 1) * 12 <= t->plan_truth.size()) {   // the pose frame `ordinal` arrived at in an identical earlier run
        memcpy(Rp, &t->plan_truth[(size_t)ordinal * 12], sizeof(Rp));
        memcpy(tp, &t->plan_truth[(size_t)ordinal * 12 + 9], sizeof(tp));
    }
    if (t->plan_perturb) {   // prediction := prediction (+) a rotation of fr * theta about a random axis, + ft * tau along a random direction
        float ax[3], dir[3], K[9], Rd[9], Rn[9];
        plan_rand_unit(t, ax); plan_rand_unit(t, dir);
        const float phi = t->plan_fr * pl.theta, sn = sinf(phi), cs = cosf(phi);
        const float Kx[9] = {0, -ax[2], ax[1], ax[2], 0, -ax[0], -ax[1], ax[0], 0};
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) K[i * 3 + j] = Kx[i * 3 + 0] * Kx[0 * 3 + j] + Kx[i * 3 + 1] * Kx[1 * 3 + j] + Kx[i * 3 + 2] * Kx[2 * 3 + j];
        for (int k = 0; k < 9; ++k) Rd[k] = ((k % 4 == 0) ? 1.0f : 0.0f) + sn * Kx[k] + (1.0f - cs) * K[k];   // Rodrigues
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) Rn[i * 3 + j] = Rp[i * 3 + 0] * Rd[0 * 3 + j] + Rp[i * 3 + 1] * Rd[1 * 3 + j] + Rp[i * 3 + 2] * Rd[2 * 3 + j];
        memcpy(Rp, Rn, sizeof(Rp));
        for (int k = 0; k < 3; ++k) tp[k] += dir[k] * t->plan_ft * pl.tau;
    }
    kt_mat33 Rinv;
    kt_mat33_inverse(Rp, Rinv.m);
    v_wrap_copy_update(t);
    KT_HIP(hipStreamWaitEvent(t->plan_stream, t->sets[set].ready, 0));
    const int made = kt_integrate_plan(t->plan_stream, &pl.plan, t->sets[set].rec, t->sets[set].dpmax, t->cfg.cols, t->cfg.rows, &t->intr, t->volume_size, &Rinv, tp,
                                       t->tranc_dist, t->v_wrap_copy, t->N, pl.theta, pl.tau);
    if (made == KT_NO_PLAN) return KT_OK;   // margins too wide for this camera: planning is an optimisation, the frame takes the in-stream pre-pass
    KT_TRY(made);
    KT_HIP(hipEventRecord(pl.done, t->plan_stream));
    memcpy(pl.R, Rp, sizeof(pl.R)); memcpy(pl.t, tp, sizeof(pl.t));
    memcpy(pl.wrap, t->v_wrap_copy, sizeof(pl.wrap));
    pl.set = set; pl.depth = next.depth; pl.rgb = next.rgb;
    pl.ordinal = ordinal;
    return KT_OK;
}

// plan `frame` as the frame with this ordinal, if planning applies; sets plan_sel when the frame is the one being handed over (ordinal ==
// frames_started - 1 is decided by the caller: process_frame passes its own ordinal and takes plan_sel from the slot)
static int plan_frame(kt_tracker* t, const Pending& frame, long long ordinal)
{
    // (-d repositions the cube once the pose is known, a ground-truth trajectory supplies the pose on the host: nothing to plan for)
    if (!(t->plan_enabled && t->hist_n >= 2 && !t->cfg.dynamic_cube && !t->has_trajectory)) return KT_OK;
    // on a gated (dense) view the plan stream is held like the read-ahead: not beside the voxel kernel that is running now
    if (t->side_gate && t->gate_armed) KT_HIP(hipStreamWaitEvent(t->plan_stream, t->gate_ev, 0));
    v_wrap_copy_update(t);
    KT_TRY(plan_ahead(t, frame, ordinal));
    if (t->plans[ordinal % 3].ordinal == ordinal && ordinal == t->frames_started - 1) t->plan_sel = (int)(ordinal % 3);
    return KT_OK;
}

// Host half of the frame enqueued by the last kt_tracker_process_frame call: wait for its pose (the copy-stream event, NOT the
// fusion kernels), do the pose bookkeeping of KintinuousTracker.cpp:574-595, 903-909 and, when the volume has to shift
// (:627-833), run the shift and redo the fusion the device parked.  Called at the start of the next frame and by every getter.
// the ONE host wait of a frame: spin on the sequence word the set-up kernel posts after the odometry iterations (the GPU goes straight on
// to integrate / raycast meanwhile)
static int wait_for_pose(kt_tracker* t)
{
    const auto w0 = std::chrono::steady_clock::now();
    volatile unsigned int* seq = &t->mirror->seq;
    long long spins = 0;
    while (__atomic_load_n(seq, __ATOMIC_ACQUIRE) != t->frame_seq) {
        if ((++spins & 0xfff) == 0) {
            const double waited = std::chrono::duration<double>(std::chrono::steady_clock::now() - w0).count();
            if (waited > 30.0) {
                const hipError_t e = hipStreamQuery(t->ctx->stream);
                kt_set_error("tracker: no pose from the device after 30 s (stream status: %s)", hipGetErrorString(e));
                return KT_ERR_STATE;
            }
            if (waited > 0.002) std::this_thread::yield();
        }
    }
    t->host_wait_s += std::chrono::duration<double>(std::chrono::steady_clock::now() - w0).count();
    return KT_OK;
}

int complete_frame(kt_tracker* t)
{
    if (!t->outstanding) return KT_OK;
    t->outstanding = false;
    kt_ctx* c = t->ctx;
    KT_TRY(wait_for_pose(t));
    if (t->out_ordinal + 1 > t->frames_observed) t->frames_observed = t->out_ordinal + 1;
    ev_collect(t);
    if (t->mirror->handoff_timeout) {
        // An inter-workgroup hand-off of this frame's odometry gave up (kt_track.hip): the frame has no pose, and the set-up kernel parked its
        // fusion (skip = 1).  The reference's icpStep is stream-ordered and cannot fail this way (reduce.cu:347-419), so neither may the frame:
        // the hand-off buffer is refilled (a sweep that gave up leaves it undefined: kt_refill_granules) and the odometry runs again, one
        // launch per iteration, from the frame's starting pose -- rmats_ / tvecs_.back() have not moved, the frame set and the previous
        // frame's predicted maps are untouched -- followed by the set-up kernel and the fusion exactly as process_frame enqueued them.
        // Only if THAT chain reports a time-out as well (no co-residency is involved: a fault, not contention) is the frame an error.
        KT_TRY(kt_refill_granules(c));
        ++t->odo_fallbacks;
        t->icp_demote = t->icp_demote_len;
        if (t->icp_demote_len < 65536) t->icp_demote_len *= 2;
        select_set(t, t->out_set);
        const bool icp = !(t->cfg.use_rgbd || t->cfg.use_rgbd_icp);
        if (icp) KT_TRY(icp_odometry(t, true));
        else KT_TRY(rgbd_odometry(t, t->out_set, t->out_last_set, true));
        if (++t->frame_seq == 0) t->frame_seq = 1;
        KT_TRY(launch_setup(t, 0, nullptr, nullptr));
        if (t->out_speculated) KT_TRY(enqueue_fusion(t, t->out_set, t->out_depth, t->out_rgb, t->plan_sel >= 0 ? &t->plans[t->plan_sel].plan : nullptr));
        KT_TRY(wait_for_pose(t));
        if (t->mirror->handoff_timeout) {
            (void)kt_refill_granules(c);   // before the caller's next frame (or its reset) launches another reduction
            kt_set_error("odometry: inter-workgroup hand-off timed out (also in the stepwise re-run of the frame)");
            return KT_ERR_STATE;
        }
    }
    float Rcurr[9], tcurr[3];
    memcpy(Rcurr, t->mirror->R, sizeof(Rcurr));
    memcpy(tcurr, t->mirror->t, sizeof(tcurr));
    if (t->pose_log_on) {   // test hook: the pose the set-up kernel of frame out_ordinal saw (before any shift of this frame)
        if (t->pose_log.size() < (size_t)(t->out_ordinal + 1) * 12) t->pose_log.resize((size_t)(t->out_ordinal + 1) * 12, 0.0f);
        memcpy(&t->pose_log[(size_t)t->out_ordinal * 12], Rcurr, sizeof(Rcurr));
        memcpy(&t->pose_log[(size_t)t->out_ordinal * 12 + 9], tcurr, sizeof(tcurr));
    }
    return finish_pose(t, Rcurr, tcurr, t->out_speculated);
}

extern "C" {

static int process_frame_impl(kt_tracker* t, const uint16_t* depth_raw, const uint8_t* colors, uint64_t timestamp);

int kt_tracker_process_frame(kt_tracker* t, const uint16_t* depth_raw, const uint8_t* colors, uint64_t timestamp)
{
    KT_ARG(t && depth_raw && colors);
    const auto c0 = std::chrono::steady_clock::now();
    const int r = process_frame_impl(t, depth_raw, colors, timestamp);
    t->host_call_s += std::chrono::duration<double>(std::chrono::steady_clock::now() - c0).count();
    t->host_calls += 1;
    return r;
}

static int process_frame_impl(kt_tracker* t, const uint16_t* depth_raw, const uint8_t* colors, uint64_t timestamp)
{
    KT_TRY(complete_frame(t));
    kt_ctx* c = t->ctx;
    const bool gt = t->has_trajectory;
    if (gt && !t->trajectory.count((int)(uint32_t)timestamp)) {
        // GroundTruthOdometry::preRun :89-111, KintinuousTracker.cpp:460-463: a frame without a trajectory entry is not tracked at
        // all.  If it was read ahead, its set goes back to the pool once written.
        for (size_t i = 0; i < t->pending.size(); ++i)
            if (t->pending[i].depth == depth_raw && t->pending[i].rgb == colors) return retire_pending(t, i, i + 1);
        return KT_OK;
    }
    t->current_ts = timestamp;
    const int cols = t->cfg.cols, rows = t->cfg.rows, N = t->N;
    const bool icp = !gt && !(t->cfg.use_rgbd || t->cfg.use_rgbd_icp);
    const int angle_color = !t->cfg.disable_color_angle;

    // [A] pyramid build, KintinuousTracker.cpp:465-479 (+ scaleDepth records): taken from the prefetch stream if this frame
    // was announced with kt_tracker_prefetch_frame, otherwise computed here
    int set = -1;
    bool read_ahead = false;
    for (size_t i = 0; i < t->pending.size(); ++i)
        if (t->pending[i].depth == depth_raw && t->pending[i].rgb == colors) {
            read_ahead = true;
            KT_TRY(retire_pending(t, 0, i));   // read-aheads announced before this one were skipped by the caller
            set = t->pending.front().set;
            t->pending.erase(t->pending.begin());
            // a read-ahead that has already retired needs no device-side join (a wait packet is a 3-5 us bubble in front of the odometry)
            if (hipEventQuery(t->sets[set].ready) != hipSuccess) KT_HIP(hipStreamWaitEvent(c->stream, t->sets[set].ready, 0));
            break;
        }
    if (set < 0) {
        // not announced: build the set here (main-stream order protects the readers of whatever it overwrites)
        set = pick_free_set(t);
        if (set < 0) {  // both spare sets hold read-aheads the caller is not consuming: give up the older one
            set = t->pending.front().set;
            KT_TRY(retire_pending(t, 0, 1));
        }
        t->last_assigned = set;
        KT_TRY(ev_begin(t, ST_PYRAMID));
        KT_TRY(build_frame_set(t, c, set, depth_raw, colors));
        KT_TRY(ev_end(t, ST_PYRAMID));
    }
    select_set(t, set);
    const long long ordinal = t->frames_started;
    t->sets[set].user = t->frames_started++;
    for (int k = 0; k < KT_NSLOTS; ++k)
        if (depth_raw == t->depth_stage[k]) t->slot_frame[k] = ordinal;
    const int last_set = t->prev_set;   // "last" of RGBDOdometry for this frame
    t->prev_set = set;
    t->out_set = set;
    t->out_last_set = last_set;
    t->carry_sel ^= 1;                  // the state the previous tracked frame left becomes "before this frame"

    if (t->global_time == 0) {  // [B] :481-557
        kt_mat33 Rcam, Rcam_inv;
        memcpy(Rcam.m, t->Rlast, sizeof(Rcam.m));
        kt_mat33_inverse(Rcam.m, Rcam_inv.m);
        const int empty[3] = {0, 0, 0};
        if (t->counting) KT_HIP(hipMemsetAsync(t->upd_dev, 0, 16 * sizeof(unsigned int), c->stream));
        KT_TRY(launch_setup(t, 2, nullptr, nullptr));   // colour-weight carry only
        KT_TRY(ev_begin(t, ST_INTEGRATE));
        tsdf23_hook_arm(t);
        kt_integrate_job j = integrate_job(t, set, depth_raw, colors);
        j.Rcurr_inv = &Rcam_inv; j.tcurr = t->tlast; j.voxel_wrap = empty;
        KT_TRY(kt_integrate_tsdf_impl(c, j));
        KT_TRY(ev_end(t, ST_INTEGRATE));
        for (int l = 0; l < KT_LEVELS; ++l)
            KT_TRY(kt_transform_maps(c, t->vmaps_curr[l], t->nmaps_curr[l], lvl_cols(t, l), lvl_rows(t, l), &Rcam, t->tlast, t->vmaps_g_prev[l],
                                     t->nmaps_g_prev[l]));
        ++t->global_time;
        t->ev_par ^= 1;
        t->gt_utime = timestamp;   // :527-528
        KT_HIP(hipEventRecord(t->odo_ev[ordinal % KT_NODO], c->stream));
        if (t->cfg.place_recognition) add_pr_sample(t);   // :546-549: the first frame is always sampled (pose index 0)
        push_pose(t, timestamp, t->Rlast, 1);
        if (t->counting) {
            unsigned int u = 0;
            KT_HIP(hipMemcpyAsync(&u, t->upd_dev, sizeof(u), hipMemcpyDeviceToHost, c->stream));
            KT_HIP(hipStreamSynchronize(c->stream));
            t->last_U = u;
            t->last_S = 0;
        }
        return KT_OK;
    }

    t->out_ts = timestamp;
    t->out_set = set;
    t->out_depth = depth_raw;
    t->out_rgb = colors;
    t->out_thresh = t->parked ? INT_MAX : t->cfg.voxel_shift;
    if (gt) {
        // the pose comes from the trajectory, on the host: nothing to defer, nothing to speculate on
        float Rcurr[9], tcurr[3];
        ev_collect(t);
        ground_truth_pose(t, timestamp, Rcurr, tcurr);
        t->gt_utime = timestamp;   // :574-575
        KT_HIP(hipEventRecord(t->odo_ev[ordinal % KT_NODO], c->stream));   // before this frame's fusion, after the previous one's
        KT_TRY(finish_pose(t, Rcurr, tcurr, false));
        t->ev_par ^= 1;
        if (t->counting) KT_TRY(read_counts(t));
        return KT_OK;
    }

    // the voxel kernel's task plan, if one was made for this frame while the previous one was tracked and the volume has not
    // shifted since (plan_ahead)
    t->plan_sel = -1;
    v_wrap_copy_update(t);
    // The plan of THIS frame, made right here from the last pose the host has seen plus ONE increment (round 6; rounds 4-5 planned the read-ahead
    // frame, two increments out, behind that frame's read-ahead).  It runs on the plan stream beside the previous frame's fusion kernels, has this
    // frame's whole odometry launch to finish, and predicts one step instead of two -- a constant-velocity error grows with the square of the
    // horizon: tighter margins, fewer misses (221 / 1 against 214 / 2 on the orbit), and a plan made AFTER a shift instead of one the shift invalidates.
    // (-d repositions the cube once the pose is known: nothing to plan for.)
    // Made by whichever call sees the previous pose first: kt_tracker_prefetch_frame of the NEXT frame, when the caller announces in front of
    // the hand-over (plan_frame_to_come: the plan is then on its stream before the read-ahead's four launches are enqueued, ~15 us of host time
    // earlier -- it has the previous frame's fusion kernels to run beside, and what is still queued when the odometry launch takes the machine
    // waits that launch out and delays the set-up kernel), or this call.
    if (read_ahead) {
        const kt_tracker::PlanSlot& pl = t->plans[ordinal % 3];
        // a plan made for this ordinal belongs to this frame only if it was made from this frame's set and buffers (the caller may hand over
        // another announced frame than the one that was next in line) for the storage wrap that still holds
        if (pl.ordinal == ordinal && pl.set == set && pl.depth == depth_raw && pl.rgb == colors && memcmp(pl.wrap, t->v_wrap_copy, sizeof(t->v_wrap_copy)) == 0)
            t->plan_sel = (int)(ordinal % 3);
        else
            KT_TRY(plan_frame(t, Pending{depth_raw, colors, set, nullptr, nullptr}, ordinal));
    }
    // [C] odometry :564-572 -- every Gauss-Newton iteration is enqueued; the pose stays on the device
    v_wrap_copy_update(t);
    if (++t->frame_seq == 0) t->frame_seq = 1;  // 0 is the mirror's initial value (the set-up kernel posts the frame's seq)
    KT_TRY(ev_begin(t, ST_ODOMETRY));
    if (icp) KT_TRY(icp_odometry(t));
    else KT_TRY(rgbd_odometry(t, set, last_set));
    // device-side frame set-up (which also posts the pose into the host's PoseMirror), then the fusion kernels -- enqueued right
    // here, speculatively, on the assumption that the volume does not shift
    v_wrap_copy_update(t);
    // the plan has had the 19 launches above to finish; a join is enqueued only if it has not (a wait packet is a bubble)
    if (t->plan_sel >= 0 && hipEventQuery(t->plans[t->plan_sel].done) != hipSuccess) KT_HIP(hipStreamWaitEvent(c->stream, t->plans[t->plan_sel].done, 0));
    // gated side streams: what they were given for the NEXT frame (its read-ahead, then its plan) ends before this frame's voxel kernel starts
    // -- one wait packet in front of the set-up kernel (3-5 us; the gate is on where the frame is a millisecond)
    if (t->side_gate && !t->pending.empty()) KT_HIP(hipStreamWaitEvent(c->stream, t->sets[t->pending.front().set].ready, 0));
    KT_TRY(launch_setup(t, 0, nullptr, nullptr));
    // -d: the cube may be repositioned once the pose is known, which changes the shift decision -- nothing to speculate on
    t->out_speculated = !t->cfg.dynamic_cube;
    if (t->out_speculated) KT_TRY(enqueue_fusion(t, set, depth_raw, colors, t->plan_sel >= 0 ? &t->plans[t->plan_sel].plan : nullptr));
    t->outstanding = true;
    t->out_ordinal = ordinal;
    t->gt_utime = timestamp;
    if (!t->out_speculated) KT_TRY(complete_frame(t));   // observe the pose, reposition, shift if needed, enqueue the fusion
    t->ev_par ^= 1;
    if (t->counting) {  // the counters are read back per frame: finish it before returning
        KT_TRY(complete_frame(t));
        KT_TRY(read_counts(t));
    }
    return KT_OK;
}

static int prefetch_impl(kt_tracker* t, const uint16_t* depth_raw, const uint8_t* colors, const uint16_t* depth_host, const uint8_t* rgb_host);

int kt_tracker_prefetch_frame(kt_tracker* t, const uint16_t* depth_raw, const uint8_t* colors)
{
    KT_ARG(t && depth_raw && colors);
    return prefetch_impl(t, depth_raw, colors, nullptr, nullptr);
}

// stage a host frame into the next slot: pinned copy, then the upload on `stream`
static int stage_host_frame(kt_tracker* t, hipStream_t stream, const uint16_t* depth_host, const uint8_t* rgb_host, int* slot_out)
{
    const size_t P = (size_t)t->cfg.cols * t->cfg.rows;
    const int slot = t->next_slot;
    t->next_slot = (t->next_slot + 1) % KT_NSLOTS;
    KT_HIP(hipEventSynchronize(t->slot_uploaded[slot]));   // the pinned copy of the frame that used this slot 4 frames ago has left
    KT_TRY(wait_frame_consumed(t, stream, t->slot_frame[slot]));   // ... and its fusion has read the device copy
    t->slot_frame[slot] = -1;
    memcpy(t->depth_stage_host[slot], depth_host, P * sizeof(uint16_t));
    memcpy(t->rgb_stage_host[slot], rgb_host, P * 3);
    KT_HIP(hipMemcpyAsync(t->depth_stage[slot], t->depth_stage_host[slot], P * sizeof(uint16_t), hipMemcpyHostToDevice, stream));
    KT_HIP(hipMemcpyAsync(t->rgb_stage[slot], t->rgb_stage_host[slot], P * 3, hipMemcpyHostToDevice, stream));
    KT_HIP(hipEventRecord(t->slot_uploaded[slot], stream));
    *slot_out = slot;
    return KT_OK;
}

int kt_tracker_prefetch_frame_host(kt_tracker* t, const uint16_t* depth_host, const uint8_t* rgb_host)
{
    KT_ARG(t && depth_host && rgb_host);
    if (t->pending.size() >= 2) { kt_set_error("kt_tracker_prefetch_frame_host: two read-ahead frames are already outstanding"); return KT_ERR_STATE; }
    KT_TRY(complete_frame(t));
    int slot;
    KT_TRY(stage_host_frame(t, t->pre_stream, depth_host, rgb_host, &slot));   // the upload rides the read-ahead stream too
    return prefetch_impl(t, t->depth_stage[slot], t->rgb_stage[slot], depth_host, rgb_host);
}

static int prefetch_impl(kt_tracker* t, const uint16_t* depth_raw, const uint8_t* colors, const uint16_t* depth_host, const uint8_t* rgb_host)
{
    if (t->pending.size() >= 2) { kt_set_error("kt_tracker_prefetch_frame: two read-ahead frames are already outstanding"); return KT_ERR_STATE; }
    // Observe the pose of the frame in flight first (the next kt_tracker_process_frame call would wait for it anyway).  After that,
    // with F = frames handed over so far, everything enqueued before the end of odometry(F - 1) has retired: fusion(F - 2) and the
    // RGB-D "last" reads of odometry(F - 1).  So a set last consumed by frame <= F - 2 is free; the set of frame F - 1 (its fusion
    // may still run, and it is RGB-D "last" for frame F) and the sets of outstanding read-aheads are not.
    KT_TRY(complete_frame(t));
    // the frame that will be handed over next is known (announced earlier) and so is the pose in front of it: plan it NOW, before this frame's
    // read-ahead goes to its stream (process_frame_impl: "made by whichever call sees the previous pose first")
    if (!t->pending.empty() && t->plans[t->frames_started % 3].ordinal != t->frames_started) KT_TRY(plan_frame(t, t->pending.front(), t->frames_started));
    const int set = pick_free_set(t);   // exists: 3 sets, at most 1 other read-ahead outstanding here
    if (set < 0) { kt_set_error("kt_tracker_prefetch_frame: no free frame set"); return KT_ERR_STATE; }
    t->last_assigned = set;
    KT_TRY(wait_frame_consumed(t, t->pre_stream, t->sets[set].user));
    t->pre_ctx.device = t->ctx->device;
    if (t->side_gate && t->gate_armed) {
        // the frame just observed is in its voxel kernel now: hold the read-ahead (and, behind its `ready` event, the plan stream) until
        // that launch has drained -- the event enqueue_fusion recorded between the voxel kernel and the ray cast
        KT_HIP(hipStreamWaitEvent(t->pre_stream, t->gate_ev, 0));
    }
    KT_TRY(build_frame_set(t, &t->pre_ctx, set, depth_raw, colors));
    KT_HIP(hipEventRecord(t->sets[set].ready, t->pre_stream));
    t->pending.push_back(Pending{depth_raw, colors, set, depth_host, rgb_host});
    return KT_OK;
}

int kt_tracker_process_frame_host(kt_tracker* t, const uint16_t* depth_host, const uint8_t* rgb_host, uint64_t timestamp)
{
    // TrackerInterface::process upload, TrackerInterface.cpp:90-91 (pinned staging + async copies instead of blocking cudaMemcpy2D)
    KT_ARG(t && depth_host && rgb_host);
    for (const Pending& p : t->pending)   // announced with kt_tracker_prefetch_frame_host: already on the device
        if (p.depth_host == depth_host && p.rgb_host == rgb_host) return kt_tracker_process_frame(t, p.depth, p.rgb, timestamp);
    KT_TRY(complete_frame(t));
    int slot;
    KT_TRY(stage_host_frame(t, t->ctx->stream, depth_host, rgb_host, &slot));
    return kt_tracker_process_frame(t, t->depth_stage[slot], t->rgb_stage[slot], timestamp);
}

// KintinuousTracker::loadTrajectory (KintinuousTracker.cpp:216-260) minus the text parsing: pose7 = n x {x y z qx qy qz qw}.
// T.setIdentity(); T.pretranslate(t).rotate(q): linear = Quaternionf::toRotationMatrix() (no normalisation), translation = t.
int kt_tracker_load_trajectory(kt_tracker* t, int n, const uint64_t* utimes, const float* pose7)
{
    KT_ARG(t && n >= 0 && (n == 0 || (utimes && pose7)));
    KT_TRY(complete_frame(t));
    t->has_trajectory = true;
    for (int i = 0; i < n; ++i) {
        std::array<float, 12> T;
        kt_host_trajectory_pose(pose7 + (size_t)i * 7, T.data());
        t->trajectory[(int)(uint32_t)utimes[i]] = T;
    }
    t->gt_utime = 0;   // :259
    return KT_OK;
}

int kt_tracker_finalise(kt_tracker* t)
{
    // finalise :1003-1048
    KT_ARG(t);
    KT_TRY(complete_frame(t));
    v_wrap_copy_update(t);
    const int lo[3] = {0, 0, 0}, hi[3] = {t->N, t->N, t->N};
    const int mhi[3] = {t->N - 1, t->N - 1, t->N - 1};
    KT_TRY(fetch_slice(t, lo, hi, 7 /* CloudSlice::FINAL */, lo, mhi));
    if (t->cfg.place_recognition) {   // :1035-1045: the final slice carries one more sample, taken at the last pose
        memcpy(t->pr_rot, t->Rlast, sizeof(t->pr_rot));
        memcpy(t->pr_trans, t->current_global_camera, sizeof(t->pr_trans));
        t->slice.back().pr_id = add_pr_sample(t);
        t->pr_samples.back().pose_index = (int)t->poses.size() - 1;   // no new pose follows: it belongs to the last one
    }
    return KT_OK;
}

int kt_tracker_set_parked(kt_tracker* t, int parked)
{
    KT_ARG(t);
    KT_TRY(complete_frame(t));
    t->parked = parked != 0;
    return KT_OK;
}

}  // extern "C"
