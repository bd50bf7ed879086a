// kt_tracker_api.hip -- the tracker's getters, counters and debug hooks (C ABI; kt_debug.h for the hooks): each completes the frame in
// flight where its answer depends on it, then reads struct kt_tracker (kt_tracker.hpp).  Nothing here enqueues a frame's work; the frame
// pipeline is kt_tracker.hip, the slices' getters are in kt_tracker_slices.hip.  Host code only.
#include "kt_tracker.hpp"

#include <string.h>

extern "C" {

/* mean seconds per kt_tracker_process_frame call since the last reset of the statistics: {total in the call, of which waiting for
 * the previous frame's pose}; the difference is enqueue work */
int kt_tracker_host_times(kt_tracker* t, double out2[2], int reset)
{
    KT_ARG(t && out2);
    out2[0] = t->host_calls ? t->host_call_s / (double)t->host_calls : 0.0;
    out2[1] = t->host_calls ? t->host_wait_s / (double)t->host_calls : 0.0;
    if (reset) { t->host_call_s = t->host_wait_s = 0.0; t->host_calls = 0; }
    return KT_OK;
}

int kt_tracker_get_volume_basis(kt_tracker* t, float* basis)
{
    KT_ARG(t && basis);
    KT_TRY(complete_frame(t));
    memcpy(basis, t->volume_basis, sizeof(t->volume_basis));
    return KT_OK;
}

/* (a negative count = the frame in flight could not be completed: kt_last_error() says why) */
int kt_tracker_num_pr_samples(kt_tracker* t) { return (t && complete_frame(t) == KT_OK) ? (int)t->pr_samples.size() : -1; }
int kt_tracker_pr_sample(kt_tracker* t, int i, uint64_t* utime, float* trans, float* rotation, int* pose_index)
{
    KT_ARG(t && utime && trans && rotation && pose_index);
    KT_TRY(complete_frame(t));
    KT_ARG(i >= 0 && i < (int)t->pr_samples.size());
    const PrSample& ps = t->pr_samples[i];
    *utime = ps.utime;
    memcpy(trans, ps.trans, sizeof(ps.trans));
    memcpy(rotation, ps.rot, sizeof(ps.rot));
    *pose_index = ps.pose_index;
    return KT_OK;
}

int kt_tracker_get_pose(kt_tracker* t, float* R, float* tv, float* gc)
{
    KT_ARG(t && R && tv && gc);
    KT_TRY(complete_frame(t));
    memcpy(R, t->Rlast, sizeof(t->Rlast));
    memcpy(tv, t->tlast, sizeof(t->tlast));
    memcpy(gc, t->current_global_camera, sizeof(t->current_global_camera));
    return KT_OK;
}
int kt_tracker_num_poses(kt_tracker* t) { return (t && complete_frame(t) == KT_OK) ? (int)t->poses.size() : -1; }
int kt_tracker_get_dense_pose(kt_tracker* t, int i, uint64_t* ts, float* pose16, int* is_loop)
{
    KT_ARG(t);
    KT_TRY(complete_frame(t));
    KT_ARG(t && i >= 0 && i < (int)t->poses.size() && ts && pose16 && is_loop);
    *ts = t->poses[i].ts;
    memcpy(pose16, t->poses[i].pose, sizeof(t->poses[i].pose));
    *is_loop = t->poses[i].is_loop;
    return KT_OK;
}
int kt_tracker_get_voxel_wrap(kt_tracker* t, int* wrap)
{
    KT_ARG(t && wrap);
    KT_TRY(complete_frame(t));
    memcpy(wrap, t->voxel_wrap, sizeof(t->voxel_wrap));
    return KT_OK;
}
int16_t* kt_tracker_volume(kt_tracker* t) { return (t && complete_frame(t) == KT_OK) ? t->tsdf : nullptr; }
uint8_t* kt_tracker_color_volume(kt_tracker* t) { return (t && complete_frame(t) == KT_OK) ? t->color : nullptr; }
float* kt_tracker_vmap_g_prev(kt_tracker* t, int l) { return (t && l >= 0 && l < KT_LEVELS && complete_frame(t) == KT_OK) ? t->vmaps_g_prev[l] : nullptr; }
float* kt_tracker_nmap_g_prev(kt_tracker* t, int l) { return (t && l >= 0 && l < KT_LEVELS && complete_frame(t) == KT_OK) ? t->nmaps_g_prev[l] : nullptr; }
uint8_t* kt_tracker_vmap_curr_color(kt_tracker* t) { return (t && complete_frame(t) == KT_OK) ? t->vmap_curr_color : nullptr; }
float kt_tracker_trunc_dist(kt_tracker* t) { return t ? t->tranc_dist : 0.f; }

int kt_tracker_enable_profiling(kt_tracker* t, int on)
{
    KT_ARG(t);
    KT_TRY(complete_frame(t));
    KT_HIP(hipStreamSynchronize(t->ctx->stream));
    ev_collect(t);
    t->profiling = on;
    memset(t->stage_ms_sum, 0, sizeof(t->stage_ms_sum));
    memset(t->stage_n, 0, sizeof(t->stage_n));
    return KT_OK;
}
int kt_tracker_stage_ms(kt_tracker* t, float* ms)
{
    KT_ARG(t && ms);
    KT_TRY(complete_frame(t));
    KT_HIP(hipStreamSynchronize(t->ctx->stream));
    ev_collect(t);
    for (int s = 0; s < ST_COUNT; ++s) ms[s] = t->stage_n[s] ? (float)(t->stage_ms_sum[s] / (double)t->stage_n[s]) : 0.f;
    return KT_OK;
}
int kt_tracker_stage_counts(kt_tracker* t, long long* n)
{
    KT_ARG(t && n);
    for (int s = 0; s < ST_COUNT; ++s) n[s] = t->stage_n[s];
    return KT_OK;
}
int kt_tracker_enable_counts(kt_tracker* t, int on)
{
    KT_ARG(t);
    t->counting = on;
    return KT_OK;
}
int kt_tracker_debug_state(kt_tracker* t, float* out29)
{
    KT_ARG(t && out29);
    KT_TRY(complete_frame(t));
    KT_HIP(hipStreamSynchronize(t->ctx->stream));
    KT_HIP(hipMemcpy(t->state_host, t->state_dev, sizeof(kt_track_state), hipMemcpyDeviceToHost));
    memcpy(out29, t->state_host->icp29, 29 * sizeof(float));
    return KT_OK;
}

int kt_tracker_odometry_fallbacks(kt_tracker* t, long long* out)
{
    KT_ARG(t && out);
    KT_TRY(complete_frame(t));
    *out = t->odo_fallbacks;
    return KT_OK;
}

int kt_tracker_plan_stats(kt_tracker* t, long long out2[2])
{
    KT_ARG(t && out2);
    KT_TRY(complete_frame(t));
    out2[0] = t->plan_hits; out2[1] = t->plan_misses;
    return KT_OK;
}
/* test hooks of the planned-ahead voxel pass (tests/test_gpu_tracker.py::test_plan_margins_*): */
int kt_tracker_debug_pose_log(kt_tracker* t, int enable, float* out12n, int max_frames, int* n_frames)
{
    KT_ARG(t);
    if (enable >= 0) t->pose_log_on = enable != 0;
    if (out12n || n_frames) {
        KT_TRY(complete_frame(t));
        const int n = (int)(t->pose_log.size() / 12);
        if (n_frames) *n_frames = n;
        if (out12n) memcpy(out12n, t->pose_log.data(), sizeof(float) * 12 * (size_t)(n < max_frames ? n : max_frames));
    }
    return KT_OK;
}
int kt_tracker_debug_plan_truth(kt_tracker* t, const float* poses12n, int n_frames, float fr, float ft, float theta_fixed, float tau_fixed, unsigned int seed)
{
    KT_ARG(t && n_frames >= 0 && (poses12n || n_frames == 0) && fr >= 0 && ft >= 0 && theta_fixed >= 0 && tau_fixed >= 0);
    t->plan_truth.assign(poses12n, poses12n + (size_t)n_frames * 12);
    t->plan_fr = fr; t->plan_ft = ft; t->plan_perturb = fr > 0.0f || ft > 0.0f;
    t->plan_theta_fixed = theta_fixed; t->plan_tau_fixed = tau_fixed;
    t->plan_rng = seed * 2654435761u + 0x9e3779b9u;
    return KT_OK;
}

int kt_tracker_debug_counts(kt_tracker* t, unsigned int* out4)
{
    KT_ARG(t && out4);
    KT_HIP(hipMemcpy(out4, t->upd_dev, 8 * sizeof(unsigned int), hipMemcpyDeviceToHost));
    { unsigned long long h[3] = {0, 0, 0}; KT_HIP(hipMemcpy(h, t->steps_dev + 1, sizeof(h), hipMemcpyDeviceToHost)); out4[7] = (unsigned int)h[0]; out4[5] = (unsigned int)h[1]; out4[6] = (unsigned int)h[2]; }
    return KT_OK;
}
// test hook: the negative-brick flags as they stand behind every frame handed in so far (tests/test_gpu_bricks.py)
int kt_tracker_debug_bricks(kt_tracker* t, unsigned char* out_host)
{
    KT_ARG(t && out_host);
    KT_TRY(complete_frame(t));
    KT_HIP(hipMemcpyAsync(out_host, t->bricks, kt_brick_count(t->N), hipMemcpyDeviceToHost, t->ctx->stream));
    KT_HIP(hipStreamSynchronize(t->ctx->stream));
    return KT_OK;
}
int kt_tracker_last_counts(kt_tracker* t, unsigned long long* U, unsigned long long* S)
{
    KT_ARG(t && U && S);
    *U = t->last_U;
    *S = t->last_S;
    return KT_OK;
}

int kt_tracker_export_poses_device(kt_tracker* t, int k, float* dst_dev)
{
    KT_ARG(t);
    KT_TRY(complete_frame(t));
    KT_ARG(k > 0 && dst_dev && k <= (int)t->poses.size());
    std::vector<float> tmp((size_t)k * 16);
    for (int i = 0; i < k; ++i) memcpy(&tmp[(size_t)i * 16], t->poses[t->poses.size() - k + i].pose, 16 * sizeof(float));
    KT_HIP(hipMemcpyAsync(dst_dev, tmp.data(), tmp.size() * sizeof(float), hipMemcpyHostToDevice, t->ctx->stream));
    KT_HIP(hipStreamSynchronize(t->ctx->stream));
    return KT_OK;
}

int kt_tracker_debug_icp_levels(kt_tracker* t) { return t && t->last_icp_levels ? 1 : 0; }
int kt_tracker_debug_side_gate(kt_tracker* t) { return t ? t->side_gate : 0; }

}  // extern "C"
