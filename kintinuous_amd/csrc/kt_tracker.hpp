// kt_tracker.hpp -- private to the tracker's three units: struct kt_tracker and the few functions that cross between them.
//   kt_tracker.hip          the frame pipeline (create / reset, process_frame, odometry, set-up kernel, fusion, shift, planning, read-ahead)
//   kt_tracker_slices.hip   kt_slice_store: the slabs that leave the volume (worker thread, slab buffers, slice / mesh / key stages, their C ABI)
//   kt_tracker_api.hip      the read-only getters and debug hooks
// C++ linkage, like kt_internal.hpp; nothing here is part of the boundary.
#pragma once

#include "kt_internal.hpp"

#include <array>
#include <condition_variable>
#include <deque>
#include <map>
#include <mutex>
#include <thread>
#include <vector>

struct DensePose { uint64_t ts; float pose[16]; int is_loop; };   // KintinuousTracker.h:151-169
struct PrSample { uint64_t utime; float trans[3], rot[9]; int pose_index; };   // PlaceRecognitionInput.h:30-56, minus the frame bytes

// Everything computed from the input frame alone (bilateral + pyramids + scaleDepth records): two sets, so the set of frame
// k + 1 can be filled on the prefetch stream while frame k is tracked and fused on the main stream.
struct FrameSet {
    uint16_t* depths[KT_LEVELS];
    float *vmaps[KT_LEVELS], *nmaps[KT_LEVELS];
    void* rec;            // per-pixel integrate records (kt_integrate_prepare)
    float* dpmax;         // per 32 x 32 pixel tile: largest |scaled depth| (interval pre-pass prune)
    float* scaled;        // depthRawScaled_
    // RGB-D odometry inputs derived from the frame alone (RGBDOdometry.cpp:140-158, 186, 296-300); a frame is "next" while it is
    // tracked and "last" for its successor, so the sets double as RGBDOdometry's lastDepth / nextDepth ... buffers
    float* depth_m[KT_LEVELS];        // metric depth pyramid
    uint8_t* image[KT_LEVELS];        // intensity pyramid
    int16_t *dIdx[KT_LEVELS], *dIdy[KT_LEVELS];
    uint8_t* cand[KT_LEVELS];         // pixels that can yield a photometric correspondence when the frame is "next" (pose-independent tests)
    float* cloud[KT_LEVELS];          // projectToPointCloud of depth_m (used when the frame is "last")
    hipEvent_t ready;     // recorded on the prefetch stream when the set is complete
    long long user = -1;  // ordinal of the process_frame call that last consumed the set (-1: none)
};
// Three sets rotate: the frame whose fusion is still running (also RGB-D "last" of its successor), the frame about to be tracked
// and the frame being read ahead.  A set is recycled behind odo_ev (wait_frame_consumed).
#define KT_NSETS 3

typedef struct kt_pose_mirror PoseMirror;   // csrc/kt_setup.hpp: the host's window on the frame in flight
struct Pending { const uint16_t* depth; const uint8_t* rgb; int set; const uint16_t* depth_host; const uint8_t* rgb_host; };
#define KT_NSLOTS 4   // host-frame staging: frame in flight + two read-aheads + the one being filled
#define KT_NODO 8     // ring of "odometry of frame f enqueued" events

enum { ST_PYRAMID = 0, ST_ODOMETRY, ST_SHIFT, ST_INTEGRATE, ST_RAYCAST, ST_RESIZE, ST_TSDF23, ST_COUNT };

// Events that only order one stream of this device behind another: no timing, no system-scope fence (the cache write-back of the
// default record is a 6 us bubble on the main stream; kernel boundaries already order device memory between streams of one agent).
#ifndef KT_EV_DEVICE
#define KT_EV_DEVICE (hipEventDisableTiming | hipEventDisableSystemFence)
#endif

// One slab on its way out (kt_slice_store::fetch): the two boxes and what the tracker holds at that moment.  The arrays are the caller's.
struct kt_slice_request {
    const int *lo, *hi;        // voxels [lo, hi) of the cloud
    const int *mlo, *mhi;      // cells [mlo, mhi) of the mesh
    int dim;                   // CloudSlice::Dimension
    const int16_t* volume; const uint8_t* color; const float* volume_size; const int *v_wrap_copy, *voxel_wrap;
    const float *Rlast, *current_global_camera; uint64_t current_ts;   // rmats_.back(), currentGlobalCamera, current_utime: KintinuousTracker.cpp:1186-1191
};

// The slabs that leave the volume, and everything that moves them to the host off the frame's critical path.  The pipeline sees fetch()
// at a shift and at finalise, back() for the sample a slab takes with it, join() / clear() at a reset and shutdown() before its kt_mem is
// released; the rest is reached through the kt_tracker_slice_* / kt_tracker_enable_* calls (kt_tracker_slices.hip).
// Who may touch what:
//   * slices[i] belongs to the worker from fetch() until the job of its buffer is waited for (wait_job / join); before that the calling
//     thread reads and writes only dim, R, cam, ts and pr_id, which the worker never touches.  at(i, true) joins first.
//   * slab i uses buffer b = i & 1 of every array below (cloud_next alternates); fetch() waits for the buffer's previous job, two slabs back,
//     before anything is enqueued into it.
//   * the buffers are pinned memory of the tracker's kt_mem: shutdown() (join, then the worker) comes before that is released, and the
//     enable_* calls join before they give an array back.
// Value-initialised with the tracker (new kt_tracker()): a store that was never created shuts down cleanly.
struct kt_slice_store {
    struct Slice {      // CloudSlice.h:28-129 (cloud + dimension; processed = CloudSlice::processedCloud when the slice stage is on)
        std::vector<kt_point_xyzrgb> pts; int dim; float R[9], cam[3]; uint64_t ts; int pr_id;
        std::vector<kt_point_xyzrgbnormal> processed; bool has_processed = false;
        // the slab's mesh when the mesh stage is on (kt_mesh.hip): true sizes (-1 = stage off), the arrays when they fitted the bounds
        std::vector<kt_mesh_vertex> mesh_v; std::vector<uint32_t> mesh_t; long long mesh_nv = -1, mesh_nt = -1; bool mesh_fit = false;
        std::vector<uint64_t> mesh_k; bool mesh_keyed = false;   // its vertices' edge keys, when it was meshed with keys on (kt_tracker_enable_mesh_keys)
    };
    struct SliceJob { bool active; bool done = true; size_t slice; hipError_t status; };
    // what the worker needs to move one slab into its slice, by value (null mev / psrc / mk: that stage was off)
    struct Download {
        Slice* dst; SliceJob* job; hipEvent_t ev, mev;
        const kt_point_xyzrgb* src; const unsigned int* cnt; size_t cap;
        const kt_point_xyzrgbnormal* psrc; const unsigned int* pcnt;
        const kt_mesh_vertex* mv; const uint32_t* mt; const unsigned long long* mcnt; size_t mcap_v, mcap_t; const unsigned long long* mk;
    };

    int create(kt_ctx* ctx, kt_mem* mem, int N, size_t cloud_cap, float leaf);   // the worker, the two slab buffers (from `mem`)
    int warm_up(const int16_t* volume, const uint8_t* color, const float volume_size[3]);   // the extraction kernel's first launch, on one voxel
    void shutdown();                        // join, stop the worker, destroy the two workspaces; before mem->release()
    int fetch(const kt_slice_request& q);   // extraction (+ stages) enqueued, a new slice appended, its download handed to the worker
    int wait_job(int b);                    // the download that uses buffer b, if any, has ended; its status
    int join();                             // ... both
    void clear() { slices.clear(); }        // (after join)
    size_t size() const { return slices.size(); }
    int at(int i, bool joined, const Slice** out);   // slice i, its points and meshes complete when `joined`
    Slice& back() { return slices.back(); }
    int enable_slice_stage(int on, int weight_cull, int k);
    int enable_mesh_stage(int on, long long max_vertices, long long max_triangles);
    int enable_mesh_keys(int on);
    int mesh_overflow(int i, const Slice& s) const;   // KT_ERR_CAPACITY and its message

private:
    int mesh_keys_reserve();
    void download(const Download& d);

    kt_ctx* ctx; kt_mem* mem;
    int N; size_t cloud_cap; float leaf;   // the volume's edge; points per slab buffer; the slice stage's voxel-grid leaf (CloudSliceProcessor.cpp:124-130)
    std::deque<Slice> slices;          // a deque: the download thread fills slices[i].pts while new slices may be appended
    // Slice download off the frame's critical path.  The extraction kernel writes the points into pinned host memory (two buffers,
    // alternating), the count follows by an asynchronous copy and an event; a helper thread waits for the event and copies the n points
    // into the slice while the main thread has long gone on enqueueing the clears and the fusion.  Getters join.
    // ONE worker thread per tracker, started at creation (where it also pays HIP's per-thread set-up): a thread per shift put its
    // creation and, worse, its first hipSetDevice -- which takes the runtime's lock for up to a millisecond -- into the shift frame
    // (frame period of the first shift of a run: 1.44 ms against 0.47-0.56 later; r03 call 16).
    SliceJob jobs[2];
    std::thread worker;
    std::mutex wmu;
    std::condition_variable wcv, wdone;
    std::deque<Download> wq;
    bool wstop;
    kt_point_xyzrgb* cloud_host[2]; unsigned int* cloud_count_host[2]; hipEvent_t cloud_ev[2];
    int cloud_next;
    // The CloudSliceProcessor stage behind a shift, on the device (kt_slice.hip; kt_tracker_enable_slice_stage): the extraction then
    // writes into device memory, and a stream of its own takes the slab from there -- raw points to pinned host memory, the stage, the
    // processed points to pinned host memory -- while the main stream goes on with the clears and the fusion.
    bool slice_stage; int slice_cull, slice_k;
    kt_slice_ws* slice_ws;
    kt_point_xyzrgb* cloud_dev[2]; unsigned int* cloud_count_dev[2]; hipEvent_t extracted[2];
    kt_point_xyzrgbnormal* proc_host[2]; unsigned int* proc_count_host[2];
    // The mesh stage (kt_tracker_enable_mesh_stage): marching cubes of the slab on the context stream between the extraction and the
    // clears, written straight into pinned host memory (two buffers, alternating with the cloud's); its sizes follow by a copy and an
    // event that the slice's helper-thread job waits for as well.
    bool mesh_stage; size_t mesh_cap_v, mesh_cap_t;
    kt_mesh_ws* mesh_ws;
    kt_mesh_vertex* mesh_v_host[2]; uint32_t* mesh_t_host[2]; unsigned long long* mesh_count_host[2]; hipEvent_t mesh_ev[2];
    // ... and, with kt_tracker_enable_mesh_keys, the vertices' edge keys beside them: mesh_k_cap entries per buffer, = mesh_cap_v once taken
    bool mesh_keys; size_t mesh_k_cap; unsigned long long* mesh_k_host[2];
};

struct kt_tracker {
    kt_ctx* ctx;
    kt_mem mem;                        // every buffer, pinned mirror, event and stream below, the slice store's included (the three workspaces and the plans own theirs)
    kt_tracker_config cfg;
    kt_intr intr;
    int N;
    float volume_size[3], voxel_size[3];
    float tranc_dist;
    float volume_basis[3];
    float initial_rotation[9];
    int voxel_wrap[3], v_wrap_copy[3];
    int global_time;
    uint64_t current_ts = 0;
    // -p ground-truth odometry: camera_trajectory (KintinuousTracker.h:237; its comparator is std::less<int>, so the keys are the
    // timestamps narrowed to int) and current_utime as GroundTruthOdometry sees it (the previous tracked frame's timestamp)
    bool has_trajectory = false;
    std::map<int, std::array<float, 12>> trajectory;   // R row-major [0..8], t [9..11]
    uint64_t gt_utime = 0;
    bool parked;
    float Rlast[9], tlast[3];          // rmats_.back(), tvecs_.back()
    float current_global_camera[3];
    // device buffers (KintinuousTracker.h:185-222)
    int16_t* tsdf; uint8_t* color;
    uint16_t* depths_curr[KT_LEVELS];
    float *vmaps_curr[KT_LEVELS], *nmaps_curr[KT_LEVELS], *vmaps_g_prev[KT_LEVELS], *nmaps_g_prev[KT_LEVELS];
    uint8_t* vmap_curr_color;
    float* depth_raw_scaled;
    void* rec_curr;                    // integrate records of the current frame (set member, like the *_curr maps above)
    // the *_curr pointers above alias sets[cur_set]
    FrameSet sets[KT_NSETS];
    int last_assigned = KT_NSETS - 1;  // set handed to the most recent frame (prefetched or inline)
    std::vector<Pending> pending;      // prefetched frames not yet processed (at most 2)
    long long frames_started;          // process_frame calls so far
    long long frames_observed;         // 1 + ordinal of the latest frame whose pose the host has seen in the mirror (complete_frame)
    long long out_ordinal = -1;        // ordinal of the frame in flight (t->outstanding)
    hipEvent_t guard_ev;               // only for out-of-pattern read-aheads (see kt_tracker_prefetch_frame)
    // odo_ev[f % KT_NODO]: recorded on the main stream between fusion(f - 1) and fusion(f), in -p mode only -- there the host never
    // waits for a pose, so a lagging GPU's fusion could otherwise read a frame set the read-ahead stream has recycled (wait_frame_consumed).
    hipEvent_t odo_ev[8];
    static_assert(KT_NSLOTS == 4, "slot_frame's initialiser");
    long long slot_frame[KT_NSLOTS] = {-1, -1, -1, -1};   // ordinal of the frame that consumed staging slot k (-1: none)
    hipStream_t pre_stream;
    kt_ctx pre_ctx;                    // the context with pre_stream as its stream (image kernels only)
    // RGBDOdometry buffers (RGBDOdometry.h:96-111)
    int prev_set;                      // set of the previous frame ("last" of RGBDOdometry), -1 before the first frame
    kt_dataterm* corres[KT_LEVELS];
    // device-resident Gauss-Newton state + pinned mirror
    kt_track_state* state_dev; kt_track_state* state_host;
    // staging for the host-frame entry point
    // KT_NSLOTS rotating slots: pinned host copy + device copy of one frame, an event recorded after its upload
    uint16_t* depth_stage[KT_NSLOTS]; uint8_t* rgb_stage[KT_NSLOTS];
    uint16_t* depth_stage_host[KT_NSLOTS]; uint8_t* rgb_stage_host[KT_NSLOTS];  // pinned
    hipEvent_t slot_uploaded[KT_NSLOTS];
    int next_slot;
    // outputs
    std::vector<DensePose> poses;
    kt_slice_store slice;              // the slabs that left the volume (kt_tracker_slices.hip)
    // place-recognition tap (KintinuousTracker.h:216, 248-249): pose of the last sampled frame, the samples
    float pr_rot[9], pr_trans[3];
    std::vector<PrSample> pr_samples;
    // deferred completion: a frame's fusion kernels are enqueued before the host has seen its pose (complete_frame)
    bool outstanding; uint64_t out_ts; int out_set;
    const uint16_t* out_depth; const uint8_t* out_rgb; int out_thresh;
    bool out_speculated;               // the fusion kernels of the frame in flight were enqueued against the device's shift decision
    kt_frame_params* fp_dev;
    // colour weight carried across frames for pixels without a valid normal (KT_REC_STALE_NZ): [carry_sel] = state before the frame
    // in flight, [carry_sel ^ 1] = state after it
    float* wrkc_carry[2]; int carry_sel;
    // Planning ahead (kt_volume.hip): the voxel kernel's task plan of a read-ahead frame is made for a PREDICTED pose on plan_stream at the start of
    // the frame's kt_tracker_process_frame call -- before its odometry is enqueued, one increment past the last pose the host has seen -- and has the
    // odometry launch to finish.  plan_sel: the slot the frame in flight was enqueued with, -1 = none (the in-stream pre-pass ran).
    // (set / depth / rgb / wrap: what the plan was built from -- kept for drop_plans_of_set and the debug state)
    struct PlanSlot { kt_tsdf_plan plan; hipEvent_t done; long long ordinal = -1; float R[9], t[3], theta, tau; int wrap[3]; int set = -1; const uint16_t* depth; const uint8_t* rgb; };
    bool icp_levels;   // ICP-only odometry: one launch per pyramid level (kt_icp_level_kernel) instead of one per iteration, while this tracker is alone
    bool last_icp_levels;   // ... and whether the last frame's chain took that form
    bool counted;           // this tracker is in kt_live_trackers (a create that failed early is not)
    // A hand-off time-out is not the end of the frame (round 6): complete_frame re-runs the frame's odometry in the stepwise form, and the
    // level form stays off for icp_demote more frames (doubling per relapse: something -- another process on the GPU, a CU-masked queue --
    // keeps its grid from being resident; the stepwise chain needs no co-residency and gives the same bits).
    int icp_demote, icp_demote_len = 64;
    long long odo_fallbacks;   // frames whose odometry was re-run (kt_tracker_odometry_fallbacks)
    int out_last_set = -1;     // RGB-D "last" set of the frame in flight (for that re-run)
    // Side-stream gate (round 6).  The read-ahead of frame f + 1 is enqueued the moment the host has seen the pose of frame f - 1 -- exactly
    // when that frame's voxel kernel starts -- and the voxel kernel is a fixed grid of 8192 waves that fills EVERY wave slot of the chip and
    // deals its task list statically over them: one foreign wave on one SIMD keeps one of its workgroups out until another has finished, and
    // the launch is as long as its slowest SIMD (farwall768: 0.49 ms by the kernel trace with nothing beside it, 0.67 with a single sleeping
    // wave of another stream resident -- profiles/r06_experiments.md, call 4; 0.85 next to the 1280x960 read-ahead).  With the gate on, the
    // read-ahead stream waits for an event recorded between the voxel kernel and the ray cast (one marker packet on the main stream: 3-5 us of
    // a millisecond frame), so the read-ahead runs beside the ray cast -- whose workgroups are handed out dynamically -- and the next odometry.
    // (A first cut had the side stream start with a one-thread kernel sleeping on a device flag the ray cast set -- no packet on the main
    // stream; that resident wave was itself the disturbance.)
    hipEvent_t gate_ev; bool gate_armed; int side_gate;   // side_gate: 0 off, 1 on
    PlanSlot plans[3]; hipStream_t plan_stream;          // (three: frame f is planned while the voxel kernels of f - 1 and f - 2 may still read theirs)
    int plan_sel; bool plan_enabled; float plan_margin_scale;
    // test hooks (kt_tracker_debug_plan_*): the pose every frame WILL arrive at, taken from an identical earlier run, as the prediction;
    // an offset of fr * theta about a random axis and ft * tau along a random direction on top of the prediction; fixed margins; a log
    // of the poses the set-up kernels saw
    std::vector<float> plan_truth; float plan_fr = 0.0f, plan_ft = 0.0f, plan_theta_fixed = 0.0f, plan_tau_fixed = 0.0f; bool plan_perturb = false;
    unsigned int plan_rng = 0x9e3779b9u; std::vector<float> pose_log; bool pose_log_on = false;
    float hist_R[2][9], hist_gc[2][3]; int hist_n;      // rotation and global camera of the two most recent tracked frames
    float pred_err_t, pred_err_r;                       // error of the most recent prediction (metres, radians): drives the margins
    long long plan_hits, plan_misses;
    unsigned char* bricks;             // negative-brick flags of the volume (tsdf23 raises, kt_volume.hip; raycast skips, kt_raycast.hip)
    float *vgz_dev, *zs_dev;           // z tables of integrate (kt_integrate_tables)
    PoseMirror* mirror;                // pinned + mapped host memory
    unsigned int frame_seq;            // sequence number of the frame in flight (PoseMirror::seq)
    long long prof_frames;             // frames seen with profiling == 1 / 5 (the tsdf23 event pair is recorded on every 8th / 4th)
    // profiling / counters (events double-buffered by frame parity: a pair is read one frame after it was recorded)
    double host_wait_s, host_call_s; long long host_calls;   // where the host thread spends a frame (kt_tracker_host_times)
    int profiling; int ev_par;
    hipEvent_t ev[2][ST_COUNT][2]; bool ev_rec[2][ST_COUNT];
    double stage_ms_sum[ST_COUNT]; long long stage_n[ST_COUNT]; float stage_ms_last[ST_COUNT];
    int counting;
    unsigned int* upd_dev; unsigned long long* steps_dev;
    unsigned long long last_U, last_S;
};

// kt_tracker.hip, for the other two units
int complete_frame(kt_tracker* t);   // host half of the frame in flight, if any: every getter starts here
void ev_collect(kt_tracker* t);      // harvest the profiling event pairs that have completed
