// kt_tracker_slices.hip -- kt_slice_store (kt_tracker.hpp): the slabs that leave the cyclical volume at a shift and at finalise
// (fetchCloud + download, TSDFVolume.cpp:135-172, KintinuousTracker.cpp:1156-1208), their way to the host behind the frame's critical
// path, the optional slice / mesh / key stages behind the extraction, and the C ABI that reads them (kt_tracker_slice_*,
// kt_tracker_enable_*).  Host code only: the kernels are those of kt_volume_shift.hip, kt_slice.hip and kt_mesh.hip.
#include "kt_tracker.hpp"

#include <string.h>

typedef kt_slice_store::Slice Slice;

int kt_slice_store::create(kt_ctx* ctx_, kt_mem* mem_, int N_, size_t cloud_cap_, float leaf_)
{
    ctx = ctx_; mem = mem_; N = N_; cloud_cap = cloud_cap_; leaf = leaf_;
    const int device = ctx->device;
    worker = std::thread([this, device]() {
        (void)hipSetDevice(device);
        std::unique_lock<std::mutex> lk(wmu);
        for (;;) {
            wcv.wait(lk, [this]() { return wstop || !wq.empty(); });
            if (wq.empty()) return;   // stop requested and nothing left to do
            const Download d = wq.front();
            wq.pop_front();
            lk.unlock();
            download(d);
            lk.lock();
            wdone.notify_all();
        }
    });
    for (int b = 0; b < 2; ++b) {
        KT_TRY(mem->pinned(&cloud_host[b], cloud_cap));
        KT_TRY(mem->pinned(&cloud_count_host[b], 1));
        KT_TRY(mem->event(&cloud_ev[b], hipEventDisableTiming));
    }
    return KT_OK;
}

// the extraction kernel's first launch, on one voxel, at creation instead of in the first shift frame (tracker_create_impl)
int kt_slice_store::warm_up(const int16_t* volume, const uint8_t* color, const float volume_size[3])
{
    const int zero[3] = {0, 0, 0};
    return kt_extract_cloud_slice_async(ctx, volume, volume_size, cloud_host[0], cloud_cap, zero, color, 0, 1, 0, 1, 0, 1, 1, zero, N, &ctx->counters[1]);
}

void kt_slice_store::shutdown()
{
    (void)join();
    if (worker.joinable()) {
        { std::lock_guard<std::mutex> lk(wmu); wstop = true; }
        wcv.notify_all();
        worker.join();
    }
    (void)kt_slice_ws_destroy(slice_ws); (void)kt_mesh_ws_destroy(mesh_ws);
}

int kt_slice_store::wait_job(int b)
{
    SliceJob& j = jobs[b];
    if (!j.active) return KT_OK;
    { std::unique_lock<std::mutex> lk(wmu); wdone.wait(lk, [&j]() { return j.done; }); }
    j.active = false;
    if (j.status != hipSuccess) { kt_set_error("slice download: %s", hipGetErrorString(j.status)); return KT_ERR_HIP; }
    return KT_OK;
}

// wait for the slice downloads in flight (every reader of slices[i].pts goes through here)
int kt_slice_store::join()
{
    int rc = KT_OK;
    for (int b = 0; b < 2; ++b)
        if (wait_job(b) != KT_OK) rc = KT_ERR_HIP;
    return rc;
}

int kt_slice_store::at(int i, bool joined, const Slice** out)
{
    KT_ARG(i >= 0 && i < (int)slices.size());
    if (joined) KT_TRY(join());
    *out = &slices[i];
    return KT_OK;
}

// the worker's half of fetch(): the slab's events have fired, its arrays move from the pinned buffers into the slice
void kt_slice_store::download(const Download& d)
{
    Slice* dst = d.dst;
    hipError_t e = hipEventSynchronize(d.ev);   // the kernel's stores to host memory and the count are complete
    if (e == hipSuccess && d.mev) e = hipEventSynchronize(d.mev);
    if (e != hipSuccess) d.job->status = e;
    else {
        size_t n = (size_t)*d.cnt;
        if (n > d.cap) n = d.cap;
        dst->pts.assign(d.src, d.src + n);
        if (d.psrc) {
            size_t m = (size_t)*d.pcnt;
            if (m > d.cap) m = d.cap;
            dst->processed.assign(d.psrc, d.psrc + m);
            dst->has_processed = true;
        }
        if (d.mev) {
            const unsigned long long tot = *d.mcnt;
            dst->mesh_nv = (long long)(tot & 0xffffffffull);
            dst->mesh_nt = (long long)(tot >> 32);
            dst->mesh_fit = (size_t)dst->mesh_nv <= d.mcap_v && (size_t)dst->mesh_nt <= d.mcap_t && dst->mesh_nv <= (1ll << 29);
            dst->mesh_keyed = d.mk != nullptr;
            if (dst->mesh_fit) {
                dst->mesh_v.assign(d.mv, d.mv + dst->mesh_nv);
                dst->mesh_t.assign(d.mt, d.mt + 3 * dst->mesh_nt);
                if (d.mk) dst->mesh_k.assign(d.mk, d.mk + dst->mesh_nv);
            }
        }
    }
    std::lock_guard<std::mutex> lk(wmu);
    d.job->done = true;
}

// Nothing here waits for the GPU: the kernel, the copy of its count and an event are enqueued, and the worker moves the points into the
// slice once the event has fired.  With the mesh stage on, the box of cells [mlo, mhi) is meshed right behind the extraction, in stream
// order before the caller's clears.
int kt_slice_store::fetch(const kt_slice_request& q)
{
    kt_ctx* c = ctx;
    const int b = cloud_next;
    cloud_next ^= 1;
    KT_TRY(wait_job(b));   // the download that used this buffer two slices ago
    const bool stage = slice_stage;
    if (!stage) {
        KT_TRY(kt_extract_cloud_slice_async(c, q.volume, q.volume_size, cloud_host[b], cloud_cap, q.v_wrap_copy, q.color, q.lo[0], q.hi[0],
                                            q.lo[1], q.hi[1], q.lo[2], q.hi[2], 1, q.voxel_wrap, N, &c->counters[1]));
        KT_HIP(hipMemcpyAsync(cloud_count_host[b], &c->counters[1], sizeof(unsigned int), hipMemcpyDeviceToHost, c->stream));
        KT_HIP(hipEventRecord(cloud_ev[b], c->stream));
    } else {
        // the slab stays on the device; everything behind the extraction kernel runs on the slice stage's own stream
        hipStream_t ss = (hipStream_t)kt_slice_ws_stream(slice_ws);
        KT_TRY(kt_extract_cloud_slice_async(c, q.volume, q.volume_size, cloud_dev[b], cloud_cap, q.v_wrap_copy, q.color, q.lo[0], q.hi[0],
                                            q.lo[1], q.hi[1], q.lo[2], q.hi[2], 1, q.voxel_wrap, N, cloud_count_dev[b]));
        KT_HIP(hipEventRecord(extracted[b], c->stream));
        KT_HIP(hipStreamWaitEvent(ss, extracted[b], 0));
        KT_TRY(kt_copy_counted(ss, cloud_dev[b], cloud_host[b], cloud_count_dev[b], (unsigned int)cloud_cap, (int)sizeof(kt_point_xyzrgb), cloud_count_host[b]));
        KT_TRY(kt_slice_process_device(slice_ws, cloud_dev[b], cloud_count_dev[b], cloud_cap, slice_cull, leaf, slice_k));
        KT_TRY(kt_copy_counted(ss, kt_slice_ws_output(slice_ws), proc_host[b], kt_slice_ws_leaves_dev(slice_ws), (unsigned int)cloud_cap,
                               (int)sizeof(kt_point_xyzrgbnormal), proc_count_host[b]));
        KT_HIP(hipEventRecord(cloud_ev[b], ss));
    }
    const bool mesh = mesh_stage;
    const bool keyed = mesh && mesh_keys;
    if (mesh) {
        KT_TRY(kt_mesh_enqueue(mesh_ws, c->stream, q.volume, q.color, q.volume_size, q.v_wrap_copy, q.mlo, q.mhi, q.voxel_wrap, N,
                               mesh_v_host[b], mesh_cap_v, mesh_t_host[b], mesh_cap_t, keyed ? mesh_k_host[b] : nullptr));
        KT_HIP(hipMemcpyAsync(mesh_count_host[b], kt_mesh_ws_total(mesh_ws), sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
        KT_HIP(hipEventRecord(mesh_ev[b], c->stream));
    }
    slices.emplace_back();
    Slice& s = slices.back();   // references into a deque survive push_back
    s.dim = q.dim;
    s.pr_id = -1;
    memcpy(s.R, q.Rlast, sizeof(s.R));
    memcpy(s.cam, q.current_global_camera, sizeof(s.cam));
    s.ts = q.current_ts;
    SliceJob& j = jobs[b];
    j.slice = slices.size() - 1;
    j.status = hipSuccess;
    j.active = true;
    j.done = false;
    const Download d = {&s, &j, cloud_ev[b], mesh ? mesh_ev[b] : nullptr,
                        cloud_host[b], cloud_count_host[b], cloud_cap,
                        stage ? proc_host[b] : nullptr, stage ? proc_count_host[b] : nullptr,
                        mesh_v_host[b], mesh_t_host[b], mesh_count_host[b], mesh_cap_v, mesh_cap_t, keyed ? mesh_k_host[b] : nullptr};
    {
        std::lock_guard<std::mutex> lk(wmu);
        wq.push_back(d);
    }
    wcv.notify_one();
    return KT_OK;
}

int kt_slice_store::enable_slice_stage(int on, int weight_cull, int k)
{
    KT_TRY(join());
    if (on && !slice_ws) {
        // A failure leaves the stage off and what was taken with the tracker (kt_tracker_destroy releases it); the next call takes what is missing.
        slice_stage = false;
        for (int b = 0; b < 2; ++b) {
            if (!cloud_dev[b]) KT_TRY(mem->device(&cloud_dev[b], cloud_cap));
            if (!cloud_count_dev[b]) KT_TRY(mem->device(&cloud_count_dev[b], 1));
            if (!proc_host[b]) KT_TRY(mem->pinned(&proc_host[b], cloud_cap));
            if (!proc_count_host[b]) KT_TRY(mem->pinned(&proc_count_host[b], 1));
            if (!extracted[b]) KT_TRY(mem->event(&extracted[b], KT_EV_DEVICE));
        }
        KT_TRY(kt_slice_ws_create(ctx, cloud_cap, nullptr, &slice_ws));
        // the stage's kernels (the library sort needs scratch memory, which the runtime allocates at a kernel's first launch) run once
        // here, on an empty slab, so that the first shift does not pay for it
        KT_HIP(hipMemsetAsync(cloud_count_dev[0], 0, sizeof(unsigned int), (hipStream_t)kt_slice_ws_stream(slice_ws)));
        KT_TRY(kt_slice_process_device(slice_ws, cloud_dev[0], cloud_count_dev[0], cloud_cap, weight_cull, leaf, k));
        KT_HIP(hipStreamSynchronize((hipStream_t)kt_slice_ws_stream(slice_ws)));
    }
    slice_stage = on != 0;
    slice_cull = weight_cull; slice_k = k;
    return KT_OK;
}

// the key arrays follow the vertex arrays' bound; nothing reads the old ones (the callers have joined the slice jobs)
int kt_slice_store::mesh_keys_reserve()
{
    if (!mesh_keys || mesh_k_cap == mesh_cap_v) return KT_OK;
    mesh_k_cap = 0;
    for (int b = 0; b < 2; ++b) {
        mem->drop(mesh_k_host[b]); mesh_k_host[b] = nullptr;
        KT_TRY(mem->pinned(&mesh_k_host[b], mesh_cap_v));
    }
    mesh_k_cap = mesh_cap_v;
    return KT_OK;
}

int kt_slice_store::enable_mesh_keys(int on)
{
    KT_TRY(join());
    mesh_keys = false;   // (a failure below leaves the keys off)
    if (on) {
        mesh_keys = true;
        const int s = mesh_keys_reserve();
        if (s != KT_OK) { mesh_keys = false; return s; }
    }
    return KT_OK;
}

int kt_slice_store::enable_mesh_stage(int on, long long max_vertices, long long max_triangles)
{
    KT_TRY(join());
    if (on) {
        mesh_stage = false;   // (a failure below leaves the stage off; the next call takes what is missing)
        const size_t cv = max_vertices > 0 ? (size_t)max_vertices : 8 * (size_t)N * (size_t)N;
        const size_t ct = max_triangles > 0 ? (size_t)max_triangles : 2 * cv;
        if (!mesh_ws) {   // the largest box is the final one, [0, N - 1)^3
            size_t voxels = 0, runs = 0;
            const int lo[3] = {0, 0, 0}, hi[3] = {N - 1, N - 1, N - 1};
            KT_TRY(kt_mesh_check(lo, hi, N, &voxels, &runs));
            KT_TRY(kt_mesh_ws_reserve(&mesh_ws, voxels, runs));
        }
        if (cv != mesh_cap_v || ct != mesh_cap_t) {   // other bounds: nothing reads the old arrays (join above)
            mesh_cap_v = mesh_cap_t = 0;
            for (int b = 0; b < 2; ++b) {
                mem->drop(mesh_v_host[b]); KT_TRY(mem->pinned(&mesh_v_host[b], cv));
                mem->drop(mesh_t_host[b]); KT_TRY(mem->pinned(&mesh_t_host[b], ct * 3));
            }
            mesh_cap_v = cv; mesh_cap_t = ct;
        }
        KT_TRY(mesh_keys_reserve());
        for (int b = 0; b < 2; ++b) {
            if (!mesh_count_host[b]) KT_TRY(mem->pinned(&mesh_count_host[b], 1));
            if (!mesh_ev[b]) KT_TRY(mem->event(&mesh_ev[b], hipEventDisableTiming));
        }
    }
    mesh_stage = on != 0;
    return KT_OK;
}

int kt_slice_store::mesh_overflow(int i, const Slice& s) const
{
    kt_set_error("slice %d: its mesh (%lld vertices, %lld triangles) exceeded the mesh stage's bounds (%zu / %zu)", i, s.mesh_nv, s.mesh_nt, mesh_cap_v,
                 mesh_cap_t);
    return KT_ERR_CAPACITY;
}

// ---- C ABI ----------------------------------------------------------------------------------------------------------------------
// The preamble of every slice getter: the tracker and the caller's pointers that are checked before anything else (args), the frame in
// flight completed, the pointers that are checked only then (late_args) with the index, and -- for point and mesh data -- the join.
static int slice_of(kt_tracker* t, int i, bool args, bool late_args, bool joined, const Slice** s)
{
    KT_ARG(t && args);
    KT_TRY(complete_frame(t));
    KT_ARG(late_args);
    return t->slice.at(i, joined, s);
}

extern "C" {

/* (a negative count = the frame in flight could not be completed: kt_last_error() says why) */
int kt_tracker_num_slices(kt_tracker* t) { return (t && complete_frame(t) == KT_OK) ? (int)t->slice.size() : -1; }
int kt_tracker_slice_pr_id(kt_tracker* t, int i, int* pr_id)
{
    const Slice* s;
    KT_TRY(slice_of(t, i, pr_id != nullptr, true, false, &s));
    *pr_id = s->pr_id;
    return KT_OK;
}
int kt_tracker_slice_info(kt_tracker* t, int i, size_t* n_points, int* dimension)
{
    const Slice* s;
    KT_TRY(slice_of(t, i, true, n_points && dimension, true, &s));
    *n_points = s->pts.size();
    *dimension = s->dim;
    return KT_OK;
}
int kt_tracker_slice_pose(kt_tracker* t, int i, float* R, float* cam, uint64_t* ts)
{
    const Slice* s;
    KT_TRY(slice_of(t, i, true, true, false, &s));
    if (R) memcpy(R, s->R, 9 * sizeof(float));
    if (cam) memcpy(cam, s->cam, 3 * sizeof(float));
    if (ts) *ts = s->ts;
    return KT_OK;
}
int kt_tracker_slice_points(kt_tracker* t, int i, kt_point_xyzrgb* out)
{
    const Slice* s;
    KT_TRY(slice_of(t, i, true, out != nullptr, true, &s));
    if (!s->pts.empty()) memcpy(out, s->pts.data(), s->pts.size() * sizeof(kt_point_xyzrgb));
    return KT_OK;
}

/* The CloudSliceProcessor stage (weight cull, voxel grid at the voxel size, k-NN normals: kt_slice_process_device) behind every slab the
 * tracker extracts from now on, on a stream of its own; the processed points travel with the slice (kt_tracker_slice_processed). */
int kt_tracker_enable_slice_stage(kt_tracker* t, int on, int weight_cull, int k)
{
    KT_ARG(t && (!on || (k >= 1 && k <= 64)));
    KT_TRY(complete_frame(t));
    return t->slice.enable_slice_stage(on, weight_cull, k);
}
/* number of processed points of slice i, or -1 when the slice was extracted without the stage */
int kt_tracker_slice_processed_info(kt_tracker* t, int i, long long* n_points)
{
    const Slice* s;
    KT_TRY(slice_of(t, i, n_points != nullptr, true, true, &s));
    *n_points = s->has_processed ? (long long)s->processed.size() : -1;
    return KT_OK;
}
int kt_tracker_slice_processed(kt_tracker* t, int i, kt_point_xyzrgbnormal* out)
{
    const Slice* s;
    KT_TRY(slice_of(t, i, out != nullptr, true, true, &s));
    KT_ARG(s->has_processed);
    if (!s->processed.empty()) memcpy(out, s->processed.data(), s->processed.size() * sizeof(kt_point_xyzrgbnormal));
    return KT_OK;
}

int kt_tracker_enable_mesh_keys(kt_tracker* t, int on)
{
    KT_ARG(t);
    KT_TRY(complete_frame(t));
    return t->slice.enable_mesh_keys(on);
}
int kt_tracker_slice_mesh_keys(kt_tracker* t, int i, uint64_t* keys)
{
    const Slice* s;
    KT_TRY(slice_of(t, i, true, true, true, &s));
    if (s->mesh_nv < 0 || !s->mesh_keyed) { kt_set_error("slice %d was meshed without keys (kt_tracker_enable_mesh_keys)", i); return KT_ERR_STATE; }
    if (!s->mesh_fit) return t->slice.mesh_overflow(i, *s);
    KT_ARG(keys || s->mesh_k.empty());
    if (!s->mesh_k.empty()) memcpy(keys, s->mesh_k.data(), s->mesh_k.size() * sizeof(uint64_t));
    return KT_OK;
}

int kt_tracker_enable_mesh_stage(kt_tracker* t, int on, long long max_vertices, long long max_triangles)
{
    KT_ARG(t && max_vertices >= 0 && max_triangles >= 0);
    KT_TRY(complete_frame(t));
    return t->slice.enable_mesh_stage(on, max_vertices, max_triangles);
}
/* true sizes of slice i's mesh, -1 when the slice was taken with the mesh stage off */
int kt_tracker_slice_mesh_info(kt_tracker* t, int i, long long* n_vertices, long long* n_triangles)
{
    const Slice* s;
    KT_TRY(slice_of(t, i, n_vertices && n_triangles, true, true, &s));
    *n_vertices = s->mesh_nv;
    *n_triangles = s->mesh_nt;
    return KT_OK;
}
int kt_tracker_slice_mesh(kt_tracker* t, int i, kt_mesh_vertex* vertices, uint32_t* triangles)
{
    const Slice* s;
    KT_TRY(slice_of(t, i, true, true, true, &s));
    KT_ARG(s->mesh_nv >= 0);
    if (!s->mesh_fit) return t->slice.mesh_overflow(i, *s);
    KT_ARG((vertices || s->mesh_v.empty()) && (triangles || s->mesh_t.empty()));
    if (!s->mesh_v.empty()) memcpy(vertices, s->mesh_v.data(), s->mesh_v.size() * sizeof(kt_mesh_vertex));
    if (!s->mesh_t.empty()) memcpy(triangles, s->mesh_t.data(), s->mesh_t.size() * sizeof(uint32_t));
    return KT_OK;
}

}  // extern "C"
