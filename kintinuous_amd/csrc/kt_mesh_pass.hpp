// kt_mesh_pass.hpp -- the host skeleton of the post-passes over the -m mesh (kt_mesh_weld.hip, kt_mesh_simplify.hip, kt_mesh_normals.hip,
// kt_mesh_components.hip, kt_mesh_holes.hip, kt_mesh_smooth.hip) and of its rasteriser (kt_mesh_render.hip).  A new
// post-pass uses this instead of a copy.
//
// A pass object is a kt_pass_head (the result words, which never grow) followed by kt_groups.  A group owns its buffers through a kt_mem
// of its own, every buffer an allocation of its own, taken on the first call that needs it.  Both forms of a call check their arguments
// before anything is allocated or enqueued (KT_ERR_ARG, nothing written), enqueue every pass on the object's stream and wait once; the
// host-array form is kt_mesh_host_form around the _device form.  The sorted key list of the passes that sort is kt_mesh_keys.hpp, the
// device rules they share (run heads, half-edge classes, vertex validity, fixed point) are kt_wave.hpp's.
#pragma once

#include "kt_internal.hpp"

#include <algorithm>

// ---- the object: `struct pass : kt_pass_head { res, res_host, groups... }`, made by `new pass()` (value-initialised: every pointer starts null) ----
struct kt_pass_head {
    kt_mem mem;                       // what never grows: the result words
    kt_ctx* ctx;
    hipStream_t stream;
    ~kt_pass_head() { mem.release(); }
};

// drains the stream and deletes: the groups release in reverse order of declaration, the head's words last
template <class T>
int kt_pass_destroy(T* w)
{
    if (!w) return KT_OK;
    if (w->stream) (void)hipStreamSynchronize(w->stream);
    delete w;
    return KT_OK;
}

// w->res: device, res_words; w->res_host: pinned, host_words
template <class T>
int kt_pass_create(kt_ctx* c, void* hip_stream, T** out, size_t res_words, size_t host_words)
{
    KT_ARG(c && out);
    *out = nullptr;
    KT_HIP(hipSetDevice(c->device));
    T* w = new T();
    w->ctx = c; w->stream = hip_stream ? (hipStream_t)hip_stream : c->stream;
    int s = w->mem.device(&w->res, res_words);
    if (s == KT_OK) s = w->mem.pinned(&w->res_host, host_words);
    if (s != KT_OK) { (void)kt_pass_destroy(w); return s; }
    *out = w;
    return KT_OK;
}

// ---- a group of buffers that grows.  P: a plain struct of the group's pointers (and any size derived with them, such as rocprim's
// byte count), reset by value; D: the capacities the group is sized by.  The rule of the side stages: nothing when every wanted
// capacity fits; otherwise drain the stream, release, forget every pointer, and allocate at the larger of the old and the wanted
// capacity per dimension -- alloc(mem, pointers, capacities) -> status; a failure leaves the group empty. ----
template <class P, int D = 1>
struct kt_group : P {
    kt_mem mem;
    size_t cap[D];
    ~kt_group() { mem.release(); }
    template <class A>
    int grow(hipStream_t stream, const size_t (&want)[D], A alloc)
    {
        size_t c[D];
        bool fits = true;
        for (int d = 0; d < D; ++d) { fits = fits && want[d] <= cap[d]; c[d] = std::max(want[d], cap[d]); }
        if (fits) return KT_OK;
        KT_HIP(hipStreamSynchronize(stream));
        forget();
        const int s = alloc(mem, static_cast<P&>(*this), (const size_t*)c);
        if (s != KT_OK) { forget(); return s; }
        std::copy(c, c + D, cap);
        return KT_OK;
    }
private:
    void forget() { mem.release(); static_cast<P&>(*this) = P(); std::fill(cap, cap + D, (size_t)0); }
};

// ---- the span table of a call, device and pinned.  For S spans: S 64-bit words of the pass's own in front (the weld's times; room for
// them is always kept), then as 32-bit words the S + 1 first vertices and the S + 1 first output vertices.  upload() before the passes
// (the call before has been waited for, so the pinned copy is free), download() behind them, get() after the wait. ----
struct kt_span_words { unsigned long long *dev, *host; };
struct kt_span_table : kt_group<kt_span_words> {
    size_t S, lead;                   // of the last upload: spans, 64-bit words in front
    int upload(hipStream_t st, const size_t* span_first, int n_spans, const uint64_t* span_time = nullptr)
    {
        KT_TRY(grow(st, {(size_t)n_spans}, [](kt_mem& m, kt_span_words& p, const size_t* c) {
            int s = m.device(&p.dev, 2 * c[0] + 1);
            if (s == KT_OK) s = m.pinned(&p.host, 2 * c[0] + 1);
            return s;
        }));
        S = (size_t)n_spans; lead = span_time ? S : 0;
        unsigned int* hf = reinterpret_cast<unsigned int*>(host + lead);
        for (size_t s = 0; s < lead; ++s) host[s] = span_time[s];
        for (size_t s = 0; s <= S; ++s) hf[s] = (unsigned int)span_first[s];
        KT_HIP(hipMemcpyAsync(dev, host, lead * sizeof(unsigned long long) + (S + 1) * sizeof(unsigned int), hipMemcpyHostToDevice, st));
        return KT_OK;
    }
    const unsigned long long* time() const { return dev; }
    const unsigned int* first() const { return reinterpret_cast<const unsigned int*>(dev + lead); }
    unsigned int* first_out() const { return reinterpret_cast<unsigned int*>(dev + lead) + (S + 1); }
    int download(hipStream_t st) const
    {
        KT_HIP(hipMemcpyAsync(reinterpret_cast<unsigned int*>(host + lead) + (S + 1), first_out(), (S + 1) * sizeof(unsigned int), hipMemcpyDeviceToHost, st));
        return KT_OK;
    }
    void get(size_t* span_first_out) const
    {
        const unsigned int* hfo = reinterpret_cast<const unsigned int*>(host + lead) + (S + 1);
        for (size_t s = 0; s <= S; ++s) span_first_out[s] = (size_t)hfo[s];
    }
};

// ---- the host form's staging of a pass that gives a mesh for a mesh: sized by {vertices in, triangles in, vertices out, triangles out};
// l: a word per input vertex, taken with `per_vertex_word` ----
struct kt_mesh_staging_ptrs { uint4 *v, *vo; unsigned int *t, *to, *l; };
struct kt_mesh_staging : kt_group<kt_mesh_staging_ptrs, 4> {
    int reserve(hipStream_t st, size_t n, size_t m, size_t o, size_t p, bool per_vertex_word)
    {
        return grow(st, {n, m, o, p}, [per_vertex_word](kt_mem& mem, kt_mesh_staging_ptrs& g, const size_t* c) {
            int s = mem.device(&g.v, c[0]);
            if (s == KT_OK) s = mem.device(&g.t, 3 * c[1]);
            if (s == KT_OK) s = mem.device(&g.vo, c[2]);
            if (s == KT_OK) s = mem.device(&g.to, 3 * c[3]);
            if (s == KT_OK && per_vertex_word) s = mem.device(&g.l, c[0]);
            return s;
        });
    }
};

// ---- the host-array form of a call, after the pass's own checks, its answer for an empty mesh, its capacity clamps and the growth of its
// staging: the uploads are enqueued (an empty one is skipped), `device` runs the _device form on the staging, `downloads` then names up to
// KT_HOST_DOWNLOADS copies back -- they depend on the counts the _device form returned -- and the host waits once.  A failure drains the
// stream before it is returned: the _device form may have failed before its own wait (a refused allocation, a workspace too small),
// and the uploads read the caller's arrays. ----
#define KT_HOST_DOWNLOADS 4
struct kt_host_copy { void* dst; const void* src; size_t bytes; };

inline int kt_enqueue_copies(hipStream_t st, const kt_host_copy* c, size_t count, hipMemcpyKind kind)
{
    for (size_t k = 0; k < count; ++k)
        if (c[k].bytes) KT_HIP(hipMemcpyAsync(c[k].dst, c[k].src, c[k].bytes, kind, st));
    return KT_OK;
}

template <size_t N, class Device, class Downloads>
int kt_mesh_host_form(hipStream_t st, const kt_host_copy (&uploads)[N], Device device, Downloads downloads)
{
    kt_host_copy down[KT_HOST_DOWNLOADS] = {};
    int s = kt_enqueue_copies(st, uploads, N, hipMemcpyHostToDevice);
    if (s == KT_OK) s = device();
    if (s == KT_OK) { downloads(down); s = kt_enqueue_copies(st, down, KT_HOST_DOWNLOADS, hipMemcpyDeviceToHost); }
    if (s != KT_OK) { (void)hipStreamSynchronize(st); return s; }
    KT_HIP(hipStreamSynchronize(st));
    return KT_OK;
}

// ---- the argument checks.  Each pass composes them in its own check function and keeps the lines that are its own. ----
inline bool kt_overlap(const void* a, size_t a_bytes, const void* b, size_t b_bytes)
{
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a && b && a_bytes && b_bytes && a0 < b0 + b_bytes && b0 < a0 + a_bytes;
}

inline int kt_mesh_check_inputs(const void* vertices, size_t n, const void* triangles, size_t m)
{
    KT_ARG((vertices && ((uintptr_t)vertices & 15) == 0) || n == 0);
    KT_ARG(triangles || m == 0 || n == 0);
    return KT_OK;
}

inline int kt_mesh_check_outputs(const void* vertices_out, size_t vertex_capacity, const void* triangles_out, size_t triangle_capacity, size_t n, size_t m)
{
    KT_ARG((vertices_out && ((uintptr_t)vertices_out & 15) == 0) || vertex_capacity == 0 || n == 0);
    KT_ARG(triangles_out || triangle_capacity == 0 || m == 0 || n == 0);
    return KT_OK;
}

// no output is or overlaps an input, and no output another output
struct kt_byte_range { const void* p; size_t bytes; };
inline int kt_mesh_check_disjoint(const kt_byte_range* outs, int n_outs, const kt_byte_range* ins, int n_ins)
{
    for (int a = 0; a < n_outs; ++a) {
        for (int i = 0; i < n_ins; ++i) KT_ARG(!outs[a].p || outs[a].p != ins[i].p);
        for (int i = 0; i < n_ins; ++i) KT_ARG(!kt_overlap(outs[a].p, outs[a].bytes, ins[i].p, ins[i].bytes));
        for (int b = a + 1; b < n_outs; ++b) KT_ARG(!kt_overlap(outs[a].p, outs[a].bytes, outs[b].p, outs[b].bytes));
    }
    return KT_OK;
}

// a table of n_spans spans over n vertices: span_first[0] = 0 <= ... <= span_first[n_spans] = n
inline int kt_mesh_check_spans(const size_t* span_first, int n_spans, size_t n)
{
    KT_ARG(n_spans >= 0 && (n == 0 || n_spans > 0));
    KT_ARG(span_first || n_spans == 0);
    if (n_spans > 0) {
        KT_ARG(span_first[0] == 0 && span_first[n_spans] == n);
        for (int s = 0; s < n_spans; ++s) KT_ARG(span_first[s] <= span_first[s + 1]);
    }
    return KT_OK;
}

// the table of an empty mesh
inline void kt_mesh_empty_spans(size_t* span_first_out, int n_spans)
{
    for (int s = 0; s <= n_spans; ++s) span_first_out[s] = 0;
}
