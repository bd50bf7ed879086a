// kt_context.hip -- context, error reporting and device memory for libkt_hip.so.
// Replaces the reference's containers/device_memory.cpp (ref-counted cudaMalloc / cudaMallocPitch),
// containers/initialization.cpp and the cudaSafeCall error path (internal.h:76-86).
// Memory is dense (no pitch): the reference's volume kernels already assume pitch == cols*sizeof(T).
#include "kt_internal.hpp"

#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <atomic>

static thread_local char g_err[512] = "";

void kt_set_error(const char* fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

int kt_check(hipError_t e, const char* what, const char* file, int line)
{
    if (e == hipSuccess) return KT_OK;
    kt_set_error("%s\t%s:%d (%s)", hipGetErrorString(e), file, line, what);
    return e == hipErrorOutOfMemory ? KT_ERR_NOMEM : KT_ERR_HIP;
}

// what all kt_mem objects of the process hold -- buffers, events, streams (kt_debug_live_allocations) -- and the request that
// kt_debug_fail_allocation refuses: g_refuse_in more requests from now, that one (0: none)
static std::atomic<long long> g_live[3];
static std::atomic<int> g_refuse_in{0};
static int refused(const char* what, const char* file, int line)
{
    if (g_refuse_in.load() <= 0 || g_refuse_in.fetch_sub(1) != 1) return KT_OK;
    kt_set_error("out of memory (kt_debug_fail_allocation)\t%s:%d (%s)", file, line, what);
    return KT_ERR_NOMEM;
}

int kt_mem::take(void** p, size_t bytes, bool pin, unsigned int flags, const char* file, int line)
{
    *p = nullptr; if (!bytes) bytes = 1;
    KT_TRY(refused(pin ? "hipHostMalloc" : "hipMalloc", file, line));
    const int s = pin ? kt_check(hipHostMalloc(p, bytes, flags), "hipHostMalloc", file, line) : kt_check(hipMalloc(p, bytes), "hipMalloc", file, line);
    if (s == KT_OK) { (pin ? host : dev).push_back(*p); ++g_live[0]; }
    return s;
}

int kt_mem::event(hipEvent_t* e, unsigned int flags, const char* file, int line)
{
    *e = nullptr;
    KT_TRY(refused("hipEventCreateWithFlags", file, line));
    const int s = kt_check(hipEventCreateWithFlags(e, flags), "hipEventCreateWithFlags", file, line);
    if (s == KT_OK) { events.push_back(*e); ++g_live[1]; }
    return s;
}

int kt_mem::stream(hipStream_t* st, const char* file, int line)
{
    *st = nullptr;
    KT_TRY(refused("hipStreamCreateWithFlags", file, line));
    const int s = kt_check(hipStreamCreateWithFlags(st, hipStreamNonBlocking), "hipStreamCreateWithFlags", file, line);
    if (s == KT_OK) { streams.push_back(*st); ++g_live[2]; }
    return s;
}

void kt_mem::drop(void* p)
{
    for (std::vector<void*>* v : {&dev, &host}) {
        const auto it = std::find(v->begin(), v->end(), p);
        if (it == v->end()) continue;   // (a null p is in neither list)
        (void)(v == &dev ? hipFree(p) : hipHostFree(p));
        v->erase(it); --g_live[0];
    }
}

void kt_mem::release()
{
    for (void* p : dev) (void)hipFree(p);
    for (void* p : host) (void)hipHostFree(p);
    for (hipEvent_t e : events) (void)hipEventDestroy(e);
    for (hipStream_t s : streams) (void)hipStreamDestroy(s);
    g_live[0] -= (long long)(dev.size() + host.size()); g_live[1] -= (long long)events.size(); g_live[2] -= (long long)streams.size();
    dev.clear(); host.clear(); events.clear(); streams.clear();
}

extern "C" {

const char* kt_last_error(void) { return g_err; }
const char* kt_version(void) { return "kintinuous_amd 0.1 (gfx950)"; }

int kt_debug_live_allocations(long long out3[3])
{
    KT_ARG(out3);
    for (int k = 0; k < 3; ++k) out3[k] = g_live[k].load();
    return KT_OK;
}
int kt_debug_fail_allocation(int nth) { g_refuse_in.store(nth > 0 ? nth : 0); return KT_OK; }

int kt_device_count(int* count)
{
    KT_ARG(count);
    KT_HIP(hipGetDeviceCount(count));
    return KT_OK;
}

// the context's own buffers and their initial contents, on its stream
static int ctx_buffers(kt_ctx* c)
{
    // 320 KB of hand-off granules: the reduction sets, the residual words, and at [32768, 40960) the level kernel's two sets (kt_track.hip; kt_icp_launch
    // checks that they fit)
    c->red_max_blocks = 1280;
    KT_TRY(c->mem.device(&c->red_partials, (size_t)32 * c->red_max_blocks)); KT_TRY(c->mem.device(&c->red_out, 64));
    KT_TRY(c->mem.device(&c->counters, 16)); KT_TRY(c->mem.device(&c->pose_gran, 16));
    KT_TRY(c->mem.pinned(&c->red_out_host, 64)); KT_TRY(c->mem.pinned(&c->int_out_host, 16));
    KT_HIP(hipMemsetAsync(c->red_partials, 0xff, sizeof(double) * 32 * c->red_max_blocks, c->stream));   // the reduction granules' sentinel (kt_track.hip)
    KT_HIP(hipMemsetAsync(c->counters, 0, sizeof(unsigned int) * 16, c->stream));
    KT_HIP(hipMemsetAsync(c->pose_gran, 0, sizeof(unsigned long long) * 16, c->stream));
    KT_HIP(hipStreamSynchronize(c->stream));
    return KT_OK;
}

int kt_ctx_create(int device, kt_ctx** out)
{
    KT_ARG(out);
    KT_HIP(hipSetDevice(device));
    kt_ctx* c = new kt_ctx();   // value-initialised: every pointer starts null, so a half-built context can be destroyed
    c->device = device;
    int s = kt_check(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking), "hipStreamCreate", __FILE__, __LINE__);
    c->own_stream = s == KT_OK;
    if (s == KT_OK) s = ctx_buffers(c);
    if (s != KT_OK) { (void)kt_ctx_destroy(c); return s; }
    *out = c;
    return KT_OK;
}

int kt_ctx_destroy(kt_ctx* c)
{
    if (!c) return KT_OK;
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    (void)kt_integrate_scratch_destroy(c->integ); (void)kt_slice_ws_destroy(c->slice_ws); (void)kt_mesh_ws_destroy(c->mesh_ws);
    (void)kt_loop_ws_destroy(c->loop_ws); (void)kt_match_ws_destroy(c->match_ws);
    c->mem.release();
    if (c->own_stream) (void)hipStreamDestroy(c->stream);
    delete c;
    return KT_OK;
}

int kt_ctx_set_stream(kt_ctx* c, void* hip_stream)
{
    KT_ARG(c);
    KT_HIP(hipStreamSynchronize(c->stream));
    if (c->own_stream) { (void)hipStreamDestroy(c->stream); c->own_stream = false; }
    c->stream = (hipStream_t)hip_stream;
    return KT_OK;
}

void* kt_ctx_stream(kt_ctx* c) { return c ? (void*)c->stream : nullptr; }

int kt_sync(kt_ctx* c)
{
    KT_ARG(c);
    KT_HIP(hipStreamSynchronize(c->stream));
    return KT_OK;
}

int kt_malloc(kt_ctx* c, size_t bytes, void** dptr)
{
    KT_ARG(c && dptr);
    KT_HIP(hipSetDevice(c->device));
    KT_HIP(hipMalloc(dptr, bytes ? bytes : 1));
    return KT_OK;
}

int kt_free(kt_ctx* c, void* dptr)
{
    KT_ARG(c);
    if (dptr) KT_HIP(hipFree(dptr));
    return KT_OK;
}

int kt_memset(kt_ctx* c, void* dptr, int value, size_t bytes)
{
    KT_ARG(c && dptr);
    KT_HIP(hipMemsetAsync(dptr, value, bytes, c->stream));
    return KT_OK;
}

int kt_upload(kt_ctx* c, void* dst, const void* src_host, size_t bytes)
{
    KT_ARG(c && dst && src_host);
    KT_HIP(hipMemcpyAsync(dst, src_host, bytes, hipMemcpyHostToDevice, c->stream));
    KT_HIP(hipStreamSynchronize(c->stream));  // blocking, like DeviceMemory::upload
    return KT_OK;
}

int kt_download(kt_ctx* c, void* dst_host, const void* src, size_t bytes)
{
    KT_ARG(c && dst_host && src);
    KT_HIP(hipMemcpyAsync(dst_host, src, bytes, hipMemcpyDeviceToHost, c->stream));
    KT_HIP(hipStreamSynchronize(c->stream));
    return KT_OK;
}

int kt_upload2d(kt_ctx* c, void* dst, const void* src_host, size_t host_pitch, size_t row_bytes, int rows)
{
    KT_ARG(c && dst && src_host && host_pitch >= row_bytes && rows >= 0);
    KT_HIP(hipMemcpy2DAsync(dst, row_bytes, src_host, host_pitch, row_bytes, (size_t)rows, hipMemcpyHostToDevice, c->stream));
    KT_HIP(hipStreamSynchronize(c->stream));
    return KT_OK;
}

int kt_download2d(kt_ctx* c, void* dst_host, size_t host_pitch, const void* src, size_t row_bytes, int rows)
{
    KT_ARG(c && dst_host && src && host_pitch >= row_bytes && rows >= 0);
    KT_HIP(hipMemcpy2DAsync(dst_host, host_pitch, src, row_bytes, row_bytes, (size_t)rows, hipMemcpyDeviceToHost, c->stream));
    KT_HIP(hipStreamSynchronize(c->stream));
    return KT_OK;
}

}  // extern "C"
