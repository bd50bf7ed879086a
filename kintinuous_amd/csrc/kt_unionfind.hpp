// kt_unionfind.hpp -- the lock-free union-find of kt_mesh_components.hip and kt_mesh_holes.hip: find with path halving, union by index (the LARGER root goes
// under the SMALLER).  It compiles for the device and, with the three atomics below taken from the compiler's builtins, for the host, where
// scripts/unionfind_host_check.cpp runs it from several threads under the thread and address sanitizers.
//
// The invariant: parent[x] <= x, with equality only at a root, and parent[x] never grows.  Every write keeps it: a root `big` takes a
// smaller root by compare-and-swap against its own index (it was a root until that instant); a non-root takes one of its ancestors, all
// smaller than its parent, by atomic minimum.  A vertex that has stopped being a root never becomes one again.  What follows:
//   - find walks strictly downwards (x -> parent[parent[x]] < x while x is no root's child), so it cannot cycle and ends after at most
//     n / 2 steps, whatever the other lanes write meanwhile;
//   - in unite every failed compare-and-swap returns the value another lane put there, which is below `big`; the next round starts from
//     find of that value and of find(small) <= small, so a + b falls by at least one per failed round: at most 2 n rounds for this lane
//     alone, with no assumption about how the other lanes are scheduled;
//   - a component's last root is its smallest index under every interleaving: a root only ever goes under a smaller index of its own
//     component, and the smallest index can go under nothing.
#pragma once

#if defined(__HIP_DEVICE_COMPILE__) || defined(__HIPCC__)
#define KT_UF_FN __device__ __forceinline__
// agent scope, relaxed: the loads bypass the compute unit's L1, which other compute units' writes do not reach within a kernel
#define KT_UF_LOAD(p) __hip_atomic_load((p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
#define KT_UF_CAS(p, expected, desired) atomicCAS((p), (expected), (desired))
#define KT_UF_MIN(p, v) ((void)atomicMin((p), (v)))
#else
#define KT_UF_FN static inline
#define KT_UF_LOAD(p) __atomic_load_n((p), __ATOMIC_RELAXED)
static inline unsigned int kt_uf_host_cas(unsigned int* p, unsigned int expected, unsigned int desired)
{
    (void)__atomic_compare_exchange_n(p, &expected, desired, false, __ATOMIC_RELAXED, __ATOMIC_RELAXED);
    return expected;   // the value found, as atomicCAS returns it
}
static inline void kt_uf_host_min(unsigned int* p, unsigned int v)
{
    unsigned int old = __atomic_load_n(p, __ATOMIC_RELAXED);
    while (v < old && !__atomic_compare_exchange_n(p, &old, v, false, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) {}   // (old falls on every failure: it ends at v >= old)
}
#define KT_UF_CAS(p, expected, desired) kt_uf_host_cas((p), (expected), (desired))
#define KT_UF_MIN(p, v) kt_uf_host_min((p), (v))
#endif

// the root of x's tree as this lane sees it; halves the path it walks
KT_UF_FN unsigned int kt_uf_find(unsigned int* parent, unsigned int x)
{
    for (;;) {   // x falls on every round (header comment)
        const unsigned int p = KT_UF_LOAD(parent + x);
        if (p == x) return x;
        const unsigned int g = KT_UF_LOAD(parent + p);
        if (g == p) return p;
        KT_UF_MIN(parent + x, g);
        x = g;
    }
}

// joins the trees of a and b
KT_UF_FN void kt_uf_unite(unsigned int* parent, unsigned int a, unsigned int b)
{
    a = kt_uf_find(parent, a);
    b = kt_uf_find(parent, b);
    while (a != b) {   // a + b falls on every failed round (header comment)
        const unsigned int big = a > b ? a : b, small = a > b ? b : a;
        const unsigned int old = KT_UF_CAS(parent + big, big, small);
        if (old == big) return;
        a = kt_uf_find(parent, old);
        b = kt_uf_find(parent, small);
    }
}

#if defined(__HIP_DEVICE_COMPILE__) || defined(__HIPCC__)
// one lane per vertex: parent[v] = find(v), by atomic minimum so that the walks of other lanes through v stay valid.  The root of a
// component is its smallest index, so parent IS the label afterwards
template <int LANES>
__global__ __launch_bounds__(LANES) void kt_uf_flatten_kernel(unsigned int* parent, unsigned int n)
{
    const size_t v = (size_t)blockIdx.x * LANES + threadIdx.x;
    if (v >= n) return;
    const unsigned int r = kt_uf_find(parent, (unsigned int)v);
    if (r != (unsigned int)v) KT_UF_MIN(parent + v, r);
}
#endif
