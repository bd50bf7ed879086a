// kt_mesh_keys.hpp -- the sorted key list of the mesh post-passes that sort (kt_mesh_weld.hip, kt_mesh_simplify.hip: a key per vertex;
// kt_mesh_holes.hip, kt_mesh_smooth.hip: a key per half-edge).  n 64-bit keys and their positions 0 .. n - 1 go through
// rocprim's stable radix sort over all 64 bits: sk holds the keys in order, si where each came from, equal keys in input order.  The
// runs of equal keys are then found by the pass's own head rule (kt_wave.hpp: kt_runs_heads_kernel, kt_half_edge_class); scan_max gives
// every entry the sorted position of its run's head.  Only the units that sort include this header: it carries rocprim.  WITH_SCAN is a
// compile-time choice because naming rocprim's scan, even for its byte count alone, instantiates its kernels: the two passes that never
// scan stay without them.
#pragma once

#include "kt_mesh_pass.hpp"

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/iterator/counting_iterator.hpp>

struct kt_sorted_key_ptrs {
    unsigned long long* sk;           // device, one per entry: the sorted keys
    unsigned int* si;                 // device, one per entry: the sorted positions
    unsigned char* tmp; size_t tmp_bytes;   // rocprim's, at least one byte
};

template <bool WITH_SCAN>
struct kt_sorted_keys : kt_group<kt_sorted_key_ptrs> {   // sized by entries
    int reserve(hipStream_t st, size_t n)
    {
        return grow(st, {n}, [](kt_mem& mem, kt_sorted_key_ptrs& g, const size_t* c) {
            size_t a = 0, b = 0;
            KT_TRY(pairs(nullptr, a, nullptr, nullptr, nullptr, c[0], (hipStream_t)0));
            if constexpr (WITH_SCAN) KT_TRY(maxima(nullptr, b, nullptr, nullptr, c[0], (hipStream_t)0));
            g.tmp_bytes = std::max<size_t>(std::max(a, b), 1);
            int s = mem.device(&g.sk, c[0]);
            if (s == KT_OK) s = mem.device(&g.si, c[0]);
            if (s == KT_OK) s = mem.device(&g.tmp, g.tmp_bytes);
            return s;
        });
    }
    // keys: device, n of them, left as they are.  who: the pass, for the message
    int sort(hipStream_t st, const unsigned long long* keys, size_t n, const char* who)
    {
        size_t tb = 0;
        KT_TRY(pairs(nullptr, tb, keys, sk, si, n, st));
        if (tb > tmp_bytes) { kt_set_error("%s: sort workspace too small (%zu > %zu)", who, tb, tmp_bytes); return KT_ERR_STATE; }
        return pairs(tmp, tb, keys, sk, si, n, st);
    }
    // hps[j] = the largest of hp[0 .. j]: with hp[j] = j at the head of a run and 0 elsewhere, the sorted position of entry j's head
    // (hp is only read; it is not const so that one instantiation of rocprim's kernels serves the byte count and the scan)
    int scan_max(hipStream_t st, unsigned int* hp, unsigned int* hps, size_t n, const char* who)
    {
        static_assert(WITH_SCAN, "reserve() has not asked for the scan's bytes");
        size_t tb = 0;
        KT_TRY(maxima(nullptr, tb, hp, hps, n, st));
        if (tb > tmp_bytes) { kt_set_error("%s: scan workspace too small (%zu > %zu)", who, tb, tmp_bytes); return KT_ERR_STATE; }
        return maxima(tmp, tb, hp, hps, n, st);
    }
private:
    // the two rocprim calls; with work == nullptr they only answer the bytes they need
    static int pairs(void* work, size_t& bytes, const unsigned long long* keys, unsigned long long* sk, unsigned int* si, size_t n, hipStream_t st)
    {
        KT_HIP(rocprim::radix_sort_pairs(work, bytes, keys, sk, rocprim::counting_iterator<unsigned int>(0), si, n, 0, 64, st));
        return KT_OK;
    }
    static int maxima(void* work, size_t& bytes, unsigned int* hp, unsigned int* hps, size_t n, hipStream_t st)
    {
        KT_HIP(rocprim::inclusive_scan(work, bytes, hp, hps, n, rocprim::maximum<unsigned int>(), st));
        return KT_OK;
    }
};
