// kt_loopdb.hip -- the source of loop-closure candidates: PlaceRecognition::process's dbowInterface->detectLoop()
// (backend/PlaceRecognition.cpp:51-88; a DLoopDetector over SURF words, DBowInterfaceSurf.cpp:34-45) as a database of the bootstrap's
// BRIEF-256 descriptor lists.  NOT a port of DBoW2 / DLoopDetector: a defined stage with the detector's role (include/kt_abi.h and
// DESIGN.md 4.9 state it; kintinuous_amd/loop_db_ref.py restates it bit for bit).  An inverted index exists to avoid comparing a query
// with every stored image; here the query IS compared with every stored image, in one launch.
//   score      a workgroup of 256 lanes owns 512 query descriptors (two per lane, in registers) and ONE entry, whose descriptors stream
//              through LDS in match_nearest's 512-descriptor tiles (every lane reads the same address: a broadcast).  Each lane keeps
//              (d1, d2) per query, applies the rule, the waves fold their counts in fixed order and ONE integer atomic per workgroup
//              adds to the entry's score (integers: the order of the atomics does not matter).
//   select     the scores come down as `size` ints; islands, the best entry and the consistency check run on the host.
// The keypoints of a frame are kt_match.hip's (kt_match_frame_enqueue), copied device to device into the arena.
#include "kt_internal.hpp"
#include "kt_wave.hpp"

#include <string.h>

#define KT_LOOPDB_LANES 256                          // lanes of a scoring workgroup
#define KT_LOOPDB_QPL 2                              // queries per lane
#define KT_LOOPDB_QTILE (KT_LOOPDB_LANES * KT_LOOPDB_QPL)
#define KT_LOOPDB_MAX_ENTRIES (1 << 20)

namespace {

// grid = (entries, query tiles).  q: nq descriptors (from the device word when given); arena: `stride` descriptors per entry, count[e] of
// them written; score[e - first] += the accepted queries of this tile (zeroed before the launch).
__global__ __launch_bounds__(KT_LOOPDB_LANES) void loopdb_score(const unsigned int* __restrict__ q, const unsigned int* __restrict__ nq_dev, int nq_arg,
                                                                const unsigned int* __restrict__ arena, const unsigned int* __restrict__ count, int stride,
                                                                int first, kt_accept_rule rule, int* __restrict__ score)
{
    __shared__ __attribute__((aligned(16))) unsigned long long tile[KT_MATCH_DESC_TILE * 4];
    __shared__ int wave_count[KT_LOOPDB_LANES / 64];
    const int nq = nq_dev ? (int)min(*nq_dev, (unsigned int)stride) : nq_arg;
    const int q0 = blockIdx.y * KT_LOOPDB_QTILE;
    if (q0 >= nq) return;   // block-uniform
    const int e = first + blockIdx.x, t = threadIdx.x;
    const int ndb = (int)min(count[e], (unsigned int)stride);
    unsigned long long a[KT_LOOPDB_QPL][4];
    int d1[KT_LOOPDB_QPL], d2[KT_LOOPDB_QPL];
#pragma unroll
    for (int s = 0; s < KT_LOOPDB_QPL; ++s) {
        const int i = q0 + s * KT_LOOPDB_LANES + t;
        a[s][0] = a[s][1] = a[s][2] = a[s][3] = 0;
        if (i < nq) {
            const uint4 lo = *(const uint4*)(q + 8 * (size_t)i), hi = *(const uint4*)(q + 8 * (size_t)i + 4);
            a[s][0] = lo.x | ((unsigned long long)lo.y << 32); a[s][1] = lo.z | ((unsigned long long)lo.w << 32);
            a[s][2] = hi.x | ((unsigned long long)hi.y << 32); a[s][3] = hi.z | ((unsigned long long)hi.w << 32);
        }
        d1[s] = d2[s] = KT_MATCH_NO_SECOND;
    }
    const unsigned long long* db64 = (const unsigned long long*)(arena + 8 * (size_t)e * (size_t)stride);
    for (int j0 = 0; j0 < ndb; j0 += KT_MATCH_DESC_TILE) {
        const int nt = min(KT_MATCH_DESC_TILE, ndb - j0);
        __syncthreads();   // the previous tile has been read by every lane
        for (int k = t; k < nt * 4; k += KT_LOOPDB_LANES) tile[k] = db64[4 * (size_t)j0 + k];
        __syncthreads();
        for (int j = 0; j < nt; ++j) {
            const ulonglong2 b0 = *(const ulonglong2*)&tile[4 * j], b1 = *(const ulonglong2*)&tile[4 * j + 2];
#pragma unroll
            for (int s = 0; s < KT_LOOPDB_QPL; ++s) {
                const int d = (__popcll(a[s][0] ^ b0.x) + __popcll(a[s][1] ^ b0.y)) + (__popcll(a[s][2] ^ b1.x) + __popcll(a[s][3] ^ b1.y));
                d2[s] = min(d2[s], max(d1[s], d));   // the two smallest, duplicates counted
                d1[s] = min(d1[s], d);
            }
        }
    }
    int mine = 0;
#pragma unroll
    for (int s = 0; s < KT_LOOPDB_QPL; ++s) mine += (q0 + s * KT_LOOPDB_LANES + t < nq && kt_match_accept(d1[s], d2[s], rule)) ? 1 : 0;
    const int w = kt_wave_sum(mine);
    if ((t & 63) == 0) wave_count[t >> 6] = w;
    __syncthreads();
    if (t == 0) {
        int sum = 0;
        for (int k = 0; k < KT_LOOPDB_LANES / 64; ++k) sum += wave_count[k];
        if (sum) atomicAdd(&score[blockIdx.x], sum);
    }
}

bool detect_params_ok(const kt_loop_db_detect_params* p)
{
    return p && p->dislocal >= 0 && p->alpha_num >= 0 && p->alpha_num <= 65536 && p->alpha_den > 0 && p->alpha_den <= 65536 && p->min_score >= 0 && p->max_gap >= 0 &&
           p->max_gap < (1 << 24) && (p->consistency == 0 || p->consistency == 1);
}

}  // namespace

struct kt_loop_db {
    kt_mem mem;
    kt_ctx* ctx;
    hipStream_t stream;
    hipEvent_t extracted;        // recorded on the context's stream behind a frame's keypoints; the database's stream waits for it
    kt_loop_match_params match;
    int max_entries, size;
    int prev_island[2];          // the preceding detect call's best island, first < 0: none
    unsigned int* arena;         // max_entries x max_keypoints x 8 words
    unsigned int* count;         // device, max_entries
    unsigned int* query;         // device, max_keypoints x 8: kt_loop_db_scores' query
    int* score;                  // device, max_entries
    unsigned int* stage_host;    // pinned, max_keypoints x 8: descriptors on their way up or down
    int* score_host;             // pinned, max_entries
    unsigned int* count_host;    // pinned mirror of count (host-side truth for entries below size)
};

extern "C" int kt_loop_db_detect_params_default(kt_loop_db_detect_params* p)
{
    KT_ARG(p);
    p->dislocal = 20; p->alpha_num = 3; p->alpha_den = 10; p->min_score = 40; p->max_gap = 3; p->consistency = 1;
    return KT_OK;
}

extern "C" int kt_loop_db_destroy(kt_loop_db* db)
{
    if (!db) return KT_OK;
    if (db->stream) (void)hipStreamSynchronize(db->stream);
    db->mem.release();
    if (db->extracted) (void)hipEventDestroy(db->extracted);
    delete db;
    return KT_OK;
}

extern "C" int kt_loop_db_create(kt_ctx* c, int max_entries, const kt_loop_match_params* mp, void* hip_stream, kt_loop_db** out)
{
    KT_ARG(c && out && max_entries >= 1 && max_entries <= KT_LOOPDB_MAX_ENTRIES && kt_match_params_valid(mp));
    KT_HIP(hipSetDevice(c->device));
    kt_loop_db* db = new kt_loop_db();   // value-initialised: every pointer starts null
    db->ctx = c; db->stream = hip_stream ? (hipStream_t)hip_stream : c->stream; db->match = *mp; db->max_entries = max_entries;
    db->prev_island[0] = db->prev_island[1] = -1;
    const size_t K = (size_t)mp->max_keypoints, E = (size_t)max_entries;
    int s = kt_check(hipEventCreateWithFlags(&db->extracted, hipEventDisableTiming), "hipEventCreateWithFlags", __FILE__, __LINE__);
    if (s == KT_OK) s = db->mem.device(&db->arena, E * K * 8);
    if (s == KT_OK) s = db->mem.device(&db->count, E);
    if (s == KT_OK) s = db->mem.device(&db->query, K * 8);
    if (s == KT_OK) s = db->mem.device(&db->score, E);
    if (s == KT_OK) s = db->mem.pinned(&db->stage_host, K * 8);
    if (s == KT_OK) s = db->mem.pinned(&db->score_host, E);
    if (s == KT_OK) s = db->mem.pinned(&db->count_host, E);
    if (s != KT_OK) { (void)kt_loop_db_destroy(db); return s; }
    *out = db;
    return KT_OK;
}

extern "C" int kt_loop_db_reset(kt_loop_db* db)
{
    KT_ARG(db);
    KT_HIP(hipStreamSynchronize(db->stream));
    db->size = 0; db->prev_island[0] = db->prev_island[1] = -1;
    return KT_OK;
}

extern "C" int kt_loop_db_size(kt_loop_db* db) { return db ? db->size : -1; }

static int loopdb_full(const kt_loop_db* db, const char* who)
{
    kt_set_error("%s: the database is full (%d entries)", who, db->max_entries);
    return KT_ERR_CAPACITY;
}

// scores of the query (q, nq) against entries first .. last into score_host[0 .. last - first], enqueued on the database's stream
static int loopdb_score_enqueue(kt_loop_db* db, const unsigned int* q, const unsigned int* nq_dev, int nq_arg, int nq_max, int first, int last)
{
    const int E = last - first + 1, tiles = kt_div_up(nq_max, KT_LOOPDB_QTILE);
    KT_HIP(hipMemsetAsync(db->score, 0, (size_t)E * sizeof(int), db->stream));
    if (tiles > 0) {
        const kt_accept_rule rule = {db->match.max_hamming, db->match.ratio_num, db->match.ratio_den};
        hipLaunchKernelGGL(loopdb_score, dim3(E, tiles), dim3(KT_LOOPDB_LANES), 0, db->stream, q, nq_dev, nq_arg, db->arena, db->count, db->match.max_keypoints, first,
                           rule, db->score);
        KT_LAUNCH_CHECK();
    }
    KT_HIP(hipMemcpyAsync(db->score_host, db->score, (size_t)E * sizeof(int), hipMemcpyDeviceToHost, db->stream));
    return KT_OK;
}

extern "C" int kt_loop_db_add_descriptors(kt_loop_db* db, const uint32_t* desc, size_t n, int* out_entry)
{
    KT_ARG(db && out_entry && (desc || n == 0) && n <= (size_t)db->match.max_keypoints);
    if (db->size >= db->max_entries) return loopdb_full(db, "kt_loop_db_add_descriptors");
    const int e = db->size;
    const size_t K = (size_t)db->match.max_keypoints;
    if (n) {
        memcpy(db->stage_host, desc, n * 8 * sizeof(uint32_t));
        KT_HIP(hipMemcpyAsync(db->arena + (size_t)e * K * 8, db->stage_host, n * 8 * sizeof(uint32_t), hipMemcpyHostToDevice, db->stream));
    }
    db->count_host[e] = (unsigned int)n;
    KT_HIP(hipMemcpyAsync(db->count + e, db->count_host + e, sizeof(unsigned int), hipMemcpyHostToDevice, db->stream));
    KT_HIP(hipStreamSynchronize(db->stream));
    db->size = e + 1;
    *out_entry = e;
    return KT_OK;
}

extern "C" int kt_loop_db_scores(kt_loop_db* db, const uint32_t* desc, size_t n, int first, int last, int32_t* out_scores)
{
    KT_ARG(db && out_scores && (desc || n == 0) && n <= (size_t)db->match.max_keypoints && first >= 0 && first <= last && last < db->size);
    if (n) {
        memcpy(db->stage_host, desc, n * 8 * sizeof(uint32_t));
        KT_HIP(hipMemcpyAsync(db->query, db->stage_host, n * 8 * sizeof(uint32_t), hipMemcpyHostToDevice, db->stream));
    }
    KT_TRY(loopdb_score_enqueue(db, db->query, nullptr, (int)n, (int)n, first, last));
    KT_HIP(hipStreamSynchronize(db->stream));
    memcpy(out_scores, db->score_host, (size_t)(last - first + 1) * sizeof(int32_t));
    return KT_OK;
}

extern "C" int kt_loop_db_entry(kt_loop_db* db, int e, uint32_t* out_desc, size_t capacity, size_t* n_out)
{
    KT_ARG(db && n_out && e >= 0 && e < db->size && (out_desc || capacity == 0));
    const size_t n = db->count_host[e], K = (size_t)db->match.max_keypoints;
    *n_out = n;
    if (n > capacity) { kt_set_error("kt_loop_db_entry: %zu descriptors, capacity %zu", n, capacity); return KT_ERR_CAPACITY; }
    if (n) {
        KT_HIP(hipMemcpyAsync(db->stage_host, db->arena + (size_t)e * K * 8, n * 8 * sizeof(uint32_t), hipMemcpyDeviceToHost, db->stream));
        KT_HIP(hipStreamSynchronize(db->stream));
        memcpy(out_desc, db->stage_host, n * 8 * sizeof(uint32_t));
    }
    return KT_OK;
}

extern "C" int kt_host_loop_db_select(const int32_t* scores, int size, const int32_t prev_island[2], const kt_loop_db_detect_params* p, kt_loop_db_result* r)
{
    KT_ARG(r && size >= 0 && (scores || size == 0) && detect_params_ok(p));
    r->entry = size; r->status = KT_LOOP_DB_EMPTY; r->candidate = -1; r->candidate_score = 0; r->reference_score = 0;
    r->island_first = r->island_last = -1; r->island_score = 0; r->n_keypoints = 0;
    if (size == 0) return KT_OK;
    const int newest = size - 1;
    const long long ref = scores[newest];
    r->reference_score = (int)ref;
    if (ref < p->min_score) { r->status = KT_LOOP_DB_LOW_REFERENCE; return KT_OK; }
    // one pass over the candidates in ascending id: the island being built and the best one so far (a later island must beat it strictly)
    long long best_sum = -1, sum = 0;
    int best_first = -1, best_last = -1, best_entry = -1, first = -1, last = -1, top = -1;
    const long long limit = (long long)newest - p->dislocal;
    for (long long e = 0; e <= limit + 1; ++e) {
        const bool cand = e <= limit && scores[e] >= p->min_score && (long long)p->alpha_den * scores[e] >= (long long)p->alpha_num * ref;
        if (first >= 0 && (e > limit || (cand && e - last > p->max_gap))) {   // the island ends
            if (sum > best_sum) { best_sum = sum; best_first = first; best_last = last; best_entry = top; }
            first = -1;
        }
        if (!cand) continue;
        if (first < 0) { first = (int)e; sum = 0; top = (int)e; }
        else if (scores[e] > scores[top]) top = (int)e;
        sum += scores[e]; last = (int)e;
    }
    if (best_first < 0) { r->status = KT_LOOP_DB_NO_CANDIDATE; return KT_OK; }
    r->island_first = best_first; r->island_last = best_last; r->island_score = (int)best_sum; r->candidate_score = scores[best_entry];
    bool stands = true;
    if (p->consistency) {
        const long long g = p->max_gap;
        stands = prev_island && prev_island[0] >= 0 && (long long)prev_island[0] - g <= (long long)best_last + g && (long long)best_first - g <= (long long)prev_island[1] + g;
    }
    r->status = stands ? KT_LOOP_DB_DETECTED : KT_LOOP_DB_NOT_CONSISTENT;
    if (stands) r->candidate = best_entry;
    return KT_OK;
}

extern "C" int kt_loop_db_detect(kt_loop_db* db, const uint8_t* rgb, const uint16_t* depth, int cols, int rows, const kt_loop_db_detect_params* p, kt_loop_db_result* r)
{
    KT_ARG(db && r && detect_params_ok(p));
    if (db->size >= db->max_entries) return loopdb_full(db, "kt_loop_db_detect");
    kt_ctx* c = db->ctx;
    const unsigned int *desc = nullptr, *n_dev = nullptr;
    KT_TRY(kt_match_frame_enqueue(c, rgb, depth, cols, rows, &db->match, &desc, &n_dev));
    if (db->stream != c->stream) {
        KT_HIP(hipEventRecord(db->extracted, c->stream));
        KT_HIP(hipStreamWaitEvent(db->stream, db->extracted, 0));
    }
    // the query goes straight into the slot it will own: scored from there, counted only once `size` moves
    const int e = db->size;
    const size_t K = (size_t)db->match.max_keypoints;
    unsigned int* slot = db->arena + (size_t)e * K * 8;
    KT_HIP(hipMemcpyAsync(slot, desc, K * 8 * sizeof(unsigned int), hipMemcpyDeviceToDevice, db->stream));
    KT_HIP(hipMemcpyAsync(db->count + e, n_dev, sizeof(unsigned int), hipMemcpyDeviceToDevice, db->stream));
    KT_HIP(hipMemcpyAsync(db->count_host + e, n_dev, sizeof(unsigned int), hipMemcpyDeviceToHost, db->stream));
    if (e > 0) KT_TRY(loopdb_score_enqueue(db, slot, db->count + e, 0, (int)K, 0, e - 1));
    KT_HIP(hipStreamSynchronize(db->stream));
    KT_TRY(kt_host_loop_db_select(db->score_host, e, db->prev_island, p, r));
    if (db->count_host[e] > (unsigned int)K) db->count_host[e] = (unsigned int)K;   // (never: the cut keeps at most max_keypoints)
    r->n_keypoints = (int)db->count_host[e];
    db->prev_island[0] = r->island_first; db->prev_island[1] = r->island_last;
    db->size = e + 1;
    return KT_OK;
}
