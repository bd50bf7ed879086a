// unionfind_host_check.cpp -- the union-find of kt_mesh_components.hip (kintinuous_amd/csrc/kt_unionfind.hpp) on the host: several
// threads hook the triangles of the chain and hub cases at once, then flatten, and every label must be the smallest index of its
// component.  A stand-alone program for the sanitizers (no GPU, no library):
//   g++ -std=c++17 -O1 -g -fsanitize=thread -pthread scripts/unionfind_host_check.cpp -o uf_tsan && ./uf_tsan
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -pthread scripts/unionfind_host_check.cpp -o uf_asan && ./uf_asan
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <numeric>
#include <random>
#include <thread>
#include <vector>

#include "../kintinuous_amd/csrc/kt_unionfind.hpp"

typedef unsigned int u32;

struct Mesh { u32 n; std::vector<u32> tri; };

static Mesh chain(u32 k, bool descending, std::mt19937& rng)
{
    Mesh m{k + 2, {}};
    std::vector<u32> idx(m.n);
    std::iota(idx.begin(), idx.end(), 0u);
    if (descending) std::reverse(idx.begin(), idx.end());
    else std::shuffle(idx.begin(), idx.end(), rng);
    for (u32 j = 0; j < k; ++j) { m.tri.push_back(idx[j]); m.tri.push_back(idx[j + 1]); m.tri.push_back(idx[j + 2]); }
    return m;
}

static Mesh hub(u32 k, bool last)
{
    Mesh m{2 * k + 1, {}};
    for (u32 j = 0; j < k; ++j) {
        if (last) { m.tri.push_back(2 * j); m.tri.push_back(m.n - 1); m.tri.push_back(2 * j + 1); }
        else { m.tri.push_back(2 * j + 1); m.tri.push_back(2 * j + 2); m.tri.push_back(0); }
    }
    return m;
}

// several components: strips of 1 .. 40 triangles under one permutation, a few vertices left alone
static Mesh islands(u32 k, std::mt19937& rng)
{
    Mesh m{0, {}};
    std::vector<u32> t;
    for (u32 done = 0; done < k;) {
        const u32 len = std::min<u32>(1 + rng() % 40, k - done);
        for (u32 j = 0; j < len; ++j) { t.push_back(m.n + j); t.push_back(m.n + j + 1); t.push_back(m.n + j + 2); }
        m.n += len + 2 + rng() % 2;
        done += len;
    }
    std::vector<u32> perm(m.n);
    std::iota(perm.begin(), perm.end(), 0u);
    std::shuffle(perm.begin(), perm.end(), rng);
    for (u32 x : t) m.tri.push_back(perm[x]);
    return m;
}

// the labels by a sequential union-find of its own: the smallest index of every component
static std::vector<u32> expected(const Mesh& m)
{
    std::vector<u32> p(m.n);
    std::iota(p.begin(), p.end(), 0u);
    auto find = [&](u32 x) { while (p[x] != x) x = p[x] = p[p[x]]; return x; };
    for (size_t t = 0; t < m.tri.size() / 3; ++t)
        for (int e = 1; e < 3; ++e) {
            const u32 a = find(m.tri[3 * t]), b = find(m.tri[3 * t + e]);
            if (a != b) p[std::max(a, b)] = std::min(a, b);
        }
    for (u32 v = 0; v < m.n; ++v) p[v] = find(v);
    return p;
}

static int run(const char* name, const Mesh& m, int threads, std::mt19937& rng)
{
    std::vector<u32> parent(m.n);
    std::iota(parent.begin(), parent.end(), 0u);
    const size_t nt = m.tri.size() / 3;
    std::vector<size_t> order(nt);
    std::iota(order.begin(), order.end(), (size_t)0);
    std::shuffle(order.begin(), order.end(), rng);   // the order of the triangles plays no part
    std::vector<std::thread> pool;
    for (int w = 0; w < threads; ++w)
        pool.emplace_back([&, w]() {
            for (size_t k = (size_t)w; k < nt; k += (size_t)threads) {   // interleaved: neighbouring triangles go to different threads
                const u32* t = &m.tri[3 * order[k]];
                kt_uf_unite(parent.data(), t[0], t[1]);
                kt_uf_unite(parent.data(), t[0], t[2]);
            }
        });
    for (auto& th : pool) th.join();
    pool.clear();
    for (u32 v = 0; v < m.n; ++v)
        if (parent[v] > v) { std::printf("%s: parent[%u] = %u breaks the invariant\n", name, v, parent[v]); return 1; }
    for (int w = 0; w < threads; ++w)
        pool.emplace_back([&, w]() {
            for (u32 v = (u32)w; v < m.n; v += (u32)threads) {
                const u32 r = kt_uf_find(parent.data(), v);
                if (r != v) KT_UF_MIN(parent.data() + v, r);
            }
        });
    for (auto& th : pool) th.join();
    const std::vector<u32> want = expected(m);
    for (u32 v = 0; v < m.n; ++v)
        if (parent[v] != want[v]) { std::printf("%s: label[%u] = %u, expected %u\n", name, v, parent[v], want[v]); return 1; }
    std::printf("%s: %u vertices, %zu triangles, %d threads: ok\n", name, m.n, nt, threads);
    return 0;
}

int main()
{
    std::mt19937 rng(12345);
    int bad = 0;
    const u32 sizes[] = {1, 63, 64, 65, 257, 4099, 70001};
    for (int threads : {2, 8})
        for (u32 k : sizes) {
            bad += run("chain descending", chain(k, true, rng), threads, rng);
            bad += run("chain random", chain(k, false, rng), threads, rng);
            bad += run("hub last", hub(k, true), threads, rng);
            bad += run("hub first", hub(k, false), threads, rng);
            bad += run("islands", islands(k, rng), threads, rng);
        }
    std::printf(bad ? "FAILED\n" : "all ok\n");
    return bad ? 1 : 0;
}
