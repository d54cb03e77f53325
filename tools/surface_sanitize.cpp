// TEST INFRASTRUCTURE: a stand-alone host program that runs segm_border_stats (csrc/surface_stats.hip) on the CPU emulation of HIP with
// every buffer allocated at its exact size, to be built with AddressSanitizer + UBSan: an index past a buffer, a misaligned access or
// an overflow in the index arithmetic is reported.  No Python, no GPU.
//
//   CXX=/opt/rocm/lib/llvm/bin/clang++
//   F="-O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -std=c++17 -pthread -Itests/emu -Wno-unused-value -DSEGM_EMU=1"
//   $CXX $F '-DSEGM_PIN_F32(x)=' '-DSEGM_SCHED_FENCE()=' '-DSEGM_PIN_F2(x)=' '-DSEGM_WAVE_LDS_SYNC()=hipemu::sync_wave()' \
//        '-DSEGM_BLOCK_LDS_SYNC()=hipemu::sync_block()' \
//        -x c++ segmamba_amd/csrc/surface_stats.hip tests/emu/hip_emu_runtime.cpp tools/surface_sanitize.cpp -o build/surface_sanitize
//   ASAN_OPTIONS=detect_leaks=0:detect_stack_use_after_return=0 build/surface_sanitize
//
// Cases: two byte volumes of sparse random bits with random squared distances (int32 keys that use all four digits, and the same as
// fp32) at 105, 5250, 4160 and 1 voxels - no multiple of 16, beyond one workgroup's 4096 with the second volume at an odd address, a
// multiple of 16 - with 1 item and with 16 items in 5 groups (a group without an item, an item without a set bit, tolerances below 0,
// ranks out of range); and the (2, 3, 300) pair of tests/surface_checks.py with its exact squared distances by brute force (keys
// above 2^16).  Every row of `out` is compared with a plain gather, sum, maximum, count and std::sort.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../include/segmamba_hip.h"

static uint32_t rng_state = 13579u;
static uint32_t rng() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }

// `count` elements at a 16-byte aligned address, not one byte more
template <typename T> struct Exact {
    T* p;
    size_t count;
    explicit Exact(size_t n) : p(nullptr), count(n) {
        void* q = nullptr;
        if (posix_memalign(&q, 16, n * sizeof(T)) != 0) abort();
        p = (T*)q;
        memset(p, 0x5a, n * sizeof(T));
    }
    ~Exact() { free(p); }
    Exact(const Exact&) = delete;
};

struct Item { int vol, bit, plane, group; float tol; };

static float root_of(uint32_t key, int fp32) {
    float f;
    if (fp32) memcpy(&f, &key, 4); else f = (float)(int32_t)key;
    return sqrtf(f);
}

static bool same(double a, double b) { return (isnan(a) && isnan(b)) || a == b; }

// borders: (2, N) bytes; edt: (planes, N) raw 32-bit keys
static int run_case(const char* name, int64_t N, int planes, int fp32, const std::vector<uint8_t>& bord, const std::vector<uint32_t>& keys,
                    const std::vector<Item>& items, int n_groups, const std::vector<int64_t>& ranks) {
    Exact<uint8_t> b((size_t)2 * N);
    Exact<uint32_t> e((size_t)planes * N);
    Exact<double> out(96);
    memcpy(b.p, bord.data(), (size_t)2 * N);
    memcpy(e.p, keys.data(), (size_t)planes * N * 4);
    const size_t ws_bytes = segm_border_stats_workspace_bytes(N, (int32_t)items.size());
    Exact<uint8_t> ws(ws_bytes);
    segm_border_stats_args a;
    memset(&a, 0, sizeof(a));
    a.voxels = N; a.n_volumes = 2; a.n_planes = planes; a.n_items = (int32_t)items.size(); a.n_groups = n_groups; a.fp32 = fp32;
    for (size_t i = 0; i < items.size(); ++i) {
        a.border_volume[i] = items[i].vol; a.border_bit[i] = items[i].bit; a.edt_plane[i] = items[i].plane;
        a.item_group[i] = items[i].group; a.tolerance[i] = items[i].tol;
    }
    for (int g = 0; g < n_groups; ++g) { a.rank[g][0] = ranks[2 * g]; a.rank[g][1] = ranks[2 * g + 1]; }
    a.borders = b.p; a.edt = e.p; a.out = out.p; a.workspace = ws.p; a.workspace_bytes = ws_bytes;
    const int rc = segm_border_stats(&a);
    if (rc != 0) { printf("%s: segm_border_stats: status %d\n", name, rc); return 1; }
    int bad = 0;
    std::vector<std::vector<float>> joined((size_t)n_groups);
    for (size_t i = 0; i < 16; ++i) {
        double want[4] = {0.0, 0.0, 0.0, 0.0};
        if (i < items.size()) {
            const Item& it = items[i];
            for (int64_t v = 0; v < N; ++v) {
                if (!((bord[(size_t)it.vol * N + v] >> it.bit) & 1)) continue;
                const float d = root_of(keys[(size_t)it.plane * N + v], fp32);
                want[0] += 1.0; want[1] += (double)d;
                if ((double)d > want[2]) want[2] = (double)d;
                if (d <= it.tol) want[3] += 1.0;
                joined[(size_t)it.group].push_back(d);
            }
        }
        for (int q = 0; q < 4; ++q) {
            const double got = out.p[4 * i + q];
            const bool ok = q == 1 ? fabs(got - want[1]) <= 2.0 * want[0] * ldexp(1.0, -53) * want[1] : got == want[q];
            if (!ok) { if (!bad) printf("%s: out[%zu][%d] = %.17g, want %.17g\n", name, i, q, got, want[q]); ++bad; }
        }
    }
    for (int g = 0; g < 16; ++g) {
        std::vector<float> s;
        if (g < n_groups) { s = joined[(size_t)g]; std::sort(s.begin(), s.end()); }
        for (int r = 0; r < 2; ++r) {
            const int64_t k = g < n_groups ? ranks[2 * g + r] : -1;
            const double want = k >= 0 && k < (int64_t)s.size() ? (double)s[(size_t)k] : (double)NAN;
            const double got = out.p[64 + 2 * g + r];
            if (!same(got, want)) { if (!bad) printf("%s: group %d rank %lld = %.9g, want %.9g\n", name, g, (long long)k, got, want); ++bad; }
        }
    }
    printf("%-22s %8lld voxels %2zu items %s: %s\n", name, (long long)N, items.size(), fp32 ? "fp32 " : "int32", bad ? "FAILED" : "ok");
    return bad ? 1 : 0;
}

static int random_cases(int64_t N) {
    const int planes = 14;
    std::vector<uint8_t> bord((size_t)2 * N, 0);
    for (auto& v : bord)
        for (int bit = 0; bit < 8; ++bit)
            if (rng() % 32 == 0) v |= (uint8_t)(1u << bit);
    bord[0] |= 0x7f; bord[(size_t)N] |= 0x7f;
    for (int64_t v = 0; v < N; ++v) bord[(size_t)N + v] &= 0x7f;            // bit 7 of volume 1: never set
    int failed = 0;
    for (int fp32 = 0; fp32 < 2; ++fp32) {
        std::vector<uint32_t> keys((size_t)planes * N);
        for (auto& k : keys) {
            // squared distances of every magnitude: the low bits of a few equal prefixes, so that every digit pass decides somewhere
            const uint32_t hi = (rng() % 5) << (8 * (rng() % 4)), raw = (hi | (rng() & 0xff)) & 0x7fffffffu;
            if (fp32) { const float f = (float)raw * 0.37f; memcpy(&k, &f, 4); } else k = raw;
        }
        std::vector<Item> one = {{1, 3, 2, 0, 1.5f}};
        long long n1 = 0;
        for (int64_t v = 0; v < N; ++v) n1 += (bord[(size_t)N + v] >> 3) & 1;
        failed += run_case("1 item", N, planes, fp32, bord, keys, one, 1, {0, n1 - 1});
        std::vector<Item> many;
        const float tols[4] = {0.0f, 40.0f, 1000.0f, -1.0f};
        for (int i = 0; i < 15; ++i) many.push_back({i & 1, (i * 3) % 7, (i * 5) % 14, i % 3, tols[i & 3]});
        many.push_back({1, 7, 0, 4, 1.0f});
        long long n[3] = {0, 0, 0};
        for (int i = 0; i < 15; ++i)
            for (int64_t v = 0; v < N; ++v) n[i % 3] += (bord[(size_t)many[i].vol * N + v] >> many[i].bit) & 1;
        const long long lo = (long long)floor(0.95 * (double)(n[0] - 1));
        failed += run_case("16 items, 5 groups", N, planes, fp32, bord, keys, many, 5,
                           {lo, lo + 1 < n[0] ? lo + 1 : n[0] - 1, 0, n[1] - 1, n[2] / 2, n[2], 0, 0, 0, -1});
    }
    return failed;
}

static int thin_case() {
    const int D = 2, H = 3, W = 300;
    const int64_t N = (int64_t)D * H * W;
    std::vector<uint8_t> bord((size_t)2 * N, 0);
    auto at = [&](int z, int y, int x) { return ((size_t)z * H + y) * W + x; };
    for (int z = 0; z < D; ++z) for (int y = 0; y < H; ++y) bord[at(z, y, 0)] = 1;
    bord[(size_t)N + at(0, 0, 299)] = 1;
    for (int y = 1; y < 3; ++y) for (int x = 296; x < 299; ++x) bord[(size_t)N + at(1, y, x)] = 1;
    std::vector<uint32_t> keys((size_t)2 * N);
    for (int p = 0; p < 2; ++p)
        for (int z = 0; z < D; ++z) for (int y = 0; y < H; ++y) for (int x = 0; x < W; ++x) {
            uint32_t best = 0x7fffffffu;
            for (int zz = 0; zz < D; ++zz) for (int yy = 0; yy < H; ++yy) for (int xx = 0; xx < W; ++xx)
                if (bord[(size_t)p * N + at(zz, yy, xx)]) {
                    const uint32_t d2 = (uint32_t)((z - zz) * (z - zz) + (y - yy) * (y - yy) + (x - xx) * (x - xx));
                    if (d2 < best) best = d2;
                }
            keys[(size_t)p * N + at(z, y, x)] = best;
        }
    const std::vector<Item> items = {{0, 0, 1, 0, 298.5f}, {1, 0, 0, 0, 298.5f}};
    int failed = 0;
    failed += run_case("2 x 3 x 300", N, 2, 0, bord, keys, items, 1, {11, 12});
    failed += run_case("2 x 3 x 300, ends", N, 2, 0, bord, keys, items, 1, {0, 13});
    return failed;
}

int main() {
    int failed = 0;
    const int64_t sizes[4] = {105, 5250, 4160, 1};
    for (int64_t n : sizes) failed += random_cases(n);
    failed += thin_case();
    printf(failed ? "%d case(s) failed\n" : "all cases ran clean\n", failed);
    return failed ? 1 : 0;
}
