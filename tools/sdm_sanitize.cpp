// TEST INFRASTRUCTURE: a stand-alone host program that runs segm_sdm_masks and segm_sdm_compose (csrc/sdm.hip), with segm_edt_sq
// (csrc/metrics.hip) between them, on the CPU emulation of HIP with every buffer allocated at its exact size, to be built with
// AddressSanitizer + UBSan: an index past a buffer, a misaligned access or an overflow in the index arithmetic is reported.
// No Python, no GPU.
//
//   CXX=/opt/rocm/lib/llvm/bin/clang++
//   F="-O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -std=c++17 -pthread -Itests/emu -Wno-unused-value -DSEGM_EMU=1"
//   $CXX $F '-DSEGM_PIN_F32(x)=' '-DSEGM_SCHED_FENCE()=' '-DSEGM_PIN_F2(x)=' '-DSEGM_WAVE_LDS_SYNC()=hipemu::sync_wave()' \
//        '-DSEGM_BLOCK_LDS_SYNC()=hipemu::sync_block()' \
//        -x c++ segmamba_amd/csrc/sdm.hip segmamba_amd/csrc/metrics.hip tests/emu/hip_emu_runtime.cpp tools/sdm_sanitize.cpp -o build/sdm_sanitize
//   ASAN_OPTIONS=detect_leaks=0:detect_stack_use_after_return=0 build/sdm_sanitize
//
// Cases: random label volumes of 1 (1 x 1 x 1), 105 (3 x 5 x 7), 4160 (4 x 8 x 130: a multiple of 4, packets) and 5250 (5 x 7 x 150:
// beyond one workgroup's 4096 voxels of the mask pass, the second volume's planes off the 16-byte grid) voxels, as uint8, int16 and
// int64 labels with -1 and 300 among the wider ones; 1 item (one volume, one region) and 16 items (two volumes x eight regions, the
// transforms of two calls of 16 planes in one buffer); all three outputs, and the edge alone without a transform.  Every bit volume,
// count and output value is compared with plain loops over the volume (the same fp64 expression, so exactly).
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../include/segmamba_hip.h"

static uint32_t rng_state = 24680u;
static uint32_t rng() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }

// `count` elements at a 16-byte aligned address, not one byte more
template <typename T> struct Exact {
    T* p;
    size_t count;
    explicit Exact(size_t n) : p(nullptr), count(n) {
        void* q = nullptr;
        if (posix_memalign(&q, 16, n * sizeof(T) ? n * sizeof(T) : 1) != 0) abort();
        p = (T*)q;
        memset(p, 0x5a, n * sizeof(T));
    }
    ~Exact() { free(p); }
    Exact(const Exact&) = delete;
};

template <typename T>
static int run_case(const char* name, int D, int H, int W, int n, int R, int dtype) {
    const int64_t N = (int64_t)D * H * W;
    std::vector<int64_t> lab((size_t)n * N);
    for (auto& v : lab) {
        const uint32_t r = rng() % 16;
        v = r < 9 ? 0 : (int64_t)(r % 5);                                   // sparse labels 0 .. 4
        if (sizeof(T) > 1 && rng() % 37 == 0) v = (rng() & 1) ? -1 : 300;
    }
    uint8_t table[256] = {0};
    for (int l = 1; l < 5; ++l)
        for (int r = 0; r < R; ++r)
            if (R == 1 ? l == 1 || l == 3 : ((l + r) % 3 != 0 || r == l)) table[l] |= (uint8_t)(1u << r);
    table[44] = 0xff;                                                       // 300 must not alias 300 - 256
    Exact<T> labels((size_t)n * N);
    for (size_t i = 0; i < lab.size(); ++i) labels.p[i] = (T)lab[i];
    Exact<uint8_t> tab(256), inside((size_t)n * N * 2), edge((size_t)n * N), boundary((size_t)n * N);     // inside, then outside: one EDT batch
    Exact<int64_t> counts((size_t)n * 8);
    memcpy(tab.p, table, 256);
    segm_sdm_masks_args m;
    memset(&m, 0, sizeof(m));
    m.depth = D; m.height = H; m.width = W; m.n = n; m.n_regions = R; m.label_dtype = dtype;
    m.labels = labels.p; m.table = tab.p; m.inside = inside.p; m.outside = inside.p + (size_t)n * N; m.edge = edge.p; m.boundary = boundary.p;
    m.counts = counts.p;
    int rc = segm_sdm_masks(&m);
    if (rc != 0) { printf("%s: segm_sdm_masks: status %d\n", name, rc); return 1; }
    int bad = 0;
    auto bits = [&](int v, int z, int y, int x) -> uint32_t {
        const int64_t l = lab[(size_t)v * N + ((size_t)z * H + y) * W + x];
        return l >= 0 && l < 256 ? (uint32_t)(table[l] & ((1u << R) - 1u)) : 0u;
    };
    std::vector<int64_t> want_counts((size_t)n * 8, 0);
    for (int v = 0; v < n; ++v)
        for (int z = 0; z < D; ++z) for (int y = 0; y < H; ++y) for (int x = 0; x < W; ++x) {
            const uint32_t p = bits(v, z, y, x);
            uint32_t pe = p, pb = p;
            const int dz[6] = {-1, 1, 0, 0, 0, 0}, dy[6] = {0, 0, -1, 1, 0, 0}, dx[6] = {0, 0, 0, 0, -1, 1};
            for (int k = 0; k < 6; ++k) {
                const int zz = z + dz[k], yy = y + dy[k], xx = x + dx[k];
                if (zz < 0 || zz >= D || yy < 0 || yy >= H || xx < 0 || xx >= W) pe = 0;
                else { pe &= bits(v, zz, yy, xx); pb &= bits(v, zz, yy, xx); }
            }
            const size_t i = (size_t)v * N + ((size_t)z * H + y) * W + x;
            const uint8_t want[4] = {(uint8_t)p, (uint8_t)(~p & ((1u << R) - 1u)), (uint8_t)(p & ~pe), (uint8_t)(p & ~pb)};
            const uint8_t got[4] = {inside.p[i], inside.p[(size_t)n * N + i], edge.p[i], boundary.p[i]};
            if (memcmp(want, got, 4) != 0) { if (!bad) printf("%s: bits at volume %d voxel (%d, %d, %d)\n", name, v, z, y, x); ++bad; }
            for (int r = 0; r < 8; ++r) want_counts[(size_t)v * 8 + r] += (p >> r) & 1;
        }
    for (size_t i = 0; i < want_counts.size(); ++i)
        if (counts.p[i] != want_counts[i]) { if (!bad) printf("%s: counts[%zu] = %lld, want %lld\n", name, i, (long long)counts.p[i], (long long)want_counts[i]); ++bad; }
    // the transforms: plane 2 i = pos^2 (seeds: bit of `outside`), 2 i + 1 = neg^2 (seeds: bit of `inside`), 8 pairs per call
    const int items = n * R;
    Exact<int32_t> edt((size_t)2 * items * N);
    for (int i0 = 0; i0 < items; i0 += 8) {
        segm_edt_sq_args e;
        memset(&e, 0, sizeof(e));
        e.depth = D; e.height = H; e.width = W; e.n_volumes = 2 * n; e.fp32 = 0;
        e.spacing_z = e.spacing_y = e.spacing_x = 1.f;
        const int cnt = items - i0 < 8 ? items - i0 : 8;
        e.n_planes = 2 * cnt;
        for (int i = 0; i < cnt; ++i) {
            const int v = (i0 + i) / R, r = (i0 + i) % R;
            e.plane_volume[2 * i] = n + v; e.plane_bit[2 * i] = r;
            e.plane_volume[2 * i + 1] = v; e.plane_bit[2 * i + 1] = r;
        }
        e.volumes = inside.p; e.out = edt.p + (size_t)2 * i0 * N;
        rc = segm_edt_sq(&e);
        if (rc != 0) { printf("%s: segm_edt_sq: status %d\n", name, rc); return 1; }
    }
    Exact<float> sdf((size_t)items * N), sdm((size_t)items * N), eo((size_t)items * N), eo2((size_t)items * N);
    Exact<uint32_t> ws(SEGM_SDM_COMPOSE_WORKSPACE_BYTES / 4);
    segm_sdm_compose_args c;
    memset(&c, 0, sizeof(c));
    c.voxels = N; c.n_items = items; c.n_volumes = n; c.n_planes = 2 * items; c.n_out_planes = items;
    for (int i = 0; i < items; ++i) {
        c.volume[i] = i / R; c.bit[i] = i % R; c.pos_plane[i] = 2 * i; c.neg_plane[i] = 2 * i + 1; c.out_plane[i] = items - 1 - i;
    }
    c.edt = edt.p; c.inside = inside.p; c.edge = edge.p; c.boundary = boundary.p; c.counts = counts.p;
    c.sdf = sdf.p; c.sdm = sdm.p; c.edge_out = eo.p; c.workspace = ws.p; c.workspace_bytes = SEGM_SDM_COMPOSE_WORKSPACE_BYTES;
    rc = segm_sdm_compose(&c);
    if (rc != 0) { printf("%s: segm_sdm_compose: status %d\n", name, rc); return 1; }
    c.sdf = nullptr; c.sdm = nullptr; c.edt = nullptr; c.n_planes = 0; c.edge_out = eo2.p;              // the edge alone
    rc = segm_sdm_compose(&c);
    if (rc != 0) { printf("%s: segm_sdm_compose (edge): status %d\n", name, rc); return 1; }
    for (int i = 0; i < items; ++i) {
        const int v = i / R, r = i % R, o = items - 1 - i;
        const int64_t cnt = want_counts[(size_t)v * 8 + r];
        const bool live = cnt > 0 && cnt < N;
        int32_t pmax = 0, nmax = 0;
        for (int64_t k = 0; k < N; ++k) {
            const int32_t a = edt.p[(size_t)(2 * i) * N + k], b = edt.p[(size_t)(2 * i + 1) * N + k];
            if (live) { pmax = a > pmax ? a : pmax; nmax = b > nmax ? b : nmax; }
        }
        for (int64_t k = 0; k < N; ++k) {
            const size_t at = (size_t)v * N + k;
            const bool in = (inside.p[at] >> r) & 1, ed = (edge.p[at] >> r) & 1, bd = (boundary.p[at] >> r) & 1;
            double s = 0.0;
            if (live && !bd)
                s = in ? -(sqrt((double)edt.p[(size_t)(2 * i) * N + k]) / sqrt((double)pmax))
                       : sqrt((double)edt.p[(size_t)(2 * i + 1) * N + k]) / sqrt((double)nmax);
            const float want[3] = {(float)s, (float)(1.0 - s + (ed ? 1.0 : 0.0)), ed ? 1.0f : 0.0f};
            const float got[3] = {sdf.p[(size_t)o * N + k], sdm.p[(size_t)o * N + k], eo.p[(size_t)o * N + k]};
            if (memcmp(want, got, 12) != 0 || eo2.p[(size_t)o * N + k] != want[2]) {
                if (!bad) printf("%s: item %d voxel %lld: got %g %g %g, want %g %g %g\n", name, i, (long long)k, got[0], got[1], got[2], want[0], want[1], want[2]);
                ++bad;
            }
        }
    }
    printf("%-10s %5lld voxels %2d items: %s\n", name, (long long)N, items, bad ? "FAILED" : "ok");
    return bad ? 1 : 0;
}

int main() {
    int failed = 0;
    const int shapes[4][3] = {{1, 1, 1}, {3, 5, 7}, {4, 8, 130}, {5, 7, 150}};
    for (const auto& s : shapes)
        for (int many = 0; many < 2; ++many) {
            const int n = many ? 2 : 1, R = many ? 8 : 1;
            failed += run_case<uint8_t>("uint8", s[0], s[1], s[2], n, R, SEGM_SDM_LABEL_U8);
            failed += run_case<int16_t>("int16", s[0], s[1], s[2], n, R, SEGM_SDM_LABEL_I16);
            failed += run_case<int64_t>("int64", s[0], s[1], s[2], n, R, SEGM_SDM_LABEL_I64);
        }
    printf(failed ? "%d case(s) failed\n" : "all cases ran clean\n", failed);
    return failed ? 1 : 0;
}
