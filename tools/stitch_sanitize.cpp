// TEST INFRASTRUCTURE: a stand-alone host program that runs segm_window_gather / _count / _blend / _finish (csrc/stitch.hip) on the CPU
// emulation of HIP with every buffer allocated at its exact size, to be built with AddressSanitizer + UBSan: an index past a buffer, a
// misaligned packet or an overflow in the index arithmetic is reported.  No Python, no GPU.
//
//   CXX=/opt/rocm/lib/llvm/bin/clang++
//   F="-O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -std=c++17 -pthread -Itests/emu -Wno-unused-value -DSEGM_EMU=1"
//   $CXX $F '-DSEGM_PIN_F32(x)=' '-DSEGM_SCHED_FENCE()=' '-DSEGM_PIN_F2(x)=' '-DSEGM_WAVE_LDS_SYNC()=hipemu::sync_wave()' \
//        -x c++ segmamba_amd/csrc/stitch.hip tests/emu/hip_emu_runtime.cpp tools/stitch_sanitize.cpp -o build/stitch_sanitize
//   ASAN_OPTIONS=detect_leaks=0:detect_stack_use_after_return=0 build/stitch_sanitize
//
// Cases, each under all eight mirror masks, with fp32 and bf16 predictions in turn:
//   5 x 6 x 7 in 8^3 windows           padding on every axis (asymmetric along y and x), one window per sample
//   6 x 11 x 13 in 8^3 windows         padding along z; window starts 3 along y and 4, 5 along x: unaligned rows, single voxels
//   4 x 4 x 32 in 4 x 4 x 16 windows   aligned rows: packets, reversed under an x-flip; starts 0, 8, 16
// 2 samples of 2 channels, 3 output channels; the volume dense and as a 2-of-3 channel slice of a buffer that ends with the last voxel
// used.  One mirror pass is gather -> blend (all windows of both samples in one launch: they overlap) -> finish as pass 0 of 2, then
// the same again as pass 1.  Everything is compared with a plain restatement of the index rules: the gather exactly, the rest to
// 1e-6 relative (gross errors only, the tests hold the bits); acc must be all zero after a finish.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../include/segmamba_hip.h"

static uint32_t rng_state = 97531u;
static uint32_t rng() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }
static float rnd() { return (float)(rng() & 0xffff) / 65536.0f - 0.4f; }

// `count` elements at a 16-byte aligned address, not one byte more
template <typename T> struct Exact {
    T* p;
    size_t count;
    explicit Exact(size_t n) : p(nullptr), count(n) {
        void* q = nullptr;
        if (posix_memalign(&q, 16, n * sizeof(T)) != 0) abort();
        p = (T*)q;
        memset(p, 0, n * sizeof(T));
    }
    ~Exact() { free(p); }
    Exact(const Exact&) = delete;
};

static uint16_t to_bf16(float f) { uint32_t u; memcpy(&u, &f, 4); return (uint16_t)(u >> 16); }
static float from_bf16(uint16_t h) { uint32_t u = (uint32_t)h << 16; float f; memcpy(&f, &u, 4); return f; }

struct Case {
    int size[3], roi[3];
    std::vector<int> starts[3];
};

static bool close_to(float got, double want) { return fabs((double)got - want) <= 1e-6 * fmax(1.0, fabs(want)); }

static int run_case(const Case& K, bool slice) {
    const int B = 2, C = 2, CS = slice ? 3 : 2, CO = 3;
    int img[3], pad0[3];
    for (int d = 0; d < 3; ++d) { img[d] = K.size[d] > K.roi[d] ? K.size[d] : K.roi[d]; pad0[d] = (img[d] - K.size[d]) / 2; }
    const int64_t V = (int64_t)K.size[0] * K.size[1] * K.size[2], RV = (int64_t)K.roi[0] * K.roi[1] * K.roi[2];
    const int64_t IV = (int64_t)img[0] * img[1] * img[2];
    std::vector<int> win;                             // b, z, y, x
    for (int b = 0; b < B; ++b)
        for (int z : K.starts[0]) for (int y : K.starts[1]) for (int x : K.starts[2]) { win.push_back(b); win.push_back(z); win.push_back(y); win.push_back(x); }
    const int n = (int)win.size() / 4;
    if (n > SEGM_STITCH_MAX_WINDOWS) { printf("too many windows\n"); return 1; }

    const size_t vol_count = slice ? (size_t)((B - 1) * CS + C) * V : (size_t)B * C * V;
    Exact<float> vol(vol_count), weight((size_t)RV), count((size_t)IV), gathered((size_t)n * C * RV), acc((size_t)B * CO * IV);
    Exact<float> total((size_t)B * CO * V), pred32((size_t)n * CO * RV);
    Exact<uint16_t> pred16((size_t)n * CO * RV);
    for (size_t i = 0; i < vol_count; ++i) vol.p[i] = rnd();
    for (int64_t i = 0; i < RV; ++i) weight.p[i] = 0.05f + (float)(rng() & 0xff) / 256.0f;
    for (size_t i = 0; i < pred32.count; ++i) { pred32.p[i] = rnd() * 3.0f; pred16.p[i] = to_bf16(pred32.p[i]); }

    segm_stitch_args a;
    memset(&a, 0, sizeof(a));
    a.batch = B;
    for (int d = 0; d < 3; ++d) {
        a.size[d] = K.size[d]; a.roi[d] = K.roi[d];
        a.n_starts[d] = (int)K.starts[d].size();
        for (size_t i = 0; i < K.starts[d].size(); ++i) a.starts[d][i] = K.starts[d][i];
    }
    a.n_windows = n;
    memcpy(a.window, win.data(), win.size() * sizeof(int));
    a.stride_b = (int64_t)CS * V; a.stride_c = V; a.stride_z = (int64_t)K.size[1] * K.size[2]; a.stride_y = K.size[2]; a.stride_x = 1;
    a.volume = vol.p; a.windows_out = gathered.p; a.weight = weight.p; a.count = count.p; a.acc = acc.p; a.total = total.p;
    a.cval = -2.5f;

    int bad = 0;
    a.channels = 1;
    int rc = segm_window_count(&a);
    if (rc != 0) { printf("segm_window_count: status %d\n", rc); return 1; }
    std::vector<double> want_count((size_t)IV, 0.0);
    for (int z : K.starts[0]) for (int y : K.starts[1]) for (int x : K.starts[2])
        for (int i = 0; i < K.roi[0]; ++i) for (int j = 0; j < K.roi[1]; ++j) for (int k = 0; k < K.roi[2]; ++k)
            want_count[(((size_t)(z + i)) * img[1] + (y + j)) * img[2] + (x + k)] += weight.p[((size_t)i * K.roi[1] + j) * K.roi[2] + k];
    for (int64_t i = 0; i < IV; ++i)
        if (!close_to(count.p[i], want_count[i]) || !(count.p[i] > 0.f)) { if (!bad) printf("count[%lld] = %g, want %g\n", (long long)i, count.p[i], want_count[i]); ++bad; }

    std::vector<double> want_total((size_t)B * CO * V, 0.0);
    for (int mask = 0; mask < 8 && !bad; ++mask) {
        const bool f[3] = {(mask & 1) != 0, (mask & 2) != 0, (mask & 4) != 0};
        const bool half = (mask & 1) != 0;            // bf16 predictions under the odd masks
        for (int pass = 0; pass < 2; ++pass) {
            a.channels = C; a.mirror = mask;
            rc = segm_window_gather(&a);
            if (rc != 0) { printf("segm_window_gather: status %d\n", rc); return 1; }
            for (int j = 0; j < n; ++j)
                for (int c = 0; c < C; ++c)
                    for (int i0 = 0; i0 < K.roi[0]; ++i0) for (int i1 = 0; i1 < K.roi[1]; ++i1) for (int i2 = 0; i2 < K.roi[2]; ++i2) {
                        const int i[3] = {i0, i1, i2};
                        int src[3];
                        bool in = true;
                        for (int d = 0; d < 3; ++d) {
                            const int u = win[4 * j + 1 + d] + i[d] - pad0[d];
                            in = in && u >= 0 && u < K.size[d];
                            src[d] = f[d] ? K.size[d] - 1 - u : u;
                        }
                        const float want = in ? vol.p[((size_t)win[4 * j] * CS + c) * V + ((size_t)src[0] * K.size[1] + src[1]) * K.size[2] + src[2]] : a.cval;
                        const float got = gathered.p[(((size_t)j * C + c) * K.roi[0] + i0) * K.roi[1] * K.roi[2] + (size_t)i1 * K.roi[2] + i2];
                        if (memcmp(&got, &want, 4) != 0) { if (!bad) printf("mask %d: gather window %d channel %d (%d, %d, %d) = %g, want %g\n", mask, j, c, i0, i1, i2, got, want); ++bad; }
                    }
            a.channels = CO;
            a.dtype = half ? SEGM_BF16 : SEGM_F32;
            a.pred = half ? (const void*)pred16.p : (const void*)pred32.p;
            rc = segm_window_blend(&a);
            if (rc != 0) { printf("segm_window_blend: status %d\n", rc); return 1; }
            std::vector<double> want_acc((size_t)B * CO * IV, 0.0);
            for (int j = 0; j < n; ++j)
                for (int c = 0; c < CO; ++c)
                    for (int i0 = 0; i0 < K.roi[0]; ++i0) for (int i1 = 0; i1 < K.roi[1]; ++i1) for (int i2 = 0; i2 < K.roi[2]; ++i2) {
                        const size_t r = ((size_t)i0 * K.roi[1] + i1) * K.roi[2] + i2, pi = ((size_t)j * CO + c) * RV + r;
                        const double p = half ? (double)from_bf16(pred16.p[pi]) : (double)pred32.p[pi];
                        want_acc[((size_t)win[4 * j] * CO + c) * IV + ((size_t)(win[4 * j + 1] + i0) * img[1] + (win[4 * j + 2] + i1)) * img[2] + (win[4 * j + 3] + i2)] +=
                            p * weight.p[r];
                    }
            for (size_t i = 0; i < acc.count; ++i)
                if (!close_to(acc.p[i], want_acc[i])) { if (!bad) printf("mask %d: acc[%zu] = %g, want %g\n", mask, i, acc.p[i], want_acc[i]); ++bad; }
            a.pass = pass; a.passes = 2;
            rc = segm_window_finish(&a);
            if (rc != 0) { printf("segm_window_finish: status %d\n", rc); return 1; }
            for (size_t i = 0; i < acc.count; ++i)
                if (acc.p[i] != 0.f) { if (!bad) printf("mask %d: acc[%zu] = %g after the finish\n", mask, i, acc.p[i]); ++bad; }
            for (int bc = 0; bc < B * CO; ++bc)
                for (int z = 0; z < K.size[0]; ++z) for (int y = 0; y < K.size[1]; ++y) for (int x = 0; x < K.size[2]; ++x) {
                    const int v[3] = {z, y, x};
                    size_t p = 0;
                    for (int d = 0; d < 3; ++d) p = p * img[d] + (size_t)(pad0[d] + (f[d] ? K.size[d] - 1 - v[d] : v[d]));
                    const size_t ti = (size_t)bc * V + ((size_t)z * K.size[1] + y) * K.size[2] + x;
                    const double q = want_acc[(size_t)bc * IV + p] / want_count[p];
                    want_total[ti] = pass == 0 ? q : (want_total[ti] + q) / 2.0;
                    if (!close_to(total.p[ti], want_total[ti])) { if (!bad) printf("mask %d pass %d: total[%zu] = %g, want %g\n", mask, pass, ti, total.p[ti], want_total[ti]); ++bad; }
                }
        }
    }
    printf("%d x %d x %d in %d x %d x %d windows (%d per launch)  %s: %s\n", K.size[0], K.size[1], K.size[2], K.roi[0], K.roi[1], K.roi[2], n,
           slice ? "channel slice" : "dense", bad ? "FAILED" : "ok");
    return bad ? 1 : 0;
}

int main() {
    const Case cases[3] = {
        {{5, 6, 7}, {8, 8, 8}, {{0}, {0}, {0}}},
        {{6, 11, 13}, {8, 8, 8}, {{0}, {0, 3}, {0, 4, 5}}},
        {{4, 4, 32}, {4, 4, 16}, {{0}, {0}, {0, 8, 16}}},
    };
    int failed = 0;
    for (const Case& k : cases)
        for (int slice = 0; slice < 2; ++slice) failed += run_case(k, slice != 0);
    printf(failed ? "%d case(s) failed\n" : "all cases ran clean\n", failed);
    return failed ? 1 : 0;
}
