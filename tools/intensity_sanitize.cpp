// TEST INFRASTRUCTURE: a stand-alone host program that runs segm_intensity_stats / segm_intensity_apply (csrc/intensity.hip) on the
// CPU emulation of HIP with every buffer allocated at its exact size, to be built with AddressSanitizer + UBSan: an index past a
// buffer, a misaligned packet or an overflow in the index arithmetic is reported.  No Python, no GPU.
//
//   CXX=/opt/rocm/lib/llvm/bin/clang++
//   F="-O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -std=c++17 -pthread -Itests/emu -Wno-unused-value -DSEGM_EMU=1"
//   $CXX $F '-DSEGM_PIN_F32(x)=' '-DSEGM_SCHED_FENCE()=' '-DSEGM_PIN_F2(x)=' '-DSEGM_WAVE_LDS_SYNC()=hipemu::sync_wave()' \
//        -x c++ segmamba_amd/csrc/intensity.hip tests/emu/hip_emu_runtime.cpp tools/intensity_sanitize.cpp -o build/intensity_sanitize
//   ASAN_OPTIONS=detect_leaks=0:detect_stack_use_after_return=0 build/intensity_sanitize
//
// Cases: V = 64 (2 x 4 x 8, the packet route), V = 65 (1 x 5 x 13, single voxels), V = 4097 (1 x 17 x 241, five workgroups per plane);
// 2 samples of 2 channels with the ops NOISE, CONTRAST (with a pre-scale), inverted GAMMA and none, dense and as a 2-of-3 channel
// slice of a buffer that ends with the last voxel used; in place without a mirror and out of place with the masks 7, 3, 5, 6.  The
// results are compared with a double evaluation at 1e-4 of the plane's largest value: gross errors only, the tests hold the bounds.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../include/segmamba_hip.h"

static uint32_t rng_state = 4321u;
static uint32_t rng() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }
static float rnd() { return ((float)(rng() & 0xffff) / 65536.0f - 0.5f) * 8.0f + 1.5f; }

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

static void want_plane(const float* v, int64_t V, int op, float a, float b, bool invert, const float* noise, std::vector<double>& y) {
    y.resize((size_t)V);
    if (op == SEGM_INTENSITY_OFF) { for (int64_t i = 0; i < V; ++i) y[i] = v[i]; return; }
    if (op == SEGM_INTENSITY_NOISE) { for (int64_t i = 0; i < V; ++i) y[i] = (double)v[i] + (double)a * noise[i]; return; }
    if (op == SEGM_INTENSITY_SCALE) { for (int64_t i = 0; i < V; ++i) y[i] = (double)v[i] * a; return; }
    std::vector<double> t((size_t)V);
    for (int64_t i = 0; i < V; ++i) t[i] = op == SEGM_INTENSITY_CONTRAST ? (double)(v[i] * a) : (invert ? -(double)v[i] : (double)v[i]);
    double mean = 0, lo = t[0], hi = t[0];
    for (double e : t) { mean += e; lo = fmin(lo, e); hi = fmax(hi, e); }
    mean /= (double)V;
    if (op == SEGM_INTENSITY_CONTRAST) {
        for (int64_t i = 0; i < V; ++i) y[i] = fmin(fmax((t[i] - mean) * b + mean, lo), hi);
        return;
    }
    double var = 0;
    for (double e : t) var += (e - mean) * (e - mean);
    const double sd0 = sqrt(var / (double)V), rng_ = hi - lo;
    double mean1 = 0;
    for (int64_t i = 0; i < V; ++i) { y[i] = pow(fmax((t[i] - lo) / (rng_ + 1e-7), 0.0), (double)a) * rng_ + lo; mean1 += y[i]; }
    mean1 /= (double)V;
    double var1 = 0;
    for (double e : y) var1 += (e - mean1) * (e - mean1);
    const double sd1 = sqrt(var1 / (double)V);
    for (int64_t i = 0; i < V; ++i) { y[i] = (y[i] - mean1) / (sd1 + 1e-8) * sd0 + mean; if (invert) y[i] = -y[i]; }
}

static int run_case(int D, int H, int W, bool slice, bool mirrored) {
    const int N = 2, C = 2, CS = slice ? 3 : 2, planes = N * C;
    const int64_t V = (int64_t)D * H * W;
    // a channel slice: the buffer ends with the last voxel of the last channel used
    const size_t count = slice ? (size_t)((N - 1) * CS + C) * V : (size_t)N * C * V;
    Exact<float> data(count), out((size_t)planes * V), noise((size_t)V);
    for (size_t i = 0; i < count; ++i) data.p[i] = rnd();
    for (int64_t i = 0; i < V; ++i) noise.p[i] = rnd() - 1.5f;
    std::vector<float> before(data.p, data.p + count);
    Exact<double> stats((size_t)planes * SEGM_INTENSITY_STATS_DOUBLES), stats2((size_t)planes * SEGM_INTENSITY_STATS_DOUBLES);
    const size_t wsb = segm_intensity_workspace_bytes(planes, V);
    if (wsb == 0) { printf("workspace_bytes refused the shape\n"); return 1; }
    Exact<double> ws(wsb / 8);
    const uint8_t ops[4] = {SEGM_INTENSITY_NOISE, SEGM_INTENSITY_CONTRAST, SEGM_INTENSITY_GAMMA, SEGM_INTENSITY_OFF};
    const uint8_t masks[4] = {7, 3, 5, 6};

    segm_intensity_args a;
    memset(&a, 0, sizeof(a));
    a.samples = N; a.channels = C; a.depth = D; a.height = H; a.width = W;
    a.stride_n = (int64_t)CS * V; a.stride_c = V; a.stride_z = (int64_t)H * W; a.stride_y = W; a.stride_x = 1;
    memcpy(a.op, ops, 4);
    a.invert[2] = 1;
    a.a[0] = 0.07f; a.a[1] = 1.2f; a.b[1] = 1.25f; a.a[2] = 0.7f;
    a.noise[0] = noise.p;
    a.data = data.p; a.stats = stats.p; a.stats2 = stats2.p;
    a.workspace = ws.p; a.workspace_bytes = wsb;
    int rc = segm_intensity_stats(&a);
    if (rc != 0) { printf("segm_intensity_stats, stage 0: status %d\n", rc); return 1; }
    a.stage = 1;
    rc = segm_intensity_stats(&a);
    if (rc != 0) { printf("segm_intensity_stats, stage 1: status %d\n", rc); return 1; }
    if (mirrored) {
        a.out = out.p;
        a.out_stride_n = (int64_t)C * V; a.out_stride_c = V; a.out_stride_z = (int64_t)H * W; a.out_stride_y = W;
        memcpy(a.mirror, masks, 4);
    }
    rc = segm_intensity_apply(&a);
    if (rc != 0) { printf("segm_intensity_apply: status %d\n", rc); return 1; }

    int bad = 0;
    std::vector<double> y;
    for (int v = 0; v < planes; ++v) {
        const int b = v / C, c = v % C;
        const float* src = before.data() + ((size_t)b * CS + c) * V;
        want_plane(src, V, ops[v], a.a[v], a.b[v], a.invert[v] != 0, noise.p, y);
        double big = 0, err = 0;
        for (double e : y) big = fmax(big, fabs(e));
        for (int z = 0; z < D; ++z)
            for (int yy = 0; yy < H; ++yy)
                for (int x = 0; x < W; ++x) {
                    const int64_t i = ((int64_t)z * H + yy) * W + x;
                    float got;
                    if (mirrored) {
                        const int m = masks[v], zo = (m & 1) ? D - 1 - z : z, yo = (m & 2) ? H - 1 - yy : yy, xo = (m & 4) ? W - 1 - x : x;
                        got = out.p[(size_t)v * V + ((int64_t)zo * H + yo) * W + xo];
                    } else {
                        got = data.p[((size_t)b * CS + c) * V + i];
                    }
                    err = fmax(err, fabs((double)got - y[i]));
                }
        if (!(err <= 1e-4 * big)) { printf("plane %d (op %d): error %.3g of %.3g\n", v, ops[v], err, big); ++bad; }
        if (mirrored && memcmp(data.p + ((size_t)b * CS + c) * V, src, (size_t)V * 4) != 0) { printf("plane %d: the input was written\n", v); ++bad; }
    }
    if (slice)                                        // the channel between the slices is nobody's
        if (memcmp(data.p + (size_t)C * V, before.data() + (size_t)C * V, (size_t)V * 4) != 0) { printf("the unused channel was written\n"); ++bad; }
    printf("%d x %d x %d  %s  %s: %s\n", D, H, W, slice ? "channel slice" : "dense", mirrored ? "out of place, mirrored" : "in place",
           bad ? "FAILED" : "ok");
    return bad ? 1 : 0;
}

int main() {
    int failed = 0;
    const int shapes[3][3] = {{2, 4, 8}, {1, 5, 13}, {1, 17, 241}};
    for (const auto& s : shapes)
        for (int slice = 0; slice < 2; ++slice)
            for (int mirrored = 0; mirrored < 2; ++mirrored) failed += run_case(s[0], s[1], s[2], slice != 0, mirrored != 0);
    printf(failed ? "%d case(s) failed\n" : "all cases ran clean\n", failed);
    return failed ? 1 : 0;
}
