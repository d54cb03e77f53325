// TEST INFRASTRUCTURE: a stand-alone host program that runs segm_zoom_slices and segm_zoom_labels_slices (csrc/resample.hip) on the
// CPU emulation of HIP with every buffer - data, table, output, counts, workspace - allocated at its exact size, to be built with
// AddressSanitizer + UBSan: an index past a buffer, a misaligned access or an overflow in the index arithmetic is reported.
// No Python, no GPU.
//
//   CXX=/opt/rocm/lib/llvm/bin/clang++
//   F="-O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -std=c++17 -pthread -Itests/emu -Wno-unused-value -DSEGM_EMU=1"
//   $CXX $F '-DSEGM_PIN_F32(x)=' '-DSEGM_SCHED_FENCE()=' '-DSEGM_PIN_F2(x)=' '-DSEGM_WAVE_LDS_SYNC()=hipemu::sync_wave()' \
//        '-DSEGM_BLOCK_LDS_SYNC()=hipemu::sync_block()' \
//        -x c++ segmamba_amd/csrc/resample.hip tests/emu/hip_emu_runtime.cpp tools/resample_sepz_sanitize.cpp -o build/resample_sepz_sanitize
//   ASAN_OPTIONS=detect_leaks=0:detect_stack_use_after_return=0 build/resample_sepz_sanitize
//
// Cases: slices x height x width of 1 x 1 x 1, 3 x 5 x 7, 2 x 3 x 300 (a row past one x tile) and 6 x 4 x 9, with 1 and 8 channels, to
// in-plane shapes that grow, shrink and stay, under tables that shrink (every second slice), grow (every slice twice), repeat one
// slice and name slices outside the volume (clamped by the kernel); orders 3 and 1 with the clip, and the label rule with its counts.
// Checked besides the sanitizers: every output slice lies inside the range of its source slice, order 1 and the labels equal plain
// loops over the volume (values to 1e-12 of the slice's amplitude; labels wherever no weight is within 1e-9 of one half), the counts
// are those of the output, and output slices that share a source slice are bit-equal.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

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
        if (posix_memalign(&q, 16, n * sizeof(T) ? n * sizeof(T) : 1) != 0) abort();
        p = (T*)q;
        memset(p, 0x5a, n * sizeof(T));
    }
    ~Exact() { free(p); }
    Exact(const Exact&) = delete;
};

static int clampi(int v, int n) { return v < 0 ? 0 : (v > n - 1 ? n - 1 : v); }

// the two taps of order 1 at output i: scipy's coordinate clamped to the line
static void taps(int i, int n_in, int n_out, int& i0, int& i1, double& w0, double& w1) {
    double u = ((double)i + 0.5) * ((double)n_in / (double)n_out) - 0.5;
    u = u < 0.0 ? 0.0 : (u > (double)(n_in - 1) ? (double)(n_in - 1) : u);
    const double fl = floor(u);
    w1 = u - fl; w0 = 1.0 - w1;
    i0 = clampi((int)fl, n_in); i1 = clampi(i0 + 1, n_in);
}

static int run_case(int C, int S, int H, int W, int h, int w, const std::vector<int32_t>& table) {
    const int K = (int)table.size();
    char name[128];
    snprintf(name, sizeof(name), "%d x %d x %d x %d -> %d x %d x %d", C, S, H, W, K, h, w);
    const size_t plane = (size_t)H * W, oplane = (size_t)h * w;
    Exact<float> data((size_t)C * S * plane), out((size_t)C * K * oplane);
    Exact<int32_t> source((size_t)K);
    for (size_t i = 0; i < data.count; ++i) data.p[i] = ((float)(rng() % 20001) - 10000.f) * 0.01f * (float)(1 + (i / plane) % 3 * 9);
    memcpy(source.p, table.data(), K * sizeof(int32_t));
    int bad = 0;
    for (int order = 3; order >= 1; order -= 2) {
        const size_t nbytes = segm_zoom_slices_workspace_bytes(C, S, H, W, h, w, order);
        if (nbytes == 0) { printf("%s: no workspace size\n", name); return 1; }
        Exact<char> ws(nbytes);
        segm_zoom_slices_args a;
        memset(&a, 0, sizeof(a));
        a.channels = C; a.slices = S; a.height = H; a.width = W; a.out_slices = K; a.out_height = h; a.out_width = w;
        a.order = order; a.clip = 1;
        a.stride_c = (int64_t)S * plane; a.stride_s = (int64_t)plane; a.stride_y = W;
        a.data = data.p; a.source = source.p; a.out = out.p; a.workspace = ws.p; a.workspace_bytes = nbytes;
        memset(out.p, 0x5a, out.count * sizeof(float));
        const int rc = segm_zoom_slices(&a);
        if (rc != 0) { printf("%s: segm_zoom_slices order %d: status %d\n", name, order, rc); return 1; }
        for (int c = 0; c < C; ++c)
            for (int k = 0; k < K; ++k) {
                const int s = clampi(table[k], S);
                const float* src = data.p + ((size_t)c * S + s) * plane;
                float lo = src[0], hi = src[0];
                for (size_t i = 1; i < plane; ++i) { lo = src[i] < lo ? src[i] : lo; hi = src[i] > hi ? src[i] : hi; }
                const double amp = fabs((double)lo) > fabs((double)hi) ? fabs((double)lo) : fabs((double)hi);
                const float* got = out.p + ((size_t)c * K + k) * oplane;
                for (int y = 0; y < h; ++y) for (int x = 0; x < w; ++x) {
                    const float g = got[(size_t)y * w + x];
                    bool ok = g >= lo && g <= hi;
                    if (ok && (order == 1 || (h == H && w == W))) {
                        int y0, y1, x0, x1; double wy0, wy1, wx0, wx1;
                        taps(y, H, h, y0, y1, wy0, wy1); taps(x, W, w, x0, x1, wx0, wx1);
                        const double v = wy0 * (wx0 * src[(size_t)y0 * W + x0] + wx1 * src[(size_t)y0 * W + x1])
                                       + wy1 * (wx0 * src[(size_t)y1 * W + x0] + wx1 * src[(size_t)y1 * W + x1]);
                        ok = fabs((double)g - v) <= 1e-12 * amp + fabs(v) * 6e-8;
                    }
                    if (!ok) { if (!bad) printf("%s: order %d channel %d slice %d (%d, %d): %g outside [%g, %g] or off the plain loop\n", name, order, c, k, y, x, g, lo, hi); ++bad; }
                }
                for (int k2 = 0; k2 < k; ++k2)
                    if (clampi(table[k2], S) == s && memcmp(got, out.p + ((size_t)c * K + k2) * oplane, oplane * sizeof(float)) != 0) {
                        if (!bad) printf("%s: order %d: slices %d and %d share a source and differ\n", name, order, k2, k); ++bad;
                    }
            }
    }
    // labels: -1, 0 .. 3 and 300
    Exact<int16_t> seg((size_t)S * plane), lout((size_t)K * oplane);
    Exact<int64_t> counts(SEGM_PREP_COUNT_BINS);
    for (size_t i = 0; i < seg.count; ++i) { const uint32_t r = rng() % 23; seg.p[i] = (int16_t)(r == 0 ? -1 : (r == 1 ? 300 : (r / 4) % 4)); }
    segm_zoom_labels_slices_args b;
    memset(&b, 0, sizeof(b));
    b.slices = S; b.height = H; b.width = W; b.out_slices = K; b.out_height = h; b.out_width = w;
    b.seg = seg.p; b.source = source.p; b.out = lout.p; b.counts = counts.p;
    const int rc = segm_zoom_labels_slices(&b);
    if (rc != 0) { printf("%s: segm_zoom_labels_slices: status %d\n", name, rc); return 1; }
    std::vector<int64_t> want_counts(SEGM_PREP_COUNT_BINS, 0);
    for (int k = 0; k < K; ++k) {
        const int16_t* src = seg.p + (size_t)clampi(table[k], S) * plane;
        for (int y = 0; y < h; ++y) for (int x = 0; x < w; ++x) {
            int iy[2], ix[2]; double wy[2], wx[2];
            taps(y, H, h, iy[0], iy[1], wy[0], wy[1]); taps(x, W, w, ix[0], ix[1], wx[0], wx[1]);
            int best = INT32_MIN; bool tie = false;
            for (int m = 0; m < 4; ++m) {
                const int lab = src[(size_t)iy[m >> 1] * W + ix[m & 1]];
                double sum = 0.0;
                for (int q = 0; q < 4; ++q) if (src[(size_t)iy[q >> 1] * W + ix[q & 1]] == lab) sum += wy[q >> 1] * wx[q & 1];
                tie |= fabs(sum - 0.5) <= 1e-9;
                if (sum >= 0.5 && lab > best) best = lab;
            }
            const int want = best == INT32_MIN ? 0 : best, got = lout.p[((size_t)k * h + y) * w + x];
            if (!tie && got != want) { if (!bad) printf("%s: label at slice %d (%d, %d): %d, want %d\n", name, k, y, x, got, want); ++bad; }
            ++want_counts[got < 0 ? 256 : (got > 255 ? 257 : got)];
        }
    }
    for (int i = 0; i < SEGM_PREP_COUNT_BINS; ++i)
        if (counts.p[i] != want_counts[i]) { if (!bad) printf("%s: counts[%d] = %lld, want %lld\n", name, i, (long long)counts.p[i], (long long)want_counts[i]); ++bad; }
    b.counts = nullptr;                                                        // without the counts
    if (segm_zoom_labels_slices(&b) != 0) ++bad;
    printf("%-40s %s\n", name, bad ? "FAILED" : "ok");
    return bad ? 1 : 0;
}

int main() {
    int failed = 0;
    const int shapes[4][3] = {{1, 1, 1}, {3, 5, 7}, {2, 3, 300}, {6, 4, 9}};
    for (const auto& s : shapes) {
        const int S = s[0], H = s[1], W = s[2];
        std::vector<int32_t> shrink, grow, repeat(5, S - 1), wild = {-3, 0, S - 1, S, 1 << 30};
        for (int k = 0; k < S; k += 2) shrink.push_back(k);
        for (int k = 0; k < 2 * S; ++k) grow.push_back(k / 2);
        for (int C = 1; C <= 8; C += 7) {
            failed += run_case(C, S, H, W, 2 * H + 1, W + W / 2 + 1, grow);
            failed += run_case(C, S, H, W, (H + 1) / 2, (W + 2) / 3, shrink);
            failed += run_case(C, S, H, W, H, W, repeat);
            failed += run_case(C, S, H, W, H, 2 * W, wild);
        }
    }
    printf(failed ? "%d case(s) failed\n" : "all cases ran clean\n", failed);
    return failed ? 1 : 0;
}
