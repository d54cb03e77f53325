// TEST INFRASTRUCTURE: a stand-alone host program that runs segm_region_loss_fwd / segm_region_loss_bwd (csrc/region_loss.hip) on the
// CPU emulation of HIP with every buffer allocated at its exact size, to be built with AddressSanitizer + UBSan: an index past a
// buffer, a misaligned packet or an overflow in the index arithmetic is reported.  No Python, no GPU.
//
//   CXX=/opt/rocm/lib/llvm/bin/clang++
//   F="-O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -std=c++17 -pthread -Itests/emu -Wno-unused-value -DSEGM_EMU=1"
//   $CXX $F '-DSEGM_PIN_F32(x)=' '-DSEGM_SCHED_FENCE()=' '-DSEGM_PIN_F2(x)=' '-DSEGM_WAVE_LDS_SYNC()=hipemu::sync_wave()' \
//        -x c++ segmamba_amd/csrc/region_loss.hip tests/emu/hip_emu_runtime.cpp tools/region_loss_sanitize.cpp -o build/region_loss_sanitize
//   ASAN_OPTIONS=detect_leaks=0:detect_stack_use_after_return=0 build/region_loss_sanitize
//
// Cases: V = 65 (5 x 13, the per-voxel route), V = 4097 (17 x 241, three workgroups per sample), V = 64 (2 x 4 x 8, the packet route),
// each in fp32 and bf16, with an int64 label map (some labels ignored) and with uint8 planes plus an ignore plane; the logits lie
// in a buffer with one region more than is used (a channel slice) where the case says so.  The sums are compared with a double
// evaluation at 1e-5 relative, the gradient at 1e-2 of its largest value (bf16 output): gross errors only, the tests hold the bounds.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../include/segmamba_hip.h"

static uint32_t rng_state = 12345u;
static uint32_t rng() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }
static float rnd() { return ((float)(rng() & 0xffff) / 65536.0f - 0.5f) * 8.0f; }

static uint16_t to_bf16(float f) { uint32_t u; memcpy(&u, &f, 4); return (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16); }
static float from_bf16(uint16_t h) { uint32_t u = (uint32_t)h << 16; float f; memcpy(&f, &u, 4); return f; }

static int run_case(int depth, int height, int width, int dtype, bool planes, bool slice) {
    const int B = 2, R = 3, RS = slice ? R + 1 : R;
    const int64_t V = (int64_t)depth * height * width;
    const size_t esize = dtype == SEGM_F32 ? 4 : 2;
    const uint32_t masks[3] = {0xau, 0xeu, 0x8u};
    std::vector<float> x((size_t)B * RS * V);
    for (auto& v : x) v = rnd();
    std::vector<unsigned char> logits(x.size() * esize), dlogits((size_t)B * R * V * esize);
    for (size_t i = 0; i < x.size(); ++i) {
        if (dtype == SEGM_F32) memcpy(&logits[i * 4], &x[i], 4);
        else { const uint16_t h = to_bf16(x[i]); memcpy(&logits[i * 2], &h, 2); x[i] = from_bf16(h); }
    }
    std::vector<int64_t> labels((size_t)B * V);
    for (auto& l : labels) l = (int64_t)(rng() % 5);                      // 4 is ignored
    std::vector<uint8_t> tplanes((size_t)B * (R + 1) * V);
    for (int b = 0; b < B; ++b)
        for (int64_t v = 0; v < V; ++v) {
            const int64_t l = labels[b * V + v];
            for (int r = 0; r < R; ++r) tplanes[((size_t)b * (R + 1) + r) * V + v] = l < 4 ? (uint8_t)((masks[r] >> l) & 1u) : 0;
            tplanes[((size_t)b * (R + 1) + R) * V + v] = l == 4;
        }
    std::vector<double> sums((size_t)4 * B * R + B, -1.0);
    std::vector<float> gi((size_t)B * R), gp((size_t)B * R), ge((size_t)B * R);
    for (size_t i = 0; i < gi.size(); ++i) { gi[i] = rnd(); gp[i] = rnd(); ge[i] = rnd(); }
    const size_t wsb = segm_region_loss_workspace_bytes(B, R, V);
    if (wsb == 0) { printf("workspace_bytes refused the shape\n"); return 1; }
    std::vector<double> ws(wsb / 8);

    segm_region_loss_args a;
    memset(&a, 0, sizeof(a));
    a.batch = B; a.regions = R; a.dtype = dtype;
    a.target_kind = planes ? SEGM_REGION_PLANES_U8 : SEGM_REGION_LABELS_I64;
    a.depth = depth; a.height = height; a.width = width;
    a.ignore_plane = planes ? 1 : 0;
    a.has_ignore = planes ? 0 : 1; a.ignore_label = 4;
    a.stride_b = (int64_t)RS * V; a.stride_r = V; a.stride_z = (int64_t)height * width; a.stride_y = width; a.stride_x = 1;
    for (int r = 0; r < R; ++r) a.masks[r] = masks[r];
    a.logits = logits.data();
    a.target = planes ? (const void*)tplanes.data() : (const void*)labels.data();
    a.sums = sums.data();
    a.g_i = gi.data(); a.g_p = gp.data(); a.g_e = ge.data();
    a.dlogits = dlogits.data();
    a.workspace = ws.data(); a.workspace_bytes = wsb;
    int rc = segm_region_loss_fwd(&a);
    if (rc != 0) { printf("segm_region_loss_fwd: status %d\n", rc); return 1; }
    rc = segm_region_loss_bwd(&a);
    if (rc != 0) { printf("segm_region_loss_bwd: status %d\n", rc); return 1; }

    int bad = 0;
    double gmax = 0.0, gerr = 0.0;
    for (int b = 0; b < B; ++b) {
        double n = 0.0;
        for (int r = 0; r < R; ++r) {
            double I = 0, P = 0, G = 0, E = 0;
            for (int64_t v = 0; v < V; ++v) {
                const int64_t l = labels[b * V + v];
                const double m = l == 4 ? 0.0 : 1.0, t = l < 4 ? (double)((masks[r] >> l) & 1u) : 0.0;
                const double xv = x[((size_t)b * RS + r) * V + v], p = 1.0 / (1.0 + exp(-xv));
                I += m * p * t; P += m * p; G += m * t; E += m * (fmax(xv, 0.0) - xv * t + log1p(exp(-fabs(xv))));
                if (r == 0) n += m;
                const double g = m * (p * (1 - p) * (gi[b * R + r] * t + gp[b * R + r]) + ge[b * R + r] * (p - t));
                float got;
                const size_t o = ((size_t)b * R + r) * V + v;
                if (dtype == SEGM_F32) memcpy(&got, &dlogits[o * 4], 4);
                else { uint16_t h; memcpy(&h, &dlogits[o * 2], 2); got = from_bf16(h); }
                gmax = fmax(gmax, fabs(g)); gerr = fmax(gerr, fabs(g - got));
                if (m == 0.0 && got != 0.f) ++bad;
            }
            const double want[4] = {I, P, G, E};
            for (int q = 0; q < 4; ++q) {
                const double got = sums[(size_t)q * B * R + b * R + r];
                if (!(fabs(got - want[q]) <= 1e-5 * fabs(want[q]))) { printf("sum %d of (%d, %d): %.9g, want %.9g\n", q, b, r, got, want[q]); ++bad; }
            }
        }
        if (sums[(size_t)4 * B * R + b] != n) { printf("N of %d: %.9g, want %.9g\n", b, sums[(size_t)4 * B * R + b], n); ++bad; }
    }
    if (!(gerr <= 1e-2 * gmax)) { printf("gradient error %.3g of %.3g\n", gerr, gmax); ++bad; }
    printf("%d x %d x %d  %s  %s%s: %s\n", depth, height, width, dtype == SEGM_F32 ? "fp32" : "bf16", planes ? "planes" : "labels",
           slice ? "  channel slice" : "", bad ? "FAILED" : "ok");
    return bad ? 1 : 0;
}

int main() {
    int failed = 0;
    const int shapes[3][3] = {{1, 5, 13}, {1, 17, 241}, {2, 4, 8}};
    for (const auto& s : shapes)
        for (int dtype : {(int)SEGM_F32, (int)SEGM_BF16})
            for (int planes = 0; planes < 2; ++planes)
                failed += run_case(s[0], s[1], s[2], dtype, planes != 0, (s[2] + planes) % 2 == 1);
    printf(failed ? "%d case(s) failed\n" : "all cases ran clean\n", failed);
    return failed ? 1 : 0;
}
