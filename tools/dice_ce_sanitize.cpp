// TEST INFRASTRUCTURE: a stand-alone host program that runs segm_softmax_dice_fwd / segm_softmax_dice_bwd (csrc/dice_ce.hip) on the
// CPU emulation of HIP with every buffer allocated at its exact size, to be built with AddressSanitizer + UBSan: an index past a
// buffer, a misaligned packet or an overflow in the index arithmetic is reported.  No Python, no GPU.
//
//   CXX=/opt/rocm/lib/llvm/bin/clang++
//   F="-O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -std=c++17 -pthread -Itests/emu -Wno-unused-value -DSEGM_EMU=1"
//   $CXX $F '-DSEGM_PIN_F32(x)=' '-DSEGM_SCHED_FENCE()=' '-DSEGM_PIN_F2(x)=' '-DSEGM_WAVE_LDS_SYNC()=hipemu::sync_wave()' \
//        -x c++ segmamba_amd/csrc/dice_ce.hip tests/emu/hip_emu_runtime.cpp tools/dice_ce_sanitize.cpp -o build/dice_ce_sanitize
//   ASAN_OPTIONS=detect_leaks=0:detect_stack_use_after_return=0 build/dice_ce_sanitize
//
// Cases: V = 65 (5 x 13, the per-voxel route), V = 4097 (17 x 241, three workgroups per sample), V = 64 (2 x 4 x 8, the packet route),
// each in fp32 and bf16, with 4 classes (a packet instantiation where the rows are aligned) and with 9 (the per-voxel route with the
// class count read from the arguments), int64 labels (some ignored) without a mask and uint8 labels with one; the logits lie in a
// buffer with one class more than is used (a channel slice) where the case says so.  The sums are compared with a double evaluation
// at 1e-5 relative, the gradient at 1e-2 of its largest value (bf16 output): gross errors only, the tests hold the bounds.
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

static int run_case(int depth, int height, int width, int dtype, int C, bool masked, bool slice) {
    const int B = 2, CS = slice ? C + 1 : C, IGN = 40;
    const int64_t V = (int64_t)depth * height * width;
    const size_t esize = dtype == SEGM_F32 ? 4 : 2;
    std::vector<float> x((size_t)B * CS * V);
    for (auto& v : x) v = rnd();
    std::vector<unsigned char> logits(x.size() * esize), dlogits((size_t)B * C * V * esize);
    for (size_t i = 0; i < x.size(); ++i) {
        if (dtype == SEGM_F32) memcpy(&logits[i * 4], &x[i], 4);
        else { const uint16_t h = to_bf16(x[i]); memcpy(&logits[i * 2], &h, 2); x[i] = from_bf16(h); }
    }
    std::vector<int64_t> labels((size_t)B * V);
    for (auto& l : labels) { l = (int64_t)(rng() % (uint32_t)(C + 1)); if (l == C) l = IGN; }
    std::vector<uint8_t> labels8(labels.begin(), labels.end()), mask((size_t)B * V);
    for (auto& m : mask) m = (uint8_t)(rng() % 4 != 0);
    std::vector<double> sums((size_t)3 * B * C + 2 * B, -1.0);
    std::vector<float> gi((size_t)B * C), gp((size_t)B * C), gce((size_t)B);
    for (size_t i = 0; i < gi.size(); ++i) { gi[i] = rnd(); gp[i] = rnd(); }
    for (auto& g : gce) g = rnd();
    const size_t wsb = segm_softmax_dice_workspace_bytes(B, C, V);
    if (wsb == 0) { printf("workspace_bytes refused the shape\n"); return 1; }
    std::vector<double> ws(wsb / 8);

    segm_softmax_dice_args a;
    memset(&a, 0, sizeof(a));
    a.batch = B; a.classes = C; a.dtype = dtype;
    a.label_kind = masked ? SEGM_REGION_LABELS_U8 : SEGM_REGION_LABELS_I64;
    a.depth = depth; a.height = height; a.width = width;
    a.has_ignore = 1; a.ignore_label = IGN;
    a.stride_b = (int64_t)CS * V; a.stride_c = V; a.stride_z = (int64_t)height * width; a.stride_y = width; a.stride_x = 1;
    a.logits = logits.data();
    a.labels = masked ? (const void*)labels8.data() : (const void*)labels.data();
    a.mask = masked ? mask.data() : nullptr;
    a.sums = sums.data();
    a.g_i = gi.data(); a.g_p = gp.data(); a.g_ce = gce.data();
    a.dlogits = dlogits.data();
    a.workspace = ws.data(); a.workspace_bytes = wsb;
    int rc = segm_softmax_dice_fwd(&a);
    if (rc != 0) { printf("segm_softmax_dice_fwd: status %d\n", rc); return 1; }
    rc = segm_softmax_dice_bwd(&a);
    if (rc != 0) { printf("segm_softmax_dice_bwd: status %d\n", rc); return 1; }

    int bad = 0;
    double gmax = 0.0, gerr = 0.0;
    std::vector<double> p((size_t)C);
    for (int b = 0; b < B; ++b) {
        std::vector<double> I((size_t)C, 0.0), P((size_t)C, 0.0), G((size_t)C, 0.0);
        double CE = 0.0, N = 0.0;
        for (int64_t v = 0; v < V; ++v) {
            const int64_t l = labels[b * V + v];
            const bool m = l != IGN && (!masked || mask[b * V + v] != 0);
            double mx = -1e300, se = 0.0;
            for (int c = 0; c < C; ++c) mx = fmax(mx, (double)x[((size_t)b * CS + c) * V + v]);
            for (int c = 0; c < C; ++c) { p[c] = exp((double)x[((size_t)b * CS + c) * V + v] - mx); se += p[c]; }
            double S = 0.0;
            for (int c = 0; c < C; ++c) { p[c] /= se; S += p[c] * ((c == l ? gi[b * C + c] : 0.0) + gp[b * C + c]); }
            if (m) {
                for (int c = 0; c < C; ++c) { P[c] += p[c]; if (c == l) { I[c] += p[c]; G[c] += 1.0; } }
                CE += log(se) + mx - (double)x[((size_t)b * CS + l) * V + v];
                N += 1.0;
            }
            for (int c = 0; c < C; ++c) {
                const double ac = (c == l ? gi[b * C + c] : 0.0) + gp[b * C + c];
                const double g = m ? p[c] * (ac - S) + gce[b] * (p[c] - (c == l ? 1.0 : 0.0)) : 0.0;
                float got;
                const size_t o = ((size_t)b * C + c) * V + v;
                if (dtype == SEGM_F32) memcpy(&got, &dlogits[o * 4], 4);
                else { uint16_t h; memcpy(&h, &dlogits[o * 2], 2); got = from_bf16(h); }
                gmax = fmax(gmax, fabs(g)); gerr = fmax(gerr, fabs(g - got));
                if (!m && got != 0.f) ++bad;
            }
        }
        for (int c = 0; c < C; ++c) {
            const double want[3] = {I[c], P[c], G[c]};
            for (int q = 0; q < 3; ++q) {
                const double got = sums[(size_t)q * B * C + b * C + c];
                if (!(fabs(got - want[q]) <= 1e-5 * fabs(want[q]))) { printf("sum %d of (%d, %d): %.9g, want %.9g\n", q, b, c, got, want[q]); ++bad; }
            }
        }
        const double gotce = sums[(size_t)3 * B * C + b], gotn = sums[(size_t)3 * B * C + B + b];
        if (!(fabs(gotce - CE) <= 1e-5 * fabs(CE))) { printf("CE of %d: %.9g, want %.9g\n", b, gotce, CE); ++bad; }
        if (gotn != N) { printf("N of %d: %.9g, want %.9g\n", b, gotn, N); ++bad; }
    }
    if (!(gerr <= 1e-2 * gmax)) { printf("gradient error %.3g of %.3g\n", gerr, gmax); ++bad; }
    printf("%d x %d x %d  %s  C = %d  %s%s: %s\n", depth, height, width, dtype == SEGM_F32 ? "fp32" : "bf16", C,
           masked ? "uint8 labels, mask" : "int64 labels", slice ? "  channel slice" : "", bad ? "FAILED" : "ok");
    return bad ? 1 : 0;
}

int main() {
    int failed = 0;
    const int shapes[3][3] = {{1, 5, 13}, {1, 17, 241}, {2, 4, 8}};
    for (const auto& s : shapes)
        for (int dtype : {(int)SEGM_F32, (int)SEGM_BF16})
            for (int C : {4, 9})
                for (int masked = 0; masked < 2; ++masked)
                    failed += run_case(s[0], s[1], s[2], dtype, C, masked != 0, (s[2] + masked) % 2 == 1);
    printf(failed ? "%d case(s) failed\n" : "all cases ran clean\n", failed);
    return failed ? 1 : 0;
}
