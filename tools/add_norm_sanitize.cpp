// TEST INFRASTRUCTURE: a stand-alone host program that runs segm_add_norm_fwd / segm_add_norm_bwd (csrc/add_norm.hip) on the CPU
// emulation of HIP with every buffer allocated at its exact size, to be built with AddressSanitizer + UBSan: an index past a buffer,
// a misaligned packet or an overflow in the index arithmetic is reported.  No Python, no GPU.
//
//   CXX=/opt/rocm/lib/llvm/bin/clang++
//   F="-O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -std=c++17 -pthread -Itests/emu -Wno-unused-value -DSEGM_EMU=1"
//   $CXX $F '-DSEGM_PIN_F32(x)=' '-DSEGM_SCHED_FENCE()=' '-DSEGM_PIN_F2(x)=' '-DSEGM_WAVE_LDS_SYNC()=hipemu::sync_wave()' \
//        '-DSEGM_BLOCK_LDS_SYNC()=hipemu::sync_block()' -Wl,--unresolved-symbols=ignore-all -x c++ segmamba_amd/csrc/add_norm.hip \
//        segmamba_amd/csrc/conv1d.hip tests/emu/hip_emu_runtime.cpp tools/add_norm_sanitize.cpp -o build/add_norm_sanitize
//   ASAN_OPTIONS=detect_leaks=0:detect_stack_use_after_return=0 build/add_norm_sanitize
// (conv1d.hip holds launch_reduce_partials, which adds the backward's partial rows; its convolution entries refer to the scan units,
// which this program never calls and does not link: hence the linker flag.)
//
// Cases: N in {1, 7, 8, 100, 1032, 8192} x M in {1, 3, 65} x the five dtype pairs (x, residual stream) x LayerNorm / RMS, forward
// and backward, each in three layouts: dense rows; a row stride of N + 8 (the packet route where N is whole packets); a row stride of
// N + 3 from an offset of one element (the element route).  The last element of the last row is the last of its allocation in all
// three.  The results are compared with a double evaluation at 2e-2 (16 bits) / 1e-4 (fp32) of the largest value, dweight and dbias at
// 1e-2: gross errors only, the tests hold the bounds.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../include/segmamba_hip.h"

static uint32_t rng_state = 4321u;
static uint32_t rng() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }
static float rnd() { return ((float)(rng() & 0xffff) / 65536.0f - 0.5f) * 4.0f; }

static size_t esize(int dtype) { return dtype == SEGM_F32 ? 4 : 2; }

static void put(unsigned char* p, int dtype, float v) {
    if (dtype == SEGM_F32) memcpy(p, &v, 4);
    else if (dtype == SEGM_F16) { const _Float16 h = (_Float16)v; memcpy(p, &h, 2); }
    else { const __bf16 h = (__bf16)v; memcpy(p, &h, 2); }
}

static float get(const unsigned char* p, int dtype) {
    if (dtype == SEGM_F32) { float v; memcpy(&v, p, 4); return v; }
    if (dtype == SEGM_F16) { _Float16 h; memcpy(&h, p, 2); return (float)h; }
    __bf16 h;
    memcpy(&h, p, 2);
    return (float)h;
}

// (M, N) rows with a row stride, `offset` elements into an allocation that ends with the last element of the last row
struct Rows {
    std::vector<unsigned char> buf;
    int64_t M, N, stride, offset;
    int dtype;
    Rows(int64_t M_, int64_t N_, int64_t stride_, int64_t offset_, int dtype_, bool fill)
        : buf((size_t)(offset_ + (M_ - 1) * stride_ + N_) * esize(dtype_)), M(M_), N(N_), stride(stride_), offset(offset_), dtype(dtype_) {
        if (fill)
            for (int64_t r = 0; r < M; ++r)
                for (int64_t c = 0; c < N; ++c) put(at(r, c), dtype, rnd());
    }
    unsigned char* at(int64_t r, int64_t c) { return buf.data() + (size_t)(offset + r * stride + c) * esize(dtype); }
    void* base() { return at(0, 0); }
    double val(int64_t r, int64_t c) { return (double)get(at(r, c), dtype); }
};

static int run_case(int64_t M, int64_t N, int dtype, int res_dtype, bool rms, int layout) {
    const int64_t stride = layout == 0 ? N : layout == 1 ? N + 8 : N + 3, offset = layout == 2 ? 1 : 0;
    const float eps = 1e-5f;
    Rows x(M, N, stride, offset, dtype, true), res(M, N, stride, offset, res_dtype, true), y(M, N, stride, offset, dtype, false);
    Rows res_out(M, N, stride, offset, res_dtype, false), dy(M, N, stride, offset, dtype, true), dres(M, N, stride, offset, res_dtype, true);
    Rows dx(M, N, stride, offset, dtype, false), dres_in(M, N, stride, offset, res_dtype, false);
    std::vector<float> w((size_t)N), b((size_t)N), mean((size_t)M), rstd((size_t)M), dw((size_t)N), db((size_t)N);
    for (auto& v : w) v = 1.0f + 0.25f * rnd();
    for (auto& v : b) v = 0.25f * rnd();
    const size_t wsb = segm_add_norm_workspace_bytes(M, (int32_t)N);
    if (wsb == 0) { printf("workspace_bytes refused the shape\n"); return 1; }
    std::vector<unsigned char> ws(wsb);

    segm_add_norm_args a;
    memset(&a, 0, sizeof(a));
    a.rows = M; a.cols = (int32_t)N; a.dtype = dtype; a.res_dtype = res_dtype; a.rms = rms; a.eps = eps;
    a.x = x.base(); a.x_stride = stride;
    a.residual = res.base(); a.residual_stride = stride;
    a.y = y.base(); a.y_stride = stride;
    a.residual_out = res_out.base(); a.residual_out_stride = stride;
    a.weight = w.data(); a.bias = rms ? nullptr : b.data();
    a.mean = rms ? nullptr : mean.data(); a.rstd = rstd.data();
    a.dy = dy.base(); a.dy_stride = stride;
    a.dresidual = dres.base(); a.dresidual_stride = stride;
    a.dx = dx.base(); a.dx_stride = stride;
    a.dresidual_in = dres_in.base(); a.dresidual_in_stride = stride;
    a.dweight = dw.data(); a.dbias = rms ? nullptr : db.data();
    a.workspace = ws.data(); a.workspace_bytes = wsb;
    int rc = segm_add_norm_fwd(&a);
    if (rc != 0) { printf("segm_add_norm_fwd: status %d\n", rc); return 1; }
    rc = segm_add_norm_bwd(&a);
    if (rc != 0) { printf("segm_add_norm_bwd: status %d\n", rc); return 1; }

    int bad = 0;
    const double tol = dtype == SEGM_F32 ? 1e-4 : 2e-2;
    double ymax = 1.0, yerr = 0.0, gmax = 1.0, gerr = 0.0, rerr = 0.0;
    std::vector<double> dwr((size_t)N, 0.0), dbr((size_t)N, 0.0);
    for (int64_t r = 0; r < M; ++r) {
        std::vector<double> s((size_t)N);
        double m = 0.0, q = 0.0;
        for (int64_t c = 0; c < N; ++c) { s[c] = (double)((float)x.val(r, c) + (float)res.val(r, c)); m += s[c]; }
        m = rms ? 0.0 : m / (double)N;
        for (int64_t c = 0; c < N; ++c) q += (s[c] - m) * (s[c] - m);
        const double rs = 1.0 / sqrt(q / (double)N + (double)eps);
        double c1 = 0.0, c2 = 0.0;
        for (int64_t c = 0; c < N; ++c) {
            const double yv = (s[c] - m) * rs * w[c] + (rms ? 0.0 : (double)b[c]);
            ymax = fmax(ymax, fabs(yv)); yerr = fmax(yerr, fabs(yv - y.val(r, c)));
            rerr = fmax(rerr, fabs(res_out.val(r, c) - s[c]) / fmax(1.0, fabs(s[c])));
            const double xh = (res_out.val(r, c) - m) * rs, wdy = w[c] * dy.val(r, c);
            c1 += xh * wdy; c2 += wdy;
            dwr[c] += dy.val(r, c) * xh; dbr[c] += dy.val(r, c);
        }
        c1 /= (double)N; c2 = rms ? 0.0 : c2 / (double)N;
        for (int64_t c = 0; c < N; ++c) {
            const double xh = (res_out.val(r, c) - m) * rs, wdy = w[c] * dy.val(r, c);
            const double g = (wdy - (xh * c1 + c2)) * rs + dres.val(r, c);
            gmax = fmax(gmax, fabs(g));
            gerr = fmax(gerr, fmax(fabs(g - dx.val(r, c)), fabs(g - dres_in.val(r, c))));
        }
    }
    double wmax = 1.0, werr = 0.0;
    for (int64_t c = 0; c < N; ++c) {
        wmax = fmax(wmax, fmax(fabs(dwr[c]), fabs(dbr[c])));
        werr = fmax(werr, fabs(dwr[c] - dw[c]));
        if (!rms) werr = fmax(werr, fabs(dbr[c] - db[c]));
    }
    if (!(yerr <= tol * ymax)) { printf("y error %.3g of %.3g\n", yerr, ymax); ++bad; }
    if (!(rerr <= (res_dtype == SEGM_F32 ? 1e-6 : 1e-2))) { printf("residual_out error %.3g\n", rerr); ++bad; }
    if (!(gerr <= tol * gmax)) { printf("dx / dresidual_in error %.3g of %.3g\n", gerr, gmax); ++bad; }
    if (!(werr <= 1e-2 * wmax)) { printf("dweight / dbias error %.3g of %.3g\n", werr, wmax); ++bad; }
    if (bad)
        printf("%lld x %lld  dtype %d  stream %d  %s  layout %d: FAILED\n", (long long)M, (long long)N, dtype, res_dtype, rms ? "rms" : "layernorm",
               layout);
    return bad ? 1 : 0;
}

int main() {
    int failed = 0, ran = 0;
    const int pairs[5][2] = {{SEGM_F32, SEGM_F32}, {SEGM_F16, SEGM_F16}, {SEGM_F16, SEGM_F32}, {SEGM_BF16, SEGM_BF16}, {SEGM_BF16, SEGM_F32}};
    for (int64_t N : {1, 7, 8, 100, 1032, 8192})
        for (int64_t M : {1, 3, 65})
            for (const auto& p : pairs)
                for (int rms = 0; rms < 2; ++rms)
                    for (int layout = 0; layout < 3; ++layout) {
                        failed += run_case(M, N, p[0], p[1], rms != 0, layout);
                        ++ran;
                    }
    if (failed) printf("%d of %d case(s) failed\n", failed, ran);
    else printf("all %d cases ran clean\n", ran);
    return failed ? 1 : 0;
}
