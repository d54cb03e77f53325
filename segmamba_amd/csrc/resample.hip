// Resampling a case to the target spacing on the device: cubic B-spline and linear zoom of the data, the label rule for the seg
// (C ABI: segm_zoom, segm_zoom_workspace_bytes, segm_zoom_labels; for the separate-z branch segm_zoom_slices,
// segm_zoom_slices_workspace_bytes, segm_zoom_labels_slices).
//
// Replaces what the reference's `resample_data_or_seg` does on the host without a separate z axis
// (light_training/preprocessing/resampling/default_resampling.py:126-217, called from default_preprocessor.py:187-201):
//   data  skimage `resize(x.astype(float64), new_shape, order, mode='edge', anti_aliasing=False)`, clip=True, per channel - for n-D
//         input that is scipy.ndimage.zoom(x, out / in, order, mode='nearest', grid_mode=True) clipped to [x.min(), x.max()];
//   seg   batchgenerators `resize_segmentation(seg, new_shape, 1)`: per label in ascending order the order-1 zoom r of its indicator,
//         out[r >= 0.5] = label on a volume of zeros.
//
// Order 3, per axis as scipy has it: the line padded by 12 edge copies on both sides, times the filter gain (1 - z)(1 - 1/z) = 6,
// the causal and the anti-causal recursion with the pole z = sqrt(3) - 2 under mirror boundary conditions on the padded line, then
// the four cubic B-spline weights at u = (i + 0.5) * (n_in / n_out) - 0.5 + 12.  The taps of every output lie in [-2, n + 1] of the
// unpadded line, so the workspace keeps n + 4 coefficients per axis, in fp64 (the reference's arithmetic is float64).
//   * zoom_minmax_kernel     per channel min and max of the input for the clip: wave shuffles, LDS, then two integer atomics per
//                            workgroup on order-preserving keys of the float bits (exact and order-free).
//   * zoom_fir_x_kernel      the x axis is contiguous: a tile of the row in LDS and the recursion's closed form, the symmetric FIR
//                            h_k = -6 z / (1 - z^2) * z^|k| on the mirrored padded line, cut at |k| = 32 (z^33 = 1e-19).  fp32 in,
//                            fp64 coefficients out at [z + 2][y + 2][0 .. W + 3].
//   * zoom_line_kernel       y, then z: one thread per line and lanes across x, so both sweeps are coalesced; in place.  The start
//                            value is scipy's sum cut at 40 terms (z^40 = 1e-23), the ten causal values past the kept range live in
//                            registers.  Loads go eight at a time ahead of the recursion that consumes them.
//   * zoom_eval_kernel       one thread per output voxel: 64 taps (order 3, from the coefficients) or 8 (order 1, from the input with
//                            the coordinate clamped to [0, n - 1] as scipy's 'nearest' does), the clip, the rounding to fp32.
//   * zoom_labels_kernel     the trilinear weights of the 8 corners summed per distinct corner label in fp64; the largest label
//                            whose sum is >= 0.5 wins, 0 if none; label counts as segm_crop_normalize has them.
// The separate-z branch (default_resampling.py:154-207, order_z = 0): every 2-D slice across the coarse axis goes through the same
// resize on its own and output slice k is the resized input slice source[k], the nearest one, from a table the host computes in
// float64 as scipy's map_coordinates(order=0) does.  order_z > 0 is not covered.
//   * zoom_slice_minmax_kernel   min and max of every slice of every channel, 2 * C * S keys at the head of the workspace.
//   * zoom_fir_x_kernel<0>, zoom_line_kernel (y)   the prefilter in the plane only: coefficients (C, S, H + 4, W + 4), no pass and
//                            no margin along the slice axis.
//   * zoom_slices_eval_kernel    one thread per output voxel: 16 taps (order 3) or 4 (order 1) in slice source[k] (clamped to the
//                            volume), the clip to THAT slice's range, the rounding to fp32; a copy where the plane keeps its shape.
//                            Outputs that share a source slice are each computed.
//   * zoom_labels_slices_kernel  the bilinear weights of the 4 corners summed per distinct corner label, and the counts.
// Every sum has a fixed order and there are no floating-point atomics: two calls are bit-equal.  Non-finite input is outside the contract.
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include "segm_device.h"
#include "spline_common.h"

namespace segm {

#ifdef SEGM_EMU
static inline void zoom_umin(uint32_t* p, uint32_t v) { __atomic_fetch_min(p, v, __ATOMIC_RELAXED); }
static inline void zoom_umax(uint32_t* p, uint32_t v) { __atomic_fetch_max(p, v, __ATOMIC_RELAXED); }
static inline void zoom_add_lds(int32_t* p, int32_t v) { __atomic_fetch_add(p, v, __ATOMIC_RELAXED); }
static inline void zoom_add64(long long* p, long long v) { __atomic_fetch_add(p, v, __ATOMIC_RELAXED); }
#else
__device__ __forceinline__ void zoom_umin(uint32_t* p, uint32_t v) { __hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void zoom_umax(uint32_t* p, uint32_t v) { __hip_atomic_fetch_max(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void zoom_add_lds(int32_t* p, int32_t v) { __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ __forceinline__ void zoom_add64(long long* p, long long v) { __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
#endif

constexpr int kPad = 12;                // scipy's npad for mode 'nearest'
constexpr int kMargin = 2;              // coefficients kept on either side of a line
constexpr int kZoomHeadBytes = 256;     // the front of the workspace: min keys [8], max keys [8]
constexpr int kZoomMaxC = SEGM_PREP_MAX_CHANNELS;
constexpr int kBinNeg = 256, kBinHigh = 257;

// floats in their order as unsigned integers
__device__ __forceinline__ uint32_t zoom_key(float f) {
    const uint32_t b = __float_as_uint(f);
    return b ^ ((b >> 31) ? 0xffffffffu : 0x80000000u);
}
__device__ __forceinline__ float zoom_unkey(uint32_t k) {
    return __uint_as_float(k ^ ((k >> 31) ? 0x80000000u : 0xffffffffu));
}

// ---- channel minimum and maximum ------------------------------------------------------------------------------------------------------
struct MinMaxDev {
    const float* data;
    uint32_t* keys;                     // [0..7] min, [8..15] max
    int64_t sc, sz, sy;
    int32_t H, W, rows;
};

__global__ void __launch_bounds__(kBlock) zoom_minmax_kernel(MinMaxDev P) {
    __shared__ float s_lo[kWavesPerBlock], s_hi[kWavesPerBlock];
    const int c = blockIdx.y;
    float lo = INFINITY, hi = -INFINITY;
    for (int row = blockIdx.x; row < P.rows; row += gridDim.x) {
        const int z = row / P.H, y = row - z * P.H;
        const float* p = P.data + (int64_t)c * P.sc + (int64_t)z * P.sz + (int64_t)y * P.sy;
        for (int x = threadIdx.x; x < P.W; x += kBlock) {
            const float v = p[x];
            lo = v < lo ? v : lo;
            hi = v > hi ? v : hi;
        }
    }
    for (int off = kWave / 2; off >= 1; off >>= 1) {
        const float a = __shfl_xor(lo, off), b = __shfl_xor(hi, off);
        lo = a < lo ? a : lo;
        hi = b > hi ? b : hi;
    }
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    if (lane == 0) { s_lo[wave] = lo; s_hi[wave] = hi; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < kWavesPerBlock; ++w) {
            lo = s_lo[w] < lo ? s_lo[w] : lo;
            hi = s_hi[w] > hi ? s_hi[w] : hi;
        }
        if (lo <= hi) {                               // the workgroup saw a row
            zoom_umin(P.keys + c, zoom_key(lo));
            zoom_umax(P.keys + kZoomMaxC + c, zoom_key(hi));
        }
    }
}

// ---- prefilter along x ----------------------------------------------------------------------------------------------------------------
struct FirDev {
    const float* data;
    double* coef;                       // (C, D + 4, H + 4, W + 4)
    int64_t sc, sz, sy;
    int64_t cs, zs, ys;                 // the coefficients' strides
    int32_t H, W, tiles;
};

// ZM: the coefficients' margin along z - kMargin for the volume zoom, 0 for the slice zoom, which has no pass along the slice axis
template <int ZM>
__global__ void __launch_bounds__(kBlock) zoom_fir_x_kernel(FirDev P) {
    __shared__ double s_in[kBlock + 2 * kFirTaps];
    const int row = blockIdx.x / P.tiles, tile = blockIdx.x - row * P.tiles;
    const int zz = row / P.H, yy = row - zz * P.H;
    const int i0 = tile * kBlock - kMargin;           // the tile's first output, as an index of the unpadded line
    const float* src = P.data + (int64_t)blockIdx.y * P.sc + (int64_t)zz * P.sz + (int64_t)yy * P.sy;
    const int N = P.W + 2 * kPad, period = 2 * N - 2;
    for (int e = threadIdx.x; e < kBlock + 2 * kFirTaps; e += kBlock) {
        int p = (i0 - kFirTaps + e + kPad) % period;  // index of the padded line, mirrored at 0 and at N - 1
        p = p < 0 ? p + period : p;
        p = p > N - 1 ? period - p : p;
        int j = p - kPad;
        j = j < 0 ? 0 : (j > P.W - 1 ? P.W - 1 : j);
        s_in[e] = (double)src[j];
    }
    __syncthreads();
    const int i = i0 + (int)threadIdx.x;
    if (i > P.W + kMargin - 1) return;
    const int e = threadIdx.x + kFirTaps;
    double hk = kFir0, acc = kFir0 * s_in[e];
#pragma unroll 8
    for (int k = 1; k <= kFirTaps; ++k) {
        hk *= kPole;
        acc += hk * (s_in[e - k] + s_in[e + k]);
    }
    P.coef[(int64_t)blockIdx.y * P.cs + (int64_t)(zz + ZM) * P.zs + (int64_t)(yy + kMargin) * P.ys + (i + kMargin)] = acc;
}

// ---- prefilter along a strided axis, in place -----------------------------------------------------------------------------------------
struct LineDev {
    double* coef;
    int64_t cs;                         // channel stride
    int64_t stride;                     // between the slots of a line
    int64_t inner, outer_stride, outer_off, lines;    // line t starts at outer_off + (t / inner) * outer_stride + t % inner
    double zn1;                         // z^(n + 23)
    int32_t n;
};

// Slot k of a line is logical index k - 2; on entry the slots 2 .. n + 1 hold the input, on exit all n + 4 hold coefficients.
__global__ void __launch_bounds__(kBlock) zoom_line_kernel(LineDev P) {
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (t >= P.lines) return;
    const int64_t o = t / P.inner, in = t - o * P.inner;
    double* p = P.coef + (int64_t)blockIdx.y * P.cs + P.outer_off + o * P.outer_stride + in;
    const int64_t s = P.stride;
    const int n = P.n, N = n + 2 * kPad;
    const double z = kPole;
    const double s0 = kGain * p[kMargin * s], sl = kGain * p[(int64_t)(n - 1 + kMargin) * s];
    // scipy's _init_causal_mirror on the padded line, cut where the pole's power no longer counts
    double acc = s0 + P.zn1 * sl, zi = z;
    const int terms = N - 1 < kInitTerms ? N - 1 : kInitTerms;
    for (int k = 1; k < terms; ++k) {
        const int ja = k - kPad, jb = n + kPad - 1 - k;
        const double a = ja <= 0 ? s0 : (ja >= n - 1 ? sl : kGain * p[(int64_t)(ja + kMargin) * s]);
        const double b = jb <= 0 ? s0 : (jb >= n - 1 ? sl : kGain * p[(int64_t)(jb + kMargin) * s]);
        acc += zi * (a + P.zn1 * b);
        zi *= z;
    }
    double cp = acc / (1.0 - P.zn1 * P.zn1);          // the causal value at logical -12
#pragma unroll
    for (int j = -kPad + 1; j < -kMargin; ++j) cp = s0 + z * cp;
    cp = s0 + z * cp; p[0] = cp;
    cp = s0 + z * cp; p[s] = cp;
    for (int j0 = 0; j0 < n; j0 += kLineBatch) {
        double v[kLineBatch];
#pragma unroll
        for (int k = 0; k < kLineBatch; ++k) v[k] = j0 + k < n ? p[(int64_t)(j0 + k + kMargin) * s] : 0.0;
#pragma unroll
        for (int k = 0; k < kLineBatch; ++k) {
            if (j0 + k < n) {
                cp = kGain * v[k] + z * cp;
                p[(int64_t)(j0 + k + kMargin) * s] = cp;
            }
        }
    }
    cp = sl + z * cp; p[(int64_t)(n + kMargin) * s] = cp;
    cp = sl + z * cp; p[(int64_t)(n + kMargin + 1) * s] = cp;
    double tail[kPad - kMargin];                      // logical n + 2 .. n + 11
#pragma unroll
    for (int k = 0; k < kPad - kMargin; ++k) { cp = sl + z * cp; tail[k] = cp; }
    double c = (z * tail[kPad - kMargin - 2] + tail[kPad - kMargin - 1]) * (z / (z * z - 1.0));
#pragma unroll
    for (int k = kPad - kMargin - 2; k >= 0; --k) c = z * (c - tail[k]);
    for (int q0 = n + 2 * kMargin - 1; q0 >= 0; q0 -= kLineBatch) {
        double v[kLineBatch];
#pragma unroll
        for (int k = 0; k < kLineBatch; ++k) v[k] = q0 - k >= 0 ? p[(int64_t)(q0 - k) * s] : 0.0;
#pragma unroll
        for (int k = 0; k < kLineBatch; ++k) {
            if (q0 - k >= 0) {
                c = z * (c - v[k]);
                p[(int64_t)(q0 - k) * s] = c;
            }
        }
    }
}

// ---- evaluation -----------------------------------------------------------------------------------------------------------------------
struct EvalDev {
    const double* coef;
    const float* data;
    const uint32_t* keys;
    float* out;
    int64_t sc, sz, sy;
    int64_t cs, zs, ys;
    int64_t nout;
    double rz, ry, rx;                  // n_in / n_out
    int32_t D, H, W, d, h, w;
    int32_t order, clip;
};

// first slot (of n + 4) and the weights of the four taps: scipy's get_spline_interpolation_weights, order 3
__device__ __forceinline__ void cubic_taps(int i, double r, int n, int& slot, double w[4]) {
    const double u = ((double)i + 0.5) * r - 0.5 + (double)kPad;
    const double fl = floor(u), y = u - fl, zc = 1.0 - y;
    w[1] = (y * y * (y - 2.0) * 3.0 + 4.0) / 6.0;
    w[2] = (zc * zc * (zc - 2.0) * 3.0 + 4.0) / 6.0;
    w[0] = zc * zc * zc / 6.0;
    w[3] = 1.0 - w[0] - w[1] - w[2];
    const int q = (int)fl - kPad - 1 + kMargin;
    slot = q < 0 ? 0 : (q > n ? n : q);               // always inside already: (i + 0.5) r - 0.5 lies in (-0.5, n - 0.5)
}

// the two taps and weights of order 1, the coordinate clamped to the line as scipy's mode 'nearest' maps it
__device__ __forceinline__ void linear_taps(int i, double r, int n, int& i0, int& i1, double& w0, double& w1) {
    double u = ((double)i + 0.5) * r - 0.5;
    u = u < 0.0 ? 0.0 : (u > (double)(n - 1) ? (double)(n - 1) : u);
    const double fl = floor(u);
    w1 = u - fl;
    w0 = 1.0 - w1;
    i0 = (int)fl;
    i0 = i0 < 0 ? 0 : (i0 > n - 1 ? n - 1 : i0);
    i1 = i0 + 1 > n - 1 ? n - 1 : i0 + 1;
}

__global__ void __launch_bounds__(kBlock) zoom_eval_kernel(EvalDev P) {
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (t >= P.nout) return;
    const int c = blockIdx.y;
    const int64_t row = t / P.w;
    const int ox = (int)(t - row * P.w), oz = (int)(row / P.h), oy = (int)(row - (int64_t)oz * P.h);
    double acc = 0.0;
    if (P.order == 3) {
        int qz, qy, qx;
        double wz[4], wy[4], wx[4];
        cubic_taps(oz, P.rz, P.D, qz, wz);
        cubic_taps(oy, P.ry, P.H, qy, wy);
        cubic_taps(ox, P.rx, P.W, qx, wx);
        const double* base = P.coef + (int64_t)c * P.cs + (int64_t)qz * P.zs + (int64_t)qy * P.ys + qx;
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            double sa = 0.0;
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const double* r = base + a * P.zs + b * P.ys;
                sa += wy[b] * (wx[0] * r[0] + wx[1] * r[1] + wx[2] * r[2] + wx[3] * r[3]);
            }
            acc += wz[a] * sa;
        }
    } else {
        int z0, z1, y0, y1, x0, x1;
        double wz0, wz1, wy0, wy1, wx0, wx1;
        linear_taps(oz, P.rz, P.D, z0, z1, wz0, wz1);
        linear_taps(oy, P.ry, P.H, y0, y1, wy0, wy1);
        linear_taps(ox, P.rx, P.W, x0, x1, wx0, wx1);
        const float* base = P.data + (int64_t)c * P.sc;
        const float* r00 = base + (int64_t)z0 * P.sz + (int64_t)y0 * P.sy;
        const float* r01 = base + (int64_t)z0 * P.sz + (int64_t)y1 * P.sy;
        const float* r10 = base + (int64_t)z1 * P.sz + (int64_t)y0 * P.sy;
        const float* r11 = base + (int64_t)z1 * P.sz + (int64_t)y1 * P.sy;
        const double a0 = wy0 * (wx0 * (double)r00[x0] + wx1 * (double)r00[x1]) + wy1 * (wx0 * (double)r01[x0] + wx1 * (double)r01[x1]);
        const double a1 = wy0 * (wx0 * (double)r10[x0] + wx1 * (double)r10[x1]) + wy1 * (wx0 * (double)r11[x0] + wx1 * (double)r11[x1]);
        acc = wz0 * a0 + wz1 * a1;
    }
    if (P.clip) {
        const double lo = (double)zoom_unkey(P.keys[c]), hi = (double)zoom_unkey(P.keys[kZoomMaxC + c]);
        acc = acc < lo ? lo : (acc > hi ? hi : acc);
    }
    P.out[(int64_t)c * P.nout + t] = (float)acc;
}

// ---- labels ---------------------------------------------------------------------------------------------------------------------------
struct LabelsDev {
    const int16_t* seg;
    int16_t* out;
    long long* counts;
    int64_t nout;
    double rz, ry, rx;
    int32_t D, H, W, d, h, w;
};

// the largest label whose corner weights sum to one half or more, 0 if none does; the sums run over the corners in their order
template <int N>
__device__ __forceinline__ int32_t zoom_pick_label(const int32_t (&lab)[N], const double (&wgt)[N]) {
    int32_t best = INT32_MIN;
#pragma unroll
    for (int m = 0; m < N; ++m) {
        double sum = 0.0;
#pragma unroll
        for (int q = 0; q < N; ++q) sum += lab[q] == lab[m] ? wgt[q] : 0.0;
        if (sum >= 0.5 && lab[m] > best) best = lab[m];
    }
    return best == INT32_MIN ? 0 : best;
}

// The label counts of a workgroup's results into counts[SEGM_PREP_COUNT_BINS], in three steps over s_hist[SEGM_PREP_COUNT_BINS] and
// s_two[kWavesPerBlock][2] in LDS: clear; per result, labels 1 .. 255 and the bin above through LDS atomics, the two frequent ones
// (negative, 0) in registers; at the end those two through wave shuffles, then one 64-bit atomic per non-empty bin.  Every thread of
// the workgroup calls the first and the last.
__device__ __forceinline__ void zoom_count_begin(int32_t* s_hist) {
    for (int b = threadIdx.x; b < SEGM_PREP_COUNT_BINS; b += kBlock) s_hist[b] = 0;
    __syncthreads();
}

__device__ __forceinline__ void zoom_count_add(int32_t* s_hist, int32_t& n_neg, int32_t& n_zero, int32_t res) {
    if (res < 0) ++n_neg;
    else if (res == 0) ++n_zero;
    else zoom_add_lds(&s_hist[res > 255 ? kBinHigh : res], 1);
}

__device__ __forceinline__ void zoom_count_end(long long* counts, int32_t* s_hist, int32_t (*s_two)[2], int32_t n_neg, int32_t n_zero) {
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    for (int off = kWave / 2; off >= 1; off >>= 1) {
        n_neg += __shfl_xor(n_neg, off);
        n_zero += __shfl_xor(n_zero, off);
    }
    if (lane == 0) { s_two[wave][0] = n_neg; s_two[wave][1] = n_zero; }
    __syncthreads();
    if (threadIdx.x == 0) {
        int32_t a = 0, b = 0;
        for (int w = 0; w < kWavesPerBlock; ++w) { a += s_two[w][0]; b += s_two[w][1]; }
        s_hist[kBinNeg] = a;
        s_hist[0] = b;
    }
    __syncthreads();
    for (int b = threadIdx.x; b < SEGM_PREP_COUNT_BINS; b += kBlock) {
        const int32_t n = s_hist[b];
        if (n) zoom_add64(counts + b, (long long)n);
    }
}

__global__ void __launch_bounds__(kBlock) zoom_labels_kernel(LabelsDev P) {
    __shared__ int32_t s_hist[SEGM_PREP_COUNT_BINS];
    __shared__ int32_t s_two[kWavesPerBlock][2];
    zoom_count_begin(s_hist);
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    int32_t n_neg = 0, n_zero = 0;
    if (t < P.nout) {
        const int64_t row = t / P.w;
        const int ox = (int)(t - row * P.w), oz = (int)(row / P.h), oy = (int)(row - (int64_t)oz * P.h);
        int iz[2], iy[2], ix[2];
        double wz[2], wy[2], wx[2];
        linear_taps(oz, P.rz, P.D, iz[0], iz[1], wz[0], wz[1]);
        linear_taps(oy, P.ry, P.H, iy[0], iy[1], wy[0], wy[1]);
        linear_taps(ox, P.rx, P.W, ix[0], ix[1], wx[0], wx[1]);
        int32_t lab[8];
        double wgt[8];
#pragma unroll
        for (int m = 0; m < 8; ++m) {
            const int a = m >> 2, b = (m >> 1) & 1, c = m & 1;
            lab[m] = P.seg[((int64_t)iz[a] * P.H + iy[b]) * P.W + ix[c]];
            wgt[m] = wz[a] * wy[b] * wx[c];
        }
        const int32_t res = zoom_pick_label<8>(lab, wgt);
        P.out[t] = (int16_t)res;
        if (P.counts) zoom_count_add(s_hist, n_neg, n_zero, res);
    }
    if (P.counts) zoom_count_end(P.counts, s_hist, s_two, n_neg, n_zero);       // uniform over the launch
}

// ---- the separate-z branch: every slice zoomed in its plane, output slice k taken from input slice source[k] ---------------------------
// keys of slice s of channel c: the minimum at [c * S + s], the maximum at [C * S + c * S + s]
struct SliceMinMaxDev {
    const float* data;
    uint32_t* keys;
    int64_t sc, ss, sy;
    int32_t S, H, W, parts;             // `parts` workgroups share a slice
};

__global__ void __launch_bounds__(kBlock) zoom_slice_minmax_kernel(SliceMinMaxDev P) {
    __shared__ float s_lo[kWavesPerBlock], s_hi[kWavesPerBlock];
    const int c = blockIdx.y, s = blockIdx.x / P.parts, part = blockIdx.x - s * P.parts;
    const float* base = P.data + (int64_t)c * P.sc + (int64_t)s * P.ss;
    float lo = INFINITY, hi = -INFINITY;
    for (int y = part; y < P.H; y += P.parts) {
        const float* p = base + (int64_t)y * P.sy;
        for (int x = threadIdx.x; x < P.W; x += kBlock) {
            const float v = p[x];
            lo = v < lo ? v : lo;
            hi = v > hi ? v : hi;
        }
    }
    for (int off = kWave / 2; off >= 1; off >>= 1) {
        const float a = __shfl_xor(lo, off), b = __shfl_xor(hi, off);
        lo = a < lo ? a : lo;
        hi = b > hi ? b : hi;
    }
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    if (lane == 0) { s_lo[wave] = lo; s_hi[wave] = hi; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < kWavesPerBlock; ++w) {
            lo = s_lo[w] < lo ? s_lo[w] : lo;
            hi = s_hi[w] > hi ? s_hi[w] : hi;
        }
        if (lo <= hi) {                               // parts <= H: every workgroup saw a row
            const int64_t at = (int64_t)c * P.S + s;
            zoom_umin(P.keys + at, zoom_key(lo));
            zoom_umax(P.keys + (int64_t)gridDim.y * P.S + at, zoom_key(hi));
        }
    }
}

struct SliceEvalDev {
    const double* coef;                 // (C, S, H + 4, W + 4): no margin along the slice axis
    const float* data;
    const uint32_t* keys;
    const int32_t* source;
    float* out;
    int64_t sc, ss, sy;
    int64_t cs, zs, ys;
    int64_t nout, plane;                // out_slices * h * w, h * w
    double ry, rx;
    int32_t S, H, W, h, w;
    int32_t order, clip;                // order 0: the in-plane shape is unchanged, the slices are copied
};

__global__ void __launch_bounds__(kBlock) zoom_slices_eval_kernel(SliceEvalDev P) {
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (t >= P.nout) return;
    const int c = blockIdx.y;
    const int k = (int)(t / P.plane);
    const int in = (int)(t - (int64_t)k * P.plane);
    const int oy = in / P.w, ox = in - oy * P.w;
    int s = P.source[k];
    s = s < 0 ? 0 : (s > P.S - 1 ? P.S - 1 : s);
    const float* slice = P.data + (int64_t)c * P.sc + (int64_t)s * P.ss;
    if (P.order == 0) {
        P.out[(int64_t)c * P.nout + t] = slice[(int64_t)oy * P.sy + ox];
        return;
    }
    double acc = 0.0;
    if (P.order == 3) {
        int qy, qx;
        double wy[4], wx[4];
        cubic_taps(oy, P.ry, P.H, qy, wy);
        cubic_taps(ox, P.rx, P.W, qx, wx);
        const double* base = P.coef + (int64_t)c * P.cs + (int64_t)s * P.zs + (int64_t)qy * P.ys + qx;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const double* r = base + b * P.ys;
            acc += wy[b] * (wx[0] * r[0] + wx[1] * r[1] + wx[2] * r[2] + wx[3] * r[3]);
        }
    } else {
        int y0, y1, x0, x1;
        double wy0, wy1, wx0, wx1;
        linear_taps(oy, P.ry, P.H, y0, y1, wy0, wy1);
        linear_taps(ox, P.rx, P.W, x0, x1, wx0, wx1);
        const float* r0 = slice + (int64_t)y0 * P.sy;
        const float* r1 = slice + (int64_t)y1 * P.sy;
        acc = wy0 * (wx0 * (double)r0[x0] + wx1 * (double)r0[x1]) + wy1 * (wx0 * (double)r1[x0] + wx1 * (double)r1[x1]);
    }
    if (P.clip) {
        const int64_t at = (int64_t)c * P.S + s;
        const double lo = (double)zoom_unkey(P.keys[at]), hi = (double)zoom_unkey(P.keys[(int64_t)gridDim.y * P.S + at]);
        acc = acc < lo ? lo : (acc > hi ? hi : acc);
    }
    P.out[(int64_t)c * P.nout + t] = (float)acc;
}

struct LabelSlicesDev {
    const int16_t* seg;
    const int32_t* source;
    int16_t* out;
    long long* counts;
    int64_t nout, plane;
    double ry, rx;
    int32_t S, H, W, h, w;
};

// A workgroup walks the output with the stride of the grid and keeps its counts in LDS until the end: the launch has at most
// kLabelSliceBlocks workgroups, so the 64-bit atomics on one address - bin 0 of every workgroup - stay in the thousands.
constexpr int kLabelSliceBlocks = 2048;

__global__ void __launch_bounds__(kBlock) zoom_labels_slices_kernel(LabelSlicesDev P) {
    __shared__ int32_t s_hist[SEGM_PREP_COUNT_BINS];
    __shared__ int32_t s_two[kWavesPerBlock][2];
    zoom_count_begin(s_hist);
    int32_t n_neg = 0, n_zero = 0;
    for (int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x; t < P.nout; t += (int64_t)gridDim.x * kBlock) {
        const int k = (int)(t / P.plane);
        const int in = (int)(t - (int64_t)k * P.plane);
        const int oy = in / P.w, ox = in - oy * P.w;
        int s = P.source[k];
        s = s < 0 ? 0 : (s > P.S - 1 ? P.S - 1 : s);
        int iy[2], ix[2];
        double wy[2], wx[2];
        linear_taps(oy, P.ry, P.H, iy[0], iy[1], wy[0], wy[1]);
        linear_taps(ox, P.rx, P.W, ix[0], ix[1], wx[0], wx[1]);
        int32_t lab[4];
        double wgt[4];
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            const int b = m >> 1, c = m & 1;
            lab[m] = P.seg[((int64_t)s * P.H + iy[b]) * P.W + ix[c]];
            wgt[m] = wy[b] * wx[c];
        }
        const int32_t res = zoom_pick_label<4>(lab, wgt);
        P.out[t] = (int16_t)res;
        if (P.counts) zoom_count_add(s_hist, n_neg, n_zero, res);
    }
    if (P.counts) zoom_count_end(P.counts, s_hist, s_two, n_neg, n_zero);       // uniform over the launch
}

static inline bool zoom_side_ok(int32_t n) { return n >= 1 && n <= SEGM_ZOOM_MAX_SIDE; }

static inline bool zoom_shape_ok(int32_t a, int32_t b, int32_t c) {
    return zoom_side_ok(a) && zoom_side_ok(b) && zoom_side_ok(c) && (int64_t)a * b * c <= SEGM_CCL_MAX_VOXELS;
}

static inline int64_t zoom_coef_count(int32_t D, int32_t H, int32_t W) {
    return (int64_t)(D + 2 * kMargin) * (H + 2 * kMargin) * (W + 2 * kMargin);
}

}  // namespace segm

using namespace segm;

extern "C" size_t segm_zoom_workspace_bytes(int32_t channels, int32_t depth, int32_t height, int32_t width, int32_t order) {
    if (channels < 1 || channels > SEGM_PREP_MAX_CHANNELS || !zoom_shape_ok(depth, height, width)) return 0;
    if (order != 1 && order != 3) return 0;
    return (size_t)kZoomHeadBytes + (order == 3 ? (size_t)channels * (size_t)zoom_coef_count(depth, height, width) * sizeof(double) : 0);
}

extern "C" int segm_zoom(const segm_zoom_args* a) {
    if (!a) return SEGM_E_NULL;
    if (!a->data || !a->out) return SEGM_E_NULL;
    if (a->channels < 1 || a->channels > SEGM_PREP_MAX_CHANNELS) return SEGM_E_SHAPE;
    if (!zoom_shape_ok(a->depth, a->height, a->width) || !zoom_shape_ok(a->out_depth, a->out_height, a->out_width)) return SEGM_E_SHAPE;
    if (a->order != 1 && a->order != 3) return SEGM_E_SHAPE;
    if (a->clip != 0 && a->clip != 1) return SEGM_E_SHAPE;
    if (a->stride_y < a->width || a->stride_z < 0 || a->stride_c < 0) return SEGM_E_SHAPE;
    if ((uintptr_t)a->data % sizeof(float) || (uintptr_t)a->out % sizeof(float)) return SEGM_E_SHAPE;
    const size_t need = segm_zoom_workspace_bytes(a->channels, a->depth, a->height, a->width, a->order);
    if (!a->workspace || a->workspace_bytes < need || (uintptr_t)a->workspace % sizeof(double)) return SEGM_E_WORKSPACE;
    hipStream_t st = (hipStream_t)a->stream;
    const int C = a->channels, D = a->depth, H = a->height, W = a->width;
    uint32_t* keys = (uint32_t*)a->workspace;
    double* coef = (double*)((char*)a->workspace + kZoomHeadBytes);
    const int64_t ys = W + 2 * kMargin, zs = (int64_t)(H + 2 * kMargin) * ys, cs = (int64_t)(D + 2 * kMargin) * zs;
    if (a->clip) {
        if (hipMemsetAsync(keys, 0xff, kZoomMaxC * sizeof(uint32_t), st) != hipSuccess) return (int)hipGetLastError();
        if (hipMemsetAsync(keys + kZoomMaxC, 0, kZoomMaxC * sizeof(uint32_t), st) != hipSuccess) return (int)hipGetLastError();
        MinMaxDev M;
        memset(&M, 0, sizeof(M));
        M.data = a->data; M.keys = keys;
        M.sc = a->stride_c; M.sz = a->stride_z; M.sy = a->stride_y;
        M.H = H; M.W = W; M.rows = D * H;
        const int blocks = M.rows < 1024 ? M.rows : 1024;
        hipLaunchKernelGGL(zoom_minmax_kernel, dim3((unsigned)blocks, (unsigned)C), dim3(kBlock), 0, st, M);
    }
    if (a->order == 3) {
        FirDev F;
        memset(&F, 0, sizeof(F));
        F.data = a->data; F.coef = coef;
        F.sc = a->stride_c; F.sz = a->stride_z; F.sy = a->stride_y;
        F.cs = cs; F.zs = zs; F.ys = ys;
        F.H = H; F.W = W; F.tiles = (W + 2 * kMargin + kBlock - 1) / kBlock;
        hipLaunchKernelGGL((zoom_fir_x_kernel<kMargin>), dim3((unsigned)((int64_t)D * H * F.tiles), (unsigned)C), dim3(kBlock), 0, st, F);
        LineDev Ly;                                   // along y: a line per (z, x), the x margins included
        memset(&Ly, 0, sizeof(Ly));
        Ly.coef = coef; Ly.cs = cs; Ly.stride = ys;
        Ly.inner = ys; Ly.outer_stride = zs; Ly.outer_off = kMargin * zs; Ly.lines = (int64_t)D * ys;
        Ly.n = H; Ly.zn1 = pow(kPole, (double)(H + 2 * kPad - 1));
        hipLaunchKernelGGL(zoom_line_kernel, dim3((unsigned)((Ly.lines + kBlock - 1) / kBlock), (unsigned)C), dim3(kBlock), 0, st, Ly);
        LineDev Lz;                                   // along z: a line per (y, x), both margins included
        memset(&Lz, 0, sizeof(Lz));
        Lz.coef = coef; Lz.cs = cs; Lz.stride = zs;
        Lz.inner = zs; Lz.outer_stride = 0; Lz.outer_off = 0; Lz.lines = zs;
        Lz.n = D; Lz.zn1 = pow(kPole, (double)(D + 2 * kPad - 1));
        hipLaunchKernelGGL(zoom_line_kernel, dim3((unsigned)((Lz.lines + kBlock - 1) / kBlock), (unsigned)C), dim3(kBlock), 0, st, Lz);
    }
    EvalDev E;
    memset(&E, 0, sizeof(E));
    E.coef = coef; E.data = a->data; E.keys = keys; E.out = a->out;
    E.sc = a->stride_c; E.sz = a->stride_z; E.sy = a->stride_y;
    E.cs = cs; E.zs = zs; E.ys = ys;
    E.D = D; E.H = H; E.W = W; E.d = a->out_depth; E.h = a->out_height; E.w = a->out_width;
    E.nout = (int64_t)E.d * E.h * E.w;
    E.rz = (double)D / (double)E.d; E.ry = (double)H / (double)E.h; E.rx = (double)W / (double)E.w;
    E.order = a->order; E.clip = a->clip;
    hipLaunchKernelGGL(zoom_eval_kernel, dim3((unsigned)((E.nout + kBlock - 1) / kBlock), (unsigned)C), dim3(kBlock), 0, st, E);
    return (int)hipGetLastError();
}

extern "C" int segm_zoom_labels(const segm_zoom_labels_args* a) {
    if (!a) return SEGM_E_NULL;
    if (!a->seg || !a->out) return SEGM_E_NULL;
    if (!zoom_shape_ok(a->depth, a->height, a->width) || !zoom_shape_ok(a->out_depth, a->out_height, a->out_width)) return SEGM_E_SHAPE;
    if ((uintptr_t)a->seg % sizeof(int16_t) || (uintptr_t)a->out % sizeof(int16_t) || (uintptr_t)a->counts % sizeof(int64_t)) return SEGM_E_SHAPE;
    LabelsDev P;
    memset(&P, 0, sizeof(P));
    P.seg = a->seg; P.out = a->out; P.counts = (long long*)a->counts;
    P.D = a->depth; P.H = a->height; P.W = a->width; P.d = a->out_depth; P.h = a->out_height; P.w = a->out_width;
    P.nout = (int64_t)P.d * P.h * P.w;
    P.rz = (double)P.D / (double)P.d; P.ry = (double)P.H / (double)P.h; P.rx = (double)P.W / (double)P.w;
    hipStream_t st = (hipStream_t)a->stream;
    if (a->counts && hipMemsetAsync(a->counts, 0, SEGM_PREP_COUNT_BINS * sizeof(int64_t), st) != hipSuccess) return (int)hipGetLastError();
    hipLaunchKernelGGL(zoom_labels_kernel, dim3((unsigned)((P.nout + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, P);
    return (int)hipGetLastError();
}

// the head of the slice zoom's workspace: 2 * channels * slices keys, rounded up to 256 bytes
static inline size_t zoom_slices_head_bytes(int32_t channels, int32_t slices) {
    const size_t keys = (size_t)2 * channels * slices * sizeof(uint32_t);
    return (keys + kZoomHeadBytes - 1) / kZoomHeadBytes * kZoomHeadBytes;
}

extern "C" size_t segm_zoom_slices_workspace_bytes(int32_t channels, int32_t slices, int32_t height, int32_t width, int32_t out_height,
                                                   int32_t out_width, int32_t order) {
    if (channels < 1 || channels > SEGM_PREP_MAX_CHANNELS || !zoom_shape_ok(slices, height, width)) return 0;
    if (!zoom_side_ok(out_height) || !zoom_side_ok(out_width) || (order != 1 && order != 3)) return 0;
    const bool coefs = order == 3 && (out_height != height || out_width != width);
    return zoom_slices_head_bytes(channels, slices)
           + (coefs ? (size_t)channels * slices * (size_t)(height + 2 * kMargin) * (width + 2 * kMargin) * sizeof(double) : 0);
}

extern "C" int segm_zoom_slices(const segm_zoom_slices_args* a) {
    if (!a) return SEGM_E_NULL;
    if (!a->data || !a->out || !a->source) return SEGM_E_NULL;
    if (a->channels < 1 || a->channels > SEGM_PREP_MAX_CHANNELS) return SEGM_E_SHAPE;
    if (!zoom_shape_ok(a->slices, a->height, a->width) || !zoom_shape_ok(a->out_slices, a->out_height, a->out_width)) return SEGM_E_SHAPE;
    if (a->order != 1 && a->order != 3) return SEGM_E_SHAPE;
    if (a->clip != 0 && a->clip != 1) return SEGM_E_SHAPE;
    if (a->stride_y < a->width || a->stride_s < 0 || a->stride_c < 0) return SEGM_E_SHAPE;
    if ((uintptr_t)a->data % sizeof(float) || (uintptr_t)a->out % sizeof(float) || (uintptr_t)a->source % sizeof(int32_t)) return SEGM_E_SHAPE;
    const size_t need = segm_zoom_slices_workspace_bytes(a->channels, a->slices, a->height, a->width, a->out_height, a->out_width, a->order);
    if (!a->workspace || a->workspace_bytes < need || (uintptr_t)a->workspace % sizeof(double)) return SEGM_E_WORKSPACE;
    hipStream_t st = (hipStream_t)a->stream;
    const int C = a->channels, S = a->slices, H = a->height, W = a->width;
    const bool copy = a->out_height == H && a->out_width == W;
    uint32_t* keys = (uint32_t*)a->workspace;
    double* coef = (double*)((char*)a->workspace + zoom_slices_head_bytes(C, S));
    const int64_t ys = W + 2 * kMargin, zs = (int64_t)(H + 2 * kMargin) * ys, cs = (int64_t)S * zs;
    if (a->clip && !copy) {
        const size_t half = (size_t)C * S * sizeof(uint32_t);
        if (hipMemsetAsync(keys, 0xff, half, st) != hipSuccess) return (int)hipGetLastError();
        if (hipMemsetAsync(keys + (size_t)C * S, 0, half, st) != hipSuccess) return (int)hipGetLastError();
        SliceMinMaxDev M;
        memset(&M, 0, sizeof(M));
        M.data = a->data; M.keys = keys;
        M.sc = a->stride_c; M.ss = a->stride_s; M.sy = a->stride_y;
        M.S = S; M.H = H; M.W = W; M.parts = H < 16 ? H : 16;
        hipLaunchKernelGGL(zoom_slice_minmax_kernel, dim3((unsigned)(S * M.parts), (unsigned)C), dim3(kBlock), 0, st, M);
    }
    if (a->order == 3 && !copy) {
        FirDev F;
        memset(&F, 0, sizeof(F));
        F.data = a->data; F.coef = coef;
        F.sc = a->stride_c; F.sz = a->stride_s; F.sy = a->stride_y;
        F.cs = cs; F.zs = zs; F.ys = ys;
        F.H = H; F.W = W; F.tiles = (W + 2 * kMargin + kBlock - 1) / kBlock;
        hipLaunchKernelGGL((zoom_fir_x_kernel<0>), dim3((unsigned)((int64_t)S * H * F.tiles), (unsigned)C), dim3(kBlock), 0, st, F);
        LineDev Ly;                                   // along y: a line per (slice, x), the x margins included
        memset(&Ly, 0, sizeof(Ly));
        Ly.coef = coef; Ly.cs = cs; Ly.stride = ys;
        Ly.inner = ys; Ly.outer_stride = zs; Ly.outer_off = 0; Ly.lines = (int64_t)S * ys;
        Ly.n = H; Ly.zn1 = pow(kPole, (double)(H + 2 * kPad - 1));
        hipLaunchKernelGGL(zoom_line_kernel, dim3((unsigned)((Ly.lines + kBlock - 1) / kBlock), (unsigned)C), dim3(kBlock), 0, st, Ly);
    }
    SliceEvalDev E;
    memset(&E, 0, sizeof(E));
    E.coef = coef; E.data = a->data; E.keys = keys; E.source = a->source; E.out = a->out;
    E.sc = a->stride_c; E.ss = a->stride_s; E.sy = a->stride_y;
    E.cs = cs; E.zs = zs; E.ys = ys;
    E.S = S; E.H = H; E.W = W; E.h = a->out_height; E.w = a->out_width;
    E.plane = (int64_t)E.h * E.w; E.nout = (int64_t)a->out_slices * E.plane;
    E.ry = (double)H / (double)E.h; E.rx = (double)W / (double)E.w;
    E.order = copy ? 0 : a->order; E.clip = copy ? 0 : a->clip;
    hipLaunchKernelGGL(zoom_slices_eval_kernel, dim3((unsigned)((E.nout + kBlock - 1) / kBlock), (unsigned)C), dim3(kBlock), 0, st, E);
    return (int)hipGetLastError();
}

extern "C" int segm_zoom_labels_slices(const segm_zoom_labels_slices_args* a) {
    if (!a) return SEGM_E_NULL;
    if (!a->seg || !a->out || !a->source) return SEGM_E_NULL;
    if (!zoom_shape_ok(a->slices, a->height, a->width) || !zoom_shape_ok(a->out_slices, a->out_height, a->out_width)) return SEGM_E_SHAPE;
    if ((uintptr_t)a->seg % sizeof(int16_t) || (uintptr_t)a->out % sizeof(int16_t) || (uintptr_t)a->counts % sizeof(int64_t)
        || (uintptr_t)a->source % sizeof(int32_t)) return SEGM_E_SHAPE;
    LabelSlicesDev P;
    memset(&P, 0, sizeof(P));
    P.seg = a->seg; P.source = a->source; P.out = a->out; P.counts = (long long*)a->counts;
    P.S = a->slices; P.H = a->height; P.W = a->width; P.h = a->out_height; P.w = a->out_width;
    P.plane = (int64_t)P.h * P.w; P.nout = (int64_t)a->out_slices * P.plane;
    P.ry = (double)P.H / (double)P.h; P.rx = (double)P.W / (double)P.w;
    hipStream_t st = (hipStream_t)a->stream;
    if (a->counts && hipMemsetAsync(a->counts, 0, SEGM_PREP_COUNT_BINS * sizeof(int64_t), st) != hipSuccess) return (int)hipGetLastError();
    const int64_t blocks = (P.nout + kBlock - 1) / kBlock;
    hipLaunchKernelGGL(zoom_labels_slices_kernel, dim3((unsigned)(blocks < kLabelSliceBlocks ? blocks : kLabelSliceBlocks)), dim3(kBlock), 0, st, P);
    return (int)hipGetLastError();
}
