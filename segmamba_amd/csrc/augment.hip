// Training augmentation at the reference's interpolation orders (C ABI: segm_spline_coefs, segm_spline_coefs_workspace_bytes,
// segm_affine_spline3, segm_affine_labels, segm_zoom_nearest, segm_gauss_blur).
//
// Replaces what batchgenerators does on the host for the reference's get_train_transforms (light_training/augment/train_augment.py:29-50):
//   SpatialTransform, data   interpolate_img: map_coordinates(x.astype(float64), p, order=3, mode='constant', cval=0).astype(float32)
//   SpatialTransform, seg    interpolate_img(is_seg=True, order=1, cval=-1): per label in ascending order
//                            result[map_coordinates(seg == c, order=1, mode='constant', cval=-1) >= 0.5] = c on a volume of zeros
//   SimulateLowResolution    the way down: skimage resize(order=0, mode='edge', anti_aliasing=False) = scipy zoom(order=0, grid_mode=True)
//   GaussianBlur             scipy.ndimage.gaussian_filter(x_fp32, sigma): truncate 4 sigma, mode 'reflect'
//
// A batch is (samples <= 8, channels <= 8, D, H, W) fp32 with element strides and a unit stride along x; the per-launch parameters -
// matrices, sigmas, on / off flags - are part of the kernel arguments.
//   * aug_fir_x_kernel       the prefilter along x, as zoom_fir_x_kernel of resample.hip: a tile of the row in LDS and the closed-form
//                            symmetric FIR, but the mirror is taken on the bare line (... c b a b c ..., as many reflections as a
//                            line shorter than the 32 taps needs).  fp32 in, fp64 coefficients out, unpadded.
//   * aug_line_kernel        y, then z, in place: one thread per line and lanes across x.  The start value is scipy's
//                            _init_causal_mirror: the whole finite sum when the line has at most 40 terms, the sum cut there otherwise.
//   * aug_affine_kernel      one thread per output voxel, the coordinates and the 12 weights shared by the sample's channels; 64 taps
//                            per channel from the coefficients, fp64, one rounding.
//   * aug_labels_kernel      the trilinear weights of the 8 corners summed per distinct corner label, as zoom_labels_kernel.
//   * aug_nearest_kernel     order-0 zoom.
//   * aug_blur_kernel        one separable pass (z, y or x) with the weights in the kernel arguments, fp64 sum, fp32 out.  Three
//                            launches per call; the neighbours of a voxel along y and x are served by the caches (no LDS tile).
// Every sum has a fixed order and there are no floating-point atomics: two calls are bit-equal.
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include "segm_device.h"
#include "spline_common.h"

namespace segm {

constexpr int kAugMaxN = SEGM_AUG_MAX_SAMPLES;
constexpr int kAugMaxC = SEGM_PREP_MAX_CHANNELS;
constexpr int kAugMaxV = SEGM_AUG_MAX_VOLUMES;
constexpr int kBlurMaxR = SEGM_BLUR_MAX_RADIUS;

// ... c b a b c ...: index q of the line mirrored at 0 and at n - 1, any number of times
__device__ __forceinline__ int mirror_idx(int q, int n) {
    if (n == 1) return 0;
    const int period = 2 * n - 2;
    q %= period;
    q = q < 0 ? q + period : q;
    return q > n - 1 ? period - q : q;
}

// d c b a | a b c d: index q of the line reflected about its edges, any number of times
__device__ __forceinline__ int reflect_idx(int q, int n) {
    const int period = 2 * n;
    q %= period;
    q = q < 0 ? q + period : q;
    return q > n - 1 ? period - 1 - q : q;
}

// ---- prefilter along x ----------------------------------------------------------------------------------------------------------------
struct AugFirDev {
    const float* data;
    double* coef;                       // (samples, channels, D, H, W)
    int64_t sn, sc, sz, sy;
    int32_t C, H, W, tiles, rows;       // rows = D * H
    uint8_t on[kAugMaxN];
};

__global__ void __launch_bounds__(kBlock) aug_fir_x_kernel(AugFirDev P) {
    __shared__ double s_in[kBlock + 2 * kFirTaps];
    const int v = blockIdx.y, b = v / P.C, c = v - b * P.C;
    if (!P.on[b]) return;                             // uniform over the workgroup
    const int row = blockIdx.x / P.tiles, tile = blockIdx.x - row * P.tiles;
    const int zz = row / P.H, yy = row - zz * P.H;
    const int i0 = tile * kBlock;
    const float* src = P.data + (int64_t)b * P.sn + (int64_t)c * P.sc + (int64_t)zz * P.sz + (int64_t)yy * P.sy;
    for (int e = threadIdx.x; e < kBlock + 2 * kFirTaps; e += kBlock) s_in[e] = (double)src[mirror_idx(i0 - kFirTaps + e, P.W)];
    __syncthreads();
    const int i = i0 + (int)threadIdx.x;
    if (i > P.W - 1) return;
    const int e = threadIdx.x + kFirTaps;
    double acc = s_in[e];                             // a line of one voxel is left unfiltered, as scipy leaves it
    if (P.W > 1) {
        double hk = kFir0;
        acc = kFir0 * s_in[e];
#pragma unroll 8
        for (int k = 1; k <= kFirTaps; ++k) {
            hk *= kPole;
            acc += hk * (s_in[e - k] + s_in[e + k]);
        }
    }
    P.coef[((int64_t)v * P.rows + row) * P.W + i] = acc;
}

// ---- prefilter along a strided axis, in place -----------------------------------------------------------------------------------------
struct AugLineDev {
    double* coef;
    int64_t vs;                         // volume stride
    int64_t stride;                     // between the voxels of a line
    int64_t inner, outer_stride, lines; // line t starts at (t / inner) * outer_stride + t % inner
    double zn1;                         // z^(n - 1)
    int32_t n, C;                       // n >= 2
    uint8_t on[kAugMaxN];
};

__global__ void __launch_bounds__(kBlock) aug_line_kernel(AugLineDev P) {
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const int v = blockIdx.y;
    if (t >= P.lines || !P.on[v / P.C]) return;
    const int64_t o = t / P.inner, in = t - o * P.inner;
    double* p = P.coef + (int64_t)v * P.vs + o * P.outer_stride + in;
    const int64_t s = P.stride;
    const int n = P.n;
    const double z = kPole;
    // scipy's _init_causal_mirror
    double acc = kGain * p[0] + P.zn1 * (kGain * p[(int64_t)(n - 1) * s]), zi = z;
    const int terms = n - 1 < kInitTerms ? n - 1 : kInitTerms;
    for (int k = 1; k < terms; ++k) {
        acc += zi * (kGain * p[(int64_t)k * s] + P.zn1 * (kGain * p[(int64_t)(n - 1 - k) * s]));
        zi *= z;
    }
    double cp = acc / (1.0 - P.zn1 * P.zn1), before = cp;
    p[0] = cp;
    for (int j0 = 1; j0 < n; j0 += kLineBatch) {
        double v8[kLineBatch];
#pragma unroll
        for (int k = 0; k < kLineBatch; ++k) v8[k] = j0 + k < n ? p[(int64_t)(j0 + k) * s] : 0.0;
#pragma unroll
        for (int k = 0; k < kLineBatch; ++k) {
            if (j0 + k < n) {
                before = cp;
                cp = kGain * v8[k] + z * cp;
                p[(int64_t)(j0 + k) * s] = cp;
            }
        }
    }
    double c = (z * before + cp) * (z / (z * z - 1.0));   // _init_anticausal_mirror
    p[(int64_t)(n - 1) * s] = c;
    for (int q0 = n - 2; q0 >= 0; q0 -= kLineBatch) {
        double v8[kLineBatch];
#pragma unroll
        for (int k = 0; k < kLineBatch; ++k) v8[k] = q0 - k >= 0 ? p[(int64_t)(q0 - k) * s] : 0.0;
#pragma unroll
        for (int k = 0; k < kLineBatch; ++k) {
            if (q0 - k >= 0) {
                c = z * (c - v8[k]);
                p[(int64_t)(q0 - k) * s] = c;
            }
        }
    }
}

// ---- the affine map -------------------------------------------------------------------------------------------------------------------
struct AugMatrices {
    double m[kAugMaxN][12];
};

// p = A (z, y, x)^T + t of sample b; false where a component leaves [0, n - 1]
__device__ __forceinline__ bool affine_point(const AugMatrices& M, int b, int oz, int oy, int ox, int D, int H, int W, double p[3]) {
    const double* m = M.m[b];
    const double z = (double)oz, y = (double)oy, x = (double)ox;
#pragma unroll
    for (int r = 0; r < 3; ++r) p[r] = m[4 * r] * z + m[4 * r + 1] * y + m[4 * r + 2] * x + m[4 * r + 3];
    return !(p[0] < 0.0 || p[0] > (double)(D - 1) || p[1] < 0.0 || p[1] > (double)(H - 1) || p[2] < 0.0 || p[2] > (double)(W - 1));
}

// the four taps (mirrored into the line) and weights of order 3 at u: scipy's get_spline_interpolation_weights
__device__ __forceinline__ void cubic_taps_at(double u, int n, int idx[4], double w[4]) {
    const double fl = floor(u), y = u - fl, zc = 1.0 - y;
    w[1] = (y * y * (y - 2.0) * 3.0 + 4.0) / 6.0;
    w[2] = (zc * zc * (zc - 2.0) * 3.0 + 4.0) / 6.0;
    w[0] = zc * zc * zc / 6.0;
    w[3] = 1.0 - w[0] - w[1] - w[2];
    const int q = (int)fl - 1;
#pragma unroll
    for (int k = 0; k < 4; ++k) idx[k] = mirror_idx(q + k, n);
}

struct AugAffineDev {
    const double* coef;
    const float* data;
    float* out;
    int64_t sn, sc, sz, sy;
    int64_t nvox;
    AugMatrices M;
    float cval;
    int32_t C, D, H, W;
    uint8_t on[kAugMaxN];
};

__global__ void __launch_bounds__(kBlock) aug_affine_kernel(AugAffineDev P) {
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (t >= P.nvox) return;
    const int b = blockIdx.y;
    const int64_t row = t / P.W;
    const int ox = (int)(t - row * P.W), oz = (int)(row / P.H), oy = (int)(row - (int64_t)oz * P.H);
    float* out = P.out + (int64_t)b * P.C * P.nvox + t;
    if (!P.on[b]) {                                   // uniform over the workgroup
        const float* src = P.data + (int64_t)b * P.sn + (int64_t)oz * P.sz + (int64_t)oy * P.sy + ox;
        for (int c = 0; c < P.C; ++c) out[(int64_t)c * P.nvox] = src[(int64_t)c * P.sc];
        return;
    }
    double p[3];
    if (!affine_point(P.M, b, oz, oy, ox, P.D, P.H, P.W, p)) {
        for (int c = 0; c < P.C; ++c) out[(int64_t)c * P.nvox] = P.cval;
        return;
    }
    int iz[4], iy[4], ix[4];
    double wz[4], wy[4], wx[4];
    cubic_taps_at(p[0], P.D, iz, wz);
    cubic_taps_at(p[1], P.H, iy, wy);
    cubic_taps_at(p[2], P.W, ix, wx);
    const int64_t ys = P.W, zs = (int64_t)P.H * P.W;
    for (int c = 0; c < P.C; ++c) {
        const double* base = P.coef + ((int64_t)b * P.C + c) * P.nvox;
        double acc = 0.0;
#pragma unroll 1                                      // 16 taps in flight: unrolled over z the kernel needs 194 VGPRs (2 waves per SIMD)
        for (int a = 0; a < 4; ++a) {
            double sa = 0.0;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const double* r = base + (int64_t)iz[a] * zs + (int64_t)iy[q] * ys;
                sa += wy[q] * (wx[0] * r[ix[0]] + wx[1] * r[ix[1]] + wx[2] * r[ix[2]] + wx[3] * r[ix[3]]);
            }
            acc += wz[a] * sa;
        }
        out[(int64_t)c * P.nvox] = (float)acc;
    }
}

// ---- labels ---------------------------------------------------------------------------------------------------------------------------
struct AugLabelsDev {
    const void* seg;
    void* out;
    int64_t nvox;
    AugMatrices M;
    int32_t D, H, W;
    uint8_t on[kAugMaxN];
};

template <typename T>
__global__ void __launch_bounds__(kBlock) aug_labels_kernel(AugLabelsDev P) {
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (t >= P.nvox) return;
    const int b = blockIdx.y;
    const T* seg = (const T*)P.seg + (int64_t)b * P.nvox;
    T* out = (T*)P.out + (int64_t)b * P.nvox;
    if (!P.on[b]) {
        out[t] = seg[t];
        return;
    }
    const int64_t row = t / P.W;
    const int ox = (int)(t - row * P.W), oz = (int)(row / P.H), oy = (int)(row - (int64_t)oz * P.H);
    double p[3];
    if (!affine_point(P.M, b, oz, oy, ox, P.D, P.H, P.W, p)) {
        out[t] = (T)0;
        return;
    }
    const int n[3] = {P.D, P.H, P.W};
    int i0[3], i1[3];
    double w0[3], w1[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const double fl = floor(p[r]);
        w1[r] = p[r] - fl;
        w0[r] = 1.0 - w1[r];
        i0[r] = (int)fl;
        i1[r] = mirror_idx(i0[r] + 1, n[r]);          // past the line only where its weight is 0
    }
    int64_t lab[8];
    double wgt[8];
#pragma unroll
    for (int m = 0; m < 8; ++m) {
        const int a = m >> 2, q = (m >> 1) & 1, c = m & 1;
        lab[m] = (int64_t)seg[((int64_t)(a ? i1[0] : i0[0]) * P.H + (q ? i1[1] : i0[1])) * P.W + (c ? i1[2] : i0[2])];
        wgt[m] = (a ? w1[0] : w0[0]) * (q ? w1[1] : w0[1]) * (c ? w1[2] : w0[2]);
    }
    bool any = false;
    int64_t best = 0;
#pragma unroll
    for (int m = 0; m < 8; ++m) {
        double sum = 0.0;
#pragma unroll
        for (int q = 0; q < 8; ++q) sum += lab[q] == lab[m] ? wgt[q] : 0.0;
        if (sum >= 0.5 && (!any || lab[m] > best)) { best = lab[m]; any = true; }
    }
    out[t] = (T)(any ? best : 0);
}

// ---- order-0 zoom ---------------------------------------------------------------------------------------------------------------------
struct AugNearestDev {
    const float* data;
    float* out;
    int64_t sc, sz, sy;
    int64_t nout;
    double rz, ry, rx;                  // n_in / n_out
    int32_t D, H, W, d, h, w;
};

__device__ __forceinline__ int nearest_index(int i, double r, int n) {
    const int q = (int)floor(((double)i + 0.5) * r - 0.5 + 0.5);
    return q < 0 ? 0 : (q > n - 1 ? n - 1 : q);
}

__global__ void __launch_bounds__(kBlock) aug_nearest_kernel(AugNearestDev P) {
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (t >= P.nout) return;
    const int c = blockIdx.y;
    const int64_t row = t / P.w;
    const int ox = (int)(t - row * P.w), oz = (int)(row / P.h), oy = (int)(row - (int64_t)oz * P.h);
    const int iz = nearest_index(oz, P.rz, P.D), iy = nearest_index(oy, P.ry, P.H), ix = nearest_index(ox, P.rx, P.W);
    P.out[(int64_t)c * P.nout + t] = P.data[(int64_t)c * P.sc + (int64_t)iz * P.sz + (int64_t)iy * P.sy + ix];
}

// ---- gaussian blur, one axis ----------------------------------------------------------------------------------------------------------
struct AugBlurDev {
    const float* in;
    float* out;                         // dense (samples, channels, D, H, W)
    int64_t sn, sc, sz, sy;             // of `in`
    int64_t nvox;
    double w[kAugMaxV][kBlurMaxR + 1];  // [0] the centre
    int32_t C, D, H, W;
    int32_t axis, copy_off;             // copy_off: volumes that are off are copied (first pass), else left alone
    int8_t radius[kAugMaxV];
    uint8_t on[kAugMaxV];
};

__global__ void __launch_bounds__(kBlock) aug_blur_kernel(AugBlurDev P) {
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const int v = blockIdx.y;
    if (t >= P.nvox || (!P.on[v] && !P.copy_off)) return;
    const int b = v / P.C, c = v - b * P.C;
    const int64_t row = t / P.W;
    const int ox = (int)(t - row * P.W), oz = (int)(row / P.H), oy = (int)(row - (int64_t)oz * P.H);
    const float* src = P.in + (int64_t)b * P.sn + (int64_t)c * P.sc;
    float* out = P.out + (int64_t)v * P.nvox + t;
    const int64_t at = (int64_t)oz * P.sz + (int64_t)oy * P.sy + ox;
    if (!P.on[v]) {
        *out = src[at];
        return;
    }
    const int n = P.axis == 0 ? P.D : (P.axis == 1 ? P.H : P.W), i = P.axis == 0 ? oz : (P.axis == 1 ? oy : ox);
    const int64_t s = P.axis == 0 ? P.sz : (P.axis == 1 ? P.sy : 1);
    const float* line = src + at - (int64_t)i * s;
    double acc = (double)src[at] * P.w[v][0];
    for (int k = P.radius[v]; k >= 1; --k)            // scipy's symmetric correlate1d: the pairs from the outermost inwards
        acc += ((double)line[(int64_t)reflect_idx(i - k, n) * s] + (double)line[(int64_t)reflect_idx(i + k, n) * s]) * P.w[v][k];
    *out = (float)acc;
}

static inline bool aug_side_ok(int32_t n) { return n >= 1 && n <= SEGM_ZOOM_MAX_SIDE; }

static inline bool aug_shape_ok(int32_t a, int32_t b, int32_t c) {
    return aug_side_ok(a) && aug_side_ok(b) && aug_side_ok(c) && (int64_t)a * b * c <= SEGM_CCL_MAX_VOXELS;
}

static inline bool aug_batch_ok(int32_t samples, int32_t channels, int32_t D, int32_t H, int32_t W) {
    return samples >= 1 && samples <= kAugMaxN && channels >= 1 && channels <= kAugMaxC && aug_shape_ok(D, H, W);
}

static inline bool aug_strides_ok(int64_t sn, int64_t sc, int64_t sz, int64_t sy, int32_t W) {
    return sy >= W && sz >= 0 && sc >= 0 && sn >= 0;
}

static inline unsigned aug_blocks(int64_t n) { return (unsigned)((n + kBlock - 1) / kBlock); }

}  // namespace segm

using namespace segm;

extern "C" size_t segm_spline_coefs_workspace_bytes(int32_t samples, int32_t channels, int32_t depth, int32_t height, int32_t width) {
    if (!aug_batch_ok(samples, channels, depth, height, width)) return 0;
    return (size_t)samples * (size_t)channels * (size_t)depth * (size_t)height * (size_t)width * sizeof(double);
}

extern "C" int segm_spline_coefs(const segm_spline_coefs_args* a) {
    if (!a) return SEGM_E_NULL;
    if (!a->data) return SEGM_E_NULL;
    if (!aug_batch_ok(a->samples, a->channels, a->depth, a->height, a->width)) return SEGM_E_SHAPE;
    if (!aug_strides_ok(a->stride_n, a->stride_c, a->stride_z, a->stride_y, a->width)) return SEGM_E_SHAPE;
    if ((uintptr_t)a->data % sizeof(float)) return SEGM_E_SHAPE;
    const size_t need = segm_spline_coefs_workspace_bytes(a->samples, a->channels, a->depth, a->height, a->width);
    if (!a->workspace || a->workspace_bytes < need || (uintptr_t)a->workspace % sizeof(double)) return SEGM_E_WORKSPACE;
    hipStream_t st = (hipStream_t)a->stream;
    const int N = a->samples, C = a->channels, D = a->depth, H = a->height, W = a->width;
    bool any = false;
    for (int b = 0; b < N; ++b) any = any || a->on[b];
    if (!any) return 0;
    double* coef = (double*)a->workspace;
    AugFirDev F;
    memset(&F, 0, sizeof(F));
    F.data = a->data; F.coef = coef;
    F.sn = a->stride_n; F.sc = a->stride_c; F.sz = a->stride_z; F.sy = a->stride_y;
    F.C = C; F.H = H; F.W = W; F.rows = D * H; F.tiles = (W + kBlock - 1) / kBlock;
    memcpy(F.on, a->on, sizeof(F.on));
    hipLaunchKernelGGL(aug_fir_x_kernel, dim3((unsigned)((int64_t)D * H * F.tiles), (unsigned)(N * C)), dim3(kBlock), 0, st, F);
    const int64_t ys = W, zs = (int64_t)H * W, vs = (int64_t)D * zs;
    if (H > 1) {                                      // along y: a line per (z, x)
        AugLineDev L;
        memset(&L, 0, sizeof(L));
        L.coef = coef; L.vs = vs; L.stride = ys;
        L.inner = W; L.outer_stride = zs; L.lines = (int64_t)D * W;
        L.n = H; L.C = C; L.zn1 = pow(kPole, (double)(H - 1));
        memcpy(L.on, a->on, sizeof(L.on));
        hipLaunchKernelGGL(aug_line_kernel, dim3(aug_blocks(L.lines), (unsigned)(N * C)), dim3(kBlock), 0, st, L);
    }
    if (D > 1) {                                      // along z: a line per (y, x)
        AugLineDev L;
        memset(&L, 0, sizeof(L));
        L.coef = coef; L.vs = vs; L.stride = zs;
        L.inner = zs; L.outer_stride = 0; L.lines = zs;
        L.n = D; L.C = C; L.zn1 = pow(kPole, (double)(D - 1));
        memcpy(L.on, a->on, sizeof(L.on));
        hipLaunchKernelGGL(aug_line_kernel, dim3(aug_blocks(L.lines), (unsigned)(N * C)), dim3(kBlock), 0, st, L);
    }
    return (int)hipGetLastError();
}

extern "C" int segm_affine_spline3(const segm_affine_spline3_args* a) {
    if (!a) return SEGM_E_NULL;
    if (!a->data || !a->out) return SEGM_E_NULL;
    if (!aug_batch_ok(a->samples, a->channels, a->depth, a->height, a->width)) return SEGM_E_SHAPE;
    if (!aug_strides_ok(a->stride_n, a->stride_c, a->stride_z, a->stride_y, a->width)) return SEGM_E_SHAPE;
    if ((uintptr_t)a->data % sizeof(float) || (uintptr_t)a->out % sizeof(float) || (uintptr_t)a->coefs % sizeof(double)) return SEGM_E_SHAPE;
    bool any = false;
    for (int b = 0; b < a->samples; ++b) any = any || a->on[b];
    if (any && !a->coefs) return SEGM_E_NULL;
    AugAffineDev P;
    memset(&P, 0, sizeof(P));
    P.coef = a->coefs; P.data = a->data; P.out = a->out;
    P.sn = a->stride_n; P.sc = a->stride_c; P.sz = a->stride_z; P.sy = a->stride_y;
    P.C = a->channels; P.D = a->depth; P.H = a->height; P.W = a->width;
    P.nvox = (int64_t)P.D * P.H * P.W;
    P.cval = a->cval;
    memcpy(P.M.m, a->matrix, sizeof(P.M.m));
    memcpy(P.on, a->on, sizeof(P.on));
    hipLaunchKernelGGL(aug_affine_kernel, dim3(aug_blocks(P.nvox), (unsigned)a->samples), dim3(kBlock), 0, (hipStream_t)a->stream, P);
    return (int)hipGetLastError();
}

extern "C" int segm_affine_labels(const segm_affine_labels_args* a) {
    if (!a) return SEGM_E_NULL;
    if (!a->seg || !a->out) return SEGM_E_NULL;
    if (a->samples < 1 || a->samples > kAugMaxN || !aug_shape_ok(a->depth, a->height, a->width)) return SEGM_E_SHAPE;
    if (a->wide != 0 && a->wide != 1) return SEGM_E_DTYPE;
    const size_t size = a->wide ? sizeof(int64_t) : sizeof(int16_t);
    if ((uintptr_t)a->seg % size || (uintptr_t)a->out % size) return SEGM_E_SHAPE;
    AugLabelsDev P;
    memset(&P, 0, sizeof(P));
    P.seg = a->seg; P.out = a->out;
    P.D = a->depth; P.H = a->height; P.W = a->width;
    P.nvox = (int64_t)P.D * P.H * P.W;
    memcpy(P.M.m, a->matrix, sizeof(P.M.m));
    memcpy(P.on, a->on, sizeof(P.on));
    const dim3 grid(aug_blocks(P.nvox), (unsigned)a->samples);
    if (a->wide) hipLaunchKernelGGL(aug_labels_kernel<int64_t>, grid, dim3(kBlock), 0, (hipStream_t)a->stream, P);
    else hipLaunchKernelGGL(aug_labels_kernel<int16_t>, grid, dim3(kBlock), 0, (hipStream_t)a->stream, P);
    return (int)hipGetLastError();
}

extern "C" int segm_zoom_nearest(const segm_zoom_nearest_args* a) {
    if (!a) return SEGM_E_NULL;
    if (!a->data || !a->out) return SEGM_E_NULL;
    if (a->channels < 1 || a->channels > kAugMaxC) return SEGM_E_SHAPE;
    if (!aug_shape_ok(a->depth, a->height, a->width) || !aug_shape_ok(a->out_depth, a->out_height, a->out_width)) return SEGM_E_SHAPE;
    if (!aug_strides_ok(0, a->stride_c, a->stride_z, a->stride_y, a->width)) return SEGM_E_SHAPE;
    if ((uintptr_t)a->data % sizeof(float) || (uintptr_t)a->out % sizeof(float)) return SEGM_E_SHAPE;
    AugNearestDev P;
    memset(&P, 0, sizeof(P));
    P.data = a->data; P.out = a->out;
    P.sc = a->stride_c; P.sz = a->stride_z; P.sy = a->stride_y;
    P.D = a->depth; P.H = a->height; P.W = a->width; P.d = a->out_depth; P.h = a->out_height; P.w = a->out_width;
    P.nout = (int64_t)P.d * P.h * P.w;
    P.rz = (double)P.D / (double)P.d; P.ry = (double)P.H / (double)P.h; P.rx = (double)P.W / (double)P.w;
    hipLaunchKernelGGL(aug_nearest_kernel, dim3(aug_blocks(P.nout), (unsigned)a->channels), dim3(kBlock), 0, (hipStream_t)a->stream, P);
    return (int)hipGetLastError();
}

extern "C" int segm_gauss_blur(const segm_gauss_blur_args* a) {
    if (!a) return SEGM_E_NULL;
    if (!a->data || !a->out) return SEGM_E_NULL;
    if (!aug_batch_ok(a->samples, a->channels, a->depth, a->height, a->width)) return SEGM_E_SHAPE;
    if (!aug_strides_ok(a->stride_n, a->stride_c, a->stride_z, a->stride_y, a->width)) return SEGM_E_SHAPE;
    if ((uintptr_t)a->data % sizeof(float) || (uintptr_t)a->out % sizeof(float) || (uintptr_t)a->workspace % sizeof(float)) return SEGM_E_SHAPE;
    const int C = a->channels, D = a->depth, H = a->height, W = a->width, V = a->samples * C;
    AugBlurDev P;
    memset(&P, 0, sizeof(P));
    bool any = false;
    for (int v = 0; v < V; ++v) {
        if (!a->on[v]) continue;
        const double sigma = a->sigma[v];
        if (!(sigma > 0.0) || !(4.0 * sigma + 0.5 < (double)(kBlurMaxR + 1))) return SEGM_E_SHAPE;
        const int r = (int)(4.0 * sigma + 0.5);
        double sum = 1.0;                             // scipy's _gaussian_kernel1d: exp(-0.5 / sigma^2 * t^2), normalised
        P.w[v][0] = 1.0;
        for (int k = 1; k <= r; ++k) {
            P.w[v][k] = exp(-0.5 / (sigma * sigma) * (double)(k * k));
            sum += 2.0 * P.w[v][k];
        }
        for (int k = 0; k <= r; ++k) P.w[v][k] /= sum;
        P.radius[v] = (int8_t)r;
        P.on[v] = 1;
        any = true;
    }
    const int64_t nvox = (int64_t)D * H * W;
    if (any && (!a->workspace || a->workspace_bytes < (size_t)V * (size_t)nvox * sizeof(float))) return SEGM_E_WORKSPACE;
    hipStream_t st = (hipStream_t)a->stream;
    const dim3 grid(aug_blocks(nvox), (unsigned)V);
    P.C = C; P.D = D; P.H = H; P.W = W; P.nvox = nvox;
    P.in = a->data; P.out = a->out;                   // z: data -> out, the volumes that are off copied
    P.sn = a->stride_n; P.sc = a->stride_c; P.sz = a->stride_z; P.sy = a->stride_y;
    P.axis = 0; P.copy_off = 1;
    hipLaunchKernelGGL(aug_blur_kernel, grid, dim3(kBlock), 0, st, P);
    if (any) {
        P.sy = W; P.sz = (int64_t)H * W; P.sc = nvox; P.sn = (int64_t)C * nvox;
        P.copy_off = 0;
        P.in = a->out; P.out = (float*)a->workspace; P.axis = 1;   // y: out -> workspace
        hipLaunchKernelGGL(aug_blur_kernel, grid, dim3(kBlock), 0, st, P);
        P.in = (const float*)a->workspace; P.out = a->out; P.axis = 2;   // x: workspace -> out
        hipLaunchKernelGGL(aug_blur_kernel, grid, dim3(kBlock), 0, st, P);
    }
    return (int)hipGetLastError();
}
