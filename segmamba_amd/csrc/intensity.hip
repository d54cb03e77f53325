// Intensity augmentation as streaming passes (C ABI: segm_intensity_workspace_bytes, segm_intensity_stats, segm_intensity_apply).
//
// Replaces the per-sample ATen arithmetic of SplineAugmenter (segmamba_amd/augment.py:333-363) - GaussianNoise,
// BrightnessMultiplicative, ContrastAugmentation, the two Gamma transforms and Mirror of the reference's get_train_transforms
// (light_training/augment/train_augment.py:40-60).  A plane is one (sample, channel) of a (samples, channels, D, H, W) fp32 tensor
// with a unit stride along x; a launch takes up to 64 planes, each with its own op and parameters in the kernel arguments.
//
//   * in_stats_kernel    a workgroup owns a stretch of `chunk` voxels of one plane.  stage 0 takes u = fl32(v m) of a CONTRAST plane
//                        and t = +-v of a GAMMA plane, stage 1 takes w of a GAMMA plane, formed from the stage-0 row by in_gamma_w,
//                        the function the apply pass uses.  The sums are those of (x - K) and (x - K)^2 in fp64, K the plane's first
//                        value, so a plane with a mean far from zero keeps its digits; min and max are exact.  Every term is added
//                        in the thread, then over the wave by shuffles, then over the four waves through LDS; the workgroup writes
//                        one row of 5 doubles (the two sums, min, max, K).
//   * in_finish_kernel   one workgroup per plane adds the rows in a fixed order (wave w takes slot w, lane l the rows l, l + 64, ...,
//                        then a shuffle tree) and writes count, mean, population sd, min, max.  No floating-point atomic: two calls
//                        are bit-equal.
//   * in_apply_kernel    one packet of 16 bytes (4 voxels along x) per thread where width, strides and base pointers allow it, one
//                        voxel otherwise; both routes call the same per-voxel functions.  The plane's statistics come from the rows
//                        in device memory.  In place, or out of place to the mirrored position: an x-mirror reverses the packet and
//                        stores it at the mirrored packet address.
// The apply pass does not reduce the statistics of what it writes: an inverted gamma followed by a plain gamma on the same plane
// reads the plane once more than it would have to.
#include <math.h>
#include <string.h>

#include "loss_common.h"

namespace segm {

constexpr int kInMaxP = SEGM_AUG_MAX_VOLUMES;
constexpr int kInQuantum = kBlock * 4;               // a chunk is a multiple of this: whole packets for every thread
constexpr int kInMaxChunks = 512;                    // per plane; 128^3 voxels -> 512 chunks of 4096
constexpr int kInPart = 5;                           // doubles of a partial row: sum (x - K), sum (x - K)^2, min, max, K
constexpr int kInRow = SEGM_INTENSITY_STATS_DOUBLES; // count, mean, sd, min, max, 0, 0, 0

struct InDev {
    const float* data;
    float* out;
    const float* noise[kInMaxP];
    double* part;                                    // [plane][nchunks][kInPart]
    const double* stats;
    const double* stats2;
    double* rows;                                    // what the finish kernel writes
    int64_t sn, sc, sz, sy;
    int64_t on, oc, oz, oy;
    int32_t C, D, H, W, V;
    int32_t chunk, nchunks, stage, dense;
    float a[kInMaxP], b[kInMaxP];
    uint8_t op[kInMaxP], invert[kInMaxP], mirror[kInMaxP];
};

// ---- the per-voxel arithmetic: one function each for every route ------------------------------------------------------------------------
__device__ __forceinline__ float in_prescale(float v, float m) {
    float u = v * m;
    RL_ROUND(u);                                     // rounded on its own: never fused into the difference that follows
    return u;
}

__device__ __forceinline__ float in_noise(float v, float n, float s) {
    float p = s * n;
    RL_ROUND(p);
    return v + p;
}

__device__ __forceinline__ float in_contrast(float u, float mean, float f, float lo, float hi) {
    return fminf(fmaxf((u - mean) * f + mean, lo), hi);
}

// the plane's constants for GAMMA, from its statistics rows
struct InGamma {
    float lo, rng, den, g;                           // den = rng + 1e-7
    float mean0, mean1, k;                           // k = sd0 / (sd1 + 1e-8)
};

__device__ __forceinline__ InGamma in_gamma_consts(const double* row0, const double* row1, float g) {
    InGamma q;
    q.lo = (float)row0[3];
    q.rng = (float)row0[4] - q.lo;
    q.den = q.rng + 1e-7f;
    q.g = g;
    q.mean0 = (float)row0[1];
    q.mean1 = row1 ? (float)row1[1] : 0.f;
    q.k = row1 ? (float)(row0[2] / (row1[2] + 1e-8)) : 0.f;
    return q;
}

// w of one voxel: the second statistics pass and the apply pass both call this, so mean1 is the mean of the w that is applied
__device__ __forceinline__ float in_gamma_w(float t, const InGamma& q) {
    const float r = fmaxf((t - q.lo) / q.den, 0.f);
    float w = __builtin_fmaf(powf(r, q.g), q.rng, q.lo);
    RL_ROUND(w);
    return w;
}

__device__ __forceinline__ float in_gamma(float v, bool invert, const InGamma& q) {
    const float w = in_gamma_w(invert ? -v : v, q);
    const float y = (w - q.mean1) * q.k + q.mean0;
    return invert ? -y : y;
}

// ---- addresses ----------------------------------------------------------------------------------------------------------------------------
// voxel i of a plane (C order over z, y, x) -> (z, y, x)
__device__ __forceinline__ void in_zyx(const InDev& P, int64_t i, int& z, int& y, int& x) {
    const uint32_t row = (uint32_t)i / (uint32_t)P.W;
    x = (int)((uint32_t)i - row * (uint32_t)P.W);
    z = (int)(row / (uint32_t)P.H);
    y = (int)(row - (uint32_t)z * (uint32_t)P.H);
}

__device__ __forceinline__ float in_wave_min(float v) {
    for (int off = kWave / 2; off >= 1; off >>= 1) v = fminf(v, __shfl_xor(v, off));
    return v;
}

__device__ __forceinline__ float in_wave_max(float v) {
    for (int off = kWave / 2; off >= 1; off >>= 1) v = fmaxf(v, __shfl_xor(v, off));
    return v;
}

// whether plane v takes part in a statistics launch
__device__ __forceinline__ bool in_takes_part(const InDev& P, int v) {
    const int op = P.op[v];
    return op == SEGM_INTENSITY_GAMMA || (P.stage == 0 && op == SEGM_INTENSITY_CONTRAST);
}

// ---- statistics ---------------------------------------------------------------------------------------------------------------------------
// the value whose statistics a launch takes: u (CONTRAST), t (GAMMA, stage 0) or w (GAMMA, stage 1)
__device__ __forceinline__ float in_stat_value(float v, int op, int stage, float m, bool invert, const InGamma& q) {
    if (op == SEGM_INTENSITY_CONTRAST) return in_prescale(v, m);
    const float t = invert ? -v : v;
    return stage == 0 ? t : in_gamma_w(t, q);
}

template <bool VEC>
__global__ void __launch_bounds__(kBlock) in_stats_kernel(InDev P) {
    constexpr int N = VEC ? 4 : 1;
    __shared__ double s_part[kWavesPerBlock][4];
    const int v = blockIdx.y;
    if (!in_takes_part(P, v)) return;                 // uniform over the workgroup
    const int op = P.op[v], stage = P.stage;
    const int b = v / P.C, c = v - b * P.C;
    const float* src = P.data + (int64_t)b * P.sn + (int64_t)c * P.sc;
    const float m = P.a[v];
    const bool invert = P.invert[v] != 0;
    InGamma q;
    memset(&q, 0, sizeof(q));
    if (stage == 1) q = in_gamma_consts(P.stats + (int64_t)v * kInRow, nullptr, P.a[v]);
    const float K = in_stat_value(src[0], op, stage, m, invert, q);
    const double Kd = (double)K;
    double s1 = 0.0, s2 = 0.0;
    float mn = K, mx = K;
    const int64_t lo = (int64_t)blockIdx.x * P.chunk;
    for (int32_t j = (int32_t)threadIdx.x * N; j < P.chunk; j += kBlock * N) {
        const int64_t i = lo + j;                     // VEC: V % N == 0, a packet is whole or absent
        if (i >= P.V) break;
        int64_t off = i;
        if (!P.dense) {
            int z, y, x;
            in_zyx(P, i, z, y, x);
            off = (int64_t)z * P.sz + (int64_t)y * P.sy + x;
        }
        Pack<float, VEC> p;
        p.load(src + off);
#pragma unroll
        for (int k = 0; k < N; ++k) {
            const float val = in_stat_value(p.v[k], op, stage, m, invert, q);
            const double d = (double)val - Kd;
            s1 += d;
            s2 += d * d;
            mn = fminf(mn, val);
            mx = fmaxf(mx, val);
        }
    }
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    s1 = rl_wave_sum(s1);
    s2 = rl_wave_sum(s2);
    mn = in_wave_min(mn);
    mx = in_wave_max(mx);
    if (lane == 0) { s_part[wave][0] = s1; s_part[wave][1] = s2; s_part[wave][2] = (double)mn; s_part[wave][3] = (double)mx; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double t1 = s_part[0][0], t2 = s_part[0][1], tn = s_part[0][2], tx = s_part[0][3];
        for (int w = 1; w < kWavesPerBlock; ++w) {
            t1 += s_part[w][0];
            t2 += s_part[w][1];
            tn = fmin(tn, s_part[w][2]);
            tx = fmax(tx, s_part[w][3]);
        }
        double* row = P.part + ((int64_t)v * P.nchunks + blockIdx.x) * kInPart;
        row[0] = t1; row[1] = t2; row[2] = tn; row[3] = tx; row[4] = Kd;
    }
}

// one workgroup per plane: wave w takes slot w (the two sums, min, max); lane l the rows l, l + 64, ...; then a shuffle tree
__global__ void __launch_bounds__(kBlock) in_finish_kernel(InDev P) {
    __shared__ double s_red[kWavesPerBlock];
    const int v = blockIdx.x;
    if (!in_takes_part(P, v)) return;                 // uniform over the workgroup
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    const double* rows = P.part + (int64_t)v * P.nchunks * kInPart;
    double acc;
    if (wave < 2) {                                   // uniform over the wave
        acc = 0.0;
        for (int r = lane; r < P.nchunks; r += kWave) acc += rows[(int64_t)r * kInPart + wave];
        acc = rl_wave_sum(acc);
    } else {
        acc = rows[wave];                             // row 0 always exists
        for (int r = lane; r < P.nchunks; r += kWave) {
            const double e = rows[(int64_t)r * kInPart + wave];
            acc = wave == 2 ? fmin(acc, e) : fmax(acc, e);
        }
        for (int off = kWave / 2; off >= 1; off >>= 1) {
            const double e = __shfl_xor(acc, off);
            acc = wave == 2 ? fmin(acc, e) : fmax(acc, e);
        }
    }
    if (lane == 0) s_red[wave] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        const double n = (double)P.V, K = rows[4];
        const double m = s_red[0] / n, var = s_red[1] / n - m * m;
        double* out = P.rows + (int64_t)v * kInRow;
        out[0] = n;
        out[1] = K + m;
        out[2] = var > 0.0 ? sqrt(var) : 0.0;
        out[3] = s_red[2];
        out[4] = s_red[3];
        out[5] = 0.0; out[6] = 0.0; out[7] = 0.0;
    }
}

// ---- apply --------------------------------------------------------------------------------------------------------------------------------
template <bool VEC, bool OOP>
__global__ void __launch_bounds__(kBlock) in_apply_kernel(InDev P) {
    constexpr int N = VEC ? 4 : 1;
    const int v = blockIdx.y;
    const int op = P.op[v];
    if (!OOP && op == SEGM_INTENSITY_OFF) return;     // uniform over the workgroup
    const int64_t i = ((int64_t)blockIdx.x * kBlock + threadIdx.x) * N;     // VEC: V % N == 0, a packet is whole or absent
    if (i >= P.V) return;
    const int b = v / P.C, c = v - b * P.C;
    int z, y, x;
    in_zyx(P, i, z, y, x);
    const float* src = P.data + (int64_t)b * P.sn + (int64_t)c * P.sc + (int64_t)z * P.sz + (int64_t)y * P.sy + x;
    Pack<float, VEC> p;
    p.load(src);
    switch (op) {                                     // uniform over the workgroup
    case SEGM_INTENSITY_NOISE: {
        Pack<float, VEC> n;
        n.load(P.noise[v] + i);
        const float s = P.a[v];
#pragma unroll
        for (int k = 0; k < N; ++k) p.v[k] = in_noise(p.v[k], n.v[k], s);
        break;
    }
    case SEGM_INTENSITY_SCALE: {
        const float m = P.a[v];
#pragma unroll
        for (int k = 0; k < N; ++k) p.v[k] = in_prescale(p.v[k], m);
        break;
    }
    case SEGM_INTENSITY_CONTRAST: {
        const double* row = P.stats + (int64_t)v * kInRow;
        const float m = P.a[v], f = P.b[v], mean = (float)row[1], lo = (float)row[3], hi = (float)row[4];
#pragma unroll
        for (int k = 0; k < N; ++k) p.v[k] = in_contrast(in_prescale(p.v[k], m), mean, f, lo, hi);
        break;
    }
    case SEGM_INTENSITY_GAMMA: {
        const InGamma q = in_gamma_consts(P.stats + (int64_t)v * kInRow, P.stats2 + (int64_t)v * kInRow, P.a[v]);
        const bool invert = P.invert[v] != 0;
#pragma unroll
        for (int k = 0; k < N; ++k) p.v[k] = in_gamma(p.v[k], invert, q);
        break;
    }
    default: break;
    }
    if (OOP) {
        const int mir = P.mirror[v];
        const int zo = (mir & 1) ? P.D - 1 - z : z, yo = (mir & 2) ? P.H - 1 - y : y, xo = (mir & 4) ? P.W - N - x : x;
        if (VEC && (mir & 4)) {
            const float t0 = p.v[0], t1 = p.v[N > 1 ? 1 : 0];
            p.v[0] = p.v[N - 1]; p.v[N - 1] = t0;
            if (N > 1) { p.v[1] = p.v[N - 2]; p.v[N - 2] = t1; }
        }
        p.store(P.out + (int64_t)b * P.on + (int64_t)c * P.oc + (int64_t)zo * P.oz + (int64_t)yo * P.oy + xo);
    } else {
        p.store(const_cast<float*>(src));
    }
}

// ---- host ---------------------------------------------------------------------------------------------------------------------------------
static int32_t in_chunk(int64_t voxels) {
    const int64_t per = (voxels + kInMaxChunks - 1) / kInMaxChunks;
    const int64_t chunk = ((per + kInQuantum - 1) / kInQuantum) * kInQuantum;
    return (int32_t)(chunk < kInQuantum ? kInQuantum : chunk);
}

static inline bool in_mult4(int64_t stride, int32_t size) { return size == 1 || stride % 4 == 0; }

// the checks the two entries share; 0 or a SEGM_E_* status.  `vec`: the data allow packets.
static int in_setup(const segm_intensity_args* a, InDev& P, bool& vec) {
    if (!a) return SEGM_E_NULL;
    if (a->samples < 1 || a->channels < 1 || (int64_t)a->samples * a->channels > kInMaxP) return SEGM_E_SHAPE;
    if (a->depth < 1 || a->height < 1 || a->width < 1) return SEGM_E_SHAPE;
    const int64_t voxels = (int64_t)a->depth * a->height * a->width;
    if (voxels >= ((int64_t)1 << 31)) return SEGM_E_SHAPE;
    if (a->stride_x != 1 || a->stride_n < 0 || a->stride_c < 0 || a->stride_z < 0 || a->stride_y < a->width) return SEGM_E_SHAPE;
    const int planes = a->samples * a->channels;
    for (int v = 0; v < planes; ++v)
        if (a->op[v] > SEGM_INTENSITY_GAMMA) return SEGM_E_DTYPE;
    if (!a->data) return SEGM_E_NULL;
    if ((uintptr_t)a->data % sizeof(float)) return SEGM_E_SHAPE;
    memset(&P, 0, sizeof(P));
    P.data = a->data;
    P.sn = a->stride_n; P.sc = a->stride_c; P.sz = a->stride_z; P.sy = a->stride_y;
    P.C = a->channels; P.D = a->depth; P.H = a->height; P.W = a->width; P.V = (int32_t)voxels;
    P.dense = (a->height == 1 || a->stride_y == a->width) && (a->depth == 1 || a->stride_z == (int64_t)a->width * a->height);
    memcpy(P.op, a->op, (size_t)planes);
    memcpy(P.invert, a->invert, (size_t)planes);
    memcpy(P.a, a->a, (size_t)planes * sizeof(float));
    memcpy(P.b, a->b, (size_t)planes * sizeof(float));
    // packets: every row starts at a multiple of 16 bytes (the strides of axes of size 1 are never used)
    vec = a->width % 4 == 0 && in_mult4(a->stride_n, a->samples) && in_mult4(a->stride_c, a->channels) &&
          in_mult4(a->stride_z, a->depth) && in_mult4(a->stride_y, a->height) && (uintptr_t)a->data % 16 == 0;
    return SEGM_OK;
}

}  // namespace segm

using namespace segm;

extern "C" size_t segm_intensity_workspace_bytes(int32_t planes, int64_t voxels) {
    if (planes < 1 || planes > kInMaxP || voxels < 1 || voxels >= ((int64_t)1 << 31)) return 0;
    const int32_t chunk = in_chunk(voxels);
    const int64_t nchunks = (voxels + chunk - 1) / chunk;
    return (size_t)planes * (size_t)nchunks * kInPart * sizeof(double);
}

extern "C" int segm_intensity_stats(const segm_intensity_args* a) {
    InDev P;
    bool vec = false;
    const int rc = in_setup(a, P, vec);
    if (rc != SEGM_OK) return rc;
    if (a->stage != 0 && a->stage != 1) return SEGM_E_SHAPE;
    const int planes = a->samples * a->channels;
    P.stage = a->stage;
    bool any = false;
    for (int v = 0; v < planes; ++v) any = any || a->op[v] == SEGM_INTENSITY_GAMMA || (a->stage == 0 && a->op[v] == SEGM_INTENSITY_CONTRAST);
    if (!any) return SEGM_OK;
    if (!a->stats || (a->stage == 1 && !a->stats2)) return SEGM_E_NULL;
    if ((uintptr_t)a->stats % sizeof(double) || (uintptr_t)a->stats2 % sizeof(double)) return SEGM_E_SHAPE;
    const size_t need = segm_intensity_workspace_bytes(planes, P.V);
    if (!a->workspace || a->workspace_bytes < need || (uintptr_t)a->workspace % sizeof(double)) return SEGM_E_WORKSPACE;
    P.part = (double*)a->workspace;
    P.stats = a->stats;
    P.rows = a->stage == 0 ? a->stats : a->stats2;
    P.chunk = in_chunk(P.V);
    P.nchunks = (int32_t)(((int64_t)P.V + P.chunk - 1) / P.chunk);
    hipStream_t st = (hipStream_t)a->stream;
    const dim3 grid((unsigned)P.nchunks, (unsigned)planes);
    if (vec) hipLaunchKernelGGL((in_stats_kernel<true>), grid, dim3(kBlock), 0, st, P);
    else hipLaunchKernelGGL((in_stats_kernel<false>), grid, dim3(kBlock), 0, st, P);
    hipLaunchKernelGGL(in_finish_kernel, dim3((unsigned)planes), dim3(kBlock), 0, st, P);
    return (int)hipGetLastError();
}

extern "C" int segm_intensity_apply(const segm_intensity_args* a) {
    InDev P;
    bool vec = false;
    const int rc = in_setup(a, P, vec);
    if (rc != SEGM_OK) return rc;
    const int planes = a->samples * a->channels;
    const bool oop = a->out != nullptr && a->out != a->data;
    bool any = false;
    for (int v = 0; v < planes; ++v) {
        const int op = a->op[v];
        any = any || op != SEGM_INTENSITY_OFF;
        if (!oop && a->mirror[v]) return SEGM_E_SHAPE;
        if (a->mirror[v] > 7) return SEGM_E_SHAPE;
        if (op == SEGM_INTENSITY_NOISE) {
            if (!a->noise[v]) return SEGM_E_NULL;
            if ((uintptr_t)a->noise[v] % sizeof(float)) return SEGM_E_SHAPE;
            vec = vec && (uintptr_t)a->noise[v] % 16 == 0;
            P.noise[v] = a->noise[v];
        }
        if ((op == SEGM_INTENSITY_CONTRAST || op == SEGM_INTENSITY_GAMMA) && !a->stats) return SEGM_E_NULL;
        if (op == SEGM_INTENSITY_GAMMA && !a->stats2) return SEGM_E_NULL;
    }
    if ((uintptr_t)a->stats % sizeof(double) || (uintptr_t)a->stats2 % sizeof(double)) return SEGM_E_SHAPE;
    if (oop) {
        if ((uintptr_t)a->out % sizeof(float)) return SEGM_E_SHAPE;
        if (a->out_stride_n < 0 || a->out_stride_c < 0 || a->out_stride_z < 0 || a->out_stride_y < a->width) return SEGM_E_SHAPE;
        vec = vec && in_mult4(a->out_stride_n, a->samples) && in_mult4(a->out_stride_c, a->channels) &&
              in_mult4(a->out_stride_z, a->depth) && in_mult4(a->out_stride_y, a->height) && (uintptr_t)a->out % 16 == 0;
        P.out = a->out;
        P.on = a->out_stride_n; P.oc = a->out_stride_c; P.oz = a->out_stride_z; P.oy = a->out_stride_y;
        memcpy(P.mirror, a->mirror, (size_t)planes);
    } else if (!any) {
        return SEGM_OK;
    }
    P.stats = a->stats;
    P.stats2 = a->stats2;
    const int64_t packets = ((int64_t)P.V + (vec ? 4 : 1) - 1) / (vec ? 4 : 1);
    const dim3 grid((unsigned)((packets + kBlock - 1) / kBlock), (unsigned)planes);
    hipStream_t st = (hipStream_t)a->stream;
    if (vec && oop) hipLaunchKernelGGL((in_apply_kernel<true, true>), grid, dim3(kBlock), 0, st, P);
    else if (vec) hipLaunchKernelGGL((in_apply_kernel<true, false>), grid, dim3(kBlock), 0, st, P);
    else if (oop) hipLaunchKernelGGL((in_apply_kernel<false, true>), grid, dim3(kBlock), 0, st, P);
    else hipLaunchKernelGGL((in_apply_kernel<false, false>), grid, dim3(kBlock), 0, st, P);
    return (int)hipGetLastError();
}
