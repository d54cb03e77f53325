// Preparing a case on the device: non-zero mask and bounding box, crop statistics, crop + z-score + seg relabelling
// (C ABI: segm_nonzero_mask_bbox, segm_crop_stats, segm_crop_normalize, segm_crop_clip_normalize).
//
// Replaces what the reference's `MultiModalityPreprocessor.run_case_npy` does on the host with numpy / scipy
// (light_training/preprocessing/preprocessors/default_preprocessor.py:154-227): `create_nonzero_mask` and `get_bbox_from_mask`
// (cropping/cropping.py:8-33), the crop and the `seg[(seg == 0) & ~mask] = -1` rule (:35-48), `ZScoreNormalization.run`
// (normalization/default_normalization_schemes.py:31-50) and the `np.max(seg)` / `np.argwhere` counts behind the seg's dtype and
// the class locations (default_preprocessor.py:203-210).  Hole filling between the first and the second step is csrc/postprocess.hip.
//
// All of it is byte work; a thread owns four consecutive voxels of a row, at x = 0 mod 4 of the UN-cropped volume, so that the
// reads of data, seg and mask are one 16 / 8 / 4-byte packet each wherever the layout allows (the crop's x0 is arbitrary: the dense
// outputs are written as dwords, contiguous over the lanes of a wave).
//   * nonzero_mask_bbox_kernel  OR over the channels of `bits(x) & 0x7fffffff` (non-zero as `!=` has it: NaN counts, -0 does not),
//                               the mask as one dword per thread, min / max of z, y, x by wave shuffles, LDS, and then at most
//                               six integer atomics per workgroup - none from a workgroup that saw only zeros.
//   * crop_stats_*              per channel, over the box or over the box's voxels whose relabelled seg is >= 0: pass 0 sums x and
//                               counts, pass 1 sums (x - mean)^2; fp64 throughout.  Every workgroup writes its partial to its own
//                               slot, one workgroup adds the slots in a fixed order: no floating-point atomics, two calls are bit-equal.
//   * crop_normalize_kernel     (x - mean) / max(std, 1e-8) in fp32 into the dense crop, the relabelled seg as int16, and the label
//                               counts: -1 and 0 (nearly every voxel) are counted in registers, the rest in an LDS histogram, the
//                               workgroup's non-zero bins go out by 64-bit integer atomic add (exact, order-free).  With the CLIP
//                               flag x is first bounded per channel: CTNormalization.run (default_normalization_schemes.py:83-95).
// Vector-memory and LDS atomics only.  The CPU emulation build (SEGM_EMU) states the same atomics with the compiler's __atomic builtins.
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include "segm_device.h"

namespace segm {

#ifdef SEGM_EMU
static inline void prep_min(int32_t* p, int32_t v) { __atomic_fetch_min(p, v, __ATOMIC_RELAXED); }
static inline void prep_max(int32_t* p, int32_t v) { __atomic_fetch_max(p, v, __ATOMIC_RELAXED); }
static inline void prep_add_lds(int32_t* p, int32_t v) { __atomic_fetch_add(p, v, __ATOMIC_RELAXED); }
static inline void prep_add64(long long* p, long long v) { __atomic_fetch_add(p, v, __ATOMIC_RELAXED); }
#else
__device__ __forceinline__ void prep_min(int32_t* p, int32_t v) { __hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void prep_max(int32_t* p, int32_t v) { __hip_atomic_fetch_max(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void prep_add_lds(int32_t* p, int32_t v) { __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ __forceinline__ void prep_add64(long long* p, long long v) { __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
#endif

constexpr int kPrepItems = 4;                       // four-voxel packets per thread of the box kernels
constexpr int kPrepChunk = kBlock * kPrepItems;
constexpr int kPrepMaxC = SEGM_PREP_MAX_CHANNELS;
constexpr int kBinMinus = 256, kBinAbove = 257, kBinInvalid = 258;

typedef uint32_t prep_raw4 __attribute__((ext_vector_type(4)));

// ---- mask and bounding box ----------------------------------------------------------------------------------------------------------
struct MaskDev {
    const float* data;
    uint8_t* mask;
    int32_t* bbox;
    int64_t sc, sz, sy;
    int32_t C, D, H, W;
    int32_t cpr;                        // four-voxel packets per row
    int32_t vec, pack;                  // the data take 16-byte loads; the mask takes dword stores
    uint32_t nthreads;
};

__global__ void __launch_bounds__(kBlock) nonzero_mask_bbox_kernel(MaskDev P) {
    __shared__ int32_t s_box[kWavesPerBlock][6];
    const uint32_t gid = (uint32_t)blockIdx.x * kBlock + threadIdx.x;
    int32_t lo[3] = {INT32_MAX, INT32_MAX, INT32_MAX}, hi[3] = {0, 0, 0};       // hi = the largest index + 1
    if (gid < P.nthreads) {
        const uint32_t row = gid / (uint32_t)P.cpr, chunk = gid - row * (uint32_t)P.cpr;
        const int z = (int)(row / (uint32_t)P.H), y = (int)(row - (uint32_t)z * (uint32_t)P.H), x = (int)chunk * 4;
        const float* p = P.data + (int64_t)z * P.sz + (int64_t)y * P.sy + x;
        uint32_t bits[4] = {0u, 0u, 0u, 0u};
        if (P.vec && x + 3 < P.W) {
            for (int c = 0; c < P.C; ++c) {
                const prep_raw4 q = *reinterpret_cast<const prep_raw4*>(p + (int64_t)c * P.sc);
#pragma unroll
                for (int k = 0; k < 4; ++k) bits[k] |= q[k] & 0x7fffffffu;
            }
        } else {
            for (int c = 0; c < P.C; ++c)
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (x + k < P.W) bits[k] |= __float_as_uint(p[(int64_t)c * P.sc + k]) & 0x7fffffffu;
        }
        const int64_t o = (int64_t)row * P.W + x;
        if (P.pack) {                                 // W % 4 == 0: the packet lies inside the row and on a dword
            *reinterpret_cast<uint32_t*>(P.mask + o) = (bits[0] ? 1u : 0u) | (bits[1] ? 1u << 8 : 0u) | (bits[2] ? 1u << 16 : 0u) |
                                                       (bits[3] ? 1u << 24 : 0u);
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (x + k < P.W) P.mask[o + k] = bits[k] ? 1 : 0;
        }
        int first = -1, last = -1;
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (bits[k]) { first = first < 0 ? k : first; last = k; }
        if (first >= 0) {
            lo[0] = z; lo[1] = y; lo[2] = x + first;
            hi[0] = z + 1; hi[1] = y + 1; hi[2] = x + last + 1;
        }
    }
    for (int off = kWave / 2; off >= 1; off >>= 1) {
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const int32_t a = __shfl_xor(lo[i], off), b = __shfl_xor(hi[i], off);
            lo[i] = a < lo[i] ? a : lo[i];
            hi[i] = b > hi[i] ? b : hi[i];
        }
    }
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < 3; ++i) { s_box[wave][i] = lo[i]; s_box[wave][3 + i] = hi[i]; }
    }
    __syncthreads();
    if (threadIdx.x < 6) {
        const int i = threadIdx.x;
        int32_t v = s_box[0][i];
        for (int w = 1; w < kWavesPerBlock; ++w) {
            const int32_t u = s_box[w][i];
            v = i < 3 ? (u < v ? u : v) : (u > v ? u : v);
        }
        if (i < 3) { if (v != INT32_MAX) prep_min(P.bbox + i, v); }
        else if (v > 0) prep_max(P.bbox + i, v);
    }
}

// ---- the box kernels ----------------------------------------------------------------------------------------------------------------
struct CropDev {
    const float* data;
    const uint8_t* mask;
    const void* seg;
    double* stats64;                    // [0..7] mean, [8..15] std, [16] the number of voxels the statistics are over
    float* stats32;                     // [0..7] mean, [8..15] std
    float* out;
    int16_t* seg_out;
    long long* counts;
    double* part;                       // [channel or C = count][workgroup]
    int64_t sc, sz, sy;
    int32_t C, D, H, W;
    int32_t z0, y0, x0, d, h, w;        // the box
    int32_t xa0, cpr;                   // x0 rounded down to a multiple of 4; packets per box row
    int32_t seg_dtype, masked, nonzero_label, labels;
    int32_t vec, mvec, svec;            // data / mask / seg take one packet per four voxels
    int32_t nblocks, pass;
    uint32_t nitems;
};

struct BoxItem { int zz, yy, xa; int64_t lin; bool in[4]; };

__device__ __forceinline__ BoxItem box_item(const CropDev& P, uint32_t i) {
    BoxItem it;
    const uint32_t row = i / (uint32_t)P.cpr, k = i - row * (uint32_t)P.cpr;
    it.zz = (int)(row / (uint32_t)P.h);
    it.yy = (int)(row - (uint32_t)it.zz * (uint32_t)P.h);
    it.xa = P.xa0 + 4 * (int)k;
    it.lin = ((int64_t)(P.z0 + it.zz) * P.H + (P.y0 + it.yy)) * P.W + it.xa;
#pragma unroll
    for (int j = 0; j < 4; ++j) it.in[j] = it.xa + j >= P.x0 && it.xa + j < P.x0 + P.w;
    return it;
}

__device__ __forceinline__ void load_data4(const CropDev& P, const BoxItem& it, int c, float v[4]) {
    const float* p = P.data + (int64_t)c * P.sc + (int64_t)(P.z0 + it.zz) * P.sz + (int64_t)(P.y0 + it.yy) * P.sy + it.xa;
    if (P.vec && it.xa + 3 < P.W) {
        const prep_raw4 q = *reinterpret_cast<const prep_raw4*>(p);
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = __uint_as_float(q[j]);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = it.in[j] ? p[j] : 0.f;
    }
}

template <typename T> struct alignas(4 * sizeof(T)) PrepQuad { T e[4]; };

template <typename T> __device__ __forceinline__ void load_quad(const T* p, bool vec, const bool in[4], T v[4]) {
    if (vec) {
        const PrepQuad<T> q = *reinterpret_cast<const PrepQuad<T>*>(p);
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = q.e[j];
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = in[j] ? p[j] : (T)0;
    }
}

// the labels of the packet's voxels after `seg[(seg == 0) & ~mask] = nonzero_label` (without a seg: 0 inside the mask,
// nonzero_label outside); bad[j]: the seg's value is no integer in [-1, 32767] (the label is then 0)
__device__ __forceinline__ void load_labels(const CropDev& P, const BoxItem& it, int32_t lab[4], bool bad[4]) {
    uint8_t m[4];
    load_quad<uint8_t>(P.mask + it.lin, P.mvec && it.xa + 3 < P.W, it.in, m);
#pragma unroll
    for (int j = 0; j < 4; ++j) { lab[j] = 0; bad[j] = false; }
    if (P.seg_dtype == SEGM_PREP_SEG_F32) {
        float s[4];
        load_quad<float>(reinterpret_cast<const float*>(P.seg) + it.lin, P.svec && it.xa + 3 < P.W, it.in, s);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const bool ok = s[j] >= -1.f && s[j] <= 32767.f && s[j] == floorf(s[j]);      // NaN fails the first
            lab[j] = ok ? (int32_t)s[j] : 0;
            bad[j] = it.in[j] && !ok;
        }
    } else if (P.seg_dtype == SEGM_PREP_SEG_U8) {
        uint8_t s[4];
        load_quad<uint8_t>(reinterpret_cast<const uint8_t*>(P.seg) + it.lin, P.svec && it.xa + 3 < P.W, it.in, s);
#pragma unroll
        for (int j = 0; j < 4; ++j) lab[j] = s[j];
    } else if (P.seg_dtype == SEGM_PREP_SEG_I16) {
        int16_t s[4];
        load_quad<int16_t>(reinterpret_cast<const int16_t*>(P.seg) + it.lin, P.svec && it.xa + 3 < P.W, it.in, s);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const bool ok = s[j] >= -1;
            lab[j] = ok ? s[j] : 0;
            bad[j] = it.in[j] && !ok;
        }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (lab[j] == 0 && !bad[j] && m[j] == 0) lab[j] = P.nonzero_label;
}

template <typename T> __device__ __forceinline__ T wave_sum(T v) {
    for (int off = kWave / 2; off >= 1; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// pass 0: part[c][b] = the workgroup's sum of x, part[C][b] = its voxel count; pass 1: part[c][b] = its sum of (x - mean[c])^2
__global__ void __launch_bounds__(kBlock) crop_stats_partial_kernel(CropDev P) {
    __shared__ double s_sum[kWavesPerBlock][kPrepMaxC + 1];
    double acc[kPrepMaxC + 1];
    double mean[kPrepMaxC];
#pragma unroll
    for (int c = 0; c <= kPrepMaxC; ++c) acc[c] = 0.0;
#pragma unroll
    for (int c = 0; c < kPrepMaxC; ++c) mean[c] = (P.pass == 1 && c < P.C) ? P.stats64[c] : 0.0;
    for (int t = 0; t < kPrepItems; ++t) {
        const int64_t i = (int64_t)blockIdx.x * kPrepChunk + (int64_t)t * kBlock + threadIdx.x;
        if (i >= (int64_t)P.nitems) break;
        BoxItem it = box_item(P, (uint32_t)i);
        if (P.masked) {
            int32_t lab[4];
            bool bad[4];
            load_labels(P, it, lab, bad);
#pragma unroll
            for (int j = 0; j < 4; ++j) it.in[j] = it.in[j] && lab[j] >= 0;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[kPrepMaxC] += it.in[j] ? 1.0 : 0.0;
#pragma unroll
        for (int c = 0; c < kPrepMaxC; ++c) {
            if (c < P.C) {
                float v[4];
                load_data4(P, it, c, v);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const double dv = (double)v[j] - mean[c];
                    acc[c] += it.in[j] ? (P.pass == 1 ? dv * dv : dv) : 0.0;
                }
            }
        }
    }
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
#pragma unroll
    for (int c = 0; c <= kPrepMaxC; ++c) {
        const double s = wave_sum(acc[c]);
        if (lane == 0) s_sum[wave][c] = s;
    }
    __syncthreads();
    if (threadIdx.x <= (unsigned)kPrepMaxC) {
        const int c = threadIdx.x;
        double s = s_sum[0][c];
        for (int w = 1; w < kWavesPerBlock; ++w) s += s_sum[w][c];
        const int slot = c == kPrepMaxC ? P.C : c;
        if ((c < P.C || c == kPrepMaxC) && !(P.pass == 1 && c == kPrepMaxC)) P.part[(size_t)slot * P.nblocks + blockIdx.x] = s;
    }
}

// one workgroup: the partials of a channel are added by thread t in the order t, t + 256, ..., the 256 sums by a fixed tree
__global__ void __launch_bounds__(kBlock) crop_stats_final_kernel(CropDev P) {
    __shared__ double s_red[kBlock];
    const int nslots = P.pass == 0 ? P.C + 1 : P.C;
    for (int c = nslots - 1; c >= 0; --c) {           // pass 0: the count (slot C) first, the means need it
        double s = 0.0;
        for (int b = threadIdx.x; b < P.nblocks; b += kBlock) s += P.part[(size_t)c * P.nblocks + b];
        s_red[threadIdx.x] = s;
        __syncthreads();
        for (int off = kBlock / 2; off >= 1; off >>= 1) {
            if ((int)threadIdx.x < off) s_red[threadIdx.x] += s_red[threadIdx.x + off];
            __syncthreads();
        }
        if (threadIdx.x == 0) {
            const double total = s_red[0];
            if (P.pass == 0 && c == P.C) {
                P.stats64[16] = total;
            } else {
                const double n = P.stats64[16];
                if (P.pass == 0) {
                    const double m = n > 0.0 ? total / n : 0.0;
                    P.stats64[c] = m;
                    P.stats32[c] = (float)m;
                } else {
                    const double sd = n > 0.0 ? sqrt(total / n) : 0.0;
                    P.stats64[8 + c] = sd;
                    P.stats32[8 + c] = (float)sd;
                }
            }
        }
        __syncthreads();
    }
}

// CLIP: stats32[16..23] / [24..31] bound x from below / above before the subtraction (segm_crop_clip_normalize); the comparisons
// leave a NaN a NaN, as np.clip does.  Without CLIP the arithmetic is what it was before the flag existed.
template <bool CLIP> __global__ void __launch_bounds__(kBlock) crop_normalize_kernel(CropDev P) {
    __shared__ int32_t s_hist[SEGM_PREP_COUNT_BINS];
    __shared__ int32_t s_two[kWavesPerBlock][2];
    for (int b = threadIdx.x; b < SEGM_PREP_COUNT_BINS; b += kBlock) s_hist[b] = 0;
    __syncthreads();
    float mean[kPrepMaxC], sd[kPrepMaxC], lower[kPrepMaxC], upper[kPrepMaxC];
#pragma unroll
    for (int c = 0; c < kPrepMaxC; ++c) {
        mean[c] = c < P.C ? P.stats32[c] : 0.f;
        const float s = c < P.C ? P.stats32[8 + c] : 1.f;
        sd[c] = s > 1e-8f ? s : 1e-8f;
        lower[c] = (CLIP && c < P.C) ? P.stats32[16 + c] : 0.f;
        upper[c] = (CLIP && c < P.C) ? P.stats32[24 + c] : 0.f;
    }
    int32_t n_minus = 0, n_zero = 0;
    for (int t = 0; t < kPrepItems; ++t) {
        const int64_t i = (int64_t)blockIdx.x * kPrepChunk + (int64_t)t * kBlock + threadIdx.x;
        if (i >= (int64_t)P.nitems) break;
        const BoxItem it = box_item(P, (uint32_t)i);
        int32_t lab[4] = {0, 0, 0, 0};
        if (P.labels) {
            bool bad[4];
            load_labels(P, it, lab, bad);
            const int64_t so = ((int64_t)it.zz * P.h + it.yy) * P.w + (it.xa - P.x0);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (!it.in[j]) continue;
                if (P.seg_out) P.seg_out[so + j] = (int16_t)lab[j];
                if (!P.counts) continue;
                if (bad[j]) prep_add_lds(&s_hist[kBinInvalid], 1);
                else if (lab[j] < 0) ++n_minus;
                else if (lab[j] == 0) ++n_zero;
                else prep_add_lds(&s_hist[lab[j] > 255 ? kBinAbove : lab[j]], 1);
            }
        }
#pragma unroll
        for (int c = 0; c < kPrepMaxC; ++c) {
            if (c < P.C) {
                float v[4];
                load_data4(P, it, c, v);
                float* o = P.out + (((int64_t)c * P.d + it.zz) * P.h + it.yy) * P.w + (it.xa - P.x0);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if (!it.in[j]) continue;
                    if (CLIP) {
                        float x = v[j];
                        x = x < lower[c] ? lower[c] : x;
                        x = x > upper[c] ? upper[c] : x;
                        o[j] = (x - mean[c]) / sd[c];
                    } else {
                        o[j] = (P.masked && lab[j] < 0) ? v[j] : (v[j] - mean[c]) / sd[c];
                    }
                }
            }
        }
    }
    if (!P.counts) return;                            // uniform over the launch
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    const int32_t wm = wave_sum(n_minus), wz = wave_sum(n_zero);
    if (lane == 0) { s_two[wave][0] = wm; s_two[wave][1] = wz; }
    __syncthreads();
    if (threadIdx.x == 0) {
        int32_t a = 0, b = 0;
        for (int w = 0; w < kWavesPerBlock; ++w) { a += s_two[w][0]; b += s_two[w][1]; }
        s_hist[kBinMinus] = a;
        s_hist[0] = b;
    }
    __syncthreads();
    for (int b = threadIdx.x; b < SEGM_PREP_COUNT_BINS; b += kBlock) {
        const int32_t n = s_hist[b];
        if (n) prep_add64(P.counts + b, (long long)n);
    }
}

static inline int64_t prep_blocks(int64_t items) { return (items + kPrepChunk - 1) / kPrepChunk; }

// the checks both box entries share, and the geometry; 0 or a SEGM_E_* status
static int crop_setup(const segm_crop_args* a, CropDev& P) {
    if (!a) return SEGM_E_NULL;
    if (!a->data) return SEGM_E_NULL;
    if (a->channels < 1 || a->channels > SEGM_PREP_MAX_CHANNELS) return SEGM_E_SHAPE;
    if (a->depth <= 0 || a->height <= 0 || a->width <= 0) return SEGM_E_SHAPE;
    if ((int64_t)a->depth * a->height > SEGM_CCL_MAX_VOXELS || (int64_t)a->depth * a->height * a->width > SEGM_CCL_MAX_VOXELS) return SEGM_E_SHAPE;
    if (a->box_depth <= 0 || a->box_height <= 0 || a->box_width <= 0 || a->box_z < 0 || a->box_y < 0 || a->box_x < 0) return SEGM_E_SHAPE;
    if ((int64_t)a->box_z + a->box_depth > a->depth || (int64_t)a->box_y + a->box_height > a->height ||
        (int64_t)a->box_x + a->box_width > a->width) return SEGM_E_SHAPE;
    if (a->stride_y < a->width || a->stride_z < 0 || a->stride_c < 0) return SEGM_E_SHAPE;
    if ((uintptr_t)a->data % sizeof(float)) return SEGM_E_SHAPE;
    if (a->seg_dtype < SEGM_PREP_SEG_NONE || a->seg_dtype > SEGM_PREP_SEG_I16) return SEGM_E_DTYPE;
    if ((a->seg_dtype != SEGM_PREP_SEG_NONE) != (a->seg != NULL)) return SEGM_E_NULL;
    if (a->masked != 0 && a->masked != 1) return SEGM_E_SHAPE;
    if (a->nonzero_label < -1 || a->nonzero_label > 32767) return SEGM_E_SHAPE;
    const int ssize = a->seg_dtype == SEGM_PREP_SEG_F32 ? 4 : a->seg_dtype == SEGM_PREP_SEG_I16 ? 2 : 1;
    if (a->seg && (uintptr_t)a->seg % ssize) return SEGM_E_SHAPE;
    memset(&P, 0, sizeof(P));
    P.data = a->data; P.mask = a->mask; P.seg = a->seg;
    P.sc = a->stride_c; P.sz = a->stride_z; P.sy = a->stride_y;
    P.C = a->channels; P.D = a->depth; P.H = a->height; P.W = a->width;
    P.z0 = a->box_z; P.y0 = a->box_y; P.x0 = a->box_x; P.d = a->box_depth; P.h = a->box_height; P.w = a->box_width;
    P.xa0 = a->box_x & ~3;
    P.cpr = (a->box_x + a->box_width + 3) / 4 - a->box_x / 4;
    P.seg_dtype = a->seg_dtype; P.masked = a->masked; P.nonzero_label = a->nonzero_label;
    P.vec = a->stride_c % 4 == 0 && a->stride_z % 4 == 0 && a->stride_y % 4 == 0 && (uintptr_t)a->data % 16 == 0;
    P.mvec = a->width % 4 == 0 && (uintptr_t)a->mask % 4 == 0;
    P.svec = a->width % 4 == 0 && (uintptr_t)a->seg % (4 * ssize) == 0;
    const int64_t items = (int64_t)a->box_depth * a->box_height * P.cpr;
    P.nitems = (uint32_t)items;
    P.nblocks = (int32_t)prep_blocks(items);
    return SEGM_OK;
}

}  // namespace segm

using namespace segm;

extern "C" int segm_nonzero_mask_bbox(const segm_nonzero_mask_bbox_args* a) {
    if (!a) return SEGM_E_NULL;
    if (!a->data || !a->mask || !a->bbox) return SEGM_E_NULL;
    if (a->channels < 1 || a->channels > SEGM_PREP_MAX_CHANNELS) return SEGM_E_SHAPE;
    if (a->depth <= 0 || a->height <= 0 || a->width <= 0) return SEGM_E_SHAPE;
    if ((int64_t)a->depth * a->height > SEGM_CCL_MAX_VOXELS || (int64_t)a->depth * a->height * a->width > SEGM_CCL_MAX_VOXELS) return SEGM_E_SHAPE;
    if (a->stride_y < a->width || a->stride_z < 0 || a->stride_c < 0) return SEGM_E_SHAPE;
    if ((uintptr_t)a->data % sizeof(float) || (uintptr_t)a->bbox % sizeof(int32_t)) return SEGM_E_SHAPE;
    MaskDev P;
    memset(&P, 0, sizeof(P));
    P.data = a->data; P.mask = a->mask; P.bbox = a->bbox;
    P.sc = a->stride_c; P.sz = a->stride_z; P.sy = a->stride_y;
    P.C = a->channels; P.D = a->depth; P.H = a->height; P.W = a->width;
    P.cpr = (a->width + 3) / 4;
    P.nthreads = (uint32_t)((int64_t)a->depth * a->height * P.cpr);
    P.vec = a->stride_c % 4 == 0 && a->stride_z % 4 == 0 && a->stride_y % 4 == 0 && (uintptr_t)a->data % 16 == 0;
    P.pack = a->width % 4 == 0 && (uintptr_t)a->mask % 4 == 0;
    hipStream_t st = (hipStream_t)a->stream;
    // the lower ends start at 0x7f7f7f7f (above every index), the upper ends at 0
    if (hipMemsetAsync(a->bbox, 0x7f, 3 * sizeof(int32_t), st) != hipSuccess) return (int)hipGetLastError();
    if (hipMemsetAsync(a->bbox + 3, 0, 3 * sizeof(int32_t), st) != hipSuccess) return (int)hipGetLastError();
    hipLaunchKernelGGL(nonzero_mask_bbox_kernel, dim3((P.nthreads + kBlock - 1) / kBlock), dim3(kBlock), 0, st, P);
    return (int)hipGetLastError();
}

extern "C" size_t segm_crop_stats_workspace_bytes(int32_t channels, int32_t box_depth, int32_t box_height, int32_t box_width) {
    if (channels < 1 || channels > SEGM_PREP_MAX_CHANNELS || box_depth <= 0 || box_height <= 0 || box_width <= 0) return 0;
    // a box row starts anywhere: at most width / 4 + 2 packets
    const int64_t items = (int64_t)box_depth * box_height * (box_width / 4 + 2);
    return (size_t)prep_blocks(items) * (size_t)(channels + 1) * sizeof(double);
}

extern "C" int segm_crop_stats(const segm_crop_args* a) {
    CropDev P;
    const int rc = crop_setup(a, P);
    if (rc != SEGM_OK) return rc;
    if (!a->stats64 || !a->stats32) return SEGM_E_NULL;
    if (a->masked && !a->mask) return SEGM_E_NULL;
    if ((uintptr_t)a->stats64 % sizeof(double) || (uintptr_t)a->stats32 % sizeof(float)) return SEGM_E_SHAPE;
    const size_t need = (size_t)P.nblocks * (size_t)(P.C + 1) * sizeof(double);
    if (!a->workspace || a->workspace_bytes < need || (uintptr_t)a->workspace % sizeof(double)) return SEGM_E_WORKSPACE;
    P.stats64 = a->stats64; P.stats32 = a->stats32; P.part = (double*)a->workspace;
    hipStream_t st = (hipStream_t)a->stream;
    for (int pass = 0; pass < 2; ++pass) {
        P.pass = pass;
        hipLaunchKernelGGL(crop_stats_partial_kernel, dim3((unsigned)P.nblocks), dim3(kBlock), 0, st, P);
        hipLaunchKernelGGL(crop_stats_final_kernel, dim3(1), dim3(kBlock), 0, st, P);
    }
    return (int)hipGetLastError();
}

static int crop_normalize_launch(const segm_crop_args* a, bool clip) {
    CropDev P;
    const int rc = crop_setup(a, P);
    if (rc != SEGM_OK) return rc;
    if (clip && a->masked) return SEGM_E_SHAPE;
    if (!a->stats32 || !a->out) return SEGM_E_NULL;
    if ((uintptr_t)a->stats32 % sizeof(float) || (uintptr_t)a->out % sizeof(float)) return SEGM_E_SHAPE;
    P.labels = (a->seg_out || a->counts || a->masked) ? 1 : 0;
    if (P.labels && !a->mask) return SEGM_E_NULL;
    if ((uintptr_t)a->seg_out % sizeof(int16_t) || (uintptr_t)a->counts % sizeof(int64_t)) return SEGM_E_SHAPE;
    P.stats32 = a->stats32; P.out = a->out; P.seg_out = a->seg_out; P.counts = (long long*)a->counts;
    hipStream_t st = (hipStream_t)a->stream;
    if (a->counts && hipMemsetAsync(a->counts, 0, SEGM_PREP_COUNT_BINS * sizeof(int64_t), st) != hipSuccess) return (int)hipGetLastError();
    if (clip) hipLaunchKernelGGL(crop_normalize_kernel<true>, dim3((unsigned)P.nblocks), dim3(kBlock), 0, st, P);
    else hipLaunchKernelGGL(crop_normalize_kernel<false>, dim3((unsigned)P.nblocks), dim3(kBlock), 0, st, P);
    return (int)hipGetLastError();
}

extern "C" int segm_crop_normalize(const segm_crop_args* a) { return crop_normalize_launch(a, false); }

extern "C" int segm_crop_clip_normalize(const segm_crop_args* a) { return crop_normalize_launch(a, true); }
