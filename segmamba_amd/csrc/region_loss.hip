// nnU-Net's region-based loss on the device: the sums behind sigmoid Dice + BCE, and their gradient (C ABI:
// segm_region_loss_workspace_bytes, segm_region_loss_fwd, segm_region_loss_bwd).
//
// Replaces what the reference's DC_and_BCE_loss (light_training/loss/compound_losses.py:84-100) and its Dice classes
// (light_training/loss/dice.py:72-113) run over the volume: torch.sigmoid, the products with the one-hot region target and the loss
// mask, five reductions over the spatial axes, BCEWithLogitsLoss, and autograd's backward of all of them.  With p = sigmoid(x),
//     I = sum m p t     P = sum m p     G = sum m t     E = sum m (max(x, 0) - x t + log1p(exp(-|x|)))     N = sum m
// per (sample, region), N per sample.  The region target t is never in memory when the caller has a label map: a region is a 32-bit
// membership mask over the labels, t = (mask >> label) & 1.
//
//   * rl_fwd_kernel     a workgroup owns a stretch of `chunk` voxels of one sample for ALL regions, so the label (or the ignore plane)
//                       is read once.  A thread takes packets of 16 bytes of logits along x (4 fp32, 8 fp16 / bf16) where the rows are
//                       aligned, single voxels otherwise; the per-voxel terms come from ONE function (rl_terms) whose products
//                       are rounded on their own, so both routes compute a voxel alike.  Every term is added in fp64 in the thread,
//                       then over the wave by shuffles, then over the four waves through LDS; the workgroup writes one row of
//                       4 x 8 + 1 doubles.  The kernel is bound by its arithmetic (four transcendental instructions per voxel and
//                       region), not by memory.
//   * rl_finish_kernel  one workgroup per sample adds the rows in a fixed order (wave w takes the sums w, w + 4, ..., lane l the
//                       rows l, l + 64, ..., then a shuffle tree) and writes the (4 B R + B) fp64 results.  No floating-point
//                       atomic: two calls are bit-equal.
//   * rl_bwd_kernel     the same packets, no reduction: the sigmoid again, dlogits = m (p (1 - p) (gI t + gP) + gE (p - t)).
#include <math.h>
#include <string.h>

#include "loss_common.h"

namespace segm {

constexpr int kRlMaxR = SEGM_REGION_MAX_REGIONS;
constexpr int kRlQuantum = kBlock * 8;               // a chunk is a multiple of this: whole packets for every thread, both packet sizes
constexpr int kRlMaxChunks = 512;                    // per sample; 128^3 voxels -> 512 chunks of 4096
constexpr int kRlRow = 4 * kRlMaxR + 1;              // doubles of a partial row: I, P, G, E per region, then N
static_assert(kRlRow <= kBlock, "one thread per slot of the row");

struct RlDev {
    const void* logits;
    const void* target;
    void* dlogits;
    double* part;                                    // [batch][nchunks][kRlRow]
    double* sums;
    const float* g_i;
    const float* g_p;
    const float* g_e;
    int64_t sb, sr, sz, sy;
    int64_t ignore_label;
    uint32_t masks[kRlMaxR];
    int32_t V, X, Y;                                 // voxels of a sample, width, height
    int32_t B, R, planes, kind, has_ignore, dense, chunk, nchunks;
};

// ---- the per-voxel arithmetic: one function for every route ---------------------------------------------------------------------------
// RL_ROUND (loss_common.h): a product that feeds a sum is rounded on its own in every route.

struct RlTerms { float p, pt, e; };

// exp(-|x|) = e in (0, 1]; u = 1 + e; log1p(e) = log(u) e / (u - 1) corrects the rounding of u (e where u rounds to 1)
__device__ __forceinline__ void rl_sigmoid(float x, float& p, float& l1p) {
#pragma clang fp contract(off)
    const float e = fast_exp(-fabsf(x));
    const float u = 1.0f + e;
    const float inv = fast_rcp(u);
    const float d = u - 1.0f;
    l1p = d == 0.f ? e : fast_log(u) * (e * fast_rcp(d));
    RL_ROUND(l1p);
    p = x >= 0.f ? inv : e * inv;
}

__device__ __forceinline__ RlTerms rl_terms(float x, float t) {
#pragma clang fp contract(off)
    float p, l1p;
    rl_sigmoid(x, p, l1p);
    RlTerms o;
    o.p = p;
    o.pt = p * t;
    float xt = x * t;
    RL_ROUND(xt);
    o.e = (fmaxf(x, 0.f) - xt) + l1p;
    return o;
}

__device__ __forceinline__ float rl_grad(float x, float t, float gi, float gp, float ge) {
#pragma clang fp contract(off)
    float p, l1p;
    rl_sigmoid(x, p, l1p);
    const float q = p * (1.0f - p);
    float a = gi * t;
    RL_ROUND(a);
    float dice = q * (a + gp);
    RL_ROUND(dice);
    float bce = ge * (p - t);
    RL_ROUND(bce);
    return dice + bce;
}

// ---- addresses ------------------------------------------------------------------------------------------------------------------------
// voxel v of a sample (C order over z, y, x) -> its element offset in a logits plane
__device__ __forceinline__ int64_t rl_offset(const RlDev& P, int64_t v) {
    if (P.dense) return v;
    const uint32_t row = (uint32_t)v / (uint32_t)P.X, col = (uint32_t)v - row * (uint32_t)P.X;
    const uint32_t z = row / (uint32_t)P.Y, y = row - z * (uint32_t)P.Y;
    return (int64_t)z * P.sz + (int64_t)y * P.sy + (int64_t)col;
}

// the labels of a packet: lab in [0, 32) (0 where it does not count), m = the voxel counts, bit k of bad = voxel k has a wrong label
template <typename S, int N>
__device__ __forceinline__ void rl_labels(const RlDev& P, int64_t i, uint32_t lab[N], bool m[N], uint32_t& bad) {
    S raw[N];
    rl_load<S, N>(P.target, i, raw);
#pragma unroll
    for (int k = 0; k < N; ++k) {
        const int64_t l = (int64_t)raw[k];
        const bool ign = P.has_ignore && l == P.ignore_label;
        const bool oob = l < 0 || l >= 32;
        m[k] = !ign;
        bad |= (!ign && oob) ? 1u << k : 0u;
        lab[k] = (ign || oob) ? 0u : (uint32_t)l;
    }
}

template <int N>
__device__ __forceinline__ void rl_labels_f32(const RlDev& P, int64_t i, uint32_t lab[N], bool m[N], uint32_t& bad) {
    float raw[N];
    rl_load<float, N>(P.target, i, raw);
#pragma unroll
    for (int k = 0; k < N; ++k) {
        const float f = raw[k];
        const bool whole = f == floorf(f) && fabsf(f) < 4.0e18f;         // NaN and inf are no integers
        const int64_t l = whole ? (int64_t)f : (int64_t)-1;
        const bool ign = whole && P.has_ignore && l == P.ignore_label;
        const bool oob = !whole || l < 0 || l >= 32;
        m[k] = !ign;
        bad |= (!ign && oob) ? 1u << k : 0u;
        lab[k] = (ign || oob) ? 0u : (uint32_t)l;
    }
}

// what a packet needs once for all regions: the labels (label modes) or the validity from the ignore plane (plane modes)
template <int N>
__device__ __forceinline__ void rl_packet_head(const RlDev& P, int b, int64_t v, uint32_t lab[N], bool m[N], uint32_t& bad) {
    const int64_t i = (int64_t)b * P.V + v;
    switch (P.kind) {                                                     // uniform over the grid
    case SEGM_REGION_LABELS_I64: rl_labels<int64_t, N>(P, i, lab, m, bad); break;
    case SEGM_REGION_LABELS_I16: rl_labels<int16_t, N>(P, i, lab, m, bad); break;
    case SEGM_REGION_LABELS_U8: rl_labels<uint8_t, N>(P, i, lab, m, bad); break;
    case SEGM_REGION_LABELS_F32: rl_labels_f32<N>(P, i, lab, m, bad); break;
    default: {
#pragma unroll
        for (int k = 0; k < N; ++k) { lab[k] = 0u; m[k] = true; }
        if (P.planes > P.R) {                                             // the reference's mask = (1 - target[:, -1:]).bool()
            const int64_t j = ((int64_t)b * P.planes + P.R) * P.V + v;
            float last[N];
            if (P.kind == SEGM_REGION_PLANES_U8) {
                uint8_t raw[N];
                rl_load<uint8_t, N>(P.target, j, raw);
#pragma unroll
                for (int k = 0; k < N; ++k) last[k] = (float)raw[k];
            } else {
                rl_load<float, N>(P.target, j, last);
            }
#pragma unroll
            for (int k = 0; k < N; ++k) m[k] = (1.0f - last[k]) != 0.f;
        }
    } break;
    }
}

// the targets of region r for a packet
template <int N>
__device__ __forceinline__ void rl_packet_target(const RlDev& P, int b, int r, uint32_t mask, int64_t v, const uint32_t lab[N], float t[N]) {
    if (P.kind <= SEGM_REGION_LABELS_F32) {
#pragma unroll
        for (int k = 0; k < N; ++k) t[k] = (float)((mask >> lab[k]) & 1u);
    } else {
        const int64_t j = ((int64_t)b * P.planes + r) * P.V + v;
        if (P.kind == SEGM_REGION_PLANES_U8) {
            uint8_t raw[N];
            rl_load<uint8_t, N>(P.target, j, raw);
#pragma unroll
            for (int k = 0; k < N; ++k) t[k] = (float)raw[k];
        } else {
            rl_load<float, N>(P.target, j, t);
        }
    }
}

// ---- forward ----------------------------------------------------------------------------------------------------------------------------
// RT: the number of regions where the instantiation knows it (the packet route: no branch between the loads of a packet, only the
// accumulators it needs), 0 where it is read from the arguments (the per-voxel route)
template <typename T, bool VEC, int RT>
__global__ void __launch_bounds__(kBlock) rl_fwd_kernel(RlDev P) {
    constexpr int N = VEC ? Vec<T>::N : 1;
    constexpr int RM = RT ? RT : kRlMaxR;
    const int nreg = RT ? RT : P.R;
    __shared__ double s_part[kWavesPerBlock][kRlRow];
    const int b = blockIdx.y;
    const int64_t lo = (int64_t)blockIdx.x * P.chunk;
    const T* xb = reinterpret_cast<const T*>(P.logits) + (int64_t)b * P.sb;
    double aI[RM], aP[RM], aG[RM], aE[RM];
#pragma unroll
    for (int r = 0; r < RM; ++r) aI[r] = aP[r] = aG[r] = aE[r] = 0.0;
    uint32_t count = 0;
    uint32_t bad = 0;
    for (int32_t j = (int32_t)threadIdx.x * N; j < P.chunk; j += kBlock * N) {
        const int64_t v = lo + j;                    // VEC: V % N == 0, a packet is whole or absent
        if (v >= P.V) break;
        uint32_t lab[N];
        bool m[N];
        rl_packet_head<N>(P, b, v, lab, m, bad);
#pragma unroll
        for (int k = 0; k < N; ++k) count += m[k] ? 1u : 0u;
        const int64_t off = rl_offset(P, v);
#pragma unroll
        for (int r = 0; r < RM; ++r) {
            if (r < nreg) {
                Pack<T, VEC> x;
                x.load(xb + (int64_t)r * P.sr + off);
                float t[N];
                rl_packet_target<N>(P, b, r, P.masks[r], v, lab, t);
#pragma unroll
                for (int k = 0; k < N; ++k) {
                    if (m[k]) {
                        const RlTerms o = rl_terms(x.v[k], t[k]);
                        aI[r] += (double)o.pt;
                        aP[r] += (double)o.p;
                        aG[r] += (double)t[k];
                        aE[r] += (double)o.e;
                    }
                }
            }
        }
    }
    const double poison = bad != 0 ? (double)__builtin_nanf("") : 0.0;         // a wrong label: NaN in this sample's I, P and E
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
#pragma unroll
    for (int r = 0; r < RM; ++r) {
        if (r < nreg) {                              // uniform: every lane of the wave takes part in the shuffles
            const double sI = rl_wave_sum(aI[r] + poison), sP = rl_wave_sum(aP[r] + poison);
            const double sG = rl_wave_sum(aG[r]), sE = rl_wave_sum(aE[r] + poison);
            if (lane == 0) {
                s_part[wave][r] = sI; s_part[wave][kRlMaxR + r] = sP;
                s_part[wave][2 * kRlMaxR + r] = sG; s_part[wave][3 * kRlMaxR + r] = sE;
            }
        }
    }
    if (lane == 0) {
        for (int r = nreg; r < kRlMaxR; ++r) {
            s_part[wave][r] = 0.0; s_part[wave][kRlMaxR + r] = 0.0;
            s_part[wave][2 * kRlMaxR + r] = 0.0; s_part[wave][3 * kRlMaxR + r] = 0.0;
        }
    }
    const double sN = rl_wave_sum((double)count);
    if (lane == 0) s_part[wave][4 * kRlMaxR] = sN;
    __syncthreads();
    if ((int)threadIdx.x < kRlRow) {
        double s = s_part[0][threadIdx.x];
        for (int w = 1; w < kWavesPerBlock; ++w) s += s_part[w][threadIdx.x];
        P.part[((int64_t)b * P.nchunks + blockIdx.x) * kRlRow + threadIdx.x] = s;
    }
}

// one workgroup per sample: wave w takes the slots w, w + 4, ...; lane l the rows l, l + 64, ...; then a shuffle tree
__global__ void __launch_bounds__(kBlock) rl_finish_kernel(RlDev P) {
    const int b = blockIdx.x;
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    const double* rows = P.part + (int64_t)b * P.nchunks * kRlRow;
    const int64_t br = (int64_t)P.B * P.R;
    for (int slot = wave; slot < kRlRow; slot += kWavesPerBlock) {
        const int q = slot / kRlMaxR, r = slot - q * kRlMaxR;
        if (q < 4 && r >= P.R) continue;             // uniform over the wave
        double acc = 0.0;
        for (int c = lane; c < P.nchunks; c += kWave) acc += rows[(int64_t)c * kRlRow + slot];
        acc = rl_wave_sum(acc);
        if (lane == 0) {
            if (q < 4) P.sums[q * br + (int64_t)b * P.R + r] = acc;
            else P.sums[4 * br + b] = acc;
        }
    }
}

// ---- backward ---------------------------------------------------------------------------------------------------------------------------
template <typename T, bool VEC, int RT>
__global__ void __launch_bounds__(kBlock) rl_bwd_kernel(RlDev P) {
    constexpr int N = VEC ? Vec<T>::N : 1;
    constexpr int RM = RT ? RT : kRlMaxR;
    const int nreg = RT ? RT : P.R;
    const int b = blockIdx.y;
    const int64_t v = ((int64_t)blockIdx.x * kBlock + threadIdx.x) * N;
    if (v >= P.V) return;
    const T* xb = reinterpret_cast<const T*>(P.logits) + (int64_t)b * P.sb;
    T* db = reinterpret_cast<T*>(P.dlogits) + (int64_t)b * P.R * P.V + v;
    uint32_t lab[N];
    bool m[N];
    uint32_t bad = 0;
    rl_packet_head<N>(P, b, v, lab, m, bad);
    const int64_t off = rl_offset(P, v);
#pragma unroll
    for (int r = 0; r < RM; ++r) {
        if (r < nreg) {
            Pack<T, VEC> x, d;
            x.load(xb + (int64_t)r * P.sr + off);
            float t[N];
            rl_packet_target<N>(P, b, r, P.masks[r], v, lab, t);
            const float gi = P.g_i[b * P.R + r], gp = P.g_p[b * P.R + r], ge = P.g_e[b * P.R + r];
#pragma unroll
            for (int k = 0; k < N; ++k) {
                const float g = rl_grad(x.v[k], t[k], gi, gp, ge);
                d.v[k] = ((bad >> k) & 1u) ? __builtin_nanf("") : (m[k] ? g : 0.f);
            }
            d.store(db + (int64_t)r * P.V);
        }
    }
}

// ---- host -------------------------------------------------------------------------------------------------------------------------------
static int32_t rl_chunk(int64_t voxels) {
    const int64_t per = (voxels + kRlMaxChunks - 1) / kRlMaxChunks;
    const int64_t chunk = ((per + kRlQuantum - 1) / kRlQuantum) * kRlQuantum;
    return (int32_t)(chunk < kRlQuantum ? kRlQuantum : chunk);
}

static size_t rl_target_esize(int kind) {
    switch (kind) {
    case SEGM_REGION_LABELS_I64: return 8;
    case SEGM_REGION_LABELS_I16: return 2;
    case SEGM_REGION_LABELS_U8: case SEGM_REGION_PLANES_U8: return 1;
    default: return 4;
    }
}

// the checks the two entries share; 0 or a SEGM_E_* status.  `vec` tells whether the packet route may be taken.
static int rl_setup(const segm_region_loss_args* a, RlDev& P, bool& vec) {
    if (!a) return SEGM_E_NULL;
    if (a->batch <= 0 || a->regions < 1 || a->regions > kRlMaxR || a->depth <= 0 || a->height <= 0 || a->width <= 0) return SEGM_E_SHAPE;
    if (a->batch > 65535) return SEGM_E_SHAPE;                            // the grid's y
    const int64_t voxels = (int64_t)a->depth * a->height * a->width;
    if (voxels >= ((int64_t)1 << 31)) return SEGM_E_SHAPE;
    if (a->stride_x != 1 || a->stride_b < 0 || a->stride_r < 0 || a->stride_z < 0 || a->stride_y < 0) return SEGM_E_SHAPE;
    if (a->dtype != SEGM_F32 && a->dtype != SEGM_F16 && a->dtype != SEGM_BF16) return SEGM_E_DTYPE;
    if (a->target_kind < SEGM_REGION_LABELS_I64 || a->target_kind > SEGM_REGION_PLANES_F32) return SEGM_E_DTYPE;
    const bool labels = a->target_kind <= SEGM_REGION_LABELS_F32;
    if (a->ignore_plane != 0 && (labels || a->ignore_plane != 1)) return SEGM_E_SHAPE;
    if (!a->logits || !a->target) return SEGM_E_NULL;
    const size_t esize = a->dtype == SEGM_F32 ? 4 : 2;
    if ((uintptr_t)a->logits % esize || (uintptr_t)a->target % rl_target_esize(a->target_kind)) return SEGM_E_SHAPE;
    memset(&P, 0, sizeof(P));
    P.logits = a->logits; P.target = a->target;
    P.sb = a->stride_b; P.sr = a->stride_r; P.sz = a->stride_z; P.sy = a->stride_y;
    P.ignore_label = a->ignore_label;
    P.has_ignore = labels && a->has_ignore ? 1 : 0;
    for (int r = 0; r < kRlMaxR; ++r) P.masks[r] = r < a->regions ? a->masks[r] : 0u;
    P.V = (int32_t)voxels; P.X = a->width; P.Y = a->height;
    P.B = a->batch; P.R = a->regions; P.planes = a->regions + a->ignore_plane; P.kind = a->target_kind;
    P.dense = (a->height == 1 || a->stride_y == a->width) && (a->depth == 1 || a->stride_z == (int64_t)a->width * a->height);
    P.chunk = rl_chunk(voxels);
    P.nchunks = (int32_t)((voxels + P.chunk - 1) / P.chunk);
    // packets: every row starts at a multiple of 16 bytes in the logits and at a multiple of the packet in the dense target
    const int64_t n = (int64_t)(16 / esize);
    // (the strides of axes of size 1 are never used)
    vec = a->width % n == 0 && (a->batch == 1 || a->stride_b % n == 0) && (a->regions == 1 || a->stride_r % n == 0) &&
          (a->depth == 1 || a->stride_z % n == 0) && (a->height == 1 || a->stride_y % n == 0) &&
          (uintptr_t)a->logits % 16 == 0 && (uintptr_t)a->target % 16 == 0;
    return SEGM_OK;
}

}  // namespace segm

using namespace segm;

extern "C" size_t segm_region_loss_workspace_bytes(int32_t batch, int32_t regions, int64_t voxels) {
    if (batch <= 0 || batch > 65535 || regions < 1 || regions > kRlMaxR || voxels < 1 || voxels >= ((int64_t)1 << 31)) return 0;
    const int32_t chunk = rl_chunk(voxels);
    const int64_t nchunks = (voxels + chunk - 1) / chunk;
    return (size_t)batch * (size_t)nchunks * kRlRow * sizeof(double);
}

extern "C" int segm_region_loss_fwd(const segm_region_loss_args* a) {
    RlDev P;
    bool vec = false;
    const int rc = rl_setup(a, P, vec);
    if (rc != SEGM_OK) return rc;
    if (!a->sums) return SEGM_E_NULL;
    if ((uintptr_t)a->sums % sizeof(double)) return SEGM_E_SHAPE;
    const size_t need = segm_region_loss_workspace_bytes(a->batch, a->regions, P.V);
    if (!a->workspace || a->workspace_bytes < need || (uintptr_t)a->workspace % sizeof(double)) return SEGM_E_WORKSPACE;
    P.part = (double*)a->workspace;
    P.sums = a->sums;
    const dim3 grid((unsigned)P.nchunks, (unsigned)P.B);
    hipStream_t st = (hipStream_t)a->stream;
#define SEGM_RL_FWD_R(T, RT) case RT: hipLaunchKernelGGL((rl_fwd_kernel<T, true, RT>), grid, dim3(kBlock), 0, st, P); break
#define SEGM_RL_FWD(T) \
    do { if (vec) switch (P.R) { SEGM_RL_FWD_R(T, 1); SEGM_RL_FWD_R(T, 2); SEGM_RL_FWD_R(T, 3); SEGM_RL_FWD_R(T, 4); \
                                 SEGM_RL_FWD_R(T, 5); SEGM_RL_FWD_R(T, 6); SEGM_RL_FWD_R(T, 7); SEGM_RL_FWD_R(T, 8); } \
         else hipLaunchKernelGGL((rl_fwd_kernel<T, false, 0>), grid, dim3(kBlock), 0, st, P); } while (0)
    if (a->dtype == SEGM_F32) SEGM_RL_FWD(float);
    else if (a->dtype == SEGM_F16) SEGM_RL_FWD(f16_t);
    else SEGM_RL_FWD(bf16_t);
#undef SEGM_RL_FWD
#undef SEGM_RL_FWD_R
    hipLaunchKernelGGL(rl_finish_kernel, dim3((unsigned)P.B), dim3(kBlock), 0, st, P);
    return (int)hipGetLastError();
}

extern "C" int segm_region_loss_bwd(const segm_region_loss_args* a) {
    RlDev P;
    bool vec = false;
    const int rc = rl_setup(a, P, vec);
    if (rc != SEGM_OK) return rc;
    if (!a->dlogits || !a->g_i || !a->g_p || !a->g_e) return SEGM_E_NULL;
    const size_t esize = a->dtype == SEGM_F32 ? 4 : 2;
    if ((uintptr_t)a->dlogits % esize || (uintptr_t)a->g_i % sizeof(float) || (uintptr_t)a->g_p % sizeof(float) ||
        (uintptr_t)a->g_e % sizeof(float)) return SEGM_E_SHAPE;
    vec = vec && (uintptr_t)a->dlogits % 16 == 0;
    P.dlogits = a->dlogits; P.g_i = a->g_i; P.g_p = a->g_p; P.g_e = a->g_e;
    const int64_t n = vec ? (int64_t)(16 / esize) : 1;
    const int64_t packets = ((int64_t)P.V + n - 1) / n;
    const dim3 grid((unsigned)((packets + kBlock - 1) / kBlock), (unsigned)P.B);
    hipStream_t st = (hipStream_t)a->stream;
#define SEGM_RL_BWD_R(T, RT) case RT: hipLaunchKernelGGL((rl_bwd_kernel<T, true, RT>), grid, dim3(kBlock), 0, st, P); break
#define SEGM_RL_BWD(T) \
    do { if (vec) switch (P.R) { SEGM_RL_BWD_R(T, 1); SEGM_RL_BWD_R(T, 2); SEGM_RL_BWD_R(T, 3); SEGM_RL_BWD_R(T, 4); \
                                 SEGM_RL_BWD_R(T, 5); SEGM_RL_BWD_R(T, 6); SEGM_RL_BWD_R(T, 7); SEGM_RL_BWD_R(T, 8); } \
         else hipLaunchKernelGGL((rl_bwd_kernel<T, false, 0>), grid, dim3(kBlock), 0, st, P); } while (0)
    if (a->dtype == SEGM_F32) SEGM_RL_BWD(float);
    else if (a->dtype == SEGM_F16) SEGM_RL_BWD(f16_t);
    else SEGM_RL_BWD(bf16_t);
#undef SEGM_RL_BWD
#undef SEGM_RL_BWD_R
    return (int)hipGetLastError();
}
