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
// The kernels stand on the skeleton that loss_common.h describes: rl_fwd_kernel writes rows of 4 x 8 + 1 doubles (I, P, G, E per
// region, then N) and is bound by its arithmetic (four transcendental instructions per voxel and region), not by memory;
// loss_finish_kernel adds them to the (4 B R + B) results; rl_bwd_kernel is dlogits = m (p (1 - p) (gI t + gP) + gE (p - t)).
#include <math.h>
#include <string.h>

#include "loss_common.h"

namespace segm {

constexpr int kRlMaxR = SEGM_REGION_MAX_REGIONS;
constexpr int kRlRow = 4 * kRlMaxR + 1;              // doubles of a partial row: I, P, G, E per region, then N
static_assert(kRlMaxR <= kLossPacketMaxN, "a packet instantiation for every region count");

struct RlDev : LossGeom {                            // n: the regions
    const void* logits;
    const void* target;
    void* dlogits;
    double* part;                                    // [batch][nchunks][kRlRow]
    double* sums;
    const float* g_i;
    const float* g_p;
    const float* g_e;
    int64_t ignore_label;
    uint32_t masks[kRlMaxR];
    int32_t planes, kind, has_ignore;
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

// ---- targets --------------------------------------------------------------------------------------------------------------------------
// what a packet needs once for all regions: the labels (label modes) or the validity from the ignore plane (plane modes)
template <int N>
__device__ __forceinline__ void rl_packet_head(const RlDev& P, int b, int64_t v, uint32_t lab[N], bool m[N], uint32_t& bad) {
    const int64_t i = (int64_t)b * P.V + v;
    if (P.kind <= SEGM_REGION_LABELS_F32) {                               // uniform over the grid
        loss_labels<N>(P.target, P.kind, i, [&](int k, int64_t l, bool whole) {
            const bool ign = whole && P.has_ignore && l == P.ignore_label;
            const bool oob = !whole || l < 0 || l >= 32;
            m[k] = !ign;
            bad |= (!ign && oob) ? 1u << k : 0u;
            lab[k] = (ign || oob) ? 0u : (uint32_t)l;
        });
    } else {
#pragma unroll
        for (int k = 0; k < N; ++k) { lab[k] = 0u; m[k] = true; }
        if (P.planes > P.n) {                                             // the reference's mask = (1 - target[:, -1:]).bool()
            const int64_t j = ((int64_t)b * P.planes + P.n) * P.V + v;
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
    const int nreg = RT ? RT : P.n;
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
        const int64_t off = loss_offset(P, v);
#pragma unroll
        for (int r = 0; r < RM; ++r) {
            if (r < nreg) {
                Pack<T, VEC> x;
                x.load(xb + (int64_t)r * P.sn + off);
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
    loss_block_row<kRlRow>(s_part, P.part, b, P.nchunks, blockIdx.x);
}

// ---- backward ---------------------------------------------------------------------------------------------------------------------------
template <typename T, bool VEC, int RT>
__global__ void __launch_bounds__(kBlock) rl_bwd_kernel(RlDev P) {
    constexpr int N = VEC ? Vec<T>::N : 1;
    constexpr int RM = RT ? RT : kRlMaxR;
    const int nreg = RT ? RT : P.n;
    const int b = blockIdx.y;
    const int64_t v = ((int64_t)blockIdx.x * kBlock + threadIdx.x) * N;
    if (v >= P.V) return;
    const T* xb = reinterpret_cast<const T*>(P.logits) + (int64_t)b * P.sb;
    T* db = reinterpret_cast<T*>(P.dlogits) + (int64_t)b * P.n * P.V + v;
    uint32_t lab[N];
    bool m[N];
    uint32_t bad = 0;
    rl_packet_head<N>(P, b, v, lab, m, bad);
    const int64_t off = loss_offset(P, v);
#pragma unroll
    for (int r = 0; r < RM; ++r) {
        if (r < nreg) {
            Pack<T, VEC> x, d;
            x.load(xb + (int64_t)r * P.sn + off);
            float t[N];
            rl_packet_target<N>(P, b, r, P.masks[r], v, lab, t);
            const float gi = P.g_i[b * P.n + r], gp = P.g_p[b * P.n + r], ge = P.g_e[b * P.n + r];
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
// the checks the two entries share; 0 or a SEGM_E_* status.  `vec` tells whether the packet route may be taken.
static int rl_setup(const segm_region_loss_args* a, RlDev& P, bool& vec) {
    if (!a) return SEGM_E_NULL;
    const bool labels = a->target_kind <= SEGM_REGION_LABELS_F32;
    int own = SEGM_OK;
    if (a->target_kind < SEGM_REGION_LABELS_I64 || a->target_kind > SEGM_REGION_PLANES_F32) own = SEGM_E_DTYPE;
    else if (a->ignore_plane != 0 && (labels || a->ignore_plane != 1)) own = SEGM_E_SHAPE;
    memset(&P, 0, sizeof(P));
    const int rc = loss_setup(a, a->regions, kRlMaxR, a->stride_r, a->target, a->target_kind, own, P);
    if (rc != SEGM_OK) return rc;
    P.logits = a->logits; P.target = a->target;
    P.ignore_label = a->ignore_label;
    P.has_ignore = labels && a->has_ignore ? 1 : 0;
    for (int r = 0; r < kRlMaxR; ++r) P.masks[r] = r < a->regions ? a->masks[r] : 0u;
    P.planes = a->regions + a->ignore_plane; P.kind = a->target_kind;
    vec = loss_rows_aligned(a, a->regions, a->stride_r) && (uintptr_t)a->target % 16 == 0;      // the dense target: whole packets
    return SEGM_OK;
}

}  // namespace segm

using namespace segm;

extern "C" size_t segm_region_loss_workspace_bytes(int32_t batch, int32_t regions, int64_t voxels) {
    return loss_workspace_bytes(batch, regions, kRlMaxR, voxels, kRlRow);
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
    SEGM_LOSS_LAUNCH(rl_fwd_kernel, a->dtype);
    hipLaunchKernelGGL((loss_finish_kernel<kRlRow, 4, kRlMaxR>), dim3((unsigned)P.B), dim3(kBlock), 0, st, P.part, P.sums, P.nchunks, P.n, P.B);
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
    const dim3 grid = loss_bwd_grid(P, vec, a->dtype);
    hipStream_t st = (hipStream_t)a->stream;
    SEGM_LOSS_LAUNCH(rl_bwd_kernel, a->dtype);
    return (int)hipGetLastError();
}
