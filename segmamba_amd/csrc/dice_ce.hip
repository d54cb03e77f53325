// nnU-Net's default loss on the device: the sums behind softmax Dice + cross entropy, and their gradient (C ABI:
// segm_softmax_dice_workspace_bytes, segm_softmax_dice_fwd, segm_softmax_dice_bwd).
//
// Replaces what the reference's Dice classes (light_training/loss/dice.py:9-116) and DC_and_CE_loss
// (light_training/loss/compound_losses.py:8-57) run over the volume: the softmax, the one-hot target, the products with it and with
// the loss mask, the reductions over the spatial axes, RobustCrossEntropyLoss, and autograd's backward of all of them.  With
// p = softmax_c(x), label y and validity m,
//     I = sum m p_c [y = c]     P = sum m p_c     G = sum m [y = c]   per (sample, class),
//     CE = sum m (logsumexp(x) - x_y)     N = sum m                   per sample.
//
// The kernels stand on the skeleton that loss_common.h describes: sd_fwd_kernel writes rows of 3 x 16 + 2 doubles (I, P, G per class,
// then CE and N; G and N are counted as integers in the thread) and takes the packet route where the instantiation knows the class
// count (1 .. kLossPacketMaxN), single voxels with the class count read from the arguments otherwise; the products of its per-voxel
// function (sd_softmax) are rounded on their own or are explicit fused multiply-adds.  loss_finish_kernel adds the rows to the
// (3 B C + 2 B) results.  sd_bwd_kernel is
//     dlogits_j = m (p_j (a_j - S) + gCE (p_j - [j = y])),  a_c = gI_c [y = c] + gP_c,  S = sum_c p_c a_c.
#include <math.h>
#include <string.h>

#include "loss_common.h"

namespace segm {

constexpr int kSdMaxC = SEGM_SOFTMAX_DICE_MAX_CLASSES;
constexpr int kSdRow = 3 * kSdMaxC + 2;              // doubles of a partial row: I, P, G per class, then CE and N
constexpr float kSdLog2eLo = (float)(1.4426950408889634 - (double)kLog2e);      // what kLog2e misses of log2(e)
constexpr float kSdLn2 = 0.6931471805599453f;

struct SdDev : LossGeom {                            // n: the classes
    const void* logits;
    const void* labels;
    const uint8_t* mask;
    void* dlogits;
    double* part;                                    // [batch][nchunks][kSdRow]
    double* sums;
    const float* g_i;
    const float* g_p;
    const float* g_ce;
    int64_t ignore_label;
    int32_t kind, has_ignore;
};

// ---- the per-voxel arithmetic: one function for every route ---------------------------------------------------------------------------
// x[c], c < nc: the logits of one voxel; y its label, or -1.  -> p[c] = softmax(x)[c] and ce = logsumexp(x) - x[y] (logsumexp - max
// where y names no class).  exp(s) for s = x - max <= 0 is exp2(t) (1 + ln2 r) with t = s log2(e) rounded and r what the roundings of
// the difference, of the product and of the constant lost, so a small p carries a relative error of a few 2^-24 whatever its size
// (the rounding of x - max alone is up to 2^-25 |s| in the exponent: 5e-7 relative at s = -10).  The first largest
// logit contributes exp(0) = 1 exactly; `rest` is the sum of the others, logsumexp - max = log1p(rest) = log(u) rest / (u - 1) with
// u = 1 + rest rounded (rest where u rounds to 1), exact to a few 2^-24 relative also where one class dominates.
template <int CM>
__device__ __forceinline__ void sd_softmax(const float x[CM], int nc, int y, float p[CM], float& ce) {
#pragma clang fp contract(off)
    float mx = x[0];
    int am = 0;
#pragma unroll
    for (int c = 1; c < CM; ++c) {
        if (c < nc) {
            const bool up = x[c] > mx;
            mx = up ? x[c] : mx;
            am = up ? c : am;
        }
    }
    float rest = 0.f, shy = 0.f;
#pragma unroll
    for (int c = 0; c < CM; ++c) {
        if (c < nc) {
            const float sh = x[c] - mx;
            const float xp = sh + mx, mp = sh - xp;                       // TwoSum: x - max = sh + lost, exactly
            const float lost = (x[c] - xp) + (-mx - mp);
            const float t = sh * kLog2e;
            const float r = __builtin_fmaf(lost, kLog2e, __builtin_fmaf(sh, kSdLog2eLo, __builtin_fmaf(sh, kLog2e, -t)));
            const float e0 = fast_exp2(t);
            const float e = __builtin_fmaf(e0, r * kSdLn2, e0);
            p[c] = e;
            rest += c == am ? 0.f : e;
            shy = c == y ? sh : shy;
        }
    }
    const float u = 1.0f + rest;
    const float d = u - 1.0f;
    const float inv = fast_rcp(u);
    float l1p = d == 0.f ? rest : fast_log(u) * (rest * fast_rcp(d));
    RL_ROUND(l1p);
    ce = l1p - shy;
#pragma unroll
    for (int c = 0; c < CM; ++c)
        if (c < nc) p[c] = p[c] * inv;
}

// x -> d[c] = p_c (a_c - S) + gce (p_c - [c = y]),  a_c = gi[c] [c = y] + gp[c],  S = sum_c p_c a_c
template <int CM>
__device__ __forceinline__ void sd_grad(const float x[CM], int nc, int y, const float gi[CM], const float gp[CM], float gce, float d[CM]) {
#pragma clang fp contract(off)
    float p[CM], a[CM], ce;
    sd_softmax<CM>(x, nc, y, p, ce);
    float S = 0.f;
#pragma unroll
    for (int c = 0; c < CM; ++c) {
        if (c < nc) {
            a[c] = (c == y ? gi[c] : 0.f) + gp[c];
            S = __builtin_fmaf(p[c], a[c], S);
        }
    }
#pragma unroll
    for (int c = 0; c < CM; ++c) {
        if (c < nc) {
            float dice = p[c] * (a[c] - S);
            RL_ROUND(dice);
            d[c] = __builtin_fmaf(gce, p[c] - (c == y ? 1.0f : 0.f), dice);
        }
    }
}

// ---- labels ----------------------------------------------------------------------------------------------------------------------------
// what a packet needs once for all classes: the labels (y in [0, C), or -1 where the label names no class), whether the voxels count
// (m), bit k of bad = voxel k counts and has a wrong label
template <int N>
__device__ __forceinline__ void sd_packet_head(const SdDev& P, int b, int64_t v, int32_t y[N], bool m[N], uint32_t& bad) {
    const int64_t i = (int64_t)b * P.V + v;
    bool ign[N];
    loss_labels<N>(P.labels, P.kind, i, [&](int k, int64_t l, bool whole) {
        ign[k] = whole && P.has_ignore && l == P.ignore_label;
        y[k] = (!whole || l < 0 || l >= (int64_t)P.n) ? -1 : (int32_t)l;
    });
#pragma unroll
    for (int k = 0; k < N; ++k) m[k] = !ign[k];
    if (P.mask) {
        uint8_t raw[N];
        rl_load<uint8_t, N>(P.mask, i, raw);
#pragma unroll
        for (int k = 0; k < N; ++k) m[k] = m[k] && raw[k] != 0;
    }
#pragma unroll
    for (int k = 0; k < N; ++k) bad |= (m[k] && y[k] < 0) ? 1u << k : 0u;
}

// ---- forward ----------------------------------------------------------------------------------------------------------------------------
// CT: the number of classes where the instantiation knows it (the packet route: no branch between the loads of a packet, only the
// registers it needs), 0 where it is read from the arguments (the per-voxel route)
template <typename T, bool VEC, int CT>
__global__ void __launch_bounds__(kBlock) sd_fwd_kernel(SdDev P) {
    constexpr int N = VEC ? Vec<T>::N : 1;
    constexpr int CM = CT ? CT : kSdMaxC;
    const int nc = CT ? CT : P.n;
    __shared__ double s_part[kWavesPerBlock][kSdRow];
    const int b = blockIdx.y;
    const int64_t lo = (int64_t)blockIdx.x * P.chunk;
    const T* xb = reinterpret_cast<const T*>(P.logits) + (int64_t)b * P.sb;
    double aI[CM], aP[CM];
    uint32_t aG[CM];
#pragma unroll
    for (int c = 0; c < CM; ++c) { aI[c] = aP[c] = 0.0; aG[c] = 0u; }
    double aCE = 0.0;
    uint32_t count = 0;
    uint32_t bad = 0;
    for (int32_t j = (int32_t)threadIdx.x * N; j < P.chunk; j += kBlock * N) {
        const int64_t v = lo + j;                    // VEC: V % N == 0, a packet is whole or absent
        if (v >= P.V) break;
        int32_t y[N];
        bool m[N];
        sd_packet_head<N>(P, b, v, y, m, bad);
        const int64_t off = loss_offset(P, v);
        Pack<T, VEC> x[CM];
#pragma unroll
        for (int c = 0; c < CM; ++c)
            if (c < nc) x[c].load(xb + (int64_t)c * P.sn + off);
#pragma unroll
        for (int k = 0; k < N; ++k) {
            if (m[k]) {
                float xs[CM], p[CM], ce;
#pragma unroll
                for (int c = 0; c < CM; ++c) xs[c] = c < nc ? x[c].v[k] : 0.f;
                sd_softmax<CM>(xs, nc, y[k], p, ce);
#pragma unroll
                for (int c = 0; c < CM; ++c) {
                    if (c < nc) {
                        const bool hit = c == y[k];
                        aP[c] += (double)p[c];
                        aI[c] += hit ? (double)p[c] : 0.0;
                        aG[c] += hit ? 1u : 0u;
                    }
                }
                aCE += (double)ce;
                count += 1u;
            }
        }
    }
    const double poison = bad != 0 ? (double)__builtin_nanf("") : 0.0;         // a wrong label: NaN in this sample's I, P and CE
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
#pragma unroll
    for (int c = 0; c < CM; ++c) {
        if (c < nc) {                                // uniform: every lane of the wave takes part in the shuffles
            const double sI = rl_wave_sum(aI[c] + poison), sP = rl_wave_sum(aP[c] + poison), sG = rl_wave_sum((double)aG[c]);
            if (lane == 0) { s_part[wave][c] = sI; s_part[wave][kSdMaxC + c] = sP; s_part[wave][2 * kSdMaxC + c] = sG; }
        }
    }
    if (lane == 0) {
        for (int c = nc; c < kSdMaxC; ++c) { s_part[wave][c] = 0.0; s_part[wave][kSdMaxC + c] = 0.0; s_part[wave][2 * kSdMaxC + c] = 0.0; }
    }
    const double sCE = rl_wave_sum(aCE + poison), sN = rl_wave_sum((double)count);
    if (lane == 0) { s_part[wave][3 * kSdMaxC] = sCE; s_part[wave][3 * kSdMaxC + 1] = sN; }
    loss_block_row<kSdRow>(s_part, P.part, b, P.nchunks, blockIdx.x);
}

// ---- backward ---------------------------------------------------------------------------------------------------------------------------
template <typename T, bool VEC, int CT>
__global__ void __launch_bounds__(kBlock) sd_bwd_kernel(SdDev P) {
    constexpr int N = VEC ? Vec<T>::N : 1;
    constexpr int CM = CT ? CT : kSdMaxC;
    const int nc = CT ? CT : P.n;
    const int b = blockIdx.y;
    const int64_t v = ((int64_t)blockIdx.x * kBlock + threadIdx.x) * N;
    if (v >= P.V) return;
    const T* xb = reinterpret_cast<const T*>(P.logits) + (int64_t)b * P.sb;
    T* db = reinterpret_cast<T*>(P.dlogits) + (int64_t)b * P.n * P.V + v;
    int32_t y[N];
    bool m[N];
    uint32_t bad = 0;
    sd_packet_head<N>(P, b, v, y, m, bad);
    const int64_t off = loss_offset(P, v);
    Pack<T, VEC> x[CM];
    float gi[CM], gp[CM];
#pragma unroll
    for (int c = 0; c < CM; ++c) {
        if (c < nc) {
            x[c].load(xb + (int64_t)c * P.sn + off);
            gi[c] = P.g_i[b * P.n + c];
            gp[c] = P.g_p[b * P.n + c];
        } else {
            gi[c] = gp[c] = 0.f;
        }
    }
    const float gce = P.g_ce[b];
#pragma unroll
    for (int k = 0; k < N; ++k) {
        float xs[CM], d[CM];
#pragma unroll
        for (int c = 0; c < CM; ++c) xs[c] = c < nc ? x[c].v[k] : 0.f;
        sd_grad<CM>(xs, nc, y[k], gi, gp, gce, d);
#pragma unroll
        for (int c = 0; c < CM; ++c)
            if (c < nc) x[c].v[k] = ((bad >> k) & 1u) ? __builtin_nanf("") : (m[k] ? d[c] : 0.f);      // the gradient takes the logit's place
    }
#pragma unroll
    for (int c = 0; c < CM; ++c)
        if (c < nc) x[c].store(db + (int64_t)c * P.V);
}

// ---- host -------------------------------------------------------------------------------------------------------------------------------
// the checks the two entries share; 0 or a SEGM_E_* status.  `vec` tells whether the packet route may be taken.
static int sd_setup(const segm_softmax_dice_args* a, SdDev& P, bool& vec) {
    if (!a) return SEGM_E_NULL;
    const int own = a->label_kind < SEGM_REGION_LABELS_I64 || a->label_kind > SEGM_REGION_LABELS_F32 ? SEGM_E_DTYPE : SEGM_OK;
    memset(&P, 0, sizeof(P));
    const int rc = loss_setup(a, a->classes, kSdMaxC, a->stride_c, a->labels, a->label_kind, own, P);
    if (rc != SEGM_OK) return rc;
    P.logits = a->logits; P.labels = a->labels; P.mask = a->mask;
    P.ignore_label = a->ignore_label;
    P.has_ignore = a->has_ignore ? 1 : 0;
    P.kind = a->label_kind;
    // the dense labels and mask: whole packets
    vec = a->classes <= kLossPacketMaxN && loss_rows_aligned(a, a->classes, a->stride_c) && (uintptr_t)a->labels % 16 == 0 &&
          (uintptr_t)a->mask % 16 == 0;
    return SEGM_OK;
}

}  // namespace segm

using namespace segm;

extern "C" size_t segm_softmax_dice_workspace_bytes(int32_t batch, int32_t classes, int64_t voxels) {
    return loss_workspace_bytes(batch, classes, kSdMaxC, voxels, kSdRow);
}

extern "C" int segm_softmax_dice_fwd(const segm_softmax_dice_args* a) {
    SdDev P;
    bool vec = false;
    const int rc = sd_setup(a, P, vec);
    if (rc != SEGM_OK) return rc;
    if (!a->sums) return SEGM_E_NULL;
    if ((uintptr_t)a->sums % sizeof(double)) return SEGM_E_SHAPE;
    const size_t need = segm_softmax_dice_workspace_bytes(a->batch, a->classes, P.V);
    if (!a->workspace || a->workspace_bytes < need || (uintptr_t)a->workspace % sizeof(double)) return SEGM_E_WORKSPACE;
    P.part = (double*)a->workspace;
    P.sums = a->sums;
    const dim3 grid((unsigned)P.nchunks, (unsigned)P.B);
    hipStream_t st = (hipStream_t)a->stream;
    SEGM_LOSS_LAUNCH(sd_fwd_kernel, a->dtype);
    hipLaunchKernelGGL((loss_finish_kernel<kSdRow, 3, kSdMaxC>), dim3((unsigned)P.B), dim3(kBlock), 0, st, P.part, P.sums, P.nchunks, P.n, P.B);
    return (int)hipGetLastError();
}

extern "C" int segm_softmax_dice_bwd(const segm_softmax_dice_args* a) {
    SdDev P;
    bool vec = false;
    const int rc = sd_setup(a, P, vec);
    if (rc != SEGM_OK) return rc;
    if (!a->dlogits || !a->g_i || !a->g_p || !a->g_ce) return SEGM_E_NULL;
    const size_t esize = a->dtype == SEGM_F32 ? 4 : 2;
    if ((uintptr_t)a->dlogits % esize || (uintptr_t)a->g_i % sizeof(float) || (uintptr_t)a->g_p % sizeof(float) ||
        (uintptr_t)a->g_ce % sizeof(float)) return SEGM_E_SHAPE;
    vec = vec && (uintptr_t)a->dlogits % 16 == 0;
    P.dlogits = a->dlogits; P.g_i = a->g_i; P.g_p = a->g_p; P.g_ce = a->g_ce;
    const dim3 grid = loss_bwd_grid(P, vec, a->dtype);
    hipStream_t st = (hipStream_t)a->stream;
    SEGM_LOSS_LAUNCH(sd_bwd_kernel, a->dtype);
    return (int)hipGetLastError();
}
