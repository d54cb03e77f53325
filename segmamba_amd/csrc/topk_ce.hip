// nnU-Net's hard-example loss on the device: the per-voxel cross entropy, the exact k-th largest of its values, and a backward pass
// that scales every voxel on its own (C ABI: segm_cross_entropy_map, segm_topk_select, segm_topk_select_workspace_bytes,
// segm_cross_entropy_map_bwd).
//
// Replaces the reference's TopKLoss (light_training/loss/robust_ce_loss.py:19-32): `nn.CrossEntropyLoss(reduce=False)` on the logits
// (:29, in ATen an fp32 copy of the logits, log-softmax and NLL), `torch.topk(res.view(-1), int(num_voxels * k / 100))` (:31, a sort on
// the device) and `res.mean()` (:32) with their backward.
//
//   * ce_map_kernel        one thread per voxel, the softmax of trainstep.hip's cross_entropy_kernel: loss = logsumexp - x[label],
//                          0 at an ignored voxel, NaN at a label outside [0, classes) that is not ignored.  4 bytes per voxel out.
//   * tk_hist_kernel       radix selection on the order-preserving key of the float bits (radix_hist.h), digits of 12 + 10 + 10 bits
//                          as in fingerprint.hip.  Pass 0 counts the top digit of every value, passes 1 and 2 the next digit of the
//                          values whose upper digits equal the prefix found so far.  Histogram in LDS, equal bins of a thread and of
//                          a wave merged before the atomic (ignored voxels put a large share of exact zeros into one bin), only
//                          non-zero bins added to global memory.  A fixed number of workgroups walks the segments.
//   * tk_select_kernel     one workgroup between the passes: the bin that holds the rank (counted from the LARGEST value), which
//                          extends the prefix, and the rank's residual inside that bin.  Nothing is read back between the passes.
//   * tk_sum_kernel        the last pass: per workgroup the number of keys above and equal to the threshold's and the fp64 sum of
//                          the values above, each to its own slot.
//   * tk_finish_kernel     one workgroup adds the slots in a fixed order and writes the 32-byte result.
//   * ce_map_bwd_kernel    one thread per voxel: the softmax again (the forward keeps only the map), times g_v.
// Integer atomics only, no floating-point atomic; sums in a fixed order: two calls of every entry are bit-equal.
#include <math.h>
#include <string.h>

#include "radix_hist.h"

namespace segm {

constexpr int kTkMaxC = 16;
constexpr int kTkSeg = kBlock * 16;                  // values a workgroup takes per step: 4 per thread, four times
constexpr int kTkMaxWg = 1024;                       // workgroups of a pass over the values; each walks the segments w, w + nwg, ...
constexpr int kTkTopBits = 12, kTkLowBits = 10;
constexpr int kTkTopBins = 1 << kTkTopBits, kTkLowBins = 1 << kTkLowBits;
constexpr int kTkPasses = 3;
static_assert(kTkTopBits + 2 * kTkLowBits == 32, "the digits cover the key");
static_assert(kTkTopBins % kBlock == 0 && kTkLowBins % kBlock == 0, "a thread of the select kernel owns whole bins");

typedef uint32_t tk_raw4 __attribute__((ext_vector_type(4)));

struct TkSel { uint32_t prefix, resid; };            // kept in the workspace between the passes
struct TkPart { double sum; uint32_t n_gt, n_eq; };  // per workgroup of the last pass
struct TkResult { float threshold; int32_t pad; int64_t n_gt, n_eq; double sum_gt; };
static_assert(sizeof(TkResult) == SEGM_TOPK_RESULT_BYTES && sizeof(TkPart) == 16, "the result is 32 bytes");

struct TkDev {
    const float* values;
    uint32_t n, rank;                                // rank = kk - 1, counted from the largest value
    int32_t nseg, nwg, pass, vec;
    uint32_t* hist;                                  // [pass][kTkTopBins]
    TkSel* sel;
    TkPart* part;                                    // [nwg]
    TkResult* result;
};

// ---- the per-voxel softmax ----------------------------------------------------------------------------------------------------------
struct CeMapDev {
    const void* logits;
    const int64_t* labels;
    void* dlogits;
    float* map;                                      // forward: out
    const float* coef;                               // backward, each optional
    const float* scale;
    const float* loss_map;
    const TkResult* select;
    int64_t kk;
    int64_t spatial, total;
    int32_t classes;
    int64_t ignore_index;
};

// exp(x[c] - max) into xv[], their sum, and x[label] - max (0 if the label names no class)
template <typename T>
__device__ __forceinline__ void ce_softmax(const T* x, int64_t spatial, int classes, int64_t lab, float xv[kTkMaxC], float& se, float& xl) {
    float mx = -3.0e38f;
#pragma unroll
    for (int c = 0; c < kTkMaxC; ++c) {
        if (c < classes) {
            xv[c] = to_f32(x[(int64_t)c * spatial]);
            mx = fmaxf(mx, xv[c]);
        }
    }
    se = 0.f; xl = 0.f;
#pragma unroll
    for (int c = 0; c < kTkMaxC; ++c) {
        if (c < classes) {
            const float sh = xv[c] - mx;
            if ((int64_t)c == lab) xl = sh;
            xv[c] = fast_exp(sh);
            se += xv[c];
        }
    }
}

template <typename T>
__global__ void __launch_bounds__(kBlock) ce_map_kernel(CeMapDev P) {
    const int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (v >= P.total) return;
    const int64_t b = v / P.spatial, s = v - b * P.spatial;
    const int64_t lab = P.labels[v];
    float loss = 0.f;
    if (lab != P.ignore_index) {
        // a label outside [0, classes) that is not ignored is a caller error: NaN, as in segm_cross_entropy - wrong labels stay loud
        if (lab < 0 || lab >= (int64_t)P.classes) {
            loss = __builtin_nanf("");
        } else {
            float xv[kTkMaxC], se, xl;
            ce_softmax(reinterpret_cast<const T*>(P.logits) + b * P.classes * P.spatial + s, P.spatial, P.classes, lab, xv, se, xl);
            loss = fast_log(se) - xl;                // logsumexp - x[label]
        }
    }
    P.map[v] = loss;
}

template <typename T>
__global__ void __launch_bounds__(kBlock) ce_map_bwd_kernel(CeMapDev P) {
    const int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (v >= P.total) return;
    const int64_t b = v / P.spatial, s = v - b * P.spatial;
    T* d = reinterpret_cast<T*>(P.dlogits) + b * P.classes * P.spatial + s;
    const int64_t lab = P.labels[v];
    if (lab == P.ignore_index) {
#pragma unroll
        for (int c = 0; c < kTkMaxC; ++c)
            if (c < P.classes) d[(int64_t)c * P.spatial] = from_f32<T>(0.f);
        return;
    }
    float g = 1.f;
    if (P.coef) g *= P.coef[v];
    if (P.scale) g *= P.scale[0];
    if (P.select) {
        // the top-k weight: 1 / kk above the threshold, the tied voxels share what is left of the kk, 0 below
        const TkResult r = *P.select;
        const uint32_t key = fg_key(P.loss_map[v]), tk = fg_key(r.threshold);
        const double kk = (double)P.kk;
        const float above = (float)(1.0 / kk), tied = (float)(((double)(P.kk - r.n_gt)) / ((double)r.n_eq * kk));
        g *= key > tk ? above : key == tk ? tied : 0.f;
    }
    const bool oob = lab < 0 || lab >= (int64_t)P.classes;
    float xv[kTkMaxC], se, xl;
    ce_softmax(reinterpret_cast<const T*>(P.logits) + b * P.classes * P.spatial + s, P.spatial, P.classes, lab, xv, se, xl);
    const float inv = oob ? __builtin_nanf("") : 1.f / se;
#pragma unroll
    for (int c = 0; c < kTkMaxC; ++c) {
        if (c < P.classes) {
            const float pr = xv[c] * inv;
            d[(int64_t)c * P.spatial] = from_f32<T>(g * (pr - ((int64_t)c == lab ? 1.f : 0.f)));
        }
    }
}

// ---- radix selection ----------------------------------------------------------------------------------------------------------------
// the four values at e .. e + 3 (e % 4 == 0) of the segment walk; on[k] tells which exist
__device__ __forceinline__ void tk_load4(const TkDev& P, uint32_t e, float x[4], bool on[4]) {
    if (P.vec && e + 3 < P.n) {
        const tk_raw4 q = *reinterpret_cast<const tk_raw4*>(P.values + e);
#pragma unroll
        for (int k = 0; k < 4; ++k) { x[k] = __uint_as_float(q[k]); on[k] = true; }
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            on[k] = e + (uint32_t)k < P.n;
            x[k] = on[k] ? P.values[e + k] : 0.f;
        }
    }
}

__global__ void __launch_bounds__(kBlock) tk_hist_kernel(TkDev P) {
    __shared__ uint32_t s_hist[kTkTopBins];
    const int nbins = P.pass == 0 ? kTkTopBins : kTkLowBins;
    for (int b = threadIdx.x; b < nbins; b += kBlock) s_hist[b] = 0;
    const uint32_t prefix = P.pass == 0 ? 0u : P.sel->prefix;
    const int hi_shift = P.pass == 1 ? 32 - kTkTopBits : kTkLowBits;      // the bits below the prefix: 20, then 10
    const int lo_shift = P.pass == 1 ? kTkLowBits : 0;
    __syncthreads();
    const int lane = threadIdx.x & (kWave - 1);
    for (int seg = blockIdx.x; seg < P.nseg; seg += P.nwg) {               // uniform over the workgroup
        for (int j = 0; j < kTkSeg / (4 * kBlock); ++j) {
            const uint32_t e = (uint32_t)seg * (uint32_t)kTkSeg + ((uint32_t)j * kBlock + threadIdx.x) * 4u;   // below 2^31 + 4096
            float x[4];
            bool on[4];
            tk_load4(P, e, x, on);
            int32_t bin[4] = {-1, -1, -1, -1};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (!on[k]) continue;
                const uint32_t key = fg_key(x[k]);
                if (P.pass == 0) bin[k] = (int32_t)(key >> (32 - kTkTopBits));
                else if ((key >> hi_shift) == prefix) bin[k] = (int32_t)((key >> lo_shift) & (uint32_t)(kTkLowBins - 1));
            }
            fg_hist_add4(s_hist, bin, lane);
        }
    }
    __syncthreads();
    uint32_t* g = P.hist + (size_t)P.pass * kTkTopBins;
    for (int b = threadIdx.x; b < nbins; b += kBlock) {
        const uint32_t n = s_hist[b];
        if (n) fg_add_glb(g + b, n);
    }
}

// one workgroup: thread t sums the bins it owns, thread 0 walks the 256 partial sums from the top, then the bins of one partial
__global__ void __launch_bounds__(kBlock) tk_select_kernel(TkDev P) {
    __shared__ uint32_t s_h[kTkTopBins];
    __shared__ uint32_t s_part[kBlock];
    const uint32_t* g = P.hist + (size_t)P.pass * kTkTopBins;
    const int nb = P.pass == 0 ? kTkTopBins : kTkLowBins, per = nb / kBlock;
    for (int b = threadIdx.x; b < nb; b += kBlock) s_h[b] = g[b];
    __syncthreads();
    uint32_t t = 0;
    for (int b = 0; b < per; ++b) t += s_h[(int)threadIdx.x * per + b];
    s_part[threadIdx.x] = t;
    __syncthreads();
    if (threadIdx.x == 0) {
        TkSel mine = {0u, 0u};
        if (P.pass > 0) mine = *P.sel;
        uint32_t k = P.pass == 0 ? P.rank : mine.resid;
        int i = kBlock - 1;
        while (i > 0 && k >= s_part[i]) { k -= s_part[i]; --i; }
        int b = i * per + per - 1;
        while (b > i * per && k >= s_h[b]) { k -= s_h[b]; --b; }
        mine.prefix = P.pass == 0 ? (uint32_t)b : ((mine.prefix << kTkLowBits) | (uint32_t)b);
        mine.resid = k;
        *P.sel = mine;
    }
}

__global__ void __launch_bounds__(kBlock) tk_sum_kernel(TkDev P) {
    __shared__ double s_sum[kWavesPerBlock];
    __shared__ uint32_t s_cnt[2][kWavesPerBlock];
    const uint32_t tk = P.sel->prefix;
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    double acc = 0.0;
    uint32_t n_gt = 0, n_eq = 0;
    for (int seg = blockIdx.x; seg < P.nseg; seg += P.nwg) {
        for (int j = 0; j < kTkSeg / (4 * kBlock); ++j) {
            const uint32_t e = (uint32_t)seg * (uint32_t)kTkSeg + ((uint32_t)j * kBlock + threadIdx.x) * 4u;
            float x[4];
            bool on[4];
            tk_load4(P, e, x, on);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (!on[k]) continue;
                const uint32_t key = fg_key(x[k]);
                if (key > tk) { ++n_gt; acc += (double)x[k]; }
                else if (key == tk) ++n_eq;
            }
        }
    }
    acc = fg_wave_sum(acc);
    n_gt = fg_wave_sum(n_gt);
    n_eq = fg_wave_sum(n_eq);
    if (lane == 0) { s_sum[wave] = acc; s_cnt[0][wave] = n_gt; s_cnt[1][wave] = n_eq; }
    __syncthreads();
    if (threadIdx.x == 0) {
        TkPart p = {s_sum[0], s_cnt[0][0], s_cnt[1][0]};
        for (int w = 1; w < kWavesPerBlock; ++w) { p.sum += s_sum[w]; p.n_gt += s_cnt[0][w]; p.n_eq += s_cnt[1][w]; }
        P.part[blockIdx.x] = p;
    }
}

// one workgroup: thread t takes the slots t, t + 256, ..., then a fixed tree
__global__ void __launch_bounds__(kBlock) tk_finish_kernel(TkDev P) {
    __shared__ double s_sum[kBlock];
    __shared__ long long s_gt[kBlock], s_eq[kBlock];
    double acc = 0.0;
    long long gt = 0, eq = 0;
    for (int w = threadIdx.x; w < P.nwg; w += kBlock) {
        const TkPart p = P.part[w];
        acc += p.sum; gt += p.n_gt; eq += p.n_eq;
    }
    s_sum[threadIdx.x] = acc; s_gt[threadIdx.x] = gt; s_eq[threadIdx.x] = eq;
    __syncthreads();
    for (int off = kBlock / 2; off >= 1; off >>= 1) {
        if ((int)threadIdx.x < off) {
            s_sum[threadIdx.x] += s_sum[threadIdx.x + off];
            s_gt[threadIdx.x] += s_gt[threadIdx.x + off];
            s_eq[threadIdx.x] += s_eq[threadIdx.x + off];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        TkResult r;
        r.threshold = fg_unkey(P.sel->prefix);
        r.pad = 0;
        r.n_gt = s_gt[0]; r.n_eq = s_eq[0]; r.sum_gt = s_sum[0];
        *P.result = r;
    }
}

// ---- host ---------------------------------------------------------------------------------------------------------------------------
struct TkLayout { size_t hist, sel, part, total; };

static TkLayout tk_layout() {
    TkLayout l;
    l.hist = 0;
    l.sel = l.hist + (size_t)kTkPasses * kTkTopBins * sizeof(uint32_t);
    l.part = l.sel + 16;
    l.total = l.part + (size_t)kTkMaxWg * sizeof(TkPart);
    return l;
}

// the checks the map and its backward share; 0 or a SEGM_E_* status
static int ce_map_setup(const segm_cross_entropy_map_args* a, CeMapDev& P) {
    if (!a) return SEGM_E_NULL;
    if (a->batch <= 0 || a->spatial <= 0 || a->classes < 1 || a->classes > kTkMaxC) return SEGM_E_SHAPE;
    if (a->dtype != SEGM_F32 && a->dtype != SEGM_F16 && a->dtype != SEGM_BF16) return SEGM_E_DTYPE;
    if (!a->logits || !a->labels) return SEGM_E_NULL;
    const int64_t total = (int64_t)a->batch * a->spatial;
    if (a->spatial >= ((int64_t)1 << 31) || total >= ((int64_t)1 << 31)) return SEGM_E_SHAPE;
    const size_t esize = a->dtype == SEGM_F32 ? 4 : 2;
    if ((uintptr_t)a->logits % esize || (uintptr_t)a->labels % sizeof(int64_t)) return SEGM_E_SHAPE;
    memset(&P, 0, sizeof(P));
    P.logits = a->logits; P.labels = a->labels;
    P.spatial = a->spatial; P.total = total; P.classes = a->classes; P.ignore_index = a->ignore_index;
    return SEGM_OK;
}

}  // namespace segm

using namespace segm;

extern "C" int segm_cross_entropy_map(const segm_cross_entropy_map_args* a) {
    CeMapDev P;
    const int rc = ce_map_setup(a, P);
    if (rc != SEGM_OK) return rc;
    if (!a->loss_map) return SEGM_E_NULL;
    if ((uintptr_t)a->loss_map % sizeof(float)) return SEGM_E_SHAPE;
    P.map = a->loss_map;
    const dim3 grid((unsigned)((P.total + kBlock - 1) / kBlock));
    hipStream_t st = (hipStream_t)a->stream;
    if (a->dtype == SEGM_F32) hipLaunchKernelGGL((ce_map_kernel<float>), grid, dim3(kBlock), 0, st, P);
    else if (a->dtype == SEGM_F16) hipLaunchKernelGGL((ce_map_kernel<f16_t>), grid, dim3(kBlock), 0, st, P);
    else hipLaunchKernelGGL((ce_map_kernel<bf16_t>), grid, dim3(kBlock), 0, st, P);
    return (int)hipGetLastError();
}

extern "C" int segm_cross_entropy_map_bwd(const segm_cross_entropy_map_args* a) {
    CeMapDev P;
    const int rc = ce_map_setup(a, P);
    if (rc != SEGM_OK) return rc;
    if (!a->dlogits) return SEGM_E_NULL;
    if ((a->select != nullptr) != (a->loss_map != nullptr)) return SEGM_E_NULL;       // the top-k weight needs both
    if (a->select && (a->kk < 1 || a->kk > P.total)) return SEGM_E_SHAPE;
    const size_t esize = a->dtype == SEGM_F32 ? 4 : 2;
    if ((uintptr_t)a->dlogits % esize || (uintptr_t)a->coef % sizeof(float) || (uintptr_t)a->scale % sizeof(float) ||
        (uintptr_t)a->loss_map % sizeof(float) || (uintptr_t)a->select % sizeof(double)) return SEGM_E_SHAPE;
    P.dlogits = a->dlogits; P.coef = a->coef; P.scale = a->scale;
    P.loss_map = a->loss_map; P.select = (const TkResult*)a->select; P.kk = a->kk;
    const dim3 grid((unsigned)((P.total + kBlock - 1) / kBlock));
    hipStream_t st = (hipStream_t)a->stream;
    if (a->dtype == SEGM_F32) hipLaunchKernelGGL((ce_map_bwd_kernel<float>), grid, dim3(kBlock), 0, st, P);
    else if (a->dtype == SEGM_F16) hipLaunchKernelGGL((ce_map_bwd_kernel<f16_t>), grid, dim3(kBlock), 0, st, P);
    else hipLaunchKernelGGL((ce_map_bwd_kernel<bf16_t>), grid, dim3(kBlock), 0, st, P);
    return (int)hipGetLastError();
}

extern "C" size_t segm_topk_select_workspace_bytes(int64_t n) {
    if (n < 1 || n >= ((int64_t)1 << 31)) return 0;
    return tk_layout().total;
}

extern "C" int segm_topk_select(const segm_topk_select_args* a) {
    if (!a) return SEGM_E_NULL;
    if (!a->values || !a->result) return SEGM_E_NULL;
    if (a->n < 1 || a->n >= ((int64_t)1 << 31) || a->kk < 1 || a->kk > a->n) return SEGM_E_SHAPE;
    if ((uintptr_t)a->values % sizeof(float) || (uintptr_t)a->result % sizeof(double)) return SEGM_E_SHAPE;
    const TkLayout l = tk_layout();
    if (!a->workspace || a->workspace_bytes < l.total || (uintptr_t)a->workspace % sizeof(double)) return SEGM_E_WORKSPACE;
    TkDev P;
    memset(&P, 0, sizeof(P));
    P.values = a->values;
    P.n = (uint32_t)a->n;
    P.rank = (uint32_t)(a->kk - 1);
    P.nseg = (int32_t)((a->n + kTkSeg - 1) / kTkSeg);
    P.nwg = P.nseg < kTkMaxWg ? P.nseg : kTkMaxWg;
    P.vec = (uintptr_t)a->values % 16 == 0;
    char* ws = (char*)a->workspace;
    P.hist = (uint32_t*)(ws + l.hist);
    P.sel = (TkSel*)(ws + l.sel);
    P.part = (TkPart*)(ws + l.part);
    P.result = (TkResult*)a->result;
    hipStream_t st = (hipStream_t)a->stream;
    if (hipMemsetAsync(P.hist, 0, (size_t)kTkPasses * kTkTopBins * sizeof(uint32_t), st) != hipSuccess) return (int)hipGetLastError();
    for (int pass = 0; pass < kTkPasses; ++pass) {
        P.pass = pass;
        hipLaunchKernelGGL(tk_hist_kernel, dim3((unsigned)P.nwg), dim3(kBlock), 0, st, P);
        hipLaunchKernelGGL(tk_select_kernel, dim3(1), dim3(kBlock), 0, st, P);
    }
    hipLaunchKernelGGL(tk_sum_kernel, dim3((unsigned)P.nwg), dim3(kBlock), 0, st, P);
    hipLaunchKernelGGL(tk_finish_kernel, dim3(1), dim3(kBlock), 0, st, P);
    return (int)hipGetLastError();
}
