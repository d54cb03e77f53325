// The intensity fingerprint of a CT case on the device: foreground count and sums, exact order statistics, rank-addressed gather
// (C ABI: segm_fg_workspace_bytes, segm_fg_count, segm_fg_order_stats, segm_fg_gather).
//
// Replaces what the reference's `DefaultPreprocessor.collect_foreground_intensities` does on the host with numpy
// (light_training/preprocessing/preprocessors/default_preprocessor.py:413-451): `foreground_mask = segmentation[0] > 0` (:431),
// `images[i][foreground_mask]` (:434), `rs.choice(foreground_pixels, num_samples, replace=True)` (:439-440) and np.mean / np.median /
// np.min / np.max / np.percentile of the foreground values (:441-449).  The n-long compaction is never materialised: the foreground
// voxels are addressed by their rank in C order through per-segment counts.
//
// The logical volume is cut into segments of SEGM_FG_SEGMENT consecutive voxels (C order of (z, y, x), whatever the strides).
//   * fg_count_kernel    one workgroup per segment: its number of voxels with seg > 0 (a NaN is none) and, per channel, the fp64 sum
//                        of its foreground values, each to its own slot.
//   * fg_scan_kernel     one workgroup: the exclusive int64 offsets of the segments, the total n, and the channel sums added in a
//                        fixed order (thread t takes the slots t, t + 256, ..., then a fixed tree) - no floating-point atomics.
//   * fg_hist_kernel     radix selection on the order-preserving 32-bit key of the float bits (csrc/resample.hip's zoom_key), digits of
//                        12 + 10 + 10 bits.  Pass 0 counts the top digit of every foreground value of a channel; passes 1 and 2 count
//                        the next digit of the values whose upper digits equal the prefix of one of the ranks.  Ranks that share a
//                        prefix share a histogram (a value matches at most one of the distinct prefixes), so all ranks of a channel
//                        ride through the same three passes over the data.  Segments without foreground are skipped by their count.
//   * fg_select_kernel   one workgroup per channel between the passes: per rank the bin that holds it, which extends the prefix, and
//                        the rank's residual inside that bin; after the last pass the prefix is the key of the answer.  Nothing is
//                        read back between the passes.
//   * fg_gather_kernel   one wave per index: binary search of the segment in the offsets; every lane builds the 64-bit foreground
//                        word of its own 64 consecutive voxels of the segment (the ballot word of that stretch, without the cross-lane
//                        operation), a wave prefix sum of the popcounts finds the lane, six popcount steps find the bit.
//
// Same-address contention.  CT intensities are integers in a narrow range: after the 12-bit digit (sign, exponent, three mantissa
// bits) most lanes of a wave hold the same bin, and LDS atomics on one address are executed one lane after the other.  Chosen here:
// aggregation of equal keys before the LDS atomic, in two steps.  A thread owns four consecutive voxels and merges those that fall
// into the bin of its first foreground voxel; then the wave takes the bin of its first active lane, sums the merged counts of all
// lanes that hold that bin by shuffles, and the leader issues ONE LDS atomic for them.  Lanes with another bin issue their own.
// Privatised sub-histograms were not chosen: they cut conflicts between waves, not between the lanes of a wave, and eight rank
// histograms of 1024 bins already take 32 KB of LDS.  The workgroup's non-zero bins go to global memory by integer atomic add, so
// the flush is as sparse as the data are narrow.  Counts are integers: exact in any order, two calls are bit-equal.
// Vector-memory and LDS atomics only.  The CPU emulation build (SEGM_EMU) states the same atomics with the compiler's __atomic builtins.
// The key, the atomics and the aggregation live in csrc/radix_hist.h, which csrc/topk_ce.hip shares.
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include "radix_hist.h"      // the key, the integer atomics, the aggregation of equal bins: shared with csrc/topk_ce.hip

namespace segm {

constexpr int kFgSeg = SEGM_FG_SEGMENT;
constexpr int kFgMaxC = SEGM_PREP_MAX_CHANNELS;
constexpr int kFgMaxR = SEGM_FG_MAX_RANKS;
constexpr int kFgTopBits = 12, kFgLowBits = 10;
constexpr int kFgTopBins = 1 << kFgTopBits, kFgLowBins = 1 << kFgLowBits;
constexpr int kFgHistBins = kFgMaxR * kFgLowBins;   // per (pass, channel): 4096 bins of pass 0, or one 1024-bin histogram per rank
constexpr int kFgPasses = 3;
constexpr int kFgLaneVox = kFgSeg / kWave;          // the voxels of a segment one lane of the gather looks at
static_assert(kFgSeg == kBlock * 16 && kFgLaneVox == 64 && kFgTopBins <= kFgHistBins, "fingerprint geometry");
static_assert(kFgTopBits + 2 * kFgLowBits == 32, "the digits cover the key");

typedef uint32_t fg_raw4 __attribute__((ext_vector_type(4)));

struct FgSel { uint32_t prefix, resid, group, pad; };     // per (channel, rank), kept in the workspace between the passes

struct FgDev {
    const float* data;
    const void* seg;
    int64_t sc, sz, sy;
    int32_t C, H, W, seg_dtype;
    int32_t dense, dvec, svec;          // a channel is contiguous; data / seg take 16-byte packets
    int32_t nseg, R, pass;
    uint32_t nvox, hw;
    int64_t* offsets;                   // [nseg + 1]: counts, then exclusive offsets and the total
    double* part;                       // [channel][segment]
    uint32_t* hist;                     // [pass][channel][kFgHistBins]
    FgSel* sel;                         // [channel][kFgMaxR]
    int64_t* count;
    double* sums;
    float* out;
    const int64_t* idx;
    int64_t m, idx_sc;
    uint32_t ranks[kFgMaxR];
};

// element offset of logical voxel v inside a channel
__device__ __forceinline__ int64_t fg_data_off(const FgDev& P, uint32_t v) {
    if (P.dense) return (int64_t)v;
    const uint32_t z = v / P.hw, rem = v - z * P.hw, y = rem / (uint32_t)P.W, x = rem - y * (uint32_t)P.W;
    return (int64_t)z * P.sz + (int64_t)y * P.sy + x;
}

__device__ __forceinline__ bool fg_is(const FgDev& P, uint32_t v) {
    if (P.seg_dtype == SEGM_PREP_SEG_F32) return reinterpret_cast<const float*>(P.seg)[v] > 0.f;      // NaN: no
    if (P.seg_dtype == SEGM_PREP_SEG_U8) return reinterpret_cast<const uint8_t*>(P.seg)[v] > 0;
    return reinterpret_cast<const int16_t*>(P.seg)[v] > 0;
}

template <typename T> struct alignas(4 * sizeof(T)) FgQuad { T e[4]; };

// fg[k] for the voxels v .. v + 3 (v % 4 == 0); those at or beyond nvox are none
__device__ __forceinline__ void fg_is4(const FgDev& P, uint32_t v, bool fg[4]) {
    if (P.svec && v + 3 < P.nvox) {
        if (P.seg_dtype == SEGM_PREP_SEG_F32) {
            const FgQuad<float> q = *reinterpret_cast<const FgQuad<float>*>(reinterpret_cast<const float*>(P.seg) + v);
#pragma unroll
            for (int k = 0; k < 4; ++k) fg[k] = q.e[k] > 0.f;
        } else if (P.seg_dtype == SEGM_PREP_SEG_U8) {
            const FgQuad<uint8_t> q = *reinterpret_cast<const FgQuad<uint8_t>*>(reinterpret_cast<const uint8_t*>(P.seg) + v);
#pragma unroll
            for (int k = 0; k < 4; ++k) fg[k] = q.e[k] > 0;
        } else {
            const FgQuad<int16_t> q = *reinterpret_cast<const FgQuad<int16_t>*>(reinterpret_cast<const int16_t*>(P.seg) + v);
#pragma unroll
            for (int k = 0; k < 4; ++k) fg[k] = q.e[k] > 0;
        }
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) fg[k] = v + k < P.nvox && fg_is(P, v + k);
    }
}

// ---- count and sums per segment -----------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kBlock) fg_count_kernel(FgDev P) {
    __shared__ int32_t s_cnt[kWavesPerBlock];
    __shared__ double s_sum[kWavesPerBlock][kFgMaxC];
    const uint32_t s = blockIdx.x, base = s * (uint32_t)kFgSeg;
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    double acc[kFgMaxC];
#pragma unroll
    for (int c = 0; c < kFgMaxC; ++c) acc[c] = 0.0;
    int32_t cnt = 0;
    for (int j = 0; j < kFgSeg / kBlock; ++j) {
        const uint32_t v = base + (uint32_t)j * kBlock + threadIdx.x;     // below 2^31 + 4096: no wrap
        if (v < P.nvox && fg_is(P, v)) {
            ++cnt;
            const float* p = P.data + fg_data_off(P, v);
#pragma unroll
            for (int c = 0; c < kFgMaxC; ++c)
                if (c < P.C) acc[c] += (double)p[(int64_t)c * P.sc];
        }
    }
    const int32_t wc = fg_wave_sum(cnt);
    if (lane == 0) s_cnt[wave] = wc;
    __syncthreads();
    int32_t total = 0;
    for (int w = 0; w < kWavesPerBlock; ++w) total += s_cnt[w];
    if (threadIdx.x == 0) P.offsets[s] = (int64_t)total;
    if (total == 0) {                                 // uniform over the workgroup
        if ((int)threadIdx.x < P.C) P.part[(size_t)threadIdx.x * P.nseg + s] = 0.0;
        return;
    }
#pragma unroll
    for (int c = 0; c < kFgMaxC; ++c) {
        if (c < P.C) {
            const double t = fg_wave_sum(acc[c]);
            if (lane == 0) s_sum[wave][c] = t;
        }
    }
    __syncthreads();
    if ((int)threadIdx.x < P.C) {
        const int c = threadIdx.x;
        double t = s_sum[0][c];
        for (int w = 1; w < kWavesPerBlock; ++w) t += s_sum[w][c];
        P.part[(size_t)c * P.nseg + s] = t;
    }
}

// one workgroup: counts -> exclusive offsets (thread t owns a contiguous run of segments), then the channel sums in a fixed order
__global__ void __launch_bounds__(kBlock) fg_scan_kernel(FgDev P) {
    __shared__ long long s_run[kBlock];
    __shared__ double s_red[kBlock];
    const int per = (P.nseg + kBlock - 1) / kBlock;
    const int t0 = (int)threadIdx.x * per, b0 = t0 < P.nseg ? t0 : P.nseg, b1 = b0 + per < P.nseg ? b0 + per : P.nseg;
    long long mine = 0;
    for (int b = b0; b < b1; ++b) mine += P.offsets[b];
    s_run[threadIdx.x] = mine;
    __syncthreads();
    if (threadIdx.x == 0) {
        long long run = 0;
        for (int t = 0; t < kBlock; ++t) { const long long c = s_run[t]; s_run[t] = run; run += c; }
        P.offsets[P.nseg] = run;
        *P.count = run;
    }
    __syncthreads();
    long long run = s_run[threadIdx.x];
    for (int b = b0; b < b1; ++b) { const long long c = P.offsets[b]; P.offsets[b] = run; run += c; }
    for (int c = 0; c < P.C; ++c) {
        double t = 0.0;
        for (int b = threadIdx.x; b < P.nseg; b += kBlock) t += P.part[(size_t)c * P.nseg + b];
        s_red[threadIdx.x] = t;
        __syncthreads();
        for (int off = kBlock / 2; off >= 1; off >>= 1) {
            if ((int)threadIdx.x < off) s_red[threadIdx.x] += s_red[threadIdx.x + off];
            __syncthreads();
        }
        if (threadIdx.x == 0) P.sums[c] = s_red[0];
        __syncthreads();
    }
}

// ---- radix selection: a histogram pass ------------------------------------------------------------------------------------------------
// grid (segments, channels).  bin of a foreground value: pass 0 its top digit; later the next digit inside the histogram of the
// rank group whose prefix its upper digits equal, none if there is no such group.
__global__ void __launch_bounds__(kBlock) fg_hist_kernel(FgDev P) {
    __shared__ uint32_t s_hist[kFgHistBins];
    const uint32_t s = blockIdx.x;
    const int c = blockIdx.y;
    if (P.offsets[s + 1] == P.offsets[s]) return;     // no foreground in this segment: uniform over the workgroup
    const int nbins = P.pass == 0 ? kFgTopBins : P.R * kFgLowBins;
    for (int b = threadIdx.x; b < nbins; b += kBlock) s_hist[b] = 0;
    uint32_t prefix[kFgMaxR];
    bool lead[kFgMaxR];
#pragma unroll
    for (int r = 0; r < kFgMaxR; ++r) {
        const bool on = P.pass > 0 && r < P.R;
        const FgSel q = on ? P.sel[c * kFgMaxR + r] : FgSel{0u, 0u, 0u, 0u};
        prefix[r] = q.prefix;
        lead[r] = on && q.group == (uint32_t)r;
    }
    const int hi_shift = P.pass == 1 ? 32 - kFgTopBits : kFgLowBits;      // the bits below the prefix: 20, then 10
    const int lo_shift = P.pass == 1 ? kFgLowBits : 0;
    __syncthreads();
    const float* dc = P.data + (int64_t)c * P.sc;
    const int lane = threadIdx.x & (kWave - 1);
    for (int j = 0; j < kFgSeg / (4 * kBlock); ++j) {
        const uint32_t v = s * (uint32_t)kFgSeg + ((uint32_t)j * kBlock + threadIdx.x) * 4u;
        bool fg[4];
        fg_is4(P, v, fg);
        int32_t bin[4] = {-1, -1, -1, -1};
        if (fg[0] || fg[1] || fg[2] || fg[3]) {
            float x[4] = {0.f, 0.f, 0.f, 0.f};
            if (P.dvec && v + 3 < P.nvox) {
                const fg_raw4 q = *reinterpret_cast<const fg_raw4*>(dc + v);
#pragma unroll
                for (int k = 0; k < 4; ++k) x[k] = __uint_as_float(q[k]);
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (fg[k]) x[k] = dc[fg_data_off(P, v + k)];
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (!fg[k]) continue;
                const uint32_t key = fg_key(x[k]);
                if (P.pass == 0) {
                    bin[k] = (int32_t)(key >> (32 - kFgTopBits));
                } else {
                    const uint32_t hi = key >> hi_shift, digit = (key >> lo_shift) & (uint32_t)(kFgLowBins - 1);
#pragma unroll
                    for (int r = 0; r < kFgMaxR; ++r)
                        if (lead[r] && hi == prefix[r]) bin[k] = r * kFgLowBins + (int32_t)digit;
                }
            }
        }
        fg_hist_add4(s_hist, bin, lane);
    }
    __syncthreads();
    uint32_t* g = P.hist + ((size_t)P.pass * P.C + c) * kFgHistBins;
    for (int b = threadIdx.x; b < nbins; b += kBlock) {
        const uint32_t n = s_hist[b];
        if (n) fg_add_glb(g + b, n);
    }
}

// ---- radix selection: from the histograms of a pass to the longer prefixes ---------------------------------------------------------------
// one workgroup per channel; thread r < R walks the 256 partial sums of its group's histogram, then the bins of one partial
__global__ void __launch_bounds__(kBlock) fg_select_kernel(FgDev P) {
    __shared__ uint32_t s_h[kFgHistBins];
    __shared__ uint32_t s_part[kFgMaxR][kBlock];
    __shared__ uint32_t s_prefix[kFgMaxR];
    const int c = blockIdx.x;
    const uint32_t* g = P.hist + ((size_t)P.pass * P.C + c) * kFgHistBins;
    const int nb = P.pass == 0 ? kFgTopBins : kFgLowBins, ngroups = P.pass == 0 ? 1 : P.R, per = nb / kBlock;
    for (int b = threadIdx.x; b < ngroups * nb; b += kBlock) s_h[b] = g[b];
    __syncthreads();
    for (int q = 0; q < ngroups; ++q) {
        uint32_t t = 0;
        for (int b = 0; b < per; ++b) t += s_h[q * nb + (int)threadIdx.x * per + b];
        s_part[q][threadIdx.x] = t;
    }
    __syncthreads();
    const int r = threadIdx.x;
    FgSel mine = {0u, 0u, 0u, 0u};
    if (r < P.R) {
        if (P.pass > 0) mine = P.sel[c * kFgMaxR + r];
        const int q = P.pass == 0 ? 0 : (int)mine.group;
        uint32_t k = P.pass == 0 ? P.ranks[r] : mine.resid;
        int i = 0;
        while (i < kBlock - 1 && k >= s_part[q][i]) { k -= s_part[q][i]; ++i; }
        int b = i * per;
        while (b < i * per + per - 1 && k >= s_h[q * nb + b]) { k -= s_h[q * nb + b]; ++b; }
        mine.prefix = P.pass == 0 ? (uint32_t)b : ((mine.prefix << kFgLowBits) | (uint32_t)b);
        mine.resid = k;
        s_prefix[r] = mine.prefix;
    }
    __syncthreads();
    if (r < P.R) {
        int first = r;
        for (int o = r - 1; o >= 0; --o)
            if (s_prefix[o] == mine.prefix) first = o;
        mine.group = (uint32_t)first;
        P.sel[c * kFgMaxR + r] = mine;
        if (P.pass == kFgPasses - 1) P.out[c * kFgMaxR + r] = fg_unkey(mine.prefix);
    }
}

// ---- gather by foreground rank ----------------------------------------------------------------------------------------------------------
// the 64-bit foreground word of the voxels base .. base + 63 (those at or beyond nvox are none)
template <typename T> __device__ __forceinline__ unsigned long long fg_word(const T* seg, uint32_t base, uint32_t nvox, bool vec) {
    unsigned long long w = 0;
    constexpr int kPer = 16 / (int)sizeof(T);
    if (vec && base + (uint32_t)kFgLaneVox <= nvox) {
        for (int p = 0; p < kFgLaneVox / kPer; ++p) {
            const fg_raw4 q = *reinterpret_cast<const fg_raw4*>(seg + base + p * kPer);
            T e[kPer];
            memcpy(e, &q, 16);
#pragma unroll
            for (int k = 0; k < kPer; ++k) w |= (e[k] > (T)0 ? 1ull : 0ull) << (p * kPer + k);
        }
    } else {
        for (int k = 0; k < kFgLaneVox; ++k)
            if (base + (uint32_t)k < nvox && seg[base + k] > (T)0) w |= 1ull << k;
    }
    return w;
}

// the position of the k-th set bit (k < popcount(w)): six popcount steps
__device__ __forceinline__ int fg_nth_bit(unsigned long long w, int k) {
    int pos = 0;
#pragma unroll
    for (int width = 32; width >= 1; width >>= 1) {
        const unsigned long long field = (w >> pos) & ((1ull << width) - 1ull);
        const int n = __builtin_popcountll(field);
        if (k >= n) { k -= n; pos += width; }
    }
    return pos;
}

__global__ void __launch_bounds__(kBlock) fg_gather_kernel(FgDev P) {
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t w = (int64_t)blockIdx.x * kWavesPerBlock + threadIdx.x / kWave;
    const int64_t nwaves = P.idx_sc ? P.m * P.C : P.m;
    if (w >= nwaves) return;                          // whole waves
    const int64_t j = w % P.m;
    const int cc = (int)(w / P.m);
    const int64_t i = P.idx[(int64_t)cc * P.idx_sc + j];
    const int c0 = P.idx_sc ? cc : 0, c1 = P.idx_sc ? cc + 1 : P.C;
    if (i < 0 || i >= P.offsets[P.nseg]) {            // refused on the host where the host knows the index; never an access
        if (lane == 0)
            for (int c = c0; c < c1; ++c) P.out[(int64_t)c * P.m + j] = __uint_as_float(0x7fc00000u);
        return;
    }
    int lo = 0, hi = P.nseg;                          // offsets[lo] <= i < offsets[hi]
    while (hi - lo > 1) {
        const int mid = lo + (hi - lo) / 2;
        if (P.offsets[mid] <= i) lo = mid; else hi = mid;
    }
    const int k = (int)(i - P.offsets[lo]);
    const uint32_t base = (uint32_t)lo * (uint32_t)kFgSeg + (uint32_t)lane * (uint32_t)kFgLaneVox;
    unsigned long long word;
    if (P.seg_dtype == SEGM_PREP_SEG_F32) word = fg_word(reinterpret_cast<const float*>(P.seg), base, P.nvox, P.svec);
    else if (P.seg_dtype == SEGM_PREP_SEG_U8) word = fg_word(reinterpret_cast<const uint8_t*>(P.seg), base, P.nvox, P.svec);
    else word = fg_word(reinterpret_cast<const int16_t*>(P.seg), base, P.nvox, P.svec);
    const int n = __builtin_popcountll(word);
    int incl = n;
    for (int d = 1; d < kWave; d <<= 1) {
        const int t = __shfl(incl, lane >= d ? lane - d : lane);
        if (lane >= d) incl += t;
    }
    const int excl = incl - n;
    if (k >= excl && k < incl) {
        const int64_t off = fg_data_off(P, base + (uint32_t)fg_nth_bit(word, k - excl));
        for (int c = c0; c < c1; ++c) P.out[(int64_t)c * P.m + j] = P.data[(int64_t)c * P.sc + off];
    }
}

// ---- host ---------------------------------------------------------------------------------------------------------------------------
struct FgLayout { size_t offsets, part, hist, sel, total; };

static FgLayout fg_layout(int32_t channels, int64_t voxels) {
    const size_t nseg = (size_t)((voxels + kFgSeg - 1) / kFgSeg);
    FgLayout l;
    l.offsets = 0;
    l.part = l.offsets + (nseg + 1) * sizeof(int64_t);
    l.hist = l.part + (size_t)channels * nseg * sizeof(double);
    l.sel = l.hist + (size_t)kFgPasses * channels * kFgHistBins * sizeof(uint32_t);
    l.total = l.sel + (size_t)channels * kFgMaxR * sizeof(FgSel);
    return l;
}

// the checks the three entries share, and the geometry; 0 or a SEGM_E_* status
static int fg_setup(const segm_fg_args* a, FgDev& P) {
    if (!a) return SEGM_E_NULL;
    if (!a->data || !a->seg) return SEGM_E_NULL;
    if (a->channels < 1 || a->channels > SEGM_PREP_MAX_CHANNELS) return SEGM_E_SHAPE;
    if (a->depth <= 0 || a->height <= 0 || a->width <= 0) return SEGM_E_SHAPE;
    const int64_t voxels = (int64_t)a->depth * a->height * a->width;
    if ((int64_t)a->depth * a->height > SEGM_CCL_MAX_VOXELS || voxels > SEGM_CCL_MAX_VOXELS) return SEGM_E_SHAPE;
    if (a->stride_y < a->width || a->stride_z < 0 || a->stride_c < 0) return SEGM_E_SHAPE;
    if (a->seg_dtype < SEGM_PREP_SEG_F32 || a->seg_dtype > SEGM_PREP_SEG_I16) return SEGM_E_DTYPE;
    const int ssize = a->seg_dtype == SEGM_PREP_SEG_F32 ? 4 : a->seg_dtype == SEGM_PREP_SEG_I16 ? 2 : 1;
    if ((uintptr_t)a->data % sizeof(float) || (uintptr_t)a->seg % ssize) return SEGM_E_SHAPE;
    const FgLayout l = fg_layout(a->channels, voxels);
    if (!a->workspace || a->workspace_bytes < l.total || (uintptr_t)a->workspace % sizeof(double)) return SEGM_E_WORKSPACE;
    memset(&P, 0, sizeof(P));
    P.data = a->data; P.seg = a->seg;
    P.sc = a->stride_c; P.sz = a->stride_z; P.sy = a->stride_y;
    P.C = a->channels; P.H = a->height; P.W = a->width; P.seg_dtype = a->seg_dtype;
    P.nvox = (uint32_t)voxels;
    P.hw = (uint32_t)((int64_t)a->height * a->width);
    P.nseg = (int32_t)((voxels + kFgSeg - 1) / kFgSeg);
    P.dense = (a->height == 1 || a->stride_y == a->width) && (a->depth == 1 || a->stride_z == (int64_t)a->height * a->width);
    P.dvec = P.dense && a->stride_c % 4 == 0 && (uintptr_t)a->data % 16 == 0;
    P.svec = (uintptr_t)a->seg % 16 == 0;
    char* ws = (char*)a->workspace;
    P.offsets = (int64_t*)(ws + l.offsets);
    P.part = (double*)(ws + l.part);
    P.hist = (uint32_t*)(ws + l.hist);
    P.sel = (FgSel*)(ws + l.sel);
    return SEGM_OK;
}

}  // namespace segm

using namespace segm;

extern "C" size_t segm_fg_workspace_bytes(int32_t channels, int64_t voxels) {
    if (channels < 1 || channels > SEGM_PREP_MAX_CHANNELS || voxels <= 0 || voxels > SEGM_CCL_MAX_VOXELS) return 0;
    return fg_layout(channels, voxels).total;
}

extern "C" int segm_fg_count(const segm_fg_args* a) {
    FgDev P;
    const int rc = fg_setup(a, P);
    if (rc != SEGM_OK) return rc;
    if (!a->count || !a->sums) return SEGM_E_NULL;
    if ((uintptr_t)a->count % sizeof(int64_t) || (uintptr_t)a->sums % sizeof(double)) return SEGM_E_SHAPE;
    P.count = a->count; P.sums = a->sums;
    hipStream_t st = (hipStream_t)a->stream;
    hipLaunchKernelGGL(fg_count_kernel, dim3((unsigned)P.nseg), dim3(kBlock), 0, st, P);
    hipLaunchKernelGGL(fg_scan_kernel, dim3(1), dim3(kBlock), 0, st, P);
    return (int)hipGetLastError();
}

extern "C" int segm_fg_order_stats(const segm_fg_args* a) {
    FgDev P;
    const int rc = fg_setup(a, P);
    if (rc != SEGM_OK) return rc;
    if (!a->out) return SEGM_E_NULL;
    if ((uintptr_t)a->out % sizeof(float)) return SEGM_E_SHAPE;
    if (a->n_ranks < 1 || a->n_ranks > SEGM_FG_MAX_RANKS) return SEGM_E_SHAPE;
    if (a->n < 1 || a->n > (int64_t)P.nvox) return SEGM_E_SHAPE;
    for (int r = 0; r < a->n_ranks; ++r) {
        if (a->ranks[r] < 0 || a->ranks[r] >= a->n) return SEGM_E_SHAPE;
        P.ranks[r] = (uint32_t)a->ranks[r];
    }
    P.R = a->n_ranks; P.out = a->out;
    hipStream_t st = (hipStream_t)a->stream;
    if (hipMemsetAsync(P.hist, 0, (size_t)kFgPasses * P.C * kFgHistBins * sizeof(uint32_t), st) != hipSuccess) return (int)hipGetLastError();
    for (int pass = 0; pass < kFgPasses; ++pass) {
        P.pass = pass;
        hipLaunchKernelGGL(fg_hist_kernel, dim3((unsigned)P.nseg, (unsigned)P.C), dim3(kBlock), 0, st, P);
        hipLaunchKernelGGL(fg_select_kernel, dim3((unsigned)P.C), dim3(kBlock), 0, st, P);
    }
    return (int)hipGetLastError();
}

extern "C" int segm_fg_gather(const segm_fg_args* a) {
    FgDev P;
    const int rc = fg_setup(a, P);
    if (rc != SEGM_OK) return rc;
    if (!a->out || !a->idx) return SEGM_E_NULL;
    if ((uintptr_t)a->out % sizeof(float) || (uintptr_t)a->idx % sizeof(int64_t)) return SEGM_E_SHAPE;
    if (a->n_idx < 1 || a->n_idx > SEGM_FG_MAX_INDICES) return SEGM_E_SHAPE;
    if (a->idx_stride_c != 0 && a->idx_stride_c < a->n_idx) return SEGM_E_SHAPE;
    if (a->n < 1 || a->n > (int64_t)P.nvox) return SEGM_E_SHAPE;
    P.out = a->out; P.idx = a->idx; P.m = a->n_idx; P.idx_sc = a->idx_stride_c;
    const int64_t nwaves = P.idx_sc ? P.m * P.C : P.m;
    hipStream_t st = (hipStream_t)a->stream;
    hipLaunchKernelGGL(fg_gather_kernel, dim3((unsigned)((nwaves + kWavesPerBlock - 1) / kWavesPerBlock)), dim3(kBlock), 0, st, P);
    return (int)hipGetLastError();
}
