// Surface-distance statistics without a distance list (C ABI: segm_border_stats, segm_border_stats_workspace_bytes).
//
// medpy's asd / assd / hd / hd95 and the surface Dice are all functions of the list `distance_transform_edt(~border(B))[border(A)]`
// (light_training/evaluation/metric.py:314-383 calls them per region): its length, its sum, its maximum, the number of entries
// within a tolerance, and two order statistics of the list joined with its mirror.  segm_border_distances writes the list and the
// host sorts it; here the same values d = sqrtf((float)edt[plane][v]) at the set voxels of a border plane are only counted:
//   * bstat_pass_kernel    grid (workgroups, items), one digit pass of an 8-bit radix selection over the border bytes of one item.
//                          A thread takes 16-byte packets of border bytes, four in flight per step, and touches `edt` only where
//                          the item's bit is set (borders are under 1 % of the voxels); a wave whose packets of a row are all
//                          clear goes on after one ballot.
//                          Pass 0 also forms the item row: count, fp64 sum, maximum and within-tolerance count, thread -> wave ->
//                          LDS -> one slot per (item, workgroup).  Every pass counts a digit of the 32-bit key of the squared value
//                          (the int32 itself, or the bits of a non-negative fp32: both orders are the order of d, sqrtf and the
//                          conversion being monotone) in an LDS histogram per rank, aggregated within the wave before the LDS
//                          atomic (radix_hist.h), and adds the non-zero bins to the group's histogram in the workspace.
//   * bstat_select_kernel  one workgroup between the passes: per (group, rank) the bin that holds the rank, which extends the prefix,
//                          and the residual rank inside the bin (csrc/fingerprint.hip's scheme, nothing is read back in between).
//                          The two ranks of a group share a histogram while their prefixes are equal.  After the last pass the prefix
//                          is the key of the answer, rooted as the list's entries are.
//   * bstat_finish_kernel  one workgroup per item: its slots added in a fixed order (thread t takes t, t + 256, ..., then a fixed
//                          tree) -> the item row.
// Integer atomics on histograms only, whose order does not matter; no floating-point atomics: two calls are bit-equal.
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include "radix_hist.h"

namespace segm {

constexpr int kBsItems = SEGM_METRICS_MAX_PLANES;   // items and groups per call
constexpr int kBsVox = 16;                          // border bytes per thread and step: one 16-byte packet
constexpr int kBsChunk = kBlock * kBsVox;           // voxels per workgroup and packet row
constexpr int kBsUnroll = 4;                        // packet rows per step: four independent 16-byte loads in flight per thread
constexpr int kBsMaxBlocks = 512;                   // workgroups per item: the rest of the volume by grid stride
constexpr int kBsBins = 256, kBsPasses = 4;         // 8-bit digits of the 32-bit key
constexpr int kBsHist = 2 * kBsBins;                // per (pass, group): one histogram per rank
static_assert(kBsPasses * 8 == 32 && kBsBins == kBlock, "the digits cover the key; a thread per bin");

typedef uint32_t bs_raw4 __attribute__((ext_vector_type(4)));

struct BsSel { uint32_t prefix, resid, hist, valid; };     // per (group, rank), kept in the workspace between the passes

struct BsDev {
    const uint8_t* borders;    // (volumes, N)
    const void* edt;           // (planes, N)
    double* out;
    double* psum;              // [item][workgroup]
    uint32_t* pcnt;            // [item][workgroup]
    uint32_t* pwithin;         // [item][workgroup]
    uint32_t* pmax;            // [item][workgroup]: the largest key
    uint32_t* hist;            // [pass][group][rank][bin]
    BsSel* sel;                // [group][rank]
    uint32_t N;
    int32_t nblocks, nsteps, is_float, n_items, n_groups, pass;
    int32_t bvol[kBsItems], bbit[kBsItems], eplane[kBsItems], group[kBsItems];
    float tol[kBsItems];
    int64_t rank[kBsItems][2];
};

// d of a key: the value segm_border_distances writes for the same voxel
__device__ __forceinline__ float bs_root(uint32_t key, int is_float) {
    return __builtin_sqrtf(is_float ? __uint_as_float(key) : (float)(int32_t)key);
}

// the border bytes of the voxels v .. v + 15, 0 for those outside the volume
__device__ __forceinline__ bs_raw4 bs_load16(const uint8_t* b, uint32_t v, uint32_t N, bool vec) {
    bs_raw4 q = {0u, 0u, 0u, 0u};
    if (v >= N) return q;
    if (vec && v + (uint32_t)kBsVox <= N) return *reinterpret_cast<const bs_raw4*>(b + v);
#pragma unroll
    for (int k = 0; k < kBsVox; ++k)
        if (v + (uint32_t)k < N) q[k >> 2] |= (uint32_t)b[v + k] << (8 * (k & 3));
    return q;
}

// bit k of the result: byte k of the packet has `bit` set
__device__ __forceinline__ uint32_t bs_bits16(bs_raw4 q, uint32_t bit) {
    if (((q[0] | q[1] | q[2] | q[3]) & (bit * 0x01010101u)) == 0) return 0;
    uint32_t set = 0;
#pragma unroll
    for (int k = 0; k < kBsVox; ++k) set |= (((q[k >> 2] >> (8 * (k & 3))) & bit) ? 1u : 0u) << k;
    return set;
}

__global__ void __launch_bounds__(kBlock) bstat_pass_kernel(BsDev P) {
    __shared__ uint32_t s_hist[kBsHist];
    __shared__ double s_sum[kWavesPerBlock];
    __shared__ uint32_t s_cnt[kWavesPerBlock], s_within[kWavesPerBlock], s_max[kWavesPerBlock];
    const int item = blockIdx.y, g = P.group[item];
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    uint32_t prefix[2] = {0u, 0u};
    bool lead[2] = {P.pass == 0, false};
    if (P.pass > 0) {
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const BsSel q = P.sel[2 * g + r];
            prefix[r] = q.prefix;
            lead[r] = q.valid && q.hist == (uint32_t)r;
        }
        if (!lead[0] && !lead[1]) return;             // no rank of this group is asked for: uniform over the workgroup
    }
    for (int b = threadIdx.x; b < kBsHist; b += kBlock) s_hist[b] = 0;
    __syncthreads();
    const uint8_t* bord = P.borders + (size_t)P.bvol[item] * P.N;
    const bool vec = (uintptr_t)bord % 16 == 0;
    const uint32_t bit = 1u << P.bbit[item];
    const size_t e0 = (size_t)P.eplane[item] * P.N;
    const uint32_t* keys = reinterpret_cast<const uint32_t*>(P.edt) + e0;
    const int hi_shift = 32 - 8 * P.pass, lo_shift = 24 - 8 * P.pass;       // pass > 0: the bits of the prefix, then the digit
    const float tol = P.tol[item];
    double sum = 0.0;
    uint32_t cnt = 0, within = 0, kmax = 0;
    for (int c = blockIdx.x; c < P.nsteps; c += P.nblocks) {                // the same trip count for every thread
        const uint32_t v0 = (uint32_t)c * (uint32_t)(kBsUnroll * kBsChunk) + threadIdx.x * (uint32_t)kBsVox;      // < 2^30 + 2^15
        bs_raw4 packet[kBsUnroll];
#pragma unroll
        for (int u = 0; u < kBsUnroll; ++u) packet[u] = bs_load16(bord, v0 + (uint32_t)u * (uint32_t)kBsChunk, P.N, vec);
#pragma unroll
        for (int u = 0; u < kBsUnroll; ++u) {
            const uint32_t set = bs_bits16(packet[u], bit), v = v0 + (uint32_t)u * (uint32_t)kBsChunk;
            if (__ballot(set != 0) == 0) continue;    // nothing of this item in the wave's 1024 voxels: `edt` is not touched
#pragma unroll
            for (int q4 = 0; q4 < kBsVox / 4; ++q4) {
                int32_t bin[4] = {-1, -1, -1, -1};
#pragma unroll
                for (int k4 = 0; k4 < 4; ++k4) {
                    const int k = 4 * q4 + k4;
                    if (!((set >> k) & 1u)) continue;
                    const uint32_t key = keys[v + k];
                    if (P.pass == 0) {
                        const float d = bs_root(key, P.is_float);
                        ++cnt;
                        sum += (double)d;
                        kmax = key > kmax ? key : kmax;
                        within += d <= tol ? 1u : 0u;
                        bin[k4] = (int32_t)(key >> 24);
                    } else {
                        const uint32_t hi = key >> hi_shift, digit = (key >> lo_shift) & (uint32_t)(kBsBins - 1);
#pragma unroll
                        for (int r = 0; r < 2; ++r)
                            if (lead[r] && hi == prefix[r]) bin[k4] = r * kBsBins + (int32_t)digit;
                    }
                }
                fg_hist_add4(s_hist, bin, lane);
            }
        }
    }
    __syncthreads();
    uint32_t* gh = P.hist + ((size_t)P.pass * kBsItems + g) * kBsHist;
    for (int b = threadIdx.x; b < kBsHist; b += kBlock) {
        const uint32_t n = s_hist[b];
        if (n) fg_add_glb(gh + b, n);
    }
    if (P.pass != 0) return;
    // the item row of this workgroup: thread -> wave -> LDS -> one slot
    sum = fg_wave_sum(sum);
    cnt = fg_wave_sum(cnt);
    within = fg_wave_sum(within);
    for (int off = kWave / 2; off >= 1; off >>= 1) {
        const uint32_t o = __shfl_xor(kmax, off);
        kmax = o > kmax ? o : kmax;
    }
    if (lane == 0) { s_sum[wave] = sum; s_cnt[wave] = cnt; s_within[wave] = within; s_max[wave] = kmax; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = s_sum[0];
        uint32_t n = s_cnt[0], w = s_within[0], m = s_max[0];
        for (int wv = 1; wv < kWavesPerBlock; ++wv) {
            t += s_sum[wv]; n += s_cnt[wv]; w += s_within[wv];
            m = s_max[wv] > m ? s_max[wv] : m;
        }
        const size_t slot = (size_t)item * P.nblocks + blockIdx.x;
        P.psum[slot] = t; P.pcnt[slot] = n; P.pwithin[slot] = w; P.pmax[slot] = m;
    }
}

// one workgroup; thread 2 g + r walks the 256 bins of the histogram of rank r of group g
__global__ void __launch_bounds__(kBlock) bstat_select_kernel(BsDev P) {
    __shared__ uint32_t s_prefix[2 * kBsItems], s_valid[2 * kBsItems];
    const int t = threadIdx.x, g = t >> 1, r = t & 1;
    const bool on = t < 2 * kBsItems && g < P.n_groups;
    BsSel mine = {0u, 0u, 0u, 0u};
    if (on) {
        if (P.pass > 0) mine = P.sel[t];
        const uint32_t* h = P.hist + ((size_t)P.pass * kBsItems + g) * kBsHist + (size_t)(P.pass == 0 ? 0u : mine.hist) * kBsBins;
        if (P.pass == 0) {                            // the group's count is the total of its first histogram
            uint64_t n = 0;
            for (int b = 0; b < kBsBins; ++b) n += h[b];
            const int64_t k = P.rank[g][r];
            mine.valid = k >= 0 && (uint64_t)k < n;
            mine.resid = mine.valid ? (uint32_t)k : 0u;
        }
        if (mine.valid) {
            uint32_t k = mine.resid;
            int b = 0;
            while (b < kBsBins - 1 && k >= h[b]) { k -= h[b]; ++b; }
            mine.prefix = (mine.prefix << 8) | (uint32_t)b;
            mine.resid = k;
        }
    }
    if (t < 2 * kBsItems) { s_prefix[t] = mine.prefix; s_valid[t] = mine.valid; }
    __syncthreads();
    if (!on) return;
    // rank 1 rides in the histogram of rank 0 while both have one prefix: a key then matches one histogram only
    mine.hist = (r == 1 && !(s_valid[t - 1] && s_prefix[t - 1] == mine.prefix)) ? 1u : 0u;
    P.sel[t] = mine;
    if (P.pass == kBsPasses - 1)
        P.out[4 * kBsItems + t] = mine.valid ? (double)bs_root(mine.prefix, P.is_float) : (double)__uint_as_float(0x7fc00000u);
}

// one workgroup per item: its slots in a fixed order -> out[4 i ..]; the first also writes the rows that no item or group uses
__global__ void __launch_bounds__(kBlock) bstat_finish_kernel(BsDev P) {
    __shared__ double s_red[kBlock];
    __shared__ unsigned long long s_cnt[kBlock], s_within[kBlock];
    __shared__ uint32_t s_max[kBlock];
    const int t = threadIdx.x;
    {
        const int i = blockIdx.x;
        double sum = 0.0;
        unsigned long long cnt = 0, within = 0;
        uint32_t kmax = 0;
        for (int b = t; b < P.nblocks; b += kBlock) {
            const size_t slot = (size_t)i * P.nblocks + b;
            sum += P.psum[slot]; cnt += P.pcnt[slot]; within += P.pwithin[slot];
            kmax = P.pmax[slot] > kmax ? P.pmax[slot] : kmax;
        }
        s_red[t] = sum; s_cnt[t] = cnt; s_within[t] = within; s_max[t] = kmax;
        __syncthreads();
        for (int off = kBlock / 2; off >= 1; off >>= 1) {
            if (t < off) {
                s_red[t] += s_red[t + off]; s_cnt[t] += s_cnt[t + off]; s_within[t] += s_within[t + off];
                s_max[t] = s_max[t + off] > s_max[t] ? s_max[t + off] : s_max[t];
            }
            __syncthreads();
        }
        if (t == 0) {
            P.out[4 * i] = (double)s_cnt[0];
            P.out[4 * i + 1] = s_red[0];
            P.out[4 * i + 2] = s_cnt[0] ? (double)bs_root(s_max[0], P.is_float) : 0.0;
            P.out[4 * i + 3] = (double)s_within[0];
        }
    }
    if (blockIdx.x != 0) return;
    if (t >= 4 * P.n_items && t < 4 * kBsItems) P.out[t] = 0.0;
    if (t >= 2 * P.n_groups && t < 2 * kBsItems) P.out[4 * kBsItems + t] = (double)__uint_as_float(0x7fc00000u);
}

struct BsLayout { size_t psum, pcnt, pwithin, pmax, hist, sel, total; int32_t nblocks, nsteps; };

static BsLayout bs_layout(int64_t voxels, int32_t n_items) {
    BsLayout l;
    l.nsteps = (int32_t)((voxels + kBsUnroll * kBsChunk - 1) / (kBsUnroll * kBsChunk));
    l.nblocks = l.nsteps < kBsMaxBlocks ? l.nsteps : kBsMaxBlocks;
    const size_t slots = (size_t)n_items * l.nblocks;
    l.psum = 0;
    l.hist = l.psum + slots * sizeof(double);                               // hist and sel are adjacent: one memset
    l.sel = l.hist + (size_t)kBsPasses * kBsItems * kBsHist * sizeof(uint32_t);
    l.pcnt = l.sel + (size_t)2 * kBsItems * sizeof(BsSel);
    l.pwithin = l.pcnt + slots * sizeof(uint32_t);
    l.pmax = l.pwithin + slots * sizeof(uint32_t);
    l.total = l.pmax + slots * sizeof(uint32_t);
    return l;
}

}  // namespace segm

using namespace segm;

extern "C" size_t segm_border_stats_workspace_bytes(int64_t voxels, int32_t n_items) {
    if (voxels <= 0 || voxels > SEGM_METRICS_MAX_VOXELS || n_items <= 0 || n_items > SEGM_METRICS_MAX_PLANES) return 0;
    return bs_layout(voxels, n_items).total;
}

extern "C" int segm_border_stats(const segm_border_stats_args* a) {
    if (!a) return SEGM_E_NULL;
    if (!a->borders || !a->edt || !a->out) return SEGM_E_NULL;
    if (a->voxels <= 0 || a->voxels > SEGM_METRICS_MAX_VOXELS) return SEGM_E_SHAPE;
    if (a->n_items <= 0 || a->n_items > SEGM_METRICS_MAX_PLANES || a->n_groups <= 0 || a->n_groups > SEGM_METRICS_MAX_PLANES) return SEGM_E_SHAPE;
    if (a->n_volumes <= 0 || a->n_planes <= 0) return SEGM_E_SHAPE;
    if (a->fp32 != 0 && a->fp32 != 1) return SEGM_E_DTYPE;
    int per_group[kBsItems] = {0};
    for (int i = 0; i < a->n_items; ++i) {
        if (a->border_volume[i] < 0 || a->border_volume[i] >= a->n_volumes || a->border_bit[i] < 0 || a->border_bit[i] > 7) return SEGM_E_SHAPE;
        if (a->edt_plane[i] < 0 || a->edt_plane[i] >= a->n_planes) return SEGM_E_SHAPE;
        if (a->item_group[i] < 0 || a->item_group[i] >= a->n_groups) return SEGM_E_SHAPE;
        ++per_group[a->item_group[i]];
    }
    for (int g = 0; g < a->n_groups; ++g)             // a joined list holds fewer than 2^32 values: the histograms count in 32 bits
        if ((int64_t)per_group[g] * a->voxels >= (int64_t)1 << 32) return SEGM_E_SHAPE;
    if ((uintptr_t)a->edt % sizeof(uint32_t) || (uintptr_t)a->out % sizeof(double)) return SEGM_E_SHAPE;
    const BsLayout l = bs_layout(a->voxels, a->n_items);
    if (!a->workspace || a->workspace_bytes < l.total || (uintptr_t)a->workspace % sizeof(double)) return SEGM_E_WORKSPACE;
    BsDev P;
    memset(&P, 0, sizeof(P));
    char* ws = (char*)a->workspace;
    P.borders = a->borders; P.edt = a->edt; P.out = a->out;
    P.psum = (double*)(ws + l.psum); P.pcnt = (uint32_t*)(ws + l.pcnt); P.pwithin = (uint32_t*)(ws + l.pwithin);
    P.pmax = (uint32_t*)(ws + l.pmax); P.hist = (uint32_t*)(ws + l.hist); P.sel = (BsSel*)(ws + l.sel);
    P.N = (uint32_t)a->voxels; P.nblocks = l.nblocks; P.nsteps = l.nsteps; P.is_float = a->fp32;
    P.n_items = a->n_items; P.n_groups = a->n_groups;
    for (int i = 0; i < a->n_items; ++i) {
        P.bvol[i] = a->border_volume[i]; P.bbit[i] = a->border_bit[i]; P.eplane[i] = a->edt_plane[i];
        P.group[i] = a->item_group[i]; P.tol[i] = a->tolerance[i];
    }
    for (int g = 0; g < a->n_groups; ++g) { P.rank[g][0] = a->rank[g][0]; P.rank[g][1] = a->rank[g][1]; }
    hipStream_t st = (hipStream_t)a->stream;
    if (hipMemsetAsync(P.hist, 0, l.pcnt - l.hist, st) != hipSuccess) return (int)hipGetLastError();
    const dim3 grid((unsigned)l.nblocks, (unsigned)a->n_items), block(kBlock);
    for (int pass = 0; pass < kBsPasses; ++pass) {
        P.pass = pass;
        hipLaunchKernelGGL(bstat_pass_kernel, grid, block, 0, st, P);
        if (pass == 0) hipLaunchKernelGGL(bstat_finish_kernel, dim3((unsigned)a->n_items), block, 0, st, P);
        hipLaunchKernelGGL(bstat_select_kernel, dim3(1), block, 0, st, P);
    }
    return (int)hipGetLastError();
}
