// Signed-distance and edge training targets on the device  (C ABI: segm_sdm_masks, segm_sdm_compose).
//
// Replaces light_training/dataloading/dataset_sdm_edge.py:33-85 (`get_edge_points`, `edge_3d`, `compute_sdf`) and the
// `seg_sdm = 1 - compute_sdf(seg) + seg_edge` of its `post` hook: per BraTS region two scipy distance transforms of the whole volume,
// a binary erosion and skimage's find_boundaries on the host - seconds per case, which is why the reference loads a file made offline.
// Here the two transforms are segm_edt_sq / segm_edt_sq_long on bit planes (csrc/metrics.hip, csrc/edt_long.hip, unchanged) and this
// file holds what stands around them:
//   * sdm_masks_kernel     grid (workgroups, volumes), one stencil pass over label volumes in their own dtype (uint8, int16, int64; a
//                          value outside 0 .. 255 is in no region): the 256-entry table turns a label into its region bits, and a voxel
//                          of a region is an EDGE voxel iff one of its six face neighbours is not in the region, outside the volume =
//                          not in the region (`img - binary_erosion(img)`, border_value 0), and a BOUNDARY voxel iff one of its face
//                          neighbours inside the volume is not (find_boundaries(mode='inner'): dilation != erosion under reflecting
//                          borders).  Consecutive lanes take consecutive x, neighbours in y and z come from the caches, as in
//                          seg_regions_kernel.  Region sizes as byte fields of a 64-bit word per thread (a thread sees 16 voxels),
//                          16-bit fields for the wave's sum, then one 64-bit integer atomic per region and workgroup.
//   * sdm_max_kernel       grid (workgroups, items): the largest pos^2 and neg^2 of a live item, thread -> wave -> LDS -> one 32-bit
//                          integer maximum per workgroup into a zeroed array.
//   * sdm_compose_kernel   grid (workgroups, items): sdf, sdm and edge per voxel in fp64, rounded to fp32 once.
// The last two read pos^2 only where the inside bit is set and neg^2 only where it is not (each is 0 elsewhere), in 16-byte packets
// where the item's pointers allow, voxel by voxel otherwise and in the tail; sdm_voxel is the one per-voxel function of both routes.
// Integer atomics on counts and maxima only, whose order does not matter; no floating-point atomics: two calls are bit-equal.
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include "segm_device.h"

namespace segm {

constexpr int kSdmVox = 16;                         // voxels per thread of the mask pass
constexpr int kSdmChunk = kBlock * kSdmVox;         // voxels per workgroup of the mask pass
constexpr int kSdmItems = SEGM_METRICS_MAX_PLANES;  // items per compose call, volumes per mask call
constexpr int kSdmMaxBlocks = 4096;                 // workgroups per item of the compose kernel: the rest by grid stride
constexpr int kSdmMaxBlocksMax = 256;               // of the maxima kernel: each ends in two atomics on the item's two words

#ifdef SEGM_EMU
static inline void sdm_add_u64(unsigned long long* p, unsigned long long v) { __atomic_fetch_add(p, v, __ATOMIC_RELAXED); }
static inline void sdm_max_u32(uint32_t* p, uint32_t v) {
    uint32_t old = __atomic_load_n(p, __ATOMIC_RELAXED);
    while (old < v && !__atomic_compare_exchange_n(p, &old, v, false, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) {}
}
#else
__device__ __forceinline__ void sdm_add_u64(unsigned long long* p, unsigned long long v) {
    __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void sdm_max_u32(uint32_t* p, uint32_t v) { __hip_atomic_fetch_max(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
#endif

// ---- region bits, edges, boundaries, sizes ------------------------------------------------------------------------------------------
struct SdmMaskDev {
    const void* labels;        // (n, N) of T
    const uint8_t* table;
    uint8_t* inside;           // (n, N) each
    uint8_t* outside;
    uint8_t* edge;
    uint8_t* boundary;
    unsigned long long* counts;    // [volume][8 regions], zeroed before the launch
    int32_t D, H, W;
    uint32_t N, all;           // all: the bits of the regions in use
};

// the region bits of a label; labels outside the table belong to no region
template <typename T> __device__ __forceinline__ uint32_t sdm_bits(const uint8_t* tab, T v) {
    const unsigned long long u = (unsigned long long)(long long)v;          // a negative label becomes a huge one
    return u < 256ull ? tab[u] : 0u;
}
template <> __device__ __forceinline__ uint32_t sdm_bits<uint8_t>(const uint8_t* tab, uint8_t v) { return tab[v]; }

// byte k of the result = bit k of m (m < 256)
__device__ __forceinline__ unsigned long long sdm_spread8(uint32_t m) {
    const unsigned long long x = ((unsigned long long)m * 0x0101010101010101ull) & 0x8040201008040201ull;
    return ((x + 0x7f7f7f7f7f7f7f7full) >> 7) & 0x0101010101010101ull;
}

template <typename T>
__global__ void __launch_bounds__(kBlock) sdm_masks_kernel(SdmMaskDev P) {
    __shared__ uint8_t s_tab[256];
    __shared__ unsigned long long s_red[kWavesPerBlock][2];
    const int tid = threadIdx.x;
    s_tab[tid] = (uint8_t)(P.table[tid] & P.all);
    __syncthreads();
    const size_t vo = (size_t)blockIdx.y * P.N;
    // the outputs alias neither the labels nor one another: the loads of the next voxels may pass the stores of this one
    const T* __restrict__ lab = reinterpret_cast<const T*>(P.labels) + vo;
    uint8_t* __restrict__ o_in = P.inside + vo;
    uint8_t* __restrict__ o_out = P.outside + vo;
    uint8_t* __restrict__ o_edge = P.edge + vo;
    uint8_t* __restrict__ o_bnd = P.boundary + vo;
    const uint32_t base = (uint32_t)blockIdx.x * kSdmChunk;
    const uint32_t W = (uint32_t)P.W, HW = (uint32_t)P.H * (uint32_t)P.W;
    unsigned long long acc = 0ull;
#pragma unroll 4
    for (int k = 0; k < kSdmVox; ++k) {
        const uint32_t idx = base + (uint32_t)k * kBlock + tid;               // < 2^30 + 2^12
        if (idx >= P.N) continue;
        const uint32_t p = sdm_bits<T>(s_tab, lab[idx]);
        uint32_t e = 0, b = 0;
        if (p) {
            const uint32_t z = idx / HW, rem = idx - z * HW, y = rem / W, x = rem - y * W;
            uint32_t pe = p, pb = p;                 // the regions whose six neighbours / whose neighbours in the volume are all inside
            if (x > 0) { const uint32_t n = sdm_bits<T>(s_tab, lab[idx - 1]); pe &= n; pb &= n; } else pe = 0;
            if (x + 1 < W) { const uint32_t n = sdm_bits<T>(s_tab, lab[idx + 1]); pe &= n; pb &= n; } else pe = 0;
            if (y > 0) { const uint32_t n = sdm_bits<T>(s_tab, lab[idx - W]); pe &= n; pb &= n; } else pe = 0;
            if (y + 1 < (uint32_t)P.H) { const uint32_t n = sdm_bits<T>(s_tab, lab[idx + W]); pe &= n; pb &= n; } else pe = 0;
            if (z > 0) { const uint32_t n = sdm_bits<T>(s_tab, lab[idx - HW]); pe &= n; pb &= n; } else pe = 0;
            if (z + 1 < (uint32_t)P.D) { const uint32_t n = sdm_bits<T>(s_tab, lab[idx + HW]); pe &= n; pb &= n; } else pe = 0;
            e = p & ~pe;
            b = p & ~pb;
            acc += sdm_spread8(p);
        }
        o_in[idx] = (uint8_t)p;
        o_out[idx] = (uint8_t)(~p & P.all);
        o_edge[idx] = (uint8_t)e;
        o_bnd[idx] = (uint8_t)b;
    }
    // byte fields (<= 16 each) -> 16-bit fields (a wave adds 64 of them: <= 1024)
    unsigned long long w[2] = {acc & 0x00ff00ff00ff00ffull, (acc >> 8) & 0x00ff00ff00ff00ffull};      // regions 0, 2, 4, 6 and 1, 3, 5, 7
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int m = kWave / 2; m >= 1; m >>= 1) w[i] += __shfl_xor(w[i], m);
    if ((tid & (kWave - 1)) == 0) { s_red[tid / kWave][0] = w[0]; s_red[tid / kWave][1] = w[1]; }
    __syncthreads();
    if (tid < SEGM_METRICS_MAX_REGIONS) {
        unsigned long long s = 0;
        for (int wv = 0; wv < kWavesPerBlock; ++wv) s += (s_red[wv][tid & 1] >> (16 * (tid >> 1))) & 0xffffull;
        if (s) sdm_add_u64(P.counts + (size_t)blockIdx.y * SEGM_METRICS_MAX_REGIONS + tid, s);
    }
}

// ---- maxima and the targets --------------------------------------------------------------------------------------------------------
typedef uint32_t sdm_u4 __attribute__((ext_vector_type(4)));
typedef float sdm_f4 __attribute__((ext_vector_type(4)));

struct SdmDev {
    const int32_t* edt;        // (planes, N)
    const uint8_t* inside;     // (volumes, N) each
    const uint8_t* edge;
    const uint8_t* boundary;
    const long long* counts;   // [volume][8]
    float* sdf;                // (out planes, N) each, nullable
    float* sdm;
    float* eout;
    uint32_t* maxima;          // [item][2]: Pmax^2, Nmax^2
    uint32_t N, nquads;
    int32_t vol[kSdmItems], bit[kSdmItems], pos[kSdmItems], neg[kSdmItems], outp[kSdmItems];
};

// Four voxels v .. v + 3 of an item (those past N are left out): bit k of `in` = voxel k is in the region; pos^2 is loaded where a
// voxel is inside and neg^2 where one is outside, 0 elsewhere (which is their value there).  PACKET: v + 4 <= N and every pointer
// is aligned to its packet.
template <bool PACKET>
__device__ __forceinline__ uint32_t sdm_load_quad(const uint8_t* in, const int32_t* pp, const int32_t* np, uint32_t bit, uint32_t v,
                                                  uint32_t N, int32_t pos[4], int32_t neg[4]) {
    uint32_t inb = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) { pos[k] = 0; neg[k] = 0; }
    if (PACKET) {
        const uint32_t word = *reinterpret_cast<const uint32_t*>(in + v);
#pragma unroll
        for (int k = 0; k < 4; ++k) inb |= ((word >> (8 * k + bit)) & 1u) << k;
        if (pp && inb != 0u) {
            const sdm_u4 q = *reinterpret_cast<const sdm_u4*>(pp + v);
#pragma unroll
            for (int k = 0; k < 4; ++k) pos[k] = (int32_t)q[k];
        }
        if (np && inb != 0xfu) {
            const sdm_u4 q = *reinterpret_cast<const sdm_u4*>(np + v);
#pragma unroll
            for (int k = 0; k < 4; ++k) neg[k] = (int32_t)q[k];
        }
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (v + (uint32_t)k >= N) continue;
            const uint32_t is_in = ((uint32_t)in[v + k] >> bit) & 1u;
            inb |= is_in << k;
            const int32_t* src = is_in ? pp : np;      // one load, then a select per plane: pos and neg stay in registers
            const int32_t d2 = src ? src[v + k] : 0;
            pos[k] = is_in ? d2 : 0;
            neg[k] = is_in ? 0 : d2;
        }
    }
    return inb;
}

// live = 0 < the region's size < N: both transforms have seeds, so neither maximum is 0 and neither plane holds the sentinel
__device__ __forceinline__ bool sdm_live(const SdmDev& P, int item) {
    const long long c = P.counts[(size_t)P.vol[item] * SEGM_METRICS_MAX_REGIONS + P.bit[item]];
    return c > 0 && c < (long long)P.N;
}

__global__ void __launch_bounds__(kBlock) sdm_max_kernel(SdmDev P) {
    __shared__ uint32_t s_max[kWavesPerBlock][2];
    const int item = blockIdx.y;
    if (!sdm_live(P, item)) return;                   // uniform over the workgroup: its transforms are not read
    const uint8_t* in = P.inside + (size_t)P.vol[item] * P.N;
    const int32_t* pp = P.edt + (size_t)P.pos[item] * P.N;
    const int32_t* np = P.edt + (size_t)P.neg[item] * P.N;
    const uint32_t bit = (uint32_t)P.bit[item];
    const bool vec = (uintptr_t)in % 4 == 0 && (uintptr_t)pp % 16 == 0 && (uintptr_t)np % 16 == 0;
    int32_t pm = 0, nm = 0;
#pragma unroll 2
    for (uint32_t q = blockIdx.x * (uint32_t)kBlock + threadIdx.x; q < P.nquads; q += gridDim.x * (uint32_t)kBlock) {
        const uint32_t v = 4u * q;                    // < 2^30
        int32_t pos[4], neg[4];
        if (vec && v + 4u <= P.N) sdm_load_quad<true>(in, pp, np, bit, v, P.N, pos, neg);
        else sdm_load_quad<false>(in, pp, np, bit, v, P.N, pos, neg);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            pm = pos[k] > pm ? pos[k] : pm;
            nm = neg[k] > nm ? neg[k] : nm;
        }
    }
    for (int off = kWave / 2; off >= 1; off >>= 1) {
        const int32_t a = __shfl_xor(pm, off), b = __shfl_xor(nm, off);
        pm = a > pm ? a : pm;
        nm = b > nm ? b : nm;
    }
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    if (lane == 0) { s_max[wave][0] = (uint32_t)pm; s_max[wave][1] = (uint32_t)nm; }
    __syncthreads();
    if (threadIdx.x < 2) {
        uint32_t m = 0;
        for (int wv = 0; wv < kWavesPerBlock; ++wv) m = s_max[wv][threadIdx.x] > m ? s_max[wv][threadIdx.x] : m;
        // every workgroup of an item meets at one address: only a value above what is already there goes out (a stale read of a
        // smaller value costs an atomic, never the result)
        uint32_t* slot = P.maxima + 2 * item + threadIdx.x;
        if (m > *reinterpret_cast<volatile uint32_t*>(slot)) sdm_max_u32(slot, m);
    }
}

// One voxel: rp = sqrt(Pmax^2), rn = sqrt(Nmax^2) in fp64.  sdf = -pos / Pmax inside, +neg / Nmax outside, 0 on the inner boundary and
// on a plane that is not live; sdm = 1 - sdf + edge.
__device__ __forceinline__ void sdm_voxel(bool live, bool in, bool bnd, bool edg, int32_t pos2, int32_t neg2, double rp, double rn,
                                          float* sdf, float* sdm, float* e) {
    double s = 0.0;
    if (live && !bnd) s = in ? -(sqrt((double)pos2) / rp) : sqrt((double)neg2) / rn;
    const double ed = edg ? 1.0 : 0.0;
    *sdf = (float)s;
    *sdm = (float)(1.0 - s + ed);
    *e = (float)ed;
}

// DIST = false: only the edge plane is asked for; no transform and no maximum is read
template <bool DIST>
__global__ void __launch_bounds__(kBlock) sdm_compose_kernel(SdmDev P) {
    const int item = blockIdx.y;
    const bool live = DIST && sdm_live(P, item);
    const size_t vo = (size_t)P.vol[item] * P.N, oo = (size_t)P.outp[item] * P.N;
    const uint8_t* in = P.inside + vo;
    const uint8_t* ed = P.edge + vo;
    const uint8_t* bd = P.boundary + vo;
    const int32_t* pp = live ? P.edt + (size_t)P.pos[item] * P.N : nullptr;
    const int32_t* np = live ? P.edt + (size_t)P.neg[item] * P.N : nullptr;
    float* o_sdf = P.sdf ? P.sdf + oo : nullptr;
    float* o_sdm = P.sdm ? P.sdm + oo : nullptr;
    float* o_e = P.eout ? P.eout + oo : nullptr;
    const uint32_t bit = (uint32_t)P.bit[item];
    const bool vec = (uintptr_t)in % 4 == 0 && (uintptr_t)ed % 4 == 0 && (uintptr_t)bd % 4 == 0 && (uintptr_t)pp % 16 == 0
                     && (uintptr_t)np % 16 == 0 && (uintptr_t)o_sdf % 16 == 0 && (uintptr_t)o_sdm % 16 == 0 && (uintptr_t)o_e % 16 == 0;
    double rp = 1.0, rn = 1.0;
    if (live) {
        rp = sqrt((double)P.maxima[2 * item]);
        rn = sqrt((double)P.maxima[2 * item + 1]);
    }
    for (uint32_t q = blockIdx.x * (uint32_t)kBlock + threadIdx.x; q < P.nquads; q += gridDim.x * (uint32_t)kBlock) {
        const uint32_t v = 4u * q;                    // < 2^30
        int32_t pos[4], neg[4];
        float f_sdf[4], f_sdm[4], f_e[4];
        if (vec && v + 4u <= P.N) {
            const uint32_t inb = sdm_load_quad<true>(in, pp, np, bit, v, P.N, pos, neg);
            const uint32_t we = *reinterpret_cast<const uint32_t*>(ed + v), wb = *reinterpret_cast<const uint32_t*>(bd + v);
#pragma unroll
            for (int k = 0; k < 4; ++k)
                sdm_voxel(live, (inb >> k) & 1u, (wb >> (8 * k + bit)) & 1u, (we >> (8 * k + bit)) & 1u, pos[k], neg[k], rp, rn,
                          &f_sdf[k], &f_sdm[k], &f_e[k]);
            if (o_sdf) *reinterpret_cast<sdm_f4*>(o_sdf + v) = sdm_f4{f_sdf[0], f_sdf[1], f_sdf[2], f_sdf[3]};
            if (o_sdm) *reinterpret_cast<sdm_f4*>(o_sdm + v) = sdm_f4{f_sdm[0], f_sdm[1], f_sdm[2], f_sdm[3]};
            if (o_e) *reinterpret_cast<sdm_f4*>(o_e + v) = sdm_f4{f_e[0], f_e[1], f_e[2], f_e[3]};
        } else {
            const uint32_t inb = sdm_load_quad<false>(in, pp, np, bit, v, P.N, pos, neg);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (v + (uint32_t)k >= P.N) continue;
                sdm_voxel(live, (inb >> k) & 1u, ((uint32_t)bd[v + k] >> bit) & 1u, ((uint32_t)ed[v + k] >> bit) & 1u, pos[k], neg[k], rp, rn,
                          &f_sdf[k], &f_sdm[k], &f_e[k]);
                if (o_sdf) o_sdf[v + k] = f_sdf[k];
                if (o_sdm) o_sdm[v + k] = f_sdm[k];
                if (o_e) o_e[v + k] = f_e[k];
            }
        }
    }
}

static inline bool sdm_volume_ok(int64_t d, int64_t h, int64_t w) {
    return d > 0 && h > 0 && w > 0 && d <= SEGM_EDT_LONG_MAX_LINE && h <= SEGM_EDT_LONG_MAX_LINE && w <= SEGM_EDT_LONG_MAX_LINE
           && d * h * w <= SEGM_METRICS_MAX_VOXELS;
}

}  // namespace segm

using namespace segm;

extern "C" int segm_sdm_masks(const segm_sdm_masks_args* a) {
    if (!a) return SEGM_E_NULL;
    if (!a->labels || !a->table || !a->inside || !a->outside || !a->edge || !a->boundary || !a->counts) return SEGM_E_NULL;
    if (!sdm_volume_ok(a->depth, a->height, a->width)) return SEGM_E_SHAPE;
    if (a->n <= 0 || a->n > kSdmItems || a->n_regions <= 0 || a->n_regions > SEGM_METRICS_MAX_REGIONS) return SEGM_E_SHAPE;
    if (a->label_dtype != SEGM_SDM_LABEL_U8 && a->label_dtype != SEGM_SDM_LABEL_I16 && a->label_dtype != SEGM_SDM_LABEL_I64) return SEGM_E_DTYPE;
    const size_t esize = a->label_dtype == SEGM_SDM_LABEL_U8 ? 1 : (a->label_dtype == SEGM_SDM_LABEL_I16 ? 2 : 8);
    if ((uintptr_t)a->labels % esize || (uintptr_t)a->counts % sizeof(int64_t)) return SEGM_E_SHAPE;
    const int64_t N = (int64_t)a->depth * a->height * a->width;
    SdmMaskDev P;
    memset(&P, 0, sizeof(P));
    P.labels = a->labels; P.table = a->table; P.inside = a->inside; P.outside = a->outside; P.edge = a->edge; P.boundary = a->boundary;
    P.counts = (unsigned long long*)a->counts;
    P.D = a->depth; P.H = a->height; P.W = a->width; P.N = (uint32_t)N; P.all = (1u << a->n_regions) - 1u;
    hipStream_t st = (hipStream_t)a->stream;
    if (hipMemsetAsync(a->counts, 0, (size_t)a->n * SEGM_METRICS_MAX_REGIONS * sizeof(int64_t), st) != hipSuccess) return (int)hipGetLastError();
    const dim3 grid((unsigned)((N + kSdmChunk - 1) / kSdmChunk), (unsigned)a->n), block(kBlock);
    if (a->label_dtype == SEGM_SDM_LABEL_U8) hipLaunchKernelGGL(sdm_masks_kernel<uint8_t>, grid, block, 0, st, P);
    else if (a->label_dtype == SEGM_SDM_LABEL_I16) hipLaunchKernelGGL(sdm_masks_kernel<int16_t>, grid, block, 0, st, P);
    else hipLaunchKernelGGL(sdm_masks_kernel<int64_t>, grid, block, 0, st, P);
    return (int)hipGetLastError();
}

extern "C" int segm_sdm_compose(const segm_sdm_compose_args* a) {
    if (!a) return SEGM_E_NULL;
    const bool dist = a->sdf || a->sdm;
    if (!dist && !a->edge_out) return SEGM_E_NULL;
    if (!a->inside || !a->edge || !a->boundary || !a->counts || (dist && !a->edt)) return SEGM_E_NULL;
    if (a->voxels <= 0 || a->voxels > SEGM_METRICS_MAX_VOXELS) return SEGM_E_SHAPE;
    if (a->n_items <= 0 || a->n_items > kSdmItems || a->n_volumes <= 0 || a->n_out_planes <= 0 || (dist && a->n_planes <= 0)) return SEGM_E_SHAPE;
    for (int i = 0; i < a->n_items; ++i) {
        if (a->volume[i] < 0 || a->volume[i] >= a->n_volumes || a->bit[i] < 0 || a->bit[i] >= SEGM_METRICS_MAX_REGIONS) return SEGM_E_SHAPE;
        if (dist && (a->pos_plane[i] < 0 || a->pos_plane[i] >= a->n_planes || a->neg_plane[i] < 0 || a->neg_plane[i] >= a->n_planes)) return SEGM_E_SHAPE;
        const int32_t o = a->out_plane[i];
        if (o < 0 || o >= a->n_out_planes) return SEGM_E_SHAPE;
        for (int j = 0; j < i; ++j)                   // two items of one call must not write one plane
            if (a->out_plane[j] == o) return SEGM_E_SHAPE;
    }
    if ((uintptr_t)a->edt % sizeof(int32_t) || (uintptr_t)a->sdf % sizeof(float) || (uintptr_t)a->sdm % sizeof(float)
        || (uintptr_t)a->edge_out % sizeof(float) || (uintptr_t)a->counts % sizeof(int64_t)) return SEGM_E_SHAPE;
    if (dist && (!a->workspace || a->workspace_bytes < SEGM_SDM_COMPOSE_WORKSPACE_BYTES || (uintptr_t)a->workspace % sizeof(uint32_t)))
        return SEGM_E_WORKSPACE;                      // the edge alone takes no maximum: its workspace is not looked at
    SdmDev P;
    memset(&P, 0, sizeof(P));
    P.edt = a->edt; P.inside = a->inside; P.edge = a->edge; P.boundary = a->boundary; P.counts = (const long long*)a->counts;
    P.sdf = a->sdf; P.sdm = a->sdm; P.eout = a->edge_out; P.maxima = (uint32_t*)a->workspace;
    P.N = (uint32_t)a->voxels; P.nquads = (uint32_t)((a->voxels + 3) / 4);
    for (int i = 0; i < a->n_items; ++i) {
        P.vol[i] = a->volume[i]; P.bit[i] = a->bit[i]; P.pos[i] = a->pos_plane[i]; P.neg[i] = a->neg_plane[i]; P.outp[i] = a->out_plane[i];
    }
    hipStream_t st = (hipStream_t)a->stream;
    const uint32_t want = (P.nquads + kBlock - 1) / kBlock;
    const dim3 grid(want < (uint32_t)kSdmMaxBlocks ? want : (uint32_t)kSdmMaxBlocks, (unsigned)a->n_items), block(kBlock);
    if (dist) {
        if (hipMemsetAsync(P.maxima, 0, SEGM_SDM_COMPOSE_WORKSPACE_BYTES, st) != hipSuccess) return (int)hipGetLastError();
        const dim3 mgrid(want < (uint32_t)kSdmMaxBlocksMax ? want : (uint32_t)kSdmMaxBlocksMax, (unsigned)a->n_items);
        hipLaunchKernelGGL(sdm_max_kernel, mgrid, block, 0, st, P);
        hipLaunchKernelGGL(sdm_compose_kernel<true>, grid, block, 0, st, P);
    } else {
        hipLaunchKernelGGL(sdm_compose_kernel<false>, grid, block, 0, st, P);
    }
    return (int)hipGetLastError();
}
