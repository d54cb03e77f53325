// Evaluation on the device: region counts and borders of two label volumes, the exact squared Euclidean distance transform of
// bit planes, and the border-to-border distances Dice / HD95 are made of  (C ABI: segm_seg_regions, segm_edt_sq,
// segm_border_distances).
//
// Replaces what the reference leaves to medpy on the host (5_compute_metrics.py:24-38 `metric.binary.dc / hd95`, and the counts of
// 3_train.py:82-119): `hd95` there is two binary erosions, two Euclidean distance transforms of the whole volume and a percentile,
// per region.  Here:
//   * seg_regions_kernel   one pass over prediction and ground truth: a 256-entry table turns a label into its region bits (up to 8
//                          regions at once), a voxel is a border voxel of a region iff it is inside and one of its six face
//                          neighbours is not (outside the volume = not inside: `mask ^ binary_erosion(mask)` with border_value 0).
//                          Counts as byte fields of 64-bit words per thread (a thread sees 16 voxels), widened to 16-bit fields for the
//                          workgroup sum, one partial row per workgroup, added by seg_counts_reduce_kernel - integers, no atomics.
//   * edt_x_kernel         x is the contiguous axis: a wave owns a row, the row's 8 bit planes become 64-bit masks in LDS and every
//                          lane finds the nearest set bit to its left and right with clz / ctz.
//   * edt_line_kernel      the y and the z pass: a workgroup takes 64 adjacent columns (lane = column, every access coalesced), keeps
//                          the whole line in LDS and takes min_j g[j] + (s (i - j))^2 over it - brute force, exact, deterministic.
//                          Groups of four rows of the slab that hold no finite value are skipped (they can never win the minimum).
//   * border_dist_kernel   per-workgroup counts of the border voxels, an exclusive scan of them, then sqrt(edt) written densely in
//                          voxel order.
// int32 arithmetic for unit spacing (exact), fp32 otherwise.
#include <stdlib.h>
#include <string.h>

#include "segm_device.h"

namespace segm {

constexpr int kMetVox = 16;                         // voxels per thread
constexpr int kMetChunk = kBlock * kMetVox;         // voxels per workgroup
constexpr int kMetFields = 40;                      // 5 quantities x 8 regions
constexpr int kEdtLine = SEGM_EDT_MAX_LINE;
constexpr int kEdtWords = kEdtLine / 64;            // 64-bit masks per row
constexpr int kEdtTile = 10;                        // output rows a thread keeps in registers per sweep over the line (240 = 4 waves x 6 x 10)
constexpr int kEdtGroup = 4;                        // rows of the line read from LDS together (and skipped together when none holds a finite value)
constexpr int32_t kEdtIntInf = 1 << 29;             // "no set voxel yet": kEdtIntInf + 3 * 255^2 stays far from overflow

// ---- region counts and borders -------------------------------------------------------------------------------------------------
struct SegRegDev {
    const uint8_t* pred;
    const uint8_t* gt;
    const uint8_t* table;
    uint8_t* bpred;
    uint8_t* bgt;
    uint32_t* part;            // [workgroup][5 quantities][8 regions]
    int32_t D, H, W, N;
};

// byte k of the result = bit k of m (m < 256)
__device__ __forceinline__ unsigned long long spread8(uint32_t m) {
    const unsigned long long x = ((unsigned long long)m * 0x0101010101010101ull) & 0x8040201008040201ull;
    return ((x + 0x7f7f7f7f7f7f7f7full) >> 7) & 0x0101010101010101ull;
}

__global__ void __launch_bounds__(kBlock) seg_regions_kernel(SegRegDev P) {
    __shared__ uint8_t s_tab[256];
    __shared__ unsigned long long s_red[kWavesPerBlock][10];
    const int tid = threadIdx.x;
    s_tab[tid] = P.table[tid];
    __syncthreads();
    unsigned long long acc[5] = {0ull, 0ull, 0ull, 0ull, 0ull};
    const uint32_t base = (uint32_t)blockIdx.x * kMetChunk;
    const uint32_t W = (uint32_t)P.W, HW = (uint32_t)P.H * (uint32_t)P.W;
    for (int k = 0; k < kMetVox; ++k) {
        const uint32_t idx = base + (uint32_t)k * kBlock + tid;
        if (idx >= (uint32_t)P.N) continue;
        const uint32_t p = s_tab[P.pred[idx]], g = s_tab[P.gt[idx]];
        uint32_t bp = 0, bg = 0;
        if (p | g) {
            const uint32_t z = idx / HW, rem = idx - z * HW, y = rem / W, x = rem - y * W;
            uint32_t pi = p, gi = g;                 // bits of the regions whose six neighbours are all inside
            if (x > 0) { pi &= s_tab[P.pred[idx - 1]]; gi &= s_tab[P.gt[idx - 1]]; } else { pi = 0; gi = 0; }
            if (x + 1 < W) { pi &= s_tab[P.pred[idx + 1]]; gi &= s_tab[P.gt[idx + 1]]; } else { pi = 0; gi = 0; }
            if (y > 0) { pi &= s_tab[P.pred[idx - W]]; gi &= s_tab[P.gt[idx - W]]; } else { pi = 0; gi = 0; }
            if (y + 1 < (uint32_t)P.H) { pi &= s_tab[P.pred[idx + W]]; gi &= s_tab[P.gt[idx + W]]; } else { pi = 0; gi = 0; }
            if (z > 0) { pi &= s_tab[P.pred[idx - HW]]; gi &= s_tab[P.gt[idx - HW]]; } else { pi = 0; gi = 0; }
            if (z + 1 < (uint32_t)P.D) { pi &= s_tab[P.pred[idx + HW]]; gi &= s_tab[P.gt[idx + HW]]; } else { pi = 0; gi = 0; }
            bp = p & ~pi;
            bg = g & ~gi;
            acc[0] += spread8(p);
            acc[1] += spread8(g);
            acc[2] += spread8(p & g);
            acc[3] += spread8(bp);
            acc[4] += spread8(bg);
        }
        P.bpred[idx] = (uint8_t)bp;
        P.bgt[idx] = (uint8_t)bg;
    }
    // byte fields (<= 16 each) -> 16-bit fields (a wave adds 64 of them: <= 1024)
    unsigned long long w[10];
#pragma unroll
    for (int q = 0; q < 5; ++q) {
        w[2 * q] = acc[q] & 0x00ff00ff00ff00ffull;               // regions 0, 2, 4, 6
        w[2 * q + 1] = (acc[q] >> 8) & 0x00ff00ff00ff00ffull;    // regions 1, 3, 5, 7
    }
#pragma unroll
    for (int i = 0; i < 10; ++i)
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) w[i] += __shfl_xor(w[i], m);
    if ((tid & 63) == 0)
#pragma unroll
        for (int i = 0; i < 10; ++i) s_red[tid >> 6][i] = w[i];
    __syncthreads();
    if (tid < kMetFields) {
        const int q = tid >> 3, r = tid & 7;
        uint32_t s = 0;
        for (int wv = 0; wv < kWavesPerBlock; ++wv) s += (uint32_t)((s_red[wv][2 * q + (r & 1)] >> (16 * (r >> 1))) & 0xffffull);
        P.part[(size_t)blockIdx.x * kMetFields + tid] = s;
    }
}

constexpr int kRedWaves = 16;
__global__ void __launch_bounds__(kRedWaves * kWave) seg_counts_reduce_kernel(const uint32_t* part, int32_t nblocks, long long* out) {
    __shared__ long long s_sum[kRedWaves][64];
    const int f = threadIdx.x & 63, q = threadIdx.x >> 6;
    long long s = 0;
    if (f < kMetFields) {
#pragma unroll 8
        for (int b = q; b < nblocks; b += kRedWaves) s += part[(size_t)b * kMetFields + f];
    }
    s_sum[q][f] = s;
    __syncthreads();
    if (threadIdx.x < kMetFields) {
        long long t = 0;
        for (int wv = 0; wv < kRedWaves; ++wv) t += s_sum[wv][threadIdx.x];
        out[threadIdx.x] = t;
    }
}

// ---- squared Euclidean distance transform -------------------------------------------------------------------------------------
template <typename T> struct EdtNum;
template <> struct EdtNum<int32_t> {
    static __device__ __forceinline__ int32_t inf() { return kEdtIntInf; }
    static __device__ __forceinline__ int32_t sq(float, int d) { return d * d; }
    // between passes "nothing yet" stays kEdtIntInf; the last pass writes the public sentinel
    static __device__ __forceinline__ int32_t store(int32_t v, bool last) { return v >= kEdtIntInf ? (last ? INT32_MAX : kEdtIntInf) : v; }
};
template <> struct EdtNum<float> {
    static __device__ __forceinline__ float inf() { return __builtin_huge_valf(); }
    static __device__ __forceinline__ float sq(float s, int d) { const float t = s * (float)d; return t * t; }
    static __device__ __forceinline__ float store(float v, bool) { return v; }
};

struct EdtDev {
    const uint8_t* vol;        // (volumes, D, H, W) bit planes
    void* out;                 // (planes, D, H, W)
    int32_t D, H, W, nplanes;
    int32_t pvol[SEGM_METRICS_MAX_PLANES], pbit[SEGM_METRICS_MAX_PLANES];
    float sx;
    int32_t reserved;
};

// grid (ceil(rows / 4), volumes): a wave owns one row of one byte volume and writes it for every plane taken from that volume
template <typename T>
__global__ void __launch_bounds__(kBlock) edt_x_kernel(EdtDev P) {
    __shared__ uint32_t s_row[kWavesPerBlock][kEdtLine / 4];
    __shared__ unsigned long long s_mask[kWavesPerBlock][8][kEdtWords];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nrows = P.D * P.H;
    const int row = blockIdx.x * kWavesPerBlock + wave;
    const bool valid = row < nrows;
    const size_t N = (size_t)nrows * P.W;
    const uint8_t* src = P.vol + (size_t)blockIdx.y * N + (size_t)(valid ? row : 0) * P.W;
    uint8_t* rowb = reinterpret_cast<uint8_t*>(s_row[wave]);
#pragma unroll
    for (int c = 0; c < kEdtWords; ++c) {
        const int x = lane + 64 * c;
        rowb[x] = (valid && x < P.W) ? src[x] : (uint8_t)0;
    }
    __syncthreads();
    if (lane < 8 * kEdtWords) {                   // lane (bit, c): the mask of plane `bit` over x = 64 c .. 64 c + 63
        const int bit = lane & 7, c = lane >> 3;
        unsigned long long m = 0;
        for (int i = 0; i < 16; ++i) {
            const uint32_t wd = s_row[wave][16 * c + i] >> bit;
            const unsigned long long nib = (wd & 1u) | ((wd >> 7) & 2u) | ((wd >> 14) & 4u) | ((wd >> 21) & 8u);
            m |= nib << (4 * i);
        }
        s_mask[wave][bit][c] = m;
    }
    __syncthreads();
    for (int p = 0; p < P.nplanes; ++p) {
        if (P.pvol[p] != (int)blockIdx.y) continue;
        unsigned long long m[kEdtWords];
#pragma unroll
        for (int k = 0; k < kEdtWords; ++k) m[k] = s_mask[wave][P.pbit[p]][k];
        T* dst = reinterpret_cast<T*>(P.out) + (size_t)p * N + (size_t)(valid ? row : 0) * P.W;
#pragma unroll
        for (int c = 0; c < kEdtWords; ++c) {
            const int x = lane + 64 * c;
            int left = -1, right = -1;
#pragma unroll
            for (int k = 0; k < kEdtWords; ++k) {
                const unsigned long long mk = m[k];
                if (k < c) {
                    if (mk) left = 64 * k + 63 - __builtin_clzll(mk);
                } else if (k == c) {
                    const unsigned long long lm = mk & (~0ull >> (63 - lane)), rm = mk >> lane;
                    if (lm) left = 64 * k + 63 - __builtin_clzll(lm);
                    if (rm) right = x + __builtin_ctzll(rm);
                } else if (mk && right < 0) {
                    right = 64 * k + __builtin_ctzll(mk);
                }
            }
            const int big = 1 << 20;
            const int dl = left >= 0 ? x - left : big, dr = right >= 0 ? right - x : big;
            const int d = dl < dr ? dl : dr;
            if (valid && x < P.W) dst[x] = d == big ? EdtNum<T>::inf() : EdtNum<T>::sq(P.sx, d);
        }
    }
}

struct EdtLineDev {
    void* buf;
    int64_t line_stride;       // elements between consecutive positions of a line
    int64_t outer_stride;      // elements between the slabs of blockIdx.y
    int32_t n;                 // line length (<= kEdtLine)
    int32_t ncol;              // unit-stride columns per slab of blockIdx.y
    float s;                   // spacing along the line
    int32_t last;              // the final pass writes the public "no set voxel" sentinel
};

// grid (ceil(ncol / 64), slabs).  In place: the whole slab is in LDS before the first store.
template <typename T>
__global__ void __launch_bounds__(kBlock) edt_line_kernel(EdtLineDev P) {
    __shared__ T s_g[kEdtLine * 64];
    __shared__ int32_t s_any[kEdtLine / kEdtGroup];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int col = blockIdx.x * 64 + lane;
    const bool ok = col < P.ncol;
    T* base = reinterpret_cast<T*>(P.buf) + (int64_t)blockIdx.y * P.outer_stride + (ok ? col : 0);
    const T inf = EdtNum<T>::inf();
    const int npad = (P.n + kEdtGroup - 1) / kEdtGroup * kEdtGroup;          // <= kEdtLine: rows n .. npad - 1 hold "nothing"
    for (int j = threadIdx.x; j < kEdtLine / kEdtGroup; j += kBlock) s_any[j] = 0;
    __syncthreads();
    for (int j = wave; j < npad; j += kWavesPerBlock) {
        const T g = (ok && j < P.n) ? base[(int64_t)j * P.line_stride] : inf;
        s_g[j * 64 + lane] = g;
        if (g < inf) s_any[j / kEdtGroup] = 1;
    }
    __syncthreads();
    for (int i0 = wave * kEdtTile; i0 < P.n; i0 += kWavesPerBlock * kEdtTile) {
        T acc[kEdtTile];
#pragma unroll
        for (int u = 0; u < kEdtTile; ++u) acc[u] = inf;
        for (int j0 = 0; j0 < npad; j0 += kEdtGroup) {
            if (__builtin_amdgcn_readfirstlane(s_any[j0 / kEdtGroup]) == 0) continue;      // nothing finite in these rows of the slab
            T g[kEdtGroup];
#pragma unroll
            for (int v = 0; v < kEdtGroup; ++v) g[v] = s_g[(j0 + v) * 64 + lane];
#pragma unroll
            for (int v = 0; v < kEdtGroup; ++v)
#pragma unroll
                for (int u = 0; u < kEdtTile; ++u) {
                    const T t = g[v] + EdtNum<T>::sq(P.s, i0 + u - j0 - v);
                    acc[u] = t < acc[u] ? t : acc[u];
                }
        }
#pragma unroll
        for (int u = 0; u < kEdtTile; ++u)
            if (ok && i0 + u < P.n) base[(int64_t)(i0 + u) * P.line_stride] = EdtNum<T>::store(acc[u], P.last != 0);
    }
}

// ---- distances at border voxels --------------------------------------------------------------------------------------------------
struct BorderDistDev {
    const uint8_t* borders;    // (volumes, N)
    const void* edt;           // (planes, N)
    float* out;
    int32_t* blk;              // [item][workgroup]
    int32_t N, nblocks, is_float, reserved;
    int32_t bvol[SEGM_METRICS_MAX_PLANES], bbit[SEGM_METRICS_MAX_PLANES], eplane[SEGM_METRICS_MAX_PLANES];
    int64_t out_off[SEGM_METRICS_MAX_PLANES], out_cnt[SEGM_METRICS_MAX_PLANES];
};

// exclusive prefix of v over the workgroup's threads (in thread order); *total = the sum.  s: kBlock ints of LDS.
__device__ __forceinline__ int block_exclusive_scan(int v, int* s, int* total) {
    const int tid = threadIdx.x;
    s[tid] = v;
    __syncthreads();
    for (int off = 1; off < kBlock; off <<= 1) {
        const int t = tid >= off ? s[tid - off] : 0;
        __syncthreads();
        s[tid] += t;
        __syncthreads();
    }
    const int incl = s[tid];
    *total = s[kBlock - 1];
    __syncthreads();
    return incl - v;
}

// grid (workgroups, items).  WRITE = false: blk[item][workgroup] = border voxels among the workgroup's voxels;
// WRITE = true: blk holds the exclusive scan of those; the distances go out in voxel order.
template <bool WRITE>
__global__ void __launch_bounds__(kBlock) border_dist_kernel(BorderDistDev P) {
    __shared__ int s_scan[kBlock];
    const int item = blockIdx.y;
    const uint8_t* b = P.borders + (size_t)P.bvol[item] * P.N;
    const uint32_t bit = 1u << P.bbit[item];
    const int64_t first = (int64_t)blockIdx.x * kMetChunk + (int64_t)threadIdx.x * kMetVox;
    uint32_t set = 0;
    for (int k = 0; k < kMetVox; ++k)
        if (first + k < P.N && (b[first + k] & bit)) set |= 1u << k;
    int total;
    const int excl = block_exclusive_scan(__builtin_popcount(set), s_scan, &total);
    if (!WRITE) {
        if (threadIdx.x == 0) P.blk[(size_t)item * P.nblocks + blockIdx.x] = total;
        return;
    }
    int64_t pos = (int64_t)P.blk[(size_t)item * P.nblocks + blockIdx.x] + excl;
    const size_t e0 = (size_t)P.eplane[item] * P.N;
    for (int k = 0; k < kMetVox; ++k) {
        if (!((set >> k) & 1u)) continue;
        float d2;
        if (P.is_float) d2 = reinterpret_cast<const float*>(P.edt)[e0 + first + k];
        else d2 = (float)reinterpret_cast<const int32_t*>(P.edt)[e0 + first + k];
        if (pos < P.out_cnt[item]) P.out[P.out_off[item] + pos] = __builtin_sqrtf(d2);
        ++pos;
    }
}

// grid (items): blk[item][0 .. nblocks) -> its exclusive scan, in place
__global__ void __launch_bounds__(kBlock) border_scan_kernel(int32_t* blk, int32_t nblocks) {
    __shared__ int s_scan[kBlock];
    int32_t* row = blk + (size_t)blockIdx.x * nblocks;
    const int per = (nblocks + kBlock - 1) / kBlock;
    const int lo = threadIdx.x * per < nblocks ? threadIdx.x * per : nblocks, hi = lo + per < nblocks ? lo + per : nblocks;
    int sum = 0;
    for (int i = lo; i < hi; ++i) sum += row[i];
    int total;
    int run = block_exclusive_scan(sum, s_scan, &total);
    for (int i = lo; i < hi; ++i) {
        const int v = row[i];
        row[i] = run;
        run += v;
    }
}

static inline int64_t metrics_blocks(int64_t nvox) { return (nvox + kMetChunk - 1) / kMetChunk; }
static inline bool metrics_volume_ok(int64_t d, int64_t h, int64_t w) {
    return d > 0 && h > 0 && w > 0 && d < (1 << 20) && h < (1 << 20) && w < (1 << 20) && d * h * w <= SEGM_METRICS_MAX_VOXELS;
}

template <typename T>
static void launch_edt(const segm_edt_sq_args* a, hipStream_t st) {
    EdtDev X;
    memset(&X, 0, sizeof(X));
    X.vol = a->volumes; X.out = a->out; X.D = a->depth; X.H = a->height; X.W = a->width; X.nplanes = a->n_planes;
    for (int p = 0; p < a->n_planes; ++p) { X.pvol[p] = a->plane_volume[p]; X.pbit[p] = a->plane_bit[p]; }
    X.sx = a->spacing_x;
    const int nrows = a->depth * a->height;
    hipLaunchKernelGGL(edt_x_kernel<T>, dim3((nrows + kWavesPerBlock - 1) / kWavesPerBlock, a->n_volumes), dim3(kBlock), 0, st, X);
    const int64_t HW = (int64_t)a->height * a->width;
    EdtLineDev Y;
    memset(&Y, 0, sizeof(Y));
    Y.buf = a->out; Y.line_stride = a->width; Y.outer_stride = HW; Y.n = a->height; Y.ncol = a->width; Y.s = a->spacing_y; Y.last = 0;
    hipLaunchKernelGGL(edt_line_kernel<T>, dim3((a->width + 63) / 64, a->n_planes * a->depth), dim3(kBlock), 0, st, Y);
    EdtLineDev Z;
    memset(&Z, 0, sizeof(Z));
    Z.buf = a->out; Z.line_stride = HW; Z.outer_stride = HW * a->depth; Z.n = a->depth; Z.ncol = (int32_t)HW; Z.s = a->spacing_z; Z.last = 1;
    hipLaunchKernelGGL(edt_line_kernel<T>, dim3((int)((HW + 63) / 64), a->n_planes), dim3(kBlock), 0, st, Z);
}

}  // namespace segm

using namespace segm;

extern "C" size_t segm_seg_regions_workspace_bytes(int64_t voxels) {
    if (voxels <= 0 || voxels > SEGM_METRICS_MAX_VOXELS) return 0;
    return (size_t)metrics_blocks(voxels) * kMetFields * sizeof(uint32_t);
}

extern "C" int segm_seg_regions(const segm_seg_regions_args* a) {
    if (!a) return SEGM_E_NULL;
    if (!a->pred || !a->gt || !a->table || !a->border_pred || !a->border_gt || !a->counts) return SEGM_E_NULL;
    if (!metrics_volume_ok(a->depth, a->height, a->width)) return SEGM_E_SHAPE;
    const int64_t N = (int64_t)a->depth * a->height * a->width;
    if (!a->workspace || a->workspace_bytes < segm_seg_regions_workspace_bytes(N)) return SEGM_E_WORKSPACE;
    SegRegDev P;
    memset(&P, 0, sizeof(P));
    P.pred = a->pred; P.gt = a->gt; P.table = a->table; P.bpred = a->border_pred; P.bgt = a->border_gt;
    P.part = (uint32_t*)a->workspace;
    P.D = a->depth; P.H = a->height; P.W = a->width; P.N = (int32_t)N;
    const int32_t nblocks = (int32_t)metrics_blocks(N);
    hipStream_t st = (hipStream_t)a->stream;
    hipLaunchKernelGGL(seg_regions_kernel, dim3(nblocks), dim3(kBlock), 0, st, P);
    hipLaunchKernelGGL(seg_counts_reduce_kernel, dim3(1), dim3(kRedWaves * kWave), 0, st, (const uint32_t*)P.part, nblocks, (long long*)a->counts);
    return (int)hipGetLastError();
}

extern "C" int segm_edt_sq(const segm_edt_sq_args* a) {
    if (!a) return SEGM_E_NULL;
    if (!a->volumes || !a->out) return SEGM_E_NULL;
    if (a->depth <= 0 || a->height <= 0 || a->width <= 0) return SEGM_E_SHAPE;
    if (a->depth > SEGM_EDT_MAX_LINE || a->height > SEGM_EDT_MAX_LINE || a->width > SEGM_EDT_MAX_LINE) return SEGM_E_SHAPE;
    if (a->n_volumes <= 0 || a->n_volumes > SEGM_METRICS_MAX_PLANES || a->n_planes <= 0 || a->n_planes > SEGM_METRICS_MAX_PLANES) return SEGM_E_SHAPE;
    for (int p = 0; p < a->n_planes; ++p)
        if (a->plane_volume[p] < 0 || a->plane_volume[p] >= a->n_volumes || a->plane_bit[p] < 0 || a->plane_bit[p] > 7) return SEGM_E_SHAPE;
    if (a->fp32 != 0 && a->fp32 != 1) return SEGM_E_DTYPE;
    if (a->fp32) {
        if (!(a->spacing_x > 0.f && a->spacing_y > 0.f && a->spacing_z > 0.f) || !(a->spacing_x + a->spacing_y + a->spacing_z < 1e15f)) return SEGM_E_SHAPE;
        launch_edt<float>(a, (hipStream_t)a->stream);
    } else {
        if (a->spacing_x != 1.f || a->spacing_y != 1.f || a->spacing_z != 1.f) return SEGM_E_DTYPE;      // int32 is the unit-spacing form
        launch_edt<int32_t>(a, (hipStream_t)a->stream);
    }
    return (int)hipGetLastError();
}

extern "C" size_t segm_border_distances_workspace_bytes(int64_t voxels, int32_t n_items) {
    if (voxels <= 0 || voxels > SEGM_METRICS_MAX_VOXELS || n_items <= 0 || n_items > SEGM_METRICS_MAX_PLANES) return 0;
    return (size_t)metrics_blocks(voxels) * n_items * sizeof(int32_t);
}

extern "C" int segm_border_distances(const segm_border_distances_args* a) {
    if (!a) return SEGM_E_NULL;
    if (!a->borders || !a->edt || !a->out) return SEGM_E_NULL;
    if (a->voxels <= 0 || a->voxels > SEGM_METRICS_MAX_VOXELS) return SEGM_E_SHAPE;
    if (a->n_items <= 0 || a->n_items > SEGM_METRICS_MAX_PLANES || a->n_volumes <= 0 || a->n_planes <= 0) return SEGM_E_SHAPE;
    if (a->fp32 != 0 && a->fp32 != 1) return SEGM_E_DTYPE;
    for (int i = 0; i < a->n_items; ++i) {
        if (a->border_volume[i] < 0 || a->border_volume[i] >= a->n_volumes || a->border_bit[i] < 0 || a->border_bit[i] > 7) return SEGM_E_SHAPE;
        if (a->edt_plane[i] < 0 || a->edt_plane[i] >= a->n_planes) return SEGM_E_SHAPE;
        if (a->out_offset[i] < 0 || a->out_count[i] < 0 || a->out_offset[i] + a->out_count[i] > a->out_capacity) return SEGM_E_SHAPE;
    }
    if (!a->workspace || a->workspace_bytes < segm_border_distances_workspace_bytes(a->voxels, a->n_items)) return SEGM_E_WORKSPACE;
    BorderDistDev P;
    memset(&P, 0, sizeof(P));
    P.borders = a->borders; P.edt = a->edt; P.out = a->out; P.blk = (int32_t*)a->workspace;
    P.N = (int32_t)a->voxels; P.nblocks = (int32_t)metrics_blocks(a->voxels); P.is_float = a->fp32;
    for (int i = 0; i < a->n_items; ++i) {
        P.bvol[i] = a->border_volume[i]; P.bbit[i] = a->border_bit[i]; P.eplane[i] = a->edt_plane[i];
        P.out_off[i] = a->out_offset[i]; P.out_cnt[i] = a->out_count[i];
    }
    hipStream_t st = (hipStream_t)a->stream;
    const dim3 grid(P.nblocks, a->n_items), block(kBlock);
    hipLaunchKernelGGL(border_dist_kernel<false>, grid, block, 0, st, P);
    hipLaunchKernelGGL(border_scan_kernel, dim3(a->n_items), block, 0, st, P.blk, P.nblocks);
    hipLaunchKernelGGL(border_dist_kernel<true>, grid, block, 0, st, P);
    return (int)hipGetLastError();
}
