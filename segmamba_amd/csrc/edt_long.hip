// Evaluation of volumes with sides beyond SEGM_EDT_MAX_LINE: the exact squared Euclidean distance transform of bit planes at a cost
// linear in the line length, and the bounding boxes of bit planes  (C ABI: segm_edt_sq_long, segm_planes_bbox).
//
// segm_edt_sq (metrics.hip) keeps a whole line of 64 columns in LDS and takes a brute-force min-plus over it: O(n^2) per column and
// n <= 256.  CT volumes are 512 x 512 x several hundred.  Here:
//   * edt_long_x_kernel     x is the contiguous axis: a wave owns a row, the row's 8 bit planes are 64-bit masks in LDS (32 words per
//                           plane at 2048), one more word per plane tells which of them hold a set bit at all, and every lane finds
//                           the nearest set bit to its left and right with clz / ctz over its own word and the nearest non-empty word
//                           on either side.
//   * edt_long_line_kernel  the y and the z pass: the lower envelope of the parabolas g[i] + (s (u - i))^2 (Meijster / Felzenszwalb-
//                           Huttenlocher).  One THREAD per line, the lanes of a wave along the unit-stride axis, so every access of a
//                           wave is 64 adjacent elements.  A forward scan builds the stack of (position i, first position of its
//                           interval, g[i]); a backward scan writes the values.  Positions that hold "nothing yet" are never pushed;
//                           an empty stack writes the sentinel.
//                           IN PLACE, with a copy of g in the stack entry: the backward scan reads the stack alone, so the line may
//                           be overwritten while it runs.  The alternative, a second buffer, costs planes x voxels x 4 bytes (419 MB per
//                           plane at 400 x 512 x 512) and turns the backward scan's g[i] into a gather across rows; the stacks cost
//                           8 bytes x line length per thread IN FLIGHT, whatever the volume: workgroups are persistent (each takes
//                           batches of 256 lines in turn and reuses its stack area), the workspace is sized by the grid.
//                           Stack entries are laid out [entry][thread]: a wave's push or pop of one level is 512 contiguous bytes.
//                           Positions and interval starts fit 16 bits (n <= 2048).
//     Expected cost of a wave per line of n positions: the lanes diverge in the pop loop, so the wave runs the LONGEST sequence of its
//     64 lanes: n loads of g, at most n pushes and n pops in the forward scan (<= 3 n steps), n stores and at most n pops backward.
//     Traffic by the algorithm's count: 4 n bytes read, 8 k written and 8 k read again (k <= n pushes), 4 n written - between 8 and
//     24 bytes per voxel and pass where a streaming pass has 8.  The top of the stack and the entry below it stay in registers,
//     so a pop compares at once and its load (of the entry two below) is only waited for by a second pop in a row; what remains is
//     latency, not bandwidth: a serial chain per lane, hidden only by the other waves of the SIMD.
//   * planes_bbox_kernel    boxes of up to 16 (volume, bit) items, an item optionally the OR of two planes, in one pass: 16-byte loads
//                           along x, a wave owns 1024 bytes of one row (z and y are wave-uniform), per item one ballot says whether
//                           the wave saw a set bit at all - if not, nothing is exchanged - and two lane reads give the x extrema.
//                           Per-workgroup boxes in LDS, then at most 6 integer min / max atomics per item and workgroup: the result
//                           does not depend on their order.
// int32 arithmetic for unit spacing (exact: every operand stays below 2^25 at sides of 2048), fp32 values otherwise with the
// intersections of the parabolas in fp64.  No floating-point atomics; two calls are bit-equal.
#include <stdlib.h>
#include <string.h>

#include "segm_device.h"

namespace segm {

constexpr int kLongLine = SEGM_EDT_LONG_MAX_LINE;
constexpr int kLongWords = kLongLine / 64;              // 64-bit masks per row and plane
constexpr int32_t kLongIntInf = 1 << 29;                // "no set voxel yet" between the passes
constexpr int kLongDefaultGroups = 1024;                // persistent workgroups of a line pass: 4 per CU, 4 waves per SIMD
constexpr int kBboxRun = kWave * 16;                    // bytes of a row that a wave takes at once
constexpr int kBboxMaxGroups = 1024;

typedef uint32_t long_raw4 __attribute__((ext_vector_type(4)));

template <typename T> struct LongNum;
template <> struct LongNum<int32_t> {
    static __device__ __forceinline__ int32_t inf() { return kLongIntInf; }
    static __device__ __forceinline__ bool finite(int32_t v) { return v < kLongIntInf; }
    static __device__ __forceinline__ int32_t sq(float, int d) { return d * d; }
    static __device__ __forceinline__ int32_t sentinel(bool last) { return last ? INT32_MAX : kLongIntInf; }
    static __device__ __forceinline__ uint32_t bits(int32_t v) { return (uint32_t)v; }
    static __device__ __forceinline__ int32_t from_bits(uint32_t v) { return (int32_t)v; }
    // does the top (position i, value gi, interval from ti) survive position u (value gu)?  If so *w = the first position at which
    // u is the smaller of the two: 1 + (u^2 - i^2 + gu - gi) div (2 (u - i)); the numerator is >= 0 then, so `/` is the floor.
    static __device__ __forceinline__ bool keeps(double, int i, int32_t gi, int ti, int u, int32_t gu, int n, int* w) {
        const int a = ti - i, b = ti - u;
        if (a * a + gi > b * b + gu) return false;
        *w = 1 + (u * u - i * i + gu - gi) / (2 * (u - i));
        return true;
    }
};
template <> struct LongNum<float> {
    static __device__ __forceinline__ float inf() { return __builtin_huge_valf(); }
    static __device__ __forceinline__ bool finite(float v) { return v < __builtin_huge_valf(); }
    static __device__ __forceinline__ float sq(float s, int d) { const float t = s * (float)d; return t * t; }
    static __device__ __forceinline__ float sentinel(bool) { return __builtin_huge_valf(); }
    static __device__ __forceinline__ uint32_t bits(float v) { return __float_as_uint(v); }
    static __device__ __forceinline__ float from_bits(uint32_t v) { return __uint_as_float(v); }
    // the parabolas of i and u meet at x = ((gu - gi) / s^2 + u^2 - i^2) / (2 (u - i)), in fp64; u is the smaller from
    // w = 1 + floor(x) on, and replaces the top when that is no later than the start of the top's interval
    static __device__ __forceinline__ bool keeps(double s2, int i, float gi, int ti, int u, float gu, int n, int* w) {
        const double x = (((double)gu - (double)gi) / s2 + (double)(u * u - i * i)) / (double)(2 * (u - i));
        const int v = x >= (double)n ? n : (x < 0.0 ? 0 : 1 + (int)x);
        *w = v;
        return v > ti;
    }
};

// ---- x pass -----------------------------------------------------------------------------------------------------------------------
struct LongXDev {
    const uint8_t* vol;        // (volumes, D, H, W) bit planes
    void* out;                 // (planes, D, H, W)
    int32_t D, H, W, nplanes;
    int32_t pvol[SEGM_METRICS_MAX_PLANES], pbit[SEGM_METRICS_MAX_PLANES];
    float sx;
    int32_t vec;               // rows start on 16 bytes: 16-byte loads
};

// grid (ceil(rows / 4), volumes): a wave owns one row of one byte volume and writes it for every plane taken from that volume
template <typename T>
__global__ void __launch_bounds__(kBlock) edt_long_x_kernel(LongXDev P) {
    __shared__ uint32_t s_row[kWavesPerBlock][kLongLine / 4];
    __shared__ unsigned long long s_mask[kWavesPerBlock][8][kLongWords];
    __shared__ uint32_t s_nz[kWavesPerBlock][8];       // bit k: word k of the plane's row holds a set bit
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nrows = P.D * P.H;
    const int row = blockIdx.x * kWavesPerBlock + wave;
    const bool valid = row < nrows;
    const size_t N = (size_t)nrows * P.W;
    const uint8_t* src = P.vol + (size_t)blockIdx.y * N + (size_t)(valid ? row : 0) * P.W;
    const int nwords = (P.W + 63) >> 6;                // <= kLongWords
    if (P.vec) {                                       // W % 16 == 0: a packet lies inside the row or past its end
        for (int q = lane; q < nwords * 4; q += kWave) {
            long_raw4 v = {0u, 0u, 0u, 0u};
            if (valid && q * 16 < P.W) v = *reinterpret_cast<const long_raw4*>(src + q * 16);
#pragma unroll
            for (int k = 0; k < 4; ++k) s_row[wave][q * 4 + k] = v[k];
        }
    } else {
        uint8_t* rowb = reinterpret_cast<uint8_t*>(s_row[wave]);
        for (int x = lane; x < nwords * 64; x += kWave) rowb[x] = (valid && x < P.W) ? src[x] : (uint8_t)0;
    }
    __syncthreads();
    for (int it = lane; it < 8 * nwords; it += kWave) {        // (bit, c): the mask of plane `bit` over x = 64 c .. 64 c + 63
        const int bit = it & 7, c = it >> 3;
        unsigned long long m = 0;
        for (int i = 0; i < 16; ++i) {
            const uint32_t wd = s_row[wave][16 * c + i] >> bit;
            const unsigned long long nib = (wd & 1u) | ((wd >> 7) & 2u) | ((wd >> 14) & 4u) | ((wd >> 21) & 8u);
            m |= nib << (4 * i);
        }
        s_mask[wave][bit][c] = m;
    }
    __syncthreads();
    if (lane < 8) {
        uint32_t nzw = 0;
        for (int k = 0; k < nwords; ++k) nzw |= s_mask[wave][lane][k] != 0ull ? 1u << k : 0u;
        s_nz[wave][lane] = nzw;
    }
    __syncthreads();
    for (int p = 0; p < P.nplanes; ++p) {
        if (P.pvol[p] != (int)blockIdx.y) continue;
        const unsigned long long* m = s_mask[wave][P.pbit[p]];
        const unsigned long long nz = s_nz[wave][P.pbit[p]];       // wave-uniform
        T* dst = reinterpret_cast<T*>(P.out) + (size_t)p * N + (size_t)(valid ? row : 0) * P.W;
        for (int c = 0; c < nwords; ++c) {
            const int x = lane + 64 * c;
            const unsigned long long mc = m[c];
            const unsigned long long lm = mc & (~0ull >> (63 - lane)), rm = mc >> lane;
            const unsigned long long below = nz & ((1ull << c) - 1ull), above = c < 63 ? nz >> (c + 1) : 0ull;
            int left = -1, right = -1;
            if (lm) left = 64 * c + 63 - __builtin_clzll(lm);
            else if (below) { const int k = 63 - __builtin_clzll(below); left = 64 * k + 63 - __builtin_clzll(m[k]); }
            if (rm) right = x + __builtin_ctzll(rm);
            else if (above) { const int k = c + 1 + __builtin_ctzll(above); right = 64 * k + __builtin_ctzll(m[k]); }
            const int big = 1 << 20;
            const int dl = left >= 0 ? x - left : big, dr = right >= 0 ? right - x : big;
            const int d = dl < dr ? dl : dr;
            if (valid && x < P.W) dst[x] = d == big ? LongNum<T>::inf() : LongNum<T>::sq(P.sx, d);
        }
    }
}

// ---- y and z pass -----------------------------------------------------------------------------------------------------------------
struct LongLineDev {
    void* buf;
    unsigned long long* stack; // [workgroup][entry < n][thread < kBlock]
    int64_t line_stride;       // elements between consecutive positions of a line
    int64_t outer_stride;      // elements between slabs
    int32_t n;                 // line length (<= kLongLine)
    int32_t ncol;              // unit-stride columns per slab
    int32_t bps;               // batches of kBlock columns per slab
    int32_t nbatch;            // slabs * bps
    float s;                   // spacing along the line
    int32_t last;              // the final pass writes the public "no set voxel" sentinel
};

struct LongEntry { int pos, start; uint32_t g; };
__device__ __forceinline__ unsigned long long long_pack(int pos, int start, uint32_t g) {
    return (unsigned long long)((uint32_t)pos | ((uint32_t)start << 16)) | ((unsigned long long)g << 32);
}
__device__ __forceinline__ LongEntry long_unpack(unsigned long long e) {
    LongEntry r;
    r.pos = (int)(e & 0xffffull); r.start = (int)((e >> 16) & 0xffffull); r.g = (uint32_t)(e >> 32);
    return r;
}

// grid (min(nbatch, cap)): workgroup b takes the batches b, b + grid, ... and reuses its stack area for each
template <typename T>
__global__ void __launch_bounds__(kBlock) edt_long_line_kernel(LongLineDev P) {
    typedef LongNum<T> Num;
    unsigned long long* stk = P.stack + (size_t)blockIdx.x * P.n * kBlock + threadIdx.x;       // entry e at stk[e * kBlock]
    const double s2 = (double)P.s * (double)P.s;
    const int n = P.n;
    for (int batch = blockIdx.x; batch < P.nbatch; batch += gridDim.x) {
        const int slab = batch / P.bps;
        const int col = (batch - slab * P.bps) * kBlock + (int)threadIdx.x;
        if (col >= P.ncol) continue;                   // no barrier in this kernel: a thread only ever meets its own stack
        T* base = reinterpret_cast<T*>(P.buf) + (int64_t)slab * P.outer_stride + col;
        // forward: the stack of the lower envelope; `top` and `nxt` mirror entries q and q - 1
        int q = -1;
        LongEntry top = {0, 0, 0u}, nxt = {0, 0, 0u};
        T gn = base[0];
        for (int u = 0; u < n; ++u) {
            const T gu = gn;
            if (u + 1 < n) gn = base[(int64_t)(u + 1) * P.line_stride];
            if (!Num::finite(gu)) continue;
            int w = 0;
            while (q >= 0) {
                if (Num::keeps(s2, top.pos, Num::from_bits(top.g), top.start, u, gu, n, &w)) break;
                top = nxt;
                --q;
                if (q >= 1) nxt = long_unpack(stk[(size_t)(q - 1) * kBlock]);
            }
            if (q >= 0 && w >= n) continue;            // u is nowhere the smallest inside the line
            if (q < 0) w = 0;
            ++q;                                       // q <= u < n: inside the thread's stack
            stk[(size_t)q * kBlock] = long_pack(u, w, Num::bits(gu));
            nxt = top;
            top.pos = u; top.start = w; top.g = Num::bits(gu);
        }
        if (q < 0) {
            for (int u = 0; u < n; ++u) base[(int64_t)u * P.line_stride] = Num::sentinel(P.last != 0);
            continue;
        }
        // backward: position u belongs to the top's interval until u passes its start
        for (int u = n - 1; u >= 0; --u) {
            base[(int64_t)u * P.line_stride] = Num::from_bits(top.g) + Num::sq(P.s, u - top.pos);
            if (u == top.start && q > 0) {
                top = nxt;
                --q;
                if (q >= 1) nxt = long_unpack(stk[(size_t)(q - 1) * kBlock]);
            }
        }
    }
}

// ---- boxes of bit planes ----------------------------------------------------------------------------------------------------------
#ifdef SEGM_EMU
static inline void bbox_min(int32_t* p, int32_t v) { __atomic_fetch_min(p, v, __ATOMIC_RELAXED); }
static inline void bbox_max(int32_t* p, int32_t v) { __atomic_fetch_max(p, v, __ATOMIC_RELAXED); }
static inline void bbox_min_lds(int32_t* p, int32_t v) { __atomic_fetch_min(p, v, __ATOMIC_RELAXED); }
static inline void bbox_max_lds(int32_t* p, int32_t v) { __atomic_fetch_max(p, v, __ATOMIC_RELAXED); }
#else
__device__ __forceinline__ void bbox_min(int32_t* p, int32_t v) { __hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void bbox_max(int32_t* p, int32_t v) { __hip_atomic_fetch_max(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void bbox_min_lds(int32_t* p, int32_t v) { __hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ __forceinline__ void bbox_max_lds(int32_t* p, int32_t v) { __hip_atomic_fetch_max(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
#endif

constexpr int kBboxItems = SEGM_METRICS_MAX_PLANES;
constexpr int32_t kBboxLow = 0x7f7f7f7f;               // the lower end of an empty box, as segm_nonzero_mask_bbox leaves it

struct BboxDev {
    const uint8_t* vol;        // (volumes, D, H, W)
    int32_t* out;              // [item][z0, z1, y0, y1, x0, x1]
    int32_t D, H, W, nvol, nitems;
    int32_t parts;             // runs of kBboxRun bytes per row
    int32_t vec;
    uint32_t nruns;            // rows * parts
    int32_t iv[kBboxItems], ib[kBboxItems], iv2[kBboxItems], ib2[kBboxItems];
};

__global__ void __launch_bounds__(kWave * 2) planes_bbox_init_kernel(int32_t* out) {
    if (threadIdx.x < kBboxItems * 6) out[threadIdx.x] = (threadIdx.x & 1) ? 0 : kBboxLow;
}

// bit k of the result = bit `bit` of byte k of the 16 bytes q
__device__ __forceinline__ uint32_t bbox_bits16(const uint32_t* q, int bit) {
    uint32_t m = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) m |= (((((q[k] >> bit) & 0x01010101u) * 0x01020408u) >> 24) & 0xfu) << (4 * k);
    return m;
}

// grid (min(ceil(runs / 4), kBboxMaxGroups)): the waves take runs of kBboxRun bytes of one row in turn
__global__ void __launch_bounds__(kBlock) planes_bbox_kernel(BboxDev P) {
    __shared__ int32_t s_box[kBboxItems][6];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (threadIdx.x < kBboxItems * 6) s_box[threadIdx.x / 6][threadIdx.x % 6] = (threadIdx.x & 1) ? 0 : INT32_MAX;
    __syncthreads();
    const size_t N = (size_t)P.D * P.H * P.W;
    for (uint32_t run = (uint32_t)blockIdx.x * kWavesPerBlock + wave; run < P.nruns; run += gridDim.x * kWavesPerBlock) {
        const uint32_t row = run / (uint32_t)P.parts;
        const int xb = (int)(run - row * (uint32_t)P.parts) * kBboxRun;
        const int z = (int)(row / (uint32_t)P.H), y = (int)(row - (uint32_t)z * (uint32_t)P.H);
        const int x0 = xb + lane * 16;
        uint32_t m[kBboxItems];
#pragma unroll
        for (int i = 0; i < kBboxItems; ++i) m[i] = 0;
        for (int v = 0; v < P.nvol; ++v) {
            const uint8_t* p = P.vol + (size_t)v * N + (size_t)row * P.W + x0;
            uint32_t q[4] = {0u, 0u, 0u, 0u};
            if (P.vec) {
                if (x0 < P.W) {
                    const long_raw4 r = *reinterpret_cast<const long_raw4*>(p);
#pragma unroll
                    for (int k = 0; k < 4; ++k) q[k] = r[k];
                }
            } else {
#pragma unroll
                for (int k = 0; k < 16; ++k)
                    if (x0 + k < P.W) q[k >> 2] |= (uint32_t)p[k] << (8 * (k & 3));
            }
#pragma unroll
            for (int i = 0; i < kBboxItems; ++i) {
                if (i >= P.nitems) continue;
                if (P.iv[i] == v) m[i] |= bbox_bits16(q, P.ib[i]);
                if (P.iv2[i] == v) m[i] |= bbox_bits16(q, P.ib2[i]);
            }
        }
#pragma unroll
        for (int i = 0; i < kBboxItems; ++i) {
            if (i >= P.nitems) continue;
            const unsigned long long any = __ballot(m[i] != 0u);
            if (any == 0ull) continue;                 // the wave saw only zeros for this item: nothing to exchange
            const int first = __builtin_ctzll(any), lastl = 63 - __builtin_clzll(any);
            const uint32_t mf = __shfl(m[i], first), ml = __shfl(m[i], lastl);
            if (lane == 0) {
                bbox_min_lds(&s_box[i][0], z); bbox_max_lds(&s_box[i][1], z + 1);
                bbox_min_lds(&s_box[i][2], y); bbox_max_lds(&s_box[i][3], y + 1);
                bbox_min_lds(&s_box[i][4], xb + first * 16 + __builtin_ctz(mf));
                bbox_max_lds(&s_box[i][5], xb + lastl * 16 + 32 - __builtin_clz(ml));
            }
        }
    }
    __syncthreads();
    if (threadIdx.x < kBboxItems * 6) {
        const int32_t v = s_box[threadIdx.x / 6][threadIdx.x % 6];
        if (threadIdx.x & 1) { if (v > 0) bbox_max(P.out + threadIdx.x, v); }
        else if (v != INT32_MAX) bbox_min(P.out + threadIdx.x, v);
    }
}

// ---- host -------------------------------------------------------------------------------------------------------------------------
static inline bool long_sides_ok(int64_t d, int64_t h, int64_t w) {
    return d > 0 && h > 0 && w > 0 && d <= kLongLine && h <= kLongLine && w <= kLongLine && d * h * w <= SEGM_METRICS_MAX_VOXELS;
}
static inline int64_t long_batches(int64_t slabs, int64_t ncol) { return slabs * ((ncol + kBlock - 1) / kBlock); }
static inline int64_t long_groups(int64_t nbatch, int32_t cap) {
    const int64_t c = (cap > 0 && cap < kLongDefaultGroups) ? cap : kLongDefaultGroups;      // the field can only lower the default
    return nbatch < c ? nbatch : c;
}
static inline size_t long_pass_bytes(int64_t nbatch, int64_t n, int32_t cap) {
    return (size_t)long_groups(nbatch, cap) * (size_t)n * kBlock * sizeof(unsigned long long);
}

template <typename T>
static void launch_edt_long(const segm_edt_sq_long_args* a, hipStream_t st) {
    LongXDev X;
    memset(&X, 0, sizeof(X));
    X.vol = a->volumes; X.out = a->out; X.D = a->depth; X.H = a->height; X.W = a->width; X.nplanes = a->n_planes;
    for (int p = 0; p < a->n_planes; ++p) { X.pvol[p] = a->plane_volume[p]; X.pbit[p] = a->plane_bit[p]; }
    X.sx = a->spacing_x;
    X.vec = a->width % 16 == 0 && (uintptr_t)a->volumes % 16 == 0;
    const int nrows = a->depth * a->height;
    hipLaunchKernelGGL(edt_long_x_kernel<T>, dim3((nrows + kWavesPerBlock - 1) / kWavesPerBlock, a->n_volumes), dim3(kBlock), 0, st, X);
    const int64_t HW = (int64_t)a->height * a->width;
    LongLineDev Y;
    memset(&Y, 0, sizeof(Y));
    Y.buf = a->out; Y.stack = (unsigned long long*)a->workspace;
    Y.line_stride = a->width; Y.outer_stride = HW; Y.n = a->height; Y.ncol = a->width;
    Y.bps = (a->width + kBlock - 1) / kBlock; Y.nbatch = (int32_t)long_batches((int64_t)a->n_planes * a->depth, a->width);
    Y.s = a->spacing_y; Y.last = 0;
    hipLaunchKernelGGL(edt_long_line_kernel<T>, dim3((int)long_groups(Y.nbatch, a->max_workgroups)), dim3(kBlock), 0, st, Y);
    LongLineDev Z = Y;
    Z.line_stride = HW; Z.outer_stride = HW * a->depth; Z.n = a->depth; Z.ncol = (int32_t)HW;
    Z.bps = (int32_t)((HW + kBlock - 1) / kBlock); Z.nbatch = (int32_t)long_batches(a->n_planes, HW);
    Z.s = a->spacing_z; Z.last = 1;
    hipLaunchKernelGGL(edt_long_line_kernel<T>, dim3((int)long_groups(Z.nbatch, a->max_workgroups)), dim3(kBlock), 0, st, Z);
}

}  // namespace segm

using namespace segm;

extern "C" size_t segm_edt_sq_long_workspace_bytes(int32_t depth, int32_t height, int32_t width, int32_t n_planes, int32_t fp32) {
    if (!long_sides_ok(depth, height, width) || n_planes <= 0 || n_planes > SEGM_METRICS_MAX_PLANES || (fp32 != 0 && fp32 != 1)) return 0;
    const size_t y = long_pass_bytes(long_batches((int64_t)n_planes * depth, width), height, 0);
    const size_t z = long_pass_bytes(long_batches(n_planes, (int64_t)height * width), depth, 0);
    return y > z ? y : z;
}

extern "C" int segm_edt_sq_long(const segm_edt_sq_long_args* a) {
    if (!a) return SEGM_E_NULL;
    if (!a->volumes || !a->out) return SEGM_E_NULL;
    if (!long_sides_ok(a->depth, a->height, a->width)) return SEGM_E_SHAPE;
    if (a->n_volumes <= 0 || a->n_volumes > SEGM_METRICS_MAX_PLANES || a->n_planes <= 0 || a->n_planes > SEGM_METRICS_MAX_PLANES) return SEGM_E_SHAPE;
    for (int p = 0; p < a->n_planes; ++p)
        if (a->plane_volume[p] < 0 || a->plane_volume[p] >= a->n_volumes || a->plane_bit[p] < 0 || a->plane_bit[p] > 7) return SEGM_E_SHAPE;
    if (a->max_workgroups < 0) return SEGM_E_SHAPE;
    if (a->fp32 != 0 && a->fp32 != 1) return SEGM_E_DTYPE;
    if (a->fp32) {
        if (!(a->spacing_x > 0.f && a->spacing_y > 0.f && a->spacing_z > 0.f) || !(a->spacing_x + a->spacing_y + a->spacing_z < 1e15f)) return SEGM_E_SHAPE;
    } else if (a->spacing_x != 1.f || a->spacing_y != 1.f || a->spacing_z != 1.f) {
        return SEGM_E_DTYPE;                           // int32 is the unit-spacing form
    }
    if (!a->workspace || (uintptr_t)a->workspace % sizeof(unsigned long long) ||
        a->workspace_bytes < segm_edt_sq_long_workspace_bytes(a->depth, a->height, a->width, a->n_planes, a->fp32)) return SEGM_E_WORKSPACE;
    if (a->fp32) launch_edt_long<float>(a, (hipStream_t)a->stream);
    else launch_edt_long<int32_t>(a, (hipStream_t)a->stream);
    return (int)hipGetLastError();
}

extern "C" int segm_planes_bbox(const segm_planes_bbox_args* a) {
    if (!a) return SEGM_E_NULL;
    if (!a->volumes || !a->boxes) return SEGM_E_NULL;
    if (a->depth <= 0 || a->height <= 0 || a->width <= 0) return SEGM_E_SHAPE;
    if (a->depth >= (1 << 20) || a->height >= (1 << 20) || a->width >= (1 << 20)) return SEGM_E_SHAPE;
    if ((int64_t)a->depth * a->height * a->width > SEGM_METRICS_MAX_VOXELS) return SEGM_E_SHAPE;
    if (a->n_volumes <= 0 || a->n_volumes > SEGM_METRICS_MAX_PLANES || a->n_items <= 0 || a->n_items > SEGM_METRICS_MAX_PLANES) return SEGM_E_SHAPE;
    for (int i = 0; i < a->n_items; ++i) {
        if (a->item_volume[i] < 0 || a->item_volume[i] >= a->n_volumes || a->item_bit[i] < 0 || a->item_bit[i] > 7) return SEGM_E_SHAPE;
        if (a->item_volume2[i] < -1 || a->item_volume2[i] >= a->n_volumes) return SEGM_E_SHAPE;
        if (a->item_volume2[i] >= 0 && (a->item_bit2[i] < 0 || a->item_bit2[i] > 7)) return SEGM_E_SHAPE;
    }
    if ((uintptr_t)a->boxes % sizeof(int32_t)) return SEGM_E_SHAPE;
    BboxDev P;
    memset(&P, 0, sizeof(P));
    P.vol = a->volumes; P.out = a->boxes;
    P.D = a->depth; P.H = a->height; P.W = a->width; P.nvol = a->n_volumes; P.nitems = a->n_items;
    P.parts = (a->width + kBboxRun - 1) / kBboxRun;
    P.vec = a->width % 16 == 0 && (uintptr_t)a->volumes % 16 == 0;
    P.nruns = (uint32_t)((int64_t)a->depth * a->height * P.parts);
    for (int i = 0; i < kBboxItems; ++i) { P.iv[i] = P.iv2[i] = -1; }
    for (int i = 0; i < a->n_items; ++i) {
        P.iv[i] = a->item_volume[i]; P.ib[i] = a->item_bit[i];
        P.iv2[i] = a->item_volume2[i]; P.ib2[i] = a->item_volume2[i] >= 0 ? a->item_bit2[i] : 0;
    }
    hipStream_t st = (hipStream_t)a->stream;
    const uint32_t want = (P.nruns + kWavesPerBlock - 1) / kWavesPerBlock;
    hipLaunchKernelGGL(planes_bbox_init_kernel, dim3(1), dim3(kWave * 2), 0, st, P.out);
    hipLaunchKernelGGL(planes_bbox_kernel, dim3(want < (uint32_t)kBboxMaxGroups ? want : (uint32_t)kBboxMaxGroups), dim3(kBlock), 0, st, P);
    return (int)hipGetLastError();
}
