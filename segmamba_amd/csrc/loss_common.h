// The skeleton of the loss kernels that stream a volume once and keep fp64 sums (region_loss.hip, dice_ce.hip), described here once.
//
//   * the forward kernel  a workgroup owns a stretch of `chunk` voxels of one sample for ALL planes (regions / classes) of the logits,
//                         so what belongs to a voxel (label, mask) is read once.  A thread takes packets of 16 bytes of logits along x
//                         (4 fp32, 8 fp16 / bf16) where the rows are aligned (loss_rows_aligned, plus each loss's own pointers),
//                         single voxels otherwise; the per-voxel terms come from ONE function of the loss whose products are rounded
//                         on their own (RL_ROUND), so both routes compute a voxel alike.  Every term is added in fp64 in the thread,
//                         then over the wave by shuffles (rl_wave_sum), then over the four waves through LDS (loss_block_row): the
//                         workgroup writes one row of partial sums, `groups` sums per plane and then the sums per sample.
//   * loss_finish_kernel  one workgroup per sample adds the rows in a fixed order (wave w takes the slots w, w + 4, ..., lane l the
//                         rows l, l + 64, ..., then a shuffle tree) and writes the fp64 results.  No floating-point atomic: two
//                         calls are bit-equal.
//   * the backward kernel the same packets, one per thread (loss_bwd_grid), no reduction.
// Each loss keeps its arithmetic, its accumulation loop and the meaning it gives a label; RL_ROUND, rl_load and rl_wave_sum also
// serve intensity.hip.
#pragma once
#include "segm_device.h"

namespace segm {

// The library is built with -ffp-contract=fast, under which the backend may fuse a product into a following sum whatever a pragma
// says, and two instantiations need not fuse alike.  RL_ROUND(x) makes x a value the compiler has to form as written (an empty asm
// that reads and writes the register, no memory clobber), so a product that feeds a sum is rounded on its own in every route.
#ifdef SEGM_EMU
#define RL_ROUND(x) ((void)0)
#else
#define RL_ROUND(x) asm("" : "+v"(x))
#endif

// N elements of a dense array from element index i; a packet starts at a multiple of N elements of a 16-byte aligned base
template <typename S, int N>
__device__ __forceinline__ void rl_load(const void* base, int64_t i, S raw[N]) {
    const S* p = reinterpret_cast<const S*>(base) + i;
    if (N == 1) raw[0] = p[0];
    else memcpy(raw, __builtin_assume_aligned(p, (N * sizeof(S) < 16 ? N * sizeof(S) : 16)), N * sizeof(S));
}

__device__ __forceinline__ double rl_wave_sum(double v) {
    for (int off = kWave / 2; off >= 1; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// ---- geometry, chunks ---------------------------------------------------------------------------------------------------------------------
constexpr int kLossQuantum = kBlock * 8;             // a chunk is a multiple of this: whole packets for every thread, both packet sizes
constexpr int kLossMaxChunks = 512;                  // per sample; 128^3 voxels -> 512 chunks of 4096
constexpr int kLossPacketMaxN = 8;                   // the packet route knows its plane count: one instantiation each for 1 .. 8

// the logits (B, n, Z, Y, X) as the kernels see them; the argument struct of a loss's kernels derives from it
struct LossGeom {
    int64_t sb, sn, sz, sy;                          // element strides of batch, plane, z, y (x: 1)
    int32_t V, X, Y;                                 // voxels of a sample, width, height
    int32_t B, n, dense, chunk, nchunks;             // n: the planes (regions / classes)
};

// voxel v of a sample (C order over z, y, x) -> its element offset in a logits plane
__device__ __forceinline__ int64_t loss_offset(const LossGeom& G, int64_t v) {
    if (G.dense) return v;
    const uint32_t row = (uint32_t)v / (uint32_t)G.X, col = (uint32_t)v - row * (uint32_t)G.X;
    const uint32_t z = row / (uint32_t)G.Y, y = row - z * (uint32_t)G.Y;
    return (int64_t)z * G.sz + (int64_t)y * G.sy + (int64_t)col;
}

// ---- labels -------------------------------------------------------------------------------------------------------------------------------
// One label as an integer and whether it is one: always for the integer kinds; a float that is none (NaN and inf among them) reads as -1.
__device__ __forceinline__ int64_t loss_label_value(float f, bool& whole) {
    whole = f == floorf(f) && fabsf(f) < 4.0e18f;
    return whole ? (int64_t)f : (int64_t)-1;
}
template <typename S>
__device__ __forceinline__ int64_t loss_label_value(S v, bool& whole) {
    whole = true;
    return (int64_t)v;
}

template <typename S, int N, typename F>
__device__ __forceinline__ void loss_labels_of(const void* base, int64_t i, F& each) {
    S raw[N];
    rl_load<S, N>(base, i, raw);
#pragma unroll
    for (int k = 0; k < N; ++k) {
        bool whole;
        const int64_t l = loss_label_value(raw[k], whole);
        each(k, l, whole);
    }
}

// N labels of a dense map of kind SEGM_REGION_LABELS_I64 / _I16 / _U8 / _F32 from element index i: each(k, label, whole) for voxel
// k = 0 .. N - 1.  What a value means (ignored, a class, out of range) is the caller's.
template <int N, typename F>
__device__ __forceinline__ void loss_labels(const void* base, int kind, int64_t i, F each) {
    switch (kind) {                                                       // uniform over the grid
    case SEGM_REGION_LABELS_I64: loss_labels_of<int64_t, N>(base, i, each); break;
    case SEGM_REGION_LABELS_I16: loss_labels_of<int16_t, N>(base, i, each); break;
    case SEGM_REGION_LABELS_U8: loss_labels_of<uint8_t, N>(base, i, each); break;
    default: loss_labels_of<float, N>(base, i, each); break;
    }
}

// ---- the reduction over the workgroup, the finish -----------------------------------------------------------------------------------------
// the waves have filled their rows of s_part: add them in the order 0 .. 3, one thread per slot, and store row `chunk` of sample b
template <int ROW>
__device__ __forceinline__ void loss_block_row(const double (&s_part)[kWavesPerBlock][ROW], double* part, int b, int nchunks, int chunk) {
    static_assert(ROW <= kBlock, "one thread per slot of the row");
    __syncthreads();
    if ((int)threadIdx.x < ROW) {
        double s = s_part[0][threadIdx.x];
        for (int w = 1; w < kWavesPerBlock; ++w) s += s_part[w][threadIdx.x];
        part[((int64_t)b * nchunks + chunk) * ROW + threadIdx.x] = s;
    }
}

// one workgroup per sample: wave w takes the slots w, w + 4, ...; lane l the rows l, l + 64, ...; then a shuffle tree.  A row of ROW
// doubles is GROUPS times MAX_N slots of sums per plane, of which n are in use -> sums[group][B][n], then the sums per sample ->
// sums[..][B].  (The row's shape is known where the kernel is compiled: the slot arithmetic costs nothing.)
template <int ROW, int GROUPS, int MAX_N>
__global__ void __launch_bounds__(kBlock) loss_finish_kernel(const double* part, double* sums, int nchunks, int n, int B) {
    constexpr int row = ROW, groups = GROUPS, max_n = MAX_N;
    const int b = blockIdx.x;
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    const double* rows = part + (int64_t)b * nchunks * row;
    const int64_t bn = (int64_t)B * n;
    for (int slot = wave; slot < row; slot += kWavesPerBlock) {
        const int q = slot / max_n, c = slot - q * max_n;
        if (q < groups && c >= n) continue;          // uniform over the wave
        double acc = 0.0;
        for (int r = lane; r < nchunks; r += kWave) acc += rows[(int64_t)r * row + slot];
        acc = rl_wave_sum(acc);
        if (lane == 0) {
            if (q < groups) sums[q * bn + (int64_t)b * n + c] = acc;
            else sums[groups * bn + (int64_t)c * B + b] = acc;
        }
    }
}

// ---- host ---------------------------------------------------------------------------------------------------------------------------------
static int32_t loss_chunk(int64_t voxels) {
    const int64_t per = (voxels + kLossMaxChunks - 1) / kLossMaxChunks;
    const int64_t chunk = ((per + kLossQuantum - 1) / kLossQuantum) * kLossQuantum;
    return (int32_t)(chunk < kLossQuantum ? kLossQuantum : chunk);
}

// the element size of a label map or of target planes, by SEGM_REGION_*
static size_t loss_label_esize(int kind) {
    switch (kind) {
    case SEGM_REGION_LABELS_I64: return 8;
    case SEGM_REGION_LABELS_I16: return 2;
    case SEGM_REGION_LABELS_U8: case SEGM_REGION_PLANES_U8: return 1;
    default: return 4;
    }
}

// bytes of the partial rows; 0 for a shape out of range
static size_t loss_workspace_bytes(int32_t batch, int32_t n, int32_t max_n, int64_t voxels, int row) {
    if (batch <= 0 || batch > 65535 || n < 1 || n > max_n || voxels < 1 || voxels >= ((int64_t)1 << 31)) return 0;
    const int32_t chunk = loss_chunk(voxels);
    const int64_t nchunks = (voxels + chunk - 1) / chunk;
    return (size_t)batch * (size_t)nchunks * row * sizeof(double);
}

// the part of the packet route's condition that the logits decide: every row starts at a multiple of 16 bytes (the strides of axes
// of size 1 are never used).  A loss adds the alignment of its own dense arrays.
template <typename A>
static bool loss_rows_aligned(const A* a, int32_t n, int64_t stride_n) {
    const int64_t p = a->dtype == SEGM_F32 ? 4 : 8;
    return a->width % p == 0 && (a->batch == 1 || a->stride_b % p == 0) && (n == 1 || stride_n % p == 0) &&
           (a->depth == 1 || a->stride_z % p == 0) && (a->height == 1 || a->stride_y % p == 0) && (uintptr_t)a->logits % 16 == 0;
}

// The argument checks of the losses' entries and the geometry; 0 or a SEGM_E_* status.  A: segm_region_loss_args or
// segm_softmax_dice_args (a is not NULL), n / max_n / stride_n its plane count, the limit and the plane stride, labels its dense
// array of `kind`; `own` is the status of the loss's own checks, reported where they stand: after the dtype, before the pointers.
template <typename A>
static int loss_setup(const A* a, int32_t n, int32_t max_n, int64_t stride_n, const void* labels, int kind, int own, LossGeom& G) {
    if (a->batch <= 0 || n < 1 || n > max_n || a->depth <= 0 || a->height <= 0 || a->width <= 0) return SEGM_E_SHAPE;
    if (a->batch > 65535) return SEGM_E_SHAPE;                            // the grid's y
    const int64_t voxels = (int64_t)a->depth * a->height * a->width;
    if (voxels >= ((int64_t)1 << 31)) return SEGM_E_SHAPE;
    if (a->stride_x != 1 || a->stride_b < 0 || stride_n < 0 || a->stride_z < 0 || a->stride_y < 0) return SEGM_E_SHAPE;
    if (a->dtype != SEGM_F32 && a->dtype != SEGM_F16 && a->dtype != SEGM_BF16) return SEGM_E_DTYPE;
    if (own != SEGM_OK) return own;
    if (!a->logits || !labels) return SEGM_E_NULL;
    if ((uintptr_t)a->logits % (a->dtype == SEGM_F32 ? 4 : 2) || (uintptr_t)labels % loss_label_esize(kind)) return SEGM_E_SHAPE;
    G.sb = a->stride_b; G.sn = stride_n; G.sz = a->stride_z; G.sy = a->stride_y;
    G.V = (int32_t)voxels; G.X = a->width; G.Y = a->height;
    G.B = a->batch; G.n = n;
    G.dense = (a->height == 1 || a->stride_y == a->width) && (a->depth == 1 || a->stride_z == (int64_t)a->width * a->height);
    G.chunk = loss_chunk(voxels);
    G.nchunks = (int32_t)((voxels + G.chunk - 1) / G.chunk);
    return SEGM_OK;
}

// the backward's grid: a packet (vec) or a voxel per thread
static dim3 loss_bwd_grid(const LossGeom& G, bool vec, int dtype) {
    const int64_t p = vec ? (dtype == SEGM_F32 ? 4 : 8) : 1;
    const int64_t packets = ((int64_t)G.V + p - 1) / p;
    return dim3((unsigned)((packets + kBlock - 1) / kBlock), (unsigned)G.B);
}

// K<T, true, n> for n = 1 .. kLossPacketMaxN on the packet route, K<T, false, 0> (the plane count read from the arguments) otherwise
#define SEGM_LOSS_CASE(K, T, NT) case NT: hipLaunchKernelGGL((K<T, true, NT>), grid, dim3(kBlock), 0, st, P); break
#define SEGM_LOSS_LAUNCH_T(K, T) \
    do { if (vec) switch (P.n) { SEGM_LOSS_CASE(K, T, 1); SEGM_LOSS_CASE(K, T, 2); SEGM_LOSS_CASE(K, T, 3); SEGM_LOSS_CASE(K, T, 4); \
                                 SEGM_LOSS_CASE(K, T, 5); SEGM_LOSS_CASE(K, T, 6); SEGM_LOSS_CASE(K, T, 7); SEGM_LOSS_CASE(K, T, 8); } \
         else hipLaunchKernelGGL((K<T, false, 0>), grid, dim3(kBlock), 0, st, P); } while (0)
// launches kernel template K for `dtype` with the caller's `vec`, `grid`, `st` and `P`
#define SEGM_LOSS_LAUNCH(K, dtype) \
    do { if ((dtype) == SEGM_F32) SEGM_LOSS_LAUNCH_T(K, float); \
         else if ((dtype) == SEGM_F16) SEGM_LOSS_LAUNCH_T(K, f16_t); \
         else SEGM_LOSS_LAUNCH_T(K, bf16_t); } while (0)
}  // namespace segm
