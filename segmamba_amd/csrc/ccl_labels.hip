// Connected components of a LABEL volume, every class in one pass, and the per-class selection
// (C ABI: segm_ccl_label_roots, segm_ccl_label_select).
//
// The reference's CT example (light_training/examples/AbdomenAtlas1.0Mini/4_predict_diffunet.py:87-109) takes the argmax over 10
// classes and writes `labels == i` per organ; `large_connected_domain` (light_training/prediction.py:17-27) keeps the largest
// component of one binary mask.  Per organ through the binary entries of postprocess.hip that is nine passes over the volume; a
// labelled volume holds every organ's components at once: two voxels are joined iff they are face neighbours with the SAME NON-ZERO
// label.  The structure is that of the binary entry (64 x 4 x 4 tiles in LDS, face joins on agent-scope relaxed atomics, a flatten
// pass; the root of a component is its smallest linear index).  What does not carry over from a binary mask:
//   * a run along x ends where the label changes (`1 1 2 2` is two runs): the run starts are a ballot of "labelled and (lane 0 or the
//     label differs from the left lane's)", not the zeros of the mask;
//   * of adjacent voxels that both continue upwards only the first starts a union - but only when the two are one run: the second
//     still starts its own when it is a run start (stripes one voxel wide along x);
//   * the merge launch's `left` and `run` tests compare labels across the tile faces.
//   * label_best_kernel    per label the maximum of (size << 32) | root and the number of roots: LDS atomics per workgroup, then one
//                          64-bit atomic max and one add per label present in the workgroup (integers: any order, same bits).
//   * label_select_kernel  a voxel keeps its label iff its root is its label's winner / its component is large enough; labels with
//                          apply[l] == 0 pass through.  Workgroup 0 also writes `info` from the winners.
// Vector-memory and LDS atomics only.  The CPU emulation build (SEGM_EMU) states the same atomics with the compiler's __atomic builtins.
#include <stdlib.h>
#include <string.h>

#include "ccl_common.h"

namespace segm {

typedef unsigned long long u64_t;
#ifdef SEGM_EMU
template <int S> static inline void key_max(u64_t* p, u64_t v) { __atomic_fetch_max(p, v, __ATOMIC_RELAXED); }
template <int S> static inline void key_add(u64_t* p, u64_t v) { __atomic_fetch_add(p, v, __ATOMIC_RELAXED); }
#else
template <int S> __device__ __forceinline__ void key_max(u64_t* p, u64_t v) { __hip_atomic_fetch_max(p, v, __ATOMIC_RELAXED, S); }
template <int S> __device__ __forceinline__ void key_add(u64_t* p, u64_t v) { __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, S); }
#endif

static_assert(kBlock == 256, "a thread per label value in the selection kernels, a wave per z of the tile");

struct LabDev {
    const uint8_t* vol;
    int32_t* lab;
    int32_t* roots;
    int32_t D, H, W, N;
    int32_t tx, ty;                     // tiles along x and y
};

__global__ void __launch_bounds__(kBlock) lccl_tile_kernel(LabDev P) {
    __shared__ int32_t s_lab[kTileVox];
    __shared__ uint8_t s_val[kTileVox];
    __shared__ unsigned long long s_start[kTileRows];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t t = blockIdx.x;
    const uint32_t bx = t % (uint32_t)P.tx;
    t /= (uint32_t)P.tx;
    const uint32_t by = t % (uint32_t)P.ty, bz = t / (uint32_t)P.ty;
    const int x = (int)bx * kTX + lane, z = (int)bz * kTZ + wave;
    int v[kTY];
    // a run ends where the label changes: a voxel starts with the first voxel of its run along x
#pragma unroll
    for (int ly = 0; ly < kTY; ++ly) {
        const int row = wave * kTY + ly, y = (int)by * kTY + ly;
        v[ly] = 0;
        if (x < P.W && y < P.H && z < P.D) v[ly] = (int)P.vol[((int64_t)z * P.H + y) * P.W + x];
        const int left = __shfl(v[ly], (lane + 63) & 63);
        const unsigned long long s = __ballot(v[ly] != 0 && (lane == 0 || left != v[ly]) ? 1 : 0);
        if (lane == 0) s_start[row] = s;
        const unsigned long long before = s & ((2ull << lane) - 1ull);       // the run starts at or left of this lane
        s_val[row * kTX + lane] = (uint8_t)v[ly];
        s_lab[row * kTX + lane] = v[ly] != 0 ? row * kTX + 63 - __builtin_clzll(before | 1ull) : -1;
    }
    __syncthreads();
    // join with the row above in y and in z.  c: the voxel has the label of the one above.  Of two adjacent voxels of c the second
    // needs no union when it continues the first one's run (then the two above are one run as well), and only then.
#pragma unroll
    for (int ly = 0; ly < kTY; ++ly) {
        const int row = wave * kTY + ly;
        const unsigned long long inner = ~s_start[row];                      // not the first voxel of a run
        if (ly > 0) {
            const unsigned long long c = __ballot(v[ly] != 0 && (int)s_val[(row - 1) * kTX + lane] == v[ly] ? 1 : 0);
            if (((c & ~((c << 1) & inner)) >> lane) & 1ull) lab_union<kScopeWorkgroup>(s_lab, row * kTX + lane, (row - 1) * kTX + lane);
        }
        if (wave > 0) {
            const unsigned long long c = __ballot(v[ly] != 0 && (int)s_val[(row - kTY) * kTX + lane] == v[ly] ? 1 : 0);
            if (((c & ~((c << 1) & inner)) >> lane) & 1ull) lab_union<kScopeWorkgroup>(s_lab, row * kTX + lane, (row - kTY) * kTX + lane);
        }
    }
    __syncthreads();
    // local index order = global index order inside a tile, so the local root is the tile's smallest global index of the component
    for (int ly = 0; ly < kTY; ++ly) {
        const int row = wave * kTY + ly, y = (int)by * kTY + ly;
        if (!(x < P.W && y < P.H && z < P.D)) continue;
        int32_t l = s_lab[row * kTX + lane];
        if (l >= 0) {
            while (s_lab[l] != l) l = s_lab[l];
            const int rz = l / (kTX * kTY), ry = (l / kTX) % kTY, rx = l % kTX;
            l = (int32_t)((((int64_t)bz * kTZ + rz) * P.H + ((int64_t)by * kTY + ry)) * P.W + (int64_t)bx * kTX + rx);
        }
        P.lab[((int64_t)z * P.H + y) * P.W + x] = l;
    }
}

// voxels on the low faces of their tile are joined with the equally labelled neighbour across the face; every access to a label in
// this launch is an agent-scope relaxed atomic (lab_union)
__global__ void __launch_bounds__(kBlock) lccl_merge_kernel(LabDev P) {
    const uint32_t i = (uint32_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= (uint32_t)P.N) return;
    const uint8_t v = P.vol[i];
    if (v == 0) return;
    const uint32_t W = (uint32_t)P.W, HW = (uint32_t)P.H * W;
    const uint32_t z = i / HW, rem = i - z * HW, y = rem / W, x = rem - y * W;
    const bool onx = (x % kTX) == 0, ony = (y % kTY) == 0 && y > 0, onz = (z % kTZ) == 0 && z > 0;
    if (!(onx || ony || onz)) return;
    const bool left = x > 0 && P.vol[i - 1] == v;
    if (onx && left) lab_union<kScopeAgent>(P.lab, (int32_t)i, (int32_t)(i - 1));
    const bool run = left && !onx;                    // the left neighbour is in this tile, has this label: one component already
    if (ony && P.vol[i - W] == v && !(run && P.vol[i - W - 1] == v)) lab_union<kScopeAgent>(P.lab, (int32_t)i, (int32_t)(i - W));
    if (onz && P.vol[i - HW] == v && !(run && P.vol[i - HW - 1] == v)) lab_union<kScopeAgent>(P.lab, (int32_t)i, (int32_t)(i - HW));
}

__global__ void __launch_bounds__(kBlock) lccl_flatten_kernel(LabDev P) {
    const uint32_t i = (uint32_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= (uint32_t)P.N) return;
    int32_t l = P.lab[i];
    if (l >= 0)
        while (P.lab[l] != l) l = P.lab[l];
    P.roots[i] = l;
}

// ---- selection per label --------------------------------------------------------------------------------------------------------------
struct LabSelDev {
    const uint8_t* vol;
    const int32_t* roots;
    const int32_t* sizes;
    const uint8_t* apply;
    uint8_t* out;
    long long* info;
    u64_t* best;                        // [256][key, components]
    int32_t N, mode, min_size;
};

__global__ void __launch_bounds__(kBlock) label_best_kernel(LabSelDev P) {
    __shared__ u64_t s_key[256], s_n[256];
    s_key[threadIdx.x] = 0;
    s_n[threadIdx.x] = 0;
    __syncthreads();
    const int64_t base = (int64_t)blockIdx.x * kPostChunk;
    for (int k = 0; k < kPostVox; ++k) {
        const int64_t i = base + (int64_t)k * kBlock + threadIdx.x;
        if (i >= P.N) break;
        const int32_t s = P.sizes[i];
        if (s > 0) {                                  // voxel i is a root: its byte is the component's label
            const int l = P.vol[i];
            key_max<kScopeWorkgroup>(s_key + l, ((u64_t)(uint32_t)s << 32) | (u64_t)(uint32_t)i);   // equal counts: the later root wins
            key_add<kScopeWorkgroup>(s_n + l, 1ull);
        }
    }
    __syncthreads();
    if (s_n[threadIdx.x]) {
        key_max<kScopeAgent>(P.best + 2 * threadIdx.x, s_key[threadIdx.x]);
        key_add<kScopeAgent>(P.best + 2 * threadIdx.x + 1, s_n[threadIdx.x]);
    }
}

__global__ void __launch_bounds__(kBlock) label_select_kernel(LabSelDev P) {
    __shared__ int32_t s_win[256];
    __shared__ uint8_t s_apply[256];
    const u64_t key = P.best[2 * threadIdx.x];        // 0: the label is absent (a component has at least one voxel)
    s_win[threadIdx.x] = key ? (int32_t)(key & 0xffffffffull) : -1;
    s_apply[threadIdx.x] = P.apply ? P.apply[threadIdx.x] : (uint8_t)1;
    if (blockIdx.x == 0) {
        P.info[3 * threadIdx.x] = (long long)P.best[2 * threadIdx.x + 1];
        P.info[3 * threadIdx.x + 1] = key ? (long long)(key & 0xffffffffull) : -1ll;
        P.info[3 * threadIdx.x + 2] = (long long)(key >> 32);
    }
    __syncthreads();
    const int64_t base = (int64_t)blockIdx.x * kPostChunk;
    for (int k = 0; k < kPostVox; ++k) {
        const int64_t i = base + (int64_t)k * kBlock + threadIdx.x;
        if (i >= P.N) break;
        const uint8_t v = P.vol[i];
        bool on = v != 0;
        if (on && s_apply[v]) {
            const int32_t r = P.roots[i];
            on = P.mode == SEGM_CCL_LARGEST ? r == s_win[v] : (r >= 0 && P.sizes[r] >= P.min_size);
        }
        P.out[i] = on ? v : (uint8_t)0;
    }
}

}  // namespace segm

using namespace segm;

extern "C" size_t segm_ccl_label_roots_workspace_bytes(int64_t voxels) {
    if (voxels <= 0 || voxels > SEGM_CCL_MAX_VOXELS) return 0;
    return (size_t)voxels * sizeof(int32_t);
}

extern "C" int segm_ccl_label_roots(const segm_ccl_label_roots_args* a) {
    if (!a) return SEGM_E_NULL;
    if (!a->labels || !a->roots) return SEGM_E_NULL;
    if (!ccl_volume_ok(a->depth, a->height, a->width)) return SEGM_E_SHAPE;
    if ((uintptr_t)a->roots % sizeof(int32_t)) return SEGM_E_SHAPE;
    const int64_t N = (int64_t)a->depth * a->height * a->width;
    if (!a->workspace || a->workspace_bytes < segm_ccl_label_roots_workspace_bytes(N) || (uintptr_t)a->workspace % sizeof(int32_t)) return SEGM_E_WORKSPACE;
    LabDev P;
    memset(&P, 0, sizeof(P));
    P.vol = a->labels; P.lab = (int32_t*)a->workspace; P.roots = a->roots;
    P.D = a->depth; P.H = a->height; P.W = a->width; P.N = (int32_t)N;
    P.tx = (a->width + kTX - 1) / kTX;
    P.ty = (a->height + kTY - 1) / kTY;
    const int64_t tiles = (int64_t)P.tx * P.ty * ((a->depth + kTZ - 1) / kTZ);      // <= N: every tile holds a voxel
    hipStream_t st = (hipStream_t)a->stream;
    const dim3 flat((unsigned)((N + kBlock - 1) / kBlock)), block(kBlock);
    hipLaunchKernelGGL(lccl_tile_kernel, dim3((unsigned)tiles), block, 0, st, P);
    hipLaunchKernelGGL(lccl_merge_kernel, flat, block, 0, st, P);
    hipLaunchKernelGGL(lccl_flatten_kernel, flat, block, 0, st, P);
    return (int)hipGetLastError();
}

extern "C" size_t segm_ccl_label_select_workspace_bytes(int64_t voxels) {
    if (voxels <= 0 || voxels > SEGM_CCL_MAX_VOXELS) return 0;
    return (size_t)256 * 2 * sizeof(u64_t);
}

extern "C" int segm_ccl_label_select(const segm_ccl_label_select_args* a) {
    if (!a) return SEGM_E_NULL;
    if (!a->labels || !a->roots || !a->sizes || !a->out || !a->info) return SEGM_E_NULL;
    if (a->mode != SEGM_CCL_LARGEST && a->mode != SEGM_CCL_MIN_SIZE) return SEGM_E_SHAPE;
    if (a->min_size < 0) return SEGM_E_SHAPE;
    if (!ccl_volume_ok(a->depth, a->height, a->width)) return SEGM_E_SHAPE;
    if ((uintptr_t)a->roots % sizeof(int32_t) || (uintptr_t)a->sizes % sizeof(int32_t) || (uintptr_t)a->info % sizeof(int64_t)) return SEGM_E_SHAPE;
    const int64_t N = (int64_t)a->depth * a->height * a->width;
    const size_t need = segm_ccl_label_select_workspace_bytes(N);
    if (!a->workspace || a->workspace_bytes < need || (uintptr_t)a->workspace % sizeof(u64_t)) return SEGM_E_WORKSPACE;
    LabSelDev P;
    memset(&P, 0, sizeof(P));
    P.vol = a->labels; P.roots = a->roots; P.sizes = a->sizes; P.apply = a->apply; P.out = a->out; P.info = (long long*)a->info;
    P.best = (u64_t*)a->workspace;
    P.N = (int32_t)N; P.mode = a->mode; P.min_size = a->min_size;
    hipStream_t st = (hipStream_t)a->stream;
    if (hipMemsetAsync(a->workspace, 0, need, st) != hipSuccess) return (int)hipGetLastError();
    hipLaunchKernelGGL(label_best_kernel, dim3((unsigned)post_blocks(N)), dim3(kBlock), 0, st, P);
    hipLaunchKernelGGL(label_select_kernel, dim3((unsigned)post_blocks(N)), dim3(kBlock), 0, st, P);
    return (int)hipGetLastError();
}
