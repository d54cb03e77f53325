// The selection per class of a label volume, from the roots of its components (C ABI: segm_ccl_label_select).
//
// The reference's CT example (light_training/examples/AbdomenAtlas1.0Mini/4_predict_diffunet.py:87-109) writes `labels == i` per
// organ and `large_connected_domain` (light_training/prediction.py:17-27) keeps the largest component of one binary mask.  The roots
// of every class's components come from one labelled pass (ccl_roots.hip), their sizes from segm_ccl_sizes (postprocess.hip); here:
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

static_assert(kBlock == 256, "a thread per label value in the selection kernels");

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
