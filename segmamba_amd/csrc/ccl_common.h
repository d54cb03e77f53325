// What the connected-component sources share (ccl_roots.hip: the roots; postprocess.hip, ccl_labels.hip: sizes and selection): the
// relaxed atomics on labels and counts in both builds, the tile, the lock-free union-find on "labels only ever decrease", and the
// volume bound.
#pragma once
#include "segm_device.h"

namespace segm {

#ifdef SEGM_EMU
constexpr int kScopeWorkgroup = 0, kScopeAgent = 1;
template <int S> static inline int32_t lab_load(int32_t* p) { return __atomic_load_n(p, __ATOMIC_RELAXED); }
template <int S> static inline int32_t lab_min(int32_t* p, int32_t v) { return __atomic_fetch_min(p, v, __ATOMIC_RELAXED); }
template <int S> static inline int32_t cnt_add(int32_t* p, int32_t v) { return __atomic_fetch_add(p, v, __ATOMIC_RELAXED); }
#else
constexpr int kScopeWorkgroup = __HIP_MEMORY_SCOPE_WORKGROUP, kScopeAgent = __HIP_MEMORY_SCOPE_AGENT;
template <int S> __device__ __forceinline__ int32_t lab_load(int32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, S); }
template <int S> __device__ __forceinline__ int32_t lab_min(int32_t* p, int32_t v) { return __hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, S); }
template <int S> __device__ __forceinline__ int32_t cnt_add(int32_t* p, int32_t v) { return __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, S); }
#endif

constexpr int kTX = 64, kTY = 4, kTZ = 4;           // the tile: a wave per z, four rows along x per wave
constexpr int kTileRows = kTY * kTZ;
constexpr int kTileVox = kTX * kTileRows;
constexpr int kPostVox = 16;                        // voxels per thread of the counting passes
constexpr int kPostChunk = kBlock * kPostVox;

// the end of a's chain: labels never grow and a root names itself
template <int S> __device__ __forceinline__ int32_t lab_find(int32_t* L, int32_t a) {
    for (;;) {
        const int32_t p = lab_load<S>(L + a);
        if (p == a) return a;
        a = p;
    }
}

// joins the components of a and b: the larger root is hung below the smaller one.  When another thread got there first (`old` is not
// the root we saw) the link it made is kept by carrying on with `old` and b.
template <int S> __device__ __forceinline__ void lab_union(int32_t* L, int32_t a, int32_t b) {
    for (;;) {
        a = lab_find<S>(L, a);
        b = lab_find<S>(L, b);
        if (a == b) return;
        if (a < b) { const int32_t t = a; a = b; b = t; }
        const int32_t old = lab_min<S>(L + a, b);
        if (old == a) return;
        a = old;
    }
}

static inline bool ccl_volume_ok(int64_t d, int64_t h, int64_t w) {
    if (d <= 0 || h <= 0 || w <= 0) return false;
    if (d > SEGM_CCL_MAX_VOXELS || h > SEGM_CCL_MAX_VOXELS || w > SEGM_CCL_MAX_VOXELS) return false;
    if (d * h > SEGM_CCL_MAX_VOXELS) return false;
    return d * h * w <= SEGM_CCL_MAX_VOXELS;
}
static inline int64_t post_blocks(int64_t nvox) { return (nvox + kPostChunk - 1) / kPostChunk; }

}  // namespace segm
