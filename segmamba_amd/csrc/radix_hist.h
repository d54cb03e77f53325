// Radix selection on float keys: what csrc/fingerprint.hip (order statistics of the foreground) and csrc/topk_ce.hip (the k-th largest
// per-voxel loss) share - the order-preserving 32-bit key of a float, the integer atomics of the histograms, and the aggregation of
// equal bins of a thread and of a wave in front of the LDS atomic (fingerprint.hip's head comment: "Same-address contention").
#pragma once
#include "segm_device.h"

namespace segm {

#ifdef SEGM_EMU
static inline void fg_add_lds(uint32_t* p, uint32_t v) { __atomic_fetch_add(p, v, __ATOMIC_RELAXED); }
static inline void fg_add_glb(uint32_t* p, uint32_t v) { __atomic_fetch_add(p, v, __ATOMIC_RELAXED); }
#else
__device__ __forceinline__ void fg_add_lds(uint32_t* p, uint32_t v) { __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ __forceinline__ void fg_add_glb(uint32_t* p, uint32_t v) { __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
#endif

// the order-preserving key of a float and back (csrc/resample.hip: zoom_key / zoom_unkey)
__device__ __forceinline__ uint32_t fg_key(float f) {
    const uint32_t b = __float_as_uint(f);
    return b ^ ((b >> 31) ? 0xffffffffu : 0x80000000u);
}
__device__ __forceinline__ float fg_unkey(uint32_t k) { return __uint_as_float(k ^ ((k >> 31) ? 0x80000000u : 0xffffffffu)); }

template <typename T> __device__ __forceinline__ T fg_wave_sum(T v) {
    for (int off = kWave / 2; off >= 1; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// Adds the four bins of a thread (-1: none) to the LDS histogram.  Every lane of the wave calls it (ballot and shuffles inside).
__device__ __forceinline__ void fg_hist_add4(uint32_t* s_hist, const int32_t bin[4], int lane) {
    // the thread: the voxels in the bin of its first counted voxel become one (bin, count); the others go out on their own
    int32_t b0 = -1;
    uint32_t n0 = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (bin[k] < 0) continue;
        if (b0 < 0) b0 = bin[k];
        if (bin[k] == b0) ++n0;
        else fg_add_lds(&s_hist[bin[k]], 1u);
    }
    // the wave: every lane that holds the bin of the first active lane adds through that lane
    const unsigned long long active = __ballot(b0 >= 0);
    if (active) {                                 // uniform over the wave
        const int leader = __builtin_ctzll(active);
        const int32_t lb = __shfl(b0, leader);
        const bool same = b0 == lb;
        const uint32_t tot = fg_wave_sum(same ? n0 : 0u);
        if (lane == leader) fg_add_lds(&s_hist[lb], tot);
        else if (b0 >= 0 && !same) fg_add_lds(&s_hist[b0], n0);
    }
}

}  // namespace segm
