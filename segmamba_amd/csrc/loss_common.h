// What the loss kernels that stream a volume once and keep fp64 sums share (region_loss.hip, dice_ce.hip).
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

}  // namespace segm
