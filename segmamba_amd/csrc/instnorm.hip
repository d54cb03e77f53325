// InstanceNorm3d (+ residual) (+ ReLU / LeakyReLU), forward and backward (C ABI: segm_instnorm_fwd / _bwd).
//
// Replaces the torch.nn.InstanceNorm3d -> (+ residual) -> activation chains of the SegMamba stem and decoder
// (reference model_segmamba/segmamba.py:96-130 GSC, :147,169-187; monai/networks/blocks/dynunet_block.py:98-111):
// no affine parameters, no running statistics, biased variance, eps inside the square root.
//
// An instance is one (batch, channel) volume of S contiguous elements (2 M at stage 0).  Everything here is HBM
// bound byte work: 16-byte accesses, every instance cut into slabs so that the grid is a few thousand workgroups
// whatever B*C is, fp32 statistics merged with Chan's (count, mean, M2) update.
//
//   forward   K1 stats   per (instance, slab): sum, sum of squares            -> partials
//             K2 apply   merge the instance's partials -> mean, rstd; y = act((x - mean) rstd + residual)
//   backward  K3 stats   g = dy act'(v);  per (instance, slab): sum g, sum g xhat  (g is parked in dresidual if asked)
//             K4 apply   dx = rstd (g - mean(g) - xhat mean(g xhat))
// The activation mask is taken from y when a residual was added (v is not recomputable from x alone), else from xhat.
//
// The residual tail y = act(IN(x) + IN(s)) of a block with a projection skip s (segm_instnorm_stats / _tail_fwd / _tail_bwd, the TAIL
// variants of K2 - K4) never stores IN(s) and never parks g:
//   forward   K1 over s, K1 over x (unless its producer summed the statistics), K2' y = act(xhat + T(shat)), both statistics written
//   backward  K3' the four sums  g, g xhat, T(g), T(g) shat  in one pass;  K4' dx and ds from T(g), g re-formed from dy and y
// T(.) rounds to the tensor type in registers where the two-call sequence rounds through memory; slabs, streaming modes, packets in
// flight, per-thread chains and the order over slabs are those of the passes replaced, the per-element arithmetic is shared with them:
// the tail gives the bits of segm_instnorm_fwd(s) -> segm_instnorm_fwd(x, residual) and their backwards (tests/norm_tail_checks.py),
// with 4 + 10 tensors of traffic per block instead of 6 + 12 and three launches fewer.  It inherits both deviations below unchanged.
//
// Two stated deviations (tests/norm_ref.py derives the per-element bounds, tests/norm_checks.py holds the kernels to them):
//   * dx is rounded twice when dresidual is wanted in a 16-bit type behind a LeakyReLU: K3 parks g ROUNDED to the type and K4 forms
//     dx from that rounded value, so dx carries rstd ulp(g) / 2 on top of its own final rounding (up to ~4 x the half-ulp bound of the
//     other cases).  A design trade - it saves K4 one read of y and of dy; fp32, ReLU (g = dy or 0) and no dresidual: not affected.
//   * the statistics are fp32 sums of x and x^2 (chains of at most 256 additions per thread, then Chan's merge): their error grows
//     with the condition number 1 + r^2 of E[x^2] - mean^2, r = |mean| / std:  |mean' - mean| rstd <= 2^-16 (1 + r),
//     |rstd' / rstd - 1| <= 2^-15 (1 + r^2)  - 3e-4 at r = 3, 2.7e-2 at r = 30, the limit of the sum-of-squares form.
#include <stdlib.h>
#include <string.h>

#include "segm_device.h"

namespace segm {

constexpr int kNormMaxSplit = 64;

struct NormDev {
    const void* x; const void* res; void* y;
    const void* dy; const void* ymask; void* dx; void* dres;
    float* mean; float* rstd;
    float2* part;
    int64_t S;
    int64_t xs, rs, ys, dys, dxs, drs;   // elements between consecutive instances of x, residual, y (ymask), dy, dx, dres: S when
                                         // dense, larger for volumes with a padded channel stride (ops_raw.volume_empty)
    int64_t slab;          // elements per slab (multiple of 8 * 256)
    int32_t nsplit;
    int32_t act;           // 0 none, 1 relu, 2 leaky relu
    float slope, eps;
    const float4* ext;     // forward: {count, sum, sum of squares, -} partials summed by the producer of x (conv3d_fwd.hip), or null
    int32_t next;          // per instance
    // the residual tail (TAIL kernels): `res` / `rs` is the skip tensor s, un-normalised; its statistics, its partials, its gradient
    float* mean3; float* rstd3;
    float2* part3;
    void* ds; int64_t dss;
};

// sum over the workgroup of two values; result valid in every thread
__device__ __forceinline__ float2 block_sum2(float a, float b, float2* lds) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        a += __shfl_xor(a, m);
        b += __shfl_xor(b, m);
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) lds[wave] = make_float2(a, b);
    __syncthreads();
    float2 r = make_float2(0.f, 0.f);
#pragma unroll
    for (int w = 0; w < kWavesPerBlock; ++w) { r.x += lds[w].x; r.y += lds[w].y; }
    return r;
}

__device__ __forceinline__ void slab_range(const NormDev& P, int split, int64_t& e0, int64_t& e1) {
    e0 = (int64_t)split * P.slab;
    e1 = e0 + P.slab;
    if (e1 > P.S) e1 = P.S;
    if (e0 > P.S) e0 = P.S;
}

// merges the (sum, sumsq) partials of an instance into mean / rstd (every thread gets the result)
__device__ __forceinline__ float2 merge_stats(const NormDev& P, const float2* part, int inst, float2* lds) {
    if (threadIdx.x == 0) {
        float n = 0.f, mean = 0.f, m2 = 0.f;
        for (int s = 0; s < P.nsplit; ++s) {
            int64_t e0, e1;
            slab_range(P, s, e0, e1);
            const float ns = (float)(e1 - e0);
            if (ns <= 0.f) continue;
            const float2 p = part[(int64_t)inst * P.nsplit + s];
            const float ms = p.x / ns;
            const float m2s = fmaxf(p.y - p.x * ms, 0.f);
            const float d = ms - mean, nt = n + ns;
            mean += d * (ns / nt);
            m2 += m2s + d * d * (n * ns / nt);
            n = nt;
        }
        const float var = m2 / n;
        lds[0] = make_float2(mean, 1.0f / sqrtf(var + P.eps));
    }
    __syncthreads();
    const float2 r = lds[0];
    __syncthreads();
    return r;
}

// Chan's update of (count, mean, M2) by another such triple (either may be empty)
__device__ __forceinline__ void chan_merge(float& n, float& mean, float& m2, float on, float omean, float om2) {
    if (on <= 0.f) return;
    if (n <= 0.f) { n = on; mean = omean; m2 = om2; return; }
    const float d = omean - mean, nt = n + on;
    mean += d * (on / nt);
    m2 += om2 + d * d * (n * on / nt);
    n = nt;
}

// the same merge over partials the PRODUCER of x summed (round 5: the statistics epilogue of the chained convolution kernels;
// hundreds of small partials per instance, not <= 64 slabs): every thread folds its strided share, the waves merge by a
// butterfly, thread 0 folds the waves - a fixed order, every thread gets the result
__device__ __forceinline__ float2 merge_ext(const NormDev& P, int inst, float2* lds) {
    __shared__ float wsum[kWavesPerBlock][3];
    float n = 0.f, mean = 0.f, m2 = 0.f;
    const float4* p = P.ext + (int64_t)inst * P.next;
    for (int i = threadIdx.x; i < P.next; i += kBlock) {
        const float4 v = p[i];
        if (v.x > 0.f) {
            const float ms = v.y / v.x;
            chan_merge(n, mean, m2, v.x, ms, fmaxf(v.z - v.y * ms, 0.f));
        }
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const float on = __shfl_xor(n, m), om = __shfl_xor(mean, m), o2 = __shfl_xor(m2, m);
        // both partners must fold in the SAME order (lower lane first), or the two halves of the butterfly drift apart by rounding
        if ((threadIdx.x & m) == 0) chan_merge(n, mean, m2, on, om, o2);
        else { float a = on, b = om, c = o2; chan_merge(a, b, c, n, mean, m2); n = a; mean = b; m2 = c; }
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) { wsum[wave][0] = n; wsum[wave][1] = mean; wsum[wave][2] = m2; }
    __syncthreads();
    if (threadIdx.x == 0) {
        float tn = 0.f, tm = 0.f, t2 = 0.f;
#pragma unroll
        for (int w = 0; w < kWavesPerBlock; ++w) chan_merge(tn, tm, t2, wsum[w][0], wsum[w][1], wsum[w][2]);
        lds[0] = make_float2(tm, 1.0f / sqrtf(t2 / tn + P.eps));
    }
    __syncthreads();
    const float2 r = lds[0];
    __syncthreads();
    return r;
}

// NT: non-temporal accesses for what is streamed once; U: packets a thread has in flight per tensor
template <typename T, bool VEC, bool NT = false, int U = 4>
__global__ void __launch_bounds__(kBlock) inorm_fwd_stats_kernel(NormDev P) {
    using Pk = Pack<T, VEC>;
    __shared__ float2 lds[kWavesPerBlock];
    const int split = blockIdx.x, inst = blockIdx.y;
    const T* x = reinterpret_cast<const T*>(P.x) + (int64_t)inst * P.xs;
    int64_t e0, e1;
    slab_range(P, split, e0, e1);
    float s[U], q[U];
#pragma unroll
    for (int k = 0; k < U; ++k) s[k] = q[k] = 0.f;
    const int64_t step = (int64_t)kBlock * Pk::N;
    int64_t i = e0 + (int64_t)threadIdx.x * Pk::N;
    for (; i + (U - 1) * step < e1; i += U * step) {       // U independent packets in flight per thread
        Pk p[U];
#pragma unroll
        for (int k = 0; k < U; ++k) p[k].template load<NT>(x + i + k * step);
#pragma unroll
        for (int k = 0; k < U; ++k)
#pragma unroll
            for (int j = 0; j < Pk::N; ++j) { s[k] += p[k].v[j]; q[k] = fmaf(p[k].v[j], p[k].v[j], q[k]); }
    }
    for (; i < e1; i += step) {
        Pk p;
        p.template load<NT>(x + i);
#pragma unroll
        for (int j = 0; j < Pk::N; ++j) { s[0] += p.v[j]; q[0] = fmaf(p.v[j], p.v[j], q[0]); }
    }
    float ss = 0.f, qq = 0.f;
    if constexpr (U == 4) { ss = (s[0] + s[1]) + (s[2] + s[3]); qq = (q[0] + q[1]) + (q[2] + q[3]); }
    else {
#pragma unroll
        for (int k = 0; k < U; ++k) { ss += s[k]; qq += q[k]; }
    }
    const float2 r = block_sum2(ss, qq, lds);
    if (threadIdx.x == 0) P.part[(int64_t)inst * P.nsplit + split] = r;
}

__device__ __forceinline__ float act_fwd(float v, int act, float slope) {
    if (act == 0) return v;
    return v > 0.f ? v : v * slope;                      // relu: slope == 0
}

// fp16 only: the compiler may fold the multiply that forms a value into its conversion to the type (v_fma_mixlo_f16: one rounding of
// the exact product, not two) and chooses element by element.  A value pinned in a register before it is converted is rounded the
// same way wherever it is formed - what makes the tail passes bit-equal to the passes they replace.  (bf16 and fp32 have no such form.)
template <typename T> struct IsF16 { static constexpr bool value = false; };
template <> struct IsF16<f16_t> { static constexpr bool value = true; };
template <typename T> __device__ __forceinline__ void pin_f16(float& v) {
#ifndef SEGM_EMU
    if constexpr (IsF16<T>::value) asm volatile("" : "+v"(v));
#endif
}

// the value a tensor of type T would have held
template <typename T> __device__ __forceinline__ float round_to(float v) {
    pin_f16<T>(v);
    return to_f32(from_f32<T>(v));
}

// TAIL: `res` is the un-normalised skip s with the partials of its own statistics pass in part3; the pass adds IN(s) rounded to T,
// the residual tensor the two-call sequence stores and reads back, and writes the statistics of both tensors
template <typename T, bool VEC, bool NT = false, int U = 2, bool TAIL = false>
__global__ void __launch_bounds__(kBlock) inorm_fwd_apply_kernel(NormDev P) {
    using Pk = Pack<T, VEC>;
    __shared__ float2 lds[kWavesPerBlock];
    const int split = blockIdx.x, inst = blockIdx.y;
    const float2 st = P.ext ? merge_ext(P, inst, lds) : merge_stats(P, P.part, inst, lds);
    const float mean = st.x, rstd = st.y;
    if (split == 0 && threadIdx.x == 0) { P.mean[inst] = mean; P.rstd[inst] = rstd; }
    float rstd3 = 0.f, shift3 = 0.f;
    if constexpr (TAIL) {
        const float2 s3 = merge_stats(P, P.part3, inst, lds);
        if (split == 0 && threadIdx.x == 0) { P.mean3[inst] = s3.x; P.rstd3[inst] = s3.y; }
        rstd3 = s3.y;
        shift3 = -s3.x * s3.y;
    }
    const T* x = reinterpret_cast<const T*>(P.x) + (int64_t)inst * P.xs;
    const T* res = P.res ? reinterpret_cast<const T*>(P.res) + (int64_t)inst * P.rs : nullptr;
    T* y = reinterpret_cast<T*>(P.y) + (int64_t)inst * P.ys;
    const float slope = P.act == 1 ? 0.f : P.slope;
    const float shift = -mean * rstd;
    int64_t e0, e1;
    slab_range(P, split, e0, e1);
    const int64_t step = (int64_t)kBlock * Pk::N;
    auto one = [&](Pk& a, const Pk& r) {
#pragma unroll
        for (int j = 0; j < Pk::N; ++j) {
            float v = fmaf(a.v[j], rstd, shift);
            if constexpr (TAIL) v += round_to<T>(fmaf(r.v[j], rstd3, shift3));
            else if (res) v += r.v[j];
            a.v[j] = act_fwd(v, P.act, slope);
            pin_f16<T>(a.v[j]);
        }
    };
    int64_t i = e0 + (int64_t)threadIdx.x * Pk::N;
    for (; i + (U - 1) * step < e1; i += U * step) {
        Pk a[U], r[U];
#pragma unroll
        for (int k = 0; k < U; ++k) a[k].template load<NT>(x + i + k * step);
        if (res) {
#pragma unroll
            for (int k = 0; k < U; ++k) r[k].template load<NT>(res + i + k * step);
        }
#pragma unroll
        for (int k = 0; k < U; ++k) {
            one(a[k], r[k]);
            a[k].template store<NT>(y + i + k * step);
        }
    }
    for (; i < e1; i += step) {
        Pk a, r;
        a.template load<NT>(x + i);
        if (res) r.template load<NT>(res + i);
        one(a, r);
        a.template store<NT>(y + i);
    }
}

// g = dy * act'(v) for one packet
template <typename Pk>
__device__ __forceinline__ void grad_through_act(Pk& g, const Pk& xh, const Pk& ym, bool use_y, int act, float slope) {
    if (act == 0) return;
#pragma unroll
    for (int j = 0; j < Pk::N; ++j) {
        const float v = use_y ? ym.v[j] : xh.v[j];
        g.v[j] = v > 0.f ? g.v[j] : g.v[j] * slope;
    }
}

// TAIL: one pass for both branches of a residual tail.  Beside sum g and sum g xhat of x it sums gr = g rounded to T and gr shat for the
// skip s (`res`), what the statistics pass of the skip's own InstanceNorm sums from the parked g; nothing is parked
template <typename T, bool VEC, bool NT = false, int U = 2, bool TAIL = false>
__global__ void __launch_bounds__(kBlock) inorm_bwd_stats_kernel(NormDev P) {
    using Pk = Pack<T, VEC>;
    __shared__ float2 lds[kWavesPerBlock];
    const int split = blockIdx.x, inst = blockIdx.y;
    const T* x = reinterpret_cast<const T*>(P.x) + (int64_t)inst * P.xs;
    const T* sk = TAIL ? reinterpret_cast<const T*>(P.res) + (int64_t)inst * P.rs : nullptr;
    const float rstd3 = TAIL ? P.rstd3[inst] : 0.f;
    const float shift3 = TAIL ? -P.mean3[inst] * rstd3 : 0.f;
    const T* dy = reinterpret_cast<const T*>(P.dy) + (int64_t)inst * P.dys;
    const T* ym = P.ymask ? reinterpret_cast<const T*>(P.ymask) + (int64_t)inst * P.ys : nullptr;
    T* dres = P.dres ? reinterpret_cast<T*>(P.dres) + (int64_t)inst * P.drs : nullptr;
    const float mean = P.mean[inst], rstd = P.rstd[inst];
    const float shift = -mean * rstd;
    const float slope = P.act == 1 ? 0.f : P.slope;
    const bool use_y = ym != nullptr;
    int64_t e0, e1;
    slab_range(P, split, e0, e1);
    float sg[U], sgx[U], sh[U], shs[U];
#pragma unroll
    for (int k = 0; k < U; ++k) sg[k] = sgx[k] = sh[k] = shs[k] = 0.f;
    const int64_t step = (int64_t)kBlock * Pk::N;
    // (x, dy and y are read again by the apply pass: never non-temporal; the parked g is)
    auto one = [&](Pk& xa, Pk& ga, const Pk& ya, float& a, float& b, int64_t at) {
#pragma unroll
        for (int j = 0; j < Pk::N; ++j) xa.v[j] = fmaf(xa.v[j], rstd, shift);
        grad_through_act(ga, xa, ya, use_y, P.act, slope);
        if (TAIL || dres) {                                 // g is about to be rounded to the type
#pragma unroll
            for (int j = 0; j < Pk::N; ++j) pin_f16<T>(ga.v[j]);
        }
#pragma unroll
        for (int j = 0; j < Pk::N; ++j) { a += ga.v[j]; b = fmaf(ga.v[j], xa.v[j], b); }
        if (dres) ga.store(dres + at);
    };
    // the skip branch: what `one` does in the skip's own pass (no activation), on the g that pass would read back
    auto skip = [&](Pk& sa, const Pk& ga, float& a, float& b) {
#pragma unroll
        for (int j = 0; j < Pk::N; ++j) {
            sa.v[j] = fmaf(sa.v[j], rstd3, shift3);
            const float gr = round_to<T>(ga.v[j]);
            a += gr;
            b = fmaf(gr, sa.v[j], b);
        }
    };
    int64_t i = e0 + (int64_t)threadIdx.x * Pk::N;
    for (; i + (U - 1) * step < e1; i += U * step) {
        Pk xa[U], ga[U], ya[U], sa[TAIL ? U : 1];
#pragma unroll
        for (int k = 0; k < U; ++k) { xa[k].template load<NT>(x + i + k * step); ga[k].template load<NT>(dy + i + k * step); }
        if (use_y && P.act) {
#pragma unroll
            for (int k = 0; k < U; ++k) ya[k].template load<NT>(ym + i + k * step);
        }
        if constexpr (TAIL) {
#pragma unroll
            for (int k = 0; k < U; ++k) sa[k].template load<NT>(sk + i + k * step);
        }
#pragma unroll
        for (int k = 0; k < U; ++k) {
            one(xa[k], ga[k], ya[k], sg[k], sgx[k], i + k * step);
            if constexpr (TAIL) skip(sa[k], ga[k], sh[k], shs[k]);
        }
    }
    for (; i < e1; i += step) {
        Pk xa, ga, ya;
        xa.template load<NT>(x + i); ga.template load<NT>(dy + i);
        if (use_y && P.act) ya.template load<NT>(ym + i);
        one(xa, ga, ya, sg[0], sgx[0], i);
        if constexpr (TAIL) {
            Pk sa;
            sa.template load<NT>(sk + i);
            skip(sa, ga, sh[0], shs[0]);
        }
    }
    float a = 0.f, b = 0.f;
#pragma unroll
    for (int k = 0; k < U; ++k) { a += sg[k]; b += sgx[k]; }
    const float2 r = block_sum2(a, b, lds);
    if (threadIdx.x == 0) P.part[(int64_t)inst * P.nsplit + split] = r;
    if constexpr (TAIL) {
        float c = 0.f, d = 0.f;
#pragma unroll
        for (int k = 0; k < U; ++k) { c += sh[k]; d += shs[k]; }
        const float2 r3 = block_sum2(c, d, lds);
        if (threadIdx.x == 0) P.part3[(int64_t)inst * P.nsplit + split] = r3;
    }
}

// the means of an instance's (sum g, sum g xhat) partials, summed by thread 0 in slab order into *out
__device__ __forceinline__ void mean_partials(const NormDev& P, const float2* part, int inst, float2* out) {
    float a = 0.f, b = 0.f;
    for (int s = 0; s < P.nsplit; ++s) {
        const float2 p = part[(int64_t)inst * P.nsplit + s];
        a += p.x; b += p.y;
    }
    *out = make_float2(a / (float)P.S, b / (float)P.S);
}

__device__ __forceinline__ float norm_dx(float g, float xh, float mg, float mgx, float rstd) {
    return rstd * (g - mg - xh * mgx);
}

// TAIL: g is formed from dy and y and rounded to T in registers (the value the two-call sequence parks and reads back); from it
// dx for x and ds for the skip s (`res`), each with its own statistics and partials
template <typename T, bool VEC, bool NT = false, int U = 1, bool TAIL = false>
__global__ void __launch_bounds__(kBlock) inorm_bwd_apply_kernel(NormDev P) {
    using Pk = Pack<T, VEC>;
    __shared__ float2 lds[kWavesPerBlock];
    const int split = blockIdx.x, inst = blockIdx.y;
    if (threadIdx.x == 0) {
        mean_partials(P, P.part, inst, &lds[0]);
        if constexpr (TAIL) mean_partials(P, P.part3, inst, &lds[1]);
    }
    __syncthreads();
    const float mg = lds[0].x, mgx = lds[0].y;
    const float mg3 = TAIL ? lds[1].x : 0.f, mgx3 = TAIL ? lds[1].y : 0.f;
    const T* sk = TAIL ? reinterpret_cast<const T*>(P.res) + (int64_t)inst * P.rs : nullptr;
    T* ds = TAIL ? reinterpret_cast<T*>(P.ds) + (int64_t)inst * P.dss : nullptr;
    const float rstd3 = TAIL ? P.rstd3[inst] : 0.f;
    const float shift3 = TAIL ? -P.mean3[inst] * rstd3 : 0.f;
    const T* x = reinterpret_cast<const T*>(P.x) + (int64_t)inst * P.xs;
    const T* dy = reinterpret_cast<const T*>(P.dy) + (int64_t)inst * P.dys;
    const T* ym = P.ymask ? reinterpret_cast<const T*>(P.ymask) + (int64_t)inst * P.ys : nullptr;
    const T* gsrc = P.dres ? reinterpret_cast<const T*>(P.dres) + (int64_t)inst * P.drs : nullptr;     // g parked by the stats pass
    T* dx = reinterpret_cast<T*>(P.dx) + (int64_t)inst * P.dxs;
    const float mean = P.mean[inst], rstd = P.rstd[inst];
    const float shift = -mean * rstd;
    const float slope = P.act == 1 ? 0.f : P.slope;
    const bool use_y = ym != nullptr;
    int64_t e0, e1;
    slab_range(P, split, e0, e1);
    const int64_t step = (int64_t)kBlock * Pk::N;
    auto one = [&](Pk& xa, Pk& ga, const Pk& ya) {
#pragma unroll
        for (int j = 0; j < Pk::N; ++j) xa.v[j] = fmaf(xa.v[j], rstd, shift);
        if (!gsrc) grad_through_act(ga, xa, ya, use_y, P.act, slope);
#pragma unroll
        for (int j = 0; j < Pk::N; ++j) { ga.v[j] = norm_dx(ga.v[j], xa.v[j], mg, mgx, rstd); pin_f16<T>(ga.v[j]); }
    };
    // both branches from the rounded g: sa -> ds, ga -> dx
    auto both = [&](Pk& xa, Pk& ga, const Pk& ya, Pk& sa) {
#pragma unroll
        for (int j = 0; j < Pk::N; ++j) xa.v[j] = fmaf(xa.v[j], rstd, shift);
        grad_through_act(ga, xa, ya, use_y, P.act, slope);
#pragma unroll
        for (int j = 0; j < Pk::N; ++j) {
            const float gr = round_to<T>(ga.v[j]);
            ga.v[j] = norm_dx(gr, xa.v[j], mg, mgx, rstd);
            sa.v[j] = norm_dx(gr, fmaf(sa.v[j], rstd3, shift3), mg3, mgx3, rstd3);
            pin_f16<T>(ga.v[j]);
            pin_f16<T>(sa.v[j]);
        }
    };
    int64_t i = e0 + (int64_t)threadIdx.x * Pk::N;
    for (; i + (U - 1) * step < e1; i += U * step) {
        Pk xa[U], ga[U], ya[U], sa[TAIL ? U : 1];
#pragma unroll
        for (int k = 0; k < U; ++k) {
            xa[k].template load<NT>(x + i + k * step);
            if (gsrc) ga[k].load(gsrc + i + k * step);         // (the residual's gradient: read again by its consumer)
            else ga[k].template load<NT>(dy + i + k * step);
        }
        if (!gsrc && use_y && P.act) {
#pragma unroll
            for (int k = 0; k < U; ++k) ya[k].template load<NT>(ym + i + k * step);
        }
        if constexpr (TAIL) {
#pragma unroll
            for (int k = 0; k < U; ++k) sa[k].template load<NT>(sk + i + k * step);
        }
#pragma unroll
        for (int k = 0; k < U; ++k) {
            if constexpr (TAIL) {
                both(xa[k], ga[k], ya[k], sa[k]);
                sa[k].template store<NT>(ds + i + k * step);
            } else one(xa[k], ga[k], ya[k]);
            ga[k].template store<NT>(dx + i + k * step);
        }
    }
    if constexpr (U > 1) {
        for (; i < e1; i += step) {
            Pk xa, ga, ya;
            xa.template load<NT>(x + i);
            if (gsrc) ga.load(gsrc + i);
            else {
                ga.template load<NT>(dy + i);
                if (use_y && P.act) ya.template load<NT>(ym + i);
            }
            if constexpr (TAIL) {
                Pk sa;
                sa.template load<NT>(sk + i);
                both(xa, ga, ya, sa);
                sa.template store<NT>(ds + i);
            } else one(xa, ga, ya);
            ga.template store<NT>(dx + i);
        }
    }
}

// A/B knobs of these streaming passes (round 5; profiles/r05_inorm_tune.log), read per call
static int norm_knob(const char* name, int dflt) {
    const char* e = getenv(name);
    return e && *e ? atoi(e) : dflt;
}

static void norm_plan(int instances, int64_t S, int vecn, int& nsplit, int64_t& slab) {
    const int64_t quantum = (int64_t)kBlock * vecn * 4;           // the stats loop's full stride
    const int target = norm_knob("SEGM_NORM_WGS", 4096);
    int64_t want = (target + instances - 1) / instances;          // ~`target` workgroups in total
    const int64_t maxs = (S + quantum - 1) / quantum;
    if (want > maxs) want = maxs;
    if (want > kNormMaxSplit) want = kNormMaxSplit;
    if (want < 1) want = 1;
    slab = (S + want - 1) / want;
    slab = (slab + quantum - 1) / quantum * quantum;
    nsplit = (int)((S + slab - 1) / slab);
}

static bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
// an instance stride argument: 0 = dense (the spatial size); never smaller than the spatial size
static bool norm_stride(int64_t given, int64_t spatial, int64_t& out) {
    out = given ? given : spatial;
    return out >= spatial;
}

// How a pass streams, by the bytes of ONE of its tensors (profiles/r05_inorm_tune.log, _tune2.log; 2 x 48 x 128^3 bf16 = 403 MB,
// 2 x 96 x 64^3 = 101 MB):
//   mode 0  < 64 MB    plain accesses, 2 / 1 packets in flight in the apply passes (rounds 1 - 4; the 256 MB last-level cache holds it)
//   mode 1  >= 64 MB   apply passes: non-temporal loads and stores, 4 packets in flight; backward statistics 4 in flight
//   mode 2  >= 192 MB  + non-temporal loads in the backward statistics pass (nothing survives between the passes anyway).  NOT in the
//                      forward statistics pass: plain loads leave part of x in the last-level cache for the apply pass behind it
//                      (403 MB: 0.200 ms with plain statistics loads, 0.212 ms without)
// 403 MB: forward 0.243 -> 0.200 ms (6.0 TB/s), with a residual 0.313 -> 0.259, backward 0.377 -> 0.326 (6.2 TB/s).
// SEGM_NORM_NT = 0 / 1 / 2 forces a mode (A/B).
static int norm_mode(int instances, int64_t S, size_t esize) {
    const int forced = norm_knob("SEGM_NORM_NT", -1);
    if (forced >= 0) return forced > 2 ? 2 : forced;
    const double bytes = (double)instances * (double)S * (double)esize;
    return bytes >= 192e6 ? 2 : (bytes >= 64e6 ? 1 : 0);
}

template <typename T>
static int launch_norm_fwd(NormDev& P, int instances, bool vec, hipStream_t st) {
    dim3 grid(P.nsplit, instances);
    const int mode = vec ? norm_mode(instances, P.S, sizeof(T)) : 0;
    if (vec) {
        if (!P.ext) hipLaunchKernelGGL((inorm_fwd_stats_kernel<T, true>), grid, dim3(kBlock), 0, st, P);
        if (mode) hipLaunchKernelGGL((inorm_fwd_apply_kernel<T, true, true, 4>), grid, dim3(kBlock), 0, st, P);
        else hipLaunchKernelGGL((inorm_fwd_apply_kernel<T, true>), grid, dim3(kBlock), 0, st, P);
    } else {
        if (!P.ext) hipLaunchKernelGGL((inorm_fwd_stats_kernel<T, false>), grid, dim3(kBlock), 0, st, P);
        hipLaunchKernelGGL((inorm_fwd_apply_kernel<T, false>), grid, dim3(kBlock), 0, st, P);
    }
    return (int)hipGetLastError();
}

template <typename T>
static int launch_norm_bwd(NormDev& P, int instances, bool vec, hipStream_t st) {
    dim3 grid(P.nsplit, instances);
    const int mode = vec ? norm_mode(instances, P.S, sizeof(T)) : 0;
    if (vec) {
        if (mode == 2) hipLaunchKernelGGL((inorm_bwd_stats_kernel<T, true, true, 4>), grid, dim3(kBlock), 0, st, P);
        else if (mode == 1) hipLaunchKernelGGL((inorm_bwd_stats_kernel<T, true, false, 4>), grid, dim3(kBlock), 0, st, P);
        else hipLaunchKernelGGL((inorm_bwd_stats_kernel<T, true>), grid, dim3(kBlock), 0, st, P);
        if (mode) hipLaunchKernelGGL((inorm_bwd_apply_kernel<T, true, true, 4>), grid, dim3(kBlock), 0, st, P);
        else hipLaunchKernelGGL((inorm_bwd_apply_kernel<T, true>), grid, dim3(kBlock), 0, st, P);
    } else {
        hipLaunchKernelGGL((inorm_bwd_stats_kernel<T, false>), grid, dim3(kBlock), 0, st, P);
        hipLaunchKernelGGL((inorm_bwd_apply_kernel<T, false>), grid, dim3(kBlock), 0, st, P);
    }
    return (int)hipGetLastError();
}

// the statistics pass alone (the skip of a residual tail: its partials wait for the tail's apply pass)
template <typename T>
static int launch_norm_stats(NormDev& P, int instances, bool vec, hipStream_t st) {
    dim3 grid(P.nsplit, instances);
    if (vec) hipLaunchKernelGGL((inorm_fwd_stats_kernel<T, true>), grid, dim3(kBlock), 0, st, P);
    else hipLaunchKernelGGL((inorm_fwd_stats_kernel<T, false>), grid, dim3(kBlock), 0, st, P);
    return (int)hipGetLastError();
}

// the tail passes stream as the passes they replace: the same slabs, modes and packets in flight
template <typename T>
static int launch_norm_tail_fwd(NormDev& P, int instances, bool vec, hipStream_t st) {
    dim3 grid(P.nsplit, instances);
    const int mode = vec ? norm_mode(instances, P.S, sizeof(T)) : 0;
    if (vec) {
        if (!P.ext) hipLaunchKernelGGL((inorm_fwd_stats_kernel<T, true>), grid, dim3(kBlock), 0, st, P);
        if (mode) hipLaunchKernelGGL((inorm_fwd_apply_kernel<T, true, true, 4, true>), grid, dim3(kBlock), 0, st, P);
        else hipLaunchKernelGGL((inorm_fwd_apply_kernel<T, true, false, 2, true>), grid, dim3(kBlock), 0, st, P);
    } else {
        if (!P.ext) hipLaunchKernelGGL((inorm_fwd_stats_kernel<T, false>), grid, dim3(kBlock), 0, st, P);
        hipLaunchKernelGGL((inorm_fwd_apply_kernel<T, false, false, 2, true>), grid, dim3(kBlock), 0, st, P);
    }
    return (int)hipGetLastError();
}

template <typename T>
static int launch_norm_tail_bwd(NormDev& P, int instances, bool vec, hipStream_t st) {
    dim3 grid(P.nsplit, instances);
    const int mode = vec ? norm_mode(instances, P.S, sizeof(T)) : 0;
    if (vec) {
        if (mode == 2) hipLaunchKernelGGL((inorm_bwd_stats_kernel<T, true, true, 4, true>), grid, dim3(kBlock), 0, st, P);
        else if (mode == 1) hipLaunchKernelGGL((inorm_bwd_stats_kernel<T, true, false, 4, true>), grid, dim3(kBlock), 0, st, P);
        else hipLaunchKernelGGL((inorm_bwd_stats_kernel<T, true, false, 2, true>), grid, dim3(kBlock), 0, st, P);
        if (mode) hipLaunchKernelGGL((inorm_bwd_apply_kernel<T, true, true, 4, true>), grid, dim3(kBlock), 0, st, P);
        else hipLaunchKernelGGL((inorm_bwd_apply_kernel<T, true, false, 1, true>), grid, dim3(kBlock), 0, st, P);
    } else {
        hipLaunchKernelGGL((inorm_bwd_stats_kernel<T, false, false, 2, true>), grid, dim3(kBlock), 0, st, P);
        hipLaunchKernelGGL((inorm_bwd_apply_kernel<T, false, false, 1, true>), grid, dim3(kBlock), 0, st, P);
    }
    return (int)hipGetLastError();
}

static int vec_width(int dtype) { return dtype == SEGM_F32 ? 4 : 8; }

}  // namespace segm

using namespace segm;

extern "C" size_t segm_instnorm_workspace_bytes(int32_t instances, int64_t spatial) {
    if (instances <= 0 || spatial <= 0) return 0;
    return (size_t)instances * kNormMaxSplit * sizeof(float2);
}

static int norm_common(int32_t instances, int64_t spatial, int32_t dtype, int32_t act, const void* ws, size_t ws_bytes) {
    if (instances <= 0 || spatial <= 0) return SEGM_E_SHAPE;
    if (dtype != SEGM_F32 && dtype != SEGM_F16 && dtype != SEGM_BF16) return SEGM_E_DTYPE;
    if (act < 0 || act > 2) return SEGM_E_SHAPE;
    if (!ws || ws_bytes < segm_instnorm_workspace_bytes(instances, spatial)) return SEGM_E_WORKSPACE;
    return SEGM_OK;
}

extern "C" int segm_instnorm_fwd(const segm_instnorm_fwd_args* a) {
    if (!a) return SEGM_E_NULL;
    int rc = norm_common(a->instances, a->spatial, a->dtype, a->act, a->workspace, a->workspace_bytes);
    if (rc != SEGM_OK) return rc;
    if (!a->x || !a->y || !a->mean || !a->rstd) return SEGM_E_NULL;
    NormDev P;
    memset(&P, 0, sizeof(P));
    P.x = a->x; P.res = a->residual; P.y = a->y; P.mean = a->mean; P.rstd = a->rstd;
    P.part = (float2*)a->workspace;
    P.S = a->spatial; P.act = a->act; P.slope = a->slope; P.eps = a->eps;
    if (a->stats_partials) {
        if (a->stats_nparts <= 0 || ((uintptr_t)a->stats_partials & 15)) return SEGM_E_SHAPE;
        P.ext = (const float4*)a->stats_partials; P.next = a->stats_nparts;
    }
    if (!norm_stride(a->x_instance_stride, a->spatial, P.xs) || !norm_stride(a->residual_instance_stride, a->spatial, P.rs) ||
        !norm_stride(a->y_instance_stride, a->spatial, P.ys))
        return SEGM_E_SHAPE;
    const int vn = vec_width(a->dtype);
    const bool vec = a->spatial % vn == 0 && P.xs % vn == 0 && P.rs % vn == 0 && P.ys % vn == 0 && aligned16(a->x) && aligned16(a->y) && (!a->residual || aligned16(a->residual));
    norm_plan(a->instances, a->spatial, vn, P.nsplit, P.slab);
    hipStream_t st = (hipStream_t)a->stream;
    if (a->dtype == SEGM_F32) return launch_norm_fwd<float>(P, a->instances, vec, st);
    if (a->dtype == SEGM_F16) return launch_norm_fwd<f16_t>(P, a->instances, vec, st);
    return launch_norm_fwd<bf16_t>(P, a->instances, vec, st);
}

extern "C" int segm_instnorm_bwd(const segm_instnorm_bwd_args* a) {
    if (!a) return SEGM_E_NULL;
    int rc = norm_common(a->instances, a->spatial, a->dtype, a->act, a->workspace, a->workspace_bytes);
    if (rc != SEGM_OK) return rc;
    if (!a->x || !a->dy || !a->dx || !a->mean || !a->rstd) return SEGM_E_NULL;
    NormDev P;
    memset(&P, 0, sizeof(P));
    P.x = a->x; P.dy = a->dy; P.ymask = a->act ? a->y : nullptr; P.dx = a->dx; P.dres = a->dresidual;
    P.mean = (float*)a->mean; P.rstd = (float*)a->rstd;
    P.part = (float2*)a->workspace;
    P.S = a->spatial; P.act = a->act; P.slope = a->slope; P.eps = 0.f;
    if (!norm_stride(a->x_instance_stride, a->spatial, P.xs) || !norm_stride(a->dy_instance_stride, a->spatial, P.dys) ||
        !norm_stride(a->y_instance_stride, a->spatial, P.ys) || !norm_stride(a->dx_instance_stride, a->spatial, P.dxs) ||
        !norm_stride(a->dresidual_instance_stride, a->spatial, P.drs))
        return SEGM_E_SHAPE;
    const int vn = vec_width(a->dtype);
    const bool vec = a->spatial % vn == 0 && P.xs % vn == 0 && P.dys % vn == 0 && P.ys % vn == 0 && P.dxs % vn == 0 && P.drs % vn == 0 &&
                     aligned16(a->x) && aligned16(a->dy) && aligned16(a->dx) &&
                     (!P.ymask || aligned16(P.ymask)) && (!a->dresidual || aligned16(a->dresidual));
    norm_plan(a->instances, a->spatial, vn, P.nsplit, P.slab);
    hipStream_t st = (hipStream_t)a->stream;
    if (a->dtype == SEGM_F32) return launch_norm_bwd<float>(P, a->instances, vec, st);
    if (a->dtype == SEGM_F16) return launch_norm_bwd<f16_t>(P, a->instances, vec, st);
    return launch_norm_bwd<bf16_t>(P, a->instances, vec, st);
}

// ---- the residual tail  y = act(IN(x) + IN(skip))  of a block with a projection skip ----------------------------------------------
//   forward   K1 over the skip (segm_instnorm_stats), K1 over x unless its producer summed the statistics, then ONE apply pass
//             (the skip's normalised value is rounded to the type in registers, never stored): 4 tensors of traffic, not 6
//   backward  ONE statistics pass (the four sums of both branches), ONE apply pass writing dx and dskip: 10 tensors, not 12
// Every sum is accumulated in the order of the two-call sequence and every element goes through the same helpers: the results are
// bit-equal to segm_instnorm_fwd(skip) -> segm_instnorm_fwd(x, residual) and their backwards with dresidual (tests/norm_tail_checks.py).
extern "C" size_t segm_instnorm_tail_workspace_bytes(int32_t instances, int64_t spatial) {
    return 2 * segm_instnorm_workspace_bytes(instances, spatial);
}

extern "C" int segm_instnorm_stats(const segm_instnorm_stats_args* a) {
    if (!a) return SEGM_E_NULL;
    int rc = norm_common(a->instances, a->spatial, a->dtype, 0, a->partials, a->partials_bytes);
    if (rc != SEGM_OK) return rc;
    if (!a->x) return SEGM_E_NULL;
    NormDev P;
    memset(&P, 0, sizeof(P));
    P.x = a->x; P.part = (float2*)a->partials; P.S = a->spatial;
    if (!norm_stride(a->x_instance_stride, a->spatial, P.xs)) return SEGM_E_SHAPE;
    const int vn = vec_width(a->dtype);
    const bool vec = a->spatial % vn == 0 && P.xs % vn == 0 && aligned16(a->x);
    norm_plan(a->instances, a->spatial, vn, P.nsplit, P.slab);
    hipStream_t st = (hipStream_t)a->stream;
    if (a->dtype == SEGM_F32) return launch_norm_stats<float>(P, a->instances, vec, st);
    if (a->dtype == SEGM_F16) return launch_norm_stats<f16_t>(P, a->instances, vec, st);
    return launch_norm_stats<bf16_t>(P, a->instances, vec, st);
}

extern "C" int segm_instnorm_tail_fwd(const segm_instnorm_tail_fwd_args* a) {
    if (!a) return SEGM_E_NULL;
    int rc = norm_common(a->instances, a->spatial, a->dtype, a->act, a->workspace, a->workspace_bytes);
    if (rc != SEGM_OK) return rc;
    if (!a->x || !a->skip || !a->y || !a->mean || !a->rstd || !a->skip_mean || !a->skip_rstd) return SEGM_E_NULL;
    if (!a->skip_partials || a->skip_partials_bytes < segm_instnorm_workspace_bytes(a->instances, a->spatial)) return SEGM_E_WORKSPACE;
    NormDev P;
    memset(&P, 0, sizeof(P));
    P.x = a->x; P.res = a->skip; P.y = a->y; P.mean = a->mean; P.rstd = a->rstd; P.mean3 = a->skip_mean; P.rstd3 = a->skip_rstd;
    P.part = (float2*)a->workspace; P.part3 = (float2*)a->skip_partials;
    P.S = a->spatial; P.act = a->act; P.slope = a->slope; P.eps = a->eps;
    if (a->stats_partials) {
        if (a->stats_nparts <= 0 || ((uintptr_t)a->stats_partials & 15)) return SEGM_E_SHAPE;
        P.ext = (const float4*)a->stats_partials; P.next = a->stats_nparts;
    }
    if (!norm_stride(a->x_instance_stride, a->spatial, P.xs) || !norm_stride(a->skip_instance_stride, a->spatial, P.rs) ||
        !norm_stride(a->y_instance_stride, a->spatial, P.ys))
        return SEGM_E_SHAPE;
    const int vn = vec_width(a->dtype);
    const bool vec = a->spatial % vn == 0 && P.xs % vn == 0 && P.rs % vn == 0 && P.ys % vn == 0 && aligned16(a->x) && aligned16(a->y) && aligned16(a->skip);
    norm_plan(a->instances, a->spatial, vn, P.nsplit, P.slab);
    hipStream_t st = (hipStream_t)a->stream;
    if (a->dtype == SEGM_F32) return launch_norm_tail_fwd<float>(P, a->instances, vec, st);
    if (a->dtype == SEGM_F16) return launch_norm_tail_fwd<f16_t>(P, a->instances, vec, st);
    return launch_norm_tail_fwd<bf16_t>(P, a->instances, vec, st);
}

extern "C" int segm_instnorm_tail_bwd(const segm_instnorm_tail_bwd_args* a) {
    if (!a) return SEGM_E_NULL;
    int rc = norm_common(a->instances, a->spatial, a->dtype, a->act, a->workspace, a->workspace_bytes);
    if (rc != SEGM_OK) return rc;
    if (a->workspace_bytes < segm_instnorm_tail_workspace_bytes(a->instances, a->spatial)) return SEGM_E_WORKSPACE;    // four sums per slab
    if (!a->x || !a->skip || !a->dy || !a->dx || !a->dskip || !a->mean || !a->rstd || !a->skip_mean || !a->skip_rstd) return SEGM_E_NULL;
    if (a->act && !a->y) return SEGM_E_NULL;             // a residual was added: the activation mask comes from y
    NormDev P;
    memset(&P, 0, sizeof(P));
    P.x = a->x; P.res = a->skip; P.dy = a->dy; P.ymask = a->act ? a->y : nullptr; P.dx = a->dx; P.ds = a->dskip;
    P.mean = (float*)a->mean; P.rstd = (float*)a->rstd; P.mean3 = (float*)a->skip_mean; P.rstd3 = (float*)a->skip_rstd;
    P.part = (float2*)a->workspace;
    P.part3 = P.part + (size_t)a->instances * kNormMaxSplit;
    P.S = a->spatial; P.act = a->act; P.slope = a->slope; P.eps = 0.f;
    if (!norm_stride(a->x_instance_stride, a->spatial, P.xs) || !norm_stride(a->skip_instance_stride, a->spatial, P.rs) ||
        !norm_stride(a->dy_instance_stride, a->spatial, P.dys) || !norm_stride(a->y_instance_stride, a->spatial, P.ys) ||
        !norm_stride(a->dx_instance_stride, a->spatial, P.dxs) || !norm_stride(a->dskip_instance_stride, a->spatial, P.dss))
        return SEGM_E_SHAPE;
    const int vn = vec_width(a->dtype);
    const bool vec = a->spatial % vn == 0 && P.xs % vn == 0 && P.rs % vn == 0 && P.dys % vn == 0 && P.ys % vn == 0 && P.dxs % vn == 0 &&
                     P.dss % vn == 0 && aligned16(a->x) && aligned16(a->skip) && aligned16(a->dy) && aligned16(a->dx) && aligned16(a->dskip) &&
                     (!P.ymask || aligned16(P.ymask));
    norm_plan(a->instances, a->spatial, vn, P.nsplit, P.slab);
    hipStream_t st = (hipStream_t)a->stream;
    if (a->dtype == SEGM_F32) return launch_norm_tail_bwd<float>(P, a->instances, vec, st);
    if (a->dtype == SEGM_F16) return launch_norm_tail_bwd<f16_t>(P, a->instances, vec, st);
    return launch_norm_tail_bwd<bf16_t>(P, a->instances, vec, st);
}
