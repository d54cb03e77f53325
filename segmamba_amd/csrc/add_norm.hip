// Residual add + LayerNorm / RMSNorm over the last dimension, forward and backward (C ABI: segm_add_norm_fwd, segm_add_norm_bwd,
// segm_add_norm_workspace_bytes).
//
// Replaces the Triton kernels of the reference's mamba_ssm/ops/triton/layernorm.py (_layer_norm_fwd, layernorm.py:123-177, and
// _layer_norm_bwd, layernorm.py:293-377): the add of the residual stream, the normalisation and the optional fp32 copy of the sum
// in one read and one write of the (M, N) token tensor.  The arithmetic is stated in include/segmamba_hip.h.
//
// A row is laid over a TEAM of lanes; a lane takes P packets of V consecutive elements (V = 16 bytes of x: 4 fp32, 8 fp16 / bf16),
// packet tl + k * team for k = 0 .. P - 1.  Team and P follow from ceil(N / V) alone (an_geometry): up to 64 packets take a power
// of two of lanes and P = 1 (N = 48 in bf16: 8 lanes, 32 rows per workgroup); up to 256 packets one wave and P = 2 or 4; wider
// rows the whole workgroup and P up to 8.  The row stays in registers between the statistics and the write: x, the residual and dy
// are read once.  Sums: the lane's elements in order, an xor-shuffle tree over the team, and for a team of four waves their four
// sums through LDS in wave order - so a row's bits do not depend on M or on the other rows.
//
// Two routes, as in stitch.hip: a packet moves with 16-byte accesses where N % V == 0, every row stride in use is a multiple of
// V and every pointer in use is 16-byte aligned, element by element otherwise.  Both keep the same elements in the same lanes and
// call the same per-element functions (an_xhat, an_y, an_wdy, an_dx), whose products are explicit fmaf or pinned (RL_ROUND): the
// library is built with -ffp-contract=fast, and two instantiations need not fuse alike.
//
// Backward: a workgroup walks a contiguous share of the row groups with dweight / dbias of its columns in registers, folds its
// teams through LDS in team order and leaves one fp32 partial row; launch_reduce_partials adds the rows in a fixed order.  No
// floating-point atomics.
#include <string.h>

#include "loss_common.h"

namespace segm {

void launch_reduce_partials(const float* part, int64_t nrows, int K, int dim, float* out0, int K0, float* out1,
                            float* out2, hipStream_t stream);                  // conv1d.hip

constexpr int kAnMaxCols = SEGM_ADD_NORM_MAX_COLS;

struct AnDev {
    const void *x, *res, *saved, *dy, *dres;
    void *y, *res_out, *dx, *dres_in;
    const float *w, *b;
    float *mean, *rstd, *part;
    int64_t sx, sres, sy, sres_out, ssaved, sdy, sdres, sdx, sdres_in;
    int64_t M, groups;                                // rows; groups of kBlock >> shift rows
    int32_t N, shift;                                 // the team is 1 << shift lanes: 0 .. 6, or 8 (the workgroup)
    int32_t rms, saved_is_res, groups_per_wg, K;      // K: 2 partial rows per workgroup with dbias, 1 without
    float eps;
};

// ---- the per-element functions ------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float an_xhat(float s, float mean, float rstd) { return (s - mean) * rstd; }

__device__ __forceinline__ float an_y(float xhat, float w, float b, bool has_b) { return has_b ? fmaf(xhat, w, b) : xhat * w; }

__device__ __forceinline__ float an_wdy(float w, float dy) {
    float t = w * dy;
    RL_ROUND(t);                                      // rounded on its own: it feeds sums and a difference
    return t;
}

__device__ __forceinline__ float an_dx(float xhat, float wdy, float c1, float c2, float rstd) {
    float d = (wdy - fmaf(xhat, c1, c2)) * rstd;
    RL_ROUND(d);                                      // never fused into the add of dresidual
    return d;
}

// ---- packets ------------------------------------------------------------------------------------------------------------------------------
// elements c0 .. c0 + V - 1 of a row of N as fp32; zeros past N and for a row that does not exist
template <typename S, int V, bool VEC>
__device__ __forceinline__ void an_load(const S* row, int c0, int N, bool live, float v[V]) {
    if (VEC) {
        if (live && c0 < N) {
            S raw[V];
            memcpy(raw, __builtin_assume_aligned(row + c0, 16), V * sizeof(S));
#pragma unroll
            for (int e = 0; e < V; ++e) v[e] = to_f32(raw[e]);
        } else {
#pragma unroll
            for (int e = 0; e < V; ++e) v[e] = 0.f;
        }
    } else {
#pragma unroll
        for (int e = 0; e < V; ++e) v[e] = (live && c0 + e < N) ? to_f32(row[c0 + e]) : 0.f;
    }
}

template <typename S, int V, bool VEC>
__device__ __forceinline__ void an_store(S* row, int c0, int N, bool live, const float v[V]) {
    if (VEC) {
        if (live && c0 < N) {
            S raw[V];
#pragma unroll
            for (int e = 0; e < V; ++e) raw[e] = from_f32<S>(v[e]);
            memcpy(__builtin_assume_aligned(row + c0, 16), raw, V * sizeof(S));
        }
    } else {
#pragma unroll
        for (int e = 0; e < V; ++e)
            if (live && c0 + e < N) row[c0 + e] = from_f32<S>(v[e]);
    }
}

// ---- sums over a team ---------------------------------------------------------------------------------------------------------------------
// every lane of the team gets the same bits; a team of four waves adds their sums in wave order (all threads of the workgroup call)
__device__ __forceinline__ void an_team_sum2(float& a, float& b, int shift, float (&s_red)[2][kWavesPerBlock]) {
    const int n = shift > 6 ? kWave : 1 << shift;
    for (int off = n >> 1; off >= 1; off >>= 1) {
        a += __shfl_xor(a, off);
        b += __shfl_xor(b, off);
    }
    if (shift > 6) {                                  // uniform over the grid
        __syncthreads();                              // the readers of the previous sums are done
        if ((threadIdx.x & (kWave - 1)) == 0) {
            s_red[0][threadIdx.x / kWave] = a;
            s_red[1][threadIdx.x / kWave] = b;
        }
        __syncthreads();
        a = ((s_red[0][0] + s_red[0][1]) + s_red[0][2]) + s_red[0][3];
        b = ((s_red[1][0] + s_red[1][1]) + s_red[1][2]) + s_red[1][3];
    }
}

__device__ __forceinline__ float an_team_sum(float a, int shift, float (&s_red)[2][kWavesPerBlock]) {
    const int n = shift > 6 ? kWave : 1 << shift;
    for (int off = n >> 1; off >= 1; off >>= 1) a += __shfl_xor(a, off);
    if (shift > 6) {
        __syncthreads();
        if ((threadIdx.x & (kWave - 1)) == 0) s_red[0][threadIdx.x / kWave] = a;
        __syncthreads();
        a = ((s_red[0][0] + s_red[0][1]) + s_red[0][2]) + s_red[0][3];
    }
    return a;
}

// ---- forward ------------------------------------------------------------------------------------------------------------------------------
template <typename T, typename RT, bool VEC, int P>
__global__ void __launch_bounds__(kBlock) an_fwd_kernel(AnDev D) {
    constexpr int V = Vec<T>::N;
    __shared__ float s_red[2][kWavesPerBlock];
    const int team_lanes = 1 << D.shift, N = D.N;
    const int team = threadIdx.x >> D.shift, tl = threadIdx.x & (team_lanes - 1);
    const int64_t row_raw = (int64_t)blockIdx.x * (kBlock >> D.shift) + team;
    const bool live = row_raw < D.M;
    const int64_t row = live ? row_raw : 0;           // the lanes of a missing row go along for the shuffles and the barriers
    const bool has_res = D.res != nullptr, has_out = D.res_out != nullptr, has_b = D.b != nullptr;
    const T* xr = reinterpret_cast<const T*>(D.x) + row * D.sx;
    const RT* rr = has_res ? reinterpret_cast<const RT*>(D.res) + row * D.sres : nullptr;
    RT* ro = has_out ? reinterpret_cast<RT*>(D.res_out) + row * D.sres_out : nullptr;
    T* yr = reinterpret_cast<T*>(D.y) + row * D.sy;

    float s[P][V];
#pragma unroll
    for (int k = 0; k < P; ++k) {
        const int c0 = (tl + k * team_lanes) * V;
        an_load<T, V, VEC>(xr, c0, N, live, s[k]);
        if (has_res) {
            float r[V];
            an_load<RT, V, VEC>(rr, c0, N, live, r);
#pragma unroll
            for (int e = 0; e < V; ++e) s[k][e] = s[k][e] + r[e];
        }
        if (has_out) an_store<RT, V, VEC>(ro, c0, N, live, s[k]);
    }
    const float fn = (float)N;
    float mean = 0.f;
    if (!D.rms) {
        float a = 0.f;
#pragma unroll
        for (int k = 0; k < P; ++k)
#pragma unroll
            for (int e = 0; e < V; ++e) a += s[k][e];              // zeros past N
        mean = an_team_sum(a, D.shift, s_red) / fn;
    }
    float q = 0.f;
#pragma unroll
    for (int k = 0; k < P; ++k) {
        const int c0 = (tl + k * team_lanes) * V;
#pragma unroll
        for (int e = 0; e < V; ++e) {
            const float d = c0 + e < N ? s[k][e] - mean : 0.f;
            q = fmaf(d, d, q);
        }
    }
    q = an_team_sum(q, D.shift, s_red);
    const float rstd = 1.0f / sqrtf(q / fn + D.eps);
    if (live && tl == 0) {
        if (!D.rms) D.mean[row] = mean;
        D.rstd[row] = rstd;
    }
#pragma unroll
    for (int k = 0; k < P; ++k) {
        const int c0 = (tl + k * team_lanes) * V;
        if (c0 >= N) continue;
        float w[V], b[V], o[V];
        an_load<float, V, VEC>(D.w, c0, N, true, w);
        if (has_b) an_load<float, V, VEC>(D.b, c0, N, true, b);
#pragma unroll
        for (int e = 0; e < V; ++e) o[e] = an_y(an_xhat(s[k][e], mean, rstd), w[e], has_b ? b[e] : 0.f, has_b);
        an_store<T, V, VEC>(yr, c0, N, live, o);
    }
}

// ---- backward -----------------------------------------------------------------------------------------------------------------------------
template <typename T, typename RT, bool VEC, int P>
__global__ void __launch_bounds__(kBlock) an_bwd_kernel(AnDev D) {
    constexpr int V = Vec<T>::N;
    constexpr int kFold = P <= 4 ? kBlock * P * V : 1;            // P = 8 belongs to the team of four waves, which folds nothing
    __shared__ float s_red[2][kWavesPerBlock];
    __shared__ float s_fold[kFold];
    const int team_lanes = 1 << D.shift, N = D.N;
    const int team = threadIdx.x >> D.shift, tl = threadIdx.x & (team_lanes - 1);
    const int teams = kBlock >> D.shift;
    const bool has_dres = D.dres != nullptr, has_in = D.dres_in != nullptr;
    const float fn = (float)N;

    float w[P][V], dw[P][V], db[P][V];
#pragma unroll
    for (int k = 0; k < P; ++k) {
        an_load<float, V, VEC>(D.w, (tl + k * team_lanes) * V, N, true, w[k]);
#pragma unroll
        for (int e = 0; e < V; ++e) { dw[k][e] = 0.f; db[k][e] = 0.f; }
    }
    const int64_t g0 = (int64_t)blockIdx.x * D.groups_per_wg;
    const int64_t g1 = g0 + D.groups_per_wg < D.groups ? g0 + D.groups_per_wg : D.groups;
    for (int64_t g = g0; g < g1; ++g) {
        const int64_t row_raw = g * teams + team;
        const bool live = row_raw < D.M;
        const int64_t row = live ? row_raw : 0;
        const float mean = (live && !D.rms) ? D.mean[row] : 0.f, rstd = live ? D.rstd[row] : 0.f;
        const T* dyr = reinterpret_cast<const T*>(D.dy) + row * D.sdy;
        float xh[P][V], wdy[P][V];
        float a = 0.f, b = 0.f;
#pragma unroll
        for (int k = 0; k < P; ++k) {
            const int c0 = (tl + k * team_lanes) * V;
            float xs[V], dyv[V];
            if (D.saved_is_res) an_load<RT, V, VEC>(reinterpret_cast<const RT*>(D.saved) + row * D.ssaved, c0, N, live, xs);
            else an_load<T, V, VEC>(reinterpret_cast<const T*>(D.saved) + row * D.ssaved, c0, N, live, xs);
            an_load<T, V, VEC>(dyr, c0, N, live, dyv);
#pragma unroll
            for (int e = 0; e < V; ++e) {                          // past N and in a missing row dy and w are zero
                xh[k][e] = an_xhat(xs[e], mean, rstd);
                wdy[k][e] = an_wdy(w[k][e], dyv[e]);
                a = fmaf(xh[k][e], wdy[k][e], a);
                b += wdy[k][e];
                dw[k][e] = fmaf(dyv[e], xh[k][e], dw[k][e]);
                db[k][e] += dyv[e];
            }
        }
        an_team_sum2(a, b, D.shift, s_red);
        const float c1 = a / fn, c2 = D.rms ? 0.f : b / fn;
#pragma unroll
        for (int k = 0; k < P; ++k) {
            const int c0 = (tl + k * team_lanes) * V;
            if (c0 >= N) continue;
            float dr[V], o[V];
            if (has_dres) an_load<RT, V, VEC>(reinterpret_cast<const RT*>(D.dres) + row * D.sdres, c0, N, live, dr);
#pragma unroll
            for (int e = 0; e < V; ++e) {
                const float d = an_dx(xh[k][e], wdy[k][e], c1, c2, rstd);
                o[e] = has_dres ? d + dr[e] : d;
            }
            if (has_in) an_store<RT, V, VEC>(reinterpret_cast<RT*>(D.dres_in) + row * D.sdres_in, c0, N, live, o);
            an_store<T, V, VEC>(reinterpret_cast<T*>(D.dx) + row * D.sdx, c0, N, live, o);
        }
    }
    // one partial row per workgroup: [dweight][dbias]
    float* prow = D.part + (int64_t)blockIdx.x * D.K * N;
    if (D.shift > 6) {
#pragma unroll
        for (int k = 0; k < P; ++k)
#pragma unroll
            for (int e = 0; e < V; ++e) {
                const int col = (tl + k * team_lanes) * V + e;
                if (col < N) {
                    prow[col] = dw[k][e];
                    if (D.K == 2) prow[N + col] = db[k][e];
                }
            }
    } else {
        const int team_cols = team_lanes * P * V;                 // N <= team_cols, teams * team_cols == kBlock * P * V
        for (int pass = 0; pass < D.K; ++pass) {
            __syncthreads();
#pragma unroll
            for (int k = 0; k < P; ++k)
#pragma unroll
                for (int e = 0; e < V; ++e) s_fold[team * team_cols + (tl + k * team_lanes) * V + e] = pass ? db[k][e] : dw[k][e];
            __syncthreads();
            for (int col = threadIdx.x; col < N; col += kBlock) {
                float t = 0.f;
                for (int r = 0; r < teams; ++r) t += s_fold[r * team_cols + col];
                prow[pass * N + col] = t;
            }
        }
    }
}

// ---- host ---------------------------------------------------------------------------------------------------------------------------------
struct AnGeom {
    int shift, P;
};

// how a row of N elements in packets of V lies over lanes: from N and the dtype alone
static AnGeom an_geometry(int N, int V) {
    const int items = (N + V - 1) / V;
    AnGeom G;
    if (items <= kWave) {
        G.shift = 0;
        while ((1 << G.shift) < items) ++G.shift;
        G.P = 1;
    } else if (items <= 4 * kWave) {
        G.shift = 6;
        G.P = items <= 2 * kWave ? 2 : 4;
    } else {
        G.shift = 8;
        const int per = (items + kBlock - 1) / kBlock;            // 2 .. 8 (fp32), 2 .. 4 (16 bits)
        G.P = per <= 2 ? 2 : per <= 4 ? 4 : 8;
    }
    return G;
}

static int64_t an_max_workgroups(int N) { return N <= 1024 ? 2048 : 512; }   // of the backward: its partial rows

static bool an_dtype_ok(int d) { return d == SEGM_F32 || d == SEGM_F16 || d == SEGM_BF16; }

// one tensor of the call: NULL or a stride below N or a misaligned pointer -> status; collects what the packet route needs
struct AnCheck {
    int N, V;
    bool vec;
    int use(const void* p, int64_t stride, int dtype, bool required) {
        if (!p) return required ? SEGM_E_NULL : SEGM_OK;
        if (stride < N) return SEGM_E_SHAPE;
        if ((uintptr_t)p % (dtype == SEGM_F32 ? 4 : 2)) return SEGM_E_SHAPE;
        if ((uintptr_t)p % 16 || stride % V) vec = false;
        return SEGM_OK;
    }
    int use_f32(const float* p, bool required) {
        if (!p) return required ? SEGM_E_NULL : SEGM_OK;
        if ((uintptr_t)p % 4) return SEGM_E_SHAPE;
        if ((uintptr_t)p % 16) vec = false;
        return SEGM_OK;
    }
};

static int an_common(const segm_add_norm_args* a, AnCheck& C) {
    if (a->cols < 1 || a->cols > kAnMaxCols || a->rows < 1 || a->rows >= ((int64_t)1 << 31)) return SEGM_E_SHAPE;
    if (!an_dtype_ok(a->dtype) || (a->res_dtype != a->dtype && a->res_dtype != SEGM_F32)) return SEGM_E_DTYPE;
    C.N = a->cols;
    C.V = a->dtype == SEGM_F32 ? 4 : 8;
    C.vec = a->cols % C.V == 0;
    return SEGM_OK;
}

template <typename T, typename RT, bool VEC>
static void an_launch_p(const AnDev& D, int P, bool bwd, unsigned grid, hipStream_t st) {
#define SEGM_AN_CASE(NP) \
    case NP: \
        if (bwd) hipLaunchKernelGGL((an_bwd_kernel<T, RT, VEC, NP>), dim3(grid), dim3(kBlock), 0, st, D); \
        else hipLaunchKernelGGL((an_fwd_kernel<T, RT, VEC, NP>), dim3(grid), dim3(kBlock), 0, st, D); \
        break
    switch (P) {
        SEGM_AN_CASE(1);
        SEGM_AN_CASE(2);
        SEGM_AN_CASE(4);
    default:
        if constexpr (sizeof(T) == 4) {                           // eight packets per lane: fp32 rows beyond 4096 only
            if (bwd) hipLaunchKernelGGL((an_bwd_kernel<T, RT, VEC, 8>), dim3(grid), dim3(kBlock), 0, st, D);
            else hipLaunchKernelGGL((an_fwd_kernel<T, RT, VEC, 8>), dim3(grid), dim3(kBlock), 0, st, D);
        }
        break;
    }
#undef SEGM_AN_CASE
}

template <typename T, typename RT>
static void an_launch_v(const AnDev& D, int P, bool vec, bool bwd, unsigned grid, hipStream_t st) {
    if (vec) an_launch_p<T, RT, true>(D, P, bwd, grid, st);
    else an_launch_p<T, RT, false>(D, P, bwd, grid, st);
}

static void an_launch(const AnDev& D, int dtype, int res_dtype, int P, bool vec, bool bwd, unsigned grid, hipStream_t st) {
    const bool wide = res_dtype != dtype;                         // an fp32 residual stream beside 16-bit tokens
    if (dtype == SEGM_F32) an_launch_v<float, float>(D, P, vec, bwd, grid, st);
    else if (dtype == SEGM_F16) { if (wide) an_launch_v<f16_t, float>(D, P, vec, bwd, grid, st); else an_launch_v<f16_t, f16_t>(D, P, vec, bwd, grid, st); }
    else { if (wide) an_launch_v<bf16_t, float>(D, P, vec, bwd, grid, st); else an_launch_v<bf16_t, bf16_t>(D, P, vec, bwd, grid, st); }
}

}  // namespace segm

using namespace segm;

extern "C" size_t segm_add_norm_workspace_bytes(int64_t rows, int32_t cols) {
    if (cols < 1 || cols > kAnMaxCols || rows < 1 || rows >= ((int64_t)1 << 31)) return 0;
    const int64_t wgs = rows < an_max_workgroups(cols) ? rows : an_max_workgroups(cols);
    return (size_t)wgs * 2 * (size_t)cols * sizeof(float);
}

extern "C" int segm_add_norm_fwd(const segm_add_norm_args* a) {
    if (!a) return SEGM_E_NULL;
    AnCheck C;
    int rc = an_common(a, C);
    if (rc != SEGM_OK) return rc;
    if (!a->x || !a->y || !a->weight || !a->rstd || (!a->rms && !a->mean)) return SEGM_E_NULL;
    if ((rc = C.use(a->x, a->x_stride, a->dtype, true)) != SEGM_OK) return rc;
    if ((rc = C.use(a->y, a->y_stride, a->dtype, true)) != SEGM_OK) return rc;
    if ((rc = C.use(a->residual, a->residual_stride, a->res_dtype, false)) != SEGM_OK) return rc;
    if ((rc = C.use(a->residual_out, a->residual_out_stride, a->res_dtype, false)) != SEGM_OK) return rc;
    if ((rc = C.use_f32(a->weight, true)) != SEGM_OK) return rc;
    if ((rc = C.use_f32(a->bias, false)) != SEGM_OK) return rc;
    if ((uintptr_t)a->rstd % 4 || (uintptr_t)a->mean % 4) return SEGM_E_SHAPE;
    const AnGeom G = an_geometry(a->cols, C.V);
    AnDev D;
    memset(&D, 0, sizeof(D));
    D.x = a->x; D.res = a->residual; D.y = a->y; D.res_out = a->residual_out;
    D.w = a->weight; D.b = a->bias; D.mean = a->mean; D.rstd = a->rstd;
    D.sx = a->x_stride; D.sres = a->residual_stride; D.sy = a->y_stride; D.sres_out = a->residual_out_stride;
    D.M = a->rows; D.N = a->cols; D.shift = G.shift; D.rms = a->rms != 0; D.eps = a->eps;
    const int64_t teams = kBlock >> G.shift;
    D.groups = (a->rows + teams - 1) / teams;
    an_launch(D, a->dtype, a->res_dtype, G.P, C.vec, false, (unsigned)D.groups, (hipStream_t)a->stream);
    return (int)hipGetLastError();
}

extern "C" int segm_add_norm_bwd(const segm_add_norm_args* a) {
    if (!a) return SEGM_E_NULL;
    AnCheck C;
    int rc = an_common(a, C);
    if (rc != SEGM_OK) return rc;
    const bool saved_is_res = a->residual_out != nullptr;
    if (!a->dy || !a->dx || !a->weight || !a->rstd || !a->dweight || (!a->rms && !a->mean)) return SEGM_E_NULL;
    if (!saved_is_res && !a->x) return SEGM_E_NULL;
    if (saved_is_res) rc = C.use(a->residual_out, a->residual_out_stride, a->res_dtype, true);
    else rc = C.use(a->x, a->x_stride, a->dtype, true);
    if (rc != SEGM_OK) return rc;
    if ((rc = C.use(a->dy, a->dy_stride, a->dtype, true)) != SEGM_OK) return rc;
    if ((rc = C.use(a->dx, a->dx_stride, a->dtype, true)) != SEGM_OK) return rc;
    if ((rc = C.use(a->dresidual, a->dresidual_stride, a->res_dtype, false)) != SEGM_OK) return rc;
    if ((rc = C.use(a->dresidual_in, a->dresidual_in_stride, a->res_dtype, false)) != SEGM_OK) return rc;
    if ((rc = C.use_f32(a->weight, true)) != SEGM_OK) return rc;
    if ((uintptr_t)a->rstd % 4 || (uintptr_t)a->mean % 4 || (uintptr_t)a->dweight % 4 || (uintptr_t)a->dbias % 4) return SEGM_E_SHAPE;
    if (!a->workspace || (uintptr_t)a->workspace % 4 || a->workspace_bytes < segm_add_norm_workspace_bytes(a->rows, a->cols))
        return SEGM_E_WORKSPACE;
    const AnGeom G = an_geometry(a->cols, C.V);
    AnDev D;
    memset(&D, 0, sizeof(D));
    D.saved = saved_is_res ? a->residual_out : a->x;
    D.ssaved = saved_is_res ? a->residual_out_stride : a->x_stride;
    D.saved_is_res = saved_is_res;
    D.dy = a->dy; D.dres = a->dresidual; D.dx = a->dx; D.dres_in = a->dresidual_in;
    D.sdy = a->dy_stride; D.sdres = a->dresidual_stride; D.sdx = a->dx_stride; D.sdres_in = a->dresidual_in_stride;
    D.w = a->weight; D.mean = a->mean; D.rstd = a->rstd; D.part = (float*)a->workspace;
    D.M = a->rows; D.N = a->cols; D.shift = G.shift; D.rms = a->rms != 0;
    D.K = a->dbias ? 2 : 1;
    const int64_t teams = kBlock >> G.shift;
    D.groups = (a->rows + teams - 1) / teams;
    const int64_t cap = an_max_workgroups(a->cols);
    D.groups_per_wg = (int32_t)((D.groups + cap - 1) / cap);
    const int64_t wgs = (D.groups + D.groups_per_wg - 1) / D.groups_per_wg;      // <= min(cap, rows): the workspace holds them
    hipStream_t st = (hipStream_t)a->stream;
    an_launch(D, a->dtype, a->res_dtype, G.P, C.vec, true, (unsigned)wgs, st);
    launch_reduce_partials(D.part, wgs, D.K, a->cols, nullptr, 0, a->dweight, a->dbias, st);
    return (int)hipGetLastError();
}
