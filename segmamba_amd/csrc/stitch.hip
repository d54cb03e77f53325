// Stitching a sliding-window prediction (C ABI: segm_window_gather, segm_window_count, segm_window_blend, segm_window_finish).
//
// Replaces the ATen chain of segmamba_amd/predictor.py around the network - torch.flip of the volume, F.pad, the torch.cat of window
// slices, the cast / multiply / slice-add per window, the full-volume divide and the flip back - i.e. monai/inferers/utils.py
// sliding_window_inference and the mirror loop of light_training/prediction.py:110-159.  The geometry is the reference's: per axis
// image = max(size, roi), pad0 = (image - size) / 2, window starts in the padded frame; a mirror mask flips z (bit 0), y (bit 1),
// x (bit 2) and is folded into the index, so no mirrored copy of the volume or of the result exists.
//
// Every kernel gives a thread a quad: four consecutive voxels along x of what it writes (the last quad of a row may be shorter).  A
// quad that is whole and whose addresses are multiples of 16 bytes (8 for a 16-bit prediction) moves as one packet, any other voxel
// by voxel; an x-flip reverses the packet.  Both routes call the same per-voxel function (st_src, st_blend, st_mean), so a voxel has
// the same bits whichever route it takes.
//
//   * st_gather_kernel   window voxel i has the padded-frame coordinate q = start + i and u = q - pad0: cval outside [0, size),
//                        otherwise the volume at size - 1 - u (flipped axis) or u.
//   * st_count_kernel    one thread per quad of the count map: the weights of the covering windows added in the order of
//                        dense_patch_starts (z outermost, x fastest) from 0 - the bits of the loop count[slice] += weight.
//   * st_blend_kernel    acc[b, :, start + i] += fl32(float(pred[n, :, i]) * w[i]).  Windows of one launch overlap, so the threads are
//                        laid over the accumulator, not over the windows: a thread takes one quad of the box around the launch's
//                        windows, finds the windows of its sample that cover it and adds their terms in window order - the order
//                        of the sequential loop.  Every voxel has ONE writer and there are no atomics: two calls are bit-equal.
//   * st_finish_kernel   total (+)= acc / count at the mirrored, padded position; the last pass divides by the number of passes.  A
//                        thread stores zeros where it has read the accumulator: measured against a memset after the kernel on
//                        4 x 138 x 176 x 144 it takes 0.032 ms where kernel + memset take 0.042 ms.  The border of a padded image is
//                        read by no thread; there (and only there) a memset of the accumulator follows.
#include <string.h>

#include "loss_common.h"

namespace segm {

constexpr int kStMaxW = SEGM_STITCH_MAX_WINDOWS;
constexpr int kStMaxS = SEGM_STITCH_MAX_STARTS;

// ---- the per-voxel functions ----------------------------------------------------------------------------------------------------------------
// the source index along one axis of the unpadded coordinate u (inside [0, size))
__device__ __forceinline__ int st_src(int u, int size, bool flip) { return flip ? size - 1 - u : u; }

__device__ __forceinline__ float st_blend(float a, float p, float w) {
    float m = p * w;
    RL_ROUND(m);                                      // rounded on its own: never fused into the sum
    return a + m;
}

__device__ __forceinline__ float st_mean(float a, float c, float t, bool first, int divisor) {
    float q = a / c;
    RL_ROUND(q);
    float s = first ? q : t + q;
    if (divisor > 1) {
        RL_ROUND(s);
        s = s / (float)divisor;
    }
    return s;
}

// ---- quads ----------------------------------------------------------------------------------------------------------------------------------
template <typename T> __device__ __forceinline__ bool st_aligned(const T* p) { return ((uintptr_t)p % (4 * sizeof(T))) == 0; }

template <typename T> __device__ __forceinline__ void st_ld4(const T* p, float v[4]) {
    T raw[4];
    memcpy(raw, __builtin_assume_aligned(p, 4 * sizeof(T)), 4 * sizeof(T));
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = to_f32(raw[e]);
}

__device__ __forceinline__ void st_st4(float* p, const float v[4]) {
    memcpy(__builtin_assume_aligned(p, 16), v, 16);
}

__device__ __forceinline__ void st_reverse(float v[4]) {
    const float t0 = v[0], t1 = v[1];
    v[0] = v[3]; v[3] = t0;
    v[1] = v[2]; v[2] = t1;
}

// row[o0 + e] for e = 0 .. 3 where 0 <= o0 + e < len; in[e] tells which
template <typename T> __device__ __forceinline__ void st_load_quad(const T* row, int o0, int len, float v[4], bool in[4]) {
    if (o0 >= 0 && o0 + 3 < len && st_aligned(row + o0)) {
        st_ld4(row + o0, v);
#pragma unroll
        for (int e = 0; e < 4; ++e) in[e] = true;
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int o = o0 + e;
            in[e] = o >= 0 && o < len;
            v[e] = in[e] ? to_f32(row[o]) : 0.f;
        }
    }
}

// the first `cnt` of four values to p
__device__ __forceinline__ void st_store_quad(float* p, const float v[4], int cnt) {
    if (cnt == 4 && st_aligned(p)) {
        st_st4(p, v);
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (e < cnt) p[e] = v[e];
    }
}

// quad t of a (rows of `height`, `nq` quads per row) plane -> z, y and the first x
__device__ __forceinline__ void st_quad(uint32_t t, int nq, int height, int& z, int& y, int& x) {
    const uint32_t row = t / (uint32_t)nq;
    x = (int)(t - row * (uint32_t)nq) * 4;
    z = (int)(row / (uint32_t)height);
    y = (int)(row - (uint32_t)z * (uint32_t)height);
}

struct StWindows {
    int32_t at[kStMaxW][4];                          // b, start z, y, x (padded frame)
};

// ---- gather ---------------------------------------------------------------------------------------------------------------------------------
struct StGather {
    const float* vol;
    float* out;
    int64_t sb, sc, sz, sy;
    int32_t C, size[3], roi[3], pad0[3];
    int32_t nq, nquads, mirror;
    float cval;
    StWindows win;
};

__global__ void __launch_bounds__(kBlock) st_gather_kernel(StGather P) {
    const uint32_t t = blockIdx.x * (uint32_t)kBlock + threadIdx.x;
    if (t >= (uint32_t)P.nquads) return;
    const int j = blockIdx.y / P.C, c = blockIdx.y - j * P.C;
    int iz, iy, ix;
    st_quad(t, P.nq, P.roi[1], iz, iy, ix);
    const int cnt = P.roi[2] - ix < 4 ? P.roi[2] - ix : 4;
    const int b = P.win.at[j][0];
    const int uz = P.win.at[j][1] + iz - P.pad0[0], uy = P.win.at[j][2] + iy - P.pad0[1], ux0 = P.win.at[j][3] + ix - P.pad0[2];
    const int X = P.size[2];
    const bool fx = (P.mirror & 4) != 0;
    float v[4] = {P.cval, P.cval, P.cval, P.cval};
    if (uz >= 0 && uz < P.size[0] && uy >= 0 && uy < P.size[1]) {
        const float* row = P.vol + (int64_t)b * P.sb + (int64_t)c * P.sc + (int64_t)st_src(uz, P.size[0], (P.mirror & 1) != 0) * P.sz +
                           (int64_t)st_src(uy, P.size[1], (P.mirror & 2) != 0) * P.sy;
        const int lo = fx ? st_src(ux0 + 3, X, true) : ux0;               // the lowest address of a whole quad
        if (cnt == 4 && ux0 >= 0 && ux0 + 3 < X && st_aligned(row + lo)) {
            st_ld4(row + lo, v);
            if (fx) st_reverse(v);
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int u = ux0 + e;
                if (e < cnt && u >= 0 && u < X) v[e] = row[st_src(u, X, fx)];
            }
        }
    }
    float* o = P.out + ((((int64_t)j * P.C + c) * P.roi[0] + iz) * P.roi[1] + iy) * (int64_t)P.roi[2] + ix;
    st_store_quad(o, v, cnt);
}

// ---- count ----------------------------------------------------------------------------------------------------------------------------------
struct StCount {
    const float* w;
    float* count;
    int32_t img[3], roi[3], ns[3];
    int32_t nq, nquads;
    int32_t starts[3][kStMaxS];
};

__global__ void __launch_bounds__(kBlock) st_count_kernel(StCount P) {
    const uint32_t t = blockIdx.x * (uint32_t)kBlock + threadIdx.x;
    if (t >= (uint32_t)P.nquads) return;
    int z, y, x0;
    st_quad(t, P.nq, P.img[1], z, y, x0);
    const int cnt = P.img[2] - x0 < 4 ? P.img[2] - x0 : 4;
    float s[4] = {0.f, 0.f, 0.f, 0.f};
    for (int a = 0; a < P.ns[0]; ++a) {
        const int oz = z - P.starts[0][a];
        if (oz < 0 || oz >= P.roi[0]) continue;
        for (int b = 0; b < P.ns[1]; ++b) {
            const int oy = y - P.starts[1][b];
            if (oy < 0 || oy >= P.roi[1]) continue;
            const float* row = P.w + ((int64_t)oz * P.roi[1] + oy) * P.roi[2];
            for (int c = 0; c < P.ns[2]; ++c) {
                const int o0 = x0 - P.starts[2][c];
                if (o0 + 3 < 0 || o0 >= P.roi[2]) continue;
                float wv[4];
                bool in[4];
                st_load_quad(row, o0, P.roi[2], wv, in);
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (in[e]) s[e] = s[e] + wv[e];
            }
        }
    }
    st_store_quad(P.count + ((int64_t)z * P.img[1] + y) * P.img[2] + x0, s, cnt);
}

// ---- blend ----------------------------------------------------------------------------------------------------------------------------------
struct StBlend {
    const void* pred;
    const float* w;
    float* acc;
    int32_t C, img[3], roi[3];
    int32_t lo[3], ext[3];                            // the box around the launch's windows; lo[2] is a multiple of 4
    int32_t nq, nquads, n;
    StWindows win;
};

template <typename T>
__global__ void __launch_bounds__(kBlock) st_blend_kernel(StBlend P) {
    const uint32_t t = blockIdx.x * (uint32_t)kBlock + threadIdx.x;
    if (t >= (uint32_t)P.nquads) return;
    const int b = blockIdx.y / P.C, c = blockIdx.y - b * P.C;
    int pz, py, px0;
    st_quad(t, P.nq, P.ext[1], pz, py, px0);
    pz += P.lo[0]; py += P.lo[1]; px0 += P.lo[2];
    const int rz = P.roi[0], ry = P.roi[1], rx = P.roi[2];
    // the windows of this sample that cover a voxel of the quad
    uint64_t covering = 0;
    for (int k = 0; k < P.n; ++k) {
        if (P.win.at[k][0] != b) continue;            // uniform over the workgroup
        const int oz = pz - P.win.at[k][1], oy = py - P.win.at[k][2], o0 = px0 - P.win.at[k][3];
        if (oz >= 0 && oz < rz && oy >= 0 && oy < ry && o0 + 3 >= 0 && o0 < rx) covering |= (uint64_t)1 << k;
    }
    if (!covering) return;
    float* ap = P.acc + ((((int64_t)b * P.C + c) * P.img[0] + pz) * P.img[1] + py) * (int64_t)P.img[2] + px0;
    const bool packet = px0 + 3 < P.img[2] && st_aligned(ap);
    float a[4] = {0.f, 0.f, 0.f, 0.f};
    bool hit[4] = {false, false, false, false};
    if (packet) st_ld4(ap, a);
    // in window order: the additions to a voxel happen as in the sequential loop
    for (uint64_t m = covering; m; m &= m - 1) {
        const int k = __builtin_ctzll(m);
        const int oz = pz - P.win.at[k][1], oy = py - P.win.at[k][2], o0 = px0 - P.win.at[k][3];
        const int64_t plane = ((int64_t)oz * ry + oy) * rx;
        const T* prow = reinterpret_cast<const T*>(P.pred) + ((int64_t)k * P.C + c) * rz * ry * (int64_t)rx + plane;
        float pv[4], wv[4];
        bool in[4], in_w[4];
        st_load_quad(prow, o0, rx, pv, in);
        st_load_quad(P.w + plane, o0, rx, wv, in_w);
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (in[e]) {
                if (!packet && !hit[e]) a[e] = ap[e];
                hit[e] = true;
                a[e] = st_blend(a[e], pv[e], wv[e]);
            }
    }
    if (packet) {                                     // voxels no window covers get back what they held: this thread is their only writer
        st_st4(ap, a);
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (hit[e]) ap[e] = a[e];
    }
}

// ---- finish ---------------------------------------------------------------------------------------------------------------------------------
struct StFinish {
    float* acc;
    const float* count;
    float* total;
    int32_t size[3], img[3], pad0[3];
    int32_t nq, nquads, mirror, first, divisor;
};

__global__ void __launch_bounds__(kBlock) st_finish_kernel(StFinish P) {
    const uint32_t t = blockIdx.x * (uint32_t)kBlock + threadIdx.x;
    if (t >= (uint32_t)P.nquads) return;
    const int bc = blockIdx.y;
    int z, y, x0;
    st_quad(t, P.nq, P.size[1], z, y, x0);
    const int X = P.size[2];
    const int cnt = X - x0 < 4 ? X - x0 : 4;
    const bool fx = (P.mirror & 4) != 0, first = P.first != 0;
    const int pz = P.pad0[0] + st_src(z, P.size[0], (P.mirror & 1) != 0), py = P.pad0[1] + st_src(y, P.size[1], (P.mirror & 2) != 0);
    const int64_t prow = ((int64_t)pz * P.img[1] + py) * P.img[2];
    float* arow = P.acc + (int64_t)bc * P.img[0] * P.img[1] * (int64_t)P.img[2] + prow;
    const float* crow = P.count + prow;
    const int lo = P.pad0[2] + (fx ? st_src(x0 + 3, X, true) : x0);       // the lowest address of a whole quad
    float a[4] = {0.f, 0.f, 0.f, 0.f}, cn[4] = {1.f, 1.f, 1.f, 1.f}, tv[4] = {0.f, 0.f, 0.f, 0.f};
    if (cnt == 4 && st_aligned(arow + lo) && st_aligned(crow + lo)) {
        st_ld4(arow + lo, a);
        st_ld4(crow + lo, cn);
        if (fx) { st_reverse(a); st_reverse(cn); }
        const float zero[4] = {0.f, 0.f, 0.f, 0.f};
        st_st4(arow + lo, zero);
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (e < cnt) {
                const int p = P.pad0[2] + st_src(x0 + e, X, fx);
                a[e] = arow[p];
                cn[e] = crow[p];
                arow[p] = 0.f;
            }
    }
    float* tp = P.total + (((int64_t)bc * P.size[0] + z) * P.size[1] + y) * (int64_t)X + x0;
    if (!first) {
        if (cnt == 4 && st_aligned(tp)) {
            st_ld4(tp, tv);
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (e < cnt) tv[e] = tp[e];
        }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) tv[e] = st_mean(a[e], cn[e], tv[e], first, P.divisor);
    st_store_quad(tp, tv, cnt);
}

// ---- host -----------------------------------------------------------------------------------------------------------------------------------
struct StGeom {
    int32_t img[3], pad0[3];
    int64_t roi_voxels, img_voxels, size_voxels;
};

// sides, planes below 2^31 voxels, the padded frame; 0 or a SEGM_E_* status
static int st_geometry(const segm_stitch_args* a, StGeom& G) {
    if (a->batch < 1 || a->channels < 1) return SEGM_E_SHAPE;
    G.roi_voxels = G.img_voxels = G.size_voxels = 1;
    for (int d = 0; d < 3; ++d) {
        if (a->size[d] < 1 || a->roi[d] < 1) return SEGM_E_SHAPE;
        G.img[d] = a->size[d] > a->roi[d] ? a->size[d] : a->roi[d];
        G.pad0[d] = (G.img[d] - a->size[d]) / 2;
        G.roi_voxels *= a->roi[d];
        G.img_voxels *= G.img[d];
        G.size_voxels *= a->size[d];
        if (G.img_voxels >= ((int64_t)1 << 31)) return SEGM_E_SHAPE;    // img >= size, roi: bounds all three
    }
    return SEGM_OK;
}

// 1 .. 64 windows of samples in [0, batch) that stay inside the image; n * channels within the grid's y
static int st_windows(const segm_stitch_args* a, const StGeom& G, StWindows& W) {
    if (a->n_windows < 1 || a->n_windows > kStMaxW) return SEGM_E_SHAPE;
    if ((int64_t)a->n_windows * a->channels > 65535) return SEGM_E_SHAPE;
    for (int j = 0; j < a->n_windows; ++j) {
        if (a->window[j][0] < 0 || a->window[j][0] >= a->batch) return SEGM_E_SHAPE;
        for (int d = 0; d < 3; ++d)
            if (a->window[j][1 + d] < 0 || a->window[j][1 + d] > G.img[d] - a->roi[d]) return SEGM_E_SHAPE;
    }
    memset(&W, 0, sizeof(W));
    memcpy(W.at, a->window, sizeof(int32_t) * 4 * (size_t)a->n_windows);
    return SEGM_OK;
}

static inline int32_t st_nq(int32_t width) { return (width + 3) / 4; }
static inline unsigned st_blocks(int64_t quads) { return (unsigned)((quads + kBlock - 1) / kBlock); }

}  // namespace segm

using namespace segm;

extern "C" int segm_window_gather(const segm_stitch_args* a) {
    if (!a) return SEGM_E_NULL;
    StGeom G;
    int rc = st_geometry(a, G);
    if (rc != SEGM_OK) return rc;
    StGather P;
    memset(&P, 0, sizeof(P));
    rc = st_windows(a, G, P.win);
    if (rc != SEGM_OK) return rc;
    if (a->mirror < 0 || a->mirror > 7) return SEGM_E_SHAPE;
    if (a->stride_x != 1 || a->stride_b < 0 || a->stride_c < 0 || a->stride_z < 0 || a->stride_y < 0) return SEGM_E_SHAPE;
    if (!a->volume || !a->windows_out) return SEGM_E_NULL;
    if ((uintptr_t)a->volume % sizeof(float) || (uintptr_t)a->windows_out % sizeof(float)) return SEGM_E_SHAPE;
    P.vol = a->volume; P.out = a->windows_out;
    P.sb = a->stride_b; P.sc = a->stride_c; P.sz = a->stride_z; P.sy = a->stride_y;
    P.C = a->channels;
    for (int d = 0; d < 3; ++d) { P.size[d] = a->size[d]; P.roi[d] = a->roi[d]; P.pad0[d] = G.pad0[d]; }
    P.nq = st_nq(a->roi[2]);
    P.nquads = (int32_t)((int64_t)a->roi[0] * a->roi[1] * P.nq);
    P.mirror = a->mirror;
    P.cval = a->cval;
    const dim3 grid(st_blocks(P.nquads), (unsigned)(a->n_windows * a->channels));
    hipLaunchKernelGGL(st_gather_kernel, grid, dim3(kBlock), 0, (hipStream_t)a->stream, P);
    return (int)hipGetLastError();
}

extern "C" int segm_window_count(const segm_stitch_args* a) {
    if (!a) return SEGM_E_NULL;
    StGeom G;
    const int rc = st_geometry(a, G);
    if (rc != SEGM_OK) return rc;
    StCount P;
    memset(&P, 0, sizeof(P));
    for (int d = 0; d < 3; ++d) {
        if (a->n_starts[d] < 1 || a->n_starts[d] > kStMaxS) return SEGM_E_SHAPE;
        for (int i = 0; i < a->n_starts[d]; ++i) {
            if (a->starts[d][i] < 0 || a->starts[d][i] > G.img[d] - a->roi[d]) return SEGM_E_SHAPE;
            P.starts[d][i] = a->starts[d][i];
        }
        P.ns[d] = a->n_starts[d]; P.img[d] = G.img[d]; P.roi[d] = a->roi[d];
    }
    if (!a->weight || !a->count) return SEGM_E_NULL;
    if ((uintptr_t)a->weight % sizeof(float) || (uintptr_t)a->count % sizeof(float)) return SEGM_E_SHAPE;
    P.w = a->weight; P.count = a->count;
    P.nq = st_nq(G.img[2]);
    P.nquads = (int32_t)((int64_t)G.img[0] * G.img[1] * P.nq);
    hipLaunchKernelGGL(st_count_kernel, dim3(st_blocks(P.nquads)), dim3(kBlock), 0, (hipStream_t)a->stream, P);
    return (int)hipGetLastError();
}

extern "C" int segm_window_blend(const segm_stitch_args* a) {
    if (!a) return SEGM_E_NULL;
    StGeom G;
    int rc = st_geometry(a, G);
    if (rc != SEGM_OK) return rc;
    StBlend P;
    memset(&P, 0, sizeof(P));
    rc = st_windows(a, G, P.win);
    if (rc != SEGM_OK) return rc;
    if ((int64_t)a->batch * a->channels > 65535) return SEGM_E_SHAPE;
    if (a->dtype != SEGM_F32 && a->dtype != SEGM_F16 && a->dtype != SEGM_BF16) return SEGM_E_DTYPE;
    if (!a->pred || !a->weight || !a->acc) return SEGM_E_NULL;
    if ((uintptr_t)a->pred % (a->dtype == SEGM_F32 ? 4 : 2) || (uintptr_t)a->weight % sizeof(float) || (uintptr_t)a->acc % sizeof(float))
        return SEGM_E_SHAPE;
    P.pred = a->pred; P.w = a->weight; P.acc = a->acc;
    P.C = a->channels; P.n = a->n_windows;
    for (int d = 0; d < 3; ++d) { P.img[d] = G.img[d]; P.roi[d] = a->roi[d]; }
    for (int d = 0; d < 3; ++d) {
        int32_t lo = P.win.at[0][1 + d], hi = lo;
        for (int j = 1; j < P.n; ++j) {
            lo = P.win.at[j][1 + d] < lo ? P.win.at[j][1 + d] : lo;
            hi = P.win.at[j][1 + d] > hi ? P.win.at[j][1 + d] : hi;
        }
        if (d == 2) lo &= ~3;                         // quads start where the accumulator's packets do
        P.lo[d] = lo;
        P.ext[d] = hi + a->roi[d] - lo;
    }
    P.nq = st_nq(P.ext[2]);
    P.nquads = (int32_t)((int64_t)P.ext[0] * P.ext[1] * P.nq);
    const dim3 grid(st_blocks(P.nquads), (unsigned)(a->batch * a->channels));
    hipStream_t st = (hipStream_t)a->stream;
    if (a->dtype == SEGM_F32) hipLaunchKernelGGL(st_blend_kernel<float>, grid, dim3(kBlock), 0, st, P);
    else if (a->dtype == SEGM_F16) hipLaunchKernelGGL(st_blend_kernel<f16_t>, grid, dim3(kBlock), 0, st, P);
    else hipLaunchKernelGGL(st_blend_kernel<bf16_t>, grid, dim3(kBlock), 0, st, P);
    return (int)hipGetLastError();
}

extern "C" int segm_window_finish(const segm_stitch_args* a) {
    if (!a) return SEGM_E_NULL;
    StGeom G;
    const int rc = st_geometry(a, G);
    if (rc != SEGM_OK) return rc;
    if ((int64_t)a->batch * a->channels > 65535) return SEGM_E_SHAPE;
    if (a->mirror < 0 || a->mirror > 7) return SEGM_E_SHAPE;
    if (a->passes < 1 || a->pass < 0 || a->pass >= a->passes) return SEGM_E_SHAPE;
    if (!a->acc || !a->count || !a->total) return SEGM_E_NULL;
    if ((uintptr_t)a->acc % sizeof(float) || (uintptr_t)a->count % sizeof(float) || (uintptr_t)a->total % sizeof(float)) return SEGM_E_SHAPE;
    StFinish P;
    memset(&P, 0, sizeof(P));
    P.acc = a->acc; P.count = a->count; P.total = a->total;
    for (int d = 0; d < 3; ++d) { P.size[d] = a->size[d]; P.img[d] = G.img[d]; P.pad0[d] = G.pad0[d]; }
    P.nq = st_nq(a->size[2]);
    P.nquads = (int32_t)((int64_t)a->size[0] * a->size[1] * P.nq);
    P.mirror = a->mirror;
    P.first = a->pass == 0;
    P.divisor = a->pass == a->passes - 1 ? a->passes : 1;
    hipStream_t st = (hipStream_t)a->stream;
    const dim3 grid(st_blocks(P.nquads), (unsigned)(a->batch * a->channels));
    hipLaunchKernelGGL(st_finish_kernel, grid, dim3(kBlock), 0, st, P);
    const int err = (int)hipGetLastError();
    if (err != 0) return err;
    if (G.img_voxels == G.size_voxels) return SEGM_OK;
    return (int)hipMemsetAsync(a->acc, 0, (size_t)a->batch * a->channels * (size_t)G.img_voxels * sizeof(float), st);
}
