// Finishing a prediction on the device: logits -> label volume in one pass, component sizes and selection
// (C ABI: segm_resample_argmax, segm_ccl_sizes, segm_ccl_select; the roots of the components: ccl_roots.hip).
//
// Replaces what the reference does between `maybe_mirror_and_predict` and the file on disk (light_training/prediction.py):
// `predict_raw_probability` (:33-62, one trilinear interpolation per class into a second full fp32 volume), the `argmax` of
// 4_predict.py:81, `predict_noncrop_probability` (:64-108, a numpy paste on the host) and `large_connected_domain` (:17-27,
// skimage.measure.label + scipy.ndimage.binary_fill_holes on the host).  Here:
//   * resample_argmax_kernel   a thread owns four consecutive output voxels of a row: outside the crop box it writes 0, inside it samples
//                              every class at the voxel's source coordinate (the weights of F.interpolate, trilinear, align_corners
//                              False, fp32), keeps the first largest and stores the four labels as one dword.  The logits are read once
//                              (the eight corners of neighbouring outputs meet in the cache; at identity size one 16-byte packet per
//                              class and thread); optionally the region bit planes of the label go out with it.
//   * ccl_sizes_kernel         counts per root by integer atomic add (exact), aggregated per thread over runs of equal roots and per
//                              workgroup for the workgroup's commonest root; flags the roots whose component touches a face.
//   * ccl_select               arg-max over (count, root index) as one 64-bit key - equal counts: the LAST root wins - by per-workgroup
//                              partials and a one-workgroup final pass; then the mask of the winner / of the components of at least
//                              min_size voxels / of the filled holes.  The winner stays on the device.
// Vector-memory and LDS atomics only.  The CPU emulation build (SEGM_EMU) states the same atomics with the compiler's __atomic builtins.
#include <stdlib.h>
#include <string.h>

#include "ccl_common.h"

namespace segm {

// ---- logits -> labels ---------------------------------------------------------------------------------------------------------------
struct ResDev {
    const void* logits;
    uint8_t* labels;
    uint8_t* regions;
    const uint8_t* table;
    int64_t sc, sz, sy;
    int32_t C, d, h, w;                 // logits
    int32_t z0, y0, x0, D, H, W;        // the box
    int32_t D0, H0, W0;                 // the output volume
    int32_t cpr;                        // four-voxel chunks per output row
    int32_t vec, pack;                  // 16-byte (8-byte) packets of logits are aligned; the outputs take dword stores
    float rz, ry, rx;                   // in / out per axis
    uint32_t nthreads;
};

struct Axis { int32_t i0, i1; float l; };
__device__ __forceinline__ Axis source_index(int dst, float ratio, int in) {
    float s = ((float)dst + 0.5f) * ratio - 0.5f;
    s = s > 0.f ? s : 0.f;
    int i0 = (int)s;                                  // floor: s >= 0
    i0 = i0 < in - 1 ? i0 : in - 1;
    Axis a;
    a.i0 = i0;
    a.i1 = i0 + 1 < in ? i0 + 1 : in - 1;
    a.l = s - (float)i0;
    return a;
}

template <typename T> struct alignas(4 * sizeof(T)) Quad { T e[4]; };

template <typename T, bool IDENT>
__global__ void __launch_bounds__(kBlock) resample_argmax_kernel(ResDev P) {
    __shared__ uint8_t s_tab[256];
    if (P.regions) s_tab[threadIdx.x] = P.table[threadIdx.x];
    __syncthreads();
    const uint32_t gid = (uint32_t)blockIdx.x * kBlock + threadIdx.x;
    if (gid >= P.nthreads) return;
    const uint32_t row = gid / (uint32_t)P.cpr, chunk = gid - row * (uint32_t)P.cpr;
    const int z = (int)(row / (uint32_t)P.H0), y = (int)(row - (uint32_t)z * (uint32_t)P.H0);
    const int x = (int)chunk * 4;
    const int zz = z - P.z0, yy = y - P.y0;
    uint32_t lab[4] = {0u, 0u, 0u, 0u};
    const T* src = reinterpret_cast<const T*>(P.logits);
    if (zz >= 0 && zz < P.D && yy >= 0 && yy < P.H && x + 3 >= P.x0 && x < P.x0 + P.W) {
        if (IDENT) {
            const int64_t base = (int64_t)zz * P.sz + (int64_t)yy * P.sy;
            const int xx = x - P.x0;
            if (P.vec && xx >= 0 && xx + 3 < P.W) {
                float best[4];
                for (int c = 0; c < P.C; ++c) {
                    const Quad<T> q = *reinterpret_cast<const Quad<T>*>(src + (int64_t)c * P.sc + base + xx);
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const float v = to_f32(q.e[k]);
                        if (c == 0) best[k] = v;
                        else if (v > best[k]) { best[k] = v; lab[k] = (uint32_t)c; }
                    }
                }
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    if (xx + k < 0 || xx + k >= P.W) continue;
                    float best = to_f32(src[base + xx + k]);
                    for (int c = 1; c < P.C; ++c) {
                        const float v = to_f32(src[(int64_t)c * P.sc + base + xx + k]);
                        if (v > best) { best = v; lab[k] = (uint32_t)c; }
                    }
                }
            }
        } else {
            const Axis az = source_index(zz, P.rz, P.d), ay = source_index(yy, P.ry, P.h);
            const int64_t r00 = (int64_t)az.i0 * P.sz + (int64_t)ay.i0 * P.sy, r01 = (int64_t)az.i0 * P.sz + (int64_t)ay.i1 * P.sy;
            const int64_t r10 = (int64_t)az.i1 * P.sz + (int64_t)ay.i0 * P.sy, r11 = (int64_t)az.i1 * P.sz + (int64_t)ay.i1 * P.sy;
            const float wz1 = az.l, wz0 = 1.f - az.l, wy1 = ay.l, wy0 = 1.f - ay.l;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int xx = x + k - P.x0;
                if (xx < 0 || xx >= P.W) continue;
                const Axis ax = source_index(xx, P.rx, P.w);
                const float wx1 = ax.l, wx0 = 1.f - ax.l;
                float best = 0.f;
                for (int c = 0; c < P.C; ++c) {
                    const T* pc = src + (int64_t)c * P.sc;
                    const float v00 = wx0 * to_f32(pc[r00 + ax.i0]) + wx1 * to_f32(pc[r00 + ax.i1]);
                    const float v01 = wx0 * to_f32(pc[r01 + ax.i0]) + wx1 * to_f32(pc[r01 + ax.i1]);
                    const float v10 = wx0 * to_f32(pc[r10 + ax.i0]) + wx1 * to_f32(pc[r10 + ax.i1]);
                    const float v11 = wx0 * to_f32(pc[r11 + ax.i0]) + wx1 * to_f32(pc[r11 + ax.i1]);
                    const float v = wz0 * (wy0 * v00 + wy1 * v01) + wz1 * (wy0 * v10 + wy1 * v11);
                    if (c == 0) best = v;
                    else if (v > best) { best = v; lab[k] = (uint32_t)c; }
                }
            }
        }
    }
    const int64_t o = (int64_t)row * P.W0 + x;
    if (P.pack) {                                     // W0 % 4 == 0: the chunk lies inside the row and on a dword
        *reinterpret_cast<uint32_t*>(P.labels + o) = lab[0] | (lab[1] << 8) | (lab[2] << 16) | (lab[3] << 24);
        if (P.regions)
            *reinterpret_cast<uint32_t*>(P.regions + o) = (uint32_t)s_tab[lab[0]] | ((uint32_t)s_tab[lab[1]] << 8) |
                                                           ((uint32_t)s_tab[lab[2]] << 16) | ((uint32_t)s_tab[lab[3]] << 24);
    } else {
        for (int k = 0; k < 4 && x + k < P.W0; ++k) {
            P.labels[o + k] = (uint8_t)lab[k];
            if (P.regions) P.regions[o + k] = s_tab[lab[k]];
        }
    }
}

template <typename T>
static void launch_resample(const ResDev& P, bool ident, hipStream_t st) {
    const dim3 grid((P.nthreads + kBlock - 1) / kBlock), block(kBlock);
    if (ident) hipLaunchKernelGGL((resample_argmax_kernel<T, true>), grid, block, 0, st, P);
    else hipLaunchKernelGGL((resample_argmax_kernel<T, false>), grid, block, 0, st, P);
}

// ---- sizes ----------------------------------------------------------------------------------------------------------------------------
struct SizesDev {
    const int32_t* roots;
    int32_t* sizes;
    uint8_t* touches;
    int32_t D, H, W, N;
};

__global__ void __launch_bounds__(kBlock) ccl_sizes_kernel(SizesDev P) {
    __shared__ int32_t s_key, s_cnt;
    if (threadIdx.x == 0) { s_key = INT32_MAX; s_cnt = 0; }
    __syncthreads();
    const int64_t first = ((int64_t)blockIdx.x * kBlock + threadIdx.x) * kPostVox;
    const uint32_t W = (uint32_t)P.W, HW = (uint32_t)P.H * W;
    int32_t cur = -1, cnt = 0;
    for (int k = 0; k < kPostVox; ++k) {
        const int64_t i = first + k;
        if (i >= P.N) break;
        const int32_t r = P.roots[i];
        if (r < 0) continue;
        const uint32_t z = (uint32_t)i / HW, rem = (uint32_t)i - z * HW, y = rem / W, x = rem - y * W;
        if (x == 0 || x + 1 == W || y == 0 || y + 1 == (uint32_t)P.H || z == 0 || z + 1 == (uint32_t)P.D) P.touches[r] = 1;
        if (r != cur) {
            if (cur >= 0) cnt_add<kScopeAgent>(P.sizes + cur, cnt);
            cur = r;
            cnt = 0;
        }
        ++cnt;
    }
    // the thread's last run: one root per workgroup (the smallest) is added up in LDS, the others go out directly
    if (cur >= 0) lab_min<kScopeWorkgroup>(&s_key, cur);
    __syncthreads();
    const int32_t key = s_key;
    if (cur >= 0) {
        if (cur == key) cnt_add<kScopeWorkgroup>(&s_cnt, cnt);
        else cnt_add<kScopeAgent>(P.sizes + cur, cnt);
    }
    __syncthreads();
    if (threadIdx.x == 0 && key != INT32_MAX) cnt_add<kScopeAgent>(P.sizes + key, s_cnt);
}

// ---- selection ------------------------------------------------------------------------------------------------------------------------
struct SelDev {
    const int32_t* roots;
    const int32_t* sizes;
    const uint8_t* touches;
    uint8_t* out;
    long long* info;
    unsigned long long* part;           // [workgroup][key, components]
    int32_t N, nblocks, mode, min_size;
};

// (key, n) -> the maximum key and the sum of n over the workgroup, valid in thread 0
__device__ __forceinline__ void block_best(unsigned long long& key, unsigned long long& n, unsigned long long* s_key, unsigned long long* s_n) {
    const int tid = threadIdx.x;
    s_key[tid] = key;
    s_n[tid] = n;
    __syncthreads();
    for (int off = kBlock / 2; off >= 1; off >>= 1) {
        if (tid < off) {
            s_key[tid] = s_key[tid] > s_key[tid + off] ? s_key[tid] : s_key[tid + off];
            s_n[tid] += s_n[tid + off];
        }
        __syncthreads();
    }
    key = s_key[0];
    n = s_n[0];
}

__global__ void __launch_bounds__(kBlock) ccl_best_kernel(SelDev P) {
    __shared__ unsigned long long s_key[kBlock], s_n[kBlock];
    unsigned long long key = 0, n = 0;
    const int64_t base = (int64_t)blockIdx.x * kPostChunk;
    for (int k = 0; k < kPostVox; ++k) {
        const int64_t i = base + (int64_t)k * kBlock + threadIdx.x;
        if (i >= P.N) break;
        const int32_t s = P.sizes[i];
        if (s > 0) {
            const unsigned long long c = ((unsigned long long)(uint32_t)s << 32) | (unsigned long long)(uint32_t)i;
            key = c > key ? c : key;                  // equal counts: the later root wins
            ++n;
        }
    }
    block_best(key, n, s_key, s_n);
    if (threadIdx.x == 0) {
        P.part[2 * (size_t)blockIdx.x] = key;
        P.part[2 * (size_t)blockIdx.x + 1] = n;
    }
}

__global__ void __launch_bounds__(kBlock) ccl_best_final_kernel(SelDev P) {
    __shared__ unsigned long long s_key[kBlock], s_n[kBlock];
    unsigned long long key = 0, n = 0;
    for (int b = threadIdx.x; b < P.nblocks; b += kBlock) {
        const unsigned long long c = P.part[2 * (size_t)b];
        key = c > key ? c : key;
        n += P.part[2 * (size_t)b + 1];
    }
    block_best(key, n, s_key, s_n);
    if (threadIdx.x == 0) {
        P.info[0] = (long long)n;
        P.info[1] = key ? (long long)(key & 0xffffffffull) : -1ll;
        P.info[2] = (long long)(key >> 32);
    }
}

__global__ void __launch_bounds__(kBlock) ccl_select_kernel(SelDev P) {
    const uint32_t i = (uint32_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= (uint32_t)P.N) return;
    const int32_t r = P.roots[i];
    bool on;
    if (P.mode == SEGM_CCL_LARGEST) on = r >= 0 && (long long)r == P.info[1];
    else if (P.mode == SEGM_CCL_MIN_SIZE) on = r >= 0 && P.sizes[r] >= P.min_size;
    else on = r < 0 || P.touches[r] == 0;
    P.out[i] = on ? 1 : 0;
}

}  // namespace segm

using namespace segm;

extern "C" int segm_resample_argmax(const segm_resample_argmax_args* a) {
    if (!a) return SEGM_E_NULL;
    if (!a->logits || !a->labels || (a->regions && !a->table)) return SEGM_E_NULL;
    if (a->classes < 1 || a->classes > SEGM_RESAMPLE_CLASS_LIMIT) return SEGM_E_SHAPE;
    if (a->in_depth <= 0 || a->in_height <= 0 || a->in_width <= 0) return SEGM_E_SHAPE;
    if (!ccl_volume_ok(a->out_depth, a->out_height, a->out_width)) return SEGM_E_SHAPE;
    if (a->box_depth <= 0 || a->box_height <= 0 || a->box_width <= 0 || a->box_z < 0 || a->box_y < 0 || a->box_x < 0) return SEGM_E_SHAPE;
    if ((int64_t)a->box_z + a->box_depth > a->out_depth || (int64_t)a->box_y + a->box_height > a->out_height ||
        (int64_t)a->box_x + a->box_width > a->out_width) return SEGM_E_SHAPE;
    if (a->stride_y < a->in_width || a->stride_z < 0 || a->stride_c < 0) return SEGM_E_SHAPE;
    if (a->dtype != SEGM_F32 && a->dtype != SEGM_F16 && a->dtype != SEGM_BF16) return SEGM_E_DTYPE;
    const int esize = a->dtype == SEGM_F32 ? 4 : 2;
    if ((uintptr_t)a->logits % esize) return SEGM_E_SHAPE;
    ResDev P;
    memset(&P, 0, sizeof(P));
    P.logits = a->logits; P.labels = a->labels; P.regions = a->regions; P.table = a->table;
    P.sc = a->stride_c; P.sz = a->stride_z; P.sy = a->stride_y;
    P.C = a->classes; P.d = a->in_depth; P.h = a->in_height; P.w = a->in_width;
    P.z0 = a->box_z; P.y0 = a->box_y; P.x0 = a->box_x; P.D = a->box_depth; P.H = a->box_height; P.W = a->box_width;
    P.D0 = a->out_depth; P.H0 = a->out_height; P.W0 = a->out_width;
    P.cpr = (a->out_width + 3) / 4;
    const int64_t nthreads = (int64_t)a->out_depth * a->out_height * P.cpr;
    P.nthreads = (uint32_t)nthreads;
    P.rz = (float)a->in_depth / (float)a->box_depth;
    P.ry = (float)a->in_height / (float)a->box_height;
    P.rx = (float)a->in_width / (float)a->box_width;
    const bool ident = a->in_depth == a->box_depth && a->in_height == a->box_height && a->in_width == a->box_width;
    P.vec = ident && a->box_x % 4 == 0 && a->out_width % 4 == 0 && a->stride_c % 4 == 0 && a->stride_z % 4 == 0 && a->stride_y % 4 == 0 &&
            (uintptr_t)a->logits % (4 * esize) == 0;
    P.pack = a->out_width % 4 == 0 && (uintptr_t)a->labels % 4 == 0 && (uintptr_t)a->regions % 4 == 0;
    hipStream_t st = (hipStream_t)a->stream;
    if (a->dtype == SEGM_F32) launch_resample<float>(P, ident, st);
    else if (a->dtype == SEGM_F16) launch_resample<f16_t>(P, ident, st);
    else launch_resample<bf16_t>(P, ident, st);
    return (int)hipGetLastError();
}

extern "C" int segm_ccl_sizes(const segm_ccl_sizes_args* a) {
    if (!a) return SEGM_E_NULL;
    if (!a->roots || !a->sizes || !a->touches) return SEGM_E_NULL;
    if (!ccl_volume_ok(a->depth, a->height, a->width)) return SEGM_E_SHAPE;
    if ((uintptr_t)a->roots % sizeof(int32_t) || (uintptr_t)a->sizes % sizeof(int32_t)) return SEGM_E_SHAPE;
    const int64_t N = (int64_t)a->depth * a->height * a->width;
    SizesDev P;
    memset(&P, 0, sizeof(P));
    P.roots = a->roots; P.sizes = a->sizes; P.touches = a->touches;
    P.D = a->depth; P.H = a->height; P.W = a->width; P.N = (int32_t)N;
    hipStream_t st = (hipStream_t)a->stream;
    if (hipMemsetAsync(a->sizes, 0, (size_t)N * sizeof(int32_t), st) != hipSuccess) return (int)hipGetLastError();
    if (hipMemsetAsync(a->touches, 0, (size_t)N, st) != hipSuccess) return (int)hipGetLastError();
    hipLaunchKernelGGL(ccl_sizes_kernel, dim3((unsigned)post_blocks(N)), dim3(kBlock), 0, st, P);
    return (int)hipGetLastError();
}

extern "C" size_t segm_ccl_select_workspace_bytes(int64_t voxels) {
    if (voxels <= 0 || voxels > SEGM_CCL_MAX_VOXELS) return 0;
    return (size_t)post_blocks(voxels) * 2 * sizeof(unsigned long long);
}

extern "C" int segm_ccl_select(const segm_ccl_select_args* a) {
    if (!a) return SEGM_E_NULL;
    if (!a->roots || !a->sizes || !a->out || !a->info) return SEGM_E_NULL;
    if (a->mode != SEGM_CCL_LARGEST && a->mode != SEGM_CCL_MIN_SIZE && a->mode != SEGM_CCL_FILL) return SEGM_E_SHAPE;
    if (a->mode == SEGM_CCL_FILL && !a->touches) return SEGM_E_NULL;
    if (!ccl_volume_ok(a->depth, a->height, a->width)) return SEGM_E_SHAPE;
    if ((uintptr_t)a->roots % sizeof(int32_t) || (uintptr_t)a->sizes % sizeof(int32_t) || (uintptr_t)a->info % sizeof(int64_t)) return SEGM_E_SHAPE;
    const int64_t N = (int64_t)a->depth * a->height * a->width;
    if (!a->workspace || a->workspace_bytes < segm_ccl_select_workspace_bytes(N) || (uintptr_t)a->workspace % sizeof(unsigned long long)) return SEGM_E_WORKSPACE;
    SelDev P;
    memset(&P, 0, sizeof(P));
    P.roots = a->roots; P.sizes = a->sizes; P.touches = a->touches; P.out = a->out; P.info = (long long*)a->info;
    P.part = (unsigned long long*)a->workspace;
    P.N = (int32_t)N; P.nblocks = (int32_t)post_blocks(N); P.mode = a->mode; P.min_size = a->min_size;
    hipStream_t st = (hipStream_t)a->stream;
    hipLaunchKernelGGL(ccl_best_kernel, dim3((unsigned)P.nblocks), dim3(kBlock), 0, st, P);
    hipLaunchKernelGGL(ccl_best_final_kernel, dim3(1), dim3(kBlock), 0, st, P);
    hipLaunchKernelGGL(ccl_select_kernel, dim3((unsigned)((N + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, P);
    return (int)hipGetLastError();
}
