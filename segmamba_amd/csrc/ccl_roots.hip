// Connected components: the root of every voxel, of a binary mask or of every class of a label volume, at connectivity 1, 2 or 3
// (C ABI: segm_ccl_roots, segm_ccl_label_roots - connectivity 1 - and segm_ccl_roots_conn, segm_ccl_label_roots_conn).
//
// The reference's `large_connected_domain` (light_training/prediction.py:17-27, skimage.measure.label on the host) labels one binary
// mask at connectivity 1; its CT example (light_training/examples/AbdomenAtlas1.0Mini/4_predict_diffunet.py:87-109) takes the argmax
// over 10 classes and writes `labels == i` per organ - per organ through a binary entry that is nine passes over the volume, while a
// label volume holds every organ's components at once.  nnU-Net's "keep the largest component of every class", cc3d and the BraTS
// lesion-wise tooling label at FULL connectivity: a vessel that hangs on its organ by an edge or a corner is one component with it.
//
// One kernel family serves all of it.  A voxel's VALUE is 0 / 1 by `bit` and `invert` for a mask (LAB = false) and its label for a
// label volume (LAB = true); two neighbours are joined iff their values are equal and not 0.  Connectivity c (CONN) is that of
// scipy.ndimage.generate_binary_structure(3, c): an offset (dz, dy, dx) is a neighbour when it has at most c non-zero coordinates,
// each +-1 (6, 18 or 26 neighbours).  In memory order a voxel has these PREVIOUS neighbours - joining every voxel with its previous
// neighbours joins every neighbouring pair exactly once:
//     (0, 0, -1)  (0, -1, 0)  (-1, 0, 0)                                              every c      3
//     (0, -1, +-1)  (-1, 0, +-1)  (-1, +-1, 0)                                        c >= 2       9
//     (-1, +-1, +-1)                                                                  c == 3      13
// The root of a component is DEFINED as its smallest linear voxel index, so the result - and with it the sizes, the selection, the
// hole filling and the tie rule above it - depends neither on the order of anything nor on which unions are made, as long as the
// unions made connect exactly the voxels of a component.  Block-based union-find (ccl_common.h: the 64 x 4 x 4 tile, lab_union /
// lab_find on relaxed atomics where labels only ever decrease and always name a voxel of the same component), three launches and no
// readback, whatever the volume and the shape of the mask:
//   * roots_tile_kernel     a workgroup owns a tile in LDS, a wave a z of it and four rows along x.  A row starts as its RUNS along x
//                           from one ballot: a voxel starts with the first voxel of its run (clz).  For a mask the run starts are the
//                           zeros of the row's mask; a run of labels ends where the label changes (`1 1 2 2` is two runs), so the
//                           starts are a ballot of "labelled and (lane 0 or the label differs from the left lane's)".  A row is then
//                           joined with each previous row of its tile: the row above in y and the row below in z, and from c = 2 the
//                           rows y - 1 and y + 1 of the plane below.  Per pair of rows three candidate words: the voxel straight
//                           across (`centre`) and, where c admits them, the two diagonal ones - for a mask `m & prev`,
//                           `m & (prev << 1)`, `m & (prev >> 1)` of the row masks in LDS (no value array is kept); for labels three
//                           ballots of "my label is the label there" on the label bytes in LDS.  Lane 0 has no left and lane 63 no
//                           right candidate (the shifts bring in zeros; the label form tests the lane): those pairs belong to the
//                           merge launch.  Local index order = global index order inside a tile, so every voxel leaves with the
//                           global index of its tile-local root.
//     Unions that are left out, and why the components stay the same:
//       - a centre candidate whose left lane is a centre candidate too and continues the same run: the two voxels are one run here
//         and the two across are one run there, and a run is one component from the start; the left lane's union covers both.  For
//         a mask adjacent candidates always continue a run; for labels the second still starts its own union when it is a run start
//         (stripes one voxel wide along x): `inner`;
//       - a diagonal candidate where the centre is a candidate too: the centre voxel and the diagonal one are x-neighbours of equal
//         value in the previous row, so they are one run; the centre union - made, or left to the left lane as above - covers both.
//   * roots_merge_kernel    a thread per voxel on a face of its tile that is no side of the volume (at c = 1 the low faces only: no
//                           previous neighbour lies across a high one): every previous neighbour under c that lies in ANOTHER tile -
//                           across a face, or diagonal to the voxel's tile in two or three axes - and has the voxel's value is joined
//                           with it by the same union-find on the global labels.  EVERY access to a label in this launch is an
//                           agent-scope relaxed atomic (__hip_atomic_load / __hip_atomic_fetch_min: they bypass the per-CU L1 and are
//                           served where all XCDs agree); no workgroup waits for another, so the loops end whatever the order.  The
//                           neighbours are taken as in the tile launch, a previous row (dz, dy) at a time - centre, then the two
//                           beside it - and a row none of whose voxels lies in another tile is not read; the plane below comes
//                           first and the left neighbour last.  The sides of the volume are tested on the coordinates: x - 1 at
//                           x = 0 and x + 1 at x = width - 1 are no neighbours although they are adjacent linear indices.
//     Left out:
//       - a diagonal neighbour (dz, dy, +-1) when the voxel (dz, dy, 0) between has the value too.  That voxel is one component with
//         this one (by the tile launch when it lies in this tile, by this launch otherwise) and with its x-neighbour (one run in a
//         tile; across an x face by the (0, 0, -1) union of whichever of the two has the larger x, which is never left out);
//       - the run rule: the neighbour straight across, (dz, dy, 0), when the left neighbour lies in this tile and has the value and
//         the voxel diagonally across, (dz, dy, -1), has it too.  This voxel and its left neighbour are one run of this tile, the
//         two across are one run of that tile, and the left neighbour's thread joins the two runs: its own union straight across
//         is made unless this rule leaves it to ITS left neighbour, which ends at the first voxel of the run or at the tile's x
//         face, where the rule does not apply.  Of a run of face voxels only the first starts a union.
//   * roots_flatten_kernel  roots[i] = the end of i's chain (plain loads: the labels are read-only now).  A chain is as long as the
//                           number of tiles a path crosses at worst (the serpentine), and is walked by the thread that owns the voxel.
// The only unbounded loops are lab_find / lab_union.  Vector-memory and LDS atomics only.  The CPU emulation build (SEGM_EMU)
// states the same atomics with the compiler's __atomic builtins.
#include <stdlib.h>
#include <string.h>

#include "ccl_common.h"

namespace segm {

static_assert(kBlock == kTX * kTZ, "a wave per z of the tile");
typedef unsigned long long u64_t;

struct RootsDev {
    const uint8_t* vol;
    int32_t* lab;
    int32_t* roots;
    int32_t D, H, W, N;
    int32_t bit, invert;
    int32_t tx, ty;                     // tiles along x and y
};

// a voxel's value: its label, or 0 / 1 for outside / inside the mask
template <bool LAB> __device__ __forceinline__ int roots_value(uint32_t v, const RootsDev& P) {
    if constexpr (LAB) return (int)v;
    const int in = P.bit >= 0 ? (int)((v >> P.bit) & 1u) : (int)(v != 0u);
    return in != P.invert ? 1 : 0;
}

// `row` with the previous row `prow` of the tile: the voxel straight across and, with DIAG, the two beside it.  s_mask: the row's
// voxels (mask) or the first voxels of the row's runs (labels); `mine`: this lane's value in `row`
template <bool LAB, bool DIAG>
__device__ __forceinline__ void roots_join_rows(int32_t* s_lab, const u64_t* s_mask, const uint8_t* s_val, int row, int prow, int lane, int mine) {
    u64_t c0, cl = 0, cr = 0, inner = ~0ull;
    if constexpr (LAB) {
        const uint8_t* pv = s_val + prow * kTX;
        c0 = __ballot(mine != 0 && (int)pv[lane] == mine ? 1 : 0);
        inner = ~s_mask[row];                                                           // not the first voxel of a run
        if constexpr (DIAG) {
            cl = __ballot(mine != 0 && lane > 0 && (int)pv[lane > 0 ? lane - 1 : 0] == mine ? 1 : 0);
            cr = __ballot(mine != 0 && lane < kTX - 1 && (int)pv[lane < kTX - 1 ? lane + 1 : lane] == mine ? 1 : 0);
        }
    } else {
        const u64_t m = s_mask[row], prev = s_mask[prow];
        c0 = m & prev;
        if constexpr (DIAG) { cl = m & (prev << 1); cr = m & (prev >> 1); }
    }
    const int me = row * kTX + lane, across = prow * kTX + lane;
    if (((c0 & ~((c0 << 1) & inner)) >> lane) & 1ull) lab_union<kScopeWorkgroup>(s_lab, me, across);
    if constexpr (DIAG) {
        if (((cl & ~c0) >> lane) & 1ull) lab_union<kScopeWorkgroup>(s_lab, me, across - 1);
        if (((cr & ~c0) >> lane) & 1ull) lab_union<kScopeWorkgroup>(s_lab, me, across + 1);
    }
}

template <bool LAB, int CONN> __global__ void __launch_bounds__(kBlock) roots_tile_kernel(RootsDev P) {
    __shared__ int32_t s_lab[kTileVox];
    __shared__ u64_t s_mask[kTileRows];
    __shared__ uint8_t s_val[LAB ? kTileVox : 1];     // labels only
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t t = blockIdx.x;
    const uint32_t bx = t % (uint32_t)P.tx;
    t /= (uint32_t)P.tx;
    const uint32_t by = t % (uint32_t)P.ty, bz = t / (uint32_t)P.ty;
    const int x = (int)bx * kTX + lane, z = (int)bz * kTZ + wave;
    int v[kTY];
#pragma unroll
    for (int ly = 0; ly < kTY; ++ly) {
        const int row = wave * kTY + ly, y = (int)by * kTY + ly;
        v[ly] = 0;
        if (x < P.W && y < P.H && z < P.D) v[ly] = roots_value<LAB>(P.vol[((int64_t)z * P.H + y) * P.W + x], P);
        int start;
        if constexpr (LAB) {
            const int left = __shfl(v[ly], (lane + 63) & 63);
            const u64_t s = __ballot(v[ly] != 0 && (lane == 0 || left != v[ly]) ? 1 : 0);
            if (lane == 0) s_mask[row] = s;
            s_val[row * kTX + lane] = (uint8_t)v[ly];
            start = 63 - __builtin_clzll((s & ((2ull << lane) - 1ull)) | 1ull);        // the last run start at or left of this lane
        } else {
            const u64_t m = __ballot(v[ly]);
            if (lane == 0) s_mask[row] = m;
            const u64_t zl = ~m & ((1ull << lane) - 1ull);
            start = zl ? 64 - __builtin_clzll(zl) : 0;
        }
        s_lab[row * kTX + lane] = v[ly] != 0 ? row * kTX + start : -1;
    }
    __syncthreads();
    constexpr bool edges = CONN >= 2, corners = CONN >= 3;
#pragma unroll
    for (int ly = 0; ly < kTY; ++ly) {
        const int row = wave * kTY + ly;
        if (ly > 0) roots_join_rows<LAB, edges>(s_lab, s_mask, s_val, row, row - 1, lane, v[ly]);                        // (0, -1, *)
        if (wave > 0) {
            roots_join_rows<LAB, edges>(s_lab, s_mask, s_val, row, row - kTY, lane, v[ly]);                              // (-1, 0, *)
            if (edges && ly > 0) roots_join_rows<LAB, corners>(s_lab, s_mask, s_val, row, row - kTY - 1, lane, v[ly]);   // (-1, -1, *)
            if (edges && ly < kTY - 1) roots_join_rows<LAB, corners>(s_lab, s_mask, s_val, row, row - kTY + 1, lane, v[ly]);   // (-1, +1, *)
        }
    }
    __syncthreads();
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

// voxel i = (x, y, z) of value v with the previous row (dz, dy): the voxel straight across and, with DIAG, the two beside it, where
// they lie in another tile.  run: the left neighbour lies in this tile and has the value
template <bool LAB, bool DIAG>
__device__ __forceinline__ void roots_merge_row(const RootsDev& P, uint32_t i, int v, int x, int y, int z, bool run, int dz, int dy) {
    if (y + dy < 0 || y + dy >= P.H || z + dz < 0) return;                                    // the sides of the volume
    const int lx = x % kTX, ly = y % kTY, lz = z % kTZ;
    const bool rowfar = (dy < 0 && ly == 0) || (dy > 0 && ly == kTY - 1) || (dz < 0 && lz == 0);
    if (!rowfar && !(DIAG && (lx == 0 || lx == kTX - 1))) return;                              // the row's three voxels are in this tile
    const int64_t j = (int64_t)i + dz * ((int64_t)P.H * P.W) + dy * (int64_t)P.W;
    if (roots_value<LAB>(P.vol[j], P) == v) {                                                  // the centre: no diagonal union
        if (rowfar && !(run && roots_value<LAB>(P.vol[j - 1], P) == v)) lab_union<kScopeAgent>(P.lab, (int32_t)i, (int32_t)j);
        return;
    }
    if constexpr (DIAG) {
        if (x > 0 && (rowfar || lx == 0) && roots_value<LAB>(P.vol[j - 1], P) == v) lab_union<kScopeAgent>(P.lab, (int32_t)i, (int32_t)(j - 1));
        if (x < P.W - 1 && (rowfar || lx == kTX - 1) && roots_value<LAB>(P.vol[j + 1], P) == v) lab_union<kScopeAgent>(P.lab, (int32_t)i, (int32_t)(j + 1));
    }
}

template <bool LAB, int CONN> __global__ void __launch_bounds__(kBlock) roots_merge_kernel(RootsDev P) {
    const uint32_t i = (uint32_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= (uint32_t)P.N) return;
    const int v = roots_value<LAB>(P.vol[i], P);
    if (v == 0) return;
    const uint32_t Wu = (uint32_t)P.W, HWu = (uint32_t)P.H * Wu;
    const uint32_t zu = i / HWu, rem = i - zu * HWu, yu = rem / Wu;
    const int x = (int)(rem - yu * Wu), y = (int)yu, z = (int)zu;
    const int lx = x % kTX, ly = y % kTY, lz = z % kTZ;
    const bool low = (lx == 0 && x > 0) || (ly == 0 && y > 0) || (lz == 0 && z > 0);
    const bool high = CONN >= 2 && ((lx == kTX - 1 && x < P.W - 1) || (ly == kTY - 1 && y < P.H - 1));
    if (!(low || high)) return;                                                                // every neighbour is in this tile
    const bool left = x > 0 && roots_value<LAB>(P.vol[i - 1], P) == v;                         // (0, 0, -1)
    const bool run = left && lx != 0;
    constexpr bool edges = CONN >= 2, corners = CONN >= 3;
    if constexpr (edges) roots_merge_row<LAB, corners>(P, i, v, x, y, z, run, -1, -1);
    roots_merge_row<LAB, edges>(P, i, v, x, y, z, run, -1, 0);
    if constexpr (edges) roots_merge_row<LAB, corners>(P, i, v, x, y, z, run, -1, 1);
    roots_merge_row<LAB, edges>(P, i, v, x, y, z, run, 0, -1);
    if (left && lx == 0) lab_union<kScopeAgent>(P.lab, (int32_t)i, (int32_t)(i - 1));
}

__global__ void __launch_bounds__(kBlock) roots_flatten_kernel(RootsDev P) {
    const uint32_t i = (uint32_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= (uint32_t)P.N) return;
    int32_t l = P.lab[i];
    if (l >= 0)
        while (P.lab[l] != l) l = P.lab[l];
    P.roots[i] = l;
}

template <bool LAB>
static int roots_launch(const uint8_t* vol, int32_t* roots, void* workspace, int d, int h, int w, int bit, int invert, int conn, void* stream) {
    RootsDev P;
    memset(&P, 0, sizeof(P));
    P.vol = vol; P.lab = (int32_t*)workspace; P.roots = roots;
    P.D = d; P.H = h; P.W = w; P.N = (int32_t)((int64_t)d * h * w);
    P.bit = bit; P.invert = invert;
    P.tx = (w + kTX - 1) / kTX;
    P.ty = (h + kTY - 1) / kTY;
    const int64_t tiles = (int64_t)P.tx * P.ty * ((d + kTZ - 1) / kTZ);             // <= N: every tile holds a voxel
    void (*tile)(RootsDev) = conn == 1 ? roots_tile_kernel<LAB, 1> : conn == 2 ? roots_tile_kernel<LAB, 2> : roots_tile_kernel<LAB, 3>;
    void (*merge)(RootsDev) = conn == 1 ? roots_merge_kernel<LAB, 1> : conn == 2 ? roots_merge_kernel<LAB, 2> : roots_merge_kernel<LAB, 3>;
    hipStream_t st = (hipStream_t)stream;
    const dim3 flat((unsigned)(((int64_t)P.N + kBlock - 1) / kBlock)), block(kBlock);
    hipLaunchKernelGGL(tile, dim3((unsigned)tiles), block, 0, st, P);
    hipLaunchKernelGGL(merge, flat, block, 0, st, P);
    hipLaunchKernelGGL(roots_flatten_kernel, flat, block, 0, st, P);
    return (int)hipGetLastError();
}

// the refusals of all four entries, in their order: NULL, connectivity, shape (bit / invert for a mask: bit = -1, invert = 0 for
// labels), workspace.  0: the call is in order
static int roots_check(const void* vol, const int32_t* roots, int conn, int64_t d, int64_t h, int64_t w, int bit, int invert,
                       const void* workspace, size_t workspace_bytes) {
    if (!vol || !roots) return SEGM_E_NULL;
    if (conn < 1 || conn > 3) return SEGM_E_SHAPE;
    if (!ccl_volume_ok(d, h, w)) return SEGM_E_SHAPE;
    if (bit < -1 || bit > 7 || (invert != 0 && invert != 1)) return SEGM_E_SHAPE;
    if ((uintptr_t)roots % sizeof(int32_t)) return SEGM_E_SHAPE;
    if (!workspace || workspace_bytes < segm_ccl_roots_workspace_bytes(d * h * w) || (uintptr_t)workspace % sizeof(int32_t)) return SEGM_E_WORKSPACE;
    return 0;
}

}  // namespace segm

using namespace segm;

extern "C" size_t segm_ccl_roots_workspace_bytes(int64_t voxels) {
    if (voxels <= 0 || voxels > SEGM_CCL_MAX_VOXELS) return 0;
    return (size_t)voxels * sizeof(int32_t);
}

extern "C" size_t segm_ccl_label_roots_workspace_bytes(int64_t voxels) { return segm_ccl_roots_workspace_bytes(voxels); }

extern "C" int segm_ccl_roots(const segm_ccl_roots_args* a) {                         // `reserved` is not read
    if (!a) return SEGM_E_NULL;
    if (const int rc = roots_check(a->volume, a->roots, 1, a->depth, a->height, a->width, a->bit, a->invert, a->workspace, a->workspace_bytes)) return rc;
    return roots_launch<false>(a->volume, a->roots, a->workspace, a->depth, a->height, a->width, a->bit, a->invert, 1, a->stream);
}

extern "C" int segm_ccl_roots_conn(const segm_ccl_roots_conn_args* a) {
    if (!a) return SEGM_E_NULL;
    if (const int rc = roots_check(a->volume, a->roots, a->connectivity, a->depth, a->height, a->width, a->bit, a->invert, a->workspace, a->workspace_bytes)) return rc;
    return roots_launch<false>(a->volume, a->roots, a->workspace, a->depth, a->height, a->width, a->bit, a->invert, a->connectivity, a->stream);
}

extern "C" int segm_ccl_label_roots(const segm_ccl_label_roots_args* a) {             // `reserved` is not read
    if (!a) return SEGM_E_NULL;
    if (const int rc = roots_check(a->labels, a->roots, 1, a->depth, a->height, a->width, -1, 0, a->workspace, a->workspace_bytes)) return rc;
    return roots_launch<true>(a->labels, a->roots, a->workspace, a->depth, a->height, a->width, -1, 0, 1, a->stream);
}

extern "C" int segm_ccl_label_roots_conn(const segm_ccl_label_roots_conn_args* a) {
    if (!a) return SEGM_E_NULL;
    if (const int rc = roots_check(a->labels, a->roots, a->connectivity, a->depth, a->height, a->width, -1, 0, a->workspace, a->workspace_bytes)) return rc;
    return roots_launch<true>(a->labels, a->roots, a->workspace, a->depth, a->height, a->width, -1, 0, a->connectivity, a->stream);
}
