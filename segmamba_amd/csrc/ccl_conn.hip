// Connected components at connectivity 2 and 3, of a binary mask and of every class of a label volume
// (C ABI: segm_ccl_roots_conn, segm_ccl_label_roots_conn; connectivity 1 forwards to segm_ccl_roots / segm_ccl_label_roots).
//
// The reference's `large_connected_domain` (light_training/prediction.py:17-27) labels at connectivity 1, and postprocess.hip /
// ccl_labels.hip restate that.  nnU-Net's "keep the largest component of every class", cc3d and the BraTS lesion-wise tooling label
// at FULL connectivity: a vessel that hangs on its organ by an edge or a corner is one component with it.  `connectivity` c is that
// of scipy.ndimage.generate_binary_structure(3, c): an offset (dz, dy, dx) is a neighbour when it has at most c non-zero coordinates,
// each +-1 (6, 18 or 26 neighbours).  In memory order a voxel has these PREVIOUS neighbours - joining every voxel with its previous
// neighbours joins every neighbouring pair exactly once:
//     (0, 0, -1)  (0, -1, 0)  (-1, 0, 0)                                              every c      3
//     (0, -1, +-1)  (-1, 0, +-1)  (-1, +-1, 0)                                        c >= 2       9
//     (-1, +-1, +-1)                                                                  c == 3      13
// The result - every voxel gets the smallest linear index of its component - and with it the sizes, the selection, the hole
// filling and the tie rule above it do not depend on c.  The structure is that of the siblings (ccl_common.h: the 64 x 4 x 4 tile in
// LDS, lab_union / lab_find on relaxed atomics, three launches, no readback); one kernel source serves both entries: a voxel's VALUE
// is 0 / 1 by `bit` and `invert` for a mask and its label for a label volume, and two neighbours are joined iff their values are
// equal and not 0.
//   * conn_tile_kernel    rows start as runs along x from one ballot, as in the siblings.  A row is then joined with each previous row
//                         of its tile: the row above in y, and the rows y - 1, y, y + 1 of the plane below in z.  Per pair of rows three
//                         candidate words: the voxel straight across (`centre`) and, where c admits them, the two diagonal ones - for a
//                         mask `m & prev`, `m & (prev << 1)`, `m & (prev >> 1)` of the row masks in LDS; for labels three ballots of
//                         "my label is the label there" on the label bytes in LDS.  Lane 0 has no left and lane 63 no right candidate
//                         (the shifts bring in zeros; the label form tests the lane): those pairs belong to the merge launch.
//     Unions that are left out, and why the components stay the same:
//       - a diagonal candidate where the centre is a candidate too: the centre voxel and the diagonal one are x-neighbours of equal
//         value in the previous row, so they are one run, which is one component from the start; the centre union covers both;
//       - a centre candidate whose left lane is a centre candidate too and (labels) continues the same run: the two voxels are one
//         run here and the two across are one run there (the siblings' rule).
//   * conn_merge_kernel   a thread per voxel: every previous neighbour under c that lies in ANOTHER tile - across a face, or diagonal to
//                         the voxel's tile in two or three axes - and has the voxel's value is joined with it on the global labels
//                         (agent-scope relaxed atomics throughout, as in the siblings).  The thirteen tests are made first (independent
//                         loads), the unions after.  The sides of the volume are tested on the coordinates: x - 1 at x = 0 and x + 1
//                         at x = width - 1 are no neighbours although they are adjacent linear indices.
//     Left out: a diagonal neighbour (dz, dy, +-1) when the voxel (dz, dy, 0) between has the value too.  That voxel is joined with this
//     one (by the tile launch when it lies in this tile, by this thread otherwise) and with its x-neighbour (one run in a tile; across
//     an x face by the (0, 0, -1) union of whichever of the two has the larger x, which is never left out).
//   * ccl_flatten_kernel  of postprocess.hip, as it is: roots[i] = the end of i's chain (plain loads: the labels are read-only now).
// The only unbounded loops are lab_find / lab_union (labels only decrease).  Vector-memory and LDS atomics only.
#include <stdlib.h>
#include <string.h>

#include "ccl_common.h"

namespace segm {

static_assert(kBlock == kTX * kTZ, "a wave per z of the tile");
typedef unsigned long long u64_t;

struct ConnDev {
    const uint8_t* vol;
    int32_t* lab;
    int32_t* roots;
    int32_t D, H, W, N;
    int32_t bit, invert, conn;
    int32_t tx, ty;                     // tiles along x and y
};

// a voxel's value: its label, or 0 / 1 for outside / inside the mask
template <bool LAB> __device__ __forceinline__ int conn_value(uint32_t v, const ConnDev& P) {
    if constexpr (LAB) return (int)v;
    const int in = P.bit >= 0 ? (int)((v >> P.bit) & 1u) : (int)(v != 0u);
    return in != P.invert ? 1 : 0;
}

template <bool LAB> __global__ void __launch_bounds__(kBlock) conn_tile_kernel(ConnDev P) {
    __shared__ int32_t s_lab[kTileVox];
    __shared__ u64_t s_mask[kTileRows];               // mask: the row's voxels; labels: the first voxels of the row's runs
    __shared__ uint8_t s_val[LAB ? kTileVox : 1];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t t = blockIdx.x;
    const uint32_t bx = t % (uint32_t)P.tx;
    t /= (uint32_t)P.tx;
    const uint32_t by = t % (uint32_t)P.ty, bz = t / (uint32_t)P.ty;
    const int x = (int)bx * kTX + lane, z = (int)bz * kTZ + wave;
    int v[kTY];
    // a voxel starts with the first voxel of its run along x; a run of labels ends where the label changes
#pragma unroll
    for (int ly = 0; ly < kTY; ++ly) {
        const int row = wave * kTY + ly, y = (int)by * kTY + ly;
        v[ly] = 0;
        if (x < P.W && y < P.H && z < P.D) v[ly] = conn_value<LAB>(P.vol[((int64_t)z * P.H + y) * P.W + x], P);
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
    const bool edges = P.conn >= 2, corners = P.conn >= 3;
#pragma unroll
    for (int ly = 0; ly < kTY; ++ly) {
        const int row = wave * kTY + ly, mine = v[ly];
        // `row` with the previous row `prow`: the voxel straight across, and with `diag` the two beside it
        auto join = [&](int prow, bool diag) {
            u64_t c0, cl = 0, cr = 0, inner = ~0ull;
            if constexpr (LAB) {
                const uint8_t* pv = s_val + prow * kTX;
                c0 = __ballot(mine != 0 && (int)pv[lane] == mine ? 1 : 0);
                inner = ~s_mask[row];                                                   // not the first voxel of a run
                if (diag) {
                    cl = __ballot(mine != 0 && lane > 0 && (int)pv[lane > 0 ? lane - 1 : 0] == mine ? 1 : 0);
                    cr = __ballot(mine != 0 && lane < kTX - 1 && (int)pv[lane < kTX - 1 ? lane + 1 : lane] == mine ? 1 : 0);
                }
            } else {
                const u64_t m = s_mask[row], prev = s_mask[prow];
                c0 = m & prev;
                if (diag) { cl = m & (prev << 1); cr = m & (prev >> 1); }
            }
            const int me = row * kTX + lane, across = prow * kTX + lane;
            if (((c0 & ~((c0 << 1) & inner)) >> lane) & 1ull) lab_union<kScopeWorkgroup>(s_lab, me, across);
            if (((cl & ~c0) >> lane) & 1ull) lab_union<kScopeWorkgroup>(s_lab, me, across - 1);
            if (((cr & ~c0) >> lane) & 1ull) lab_union<kScopeWorkgroup>(s_lab, me, across + 1);
        };
        if (ly > 0) join(row - 1, edges);                                               // (0, -1, *)
        if (wave > 0) {
            join(row - kTY, edges);                                                     // (-1, 0, *)
            if (edges && ly > 0) join(row - kTY - 1, corners);                          // (-1, -1, *)
            if (edges && ly < kTY - 1) join(row - kTY + 1, corners);                    // (-1, +1, *)
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

template <bool LAB> __global__ void __launch_bounds__(kBlock) conn_merge_kernel(ConnDev P) {
    const uint32_t i = (uint32_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= (uint32_t)P.N) return;
    const int v = conn_value<LAB>(P.vol[i], P);
    if (v == 0) return;
    const uint32_t Wu = (uint32_t)P.W, HWu = (uint32_t)P.H * Wu;
    const uint32_t zu = i / HWu, rem = i - zu * HWu, yu = rem / Wu;
    const int x = (int)(rem - yu * Wu), y = (int)yu, z = (int)zu;
    const int lx = x % kTX, ly = y % kTY;
    if (!(lx == 0 || lx == kTX - 1 || ly == 0 || ly == kTY - 1 || z % kTZ == 0)) return;       // every neighbour is in this tile
    const int64_t W = P.W, HW = (int64_t)P.H * P.W;
    // previous neighbour k = 9 (dz + 1) + 3 (dy + 1) + (dx + 1), k < 13 (13 is the voxel itself).  same: it is inside the volume, a
    // neighbour under c and has this voxel's value; far: it lies in another tile
    uint32_t same = 0, far = 0;
#pragma unroll
    for (int k = 0; k < 13; ++k) {
        const int dz = k / 9 - 1, dy = (k / 3) % 3 - 1, dx = k % 3 - 1;
        if ((dz != 0) + (dy != 0) + (dx != 0) > P.conn) continue;
        const int nx = x + dx, ny = y + dy, nz = z + dz;
        if (nx < 0 || nx >= P.W || ny < 0 || ny >= P.H || nz < 0) continue;                    // the sides of the volume
        if (conn_value<LAB>(P.vol[(int64_t)i + dz * HW + dy * W + dx], P) != v) continue;
        same |= 1u << k;
        if (nx / kTX != x / kTX || ny / kTY != y / kTY || nz / kTZ != z / kTZ) far |= 1u << k;
    }
    uint32_t need = same & far;
#pragma unroll
    for (int r = 0; r < 4; ++r)                                                                // rows (dz, dy) with a centre voxel
        if ((same >> (3 * r + 1)) & 1u) need &= ~(5u << (3 * r));
#pragma unroll
    for (int k = 0; k < 13; ++k) {
        const int dz = k / 9 - 1, dy = (k / 3) % 3 - 1, dx = k % 3 - 1;
        if ((need >> k) & 1u) lab_union<kScopeAgent>(P.lab, (int32_t)i, (int32_t)((int64_t)i + dz * HW + dy * W + dx));
    }
}

template <bool LAB>
static int conn_launch(const uint8_t* vol, int32_t* roots, void* workspace, int d, int h, int w, int bit, int invert, int conn, void* stream) {
    ConnDev P;
    memset(&P, 0, sizeof(P));
    P.vol = vol; P.lab = (int32_t*)workspace; P.roots = roots;
    P.D = d; P.H = h; P.W = w; P.N = (int32_t)((int64_t)d * h * w);
    P.bit = bit; P.invert = invert; P.conn = conn;
    P.tx = (w + kTX - 1) / kTX;
    P.ty = (h + kTY - 1) / kTY;
    const int64_t tiles = (int64_t)P.tx * P.ty * ((d + kTZ - 1) / kTZ);             // <= N: every tile holds a voxel
    hipStream_t st = (hipStream_t)stream;
    const dim3 flat((unsigned)(((int64_t)P.N + kBlock - 1) / kBlock)), block(kBlock);
    hipLaunchKernelGGL((conn_tile_kernel<LAB>), dim3((unsigned)tiles), block, 0, st, P);
    hipLaunchKernelGGL((conn_merge_kernel<LAB>), flat, block, 0, st, P);
    CclDev F;                                         // the binary entry's flatten launch as it is: it reads lab, roots and N
    memset(&F, 0, sizeof(F));
    F.lab = P.lab; F.roots = P.roots; F.N = P.N;
    hipLaunchKernelGGL(ccl_flatten_kernel, flat, block, 0, st, F);
    return (int)hipGetLastError();
}

}  // namespace segm

using namespace segm;

extern "C" int segm_ccl_roots_conn(const segm_ccl_roots_conn_args* a) {
    if (!a) return SEGM_E_NULL;
    if (!a->volume || !a->roots) return SEGM_E_NULL;
    if (a->connectivity < 1 || a->connectivity > 3) return SEGM_E_SHAPE;
    if (a->connectivity == 1) {                       // the launches of segm_ccl_roots, its refusals included
        segm_ccl_roots_args r;
        memset(&r, 0, sizeof(r));
        r.depth = a->depth; r.height = a->height; r.width = a->width; r.bit = a->bit; r.invert = a->invert;
        r.volume = a->volume; r.roots = a->roots; r.workspace = a->workspace; r.workspace_bytes = a->workspace_bytes; r.stream = a->stream;
        return segm_ccl_roots(&r);
    }
    if (!ccl_volume_ok(a->depth, a->height, a->width)) return SEGM_E_SHAPE;
    if (a->bit < -1 || a->bit > 7 || (a->invert != 0 && a->invert != 1)) return SEGM_E_SHAPE;
    if ((uintptr_t)a->roots % sizeof(int32_t)) return SEGM_E_SHAPE;
    const int64_t N = (int64_t)a->depth * a->height * a->width;
    if (!a->workspace || a->workspace_bytes < segm_ccl_roots_workspace_bytes(N) || (uintptr_t)a->workspace % sizeof(int32_t)) return SEGM_E_WORKSPACE;
    return conn_launch<false>(a->volume, a->roots, a->workspace, a->depth, a->height, a->width, a->bit, a->invert, a->connectivity, a->stream);
}

extern "C" int segm_ccl_label_roots_conn(const segm_ccl_label_roots_conn_args* a) {
    if (!a) return SEGM_E_NULL;
    if (!a->labels || !a->roots) return SEGM_E_NULL;
    if (a->connectivity < 1 || a->connectivity > 3) return SEGM_E_SHAPE;
    if (a->connectivity == 1) {                       // the launches of segm_ccl_label_roots, its refusals included
        segm_ccl_label_roots_args r;
        memset(&r, 0, sizeof(r));
        r.depth = a->depth; r.height = a->height; r.width = a->width;
        r.labels = a->labels; r.roots = a->roots; r.workspace = a->workspace; r.workspace_bytes = a->workspace_bytes; r.stream = a->stream;
        return segm_ccl_label_roots(&r);
    }
    if (!ccl_volume_ok(a->depth, a->height, a->width)) return SEGM_E_SHAPE;
    if ((uintptr_t)a->roots % sizeof(int32_t)) return SEGM_E_SHAPE;
    const int64_t N = (int64_t)a->depth * a->height * a->width;
    if (!a->workspace || a->workspace_bytes < segm_ccl_label_roots_workspace_bytes(N) || (uintptr_t)a->workspace % sizeof(int32_t)) return SEGM_E_WORKSPACE;
    return conn_launch<true>(a->labels, a->roots, a->workspace, a->depth, a->height, a->width, -1, 0, a->connectivity, a->stream);
}
