// TEST INFRASTRUCTURE: a stand-alone host program that runs segm_ccl_roots_conn and segm_ccl_label_roots_conn
// (csrc/ccl_roots.hip) on the CPU emulation of HIP with every buffer allocated at its exact size, to be built with AddressSanitizer +
// UBSan: a neighbour index past a buffer - x - 1 at x = 0 of the first row, x + 1 at the end of the last - a misaligned access or an
// overflow in the index arithmetic is reported.  No Python, no GPU.
//
//   CXX=/opt/rocm/lib/llvm/bin/clang++
//   F="-O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -std=c++17 -pthread -Itests/emu -Wno-unused-value -DSEGM_EMU=1"
//   $CXX $F '-DSEGM_PIN_F32(x)=' '-DSEGM_SCHED_FENCE()=' '-DSEGM_PIN_F2(x)=' '-DSEGM_WAVE_LDS_SYNC()=hipemu::sync_wave()' \
//        '-DSEGM_BLOCK_LDS_SYNC()=hipemu::sync_block()' \
//        -x c++ segmamba_amd/csrc/ccl_roots.hip tests/emu/hip_emu_runtime.cpp tools/ccl_conn_sanitize.cpp -o build/ccl_conn_sanitize
//   ASAN_OPTIONS=detect_leaks=0:detect_stack_use_after_return=0 build/ccl_conn_sanitize
//
// Cases, each at connectivity 1, 2 and 3: random masks of density 0.1, 0.3 and 0.6 on the 27 volumes whose sides are 1 below, at and
// 1 above the tile's (63 / 64 / 65 x 3 / 4 / 5 x 3 / 4 / 5), the hand case (6 x 6 x 70, six voxels: 5, 4, 3 components), the 3-D
// checkerboard and the body-centred lattice on 5 x 6 x 66.  The binary entry runs on the mask as it is (bit -1), on bit 5 of bytes
// whose other bits are noise, and inverted; the labelled entry on the mask times a random label 1 .. 3.  Every result is compared
// with a plain union-find over the explicit list of previous neighbours.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../include/segmamba_hip.h"

static uint32_t rng_state = 13579u;
static uint32_t rng() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }

// `count` elements at a 16-byte aligned address, not one byte more
template <typename T> struct Exact {
    T* p;
    size_t count;
    explicit Exact(size_t n) : p(nullptr), count(n) {
        void* q = nullptr;
        if (posix_memalign(&q, 16, n * sizeof(T)) != 0) abort();
        p = (T*)q;
        memset(p, 0x5a, n * sizeof(T));
    }
    ~Exact() { free(p); }
    Exact(const Exact&) = delete;
};

static int find(std::vector<int>& parent, int a) {
    while (parent[a] != a) a = parent[a] = parent[parent[a]];
    return a;
}

// the restatement: union of equally valued non-zero voxels over the previous neighbours with at most c non-zero coordinates
static std::vector<int> want_roots(int D, int H, int W, const std::vector<uint8_t>& val, int c) {
    const int N = D * H * W;
    std::vector<int> parent(N), out(N);
    for (int i = 0; i < N; ++i) parent[i] = i;
    for (int z = 0; z < D; ++z) for (int y = 0; y < H; ++y) for (int x = 0; x < W; ++x) {
        const int i = (z * H + y) * W + x;
        if (!val[i]) continue;
        for (int dz = -1; dz <= 0; ++dz) for (int dy = -1; dy <= 1; ++dy) for (int dx = -1; dx <= 1; ++dx) {
            if (!(dz < 0 || dy < 0 || (dy == 0 && dx < 0))) continue;          // not a previous neighbour
            if ((dz != 0) + (dy != 0) + (dx != 0) > c) continue;
            const int nz = z + dz, ny = y + dy, nx = x + dx;
            if (nz < 0 || ny < 0 || ny >= H || nx < 0 || nx >= W) continue;
            const int j = (nz * H + ny) * W + nx;
            if (val[j] != val[i]) continue;
            const int a = find(parent, i), b = find(parent, j);
            if (a != b) parent[a > b ? a : b] = a > b ? b : a;
        }
    }
    for (int i = 0; i < N; ++i) out[i] = val[i] ? find(parent, i) : -1;
    return out;
}

static int compare(const char* name, const char* what, int c, const int32_t* got, const std::vector<int>& want) {
    int bad = 0;
    for (size_t i = 0; i < want.size(); ++i)
        if (got[i] != want[i]) { if (!bad) printf("%s, %s, c = %d: roots[%zu] = %d, want %d\n", name, what, c, i, got[i], want[i]); ++bad; }
    return bad;
}

static int run_case(const char* name, int D, int H, int W, const std::vector<uint8_t>& mask) {
    const int N = D * H * W;
    std::vector<uint8_t> inverse(N), labels(N);
    Exact<uint8_t> vol((size_t)N), packed((size_t)N), lab((size_t)N);
    Exact<int32_t> roots((size_t)N);
    for (int i = 0; i < N; ++i) {
        inverse[i] = mask[i] ? 0 : 1;
        labels[i] = mask[i] ? (uint8_t)(1 + rng() % 3) : 0;
        vol.p[i] = mask[i];
        packed.p[i] = (uint8_t)((rng() & 0xdf) | (mask[i] << 5));
        lab.p[i] = labels[i];
    }
    const size_t ws_bytes = segm_ccl_roots_workspace_bytes(N);
    if (ws_bytes != segm_ccl_label_roots_workspace_bytes(N)) { printf("%s: workspace sizes differ\n", name); return 1; }
    Exact<uint8_t> ws(ws_bytes);
    int bad = 0, components[4] = {0, 0, 0, 0};
    for (int c = 1; c <= 3; ++c) {
        const std::vector<int> want = want_roots(D, H, W, mask, c), want_inv = want_roots(D, H, W, inverse, c),
                               want_lab = want_roots(D, H, W, labels, c);
        for (int i = 0; i < N; ++i) components[c] += want[i] == i;
        for (int pass = 0; pass < 3; ++pass) {            // 0: the mask, bit -1; 1: bit 5 among noise; 2: bit 5, inverted
            segm_ccl_roots_conn_args r;
            memset(&r, 0, sizeof(r));
            r.depth = D; r.height = H; r.width = W; r.connectivity = c;
            r.bit = pass ? 5 : -1; r.invert = pass == 2;
            r.volume = pass ? packed.p : vol.p; r.roots = roots.p; r.workspace = ws.p; r.workspace_bytes = ws_bytes;
            memset(roots.p, 0x5a, (size_t)N * sizeof(int32_t));
            const int rc = segm_ccl_roots_conn(&r);
            if (rc != 0) { printf("%s: segm_ccl_roots_conn: status %d\n", name, rc); return 1; }
            bad += compare(name, pass == 0 ? "mask" : pass == 1 ? "bit 5" : "bit 5 inverted", c, roots.p, pass == 2 ? want_inv : want);
        }
        segm_ccl_label_roots_conn_args l;
        memset(&l, 0, sizeof(l));
        l.depth = D; l.height = H; l.width = W; l.connectivity = c;
        l.labels = lab.p; l.roots = roots.p; l.workspace = ws.p; l.workspace_bytes = ws_bytes;
        memset(roots.p, 0x5a, (size_t)N * sizeof(int32_t));
        const int rc = segm_ccl_label_roots_conn(&l);
        if (rc != 0) { printf("%s: segm_ccl_label_roots_conn: status %d\n", name, rc); return 1; }
        bad += compare(name, "labels", c, roots.p, want_lab);
    }
    printf("%-14s %d x %d x %d  components %d / %d / %d: %s\n", name, D, H, W, components[1], components[2], components[3], bad ? "FAILED" : "ok");
    return bad ? 1 : 0;
}

int main() {
    int failed = 0;
    const int ws[3] = {63, 64, 65}, hs[3] = {3, 4, 5}, tenths[3] = {1, 3, 6};
    for (int W : ws) for (int H : hs) for (int D : hs) for (int d : tenths) {
        std::vector<uint8_t> m((size_t)D * H * W);
        for (size_t i = 0; i < m.size(); ++i) m[i] = (uint8_t)(rng() % 10 < (uint32_t)d);
        char name[32];
        snprintf(name, sizeof(name), "tile edges .%d", d);
        failed += run_case(name, D, H, W, m);
    }
    {
        const int D = 6, H = 6, W = 70, pts[6][3] = {{3, 3, 63}, {4, 4, 64}, {1, 3, 10}, {1, 4, 11}, {3, 1, 20}, {4, 1, 20}};
        std::vector<uint8_t> m((size_t)D * H * W, 0);
        for (const auto& p : pts) m[((size_t)p[0] * H + p[1]) * W + p[2]] = 1;
        failed += run_case("hand", D, H, W, m);
    }
    for (int lattice = 0; lattice < 2; ++lattice) {
        const int D = 5, H = 6, W = 66;
        std::vector<uint8_t> m((size_t)D * H * W);
        for (int z = 0; z < D; ++z) for (int y = 0; y < H; ++y) for (int x = 0; x < W; ++x)
            m[((size_t)z * H + y) * W + x] = lattice == 0 ? (uint8_t)((z + y + x) % 2 == 0)
                                                          : (uint8_t)((z % 2 == y % 2 && y % 2 == x % 2));
        failed += run_case(lattice == 0 ? "checkerboard" : "body-centred", D, H, W, m);
    }
    printf(failed ? "%d case(s) failed\n" : "all cases ran clean\n", failed);
    return failed ? 1 : 0;
}
