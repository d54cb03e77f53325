// TEST INFRASTRUCTURE: a stand-alone host program that runs segm_ccl_label_roots (csrc/ccl_roots.hip) and segm_ccl_label_select
// (csrc/ccl_labels.hip) on the CPU emulation of HIP with every buffer allocated at its exact size, to be built with AddressSanitizer
// + UBSan: an index past a buffer, a misaligned access or an overflow in the index arithmetic is reported.  No Python, no GPU.
//
//   CXX=/opt/rocm/lib/llvm/bin/clang++
//   F="-O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -std=c++17 -pthread -Itests/emu -Wno-unused-value -DSEGM_EMU=1"
//   $CXX $F '-DSEGM_PIN_F32(x)=' '-DSEGM_SCHED_FENCE()=' '-DSEGM_PIN_F2(x)=' '-DSEGM_WAVE_LDS_SYNC()=hipemu::sync_wave()' \
//        '-DSEGM_BLOCK_LDS_SYNC()=hipemu::sync_block()' \
//        -x c++ segmamba_amd/csrc/ccl_roots.hip segmamba_amd/csrc/ccl_labels.hip tests/emu/hip_emu_runtime.cpp tools/ccl_labels_sanitize.cpp \
//        -o build/ccl_labels_sanitize
//   ASAN_OPTIONS=detect_leaks=0:detect_stack_use_after_return=0 build/ccl_labels_sanitize
//
// Cases: random labels 0 .. 3 in runs of two along x on the 27 volumes whose sides are 1 below, at and 1 above the tile's
// (63 / 64 / 65 x 3 / 4 / 5 x 3 / 4 / 5), the stripes `1 + x % 3` on 5 x 6 x 70 and the two-label checkerboard on 4 x 6 x 66.  Every
// result is compared with a plain union-find and a plain selection: roots, the kept labels under LARGEST (all labels, and with label 2
// passed through by an apply table) and under MIN_SIZE 3, and all 256 x 3 entries of `info`.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../include/segmamba_hip.h"

static uint32_t rng_state = 24680u;
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

static int run_case(const char* name, int D, int H, int W, const std::vector<uint8_t>& lab) {
    const int N = D * H * W;
    // the restatement: union of equally labelled face neighbours, the smaller root wins
    std::vector<int> parent(N), want_roots(N), cnt(N, 0);
    for (int i = 0; i < N; ++i) parent[i] = i;
    for (int i = 0; i < N; ++i) {
        if (!lab[i]) continue;
        const int x = i % W, y = (i / W) % H, z = i / (W * H);
        const int nb[3] = {x > 0 ? i - 1 : -1, y > 0 ? i - W : -1, z > 0 ? i - W * H : -1};
        for (int j : nb)
            if (j >= 0 && lab[j] == lab[i]) {
                const int a = find(parent, i), b = find(parent, j);
                if (a != b) parent[a > b ? a : b] = a > b ? b : a;
            }
    }
    for (int i = 0; i < N; ++i) { want_roots[i] = lab[i] ? find(parent, i) : -1; if (lab[i]) ++cnt[want_roots[i]]; }
    long long want_info[256][3];
    for (int l = 0; l < 256; ++l) { want_info[l][0] = 0; want_info[l][1] = -1; want_info[l][2] = 0; }
    for (int i = 0; i < N; ++i)
        if (cnt[i] > 0) {
            long long* w = want_info[lab[i]];
            ++w[0];
            if (cnt[i] >= w[2]) { w[1] = i; w[2] = cnt[i]; }      // equal sizes: the later root
        }

    Exact<uint8_t> vol((size_t)N), out((size_t)N), apply(256);
    Exact<int32_t> roots((size_t)N), sizes((size_t)N);
    Exact<int64_t> info(256 * 3);
    memcpy(vol.p, lab.data(), (size_t)N);
    const size_t ws_roots = segm_ccl_label_roots_workspace_bytes(N), ws_sel = segm_ccl_label_select_workspace_bytes(N);
    Exact<uint8_t> w1(ws_roots), w2(ws_sel);
    int bad = 0;

    segm_ccl_label_roots_args r;
    memset(&r, 0, sizeof(r));
    r.depth = D; r.height = H; r.width = W;
    r.labels = vol.p; r.roots = roots.p; r.workspace = w1.p; r.workspace_bytes = ws_roots;
    int rc = segm_ccl_label_roots(&r);
    if (rc != 0) { printf("%s: segm_ccl_label_roots: status %d\n", name, rc); return 1; }
    for (int i = 0; i < N; ++i)
        if (roots.p[i] != want_roots[i]) { if (!bad) printf("%s: roots[%d] = %d, want %d\n", name, i, roots.p[i], want_roots[i]); ++bad; }
    for (int i = 0; i < N; ++i) sizes.p[i] = cnt[i];

    for (int pass = 0; pass < 3 && !bad; ++pass) {        // 0: LARGEST; 1: LARGEST, label 2 passes through; 2: MIN_SIZE 3
        memset(apply.p, 1, 256);
        if (pass == 1) apply.p[2] = 0;
        segm_ccl_label_select_args s;
        memset(&s, 0, sizeof(s));
        s.depth = D; s.height = H; s.width = W;
        s.mode = pass == 2 ? SEGM_CCL_MIN_SIZE : SEGM_CCL_LARGEST;
        s.min_size = 3;
        s.labels = vol.p; s.roots = roots.p; s.sizes = sizes.p; s.apply = pass == 1 ? apply.p : nullptr;
        s.out = out.p; s.info = info.p; s.workspace = w2.p; s.workspace_bytes = ws_sel;
        memset(out.p, 0x5a, (size_t)N);
        rc = segm_ccl_label_select(&s);
        if (rc != 0) { printf("%s: segm_ccl_label_select: status %d\n", name, rc); return 1; }
        for (int i = 0; i < N; ++i) {
            uint8_t want = 0;
            if (lab[i]) {
                const bool on = !apply.p[lab[i]] || (pass == 2 ? cnt[want_roots[i]] >= 3 : want_roots[i] == want_info[lab[i]][1]);
                want = on ? lab[i] : 0;
            }
            if (out.p[i] != want) { if (!bad) printf("%s pass %d: out[%d] = %d, want %d\n", name, pass, i, out.p[i], want); ++bad; }
        }
        for (int l = 0; l < 256; ++l)
            for (int k = 0; k < 3; ++k)
                if (info.p[3 * l + k] != want_info[l][k]) {
                    if (!bad) printf("%s pass %d: info[%d][%d] = %lld, want %lld\n", name, pass, l, k, (long long)info.p[3 * l + k], want_info[l][k]);
                    ++bad;
                }
    }
    int components = 0;
    for (int i = 0; i < N; ++i) components += cnt[i] > 0;
    printf("%-14s %d x %d x %d  %d components: %s\n", name, D, H, W, components, bad ? "FAILED" : "ok");
    return bad ? 1 : 0;
}

int main() {
    int failed = 0;
    const int ws[3] = {63, 64, 65}, hs[3] = {3, 4, 5};
    for (int W : ws) for (int H : hs) for (int D : hs) {
        std::vector<uint8_t> lab((size_t)D * H * W);
        for (int row = 0; row < D * H; ++row)
            for (int x = 0; x < W; x += 2) {
                const uint8_t v = (uint8_t)(rng() & 3);
                lab[(size_t)row * W + x] = v;
                if (x + 1 < W) lab[(size_t)row * W + x + 1] = v;
            }
        failed += run_case("tile edges", D, H, W, lab);
    }
    {
        const int D = 5, H = 6, W = 70;
        std::vector<uint8_t> lab((size_t)D * H * W);
        for (size_t i = 0; i < lab.size(); ++i) lab[i] = (uint8_t)(1 + (i % W) % 3);
        failed += run_case("stripes", D, H, W, lab);
    }
    {
        const int D = 4, H = 6, W = 66;
        std::vector<uint8_t> lab((size_t)D * H * W);
        for (int z = 0; z < D; ++z) for (int y = 0; y < H; ++y) for (int x = 0; x < W; ++x) lab[((size_t)z * H + y) * W + x] = (uint8_t)(1 + (z + y + x) % 2);
        failed += run_case("checkerboard", D, H, W, lab);
    }
    printf(failed ? "%d case(s) failed\n" : "all cases ran clean\n", failed);
    return failed ? 1 : 0;
}
