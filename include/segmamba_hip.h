/*
 * segmamba_hip.h - C ABI of libsegmamba_hip.so: the MI355X (gfx950) kernels of SegMamba's hot path.
 *
 * Every entry point replaces one native binding of the reference (ge-xing/SegMamba); the reference
 * line it replaces is cited next to it.  Plain pointers, sizes and strides only - no torch types.
 *
 *   - all tensors are caller-allocated DEVICE memory; the library never allocates, frees or retains
 *     a pointer (SURVEY.md §8b "Ownership");
 *   - every call is asynchronous on `stream` (a hipStream_t; NULL = the null stream) and may be issued
 *     concurrently from several host threads / processes;
 *   - return value: 0 on success, <0 = SEGM_E_* argument error (nothing was launched),
 *     >0 = the hipError_t reported by a launch.
 *
 * Layout.  Sequence tensors are described by explicit element strides for the logical index
 * (batch, time, channel), so both the reference's channel-first (B, D, L) tensors
 * (stride_t == 1) and the channel-last (B, L, D) tensors the kernels are tuned for
 * (stride_d == 1: one lane per channel, coalesced 64-channel rows) are accepted as they are.
 * Views into larger buffers (e.g. the x / z halves of `xz`, or dx / dz halves of `dxz`,
 * reference selective_scan_interface.py:175,244-245) are expressed through the strides.
 *
 * Time order.  The tri-directional Mamba block (reference mamba_simple.py:215-264) runs the same
 * operator on the sequence as stored, reversed (`xz.flip(-1)`, :231) and slice-interleaved
 * (`stack(chunk(nslices))`, :245-247).  Instead of materialising those copies, every operator takes
 * `time_order`: logical step tau is read from / written to physical index
 *      FORWARD      t = tau
 *      REVERSED     t = L-1-tau
 *      INTERLEAVED  t = (tau % nslices) * (L / nslices) + tau / nslices      (needs L % nslices == 0)
 * so outputs land where the reference's `.flip(-1)` / inverse permutation (:261,264) would put them.
 */
#ifndef SEGMAMBA_HIP_H
#define SEGMAMBA_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SEGM_ABI_VERSION 10

enum segm_dtype { SEGM_F32 = 0, SEGM_F16 = 1, SEGM_BF16 = 2 };
enum segm_time_order { SEGM_TIME_FORWARD = 0, SEGM_TIME_REVERSED = 1, SEGM_TIME_INTERLEAVED = 2 };

enum segm_status {
    SEGM_OK = 0,
    SEGM_E_NULL = -1,        /* a required pointer is NULL                                            */
    SEGM_E_SHAPE = -2,       /* non-positive size, dim % n_groups != 0, L % nslices != 0, ...        */
    SEGM_E_DSTATE = -3,      /* dstate outside [1, 16] for the scan (reference limit is 256,
                                selective_scan.cpp:247; SegMamba uses 16), [1, 256] for the decode step   */
    SEGM_E_DTYPE = -4,       /* unknown dtype code                                                    */
    SEGM_E_WIDTH = -5,       /* conv width outside [2, 4]  (reference causal_conv1d.cpp:157)          */
    SEGM_E_WORKSPACE = -6,   /* workspace pointer NULL or too small                                   */
    SEGM_E_TIME_ORDER = -7   /* unknown time order                                                    */
};

/* logical (batch, time, channel) view; strides in ELEMENTS */
typedef struct segm_seq {
    void* ptr;
    int64_t stride_b, stride_t, stride_d;
} segm_seq;

/* logical (batch, group, time, state) view of the input-dependent B / C matrices; strides in ELEMENTS */
typedef struct segm_bc {
    void* ptr;
    int64_t stride_b, stride_g, stride_t, stride_n;
} segm_bc;

/* ------------------------------------------------------------------------------------------------
 * Selective scan, forward.
 * Replaces  selective_scan_cuda.fwd(u, delta, A, B, C, D?, z?, delta_bias?, delta_softplus)
 *           -> [out, x, (out_z)]      reference mamba/csrc/selective_scan/selective_scan.cpp:226-336
 *           (kernel selective_scan_fwd_kernel.cuh:67-303).
 *
 *   h_t = exp(delta_t * A) . h_{t-1} + delta_t * u_t * B_t ,  y_t = <C_t, h_t> + D * u_t ,
 *   out = y ,  out_z = y * silu(z) ,  delta = softplus(delta + delta_bias) if delta_softplus.
 *
 * Real A, input-dependent B and C (the only variant on the SegMamba path).
 * Instead of the reference's opaque `x` (per-2048-chunk scan state, selective_scan.cpp:304-313) the
 * state needed by the backward is an opaque checkpoint buffer `ckpt` of
 * segm_selective_scan_ckpt_bytes(); the reference's only other use of `x`
 * (`last_state = x[:, :, -1, 1::2]`, selective_scan_interface.py:40) is the explicit `last_state`.
 * ------------------------------------------------------------------------------------------------ */
typedef struct segm_scan_fwd_args {
    int32_t batch, dim, dstate, n_groups;
    int64_t seqlen;
    int32_t dtype;            /* segm_dtype of u, delta, z, B, C, out, out_z                         */
    int32_t delta_softplus;
    int32_t time_order;       /* segm_time_order                                                     */
    int32_t nslices;          /* INTERLEAVED only                                                    */
    int32_t chunk;            /* steps per work item; 0 = choose. Must match between fwd and bwd     */
    int32_t reserved;
    segm_seq u, delta;        /* required                                                            */
    segm_seq z;               /* ptr NULL = no gate                                                  */
    segm_seq out;             /* ptr NULL = do not store the un-gated y                              */
    segm_seq out_z;           /* required iff z.ptr                                                  */
    segm_bc B, C;             /* required                                                            */
    const float* A;           /* (dim, dstate) contiguous, fp32                                      */
    const float* D;           /* (dim) fp32 or NULL                                                  */
    const float* delta_bias;  /* (dim) fp32 or NULL                                                  */
    float* last_state;        /* (batch, dim, dstate) contiguous fp32 or NULL                        */
    float* ckpt;              /* segm_selective_scan_ckpt_bytes() or NULL (inference)                */
    void* workspace;          /* segm_selective_scan_fwd_workspace_bytes()                           */
    size_t workspace_bytes;
    void* stream;
    /* Optional (ABI 4): the causal depthwise conv1d + SiLU in front of the scan computed INSIDE the scan launches ("causal
     * depthwise conv1d fused into the same launch").  conv_width 0 = off.  With conv_width in [2, 4], `u` is the conv INPUT x and
     * every pass forms u_t = SiLU(conv_bias + sum_k conv_weight[d][k] x[t - (width-1-k)]) along this call's time order, rounded to
     * the element type exactly as segm_causal_conv1d_fwd stores it (results are bit-identical to conv1d followed by the scan).
     * Regular shapes with delta_softplus and a gate z only (SEGM_E_SHAPE otherwise).  Measured slower than the separate conv1d
     * launch on MI355X (the scan passes are bound by instructions issued): opt-in, see DESIGN.md section 0 row N1. */
    const float* conv_weight; /* (dim, conv_width) contiguous fp32                                  */
    const float* conv_bias;   /* (dim) fp32 or NULL                                                  */
    int32_t conv_width, reserved2;
    /* Optional (ABI 6): delta = dt_proj(x_dbl[:, :dt_rank]) formed INSIDE the forward passes (reference
     * selective_scan_interface.py:181-182 computes it with a GEMM launch and stores it).  dt_rank 0 = off.  With dt_rank in
     * [1, 8]: `dt_x` points at the dt columns of x_dbl (element type `dtype`, dt_rank consecutive columns per time row, strides in
     * elements), `dt_weight` is the (dim, dt_rank) projection weight as fp32, and `delta` becomes an OUTPUT: both passes form
     * delta_t = sum_r dt_weight[d][r] dt_x[t][r], rounded to `dtype` as the stored tensor is, and the apply pass writes it for the
     * backward.  Regular shapes with one B / C group only (SEGM_E_SHAPE otherwise).  Opt-in: see DESIGN.md section 0 row N1. */
    const void* dt_x;
    int64_t dt_stride_b, dt_stride_t;
    const float* dt_weight;
    int32_t dt_rank, reserved3;
} segm_scan_fwd_args;

int segm_selective_scan_fwd(const segm_scan_fwd_args* args);
/* `n` forward scans in one call: the three directions of a Mamba(bimamba_type="v3") layer (reference
 * mamba_simple.py:216-264 issues three selective_scan_cuda.fwd calls per layer, one per parameter set).  When the blocks share
 * batch / dim / dstate / seqlen / dtype / chunk / stream, have one B / C group and a regular shape, they run as ONE grid with a
 * direction axis (3 x the waves: the small stages of SegMamba cannot fill 1024 SIMDs with one direction); otherwise one after
 * the other, exactly as n calls of segm_selective_scan_fwd.  Every block owns its workspace / outputs. */
int segm_selective_scan_fwd_multi(const segm_scan_fwd_args* args, int32_t n);
size_t segm_selective_scan_fwd_workspace_bytes(int32_t batch, int32_t dim, int32_t dstate, int64_t seqlen,
                                               int32_t chunk);
size_t segm_selective_scan_ckpt_bytes(int32_t batch, int32_t dim, int32_t dstate, int64_t seqlen);
/* the chunk length `chunk = 0` resolves to (so callers can record it for the backward) */
int32_t segm_selective_scan_default_chunk(int32_t batch, int32_t dim, int64_t seqlen);
/* 1 when a scan of this geometry runs on the regular-shape kernels (dstate 16, channel count a multiple of 16 / 32 / 64, whole
 * chunks, a time order that is affine inside 8-step sub-tiles): the condition of segm_selective_scan_{fwd,bwd}_multi sharing one
 * grid and of the conv_weight option.  One B / C group is assumed; chunk 0 = the default chunk. */
int32_t segm_selective_scan_regular_shape(int32_t batch, int32_t dim, int32_t dstate, int64_t seqlen, int32_t chunk,
                                          int32_t time_order, int32_t nslices);

/* ------------------------------------------------------------------------------------------------
 * Selective scan, backward.
 * Replaces  selective_scan_cuda.bwd(u, delta, A, B, C, D?, z?, delta_bias?, dout, x?, out?, dz?,
 *                                   delta_softplus, recompute_out_z)
 *           -> [du, ddelta, dA, dB, dC, dD, ddelta_bias, (dz), (out_z)]
 *           reference selective_scan.cpp:338-492 (kernel selective_scan_bwd_kernel.cuh:75-489).
 *
 * du / ddelta / dz may alias slices of a larger buffer (dx / dz halves of dxz).  dA, dD,
 * ddelta_bias, dB, dC are fp32 and are OVERWRITTEN (the reference zero-fills then accumulates,
 * selective_scan.cpp:460-466; here the library clears what it accumulates into).
 * `out` (the un-gated y written by the forward) is required iff z.ptr; `ckpt` is the forward's.
 * ------------------------------------------------------------------------------------------------ */
typedef struct segm_scan_bwd_args {
    segm_scan_fwd_args f;     /* same meaning as in the forward; f.out = saved y (read), f.out_z ignored,
                                 f.last_state ignored, f.workspace ignored                             */
    segm_seq dout;            /* required; gradient w.r.t. out_z (or out when no z)                    */
    segm_seq du, ddelta;      /* required                                                             */
    segm_seq dz;              /* required iff f.z.ptr                                                  */
    segm_bc dB, dC;           /* logical (batch, group, time, state); fp32 unless dbc_native           */
    float* dA;                /* (dim, dstate) fp32                                                    */
    float* dD;                /* (dim) fp32 or NULL                                                    */
    float* ddelta_bias;       /* (dim) fp32 or NULL                                                    */
    void* workspace;          /* segm_selective_scan_bwd_workspace_bytes()                             */
    size_t workspace_bytes;
    int32_t dbc_native;       /* ABI 5.  0: dB / dC are fp32 (the reference's accumulation buffers,
                                 selective_scan.cpp:461-462).  1: dB / dC have f.dtype - what the reference
                                 returns after its final cast (:488) - and are written once, finished, e.g.
                                 straight into columns of the x_proj gradient operand.  Only the
                                 deterministic kernel does this (segm_selective_scan_bwd_deterministic()
                                 tells whether a launch takes it); SEGM_E_SHAPE otherwise             */
    int32_t reserved_b;
} segm_scan_bwd_args;

int segm_selective_scan_bwd(const segm_scan_bwd_args* args);
int segm_selective_scan_bwd_multi(const segm_scan_bwd_args* args, int32_t n);   /* see segm_selective_scan_fwd_multi */
size_t segm_selective_scan_bwd_workspace_bytes(int32_t batch, int32_t dim, int32_t dstate, int64_t seqlen,
                                               int32_t chunk);
/* 1 when segm_selective_scan_bwd(args) runs the kernels whose dB / dC are sums in a fixed order (per-d-tile fp32 slabs added in
 * tile order: no atomics, no zero-initialised buffer, dbc_native allowed), 0 when it takes the kernels that accumulate dB / dC
 * atomically over d-tiles - irregular shapes (dim not a multiple of 16, dstate != 16, ...) and views whose rows span more than
 * 4 GiB per batch element; those results are NOT bit-reproducible run to run (float atomics).  The answer is formed from the
 * forward tensors of args->f (shape, layout and the 32-bit span bound) - the same predicate the launch applies to all tensors: a
 * gradient tensor that breaks the span bound sends a dbc_native = 0 launch to the general kernels and makes a dbc_native = 1
 * launch return SEGM_E_SHAPE.  No launch, no side effect. */
int segm_selective_scan_bwd_deterministic(const segm_scan_bwd_args* args);

/* ------------------------------------------------------------------------------------------------
 * Causal depthwise conv1d (+ optional SiLU), forward / backward.
 * Replaces  causal_conv1d_cuda.causal_conv1d_fwd(x, weight, bias?, silu) -> out
 *           reference causal-conv1d/csrc/causal_conv1d.cpp:130-189 (kernel causal_conv1d_fwd.cu:39-130)
 *      and  causal_conv1d_cuda.causal_conv1d_bwd(x, weight, bias?, dout, dx?, silu)
 *           -> [dx, dweight, dbias]   reference causal_conv1d.cpp:191-268 (kernel causal_conv1d_bwd.cu:46-240).
 *
 *   o_t = bias + sum_w weight[d, w] * x_{t-(width-1-w)}   (zero left pad),  out = o * sigmoid(o) if silu.
 *
 * weight (dim, width) and bias (dim) are fp32 contiguous (the reference also accepts 16-bit
 * weights; cast on the host).  dweight / dbias are fp32 and OVERWRITTEN.
 * ------------------------------------------------------------------------------------------------ */
typedef struct segm_conv1d_args {
    int32_t batch, dim, width, silu;
    int64_t seqlen;
    int32_t dtype;            /* of x, out, dout, dx */
    int32_t time_order, nslices;
    int32_t reserved;
    segm_seq x;               /* required */
    segm_seq out;             /* forward: required.  backward: ignored */
    const float* weight;      /* required */
    const float* bias;        /* or NULL  */
    /* backward only */
    segm_seq dout, dx;
    float* dweight;           /* (dim, width) */
    float* dbias;             /* (dim) or NULL */
    void* workspace;          /* backward: segm_causal_conv1d_bwd_workspace_bytes() */
    size_t workspace_bytes;
    void* stream;
} segm_conv1d_args;

int segm_causal_conv1d_fwd(const segm_conv1d_args* args);
int segm_causal_conv1d_bwd(const segm_conv1d_args* args);
/* `n` launches in one call; consecutive blocks that share batch / dim / width / seqlen / dtype / stream (up to three: the three
 * directions of a Mamba v3 layer, reference mamba_simple.py:216-264) run as one grid with a direction axis */
int segm_causal_conv1d_fwd_multi(const segm_conv1d_args* args, int32_t n);
int segm_causal_conv1d_bwd_multi(const segm_conv1d_args* args, int32_t n);
size_t segm_causal_conv1d_bwd_workspace_bytes(int32_t batch, int32_t dim, int32_t width, int64_t seqlen);

/* ------------------------------------------------------------------------------------------------
 * Weight gradient of a 3x3x3 stride-1 pad-1 convolution (the stem / decoder convolutions of SegMamba).
 * The reference gets this from cuDNN through torch.nn.Conv3d (monai/networks/blocks/convolutions.py:143-151,
 * model_segmamba/segmamba.py:95-99); on MI355X MIOpen's im2col solver for the 48-channel 128^3 layers is the single
 * largest item of a training step, so this one operator has a hand-written MFMA kernel.
 *
 *   dW[co, ci, kz, ky, kx] = sum_{b,z,y,x} dY[b, co, z, y, x] * X[b, ci, z+kz-1, y+ky-1, x+kx-1]
 *
 * x, dy: bf16 or fp16, logical (batch, channel, depth, height, width), W contiguous, every other stride a multiple of 8
 * elements, 16-byte aligned bases (channel slices of NCDHW tensors qualify).  cout a multiple of 48, cin a multiple of
 * 48 or below 48 (a narrow first layer), width a multiple of 8.  dw: contiguous (cout, cin, 3, 3, 3), fp32 or bf16, OVERWRITTEN.
 * ------------------------------------------------------------------------------------------------ */
typedef struct segm_conv3d_wgrad_args {
    int32_t batch, cin, cout, depth, height, width;
    int32_t dtype;            /* of x and dy: SEGM_BF16 or SEGM_F16      */
    int32_t dw_dtype;         /* SEGM_BF16, SEGM_F16 or SEGM_F32         */
    const void* x;   int64_t x_stride_b, x_stride_c, x_stride_z, x_stride_y;
    const void* dy;  int64_t dy_stride_b, dy_stride_c, dy_stride_z, dy_stride_y;
    void* dw;
    void* workspace;          /* segm_conv3d_k3_wgrad_workspace_bytes() */
    size_t workspace_bytes;
    void* stream;
} segm_conv3d_wgrad_args;

int segm_conv3d_k3_wgrad(const segm_conv3d_wgrad_args* args);
size_t segm_conv3d_k3_wgrad_workspace_bytes(int32_t batch, int32_t cin, int32_t cout, int32_t depth, int32_t height,
                                            int32_t width);

/* ------------------------------------------------------------------------------------------------
 * 3x3x3 stride-1 pad-1 convolution, forward (and data gradient, given flipped / transposed weights).
 * Replaces torch.nn.Conv3d -> cuDNN for the 48-input-channel 3x3x3 layers (reference model_segmamba/segmamba.py:95-131,
 * monai/networks/blocks/dynunet_block.py:44-111; the data gradient is what autograd asks cuDNN for in their backward).
 *
 *   y[b, co, z, y, x] = bias[co] + sum_{ci, kz, ky, kx} w[co, ci, kz, ky, kx] * x[b, ci, z+kz-1, y+ky-1, x+kx-1]
 *
 * x, y, w_packed: bf16 or fp16 (one dtype).  x (batch, cin, depth, height, width); y (batch, cout, depth, height,
 * width); W contiguous, every other stride a
 * multiple of 8 elements, 16-byte aligned bases.  1 <= cin <= 48 (wider layers are sums over 48-channel blocks), cout a
 * multiple of 16, width a multiple of 8.
 * w_packed: (cout, 3, 3, 3, 48) contiguous, i.e. weight.permute(0, 2, 3, 4, 1) - the input channel fastest - zero
 * padded to 48 input channels.
 * bias: (cout) fp32 or NULL.
 * flags: SEGM_CONV_FWD_ACCUMULATE adds the result to what `y` already holds (the 48-channel blocks of a wider layer
 * accumulate in place); SEGM_CONV_FWD_CHAIN (cout % 48 == 0 only) selects the kernel whose K parts are pipelined
 * through LDS instead of reduced at every output row - same results up to the order of fp32 additions;
 * SEGM_CONV_FWD_PITCH48 (with CHAIN only) lays its LDS rows out without padding (a bank-conflict experiment);
 * SEGM_CONV_FWD_CHAIN32 (alone or with ACCUMULATE) is the chained kernel on 32-wide x blocks, two workgroups per CU.
 * ------------------------------------------------------------------------------------------------ */
enum segm_conv_fwd_flags { SEGM_CONV_FWD_ACCUMULATE = 1, SEGM_CONV_FWD_CHAIN = 2, SEGM_CONV_FWD_PITCH48 = 4,
                           SEGM_CONV_FWD_CHAIN32 = 8 };

typedef struct segm_conv3d_fwd_args {
    int32_t batch, cin, cout, depth, height, width;
    int32_t dtype, flags;
    const void* x;   int64_t x_stride_b, x_stride_c, x_stride_z, x_stride_y;
    void* y;         int64_t y_stride_b, y_stride_c, y_stride_z, y_stride_y;
    const void* w_packed;
    const float* bias;
    void* stream;
    /* ABI 8: statistics of the result for the InstanceNorm behind the convolution (reference dynunet_block.py:98-111: every 3x3x3
     * convolution of the stem / decoder is followed by one).  stats_partials (NULL = off): fp32 (batch, cout, stats_nparts, 4) that
     * receives {count, sum y, sum y^2, 0} of the values this launch stores (the fp32 sums before rounding; with
     * SEGM_CONV_FWD_ACCUMULATE: of the accumulated values), one partial per (depth, y part, x block [, x pair]) - hand it to
     * segm_instnorm_fwd's stats_partials.  stats_nparts must equal segm_conv3d_k3_fwd_stats_parts(); only the launches with
     * SEGM_CONV_FWD_CHAIN | SEGM_CONV_FWD_PITCH48 or SEGM_CONV_FWD_CHAIN32 have the epilogue (SEGM_E_SHAPE otherwise). */
    float* stats_partials;
    int32_t stats_nparts, reserved;
} segm_conv3d_fwd_args;

int segm_conv3d_k3_fwd(const segm_conv3d_fwd_args* args);
int32_t segm_conv3d_k3_fwd_stats_parts(int32_t depth, int32_t height, int32_t width, int32_t batch, int32_t cout, int32_t flags);

/* ------------------------------------------------------------------------------------------------
 * ABI 9 (round 6): the same convolution on CHANNEL-LAST volumes, 48 -> 48 channels (csrc/conv3d_cl.hip).
 * Replaces the same reference calls as segm_conv3d_k3_fwd (model_segmamba/segmamba.py:91-132,
 * monai/networks/blocks/dynunet_block.py:44-111) for activations stored (batch, depth, height, width, channel):
 *
 *   y[b, z, y, x, co] = bias[co] + sum_{ci, kz, ky, kx} w[co, ci, kz, ky, kx] * x[b, z+kz-1, y+ky-1, x+kx-1, ci]
 *
 * x, y: bf16 or fp16 (one dtype), channels contiguous, every other stride a multiple of 8 elements and >= 48, 16-byte aligned
 * bases, width a multiple of 16, channels == 48 (wider layers: sums over 48-channel blocks with SEGM_CONV_CL_ACCUMULATE).
 * w_image: the weights as MFMA operand fragments, (14, 9, 64, 8) elements of the activations' dtype: element i is
 * w.flatten()[index[i]] (0 where index[i] < 0) with index from segm_conv3d_k3_cl_pack_index (host function, no GPU work).
 * The data gradient is the same call on dy with the image of flip(w, (2, 3, 4)).transpose(0, 1).
 * bias: (48) fp32 or NULL.  flags: SEGM_CONV_CL_ACCUMULATE adds to what y holds; SEGM_CONV_CL_WAVES8 runs eight waves of two
 * voxel tiles per workgroup instead of four waves of four (a scheduling choice, same results).
 * ------------------------------------------------------------------------------------------------ */
enum segm_conv_cl_flags { SEGM_CONV_CL_ACCUMULATE = 1, SEGM_CONV_CL_WAVES8 = 2 };

typedef struct segm_conv3d_cl_args {
    int32_t batch, channels, depth, height, width;
    int32_t dtype, flags, reserved;
    const void* x;   int64_t x_stride_b, x_stride_z, x_stride_y, x_stride_x;
    void* y;         int64_t y_stride_b, y_stride_z, y_stride_y, y_stride_x;
    const void* w_image;
    const float* bias;
    void* stream;
} segm_conv3d_cl_args;

int segm_conv3d_k3_fwd_cl(const segm_conv3d_cl_args* args);
int segm_conv3d_k3_cl_pack_index(int32_t* out, int64_t n);

/* ------------------------------------------------------------------------------------------------
 * ABI 10: 3x3x3 stride-1 pad-1 convolution of WIDE layers on SMALL volumes (csrc/conv3d_cube.hip): NCDHW, cin % 32 == 0,
 * cout a multiple of 64 or 96, depth / height / width multiples of 8 - the 16^3 / 8^3 levels of SegMamba's encoder and decoder (192 ... 768
 * channels; reference model_segmamba/segmamba.py:91-132, monai/networks/blocks/dynunet_block.py:44-111, unetr_block.py:82-84;
 * torch.nn.Conv3d -> cuDNN there).  A workgroup owns 8 x 8 x 8 voxels x 64 / 96 / 128 output channels, stages the halo cube of
 * 32 input channels per round in LDS and runs all 27 taps from it; the contraction is split over workgroups and a second launch
 * adds the fp32 partial sums in a fixed order (+ bias, + the existing y with SEGM_CONV_CUBE_ACCUMULATE) and rounds once; with one
 * split (enough cubes to fill the device) the first launch finishes the values itself.
 *
 * x: (batch, cin, D, H, W), y: (batch, cout, D, H, W), element strides for b / c / z / y (x contiguous), every stride a multiple
 * of 8, 16-byte aligned bases.  w_image: cout * cin * 27 elements of x's dtype arranged by segm_conv3d_k3_cube_pack_index:
 * out[i] = flat index into the (cout_w, cin_w, 3, 3, 3) weight; flipped = 1 gives the image of the DATA GRADIENT (a convolution
 * of dy with cout = cin_w, cin = cout_w and mirrored taps) - the same launch computes it.
 * segm_conv3d_k3_cube_plan: the column tiles per wave (nt: 2 / 3 / 4 = 64 / 96 / 128 channels per workgroup) and the number of
 * splits the launch will use (values > 0 on entry are kept when valid), and the fp32 elements the workspace must hold.
 * ------------------------------------------------------------------------------------------------ */
enum segm_conv_cube_flags { SEGM_CONV_CUBE_ACCUMULATE = 1 };

typedef struct segm_conv3d_cube_args {
    int32_t batch, cin, cout, depth, height, width;
    int32_t dtype, flags;
    int32_t nt, splits;       /* 0 = the plan's choice */
    const void* x;   int64_t x_stride_b, x_stride_c, x_stride_z, x_stride_y;
    void* y;         int64_t y_stride_b, y_stride_c, y_stride_z, y_stride_y;
    const void* w_image;
    const float* bias;        /* (cout) fp32 or NULL */
    void* workspace;          /* fp32, segm_conv3d_k3_cube_plan's workspace_elems (0 with one split: may be NULL) */
    int64_t workspace_elems;
    void* stream;
    /* InstanceNorm partials of what the launch stores (segm_instnorm_fwd_args.stats_partials): fp32 (batch * cout, stats_nparts, 4)
     * {count, sum, sum of squares, -}, stats_nparts = segm_conv3d_k3_cube_stats_parts(depth, height, width, the plan's splits);
     * NULL = not wanted */
    float* stats_partials;
    int32_t stats_nparts, reserved;
} segm_conv3d_cube_args;

int segm_conv3d_k3_cube_fwd(const segm_conv3d_cube_args* args);
int segm_conv3d_k3_cube_plan(int32_t batch, int32_t cin, int32_t cout, int32_t depth, int32_t height, int32_t width,
                             int32_t* nt, int32_t* splits, int64_t* workspace_elems);
int segm_conv3d_k3_cube_pack_index(int32_t* out, int64_t n, int32_t cout_w, int32_t cin_w, int32_t flipped);
int32_t segm_conv3d_k3_cube_stats_parts(int32_t depth, int32_t height, int32_t width, int32_t splits);

/* The images of many weights in ONE launch (what a training step needs after every weight update): descriptor i says where the
 * (cout_w, cin_w, 3, 3, 3) weight starts in `src` (element offset; co_stride = elements between its output channels - a channel
 * slice of a wider weight keeps the wide stride; the (cin, 27) part contiguous), where its image starts in `out` (a multiple of
 * 8), whether it is the data-gradient image, and the first block of the grid that works on it; blocks per image =
 * (Cout / 16) * (Cin / 32) of the convolution the image is for.  descs is a DEVICE array, first_block ascending.  The result is
 * element for element what segm_conv3d_k3_cube_pack_index describes. */
typedef struct segm_cube_pack_desc {
    int64_t src_off, out_off;
    int32_t cout_w, cin_w, co_stride, flipped;
    int32_t first_block, reserved;
} segm_cube_pack_desc;

int segm_conv3d_k3_cube_pack_multi(const void* src, void* out, const segm_cube_pack_desc* descs, int32_t ndesc, int32_t nblocks,
                                   void* stream);

/* The weight gradient of those layers (segm_conv3d_wgrad_args as for segm_conv3d_k3_wgrad): cin % 32 == 0, cout % 64 == 0, depth /
 * height / width multiples of 8.  The contraction runs over voxels and NCDHW has x contiguous: both operands are staged in LDS in
 * their native row layout (dY cube and X halo cube of 64 x 32 channels), a wave owns a 16 x 16 (co, ci) tile for all 27 taps, the
 * kx = 0 / 2 operands are register shifts; cube ranges are split over workgroups and a second launch adds the partial sums in a
 * fixed order.  Replaces what autograd asks cuDNN for in the backward of those Conv3d layers. */
int segm_conv3d_k3_cube_wgrad(const segm_conv3d_wgrad_args* args);
size_t segm_conv3d_k3_cube_wgrad_workspace_bytes(int32_t batch, int32_t cin, int32_t cout, int32_t depth, int32_t height,
                                                 int32_t width);

/* ------------------------------------------------------------------------------------------------
 * InstanceNorm3d (+ residual) (+ activation), forward and backward.
 * Replaces the torch.nn.InstanceNorm3d -> [+ residual] -> ReLU / LeakyReLU chains of the stem and decoder
 * (reference model_segmamba/segmamba.py:96-130,147,169-187; monai/networks/blocks/dynunet_block.py:98-111), which the
 * reference runs as three to four separate ATen kernels per call: no affine parameters, no running statistics,
 * biased variance, y = act((x - mean) / sqrt(var + eps) + residual).
 *
 * x, residual, y, dy, dx, dresidual: (instances, spatial) contiguous, instances = batch * channels, one dtype.
 * mean, rstd: (instances) fp32, written by the forward and read by the backward.
 * act: 0 none, 1 ReLU, 2 LeakyReLU(slope).
 * Backward: `y` (the forward's output) is required iff act != 0 and a residual was added (the activation mask is then
 * not recomputable from x); pass NULL otherwise.  dresidual (NULL = not wanted) receives dy * act'(.).
 * Two stated deviations (held per element against a float64 restatement by tests/norm_ref.py, tests/norm_checks.py):
 *  - when dresidual is wanted, the type has 16 bits and act is LeakyReLU, g = dy * act'(.) is parked in dresidual ROUNDED to the
 *    type by the statistics pass and dx is formed from that rounded value: dx is rounded twice, rstd * ulp(g) / 2 on top of its own
 *    final rounding (it saves one read of y and of dy).  fp32, ReLU and calls without dresidual are not affected.
 *  - the statistics are fp32 sums of x and x^2: their error grows with the condition number 1 + r^2 of E[x^2] - mean^2,
 *    r = |mean| / std:  |mean' - mean| rstd <= 2^-16 (1 + r),  |rstd' / rstd - 1| <= 2^-15 (1 + r^2)  (3e-4 at r = 3, 2.7e-2 at r = 30).
 * ------------------------------------------------------------------------------------------------ */
typedef struct segm_instnorm_fwd_args {
    int32_t instances, dtype, act, reserved;
    int64_t spatial;
    float slope, eps;
    const void* x;
    const void* residual;     /* or NULL */
    void* y;
    float* mean;
    float* rstd;
    void* workspace;          /* segm_instnorm_workspace_bytes() */
    size_t workspace_bytes;
    void* stream;
    /* elements between consecutive (b, c) instances of x / residual / y; 0 = spatial (dense).  128^3 volumes are kept with a
     * padded channel stride (a 4 MiB stride puts all channels of a row into one L2 set / memory channel) */
    int64_t x_instance_stride, residual_instance_stride, y_instance_stride;
    /* ABI 8: statistics already summed by the producer of x (segm_conv3d_k3_fwd's stats_partials): fp32 (instances, stats_nparts, 4)
     * of {count, sum, sum of squares, -}; the statistics launch is skipped and the partials are merged (Chan's update, fixed order)
     * by the apply launch.  NULL / 0: the library makes its own pass over x. */
    const float* stats_partials;
    int32_t stats_nparts, reserved2;
} segm_instnorm_fwd_args;

typedef struct segm_instnorm_bwd_args {
    int32_t instances, dtype, act, reserved;
    int64_t spatial;
    float slope, reserved2;
    const void* x;
    const void* dy;
    const void* y;            /* see above; or NULL */
    const float* mean;
    const float* rstd;
    void* dx;
    void* dresidual;          /* or NULL.  16-bit + LeakyReLU: also the staging buffer of g, dx is then rounded twice (see above) */
    void* workspace;
    size_t workspace_bytes;
    void* stream;
    int64_t x_instance_stride, dy_instance_stride, y_instance_stride, dx_instance_stride, dresidual_instance_stride;   /* as above */
} segm_instnorm_bwd_args;

int segm_instnorm_fwd(const segm_instnorm_fwd_args* args);
int segm_instnorm_bwd(const segm_instnorm_bwd_args* args);
size_t segm_instnorm_workspace_bytes(int32_t instances, int64_t spatial);

/* The residual tail of a block with a projection skip (monai dynunet_block.py:98-111 with `downsample`):
 *     y = act(IN(x) + IN(skip))
 * in one apply pass per direction.  IN(skip) is never stored (forward: 4 tensors of traffic, not 6) and its gradient never
 * parked (backward: 10, not 12).  The results - y, both mean / rstd pairs, dx, dskip - are bit-equal to
 *     segm_instnorm_fwd(skip, act 0) -> residual;  segm_instnorm_fwd(x, residual, act)
 * and their two backwards with dresidual wanted: IN(skip) and g = dy act'(.) are rounded to the type in registers where that
 * sequence rounds them through memory, and every sum runs in the same order.  Both stated deviations above are inherited unchanged.
 *   segm_instnorm_stats      the statistics pass over one tensor into `partials` (segm_instnorm_workspace_bytes()), which the
 *                            caller keeps until segm_instnorm_tail_fwd has consumed them as skip_partials
 *   segm_instnorm_tail_fwd   statistics of x (its own pass, or stats_partials as in segm_instnorm_fwd), then the apply pass;
 *                            writes mean / rstd of x and skip_mean / skip_rstd.  workspace: segm_instnorm_workspace_bytes()
 *   segm_instnorm_tail_bwd   y is required iff act != 0.  workspace: segm_instnorm_tail_workspace_bytes() (four sums per slab)
 * Additive to ABI 10 (no existing struct or function changes). */
typedef struct segm_instnorm_stats_args {
    int32_t instances, dtype;
    int64_t spatial;
    const void* x;
    int64_t x_instance_stride;   /* 0 = spatial */
    void* partials;
    size_t partials_bytes;
    void* stream;
} segm_instnorm_stats_args;

typedef struct segm_instnorm_tail_fwd_args {
    int32_t instances, dtype, act, reserved;
    int64_t spatial;
    float slope, eps;
    const void* x;
    const void* skip;
    void* y;
    float* mean;
    float* rstd;
    float* skip_mean;
    float* skip_rstd;
    const void* skip_partials;   /* written by segm_instnorm_stats(skip) with the same instances, spatial and dtype */
    size_t skip_partials_bytes;
    void* workspace;
    size_t workspace_bytes;
    void* stream;
    int64_t x_instance_stride, skip_instance_stride, y_instance_stride;
    const float* stats_partials; /* of x, as in segm_instnorm_fwd_args; or NULL */
    int32_t stats_nparts, reserved2;
} segm_instnorm_tail_fwd_args;

typedef struct segm_instnorm_tail_bwd_args {
    int32_t instances, dtype, act, reserved;
    int64_t spatial;
    float slope, reserved2;
    const void* x;
    const void* skip;
    const void* dy;
    const void* y;
    const float* mean;
    const float* rstd;
    const float* skip_mean;
    const float* skip_rstd;
    void* dx;
    void* dskip;
    void* workspace;
    size_t workspace_bytes;
    void* stream;
    int64_t x_instance_stride, skip_instance_stride, dy_instance_stride, y_instance_stride, dx_instance_stride, dskip_instance_stride;
} segm_instnorm_tail_bwd_args;

int segm_instnorm_stats(const segm_instnorm_stats_args* args);
int segm_instnorm_tail_fwd(const segm_instnorm_tail_fwd_args* args);
int segm_instnorm_tail_bwd(const segm_instnorm_tail_bwd_args* args);
size_t segm_instnorm_tail_workspace_bytes(int32_t instances, int64_t spatial);

/* ------------------------------------------------------------------------------------------------
 * Batched transpose (+ add): out[b, c, r] = in[b, r, c] (+ add[b, c, r]).
 * Replaces the transposing copies around a Mamba layer - `x.reshape(B, C, n).transpose(-1, -2)` feeding LayerNorm and
 * `out.transpose(-1, -2).reshape(B, C, *dims)` + skip (reference model_segmamba/segmamba.py:60-75) - which the
 * reference leaves to strided ATen copies.  in (batch, rows, cols), add / out (batch, cols, rows), contiguous.
 * ------------------------------------------------------------------------------------------------ */
typedef struct segm_transpose_args {
    int32_t batch, rows, cols, dtype;
    const void* in;
    const void* add;          /* or NULL */
    void* out;
    void* stream;
} segm_transpose_args;

int segm_transpose_add(const segm_transpose_args* args);

/* ------------------------------------------------------------------------------------------------
 * ABI 9: out = a + b + c, element-wise, one pass (fp32 sum, one rounding).  Replaces the two binary adds of
 * `out + out_b + out_s` in front of out_proj (reference mamba/mamba_ssm/modules/mamba_simple.py:160 / :264) and of the three
 * directions' `dxz` contributions in the backward pass of the v3 block (autograd's fan-in adds in the reference).
 * a, b, c, out: `count` elements of one dtype (fp32 / fp16 / bf16), dense, 16-byte aligned, count a multiple of 16 bytes' worth;
 * out may be a.
 * ------------------------------------------------------------------------------------------------ */
typedef struct segm_add3_args {
    int64_t count;
    int32_t dtype, reserved;
    const void* a;
    const void* b;
    const void* c;
    void* out;
    void* stream;
} segm_add3_args;

int segm_add3(const segm_add3_args* args);

/* ------------------------------------------------------------------------------------------------
 * ABI 10: out[i] = src[map(i)] for 16-bit elements, i < count (count % 8 == 0, out and map 16-byte aligned) - the one gather per
 * training step that refreshes every re-arranged 16-bit copy of a weight (fragment images, packed blocks; the reference casts and
 * re-lays-out nothing: torch.nn.Conv3d -> cuDNN reads the fp32 / autocast weight as it is).  mode 0: map = int32 source index per
 * element; mode 1: map = int32 (first index, step) per group of eight consecutive elements (an arithmetic progression in src).
 * ------------------------------------------------------------------------------------------------ */
typedef struct segm_gather16_args {
    int64_t count;
    int32_t mode, reserved;
    const void* src;
    const int32_t* map;
    void* out;
    void* stream;
} segm_gather16_args;

int segm_gather16(const segm_gather16_args* args);

/* ------------------------------------------------------------------------------------------------
 * Volume -> tokens with LayerNorm over the channels, forward and backward.
 * Replaces `x.reshape(B, C, n).transpose(-1, -2)` followed by `nn.LayerNorm(C)` at the entry of a Mamba layer
 * (reference model_segmamba/segmamba.py:60-66): a transposing copy, an fp32 LayerNorm and a cast in the reference.
 *
 *   forward   x (batch, channels, spatial) -> y (batch, spatial, channels) = (x - mean_c) * rstd_c * gamma + beta,
 *             mean / rstd (batch, spatial) fp32 (kept for the backward)
 *   backward  dy (batch, spatial, channels), x, mean, rstd, gamma -> dx (batch, channels, spatial), dgamma, dbeta (fp32,
 *             OVERWRITTEN)
 * x, y, dy, dx: one dtype, contiguous.  gamma, beta, dgamma, dbeta: fp32 (channels).  channels and spatial multiples of 8
 * (4 for fp32); channels <= 384 (192 for fp32).
 * ------------------------------------------------------------------------------------------------ */
typedef struct segm_layernorm_args {
    int32_t batch, channels, dtype, reserved;
    int64_t spatial;
    float eps, reserved2;
    const void* x;
    void* y;                  /* forward */
    const float* gamma;
    const float* beta;        /* forward */
    float* mean;
    float* rstd;
    const void* dy;           /* backward ... */
    void* dx;
    float* dgamma;
    float* dbeta;
    void* workspace;          /* segm_layernorm_tokens_workspace_bytes(); backward only */
    size_t workspace_bytes;
    void* stream;
} segm_layernorm_args;

int segm_layernorm_tokens_fwd(const segm_layernorm_args* args);
int segm_layernorm_tokens_bwd(const segm_layernorm_args* args);
size_t segm_layernorm_tokens_workspace_bytes(int32_t batch, int32_t channels, int64_t spatial);

/* ------------------------------------------------------------------------------------------------
 * Gradient clipping + SGD (momentum, Nesterov, weight decay) over a list of fp32 tensors, in two passes.
 * Replaces `torch.nn.utils.clip_grad_norm_(model.parameters(), 12)` followed by `optimizer.step()` of
 * `torch.optim.SGD(lr=1e-2, weight_decay=3e-5, momentum=0.99, nesterov=True)` (reference light_training/trainer.py:461-470,
 * 3_train.py:51-52):
 *
 *   norm = ||all gradients||_2 ;  c = min(1, max_norm / (norm + 1e-6))        (max_norm <= 0: c = 1)
 *   g' = c g + weight_decay p ;  m = momentum m + g' ;  p -= lr (nesterov ? g' + momentum m : m)
 *
 * params / grads / momenta / numel are HOST arrays of `ntensors` entries (device pointers; numel may be 0).  Momentum
 * buffers start at zero (torch's first step, buf = g', is then the same formula).  The gradients are read, not
 * rescaled in place.  workspace: segm_sgd_clip_step_workspace_bytes(); on return (stream order) its first two floats hold
 * {c, norm}.
 * ------------------------------------------------------------------------------------------------ */
typedef struct segm_sgd_args {
    int32_t ntensors, nesterov;
    float* const* params;
    const float* const* grads;
    float* const* momenta;
    const int64_t* numel;
    float lr, momentum, weight_decay, max_norm;
    void* workspace;
    size_t workspace_bytes;
    void* stream;
    /* ABI 8: fp16 autocast with a loss scale (GradScaler, reference light_training/trainer.py:65-67,461-466).  loss_scale: device
     * pointer to the scale S the gradients carry, or NULL (no scaling).  With it the step is unscale_ -> clip -> step without a pass
     * over the gradients: norm = |g| / S, update coefficient = clip / S; if |g| is inf / nan the parameters and momenta are left
     * untouched.  found_inf: device pointer that receives 1.0f (skipped) or 0.0f - the tensor torch._amp_update_scale_ takes - or NULL. */
    const float* loss_scale;
    float* found_inf;
} segm_sgd_args;

int segm_sgd_clip_step(const segm_sgd_args* args);
size_t segm_sgd_clip_step_workspace_bytes(int32_t ntensors, const int64_t* numel);

/* ------------------------------------------------------------------------------------------------
 * Cross entropy over the class axis of (batch, classes, spatial) logits, forward and gradient in one pass.
 * Replaces `nn.CrossEntropyLoss()(pred, label)` and its backward (reference 3_train.py:48,57-66).
 *
 *   loss_v = logsumexp_c(x[b, :, s]) - x[b, label, s] ;  dlogits[b, c, s] = softmax_c(x)[c] - [c == label]
 *   voxels whose label == ignore_index contribute neither loss nor gradient.  Any other label outside [0, classes) is a
 *   caller error (ATen raises a device-side assertion): it turns the loss sum and that voxel's gradient into NaN.
 *
 * logits, dlogits: (batch, classes, spatial) contiguous, one dtype (fp32 / fp16 / bf16; arithmetic in fp32); labels
 * (batch, spatial) int64; classes <= 16.  loss_partial / count_partial: fp32 arrays of segm_cross_entropy_partials()
 * entries (per-workgroup sums of the losses and of the number of counted voxels; the caller adds them and divides -
 * `mean` reduction - and scales dlogits by 1 / count).
 * ------------------------------------------------------------------------------------------------ */
typedef struct segm_cross_entropy_args {
    int32_t batch, classes, dtype, reserved;
    int64_t spatial, ignore_index;
    const void* logits;
    const int64_t* labels;
    void* dlogits;
    float* loss_partial;
    float* count_partial;
    void* stream;
} segm_cross_entropy_args;

int segm_cross_entropy(const segm_cross_entropy_args* args);
int32_t segm_cross_entropy_partials(int32_t batch, int64_t spatial);

/* ------------------------------------------------------------------------------------------------
 * Single-token decode steps (the native ops behind `Mamba.step`, reference mamba_simple.py:356-401).
 *
 * segm_causal_conv1d_update replaces causal_conv1d_cuda.causal_conv1d_update(x, conv_state, weight, bias?, silu)
 *   (reference causal-conv1d/csrc/causal_conv1d.cpp:270-330; Python causal_conv1d_interface.py:68-82):
 *   conv_state <- roll(conv_state, -1) with x in the last slot; out = act(sum_w conv_state * weight + bias).
 *   x, out (batch, dim), conv_state (batch, dim, width) of `dtype`, element strides; weight (dim, width), bias (dim) fp32.
 *
 * segm_selective_state_update replaces selective_state_update(state, x, dt, A, B, C, D?, z?, dt_bias?, dt_softplus)
 *   (reference mamba/mamba_ssm/ops/triton/selective_state_update.py:99-155, a Triton kernel):
 *   dt' = softplus(dt + dt_bias); state <- state exp(dt' A) + dt' B x; out = <state, C> + D x; out *= silu(z).
 *   state (batch, dim, dstate) of `state_dtype` (updated in place); x, dt, z, out (batch, dim) and B, C (batch, dstate) of
 *   `dtype`; A (dim, dstate), D, dt_bias (dim) fp32.  1 <= dstate <= 256.
 * ------------------------------------------------------------------------------------------------ */
typedef struct segm_conv1d_update_args {
    int32_t batch, dim, width, silu;
    int32_t dtype, reserved;
    const void* x;      int64_t x_stride_b, x_stride_d;
    void* conv_state;   int64_t state_stride_b, state_stride_d, state_stride_w;
    void* out;          int64_t out_stride_b, out_stride_d;
    const float* weight;
    const float* bias;        /* or NULL */
    void* stream;
} segm_conv1d_update_args;

int segm_causal_conv1d_update(const segm_conv1d_update_args* args);

typedef struct segm_state_update_args {
    int32_t batch, dim, dstate, dt_softplus;
    int32_t dtype, state_dtype;
    void* state;        int64_t state_stride_b, state_stride_d, state_stride_n;
    const void* x;      int64_t x_stride_b, x_stride_d;
    const void* dt;     int64_t dt_stride_b, dt_stride_d;
    const void* z;      int64_t z_stride_b, z_stride_d;      /* z NULL = no gate */
    void* out;          int64_t out_stride_b, out_stride_d;
    const void* B;      int64_t B_stride_b, B_stride_n;
    const void* C;      int64_t C_stride_b, C_stride_n;
    const float* A;
    const float* D;           /* or NULL */
    const float* dt_bias;     /* or NULL */
    void* stream;
} segm_state_update_args;

int segm_selective_state_update(const segm_state_update_args* args);

/* ------------------------------------------------------------------------------------------------
 * Row-streaming projection  y[m, :] = x[m, :] W^T + bias  for tall activations (rows >> k, n).
 * Replaces the `nn.Linear` calls of the Mamba block on (batch * length, channels) activations - in_proj, x_proj,
 * out_proj - and their data gradients (reference mamba_simple.py:204-208, 264; selective_scan_interface.py:185-205,
 * 247-275), which the reference hands to cuBLAS.  x (rows, k) and y (rows, n) with element row strides (views into wider
 * tensors are fine), w (n, k) contiguous - the nn.Linear layout - all of one 16-bit dtype; bias (n) fp32 or NULL.
 * k a multiple of 8, at most 2048 (up to 192: W stationary in registers; beyond, round 6: W streamed from L2 as well - the
 * projections of stages 2 / 3); n a multiple of 4; x rows 16-byte aligned, y rows 8-byte aligned.
 * accumulate != 0: y += x W^T (+ bias), e.g. `torch.addmm(dconv, dx_dbl, x_proj_weight)` of the reference's backward
 * (selective_scan_interface.py:276).
 * ------------------------------------------------------------------------------------------------ */
typedef struct segm_linear_args {
    int64_t rows;
    int32_t k, n;
    int32_t dtype, accumulate;
    const void* x;      int64_t x_stride_row;
    const void* w;
    const float* bias;
    void* y;            int64_t y_stride_row;
    void* stream;
} segm_linear_args;

int segm_linear_rows(const segm_linear_args* args);

/* ------------------------------------------------------------------------------------------------
 * Channel-first 1x1x1 convolution  y[b, co, s] = sum_ci w[co, ci] x[b, ci, s] + bias[co]  on (batch, channels, voxels)
 * activations whose voxels are contiguous (NCDHW, or channel slices of it).  Replaces the `Conv3d(kernel_size=1)` calls of
 * the conv stem that the reference hands to cuDNN: the residual branch `conv3` of MONAI's UnetResBlock
 * (monai/networks/blocks/dynunet_block.py:72-96), UnetOutBlock (:247-263), GSC.proj3 / proj4 and MlpChannel.fc1 / fc2
 * (model_segmamba/segmamba.py:78-131) - and, with the transposed weight, their data gradients.
 * x, w, y of one 16-bit dtype; w (cout, w_stride) row-major with w_stride >= cin a multiple of 8 and zero padding columns;
 * bias (cout) fp32 or NULL; cin, cout <= 96; spatial (voxels per channel) a multiple of 64; element strides of batch and
 * channel: multiples of 8 for x (16-byte aligned rows), of 4 for y.  accumulate != 0: y += ... (the second half of a
 * concatenated input, `conv3(cat(up, skip))` = conv3a(up) + conv3b(skip)).
 * ------------------------------------------------------------------------------------------------ */
typedef struct segm_pointwise_args {
    int32_t batch, cin, cout;
    int32_t dtype, accumulate;
    int64_t spatial;
    const void* x;      int64_t x_stride_b, x_stride_c;
    const void* w;      int32_t w_stride;
    const float* bias;
    void* y;            int64_t y_stride_b, y_stride_c;
    void* stream;
} segm_pointwise_args;

int segm_pointwise_cf(const segm_pointwise_args* args);

/* ------------------------------------------------------------------------------------------------
 * The encoder's stem convolution: Conv3d(kernel 7, stride 2, padding 3) on at most 4 input channels
 * (model_segmamba/segmamba.py:141; cuDNN in the reference), forward.
 * x4: the input channel-LAST with exactly 4 channels, (batch, din, hin, win, 4) contiguous (missing channels zero) - one
 * transposing copy of the small input, made by the caller; w_packed: (cout, 7, 7, 8, 4) contiguous = weight[co][ci][kz][ky][kx]
 * at [co][kz][ky][kx][ci], kx slot 7 and missing channels zero; bias (cout) fp32 or NULL; y (batch, cout, din/2, hin/2, win/2)
 * contiguous.  One 16-bit dtype; cout <= 48; din, hin even; win a multiple of 32.
 * ------------------------------------------------------------------------------------------------ */
typedef struct segm_stem_args {
    int32_t batch, cout;
    int32_t din, hin, win;
    int32_t dtype;
    const void* x4;
    const void* w_packed;
    const float* bias;
    void* y;
    void* stream;
    /* 0 / 0 = the stem proper (kernel 7, stride 2).  3 / 1: the first 3x3x3 stride-1 padding-1 convolution of the conv stem on
     * the same few input channels (UnetResBlock conv1 of `encoder1`, model_segmamba/segmamba.py:236-244): w_packed (cout, 3, 3, 8, 4),
     * y (batch, cout, din, hin, win), win a multiple of 16. */
    int32_t kernel_size, stride;
    int64_t y_channel_stride;   /* elements between channels of y (batch stride = cout x that); 0 = dense */
} segm_stem_args;

int segm_stem_conv_fwd(const segm_stem_args* args);

/* Weight gradient of the same convolution (the reference: cuDNN's backward-filter through autograd).
 * x4 as above; dy (batch, cout, din/2, hin/2, win/2) contiguous, same 16-bit dtype; dw_packed: fp32 (7, 7, cout16, 32) with
 * cout16 = cout rounded up to 16: [kz][ky][co][kx slot * 4 + ci] (slot 7 / missing channels / co >= cout are padding);
 * workspace: segm_stem_conv_wgrad_workspace_bytes() of per-slab partials, added in a fixed order (deterministic).
 * win in {64, 128, 256}. */
typedef struct segm_stem_wgrad_args {
    int32_t batch, cout;
    int32_t din, hin, win;
    int32_t dtype;
    const void* x4;
    const void* dy;
    float* dw_packed;
    void* workspace;    size_t workspace_bytes;
    void* stream;
    /* 0 / 0 = kernel 7, stride 2.  3 / 1: the 3x3x3 stride-1 layer (see segm_stem_args): dw_packed fp32 (3, 3, cout16, 16) =
     * [kz][ky][co][kx slot (4) * 4 + ci], workspace from segm_stem_conv_wgrad_workspace_bytes2; win in {32, 64, 128}. */
    int32_t kernel_size, stride;
    int64_t dy_channel_stride;  /* elements between channels of dy; 0 = dense */
} segm_stem_wgrad_args;

size_t segm_stem_conv_wgrad_workspace_bytes(int32_t batch, int32_t cout, int32_t din, int32_t hin);
size_t segm_stem_conv_wgrad_workspace_bytes2(int32_t batch, int32_t cout, int32_t din, int32_t hin, int32_t kernel_size, int32_t stride);
int segm_stem_conv_wgrad(const segm_stem_wgrad_args* args);

/* ------------------------------------------------------------------------------------------------
 * Weight gradients of the projections: out (m, n) fp32 = sum_k a[k][.] b[k][.] over a long k (tokens / voxels).
 * The reference gets them from autograd -> cuBLAS: dW of in_proj / out_proj / x_proj / dt_proj
 * (mamba/mamba_ssm/modules/mamba_simple.py:204-208,264; ops/selective_scan_interface.py:272-276) and of the 1x1x1
 * convolutions (monai/networks/blocks/dynunet_block.py:72-96,247-263).
 *   SEGM_WGEMM_TN  a (k, m), b (k, n) row-major, row strides a_stride_row / b_stride_row (elements; any alignment: rows that are
 *                  not 16-byte aligned take 2-byte loads); batch strides ignored; m, n <= 1024
 *   SEGM_WGEMM_NT  a (batch, m, k), b (batch, n, k), unit stride along k, k % 32 == 0, strides % 8 == 0, 16-byte aligned;
 *                  out = sum over the batch of a[i] b[i]^T; m, n <= 96
 * 16-bit operands, fp32 accumulation, per-wave partial sums in the workspace added in a fixed order (bitwise repeatable).
 * ------------------------------------------------------------------------------------------------ */
enum segm_wgemm_layout { SEGM_WGEMM_TN = 0, SEGM_WGEMM_NT = 1 };

typedef struct segm_wgrad_gemm_args {
    int32_t layout, dtype;
    int32_t m, n;
    int64_t k;
    int32_t batch, reserved;
    const void* a;  int64_t a_stride_row, a_stride_batch;
    const void* b;  int64_t b_stride_row, b_stride_batch;
    float* out;
    void* workspace;    size_t workspace_bytes;
    void* stream;
} segm_wgrad_gemm_args;

size_t segm_wgrad_gemm_workspace_bytes(int32_t layout, int32_t m, int32_t n, int64_t k, int32_t batch);

/* out (m, n) fp32 = wide^T skinny: wide (k, m) with unit column stride, m % 8 == 0, m <= 2048, rows 16-byte aligned (base pointer and
 * wide_stride_row % 8 == 0; otherwise SEGM_E_SHAPE); skinny (k, n <= 32); both 16-bit, row strides in elements, k = tokens.  The weight gradient of Mamba's dt_proj - `einsum("dB,Br->dr", ddelta, x_dbl[:, :R])`, reference
 * selective_scan_interface.py:272, R = 3 ... 24 - as the streaming reduction it is (the vendor GEMM spends a tile on three
 * columns).  Per-slab partial sums in the workspace, added in a fixed order.  out is OVERWRITTEN. */
typedef struct segm_skinny_tn_args {
    int64_t k;
    int32_t m, n;
    int32_t dtype, reserved;
    const void* wide;    int64_t wide_stride_row;
    const void* skinny;  int64_t skinny_stride_row;
    float* out;
    void* workspace;     size_t workspace_bytes;
    void* stream;
} segm_skinny_tn_args;
size_t segm_skinny_tn_workspace_bytes(int32_t m, int32_t n, int64_t k);
int segm_skinny_tn(const segm_skinny_tn_args* args);
int segm_wgrad_gemm(const segm_wgrad_gemm_args* args);
/* out[c] (fp32, OVERWRITTEN) = sum over batch and voxels of x[b][c][s]: the bias gradient `dy.sum((0, 2, 3, 4))` of the convolutions
 * that have a bias (reference segmamba.py:78-89, 95-131, 141, 254; cuDNN backward-bias / ATen there).  x (batch, channels, spatial)
 * with unit voxel stride, strides in elements (stride_channel >= spatial: padded volumes are fine); fp32 / fp16 / bf16.  Partials per
 * (b, segment, c) in the workspace, added in a fixed order. */
typedef struct segm_channel_sum_args {
    const void* x;
    int64_t stride_batch, stride_channel, spatial;
    int32_t batch, channels, dtype, reserved;
    float* out;
    void* workspace;     size_t workspace_bytes;
    void* stream;
} segm_channel_sum_args;
size_t segm_channel_sum_workspace_bytes(int32_t batch, int32_t channels, int64_t spatial);
int segm_channel_sum(const segm_channel_sum_args* args);

/* ------------------------------------------------------------------------------------------------
 * Evaluation: Dice and Hausdorff distances of label volumes (additive to ABI 10).
 * Replaces  medpy.metric.binary.dc / hd95 as called per region by reference 5_compute_metrics.py:24-38
 *           (`cal_metric` / `each_cases_metric`), and the counts behind the validation Dice of 3_train.py:82-119.
 *
 * Label volumes are (depth, height, width) uint8, contiguous, x fastest.  A REGION is a set of label values, given by a 256-entry
 * uint8 table in device memory: bit r of table[l] says that label l belongs to region r (up to SEGM_METRICS_MAX_REGIONS at once;
 * BraTS: TC = {1, 3}, WT = {1, 2, 3}, ET = {3}, 5_compute_metrics.py:40-46).  Volumes of region bits ("bit planes": bit r of a
 * byte = region r) are what the three entries hand to one another.
 * ------------------------------------------------------------------------------------------------ */
#define SEGM_METRICS_MAX_REGIONS 8
#define SEGM_METRICS_MAX_PLANES 16                 /* planes per distance-transform call, items per border-distance call */
#define SEGM_METRICS_MAX_VOXELS (1 << 30)
#define SEGM_EDT_MAX_LINE 256                      /* largest depth, height and width of the distance transform */

/* One pass over a prediction and a ground truth.  Per region r:
 *   counts[q * 8 + r], q = 0 .. 4:  |P|, |G|, |P and G|, |border of P|, |border of G|   (40 int64, all OVERWRITTEN; unused regions 0)
 *   border_pred / border_gt: bit r set iff the voxel is in the region and one of its six face neighbours is not, everything outside
 *   the volume counting as not in the region (scipy's binary_erosion with the connectivity-1 cross and border_value 0, which is
 *   medpy's `mask ^ erosion(mask)`).
 * Per-workgroup partial counts in the workspace, added by a second kernel: integers, no atomics.
 * depth * height * width <= SEGM_METRICS_MAX_VOXELS. */
typedef struct segm_seg_regions_args {
    int32_t depth, height, width, reserved;
    const uint8_t* pred;
    const uint8_t* gt;
    const uint8_t* table;          /* 256 bytes, device memory */
    uint8_t* border_pred;          /* (depth, height, width) */
    uint8_t* border_gt;
    int64_t* counts;               /* 40 values, device memory */
    void* workspace;     size_t workspace_bytes;
    void* stream;
} segm_seg_regions_args;
size_t segm_seg_regions_workspace_bytes(int64_t voxels);
int segm_seg_regions(const segm_seg_regions_args* args);

/* Exact squared Euclidean distance transform of a batch of bit planes:
 *   out[p][z][y][x] = min over the voxels v whose bit plane_bit[p] is set in volume plane_volume[p] of
 *                     (spacing_z dz)^2 + (spacing_y dy)^2 + (spacing_x dx)^2
 * i.e. scipy.ndimage.distance_transform_edt(~plane, sampling = spacing) ** 2.  Separable, three passes (x, then y, then z; the y and z
 * passes in place in `out`), brute-force min-plus over the whole line held in LDS: exact and deterministic.
 * fp32 = 0: int32 arithmetic and output, spacing must be (1, 1, 1) (else SEGM_E_DTYPE); a plane without a set bit gives INT32_MAX.
 * fp32 = 1: fp32 arithmetic and output, any positive spacing; a plane without a set bit gives +inf.
 * depth, height, width in [1, SEGM_EDT_MAX_LINE] (else SEGM_E_SHAPE); n_volumes, n_planes in [1, SEGM_METRICS_MAX_PLANES]. */
typedef struct segm_edt_sq_args {
    int32_t depth, height, width;
    int32_t n_volumes, n_planes, fp32;
    float spacing_z, spacing_y, spacing_x;
    int32_t reserved;
    int32_t plane_volume[SEGM_METRICS_MAX_PLANES];
    int32_t plane_bit[SEGM_METRICS_MAX_PLANES];
    const uint8_t* volumes;        /* (n_volumes, depth, height, width) */
    void* out;                     /* (n_planes, depth, height, width) int32 or fp32 */
    void* stream;
} segm_edt_sq_args;
int segm_edt_sq(const segm_edt_sq_args* args);

/* Distances from border voxels to another border, from the squared distance transform of that other border.  Item i:
 *   out[out_offset[i] + k] = sqrt(edt[edt_plane[i]][v_k]),  v_k = the k-th voxel (in memory order) whose bit border_bit[i] is set in
 *   volume border_volume[i],  k < out_count[i]
 * (medpy's `__surface_distances`: `distance_transform_edt(~reference_border)[result_border]`).  out_count[i] is the border count
 * that the region pass reported; out_offset[i] + out_count[i] <= out_capacity.  The order is fixed: per-workgroup counts, an
 * exclusive scan of them (both in the workspace), then the write - no atomics.  `edt` is int32 (fp32 = 0) or fp32 (fp32 = 1). */
typedef struct segm_border_distances_args {
    int64_t voxels;                /* depth * height * width <= SEGM_METRICS_MAX_VOXELS */
    int32_t n_volumes, n_planes, n_items, fp32;
    int32_t border_volume[SEGM_METRICS_MAX_PLANES];
    int32_t border_bit[SEGM_METRICS_MAX_PLANES];
    int32_t edt_plane[SEGM_METRICS_MAX_PLANES];
    int64_t out_offset[SEGM_METRICS_MAX_PLANES];
    int64_t out_count[SEGM_METRICS_MAX_PLANES];
    int64_t out_capacity;          /* elements of `out` */
    const uint8_t* borders;        /* (n_volumes, voxels) bit planes */
    const void* edt;               /* (n_planes, voxels) */
    float* out;
    void* workspace;     size_t workspace_bytes;
    void* stream;
} segm_border_distances_args;
size_t segm_border_distances_workspace_bytes(int64_t voxels, int32_t n_items);
int segm_border_distances(const segm_border_distances_args* args);

/* What the surface metrics need of those lists, without the lists (additive to ABI 10; csrc/surface_stats.hip): medpy's asd / assd /
 * hd / hd95 (light_training/evaluation/metric.py:314-383) and the voxel-counted surface Dice.  An ITEM is a list as above: the values
 * d = sqrtf((float)edt[edt_plane[i]][v]) at the voxels v whose bit border_bit[i] is set in volume border_volume[i], formed as
 * segm_border_distances forms them (the two entries agree bit for bit).  The items with item_group[i] == g form the JOINED list of
 * group g (a region: prediction -> ground truth and back).  `out`, 16 x 4 + 16 x 2 doubles in device memory, all OVERWRITTEN:
 *   out[4 i ..]      = count, sum of d (fp64), max d, number of voxels with d <= tolerance[i] (tolerance[i] < 0: none); an item
 *                      without a set voxel gives 0, 0, 0, 0, as do the rows past n_items
 *   out[64 + 2 g ..] = d at rank[g][0] and at rank[g][1] (0-based) of the ascending joined list; NaN for a rank that is negative or
 *                      not below the group's count, and in the rows past n_groups
 * Radix selection on the 32-bit key of the squared value (the int32, or the bits of the non-negative fp32), 8-bit digits: four passes
 * over the border bytes, `edt` is read at set voxels only; sqrtf and the conversion are monotone, so the result equals "sort the
 * list, index it".  An EDT sentinel (the target plane had no set voxel) is an ordinary key: callers pass live regions.
 * Integer atomics on the histograms only; the fp64 sums go thread -> wave -> LDS -> one slot per workgroup, added by one workgroup in
 * a fixed order: two calls are bit-equal.
 * SEGM_E_SHAPE: voxels outside [1, SEGM_METRICS_MAX_VOXELS]; n_items or n_groups outside [1, SEGM_METRICS_MAX_PLANES]; an item_group
 * outside [0, n_groups); a volume, bit or plane index out of range; a group whose items x voxels reach 2^32 (the histograms count in
 * 32 bits); edt or out misaligned.  SEGM_E_NULL: a NULL pointer.  SEGM_E_DTYPE: fp32 not 0 or 1.  SEGM_E_WORKSPACE: workspace NULL,
 * misaligned (8 bytes) or smaller than segm_border_stats_workspace_bytes (0 for arguments out of range).  Nothing is launched then. */
typedef struct segm_border_stats_args {
    int64_t voxels;                /* depth * height * width <= SEGM_METRICS_MAX_VOXELS */
    int32_t n_volumes, n_planes, n_items, n_groups;
    int32_t fp32, reserved;        /* edt is int32 (0) or fp32 (1) */
    int32_t border_volume[SEGM_METRICS_MAX_PLANES];
    int32_t border_bit[SEGM_METRICS_MAX_PLANES];
    int32_t edt_plane[SEGM_METRICS_MAX_PLANES];
    int32_t item_group[SEGM_METRICS_MAX_PLANES];
    float tolerance[SEGM_METRICS_MAX_PLANES];
    int64_t rank[SEGM_METRICS_MAX_PLANES][2];
    const uint8_t* borders;        /* (n_volumes, voxels) bit planes */
    const void* edt;               /* (n_planes, voxels) */
    double* out;
    void* workspace;     size_t workspace_bytes;
    void* stream;
} segm_border_stats_args;
size_t segm_border_stats_workspace_bytes(int64_t voxels, int32_t n_items);
int segm_border_stats(const segm_border_stats_args* args);

/* The same transform for sides up to SEGM_EDT_LONG_MAX_LINE, at a cost linear in the line length (additive to ABI 10;
 * csrc/edt_long.hip).  Meaning, planes, spacing rules and sentinels are those of segm_edt_sq, and the struct has its layout up to
 * `stream` with `reserved` taken by max_workgroups; segm_edt_sq itself keeps its limit and its refusals.
 * x pass: the row's bit planes as 64-bit masks in LDS, clz / ctz per lane.  y and z pass: the lower envelope of the parabolas
 * g[i] + (s (u - i))^2 (Meijster / Felzenszwalb-Huttenlocher), one thread per line, a forward scan that stacks (position, start of its
 * interval, g) and a backward scan that writes - in place in `out`.  The stacks live in the workspace, 8 bytes x line length per
 * thread in flight: workgroups are persistent and reuse their area for one batch of 256 lines after the other, so the size follows
 * the grid, not the volume (1 GiB at 400 x 512 x 512, reached by any volume with at least 1024 batches of 512-long lines).
 * max_workgroups: 0 = the default (1024); a smaller positive value lowers the grid of the line passes (larger ones change nothing).
 * fp32 = 0: integer arithmetic, equal to segm_edt_sq at every voxel.  fp32 = 1: intersections in fp64, values in fp32 rounded as
 * segm_edt_sq rounds them - within its 1e-6 relative bound of the exact value, not bit-equal to it (the two may pick different
 * minimisers among candidates that differ by a rounding).  Deterministic: no atomics, two calls are bit-equal.
 * depth, height, width in [1, SEGM_EDT_LONG_MAX_LINE], depth * height * width <= SEGM_METRICS_MAX_VOXELS (else SEGM_E_SHAPE);
 * workspace NULL, misaligned (8 bytes) or smaller than segm_edt_sq_long_workspace_bytes: SEGM_E_WORKSPACE. */
#define SEGM_EDT_LONG_MAX_LINE 2048
typedef struct segm_edt_sq_long_args {
    int32_t depth, height, width;
    int32_t n_volumes, n_planes, fp32;
    float spacing_z, spacing_y, spacing_x;
    int32_t max_workgroups;        /* 0 = default */
    int32_t plane_volume[SEGM_METRICS_MAX_PLANES];
    int32_t plane_bit[SEGM_METRICS_MAX_PLANES];
    const uint8_t* volumes;        /* (n_volumes, depth, height, width) */
    void* out;                     /* (n_planes, depth, height, width) int32 or fp32 */
    void* stream;
    void* workspace;     size_t workspace_bytes;
} segm_edt_sq_long_args;
size_t segm_edt_sq_long_workspace_bytes(int32_t depth, int32_t height, int32_t width, int32_t n_planes, int32_t fp32);
int segm_edt_sq_long(const segm_edt_sq_long_args* args);

/* Bounding boxes of bit planes in one pass over the volumes.  Item i: the voxels whose bit item_bit[i] is set in volume
 * item_volume[i], OR-ed with bit item_bit2[i] of volume item_volume2[i] unless that is -1 (the border of a prediction and the border
 * of a ground truth: every border voxel of either lies in the box, so the nearest one does too, and the distance transform may
 * run on the crop).
 *   boxes[6 i ..] = z0, z1, y0, y1, x0, x1, half-open; an item without a set voxel leaves z1 = y1 = x1 = 0 (and the lower ends at
 *   0x7f7f7f7f), as segm_nonzero_mask_bbox marks an empty mask.  All SEGM_METRICS_MAX_PLANES x 6 values are OVERWRITTEN.
 * 16-byte loads along x when width % 16 == 0; a wave that saw no set bit of an item exchanges nothing for it; per workgroup at
 * most 6 integer min / max atomics per item, whose order does not matter: deterministic.
 * Sides below 2^20, depth * height * width <= SEGM_METRICS_MAX_VOXELS, n_volumes and n_items in [1, SEGM_METRICS_MAX_PLANES]. */
typedef struct segm_planes_bbox_args {
    int32_t depth, height, width;
    int32_t n_volumes, n_items, reserved;
    int32_t item_volume[SEGM_METRICS_MAX_PLANES];
    int32_t item_bit[SEGM_METRICS_MAX_PLANES];
    int32_t item_volume2[SEGM_METRICS_MAX_PLANES];     /* -1: a single plane */
    int32_t item_bit2[SEGM_METRICS_MAX_PLANES];
    const uint8_t* volumes;        /* (n_volumes, depth, height, width) */
    int32_t* boxes;                /* SEGM_METRICS_MAX_PLANES x 6 int32 in device memory */
    void* stream;
} segm_planes_bbox_args;
int segm_planes_bbox(const segm_planes_bbox_args* args);

/* ------------------------------------------------------------------------------------------------
 * Signed-distance and edge training targets (additive to ABI 10; csrc/sdm.hip).
 * Replaces, of the reference's light_training/dataloading/dataset_sdm_edge.py: compute_sdf (:56-85: two
 * scipy.ndimage.distance_transform_edt and skimage's find_boundaries(mode='inner') per region), get_edge_points / edge_3d (:33-54:
 * `img - binary_erosion(img)`), and `seg_sdm = 1 - compute_sdf(seg) + seg_edge` of its `post` hook (:143-157).
 * segm_sdm_masks makes the bit volumes, segm_edt_sq / segm_edt_sq_long transform their planes (unit spacing, int32, unchanged),
 * segm_sdm_compose normalises, signs and adds.
 * ------------------------------------------------------------------------------------------------ */
enum segm_sdm_label_dtype { SEGM_SDM_LABEL_U8 = 0, SEGM_SDM_LABEL_I16 = 1, SEGM_SDM_LABEL_I64 = 2 };

/* One stencil pass over n label volumes (n, depth, height, width), contiguous, read in their own dtype (no cast pass); a value
 * outside [0, 255] belongs to no region.  `table` as above: bit r of table[l] = label l is in region r, r < n_regions.  Per volume
 * four uint8 volumes of region bits, all written at every voxel:
 *   inside    bit r set iff the voxel is in region r
 *   outside   bit r set iff the voxel is not in region r, for r < n_regions (the bits above stay clear)
 *   edge      bit r set iff the voxel is in the region and one of its six face neighbours is not, everything outside the volume
 *             counting as not in the region: `img - binary_erosion(img, cross)` with border_value 0, segm_seg_regions' border rule
 *   boundary  bit r set iff the voxel is in the region and one of its face neighbours INSIDE the volume is not: skimage's
 *             find_boundaries(mode='inner') on a boolean image (dilation != erosion with reflecting borders, then the foreground).
 *             A subset of `edge`; the two differ at region voxels on a face of the volume whose in-volume neighbours are all inside.
 *   counts[v * 8 + r] = the voxels of volume v in region r (n x 8 int64, all OVERWRITTEN; unused regions 0)
 * The four outputs overlap neither the labels nor one another.
 * Rows along x go across the lanes, the neighbours in y and z come from the caches.  The counts go thread -> wave -> workgroup ->
 * one 64-bit integer atomic per region that has a voxel in the workgroup: integers only, the order does not matter.
 * SEGM_E_SHAPE: a side outside [1, SEGM_EDT_LONG_MAX_LINE], more than SEGM_METRICS_MAX_VOXELS voxels per volume, n outside
 * [1, SEGM_METRICS_MAX_PLANES], n_regions outside [1, SEGM_METRICS_MAX_REGIONS], labels or counts not aligned to their element.
 * SEGM_E_NULL: a NULL pointer.  SEGM_E_DTYPE: label_dtype not of segm_sdm_label_dtype.  Nothing is launched then. */
typedef struct segm_sdm_masks_args {
    int32_t depth, height, width;
    int32_t n, n_regions, label_dtype;
    const void* labels;            /* (n, depth, height, width) uint8, int16 or int64 */
    const uint8_t* table;          /* 256 bytes, device memory */
    uint8_t* inside;               /* (n, depth, height, width) each */
    uint8_t* outside;
    uint8_t* edge;
    uint8_t* boundary;
    int64_t* counts;               /* n x 8 values, device memory */
    void* stream;
} segm_sdm_masks_args;
int segm_sdm_masks(const segm_sdm_masks_args* args);

/* The targets of up to SEGM_METRICS_MAX_PLANES (volume, region) pairs from the bit volumes above and the int32 squared distance
 * transforms of their planes.  Item i is region bit[i] of volume[i]; edt[pos_plane[i]] holds pos^2, the transform whose seeds are
 * that bit of `outside`, edt[neg_plane[i]] holds neg^2, seeded by that bit of `inside`; c = counts[volume[i] * 8 + bit[i]] and
 * live = 0 < c < voxels.  Two kernels:
 *   maxima   Pmax^2 = max pos^2 and Nmax^2 = max neg^2 of every live item: thread -> wave -> workgroup, then one 32-bit integer
 *            maximum per workgroup and item into the workspace, which the entry zeroes first.  pos^2 is read where the inside bit
 *            is set and neg^2 where it is not (each is 0 elsewhere).
 *   compose  per voxel, in fp64:  sdf = 0 if not live, else 0 exactly if the boundary bit is set, else
 *            -sqrt(pos^2) / sqrt(Pmax^2) if the inside bit is set, else +sqrt(neg^2) / sqrt(Nmax^2);  sdm = 1 - sdf + edge.
 *            This is compute_sdf's formula: both minima are 0 for a live region, one of the two distances is 0 at every voxel
 *            (nothing cancels), and a live plane cannot divide by zero.  A plane that is not live never reads its transforms,
 *            which hold the EDT's sentinel.
 * Outputs, fp32, plane out_plane[i] of (n_out_planes, voxels) each, rounded from fp64 once: sdf, sdm, and edge as 0.0 / 1.0.  Each
 * is nullable, at least one must be given; with sdf and sdm both NULL `edt` and `workspace` may be NULL and no maximum is taken.
 * A thread takes 16-byte packets (four int32 of a plane, four bytes of a bit volume, one 16-byte store) where the item's planes
 * and outputs are 16-byte aligned, single voxels otherwise and in the tail; both routes call one per-voxel function.
 * Integer atomics only; no floating-point atomics: two calls are bit-equal.
 * SEGM_E_SHAPE: voxels outside [1, SEGM_METRICS_MAX_VOXELS]; n_items outside [1, SEGM_METRICS_MAX_PLANES]; a volume, bit, plane or
 * output plane index out of range; two items with one output plane; edt or an output not aligned to 4 bytes, counts to 8.
 * SEGM_E_NULL: a required pointer is NULL, or no output is given.  SEGM_E_WORKSPACE, when sdf or sdm is given: workspace NULL, not
 * aligned to 4 bytes or smaller than SEGM_SDM_COMPOSE_WORKSPACE_BYTES.  Nothing is launched then. */
#define SEGM_SDM_COMPOSE_WORKSPACE_BYTES (2 * SEGM_METRICS_MAX_PLANES * 4)
typedef struct segm_sdm_compose_args {
    int64_t voxels;                /* depth * height * width <= SEGM_METRICS_MAX_VOXELS */
    int32_t n_items, n_volumes, n_planes, n_out_planes;
    int32_t volume[SEGM_METRICS_MAX_PLANES];
    int32_t bit[SEGM_METRICS_MAX_PLANES];
    int32_t pos_plane[SEGM_METRICS_MAX_PLANES];
    int32_t neg_plane[SEGM_METRICS_MAX_PLANES];
    int32_t out_plane[SEGM_METRICS_MAX_PLANES];
    const int32_t* edt;            /* (n_planes, voxels) */
    const uint8_t* inside;         /* (n_volumes, voxels) each */
    const uint8_t* edge;
    const uint8_t* boundary;
    const int64_t* counts;         /* n_volumes x 8, as segm_sdm_masks wrote them */
    float* sdf;                    /* (n_out_planes, voxels) each, nullable */
    float* sdm;
    float* edge_out;
    void* workspace;     size_t workspace_bytes;
    void* stream;
} segm_sdm_compose_args;
int segm_sdm_compose(const segm_sdm_compose_args* args);

/* ------------------------------------------------------------------------------------------------
 * Finishing a prediction on the device (additive to ABI 10; csrc/postprocess.hip, csrc/ccl_roots.hip).
 * Replaces, of the reference's light_training/prediction.py: predict_raw_probability (:33-62) + the argmax of 4_predict.py:81 +
 * predict_noncrop_probability (:64-108) by ONE launch, and large_connected_domain (:17-27: skimage.measure.label at connectivity 1,
 * keep the largest, scipy.ndimage.binary_fill_holes) by connected components on the device.
 * ------------------------------------------------------------------------------------------------ */
#define SEGM_RESAMPLE_MAX_CLASSES 8              /* the default bound of the Python wrapper (a BraTS-sized class count) */
#define SEGM_RESAMPLE_CLASS_LIMIT 32             /* what segm_resample_argmax accepts: the kernel loops over the classes */
#define SEGM_CCL_MAX_VOXELS 2147483647LL         /* depth * height * width < 2^31: labels are int32 linear indices */

/* Logits (classes, in_depth, in_height, in_width) -> uint8 label volume (out_depth, out_height, out_width).  For every voxel of the
 * box [box_z, box_z + box_depth) x [box_y, ..) x [box_x, ..) the trilinear sample of each class at the voxel's source coordinate
 * (F.interpolate(mode="trilinear", align_corners=False) from the logits' size to the box's size: per axis
 * src = max((dst + 0.5) * (in / out) - 0.5, 0), i0 = floor(src), i1 = min(i0 + 1, in - 1), lambda = src - i0, fp32 arithmetic), the index
 * of the largest (the first of equal values), one byte; every voxel outside the box is written 0 by the same launch.  When the box has
 * the logits' size the weights are exactly 0 / 1 and the result is the plain argmax.
 * regions (optional, else NULL): a second (out_depth, out_height, out_width) uint8 volume = table[label], the region bit planes that
 * the evaluation entries take; `table` (256 bytes, device memory) is required with it.
 * dtype SEGM_F32 / SEGM_F16 / SEGM_BF16; element strides for class, z and y, unit stride along x; `logits` aligned to its element size.
 * 1 .. SEGM_RESAMPLE_CLASS_LIMIT classes (the reference's CT example takes the argmax over 10:
 * light_training/examples/AbdomenAtlas1.0Mini/4_predict_diffunet.py:87-109). */
typedef struct segm_resample_argmax_args {
    int32_t classes, dtype;
    int32_t in_depth, in_height, in_width;
    int32_t box_z, box_y, box_x;
    int32_t box_depth, box_height, box_width;
    int32_t out_depth, out_height, out_width;
    int64_t stride_c, stride_z, stride_y;
    const void* logits;
    uint8_t* labels;
    uint8_t* regions;              /* optional */
    const uint8_t* table;          /* required with regions */
    void* stream;
} segm_resample_argmax_args;
int segm_resample_argmax(const segm_resample_argmax_args* args);

/* Connected components at connectivity 1 (six face neighbours; the outside of the volume connects nothing).  Connectivity 2 and 3:
 * segm_ccl_roots_conn below.
 * A voxel is inside the mask iff ((bit >= 0 ? (v >> bit) & 1 : v != 0) != invert), v its byte of `volume`.
 *   roots[i] = -1 outside the mask, otherwise the SMALLEST linear index (z * height + y) * width + x of the voxel's component
 * - a definition that does not depend on the order in which anything happened: two calls are bit-equal.
 * Three launches, no readback, whatever the volume: labels of 64 x 4 x 4 tiles converge in LDS, tile faces are joined by a
 * lock-free union-find on agent-scope atomic min (workspace: one int32 per voxel), a last pass replaces every label by its root. */
typedef struct segm_ccl_roots_args {
    int32_t depth, height, width;
    int32_t bit;                   /* 0 .. 7, or -1: value != 0 */
    int32_t invert, reserved;
    const uint8_t* volume;
    int32_t* roots;                /* (depth, height, width) */
    void* workspace;     size_t workspace_bytes;
    void* stream;
} segm_ccl_roots_args;
size_t segm_ccl_roots_workspace_bytes(int64_t voxels);
int segm_ccl_roots(const segm_ccl_roots_args* args);

/* From the roots: sizes[i] = the voxel count of the component whose root is voxel i, 0 at every other voxel (integer atomics:
 * exact); touches[i] = 1 at a root whose component has a voxel on a face of the volume, 0 elsewhere.  Both are OVERWRITTEN. */
typedef struct segm_ccl_sizes_args {
    int32_t depth, height, width, reserved;
    const int32_t* roots;
    int32_t* sizes;                /* (depth, height, width) */
    uint8_t* touches;              /* (depth, height, width) */
    void* stream;
} segm_ccl_sizes_args;
int segm_ccl_sizes(const segm_ccl_sizes_args* args);

enum segm_ccl_select_mode {
    SEGM_CCL_LARGEST = 0,          /* the component with the most voxels; of equally large ones the one whose root comes LAST in memory */
    SEGM_CCL_MIN_SIZE = 1,         /* every component of at least min_size voxels */
    SEGM_CCL_FILL = 2              /* roots of the INVERTED mask: out = mask | (zero voxels whose zero-component touches no face) */
};
/* out (uint8 0 / 1) by `mode`.  info (3 int64 in device memory, OVERWRITTEN): the number of components, the root of the largest
 * (-1 when there is none) and its voxel count - a device reduction over the root counts (per-workgroup partials in the workspace). */
typedef struct segm_ccl_select_args {
    int32_t depth, height, width;
    int32_t mode, min_size, reserved;
    const int32_t* roots;
    const int32_t* sizes;
    const uint8_t* touches;        /* SEGM_CCL_FILL only, else may be NULL */
    uint8_t* out;                  /* (depth, height, width) */
    int64_t* info;
    void* workspace;     size_t workspace_bytes;
    void* stream;
} segm_ccl_select_args;
size_t segm_ccl_select_workspace_bytes(int64_t voxels);
int segm_ccl_select(const segm_ccl_select_args* args);

/* Labelled connected components (additive to ABI 10; csrc/ccl_roots.hip, csrc/ccl_labels.hip): every class of a label map in ONE pass.
 * What the reference's CT example needs per organ (4_predict_diffunet.py:97-109 writes `labels == i` per organ; prediction.py:17-27
 * `large_connected_domain` keeps the largest component) and nnU-Net's "keep the largest component of every class".
 * Two voxels belong to one component when a path of face neighbours (connectivity 1) with the SAME NON-ZERO label joins them.
 *   roots[i] = -1 where the label is 0, otherwise the SMALLEST linear index of the voxel's component
 * - the definition of segm_ccl_roots, so roots[labels == c] equals segm_ccl_roots of the mask `labels == c` on those voxels, the
 * result depends on no order and two calls are bit-equal.  Three launches, no readback; workspace: one int32 per voxel.
 * segm_ccl_sizes takes these roots unchanged. */
typedef struct segm_ccl_label_roots_args {
    int32_t depth, height, width, reserved;
    const uint8_t* labels;         /* (depth, height, width) */
    int32_t* roots;                /* (depth, height, width) */
    void* workspace;     size_t workspace_bytes;
    void* stream;
} segm_ccl_label_roots_args;
size_t segm_ccl_label_roots_workspace_bytes(int64_t voxels);
int segm_ccl_label_roots(const segm_ccl_label_roots_args* args);

/* Selection per label from the label volume, its roots and their sizes.  mode SEGM_CCL_LARGEST: a voxel keeps its label iff its
 * component is the largest OF ITS LABEL (equal sizes: the root that comes LAST in memory); SEGM_CCL_MIN_SIZE: iff its component has
 * at least min_size voxels; otherwise it becomes 0.  SEGM_CCL_FILL is not a mode here.
 * apply (optional, 256 bytes, device memory): apply[l] == 0 passes label l through untouched; NULL selects on every label.
 * info (256 x 3 int64 in device memory, OVERWRITTEN): per label the number of components, the winner's root (-1: label absent) and
 * the winner's voxel count.  The winner is an integer maximum over (size << 32) | root: per workgroup in LDS, then one 64-bit atomic
 * max per label and workgroup into the workspace - no floating point, two calls are bit-equal.  One memset and two launches. */
typedef struct segm_ccl_label_select_args {
    int32_t depth, height, width;
    int32_t mode, min_size, reserved;
    const uint8_t* labels;
    const int32_t* roots;
    const int32_t* sizes;
    const uint8_t* apply;          /* optional */
    uint8_t* out;                  /* (depth, height, width) */
    int64_t* info;                 /* [256][3] */
    void* workspace;     size_t workspace_bytes;
    void* stream;
} segm_ccl_label_select_args;
size_t segm_ccl_label_select_workspace_bytes(int64_t voxels);
int segm_ccl_label_select(const segm_ccl_label_select_args* args);

/* Connected components at connectivity 1, 2 or 3 (additive to ABI 10; csrc/ccl_roots.hip).  `connectivity` c is that of
 * scipy.ndimage.generate_binary_structure(3, c) and skimage.measure.label(connectivity=c): two voxels are neighbours when their
 * offset has at most c non-zero coordinates, each of them +-1 - 6 (faces), 18 (faces and edges) or 26 (faces, edges and corners)
 * neighbours.  nnU-Net's post-processing, cc3d and the BraTS lesion-wise tooling label at full connectivity (3); the reference's
 * large_connected_domain at 1.  The outside of the volume connects nothing: a row's last voxel is no neighbour of the next row's first.
 * Everything else is the contract of segm_ccl_roots: the mask by `bit` / `invert`, roots[i] = -1 outside the mask, otherwise the
 * SMALLEST linear index of the voxel's component (independent of any order: two calls are bit-equal), three launches, no readback,
 * a workspace of segm_ccl_roots_workspace_bytes.  The roots go to segm_ccl_sizes / segm_ccl_select unchanged.
 * connectivity == 1 makes the launches of segm_ccl_roots.  Any other value than 1, 2, 3 is SEGM_E_SHAPE.  Every refusal launches
 * nothing and leaves `roots` untouched. */
typedef struct segm_ccl_roots_conn_args {
    int32_t depth, height, width;
    int32_t bit;                   /* 0 .. 7, or -1: value != 0 */
    int32_t invert, connectivity;  /* 1, 2, 3 */
    const uint8_t* volume;
    int32_t* roots;                /* (depth, height, width) */
    void* workspace;     size_t workspace_bytes;
    void* stream;
} segm_ccl_roots_conn_args;
int segm_ccl_roots_conn(const segm_ccl_roots_conn_args* args);

/* The labelled form: two voxels are one component when a path of c-neighbours with the SAME NON-ZERO label joins them (two different
 * labels that touch, diagonally or not, are never joined).  The contract of segm_ccl_label_roots otherwise: on `labels == k` the
 * roots equal segm_ccl_roots_conn of that mask at the same connectivity; workspace of segm_ccl_label_roots_workspace_bytes;
 * connectivity == 1 makes the launches of segm_ccl_label_roots.  segm_ccl_sizes and segm_ccl_label_select take the roots unchanged. */
typedef struct segm_ccl_label_roots_conn_args {
    int32_t depth, height, width, connectivity;
    const uint8_t* labels;         /* (depth, height, width) */
    int32_t* roots;                /* (depth, height, width) */
    void* workspace;     size_t workspace_bytes;
    void* stream;
} segm_ccl_label_roots_conn_args;
int segm_ccl_label_roots_conn(const segm_ccl_label_roots_conn_args* args);

/* ------------------------------------------------------------------------------------------------
 * Preparing a case on the device (additive to ABI 10; csrc/preprocess.hip).
 * Replaces, of the reference's light_training/preprocessing: create_nonzero_mask + get_bbox_from_mask (cropping/cropping.py:8-33; the
 * hole filling between them is segm_ccl_* with SEGM_CCL_FILL), the crop and the `seg[(seg == 0) & ~mask] = -1` rule (:35-48),
 * ZScoreNormalization.run (normalization/default_normalization_schemes.py:31-50) and the `np.max(seg)` / per-class counts of
 * run_case_npy (preprocessors/default_preprocessor.py:203-210).
 * ------------------------------------------------------------------------------------------------ */
#define SEGM_PREP_MAX_CHANNELS 8
#define SEGM_PREP_COUNT_BINS 260

/* data (channels, depth, height, width) fp32, element strides for channel, z and y, unit stride along x.
 *   mask[z, y, x] = 1 where any channel is != 0 (NaN is, -0 is not), else 0                     (cropping.py:16-19)
 *   bbox = [z0, y0, x0, z1, y1, x1], half-open, of the mask                                     (get_bbox_from_mask, cropping.py:33)
 * in one pass.  An all-zero volume leaves z1 = y1 = x1 = 0.  The box of the mask is the box of the hole-filled mask (a hole is
 * enclosed along every axis), so it does not wait for the filling.  Both outputs are OVERWRITTEN. */
typedef struct segm_nonzero_mask_bbox_args {
    int32_t channels, depth, height, width;
    int64_t stride_c, stride_z, stride_y;
    const float* data;
    uint8_t* mask;                 /* (depth, height, width), contiguous */
    int32_t* bbox;                 /* 6 int32 in device memory */
    void* stream;
} segm_nonzero_mask_bbox_args;
int segm_nonzero_mask_bbox(const segm_nonzero_mask_bbox_args* args);

enum segm_prep_seg_dtype { SEGM_PREP_SEG_NONE = 0, SEGM_PREP_SEG_F32 = 1, SEGM_PREP_SEG_U8 = 2, SEGM_PREP_SEG_I16 = 3 };

/* The box [box_z, box_z + box_depth) x [box_y, ..) x [box_x, ..) of `data` (as above), of the contiguous (depth, height, width)
 * volumes `mask` (uint8, the FILLED non-zero mask) and `seg` (seg_dtype; NULL with SEGM_PREP_SEG_NONE).
 * The relabelled seg of a voxel: its seg value, but nonzero_label where the seg is 0 and the mask is 0 (cropping.py:43); without a
 * seg 0 inside the mask and nonzero_label outside (cropping.py:45-48).
 *
 * segm_crop_stats: per channel the mean and the population standard deviation (numpy's mean() / std()) over the box, or with
 * `masked` over the box's voxels whose relabelled seg is >= 0 (default_normalization_schemes.py:42-44).  fp64 accumulation in two
 * passes (sum, then sum of squared deviations from the mean) with a fixed reduction order: per-workgroup partials in the
 * workspace, one workgroup adds them in index order - two calls are bit-equal.  The results stay on the device:
 *   stats64[0..7] mean, stats64[8..15] std, stats64[16] the voxel count; stats32[0..7] / [8..15] the same rounded to fp32.
 * `mask` may be NULL unless `masked`.
 *
 * segm_crop_normalize: one launch writes
 *   out (channels, box_depth, box_height, box_width) fp32, dense = (x - stats32 mean) / max(stats32 std, 1e-8) in fp32 arithmetic
 *       (:49); with `masked` the voxels whose relabelled seg is < 0 are copied unchanged (:45);
 *   seg_out (box_depth, box_height, box_width) int16 = the relabelled seg (optional);
 *   counts[SEGM_PREP_COUNT_BINS] int64, OVERWRITTEN (optional): [l] the voxels of label l for l = 0 .. 255, [256] the negative
 *       ones, [257] those above 255, [258] the voxels whose seg value is no integer in [-1, 32767] (written as label 0: a caller
 *       must treat a non-zero [258] as an error), [259] 0.
 * `mask` may be NULL when neither seg_out, counts nor `masked` is given (plain normalisation). */
typedef struct segm_crop_args {
    int32_t channels, depth, height, width;
    int32_t box_z, box_y, box_x, box_depth, box_height, box_width;
    int32_t seg_dtype, masked, nonzero_label, reserved;
    int64_t stride_c, stride_z, stride_y;
    const float* data;
    const uint8_t* mask;
    const void* seg;
    double* stats64;               /* 17 doubles; segm_crop_stats only */
    float* stats32;                /* 16 floats: written by segm_crop_stats, read by segm_crop_normalize */
    float* out;                    /* segm_crop_normalize only, as seg_out and counts */
    int16_t* seg_out;
    int64_t* counts;
    void* workspace;     size_t workspace_bytes;      /* segm_crop_stats only */
    void* stream;
} segm_crop_args;
size_t segm_crop_stats_workspace_bytes(int32_t channels, int32_t box_depth, int32_t box_height, int32_t box_width);
int segm_crop_stats(const segm_crop_args* args);
int segm_crop_normalize(const segm_crop_args* args);

/* segm_crop_normalize with a per-channel clip in front of the subtraction: CTNormalization.run
 * (normalization/default_normalization_schemes.py:83-95) on the box,
 *   out = (min(max(x, lower), upper) - mean) / max(std, 1e-8)      in fp32 arithmetic, the division correctly rounded.
 * stats32 holds 32 floats here: [0..7] mean, [8..15] std, [16..23] lower, [24..31] upper (the dataset's foreground mean, std and
 * 0.5 / 99.5 percentiles, rounded to fp32).  A NaN stays a NaN, as under np.clip.  The crop, the relabelled seg, the label counts
 * and every limit are segm_crop_normalize's - one kernel body serves both; `masked` must be 0 (the reference normalises CT with
 * use_mask_for_norm=False, default_preprocessor.py:239), else SEGM_E_SHAPE. */
int segm_crop_clip_normalize(const segm_crop_args* args);

/* ------------------------------------------------------------------------------------------------
 * The intensity fingerprint of a case (additive to ABI 10; csrc/fingerprint.hip).
 * Replaces the reference's DefaultPreprocessor.collect_foreground_intensities (preprocessors/default_preprocessor.py:413-451):
 * the foreground mask `segmentation[0] > 0` (:431), the compaction `images[i][foreground_mask]` (:434), the draw of num_samples
 * of its values (:439-440) and np.min / np.max / np.median / np.percentile / np.mean of them (:441-449).  The compaction is never
 * written: foreground voxels are addressed by their rank in C order of the logical (depth, height, width) volume.
 *
 * data (channels, depth, height, width) fp32, element strides for channel, z and y, unit stride along x; seg (depth, height, width)
 * contiguous, float32 / uint8 / int16 by seg_dtype (SEGM_PREP_SEG_NONE is refused: SEGM_E_DTYPE).  A voxel is foreground where
 * seg > 0; a NaN is not.  The three entries share the workspace: segm_fg_count fills it, the other two read what it left there,
 * on the same stream and for the same data, seg and shape.
 * Limits (SEGM_E_SHAPE, nothing is launched): channels in [1, SEGM_PREP_MAX_CHANNELS]; fewer than 2^31 voxels per channel;
 * stride_y >= width.  Workspace NULL, misaligned (8 bytes) or smaller than segm_fg_workspace_bytes: SEGM_E_WORKSPACE.
 * Workspace: per segment of SEGM_FG_SEGMENT voxels an int64 offset and one double per channel, and 96 KB of histograms per
 * channel - 0.5 MB for one channel of 400 x 512 x 512.
 * Integer atomics only, sums in a fixed order: two calls of every entry are bit-equal.
 * ------------------------------------------------------------------------------------------------ */
#define SEGM_FG_SEGMENT 4096
#define SEGM_FG_MAX_RANKS 8
#define SEGM_FG_MAX_INDICES (1 << 24)

typedef struct segm_fg_args {
    int32_t channels, depth, height, width;
    int32_t seg_dtype, n_ranks;
    int64_t stride_c, stride_z, stride_y;
    const float* data;
    const void* seg;
    int64_t n;                     /* order_stats, gather: the foreground count segm_fg_count reported (>= 1) */
    int64_t ranks[SEGM_FG_MAX_RANKS];   /* order_stats */
    const int64_t* idx;            /* gather: device memory */
    int64_t n_idx, idx_stride_c;
    int64_t* count;                /* count: 1 int64 in device memory */
    double* sums;                  /* count: SEGM_PREP_MAX_CHANNELS doubles in device memory */
    float* out;                    /* order_stats: channels x SEGM_FG_MAX_RANKS floats; gather: channels x n_idx floats */
    void* workspace;     size_t workspace_bytes;
    void* stream;
} segm_fg_args;
size_t segm_fg_workspace_bytes(int32_t channels, int64_t voxels);

/* One pass over the seg (and over the data where the seg is > 0): per segment of SEGM_FG_SEGMENT consecutive logical voxels the
 * number of foreground voxels (:431), then by one workgroup the exclusive int64 offsets of the segments (kept in the workspace),
 *   count[0] = n, the number of foreground voxels                                               (len(foreground_pixels), :435)
 *   sums[c]  = the fp64 sum of channel c's foreground values, c < channels                     (np.mean's numerator, :442)
 * The sums are per-workgroup partials added in a fixed order by one workgroup, as in segm_crop_stats: no floating-point atomics. */
int segm_fg_count(const segm_fg_args* args);

/* out[c * SEGM_FG_MAX_RANKS + r] = the ranks[r]-th smallest foreground value of channel c (0-based; np.sort(images[c][mask])[k]),
 * for n_ranks in [1, SEGM_FG_MAX_RANKS] ranks in [0, n), repeats allowed (SEGM_E_SHAPE otherwise) - what np.min, np.max, np.median
 * and np.percentile (:443-447) partition the n values for.  Radix selection on the order-preserving 32-bit key of the float bits,
 * digits of 12 + 10 + 10 bits: three histogram passes over the data for all ranks and channels together, a one-workgroup kernel
 * after each turns every rank into a longer prefix and a residual rank; nothing is read back in between.  -0.0 and +0.0 are equal
 * values, either may be returned.  NaN among the foreground values is outside the contract (the reference asserts there is none, :422). */
int segm_fg_order_stats(const segm_fg_args* args);

/* out[c * n_idx + j] = channel c at the foreground voxel of rank i in C order, what images[c][mask][i] gives (:434, :440), with
 * i = idx[j] for every channel (idx_stride_c = 0) or i = idx[c * idx_stride_c + j] (idx_stride_c >= n_idx: a draw per channel).
 * idx: n_idx in [1, SEGM_FG_MAX_INDICES] int64 in device memory, unsorted, repeats allowed, each in [0, n).  An index outside
 * [0, n) reads nothing and gives NaN: a caller that holds the indices on the host checks them there. */
int segm_fg_gather(const segm_fg_args* args);

/* ------------------------------------------------------------------------------------------------
 * The top-k ("hard example") cross entropy (additive to ABI 10; csrc/topk_ce.hip).
 * Replaces the reference's TopKLoss (light_training/loss/robust_ce_loss.py:19-32) and its backward:
 *   `nn.CrossEntropyLoss(reduce=False)(inp, target)` (:29)                   -> segm_cross_entropy_map
 *   `torch.topk(res.view((-1, )), int(num_voxels * k / 100), sorted=False)` (:31), `res.mean()` (:32)
 *                                                                             -> segm_topk_select, the mean is arithmetic on its result
 *   the backward of the three                                                 -> segm_cross_entropy_map_bwd
 *
 * logits, dlogits: (batch, classes, spatial) contiguous, one dtype (fp32 / fp16 / bf16; arithmetic in fp32), classes <= 16; labels
 * (batch, spatial) int64; batch * spatial < 2^31 (SEGM_E_SHAPE otherwise).  NULL where a pointer is required: SEGM_E_NULL.
 * Integer atomics only, sums in a fixed order: two calls of every entry are bit-equal.
 * ------------------------------------------------------------------------------------------------ */
#define SEGM_TOPK_RESULT_BYTES 32

typedef struct segm_cross_entropy_map_args {
    int32_t batch, classes, dtype, reserved;
    int64_t spatial, ignore_index;
    const void* logits;
    const int64_t* labels;
    float* loss_map;               /* map: out, (batch, spatial) fp32.  bwd: in, with `select` (both or neither) */
    void* dlogits;                 /* bwd: out */
    const float* coef;             /* bwd, optional: (batch, spatial) fp32, the upstream gradient of the map */
    const float* scale;            /* bwd, optional: one fp32 in device memory, the upstream gradient of a reduced loss */
    const void* select;            /* bwd, optional: the SEGM_TOPK_RESULT_BYTES segm_topk_select wrote for loss_map and kk */
    int64_t kk;                    /* bwd with select: in [1, batch * spatial] */
    void* stream;
} segm_cross_entropy_map_args;

/* loss_map[b, s] = logsumexp_c(x[b, :, s]) - x[b, label, s]; 0 where label == ignore_index; NaN where the label is outside
 * [0, classes) and not ignored (segm_cross_entropy's rule: wrong labels stay loud).  One thread per voxel. */
int segm_cross_entropy_map(const segm_cross_entropy_map_args* args);

/* dlogits[b, c, s] = g (softmax_c(x)[c] - [c == label]); 0 where the label is ignored; NaN where it is wrong.  g is the product of
 * whichever are given: coef[b, s]; scale[0]; the top-k weight of loss_map[b, s] - 1 / kk where its key is above the threshold's,
 * (kk - n_gt) / (n_eq kk) where it is equal (the tied voxels share what is left of the kk), 0 below.  The softmax is recomputed. */
int segm_cross_entropy_map_bwd(const segm_cross_entropy_map_args* args);

/* result (SEGM_TOPK_RESULT_BYTES of device memory, 8-byte aligned, overwritten):
 *   { float threshold; int32 pad; int64 n_gt; int64 n_eq; double sum_gt }
 * threshold = the kk-th largest of the n values under the order of the 32-bit key of csrc/radix_hist.h (the float order; -0.0 below
 * +0.0; a positive NaN above +inf); n_gt, n_eq = the number of keys greater than / equal to the threshold's; sum_gt = the fp64 sum of
 * the values counted in n_gt (per-workgroup partials added by one workgroup in a fixed order).  The mean of the kk largest is
 * (sum_gt + (kk - n_gt) threshold) / kk.  Radix selection, digits of 12 + 10 + 10 bits: a histogram pass over the values and a
 * one-workgroup kernel per digit, a last pass for the counts and the sum; nothing is read back.
 * values: n fp32, 1 <= n < 2^31; kk in [1, n] (SEGM_E_SHAPE otherwise).  Workspace NULL, misaligned (8 bytes) or smaller than
 * segm_topk_select_workspace_bytes(n) (0 for an n out of range): SEGM_E_WORKSPACE. */
typedef struct segm_topk_select_args {
    const float* values;
    int64_t n, kk;
    void* result;
    void* workspace;     size_t workspace_bytes;
    void* stream;
} segm_topk_select_args;
size_t segm_topk_select_workspace_bytes(int64_t n);
int segm_topk_select(const segm_topk_select_args* args);

/* ------------------------------------------------------------------------------------------------
 * The region-based loss: sigmoid Dice + BCE sums and their gradient (additive to ABI 10; csrc/region_loss.hip).
 * Replaces what the reference's DC_and_BCE_loss (light_training/loss/compound_losses.py:84-100) and its Dice classes
 * (light_training/loss/dice.py:72-113) run over the volume: the sigmoid, the products with the one-hot region target and the loss
 * mask, the reductions over the spatial axes, BCEWithLogitsLoss, and the backward of all of them.  What follows the sums is
 * arithmetic on (batch, regions) tensors and stays with the caller.
 *
 * With p = sigmoid(x), the region target t(b, r, v) and the validity m(b, v), per (b, r)
 *     I = sum_v m p t     P = sum_v m p     G = sum_v m t     E = sum_v m (max(x, 0) - x t + log1p(exp(-|x|)))
 * and per b the count N = sum_v m.
 *
 * logits: (batch, regions, depth, height, width), regions in [1, SEGM_REGION_MAX_REGIONS], fp32 / fp16 / bf16 (arithmetic in
 * fp32), element strides for batch, region, z and y, stride_x == 1 (SEGM_E_SHAPE otherwise), aligned to its element size;
 * depth * height * width < 2^31.  A caller with fewer spatial axes passes 1 for the missing ones.
 * target, dense, by target_kind:
 *   SEGM_REGION_LABELS_*: a label map (batch, depth, height, width); t = (masks[r] >> label) & 1.  With has_ignore a label equal
 *     to ignore_label (any value; compared before the range check) has m = 0.  Any other label outside [0, 32), or a float label
 *     that is no integer, puts NaN into that sample's I, P and E (a wrong label stays loud) and into its voxel of dlogits.
 *   SEGM_REGION_PLANES_*: (batch, regions + ignore_plane, depth, height, width), the values used as they are (soft targets
 *     work); with ignore_plane = 1 the last plane L gives m = ((1 - L) != 0), the reference's use_ignore_label (:87).
 * Per-workgroup partial rows in the workspace, added by one workgroup per sample in a fixed order, all in fp64; no floating-point
 * atomic: two calls on the same tensors are bit-equal.  The aligned route (16-byte packets of logits) and the per-voxel route
 * compute every voxel's terms alike but add them in another order: no bit-equality between differently aligned views.
 * ------------------------------------------------------------------------------------------------ */
#define SEGM_REGION_MAX_REGIONS 8
enum segm_region_target {
    SEGM_REGION_LABELS_I64 = 0, SEGM_REGION_LABELS_I16 = 1, SEGM_REGION_LABELS_U8 = 2, SEGM_REGION_LABELS_F32 = 3,
    SEGM_REGION_PLANES_U8 = 4, SEGM_REGION_PLANES_F32 = 5
};

typedef struct segm_region_loss_args {
    int32_t batch, regions, dtype, target_kind;
    int32_t depth, height, width;
    int32_t ignore_plane;          /* planes: 1 if the target has regions + 1 planes; labels: must be 0 */
    int32_t has_ignore, reserved;  /* labels: whether ignore_label counts */
    int64_t ignore_label;
    int64_t stride_b, stride_r, stride_z, stride_y, stride_x;      /* of logits, in elements; stride_x must be 1 */
    uint32_t masks[SEGM_REGION_MAX_REGIONS];                       /* labels: bit l of masks[r] = label l belongs to region r */
    const void* logits;
    const void* target;
    double* sums;                  /* fwd: out, fp64 [I (batch, regions) | P | G | E | N (batch)], 4 batch regions + batch values */
    const float* g_i;              /* bwd: (batch, regions) fp32, dense, in device memory: d loss / d I, / d P, / d E */
    const float* g_p;
    const float* g_e;
    void* dlogits;                 /* bwd: out, (batch, regions, depth, height, width) dense, the logits' dtype */
    void* workspace;     size_t workspace_bytes;                    /* fwd only */
    void* stream;
} segm_region_loss_args;

/* 0 for a shape out of range.  Workspace NULL, misaligned (8 bytes) or smaller than this: SEGM_E_WORKSPACE. */
size_t segm_region_loss_workspace_bytes(int32_t batch, int32_t regions, int64_t voxels);

/* The five sums (compound_losses.py:84-100 and dice.py:72-113 up to the sums).  Two launches, nothing is read back. */
int segm_region_loss_fwd(const segm_region_loss_args* args);

/* dlogits = m (p (1 - p) (g_i t + g_p) + g_e (p - t)), exactly 0 where m = 0; the sigmoid is recomputed (the backward of
 * compound_losses.py:84-100 and dice.py:72-113 given the gradients of the loss by the sums).  One launch, nothing is read back. */
int segm_region_loss_bwd(const segm_region_loss_args* args);

/* ------------------------------------------------------------------------------------------------
 * Softmax Dice + cross entropy: the sums behind nnU-Net's default loss and their gradient (additive to ABI 10; csrc/dice_ce.hip).
 * Replaces what the reference's Dice classes (light_training/loss/dice.py:9-116) and DC_and_CE_loss
 * (light_training/loss/compound_losses.py:8-57) run over the volume: the softmax, the one-hot target, the products with it and with
 * the loss mask, the reductions over the spatial axes, RobustCrossEntropyLoss, and the backward of all of them.  What follows the
 * sums (batch_dice, do_bg, smooth, clip_tp, the means, the weights) is arithmetic on (batch, classes) tensors and stays with the
 * caller.
 *
 * With p = softmax_c(x), the label y(b, v) and the validity m(b, v), per (b, c)
 *     I = sum_v m p_c [y = c]     P = sum_v m p_c     G = sum_v m [y = c]
 * and per b     CE = sum_v m (logsumexp_c(x) - x_y)     N = sum_v m.
 *
 * logits: (batch, classes, depth, height, width), classes in [1, SEGM_SOFTMAX_DICE_MAX_CLASSES] (the limit of
 * segm_cross_entropy_map), fp32 / fp16 / bf16 (arithmetic in fp32, every term added in fp64), element strides for batch, class, z
 * and y, stride_x == 1 (SEGM_E_SHAPE otherwise), aligned to its element size; depth * height * width < 2^31.  A caller with fewer
 * spatial axes passes 1 for the missing ones.
 * labels: (batch, depth, height, width), dense, label_kind one of SEGM_REGION_LABELS_I64 / _I16 / _U8 / _F32.  With has_ignore a
 * label equal to ignore_label (any value; compared before the range check) has m = 0.  mask: optional, uint8, dense, the labels'
 * shape; m = 0 where it is 0.  A label with m = 1 outside [0, classes), or a float label that is no integer (NaN included), puts NaN
 * into that sample's I, P and CE (a wrong label stays loud) and into its voxel of dlogits; the other samples stay finite.
 * G and N are exact; I is exactly 0 for a class that never occurs.
 * Per-workgroup partial rows in the workspace, added by one workgroup per sample in a fixed order, all in fp64; no floating-point
 * atomic: two calls on the same tensors are bit-equal.  The aligned route (16-byte packets of logits) and the per-voxel route
 * compute every voxel's terms alike but add them in another order: no bit-equality between differently aligned views.
 * ------------------------------------------------------------------------------------------------ */
#define SEGM_SOFTMAX_DICE_MAX_CLASSES 16

typedef struct segm_softmax_dice_args {
    int32_t batch, classes, dtype, label_kind;
    int32_t depth, height, width;
    int32_t has_ignore;            /* whether ignore_label counts */
    int64_t ignore_label;
    int64_t stride_b, stride_c, stride_z, stride_y, stride_x;      /* of logits, in elements; stride_x must be 1 */
    const void* logits;
    const void* labels;
    const uint8_t* mask;           /* optional */
    double* sums;                  /* fwd: out, fp64 [I (batch, classes) | P | G | CE (batch) | N (batch)] */
    const float* g_i;              /* bwd: (batch, classes) fp32, dense, in device memory: d loss / d I, / d P */
    const float* g_p;
    const float* g_ce;             /* bwd: (batch) fp32: d loss / d CE */
    void* dlogits;                 /* bwd: out, (batch, classes, depth, height, width) dense, the logits' dtype */
    void* workspace;     size_t workspace_bytes;                    /* fwd only */
    void* stream;
} segm_softmax_dice_args;

/* 0 for a shape out of range.  Workspace NULL, misaligned (8 bytes) or smaller than this: SEGM_E_WORKSPACE. */
size_t segm_softmax_dice_workspace_bytes(int32_t batch, int32_t classes, int64_t voxels);

/* The five sums (dice.py:9-116 and compound_losses.py:8-57 up to the sums).  Two launches - the streaming kernel and a
 * one-workgroup-per-sample kernel that adds the partial rows - nothing is read back. */
int segm_softmax_dice_fwd(const segm_softmax_dice_args* args);

/* dlogits_j = m (p_j (a_j - S) + g_ce (p_j - [j = y])) with a_c = g_i[c] [y = c] + g_p[c] and S = sum_c p_c a_c; exactly 0 where
 * m = 0; the softmax is recomputed (the backward of dice.py:9-116 and compound_losses.py:8-57 given the gradients of the loss by the
 * sums).  One launch, nothing is read back. */
int segm_softmax_dice_bwd(const segm_softmax_dice_args* args);

/* ------------------------------------------------------------------------------------------------
 * Resampling a case to the target spacing (additive to ABI 10; csrc/resample.hip).
 * Replaces the reference's resample_data_or_seg without a separate z axis (light_training/preprocessing/resampling/
 * default_resampling.py:126-217 as default_preprocessor.py:187-201 calls it): skimage's resize(order 3 or 1, mode='edge',
 * anti_aliasing=False, clip=True) for the data - for n-D input scipy.ndimage.zoom(mode='nearest', grid_mode=True) - and
 * batchgenerators' resize_segmentation(order 1) for the seg.  Its separate-z branch (:154-207; every slice resized in its plane, the
 * nearest slice along the coarse axis) is segm_zoom_slices / segm_zoom_labels_slices below, for order_z = 0; order_z > 0 is not
 * covered.  Non-finite input values are outside the contract.
 * ------------------------------------------------------------------------------------------------ */
#define SEGM_ZOOM_MAX_SIDE 2048

/* data (channels, depth, height, width) fp32, element strides for channel, z and y, unit stride along x ->
 * out (channels, out_depth, out_height, out_width) fp32, dense.  Output voxel i of an axis samples the input at
 * (i + 0.5) * (n_in / n_out) - 0.5.
 *   order 3: cubic B-spline.  Per axis the line is padded by 12 edge copies, multiplied by 6 and run through the causal and
 *            anti-causal recursion with the pole sqrt(3) - 2 under mirror boundary conditions (scipy's spline_filter on the padded
 *            array); the coefficients are kept in fp64 in the workspace, the 64 taps of an output are summed in fp64.
 *   order 1: trilinear, the coordinate clamped to [0, n_in - 1]; fp64 arithmetic on the fp32 input.
 * clip = 1 clamps every channel to the minimum and maximum of its own input, found on the device (skimage's clip=True); then the
 * result is rounded to fp32.  Sums have a fixed order and there are no floating-point atomics: two calls are bit-equal.
 * Limits (SEGM_E_SHAPE, nothing is launched): channels in [1, SEGM_PREP_MAX_CHANNELS]; every side, in and out, in
 * [1, SEGM_ZOOM_MAX_SIDE]; fewer than 2^31 voxels per channel, in and out; order 1 or 3; clip 0 or 1.
 * Workspace: 256 bytes, and for order 3 channels * (depth + 4) * (height + 4) * (width + 4) doubles behind them. */
typedef struct segm_zoom_args {
    int32_t channels, depth, height, width;
    int32_t out_depth, out_height, out_width;
    int32_t order, clip, reserved;
    int64_t stride_c, stride_z, stride_y;
    const float* data;
    float* out;
    void* workspace;     size_t workspace_bytes;
    void* stream;
} segm_zoom_args;
size_t segm_zoom_workspace_bytes(int32_t channels, int32_t depth, int32_t height, int32_t width, int32_t order);
int segm_zoom(const segm_zoom_args* args);

/* seg (depth, height, width) int16, contiguous (what segm_crop_normalize writes: labels >= -1) -> out (out_depth, out_height,
 * out_width) int16.  Per output voxel the trilinear weights of its 8 corners (coordinates as order 1 above, fp64) are summed per
 * distinct corner label; the largest label whose sum is >= 0.5 wins, 0 if there is none - resize_segmentation's
 * `out[resize(seg == c) >= 0.5] = c` over the labels in ascending order.  Label -1 takes part like any other.
 * counts[SEGM_PREP_COUNT_BINS] int64, OVERWRITTEN (optional): the labels of `out` in segm_crop_normalize's layout ([258] and [259] 0).
 * Limits as for segm_zoom. */
typedef struct segm_zoom_labels_args {
    int32_t depth, height, width;
    int32_t out_depth, out_height, out_width;
    const int16_t* seg;
    int16_t* out;
    int64_t* counts;
    void* stream;
} segm_zoom_labels_args;
int segm_zoom_labels(const segm_zoom_labels_args* args);

/* The separate-z branch of resample_data_or_seg (default_resampling.py:154-207) with order_z = 0: every slice is resized in its own
 * plane, and output slice k is the resized input slice source[k] - the nearest slice, which the caller computes as
 * clip(floor((n_in / n_out) * (k + 0.5) - 0.5 + 0.5), 0, n_in - 1) in float64 (scipy's map_coordinates(order=0, mode='nearest')).
 * data (channels, slices, height, width) fp32, the slice axis outermost: element strides for channel, slice and y, unit stride along
 * x -> out (channels, out_slices, out_height, out_width) fp32, dense.  source: out_slices int32 on the device; the kernel clamps
 * them to [0, slices), so no table reads outside the input.
 *   order 3: the prefilter of segm_zoom along x and y only - fp64 coefficients (channels, slices, height + 4, width + 4), no pass and
 *            no margin along the slice axis - and 16 taps per output voxel; order 1: four taps of the fp32 input.
 * clip = 1 clamps every output slice to the minimum and maximum of ITS SOURCE SLICE (skimage's clip=True on a 2-D resize), not of
 * the channel; then the result is rounded to fp32.  Where out_height == height and out_width == width the slices are copied as they
 * are (the reference's factor-1 resize reproduces them only up to fp64 rounding).  Several outputs that share a source slice are
 * each computed.  Fixed summation orders, no floating-point atomics: two calls are bit-equal.
 * Limits (SEGM_E_SHAPE, nothing is launched): as for segm_zoom, the slice axis counting as a side.
 * Workspace: 2 * channels * slices 32-bit keys rounded up to 256 bytes, and - for order 3 with a changed in-plane shape - the
 * coefficients behind them. */
typedef struct segm_zoom_slices_args {
    int32_t channels, slices, height, width;
    int32_t out_slices, out_height, out_width;
    int32_t order, clip, reserved;
    int64_t stride_c, stride_s, stride_y;
    const float* data;
    const int32_t* source;
    float* out;
    void* workspace;     size_t workspace_bytes;
    void* stream;
} segm_zoom_slices_args;
size_t segm_zoom_slices_workspace_bytes(int32_t channels, int32_t slices, int32_t height, int32_t width, int32_t out_height,
                                        int32_t out_width, int32_t order);
int segm_zoom_slices(const segm_zoom_slices_args* args);

/* The same branch for a seg: seg (slices, height, width) int16, contiguous -> out (out_slices, out_height, out_width) int16.  Per
 * output voxel the bilinear weights of its 4 corners in slice source[k] (clamped as above) are summed in fp64 per distinct corner
 * label; the largest label whose sum is >= 0.5 wins, 0 if there is none (resize_segmentation(slice, shape, 1)).  Label -1 takes part
 * like any other.  counts as for segm_zoom_labels (optional, OVERWRITTEN).  Limits as for segm_zoom_slices. */
typedef struct segm_zoom_labels_slices_args {
    int32_t slices, height, width;
    int32_t out_slices, out_height, out_width;
    const int16_t* seg;
    const int32_t* source;
    int16_t* out;
    int64_t* counts;
    void* stream;
} segm_zoom_labels_slices_args;
int segm_zoom_labels_slices(const segm_zoom_labels_slices_args* args);


/* ------------------------------------------------------------------------------------------------
 * Training augmentation at the reference's interpolation orders (additive to ABI 10; csrc/augment.hip).
 * The stencil / gather transforms of the reference's get_train_transforms (light_training/augment/train_augment.py:29-50) as
 * batchgenerators runs them through scipy: SpatialTransform with order_data=3 / order_seg=1, SimulateLowResolution's nearest
 * down-sampling, GaussianBlur.  A launch takes a batch (samples, channels, depth, height, width) fp32 with element strides for
 * sample, channel, z and y and unit stride along x; at most SEGM_AUG_MAX_SAMPLES samples and SEGM_PREP_MAX_CHANNELS channels; every
 * side in [1, SEGM_ZOOM_MAX_SIDE]; fewer than 2^31 voxels per volume.  Matrices, sigmas and on / off flags travel by value in the
 * argument structs: no call copies anything to the device.  Sums have a fixed order and there are no floating-point atomics: two
 * calls are bit-equal.  Non-finite input values are outside the contract.
 * ------------------------------------------------------------------------------------------------ */
#define SEGM_AUG_MAX_SAMPLES 8
#define SEGM_AUG_MAX_VOLUMES (SEGM_AUG_MAX_SAMPLES * SEGM_PREP_MAX_CHANNELS)
#define SEGM_BLUR_MAX_RADIUS 4

/* Cubic B-spline coefficients of every volume of the samples whose `on` flag is set, fp64, into the dense workspace
 * (samples, channels, depth, height, width): scipy.ndimage.spline_filter(x, 3, output=float64, mode='mirror'), which is what
 * map_coordinates(order=3, mode='constant') filters with - gain 6, the causal and the anti-causal recursion with the pole
 * sqrt(3) - 2 under mirror boundary conditions on the bare line, axes of length 1 left alone.  Volumes of samples that are off
 * are not written.  Workspace: samples * channels * depth * height * width doubles. */
typedef struct segm_spline_coefs_args {
    int32_t samples, channels, depth, height, width, reserved;
    int64_t stride_n, stride_c, stride_z, stride_y;
    uint8_t on[SEGM_AUG_MAX_SAMPLES];
    const float* data;
    void* workspace;     size_t workspace_bytes;
    void* stream;
} segm_spline_coefs_args;
size_t segm_spline_coefs_workspace_bytes(int32_t samples, int32_t channels, int32_t depth, int32_t height, int32_t width);
int segm_spline_coefs(const segm_spline_coefs_args* args);

/* out (samples, channels, depth, height, width) fp32, dense.  Output voxel (z, y, x) of sample n samples the input at
 * p = A_n (z, y, x)^T + t_n, matrix[n] = the rows [A | t] of a 3 x 4 fp64 matrix.  If a component of p is < 0 or > side - 1 the
 * output is cval; otherwise the 64 taps of the cubic B-spline around p are gathered from `coefs` (what segm_spline_coefs wrote),
 * tap indices outside the line mirrored, summed in fp64 and rounded once to fp32 - batchgenerators' interpolate_img:
 * map_coordinates(x.astype(float64), p, order=3, mode='constant', cval).astype(float32).  Every channel of a sample shares the
 * sample's coordinates.  Samples that are off are copied from `data` bit for bit (their coefficients are not read). */
typedef struct segm_affine_spline3_args {
    int32_t samples, channels, depth, height, width, reserved;
    int64_t stride_n, stride_c, stride_z, stride_y;      /* of data */
    double matrix[SEGM_AUG_MAX_SAMPLES][12];
    float cval;          int32_t reserved2;
    uint8_t on[SEGM_AUG_MAX_SAMPLES];
    const float* data;
    const double* coefs;
    float* out;
    void* stream;
} segm_affine_spline3_args;
int segm_affine_spline3(const segm_affine_spline3_args* args);

/* seg, out (samples, depth, height, width) int16 (wide = 0) or int64 (wide = 1), dense; matrices as above.  Outside the volume the
 * output is 0; inside, the trilinear weights of the 8 corners are summed per distinct corner label in fp64 and the largest label
 * whose sum is >= 0.5 wins, 0 if none does - batchgenerators' interpolate_img(is_seg=True, order=1, cval=-1):
 * result[map_coordinates(seg == c, order=1, mode='constant', cval=-1) >= 0.5] = c over the labels in ascending order, on zeros.
 * Samples that are off are copied. */
typedef struct segm_affine_labels_args {
    int32_t samples, depth, height, width, wide, reserved;
    double matrix[SEGM_AUG_MAX_SAMPLES][12];
    uint8_t on[SEGM_AUG_MAX_SAMPLES];
    const void* seg;
    void* out;
    void* stream;
} segm_affine_labels_args;
int segm_affine_labels(const segm_affine_labels_args* args);

/* Order-0 zoom: data (channels, depth, height, width) fp32 (strides as segm_zoom) -> out (channels, out_depth, out_height,
 * out_width), dense - scipy.ndimage.zoom(order=0, mode='nearest', grid_mode=True), skimage's resize(order=0, mode='edge',
 * anti_aliasing=False) as SimulateLowResolutionTransform calls it.  Per axis output i takes input
 * clamp(floor((i + 0.5) * (n_in / n_out) - 0.5 + 0.5), 0, n_in - 1), in fp64. */
typedef struct segm_zoom_nearest_args {
    int32_t channels, depth, height, width;
    int32_t out_depth, out_height, out_width, reserved;
    int64_t stride_c, stride_z, stride_y;
    const float* data;
    float* out;
    void* stream;
} segm_zoom_nearest_args;
int segm_zoom_nearest(const segm_zoom_nearest_args* args);

/* scipy.ndimage.gaussian_filter(x_fp32, sigma) of every volume whose `on` flag is set (volume v = sample * channels + channel):
 * radius int(4 sigma + 0.5) <= SEGM_BLUR_MAX_RADIUS, weights exp(-0.5 (t / sigma)^2) normalised in fp64, boundary 'reflect'
 * (d c b a | a b c d), the axes in the order z, y, x, each pass summed in fp64 (centre first, then the pairs from the outermost
 * inwards, as scipy's symmetric correlate1d) and rounded to fp32.  Volumes that are off are copied to `out` and take no part in the
 * second and third pass.  out (samples, channels, depth, height, width) fp32, dense; workspace: as many bytes as `out`. */
typedef struct segm_gauss_blur_args {
    int32_t samples, channels, depth, height, width, reserved;
    int64_t stride_n, stride_c, stride_z, stride_y;
    double sigma[SEGM_AUG_MAX_VOLUMES];
    uint8_t on[SEGM_AUG_MAX_VOLUMES];
    const float* data;
    float* out;
    void* workspace;     size_t workspace_bytes;
    void* stream;
} segm_gauss_blur_args;
int segm_gauss_blur(const segm_gauss_blur_args* args);


/* ------------------------------------------------------------------------------------------------
 * Intensity augmentation (additive to ABI 10; csrc/intensity.hip): noise, brightness, contrast, the two gammas and the mirror of
 * the reference's get_train_transforms (light_training/augment/train_augment.py:40-60) as streaming passes, in place of the
 * per-sample ATen arithmetic of SplineAugmenter (segmamba_amd/augment.py:333-363).
 * A launch works on up to SEGM_AUG_MAX_VOLUMES planes; plane v = sample * channels + channel of a (samples, channels, depth, height,
 * width) fp32 tensor with element strides for sample, channel, z and y, a unit stride along x and any storage offset.  Every plane
 * carries its own op and parameters by value (all fp32), so one launch serves planes with different transforms on.  With v the
 * input voxel and every statistic taken over the plane's voxels:
 *   SEGM_INTENSITY_OFF       nothing: skipped in place, copied bit for bit out of place (the mirror of a plane with no op on)
 *   SEGM_INTENSITY_NOISE     y = v + fl32(a * n), n the voxel of the plane noise[v] (dense)          augment.py:336
 *   SEGM_INTENSITY_SCALE     y = fl32(v * a)                                                          augment.py:342
 *   SEGM_INTENSITY_CONTRAST  u = fl32(v * a); mean, lo, hi of u; y = min(max((u - mean) * b + mean, lo), hi)   augment.py:342-348
 *   SEGM_INTENSITY_GAMMA     t = invert ? -v : v; mean0, sd0, lo, hi of t, rng = hi - lo;
 *                            w = max((t - lo) / (rng + 1e-7), 0) ^ a * rng + lo; mean1, sd1 of w;
 *                            y = +-((w - mean1) / (sd1 + 1e-8) * sd0 + mean0)                         augment.py:305-315, 354
 * sd is the population standard deviation (numpy.std, what the published transform uses).
 * A statistics row is SEGM_INTENSITY_STATS_DOUBLES fp64: count, mean, sd, min, max, then zeros.  Rows are written by
 * segm_intensity_stats and read by later launches from device memory: nothing is read back to the host.  Sums are taken about the
 * plane's first value in fp64 (thread, wave shuffles, LDS, one row of partials per workgroup, a finish kernel that adds the rows in a
 * fixed order), min and max are exact, there are no floating-point atomics: two calls are bit-equal.
 * Refused with nothing launched: samples * channels outside [1, SEGM_AUG_MAX_VOLUMES], a side < 1, 2^31 voxels per plane or more,
 * stride_x != 1, a negative stride or stride_y < width (SEGM_E_SHAPE); an unknown op (SEGM_E_DTYPE); a required pointer that is
 * NULL (SEGM_E_NULL); a workspace that is NULL, misaligned (8 bytes) or smaller than segm_intensity_workspace_bytes
 * (SEGM_E_WORKSPACE); a mirror mask on an in-place call (SEGM_E_SHAPE).  Non-finite input values are outside the contract.
 * ------------------------------------------------------------------------------------------------ */
#define SEGM_INTENSITY_OFF 0
#define SEGM_INTENSITY_NOISE 1
#define SEGM_INTENSITY_SCALE 2
#define SEGM_INTENSITY_CONTRAST 3
#define SEGM_INTENSITY_GAMMA 4
#define SEGM_INTENSITY_STATS_DOUBLES 8

typedef struct segm_intensity_args {
    int32_t samples, channels, depth, height, width;
    int32_t stage;                                        /* segm_intensity_stats: 0 or 1 */
    int64_t stride_n, stride_c, stride_z, stride_y, stride_x;              /* of data */
    int64_t out_stride_n, out_stride_c, out_stride_z, out_stride_y;        /* of out (unit stride along x) */
    uint8_t op[SEGM_AUG_MAX_VOLUMES];
    uint8_t invert[SEGM_AUG_MAX_VOLUMES];                 /* GAMMA on the negated plane */
    uint8_t mirror[SEGM_AUG_MAX_VOLUMES];                 /* bit 0: flip z, bit 1: flip y, bit 2: flip x; out of place only */
    float a[SEGM_AUG_MAX_VOLUMES];                        /* NOISE: scale; SCALE: factor; CONTRAST: pre-scale (1 = none); GAMMA: exponent */
    float b[SEGM_AUG_MAX_VOLUMES];                        /* CONTRAST: factor */
    const float* noise[SEGM_AUG_MAX_VOLUMES];             /* per NOISE plane: depth * height * width fp32, dense */
    const float* data;
    float* out;                                           /* segm_intensity_apply: NULL or == data: in place */
    double* stats;                                        /* (planes, SEGM_INTENSITY_STATS_DOUBLES): of u (CONTRAST) / of t (GAMMA) */
    double* stats2;                                       /* the same shape: of w (GAMMA) */
    void* workspace;     size_t workspace_bytes;          /* segm_intensity_stats */
    void* stream;
} segm_intensity_args;

/* 0 for a shape out of range */
size_t segm_intensity_workspace_bytes(int32_t planes, int64_t voxels);

/* stage 0: the rows `stats` of the CONTRAST planes (of u) and of the GAMMA planes (of t).  stage 1: the rows `stats2` of the GAMMA
 * planes (of w, formed from the rows `stats` by the function the apply pass uses).  Rows of other planes are not written.  One
 * streaming launch and one finish launch; none when no plane takes part. */
int segm_intensity_stats(const segm_intensity_args* args);

/* Every plane's op, in place (out NULL or == data; planes that are OFF are not touched) or out of place (every plane written, plane
 * v at its mirrored position: out[z', y', x'] with z' = depth - 1 - z where bit 0 of mirror[v] is set, and so on; out must not
 * overlap data).  CONTRAST reads its row of `stats`, GAMMA its rows of `stats` and `stats2`.  Where width, the strides in use and
 * the base pointers are multiples of 16 bytes a thread takes a packet of 4 voxels along x (an x-mirror reverses the packet and
 * stores it at the mirrored packet address), single voxels otherwise; both routes call the same per-voxel functions, and NOISE,
 * SCALE and OFF give the same bits on both. */
int segm_intensity_apply(const segm_intensity_args* args);


/* ------------------------------------------------------------------------------------------------
 * Stitching a sliding-window prediction (additive to ABI 10; csrc/stitch.hip): the window gather, the count map, the weighted
 * blending and the close of a mirror pass, in place of the ATen chain around the network in segmamba_amd/predictor.py - the
 * reference's monai/inferers/utils.py sliding_window_inference (pad, slice + cat, cast, multiply, slice-add, divide, crop) and the
 * mirror loop of light_training/prediction.py:110-159 (torch.flip of the input and of every result, the running sum, the mean).
 * Geometry, as sliding_window_inference defines it: the volume (batch, channels, size z, y, x) fp32; per axis
 * image = max(size, roi) and pad0 = (image - size) / 2 (the volume is centred in the padded frame, the odd voxel behind it); a
 * window is (sample, start z, y, x) with 0 <= start <= image - roi in the padded frame.  mirror: bit 0 flips z, bit 1 flips y,
 * bit 2 flips x - the convention of segm_intensity_args.  The flip and the padding are folded into the index: neither a mirrored
 * nor a padded copy exists.  A launch carries 1 .. SEGM_STITCH_MAX_WINDOWS windows by value; a caller with more splits the list
 * and keeps its order.
 *   segm_window_gather   windows_out (n_windows, channels, roi) fp32 dense.  Window voxel i along an axis has the padded-frame
 *                        coordinate q = start + i and u = q - pad0: cval where u is outside [0, size), otherwise the volume at
 *                        size - 1 - u (flipped axis) or u.  The volume has element strides for sample, channel, z and y and a unit
 *                        stride along x.
 *   segm_window_count    count (image) fp32 from weight (roi) fp32 dense and the start lists of the three axes: per voxel the
 *                        weights of the covering windows added in the order of the lists' product (z outermost, x fastest), from 0 -
 *                        the bits of the loop `count[slice] += weight`.
 *   segm_window_blend    acc[sample, :, start + i] += fl32(float(pred[n, :, i]) * weight[i]) for the windows of the launch; acc
 *                        (batch, channels, image) fp32 dense, pred (n_windows, channels, roi) dense in `dtype`.  The product is
 *                        rounded on its own; the additions to one voxel happen in window order; every voxel of acc has one writer
 *                        (a thread takes voxels of acc and walks the windows that cover them), no atomics.
 *   segm_window_finish   closes pass `pass` of `passes`: for every voxel v of total (batch, channels, size) fp32 dense, with
 *                        p = pad0 + (flipped ? size - 1 - v : v) and q = acc[p] / count[p] (fp32, correctly rounded):
 *                        total = q for pass 0, total + q later; the last pass then divides by `passes`.  acc is all zero afterwards
 *                        (the kernel stores zeros where it has read; the border of a padded image, which it does not read, is
 *                        zeroed by a memset on the same stream).  passes = 1, mirror = 0: acc / count without the centring padding.
 * A thread takes four voxels along x: as one packet of 16 bytes where they are whole and aligned, voxel by voxel otherwise; an
 * x-flip reverses the packet; both routes call the same per-voxel function.  No floating-point atomics: two calls are bit-equal.
 * Refused with nothing launched: n_windows outside [1, SEGM_STITCH_MAX_WINDOWS], a start list outside [1, SEGM_STITCH_MAX_STARTS],
 * batch, channels or a side < 1, 2^31 voxels per image plane or more, n_windows * channels (blend, finish: batch * channels) > 65535, a
 * window or a start that leaves the image, a sample outside [0, batch), stride_x != 1, a negative stride, a mirror outside 0 .. 7,
 * pass outside [0, passes), a pointer not aligned to its element (SEGM_E_SHAPE); an unknown dtype (SEGM_E_DTYPE); a required
 * pointer that is NULL (SEGM_E_NULL).
 * ------------------------------------------------------------------------------------------------ */
#define SEGM_STITCH_MAX_WINDOWS 64
#define SEGM_STITCH_MAX_STARTS 64

typedef struct segm_stitch_args {
    int32_t batch, channels;                              /* of volume (gather); of acc, pred and total (blend, finish) */
    int32_t size[3];                                      /* z, y, x of the volume / of total */
    int32_t roi[3];
    int32_t n_windows;                                    /* gather, blend */
    int32_t mirror;                                       /* gather, finish */
    int32_t dtype;                                        /* blend: of pred, SEGM_F32 / SEGM_F16 / SEGM_BF16 */
    int32_t pass, passes;                                 /* finish */
    float cval;                                           /* gather: the padding value */
    int32_t n_starts[3];                                  /* count */
    int32_t reserved;
    int32_t window[SEGM_STITCH_MAX_WINDOWS][4];           /* gather, blend: sample, start z, y, x */
    int32_t starts[3][SEGM_STITCH_MAX_STARTS];            /* count: the window starts of each axis, in order */
    int64_t stride_b, stride_c, stride_z, stride_y, stride_x;              /* gather: of volume */
    const float* volume;                                  /* gather */
    float* windows_out;                                   /* gather */
    const float* weight;                                  /* count, blend */
    float* count;                                         /* count: written; finish: read */
    const void* pred;                                     /* blend */
    float* acc;                                           /* blend: accumulated into; finish: read, then zeroed */
    float* total;                                         /* finish */
    void* stream;
} segm_stitch_args;

int segm_window_gather(const segm_stitch_args* args);
int segm_window_count(const segm_stitch_args* args);
int segm_window_blend(const segm_stitch_args* args);
int segm_window_finish(const segm_stitch_args* args);


/* ------------------------------------------------------------------------------------------------
 * Fused residual add + LayerNorm / RMSNorm over the last dimension, forward and backward (additive to ABI 10;
 * csrc/add_norm.hip).  Replaces the Triton kernels behind mamba_ssm/ops/triton/layernorm.py - _layer_norm_fwd
 * (layernorm.py:123-177) and _layer_norm_bwd (layernorm.py:293-377) - the native code of `layer_norm_fn`, `rms_norm_fn`,
 * `RMSNorm` and of `Block` with fused_add_norm (mamba_simple.py:445-501).
 * Operands: `rows` = M rows of `cols` = N elements, unit stride along a row, one row stride (in elements, >= N) per tensor.
 * x, y, dy, dx have `dtype`; residual, residual_out, dresidual, dresidual_in have `res_dtype`, which is `dtype` or SEGM_F32;
 * weight, bias, dweight, dbias are fp32 of N elements; mean, rstd fp32 of M elements.  `rms` != 0 selects the RMS form, which
 * has no mean (the pointer is not used).
 * Forward, all in fp32:
 *   s = float(x) + float(residual)                (s = float(x) without a residual)
 *   residual_out = round(s) to res_dtype          (when the pointer is given)
 *   LayerNorm: mean = sum(s) / N, var = sum((s - mean)^2) / N        RMS: mean = 0, var = sum(s^2) / N
 *   rstd = 1.0f / sqrtf(var + eps)                (IEEE square root and division)
 *   y = round((s - mean) * rstd * weight + bias) to dtype
 * The statistics come from the unrounded s, in two passes over the row, which stays in registers between them.
 * Backward, from mean, rstd and the saved row x_saved = residual_out (when that pointer is given: res_dtype) or x (dtype):
 *   xhat = (x_saved - mean) * rstd, wdy = weight * dy, c1 = sum(xhat * wdy) / N, c2 = sum(wdy) / N  (0 for RMS)
 *   dx = (wdy - (xhat * c1 + c2)) * rstd + float(dresidual)          (the last term when the pointer is given)
 *   dresidual_in = round(dx) to res_dtype (when the pointer is given); dx is rounded to dtype
 *   dweight[j] = sum over rows of dy * xhat, dbias[j] = sum over rows of dy (dbias may be NULL)
 * A workgroup walks a fixed share of the rows and leaves one fp32 partial row in the workspace; the partial rows are added in a
 * fixed order.  No floating-point atomics: two calls are bit-equal.  How a row is laid over lanes depends on N and dtype only, so
 * a row's y, residual_out, dx and dresidual_in do not depend on M or on the other rows.  A lane takes packets of 16 bytes of x
 * (4 fp32, 8 fp16 / bf16): whole packets where N is a multiple of the packet, every row stride in use too and every pointer in
 * use is 16-byte aligned; element by element otherwise.  Both routes keep the same elements in the same lanes and call the same
 * per-element functions: they give the same bits.
 * Refused with nothing launched: cols outside [1, SEGM_ADD_NORM_MAX_COLS], rows outside [1, 2^31), a row stride of a tensor in
 * use below cols, a pointer not aligned to its element (SEGM_E_SHAPE); an unknown dtype, a res_dtype that is neither dtype nor
 * SEGM_F32 (SEGM_E_DTYPE); a required pointer that is NULL (SEGM_E_NULL: forward x, y, weight, rstd, and mean unless rms;
 * backward dy, dx, weight, rstd, dweight, x or residual_out, and mean unless rms); backward only, a workspace that is NULL or
 * smaller than segm_add_norm_workspace_bytes (SEGM_E_WORKSPACE).  No host synchronisation, everything on `stream`.
 * ------------------------------------------------------------------------------------------------ */
#define SEGM_ADD_NORM_MAX_COLS 8192

typedef struct segm_add_norm_args {
    int64_t rows;
    int32_t cols, dtype, res_dtype, rms;
    float eps;
    int32_t reserved;
    const void* x;              int64_t x_stride;              /* forward; backward: x_saved when residual_out is NULL */
    const void* residual;       int64_t residual_stride;       /* forward, optional */
    void* y;                    int64_t y_stride;              /* forward */
    void* residual_out;         int64_t residual_out_stride;   /* forward: optional, written; backward: optional, x_saved */
    const float* weight;
    const float* bias;                                         /* forward, optional */
    float* mean;                                               /* forward: written; backward: read */
    float* rstd;
    const void* dy;             int64_t dy_stride;             /* backward */
    const void* dresidual;      int64_t dresidual_stride;      /* backward, optional */
    void* dx;                   int64_t dx_stride;             /* backward */
    void* dresidual_in;         int64_t dresidual_in_stride;   /* backward, optional */
    float* dweight;                                            /* backward */
    float* dbias;                                              /* backward, optional */
    void* workspace;                                           /* backward */
    size_t workspace_bytes;
    void* stream;
} segm_add_norm_args;

/* 0 for a shape out of range */
size_t segm_add_norm_workspace_bytes(int64_t rows, int32_t cols);
int segm_add_norm_fwd(const segm_add_norm_args* args);
int segm_add_norm_bwd(const segm_add_norm_args* args);


/* ------------------------------------------------------------------------------------------------ */
int segm_abi_version(void);
const char* segm_status_string(int status);

/* ------------------------------------------------------------------------------------------------
 * Depth-to-space / space-to-depth by 2 x 2 x 2 (ABI 7).
 * Replaces the permuting copy behind the GEMM of a ConvTranspose3d with kernel_size = stride = 2 (reference
 * monai/networks/blocks/unetr_block.py:52-60 via dynunet_block.get_conv_layer) and, in its backward, the inverse gather:
 *
 *   direction 0 (depth-to-space)   vol[b, c, 2z+i, 2y+j, 2x+k] = blk[b, c, i, j, k, z, y, x]
 *   direction 1 (space-to-depth)   blk[b, c, i, j, k, z, y, x] = vol[b, c, 2z+i, 2y+j, 2x+k]
 *
 * blk is contiguous (batch, channels, 2, 2, 2, depth, height, width); vol is (batch, channels, 2 depth, 2 height, 2 width) with
 * element strides vol_stride_b / _c / _z / _y and unit stride along x (padded volumes).  16-bit element types; width % 8 == 0;
 * 16-byte aligned rows.
 * ------------------------------------------------------------------------------------------------ */
typedef struct segm_d2s_args {
    int32_t batch, channels, depth, height, width;      /* of the LOW-resolution block tensor */
    int32_t dtype, direction, reserved;
    void* blk;
    void* vol;
    int64_t vol_stride_b, vol_stride_c, vol_stride_z, vol_stride_y;
    void* stream;
} segm_d2s_args;

int segm_depth_to_space2(const segm_d2s_args* args);

#ifdef __cplusplus
}
#endif
#endif /* SEGMAMBA_HIP_H */
