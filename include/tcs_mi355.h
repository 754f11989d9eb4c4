/*
 * tcs_mi355.h — C ABI of libtcs_mi355.so: the TC-Stereo inference hot path on MI355X (gfx950).
 *
 * The reference (jiaxiZeng/Temporally-Consistent-Stereo-Matching) has no FFI layer: its "operator
 * API" is Python call signatures over torch tensors, plus ONE native entry point, the CuPy-JIT CUDA
 * kernel `softsplat_out(n, tenIn, tenFlow, tenOut)` (core/utils/splatting/softsplat.py:285-290).
 * Every function below replaces one of those Python-level operators (cited per function) with a
 * hand-written HIP kernel sequence.  The Python mirror in
 * `temporally-consistent-stereo-matching_amd/core/` binds these with ctypes; INTEGRATION.md shows the
 * stub a maintainer of the reference would add.
 *
 * Conventions
 *  - Every tensor is a raw DEVICE pointer to contiguous float32 in NCHW order unless stated.
 *  - The caller owns every buffer, including outputs and workspaces (`*_workspace_bytes`).
 *    Nothing is allocated, freed or synchronised inside; all work is enqueued on `stream`
 *    (a hipStream_t passed as void*; NULL = the default stream).  Safe under HIP graph capture.
 *  - Return value: 0 on success, negative TCS_E* otherwise.  Never throws, never exits.
 *  - Re-entrant per stream.  The only mutable global state is the set of device-side S16 domain-flag words, written by kernels on
 *    a domain violation and read-and-cleared by tcs_s16_flags / tcs_s16_flags_detail (which synchronise the device).
 */
#ifndef TCS_MI355_H
#define TCS_MI355_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TCS_OK 0
#define TCS_EINVAL (-1)      /* bad argument (null pointer, non-positive size, unsupported shape) */
#define TCS_ELAUNCH (-2)     /* the HIP runtime rejected a launch / memset */
#define TCS_EUNSUPPORTED (-3)

typedef void* tcs_stream_t;

int tcs_abi_version(void);                 /* bumped when a signature changes (7: grouped launches, blend_warm_*; 8: `products`, the
                                              last field of tcs_conv_desc and tcs_conv_s16_desc; 9: the ordered splat entry points;
                                              10: tcs_conv2d_group_fused; 11: the *_mixed entry points;
                                              12: tcs_convex_upsample_pair, tcs_resize_bilinear_scaled; 13: the tcs_*loss* entry points;
                                              14: tcs_corr_lookup_backward, tcs_corr_build_backward*;
                                              15: tcs_loss_finish_counts, the tcs_*loss*_bwd entry points;
                                              16: tcs_upsample_flow*, tcs_convex_upsample*_backward*, tcs_refine_blend*;
                                              17: tcs_conv2d_s16_plan;
                                              18: tcs_gru_reset*, tcs_gru_update*) */
const char* tcs_error_string(int code);

/* ------------------------------------------------------------------------------------------------
 * Correlation volume: build, pyramid, first-frame argmax, lookup           (core/corr.py)
 *
 * HBM layout of the pyramid ("skewed"): level i is stored as P_i[b][h][d][w1], d in [0, W_i),
 * W_i = W >> i, holding L_i[b][h][w1][j] at d = ((w1 >> i) - j) mod W_i.  For a smooth disparity
 * field the 2r+2 taps of horizontally adjacent pixels then sit in the same few rows `d`, contiguous
 * along w1, so one wavefront's loads coalesce into a handful of 256-byte segments instead of 64
 * scattered lines (the reference layout [b][h][w1][j] puts every pixel's window in its own row).
 * ---------------------------------------------------------------------------------------------- */

/* bytes of one skewed level i (i = 0..3) for a [B,C,H,W] feature map */
size_t tcs_corr_level_bytes(int B, int H, int W, int level);
/* scratch needed by tcs_corr_build (natural-layout level 0 + inverse norms) */
size_t tcs_corr_build_workspace_bytes(int B, int H, int W);

/*
 * CorrBlock1D.__init__ + CorrBlock1D.corr (core/corr.py:8-31,54-62) and, when sparse_* are given,
 * CorrBlock1D.argmax_disp (core/corr.py:67-79) fused into the same pass.
 *   fmap1, fmap2 : [B,C,H,W]
 *   pyr0..pyr3   : skewed levels (sizes from tcs_corr_level_bytes)                    (required)
 *   nat1..nat3   : natural-layout levels [B,H,W,W>>i] as the reference stores them    (nullable; tests)
 *                  (natural level 0 is always left in the workspace: see tcs_corr_ws_level0)
 *   cost_volume  : [B,W,H,W] masked volume cost[b,w2,h,w1] = V*(w2<=w1), corr.py:25-31 (nullable)
 *   sparse_disp, sparse_cost, sparse_mask : [B,1,H,W] each                             (all or none)
 */
int tcs_corr_build(const float* fmap1, const float* fmap2, int B, int C, int H, int W,
                   float* pyr0, float* pyr1, float* pyr2, float* pyr3,
                   float* nat1, float* nat2, float* nat3,
                   float* cost_volume,
                   float* sparse_disp, float* sparse_cost, float* sparse_mask,
                   void* workspace, tcs_stream_t stream);
/* pointer to the natural-layout level 0 volume [B,H,W,W] inside a build workspace */
float* tcs_corr_ws_level0(void* workspace);

/*
 * CorrBlock1D.__call__ (core/corr.py:33-52) with bilinear_sampler (core/utils/utils.py:82-97):
 *   coords [B,1,H,W] (x position in the right image) -> out [B, 4*(2*radius+1), H, W].
 * Channel = level*(2r+1) + tap, taps ascending in dx; samples outside a level read 0.
 */
int tcs_corr_lookup(const float* pyr0, const float* pyr1, const float* pyr2, const float* pyr3,
                    const float* coords, int B, int H, int W, int radius, float* out,
                    unsigned long long* stamps, tcs_stream_t stream);
/* Measurement hook: when `stamps` is non-NULL (device uint64[2 * tcs_corr_lookup_blocks(B,H,W)], zeroed by the
 * caller) every workgroup records the device wall clock (s_memrealtime, 100 MHz) at its start and end, so the
 * launch duration = max(end) - min(start) can be read without a profiler.  NULL in production. */
int tcs_corr_lookup_blocks(int B, int H, int W);

/*
 * Backward of CorrBlock1D.__call__ (core/corr.py:33-52 with core/utils/utils.py:82-97): what autograd
 * of the four F.grid_sample calls and the avg_pool2d chain (corr.py:20-23) gives for one lookup.
 *   pyr0..pyr3, coords, radius : as passed to tcs_corr_lookup (the levels are read only for grad_coords)
 *   grad_out    : [B, 4*(2r+1), H, W], the gradient of the lookup's output
 *   grad_vol    : [B,H,W,W] gradient w.r.t. the natural level 0 volume V, every entry written  (nullable)
 *                 dV[b,h,w1,w2] = sum_i 2^-i sum_t g_i[t] * lerp weight of tap w2>>i (taps outside a level: 0)
 *   grad_coords : [B,1,H,W], sum_i 2^-i sum_t g_i[t] (v_i[t+1] - v_i[t]) (floor-based lerp)   (nullable)
 * No atomics: two calls on the same inputs are bit-equal.
 */
int tcs_corr_lookup_backward(const float* pyr0, const float* pyr1, const float* pyr2, const float* pyr3,
                             const float* coords, const float* grad_out, int B, int H, int W, int radius,
                             float* grad_vol, float* grad_coords, tcs_stream_t stream);

/* scratch needed by tcs_corr_build_backward (0 at this version: the call then accepts scratch = NULL) */
size_t tcs_corr_build_backward_scratch_bytes(int B, int C, int H, int W);
/*
 * Backward of CorrBlock1D.corr (core/corr.py:54-62): autograd of the einsum and of both F.normalize
 * calls (eps 1e-12; a pixel with |f| < eps takes d f = d n / eps, as torch does).
 *   fmap1, fmap2 : [B,C,H,W], the inputs of the tcs_corr_build call that filled `workspace`
 *   workspace    : that build's workspace (its inverse norms are read)
 *   grad_vol     : [B,H,W,W] gradient w.r.t. V (the sum of every consumer's contribution)
 *   grad_fmap1, grad_fmap2 : [B,C,H,W], written in full                                    (nullable each)
 * Fixed reduction order, no atomics: repeated calls are bit-equal.
 */
int tcs_corr_build_backward(const float* fmap1, const float* fmap2, const void* workspace, const float* grad_vol,
                            int B, int C, int H, int W, float* grad_fmap1, float* grad_fmap2, void* scratch,
                            tcs_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Temporal warp                                 (core/utils/geo_utils.py, core/utils/splatting/softsplat.py)
 * ---------------------------------------------------------------------------------------------- */
size_t tcs_warp_workspace_bytes(int B, int C, int H, int W);

/*
 * warp() (geo_utils.py:158-198) = disparity -> 3-D -> relative pose -> reprojection, then
 * softsplat(..., 'soft-clipeps', valid) (softsplat.py:232-274, kernel softsplat_out :285-335),
 * optionally followed by the temporal matching cost of tc_stereo.py:139-140.
 *   prev_disp [B,1,H,W] (>= 0), prev_fmap [B,C,H,W]
 *   T_rel [B,4,4], K [B,3,3], K_inv [B,3,3] (K already scaled to the 1/4 grid), baseline [B]
 *   out_disp [B,1,H,W], out_mask [B,1,H,W]                                   (required)
 *   out_fmap [B,C,H,W]                                                       (nullable)
 *   cur_fmap [B,C,H,W] + out_cost [B,1,H,W]: cosine cost vs the current frame (both or none)
 * Float atomics are used for the splat, like the reference's atomicAdd: the summation order, and
 * therefore the last bits, can differ from run to run (tcs_warp_forward_ordered below fixes the order).
 */
int tcs_warp_forward(const float* prev_disp, const float* prev_fmap, const float* T_rel, const float* K,
                     const float* K_inv, const float* baseline, int B, int C, int H, int W,
                     float* out_disp, float* out_fmap, float* out_mask,
                     const float* cur_fmap, float* out_cost,
                     void* workspace, tcs_stream_t stream);

/*
 * Ordered splat (tcs_warp_forward_ordered, tcs_softsplat_sum_ordered): bit-reproducible from run to run, whatever the scheduling,
 * the stream, graph or eager launches, or what runs beside it.  The contributions are those of the atomic splat; their sum has a
 * fixed order.  For source pixel p = y*W + x of batch element b (batch elements are independent):
 *   fx = (float)x + flow[b,0,p], fy = (float)y + flow[b,1,p]; no contribution if fx or fy is not finite, if valid[b,p] == 0
 *   (warp only), or unless -2 <= floor(fx) <= W and -2 <= floor(fy) <= H.  x0 = floor(fx), y0 = floor(fy); corner weights
 *   w00 = (x0+1-fx)*(y0+1-fy), w10 = (fx-x0)*(y0+1-fy), w01 = (x0+1-fx)*(fy-y0), w11 = (fx-x0)*(fy-y0) (each op one fp32 rounding),
 *   each to target (x0+dx, y0+dy) when that is inside the frame.
 * Target t's channel c is    acc = 0;  for its contributions in ASCENDING p:  acc = fl(acc + fl(v * w))
 * in plain fp32 (no FMA contraction), v = in[b,c,p] (summation splat) or, for warp(), fl(v' * s) with s = expf(clamp(cur_disp[p] -
 * mean, +-50)) and v' = prev_fmap[b,c,p] (channels < C), cur_disp[p] (the disparity sum) or 1 (the normaliser, v = s).  A source adds
 * at most one corner to a target, so the order is total.  warp() then normalises, splits and forms the cosine cost exactly as
 * tcs_warp_forward does.  Same arguments and outputs as the atomic entry points, except that tcs_softsplat_sum_ordered WRITES `out`
 * (no zeroing needed) and both take a workspace of their own size query.  Needs B*4*H*W < 2^31.
 */
size_t tcs_warp_ordered_workspace_bytes(int B, int C, int H, int W);
int tcs_warp_forward_ordered(const float* prev_disp, const float* prev_fmap, const float* T_rel, const float* K,
                             const float* K_inv, const float* baseline, int B, int C, int H, int W,
                             float* out_disp, float* out_fmap, float* out_mask,
                             const float* cur_fmap, float* out_cost,
                             void* workspace, tcs_stream_t stream);
/*
 * Mixed batches (tcs_warp_forward_mixed, tcs_warp_forward_ordered_mixed): independent sequences on the batch dimension, some of which
 * start on this frame.  start [B] (device, unsigned char): nonzero = batch element b begins a sequence.  Arguments and outputs as in
 * tcs_warp_forward / _ordered (same workspace size queries), plus the mask and the first-frame prior prior_disp, prior_cost,
 * prior_mask [B,1,H,W] (tcs_corr_build's sparse_* outputs; all three required).
 *   A start element reads none of prev_disp, prev_fmap, T_rel, K, K_inv, baseline (they may hold anything, NaN included); it adds
 *   nothing to the mean and no splat contributions (no index entries in the ordered path).  Its out_disp, out_mask and out_cost are
 *   copied from the prior, its out_fmap (when requested) is 0.
 *   A temporal element (start[b] == 0) gets the arithmetic of the non-mixed entry point, except that the softmax metric's mean is
 *   over the temporal elements' pixels only: exactly warp() on the sub-batch of temporal elements.  With no temporal element no mean
 *   is formed.  With an all-zero mask the outputs are bit-equal to tcs_warp_forward / _ordered on the same inputs.
 */
int tcs_warp_forward_mixed(const float* prev_disp, const float* prev_fmap, const float* T_rel, const float* K,
                           const float* K_inv, const float* baseline, const unsigned char* start, const float* prior_disp,
                           const float* prior_cost, const float* prior_mask, int B, int C, int H, int W,
                           float* out_disp, float* out_fmap, float* out_mask, const float* cur_fmap, float* out_cost,
                           void* workspace, tcs_stream_t stream);
int tcs_warp_forward_ordered_mixed(const float* prev_disp, const float* prev_fmap, const float* T_rel, const float* K,
                                   const float* K_inv, const float* baseline, const unsigned char* start, const float* prior_disp,
                                   const float* prior_cost, const float* prior_mask, int B, int C, int H, int W,
                                   float* out_disp, float* out_fmap, float* out_mask, const float* cur_fmap, float* out_cost,
                                   void* workspace, tcs_stream_t stream);
size_t tcs_softsplat_ordered_workspace_bytes(int B, int H, int W);
int tcs_softsplat_sum_ordered(const float* in, const float* flow, int B, int C, int H, int W, float* out, void* workspace,
                              tcs_stream_t stream);

/* The pre-splat quantities of warp() (geo_utils.py:169-193), exposed for parity tests:
 * cur_disp, valid, flow [B,2,H,W], metric — all [B,1,H,W] unless noted. */
int tcs_warp_geometry(const float* prev_disp, const float* T_rel, const float* K, const float* K_inv,
                      const float* baseline, int B, int H, int W,
                      float* cur_disp, float* valid, float* flow, float* metric,
                      void* workspace, tcs_stream_t stream);

/* softsplat 'summation' core (softsplat.py:285-335): out[B,C,H,W] += bilinear splat of in along flow.
 * `out` must be zeroed by the caller.  One thread per source pixel; 4 x C float atomics each. */
int tcs_softsplat_sum(const float* in, const float* flow, int B, int C, int H, int W, float* out,
                      tcs_stream_t stream);

/* get_backward_grid (geo_utils.py:201-236): grid [B,2,H,W] of previous-frame pixel coordinates. */
int tcs_backward_grid(const float* disp, const float* T_rel, const float* K, const float* K_inv,
                      const float* baseline, int B, int H, int W, float* grid, tcs_stream_t stream);

/* Camera algebra of TCStereo.forward (tc_stereo.py:121-127,159) on the device, no host round trip:
 * K_scaled = K * [scale,scale,1]^T (rows 0,1), its inverse, and — when T / T_prev are given —
 * T_rel = T * inv(T_prev) (geo_utils.py:148-155) and T_back = T_prev * inv(T).  K [B,3,3], T [B,4,4]. */
int tcs_pose_prepare(const float* K, const float* T, const float* T_prev, float scale, int B,
                     float* K_scaled, float* K_scaled_inv, float* T_rel, float* T_back, tcs_stream_t stream);
/* The same for a mixed batch (start [B], device): start elements get identity T_rel / T_back without their T or T_prev being read;
 * K_scaled and its inverse are formed for every element.  T, T_prev, T_rel, T_back are required. */
int tcs_pose_prepare_mixed(const float* K, const float* T, const float* T_prev, const unsigned char* start, float scale, int B,
                           float* K_scaled, float* K_scaled_inv, float* T_rel, float* T_back, tcs_stream_t stream);

/* bilinear_sampler (core/utils/utils.py:82-97): img [B,C,Hi,Wi] sampled at grid [B,2,Ho,Wo] (x,y in
 * pixels), zeros outside, align_corners=True -> out [B,C,Ho,Wo]. */
int tcs_bilinear_sample(const float* img, const float* grid, int B, int C, int Hi, int Wi, int Ho, int Wo,
                        float* out, tcs_stream_t stream);
/* The same for a mixed batch (start [B], device): a start element's output is +0.0 everywhere (a first frame's warped hidden
 * states), and neither its img nor its grid is read. */
int tcs_bilinear_sample_mixed(const float* img, const float* grid, const unsigned char* start, int B, int C, int Hi, int Wi, int Ho,
                              int Wo, float* out, tcs_stream_t stream);

/* 0.5 * F.interpolate(grid, scale_factor=0.5, bilinear, align_corners=True) (tc_stereo.py:163):
 * grid [B,2,H,W] -> [B,2,H/2,W/2]. */
int tcs_grid_halve(const float* grid, int B, int H, int W, float* out, tcs_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Stencils of the refinement loop
 * ---------------------------------------------------------------------------------------------- */
/* coords bookkeeping (tc_stereo.py:188-189): coords1 += delta; disp_q = x - coords1 (in place on coords1). */
int tcs_flow_step(float* coords1, const float* delta, int B, int H, int W, float* disp_q, tcs_stream_t stream);

/* The three stencils that open an iteration's gradient stage, fused: disp_q = x - (coords1 + delta)
 * (tc_stereo.py:188-189; coords1 itself is left untouched), grad = scale * disp2disp_gradient_xy(disp_q)
 * (geo_utils.py:115-132, update.py:199), cands = disp2disp_grad_candidates(disp_q, level=2) (geo_utils.py:73-101).
 * Outputs equal tcs_flow_step + tcs_disp_gradient_xy + tcs_grad_candidates bit for bit.
 * coords1, delta, disp_q [B,1,H,W]; grad [B,2,H,W]; cands [B,32,H,W]. */
int tcs_flow_step_grads(const float* coords1, const float* delta, int B, int H, int W, float scale, float* disp_q, float* grad,
                        float* cands, tcs_stream_t stream);

/* disp2disp_gradient_xy (geo_utils.py:115-132) scaled by `scale` (the 5x of update.py:199):
 * disp [B,1,H,W] -> grad [B,2,H,W]. */
int tcs_disp_gradient_xy(const float* disp, int B, int H, int W, float scale, float* grad, tcs_stream_t stream);

/* disp2disp_grad_candidates(level=2) (geo_utils.py:73-101) flattened as update.py:202-204:
 * disp [B,1,H,W] -> cands [B,32,H,W], channel = comp*16 + k. */
int tcs_grad_candidates(const float* disp, int B, int H, int W, float* cands, tcs_stream_t stream);

/* DispRefine.propagate_disparity (update.py:259-289): grad [B,2,H,W], disp [B,1,H,W] ->
 * out [B,27,H,W] = cat(candidates(9), |grad diff|(18)) — the input of disp_f_stem (update.py:295). */
int tcs_propagate_disparity(const float* grad, const float* disp, int B, int H, int W, float* out27,
                            tcs_stream_t stream);

/* update.py:298-300 + tc_stereo.py:198-202: softmax over the 9 logits (max-subtracted), blend the 9
 * candidates (first 9 channels of a [B,cand_ctot,H,W] buffer), and emit
 *   refined [B,1,H,W], delta_disp = refined - disp_q [B,1,H,W] (nullable), coords1 = x - refined (nullable),
 *   and the next iteration's motion-encoder input coords1 - x (tc_stereo.py:180) twice (both nullable): flow_x [B,1,H,W]
 *   and flow_x_ch, one channel plane per batch element at a stride of flow_x_ch_bstride floats (channel 127 of the
 *   [B,128,H,W] motion feature buffer, update.py:126). */
int tcs_softmax_blend(const float* logits9, const float* cand, int cand_ctot, const float* disp_q,
                      int B, int H, int W, float* refined, float* delta_disp, float* coords1, float* flow_x, float* flow_x_ch,
                      long long flow_x_ch_bstride, tcs_stream_t stream);

/* TCStereo.upsample_flow (tc_stereo.py:75-88) with factor 4, applied to flow = -disp:
 * disp [B,1,H,W], mask [B,144,H,W] -> flow_up [B,1,4H,4W]; flow_q [B,1,H,W] = -disp (nullable).
 * clip != 0 additionally applies the torch.clip(., max=0) of the returned dict (tc_stereo.py:223-224)
 * to both outputs. */
int tcs_convex_upsample(const float* disp, const float* mask, int B, int H, int W, int clip, float* flow_up, float* flow_q,
                        tcs_stream_t stream);

/* The two upsamplings of one iteration's non-test-mode outputs (tc_stereo.py:204-215), which share that iteration's mask:
 * disp_a, disp_b [B,1,H,W] (disp_q and refined_disp), mask [B,144,H,W] -> up_a, up_b [B,1,4H,4W] and q_a = -disp_a, q_b = -disp_b
 * [B,1,H,W].  The mask is read and each output pixel's 9-way softmax computed once for both.  Not clipped.  Each output is
 * bit-equal to tcs_convex_upsample(..., clip = 0) on that disparity (up_x to its flow_up, q_x to its flow_q).  The outputs are
 * dense [B,...] blocks and may be slots of larger stacked tensors. */
int tcs_convex_upsample_pair(const float* disp_a, const float* disp_b, const float* mask, int B, int H, int W, float* up_a, float* up_b,
                             float* q_a, float* q_b, tcs_stream_t stream);

/* pool2x = avg_pool2d(3, stride 2, pad 1), divisor 9 everywhere (update.py:114-115): [B,C,H,W] -> [B,C,Ho,Wo],
 * Ho = (H-1)/2+1. */
int tcs_avgpool3s2(const float* x, int B, int C, int H, int W, float* out, tcs_stream_t stream);

/* interp(): bilinear resize with align_corners=True (update.py:122-124): [B,C,H,W] -> [B,C,Ho,Wo]. */
int tcs_resize_bilinear(const float* x, int B, int C, int H, int W, int Ho, int Wo, float* out, tcs_stream_t stream);
/* tcs_resize_bilinear times `scale` (the -4 * F.interpolate(., scale_factor=4, bilinear, align_corners=True) of flow_mono /
 * flow_init, tc_stereo.py:233-234).  With scale = 1 it equals tcs_resize_bilinear; a power-of-two scale scales it exactly. */
int tcs_resize_bilinear_scaled(const float* x, int B, int C, int H, int W, int Ho, int Wo, float scale, float* out, tcs_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Convolutions on the matrix cores, fp32 NCHW tensors in and out: fp32 MFMA (TCS_MATH_F32) or fp16-split operands with fp32
 * accumulation (TCS_MATH_F16X3, the default of the Python mirror) — see tcs_conv_desc.math
 * ---------------------------------------------------------------------------------------------- */
#define TCS_ACT_NONE 0
#define TCS_ACT_RELU 1
#define TCS_ACT_SIGMOID 2
#define TCS_ACT_TANH 3
#define TCS_ACT_LEAKY 4          /* LeakyReLU(0.01) */
#define TCS_ACT_RELU_ADD_RELU 5  /* relu(relu(v) + addend): the tail of a residual block (extractor.py:44-58); needs addend */

#define TCS_EPI_LINEAR 0         /* out = act(conv + bias + addend) * post_scale                   */
#define TCS_EPI_GRU_ZR 1         /* first half: z = sigmoid(. + cz) -> out; second half: r = sigmoid(. + cr), out2 = r*h */
#define TCS_EPI_GRU_Q 2          /* q = tanh(. + cq); out = blend(z, h, q)                           */
#define TCS_EPI_BLEND9 4         /* tcs_conv2d_s16 only, Cout = 9: the nine outputs are the logits of DispRefine's softmax blend
                                    (core/update.py:298-300), which runs in the epilogue — see tcs_conv_s16_desc.blend_*     */
#define TCS_EPI_DECONV2X 3       /* ConvTranspose2d(k=4, stride 2, pad 1, no bias): weights from
                                    tcs_pack_deconv4x4s2_f16x3, out [B, Cout/4, 2H, 2W]   (F16X3 only)      */

#define TCS_MATH_F32 0           /* v_mfma_f32_32x32x2_f32: fp32 in, fp32 accumulate                                  */
#define TCS_MATH_F16X3 1         /* fp16 hi/lo split, 3 x v_mfma_f32_32x32x16_f16 per product, fp32 accumulate (~2^-21) */

#define TCS_MAX_SRC 4

typedef struct tcs_conv_desc {
    /* virtual concatenation of up to 4 NCHW sources along channels (replaces torch.cat, update.py:79-80) */
    const float* src[TCS_MAX_SRC];
    int src_ch[TCS_MAX_SRC];
    int n_src;
    const float* weight;     /* packed by tcs_pack_conv_weight */
    const float* bias;       /* [Cout] or NULL */
    int B, H, W;             /* stride-1 'same' convolution: output H,W = input H,W */
    int Cin, Cout, ksize;    /* ksize in {1,3,7} */
    int epilogue;            /* TCS_EPI_* */
    int act;                 /* TCS_ACT_*  (LINEAR epilogue only) */
    float post_scale;        /* LINEAR epilogue: multiplies the activated value (e.g. 0.25 of update.py:304) */
    const float* addend;     /* LINEAR: optional [B,Cout,H,W] added before the activation.
                                GRU_ZR: cz;  GRU_Q: cq  ([B,hidden,H,W], nullable)                   */
    const float* addend2;    /* GRU_ZR: cr (nullable) */
    const float* h;          /* GRU_ZR / GRU_Q: hidden state [B,hidden,H,W] */
    const float* z;          /* GRU_Q: update gate from the ZR pass */
    int blend_keep_z;        /* GRU_Q: 0 -> (1-z)h + zq (ConvGRU, update.py:85); 1 -> zh + (1-z)q (update.py:34,66) */
    float* out;              /* LINEAR: [B,out_ctot,H,W] written at channel offset out_coff. GRU_ZR: z. GRU_Q: new h */
    int out_ctot, out_coff;
    float* out2;             /* GRU_ZR: r*h */
    int stride;              /* 0 or 1: 'same' convolution; 2: 3x3 stride-2 pad-1 (F16X3 only), output (H-1)/2+1 x (W-1)/2+1 */
    int math;                /* TCS_MATH_F32: weights from tcs_pack_conv_weight; TCS_MATH_F16X3: from ..._f16x3 */
    float weight_unscale;    /* F16X3: 2^-scale_log2 given to tcs_pack_conv_weight_f16x3 */
    void* out16;             /* LINEAR, stride 1: optional S16 ("pre-split", see below) copy of the output, so that a layer fed by a
                                fp32 tensor (correlation features, disparity stencils) hands its result to tcs_conv2d_s16 consumers
                                without a conversion pass; `out` may then be NULL */
    int out16_groups, out16_group_offset;
    /* 7x7 RGB stem only (Cin = 3): the image preparation of TCStereo.forward folded into its input staging (core/tc_stereo.py:101-107).
     * in_transform = 1: every in-image sample x is read as 2 * (x / 255) - 1 (padding stays 0).  src_batch2 / batch_split: batch
     * elements >= batch_split come from this second tensor [B - batch_split, 3, H, W] instead of src[0] — torch.cat((image1, image2), 0)
     * without the copy.  0 / NULL = off. */
    int in_transform;
    const float* src_batch2;
    int batch_split;
    /* MFMA products per (16-channel k-step, tap) of TCS_MATH_F16X3: 0 or 3 = the fp16-split contraction (a_lo.b_hi + a_hi.b_lo +
     * a_hi.b_hi, fp32-grade; the default); 1 = a_hi.b_hi only: sum f16(x) * f16(w * 2^s) * 2^-s with fp32 accumulation (the opt-in fp16
     * mode of the Python layer).  Storage, epilogues and the domain guard are the same in both.  Any other value, and 1 with
     * TCS_MATH_F32, is TCS_EINVAL. */
    int products;
} tcs_conv_desc;

/* packed weight size in floats for a [Cout,Cin,k,k] convolution */
size_t tcs_conv_packed_floats(int Cout, int Cin, int ksize);
/* OIHW device weights -> the kernel's layout ([Cin_pad][k*k][Cout_pad], zero padded) */
int tcs_pack_conv_weight(const float* w_oihw, int Cout, int Cin, int ksize, float* packed, tcs_stream_t stream);
/* fp16-split weights: OIHW * 2^scale_log2, split into (hi, lo) halves, in the kernel's LDS image order.
 * Choose scale_log2 so that max|w| * 2^scale_log2 is ~2^10..2^14 (keeps the lo halves normal). ksize in {1,3}. */
size_t tcs_conv_packed_floats_f16x3(int Cout, int Cin, int ksize);
int tcs_pack_conv_weight_f16x3(const float* w_oihw, int Cout, int Cin, int ksize, int scale_log2, float* packed,
                               tcs_stream_t stream);
/* nn.ConvTranspose2d(Cin, Cout, 4, stride 2, padding 1, bias=False) weights [Cin,Cout,4,4] -> the F16X3 layout of
 * the equivalent 3x3 convolution with 4*Cout outputs (one group per output parity); use with TCS_EPI_DECONV2X,
 * desc.Cout = 4*Cout, ksize = 3.  (core/utils/basic_layers.py:17-21,57) */
size_t tcs_deconv_packed_floats_f16x3(int Cin, int Cout);
int tcs_pack_deconv4x4s2_f16x3(const float* w_iohw, int Cin, int Cout, int scale_log2, float* packed, float* scratch_oihw,
                               tcs_stream_t stream);
/* nn.InstanceNorm2d (affine=False, eps, biased variance) + activation + optional addend, per (b, c) plane:
 * out = act((x - mean) / sqrt(var + eps)) + addend      (basic_layers.py:28-35,65-76; update.py:325-367) */
int tcs_instance_norm(const float* x, int B, int C, int H, int W, float eps, int act, const float* addend, float* out,
                      tcs_stream_t stream);
/* nn.Conv2d(Cin, 1, 3, padding=1): single-output-channel 3x3 convolution as a plain fp32 reduction (FlowHead.conv2,
 * core/update.py:13).  w_oihw is the ORIGINAL [1,Cin,3,3] weight (no packing); out [B,1,H,W]. */
int tcs_conv3x3_cout1(const float* x, const float* w_oihw, const float* bias, int B, int Cin, int H, int W, float* out,
                      tcs_stream_t stream);
/* nn.Conv2d(k, padding=k/2) + fused epilogue; covers ConvGRU / Lightfuse / HiddenstateUpdater /
 * BasicMotionEncoder / FlowHead / the stride-1 convs of DispRefine and DispGradPredictor (core/update.py). */
int tcs_conv2d(const tcs_conv_desc* desc, tcs_stream_t stream);
/* n (1 or 2) INDEPENDENT convolutions of tcs_conv2d as one launch where a grouped kernel exists for them (two fp32-MFMA 3x3 layers of
 * <= 32-channel tiles: the first layers of DispGradPredictor's stems, core/update.py:200-205), otherwise one after the other; bit-equal
 * to n calls of tcs_conv2d either way (see tcs_conv2d_s16_group).  Layers without a planned kernel (fp16-split, 7x7, Cin == 1) are
 * launched while the pair is planned, ahead of the other layer.  tcs_conv2d_group_fused: 1 when the two descriptors would run as one
 * launch (no launch is made, also not for the layers without a planned kernel: they answer 0). */
int tcs_conv2d_group(const tcs_conv_desc* const* descs, int n, tcs_stream_t stream);
int tcs_conv2d_group_fused(const tcs_conv_desc* const* descs, int n);

/* ---------------------------------------------------------------------------------------------------------------------
 * Pre-split activations ("S16" tensors): the refinement loop's internal activation format.
 *
 * The convolutions contract fp16 hi/lo halves of every fp32 operand (TCS_MATH_F16X3).  Inside the refinement loop
 * (core/tc_stereo.py:176-210, core/update.py) the PRODUCER of an activation splits it once and stores it in operand
 * form, so that the consuming convolution stages it with plain 16-byte copies (LDS-DMA) instead of converting it again
 * for every output tile:
 *
 *     logical [B][C][H][W] fp32   ->   _Float16 [B][G][2][H+2][W+2][8]
 *         G = 2*ceil(C/16) channel groups of 8, [2] = {hi, lo} with x = hi + lo (+ <= 2^-22 |x|, |x| <= 65504),
 *         a one-pixel ZERO border (the 'same' padding of a 3x3 convolution), zero padding channels.
 *
 * The caller allocates the buffer ZERO-FILLED once (tcs_s16_bytes); producers only ever write interior pixels of real
 * channel groups, so the border stays zero for the buffer's lifetime.  fp32 NCHW remains the format of every reference-facing
 * entry point above; tcs_s16_from_f32 / tcs_s16_to_f32 convert at the loop's boundary.
 * ------------------------------------------------------------------------------------------------------------------- */
size_t tcs_s16_bytes(int B, int C, int H, int W);
/* Domain guard of the split (|x| <= 65504): every producer of S16 data marks a device-side flag word when it had to clamp a
 * finite value (bit 0) or met a NaN / Inf (bit 1) — the replacement of the reference's per-iteration NaN asserts
 * (core/update.py:27-35,58-67,78-86,155-158).  Reads and clears the word; SYNCHRONISES the device (call it once per frame or
 * sequence, outside any graph capture). */
int tcs_s16_flags(unsigned int* flags_out);
/* The same read-and-clear, one word per producing source file of the library, for locating a violation:
 * [0] tcs_conv_s16.hip (S16 convolutions, GRU / deconv / blend epilogues, tcs_s16_from_f32), [1] tcs_s16_ops.hip (pool, interp, InstanceNorm,
 * propagate stencil, fused HiddenstateUpdater), [2] tcs_conv.hip (fp32-MFMA and 7x7 convolutions with an S16 epilogue),
 * [3] tcs_conv_f16.hip (fp32-tensor fp16-split convolutions with an S16 epilogue), [4] tcs_stencil.hip (the stand-alone blend kernel's flow channel). */
#define TCS_S16_FLAG_UNITS 5
int tcs_s16_flags_detail(unsigned int* per_unit);
/* x [B,C,H,W] fp32 -> groups [group_offset, group_offset + 2*ceil(C/16)) of an S16 tensor with groups_total groups */
int tcs_s16_from_f32(const float* x, int B, int C, int H, int W, void* s16, int groups_total, int group_offset, tcs_stream_t stream);
/* channels [8*group_offset, 8*group_offset + C) of an S16 tensor -> out [B,C,H,W] fp32 (hi + lo) */
int tcs_s16_to_f32(const void* s16, int B, int C, int H, int W, int groups_total, int group_offset, float* out, tcs_stream_t stream);

typedef struct tcs_conv_s16_desc {
    /* virtual concatenation of up to 4 S16 sources along channels (torch.cat of update.py:79-80); every source but the
     * last must carry a multiple of 16 channels */
    const void* src[TCS_MAX_SRC];
    int src_ch[TCS_MAX_SRC];        /* logical channels per source */
    int src_groups[TCS_MAX_SRC];    /* groups allocated per source tensor */
    int n_src;
    const float* weight;     /* tcs_pack_conv_weight_f16x3 / tcs_pack_deconv4x4s2_f16x3 of the [Cout, Cin, k, k] weight */
    const float* bias;       /* [Cout] or NULL */
    int B, H, W;             /* INPUT grid */
    int Cin, Cout, ksize;    /* ksize in {1,3} */
    int stride;              /* 1, or 2 (3x3 pad 1 or 1x1 pad 0, LINEAR): output (H-1)/2+1 x (W-1)/2+1 */
    int epilogue;            /* TCS_EPI_* as for tcs_conv2d */
    int act;
    float post_scale;
    float weight_unscale;
    const float* addend;     /* fp32 NCHW: LINEAR addend [B,Cout,Ho,Wo]; GRU_ZR cz / GRU_Q cq [B,hidden,H,W] (nullable) */
    const float* addend2;    /* GRU_ZR: cr */
    const void* addend16;    /* LINEAR: S16 addend on the output grid (the skip of a residual block, extractor.py:44-58; use with
                                TCS_ACT_RELU_ADD_RELU), addend16_groups groups; nullable */
    int addend16_groups;
    const void* h;           /* GRU: hidden state, S16 with h_groups groups */
    int h_groups;
    const float* z;          /* GRU_Q: update gate, fp32 [B,hidden,H,W] */
    int blend_keep_z;
    void* out16;             /* S16 output (LINEAR: act(.)*post_scale; DECONV2X: [C/4 channels, 2H, 2W]; GRU_ZR: r*h;
                                GRU_Q: new h, may alias `h`), written at group offset out16_group_offset; nullable for LINEAR */
    int out16_groups, out16_group_offset;
    float* out32;            /* fp32 NCHW output: LINEAR (nullable; [B,out_ctot,Ho,Wo] at channel out_coff); GRU_ZR: z (required);
                                GRU_Q: optional fp32 copy of the new h */
    int out_ctot, out_coff;
    int tile_cfg;            /* 0 = choose by grid size; otherwise CSPLIT*100000 + RS*10000 + MT*1000 + ROWS*100 + KSTEPS*10 + NSTAGE
                                (benchmarks, tests; csrc/tcs_conv_s16.hip) */
    int addend_ctot;         /* channels per batch element of `addend` / `addend2` (0 = Cout, or hidden for the GRU epilogues).  A wider
                                value lets them be channel slices of one tensor: a convolution is linear in its input channels, so a
                                layer whose inputs become available at different times runs as partial convolutions that
                                accumulate into one fp32 [B, addend_ctot, H, W] tensor (LINEAR: addend = out32), and the last
                                partial applies the real epilogue with that sum as its addend (GRU_ZR: cz = sum[:, :hidden],
                                cr = sum[:, hidden:]) */
    /* TCS_EPI_BLEND9 (w_head's last 1x1 convolution + tcs_softmax_blend_s16 in one launch; same arithmetic, same outputs):
     * refined = sum_k softmax(logits)_k * cand[:, k]; delta = refined - disp; coords1 = x - refined; flow_x = coords1 - x, also
     * written into channel blend_flow16_channel of the S16 tensor blend_flow16 (the motion features, core/update.py:126). */
    const float* blend_cand;        /* [B, blend_cand_ctot >= 9, H, W]: the nine candidates are its first channels */
    int blend_cand_ctot;
    const float* blend_disp;        /* [B,1,H,W] */
    float* blend_refined;           /* [B,1,H,W], required */
    float* blend_delta;             /* [B,1,H,W] or NULL */
    float* blend_coords1;           /* [B,1,H,W] or NULL */
    float* blend_flow_x;            /* [B,1,H,W] or NULL */
    void* blend_flow16;             /* S16 tensor or NULL */
    int blend_flow16_groups, blend_flow16_channel;
    /* LINEAR: two layers that read the same input as ONE launch (weights concatenated along Cout): output channels
     * [out16_split, Cout) go to groups [0, ...) of the second S16 tensor `out16b` instead of `out16`
     * (DispGradPredictor's residual_head[0] and conv_out[0] both read x4_up, core/update.py:212-214).
     * out16_split must be a multiple of 32; NULL = single output. */
    void* out16b;
    int out16b_groups, out16_split;
    /* DECONV2X: InstanceNorm2d statistics of the output accumulated by the transposed convolution itself (the up-blocks are
     * ConvTranspose2d -> InstanceNorm2d -> LeakyReLU, core/utils/basic_layers.py:28-35,57): every workgroup ADDS (sum x, sum x^2) of its
     * tile, in 64-bit fixed point (2^20 / 2^16 units; integer atomics, so the result does not depend on the order of arrival), to
     * in_stats[b][channel][2]; tcs_instance_norm_apply_s16 turns them into mean / rstd.  in_stats: tcs_deconv_in_stats_bytes() bytes
     * (16 per (b, channel)), ZERO-FILLED by the caller before EVERY launch that accumulates into it; needs Cout/4 % 32 == 0 and an
     * output grid of <= 2^20 pixels.  NULL = off.  in_eps: unused since ABI 6 (the apply call takes eps). */
    void* in_stats;
    float in_eps;
    /* LINEAR, stride 1: "tap partials" of a FOLLOWING 3x3 convolution to tap_nout = 1 or 2 channels (FlowHead.conv2, core/update.py:13-17;
     * DispGradPredictor.residual_head[2], core/update.py:196,213), so that that convolution never runs as a launch: for each of the first
     * tap_tiles 32-channel output tiles this launch also writes tap_out[b][tile][o*9 + t][H][W] = sum_{c in tile} w2[o][c][t] * out[c]
     * (fp32), w2 packed by tcs_pack_tap_weights.  tcs_taps_sum / tcs_flow_taps_step_grads / tcs_taps_propagate_s16 finish the sum over
     * tiles and taps.  With tap_out the S16 / fp32 outputs of those tiles are optional (out16 may be NULL). */
    const float* tap_weights;
    float* tap_out;
    int tap_nout, tap_tiles;
    float tap_unscale;              /* 2^-scale_log2 given to tcs_pack_tap_weights */
    /* TCS_EPI_BLEND9, optional: the skewed correlation pyramid of the frame (tcs_corr_build's pyr0..3; [B,H,W>>i,W] each, this launch's
     * grid).  The lane that has just computed a pixel's new coords1 also issues the 4 x (2r+2) tap loads the NEXT tcs_corr_lookup will
     * make for that pixel and discards the values: between two lookups ~300 MB of convolution traffic push the pyramid rows out of
     * L2 and the Infinity Cache, and the lookup is three dependent memory round trips long, so where its taps come from decides
     * its duration.  No effect on any result.  NULL = off. */
    const float* blend_warm_pyr[4];
    int blend_warm_radius;
    /* MFMA products per (k-step, tap): 0 or 3 = the fp16-split contraction (default); 1 = hi halves only, f16(x) . f16(w * 2^s) * 2^-s
     * with fp32 accumulation: the stage stages the hi plane of the inputs and the hi weight pieces only (as tcs_conv_desc.products).
     * The tap-partial fold (tap_*) stays a 3-product contraction.  tcs_conv2d_s16_group fuses two descriptors only when their counts
     * match.  Any other value is TCS_EINVAL. */
    int products;
} tcs_conv_s16_desc;

/* S16 glue of the loop: pool2x / interp (core/update.py:114-124), the up-blocks' InstanceNorm + LeakyReLU + skip
 * (core/utils/basic_layers.py:28-35,65-76), DispRefine's candidate stencil (core/update.py:259-289: 27 channels into 4 groups
 * for the 1x1 stem, the 9 candidates also as fp32 for the blend), one fp32 channel into an S16 tensor, and the blend
 * kernel writing the next iteration's flow input into a channel of the S16 motion features (core/update.py:126). */
int tcs_avgpool3s2_s16(const void* x, int B, int groups, int H, int W, void* out, int out_groups, tcs_stream_t stream);
int tcs_resize_bilinear_s16(const void* x, int B, int groups, int H, int W, int Ho, int Wo, void* out, int out_groups, tcs_stream_t stream);
size_t tcs_instance_norm_s16_workspace_bytes(int B, int groups, int H, int W);
int tcs_instance_norm_s16(const void* x, int B, int groups, int H, int W, float eps, int act, const void* addend, int addend_groups,
                          void* out, int out_groups, void* workspace, tcs_stream_t stream);
/* The apply half of tcs_instance_norm_s16 for statistics accumulated by the producing transposed convolution
 * (tcs_conv_s16_desc.in_stats; C = its Cout/4 channels, [H,W] = its OUTPUT grid): out = act((x - mean) / sqrt(var + eps)) + addend,
 * biased variance as nn.InstanceNorm2d. */
size_t tcs_deconv_in_stats_bytes(int B, int C, int H_in, int W_in);
int tcs_instance_norm_apply_s16(const void* x, int B, int groups, int H, int W, int act, const void* addend, int addend_groups,
                                void* out, int out_groups, const void* in_stats, int C, float eps, tcs_stream_t stream);
/* Tap partials (tcs_conv_s16_desc.tap_*): weights [nout][C][3][3] * 2^scale_log2 -> fp16-split MFMA A fragments in the producer's
 * accumulator channel order, rows o*9 + t (tcs_tap_weights_floats floats; choose scale_log2 like tcs_pack_conv_weight_f16x3);
 * tcs_taps_sum: out[B,nout,H,W] = (addend + bias + sum over tiles and in-image taps) * scale (addend, bias nullable);
 * tcs_flow_taps_step_grads = tcs_flow_step_grads with delta = bias[0] + taps (FlowHead's output, also written to delta_out when
 * non-NULL); tcs_taps_propagate_s16 = tcs_propagate_disparity_s16 with grad = (g5 + bias2 + taps) * post_scale (core/update.py:213),
 * also written to grad_out [B,2,H,W] when non-NULL. */
size_t tcs_tap_weights_floats(int nout, int C);
int tcs_pack_tap_weights(const float* w_oihw, int nout, int C, int scale_log2, float* packed, tcs_stream_t stream);
int tcs_taps_sum(const float* taps, int ntile, int nout, const float* bias, const float* addend, float scale, int B, int H, int W, float* out,
                 tcs_stream_t stream);
int tcs_flow_taps_step_grads(const float* coords1, const float* taps, int ntile, const float* bias, int B, int H, int W, float scale,
                             float* disp_q, float* grad, float* cands, float* delta_out, tcs_stream_t stream);
int tcs_taps_propagate_s16(const float* taps, int ntile, const float* bias2, const float* g5, float post_scale, const float* disp, int B, int H,
                           int W, float* grad_out, float* cand9, void* out16, int out_groups, tcs_stream_t stream);
int tcs_propagate_disparity_s16(const float* grad, const float* disp, int B, int H, int W, float* cand9, void* out16, int out_groups,
                                tcs_stream_t stream);
int tcs_s16_set_channel(const float* x, int B, int H, int W, void* s16, int groups_total, int channel, tcs_stream_t stream);
int tcs_softmax_blend_s16(const float* logits9, const float* cand, int cand_ctot, const float* disp_q,
                          int B, int H, int W, float* refined, float* delta_disp, float* coords1, float* flow_x,
                          void* flow_x_s16, int flow_x_s16_groups, int flow_x_s16_channel, tcs_stream_t stream);

/* HiddenstateUpdater.forward (core/update.py:57-68) as one launch: x = W2.LeakyReLU(w1*delta + b1) + b2; z,r = sigmoid(Wzr.[h,x] + bzr);
 * q = tanh(Wq.[r*h,x] + bq); h <- z*h + (1-z)*q, in place on the S16 hidden state (128 channels).  The three 1x1 weight
 * matrices are A-fragment images from tcs_pack_weight_frags: `natural_channels` leading input channels in S16 order (operands read
 * from an S16 tensor), the rest in accumulator order (operands handed over in registers by the preceding layer):
 * W2: natural 64; Wzr [256 x 192]: natural 0 (h is fetched in accumulator order too); Wq [128 x 192]: natural 0. */
size_t tcs_weight_frags_bytes(int Cout, int Cin);
int tcs_pack_weight_frags(const float* w_oi, int Cout, int Cin, int natural_channels, int scale_log2, void* packed, tcs_stream_t stream);
int tcs_hidden_update_s16(void* h, int h_groups, const float* delta, const float* w1, const float* b1, const void* W2, const float* b2,
                          float unscale2, const void* Wzr, const float* bzr, float unscale_zr, const void* Wq, const float* bq,
                          float unscale_q, int B, int H, int W, tcs_stream_t stream);

/* nn.Conv2d / ConvGRU step on S16 activations (core/update.py:16-17,26-36,57-68,77-87,103-111,198-214,291-305) */
int tcs_conv2d_s16(const tcs_conv_s16_desc* desc, tcs_stream_t stream);

/* n (1 or 2) INDEPENDENT convolutions of tcs_conv2d_s16 — no output of one is an input of another; same batch size — issued as ONE
 * launch where a grouped kernel exists for their tile instances (the pairs of the refinement loop: BasicMotionEncoder.convc2 | convf2
 * core/update.py:105-108, the second layers of DispGradPredictor's stems :200-205, DispRefine.context_compress | disp_f_stem :293-297),
 * otherwise one after the other.  Results are bit-equal to n calls of tcs_conv2d_s16 in either case; what the grouped launch saves is the
 * cross-queue dependency a fork / join of two graph branches costs.  tcs_conv2d_s16_group_fused: 1 when the two
 * descriptors would run as one launch (no launch is made). */
int tcs_conv2d_s16_group(const tcs_conv_s16_desc* const* descs, int n, tcs_stream_t stream);
int tcs_conv2d_s16_group_fused(const tcs_conv_s16_desc* const* descs, int n);

/* The tile instance tcs_conv2d_s16 would launch for a descriptor: the kernel's template parameters (ksize, stride, epilogue, cout tiles of
 * 32 per workgroup `mt`, output rows per workgroup `rows`, 16-channel k-steps per stage `ksteps`, LDS stages `nstage`, `row_split` and
 * `rows_per_wave` of the tile code's fifth digit, `taps` = 1 for the tap-partial instances), the MFMA products per k-step (a descriptor
 * that says 0 reports 3), the block -> XCD mapping digit `csplit` as the launch would use it, and the launch geometry (`blocks` per batch
 * element, `threads` = 64 * rows / rows_per_wave, dynamic LDS).  With tile_cfg = 0 this is the heuristic's choice.  Launches nothing and
 * dereferences no tensor pointer, so it also answers on a machine without a GPU.  Returns what tcs_conv2d_s16 would return before its
 * launch (TCS_OK, TCS_EINVAL, TCS_EUNSUPPORTED); `out` is written on TCS_OK only.  The tests take the library's instance table and the
 * instances of the model's layers from here instead of restating launch_s16_cfg / s16_heuristic (tests/s16_instances.py). */
typedef struct tcs_s16_instance { int ksize, stride, epilogue, mt, rows, ksteps, nstage, row_split, rows_per_wave, taps,
                                  products, csplit, blocks, threads; long long lds_bytes; } tcs_s16_instance;
int tcs_conv2d_s16_plan(const tcs_conv_s16_desc* desc, tcs_s16_instance* out);

/* ------------------------------------------------------------------------------------------------
 * The training objective (train_stereo.py:41-180, 362-399): targets, the four losses, metrics
 *
 * Scale 1/4 only (n_downsample 2): quarter-resolution maps are [B,*,H/4,W/4] (floor).  Per-element arithmetic is fp32 in the reference's
 * order with no FMA contraction; sums are fp64, written per block to `workspace` (tcs_loss_workspace_bytes; one workspace holds the
 * partials of every loss of a call) and finished in a fixed order by tcs_loss_finish, so that two calls are bit-equal.
 * valid_mode: 0 = float32 values as given, 1 = the trainer's rule (valid >= 0.5) & (|flow| < 700) on the dataset's float32 valid,
 * 2 = a bool / uint8 mask.  The valid map is [B,1,H,W] (or [B,H,W]); masks out are uint8.
 * ------------------------------------------------------------------------------------------------ */
#define TCS_LOSS_MAX_ITERS 64
#define TCS_LOSS_SEQ 1          /* `parts` bits of tcs_loss_finish */
#define TCS_LOSS_INIT 2
#define TCS_LOSS_GRAD 4
#define TCS_LOSS_NORM 8
/* tcs_loss_finish's fp64 output vector; a loss whose part is absent is NaN, as is a mean over an empty mask.  out32 holds the first
 * five in fp32.  FLAGS: bit 0 a non-finite flow prediction (or NaN flow_init / flow_mono), bit 1 a non-finite cost volume entry,
 * bit 2 a non-finite gradient prediction */
#define TCS_LOSS_OUT_TOTAL 0    /* seq + init + 0.25 norm + 5 grad */
#define TCS_LOSS_OUT_SEQ 1
#define TCS_LOSS_OUT_INIT 2
#define TCS_LOSS_OUT_NORM 3
#define TCS_LOSS_OUT_GRAD 4
#define TCS_LOSS_OUT_EPE 5      /* epe, epe_refine, epe_init, 1px, 3px, 5px, 1px_refine, 3px_refine, 5px_refine: 5 .. 13 */
#define TCS_LOSS_OUT_INIT_GT 14
#define TCS_LOSS_OUT_INIT_NM 15
#define TCS_LOSS_OUT_FMR 16     /* forward_mask_rate */
#define TCS_LOSS_OUT_FLAGS 17
#define TCS_LOSS_NOUT 18

size_t tcs_loss_workspace_bytes(int B, int H, int W, int iters);
/* flow_gt [B,1,H,W] + valid -> the median-pooled gradient of -flow [B,2,h,w] and its normal [B,3,h,w] (MedianPool2d(4,4): the lower
 * median of each 4x4 window, bit-equal to torch), their GT masks (< 5; n_x/n_z, n_y/n_z < 5), max_pool2d(valid, 4) != 0 (dense) and
 * bilinear(valid, align_corners=True) == 1 (sparse).  The full-resolution gradient is never written. */
int tcs_loss_targets(const float* flow_gt, const void* valid, int valid_mode, int B, int H, int W, float* grad_gt, float* norm_gt,
                     uint8_t* grad_mask, uint8_t* norm_mask, uint8_t* valid_dense, uint8_t* valid_sparse, tcs_stream_t stream);
/* the same from a full-resolution GT [B,C,H,W]: C = 2 gradients, C = 3 normals (valid_mode 0 or 2) */
int tcs_loss_targets_full(const float* gt, int C, const void* valid, int valid_mode, int B, int H, int W, float* out, uint8_t* gt_mask,
                          uint8_t* valid_dense, uint8_t* valid_sparse, tcs_stream_t stream);
/* sequence_loss: iteration i's flow_q-upsampled prediction at preds + i * iter_stride, its refined one at + refine_offset (floats;
 * [B,1,H,W] each) */
int tcs_sequence_loss(const float* preds, long long iter_stride, long long refine_offset, int iters, const float* flow_gt,
                      const void* valid, int valid_mode, const float* flow_mono, const float* flow_init, int B, int H, int W,
                      double* workspace, tcs_stream_t stream);
/* init_loss on cost_volume [B,D,H/4,W/4], the top-k of the masked, zero-filled candidates (1 <= k <= min(8, D)); `iters` locates the
 * partials in the workspace */
int tcs_init_loss(const float* cost_volume, int D, const float* flow_gt, const void* valid, int valid_mode, int B, int H, int W, int k,
                  float threshold, int iters, double* workspace, tcs_stream_t stream);
/* disp_grad_loss (grad_preds: iteration i [B,2,h,w] at + i * grad_stride) and disp_normal_loss (q_preds: flow_q at + i * q_stride,
 * flow_q_refine at + q_refine_offset, [B,1,h,w]); either may be NULL.  *_valid: the dense or sparse mask of tcs_loss_targets* */
int tcs_grad_normal_loss(const float* grad_preds, long long grad_stride, const float* q_preds, long long q_stride, long long q_refine_offset,
                         int iters, const float* grad_gt, const uint8_t* grad_mask, const uint8_t* grad_valid, const float* norm_gt,
                         const uint8_t* norm_mask, const uint8_t* norm_valid, int B, int H, int W, double* workspace, tcs_stream_t stream);
/* the partials of `parts` -> out [TCS_LOSS_NOUT] (fp64) and out32 [5]; loss_weights: a HOST array of `iters` doubles */
int tcs_loss_finish(const double* workspace, int parts, int B, int H, int W, int iters, int k, const double* loss_weights, double* out,
                    float* out32, tcs_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * The objective's backward.  Gradients of the four losses with respect to every prediction, float32,
 * each output element written exactly once (zeros included; no memset, no atomics: two calls are bit-equal).  Nothing is read on
 * the host: `upstream` is the DEVICE vector of five float32 d/d out32 (TCS_LOSS_OUT_TOTAL .. TCS_LOSS_OUT_GRAD: a part's effective
 * coefficient is its own entry plus the total's entry times the part's weight in the total, 1, 1, 0.25, 5), `counts` the DEVICE vector
 * tcs_loss_finish_counts wrote; a count of 0 (an empty mask) gives all-zero gradients.  loss_weights: a HOST array of `iters` doubles.
 * Masks, targets and arguments are the forward's; gradient buffers have the layout of the predictions they belong to.
 * ---------------------------------------------------------------------------------------------- */
#define TCS_LOSS_COUNT_SEQ 0    /* valid full-resolution pixels */
#define TCS_LOSS_COUNT_INIT 1   /* init_loss's quarter-resolution mask */
#define TCS_LOSS_COUNT_NORM 2
#define TCS_LOSS_COUNT_GRAD 3
#define TCS_LOSS_NCOUNTS 4
/* tcs_loss_finish, and the mask counts of `parts` (0 for an absent part) into counts [TCS_LOSS_NCOUNTS] (fp64, device) */
int tcs_loss_finish_counts(const double* workspace, int parts, int B, int H, int W, int iters, int k, const double* loss_weights,
                           double* out, float* out32, double* counts, tcs_stream_t stream);
/* sequence_loss: any of grad_preds (layout of preds), grad_mono, grad_init may be NULL (not wanted), not all three */
int tcs_sequence_loss_bwd(const float* preds, long long iter_stride, long long refine_offset, int iters, const float* flow_gt,
                          const void* valid, int valid_mode, const float* flow_mono, const float* flow_init, int B, int H, int W,
                          const double* loss_weights, const double* counts, const float* upstream, float* grad_preds, float* grad_mono,
                          float* grad_init, tcs_stream_t stream);
/* init_loss: the whole of grad_cost_volume [B,D,H/4,W/4] is written.  Among equal real values at the top-k boundary the lowest
 * candidate index is taken first; a zero-filled candidate takes a slot and receives nothing; a hinge of exactly 0 passes gradient */
int tcs_init_loss_bwd(const float* cost_volume, int D, const float* flow_gt, const void* valid, int valid_mode, int B, int H, int W, int k,
                      float threshold, const double* counts, const float* upstream, float* grad_cost_volume, tcs_stream_t stream);
/* disp_grad_loss and disp_normal_loss: grad_preds / q_preds as in tcs_grad_normal_loss, either may be NULL with its outputs */
int tcs_grad_normal_loss_bwd(const float* grad_preds, long long grad_stride, const float* q_preds, long long q_stride,
                             long long q_refine_offset, int iters, const float* grad_gt, const uint8_t* grad_mask, const uint8_t* grad_valid,
                             const float* norm_gt, const uint8_t* norm_mask, const uint8_t* norm_valid, int B, int H, int W,
                             const double* loss_weights, const double* counts, const float* upstream, float* grad_grad_preds,
                             float* grad_q_preds, tcs_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Differentiable convex upsampling and propagate-blend (tcs_mi355/train_ops.py).  The forwards take the
 * reference's own arguments; the backwards recompute the softmax from the saved inputs, write every wanted output element exactly
 * once (zeros included; no memset, no float atomics: two calls are bit-equal) and read nothing on the host.  A NULL gradient
 * output means "not wanted".
 * ---------------------------------------------------------------------------------------------- */
/* TCStereo.upsample_flow(flow, mask, scale=True) at factor 4 (tc_stereo.py:75-88): flow [B,1,H,W], mask [B,144,H,W] ->
 * flow_up [B,1,4H,4W], bit-equal to tcs_convex_upsample(disp = -flow, clip = 0). */
int tcs_upsample_flow(const float* flow, const float* mask, int B, int H, int W, float* flow_up, tcs_stream_t stream);
/* both upsamplings of one iteration (tc_stereo.py:213-214) on one shared mask: bit-equal to tcs_convex_upsample_pair(-flow_a, -flow_b) */
int tcs_upsample_flow_pair(const float* flow_a, const float* flow_b, const float* mask, int B, int H, int W, float* up_a, float* up_b,
                           tcs_stream_t stream);
/* floats of the caller-owned workspace of the two backwards below when n_flows (0, 1 or 2) flow gradients are wanted */
size_t tcs_convex_upsample_backward_workspace_floats(int B, int H, int W, int n_flows);
/* grad_up [B,1,4H,4W] (16-byte aligned) -> grad_mask [B,144,H,W] and grad_flow [B,1,H,W]; flow is read for grad_mask only and may be
 * NULL without it.  One launch; a wanted grad_flow adds the workspace's fixed-order 9-term gather as a second, small one. */
int tcs_convex_upsample_backward(const float* flow, const float* mask, const float* grad_up, int B, int H, int W, float* grad_mask,
                                 float* grad_flow, float* workspace, tcs_stream_t stream);
/* the pair's: the mask was detached in output a, so grad_mask comes from flow_b and grad_up_b alone and is bit-equal to
 * tcs_convex_upsample_backward(flow_b, mask, grad_up_b)'s; an upstream gradient that no wanted output reads may be NULL */
int tcs_convex_upsample_pair_backward(const float* flow_b, const float* mask, const float* grad_up_a, const float* grad_up_b, int B, int H,
                                      int W, float* grad_mask, float* grad_flow_a, float* grad_flow_b, float* workspace, tcs_stream_t stream);
/* update.py:294,298-300 in one launch: refined [B,1,H,W] = sum_k softmax(logits9 - max)_k * cand_k(disp_grads, disp), the candidates
 * of tcs_propagate_disparity formed in registers; bit-equal to tcs_softmax_blend on tcs_propagate_disparity's output. */
int tcs_refine_blend(const float* logits9, const float* disp_grads, const float* disp, int B, int H, int W, float* refined,
                     tcs_stream_t stream);
/* grad_refined [B,1,H,W] -> grad_logits [B,9,H,W], grad_disp_grads [B,2,H,W]; disp gets no gradient (the reference detaches it) */
int tcs_refine_blend_backward(const float* logits9, const float* disp_grads, const float* disp, const float* grad_refined, int B, int H,
                              int W, float* grad_logits, float* grad_disp_grads, tcs_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Differentiable gate stages of the recurrent cells (tcs_mi355/train_ops.py): what ConvGRU (update.py:81-85),
 * Lightfuse (:30-34) and HiddenstateUpdater (:62-66) do around their second convolution, one launch each.  All tensors are
 * [B,C,H,W] float32 with contiguous planes and contiguous channels; every INPUT has its own batch stride in elements (>= C*H*W), so
 * chunk / split views along the channels of a wider tensor are read in place.  Outputs, upstream gradients and gradients are
 * contiguous.  Context terms (cr, cz, cq) may be NULL = zero.  16-byte accesses are used when C*H*W, every batch stride and every
 * base address are multiples of 16 bytes, 4-byte accesses otherwise.  The backwards recompute the gates from the inputs and write
 * every wanted output element exactly once (no memset, no atomics: two calls are bit-equal); a NULL gradient output means "not
 * wanted", and the gradient of a context term IS the gradient of its pre-activation.  A NULL required pointer, a batch stride
 * below C*H*W, a non-positive size or no wanted gradient is TCS_EINVAL before any HIP call.
 * ---------------------------------------------------------------------------------------------- */
/* rh = sigmoid(r_pre + cr) * h */
int tcs_gru_reset(const float* r_pre, long long r_pre_stride, const float* h, long long h_stride, const float* cr, long long cr_stride,
                  int B, int C, int H, int W, float* rh, tcs_stream_t stream);
/* grad_r_pre (= d cr) = g h r (1 - r), grad_h = g r; h is read for grad_r_pre only and may be NULL without it */
int tcs_gru_reset_backward(const float* r_pre, long long r_pre_stride, const float* h, long long h_stride, const float* cr,
                           long long cr_stride, const float* grad_rh, int B, int C, int H, int W, float* grad_r_pre, float* grad_h,
                           tcs_stream_t stream);
/* z = sigmoid(z_pre + cz), q = tanh(q_pre + cq); h_new = (1 - z) h + z q (z_keeps_h = 0, ConvGRU) or z h + (1 - z) q (z_keeps_h != 0,
 * Lightfuse and HiddenstateUpdater) */
int tcs_gru_update(const float* z_pre, long long z_pre_stride, const float* q_pre, long long q_pre_stride, const float* h,
                   long long h_stride, const float* cz, long long cz_stride, const float* cq, long long cq_stride, int z_keeps_h, int B,
                   int C, int H, int W, float* h_new, tcs_stream_t stream);
/* z_keeps_h = 0: grad_q_pre (= d cq) = g z (1 - q^2), grad_z_pre (= d cz) = g (q - h) z (1 - z), grad_h = g (1 - z); z_keeps_h != 0: z and
 * 1 - z change places in grad_q_pre and grad_h, and grad_z_pre changes sign.  q_pre and cq are read for grad_z_pre and grad_q_pre only,
 * h for grad_z_pre only; they may be NULL otherwise */
int tcs_gru_update_backward(const float* z_pre, long long z_pre_stride, const float* q_pre, long long q_pre_stride, const float* h,
                            long long h_stride, const float* cz, long long cz_stride, const float* cq, long long cq_stride,
                            const float* grad_h_new, int z_keeps_h, int B, int C, int H, int W, float* grad_z_pre, float* grad_q_pre,
                            float* grad_h, tcs_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* TCS_MI355_H */
