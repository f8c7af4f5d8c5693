/*
 * ufr.h -- C ABI of libufr.so: the MI355X (gfx950) implementation of UFORecon's per-ray
 * volume-rendering path.
 *
 * Every entry point replaces a piece of the reference's Python hot path (paths relative
 * to the upstream repo, code1/...).  Plain pointers and sizes only; all tensor pointers
 * are DEVICE pointers to contiguous fp32 (int64 for ray indices) unless marked "host".
 * Kernels are enqueued on the given HIP stream and never synchronise.  Return value:
 * 0 on success, negative ufr_status otherwise; ufr_last_error() gives the message
 * (thread-local).  Shapes use the reference's names: NV source views, RN rays, SN samples
 * per ray, P = RN*SN points, H x W image, h x w = H/4 x W/4 feature maps.
 */
#ifndef UFR_H
#define UFR_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* ufr_stream; /* hipStream_t */

enum ufr_status {
  UFR_OK = 0,
  UFR_ERR_ARG = -1,       /* bad shape / null pointer / unsupported size */
  UFR_ERR_HIP = -2,       /* a HIP runtime call failed */
  UFR_ERR_WORKSPACE = -3, /* workspace too small */
  UFR_ERR_RANGE = -4      /* a value left the range the split-precision planes can hold (see ufr_status_poll) */
};

/* Version of this header's ABI (argument lists, struct layouts, packed-blob layout).  ufr_version() returns the value
 * the library was built with: a binding must refuse a library whose version differs (uforecon_amd/_lib.py does). */
#define UFR_ABI_VERSION 507

#define UFR_MAX_VIEWS 7
#define UFR_NUM_STAGES 3
#define UFR_TOKEN_DIM 80 /* [img feat 32 | volume 24 | similarity 16 | depth PE 8], ray_transformer.py:258-281 */
#define UFR_RAY_DIM 88   /* token dim + 8 order PE, ray_transformer.py:301-303 */

int ufr_version(void);
const char* ufr_last_error(void);

/* ------------------------------------------------------------------ weights
 * Device pointers to the per-ray parameters in the reference's own layout (nn.Linear
 * weight = row-major [out][in]); names follow the state_dict keys under
 * "ray_transformer." (parameter inventory). */
typedef struct ufr_layer_weights { /* one LoFTREncoderLayer, attention/transformer.py:7-58 */
  const float *q, *k, *v, *merge; /* [d][d]            */
  const float *mlp0;              /* [2d][2d]          */
  const float *mlp2;              /* [d][2d]           */
  const float *norm1_w, *norm1_b, *norm2_w, *norm2_b; /* [d] */
} ufr_layer_weights;

typedef struct ufr_mlp3_weights { /* Linear-ReLU-Linear-ReLU-Linear with bias */
  const float *w0, *b0, *w2, *b2, *w4, *b4;
} ufr_mlp3_weights;

typedef struct ufr_raw_weights {
  ufr_mlp3_weights pre_sim;   /* pre_sim_mlp.{0,2,4}: 8->32->32->16          (ray_transformer.py:128-132) */
  ufr_layer_weights view;     /* density_view_transformer.layers.0, d=80     (ray_transformer.py:135)     */
  ufr_layer_weights ray;      /* density_ray_transformer.layers.0, d=88      (ray_transformer.py:138)     */
  ufr_mlp3_weights density;   /* DensityMLP.{0,2,4}: 88->32->16->1           (ray_transformer.py:147-150) */
  ufr_mlp3_weights radiance;  /* linear_radianceweight_1_softmax: 83->16->8->1 (ray_transformer.py:159-163) */
  const float* view_token;    /* viewToken.view_token [80]                   (ray_transformer.py:325-331) */
  const float* variance;      /* deviation_network.variance, scalar          (single_variance_network.py:8) */
} ufr_raw_weights;

/* Matrix precision of the dense layers.  Every entry point that runs dense layers takes a `precision` argument
 * (ufr_render_args has a field); the forward and the backward of one training step must be given the same value
 * (uforecon_amd/autograd.py records the forward's in the autograd context).
 *   UFR_PRECISION_DEFAULT the process default, FP32 unless ufr_set_matrix_precision changed it (a convenience for
 *                       command-line tools; library code that pairs a forward with a backward passes an explicit mode)
 *   UFR_PRECISION_FP32  fp32-grade FORWARD: every product as three fp16 plane products (22+ significand bits per operand),
 *                       fp32 accumulate -- the mode all 1e-4 parity statements refer to.  The BACKWARD of this mode splits
 *                       its operands into bf16 hi + lo planes (16 significand bits per operand, three products, fp32
 *                       accumulate: "bf16x3"): gradient-grade, not fp32-grade -- every gradient tensor within 5e-5 of its
 *                       scale of the reference's fp32 autograd (tests/test_gpu_backward.py; the bench line says
 *                       `bwd_operand_dtype`).
 *   UFR_PRECISION_16BIT the "bf16" training mode of the reference's mixed-precision recipe (BASELINE configs[4]): one
 *                       16-bit plane per operand (fp16 hi planes in the forward, bf16 operands in the backward GEMMs and
 *                       weight gradients), fp32 accumulation, LayerNorm / attention / softmax / compositor in fp32.
 *                       Tolerance: 2e-3 of scale on forward rows, 3e-2 on gradients (tests/test_gpu_backward.py). */
#define UFR_PRECISION_DEFAULT (-1)
#define UFR_PRECISION_FP32 0
#define UFR_PRECISION_16BIT 1
int ufr_set_matrix_precision(int mode); /* sets what UFR_PRECISION_DEFAULT resolves to (FP32 or 16BIT) */
int ufr_get_matrix_precision(void);

/* Sticky range status of the current device.  The dense layers run on fp16 planes whose power-of-two scales are chosen
 * when the weights are packed: per matrix from max |w| (any finite weight fits), per layer from an analytic upper bound
 * of the layer's input that starts at the bound of the token features and is carried through the matrices' infinity
 * norms, the LayerNorm gains and the biases.  The bound of the token features is MEASURED: ufr_frame_prepare takes the
 * maximum magnitude of the frame's feature maps and volume features while it re-lays them out, and ufr_render_rays /
 * ufr_weights_fit_frame re-derive the layer exponents (scalars of the table; the weight planes do not change) for a frame
 * beyond the bound the table serves -- ufr_weights_pack_for's input_abs_max, default 4094, is only the floor and an
 * optional override.  With a true input bound no layer can overflow.  The kernels never synchronise, so a violation
 * (tokens handed to ufr_aggregate / ufr_view_transform directly, beyond the floor and without a frame) raises a
 * device-side sticky flag instead of failing the launch:
 *   bit 0  a dense-layer input of a transformer kernel left the range of its planes: a token feature beyond the bound
 *          the table serves, or +-inf -- ufr_weights_fit_frame with the frame the tokens come from, or repack with a
 *          larger input_abs_max
 *   bit 1  NaN among the externally supplied inputs of a transformer kernel (token rows, dir); +-inf inputs and
 *          internally produced overflows raise bit 0
 *   bit 2  ufr_weights_pack met a parameter that is not finite
 * ufr_status_poll copies the flag to the host on `stream`; with synchronize != 0 it waits for the stream and returns
 * UFR_ERR_RANGE (message: which bits) when the flag is set, clearing it.  Without synchronize it returns what an
 * EARLIER poll / launch has already delivered.  ufr_render_rays, ufr_aggregate, ufr_view_transform and
 * ufr_ray_transform poll lazily: each enqueues the copy after its kernels and fails with UFR_ERR_RANGE on entry when a
 * previous call's copy arrived set -- one call late, without a host synchronisation in the ray loop.  `flags_out`
 * (nullable) receives the bits.  Across streams: every copy waits (on its own stream) for the last report-and-clear, so a
 * poll on another stream than the one that reported cannot miss bits raised since; a bit raised again between a report's
 * copy and its clear is reported with the next violation rather than at once (reports can be late, never spurious). */
int ufr_status_poll(ufr_stream stream, int32_t synchronize, int32_t* flags_out);
/* The same, restricted to the bits of `mask`: other bits stay set for whoever polls for them (uforecon_amd.ops.PackedWeights
 * checks a fresh pack with mask 4, so that an unrelated, still unreported activation overflow does not fail a valid pack). */
int ufr_status_poll_bits(ufr_stream stream, int32_t synchronize, int32_t mask, int32_t* flags_out);

/* Re-orders the dense matrices into MFMA A-fragment order (one 16x16 output tile x 16
 * input features = 64 lanes x float4, zero padded) so the kernels stream them with
 * contiguous 1 KiB wave loads.  Call again whenever the parameters change. */
size_t ufr_packed_weights_bytes(void);
int ufr_weights_pack(const ufr_raw_weights* raw, void* packed, ufr_stream stream);   /* input_abs_max = 4094 */
/* The same for feature maps and volume features bounded by input_abs_max (positive, finite) -- what the encoder hands to
 * ufr_frame_prepare; for ufr_aggregate / ufr_view_transform callers: columns 0..55 and 72..79 of x_tokens (the 16
 * pre-similarity columns are bounded from pre_sim_mlp's own weights, the positional columns by 1).  The bound
 * only sets the exponents the activations' planes carry (a pessimistic one costs no accuracy: the planes keep 22
 * significand bits down to 2^-17 of each layer's bound), so state it generously. */
int ufr_weights_pack_for(const ufr_raw_weights* raw, void* packed, float input_abs_max, ufr_stream stream);
/* (ufr_weights_fit_frame, declared with the frame handle below: the table follows a frame's measured bound) */
/* Host-only description of that re-ordering (for tests / other bindings): for every packed
 * float, param_id (index into the pointer list of ufr_raw_weights in declaration order, -1 =
 * zero padding) and elem (flat element index inside that parameter).  Arrays of
 * ufr_packed_weights_bytes()/4 int32 each.  No GPU needed. */
int ufr_pack_plan(int32_t* param_id, int32_t* elem);
/* The packed blob is [fp32 region: ufr_packed_fp32_floats() floats | fp16 plane region: ufr_packed_f16_halfwords()
 * 16-bit words | bf16 plane region of the backward kernels: ufr_packed_bwd_halfwords() 16-bit words | 16-byte tail].
 * The bf16 region holds the TRANSPOSED dense matrices of the data-gradient chains (hi = bf16(w), lo = bf16(w - hi), same
 * fragment order as the forward planes).  The fp16 plane region holds the dense layers of both transformer chains as two fp16
 * planes per weight (w' = 2^s_M w with the matrix's exponent s_M: hi = fp16(w'), lo = fp16(w' - hi); plane 0/1) for the
 * split-precision MFMA path;
 * ufr_pack_plan_f16 describes it like ufr_pack_plan (one entry per halfword, plus the plane).  Of the fp32 region
 * ufr_weights_pack fills only the trailing vector fragments (biases, LayerNorm, view token) and, behind them, the scale
 * table: per dense matrix M (ufr_packed_scale_table_offset() floats into the blob, 4 floats each, in the order of
 * csrc/ufr_layout.h: Mat) {2^a_M, 2^-(s_M + a_M), 2^(s_M + a_M), 2^s_M}, then the two kernels' scalar lists and the weight
 * statistics the exponents derive from (kept for ufr_weights_fit_frame); the kernels read nothing else of the region.
 * ufr_weights_pack does not synchronise: a parameter that is not finite raises bit 2 of the sticky status -- call
 * ufr_status_poll(stream, 1, ...) after packing to fail at once (uforecon_amd.ops.PackedWeights does), or let the next
 * compute entry point report it. */
size_t ufr_packed_scale_table_offset(void);
int ufr_packed_scale_table_entries(void);
size_t ufr_packed_fp32_floats(void);
size_t ufr_packed_f16_halfwords(void);
size_t ufr_packed_bwd_halfwords(void);
int ufr_pack_plan_bwd(int32_t* param_id, int32_t* elem, int32_t* plane);   /* the bf16 region, like ufr_pack_plan_f16 */
int ufr_pack_plan_f16(int32_t* param_id, int32_t* elem, int32_t* plane);

/* ------------------------------------------------------------------ frame
 * Per-frame tensors produced by the encoder (model.py:780-808), in the reference layout.
 * ufr_frame_prepare re-lays them out channel-last into `workspace` (one tap = one
 * contiguous line), measures max |value| of the feature maps and volume features on the way (a device word inside
 * `workspace`: what ufr_weights_fit_frame reads) and records the camera constants; the result is immutable during the
 * ray loop (model.py:814-823). */
typedef struct ufr_frame_desc {
  int32_t NV, H, W;               /* full-resolution image size; feature maps are H/4 x W/4          */
  const float* source_imgs;       /* (NV,3,H,W)   batch['source_imgs']                               */
  const float* depth_info;        /* (NV,H,W)     batch['depth_info'] (model.py:807-808)             */
  const float* feat;              /* (NV,32,h,w)  source_imgs_feat                                   */
  const float* match;             /* (NV,32*(NV-1),h,w) match_feature[0]; NULL: ufr_project_gather needs sim8_in */
  const float* vol_feat[UFR_NUM_STAGES];   /* (NV,8,D,Hs,Ws) feature_volume[stage]['feature_volume']; all NULL (with
                                              vol_weight): ufr_project_gather needs vol24_in              */
  const float* vol_weight[UFR_NUM_STAGES]; /* (NV,1,D,Hs,Ws) feature_volume[stage]['weight_volume']   */
  int32_t vol_D[UFR_NUM_STAGES], vol_H[UFR_NUM_STAGES], vol_W[UFR_NUM_STAGES];
  /* camera constants, HOST pointers (copied) */
  const float* source_poses;      /* (NV,4,4) normalize @ K_pad @ w2c  (dtu_test_sparse.py:409-416)  */
  const float* source_cam_pos;    /* (NV,3)   source_poses_inv[:, :3, 3] (ray_transformer.py:187)    */
  const float* ref_cam_pos;       /* (3)      ref_pose_inv[:3, 3]        (ray_transformer.py:185)    */
  const float* w2c_row2;          /* (NV,4)   w2cs[s_idx:, 2, :]         (ray_transformer.py:240-243) */
  float vol_near, vol_far;        /* batch['near_fars'][0][0]            (model.py:328)              */
} ufr_frame_desc;

/* Host-side handle filled by ufr_frame_prepare (device pointers into `workspace`, sizes, camera
 * constants).  Plain data: copy it freely; it stays valid while `workspace` and the borrowed
 * depth_info tensor are alive. */
typedef struct ufr_frame { uint64_t opaque[160]; } ufr_frame;

size_t ufr_frame_workspace_bytes(const ufr_frame_desc* d);
int ufr_frame_prepare(const ufr_frame_desc* d, void* workspace, size_t workspace_bytes, ufr_frame* out,
                      ufr_stream stream);
/* The activation exponents of `packed` follow a frame: when the feature bound ufr_frame_prepare measured for `frame`
 * exceeds the one the table was derived for, the table is re-derived on the device for the next power of two above it
 * (one 64-thread kernel; otherwise it returns at once).  Asynchronous, no host read-back.  The bound only grows until the
 * next ufr_weights_pack, so the backward of an earlier forward stays in range whatever frames are fitted in between.
 * ufr_render_rays does this itself; callers of the stepwise entry points (ufr_project_gather -> ufr_aggregate ...) call it
 * once per (frame, pack) -- uforecon_amd.ops does, in FrameHandle-taking calls.  Replaces "state input_abs_max for this
 * checkpoint": the reference loads any checkpoint without side information (main.py:186-190).
 * OWNERSHIP: the refit WRITES the scale table inside `packed` (ufr_render_rays does too, although it takes the blob as
 * const void*: the planes are const, the table is not).  A packed blob therefore belongs to ONE stream at a time: kernels of
 * another stream, or of an earlier call on another stream, that still read the table while a refit runs would race.  Fit on
 * the stream the render / aggregate calls use (stream order then serialises refit and readers), and give every
 * concurrently rendered frame stream its own packed copy.  Activations taped under an older, smaller table stay valid:
 * the bound only grows, and a backward recomputes with the table it finds. */
int ufr_weights_fit_frame(void* packed, const ufr_frame* frame, ufr_stream stream);

/* ------------------------------------------------------------------ per-op entry points
 * (each mirrors one reference function; used by the drop-in Python classes and the parity
 * tests; ufr_render_rays below chains them for whole-frame inference) */

/* FixedSampler.sample_ray with near/far (encoder_utils/sampler.py:15-50).
 * U: (SN,RN) uniforms exactly as torch.rand((SN,RN)) produced them.  z_out: (RN,SN). */
int ufr_sample_fixed(const float* near, const float* far, const float* U, float* z_out,
                     int32_t RN, int32_t SN, ufr_stream stream);

/* ImportanceSampler.sample_ray (sampler.py:74-108) fused with the coarse+fine merge
 * (model.py:466-470).  weight,z: (RN,SN); U2: (PN,RN) as drawn by torch.rand(PN,RN);
 * z_fine: (RN,PN) sorted (may be NULL); z_all: (RN,SN+PN) sorted.
 * "Sorted" is the order of torch.sort(stable=True), a total order on every float: numbers ascending with -0 == +0, every
 * NaN behind +inf, and equal values -- NaNs among themselves included -- in the order of their index in the list that is
 * sorted (z_all: the SN coarse positions, then the new ones in their own sorted order).  So every slot of every output is
 * written whatever a ray holds (a NaN or infinite weight, position or uniform; a weight sum that overflows): a ray that
 * is not finite comes out not finite, in its own slots, and changes nothing of any other ray. */
int ufr_sample_importance_merge(const float* weight, const float* z, const float* U2, float* z_fine,
                                float* z_all, int32_t RN, int32_t SN, int32_t PN, ufr_stream stream);

/* points = ray_o + z * ray_d (sampler.py:47).  ray_o: (3) or (RN,3) by `ray_o_stride` (0 or 3). */
int ufr_points(const float* ray_o, int32_t ray_o_stride, const float* ray_d, const float* z, float* points,
               int32_t RN, int32_t SN, ufr_stream stream);

/* Projection + all gathers of one pass: camera.get_coord_ref_ndc (misc/camera.py:378-407),
 * query_cond_info (model.py:218-305), query_depth_from_volume (model.py:350-390) and
 * ray_transformer.py:185-281 up to the token assembly (incl. pre_sim_mlp).
 * Outputs: x_tokens (P,NV,80); rgb (P,NV,4) [r,g,b,mask]; dir (P,NV,4) [dx,dy,dz,0].
 * Optional outputs (may be NULL): sim8 (P,8) = cond_info['feat_info'], vol24 (P,24) = the blended frustum lookup,
 * xy (NV,P,2) = points_pixel, mask_z (NV,P) = mask_valid.
 * Optional inputs (may be NULL): vol24_in (P,24) / sim8_in (P,8) replace the kernel's own frustum lookup / pair
 * similarity -- RayTransformer.forward receives them as `fea_volume` / cond_info['feat_info']
 * (ray_transformer.py:175, 199, 265); a frame prepared without volumes / matching features requires them. */
int ufr_project_gather(const ufr_frame* frame, const ufr_raw_weights* raw, const float* ray_o,
                       int32_t ray_o_stride, const float* ray_d, const float* z, int32_t RN, int32_t SN,
                       float* x_tokens, float* rgb, float* dir, float* sim8, float* vol24, float* xy,
                       float* mask_z, const float* vol24_in, const float* sim8_in, ufr_stream stream);

/* View transformer + ray transformer + SRDF / radiance heads (ray_transformer.py:283-320).
 * radiance: (P,3); srdf: (RN,SN).  workspace >= ufr_aggregate_workspace_bytes(RN,SN).
 * Optional debug outputs (may be NULL): view_out (P,NV+1,80), ray_out (P,88).
 * One call handles at most P * (NV + 1) * 80 < 2^30 token values (6.7 M points at NV = 3; the view-transformer kernel
 * addresses its buffers with 32-bit offsets): UFR_ERR_ARG beyond it -- chunk the points (ufr_render_rays does). */
size_t ufr_aggregate_workspace_bytes(int32_t RN, int32_t SN, int32_t NV);
int ufr_aggregate(const void* packed_weights, const float* x_tokens, const float* rgb, const float* dir,
                  int32_t RN, int32_t SN, int32_t NV, float* radiance, float* srdf, void* workspace,
                  float* view_out, float* ray_out, int32_t precision, ufr_stream stream);

/* VolumeRenderer.render (encoder_utils/renderer.py:7-48) with SingleVarianceNetwork
 * (single_variance_network.py:10-11).  z,srdf: (RN,SN); radiance: (RN,SN,3); variance: device scalar.
 * row (nullable, (RN,SN) int32): the colour of slot (ray, s) is radiance[row[ray][s]] -- the sample pool of the two-pass
 * step (ufr_sample_importance_pool); NULL = slot order.  PRECONDITION: row is what ufr_sample_importance_pool writes, per
 * ray a permutation of that ray's rows of the pool; it is not range-checked here or in ufr_composite_bwd.
 * Outputs: rgb (RN,3), depth (RN), opacity (RN), weight (RN,SN); any may be NULL except depth. */
int ufr_composite(const float* z, const float* radiance, const int32_t* row, const float* srdf, const float* variance,
                  int32_t RN, int32_t SN, float* rgb, float* depth, float* opacity, float* weight,
                  ufr_stream stream);

/* ------------------------------------------------------------------ backward (training step, BASELINE configs[4])
 * The reference gets these from autograd over code1/model.py:540-566 (training_step: infer -> losses).  Which
 * tensors receive gradients: every ray_transformer.* parameter, deviation_network.variance and the six sampled
 * volumes (through which feature_volume.cost_reg_2.* trains); not the 2-D feature maps / matching features (their
 * producer is frozen, model.py:82-83) and not the sample positions (model.py:456-457 detaches them).
 * Each *_bwd entry point is the adjoint of the forward entry point of the same name and takes that call's inputs
 * again (activations are recomputed, not stored).  Parameter gradients are ACCUMULATED (+=) into caller-owned
 * tensors of the parameters' own shapes: zero them once per step. */
#define UFR_NUM_PARAMS 40
typedef struct ufr_raw_grads {
  float* p[UFR_NUM_PARAMS]; /* one per pointer of ufr_raw_weights, in its declaration order; same shapes */
} ufr_raw_grads;

/* Adjoint of ufr_composite (autograd of renderer.py:19-46).  d_rgb (RN,3), d_depth (RN), d_opacity (RN),
 * d_weight (RN,SN): gradients of the outputs, any may be NULL (= zero).  Outputs: d_radiance (rows as `radiance`: slot
 * order, or pool rows through `row`; overwritten, or added to when accumulate != 0 -- every row is touched once per call),
 * d_srdf (RN,SN) (overwritten); d_variance: device scalar, ACCUMULATED. */
int ufr_composite_bwd(const float* z, const float* radiance, const int32_t* row, const float* srdf, const float* variance,
                      int32_t RN, int32_t SN, const float* d_rgb, const float* d_depth, const float* d_opacity,
                      const float* d_weight, float* d_radiance, int32_t accumulate, float* d_srdf, float* d_variance,
                      ufr_stream stream);

/* The training loss of a ray batch and its cotangents in one launch (code1/model.py:552-566):
 *   loss = weight_rgb (mse(rgb_c, rgb_gt) + mse(rgb_f, rgb_gt)) + weight_depth (l1(depth_c, depth_gt | valid) + l1(depth_f, ...)),
 *   valid = (depth_gt != 0) & (depth_gt >= near) & (depth_gt <= far), the two L1 terms 0 when no ray is valid.
 * rgb_* (B*RN,3), depth_* (B*RN): both passes' rendered colours / ray depths and the ground truth, batch-major;
 * near_far: near = near_far[b * nf_stride], far = near_far[b * nf_stride + 1] of batch element b (batch['near_fars'][b, 0]:
 * nf_stride = V*2).  Outputs: loss[5] = {total, rgb_c, rgb_f, depth_c, depth_f} (the reference logs all five);
 * d_rgb_c (B*RN,3), d_depth_c (B*RN), d_rgb_f, d_depth_f = d total / d input (sign(0) = 0 in the L1 terms, as torch). */
int ufr_render_loss(const float* rgb_c, const float* depth_c, const float* rgb_f, const float* depth_f, const float* rgb_gt,
                    const float* depth_gt, const float* near_far, int32_t nf_stride, int32_t B, int32_t RN, float weight_rgb,
                    float weight_depth, float* loss, float* d_rgb_c, float* d_depth_c, float* d_rgb_f, float* d_depth_f,
                    ufr_stream stream);

/* Adjoint of ufr_aggregate (autograd of ray_transformer.py:283-320).  x_tokens / rgb / dir: the forward's inputs;
 * token0 (P,80): the view transformer's token-0 output = the first RN*SN*80 floats of the forward's workspace;
 * d_radiance (P,3), d_srdf (RN,SN): gradients of the forward's outputs.  Accumulates the gradients of the view / ray
 * transformer, DensityMLP, radiance-weight MLP and view-token parameters into `grads`; writes d_pv (P,40): gradient
 * w.r.t. token columns 32..71 (24 frustum features | 16 pre_sim_mlp outputs) summed over the NV view tokens of a
 * point -- the input of ufr_project_gather_bwd.  packed_weights: ufr_weights_pack of the same parameters (the view
 * transformer's backward re-runs the forward kernel with a tape and walks the chain backwards on transposed weight planes
 * of the packed blob; its weight gradients are one streaming contraction over the tokens).  The workspace holds the tape
 * and the cotangent tiles: ~15 KB per point at NV = 3.  (ABI 500: the `debug_ray` dump argument of earlier versions, ignored
 * since the round-4 kernels, is gone.) */
size_t ufr_aggregate_bwd_workspace_bytes(int32_t RN, int32_t SN, int32_t NV);
int ufr_aggregate_bwd(const ufr_raw_weights* raw, const ufr_raw_grads* grads, const void* packed_weights, const float* x_tokens,
                      const float* rgb, const float* dir, const float* token0, int32_t RN, int32_t SN, int32_t NV,
                      const float* d_radiance, const float* d_srdf, float* d_pv, void* workspace,
                      int32_t precision, ufr_stream stream);

/* Adjoint of ufr_project_gather w.r.t. the sampled volumes and pre_sim_mlp (autograd of model.py:350-390 and
 * ray_transformer.py:268).  sim8 (P,8): the forward's `sim8` output; d_pv (P,40) from ufr_aggregate_bwd.
 * row (nullable, (RN,SN) int32): d_pv / sim8 are POOL tensors and slot (ray, s) owns row row[ray][s] of d_pv (the two-pass
 * step hands over all merged samples of a ray in one call; sim8 is only summed over, any row order).
 * grad_vol_feat[s] (NV,8,D,Hs,Ws) / grad_vol_weight[s] (NV,1,D,Hs,Ws): reference layout, written whole -- overwritten, or
 * added to when accumulate != 0 (the scatter itself goes into a channel-last record volume in `workspace`,
 * ufr_project_gather_bwd_workspace_bytes(frame) bytes = 1.33 x the volumes: nine lanes of one atomic instruction add the
 * nine values of a voxel corner as ONE L2 transaction, then one coalesced pass writes these tensors);
 * both arrays NULL: only the pre_sim_mlp gradients (accumulated into `grads`) are computed, no workspace needed.
 * `accumulate` is a bit set: UFR_GBWD_ACCUMULATE, and UFR_GBWD_WORKSPACE_ZEROED = `workspace` is all zero on entry
 * (ordered before this call on `stream`) -- the library then skips its own memset (0.9 GB at the configs[4] size).
 * The call LEAVES THE WORKSPACE ZERO: the scatter marks the groups of 8 voxels it adds into, and the pass that writes the
 * gradient tensors reads -- and zeroes again -- only those (a step's rays reach a fraction of the voxels).  A caller that
 * keeps the workspace between calls therefore zero-fills it once and passes UFR_GBWD_WORKSPACE_ZEROED from then on (a
 * call that returned an error leaves it undefined: fill it again). */
#define UFR_GBWD_ACCUMULATE 1
#define UFR_GBWD_WORKSPACE_ZEROED 2
#define UFR_GBWD_NO_PRESIM 4 /* the volume scatter only: the pre_sim_mlp gradients come from another call (both arrays NULL),
                                which a caller may put on another stream -- the two halves share no output */
size_t ufr_project_gather_bwd_workspace_bytes(const ufr_frame* frame);
int ufr_project_gather_bwd(const ufr_frame* frame, const ufr_raw_weights* raw, const ufr_raw_grads* grads,
                           const float* ray_o, int32_t ray_o_stride, const float* ray_d, const float* z, int32_t RN,
                           int32_t SN, const float* sim8, const float* d_pv, const int32_t* row,
                           float* const* grad_vol_feat, float* const* grad_vol_weight, int32_t accumulate, void* workspace,
                           int32_t precision, ufr_stream stream);

/* ------------------------------------------------------------------ the two halves of ufr_aggregate, and the sample pool
 * The fine pass of `infer` (model.py:455-473) re-evaluates all SN+PN merged samples, but a sample's gathers and
 * view-transformer output depend on its own position only: evaluating the PN NEW samples and re-using the coarse pass's
 * rows gives the same numbers (ufr_render_rays does that internally).  These entry points expose the pieces so that the
 * training step can do the same, forwards and backwards:
 *   ufr_sample_importance_pool = ufr_sample_importance_merge that also returns the new positions z_new (RN,PN), sorted
 *     along the ray, and for every merged slot its row in the pool [RN*SN coarse rows (ray-major) | RN*PN new rows]: row (RN,SN+PN) int32.
 *     z_all / z_new stand in the order stated at ufr_sample_importance_merge, and row[ray] is ALWAYS a permutation of the
 *     ray's own rows { ray*SN + s } and { RN*SN + ray*PN + p } (row p of the new block holds z_new[ray][p]), also for a ray
 *     whose weights, positions or uniforms are NaN or infinite: the producer is the one place that guarantees the table.
 *     PRECONDITION of every `row` argument below and of ufr_composite / ufr_composite_bwd / ufr_project_gather_bwd: per ray
 *     a permutation of that ray's pool rows, as this entry point writes it.  The kernels index the pool with it -- the
 *     adjoints WRITE through it -- and check no range;
 *   ufr_view_transform / ufr_ray_transform = the view-transformer and ray-transformer halves of ufr_aggregate
 *     (token0 (P,80), radiance (P,3) | token0 rows of the RN*SN samples -> srdf (RN,SN)); `row` (nullable, (RN,SN) int32)
 *     maps slot (ray, s) to its row of token0 (NULL = slot order), so the fine pass reads the pool in place;
 *   ufr_view_transform_bwd / ufr_ray_transform_bwd = the corresponding halves of ufr_aggregate_bwd (d_token0 comes out
 *     in d_token0_a, written at the same rows `row` names -- overwritten, or added to when accumulate != 0 (the coarse
 *     pass adds its cotangents onto the fine pass's coarse rows); d_token0_b (nullable) is the second partial buffer of
 *     the interface's earlier two-sweep form: zero-filled when not accumulating, so that a + b is the gradient; pass
 *     both, or a and NULL, to ufr_view_transform_bwd). */
int ufr_sample_importance_pool(const float* weight, const float* z, const float* U2, float* z_all, float* z_new,
                               int32_t* row, int32_t RN, int32_t SN, int32_t PN, ufr_stream stream);
int ufr_view_transform(const void* packed_weights, const float* x_tokens, const float* rgb, const float* dir, int32_t P,
                       int32_t NV, float* token0, float* radiance, int32_t precision, ufr_stream stream);
size_t ufr_ray_transform_workspace_bytes(int32_t SN);
int ufr_ray_transform(const void* packed_weights, const float* token0, const int32_t* row, int32_t RN, int32_t SN,
                      float* srdf, void* workspace, int32_t precision, ufr_stream stream);
size_t ufr_ray_transform_bwd_workspace_bytes(int32_t RN, int32_t SN);   /* tape, per-ray attention state, cotangent tiles */
int ufr_ray_transform_bwd(const ufr_raw_weights* raw, const ufr_raw_grads* grads, const void* packed_weights, const float* token0,
                          const int32_t* row, int32_t RN, int32_t SN, const float* d_srdf, float* d_token0_a, float* d_token0_b,
                          int32_t accumulate, void* workspace, int32_t precision, ufr_stream stream);
size_t ufr_view_transform_bwd_workspace_bytes(int32_t P, int32_t NV);
int ufr_view_transform_bwd(const ufr_raw_weights* raw, const ufr_raw_grads* grads, const void* packed_weights,
                           const float* x_tokens, const float* rgb, const float* dir, const float* d_token0_a,
                           const float* d_token0_b, const float* d_radiance, int32_t P, int32_t NV, float* d_pv, void* workspace,
                           int32_t precision, ufr_stream stream);
/* The same in stages, for callers that overlap them with independent work on other streams (uforecon_amd/autograd.py does):
 *   TAPE   the forward again, recording the activations into the workspace -- needs only the forward's inputs, so it can run
 *          beside the ray transformer's backward (pointers of later stages may be NULL);
 *   DGRAD  the data-gradient chain: reads the tape, d_token0_a/b, d_radiance; writes d_pv and the cotangent tiles;
 *   WGRAD  the weight-gradient contractions: read tape and cotangent tiles, add into `grads` -- nothing downstream waits for
 *          them, so they can run beside ufr_project_gather_bwd (which needs d_pv only).
 * The SAME workspace must be passed to every stage, and the stages must execute in this order (stream events are the
 * caller's business).  stages = UFR_BWD_STAGE_ALL is ufr_view_transform_bwd. */
#define UFR_BWD_STAGE_TAPE 1
#define UFR_BWD_STAGE_DGRAD 2
#define UFR_BWD_STAGE_WGRAD 4
#define UFR_BWD_STAGE_ALL 7
int ufr_view_transform_bwd_stages(const ufr_raw_weights* raw, const ufr_raw_grads* grads, const void* packed_weights,
                                  const float* x_tokens, const float* rgb, const float* dir, const float* d_token0_a,
                                  const float* d_token0_b, const float* d_radiance, int32_t P, int32_t NV, float* d_pv,
                                  void* workspace, int32_t stages, int32_t precision, ufr_stream stream);
/* Training forward WITH the tape: what ufr_view_transform / ufr_ray_transform compute (same numbers), recorded into the
 * workspace of the matching backward call, whose TAPE stage is then skipped (stages = DGRAD | WGRAD): nothing is computed
 * twice.  View: the points [p0, p0 + P) of a pool of P_total points that ONE backward will walk; x_tokens / rgb / dir /
 * token0 / radiance point at the range's first row; p0 (and P, unless the range closes the pool) must be multiples of
 * ufr_view_tape_block_points(NV); workspace: ufr_view_transform_bwd_workspace_bytes(P_total, NV).  Ray: one pass;
 * workspace: ufr_ray_transform_bwd_workspace_bytes(RN, SN). */
int32_t ufr_view_tape_block_points(int32_t NV);
int ufr_view_transform_tape(const void* packed_weights, const float* x_tokens, const float* rgb, const float* dir, int32_t P,
                            int32_t NV, float* token0, float* radiance, void* workspace, int32_t p0, int32_t P_total,
                            int32_t precision, ufr_stream stream);
int ufr_ray_transform_tape(const void* packed_weights, const float* token0, const int32_t* row, int32_t RN, int32_t SN,
                           float* srdf, void* workspace, int32_t precision, ufr_stream stream);
int ufr_ray_transform_bwd_stages(const ufr_raw_weights* raw, const ufr_raw_grads* grads, const void* packed_weights,
                                 const float* token0, const int32_t* row, int32_t RN, int32_t SN, const float* d_srdf,
                                 float* d_token0_a, float* d_token0_b, int32_t accumulate, void* workspace, int32_t stages,
                                 int32_t precision, ufr_stream stream);   /* the ray transformer's backward likewise */

/* ------------------------------------------------------------------ whole-path inference
 * UFORecon.infer(extract_geometry=True) (model.py:393-478) for RN rays of one frame:
 * ray gather by index, near/far / cam_ray_d.z, coarse pass, importance sampling + merge, fine
 * pass.  Depth is the ray length (model.py:821 converts to z-depth: see depth_z). */
typedef struct ufr_render_args {
  const ufr_frame* frame;     /* from ufr_frame_prepare                                   */
  const void* packed_weights; /* from ufr_weights_pack                                    */
  const ufr_raw_weights* raw; /* same parameters, reference layout (pre_sim_mlp, variance) */
  const int64_t* ray_idx;     /* (RN) indices into H*W                      (model.py:409) */
  const float* ray_d;         /* (3,H*W) batch['ray_d']                                   */
  const float* cam_ray_d;     /* (3,H*W) batch['cam_ray_d']                (model.py:424) */
  float ray_o[3];             /* batch['ray_o']                                           */
  float near_z, far_z;        /* batch['near_fars'][0,0,:]              (model.py:416-421) */
  const float* U1;            /* (SN,RN) coarse jitter uniforms         (sampler.py:42)    */
  const float* U2;            /* (PN,RN) importance uniforms; NULL if coarse_only (sampler.py:86) */
  int32_t RN, SN, PN;         /* rays, coarse samples, fine samples                        */
  int32_t coarse_only;        /* args.test_coarse_only                  (model.py:449-452) */
  int32_t precision;          /* UFR_PRECISION_*                                           */
  /* outputs (device) */
  float* depth;               /* (RN) ray-length depth                                     */
  float* depth_z;             /* (RN) depth * cam_ray_d.z (model.py:821), may be NULL      */
  float* rgb;                 /* (RN,3)                                                    */
  float* srdf;                /* (RN,S) S = SN or SN+PN, may be NULL                        */
  float* z_all;               /* (RN,S) sample distances of the returned pass, may be NULL  */
  int32_t chunk_rays;         /* rays per internal launch group (0 = library default)       */
  int32_t n_streams;          /* >1: chunks are issued round-robin on that many library-owned side streams
                                 (forked from / joined to `stream`); needs n_streams x the workspace   */
  void* workspace;            /* >= ufr_render_workspace_bytes(chunk_rays,SN,PN,NV) (x n_streams)     */
  size_t workspace_bytes;
} ufr_render_args;

size_t ufr_render_workspace_bytes(int32_t chunk_rays, int32_t SN, int32_t PN, int32_t NV);
int32_t ufr_default_chunk_rays(void);
int ufr_render_rays(const ufr_render_args* a, ufr_stream stream);
/* ufr_render_rays that also hands out the COARSE pass (ABI 507, additive): the same checks, launches and bits in a's
 * outputs; the one difference is that the coarse compositor writes its colour and ray-length depth to rgb_coarse (RN,3) /
 * depth_coarse (RN) instead of the workspace.  Refuses coarse_only (one pass: call ufr_render_rays).  a->cam_ray_d == NULL
 * is UFORecon.infer(extract_geometry=False) as validation_step calls it (model.py:423: near/far as given, no division by
 * cam_ray_d.z); depth_z must then be NULL. */
int ufr_render_rays_pair(const ufr_render_args* a, float* rgb_coarse, float* depth_coarse, ufr_stream stream);

/* ---- the scores and previews of a validation frame (ABI 507, additive) -----------------------------------------
 * UFORecon.validation_step's metrics (model.py:708-726) and save arithmetic (:731, :734, :742) for one frame of n rays.
 * ufr_frame_metrics: rgb_c / rgb_f (n,3) the coarse / fine colours, rgb_gt (3,n) PLANAR (batch['ref_img']), depth_c / depth_f
 *   / depth_gt (n): device fp32.  out8: eight device doubles
 *     [0] [1]  MSE coarse / fine    mean over 3n of (x - y)^2                                   (F.mse_loss)
 *     [2] [3]  PSNR coarse / fine   -10 log10(mean((clamp(x,0,1) - clamp(y,0,1))^2) + 1e-8)     (piq.psnr, data_range 1)
 *     [4] [5]  L1 depth coarse / fine over the pixels with depth_gt != 0 && near <= depth_gt <= far; 0 when there is none
 *     [6]      the number of such pixels
 *     [7]      max of depth_c (NaN if one is NaN, as np.max)
 *   Differences are formed in double from the fp32 inputs.  One pass over the inputs on a grid that depends on n alone: double
 *   partials per thread, reduced across the wave and the block in a fixed order, one row per block; a second one-block
 *   kernel adds the rows in index order.  No atomics: a rerun gives the same bits.  NaN inputs propagate as in torch (a NaN
 *   depth_gt fails the mask).  workspace >= ufr_frame_metrics_workspace_bytes(n) (device).  1 <= n < 2^31 / 3.
 * ufr_frame_preview_u8: rgb8 (n,3) = (uint8)(rgb * 255) and, when depth is given, depth8 (n) = (uint8)((depth * depth_scale)
 *   / (max * depth_scale) * 255) with max = (float)*depth_max (DEVICE: &out8[7]); every product and the quotient are fp32,
 *   unfused, so the bytes equal numpy's for the same expression; the float -> uint8 step truncates towards zero and keeps the
 *   low 8 bits (values beyond int32 saturate first, NaN gives 0).  rgb / rgb8 or depth / depth_max / depth8 may be NULL as a
 *   group.  Neither call synchronises; every argument error is UFR_ERR_ARG. */
size_t ufr_frame_metrics_workspace_bytes(int32_t n);
int ufr_frame_metrics(const float* rgb_c, const float* rgb_f, const float* rgb_gt, const float* depth_c, const float* depth_f,
                      const float* depth_gt, float near, float far, int32_t n, double* out8, void* workspace, ufr_stream stream);
int ufr_frame_preview_u8(const float* rgb, const float* depth, const double* depth_max, float depth_scale, int32_t n, uint8_t* rgb8,
                         uint8_t* depth8, ufr_stream stream);
/* ufr_depth_gt_prepare: the ground-truth ray depth of one view of the DTU training layout (code1/dataset/dtu_train.py: read_depth
 *   :249-254, :429, :485) from pfm = the (Hs,Ws) fp32 rows of `Depths_raw/<scan>/depth_map_%04d.pfm` AS STORED (device):
 *     depth[y, x] = (float)((double)(S[2 (y + y0), 2 (x + x0)] * scale_factor) / cam_ray_z[y * W + x])
 *   with S the picture the file holds -- row r of S is stored row Hs - 1 - r when bottom_up (read_pfm's flip; every PFM file),
 *   row r otherwise.  The factor 2 is OpenCV's INTER_NEAREST at fx = fy = 0.5, restated and not compared; the half-size
 *   picture has rint(Hs / 2) x rint(Ws / 2) pixels (half to even) and the crop (y0, x0, H, W) must lie inside it (DTU: 1200 x
 *   1600 -> 600 x 800, crop 512 x 640 at (44, 80)).  The product is fp32 (the reference multiplies float32 arrays), the
 *   quotient double: cam_ray_z (H*W) is row 2 of the reference's cam_ray_d, which it leaves in float64 (device).  A hole (0)
 *   stays 0; the scale of the PFM header is not applied (read_pfm returns it and the reference drops it).  Does not
 *   synchronise; every argument error is UFR_ERR_ARG. */
int ufr_depth_gt_prepare(const float* pfm, int32_t Hs, int32_t Ws, int32_t bottom_up, int32_t y0, int32_t x0, int32_t H, int32_t W,
                         float scale_factor, const double* cam_ray_z, float* depth, ufr_stream stream);

/* Per-kernel HIP-event timing of the most recent ufr_render_rays on this thread when
 * enabled (for bench.py's roofline line).  names/ms arrays of length `cap`; returns count. */
/* ---- correlation-volume construction (first step) -------------------------------------
 * Replaces, for one frame and one cascade stage, the loop body of DepthNet.forward step 2
 * (code1/encoder_utils/fmt/TransMVSNet.py:66-97): homo_warping_trans (code1/encoder_utils/fmt/module.py:329-367)
 * of every source view onto the D depth hypotheses of the reference view, similarity = mean over channels of
 * warped x reference, and -- when pixel-wise view weights are given -- the weighted aggregate over the views.
 * The (C,D,H,W) warped volume is never materialised.
 *   ref_fea [C][H][W], src_fea [NS][C][H][W], depth_values [D][H][W], view_weights [NS][H][W] (nullable): device, fp32
 *   rel_proj: HOST array [NS][12], rows of (src_proj_new @ inverse(ref_proj_new))[:3,:4] (module.py:340-342)
 *   similarity [NS][D][H][W] (nullable), aggregated [D][H][W] (nullable; needs view_weights): device outputs
 *   C in {4,8,16,32,64}; 1 <= NS <= UFR_MAX_VIEWS                                                              */
size_t ufr_correlate_workspace_bytes(int32_t C, int32_t H, int32_t W, int32_t NS);
int ufr_frustum_correlate(const float* ref_fea, const float* src_fea, const float* rel_proj, const float* depth_values,
                          const float* view_weights, int32_t C, int32_t H, int32_t W, int32_t D, int32_t NS,
                          float* similarity, float* aggregated, void* workspace, size_t workspace_bytes,
                          ufr_stream stream);

/* ---- 3-D convolutions of the frustum construction's U-Nets ---------------------
 * One layer of CostRegNet / CostRegNetWeight (code1/encoder_utils/fmt/module.py:469-543; Conv3d / Deconv3d = convolution
 * + BatchNorm + ReLU, :110-187): 3x3x3, padding 1, fp32, volumes CHANNEL-LAST [B][D][H][W][C] (a (B,1,D,H,W) tensor is
 * both layouts at once).
 *   mode   UFR_CONV3D_S1 stride 1 | UFR_CONV3D_S2 stride 2 (output ceil(n/2)) | UFR_CONV3D_T2 transposed, stride 2,
 *          output_padding 1 (output 2n)
 *   weight the layer's weight in the checkpoint's layout: conv (cout,cin,3,3,3), transposed conv (cin,cout,3,3,3)
 *   bias (cout, nullable); bn_scale / bn_shift (cout, nullable together): eval-mode BatchNorm folded to
 *          y = conv * scale + shift with scale = gamma / sqrt(var + eps), shift = beta - mean * scale; relu != 0: ReLU
 *   skip   (nullable) channel-last tensor of the output's shape, added after the activation (the U-Net's "convK + ...")
 *   out    channel-last [B][Do][Ho][Wo][cout]; with out_ncdhw != 0 the reference's (B,cout,Do,Ho,Wo) instead, and then
 *          weight2 (cout2,cin,3,3,3) / out2 (B,cout2,Do,Ho,Wo) may name a second head on the same input whose output goes
 *          through a sigmoid (CostRegNetWeight's `features` + `weights`, module.py:541-543) -- both heads in one pass.
 *   out_absmax (nullable; ABI 503; channel-last outputs with at most 16 channels -- the vector kernel): a device float the
 *          caller has zeroed, raised to max |out| (skip included): the bound ufr_conv3d_planes wants of its input.
 * Supported (cin, cout + cout2): the layers of the two networks with base_channels 8:
 *   S1: (1,8) (16,16) (32,32) (64,64) (8,1) (8,8) (8,8+1);  S2: (8,16) (16,32) (32,64);  T2: (64,32) (32,16) (16,8).    */
#define UFR_CONV3D_S1 0
#define UFR_CONV3D_S2 1
#define UFR_CONV3D_T2 2
int ufr_conv3d(const float* in, const float* weight, const float* weight2, const float* bias, const float* bn_scale,
               const float* bn_shift, const float* skip, float* out, float* out2, int32_t B, int32_t D, int32_t H,
               int32_t W, int32_t cin, int32_t cout, int32_t cout2, int32_t mode, int32_t relu, int32_t out_ncdhw,
               float* out_absmax, ufr_stream stream);
/* Backward of the plain layers (bias, no BatchNorm / activation): CostRegNetWeight, i.e. `feature_volume.cost_reg_2` -- the
 * one producer the reference trains (model.py:72-87; module.py:502-543).  B, D, H, W, cin, cout, mode describe the FORWARD
 * layer (its input extent and channels); tensors are channel-last.
 *   ufr_conv3d_bwd_data    d_in (B,D,H,W,cin) = adjoint of the layer applied to d_out (the layer's output extent, cout
 *                          channels) [+ accumulate (same shape as d_in, nullable): a gradient that arrives on two paths,
 *                          the U-Net's skip additions].  The forward kernel itself: mirrored taps for stride 1, the
 *                          transposed / strided twin for the strided / transposed layers, all on the forward weight as it
 *                          stands.  cin = 1: no `accumulate`.
 *   ufr_conv3d_bwd_weight  d_weight (the reference's parameter layout: (cout,cin,3,3,3); transposed: (cin,cout,3,3,3)) +=
 *                          sum over voxels of d_out x in per tap; d_bias (cout, nullable) += column sums of d_out.
 *                          Both are ACCUMULATED into (zero them, or keep a running sum over frames). */
int ufr_conv3d_bwd_data(const float* d_out, const float* weight, const float* accumulate, float* d_in, int32_t B, int32_t D,
                        int32_t H, int32_t W, int32_t cin, int32_t cout, int32_t mode, ufr_stream stream);
int ufr_conv3d_bwd_weight(const float* in, const float* d_out, float* d_weight, float* d_bias, int32_t B, int32_t D, int32_t H,
                          int32_t W, int32_t cin, int32_t cout, int32_t mode, ufr_stream stream);

/* CostRegNetWeight's two heads (module.py:541-543: `features` 8 -> 8 and `weights` 8 -> 1 on the same input) in one pass:
 * d_weight (8,8,3,3,3) += d_out x in, d_weight2 (1,8,3,3,3) += d_out2 x in per tap; in (B,D,H,W,8), d_out (B,D,H,W,8),
 * d_out2 (B,D,H,W,1) channel-last.  Both are ACCUMULATED into.  (ABI 503)                                                  */
int ufr_conv3d_bwd_weight_heads(const float* in, const float* d_out, const float* d_out2, float* d_weight, float* d_weight2, int32_t B,
                                int32_t D, int32_t H, int32_t W, ufr_stream stream);

/* ---- the same layers on the 16-bit matrix cores (ABI 503) -------------------------------------------------------
 * The stride-1 layers of the U-Nets (module.py:469-543: conv2, conv4, conv6, `prob`, `features` + `weights`; and, with
 * flip != 0, their data gradients) as an implicit GEMM on
 * v_mfma_f32_16x16x32_f16 with the input brick staged once through LDS (csrc/conv3d_planes.hip).  Every fp32 product is
 * three fp16 plane products accumulated in fp32 (22 significand bits): not bit-identical to ufr_conv3d, within ~1e-6 of it.
 *   in_absmax   device pointer to ONE float >= max |in| (> 0 unless the tensor is zero): the planes' power-of-two scale.
 *               ufr_absmax measures it; a layer's out_absmax is the next layer's in_absmax.
 *   out_absmax  (nullable, channel-last outputs only) device float the caller has zeroed; raised to max |out| (skip included)
 *   flip        0: `weight` (cout,cin,3,3,3).  1: the data gradient of a stride-1 layer -- `weight` is that layer's FORWARD
 *               weight (cin of this call, cout of this call, 3,3,3) and the taps are mirrored (ufr_conv3d_bwd_data, S1).
 *   mode        UFR_CONV3D_S1; UFR_CONV3D_S2 (conv1 / conv3 / conv5, and -- on the transposed layers' forward weights as they
 *               stand -- the data gradients of conv11 / conv9 / conv7); UFR_CONV3D_T2 (conv7 / conv9 / conv11 -- `weight`
 *               (cin,cout,3,3,3) -- and, on the strided layers' forward weights, the data gradients of conv5 / conv3 / conv1):
 *               the transposed layer runs as a 2 x 2 x 2 convolution of the input grid with 8 x cout output rows, one group
 *               per output parity class
 *   workspace   ufr_conv3d_planes_workspace_bytes(cin, cout, cout2, mode) bytes (the weights' planes); 0 = combination not
 *               supported here (use ufr_conv3d).  S1: cin in {8, 16} with cout + cout2 <= 16, (32, 32), (64, 64); S2: (8, 16),
 *               (16, 32), (32, 64); T2: (16, 8), (32, 16), (64, 32).
 *   planes_ready  0: the planes are made from `weight` (/ `weight2`) by this call (three small launches).  1: `workspace` still
 *               holds the planes a call with planes_ready = 0 made from the SAME weights, flip and channel counts (frozen
 *               weights: once per checkpoint, not once per frame); the caller vouches for that.
 * bias / bn_scale / bn_shift / relu / skip / out_ncdhw / weight2 / out2 as for ufr_conv3d.                              */
size_t ufr_conv3d_planes_workspace_bytes(int32_t cin, int32_t cout, int32_t cout2, int32_t mode);
int ufr_conv3d_planes(const float* in, const float* in_absmax, const float* weight, const float* weight2, const float* bias,
                      const float* bn_scale, const float* bn_shift, const float* skip, float* out, float* out2,
                      float* out_absmax, int32_t B, int32_t D, int32_t H, int32_t W, int32_t cin, int32_t cout, int32_t cout2,
                      int32_t mode, int32_t relu, int32_t out_ncdhw, int32_t flip, void* workspace, size_t workspace_bytes, int32_t planes_ready,
                      ufr_stream stream);
/* *absmax = max(*absmax, max |x[0..n)|) (device float; zero it first).  One pass at HBM speed.                          */
int ufr_absmax(const float* x, size_t n, float* absmax, ufr_stream stream);

/* ---- TSDF fusion -------------------------------------------------------------------
 * Replaces the reference's `integrate` kernel (tsdf_fusion.py:77-152, a CUDA string compiled through pycuda) and the
 * launch loop of TSDFVolume.integrate (:240-265): one depth (+ colour) observation into the (X,Y,Z) fp32 volumes,
 * z fastest.  tsdf / weight / color, depth_im [H][W], color_im [H][W] (folded b*65536+g*256+r, nullable): device;
 * dim, origin, cam_intr (3x3 row-major), cam_pose (4x4 row-major camera-to-world): host.
 * integrate_color = 0 reproduces the reference (its colour block is unreachable).                             */
int ufr_tsdf_integrate(float* tsdf, float* weight, float* color, const int32_t* dim, const float* origin,
                       float voxel_size, float trunc_margin, const float* cam_intr, const float* cam_pose,
                       const float* depth_im, const float* color_im, int32_t im_h, int32_t im_w, float obs_weight,
                       int32_t integrate_color, ufr_stream stream);

/* ---- marching cubes over a fused TSDF volume (ABI 504) ----------------------------------------------------
 * Replaces skimage.measure.marching_cubes_lewiner(tsdf_vol, level=0) in TSDFVolume.get_mesh / get_point_cloud
 * (tsdf_fusion.py:319-357) on the device: vol (X,Y,Z) fp32, z fastest (device), dim host int32[3], each >= 2, fewer than
 * 2^31 voxels.  Output: an indexed triangle mesh with shared vertices, in voxel-index coordinates:
 *   a corner is below iff v < level; the edge p -> p + e_a (values a, b) carries a vertex iff exactly one end is below,
 *   at p with p[a] + t, t = (level - a) / (b - a); vertex order = (owner voxel p linear index, axis x < y < z);
 *   normal = +grad f (central differences, one-sided at the border) interpolated with t, normalised ((0,0,0) if zero);
 *   faces in (cube linear index, case-table order) order, wound so that the right-hand normal points towards increasing
 *   f.  Ambiguous cube faces are split around their below corners (tools/gen_mcubes_table.py): closed surfaces come out
 *   closed and consistently oriented.  No atomics: the output is deterministic.
 * Two calls with the same vol, dim, level and workspace (>= ufr_marching_cubes_workspace_bytes(dim), 4 B per voxel + a
 * little, device):
 *   ufr_marching_cubes_count: counts_host[0] = V, counts_host[1] = F.  SYNCHRONISES the stream (the host needs the two
 *     counts to size the outputs); V or F >= 2^31 is an error.
 *   ufr_marching_cubes_emit: verts (V,3) fp32, normals (V,3) fp32, faces (F,3) int32 (device; nullable when their count
 *     is 0).  n_verts / n_faces: the capacities of those arrays (the counts the first call returned); nothing beyond
 *     them is written.  Does not synchronise.
 * ufr_marching_cubes_table: host copy of the 256-case table, UFR_MC_TABLE_ROW int8 per case (edge triples, -1 padded;
 *   numbering in tools/gen_mcubes_table.py).  out_len >= 256 * UFR_MC_TABLE_ROW; returns UFR_MC_TABLE_ROW.        */
#define UFR_MC_TABLE_ROW 16
size_t ufr_marching_cubes_workspace_bytes(const int32_t* dim);
int ufr_marching_cubes_count(const float* vol, const int32_t* dim, float level, void* workspace, size_t workspace_bytes,
                             int32_t* counts_host, ufr_stream stream);
int ufr_marching_cubes_emit(const float* vol, const int32_t* dim, float level, void* workspace, size_t workspace_bytes,
                            float* verts, float* normals, int32_t* faces, int32_t n_verts, int32_t n_faces, ufr_stream stream);
int ufr_marching_cubes_table(int8_t* out, int32_t out_len);

/* ---- the similarity field of a frame's matching features (ABI 507, additive) ----------------------------------
 * UFORecon.extract_fields with query_cond_info (model.py:891-911, 218-305): u (X,Y,Z) fp32, z fastest (device; the layout
 * ufr_marching_cubes_* takes), voxel (i,j,k) at p = (gx[i], gy[j], gz[k]).  gx / gy / gz are HOST fp32 tables of dim[0] /
 * dim[1] / dim[2] entries (the reference's torch.linspace per axis); they are consumed before the call returns.
 * Per view v: q = pose[v] (p, 1), xy = q.xy / q.z (ufr_project_gather's arithmetic), NO depth mask; the frame's match maps
 * sampled bilinearly with align_corners=True and border clamping; for every pair (a, b), 0 <= a <= b <= NV-2, the sides (view
 * a, chunk b) and (view b+1, chunk a), 8 groups of 4 channels each, cosine similarity by ufr_project_gather's sim8 expression;
 * u = the mean over the pairs, then over the 8 groups.
 * Two options, both off (= the reference) by default:
 *   n_vis (X,Y,Z) uint8 (device, nullable): the number of views with q.z > 0 and -1 < x < 1 and -1 < y < 1.
 *   min_views > 0: a voxel with n_vis < min_views gets u = -1.0 exactly (border clamping gives a voxel outside every
 *     frustum an arbitrary similarity).
 * One stated difference: a voxel whose projected x or y is not finite in some view (q.z = 0) gets u = -1.0; the reference
 * would sample at NaN there.
 * Asynchronous, no workspace.  UFR_ERR_ARG before any launch: a frame that is not prepared or has no match maps, a null
 * table / dim / u, a dim below 2, X Y Z >= 2^31, min_views outside 0 .. NV.                                          */
int ufr_similarity_field(const ufr_frame* frame, const float* gx, const float* gy, const float* gz, const int32_t* dim, float* u,
                         uint8_t* n_vis, int32_t min_views, ufr_stream stream);

/* ---- DTU chamfer evaluation of a mesh or point cloud (ABI 505) ----------------------------------------------
 * The device side of evaluation/dtu_eval.py: sample the mesh (:68-91), thin the cloud to the density (:105-115), nearest
 * neighbour distances and their means (:139-155).  Positions and distances are fp64 as in the reference; every count n, V, F
 * below is 1 .. 2^31 - 1.  uforecon_amd/dtu_eval.py is the caller that strings them together.
 *
 * ufr_mesh_sample_*: verts (V,3) fp64, faces (F,3) int32 (device).  Per triangle (p0, p1, p2), v1 = p1 - p0, v2 = p2 - p0,
 *   l = |v|, area2 = |v1 x v2| (sums of three squares left to right, no fused multiply-add): none if area2 <= 0; else
 *   thr = density * sqrt(l1 * l2 / area2), n = floor(l / thr), none if n1 or n2 is 0; else the points (v1 * a + v2 * b) + p0
 *   for a = (i + 0.5) / n1, b = (j + 0.5) / n2, i = 0..n1, j = 0..n2 where a + b < 1, in (triangle, i, j) order.  A
 *   triangle with an index outside 0..V-1 gives none.  Two calls with the same arguments and workspace
 *   (>= ufr_mesh_sample_workspace_bytes(F), device):
 *     ufr_mesh_sample_count: *total_host = the number of points.  SYNCHRONISES the stream.
 *     ufr_mesh_sample_emit: out (capacity,3) fp64 (device); nothing beyond capacity is written.  Does not synchronise.
 * ufr_points_cell_keys: keys[i] = the 63-bit Morton key (x the highest of every bit triple) of point i's grid cell,
 *   floor((p - origin) / cell) per axis clamped to 0 .. 2^21 - 1.  points (n,3) fp64, keys (n) int64: device; origin: host
 *   double[3]; cell > 0.  Does not synchronise.  The two calls below take points sorted by this key.
 * ufr_points_thin: the keep-mask of the reference's sequential thinning: in the order given by rank (a permutation of
 *   0..n-1, int32), a point is kept iff no earlier kept point lies within (dx*dx + dy*dy) + dz*dz <= radius*radius.
 *   points / keys / rank: sorted by key, keys made with cell >= radius * (1 + 1e-9) and an origin below every point by at
 *   least one cell.  state (n) uint8 (device): 1 = kept, 2 = removed on return.  Runs rounds of a fixpoint whose result
 *   does not depend on scheduling; SYNCHRONISES the stream once per round; *rounds_host (nullable) = rounds taken.  A round
 *   without progress, or more than n rounds, is UFR_ERR_HIP (cannot happen for a valid rank).
 * ufr_points_nn_dist: dist[i] = the distance from query i to its nearest reference point, sqrt((dx*dx + dy*dy) + dz*dz),
 *   exact wherever it is < max_dist; elsewhere some value >= max_dist (+inf when nothing is near).  query (nq,3), dist (nq):
 *   device, any order (a wave is fastest when its queries are neighbours); ref (nr,3) with ref_keys (nr): sorted by key, with
 *   the origin and cell the keys were made with.  mean_out (device double[2], nullable): the sum of the distances < max_dist
 *   and their count, summed in a fixed order (the same bits run after run).  workspace >=
 *   ufr_points_nn_dist_workspace_bytes(nq) (device).  Does not synchronise.                                         */
size_t ufr_mesh_sample_workspace_bytes(int64_t F);
int ufr_mesh_sample_count(const double* verts, const int32_t* faces, int64_t V, int64_t F, double density, void* workspace,
                          size_t workspace_bytes, int64_t* total_host, ufr_stream stream);
int ufr_mesh_sample_emit(const double* verts, const int32_t* faces, int64_t V, int64_t F, double density, void* workspace,
                         size_t workspace_bytes, double* out, int64_t capacity, ufr_stream stream);
int ufr_points_cell_keys(const double* points, int64_t n, const double* origin, double cell, int64_t* keys, ufr_stream stream);
size_t ufr_points_thin_workspace_bytes(int64_t n);
int ufr_points_thin(const double* points, const int64_t* keys, const int32_t* rank, int64_t n, double radius, uint8_t* state,
                    void* workspace, size_t workspace_bytes, int32_t* rounds_host, ufr_stream stream);
size_t ufr_points_nn_dist_workspace_bytes(int64_t nq);
int ufr_points_nn_dist(const double* query, int64_t nq, const double* ref, const int64_t* ref_keys, int64_t nr,
                       const double* origin, double cell, double max_dist, double* dist, double* mean_out, void* workspace,
                       size_t workspace_bytes, ufr_stream stream);

/* ---- depth-map fusion (ABI 506) ------------------------------------------------------------------------------
 * The device side of code1/encoder_utils/depth_fusion.py (MVSNet-style geometric-consistency filtering of rendered depth
 * maps into a point cloud); uforecon_amd/depth_fusion.py is the caller that strings these together.
 *
 * ufr_depth_consistency: reproject_with_depth + check_geometric_consistency (:35-90) of one reference view against its S
 *   source views (1 <= S <= UFR_DEPTH_MAX_SOURCES), and the accumulation of filter_depth (:176-192).  ref_depth (H,W) fp32
 *   (device); src_depth: HOST array of S device pointers, map s being (src_hw[2s], src_hw[2s+1]) fp32 -- sizes need not
 *   equal the reference's; src_hw: host int32[2S].  mats: DEVICE table of S records of UFR_DEPTH_PAIR_DOUBLES fp64, the
 *   row-major matrices the caller forms with the reference's own numpy expressions in the dtypes its inputs have, then
 *   widens: inv(K_ref) 3x3 | E_src inv(E_ref) 4x4 | K_src 3x3 | inv(K_src) 3x3 | E_ref inv(E_src) 4x4 | K_ref 3x3.
 *   All arithmetic is fp64, narrowed to fp32 where numpy narrows (x_src, y_src, the sampled depth, depth_reprojected,
 *   x / y_reprojected, depth_diff, relative_depth_diff); relative_depth_diff < (float)geo_depth_thres is an fp32 comparison
 *   (numpy 2), dist < geo_pixel_thres an fp64 one.  The source depth is sampled as cv2.remap(INTER_LINEAR, constant border
 *   0) does, restated in csrc/depth_fusion.hip (1/32-pixel coordinates; not compared with a real OpenCV); a non-finite or
 *   far-away coordinate samples 0, and no input makes the kernel read outside a depth map.
 *   Outputs (device, (H,W)): mask_sum int32 = the number of consistent sources; mask uint8 = mask_sum >= geo_mask_thres;
 *   depth_avg fp64 = (fp32 sum of the consistent depth_reprojected in source order + ref_depth) / (mask_sum + 1);
 *   pair_masks (S,H,W) uint8, nullable: the per-pair masks.  Does not synchronise.
 * ufr_depth_points_*: the valid pixels (mask != 0) of one reference view as points, in row-major pixel order (:202-214).
 *   Two calls with the same mask, H, W and workspace (>= ufr_depth_points_workspace_bytes(H, W), device):
 *     ufr_depth_points_count: *n_host = N, the number of valid pixels.  SYNCHRONISES the stream.
 *     ufr_depth_points_emit: xyz (N,3) fp32 = (inv_e [inv_k (x, y, 1) depth_avg ; 1])[:3] in fp64, narrowed; rgb (N,3)
 *       uint8 = color (H,W,3) uint8 at the pixel.  depth_avg (H,W) fp64, color: device; inv_k (3x3), inv_e (4x4): host,
 *       row-major fp64.  capacity: the rows of xyz and rgb; capacity < N is an error (the count is read back from the
 *       workspace: SYNCHRONISES the stream), nothing beyond N is written.  xyz / rgb are nullable when N = 0, which is
 *       legal and writes nothing.  No atomics: the output is deterministic.
 * H, W >= 1 and H * W < 2^31 throughout.                                                                            */
#define UFR_DEPTH_MAX_SOURCES 64
#define UFR_DEPTH_PAIR_DOUBLES 68
int ufr_depth_consistency(const float* ref_depth, int32_t H, int32_t W, const float* const* src_depth, const int32_t* src_hw,
                          const double* mats, int32_t S, double geo_pixel_thres, double geo_depth_thres, int32_t geo_mask_thres,
                          int32_t* mask_sum, uint8_t* mask, double* depth_avg, uint8_t* pair_masks, ufr_stream stream);
size_t ufr_depth_points_workspace_bytes(int32_t H, int32_t W);
int ufr_depth_points_count(const uint8_t* mask, int32_t H, int32_t W, void* workspace, size_t workspace_bytes, int64_t* n_host,
                           ufr_stream stream);
int ufr_depth_points_emit(const uint8_t* mask, const double* depth_avg, const uint8_t* color, int32_t H, int32_t W,
                          const double* inv_k, const double* inv_e, void* workspace, size_t workspace_bytes, float* xyz,
                          uint8_t* rgb, int64_t capacity, ufr_stream stream);

/* ---- DTU mesh cleaning (ABI 507) ------------------------------------------------------------------------------
 * The device side of evaluation/clean_mesh.py (mask votes, first-hit faces, small components); uforecon_amd/clean_mesh.py is
 * the caller that strings these together, tests/clean_mesh_ref.py the numpy statement of every rule below.  verts (V,3) fp64,
 * faces (F,3) int32, images (H,W) row-major: device.  H, W >= 1, H * W < 2^31; V, F >= 1.
 *
 * ufr_mask_half_widths: the rows of cv.getStructuringElement(MORPH_ELLIPSE, (k, k)) as half-widths, k odd, 1 .. UFR_MASK_MAX_KERNEL:
 *   with r = k / 2, row dy = i - r covers columns -dx .. dx, dx = rint(r * sqrt((r*r - dy*dy) / (r*r))) in fp64, round half to
 *   even (0 for r = 0).  k = 11: 0 3 4 5 5 5 5 5 4 3 0.  out: HOST int32[k].  No OpenCV was at hand: this table is the rule.
 * ufr_mask_dilate: cv.dilate(image, that element) of a uint8 image: the maximum over the element centred on the pixel, pixels
 *   outside the image ignored (OpenCV's default border).  dilated (nullable): the uint8 result; mask (nullable): 1 where the
 *   result > threshold (the reference: 128), else 0.  Does not synchronise.
 * ufr_mesh_vertex_votes: clean_points_by_mask (:106-147) without its final comparison.  P: (n_views,3,4) fp32 DEVICE, the
 *   reference's read_cam_file product K4 @ E; masks (n_views,H,W) uint8 device, non-zero = set.  Per view in fp64 with P widened:
 *   q = P[:3,:3] x + P[:3,3] (products summed left to right, then the translation), q / q.z, px = rint(q.x), py = rint(q.y)
 *   (round half to even).  The vertex counts for the view iff -1 <= px <= W-1 and -1 <= py <= H-1 and (px == -1 or py == -1 or
 *   masks[view][py][px] != 0): the reference's +1 shift into a ones border, asymmetry included.  No z > 0 test, as in the
 *   reference; q.z = 0 or a non-finite q does not count.  votes (V) int32 = the number of views.  Integer atomics: the same
 *   bits run after run.  Does not synchronise.
 * ufr_mesh_first_hit: the face every masked pixel's ray hits first, for one view (clean_mesh_faces_outside_frustum :220-247
 *   with trimesh's intersects_first).  k_inv 3x3 and c2w 4x4: HOST fp32 row-major, the inverse intrinsics and the pose that
 *   gen_rays_from_single_image is given.  Ray of pixel (x, y) in fp32, no fused multiply-add, products summed left to right:
 *   p = k_inv (x, y, 1), v = p / sqrt((p.x*p.x + p.y*p.y) + p.z*p.z), d = c2w[:3,:3] v, o = c2w[:3,3].  Intersection in fp64
 *   from those values widened: a, b, c = the vertices - o; for each edge the product e = d . (u x v) of its vertex pair taken
 *   in ascending vertex-index order, negated for the other direction, so both faces of an edge use one number; hit iff the
 *   three are all >= 0 or all <= 0 (both sides, edges and vertices inclusive) and not all 0; n = (b - a) x (c - a),
 *   t = (n . a) / (n . d), no hit when n . d = 0 (zero area) or not t > 0.  The first hit is the smallest (float)t, ties to the
 *   lowest face index (a 64-bit atomic minimum over (float bits of t) << 32 | face: order-independent).  face_id (H,W) int32:
 *   the face, or -1 where mask is 0 or nothing is hit.  face_hit (F) uint8, nullable: set to 1 for every face in face_id and
 *   otherwise left alone, so that a caller accumulates over views.  A face with an index outside 0..V-1 is never hit.  Only
 *   the pixels inside a triangle's projected box (padded by 1/16 pixel) are tested; a triangle with a vertex at camera depth
 *   <= 0 is tested against the whole image, one wholly behind the camera against none.  workspace >=
 *   ufr_mesh_first_hit_workspace_bytes(F, H, W) (device).  Does not synchronise.
 * ufr_mesh_edge_keys: keys (3F) int64: slot 3f + e is edge (faces[f][e], faces[f][(e+1)%3]) as lo << 32 | hi of
 *   vertex_id[index] (vertex_id (V) int32 >= 0, device, nullable = the index itself: the caller's merge of equal vertices).  A
 *   face with an index out of range or two equal ids gets the unique negative keys -(slot + 1).  Does not synchronise.
 * ufr_mesh_face_components: sorted_keys (3F): those keys sorted ascending; order (3F) int64: the slot each came from (what
 *   torch.sort returns).  Two faces are adjacent iff they share a key that occurs exactly twice (trimesh.face_adjacency).
 *   labels (F) int32: the lowest face index of the face's component, -1 for a face with no adjacency.  Union-find: rounds of
 *   hooking (the larger of two roots under the smaller, atomic minimum) and pointer jumping until a round hooks nothing;
 *   SYNCHRONISES the stream once per round; *rounds_host (nullable) = rounds run, the last, idle one included.  The labels do
 *   not depend on scheduling.  workspace >= ufr_mesh_face_components_workspace_bytes(F) (device); F <= (2^31 - 1) / 3.   */
#define UFR_MASK_MAX_KERNEL 127
#define UFR_MESH_MAX_VIEWS 64
int ufr_mask_half_widths(int32_t k, int32_t* out);
int ufr_mask_dilate(const uint8_t* image, int32_t H, int32_t W, int32_t k, int32_t threshold, uint8_t* dilated, uint8_t* mask,
                    ufr_stream stream);
int ufr_mesh_vertex_votes(const double* verts, int64_t V, const float* P, const uint8_t* masks, int32_t n_views, int32_t H,
                          int32_t W, int32_t* votes, ufr_stream stream);
size_t ufr_mesh_first_hit_workspace_bytes(int64_t F, int32_t H, int32_t W);
int ufr_mesh_first_hit(const double* verts, const int32_t* faces, int64_t V, int64_t F, const float* k_inv, const float* c2w,
                       const uint8_t* mask, int32_t H, int32_t W, int32_t* face_id, uint8_t* face_hit, void* workspace,
                       size_t workspace_bytes, ufr_stream stream);
int ufr_mesh_edge_keys(const int32_t* faces, const int32_t* vertex_id, int64_t V, int64_t F, int64_t* keys, ufr_stream stream);
size_t ufr_mesh_face_components_workspace_bytes(int64_t F);
int ufr_mesh_face_components(const int64_t* sorted_keys, const int64_t* order, int64_t F, int32_t* labels, void* workspace,
                             size_t workspace_bytes, int32_t* rounds_host, ufr_stream stream);

/* ---- mesh rendering (ABI 507, additive) -----------------------------------------------------------------------
 * The device side of render_trajectory_dtu.py / render_trajectory_open3d.py (a fly-through of a reconstructed mesh) without
 * Open3D, OpenGL or a display; uforecon_amd/render_trajectory.py is the caller, tests/raster_ref.py the numpy statement of
 * every rule below.  verts (V,3) fp64, faces (F,3) int32, images row-major: device.  H, W >= 1, H * W < 2^31; V, F >= 1.
 * The same calls give z-depth, face-id and normal maps of a mesh from any camera.
 *
 * ufr_raster_vertex_normals: normals (V,3) fp64 = for each vertex the sum of the unnormalised face normals (b - a) x (c - a) of
 *   the faces that use it (a, b, c in the face's own order, whichever corner the vertex is), divided by the length of the
 *   sum: area weighting, as Open3D's compute_vertex_normals is remembered to do.  No Open3D was at hand: this rule is the
 *   specification.  sorted_slots (3F) int64: the corner slots 3f + e stably sorted by their vertex index (what torch.sort with
 *   stable=True returns as indices); run_starts (V+1) int64: vertex v owns positions run_starts[v] .. run_starts[v+1] - 1.
 *   A run is summed in ascending position (= ascending slot) order in fp64, each component on its own, by one thread: no
 *   floating-point atomics, the same bits run after run.  A vertex that no face uses and a vertex whose sum has length 0
 *   (or is not finite) get (0, 0, 0); a zero-area face adds zero; a face with an index outside 0..V-1, a slot outside
 *   0..3F-1 and a slot whose corner is not the vertex contribute nothing.  F <= (2^31 - 1) / 3.  Does not synchronise.
 * ufr_raster_frames: n_frames >= 1 views of the mesh in one call.  k_inv 3x3 (shared) and c2w (n_frames,4,4): HOST fp32
 *   row-major, with the meaning ufr_mesh_first_hit gives them.  Per frame: (1) that entry point's first hit over EVERY pixel
 *   (the same kernels through the same launcher, with no mask; the key image is re-initialised for every frame), then (2)
 *   one thread per pixel shades.  No hit: background, depth 0, face -1, normal 0.  Hit: the ray (fp32) and a, b, c, the ordered
 *   edge products e_bc, e_ca, e_ab and n (fp64) are formed again with the first hit's expressions, then in fp64
 *     w = (e_bc, e_ca, e_ab) / ((e_bc + e_ca) + e_ab)  (barycentrics of a, b, c),  t = (n . a) / (n . d),
 *     shading normal N: smooth = (w_a N_a + w_b N_b) + w_c N_c divided by its length; flat (normals null, or that length
 *       is not > 0) = n / |n|,
 *     I = ambient + (1 - ambient) * |N . d|: a headlight with two-sided shading, so the winding does not matter,
 *     colour = base_color, or with colors ((V,3) uint8, device, nullable) ((w_a C_a + w_b C_b) + w_c C_c) / 255,
 *     pixel = rint((255 * colour) * I), round half to even, clamped to 0..255.
 *   normals: (V,3) fp64 device, nullable (what ufr_raster_vertex_normals writes).  base_color: HOST float[3] in 0..1,
 *   nullable = white (as the reference paints the mesh); background: HOST uint8[3], nullable = 255 255 255; ambient in
 *   0..1 (the callers' default: 0.25).  Outputs (device, n_frames images): image (H,W,3) uint8; depth (H,W) fp32,
 *   nullable = (float)(t * v.z) with v the camera-space unit ray: z-depth; face_id (H,W) int32, nullable; normal_map (H,W,3)
 *   fp32, nullable = R^T N (camera coordinates, R = c2w[:3,:3]), negated when N . d > 0 so that it faces the camera.
 *   workspace >= ufr_raster_frames_workspace_bytes(F, H, W) (device; 0 for unsupported sizes).  A camera that is singular or
 *   not finite fails before anything is launched.  Enqueues 2 memsets and 4 kernels per frame and synchronises nowhere.
 * ufr_raster_downsample: dst (n,H,W,3) uint8 = the mean of the s x s blocks of src (n,s*H,s*W,3) uint8, s in 1..4 (1 copies),
 *   in integers: with n2 = s*s, q = sum / n2, r = sum % n2 the result is q + 1 iff 2r > n2, or 2r == n2 and q is odd (round
 *   half to even), else q.  s*H * s*W < 2^31, n*H*W*3 < 2^38.  Does not synchronise.
 * Every argument error (null pointer, H, W or n_frames < 1, H * W >= 2^31, s outside 1..4, ambient or a base colour outside
 * 0..1, a workspace that is too small) is UFR_ERR_ARG with the reason in the thread's last-error text.                  */
int ufr_raster_vertex_normals(const double* verts, const int32_t* faces, int64_t V, int64_t F, const int64_t* sorted_slots,
                              const int64_t* run_starts, double* normals, ufr_stream stream);
size_t ufr_raster_frames_workspace_bytes(int64_t F, int32_t H, int32_t W);
int ufr_raster_frames(const double* verts, const int32_t* faces, int64_t V, int64_t F, const double* normals, const uint8_t* colors,
                      const float* k_inv, const float* c2w, int32_t n_frames, int32_t H, int32_t W, const float* base_color,
                      const uint8_t* background, double ambient, uint8_t* image, float* depth, int32_t* face_id, float* normal_map,
                      void* workspace, size_t workspace_bytes, ufr_stream stream);
int ufr_raster_downsample(const uint8_t* src, int32_t n, int32_t H, int32_t W, int32_t s, uint8_t* dst, ufr_stream stream);

/* ---- point-cloud rendering (ABI 507, additive) ----------------------------------------------------------------
 * A z-buffered splat renderer with eye-dome lighting for the clouds the chain writes (depth_fusion's and tsdf's PLY files under pcd/,
 * dtu_eval's error clouds): the reference looks at them in an Open3D window, here there is no display.
 * uforecon_amd/render_trajectory.py (render_points) is the caller, tests/points_ref.py the numpy statement of every rule
 * below.  points (N,3) fp64, images row-major: device.  H, W >= 1, H * W < 2^31; 1 <= N <= 2^32 - 2 (2^31 - 1 with point_id).
 *
 * ufr_splat_frames: n_frames >= 1 views of the cloud in one call.  k 3x3 (shared; the caller has divided it by k[2][2]) and
 *   w2c (n_frames,4,4): HOST fp64 row-major, w2c the caller's fp64 inverse of the camera-to-world matrix.  Per frame the key
 *   image (H,W) uint64 is set to all ones, then
 *   (1) one thread per point, in fp64, products summed left to right, no fused multiply-add:
 *         c = w2c[:3,:3] p + w2c[:3,3] (the three products, then the translation),  q = k c,
 *         px = rint(q.x / q.z), py = rint(q.y / q.z), round half to even; pixel centres are the integers, as in
 *         ufr_mesh_first_hit.
 *       The point is dropped when a coordinate of p is not finite, when not c.z > z_min (z_min >= 0), when px or py is not
 *       finite, and when its whole footprint lies outside the image.  Footprint: the pixels (px + dx, py + dy) with
 *       dx^2 + dy^2 <= r^2 + r, r = radius in 0..4 (0: one pixel, 1: the 3x3 block, 2: a 21-pixel disc), clipped to the image.
 *       Every pixel of it takes key = (bits of (float)c.z) << 32 | point index with a 64-bit unsigned atomic minimum: the
 *       nearest (float) depth wins, ties go to the lowest index, whatever the order of arrival -- the same bits run after run.
 *       (The pixel's key is read with a plain load first and the atomic skipped when the point cannot win.)
 *   (2) one thread per pixel resolves.  Key all ones: background, depth 0, point_id -1.  Otherwise z = the stored float and,
 *       in fp64 with z widened,
 *         o_k = max(0, log2(z) - log2(z_k)) over the neighbours (x - d, y), (x + d, y), (x, y - d), (x, y + d), d = edl_radius
 *               >= 1; a neighbour that is empty or outside the image gives 0,
 *         s = ((o_1 + o_2) + o_3) + o_4,  I = exp(-(edl_strength * s) / 4): eye-dome lighting, a pixel darkens by how far it
 *               lies behind its neighbours in log depth; edl_strength = 0 or s = 0 give I = 1 with no call of exp,
 *         colour = colors[index] ((N,3) uint8, device, nullable) or 255 * base_color,
 *         pixel = rint(colour * I), round half to even, clamped to 0..255.
 *   base_color: HOST float[3] in 0..1, nullable = white; background: HOST uint8[3], nullable = 255 255 255.  Outputs (device,
 *   n_frames images): image (H,W,3) uint8; depth (H,W) fp32, nullable = the stored z: z-depth, comparable with
 *   ufr_raster_frames' depth; point_id (H,W) int32, nullable.  workspace >= ufr_splat_frames_workspace_bytes(H, W) (device; 0
 *   for unsupported sizes).  A camera that is not finite or whose w2c[:3,:3] is singular fails before anything is launched.
 *   Enqueues 1 memset and 2 kernels per frame and synchronises nowhere.
 * Every argument error (null pointer, N < 1 or too large, H, W or n_frames < 1, H * W >= 2^31, radius outside 0..4, edl_radius
 * < 1, a negative or non-finite edl_strength or z_min, a base colour outside 0..1, a workspace that is too small) is
 * UFR_ERR_ARG with the reason in the thread's last-error text.                                                       */
size_t ufr_splat_frames_workspace_bytes(int32_t H, int32_t W);
int ufr_splat_frames(const double* points, int64_t N, const uint8_t* colors, const double* k, const double* w2c, int32_t n_frames,
                     int32_t H, int32_t W, int32_t radius, double z_min, const float* base_color, const uint8_t* background,
                     double edl_strength, int32_t edl_radius, uint8_t* image, float* depth, int32_t* point_id, void* workspace,
                     size_t workspace_bytes, ufr_stream stream);

/* ---- mesh colouring (ABI 507, additive) -----------------------------------------------------------------------
 * Per-vertex colour from the photographs, visibility-aware: the last stage of the chain, between clean_mesh and
 * render_trajectory; the reference has no such stage.  uforecon_amd/color_mesh.py is the caller, tests/color_mesh_ref.py the
 * numpy statement of every rule below.  Neither Open3D nor MVS-texturing was compared against: the rule written here is the
 * rule.  Everything is fp64, every product and sum rounded on its own (no fused multiply-add), sums taken left to right;
 * there is no floating-point atomic, so a rerun gives the same bits.
 *
 * ufr_color_vertices: verts (V,3) fp64, device; normals (V,3) fp64, device, nullable; images (n_views,H,W,3) uint8,
 *   device, all views of one size; depth (n_views,H,W) fp32, device, nullable: the z-depth ufr_raster_frames writes, 0 = no
 *   hit.  Cameras: HOST fp64 row-major, the convention of ufr_splat_frames: k (n_views,3,3), already divided by k[2][2];
 *   w2c (n_views,4,4); centre (n_views,3), the camera centres in world coordinates.  1 <= n_views <= UFR_MESH_MAX_VIEWS;
 *   H, W >= 2, H * W < 2^31; 1 <= V <= 2^31 - 1.  z_min >= 0, depth_tol >= 0 (both finite), min_cos in 0..1, power in 0..8,
 *   mode UFR_MESH_COLOR_MEAN or UFR_MESH_COLOR_BEST, fill HOST uint8[3].  Outputs (device): colors (V,3) uint8, views_used
 *   (V) uint8.  One thread owns vertex p and walks the views k in ascending order:
 *     c = w2c[:3,:3] p + w2c[:3,3] (the three products, then the translation).  The view is skipped when a coordinate of p
 *       or c is not finite, or not c.z > z_min.
 *     q = k c, x = q.x / q.z, y = q.y / q.z; pixel centres are the integers, as in ufr_mesh_first_hit.
 *     x0 = floor(x), y0 = floor(y), fx = x - x0, fy = y - y0.  The view is skipped unless 0 <= x0, x0 + 1 <= W - 1, 0 <= y0
 *       and y0 + 1 <= H - 1: all four texels lie in the picture.
 *     Occlusion (depth given): the four depths D(y0..y0+1, x0..x0+1) must all be > 0 and c.z <= (1 + depth_tol) * min(D), D
 *       widened, 1 + depth_tol rounded once.  Conservative on purpose: a vertex whose footprint touches a pixel without a
 *       hit, or a pixel nearer than it, takes no colour from that view, so neither the picture's background nor a nearer
 *       surface bleeds onto it.
 *     Angle (normals given): e = p - centre, d = e / sqrt((e.x*e.x + e.y*e.y) + e.z*e.z), cosv = |(N.x*d.x + N.y*d.y) +
 *       N.z*d.z|: two-sided, as the rasteriser shades, because the winding is not trusted.  The view is skipped unless cosv
 *       >= min_cos and cosv > 0: a zero normal is never seen.  Without normals cosv = 1.
 *     Weight: w = 1, then w = w * cosv, power times (no pow: its last bit differs between libraries).
 *     Sample, per channel, I the widened bytes at (y0, x0), (y0, x0+1), (y0+1, x0), (y0+1, x0+1):
 *       s = (1 - fy) * ((1 - fx) * I00 + fx * I01) + fy * ((1 - fx) * I10 + fx * I11).
 *     Mode mean: A += w * s per channel and Wsum += w, in view order; colour = rint(A / Wsum), round half to even, clamped
 *       to 0..255 (not a number: 0).  Mode best: the view of largest w wins, ties to the lowest view index; colour = rint(s)
 *       of that view, clamped likewise.
 *   views_used = the number of views not skipped; when it is 0 the vertex gets fill.  workspace >=
 *   ufr_color_vertices_workspace_bytes(n_views) (device; the camera table, which travels there as kernel arguments of
 *   small upload kernels: no copy, no allocation).  A camera that is not finite or whose w2c[:3,:3] is singular fails
 *   before anything is launched.  Does not synchronise.
 * ufr_color_fill_round: one Jacobi round that gives colour to empty vertices from their neighbours.  faces (F,3) int32,
 *   sorted_slots (3F) and run_starts (V+1) int64 as ufr_raster_vertex_normals takes them; colors_in (V,3) uint8; state_in (V)
 *   uint8, 0 = empty.  A vertex with state_in != 0 is copied (colour and state).  For an empty vertex its corner run is
 *   walked in ascending position; for each slot 3f + e the face's other two corners are visited in the order (e + 1) % 3,
 *   (e + 2) % 3, and every visited corner with state_in != 0 adds its three channels to integer sums and 1 to a count.  A
 *   neighbour shared by two faces counts twice: that is the rule.  count > 0: each channel = sum / count rounded half to
 *   even in integers (q = sum / count, r = sum % count, q + 1 iff 2r > count, or 2r == count and q is odd: the rule of
 *   ufr_raster_downsample), state_out = 1 and *filled (device int32, the caller zeroes it) += 1 by an integer atomic.  count
 *   = 0: the vertex stays empty, colour copied.  A slot outside 0..3F-1, a slot whose corner is not the vertex and a corner
 *   outside 0..V-1 contribute nothing.  colors_out / state_out must not alias the inputs: the round is double-buffered, so
 *   it does not depend on scheduling.  Integers only.  F <= (2^31 - 1) / 3.  Does not synchronise.
 * Every argument error (null pointer, a size or count out of range, z_min or depth_tol negative or not finite, min_cos
 * outside 0..1, power outside 0..8, an unknown mode, a workspace that is too small) is UFR_ERR_ARG with the reason in the
 * thread's last-error text; nothing is launched then.                                                                  */
#define UFR_MESH_COLOR_MEAN 0
#define UFR_MESH_COLOR_BEST 1
#define UFR_MESH_COLOR_MAX_POWER 8
size_t ufr_color_vertices_workspace_bytes(int32_t n_views);
int ufr_color_vertices(const double* verts, const double* normals, int64_t V, const uint8_t* images, const float* depth,
                           const double* k, const double* w2c, const double* centre, int32_t n_views, int32_t H, int32_t W,
                           double z_min, double depth_tol, double min_cos, int32_t power, int32_t mode, const uint8_t* fill,
                           uint8_t* colors, uint8_t* views_used, void* workspace, size_t workspace_bytes, ufr_stream stream);
int ufr_color_fill_round(const int32_t* faces, int64_t V, int64_t F, const int64_t* sorted_slots, const int64_t* run_starts,
                              const uint8_t* colors_in, const uint8_t* state_in, uint8_t* colors_out, uint8_t* state_out,
                              int32_t* filled, ufr_stream stream);

/* ---- mesh texturing (ABI 507, additive) -----------------------------------------------------------------------
 * A per-face texture atlas baked from the photographs: what a thinned mesh needs to carry the pictures' detail, which one
 * colour per vertex cannot.  The stage after simplify_mesh, beside mesh colouring; the reference has no such stage.
 * uforecon_amd/texture_mesh.py is the caller, uforecon_amd/texture_ops.py holds the wrappers, tests/texture_ref.py is the
 * numpy statement of every rule below.  Neither Open3D nor MVS-texturing was compared against: the rule written here is the
 * rule.  Everything is fp64, every product and sum rounded on its own (no fused multiply-add), sums taken left to right;
 * there is no floating-point atomic, so a rerun gives the same bits.  All arrays live on the device unless marked HOST.
 *
 * The atlas, in closed form: host and device agree by construction.  Patch size S, 1 <= S <= UFR_TEXTURE_MAX_PATCH, is the
 *   number of texel steps along a triangle's legs; the cell side is C = S + 3.  Faces 2q and 2q + 1 share cell q; n_cells =
 *   (F + 1) / 2, cols = ceil(sqrt(n_cells)) (exact, in integers), rows = ceil(n_cells / cols).  Cell q sits at column q % cols
 *   and row q / cols; the atlas is Wt = cols * C by Ht = rows * C texels, each <= UFR_TEXTURE_MAX_SIDE.  Texel centres are the
 *   integers, as pixel centres are everywhere in this header.  Local texel (i, j) of a cell (i along x) belongs to the even
 *   face when i + j <= S + 2, otherwise to the odd face with (i, j) := (C-1-i, C-1-j): a half turn, so nothing is mirrored.
 *   In those face-local indices corner a sits at (0, 0), b at (S, 0), c at (0, S) -- for the odd face the cell-local texels
 *   (C-1, C-1), (C-1-S, C-1), (C-1, C-1-S) -- and a texel's weights are wb = i / S, wc = j / S, wa = (1 - wb) - wc.  wa goes
 *   negative in the gutter, the diagonal band i + j > S past the hypotenuse (two texels deep for the even face, one for
 *   the odd); the legs lie on the cell's border and need none.  The gutter is what keeps the bilinear footprint of any point of a face, edges and corners included, on that face's own
 *   texels.  A texel whose face index is >= F belongs to no face.  Patch sizes are uniform: there are no charts and no sizes
 *   by face area, which suits marching-cubes and clustered meshes, whose faces are of one size.
 * ufr_texture_bake: one thread per texel.  verts (V,3) fp64; faces (F,3) int32; images, depth, k, w2c, centre, n_views, H, W,
 *   z_min, depth_tol, min_cos, power, mode, fill: exactly as ufr_color_vertices takes them, with its ranges; S, Ht, Wt: the
 *   atlas, which must equal the closed form for (F, S); fallback (V,3) uint8, nullable: vertex colours for the texels no view
 *   saw.  Outputs: texture (Ht,Wt,3) uint8 and views_used (Ht,Wt) uint8.  For a texel of face f with corners a, b, c:
 *     p = (wa * a + wb * b) + wc * c per component.
 *     n = (b - a) x (c - a), each component two products and a difference, divided by len = sqrt((n.x*n.x + n.y*n.y) + n.z*n.z);
 *       a len that is not > 0, or not finite, gives the zero normal, which no view sees.
 *     The views are walked in ascending order by the per-view rule of ufr_color_vertices (projection, bounds, angle against
 *       n, occlusion, weight, sample, accumulate), and the colour is formed as there; views_used = the views not skipped.
 *     No view: to_byte((wa * Ca + wb * Cb) + wc * Cc) per channel of the face's fallback colours when fallback is given
 *       (to_byte: rint, half to even, clamped to 0..255, not a number: 0), else fill; views_used = 0.
 *   A texel of no face, and a texel of a face with an index outside 0..V-1, gets fill and 0.  workspace >=
 *   ufr_color_vertices_workspace_bytes(n_views): the camera table.  Nothing synchronises.
 * ufr_texture_fill_round: one Jacobi round in texel space, integers only.  colors_in (Ht,Wt,3) uint8, state_in (Ht,Wt) uint8,
 *   0 = empty; S, Ht, Wt, F: the atlas as above.  A texel with state_in != 0, or of no face, is copied (colour and state).
 *   An empty one visits (x-1, y), (x+1, y), (x, y-1), (x, y+1) in that order; a neighbour counts when it is inside the atlas,
 *   belongs to the same face and has state_in != 0.  count > 0: each channel = sum / count rounded half to even in integers
 *   (the rule of ufr_color_fill_round), state_out = 1 and *filled (device int32, the caller zeroes it) += 1 by an integer
 *   atomic.  count = 0: copied.  Fallback colours sit in state-0 texels and are never read by a round.  colors_out /
 *   state_out must not alias the inputs.  Two rounds reach the gutter's depth.  Does not synchronise.
 * ufr_texture_frames: ufr_raster_frames with the colour taken from a texture: the same first hit, barycentrics, normals,
 *   shading, depth, face-id and normal outputs, and workspace >= ufr_raster_frames_workspace_bytes(F, H, W).  corner_xy (F,3,2)
 *   fp64: the texel coordinates (x, y) of every face's corners a, b, c; texture (Ht,Wt,3) uint8, Ht, Wt in 1 ..
 *   UFR_TEXTURE_MAX_SIDE (any texture: the closed form is not asked for here).  With the shade kernel's own w_a, w_b, w_c:
 *     tx = (w_a * xa + w_b * xb) + w_c * xc, ty likewise.  A tx or ty that is not finite gives the colour white (1, 1, 1).
 *     x0 = floor(tx), fx = tx - x0; the indices x0 and x0 + 1 are each clamped to 0..Wt-1 after fx is formed (in double,
 *       before the conversion); the same in y.
 *     s = (1 - fy) * ((1 - fx) * T00 + fx * T01) + fy * ((1 - fx) * T10 + fx * T11) per channel, T the widened bytes;
 *       colour = s / 255; pixel = rint((255 * colour) * I), as ufr_raster_frames.
 *   There are no mipmaps: a texture seen from afar aliases, and rendering larger and averaging down (ufr_raster_downsample,
 *   render_trajectory --supersample) is the antialiasing.
 * Not done: per-face view selection and seam levelling (a texel is blended over all views that see it, like a vertex);
 * exposure compensation; mipmaps; charts.  Every argument error (null pointer, S outside 1..125, an atlas that is not the
 * closed form for (F, S), Ht or Wt above 16384, the ranges of ufr_color_vertices, a workspace that is too small, out buffers
 * that alias in buffers) is UFR_ERR_ARG with the reason in the thread's last-error text; nothing is launched then.       */
#define UFR_TEXTURE_MAX_PATCH 125
#define UFR_TEXTURE_MAX_SIDE 16384
int ufr_texture_bake(const double* verts, const int32_t* faces, int64_t V, int64_t F, const uint8_t* images, const float* depth,
                     const double* k, const double* w2c, const double* centre, int32_t n_views, int32_t H, int32_t W, int32_t S,
                     int32_t Ht, int32_t Wt, double z_min, double depth_tol, double min_cos, int32_t power, int32_t mode,
                     const uint8_t* fill, const uint8_t* fallback, uint8_t* texture, uint8_t* views_used, void* workspace,
                     size_t workspace_size, ufr_stream stream);
int ufr_texture_fill_round(const uint8_t* colors_in, const uint8_t* state_in, int32_t S, int32_t Ht, int32_t Wt, int64_t F,
                           uint8_t* colors_out, uint8_t* state_out, int32_t* filled, ufr_stream stream);
int ufr_texture_frames(const double* verts, const int32_t* faces, int64_t V, int64_t F, const double* normals, const double* corner_xy,
                       const uint8_t* texture, int32_t Ht, int32_t Wt, const float* k_inv, const float* c2w, int32_t n_frames,
                       int32_t H, int32_t W, const uint8_t* background, double ambient, uint8_t* image, float* depth,
                       int32_t* face_id, float* normal_map, void* workspace, size_t workspace_size, ufr_stream stream);

/* ---- mesh smoothing (ABI 507, additive) ------------------------------------------------------------------------
 * Laplacian and Taubin smoothing with uniform or cotangent weights: the denoising stage of the mesh route, between cleaning
 * and simplification; the reference leaves it to Open3D and trimesh.  uforecon_amd/smooth_mesh.py is the caller,
 * ops.mesh_smooth strings the calls together, tests/smooth_ref.py is the numpy statement of every rule below.  Open3D was
 * not compared against: the rule written here is the rule.  The feature-preserving filter is mesh denoising, below.  Only vertex
 * positions change.  Everything is fp64, every product, quotient, square root and sum rounded on its own (no fused
 * multiply-add), sums taken left to right; there is no floating-point atomic, so a rerun gives the same bits.  All arrays
 * live on the device unless marked HOST.  V: 1 .. 2^31 - 1, F: 1 .. (2^31 - 1) / 3.
 *
 * Rows.  Corner slot s = 3f + e names the vertex faces[f][e].  sorted_slots (3F) and run_starts (V+1) int64 are those of
 *   ufr_raster_vertex_normals: the slots sorted by the vertex they name with one STABLE sort, and where every vertex's run
 *   starts.  Row i is sorted slot i; vertex v's rows run_starts[v] .. run_starts[v+1] - 1 are its corners in ascending s.  A row
 *   in face f at corner e names the two other corners a = faces[f][(e+1)%3], b = faces[f][(e+2)%3].  A face that names a
 *   vertex twice, or a vertex outside 0 .. V-1, is dead: its three rows contribute nothing anywhere.
 * Weights (wa, wb) of a row.  UFR_SMOOTH_UNIFORM: (1, 1) -- on a closed manifold the umbrella operator with every neighbour
 *   counted twice.  UFR_SMOOTH_COTANGENT, from the positions p given to ufr_smooth_rows and fixed for all steps: with
 *   (c0, c1, c2) the face's corners in its own order, u = p[c1] - p[c0], t = p[c2] - p[c0], n0 = u1*t2 - u2*t1,
 *   n1 = u2*t0 - u0*t2, n2 = u0*t1 - u1*t0, nf = sqrt((n0*n0 + n1*n1) + n2*n2) -- once per face, the same for its three rows;
 *   a face with nf = 0 or nf not finite is dead in this mode.  With x.y = (x0*y0 + x1*y1) + x2*y2 and v the row's vertex:
 *   wa = clamp(((p[v] - p[b]).(p[a] - p[b])) / nf), the cotangent of the angle at b, and wb = clamp(((p[v] - p[a]).(p[b] -
 *   p[a])) / nf), the cotangent at a; clamp(w) = 0 unless w > 0 (so for a NaN too), then 64 if w > 64.  The bounds are
 *   derived, not tuned: a negative weight (an obtuse angle) can flip a triangle, and 64 is the cotangent of a sliver angle
 *   under 0.9 degrees.
 * Border.  border (V) uint8 = 1 iff some neighbour stands in the vertex's live rows a number of times other than 2 (an open
 *   edge, a non-manifold edge), else 0; a vertex without live rows gets 0.
 * ufr_smooth_rows: writes, into the workspace, every row's (a, b) as int32 -- (-1, -1) for a dead row -- and, for
 *   cotangent weights, its (wa, wb); then border.  Two launches, no synchronisation.
 * ufr_smooth_steps: n_steps Jacobi steps over the rows a ufr_smooth_rows call with the same V, F, weights and
 *   workspace left; factors (n_steps) HOST fp64, all finite.  Step i reads pos_a and writes pos_b when i is even, reads pos_b
 *   and writes pos_a when i is odd: the caller puts the positions into pos_a (V,3) and finds the result in pos_a when n_steps
 *   is even, in pos_b (V,3) when it is odd.  One step with factor t, for every vertex v with previous position p:
 *     num_k = 0, den = 0; per row in order:  num_k = num_k + (wa * (p[a]_k - p[v]_k) + wb * (p[b]_k - p[v]_k))  for k = 0, 1, 2,
 *     den = den + (wa + wb);  then  p'[v]_k = p[v]_k + (t * num_k) / den  when den > 0 and v is not held,
 *   else p'[v] = p[v], bit for bit.  v is held when border is given and border[v] != 0 (a null border: the border moves like
 *   the rest) or pinned (V, uint8, nullable) is given and pinned[v] != 0.  Laplacian smoothing is n steps with factor lam;
 *   Taubin smoothing alternates lam and mu < -lam; the caller writes the factors.  All steps are issued from this one call and
 *   the host reads nothing between them.  Does not synchronise.
 * workspace >= ufr_smooth_workspace_bytes (device; 8 bytes a row, 24 with cotangent weights; 0 for arguments out of
 * range).  Every argument error (null pointer, a count out of range, unknown weights, a factor that is not finite, pos_a ==
 * pos_b, a workspace that is too small) is UFR_ERR_ARG (UFR_ERR_WORKSPACE for the workspace) with the reason in the thread's
 * last-error text; nothing is launched then.                                                                           */
#define UFR_SMOOTH_UNIFORM 0
#define UFR_SMOOTH_COTANGENT 1
size_t ufr_smooth_workspace_bytes(int64_t V, int64_t F, int32_t weights);
int ufr_smooth_rows(const double* verts, const int32_t* faces, int64_t V, int64_t F, const int64_t* sorted_slots,
                         const int64_t* run_starts, int32_t weights, uint8_t* border, void* workspace, size_t workspace_bytes,
                         ufr_stream stream);
int ufr_smooth_steps(int64_t V, int64_t F, const int64_t* run_starts, int32_t weights, const uint8_t* border,
                          const uint8_t* pinned, const double* factors, int32_t n_steps, double* pos_a, double* pos_b,
                          const void* workspace, size_t workspace_bytes, ufr_stream stream);

/* ---- mesh denoising (ABI 507, additive) ------------------------------------------------------------------------
 * Feature-preserving denoising: the local iterative bilateral normal filter of Zheng et al. 2011 ("Bilateral normal filtering
 * for mesh denoising") followed by the vertex update of Sun et al. 2007 -- a sibling of mesh smoothing, which rounds a crease
 * like noise.  uforecon_amd/denoise_mesh.py is the caller, ops.mesh_denoise strings the calls together, tests/denoise_ref.py is
 * the numpy statement of every rule below.  Open3D and MeshLab were not compared against: the rule written here is the rule.
 * Only vertex positions change.  Everything is fp64, every product, quotient, square root and sum rounded on its own (no
 * fused multiply-add), sums taken left to right in the order stated; there is no floating-point atomic, so a rerun gives the
 * same bits.  dot3(x, y) = (x0*y0 + x1*y1) + x2*y2.  All arrays live on the device unless marked HOST.  V: 1 .. 2^31 - 1,
 * F: 1 .. (2^31 - 1) / 3.  sorted_slots (3F), run_starts (V+1) and "rows" are those of mesh smoothing.
 *
 * Face records, from the positions p given to ufr_denoise_faces and fixed for all steps.  With (c0, c1, c2) the face's
 *   corners in its own order, u = p[c1] - p[c0], t = p[c2] - p[c0], m0 = u1*t2 - u2*t1, m1 = u2*t0 - u0*t2,
 *   m2 = u0*t1 - u1*t0, nf = sqrt(dot3(m, m)): the face is LIVE when its three indices are in 0 .. V-1 and distinct and nf is
 *   finite and above 0.  A live face has the unit normal n = m / nf (three divisions), the area A = 0.5 * nf and the centroid
 *   c_k = ((p[c0]_k + p[c1]_k) + p[c2]_k) / 3.0.  A dead face has zeros for all three, is nobody's neighbour and is never filtered.
 * Neighbourhood of a live face f, in this order: f itself; then, for corner e = 0, 1, 2, the rows of vertex faces[f][e] in
 *   ascending slot, each giving g = slot / 3, skipped when g == f, when g is dead, or when g names faces[f][e'] for some
 *   e' < e (a face across an edge counts once, at the first corner that reaches it).
 * Weight kernel k(u): x = 1 - u / 256; 0 when !(x > 0) (so from u = 256 on, and for a NaN); otherwise x squared eight times,
 *   (1 - u/256)^256.  It stands in for exp(-u) -- the largest difference is 1.06e-3, at u = 2 -- without a transcendental call.
 * One normal step (Jacobi: every read from the previous normals).  acc = 0; for g over the neighbourhood in order:
 *     dc = c_g - c_f, dn = n_g - n_f, w = (A_g * k(dot3(dc, dc) / two_ss)) * k(dot3(dn, dn) / two_rr),
 *     acc_k = acc_k + w * n_g[k];
 *   L = sqrt(dot3(acc, acc)); the next normal is acc / L (three divisions) when L is finite and above 0, else the previous
 *   normal, bit for bit.  two_ss = 2.0 * (sigma_s * sigma_s) and two_rr = 2.0 * (sigma_r * sigma_r) are computed by the caller.
 * One vertex step (Jacobi over positions q, the filtered normals fixed), for a vertex v that is not held: s = 0, cnt = 0;
 *   per row of v in ascending slot whose face g is live, with (a, b, c) g's corners in its own order:
 *     cg_k = ((q[a]_k + q[b]_k) + q[c]_k) / 3.0, d = dot3(cg - q[v], n_g), s_k = s_k + n_g[k] * d, cnt = cnt + 1;
 *   q'[v]_k = q[v]_k + s_k / (double)cnt when cnt > 0, else q'[v] = q[v]; a held vertex keeps its bits.  v is held when border
 *   is given and border[v] != 0 (a null border: the border moves like the rest) or pinned (V, uint8, nullable) is given and
 *   pinned[v] != 0.
 * Border.  border (V) uint8 = 1 iff some neighbour stands in the vertex's live rows a number of times other than 2, else 0:
 *   the border ufr_smooth_rows reports with cotangent weights for the same input.
 * ufr_denoise_faces: writes the records and the rows into the workspace, every face's own normal into normals (F,3) and
 *   border.  Three launches, no synchronisation.
 * ufr_denoise_normals: n_steps normal steps over what a ufr_denoise_faces call with the same V, F and workspace left,
 *   ping-ponging two record buffers inside the workspace; the last step writes normals (F,3).  n_steps = 0 leaves the faces'
 *   own normals there.  Call it once per ufr_denoise_faces call.
 * ufr_denoise_vertices: n_steps vertex steps with normals (F,3) fixed.  Step i reads pos_a and writes pos_b when i is even,
 *   the other way round when i is odd: the caller puts the positions into pos_a (V,3) and finds the result in pos_a when
 *   n_steps is even, in pos_b (V,3) when it is odd.
 * Each phase issues all of its steps from one call and the host reads nothing between them.  Does not synchronise.
 * workspace >= ufr_denoise_workspace_bytes (device; two records of 64 bytes a face and 20 bytes a row: 188 bytes a face; 0
 * for arguments out of range).  Every argument error (null pointer, a count out of range, a sigma term that is not finite or
 * not above 0, a negative n_steps, buffers that alias, a workspace that is too small) is UFR_ERR_ARG (UFR_ERR_WORKSPACE for
 * the workspace) with the reason in the thread's last-error text; nothing is launched then.  Limits: sigma_r has to grow with
 * the noise (noise of a third of an edge defeats 0.35); no real scan has been denoised.                                  */
size_t ufr_denoise_workspace_bytes(int64_t V, int64_t F);
int ufr_denoise_faces(const double* verts, const int32_t* faces, int64_t V, int64_t F, const int64_t* sorted_slots,
                      const int64_t* run_starts, double* normals, uint8_t* border, void* workspace, size_t workspace_bytes,
                      ufr_stream stream);
int ufr_denoise_normals(const int32_t* faces, int64_t V, int64_t F, const int64_t* run_starts, double two_ss, double two_rr,
                        int32_t n_steps, double* normals, void* workspace, size_t workspace_bytes, ufr_stream stream);
int ufr_denoise_vertices(int64_t V, int64_t F, const int64_t* run_starts, const double* normals, const uint8_t* border,
                         const uint8_t* pinned, int32_t n_steps, double* pos_a, double* pos_b, const void* workspace,
                         size_t workspace_bytes, ufr_stream stream);

/* ---- mesh simplification (ABI 507, additive) -----------------------------------------------------------------
 * Vertex clustering with quadric placement: the thinning stage of the mesh route, as ufr_points_voxel_mean is the point
 * route's; the reference leaves it to Open3D and trimesh.  uforecon_amd/simplify_mesh.py is the caller, ops.mesh_simplify
 * strings the calls together, tests/simplify_ref.py is the numpy statement of every rule below.  Open3D was not compared
 * against: the rule written here is the rule.  There is no edge-collapse decimation and no topology guarantee (clustering
 * can pinch a thin part into non-manifold edges); normals are not carried.  Everything is fp64, every product and sum
 * rounded on its own (no fused multiply-add), sums taken left to right; there is no floating-point atomic, so a rerun gives
 * the same bits.  All arrays live on the device unless marked HOST.  V, F, the cluster count C: each 1 .. 2^31 - 1.
 *
 * Clusters.  With h the cell edge, the caller puts the origin o at min_bound - h / 2, refuses more than 2^21 - 4 cells on
 *   an axis, takes the keys of ufr_points_cell_keys at cell = h and sorts them with a STABLE sort: exactly the setup of
 *   ufr_points_voxel_mean, which then gives, per occupied cell in key order, the vertex count, the mean position xm (summed
 *   in ascending vertex index) and the rounded mean colour.  A cluster's cell (i0, i1, i2) is its key's Morton triple and
 *   its centre is m_a = o_a + ((double)i_a + 0.5) * h.  Quadrics live in coordinates relative to m, so they stay well scaled.
 * ufr_simplify_clusters: sorted_keys (V) and order (V) int64 as the stable sort returns them (order[i] = the input index of
 *   sorted row i).  cluster (V) int32: the cluster of every INPUT vertex = the number of run heads before its row;
 *   cluster_key (capacity) int64: the key of every cluster.  *total_host = C.  SYNCHRONISES the stream once.
 * ufr_simplify_face_keys: keys (3F) int64.  With (ca, cb, cc) the clusters of face f's corners: keys[3f] = ca << 32 | f;
 *   keys[3f+1] = cb << 32 | f if cb != ca; keys[3f+2] = cc << 32 | f if cc != ca and cc != cb; an unused slot (and every
 *   slot of a face with a corner outside 0 .. V-1) holds 2^63 - 1.  A face with two corners in one cluster so contributes
 *   once to it.  The caller sorts the keys (one stable sort): every cluster's faces then stand in ascending face index.
 * ufr_simplify_quadrics: sorted_keys (3F) from above; quadrics (C,10) fp64 and n_faces (C) int32 are zeroed, then the head
 *   of every run of equal key >> 32 sums its run left to right.  For face f with corner positions pa, pb, pc and the run's
 *   cluster centre m:  u = pb - pa, v = pc - pa,  n0 = u1*v2 - u2*v1, n1 = u2*v0 - u0*v2, n2 = u0*v1 - u1*v0 (the
 *   unnormalised normal: area-squared weighting, as in Lindstrom's out-of-core simplification);  r = pa - m,
 *   d = -((n0*r0 + n1*r1) + n2*r2);  the ten terms, in the order stored:  A00 = n0*n0, A01 = n0*n1, A02 = n0*n2, A11 = n1*n1,
 *   A12 = n1*n2, A22 = n2*n2, b0 = n0*d, b1 = n1*d, b2 = n2*d, c = d*d.  n_faces = the run's length.
 * ufr_simplify_place: mean (C,3) = xm; position (C,3) fp64 and placed (C) uint8 out.  placement UFR_SIMPLIFY_MEAN, or a
 *   cluster with n_faces = 0: position = xm, placed = 0.  UFR_SIMPLIFY_QUADRIC:  xb = xm - m;  w = 2^-10 * ((A00 + A11) + A22);
 *   A'kk = Akk + w;  b'k = bk - w * xbk;  c' = c + w * ((xb0*xb0 + xb1*xb1) + xb2*xb2): the quadric regularised towards the
 *   mean.  2^-10 is a stated choice, not a tuned one; it plays the part of Lindstrom's 1e-3 singular-value cut-off, costs no
 *   rounding, and makes A' positive definite wherever a face contributes, so a planar or crease cluster's minimiser slides
 *   to the mean along its free directions.  A' x = -b' by cofactors:
 *     C00 = A'11*A'22 - A12*A12,  C01 = A02*A12 - A01*A'22,  C02 = A01*A12 - A02*A'11,
 *     C11 = A'00*A'22 - A02*A02,  C12 = A01*A02 - A'00*A12,  C22 = A'00*A'11 - A01*A01,
 *     det = (A'00*C00 + A01*C01) + A02*C02,  rk = -b'k,
 *     x0 = ((C00*r0 + C01*r1) + C02*r2) / det,  x1 = ((C01*r0 + C11*r1) + C12*r2) / det,  x2 = ((C02*r0 + C12*r1) + C22*r2) / det.
 *   E'(y) = (((y0*g0 + y1*g1) + y2*g2) + 2 * ((b'0*y0 + b'1*y1) + b'2*y2)) + c' with g0 = (A'00*y0 + A01*y1) + A02*y2,
 *   g1 = (A01*y0 + A'11*y1) + A12*y2, g2 = (A02*y0 + A12*y1) + A'22*y2.  x is taken iff x0, x1, x2 are finite, every
 *   |xk| <= 0.5 * h, and E'(x) <= E'(xb):  position = m + x, placed = 1.  Otherwise position = xm, placed = 0.
 * ufr_simplify_face_triples: triples (F,3) int32, key_a (F) and key_bc (F) int64.  A face whose corners do not lie in three
 *   different clusters (or with a corner outside 0 .. V-1) is collapsed: triple (-1,-1,-1), both keys 2^63 - 1.  The others
 *   are rotated so that the smallest cluster number stands first, (a, b, c), orientation kept: key_a = a, key_bc = b << 32 | c.
 *   The caller sorts stably by key_bc, then stably by key_a: equal triples then stand together in ascending face index.
 * ufr_simplify_face_heads: order (F) int64 = the input index of every row after both sorts.  keep (F) uint8, by INPUT index:
 *   1 for the first row of every run of equal (key_a, key_bc) that is not collapsed, else 0: among faces with the same
 *   rotated triple the lowest input index survives.  (a,b,c) and (a,c,b) are different triples; both stay.
 * ufr_simplify_compact_faces: the kept triples in ascending input index (the ordered compaction of marching cubes):
 *   out_faces (capacity,3) int32 in CLUSTER numbers, face_map (capacity) int32 = the input index of every output face;
 *   referenced (C) uint8 is zeroed, then set to 1 for every cluster a kept face names.  *total_host = F', which may exceed
 *   capacity (nothing beyond is written).  SYNCHRONISES the stream once.
 * ufr_simplify_compact_vertices: the referenced clusters, renumbered in key order: cluster_vertex (C) int32 = the output
 *   vertex of every cluster or -1; out_verts / out_colors (nullable with colors) / out_placed / out_count (capacity rows)
 *   = position / colors / placed / count of the referenced clusters; vertex_map (V) int32 = cluster_vertex[cluster[v]];
 *   faces (n_faces,3) int32 are rewritten IN PLACE from cluster numbers to output vertices (n_faces may be 0, faces then
 *   nullable).  *total_host = V'.  SYNCHRONISES the stream once.
 * workspace >= ufr_simplify_workspace_bytes(n) (device) with n >= the call's V, F or C, whichever it scans.
 * Every argument error (null pointer, a count outside its range, a cell or origin that is not finite or a cell <= 0, an
 * unknown placement, a negative capacity, a workspace that is too small) is UFR_ERR_ARG (UFR_ERR_WORKSPACE for the
 * workspace) with the reason in the thread's last-error text; nothing is launched then.                              */
#define UFR_SIMPLIFY_QUADRIC 0
#define UFR_SIMPLIFY_MEAN 1
size_t ufr_simplify_workspace_bytes(int64_t n);
int ufr_simplify_clusters(const int64_t* sorted_keys, const int64_t* order, int64_t V, int32_t* cluster, int64_t* cluster_key,
                          int64_t capacity, void* workspace, size_t workspace_bytes, int64_t* total_host, ufr_stream stream);
int ufr_simplify_face_keys(const int32_t* faces, const int32_t* cluster, int64_t V, int64_t F, int64_t* keys, ufr_stream stream);
int ufr_simplify_quadrics(const double* verts, const int32_t* faces, const int64_t* cluster_key, int64_t V, int64_t F, int64_t C,
                          const double* origin, double cell, const int64_t* sorted_keys, double* quadrics, int32_t* n_faces,
                          ufr_stream stream);
int ufr_simplify_place(const double* quadrics, const int32_t* n_faces, const double* mean, const int64_t* cluster_key, int64_t C,
                       const double* origin, double cell, int32_t placement, double* position, uint8_t* placed,
                       ufr_stream stream);
int ufr_simplify_face_triples(const int32_t* faces, const int32_t* cluster, int64_t V, int64_t F, int32_t* triples,
                              int64_t* key_a, int64_t* key_bc, ufr_stream stream);
int ufr_simplify_face_heads(const int64_t* key_a, const int64_t* key_bc, const int64_t* order, int64_t F, uint8_t* keep,
                            ufr_stream stream);
int ufr_simplify_compact_faces(const int32_t* triples, const uint8_t* keep, int64_t F, int64_t C, int32_t* out_faces,
                               int32_t* face_map, int64_t capacity, uint8_t* referenced, void* workspace,
                               size_t workspace_bytes, int64_t* total_host, ufr_stream stream);
int ufr_simplify_compact_vertices(const uint8_t* referenced, int64_t C, const double* position, const uint8_t* colors,
                                  const uint8_t* placed, const int32_t* count, const int32_t* cluster, int64_t V, int32_t* faces,
                                  int64_t n_faces, double* out_verts, uint8_t* out_colors, uint8_t* out_placed,
                                  int32_t* out_count, int64_t capacity, int32_t* cluster_vertex, int32_t* vertex_map,
                                  void* workspace, size_t workspace_bytes, int64_t* total_host, ufr_stream stream);

/* ---- point-cloud filtering (ABI 507, additive) ----------------------------------------------------------------
 * The cleanup between depth fusion and scoring that an MVS pipeline expects (voxel downsampling, statistical and radius
 * outlier removal, normal estimation); the reference leaves it to Open3D.  uforecon_amd/pcd_filter.py is the caller,
 * tests/pcd_ref.py the numpy statement of every rule below.  The rules follow the public descriptions of PCL's and Open3D's
 * filters; neither library was compared against: the rule written here is the rule.  All positions and distances are fp64,
 * every product and sum rounded on its own (no fused multiply-add); there is no floating-point atomic, so a rerun gives the
 * same bits.  Every count nq, nr, n below is 1 .. 2^31 - 1.  None of the three takes a point set on the host.
 *
 * ufr_points_knn: for every query its k nearest reference points, 1 <= k <= UFR_KNN_MAX_K.  query (nq,3): device, any order
 *   (a wave is fastest when its queries are neighbours).  ref (nr,3) with ref_keys (nr): sorted by ufr_points_cell_keys' key,
 *   with the origin and cell the keys were made with, exactly as ufr_points_nn_dist takes them.  ref_index (nr) int32: the
 *   caller's index of every sorted point (>= 0).  self_index (nq) int32, nullable: a caller's index that query i skips (a
 *   point that looks for its neighbours in its own set).  A candidate's key is (d2, ref_index) with
 *   d2 = (dx*dx + dy*dy) + dz*dz; it is admitted iff d2 <= max_dist*max_dist (max_dist > 0, +inf allowed).  The result is the
 *   k smallest keys in lexicographic order: ties in distance go to the lower caller's index, whatever the sorted order.
 *   idx (nq,k) int32: caller's indices; dist (nq,k) fp64 = sqrt(d2), ascending; empty slots get -1 and +inf.  A query with a
 *   coordinate that is not finite gets only empty slots; a reference point with one is never admitted.  The octree walk
 *   (depth-first, nearest octant first) drops a node only when its box is strictly farther than the k-th d2 so far, visits
 *   every node at most once and has a bounded stack: it ends whatever the data.  No workspace.  Does not synchronise.
 * ufr_points_normals: points (n,3); idx (n,k) int32, 1 <= k <= UFR_KNN_MAX_K: the neighbours of every point, the point itself
 *   included, as ufr_points_knn writes them; an entry outside 0 .. n-1 is an empty slot.  Per point, over its m non-empty
 *   slots in slot order: centroid c = the left-to-right sum / m; covariance = the six left-to-right sums of the products of
 *   (p_j - c), each / m; its eigen-decomposition by eight sweeps of cyclic Jacobi ((0,1), (0,2), (1,2)) in fp64.
 *   normal (n,3) = the unit eigenvector of the smallest eigenvalue l0; curvature (n) = l0 / (l0 + l1 + l2), 0 when the sum
 *   is 0; valid (n) uint8 = 1.  With m < 3 (or a result that is not finite) valid = 0 and normal and curvature are 0.
 *   Orientation: viewpoints (V,3) fp64, device, V >= 0 (nullable when V = 0).  V >= 1: with p the point and c_j the
 *   viewpoints, the j with the largest |n . (c_j - p)| / |c_j - p| decides, ties to the lowest j: n is negated when
 *   n . (c_j - p) < 0 (dot products summed left to right).  V = 0: n is negated when its component of largest magnitude is
 *   negative, ties to the lowest axis.  No workspace.  Does not synchronise.
 * ufr_points_voxel_mean: points (n,3) with keys (n): sorted by ufr_points_cell_keys' key at cell = the voxel size, by a STABLE
 *   sort, so that every voxel's points stand in ascending caller's index; the caller puts the origin at min_bound - voxel / 2
 *   and refuses an extent of more than 2^21 - 4 cells on an axis.  colors (n,3) uint8 and normals (n,3) fp64: nullable, in
 *   the same order.  Per run of equal keys, in key order: out_points = the left-to-right sum / count; out_colors per channel
 *   = (2 * sum + count) / (2 * count) in integers (the mean, halves up); out_normals = the left-to-right sum divided by its
 *   length, 0 when that is 0; count int32 = the run's length.  Outputs have `capacity` rows (device); nothing beyond is
 *   written, and out_colors / out_normals are needed exactly when their input is given.  *total_host = the number of runs,
 *   which may exceed capacity.  Run heads are ranked with the ordered compaction's integer scans.  workspace >=
 *   ufr_points_voxel_mean_workspace_bytes(n) (device).  SYNCHRONISES the stream once, to hand the total to the host.
 * Every argument error (null pointer, a count outside its range, k outside 1 .. UFR_KNN_MAX_K, max_dist not > 0, a cell or
 * origin that is not finite, V < 0, a negative capacity, a workspace that is too small) is UFR_ERR_ARG (UFR_ERR_WORKSPACE for
 * the workspace) with the reason in the thread's last-error text; nothing is launched then.                             */
#define UFR_KNN_MAX_K 32
int ufr_points_knn(const double* query, int64_t nq, const double* ref, const int64_t* ref_keys, const int32_t* ref_index,
                   int64_t nr, const double* origin, double cell, const int32_t* self_index, int32_t k, double max_dist,
                   int32_t* idx, double* dist, ufr_stream stream);
int ufr_points_normals(const double* points, int64_t n, const int32_t* idx, int32_t k, const double* viewpoints, int32_t V,
                       double* normal, double* curvature, uint8_t* valid, ufr_stream stream);
size_t ufr_points_voxel_mean_workspace_bytes(int64_t n);
int ufr_points_voxel_mean(const double* points, const int64_t* keys, int64_t n, const uint8_t* colors, const double* normals,
                          double* out_points, uint8_t* out_colors, double* out_normals, int32_t* count, int64_t capacity,
                          void* workspace, size_t workspace_bytes, int64_t* total_host, ufr_stream stream);

/* ---- a scan loader's per-pixel work (ABI 507, additive) -----------------------------------------------------
 * What DtuFitSparse (code1/dataset/dtu_test_sparse.py:247-298, 412-429) computes per pixel; uforecon_amd/dtu_scan.py does the
 * 4x4 camera arithmetic on the host and calls these two.  Neither synchronises.
 * ufr_image_resize_u8: src = n interleaved RGB images (n,Hs,Ws,3) uint8, device -> dst (n,3,Ho,Wo) fp32 planes, device:
 *   each image resized to H x W, cropped, divided by 255.  clip4: HOST int32[4] = columns dropped on the left, rows on the
 *   top, columns on the right, rows on the bottom (the reference's clip_wh doubled), nullable = none; Ho = H - top - bottom,
 *   Wo = W - left - right.  The resize is OpenCV's resize() for 8-bit images with INTER_LINEAR, restated (no OpenCV was
 *   compared): for output index d of an axis with scale = (double)source size / size,
 *     f = (float)((d + 0.5) * scale - 0.5), s = floor(f), f -= s, weights rint((1.f - f) * 2048.f) and rint(f * 2048.f);
 *     along x a tap outside the row moves s to the edge and sets f = 0; along y the rows s and s + 1 are clamped to the
 *     image and the weights stay;  row = S[s] * a0 + S[s + 1] * a1 in int32;
 *     value = (((b0 * (row0 >> 4)) >> 16) + ((b1 * (row1 >> 4)) >> 16) + 2) >> 2;
 *   when Hs == 2 H and Ws == 2 W the value is the box mean (s00 + s01 + s10 + s11 + 2) >> 2 instead.  Each output is
 *   (float)((double)value / 255.0).  Hs * Ws and H * W < 2^31, n * Ho * Wo * 3 < 2^38.
 * ufr_pixel_rays: dir (3,H*W) fp32, device = unit vectors through the pixel centres of the normalised grid.  m_inv: HOST
 *   float[16], row-major 4x4; origin: HOST float[3], nullable = 0.  Per pixel (x, y), in double:
 *     p = (x * 2 / (W - 1) - 1, y * 2 / (H - 1) - 1, 1, 1), v = (m_inv p)[:3] - origin, dir[:, y * W + x] = (float)(v / |v|).
 *   With m_inv = ref_pose_inv and origin = ray_o this is the batch's ray_d; with the inverse of the normalised intrinsics
 *   and no origin it is cam_ray_d.  H, W >= 2 (the grid divides by H - 1 and W - 1), H * W < 2^31.
 * Every argument error (null src, dst, m_inv or dir, a size < 1, H or W < 2 for the rays, a negative clip or one that leaves
 * nothing) is UFR_ERR_ARG with the reason in the thread's last-error text.                                            */
int ufr_image_resize_u8(const uint8_t* src, int32_t n, int32_t Hs, int32_t Ws, int32_t H, int32_t W, const int32_t* clip4, float* dst,
                        ufr_stream stream);
int ufr_pixel_rays(const float* m_inv, const float* origin, int32_t H, int32_t W, float* dir, ufr_stream stream);

/* ---- a custom scene's loader and converter (ABI 507, additive) ------------------------------------------------
 * What GeneralFit (code1/dataset/general_fit.py) adds to the per-pixel work above, and the view selection of
 * colmap2mvsnet.py (:379-408); uforecon_amd/general_scan.py and uforecon_amd/colmap2mvsnet.py are the callers.  Neither
 * synchronises; every argument error is UFR_ERR_ARG with the reason in the thread's last-error text.
 *
 * ufr_image_resize_mask_u8: ufr_image_resize_u8's contract (sizes, clip4, limits, errors, the resize rule stated there) with a
 *   second source, mask (n,Hs,Ws) uint8, device: colour and mask are each resized by that rule (the box mean included), and
 *   each output is (float)(((double)v / 255.0) * ((double)m / 254.0)) -- general_fit.py:174-180; the 254 is the reference's
 *   own and is kept, so a mask value of 255 gives slightly more than the colour.  A null mask is an error.
 *
 * ufr_view_pair_scores: score (N,N) fp64, device.  The N images' observation lists are CSR: offsets, HOST int64[N + 1], read
 *   before the call returns (offsets[0] = 0, offsets[N] = n_obs, non-decreasing); obs, DEVICE int32[n_obs]: image i's
 *   observations in file order are obs[offsets[i] .. offsets[i+1]), each the row of `points` of the 3-D point it saw or -1 for
 *   none; an index may repeat.  points (M,3) and centres (N,3): device fp64.  For i < j, with c_i, c_j the centres:
 *     score[i][j] = sum over the observations o of image i whose p = obs[o] is not -1 and occurs in image j's list of
 *       term(p) = exp( -(theta - theta0)^2 / (2 sigma^2) ),  sigma = sigma1 if theta <= theta0 else sigma2,
 *       theta   = (180 / pi) acos( ((c_i - p) . (c_j - p)) / |c_i - p| / |c_j - p| )      (degrees)
 *   A point that occurs twice in image i counts twice; how often it occurs in image j does not matter.  score[j][i] is a copy
 *   of score[i][j], not a second sum; the diagonal is 0.  The acos argument is clamped to [-1, 1]: where rounding carries it
 *   past 1 the reference gets NaN and this gets the term of theta = 0 (a point AT a camera centre still gives NaN: 0 / 0).
 *   All arithmetic is fp64, each product and sum rounded on its own.  One workgroup of 256 threads per pair: thread t adds the
 *   terms of observations t, t + 256, ... in that order, the 256 partial sums are added in a fixed tree (lanes l + 32, 16, 8,
 *   4, 2, 1 inside a wave, then (w0 + w1) + (w2 + w3)): the order depends on the list's length alone, there is no
 *   floating-point atomic, and a rerun gives the same bits.  It is NOT the reference's order (one running sum in file
 *   order): tests/test_gpu_view_select.py bounds the difference by what reversing that sum moves it.
 *   Membership is a binary search in a per-image sorted copy of the lists, which THIS CALL makes on the device, in the
 *   workspace (the caller passes no sorted copy).
 *   obs_host: HOST copy of obs, nullable.  An entry point cannot read device memory without waiting for the stream, so the
 *   range check of the indices runs on this copy, before anything is launched: an index outside [-1, M) is an argument error.
 *   With a null obs_host the caller vouches for the range; the kernels treat an index outside 0 .. M-1 as -1 either way, so
 *   no input makes them read outside `points`.
 *   Errors: a null pointer (obs may be null when n_obs = 0, points when M = 0), N < 1, offsets that do not start at 0, end at
 *   n_obs or decrease, an index outside [-1, M) in obs_host, sigma1 or sigma2 <= 0 or a non-finite parameter, a workspace
 *   smaller than ufr_view_pair_scores_workspace_bytes(N, n_obs) (device; 0 and an error text for sizes outside the range).
 *   1 <= N <= 32768, n_obs < 2^31, M < 2^31.  Enqueues ceil((N + 1) / 448) + 2 kernels (the offsets travel in launch
 *   arguments) and one memset.                                                                                          */
int ufr_image_resize_mask_u8(const uint8_t* src, const uint8_t* mask, int32_t n, int32_t Hs, int32_t Ws, int32_t H, int32_t W,
                             const int32_t* clip4, float* dst, ufr_stream stream);
size_t ufr_view_pair_scores_workspace_bytes(int32_t N, int64_t n_obs);
int ufr_view_pair_scores(const int64_t* offsets, const int32_t* obs, const int32_t* obs_host, int64_t n_obs, const double* points,
                         int64_t M, const double* centres, int32_t N, double theta0, double sigma1, double sigma2, double* score,
                         void* workspace, size_t workspace_bytes, ufr_stream stream);

/* ---- undistortion of a custom scene's pictures (ABI 507, additive) -------------------------------------------
 * What the reference leaves to COLMAP's own undistorter, which is expected to run before its colmap2mvsnet.py: the pictures
 * of a camera with lens distortion, resampled to a pinhole camera.  uforecon_amd/colmap2mvsnet.py (--undistort) is the caller,
 * uforecon_amd/undistort.py has the host form.  The rule below restates COLMAP's public camera models; it was compared with
 * neither COLMAP nor OpenCV: the rule written here is the rule.
 *
 * ufr_image_undistort_u8: src = n interleaved images (n,Hs,Ws,C) uint8, device, C = 1 .. 4, all taken by ONE camera -> dst
 *   (n,H,W,C) uint8, device; valid (H,W) uint8, device, nullable: 255 where the output pixel has a source, else 0 (one map for
 *   the n images: it is computed once per output pixel).  model: COLMAP's camera model id; params: HOST double[], that model's
 *   COLMAP parameter list; k_out: HOST double[4] = fx' fy' cx' cy' of the output pinhole camera; both are read before the call
 *   returns.  Per output pixel (x, y), everything in fp64, each product, sum and quotient rounded on its own (no fused
 *   multiply-add), in the order the parentheses give; fx fy cx cy are the source camera's (fy = fx for a one-focal model):
 *     xn = ((x + 0.5) - cx') / fx'                     yn = ((y + 0.5) - cy') / fy'
 *     (xd, yd) = distort(xn, yn)                       (below)
 *     u = ((fx * xd) + cx) - 0.5                       v = ((fy * yd) + cy) - 0.5        (COLMAP: pixel centres at +0.5)
 *     ok = 0 <= u <= Ws - 1 and 0 <= v <= Hs - 1       (a NaN is not ok)
 *     x0 = min(floor(u), Ws - 1), x1 = min(x0 + 1, Ws - 1), a = u - x0;   y0, y1, b likewise from v and Hs
 *     top = ((1 - a) * S[y0][x0]) + (a * S[y0][x1]),  bot = ((1 - a) * S[y1][x0]) + (a * S[y1][x1])
 *     val = ((1 - b) * top) + (b * bot),  dst = (uint8) rint(val), round half to even     (per image and channel)
 *   A pixel that is not ok reads nothing and gets 0 in every channel of every image and 0 in valid.
 *   distort, with xx = x * x, yy = y * y, r2 = xx + yy, r4 = r2 * r2, r6 = r4 * r2, xy = x * y and COLMAP's parameter order;
 *   a coefficient that a model does not have is 0 (adding a zero term changes no finite result, so each line is every
 *   one of its models' own formula):
 *     SIMPLE_PINHOLE 0 (f cx cy), PINHOLE 1 (fx fy cx cy), SIMPLE_RADIAL 2 (f cx cy k1), RADIAL 3 (f cx cy k1 k2),
 *     OPENCV 4 (fx fy cx cy k1 k2 p1 p2):
 *       rad = (k1 * r2) + (k2 * r4)
 *       tx = ((2 * p1) * xy) + (p2 * (r2 + (2 * xx)))      ty = ((2 * p2) * xy) + (p1 * (r2 + (2 * yy)))
 *       xd = (x + (x * rad)) + tx                          yd = (y + (y * rad)) + ty
 *       (the two pinhole models come out as the identity)
 *     FULL_OPENCV 6 (fx fy cx cy k1 k2 p1 p2 k3 k4 k5 k6): tx, ty as above,
 *       rad = (((1 + (k1 * r2)) + (k2 * r4)) + (k3 * r6)) / (((1 + (k4 * r2)) + (k5 * r4)) + (k6 * r6))
 *       xd = (x * rad) + tx                                yd = (y * rad) + ty
 *     OPENCV_FISHEYE 5 (fx fy cx cy k1 k2 k3 k4), SIMPLE_RADIAL_FISHEYE 8 (f cx cy k1), RADIAL_FISHEYE 9 (f cx cy k1 k2):
 *       r = sqrt(r2), t = atan(r), t2 = t * t, t4 = t2 * t2, t6 = t4 * t2, t8 = t4 * t4
 *       s = (t * ((((1 + (k1 * t2)) + (k2 * t4)) + (k3 * t6)) + (k4 * t8))) / r,  and s = 1 where r < 1e-8
 *       xd = x * s                                         yd = y * s
 *       (sqrt is correctly rounded; atan is the math library's and may differ between libraries in the last place)
 *     FOV 7 and THIN_PRISM_FISHEYE 10 are refused.
 *   One thread per output pixel; no workspace; enqueues one kernel and synchronises nowhere.
 *   Errors: a null src, dst, params or k_out; n, Hs, Ws, H or W < 1; C outside 1 .. 4; a model that is unknown or refused; a
 *   parameter of the model or of k_out that is not finite; fx' or fy' <= 0; Hs * Ws or H * W >= 2^31 -- each UFR_ERR_ARG with
 *   the reason in the thread's last-error text.                                                                          */
int ufr_image_undistort_u8(const uint8_t* src, int32_t n, int32_t Hs, int32_t Ws, int32_t C, int32_t model, const double* params,
                           const double* k_out, int32_t H, int32_t W, uint8_t* dst, uint8_t* valid, ufr_stream stream);

/* ---- the optimizer update and the ray draw of a training step (ABI 507, additive) ----------------------------
 * What UFORecon.training_step / configure_optimizers (code1/model.py:72-87, 537) run around the ray path, each as one call.
 * Neither synchronises; every argument error is UFR_ERR_ARG with the reason in the thread's last-error text.
 *
 * ufr_adam_step: torch.optim.Adam with its defaults (no weight decay, no amsgrad, no maximize) for n_tensors tensors in
 *   ceil(n_tensors / UFR_ADAM_TABLE_CAPACITY) launches.  Per tensor (device fp32, numel elements each, 0 <= numel < 2^31):
 *     exp_avg    += (grad - exp_avg) (1 - beta1)
 *     exp_avg_sq  = beta2 exp_avg_sq + (1 - beta2) grad^2
 *     param      -= (lr / bias_correction1) exp_avg / (sqrt(exp_avg_sq) / sqrt(bias_correction2) + eps)
 *   bias_correction1 / 2 = 1 - beta1^step / 1 - beta2^step for THAT tensor's step count (after this step), formed by the
 *   caller in double: a tensor without a gradient is left out of a call and its count does not advance, so the counts of
 *   one call may differ.  lr / bias_correction1 and sqrt(bias_correction2) are formed in double and rounded to fp32, the
 *   rest is fp32.  The table is HOST memory, read before the call returns; it travels to the kernel in the launch's own
 *   arguments (no staging buffer).  The grid is split over elements, one block per 4096 elements of one tensor.  Pointers
 *   need 4-byte alignment only: a tensor whose four pointers are all 16-byte aligned is updated with 16-byte accesses, any
 *   other one with 4-byte accesses.  No two tensors of a call may overlap.
 * ufr_select_rays: idx_out[0..k) (device int64) = the first k entries of the STABLE ascending argsort of u[0..n) (device
 *   fp32) -- argsort(rand(H W))[:train_ray_num] of model.py:537 with equal values in index order.  The order is that of
 *   the values' bit patterns as unsigned integers: the floats' own order for non-negative, non-NaN input; for any other
 *   input the result is still k distinct indices in [0, n).  A radix select over the patterns (three digit passes), an
 *   ordered compaction of the k smallest and one block sorting them; integer counters only, so a rerun gives the same
 *   bits.  1 <= k <= min(n, 4096), n <= 2^24.  workspace >= ufr_select_rays_workspace_bytes(n, k) (device, 8-byte
 *   aligned; 0 and an error text for sizes outside the range). */
#define UFR_ADAM_TABLE_CAPACITY 64
typedef struct ufr_adam_tensor {
  float* param;
  const float* grad;
  float* exp_avg;
  float* exp_avg_sq;
  int64_t numel;
  double bias_correction1, bias_correction2;
} ufr_adam_tensor;
int32_t ufr_adam_table_capacity(void);
int ufr_adam_step(const ufr_adam_tensor* tensors, int32_t n_tensors, double lr, double beta1, double beta2, double eps,
                  ufr_stream stream);
size_t ufr_select_rays_workspace_bytes(int32_t n, int32_t k);
int ufr_select_rays(const float* u, int32_t n, int32_t k, int64_t* idx_out, void* workspace, size_t workspace_bytes,
                    ufr_stream stream);

/* Pixel-wise view weights of the first cascade stage and the weighted aggregate (DepthNet.forward,
 * code1/encoder_utils/fmt/TransMVSNet.py:80-97 with PixelwiseNet :23-41), one pass over the similarity volume:
 *   view_weights[i] = max_d sigmoid(conv2(relu(bn1(conv1(relu(bn0(conv0(similarity[i]))))))))      (1x1x1 convolutions)
 *   aggregated[d]   = (sum_i similarity[i][d] view_weights[i]) / (1e-5 + sum_i view_weights[i])       (nullable)
 * similarity [NS][D][H][W], view_weights [NS][H][W], aggregated [D][H][W]: device fp32.  params: 185 device floats
 * [a0 16 | b0 16 | W1 8x16 | a1 8 | b1 8 | w2 8 | b2 1], the eval-mode BatchNorms folded by the caller: a0 = conv0.weight *
 * scale0, b0 = shift0, W1 = conv1.weight, a1 = scale1, b1 = shift1, w2 = conv2.weight, b2 = conv2.bias. */
int ufr_pixelwise_view_weights(const float* similarity, const float* params, float* view_weights, float* aggregated, int32_t NS,
                               int32_t D, int32_t H, int32_t W, ufr_stream stream);

/* ---- deformable convolution of the feature backbone -------------------------------------------------------
 * Replaces torchvision.ops.deform_conv2d as called by DCN.forward (code1/encoder_utils/fmt/dcn.py:66-80; every use in
 * FeatureNet, code1/encoder_utils/fmt/module.py:407-440, is 3x3, stride 1, padding 1, dilation 1, one offset group,
 * modulated).  input [B][C][H][W], offset [B][18][H][W] (channel 2k = dy, 2k+1 = dx of tap k), mask [B][9][H][W]
 * (nullable), weight [Cout][C][3][3], bias [Cout] (nullable), output [B][Cout][H][W]: device, fp32.
 * C a multiple of 4, <= 32; Cout in {8, 16, 32}.                                                                */
size_t ufr_deform_conv2d_workspace_bytes(int32_t B, int32_t C, int32_t H, int32_t W);
int ufr_deform_conv2d(const float* input, const float* offset, const float* mask, const float* weight,
                      const float* bias, float* output, int32_t B, int32_t C, int32_t Cout, int32_t H, int32_t W,
                      void* workspace, size_t workspace_bytes, ufr_stream stream);

/* ---- the feature backbone on channel-last tensors (ABI 502) --------------------------------------------------
 * FeatureNet.forward (code1/encoder_utils/fmt/module.py:388-468) is convolution -> BatchNorm -> ReLU blocks (module.py:26-62),
 * 1x1 lateral connections added to a nearest-upsampled map (:452-466), and deformable layers whose offsets / masks come from
 * a plain convolution (fmt/dcn.py:41-80).  These two entry points run that chain without a layout change and without a
 * separate elementwise pass; `uforecon_amd/featurenet.py` is the plan that calls them.
 *
 * ufr_conv2d: out = [relu]( conv(input, weight) * scale + shift ) [+ up2(skip)], zero padding ksize / 2.
 *   input [B][H][W][cin] (UFR_CONV2D_IN_PLANAR: [B][3][H][W], the image); weight [cout][cin][ksize][ksize]; scale / shift
 *   [cout], nullable (eval-mode BatchNorm and / or bias folded by the caller); skip [B][Ho/2][Wo/2][cout], nullable: added
 *   after nearest 2x upsampling (F.interpolate(scale_factor=2, mode='nearest')); output [B][Ho][Wo][cout], or planar
 *   [B][cout][Ho][Wo] with UFR_CONV2D_OUT_PLANAR; sigmoid_from >= 0: sigmoid on output channels >= sigmoid_from (the mask
 *   channels 18..26 of DCN.conv_offset_mask, whose planar output IS ufr_deform_conv2d*'s offset | mask pair), < 0: none.
 *   Shapes: the layer shapes of FeatureNet (cin in {3 planar, 8, 16, 32}, ksize 1 / 3 / 5, stride 1 / 2, cout <= 32);
 *   anything else returns UFR_ERR_ARG.  fp32 products and sums (v_mfma_f32_16x16x4_f32).
 * ufr_deform_conv2d_cl: ufr_deform_conv2d on a channel-last input [B][H][W][32] (no re-layout, no workspace) with the
 *   epilogue out = [relu]((dcn + bias) * scale + shift); offset_mask [B][27][H][W] = planes 0..17 the offsets (2k = dy,
 *   2k+1 = dx of tap k), planes 18..26 the masks (after the sigmoid) -- ufr_conv2d(..., UFR_CONV2D_OUT_PLANAR, sigmoid_from
 *   = 18) of DCN.conv_offset_mask; output channel-last [B][H][W][Cout] unless UFR_CONV2D_OUT_PLANAR. */
#define UFR_CONV2D_RELU 1
#define UFR_CONV2D_IN_PLANAR 2
#define UFR_CONV2D_OUT_PLANAR 4
int ufr_conv2d(const float* input, const float* weight, const float* scale, const float* shift, const float* skip, float* output,
               int32_t B, int32_t cin, int32_t cout, int32_t H, int32_t W, int32_t ksize, int32_t stride, int32_t flags,
               int32_t sigmoid_from, ufr_stream stream);
/* The sum the smoothing convolutions of the FMT's top-down pathway read (FMT_with_pathway, code1/encoder_utils/fmt/FMT.py:
 * 226-255: smooth(interpolate(reduce(coarse), size = fine, mode = 'bilinear') + fine)): output_cl [B][2h][2w][C] =
 * bilinear 2x of reduced_cl [B][h][w][C] (align_corners = False, torch's tap order) + fine [B][C][2h][2w] (planar, as the
 * reference holds the backbone's maps).  C in {8, 16}.  The reduction and the smoothing are ufr_conv2d calls. */
int ufr_upsample_add(const float* reduced_cl, const float* fine, float* output_cl, int32_t B, int32_t C, int32_t h, int32_t w,
                     ufr_stream stream);
int ufr_deform_conv2d_cl(const float* input_cl, const float* offset_mask, const float* weight, const float* bias,
                         const float* scale, const float* shift, float* output, int32_t B, int32_t C, int32_t Cout, int32_t H,
                         int32_t W, int32_t flags, ufr_stream stream);


/* ---- feature-matching transformer layer ----------------------------------------------
 * One EncoderLayer of the FMT (code1/encoder_utils/fmt/FMT.py:82-113: linear attention with the elu+1 feature map, FMT.py:17-39,
 * d_model 32, 8 heads; out-projection + residual, LayerNorm, 32-64-32 ReLU MLP + residual, LayerNorm; dropout 0).
 * x (N,T,32): query tokens; src (N,S,32): key/value tokens (NULL = x, self-attention); out (N,T,32) (may alias neither).
 * All nn.Linear weights row-major [out][in] as in the checkpoint.  workspace >= ufr_fmt_layer_workspace_bytes(N). */
typedef struct ufr_fmt_layer_weights {
  const float *wq, *bq, *wk, *bk, *wv, *bv, *wo, *bo; /* attention.{query,key,value,out}_projection: [32][32], [32] */
  const float *w1, *b1, *w2, *b2;                     /* linear1 [64][32], [64]; linear2 [32][64], [32]             */
  const float *n1w, *n1b, *n2w, *n2b;                 /* norm1 / norm2 weight, bias [32]                            */
} ufr_fmt_layer_weights;
size_t ufr_fmt_layer_workspace_bytes(int32_t N, int32_t S);   /* S: source tokens per sample (T for self-attention) */
int ufr_fmt_layer(const ufr_fmt_layer_weights* w, const float* x, const float* src, int32_t N, int32_t T, int32_t S,
                  float* out, void* workspace, ufr_stream stream);

/* ---- Poisson surface reconstruction (ABI 507, additive) -------------------------------------------------------
 * From an oriented point cloud (what uforecon_amd/pcd_filter.py writes with --normals) to an indicator field on a uniform
 * grid, whose level set ufr_marching_cubes_* turns into a mesh; the reference leaves this to Open3D.  uforecon_amd/
 * poisson_mesh.py is the caller, tests/poisson_ref.py the numpy / scipy statement of every rule below.  The rules are a
 * uniform-grid form of Kazhdan's Poisson reconstruction; neither Open3D nor PoissonRecon was compared against: the rule
 * written here is the rule.  There is no adaptive octree, no screening term and no multigrid preconditioner.  Everything is
 * fp64, every product and sum rounded on its own (no fused multiply-add); there is no floating-point atomic and every grid
 * is a function of the sizes alone, so a rerun gives the same bits.  A volume is (X,Y,Z) = dims[0..2] fp64 on the device, z
 * fastest: node (i,j,k) at [(i*Y + j)*Z + k], at the position origin + h*(i,j,k).  Every dim is >= 2 and X*Y*Z < 2^31.
 *
 * ufr_poisson_grid (host only, no device touched): bound_min / bound_max: the extent of the samples, HOST fp64[3].
 *   h = max over the axes of (max - min) / resolution; origin[a] = min[a] - pad*h; dims[a] = ceil((max[a] - min[a]) / h) + 1
 *   + 2*pad.  Refused: resolution < 4; pad < 2 (the splat and the central differences must stay inside the grid); a bound
 *   that is not finite; max < min; a degenerate extent (h = 0, or h^2 outside the fp64 range); 2^31 nodes or more.
 * ufr_poisson_splat_keys: points (n,3), 1 <= n < 2^28.  Per point and axis u = (p - origin) / h clamped to [0, dim - 1], the
 *   cell c = min(floor(u), dim - 2), the offset t = u - c.  keys (8n) int64: keys[8p + 4a + 2b + g] = the linear index of the
 *   node c + (a,b,g).  A point with a coordinate that is not finite gets eight keys of -1.
 * ufr_poisson_splat: keys (8n) sorted ascending by a STABLE sort and rows (8n) int64 = the sort's permutation (rows[s] = the
 *   unsorted position 8p + corner of sorted row s), so that the rows of a node stand in ascending sample index.  The weight
 *   of corner (a,b,g) is (wx*wy)*wz with wx = a ? t[0] : 1 - t[0] and so on.  Per node, summed left to right along its run:
 *   V[c][node] = sum w*normal[c] (V is PLANAR: (3,X,Y,Z)) and W[node] = sum w; a node without a row gets 0.  Rows with a key
 *   outside 0 .. XYZ-1 are skipped.  normals (n,3): the caller has dropped samples whose normal is not finite or is 0.
 * ufr_poisson_divergence: b = ((dx + dy) + dz) / (2h), dx = Vx[i+1] - Vx[i-1] and so on, V = 0 outside the grid.
 * ufr_poisson_laplacian: one application of A: q = (6*p - (((p[i-1] + p[i+1]) + (p[j-1] + p[j+1])) + (p[k-1] + p[k+1]))) /
 *   (h*h), p = 0 outside the grid: the negated 7-point Laplacian with Dirichlet walls one node outside, symmetric positive
 *   definite.  q must not alias p.
 * ufr_poisson_solve: x = the solution of A x = -b by plain conjugate gradients from x = 0 (r = p = -b; per iteration q = A p,
 *   alpha = r.r / p.q, x += alpha p, r -= alpha q, beta = r'.r' / r.r, p = r + beta p; a quotient whose denominator is 0 is
 *   0).  A dot product is per-block partial sums (at most UFR_POISSON_MAX_PARTIALS) that every block of the next kernel adds
 *   up in the same fixed order; the scalars stay on the device.  After every check_every iterations (and after the last)
 *   the host reads r.r: one 8-byte copy and one stream synchronisation; one more such look follows the set-up (b.b).  The
 *   iteration ends when sqrt(r.r) <= tol * sqrt(b.b), seen at a look, or after max_iter iterations.  *iterations_host = the
 *   iterations run, *residual_host = sqrt(r.r / b.b) of the recurrence at the last look, *converged_host = 1 / 0; reaching
 *   max_iter is not an error.  b = 0: x = 0, 0 iterations, residual 0, converged.  tol >= 0, max_iter >= 1, check_every >=
 *   1.  workspace >= ufr_poisson_workspace_bytes(dims) (device; three volumes and the partial sums); no allocation.
 * ufr_poisson_sample: values[p] = the trilinear value of vol at point p (cell, offsets and weights as in the splat, the eight
 *   terms added in corner order 0 .. 7); NaN for a point that is not finite.  mean_out (device fp64, nullable): the sum of
 *   the values through the same partial sums, divided by n.  1 <= n < 2^31.  workspace >=
 *   ufr_poisson_sample_workspace_bytes(n) (device).  Does not synchronise.
 * Only ufr_poisson_solve synchronises.  Every argument error (null pointer, a dim below 2, 2^31 nodes or more, h or h*h not
 * positive and finite, an origin that is not finite, a count outside its range, a workspace that is too small) is
 * UFR_ERR_ARG (UFR_ERR_WORKSPACE for the workspace) with the reason in the thread's last-error text; nothing is launched
 * then.  b with a value that is not finite is UFR_ERR_ARG after the set-up kernel.                                     */
#define UFR_POISSON_MAX_PARTIALS 1024
int ufr_poisson_grid(const double* bound_min, const double* bound_max, int32_t resolution, int32_t pad, double* origin, double* h,
                     int32_t* dims);
int ufr_poisson_splat_keys(const double* points, int64_t n, const double* origin, double h, const int32_t* dims, int64_t* keys,
                           ufr_stream stream);
int ufr_poisson_splat(const double* points, const double* normals, int64_t n, const double* origin, double h, const int32_t* dims,
                      const int64_t* keys, const int64_t* rows, double* V, double* W, ufr_stream stream);
int ufr_poisson_divergence(const double* V, const int32_t* dims, double h, double* b, ufr_stream stream);
int ufr_poisson_laplacian(const double* p, const int32_t* dims, double h, double* q, ufr_stream stream);
size_t ufr_poisson_workspace_bytes(const int32_t* dims);
int ufr_poisson_solve(const double* b, const int32_t* dims, double h, double tol, int32_t max_iter, int32_t check_every, double* x,
                      void* workspace, size_t workspace_bytes, int32_t* iterations_host, double* residual_host,
                      int32_t* converged_host, ufr_stream stream);
size_t ufr_poisson_sample_workspace_bytes(int64_t n);
int ufr_poisson_sample(const double* vol, const int32_t* dims, const double* origin, double h, const double* points, int64_t n,
                       double* values, double* mean_out, void* workspace, size_t workspace_bytes, ufr_stream stream);

void ufr_profile_enable(int on);
int ufr_profile_read(const char** names, float* ms, int32_t* launches, int cap);

#ifdef __cplusplus
}
#endif
#endif /* UFR_H */
