// extern "C" surface of libufr.so (include/ufr.h): training -- the compositor's backward and the loss, the
// forwards that record a tape, the streaming backwards of both transformers and the gather's backward.
#include "api_common.h"
#include "bwd_tape.h"

using namespace ufr;
using namespace ufr::api;

namespace {

int raw_and_grads(const ufr_raw_weights* raw, const ufr_raw_grads* grads, RawPtrs& rp, GradPtrs& gp, const char* who) {
  static_assert(sizeof(ufr_raw_grads) == sizeof(GradPtrs) && UFR_NUM_PARAMS == P_COUNT, "ufr_raw_grads layout");
  UFR_REQUIRE(raw && grads, "%s: null weights / grads", who);
  memcpy(&rp, raw, sizeof(rp));
  memcpy(&gp, grads, sizeof(gp));
  for (int i = 0; i < P_COUNT; ++i) UFR_REQUIRE(rp.p[i] && gp.p[i], "%s: parameter %d has a null pointer", who, i);
  return UFR_OK;
}

// The three kernels of the view transformer's backward (bwd_tape.h) over a caller workspace:
// [tape | dY tiles | token0 scratch | radiance scratch]
struct ViewBwdWs { float *tape, *dbuf, *token0, *radiance; int blocks; };
ViewBwdWs carve_view_bwd(Carver& c, int P, int NV) {
  ViewBwdWs w;
  w.blocks = view_tape_blocks(P, NV);
  // sized for the fp32 layouts (the 16-bit mode's are smaller)
  w.tape = c.f32((size_t)w.blocks * ViewTapeLayout<false>::block_units * 128);
  w.dbuf = c.f32((size_t)w.blocks * ViewGradLayout<false>::block_units * 128);
  w.token0 = c.f32((size_t)P * UFR_TOKEN_DIM);
  w.radiance = c.f32((size_t)P * 3);
  return w;
}
int view_bwd_impl(const void* packed, const GradPtrs& gp, const float* x_tokens, const float* rgb, const float* dir,
                  const float* d_tok_a, const float* d_tok_b, const float* d_radiance, int P, int NV, float* d_pv,
                  const ViewBwdWs& w, bool lowp, int* status, hipStream_t s, int stages = UFR_BWD_STAGE_ALL) {
  UFR_REQUIRE((unsigned long long)P * (NV + 1) * UFR_TOKEN_DIM < (1ull << 30),
              "view transformer backward: %d points x %d tokens exceed the 2^30 token values one call addresses; chunk the points", P, NV + 1);
  const float* pk = static_cast<const float*>(packed);
  if (stages & UFR_BWD_STAGE_TAPE) UFR_TIMED("view_tape", s, launch_view_tape(pk, x_tokens, rgb, dir, P, NV, w.token0, w.radiance, w.tape,
      lowp, status, s));
  if (stages & UFR_BWD_STAGE_DGRAD) UFR_TIMED("view_dgrad", s, launch_view_dgrad(pk, w.tape, rgb, d_tok_a, d_tok_b, d_radiance, P, NV,
      w.dbuf, d_pv, gp, lowp, s));
  if (stages & UFR_BWD_STAGE_WGRAD) UFR_TIMED("view_wgrad", s, launch_view_wgrad(w.tape, w.dbuf, w.blocks, gp, lowp, s));
  return UFR_OK;
}

// ... and of the ray transformer's: [order code | tape | per-ray state | dY tiles | srdf scratch]
struct RayBwdWs { float *order_pe, *tape, *state, *dbuf, *srdf; int blocks; };
RayBwdWs carve_ray_bwd(Carver& c, int RN, int SN) {
  RayBwdWs w;
  w.blocks = RN * ((SN / 16 + 1) / 2);
  w.order_pe = c.f32((size_t)SN * 8);
  w.tape = c.f32((size_t)w.blocks * RayTapeLayout<false>::block_units * 128);
  w.state = c.f32((size_t)RN * kRayStateTiles * kTileFloats);
  w.dbuf = c.f32((size_t)w.blocks * RayGradLayout<false>::block_units * 128);
  w.srdf = c.f32((size_t)RN * SN);
  return w;
}
int ray_bwd_impl(const void* packed, const GradPtrs& gp, const float* token0, const int* row, bool accumulate,
                 const float* d_srdf, int RN, int SN, float* d_tok_a, float* d_tok_b, const RayBwdWs& w, bool lowp,
                 int* status, hipStream_t s, int stages = UFR_BWD_STAGE_ALL) {
  const float* pk = static_cast<const float*>(packed);
  if (stages & UFR_BWD_STAGE_TAPE) {
    UFR_HIP(launch_order_pe(w.order_pe, SN, s));
    UFR_TIMED("ray_tape", s, launch_ray_tape(pk, token0, row, w.order_pe, RN, SN, w.srdf, w.tape, w.state, lowp, status, s));
  }
  if (stages & UFR_BWD_STAGE_DGRAD) UFR_TIMED("ray_dgrad", s, launch_ray_dgrad(pk, w.tape, w.state, d_srdf, row, accumulate, RN, SN,
      w.dbuf, d_tok_a, d_tok_b, gp, lowp, s));
  if (stages & UFR_BWD_STAGE_WGRAD) UFR_TIMED("ray_wgrad", s, launch_ray_wgrad(w.tape, w.dbuf, w.blocks, gp, lowp, s));
  return UFR_OK;
}

// ufr_aggregate_bwd's: [d token0 | ray backward | view backward]
struct AggregateBwdWs { float* d_tok; RayBwdWs ray; ViewBwdWs view; };
AggregateBwdWs carve_aggregate_bwd(Carver& c, int RN, int SN, int NV) {
  AggregateBwdWs w;
  w.d_tok = c.f32((size_t)RN * SN * UFR_TOKEN_DIM);
  w.ray = carve_ray_bwd(c, RN, SN);
  w.view = carve_view_bwd(c, RN * SN, NV);
  return w;
}

}  // namespace

extern "C" {

int ufr_composite_bwd(const float* z, const float* radiance, const int32_t* row, const float* srdf, const float* variance,
                      int32_t RN, int32_t SN, const float* d_rgb, const float* d_depth, const float* d_opacity,
                      const float* d_weight, float* d_radiance, int32_t accumulate, float* d_srdf, float* d_variance,
                      ufr_stream stream) {
  UFR_REQUIRE(z && radiance && srdf && variance && d_radiance && d_srdf && d_variance, "ufr_composite_bwd: null argument");
  UFR_REQUIRE(RN > 0 && SN >= 2 && SN <= 256, "ufr_composite_bwd: SN=%d out of range [2,256]", SN);
  hipStream_t s = static_cast<hipStream_t>(stream);
  UFR_TIMED("composite_bwd", s, launch_composite_bwd(z, radiance, row, accumulate != 0, srdf, variance, RN, SN, d_rgb, d_depth, d_opacity,
      d_weight, d_radiance, d_srdf, d_variance, s));
  return UFR_OK;
}

int ufr_render_loss(const float* rgb_c, const float* depth_c, const float* rgb_f, const float* depth_f, const float* rgb_gt,
                    const float* depth_gt, const float* near_far, int32_t nf_stride, int32_t B, int32_t RN, float weight_rgb,
                    float weight_depth, float* loss, float* d_rgb_c, float* d_depth_c, float* d_rgb_f, float* d_depth_f,
                    ufr_stream stream) {
  UFR_REQUIRE(rgb_c && depth_c && rgb_f && depth_f && rgb_gt && depth_gt && near_far && loss && d_rgb_c && d_depth_c && d_rgb_f && d_depth_f,
              "ufr_render_loss: null argument");
  UFR_REQUIRE(B > 0 && RN > 0 && nf_stride >= 2 && (long long)B * RN < (1ll << 24), "ufr_render_loss: B=%d RN=%d nf_stride=%d", B, RN, nf_stride);
  hipStream_t s = static_cast<hipStream_t>(stream);
  UFR_TIMED("render_loss", s, launch_render_loss(rgb_c, depth_c, rgb_f, depth_f, rgb_gt, depth_gt, near_far, nf_stride, B, RN, weight_rgb,
      weight_depth, loss, d_rgb_c, d_depth_c, d_rgb_f, d_depth_f, s));
  return UFR_OK;
}

size_t ufr_ray_transform_bwd_workspace_bytes(int32_t RN, int32_t SN) {
  if (RN <= 0 || SN < 16 || SN % 16 != 0) return 0;
  return carved_bytes(carve_ray_bwd, RN, SN);
}

size_t ufr_view_transform_bwd_workspace_bytes(int32_t P, int32_t NV) {
  if (P <= 0 || !views_ok(NV)) return 0;
  return carved_bytes(carve_view_bwd, P, NV);
}

size_t ufr_aggregate_bwd_workspace_bytes(int32_t RN, int32_t SN, int32_t NV) {
  if (RN <= 0 || SN < 16 || SN % 16 != 0 || !views_ok(NV)) return 0;
  return carved_bytes(carve_aggregate_bwd, RN, SN, NV);
}

int ufr_aggregate_bwd(const ufr_raw_weights* raw, const ufr_raw_grads* grads, const void* packed_weights, const float* x_tokens,
                      const float* rgb, const float* dir, const float* token0, int32_t RN, int32_t SN, int32_t NV,
                      const float* d_radiance, const float* d_srdf, float* d_pv, void* workspace,
                      int32_t precision, ufr_stream stream) {
  RawPtrs rp;
  GradPtrs gp;
  UFR_CHECK(raw_and_grads(raw, grads, rp, gp, "ufr_aggregate_bwd"));
  UFR_PRECISION(precision, lowp, "ufr_aggregate_bwd");
  UFR_REQUIRE(packed_weights && x_tokens && rgb && dir && token0 && d_radiance && d_srdf && d_pv && workspace, "ufr_aggregate_bwd: null argument");
  UFR_CHECK(check_views("ufr_aggregate_bwd", NV));
  UFR_CHECK(check_ray_samples("ufr_aggregate_bwd", RN, SN));
  hipStream_t s = static_cast<hipStream_t>(stream);
  Carver c(workspace);
  const AggregateBwdWs w = carve_aggregate_bwd(c, RN, SN, NV);
  UFR_STATUS_SLOT(sl);
  UFR_CHECK(ray_bwd_impl(packed_weights, gp, token0, nullptr, false, d_srdf, RN, SN, w.d_tok, nullptr, w.ray, lowp, status_word(sl), s));
  return view_bwd_impl(packed_weights, gp, x_tokens, rgb, dir, w.d_tok, nullptr, d_radiance, RN * SN, NV, d_pv, w.view, lowp,
                       status_word(sl), s);
}

size_t ufr_project_gather_bwd_workspace_bytes(const ufr_frame* frame) {
  const FrameDev* f = frame_of(frame);
  return (f && f->vol[0]) ? align_up(gather_bwd_scratch_floats(*f) * sizeof(float)) : 0;
}

int ufr_project_gather_bwd(const ufr_frame* frame, const ufr_raw_weights* raw, const ufr_raw_grads* grads,
                           const float* ray_o, int32_t ray_o_stride, const float* ray_d, const float* z, int32_t RN,
                           int32_t SN, const float* sim8, const float* d_pv, const int32_t* row,
                           float* const* grad_vol_feat, float* const* grad_vol_weight, int32_t accumulate, void* workspace,
                           int32_t precision, ufr_stream stream) {
  const FrameDev* f = frame_of(frame);
  UFR_REQUIRE(f, "ufr_project_gather_bwd: frame handle not prepared");
  UFR_PRECISION(precision, lowp, "ufr_project_gather_bwd");
  RawPtrs rp;
  GradPtrs gp;
  UFR_CHECK(raw_and_grads(raw, grads, rp, gp, "ufr_project_gather_bwd"));
  UFR_REQUIRE(ray_o && ray_d && z && sim8 && d_pv, "ufr_project_gather_bwd: null argument");
  const bool scatter = grad_vol_feat != nullptr || grad_vol_weight != nullptr;   // both NULL: pre_sim_mlp gradients only
  UFR_REQUIRE(!scatter || (grad_vol_feat && grad_vol_weight && f->vol[0]),
              "ufr_project_gather_bwd: volume gradients need both pointer arrays and a frame prepared with volumes");
  UFR_REQUIRE(ray_o_stride == 0 || ray_o_stride == 3, "ufr_project_gather_bwd: ray_o_stride must be 0 or 3");
  UFR_REQUIRE(RN > 0 && SN > 0, "ufr_project_gather_bwd: RN=%d SN=%d", RN, SN);
  for (int i = 0; scatter && i < UFR_NUM_STAGES; ++i)
    UFR_REQUIRE(grad_vol_feat[i] && grad_vol_weight[i], "ufr_project_gather_bwd: null volume gradient (stage %d)", i + 1);
  UFR_REQUIRE(!scatter || workspace, "ufr_project_gather_bwd: the volume scatter needs its workspace");
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (scatter) UFR_TIMED("gather_bwd", s, launch_gather_bwd(*f, grad_vol_feat, grad_vol_weight, ray_o, ray_o_stride, ray_d, z, d_pv, row,
      RN, SN, static_cast<float*>(workspace), (accumulate & UFR_GBWD_ACCUMULATE) != 0, (accumulate & UFR_GBWD_WORKSPACE_ZEROED) != 0, s));
  if (!(accumulate & UFR_GBWD_NO_PRESIM)) UFR_TIMED("presim_bwd", s, launch_presim_bwd(rp, gp, sim8, d_pv, RN * SN, lowp, s));
  return UFR_OK;
}

// The forward WITH the tape (training): the TAPE instantiation of the forward kernel writes token0 / radiance like
// ufr_view_transform and records the activations into the backward's workspace, so that the backward starts at its
// data-gradient stage -- nothing is computed twice.
int32_t ufr_view_tape_block_points(int32_t NV) { return views_ok(NV) ? (16 / (NV + 1)) * kBlockCols : 0; }

int ufr_view_transform_tape(const void* packed_weights, const float* x_tokens, const float* rgb, const float* dir, int32_t P,
                            int32_t NV, float* token0, float* radiance, void* workspace, int32_t p0, int32_t P_total,
                            int32_t precision, ufr_stream stream) {
  UFR_REQUIRE(packed_weights && x_tokens && rgb && dir && token0 && radiance && workspace, "ufr_view_transform_tape: null argument");
  UFR_CHECK(check_views("ufr_view_transform_tape", NV));
  UFR_REQUIRE(P > 0 && p0 >= 0 && p0 + P <= P_total, "ufr_view_transform_tape: P=%d p0=%d P_total=%d", P, p0, P_total);
  const int ppw = ufr_view_tape_block_points(NV);
  UFR_REQUIRE(p0 % ppw == 0 && (p0 + P == P_total || P % ppw == 0),
              "ufr_view_transform_tape: the point range [%d, %d) must start and (unless it closes the pool) end on a multiple of %d points",
              p0, p0 + P, ppw);
  UFR_REQUIRE((unsigned long long)P_total * (NV + 1) * UFR_TOKEN_DIM < (1ull << 30),
              "ufr_view_transform_tape: %d points x %d tokens exceed the 2^30 token values one backward addresses", P_total, NV + 1);
  UFR_PRECISION(precision, lowp, "ufr_view_transform_tape");
  hipStream_t s = static_cast<hipStream_t>(stream);
  Carver c(workspace);
  const ViewBwdWs vw = carve_view_bwd(c, P_total, NV);
  UFR_STATUS_ENTER(sl, s, "ufr_view_transform_tape");
  const size_t blk_floats = (size_t)(lowp ? ViewTapeLayout<true>::block_units : ViewTapeLayout<false>::block_units) * 128;
  UFR_TIMED("view_tape", s, launch_view_tape(static_cast<const float*>(packed_weights), x_tokens, rgb, dir, P, NV, token0, radiance,
      vw.tape + (size_t)(p0 / ppw) * blk_floats, lowp, status_word(sl), s));
  return status_leave(sl, s);
}

int ufr_ray_transform_tape(const void* packed_weights, const float* token0, const int32_t* row, int32_t RN, int32_t SN,
                           float* srdf, void* workspace, int32_t precision, ufr_stream stream) {
  UFR_REQUIRE(packed_weights && token0 && srdf && workspace, "ufr_ray_transform_tape: null argument");
  UFR_CHECK(check_ray_samples("ufr_ray_transform_tape", RN, SN));
  UFR_PRECISION(precision, lowp, "ufr_ray_transform_tape");
  hipStream_t s = static_cast<hipStream_t>(stream);
  Carver c(workspace);
  const RayBwdWs rw = carve_ray_bwd(c, RN, SN);
  UFR_STATUS_ENTER(sl, s, "ufr_ray_transform_tape");
  UFR_HIP(launch_order_pe(rw.order_pe, SN, s));
  UFR_TIMED("ray_tape", s, launch_ray_tape(static_cast<const float*>(packed_weights), token0, row, rw.order_pe, RN, SN, srdf, rw.tape,
      rw.state, lowp, status_word(sl), s));
  return status_leave(sl, s);
}

int ufr_ray_transform_bwd(const ufr_raw_weights* raw, const ufr_raw_grads* grads, const void* packed_weights, const float* token0,
                          const int32_t* row, int32_t RN, int32_t SN, const float* d_srdf, float* d_token0_a, float* d_token0_b,
                          int32_t accumulate, void* workspace, int32_t precision, ufr_stream stream) {
  return ufr_ray_transform_bwd_stages(raw, grads, packed_weights, token0, row, RN, SN, d_srdf, d_token0_a, d_token0_b, accumulate,
                                      workspace, UFR_BWD_STAGE_ALL, precision, stream);
}

int ufr_ray_transform_bwd_stages(const ufr_raw_weights* raw, const ufr_raw_grads* grads, const void* packed_weights,
                                 const float* token0, const int32_t* row, int32_t RN, int32_t SN, const float* d_srdf,
                                 float* d_token0_a, float* d_token0_b, int32_t accumulate, void* workspace, int32_t stages,
                                 int32_t precision, ufr_stream stream) {
  RawPtrs rp;
  GradPtrs gp;
  UFR_CHECK(raw_and_grads(raw, grads, rp, gp, "ufr_ray_transform_bwd"));
  UFR_PRECISION(precision, lowp, "ufr_ray_transform_bwd");
  UFR_REQUIRE(stages > 0 && (stages & ~UFR_BWD_STAGE_ALL) == 0, "ufr_ray_transform_bwd_stages: stages=%d", stages);
  UFR_REQUIRE(packed_weights && workspace, "ufr_ray_transform_bwd: null argument");
  UFR_REQUIRE(!(stages & UFR_BWD_STAGE_TAPE) || token0, "ufr_ray_transform_bwd: the tape stage needs token0");
  UFR_REQUIRE(!(stages & UFR_BWD_STAGE_DGRAD) || (d_srdf && d_token0_a), "ufr_ray_transform_bwd: the data-gradient stage needs d_srdf, d_token0_a");
  UFR_CHECK(check_ray_samples("ufr_ray_transform_bwd", RN, SN));
  hipStream_t s = static_cast<hipStream_t>(stream);
  Carver c(workspace);
  const RayBwdWs rw = carve_ray_bwd(c, RN, SN);
  UFR_STATUS_SLOT(sl);
  return ray_bwd_impl(packed_weights, gp, token0, row, accumulate != 0, d_srdf, RN, SN, d_token0_a, d_token0_b, rw, lowp,
                      status_word(sl), s, stages);
}

int ufr_view_transform_bwd(const ufr_raw_weights* raw, const ufr_raw_grads* grads, const void* packed_weights,
                           const float* x_tokens, const float* rgb, const float* dir, const float* d_token0_a,
                           const float* d_token0_b, const float* d_radiance, int32_t P, int32_t NV, float* d_pv, void* workspace,
                           int32_t precision, ufr_stream stream) {
  return ufr_view_transform_bwd_stages(raw, grads, packed_weights, x_tokens, rgb, dir, d_token0_a, d_token0_b, d_radiance, P, NV, d_pv,
                                       workspace, UFR_BWD_STAGE_ALL, precision, stream);
}

int ufr_view_transform_bwd_stages(const ufr_raw_weights* raw, const ufr_raw_grads* grads, const void* packed_weights,
                                  const float* x_tokens, const float* rgb, const float* dir, const float* d_token0_a,
                                  const float* d_token0_b, const float* d_radiance, int32_t P, int32_t NV, float* d_pv,
                                  void* workspace, int32_t stages, int32_t precision, ufr_stream stream) {
  RawPtrs rp;
  GradPtrs gp;
  UFR_CHECK(raw_and_grads(raw, grads, rp, gp, "ufr_view_transform_bwd"));
  UFR_PRECISION(precision, lowp, "ufr_view_transform_bwd");
  UFR_REQUIRE(stages > 0 && (stages & ~UFR_BWD_STAGE_ALL) == 0, "ufr_view_transform_bwd_stages: stages=%d", stages);
  UFR_REQUIRE(packed_weights && workspace, "ufr_view_transform_bwd: null argument");
  UFR_REQUIRE(!(stages & UFR_BWD_STAGE_TAPE) || (x_tokens && rgb && dir), "ufr_view_transform_bwd: the tape stage needs x_tokens, rgb, dir");
  UFR_REQUIRE(!(stages & UFR_BWD_STAGE_DGRAD) || (rgb && d_token0_a && d_radiance && d_pv),
              "ufr_view_transform_bwd: the data-gradient stage needs rgb, d_token0_a, d_radiance, d_pv");
  UFR_CHECK(check_views("ufr_view_transform_bwd", NV));
  UFR_REQUIRE(P > 0, "ufr_view_transform_bwd: P=%d", P);
  hipStream_t s = static_cast<hipStream_t>(stream);
  Carver c(workspace);
  const ViewBwdWs vw = carve_view_bwd(c, P, NV);
  UFR_STATUS_SLOT(sl);
  return view_bwd_impl(packed_weights, gp, x_tokens, rgb, dir, d_token0_a, d_token0_b, d_radiance, P, NV, d_pv, vw, lowp,
                       status_word(sl), s, stages);
}

}  // extern "C"
