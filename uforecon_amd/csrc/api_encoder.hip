// extern "C" surface of libufr.so (include/ufr.h): the encoder -- correlation volumes and view weights, the
// 3-D convolutions of the frustum U-Nets, the 2-D and deformable convolutions of the feature backbone, the FMT layer, and
// what a scan loader feeds them (image planes from 8-bit pictures, with or without a foreground mask; the per-pixel ray tables)
// and what a COLMAP model's converter asks before any of it (the pair scores of the view selection, the undistorted pictures).
#include "api_common.h"

using namespace ufr;
using namespace ufr::api;

namespace {
// [reference features, channel-last | source features, channel-last]
struct CorrelateWs { float *ref_cl, *src_cl; };
CorrelateWs carve_correlate(Carver& c, int C, int H, int W, int NS) {
  CorrelateWs w;
  w.ref_cl = c.f32((size_t)H * W * C);
  w.src_cl = c.f32((size_t)NS * H * W * C);
  return w;
}

// [input, channel-last]
float* carve_deform_conv2d(Carver& c, int B, int C, int H, int W) { return c.f32((size_t)B * H * W * C); }
}  // namespace

extern "C" {

// ------------------------------------------------------------------ correlation-volume construction
size_t ufr_correlate_workspace_bytes(int32_t C, int32_t H, int32_t W, int32_t NS) {
  return carved_bytes(carve_correlate, C, H, W, NS);
}

int ufr_frustum_correlate(const float* ref_fea, const float* src_fea, const float* rel_proj, const float* depth_values,
                          const float* view_weights, int32_t C, int32_t H, int32_t W, int32_t D, int32_t NS,
                          float* similarity, float* aggregated, void* workspace, size_t workspace_bytes,
                          ufr_stream stream) {
  UFR_REQUIRE(ref_fea && src_fea && rel_proj && depth_values && workspace, "ufr_frustum_correlate: null argument");
  UFR_REQUIRE(similarity || aggregated, "ufr_frustum_correlate: no output requested");
  UFR_REQUIRE(!aggregated || view_weights, "ufr_frustum_correlate: aggregated output needs view_weights");
  UFR_REQUIRE(C == 4 || C == 8 || C == 16 || C == 32 || C == 64, "ufr_frustum_correlate: C=%d unsupported (4,8,16,32,64)", C);
  UFR_REQUIRE(NS >= 1 && NS <= UFR_MAX_VIEWS, "ufr_frustum_correlate: NS=%d unsupported (1..%d)", NS, UFR_MAX_VIEWS);
  UFR_REQUIRE(H >= 2 && W >= 2 && D >= 1, "ufr_frustum_correlate: H=%d W=%d D=%d", H, W, D);
  Carver c(workspace);
  const CorrelateWs w = carve_correlate(c, C, H, W, NS);
  UFR_CHECK(check_workspace("ufr_frustum_correlate", workspace_bytes, c.off));
  hipStream_t s = static_cast<hipStream_t>(stream);
  ProfScope p("correlate", s);
  UFR_HIP(launch_chw_to_hwc(ref_fea, w.ref_cl, 1, C, H * W, s));
  UFR_HIP(launch_chw_to_hwc(src_fea, w.src_cl, NS, C, H * W, s));
  UFR_HIP(launch_correlate(w.ref_cl, w.src_cl, rel_proj, NS, depth_values, view_weights, similarity, aggregated, C, H, W, D, s));
  return UFR_OK;
}

int ufr_pixelwise_view_weights(const float* similarity, const float* params, float* view_weights, float* aggregated, int32_t NS,
                               int32_t D, int32_t H, int32_t W, ufr_stream stream) {
  UFR_REQUIRE(similarity && params && view_weights, "ufr_pixelwise_view_weights: null argument");
  UFR_REQUIRE(NS >= 1 && NS <= UFR_MAX_VIEWS && D >= 1 && H >= 1 && W >= 1, "ufr_pixelwise_view_weights: NS=%d D=%d H=%d W=%d", NS, D, H, W);
  hipStream_t s = static_cast<hipStream_t>(stream);
  UFR_TIMED("pixelwise_view_weights", s, launch_pixelwise_weights(similarity, params, view_weights, aggregated, NS, D, H, W, s));
  return UFR_OK;
}

// ------------------------------------------------------------------ 3-D convolutions of the frustum U-Nets
int ufr_conv3d(const float* in, const float* weight, const float* weight2, const float* bias, const float* bn_scale,
               const float* bn_shift, const float* skip, float* out, float* out2, int32_t B, int32_t D, int32_t H,
               int32_t W, int32_t cin, int32_t cout, int32_t cout2, int32_t mode, int32_t relu, int32_t out_ncdhw,
               float* out_absmax, ufr_stream stream) {
  UFR_REQUIRE(in && weight && out, "ufr_conv3d: null argument");
  UFR_REQUIRE(B > 0 && D > 0 && H > 0 && W > 0, "ufr_conv3d: B=%d D=%d H=%d W=%d", B, D, H, W);
  UFR_CHECK(check_conv3d_mode("ufr_conv3d", mode));
  UFR_REQUIRE((bn_scale == nullptr) == (bn_shift == nullptr), "ufr_conv3d: bn_scale and bn_shift go together");
  UFR_REQUIRE(cout2 == 0 || (weight2 && out2 && out_ncdhw && mode == UFR_CONV3D_S1),
              "ufr_conv3d: a second head needs weight2, out2, out_ncdhw and stride 1");
  UFR_REQUIRE(out_ncdhw || (cout % 4 == 0 && cout2 == 0), "ufr_conv3d: channel-last outputs need cout %% 4 == 0 (got %d)", cout);
  UFR_REQUIRE(!skip || !out_ncdhw, "ufr_conv3d: skip is a channel-last tensor; not with out_ncdhw");
  UFR_REQUIRE((long long)B * D * H * W * (cin > cout ? cin : cout) < (1ll << 40), "ufr_conv3d: volume too large");
  hipStream_t s = static_cast<hipStream_t>(stream);
  ProfScope p("conv3d", s);
  UFR_REQUIRE(!out_absmax || (!out_ncdhw && cout <= 16), "ufr_conv3d: out_absmax goes with channel-last outputs of at most 16 channels");
  const hipError_t e = launch_conv3d(in, weight, weight2, bias, bn_scale, bn_shift, skip, out, out2, B, D, H, W, cin, cout,
                                     cout2, mode, relu, out_ncdhw, s, 0, out_absmax);
  if (e == hipErrorInvalidValue)
    return fail(UFR_ERR_ARG, "ufr_conv3d: (cin %d, cout %d+%d, mode %d) is not a layer of CostRegNet / CostRegNetWeight", cin,
                cout, cout2, mode);
  UFR_HIP(e);
  return UFR_OK;
}

// the stride-1 8 / 16-channel layers on the 16-bit matrix cores (conv3d_planes.hip)
size_t ufr_conv3d_planes_workspace_bytes(int32_t cin, int32_t cout, int32_t cout2, int32_t mode) {
  return conv3d_planes_workspace_bytes(cin, cout, cout2, mode);
}

int ufr_conv3d_planes(const float* in, const float* in_absmax, const float* weight, const float* weight2, const float* bias,
                      const float* bn_scale, const float* bn_shift, const float* skip, float* out, float* out2,
                      float* out_absmax, int32_t B, int32_t D, int32_t H, int32_t W, int32_t cin, int32_t cout, int32_t cout2,
                      int32_t mode, int32_t relu, int32_t out_ncdhw, int32_t flip, void* workspace, size_t workspace_bytes, int32_t planes_ready,
                      ufr_stream stream) {
  UFR_REQUIRE(in && in_absmax && weight && out && workspace, "ufr_conv3d_planes: null argument");
  UFR_REQUIRE(B > 0 && D > 0 && H > 0 && W > 0, "ufr_conv3d_planes: B=%d D=%d H=%d W=%d", B, D, H, W);
  UFR_REQUIRE((bn_scale == nullptr) == (bn_shift == nullptr), "ufr_conv3d_planes: bn_scale and bn_shift go together");
  UFR_REQUIRE(cout2 == 0 || (weight2 && out2 && out_ncdhw && !flip), "ufr_conv3d_planes: a second head needs weight2, out2, out_ncdhw");
  UFR_REQUIRE(out_ncdhw || (cout % 4 == 0 && cout2 == 0), "ufr_conv3d_planes: channel-last outputs need cout %% 4 == 0 (got %d)", cout);
  UFR_REQUIRE(!(out_ncdhw && (skip || out_absmax)), "ufr_conv3d_planes: skip / out_absmax go with channel-last outputs");
  UFR_CHECK(check_conv3d_mode("ufr_conv3d_planes", mode));
  UFR_REQUIRE(!(mode != UFR_CONV3D_S1 && flip), "ufr_conv3d_planes: flip is the stride-1 data gradient");
  UFR_REQUIRE(!(mode == UFR_CONV3D_T2 && out_ncdhw), "ufr_conv3d_planes: the transposed layers write channel-last");
  const size_t need = conv3d_planes_workspace_bytes(cin, cout, cout2, mode);
  if (!need) return fail(UFR_ERR_ARG, "ufr_conv3d_planes: (cin %d, cout %d+%d, mode %d) is not a layer of this kernel family", cin, cout, cout2, mode);
  UFR_CHECK(check_workspace("ufr_conv3d_planes", workspace_bytes, need));
  UFR_REQUIRE((long long)D * H * W * cin * 4 < (1ll << 31), "ufr_conv3d_planes: one batch element reaches 2 GiB");
  hipStream_t s = static_cast<hipStream_t>(stream);
  UFR_TIMED(flip ? "conv3d_dgrad" : "conv3d", s, launch_conv3d_planes(in, in_absmax, weight, weight2, bias, bn_scale, bn_shift, skip, out,
      out2, out_absmax, B, D, H, W, cin, cout, cout2, mode, relu, out_ncdhw, flip, workspace, planes_ready != 0, s));
  return UFR_OK;
}

int ufr_absmax(const float* x, size_t n, float* absmax, ufr_stream stream) {
  UFR_REQUIRE(x && absmax, "ufr_absmax: null argument");
  UFR_HIP(launch_absmax(x, n, absmax, static_cast<hipStream_t>(stream)));
  return UFR_OK;
}

// backward of the plain layers (CostRegNetWeight: the producer the reference trains) -- conv3d.hip, second half
int ufr_conv3d_bwd_data(const float* d_out, const float* weight, const float* accumulate, float* d_in, int32_t B, int32_t D,
                        int32_t H, int32_t W, int32_t cin, int32_t cout, int32_t mode, ufr_stream stream) {
  UFR_REQUIRE(d_out && weight && d_in, "ufr_conv3d_bwd_data: null argument");
  UFR_REQUIRE(B > 0 && D > 0 && H > 0 && W > 0, "ufr_conv3d_bwd_data: B=%d D=%d H=%d W=%d", B, D, H, W);
  UFR_CHECK(check_conv3d_mode("ufr_conv3d_bwd_data", mode));
  UFR_REQUIRE(mode != UFR_CONV3D_S2 || (D % 2 == 0 && H % 2 == 0 && W % 2 == 0), "ufr_conv3d_bwd_data: stride 2 needs even extents");
  UFR_REQUIRE(cin == 1 || cin % 4 == 0, "ufr_conv3d_bwd_data: cin=%d", cin);
  UFR_REQUIRE(!(cin == 1 && accumulate), "ufr_conv3d_bwd_data: no fused addition into a 1-channel gradient");
  hipStream_t s = static_cast<hipStream_t>(stream);
  ProfScope p("conv3d_dgrad", s);
  const hipError_t e = launch_conv3d_bwd_data(d_out, weight, accumulate, d_in, B, D, H, W, cin, cout, mode, s);
  if (e == hipErrorInvalidValue)
    return fail(UFR_ERR_ARG, "ufr_conv3d_bwd_data: (cin %d, cout %d, mode %d) is not a layer of CostRegNetWeight", cin, cout, mode);
  UFR_HIP(e);
  return UFR_OK;
}

int ufr_conv3d_bwd_weight(const float* in, const float* d_out, float* d_weight, float* d_bias, int32_t B, int32_t D, int32_t H,
                          int32_t W, int32_t cin, int32_t cout, int32_t mode, ufr_stream stream) {
  UFR_REQUIRE(in && d_out && d_weight, "ufr_conv3d_bwd_weight: null argument");
  UFR_REQUIRE(B > 0 && D > 0 && H > 0 && W > 0, "ufr_conv3d_bwd_weight: B=%d D=%d H=%d W=%d", B, D, H, W);
  UFR_CHECK(check_conv3d_mode("ufr_conv3d_bwd_weight", mode));
  UFR_REQUIRE(mode != UFR_CONV3D_S2 || (D % 2 == 0 && H % 2 == 0 && W % 2 == 0), "ufr_conv3d_bwd_weight: stride 2 needs even extents");
  hipStream_t s = static_cast<hipStream_t>(stream);
  ProfScope p("conv3d_wgrad", s);
  const hipError_t e = launch_conv3d_bwd_weight(in, d_out, d_weight, d_bias, B, D, H, W, cin, cout, mode, s);
  if (e == hipErrorInvalidValue)
    return fail(UFR_ERR_ARG, "ufr_conv3d_bwd_weight: (cin %d, cout %d, mode %d) is not a layer of CostRegNetWeight", cin, cout, mode);
  UFR_HIP(e);
  return UFR_OK;
}

int ufr_conv3d_bwd_weight_heads(const float* in, const float* d_out, const float* d_out2, float* d_weight, float* d_weight2, int32_t B,
                                int32_t D, int32_t H, int32_t W, ufr_stream stream) {
  UFR_REQUIRE(in && d_out && d_out2 && d_weight && d_weight2, "ufr_conv3d_bwd_weight_heads: null argument");
  UFR_REQUIRE(B > 0 && D > 0 && H > 0 && W > 0, "ufr_conv3d_bwd_weight_heads: B=%d D=%d H=%d W=%d", B, D, H, W);
  UFR_REQUIRE((long long)D * H * W * 32 < (1ll << 31), "ufr_conv3d_bwd_weight_heads: one batch element reaches 2 GiB");
  hipStream_t s = static_cast<hipStream_t>(stream);
  UFR_TIMED("conv3d_wgrad", s, launch_conv3d_wgrad_heads(in, d_out, d_out2, d_weight, d_weight2, B, D, H, W, s));
  return UFR_OK;
}

// ------------------------------------------------------------------ deformable convolution
size_t ufr_deform_conv2d_workspace_bytes(int32_t B, int32_t C, int32_t H, int32_t W) {
  return carved_bytes(carve_deform_conv2d, B, C, H, W);
}

int ufr_deform_conv2d(const float* input, const float* offset, const float* mask, const float* weight,
                      const float* bias, float* output, int32_t B, int32_t C, int32_t Cout, int32_t H, int32_t W,
                      void* workspace, size_t workspace_bytes, ufr_stream stream) {
  UFR_REQUIRE(input && offset && weight && output && workspace, "ufr_deform_conv2d: null argument");
  UFR_REQUIRE(C > 0 && C % 4 == 0 && C <= 32, "ufr_deform_conv2d: C=%d unsupported (multiple of 4, <= 32)", C);
  UFR_REQUIRE(Cout == 8 || Cout == 16 || Cout == 32, "ufr_deform_conv2d: Cout=%d unsupported (8, 16, 32)", Cout);
  UFR_REQUIRE(B > 0 && H > 0 && W > 0, "ufr_deform_conv2d: B=%d H=%d W=%d", B, H, W);
  Carver c(workspace);
  float* in_cl = carve_deform_conv2d(c, B, C, H, W);
  UFR_CHECK(check_workspace("ufr_deform_conv2d", workspace_bytes, c.off));
  hipStream_t s = static_cast<hipStream_t>(stream);
  ProfScope p("deform_conv2d", s);
  UFR_HIP(launch_chw_to_hwc(input, in_cl, B, C, H * W, s));
  UFR_HIP(launch_deform_conv3x3(in_cl, offset, mask, weight, bias, output, B, C, Cout, H, W, s));
  return UFR_OK;
}

int ufr_deform_conv2d_cl(const float* input_cl, const float* offset_mask, const float* weight, const float* bias,
                         const float* scale, const float* shift, float* output, int32_t B, int32_t C, int32_t Cout, int32_t H,
                         int32_t W, int32_t flags, ufr_stream stream) {
  const float* offset = offset_mask;
  UFR_REQUIRE(input_cl && offset && weight && output, "ufr_deform_conv2d_cl: null argument");
  const float* mask = offset_mask + (size_t)18 * H * W;
  UFR_REQUIRE(C == 32, "ufr_deform_conv2d_cl: C=%d (the channel-last form exists for the 32-channel layers of FeatureNet)", C);
  UFR_REQUIRE(Cout == 8 || Cout == 16 || Cout == 32, "ufr_deform_conv2d_cl: Cout=%d unsupported (8, 16, 32)", Cout);
  UFR_REQUIRE(B > 0 && H > 0 && W > 0, "ufr_deform_conv2d_cl: B=%d H=%d W=%d", B, H, W);
  UFR_REQUIRE((scale == nullptr) == (shift == nullptr), "ufr_deform_conv2d_cl: scale and shift come together");
  hipStream_t s = static_cast<hipStream_t>(stream);
  UFR_TIMED("deform_conv2d", s, launch_deform_conv3x3(input_cl, offset, mask, weight, bias, output, B, C, Cout, H, W, s,
      DcnEpilogue{scale, shift, (flags & UFR_CONV2D_RELU) != 0, (flags & UFR_CONV2D_OUT_PLANAR) == 0, 27}));
  return UFR_OK;
}

// channel-last pipeline of the feature backbone (conv2d.hip; featurenet.py is the plan)
int ufr_conv2d(const float* input, const float* weight, const float* scale, const float* shift, const float* skip, float* output,
               int32_t B, int32_t cin, int32_t cout, int32_t H, int32_t W, int32_t ksize, int32_t stride, int32_t flags,
               int32_t sigmoid_from, ufr_stream stream) {
  UFR_REQUIRE(input && weight && output, "ufr_conv2d: null argument");
  UFR_REQUIRE(B > 0 && H > 0 && W > 0 && cout > 0 && cout <= 32, "ufr_conv2d: B=%d H=%d W=%d cout=%d", B, H, W, cout);
  UFR_REQUIRE((ksize == 1 || ksize == 3 || ksize == 5) && (stride == 1 || stride == 2), "ufr_conv2d: ksize=%d stride=%d", ksize, stride);
  UFR_REQUIRE((unsigned long long)H * W * (cin > 3 ? cin : 4) * 4ull < (1ull << 31), "ufr_conv2d: %d x %d x %d exceeds 2^31 bytes per image", H, W, cin);
  Conv2dArgs a;
  a.in = input; a.w = weight; a.scale = scale; a.shift = shift; a.skip = skip; a.out = output;
  a.B = B; a.H = H; a.W = W; a.cout = cout;
  a.Ho = (H + 2 * (ksize / 2) - ksize) / stride + 1;
  a.Wo = (W + 2 * (ksize / 2) - ksize) / stride + 1;
  a.relu = (flags & UFR_CONV2D_RELU) != 0;
  a.out_planar = (flags & UFR_CONV2D_OUT_PLANAR) != 0;
  a.sigmoid_from = sigmoid_from;
  UFR_REQUIRE(!skip || (a.Ho % 2 == 0 && a.Wo % 2 == 0 && cout % 4 == 0), "ufr_conv2d: the upsampled skip needs even output extents and cout %% 4 == 0");
  hipStream_t s = static_cast<hipStream_t>(stream);
  ProfScope p("conv2d", s);
  const hipError_t e = launch_conv2d(a, cin, ksize, stride, (flags & UFR_CONV2D_IN_PLANAR) != 0, s);
  if (e == hipErrorInvalidValue)
    return fail(UFR_ERR_ARG, "ufr_conv2d: %d -> %d channels, %dx%d, stride %d is not a layer shape of FeatureNet (conv2d.hip)", cin, cout, ksize, ksize, stride);
  UFR_HIP(e);
  return UFR_OK;
}

int ufr_upsample_add(const float* reduced_cl, const float* fine, float* output_cl, int32_t B, int32_t C, int32_t h, int32_t w,
                     ufr_stream stream) {
  UFR_REQUIRE(reduced_cl && fine && output_cl, "ufr_upsample_add: null argument");
  UFR_REQUIRE((C == 8 || C == 16) && B > 0 && h > 0 && w > 0, "ufr_upsample_add: B=%d C=%d h=%d w=%d (C in {8, 16})", B, C, h, w);
  hipStream_t s = static_cast<hipStream_t>(stream);
  UFR_TIMED("upsample_add", s, launch_upsample_add(reduced_cl, fine, output_cl, B, C, h, w, s));
  return UFR_OK;
}

// ------------------------------------------------------------------ feature-matching transformer layer
size_t ufr_fmt_layer_workspace_bytes(int32_t N, int32_t S) {
  return align_up((size_t)(N > 0 ? N : 1) * 160 * sizeof(float) * (1 + (size_t)fmt_state_parts(S > 0 ? S : 1)));
}

int ufr_fmt_layer(const ufr_fmt_layer_weights* w, const float* x, const float* src, int32_t N, int32_t T, int32_t S,
                  float* out, void* workspace, ufr_stream stream) {
  static_assert(sizeof(ufr_fmt_layer_weights) == sizeof(FmtWeights), "ufr_fmt_layer_weights layout");
  UFR_REQUIRE(w && x && out && workspace, "ufr_fmt_layer: null argument");
  FmtWeights fw;
  memcpy(&fw, w, sizeof(fw));
  const float* const* pw = reinterpret_cast<const float* const*>(&fw);
  for (int i = 0; i < 16; ++i) UFR_REQUIRE(pw[i], "ufr_fmt_layer: weight pointer %d is null", i);
  if (!src) { src = x; S = T; }
  UFR_REQUIRE(N > 0 && T > 0 && S > 0, "ufr_fmt_layer: N=%d T=%d S=%d", N, T, S);
  UFR_REQUIRE(out != x && out != src, "ufr_fmt_layer: out must not alias an input");
  hipStream_t s = static_cast<hipStream_t>(stream);
  UFR_TIMED("fmt_layer", s, launch_fmt_layer(fw, x, src, N, T, S, out, static_cast<float*>(workspace), s));
  return UFR_OK;
}

}  // extern "C"

// ------------------------------------------------------------------ the encoder's inputs: image planes and ray tables
namespace {
// ufr_image_resize_u8 (mask null, masked false) and ufr_image_resize_mask_u8: one contract, one launcher
int image_resize(const char* who, const char* timer, const uint8_t* src, const uint8_t* mask, bool masked, int32_t n, int32_t Hs,
                 int32_t Ws, int32_t H, int32_t W, const int32_t* clip4, float* dst, ufr_stream stream) {
  UFR_REQUIRE(src && dst && (mask || !masked), "%s: null argument", who);
  UFR_REQUIRE(n >= 1 && Hs >= 1 && Ws >= 1 && H >= 1 && W >= 1, "%s: n %d, source %dx%d, resized %dx%d (each must be >= 1)", who, n, Hs,
              Ws, H, W);
  UFR_REQUIRE((long long)Hs * Ws < (1ll << 31) && (long long)H * W < (1ll << 31), "%s: an image of %dx%d or %dx%d has 2^31 pixels or more",
              who, Hs, Ws, H, W);
  int clip[4] = {0, 0, 0, 0};   // left, top, right, bottom
  if (clip4) memcpy(clip, clip4, sizeof(clip));
  UFR_REQUIRE(clip[0] >= 0 && clip[1] >= 0 && clip[2] >= 0 && clip[3] >= 0, "%s: clip %d %d %d %d (each must be >= 0)", who, clip[0],
              clip[1], clip[2], clip[3]);
  const long long Wo = (long long)W - clip[0] - clip[2], Ho = (long long)H - clip[1] - clip[3];
  UFR_REQUIRE(Wo >= 1 && Ho >= 1, "%s: clip %d %d %d %d leaves nothing of %dx%d", who, clip[0], clip[1], clip[2], clip[3], H, W);
  UFR_REQUIRE((long long)n * Ho * Wo * 3 < (1ll << 38) && (long long)n * Hs * Ws * 3 < (1ll << 40),
              "%s: %d images of %dx%d from %dx%d are too many bytes", who, n, H, W, Hs, Ws);
  hipStream_t s = static_cast<hipStream_t>(stream);
  UFR_TIMED(timer, s, launch_image_resize_u8(src, mask, n, Hs, Ws, H, W, clip[0], clip[1], (int)Ho, (int)Wo, dst, s));
  return UFR_OK;
}

// view selection: [the CSR offsets, on the device, int64 x (N + 1) | every image's observation list sorted, int32 x n_obs]
struct ViewSelectWs { long long* offsets; int* sorted; };
ViewSelectWs carve_view_select(Carver& c, int N, long long n_obs) {
  ViewSelectWs w;
  w.offsets = c.take<long long>((size_t)N + 1);
  w.sorted = c.take<int>((size_t)n_obs);
  return w;
}
constexpr int kViewSelectMaxImages = 32768;   // N (N - 1) / 2 workgroups in one grid
bool view_select_sizes_ok(int N, long long n_obs) { return N >= 1 && N <= kViewSelectMaxImages && n_obs >= 0 && n_obs < (1ll << 31); }
}  // namespace

extern "C" {

int ufr_image_resize_u8(const uint8_t* src, int32_t n, int32_t Hs, int32_t Ws, int32_t H, int32_t W, const int32_t* clip4, float* dst,
                        ufr_stream stream) {
  return image_resize("ufr_image_resize_u8", "image_resize_u8", src, nullptr, false, n, Hs, Ws, H, W, clip4, dst, stream);
}

int ufr_image_resize_mask_u8(const uint8_t* src, const uint8_t* mask, int32_t n, int32_t Hs, int32_t Ws, int32_t H, int32_t W,
                             const int32_t* clip4, float* dst, ufr_stream stream) {
  return image_resize("ufr_image_resize_mask_u8", "image_resize_mask_u8", src, mask, true, n, Hs, Ws, H, W, clip4, dst, stream);
}

int ufr_image_undistort_u8(const uint8_t* src, int32_t n, int32_t Hs, int32_t Ws, int32_t C, int32_t model, const double* params,
                           const double* k_out, int32_t H, int32_t W, uint8_t* dst, uint8_t* valid, ufr_stream stream) {
  const char* who = "ufr_image_undistort_u8";
  // parameters per COLMAP model id; 0 = not supported (FOV 7, THIN_PRISM_FISHEYE 10)
  static const int kParams[11] = {3, 4, 4, 5, 8, 8, 12, 0, 4, 5, 0};
  UFR_REQUIRE(src && dst && params && k_out, "%s: null argument", who);
  UFR_REQUIRE(n >= 1 && Hs >= 1 && Ws >= 1 && H >= 1 && W >= 1, "%s: n %d, source %dx%d, output %dx%d (each must be >= 1)", who, n, Hs,
              Ws, H, W);
  UFR_REQUIRE(C >= 1 && C <= 4, "%s: C %d (1 .. 4 channels)", who, C);
  UFR_REQUIRE(model >= 0 && model <= 10 && kParams[model] > 0,
              "%s: camera model %d is not supported (COLMAP ids 0 .. 6, 8, 9; FOV 7 and THIN_PRISM_FISHEYE 10 are refused)", who, model);
  for (int k = 0; k < kParams[model]; ++k)
    UFR_REQUIRE(std::isfinite(params[k]), "%s: parameter %d of camera model %d is not finite (%g)", who, k, model, params[k]);
  for (int k = 0; k < 4; ++k) UFR_REQUIRE(std::isfinite(k_out[k]), "%s: k_out[%d] is not finite (%g)", who, k, k_out[k]);
  UFR_REQUIRE(k_out[0] > 0.0 && k_out[1] > 0.0, "%s: output focal lengths %g %g (each must be > 0)", who, k_out[0], k_out[1]);
  UFR_REQUIRE((long long)Hs * Ws < (1ll << 31) && (long long)H * W < (1ll << 31), "%s: an image of %dx%d or %dx%d has 2^31 pixels or more",
              who, Hs, Ws, H, W);
  hipStream_t s = static_cast<hipStream_t>(stream);
  UFR_TIMED("image_undistort_u8", s, launch_image_undistort(src, n, Hs, Ws, C, model, params, k_out, H, W, dst, valid, s));
  return UFR_OK;
}

// ------------------------------------------------------------------ view selection of a COLMAP model
size_t ufr_view_pair_scores_workspace_bytes(int32_t N, int64_t n_obs) {
  if (!view_select_sizes_ok(N, n_obs)) {
    fail(UFR_ERR_ARG, "ufr_view_pair_scores_workspace_bytes: N %d, n_obs %lld (1 <= N <= %d, 0 <= n_obs < 2^31)", N, (long long)n_obs,
         kViewSelectMaxImages);
    return 0;
  }
  return carved_bytes(carve_view_select, (int)N, (long long)n_obs);
}

int ufr_view_pair_scores(const int64_t* offsets, const int32_t* obs, const int32_t* obs_host, int64_t n_obs, const double* points,
                         int64_t M, const double* centres, int32_t N, double theta0, double sigma1, double sigma2, double* score,
                         void* workspace, size_t workspace_bytes, ufr_stream stream) {
  const char* who = "ufr_view_pair_scores";
  UFR_REQUIRE(offsets && centres && score && workspace && (obs || n_obs == 0) && (points || M == 0), "%s: null argument", who);
  UFR_REQUIRE(view_select_sizes_ok(N, n_obs), "%s: N %d, n_obs %lld (1 <= N <= %d, 0 <= n_obs < 2^31)", who, N, (long long)n_obs,
              kViewSelectMaxImages);
  UFR_REQUIRE(M >= 0 && M < (1ll << 31), "%s: M %lld (0 <= M < 2^31)", who, (long long)M);
  UFR_REQUIRE(offsets[0] == 0 && offsets[N] == n_obs, "%s: offsets run from %lld to %lld, the lists hold %lld indices", who,
              (long long)offsets[0], (long long)offsets[N], (long long)n_obs);
  for (int i = 0; i < N; ++i)
    UFR_REQUIRE(offsets[i] <= offsets[i + 1], "%s: offsets are not monotone at image %d (%lld > %lld)", who, i, (long long)offsets[i],
                (long long)offsets[i + 1]);
  if (obs_host)
    for (long long o = 0; o < n_obs; ++o)
      UFR_REQUIRE(obs_host[o] >= -1 && obs_host[o] < M, "%s: observation %lld holds index %d, outside [-1, %lld)", who, o, obs_host[o],
                  (long long)M);
  UFR_REQUIRE(sigma1 > 0.0 && sigma2 > 0.0 && std::isfinite(sigma1) && std::isfinite(sigma2) && std::isfinite(theta0),
              "%s: theta0 %g, sigma1 %g, sigma2 %g (sigma > 0, all finite)", who, theta0, sigma1, sigma2);
  Carver c(workspace);
  const ViewSelectWs w = carve_view_select(c, N, n_obs);
  UFR_REQUIRE(workspace_bytes >= c.off, "%s: workspace too small: %zu < %zu bytes", who, workspace_bytes, c.off);
  hipStream_t s = static_cast<hipStream_t>(stream);
  UFR_TIMED("view_pair_scores", s, launch_view_pair_scores(reinterpret_cast<const long long*>(offsets), obs, points, M, centres, N, theta0,
                                                           sigma1, sigma2, score, w.offsets, w.sorted, s));
  return UFR_OK;
}

int ufr_pixel_rays(const float* m_inv, const float* origin, int32_t H, int32_t W, float* dir, ufr_stream stream) {
  const char* who = "ufr_pixel_rays";
  UFR_REQUIRE(m_inv && dir, "%s: null argument", who);
  UFR_REQUIRE(H >= 2 && W >= 2, "%s: image %dx%d (H and W must be >= 2: the pixel grid divides by H - 1 and W - 1)", who, H, W);
  UFR_REQUIRE((long long)H * W < (1ll << 31), "%s: image %dx%d has 2^31 pixels or more", who, H, W);
  hipStream_t s = static_cast<hipStream_t>(stream);
  UFR_TIMED("pixel_rays", s, launch_pixel_rays(m_inv, origin, H, W, dir, s));
  return UFR_OK;
}

}  // extern "C"
