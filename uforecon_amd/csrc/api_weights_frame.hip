// extern "C" surface of libufr.so (include/ufr.h): the packed-weight blob (sizes, pack plans, packing) and
// the preparation of a frame.
#include "api_common.h"
#include "ufr_layout_f16.h"

using namespace ufr;
using namespace ufr::api;

namespace {

int frame_check(const ufr_frame_desc* d) {
  UFR_REQUIRE(d, "frame desc is null");
  UFR_CHECK(check_views("frame desc", d->NV));
  UFR_REQUIRE(d->H >= 8 && d->W >= 8 && d->H % 4 == 0 && d->W % 4 == 0, "H,W must be multiples of 4 (got %dx%d)",
              d->H, d->W);
  UFR_REQUIRE(d->source_imgs && d->depth_info && d->feat, "null frame tensor");
  UFR_REQUIRE((long long)d->H * d->W < (1 << 24) && (long long)(d->H / 4) * (d->W / 4) * 32 * (d->NV - 1) < (1ll << 32),
              "image of %dx%d is too large for the gather's 24-bit texel indices", d->H, d->W);
  // the gathers read through raw buffer descriptors whose masked taps are sent to offset 0x80000000 (kBufOut) and rely on
  // that offset lying OUTSIDE the buffer: every descriptor must stay below 2^31 bytes (gather.hip:236-288, 358)
  {
    const long long px = (long long)d->H * d->W, mpx = (long long)(d->H / 4) * (d->W / 4), lim = 1ll << 31;
    UFR_REQUIRE(px * 16 < lim && d->NV * mpx * 128 < lim && d->NV * mpx * 32 * (d->NV - 1) * 4 < lim,
                "frame of %dx%d with %d views: an image / feature-map buffer reaches 2 GiB (the gathers' zero-fill offset)",
                d->H, d->W, d->NV);
  }
  // match / volumes may be absent: such a frame only serves ufr_project_gather calls that pass sim8_in / vol24_in
  const bool has_vol = d->vol_feat[0] != nullptr;
  for (int s = 0; s < UFR_NUM_STAGES; ++s) {
    UFR_REQUIRE((d->vol_feat[s] != nullptr) == has_vol && (d->vol_weight[s] != nullptr) == has_vol,
                "volumes must be given for all stages or for none (stage %d)", s + 1);
    if (has_vol) UFR_REQUIRE(d->vol_D[s] >= 2 && d->vol_H[s] >= 2 && d->vol_W[s] >= 2, "degenerate volume (stage %d)", s + 1);
    // the gathers index texels with 24-bit multiplies and 32-bit float offsets inside one view
    if (has_vol)
      UFR_REQUIRE((long long)d->vol_D[s] * d->vol_H[s] < (1 << 24) && (long long)d->vol_W[s] * kVolCh < (1 << 24) &&
                      (long long)d->vol_D[s] * d->vol_H[s] * d->vol_W[s] * kVolCh * 4 < (1ll << 31),
                  "volume of stage %d is too large for the gather's 31-bit byte offsets (per view: < 2 GiB)", s + 1);
  }
  UFR_REQUIRE(d->source_poses && d->source_cam_pos && d->ref_cam_pos && d->w2c_row2, "null camera constants");
  return UFR_OK;
}

// [feat | match (if given) | rgb | volumes of the stages (if given) | measured feature bound]
struct FrameWs { float *feat, *match, *rgb, *vol[UFR_NUM_STAGES]; unsigned* abs_max; };
FrameWs carve_frame(Carver& c, const ufr_frame_desc* d) {
  const size_t NV = d->NV, hw = (size_t)(d->H / 4) * (d->W / 4);
  FrameWs w = {};
  w.feat = c.f32(NV * hw * 32);
  if (d->match) w.match = c.f32(NV * hw * 32 * (NV - 1));
  w.rgb = c.f32(NV * d->H * d->W * 4);
  if (d->vol_feat[0])
    for (int s = 0; s < UFR_NUM_STAGES; ++s) w.vol[s] = c.f32(NV * d->vol_D[s] * d->vol_H[s] * d->vol_W[s] * kVolCh);
  w.abs_max = c.take<unsigned>(64);   // one word; its own 256 bytes
  return w;
}

}  // namespace

extern "C" {

// ------------------------------------------------------------------ weights
// [fp32 region | fp16 plane region (forward) | bf16 plane region (backward data-gradient chains) | 16-byte tail (reserved)]
size_t ufr_packed_weights_bytes(void) { return (size_t)blob_floats() * sizeof(float) + (size_t)kF16Bytes + (size_t)kBwdBytes + 16; }
size_t ufr_packed_bwd_halfwords(void) { return (size_t)kBwdHalfwords; }
size_t ufr_packed_fp32_floats(void) { return (size_t)blob_floats(); }
size_t ufr_packed_f16_halfwords(void) { return (size_t)kF16Halfwords; }
size_t ufr_packed_scale_table_offset(void) { return (size_t)scale_table_offset(); }
int ufr_packed_scale_table_entries(void) { return M_COUNT; }

int ufr_pack_plan_f16(int32_t* param_id, int32_t* elem, int32_t* plane) {
  UFR_REQUIRE(param_id && elem && plane, "ufr_pack_plan_f16: null output");
  for (int h = 0; h < kF16Halfwords; ++h) plan_entry_f16(h, &param_id[h], &elem[h], &plane[h]);
  return UFR_OK;
}

int ufr_pack_plan_bwd(int32_t* param_id, int32_t* elem, int32_t* plane) {
  UFR_REQUIRE(param_id && elem && plane, "ufr_pack_plan_bwd: null output");
  for (int h = 0; h < kBwdHalfwords; ++h) plan_entry_f16(kF16Halfwords + h, &param_id[h], &elem[h], &plane[h]);
  return UFR_OK;
}

int ufr_pack_plan(int32_t* param_id, int32_t* elem) {
  UFR_REQUIRE(param_id && elem, "ufr_pack_plan: null output");
  for (int i = 0; i < blob_floats(); ++i) {
    int p, e;
    plan_entry(i, &p, &e);
    param_id[i] = p;
    elem[i] = e;
  }
  return UFR_OK;
}

int ufr_weights_pack_for(const ufr_raw_weights* raw, void* packed, float input_abs_max, ufr_stream stream) {
  UFR_REQUIRE(raw && packed, "ufr_weights_pack: null argument");
  static_assert(sizeof(ufr_raw_weights) == sizeof(RawPtrs), "ufr_raw_weights must be P_COUNT pointers");
  RawPtrs rp;
  memcpy(&rp, raw, sizeof(rp));
  for (int i = 0; i < P_COUNT; ++i) UFR_REQUIRE(rp.p[i], "ufr_weights_pack: parameter %d is null", i);
  UFR_REQUIRE(input_abs_max > 0.f && input_abs_max <= 3.0e38f, "ufr_weights_pack_for: input_abs_max=%g must be positive and finite",
              (double)input_abs_max);
  hipStream_t s = static_cast<hipStream_t>(stream);
  UFR_STATUS_SLOT(sl);
  // every exponent of the planes is chosen on the device from the parameters themselves (prep.hip: weight_scale_kernel):
  // any finite weight fits; a non-finite one raises bit 2 of the sticky status (no synchronisation here: training re-packs
  // after every optimizer step)
  UFR_HIP(launch_pack_weights(rp, static_cast<float*>(packed), input_abs_max, status_word(sl), s));
  return status_leave(sl, s);
}

int ufr_weights_fit_frame(void* packed, const ufr_frame* frame, ufr_stream stream) {
  const FrameDev* f = frame_of(frame);
  UFR_REQUIRE(packed && f, "ufr_weights_fit_frame: null weights / frame handle not prepared");
  hipStream_t s = static_cast<hipStream_t>(stream);
  UFR_STATUS_SLOT(sl);
  UFR_HIP(launch_refit_weights(static_cast<float*>(packed), f->abs_max, status_word(sl), s));
  return UFR_OK;
}

int ufr_weights_pack(const ufr_raw_weights* raw, void* packed, ufr_stream stream) {
  return ufr_weights_pack_for(raw, packed, kDefaultInputAbsMax, stream);
}

// ------------------------------------------------------------------ frame
size_t ufr_frame_workspace_bytes(const ufr_frame_desc* d) {
  if (frame_check(d) != UFR_OK) return 0;
  return carved_bytes(carve_frame, d);
}

int ufr_frame_prepare(const ufr_frame_desc* d, void* workspace, size_t workspace_bytes, ufr_frame* out,
                      ufr_stream stream) {
  UFR_CHECK(frame_check(d));
  UFR_REQUIRE(workspace && out, "ufr_frame_prepare: null workspace/out");
  Carver c(workspace);
  const FrameWs w = carve_frame(c, d);
  UFR_CHECK(check_workspace("ufr_frame_prepare", workspace_bytes, c.off));
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int NV = d->NV, h = d->H / 4, hw = h * (d->W / 4);
  const bool has_vol = d->vol_feat[0] != nullptr;

  // the passes that re-lay the token features out also measure their magnitude (the matching features only enter as cosine
  // similarities, the colours only the blend: neither is a dense-layer input)
  UFR_HIP(hipMemsetAsync(w.abs_max, 0, 256, s));
  UFR_HIP(launch_nchw_to_nhwc(d->feat, w.feat, NV, 32, hw, 32, s, w.abs_max));
  if (w.match) UFR_HIP(launch_nchw_to_nhwc(d->match, w.match, NV, 32 * (NV - 1), hw, 32 * (NV - 1), s));
  UFR_HIP(launch_nchw_to_nhwc(d->source_imgs, w.rgb, NV, 3, d->H * d->W, 4, s));
  if (has_vol)
    for (int st = 0; st < UFR_NUM_STAGES; ++st)
      UFR_HIP(launch_volume_pack(d->vol_feat[st], d->vol_weight[st], w.vol[st], NV, d->vol_D[st] * d->vol_H[st] * d->vol_W[st], s, w.abs_max));

  FrameDev f;
  memset(&f, 0, sizeof(f));
  f.NV = NV; f.H = d->H; f.W = d->W; f.h = h; f.w = d->W / 4; f.match_ch = 32 * (NV - 1);
  f.feat = w.feat; f.match = w.match; f.rgb = w.rgb; f.depth = d->depth_info;
  for (int st = 0; st < UFR_NUM_STAGES; ++st) {
    f.vol[st] = w.vol[st];
    if (has_vol) { f.vD[st] = d->vol_D[st]; f.vH[st] = d->vol_H[st]; f.vW[st] = d->vol_W[st]; }
  }
  for (int v = 0; v < NV; ++v) {
    memcpy(f.pose[v], d->source_poses + 16 * v, 12 * sizeof(float));
    memcpy(f.cam_pos[v], d->source_cam_pos + 3 * v, 3 * sizeof(float));
    memcpy(f.w2c_z[v], d->w2c_row2 + 4 * v, 4 * sizeof(float));
  }
  memcpy(f.ref_pos, d->ref_cam_pos, 3 * sizeof(float));
  f.vol_near = d->vol_near; f.vol_far = d->vol_far;
  f.abs_max = w.abs_max;
  f.magic = kFrameMagic;
  memset(out, 0, sizeof(*out));
  memcpy(out, &f, sizeof(f));
  return UFR_OK;
}

}  // extern "C"
