// extern "C" surface of libufr.so (include/ufr.h): the forward ray path -- its per-op entry points and the
// whole-path two-pass renderer with its side streams.
#include "api_common.h"

using namespace ufr;
using namespace ufr::api;

namespace {
__global__ void order_pe_kernel(float* __restrict__ table, int SN) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= SN * 8) return;
  int pos = i >> 3, jj = i & 7;
  // ray_transformer.py:165-173: float64 table pos / 10000^(2*(j//2)/8), sin on even / cos on odd dims
  double ang = (double)pos / pow(10000.0, 2.0 * (double)(jj / 2) / 8.0);
  table[i] = (float)((jj & 1) ? cos(ang) : sin(ang));
}
}  // namespace

namespace ufr {
hipError_t launch_order_pe(float* table, int SN, hipStream_t s) {
  hipLaunchKernelGGL(order_pe_kernel, dim3((SN * 8 + 255) / 256), dim3(256), 0, s, table, SN);
  return hipGetLastError();
}
}  // namespace ufr

namespace {
// [token0 | order code]: ops.aggregate(keep_workspace=True) reads token0 at the head
struct AggregateWs { float *token0, *order_pe; };
AggregateWs carve_aggregate(Carver& c, int RN, int SN) {
  AggregateWs w;
  w.token0 = c.f32((size_t)RN * SN * UFR_TOKEN_DIM);
  w.order_pe = c.f32((size_t)SN * 8);
  return w;
}

int aggregate_impl(const void* packed, const float* x_tokens, const float* x_point, const float* rgb, const float* dir, int RN, int SN,
                   int NV, float* radiance, float* srdf, float* token0, float* order_pe, bool pe_ready,
                   float* view_out, float* ray_out, bool lowp, int* status, hipStream_t s) {
  UFR_REQUIRE((unsigned long long)RN * SN * (NV + 1) * UFR_TOKEN_DIM < (1ull << 30),
              "view transformer: %d x %d points x %d tokens exceed the 2^30 token values one call addresses; chunk the points", RN, SN, NV + 1);
  UFR_TIMED("view_transformer", s, launch_view_transformer(static_cast<const float*>(packed), x_tokens, x_point, rgb, dir, RN * SN, NV,
      token0, radiance, view_out, lowp, status, s));
  if (!pe_ready) UFR_HIP(launch_order_pe(order_pe, SN, s));
  UFR_TIMED("ray_transformer", s, launch_ray_transformer(static_cast<const float*>(packed), token0, nullptr, order_pe, RN, SN, srdf,
      ray_out, lowp, status, s));
  return UFR_OK;
}
}  // namespace

extern "C" {

// ------------------------------------------------------------------ per-op entry points
int ufr_sample_fixed(const float* near, const float* far, const float* U, float* z_out, int32_t RN, int32_t SN,
                     ufr_stream stream) {
  UFR_REQUIRE(near && far && U && z_out, "ufr_sample_fixed: null argument");
  UFR_REQUIRE(RN > 0 && SN >= 2, "ufr_sample_fixed: RN=%d SN=%d", RN, SN);
  UFR_HIP(launch_sample_fixed(near, far, U, RN, z_out, RN, SN, static_cast<hipStream_t>(stream)));
  return UFR_OK;
}

int ufr_sample_importance_merge(const float* weight, const float* z, const float* U2, float* z_fine, float* z_all,
                                int32_t RN, int32_t SN, int32_t PN, ufr_stream stream) {
  UFR_REQUIRE(weight && z && U2 && z_all, "ufr_sample_importance_merge: null argument");
  UFR_REQUIRE(RN > 0 && SN >= 2 && SN <= 256 && PN >= 1 && PN <= 256, "ufr_sample_importance_merge: RN=%d SN=%d PN=%d", RN, SN, PN);
  UFR_HIP(launch_importance_merge(weight, z, U2, RN, z_fine, z_all, RN, SN, PN, nullptr, nullptr, static_cast<hipStream_t>(stream)));
  return UFR_OK;
}

int ufr_sample_importance_pool(const float* weight, const float* z, const float* U2, float* z_all, float* z_new,
                               int32_t* row, int32_t RN, int32_t SN, int32_t PN, ufr_stream stream) {
  UFR_REQUIRE(weight && z && U2 && z_all && z_new && row, "ufr_sample_importance_pool: null argument");
  UFR_REQUIRE(RN > 0 && SN >= 2 && SN <= 256 && PN >= 1 && PN <= 256, "ufr_sample_importance_pool: RN=%d SN=%d PN=%d", RN, SN, PN);
  UFR_HIP(launch_importance_merge(weight, z, U2, RN, nullptr, z_all, RN, SN, PN, z_new, row, static_cast<hipStream_t>(stream)));
  return UFR_OK;
}

int ufr_points(const float* ray_o, int32_t ray_o_stride, const float* ray_d, const float* z, float* points, int32_t RN,
               int32_t SN, ufr_stream stream) {
  UFR_REQUIRE(ray_o && ray_d && z && points, "ufr_points: null argument");
  UFR_REQUIRE(ray_o_stride == 0 || ray_o_stride == 3, "ufr_points: ray_o_stride must be 0 or 3");
  UFR_HIP(launch_points(ray_o, ray_o_stride, ray_d, z, points, RN, SN, static_cast<hipStream_t>(stream)));
  return UFR_OK;
}

int ufr_project_gather(const ufr_frame* frame, const ufr_raw_weights* raw, const float* ray_o, int32_t ray_o_stride,
                       const float* ray_d, const float* z, int32_t RN, int32_t SN, float* x_tokens, float* rgb,
                       float* dir, float* sim8, float* vol24, float* xy, float* mask_z, const float* vol24_in,
                       const float* sim8_in, ufr_stream stream) {
  const FrameDev* f = frame_of(frame);
  UFR_REQUIRE(f, "ufr_project_gather: frame handle not prepared");
  UFR_REQUIRE(raw && ray_o && ray_d && z && x_tokens && rgb && dir, "ufr_project_gather: null argument");
  UFR_REQUIRE(ray_o_stride == 0 || ray_o_stride == 3, "ufr_project_gather: ray_o_stride must be 0 or 3");
  UFR_REQUIRE(RN > 0 && SN > 0, "ufr_project_gather: RN=%d SN=%d", RN, SN);
  UFR_REQUIRE(f->match || sim8_in, "ufr_project_gather: the frame has no matching features: sim8_in is required");
  UFR_REQUIRE(f->vol[0] || vol24_in, "ufr_project_gather: the frame has no volumes: vol24_in is required");
  UFR_TIMED("gather", static_cast<hipStream_t>(stream), launch_gather(*f, presim_of(raw), ray_o, ray_o_stride, ray_d, z, RN, SN, x_tokens,
      nullptr, rgb, dir, sim8, vol24, xy, mask_z, vol24_in, sim8_in, static_cast<hipStream_t>(stream)));
  return UFR_OK;
}

size_t ufr_aggregate_workspace_bytes(int32_t RN, int32_t SN, int32_t /*NV*/) {
  return carved_bytes(carve_aggregate, RN, SN);
}

int ufr_aggregate(const void* packed_weights, const float* x_tokens, const float* rgb, const float* dir, int32_t RN,
                  int32_t SN, int32_t NV, float* radiance, float* srdf, void* workspace, float* view_out,
                  float* ray_out, int32_t precision, ufr_stream stream) {
  UFR_REQUIRE(packed_weights && x_tokens && rgb && dir && radiance && srdf && workspace, "ufr_aggregate: null argument");
  UFR_CHECK(check_views("ufr_aggregate", NV));
  UFR_CHECK(check_ray_samples("ufr_aggregate", RN, SN));
  UFR_PRECISION(precision, lowp, "ufr_aggregate");
  hipStream_t s = static_cast<hipStream_t>(stream);
  UFR_STATUS_ENTER(sl, s, "ufr_aggregate");
  Carver c(workspace);
  const AggregateWs w = carve_aggregate(c, RN, SN);
  UFR_CHECK(aggregate_impl(packed_weights, x_tokens, nullptr, rgb, dir, RN, SN, NV, radiance, srdf, w.token0, w.order_pe, false,
                           view_out, ray_out, lowp, status_word(sl), s));
  return status_leave(sl, s);
}

int ufr_composite(const float* z, const float* radiance, const int32_t* row, const float* srdf, const float* variance,
                  int32_t RN, int32_t SN, float* rgb, float* depth, float* opacity, float* weight, ufr_stream stream) {
  UFR_REQUIRE(z && radiance && srdf && variance && depth, "ufr_composite: null argument");
  UFR_REQUIRE(RN > 0 && SN >= 2 && SN <= 256, "ufr_composite: SN=%d out of range [2,256]", SN);
  UFR_TIMED("composite", static_cast<hipStream_t>(stream), launch_composite(z, radiance, row, srdf, variance, RN, SN, rgb, depth, opacity,
      weight, nullptr, nullptr, static_cast<hipStream_t>(stream)));
  return UFR_OK;
}

// ------------------------------------------------------------------ halves of aggregate
int ufr_view_transform(const void* packed_weights, const float* x_tokens, const float* rgb, const float* dir, int32_t P,
                       int32_t NV, float* token0, float* radiance, int32_t precision, ufr_stream stream) {
  UFR_REQUIRE(packed_weights && x_tokens && rgb && dir && token0 && radiance, "ufr_view_transform: null argument");
  UFR_CHECK(check_views("ufr_view_transform", NV));
  UFR_REQUIRE(P > 0, "ufr_view_transform: P=%d", P);
  UFR_PRECISION(precision, lowp, "ufr_view_transform");
  hipStream_t s = static_cast<hipStream_t>(stream);
  UFR_STATUS_ENTER(sl, s, "ufr_view_transform");
  UFR_REQUIRE((unsigned long long)P * (NV + 1) * UFR_TOKEN_DIM < (1ull << 30),
              "ufr_view_transform: %d points x %d tokens exceed the 2^30 token values one call addresses; chunk the points", P, NV + 1);
  UFR_TIMED("view_transformer", s, launch_view_transformer(static_cast<const float*>(packed_weights), x_tokens, nullptr, rgb, dir, P, NV,
      token0, radiance, nullptr, lowp, status_word(sl), s));
  return status_leave(sl, s);
}

size_t ufr_ray_transform_workspace_bytes(int32_t SN) { return align_up((size_t)(SN > 0 ? SN : 1) * 8 * sizeof(float)); }

int ufr_ray_transform(const void* packed_weights, const float* token0, const int32_t* row, int32_t RN, int32_t SN,
                      float* srdf, void* workspace, int32_t precision, ufr_stream stream) {
  UFR_REQUIRE(packed_weights && token0 && srdf && workspace, "ufr_ray_transform: null argument");
  UFR_CHECK(check_ray_samples("ufr_ray_transform", RN, SN));
  UFR_PRECISION(precision, lowp, "ufr_ray_transform");
  hipStream_t s = static_cast<hipStream_t>(stream);
  UFR_STATUS_ENTER(sl, s, "ufr_ray_transform");
  float* order_pe = static_cast<float*>(workspace);
  UFR_HIP(launch_order_pe(order_pe, SN, s));
  UFR_TIMED("ray_transformer", s, launch_ray_transformer(static_cast<const float*>(packed_weights), token0, row, order_pe, RN, SN, srdf,
      nullptr, lowp, status_word(sl), s));
  return status_leave(sl, s);
}

// ------------------------------------------------------------------ whole-path inference
int32_t ufr_default_chunk_rays(void) { return 4096; }

}  // extern "C"

namespace {
struct RenderWs {
  float *ray_o, *rd, *near, *far, *camz, *z1, *w1, *srdf1, *depth1, *rgb1, *z2, *srdf2, *rad, *x, *xp, *rgbm, *dir, *token0,
      *pe1, *pe2, *z_new;
  int* row;  // merged slot -> row of the [coarse | new] evaluation pool (token0, rad)
  size_t bytes;
};
RenderWs carve_render(void* ws, int R, int SN, int PN, int NV) {
  // Smax: samples per ray in the evaluation pool (coarse + new); Sg: points per ray one gather / view-transformer
  // launch handles (the fine pass evaluates only its PN new points)
  const size_t S2 = (size_t)SN + PN, Smax = S2 > (size_t)SN ? S2 : SN, Sg = (size_t)(SN > PN ? SN : PN);
  Carver c(ws);
  RenderWs r;
  r.ray_o = c.f32(4);
  r.rd = c.f32((size_t)R * 3);
  r.near = c.f32(R);
  r.far = c.f32(R);
  r.camz = c.f32(R);
  r.z1 = c.f32((size_t)R * SN);
  r.w1 = c.f32((size_t)R * SN);
  r.srdf1 = c.f32((size_t)R * SN);
  r.depth1 = c.f32(R);
  r.rgb1 = c.f32((size_t)R * 3);
  r.z2 = c.f32((size_t)R * S2);
  r.srdf2 = c.f32((size_t)R * S2);
  r.rad = c.f32((size_t)R * Smax * 3);
  r.x = c.f32((size_t)R * Sg * NV * kViewCols);   // compact token layout (ufr_internal.h): per-view columns ...
  r.xp = c.f32((size_t)R * Sg * kPointCols);      // ... and the per-point ones, once
  r.rgbm = c.f32((size_t)R * Sg * NV * 4);
  r.dir = c.f32((size_t)R * Sg * NV * 4);
  r.z_new = c.f32((size_t)R * (PN > 0 ? PN : 1));
  r.row = c.take<int>((size_t)R * S2);
  r.token0 = c.f32((size_t)R * Smax * UFR_TOKEN_DIM);
  r.pe1 = c.f32((size_t)SN * 8);
  r.pe2 = c.f32(S2 * 8);
  r.bytes = c.off;
  return r;
}

// Side streams: consecutive ray chunks are independent, so they are issued round-robin on a few
// library-owned HIP streams -- the gather kernel of one chunk (L2/latency-bound, no MFMA) then runs
// beside the transformer kernels of another (MFMA-bound) instead of in front of them.
constexpr int kMaxLanes = 4;
struct SidePool {
  hipStream_t s[kMaxLanes] = {};
  hipEvent_t fork = nullptr, join[kMaxLanes] = {};
  int n = 0;
};
thread_local SidePool g_side_by_device[kMaxDevices];   // streams and events belong to the device they were created on

int side_pool_get(int n, SidePool** out) {
  int dev = 0;
  UFR_HIP(hipGetDevice(&dev));
  UFR_REQUIRE(dev >= 0 && dev < kMaxDevices, "side streams: device %d out of range", dev);
  SidePool& p = g_side_by_device[dev];
  if (!p.fork) UFR_HIP(hipEventCreateWithFlags(&p.fork, hipEventDisableTiming));
  for (; p.n < n; ++p.n) {
    // the ray path's chunks at the device's HIGHEST stream priority: whatever the caller runs beside a frame (the next
    // frame's producers on a default- or low-priority stream, uforecon_amd/evalset.py) then fills the gaps the ray kernels
    // leave instead of taking turns with them
    int least = 0, greatest = 0;
    UFR_HIP(hipDeviceGetStreamPriorityRange(&least, &greatest));
    // (measured round 6, configs[2] on one GPU, 24 frames, two runs each: 137.5 / 139.4 ms per frame with the overlap,
    // 145.4 / 143.8 without it.  The A/B's "flat priorities" leg, 140.5 / 140.6, changed no priority -- the variables it
    // set were read nowhere -- so it ran this same configuration again: what the priorities themselves buy is unmeasured)
    UFR_HIP(hipStreamCreateWithPriority(&p.s[p.n], hipStreamNonBlocking, greatest));
    UFR_HIP(hipEventCreateWithFlags(&p.join[p.n], hipEventDisableTiming));
  }
  *out = &p;
  return UFR_OK;
}

// where the coarse compositor's colour and depth go: the workspace (ufr_render_rays drops them) or the caller's
// buffers (ufr_render_rays_pair)
struct CoarseOut { float *rgb, *depth; };

// one chunk of R rays starting at r0, entirely on stream s with workspace w
int render_chunk(const ufr_render_args* a, const FrameDev* f, const RenderWs& w, bool& pe_ready, int r0, int R, bool lowp,
                 int* status, CoarseOut co, hipStream_t s) {
  const int RN = a->RN, SN = a->SN, PN = a->coarse_only ? 0 : a->PN, NV = f->NV;
  const PreSim ps = presim_of(a->raw);
  const int S2 = SN + PN, HW = f->H * f->W;
  {
    ProfScope p("sampler", s);
    UFR_HIP(launch_ray_setup(a->ray_idx + r0, a->ray_d, a->cam_ray_d, HW, a->near_z, a->far_z, R, w.rd, w.near, w.far,
                             w.camz, a->ray_o, w.ray_o, s));
    UFR_HIP(launch_sample_fixed(w.near, w.far, a->U1 + r0, RN, w.z1, R, SN, s));
    if (!pe_ready) {
      UFR_HIP(launch_order_pe(w.pe1, SN, s));
      if (!a->coarse_only) UFR_HIP(launch_order_pe(w.pe2, S2, s));
      pe_ready = true;
    }
  }
  // ---- coarse pass (model.py:445)
  UFR_TIMED("gather", s, launch_gather(*f, ps, w.ray_o, 0, w.rd, w.z1, R, SN, w.x, w.xp, w.rgbm, w.dir, nullptr, nullptr, nullptr,
      nullptr, nullptr, nullptr, s));
  UFR_CHECK(aggregate_impl(a->packed_weights, w.x, w.xp, w.rgbm, w.dir, R, SN, NV, w.rad, w.srdf1, w.token0, w.pe1, true,
                           nullptr, nullptr, lowp, status, s));
  const bool last = a->coarse_only != 0;
  UFR_TIMED("composite", s, launch_composite(w.z1, w.rad, nullptr, w.srdf1, a->raw->variance, R, SN,
      last ? a->rgb + 3 * (size_t)r0 : co.rgb ? co.rgb + 3 * (size_t)r0 : w.rgb1,
      last ? a->depth + r0 : co.depth ? co.depth + r0 : w.depth1, nullptr, w.w1, w.camz,
      (last && a->depth_z) ? a->depth_z + r0 : nullptr, s));
  if (last) {
    if (a->srdf) UFR_HIP(hipMemcpyAsync(a->srdf + (size_t)r0 * SN, w.srdf1, (size_t)R * SN * 4, hipMemcpyDeviceToDevice, s));
    if (a->z_all) UFR_HIP(hipMemcpyAsync(a->z_all + (size_t)r0 * SN, w.z1, (size_t)R * SN * 4, hipMemcpyDeviceToDevice, s));
    return UFR_OK;
  }
  // ---- importance sampling + merge (model.py:455-470), fine pass (model.py:472).  The reference re-evaluates
  // all SN+PN merged samples; a sample's gathers and view-transformer output depend on its own position only,
  // so the SN coarse evaluations (token0, radiance: rows [0, R*SN) of the pool) are kept and only the PN new
  // points go through gather + view transformer (rows [R*SN, R*(SN+PN))).  The ray transformer and the
  // compositor, which do couple the samples of a ray, run over all SN+PN through the slot -> row table.
  UFR_TIMED("sampler", s, launch_importance_merge(w.w1, w.z1, a->U2 + r0, RN, nullptr, w.z2, R, SN, PN, w.z_new, w.row, s));
  UFR_TIMED("gather", s, launch_gather(*f, ps, w.ray_o, 0, w.rd, w.z_new, R, PN, w.x, w.xp, w.rgbm, w.dir, nullptr, nullptr, nullptr,
      nullptr, nullptr, nullptr, s));
  UFR_TIMED("view_transformer", s, launch_view_transformer(static_cast<const float*>(a->packed_weights), w.x, w.xp, w.rgbm, w.dir, R * PN,
      NV, w.token0 + (size_t)R * SN * UFR_TOKEN_DIM, w.rad + (size_t)R * SN * 3, nullptr, lowp, status, s));
  UFR_TIMED("ray_transformer", s, launch_ray_transformer(static_cast<const float*>(a->packed_weights), w.token0, w.row, w.pe2, R, S2,
      w.srdf2, nullptr, lowp, status, s));
  UFR_TIMED("composite", s, launch_composite(w.z2, w.rad, w.row, w.srdf2, a->raw->variance, R, S2, a->rgb + 3 * (size_t)r0, a->depth + r0,
      nullptr, nullptr, w.camz, a->depth_z ? a->depth_z + r0 : nullptr, s));
  if (a->srdf) UFR_HIP(hipMemcpyAsync(a->srdf + (size_t)r0 * S2, w.srdf2, (size_t)R * S2 * 4, hipMemcpyDeviceToDevice, s));
  if (a->z_all) UFR_HIP(hipMemcpyAsync(a->z_all + (size_t)r0 * S2, w.z2, (size_t)R * S2 * 4, hipMemcpyDeviceToDevice, s));
  return UFR_OK;
}
}  // namespace

extern "C" {

size_t ufr_render_workspace_bytes(int32_t chunk_rays, int32_t SN, int32_t PN, int32_t NV) {
  if (chunk_rays <= 0) chunk_rays = ufr_default_chunk_rays();
  return carve_render(nullptr, chunk_rays, SN, PN, NV).bytes;
}

}  // extern "C"

namespace {
int render_impl(const ufr_render_args* a, CoarseOut co, ufr_stream stream) {
  const FrameDev* f = frame_of(a->frame);
  UFR_REQUIRE(f, "ufr_render_rays: frame handle not prepared");
  UFR_REQUIRE(f->match && f->vol[0], "ufr_render_rays: the frame was prepared without matching features / volumes");
  UFR_REQUIRE(a->packed_weights && a->raw && a->ray_idx && a->ray_d && a->U1 && a->depth && a->rgb && a->workspace,
              "ufr_render_rays: null argument");
  UFR_REQUIRE(a->coarse_only || a->U2, "ufr_render_rays: U2 required unless coarse_only");
  const int RN = a->RN, SN = a->SN, PN = a->coarse_only ? 0 : a->PN, NV = f->NV;
  UFR_REQUIRE(RN > 0, "ufr_render_rays: RN=%d", RN);
  UFR_CHECK(check_ray_samples("ufr_render_rays", RN, SN));
  UFR_REQUIRE(a->coarse_only || (PN >= 16 && (SN + PN) % 16 == 0 && SN + PN <= 256 && PN <= 256),
              "ufr_render_rays: fine samples %d unsupported", PN);
  const int chunk = a->chunk_rays > 0 ? a->chunk_rays : ufr_default_chunk_rays();
  // the transformer kernels address a launch's buffers with 32-bit offsets: validate the caller's chunk size up front, not
  // after the gather and earlier chunks were enqueued (the default 4096 rays is 160 x below the limit)
  UFR_REQUIRE((unsigned long long)chunk * (SN > PN ? SN : PN) * (NV + 1) * UFR_TOKEN_DIM < (1ull << 30),
              "ufr_render_rays: chunk_rays=%d x %d samples x %d tokens exceeds the 2^30 token values one launch addresses; use a "
              "smaller chunk", chunk, SN > PN ? SN : PN, NV + 1);
  const size_t need = ufr_render_workspace_bytes(chunk, SN, PN, NV);
  UFR_CHECK(check_workspace("ufr_render_rays", a->workspace_bytes, need));
  UFR_PRECISION(a->precision, lowp, "ufr_render_rays");
  hipStream_t s = static_cast<hipStream_t>(stream);
  UFR_STATUS_ENTER(sl, s, "ufr_render_rays");
  // the planes' activation exponents follow THIS frame's measured feature bound (a no-op kernel unless the frame exceeds
  // what the table serves; ufr_weights_fit_frame) -- on the caller's stream, in front of the fork to the side streams
  UFR_HIP(launch_refit_weights(static_cast<float*>(const_cast<void*>(a->packed_weights)), f->abs_max, status_word(sl), s));
  int lanes = a->n_streams > 1 ? a->n_streams : 1;
  if (lanes > kMaxLanes) lanes = kMaxLanes;
  if ((size_t)lanes * need > a->workspace_bytes) lanes = (int)(a->workspace_bytes / need);  // one workspace per lane
  // a small ray set (one rank's tile of a frame split over 8 GPUs) is cut finer so that every side stream still
  // gets >= 4 chunks: the last round of a round-robin over few chunks otherwise leaves streams idle
  int eff_chunk = chunk;
  if (lanes > 1) {
    // ... in multiples of 2048 rays: 512 resident workgroup slots x 4 rays fill whole rounds of the ray transformer
    int target = (RN + 4 * lanes - 1) / (4 * lanes) / 2048 * 2048;
    if (target < 2048) target = 2048;
    if (target < eff_chunk) eff_chunk = target;
  }
  const int n_chunks = (RN + eff_chunk - 1) / eff_chunk;
  if (lanes > n_chunks) lanes = n_chunks;

  if (lanes <= 1) {
    RenderWs w = carve_render(a->workspace, chunk, SN, PN, NV);
    bool pe_ready = false;
    for (int r0 = 0; r0 < RN; r0 += eff_chunk)
      UFR_CHECK(render_chunk(a, f, w, pe_ready, r0, (RN - r0) < eff_chunk ? (RN - r0) : eff_chunk, lowp, status_word(sl), co, s));
    return status_leave(sl, s);
  }
  SidePool* side = nullptr;
  UFR_CHECK(side_pool_get(lanes, &side));
  UFR_HIP(hipEventRecord(side->fork, s));
  RenderWs w[kMaxLanes];
  bool pe_ready[kMaxLanes] = {};
  for (int l = 0; l < lanes; ++l) {
    w[l] = carve_render(static_cast<char*>(a->workspace) + (size_t)l * need, chunk, SN, PN, NV);
    UFR_HIP(hipStreamWaitEvent(side->s[l], side->fork, 0));
  }
  int rc = UFR_OK;
  for (int c = 0; c < n_chunks && rc == UFR_OK; ++c) {
    const int l = c % lanes, r0 = c * eff_chunk;
    rc = render_chunk(a, f, w[l], pe_ready[l], r0, (RN - r0) < eff_chunk ? (RN - r0) : eff_chunk, lowp, status_word(sl), co, side->s[l]);
  }
  // join even when a chunk failed: the caller's stream must not run ahead of (and its allocator must not recycle the
  // workspace under) side-stream kernels that were already enqueued
  for (int l = 0; l < lanes; ++l) {
    hipError_t e = hipEventRecord(side->join[l], side->s[l]);
    if (e == hipSuccess) e = hipStreamWaitEvent(s, side->join[l], 0);
    if (e != hipSuccess) hipStreamSynchronize(side->s[l]);
  }
  return rc != UFR_OK ? rc : status_leave(sl, s);
}
}  // namespace

extern "C" {

int ufr_render_rays(const ufr_render_args* a, ufr_stream stream) {
  UFR_REQUIRE(a, "ufr_render_rays: null args");
  return render_impl(a, CoarseOut{nullptr, nullptr}, stream);
}

int ufr_render_rays_pair(const ufr_render_args* a, float* rgb_coarse, float* depth_coarse, ufr_stream stream) {
  UFR_REQUIRE(a, "ufr_render_rays_pair: null args");
  UFR_REQUIRE(rgb_coarse && depth_coarse, "ufr_render_rays_pair: null coarse output");
  UFR_REQUIRE(!a->coarse_only, "ufr_render_rays_pair: coarse_only renders one pass; call ufr_render_rays");
  UFR_REQUIRE(a->cam_ray_d || !a->depth_z, "ufr_render_rays_pair: depth_z needs cam_ray_d (without it near/far are ray lengths already)");
  return render_impl(a, CoarseOut{rgb_coarse, depth_coarse}, stream);
}

}  // extern "C"
