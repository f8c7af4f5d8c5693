// extern "C" surface of libufr.so (include/ufr.h), meshes: cleaning (mask votes, first hit, face components), rendering,
// colouring, texturing, simplification, smoothing and denoising.  The rounds of the face components and the scans of the simplifier
// synchronise the stream to hand a flag or a count to the host; nothing else here waits.
#include "api_geometry_common.h"

using namespace ufr;
using namespace ufr::api;

namespace {

// what every stage over the sorted corner slots takes: 3F must fit an int32 too
int check_mesh_rows(const char* who, int64_t V, int64_t F) {
  UFR_REQUIRE(V >= 1 && V <= kChMax && F >= 1 && F <= kChMax / 3, "%s: V %lld, F %lld (V must be 1 .. 2^31 - 1, F 1 .. (2^31 - 1) / 3)",
              who, (long long)V, (long long)F);
  return UFR_OK;
}

// step i of a Jacobi loop over two buffers reads `in` and writes `out`: a -> b on the even steps, b -> a on the odd ones
template <class T>
struct PingPong { T *in, *out; };
template <class T>
PingPong<T> ping_pong(int i, T* a, T* b) { return (i & 1) ? PingPong<T>{b, a} : PingPong<T>{a, b}; }

// ---- mesh cleaning
// first hit: [key image uint64 per pixel | big-triangle count int32 | big-triangle list int32 per face]
struct FirstHitWs { unsigned long long* keys; int *big_count, *big_list; };
FirstHitWs carve_first_hit(Carver& c, long long F, long long pixels) {
  FirstHitWs w;
  w.keys = c.take<unsigned long long>((size_t)pixels);
  w.big_count = c.take<int>(1);
  w.big_list = c.take<int>((size_t)F);
  return w;
}

// rendering: [the first hit's workspace | face image int32 per pixel]
struct RasterFramesWs { FirstHitWs hit; int* face_img; };
RasterFramesWs carve_raster_frames(Carver& c, long long F, long long pixels) {
  RasterFramesWs w;
  w.hit = carve_first_hit(c, F, pixels);
  w.face_img = c.take<int>((size_t)pixels);
  return w;
}

// components: [pair faces int32 x2 per edge slot | parent int32 per face | adjacency flag uint8 per face | changed int32]
struct ComponentsWs { int *pair_a, *pair_b, *parent, *changed; unsigned char* has_adj; };
ComponentsWs carve_components(Carver& c, long long F) {
  ComponentsWs w;
  w.pair_a = c.take<int>((size_t)F * 3);
  w.pair_b = c.take<int>((size_t)F * 3);
  w.parent = c.take<int>((size_t)F);
  w.has_adj = c.take<unsigned char>((size_t)F);
  w.changed = c.take<int>(1);
  return w;
}

// ---- mesh colouring and texturing
// [camera table: one MeshColorCam per view]
MeshColorCam* carve_mesh_colors(Carver& c, int n_views) { return c.take<MeshColorCam>((size_t)n_views); }

// the ranges of what the per-view rule takes (ufr_color_vertices and ufr_texture_bake)
int color_rule_check(const char* who, int32_t n_views, int32_t H, int32_t W, double z_min, double depth_tol, double min_cos,
                     int32_t power, int32_t mode) {
  UFR_REQUIRE(n_views >= 1 && n_views <= UFR_MESH_MAX_VIEWS, "%s: n_views %d (must be 1 .. %d)", who, n_views, UFR_MESH_MAX_VIEWS);
  UFR_REQUIRE(H >= 2 && W >= 2, "%s: image %dx%d (H and W must be >= 2)", who, H, W);
  UFR_CHECK(depth_image_check(who, H, W));
  UFR_REQUIRE(z_min >= 0.0 && std::isfinite(z_min), "%s: z_min %g (must be >= 0 and finite)", who, z_min);
  UFR_REQUIRE(depth_tol >= 0.0 && std::isfinite(depth_tol), "%s: depth_tol %g (must be >= 0 and finite)", who, depth_tol);
  UFR_REQUIRE(min_cos >= 0.0 && min_cos <= 1.0, "%s: min_cos %g (must be 0 .. 1)", who, min_cos);
  UFR_REQUIRE(power >= 0 && power <= UFR_MESH_COLOR_MAX_POWER, "%s: power %d (must be 0 .. %d)", who, power, UFR_MESH_COLOR_MAX_POWER);
  UFR_REQUIRE(mode == UFR_MESH_COLOR_MEAN || mode == UFR_MESH_COLOR_BEST, "%s: unknown mode %d", who, mode);
  return UFR_OK;
}

// the host cameras of n_views views as the records the kernels read; every view is checked
int color_cameras(const char* who, const double* k, const double* w2c, const double* centre, int32_t n_views, MeshColorCam* cams) {
  for (int32_t f = 0; f < n_views; ++f) {
    const double *kk = k + 9 * (size_t)f, *m = w2c + 16 * (size_t)f, *cc = centre + 3 * (size_t)f;
    for (int i = 0; i < 9; ++i) UFR_REQUIRE(std::isfinite(kk[i]), "%s: view %d: k is not finite", who, f);
    for (int i = 0; i < 16; ++i) UFR_REQUIRE(std::isfinite(m[i]), "%s: view %d: w2c is not finite", who, f);
    for (int i = 0; i < 3; ++i) UFR_REQUIRE(std::isfinite(cc[i]), "%s: view %d: the camera centre is not finite", who, f);
    const double r3[9] = {m[0], m[1], m[2], m[4], m[5], m[6], m[8], m[9], m[10]};
    double inv[9];
    UFR_REQUIRE(invert3(r3, inv), "%s: view %d: w2c is singular", who, f);
    for (int i = 0; i < 9; ++i) cams[f].k[i] = kk[i], cams[f].r[i] = r3[i];
    for (int i = 0; i < 3; ++i) cams[f].t[i] = m[4 * i + 3], cams[f].c[i] = cc[i];
  }
  return UFR_OK;
}

// The atlas of F faces at patch size S in closed form (include/ufr.h, "mesh texturing"): cells of side S + 3, two faces a cell,
// cols = ceil(sqrt(cells)) in integers.  False when S or F is out of range; the caller compares Ht and Wt with its own.
bool texture_atlas(int64_t F, int32_t S, TextureAtlas* at) {
  if (F < 1 || F > kChMax || S < 1 || S > UFR_TEXTURE_MAX_PATCH) return false;
  const long long cells = ((long long)F + 1) / 2;
  long long cols = (long long)std::sqrt((double)cells);
  while (cols * cols < cells) ++cols;
  while (cols > 1 && (cols - 1) * (cols - 1) >= cells) --cols;
  const long long rows = (cells + cols - 1) / cols, C = S + 3;
  if (cols * C > UFR_TEXTURE_MAX_SIDE || rows * C > UFR_TEXTURE_MAX_SIDE) return false;
  at->S = S, at->cols = (int)cols, at->Wt = (int)(cols * C), at->Ht = (int)(rows * C), at->F = F;
  return true;
}

int texture_atlas_check(const char* who, int64_t F, int32_t S, int32_t Ht, int32_t Wt, TextureAtlas* at) {
  UFR_REQUIRE(S >= 1 && S <= UFR_TEXTURE_MAX_PATCH, "%s: S %d (must be 1 .. %d)", who, S, UFR_TEXTURE_MAX_PATCH);
  UFR_REQUIRE(F >= 1 && F <= kChMax, "%s: F %lld (must be 1 .. 2^31 - 1)", who, (long long)F);
  UFR_REQUIRE(Ht >= 1 && Wt >= 1 && Ht <= UFR_TEXTURE_MAX_SIDE && Wt <= UFR_TEXTURE_MAX_SIDE, "%s: atlas %dx%d (Ht and Wt must be 1 .. %d)",
              who, Wt, Ht, UFR_TEXTURE_MAX_SIDE);
  UFR_REQUIRE(texture_atlas(F, S, at), "%s: %lld faces at S %d need an atlas with a side above %d", who, (long long)F, S,
              UFR_TEXTURE_MAX_SIDE);
  UFR_REQUIRE(at->Ht == Ht && at->Wt == Wt, "%s: atlas %dx%d is not the closed form for F %lld, S %d: %dx%d", who, Wt, Ht, (long long)F, S,
              at->Wt, at->Ht);
  return UFR_OK;
}

// ---- mesh simplification
// every scanning call: one scan workspace over its items
ScanWs carve_simplify(Carver& c, long long n) { return carve_scan(c, (size_t)simplify_blocks(n)); }

int simplify_counts_check(const char* who, int64_t V, int64_t F) {
  UFR_REQUIRE(V >= 1 && V <= kChMax && F >= 1 && F <= kChMax, "%s: V %lld, F %lld (each must be 1 .. 2^31 - 1)", who, (long long)V,
              (long long)F);
  return UFR_OK;
}

// ---- mesh smoothing
// [neighbour pairs int32 (3F,2) | weight pairs fp64 (3F,2), cotangent weights only], both in row order
struct SmoothWs { int* nbr; double* wgt; };
SmoothWs carve_mesh_smooth(Carver& c, long long F, int weights) {
  SmoothWs w;
  w.nbr = c.take<int>((size_t)(6 * F));
  w.wgt = weights == UFR_SMOOTH_COTANGENT ? c.take<double>((size_t)(6 * F)) : nullptr;
  return w;
}

int smooth_check(const char* who, int64_t V, int64_t F, int32_t weights) {
  UFR_CHECK(check_mesh_rows(who, V, F));
  UFR_REQUIRE(weights == UFR_SMOOTH_UNIFORM || weights == UFR_SMOOTH_COTANGENT, "%s: unknown weights %d", who, weights);
  return UFR_OK;
}

// ---- mesh denoising
// [face records fp64 (F,8), two of them: the normal steps ping-pong | rows int32 (3F,4) | the rows' faces int32 (3F)], in row order
struct DenoiseWs { double* rec_a; double* rec_b; int* rows; int* row_face; };
DenoiseWs carve_mesh_denoise(Carver& c, long long F) {
  DenoiseWs w;
  w.rec_a = c.take<double>((size_t)(8 * F));
  w.rec_b = c.take<double>((size_t)(8 * F));
  w.rows = c.take<int>((size_t)(12 * F));
  w.row_face = c.take<int>((size_t)(3 * F));
  return w;
}

// what ufr_raster_frames and ufr_texture_frames share: the checks, the workspace and the two launches a frame.  tex null: the
// colour is the base colour or the vertex colours; given: the texture's (colors and base_color are then null)
int raster_frames(const char* who, const double* verts, const int32_t* faces, int64_t V, int64_t F, const double* normals,
                  const uint8_t* colors, const RasterTexture* tex, const float* k_inv, const float* c2w, int32_t n_frames, int32_t H,
                  int32_t W, const float* base_color, const uint8_t* background, double ambient, uint8_t* image, float* depth,
                  int32_t* face_id, float* normal_map, void* workspace, size_t workspace_bytes, ufr_stream stream) {
  UFR_REQUIRE(verts && faces && k_inv && c2w && image && workspace, "%s: null argument", who);
  UFR_REQUIRE(V >= 1 && V <= kChMax && F >= 1 && F <= kChMax, "%s: V %lld, F %lld (each must be 1 .. 2^31 - 1)", who, (long long)V,
              (long long)F);
  UFR_REQUIRE(n_frames >= 1, "%s: n_frames %d (must be >= 1)", who, n_frames);
  UFR_CHECK(depth_image_check(who, H, W));
  UFR_REQUIRE(ambient >= 0.0 && ambient <= 1.0, "%s: ambient %g (must be 0 .. 1)", who, ambient);
  double base[3];
  unsigned char bg[3];
  UFR_CHECK(frame_colors(who, base_color, background, base, bg));
  Carver c(workspace);
  const RasterFramesWs w = carve_raster_frames(c, F, (long long)H * W);
  UFR_REQUIRE(workspace_bytes >= c.off, "%s: workspace too small: %zu < %zu bytes", who, workspace_bytes, c.off);
  float rot[9], org[3];
  double proj[12];
  for (int32_t i = 0; i < n_frames; ++i) UFR_CHECK(hit_camera(who, k_inv, c2w + 16 * (size_t)i, rot, org, proj));   // all, before any launch
  const size_t px = (size_t)H * W;
  hipStream_t s = static_cast<hipStream_t>(stream);
  for (int32_t i = 0; i < n_frames; ++i) {   // launches only: the cameras travel as kernel arguments, nothing waits for a frame
    UFR_CHECK(hit_camera(who, k_inv, c2w + 16 * (size_t)i, rot, org, proj));
    UFR_TIMED("raster_first_hit", s, launch_first_hit(verts, faces, V, F, k_inv, rot, org, proj, nullptr, H, W, w.hit.keys,
        w.hit.big_count, w.hit.big_list, w.face_img, nullptr, s));
    UFR_TIMED("raster_shade", s, launch_raster_shade(verts, faces, V, F, normals, colors, k_inv, rot, org, proj, base, ambient, bg,
        w.face_img, H, W, image + 3 * px * i, depth ? depth + px * i : nullptr, face_id ? face_id + px * i : nullptr,
        normal_map ? normal_map + 3 * px * i : nullptr, s, tex));
  }
  return UFR_OK;
}

}  // namespace

extern "C" {

// ------------------------------------------------------------------ mesh cleaning
int ufr_mask_half_widths(int32_t k, int32_t* out) {
  UFR_REQUIRE(out, "ufr_mask_half_widths: null argument");
  UFR_REQUIRE(k >= 1 && k <= UFR_MASK_MAX_KERNEL && k % 2 == 1, "ufr_mask_half_widths: k %d (must be odd, 1 .. %d)", k,
              UFR_MASK_MAX_KERNEL);
  const int r = k / 2;
  for (int i = 0; i < k; ++i) {
    const double dy = (double)(i - r), r2 = (double)r * r;
    out[i] = r ? (int32_t)rint((double)r * sqrt((r2 - dy * dy) / r2)) : 0;   // rint: round half to even
  }
  return UFR_OK;
}

int ufr_mask_dilate(const uint8_t* image, int32_t H, int32_t W, int32_t k, int32_t threshold, uint8_t* dilated, uint8_t* mask,
                    ufr_stream stream) {
  const char* who = "ufr_mask_dilate";
  UFR_REQUIRE(image && (dilated || mask), "%s: null argument", who);
  UFR_CHECK(depth_image_check(who, H, W));
  int32_t hw[UFR_MASK_MAX_KERNEL];
  UFR_CHECK(ufr_mask_half_widths(k, hw));
  short hs[UFR_MASK_MAX_KERNEL];
  for (int i = 0; i < k; ++i) hs[i] = (short)hw[i];
  hipStream_t s = static_cast<hipStream_t>(stream);
  UFR_TIMED("mask_dilate", s, launch_mask_dilate(image, H, W, k, hs, threshold, dilated, mask, s));
  return UFR_OK;
}

int ufr_mesh_vertex_votes(const double* verts, int64_t V, const float* P, const uint8_t* masks, int32_t n_views, int32_t H,
                          int32_t W, int32_t* votes, ufr_stream stream) {
  const char* who = "ufr_mesh_vertex_votes";
  UFR_REQUIRE(verts && P && masks && votes, "%s: null argument", who);
  UFR_REQUIRE(V >= 1 && V <= kChMax, "%s: V %lld (must be 1 .. 2^31 - 1)", who, (long long)V);
  UFR_REQUIRE(n_views >= 1 && n_views <= UFR_MESH_MAX_VIEWS, "%s: n_views %d (must be 1 .. %d)", who, n_views, UFR_MESH_MAX_VIEWS);
  UFR_CHECK(depth_image_check(who, H, W));
  UFR_REQUIRE((long long)H * W * n_views < (1ll << 31), "%s: %d masks of %dx%d have 2^31 pixels or more", who, n_views, H, W);
  hipStream_t s = static_cast<hipStream_t>(stream);
  UFR_HIP(hipMemsetAsync(votes, 0, (size_t)V * sizeof(int32_t), s));
  UFR_TIMED("mesh_vertex_votes", s, launch_vertex_votes(verts, V, P, n_views, masks, H, W, votes, s));
  return UFR_OK;
}

size_t ufr_mesh_first_hit_workspace_bytes(int64_t F, int32_t H, int32_t W) {
  if (F < 1 || F > kChMax || H < 1 || W < 1 || (long long)H * W >= (1ll << 31)) return 0;
  return carved_bytes(carve_first_hit, (long long)F, (long long)H * W);
}

int ufr_mesh_first_hit(const double* verts, const int32_t* faces, int64_t V, int64_t F, const float* k_inv, const float* c2w,
                       const uint8_t* mask, int32_t H, int32_t W, int32_t* face_id, uint8_t* face_hit, void* workspace,
                       size_t workspace_bytes, ufr_stream stream) {
  const char* who = "ufr_mesh_first_hit";
  UFR_REQUIRE(verts && faces && k_inv && c2w && mask && face_id && workspace, "%s: null argument", who);
  UFR_REQUIRE(V >= 1 && V <= kChMax && F >= 1 && F <= kChMax, "%s: V %lld, F %lld (each must be 1 .. 2^31 - 1)", who, (long long)V,
              (long long)F);
  UFR_CHECK(depth_image_check(who, H, W));
  Carver c(workspace);
  const FirstHitWs w = carve_first_hit(c, F, (long long)H * W);
  UFR_CHECK(check_workspace(who, workspace_bytes, c.off));
  float rot[9], org[3];
  double proj[12];
  UFR_CHECK(hit_camera(who, k_inv, c2w, rot, org, proj));
  hipStream_t s = static_cast<hipStream_t>(stream);
  UFR_TIMED("mesh_first_hit", s, launch_first_hit(verts, faces, V, F, k_inv, rot, org, proj, mask, H, W, w.keys, w.big_count,
      w.big_list, face_id, face_hit, s));
  return UFR_OK;
}

int ufr_mesh_edge_keys(const int32_t* faces, const int32_t* vertex_id, int64_t V, int64_t F, int64_t* keys, ufr_stream stream) {
  const char* who = "ufr_mesh_edge_keys";
  UFR_REQUIRE(faces && keys, "%s: null argument", who);
  UFR_CHECK(check_mesh_rows(who, V, F));
  hipStream_t s = static_cast<hipStream_t>(stream);
  UFR_TIMED("mesh_edge_keys", s, launch_edge_keys(faces, vertex_id, V, F, reinterpret_cast<long long*>(keys), s));
  return UFR_OK;
}

size_t ufr_mesh_face_components_workspace_bytes(int64_t F) {
  return (F >= 1 && F <= kChMax / 3) ? carved_bytes(carve_components, (long long)F) : 0;
}

int ufr_mesh_face_components(const int64_t* sorted_keys, const int64_t* order, int64_t F, int32_t* labels, void* workspace,
                             size_t workspace_bytes, int32_t* rounds_host, ufr_stream stream) {
  const char* who = "ufr_mesh_face_components";
  UFR_REQUIRE(sorted_keys && order && labels && workspace, "%s: null argument", who);
  UFR_REQUIRE(F >= 1 && F <= kChMax / 3, "%s: F %lld (must be 1 .. (2^31 - 1) / 3)", who, (long long)F);
  Carver c(workspace);
  const ComponentsWs w = carve_components(c, F);
  UFR_CHECK(check_workspace(who, workspace_bytes, c.off));
  hipStream_t s = static_cast<hipStream_t>(stream);
  UFR_TIMED("mesh_mark_pairs", s, launch_mark_pairs(reinterpret_cast<const long long*>(sorted_keys),
      reinterpret_cast<const long long*>(order), F, w.pair_a, w.pair_b, w.has_adj, w.parent, s));
  int rounds = 0;
  for (;;) {   // a round that hooks lowers some parent, and parents are >= 0: it ends; F + 1 rounds is label propagation's bound
    if (rounds > F) return fail(UFR_ERR_HIP, "%s: no fixpoint after %d rounds", who, rounds);
    int changed = 0;
    UFR_HIP(hipMemsetAsync(w.changed, 0, sizeof(int), s));
    UFR_TIMED("mesh_component_round", s, launch_component_round(w.pair_a, w.pair_b, F, w.parent, w.changed, s));
    UFR_HIP(hipMemcpyAsync(&changed, w.changed, sizeof(int), hipMemcpyDeviceToHost, s));
    UFR_HIP(hipStreamSynchronize(s));
    ++rounds;
    if (!changed) break;
  }
  UFR_TIMED("mesh_component_labels", s, launch_component_labels(w.parent, w.has_adj, F, labels, s));
  if (rounds_host) *rounds_host = rounds;
  return UFR_OK;
}

// ------------------------------------------------------------------ mesh rendering
int ufr_raster_vertex_normals(const double* verts, const int32_t* faces, int64_t V, int64_t F, const int64_t* sorted_slots,
                              const int64_t* run_starts, double* normals, ufr_stream stream) {
  const char* who = "ufr_raster_vertex_normals";
  UFR_REQUIRE(verts && faces && sorted_slots && run_starts && normals, "%s: null argument", who);
  UFR_CHECK(check_mesh_rows(who, V, F));
  hipStream_t s = static_cast<hipStream_t>(stream);
  UFR_TIMED("raster_vertex_normals", s, launch_raster_vertex_normals(verts, faces, V, F, reinterpret_cast<const long long*>(sorted_slots),
      reinterpret_cast<const long long*>(run_starts), normals, s));
  return UFR_OK;
}

size_t ufr_raster_frames_workspace_bytes(int64_t F, int32_t H, int32_t W) {
  if (F < 1 || F > kChMax || H < 1 || W < 1 || (long long)H * W >= (1ll << 31)) return 0;
  return carved_bytes(carve_raster_frames, (long long)F, (long long)H * W);
}

int ufr_raster_frames(const double* verts, const int32_t* faces, int64_t V, int64_t F, const double* normals, const uint8_t* colors,
                      const float* k_inv, const float* c2w, int32_t n_frames, int32_t H, int32_t W, const float* base_color,
                      const uint8_t* background, double ambient, uint8_t* image, float* depth, int32_t* face_id, float* normal_map,
                      void* workspace, size_t workspace_bytes, ufr_stream stream) {
  return raster_frames("ufr_raster_frames", verts, faces, V, F, normals, colors, nullptr, k_inv, c2w, n_frames, H, W, base_color,
                       background, ambient, image, depth, face_id, normal_map, workspace, workspace_bytes, stream);
}

int ufr_raster_downsample(const uint8_t* src, int32_t n, int32_t H, int32_t W, int32_t s, uint8_t* dst, ufr_stream stream) {
  const char* who = "ufr_raster_downsample";
  UFR_REQUIRE(src && dst, "%s: null argument", who);
  UFR_REQUIRE(n >= 1, "%s: n %d (must be >= 1)", who, n);
  UFR_REQUIRE(s >= 1 && s <= 4, "%s: s %d (must be 1 .. 4)", who, s);
  UFR_CHECK(depth_image_check(who, H, W));
  UFR_REQUIRE((long long)H * s * W * s < (1ll << 31), "%s: %dx%d times %d squared has 2^31 pixels or more", who, H, W, s);
  UFR_REQUIRE((long long)n * H * W * 3 < (1ll << 38), "%s: %d images of %dx%d have 2^38 bytes or more", who, n, H, W);
  hipStream_t st = static_cast<hipStream_t>(stream);
  UFR_TIMED("raster_downsample", st, launch_raster_downsample(src, n, H, W, s, dst, st));
  return UFR_OK;
}

// ------------------------------------------------------------------ mesh colouring
size_t ufr_color_vertices_workspace_bytes(int32_t n_views) {
  return (n_views >= 1 && n_views <= UFR_MESH_MAX_VIEWS) ? carved_bytes(carve_mesh_colors, (int)n_views) : 0;
}

int ufr_color_vertices(const double* verts, const double* normals, int64_t V, const uint8_t* images, const float* depth,
                           const double* k, const double* w2c, const double* centre, int32_t n_views, int32_t H, int32_t W,
                           double z_min, double depth_tol, double min_cos, int32_t power, int32_t mode, const uint8_t* fill,
                           uint8_t* colors, uint8_t* views_used, void* workspace, size_t workspace_bytes, ufr_stream stream) {
  const char* who = "ufr_color_vertices";
  UFR_REQUIRE(verts && images && k && w2c && centre && fill && colors && views_used && workspace, "%s: null argument", who);
  UFR_REQUIRE(V >= 1 && V <= kChMax, "%s: V %lld (must be 1 .. 2^31 - 1)", who, (long long)V);
  UFR_CHECK(color_rule_check(who, n_views, H, W, z_min, depth_tol, min_cos, power, mode));
  Carver cv(workspace);
  MeshColorCam* table = carve_mesh_colors(cv, n_views);
  UFR_REQUIRE(workspace_bytes >= cv.off, "%s: workspace too small: %zu < %zu bytes", who, workspace_bytes, cv.off);
  MeshColorCam cams[UFR_MESH_MAX_VIEWS];
  UFR_CHECK(color_cameras(who, k, w2c, centre, n_views, cams));   // all, before any launch
  hipStream_t s = static_cast<hipStream_t>(stream);
  UFR_TIMED("mesh_color_cams", s, launch_mesh_color_cams(cams, n_views, table, s));
  UFR_TIMED("mesh_vertex_colors", s, launch_mesh_vertex_colors(verts, normals, V, images, depth, table, n_views, H, W, z_min, depth_tol,
      min_cos, power, mode, fill, colors, views_used, s));
  return UFR_OK;
}

int ufr_color_fill_round(const int32_t* faces, int64_t V, int64_t F, const int64_t* sorted_slots, const int64_t* run_starts,
                              const uint8_t* colors_in, const uint8_t* state_in, uint8_t* colors_out, uint8_t* state_out,
                              int32_t* filled, ufr_stream stream) {
  const char* who = "ufr_color_fill_round";
  UFR_REQUIRE(faces && sorted_slots && run_starts && colors_in && state_in && colors_out && state_out && filled, "%s: null argument", who);
  UFR_CHECK(check_mesh_rows(who, V, F));
  UFR_REQUIRE(colors_out != colors_in && state_out != state_in, "%s: the round is double-buffered: out must not alias in", who);
  hipStream_t s = static_cast<hipStream_t>(stream);
  UFR_TIMED("mesh_color_fill_round", s, launch_mesh_color_fill_round(faces, V, F, reinterpret_cast<const long long*>(sorted_slots),
      reinterpret_cast<const long long*>(run_starts), colors_in, state_in, colors_out, state_out, filled, s));
  return UFR_OK;
}

// ------------------------------------------------------------------ mesh texturing
int ufr_texture_bake(const double* verts, const int32_t* faces, int64_t V, int64_t F, const uint8_t* images, const float* depth,
                     const double* k, const double* w2c, const double* centre, int32_t n_views, int32_t H, int32_t W, int32_t S,
                     int32_t Ht, int32_t Wt, double z_min, double depth_tol, double min_cos, int32_t power, int32_t mode,
                     const uint8_t* fill, const uint8_t* fallback, uint8_t* texture, uint8_t* views_used, void* workspace,
                     size_t workspace_size, ufr_stream stream) {
  const char* who = "ufr_texture_bake";
  UFR_REQUIRE(verts && faces && images && k && w2c && centre && fill && texture && views_used && workspace, "%s: null argument", who);
  UFR_REQUIRE(V >= 1 && V <= kChMax, "%s: V %lld (must be 1 .. 2^31 - 1)", who, (long long)V);
  TextureAtlas at;
  UFR_CHECK(texture_atlas_check(who, F, S, Ht, Wt, &at));
  UFR_CHECK(color_rule_check(who, n_views, H, W, z_min, depth_tol, min_cos, power, mode));
  Carver cv(workspace);
  MeshColorCam* table = carve_mesh_colors(cv, n_views);
  UFR_REQUIRE(workspace_size >= cv.off, "%s: workspace too small: %zu < %zu bytes", who, workspace_size, cv.off);
  MeshColorCam cams[UFR_MESH_MAX_VIEWS];
  UFR_CHECK(color_cameras(who, k, w2c, centre, n_views, cams));   // all, before any launch
  hipStream_t s = static_cast<hipStream_t>(stream);
  UFR_TIMED("mesh_color_cams", s, launch_mesh_color_cams(cams, n_views, table, s));
  UFR_TIMED("mesh_texture_bake", s, launch_texture_bake(verts, faces, V, at, images, depth, table, n_views, H, W, z_min, depth_tol,
      min_cos, power, mode, fill, fallback, texture, views_used, s));
  return UFR_OK;
}

int ufr_texture_fill_round(const uint8_t* colors_in, const uint8_t* state_in, int32_t S, int32_t Ht, int32_t Wt, int64_t F,
                           uint8_t* colors_out, uint8_t* state_out, int32_t* filled, ufr_stream stream) {
  const char* who = "ufr_texture_fill_round";
  UFR_REQUIRE(colors_in && state_in && colors_out && state_out && filled, "%s: null argument", who);
  TextureAtlas at;
  UFR_CHECK(texture_atlas_check(who, F, S, Ht, Wt, &at));
  UFR_REQUIRE(colors_out != colors_in && state_out != state_in, "%s: the round is double-buffered: out must not alias in", who);
  hipStream_t s = static_cast<hipStream_t>(stream);
  UFR_TIMED("mesh_texture_fill_round", s, launch_texture_fill_round(at, colors_in, state_in, colors_out, state_out, filled, s));
  return UFR_OK;
}

int ufr_texture_frames(const double* verts, const int32_t* faces, int64_t V, int64_t F, const double* normals, const double* corner_xy,
                       const uint8_t* texture, int32_t Ht, int32_t Wt, const float* k_inv, const float* c2w, int32_t n_frames,
                       int32_t H, int32_t W, const uint8_t* background, double ambient, uint8_t* image, float* depth,
                       int32_t* face_id, float* normal_map, void* workspace, size_t workspace_size, ufr_stream stream) {
  const char* who = "ufr_texture_frames";
  UFR_REQUIRE(verts && faces && corner_xy && texture && k_inv && c2w && image && workspace, "%s: null argument", who);
  UFR_REQUIRE(V >= 1 && V <= kChMax && F >= 1 && F <= kChMax, "%s: V %lld, F %lld (each must be 1 .. 2^31 - 1)", who, (long long)V,
              (long long)F);
  UFR_REQUIRE(Ht >= 1 && Wt >= 1 && Ht <= UFR_TEXTURE_MAX_SIDE && Wt <= UFR_TEXTURE_MAX_SIDE, "%s: texture %dx%d (Ht and Wt must be 1 .. %d)",
              who, Wt, Ht, UFR_TEXTURE_MAX_SIDE);
  const RasterTexture tex{corner_xy, texture, Ht, Wt};
  return raster_frames(who, verts, faces, V, F, normals, nullptr, &tex, k_inv, c2w, n_frames, H, W, nullptr, background, ambient, image,
                       depth, face_id, normal_map, workspace, workspace_size, stream);
}

// ------------------------------------------------------------------ mesh simplification
size_t ufr_simplify_workspace_bytes(int64_t n) { return (n >= 1 && n <= kChMax) ? carved_bytes(carve_simplify, (long long)n) : 0; }

int ufr_simplify_clusters(const int64_t* sorted_keys, const int64_t* order, int64_t V, int32_t* cluster, int64_t* cluster_key,
                          int64_t capacity, void* workspace, size_t workspace_bytes, int64_t* total_host, ufr_stream stream) {
  const char* who = "ufr_simplify_clusters";
  UFR_REQUIRE(sorted_keys && order && cluster && cluster_key && workspace && total_host, "%s: null argument", who);
  UFR_REQUIRE(V >= 1 && V <= kChMax, "%s: V %lld (must be 1 .. 2^31 - 1)", who, (long long)V);
  UFR_REQUIRE(capacity >= 0, "%s: capacity %lld", who, (long long)capacity);
  Carver c(workspace);
  const ScanWs w = carve_simplify(c, V);
  UFR_CHECK(check_workspace(who, workspace_bytes, c.off));
  hipStream_t s = static_cast<hipStream_t>(stream);
  UFR_TIMED("simplify_clusters", s, launch_simplify_clusters(reinterpret_cast<const long long*>(sorted_keys),
      reinterpret_cast<const long long*>(order), V, cluster, reinterpret_cast<long long*>(cluster_key), capacity, w.block_tot,
      w.block_off, w.total, s));
  long long tot = 0;
  UFR_CHECK(read_counts(&tot, w.total, 1, s));
  *total_host = (int64_t)tot;
  return UFR_OK;
}

int ufr_simplify_face_keys(const int32_t* faces, const int32_t* cluster, int64_t V, int64_t F, int64_t* keys, ufr_stream stream) {
  const char* who = "ufr_simplify_face_keys";
  UFR_REQUIRE(faces && cluster && keys, "%s: null argument", who);
  UFR_CHECK(simplify_counts_check(who, V, F));
  hipStream_t s = static_cast<hipStream_t>(stream);
  UFR_TIMED("simplify_face_keys", s, launch_simplify_face_keys(faces, cluster, V, F, reinterpret_cast<long long*>(keys), s));
  return UFR_OK;
}

int ufr_simplify_quadrics(const double* verts, const int32_t* faces, const int64_t* cluster_key, int64_t V, int64_t F, int64_t C,
                          const double* origin, double cell, const int64_t* sorted_keys, double* quadrics, int32_t* n_faces,
                          ufr_stream stream) {
  const char* who = "ufr_simplify_quadrics";
  UFR_REQUIRE(verts && faces && cluster_key && origin && sorted_keys && quadrics && n_faces, "%s: null argument", who);
  UFR_CHECK(simplify_counts_check(who, V, F));
  UFR_REQUIRE(C >= 1 && C <= V, "%s: C %lld (must be 1 .. V)", who, (long long)C);
  UFR_CHECK(cell_grid_check(who, cell, origin));
  hipStream_t s = static_cast<hipStream_t>(stream);
  UFR_TIMED("simplify_quadrics", s, launch_simplify_quadrics(verts, faces, reinterpret_cast<const long long*>(cluster_key), V, F, C,
      origin, cell, reinterpret_cast<const long long*>(sorted_keys), quadrics, n_faces, s));
  return UFR_OK;
}

int ufr_simplify_place(const double* quadrics, const int32_t* n_faces, const double* mean, const int64_t* cluster_key, int64_t C,
                       const double* origin, double cell, int32_t placement, double* position, uint8_t* placed,
                       ufr_stream stream) {
  const char* who = "ufr_simplify_place";
  UFR_REQUIRE(quadrics && n_faces && mean && cluster_key && origin && position && placed, "%s: null argument", who);
  UFR_REQUIRE(C >= 1 && C <= kChMax, "%s: C %lld (must be 1 .. 2^31 - 1)", who, (long long)C);
  UFR_CHECK(cell_grid_check(who, cell, origin));
  UFR_REQUIRE(placement == UFR_SIMPLIFY_QUADRIC || placement == UFR_SIMPLIFY_MEAN, "%s: unknown placement %d", who, placement);
  hipStream_t s = static_cast<hipStream_t>(stream);
  UFR_TIMED("simplify_place", s, launch_simplify_place(quadrics, n_faces, mean, reinterpret_cast<const long long*>(cluster_key), C,
      origin, cell, placement, position, placed, s));
  return UFR_OK;
}

int ufr_simplify_face_triples(const int32_t* faces, const int32_t* cluster, int64_t V, int64_t F, int32_t* triples,
                              int64_t* key_a, int64_t* key_bc, ufr_stream stream) {
  const char* who = "ufr_simplify_face_triples";
  UFR_REQUIRE(faces && cluster && triples && key_a && key_bc, "%s: null argument", who);
  UFR_CHECK(simplify_counts_check(who, V, F));
  hipStream_t s = static_cast<hipStream_t>(stream);
  UFR_TIMED("simplify_face_triples", s, launch_simplify_face_triples(faces, cluster, V, F, triples,
      reinterpret_cast<long long*>(key_a), reinterpret_cast<long long*>(key_bc), s));
  return UFR_OK;
}

int ufr_simplify_face_heads(const int64_t* key_a, const int64_t* key_bc, const int64_t* order, int64_t F, uint8_t* keep,
                            ufr_stream stream) {
  const char* who = "ufr_simplify_face_heads";
  UFR_REQUIRE(key_a && key_bc && order && keep, "%s: null argument", who);
  UFR_REQUIRE(F >= 1 && F <= kChMax, "%s: F %lld (must be 1 .. 2^31 - 1)", who, (long long)F);
  hipStream_t s = static_cast<hipStream_t>(stream);
  UFR_TIMED("simplify_face_heads", s, launch_simplify_face_heads(reinterpret_cast<const long long*>(key_a),
      reinterpret_cast<const long long*>(key_bc), reinterpret_cast<const long long*>(order), F, keep, s));
  return UFR_OK;
}

int ufr_simplify_compact_faces(const int32_t* triples, const uint8_t* keep, int64_t F, int64_t C, int32_t* out_faces,
                               int32_t* face_map, int64_t capacity, uint8_t* referenced, void* workspace,
                               size_t workspace_bytes, int64_t* total_host, ufr_stream stream) {
  const char* who = "ufr_simplify_compact_faces";
  UFR_REQUIRE(triples && keep && referenced && workspace && total_host, "%s: null argument", who);
  UFR_REQUIRE(F >= 1 && F <= kChMax && C >= 1 && C <= kChMax, "%s: F %lld, C %lld (each must be 1 .. 2^31 - 1)", who, (long long)F,
              (long long)C);
  UFR_REQUIRE(capacity >= 0, "%s: capacity %lld", who, (long long)capacity);
  UFR_REQUIRE(capacity == 0 || (out_faces && face_map), "%s: null argument (an output with capacity %lld)", who, (long long)capacity);
  Carver c(workspace);
  const ScanWs w = carve_simplify(c, F);
  UFR_CHECK(check_workspace(who, workspace_bytes, c.off));
  hipStream_t s = static_cast<hipStream_t>(stream);
  UFR_TIMED("simplify_compact_faces", s, launch_simplify_compact_faces(triples, keep, F, C, out_faces, face_map, capacity, referenced,
      w.block_tot, w.block_off, w.total, s));
  long long tot = 0;
  UFR_CHECK(read_counts(&tot, w.total, 1, s));
  *total_host = (int64_t)tot;
  return UFR_OK;
}

int ufr_simplify_compact_vertices(const uint8_t* referenced, int64_t C, const double* position, const uint8_t* colors,
                                  const uint8_t* placed, const int32_t* count, const int32_t* cluster, int64_t V, int32_t* faces,
                                  int64_t n_faces, double* out_verts, uint8_t* out_colors, uint8_t* out_placed,
                                  int32_t* out_count, int64_t capacity, int32_t* cluster_vertex, int32_t* vertex_map,
                                  void* workspace, size_t workspace_bytes, int64_t* total_host, ufr_stream stream) {
  const char* who = "ufr_simplify_compact_vertices";
  UFR_REQUIRE(referenced && position && placed && count && cluster && cluster_vertex && vertex_map && workspace && total_host,
              "%s: null argument", who);
  UFR_REQUIRE(C >= 1 && C <= kChMax && V >= 1 && V <= kChMax, "%s: C %lld, V %lld (each must be 1 .. 2^31 - 1)", who, (long long)C,
              (long long)V);
  UFR_REQUIRE(n_faces >= 0 && n_faces <= kChMax && (n_faces == 0 || faces), "%s: n_faces %lld (must be 0 .. 2^31 - 1, faces given)", who,
              (long long)n_faces);
  UFR_REQUIRE(capacity >= 0, "%s: capacity %lld", who, (long long)capacity);
  UFR_REQUIRE(capacity == 0 || (out_verts && out_placed && out_count && (!colors || out_colors)),
              "%s: null argument (an output with capacity %lld)", who, (long long)capacity);
  Carver c(workspace);
  const ScanWs w = carve_simplify(c, C);
  UFR_CHECK(check_workspace(who, workspace_bytes, c.off));
  hipStream_t s = static_cast<hipStream_t>(stream);
  UFR_TIMED("simplify_compact_vertices", s, launch_simplify_compact_vertices(referenced, C, position, colors, placed, count, cluster, V,
      faces, n_faces, out_verts, out_colors, out_placed, out_count, capacity, cluster_vertex, vertex_map, w.block_tot, w.block_off,
      w.total, s));
  long long tot = 0;
  UFR_CHECK(read_counts(&tot, w.total, 1, s));
  *total_host = (int64_t)tot;
  return UFR_OK;
}

// ------------------------------------------------------------------ mesh smoothing
size_t ufr_smooth_workspace_bytes(int64_t V, int64_t F, int32_t weights) {
  if (V < 1 || V > kChMax || F < 1 || F > kChMax / 3 || (weights != UFR_SMOOTH_UNIFORM && weights != UFR_SMOOTH_COTANGENT)) return 0;
  return carved_bytes(carve_mesh_smooth, (long long)F, (int)weights);
}

int ufr_smooth_rows(const double* verts, const int32_t* faces, int64_t V, int64_t F, const int64_t* sorted_slots,
                         const int64_t* run_starts, int32_t weights, uint8_t* border, void* workspace, size_t workspace_bytes,
                         ufr_stream stream) {
  const char* who = "ufr_smooth_rows";
  UFR_REQUIRE(verts && faces && sorted_slots && run_starts && border && workspace, "%s: null argument", who);
  UFR_CHECK(smooth_check(who, V, F, weights));
  Carver c(workspace);
  const SmoothWs w = carve_mesh_smooth(c, F, weights);
  UFR_CHECK(check_workspace(who, workspace_bytes, c.off));
  hipStream_t s = static_cast<hipStream_t>(stream);
  UFR_TIMED("mesh_smooth_rows", s, launch_mesh_smooth_rows(verts, faces, V, F, reinterpret_cast<const long long*>(sorted_slots),
      weights == UFR_SMOOTH_COTANGENT, w.nbr, w.wgt, s));
  UFR_TIMED("mesh_smooth_border", s, launch_mesh_smooth_border(V, F, reinterpret_cast<const long long*>(run_starts), w.nbr, border, s));
  return UFR_OK;
}

int ufr_smooth_steps(int64_t V, int64_t F, const int64_t* run_starts, int32_t weights, const uint8_t* border,
                          const uint8_t* pinned, const double* factors, int32_t n_steps, double* pos_a, double* pos_b,
                          const void* workspace, size_t workspace_bytes, ufr_stream stream) {
  const char* who = "ufr_smooth_steps";
  UFR_REQUIRE(run_starts && pos_a && pos_b && workspace && (factors || n_steps == 0), "%s: null argument", who);
  UFR_REQUIRE(pos_a != pos_b, "%s: pos_a and pos_b are one buffer", who);
  UFR_CHECK(smooth_check(who, V, F, weights));
  UFR_REQUIRE(n_steps >= 0, "%s: n_steps %d (must be >= 0)", who, n_steps);
  for (int i = 0; i < n_steps; ++i)
    UFR_REQUIRE(std::isfinite(factors[i]), "%s: factor %d is %g (must be finite)", who, i, factors[i]);
  Carver c(const_cast<void*>(workspace));
  const SmoothWs w = carve_mesh_smooth(c, F, weights);
  UFR_CHECK(check_workspace(who, workspace_bytes, c.off));
  hipStream_t s = static_cast<hipStream_t>(stream);
  for (int i = 0; i < n_steps; ++i) {
    const auto pos = ping_pong(i, pos_a, pos_b);
    UFR_TIMED("mesh_smooth_step", s, launch_mesh_smooth_step(V, F, reinterpret_cast<const long long*>(run_starts), w.nbr, w.wgt, border,
        pinned, factors[i], pos.in, pos.out, s));
  }
  return UFR_OK;
}

// ------------------------------------------------------------------ mesh denoising
size_t ufr_denoise_workspace_bytes(int64_t V, int64_t F) {
  if (V < 1 || V > kChMax || F < 1 || F > kChMax / 3) return 0;
  return carved_bytes(carve_mesh_denoise, (long long)F);
}

int ufr_denoise_faces(const double* verts, const int32_t* faces, int64_t V, int64_t F, const int64_t* sorted_slots,
                      const int64_t* run_starts, double* normals, uint8_t* border, void* workspace, size_t workspace_bytes,
                      ufr_stream stream) {
  const char* who = "ufr_denoise_faces";
  UFR_REQUIRE(verts && faces && sorted_slots && run_starts && normals && border && workspace, "%s: null argument", who);
  UFR_REQUIRE(normals != verts, "%s: normals and verts are one buffer", who);
  UFR_CHECK(check_mesh_rows(who, V, F));
  Carver c(workspace);
  const DenoiseWs w = carve_mesh_denoise(c, F);
  UFR_CHECK(check_workspace(who, workspace_bytes, c.off));
  hipStream_t s = static_cast<hipStream_t>(stream);
  UFR_TIMED("mesh_denoise_faces", s, launch_mesh_denoise_faces(verts, faces, V, F, w.rec_a, normals, s));
  UFR_TIMED("mesh_denoise_rows", s, launch_mesh_denoise_rows(faces, V, F, reinterpret_cast<const long long*>(sorted_slots), w.rec_a,
      w.rows, w.row_face, s));
  UFR_TIMED("mesh_denoise_border", s, launch_mesh_denoise_border(V, F, reinterpret_cast<const long long*>(run_starts), w.rows, border, s));
  return UFR_OK;
}

int ufr_denoise_normals(const int32_t* faces, int64_t V, int64_t F, const int64_t* run_starts, double two_ss, double two_rr,
                        int32_t n_steps, double* normals, void* workspace, size_t workspace_bytes, ufr_stream stream) {
  const char* who = "ufr_denoise_normals";
  UFR_REQUIRE(faces && run_starts && normals && workspace, "%s: null argument", who);
  UFR_CHECK(check_mesh_rows(who, V, F));
  UFR_REQUIRE(std::isfinite(two_ss) && two_ss > 0.0, "%s: two_ss %g (must be finite and above 0)", who, two_ss);
  UFR_REQUIRE(std::isfinite(two_rr) && two_rr > 0.0, "%s: two_rr %g (must be finite and above 0)", who, two_rr);
  UFR_REQUIRE(n_steps >= 0, "%s: n_steps %d (must be >= 0)", who, n_steps);
  Carver c(workspace);
  const DenoiseWs w = carve_mesh_denoise(c, F);
  UFR_CHECK(check_workspace(who, workspace_bytes, c.off));
  hipStream_t s = static_cast<hipStream_t>(stream);
  for (int i = 0; i < n_steps; ++i) {
    const auto rec = ping_pong(i, w.rec_a, w.rec_b);
    UFR_TIMED("mesh_denoise_normals", s, launch_mesh_denoise_normals(faces, V, F, reinterpret_cast<const long long*>(run_starts), w.row_face,
        two_ss, two_rr, rec.in, rec.out, i == n_steps - 1 ? normals : nullptr, s));
  }
  return UFR_OK;
}

int ufr_denoise_vertices(int64_t V, int64_t F, const int64_t* run_starts, const double* normals, const uint8_t* border,
                         const uint8_t* pinned, int32_t n_steps, double* pos_a, double* pos_b, const void* workspace,
                         size_t workspace_bytes, ufr_stream stream) {
  const char* who = "ufr_denoise_vertices";
  UFR_REQUIRE(run_starts && normals && pos_a && pos_b && workspace, "%s: null argument", who);
  UFR_REQUIRE(pos_a != pos_b, "%s: pos_a and pos_b are one buffer", who);
  UFR_REQUIRE(normals != pos_a && normals != pos_b, "%s: normals and a position buffer are one buffer", who);
  UFR_CHECK(check_mesh_rows(who, V, F));
  UFR_REQUIRE(n_steps >= 0, "%s: n_steps %d (must be >= 0)", who, n_steps);
  Carver c(const_cast<void*>(workspace));
  const DenoiseWs w = carve_mesh_denoise(c, F);
  UFR_CHECK(check_workspace(who, workspace_bytes, c.off));
  hipStream_t s = static_cast<hipStream_t>(stream);
  for (int i = 0; i < n_steps; ++i) {
    const auto pos = ping_pong(i, pos_a, pos_b);
    UFR_TIMED("mesh_denoise_vertices", s, launch_mesh_denoise_vertices(V, F, reinterpret_cast<const long long*>(run_starts), w.rows, normals,
        border, pinned, pos.in, pos.out, s));
  }
  return UFR_OK;
}

}  // extern "C"
