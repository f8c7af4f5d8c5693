// extern "C" surface of libufr.so (include/ufr.h), geometry after the network other than meshes: TSDF fusion, marching cubes,
// the similarity field, the DTU chamfer evaluation, point-cloud filtering, depth-map fusion, point-cloud rendering and Poisson
// surface reconstruction (meshes: api_mesh.hip).  The count / emit pairs synchronise the stream to hand a count to the host; so
// do the rounds of point thinning and the looks of the Poisson solver.
#include "api_geometry_common.h"
#include "mcubes_table.h"

using namespace ufr;
using namespace ufr::api;

namespace {

// ---- marching cubes: [tile sums int32 x2 | tile offsets int64 x2 | totals int64 x2 | index volume int32 per voxel]
struct McWs { int *tile_counts, *index; long long *tile_off, *totals; };
McWs carve_mcubes(Carver& c, const int32_t* dim) {
  const size_t tiles = (size_t)mcubes_tiles(dim), n = (size_t)dim[0] * dim[1] * dim[2];
  McWs w;
  w.tile_counts = c.take<int>(tiles * 2);
  w.tile_off = c.take<long long>(tiles * 2);
  w.totals = c.take<long long>(2);
  w.index = c.take<int>(n);
  return w;
}

int mc_check(const char* who, const float* vol, const int32_t* dim, void* ws, size_t ws_bytes, McWs* w) {
  UFR_REQUIRE(vol && dim && ws, "%s: null argument", who);
  UFR_REQUIRE(dim[0] >= 2 && dim[1] >= 2 && dim[2] >= 2, "%s: volume %dx%dx%d (every dim must be >= 2)", who, dim[0], dim[1], dim[2]);
  UFR_REQUIRE((long long)dim[0] * dim[1] * dim[2] < (1ll << 31), "%s: volume %dx%dx%d has 2^31 voxels or more", who, dim[0], dim[1],
              dim[2]);
  Carver c(ws);
  *w = carve_mcubes(c, dim);
  return check_workspace(who, ws_bytes, c.off);
}

// ---- DTU chamfer evaluation
// mesh sampling: [per-triangle offset in its block int64 | block sums int64 | block offsets int64 | total int64]
struct SampleWs { long long* tri_off; ScanWs scan; };
SampleWs carve_mesh_sample(Carver& c, long long F) {
  SampleWs w;
  w.tri_off = c.take<long long>((size_t)F);
  w.scan = carve_scan(c, (size_t)chamfer_blocks(F));
  return w;
}

int sample_check(const char* who, const double* verts, const int32_t* faces, int64_t V, int64_t F, double density, void* ws,
                 size_t ws_bytes, SampleWs* w) {
  UFR_REQUIRE(verts && faces && ws, "%s: null argument", who);
  UFR_REQUIRE(V >= 1 && V <= kChMax && F >= 1 && F <= kChMax, "%s: V %lld, F %lld (each must be 1 .. 2^31 - 1)", who, (long long)V,
              (long long)F);
  UFR_REQUIRE(density > 0.0 && std::isfinite(density), "%s: density %g (must be positive and finite)", who, density);
  Carver c(ws);
  *w = carve_mesh_sample(c, F);
  return check_workspace(who, ws_bytes, c.off);
}

// thinning: [undecided count int32]
int* carve_points_thin(Carver& c) { return c.take<int>(1); }

// nearest neighbours: [block sums fp64 | block counts int64]
struct NnWs { double* block_sum; long long* block_cnt; };
NnWs carve_nn_dist(Carver& c, long long nq) {
  const size_t blocks = (size_t)chamfer_blocks(nq);
  NnWs w;
  w.block_sum = c.take<double>(blocks);
  w.block_cnt = c.take<long long>(blocks);
  return w;
}

// ---- point-cloud filtering (voxel means) and depth-map fusion (the valid pixels) each take one scan workspace
int depth_points_check(const char* who, const uint8_t* mask, int32_t H, int32_t W, void* ws, size_t ws_bytes, ScanWs* w) {
  UFR_REQUIRE(mask && ws, "%s: null argument", who);
  UFR_CHECK(depth_image_check(who, H, W));
  Carver c(ws);
  *w = carve_scan(c, (size_t)depth_points_blocks((long long)H * W));
  return check_workspace(who, ws_bytes, c.off);
}

// point-cloud rendering: [key image uint64 per pixel]
unsigned long long* carve_splat_frames(Carver& c, long long pixels) { return c.take<unsigned long long>((size_t)pixels); }

}  // namespace

extern "C" {

// ------------------------------------------------------------------ TSDF fusion
int ufr_tsdf_integrate(float* tsdf, float* weight, float* color, const int32_t* dim, const float* origin,
                       float voxel_size, float trunc_margin, const float* cam_intr, const float* cam_pose,
                       const float* depth_im, const float* color_im, int32_t im_h, int32_t im_w, float obs_weight,
                       int32_t integrate_color, ufr_stream stream) {
  UFR_REQUIRE(tsdf && weight && dim && origin && cam_intr && cam_pose && depth_im, "ufr_tsdf_integrate: null argument");
  UFR_REQUIRE(dim[0] > 0 && dim[1] > 0 && dim[2] > 0, "ufr_tsdf_integrate: volume %dx%dx%d", dim[0], dim[1], dim[2]);
  UFR_REQUIRE(im_h > 0 && im_w > 0, "ufr_tsdf_integrate: image %dx%d", im_h, im_w);
  UFR_REQUIRE(voxel_size > 0.f && trunc_margin > 0.f, "ufr_tsdf_integrate: voxel_size %g, trunc_margin %g", voxel_size, trunc_margin);
  UFR_REQUIRE(!integrate_color || (color && color_im), "ufr_tsdf_integrate: colour integration needs color and color_im");
  hipStream_t s = static_cast<hipStream_t>(stream);
  UFR_TIMED("tsdf_integrate", s, launch_tsdf_integrate(tsdf, weight, color, dim, origin, voxel_size, trunc_margin, cam_intr, cam_pose,
      depth_im, color_im, im_h, im_w, obs_weight, integrate_color, s));
  return UFR_OK;
}

// ------------------------------------------------------------------ marching cubes
size_t ufr_marching_cubes_workspace_bytes(const int32_t* dim) {
  if (!dim || dim[0] < 2 || dim[1] < 2 || dim[2] < 2 || (long long)dim[0] * dim[1] * dim[2] >= (1ll << 31)) return 0;
  return carved_bytes(carve_mcubes, dim);
}

int ufr_marching_cubes_count(const float* vol, const int32_t* dim, float level, void* workspace, size_t workspace_bytes,
                             int32_t* counts_host, ufr_stream stream) {
  McWs w;
  UFR_CHECK(mc_check("ufr_marching_cubes_count", vol, dim, workspace, workspace_bytes, &w));
  UFR_REQUIRE(counts_host, "ufr_marching_cubes_count: null argument (counts_host)");
  hipStream_t s = static_cast<hipStream_t>(stream);
  UFR_TIMED("mcubes_count", s, launch_mcubes_count(vol, dim, level, w.tile_counts, s));
  UFR_TIMED("mcubes_scan", s, launch_mcubes_scan(w.tile_counts, mcubes_tiles(dim), w.tile_off, w.totals, s));
  long long tot[2] = {0, 0};
  UFR_CHECK(read_counts(tot, w.totals, 2, s));
  UFR_REQUIRE(tot[0] < (1ll << 31) && tot[1] < (1ll << 31), "ufr_marching_cubes_count: %lld vertices, %lld faces: 2^31 or more",
              tot[0], tot[1]);
  counts_host[0] = (int32_t)tot[0];
  counts_host[1] = (int32_t)tot[1];
  return UFR_OK;
}

int ufr_marching_cubes_emit(const float* vol, const int32_t* dim, float level, void* workspace, size_t workspace_bytes,
                            float* verts, float* normals, int32_t* faces, int32_t n_verts, int32_t n_faces, ufr_stream stream) {
  McWs w;
  UFR_CHECK(mc_check("ufr_marching_cubes_emit", vol, dim, workspace, workspace_bytes, &w));
  UFR_REQUIRE(n_verts >= 0 && n_faces >= 0, "ufr_marching_cubes_emit: n_verts %d, n_faces %d", n_verts, n_faces);
  UFR_REQUIRE((n_verts == 0 || (verts && normals)) && (n_faces == 0 || faces), "ufr_marching_cubes_emit: null argument");
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (n_verts == 0 && n_faces == 0) return UFR_OK;
  // the vertices, and the index volume the faces need
  UFR_TIMED("mcubes_verts", s, launch_mcubes_verts(vol, dim, level, w.tile_off, w.index, verts, normals, n_verts, s));
  if (n_faces > 0) UFR_TIMED("mcubes_faces", s, launch_mcubes_faces(vol, dim, level, w.tile_off, w.index, faces, n_faces, s));
  return UFR_OK;
}

int ufr_marching_cubes_table(int8_t* out, int32_t out_len) {
  static_assert(sizeof(kMcTable[0]) == UFR_MC_TABLE_ROW, "mcubes_table.h and ufr.h disagree on the row length");
  UFR_REQUIRE(out, "ufr_marching_cubes_table: null argument");
  UFR_REQUIRE(out_len >= 256 * UFR_MC_TABLE_ROW, "ufr_marching_cubes_table: out_len %d < %d", out_len, 256 * UFR_MC_TABLE_ROW);
  memcpy(out, kMcTable, sizeof(kMcTable));
  return UFR_MC_TABLE_ROW;
}

// ------------------------------------------------------------------ similarity field
int ufr_similarity_field(const ufr_frame* frame, const float* gx, const float* gy, const float* gz, const int32_t* dim, float* u,
                         uint8_t* n_vis, int32_t min_views, ufr_stream stream) {
  const FrameDev* f = frame_of(frame);
  UFR_REQUIRE(f, "ufr_similarity_field: frame handle not prepared");
  UFR_REQUIRE(f->match, "ufr_similarity_field: the frame has no matching features");
  UFR_REQUIRE(gx && gy && gz && dim && u, "ufr_similarity_field: null argument");
  UFR_REQUIRE(dim[0] >= 2 && dim[1] >= 2 && dim[2] >= 2, "ufr_similarity_field: grid %dx%dx%d (every dim must be >= 2)", dim[0], dim[1],
              dim[2]);
  UFR_REQUIRE((long long)dim[0] * dim[1] * dim[2] < (1ll << 31), "ufr_similarity_field: grid %dx%dx%d has 2^31 voxels or more", dim[0],
              dim[1], dim[2]);
  UFR_REQUIRE(min_views >= 0 && min_views <= f->NV, "ufr_similarity_field: min_views %d (0 .. NV = %d)", min_views, f->NV);
  hipStream_t s = static_cast<hipStream_t>(stream);
  UFR_TIMED("similarity_field", s, launch_similarity_field(*f, gx, gy, gz, dim, u, n_vis, min_views, s));
  return UFR_OK;
}

// ------------------------------------------------------------------ DTU chamfer evaluation
size_t ufr_mesh_sample_workspace_bytes(int64_t F) {
  return (F >= 1 && F <= kChMax) ? carved_bytes(carve_mesh_sample, F) : 0;
}

int ufr_mesh_sample_count(const double* verts, const int32_t* faces, int64_t V, int64_t F, double density, void* workspace,
                          size_t workspace_bytes, int64_t* total_host, ufr_stream stream) {
  SampleWs w;
  UFR_CHECK(sample_check("ufr_mesh_sample_count", verts, faces, V, F, density, workspace, workspace_bytes, &w));
  UFR_REQUIRE(total_host, "ufr_mesh_sample_count: null argument (total_host)");
  hipStream_t s = static_cast<hipStream_t>(stream);
  UFR_TIMED("mesh_sample_count", s, launch_mesh_sample_count(verts, faces, V, F, density, w.tri_off, w.scan.block_tot, s));
  UFR_TIMED("mesh_sample_scan", s, launch_mesh_sample_scan(w.scan.block_tot, chamfer_blocks(F), w.scan.block_off, w.scan.total, s));
  long long tot = 0;
  UFR_CHECK(read_counts(&tot, w.scan.total, 1, s));
  *total_host = (int64_t)tot;
  return UFR_OK;
}

int ufr_mesh_sample_emit(const double* verts, const int32_t* faces, int64_t V, int64_t F, double density, void* workspace,
                         size_t workspace_bytes, double* out, int64_t capacity, ufr_stream stream) {
  SampleWs w;
  UFR_CHECK(sample_check("ufr_mesh_sample_emit", verts, faces, V, F, density, workspace, workspace_bytes, &w));
  UFR_REQUIRE(capacity >= 0, "ufr_mesh_sample_emit: capacity %lld", (long long)capacity);
  UFR_REQUIRE(capacity == 0 || out, "ufr_mesh_sample_emit: null argument (out)");
  if (capacity == 0) return UFR_OK;
  hipStream_t s = static_cast<hipStream_t>(stream);
  UFR_TIMED("mesh_sample_emit", s, launch_mesh_sample_emit(verts, faces, V, F, density, w.tri_off, w.scan.block_off, out, capacity, s));
  return UFR_OK;
}

int ufr_points_cell_keys(const double* points, int64_t n, const double* origin, double cell, int64_t* keys, ufr_stream stream) {
  UFR_REQUIRE(points && origin && keys, "ufr_points_cell_keys: null argument");
  UFR_REQUIRE(n >= 1 && n <= kChMax, "ufr_points_cell_keys: n %lld (must be 1 .. 2^31 - 1)", (long long)n);
  UFR_CHECK(cell_grid_check("ufr_points_cell_keys", cell, origin));
  hipStream_t s = static_cast<hipStream_t>(stream);
  UFR_TIMED("points_cell_keys", s, launch_points_cell_keys(points, n, origin, cell, reinterpret_cast<long long*>(keys), s));
  return UFR_OK;
}

size_t ufr_points_thin_workspace_bytes(int64_t n) {
  return (n >= 1 && n <= kChMax) ? carved_bytes(carve_points_thin) : 0;
}

int ufr_points_thin(const double* points, const int64_t* keys, const int32_t* rank, int64_t n, double radius, uint8_t* state,
                    void* workspace, size_t workspace_bytes, int32_t* rounds_host, ufr_stream stream) {
  UFR_REQUIRE(points && keys && rank && state && workspace, "ufr_points_thin: null argument");
  UFR_REQUIRE(n >= 1 && n <= kChMax, "ufr_points_thin: n %lld (must be 1 .. 2^31 - 1)", (long long)n);
  UFR_REQUIRE(radius >= 0.0 && std::isfinite(radius), "ufr_points_thin: radius %g (must be finite and >= 0)", radius);
  Carver c(workspace);
  int* undecided = carve_points_thin(c);
  UFR_CHECK(check_workspace("ufr_points_thin", workspace_bytes, c.off));
  hipStream_t s = static_cast<hipStream_t>(stream);
  UFR_HIP(hipMemsetAsync(state, 0, (size_t)n, s));
  long long prev = n;
  int rounds = 0;
  while (prev > 0) {       // every round decides at least the earliest undecided point: at most n rounds
    if (rounds >= n) return fail(UFR_ERR_HIP, "ufr_points_thin: no fixpoint after %d rounds", rounds);
    int und = 0;
    UFR_HIP(hipMemsetAsync(undecided, 0, sizeof(int), s));
    UFR_TIMED("points_thin_round", s, launch_thin_round(points, reinterpret_cast<const long long*>(keys), rank, n, radius, state,
        undecided, s));
    UFR_HIP(hipMemcpyAsync(&und, undecided, sizeof(int), hipMemcpyDeviceToHost, s));
    UFR_HIP(hipStreamSynchronize(s));
    ++rounds;
    if (und < 0 || und >= prev)
      return fail(UFR_ERR_HIP, "ufr_points_thin: round %d left %d of %lld points undecided (rank is not a permutation?)", rounds, und,
                  prev);
    prev = und;
  }
  if (rounds_host) *rounds_host = rounds;
  return UFR_OK;
}

size_t ufr_points_nn_dist_workspace_bytes(int64_t nq) {
  return (nq >= 1 && nq <= kChMax) ? carved_bytes(carve_nn_dist, nq) : 0;
}

int ufr_points_nn_dist(const double* query, int64_t nq, const double* ref, const int64_t* ref_keys, int64_t nr,
                       const double* origin, double cell, double max_dist, double* dist, double* mean_out, void* workspace,
                       size_t workspace_bytes, ufr_stream stream) {
  UFR_REQUIRE(query && ref && ref_keys && origin && dist && workspace, "ufr_points_nn_dist: null argument");
  UFR_REQUIRE(nq >= 1 && nq <= kChMax && nr >= 1 && nr <= kChMax, "ufr_points_nn_dist: nq %lld, nr %lld (each must be 1 .. 2^31 - 1)",
              (long long)nq, (long long)nr);
  UFR_CHECK(cell_grid_check("ufr_points_nn_dist", cell, origin));
  UFR_REQUIRE(max_dist > 0.0 && max_dist < 1e150, "ufr_points_nn_dist: max_dist %g (must be positive, below 1e150)", max_dist);
  Carver c(workspace);
  const NnWs w = carve_nn_dist(c, nq);
  UFR_CHECK(check_workspace("ufr_points_nn_dist", workspace_bytes, c.off));
  hipStream_t s = static_cast<hipStream_t>(stream);
  UFR_TIMED("points_nn_dist", s, launch_nn_dist(query, nq, ref, reinterpret_cast<const long long*>(ref_keys), nr, origin, cell, max_dist,
      dist, w.block_sum, w.block_cnt, mean_out, s));
  return UFR_OK;
}

// ------------------------------------------------------------------ point-cloud filtering
int ufr_points_knn(const double* query, int64_t nq, const double* ref, const int64_t* ref_keys, const int32_t* ref_index,
                   int64_t nr, const double* origin, double cell, const int32_t* self_index, int32_t k, double max_dist,
                   int32_t* idx, double* dist, ufr_stream stream) {
  const char* who = "ufr_points_knn";
  UFR_REQUIRE(query && ref && ref_keys && ref_index && origin && idx && dist, "%s: null argument", who);
  UFR_REQUIRE(nq >= 1 && nq <= kChMax && nr >= 1 && nr <= kChMax, "%s: nq %lld, nr %lld (each must be 1 .. 2^31 - 1)", who,
              (long long)nq, (long long)nr);
  UFR_REQUIRE(k >= 1 && k <= UFR_KNN_MAX_K, "%s: k %d (must be 1 .. %d)", who, k, UFR_KNN_MAX_K);
  UFR_CHECK(cell_grid_check(who, cell, origin));
  UFR_REQUIRE(max_dist > 0.0, "%s: max_dist %g (must be positive; +inf for no limit)", who, max_dist);
  hipStream_t s = static_cast<hipStream_t>(stream);
  UFR_TIMED("points_knn", s, launch_points_knn(query, nq, ref, reinterpret_cast<const long long*>(ref_keys), ref_index, nr, origin,
      cell, self_index, k, max_dist, idx, dist, s));
  return UFR_OK;
}

int ufr_points_normals(const double* points, int64_t n, const int32_t* idx, int32_t k, const double* viewpoints, int32_t V,
                       double* normal, double* curvature, uint8_t* valid, ufr_stream stream) {
  const char* who = "ufr_points_normals";
  UFR_REQUIRE(points && idx && normal && curvature && valid, "%s: null argument", who);
  UFR_REQUIRE(n >= 1 && n <= kChMax, "%s: n %lld (must be 1 .. 2^31 - 1)", who, (long long)n);
  UFR_REQUIRE(k >= 1 && k <= UFR_KNN_MAX_K, "%s: k %d (must be 1 .. %d)", who, k, UFR_KNN_MAX_K);
  UFR_REQUIRE(V >= 0 && (V == 0 || viewpoints), "%s: V %d with %s viewpoints (V must be >= 0)", who, V, viewpoints ? "given" : "null");
  hipStream_t s = static_cast<hipStream_t>(stream);
  UFR_TIMED("points_normals", s, launch_points_normals(points, n, idx, k, viewpoints, V, normal, curvature, valid, s));
  return UFR_OK;
}

size_t ufr_points_voxel_mean_workspace_bytes(int64_t n) {
  return (n >= 1 && n <= kChMax) ? carved_bytes(carve_scan, (size_t)points_filter_blocks(n)) : 0;
}

int ufr_points_voxel_mean(const double* points, const int64_t* keys, int64_t n, const uint8_t* colors, const double* normals,
                          double* out_points, uint8_t* out_colors, double* out_normals, int32_t* count, int64_t capacity,
                          void* workspace, size_t workspace_bytes, int64_t* total_host, ufr_stream stream) {
  const char* who = "ufr_points_voxel_mean";
  UFR_REQUIRE(points && keys && workspace && total_host, "%s: null argument", who);
  UFR_REQUIRE(n >= 1 && n <= kChMax, "%s: n %lld (must be 1 .. 2^31 - 1)", who, (long long)n);
  UFR_REQUIRE(capacity >= 0, "%s: capacity %lld", who, (long long)capacity);
  UFR_REQUIRE(capacity == 0 || (out_points && count && (!colors || out_colors) && (!normals || out_normals)),
              "%s: null argument (an output with capacity %lld)", who, (long long)capacity);
  Carver c(workspace);
  const ScanWs w = carve_scan(c, (size_t)points_filter_blocks(n));
  UFR_CHECK(check_workspace(who, workspace_bytes, c.off));
  hipStream_t s = static_cast<hipStream_t>(stream);
  const long long* k64 = reinterpret_cast<const long long*>(keys);
  UFR_TIMED("points_voxel_count", s, launch_voxel_count(k64, n, w.block_tot, w.block_off, w.total, s));
  if (capacity > 0)
    UFR_TIMED("points_voxel_mean", s, launch_voxel_mean(points, k64, n, colors, normals, w.block_off, out_points, out_colors, out_normals,
        count, capacity, s));
  long long tot = 0;
  UFR_CHECK(read_counts(&tot, w.total, 1, s));
  *total_host = (int64_t)tot;
  return UFR_OK;
}

// ------------------------------------------------------------------ depth-map fusion
int ufr_depth_consistency(const float* ref_depth, int32_t H, int32_t W, const float* const* src_depth, const int32_t* src_hw,
                          const double* mats, int32_t S, double geo_pixel_thres, double geo_depth_thres, int32_t geo_mask_thres,
                          int32_t* mask_sum, uint8_t* mask, double* depth_avg, uint8_t* pair_masks, ufr_stream stream) {
  const char* who = "ufr_depth_consistency";
  UFR_REQUIRE(ref_depth && src_depth && src_hw && mats && mask_sum && mask && depth_avg, "%s: null argument", who);
  UFR_CHECK(depth_image_check(who, H, W));
  UFR_REQUIRE(S >= 1 && S <= UFR_DEPTH_MAX_SOURCES, "%s: S %d (must be 1 .. %d)", who, S, UFR_DEPTH_MAX_SOURCES);
  for (int k = 0; k < S; ++k) {
    UFR_REQUIRE(src_depth[k], "%s: null argument (source %d)", who, k);
    UFR_REQUIRE(src_hw[2 * k] >= 1 && src_hw[2 * k + 1] >= 1 && (long long)src_hw[2 * k] * src_hw[2 * k + 1] < (1ll << 31),
                "%s: source %d is %dx%d (H and W must be >= 1, fewer than 2^31 pixels)", who, k, src_hw[2 * k], src_hw[2 * k + 1]);
  }
  UFR_REQUIRE(!std::isnan(geo_pixel_thres) && !std::isnan(geo_depth_thres), "%s: a threshold is NaN", who);
  hipStream_t s = static_cast<hipStream_t>(stream);
  UFR_TIMED("depth_consistency", s, launch_depth_consistency(ref_depth, H, W, src_depth, src_hw, mats, S, geo_pixel_thres,
      (float)geo_depth_thres, geo_mask_thres, mask_sum, mask, depth_avg, pair_masks, s));
  return UFR_OK;
}

size_t ufr_depth_points_workspace_bytes(int32_t H, int32_t W) {
  if (H < 1 || W < 1 || (long long)H * W >= (1ll << 31)) return 0;
  return carved_bytes(carve_scan, (size_t)depth_points_blocks((long long)H * W));
}

int ufr_depth_points_count(const uint8_t* mask, int32_t H, int32_t W, void* workspace, size_t workspace_bytes, int64_t* n_host,
                           ufr_stream stream) {
  ScanWs w;
  UFR_CHECK(depth_points_check("ufr_depth_points_count", mask, H, W, workspace, workspace_bytes, &w));
  UFR_REQUIRE(n_host, "ufr_depth_points_count: null argument (n_host)");
  hipStream_t s = static_cast<hipStream_t>(stream);
  UFR_TIMED("depth_points_count", s, launch_depth_points_count(mask, (long long)H * W, w.block_tot, w.block_off, w.total, s));
  long long tot = 0;
  UFR_CHECK(read_counts(&tot, w.total, 1, s));
  *n_host = (int64_t)tot;
  return UFR_OK;
}

int ufr_depth_points_emit(const uint8_t* mask, const double* depth_avg, const uint8_t* color, int32_t H, int32_t W,
                          const double* inv_k, const double* inv_e, void* workspace, size_t workspace_bytes, float* xyz,
                          uint8_t* rgb, int64_t capacity, ufr_stream stream) {
  const char* who = "ufr_depth_points_emit";
  ScanWs w;
  UFR_CHECK(depth_points_check(who, mask, H, W, workspace, workspace_bytes, &w));
  UFR_REQUIRE(depth_avg && color && inv_k && inv_e, "%s: null argument", who);
  UFR_REQUIRE(capacity >= 0, "%s: capacity %lld", who, (long long)capacity);
  UFR_REQUIRE(capacity == 0 || (xyz && rgb), "%s: null argument (xyz / rgb with capacity %lld)", who, (long long)capacity);
  hipStream_t s = static_cast<hipStream_t>(stream);
  long long tot = 0;
  UFR_CHECK(read_counts(&tot, w.total, 1, s));
  UFR_REQUIRE(tot >= 0 && tot <= (long long)H * W, "%s: the workspace holds no count (call ufr_depth_points_count first)", who);
  UFR_REQUIRE(capacity >= tot, "%s: capacity %lld is smaller than the %lld points counted", who, (long long)capacity, tot);
  if (tot == 0) return UFR_OK;
  UFR_TIMED("depth_points_emit", s, launch_depth_points_emit(mask, depth_avg, color, H, W, inv_k, inv_e, w.block_off, xyz, rgb, tot, s));
  return UFR_OK;
}

// ------------------------------------------------------------------ point-cloud rendering
size_t ufr_splat_frames_workspace_bytes(int32_t H, int32_t W) {
  if (H < 1 || W < 1 || (long long)H * W >= (1ll << 31)) return 0;
  return carved_bytes(carve_splat_frames, (long long)H * W);
}

int ufr_splat_frames(const double* points, int64_t N, const uint8_t* colors, const double* k, const double* w2c, int32_t n_frames,
                     int32_t H, int32_t W, int32_t radius, double z_min, const float* base_color, const uint8_t* background,
                     double edl_strength, int32_t edl_radius, uint8_t* image, float* depth, int32_t* point_id, void* workspace,
                     size_t workspace_bytes, ufr_stream stream) {
  const char* who = "ufr_splat_frames";
  UFR_REQUIRE(points && k && w2c && image && workspace, "%s: null argument", who);
  UFR_REQUIRE(N >= 1 && N <= (1ll << 32) - 2, "%s: N %lld (must be 1 .. 2^32 - 2)", who, (long long)N);
  UFR_REQUIRE(!point_id || N <= kChMax, "%s: N %lld with a point-id image (must be 1 .. 2^31 - 1)", who, (long long)N);
  UFR_REQUIRE(n_frames >= 1, "%s: n_frames %d (must be >= 1)", who, n_frames);
  UFR_CHECK(depth_image_check(who, H, W));
  UFR_REQUIRE(radius >= 0 && radius <= 4, "%s: radius %d (must be 0 .. 4)", who, radius);
  UFR_REQUIRE(edl_radius >= 1, "%s: edl_radius %d (must be >= 1)", who, edl_radius);
  UFR_REQUIRE(edl_strength >= 0.0 && std::isfinite(edl_strength), "%s: edl_strength %g (must be >= 0 and finite)", who, edl_strength);
  UFR_REQUIRE(z_min >= 0.0 && std::isfinite(z_min), "%s: z_min %g (must be >= 0 and finite)", who, z_min);
  double base[3];
  unsigned char bg[3];
  UFR_CHECK(frame_colors(who, base_color, background, base, bg));
  Carver cv(workspace);
  unsigned long long* keys = carve_splat_frames(cv, (long long)H * W);
  UFR_REQUIRE(workspace_bytes >= cv.off, "%s: workspace too small: %zu < %zu bytes", who, workspace_bytes, cv.off);
  for (int i = 0; i < 9; ++i) UFR_REQUIRE(std::isfinite(k[i]), "%s: k is not finite", who);
  for (int32_t f = 0; f < n_frames; ++f) {   // all, before any launch
    const double* m = w2c + 16 * (size_t)f;
    for (int i = 0; i < 16; ++i) UFR_REQUIRE(std::isfinite(m[i]), "%s: frame %d: w2c is not finite", who, f);
    const double r3[9] = {m[0], m[1], m[2], m[4], m[5], m[6], m[8], m[9], m[10]};
    double inv[9];
    UFR_REQUIRE(invert3(r3, inv), "%s: frame %d: w2c is singular", who, f);
  }
  const size_t px = (size_t)H * W;
  hipStream_t s = static_cast<hipStream_t>(stream);
  for (int32_t f = 0; f < n_frames; ++f) {   // launches only: the cameras travel as kernel arguments, nothing waits for a frame
    UFR_TIMED("splat", s, launch_splat(points, N, k, w2c + 16 * (size_t)f, H, W, radius, z_min, keys, s));
    UFR_TIMED("splat_resolve", s, launch_splat_resolve(keys, N, colors, base, bg, edl_strength, edl_radius, H, W, image + 3 * px * f,
        depth ? depth + px * f : nullptr, point_id ? point_id + px * f : nullptr, s));
  }
  return UFR_OK;
}

}  // extern "C"

// ------------------------------------------------------------------ Poisson surface reconstruction
namespace {

int poisson_dims_check(const char* who, const int32_t* dims) {
  UFR_REQUIRE(dims, "%s: null argument (dims)", who);
  UFR_REQUIRE(dims[0] >= 2 && dims[1] >= 2 && dims[2] >= 2, "%s: grid %dx%dx%d (every dim must be >= 2)", who, dims[0], dims[1],
              dims[2]);
  UFR_REQUIRE((long long)dims[0] * dims[1] * dims[2] < (1ll << 31), "%s: grid %dx%dx%d has 2^31 nodes or more", who, dims[0], dims[1],
              dims[2]);
  return UFR_OK;
}

int poisson_grid_check(const char* who, const int32_t* dims, const double* origin, double h) {
  UFR_CHECK(poisson_dims_check(who, dims));
  UFR_REQUIRE(origin, "%s: null argument (origin)", who);
  return cell_grid_check(who, h, origin);
}

int poisson_h_check(const char* who, double h) {
  UFR_REQUIRE(h > 0.0 && std::isfinite(h) && std::isfinite(1.0 / (h * h)) && h * h > 0.0, "%s: h %g (must be positive and finite, and so must h^2)", who, h);
  return UFR_OK;
}

// solver: [r | p | q, one volume each | partials of p.q | partials of r.r | state fp64 x 4]
struct PoissonWs { double *r, *p, *q, *pq_part, *rr_part, *state; };
PoissonWs carve_poisson(Carver& c, long long n) {
  PoissonWs w;
  w.r = c.take<double>((size_t)n);
  w.p = c.take<double>((size_t)n);
  w.q = c.take<double>((size_t)n);
  w.pq_part = c.take<double>(kPsMaxBlocks);
  w.rr_part = c.take<double>(kPsMaxBlocks);
  w.state = c.take<double>(4);
  return w;
}

// samples: [partials fp64]
double* carve_poisson_sample(Carver& c) { return c.take<double>(kPsMaxBlocks); }

bool poisson_dims_ok(const int32_t* dims) {
  return dims && dims[0] >= 2 && dims[1] >= 2 && dims[2] >= 2 && (long long)dims[0] * dims[1] * dims[2] < (1ll << 31);
}

}  // namespace

extern "C" {

int ufr_poisson_grid(const double* bound_min, const double* bound_max, int32_t resolution, int32_t pad, double* origin, double* h,
                     int32_t* dims) {
  const char* who = "ufr_poisson_grid";
  UFR_REQUIRE(bound_min && bound_max && origin && h && dims, "%s: null argument", who);
  UFR_REQUIRE(resolution >= 4, "%s: resolution %d (must be >= 4)", who, resolution);
  UFR_REQUIRE(pad >= 2, "%s: pad %d (must be >= 2: the splat and the central differences stay inside the grid)", who, pad);
  double extent = 0.0;
  for (int a = 0; a < 3; ++a) {
    UFR_REQUIRE(std::isfinite(bound_min[a]) && std::isfinite(bound_max[a]), "%s: the bounds are not finite (axis %d: %g .. %g)", who, a,
                bound_min[a], bound_max[a]);
    UFR_REQUIRE(bound_max[a] >= bound_min[a], "%s: axis %d: max %g < min %g", who, a, bound_max[a], bound_min[a]);
    const double e = bound_max[a] - bound_min[a];
    if (e > extent) extent = e;
  }
  const double hh = extent / (double)resolution;
  UFR_REQUIRE(hh > 0.0 && std::isfinite(hh) && hh * hh > 0.0 && std::isfinite(1.0 / (hh * hh)),
              "%s: degenerate extent %g (the samples span no axis, or h^2 leaves the fp64 range)", who, extent);
  long long d[3], nodes = 1;
  for (int a = 0; a < 3; ++a) {
    d[a] = (long long)ceil((bound_max[a] - bound_min[a]) / hh) + 1 + 2ll * pad;
    UFR_REQUIRE(d[a] < (1ll << 31), "%s: %lld nodes on axis %d", who, d[a], a);
    nodes *= d[a];
    UFR_REQUIRE(nodes < (1ll << 31), "%s: resolution %d, pad %d: 2^31 nodes or more", who, resolution, pad);
  }
  for (int a = 0; a < 3; ++a) {
    origin[a] = bound_min[a] - (double)pad * hh;
    dims[a] = (int32_t)d[a];
  }
  *h = hh;
  return UFR_OK;
}

int ufr_poisson_splat_keys(const double* points, int64_t n, const double* origin, double h, const int32_t* dims, int64_t* keys,
                           ufr_stream stream) {
  const char* who = "ufr_poisson_splat_keys";
  UFR_REQUIRE(points && keys, "%s: null argument", who);
  UFR_REQUIRE(n >= 1 && n < (1ll << 28), "%s: n %lld (must be 1 .. 2^28 - 1)", who, (long long)n);
  UFR_CHECK(poisson_grid_check(who, dims, origin, h));
  hipStream_t s = static_cast<hipStream_t>(stream);
  UFR_TIMED("poisson_splat_keys", s, launch_poisson_splat_keys(points, n, origin, h, dims, reinterpret_cast<long long*>(keys), s));
  return UFR_OK;
}

int ufr_poisson_splat(const double* points, const double* normals, int64_t n, const double* origin, double h, const int32_t* dims,
                      const int64_t* keys, const int64_t* rows, double* V, double* W, ufr_stream stream) {
  const char* who = "ufr_poisson_splat";
  UFR_REQUIRE(points && normals && keys && rows && V && W, "%s: null argument", who);
  UFR_REQUIRE(n >= 1 && n < (1ll << 28), "%s: n %lld (must be 1 .. 2^28 - 1)", who, (long long)n);
  UFR_CHECK(poisson_grid_check(who, dims, origin, h));
  hipStream_t s = static_cast<hipStream_t>(stream);
  UFR_TIMED("poisson_splat", s, launch_poisson_splat_sum(points, normals, n, origin, h, dims, reinterpret_cast<const long long*>(keys),
      reinterpret_cast<const long long*>(rows), V, W, s));
  return UFR_OK;
}

int ufr_poisson_divergence(const double* V, const int32_t* dims, double h, double* b, ufr_stream stream) {
  const char* who = "ufr_poisson_divergence";
  UFR_REQUIRE(V && b, "%s: null argument", who);
  UFR_CHECK(poisson_dims_check(who, dims));
  UFR_CHECK(poisson_h_check(who, h));
  hipStream_t s = static_cast<hipStream_t>(stream);
  UFR_TIMED("poisson_divergence", s, launch_poisson_divergence(V, dims, h, b, s));
  return UFR_OK;
}

int ufr_poisson_laplacian(const double* p, const int32_t* dims, double h, double* q, ufr_stream stream) {
  const char* who = "ufr_poisson_laplacian";
  UFR_REQUIRE(p && q && p != q, "%s: null argument, or q aliases p", who);
  UFR_CHECK(poisson_dims_check(who, dims));
  UFR_CHECK(poisson_h_check(who, h));
  hipStream_t s = static_cast<hipStream_t>(stream);
  UFR_TIMED("poisson_laplacian", s, launch_poisson_laplace(p, dims, h, q, nullptr, s));
  return UFR_OK;
}

size_t ufr_poisson_workspace_bytes(const int32_t* dims) {
  return poisson_dims_ok(dims) ? carved_bytes(carve_poisson, (long long)dims[0] * dims[1] * dims[2]) : 0;
}

int ufr_poisson_solve(const double* b, const int32_t* dims, double h, double tol, int32_t max_iter, int32_t check_every, double* x,
                      void* workspace, size_t workspace_bytes, int32_t* iterations_host, double* residual_host,
                      int32_t* converged_host, ufr_stream stream) {
  const char* who = "ufr_poisson_solve";
  UFR_REQUIRE(b && x && workspace && iterations_host && residual_host && converged_host, "%s: null argument", who);
  UFR_CHECK(poisson_dims_check(who, dims));
  UFR_CHECK(poisson_h_check(who, h));
  UFR_REQUIRE(tol >= 0.0 && std::isfinite(tol), "%s: tol %g (must be >= 0 and finite)", who, tol);
  UFR_REQUIRE(max_iter >= 1 && check_every >= 1, "%s: max_iter %d, check_every %d (each must be >= 1)", who, max_iter, check_every);
  const long long n = (long long)dims[0] * dims[1] * dims[2];
  Carver c(workspace);
  const PoissonWs w = carve_poisson(c, n);
  UFR_CHECK(check_workspace(who, workspace_bytes, c.off));
  hipStream_t s = static_cast<hipStream_t>(stream);
  UFR_TIMED("poisson_cg_init", s, launch_poisson_cg_init(b, n, x, w.r, w.p, w.rr_part, w.state, s));
  double rr = 0.0;
  UFR_HIP(hipMemcpyAsync(&rr, w.state, sizeof(double), hipMemcpyDeviceToHost, s));
  UFR_HIP(hipStreamSynchronize(s));
  UFR_REQUIRE(std::isfinite(rr), "%s: b.b = %g (b holds values that are not finite, or its square sum leaves the fp64 range)", who, rr);
  const double bnorm = sqrt(rr);
  int it = 0, conv = 0;
  if (rr == 0.0) {           // b = 0: x = 0 is the answer, and no quotient is formed
    conv = 1;
  } else {
    int slot = 0;
    while (it < max_iter && !conv) {
      UFR_TIMED("poisson_cg_iteration", s, launch_poisson_cg_iteration(dims, h, x, w.r, w.p, w.q, w.pq_part, w.rr_part, w.state, slot, s));
      slot ^= 1;
      ++it;
      if (it % check_every == 0 || it == max_iter) {       // the look: one 8-byte copy, one synchronisation
        UFR_HIP(hipMemcpyAsync(&rr, w.state + slot, sizeof(double), hipMemcpyDeviceToHost, s));
        UFR_HIP(hipStreamSynchronize(s));
        if (!(rr == rr)) return fail(UFR_ERR_HIP, "%s: the residual became NaN at iteration %d", who, it);
        conv = sqrt(rr) <= tol * bnorm;
      }
    }
  }
  *iterations_host = it;
  *residual_host = bnorm > 0.0 ? sqrt(rr) / bnorm : 0.0;
  *converged_host = conv;
  return UFR_OK;
}

size_t ufr_poisson_sample_workspace_bytes(int64_t n) {
  return (n >= 1 && n <= kChMax) ? carved_bytes(carve_poisson_sample) : 0;
}

int ufr_poisson_sample(const double* vol, const int32_t* dims, const double* origin, double h, const double* points, int64_t n,
                       double* values, double* mean_out, void* workspace, size_t workspace_bytes, ufr_stream stream) {
  const char* who = "ufr_poisson_sample";
  UFR_REQUIRE(vol && points && values && workspace, "%s: null argument", who);
  UFR_REQUIRE(n >= 1 && n <= kChMax, "%s: n %lld (must be 1 .. 2^31 - 1)", who, (long long)n);
  UFR_CHECK(poisson_grid_check(who, dims, origin, h));
  Carver c(workspace);
  double* part = carve_poisson_sample(c);
  UFR_CHECK(check_workspace(who, workspace_bytes, c.off));
  hipStream_t s = static_cast<hipStream_t>(stream);
  UFR_TIMED("poisson_sample", s, launch_poisson_sample(vol, dims, origin, h, points, n, values, mean_out, part, s));
  return UFR_OK;
}

}  // extern "C"
