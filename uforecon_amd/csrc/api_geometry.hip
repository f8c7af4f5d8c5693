// extern "C" surface of libufr.so (include/ufr.h), part 6 of 7: geometry after the network -- TSDF fusion, marching cubes,
// the similarity field, the DTU chamfer evaluation, point-cloud filtering, depth-map fusion, mesh cleaning, mesh rendering and point-cloud rendering.  The count / emit pairs synchronise the
// stream to hand a count to the host; so do the rounds of the two fixpoints (point thinning, face components).
#include "api_common.h"
#include "mcubes_table.h"

using namespace ufr;
using namespace ufr::api;

namespace {

// the counts a scan left in a workspace, on the host: the one synchronisation of a count / emit pair
int read_counts(long long* host, const long long* dev, int n, hipStream_t s) {
  UFR_HIP(hipMemcpyAsync(host, dev, n * sizeof(long long), hipMemcpyDeviceToHost, s));
  UFR_HIP(hipStreamSynchronize(s));
  return UFR_OK;
}

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
constexpr long long kChMax = (1ll << 31) - 1;

int cell_grid_check(const char* who, double cell, const double* origin) {
  UFR_REQUIRE(cell > 0.0 && std::isfinite(cell) && std::isfinite(origin[0]) && std::isfinite(origin[1]) && std::isfinite(origin[2]),
              "%s: cell %g, origin (%g, %g, %g) (cell must be positive, all finite)", who, cell, origin[0], origin[1], origin[2]);
  return UFR_OK;
}

// mesh sampling: [per-triangle offset in its block int64 | block sums int64 | block offsets int64 | total int64]
struct SampleWs { long long *tri_off, *block_tot, *block_off, *total; };
SampleWs carve_mesh_sample(Carver& c, long long F) {
  const size_t blocks = (size_t)chamfer_blocks(F);
  SampleWs w;
  w.tri_off = c.take<long long>((size_t)F);
  w.block_tot = c.take<long long>(blocks);
  w.block_off = c.take<long long>(blocks);
  w.total = c.take<long long>(1);
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

// ---- point-cloud filtering, voxel means: [run heads per block int64 | block offsets int64 | total int64]
struct VoxelWs { long long *block_tot, *block_off, *total; };
VoxelWs carve_voxel_mean(Carver& c, long long n) {
  const size_t blocks = (size_t)points_filter_blocks(n);
  VoxelWs w;
  w.block_tot = c.take<long long>(blocks);
  w.block_off = c.take<long long>(blocks);
  w.total = c.take<long long>(1);
  return w;
}

// ---- depth-map fusion: [block sums int64 | block offsets int64 | total int64]
struct DepthPointsWs { long long *block_tot, *block_off, *total; };
DepthPointsWs carve_depth_points(Carver& c, long long n) {
  const size_t blocks = (size_t)depth_points_blocks(n);
  DepthPointsWs w;
  w.block_tot = c.take<long long>(blocks);
  w.block_off = c.take<long long>(blocks);
  w.total = c.take<long long>(1);
  return w;
}

int depth_image_check(const char* who, int32_t H, int32_t W) {
  UFR_REQUIRE(H >= 1 && W >= 1, "%s: image %dx%d (H and W must be >= 1)", who, H, W);
  UFR_REQUIRE((long long)H * W < (1ll << 31), "%s: image %dx%d has 2^31 pixels or more", who, H, W);
  return UFR_OK;
}

int depth_points_check(const char* who, const uint8_t* mask, int32_t H, int32_t W, void* ws, size_t ws_bytes, DepthPointsWs* w) {
  UFR_REQUIRE(mask && ws, "%s: null argument", who);
  UFR_CHECK(depth_image_check(who, H, W));
  Carver c(ws);
  *w = carve_depth_points(c, (long long)H * W);
  return check_workspace(who, ws_bytes, c.off);
}

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

// point-cloud rendering: [key image uint64 per pixel]
unsigned long long* carve_splat_frames(Carver& c, long long pixels) { return c.take<unsigned long long>((size_t)pixels); }

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

bool invert3(const double* m, double* o) {
  const double c0 = m[4] * m[8] - m[5] * m[7], c1 = m[5] * m[6] - m[3] * m[8], c2 = m[3] * m[7] - m[4] * m[6];
  const double det = m[0] * c0 + m[1] * c1 + m[2] * c2;
  if (!(det != 0.0) || !std::isfinite(det)) return false;
  o[0] = c0 / det, o[1] = (m[2] * m[7] - m[1] * m[8]) / det, o[2] = (m[1] * m[5] - m[2] * m[4]) / det;
  o[3] = c1 / det, o[4] = (m[0] * m[8] - m[2] * m[6]) / det, o[5] = (m[2] * m[3] - m[0] * m[5]) / det;
  o[6] = c2 / det, o[7] = (m[1] * m[6] - m[0] * m[7]) / det, o[8] = (m[0] * m[4] - m[1] * m[3]) / det;
  for (int i = 0; i < 9; ++i)
    if (!std::isfinite(o[i])) return false;
  return true;
}

// rot, org of a host fp32 c2w, and the fp64 inverse of the fp32 ray generator: pixel ~ inv(k_inv) inv(R) (X - o)
int hit_camera(const char* who, const float* k_inv, const float* c2w, float* rot, float* org, double* proj) {
  double ki[9], r[9], kf[9], rw[9], m[9];
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) rot[3 * i + j] = c2w[4 * i + j], r[3 * i + j] = (double)c2w[4 * i + j], ki[3 * i + j] = (double)k_inv[3 * i + j];
    org[i] = c2w[4 * i + 3];
  }
  UFR_REQUIRE(invert3(ki, kf) && invert3(r, rw), "%s: k_inv or the rotation of c2w is singular or not finite", who);
  UFR_REQUIRE(std::isfinite(org[0]) && std::isfinite(org[1]) && std::isfinite(org[2]), "%s: the camera centre is not finite", who);
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) m[3 * i + j] = kf[3 * i] * rw[j] + kf[3 * i + 1] * rw[3 + j] + kf[3 * i + 2] * rw[6 + j];
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) proj[4 * i + j] = m[3 * i + j];
    proj[4 * i + 3] = -(m[3 * i] * (double)org[0] + m[3 * i + 1] * (double)org[1] + m[3 * i + 2] * (double)org[2]);
  }
  return UFR_OK;
}

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
  UFR_TIMED("mesh_sample_count", s, launch_mesh_sample_count(verts, faces, V, F, density, w.tri_off, w.block_tot, s));
  UFR_TIMED("mesh_sample_scan", s, launch_mesh_sample_scan(w.block_tot, chamfer_blocks(F), w.block_off, w.total, s));
  long long tot = 0;
  UFR_CHECK(read_counts(&tot, w.total, 1, s));
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
  UFR_TIMED("mesh_sample_emit", s, launch_mesh_sample_emit(verts, faces, V, F, density, w.tri_off, w.block_off, out, capacity, s));
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
  return (n >= 1 && n <= kChMax) ? carved_bytes(carve_voxel_mean, (long long)n) : 0;
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
  const VoxelWs w = carve_voxel_mean(c, n);
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
  return carved_bytes(carve_depth_points, (long long)H * W);
}

int ufr_depth_points_count(const uint8_t* mask, int32_t H, int32_t W, void* workspace, size_t workspace_bytes, int64_t* n_host,
                           ufr_stream stream) {
  DepthPointsWs w;
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
  DepthPointsWs w;
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
  UFR_REQUIRE(V >= 1 && V <= kChMax && F >= 1 && F <= kChMax / 3, "%s: V %lld, F %lld (V must be 1 .. 2^31 - 1, F 1 .. (2^31 - 1) / 3)",
              who, (long long)V, (long long)F);
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
  UFR_REQUIRE(V >= 1 && V <= kChMax && F >= 1 && F <= kChMax / 3, "%s: V %lld, F %lld (V must be 1 .. 2^31 - 1, F 1 .. (2^31 - 1) / 3)",
              who, (long long)V, (long long)F);
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
  const char* who = "ufr_raster_frames";
  UFR_REQUIRE(verts && faces && k_inv && c2w && image && workspace, "%s: null argument", who);
  UFR_REQUIRE(V >= 1 && V <= kChMax && F >= 1 && F <= kChMax, "%s: V %lld, F %lld (each must be 1 .. 2^31 - 1)", who, (long long)V,
              (long long)F);
  UFR_REQUIRE(n_frames >= 1, "%s: n_frames %d (must be >= 1)", who, n_frames);
  UFR_CHECK(depth_image_check(who, H, W));
  UFR_REQUIRE(ambient >= 0.0 && ambient <= 1.0, "%s: ambient %g (must be 0 .. 1)", who, ambient);
  double base[3] = {1.0, 1.0, 1.0};
  unsigned char bg[3] = {255, 255, 255};
  for (int k = 0; k < 3; ++k) {
    if (base_color) base[k] = (double)base_color[k];
    if (background) bg[k] = background[k];
    UFR_REQUIRE(base[k] >= 0.0 && base[k] <= 1.0, "%s: base colour %g (must be 0 .. 1)", who, base[k]);
  }
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
        normal_map ? normal_map + 3 * px * i : nullptr, s));
  }
  return UFR_OK;
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
  double base[3] = {1.0, 1.0, 1.0};
  unsigned char bg[3] = {255, 255, 255};
  for (int c = 0; c < 3; ++c) {
    if (base_color) base[c] = (double)base_color[c];
    if (background) bg[c] = background[c];
    UFR_REQUIRE(base[c] >= 0.0 && base[c] <= 1.0, "%s: base colour %g (must be 0 .. 1)", who, base[c]);
  }
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

// ------------------------------------------------------------------ mesh colouring
// [camera table: one MeshColorCam per view]
MeshColorCam* carve_mesh_colors(Carver& c, int n_views) { return c.take<MeshColorCam>((size_t)n_views); }

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
  UFR_REQUIRE(n_views >= 1 && n_views <= UFR_MESH_MAX_VIEWS, "%s: n_views %d (must be 1 .. %d)", who, n_views, UFR_MESH_MAX_VIEWS);
  UFR_REQUIRE(H >= 2 && W >= 2, "%s: image %dx%d (H and W must be >= 2)", who, H, W);
  UFR_CHECK(depth_image_check(who, H, W));
  UFR_REQUIRE(z_min >= 0.0 && std::isfinite(z_min), "%s: z_min %g (must be >= 0 and finite)", who, z_min);
  UFR_REQUIRE(depth_tol >= 0.0 && std::isfinite(depth_tol), "%s: depth_tol %g (must be >= 0 and finite)", who, depth_tol);
  UFR_REQUIRE(min_cos >= 0.0 && min_cos <= 1.0, "%s: min_cos %g (must be 0 .. 1)", who, min_cos);
  UFR_REQUIRE(power >= 0 && power <= UFR_MESH_COLOR_MAX_POWER, "%s: power %d (must be 0 .. %d)", who, power, UFR_MESH_COLOR_MAX_POWER);
  UFR_REQUIRE(mode == UFR_MESH_COLOR_MEAN || mode == UFR_MESH_COLOR_BEST, "%s: unknown mode %d", who, mode);
  Carver cv(workspace);
  MeshColorCam* table = carve_mesh_colors(cv, n_views);
  UFR_REQUIRE(workspace_bytes >= cv.off, "%s: workspace too small: %zu < %zu bytes", who, workspace_bytes, cv.off);
  MeshColorCam cams[UFR_MESH_MAX_VIEWS];
  for (int32_t f = 0; f < n_views; ++f) {   // all, before any launch
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
  UFR_REQUIRE(V >= 1 && V <= kChMax && F >= 1 && F <= kChMax / 3, "%s: V %lld, F %lld (V must be 1 .. 2^31 - 1, F 1 .. (2^31 - 1) / 3)",
              who, (long long)V, (long long)F);
  UFR_REQUIRE(colors_out != colors_in && state_out != state_in, "%s: the round is double-buffered: out must not alias in", who);
  hipStream_t s = static_cast<hipStream_t>(stream);
  UFR_TIMED("mesh_color_fill_round", s, launch_mesh_color_fill_round(faces, V, F, reinterpret_cast<const long long*>(sorted_slots),
      reinterpret_cast<const long long*>(run_starts), colors_in, state_in, colors_out, state_out, filled, s));
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

// ------------------------------------------------------------------ mesh simplification
namespace {

// every scanning call: [flags per block int64 | block offsets int64 | total int64]
struct SimplifyWs { long long *block_tot, *block_off, *total; };
SimplifyWs carve_simplify(Carver& c, long long n) {
  const size_t blocks = (size_t)simplify_blocks(n);
  SimplifyWs w;
  w.block_tot = c.take<long long>(blocks);
  w.block_off = c.take<long long>(blocks);
  w.total = c.take<long long>(1);
  return w;
}

int simplify_counts_check(const char* who, int64_t V, int64_t F) {
  UFR_REQUIRE(V >= 1 && V <= kChMax && F >= 1 && F <= kChMax, "%s: V %lld, F %lld (each must be 1 .. 2^31 - 1)", who, (long long)V,
              (long long)F);
  return UFR_OK;
}

}  // namespace

extern "C" {

size_t ufr_simplify_workspace_bytes(int64_t n) { return (n >= 1 && n <= kChMax) ? carved_bytes(carve_simplify, (long long)n) : 0; }

int ufr_simplify_clusters(const int64_t* sorted_keys, const int64_t* order, int64_t V, int32_t* cluster, int64_t* cluster_key,
                          int64_t capacity, void* workspace, size_t workspace_bytes, int64_t* total_host, ufr_stream stream) {
  const char* who = "ufr_simplify_clusters";
  UFR_REQUIRE(sorted_keys && order && cluster && cluster_key && workspace && total_host, "%s: null argument", who);
  UFR_REQUIRE(V >= 1 && V <= kChMax, "%s: V %lld (must be 1 .. 2^31 - 1)", who, (long long)V);
  UFR_REQUIRE(capacity >= 0, "%s: capacity %lld", who, (long long)capacity);
  Carver c(workspace);
  const SimplifyWs w = carve_simplify(c, V);
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
  const SimplifyWs w = carve_simplify(c, F);
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
  const SimplifyWs w = carve_simplify(c, C);
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

}  // extern "C"

// ------------------------------------------------------------------ mesh smoothing
namespace {

// [neighbour pairs int32 (3F,2) | weight pairs fp64 (3F,2), cotangent weights only], both in row order
struct SmoothWs { int* nbr; double* wgt; };
SmoothWs carve_mesh_smooth(Carver& c, long long F, int weights) {
  SmoothWs w;
  w.nbr = c.take<int>((size_t)(6 * F));
  w.wgt = weights == UFR_SMOOTH_COTANGENT ? c.take<double>((size_t)(6 * F)) : nullptr;
  return w;
}

int smooth_check(const char* who, int64_t V, int64_t F, int32_t weights) {
  UFR_REQUIRE(V >= 1 && V <= kChMax && F >= 1 && F <= kChMax / 3, "%s: V %lld, F %lld (V must be 1 .. 2^31 - 1, F 1 .. (2^31 - 1) / 3)",
              who, (long long)V, (long long)F);
  UFR_REQUIRE(weights == UFR_SMOOTH_UNIFORM || weights == UFR_SMOOTH_COTANGENT, "%s: unknown weights %d", who, weights);
  return UFR_OK;
}

}  // namespace

extern "C" {

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
  for (int i = 0; i < n_steps; ++i)
    UFR_TIMED("mesh_smooth_step", s, launch_mesh_smooth_step(V, F, reinterpret_cast<const long long*>(run_starts), w.nbr, w.wgt, border,
        pinned, factors[i], (i & 1) ? pos_b : pos_a, (i & 1) ? pos_a : pos_b, s));
  return UFR_OK;
}

}  // extern "C"

// ------------------------------------------------------------------ mesh denoising
namespace {

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

int denoise_check(const char* who, int64_t V, int64_t F) {
  UFR_REQUIRE(V >= 1 && V <= kChMax && F >= 1 && F <= kChMax / 3, "%s: V %lld, F %lld (V must be 1 .. 2^31 - 1, F 1 .. (2^31 - 1) / 3)",
              who, (long long)V, (long long)F);
  return UFR_OK;
}

}  // namespace

extern "C" {

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
  UFR_CHECK(denoise_check(who, V, F));
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
  UFR_CHECK(denoise_check(who, V, F));
  UFR_REQUIRE(std::isfinite(two_ss) && two_ss > 0.0, "%s: two_ss %g (must be finite and above 0)", who, two_ss);
  UFR_REQUIRE(std::isfinite(two_rr) && two_rr > 0.0, "%s: two_rr %g (must be finite and above 0)", who, two_rr);
  UFR_REQUIRE(n_steps >= 0, "%s: n_steps %d (must be >= 0)", who, n_steps);
  Carver c(workspace);
  const DenoiseWs w = carve_mesh_denoise(c, F);
  UFR_CHECK(check_workspace(who, workspace_bytes, c.off));
  hipStream_t s = static_cast<hipStream_t>(stream);
  for (int i = 0; i < n_steps; ++i)
    UFR_TIMED("mesh_denoise_normals", s, launch_mesh_denoise_normals(faces, V, F, reinterpret_cast<const long long*>(run_starts), w.row_face,
        two_ss, two_rr, (i & 1) ? w.rec_b : w.rec_a, (i & 1) ? w.rec_a : w.rec_b, i == n_steps - 1 ? normals : nullptr, s));
  return UFR_OK;
}

int ufr_denoise_vertices(int64_t V, int64_t F, const int64_t* run_starts, const double* normals, const uint8_t* border,
                         const uint8_t* pinned, int32_t n_steps, double* pos_a, double* pos_b, const void* workspace,
                         size_t workspace_bytes, ufr_stream stream) {
  const char* who = "ufr_denoise_vertices";
  UFR_REQUIRE(run_starts && normals && pos_a && pos_b && workspace, "%s: null argument", who);
  UFR_REQUIRE(pos_a != pos_b, "%s: pos_a and pos_b are one buffer", who);
  UFR_REQUIRE(normals != pos_a && normals != pos_b, "%s: normals and a position buffer are one buffer", who);
  UFR_CHECK(denoise_check(who, V, F));
  UFR_REQUIRE(n_steps >= 0, "%s: n_steps %d (must be >= 0)", who, n_steps);
  Carver c(const_cast<void*>(workspace));
  const DenoiseWs w = carve_mesh_denoise(c, F);
  UFR_CHECK(check_workspace(who, workspace_bytes, c.off));
  hipStream_t s = static_cast<hipStream_t>(stream);
  for (int i = 0; i < n_steps; ++i)
    UFR_TIMED("mesh_denoise_vertices", s, launch_mesh_denoise_vertices(V, F, reinterpret_cast<const long long*>(run_starts), w.rows, normals,
        border, pinned, (i & 1) ? pos_b : pos_a, (i & 1) ? pos_a : pos_b, s));
  return UFR_OK;
}

}  // extern "C"
