// Internal host/device structs behind the opaque handles of include/ufr.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <mutex>

#include "../../include/ufr.h"
#include "ufr_layout.h"

namespace ufr {

constexpr int kVolCh = 12;  // channel-last volume texel: 8 features + 1 weight + 3 pad = 48 B

// What ufr_frame_prepare records (lives inside the caller's ufr_frame; passed BY VALUE to kernels).
struct FrameDev {
  int32_t NV, H, W, h, w, match_ch;      // match_ch = 32*(NV-1)
  const float* feat;                     // [NV][h][w][32]
  const float* match;                    // [NV][h][w][match_ch]
  const float* rgb;                      // [NV][H][W][4]
  const float* depth;                    // [NV][H][W]   (borrowed, reference layout)
  const float* vol[UFR_NUM_STAGES];      // [NV][D][Hs][Ws][12]
  int32_t vD[UFR_NUM_STAGES], vH[UFR_NUM_STAGES], vW[UFR_NUM_STAGES];
  float pose[UFR_MAX_VIEWS][12];         // rows 0..2 of source_poses
  float cam_pos[UFR_MAX_VIEWS][3];
  float w2c_z[UFR_MAX_VIEWS][4];
  float ref_pos[3];
  float vol_near, vol_far;
  uint32_t magic;
  // device word: the largest |value| among the frame's feature maps and volume features, as a float's bit pattern --
  // measured by the re-layout kernels (prep.hip), consumed by ufr_weights_fit_frame
  const unsigned* abs_max;
};
static_assert(sizeof(FrameDev) <= sizeof(ufr_frame), "ufr_frame too small");
constexpr uint32_t kFrameMagic = 0x55465246u;  // "UFRF"

struct PreSim {  // pre_sim_mlp raw pointers (reference layout) used by the gather kernel
  const float *w0, *b0, *w2, *b2, *w4, *b4;
};

// hipFuncAttributeMaxDynamicSharedMemorySize is a per-device attribute of a kernel: set it once per (kernel, device),
// safely from any thread (the entry points are called from the caller's thread AND from autograd's workers).
struct LdsAttrOnce {
  std::once_flag flag[16];
  hipError_t err[16];
  hipError_t set(const void* kernel, int bytes) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 16) return hipErrorInvalidDevice;
    std::call_once(flag[dev], [&] { err[dev] = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes); });
    return err[dev];
  }
};

// kernel launchers (one per .hip file); all enqueue on `s` and return hipGetLastError()
hipError_t launch_nchw_to_nhwc(const float* in, float* out, int N, int C, int S, int Cpad, hipStream_t s, unsigned* abs_max = nullptr);
hipError_t launch_volume_pack(const float* feat, const float* weight, float* out, int N, int S, hipStream_t s, unsigned* abs_max = nullptr);
hipError_t launch_ray_setup(const int64_t* ray_idx, const float* ray_d, const float* cam_ray_d, int HW, float near_z,
                            float far_z, int RN, float* rd_out, float* near_out, float* far_out, float* camz_out,
                            const float* ray_o_host, float* ray_o_out, hipStream_t s);
hipError_t launch_sample_fixed(const float* near, const float* far, const float* U, int u_stride, float* z, int RN,
                               int SN, hipStream_t s);
hipError_t launch_importance_merge(const float* weight, const float* z, const float* U2, int u_stride, float* z_fine,
                                   float* z_all, int RN, int SN, int PN, float* z_new, int* src_row, hipStream_t s);
hipError_t launch_order_pe(float* table, int SN, hipStream_t s);
hipError_t launch_points(const float* ray_o, int o_stride, const float* ray_d, const float* z, float* pts, int RN,
                         int SN, hipStream_t s);
// Token rows.  Public layout (x_point == nullptr): x_tokens (P, NV, 80) = [feat 32 | frustum lookup 24 | pre_sim_mlp 16 |
// depth PE 8] per (point, view).  Columns 32..71 are the same for all views of a point, and writing them NV times is a
// sixth of the gather kernel's time (ablation, round 3): the whole-path entry point keeps them once per point --
// compact layout (x_point != nullptr): x_tokens (P, NV, kViewCols) = [feat 32 | depth PE 8], x_point (P, kPointCols) =
// [frustum lookup 24 | pre_sim_mlp 16].
constexpr int kViewCols = 40, kPointCols = 40;
hipError_t launch_gather(const FrameDev& f, const PreSim& ps, const float* ray_o, int o_stride, const float* ray_d,
                         const float* z, int RN, int SN, float* x_tokens, float* x_point, float* rgb, float* dir, float* sim8,
                         float* vol24, float* xy, float* mask_z, const float* vol24_in, const float* sim8_in,
                         hipStream_t s);
// lowp: matrix precision of the call (include/ufr.h): false = fp32-grade split precision, true = one 16-bit plane per
// operand ("bf16" training mode of BASELINE configs[4]).  status: the device's sticky range word (ufr_status_poll).
hipError_t launch_view_transformer(const float* packed, const float* x_tokens, const float* x_point, const float* rgb,
                                   const float* dir, int P, int NV, float* token0, float* radiance, float* view_out, bool lowp, int* status,
                                   hipStream_t s);
// tok_row / rad_row (nullable): row of token0 / radiance holding sample (ray, s) -- the fine pass of the whole-path
// renderer keeps coarse and new evaluations in one pool instead of re-evaluating the coarse points
hipError_t launch_ray_transformer(const float* packed, const float* token0, const int* tok_row, const float* order_pe,
                                  int RN, int SN, float* srdf, float* ray_out, bool lowp, int* status, hipStream_t s);
hipError_t launch_composite(const float* z, const float* radiance, const int* rad_row, const float* srdf,
                            const float* variance, int RN, int SN, float* rgb, float* depth, float* opacity, float* weight,
                            const float* camz, float* depth_z, hipStream_t s);
// render_loss.hip: the training loss of a ray batch and its cotangents (model.py:552-566), one launch
hipError_t launch_render_loss(const float* rgb_c, const float* depth_c, const float* rgb_f, const float* depth_f,
                              const float* rgb_gt, const float* depth_gt, const float* near_far, int nf_stride, int B, int RN,
                              float weight_rgb, float weight_depth, float* loss, float* d_rgb_c, float* d_depth_c,
                              float* d_rgb_f, float* d_depth_f, hipStream_t s);
hipError_t launch_composite_bwd(const float* z, const float* radiance, const int* rad_row, bool accumulate, const float* srdf,
                                const float* variance, int RN, int SN, const float* d_rgb, const float* d_depth,
                                const float* d_opacity, const float* d_weight, float* d_radiance, float* d_srdf,
                                float* d_variance, hipStream_t s);
// one gradient tensor per parameter, in the reference layout (= ufr_raw_grads); the backward kernels add into them
struct GradPtrs { float* p[P_COUNT]; };
__device__ __forceinline__ void atomic_add_f32(float* p, float v) { unsafeAtomicAdd(p, v); }
// The streaming view-transformer backward (round 4; bwd_tape.h): the forward again with a tape, the data-gradient chain,
// the weight-gradient contraction.  tape: view_tape_blocks(P, NV) blocks of TV_COUNT tiles; dbuf: as many blocks of DV_COUNT.
int view_tape_blocks(int P, int NV);
hipError_t launch_view_tape(const float* packed, const float* x_tokens, const float* rgb, const float* dir, int P, int NV,
                            float* token0, float* radiance, float* tape, bool lowp, int* status, hipStream_t s);
hipError_t launch_view_dgrad(const float* packed, const float* tape, const float* rgbm, const float* d_tok_a,
                             const float* d_tok_b, const float* d_radiance, int P, int NV, float* dbuf, float* d_pv,
                             const GradPtrs& gp, bool lowp, hipStream_t s);
hipError_t launch_view_wgrad(const float* tape, const float* dbuf, int n_blocks, const GradPtrs& gp, bool lowp, hipStream_t s);
// ... and the ray transformer's: tape = RN x ceil(SN / 32) blocks of RT_COUNT tiles, ray_state = RN x kRayStateTiles tiles,
// dbuf = as many blocks of DR_COUNT tiles.  d_tok_a receives the whole gradient (rows through tok_row, += when accumulate),
// d_tok_b (nullable) is zero-filled when not accumulating: the two-buffer form of the former kernel's interface.
hipError_t launch_ray_tape(const float* packed, const float* token0, const int* tok_row, const float* order_pe, int RN, int SN,
                           float* srdf, float* tape, float* ray_state, bool lowp, int* status, hipStream_t s);
hipError_t launch_ray_dgrad(const float* packed, const float* tape, const float* ray_state, const float* d_srdf, const int* tok_row,
                            bool accumulate, int RN, int SN, float* dbuf, float* d_tok_a, float* d_tok_b, const GradPtrs& gp, bool lowp,
                            hipStream_t s);
hipError_t launch_ray_wgrad(const float* tape, const float* dbuf, int n_blocks, const GradPtrs& gp, bool lowp, hipStream_t s);
hipError_t launch_presim_bwd(const RawPtrs& wp, const GradPtrs& gp, const float* sim8, const float* d_pv, int P, bool lowp,
                             hipStream_t s);
// scratch: gather_bwd_scratch_floats(f) floats (zeroed by the launcher): the channel-last record volumes of the scatter
size_t gather_bwd_scratch_floats(const FrameDev& f);
hipError_t launch_gather_bwd(const FrameDev& f, float* const* grad_feat, float* const* grad_weight, const float* ray_o,
                             int o_stride, const float* ray_d, const float* z, const float* d_pv, const int* pv_row, int RN,
                             int SN, float* scratch, bool accumulate, bool scratch_zeroed, hipStream_t s);
struct FmtWeights {  // = ufr_fmt_layer_weights
  const float *wq, *bq, *wk, *bk, *wv, *bv, *wo, *bo, *w1, *b1, *w2, *b2, *n1w, *n1b, *n2w, *n2b;
};
int fmt_state_parts(int S);   // per-wave partial states of one sample's source tokens
hipError_t launch_fmt_layer(const FmtWeights& w, const float* x, const float* src, int N, int T, int S, float* out,
                            float* state, hipStream_t s);
hipError_t launch_pack_weights(const RawPtrs& raw, float* packed, float input_abs_max, int* range_flag, hipStream_t s);
hipError_t launch_refit_weights(float* packed, const unsigned* frame_bound, int* range_flag, hipStream_t s);
hipError_t launch_tsdf_integrate(float* tsdf, float* weight, float* color, const int* dim, const float* origin,
                                 float voxel_size, float trunc_margin, const float* K, const float* P,
                                 const float* depth_im, const float* color_im, int im_h, int im_w, float obs_weight,
                                 int integrate_color, hipStream_t s);
// mcubes.hip: marching cubes (count -> scan -> verts -> faces; see the file header)
int mcubes_tiles(const int* dim);
hipError_t launch_mcubes_count(const float* vol, const int* dim, float level, int* tile_counts, hipStream_t s);
hipError_t launch_mcubes_scan(const int* tile_counts, int n_tiles, long long* tile_off, long long* totals, hipStream_t s);
hipError_t launch_mcubes_verts(const float* vol, const int* dim, float level, const long long* tile_off, int* index,
                               float* verts, float* normals, long long n_verts, hipStream_t s);
hipError_t launch_mcubes_faces(const float* vol, const int* dim, float level, const long long* tile_off, const int* index,
                               int* faces, long long n_faces, hipStream_t s);
// similarity_field.hip: the pair similarity of the match maps on a voxel grid; gx / gy / gz are HOST tables (kernel arguments)
hipError_t launch_similarity_field(const FrameDev& f, const float* gx, const float* gy, const float* gz, const int* dim, float* u,
                                   unsigned char* n_vis, int min_views, hipStream_t s);
// chamfer.hip: DTU chamfer evaluation in fp64 (mesh sampling, cell keys, thinning rounds, nearest neighbours; see the file header)
long long chamfer_blocks(long long n);   // blocks of the per-item kernels: sizes the per-block workspace arrays
hipError_t launch_points_cell_keys(const double* pts, long long n, const double* origin, double cell, long long* keys,
                                   hipStream_t s);
hipError_t launch_mesh_sample_count(const double* verts, const int* faces, long long V, long long F, double density,
                                    long long* tri_off, long long* block_tot, hipStream_t s);
hipError_t launch_mesh_sample_scan(const long long* block_tot, long long n_blocks, long long* block_off, long long* total,
                                   hipStream_t s);
hipError_t launch_mesh_sample_emit(const double* verts, const int* faces, long long V, long long F, double density,
                                   const long long* tri_off, const long long* block_off, double* out, long long capacity,
                                   hipStream_t s);
hipError_t launch_thin_round(const double* pts, const long long* keys, const int* rank, long long n, double radius,
                             unsigned char* state, int* undecided, hipStream_t s);
hipError_t launch_nn_dist(const double* query, long long nq, const double* ref, const long long* keys, long long nr,
                          const double* origin, double cell, double max_dist, double* dist, double* block_sum,
                          long long* block_cnt, double* mean_out, hipStream_t s);
// points_filter.hip: point-cloud filtering in fp64 (k nearest neighbours, normals, voxel means; see the file header)
long long points_filter_blocks(long long n);   // blocks of the voxel kernels: sizes the per-block workspace arrays
hipError_t launch_points_knn(const double* query, long long nq, const double* ref, const long long* keys, const int* ref_index,
                             long long nr, const double* origin, double cell, const int* self_index, int k, double max_dist,
                             int* idx, double* dist, hipStream_t s);
hipError_t launch_points_normals(const double* pts, long long n, const int* idx, int k, const double* views, int V, double* normal,
                                 double* curvature, unsigned char* valid, hipStream_t s);
hipError_t launch_voxel_count(const long long* keys, long long n, long long* block_tot, long long* block_off, long long* total,
                              hipStream_t s);
hipError_t launch_voxel_mean(const double* pts, const long long* keys, long long n, const unsigned char* colors,
                             const double* normals, const long long* block_off, double* out_pts, unsigned char* out_colors,
                             double* out_normals, int* out_count, long long capacity, hipStream_t s);
// depth_fusion.hip: geometric-consistency filtering of depth maps and the ordered compaction of the valid pixels (see the file header)
long long depth_points_blocks(long long n);   // blocks of the compaction kernels: sizes the per-block workspace arrays
hipError_t launch_depth_consistency(const float* ref, int H, int W, const float* const* src_depth, const int* src_hw,
                                    const double* mats, int S, double pix_thres, float depth_thres, int mask_thres, int* mask_sum,
                                    unsigned char* mask, double* depth_avg, unsigned char* pair_masks, hipStream_t s);
hipError_t launch_depth_points_count(const unsigned char* mask, long long n, long long* block_tot, long long* block_off,
                                     long long* total, hipStream_t s);
hipError_t launch_depth_points_emit(const unsigned char* mask, const double* depth_avg, const unsigned char* color, int H, int W,
                                    const double* inv_k, const double* inv_e, const long long* block_off, float* xyz,
                                    unsigned char* rgb, long long capacity, hipStream_t s);
// mesh_clean.hip: DTU mesh cleaning -- mask dilation, vertex votes, first-hit faces, face components (see the file header)
hipError_t launch_mask_dilate(const unsigned char* src, int H, int W, int k, const short* half_widths, int thresh,
                              unsigned char* dilated, unsigned char* mask, hipStream_t s);
hipError_t launch_vertex_votes(const double* verts, long long V, const float* P, int NV, const unsigned char* masks, int H, int W,
                               int* votes, hipStream_t s);
// (the one first hit of the tree: ufr_mesh_first_hit and ufr_raster_frames both come here; mask null = every pixel; the key
// image is re-initialised by every call)
hipError_t launch_first_hit(const double* verts, const int* faces, long long V, long long F, const float* kinv, const float* rot,
                            const float* org, const double* proj, const unsigned char* mask, int H, int W,
                            unsigned long long* keys, int* big_count, int* big_list, int* face_id, unsigned char* face_hit,
                            hipStream_t s);
hipError_t launch_edge_keys(const int* faces, const int* vid, long long V, long long F, long long* keys, hipStream_t s);
hipError_t launch_mark_pairs(const long long* keys, const long long* order, long long F, int* pair_a, int* pair_b,
                             unsigned char* has_adj, int* parent, hipStream_t s);
hipError_t launch_component_round(const int* pair_a, const int* pair_b, long long F, int* parent, int* changed, hipStream_t s);
hipError_t launch_component_labels(const int* parent, const unsigned char* has_adj, long long F, int* labels, hipStream_t s);
// raster.hip: mesh rendering -- vertex normals, shading of a first-hit face image, box downsampling (see the file header)
hipError_t launch_raster_vertex_normals(const double* verts, const int* faces, long long V, long long F, const long long* slots,
                                        const long long* runs, double* normals, hipStream_t s);
// (tex given: the colour of a pixel is the bilinear sample of `texture` (Ht,Wt,3) at the barycentric mix of the face's three
// texel coordinates corner_xy (F,3,2), ufr_texture_frames; colors and base are then not looked at)
struct RasterTexture {
  const double* corner_xy;
  const unsigned char* texture;
  int Ht, Wt;
};
hipError_t launch_raster_shade(const double* verts, const int* faces, long long V, long long F, const double* normals,
                               const unsigned char* colors, const float* kinv, const float* rot, const float* org,
                               const double* proj, const double* base, double ambient, const unsigned char* bg, const int* face_img,
                               int H, int W, unsigned char* image, float* depth, int* face_out, float* normal_out, hipStream_t s,
                               const RasterTexture* tex = nullptr);
hipError_t launch_raster_downsample(const unsigned char* src, long long n, int H, int W, int sf, unsigned char* dst, hipStream_t s);
// splat.hip: point-cloud rendering -- z-buffered splat into a key image, resolve with eye-dome lighting (see the file header)
// (k 3x3 and w2c 4x4: host fp64; launch_splat presets the key image before its kernel)
hipError_t launch_splat(const double* points, long long N, const double* k, const double* w2c, int H, int W, int radius, double z_min,
                        unsigned long long* keys, hipStream_t s);
hipError_t launch_splat_resolve(const unsigned long long* keys, long long N, const unsigned char* colors, const double* base,
                                const unsigned char* bg, double edl_strength, int edl_radius, int H, int W, unsigned char* image,
                                float* depth, int* point_id, hipStream_t s);
// frame_input.hip: a scan loader's per-pixel work -- 8-bit images to resized, cropped float planes; ray tables (see the file header)
// (mask: null, or a second source (n,Hs,Ws) resized by the same rule and multiplied in as m / 254)
hipError_t launch_image_resize_u8(const unsigned char* src, const unsigned char* mask, long long n, int Hs, int Ws, int H, int W, int x0,
                                  int y0, int Ho, int Wo, float* dst, hipStream_t s);
// view_select.hip: the pair scores of a COLMAP model's view selection (see the file header)
hipError_t launch_view_pair_scores(const long long* offsets_host, const int* obs, const double* points, long long M,
                                   const double* centres, int N, double theta0, double sigma1, double sigma2, double* score,
                                   long long* offsets_dev, int* sorted, hipStream_t s);
// undistort.hip: n pictures of one COLMAP camera resampled to a pinhole camera (see the file header)
// (model: one of the nine ids the file header lists; params, k_out: host fp64, checked by the entry point)
hipError_t launch_image_undistort(const unsigned char* src, int n, int Hs, int Ws, int C, int model, const double* params,
                                  const double* k_out, int H, int W, unsigned char* dst, unsigned char* valid, hipStream_t s);
hipError_t launch_pixel_rays(const float* m_inv, const float* origin, int H, int W, float* dir, hipStream_t s);
hipError_t launch_depth_gt(const float* pfm, int Hs, int Ws, int bottom_up, int y0, int x0, int H, int W, float scale_factor,
                           const double* cam_ray_z, float* depth, hipStream_t s);
// poisson.hip: uniform-grid Poisson reconstruction -- splat, divergence, q = A p, conjugate gradients, samples (see the file header)
constexpr int kPsTileX = 8, kPsTileY = 4, kPsTileZ = 64;   // nodes one block of the q = A p kernel owns at a time (x marched)
constexpr int kPsMaxBlocks = UFR_POISSON_MAX_PARTIALS;                       // most partial sums one dot product leaves in the workspace
long long poisson_tiles(const int* dims);
int poisson_blocks(long long work_items);
hipError_t launch_poisson_splat_keys(const double* pts, long long n, const double* origin, double h, const int* dims, long long* keys,
                                     hipStream_t s);
hipError_t launch_poisson_splat_sum(const double* pts, const double* nrm, long long n, const double* origin, double h, const int* dims,
                                    const long long* keys, const long long* rows, double* V, double* W, hipStream_t s);
hipError_t launch_poisson_divergence(const double* V, const int* dims, double h, double* b, hipStream_t s);
hipError_t launch_poisson_laplace(const double* p, const int* dims, double h, double* q, double* part, hipStream_t s);
hipError_t launch_poisson_cg_init(const double* b, long long n, double* x, double* r, double* p, double* part, double* state,
                                  hipStream_t s);
hipError_t launch_poisson_cg_iteration(const int* dims, double h, double* x, double* r, double* p, double* q, double* pq_part,
                                       double* rr_part, double* state, int slot, hipStream_t s);
hipError_t launch_poisson_sample(const double* vol, const int* dims, const double* origin, double h, const double* pts, long long n,
                                 double* values, double* mean_out, double* part, hipStream_t s);
// mesh_color.hip: per-vertex colour from the photographs and the neighbour fill (see the file header)
constexpr int kColorThreads = 256;         // vertices a block owns (ops.MESH_COLOR_BLOCK says the same to the tests)
constexpr int kColorCamsPerLaunch = 16;    // camera records one upload launch carries in its argument segment
struct MeshColorCam {
  double k[9], r[9], t[3], c[3];           // intrinsics, w2c's rotation and translation, the centre in world coordinates
};
hipError_t launch_mesh_color_cams(const MeshColorCam* cams_host, int n_views, MeshColorCam* table, hipStream_t s);
hipError_t launch_mesh_vertex_colors(const double* verts, const double* normals, long long V, const unsigned char* images,
                                     const float* depth, const MeshColorCam* table, int n_views, int H, int W, double z_min,
                                     double depth_tol, double min_cos, int power, int mode, const unsigned char* fill,
                                     unsigned char* colors, unsigned char* views_used, hipStream_t s);
hipError_t launch_mesh_color_fill_round(const int* faces, long long V, long long F, const long long* slots, const long long* runs,
                                        const unsigned char* colors_in, const unsigned char* state_in, unsigned char* colors_out,
                                        unsigned char* state_out, int* filled, hipStream_t s);
// mesh_texture.hip: a per-face texture atlas baked from the photographs and its texel-space fill (see the file header)
constexpr int kTextureThreads = 256;       // texels a block owns (texture_ops.TEXTURE_BLOCK says the same to the tests)
constexpr bool kTextureBakeCellMajor = true;   // the bake's thread order: profiles/mesh_texture_launch_shapes.md
struct TextureAtlas {
  int S, cols, Ht, Wt;                     // patch size, cells a row, the atlas: Wt = cols * (S + 3), Ht = rows * (S + 3)
  long long F;                             // faces: cell q holds faces 2q and 2q + 1
};
hipError_t launch_texture_bake(const double* verts, const int* faces, long long V, const TextureAtlas& at, const unsigned char* images,
                               const float* depth, const MeshColorCam* table, int n_views, int H, int W, double z_min,
                               double depth_tol, double min_cos, int power, int mode, const unsigned char* fill,
                               const unsigned char* fallback, unsigned char* texture, unsigned char* views_used, hipStream_t s);
hipError_t launch_texture_fill_round(const TextureAtlas& at, const unsigned char* colors_in, const unsigned char* state_in,
                                     unsigned char* colors_out, unsigned char* state_out, int* filled, hipStream_t s);
// mesh_simplify.hip: vertex clustering with quadric placement (see the file header)
constexpr int kSimplifyThreads = 256;      // items a block owns (ops.SIMPLIFY_BLOCK says the same to the tests)
long long simplify_blocks(long long n);    // blocks of the scanning kernels: sizes the per-block workspace arrays
hipError_t launch_simplify_clusters(const long long* keys, const long long* order, long long V, int* cluster,
                                    long long* cluster_key, long long capacity, long long* block_tot, long long* block_off,
                                    long long* total, hipStream_t s);
hipError_t launch_simplify_face_keys(const int* faces, const int* cluster, long long V, long long F, long long* keys, hipStream_t s);
hipError_t launch_simplify_quadrics(const double* verts, const int* faces, const long long* cluster_key, long long V, long long F,
                                    long long C, const double* origin, double cell, const long long* sorted_keys,
                                    double* quadrics, int* n_faces, hipStream_t s);
hipError_t launch_simplify_place(const double* quadrics, const int* n_faces, const double* mean, const long long* cluster_key,
                                 long long C, const double* origin, double cell, int placement, double* position,
                                 unsigned char* placed, hipStream_t s);
hipError_t launch_simplify_face_triples(const int* faces, const int* cluster, long long V, long long F, int* triples,
                                        long long* key_a, long long* key_bc, hipStream_t s);
hipError_t launch_simplify_face_heads(const long long* key_a, const long long* key_bc, const long long* order, long long F,
                                      unsigned char* keep, hipStream_t s);
hipError_t launch_simplify_compact_faces(const int* triples, const unsigned char* keep, long long F, long long C, int* out_faces,
                                         int* face_map, long long capacity, unsigned char* referenced, long long* block_tot,
                                         long long* block_off, long long* total, hipStream_t s);
hipError_t launch_simplify_compact_vertices(const unsigned char* referenced, long long C, const double* position,
                                            const unsigned char* colors, const unsigned char* placed, const int* count,
                                            const int* cluster, long long V, int* faces, long long n_faces, double* out_verts,
                                            unsigned char* out_colors, unsigned char* out_placed, int* out_count,
                                            long long capacity, int* cluster_vertex, int* vertex_map, long long* block_tot,
                                            long long* block_off, long long* total, hipStream_t s);
// mesh_smooth.hip: Laplacian and Taubin smoothing with uniform or cotangent weights (see the file header; block and chunk sizes: mesh_rows.h)
hipError_t launch_mesh_smooth_rows(const double* verts, const int* faces, long long V, long long F, const long long* slots,
                                   int cotangent, int* nbr, double* wgt, hipStream_t s);
hipError_t launch_mesh_smooth_border(long long V, long long F, const long long* runs, const int* nbr, unsigned char* border,
                                     hipStream_t s);
hipError_t launch_mesh_smooth_step(long long V, long long F, const long long* runs, const int* nbr, const double* wgt,
                                   const unsigned char* border, const unsigned char* pinned, double t, const double* in,
                                   double* out, hipStream_t s);
// mesh_denoise.hip: bilateral normal filtering and the vertex update that follows the filtered normals (see the file header)
hipError_t launch_mesh_denoise_faces(const double* verts, const int* faces, long long V, long long F, double* rec, double* normals,
                                     hipStream_t s);
hipError_t launch_mesh_denoise_rows(const int* faces, long long V, long long F, const long long* slots, const double* rec, int* rows,
                                    int* row_face, hipStream_t s);
hipError_t launch_mesh_denoise_border(long long V, long long F, const long long* runs, const int* rows, unsigned char* border,
                                      hipStream_t s);
hipError_t launch_mesh_denoise_normals(const int* faces, long long V, long long F, const long long* runs, const int* row_face, double two_ss,
                                       double two_rr, const double* in, double* out, double* normals, hipStream_t s);
hipError_t launch_mesh_denoise_vertices(long long V, long long F, const long long* runs, const int* rows, const double* normals,
                                        const unsigned char* border, const unsigned char* pinned, const double* in, double* out,
                                        hipStream_t s);
// frame_metrics.hip: the scores and 8-bit previews of a validation frame (see the file header)
constexpr int kFrameMetricsBlocks = 256;   // most partial rows one frame leaves in the workspace
hipError_t launch_frame_metrics(const float* rgb_c, const float* rgb_f, const float* rgb_gt, const float* depth_c, const float* depth_f,
                                const float* depth_gt, float near_z, float far_z, int n, double* out8, double* rows, hipStream_t s);
hipError_t launch_frame_preview_u8(const float* rgb, const float* depth, const double* depth_max, float depth_scale, int n,
                                   unsigned char* rgb8, unsigned char* depth8, hipStream_t s);
// conv2d.hip: the plain 2-D convolutions of FeatureNet on channel-last tensors, epilogue fused (see the file header)
struct Conv2dArgs {
  const float* in;      // [B][H][W][CIN] (the stem: planar [B][3][H][W])
  const float* w;       // [cout][CIN][KS][KS]
  const float* scale;   // [cout] or null (= 1)
  const float* shift;   // [cout] or null (= 0)
  const float* skip;    // [B][Ho/2][Wo/2][cout] added after nearest 2x upsampling, or null
  float* out;           // [B][Ho][Wo][cout], or planar [B][cout][Ho][Wo]
  int B, H, W, Ho, Wo, cout;
  int relu, out_planar, sigmoid_from;   // sigmoid on channels >= sigmoid_from (< 0: none)
};
hipError_t launch_conv2d(const Conv2dArgs& a, int cin, int ks, int stride, int in_planar, hipStream_t s);
hipError_t launch_upsample_add(const float* reduced, const float* fine, float* out, int B, int C, int h, int w, hipStream_t s);
// dcn.hip, channel-last form: epilogue out = [relu]((dcn + bias) * scale + shift), channel-last or planar output
struct DcnEpilogue {
  const float* scale;
  const float* shift;
  int relu, out_cl;
  int om_planes;      // 0: offset [B][18][H][W] and mask [B][9][H][W]; 27: one [B][27][H][W] block, mask = offset + 18 planes
};
hipError_t launch_deform_conv3x3(const float* in_cl, const float* offset, const float* mask, const float* weight,
                                 const float* bias, float* out, int B, int C, int Cout, int H, int W, hipStream_t s,
                                 DcnEpilogue ep = DcnEpilogue{nullptr, nullptr, 0, 0, 0});
size_t conv3d_planes_workspace_bytes(int cin, int cout, int cout2, int mode);
hipError_t launch_conv3d_wgrad_heads(const float* in, const float* d_out, const float* d_out2, float* dw, float* dw2, int B, int D, int H,
                                     int W, hipStream_t s);
hipError_t launch_conv3d_wgrad_planes(const float* tp, const float* tq, float* dw, float* dbias, int B, int Dp, int Hp, int Wp, int Dq,
                                      int Hq, int Wq, int ca, int cb, int S, hipStream_t s);
hipError_t launch_absmax(const float* x, size_t n, float* absmax, hipStream_t s);
hipError_t launch_conv3d_planes(const float* in, const float* in_absmax, const float* weight, const float* weight2, const float* bias,
                                const float* scale, const float* shift, const float* skip, float* out, float* out2, float* out_absmax,
                                int B, int D, int H, int W, int cin, int cout, int cout2, int mode, int relu, int ncdhw, int flip,
                                void* ws, int planes_ready, hipStream_t s);
hipError_t launch_conv3d(const float* in, const float* weight, const float* weight2, const float* bias, const float* scale,
                         const float* shift, const float* skip, float* out, float* out2, int B, int D, int H, int W,
                         int cin, int cout, int cout2, int mode, int relu, int ncdhw, hipStream_t s, int flip = 0,
                         float* out_absmax = nullptr);
hipError_t launch_conv3d_bwd_data(const float* d_out, const float* weight, const float* accumulate, float* d_in, int B, int D,
                                  int H, int W, int cin, int cout, int mode, hipStream_t s);
hipError_t launch_conv3d_bwd_weight(const float* in, const float* d_out, float* d_weight, float* d_bias, int B, int D, int H, int W,
                                    int cin, int cout, int mode, hipStream_t s);
hipError_t launch_chw_to_hwc(const float* in, float* out, int N, int C, int S, hipStream_t s);
hipError_t launch_pixelwise_weights(const float* sim, const float* params, float* vw, float* agg, int NS, int D, int H, int W,
                                    hipStream_t s);
hipError_t launch_correlate(const float* ref_cl, const float* src_cl, const float* proj_host, int NS, const float* depth,
                            const float* vw, float* sim, float* agg, int C, int H, int W, int D, hipStream_t s);
// train_step.hip: the optimizer update and the ray draw of a training step (see the file header)
constexpr int kAdamTableCap = UFR_ADAM_TABLE_CAPACITY;   // tensors per launch
constexpr int kSelectMaxK = 4096;                        // pairs the sorting block holds in LDS
struct SelectWorkspace {
  uint32_t* hist;              // [3][2048] digit counters, then 4 words of state
  int* totals;                 // [blocks][2]
  long long* off;              // [blocks][2]
  long long* grand;            // [2]
  unsigned long long* cand;    // [k]
};
int select_compact_blocks(int n);
hipError_t launch_adam(const ufr_adam_tensor* t, int nt, double lr, double beta1, double beta2, double eps, hipStream_t s);
hipError_t launch_select_rays(const float* u, int n, int k, long long* idx_out, const SelectWorkspace& w, hipStream_t s);

}  // namespace ufr
