/*
 * sfgs.h -- C ABI of libsfgs.so, the MI355X (gfx950) Gaussian-splat rasterizer hot path.
 *
 * This header is the drop-in boundary. Everything here is plain C: device pointers, sizes and
 * a HIP stream handle passed as void*. No torch types, no C++ types. The Python packages
 * diff_gauss / fused_ssim / simple_knn (skyfall-gs_amd/) bind these symbols with ctypes; the
 * binding a maintainer of the reference would add is shown in INTEGRATION.md.
 *
 * Reference interface each entry point replaces (paths relative to the reference tree):
 *
 *   sfgs_raster_*      diff_gauss.GaussianRasterizer.__call__      gaussian_renderer/__init__.py:57,132-140
 *                      diff_gauss.GaussianRasterizationSettings    gaussian_renderer/__init__.py:40-55
 *                      autograd backward of that call              train.py:279,845
 *   sfgs_ssim_*        fused_ssim.fused_ssim(img1, img2)           train.py:42,222,778
 *   sfgs_loss_*        the loss statements: mask products, l1_loss, fused_ssim, scrub, pearson_corrcoef   train.py:205-234,760-799
 *   sfgs_resample_gt   create_offset_gt(mask * original_image, subpixel_offset): meshgrid + grid_sample   train.py:64-77,207,214-215,770-771
 *   sfgs_opacity_entropy_*  the opacity regulariser: get_opacity.clamp + binary_cross_entropy(o, o)     train.py:236-242,834-843
 *   sfgs_depthvis_*    colorize_depth_torch(depth, mask, normalize) render_video.py:129-170, render_video_from_ply.py:126-167, train.py:1001-1041
 *   sfgs_frame_quantize  (img * 255 + 0.5).clip(0, 255).astype(uint8)  render_video.py:264
 *   sfgs_metrics_*     the evaluation pass of training_report: clamp, l1_loss, psnr (and ssim)   train.py:1064,1075,1090-1091, utils/image_utils.py:14-19, utils/loss_utils.py:17-18,33-63
 *   sfgs_dsm_*         depth_to_point_cloud + create_dsm_manual_satnerf_style, compute_dsm_metrics, register_dsms_simple   evaluate_gs_geometry.py:132-215,270-312,528-585
 *   sfgs_dsmr_*        dsmr.compute_shift (recursive_ncc, mean_std), dsmr.apply_shift_   dsmr.py:16-149
 *   sfgs_pointcloud_*  depth_to_point_cloud per view, np.vstack, the cloud's bounds   evaluate_gs_geometry.py:132-215,776,787-790
 *   sfgs_ortho_*       (no counterpart: the script renders RGB per camera next to the depth, writes it to a PNG and keeps no georeferenced colour)   evaluate_gs_geometry.py:736-765
 *   sfgs_consistency_* (no counterpart: the script unprojects every rendered depth pixel it gets, evaluate_gs_geometry.py:767-776, and has no filter between the views)
 *   sfgs_tsdf_*        (no counterpart: the script has no mesh step; its geometry products are the DSM and the merged cloud, evaluate_gs_geometry.py:776-784)
 *   sfgs_mesh_*        (no counterpart: the soup of sfgs_tsdf_extract welded into an indexed mesh, its components labelled, floaters removed)
 *   sfgs_raster_blend_stats, sfgs_blend_stats_views  (no counterpart: the reference's only pruning tool is GaussianModel.prune_by_radius, scene/gaussian_model.py:752, by distance)
 *   sfgs_similarity_transform  (no counterpart: the reference never merges scenes; it trains each in a frame of its own, scene/dataset_readers.py:378-390)
 *   sfgs_knn_dist2     simple_knn._C.distCUDA2(points)             scene/gaussian_model.py:25,324
 *   sfgs_prepass_*     GaussianModel.get_*_with_3D_filter/get_rotation  scene/gaussian_model.py:207-249 (next row)
 *
 * Ownership: every buffer (inputs, outputs, gradients, scratch "blobs") is allocated by the
 * caller (PyTorch's caching allocator on the right device). The library never allocates or
 * frees device memory and keeps no device state between calls, so it is thread-safe per
 * stream by construction (the autograd backward runs on a different host thread).
 *
 * Errors: every function returns SFGS_OK (0) or a negative SfgsStatus. Nothing throws across
 * the ABI, nothing calls exit(). sfgs_last_error() returns a thread-local message.
 */
#ifndef SFGS_H
#define SFGS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SFGS_ABI_VERSION 28

typedef enum SfgsStatus {
  SFGS_OK = 0,
  SFGS_E_ARG = -1,         /* bad argument (null pointer, negative size, struct_size mismatch) */
  SFGS_E_HIP = -2,         /* a HIP runtime call or kernel launch failed                       */
  SFGS_E_CAPACITY = -3,    /* a caller-owned blob is smaller than the plan requires            */
  SFGS_E_UNSUPPORTED = -4  /* e.g. sh_degree > 4, image wider than 65535 tiles                 */
} SfgsStatus;

/* Depth output convention (SURVEY 8c "unpinned semantic decisions"). */
#define SFGS_DEPTH_NORMALISED 0 /* depth = sum(T a z) / (1 - T_final); NaN where nothing hit (default) */
#define SFGS_DEPTH_RAW 1        /* depth = sum(T a z)                                                  */

/* One camera frame = diff_gauss.GaussianRasterizationSettings (14 fields,
 * gaussian_renderer/__init__.py:40-55). Matrix pointers are DEVICE pointers to the 16 floats of
 * the reference's row-major *transposed* matrices (scene/cameras.py:62-73):
 * p_view = [p,1] * viewmatrix, p_hom = [p,1] * projmatrix. */
typedef struct SfgsFrame {
  uint32_t struct_size;          /* = sizeof(SfgsFrame), ABI versioning                         */
  int32_t image_height;
  int32_t image_width;
  float tanfovx;
  float tanfovy;
  float kernel_size;             /* Mip-Splatting 2D filter variance (arguments/__init__.py:111) */
  float scale_modifier;
  int32_t sh_degree;             /* active SH degree 0..4 (sh_coeffs 1 / 4 / 9 / 16 / 25 stored)     */
  int32_t sh_coeffs;             /* coefficients stored per Gaussian in `shs` (max_degree+1)^2   */
  int32_t prefiltered;           /* accepted, ignored (reference always passes False)            */
  int32_t debug;                 /* !=0: synchronise + check after every launch                  */
  int32_t depth_mode;            /* SFGS_DEPTH_*                                                 */
  int32_t tile_row_begin;        /* band rendering (multi-GPU joint render): only 8-pixel  */
  int32_t tile_row_end;          /* tile rows [begin, end) are binned/composited; end <= 0 = all rows.
                                    Pixels outside the band are left untouched in the outputs.      */
  const float* subpixel_offset;  /* device [H,W,2] or NULL (= zeros)                             */
  const float* bg;               /* device [3]                                                   */
  const float* viewmatrix;       /* device [16]                                                  */
  const float* projmatrix;       /* device [16]                                                  */
  const float* campos;           /* device [3]                                                   */
  uint32_t launch_hints;         /* SFGS_HINT_* bits, 0 = none (see below)                       */
  void* feedback;                /* optional: 64 bytes of DEVICE memory, caller-owned and persistent across the frames of
                                    one stream (zero it once). The render / backward stages leave the frame's late
                                    statistics there -- they only exist once those stages have run -- and the NEXT
                                    sfgs_raster_forward_plan reports them (SfgsRasterCounters.prev_*): the feedback the
                                    launch hints are chosen from.                                                */
} SfgsFrame;

/* Launch hints. A frame's optional kernels -- the huge-splat walk, the three long-list sorts, the backward's dead-entry
 * prefill and chunk pre-reduction -- each cost ~5 us of queue time even when they find nothing to do, and whether they
 * have work is only known on the device. The caller may assert what it learnt from the previous frames:
 *   NO_HUGE_SPLATS  plan: do not launch the huge-splat walk. If SfgsRasterCounters.num_huge_splats comes back != 0 the
 *                   frame was binned WITHOUT those splats: redo plan + render without the hint.
 *   FEW_LONG_LISTS  render: ONE catch-all kernel sorts every list longer than 512 entries instead of three size-class
 *                   kernels. Always correct; slower when many lists are long.
 *   SHORT_LISTS     render: the caller expects per-tile lists of a few hundred entries at most and coarse bins of a few
 *                   thousand items (what the previous frame's plan / feedback reported): fine binning and the sort of the
 *                   short lists run as ONE kernel that never writes per-tile items to memory (select_sort_kernel). Always
 *                   correct -- both routes build bit-identical lists --; slower than the two-kernel route when lists
 *                   or bins are long.
 *   MEDIUM_LISTS    render: as SHORT_LISTS, for frames whose lists reach 513 .. 1 024 entries (what the feedback of the
 *                   previous frame reported): the same kernel with twice the list capacity (48 KB of LDS per workgroup,
 *                   the 16-key register network for the lists beyond 512). Always correct; implies the fused route.
 *   LISTS_768       render, with MEDIUM_LISTS: the fused kernel with room for 768 instead of 1 024 entries per list (36 KB of LDS
 *                   per workgroup: four instead of three workgroups per CU) -- for frames whose lists exceed 512 but (almost)
 *                   never 768 entries; the few longer ones take the long-list kernels. Always correct.
 *   TILE_ORDER      render: the caller expects tile lists of very different lengths (the previous frame's longest list
 *                   several times its mean: a city seen from above, a few facades edge-on). The compositing kernels then
 *                   take their tiles longest list first within each XCD's share of the image (two launches of a small
 *                   ordering kernel) instead of in image order, so that the kernels' last stretch is filled with SHORT
 *                   lists. Always correct: tiles are independent, the results are the same bits in any order.
 *   NO_PREFILL      backward: do not launch the dead-entry prefill kernel (its decision then reads "no"). Always correct.
 *   NO_BIG_CHUNKS   backward: do not launch the chunk pre-reduction. Only valid when THIS frame's plan reported
 *                   num_big_chunks == 0. */
#define SFGS_HINT_NO_HUGE_SPLATS 1u
#define SFGS_HINT_FEW_LONG_LISTS 2u
#define SFGS_HINT_NO_PREFILL 4u
#define SFGS_HINT_NO_BIG_CHUNKS 8u
#define SFGS_HINT_SHORT_LISTS 16u
#define SFGS_HINT_MEDIUM_LISTS 32u
#define SFGS_HINT_TILE_ORDER 64u
#define SFGS_HINT_LISTS_768 128u

/* Per-Gaussian inputs = keyword arguments of GaussianRasterizer.__call__
 * (gaussian_renderer/__init__.py:132-140). All float32, contiguous, device memory.
 * Exactly one of colors_precomp / shs is non-NULL. cov3Ds_precomp must be NULL: that path is
 * dead in the reference (scales.float() at :138 dereferences None when it would be used). */
typedef struct SfgsGaussians {
  uint32_t struct_size;
  int32_t count;                 /* N                                              */
  const float* means3D;          /* [N,3]                                          */
  const float* scales;           /* [N,3]  (already 3D-filtered, activated)        */
  const float* rotations;        /* [N,4]  (w,x,y,z), normalised by the caller     */
  const float* opacities;        /* [N,1]  (already 3D-filter compensated)         */
  const float* colors_precomp;   /* [N,3] or NULL                                  */
  const float* shs;              /* [N,sh_coeffs,3] or NULL                        */
  /* RAW-PARAMETER MODE (the activations + Mip-Splatting 3D filter folded into preprocess and
   * preprocess_bwd). When filter_3D is non-NULL, `scales`, `rotations` and `opacities` above are the model's RAW
   * parameters -- _scaling, _rotation, _opacity of scene/gaussian_model.py -- and the library evaluates
   * get_scaling_with_3D_filter (:207-213), get_opacity_with_3D_filter (:237-249) and get_rotation (:216-217) itself, with
   * the same float sequence as sfgs_prepass_forward (the frame equals, bit for bit, the one rendered from that function's
   * outputs). The backward then writes the gradients of the RAW parameters (sfgs_prepass_backward's results) into
   * SfgsGaussianGrads.scales / rotations / opacities. */
  const void* filter_3D;         /* [N,1] float32 or float64, or NULL = activated inputs (the mode above this comment) */
  int32_t raw_f64_mask;          /* bit 0: filter_3D is float64; bit 1: `opacities` points to float64 raw opacities
                                    (the reference's _opacity after its first reset_opacity, :483-501); 0 when
                                    filter_3D is NULL */
  /* EVAL_SH-FOLDED COLOUR PATH (ABI 12; SURVEY 8f row 1, last part). render()'s Python colour paths -- the appearance
   * MLP's toned coefficients and `convert_SHs_python` -- compute
   *     colors_precomp = clamp_min(eval_sh(active_sh_degree, sh[N,3,K], dirs[N,3]) + 0.5, 0)
   * (gaussian_renderer/__init__.py:112-118,121-125; utils/sh_utils.py:57-112) with torch kernels and hand the result over
   * as colors_precomp. When sh_dirs is non-NULL, `shs` above is that CHANNEL-MAJOR [N,3,sh_coeffs] coefficient tensor and
   * (shs_channel_major = 1) and sh_dirs the `dirs` argument ([N,3], used as given: eval_sh does not normalise it either), and preprocess /
   * preprocess_bwd evaluate the expression themselves (degrees 0-4): no N x 3 intermediate, no eval_sh launch. The
   * backward writes SfgsGaussianGrads.shs channel-major and the direction gradient to SfgsGaussianGrads.sh_dirs (it does
   * NOT flow into grads.means3D: `dirs` is an input of its own, the caller's graph carries it on). */
  const float* sh_dirs;          /* [N,3] or NULL = `shs` is [N,sh_coeffs,3] and the direction is normalize(means3D - campos) */
  int32_t shs_channel_major;     /* with sh_dirs: 1 = `shs` is eval_sh's [N,3,sh_coeffs]; 0 = it is [N,sh_coeffs,3] (what
                                    render()'s convert_SHs_python path passes to eval_sh is a transposed VIEW of the
                                    model's [N,K,3] features: hand over the features themselves). 0 without sh_dirs */
  /* SPLIT SH STORAGE (ABI 13). The reference's model keeps the SH coefficients as two parameters, _features_dc [N,1,3]
   * and _features_rest [N,K-1,3], and concatenates them on every get_features call (scene/gaussian_model.py:227-231; two
   * calls per render(): gaussian_renderer/__init__.py:114,121-122,127). When shs_rest is non-NULL, `shs` above holds
   * coefficient 0 only ([N,1,3]) and shs_rest coefficients 1 .. sh_coeffs-1 ([N,sh_coeffs-1,3]); preprocess reads the two
   * arrays, the backward writes SfgsGaussianGrads.shs ([N,1,3]) and .shs_rest: no concatenated copy, no split of its
   * gradient. Needs sh_coeffs > 1 and shs_channel_major == 0; with or without sh_dirs. */
  const float* shs_rest;         /* [N,sh_coeffs-1,3] or NULL = `shs` holds all sh_coeffs coefficients */
  /* DIRECTIONS FROM CENTRES (ABI 15). render()'s Python colour paths compute eval_sh's `dirs` as
   *     dir_pp = xyz - camera_center.repeat(N, 1);  dirs = dir_pp / dir_pp.norm(dim=1, keepdim=True)
   * (gaussian_renderer/__init__.py:114-115, :122-123): six elementwise / reduction launches and eight more on the way
   * back. sh_centers, an alternative to sh_dirs, hands over the subtrahend ([N,3], as render() built it -- any values)
   * instead of the finished directions: preprocess evaluates normalize(means3D - sh_centers) itself (the float sequence
   * of the in-kernel SH path's normalize(means3D - campos)) and preprocess_bwd adds the direction's gradient to
   * grads.means3D; grads.sh_dirs stays NULL. Everything else as with sh_dirs (shs layout, shs_channel_major, shs_rest). */
  const float* sh_centers;       /* [N,3] or NULL */
} SfgsGaussians;

/* Gradient outputs of the backward pass (all device, float32, fully overwritten). */
typedef struct SfgsGaussianGrads {
  uint32_t struct_size;
  float* means3D;        /* [N,3] */
  float* means2D;        /* [N,3]: cols 0:2 = dL/dmean2D in NDC units, col 2 = abs-grad magnitude
                            (scene/gaussian_model.py:744-749)                                    */
  float* scales;         /* [N,3] */
  float* rotations;      /* [N,4] */
  float* opacities;      /* [N,1]; raw-parameter mode with raw_f64_mask bit 1: [N,1] float64 (cast the pointer) */
  float* colors_precomp; /* [N,3] or NULL */
  float* shs;            /* [N,sh_coeffs,3] or NULL ([N,3,sh_coeffs] with SfgsGaussians.shs_channel_major) */
  float* sh_dirs;        /* [N,3]; non-NULL exactly when SfgsGaussians.sh_dirs is (NULL with sh_centers) */
  float* shs_rest;       /* [N,sh_coeffs-1,3]; non-NULL exactly when SfgsGaussians.shs_rest is (`shs` is then [N,1,3]) */
} SfgsGaussianGrads;

/* Sizes (bytes) of the caller-owned scratch blobs. */
typedef struct SfgsRasterSizes {
  uint32_t struct_size;
  size_t geom_bytes;     /* f(N):   per-Gaussian 2D records, duplicate offsets (72 bytes per Gaussian)   */
  size_t tiles_bytes;    /* f(W,H,N): counters, per-tile counts/offsets, per-block scan partials, the
                            binning radix pass's [workgroup][coarse bin] matrices                 */
  size_t bins_bytes;     /* f(D, coarse_capacity, N): coarse-bin slabs, per-tile duplicates, sorted lists; during
                            the plan the binning's pair list (96 bytes per Gaussian) lies on top of the per-tile
                            arrays, which only the render stage writes */
  size_t image_bytes;    /* f(W,H,D): per-pixel last contributor, final T, raw depth, and one 8-byte
                            blended-entries mask per pixel and 64-entry list batch (for backward) */
  size_t dupgrad_bytes;  /* f(D):   per-duplicate 2D gradient records + flags (backward only)    */
  int64_t coarse_bins;   /* number of 32x32-pixel coarse bins of this image (informational)      */
} SfgsRasterSizes;

/* Counters produced by the plan stage (host copy). */
typedef struct SfgsRasterCounters {
  int64_t num_duplicates;      /* D_eff: (Gaussian, 8x8 tile) pairs binned (opacity-aware test)             */
  int64_t num_duplicates_ref;  /* D:     sum of tiles_touched by the reference's 3-sigma 16x16 rule         */
  int64_t num_visible;         /* N_vis: count(radii > 0)                                                   */
  int64_t max_tile_list;       /* longest per-tile list (valid when read after sfgs_raster_forward_render)  */
  int64_t overflow;            /* != 0: dup_capacity or coarse_capacity was too small: redo the plan with
                                  dup_capacity >= sfgs_raster_slot_capacity(W, H, num_duplicates) and
                                  coarse_capacity >= max_coarse_bin. If both ALREADY hold, one of the 8 duplicate-index
                                  pools (each owns dup_capacity / 8 indices; a workgroup draws from pool id % 8) ran
                                  over because a few workgroups own most of the frame's duplicates: double
                                  dup_capacity. A caller should also treat max_coarse_bin > coarse_capacity as
                                  overflow (the library ORs it in; belt and braces)                         */
  int64_t max_coarse_bin;      /* most items appended DIRECTLY to one 32x32-pixel coarse bin's slab: those of the splats
                                  that reach more than 6 coarse bins (a whole wave walks them) or, with one-pass binning,
                                  every item. ABI 14: the items of the default two-pass binning no longer count -- they are
                                  stored bin-sorted and exactly sized, without a per-bin capacity -- so this is 0 for a
                                  frame of small splats, however skewed (a distant view: the scene in a few bins) */
  int64_t num_huge_splats;     /* splats reaching >= 64 coarse bins (their walk is a kernel of its own)        */
  int64_t num_big_chunks;      /* 1024-record chunks of Gaussians with > 2048 duplicates (backward pre-reduction) */
  int64_t prev_valid;          /* != 0: the prev_* fields below were read from SfgsFrame.feedback              */
  int64_t prev_long_tiles;     /* previous frame: tiles with lists longer than 512 entries                     */
  int64_t prev_max_tile_list;  /* previous frame: longest list                                                 */
  int64_t prev_prefilled;      /* previous frame's backward: the prefill kernel ran and chose to fill          */
  int64_t prev_tiles_over_512; /* previous frame: tiles with more than 512 entries, whichever route sorted them
                                  (prev_long_tiles counts the tiles LEFT to the long-list kernels: under MEDIUM_LISTS
                                  only those beyond 1 024): MEDIUM_LISTS pays when they are a sizeable part of the frame */
  int64_t max_bin_items;       /* ALL items of the fullest coarse bin (slab + bin-sorted run): what SFGS_HINT_SHORT_LISTS is
                                  chosen from. Filled by sfgs_raster_counters_decode / sfgs_raster_read_counters; 0 from
                                  sfgs_raster_read_counters_pinned (its 64 bytes end before it) */
  int64_t sort_wide_tiles;     /* ABI 24: tiles whose list the fused select + sort kernel sorted on the 64-bit (depth, id) key:
                                  every tile it sorts under "sort_key" = "wide"; otherwise those whose depth range does not fit
                                  the 32-bit tile-relative key or that hold two entries of equal depth. Produced by the render
                                  stage like max_tile_list: valid from sfgs_raster_read_counters after the render, 0 elsewhere
                                  and 0 under the split sort route */
} SfgsRasterCounters;

int sfgs_abi_version(void);
const char* sfgs_last_error(void);

/* Process-wide ROUTE options (ABI 16; tests and A/B runs -- never needed for correctness: every route builds bit-identical
 * results, tests/test_gpu_raster.py). They replace the getenv() calls the library used to make on every render: the
 * environment is read ONCE, when the library is loaded (SFGS_SORT, SFGS_PLAN_SCAN, SFGS_BINNING, SFGS_PREFILL, SFGS_KNN, SFGS_TILE_ORDER,
 * SFGS_SORT_KEY: same values),
 * and changed afterwards only through this call. Thread-safe: one atomic word per option; a render running on another
 * thread sees the old or the new value, never a mixture.
 *   key "sort"       "auto" (the frame's launch hints decide) | "fused" | "fused768" | "fused1024" | "split"
 *   key "plan_scan"  "fused" (the plan's epilogues ride in the scatter launch) | "separate"
 *   key "binning"    "auto" (two-pass below 65 536 coarse bins) | "direct"
 *   key "prefill"    "auto" (dead-entry prefill decided per frame on the device) | "always" | "never"
 *   key "knn"        "auto" (spatial search above 4 096 points) | "brute" (the exact all-pairs kernel at every size)
 *   key "tile_order" "auto" (SFGS_HINT_TILE_ORDER decides) | "always" | "never": longest-first tile order of the compositing kernels
 *   key "sort_key"   "auto" (= "narrow" for the kernel's 512-entry form, "wide" for its 768- and 1 024-entry forms) | "narrow": the
 *                    fused select + sort kernel sorts a tile on one exact 32-bit word per entry
 *                    (depth bits relative to the tile's nearest entry, above the entry's list position) when the tile's depth
 *                    range fits it and no two of its entries share a depth, on the 64-bit (depth, id) key otherwise | "wide":
 *                    the 64-bit key for every tile
 * sfgs_set_option returns SFGS_E_ARG for an unknown key or value; sfgs_get_option returns the current value's name
 * (a string constant) or NULL for an unknown key. */
int sfgs_set_option(const char* key, const char* value);
const char* sfgs_get_option(const char* key);

/* Optional per-kernel timing (bench.py's roofline leg): when enabled, every kernel launch of the
 * library is bracketed by HIP events recorded on the launch stream. sfgs_profile_collect waits for
 * the recorded events, returns per-kernel summed milliseconds and launch counts (arrays of
 * sfgs_profile_kernel_count() entries) and clears the record. Off by default; costs nothing then. */
int sfgs_profile_enable(int32_t on);
int sfgs_profile_select(uint64_t kernel_mask); /* bit i = time kernel id i (default: all); events cost ~4 us each */
int sfgs_profile_kernel_count(void);
const char* sfgs_profile_kernel_name(int32_t id);
int sfgs_profile_collect(double* ms_sum, int64_t* launches, int32_t n);

/* Box probe (ABI 17; bench.py, before its timed region -- not on the rendering path): a fixed FP32 multiply-add loop at 8 waves
 * per SIMD on every CU, timed with HIP events on `stream` (synchronous: returns when it has run, ~0.1 s). *valu_tflops = what
 * the box sustains on plain v_fma_f32; *sclk_mhz_effective = the shader clock that rate implies at one wave64 FMA per two cycles
 * per SIMD. Boxes of one pool run the same binary 3-8 % apart: a bench line carries these so that rounds can be compared. */
int sfgs_box_probe(double* valu_tflops, double* sclk_mhz_effective, void* stream);

/* Blob sizes for N Gaussians, a W x H image, a list-slot capacity D (bins, image, dupgrad) and a per-coarse-bin
 * item capacity (bins). Every 8x8 tile's list starts on a multiple of 64 slots and every 32x32-pixel coarse bin's lists
 * are placed from the bin's tile-hit total (an upper bound, scanned by the plan: no allocator), so a frame with
 * num_duplicates (Gaussian, tile) pairs needs D >= sfgs_raster_slot_capacity(W, H, num_duplicates) = num_duplicates +
 * 1088 * coarse bins (index space only: unused slots are never touched). */
int sfgs_raster_sizes(int32_t N, int32_t W, int32_t H, int64_t D, int64_t coarse_capacity,
                      SfgsRasterSizes* out);
int64_t sfgs_raster_slot_capacity(int32_t W, int32_t H, int64_t num_duplicates);

/* Forward, stage 1 ("plan"): preprocess every Gaussian (cull, EWA projection, 2D mip filter,
 * radius, SH->RGB), write radii[N] (int32) and bin every Gaussian COARSELY: one 16-byte item per
 * (Gaussian, 32x32-pixel coarse bin) holding the mask of the 8x8 tiles it can contribute to. The items
 * are sorted by bin into an exactly sized array inside `bins` (one radix pass; memory in proportion to
 * the items, whatever the frame's skew -- ABI 14); only the items of splats that reach more than 6
 * coarse bins are appended to their bin's slab (coarse_capacity items per bin) with an atomic each.
 * dup_capacity = duplicate indices / list slots. Neither count is known beforehand: if the counters
 * report overflow, call again with a bins blob sized for counters.num_duplicates /
 * counters.max_coarse_bin. Asynchronous on `stream`.
 * counters_pinned_host_128 (optional): 128 bytes of PINNED host memory (hipHostMalloc / torch pin_memory) that the
 * plan's last kernel fills with the frame's counters. Record an event right after this call, enqueue
 * sfgs_raster_forward_render, THEN wait for the event and sfgs_raster_counters_decode the buffer: the capacity
 * check overlaps with the render stage instead of draining the stream (max_tile_list is produced by the render
 * stage and reads 0 there; sfgs_raster_read_counters after the render returns it). */
int sfgs_raster_forward_plan(const SfgsFrame* frame, const SfgsGaussians* g, int32_t* radii,
                             void* geom, size_t geom_bytes, void* tiles, size_t tiles_bytes,
                             void* bins, size_t bins_bytes, int64_t dup_capacity,
                             int64_t coarse_capacity, void* counters_pinned_host_128, void* stream);
int sfgs_raster_counters_decode(const void* host_128, SfgsRasterCounters* out); /* host only, no GPU work */

/* Copies the plan counters to the host. SYNCHRONISES `stream` (the one host sync of the forward,
 * as in the reference, where the duplicate total sizes the sort buffers). */
int sfgs_raster_read_counters(const void* tiles, SfgsRasterCounters* out, void* stream);
/* Same, through a caller-owned PINNED host buffer of >= 64 bytes (no pageable staging copy: a few
 * microseconds less per frame; the library itself owns no host or device memory). */
int sfgs_raster_read_counters_pinned(const void* tiles, void* pinned_host_64, SfgsRasterCounters* out,
                                     void* stream);

/* Forward, stage 2 ("render"): expand the coarse items into per-tile lists (LDS-ranked), sort each
 * list by (depth, Gaussian index), alpha-composite front to back. Outputs: out_color[3,H,W],
 * out_depth[1,H,W], out_alpha[1,H,W]. num_duplicates = counters.num_duplicates of the plan that
 * filled `bins` (same capacities), or -1 when the caller enqueues the render BEFORE reading the
 * counters (no mid-frame host sync): an overflowing plan is memory-safe -- it drops the items that
 * did not fit -- so the caller may read the counters after the render and redo both stages on
 * overflow. `image` may be NULL when no backward will follow. A plan is SINGLE-USE: the render stage consumes
 * header words of the `tiles` blob (long-list count, longest list) that only a new plan resets; rendering the same plan
 * twice is undefined. Asynchronous. */
int sfgs_raster_forward_render(const SfgsFrame* frame, int32_t N, const void* geom, void* tiles,
                               void* bins, size_t bins_bytes, int64_t dup_capacity,
                               int64_t coarse_capacity, int64_t num_duplicates, float* out_color,
                               float* out_depth, float* out_alpha, void* image, size_t image_bytes,
                               void* stream);

/* Backward of the two calls above. dL_dcolor[3,H,W], dL_ddepth[1,H,W], dL_dalpha[1,H,W] may each
 * be NULL (= zeros). Needs the forward's blobs (geom, tiles, bins with the same capacities, image)
 * and radii unchanged. `dupgrad` is scratch: a 48-byte record and (ABI 18) a one-byte "record written" flag for each
 * duplicate INDEX of the plan, plus one line of zeros -- the indices are handed out from 8 disjoint ranges of
 * [0, dup_capacity), so it spans the capacity, not the count (ask sfgs_raster_sizes(N, W, H, dup_capacity, ..).dupgrad_bytes,
 * do not compute it; the gaps are never touched; nothing in it need survive the call). Every gradient tensor in `grads` is
 * fully overwritten. Deterministic (no float atomics). Asynchronous. Writes one word of the `tiles` header: whether this
 * frame's dead list entries (behind their tile's last contributor) are skipped through the flags or receive zero records
 * one by one; decided per frame on the device, sfgs_set_option("prefill", "always" | "never") forces either path for
 * tests: the gradients are bit-identical. With num_duplicates == 0 `dupgrad` may be NULL or of any size: nothing is read from it
 * or written to it, whatever the option says. */
int sfgs_raster_backward(const SfgsFrame* frame, const SfgsGaussians* g, const int32_t* radii,
                         const void* geom, const void* tiles, const void* bins, int64_t dup_capacity,
                         int64_t coarse_capacity, int64_t num_duplicates, const void* image, const float* dL_dcolor,
                         const float* dL_ddepth, const float* dL_dalpha, void* dupgrad,
                         size_t dupgrad_bytes, const SfgsGaussianGrads* grads, void* stream);

/* ---- One call per stage on ONE scratch allocation (ABI 11) -----------------------------------------------------------
 * The four blobs above as consecutive 256-byte aligned regions of a single caller-owned allocation: the caller asks for
 * the layout once per (N, W, H, capacities) and hands the library one pointer per frame; the library carves it up
 * (still allocates nothing, keeps no state). `with_image` != 0: the frame will be differentiated (image blob included).
 * slot_overhead: sfgs_raster_slot_capacity(W, H, d) == d + slot_overhead (saves the caller a call per frame). */
typedef struct SfgsScratchLayout {
  uint32_t struct_size;
  uint32_t reserved;
  size_t geom_offset, tiles_offset, bins_offset, image_offset;
  size_t total_bytes;      /* size of the allocation (through `bins` without an image, through `image` with one) */
  size_t dupgrad_bytes;    /* separate scratch of the backward (not part of the allocation)                       */
  int64_t coarse_bins;
  int64_t slot_overhead;
} SfgsScratchLayout;
int sfgs_raster_scratch_layout(int32_t N, int32_t W, int32_t H, int64_t dup_capacity, int64_t coarse_capacity,
                               int32_t with_image, SfgsScratchLayout* out);

/* sfgs_raster_forward_plan, hipEventRecord(plan_done_event, stream), sfgs_raster_forward_render(num_duplicates = -1) as
 * ONE call: replaces the autograd forward behind gaussian_renderer/__init__.py:132-140 with a single host -> library
 * transition per frame. plan_done_event: a hipEvent_t (NULL: none); the caller waits on it, decodes
 * counters_pinned_host_128 and redoes the call with larger capacities if the plan overflowed -- the render stage is
 * already running meanwhile. out_* as in sfgs_raster_forward_render. */
int sfgs_raster_forward(const SfgsFrame* frame, const SfgsGaussians* g, int32_t* radii, void* scratch,
                        size_t scratch_bytes, int64_t dup_capacity, int64_t coarse_capacity, int32_t with_image,
                        void* counters_pinned_host_128, void* plan_done_event, float* out_color, float* out_depth,
                        float* out_alpha, void* stream);
/* sfgs_raster_backward on the same allocation (laid out with with_image != 0). */
int sfgs_raster_backward_scratch(const SfgsFrame* frame, const SfgsGaussians* g, const int32_t* radii,
                                 const void* scratch, size_t scratch_bytes, int64_t dup_capacity,
                                 int64_t coarse_capacity, int64_t num_duplicates, const float* dL_dcolor,
                                 const float* dL_ddepth, const float* dL_dalpha, void* dupgrad, size_t dupgrad_bytes,
                                 const SfgsGaussianGrads* grads, void* stream);

/* fused_ssim: mean SSIM (11x11 Gaussian window, sigma 1.5, zero "same" padding, C1=0.01^2,
 * C2=0.03^2 == utils/loss_utils.py:23-63) of img1,img2 [B,C,H,W] float32.
 * forward: writes the mean into *ssim_mean (device float), the per-element map into ssim_map when
 * non-NULL and, when with_grad != 0, the three partial-derivative maps the backward consumes into
 * `scratch` (sfgs_ssim_scratch_bytes). The mean is reduced in a fixed order (bit-reproducible run to run).
 * Numerics: value and gradient are TOLERANCE-equal to the reference formula (utils/loss_utils.py:33-63; tests: 2e-6 on the
 * mean, 5e-5 relative on the gradient), not bit-equal to it nor across ABI 15 -> 16: since ABI 16 the derivative maps use
 * 1/B1 = B2 * inv and 1/B2 = B1 * inv with one reciprocal of B1 * B2 where the reference divides twice, and the 32 x 22
 * tiling sums the mean's partials in a different (fixed) order.
 * backward: dL_dimg1 = *dL_dmean (device float) * d(mean ssim)/d(img1); img2 gets no gradient
 * (it is the ground truth, train.py:222).
 * Limits (SFGS_E_UNSUPPORTED): H * W < 2^30 pixels per plane, at most 2^31 - 1 tiles of 32 x 22 pixels in all. */
size_t sfgs_ssim_scratch_bytes(int32_t B, int32_t C, int32_t H, int32_t W, int32_t with_grad);
int sfgs_ssim_forward(const float* img1, const float* img2, int32_t B, int32_t C, int32_t H,
                      int32_t W, float* ssim_map_or_null, float* ssim_mean, void* scratch,
                      size_t scratch_bytes, int32_t with_grad, void* stream);
int sfgs_ssim_backward(const float* img1, const float* img2, int32_t B, int32_t C, int32_t H,
                       int32_t W, const void* scratch, const float* dL_dmean, float* dL_dimg1,
                       void* stream);

/* Fused training loss (ABI 19): the statements between render() and loss.backward() (train.py:205-234; :760-799 in the
 * IDU episode) as three launches forward and two backward, with no host read of a device value:
 *   x' = mask * image, y' = mask * gt_image, a = mask * gt_depth, b = mask * depth
 *   Ll1 = mean |x' - y'|;   ssim = mean SSIM(x', y') (the fused_ssim kernels' arithmetic: bit-identical to the fused_ssim
 *   value when there is no mask or it is all ones);   r = pearson(a, b) over the pairs the scrub keeps, clamped to [-1, 1]
 *   (torchmetrics' formula on the centred sums, moments accumulated in float64);   depth_loss = 1 - r;
 *   loss = (1 - lambda_dssim) * Ll1 + lambda_dssim * (1 - ssim) + lambda_depth * depth_loss.
 * A pair (a, b) with a non-finite member is scrubbed: SFGS_LOSS_INVALID_ZERO makes it (0, 0) and keeps it in the count
 * (train.py:229-231), _DROP leaves it out (train.py:788-790; n is counted on the device), _KEEP does not scrub. n = 0 or a
 * constant member gives NaN (0 / 0), as in torch. Every reduction runs in a fixed order: bit-reproducible run to run.
 * image, gt_image: [C,H,W] float32. depth, gt_depth: [H*W] float32 (NULL without SFGS_LOSS_DEPTH). mask: NULL
 * (mask_elems 0), ONE device float (mask_elems 1: Camera.original_mask of a view without a mask) or [H*W].
 * SFGS_LOSS_L1_STREAM (alone; no mask; invalid_mode _KEEP): Ll1 = mean |gt_depth - depth| over C*H*W elements of two
 * arbitrary arrays, through the streaming kernels -- the l1_loss drop-in.
 * out5 / grad_out5: five device floats -- loss, Ll1, ssim, depth_loss, r -- and the gradients arriving at them (terms that
 * were not asked for are written as 0). The backward needs the forward's scratch and a with_grad != 0 forward for g_image;
 * g_image [C,H,W], g_depth, g_gt_depth [H*W] may each be NULL (not wanted).
 * SFGS_LOSS_GT_PREMASKED (ABI 23; with SFGS_LOSS_PHOTOMETRIC): gt_image already carries the mask -- y' = gt_image, in the
 * forward and the backward photometric kernels; x', a and b keep their mask. For a target that was resampled AFTER the mask
 * product (sfgs_resample_gt; train.py:207 comes before :215): a masked-out pixel next to kept ones is not zero there. With
 * the bit clear every value and gradient is what ABI 22 computed, bit for bit. */
#define SFGS_LOSS_PHOTOMETRIC 1
#define SFGS_LOSS_DEPTH 2
#define SFGS_LOSS_L1_STREAM 4
#define SFGS_LOSS_GT_PREMASKED 8
#define SFGS_LOSS_INVALID_ZERO 0
#define SFGS_LOSS_INVALID_DROP 1
#define SFGS_LOSS_INVALID_KEEP 2
typedef struct SfgsLossArgs {
  uint32_t struct_size;          /* = sizeof(SfgsLossArgs) */
  int32_t C, H, W;
  const float* image;
  const float* gt_image;
  const float* depth;
  const float* gt_depth;
  const float* mask;
  int64_t mask_elems;            /* 0, 1 or H * W */
  float lambda_dssim, lambda_depth;
  int32_t invalid_mode;          /* SFGS_LOSS_INVALID_*  */
  int32_t terms;                 /* SFGS_LOSS_* bits     */
  int32_t with_grad;             /* forward keeps the three SSIM derivative maps in the scratch */
  int32_t reserved;
} SfgsLossArgs;
size_t sfgs_loss_scratch_bytes(const SfgsLossArgs* args);   /* 0: bad arguments (sfgs_last_error) */
int sfgs_loss_forward(const SfgsLossArgs* args, float* out5, void* scratch, size_t scratch_bytes, void* stream);
int sfgs_loss_backward(const SfgsLossArgs* args, const void* scratch, const float* grad_out5, float* g_image,
                       float* g_depth, float* g_gt_depth, void* stream);

/* Jittered ground truth (ABI 23; csrc/resample.hip): create_offset_gt of train.py:64-77 applied to mask * original_image
 * (train.py:207, 214-215; :770-771 in the IDU episode) -- the target sampled where the jittered rays of
 * SfgsFrame.subpixel_offset went -- in ONE launch, with no pixel grid, no intermediate tensor and no host read:
 *     s = mask * src                                   one rounded float32 product per TAP (the mask is applied first)
 *     u = clamp(x + ox, 0, W - 1), v = clamp(y + oy, 0, H - 1)      grid_sample: bilinear, padding_mode "border",
 *     x0 = floor(u), fx = u - x0, x1 = min(x0 + 1, W - 1)  (y alike)  align_corners = True; the neighbour index is clamped,
 *                                                                    its weight is 0 there: nothing is read out of bounds
 *     out[c][y][x] = ((s[c][y0][x0] (1 - fx)(1 - fy) + s[c][y0][x1] fx (1 - fy)) + s[c][y1][x0] (1 - fx) fy) + s[c][y1][x1] fx fy
 * every operation rounded to float32, nothing contracted. x + ox is formed directly (the reference divides by W - 1 and
 * multiplies back: two more roundings at magnitude W). Non-finite offsets behave as in torch's device grid_sample after its
 * clip: NaN and -inf give 0, +inf gives W - 1 (H - 1). One thread per output pixel, x fastest; deterministic.
 * src, out: [C][H][W] float32, 1 <= C <= 4, H >= 2, W >= 2 (the reference divides by W - 1 and H - 1), C * H * W < 2^31.
 * mask: NULL (mask_elems 0), ONE device float (mask_elems 1) or [H*W] -- SfgsLossArgs.mask's three forms. offset: [H][W][2]
 * float32, channel 0 = x, channel 1 = y. out must not overlap src. No profiler id (as the depthvis kernels). */
typedef struct SfgsResampleArgs {
  uint32_t struct_size;          /* = sizeof(SfgsResampleArgs) */
  int32_t C, H, W;
  const float* src;
  const float* mask;
  int64_t mask_elems;            /* 0, 1 or H * W */
  const float* offset;
} SfgsResampleArgs;
int sfgs_resample_gt(const SfgsResampleArgs* args, float* out, void* stream);

/* Opacity-entropy regulariser (ABI 20): the lambda_opacity term of train.py:236-242 (and :834-843 in the IDU episode),
 *     opacity = gaussians.get_opacity.clamp(1.0e-3, 1.0 - 1.0e-3)
 *     opacity_loss = torch.nn.functional.binary_cross_entropy(opacity, opacity)
 * on the RAW opacity x[n] (float32, or float64 when is_f64 != 0), two launches forward and one backward, no host read of a
 * device value, no N-sized scratch:
 *     o = sigmoid(x), c = min(max(o, lo), hi), inside = (lo <= o <= hi); lo and hi are rounded to x's dtype first, as
 *     torch's clamp does with Python scalars
 *     value = mean over n of h(c),  h(c) = -(c log c + (1 - c) log(1 - c))
 *     grad_raw[i] = g / n * (log(1 - c) - log c) * inside * o (1 - o)     (the cross entropy's derivative with respect to
 *     its input is exactly 0 when input and target are the same tensor; this is the one with respect to its target)
 * evaluated in float64 for both dtypes. A NaN in x gives a NaN value and a NaN in that gradient element only; +-Inf gives a
 * finite value and a zero gradient. The partial sums are reduced in a fixed order: bit-reproducible run to run.
 * out_scalar, grad_out_scalar (one element each, device memory) and grad_raw[n] have the dtype of opacity_raw. The forward's
 * scratch holds its per-block partial sums only; the backward needs none of it, but a with_grad != 0 argument block.
 * Profiler ids (sfgs_profile_kernel_name): opacity_entropy_fwd / _final / _bwd are 27..29, behind the 27 ids of ABI 18 and
 * in front of the five loss kernels of ABI 19, which move to 30..34 and stay the last of the list. Resolve ids by name. */
typedef struct SfgsOpacityEntropyArgs {
  uint32_t struct_size;          /* = sizeof(SfgsOpacityEntropyArgs) */
  int64_t n;                     /* > 0 */
  const void* opacity_raw;       /* device pointer, n elements */
  int32_t is_f64;                /* 0: float32, otherwise float64 */
  double lo, hi;                 /* 0 < lo < hi < 1 (after rounding to the dtype) */
  int32_t with_grad;             /* a backward call will follow */
} SfgsOpacityEntropyArgs;
size_t sfgs_opacity_entropy_scratch_bytes(const SfgsOpacityEntropyArgs* args);   /* 0: bad arguments (sfgs_last_error) */
int sfgs_opacity_entropy_forward(const SfgsOpacityEntropyArgs* args, void* out_scalar, void* scratch, size_t scratch_bytes,
                                 void* stream);
int sfgs_opacity_entropy_backward(const SfgsOpacityEntropyArgs* args, const void* grad_out_scalar, void* grad_raw,
                                  void* stream);

/* Depth colorisation (ABI 21): colorize_depth_torch of render_video.py:129-170 (the same function in
 * render_video_from_ply.py:126-167 and train.py:1001-1041) without leaving the device. With F = float32, every operation
 * rounded to float32, divisions correctly rounded, nothing contracted:
 *     valid = depth > 0 (and mask != 0)                  NaN fails the test; +inf passes and gives disp 0
 *     disp  = F(1) / depth on valid pixels, NaN elsewhere
 *     normalize: lo, hi = the 0.01 and 0.99 quantiles of the valid disparities as numpy's nanquantile ("linear") forms
 *         them on a float32 array: v = the n valid disparities sorted, vi = F(n - 1) * F(q), i = floor(vi), g = vi - i,
 *         a = v[i], b = v[min(i + 1, n - 1)], d = b - a, r = a + d * g, and r = b - d * (1 - g) when g >= 0.5; n = 0: NaN
 *         x = 1 - (disp - lo) / (hi - lo);     otherwise x = 1 - disp
 *     t = x * 256; index k = 255 when t == 256, 0 when t < 0, 255 when t >= 256, trunc(t) otherwise
 *     pixel = lut[k] (lut: [256][3] uint8 on the device), (0, 0, 0) when x is NaN
 * v[i] and v[i + 1] of both quantiles are EXACT order statistics: a three-pass radix select (11 + 11 + 10 bits) over the
 * disparity's bit pattern -- per-workgroup LDS histograms with integer atomics, flushed with integer global atomics, so
 * the result does not depend on arrival order -- with a one-workgroup scan after every pass. Launches on `stream`:
 * one memset of the scratch, three histogram passes, three scans, one colourise pass (normalize = 0: the colourise pass
 * alone; the scratch may then be NULL). The host reads no device value.
 * out_kind SFGS_DEPTHVIS_FLOAT_CHW: out is float32 [3][H][W] with k / 255 (a correctly rounded division), the reference's
 * return value; SFGS_DEPTHVIS_UINT8_HWC: out is uint8 [H][W][3], what a video writer takes. */
#define SFGS_DEPTHVIS_FLOAT_CHW 0
#define SFGS_DEPTHVIS_UINT8_HWC 1
typedef struct SfgsDepthVisArgs {
  uint32_t struct_size;          /* = sizeof(SfgsDepthVisArgs) */
  int32_t H, W;                  /* > 0, H * W <= 2^30 */
  const float* depth;            /* device, [H][W] float32 */
  const unsigned char* mask;     /* device, [H][W] one byte per pixel (bool / uint8), or NULL */
  const unsigned char* lut;      /* device, [256][3] uint8 */
  int32_t normalize;             /* != 0: the two quantiles */
  int32_t out_kind;              /* SFGS_DEPTHVIS_FLOAT_CHW or SFGS_DEPTHVIS_UINT8_HWC */
} SfgsDepthVisArgs;
size_t sfgs_depthvis_scratch_bytes(const SfgsDepthVisArgs* args);   /* 0: bad arguments (sfgs_last_error) */
int sfgs_depthvis_forward(const SfgsDepthVisArgs* args, void* out, void* scratch, size_t scratch_bytes, void* stream);
/* Frame quantiser: image float32 [3][H][W] -> out uint8 [H][W][3] as render_video.py:264 spells it,
 * (img * 255 + 0.5).clip(0, 255).astype(uint8), in float32 (two roundings, truncation). NaN gives 0 (numpy leaves the
 * conversion of NaN undefined). One launch. */
int sfgs_frame_quantize(const float* image, int32_t H, int32_t W, unsigned char* out, void* stream);

/* Evaluation metrics (ABI 25; csrc/metrics.hip): what training_report computes per view (train.py:1064,1075,1090-1091)
 *     image = clamp(render, 0, 1); gt_image = clamp(original_image, 0, 1)
 *     l1_test += l1_loss(image, gt_image).mean().double();  psnr_test += psnr(image, gt_image).mean().double()
 * with l1_loss = mean |a - b| (utils/loss_utils.py:17-18), psnr = 20 log10(1 / sqrt(mse)) per plane and mse = mean (a - b)^2
 * per plane (utils/image_utils.py:14-19), and next to them the SSIM of utils/loss_utils.py:33-63 (the fused_ssim kernels'
 * arithmetic), in TWO launches with no host read of a device value:
 *     SFGS_METRICS_SSIM set: one workgroup per 32 x 22 tile -- ssim.hip's tile, staging, fma chains and tile order -- writes
 *         three float partials per tile: the SSIM sum, sum |a - b|, sum (a - b)^2 (a - b and its square rounded to float32)
 *     clear: a streaming pass (16-byte loads when H * W is a multiple of 4 and both pointers are 16-byte aligned, scalar loads
 *         otherwise) writes float64 partials of sum |a - b| and sum (a - b)^2 per block; a block never straddles two planes
 *     one workgroup then sums every partial in float64 in a fixed order (bit-reproducible: no float atomics) and writes
 *     row8 = [l1, psnr, ssim, mse, psnr_c0, psnr_c1, psnr_c2, psnr_c3]   (float64, device memory):
 *         l1, mse: means over all P * H * W elements;  psnr_c = 20 log10(1 / sqrt(mse_c)) of plane c, in float64;
 *         psnr = mean of the P psnr_c;  ssim = mean of the SSIM map (its float32 rounding is fused_ssim's value bit for bit),
 *         NaN without SFGS_METRICS_SSIM;  psnr_c of planes >= P: NaN.  mse_c = 0 gives +inf; a NaN in plane c gives NaN in
 *         psnr_c, psnr, l1 and mse -- both as the reference's statements do.
 * SFGS_METRICS_CLAMP: both operands are clamped to [0, 1] on their way in, NaN staying NaN as in torch.clamp.
 * SFGS_METRICS_PLANE_MSE: slots 4..7 of the row hold mse_c instead of psnr_c (the utils.image_utils.mse drop-in).
 * a, b: [P][H][W] float32, 1 <= P <= 4, H * W < 2^30 (a plane is at most 2^32 - 1 bytes); the streaming route uses H * W only.
 * No profiler ids (as the depthvis kernels). */
#define SFGS_METRICS_CLAMP 1
#define SFGS_METRICS_SSIM 2
#define SFGS_METRICS_PLANE_MSE 4
typedef struct SfgsMetricsArgs {
  uint32_t struct_size;          /* = sizeof(SfgsMetricsArgs) */
  int32_t P;                     /* planes, 1..4 */
  int32_t H, W;                  /* plane = H x W; the stream route only needs H * W */
  const float* a;
  const float* b;
  int32_t flags;                 /* SFGS_METRICS_* bits */
  int32_t reserved;
} SfgsMetricsArgs;
size_t sfgs_metrics_scratch_bytes(const SfgsMetricsArgs* args);   /* 0: bad arguments (sfgs_last_error) */
int sfgs_metrics_view(const SfgsMetricsArgs* args, double* row8, void* scratch, size_t scratch_bytes, void* stream);

/* Similarity transform of a Gaussian scene (ABI 26; csrc/transform.hip): x' = s R x + t applied to everything a trained scene
 * carries that depends on its frame. The reference trains every satellite scene in a frame of its own (readSatelliteInfo,
 * scene/dataset_readers.py:378-390: rotated by the dataset's R / T, scaled to a 99th-percentile radius of 256, dropped so that
 * the 1st percentile of z is 0), so two trained tiles differ by a full similarity; this is how they get into one frame.
 * Per Gaussian, every pair (in, out) optional -- a pair with a NULL `in` is skipped -- and out == in allowed:
 *     xyz [N][3]        out = s * ((R[0] x + R[1] y) + R[2] z per row of R) + t       (product with s after the dot product)
 *     scaling [N][3]    SFGS_SIM_SCALING_LOG set: out = in + log_s (the model's _scaling, a fused PLY's scale_*);  clear: out = in * s
 *     rotation [N][4]   (w, x, y, z), as given, not renormalised: out = q_R (x) q (Hamilton product, q_R on the left)
 *     sh_rest           sh_rest_coeffs in {0, 3, 8, 15} coefficients per channel beyond DC, [N][K-1][3] (the model's
 *                       _features_rest) or, with SFGS_SIM_REST_N3K, [N][3][K-1] (a fused PLY's f_rest_* order,
 *                       scene/gaussian_model.py:461-467): the coefficients of band l = 1, 2, 3 are multiplied by D_l per channel,
 *                       out_i = sum_j D_l[i][j] in_j, whatever the active degree is
 *     filter_3D [N][1]  out = in * s
 * DC colour and opacity do not change (the 3D filter's opacity compensation is scale-invariant) and are not passed. D_l is the
 * real-SH rotation matrix of band l in the basis order and signs of eval_sh (utils/sh_utils.py:57-112):
 * eval_sh(D sh, R d) == eval_sh(sh, d) for every unit d. All constants travel by value as float32; the caller forms them in
 * float64 and rounds once. Arithmetic: float32, products and sums as written, sums in index order from the first term,
 * nothing contracted; no atomics. ONE launch, no scratch: a workgroup stages the contiguous block of 256 rows of xyz and
 * sh_rest through LDS (coalesced 16-byte global accesses; a lane then walks its own row at an odd dword stride, which is
 * conflict-free), scaling and filter_3D are elementwise, a quaternion is one 16-byte access. No profiler id. */
#define SFGS_SIM_SCALING_LOG 1
#define SFGS_SIM_REST_N3K 2
typedef struct SfgsSimilarityArgs {
  uint32_t struct_size;          /* = sizeof(SfgsSimilarityArgs) */
  int32_t flags;                 /* SFGS_SIM_* bits */
  int64_t n;                     /* Gaussians, 0 <= n < 2^31 (0: nothing is launched) */
  int32_t sh_rest_coeffs;        /* K - 1: 0, 3, 8 or 15 (0: sh_rest is not touched) */
  int32_t reserved;
  const float* xyz_in;       float* xyz_out;
  const float* scaling_in;   float* scaling_out;
  const float* rotation_in;  float* rotation_out;
  const float* sh_rest_in;   float* sh_rest_out;
  const float* filter3d_in;  float* filter3d_out;
  float R[9];                    /* row-major */
  float s, log_s;
  float t[3];
  float q[4];                    /* the rotation's quaternion (w, x, y, z) */
  float D1[9], D2[25], D3[49];   /* row-major */
} SfgsSimilarityArgs;
int sfgs_similarity_transform(const SfgsSimilarityArgs* args, void* stream);

/* ---- Geometry evaluation (ABI 22; csrc/geometry.hip): evaluate_gs_geometry.py + dsmr.py without their host stages ----------
 * Stage 1, depth map -> height grid (DSM). One call per view into the SAME accumulators; the merged point cloud is never
 * formed. A pixel is used when depth > 0, the depth is finite and the mask (one byte per pixel, or NULL) is non-zero. (The
 * reference's test is depth > 0 alone, which accepts +inf; its caller scrubs +inf to 0 first.) All arithmetic is float64 in
 * the reference's order (:173-204), nothing contracted:
 *     z = depth, x = (col - cx_pix) * z / focal_x, y = (row - cy_pix) * z / focal_y
 *     w_j = ((x M[0][j] + y M[1][j]) + z M[2][j]) + c[j], then + origin[j] as a rounding step of its own   (east, north, up)
 *     gx = (int)((east - xoff) / resolution), gy = (int)((yoff_top - north) / resolution)       truncation toward zero
 * M is R transposed (row-major), c = -(M T) and cx_pix = cx / 2 * W + W / 2 (cy_pix alike) are formed by the caller in
 * float64. A point whose cell lies outside [0, xsize) x [0, ysize) is dropped before any atomic; (-1, 0) truncates to 0,
 * as in the reference. *num_points (device, uint64) counts the points that landed.
 * SFGS_DSM_MAX: acc is uint64 [ysize][xsize], zeroed by the caller; every point takes an atomic max with an order-preserving
 * integer key of its height (0 = empty). SFGS_DSM_MEAN: acc is int64 [ysize][xsize] of heights in units of 2^-20 m
 * (round to nearest), count uint32 [ysize][xsize], both zeroed by the caller; a point adds to every cell within `radius`
 * (0 ... 3) columns and rows of its own that lies inside the grid. Integer atomics only: both modes give the same bits
 * whatever the arrival order. sfgs_dsm_finalize writes float64 [ysize][xsize]: the maximum / sum / count, NaN where empty. */
#define SFGS_DSM_MAX 0
#define SFGS_DSM_MEAN 1
typedef struct SfgsDsmViewArgs {
  uint32_t struct_size;          /* = sizeof(SfgsDsmViewArgs) */
  int32_t H, W;                  /* > 0, H * W <= 2^30 */
  const float* depth;            /* device, [H][W] float32 */
  const unsigned char* mask;     /* device, [H][W] one byte per pixel, or NULL */
  double M[9];                   /* camera-to-world rotation, row-major: world = cam @ M + c */
  double c[3];                   /* camera centre */
  double origin[3];              /* added after c (the ENU -> UTM translation); zeros for none */
  double cx_pix, cy_pix, focal_x, focal_y;
  double xoff, yoff_top, resolution;
  int32_t xsize, ysize;          /* > 0, xsize * ysize <= 2^28 */
  int32_t mode;                  /* SFGS_DSM_MAX or SFGS_DSM_MEAN */
  int32_t radius;                /* mean mode: 0 ... 3 */
} SfgsDsmViewArgs;
int sfgs_dsm_accumulate(const SfgsDsmViewArgs* args, void* acc, uint32_t* count, unsigned long long* num_points, void* stream);
int sfgs_dsm_finalize(int32_t mode, int32_t xsize, int32_t ysize, const void* acc, const uint32_t* count, double* out,
                      void* stream);
/* Stage 2, dsmr.compute_shift(ref, sec) on float64 rasters of their own shapes (valnan checks each by its own shape).
 * Pyramid: while min(ref_h, ref_w) > 100 both rasters are halved by downsample2x (output ceil(H / 2) x ceil(W / 2); cell
 * (J, I) = the mean of the finite pixels of the 2 x 2 window whose corner is (min(2J + 1, H - 1), min(2I + 1, W - 1)):
 * the reference's loop lets the last write win); the start (init_dx, init_dy) is floor-halved per level on the way down,
 * a level starts at twice the result of the level below, read from device memory. Per level: for every shift of
 * start +- irange, mean_std over the pixels (i, j) of ref paired with sec(i + dx, j + dy), pairs with both values finite
 * (NaN and +-inf are skipped): means first, then centred sums, sigma = sqrt(sum / count), xcorr = sum / count, score =
 * xcorr / (sigma_u sigma_v); scan y outer, x inner, update on strict >. A shift with no finite pair or with
 * sigma_u sigma_v == 0 -- where the reference divides by zero -- is skipped. shift_out: int32 [2] = (dx, dy);
 * stats_out: float64 [8] = a, b, mu_u, mu_v, sigma_u, sigma_v, xcorr, score at that shift, a = sigma_u / sigma_v with
 * `scaling`, else 1, b = mu_u - mu_v a. Every shift skipped: (dx, dy) = the start, b and the statistics NaN.
 * Sums are per 32 x 32 tile of ref, added in tile order by one workgroup: no float atomics, the same bits every run. */
typedef struct SfgsDsmrArgs {
  uint32_t struct_size;          /* = sizeof(SfgsDsmrArgs) */
  int32_t ref_h, ref_w, sec_h, sec_w;   /* 1 ... 32768 */
  const double* ref;             /* device, [ref_h][ref_w] float64 */
  const double* sec;             /* device, [sec_h][sec_w] float64 */
  int32_t irange;                /* 1 ... 7 */
  int32_t scaling;
  int32_t init_dx, init_dy;      /* recursive_ncc's dx, dy arguments (compute_shift passes 0, 0) */
} SfgsDsmrArgs;
size_t sfgs_dsmr_scratch_bytes(const SfgsDsmrArgs* args);   /* 0: bad arguments (sfgs_last_error) */
int sfgs_dsmr_register(const SfgsDsmrArgs* args, int32_t* shift_out, double* stats_out, void* scratch, size_t scratch_bytes,
                       void* stream);
/* Stage 3. dsmr.apply_shift_ with c = d = 0: out(i, j) = a sec(i + dx, j + dy) + b, NaN outside; shift int32 [2] and
 * ab float64 [2] on the device. compute_dsm_metrics + register_dsms_simple: pred and gt float64 [H][W], mask one byte per
 * pixel (non-zero = keep) or NULL, shift / ab both NULL or both set (the shifted prediction is formed on the fly);
 * valid = not NaN. out: float64 [5] = mae, rmse, valid_pixels, completeness (0 when gt has no valid pixel), mean of
 * gt - pred over the pixels valid in both (0 when none). No valid pixel: NaN, NaN, 0, 0. Per-workgroup partials added in
 * a fixed order. */
int sfgs_dsm_apply_shift(const double* sec, int32_t H, int32_t W, const int32_t* shift, const double* ab, double* out,
                         void* stream);
size_t sfgs_dsm_metrics_scratch_bytes(int32_t H, int32_t W);   /* 0: bad arguments */
int sfgs_dsm_metrics(const double* pred, const double* gt, const unsigned char* mask, int32_t H, int32_t W,
                     const int32_t* shift, const double* ab, double* out, void* scratch, size_t scratch_bytes, void* stream);

/* ---- Merged point cloud (ABI 27; csrc/pointcloud.hip): depth_to_point_cloud per view + np.vstack over the views
 * (evaluate_gs_geometry.py:132-215, :776), the file and the bounds the script prints (:779-790), with no host read per view.
 * The pixel rule and the float64 arithmetic are stage 1's above (one device function serves both files): a pixel is used when
 * depth > 0, the depth is finite and the mask is non-zero or NULL; +inf is dropped.
 * sfgs_pointcloud_append adds ONE view in three launches: per-workgroup counts of used pixels (256 pixels each); one
 * workgroup scans them exclusively, 1024 at a time with a carry that starts at *state, and advances *state by the view's
 * count; the scatter pass ranks the used pixels inside each workgroup and writes points[row] = (east, north, up) as float64
 * and, with colours, colors[row] = three uint8 quantised from image [3][H][W] float32 by sfgs_frame_quantize's rule. Rows keep
 * the view's row-major pixel order and a view's rows follow the previous view's: points[0 .. n) IS the reference's vstack.
 * No kernel waits for another workgroup.
 *   state     device, ONE uint64 the caller zeroes before the first view: the points SEEN so far. A row >= capacity is not
 *             written but still counted, so *state > capacity tells the caller afterwards which capacity would have sufficed.
 *   points    device, float64 [capacity][3];  colors: device, uint8 [capacity][3], given exactly when args->image is.
 *   scratch   sfgs_pointcloud_scratch_bytes bytes for the view's H, W (8 bytes per 256 pixels, at least 48 KiB), 8-byte aligned;
 *             what it answers for ANY valid H, W is enough for sfgs_pointcloud_bounds.
 * sfgs_pointcloud_bounds writes out6 = (min east, north, up, max east, north, up) over the min(*state, capacity) stored rows:
 * per-workgroup partials, folded by one workgroup in a fixed order (no float atomics); a NaN coordinate gives NaN, as numpy's
 * min / max; an empty cloud gives +inf / -inf.
 * Every refusal of these entry points is SFGS_E_ARG, made before any GPU work: a NULL pointer, H or W < 1 or H * W > 2^30, a zero
 * focal length, a negative capacity, a scratch that is too small, a wrong struct_size. No profiler ids. */
typedef struct SfgsPointCloudViewArgs {
  uint32_t struct_size;          /* = sizeof(SfgsPointCloudViewArgs) */
  int32_t H, W;                  /* > 0, H * W <= 2^30 */
  const float* depth;            /* device, [H][W] float32 */
  const unsigned char* mask;     /* device, [H][W] one byte per pixel, or NULL */
  const float* image;            /* device, [3][H][W] float32, or NULL (no colours) */
  double M[9];                   /* camera-to-world rotation, row-major: world = cam @ M + c */
  double c[3];                   /* camera centre */
  double origin[3];              /* added after c (the ENU -> UTM translation); zeros for none */
  double cx_pix, cy_pix, focal_x, focal_y;
} SfgsPointCloudViewArgs;
size_t sfgs_pointcloud_scratch_bytes(int32_t H, int32_t W);   /* 0: bad arguments (sfgs_last_error) */
int sfgs_pointcloud_append(const SfgsPointCloudViewArgs* args, double* points, unsigned char* colors, int64_t capacity,
                           unsigned long long* state, void* scratch, size_t scratch_bytes, void* stream);
int sfgs_pointcloud_bounds(const double* points, const unsigned long long* state, int64_t capacity, double* out6, void* scratch,
                           size_t scratch_bytes, void* stream);

/* ---- True orthophoto on the DSM's grid (added under ABI 28: new symbols only; csrc/ortho.hip; Python: sfgs.ortho): per cell
 * the colour of the HIGHEST point the views put there. The pixel rule, the float64 arithmetic and the cell rule are stage 1's
 * of the geometry evaluation above (one device function each serves both files), so with the same camera numbers the cells
 * agree with SFGS_DSM_MAX's bit for bit. One call per view into the SAME accumulator:
 *   acc   device, uint64 [ysize][xsize], zeroed by the caller; 0 = empty. Every landed point takes a 64-bit integer atomic max with
 *         bits 63-32  K32(float32(up)): float32() rounds the float64 height to nearest even; on its bit pattern b,
 *                     K32(b) = (b >> 31) ? ~b : (b | 0x80000000) -- order preserving, and no number maps to 0
 *         bits 31-24, 23-16, 15-8   r, g, b of the pixel from image [3][H][W] by the frame quantiser's rule
 *                     (float32 v * 255 + 0.5, clip to 0 ... 255, truncate, NaN -> 0)
 *         bits 7-0    the view's tag, 1 ... 255
 *         The winner of a cell is the maximum over (float32 height, r, g, b, tag), lexicographically: heights that differ
 *         only below float32 resolution tie and colour decides, then the tag. Rounding is monotone, so the winner's height is
 *         float32(SFGS_DSM_MAX's height) in every cell. A point whose float64 height is not finite is dropped.
 *   *num_points (device, uint64) counts the points that landed. Integer atomics only: any view order gives the same bits.
 * The resolve call, ONE launch, unpacks acc; with fill r = 1 ... 3 an EMPTY cell takes the maximum key among the non-empty
 * cells of its (2r + 1)^2 window clipped to the grid (a single pass: donated values do not propagate):
 *   rgb      uint8 [ysize][xsize][3], 0 where empty        height  float32 [ysize][xsize], NaN where empty
 *   source   uint8 [ysize][xsize]: the winning tag, 0 where empty       state  uint8 [ysize][xsize]: 0 empty, 1 own, 2 donated
 *   coverage uint64 [256], zeroed by the caller (the call ADDS): [0] cells still empty, [t] cells coloured by tag t, own or donated
 * Limits, status codes and messages are those of the two DSM entry points; a tag outside 1 ... 255 and a fill outside
 * 0 ... 3 are SFGS_E_ARG. No profiler ids. */
typedef struct SfgsOrthoViewArgs {
  uint32_t struct_size;          /* = sizeof(SfgsOrthoViewArgs) */
  int32_t H, W;                  /* > 0, H * W <= 2^30 */
  const float* depth;            /* device, [H][W] float32 */
  const unsigned char* mask;     /* device, [H][W] one byte per pixel, or NULL */
  double M[9];                   /* camera-to-world rotation, row-major: world = cam @ M + c */
  double c[3];                   /* camera centre */
  double origin[3];              /* added after c (the ENU -> UTM translation); zeros for none */
  double cx_pix, cy_pix, focal_x, focal_y;
  double xoff, yoff_top, resolution;
  int32_t xsize, ysize;          /* > 0, xsize * ysize <= 2^28 */
  const float* image;            /* device, [3][H][W] float32 */
  int32_t tag;                   /* 1 ... 255 */
} SfgsOrthoViewArgs;
int sfgs_ortho_accumulate(const SfgsOrthoViewArgs* args, void* acc, unsigned long long* num_points, void* stream);
int sfgs_ortho_resolve(int32_t xsize, int32_t ysize, int32_t fill, const void* acc, unsigned char* rgb, float* height,
                       unsigned char* source, unsigned char* state, unsigned long long* coverage, void* stream);

/* ---- Multi-view depth consistency masks (added under ABI 28: new symbols only; csrc/consistency.hip; Python: sfgs.consistency):
 * the per-view pixel mask the three geometry products above take. A rendered depth is an alpha-blended expectation: at a roof
 * edge it mixes roof and ground and unprojects to a point in mid-air. A pixel of view i is kept when at least min_views OTHER
 * views see the same surface there. float64 throughout, nothing contracted, products, sums and quotients in the order written.
 *   project(k, w):  q_n = w_n - c_k[n];  cam_a = (q_0 M_k[3a] + q_1 M_k[3a+1]) + q_2 M_k[3a+2];  z = cam_2;
 *                   u = cam_0 focal_x / z + cx_pix;  v = cam_1 focal_y / z + cy_pix
 *   unproject(k, row, col, d): stage 1's of the geometry evaluation above (the same device function), origin = 0.
 *   A pixel is USED by stage 1's rule: depth > 0, finite, mask byte (if any) non-zero.
 * For pixel (r, c) of the reference view i: not used -> count = keep = 0. Otherwise w = unproject(i, r, c, d) and every
 * j != i, ascending, is accepted if all of these hold in turn:
 *   (u, v, z) = project(j, w), z > 0;
 *   fu = floor(u + 0.5), fv = floor(v + 0.5), 0 <= fu < W_j, 0 <= fv < H_j (tested on the doubles; NaN fails);
 *   pixel (fv, fu) of j is used, with depth d_j;
 *   |(double)d_j - z| <= rel_tol * z;
 *   w' = unproject(j, fv, fu, d_j), (u', v', z') = project(i, w'), z' > 0 and (u' - c)^2 + (v' - r)^2 <= px_tol2.
 * count[r][c] = the accepted sources (<= 255), keep[r][c] = count >= min_views; one byte each.
 * The views live in a DEVICE table of V records, written once per set by the caller (sfgs_consistency_table_check vets the
 * host copy before it is uploaded: V, sizes, NULL depth, zero focal lengths); sfgs_consistency_check is ONE launch for one
 * reference view, a thread per pixel, no atomics, no host read, no synchronise: two runs give the same bytes.
 * args->H, W size the launch and the two outputs; they must be record `ref`'s (the kernel compares and writes nothing otherwise).
 * Refusals are SFGS_E_ARG, made before any GPU work. No profiler ids. */
typedef struct SfgsConsistencyView {
  const float* depth;            /* device, [H][W] float32 */
  const unsigned char* mask;     /* device, [H][W] one byte per pixel, or NULL */
  int32_t H, W;                  /* > 0, H * W <= 2^30 */
  double M[9];                   /* camera-to-world rotation, row-major: world = cam @ M + c (orthonormal) */
  double c[3];                   /* camera centre */
  double cx_pix, cy_pix, focal_x, focal_y;
} SfgsConsistencyView;
typedef struct SfgsConsistencyArgs {
  uint32_t struct_size;          /* = sizeof(SfgsConsistencyArgs) */
  int32_t V;                     /* records in the table, 2 ... 256 */
  int32_t ref;                   /* the reference view, 0 ... V - 1 */
  int32_t H, W;                  /* of the reference view */
  int32_t min_views;             /* >= 1 */
  const void* table;             /* device, SfgsConsistencyView [V], 8-byte aligned */
  double rel_tol;                /* finite, > 0 */
  double px_tol2;                /* the pixel tolerance SQUARED, > 0; +inf: no bound on the round trip (z' > 0 still holds) */
} SfgsConsistencyArgs;
int sfgs_consistency_table_check(const SfgsConsistencyView* host_views, int32_t V);
int sfgs_consistency_check(const SfgsConsistencyArgs* args, unsigned char* count, unsigned char* keep, void* stream);

/* ---- TSDF fusion and mesh extraction (added under ABI 28: new symbols only; csrc/tsdf.hip, csrc/tsdf_math.h; Python: sfgs.tsdf):
 * depth views -> a truncated signed distance volume -> a triangle soup by marching tetrahedra. The volume is axis-aligned in the
 * cameras' frame: voxel (i, j, k) has its centre at origin + (i + 0.5, j + 0.5, k + 0.5) * voxel_size, formed in float64 as
 * written; storage is planar float32, x fastest: tsdf [nz][ny][nx], weight [nz][ny][nx], rgb [3][nz][ny][nx] (or NULL).
 * INTEGRATION, sfgs_tsdf_integrate: ONE launch for V <= 256 views held in a device table (sfgs_tsdf_table_check vets the host copy
 * first, with with_images = (vol->rgb != NULL): the library cannot read the device copy). A thread owns one voxel, keeps (D, W, rgb) in registers and walks the views in ascending order; float64 on the stored
 * float32 values, nothing contracted; project() and the USED rule are those of the consistency check above (the same device functions):
 *   (u, v, z) = project(view, centre); leave unless z > 0;
 *   fu = floor(u + 0.5), fv = floor(v + 0.5); leave unless 0 <= fu < W and 0 <= fv < H (tested on the doubles; NaN fails);
 *   leave unless pixel (fv, fu) is used, with depth d;   sdf = (double)d - z; leave if sdf < -trunc;   s = min(1, sdf / trunc);
 *   D = float32((W D + s) / (W + 1));  with colours, per channel, C = float32((W C + image[ch][fv][fu]) / (W + 1));
 *   W = float32(min(W + 1, max_weight)).
 * A voxel is stored only if some view updated it. No atomics, no workgroup waits for another; a voxel's bits depend on the order
 * of the views alone, so one call with all views, one call per view and any split of the list give the same bytes.
 * EXTRACTION, sfgs_tsdf_extract, three launches. Cell (x, y, z) spans voxels x..x+1, y..y+1, z..z+1; cells are numbered in the
 * volume's linear order over (nz-1, ny-1, nx-1); a cell is used only if all eight corner weights are > 0. Corner k has the offsets
 * (k & 1, (k >> 1) & 1, (k >> 2) & 1). The six tetrahedra are the corner paths (0, 1<<a, (1<<a)|(1<<b), 7) over the permutations
 * (a, b, c) of (0, 1, 2) in lexicographic order; the local vertices 0..3 of a tetrahedron are its path. A vertex is inside when
 * its value is < 0 (0 is outside). The point on the edge of local vertices l < m, float32 as written, a = vertex l, b = vertex m:
 *   t = va / (va - vb);  pos = pa + t * (pb - pa) per axis in voxel-index units;  world = float32(origin) + (pos + 0.5) * float32(voxel_size);
 *   colour = ca + t * (cb - ca) per channel
 * (the same bytes from every tetrahedron that shares the edge: the soup welds by byte equality). Triangles of a tetrahedron:
 *   one inside, vertex i: the edge points (i, j), j ascending;   three inside, outside vertex o: the edge points (i, o), i ascending;
 *   two inside, i0 < i1, o0 < o1: q0 = (i0, o0), q1 = (i0, o1), q2 = (i1, o1), q3 = (i1, o0): (q0, q1, q2) and (q0, q2, q3);
 * then the last two vertices are swapped where a 6 x 16 bit table says so, so that (b - a) x (c - a) points toward positive values.
 * Pass 1 counts the triangles of each workgroup of 256 consecutive cells (0 ... 12 per cell); pass 2, ONE workgroup, scans the
 * counts 1024 at a time with a carry and leaves the total in *state; pass 3 writes each workgroup's triangles as one run:
 *   vertices  float32 [capacity][3][3], colors float32 [capacity][3][3] (given exactly when vol->rgb is), ordered by cell, then
 *             tetrahedron, then triangle. A row at or beyond capacity is not written; *state counts it all the same.
 *   scratch   sfgs_tsdf_scratch_bytes bytes for the volume's dims, 8-byte aligned.
 * Refusals are SFGS_E_ARG, made before any GPU work: a NULL pointer, a wrong struct_size, a dimension < 1 or nx ny nz > 2^30,
 * voxel_size or trunc not finite and > 0, max_weight < 1 or NaN, V outside 1 ... 256, a record with H or W < 1, H W > 2^30, a NULL
 * depth, a zero focal length, an image pointer that does not go with vol->rgb, a negative capacity, a scratch too small. No profiler ids. */
typedef struct SfgsTsdfView {
  const float* depth;            /* device, [H][W] float32 */
  const unsigned char* mask;     /* device, [H][W] one byte per pixel, or NULL */
  const float* image;            /* device, [3][H][W] float32, or NULL (a volume without colours) */
  int32_t H, W;                  /* > 0, H * W <= 2^30 */
  double M[9];                   /* camera-to-world rotation, row-major: world = cam @ M + c (orthonormal) */
  double c[3];                   /* camera centre */
  double cx_pix, cy_pix, focal_x, focal_y;
} SfgsTsdfView;
typedef struct SfgsTsdfVolume {
  uint32_t struct_size;          /* = sizeof(SfgsTsdfVolume) */
  int32_t nx, ny, nz;            /* > 0, nx * ny * nz <= 2^30 */
  double origin[3];              /* the corner of voxel (0, 0, 0) */
  double voxel_size;             /* finite, > 0 */
  double trunc;                  /* finite, > 0 */
  double max_weight;             /* >= 1 (+inf: no cap) */
  float* tsdf;                   /* device, [nz][ny][nx] */
  float* weight;                 /* device, [nz][ny][nx] */
  float* rgb;                    /* device, [3][nz][ny][nx], or NULL */
} SfgsTsdfVolume;
int sfgs_tsdf_table_check(const SfgsTsdfView* host_views, int32_t V, int32_t with_images);
int sfgs_tsdf_integrate(const SfgsTsdfVolume* vol, const void* table, int32_t V, void* stream);
size_t sfgs_tsdf_scratch_bytes(int32_t nx, int32_t ny, int32_t nz);   /* 0: bad arguments (sfgs_last_error) */
int sfgs_tsdf_extract(const SfgsTsdfVolume* vol, float* vertices, float* colors, int64_t capacity, unsigned long long* state,
                      void* scratch, size_t scratch_bytes, void* stream);

/* ---- TSDF ray-casting (added under ABI 28: new symbols only; csrc/tsdf.hip, csrc/tsdf_math.h; Python: TsdfVolume.raycast): the
 * volume seen from a camera -- depth along the forward axis, the world-frame normal toward the free side and the colour of the
 * first surface along each pixel's ray. sfgs_tsdf_raycast is ONE launch, a thread per pixel; tests/tsdf_raycast_np.py states the
 * sequence in numpy and the kernel equals it byte for byte. Float64 on the stored float32 values, in the order written, nothing
 * contracted; lerp(a, b, f) = a + f * (b - a).
 *   1. ray of pixel (row, col): x = (col - cx_pix) / focal_x, y = (row - cy_pix) / focal_y, d[a] = (x M[a] + y M[3 + a]) + M[6 + a];
 *      the point at depth z is p[a] = c[a] + z d[a] (M, c as in SfgsTsdfView).
 *   2. clip to the box of voxel centres, per axis lo = origin + 0.5 voxel_size, hi = origin + (n - 0.5) voxel_size: with
 *      d[a] == 0 the ray misses unless lo <= c[a] <= hi; otherwise t0 = (lo - c[a]) / d[a], t1 = (hi - c[a]) / d[a], swapped if
 *      t0 > t1, then if (t0 > z0) z0 = t0, if (t1 < z1) z1 = t1, from z0 = near and z1 = far. The ray misses unless z0 <= z1 (NaN
 *      fails). A volume with a dimension of 1 has no cell: every ray misses, nothing is launched.
 *   3. samples z_k = z0 + (double)k step, k = 0 ... K - 1, K = floor((z1 - z0) / step) + 1, capped at 2^20 on the double.
 *   4. a sample: per axis g = (p - origin) * inv_voxel - 0.5 with inv_voxel = 1.0 / voxel_size formed once on the host; i = floor(g)
 *      clamped to [0, n - 2] on the double, f = g - i clamped to [0, 1]. It is VALID when the eight corner weights of cell i are
 *      > 0 (extraction's rule). With v0 ... v7 the corner values (corner k at the offsets (k & 1, (k >> 1) & 1, (k >> 2) & 1)):
 *        x00 = lerp(v0, v1, fx), x10 = lerp(v2, v3, fx), x01 = lerp(v4, v5, fx), x11 = lerp(v6, v7, fx),
 *        y0 = lerp(x00, x10, fy), y1 = lerp(x01, x11, fy), val = lerp(y0, y1, fz);
 *        gz = y1 - y0, gy = lerp(x10 - x00, x11 - x01, fz), gx = lerp(lerp(v1 - v0, v3 - v2, fy), lerp(v5 - v4, v7 - v6, fy), fz);
 *      a colour channel takes the value's sequence on its plane.
 *   5. the hit is the smallest k >= 1 whose sample is valid with val < 0 and whose predecessor k - 1 is valid with val >= 0
 *      (a zero is outside, as in extraction). Nothing else ends a ray: not a first sample that is already negative, not an
 *      unobserved gap, not a crossing from negative to positive.
 *   6. with vp, vc the two values, w = vp / (vp - vc): depth = (float)(z_{k-1} + w (z_k - z_{k-1})); g = gp + w (gc - gp) per
 *      component, len = sqrt((gx gx + gy gy) + gz gz), normal = (float)(g / len), zeros unless len > 0; rgb = (float)(cp + w (cc - cp)).
 *      A pixel without a hit gets zeros in every output. No output reads an unobserved voxel.
 *   7. empty-space skipping changes no byte. The table (sfgs_tsdf_skip_build, one launch, a workgroup per brick, no atomics) has
 *      one byte per brick of 8 x 8 x 8 cells, laid out [bz][by][bx] over the (n - 1) cells per axis, non-zero when some voxel
 *      of the brick's footprint -- voxels 8b ... min(8b + 8, n - 1) per axis -- has weight > 0 && tsdf < 0. A trilinear value
 *      of non-negative corners is non-negative in this lerp form (rounding is monotone), so a sample whose cell lies in a brick
 *      with a zero byte is never the negative end of a hit and is not evaluated. The march visits k in ascending order; from a
 *      sample in such a brick it proposes a jump of j lattice steps from the ray's exit of the brick's slab and takes it only
 *      after the cell of sample k + j has been recomputed and found in the same brick (a cell coordinate is monotone in k, so
 *      equal ends mean an equal interior); otherwise it advances by one. A valid negative sample whose predecessor was skipped has
 *      that predecessor evaluated on demand. The table describes the volume as it was when built; skip == NULL marches every sample.
 *   depth   float32 [H][W]; normal float32 [3][H][W] or NULL; rgb float32 [3][H][W], NULL exactly when vol->rgb is.
 *   step    measured along the forward axis, like the depths; the library refuses a step so small that the box diagonal
 *           holds more than 2^20 of them.
 * Refusals are SFGS_E_ARG, made before any GPU work: what SfgsTsdfVolume is refused for, a NULL pointer, a wrong struct_size,
 * H or W < 1, H W > 2^30, a non-finite M, c or principal point, a focal length that is zero or not finite, near < 0 or not finite,
 * far <= near or NaN, a step that is not finite and > 0 or too small, an rgb pointer that does not go with vol->rgb, a table
 * smaller than sfgs_tsdf_skip_bytes. No profiler ids. */
typedef struct SfgsTsdfRay {
  uint32_t struct_size;          /* = sizeof(SfgsTsdfRay) */
  int32_t H, W;
  double M[9];                   /* world = cam @ M + c */
  double c[3];
  double cx_pix, cy_pix, focal_x, focal_y, near, far, step;
  float* depth;                  /* device, [H][W] */
  float* normal;                 /* device, [3][H][W], or NULL */
  float* rgb;                    /* device, [3][H][W]; NULL exactly when the volume has no colours */
} SfgsTsdfRay;
size_t sfgs_tsdf_skip_bytes(int32_t nx, int32_t ny, int32_t nz);      /* 0: bad arguments (sfgs_last_error) */
int sfgs_tsdf_skip_build(const SfgsTsdfVolume* vol, void* skip, size_t bytes, void* stream);
int sfgs_tsdf_raycast(const SfgsTsdfVolume* vol, const SfgsTsdfRay* ray, const void* skip, size_t skip_bytes, void* stream);

/* ---- Mesh: weld, components, clean (added under ABI 28: new symbols only; csrc/mesh.hip, csrc/mesh_math.h; Python: sfgs.mesh):
 * the triangle soup finished on the device. Results are integers and copied bytes; tests/mesh_np.py states them in numpy and the
 * kernels equal that restatement byte for byte, run after run. A `state` is four int64 words on the device, rewritten by every call:
 * word 0 and 1 are counts (below), word 2 is a status (0: every loop ran to its end; bit 0 / 1 / 2: a probe, a find chain or a
 * row of failed hooks reached its trip bound -- the slot count, m, 2^16 -- which valid input cannot; bit 3: a face index outside
 * 0 ... m - 1 was met, its face skipped), word 3 is the weld's diagnostic.
 * WELD, sfgs_mesh_weld. soup: float32 [n][3][3], the flat vertex index is q = 3 t + c; soup_colors: the same shape, or NULL.
 *   key(q) is the three 32-bit words of soup[q] compared as BIT PATTERNS (-0.0 differs from +0.0, NaNs are equal when their bits are);
 *   rep(q) = the smallest q' with key(q') == key(q); unique vertices are numbered in order of first appearance,
 *   vid(q) = the number of representatives below rep(q). Outputs: vertices float32 [>= m][3] with vertices[vid] = soup[rep],
 *   colors[vid] = soup_colors[rep] (given exactly when soup_colors is), faces int32 [n][3] with faces[t][c] = vid(3 t + c), state
 *   word 0 = m, word 1 = n. m <= 3 n: buffers of 3 n rows always suffice. 0 <= n <= 2^29; n = 0 writes the state and launches nothing.
 *   Mechanism: an open-addressing table of 32-bit slots holding soup vertex indices in `scratch` (the power of two >= 6 n slots),
 *   linear probing, compare-and-swap into an empty slot, fetch-min on a slot whose witness has the same words; then the row
 *   compaction below on the flags q == rep(q). flags: bit 0 = also sum the slots every insertion looked at into state word 3.
 * VET, sfgs_mesh_vet: state of a caller's indexed mesh -- word 0 = m, word 1 = n, status bit 3 if a face index is out of range.
 * COMPONENTS, sfgs_mesh_components. Vertices 0 ... m - 1, every face joins its three indices (degenerate faces too); labels int32
 *   [m]: the smallest vertex index of the vertex's component (a vertex in no face is its own); per root r (labels[r] == r):
 *   triangles[r] = the faces whose FIRST index lies in r's component, vertices_in[r] = its vertices; both int32 [m], zero elsewhere.
 *   State word 0 = the number of components. Lock-free union-find on a parent array in `scratch`, larger root hooked under
 *   the smaller; counts by integer atomics summed per wave and workgroup first. No float atomics.
 * CLEAN, sfgs_mesh_clean. keep_root: one byte per vertex, read at roots only. A face is kept when keep_root[labels[faces[t][0]]]
 *   is non-zero and (drop_degenerate == 0 or its three indices differ); a vertex is kept when a kept face references it. Both
 *   compactions preserve order, faces are renumbered through the vertex ranks, colours travel with vertices. Outputs hold m / n
 *   rows; state word 0 / 1 = the vertices / faces kept. Nothing is read back.
 * Refusals are SFGS_E_ARG, made before any GPU work: a NULL pointer, n outside 0 ... 2^29, m outside 0 ... 2^31 - 1, faces over
 * no vertex, colour pointers that do not come together, unknown flags, a scratch too small. No profiler ids of their own. */
size_t sfgs_mesh_weld_scratch_bytes(int64_t n);                        /* 0: bad arguments (sfgs_last_error) */
int sfgs_mesh_weld(const float* soup, const float* soup_colors, int64_t n, float* vertices, float* colors, int32_t* faces,
                   long long* state, int32_t flags, void* scratch, size_t scratch_bytes, void* stream);
int sfgs_mesh_vet(const int32_t* faces, int64_t n, int64_t m, long long* state, void* stream);
size_t sfgs_mesh_components_scratch_bytes(int64_t m);                  /* 0: bad arguments */
int sfgs_mesh_components(const int32_t* faces, int64_t n, int64_t m, int32_t* labels, int32_t* triangles, int32_t* vertices_in,
                         long long* state, void* scratch, size_t scratch_bytes, void* stream);
size_t sfgs_mesh_clean_scratch_bytes(int64_t m, int64_t n);            /* 0: bad arguments */
int sfgs_mesh_clean(const float* vertices, const float* colors, const int32_t* faces, int64_t m, int64_t n, const int32_t* labels,
                    const unsigned char* keep_root, int32_t drop_degenerate, float* vertices_out, float* colors_out,
                    int32_t* faces_out, long long* state, void* scratch, size_t scratch_bytes, void* stream);

/* ---- Mesh: decimation, vertex -> face adjacency, vertex normals (added under ABI 28: new symbols only; csrc/mesh.hip,
 * csrc/mesh_math.h; Python: Mesh.decimate / vertex_faces / vertex_normals). tests/mesh_simplify_np.py states the results in numpy
 * from these definitions and the kernels equal it byte for byte, run after run. `state` as above; two more meanings of its status:
 * bit 1 is also raised when the adjacency's segment sort reaches its trip bound, bit 4 (16) when the decimation met a BAD vertex.
 * All float64 arithmetic below is one rounded operation at a time (no fused multiply-add).
 * DECIMATE, sfgs_mesh_decimate: vertex clustering on the grid of `cell` (finite, > 0) at `origin` (finite). m vertices, n faces.
 *   1. Cell of vertex v, per axis a: u = (float64(V[v][a]) - origin[a]) / cell (a division), i = floor(u), f = u - i (0 <= f <= 1;
 *      1 only when a tiny negative u rounds), p = uint64(floor(f * 2^32)). v is BAD when some u is not finite or some i lies
 *      outside int32: it joins no cluster, every face that names it is dropped, status bit 4 is raised.
 *   2. Vertices with the same three int32 cell indices form a cluster; clusters are numbered in order of first appearance (by
 *      their smallest member). All m vertices take part, referenced by a face or not.
 *   3. Cluster vertex: c = the member count, S[a] = the sum of p in uint64 (<= 2^31 * 2^32);
 *      P[a] = float32((float64(i[a]) + float64(S[a] / c) * 2^-32) * cell + origin[a]), the division an integer division.
 *      Colours: x = the member's component, NaN -> 0, clamped to [0, 1] in float64, Sc = the sum of uint64(floor(x * 2^32)),
 *      colour = float32(float64(Sc / c) * 2^-32). A cluster with ONE member copies that member's position and colour bytes.
 *   4. Faces: G[t] = cluster_of[F[t]]. A face is dropped when an index is out of range (status bit 3) or names a bad vertex, when
 *      two of its new indices are equal, or -- flags bit 0, drop_duplicates -- when an earlier face that was not dropped for the
 *      reasons before has the same SET of three new indices: of such faces the smallest t stays, with its own winding.
 *   5. A cluster is kept when a kept face references it. Both compactions preserve order; faces are renumbered through the
 *      cluster ranks. Outputs hold m / n rows; state word 0 / 1 = the vertices / faces kept; vertex_map (or NULL): int32 [m], the
 *      output index of each input vertex's cluster, -1 when that cluster was dropped or the vertex was bad.
 *   flags bit 1: also sum the table slots the cluster insertions looked at into state word 3 (0 otherwise).
 *   Mechanism: the weld's table over the twelve-byte cell keys (the power of two >= 2 m slots), the row compaction's plan for the
 *   first-appearance ranks, relaxed agent-scope integer atomics for the count and the 64-bit sums, the same table again over the
 *   sorted triples of the faces (>= 2 n slots), the clean's compactions. Nothing depends on the order of arrival.
 * VERTEX_FACES, sfgs_mesh_vertex_faces: the inverted index. The flat corner record of face t, corner c is r = 3 t + c. offsets
 *   int32 [m + 1], records int32 [3 n]: records[offsets[v] ... offsets[v + 1]) holds every r with F[t][c] == v, ASCENDING
 *   (a stable argsort of the flattened faces, and the cumulative counts); a face that names v twice appears twice. A corner
 *   whose index is out of range is left out (status bit 3). State word 0 / 1 = m / n. Mechanism: integer-atomic counts, an
 *   exclusive scan, a fill through atomic cursors, then a thread per vertex sorts its own segment (insertion sort up to 32
 *   records, heapsort beyond, trip bound 2 k (log2 k + 2)).
 * VERTEX_NORMALS, sfgs_mesh_vertex_normals: normals float32 [m][3]. Face normal in float64 from the float32 positions a, b, c of
 *   F[t]: e1 = b - a, e2 = c - a, n_t = (e1y e2z - e1z e2y, e1z e2x - e1x e2z, e1x e2y - e1y e2x) (area-weighted, winding as
 *   stored). N_v = the sum of n_(r / 3) over v's records in ascending r, from +0.0, in float64; len = sqrt((Nx Nx + Ny Ny) + Nz Nz);
 *   the output is float32(N / len) per component when len > 0 and finite, else (0, 0, 0). One thread per vertex walks its
 *   segment: no atomics. offsets / records: a vertex_faces result of the same mesh. `state` is NOT reset: status bits are added.
 * Refusals are SFGS_E_ARG, made before any GPU work: a NULL pointer, sizes out of range, faces over no vertex, a cell that is not
 * finite and positive, an origin that is not finite, colour pointers that do not come together, unknown flags, a scratch too small. */
size_t sfgs_mesh_decimate_scratch_bytes(int64_t m, int64_t n, int32_t with_colors);      /* 0: bad arguments */
int sfgs_mesh_decimate(const float* vertices, const float* colors, const int32_t* faces, int64_t m, int64_t n, double cell,
                       double origin_x, double origin_y, double origin_z, int32_t flags, float* vertices_out, float* colors_out,
                       int32_t* faces_out, int32_t* vertex_map, long long* state, void* scratch, size_t scratch_bytes, void* stream);
size_t sfgs_mesh_vertex_faces_scratch_bytes(int64_t m);                /* 0: bad arguments */
int sfgs_mesh_vertex_faces(const int32_t* faces, int64_t n, int64_t m, int32_t* offsets, int32_t* records, long long* state,
                           void* scratch, size_t scratch_bytes, void* stream);
int sfgs_mesh_vertex_normals(const float* vertices, const int32_t* faces, int64_t m, int64_t n, const int32_t* offsets,
                             const int32_t* records, float* normals, long long* state, void* stream);

/* ---- Mesh rendering (added under ABI 28: new symbols only; csrc/mesh_raster.hip, csrc/mesh_raster_math.h; Python: Mesh.render):
 * the mesh seen from a camera -- depth along the forward axis, the index of the visible face, its normal and its colour per
 * pixel. tests/mesh_render_np.py states the result in numpy and the kernels equal it byte for byte, run after run: coverage is
 * decided in integers and a pixel's winner by an integer minimum, so neither the order of arrival nor the route of a face
 * (small_max) nor the launch shape changes a byte. Float64 arithmetic is one rounded operation at a time, in the order written.
 *   1. VERTEX. p = float64 of the float32 position; q = p - c; cam[a] = (q0 M[3a] + q1 M[3a+1]) + q2 M[3a+2]; z = cam[2];
 *      u = cam[0] focal_x / z + cx_pix, v = cam[1] focal_y / z + cy_pix (geo_project's sequence; M, c as in SfgsTsdfView; pixel
 *      centres sit at integer (col, row)). X = rint(256 u), Y = rint(256 v), ties to even. A vertex is UNUSABLE when u, v or z
 *      is not finite, when z <= near, or when |X| or |Y| exceeds 2^28. A face with an unusable vertex (or with an index outside
 *      0 ... m - 1, which also raises status bit 3) is not drawn and counts as CLIPPED. There is NO near-plane clipping: a face
 *      that crosses the plane z = near disappears as a whole.
 *   2. FACE (a, b, c). As = (Xb - Xa)(Yc - Ya) - (Yb - Ya)(Xc - Xa) in int64 (every product < 2^59). As == 0, two equal indices
 *      included: not drawn, DEGENERATE. With sigma = the sign of focal_x focal_y det(M) (det = (M0 (M4 M8 - M5 M7) - M1 (M3 M8 -
 *      M5 M6)) + M2 (M3 M7 - M4 M6)), the normal (b - a) x (c - a) points toward the camera exactly when sigma As < 0: in the
 *      camera's frame n . a = det[a b c], and the screen area has the sign of det[a b c] focal_x focal_y / (za zb zc). That is the
 *      outward, free side of sfgs_tsdf_extract's winding. cull == 1: a face turned away is not drawn, CULLED. Every other face is DRAWN
 *      (whether or not it covers a pixel). sgn = the sign of As, A = |As|.
 *   3. COVERAGE. The edge opposite corner i runs from corner j = i + 1 to k = i + 2 (mod 3): (dx, dy) = sgn (Xk - Xj, Yk - Yj),
 *      E_i(col, row) = dx (256 row - Yj) - dy (256 col - Xj), so that E_0 + E_1 + E_2 = A and the inside is positive. Pixel (col, row)
 *      is covered when every E_i > 0, or E_i == 0 and (dy < 0 or (dy == 0 and dx > 0)): a zero belongs to left and top edges. The
 *      rule reads the direction alone and answers the two directions of an edge differently, so a pixel centre on an edge shared by
 *      two faces belongs to exactly one of them, one on a shared vertex to at most one of the fan. Only pixels of the image inside
 *      the box ceil(min X / 256) ... floor(max X / 256) (and Y) are tested; no other can be covered.
 *   4. DEPTH. q_i = (double)E_i / z_i, s = (q0 + q1) + q2, depth = (float)((double)A / s). The pixel is kept when depth > 0 and
 *      (double)depth <= far.
 *   5. WINNER. The minimum over the kept faces of the key (float32 depth bits << 32) | face index: the nearest face, of equal
 *      depths the smaller index. A pixel nothing covers: depth 0, face -1, zeros in normal and rgb.
 *   6. ATTRIBUTES of the winner. b_i = q_i / s; an attribute is (b0 a0 + b1 a1) + b2 a2 in float64 on the corners' float32
 *      values. rgb = its float32. normal: with vertex_normals == NULL the face's flat normal -- N = (b - a) x (c - a) as in
 *      VERTEX_NORMALS above, winding as stored, not turned toward the camera; with vertex_normals (float32 [m][3]) N = the
 *      interpolated attribute, kept in float64; either way float32(N / len), len = sqrt((Nx Nx + Ny Ny) + Nz Nz), or (0, 0, 0)
 *      unless len is finite and > 0.
 *   depth float32 [H][W]; face int32 [H][W]; normal float32 [3][H][W] or NULL; rgb float32 [3][H][W], NULL exactly when colors is.
 *   state: EIGHT int64 words on the device, rewritten by every call: 0 ... 3 = the faces DRAWN, CULLED, CLIPPED, DEGENERATE (they
 *   sum to n), 4 = a status (bit 3: a face index out of range; bit 0: a list of larger faces was asked for more than its n entries
 *   -- a face is appended at most once, so this is never raised; it exists so that a broken invariant is reported, not a face
 *   dropped in silence), 5 ... 7 zero.
 *   small_max: a face whose clipped box holds at most this many pixels is rasterised by its own thread, a larger one by waves
 *   over 8 x 8 tiles; -1 = the library's default. The routes give the same bytes. Mechanism: four kernels (project, faces, large
 *   faces, resolve), relaxed agent-scope atomicMin on 64-bit keys in `scratch`, no float atomics; the two lists of larger faces
 *   (up to 64 tiles: a wave per face; beyond: 256 waves per face) hold n entries each and a face is appended at most once, so
 *   they cannot overflow; their lengths stay on the device.
 * Refusals are SFGS_E_ARG, made before any GPU work: a NULL pointer, a wrong struct_size, m or n out of range, faces over no
 * vertex, H or W < 1, H W > 2^30, a non-finite M, c or principal point, a focal length that is zero or not finite, near < 0 or not
 * finite, far <= near or NaN, an unknown cull, small_max outside -1 ... 2^30, rgb that does not go with colors, vertex_normals
 * without normal, a scratch too small. No profiler ids. */
typedef struct SfgsMeshRender {
  uint32_t struct_size;          /* = sizeof(SfgsMeshRender) */
  int32_t H, W;
  int32_t cull;                  /* 0: draw both sides; 1: do not draw faces turned away */
  double M[9];                   /* world = cam @ M + c */
  double c[3];
  double cx_pix, cy_pix, focal_x, focal_y, near, far;
  int64_t m, n, small_max;
  const float* vertices;         /* device, [m][3] */
  const float* colors;           /* device, [m][3], or NULL */
  const int32_t* faces;          /* device, [n][3] */
  const float* vertex_normals;   /* device, [m][3], or NULL: the flat normal */
  float* depth;                  /* device, [H][W] */
  int32_t* face;                 /* device, [H][W] */
  float* normal;                 /* device, [3][H][W], or NULL */
  float* rgb;                    /* device, [3][H][W]; NULL exactly when colors is */
  long long* state;              /* device, [8] */
} SfgsMeshRender;
size_t sfgs_mesh_render_scratch_bytes(int64_t m, int64_t n, int32_t H, int32_t W);      /* 0: bad arguments */
int sfgs_mesh_render(const SfgsMeshRender* args, void* scratch, size_t scratch_bytes, void* stream);

/* ---- Mesh queries (added under ABI 28: new symbols only; csrc/mesh_query.hip, csrc/mesh_query_math.h; Python: Mesh.face_grid,
 * Mesh.closest, Mesh.sample): a uniform grid over the faces, the closest face of a point, points on the surface. The reference
 * has no mesh step; tests/mesh_query_np.py states the results in numpy and the kernels equal it byte for byte. Float64 arithmetic
 * is one rounded operation at a time, in the order written.
 *   CELL. The cell of a coordinate x on an axis is floor((x - origin) / cell) in float64, for the vertices of a face and for a
 *     query point alike. The function is monotone in x.
 *   GRID, sfgs_mesh_grid_count then sfgs_mesh_grid_fill with the same struct and the same scratch. nx x ny x nz cells, cell
 *     (x, y, z) has the index (z ny + y) nx + x. A face is LEFT OUT when one of its indices lies outside 0 ... m - 1 or one of its
 *     nine coordinates is not finite. Every other face has, per axis, the range of cells from that of its smallest to that of its
 *     largest coordinate, both clamped into 0 ... dim - 1. A face whose range holds more than max_cells cells (-1: the default,
 *     4096) is LARGE: it goes to the large list (int32 [n], in no particular order; a face is appended at most once, so the list
 *     cannot overflow) and every query tests it. Every other face is registered in every cell of its range: cell_start int32
 *     [cells + 1] is the exclusive prefix sum of the cells' counts, pairs int32 [capacity] holds the face indices of cell c at
 *     cell_start[c] ... cell_start[c + 1], ASCENDING. max_cells bounds the fill loop of any thread; 0 puts every face on the
 *     large list, 2^30 none. state: FOUR int64 words, cleared by _count: 0 = the pairs in all (the capacity needed), 1 = the
 *     length of the large list, 2 = a status, 3 = the faces left out. Status bit 5 (32): capacity < word 0, pairs beyond it
 *     were not written and the table is not valid; bit 6 (64): more than 2^31 - 1 pairs; bit 3: a run outside the table; bit 1:
 *     the segment sort reached its trip bound; bit 0: the large list was asked for more than n entries (never).
 *     _count reads neither pairs nor capacity: a caller may read word 0 between the two calls and size pairs by it.
 *     Mechanism: integer-atomic counts, an exclusive scan (three launches), a fill through atomic cursors, the segment sort of
 *     VERTEX_FACES with a thread per cell.
 *   CLOSEST, sfgs_mesh_closest over a FILLED grid. points: float32 or float64 [k][3] (points_f64), taken to float64. For each point
 *     the answer is the minimum over all faces not left out of (d2, face index): d2 is the float64 squared distance to the
 *     closed triangle by ONE function (mq_closest in csrc/mesh_query_math.h): with ab = b - a, ac = c - a, bc = c - b, ap, bp, cp
 *     = p - a, p - b, p - c, dot(u, v) = (u0 v0 + u1 v1) + u2 v2, d1 ... d6 = dot(ab, ap), dot(ac, ap), dot(ab, bp), dot(ac, bp),
 *     dot(ab, cp), dot(ac, cp), vc = d1 d4 - d3 d2, vb = d5 d2 - d1 d6, va = d3 d6 - d5 d4, the first of these that holds decides:
 *       d1 <= 0 and d2 <= 0: a;  d3 >= 0 and d4 <= d3: b;  vc <= 0, d1 >= 0, d3 <= 0: a + (d1 / (d1 - d3)) ab;
 *       d6 >= 0 and d5 <= d6: c;  vb <= 0, d2 >= 0, d6 <= 0: a + (d2 / (d2 - d6)) ac;
 *       va <= 0, d4 - d3 >= 0, d5 - d6 >= 0: b + ((d4 - d3) / ((d4 - d3) + (d5 - d6))) bc;
 *       else with s = (va + vb) + vc: (a + (vb / s) ab) + (vc / s) ac;
 *     a quotient whose denominator is not > 0 is taken as 0; d2 = dot(p - q, p - q). A d2 that is not finite never wins, equal d2
 *     goes to the smaller face index. An answer with d2 > max_distance max_distance (max_distance >= 0, +inf: none), a point with a
 *     coordinate that is not finite and a point without any face get face -1, sqdist +inf and closest (0, 0, 0). sqdist float64
 *     [k], face int32 [k], closest float32 [k][3] or NULL (q rounded once). state: FOUR int64 words: 0 = the queries answered,
 *     1 = those without a face, 2 = a status (bit 3: a table entry out of range), 3 = the grid's faces left out.
 *     The grid does not change a byte of this. Search: the large list in full, then the Chebyshev rings of cells around the
 *     query's own cell (clamped to +-2^30, which only brings it nearer), from the first ring r0 that holds a cell of the grid,
 *     intersected with the grid. After ring r the search stops when best d2 < (r cell)^2 (1 - 2^-20), or when
 *     r cell (1 - 2^-20) > max_distance, at the latest after the ring of the grid's farthest cell, which is at most r0 + the
 *     largest dimension - 1. Exact because, from ring r0 on, a face registered in no visited cell has a coordinate whose cell
 *     differs from the query's by more than r on some axis (a range is clamped only toward cells that were visited), and CELL
 *     is monotone and shared: that coordinate is at least r cell (1 - 2^-40) away; the margin covers the rounding of the
 *     quotients and of d2. The rule does not hold below r0: a face outside the grid sits in a border cell, however near a
 *     query outside the grid it is.
 *     One thread per query, its result written by that thread alone; no float atomics, no atomics on the outputs.
 *   SAMPLE, sfgs_mesh_sample. Face t with positions a, b, c has the area A = 0.5 sqrt(dot(N, N)), N as in VERTEX_NORMALS, and
 *     e = A density. mix(seed, t, j) = f(f(f(seed ^ 0x9e3779b9) ^ t 0x7feb352d) ^ j 0x846ca68b) in uint32 arithmetic with f =
 *     murmur3's 32-bit finaliser; unit(h) = (h + 0.5) / 2^32. The face gets floor(e) + (unit(mix(seed, t, 2^32 - 1)) < e -
 *     floor(e)) samples. Sample j: u1, u2 = unit(mix(seed, t, 2 j)), unit(mix(seed, t, 2 j + 1)), both replaced by 1 - u when
 *     u1 + u2 > 1; a component of its position (and, with colours, of its colour) is float32((a + u1 (b - a)) + u2 (c - a)) in
 *     float64. Rows are ordered by face, then j. A face with an index out of range samples nothing (status bit 3); so does one
 *     whose e is not finite or whose count exceeds 2^20 (status bit 7, 128). points float32 [capacity][3], face int32
 *     [capacity], colors_out float32 [capacity][3] or NULL; a row at or beyond capacity is not written but still counted.
 *     state: FOUR int64 words: 0 = the samples found, 2 = the status (bit 6: more than 2^31 - 1 samples). capacity 0 only counts.
 * Refusals are SFGS_E_ARG, made before any GPU work: a NULL pointer, a wrong struct_size, m or n out of range, faces over no
 * vertex, a dimension < 1 or more than 2^28 cells, a cell that is not finite and positive, an origin that is not finite, max_cells
 * outside -1 ... 2^30, a capacity outside 0 ... 2^31 - 1, a negative or NaN max_distance or density, a scratch too small. No
 * profiler ids. */
typedef struct SfgsMeshGrid {
  uint32_t struct_size;          /* = sizeof(SfgsMeshGrid) */
  int32_t nx, ny, nz;
  double origin[3], cell;
  int64_t m, n, max_cells, capacity;
  const float* vertices;         /* device, [m][3] */
  const int32_t* faces;          /* device, [n][3] */
  int32_t* cell_start;           /* device, [nx ny nz + 1] */
  int32_t* pairs;                /* device, [capacity]; not read by _count */
  int32_t* large;                /* device, [n] */
  long long* state;              /* device, [4] */
} SfgsMeshGrid;
size_t sfgs_mesh_grid_scratch_bytes(int32_t nx, int32_t ny, int32_t nz);                 /* 0: bad arguments */
int sfgs_mesh_grid_count(const SfgsMeshGrid* grid, void* scratch, size_t scratch_bytes, void* stream);
int sfgs_mesh_grid_fill(const SfgsMeshGrid* grid, void* scratch, size_t scratch_bytes, void* stream);
int sfgs_mesh_closest(const SfgsMeshGrid* grid, const void* points, int32_t points_f64, int64_t k, double max_distance, double* sqdist,
                      int32_t* face, float* closest, long long* state, void* stream);
/* SUMMARY, sfgs_mesh_distance_summary, of a CLOSEST result: over the ANSWERED queries (face >= 0), with d = sqrt(sqdist) in float64.
 *   out: TWENTY int64 words, rewritten by every call: 0 ... 2 = the bits of three float64 -- the sum of d, the sum of sqdist, the
 *   largest d (0 without an answer); 3 = the queries answered; 4 + j = those with d <= thresholds[j] (j < num_thresholds <= 16,
 *   thresholds: HOST doubles >= 0), the rest zero. The counts are integers and exact. The sums are formed in a fixed order: the
 *   workgroup of queries 4096 b ... 4096 b + 4095 adds, per thread t, its items t, t + 256, ... in that order from +0.0, then
 *   the 256 threads' values in a binary tree (s = 128, 64, ..., 1: value[t] += value[t + s]); the workgroups' sums are added the
 *   same way, thread t taking workgroups t, t + 256, ...: the same bytes run after run. One launch; the last workgroup to
 *   finish (an integer ticket in `scratch`) adds the partials. No float atomics. */
size_t sfgs_mesh_distance_summary_scratch_bytes(int64_t k);            /* 0: bad arguments */
int sfgs_mesh_distance_summary(const double* sqdist, const int32_t* face, int64_t k, const double* thresholds, int32_t num_thresholds,
                               long long* out, void* scratch, size_t scratch_bytes, void* stream);
size_t sfgs_mesh_sample_scratch_bytes(int64_t n);                      /* 0: bad arguments */
int sfgs_mesh_sample(const float* vertices, const float* colors, const int32_t* faces, int64_t m, int64_t n, double density,
                     uint32_t seed, int64_t capacity, float* points, int32_t* face, float* colors_out, long long* state, void* scratch,
                     size_t scratch_bytes, void* stream);

/* ---- Per-Gaussian blend-weight statistics (ABI 28; csrc/importance.hip; Python: sfgs.importance): which Gaussians of a scene
 * show up in a set of views, and how much. For every (pixel, Gaussian) pair that the forward BLENDED -- accepted by the
 * per-pixel tests, before the pixel saturated -- with blend weight w = alpha T:
 *   weight_sum_q32[g] += floor(w 2^32)   (w <= 0.99; an integer sum: exact, the same bits in any order; sum w = q 2^-32)
 *   hits[g]           += 1
 *   weight_max[g]      = max(weight_max[g], w)
 * sfgs_raster_blend_stats runs on the blobs of a FINISHED sfgs_raster_forward_render of the same frame (same N, capacities,
 * tile-row band), on the same stream: it re-walks the per-tile lists with the forward's own per-pixel functions, in list
 * order, so every decision, T and w are those of the image, bit for bit. It ADDS into the caller's tables (zero them before
 * the first view). One launch, three integer atomics per (tile, Gaussian with a blended pixel); no float atomics: two runs
 * give the same bits.
 *   pixel_mask  device [H][W], one byte per pixel, or NULL: pairs of pixels whose byte is 0 are not counted (the pixel still
 *               composites: its transmittance is its own).
 * sfgs_blend_stats_views, once per view after it: if (hits[i] != hits_seen[i]) { ++views[i]; hits_seen[i] = hits[i]; } --
 * the number of views a Gaussian was blended in (hits_seen, views: caller-owned, zeroed with the tables).
 * Refusals are SFGS_E_ARG / SFGS_E_CAPACITY, made before any GPU work: a NULL pointer, a wrong struct_size, N < 0,
 * out->N != N, a bins blob smaller than the render stage's. N == 0 launches nothing. No profiler ids. */
typedef struct SfgsBlendStats {
  uint32_t struct_size;                 /* = sizeof(SfgsBlendStats) */
  int32_t N;                            /* rows of the three tables = the scene's Gaussians */
  unsigned long long* weight_sum_q32;   /* device [N]: sum of floor(w * 2^32) */
  unsigned long long* hits;             /* device [N]: blended (pixel, Gaussian) pairs */
  float* weight_max;                    /* device [N]: max w (>= 0) */
} SfgsBlendStats;
int sfgs_raster_blend_stats(const SfgsFrame* frame, int32_t N, const void* geom, const void* tiles, const void* bins,
                            size_t bins_bytes, int64_t dup_capacity, int64_t coarse_capacity, const unsigned char* pixel_mask,
                            const SfgsBlendStats* out, void* stream);
int sfgs_blend_stats_views(int32_t N, const unsigned long long* hits, unsigned long long* hits_seen, uint32_t* views,
                           void* stream);

/* Joint render with the Gaussians sharded over ranks (SURVEY 8e "all-gather the preprocessed 2D records"; the reference
 * has no multi-scene render). Every rank runs sfgs_raster_forward_plan on ITS Gaussians for the whole frame, then:
 *   sfgs_raster_plan_export  copies the plan's per-Gaussian compositing records rec_out[N][12 floats], the per-coarse-bin
 *                            item counts count_out[coarse_bins] and the items items_out[coarse_bins][export_capacity]
 *                            (16 bytes each) into caller-owned device buffers with FIXED strides, ready for an
 *                            all-gather (export_capacity >= the fullest coarse bin of any rank: all-reduce MAX of
 *                            SfgsRasterCounters.max_coarse_bin);
 *   sfgs_raster_plan_merge   builds ONE plan (geom / tiles / bins blobs sized by sfgs_raster_sizes for the total N, the
 *                            summed duplicate count and coarse_capacity >= parts x export_capacity) from the gathered
 *                            parts; Gaussian ids become positions in the concatenation (part order), so the per-tile
 *                            order -- ascending (depth bits, id) -- is the single-process one and
 *                            sfgs_raster_forward_render (num_duplicates = -1, any tile-row band) produces the same pixels
 *                            bit for bit. Forward only: a merged plan carries no duplicate indices for a backward.
 * Up to 16 parts. Asynchronous on `stream`. `bins` of sfgs_raster_plan_export is the blob the plan was given, in full
 * (sfgs_raster_sizes().bins_bytes: the bin-sorted items it reads lie at the blob's end; the call takes no size to check). */
int sfgs_raster_plan_export(const SfgsFrame* frame, int32_t N, const void* geom, const void* tiles, const void* bins,
                            int64_t dup_capacity, int64_t coarse_capacity, int64_t export_capacity, float* rec_out,
                            uint32_t* count_out, void* items_out, void* stream);
int sfgs_raster_plan_merge(const SfgsFrame* frame, int32_t parts, const int32_t* part_N, const float* const* part_rec,
                           const uint32_t* const* part_count, const void* const* part_items, int64_t export_capacity,
                           void* geom, size_t geom_bytes, void* tiles, size_t tiles_bytes, void* bins, size_t bins_bytes,
                           int64_t dup_capacity, int64_t coarse_capacity, void* stream);

/* simple_knn distCUDA2: out[i] = mean squared distance from point i to its 3 nearest other
 * points (index-excluded; fewer than 3 others: mean over those that exist). Exact for every input (brute force up to
 * 32 768 points; above, a Z-curve counting sort with box-pruned search -- the layout of the reference's simple-knn).
 * scratch: sfgs_knn_scratch_bytes(N) bytes, 256-byte aligned (0 / NULL for small N). Non-finite points get 0 and are
 * nobody's neighbour. */
size_t sfgs_knn_scratch_bytes(int32_t N);
int sfgs_knn_dist2(const float* xyz, int32_t N, float* out, void* scratch, size_t scratch_bytes,
                   void* stream);

/* Fused per-Gaussian pre-pass of render(): activations + Mip-Splatting 3D filter, i.e.
 *   scales    = sqrt(exp(scaling_raw)^2 + filter3d^2)        GaussianModel.get_scaling_with_3D_filter  scene/gaussian_model.py:207-213
 *   opacities = sigmoid(opacity_raw) * sqrt(prod s^2 / prod (s^2 + filter3d^2))  get_opacity_with_3D_filter  :237-249
 *   rotations = normalize(rotation_raw)                       get_rotation                               :216-217
 * filter3d is [N,1] float64 (training) or float32 (after load_ply); opacity_raw is float32 until the reference's first
 * reset_opacity (scene/gaussian_model.py:483-501), float64 afterwards (the reset divides by a float64 coefficient).
 * f64_mask: bit 0 = filter3d is float64, bit 1 = opacity_raw (and, in the backward, g_opacity_raw) is float64; torch's
 * type promotion is followed in every combination. Outputs float32.
 * backward: gradients w.r.t. the three raw tensors given gradients of the three outputs (each may be NULL = 0). */
int sfgs_prepass_forward(int32_t N, const float* scaling_raw, const void* opacity_raw,
                         const float* rotation_raw, const void* filter3d, int32_t f64_mask,
                         float* scales, float* opacities, float* rotations, void* stream);
int sfgs_prepass_backward(int32_t N, const float* scaling_raw, const void* opacity_raw,
                          const float* rotation_raw, const void* filter3d, int32_t f64_mask,
                          const float* g_scales, const float* g_opacities, const float* g_rotations,
                          float* g_scaling_raw, void* g_opacity_raw, float* g_rotation_raw, void* stream);

/* GaussianModel.compute_3D_filter (scene/gaussian_model.py:255-308): filter_out[N] (float64) =
 * (smallest camera-space depth at which any camera sees the point with a 15 % screen margin) / max_focal *
 * sqrt(0.2); points no camera sees get the largest seen depth. cams: device [C][18] float64 =
 * R[9] (row-major, used as xyz @ R like the reference), T[3], focal_x, focal_y, cx_ori, cy_ori, width, height. */
size_t sfgs_filter3d_scratch_bytes(int32_t N);
int sfgs_filter3d(const float* xyz, int32_t N, const double* cams, int32_t C, double max_focal,
                  double* filter_out, void* scratch, size_t scratch_bytes, void* stream);

/* GaussianModel.add_densification_stats (scene/gaussian_model.py:744-749), in place, no host
 * sync: for every i with update_filter[i] != 0 (bool/uint8 [N]):
 *   accum[i] += hypot(grad[i,0], grad[i,1]); accum_abs[i] += |grad[i,2]|; accum_abs_max[i] = max(., |grad[i,2]|);
 *   denom[i] += 1.   viewspace_grad is means2D.grad [N,3]; accum_abs_max may be NULL. */
int sfgs_densify_stats(int32_t N, const float* viewspace_grad, const unsigned char* update_filter,
                       float* xyz_gradient_accum, float* xyz_gradient_accum_abs,
                       float* xyz_gradient_accum_abs_max_or_null, float* denom, void* stream);

/* One Adam step over a list of float32 tensors in one launch. Replaces the per-iteration
 * `gaussians.optimizer.step()` (train.py:339,906) of `torch.optim.Adam(l, lr=0.0, eps=1e-15)`
 * (scene/gaussian_model.py:382); arithmetic = torch's default ("foreach") CUDA path, operation by operation:
 *   g' = grad + weight_decay*param (if weight_decay != 0);  m += (1-b1)*(g'-m);  v = v*b2 + (1-b2)*g'*g';
 *   param += neg_step_size * (m / (sqrt(v)/bias_correction2_sqrt + eps))
 * The host computes, in double like torch does, neg_step_size = -lr/(1-b1^t) and bias_correction2_sqrt =
 * sqrt(1-b2^t) for the tensor's own step count t (already incremented). `tensors` is a HOST array; all pointers are
 * device pointers to contiguous float32 (or, with SFGS_ADAM_F64, float64) storage of `count` elements, updated in place. */
#define SFGS_ADAM_F64 1u   /* flags: param, grad and both moments are float64 (the reference's `_opacity` group after
                              reset_opacity, scene/gaussian_model.py:483-501); the update then runs in float64 like torch's */
typedef struct SfgsAdamTensor {
  void* param;
  const void* grad;
  void* exp_avg;
  void* exp_avg_sq;
  int64_t count;
  double neg_step_size;           /* the scalars as torch forms them (Python floats = double); the float32 path */
  double one_minus_beta1;         /* rounds them to float, the float64 path uses them as they are             */
  double beta2;
  double one_minus_beta2;
  double bias_correction2_sqrt;
  double eps;
  double weight_decay;
  uint32_t flags;                 /* SFGS_ADAM_* */
  uint32_t reserved;
} SfgsAdamTensor;
int sfgs_adam_step(const SfgsAdamTensor* tensors, int32_t count, void* stream);

/* utils/sh_utils.py:57-112 eval_sh: out[n,c] = sum_{k < (deg+1)^2} basis_k(dirs[n]) * sh[n,c,k], the reference's
 * channel-major layout sh[N,3,K] with K >= (deg+1)^2 stored coefficients (used by render() at
 * gaussian_renderer/__init__.py:115,124). No normalisation of dirs, no +0.5, no clamp -- like the reference function.
 * backward: g_sh[N,3,K] fully written (zeros beyond the active degree), g_dirs[N,3] optional. */
int sfgs_sh_eval_forward(int32_t N, int32_t deg, int32_t K, const float* sh, const float* dirs, float* out,
                         void* stream);
int sfgs_sh_eval_backward(int32_t N, int32_t deg, int32_t K, const float* sh, const float* dirs, const float* g_out,
                          float* g_sh, float* g_dirs_or_null, void* stream);

/* Row compaction of many tensors by ONE keep-mask (replaces the 26 `tensor[mask]` operations of
 * GaussianModel.prune_points/_prune_optimizer, scene/gaussian_model.py:563-603). keep[N]: bool/uint8, nonzero = the
 * row survives. sfgs_compact_plan scans the mask into caller-owned scratch and, if kept_out != NULL, synchronises the
 * stream once to report the number of surviving rows (the caller allocates dst tensors of that many rows).
 * sfgs_compact_rows then copies row i of every src to row rank(i) of its dst in one launch; src/dst are device
 * pointers to contiguous [N, row_bytes] / [kept, row_bytes] storage, `tensors` is a HOST array. */
typedef struct SfgsCompactTensor {
  const void* src;
  void* dst;
  int64_t row_bytes;
} SfgsCompactTensor;
size_t sfgs_compact_scratch_bytes(int64_t N);
int sfgs_compact_plan(const unsigned char* keep, int64_t N, void* scratch, size_t scratch_bytes, int64_t* kept_out,
                      void* stream);
int sfgs_compact_rows(const unsigned char* keep, int64_t N, const void* scratch, const SfgsCompactTensor* tensors,
                      int32_t count, void* stream);

/* GaussianModel.densify_and_prune (scene/gaussian_model.py:603-742) as a handful of launches.
 *
 * sfgs_select_kth: exact order statistics of N non-negative floats by radix select, for ANY N (torch.quantile refuses
 * more than 16 M elements and the reference then falls back to Q = 0.99, :716-723). rank_dev: DEVICE float r (as
 * torch.quantile forms it: q * (N - 1)); out2[0] = value at rank floor(r), out2[1] = value at rank ceil(r) (device);
 * the caller interpolates like torch (lerp). Asynchronous.
 *
 * sfgs_densify_decide: per Gaussian, from grad_norm[N] = |xyz_gradient_accum / denom|, grad_abs[N] (the abs column),
 * the ACTIVATED scaling[N,3] / opacity[N] (float32, or float64 after the reference's reset_opacity) and the thresholds:
 * clone = selected and max(scaling) <= dense_threshold, split = selected and max(scaling) > dense_threshold with
 * selected = grad_norm >= max_grad or grad_abs >= Q (Q read from Q_dev when non-NULL, else Q_host), and which rows
 * survive the final prune (opacity < min_opacity, or -- when use_big_threshold -- max(scaling) > big_threshold; the
 * screen-size term never fires in the reference because densification_postfix resets max_radii2D first). Fills
 * `scratch` (sfgs_densify_scratch_bytes) and returns, with ONE host synchronisation, totals_out[5] = rows kept of
 * {originals, clones, children per child index} and the raw {clone, split} counts.
 * sfgs_densify_gather: writes every dst tensor [totals[0] + totals[1] + 2 * totals[2] rows] in the reference's final
 * order [surviving originals | clones | first children | second children]; zero_new_rows: clones / children get zeros
 * (Adam moments). sfgs_densify_children then overwrites the child rows of xyz (parent + R(q) * sample) and of the raw
 * scaling (log(scaling / 1.6)); samples[2 * totals[4], 3] = std * z in the layout of the reference's `samples` (:666),
 * or -- unit_samples != 0 -- just z ~ N(0, 1), which the kernel multiplies by the parent's scaling itself (no mask
 * gather on the host side).
 * sfgs_densify_masks: the decisions as byte masks (tests / diagnostics). */
typedef struct SfgsDensifyTensor {
  const void* src;
  void* dst;
  int64_t row_bytes;       /* multiple of 4 */
  int32_t zero_new_rows;
  int32_t reserved;
} SfgsDensifyTensor;
size_t sfgs_select_scratch_bytes(void);
int sfgs_select_kth(const float* values, int64_t N, const float* rank_dev, float* out2, void* scratch,
                    size_t scratch_bytes, void* stream);
size_t sfgs_densify_scratch_bytes(int64_t N);
int sfgs_densify_decide(int64_t N, const float* grad_norm, const float* grad_abs, const float* scaling,
                        const void* opacity, int32_t opacity_is_f64, const float* Q_dev, float Q_host, float max_grad,
                        double min_opacity, float dense_threshold, float big_threshold, int32_t use_big_threshold,
                        void* scratch, size_t scratch_bytes, int64_t totals_out[5], void* stream);
int sfgs_densify_masks(int64_t N, const void* scratch, unsigned char* clone_out, unsigned char* split_out,
                       unsigned char* keep_out, void* stream);
int sfgs_densify_gather(int64_t N, const void* scratch, const int64_t totals[5], const SfgsDensifyTensor* tensors,
                        int32_t count, void* stream);
int sfgs_densify_children(int64_t N, const void* scratch, const int64_t totals[5], const float* xyz,
                          const float* rotation_raw, const float* scaling, const float* samples, int32_t unit_samples,
                          float* xyz_out, float* scaling_raw_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SFGS_H */
