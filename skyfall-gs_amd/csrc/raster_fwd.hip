// raster_fwd.hip -- the forward of the Gaussian-splat rasterizer for gfx950 (MI355X): its C ABI (include/sfgs.h).
//
// Replaces diff_gauss.GaussianRasterizer.__call__ (reference: gaussian_renderer/__init__.py:132-140). The entry points
// here validate, build the views of the caller's blobs (sfgs_internal.h) and call the stages, each a translation unit of
// its own that launches the kernels it defines (all wave64, no MFMA: the path is gather/sort/VALU bound):
//
//   plan    raster_preprocess.hip  subpix_bound -> preprocess (per Gaussian: project, radii, 48-B record, coarse items)
//                                  -> big_walk (the screen-filling splats)
//           raster_binning.hip     bin_count -> bin_rank -> bin_scatter (two-pass binning: the items sorted by coarse bin;
//                                  the plan's scans ride in the last launch) or plan_scan (one-pass binning); the joint
//                                  render's plan export / merge
//   render  raster_sort.hip        select_sort (short lists: select + sort in one kernel) or fine_bin -> sort_tiles_reg;
//                                  then sort_tiles_reg_long (513 .. 1 024 entries) and sort_tiles_long (bucketed sort,
//                                  LDS network, LDS/global hybrid beyond)
//           composite_fwd.hip      tile_order (on a hint) -> composite_fwd (one wave per 8x8 tile, front to back)
//
// The five files are compiled with the same flags (csrc/Makefile); the backward is raster_bwd.hip + composite_bwd.hip.
#include <algorithm>

#include "sfgs_internal.h"

namespace sfgs {

int check_frame(const SfgsFrame* f) {
  SFGS_REQUIRE(f != nullptr, SFGS_E_ARG, "frame is NULL");
  SFGS_REQUIRE(f->struct_size == sizeof(SfgsFrame), SFGS_E_ARG, "SfgsFrame.struct_size %u != %zu (ABI mismatch)",
               f->struct_size, sizeof(SfgsFrame));
  SFGS_REQUIRE(f->image_width > 0 && f->image_height > 0, SFGS_E_ARG, "image size %dx%d", f->image_width,
               f->image_height);
  SFGS_REQUIRE(f->bg && f->viewmatrix && f->projmatrix && f->campos, SFGS_E_ARG, "frame tensor pointer is NULL");
  SFGS_REQUIRE(f->sh_degree >= 0 && f->sh_degree <= 4, SFGS_E_UNSUPPORTED, "sh_degree %d not in 0..4", f->sh_degree);
  SFGS_REQUIRE(f->tanfovx > 0.f && f->tanfovy > 0.f, SFGS_E_ARG, "tanfov must be positive");
  SFGS_REQUIRE((int64_t)f->image_width * f->image_height < (1ll << 31), SFGS_E_UNSUPPORTED, "image too large");
  return SFGS_OK;
}

}  // namespace sfgs

// =================================================================================================
// C ABI
// =================================================================================================
using namespace sfgs;

static bool binning_direct() { return option(OPT_BINNING) != 0; }

static int check_gaussians(const SfgsFrame* f, const SfgsGaussians* g) {
  SFGS_REQUIRE(g != nullptr, SFGS_E_ARG, "gaussians is NULL");
  SFGS_REQUIRE(g->struct_size == sizeof(SfgsGaussians), SFGS_E_ARG, "SfgsGaussians.struct_size mismatch");
  SFGS_REQUIRE(g->count >= 0, SFGS_E_ARG, "negative Gaussian count");
  if (g->count > 0) {
    SFGS_REQUIRE(g->means3D && g->scales && g->rotations && g->opacities, SFGS_E_ARG, "Gaussian tensor pointer is NULL");
    SFGS_REQUIRE((g->colors_precomp != nullptr) != (g->shs != nullptr), SFGS_E_ARG,
                 "provide exactly one of colors_precomp / shs");
    SFGS_REQUIRE(g->filter_3D ? (g->raw_f64_mask & ~3) == 0 : g->raw_f64_mask == 0, SFGS_E_ARG,
                 "raw_f64_mask %d: bit 0 = filter_3D is float64, bit 1 = raw opacities are float64; 0 without filter_3D",
                 g->raw_f64_mask);
    SFGS_REQUIRE(!(g->sh_dirs || g->sh_centers) || g->shs, SFGS_E_ARG, "sh_dirs / sh_centers (eval_sh-folded colour path) need shs");
    SFGS_REQUIRE(!(g->sh_dirs && g->sh_centers), SFGS_E_ARG, "sh_dirs and sh_centers are alternatives");
    SFGS_REQUIRE((g->sh_dirs || g->sh_centers) ? (g->shs_channel_major & ~1) == 0 : g->shs_channel_major == 0, SFGS_E_ARG,
                 "shs_channel_major %d: 0 or 1, and 0 without sh_dirs / sh_centers", g->shs_channel_major);
    SFGS_REQUIRE(!g->shs_rest || (g->shs && f->sh_coeffs > 1 && g->shs_channel_major == 0), SFGS_E_ARG,
                 "shs_rest (split SH storage) needs shs, sh_coeffs > 1 and coefficient-major storage");
    if (g->shs)
      SFGS_REQUIRE(f->sh_coeffs >= (f->sh_degree + 1) * (f->sh_degree + 1) &&
                       (f->sh_coeffs == 1 || f->sh_coeffs == 4 || f->sh_coeffs == 9 || f->sh_coeffs == 16 || f->sh_coeffs == 25),
                   SFGS_E_ARG, "sh_coeffs %d: must be 1, 4, 9, 16 or 25 and hold degree %d", f->sh_coeffs, f->sh_degree);
  }
  return SFGS_OK;
}

// The plan clears the head of the tiles blob (header, duplicate pools, the coarse bins' counter lines: 261 KB at 1080p).
// A kernel of our own instead of hipMemsetAsync (profiles/r4_plan_memset_ab.txt): the runtime's fill goes through its blit path,
// which showed up in the kernel traces with 4 - 6 us of idle queue in front of it on every frame.
__global__ void __launch_bounds__(256) zero_head_kernel(uint4* __restrict__ p, unsigned n16) {
  const unsigned i = blockIdx.x * 256u + threadIdx.x;
  if (i < n16) p[i] = make_uint4(0u, 0u, 0u, 0u);
}
hipError_t sfgs::zero_head(void* p, size_t bytes, hipStream_t stream) {
  const unsigned n16 = (unsigned)(bytes / 16);   // zero_bytes is a multiple of 256
  hipLaunchKernelGGL(zero_head_kernel, dim3((n16 + 255) / 256), dim3(256), 0, stream, (uint4*)p, n16);
  return hipGetLastError();
}

extern "C" int sfgs_raster_sizes(int32_t N, int32_t W, int32_t H, int64_t D, int64_t coarse_capacity,
                                 SfgsRasterSizes* out) {
  SFGS_REQUIRE(out && out->struct_size == sizeof(SfgsRasterSizes), SFGS_E_ARG, "SfgsRasterSizes.struct_size mismatch");
  SFGS_REQUIRE(N >= 0 && W > 0 && H > 0 && D >= 0 && coarse_capacity >= 0, SFGS_E_ARG,
               "bad sizes N=%d W=%d H=%d D=%lld coarse_capacity=%lld", N, W, H, (long long)D, (long long)coarse_capacity);
  SFGS_REQUIRE(D < (1ll << 32) && coarse_capacity < (1ll << 31), SFGS_E_UNSUPPORTED, "more than 2^32 duplicates");
  size_t tb = 0;
  tiles_view(nullptr, W, H, N, &tb);
  out->geom_bytes = geom_bytes(N);
  out->tiles_bytes = tb;
  out->bins_bytes = bins_bytes_plan(D, coarse_bins(W, H), coarse_capacity, N);
  out->image_bytes = image_bytes(W, H, D);
  out->dupgrad_bytes = dupgrad_bytes(D);   // D = the duplicate capacity the frame was planned with (sparse index space)
  out->coarse_bins = coarse_bins(W, H);
  return SFGS_OK;
}

extern "C" int64_t sfgs_raster_slot_capacity(int32_t W, int32_t H, int64_t num_duplicates) {
  if (W <= 0 || H <= 0 || num_duplicates < 0) return -1;
  // every coarse bin's lists take at most its tile hits + 16 x 63 alignment slots, rounded up to 64 (bin_slots_needed)
  return num_duplicates + (int64_t)(COARSE_TILES * (LIST_ALIGN - 1) + 2 * LIST_ALIGN - 1) / LIST_ALIGN * LIST_ALIGN * coarse_bins(W, H);
}

extern "C" int sfgs_raster_forward_plan(const SfgsFrame* frame, const SfgsGaussians* g, int32_t* radii, void* geom,
                                        size_t geom_sz, void* tiles, size_t tiles_sz, void* bins, size_t bins_sz,
                                        int64_t dup_capacity, int64_t coarse_capacity, void* counters_pinned_host,
                                        void* stream_) {
  if (int rc = check_frame(frame)) return rc;
  if (int rc = check_gaussians(frame, g)) return rc;
  hipStream_t stream = (hipStream_t)stream_;
  const int N = g->count, W = frame->image_width, H = frame->image_height;
  size_t tb = 0;
  SFGS_REQUIRE(tiles != nullptr, SFGS_E_ARG, "tiles blob is NULL");
  const TilesView tv = tiles_view(tiles, W, H, N, &tb);
  const int64_t NCB = coarse_bins(W, H);
  SFGS_REQUIRE(tiles_sz >= tb, SFGS_E_CAPACITY, "tiles blob: %zu bytes given, %zu needed", tiles_sz, tb);
  SFGS_REQUIRE(geom_sz >= geom_bytes(N), SFGS_E_CAPACITY, "geom blob: %zu bytes given, %zu needed", geom_sz, geom_bytes(N));
  SFGS_REQUIRE(N == 0 || (radii && geom), SFGS_E_ARG, "radii / geom is NULL");
  SFGS_REQUIRE(dup_capacity >= 0 && dup_capacity < (1ll << 32) && coarse_capacity >= 0 && coarse_capacity < (1ll << 31),
               SFGS_E_ARG, "bad dup_capacity / coarse_capacity");
  SFGS_REQUIRE(bins_sz >= bins_bytes_plan(dup_capacity, NCB, coarse_capacity, N), SFGS_E_CAPACITY,
               "bins blob: %zu bytes given, %zu needed (sfgs_raster_sizes; the plan keeps its pair list there)", bins_sz,
               bins_bytes_plan(dup_capacity, NCB, coarse_capacity, N));
  SFGS_REQUIRE(bins, SFGS_E_ARG, "bins blob is NULL");
  const GeomView gv = geom_view(geom, N);
  const BinsView bv = bins_view_csr(bins, dup_capacity, NCB, coarse_capacity, N);
  const KFrame kf = make_kframe(frame);
  SFGS_CHECK_HIP(zero_head(tiles, tv.zero_bytes, stream));
  // two-pass binning (pair list + bin_scatter_kernel) unless the coarse-bin index does not fit the pair's 16 bits (images
  // beyond 65 536 coarse bins = 8 192 x 8 192 pixels) or SFGS_BINNING=direct asks for the one-pass path (A/B, tests)
  const bool two_pass = NCB <= 65536 && !binning_direct();
  if (int rc = plan_preprocess(frame, g, radii, kf, gv, tv, bv, dup_capacity, coarse_capacity, two_pass, stream)) return rc;
  return plan_binning(frame, N, gv, tv, bv, coarse_capacity, two_pass, counters_pinned_host, stream);
}

static void unpack_counters(const unsigned long long* h, SfgsRasterCounters* out) {
  out->num_duplicates = (int64_t)h[HDR_D_EFF];
  out->num_duplicates_ref = (int64_t)h[HDR_D_REF];
  out->num_visible = (int64_t)h[HDR_N_VIS];
  out->max_tile_list = (int64_t)h[HDR_MAX_LIST];
  out->overflow = (int64_t)h[HDR_OVERFLOW];
  out->max_coarse_bin = (int64_t)h[HDR_MAX_COARSE];
  out->max_bin_items = (int64_t)h[HDR_MAX_BIN_ITEMS];
  out->sort_wide_tiles = (int64_t)h[HDR_SORT_WIDE];
  out->num_huge_splats = (int64_t)h[HDR_BIG_COUNT];
  out->num_big_chunks = (int64_t)h[HDR_BIG_CHUNKS];
  out->prev_valid = out->prev_long_tiles = out->prev_max_tile_list = out->prev_prefilled = out->prev_tiles_over_512 = 0;
}

extern "C" int sfgs_raster_counters_decode(const void* host_128, SfgsRasterCounters* out) {
  SFGS_REQUIRE(host_128 && out, SFGS_E_ARG, "NULL argument");
  // words 0..7 = the first header words; 8..13 as plan_scan_kernel lays them out
  const unsigned long long* h = (const unsigned long long*)host_128;
  unsigned long long hdr[HDR_WORDS] = {0};
  for (int i = 0; i < 8; ++i) hdr[i] = h[i];
  hdr[HDR_BIG_COUNT] = h[8];
  hdr[HDR_BIG_CHUNKS] = h[9];
  unpack_counters(hdr, out);
  out->prev_valid = (int64_t)h[10];
  out->prev_long_tiles = (int64_t)h[11];
  out->prev_max_tile_list = (int64_t)h[12];
  out->prev_prefilled = (int64_t)h[13];
  out->prev_tiles_over_512 = (int64_t)h[14];
  out->max_bin_items = (int64_t)h[15];
  return SFGS_OK;
}

extern "C" int sfgs_raster_read_counters(const void* tiles, SfgsRasterCounters* out, void* stream_) {
  SFGS_REQUIRE(tiles && out, SFGS_E_ARG, "NULL argument");
  hipStream_t stream = (hipStream_t)stream_;
  unsigned long long h[HDR_WORDS] = {0};
  SFGS_CHECK_HIP(hipMemcpyAsync(h, tiles, 16 * sizeof(unsigned long long), hipMemcpyDeviceToHost, stream));
  SFGS_CHECK_HIP(hipStreamSynchronize(stream));
  unpack_counters(h, out);
  return SFGS_OK;
}

extern "C" int sfgs_raster_read_counters_pinned(const void* tiles, void* pinned_host_64, SfgsRasterCounters* out,
                                                void* stream_) {
  SFGS_REQUIRE(tiles && out && pinned_host_64, SFGS_E_ARG, "NULL argument");
  hipStream_t stream = (hipStream_t)stream_;
  SFGS_CHECK_HIP(hipMemcpyAsync(pinned_host_64, tiles, 64, hipMemcpyDeviceToHost, stream));
  SFGS_CHECK_HIP(hipStreamSynchronize(stream));
  unsigned long long hdr[HDR_WORDS] = {0};   // the first 8 header words; the optional-work counts read 0 (use
  for (int i = 0; i < 8; ++i) hdr[i] = ((const unsigned long long*)pinned_host_64)[i];   // sfgs_raster_read_counters)
  unpack_counters(hdr, out);
  return SFGS_OK;
}

extern "C" int sfgs_raster_forward_render(const SfgsFrame* frame, int32_t N, const void* geom, void* tiles,
                                          void* bins, size_t bins_sz, int64_t dup_capacity, int64_t coarse_capacity,
                                          int64_t num_duplicates, float* out_color, float* out_depth, float* out_alpha,
                                          void* image, size_t image_sz, void* stream_) {
  if (int rc = check_frame(frame)) return rc;
  hipStream_t stream = (hipStream_t)stream_;
  const int W = frame->image_width, H = frame->image_height;
  const int64_t NCB = coarse_bins(W, H);
  SFGS_REQUIRE(N >= 0 && tiles && out_color && out_depth && out_alpha && bins, SFGS_E_ARG, "NULL argument");
  SFGS_REQUIRE(dup_capacity >= 0 && dup_capacity < (1ll << 32) && coarse_capacity >= 0, SFGS_E_ARG, "bad capacity");
  SFGS_REQUIRE(num_duplicates < 0 || sfgs_raster_slot_capacity(W, H, num_duplicates) <= dup_capacity, SFGS_E_CAPACITY,
               "%lld duplicates need %lld list slots, dup_capacity is %lld: redo the plan with larger blobs",
               (long long)num_duplicates, (long long)sfgs_raster_slot_capacity(W, H, num_duplicates),
               (long long)dup_capacity);
  SFGS_REQUIRE(bins_sz >= bins_bytes(dup_capacity, NCB, coarse_capacity), SFGS_E_CAPACITY,
               "bins blob: %zu bytes given, %zu needed", bins_sz, bins_bytes(dup_capacity, NCB, coarse_capacity));
  SFGS_REQUIRE(image == nullptr || image_sz >= image_bytes(W, H, dup_capacity), SFGS_E_CAPACITY, "image blob too small");
  const TilesView tv = tiles_view(tiles, W, H, N, nullptr);
  const GeomView gv = geom_view(const_cast<void*>(geom), N);
  const BinsView bv = bins_view_csr(bins, dup_capacity, NCB, coarse_capacity, N);
  const KFrame kf = make_kframe(frame);
  if (int rc = sort_tile_lists(frame, tv, bv, dup_capacity, coarse_capacity, num_duplicates, stream)) return rc;
  const ImageView iv = image ? image_view(image, W, H, dup_capacity) : ImageView{};
  return composite_forward(frame, kf, gv, tv, bv, image ? &iv : nullptr, out_color, out_depth, out_alpha, stream);
}

// ---- one scratch allocation, one call per stage (ABI 11) --------------------------------------------------------------
namespace sfgs {
int scratch_layout(int32_t N, int32_t W, int32_t H, int64_t D, int64_t ccap, bool with_image, SfgsScratchLayout* out) {
  SFGS_REQUIRE(N >= 0 && W > 0 && H > 0 && D >= 0 && ccap >= 0, SFGS_E_ARG, "bad sizes N=%d W=%d H=%d D=%lld coarse_capacity=%lld",
               N, W, H, (long long)D, (long long)ccap);
  SFGS_REQUIRE(D < (1ll << 32) && ccap < (1ll << 31), SFGS_E_UNSUPPORTED, "more than 2^32 duplicates");
  size_t tb = 0;
  tiles_view(nullptr, W, H, N, &tb);
  const size_t a = 256;
  out->geom_offset = 0;
  out->tiles_offset = align_up(std::max<size_t>(geom_bytes(N), 1), a);
  out->bins_offset = out->tiles_offset + align_up(tb, a);
  out->image_offset = out->bins_offset + align_up(std::max<size_t>(bins_bytes_plan(D, coarse_bins(W, H), ccap, N), 1), a);
  out->total_bytes = out->image_offset + (with_image ? align_up(image_bytes(W, H, D), a) : 0);
  out->dupgrad_bytes = dupgrad_bytes(D);
  out->coarse_bins = coarse_bins(W, H);
  out->slot_overhead = sfgs_raster_slot_capacity(W, H, 0);
  return SFGS_OK;
}
}  // namespace sfgs

extern "C" int sfgs_raster_scratch_layout(int32_t N, int32_t W, int32_t H, int64_t dup_capacity, int64_t coarse_capacity,
                                          int32_t with_image, SfgsScratchLayout* out) {
  SFGS_REQUIRE(out && out->struct_size == sizeof(SfgsScratchLayout), SFGS_E_ARG, "SfgsScratchLayout.struct_size mismatch");
  return scratch_layout(N, W, H, dup_capacity, coarse_capacity, with_image != 0, out);
}

extern "C" int sfgs_raster_forward(const SfgsFrame* frame, const SfgsGaussians* g, int32_t* radii, void* scratch,
                                   size_t scratch_bytes, int64_t dup_capacity, int64_t coarse_capacity, int32_t with_image,
                                   void* counters_pinned_host, void* plan_done_event, float* out_color, float* out_depth,
                                   float* out_alpha, void* stream_) {
  if (int rc = check_frame(frame)) return rc;
  SFGS_REQUIRE(g != nullptr && scratch != nullptr, SFGS_E_ARG, "NULL argument");
  SfgsScratchLayout lay;
  if (int rc = scratch_layout(g->count, frame->image_width, frame->image_height, dup_capacity, coarse_capacity,
                              with_image != 0, &lay)) return rc;
  SFGS_REQUIRE(scratch_bytes >= lay.total_bytes, SFGS_E_CAPACITY, "scratch: %zu bytes given, %zu needed", scratch_bytes,
               lay.total_bytes);
  SFGS_REQUIRE(((uintptr_t)scratch & 255u) == 0, SFGS_E_ARG, "scratch must be 256-byte aligned");
  char* base = (char*)scratch;
  const size_t geom_sz = lay.tiles_offset, tiles_sz = lay.bins_offset - lay.tiles_offset,
               bins_sz = lay.image_offset - lay.bins_offset, image_sz = lay.total_bytes - lay.image_offset;
  if (int rc = sfgs_raster_forward_plan(frame, g, radii, base + lay.geom_offset, geom_sz, base + lay.tiles_offset, tiles_sz,
                                        base + lay.bins_offset, bins_sz, dup_capacity, coarse_capacity,
                                        counters_pinned_host, stream_)) return rc;
  if (plan_done_event) SFGS_CHECK_HIP(hipEventRecord((hipEvent_t)plan_done_event, (hipStream_t)stream_));
  return sfgs_raster_forward_render(frame, g->count, base + lay.geom_offset, base + lay.tiles_offset, base + lay.bins_offset,
                                    bins_sz, dup_capacity, coarse_capacity, -1, out_color, out_depth, out_alpha,
                                    with_image ? base + lay.image_offset : nullptr, image_sz, stream_);
}
