// gsr_hip.hip — MI355X (gfx950 / CDNA4) differentiable 3D-Gaussian rasterizer, C ABI in include/gsr.h.
//
// Replaces, behind the same operator surface, the external CUDA extension the reference calls at
// src/model/decoder/cuda_splatting.py:113-124 (forward) and through autograd (backward).  The
// arithmetic it must reproduce is restated in oracle/gsr_oracle.hpp; this
// library is not a translation of the CUDA package's structure:
//
//   * one launch chain renders V views (grid.y / per-view tile ranges) instead of one chain per view;
//   * tiles are 8x8 pixels = ONE 64-lane wavefront per tile: no block barriers in the blend loops,
//     wave-uniform early-out, per-splat gradients reduced across the wavefront before a single
//     atomic per value.  Membership keeps the reference's rule (a splat reaches a pixel iff the
//     pixel's 16x16 parent tile is inside the ceil(3 sigma) rect) and then drops (8x8 tile, splat)
//     pairs that provably cannot reach alpha >= 1/255 anywhere in the tile (exact min of the conic
//     quadratic over the tile box) - a result-preserving cull;
//   * binning is a counting sort by tile done inside the preprocess kernel (per-workgroup LDS histogram -> scan over the
//     tiles -> the workgroup's own region of the key buffer; no cross-workgroup prefix, no global atomics), followed by a
//     per-tile gather + depth sort in LDS (64-bit key = depth bits : Gaussian index, so ties break by index as the
//     reference's stable radix sort does); no global 64-bit radix sort and no device->host read of the pair count;
//   * the blend kernels cut a tile's list into segments, one per wave: transmittance and the backward's accumulators are
//     linear recurrences, so a segment needs from its predecessors only a product (and a sum);
//   * SH coefficients (300 of the ~350 input bytes per Gaussian) are staged wave-cooperatively
//     through LDS with 16-byte coalesced loads and read once per set for all of its views, forward and backward.
//
// Built with -ffp-contract=off: projection / EWA / SH arithmetic then evaluates the same expression
// trees as the fp32 oracle (IEEE +,-,*,/ and sqrt are correctly rounded on both sides).
//
// The library is ONE translation unit: this file holds the rasterizer's host side and includes the headers below, stages and operators,
// in the order their text always had, which is the order of the kernels in the code object and with it their addresses
// (tools/compare_code_objects.py is the gate for a change that must not move them).  Every header includes what it uses and
// compiles alone (tools/check_headers.py).
//
//   gsr_common.h       GSR_ABL, constants, GeomRec / PreRec / Grid / Layout / Params, choose_chunk, make_layout, small device helpers,
//                      GSR_CHECK, dispatch_bools
//   gsr_binning.h      K1 preprocess and binning, k_color, the windowed chain
//   gsr_tiles_fwd.h    K5 per-tile sort, K6 / K2 forward tile kernels
//   gsr_backward.h     B1 / B2 backward (preprocess_bwd.inc, twice), pose reductions
//   gsr_cameras.h      camera set-up, with its entry points
//   gsr_covariance.h   covariance kernels, with their entry points
//   gsr_hip.hip        dims_ok, base_params, forward_impl / backward_impl, the rasterizer's entry points; no kernel
//   gsr_image.h        image loss, evaluation metrics, the perceptual distance's head (routines of k_pose_ops)  }
//   gsr_adapter.h      Gaussian adapter                            }  operators next to the raster path, each with its
//   gsr_pose_loss.h    pose loss                                   }  kernels and its own entry points
//   gsr_cost_volume.h  plane-sweep cost volume                     }
//   gsr_lift.h         depth lift, mono cue, Pluecker rays         }
//   gsr_mono_attention.h  mono-guided attention, the MFMA tile helpers (ma_*)  }
//   gsr_attention.h    multi-head attention (k_mha_ops) and the ragged attention of the matcher's transformer (k_ragged_ops), on those helpers; the match assignment's passes and entry points  }
//   gsr_pnp_solver.h   namespace gsr::pnp: host + device arithmetic of the coarse-pose solver (a host program includes it alone)
//   gsr_coarse_pose.h  PnP RANSAC kernels, k_camera_sync, entry points
//   gsr_pose_refine.h  the refined poses and the pose errors (k_pose_ops, which also runs the match assignment's, the keypoint extraction's and the perceptual head's passes)
#include "gsr_common.h"
#include "gsr_binning.h"
#include "gsr_tiles_fwd.h"
#include "gsr_backward.h"
#include "gsr_cameras.h"
#include "gsr_covariance.h"

namespace gsr {

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
// sh_frame_ok: the GSR_FLAG_SH_IN_FRAME bits may be set (only the launches of the scale / rotation form take them: sh_frame_args_ok)
static bool dims_ok(const GsrDims* d, bool sh_frame_ok = false) {
  if (!d || d->abi_version != GSR_ABI_VERSION) return false;
  if (!sh_frame_ok && (d->flags & (GSR_FLAG_SH_IN_FRAME | GSR_FLAG_SH_FRAME_E3NN))) return false;
  if (d->num_views < 0 || d->num_sets < 0 || d->views_per_set < 0 || d->num_gaussians < 0) return false;
  if ((int64_t)d->num_sets * d->views_per_set != d->num_views) return false;
  if (d->height <= 0 || d->width <= 0 || d->height > 32768 || d->width > 32768) return false;
  if (d->sh_coeffs < 0 || d->sh_coeffs > 25 || d->sh_degree < 0 || d->sh_degree > 4) return false;
  if (d->num_views > 65535 || d->pair_capacity < 0 || d->pair_capacity > 0xfffffff0ll) return false;
  {
    int valid = GSR_FLAG_VALID_MASK;
#ifdef GSR_ABLATE
    valid |= GSR_FLAG_ABLATE_MASK;
#endif
    if ((d->flags & ~valid) != 0 || ((d->flags >> 4) & 7) > GSR_EXTRA_LOG) return false;
  }
  const Grid g = make_grid(d->width, d->height);
  if ((int64_t)d->num_views * g.T > 0x7fffffffll) return false;
  const Layout L = make_layout(*d);  // key offsets are 32-bit: slots + page pool must stay below 2^32 keys
  if (L.key_slots + L.key_pages * (size_t)kPage > 0xfffffff0ull) return false;
  return true;
}

static Params base_params(const GsrDims* d, const GsrView* views, const float* means, const float* cov6, const float* opac,
                   const float* colors, const float* extra, void* geom, void* bin, void* img) {
  Params p{};
  p.d = *d;
  p.g = make_grid(d->width, d->height);
  p.chunk = choose_chunk(*d);
  p.rows = (d->num_gaussians + p.chunk - 1) / p.chunk;
  p.views = views; p.means = means; p.cov6 = cov6; p.opac = opac; p.colors = colors; p.extra = extra;
  const Layout L = make_layout(*d);
  char* b = static_cast<char*>(bin);
  p.geom = static_cast<GeomRec*>(geom);
  p.aux = (geom && L.o_aux) ? reinterpret_cast<float4*>(static_cast<char*>(geom) + L.o_aux) : nullptr;
  p.rgbc = geom ? reinterpret_cast<float4*>(static_cast<char*>(geom) + L.o_rgbc) : nullptr;
  p.grad_rows = (geom && (d->flags & GSR_FLAG_BACKWARD_FOLLOWS)) ? reinterpret_cast<float4*>(static_cast<char*>(geom) + L.o_rows) : nullptr;
  p.shj = (geom && saves_jacobian(*d)) ? reinterpret_cast<float4*>(static_cast<char*>(geom) + L.o_shj) : nullptr;
  p.status = reinterpret_cast<GsrStatus*>(b + L.o_status);
  p.counts = reinterpret_cast<uint32_t*>(b + L.o_counts);
  p.pair_mat = reinterpret_cast<uint2*>(b + L.o_counts);
  p.blk_base = reinterpret_cast<uint32_t*>(b + L.o_blk);
  p.blk_total = reinterpret_cast<uint32_t*>(b + L.o_blktot);
  p.key_pages = (uint32_t)L.key_pages;
  p.pool_off = (uint32_t)L.key_slots;
  p.stride = (uint32_t)(L.stride > 0xffffffffull ? 0xffffffffull : L.stride);
  {
    const unsigned long long VTs = (unsigned long long)d->num_views * p.g.T * p.stride;
    const unsigned long long capq = d->pair_capacity > 0 ? (unsigned long long)d->pair_capacity : 0ull;
    p.tail_off = (uint32_t)(VTs > 0xffffffffull ? 0xffffffffull : VTs);
    p.tail_cap = (uint32_t)(capq > VTs ? (capq - VTs > 0xffffffffull ? 0xffffffffull : capq - VTs) : 0ull);
  }
  p.tail_counter = reinterpret_cast<uint32_t*>(&reinterpret_cast<GsrStatus*>(b + L.o_status)->reserved[1]);
  p.page_counter = reinterpret_cast<unsigned long long*>(&reinterpret_cast<GsrStatus*>(b + L.o_status)->reserved[0]);
  p.page_counter_tiles = reinterpret_cast<unsigned long long*>(&reinterpret_cast<GsrStatus*>(b + L.o_status)->reserved[2]);
  p.tile_total = reinterpret_cast<uint32_t*>(b + L.o_total);
  p.ranges = reinterpret_cast<uint2*>(b + L.o_ranges);
  p.keys = reinterpret_cast<unsigned long long*>(b + L.o_keys);
  p.point_list = reinterpret_cast<uint32_t*>(b + L.o_list);
  char* im = static_cast<char*>(img);
  p.final_T = reinterpret_cast<float*>(im + L.o_finalT);
  p.n_contrib = reinterpret_cast<uint32_t*>(im + L.o_ncontrib);
  return p;
}

}  // namespace gsr

using namespace gsr;

static thread_local int g_failed_stage = -1;  // debug mode: stage whose check failed (gsr_last_failed_stage)

struct SrArgs {  // scale / rotation input form: cov6 is (S, N, 7); frames (S, F, 3, 3) or null
  const float* frames;
  int num_frames;
};
// the options of an _ex call as the launches take them: null unless the call is in the scale / rotation form
template <class Options>
static const SrArgs* sr_of(const Options* opt, SrArgs* sr) {
  if (!opt || !opt->scale_rot) return nullptr;
  *sr = {opt->frames, opt->num_frames};
  return sr;
}

// opt->stage_ms of the _ex calls (measurement aid, never on the product path): `run` enqueues the launch chain with a HIP event
// between its kStages stages; the stream is synchronised and the stage durations come back in milliseconds (zeros for an
// empty call).  stage_ms == nullptr: just `run`, without events.
template <int kStages, class Run>
static int with_stage_events(const GsrDims* dims, hipStream_t st, float* stage_ms, Run&& run) {
  if (!stage_ms) return run(nullptr);
  hipEvent_t ev[kStages + 1];
  for (int i = 0; i <= kStages; ++i) GSR_CHECK(hipEventCreate(&ev[i]));
  int rc = run(ev);
  for (int i = 0; i < kStages; ++i) stage_ms[i] = 0.f;
  if (rc == GSR_OK && dims->num_views > 0 && dims->num_gaussians > 0) {
    if (hipStreamSynchronize(st) != hipSuccess) rc = GSR_ERR_LAUNCH;
    for (int i = 0; i < kStages && rc == GSR_OK; ++i)
      if (hipEventElapsedTime(&stage_ms[i], ev[i], ev[i + 1]) != hipSuccess) rc = GSR_ERR_LAUNCH;
  }
  for (int i = 0; i <= kStages; ++i) (void)hipEventDestroy(ev[i]);
  return rc;
}

extern "C" {

int gsr_abi_version(void) { return GSR_ABI_VERSION; }

const char* gsr_build_info(void) {
  return "gsr_hip gfx950 wave64 tile8x8 binning+colour tile-sort+segment-blend single-stream abi5";
}

int gsr_last_failed_stage(void) { return g_failed_stage; }

const char* gsr_stage_name(int backward, int stage) {
  static const char* const fwd[GSR_FWD_STAGES] = {"colour", "preprocess/binning", "count + scans", "emit", "per-tile sort + blend"};
  static const char* const bwd[GSR_BWD_STAGES] = {"blend_bwd", "preprocess_bwd"};
  if (stage < 0 || stage >= (backward ? GSR_BWD_STAGES : GSR_FWD_STAGES)) return nullptr;
  return backward ? bwd[stage] : fwd[stage];
}

// 1 when gsr_forward runs the colour pass inside the binning launch for these dims (k_preprocess_bin<true, .>: two launches),
// 0 when it is a launch of its own (three or more), negative on bad dims.  Measurement aid (bench.py attributes bytes to launches).
// Per device, once: more than 64 KB of dynamic LDS has to be asked for.  The plain binning kernel needs 64 KB + the tile counters;
// the variants with the colour pass inside want all of a CU's 160 KB - a device (or runtime) that does not grant that runs the
// colour pass as a launch of its own instead (bit in g_color_bin_ok).
static std::atomic<unsigned long long> g_lds_set{0ull}, g_color_bin_ok{0ull};
// The instances of k_preprocess_bin, named here and nowhere else, each with the most dynamic LDS it is launched with: ensure_bin_attributes
// walks them all, forward_impl picks one.  0: plain; 1: plain, two workgroups per CU; 2 + kJ + 2 * kShFrame: the colour pass inside.
struct BinInstance {
  void (*kernel)(const Params);
  int max_lds;
};
constexpr int kBinInstances = 6;
static BinInstance bin_instance(int i) {
  if (i == 0) return {k_preprocess_bin<false, false>, (int)bin_lds_bytes(kFusedMaxTiles, false)};
  if (i == 1) return {k_preprocess_bin<false, false, kBinTwoMaxT>, (int)bin_lds_bytes(kBinTwoMaxT, false)};
  BinInstance b{nullptr, 160 * 1024 - 10400};
  // (the bools negated: the four are then emitted in the order of their indices, where the code object has always had them)
  dispatch_bools([&](auto no_frame, auto no_j) { b.kernel = k_preprocess_bin<true, !no_j.value, kFusedMaxTiles, !no_frame.value>; }, i < 4, (i & 1) == 0);
  return b;
}
static int ensure_bin_attributes(int* dev_out) {
  int dev = 0;
  GSR_CHECK(hipGetDevice(&dev));
  if (dev_out) *dev_out = dev;
  const unsigned long long bit = 1ull << (dev & 63);
  if (g_lds_set.load(std::memory_order_acquire) & bit) return GSR_OK;
  bool ok = true;
  for (int i = 0; i < kBinInstances; ++i) {
    const BinInstance b = bin_instance(i);
    const hipError_t err = hipFuncSetAttribute(reinterpret_cast<const void*>(b.kernel), hipFuncAttributeMaxDynamicSharedMemorySize, b.max_lds);
    if (i < 2) GSR_CHECK(err);
    else ok = ok && err == hipSuccess;
  }
  if (ok) g_color_bin_ok.fetch_or(bit, std::memory_order_relaxed);
  else (void)hipGetLastError();
  g_lds_set.fetch_or(bit, std::memory_order_release);
  return GSR_OK;
}
static bool color_in_bin_for(const GsrDims& d, const Grid& g, int dev) {
  return color_in_bin_by_dims(d, g) && ((g_color_bin_ok.load(std::memory_order_relaxed) >> (dev & 63)) & 1ull);
}
int gsr_colour_in_binning(const GsrDims* dims) {
  if (!dims_ok(dims)) return GSR_ERR_INVALID_ARGUMENT;
  int dev = 0;
  const int rc = ensure_bin_attributes(&dev);
  if (rc != GSR_OK) return rc;
  return color_in_bin_for(*dims, make_grid(dims->width, dims->height), dev) ? 1 : 0;
}

// Debug aid for tests: the host statement of the forward tile launch's deal (gsr_common.h: tile_deal_order_host) for one XCD.
int gsr_tile_deal_order(const uint32_t* walked, const uint32_t* list_length, int count, uint32_t* order_out) {
  if (!walked || !list_length || !order_out || count < 1 || count > kBalanceMax) return GSR_ERR_INVALID_ARGUMENT;
  tile_deal_order_host(walked, list_length, count, order_out);
  return GSR_OK;
}

static size_t scratch_bytes_of(const GsrDims& d) {
  const size_t rows = (size_t)d.num_views * (size_t)d.num_gaussians;
  if (!(d.flags & GSR_FLAG_DETERMINISTIC)) return rows * GSR_SCREEN_GRAD_FLOATS * sizeof(float);
  return rows * GSR_SCREEN_GRAD_FLOATS * sizeof(long long) + (size_t)d.num_views * sizeof(uint32_t);  // + the views' words (det_max_words)
}
size_t gsr_backward_scratch_bytes(const GsrDims* dims) {
  if (!dims_ok(dims)) return 0;
  return scratch_bytes_of(*dims);
}

int gsr_workspace_sizes(const GsrDims* dims, size_t* geom_bytes, size_t* bin_bytes, size_t* img_bytes) {
  if (!dims_ok(dims)) return GSR_ERR_INVALID_ARGUMENT;
  const Layout L = make_layout(*dims);
  if (geom_bytes) *geom_bytes = L.geom_bytes;
  if (bin_bytes) *bin_bytes = L.bin_bytes;
  if (img_bytes) *img_bytes = L.img_bytes;
  return GSR_OK;
}

int64_t gsr_capacity_for(const GsrDims* dims, uint64_t num_pairs, uint32_t max_list) {
  if (!dims_ok(dims)) return GSR_ERR_INVALID_ARGUMENT;
  const Grid g = make_grid(dims->width, dims->height);
  // every (view, tile) owns capacity / (2 views tiles) entries of the index list; a list longer than that takes a run of the
  // shared second half.  So the slot need not fit the ONE longest list of the call: twice the mean length (or the longest,
  // if shorter) keeps all but a few outliers in their slots and bounds the workspace by 4 x the pairs whatever the skew.
  const uint64_t VT = (uint64_t)dims->num_views * (uint64_t)g.T;
  const uint64_t twice_mean = VT ? 2 * ((num_pairs + VT - 1) / VT) : 0;
  const uint64_t slot = max_list < twice_mean ? max_list : (twice_mean > 256 ? twice_mean : (max_list < 256 ? max_list : 256));
  const uint64_t slots = VT * slot;
  return (int64_t)(2 * (slots > num_pairs ? slots : num_pairs));
}

// Debug aid for tests: byte offsets of the sub-buffers inside bin (6), img (2) and, appended, bin's tile_order.
int gsr_workspace_layout(const GsrDims* dims, int64_t* offsets9) {
  if (!dims_ok(dims) || !offsets9) return GSR_ERR_INVALID_ARGUMENT;
  const Layout L = make_layout(*dims);
  offsets9[0] = (int64_t)L.o_status; offsets9[1] = (int64_t)L.o_counts; offsets9[2] = (int64_t)L.o_total;
  offsets9[3] = (int64_t)L.o_ranges; offsets9[4] = (int64_t)L.o_keys; offsets9[5] = (int64_t)L.o_list;
  offsets9[6] = (int64_t)L.o_finalT; offsets9[7] = (int64_t)L.o_ncontrib;
  offsets9[8] = (int64_t)L.o_order;
  return GSR_OK;
}

int gsr_geom_layout(const GsrDims* dims, int64_t* offsets4) {
  if (!dims_ok(dims) || !offsets4) return GSR_ERR_INVALID_ARGUMENT;
  const Layout L = make_layout(*dims);
  offsets4[0] = (int64_t)sizeof(GeomRec);
  offsets4[1] = L.o_aux ? (int64_t)L.o_aux : -1;
  offsets4[2] = (int64_t)L.o_rgbc;
  offsets4[3] = (dims->flags & GSR_FLAG_BACKWARD_FOLLOWS) ? (int64_t)L.o_rows : -1;
  return GSR_OK;
}

static bool sr_ok(const GsrDims* d, const SrArgs* sr) {
  if (!sr) return true;
  if (d->flags & GSR_FLAG_COV_3X3) return false;
  if (!sr->frames) return sr->num_frames == 0;
  return sr->num_frames > 0 && d->num_gaussians % sr->num_frames == 0;
}
// the call shape of the launches: GSR_FLAG_SH_IN_FRAME needs the scale / rotation form with frames and harmonics; the e3nn bit
// goes with it
static bool call_dims_ok(const GsrDims* d, const SrArgs* sr) {
  if (!d) return false;
  const int fl = d->flags & (GSR_FLAG_SH_IN_FRAME | GSR_FLAG_SH_FRAME_E3NN);
  if (fl && (!(fl & GSR_FLAG_SH_IN_FRAME) || !sr || !sr->frames || d->sh_coeffs <= 0)) return false;
  return dims_ok(d, true) && sr_ok(d, sr);
}

// debug (flags bit 1, upstream's `debug`): synchronise and check after every stage, report the stage that failed
#define GSR_STAGE_DONE(idx)                                                            \
  do {                                                                                  \
    if (d.flags & GSR_FLAG_DEBUG) {                                                     \
      if (hipStreamSynchronize(st) != hipSuccess || hipGetLastError() != hipSuccess) {  \
        g_failed_stage = (idx);                                                         \
        return GSR_ERR_LAUNCH;                                                          \
      }                                                                                 \
    }                                                                                   \
  } while (0)
// the events of with_stage_events: one between every two stages (ev: null on the product path)
#define GSR_MARK() do { if (ev) GSR_CHECK(hipEventRecord(ev[e++], st)); } while (0)

static_assert(sizeof(GsrForwardOptions) == 32 && sizeof(GsrBackwardOptions) == 56, "options structs as tests/test_abi.py mirrors them");

static int forward_impl(const GsrDims* dims, const GsrView* views, const float* means, const float* cov6,
                        const float* opacities, const float* colors, const float* extra, float* out_color,
                        float* out_extra, int32_t* radii, void* geom, void* bin, void* img, hipStream_t st,
                        hipEvent_t* ev, const SrArgs* sr, float* out_alpha) {
  if (!call_dims_ok(dims, sr)) return GSR_ERR_INVALID_ARGUMENT;
  const GsrDims& d = *dims;
  const size_t V = d.num_views, N = d.num_gaussians, HW = (size_t)d.height * d.width;
  if (V == 0) return GSR_OK;
  if (!views || !out_color || !bin || !img) return GSR_ERR_INVALID_ARGUMENT;
  if (d.has_extra && !out_extra) return GSR_ERR_INVALID_ARGUMENT;
  if (d.has_extra && N > 0 && !extra && ((d.flags >> 4) & 7) == 0) return GSR_ERR_INVALID_ARGUMENT;  // (an empty array has no address)
  Params p = base_params(dims, views, means, cov6, opacities, colors, extra, geom, bin, img);
  p.out_color = out_color; p.out_extra = out_extra; p.radii = radii; p.out_alpha = out_alpha;
  if (sr) { p.scale_rot = 1; p.frames = sr->frames; p.num_frames = sr->frames ? sr->num_frames : 1; }
  static std::atomic<uint32_t> call_counter{1u};
  p.call_tag = call_counter.fetch_add(1u, std::memory_order_relaxed);
  const Layout L = make_layout(d);
  if (N == 0) {  // upstream returns an all-zero image when there is nothing to rasterize
    GSR_CHECK(hipMemsetAsync(out_color, 0, V * 3 * HW * sizeof(float), st));
    if (d.has_extra) GSR_CHECK(hipMemsetAsync(out_extra, 0, V * HW * sizeof(float), st));
    if (out_alpha) GSR_CHECK(hipMemsetAsync(out_alpha, 0, V * HW * sizeof(float), st));
    GSR_CHECK(hipMemsetAsync(bin, 0, L.o_counts, st));
    GSR_CHECK(hipMemsetAsync(img, 0, L.img_bytes, st));
    return GSR_OK;
  }
  if (!means || !cov6 || !opacities || !colors || !radii || !geom) return GSR_ERR_INVALID_ARGUMENT;
  const size_t VT = V * (size_t)p.g.T;
  int e = 0;
  const bool do_color = !GSR_ABL(d.flags, GSR_FLAG_ABLATE_NO_SH);
  p.color_units = (uint32_t)((N + 63) / 64);
  const unsigned color_blocks = do_color ? p.color_units * (unsigned)d.num_sets : 0u;
  // One stream, two launches (images of up to 4608 tiles, e.g. 512 x 512): the binning with the colour pass inside it (k_preprocess_bin<true, .>:
  // five of its sixteen waves stream the harmonics while eleven project, count and list the pairs), then one launch per tile for its sort AND its
  // blend.  Larger images: the colour pass as its own first launch (k_color), then the binning chain, then the tile launch.
  // Binning: images of up to kTileWindow tiles take the fused path (k_preprocess_bin, the tile launch gathers);
  // larger ones the windowed path (preprocess, count, prefix, scan, emit, then the tile launch).
  const bool fused_bin = p.g.T <= kFusedMaxTiles && !GSR_ABL(d.flags, GSR_FLAG_ABLATE_NO_COUNT) && !(d.flags & GSR_FLAG_WINDOWED_BINNING);
  int dev = 0;
  {
    const int rc = ensure_bin_attributes(&dev);
    if (rc != GSR_OK) return rc;
  }
  const bool color_in_bin = color_blocks && color_in_bin_for(d, p.g, dev);
  // harmonics in their group's frame (GSR_FLAG_SH_IN_FRAME): the colour passes' own instances
  const bool sh_frame = (d.flags & GSR_FLAG_SH_IN_FRAME) && d.sh_coeffs > 0;
  GSR_MARK();
  if (color_blocks && !color_in_bin)
    dispatch_bools([&](auto frame, auto j) { hipLaunchKernelGGL((k_color<j.value, frame.value>), dim3(color_blocks), dim3(kColorThreads), 0, st, p); },
                   sh_frame, p.shj != nullptr);
  GSR_STAGE_DONE(0);
  GSR_MARK();
  if (fused_bin) {
    // the tile launch's deal: its table from kDealBlocks more workgroups of the binning launch, or from a launch of its own
    if (fwd_deal_active(p) && !color_in_bin) hipLaunchKernelGGL(k_tile_order, dim3(kDealBlocks), dim3(256), 0, st, p);
    const dim3 bgrid((unsigned)p.rows + (fwd_deal_active(p) && color_in_bin ? kDealBlocks : 0), (unsigned)V);
    const size_t shmem = bin_lds_bytes(p.g.T, color_in_bin);
    // (two plain workgroups per CU where the image's tile counters leave the LDS for it: LDS comes in 1280-byte steps)
    const bool two_per_cu = bin_two_per_cu(p.g, color_in_bin);
    const BinInstance b = bin_instance(two_per_cu ? 1 : !color_in_bin ? 0 : 2 + (p.shj != nullptr) + 2 * sh_frame);
    hipLaunchKernelGGL(b.kernel, bgrid, dim3(kBinThreads), shmem, st, p);
  } else {
    hipLaunchKernelGGL(k_preprocess, dim3((unsigned)((N + kPreThreads - 1) / kPreThreads), (unsigned)V), dim3(kPreThreads), 0, st, p);
  }
  GSR_STAGE_DONE(1);
  GSR_MARK();
  if (!fused_bin) {
    hipLaunchKernelGGL(k_count, dim3((unsigned)p.rows, (unsigned)V), dim3(kBinThreads), 0, st, p);
    hipLaunchKernelGGL(k_tile_prefix, dim3((unsigned)((VT + 15) / 16)), dim3(1024), 0, st, p);
  }
  const bool scan_in_emit = VT <= (size_t)kEmitScanMax && p.g.T <= kTileWindow;
  if (!fused_bin && !scan_in_emit) hipLaunchKernelGGL(k_tile_scan, dim3(tile_scan_blocks(VT)), dim3(1024), 0, st, p);
  GSR_STAGE_DONE(2);
  GSR_MARK();
  if (!fused_bin) {
    if (scan_in_emit) hipLaunchKernelGGL(k_emit<true>, dim3((unsigned)p.rows, (unsigned)V), dim3(kBinThreads), 0, st, p);
    else hipLaunchKernelGGL(k_emit<false>, dim3((unsigned)p.rows, (unsigned)V), dim3(kBinThreads), 0, st, p);
  }
  GSR_STAGE_DONE(3);
  GSR_MARK();
  p.sort_blocks = (uint32_t)VT;
  {
    const dim3 tgrid((unsigned)VT);
    const bool extra = d.has_extra != 0, alpha = out_alpha != nullptr;  // (alpha: the kAlpha instances, which also store 1 - final_T)
    // every list that sits in its slot is at most `stride` long: a small slot means short lists, and the 2048-key variant
    // (windowed chain: lists are contiguous ranges of any length; short ones on average - a large image - sort in the 2048-key
    // variant, whose smaller LDS footprint lets six workgroups share a CU; a list longer than the LDS array sorts in memory either way)
    auto tiles = [&](auto gather, bool short_lists) {
      dispatch_bools([&](auto a, auto sh, auto x) { hipLaunchKernelGGL((k_tile_fwd<decltype(gather)::value, sh.value ? 2048 : 4096, x.value, a.value>), tgrid, dim3(kFwdThreads), 0, st, p); },
                     alpha, short_lists, extra);
    };
    // (more tiles than five workgroups per CU hold at once: the compact instance, six per CU.  Round 5: with the extra channel too - until
    // stage A formed its weights after the death decision (blend_range) that instance spilled the record in flight at 80 registers)
    const bool compact = VT > (size_t)GSR_PF_COMPACT_MIN_TILES;
    if (!fused_bin) tiles(std::false_type{}, VT > 0 && (size_t)d.pair_capacity / VT <= (size_t)GSR_WINDOWED_SHORT);
    // the usual case (cursor gather + prefix rank): long lists.  A slot of at most kPrefix (+ 25 %) entries means lists that are
    // ranked whole anyway - many small tiles, e.g. one 1024 x 1024 view of the 300 k scene: 78 entries per tile.  With the 32 KB
    // instance those were better off with k_tile_fwd's smaller LDS footprint (192 vs 217 us for that view, round 4); the COMPACT
    // instance (25.8 KB, 80 registers: six workgroups per CU, like k_tile_fwd's) keeps its cheaper gather - no scan over the rows,
    // four barriers fewer - and takes them when the call has more tiles than the chip holds at once: that view 174.3 -> 167.3 us.
    else if (p.stride <= 2048u && (p.stride > (uint32_t)(kPrefix + kPrefix / 4) || compact) && p.rows <= kSortThreads)
      dispatch_bools([&](auto a, auto x, auto c) { hipLaunchKernelGGL((k_tile_fwd_prefix<x.value, c.value, a.value>), tgrid, dim3(kFwdThreads), 0, st, p); }, alpha, extra, compact);
    else tiles(std::true_type{}, p.stride <= 2048u);
  }
  GSR_STAGE_DONE(4);
  GSR_MARK();
  GSR_CHECK(hipGetLastError());
  return GSR_OK;
}

int gsr_forward_ex(const GsrDims* dims, const GsrView* views, const float* means, const float* cov, const float* opacities,
                   const float* colors, const float* extra, float* out_color, float* out_extra, int32_t* radii, void* geom,
                   void* bin, void* img, const GsrForwardOptions* opt, void* stream_) {
  hipStream_t st = static_cast<hipStream_t>(stream_);
  SrArgs sr_store;
  const SrArgs* sr = sr_of(opt, &sr_store);
  return with_stage_events<GSR_FWD_STAGES>(dims, st, opt ? opt->stage_ms : nullptr, [&](hipEvent_t* ev) {
    return forward_impl(dims, views, means, cov, opacities, colors, extra, out_color, out_extra, radii, geom, bin, img, st, ev, sr,
                        opt ? opt->out_alpha : nullptr);
  });
}

int gsr_forward(const GsrDims* dims, const GsrView* views, const float* means, const float* cov6,
                const float* opacities, const float* colors, const float* extra, float* out_color,
                float* out_extra, int32_t* radii, void* geom, void* bin, void* img, void* stream) {
  return gsr_forward_ex(dims, views, means, cov6, opacities, colors, extra, out_color, out_extra, radii, geom, bin, img, nullptr, stream);
}

static int backward_impl(const GsrDims* dims, const GsrView* views, const float* means, const float* cov6,
                         const float* opacities, const float* colors, const float* extra, const void* geom,
                         const void* bin, const void* img, const float* dL_dcolor, const float* dL_dextra_img,
                         void* scratch, float* dL_dmeans, float* dL_dcov6, float* dL_dopacities,
                         float* dL_dcolors, float* dL_dextra, float* dL_dmeans2D, hipStream_t st, hipEvent_t* ev,
                         const SrArgs* sr, float* dL_dviews, float* pose_partials, int depth_term_only,
                         const float* dL_dalpha_img) {
  if (!call_dims_ok(dims, sr)) return GSR_ERR_INVALID_ARGUMENT;
  const GsrDims& d = *dims;
  const size_t V = d.num_views, N = d.num_gaussians;
  if (V == 0 || N == 0) return GSR_OK;
  const bool own_rows = !scratch && (d.flags & GSR_FLAG_BACKWARD_FOLLOWS);  // zero-filled by the forward, inside geom
  if (!views || !means || !cov6 || !opacities || !colors || !geom || !bin || !img || !dL_dcolor || (!scratch && !own_rows) ||
      !dL_dmeans || !dL_dcov6 || !dL_dopacities || !dL_dcolors)
    return GSR_ERR_INVALID_ARGUMENT;
  Params p = base_params(dims, views, means, cov6, opacities, colors, extra, const_cast<void*>(geom),
                         const_cast<void*>(bin), const_cast<void*>(img));
  p.dL_dcolor = dL_dcolor; p.dL_dextra_img = d.has_extra ? dL_dextra_img : nullptr; p.dL_dalpha_img = dL_dalpha_img;
  if (sr) { p.scale_rot = 1; p.frames = sr->frames; p.num_frames = sr->frames ? sr->num_frames : 1; }
  p.scratch = own_rows ? reinterpret_cast<float*>(p.grad_rows) : static_cast<float*>(scratch);
  p.dL_dmeans = dL_dmeans; p.dL_dcov6 = dL_dcov6; p.dL_dopac = dL_dopacities; p.dL_dcolors = dL_dcolors;
  p.dL_dextra = d.has_extra ? dL_dextra : nullptr; p.dL_dmeans2D = dL_dmeans2D;
  int e = 0;
  GSR_MARK();
  const bool det = (d.flags & GSR_FLAG_DETERMINISTIC) != 0;
  if (!own_rows) GSR_CHECK(hipMemsetAsync(scratch, 0, scratch_bytes_of(d), st));
  if (det) {  // the views' largest cotangents, behind the rows (the forward's zero-fill of rows inside geom stops at the rows)
    uint32_t* words = reinterpret_cast<uint32_t*>(reinterpret_cast<long long*>(p.scratch) + V * N * GSR_SCREEN_GRAD_FLOATS);
    if (own_rows) GSR_CHECK(hipMemsetAsync(words, 0, V * sizeof(uint32_t), st));
    const size_t HW = (size_t)d.height * d.width;
    const unsigned mblocks = (unsigned)std::min<size_t>(128, std::max<size_t>(1, (3 * HW / 4 + 255) / 256));
    hipLaunchKernelGGL(k_cotangent_max, dim3((unsigned)V, mblocks), dim3(256), 0, st, p, words);
  }
  const dim3 bgrid((unsigned)p.g.T, (unsigned)V);
  dispatch_bools([&](auto a, auto x, auto dt) { hipLaunchKernelGGL((k_blend_bwd<x.value, dt.value, a.value>), bgrid, dim3(kBwdThreads), 0, st, p); },
                 dL_dalpha_img != nullptr, p.dL_dextra_img != nullptr, det);
  GSR_STAGE_DONE(0);
  GSR_MARK();
  const int rowf = 3 * d.sh_coeffs, ldstride = rowf | 1;
  const size_t shmem = d.sh_coeffs > 0 ? (size_t)64 * ldstride * sizeof(float) : 0;
  const dim3 pgrid((unsigned)((N + 63) / 64), (unsigned)d.num_sets);
  const bool sh_frame = (d.flags & GSR_FLAG_SH_IN_FRAME) && d.sh_coeffs > 0;
  auto launch_pbwd = [&](auto pose) {  // the instance of the call: camera gradient, saved Jacobian, harmonics in their frame
    dispatch_bools([&](auto frame, auto j) {
      if (det) hipLaunchKernelGGL((k_preprocess_bwd_det<decltype(pose)::value, j.value, frame.value>), pgrid, dim3(64), shmem, st, p);
      else hipLaunchKernelGGL((k_preprocess_bwd<decltype(pose)::value, j.value, frame.value>), pgrid, dim3(64), shmem, st, p);
    }, sh_frame, p.shj != nullptr);
  };
  if (dL_dviews && depth_term_only) {
    if (!pose_partials) return GSR_ERR_INVALID_ARGUMENT;
    p.pose_partials = pose_partials;
    const int emode = (d.flags >> 4) & 7;
    if (!d.has_extra || emode == 0) {  // no built-in depth channel: nothing of this call reads the camera's z row
      GSR_CHECK(hipMemsetAsync(dL_dviews, 0, V * sizeof(GsrView), st));
      launch_pbwd(std::integral_constant<int, 0>{});
    } else {
      launch_pbwd(std::integral_constant<int, 2>{});
      // one 16-byte row per (view, 64-Gaussian unit): up to 16 384 rows per view are summed by one block per view in one launch
      const int rows1 = (int)pgrid.x, blocks1 = rows1 <= 16384 ? 1 : 64;
      float* level1 = pose_partials + (size_t)V * rows1 * kPoseZFloats;  // behind the rows of the first level
      if (blocks1 > 1) {
        hipLaunchKernelGGL(k_pose_reduce_z, dim3((unsigned)V, (unsigned)blocks1), dim3(256), 0, st, pose_partials, rows1, level1, 0);
        hipLaunchKernelGGL(k_pose_reduce_z, dim3((unsigned)V, 1), dim3(256), 0, st, level1, blocks1, dL_dviews, 1);
      } else {
        hipLaunchKernelGGL(k_pose_reduce_z, dim3((unsigned)V, 1), dim3(256), 0, st, pose_partials, rows1, dL_dviews, 1);
      }
    }
  } else if (dL_dviews) {
    if (!pose_partials) return GSR_ERR_INVALID_ARGUMENT;
    p.pose_partials = pose_partials;
    const int rows1 = (int)pgrid.x * 4;
    auto full = [&](auto pose, auto cols) {  // the rows of `cols` floats, then their two-level sum (level 1 behind the rows)
      constexpr int kCols = decltype(cols)::value;
      launch_pbwd(pose);
      float* level1 = pose_partials + (size_t)V * rows1 * kCols;
      hipLaunchKernelGGL(k_pose_reduce<kCols>, dim3((unsigned)V, kPoseBlocks), dim3(256), 0, st, pose_partials, rows1, level1, kCols, kPoseBlocks);
      hipLaunchKernelGGL(k_pose_reduce<kCols>, dim3((unsigned)V, 1), dim3(256), 0, st, level1, kPoseBlocks, dL_dviews, 48, 1);
    };
    if (d.flags & GSR_FLAG_FOV_GRADIENT) full(std::integral_constant<int, 3>{}, std::integral_constant<int, kPoseFovFloats>{});  // (pose_partials: 37-float rows)
    else full(std::integral_constant<int, 1>{}, std::integral_constant<int, kPoseFloats>{});
  } else {
    launch_pbwd(std::integral_constant<int, 0>{});
  }
  GSR_STAGE_DONE(1);
  GSR_MARK();
  GSR_CHECK(hipGetLastError());
  return GSR_OK;
}

size_t gsr_pose_partials_bytes(const GsrDims* dims) {
  if (!dims_ok(dims)) return 0;
  const int cols = (dims->flags & GSR_FLAG_FOV_GRADIENT) ? kPoseFovFloats : kPoseFloats;
  return (size_t)dims->num_views * ((size_t)((dims->num_gaussians + 63) / 64) * 4 + kPoseBlocks) * cols * sizeof(float);
}

int gsr_backward_ex(const GsrDims* dims, const GsrView* views, const float* means, const float* cov, const float* opacities,
                    const float* colors, const float* extra, const void* geom, const void* bin, const void* img,
                    const float* dL_dcolor, const float* dL_dextra_img, void* scratch, float* dL_dmeans, float* dL_dcov,
                    float* dL_dopacities, float* dL_dcolors, float* dL_dextra, float* dL_dmeans2D, const GsrBackwardOptions* opt,
                    void* stream_) {
  hipStream_t st = static_cast<hipStream_t>(stream_);
  SrArgs sr_store;
  const SrArgs* sr = sr_of(opt, &sr_store);
  return with_stage_events<GSR_BWD_STAGES>(dims, st, opt ? opt->stage_ms : nullptr, [&](hipEvent_t* ev) {
    return backward_impl(dims, views, means, cov, opacities, colors, extra, geom, bin, img, dL_dcolor, dL_dextra_img, scratch, dL_dmeans, dL_dcov,
                         dL_dopacities, dL_dcolors, dL_dextra, dL_dmeans2D, st, ev, sr, opt ? opt->dL_dviews : nullptr,
                         opt ? opt->pose_partials : nullptr, opt ? opt->depth_term_only : 0, opt ? opt->dL_dalpha_img : nullptr);
  });
}

int gsr_backward(const GsrDims* dims, const GsrView* views, const float* means, const float* cov6,
                 const float* opacities, const float* colors, const float* extra, const void* geom,
                 const void* bin, const void* img, const float* dL_dcolor, const float* dL_dextra_img,
                 void* scratch, float* dL_dmeans, float* dL_dcov6, float* dL_dopacities,
                 float* dL_dcolors, float* dL_dextra, float* dL_dmeans2D, void* stream) {
  return gsr_backward_ex(dims, views, means, cov6, opacities, colors, extra, geom, bin, img, dL_dcolor, dL_dextra_img, scratch, dL_dmeans, dL_dcov6,
                         dL_dopacities, dL_dcolors, dL_dextra, dL_dmeans2D, nullptr, stream);
}

int gsr_mark_visible(const GsrDims* dims, const GsrView* views, const float* means, uint8_t* present, void* stream_) {
  if (!dims_ok(dims) || !views || !present) return GSR_ERR_INVALID_ARGUMENT;
  if (dims->num_gaussians == 0 || dims->num_sets == 0) return GSR_OK;
  if (!means) return GSR_ERR_INVALID_ARGUMENT;
  Params p{};
  p.d = *dims; p.g = make_grid(dims->width, dims->height); p.views = views; p.means = means;
  hipLaunchKernelGGL(k_mark_visible, dim3((unsigned)((dims->num_gaussians + 255) / 256), (unsigned)dims->num_sets),
                     dim3(256), 0, static_cast<hipStream_t>(stream_), p, present);
  GSR_CHECK(hipGetLastError());
  return GSR_OK;
}

}  // extern "C"

// The operators next to the raster path (see the map at the top of this file).
#include "gsr_image.h"
#include "gsr_adapter.h"
#include "gsr_pose_loss.h"
#include "gsr_cost_volume.h"
#include "gsr_lift.h"
#include "gsr_mono_attention.h"
#include "gsr_attention.h"
#include "gsr_pnp_solver.h"
#include "gsr_coarse_pose.h"
#include "gsr_pose_refine.h"
