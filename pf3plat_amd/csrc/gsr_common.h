#pragma once
// gsr_common.h - what every other file of the library builds on: the ablation switch, the constants, the records and layouts of the
// workspaces, the launch parameters, the chunk choice and the small device helpers.  (Map of the files: gsr_hip.hip.)
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <algorithm>
#include <atomic>
#include <type_traits>

#include "../../include/gsr.h"

// Measurement-only switches (tools/ablate.py builds its own library with -DGSR_ABLATE): ablation bits that make results
// WRONG on purpose and device-side phase stamps.  The product library is compiled without them - the branches do not
// exist in it, and dims_ok() rejects the bits.
#ifdef GSR_ABLATE
#define GSR_ABL(flags, bit) (((flags) & (bit)) != 0)
#else
#define GSR_ABL(flags, bit) false
#endif

namespace gsr {

constexpr int kChunkMax = 2048;   // most Gaussians per binning workgroup (= one row of the per-view count matrix)
constexpr int kChunkMin = 1024;    // ... unless ONE round of smaller chunks (down to kChunkSmall) still fits the chip: see choose_chunk
constexpr int kChunkSmall = 512;
constexpr int kCUs = 256;
// de-phasing of a tile launch's first resident round (sort_tile, k_tile_fwd_prefix): group = the workgroup's residency slot on its CU
constexpr int kDephaseShift = 8, kDephaseGroups = 4;
constexpr int kBinThreads = 1024; // threads of a binning workgroup (count / emit)
constexpr int kTileWindow = 8192; // tiles histogrammed in LDS at a time by a binning workgroup of the WINDOWED chain (32 KiB, static)
#ifndef GSR_FUSED_MAX_TILES
#define GSR_FUSED_MAX_TILES 20480
#endif
// most tiles of an image that takes the fused binning launch (k_preprocess_bin: its per-tile counters are dynamic LDS, T x 4 bytes
// next to the 64 KB record-transpose / pair-staging area and ~10 KB of static LDS); larger images take the windowed chain.
// (Round 2 stopped at 8192; one 1024 x 1024 view of the 300 k scene: 236 us through the windowed chain, 187 us this way.)
constexpr int kFusedMaxTiles = GSR_FUSED_MAX_TILES;
static_assert(kFusedMaxTiles % 1024 == 0 && kFusedMaxTiles >= kTileWindow && 65536 + kFusedMaxTiles * 4 + 10400 <= 160 * 1024, "LDS of the fused binning launch");
constexpr int kSortThreads = 256; // threads cooperating on one tile's sort
constexpr int kPage = 1024;        // pairs per page of the key buffer: a binning workgroup's private region is whole pages
constexpr int kSlotStride = 8192 + 136;  // keys between the fixed slots of consecutive binning workgroups: NOT a multiple of the memory
                                        // channel interleave - the sort reads the same tile from every slot at once, and with a
                                        // power-of-two stride all those reads landed on one channel (gather 16 us instead of 3)
constexpr int kStagePairs = 8192;  // pairs a binning workgroup collects in LDS (the 64 KB record-transpose area) before one linear copy-out
constexpr float kNear = 0.2f;     // [EXT] auxiliary.h in_frustum: p_view.z <= 0.2f culls

struct __attribute__((aligned(32))) GeomRec {  // 32 B per (view, Gaussian): everything the blends gather, nothing else
  float4 q0;  // x, y, conic a, conic b
  float4 q1;  // conic c, opacity, extra channel, bits(radius)
};
// What preprocess_one produces: the record plus the footprint word q3 = bits(hit mask lo), bits(hit mask hi),
// bits(window origin: sx0 | sy0 << 12 | big << 31), depth.  The mask lists the 8x8 tiles this splat must be listed in, over
// the 8x8-tile window whose top-left tile is (sx0, sy0) (bit = (sy - sy0) * 8 + (sx - sx0)); footprints wider than 8 tiles set
// `big` and are re-derived from the record by the binning kernels.  The fused binning launch consumes q3 from registers; only
// the windowed chain (k_preprocess -> k_count / k_emit) keeps it in memory (Params::aux, 16 B per (view, Gaussian)).
struct PreRec {
  float4 q0, q1, q3;
};
// The view-dependent colour lives in its own array (float4 per (view, Gaussian): r, g, b, bits(clamp mask)) because it is
// produced by the colour pass (k_color / color_unit), not by the geometry/binning kernel.

typedef unsigned long long ull2 __attribute__((ext_vector_type(2), aligned(8)));  // two keys, 8-byte aligned

struct Grid {
  int W, H, gx16, gy16, sgx, sgy, sw, sh, T;  // sw/sh: 8x8 tiles that contain at least one pixel
};

__host__ __device__ inline Grid make_grid(int W, int H) {
  Grid g;
  g.W = W; g.H = H;
  g.gx16 = (W + 15) / 16; g.gy16 = (H + 15) / 16;
  g.sgx = 2 * g.gx16; g.sgy = 2 * g.gy16;
  g.sw = (W + 7) / 8; g.sh = (H + 7) / 8;
  g.T = g.sgx * g.sgy;
  return g;
}

struct Layout {
  size_t geom_bytes, bin_bytes, img_bytes;
  size_t o_aux, o_rgbc, o_rows, o_shj;  // o_aux: 0 = none (fused binning path)  // in geom (only with GSR_FLAG_BACKWARD_FOLLOWS: o_rows screen-space gradient rows, o_shj d rgb / d direction)
  size_t o_status, o_counts, o_total, o_ranges, o_keys, o_list, o_blk, o_blktot, o_order;  // in bin
  size_t key_slots;  // keys: one fixed slot of kStagePairs keys per binning workgroup, then ...
  size_t key_pages;  // ... a pool of pages of kPage keys (regions / scratch too long for a slot)
  size_t stride;     // fused binning: entries of the index list owned by every (view, tile)
  size_t o_finalT, o_ncontrib;                                   // in img
};

static inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

// Gaussians per binning workgroup.  The binning kernels are latency/VALU bound per workgroup, so the chip is fullest
// when one round of workgroups covers all CUs: the chunk (a multiple of 64 in [kChunkMin, kChunkMax]) that minimises
// rounds x chunk, the larger one on ties (fewer rows in the count matrix).
// Chunks above kChunkPrefer are not considered: a workgroup stages its pairs in LDS (kStagePairs = 8192) for one linear copy-out,
// and at the ~4.2 pairs per Gaussian of PF3plat-shaped scenes a 2048-Gaussian chunk lists ~8600 - past the staging area, every
// pair then leaves as an 8-byte store of its own (measured: 48 views x 131 072 Gaussians chose 2048 by a tie and the binning
// launch took 2437 us instead of ~600).
constexpr int kChunkPrefer = 1600;
#ifndef GSR_BIN_TWO
#define GSR_BIN_TWO 1  // 0: measurement builds without the two-per-CU instance of the plain binning launch
#endif
#ifndef GSR_CIB_MAX_VPS
#define GSR_CIB_MAX_VPS 4  // most views per set whose colour pass runs inside the binning launch (see color_in_bin_for)
#endif
// (a launch whose workgroups sit two to a CU - the plain binning launch of a small image, k_preprocess_bin<false, false, 2048> - has
// twice the slots per round: 8 views of 300 k Gaussians then take 1600-Gaussian chunks, three rounds, instead of 1344, four)
// ONE statement of "which binning launch will this call take", shared by the chunk choice (host arithmetic at sizing time) and by
// forward_impl (defined behind bin_lds_bytes, next to the launch): the colour pass inside the binning launch as far as the call's
// dims say (forward_impl adds what only the device knows: whether it granted the LDS attribute), and whether the plain launch's
// workgroups sit two to a CU (LDS in 1280-byte steps: images of up to 1496 tiles).
static bool color_in_bin_by_dims(const GsrDims& d, const Grid& g);
static bool bin_two_per_cu(const Grid& g, bool color_in_bin);
// A round of binning workgroups costs its chunk AND a fixed part (prologue, scan, pair walk, copy-out: ~6 of the 23 us a 1600-Gaussian
// workgroup lives) - in Gaussians.  It only decides between chunk sizes that need different numbers of rounds: PF3plat's training batch
// (4 scenes x 3 views x 131 072: 984 workgroups of 1600 in four rounds, against 1536 of 1024 in six as the plain product chose) forward
// 300 -> 292 us; 0 / 400 / 800 measured, forced 1344 / 1408 / 1472 (whole passes of the eleven binning waves) are slower than 1600.
#ifndef GSR_CHUNK_FIXED
#define GSR_CHUNK_FIXED 400
#endif
static int choose_chunk(const GsrDims& d) {
  const long long V = d.num_views > 0 ? d.num_views : 1, N = d.num_gaussians > 0 ? d.num_gaussians : 1;
  const Grid g = make_grid(d.width, d.height);
  const bool plain_two = bin_two_per_cu(g, color_in_bin_by_dims(d, g));
  const long long slots = plain_two ? 2 * kCUs : kCUs;
  long long best_cost = -1;
  int best = kChunkPrefer;
  for (int c = kChunkPrefer; c >= kChunkSmall; c -= 64) {
    const long long blocks = V * ((N + c - 1) / c), cost = ((blocks + slots - 1) / slots) * (c + GSR_CHUNK_FIXED);
    // chunks below kChunkMin only while a single round of workgroups holds them all: one 131 072-Gaussian view (configs[4]'s share of
    // a GPU, PF3plat's native size) took 128 workgroups of 1024 - half the chip idle through the whole binning launch (19.5 us); 256
    // workgroups of 512 are one projection pass per wave instead of two.  With several rounds the per-workgroup prologue, scan and
    // copy-out are paid per round: there the larger chunks stay.
    if (c < kChunkMin && blocks > slots) break;
    if (best_cost < 0 || cost < best_cost) { best_cost = cost; best = c; }
  }
  return best;
}

// Does a forward that announces its backward (GSR_FLAG_BACKWARD_FOLLOWS) save d rgb / d direction per (view, Gaussian) for it?
// The rows are 48 bytes per view and Gaussian, written by the colour pass and read back by k_preprocess_bwd; the alternative - the
// backward reads the harmonics again and re-derives them - is 12 K bytes per Gaussian ONCE for all views of its set, fewer bytes from
// three views per set on.  Measured (fwd + bwd, saved / re-derived): one view 124.8 / 135.8 us, two 107 / 116 per view, three views of
// 131 072 Gaussians 73.0 / 75.0, eight views 86.4 / 89.7 - the re-derivation is arithmetic in a launch that has none to spare; always saved.
#ifndef GSR_SHJ_MAX_VIEWS
#define GSR_SHJ_MAX_VIEWS (1 << 30)
#endif
static inline bool saves_jacobian(const GsrDims& d) {
  return (d.flags & GSR_FLAG_BACKWARD_FOLLOWS) && d.sh_coeffs > 0 && d.views_per_set <= GSR_SHJ_MAX_VIEWS;
}

static Layout make_layout(const GsrDims& d) {
  Layout L;
  const Grid g = make_grid(d.width, d.height);
  const size_t V = d.num_views, N = d.num_gaussians, VT = V * (size_t)g.T;
  const size_t cap = d.pair_capacity > 0 ? (size_t)d.pair_capacity : 0;
  const bool windowed = g.T > kFusedMaxTiles || (d.flags & GSR_FLAG_WINDOWED_BINNING) != 0;
  // every sub-array of `geom` starts on a 2 MiB boundary: the backward kernels gather / scatter by Gaussian index into three of
  // them at once, and with the arrays packed at 256-byte granularity the 300 k-Gaussian training step was 2-3 us slower for
  // some sizes of the first array than for others (measured: 143.5-144.2 us packed, 141.4-142.6 aligned)
#ifndef GSR_GEOM_ALIGN
#define GSR_GEOM_ALIGN 2097152
#endif
  constexpr size_t kGA = GSR_GEOM_ALIGN;
  const size_t rec_bytes = align_up(V * N * sizeof(GeomRec), kGA);
  L.o_aux = windowed ? rec_bytes : 0;
  L.o_rgbc = rec_bytes + (windowed ? align_up(V * N * sizeof(float4), kGA) : 0);
  L.o_rows = L.o_rgbc + align_up(V * N * sizeof(float4), kGA);
  L.o_shj = L.o_rows + ((d.flags & GSR_FLAG_BACKWARD_FOLLOWS)
                            ? align_up((d.flags & GSR_FLAG_DETERMINISTIC) ? V * N * GSR_SCREEN_GRAD_FLOATS * 8 + V * 4  // (det_max_words)
                                                                          : V * N * GSR_SCREEN_GRAD_FLOATS * 4, kGA) : 0);
  L.geom_bytes = L.o_shj + (saves_jacobian(d) ? align_up(V * N * 3 * sizeof(float4), 256) : 0);
  size_t o = 0;
  L.o_status = o; o = align_up(o + sizeof(GsrStatus), 256);
  const size_t rows = (N + choose_chunk(d) - 1) / choose_chunk(d);
  L.o_counts = o; o = align_up(o + V * (rows > 0 ? rows : 1) * (size_t)(g.T + 8) * 8, 256);  // uint2 (offset, count); rows padded by 8
  L.o_total = o; o = align_up(o + VT * 4, 256);
  L.o_ranges = o; o = align_up(o + VT * 8, 256);
  // keys: a fixed slot per binning workgroup (all it needs unless it lists more than kStagePairs pairs), then a page pool
  // for the longer regions and for the contiguous scratch of per-tile lists too long for the LDS sort
  const size_t blocks = V * (rows > 0 ? rows : 1);
  L.key_slots = blocks * (size_t)kSlotStride;
  L.key_pages = (cap + kPage - 1) / kPage + 64;  // (capacity = 2 x pairs, what gsr_capacity_for returns, holds every pair twice)
  L.o_keys = o; o = align_up(o + (L.key_slots + L.key_pages * kPage) * 8 + 64, 256);  // + padding: 16-byte reads may overrun a run by one key
  L.o_list = o; o = align_up(o + cap * 4, 256);
  L.o_blk = o; o = align_up(o + blocks * 4, 256);
  L.o_blktot = o; o = align_up(o + blocks * 4, 256);
  L.o_order = o; o = align_up(o + VT * 4, 256);  // tile_order (device side: tile_order_of - directly behind blk_total)
  L.stride = VT > 0 ? cap / (2 * VT) : 0;  // half of the index list in per-tile slots, the rest a shared tail (longer lists)
  L.bin_bytes = o;
  const size_t px = V * (size_t)d.height * d.width;
  L.o_finalT = 0;
  L.o_ncontrib = align_up(px * 4, 256);
  L.img_bytes = align_up(L.o_ncontrib + px * 4, 256);
  return L;
}

struct Params {
  GsrDims d;
  Grid g;
  int rows;   // binning chunks per view = ceil(N / chunk)
  int chunk;  // Gaussians per binning workgroup (choose_chunk)
  const GsrView* views;
  const float *means, *cov6, *opac, *colors, *extra;
  const float* frames;   // scale/rotation input form (GsrForwardOptions.scale_rot): cov6 points at (S, N, 7) records, frames at
  int num_frames;        // (S, F, 3, 3) rotations (nullable) applied to the Gaussians of each of the F equal groups of a set
  int scale_rot;         // 1: that form is in use
  float* out_color;
  float* out_extra;
  union {
    int32_t* radii;              // forward
    const float* dL_dalpha_img;  // backward - (V, H, W), or null (shares the forward-only pointer's storage: see out_alpha)
  };
  GeomRec* geom;
  float4* aux;  // footprint words of the windowed binning chain (null on the fused path)
  float4* rgbc;
  float4* grad_rows;  // forward with GSR_FLAG_BACKWARD_FOLLOWS: the rows the geometry kernels zero-fill (else null)
  float4* shj;        // same flag, SH colours: d rgb / d (unit view direction) of every (view, Gaussian), 3 x float4 = rows x, y, z
                      // (r, g, b, -): saved by the colour pass so that the backward need not read the harmonics again (else null)
  GsrStatus* status;
  uint32_t* counts;      // windowed path: u32 count matrix; fused path: the same storage as uint2 (offset, count)
  uint2* pair_mat;
  uint32_t* blk_base;    // fused path: first key of every binning workgroup's region (0xffffffff: not stored)
  uint32_t* blk_total;   // fused path: pairs listed by every binning workgroup
  uint32_t key_pages;    // pages in the pool behind the fixed slots
  uint32_t pool_off;     // first key of the pool
  uint32_t stride;       // index-list entries owned by every (view, tile)
  uint32_t tail_off, tail_cap;  // the rest of the index list: lists longer than `stride`, bump-allocated
  uint32_t* tail_counter;
  unsigned long long* page_counter;  // in the status block: (call tag << 32) | pool pages handed out so far by the binning launch
  unsigned long long* page_counter_tiles;  // same form, by the tile launch (its pages are the upper half of the pool)
  uint32_t call_tag;       // unique per gsr_forward call of this process: a counter left by another call reads as zero
  uint32_t sort_blocks;    // workgroups of the tile launch = views x tiles
  uint32_t color_units;    // colour units per set = ceil(N / 64)
  uint32_t* tile_total;
  uint2* ranges;
  unsigned long long* keys;
  uint32_t* point_list;
  float* final_T;
  uint32_t* n_contrib;
  // backward only
  const float *dL_dcolor, *dL_dextra_img;
  float* scratch;
  float *dL_dmeans, *dL_dcov6, *dL_dopac, *dL_dcolors, *dL_dextra, *dL_dmeans2D;  // (scale_rot: dL_dcov6 is (S, N, 7))
  // accumulated alpha (GsrForwardOptions.out_alpha / GsrBackwardOptions.dL_dalpha_img; read by the kAlpha instances only).  The struct keeps its size and
  // every field its offset - kernels that take their arguments from it, copy it or carry an argument behind it are then the code
  // they were - so the two pointers share the storage of one that only the OTHER direction's kernels read.  (A backward kernel that
  // ever needs `radii`, or a forward kernel `pose_partials`, takes that pointer out of its union first.)
  union {
    float* pose_partials;  // backward - camera gradients requested: [view][preprocess_bwd workgroup][DPP row 0..3][kPoseFloats]
    float* out_alpha;      // forward - (V, H, W) 1 - final_T, or null
  };
};
static_assert(sizeof(Params) == 464, "Params as the kernels without kAlpha were built around it");

// ------------------------------------------------------------------------------------------------
// small device helpers
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}
// Inclusive prefix sum over the 64 lanes of a wave, DPP only (no LDS permutes): Hillis-Steele inside each 16-lane row
// (row_shr 1, 2, 4, 8; lanes shifted in from outside the row read 0), then lane 15 of row 0 / 2 into rows 1 / 3
// (row_bcast15) and lane 31 into rows 2 and 3 (row_bcast31).
template <int CTRL, int ROW_MASK, bool BOUND>
__device__ __forceinline__ uint32_t dpp_take_u32(uint32_t v) {
  return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, ROW_MASK, 0xf, BOUND);
}
__device__ __forceinline__ uint32_t wave_inclusive_scan_u32(uint32_t v) {
  v += dpp_take_u32<0x111, 0xf, true>(v);   // row_shr:1
  v += dpp_take_u32<0x112, 0xf, true>(v);   // row_shr:2
  v += dpp_take_u32<0x114, 0xf, true>(v);   // row_shr:4
  v += dpp_take_u32<0x118, 0xf, true>(v);   // row_shr:8
  v += dpp_take_u32<0x142, 0xa, false>(v);  // row_bcast15 -> rows 1 and 3
  v += dpp_take_u32<0x143, 0xc, false>(v);  // row_bcast31 -> rows 2 and 3
  return v;
}
// Maximum over the 64 lanes of a wave (every lane active), DPP rotations inside the 16-lane rows, then the four row results
// through scalar registers.
template <int CTRL>
__device__ __forceinline__ uint32_t dpp_row_max_u32(uint32_t v) {
  const uint32_t o = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xf, 0xf, false);
  return o > v ? o : v;
}
__device__ __forceinline__ uint32_t wave_max_u32(uint32_t v) {
  v = dpp_row_max_u32<0x128>(v);  // row_ror:8
  v = dpp_row_max_u32<0x124>(v);  // row_ror:4
  v = dpp_row_max_u32<0x122>(v);  // row_ror:2
  v = dpp_row_max_u32<0x121>(v);  // row_ror:1
  const uint32_t r0 = (uint32_t)__builtin_amdgcn_readlane((int)v, 0), r1 = (uint32_t)__builtin_amdgcn_readlane((int)v, 16);
  const uint32_t r2 = (uint32_t)__builtin_amdgcn_readlane((int)v, 32), r3 = (uint32_t)__builtin_amdgcn_readlane((int)v, 48);
  const uint32_t a = r0 > r1 ? r0 : r1, b = r2 > r3 ? r2 : r3;
  return a > b ? a : b;
}

// What the colour pass reads of a view: fetched through the CONSTANT address space, i.e. by scalar loads (s_load_dword, the scalar
// cache) into scalar registers - the records are written by an earlier launch and wave-uniform here.  As a plain `p.views[v]` read
// the compiler issues a per-lane global load, and every unit's evaluation then starts by waiting a memory round trip for it
// under the colour stream.  The colour waves of the binning launch ask for the first view's values BEFORE they wait for the
// unit's rows (cam_lite early, `cam0`), so the values are there when the rows are.
struct CamLite { float scale, cx, cy, cz; };
__device__ __forceinline__ CamLite cam_lite(const GsrView* views, int v_uniform) {
  typedef const __attribute__((address_space(4))) float* cptr;
  cptr c = reinterpret_cast<cptr>(reinterpret_cast<uintptr_t>(views + v_uniform));
  return CamLite{c[40], c[32], c[33], c[34]};  // GsrView: scale at float 40, campos at 32..34
}

// The whole record that way (fields that are not used cost nothing): for the kernels whose lanes all work on one view at a time.
__device__ __forceinline__ GsrView view_const(const GsrView* views, int v_uniform) {
  typedef const __attribute__((address_space(4))) float* cptr;
  cptr c = reinterpret_cast<cptr>(reinterpret_cast<uintptr_t>(views + __builtin_amdgcn_readfirstlane(v_uniform)));
  GsrView o;
  float* f = reinterpret_cast<float*>(&o);
#pragma unroll
  for (int k = 0; k < (int)(sizeof(GsrView) / 4); ++k) f[k] = c[k];
  return o;
}

// XCD-aware tile order: workgroup b runs on XCD b % 8 (observed dispatch order; speed only), so give
// each XCD a contiguous run of tiles - neighbouring tiles gather the same splat records from one L2.
__device__ __forceinline__ int xcd_remap(int b, int n) {
  const int q = n >> 3, r = n & 7;
  const int xcd = b & 7, k = b >> 3;
  const int base = xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
  return base + k;
}

// ---- The deal of an XCD's tiles to its 32 CUs by load: heaviest first, every other round of 32 mirrored (k_blend_bwd has the
// measurements).  Shared by k_blend_bwd, which finds its tile from the forward's walked counts, and by the single view's forward
// tile launch, which takes its tile from a table (tile_order) the binning launch builds from what the PREVIOUS forward walked.
constexpr int kBalanceMax = 256;  // tiles per XCD up to which the deal is computed (more: image order; later rounds balance themselves)
// keys (load + 1) << 8 | (255 - index): distinct, heavier first, equal loads in index order.  CORRECTNESS rests on the low 8 bits
// alone - they are distinct, so the deal is a bijection of the XCD's tiles whatever the counts hold (walked counts after a normal
// forward; binning totals or anything else after an overflowed one, or in a fresh workspace) - the load only decides the ORDER; it
// is clamped so that the shift cannot drop its high bits (the order stays monotonic)
__device__ __forceinline__ uint32_t deal_key(uint32_t load, int index) {
  return ((min(load, 0xfffffeu) + 1u) << 8) | (uint32_t)(255 - index);
}
// position in heaviest-first order that the XCD's k-th workgroup takes; its own inverse (the k of the workgroup that takes position k)
__device__ __forceinline__ int deal_position(int k, int cnt) {
  const int round = k >> 5, in = k & 31, len = cnt - (round << 5) < 32 ? cnt - (round << 5) : 32;
  return (round << 5) + ((round & 1) ? len - 1 - in : in);
}
// The forward's deal: one view whose tile workgroups are all resident at once (four per CU) - what a CU is busy for is then the sum
// of its up to four tiles, and nothing rebalances it.  Every other call keeps xcd_remap's image order: several views, more tiles
// than one round, no more tiles than CUs (nothing to balance) - or a binning launch without kDealBlocks idle CUs for the table's
// builders (below): they would be a second round of that launch (one 131 072-Gaussian view, 256 binning workgroups: binning
// 16.7 -> 19.7 us for a tile launch 2.3 us shorter).
constexpr int kDealBlocks = 8;  // one builder workgroup per XCD
__host__ __device__ __forceinline__ bool fwd_deal_active(const Params& p) {
  return p.d.num_views == 1 && p.g.T > kCUs && p.g.T <= 4 * kCUs && p.rows + kDealBlocks <= kCUs;
}
// tile_order: one word per (view, tile), behind blk_total in `bin` (make_layout: o_order)
__device__ __forceinline__ uint32_t* tile_order_of(const Params& p) {
  return p.blk_total + ((((size_t)p.d.num_views * p.rows * 4 + 255) & ~(size_t)255) >> 2);
}
// ---- The forward's deal by a measured time model.  Stamps of the 1024-tile single view under 24 random and 192 structured deals
// (docs/KERNEL_HISTORY.md, profiles/r11_deal_model.md; tools/deal_model.py): the four tile workgroups of a compute unit start their
// blends in the order of their de-phase slots (workgroup >> 8) and END in that order - the tile of slot 3 ended last on 256 of 256
// units - so what a unit is busy for is not the sum of its tiles' batches: its end, in microseconds, follows
//     0.143 n0 + 0.143 n1 + 0.121 n2 + 0.699 n3  +  0.00053 l0 + 0.00035 l1 + 0.00025 l2 + 0.00040 l3  (+ a constant)
// with n_s the batches the tile of slot s walks and l_s its list length (least squares over half of the deals; on the other half
// the modelled slowest unit follows the stamped end of the launch with r = 0.86 - 0.91, the largest batch sum with r = 0.41).
// deal_term is that cost of one tile in one slot in units of 2^-16 us, on the previous call's walked entries (batches x 32:
// tile_total) and list length (ranges); both clamped, so that a unit's four terms and a shift by 5 stay inside 32 bits whatever
// the words hold.  Integer arithmetic: the host's answer (gsr_tile_deal_order, for the tests) is the device's.
constexpr int kDealPasses = 8;          // exchanges per XCD at the most (below)
constexpr int kDealMaxTiles = 128;      // tiles of an XCD the model deals: four slots x 32 units (fwd_deal_active: T <= 4 kCUs)
constexpr uint32_t kDealClamp = 0x3fffu;
// The coefficients were measured on tiles that list 615 - 1663 keys and walk 7 - 14 batches.  Below that range nothing says that a
// unit ends as the model has it, and a light tile launch is not bound by its blends: an XCD whose tiles listed fewer than
// kDealMinMeanList keys on average in the previous call (a fresh workspace lists none) keeps the shipped order.
constexpr uint32_t kDealMinMeanList = 512u;
__host__ __device__ __forceinline__ uint32_t deal_term(const int slot, const uint32_t walked, const uint32_t len) {
  const uint32_t wn = slot == 3 ? 1432u : slot == 2 ? 249u : 294u, wl = slot == 0 ? 35u : slot == 1 ? 23u : slot == 2 ? 17u : 26u;
  return wn * (walked < kDealClamp ? walked : kDealClamp) + wl * (len < kDealClamp ? len : kDealClamp);
}
// A tile's list length from the words in `ranges`: counted only where the words are a range this plan's tile launch writes for that
// tile - its own slot of `stride` entries, or a longer list in the tail pool; (0, 0) after a tile that could not place its list.
// Anything else (a workspace no forward has run in yet holds whatever the allocator left) lists nothing, and an XCD of such
// words keeps the shipped order (kDealMinMeanList).
__host__ __device__ __forceinline__ uint32_t deal_list_length(const uint2 r, const uint32_t tile, const uint32_t stride, const uint32_t tail_off) {
  const uint32_t n = r.y - r.x;
  const bool own = r.x == tile * stride && n <= stride, tail = r.x >= tail_off && n > stride;
  return own || tail ? n : 0u;
}
// Are a tile's two words what a forward leaves?  Its blend walks whole batches of 32 entries or its whole list, never more than
// the list and never nothing of a list that has entries.  An XCD with one tile whose words are not (a hint from elsewhere, a
// workspace no forward has run in) keeps the shipped order.
__host__ __device__ __forceinline__ bool deal_words_plausible(const uint32_t walked, const uint32_t len) {
  return walked <= len && ((walked & 31u) == 0u || walked == len) && (walked != 0u || len == 0u);
}
// What a candidate exchange leaves on the costlier of its two units: tile a (slot sa of the unit that costs cw) against tile b
// (slot sb of a unit that costs cd).
__host__ __device__ __forceinline__ uint32_t deal_exchange(const uint32_t cw, const uint32_t cd, const int sa, const uint32_t wa, const uint32_t la,
                                                           const int sb, const uint32_t wb, const uint32_t lb) {
  const uint32_t nw = cw - deal_term(sa, wa, la) + deal_term(sa, wb, lb), nd = cd - deal_term(sb, wb, lb) + deal_term(sb, wa, la);
  return nw > nd ? nw : nd;
}
// The XCD's k-th workgroup (k = workgroup >> 3) runs in slot k >> 5 on unit k & 31 (observed dispatch order; speed only).  The deal:
//   1. the shipped order - heaviest first by deal_key, every other round mirrored (deal_position); that is all for an XCD
//      of short lists (kDealMinMeanList);
//   2. up to kDealPasses times: the costliest unit (lowest index on a tie) gives one of its tiles for a tile of another unit - the
//      exchange that leaves the smaller cost on the costlier of the two units, if that is below what the unit costs now (ties: the
//      lowest lane, its first tile before its second, the lowest slot of the costly unit); no such exchange: done.
// A permutation of the XCD's tiles whatever the words hold: step 1 is one (deal_key's low bits), step 2 only exchanges.
// The slot order inside a unit is part of step 2's moves only through exchanges with other units; on the measured deals 8, 32 and
// 400 passes ended alike (K2 23.3 - 23.5 us against the shipped order's 23.5 - 24.2), so a search over the 24 orders is not made.
// Host statement (serial), the reference of the tests: out[k] = index inside the XCD of the tile of its k-th workgroup.
static inline void tile_deal_order_host(const uint32_t* walked, const uint32_t* len, const int cnt, uint32_t* out) {
  auto key = [&](int i) { return (((walked[i] < 0xfffffeu ? walked[i] : 0xfffffeu) + 1u) << 8) | (uint32_t)(255 - i); };
  auto pos = [&](int k) { const int r = k >> 5, in = k & 31, ln = cnt - (r << 5) < 32 ? cnt - (r << 5) : 32; return (r << 5) + ((r & 1) ? ln - 1 - in : in); };
  for (int i = 0; i < cnt; ++i) {
    int rank = 0;
    for (int j = 0; j < cnt; ++j) rank += key(j) > key(i) ? 1 : 0;
    out[pos(rank)] = (uint32_t)i;  // (deal_position is its own inverse)
  }
  if (cnt > kDealMaxTiles) return;
  uint32_t listed = 0;
  bool plausible = true;
  for (int i = 0; i < cnt; ++i) {
    listed += len[i] < kDealClamp ? len[i] : kDealClamp;
    plausible = plausible && deal_words_plausible(walked[i], len[i]);
  }
  if (!plausible || listed < kDealMinMeanList * (uint32_t)cnt) return;  // (outside the measured range: the shipped order)
  for (int pass = 0; pass < kDealPasses; ++pass) {
    uint32_t cost[32] = {};
    for (int k = 0; k < cnt; ++k) cost[k & 31] += deal_term(k >> 5, walked[out[k]], len[out[k]]);
    int worst = 0;
    for (int c = 1; c < 32; ++c) worst = cost[c] > cost[worst] ? c : worst;
    uint32_t best = cost[worst];
    int bk = -1, bka = -1;
    for (int lane = 0; lane < 64; ++lane)
      for (int sel = 0; sel < 2; ++sel) {
        const int k = lane + 64 * sel;
        if (k >= cnt || (k & 31) == worst) continue;
        for (int sa = 0; sa < 4; ++sa) {
          const int ka = 32 * sa + worst;
          if (ka >= cnt) continue;
          const uint32_t m = deal_exchange(cost[worst], cost[k & 31], sa, walked[out[ka]], len[out[ka]], k >> 5, walked[out[k]], len[out[k]]);
          if (m < best) { best = m; bk = k; bka = ka; }
        }
      }
    if (bk < 0) break;
    const uint32_t t = out[bk];
    out[bk] = out[bka];
    out[bka] = t;
  }
}
// K1's side, ONE wave per XCD (no LDS, no barrier: everything passes between lanes - DPP maxima, lane reads by scalar index, one
// LDS permute per pass): lane l holds the tiles of workgroups l and l + 64 of the XCD - slots (l >> 5) and 2 + (l >> 5) of unit
// l & 31.  A lone wave issues an instruction every 5 - 7 cycles: ranking 128 keys and finding each workgroup's tile are ~1 700
// instructions, a pass ~200.  Stamped on the 300 k view: the deal workgroups end 14.9 - 15.4 us after the launch's first workgroup
// starts, the colour waves 25.6 us (a first form - 16 passes, every reduction and broadcast an LDS permute - ended at 23.1 - 24.7
// us and made the forward 0.6 us SLOWER than the shipped order).  kDealPasses = 8: on the CPU replay of the headline's counts the
// first 8 exchanges per XCD bring the modelled slowest unit from 23.37 to 22.93 us, 32 to 22.68 (the search ends by itself after
// ~36), and imposed on the device through the hint 8, 32 and all of them measured alike.
__device__ __forceinline__ void build_tile_order_model(const Params& p, const int xcd, const int lane) {
  static_assert(4 * kCUs / 8 <= kDealMaxTiles, "fwd_deal_active's calls fit the model's 128 tiles per XCD");
  const int T = p.g.T, cnt = (T >> 3) + (xcd < (T & 7) ? 1 : 0), base = xcd_remap(xcd, T);  // this XCD's tiles: [base, base + cnt)
  if (cnt > kDealMaxTiles) return;
  const uint32_t* tot = p.tile_total + base;
  const uint2* rng = p.ranges + base;
  // 1. the shipped order: rank of my two keys among all, then the tile whose rank my workgroups take
  uint32_t key[2];
  int rank[2] = {0, 0}, tile[2] = {0, 0};
#pragma unroll
  for (int q = 0; q < 2; ++q) key[q] = lane + 64 * q < cnt ? deal_key(tot[lane + 64 * q], lane + 64 * q) : 0u;  // (0: below every key)
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    if (64 * q >= cnt) break;
#pragma unroll 8
    for (int j = 0; j < 64; ++j) {
      const uint32_t kj = (uint32_t)__builtin_amdgcn_readlane((int)key[q], j);
      rank[0] += kj > key[0] ? 1 : 0;
      rank[1] += kj > key[1] ? 1 : 0;
    }
  }
  const bool valid[2] = {lane < cnt, lane + 64 < cnt};
  const int want[2] = {valid[0] ? deal_position(lane, cnt) : -1, valid[1] ? deal_position(lane + 64, cnt) : -1};
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    if (64 * q >= cnt) break;
#pragma unroll 8
    for (int j = 0; j < 64; ++j) {
      const int rj = j + 64 * q < cnt ? __builtin_amdgcn_readlane(rank[q], j) : -2;
      tile[0] = rj == want[0] ? j + 64 * q : tile[0];
      tile[1] = rj == want[1] ? j + 64 * q : tile[1];
    }
  }
  uint32_t wk[2], ln[2];
  bool plausible = true;
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    const uint2 r = valid[q] ? rng[tile[q]] : make_uint2(0u, 0u);
    const uint32_t w_raw = valid[q] ? tot[tile[q]] : 0u, l_raw = deal_list_length(r, (uint32_t)(base + tile[q]), p.stride, p.tail_off);
    plausible = plausible && deal_words_plausible(w_raw, l_raw);
    wk[q] = min(w_raw, kDealClamp);
    ln[q] = min(l_raw, kDealClamp);
  }
  // 2. the exchanges (inside the measured range only: kDealMinMeanList)
  const int cu = lane & 31, slot[2] = {lane >> 5, 2 + (lane >> 5)};
  const uint32_t listed = (uint32_t)__builtin_amdgcn_readlane((int)wave_inclusive_scan_u32(ln[0] + ln[1]), 63);
  const bool search = __ballot(!plausible) == 0ull && listed >= kDealMinMeanList * (uint32_t)cnt;  // (wave-uniform)
  for (int pass = 0; pass < (search ? kDealPasses : 0); ++pass) {
    const uint32_t mine = (valid[0] ? deal_term(slot[0], wk[0], ln[0]) : 0u) + (valid[1] ? deal_term(slot[1], wk[1], ln[1]) : 0u);
    const uint32_t cost = mine + (uint32_t)__shfl_xor((int)mine, 32);  // my unit's
    const uint32_t top = wave_max_u32((cost << 5) | (uint32_t)(31 - cu));  // (wave-uniform from here: lanes are read by scalar index)
    const int worst = 31 - (int)(top & 31u);
    const uint32_t cw = top >> 5;
    uint32_t best = cw;
    int pick = -1;
    uint32_t wa[4], la[4];
#pragma unroll
    for (int sa = 0; sa < 4; ++sa) {  // the costly unit's four tiles
      wa[sa] = (uint32_t)__builtin_amdgcn_readlane((int)wk[sa >> 1], (sa & 1) * 32 + worst);
      la[sa] = (uint32_t)__builtin_amdgcn_readlane((int)ln[sa >> 1], (sa & 1) * 32 + worst);
    }
#pragma unroll
    for (int sel = 0; sel < 2; ++sel) {
#pragma unroll
      for (int sa = 0; sa < 4; ++sa) {
        const uint32_t m = deal_exchange(cw, cost, sa, wa[sa], la[sa], slot[sel], wk[sel], ln[sel]);
        const bool ok = valid[sel] && cu != worst && 32 * sa + worst < cnt && m < best;
        best = ok ? m : best;
        pick = ok ? sel * 4 + sa : pick;
      }
    }
    const uint32_t low = ~wave_max_u32(~best);
    const unsigned long long who = __ballot(pick >= 0 && best == low);
    if (who == 0ull) break;  // (wave-uniform) nothing helps the costliest unit
    const int from = __builtin_ctzll(who), choice = __builtin_amdgcn_readlane(pick, from), sel = choice >> 2, sa = choice & 3;
    const int to = (sa & 1) * 32 + worst;  // the lane that holds the costly unit's tile, in its register sa >> 1
    const int tb = __builtin_amdgcn_readlane(sel ? tile[1] : tile[0], from), ta = __builtin_amdgcn_readlane(sa >> 1 ? tile[1] : tile[0], to);
    const uint32_t wb = (uint32_t)__builtin_amdgcn_readlane((int)(sel ? wk[1] : wk[0]), from);
    const uint32_t lb = (uint32_t)__builtin_amdgcn_readlane((int)(sel ? ln[1] : ln[0]), from);
    const uint32_t was = sa == 0 ? wa[0] : sa == 1 ? wa[1] : sa == 2 ? wa[2] : wa[3], las = sa == 0 ? la[0] : sa == 1 ? la[1] : sa == 2 ? la[2] : la[3];
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const bool takes_a = lane == from && sel == q, takes_b = lane == to && (sa >> 1) == q;
      tile[q] = takes_a ? ta : takes_b ? tb : tile[q];
      wk[q] = takes_a ? was : takes_b ? wb : wk[q];
      ln[q] = takes_a ? las : takes_b ? lb : ln[q];
    }
  }
#pragma unroll
  for (int q = 0; q < 2; ++q)
    if (valid[q]) tile_order_of(p)[((lane + 64 * q) << 3) | xcd] = (uint32_t)(base + tile[q]);
}
// Who builds it: kDealBlocks workgroups of the fused binning launch BEHIND its `rows` binning workgroups, one per XCD's table (the
// tile launch runs after that kernel, the previous call's tile launch - which left the counts - before it).  They are workgroups of
// their own because the launch has compute units to spare for them - 247 binning workgroups on 256 CUs in the 300 k view - and
// none of its own waves has: built by the binning waves of rows 0 ... 7 in their tail, under the harmonics stream, the same table
// made the launch 1.0 us longer (23.9 -> 24.9 us; a trip to memory and ~400 VALU instructions per wave on SIMDs the colour waves fill).
// A single view that takes the binning launch WITHOUT colour waves (a device that does not grant it the LDS) gets the table from
// a launch of its own, k_tile_order, in front: those instances stay the code they were (the two-per-CU one spills with it).
__device__ __forceinline__ void build_tile_order(const Params& p, const int xcd, const int w, const int lane) {
  if (w == 0) build_tile_order_model(p, xcd, lane);
}
__global__ __launch_bounds__(256) void k_tile_order(const Params p) {
  build_tile_order(p, (int)blockIdx.x, (int)(threadIdx.x >> 6), (int)(threadIdx.x & 63));
}
// K2's side: the (view, tile) of workgroup `bid` of a gathering tile launch, in two steps so that a kernel can ask for the word at
// its start and look at it where it first needs the tile.  The dealt tile is read from the table - never from tile_total itself,
// which tiles of the same launch overwrite - and is clamped: whatever the word holds, the tile exists.  A VECTOR load (the
// relaxed atomic keeps it one): the scalar loads of a wave return in any order, so the next wait for one of them - the status
// word thread 0 asks for - would wait for this word too, one round trip behind the other.
__device__ __forceinline__ uint32_t fwd_tile_word(const Params& p, const uint32_t bid) {
  if (!fwd_deal_active(p)) return (uint32_t)xcd_remap((int)bid, (int)p.sort_blocks);
  return __hip_atomic_load(tile_order_of(p) + bid, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ int fwd_tile_of(const Params& p, const uint32_t word) {
  return (int)min((uint32_t)__builtin_amdgcn_readfirstlane((int)word), p.sort_blocks - 1u);
}

// Real-SH polynomial basis and its x/y/z partials, visited in coefficient order with compile-time k.
// Same expression trees as oracle/gsr_oracle.hpp sh_basis / sh_basis_grad ([EXT] forward.cu
// computeColorFromSH, backward.cu computeColorFromSH; band 4 per SURVEY.md Appendix A.1).
template <class F>
__device__ __forceinline__ void sh_visit(int deg, float x, float y, float z, F&& f) {
  constexpr float C0 = 0.28209479177387814f, C1 = 0.4886025119029199f;
  constexpr float C20 = 1.0925484305920792f, C21 = -1.0925484305920792f, C22 = 0.31539156525252005f,
                  C23 = -1.0925484305920792f, C24 = 0.5462742152960396f;
  constexpr float C30 = -0.5900435899266435f, C31 = 2.890611442640554f, C32 = -0.4570457994644658f,
                  C33 = 0.3731763325901154f, C34 = -0.4570457994644658f, C35 = 1.445305721320277f,
                  C36 = -0.5900435899266435f;
  constexpr float C40 = 2.5033429417967046f, C41 = -1.7701307697799304f, C42 = 0.9461746957575601f,
                  C43 = -0.6690465435572892f, C44 = 0.10578554691520431f, C45 = -0.6690465435572892f,
                  C46 = 0.47308734787878004f, C47 = -1.7701307697799304f, C48 = 0.6258357354491761f;
  f(0, C0, 0.f, 0.f, 0.f);
  if (deg > 0) {
    f(1, -C1 * y, 0.f, -C1, 0.f);
    f(2, C1 * z, 0.f, 0.f, C1);
    f(3, -C1 * x, -C1, 0.f, 0.f);
    if (deg > 1) {
      const float xx = x * x, yy = y * y, zz = z * z, xy = x * y, yz = y * z, xz = x * z;
      f(4, C20 * xy, C20 * y, C20 * x, 0.f);
      f(5, C21 * yz, 0.f, C21 * z, C21 * y);
      f(6, C22 * (2.f * zz - xx - yy), C22 * -2.f * x, C22 * -2.f * y, C22 * 4.f * z);
      f(7, C23 * xz, C23 * z, 0.f, C23 * x);
      f(8, C24 * (xx - yy), C24 * 2.f * x, C24 * -2.f * y, 0.f);
      if (deg > 2) {
        f(9, C30 * y * (3.f * xx - yy), C30 * 6.f * xy, C30 * (3.f * xx - 3.f * yy), 0.f);
        f(10, C31 * xy * z, C31 * yz, C31 * xz, C31 * xy);
        f(11, C32 * y * (4.f * zz - xx - yy), C32 * -2.f * xy, C32 * (4.f * zz - xx - 3.f * yy), C32 * 8.f * yz);
        f(12, C33 * z * (2.f * zz - 3.f * xx - 3.f * yy), C33 * -6.f * xz, C33 * -6.f * yz,
          C33 * (6.f * zz - 3.f * xx - 3.f * yy));
        f(13, C34 * x * (4.f * zz - xx - yy), C34 * (4.f * zz - 3.f * xx - yy), C34 * -2.f * xy, C34 * 8.f * xz);
        f(14, C35 * z * (xx - yy), C35 * 2.f * xz, C35 * -2.f * yz, C35 * (xx - yy));
        f(15, C36 * x * (xx - 3.f * yy), C36 * (3.f * xx - 3.f * yy), C36 * -6.f * xy, 0.f);
        if (deg > 3) {
          f(16, C40 * xy * (xx - yy), C40 * (3.f * xx * y - yy * y), C40 * (xx * x - 3.f * x * yy), 0.f);
          f(17, C41 * yz * (3.f * xx - yy), C41 * 6.f * xy * z, C41 * z * (3.f * xx - 3.f * yy), C41 * y * (3.f * xx - yy));
          f(18, C42 * xy * (7.f * zz - 1.f), C42 * y * (7.f * zz - 1.f), C42 * x * (7.f * zz - 1.f), C42 * 14.f * xy * z);
          f(19, C43 * yz * (7.f * zz - 3.f), 0.f, C43 * z * (7.f * zz - 3.f), C43 * y * (21.f * zz - 3.f));
          f(20, C44 * (zz * (35.f * zz - 30.f) + 3.f), 0.f, 0.f, C44 * (140.f * zz * z - 60.f * z));
          f(21, C45 * xz * (7.f * zz - 3.f), C45 * z * (7.f * zz - 3.f), 0.f, C45 * x * (21.f * zz - 3.f));
          f(22, C46 * (xx - yy) * (7.f * zz - 1.f), C46 * 2.f * x * (7.f * zz - 1.f), C46 * -2.f * y * (7.f * zz - 1.f),
            C46 * 14.f * z * (xx - yy));
          f(23, C47 * xz * (xx - 3.f * yy), C47 * z * (3.f * xx - 3.f * yy), C47 * -6.f * xy * z, C47 * x * (xx - 3.f * yy));
          f(24, C48 * (xx * (xx - 3.f * yy) - yy * (3.f * xx - yy)), C48 * (4.f * xx * x - 12.f * x * yy),
            C48 * (4.f * yy * y - 12.f * xx * y), 0.f);
        }
      }
    }
  }
}

// Input layouts (GsrDims.flags): covariances as 6 floats xx,xy,xz,yy,yz,zz (the rasterizer's cov3D_precomp) or, with
// GSR_FLAG_COV_3X3, as the full symmetric 3x3 PF3plat carries (only its upper triangle is read, and only the upper
// triangle receives gradient - exactly what the reference's fancy-index gather does, cuda_splatting.py:115,123);
// SH as (N, M, 3) (the rasterizer's shs) or, with GSR_FLAG_SH_PLANAR, as PF3plat's harmonics (N, 3, M).
__device__ __forceinline__ void load_cov6(const float* cov, size_t gi, bool c9, float* o) {
  if (c9) {
    const float* c = cov + 9 * gi;
    o[0] = c[0]; o[1] = c[1]; o[2] = c[2]; o[3] = c[4]; o[4] = c[5]; o[5] = c[8];
  } else {
    const float* c = cov + 6 * gi;
#pragma unroll
    for (int k = 0; k < 6; ++k) o[k] = c[k];
  }
}

// Scale / rotation input form: what PF3plat's GaussianAdapter does between its raw network outputs and the covariance it
// hands to the decoder (reference src/model/encoder/common/gaussians.py:8-44 quaternion_to_matrix + build_covariance,
// gaussian_adapter.py:79-83 rotation into world space), evaluated on load instead of materialising (N, 3, 3) matrices:
//   record = scale (x, y, z), quaternion (x, y, z, w);   two_s = 2 / (|q|^2 + 1e-8);   Rq from the quaternion;
//   M = F Rq  (F: camera-to-world rotation of the Gaussian's source view, optional);   Sigma = M diag(s^2) M^T.
__device__ __forceinline__ void sr_matrix(const float* sr, const float* F, float* M, float& ts) {
  const float i = sr[3], j = sr[4], k = sr[5], r = sr[6];
  ts = 2.f / (i * i + j * j + k * k + r * r + 1e-8f);
  const float Rq[9] = {1.f - ts * (j * j + k * k), ts * (i * j - k * r), ts * (i * k + j * r),
                       ts * (i * j + k * r), 1.f - ts * (i * i + k * k), ts * (j * k - i * r),
                       ts * (i * k - j * r), ts * (j * k + i * r), 1.f - ts * (i * i + j * j)};
  if (F) {
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
      for (int b = 0; b < 3; ++b) M[3 * a + b] = F[3 * a] * Rq[b] + F[3 * a + 1] * Rq[3 + b] + F[3 * a + 2] * Rq[6 + b];
  } else {
#pragma unroll
    for (int a = 0; a < 9; ++a) M[a] = Rq[a];
  }
}
__device__ __forceinline__ void cov6_from_sr(const float* sr, const float* F, float* o) {
  float M[9], ts;
  sr_matrix(sr, F, M, ts);
  const float s0 = sr[0] * sr[0], s1 = sr[1] * sr[1], s2 = sr[2] * sr[2];
  auto S = [&](int a, int b) { return M[3 * a] * s0 * M[3 * b] + M[3 * a + 1] * s1 * M[3 * b + 1] + M[3 * a + 2] * s2 * M[3 * b + 2]; };
  o[0] = S(0, 0); o[1] = S(0, 1); o[2] = S(0, 2); o[3] = S(1, 1); o[4] = S(1, 2); o[5] = S(2, 2);
}
// dL/d(record) from dL/dcov6 (doubled off-diagonals, as the raster backward produces them)
__device__ __forceinline__ void sr_backward(const float* sr, const float* F, const float* dc, float* dsr) {
  float M[9], ts;
  sr_matrix(sr, F, M, ts);
  const float G[9] = {dc[0], 0.5f * dc[1], 0.5f * dc[2], 0.5f * dc[1], dc[3], 0.5f * dc[4], 0.5f * dc[2], 0.5f * dc[4], dc[5]};
  float dM[9];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float m[3] = {M[k], M[3 + k], M[6 + k]};  // column k of M
    float Gm[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) Gm[a] = G[3 * a] * m[0] + G[3 * a + 1] * m[1] + G[3 * a + 2] * m[2];
    dsr[k] = 2.f * sr[k] * (m[0] * Gm[0] + m[1] * Gm[1] + m[2] * Gm[2]);
    const float s2 = 2.f * sr[k] * sr[k];
#pragma unroll
    for (int a = 0; a < 3; ++a) dM[3 * a + k] = s2 * Gm[a];
  }
  float D[9];  // dL/dRq = F^T dL/dM
  if (F) {
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
      for (int b = 0; b < 3; ++b) D[3 * a + b] = F[a] * dM[b] + F[3 + a] * dM[3 + b] + F[6 + a] * dM[6 + b];
  } else {
#pragma unroll
    for (int a = 0; a < 9; ++a) D[a] = dM[a];
  }
  const float i = sr[3], j = sr[4], k = sr[5], r = sr[6];
  // Rq = I + two_s P(q):  dL/dq = two_s sum D : dP/dq  -  two_s^2 q sum D : P
  const float DP = D[0] * -(j * j + k * k) + D[1] * (i * j - k * r) + D[2] * (i * k + j * r) + D[3] * (i * j + k * r) +
                   D[4] * -(i * i + k * k) + D[5] * (j * k - i * r) + D[6] * (i * k - j * r) + D[7] * (j * k + i * r) +
                   D[8] * -(i * i + j * j);
  const float di = D[1] * j + D[2] * k + D[3] * j - 2.f * i * D[4] - r * D[5] + k * D[6] + r * D[7] - 2.f * i * D[8];
  const float dj = -2.f * j * D[0] + i * D[1] + r * D[2] + i * D[3] + k * D[5] - r * D[6] + k * D[7] - 2.f * j * D[8];
  const float dk = -2.f * k * D[0] - r * D[1] + i * D[2] + r * D[3] - 2.f * k * D[4] + j * D[5] + i * D[6] + j * D[7];
  const float dr = -k * D[1] + j * D[2] + k * D[3] - i * D[5] - j * D[6] + i * D[7];
  const float c = ts * ts * DP;
  dsr[3] = ts * di - c * i; dsr[4] = ts * dj - c * j; dsr[5] = ts * dk - c * k; dsr[6] = ts * dr - c * r;
}
// The covariance of Gaussian i of `set` in whichever input form the call uses
__device__ __forceinline__ void load_covariance(const Params& p, int set, int i, size_t gi, float* o) {
  if (p.scale_rot) {
    const int N = p.d.num_gaussians;
    const float* F = p.frames ? p.frames + ((size_t)set * p.num_frames + (size_t)i / (size_t)(N / p.num_frames)) * 9 : nullptr;
    cov6_from_sr(p.cov6 + 7 * gi, F, o);
  } else {
    load_cov6(p.cov6, gi, (p.d.flags & GSR_FLAG_COV_3X3) != 0, o);
  }
}

// GSR_FLAG_SH_IN_FRAME: the harmonics of Gaussian i of `set` are in the coordinates of G = F = frames[set, i / (N / F)], or, with
// GSR_FLAG_SH_FRAME_E3NN, of G = M F M^T (M = Z P, P: (x, y, z) -> (z, x, y), Z = diag(-1, -1, 1)).  Evaluating them at the
// view direction d' = G^T d is the same as evaluating rotate_sh(harmonics, F, basis) at d.  T receives G^T row by row (T[3k + j]
// = G[j][k]); the direction gradient goes back to world coordinates as dd = T^T dd'.  M is a signed permutation, so the e3nn
// form is a re-indexing with signs: G[j][k] = s_j s_k F[pi_j][pi_k], pi = (2, 0, 1), s = (-1, -1, 1).  The lanes of a unit read
// the same 36 bytes unless a group boundary falls inside the unit (one cache line per load instruction either way).
__device__ __forceinline__ void load_dir_frame(const Params& p, int set, int i, float (&T)[9]) {
  const int N = p.d.num_gaussians;
  const int f = min(i, N - 1) / (N / p.num_frames);
  const float* F = p.frames + ((size_t)set * p.num_frames + f) * 9;
  float R[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) R[k] = F[k];
  if (p.d.flags & GSR_FLAG_SH_FRAME_E3NN) {
    const int pi[3] = {2, 0, 1};
    const float s[3] = {-1.f, -1.f, 1.f};
#pragma unroll
    for (int j = 0; j < 3; ++j)
#pragma unroll
      for (int k = 0; k < 3; ++k) T[3 * k + j] = s[j] * s[k] * R[3 * pi[j] + pi[k]];
  } else {
#pragma unroll
    for (int j = 0; j < 3; ++j)
#pragma unroll
      for (int k = 0; k < 3; ++k) T[3 * k + j] = R[3 * j + k];
  }
}
// d' = T d (the direction in the harmonics' frame); in place
__device__ __forceinline__ void dir_to_frame(const float (&T)[9], float& x, float& y, float& z) {
  const float a = T[0] * x + T[1] * y + T[2] * z, b = T[3] * x + T[4] * y + T[5] * z, c = T[6] * x + T[7] * y + T[8] * z;
  x = a; y = b; z = c;
}
// dd = T^T dd' (a gradient w.r.t. the frame's direction back to world coordinates); in place
__device__ __forceinline__ void grad_to_world(const float (&T)[9], float& x, float& y, float& z) {
  const float a = T[0] * x + T[3] * y + T[6] * z, b = T[1] * x + T[4] * y + T[7] * z, c = T[2] * x + T[5] * y + T[8] * z;
  x = a; y = b; z = c;
}

// Built-in extra channel (GsrDims.flags bits 4-6, GSR_EXTRA_*): the scalar the reference's depth render blends
// (cuda_splatting.py:238-251) - camera-space z in UN-normalised units (z_scaled / scale), mapped by the mode - and its
// derivative w.r.t. z for the backward chain.  near/far are the caller's un-normalised values (GsrView.near/far).
__device__ __forceinline__ float extra_from_depth(int mode, float z, float nr, float fr, float& dfdz) {
  const float eps = 1e-10f;
  if (mode == GSR_EXTRA_DEPTH) { dfdz = 1.f; return z; }
  if (mode == GSR_EXTRA_DISPARITY) { const float r = 1.f / z; dfdz = -r * r; return r; }
  if (mode == GSR_EXTRA_RELATIVE_DISPARITY) {  // depth_to_relative_disparity, conversions.py:17-27
    const float dn = 1.f / (nr + eps), df = 1.f / (fr + eps), d = 1.f / (z + eps);
    const float k = 1.f / (dn - df + eps);
    dfdz = d * d * k;
    return 1.f - (d - df) * k;
  }
  dfdz = 0.f;  // GSR_EXTRA_LOG: the reference's min(near).max(far).log() is the constant log(far) (cuda_splatting.py:251)
  return logf(fmaxf(fminf(z, nr), fr));
}

// EWA projection pieces shared by forward and backward ([EXT] forward.cu computeCov2D);
// same expression trees as oracle cov2d_parts.
struct Cov2D {
  float t0, t1, t2;
  float M[6];
  float a, b, c;
  float fx, fy;
  bool xcl, ycl;
};

__device__ __forceinline__ void cov2d_parts(const float mx, const float my, const float mz, const float* cov6,
                                            const GsrView& cam, int W, int H, Cov2D& o) {
  const float* v = cam.viewmatrix;
  float t0 = v[0] * mx + v[4] * my + v[8] * mz + v[12];
  float t1 = v[1] * mx + v[5] * my + v[9] * mz + v[13];
  const float t2 = v[2] * mx + v[6] * my + v[10] * mz + v[14];
  const float limx = 1.3f * cam.tanfovx, limy = 1.3f * cam.tanfovy;
  const float txtz = t0 / t2, tytz = t1 / t2;
  o.xcl = (txtz < -limx) || (txtz > limx);
  o.ycl = (tytz < -limy) || (tytz > limy);
  t0 = fminf(limx, fmaxf(-limx, txtz)) * t2;
  t1 = fminf(limy, fmaxf(-limy, tytz)) * t2;
  o.t0 = t0; o.t1 = t1; o.t2 = t2;
  o.fx = (float)W / (2.f * cam.tanfovx);
  o.fy = (float)H / (2.f * cam.tanfovy);
  const float J00 = o.fx / t2, J02 = -(o.fx * t0) / (t2 * t2);
  const float J11 = o.fy / t2, J12 = -(o.fy * t1) / (t2 * t2);
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    o.M[j] = J00 * v[4 * j + 0] + J02 * v[4 * j + 2];
    o.M[3 + j] = J11 * v[4 * j + 1] + J12 * v[4 * j + 2];
  }
  const float S[9] = {cov6[0], cov6[1], cov6[2], cov6[1], cov6[3], cov6[4], cov6[2], cov6[4], cov6[5]};
  float MS[6];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j)
      MS[3 * i + j] = o.M[3 * i + 0] * S[0 * 3 + j] + o.M[3 * i + 1] * S[1 * 3 + j] + o.M[3 * i + 2] * S[2 * 3 + j];
  o.a = MS[0] * o.M[0] + MS[1] * o.M[1] + MS[2] * o.M[2] + 0.3f;
  o.b = MS[0] * o.M[3] + MS[1] * o.M[4] + MS[2] * o.M[5];
  o.c = MS[3] * o.M[3] + MS[4] * o.M[4] + MS[5] * o.M[5] + 0.3f;
}

// Footprint of one projected Gaussian over the 8x8-tile grid.  The candidate range is the reference's
// 16x16-tile rect ([EXT] auxiliary.h getRect) expressed in 8x8 tiles, clipped to the image and to the
// axis-aligned bounds of the ellipse {q <= tau}, q = a dx^2 + 2 b dx dy + c dy^2, tau = 2 ln(255 o):
// outside it alpha = o exp(-q/2) < 1/255 and the blend would skip the pixel anyway.
struct Foot {
  float cx, cy, A, B, C, tau, nBiC, nBiA;  // nBiC = -B/C, nBiA = -B/A
  float detc, hx, hy;                          // conic determinant, half extents of the ellipse {q <= tau}
  bool convex;
  int sx0, sx1, sy0, sy1;
};

__device__ __forceinline__ int f2i_clamped(float f) { return (int)fminf(1e9f, fmaxf(-1e9f, f)); }

__device__ __forceinline__ void ref_rect16(float x, float y, float r, const Grid& g, int& rx0, int& ry0, int& rx1, int& ry1) {
  rx0 = min(g.gx16, max(0, f2i_clamped((x - r) / 16.f)));
  ry0 = min(g.gy16, max(0, f2i_clamped((y - r) / 16.f)));
  rx1 = min(g.gx16, max(0, f2i_clamped((x + r + 15.f) / 16.f)));
  ry1 = min(g.gy16, max(0, f2i_clamped((y + r + 15.f) / 16.f)));
}

__device__ __forceinline__ Foot make_foot(float x, float y, float A, float B, float C, float o, float r, const Grid& g) {
  Foot f;
  f.cx = x; f.cy = y; f.A = A; f.B = B; f.C = C;
  // Hardware reciprocal / square root / log2 (about 1 ulp) are enough here: every test built on the footprint carries a margin
  // orders of magnitude above that, and the count and emit passes see bit-identical values either way.
  f.nBiC = -B * __builtin_amdgcn_rcpf(C); f.nBiA = -B * __builtin_amdgcn_rcpf(A);
  int rx0, ry0, rx1, ry1;
  ref_rect16(x, y, r, g, rx0, ry0, rx1, ry1);
  f.sx0 = 2 * rx0; f.sy0 = 2 * ry0;
  f.sx1 = min(2 * rx1, g.sw); f.sy1 = min(2 * ry1, g.sh);
  const float tau = (2.f * 0.6931471805599453f) * __builtin_amdgcn_logf(255.f * o);  // 2 ln(255 o)
  f.tau = tau + 1e-4f * fabsf(tau) + 0.02f;  // margin >> fp32 error of the blend's own power evaluation
  const float detc = A * C - B * B;
  f.convex = (A > 0.f) && (C > 0.f) && (detc > 0.f) && (detc < 3.0e38f);
  f.detc = detc; f.hx = 0.f; f.hy = 0.f;
  if (!(f.tau >= 0.f)) {  // opacity < 1/255 (or NaN): alpha < 1/255 everywhere
    f.sx1 = f.sx0; f.sy1 = f.sy0;
  } else if (f.convex) {
    f.detc = detc;
    const float rdet = __builtin_amdgcn_rcpf(detc);
    f.hx = __builtin_amdgcn_sqrtf(f.tau * C * rdet); f.hy = __builtin_amdgcn_sqrtf(f.tau * A * rdet);
    const float hx = f.hx + 0.5f, hy = f.hy + 0.5f;
    f.sx0 = max(f.sx0, f2i_clamped(floorf((x - hx) * 0.125f)));
    f.sx1 = min(f.sx1, f2i_clamped(floorf((x + hx) * 0.125f)) + 1);
    f.sy0 = max(f.sy0, f2i_clamped(floorf((y - hy) * 0.125f)));
    f.sy1 = min(f.sy1, f2i_clamped(floorf((y + hy) * 0.125f)) + 1);
  }
  return f;
}

// Exact minimum of q over the pixel-centre box of 8x8 tile (sx, sy); true if some pixel may reach alpha >= 1/255.
__device__ __forceinline__ bool subtile_hit(const Foot& f, int sx, int sy, const Grid& g) {
  if (!f.convex) return true;
  const float dx0 = (float)(8 * sx) - f.cx, dx1 = (float)min(8 * sx + 7, g.W - 1) - f.cx;
  const float dy0 = (float)(8 * sy) - f.cy, dy1 = (float)min(8 * sy + 7, g.H - 1) - f.cy;
  const bool inx = (dx0 <= 0.f) && (dx1 >= 0.f), iny = (dy0 <= 0.f) && (dy1 >= 0.f);
  if (inx && iny) return true;
  auto qx = [&](float dxe) {
    const float ys = fminf(fmaxf(f.nBiC * dxe, dy0), dy1);
    return f.A * dxe * dxe + 2.f * f.B * dxe * ys + f.C * ys * ys;
  };
  auto qy = [&](float dye) {
    const float xs = fminf(fmaxf(f.nBiA * dye, dx0), dx1);
    return f.A * xs * xs + 2.f * f.B * xs * dye + f.C * dye * dye;
  };
  const float qmin = fminf(fminf(qx(dx0), qx(dx1)), fminf(qy(dy0), qy(dy1)));
  return qmin <= f.tau;
}

// All hit tiles of one row of 8x8 tiles at once: the ellipse {q <= tau} cut by the row's band of pixel centres is convex,
// so its x-projection is an interval [xl, xr]; xr(y) = (-B y + sqrt(A tau - det y^2)) / A is concave with its maximum at the
// ellipse's rightmost point y_r = -B hx / C, hence the band maximum sits at y_r clamped into the band (xl symmetrically).
// Returns the bits (relative to f.sx0) of the tiles whose pixel-centre span meets that interval - the same set the
// per-tile box minimum (subtile_hit) accepts, at the cost of two square roots per row instead of ~50 ops per tile.
__device__ __forceinline__ uint32_t row_hit_bits(const Foot& f, int sy, const Grid& g) {
  const int w = f.sx1 - f.sx0;
  const uint32_t all = w >= 32 ? 0xffffffffu : ((1u << w) - 1u);
  if (!f.convex) return all;
  const float ya = fmaxf((float)(8 * sy) - f.cy, -f.hy), yb = fminf((float)min(8 * sy + 7, g.H - 1) - f.cy, f.hy);
  if (ya > yb) return 0u;
  const float yrt = f.nBiC * f.hx;  // y of the rightmost point; the leftmost is at -yrt
  const float yr = fminf(fmaxf(yrt, ya), yb), yl = fminf(fmaxf(-yrt, ya), yb);
  const float inva = __builtin_amdgcn_rcpf(f.A), at = f.A * f.tau;
  const float xr = (-f.B * yr + __builtin_amdgcn_sqrtf(fmaxf(0.f, at - f.detc * yr * yr))) * inva + 1e-3f;
  const float xl = (-f.B * yl - __builtin_amdgcn_sqrtf(fmaxf(0.f, at - f.detc * yl * yl))) * inva - 1e-3f;
  const int lo = max(f.sx0, f2i_clamped(ceilf((xl + f.cx - 7.f) * 0.125f)));
  const int hi = min(f.sx1 - 1, f2i_clamped(floorf((xr + f.cx) * 0.125f)));
  if (hi < lo) return 0u;
  const int n = hi - lo + 1;
  return (n >= 32 ? 0xffffffffu : ((1u << n) - 1u)) << (lo - f.sx0);
}

// Walks of a footprint wider than the mask window: by one lane, or by all 64 lanes of a wave (wave-uniform foot).
template <class F>
__device__ __forceinline__ void big_walk_lane(const Foot& ft, const Grid& g, F&& f) {
  for (int sy = ft.sy0; sy < ft.sy1; ++sy)
    for (int sx = ft.sx0; sx < ft.sx1; ++sx)
      if (subtile_hit(ft, sx, sy, g)) f(sy * g.sgx + sx);
}
template <class F>
__device__ __forceinline__ void big_walk_wave(const Foot& ft, const Grid& g, int lane, F&& f) {
  const int w = ft.sx1 - ft.sx0, cnt = w * (ft.sy1 - ft.sy0);
  for (int c = lane; c < cnt; c += 64) {
    const int dy = c / w, sx = ft.sx0 + (c - dy * w), sy = ft.sy0 + dy;
    if (subtile_hit(ft, sx, sy, g)) f(sy * g.sgx + sx);
  }
}
constexpr int kBigList = 256;  // deferred wide footprints per binning workgroup (more are walked in line)

__device__ __forceinline__ Foot foot_of_record(const GeomRec* rec, const Grid& g) {
  const float4 q0 = rec->q0, q1 = rec->q1;
  return make_foot(q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, (float)(__float_as_uint(q1.w) & 0x0fffffffu), g);
}
// Walks the (tile) pairs of one Gaussian from its record's q3 word (hit mask, origin, depth).
template <class F, class B>
__device__ __forceinline__ void walk_pairs(const Params& p, const float4 q3, int i, int t0, int t1, F&& f, B&& big) {
  const Grid& g = p.g;
  const uint32_t origin = __float_as_uint(q3.z);
  unsigned long long m = ((unsigned long long)__float_as_uint(q3.y) << 32) | __float_as_uint(q3.x);
  const int sx0 = (int)(origin & 0xfffu), sy0 = (int)((origin >> 12) & 0xfffu);
  while (m) {
    const int b = __ffsll((long long)m) - 1;
    m &= m - 1;
    const int t = (sy0 + (b >> 3)) * g.sgx + sx0 + (b & 7);
    if (t >= t0 && t < t1) f(i, t, q3.w);
  }
  if (origin & 0x80000000u) big(i);  // footprint wider than the 8x8-tile mask window
}
template <class F>
__device__ __forceinline__ void for_each_pair(const Params& p, int v, int row, int tid, int t0, int t1, F&& f) {
  const int N = p.d.num_gaussians;
  const int end = min(N, (row + 1) * p.chunk);
  for (int i = row * p.chunk + tid; i < end; i += kBinThreads) {
    const GeomRec* rec = p.geom + (size_t)v * N + i;
    const float4 q3 = p.aux[(size_t)v * N + i];
    walk_pairs(p, q3, i, t0, t1, f, [&](int) {
      const Foot ft = foot_of_record(rec, p.g);
      big_walk_lane(ft, p.g, [&](int t) { if (t >= t0 && t < t1) f(i, t, q3.w); });
    });
  }
}

// Wave-cooperative copy of `cnt` rows of `rowf` floats from global to LDS (row stride ldstride floats).
__device__ __forceinline__ void stage_rows(float* lds, const float* src, int cnt, int rowf, int ldstride, int lane) {
  const int total = cnt * rowf;
  if (ldstride == rowf) {
    if ((((uintptr_t)src) & 15) == 0) {
      const int n4 = total >> 2;
      for (int k = lane; k < n4; k += 64) reinterpret_cast<float4*>(lds)[k] = reinterpret_cast<const float4*>(src)[k];
      for (int k = (n4 << 2) + lane; k < total; k += 64) lds[k] = src[k];
    } else {
      for (int k = lane; k < total; k += 64) lds[k] = src[k];
    }
  } else {
    for (int k = lane; k < total; k += 64) {
      const int row = k / rowf;
      lds[row * ldstride + (k - row * rowf)] = src[k];
    }
  }
}
__device__ __forceinline__ void unstage_rows(float* dst, const float* lds, int cnt, int rowf, int ldstride, int lane) {
  const int total = cnt * rowf;
  if (ldstride == rowf) {
    if ((((uintptr_t)dst) & 15) == 0) {
      const int n4 = total >> 2;
      // streaming stores: the dense SH gradient (300 B per Gaussian, written once, not read again by this library) should not
      // push the arrays the next forward streams (the harmonics themselves) out of the Infinity Cache: fwd + bwd steps -3 us
      typedef float f4v_ __attribute__((ext_vector_type(4)));
      for (int k = lane; k < n4; k += 64) {
        const float4 x = reinterpret_cast<const float4*>(lds)[k];
        __builtin_nontemporal_store(f4v_{x.x, x.y, x.z, x.w}, reinterpret_cast<f4v_*>(dst) + k);
      }
      for (int k = (n4 << 2) + lane; k < total; k += 64) dst[k] = lds[k];
    } else {
      for (int k = lane; k < total; k += 64) dst[k] = lds[k];
    }
  } else {
    for (int k = lane; k < total; k += 64) {
      const int row = k / rowf;
      dst[k] = lds[row * ldstride + (k - row * rowf)];
    }
  }
}

// ---- Host side: what every entry point of the library uses.
#define GSR_CHECK(expr)                       \
  do {                                        \
    if ((expr) != hipSuccess) return GSR_ERR_LAUNCH; \
  } while (0)

// Run-time bools as compile-time constants: dispatch_bools(f, a, b) calls f(std::bool_constant<a>{}, std::bool_constant<b>{}).  A generic
// lambda f names a kernel's template arguments once, where it is launched; every combination of its bools is instantiated.
template <class F>
static inline void dispatch_bools(F&& f) { f(); }
template <class F, class... Bools>
static inline void dispatch_bools(F&& f, bool b, Bools... rest) {
  if (b) dispatch_bools([&](auto... cs) { f(std::true_type{}, cs...); }, rest...);
  else dispatch_bools([&](auto... cs) { f(std::false_type{}, cs...); }, rest...);
}

}  // namespace gsr
