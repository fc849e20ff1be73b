/* gsr.h — C ABI of libgsr_hip.so, the MI355X (gfx950) differentiable 3D-Gaussian rasterizer.
 *
 * This is the drop-in boundary for the one native operator PF3plat depends on: the external
 * CUDA extension `diff_gaussian_rasterization` (reference requirements.txt:2), reached from
 * src/model/decoder/cuda_splatting.py:5-8 (import), :99-124 and :192-217 (call sites).  The
 * upstream extension exposes three pybind entry points (`rasterize_gaussians`,
 * `rasterize_gaussians_backward`, `mark_visible`; SURVEY.md §2 #6, Appendix A "Python-side");
 * the entry points below replace them one for one, with plain pointers and sizes instead of
 * torch tensors, and with two MI355X-first extensions the reference's per-view Python loop
 * (cuda_splatting.py:91-126) cannot express:
 *   - a call renders V views in one launch chain; views are grouped in `num_sets` sets that share
 *     one copy of the Gaussian arrays (kills decoder_splatting_cuda.py:52-56's V-fold `repeat`);
 *   - the scale-invariant pre-scale of cuda_splatting.py:64-71 is a per-view factor applied on
 *     load, and an optional extra blended channel carries the depth image of :226-269 in the same
 *     pass instead of a second raster pass.
 *
 * Conventions (all pointers are DEVICE pointers owned by the caller unless noted; the library
 * allocates nothing and keeps no state between calls, enqueues all work on `stream` as a plain chain of kernel launches
 * (capturable into a HIP graph), never synchronises the host (except in GSR_FLAG_DEBUG mode and when an _ex call is given stage_ms), never
 * throws; every entry point returns GSR_OK or a negative error code):
 *   means     (num_sets, N, 3)   fp32 world-space centres                     (means3D)
 *   cov6      (num_sets, N, 6)   fp32 xx,xy,xz,yy,yz,zz                       (cov3D_precomp)
 *   opacities (num_sets, N)      fp32 in (0,1)
 *   colors    (num_sets, N, M, 3) SH coefficients if sh_coeffs = M > 0        (shs)
 *             (num_sets, N, 3)   precomputed RGB if sh_coeffs == 0            (colors_precomp)
 *   extra     (V, N)             optional per-(view,Gaussian) scalar blended as a 4th channel
 *   views     (V) GsrView        cameras, in set-major order: view v uses set v / views_per_set
 *   out_color (V, 3, H, W), out_extra (V, H, W), radii (V, N) int32
 */
#ifndef GSR_H_
#define GSR_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GSR_OK 0
#define GSR_ERR_INVALID_ARGUMENT (-1)
#define GSR_ERR_LAUNCH (-2)
#define GSR_ERR_UNSUPPORTED (-3)
#define GSR_ABI_VERSION 5
/* GsrDims.flags input-layout bits: the arrays PF3plat's `Gaussians` record carries (src/model/types.py:7-18) can be passed
 * as they are, with no re-layout copy (the reference wrapper makes two per call: cuda_splatting.py:75 and :115,123). */
#define GSR_FLAG_SH_PLANAR 0x4  /* colors are (num_sets, N, 3, M) "harmonics" instead of (num_sets, N, M, 3); grads likewise */
#define GSR_FLAG_COV_3X3 0x8    /* cov6 points at (num_sets, N, 3, 3) symmetric matrices; dL_dcov6 is (num_sets, N, 3, 3) with
                                   the gradient on the upper triangle only (as the reference's triu gather yields) */
/* Harmonics in their group's frame (the encoder's adapter hands them over unrotated: gaussian_adapter.py:90-92 rotates them by
 * the source view's camera-to-world rotation F in torch).  GSR_FLAG_SH_IN_FRAME: the harmonics of Gaussian i of set s are in
 * the coordinates of frames[s, i / (N / F)] (the `frames` of GsrForwardOptions), and the kernels evaluate them at the view
 * direction d carried into that frame instead of rotating the coefficients.  With B the basis the kernels evaluate and
 * rotate_sh the rotation of pf3plat_amd/sh_rotation.py, for every rotation F and unit direction d:
 *   basis "rasterizer" (no second bit):     B(d) . rotate_sh(c, F) = B(F^T d) . c
 *   basis "e3nn" (GSR_FLAG_SH_FRAME_E3NN):   B(d) . rotate_sh(c, F) = B(G^T d) . c,  G = M F M^T,  M = Z P,
 *     P: (x, y, z) -> (z, x, y) (e3nn's polar axis is y), Z = diag(-1, -1, 1) (the (-1)^m phase: a half-turn about z).
 * The image and every gradient are those of the rotated coefficients; dL_dcolors comes back in the frame's coordinates, the
 * direction's gradient (dL_dmeans, and the camera centre of gsr_backward_ex) in world coordinates.  Frames get no gradient.
 * Valid only through gsr_forward_ex and gsr_backward_ex with opt->scale_rot != 0, with
 * non-NULL frames and sh_coeffs > 0 (GSR_FLAG_SH_FRAME_E3NN only together with GSR_FLAG_SH_IN_FRAME); anything else, and
 * gsr_workspace_sizes and the other helpers, return GSR_ERR_INVALID_ARGUMENT.  The bits do not change any workspace size:
 * size with the same dims without them.  At an evaluated degree of 0 they change nothing. */
#define GSR_FLAG_SH_IN_FRAME 0x40000
#define GSR_FLAG_SH_FRAME_E3NN 0x80000
/* GsrDims.flags bits 4-6: built-in extra channel.  0 = blend the caller's `extra` array; otherwise `extra` may be NULL and
 * the kernels blend f(z) of the camera-space depth in un-normalised units, i.e. the image the reference's
 * render_depth_cuda produces in each DepthRenderingMode (cuda_splatting.py:238-251) - in the same pass as the colour.
 * The backward then adds dL/dextra * f'(z) * dz/dmean to dL_dmeans itself (dL_dextra is not written). */
#define GSR_EXTRA_DEPTH 1
#define GSR_EXTRA_DISPARITY 2
#define GSR_EXTRA_RELATIVE_DISPARITY 3
#define GSR_EXTRA_LOG 4
#define GSR_FLAG_EXTRA_MODE(m) ((m) << 4)
/* GsrDims.flags bit 0: upstream's `prefiltered` (accepted and ignored: nothing is pre-filtered, exactly as upstream behaves
 * with prefiltered = False); bit 1: upstream's `debug` (cuda_splatting.py:111) - the library synchronises the stream after
 * every stage of the call and checks for errors; on failure the entry point returns GSR_ERR_LAUNCH and
 * gsr_last_failed_stage() names the stage. */
#define GSR_FLAG_PREFILTERED 0x1
#define GSR_FLAG_DEBUG 0x2
/* Deterministic backward: the per-(view, Gaussian) screen-space gradients are accumulated as 64-bit fixed-point integers
 * (integer atomics commute), so two runs on the same inputs return bit-identical gradients whatever order the tiles finish
 * in.  The resolution is relative, per view: the sums are kept in units of 2^-e, the power of two that brings the largest finite
 * |value| of that view's cotangent images (dL_dcolor, dL_dextra_img, dL_dalpha_img) into [1, 2), with a step of 2^-32 of that
 * unit and a clamp at 2^30 units per contribution - a loss that is a mean over millions of pixels (cotangents of 1e-8) or a
 * loss-scaled sum (2^20) is served like one of order one, and scaling every cotangent of a view by a power of two scales its
 * gradients by exactly that power.  A view's pixel whose cotangent is below 2^-32 of the view's largest is below the step.
 * Non-finite cotangents are not looked at for the unit.  The scratch buffer is then twice as large, plus one 4-byte word per
 * view (gsr_backward_scratch_bytes). */
#define GSR_FLAG_DETERMINISTIC 0x80
/* The caller will run gsr_backward on this forward's workspaces: the forward then also zero-fills the per-(view, Gaussian)
 * screen-space gradient rows (inside `geom`, which is that much larger) from its VALU-bound geometry kernel, and
 * gsr_backward called with the same dims and scratch == NULL accumulates into them - no separate zero-fill pass and no
 * extra launch in the backward.  A second backward over the same forward must bring its own `scratch` (the rows are used).
 * With harmonics (sh_coeffs > 0) the colour pass also saves d rgb / d (view direction) of every (view, Gaussian) (48 B, in
 * `geom`), and any backward called with this flag in its dims reads those instead of the harmonics themselves (300 of the
 * ~750 bytes per Gaussian the backward preprocess moves).  Forward and backward must therefore be called with the same flags. */
#define GSR_FLAG_BACKWARD_FOLLOWS 0x10000
/* Test aid: take the windowed binning path (preprocess, count, prefix, scan, emit, sort) even when the image has few enough
 * tiles for the fused one (k_preprocess_bin + gathering sort). */
#define GSR_FLAG_WINDOWED_BINNING 0x4000
/* Test aid: every per-tile index list is depth-ordered to its end.  Without it the tile launch of the usual case orders only
 * the nearest ~512 entries of a list before it blends and the rest only if the blend gets that far (a tile of a dense scene
 * stops after a quarter of its list): positions of a list beyond max(512, entries the tile walked) are then undefined.  The
 * backward never reads them.  Images, gradients and the status block are the same either way. */
#define GSR_FLAG_FULL_LISTS 0x20000
/* Tan-fov gradient (opt-in; learnable intrinsics): gsr_backward_ex with opt->dL_dviews and depth_term_only == 0 also writes
 * dL/dtanfovx and dL/dtanfovy into floats [35] and [36] of each view's row - as the operator reads the two fields: through
 * fx = W / (2 tanfovx), fy = H / (2 tanfovy) of the EWA Jacobian and the 1.3 tanfov limit a clamped t = V p sits on; the projection
 * matrix stays an independent input, as for the other blocks (gsr_setup_views_backward_ex joins the two halves).  Floats [37, 48)
 * stay zero.  The partial rows are then 37 floats wide: size pose_partials with gsr_pose_partials_bytes from dims that carry the bit.
 * Every other entry point, a backward without dL_dviews and one with depth_term_only != 0 accept the bit and ignore it: the same
 * kernel instances, the same bits out, the same workspace and scratch sizes. */
#define GSR_FLAG_FOV_GRADIENT 0x200000
/* Every other bit is rejected (GSR_ERR_INVALID_ARGUMENT). */
#define GSR_FLAG_VALID_MASK (GSR_FLAG_PREFILTERED | GSR_FLAG_DEBUG | GSR_FLAG_SH_PLANAR | GSR_FLAG_COV_3X3 | 0x70 | \
                             GSR_FLAG_DETERMINISTIC | GSR_FLAG_WINDOWED_BINNING | GSR_FLAG_BACKWARD_FOLLOWS | GSR_FLAG_FULL_LISTS | \
                             GSR_FLAG_SH_IN_FRAME | GSR_FLAG_SH_FRAME_E3NN | GSR_FLAG_FOV_GRADIENT)
#ifdef GSR_ABLATE
/* Measurement-only build (tools/ablate.py compiles its own copy of the library with -DGSR_ABLATE; the product library does
 * not contain these branches and rejects the bits): switches that make results WRONG on purpose to time a kernel without
 * one of its parts, and device-side phase stamps written into unused workspace. */
#define GSR_FLAG_ABLATE_NO_COUNT 0x100       /* preprocess: skip the per-tile pair counting atomics */
#define GSR_FLAG_ABLATE_NO_SH 0x200          /* skip the colour pass */
#define GSR_FLAG_ABLATE_EMIT_NO_STORE 0x400  /* emit: skip the key stores */
#define GSR_FLAG_ABLATE_EMIT_NO_ATOMIC 0x800 /* emit: skip the slot atomics */
#define GSR_FLAG_ABLATE_NO_GEOM_STORE 0x1000 /* preprocess: skip the projected-record store */
#define GSR_FLAG_DEBUG_TIMING 0x2000         /* phase stamps (100 MHz counter) into the tail of the key buffer */
#define GSR_FLAG_ABLATE_BWD_NO_ATOMIC 0x8000 /* backward blend: skip the per-splat atomic adds */
#define GSR_FLAG_ABLATE_MASK 0xbf00
#endif

/* One camera = the non-tensor fields of upstream's GaussianRasterizationSettings
 * (constructed at cuda_splatting.py:99-112), 48 floats = 192 bytes. */
typedef struct GsrView {
  float viewmatrix[16];  /* world->camera, transposed (row-vector convention), cuda_splatting.py:86,106 */
  float projmatrix[16];  /* full projection = view @ proj, transposed, cuda_splatting.py:87,107 */
  float campos[3];       /* camera centre in (pre-scaled) world units, cuda_splatting.py:109 */
  float tanfovx, tanfovy;
  float bg[3];
  float scale;           /* scale-invariant factor s applied on load: mean*s (cuda_splatting.py:70) */
  float scale2;          /* s*s computed by the caller in fp32: cov*s2 (cuda_splatting.py:69) */
  float scale_modifier;  /* upstream scale_modifier (only with scales/rotations; 1.0) */
  float reserved[5];     /* [0], [1]: un-normalised near / far of the view (used by GSR_EXTRA_RELATIVE_DISPARITY / _LOG) */
} GsrView;

typedef struct GsrDims {
  int32_t abi_version;    /* GSR_ABI_VERSION */
  int32_t num_views;      /* V = num_sets * views_per_set */
  int32_t num_sets;       /* independent Gaussian sets (scenes) */
  int32_t views_per_set;  /* views sharing one set */
  int32_t num_gaussians;  /* N per set */
  int32_t height, width;
  int32_t sh_degree;      /* active degree D (settings.sh_degree) */
  int32_t sh_coeffs;      /* M coefficients in memory; 0 => colours are precomputed RGB */
  int32_t max_sh_eval;    /* highest SH band evaluated (4; 3 = vanilla upstream) */
  int32_t has_extra;      /* 1 => `extra`/`out_extra` are used */
  int32_t flags;          /* GSR_FLAG_* | GSR_FLAG_EXTRA_MODE(m); unknown bits are rejected */
  int64_t pair_capacity;  /* capacity of the (tile,splat) pair workspaces, in pairs; see gsr_capacity_for */
} GsrDims;

/* Host-visible status block written by gsr_forward at the start of the `bin` workspace. */
typedef struct GsrStatus {
  uint64_t num_pairs;     /* total (8x8-tile, splat) pairs this call needs ("num_rendered") */
  uint32_t overflow;      /* 1 => pair_capacity too small (gsr_capacity_for): nothing was blended, call again bigger */
  uint32_t max_list;      /* longest per-tile list */
  uint64_t reserved[6];
} GsrStatus;

/* ABI/arch self-description; safe without a GPU. */
int gsr_abi_version(void);
const char* gsr_build_info(void);

/* Workspace sizes in bytes for a call with these dims (host-only arithmetic; no GPU needed).
 * geom: per-(view,Gaussian) projected records + colours; bin: status + per-tile counters/ranges + pair
 * lists (scales with pair_capacity); img: per-pixel final transmittance + contributor count.
 * Replaces upstream's geomBuffer/binningBuffer/imgBuffer resize callbacks. */
int gsr_workspace_sizes(const GsrDims* dims, size_t* geom_bytes, size_t* bin_bytes, size_t* img_bytes);

/* The pair_capacity that suits a call of these dims, given the status block of an earlier (possibly overflowed) call on
 * the same inputs.  Half of the index list is cut into one fixed slot per (view, tile), the other half is a shared region
 * for lists longer than a slot: 2 x num_pairs always suffices.  A slot of min(max_list, max(2 x mean list length, 256)) entries
 * keeps all but a few outlier lists in their slots (an outlier takes a run of the shared half from one bump counter) and
 * bounds the workspace by 4 x num_pairs however skewed the lists are (one dense tile does not size every slot).  Returns
 * 2 x max(num_pairs, views x tiles x slot).  Host-only arithmetic; callers add headroom. */
int64_t gsr_capacity_for(const GsrDims* dims, uint64_t num_pairs, uint32_t max_list);

/* Forward: replaces upstream `_C.rasterize_gaussians` (called through
 * GaussianRasterizer.forward at cuda_splatting.py:116-124).  `extra`/`out_extra` may be NULL when
 * has_extra == 0.  geom/bin/img must stay alive and untouched until gsr_backward has run. */
int gsr_forward(const GsrDims* dims, const GsrView* views, const float* means, const float* cov6,
                const float* opacities, const float* colors, const float* extra, float* out_color,
                float* out_extra, int32_t* radii, void* geom, void* bin, void* img, void* stream);

/* Backward: replaces upstream `_C.rasterize_gaussians_backward` (autograd of the call above).
 * dL_dcolor (V,3,H,W); dL_dextra_img (V,H,W) or NULL.  Outputs are fully written (zeros for culled
 * Gaussians): dL_dmeans (num_sets,N,3), dL_dcov6 (num_sets,N,6), dL_dopacities (num_sets,N),
 * dL_dcolors (same shape as colors), dL_dextra (V,N) or NULL, dL_dmeans2D (V,N,3) or NULL.
 * Gradients of views sharing a set are summed, including the scale / scale2 chain factors.
 * `scratch` holds gsr_backward_scratch_bytes(dims) bytes of screen-space accumulators (zero-filled by the call); it may be
 * NULL when the forward ran with GSR_FLAG_BACKWARD_FOLLOWS (the rows inside `geom` are used, once). */
#define GSR_SCREEN_GRAD_FLOATS 12
int gsr_backward(const GsrDims* dims, const GsrView* views, const float* means, const float* cov6,
                 const float* opacities, const float* colors, const float* extra, const void* geom,
                 const void* bin, const void* img, const float* dL_dcolor, const float* dL_dextra_img,
                 void* scratch, float* dL_dmeans, float* dL_dcov6, float* dL_dopacities,
                 float* dL_dcolors, float* dL_dextra, float* dL_dmeans2D, void* stream);

/* The extended calls: gsr_forward / gsr_backward with an options struct in front of `stream`.  opt == NULL: exactly the plain call,
 * and so is a zero-filled struct (every field opts in by being non-zero).  An optional image output or cotangent is a field of
 * these structs, appended behind the existing ones; it never gets an entry point of its own.
 *
 * scale_rot != 0: the covariances in the form PF3plat's encoder produces them (reference
 * src/model/encoder/common/gaussian_adapter.py:63-83, gaussians.py:8-44): `cov` is (num_sets, N, 7) = scale x, y, z and a
 * quaternion x, y, z, w; Sigma = M diag(scale^2) M^T with M = F Rq, Rq the rotation of the quaternion (normalised through
 * two_s = 2 / (|q|^2 + 1e-8), as quaternion_to_matrix does) and F an optional rotation into world space: `frames`
 * (num_sets, num_frames, 3, 3), the N Gaussians of a set being num_frames equal consecutive groups (one per source view:
 * the camera-to-world rotation of gaussian_adapter.py:81-83); NULL / 0 = no frame.  The covariance is built in registers
 * on load - no (N, 3, 3) array exists - and the backward returns dL_dcov as (num_sets, N, 7) directly.  GSR_FLAG_COV_3X3 does
 * not apply.  Without scale_rot, `frames` / `num_frames` are not read.
 *
 * stage_ms != NULL (measurement aid for bench.py, never on the product path): a host array of GSR_FWD_STAGES / GSR_BWD_STAGES
 * floats.  The same launch chain with a HIP event recorded on `stream` between stages; the call synchronises the stream and
 * returns per-stage milliseconds (zeros for an empty call).
 * Forward stages, in launch order: 0 the colour pass when it is a launch of its own (gsr_colour_in_binning == 0; otherwise
 * empty: it runs inside stage 1) 1 preprocess (geometry, hit masks and - images of up to 20 480 tiles - the whole binning)
 * 2 count + tile scans and 3 emit (windowed binning path only: empty, i.e. one event gap each, otherwise) 4 the tile launch
 * (per tile: gather + sort of its list, then its blend).
 * Backward stages: 0 blend backward 1 preprocess backward.
 *
 * dL_dviews != NULL (camera-pose gradients, opt-in - the reference gets none through the operator although
 * PF3plat learns poses): (V, 48) floats laid out like GsrView receive
 * dL/d viewmatrix [0, 16), dL/d projmatrix [16, 32), dL/d campos [32, 35) (zeros behind) - the two matrices as independent
 * inputs, the way the operator takes them; tan-fov gets one only with GSR_FLAG_FOV_GRADIENT (floats [35], [36]), background and
 * scale get none.  Every place the forward reads a camera
 * is differentiated (EWA covariance through t = V p and J Wr, projection to pixel coordinates, view direction of the
 * harmonics, depth of the built-in extra channel); depth ordering and culling are not, as for the Gaussians.  pose_partials:
 * gsr_pose_partials_bytes(dims) bytes of scratch (four rows per view and 64-Gaussian unit, of 35 floats - 37 with
 * GSR_FLAG_FOV_GRADIENT in the dims; reduced in a fixed order). */
#define GSR_FWD_STAGES 5
#define GSR_BWD_STAGES 2
typedef struct GsrForwardOptions {
  const float* frames;
  int32_t num_frames;
  int32_t scale_rot;
  float* stage_ms; /* [GSR_FWD_STAGES] host, or NULL */
  float* out_alpha; /* (V, H, W) accumulated alpha, or NULL: see below */
} GsrForwardOptions;
int gsr_forward_ex(const GsrDims* dims, const GsrView* views, const float* means, const float* cov, const float* opacities,
                   const float* colors, const float* extra, float* out_color, float* out_extra, int32_t* radii, void* geom,
                   void* bin, void* img, const GsrForwardOptions* opt, void* stream);
typedef struct GsrBackwardOptions {
  const float* frames;
  int32_t num_frames;
  int32_t scale_rot;
  float* dL_dviews;
  float* pose_partials;
  float* stage_ms; /* [GSR_BWD_STAGES] host, or NULL */
  int32_t depth_term_only; /* != 0: dL_dviews receives ONLY what the built-in depth channel (GSR_FLAG_EXTRA_MODE) sends to the
                              camera - floats 2, 6, 10, 14 of the view matrix, the row that forms z; zeros elsewhere.  This is the
                              one camera gradient the reference's own training graph carries: its depth render forms z with
                              extrinsics.inverse() in torch (cuda_splatting.py:239-242, extrinsics requiring grad at
                              model_wrapper.py:148-156) while nothing reaches a camera through the rasterizer.  Costs four wave
                              reductions in the backward preprocess instead of thirty-five and two small reduce launches. */
  int32_t reserved_;       /* 0: spells the padding in front of the next pointer out */
  const float* dL_dalpha_img; /* (V, H, W) cotangent of the accumulated alpha, or NULL: see below */
} GsrBackwardOptions;
size_t gsr_pose_partials_bytes(const GsrDims* dims);
int gsr_backward_ex(const GsrDims* dims, const GsrView* views, const float* means, const float* cov, const float* opacities,
                    const float* colors, const float* extra, const void* geom, const void* bin, const void* img,
                    const float* dL_dcolor, const float* dL_dextra_img, void* scratch, float* dL_dmeans, float* dL_dcov,
                    float* dL_dopacities, float* dL_dcolors, float* dL_dextra, float* dL_dmeans2D, const GsrBackwardOptions* opt,
                    void* stream);

/* Accumulated alpha.  GsrForwardOptions.out_alpha != NULL: one more output, (V, H, W),
 *   A = sum_j alpha_j T_j = 1 - T_final,   T_j = prod_{i < j} (1 - alpha_i),
 * over the splats the pixel blends, in the same pass and from the transmittance the colour pass keeps anyway (`img`): what the
 * extra channel blends for an `extra` array of ones, without spending that channel.  A pixel no splat reaches has A = 0 exactly.
 * A pixel that stops early (the next splat would leave T (1 - alpha) < 1e-4) reports the T in front of the rejected splat - the
 * value the background is weighted with - so colour = sum + (1 - A) bg holds exactly and A never reaches 1.  An empty call
 * (num_gaussians == 0) writes zeros; an overflowed one (GsrStatus.overflow) NaN, as for the colour.  The expected depth of a
 * pixel is out_extra / A with GSR_EXTRA_DEPTH, one pass; the clamp for small A is the caller's (no normalised mode exists).
 * GsrBackwardOptions.dL_dalpha_img != NULL: one more cotangent, (V, H, W): with
 * dA / dalpha_j = T_final / (1 - alpha_j) it enters the blend's backward where the background does and reaches every output
 * (dL_dviews included) through the splats' alphas.  dL_dcolor stays required: a caller with a loss on A alone passes zeros.
 * Neither field changes a workspace size or layout: size with gsr_workspace_sizes as usual, and either backward may follow
 * either forward (a backward with the cotangent after a forward without the image, and the other way round). */

/* GSR_FLAG_DEBUG: the stage of the last failed call of this host thread (an index into the stages above), or -1; and the
 * name of stage `stage` of the forward (backward == 0) or the backward - the one statement of the names every caller prints -
 * or NULL outside [0, GSR_FWD_STAGES) / [0, GSR_BWD_STAGES). */
int gsr_last_failed_stage(void);
const char* gsr_stage_name(int backward, int stage);

/* Bytes of the `scratch` buffer gsr_backward needs for these dims (V * N * 12 floats; twice that with
 * GSR_FLAG_DETERMINISTIC). */
size_t gsr_backward_scratch_bytes(const GsrDims* dims);

/* One camera record from the fields of upstream's GaussianRasterizationSettings, in ONE launch: the set-up of the per-view
 * API (the reference builds a settings object per view, cuda_splatting.py:99-112, and this library's own Python layer used to
 * assemble the record with a dozen small tensor ops).  viewmatrix / projmatrix: 16 contiguous device floats each, transposed as
 * the reference passes them; campos: 3 device floats `campos_stride` floats apart (the reference hands over extrinsics[i, :3, 3],
 * stride 4); bg: 3 device floats; tan-fov: host values, or - when the settings hold tensors, as render_cuda_orthographic's do
 * (:195-196) - one device float each (non-NULL pointer wins).  scale = 1 (the per-view API gets pre-scaled Gaussians). */
int gsr_pack_view(const float* viewmatrix, const float* projmatrix, const float* campos, int campos_stride, const float* bg,
                  float tanfovx, float tanfovy, const float* tanfovx_dev, const float* tanfovy_dev, float scale_modifier,
                  GsrView* out, void* stream);

/* Camera set-up in one launch: fills views[0..num_views) from camera-to-world extrinsics (V,4,4), normalised intrinsics
 * (V,3,3), near/far (V) and a background colour (background_stride 3: one per view; 0: one shared) - the arithmetic of the
 * reference wrapper at cuda_splatting.py:64-71 and :80-87 (get_fov of projection.py:233-247, get_projection_matrix of
 * cuda_splatting.py:17-44, extrinsics.inverse(), view @ proj).  scale_invariant != 0 applies the 1/near rescale. */
int gsr_setup_views(int num_views, const float* extrinsics, const float* intrinsics, const float* near, const float* far,
                    const float* background, int background_stride, int scale_invariant, GsrView* views, void* stream);

/* Backward of gsr_setup_views (scale_invariant as the records say): dL_dviews (V, 48) - the camera-record gradient gsr_backward_ex
 * returns, laid out like GsrView - carried to dL_dextrinsics (V, 4, 4) in closed form (view = (E'^-1)^T, full = view P^T,
 * campos = E'[:3, 3]; fp64 inside), one launch.  Intrinsics, near, far receive nothing here (intrinsics: the _ex call below).  This is the path by which the one camera
 * gradient of the reference's training graph - the depth render's extrinsics.inverse(), cuda_splatting.py:239-242 - reaches
 * `extrinsics` without a torch op. */
int gsr_setup_views_backward(int num_views, const GsrView* views, const float* dL_dviews, float* dL_dextrinsics, void* stream);

/* The same with the intrinsics' share, one launch, one thread per view, fp64 inside.  dL_dextrinsics (V, 4, 4), nullable: exactly
 * what gsr_setup_views_backward writes.  dL_dintrinsics (V, 3, 3), nullable, fully written: the cotangent of tanfovx is
 *   dL_dviews[35] + dL/dP[0][0] * (-1 / tanfovx^2),   dL/dP[0][0] = sum_i dL_dviews[16 + 4 i] * viewmatrix[4 i]
 * (its direct slot - GSR_FLAG_FOV_GRADIENT fills it - plus what the projection block says about P[0][0] = 1 / tanfovx), the y
 * component likewise with [36], P[1][1] and the indices + 1; both go back through tanf(0.5 acosf(l . r)), the normalised
 * edge-midpoint rays K^-1 (x, y, 1) of get_fov and K^-1 to `intrinsics` (V, 3, 3), the array gsr_setup_views took, all recomputed from
 * it in fp64.  Near, far, background and scale still receive nothing.  GSR_ERR_INVALID_ARGUMENT on a negative count or a NULL
 * views / intrinsics / dL_dviews; nothing is launched for a count of 0. */
int gsr_setup_views_backward_ex(int num_views, const GsrView* views, const float* intrinsics, const float* dL_dviews,
                                float* dL_dextrinsics, float* dL_dintrinsics, void* stream);

/* The same for the reference's fake orthographic camera (render_cuda_orthographic, cuda_splatting.py:153-181): per view the
 * extent (width, height) of the orthographic window in world units; the camera is moved back along its own -z by
 * (width / 2) / tan(fov_degrees / 2) and near / far move with it; no scale-invariant step.  The reference's quirk is kept:
 * the projection's y scale uses fov_y = atan(2 tan_fov_y) (:160) while tanfovy holds tan_fov_y.  `dump` (nullable,
 * num_views x 20 floats): moved extrinsics (16), fov_x, fov_y, near, far - the values of the wrapper's `dump` dict. */
int gsr_setup_views_orthographic(int num_views, const float* extrinsics, const float* width, const float* height,
                                 const float* near, const float* far, const float* background, int background_stride,
                                 float fov_degrees, GsrView* views, float* dump, void* stream);

/* Replaces upstream `_C.mark_visible` (GaussianRasterizer.markVisible): present[i] = 1 iff the
 * Gaussian passes the near-plane test of view 0 of its set (p_view.z > 0.2). */
int gsr_mark_visible(const GsrDims* dims, const GsrView* views, const float* means, uint8_t* present,
                     void* stream);

/* Covariances from scales + rotations: what upstream's preprocess does when `scales`/`rotations` are given instead of
 * `cov3D_precomp` ([EXT] forward.cu computeCov3D; quaternion (r, x, y, z), not normalised): cov6 (n, 6) = upper triangle of
 * R diag((scale_modifier * s)^2) R^T, and its backward ([EXT] backward.cu computeCov3D) from the dL/dcov6 that gsr_backward
 * returns (doubled off-diagonals).  dL_dscales / dL_drotations may be null.  Reference call site: the `scales=`, `rotations=`
 * arguments of GaussianRasterizer.forward (PF3plat itself passes cov3D_precomp, cuda_splatting.py:123). */
int gsr_cov_from_scale_rot(int64_t n, const float* scales, const float* rotations, float scale_modifier, float* cov6,
                           void* stream);
int gsr_cov_from_scale_rot_backward(int64_t n, const float* scales, const float* rotations, float scale_modifier,
                                    const float* dL_dcov6, float* dL_dscales, float* dL_drotations, void* stream);

/* Image losses of the step right after the raster path, one launch: for `num_images` images (num_images, 3, H, W)
 *   L = mse_weight * mean((prediction - target)^2) + ssim_weight * (1 - mean(SSIM map))
 * with the reference's definitions (src/loss/loss_mse.py:23-36; src/loss/loss_multissim.py:24-83: 11 x 11 Gaussian window, sigma
 * 1.5, zero padding, C1 = 0.01^2, C2 = 0.03^2; both means run over every element of the batch).  Writes dL/dprediction
 * (nullable) in the layout gsr_backward takes as dL_dcolor, and one slot of 4 floats per workgroup into `partials`
 * (gsr_image_loss_partials(...) slots, workgroups of an image consecutive): sum of squared errors, sum of squared errors of
 * the inputs clipped to [0, 1] (compute_psnr, src/evaluation/metrics.py:11-19), sum of the SSIM map, 0.  The caller adds the
 * slots up (a deterministic reduction) and forms the scalars. */
size_t gsr_image_loss_partials(int num_images, int height, int width);
int gsr_image_loss(int num_images, int height, int width, const float* prediction, const float* target, float mse_weight,
                   float ssim_weight, float* dL_dprediction, float* partials, void* stream);
/* The slots of gsr_image_loss added up on the device, in a fixed order (one more launch instead of the caller's reductions):
 * sums (num_images, 4) - per image the three sums and a 0 - and totals[0..2] = L as defined above, mean squared error, mean SSIM
 * over the batch (`totals`: four floats, the fourth 0).  One workgroup, no atomics: the same bits every time. */
int gsr_image_loss_finish(int num_images, int height, int width, const float* partials, float mse_weight, float ssim_weight,
                          float* sums, float* totals, void* stream);

/* Evaluation metrics of the raster path (reference src/evaluation/metrics.py: compute_psnr :11-19, compute_ssim :36-52), forward
 * only, for `num_images` pairs (num_images, 3, H, W), H and W at least 11.  The SSIM here is the METRIC, what
 *   skimage.metrics.structural_similarity(ground_truth, prediction, win_size=11, gaussian_weights=True, channel_axis=0, data_range=1.0)
 * returns for one image, and differs from the SSIM of gsr_image_loss (the training loss's) in four places.  Per image and channel,
 * x the ground truth and y the prediction:
 *   window    w[k] = exp(-k^2 / (2 * 1.5^2)), k = -5..5, normalised to sum 1, applied along both axes (the loss's eleven numbers);
 *   boundary  the image is extended by reflection about its edge, d c b a | a b c d | d c b a: index -1 - j reads j and H + j reads
 *             H - 1 - j (scipy.ndimage mode="reflect", numpy pad "symmetric").  The loss pads with zeros.
 *   moments   ux, uy, uxx, uyy, uxy = the filtered x, y, x^2, y^2, x y;
 *   variances the SAMPLE ones: vx = cn (uxx - ux^2), vy = cn (uyy - uy^2), vxy = cn (uxy - ux uy), cn = 121 / 120.  The loss uses cn = 1.
 *   map       S = (2 ux uy + C1)(2 vxy + C2) / ((ux^2 + uy^2 + C1)(vx + vy + C2)), C1 = 1e-4, C2 = 9e-4, on every pixel;
 *   mean      a channel's value is the mean of S over 5 <= row < H - 5, 5 <= col < W - 5 (the loss: over every pixel), an image's
 *             value the mean of its three channels' (the loss: one mean over the batch).  The inputs are not clipped.
 * gsr_image_metrics is one launch: it writes S to ssim_map (num_images, 3, H, W) unless that is NULL, and one slot of 4 floats per
 * workgroup into `partials` (gsr_image_metrics_partials(...) slots; layout and order of gsr_image_loss's): sum of squared errors,
 * sum of squared errors of the inputs clipped to [0, 1], sum of S over the workgroup's interior pixels, 0.
 * gsr_image_metrics_partials is 0 for whatever the launch refuses (a side below 11, num_images <= 0 or 3 num_images > 65535).
 * The slots are added up by this call's OWN finish, gsr_image_metrics_finish (one workgroup, fixed order, no atomics: the same bits
 * every time, an image's row independent of the rest of the batch): metrics (4, num_images) floats = per image the SSIM, the PSNR
 * -10 log10(clipped squared error / (3 H W)), the interior sum of S and the clipped squared-error sum.  (gsr_image_loss_finish reads
 * the same slots and would return the three raw sums; its totals divide by every pixel and mean nothing here.) */
size_t gsr_image_metrics_partials(int num_images, int height, int width);
int gsr_image_metrics(int num_images, int height, int width, const float* ground_truth, const float* prediction,
                      float* ssim_map /* NULL = none */, float* partials, void* stream);
int gsr_image_metrics_finish(int num_images, int height, int width, const float* partials, float* metrics, void* stream);

/* The perceptual distance's head: what lpips.LPIPS(net="vgg"), version "0.1", in eval() mode does AFTER its VGG16 convolutions
 * (reference src/loss/loss_lpips.py and compute_lpips, src/evaluation/metrics.py:27-33, which call that package with
 * normalize=True).  The package is not part of the reference tree, so this text is the definition the operator is held to.
 *   input     two image batches (N, 3, H, W) in [0, 1]; x <- 2 x - 1 (normalize=True), then (x - shift) / scale per channel,
 *             shift = (-.030, -.088, -.188), scale = (.458, .448, .450).
 *   features  VGG16 `features`, tapped after relu1_2, relu2_2, relu3_3, relu4_3, relu5_3: C_l = 64, 128, 256, 512, 512 channels on
 *             floor(H / 2^l) x floor(W / 2^l) pixels, l = 0 .. 4 (a 2 x 2 max-pool opens slices 2 to 5).  The convolutions are the
 *             caller's (torch / MIOpen); everything from here on is this operator.
 *   head      per layer l, for the feature maps a, b (N, C, h, w) of the two images and non-negative weights w_c (the `lin` layers):
 *               r_a = sqrt(sum_c a_c^2), n_a = r_a + 1e-10, a^_c = a_c / n_a, the same for b, at every pixel;
 *               d_l(n) = (1 / (h w)) sum over the pixels of sum_c w_c (a^_c - b^_c)^2;      value(n) = sum_l d_l(n).
 *             The difference a^_c - b^_c is formed per channel: the expanded form sum w a^2 / n_a^2 + sum w b^2 / n_b^2 -
 *             2 sum w a b / (n_a n_b) loses the value in f32 when the prediction approaches the target (6 % at a relative
 *             difference of 1e-3, C = 512) and is not used.
 *   gradient  given g_n = dL/dvalue(n), at every pixel: u_c = 2 g_n w_c (a^_c - b^_c) / (h w), s = sum_c u_c a_c,
 *               dL/da_c = u_c / n_a - a_c s / (r_a n_a^2);        dL/db_c the same with a and b exchanged and the sign of u flipped.
 *             It is evaluated as (u_c - t_c q) / n_a + t_c q eps / n_a^2 with t = a / r_a, q = sum_c u_c t_c, eps = 1e-10 - the same
 *             number, since r_a / n_a = 1 - eps / n_a -, which cancels exactly where u is parallel to a (always at one channel); the
 *             form above returns rounding noise there in f32.
 *   DEPARTURE at a pixel whose feature vector is entirely zero (r_a = 0) autograd of the package's lines returns NaN (0 / 0 in
 *             sqrt's backward) - the reason the reference skips optimiser steps on NaN gradients.  This operator returns an exact 0
 *             for that vector's gradient (the ReLU behind it would zero any finite value anyway); the VALUE at such a pixel follows
 *             the definition, a^ = 0.  The other image's vector at that pixel has its usual gradient.
 *             "Entirely zero" is decided on the f32 sum of squares: a non-zero vector whose elements are all below about 1e-23
 *             underflows it and is treated as zero, value and gradient (VGG features are not of that size).
 * GsrLpipsLayers, passed BY VALUE, is the layer table: 1 <= num_layers <= GSR_LPIPS_MAX_LAYERS rows of the two feature arrays
 * (N, channels, height, width), contiguous f32, and the `channels` weights; 1 <= channels <= 1024, height, width >= 1,
 * height x width <= 2^31 - 1.  The layers need not be a VGG pyramid: any channel counts and sizes.
 * gsr_lpips_head: ONE launch for all layers.  A unit of work is (layer, image, run of gsr_lpips_head_pixel_run(channels) consecutive
 *   pixels): a workgroup of 256 threads holds its unit's two feature blocks in registers - lanes along the pixels, the channels
 *   (stride h w) dealt over 256 / run groups of at most gsr_lpips_head_channel_slots() each - so the norms (first trip over the
 *   channels) and the differences (second trip) read memory once.  It writes ONE float per workgroup into `partials`
 *   (gsr_lpips_head_partials(num_images, layers) floats: host arithmetic, 0 for what the launch refuses - num_images < 1, a bad
 *   table, more than 16 777 215 units: a launch takes at most 2^32 - 1 threads).
 * gsr_lpips_head_finish: one workgroup, a fixed order, no atomics: values (num_images) and per_layer (num_images,
 *   GSR_LPIPS_MAX_LAYERS) = d_l(n), 0 in the columns from num_layers on.  The same bits on every call, and an image has the bits
 *   in a batch that it has alone.
 * gsr_lpips_head_backward: ONE launch for all layers, the same units; `g` (num_images) f32; dL_da, dL_db: HOST arrays of num_layers
 *   device pointers, each shaped like its feature array; an array pointer or any entry may be NULL: that gradient is neither
 *   computed nor stored.  Nothing to write: nothing is launched.  Every element of a requested gradient is written.
 * GSR_ERR_INVALID_ARGUMENT, nothing launched: whatever the partials query refuses, a NULL feature, weight, partials or output
 * pointer.  num_images == 0 is refused too (there is nothing to size). */
#define GSR_LPIPS_MAX_LAYERS 5
typedef struct GsrLpipsLayer {
  const float* a;       /* (N, channels, height, width) */
  const float* b;       /* the same shape */
  const float* weight;  /* (channels) */
  int32_t channels, height, width, reserved_;
} GsrLpipsLayer;
typedef struct GsrLpipsLayers {
  int32_t num_layers, reserved_;
  GsrLpipsLayer layer[GSR_LPIPS_MAX_LAYERS];
} GsrLpipsLayers;
int gsr_lpips_head_channel_slots(void);
int gsr_lpips_head_pixel_run(int channels); /* 0 for channels outside 1 .. 1024 */
size_t gsr_lpips_head_partials(int num_images, GsrLpipsLayers layers);
int gsr_lpips_head(int num_images, GsrLpipsLayers layers, float* partials, void* stream);
int gsr_lpips_head_finish(int num_images, GsrLpipsLayers layers, const float* partials, float* values, float* per_layer, void* stream);
int gsr_lpips_head_backward(int num_images, GsrLpipsLayers layers, const float* g, float* const* dL_da /* NULL = none */,
                            float* const* dL_db /* NULL = none */, void* stream);

/* The encoder-side Gaussian adapter, the step right in front of the raster path (reference
 * src/model/encoder/common/gaussian_adapter.py:60-87 with get_world_rays), one launch: G groups (scene x source view) of P
 * pixel-aligned Gaussians each, M = (sh_degree + 1)^2 for sh_degree 0..4.
 *   extrinsics (G, 4, 4) camera-to-world, intrinsics (G, 3, 3) normalised, coordinates (G, P, 2), depths (G, P);
 *   raw: G x P rows of 7 + 3 M floats = scale features (3) | quaternion x, y, z, w (4) | harmonics (3, M), consecutive rows
 *        `raw_row_stride` floats apart (>= 7 + 3 M) - the encoder hands over the slice `gaussians[..., 2:]` of an 84-wide tensor
 *        (encoder_costvolume.py:535-538), which is read where it is (stride 84);
 *   means (G, P, 3) = t + depth R normalise(K^-1 (u, v, 1));
 *   scale_rot (G, P, 7), the record form gsr_forward_ex takes with scale_rot: (scale_min + (scale_max - scale_min) sigmoid(r)) x depth x
 *        0.1 sum(K[:2, :2]^-1 (1 / width, 1 / height)), and q / (|q| + eps);
 *   harmonics (G, P, 3, M) (GSR_FLAG_SH_PLANAR layout): the raw coefficients times 1 (DC) or 0.1 x 0.25^l (band l).
 * K^-1 and the multiplier are formed once per group.  Opacities do not pass through here.
 * gsr_adapt_backward takes the forward's inputs again (everything is recomputed: nothing is saved) and the cotangents dL_dmeans
 * (G, P, 3), dL_dscale_rot (G, P, 7) - the array gsr_backward_ex writes with scale_rot - and dL_dharmonics (G, P, 3, M), each of which
 * may be NULL (zeros).  Outputs, all fully written: dL_draw (G, P, 7 + 3 M) contiguous, dL_ddepths (G, P), dL_dcoordinates (G, P, 2)
 * and dL_dextrinsics (G, 4, 4): rows 0-2 x columns 0-2 the sum over the group of dmean (x) (depth ray), column 3 the sum of
 * dmean, bottom row zero (PF3plat's extrinsics are learned poses: this is how the render loss reaches them through the means).
 * That sum is formed in a fixed order - one row per workgroup in `partials` (gsr_adapt_partials_bytes(G, P) bytes of scratch:
 * host arithmetic), then one reduce launch - so the same bits come out on every run.  A zero quaternion takes the norm's
 * gradient as 0, as torch does.
 * gsr_adapt_backward_ex is gsr_adapt_backward with one more output, dL_dintrinsics (G, 3, 3), nullable.  NULL: the same kernels,
 * launches, output bits and `partials` size as gsr_adapt_backward (which is this call with NULL).  Otherwise `partials` holds
 * gsr_adapt_partials_bytes_ex(G, P, 1) bytes (rows of 22 floats instead of 12; with_intrinsics = 0 gives gsr_adapt_partials_bytes),
 * the per-workgroup rows also carry Ginv = sum over the group of d_p (x) (u, v, 1) - d_p the cotangent of p = K^-1 (u, v, 1),
 * taken as orthogonal to the ray where the norm was not clamped - and g_mult = sum of depth x sum_r dL_dscale[r] (scale_min +
 * (scale_max - scale_min) sigmoid(r)), the cotangent of the multiplier, and the reduce launch (still the only one) writes, in fp64,
 *   dL/dK          = -K^-T Ginv K^-T                                  (all nine entries)
 *   dL/dK[:2, :2] += -0.1 g_mult (K2^-T 1) (K2^-1 q)^T,   K2 = K[:2, :2], q = (1 / width, 1 / height), 1 = (1, 1)
 * the second line being the backward of the multiplier 0.1 1^T K2^-1 q.  dL_dintrinsics is fully written; a group whose cotangents
 * are all NULL or zero gets zeros.
 * All calls: GSR_ERR_INVALID_ARGUMENT on negative sizes, a degree outside 0..4, a stride below 7 + 3 M or a NULL required pointer;
 * nothing is launched when G or P is 0. */
size_t gsr_adapt_partials_bytes(int num_groups, int gaussians_per_group);
size_t gsr_adapt_partials_bytes_ex(int num_groups, int gaussians_per_group, int with_intrinsics);
int gsr_adapt(int num_groups, int gaussians_per_group, int sh_degree, const float* extrinsics, const float* intrinsics,
              const float* coordinates, const float* depths, const float* raw, int64_t raw_row_stride, float scale_min,
              float scale_max, int height, int width, float eps, float* means, float* scale_rot, float* harmonics, void* stream);
int gsr_adapt_backward(int num_groups, int gaussians_per_group, int sh_degree, const float* extrinsics, const float* intrinsics,
                       const float* coordinates, const float* depths, const float* raw, int64_t raw_row_stride, float scale_min,
                       float scale_max, int height, int width, float eps, const float* dL_dmeans, const float* dL_dscale_rot,
                       const float* dL_dharmonics, float* dL_draw, float* dL_ddepths, float* dL_dcoordinates, float* dL_dextrinsics,
                       float* partials, void* stream);
int gsr_adapt_backward_ex(int num_groups, int gaussians_per_group, int sh_degree, const float* extrinsics, const float* intrinsics,
                          const float* coordinates, const float* depths, const float* raw, int64_t raw_row_stride, float scale_min,
                          float scale_max, int height, int width, float eps, const float* dL_dmeans, const float* dL_dscale_rot,
                          const float* dL_dharmonics, float* dL_draw, float* dL_ddepths, float* dL_dcoordinates, float* dL_dextrinsics,
                          float* dL_dintrinsics, float* partials, void* stream);

/* The pose loss of the training step (reference src/loss/loss_pose.py:28-129, `Losspose`), one launch chain each way.
 * Inputs, all f32 unless said otherwise, b scenes of v >= 2 views of H x W pixels:
 *   xyz (b, v, 3, H, W) per-pixel points; depth (b, v, H, W); poses (b, v, 4, 4) - of a pose only the top three rows are read and
 *   only they receive a gradient (the bottom row is taken as (0, 0, 0, 1)); intrinsics (b, v, 3, 3), normalised, no gradient;
 *   one match list per pair p = (i, j), i < j - pairs in the order [(a, c) for a in range(v) for c in range(a + 1, v)], num_pairs =
 *   v (v - 1) / 2 - and per scene s, list l = p b + s (pair-major): entries offsets[l] .. offsets[l + 1] of ids_i, ids_j (int64, flat
 *   pixel indices y W + x) and weights (the matcher's scores); conf (num_pairs b) one confidence per list.  Scores and confidences get
 *   no gradient.  A list may be empty; its length is not bounded.  IDS ARE NOT CHECKED: an id outside [0, H W) is the caller's error
 *   and reads or adds out of bounds.
 * Per list: Rt = poses[s, j] when i == 0 (the reference's shortcut: poses[s, 0] is never read, whatever it holds), otherwise
 *   Rt = poses[s, j] poses[s, i]^-1, the affine inverse with a general 3 x 3 inverse, formed in fp64 once per list; R, t its parts.
 *   3D term  L3 = conf sum_m w_m |R x_i[id_i_m] + t - x_j[id_j_m]| / max(sum_m |w_m|, 1e-12)
 *   2D term  c(id) = ((id % W + 0.5) / W, (id / W + 0.5) / H) in fp32;  P = depth_i[id_i] K_i^-1 (c(id_i), 1);
 *            Q = (R P + t) / (1 + 1e-6);  q = (K_j Q)_xy / ((K_j Q)_z + 1e-6);  r = |q - c(id_j)|;
 *            L2 = sum_m huber(r_m, delta = 0.01) / 0.01   (a sum, unweighted)
 *   loss = weight_3d mean_l L3 + weight_2d mean_l L2; an empty list adds 0 and counts in the means' denominators; the gradient of a
 *   norm at an exactly zero residual is 0.
 * Work is cut into units of 256 consecutive matches of one list; gsr_pose_loss_units (host arithmetic) counts them from the
 * num_lists + 1 offsets - -1 for a NULL pointer, a negative count or start, or offsets that decrease.  `offsets` is that HOST array
 * (it is validated and sizes the launch), `offsets_device` the same numbers in device memory (the kernels read them).
 * gsr_pose_loss: one launch over the units - `partials`: units x 4 floats - and a one-workgroup finish that adds the rows of each
 *   list and then the lists in fp64 in a fixed order: out[0..3] = loss, mean L3, mean L2, 0; lists (num_lists, 4) = per list L3, L2,
 *   the factor weight_3d conf / (max(sum |w|, 1e-12) num_lists) the backward takes, sum |w|.  The same bits on every run, and a
 *   list's row does not depend on the other lists.
 * gsr_pose_loss_backward: takes the same inputs again (everything is recomputed), `lists` as the forward wrote it and the upstream
 *   cotangent dL_dloss as ONE FLOAT IN DEVICE MEMORY (no host read).  It zero-fills dL_dxyz (b, v, 3, H, W) and dL_ddepth (b, v, H, W)
 *   and adds into them with float atomics - order-independent, hence the same bits on every run, wherever a pixel receives at most
 *   two contributions (with three views nearly everywhere; a pixel can occur in several lists, and twice in one when two keypoints
 *   truncate to it); elsewhere the last bits may differ between runs.  dL/dRt leaves as one row of 12 floats per unit (`partials`:
 *   units x 12 floats) that a reduce launch adds per list in fp64 in a fixed order, carries to poses[s, j] and, for i > 0, through
 *   the inverse to poses[s, i], and sums per view over its pairs in their order: dL_dposes (b, v, 4, 4), bottom rows zero, the
 *   same bits on every run.
 * Both: GSR_ERR_INVALID_ARGUMENT, nothing launched, on a NULL required pointer, negative or decreasing offsets, num_views < 2,
 * num_pairs != v (v - 1) / 2, a non-positive extent or H W > 2^31 - 1.  num_scenes == 0: the forward writes zeros to `out`. */
int64_t gsr_pose_loss_units(int num_lists, const int32_t* offsets);
int gsr_pose_loss(int num_scenes, int num_views, int height, int width, int num_pairs, const float* xyz, const float* depth,
                  const float* poses, const float* intrinsics, const int64_t* ids_i, const int64_t* ids_j, const float* weights,
                  const float* conf, const int32_t* offsets, const int32_t* offsets_device, float weight_2d, float weight_3d,
                  float* partials, float* lists, float* out, void* stream);
int gsr_pose_loss_backward(int num_scenes, int num_views, int height, int width, int num_pairs, const float* xyz, const float* depth,
                           const float* poses, const float* intrinsics, const int64_t* ids_i, const int64_t* ids_j,
                           const float* weights, const float* conf, const int32_t* offsets, const int32_t* offsets_device,
                           float weight_2d, float weight_3d, const float* lists, const float* dL_dloss, float* dL_dxyz,
                           float* dL_ddepth, float* dL_dposes, float* partials, void* stream);

/* The plane-sweep cost volume of the encoder (reference src/model/encoder/costvolume/depth_predictor_multiview.py:28-141 and
 * 321-343: prepare_feat_proj_data_lists, warp_with_pose_depth_candidates and the correlation), one launch chain each way.
 * Inputs, all f32: features (b, v, c, h, w); intrinsics (b, v, 3, 3), normalised; extrinsics (b, v, 4, 4), camera-to-world - the top
 * three rows are read, the bottom row is taken as (0, 0, 0, 1); near, far (b, v); D = num_depth_candidates.
 * Output: cost (v b, D, h, w), VIEW-MAJOR: row i b + s is view i of scene s (the reference's `(v b)` order).
 * For row (i, s), pixel (x, y) with integer x in 0..w-1, y in 0..h-1 (no half-pixel offset) and candidate d:
 *   K       = intrinsics[s, i] with row 0 x w and row 1 x h; view i's K both unprojects and reprojects into the other view (a
 *             property of the reference, kept);
 *   depth_d = 1 / (1 / far[s, i] + lin_d (1 / near[s, i] - 1 / far[s, i])), lin = linspace(0, 1, D) formed in float32 (D = 1: lin = [0]);
 *   for k = 1 .. v-1 the other view is j = (i + k) mod v and P = extrinsics[s, j]^-1 extrinsics[s, i] (for v = 2, i = 1 the reference
 *             forms the inverse of row 0's matrix: the same matrix), R_P, t_P its parts;
 *   q       = K (R_P K^-1 (x, y, 1)^T depth_d + t_P);  px = q_x / max(q_z, 1e-3), py = q_y / max(q_z, 1e-3);
 *   warp_k[c] = the bilinear sample of features[s, j, c] at (px, py) in pixel-index units (grid_sample with align_corners = True,
 *             the reference's 2 px / (w - 1) - 1 undone), zero padding: a tap outside [0, w-1] x [0, h-1] contributes 0;
 *   cost[i b + s, d, y, x] = 1 / (v - 1) sum_k sum_c features[s, i, c, y, x] warp_k[c] / sqrt(c).
 * Set-up (P, K R_P K^-1, K t_P, the candidates) is formed in fp64 once per (row, other view); a sample is q = depth a + K t in
 * fp32.  Whether a tap is inside is decided on floats before anything is converted to an integer: no px, py - huge, infinite or
 * NaN (points behind the camera, q_z clamped) - leads to a read or an add outside the arrays.
 * Gradients go to `features` only (the reference builds its grid under no_grad and detaches the candidates): each features row
 * receives one gradient as the reference feature of its own row and one as the sampled feature of every row that samples it.
 * Nothing proportional to c D h w exists in either direction.  `scratch`: gsr_cost_volume_scratch_bytes(b, v, c, h, w, backward)
 * bytes (host arithmetic; 0 for sizes the calls refuse) - forward one channels-last copy of the features, (b, v, h, w, c rounded up
 * to 4) floats; backward that copy again (everything is recomputed from the inputs: nothing is saved) and a gradient of the same
 * shape, which the call zero-fills.
 * gsr_cost_volume: a transpose launch and one launch over the volume; the same bits on every run.
 * gsr_cost_volume_backward: takes the forward's inputs and dL_dcost (v b, D, h, w); a zero-fill, the transpose, one launch over the
 *   volume and a transpose back; dL_dfeatures (b, v, c, h, w) is fully written.  The sampled-feature gradient is a scatter with
 *   float atomics (the taps of consecutive candidates on the same source pixels are summed on chip first), and a pixel receives
 *   adds from many rows' pixels in the order they arrive: dL_dfeatures is NOT bit-reproducible - its last bits can differ from run
 *   to run wherever a source pixel is sampled from more than one pixel or walk segment (nearly everywhere).
 * All three: GSR_ERR_INVALID_ARGUMENT (0 bytes), nothing launched, on a NULL pointer, b < 0, v < 2, c < 1, h < 2 or w < 2 (the
 * reference's normalisation divides by w - 1), D < 1, or more than 2^31 - 1 elements in the features, the padded copy or the
 * volume.  b == 0: nothing is launched. */
size_t gsr_cost_volume_scratch_bytes(int num_scenes, int num_views, int channels, int height, int width, int backward);
int gsr_cost_volume(int num_scenes, int num_views, int channels, int height, int width, int num_depth_candidates, const float* features,
                    const float* intrinsics, const float* extrinsics, const float* near, const float* far, float* cost, void* scratch,
                    void* stream);
int gsr_cost_volume_backward(int num_scenes, int num_views, int channels, int height, int width, int num_depth_candidates,
                             const float* features, const float* intrinsics, const float* extrinsics, const float* near,
                             const float* far, const float* dL_dcost, float* dL_dfeatures, void* scratch, void* stream);

/* The encoder's coarse camera poses (reference src/model/encoder/encoder_costvolume.py:323-381: cv2.solvePnPRansac per pair and scene,
 * then src/flow_util.py:623-743 camera_synchronization), forward only, three launches and no host synchronisation.
 * Inputs, b scenes of 2 <= v <= 8 views of H x W pixels: xyz (b, v, 3, H, W) f32; intrinsics_px (b, v, 3, 3) f32 IN PIXEL UNITS, of
 *   which fx = [0][0], fy = [1][1], cx = [0][2], cy = [1][2] are read; the match lists as gsr_pose_loss takes them (list l = p b + s,
 *   pairs p = (i, j), i < j, in the order [(a, c) for a in range(v) for c in range(a + 1, v)]; ids_i, ids_j int64, weights f32 the
 *   matcher's scores, offsets on the host and on the device); points_2d (M, 2) f32 or NULL, sub-pixel keypoints (x, y) in the pair's
 *   first view - NULL: the 2-D point of match k is (ids_i[k] % W, ids_i[k] / W); hypotheses Hy >= 1 (the reference: 1000);
 *   reprojection_error > 0 in pixels (5); confidence_min < 1 (0.5); seed.  An id outside [0, H W) is the caller's error; it is
 *   clamped into the image, not followed out of the array.
 * Per list (pair (i, j), scene s, n matches): X_k = xyz[s, j, :, ids_j[k]], u_k the 2-D point, K = intrinsics_px[s, i].  Sought is
 *   (R, t) with u ~ pi(K (R X + t)); the list's output is the rigid inverse [R^T | -R^T t] (the reference's `relpose`).
 *   1. Hypothesis t = 0 .. Hy-1 draws four matches, slot = 0 .. 3, index draw(seed, l, t, slot) mod n in uint32 arithmetic with
 *        fmix(x): x ^= x >> 16; x *= 0x85EBCA6B; x ^= x >> 13; x *= 0xC2B2AE35; x ^= x >> 16
 *        draw = fmix(fmix(fmix(seed ^ 0x9E3779B9 (l + 1)) ^ 0x85EBCA6B (t + 1)) ^ 0xC2B2AE35 (slot + 1)).
 *      Duplicates are allowed and give a degenerate hypothesis.  A P3P solve in fp64 on the first three (the law of cosines on the
 *      three rays; a quartic by Ferrari's resolvent, its real roots polished by two Newton steps; every root with both signs of the
 *      depths, the equations' solutions behind the camera included) gives up to eight poses; the one under which the fourth point
 *      has the smallest reprojection error is kept (the first of equals; the depth is judged by the score, not here).  A hypothesis
 *      with no finite pose is skipped.  ALL Hy hypotheses are evaluated:
 *      there is no early exit on a confidence as OpenCV's RANSAC has (its `confidence=0.9999`).
 *   2. Score: the number of matches with (R X + t)_z > 0 and |pi - u|^2 < reprojection_error^2, the pose rounded to fp32 and the
 *      test in fp32, written so that a NaN fails it.  The winner is the maximum of the words (score << 32) | (Hy - 1 - t) - an
 *      integer maximum, independent of the order: the highest score, of equals the lowest t.
 *   3. Refinement in fp64: three rounds of { the consensus set (the same test in fp64) under the current pose; ten Gauss-Newton steps
 *      on sum |pi - u|^2 over that set, update R <- exp(w) R, t <- t + d, the 6 x 6 normal equations summed in fp64 in a fixed
 *      order and solved by Cholesky }.  The consensus set under the final pose is the list's inlier count and, on request, `mask`
 *      (M) uint8.
 *   4. Failure gives the identity, inlier count 0 and a zero mask; status: 0 a pose, 1 n < 4 (gsr_pnp_min_matches), 2 the winner
 *      explains fewer than 4 matches (or no hypothesis had a pose), 3 the refined pose is not finite.
 *   5. confidence[l] = the mean of the list's weights (fp64 sum in a fixed order), 0 FOR AN EMPTY LIST - the reference has NaN there,
 *      which poisons the whole batch: a deliberate difference; for pairs with j - i > 1 then relu(c - confidence_min) /
 *      (1 - confidence_min) in fp32.
 * gsr_pnp_ransac: launch 1 over (list, block of 256 hypotheses) - a lane solves one hypothesis, then the workgroup walks the list in
 *   LDS stages of 1024 matches (3-D point + 2-D point, 20 bytes each; longer lists in several stages), every lane counting for its own
 *   pose, and publishes the integer maximum of its words to its slot of `scratch` (gsr_pnp_ransac_scratch_bytes(b, v, Hy) bytes, 8 per
 *   (list, block); host arithmetic, 0 for sizes the call refuses); launch 2, one workgroup per list, takes the maximum of the list's
 *   slots, solves the winner again from its index (the same arithmetic, the same pose: no pose is stored), refines, and writes
 *   pairwise (b, P, 4, 4) - row [s, p] -, inliers, status, confidence (P b, in list order) and mask.  Nothing proportional to Hy x n
 *   exists.
 * gsr_camera_sync: pairwise (b, P, 4, 4), confidence (P b) -> absolute (b, v, 4, 4): camera_synchronization at its default arguments,
 *   one workgroup per scene: confidences normalised per column and the (4 v)^2 matrix formed in fp32 in the reference's order of
 *   operations - the column sums of the normalisation included, which torch's CPU kernel takes row by row for columns in groups of
 *   four and with four interleaved partial sums (rows 4 m + k; the rows left over go to the first; ((p0 + p1) + p2) + p3) for the
 *   columns left over at v = 5, 6, 7 and for every column at v = 8: one fp32 ulp there moves the result by about 1e-6 -,
 *   converted to fp64, squared 10 times in LDS, block column 0 divided by its mass, the rotations projected onto SO(3)
 *   as U diag(1, 1, det(U V^T)) V^T (8 sweeps of one-sided Jacobi), rounded once to fp32.  v = 2: camera_chaining (identity, then
 *   P(i, i+1) times the pose before it, fp32).  A scene one of whose v masses is exactly 0 takes camera_chaining FOR THAT SCENE, decided
 *   on the device; the reference decides for the whole batch after a host read: a difference for batches that mix such scenes.
 * Every value is a pure function of the inputs and the seed - the same bits on every run; no floating-point atomics; every loop's
 * trip count is fixed by the arguments (hypotheses, rounds, steps, sweeps, squarings, list lengths): no loop waits on data.
 * Both: GSR_ERR_INVALID_ARGUMENT, nothing launched, on v < 2, v > 8, num_pairs != v (v - 1) / 2, b < 0, Hy < 1 or > 2^24, a
 * non-positive extent, H W > 2^31 - 1, negative or decreasing offsets, a threshold that is not positive, confidence_min >= 1 or a NULL
 * required pointer (mask, points_2d may be NULL; ids and weights when there is no match).  b == 0: nothing is launched. */
int gsr_pnp_min_matches(void);
size_t gsr_pnp_ransac_scratch_bytes(int num_scenes, int num_views, int hypotheses);
int gsr_pnp_ransac(int num_scenes, int num_views, int height, int width, int num_pairs, const float* xyz, const float* intrinsics_px,
                   const int64_t* ids_i, const int64_t* ids_j, const float* weights, const float* points_2d, const int32_t* offsets,
                   const int32_t* offsets_device, int hypotheses, float reprojection_error, float confidence_min, uint32_t seed,
                   void* scratch, float* pairwise, int32_t* inliers, int32_t* status, float* confidence, uint8_t* mask, void* stream);
int gsr_camera_sync(int num_scenes, int num_views, const float* pairwise, const float* confidence, float* absolute, void* stream);

/* The depth lift of the encoder (reference src/model/encoder/encoder_costvolume.py:265, 287-307, 506, 525-528: the two clamps, the
 * one-hot "mono cue" and the unprojection; :211-221, 387-392: the Pluecker ray map).  All arrays f32; b scenes of v >= 1 views of
 * h x w pixels, h, w >= 4 (any such size, not only multiples of 4); hq = h / 4, wq = w / 4 (integer division); D candidates.
 * gsr_lift_depth: depth_raw, shift ((b v), 1, h, w); near, far (b, v); intrinsics (b, v, 3, 3), normalised; `lin` (D) the candidates'
 *   positions in [0, 1] in device memory, or NULL for torch's float32 linspace(0, 1, D) (formed as the cost volume forms it: from the
 *   start below the middle, from the end above it) -> depth ((b v), 1, h, w), xyz (b, v, 3, h, w), cue ((v b), D, hq, wq).  One launch.
 *   depth = clamp(clamp(depth_raw, near, far) + shift, near, far) with the view's own bounds, clamp(x, lo, hi) = min(max(x, lo), hi):
 *     one fp32 rounding (the addition), bit-equal to the float32 torch form.  A NaN in depth_raw or shift stays a NaN in depth and
 *     in the pixel's xyz.
 *   xyz[s, i, :, y, x] = K^-1 ((x + 0.5) / w, (y + 0.5) / h, 1)^T depth, K = intrinsics[s, i]: the FULL 3 x 3 inverse by cofactors
 *     in fp64 once per view (no upper-triangular assumption; a singular K is the caller's error and is not checked), the ray in fp64,
 *     rounded once, times the depth in fp32.  The reference unprojects twice (`xyz_up_h`, and `xyz_refine` after a third clamp with
 *     the same bounds, which changes nothing): both are this tensor.
 *   cue: VIEW-MAJOR rows as the cost volume's - row i b + s is view i of scene s.  down = the bilinear resize of depth to (hq, wq)
 *     in torch's arithmetic (F.interpolate, align_corners = False: source index max((dst + 0.5) in / out - 0.5, 0) in fp32, the
 *     second tap clamped to the last row / column; value l0y (l0x v00 + l1x v01) + l1y (l0x v10 + l1x v11)), its taps recomputed from
 *     depth_raw and shift.  hyp_d = 1 / far[0, 0] + lin_d (1 / near[0, 0] - 1 / far[0, 0]) in fp32.  Every quarter-resolution pixel has
 *     1 in channel argmin_d |down - hyp_d| - the first minimum, as torch.argmin: ties go to the lowest channel - and 0 in the other
 *     D - 1.  TWO QUIRKS OF THE REFERENCE ARE KEPT: (1) the hypotheses are INVERSE depths and are compared with a DEPTH; (2) they come
 *     from scene 0, view 0 for the whole batch, whatever the other views' bounds are (read on the device: no host synchronisation).
 *     The written channel is in [0, D) whatever the inputs: a pixel with a NaN or infinite tap gets a valid, otherwise unspecified
 *     channel.  The cue is written exactly once, as whole row segments; there is no zero-fill and no scatter, and no array of the
 *     cue's size other than the cue.
 * gsr_lift_depth_backward: the forward's inputs again (everything is recomputed) and the cotangents dL_ddepth ((b v), 1, h, w) and
 *   dL_dxyz (b, v, 3, h, w), either or both NULL (taken as zero):
 *     dL_dshift = m2 (dL_ddepth + sum_c dL_dxyz_c ray_c),  dL_ddepth_raw = m1 dL_dshift,
 *   m1 = near <= depth_raw <= far and m2 = near <= clamp(depth_raw) + shift <= far, the clamps' pass-through masks, inclusive at the
 *   bounds as torch's clamp backward; where a mask is false the gradient is an exact zero.  The sum is taken in fp64 and rounded once.
 *   Either output may be NULL.  The cue has no gradient (the reference detaches it); near and far receive none.  One launch.
 *   dL_dintrinsics (b, v, 3, 3), when not NULL: the chain through K^-1, dK = -K^-T (sum_p dL_dxyz_p ((x + 0.5) / w, (y + 0.5) / h, 1)
 *   depth_p) K^-T, summed in fp64 in a fixed order - per thread, per wave, per workgroup of 1024 pixels into `scratch`
 *   (gsr_lift_scratch_bytes(b, v, h, w) bytes, host arithmetic, 0 for sizes the calls refuse; 9 doubles per workgroup), then one
 *   finishing launch that adds an image's workgroups in order: the same bits on every run.  Zero when dL_dxyz is NULL.
 * gsr_plucker_rays: c2w (b, v, 4, 4) camera-to-world, of which the top three rows are read; intrinsics (b, v, 3, 3), normalised ->
 *   out ((b v), 6, H, W), H, W >= 1: channels 0-2 the world-space unit direction of pixel centre ((x + 0.5) / W, (y + 0.5) / H) -
 *   K^-1 (u, v, 1) normalised in camera space, then rotated by c2w[:3, :3] (the reference's get_world_rays) -, channels 3-5
 *   cross(c2w[:3, 3], direction) (its plucker_embedding).  fp64 throughout, rounded once.  Forward only; one launch.
 * All: GSR_ERR_INVALID_ARGUMENT, nothing launched, on a NULL required pointer, b < 0, v < 1, h or w < 4 (the lift), D < 1 or more than
 * 2^31 - 1 elements in any array; b == 0: nothing is launched.  No floating-point atomics anywhere. */
size_t gsr_lift_scratch_bytes(int num_scenes, int num_views, int height, int width);
int gsr_lift_depth(int num_scenes, int num_views, int height, int width, int num_depth_candidates, const float* depth_raw,
                   const float* shift, const float* near, const float* far, const float* intrinsics, const float* lin, float* depth,
                   float* xyz, float* cue, void* stream);
int gsr_lift_depth_backward(int num_scenes, int num_views, int height, int width, const float* depth_raw, const float* shift,
                            const float* near, const float* far, const float* intrinsics, const float* dL_ddepth, const float* dL_dxyz,
                            float* dL_ddepth_raw, float* dL_dshift, float* dL_dintrinsics, void* scratch, void* stream);
int gsr_plucker_rays(int num_scenes, int num_views, int height, int width, const float* c2w, const float* intrinsics, float* out,
                     void* stream);

/* The "multi guided by mono" attention of the depth predictor (reference src/model/encoder/costvolume/depth_predictor_multiview.py:
 * 360-366), which follows the cost volume.  All arrays f32 and CHANNEL-MAJOR: q, k (n, E, L), v (n, C, L); n rows ((v b) in the
 * reference), L = h_down w_down positions, E score channels, C value channels.
 *   s[b, i, j] = sum_e q[b, e, i] k[b, e, j]          (no 1 / sqrt(E) factor: the reference has none)
 *   p = softmax_j s
 *   out[b, c, i] = sum_j p[b, i, j] v[b, c, j]        (n, C, L)
 *   lse[b, i] = log sum_j exp s[b, i, j]              (n, L), kept for the backward
 * gsr_mono_attention: one launch over (row, block of 128 queries, chunk of 64 value channels); the key axis is streamed 32 keys at a
 *   time with the online softmax (running maximum and sum, rescaled accumulator), so scores of any size are safe and NO array of
 *   L x L elements exists anywhere.  Every channel chunk forms the same scores and statistics in the same order.  Every product runs on the f32-input matrix instruction (v_mfma_f32_32x32x2_f32): exact f32, one rounding per
 *   product, accumulated in key order.  exp and log are the accurate f32 functions.  The same bits on every run.
 * gsr_mono_attention_backward: S and P are recomputed from q, k and lse;
 *     delta[i] = sum_c dO[c, i] out[c, i],  dV[c, j] = sum_i dO[c, i] P[i, j],  dP[i, j] = sum_c dO[c, i] v[c, j],
 *     dS = P (dP - delta),  dK[e, j] = sum_i dS[i, j] q[e, i],  dQ[e, i] = sum_j dS[i, j] k[e, j].
 *   Three launches: delta into `scratch` (gsr_mono_attention_scratch_bytes(n, E, L, C) bytes: n L floats; host arithmetic, 0 for
 *   sizes the calls refuse); a pass over blocks of 128 keys that streams the queries and leaves dK and dV; a pass over blocks of 128
 *   queries that streams the keys and leaves dQ (the second pass recomputes P and dP: no sum ever crosses a workgroup).  No
 *   atomics: every gradient has the same bits on every run.  Any of dL_dq, dL_dk, dL_dv may be NULL; a pass none of whose outputs is
 *   wanted is not launched.  Saved state and scratch are O(n L (E + C)).
 * Both: GSR_ERR_INVALID_ARGUMENT, nothing launched, unless 1 <= E <= 32, 1 <= C <= 256, L >= 1, n >= 1 and
 * n max(E, C) L <= 2^31 - 1, or on a NULL required pointer.  No host synchronisation, no internal streams. */
size_t gsr_mono_attention_scratch_bytes(int n, int E, int L, int C);
int gsr_mono_attention(int n, int E, int L, int C, const float* q, const float* k, const float* v, float* out, float* lse, void* stream);
int gsr_mono_attention_backward(int n, int E, int L, int C, const float* q, const float* k, const float* v, const float* out,
                                const float* lse, const float* dL_dout, float* dL_dq, float* dL_dk, float* dL_dv, void* scratch,
                                void* stream);

/* Multi-head attention: the softmax attention of LightGlue's SelfBlock and CrossBlock (reference src/model/LightGlue/lightglue/
 * lightglue.py:133-224), of which the encoder's pose transformer is built (src/model/encoder/encoder_costvolume.py:401-441).  All f32.
 * Operands: q is logically (B, H, N, D), k and v are logically (B, H, M, D); each comes with FOUR ELEMENT STRIDES (batch, head,
 *   token, channel) and is read where it lies, offsets formed in 64 bits - the reference's two layouts without a copy:
 *   qkv.unflatten(-1, (H, -1, 3)).transpose(1, 2)[..., i] has strides (3 N H D, 3 D, 3 H D, 3), .unflatten(-1, (H, -1))
 *   .transpose(1, 2) has (N H D, D, H D, 1).
 *     s[b, h, i, j] = scale * sum_c q[b, h, i, c] k[b, h, j, c]
 *     p = softmax_j s
 *     out[b, i, h, c] = sum_j p[b, h, i, j] v[b, h, j, c]
 *     lse[b, h, i] = log sum_j exp s[b, h, i, j]          (B, H, N), kept for the backward
 * Results are TOKEN-MAJOR and contiguous: out, dL_dout and dL_dq are (B, N, H, D), dL_dk and dL_dv (B, M, H, D) - what
 *   context.transpose(1, 2).flatten(-2) hands to the output projection without a copy.
 * gsr_attention: one launch over (batch, head, block of 128 queries).  As the mono attention above: the key axis is streamed 32 keys
 *   at a time with the online softmax, so scores of any size are safe and NOTHING of N x M elements exists anywhere; every product
 *   runs on v_mfma_f32_32x32x2_f32 (exact f32, accumulated in key order); expf and logf are the accurate functions.  `scale`
 *   MULTIPLIES THE SCORE TILE: s is the f32 product scale * (q . k), rounded once after the channel sum, with the same bits in the
 *   forward and in both backward passes; dQ and dK take the factor once, on the finished sum.
 * gsr_attention_backward: S and P are recomputed from q, k and lse;
 *     delta[b, h, i] = sum_c dO[b, i, h, c] out[b, i, h, c],  dV[j] = sum_i P[i, j] dO[i],  dP[i, j] = sum_c dO[i, c] v[j, c],
 *     dS = P (dP - delta),  dK[j] = scale sum_i dS[i, j] q[i],  dQ[i] = scale sum_j dS[i, j] k[j].
 *   Three launches: delta into `scratch` (gsr_attention_scratch_bytes(B, H, N, M, D) bytes: B H N floats; host arithmetic, 0 for
 *   sizes the calls refuse); a pass over blocks of 128 keys that streams the queries and leaves dK and dV; a pass over blocks of 128
 *   queries that streams the keys and leaves dQ.  Any of dL_dq, dL_dk, dL_dv may be NULL; a pass none of whose outputs is wanted is
 *   not launched.  No atomics and no sum crosses a workgroup: forward and gradients have the same bits on every run.  Saved state and
 *   scratch are O(B H (N + M) D).
 * All: GSR_ERR_INVALID_ARGUMENT, nothing launched, unless B, H, N, M >= 1, 1 <= D <= 32, B H max(N, M) D <= 2^31 - 1, `scale` is
 * finite and no required pointer (the stride arrays included) is NULL.  No host synchronisation, no internal streams. */
size_t gsr_attention_scratch_bytes(int B, int H, int N, int M, int D);
int gsr_attention(int B, int H, int N, int M, int D, float scale, const float* q, const int64_t* q_strides, const float* k,
                  const int64_t* k_strides, const float* v, const int64_t* v_strides, float* out, float* lse, void* stream);
int gsr_attention_backward(int B, int H, int N, int M, int D, float scale, const float* q, const int64_t* q_strides, const float* k,
                           const int64_t* k_strides, const float* v, const int64_t* v_strides, const float* out, const float* lse,
                           const float* dL_dout, float* dL_dq, float* dL_dk, float* dL_dv, void* scratch, void* stream);

/* Ragged multi-head attention: the attention of LightGlue's matcher transformer (reference src/model/LightGlue/lightglue/
 * lightglue.py:133-256: SelfBlock on both images, the bidirectional CrossBlock; heads of 64 channels), for every (pair, scene) list
 * of a batch in one launch.  Forward only (the reference runs the matcher under no_grad).  All f32.
 * Units: a call has U >= 1 units.  Unit u is a query row range [q_begin[u], q_begin[u] + q_count[u]) and a key row range
 *   [k_begin[u], k_begin[u] + k_count[u]) of ONE row space of T rows - the packed token buffer; counts >= 0, every range inside
 *   [0, T].  Self-attention of both images of L lists is 2 L units whose key range is their query range; both directions of the
 *   cross-attention are 2 L units whose key range is the partner's.  The four arrays (U int32 each) are given on the host - the grid is
 *   sized from them - and on the device, where the kernel reads them (clamped to [0, T]), as the match assignment takes its offsets.
 *   The query ranges of a call should be disjoint: a row two units own is written by both.
 * Operands: q, k, v are each logically (T, H, D) with THREE ELEMENT STRIDES (token, head, channel), read where they lie, offsets
 *   formed in 64 bits: the interleaved Wqkv output, (T, 3 H D) viewed as (T, H, D, 3)[..., i], has (3 H D, 3 D, 3); a plain
 *   projection has (H D, D, 1).  1 <= D <= 64.
 * Rotary encoding: `rot`, or NULL, is (2, T, D) contiguous - cosines, then sines, row t for packed row t - and D is even.  q and k
 *   (not v) are rotated while they are staged, as apply_cached_rotary_emb (lightglue.py:57-58), each product and the sum rounded:
 *     x'[2 p] = x[2 p] cos[2 p] - x[2 p + 1] sin[2 p]        x'[2 p + 1] = x[2 p + 1] cos[2 p + 1] + x[2 p] sin[2 p + 1]
 * With i a query row and j a key row of unit u:
 *     s[h, i, j] = scale * sum_c q'[i, h, c] k'[j, h, c]        (the f32 sum over c in order, rounded once more by scale)
 *     p = softmax over the unit's keys j of s
 *     out[i, h, c] = sum_j p[h, i, j] v[j, h, c]               (T, H, D), token-major and contiguous
 *     lse[h, i] = log sum_j exp s[h, i, j]                      (H, T)
 *   A unit with k_count = 0 writes out = 0 and lse = -inf for its rows (the reference's Attention.forward returns zeros there,
 *   :107-108).  Rows no unit owns as queries are NOT written.
 * One launch over (unit, block of 128 queries, head): the keys are streamed 32 at a time with the online softmax, NOTHING of n x m
 *   elements exists anywhere; every product runs on v_mfma_f32_32x32x2_f32 (exact f32, accumulated in key order); expf and logf are
 *   the accurate functions.  A workgroup finds its unit by a scan of the device counts: no table is built, no host read, and
 *   `scratch` (gsr_ragged_attention_scratch_bytes(...) bytes: 16 for a call it accepts, 0 for one it refuses; host arithmetic) is
 *   not touched.  No atomics: the same bits on every call.  A call none of whose units has a query launches nothing.
 * GSR_ERR_INVALID_ARGUMENT, nothing launched, unless U, T, H >= 1, 1 <= D <= 64, D is even when `rot` is given, every begin and
 *   count is >= 0 and every range ends at or before T, T H D <= 2^31 - 1 (and H times the query blocks, which only overlapping units
 *   can push there), `scale` is finite and no required pointer (the host and device arrays, the stride arrays and `scratch`
 *   included; `rot` may be NULL) is NULL.  All of it is host arithmetic.  No host synchronisation, no internal streams. */
size_t gsr_ragged_attention_scratch_bytes(int U, int T, int H, int D, const int32_t* q_begin_host, const int32_t* q_count_host,
                                          const int32_t* k_begin_host, const int32_t* k_count_host);
int gsr_ragged_attention(int U, int T, int H, int D, float scale, const int32_t* q_begin_host, const int32_t* q_begin_device,
                         const int32_t* q_count_host, const int32_t* q_count_device, const int32_t* k_begin_host,
                         const int32_t* k_begin_device, const int32_t* k_count_host, const int32_t* k_count_device, const float* q,
                         const int64_t* q_strides, const float* k, const int64_t* k_strides, const float* v, const int64_t* v_strides,
                         const float* rot, float* out, float* lse, void* scratch, void* stream);

/* Match assignment: the tail of LightGlue - MatchAssignment.forward after its two projections, sigmoid_log_double_softmax and
 * filter_matches (reference src/model/LightGlue/lightglue/lightglue.py:259-312) and the list building of :586-597 - for a whole batch
 * of (pair, scene) lists at once.  Forward only (the reference runs the matcher under no_grad).
 * A call has L >= 1 lists; list l has m_l >= 0 keypoints of the first image and n_l >= 0 of the second.  Operands are packed along
 *   the keypoint axis, contiguous f32: mdesc0 (sum m_l, d), mdesc1 (sum n_l, d) - the outputs of final_proj, NOT yet divided by
 *   d ** 0.25 -, z0 (sum m_l), z1 (sum n_l) the matchability logits.  The two offset arrays (L + 1 int32 each, list l is entries
 *   offsets[l] .. offsets[l + 1]) are given on the host and on the device, as the PnP call takes its own: they come from shapes.
 *   1 <= d <= 256; offsets_m[L] d and offsets_n[L] d at most 2^31 - 1; `scale` (the reference: d ** -0.5) and `threshold` finite.
 * With ls = logsigmoid, per list (indices local to the list):
 *     s[i, j]  = scale * sum_c mdesc0[i, c] mdesc1[j, c]      (the f32 sum over c in order, times scale: one more rounding)
 *     lr[i]    = log sum_j exp s[i, j]        lc[j] = log sum_i exp s[i, j]
 *     a[i, j]  = 2 s[i, j] - lc[j] + ls(z1[j])        m0[i] = the lowest j that maximises a[i, .]
 *     b[i, j]  = 2 s[i, j] - lr[i] + ls(z0[i])        m1[j] = the lowest i that maximises b[., j]
 *     max0[i]  = a[i, m0[i]] - lr[i] + ls(z0[i])      (the reference's scores[:, :m, :n].max(2).values)
 *     mutual0[i] = (m1[m0[i]] == i)     mscores0[i] = mutual0 ? exp(max0[i]) : 0     valid0 = mutual0 and mscores0 > threshold
 *     mutual1[j] = (m0[m1[j]] == j)     mscores1[j] = mutual1 ? mscores0[m1[j]] : 0
 *     matches0[i] = valid0[i] ? m0[i] : -1            matches1[j] = (mutual1[j] and valid0[m1[j]]) ? m1[j] : -1
 *   - the reference's lines with the per-row and per-column constants taken out of the two arg-maxima.  In f32 the arg-maxima compare
 *   2 s + (ls(z) - l)[the other index], one fused rounding, and max0 is formed from s at the arg-maximum in the reference's order of
 *   operations: ((s - lr[i]) + (s - lc[j])) + (ls(z0[i]) + ls(z1[j])), each s - l as log_softmax forms it, (s - max) - log sum exp(. - max)
 *   (l is kept as the pair: where a row is peaked s - max is exact).  ls(z) = min(z, 0) - log1p(exp(-|z|)).
 * Differences from the reference: the dust-bin row and column (scores[:, :-1, -1], scores[:, -1, :-1]) are not computed -
 *   filter_matches never reads them; the reference divides each operand by d ** 0.25, here one factor multiplies the sum; TIES GO TO
 *   THE LOWEST INDEX (torch.max promises no order); a list with m_l = 0 or n_l = 0 has no matches: -1 and 0 everywhere, as the
 *   reference's lines 563-583; NaN or infinite inputs are the caller's error (every index read back stays inside its list).
 * Outputs: matches0 (sum m_l), matches1 (sum n_l) int32; mscores0, mscores1 f32; and the COMPACT form: for list l the valid
 *   (i, matches0[i], mscores0[i]) in ascending i in idx0, idx1 (int32), score (f32) at entries offsets_m[l] .. + count[l], count (L)
 *   int32.  The capacity is sum m_l: no prefix sum crosses lists and nothing is read back; entries past a list's count are not
 *   written.  With kpts0 (sum m_l, 2), kpts1 (sum n_l, 2) (x, y), both or neither, and an image width w >= 1, the same launch writes
 *   next to each compact entry ids_i = trunc(y0) w + trunc(x0), ids_j likewise (int64: the reference's `.long()` of
 *   src/model/encoder/encoder_costvolume.py:340-342) and points (.., 2) = (x0, y0), the sub-pixel point the PnP call takes.
 * Three launches of one kernel on the caller's stream (one when no list has both sides), no host synchronisation:
 *   1. statistics: grid over (list, side, block of 128 owned keypoints); the owned descriptors in registers, the other image's
 *      streamed in tiles of 32 through LDS, each s tile on v_mfma_f32_32x32x2_f32 over the channels in order; lr by the online
 *      log-sum-exp (a running maximum: scores of any size are safe); lc by the MIRRORED pass, the other half of the grid's rows.
 *   2. arg-maxima: the same tiling and the same s bits (the same products in the same order, scale at the same place): m0 and m1
 *      with s there.
 *   3. filter and compaction: one workgroup per list; rows in ascending chunks of 256 ranked by a workgroup scan.
 *   `scratch`: gsr_match_assignment_scratch_bytes(L, offsets_m, offsets_n, d) bytes - 16 per keypoint of either image; host
 *   arithmetic, 0 for sizes the call refuses.  NOTHING of m x n elements exists.  No atomics, no sum across workgroups, expf / logf /
 *   log1pf the accurate functions: the same bits on every run.
 * GSR_ERR_INVALID_ARGUMENT, nothing launched: L < 1, d outside 1 .. 256, negative or decreasing offsets, a total times d above
 *   2^31 - 1, a `scale` or `threshold` that is not finite, a NULL required pointer (kpts0, kpts1, ids_i, ids_j, points may be NULL
 *   together), keypoints without a positive width or without their three outputs. */
size_t gsr_match_assignment_scratch_bytes(int L, const int32_t* offsets_m_host, const int32_t* offsets_n_host, int d);
int gsr_match_assignment(int L, int d, float scale, float threshold, int width, const float* mdesc0, const float* mdesc1, const float* z0,
                         const float* z1, const int32_t* offsets_m_host, const int32_t* offsets_m_device, const int32_t* offsets_n_host,
                         const int32_t* offsets_n_device, const float* kpts0, const float* kpts1, void* scratch, int32_t* matches0,
                         int32_t* matches1, float* mscores0, float* mscores1, int32_t* idx0, int32_t* idx1, float* score, int64_t* ids_i,
                         int64_t* ids_j, float* points, int32_t* count, void* stream);

/* Keypoint extraction: what SuperPoint.forward does after its last two convolutions (reference
 * src/model/LightGlue/lightglue/superpoint.py:52-95, 171-227, with the rescale of utils.py:146) - the 65-way softmax, the 8 x 8
 * depth-to-space, simple_nms, the border cut, torch.where against the threshold, the dense descriptor normalisation and
 * sample_descriptors - for a batch of B equally sized images.  Forward only (the reference runs the extractor under no_grad).
 * Inputs, f32: `logits` (B, 65, h, w) contiguous, convPb's output before the softmax; `descriptors` (B, C, h, w), 0 <= C <= 256
 *   (0: none), convDb's output, NOT normalised, read through its four element strides (contiguous and channels_last both work
 *   without a copy); `scales` (B, 2) the preprocessor's (sx, sy), or NULL.  `height` = H = 8 h and `width` = W = 8 w are given in PIXELS.
 *   mode GSR_KEYPOINTS_FROM_LOGITS: step 1 below WRITES `scores` (B, H, W) - the one dense array of the call.
 *   mode GSR_KEYPOINTS_FROM_SCORES: the chain is entered after step 1: `scores` (B, H, W) is the caller's and only read, `logits` is
 *   ignored, and H, W need not be multiples of 8 unless C > 0.
 * 1. scores: p = softmax of a cell's 65 logits (maximum m, e_c = exp(l_c - m), their f32 sum in channel order, e_c / sum); channel 64
 *    is dropped; cell (i, j)'s channel 8 a + c is pixel (8 i + a, 8 j + c).
 * 2. NMS, exactly simple_nms with windows of (2 r + 1) squared padded with -inf, 0 <= r <= 4:
 *      max_mask = (s == maxpool(s));  TWICE (not "until stable" - two rounds are the definition):
 *        supp_mask = maxpool(max_mask) > 0;  supp_scores = supp_mask ? 0 : s;
 *        max_mask |= (supp_scores == maxpool(supp_scores)) and not supp_mask.
 *    A pixel's result depends on scores up to 5 r pixels away.  Equal scores are all kept.  Every decision is a comparison of
 *    scores: nothing is rounded from step 2 on.
 * 3. selection: pixels with remove_borders <= y < H - remove_borders, the same in x, in max_mask and with s > threshold
 *    (threshold >= 0, finite), per image in row-major order - torch.where's.  counts[b] = the number found, WHATEVER the capacity.
 *    max_num_keypoints = k > 0 and k < counts[b] <= capacity: the k highest scores in descending order, TIES TO THE LOWER ROW-MAJOR
 *    INDEX (the reference's topk leaves the order of ties open); 0: no cut.  counts[b] > capacity: the image OVERFLOWS: its first
 *    `capacity` pixels in row-major order are stored, without the cut, nothing is written past them, and counts[b] tells.
 *    stored(b) = counts[b] > capacity ? capacity : (k > 0 and counts[b] > k ? k : counts[b]).
 * 4. descriptors (C > 0), sample_descriptors on the L2-normalised map without forming that map: pixel (x, y) samples at
 *    (ix, iy) = ((x - 3.5) / (8 w - 4.5) (w - 1), (y - 3.5) / (8 h - 4.5) (h - 1)), bilinearly, zeros outside (reachable only with
 *    remove_borders < 4): with x0 = floor(ix), t = ix - x0 and the same in y, weights (1 - tx)(1 - ty), tx (1 - ty), (1 - tx) ty,
 *    tx ty on the columns at (x0, y0), (x0 + 1, y0), (x0, y0 + 1), (x0 + 1, y0 + 1), EACH DIVIDED BY max(its norm over C, 1e-12);
 *    the blend, summed in that order, is divided by max(its own norm, 1e-12).
 * 5. keypoints (x, y) f32 = (pixel + 0.5) / scale - 0.5 with IEEE division; without `scales` the pixel itself.
 * Outputs, PACKED image after image: image b's rows are base(b) .. base(b) + stored(b), base(b) = sum of stored over the images
 *   before it, formed on the device: `keypoints` (B capacity, 2) f32, `pixels` (B capacity, 2) int32 (x, y), `keypoint_scores`
 *   (B capacity) f32, `out_descriptors` (B capacity, C) f32, `counts` (B) int32.  Rows from the total on are not written.
 * Up to six launches of one kernel on the caller's stream, no host synchronisation: (1) scores, a thread per cell; (2) NMS, a
 *   workgroup per tile of gsr_keypoints_tile() squared pixels with its halo of 5 r in LDS, separable pools, masks and suppressed
 *   scores on chip, one 32-bit keep word per tile row out; (3) a scan of the words' counts per image, in row-major order; (4) the
 *   writes, a thread per word; (5) only with k > 0: rank by counting per image; (6) only with C > 0: a wave per keypoint, the five
 *   norms as wave sums.  No atomics, no order that depends on scheduling: the same bits on every call, and an image has the bits in a
 *   batch that it has alone.
 *   `scratch`: gsr_keypoints_scratch_bytes(B, height, width, C, capacity) bytes (host arithmetic; 0 for sizes the call refuses):
 *   the keep words, their offsets and three staging words per row of capacity.
 * GSR_ERR_INVALID_ARGUMENT, nothing launched: another mode, B outside 1 .. 65535, C outside 0 .. 256, capacity < 1, r outside 0 .. 4,
 *   remove_borders < 0, max_num_keypoints < 0, a threshold that is negative or not finite, H or W no multiple of 8 where logits or
 *   descriptors are read, more than 2^31 - 1 elements in an array, a NULL required pointer (logits in the scores mode, scales, and
 *   with C == 0 the three descriptor arguments may be NULL). */
#define GSR_KEYPOINTS_FROM_LOGITS 0
#define GSR_KEYPOINTS_FROM_SCORES 1
int gsr_keypoints_tile(void);
size_t gsr_keypoints_scratch_bytes(int B, int height, int width, int C, int capacity);
int gsr_keypoints(int mode, int B, int height, int width, int C, int nms_radius, float threshold, int remove_borders, int max_num_keypoints,
                  int capacity, const float* logits, float* scores, const float* descriptors, const int64_t* descriptor_strides,
                  const float* scales, void* scratch, float* keypoints, int32_t* pixels, float* keypoint_scores, float* out_descriptors,
                  int32_t* counts, void* stream);

/* The refined poses of the encoder (reference src/model/encoder/encoder_costvolume.py:447-450, 460-473, with r6d2mat :189-209 and
 * matrix_to_rotation_6d :223-224, and the three inversions `refine_sync_abspose.inverse()` :492, :530 and `c2w[1].inverse()`
 * src/model/model_wrapper.py:150) and the per-step pose errors (model_wrapper.py:182-190, 306-313, 345;
 * compute_geodesic_distance_from_two_matrices, src/flow_util.py:20-32).  All arrays f32; b scenes of v >= 1 views; poses are rows of
 * 16 floats, row-major 4 x 4.  One thread per pose (per scene for the errors), fp64 inside the thread, one rounding on store.
 * gsr_pose_refine: sync_pose (b, v, 4, 4), of which the top three rows are read; delta: row (s, i) begins at
 *   delta + (s v + i) delta_row_stride and its first nine floats are read, delta_row_stride >= 9 - the first nine channels of the
 *   pose head's (b, v, 139) output where they lie, no copy, nothing after them is touched; gamma: ONE float in device memory
 *   -> c2w, w2c (b, v, 4, 4).  For pose (s, i):
 *     enc = (row 0 of R, row 1 of R, t) of sync_pose[s, i];  for i >= 1: enc += gamma delta[s, i, 0:9].  VIEW 0 TAKES NO RESIDUAL
 *       (:465-466), whatever its row of delta holds.
 *     a1 = enc[0:3], a2 = enc[3:6], t = enc[6:9];  b1 = a1 / max(|a1|, 1e-12) - THE CLAMP OF F.normalize, not a division by the norm:
 *       a zero row gives a zero row, finite -;  b2 = u / max(|u|, 1e-12), u = a2 - (b1 . a2) b1;  b3 = b1 x b2.
 *     c2w = [[b1; b2; b3] | t], bottom row (0, 0, 0, 1): the b are the ROWS of the rotation, as the reference stacks them.
 *     w2c = [R^T | -R^T t], bottom row (0, 0, 0, 1): THE RIGID INVERSE in place of the reference's batched LU.  c2w is rigid for
 *       every value of delta and gamma (short of the clamp), so the two agree in value and in their gradients with respect to delta
 *       and gamma.
 * gsr_pose_refine_backward: the forward's inputs again (everything is recomputed) and the cotangents dL_dc2w, dL_dw2c (b, v, 4, 4),
 *   either or both NULL (taken as zero; their bottom rows are not read) -> dL_ddelta (b, v, 9), contiguous, FULLY written, the rows of
 *   view 0 zero; dL_dgamma, one float = sum over (s, i >= 1, k) of delta[s, i, k] dL_denc[s, i, k].  An output that is NULL is
 *   skipped.  With dL_dR[i][j] = dL_dc2w[i][j] + dL_dw2c[j][i] - t[i] dL_dw2c[j][3] and dL_dt[i] = dL_dc2w[i][3] - sum_j R[i][j]
 *   dL_dw2c[j][3], back through the cross product, the two normalisations (below the clamp: a division by 1e-12) and the
 *   projection.  One launch of ONE workgroup of 256 threads, which walks the poses with stride 256, keeps an fp64 partial of
 *   dL_dgamma per thread and folds the 256 partials in LDS by a fixed tree: no atomics, the same bits on every run.  sync_pose
 *   receives nothing (the reference's coarse poses come back from numpy).
 * gsr_pose_errors: c2w_pred, extrinsics_gt (b, v, 4, 4) -> out (3, b), forward only, one thread per scene:
 *     gt_rel = extrinsics_gt[s, v - 1]^-1 extrinsics_gt[s, 0], the affine inverse [R^-1 | -R^-1 t] with bottom row (0, 0, 0, 1)
 *       as everywhere in this library;  pred = c2w_pred[s, v - 1];
 *     out[0, s] = acos(clamp((trace(R_pred R_gt^T) - 1) / 2, -1, 1)), RADIANS as the reference logs it;
 *     out[1, s] = acos(clamp(t_pred / |t_pred| . t_gt / |t_gt|, -1, 1)) 180 / pi, degrees;  out[2, s] = |t_pred - t_gt|.
 *   A ZERO TRANSLATION on either side gives NaN in out[1, s], as the reference's 0 / 0 does (the clamp keeps a NaN).
 * All: GSR_ERR_INVALID_ARGUMENT, nothing launched, on a NULL required pointer, b < 0, v < 1, delta_row_stride < 9 or more than
 * 2^31 - 1 elements in the poses or in delta as strided; b == 0: GSR_OK, nothing is launched.  No host synchronisation. */
int gsr_pose_refine(int num_scenes, int num_views, const float* sync_pose, const float* delta, int delta_row_stride, const float* gamma,
                    float* c2w, float* w2c, void* stream);
int gsr_pose_refine_backward(int num_scenes, int num_views, const float* sync_pose, const float* delta, int delta_row_stride,
                             const float* gamma, const float* dL_dc2w, const float* dL_dw2c, float* dL_ddelta, float* dL_dgamma,
                             void* stream);
int gsr_pose_errors(int num_scenes, int num_views, const float* c2w_pred, const float* extrinsics_gt, float* out /* (3, b) */,
                    void* stream);

/* Measurement aid: 1 when gsr_forward runs the colour pass inside the binning launch for these dims (two launches: binning +
 * colour, per-tile sort + blend), 0 when the colour pass is a launch of its own (images of more than 4608 8x8 tiles, more than
 * four views per set, the windowed binning path), negative on bad dims. */
int gsr_colour_in_binning(const GsrDims* dims);

/* Debug aid for tests: the order in which the single view's forward tile launch deals the `count` (1 ... 256) tiles of one XCD to
 * that XCD's workgroups, from what the previous forward left per tile: `walked` entries (tile_total) and `list_length` (ranges).
 * A tile's list_length is end - start of its `ranges` words where those are a range the tile launch writes for that tile (start ==
 * tile x slot and at most a slot long, or longer than a slot and in the tail pool behind tiles x slot), and 0 for any other words.
 * An XCD whose tiles list fewer than 512 keys on average, or with a tile whose words are not what a forward leaves (walked is whole
 * batches of 32 or the whole list, at most the list, and not 0 of a list with entries), keeps heaviest first, every other round of
 * 32 mirrored.
 * order_out[k] = index, inside the XCD's run of tiles, of the tile its k-th workgroup (workgroup 8 k + xcd of the launch) takes.
 * Host code, integer arithmetic: what the device builds.  A permutation of 0 ... count - 1 whatever the words hold. */
int gsr_tile_deal_order(const uint32_t* walked, const uint32_t* list_length, int count, uint32_t* order_out);

/* Debug aid for tests: byte offsets of the sub-buffers inside `bin` (status, counts, tile_total, ranges, keys,
 * point_list) and `img` (final_T, n_contrib), then - NINE entries - `bin`'s tile_order: one uint32 per (view, tile), the tile every
 * workgroup of the tile launch took where the forward deals its tiles by the previous call's walked counts (one view of 257 ... 1024
 * tiles on the fused binning path whose binning launch leaves eight compute units idle; unused by every other call). */
int gsr_workspace_layout(const GsrDims* dims, int64_t* offsets9);
/* The same for `geom`: [0] bytes per projected record (32: x, y, conic a b c, opacity, extra channel, radius bits),
 * [1] offset of the 16-byte footprint words of the windowed binning chain (-1 on the fused path: they never leave registers),
 * [2] offset of the (r, g, b, clamp bits) array, [3] offset of the backward's accumulator rows (-1 without
 * GSR_FLAG_BACKWARD_FOLLOWS). */
int gsr_geom_layout(const GsrDims* dims, int64_t* offsets4);

#ifdef __cplusplus
}
#endif
#endif /* GSR_H_ */
