#pragma once
#include "gsr_common.h"
#include "gsr_pose_loss.h"  // pose_affine_inverse (k_pose_errors)
#include "gsr_attention.h"  // k_match_ops, k_keypoint_ops: the match assignment's and the keypoint extraction's passes are routines of k_pose_ops (the reason is given there)
#include "gsr_image.h"      // k_lpips_ops: so are the perceptual distance's head, its finish and its gradient

// ------------------------------------------------------------------------------------------------
// Refined poses (reference src/model/encoder/encoder_costvolume.py:447-450, 460-473 with r6d2mat :189-209 and matrix_to_rotation_6d
// :223-224, the .inverse() calls of :492, :530 and src/model/model_wrapper.py:150; definition: include/gsr.h) and the per-step pose
// errors (model_wrapper.py:182-190, 306-313, 345; src/flow_util.py:20-32).  One thread per pose, fp64 inside the thread, one
// rounding on store, as the other per-view set-up kernels (pose_affine_inverse, k_cv_*).  k_pose_refine_fwd: the 6D + translation
// encoding of sync_pose, + gamma delta for the views after the first, Gram-Schmidt with F.normalize's clamp, c2w and its RIGID inverse
// w2c = [R^T | -R^T t] (no LU: c2w is rigid for every value of the parameters, so this is torch.inverse and its gradient).
// k_pose_refine_bwd: ONE workgroup of kRefineThreads walks the poses with that stride - back through the inverse, the Gram-Schmidt
// and the residual -, writes dL/ddelta (view 0: zeros) and folds its fp64 partials of dL/dgamma in LDS by a fixed tree: no atomics,
// the same bits on every run.  k_pose_errors: one thread per scene.  The three are device routines of ONE kernel, k_pose_ops<256>,
// which a launch-uniform `op` switches between: the code object's read-only segment in front of .text (metadata note, symbol and
// hash tables, kernel descriptors) had 1920 bytes left in its last page, a kernel costs about 700 there, and three of them moved
// .text - every kernel of the library - by a page, which cost the headline forward 0.5 us in three alternations of three
// (docs/KERNEL_HISTORY.md); one kernel leaves every address where it was.  It is a template (one instance) for the same reason as
// the pose loss's: as an instance it follows every plain kernel and nothing in front of it moves.
// The match assignment's three passes (gsr_attention.h: k_match_ops) are routines of this kernel as well, op kPoseOpMatch, for the same
// reason: there were 512 bytes left.  The routines above are launch-bound and do not feel the registers and LDS those passes take.
// The keypoint extraction's six passes (gsr_attention.h: k_keypoint_ops) are op kPoseOpKeypoints, in the same arena.
// The perceptual distance's head (gsr_image.h: k_lpips_ops) is op kPoseOpLpips: 4 KB of the arena, and the kernel's one workgroup per
// CU with its whole register file is the shape those routines are written for.
// ------------------------------------------------------------------------------------------------
namespace gsr {
constexpr int kRefineThreads = 256;
constexpr double kRefineEps = 1e-12;  // F.normalize's eps: x / max(|x|, eps)

struct RefineArgs {
  int N, V, stride;  // poses (b v), views, floats per row of delta (>= 9)
  const float *sync, *delta, *gamma;
  float *c2w, *w2c;                    // forward
  const float *d_c2w, *d_w2c;          // backward: either may be null
  float *d_delta, *d_gamma;            // either may be null
};

// The encoding of pose n (9 doubles: rows 0 and 1 of R, t), the residual added for a view after the first.
__device__ __forceinline__ void refine_encoding(const RefineArgs& a, int n, double* enc) {
  const float* P = a.sync + (size_t)n * 16;
#pragma unroll
  for (int k = 0; k < 3; ++k) { enc[k] = (double)P[k]; enc[3 + k] = (double)P[4 + k]; enc[6 + k] = (double)P[4 * k + 3]; }
  if (n % a.V != 0) {
    const double g = (double)a.gamma[0];
    const float* d = a.delta + (size_t)n * a.stride;
#pragma unroll
    for (int k = 0; k < 9; ++k) enc[k] += g * (double)d[k];
  }
}

struct RefineFrame {
  double b1[3], b2[3], b3[3], a2[3], n1, n2, a1n, un;  // n = max(norm, eps); a1n, un the norms themselves
};

__device__ __forceinline__ double refine_dot(const double* x, const double* y) { return x[0] * y[0] + x[1] * y[1] + x[2] * y[2]; }
__device__ __forceinline__ void refine_cross(const double* x, const double* y, double* z) {
  z[0] = x[1] * y[2] - x[2] * y[1]; z[1] = x[2] * y[0] - x[0] * y[2]; z[2] = x[0] * y[1] - x[1] * y[0];
}

__device__ __forceinline__ void refine_gram_schmidt(const double* enc, RefineFrame& f) {
  f.a1n = sqrt(refine_dot(enc, enc));
  f.n1 = fmax(f.a1n, kRefineEps);
  double u[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) { f.b1[k] = enc[k] / f.n1; f.a2[k] = enc[3 + k]; }
  const double p = refine_dot(f.b1, f.a2);
#pragma unroll
  for (int k = 0; k < 3; ++k) u[k] = f.a2[k] - p * f.b1[k];
  f.un = sqrt(refine_dot(u, u));
  f.n2 = fmax(f.un, kRefineEps);
#pragma unroll
  for (int k = 0; k < 3; ++k) f.b2[k] = u[k] / f.n2;
  refine_cross(f.b1, f.b2, f.b3);
}

// op kPoseOpRefineFwd: a thread per pose
__device__ __forceinline__ void k_pose_refine_fwd(const RefineArgs& a, int n) {
  if (n >= a.N) return;
  double enc[9];
  refine_encoding(a, n, enc);
  RefineFrame f;
  refine_gram_schmidt(enc, f);
  const double* rows[3] = {f.b1, f.b2, f.b3};
  const double* t = enc + 6;
  float* C = a.c2w + (size_t)n * 16;
  float* W = a.w2c + (size_t)n * 16;
#pragma unroll
  for (int r = 0; r < 3; ++r) {
#pragma unroll
    for (int c = 0; c < 3; ++c) { C[4 * r + c] = (float)rows[r][c]; W[4 * r + c] = (float)rows[c][r]; }
    C[4 * r + 3] = (float)t[r];
    W[4 * r + 3] = (float)(-(f.b1[r] * t[0] + f.b2[r] * t[1] + f.b3[r] * t[2]));
    C[12 + r] = 0.f; W[12 + r] = 0.f;
  }
  C[15] = 1.f; W[15] = 1.f;
}

// d(x / max(|x|, eps)): the projection off the unit vector over the norm; below the clamp the division by eps alone.
__device__ __forceinline__ void refine_normalize_bwd(const double* unit, double norm, double clamped, const double* g, double* out) {
  if (norm > kRefineEps) {
    const double p = refine_dot(unit, g);
#pragma unroll
    for (int k = 0; k < 3; ++k) out[k] = (g[k] - p * unit[k]) / clamped;
  } else {
#pragma unroll
    for (int k = 0; k < 3; ++k) out[k] = g[k] / clamped;
  }
}

// op kPoseOpRefineBwd: ONE workgroup; `part`: kThreads doubles of LDS
template <int kThreads>
__device__ __forceinline__ void k_pose_refine_bwd(const RefineArgs& a, double* part) {
  const int tid = threadIdx.x;
  double sum = 0.0;
  for (int n = tid; n < a.N; n += kThreads) {
    double enc[9], denc[9];
    refine_encoding(a, n, enc);
    RefineFrame f;
    refine_gram_schmidt(enc, f);
    const double* rows[3] = {f.b1, f.b2, f.b3};
    const double* t = enc + 6;
    const float* G = a.d_c2w ? a.d_c2w + (size_t)n * 16 : nullptr;
    const float* Hm = a.d_w2c ? a.d_w2c + (size_t)n * 16 : nullptr;
    // dL/dR[i][j] = G[i][j] + H[j][i] - t[i] H[j][3],  dL/dt[i] = G[i][3] - sum_j R[i][j] H[j][3]
    double dR[3][3], hp[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) hp[j] = Hm ? (double)Hm[4 * j + 3] : 0.0;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
      for (int j = 0; j < 3; ++j) dR[i][j] = (G ? (double)G[4 * i + j] : 0.0) + (Hm ? (double)Hm[4 * j + i] : 0.0) - t[i] * hp[j];
      denc[6 + i] = (G ? (double)G[4 * i + 3] : 0.0) - refine_dot(rows[i], hp);
    }
    double db1[3], db2[3], x[3], du[3];
    refine_cross(f.b2, dR[2], x);  // b3 = b1 x b2
#pragma unroll
    for (int k = 0; k < 3; ++k) db1[k] = dR[0][k] + x[k];
    refine_cross(dR[2], f.b1, x);
#pragma unroll
    for (int k = 0; k < 3; ++k) db2[k] = dR[1][k] + x[k];
    refine_normalize_bwd(f.b2, f.un, f.n2, db2, du);
    const double p = refine_dot(f.b1, f.a2), q = refine_dot(f.b1, du);  // u = a2 - (b1 . a2) b1
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      denc[3 + k] = du[k] - q * f.b1[k];
      db1[k] -= p * du[k] + q * f.a2[k];
    }
    refine_normalize_bwd(f.b1, f.a1n, f.n1, db1, denc);
    const bool first = (n % a.V) == 0;
    const double g = (double)a.gamma[0];
    const float* d = a.delta + (size_t)n * a.stride;
#pragma unroll
    for (int k = 0; k < 9; ++k) {
      if (a.d_delta) a.d_delta[(size_t)n * 9 + k] = first ? 0.f : (float)(g * denc[k]);
      if (!first) sum += (double)d[k] * denc[k];
    }
  }
  part[tid] = sum;
  __syncthreads();
#pragma unroll
  for (int w = kThreads / 2; w >= 1; w >>= 1) {
    if (tid < w) part[tid] += part[tid + w];
    __syncthreads();
  }
  if (tid == 0 && a.d_gamma) a.d_gamma[0] = (float)part[0];
}

struct PoseErrArgs {
  int B, V;
  const float *pred, *gt;
  float* out;
};

__device__ __forceinline__ double refine_clip1(double x) { return x < -1.0 ? -1.0 : (x > 1.0 ? 1.0 : x); }  // (a NaN stays a NaN, as torch.clip's)

// gt_rel = E[s, v - 1]^-1 E[s, 0] (affine inverse, bottom rows (0, 0, 0, 1)); pred = c2w[s, v - 1].  A zero translation on either
// side gives 0 / 0 = NaN in the translation angle, as the reference's division does.
// op kPoseOpErrors: a thread per scene
__device__ __forceinline__ void k_pose_errors(const PoseErrArgs& a, int s) {
  if (s >= a.B) return;
  const float* E0 = a.gt + (size_t)s * a.V * 16;
  const float* P = a.pred + ((size_t)s * a.V + (a.V - 1)) * 16;
  double A[12], Rg[9], tg[3];
  pose_affine_inverse(E0 + (size_t)(a.V - 1) * 16, A);
#pragma unroll
  for (int r = 0; r < 3; ++r) {
#pragma unroll
    for (int c = 0; c < 3; ++c)
      Rg[3 * r + c] = A[4 * r] * (double)E0[c] + A[4 * r + 1] * (double)E0[4 + c] + A[4 * r + 2] * (double)E0[8 + c];
    tg[r] = A[4 * r] * (double)E0[3] + A[4 * r + 1] * (double)E0[7] + A[4 * r + 2] * (double)E0[11] + A[4 * r + 3];
  }
  double trace = 0.0, tp[3], np2 = 0.0, ng2 = 0.0, d2 = 0.0;
#pragma unroll
  for (int r = 0; r < 3; ++r) {
#pragma unroll
    for (int c = 0; c < 3; ++c) trace += (double)P[4 * r + c] * Rg[3 * r + c];  // trace(R_pred R_gt^T)
    tp[r] = (double)P[4 * r + 3];
    np2 += tp[r] * tp[r]; ng2 += tg[r] * tg[r]; d2 += (tp[r] - tg[r]) * (tp[r] - tg[r]);
  }
  const double np = sqrt(np2), ng = sqrt(ng2);
  double cs = 0.0;
#pragma unroll
  for (int r = 0; r < 3; ++r) cs += (tp[r] / np) * (tg[r] / ng);
  a.out[s] = (float)acos(refine_clip1((trace - 1.0) / 2.0));
  a.out[(size_t)a.B + s] = (float)(acos(refine_clip1(cs)) * 180.0 / 3.14159265358979323846);
  a.out[2 * (size_t)a.B + s] = (float)sqrt(d2);
}

// The one kernel of this section: `op` (uniform over the launch) picks the routine.
enum { kPoseOpRefineFwd = 0, kPoseOpRefineBwd = 1, kPoseOpErrors = 2, kPoseOpMatch = 3, kPoseOpKeypoints = 4, kPoseOpLpips = 5 };
struct PoseOpArgs {
  int op;
  RefineArgs r;
  PoseErrArgs e;
  MatchArgs m;  // kPoseOpMatch: the match assignment's pass m.op (gsr_attention.h)
  KeypointArgs k;  // kPoseOpKeypoints: the keypoint extraction's pass k.op (gsr_attention.h)
  LpipsArgs l;     // kPoseOpLpips: the perceptual head's routine l.op (gsr_image.h)
};
static_assert(kLpThreads == kRefineThreads && 4 * kLpThreads <= kMtLdsFloats, "the perceptual head's units are this kernel's workgroups");

template <int kThreads>
__global__ __launch_bounds__(kRefineThreads) void k_pose_ops(const PoseOpArgs a) {
  __shared__ double arena[kMtLdsFloats / 2];  // the match passes' streamed tiles; the refinement's backward folds its kThreads partials in it
  static_assert(kMtLdsFloats % 2 == 0 && kMtLdsFloats / 2 >= kThreads, "the arena holds either use");
  const int item = blockIdx.x * kThreads + threadIdx.x;
  if (a.op == kPoseOpRefineFwd) k_pose_refine_fwd(a.r, item);
  else if (a.op == kPoseOpRefineBwd) k_pose_refine_bwd<kThreads>(a.r, arena);
  else if (a.op == kPoseOpErrors) k_pose_errors(a.e, item);
  else if (a.op == kPoseOpMatch) k_match_ops(a.m, reinterpret_cast<float*>(arena));
  else if (a.op == kPoseOpKeypoints) k_keypoint_ops(a.k, reinterpret_cast<float*>(arena));
  else k_lpips_ops(a.l, reinterpret_cast<float*>(arena));
}

static int match_op_launch(const MatchArgs& m, dim3 grid, void* stream_) {
  PoseOpArgs a{};
  a.op = kPoseOpMatch;
  a.m = m;
  hipLaunchKernelGGL(k_pose_ops<kRefineThreads>, grid, dim3(kRefineThreads), 0, static_cast<hipStream_t>(stream_), a);
  GSR_CHECK(hipGetLastError());
  return GSR_OK;
}

static int keypoint_op_launch(const KeypointArgs& k, dim3 grid, void* stream_) {
  PoseOpArgs a{};
  a.op = kPoseOpKeypoints;
  a.k = k;
  hipLaunchKernelGGL(k_pose_ops<kRefineThreads>, grid, dim3(kRefineThreads), 0, static_cast<hipStream_t>(stream_), a);
  GSR_CHECK(hipGetLastError());
  return GSR_OK;
}

static int lpips_op_launch(const LpipsArgs& l, unsigned blocks, void* stream_) {
  PoseOpArgs a{};
  a.op = kPoseOpLpips;
  a.l = l;
  hipLaunchKernelGGL(k_pose_ops<kRefineThreads>, dim3(blocks), dim3(kRefineThreads), 0, static_cast<hipStream_t>(stream_), a);
  GSR_CHECK(hipGetLastError());
  return GSR_OK;
}

static int pose_op_launch(const PoseOpArgs& a, int blocks, void* stream_) {
  hipLaunchKernelGGL(k_pose_ops<kRefineThreads>, dim3((unsigned)blocks), dim3(kRefineThreads), 0, static_cast<hipStream_t>(stream_), a);
  GSR_CHECK(hipGetLastError());
  return GSR_OK;
}

static bool refine_sizes_ok(int B, int V, int stride) {
  if (B < 0 || V < 1 || stride < 9) return false;
  const int64_t n = (int64_t)B * V;
  return n * 16 <= 0x7fffffffll && n * stride <= 0x7fffffffll;
}

}  // namespace gsr

extern "C" {

int gsr_pose_refine(int num_scenes, int num_views, const float* sync_pose, const float* delta, int delta_row_stride, const float* gamma,
                    float* c2w, float* w2c, void* stream_) {
  using namespace gsr;
  if (!refine_sizes_ok(num_scenes, num_views, delta_row_stride)) return GSR_ERR_INVALID_ARGUMENT;
  if (num_scenes == 0) return GSR_OK;
  if (!sync_pose || !delta || !gamma || !c2w || !w2c) return GSR_ERR_INVALID_ARGUMENT;
  PoseOpArgs op{};
  op.op = kPoseOpRefineFwd;
  RefineArgs& a = op.r;
  a.N = num_scenes * num_views; a.V = num_views; a.stride = delta_row_stride;
  a.sync = sync_pose; a.delta = delta; a.gamma = gamma; a.c2w = c2w; a.w2c = w2c;
  return pose_op_launch(op, (a.N + kRefineThreads - 1) / kRefineThreads, stream_);
}

int gsr_pose_refine_backward(int num_scenes, int num_views, const float* sync_pose, const float* delta, int delta_row_stride,
                             const float* gamma, const float* dL_dc2w, const float* dL_dw2c, float* dL_ddelta, float* dL_dgamma,
                             void* stream_) {
  using namespace gsr;
  if (!refine_sizes_ok(num_scenes, num_views, delta_row_stride)) return GSR_ERR_INVALID_ARGUMENT;
  if (num_scenes == 0) return GSR_OK;
  if (!sync_pose || !delta || !gamma) return GSR_ERR_INVALID_ARGUMENT;
  if (!dL_ddelta && !dL_dgamma) return GSR_OK;
  PoseOpArgs op{};
  op.op = kPoseOpRefineBwd;
  RefineArgs& a = op.r;
  a.N = num_scenes * num_views; a.V = num_views; a.stride = delta_row_stride;
  a.sync = sync_pose; a.delta = delta; a.gamma = gamma; a.d_c2w = dL_dc2w; a.d_w2c = dL_dw2c; a.d_delta = dL_ddelta; a.d_gamma = dL_dgamma;
  return pose_op_launch(op, 1, stream_);
}

int gsr_pose_errors(int num_scenes, int num_views, const float* c2w_pred, const float* extrinsics_gt, float* out, void* stream_) {
  using namespace gsr;
  if (!refine_sizes_ok(num_scenes, num_views, 9)) return GSR_ERR_INVALID_ARGUMENT;
  if (num_scenes == 0) return GSR_OK;
  if (!c2w_pred || !extrinsics_gt || !out) return GSR_ERR_INVALID_ARGUMENT;
  PoseOpArgs op{};
  op.op = kPoseOpErrors;
  op.e = PoseErrArgs{num_scenes, num_views, c2w_pred, extrinsics_gt, out};
  return pose_op_launch(op, (num_scenes + kRefineThreads - 1) / kRefineThreads, stream_);
}

}  // extern "C"
