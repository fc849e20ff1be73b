#pragma once
#include "gsr_common.h"
#include "gsr_pose_loss.h"

// ------------------------------------------------------------------------------------------------
// Plane-sweep cost volume (reference src/model/encoder/costvolume/depth_predictor_multiview.py:28-141, 321-343; definition:
// include/gsr.h): cost[(i s), d, p] = 1 / ((v - 1) sqrt(c)) sum_k f_i[:, p] . bilinear(f_j, proj_k(p, depth_d)).  The warped features
// (v b, c, D, h, w) never exist: a wave takes one pixel p of one row (i, s), walks the candidates and reads each tap as ONE contiguous
// channel row of a channels-last staging copy of the features, (b, v, h, w, Cp) floats, Cp = c rounded up to 4 and the pad zero
// (k_cv_transpose<0>; a row is 1 KB at c = 256 and every float4 of it aligned).  Set-up per (row, other view), every thread, fp64,
// uniform loads: P = E_j^-1 E_i (affine inverse), M = K R_P K^-1, K t_P; per pixel a = M (x, y, 1) in fp64; per sample
// q = depth a + K t in fp32 and two divisions.  The 64 lanes form px, py of 64 candidates at once; the walk then takes one candidate
// at a time with readlane, so px, py, the inside test and the tap addresses are scalars and every branch on them is uniform.
// A tap is inside by a comparison of FLOATS (NaN and +-inf compare false); only an inside tap is converted to an integer.
// Forward: workgroup = 16 consecutive pixels of one row, wave w pixels w, w + 4, ...; lane l holds float4 l of a 256-channel pass
// (the first pass's reference feature stays in registers); 64 candidates x 16 pixels go through LDS to leave as 64-byte segments.
// Backward: one launch over the same walk with channel = pass + 64 m + lane (every atomic instruction adds 256 contiguous bytes of a
// row).  dL/df_i[:, p] = sum_k sum_d G[d, p] warp: registers, one row add at the end.  dL/df_j is the scatter: the contribution of a
// tap is (G[d, p] weight) f_i[:, p] - a SCALAR times a row that is fixed for the walk - so the four scalars of consecutive candidates
// with the same base pixel are summed in scalar registers and a row leaves the CU only when the walk moves on to another base
// pixel.  Both go with float atomics into a zero-filled channels-last gradient (b, v, h, w, Cp), which k_cv_transpose<1> returns
// as (b, v, c, h, w).  Templates for the code object's layout alone, as the pose loss above.
// ------------------------------------------------------------------------------------------------
namespace gsr {
constexpr int kCvPix = 16;       // pixels of a forward workgroup
constexpr int kCvPass = 256;     // channels of one pass of a wave
constexpr float kCvMinZ = 1e-3f;  // the reference's clamp_min_depth

struct CostVolArgs {
  int B, V, C, Cp, H, W, D;
  const float *feat, *intr, *extr, *near, *far;
  float* fcl;      // (B, V, H, W, Cp) channels-last features
  float* cost;     // forward: (V B, D, H, W)
  const float* g;  // backward: dL/dcost
  float* gcl;      // backward: (B, V, H, W, Cp) channels-last gradient, zero-filled
  float* d_feat;   // backward: (B, V, C, H, W)
  float scale;     // 1 / ((V - 1) sqrt(C))
};

// kDir 0: features (img, C, HW) -> fcl (img, HW, Cp), pad channels zero; kDir 1: gcl (img, HW, Cp) -> d_feat (img, C, HW).
template <int kDir>
__global__ __launch_bounds__(256) void k_cv_transpose(const CostVolArgs a) {
  __shared__ float tile[32][33];
  const int HW = a.H * a.W, tpx = (HW + 31) / 32, tch = (a.Cp + 31) / 32;
  unsigned bid = blockIdx.x;
  const int p0 = (int)(bid % (unsigned)tpx) * 32;
  bid /= (unsigned)tpx;
  const int c0 = (int)(bid % (unsigned)tch) * 32;
  const size_t img = bid / (unsigned)tch;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  if (kDir == 0) {
    const float* src = a.feat + img * (size_t)a.C * HW;
    for (int r = ty; r < 32; r += 8) tile[r][tx] = (c0 + r < a.C && p0 + tx < HW) ? src[(size_t)(c0 + r) * HW + p0 + tx] : 0.f;
    __syncthreads();
    float* dst = a.fcl + img * (size_t)HW * a.Cp;
    for (int r = ty; r < 32; r += 8)
      if (p0 + r < HW && c0 + tx < a.Cp) dst[(size_t)(p0 + r) * a.Cp + c0 + tx] = tile[tx][r];
  } else {
    const float* src = a.gcl + img * (size_t)HW * a.Cp;
    for (int r = ty; r < 32; r += 8) tile[r][tx] = (p0 + r < HW && c0 + tx < a.C) ? src[(size_t)(p0 + r) * a.Cp + c0 + tx] : 0.f;
    __syncthreads();
    float* dst = a.d_feat + img * (size_t)a.C * HW;
    for (int r = ty; r < 32; r += 8)
      if (c0 + r < a.C && p0 + tx < HW) dst[(size_t)(c0 + r) * HW + p0 + tx] = tile[tx][r];
  }
}

// torch.linspace(0, 1, D) in float32: from the start below the middle, from the end above it.
__device__ __forceinline__ float cv_lin(int d, int D) {
  if (D < 2) return 0.f;
  const float step = 1.f / (float)(D - 1);
  return d < D / 2 ? (float)d * step : 1.f - (float)(D - 1 - d) * step;
}

// The candidate depth of a lane: 1 / (1 / far + lin (1 / near - 1 / far)), fp64 from the float32 bounds and lin.
__device__ __forceinline__ float cv_depth(const CostVolArgs& a, size_t cam, int d) {
  const double dmin = 1.0 / (double)a.far[cam], dmax = 1.0 / (double)a.near[cam];
  return (float)(1.0 / (dmin + (double)cv_lin(d, a.D) * (dmax - dmin)));
}

// M = K R_P K^-1 and K t_P of row (i, s) against view j, P = E_j^-1 E_i, K = intrinsics[s, i] with row 0 x W, row 1 x H; fp64, uniform.
__device__ __forceinline__ void cv_setup(const CostVolArgs& a, int s, int i, int j, double* M, double* kt) {
  const float* Ei = a.extr + ((size_t)s * a.V + i) * 16;
  double A[12], R[9], t[3], K[9], Ki[9], KR[9];
  pose_affine_inverse(a.extr + ((size_t)s * a.V + j) * 16, A);
#pragma unroll
  for (int r = 0; r < 3; ++r) {
#pragma unroll
    for (int c = 0; c < 3; ++c) R[3 * r + c] = A[4 * r] * (double)Ei[c] + A[4 * r + 1] * (double)Ei[4 + c] + A[4 * r + 2] * (double)Ei[8 + c];
    t[r] = A[4 * r] * (double)Ei[3] + A[4 * r + 1] * (double)Ei[7] + A[4 * r + 2] * (double)Ei[11] + A[4 * r + 3];
  }
  const float* Kn = a.intr + ((size_t)s * a.V + i) * 9;
#pragma unroll
  for (int c = 0; c < 3; ++c) { K[c] = (double)Kn[c] * (double)a.W; K[3 + c] = (double)Kn[3 + c] * (double)a.H; K[6 + c] = (double)Kn[6 + c]; }
  pose_inv3(K, Ki);
#pragma unroll
  for (int r = 0; r < 3; ++r) {
#pragma unroll
    for (int c = 0; c < 3; ++c) KR[3 * r + c] = K[3 * r] * R[c] + K[3 * r + 1] * R[3 + c] + K[3 * r + 2] * R[6 + c];
    kt[r] = K[3 * r] * t[0] + K[3 * r + 1] * t[1] + K[3 * r + 2] * t[2];
  }
#pragma unroll
  for (int r = 0; r < 3; ++r) {
#pragma unroll
    for (int c = 0; c < 3; ++c) M[3 * r + c] = KR[3 * r] * Ki[c] + KR[3 * r + 1] * Ki[3 + c] + KR[3 * r + 2] * Ki[6 + c];
  }
}

// This lane's sample position for pixel (x, y): q = depth M (x, y, 1) + K t; px = q_x / max(q_z, 1e-3), py likewise.
__device__ __forceinline__ void cv_project(const double* M, const double* kt, int x, int y, float depth, float& px, float& py) {
  const float ax = (float)(M[0] * (double)x + M[1] * (double)y + M[2]), ay = (float)(M[3] * (double)x + M[4] * (double)y + M[5]);
  const float az = (float)(M[6] * (double)x + M[7] * (double)y + M[8]);
  const float qx = depth * ax + (float)kt[0], qy = depth * ay + (float)kt[1], qz = depth * az + (float)kt[2];
  const float z = fmaxf(qz, kCvMinZ);  // (a NaN q_z gives the clamp: the sample then lands wherever q_x / 1e-3 does)
  px = qx / z;
  py = qy / z;
}

// The four taps of a sample (x0 y0, x1 y0, x0 y1, x1 y1): weights, and the pixel index y W + x of the taps that are inside; -1 outside.
struct CvTaps {
  float w[4];
  int at[4];
};

// false: no tap inside (nothing may be read or added).  The comparisons are on floats - false for NaN, true for no value outside
// [0, W - 1] x [0, H - 1] - and only what passed them is converted: x0 in [-1, W - 1], y0 in [-1, H - 1].
__device__ __forceinline__ bool cv_taps(float px, float py, int W, int H, CvTaps& t) {
  const float x0 = floorf(px), y0 = floorf(py), x1 = x0 + 1.f, y1 = y0 + 1.f;
  const float wm1 = (float)(W - 1), hm1 = (float)(H - 1);
  const bool ix0 = x0 >= 0.f && x0 <= wm1, ix1 = x1 >= 0.f && x1 <= wm1, iy0 = y0 >= 0.f && y0 <= hm1, iy1 = y1 >= 0.f && y1 <= hm1;
  if (!((ix0 || ix1) && (iy0 || iy1))) return false;
  const int xi = ix0 ? (int)x0 : -1, yi = iy0 ? (int)y0 : -1;  // (an x0 that is not inside while x1 is, is -1)
  const float wx1 = px - x0, wx0 = x1 - px, wy1 = py - y0, wy0 = y1 - py;
  t.w[0] = wx0 * wy0; t.w[1] = wx1 * wy0; t.w[2] = wx0 * wy1; t.w[3] = wx1 * wy1;
  t.at[0] = (ix0 && iy0) ? yi * W + xi : -1;
  t.at[1] = (ix1 && iy0) ? yi * W + xi + 1 : -1;
  t.at[2] = (ix0 && iy1) ? (yi + 1) * W + xi : -1;
  t.at[3] = (ix1 && iy1) ? (yi + 1) * W + xi + 1 : -1;
  return true;
}

__device__ __forceinline__ float cv_lane_value(float v, int lane) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane)); }

template <int kUnit>
__global__ __launch_bounds__(256) void k_cost_volume_fwd(const CostVolArgs a) {
  __shared__ float tile[64][kCvPix + 1];
  const int HW = a.H * a.W, groups = (HW + kCvPix - 1) / kCvPix;
  const int row = (int)(blockIdx.x / (unsigned)groups), p0 = (int)(blockIdx.x - (unsigned)row * (unsigned)groups) * kCvPix;
  const int i = row / a.B, s = row - i * a.B;
  const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const size_t cam = (size_t)s * a.V + i;
  const float* fi = a.fcl + cam * (size_t)HW * a.Cp;
  const int c4 = lane * 4;
  for (int d0 = 0; d0 < a.D; d0 += 64) {
    const int nd = min(64, a.D - d0);
    const float depth = cv_depth(a, cam, min(d0 + lane, a.D - 1));
    float res[kCvPix / 4];
#pragma unroll
    for (int q = 0; q < kCvPix / 4; ++q) res[q] = 0.f;
    for (int k = 1; k < a.V; ++k) {
      const int j = (i + k) % a.V;
      double M[9], kt[3];
      cv_setup(a, s, i, j, M, kt);
      const float* fj = a.fcl + ((size_t)s * a.V + j) * (size_t)HW * a.Cp;
#pragma unroll
      for (int q = 0; q < kCvPix / 4; ++q) {
        const int p = p0 + wv + 4 * q;
        if (p >= HW) continue;  // (uniform over the wave)
        const int y = p / a.W, x = p - y * a.W;
        float px, py;
        cv_project(M, kt, x, y, depth, px, py);
        const float* ref = fi + (size_t)p * a.Cp;
        const float4 ref0 = c4 < a.Cp ? *reinterpret_cast<const float4*>(ref + c4) : make_float4(0.f, 0.f, 0.f, 0.f);
        for (int dd = 0; dd < nd; ++dd) {
          CvTaps t;
          if (!cv_taps(cv_lane_value(px, dd), cv_lane_value(py, dd), a.W, a.H, t)) continue;  // (scalars: uniform)
          float part = 0.f;
          for (int c = c4; c < a.Cp; c += kCvPass) {
            const float4 r = c == c4 ? ref0 : *reinterpret_cast<const float4*>(ref + c);
            float4 w = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
            for (int n = 0; n < 4; ++n) {
              if (t.at[n] < 0) continue;
              const float4 f = *reinterpret_cast<const float4*>(fj + (size_t)t.at[n] * a.Cp + c);
              w.x += t.w[n] * f.x; w.y += t.w[n] * f.y; w.z += t.w[n] * f.z; w.w += t.w[n] * f.w;
            }
            part += r.x * w.x + r.y * w.y + r.z * w.z + r.w * w.w;
          }
          part = wave_sum(part);
          if (lane == dd) res[q] += part;
        }
      }
    }
#pragma unroll
    for (int q = 0; q < kCvPix / 4; ++q) tile[lane][wv + 4 * q] = res[q] * a.scale;
    __syncthreads();
    for (int e = tid; e < 64 * kCvPix; e += 256) {
      const int dd = e / kCvPix, pp = e - dd * kCvPix;
      if (dd < nd && p0 + pp < HW) a.cost[((size_t)row * a.D + d0 + dd) * HW + p0 + pp] = tile[dd][pp];
    }
    __syncthreads();
  }
}

// Adds coef[n] x ref[m] to the channel rows of the (up to four) taps of base pixel `at`; channel c0 + 64 m + lane.
__device__ __forceinline__ void cv_flush(float* gj, const int* at, float* coef, const float* ref, int c0, int lane, int C, int Cp) {
#pragma unroll
  for (int n = 0; n < 4; ++n) {
    if (at[n] >= 0 && coef[n] != 0.f) {  // (scalars: uniform)
      float* rowp = gj + (size_t)at[n] * Cp + c0 + lane;
#pragma unroll
      for (int m = 0; m < 4; ++m)
        if (c0 + 64 * m + lane < C) unsafeAtomicAdd(rowp + 64 * m, coef[n] * ref[m]);
    }
    coef[n] = 0.f;
  }
}

template <int kUnit>
__global__ __launch_bounds__(256) void k_cost_volume_bwd(const CostVolArgs a) {
  const int HW = a.H * a.W, groups = (HW + 3) / 4;
  const int row = (int)(blockIdx.x / (unsigned)groups);
  const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int p = (int)(blockIdx.x - (unsigned)row * (unsigned)groups) * 4 + wv;
  if (p >= HW) return;  // (uniform over the wave; no barrier below)
  const int i = row / a.B, s = row - i * a.B;
  const size_t cam = (size_t)s * a.V + i;
  const int y = p / a.W, x = p - y * a.W;
  const float* ref_row = a.fcl + (cam * (size_t)HW + p) * a.Cp;
  float* gi = a.gcl + (cam * (size_t)HW + p) * a.Cp;
  for (int c0 = 0; c0 < a.C; c0 += kCvPass) {
    float ref[4], acc[4];
#pragma unroll
    for (int m = 0; m < 4; ++m) { ref[m] = c0 + 64 * m + lane < a.C ? ref_row[c0 + 64 * m + lane] : 0.f; acc[m] = 0.f; }
    for (int k = 1; k < a.V; ++k) {
      const int j = (i + k) % a.V;
      double M[9], kt[3];
      cv_setup(a, s, i, j, M, kt);
      const float* fj = a.fcl + ((size_t)s * a.V + j) * (size_t)HW * a.Cp;
      float* gj = a.gcl + ((size_t)s * a.V + j) * (size_t)HW * a.Cp;
      int cur[4] = {-1, -1, -1, -1};
      float coef[4] = {0.f, 0.f, 0.f, 0.f};
      for (int d0 = 0; d0 < a.D; d0 += 64) {
        const int nd = min(64, a.D - d0);
        const int d = min(d0 + lane, a.D - 1);
        float px, py;
        cv_project(M, kt, x, y, cv_depth(a, cam, d), px, py);
        const float gl = a.g[((size_t)row * a.D + d) * HW + p] * a.scale;
        for (int dd = 0; dd < nd; ++dd) {
          CvTaps t;
          if (!cv_taps(cv_lane_value(px, dd), cv_lane_value(py, dd), a.W, a.H, t)) continue;  // (scalars: uniform)
          const float g = cv_lane_value(gl, dd);
          if (t.at[0] != cur[0] || t.at[1] != cur[1] || t.at[2] != cur[2] || t.at[3] != cur[3]) {
            cv_flush(gj, cur, coef, ref, c0, lane, a.C, a.Cp);
#pragma unroll
            for (int n = 0; n < 4; ++n) cur[n] = t.at[n];
          }
#pragma unroll
          for (int n = 0; n < 4; ++n) {
            if (t.at[n] < 0) continue;
            const float gw = g * t.w[n];
            coef[n] += gw;
            const float* src = fj + (size_t)t.at[n] * a.Cp + c0 + lane;
#pragma unroll
            for (int m = 0; m < 4; ++m)
              if (c0 + 64 * m + lane < a.C) acc[m] += gw * src[64 * m];
          }
        }
      }
      cv_flush(gj, cur, coef, ref, c0, lane, a.C, a.Cp);
    }
#pragma unroll
    for (int m = 0; m < 4; ++m)
      if (c0 + 64 * m + lane < a.C) unsafeAtomicAdd(gi + c0 + 64 * m + lane, acc[m]);
  }
}

// The checks of the three entry points: 0 when the sizes are in range, and Cp.
static bool cv_sizes_ok(int B, int V, int C, int H, int W, int D, int64_t* cp) {
  if (B < 0 || V < 2 || C < 1 || H < 2 || W < 2 || D < 1) return false;
  const int64_t Cp = ((int64_t)C + 3) / 4 * 4, lim = 0x7fffffff;
  const int64_t rows = (int64_t)B * V, hw = (int64_t)H * W;
  if (rows > lim || hw > lim || rows * hw > lim || rows * hw * Cp > lim || rows * hw * (int64_t)D > lim) return false;
  *cp = Cp;
  return true;
}
}  // namespace gsr

extern "C" {

size_t gsr_cost_volume_scratch_bytes(int num_scenes, int num_views, int channels, int height, int width, int backward) {
  int64_t cp;
  if (!gsr::cv_sizes_ok(num_scenes, num_views, channels, height, width, 1, &cp)) return 0;
  return (size_t)num_scenes * num_views * height * width * (size_t)cp * sizeof(float) * (backward ? 2 : 1);
}

int gsr_cost_volume(int num_scenes, int num_views, int channels, int height, int width, int num_depth_candidates, const float* features,
                    const float* intrinsics, const float* extrinsics, const float* near, const float* far, float* cost, void* scratch,
                    void* stream_) {
  using namespace gsr;
  int64_t cp;
  if (!cv_sizes_ok(num_scenes, num_views, channels, height, width, num_depth_candidates, &cp)) return GSR_ERR_INVALID_ARGUMENT;
  if (!features || !intrinsics || !extrinsics || !near || !far || !cost || !scratch) return GSR_ERR_INVALID_ARGUMENT;
  if (num_scenes == 0) return GSR_OK;
  hipStream_t st = static_cast<hipStream_t>(stream_);
  CostVolArgs a{};
  a.B = num_scenes; a.V = num_views; a.C = channels; a.Cp = (int)cp; a.H = height; a.W = width; a.D = num_depth_candidates;
  a.feat = features; a.intr = intrinsics; a.extr = extrinsics; a.near = near; a.far = far;
  a.fcl = static_cast<float*>(scratch); a.cost = cost;
  a.scale = (float)(1.0 / ((double)(num_views - 1) * sqrt((double)channels)));
  const int64_t hw = (int64_t)height * width, rows = (int64_t)num_scenes * num_views;
  const int64_t tblocks = (hw + 31) / 32 * ((cp + 31) / 32) * rows, blocks = (hw + kCvPix - 1) / kCvPix * rows;
  hipLaunchKernelGGL(k_cv_transpose<0>, dim3((unsigned)tblocks), dim3(256), 0, st, a);
  GSR_CHECK(hipGetLastError());
  hipLaunchKernelGGL(k_cost_volume_fwd<kCvPix>, dim3((unsigned)blocks), dim3(256), 0, st, a);
  GSR_CHECK(hipGetLastError());
  return GSR_OK;
}

int gsr_cost_volume_backward(int num_scenes, int num_views, int channels, int height, int width, int num_depth_candidates,
                             const float* features, const float* intrinsics, const float* extrinsics, const float* near, const float* far,
                             const float* dL_dcost, float* dL_dfeatures, void* scratch, void* stream_) {
  using namespace gsr;
  int64_t cp;
  if (!cv_sizes_ok(num_scenes, num_views, channels, height, width, num_depth_candidates, &cp)) return GSR_ERR_INVALID_ARGUMENT;
  if (!features || !intrinsics || !extrinsics || !near || !far || !dL_dcost || !dL_dfeatures || !scratch) return GSR_ERR_INVALID_ARGUMENT;
  if (num_scenes == 0) return GSR_OK;
  hipStream_t st = static_cast<hipStream_t>(stream_);
  const int64_t hw = (int64_t)height * width, rows = (int64_t)num_scenes * num_views;
  const size_t floats = (size_t)(rows * hw * cp);
  CostVolArgs a{};
  a.B = num_scenes; a.V = num_views; a.C = channels; a.Cp = (int)cp; a.H = height; a.W = width; a.D = num_depth_candidates;
  a.feat = features; a.intr = intrinsics; a.extr = extrinsics; a.near = near; a.far = far;
  a.fcl = static_cast<float*>(scratch); a.gcl = a.fcl + floats; a.g = dL_dcost; a.d_feat = dL_dfeatures;
  a.scale = (float)(1.0 / ((double)(num_views - 1) * sqrt((double)channels)));
  const int64_t tblocks = (hw + 31) / 32 * ((cp + 31) / 32) * rows, blocks = (hw + 3) / 4 * rows;
  GSR_CHECK(hipMemsetAsync(a.gcl, 0, floats * sizeof(float), st));
  hipLaunchKernelGGL(k_cv_transpose<0>, dim3((unsigned)tblocks), dim3(256), 0, st, a);
  GSR_CHECK(hipGetLastError());
  hipLaunchKernelGGL(k_cost_volume_bwd<kCvPix>, dim3((unsigned)blocks), dim3(256), 0, st, a);
  GSR_CHECK(hipGetLastError());
  hipLaunchKernelGGL(k_cv_transpose<1>, dim3((unsigned)tblocks), dim3(256), 0, st, a);
  GSR_CHECK(hipGetLastError());
  return GSR_OK;
}

}  // extern "C"

// ------------------------------------------------------------------------------------------------
// Depth lift (reference src/model/encoder/encoder_costvolume.py:265, 287-307, 506, 525-528; definition: include/gsr.h): the mono-depth
// network's output -> the refined depth, the per-pixel points and the one-hot mono cue, one launch; and the Pluecker ray map
// (:211-221, 387-392).  They live in this header because the cue is the cost volume's neighbour in the depth predictor's input: it
// shares the volume's (v b) row order, its candidates (cv_lin) and the fp64 3 x 3 inverse this header already includes.
// One grid, two kinds of workgroup, told apart by blockIdx (uniform):
//   cue   - 64 consecutive quarter-resolution pixels of one image.  Wave 0 forms `down`, torch's bilinear resize, from taps that are
//           recomputed from depth_raw and shift (the `depth` output is never read back: no ordering inside the launch); thread
//           (part, q) scans a quarter of the candidates for pixel q - a full first-minimum scan, strict <, so ties go to the lowest
//           channel and a NaN or an infinite `down` leaves channel 0 -; the four parts are merged in ascending order.  Then the
//           workgroup writes its 64-pixel segment of every channel row once: a lane holds four pixels' channels and stores
//           float4(ch == d), a wave instruction four rows x 256 contiguous bytes.  No zero-fill, no scatter, no volume but the output.
//   full  - 1024 consecutive pixels of one image, four per thread (float4 where h w is a multiple of 4 and the arrays are 16-byte
//           aligned): depth = clamp(clamp(raw) + shift), one fp32 rounding; the ray K^-1 (u, v, 1) is affine in (x, y) with fp64
//           coefficients formed once per thread from the full fp64 inverse, rounded once to fp32 and multiplied by the depth.
// Backward: the full partition again; m1, m2 and the ray are recomputed.  The intrinsics gradient, on request, is G = sum_p g_xyz
// (u, v, 1)^T depth per image: fp64 per thread, xor tree per wave, waves in order -> 9 doubles per workgroup in the caller's scratch;
// a finishing launch adds an image's workgroups in order and forms -K^-T G K^-T.  No atomics: the same bits on every run.
// ------------------------------------------------------------------------------------------------
namespace gsr {
constexpr int kLiftPix = 1024;  // full-resolution pixels of a workgroup
constexpr int kLiftQ = 64;      // quarter-resolution pixels of a cue workgroup

struct LiftArgs {
  int B, V, H, W, D, Hq, Wq;
  int full_chunks, cue_chunks;  // workgroups per image of each kind
  int vec_full, vec_cue;        // float4 accesses are aligned
  const float *raw, *shift, *near, *far, *intr, *lin;
  float *depth, *xyz, *cue;
  const float *g_depth, *g_xyz;  // backward
  float *d_raw, *d_shift, *d_intr;
  double* partials;  // (images, full_chunks, 9)
};

// torch's clamp(x, lo, hi) = min(max(x, lo), hi) as comparisons: a NaN x fails both and stays.
__device__ __forceinline__ float lift_clamp(float x, float lo, float hi) {
  const float t = x < lo ? lo : x;
  return hi < t ? hi : t;
}

// The refined depth of one pixel; m1, m2: whether the first and the second clamp pass a gradient (inclusive at the bounds).
__device__ __forceinline__ float lift_depth_of(float raw, float shift, float lo, float hi, bool& m1, bool& m2) {
  const float t = lift_clamp(raw, lo, hi) + shift;
  m1 = raw >= lo && raw <= hi;
  m2 = t >= lo && t <= hi;
  return lift_clamp(t, lo, hi);
}

// K^-1 of one image in fp64 (all nine entries, by cofactors) and the ray of pixel (x, y)'s centre as an affine map:
// ray_c = R[3 c] x + R[3 c + 1] y + R[3 c + 2].
__device__ __forceinline__ void lift_rays(const float* Kn, int W, int H, double* Ki, double* R) {
  double K[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) K[k] = (double)Kn[k];
  pose_inv3(K, Ki);
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    R[3 * c] = Ki[3 * c] / (double)W;
    R[3 * c + 1] = Ki[3 * c + 1] / (double)H;
    R[3 * c + 2] = 0.5 * R[3 * c] + 0.5 * R[3 * c + 1] + Ki[3 * c + 2];
  }
}

// One axis of torch's bilinear resize (align_corners = False): the two source indices and the weight of the second.
__device__ __forceinline__ void lift_resize_axis(int dst, int in, int out, int& i0, int& i1, float& l1) {
  const float scale = (float)in / (float)out;
  float src = scale * ((float)dst + 0.5f) - 0.5f;
  src = src < 0.f ? 0.f : src;
  i0 = min((int)src, in - 1);
  i1 = i0 + (i0 < in - 1 ? 1 : 0);
  l1 = src - (float)i0;
}

__device__ __forceinline__ void lift_cue_block(const LiftArgs& a, int blk) {
  __shared__ float down_s[kLiftQ];
  __shared__ float best_v[4][kLiftQ];
  __shared__ int best_i[4][kLiftQ];
  const int Q = a.Hq * a.Wq;
  const int img = blk / a.cue_chunks, q0 = (blk - img * a.cue_chunks) * kLiftQ;
  const int s = img / a.V, i = img - s * a.V;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int q = q0 + lane;
  if (wv == 0) {
    float down = 0.f;
    if (q < Q) {
      const int qy = q / a.Wq, qx = q - qy * a.Wq;
      int x0, x1, y0, y1;
      float lx, ly;
      lift_resize_axis(qx, a.W, a.Wq, x0, x1, lx);
      lift_resize_axis(qy, a.H, a.Hq, y0, y1, ly);
      const float lo = a.near[img], hi = a.far[img];
      const size_t base = (size_t)img * a.H * a.W;
      const size_t r0 = base + (size_t)y0 * a.W, r1 = base + (size_t)y1 * a.W;
      bool m1, m2;
      const float v00 = lift_depth_of(a.raw[r0 + x0], a.shift[r0 + x0], lo, hi, m1, m2);
      const float v01 = lift_depth_of(a.raw[r0 + x1], a.shift[r0 + x1], lo, hi, m1, m2);
      const float v10 = lift_depth_of(a.raw[r1 + x0], a.shift[r1 + x0], lo, hi, m1, m2);
      const float v11 = lift_depth_of(a.raw[r1 + x1], a.shift[r1 + x1], lo, hi, m1, m2);
      down = (1.f - ly) * ((1.f - lx) * v00 + lx * v01) + ly * ((1.f - lx) * v10 + lx * v11);
    }
    down_s[lane] = down;
  }
  __syncthreads();
  {  // the scan of candidates [wv per, (wv + 1) per) for pixel `lane`: the hypotheses of scene 0, view 0, INVERSE depths against a depth
    const float lo_h = 1.f / a.far[0], step = 1.f / a.near[0] - lo_h;
    const float down = down_s[lane];
    const int per = (a.D + 3) / 4, d_end = min(a.D, (wv + 1) * per);
    float best = INFINITY;
    int at = 0;
    for (int d = wv * per; d < d_end; ++d) {
      const float lin = a.lin ? a.lin[d] : cv_lin(d, a.D);
      const float diff = fabsf(down - (lo_h + lin * step));
      if (diff < best) { best = diff; at = d; }
    }
    best_v[wv][lane] = best;
    best_i[wv][lane] = at;
  }
  __syncthreads();
  const size_t row = (size_t)i * a.B + s;  // view-major, as the cost volume's rows
  float* out = a.cue + row * (size_t)a.D * Q;
  if (a.vec_cue) {  // (Q is a multiple of 4: a float4 is inside the image or outside it)
    const int qq = (lane & 15) * 4;
    int ch[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      float best = best_v[0][qq + k];
      ch[k] = best_i[0][qq + k];
#pragma unroll
      for (int part = 1; part < 4; ++part)
        if (best_v[part][qq + k] < best) { best = best_v[part][qq + k]; ch[k] = best_i[part][qq + k]; }
    }
    if (q0 + qq < Q)
      for (int d = wv * 4 + (lane >> 4); d < a.D; d += 16)
        *reinterpret_cast<float4*>(out + (size_t)d * Q + q0 + qq) =
            make_float4(ch[0] == d ? 1.f : 0.f, ch[1] == d ? 1.f : 0.f, ch[2] == d ? 1.f : 0.f, ch[3] == d ? 1.f : 0.f);
  } else {
    float best = best_v[0][lane];
    int ch = best_i[0][lane];
#pragma unroll
    for (int part = 1; part < 4; ++part)
      if (best_v[part][lane] < best) { best = best_v[part][lane]; ch = best_i[part][lane]; }
    if (q < Q)
      for (int d = wv; d < a.D; d += 4) out[(size_t)d * Q + q] = ch == d ? 1.f : 0.f;
  }
}

__device__ __forceinline__ void lift_full_block(const LiftArgs& a, int blk) {
  const int HW = a.H * a.W;
  const int img = blk / a.full_chunks, p0 = (blk - img * a.full_chunks) * kLiftPix + (int)threadIdx.x * 4;
  if (p0 >= HW) return;
  const int n = min(4, HW - p0);
  double Ki[9], R[9];
  lift_rays(a.intr + (size_t)img * 9, a.W, a.H, Ki, R);
  const float lo = a.near[img], hi = a.far[img];
  const size_t at = (size_t)img * HW + p0, at3 = (size_t)img * 3 * HW + p0;
  float raw[4] = {0.f, 0.f, 0.f, 0.f}, sh[4] = {0.f, 0.f, 0.f, 0.f}, dep[4], pt[3][4];
  if (a.vec_full) {
    const float4 r4 = *reinterpret_cast<const float4*>(a.raw + at), s4 = *reinterpret_cast<const float4*>(a.shift + at);
    raw[0] = r4.x; raw[1] = r4.y; raw[2] = r4.z; raw[3] = r4.w;
    sh[0] = s4.x; sh[1] = s4.y; sh[2] = s4.z; sh[3] = s4.w;
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (k < n) { raw[k] = a.raw[at + k]; sh[k] = a.shift[at + k]; }
  }
  int y = p0 / a.W, x = p0 - y * a.W;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    bool m1, m2;
    dep[k] = lift_depth_of(raw[k], sh[k], lo, hi, m1, m2);
#pragma unroll
    for (int c = 0; c < 3; ++c) pt[c][k] = (float)(R[3 * c] * (double)x + R[3 * c + 1] * (double)y + R[3 * c + 2]) * dep[k];
    if (++x == a.W) { x = 0; ++y; }
  }
  if (a.vec_full) {
    *reinterpret_cast<float4*>(a.depth + at) = make_float4(dep[0], dep[1], dep[2], dep[3]);
#pragma unroll
    for (int c = 0; c < 3; ++c) *reinterpret_cast<float4*>(a.xyz + at3 + (size_t)c * HW) = make_float4(pt[c][0], pt[c][1], pt[c][2], pt[c][3]);
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (k < n) {
        a.depth[at + k] = dep[k];
#pragma unroll
        for (int c = 0; c < 3; ++c) a.xyz[at3 + (size_t)c * HW + k] = pt[c][k];
      }
  }
}

__global__ __launch_bounds__(256) void k_lift_fwd(const LiftArgs a) {
  const int cue_blocks = a.B * a.V * a.cue_chunks;  // (the cue, most of the traffic, first)
  if ((int)blockIdx.x < cue_blocks) lift_cue_block(a, (int)blockIdx.x);
  else lift_full_block(a, (int)blockIdx.x - cue_blocks);
}

template <bool kIntr>
__global__ __launch_bounds__(256) void k_lift_bwd(const LiftArgs a) {
  __shared__ double red[4][9];
  const int HW = a.H * a.W;
  const int img = (int)blockIdx.x / a.full_chunks, p0 = ((int)blockIdx.x - img * a.full_chunks) * kLiftPix + (int)threadIdx.x * 4;
  const int n = max(0, min(4, HW - p0));
  double G[9] = {0., 0., 0., 0., 0., 0., 0., 0., 0.};
  if (n > 0) {
    double Ki[9], R[9];
    lift_rays(a.intr + (size_t)img * 9, a.W, a.H, Ki, R);
    const float lo = a.near[img], hi = a.far[img];
    const size_t at = (size_t)img * HW + p0, at3 = (size_t)img * 3 * HW + p0;
    float raw[4] = {0.f, 0.f, 0.f, 0.f}, sh[4] = {0.f, 0.f, 0.f, 0.f}, gd[4] = {0.f, 0.f, 0.f, 0.f}, gx[3][4] = {};
    float ds[4], dr[4];
    if (a.vec_full) {
      const float4 r4 = *reinterpret_cast<const float4*>(a.raw + at), s4 = *reinterpret_cast<const float4*>(a.shift + at);
      raw[0] = r4.x; raw[1] = r4.y; raw[2] = r4.z; raw[3] = r4.w;
      sh[0] = s4.x; sh[1] = s4.y; sh[2] = s4.z; sh[3] = s4.w;
      if (a.g_depth) {
        const float4 g4 = *reinterpret_cast<const float4*>(a.g_depth + at);
        gd[0] = g4.x; gd[1] = g4.y; gd[2] = g4.z; gd[3] = g4.w;
      }
      if (a.g_xyz) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const float4 g4 = *reinterpret_cast<const float4*>(a.g_xyz + at3 + (size_t)c * HW);
          gx[c][0] = g4.x; gx[c][1] = g4.y; gx[c][2] = g4.z; gx[c][3] = g4.w;
        }
      }
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (k < n) {
          raw[k] = a.raw[at + k];
          sh[k] = a.shift[at + k];
          if (a.g_depth) gd[k] = a.g_depth[at + k];
          if (a.g_xyz) {
#pragma unroll
            for (int c = 0; c < 3; ++c) gx[c][k] = a.g_xyz[at3 + (size_t)c * HW + k];
          }
        }
    }
    int y = p0 / a.W, x = p0 - y * a.W;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      bool m1, m2;
      const float dep = lift_depth_of(raw[k], sh[k], lo, hi, m1, m2);
      double g = (double)gd[k];
#pragma unroll
      for (int c = 0; c < 3; ++c) g += (double)gx[c][k] * (R[3 * c] * (double)x + R[3 * c + 1] * (double)y + R[3 * c + 2]);
      ds[k] = m2 ? (float)g : 0.f;
      dr[k] = m1 ? ds[k] : 0.f;
      if (kIntr && k < n) {
        const double u = ((double)x + 0.5) / (double)a.W, v = ((double)y + 0.5) / (double)a.H;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const double gz = (double)gx[c][k] * (double)dep;
          G[3 * c] += gz * u; G[3 * c + 1] += gz * v; G[3 * c + 2] += gz;
        }
      }
      if (++x == a.W) { x = 0; ++y; }
    }
    if (a.vec_full) {
      if (a.d_shift) *reinterpret_cast<float4*>(a.d_shift + at) = make_float4(ds[0], ds[1], ds[2], ds[3]);
      if (a.d_raw) *reinterpret_cast<float4*>(a.d_raw + at) = make_float4(dr[0], dr[1], dr[2], dr[3]);
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (k < n) {
          if (a.d_shift) a.d_shift[at + k] = ds[k];
          if (a.d_raw) a.d_raw[at + k] = dr[k];
        }
    }
  }
  if (kIntr) {  // (every thread of the workgroup arrives here)
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
#pragma unroll
    for (int k = 0; k < 9; ++k) G[k] = wave_sum_f64(G[k]);
    if (lane == 0) {
#pragma unroll
      for (int k = 0; k < 9; ++k) red[wv][k] = G[k];
    }
    __syncthreads();
    if (tid < 9) a.partials[(size_t)blockIdx.x * 9 + tid] = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
  }
}

// One workgroup of 64 per image: lane k < 9 adds entry k of the image's workgroups in order; dK = -K^-T G K^-T.
__global__ __launch_bounds__(64) void k_lift_intr_finish(const LiftArgs a) {
  __shared__ double Gs[9];
  const int img = blockIdx.x, tid = threadIdx.x;
  if (tid < 9) {
    double sum = 0.;
    for (int c = 0; c < a.full_chunks; ++c) sum += a.partials[((size_t)img * a.full_chunks + c) * 9 + tid];
    Gs[tid] = sum;
  }
  __syncthreads();
  if (tid < 9) {
    double Ki[9], R[9];
    lift_rays(a.intr + (size_t)img * 9, a.W, a.H, Ki, R);
    const int r = tid / 3, c = tid - 3 * r;
    double sum = 0.;
    for (int m = 0; m < 3; ++m)
      for (int n = 0; n < 3; ++n) sum += Ki[3 * m + r] * Gs[3 * m + n] * Ki[3 * c + n];
    a.d_intr[(size_t)img * 9 + tid] = (float)(-sum);
  }
}

struct PluckerArgs {
  int images, H, W;
  const float *c2w, *intr;
  float* out;
};

// A thread per pixel; everything in fp64 (the map is small), rounded once.  Six coalesced plane stores.
__global__ __launch_bounds__(256) void k_plucker_rays(const PluckerArgs a) {
  const int HW = a.H * a.W, chunks = (HW + 255) / 256;
  const int img = (int)blockIdx.x / chunks, p = ((int)blockIdx.x - img * chunks) * 256 + (int)threadIdx.x;
  if (p >= HW) return;
  double Ki[9], R[9];
  lift_rays(a.intr + (size_t)img * 9, a.W, a.H, Ki, R);
  const int y = p / a.W, x = p - y * a.W;
  double d[3], wd[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) d[c] = R[3 * c] * (double)x + R[3 * c + 1] * (double)y + R[3 * c + 2];
  const double rn = 1.0 / sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
  const float* E = a.c2w + (size_t)img * 16;
#pragma unroll
  for (int c = 0; c < 3; ++c) wd[c] = ((double)E[4 * c] * d[0] + (double)E[4 * c + 1] * d[1] + (double)E[4 * c + 2] * d[2]) * rn;
  const double o[3] = {(double)E[3], (double)E[7], (double)E[11]};
  float* out = a.out + (size_t)img * 6 * HW + p;
  out[0] = (float)wd[0];
  out[(size_t)HW] = (float)wd[1];
  out[(size_t)2 * HW] = (float)wd[2];
  out[(size_t)3 * HW] = (float)(o[1] * wd[2] - o[2] * wd[1]);
  out[(size_t)4 * HW] = (float)(o[2] * wd[0] - o[0] * wd[2]);
  out[(size_t)5 * HW] = (float)(o[0] * wd[1] - o[1] * wd[0]);
}

// The checks of the lift's entry points; D = 1 for the calls that have no cue.
static bool lift_sizes_ok(int B, int V, int H, int W, int D) {
  if (B < 0 || V < 1 || H < 4 || W < 4 || D < 1) return false;
  const int64_t lim = 0x7fffffff, rows = (int64_t)B * V, hw = (int64_t)H * W, q = (int64_t)(H / 4) * (W / 4);
  return rows <= lim && hw <= lim && rows * hw <= lim && rows * hw * 3 <= lim && rows * q <= lim && rows * q * (int64_t)D <= lim;
}

static bool lift_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

static void lift_fill(LiftArgs& a, int B, int V, int H, int W, int D) {
  a.B = B; a.V = V; a.H = H; a.W = W; a.D = D; a.Hq = H / 4; a.Wq = W / 4;
  a.full_chunks = (int)(((int64_t)H * W + kLiftPix - 1) / kLiftPix);
  a.cue_chunks = (int)(((int64_t)a.Hq * a.Wq + kLiftQ - 1) / kLiftQ);
}
}  // namespace gsr

extern "C" {

size_t gsr_lift_scratch_bytes(int num_scenes, int num_views, int height, int width) {
  if (!gsr::lift_sizes_ok(num_scenes, num_views, height, width, 1)) return 0;
  const int64_t chunks = ((int64_t)height * width + gsr::kLiftPix - 1) / gsr::kLiftPix;
  return (size_t)num_scenes * num_views * (size_t)chunks * 9 * sizeof(double);
}

int gsr_lift_depth(int num_scenes, int num_views, int height, int width, int num_depth_candidates, const float* depth_raw,
                   const float* shift, const float* near, const float* far, const float* intrinsics, const float* lin, float* depth,
                   float* xyz, float* cue, void* stream_) {
  using namespace gsr;
  if (!lift_sizes_ok(num_scenes, num_views, height, width, num_depth_candidates)) return GSR_ERR_INVALID_ARGUMENT;
  if (!depth_raw || !shift || !near || !far || !intrinsics || !depth || !xyz || !cue) return GSR_ERR_INVALID_ARGUMENT;
  if (num_scenes == 0) return GSR_OK;
  LiftArgs a{};
  lift_fill(a, num_scenes, num_views, height, width, num_depth_candidates);
  a.raw = depth_raw; a.shift = shift; a.near = near; a.far = far; a.intr = intrinsics; a.lin = lin;
  a.depth = depth; a.xyz = xyz; a.cue = cue;
  a.vec_full = (height * width) % 4 == 0 && lift_aligned16(depth_raw) && lift_aligned16(shift) && lift_aligned16(depth) && lift_aligned16(xyz);
  a.vec_cue = (a.Hq * a.Wq) % 4 == 0 && lift_aligned16(cue);
  const int64_t blocks = (int64_t)num_scenes * num_views * ((int64_t)a.full_chunks + a.cue_chunks);
  if (blocks > 0x7fffffff) return GSR_ERR_INVALID_ARGUMENT;
  hipLaunchKernelGGL(k_lift_fwd, dim3((unsigned)blocks), dim3(256), 0, static_cast<hipStream_t>(stream_), a);
  GSR_CHECK(hipGetLastError());
  return GSR_OK;
}

int gsr_lift_depth_backward(int num_scenes, int num_views, int height, int width, const float* depth_raw, const float* shift,
                            const float* near, const float* far, const float* intrinsics, const float* dL_ddepth, const float* dL_dxyz,
                            float* dL_ddepth_raw, float* dL_dshift, float* dL_dintrinsics, void* scratch, void* stream_) {
  using namespace gsr;
  if (!lift_sizes_ok(num_scenes, num_views, height, width, 1)) return GSR_ERR_INVALID_ARGUMENT;
  if (!depth_raw || !shift || !near || !far || !intrinsics || (dL_dintrinsics && !scratch)) return GSR_ERR_INVALID_ARGUMENT;
  if (num_scenes == 0) return GSR_OK;
  hipStream_t st = static_cast<hipStream_t>(stream_);
  LiftArgs a{};
  lift_fill(a, num_scenes, num_views, height, width, 1);
  a.raw = depth_raw; a.shift = shift; a.near = near; a.far = far; a.intr = intrinsics;
  a.g_depth = dL_ddepth; a.g_xyz = dL_dxyz; a.d_raw = dL_ddepth_raw; a.d_shift = dL_dshift; a.d_intr = dL_dintrinsics;
  a.partials = static_cast<double*>(scratch);
  a.vec_full = (height * width) % 4 == 0 && lift_aligned16(depth_raw) && lift_aligned16(shift) && lift_aligned16(dL_ddepth) &&
               lift_aligned16(dL_dxyz) && lift_aligned16(dL_ddepth_raw) && lift_aligned16(dL_dshift);
  const int64_t blocks = (int64_t)num_scenes * num_views * a.full_chunks;
  if (dL_dintrinsics) {
    hipLaunchKernelGGL(k_lift_bwd<true>, dim3((unsigned)blocks), dim3(256), 0, st, a);
    GSR_CHECK(hipGetLastError());
    hipLaunchKernelGGL(k_lift_intr_finish, dim3((unsigned)(num_scenes * num_views)), dim3(64), 0, st, a);
  } else {
    hipLaunchKernelGGL(k_lift_bwd<false>, dim3((unsigned)blocks), dim3(256), 0, st, a);
  }
  GSR_CHECK(hipGetLastError());
  return GSR_OK;
}

int gsr_plucker_rays(int num_scenes, int num_views, int height, int width, const float* c2w, const float* intrinsics, float* out,
                     void* stream_) {
  using namespace gsr;
  if (num_scenes < 0 || num_views < 1 || height < 1 || width < 1 || !c2w || !intrinsics || !out) return GSR_ERR_INVALID_ARGUMENT;
  const int64_t lim = 0x7fffffff, rows = (int64_t)num_scenes * num_views, hw = (int64_t)height * width;
  if (rows > lim || hw > lim || rows * hw > lim || rows * hw * 6 > lim) return GSR_ERR_INVALID_ARGUMENT;
  if (num_scenes == 0) return GSR_OK;
  PluckerArgs a{(int)rows, height, width, c2w, intrinsics, out};
  hipLaunchKernelGGL(k_plucker_rays, dim3((unsigned)(rows * ((hw + 255) / 256))), dim3(256), 0, static_cast<hipStream_t>(stream_), a);
  GSR_CHECK(hipGetLastError());
  return GSR_OK;
}

}  // extern "C"

// ------------------------------------------------------------------------------------------------
// Mono-guided attention over the cost volume (reference src/model/encoder/costvolume/depth_predictor_multiview.py:360-366;
// definition: include/gsr.h): out[b, c, i] = sum_j softmax_j(sum_e q[b, e, i] k[b, e, j]) v[b, c, j], all arrays channel-major.  It
// lives in this header because it is the cost volume's consumer: `v` is the 1 x 1 convolution of the volume's features.  Nothing of
// L x L floats exists: the scores are formed, used and dropped 32 x 32 at a time, in the registers of one wave.
// Every product is __builtin_amdgcn_mfma_f32_32x32x2f32 (D = A B + C over 32 x 32 with two k values per instruction, exact f32, a
// k-ordered fmaf chain: lane l gives A[l & 31][l >> 5] and B[l >> 5][l & 31]; register r of the result is row ma_row(r, l >> 5) =
// (r & 3) + 8 (r >> 2) + 4 (l >> 5) of column l & 31).  A workgroup is four waves; a wave OWNS 32 columns - queries in the forward
// and in the dQ pass, keys in the dK / dV pass - and the workgroup streams tiles of 32 of the other index through LDS (fetched one
// tile ahead into registers, two LDS buffers, one barrier per tile; in the backward one buffer and two barriers at more than 128
// value channels).
// The score tile is formed with the owned index on the lane, so its 16 registers are directly the B operand of the products
// that sum over the streamed index: register r is k value ma_row(r, h) of lane half h, and the A operand is read from LDS in that
// same order.  A row statistic (maximum, sum) is a reduction over a lane's registers and one exchange with lane ^ 32.
//   forward  S^T = K^T Q (k = e), online softmax per query column, out_tile += V_tile P^T (A = V[c][j] from a [j][c] LDS image).
//   dK / dV  S = Q^T K, P = exp(S - lse_i), dV += dO P (A = dO[c][i] from an [i][c] image), dP = dO^T V (k = c, B = the wave's v
//            columns, in registers), dS = P (dP - delta_i), dK += Q dS (A = q[e][i]).
//   dQ       S^T and P^T as the forward, dP^T = V^T dO (k = c, B = the wave's dO columns, in registers), dQ += K dS^T.
// The forward splits the value channels over blockIdx.y in chunks of 64 (NT = 2 tiles of 32; one tile at C <= 32): the chunks of a
// query block are workgroups of their own that each form the same scores and statistics, so two or more waves share a SIMD and
// one's softmax runs under the other's matrix instructions; chunk 0 writes lse.  The backward passes sum over ALL channels for dP
// and pad the channel count to NT = 1, 2, 4 or 8 tiles of 32 (zeros in LDS and registers; nothing is stored for them); E is padded
// to 32.  Sums over the streamed index stay inside one wave, in tile order: no atomics, no cross-workgroup sums, the
// same bits on every run, forward and backward.  delta = sum_c dO out is a small launch of its own into the caller's scratch.
// ------------------------------------------------------------------------------------------------
namespace gsr {
typedef float ma_f16 __attribute__((ext_vector_type(16)));
constexpr int kMaOwn = 128;  // owned columns of a workgroup: 4 waves x 32
constexpr int kMaTile = 32;  // streamed rows of a tile

struct MonoAttnArgs {
  int n, E, L, C;
  const float *q, *k, *v;      // (n, E, L), (n, E, L), (n, C, L)
  const float *out, *lse, *g;  // backward: the forward's results and dL/dout
  float *o_out, *o_lse;        // forward
  float *dq, *dk, *dv, *delta;
};

__device__ __forceinline__ int ma_row(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }

__device__ __forceinline__ ma_f16 ma_mfma(float a, float b, ma_f16 c) { return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0); }

__device__ __forceinline__ ma_f16 ma_zero() {
  ma_f16 z;
#pragma unroll
  for (int r = 0; r < 16; ++r) z[r] = 0.f;
  return z;
}

// Rows [0, ROWS) x columns [col0, col0 + 32) of a (rows, L) matrix into ROWS / 8 registers of each of 256 threads: element
// idx = tid + 256 u is row idx >> 5, column idx & 31; zero outside [0, valid) x [0, L).
template <int ROWS>
__device__ __forceinline__ void ma_fetch(const float* base, int valid, int L, int col0, int tid, float* regs) {
#pragma unroll
  for (int u = 0; u < ROWS / 8; ++u) {
    const int idx = tid + 256 * u, row = idx >> 5, col = col0 + (idx & 31);
    regs[u] = (row < valid && col < L) ? base[(size_t)row * L + col] : 0.f;
  }
}

// ... to LDS as [row][column] (kT = false) or [column][row] (kT = true), `stride` floats per line.
template <int ROWS, bool kT>
__device__ __forceinline__ void ma_put(float* dst, int stride, int tid, const float* regs) {
#pragma unroll
  for (int u = 0; u < ROWS / 8; ++u) {
    const int idx = tid + 256 * u, row = idx >> 5, col = idx & 31;
    dst[kT ? col * stride + row : row * stride + col] = regs[u];
  }
}

// The owned columns' q or k block, [e][kMaOwn], zero outside.
__device__ __forceinline__ void ma_put_own(float* dst, const float* base, int E, int L, int col0, int tid) {
  for (int idx = tid; idx < 32 * kMaOwn; idx += 256) {
    const int e = idx / kMaOwn, col = col0 + (idx - e * kMaOwn);
    dst[idx] = (e < E && col < L) ? base[(size_t)e * L + col] : 0.f;
  }
}

template <int NT>
__global__ __launch_bounds__(256) void k_mono_attn_fwd(const MonoAttnArgs a) {
  constexpr int CS = 32 * NT + 8, NB = 2;  // (4 CS = 32 mod 64: the two lane halves read disjoint banks)
  __shared__ float Qs[32 * kMaOwn];
  __shared__ float Ks[NB][32 * 32];
  __shared__ float Vs[NB][32 * CS];
  const int blocks = (a.L + kMaOwn - 1) / kMaOwn;
  const int b = (int)blockIdx.x / blocks, i0 = ((int)blockIdx.x - b * blocks) * kMaOwn;
  const int c0 = (int)blockIdx.y * 32 * NT, cn = a.C - c0;  // this workgroup's value channels [c0, c0 + min(cn, 32 NT))
  const int tid = threadIdx.x, lane = tid & 63, x = lane & 31, h = lane >> 5, wv = tid >> 6;
  const int L = a.L, EP = (a.E + 1) / 2, T = (L + kMaTile - 1) / kMaTile;
  const float* kb = a.k + (size_t)b * a.E * L;
  const float* vb = a.v + ((size_t)b * a.C + c0) * L;
  float kp[4], vp[4 * NT];
  ma_put_own(Qs, a.q + (size_t)b * a.E * L, a.E, L, i0, tid);
  ma_fetch<32>(kb, a.E, L, 0, tid, kp);
  ma_fetch<32 * NT>(vb, cn, L, 0, tid, vp);
  ma_put<32, false>(Ks[0], 32, tid, kp);
  ma_put<32 * NT, true>(Vs[0], CS, tid, vp);
  __syncthreads();
  ma_f16 acc[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) acc[t] = ma_zero();
  float m = -INFINITY, l = 0.f;
  for (int tile = 0; tile < T; ++tile) {
    const int cur = tile & 1, nxt = cur ^ 1, j0 = tile * kMaTile;
    const bool more = tile + 1 < T;
    if (more) {
      ma_fetch<32>(kb, a.E, L, j0 + kMaTile, tid, kp);
      ma_fetch<32 * NT>(vb, cn, L, j0 + kMaTile, tid, vp);
    }
    ma_f16 s = ma_zero();  // S^T[j][i]
    for (int p = 0; p < EP; ++p) s = ma_mfma(Ks[cur][(2 * p + h) * 32 + x], Qs[(2 * p + h) * kMaOwn + wv * 32 + x], s);
    float mx = -INFINITY;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      if (j0 + ma_row(r, h) >= L) s[r] = -INFINITY;
      mx = fmaxf(mx, s[r]);
    }
    mx = fmaxf(mx, __shfl_xor(mx, 32));
    const float m_new = fmaxf(m, mx), alpha = expf(m - m_new);  // (every tile holds a key: m_new is finite; exp(-inf) = 0)
    float sum = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      s[r] = expf(s[r] - m_new);
      sum += s[r];
    }
    sum += __shfl_xor(sum, 32);
    l = l * alpha + sum;
    m = m_new;
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[t] *= alpha;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
#pragma unroll
      for (int t = 0; t < NT; ++t) acc[t] = ma_mfma(Vs[cur][ma_row(r, h) * CS + 32 * t + x], s[r], acc[t]);
    }
    if (more) {
      ma_put<32, false>(Ks[nxt], 32, tid, kp);
      ma_put<32 * NT, true>(Vs[nxt], CS, tid, vp);
    }
    __syncthreads();
  }
  const int i = i0 + wv * 32 + x;
  if (i < L) {
    float* ob = a.o_out + ((size_t)b * a.C + c0) * L + i;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int c = 32 * t + ma_row(r, h);
        if (c < cn) ob[(size_t)c * L] = acc[t][r] / l;
      }
    }
    if (h == 0 && blockIdx.y == 0) a.o_lse[(size_t)b * L + i] = m + logf(l);
  }
}

// delta[b, i] = sum_c dO[b, c, i] out[b, c, i], an fmaf chain in channel order.
__global__ __launch_bounds__(256) void k_mono_attn_delta(const MonoAttnArgs a) {
  const int chunks = (a.L + 255) / 256;
  const int b = (int)blockIdx.x / chunks, i = ((int)blockIdx.x - b * chunks) * 256 + (int)threadIdx.x;
  if (i >= a.L) return;
  const size_t at = (size_t)b * a.C * a.L + i;
  float sum = 0.f;
  for (int c = 0; c < a.C; ++c) sum = fmaf(a.g[at + (size_t)c * a.L], a.out[at + (size_t)c * a.L], sum);  // (the chain dP is summed by)
  a.delta[(size_t)b * a.L + i] = sum;
}

// dK and dV: a wave owns 32 keys (the lane column); query tiles are streamed.
template <int NT>
__global__ __launch_bounds__(256) void k_mono_attn_bwd_kv(const MonoAttnArgs a) {
  constexpr int CS = 32 * NT + 1, NB = NT == 8 ? 1 : 2;  // (odd: the [i][c] image is read by rows and by columns)
  __shared__ float Ks[32 * kMaOwn];
  __shared__ float Qs[NB][32 * 33];
  __shared__ float Gs[NB][32 * CS];
  __shared__ float Ls[NB][2][32];
  const int blocks = (a.L + kMaOwn - 1) / kMaOwn;
  const int b = (int)blockIdx.x / blocks, j0 = ((int)blockIdx.x - b * blocks) * kMaOwn;
  const int tid = threadIdx.x, lane = tid & 63, x = lane & 31, h = lane >> 5, wv = tid >> 6;
  const int L = a.L, EP = (a.E + 1) / 2, T = (L + kMaTile - 1) / kMaTile;
  const int j = j0 + wv * 32 + x;
  const float* qb = a.q + (size_t)b * a.E * L;
  const float* gb = a.g + (size_t)b * a.C * L;
  const float* lb = a.lse + (size_t)b * L;
  const float* db = a.delta + (size_t)b * L;
  float qp[4], gp[4 * NT], sp = 0.f;
  float vreg[16 * NT];  // v[c = 2 p + h][j]
#pragma unroll
  for (int p = 0; p < 16 * NT; ++p) vreg[p] = (2 * p + h < a.C && j < L) ? a.v[((size_t)b * a.C + 2 * p + h) * L + j] : 0.f;
  ma_put_own(Ks, a.k + (size_t)b * a.E * L, a.E, L, j0, tid);
  ma_fetch<32>(qb, a.E, L, 0, tid, qp);
  ma_fetch<32 * NT>(gb, a.C, L, 0, tid, gp);
  if (tid < 64) sp = (tid & 31) < L ? (tid < 32 ? lb : db)[tid & 31] : 0.f;
  ma_put<32, false>(Qs[0], 33, tid, qp);
  ma_put<32 * NT, true>(Gs[0], CS, tid, gp);
  if (tid < 64) Ls[0][tid >> 5][tid & 31] = sp;
  __syncthreads();
  ma_f16 dv[NT], dk = ma_zero();
#pragma unroll
  for (int t = 0; t < NT; ++t) dv[t] = ma_zero();
  for (int tile = 0; tile < T; ++tile) {
    const int cur = NB == 2 ? (tile & 1) : 0, nxt = NB == 2 ? (cur ^ 1) : 0, i0 = tile * kMaTile;
    const bool more = tile + 1 < T;
    if (more) {
      ma_fetch<32>(qb, a.E, L, i0 + kMaTile, tid, qp);
      ma_fetch<32 * NT>(gb, a.C, L, i0 + kMaTile, tid, gp);
      if (tid < 64) sp = i0 + kMaTile + (tid & 31) < L ? (tid < 32 ? lb : db)[i0 + kMaTile + (tid & 31)] : 0.f;
    }
    ma_f16 s = ma_zero();  // S[i][j]
    for (int p = 0; p < EP; ++p) s = ma_mfma(Qs[cur][(2 * p + h) * 33 + x], Ks[(2 * p + h) * kMaOwn + wv * 32 + x], s);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int ri = ma_row(r, h);
      s[r] = (i0 + ri < L && j < L) ? expf(s[r] - Ls[cur][0][ri]) : 0.f;
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
#pragma unroll
      for (int t = 0; t < NT; ++t) dv[t] = ma_mfma(Gs[cur][ma_row(r, h) * CS + 32 * t + x], s[r], dv[t]);
    }
    ma_f16 dp = ma_zero();  // dP[i][j]
#pragma unroll
    for (int p = 0; p < 16 * NT; ++p) dp = ma_mfma(Gs[cur][x * CS + 2 * p + h], vreg[p], dp);
#pragma unroll
    for (int r = 0; r < 16; ++r) s[r] = s[r] * (dp[r] - Ls[cur][1][ma_row(r, h)]);
#pragma unroll
    for (int r = 0; r < 16; ++r) dk = ma_mfma(Qs[cur][x * 33 + ma_row(r, h)], s[r], dk);
    if (NB == 1) __syncthreads();
    if (more) {
      ma_put<32, false>(Qs[nxt], 33, tid, qp);
      ma_put<32 * NT, true>(Gs[nxt], CS, tid, gp);
      if (tid < 64) Ls[nxt][tid >> 5][tid & 31] = sp;
    }
    __syncthreads();
  }
  if (j < L) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = ma_row(r, h);
      if (a.dk && row < a.E) a.dk[((size_t)b * a.E + row) * L + j] = dk[r];
      if (a.dv) {
#pragma unroll
        for (int t = 0; t < NT; ++t)
          if (32 * t + row < a.C) a.dv[((size_t)b * a.C + 32 * t + row) * L + j] = dv[t][r];
      }
    }
  }
}

// dQ: a wave owns 32 queries (the lane column), as the forward; key tiles are streamed.
template <int NT>
__global__ __launch_bounds__(256) void k_mono_attn_bwd_q(const MonoAttnArgs a) {
  constexpr int NB = NT == 8 ? 1 : 2;
  __shared__ float Qs[32 * kMaOwn];
  __shared__ float Ks[NB][32 * 33];
  __shared__ float Vs[NB][32 * NT * 32];
  const int blocks = (a.L + kMaOwn - 1) / kMaOwn;
  const int b = (int)blockIdx.x / blocks, i0 = ((int)blockIdx.x - b * blocks) * kMaOwn;
  const int tid = threadIdx.x, lane = tid & 63, x = lane & 31, h = lane >> 5, wv = tid >> 6;
  const int L = a.L, EP = (a.E + 1) / 2, T = (L + kMaTile - 1) / kMaTile;
  const int i = i0 + wv * 32 + x;
  const float* kb = a.k + (size_t)b * a.E * L;
  const float* vb = a.v + (size_t)b * a.C * L;
  const float lse_i = i < L ? a.lse[(size_t)b * L + i] : 0.f, delta_i = i < L ? a.delta[(size_t)b * L + i] : 0.f;
  float kp[4], vp[4 * NT];
  float greg[16 * NT];  // dO[c = 2 p + h][i]
#pragma unroll
  for (int p = 0; p < 16 * NT; ++p) greg[p] = (2 * p + h < a.C && i < L) ? a.g[((size_t)b * a.C + 2 * p + h) * L + i] : 0.f;
  ma_put_own(Qs, a.q + (size_t)b * a.E * L, a.E, L, i0, tid);
  ma_fetch<32>(kb, a.E, L, 0, tid, kp);
  ma_fetch<32 * NT>(vb, a.C, L, 0, tid, vp);
  ma_put<32, false>(Ks[0], 33, tid, kp);
  ma_put<32 * NT, false>(Vs[0], 32, tid, vp);
  __syncthreads();
  ma_f16 dq = ma_zero();
  for (int tile = 0; tile < T; ++tile) {
    const int cur = NB == 2 ? (tile & 1) : 0, nxt = NB == 2 ? (cur ^ 1) : 0, j0 = tile * kMaTile;
    const bool more = tile + 1 < T;
    if (more) {
      ma_fetch<32>(kb, a.E, L, j0 + kMaTile, tid, kp);
      ma_fetch<32 * NT>(vb, a.C, L, j0 + kMaTile, tid, vp);
    }
    ma_f16 s = ma_zero();  // S^T[j][i]
    for (int p = 0; p < EP; ++p) s = ma_mfma(Ks[cur][(2 * p + h) * 33 + x], Qs[(2 * p + h) * kMaOwn + wv * 32 + x], s);
    ma_f16 dp = ma_zero();  // dP^T[j][i]
#pragma unroll
    for (int p = 0; p < 16 * NT; ++p) dp = ma_mfma(Vs[cur][(2 * p + h) * 32 + x], greg[p], dp);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float pr = j0 + ma_row(r, h) < L ? expf(s[r] - lse_i) : 0.f;
      s[r] = pr * (dp[r] - delta_i);
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) dq = ma_mfma(Ks[cur][x * 33 + ma_row(r, h)], s[r], dq);
    if (NB == 1) __syncthreads();
    if (more) {
      ma_put<32, false>(Ks[nxt], 33, tid, kp);
      ma_put<32 * NT, false>(Vs[nxt], 32, tid, vp);
    }
    __syncthreads();
  }
  if (i < L) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int e = ma_row(r, h);
      if (e < a.E) a.dq[((size_t)b * a.E + e) * L + i] = dq[r];
    }
  }
}

static bool ma_sizes_ok(int n, int E, int L, int C) {
  if (n < 1 || E < 1 || E > 32 || C < 1 || C > 256 || L < 1) return false;
  const int64_t lim = 0x7fffffff;
  return (int64_t)n * (E > C ? E : C) * (int64_t)L <= lim && (int64_t)n * (((int64_t)L + kMaOwn - 1) / kMaOwn) <= lim;
}

static int ma_tiles(int C) { return C <= 32 ? 1 : C <= 64 ? 2 : C <= 128 ? 4 : 8; }

#define GSR_MA_LAUNCH(kernel, grid, st, a)                                                       \
  switch (ma_tiles((a).C)) {                                                                     \
    case 1: hipLaunchKernelGGL(kernel<1>, dim3((unsigned)(grid)), dim3(256), 0, st, a); break;   \
    case 2: hipLaunchKernelGGL(kernel<2>, dim3((unsigned)(grid)), dim3(256), 0, st, a); break;   \
    case 4: hipLaunchKernelGGL(kernel<4>, dim3((unsigned)(grid)), dim3(256), 0, st, a); break;   \
    default: hipLaunchKernelGGL(kernel<8>, dim3((unsigned)(grid)), dim3(256), 0, st, a); break;  \
  }
}  // namespace gsr

extern "C" {

size_t gsr_mono_attention_scratch_bytes(int n, int E, int L, int C) {
  if (!gsr::ma_sizes_ok(n, E, L, C)) return 0;
  return (size_t)n * (size_t)L * sizeof(float);
}

int gsr_mono_attention(int n, int E, int L, int C, const float* q, const float* k, const float* v, float* out, float* lse,
                       void* stream_) {
  using namespace gsr;
  if (!ma_sizes_ok(n, E, L, C)) return GSR_ERR_INVALID_ARGUMENT;
  if (!q || !k || !v || !out || !lse) return GSR_ERR_INVALID_ARGUMENT;
  hipStream_t st = static_cast<hipStream_t>(stream_);
  MonoAttnArgs a{};
  a.n = n; a.E = E; a.L = L; a.C = C; a.q = q; a.k = k; a.v = v; a.o_out = out; a.o_lse = lse;
  const int64_t grid = (int64_t)n * ((L + kMaOwn - 1) / kMaOwn);
  if (C <= 32) hipLaunchKernelGGL(k_mono_attn_fwd<1>, dim3((unsigned)grid), dim3(256), 0, st, a);
  else hipLaunchKernelGGL(k_mono_attn_fwd<2>, dim3((unsigned)grid, (unsigned)((C + 63) / 64)), dim3(256), 0, st, a);
  GSR_CHECK(hipGetLastError());
  return GSR_OK;
}

int gsr_mono_attention_backward(int n, int E, int L, int C, const float* q, const float* k, const float* v, const float* out,
                                const float* lse, const float* dL_dout, float* dL_dq, float* dL_dk, float* dL_dv, void* scratch,
                                void* stream_) {
  using namespace gsr;
  if (!ma_sizes_ok(n, E, L, C)) return GSR_ERR_INVALID_ARGUMENT;
  if (!q || !k || !v || !out || !lse || !dL_dout || !scratch) return GSR_ERR_INVALID_ARGUMENT;
  if (!dL_dq && !dL_dk && !dL_dv) return GSR_OK;
  hipStream_t st = static_cast<hipStream_t>(stream_);
  MonoAttnArgs a{};
  a.n = n; a.E = E; a.L = L; a.C = C; a.q = q; a.k = k; a.v = v; a.out = out; a.lse = lse; a.g = dL_dout;
  a.dq = dL_dq; a.dk = dL_dk; a.dv = dL_dv; a.delta = static_cast<float*>(scratch);
  const int64_t grid = (int64_t)n * ((L + kMaOwn - 1) / kMaOwn);
  hipLaunchKernelGGL(k_mono_attn_delta, dim3((unsigned)((int64_t)n * ((L + 255) / 256))), dim3(256), 0, st, a);
  GSR_CHECK(hipGetLastError());
  if (dL_dk || dL_dv) {
    GSR_MA_LAUNCH(k_mono_attn_bwd_kv, grid, st, a);
    GSR_CHECK(hipGetLastError());
  }
  if (dL_dq) {
    GSR_MA_LAUNCH(k_mono_attn_bwd_q, grid, st, a);
    GSR_CHECK(hipGetLastError());
  }
  return GSR_OK;
}

}  // extern "C"

// ------------------------------------------------------------------------------------------------
// Multi-head attention (LightGlue's SelfBlock / CrossBlock in the pose transformer, reference src/model/LightGlue/lightglue/
// lightglue.py:133-224 as src/model/encoder/encoder_costvolume.py:401-441 uses them; definition: include/gsr.h): the mono kernels'
// tile scheme - four waves, a wave owns 32 columns, tiles of 32 of the other index through two LDS buffers, the score tile in
// registers as the next product's B operand - with what the transformer needs and the mono attention has not: N queries and M keys,
// (batch, head) as the row, operands read through four element strides (batch, head, token, channel; offsets in 64 bits), a scale
// factor, and TOKEN-MAJOR results: out, dL_dout, dQ are (B, N, H, D), dK, dV (B, M, H, D).  D <= 32: one value tile, D padded to 32
// by zeros in LDS.  The passes are device functions of ONE kernel, k_mha_ops, and share the mono kernels' device functions (ma_row,
// ma_mfma, ma_zero).
// Loads: the lane index of every global load runs along the CHANNELS (element idx of a tile is token idx >> 5, channel idx & 31), so
//   with a channel stride of 1 a token's D floats are one segment; the images the products read by channel rows ([c][token], stride
//   33) are transposed by the LDS store.  The owned operands - q or k for the score product, v or dO for dP - are the same for every
//   streamed tile: they are staged through the owned block's LDS image once, not gathered token by token, and then live in registers.
// Stores: an accumulator holds a token per lane; after the last tile it goes through the (then free) owned block's LDS as
//   [token][33] and leaves as D contiguous floats per token.
// Scale: the SCORE TILE is multiplied by `scale` (one rounding of scale * (q . k), the same bits in all three passes, so P of the
//   backward is the forward's); dQ and dK take the factor once, on the finished accumulator.
// Masking: keys past M are -inf before the running maximum (every streamed tile holds a real key: the maximum stays finite); in the
//   backward P is zero outside N x M.  Queries past N are zero columns that nothing stores.
// ------------------------------------------------------------------------------------------------
namespace gsr {
constexpr int kMhOwnS = kMaOwn + 1;  // line stride of the owned [c][token] image (odd: filled by channel, read by token)
constexpr int kMhOwnFloats = 4 * 32 * 33;  // the owned image, and after the loop four [token][33] output tiles
constexpr int kMhFwdCS = 40;               // line stride of the forward's [key][channel] value image
constexpr int kMhLdsFloats = kMhOwnFloats + 2 * 32 * 33 + 2 * 32 * kMhFwdCS;  // the forward's need, the largest of the passes
enum { kMhFwd = 0, kMhDelta = 1, kMhBwdKV = 2, kMhBwdQ = 3 };

struct MhaArgs {
  int op, B, H, N, M, D;  // op: the pass of k_mha_ops this launch runs
  float scale;
  const float *q, *k, *v;
  int64_t qs[4], ks[4], vs[4];  // element strides: batch, head, token, channel
  const float *out, *lse, *g;   // backward: the forward's results and dL/dout, (B, N, H, D), (B, H, N), (B, N, H, D)
  float *o_out, *o_lse;
  float *dq, *dk, *dv, *delta;  // (B, N, H, D), (B, M, H, D), (B, M, H, D), (B, H, N)
};

// Tokens [tok0, tok0 + 32) x channels [0, 32) of a strided operand into 4 registers of each of 256 threads: element idx = tid + 256 u
// is token idx >> 5, channel idx & 31; zero outside [0, ntok) x [0, D).
__device__ __forceinline__ void mh_fetch(const float* base, int64_t st, int64_t sc, int D, int ntok, int tok0, int tid, float* regs) {
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int idx = tid + 256 * u, tok = tok0 + (idx >> 5), c = idx & 31;
    regs[u] = (c < D && tok < ntok) ? base[(int64_t)tok * st + (int64_t)c * sc] : 0.f;
  }
}

// ... to LDS as [token][channel] (kT = false) or [channel][token] (kT = true), `stride` floats per line.
template <bool kT>
__device__ __forceinline__ void mh_put(float* dst, int stride, int tid, const float* regs) {
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int idx = tid + 256 * u, tok = idx >> 5, c = idx & 31;
    dst[kT ? c * stride + tok : tok * stride + c] = regs[u];
  }
}

// The owned tokens' block of a strided operand, [c][kMhOwnS], zero outside.
__device__ __forceinline__ void mh_put_own(float* dst, const float* base, int64_t st, int64_t sc, int D, int ntok, int tok0, int tid) {
  for (int idx = tid; idx < 32 * kMaOwn; idx += 256) {
    const int t = idx >> 5, c = idx & 31, tok = tok0 + t;
    dst[c * kMhOwnS + t] = (c < D && tok < ntok) ? base[(int64_t)tok * st + (int64_t)c * sc] : 0.f;
  }
}

// The owned operand of the score product, out of its LDS image into registers once: it is the same for every streamed tile.
__device__ __forceinline__ void mh_own_regs(const float* own, int wv, int x, int h, float* regs) {
#pragma unroll
  for (int p = 0; p < 16; ++p) regs[p] = own[(2 * p + h) * kMhOwnS + wv * 32 + x];
}

// The score tile: A from the streamed [c][token] image (stride 33), B the owned registers; channel pairs past D are skipped (DP is
// launch-uniform; the loop is unrolled so that the registers are addressed statically).
__device__ __forceinline__ ma_f16 mh_scores(const float* tile, const float* own_regs, int DP, int x, int h) {
  ma_f16 s = ma_zero();
#pragma unroll
  for (int p = 0; p < 16; ++p)
    if (p < DP) s = ma_mfma(tile[(2 * p + h) * 33 + x], own_regs[p], s);
  return s;
}

// A wave's finished 32 x 32 accumulator (register r = channel ma_row(r, h) of the lane's token) times `f` to a token-major array:
// through the wave's [token][33] tile of `own`, then D contiguous floats per token.  `dst` is row 0 of the (batch, head): token t,
// channel c is dst[t tstride + c].  Every thread of the workgroup calls it (two barriers).
__device__ __forceinline__ void mh_store_tile(float* own, const ma_f16& acc, float f, float* dst, int64_t tstride, int tok0, int ntok, int D,
                                              int lane, int wv) {
  float* os = own + wv * 32 * 33;
  const int x = lane & 31, h = lane >> 5;
  __syncthreads();  // (the owned image, or the tile stored before this one, has been read)
#pragma unroll
  for (int r = 0; r < 16; ++r) os[x * 33 + ma_row(r, h)] = acc[r] * f;
  __syncthreads();
#pragma unroll
  for (int u = 0; u < 16; ++u) {
    const int idx = lane + 64 * u, t = idx >> 5, c = idx & 31, tok = tok0 + wv * 32 + t;
    if (c < D && tok < ntok) dst[(int64_t)tok * tstride + c] = os[t * 33 + c];
  }
}

__device__ __forceinline__ void k_mha_fwd(const MhaArgs& a, float* lds) {
  constexpr int CS = kMhFwdCS;  // (4 CS = 32 mod 64: the two lane halves read disjoint banks)
  float* Qs = lds;
  float(*Ks)[32 * 33] = reinterpret_cast<float(*)[32 * 33]>(lds + kMhOwnFloats);
  float(*Vs)[32 * CS] = reinterpret_cast<float(*)[32 * CS]>(lds + kMhOwnFloats + 2 * 32 * 33);
  const int blocks = (a.N + kMaOwn - 1) / kMaOwn;
  const int bh = (int)blockIdx.x / blocks, i0 = ((int)blockIdx.x - bh * blocks) * kMaOwn;
  const int b = bh / a.H, hd = bh - b * a.H;
  const int tid = threadIdx.x, lane = tid & 63, x = lane & 31, h = lane >> 5, wv = tid >> 6;
  const int N = a.N, M = a.M, D = a.D, DP = (D + 1) / 2, T = (M + kMaTile - 1) / kMaTile;
  const float* kb = a.k + (int64_t)b * a.ks[0] + (int64_t)hd * a.ks[1];
  const float* vb = a.v + (int64_t)b * a.vs[0] + (int64_t)hd * a.vs[1];
  float kp[4], vp[4];
  mh_put_own(Qs, a.q + (int64_t)b * a.qs[0] + (int64_t)hd * a.qs[1], a.qs[2], a.qs[3], D, N, i0, tid);
  mh_fetch(kb, a.ks[2], a.ks[3], D, M, 0, tid, kp);
  mh_fetch(vb, a.vs[2], a.vs[3], D, M, 0, tid, vp);
  mh_put<true>(Ks[0], 33, tid, kp);
  mh_put<false>(Vs[0], CS, tid, vp);
  __syncthreads();
  float qreg[16];  // q[c = 2 p + h][i]
  mh_own_regs(Qs, wv, x, h, qreg);
  ma_f16 acc = ma_zero();
  float m = -INFINITY, l = 0.f;
  for (int tile = 0; tile < T; ++tile) {
    const int cur = tile & 1, nxt = cur ^ 1, j0 = tile * kMaTile;
    const bool more = tile + 1 < T;
    if (more) {
      mh_fetch(kb, a.ks[2], a.ks[3], D, M, j0 + kMaTile, tid, kp);
      mh_fetch(vb, a.vs[2], a.vs[3], D, M, j0 + kMaTile, tid, vp);
    }
    ma_f16 s = mh_scores(Ks[cur], qreg, DP, x, h);  // S^T[j][i]
    float mx = -INFINITY;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      s[r] = j0 + ma_row(r, h) < M ? s[r] * a.scale : -INFINITY;
      mx = fmaxf(mx, s[r]);
    }
    mx = fmaxf(mx, __shfl_xor(mx, 32));
    const float m_new = fmaxf(m, mx), alpha = expf(m - m_new);  // (every tile holds a key: m_new is finite; exp(-inf) = 0)
    float sum = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      s[r] = expf(s[r] - m_new);
      sum += s[r];
    }
    sum += __shfl_xor(sum, 32);
    l = l * alpha + sum;
    m = m_new;
    acc *= alpha;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc = ma_mfma(Vs[cur][ma_row(r, h) * CS + x], s[r], acc);
    if (more) {
      mh_put<true>(Ks[nxt], 33, tid, kp);
      mh_put<false>(Vs[nxt], CS, tid, vp);
    }
    __syncthreads();
  }
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = acc[r] / l;
  const int64_t hdD = (int64_t)a.H * D;
  mh_store_tile(Qs, acc, 1.f, a.o_out + ((int64_t)b * N * a.H + hd) * D, hdD, i0, N, D, lane, wv);
  const int i = i0 + wv * 32 + x;
  if (i < N && h == 0) a.o_lse[(int64_t)bh * N + i] = m + logf(l);
}

// delta[b, h, i] = sum_c dO[b, i, h, c] out[b, i, h, c], an fmaf chain in channel order.  One thread per (b, i, h): rows of D floats.
__device__ __forceinline__ void k_mha_delta(const MhaArgs& a) {
  const int64_t row = (int64_t)blockIdx.x * 256 + threadIdx.x, rows = (int64_t)a.B * a.N * a.H;
  if (row >= rows) return;
  const int64_t bi = row / a.H;
  const int hd = (int)(row - bi * a.H), b = (int)(bi / a.N), i = (int)(bi - (int64_t)b * a.N);
  const float *g = a.g + row * a.D, *o = a.out + row * a.D;
  float sum = 0.f;
  for (int c = 0; c < a.D; ++c) sum = fmaf(g[c], o[c], sum);  // (the chain dP is summed by)
  a.delta[((int64_t)b * a.H + hd) * a.N + i] = sum;
}

// dK and dV: a wave owns 32 keys (the lane column); query tiles are streamed.
__device__ __forceinline__ void k_mha_bwd_kv(const MhaArgs& a, float* lds) {
  float* Ks = lds;
  float(*Qs)[32 * 33] = reinterpret_cast<float(*)[32 * 33]>(lds + kMhOwnFloats);
  float(*Gs)[32 * 33] = reinterpret_cast<float(*)[32 * 33]>(lds + kMhOwnFloats + 2 * 32 * 33);  // (odd stride: the [i][c] image is read by rows and by columns)
  float(*Ls)[2][32] = reinterpret_cast<float(*)[2][32]>(lds + kMhOwnFloats + 4 * 32 * 33);
  const int blocks = (a.M + kMaOwn - 1) / kMaOwn;
  const int bh = (int)blockIdx.x / blocks, j0 = ((int)blockIdx.x - bh * blocks) * kMaOwn;
  const int b = bh / a.H, hd = bh - b * a.H;
  const int tid = threadIdx.x, lane = tid & 63, x = lane & 31, h = lane >> 5, wv = tid >> 6;
  const int N = a.N, M = a.M, D = a.D, DP = (D + 1) / 2, T = (N + kMaTile - 1) / kMaTile;
  const int j = j0 + wv * 32 + x;
  const int64_t hdD = (int64_t)a.H * D;
  const float* qb = a.q + (int64_t)b * a.qs[0] + (int64_t)hd * a.qs[1];
  const float* gb = a.g + ((int64_t)b * N * a.H + hd) * D;
  const float* lb = a.lse + (int64_t)bh * N;
  const float* db = a.delta + (int64_t)bh * N;
  float qp[4], gp[4], sp = 0.f;
  float vreg[16];  // v[c = 2 p + h][j], through the owned image
  mh_put_own(Ks, a.v + (int64_t)b * a.vs[0] + (int64_t)hd * a.vs[1], a.vs[2], a.vs[3], D, M, j0, tid);
  __syncthreads();
  mh_own_regs(Ks, wv, x, h, vreg);
  __syncthreads();
  mh_put_own(Ks, a.k + (int64_t)b * a.ks[0] + (int64_t)hd * a.ks[1], a.ks[2], a.ks[3], D, M, j0, tid);
  mh_fetch(qb, a.qs[2], a.qs[3], D, N, 0, tid, qp);
  mh_fetch(gb, hdD, 1, D, N, 0, tid, gp);
  if (tid < 64) sp = (tid & 31) < N ? (tid < 32 ? lb : db)[tid & 31] : 0.f;
  mh_put<true>(Qs[0], 33, tid, qp);
  mh_put<false>(Gs[0], 33, tid, gp);
  if (tid < 64) Ls[0][tid >> 5][tid & 31] = sp;
  __syncthreads();
  float kreg[16];  // k[c = 2 p + h][j]
  mh_own_regs(Ks, wv, x, h, kreg);
  ma_f16 dv = ma_zero(), dk = ma_zero();
  for (int tile = 0; tile < T; ++tile) {
    const int cur = tile & 1, nxt = cur ^ 1, i0 = tile * kMaTile;
    const bool more = tile + 1 < T;
    if (more) {
      mh_fetch(qb, a.qs[2], a.qs[3], D, N, i0 + kMaTile, tid, qp);
      mh_fetch(gb, hdD, 1, D, N, i0 + kMaTile, tid, gp);
      if (tid < 64) sp = i0 + kMaTile + (tid & 31) < N ? (tid < 32 ? lb : db)[i0 + kMaTile + (tid & 31)] : 0.f;
    }
    ma_f16 s = mh_scores(Qs[cur], kreg, DP, x, h);  // S[i][j]
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int ri = ma_row(r, h);
      s[r] = (i0 + ri < N && j < M) ? expf(s[r] * a.scale - Ls[cur][0][ri]) : 0.f;
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) dv = ma_mfma(Gs[cur][ma_row(r, h) * 33 + x], s[r], dv);
    ma_f16 dp = ma_zero();  // dP[i][j]
#pragma unroll
    for (int p = 0; p < 16; ++p) dp = ma_mfma(Gs[cur][x * 33 + 2 * p + h], vreg[p], dp);
#pragma unroll
    for (int r = 0; r < 16; ++r) s[r] = s[r] * (dp[r] - Ls[cur][1][ma_row(r, h)]);
#pragma unroll
    for (int r = 0; r < 16; ++r) dk = ma_mfma(Qs[cur][x * 33 + ma_row(r, h)], s[r], dk);
    if (more) {
      mh_put<true>(Qs[nxt], 33, tid, qp);
      mh_put<false>(Gs[nxt], 33, tid, gp);
      if (tid < 64) Ls[nxt][tid >> 5][tid & 31] = sp;
    }
    __syncthreads();
  }
  const int64_t row0 = ((int64_t)b * M * a.H + hd) * D;
  if (a.dk) mh_store_tile(Ks, dk, a.scale, a.dk + row0, hdD, j0, M, D, lane, wv);
  if (a.dv) mh_store_tile(Ks, dv, 1.f, a.dv + row0, hdD, j0, M, D, lane, wv);
}

// dQ: a wave owns 32 queries (the lane column), as the forward; key tiles are streamed.
__device__ __forceinline__ void k_mha_bwd_q(const MhaArgs& a, float* lds) {
  float* Qs = lds;
  float(*Ks)[32 * 33] = reinterpret_cast<float(*)[32 * 33]>(lds + kMhOwnFloats);
  float(*Vs)[32 * 33] = reinterpret_cast<float(*)[32 * 33]>(lds + kMhOwnFloats + 2 * 32 * 33);
  const int blocks = (a.N + kMaOwn - 1) / kMaOwn;
  const int bh = (int)blockIdx.x / blocks, i0 = ((int)blockIdx.x - bh * blocks) * kMaOwn;
  const int b = bh / a.H, hd = bh - b * a.H;
  const int tid = threadIdx.x, lane = tid & 63, x = lane & 31, h = lane >> 5, wv = tid >> 6;
  const int N = a.N, M = a.M, D = a.D, DP = (D + 1) / 2, T = (M + kMaTile - 1) / kMaTile;
  const int i = i0 + wv * 32 + x;
  const int64_t hdD = (int64_t)a.H * D;
  const float* kb = a.k + (int64_t)b * a.ks[0] + (int64_t)hd * a.ks[1];
  const float* vb = a.v + (int64_t)b * a.vs[0] + (int64_t)hd * a.vs[1];
  const float lse_i = i < N ? a.lse[(int64_t)bh * N + i] : 0.f, delta_i = i < N ? a.delta[(int64_t)bh * N + i] : 0.f;
  float kp[4], vp[4];
  float greg[16];  // dO[c = 2 p + h][i], through the owned image
  mh_put_own(Qs, a.g + ((int64_t)b * N * a.H + hd) * D, hdD, 1, D, N, i0, tid);
  __syncthreads();
  mh_own_regs(Qs, wv, x, h, greg);
  __syncthreads();
  mh_put_own(Qs, a.q + (int64_t)b * a.qs[0] + (int64_t)hd * a.qs[1], a.qs[2], a.qs[3], D, N, i0, tid);
  mh_fetch(kb, a.ks[2], a.ks[3], D, M, 0, tid, kp);
  mh_fetch(vb, a.vs[2], a.vs[3], D, M, 0, tid, vp);
  mh_put<true>(Ks[0], 33, tid, kp);
  mh_put<true>(Vs[0], 33, tid, vp);
  __syncthreads();
  float qreg[16];  // q[c = 2 p + h][i]
  mh_own_regs(Qs, wv, x, h, qreg);
  ma_f16 dq = ma_zero();
  for (int tile = 0; tile < T; ++tile) {
    const int cur = tile & 1, nxt = cur ^ 1, j0 = tile * kMaTile;
    const bool more = tile + 1 < T;
    if (more) {
      mh_fetch(kb, a.ks[2], a.ks[3], D, M, j0 + kMaTile, tid, kp);
      mh_fetch(vb, a.vs[2], a.vs[3], D, M, j0 + kMaTile, tid, vp);
    }
    ma_f16 s = mh_scores(Ks[cur], qreg, DP, x, h);  // S^T[j][i]
    ma_f16 dp = ma_zero();  // dP^T[j][i]
#pragma unroll
    for (int p = 0; p < 16; ++p) dp = ma_mfma(Vs[cur][(2 * p + h) * 33 + x], greg[p], dp);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float pr = j0 + ma_row(r, h) < M ? expf(s[r] * a.scale - lse_i) : 0.f;
      s[r] = pr * (dp[r] - delta_i);
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) dq = ma_mfma(Ks[cur][x * 33 + ma_row(r, h)], s[r], dq);
    if (more) {
      mh_put<true>(Ks[nxt], 33, tid, kp);
      mh_put<true>(Vs[nxt], 33, tid, vp);
    }
    __syncthreads();
  }
  mh_store_tile(Qs, dq, a.scale, a.dq + ((int64_t)b * N * a.H + hd) * D, hdD, i0, N, D, lane, wv);
}

// The four passes are ONE kernel switched by the launch-uniform a.op, as k_pose_ops: a kernel costs some 650 bytes of notes,
// symbols and descriptor in front of .text, four of them moved .text - every kernel of the library - up by a page, and the
// rasterizer's headline forward lost 0.5 us to that move (docs/KERNEL_HISTORY.md).  The passes share one LDS arena, carved per pass.
// (A template instance, so that it follows every plain kernel and none of them moves; three waves per SIMD, which the dK / dV pass had as a kernel of its own.)
template <int kThreads>
__global__ __launch_bounds__(kThreads, 3) void k_mha_ops(const MhaArgs a) {
  __shared__ float lds[kMhLdsFloats];
  switch (a.op) {
    case kMhFwd: k_mha_fwd(a, lds); break;
    case kMhDelta: k_mha_delta(a); break;
    case kMhBwdKV: k_mha_bwd_kv(a, lds); break;
    default: k_mha_bwd_q(a, lds); break;
  }
}

static bool mh_sizes_ok(int B, int H, int N, int M, int D, float scale) {
  if (B < 1 || H < 1 || N < 1 || M < 1 || D < 1 || D > 32 || !std::isfinite(scale)) return false;
  const int64_t lim = 0x7fffffff, bh = (int64_t)B * H;
  if (bh > lim) return false;
  return bh * (N > M ? N : M) <= lim / D;  // (B H max(N, M) D <= 2^31 - 1, without overflow; it bounds every grid as well)
}

static void mh_fill(MhaArgs& a, int B, int H, int N, int M, int D, float scale, const float* q, const int64_t* qs, const float* k,
                    const int64_t* ks, const float* v, const int64_t* vs) {
  a.B = B; a.H = H; a.N = N; a.M = M; a.D = D; a.scale = scale; a.q = q; a.k = k; a.v = v;
  for (int s = 0; s < 4; ++s) { a.qs[s] = qs[s]; a.ks[s] = ks[s]; a.vs[s] = vs[s]; }
}
}  // namespace gsr

extern "C" {

size_t gsr_attention_scratch_bytes(int B, int H, int N, int M, int D) {
  if (!gsr::mh_sizes_ok(B, H, N, M, D, 1.f)) return 0;
  return (size_t)B * (size_t)H * (size_t)N * sizeof(float);
}

int gsr_attention(int B, int H, int N, int M, int D, float scale, const float* q, const int64_t* q_strides, const float* k,
                  const int64_t* k_strides, const float* v, const int64_t* v_strides, float* out, float* lse, void* stream_) {
  using namespace gsr;
  if (!mh_sizes_ok(B, H, N, M, D, scale)) return GSR_ERR_INVALID_ARGUMENT;
  if (!q || !q_strides || !k || !k_strides || !v || !v_strides || !out || !lse) return GSR_ERR_INVALID_ARGUMENT;
  MhaArgs a{};
  mh_fill(a, B, H, N, M, D, scale, q, q_strides, k, k_strides, v, v_strides);
  a.o_out = out; a.o_lse = lse;
  const int64_t grid = (int64_t)B * H * ((N + kMaOwn - 1) / kMaOwn);
  a.op = kMhFwd;
  hipLaunchKernelGGL(k_mha_ops<256>, dim3((unsigned)grid), dim3(256), 0, static_cast<hipStream_t>(stream_), a);
  GSR_CHECK(hipGetLastError());
  return GSR_OK;
}

int gsr_attention_backward(int B, int H, int N, int M, int D, float scale, const float* q, const int64_t* q_strides, const float* k,
                           const int64_t* k_strides, const float* v, const int64_t* v_strides, const float* out, const float* lse,
                           const float* dL_dout, float* dL_dq, float* dL_dk, float* dL_dv, void* scratch, void* stream_) {
  using namespace gsr;
  if (!mh_sizes_ok(B, H, N, M, D, scale)) return GSR_ERR_INVALID_ARGUMENT;
  if (!q || !q_strides || !k || !k_strides || !v || !v_strides || !out || !lse || !dL_dout || !scratch) return GSR_ERR_INVALID_ARGUMENT;
  if (!dL_dq && !dL_dk && !dL_dv) return GSR_OK;
  hipStream_t st = static_cast<hipStream_t>(stream_);
  MhaArgs a{};
  mh_fill(a, B, H, N, M, D, scale, q, q_strides, k, k_strides, v, v_strides);
  a.out = out; a.lse = lse; a.g = dL_dout; a.dq = dL_dq; a.dk = dL_dk; a.dv = dL_dv; a.delta = static_cast<float*>(scratch);
  const int64_t bh = (int64_t)B * H;
  a.op = kMhDelta;
  hipLaunchKernelGGL(k_mha_ops<256>, dim3((unsigned)((bh * N + 255) / 256)), dim3(256), 0, st, a);
  GSR_CHECK(hipGetLastError());
  if (dL_dk || dL_dv) {
    a.op = kMhBwdKV;
    hipLaunchKernelGGL(k_mha_ops<256>, dim3((unsigned)(bh * ((M + kMaOwn - 1) / kMaOwn))), dim3(256), 0, st, a);
    GSR_CHECK(hipGetLastError());
  }
  if (dL_dq) {
    a.op = kMhBwdQ;
    hipLaunchKernelGGL(k_mha_ops<256>, dim3((unsigned)(bh * ((N + kMaOwn - 1) / kMaOwn))), dim3(256), 0, st, a);
    GSR_CHECK(hipGetLastError());
  }
  return GSR_OK;
}

}  // extern "C"
