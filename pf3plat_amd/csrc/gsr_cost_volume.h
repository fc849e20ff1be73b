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
