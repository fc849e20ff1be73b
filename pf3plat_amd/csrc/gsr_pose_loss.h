#pragma once
#include "gsr_common.h"

// ------------------------------------------------------------------------------------------------
// Pose loss (reference src/loss/loss_pose.py:28-129, the fourth loss of the training step; definition: include/gsr.h): per match of a
// ragged list per (pair, scene) a 3D residual |Rt x_i - x_j| and a reprojection residual through depth, K_i^-1, Rt and K_j.  Work is
// cut into units of kPoseUnit consecutive matches of ONE list, one workgroup per unit (the L1 normalisation of the scores is linear,
// so a unit only needs its own three sums); every thread builds the list's Rt (fp64: P_j P_i^-1, general 3 x 3 inverse), K_i^-1 and
// K_j from uniform loads, then takes one match: two int64 ids, a score, seven gathered floats.  k_pose_loss_finish - one workgroup,
// a wave per list, fp64, fixed shuffle tree - adds the rows of each list and then the lists.  The backward recomputes everything
// from the inputs (nothing per match is saved), adds dL/dxyz and dL/ddepth into zero-filled arrays with float atomics and writes
// one row of 12 floats (dL/dRt) per unit; k_pose_loss_pose_reduce, a wave per (scene, view), sums the rows of each list in fp64 and
// carries them to the poses, through the inverse for the first view of a pair, its pairs in their fixed order.
// The four kernels are templates (one instance each, <kPoseUnit>) for the code object's layout alone: a plain kernel is emitted in
// front of every template instance, and four new ones there moved the raster kernels 28 KB against the kernels in front of them -
// the headline benchmark lost 0.25 % in six rounds of seven.  As instances they come last and nothing else moves against anything.
// ------------------------------------------------------------------------------------------------
namespace gsr {
constexpr int kPoseUnit = 256;        // matches per workgroup, one per thread
constexpr int kPoseFwdFloats = 4;     // a unit's forward row: sum |w|, sum w r3, sum huber(r2) / delta, 0
constexpr int kPoseBwdFloats = 12;    // a unit's backward row: dL/dRt, rows 0-2 x (R columns 0-2, t)
constexpr int kPoseListFloats = 4;    // a list's row: conf L3, L2, the backward's 3D factor, sum |w|
constexpr float kPoseDelta = 0.01f;   // the Huber threshold of the 2D term
constexpr float kPoseHomEps = 1e-6f;  // from_homogeneous's epsilon

struct PoseLossArgs {
  int B, V, H, W, L;
  const float *xyz, *depth, *poses, *intr;
  const int64_t *ids_i, *ids_j;
  const float *wgt, *conf;
  const int32_t* offs;
  float w2d, w3d;
  float *partials, *lists, *out;                 // forward
  const float* d_loss;                           // backward: the upstream cotangent, one float on the device
  float *d_xyz, *d_depth, *d_poses;
};

struct PoseList {
  int list, s, i, j, begin, end;
  float R[9], t[3], Kj[9];      // Rt of the list (i -> j), K_j
  double Rd[9], td[3], Kid[9];  // Rt before its rounding to float and K_i^-1: the reprojection chain (pose_match) runs in fp64
};

__device__ __forceinline__ int pose_units_of(int m0, int m1) { return (m1 - m0 + kPoseUnit - 1) / kPoseUnit; }

__device__ __forceinline__ void pose_pair_of(int p, int V, int& i, int& j) {
  i = 0;
  while (p >= V - 1 - i) { p -= V - 1 - i; ++i; }
  j = i + 1 + p;
}

// inverse of a 3 x 3 (row-major) in fp64, by the adjugate
__device__ __forceinline__ void pose_inv3(const double* m, double* inv) {
  const double a = m[0], b = m[1], c = m[2], d = m[3], e = m[4], f = m[5], g = m[6], h = m[7], i = m[8];
  inv[0] = e * i - f * h; inv[1] = c * h - b * i; inv[2] = b * f - c * e;
  inv[3] = f * g - d * i; inv[4] = a * i - c * g; inv[5] = c * d - a * f;
  inv[6] = d * h - e * g; inv[7] = b * g - a * h; inv[8] = a * e - b * d;
  const double rdet = 1.0 / (a * inv[0] + b * inv[3] + c * inv[6]);
#pragma unroll
  for (int k = 0; k < 9; ++k) inv[k] *= rdet;
}

// The top three rows of the affine inverse of a pose (rows of 4 floats): A = [R^-1 | -R^-1 t], 12 doubles, rows of 4.
__device__ __forceinline__ void pose_affine_inverse(const float* P, double* A) {
  double r[9], ri[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) r[k] = (double)P[4 * (k / 3) + k % 3];
  pose_inv3(r, ri);
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    A[4 * k] = ri[3 * k]; A[4 * k + 1] = ri[3 * k + 1]; A[4 * k + 2] = ri[3 * k + 2];
    A[4 * k + 3] = -(ri[3 * k] * (double)P[3] + ri[3 * k + 1] * (double)P[7] + ri[3 * k + 2] * (double)P[11]);
  }
}

// Which list a unit belongs to and that list's matrices; all of it uniform over the workgroup.
__device__ __forceinline__ void pose_list_of_unit(const PoseLossArgs& a, int unit, PoseList& c) {
  int l = 0, first = 0, m0 = a.offs[0], m1 = m0;
  for (; l < a.L; ++l) {
    m1 = a.offs[l + 1];
    const int n = pose_units_of(m0, m1);
    if (unit < first + n) break;
    first += n;
    m0 = m1;
  }
  c.list = l;
  c.begin = m0 + (unit - first) * kPoseUnit;
  c.end = min(c.begin + kPoseUnit, m1);
  const int p = l / a.B;
  c.s = l - p * a.B;
  pose_pair_of(p, a.V, c.i, c.j);
  const float* Pj = a.poses + ((size_t)c.s * a.V + c.j) * 16;
  if (c.i == 0) {  // the reference's shortcut: poses[s, 0] is taken as the identity, whatever it holds
#pragma unroll
    for (int k = 0; k < 3; ++k) { c.R[3 * k] = Pj[4 * k]; c.R[3 * k + 1] = Pj[4 * k + 1]; c.R[3 * k + 2] = Pj[4 * k + 2]; c.t[k] = Pj[4 * k + 3]; }
#pragma unroll
    for (int k = 0; k < 9; ++k) c.Rd[k] = (double)c.R[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) c.td[k] = (double)c.t[k];
  } else {
    double A[12];
    pose_affine_inverse(a.poses + ((size_t)c.s * a.V + c.i) * 16, A);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const double x = Pj[4 * k], y = Pj[4 * k + 1], z = Pj[4 * k + 2];
#pragma unroll
      for (int q = 0; q < 3; ++q) { c.Rd[3 * k + q] = x * A[q] + y * A[4 + q] + z * A[8 + q]; c.R[3 * k + q] = (float)c.Rd[3 * k + q]; }
      c.td[k] = x * A[3] + y * A[7] + z * A[11] + (double)Pj[4 * k + 3];
      c.t[k] = (float)c.td[k];
    }
  }
  const float* Ki = a.intr + ((size_t)c.s * a.V + c.i) * 9;
  const float* Kj = a.intr + ((size_t)c.s * a.V + c.j) * 9;
  double k64[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) { k64[k] = (double)Ki[k]; c.Kj[k] = Kj[k]; }
  pose_inv3(k64, c.Kid);
}

struct PoseMatch {
  float xi[3], y[3], r3;          // x_i, R x_i + t - x_j, its norm
  float ray[3], P[3], uz, q[2];   // K_i^-1 (c, 1), depth x ray, (K_j Q)_z + eps, the projection
  float e[2], r2;                 // q - c(id_j), its norm
};

__device__ __forceinline__ void pose_match(const PoseLossArgs& a, const PoseList& c, uint32_t ia, uint32_t ib, PoseMatch& m) {
  const size_t hw = (size_t)a.H * a.W;
  const float* xi = a.xyz + ((size_t)c.s * a.V + c.i) * 3 * hw + ia;
  const float* xj = a.xyz + ((size_t)c.s * a.V + c.j) * 3 * hw + ib;
  m.xi[0] = xi[0]; m.xi[1] = xi[hw]; m.xi[2] = xi[2 * hw];
  const float xj0 = xj[0], xj1 = xj[hw], xj2 = xj[2 * hw];
  const float d = a.depth[((size_t)c.s * a.V + c.i) * hw + ia];
  const float xjv[3] = {xj0, xj1, xj2};
#pragma unroll
  for (int k = 0; k < 3; ++k) m.y[k] = c.R[3 * k] * m.xi[0] + c.R[3 * k + 1] * m.xi[1] + c.R[3 * k + 2] * m.xi[2] + c.t[k] - xjv[k];
  m.r3 = sqrtf(m.y[0] * m.y[0] + m.y[1] * m.y[1] + m.y[2] * m.y[2]);
  const uint32_t W = (uint32_t)a.W;
  const uint32_t ya = ia / W, yb = ib / W;
  const float fw = (float)a.W, fh = (float)a.H;
  const float cx = ((float)(ia - ya * W) + 0.5f) / fw, cy = ((float)ya + 0.5f) / fh;
  const float bx = ((float)(ib - yb * W) + 0.5f) / fw, by = ((float)yb + 0.5f) / fh;
  // The reprojection in fp64, from the float32 pixel centres to the residual: where the poses are near the identity q and c(id_j)
  // agree to 1e-3 and float32 would keep four digits of their difference (and of the 2D term and its gradient, list after list:
  // much of that rounding sits in Rt and K_i^-1, common to a list's matches).  What the backward reads comes out as floats.
  const double eps = 1e-6;
  double ray[3], P[3], Q[3], u[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) { ray[k] = c.Kid[3 * k] * (double)cx + c.Kid[3 * k + 1] * (double)cy + c.Kid[3 * k + 2]; P[k] = ray[k] * (double)d; }
#pragma unroll
  for (int k = 0; k < 3; ++k) Q[k] = (c.Rd[3 * k] * P[0] + c.Rd[3 * k + 1] * P[1] + c.Rd[3 * k + 2] * P[2] + c.td[k]) / (1.0 + eps);
#pragma unroll
  for (int k = 0; k < 3; ++k) u[k] = (double)c.Kj[3 * k] * Q[0] + (double)c.Kj[3 * k + 1] * Q[1] + (double)c.Kj[3 * k + 2] * Q[2];
  const double uz = u[2] + eps, q0 = u[0] / uz, q1 = u[1] / uz, e0 = q0 - (double)bx, e1 = q1 - (double)by;
#pragma unroll
  for (int k = 0; k < 3; ++k) { m.ray[k] = (float)ray[k]; m.P[k] = (float)P[k]; }
  m.uz = (float)uz;
  m.q[0] = (float)q0; m.q[1] = (float)q1;
  m.e[0] = (float)e0; m.e[1] = (float)e1;
  m.r2 = (float)sqrt(e0 * e0 + e1 * e1);
}

template <int kUnit>
__global__ __launch_bounds__(kPoseUnit) void k_pose_loss_fwd(const PoseLossArgs a) {
  __shared__ float red[3][kPoseUnit / 64];
  PoseList c;
  pose_list_of_unit(a, (int)blockIdx.x, c);
  const int tid = threadIdx.x, at = c.begin + tid;
  float sw = 0.f, s3 = 0.f, s2 = 0.f;
  if (at < c.end) {
    PoseMatch m;
    pose_match(a, c, (uint32_t)a.ids_i[at], (uint32_t)a.ids_j[at], m);
    const float w = a.wgt[at];
    sw = fabsf(w);
    s3 = w * m.r3;
    s2 = (m.r2 <= kPoseDelta ? 0.5f * m.r2 * m.r2 : kPoseDelta * (m.r2 - 0.5f * kPoseDelta)) / kPoseDelta;
  }
  sw = wave_sum(sw); s3 = wave_sum(s3); s2 = wave_sum(s2);
  if ((tid & 63) == 0) { red[0][tid >> 6] = sw; red[1][tid >> 6] = s3; red[2][tid >> 6] = s2; }
  __syncthreads();
  if (tid < kPoseFwdFloats) a.partials[(size_t)blockIdx.x * kPoseFwdFloats + tid] = tid < 3 ? red[tid][0] + red[tid][1] + red[tid][2] + red[tid][3] : 0.f;
}

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}

// One workgroup of 16 waves; wave q takes lists q, q + 16, ...: the rows of a list added in fp64 (lane k the rows k, k + 64, ...,
// then the xor tree: a fixed order), so a list's row does not depend on the other lists.  Then the first wave adds the lists the
// same way.  lists[l] = (conf L3 term, L2 term, w3d conf / (max(sum |w|, 1e-12) L), sum |w|); out = (loss, mean L3, mean L2, 0).
template <int kUnit>
__global__ __launch_bounds__(1024) void k_pose_loss_finish(const PoseLossArgs a) {
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  int first = 0;
  for (int base = 0; base < a.L; base += 16) {
    const int mine = (lane < 16 && base + lane < a.L) ? pose_units_of(a.offs[base + lane], a.offs[base + lane + 1]) : 0;
    int before = 0, total = 0, count = 0;
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const int n = __shfl(mine, q, 64);
      if (q < wv) before += n;
      if (q == wv) count = n;
      total += n;
    }
    const int l = base + wv;
    if (l < a.L) {
      const float* rows = a.partials + (size_t)(first + before) * kPoseFwdFloats;
      double sw = 0.0, s3 = 0.0, s2 = 0.0;
      for (int k = lane; k < count; k += 64) {
        const float4 v = *reinterpret_cast<const float4*>(rows + (size_t)k * kPoseFwdFloats);
        sw += (double)v.x; s3 += (double)v.y; s2 += (double)v.z;
      }
      sw = wave_sum_f64(sw); s3 = wave_sum_f64(s3); s2 = wave_sum_f64(s2);
      if (lane == 0) {
        const double conf = (double)a.conf[l], den = fmax(sw, 1e-12);
        float* o = a.lists + (size_t)l * kPoseListFloats;
        o[0] = (float)(conf * s3 / den);
        o[1] = (float)s2;
        o[2] = (float)((double)a.w3d * conf / (den * (double)a.L));
        o[3] = (float)sw;
      }
    }
    first += total;
  }
  __syncthreads();
  if (wv == 0) {
    double t3 = 0.0, t2 = 0.0;
    for (int l = lane; l < a.L; l += 64) { t3 += (double)a.lists[(size_t)l * kPoseListFloats]; t2 += (double)a.lists[(size_t)l * kPoseListFloats + 1]; }
    t3 = wave_sum_f64(t3); t2 = wave_sum_f64(t2);
    if (lane == 0) {
      const double m3 = a.L > 0 ? t3 / (double)a.L : 0.0, m2 = a.L > 0 ? t2 / (double)a.L : 0.0;
      a.out[0] = (float)((double)a.w3d * m3 + (double)a.w2d * m2);
      a.out[1] = (float)m3;
      a.out[2] = (float)m2;
      a.out[3] = 0.f;
    }
  }
}

template <int kUnit>
__global__ __launch_bounds__(kPoseUnit) void k_pose_loss_bwd(const PoseLossArgs a) {
  __shared__ float red[kPoseUnit / 64][kPoseBwdFloats];
  PoseList c;
  pose_list_of_unit(a, (int)blockIdx.x, c);
  const int tid = threadIdx.x, at = c.begin + tid;
  const float up = a.d_loss[0];
  const float f3 = up * a.lists[(size_t)c.list * kPoseListFloats + 2];  // dL / d(sum w r3) of this list
  const float f2 = up * a.w2d / (float)a.L;                             // dL / d(sum huber / delta)
  float g[kPoseBwdFloats];
#pragma unroll
  for (int k = 0; k < kPoseBwdFloats; ++k) g[k] = 0.f;
  if (at < c.end) {
    PoseMatch m;
    const uint32_t ia = (uint32_t)a.ids_i[at], ib = (uint32_t)a.ids_j[at];
    pose_match(a, c, ia, ib, m);
    const size_t hw = (size_t)a.H * a.W;
    // 3D term: w r3, r3 = |y|; the norm's gradient at y = 0 is 0
    const float s3 = m.r3 > 0.f ? f3 * a.wgt[at] / m.r3 : 0.f;
    const float gy[3] = {s3 * m.y[0], s3 * m.y[1], s3 * m.y[2]};
    // 2D term: huber(r2) / delta, r2 = |e|: d/de = e / delta on the quadratic side, e / r2 on the linear one
    const float s2 = m.r2 <= kPoseDelta ? f2 / kPoseDelta : f2 / m.r2;
    const float dq[2] = {s2 * m.e[0], s2 * m.e[1]};
    const float du[3] = {dq[0] / m.uz, dq[1] / m.uz, -(dq[0] * m.q[0] + dq[1] * m.q[1]) / m.uz};
    float dY[3], dP[3], dxi[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) dY[k] = (c.Kj[k] * du[0] + c.Kj[3 + k] * du[1] + c.Kj[6 + k] * du[2]) / (1.f + kPoseHomEps);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      dP[k] = c.R[k] * dY[0] + c.R[3 + k] * dY[1] + c.R[6 + k] * dY[2];
      dxi[k] = c.R[k] * gy[0] + c.R[3 + k] * gy[1] + c.R[6 + k] * gy[2];
    }
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
      for (int q = 0; q < 3; ++q) g[4 * r + q] = gy[r] * m.xi[q] + dY[r] * m.P[q];
      g[4 * r + 3] = gy[r] + dY[r];
    }
    float* di = a.d_xyz + ((size_t)c.s * a.V + c.i) * 3 * hw + ia;
    float* dj = a.d_xyz + ((size_t)c.s * a.V + c.j) * 3 * hw + ib;
#pragma unroll
    for (int k = 0; k < 3; ++k) { unsafeAtomicAdd(di + k * hw, dxi[k]); unsafeAtomicAdd(dj + k * hw, -gy[k]); }
    unsafeAtomicAdd(a.d_depth + ((size_t)c.s * a.V + c.i) * hw + ia, dP[0] * m.ray[0] + dP[1] * m.ray[1] + dP[2] * m.ray[2]);
  }
#pragma unroll
  for (int k = 0; k < kPoseBwdFloats; ++k) g[k] = wave_sum(g[k]);
  if ((tid & 63) == 0) {
#pragma unroll
    for (int k = 0; k < kPoseBwdFloats; ++k) red[tid >> 6][k] = g[k];
  }
  __syncthreads();
  if (tid < kPoseBwdFloats) a.partials[(size_t)blockIdx.x * kPoseBwdFloats + tid] = red[0][tid] + red[1][tid] + red[2][tid] + red[3][tid];
}

// dL/dposes (B, V, 4, 4), one wave per (scene, view u): for each pair (i, j) holding u, in the pairs' order, lane k < 12 adds
// entry k of the list's rows in fp64 (G = dL/dRt), then entry (r, c) of the view's top three rows receives
//   u == j:          (G A4^T)[r][c], A4 = P_i^-1 (the identity when i == 0: the shortcut);
//   u == i, i > 0:   -(A^T (P_j^T G)[:3] A4^T)[r][c]     (Rt = P_j P_i^-1, d(P^-1) = -P^-1 dP P^-1; rows of A4 above its last);
//   u == i == 0:     nothing (the shortcut never reads poses[s, 0]).
// The bottom row is written as zeros.
template <int kUnit>
__global__ __launch_bounds__(64) void k_pose_loss_pose_reduce(const PoseLossArgs a) {
  __shared__ double G[kPoseBwdFloats];
  const int lane = threadIdx.x, s = (int)blockIdx.x / a.V, u = (int)blockIdx.x - s * a.V;
  const int r = (lane >> 2) % 3, col = lane & 3;
  double acc = 0.0;
  const int pairs = a.V * (a.V - 1) / 2;
  for (int p = 0; p < pairs; ++p) {
    int i, j;
    pose_pair_of(p, a.V, i, j);
    if (i != u && j != u) continue;  // (uniform)
    const int l = p * a.B + s;
    int before = 0;
    for (int q = lane; q < l; q += 64) before += pose_units_of(a.offs[q], a.offs[q + 1]);
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) before += __shfl_xor(before, m, 64);
    const int count = pose_units_of(a.offs[l], a.offs[l + 1]);
    __syncthreads();
    if (lane < kPoseBwdFloats) {
      double sum = 0.0;
      const float* rows = a.partials + (size_t)before * kPoseBwdFloats + lane;
      for (int k = 0; k < count; ++k) sum += (double)rows[(size_t)k * kPoseBwdFloats];
      G[lane] = sum;
    }
    __syncthreads();
    if (i == 0) {
      if (u == j) acc += G[4 * r + col];
      continue;
    }
    double A[16];
    pose_affine_inverse(a.poses + ((size_t)s * a.V + i) * 16, A);
    A[12] = 0.0; A[13] = 0.0; A[14] = 0.0; A[15] = 1.0;
    if (u == j) {
#pragma unroll
      for (int m = 0; m < 4; ++m) acc += G[4 * r + m] * A[4 * col + m];
    } else {
      const float* Pj = a.poses + ((size_t)s * a.V + j) * 16;
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        double t = 0.0;  // (dA A4^T)[k][col], dA[k][m] = sum_q P_j[q][k] G[q][m]
#pragma unroll
        for (int m = 0; m < 4; ++m) {
          const double dA = (double)Pj[k] * G[m] + (double)Pj[4 + k] * G[4 + m] + (double)Pj[8 + k] * G[8 + m];
          t += dA * A[4 * col + m];
        }
        acc -= A[4 * k + r] * t;
      }
    }
  }
  if (lane < 16) a.d_poses[(size_t)blockIdx.x * 16 + lane] = lane < 12 ? (float)acc : 0.f;
}

// Host side: the unit count of a set of lists, -1 for offsets that are not a monotone sequence from a non-negative start.
static int64_t pose_units_host(int num_lists, const int32_t* offsets) {
  if (num_lists < 0 || !offsets || offsets[0] < 0) return -1;
  int64_t units = 0;
  for (int l = 0; l < num_lists; ++l) {
    if (offsets[l + 1] < offsets[l]) return -1;
    units += ((int64_t)offsets[l + 1] - offsets[l] + kPoseUnit - 1) / kPoseUnit;
  }
  return units;
}

// Everything the two entry points check alike; the unit count, or -1.
static int64_t pose_args_ok(int B, int V, int H, int W, int pairs, const void* xyz, const void* depth, const void* poses, const void* intr,
                            const void* ids_i, const void* ids_j, const void* wgt, const void* conf, const int32_t* offsets, const void* offsets_dev) {
  if (B < 0 || V < 2 || H <= 0 || W <= 0 || (int64_t)H * W > 0x7fffffff || (int64_t)V * (V - 1) / 2 != pairs) return -1;
  if ((int64_t)B * pairs > 0x7fffff || (int64_t)B * V > 0x7fffffff) return -1;
  if (!offsets) return -1;
  const int L = B * pairs;
  const int64_t units = pose_units_host(L, offsets);
  if (units < 0 || units > 0x7fffffff) return -1;
  if (L > 0 && (!xyz || !depth || !poses || !intr || !conf || !offsets_dev)) return -1;
  if (L > 0 && offsets[L] > offsets[0] && (!ids_i || !ids_j || !wgt)) return -1;
  return units;
}
}  // namespace gsr

extern "C" {

int64_t gsr_pose_loss_units(int num_lists, const int32_t* offsets) { return gsr::pose_units_host(num_lists, offsets); }

int gsr_pose_loss(int num_scenes, int num_views, int height, int width, int num_pairs, const float* xyz, const float* depth, const float* poses,
                  const float* intrinsics, const int64_t* ids_i, const int64_t* ids_j, const float* weights, const float* conf,
                  const int32_t* offsets, const int32_t* offsets_device, float weight_2d, float weight_3d, float* partials, float* lists,
                  float* out, void* stream_) {
  using namespace gsr;
  const int64_t units = pose_args_ok(num_scenes, num_views, height, width, num_pairs, xyz, depth, poses, intrinsics, ids_i, ids_j, weights, conf,
                                     offsets, offsets_device);
  if (units < 0 || !out || (num_scenes > 0 && !lists) || (units > 0 && !partials)) return GSR_ERR_INVALID_ARGUMENT;
  hipStream_t st = static_cast<hipStream_t>(stream_);
  PoseLossArgs a{};
  a.B = num_scenes; a.V = num_views; a.H = height; a.W = width; a.L = num_scenes * num_pairs;
  a.xyz = xyz; a.depth = depth; a.poses = poses; a.intr = intrinsics; a.ids_i = ids_i; a.ids_j = ids_j; a.wgt = weights; a.conf = conf;
  a.offs = offsets_device; a.w2d = weight_2d; a.w3d = weight_3d; a.partials = partials; a.lists = lists; a.out = out;
  if (units > 0) {
    hipLaunchKernelGGL(k_pose_loss_fwd<kPoseUnit>, dim3((unsigned)units), dim3(kPoseUnit), 0, st, a);
    GSR_CHECK(hipGetLastError());
  }
  hipLaunchKernelGGL(k_pose_loss_finish<kPoseUnit>, dim3(1), dim3(1024), 0, st, a);
  GSR_CHECK(hipGetLastError());
  return GSR_OK;
}

int gsr_pose_loss_backward(int num_scenes, int num_views, int height, int width, int num_pairs, const float* xyz, const float* depth,
                           const float* poses, const float* intrinsics, const int64_t* ids_i, const int64_t* ids_j, const float* weights,
                           const float* conf, const int32_t* offsets, const int32_t* offsets_device, float weight_2d, float weight_3d,
                           const float* lists, const float* dL_dloss, float* dL_dxyz, float* dL_ddepth, float* dL_dposes, float* partials,
                           void* stream_) {
  using namespace gsr;
  const int64_t units = pose_args_ok(num_scenes, num_views, height, width, num_pairs, xyz, depth, poses, intrinsics, ids_i, ids_j, weights, conf,
                                     offsets, offsets_device);
  if (units < 0 || (units > 0 && !partials)) return GSR_ERR_INVALID_ARGUMENT;
  if (num_scenes == 0) return GSR_OK;
  if (!lists || !dL_dloss || !dL_dxyz || !dL_ddepth || !dL_dposes) return GSR_ERR_INVALID_ARGUMENT;
  hipStream_t st = static_cast<hipStream_t>(stream_);
  PoseLossArgs a{};
  a.B = num_scenes; a.V = num_views; a.H = height; a.W = width; a.L = num_scenes * num_pairs;
  a.xyz = xyz; a.depth = depth; a.poses = poses; a.intr = intrinsics; a.ids_i = ids_i; a.ids_j = ids_j; a.wgt = weights; a.conf = conf;
  a.offs = offsets_device; a.w2d = weight_2d; a.w3d = weight_3d; a.partials = partials; a.lists = const_cast<float*>(lists);
  a.d_loss = dL_dloss; a.d_xyz = dL_dxyz; a.d_depth = dL_ddepth; a.d_poses = dL_dposes;
  const size_t pixels = (size_t)num_scenes * num_views * height * width;
  GSR_CHECK(hipMemsetAsync(dL_dxyz, 0, pixels * 3 * sizeof(float), st));
  GSR_CHECK(hipMemsetAsync(dL_ddepth, 0, pixels * sizeof(float), st));
  if (units > 0) {
    hipLaunchKernelGGL(k_pose_loss_bwd<kPoseUnit>, dim3((unsigned)units), dim3(kPoseUnit), 0, st, a);
    GSR_CHECK(hipGetLastError());
  }
  hipLaunchKernelGGL(k_pose_loss_pose_reduce<kPoseUnit>, dim3((unsigned)(num_scenes * num_views)), dim3(64), 0, st, a);
  GSR_CHECK(hipGetLastError());
  return GSR_OK;
}

}  // extern "C"
