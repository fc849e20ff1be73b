#pragma once
// Camera set-up kernels and their entry points.
#include "gsr_common.h"

namespace gsr {

// ------------------------------------------------------------------------------------------------
// Camera set-up: what the reference wrapper does with ~40 tiny torch launches per call (cuda_splatting.py:64-71, 80-87:
// scale-invariant rescale, get_fov, get_projection_matrix, extrinsics.inverse(), view @ proj) in ONE launch, one
// thread per view, straight into the GsrView records the raster kernels read.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool inv3(const float* m, float* o) {
  const float c00 = m[4] * m[8] - m[5] * m[7], c01 = m[5] * m[6] - m[3] * m[8], c02 = m[3] * m[7] - m[4] * m[6];
  const float det = m[0] * c00 + m[1] * c01 + m[2] * c02;
  const float id = 1.f / det;
  o[0] = c00 * id; o[1] = (m[2] * m[7] - m[1] * m[8]) * id; o[2] = (m[1] * m[5] - m[2] * m[4]) * id;
  o[3] = c01 * id; o[4] = (m[0] * m[8] - m[2] * m[6]) * id; o[5] = (m[2] * m[3] - m[0] * m[5]) * id;
  o[6] = c02 * id; o[7] = (m[1] * m[6] - m[0] * m[7]) * id; o[8] = (m[0] * m[4] - m[1] * m[3]) * id;
  return det != 0.f;
}
__device__ __forceinline__ void inv4(const float* m, float* inv) {  // general 4x4 inverse by cofactors
  inv[0] = m[5] * m[10] * m[15] - m[5] * m[11] * m[14] - m[9] * m[6] * m[15] + m[9] * m[7] * m[14] + m[13] * m[6] * m[11] - m[13] * m[7] * m[10];
  inv[4] = -m[4] * m[10] * m[15] + m[4] * m[11] * m[14] + m[8] * m[6] * m[15] - m[8] * m[7] * m[14] - m[12] * m[6] * m[11] + m[12] * m[7] * m[10];
  inv[8] = m[4] * m[9] * m[15] - m[4] * m[11] * m[13] - m[8] * m[5] * m[15] + m[8] * m[7] * m[13] + m[12] * m[5] * m[11] - m[12] * m[7] * m[9];
  inv[12] = -m[4] * m[9] * m[14] + m[4] * m[10] * m[13] + m[8] * m[5] * m[14] - m[8] * m[6] * m[13] - m[12] * m[5] * m[10] + m[12] * m[6] * m[9];
  inv[1] = -m[1] * m[10] * m[15] + m[1] * m[11] * m[14] + m[9] * m[2] * m[15] - m[9] * m[3] * m[14] - m[13] * m[2] * m[11] + m[13] * m[3] * m[10];
  inv[5] = m[0] * m[10] * m[15] - m[0] * m[11] * m[14] - m[8] * m[2] * m[15] + m[8] * m[3] * m[14] + m[12] * m[2] * m[11] - m[12] * m[3] * m[10];
  inv[9] = -m[0] * m[9] * m[15] + m[0] * m[11] * m[13] + m[8] * m[1] * m[15] - m[8] * m[3] * m[13] - m[12] * m[1] * m[11] + m[12] * m[3] * m[9];
  inv[13] = m[0] * m[9] * m[14] - m[0] * m[10] * m[13] - m[8] * m[1] * m[14] + m[8] * m[2] * m[13] + m[12] * m[1] * m[10] - m[12] * m[2] * m[9];
  inv[2] = m[1] * m[6] * m[15] - m[1] * m[7] * m[14] - m[5] * m[2] * m[15] + m[5] * m[3] * m[14] + m[13] * m[2] * m[7] - m[13] * m[3] * m[6];
  inv[6] = -m[0] * m[6] * m[15] + m[0] * m[7] * m[14] + m[4] * m[2] * m[15] - m[4] * m[3] * m[14] - m[12] * m[2] * m[7] + m[12] * m[3] * m[6];
  inv[10] = m[0] * m[5] * m[15] - m[0] * m[7] * m[13] - m[4] * m[1] * m[15] + m[4] * m[3] * m[13] + m[12] * m[1] * m[7] - m[12] * m[3] * m[5];
  inv[14] = -m[0] * m[5] * m[14] + m[0] * m[6] * m[13] + m[4] * m[1] * m[14] - m[4] * m[2] * m[13] - m[12] * m[1] * m[6] + m[12] * m[2] * m[5];
  inv[3] = -m[1] * m[6] * m[11] + m[1] * m[7] * m[10] + m[5] * m[2] * m[11] - m[5] * m[3] * m[10] - m[9] * m[2] * m[7] + m[9] * m[3] * m[6];
  inv[7] = m[0] * m[6] * m[11] - m[0] * m[7] * m[10] - m[4] * m[2] * m[11] + m[4] * m[3] * m[10] + m[8] * m[2] * m[7] - m[8] * m[3] * m[6];
  inv[11] = -m[0] * m[5] * m[11] + m[0] * m[7] * m[9] + m[4] * m[1] * m[11] - m[4] * m[3] * m[9] - m[8] * m[1] * m[7] + m[8] * m[3] * m[5];
  inv[15] = m[0] * m[5] * m[10] - m[0] * m[6] * m[9] - m[4] * m[1] * m[10] + m[4] * m[2] * m[9] + m[8] * m[1] * m[6] - m[8] * m[2] * m[5];
  const float det = m[0] * inv[0] + m[1] * inv[4] + m[2] * inv[8] + m[3] * inv[12];
  const float id = 1.f / det;
#pragma unroll
  for (int i = 0; i < 16; ++i) inv[i] *= id;
}

// Camera record from a camera-to-world matrix E (already rescaled / moved), clip distances and the tangents: `tpx, tpy`
// shape the projection matrix (get_projection_matrix, cuda_splatting.py:17-44), `tx, ty` are what the rasterizer is told.
__device__ __forceinline__ void finish_view(const float* E, float nr, float fr, float tpx, float tpy, float tx, float ty, float s,
                                            const float* bg, float near_raw, float far_raw, GsrView& o) {
  const float top = tpy * nr, right = tpx * nr;
  float P[16] = {0};
  P[0] = 2.f * nr / (right + right); P[5] = 2.f * nr / (top + top); P[14] = 1.f;
  P[10] = fr / (fr - nr); P[11] = -(fr * nr) / (fr - nr);
  float Ei[16];
  inv4(E, Ei);
  // viewmatrix = (E^-1)^T, projmatrix = (E^-1)^T P^T, both stored row-major (cuda_splatting.py:85-87)
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      o.viewmatrix[4 * i + j] = Ei[4 * j + i];
      float a = 0.f;
#pragma unroll
      for (int k = 0; k < 4; ++k) a += Ei[4 * k + i] * P[4 * j + k];
      o.projmatrix[4 * i + j] = a;
    }
  o.campos[0] = E[3]; o.campos[1] = E[7]; o.campos[2] = E[11];
  o.tanfovx = tx; o.tanfovy = ty;
  o.bg[0] = bg[0]; o.bg[1] = bg[1]; o.bg[2] = bg[2];
  o.scale = s; o.scale2 = s * s; o.scale_modifier = 1.f;
  o.reserved[0] = near_raw; o.reserved[1] = far_raw;  // un-normalised near / far (built-in relative-disparity / log extra channel)
#pragma unroll
  for (int i = 2; i < 5; ++i) o.reserved[i] = 0.f;
}

__global__ void k_setup_views(int V, const float* ext, const float* intr, const float* near_, const float* far_, const float* bg,
                              int bg_stride, int scale_invariant, GsrView* out) {
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= V) return;
  float E[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) E[i] = ext[16 * v + i];
  float nr = near_[v], fr = far_[v];
  const float s = scale_invariant ? 1.f / nr : 1.f;
  if (scale_invariant) { E[3] *= s; E[7] *= s; E[11] *= s; nr = nr * s; fr = fr * s; }
  // get_fov (projection.py:233-247): angle between the un-projected edge-midpoint rays
  float Ki[9];
  inv3(intr + 9 * v, Ki);
  auto ray = [&](float x, float y, float* o) {
    o[0] = Ki[0] * x + Ki[1] * y + Ki[2]; o[1] = Ki[3] * x + Ki[4] * y + Ki[5]; o[2] = Ki[6] * x + Ki[7] * y + Ki[8];
    const float n = sqrtf(o[0] * o[0] + o[1] * o[1] + o[2] * o[2]);
    o[0] /= n; o[1] /= n; o[2] /= n;
  };
  float l[3], r[3], t[3], b[3];
  ray(0.f, 0.5f, l); ray(1.f, 0.5f, r); ray(0.5f, 0.f, t); ray(0.5f, 1.f, b);
  const float fov_x = acosf(l[0] * r[0] + l[1] * r[1] + l[2] * r[2]);
  const float fov_y = acosf(t[0] * b[0] + t[1] * b[1] + t[2] * b[2]);
  const float tx = tanf(0.5f * fov_x), ty = tanf(0.5f * fov_y);
  GsrView o;
  finish_view(E, nr, fr, tx, ty, tx, ty, s, bg + bg_stride * v, near_[v], far_[v], o);
  out[v] = o;
}

// The reference's fake orthographic camera (render_cuda_orthographic, cuda_splatting.py:153-181): the camera moves back
// along its own -z by d = (width / 2) / tan(fov_x / 2) with a narrow fov_x, near and far move with it, no scale-invariant
// step.  Quirk kept (:160): the projection's y scale comes from fov_y = atan(2 tan_fov_y) while the rasterizer is told
// tan_fov_y itself.  `dump` (optional, 20 floats per view): the moved extrinsics, fov_x, fov_y, near, far - the wrapper's
// `dump` dict.
__global__ void k_setup_views_ortho(int V, const float* ext, const float* width, const float* height, const float* near_,
                                    const float* far_, const float* bg, int bg_stride, float fov_degrees, GsrView* out, float* dump) {
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= V) return;
  const float fov_x = fov_degrees * 0.017453292519943295f;
  const float tx = tanf(0.5f * fov_x);
  const float dist = (0.5f * width[v]) / tx;
  const float ty = 0.5f * height[v] / dist;
  const float fov_y = atanf(2.f * ty);
  const float nr = near_[v] + dist, fr = far_[v] + dist;
  float E[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) E[i] = ext[16 * v + i];
#pragma unroll
  for (int i = 0; i < 4; ++i) E[4 * i + 3] = E[4 * i + 2] * -dist + E[4 * i + 3];  // E @ [I | (0, 0, -d)]
  GsrView o;
  finish_view(E, nr, fr, tx, tanf(0.5f * fov_y), tx, ty, 1.f, bg + bg_stride * v, nr, fr, o);
  out[v] = o;
  if (dump) {
    float* dp = dump + 20 * v;
#pragma unroll
    for (int i = 0; i < 16; ++i) dp[i] = E[i];
    dp[16] = fov_x; dp[17] = fov_y; dp[18] = nr; dp[19] = fr;
  }
}

// Backward of k_setup_views: the gradient of the (V, 48) camera records (as gsr_backward_ex returns it: d viewmatrix [0, 16),
// d projmatrix [16, 32), d campos [32, 35)) carried to the (V, 4, 4) camera-to-world extrinsics, one thread per view, in fp64:
//   view = (E'^-1)^T,  full = view P^T,  campos = E'[:3, 3]   with E' = E, translation times s (the scale-invariant factor)
//   => dL/dview += dL/dfull P;  dL/dE' = -(E'^-1)^T (dL/d(E'^-1)) (E'^-1)^T;  translation column += dL/dcampos, then times s.
// Intrinsics, near and far get nothing here (the intrinsics' share: k_setup_views_bwd_ex below).  What the Python layer used to do
// with a dozen fp64 torch launches per backward (190 us of device time for three cameras) is one ~3 us launch.
__global__ void k_setup_views_bwd(int V, const GsrView* views, const float* d_views, float* d_ext) {
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= V) return;
  const GsrView& c = views[v];
  const float* g = d_views + (size_t)v * 48;
  const double s = c.scale, nr = (double)c.reserved[0] * s, fr = (double)c.reserved[1] * s;
  double P[16] = {0};  // the projection matrix of finish_view (row-major)
  P[0] = 1.0 / c.tanfovx; P[5] = 1.0 / c.tanfovy; P[14] = 1.0;
  P[10] = fr / (fr - nr); P[11] = -(fr * nr) / (fr - nr);
  // A = E'^-1 (world -> camera); the record holds A^T:  A[i][j] = viewmatrix[4 j + i]
  double A[16], dV[16], dA[16];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) A[4 * i + j] = c.viewmatrix[4 * j + i];
  // dL/dview = dL/dviewmatrix + dL/dprojmatrix P   (full = view P^T, both stored transposed)
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      double a = g[4 * i + j];
#pragma unroll
      for (int k = 0; k < 4; ++k) a += (double)g[16 + 4 * i + k] * P[4 * k + j];
      dV[4 * i + j] = a;
    }
  // view = A^T  =>  dL/dA = (dL/dview)^T
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) dA[4 * i + j] = dV[4 * j + i];
  // A = E'^-1  =>  dL/dE' = -A^T dA A^T
  double T[16];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      double a = 0.0;
#pragma unroll
      for (int k = 0; k < 4; ++k) a += A[4 * k + i] * dA[4 * k + j];  // (A^T dA)[i][j]
      T[4 * i + j] = a;
    }
  float* o = d_ext + (size_t)v * 16;
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      double a = 0.0;
#pragma unroll
      for (int k = 0; k < 4; ++k) a += T[4 * i + k] * A[4 * j + k];  // (T A^T)[i][j]
      a = -a;
      if (j == 3 && i < 3) a = (a + (double)g[32 + i]) * s;
      o[4 * i + j] = (float)a;
    }
}

// The body of k_setup_views_bwd once more, for k_setup_views_bwd_ex: the same expressions in the same order, hence the same bits.  (The
// kernel above keeps its own text: called through a shared function it compiled to other instructions - commuted operands.)
__device__ __forceinline__ void setup_views_bwd_ext(const GsrView& c, const float* g, float* o) {
  const double s = c.scale, nr = (double)c.reserved[0] * s, fr = (double)c.reserved[1] * s;
  double P[16] = {0};  // the projection matrix of finish_view (row-major)
  P[0] = 1.0 / c.tanfovx; P[5] = 1.0 / c.tanfovy; P[14] = 1.0;
  P[10] = fr / (fr - nr); P[11] = -(fr * nr) / (fr - nr);
  // A = E'^-1 (world -> camera); the record holds A^T:  A[i][j] = viewmatrix[4 j + i]
  double A[16], dV[16], dA[16];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) A[4 * i + j] = c.viewmatrix[4 * j + i];
  // dL/dview = dL/dviewmatrix + dL/dprojmatrix P   (full = view P^T, both stored transposed)
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      double a = g[4 * i + j];
#pragma unroll
      for (int k = 0; k < 4; ++k) a += (double)g[16 + 4 * i + k] * P[4 * k + j];
      dV[4 * i + j] = a;
    }
  // view = A^T  =>  dL/dA = (dL/dview)^T
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) dA[4 * i + j] = dV[4 * j + i];
  // A = E'^-1  =>  dL/dE' = -A^T dA A^T
  double T[16];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      double a = 0.0;
#pragma unroll
      for (int k = 0; k < 4; ++k) a += A[4 * k + i] * dA[4 * k + j];  // (A^T dA)[i][j]
      T[4 * i + j] = a;
    }
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      double a = 0.0;
#pragma unroll
      for (int k = 0; k < 4; ++k) a += T[4 * i + k] * A[4 * j + k];  // (T A^T)[i][j]
      a = -a;
      if (j == 3 && i < 3) a = (a + (double)g[32 + i]) * s;
      o[4 * i + j] = (float)a;
    }
}

// gsr_setup_views_backward_ex: the same (d_ext, nullable) and the intrinsics' share (d_intr, nullable) in one launch, one thread per
// view, fp64.  The two tangents of k_setup_views, tx = tan(acos(l . r) / 2) over the normalised edge-midpoint rays K^-1 (x, y, 1),
// receive  g[35] + dL/dP[0][0] (-1 / tx^2)  and  g[36] + dL/dP[1][1] (-1 / ty^2):  their own slots (GSR_FLAG_FOV_GRADIENT) and what
// the projection block sends through P[0][0] = 1 / tx, P[1][1] = 1 / ty (full = view P^T => dL/dP[a][a] = sum_i g[16 + 4 i + a]
// view[4 i + a]).  Back through tan, acos, the two normalisations and K^-1 (dL/dK = -K^-T dL/dK^-1 K^-T), everything recomputed from
// the intrinsics in fp64.  Near, far, background and scale get nothing.
__global__ void k_setup_views_bwd_ex(int V, const GsrView* views, const float* intr, const float* d_views, float* d_ext, float* d_intr) {
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= V) return;
  const GsrView& c = views[v];
  const float* g = d_views + (size_t)v * 48;
  if (d_ext) setup_views_bwd_ext(c, g, d_ext + (size_t)v * 16);
  if (!d_intr) return;
  double K[9], Ki[9];
#pragma unroll
  for (int i = 0; i < 9; ++i) K[i] = intr[9 * v + i];
  {
    const double c00 = K[4] * K[8] - K[5] * K[7], c01 = K[5] * K[6] - K[3] * K[8], c02 = K[3] * K[7] - K[4] * K[6];
    const double id = 1.0 / (K[0] * c00 + K[1] * c01 + K[2] * c02);
    Ki[0] = c00 * id; Ki[1] = (K[2] * K[7] - K[1] * K[8]) * id; Ki[2] = (K[1] * K[5] - K[2] * K[4]) * id;
    Ki[3] = c01 * id; Ki[4] = (K[0] * K[8] - K[2] * K[6]) * id; Ki[5] = (K[2] * K[3] - K[0] * K[5]) * id;
    Ki[6] = c02 * id; Ki[7] = (K[1] * K[6] - K[0] * K[7]) * id; Ki[8] = (K[0] * K[4] - K[1] * K[3]) * id;
  }
  double dKi[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  // one field of view: the rays through (x0, y0) and (x1, y1), its slot gslot and dL/dP[a][a]
  auto edge = [&](double x0, double y0, double x1, double y1, double gslot, double dP) {
    const double p0[3] = {x0, y0, 1.0}, p1[3] = {x1, y1, 1.0};
    double a0[3], a1[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      a0[i] = Ki[3 * i] * p0[0] + Ki[3 * i + 1] * p0[1] + Ki[3 * i + 2];
      a1[i] = Ki[3 * i] * p1[0] + Ki[3 * i + 1] * p1[1] + Ki[3 * i + 2];
    }
    const double n0 = sqrt(a0[0] * a0[0] + a0[1] * a0[1] + a0[2] * a0[2]), n1 = sqrt(a1[0] * a1[0] + a1[1] * a1[1] + a1[2] * a1[2]);
#pragma unroll
    for (int i = 0; i < 3; ++i) { a0[i] /= n0; a1[i] /= n1; }
    const double cs = a0[0] * a1[0] + a0[1] * a1[1] + a0[2] * a1[2];
    const double t = tan(0.5 * acos(cs));
    const double gt = gslot + dP * (-1.0 / (t * t));
    const double gc = gt * (-0.5 * (1.0 + t * t) / sqrt(1.0 - cs * cs));  // d tan(acos(c) / 2) / dc
#pragma unroll
    for (int i = 0; i < 3; ++i) {  // through the normalisations: d(u / |u|) = (I - a a^T) / |u|
      const double du0 = gc * (a1[i] - a0[i] * cs) / n0, du1 = gc * (a0[i] - a1[i] * cs) / n1;
#pragma unroll
      for (int j = 0; j < 3; ++j) dKi[3 * i + j] += du0 * p0[j] + du1 * p1[j];
    }
  };
  double dP[2] = {0.0, 0.0};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    dP[0] += (double)g[16 + 4 * i] * (double)c.viewmatrix[4 * i];
    dP[1] += (double)g[16 + 4 * i + 1] * (double)c.viewmatrix[4 * i + 1];
  }
  edge(0.0, 0.5, 1.0, 0.5, (double)g[35], dP[0]);
  edge(0.5, 0.0, 0.5, 1.0, (double)g[36], dP[1]);
  float* o = d_intr + (size_t)v * 9;
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) {  // dL/dK = -Ki^T dKi Ki^T
      double a = 0.0;
#pragma unroll
      for (int p = 0; p < 3; ++p)
#pragma unroll
        for (int q = 0; q < 3; ++q) a += Ki[3 * p + i] * dKi[3 * p + q] * Ki[3 * j + q];
      o[3 * i + j] = (float)-a;
    }
}

// One record of the per-view API (gsr_pack_view): thread k writes float k.
__global__ __launch_bounds__(64) void k_pack_view(const float* vm, const float* pm, const float* campos, int cstride, const float* bg,
                                                  float tx, float ty, const float* txd, const float* tyd, float smod, float* out) {
  const int k = threadIdx.x;
  if (k >= 48) return;
  float v = 0.f;
  if (k < 16) v = vm[k];
  else if (k < 32) v = pm[k - 16];
  else if (k < 35) v = campos[(size_t)(k - 32) * cstride];
  else if (k == 35) v = txd ? *txd : tx;
  else if (k == 36) v = tyd ? *tyd : ty;
  else if (k < 40) v = bg[k - 37];
  else if (k < 42) v = 1.f;  // scale, scale^2
  else if (k == 42) v = smod;
  out[k] = v;
}

__global__ __launch_bounds__(256) void k_mark_visible(const Params p, uint8_t* present) {
  const int set = blockIdx.y;
  const int i = blockIdx.x * 256 + threadIdx.x;
  const int N = p.d.num_gaussians;
  if (i >= N) return;
  const GsrView& cam = p.views[set * p.d.views_per_set];
  const size_t gi = (size_t)set * N + i;
  const float mx = p.means[3 * gi] * cam.scale, my = p.means[3 * gi + 1] * cam.scale, mz = p.means[3 * gi + 2] * cam.scale;
  const float* vm = cam.viewmatrix;
  const float pvz = vm[2] * mx + vm[6] * my + vm[10] * mz + vm[14];
  present[gi] = !(pvz <= kNear) ? 1 : 0;
}

}  // namespace gsr

using namespace gsr;  // (as in gsr_hip.hip; the library is one translation unit)

extern "C" {

int gsr_setup_views(int num_views, const float* extrinsics, const float* intrinsics, const float* near_, const float* far_,
                    const float* background, int background_stride, int scale_invariant, GsrView* views, void* stream_) {
  if (num_views < 0 || (background_stride != 0 && background_stride != 3)) return GSR_ERR_INVALID_ARGUMENT;
  if (num_views == 0) return GSR_OK;
  if (!extrinsics || !intrinsics || !near_ || !far_ || !background || !views) return GSR_ERR_INVALID_ARGUMENT;
  hipLaunchKernelGGL(k_setup_views, dim3((unsigned)((num_views + 63) / 64)), dim3(64), 0, static_cast<hipStream_t>(stream_),
                     num_views, extrinsics, intrinsics, near_, far_, background, background_stride, scale_invariant, views);
  GSR_CHECK(hipGetLastError());
  return GSR_OK;
}

int gsr_setup_views_backward(int num_views, const GsrView* views, const float* dL_dviews, float* dL_dextrinsics, void* stream_) {
  if (num_views < 0) return GSR_ERR_INVALID_ARGUMENT;
  if (num_views == 0) return GSR_OK;
  if (!views || !dL_dviews || !dL_dextrinsics) return GSR_ERR_INVALID_ARGUMENT;
  hipLaunchKernelGGL(k_setup_views_bwd, dim3((unsigned)((num_views + 63) / 64)), dim3(64), 0, static_cast<hipStream_t>(stream_),
                     num_views, views, dL_dviews, dL_dextrinsics);
  GSR_CHECK(hipGetLastError());
  return GSR_OK;
}

int gsr_setup_views_backward_ex(int num_views, const GsrView* views, const float* intrinsics, const float* dL_dviews, float* dL_dextrinsics,
                                float* dL_dintrinsics, void* stream_) {
  if (num_views < 0) return GSR_ERR_INVALID_ARGUMENT;
  if (num_views == 0) return GSR_OK;
  if (!views || !intrinsics || !dL_dviews) return GSR_ERR_INVALID_ARGUMENT;
  hipLaunchKernelGGL(k_setup_views_bwd_ex, dim3((unsigned)((num_views + 63) / 64)), dim3(64), 0, static_cast<hipStream_t>(stream_),
                     num_views, views, intrinsics, dL_dviews, dL_dextrinsics, dL_dintrinsics);
  GSR_CHECK(hipGetLastError());
  return GSR_OK;
}

int gsr_setup_views_orthographic(int num_views, const float* extrinsics, const float* width, const float* height, const float* near_,
                                 const float* far_, const float* background, int background_stride, float fov_degrees,
                                 GsrView* views, float* dump, void* stream_) {
  if (num_views < 0 || (background_stride != 0 && background_stride != 3) || !(fov_degrees > 0.f)) return GSR_ERR_INVALID_ARGUMENT;
  if (num_views == 0) return GSR_OK;
  if (!extrinsics || !width || !height || !near_ || !far_ || !background || !views) return GSR_ERR_INVALID_ARGUMENT;
  hipLaunchKernelGGL(k_setup_views_ortho, dim3((unsigned)((num_views + 63) / 64)), dim3(64), 0, static_cast<hipStream_t>(stream_),
                     num_views, extrinsics, width, height, near_, far_, background, background_stride, fov_degrees, views, dump);
  GSR_CHECK(hipGetLastError());
  return GSR_OK;
}

int gsr_pack_view(const float* viewmatrix, const float* projmatrix, const float* campos, int campos_stride, const float* bg,
                  float tanfovx, float tanfovy, const float* tanfovx_dev, const float* tanfovy_dev, float scale_modifier,
                  GsrView* out, void* stream_) {
  if (!viewmatrix || !projmatrix || !campos || !bg || !out || campos_stride < 1) return GSR_ERR_INVALID_ARGUMENT;
  hipLaunchKernelGGL(k_pack_view, dim3(1), dim3(64), 0, static_cast<hipStream_t>(stream_), viewmatrix, projmatrix, campos,
                     campos_stride, bg, tanfovx, tanfovy, tanfovx_dev, tanfovy_dev, scale_modifier, reinterpret_cast<float*>(out));
  GSR_CHECK(hipGetLastError());
  return GSR_OK;
}

}  // extern "C"
