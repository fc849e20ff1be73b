#pragma once
// ------------------------------------------------------------------------------------------------
// Coarse camera poses (include/gsr.h states the definition): PnP RANSAC per match list - a P3P hypothesis per lane, scored by the
// workgroup over points staged in LDS, the winner refined by Gauss-Newton on its consensus set - and the synchronisation of the
// pairwise poses (gsr_pnp_ransac, gsr_camera_sync).  The minimal solver and the Gauss-Newton step are host + device functions
// (namespace gsr::pnp) that a host program can check in fp64 without a GPU: this header is that arithmetic alone and needs nothing
// else - a host compiler gets plain inline functions, hipcc host + device ones.  The kernels and entry points: gsr_coarse_pose.h.
// ------------------------------------------------------------------------------------------------
#include <cmath>
#include <cstdint>
#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define GSR_HD __host__ __device__ inline
#else
#define GSR_HD inline
#endif

namespace gsr {
namespace pnp {

constexpr int kMinMatches = 4;     // three matches for the P3P solve and one to choose among its poses
constexpr int kRefineRounds = 3;   // consensus set, then kGnSteps Gauss-Newton steps on it
constexpr int kGnSteps = 10;
constexpr int kJacobiSweeps = 8;   // of the 3 x 3 one-sided Jacobi SVD
constexpr int kSquarings = 10;
constexpr int kMaxViews = 8;

struct Pose {
  double R[9];  // row-major
  double t[3];
};

GSR_HD uint32_t fmix32(uint32_t x) {
  x ^= x >> 16; x *= 0x85EBCA6Bu; x ^= x >> 13; x *= 0xC2B2AE35u; x ^= x >> 16;
  return x;
}

// The draw of hypothesis t's slot (0..3) in list l: three rounds of murmur3's finaliser; the index is draw % n.
GSR_HD uint32_t draw(uint32_t seed, uint32_t l, uint32_t t, uint32_t slot) {
  uint32_t x = fmix32(seed ^ (0x9E3779B9u * (l + 1u)));
  x = fmix32(x ^ (0x85EBCA6Bu * (t + 1u)));
  return fmix32(x ^ (0xC2B2AE35u * (slot + 1u)));
}

// The largest real root of x^3 + a2 x^2 + a1 x + a0 (closed form, then three Newton steps).
GSR_HD double cubic_largest_root(double a2, double a1, double a0) {
  const double Q = (3.0 * a1 - a2 * a2) / 9.0, R = (9.0 * a2 * a1 - 27.0 * a0 - 2.0 * a2 * a2 * a2) / 54.0;
  const double D = Q * Q * Q + R * R;
  double x;
  if (D < 0.0) {  // three real roots
    const double sq = sqrt(-Q);
    double c = R / (sq * sq * sq);
    c = c > 1.0 ? 1.0 : (c < -1.0 ? -1.0 : c);
    x = 2.0 * sq * cos(acos(c) / 3.0) - a2 / 3.0;
  } else {
    const double s = sqrt(D);
    x = cbrt(R + s) + cbrt(R - s) - a2 / 3.0;
  }
  for (int it = 0; it < 3; ++it) {
    const double f = ((x + a2) * x + a1) * x + a0, d = (3.0 * x + 2.0 * a2) * x + a1;
    if (fabs(d) > 1e-300) x -= f / d;
  }
  return x;
}

// The real roots of c[4] y^4 + ... + c[0] by Ferrari's resolvent, each polished by two Newton steps; their number (0..4).
GSR_HD int quartic_real_roots(const double c[5], double roots[4]) {
  const double B = c[3] / c[4], C = c[2] / c[4], D = c[1] / c[4], E = c[0] / c[4];
  const double B2 = B * B;
  const double p = C - 0.375 * B2, q = D - 0.5 * B * C + 0.125 * B2 * B, r = E - 0.25 * B * D + B2 * C / 16.0 - 3.0 * B2 * B2 / 256.0;
  const double m = cubic_largest_root(p, 0.25 * p * p - r, -0.125 * q * q);
  if (!(m > 0.0)) return 0;  // (q == 0 with no positive root of the resolvent, or a non-finite coefficient: no hypothesis)
  const double s = sqrt(2.0 * m), h = 0.5 * p + m, k = q / (2.0 * s);
  int n = 0;
  const double d1 = s * s - 4.0 * (h + k), d2 = s * s - 4.0 * (h - k);
  if (d1 >= 0.0) { const double w = sqrt(d1); roots[n++] = 0.5 * (s + w); roots[n++] = 0.5 * (s - w); }
  if (d2 >= 0.0) { const double w = sqrt(d2); roots[n++] = 0.5 * (-s + w); roots[n++] = 0.5 * (-s - w); }
  for (int i = 0; i < n; ++i) {
    double y = roots[i] - 0.25 * B;
    for (int it = 0; it < 2; ++it) {
      const double f = (((y + B) * y + C) * y + D) * y + E, d = ((4.0 * y + 3.0 * B) * y + 2.0 * C) * y + D;
      if (fabs(d) > 1e-300) y -= f / d;
    }
    roots[i] = y;
  }
  return n;
}

GSR_HD void cross3(const double a[3], const double b[3], double o[3]) {
  o[0] = a[1] * b[2] - a[2] * b[1]; o[1] = a[2] * b[0] - a[0] * b[2]; o[2] = a[0] * b[1] - a[1] * b[0];
}
GSR_HD double dot3(const double a[3], const double b[3]) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }

// The right-handed orthonormal frame of a triangle, as the columns e1 e2 e3 (F[3 * r + c]).
GSR_HD void triangle_frame(const double P0[3], const double P1[3], const double P2[3], double F[9]) {
  double a[3], b[3], e3[3], e2[3];
  for (int i = 0; i < 3; ++i) { a[i] = P1[i] - P0[i]; b[i] = P2[i] - P0[i]; }
  const double na = sqrt(dot3(a, a));
  for (int i = 0; i < 3; ++i) a[i] /= na;
  cross3(a, b, e3);
  const double n3 = sqrt(dot3(e3, e3));
  for (int i = 0; i < 3; ++i) e3[i] /= n3;
  cross3(e3, a, e2);
  for (int i = 0; i < 3; ++i) { F[3 * i] = a[i]; F[3 * i + 1] = e2[i]; F[3 * i + 2] = e3[i]; }
}

// P3P: world points X[0..2], unit bearings f[0..2] in the camera -> up to eight poses (R, t) with s_i f_i = R X_i + t.
// With the depths s1, s2 = x s1, s3 = y s1 and the law of cosines on the three sides, x is a rational function N(y) / D(y) and y a
// root of the quartic N^2 - 2 cos(gamma) N D - p D^2 (the polynomials are multiplied out here, not typed in).  Every real root gives
// two poses, s1 = +sqrt and s1 = -sqrt: a solution with negative depths is a solution of the equations as well, and the one the
// data came from when the points lie behind the camera - the caller's fourth point chooses, the score's depth test judges.
GSR_HD int p3p(const double X[3][3], const double f[3][3], Pose out[8]) {
  double d12[3], d02[3], d01[3];
  for (int i = 0; i < 3; ++i) { d12[i] = X[1][i] - X[2][i]; d02[i] = X[0][i] - X[2][i]; d01[i] = X[0][i] - X[1][i]; }
  const double a2 = dot3(d12, d12), b2 = dot3(d02, d02), c2 = dot3(d01, d01);
  const double ca = dot3(f[1], f[2]), cb = dot3(f[0], f[2]), cg = dot3(f[0], f[1]);
  const double kc = c2 / b2, ka = a2 / b2;
  const double p[3] = {kc - 1.0, -2.0 * cb * kc, kc};              // x^2 = 2 cg x + p(y)
  const double q[3] = {-ka, 2.0 * cb * ka, 1.0 - ka};              // x^2 - 2 ca y x + q(y) = 0
  const double N[3] = {-(p[0] + q[0]), -(p[1] + q[1]), -(p[2] + q[2])};
  const double Dn[2] = {2.0 * cg, -2.0 * ca};                      // x = N(y) / D(y)
  double quart[5] = {0, 0, 0, 0, 0};
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) quart[i + j] += N[i] * N[j];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 2; ++j) quart[i + j] -= 2.0 * cg * N[i] * Dn[j];
  const double DD[3] = {Dn[0] * Dn[0], 2.0 * Dn[0] * Dn[1], Dn[1] * Dn[1]};
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) quart[i + j] -= p[i] * DD[j];
  double ys[4];
  const int nr = quartic_real_roots(quart, ys);
  double FX[9];
  triangle_frame(X[0], X[1], X[2], FX);
  int n = 0;
  for (int k = 0; k < nr; ++k) {
    const double y = ys[k];
    const double x = ((N[2] * y + N[1]) * y + N[0]) / (Dn[1] * y + Dn[0]);
    const double w = 1.0 + y * y - 2.0 * y * cb;
    if (!(w > 0.0)) continue;
    for (int sign = 0; sign < 2; ++sign) {
      const double s1 = sign ? -sqrt(b2 / w) : sqrt(b2 / w), s2 = x * s1, s3 = y * s1;
      double P[3][3];
      for (int i = 0; i < 3; ++i) { P[0][i] = s1 * f[0][i]; P[1][i] = s2 * f[1][i]; P[2][i] = s3 * f[2][i]; }
      double FP[9];
      triangle_frame(P[0], P[1], P[2], FP);
      Pose& o = out[n];
      for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) o.R[3 * r + c] = FP[3 * r] * FX[3 * c] + FP[3 * r + 1] * FX[3 * c + 1] + FP[3 * r + 2] * FX[3 * c + 2];
      for (int r = 0; r < 3; ++r) o.t[r] = P[0][r] - (o.R[3 * r] * X[0][0] + o.R[3 * r + 1] * X[0][1] + o.R[3 * r + 2] * X[0][2]);
      ++n;
    }
  }
  return n;
}

struct Camera { double fx, fy, cx, cy; };

GSR_HD bool pose_finite(const Pose& P) {
  bool ok = true;
  for (int i = 0; i < 9; ++i) ok = ok && (fabs(P.R[i]) <= 1.7e308);
  for (int i = 0; i < 3; ++i) ok = ok && (fabs(P.t[i]) <= 1.7e308);
  return ok;  // (a NaN fails the comparison)
}

// Squared reprojection error of X under P, and its depth; the caller tests `z > 0 && e2 < thr^2`, which a NaN fails.
GSR_HD double reproj2(const Pose& P, const Camera& K, const double X[3], const double u[2], double* z) {
  const double Y0 = P.R[0] * X[0] + P.R[1] * X[1] + P.R[2] * X[2] + P.t[0];
  const double Y1 = P.R[3] * X[0] + P.R[4] * X[1] + P.R[5] * X[2] + P.t[1];
  const double Y2 = P.R[6] * X[0] + P.R[7] * X[1] + P.R[8] * X[2] + P.t[2];
  const double dx = K.fx * Y0 / Y2 + K.cx - u[0], dy = K.fy * Y1 / Y2 + K.cy - u[1];
  *z = Y2;
  return dx * dx + dy * dy;
}

// One hypothesis: P3P on the first three of four matches, the pose that reprojects the fourth best (the first of equals).
GSR_HD bool hypothesis(const double X[4][3], const double u[4][2], const Camera& K, Pose* best) {
  double f[3][3];
  for (int i = 0; i < 3; ++i) {
    const double bx = (u[i][0] - K.cx) / K.fx, by = (u[i][1] - K.cy) / K.fy;
    const double inv = 1.0 / sqrt(bx * bx + by * by + 1.0);
    f[i][0] = bx * inv; f[i][1] = by * inv; f[i][2] = inv;
  }
  Pose cand[8];
  const int n = p3p(X, f, cand);
  double best_e = 1.7e308;
  bool found = false;
  for (int k = 0; k < n; ++k) {
    if (!pose_finite(cand[k])) continue;
    double z;
    const double e = reproj2(cand[k], K, X[3], u[3], &z);
    if (e < best_e) { best_e = e; *best = cand[k]; found = true; }  // (a NaN fails the comparison)
  }
  return found;
}

// Gauss-Newton on sum |pi(K (R X + t)) - u|^2 with the update R <- exp(w) R, t <- t + d: one match's share of the upper triangle
// of J^T J (21 numbers, row by row) and of J^T r (6), parameters (w, d).
GSR_HD void gn_accumulate(const Pose& P, const Camera& K, const double X[3], const double u[2], double acc[27]) {
  const double Q0 = P.R[0] * X[0] + P.R[1] * X[1] + P.R[2] * X[2];
  const double Q1 = P.R[3] * X[0] + P.R[4] * X[1] + P.R[5] * X[2];
  const double Q2 = P.R[6] * X[0] + P.R[7] * X[1] + P.R[8] * X[2];
  const double Y0 = Q0 + P.t[0], Y1 = Q1 + P.t[1], Y2 = Q2 + P.t[2];
  const double iz = 1.0 / Y2;
  const double r0 = K.fx * Y0 * iz + K.cx - u[0], r1 = K.fy * Y1 * iz + K.cy - u[1];
  // d pi / d Y
  const double a0[3] = {K.fx * iz, 0.0, -K.fx * Y0 * iz * iz}, a1[3] = {0.0, K.fy * iz, -K.fy * Y1 * iz * iz};
  // d Y / d w_k = e_k x Q, so a row of J is (Q x a)
  double J0[6], J1[6];
  J0[0] = Q1 * a0[2] - Q2 * a0[1];  J0[1] = Q2 * a0[0] - Q0 * a0[2];  J0[2] = Q0 * a0[1] - Q1 * a0[0];
  J1[0] = Q1 * a1[2] - Q2 * a1[1];  J1[1] = Q2 * a1[0] - Q0 * a1[2];  J1[2] = Q0 * a1[1] - Q1 * a1[0];
  for (int k = 0; k < 3; ++k) { J0[3 + k] = a0[k]; J1[3 + k] = a1[k]; }
  int e = 0;
  for (int i = 0; i < 6; ++i)
    for (int j = i; j < 6; ++j) acc[e++] += J0[i] * J0[j] + J1[i] * J1[j];
  for (int i = 0; i < 6; ++i) acc[21 + i] += J0[i] * r0 + J1[i] * r1;
}

// Solve the normal equations (Cholesky, no pivoting) and apply the step.  A matrix that is not positive definite gives a non-finite
// pose, which the caller reports.
GSR_HD void gn_step(Pose* P, const double acc[27]) {
  double A[36], g[6];
  int e = 0;
  for (int i = 0; i < 6; ++i)
    for (int j = i; j < 6; ++j) { A[6 * i + j] = acc[e]; A[6 * j + i] = acc[e]; ++e; }
  for (int i = 0; i < 6; ++i) g[i] = -acc[21 + i];
  for (int j = 0; j < 6; ++j) {  // A = L L^T, L in the lower triangle
    double d = A[6 * j + j];
    for (int k = 0; k < j; ++k) d -= A[6 * j + k] * A[6 * j + k];
    d = sqrt(d);  // (NaN when d < 0)
    A[6 * j + j] = d;
    for (int i = j + 1; i < 6; ++i) {
      double s = A[6 * i + j];
      for (int k = 0; k < j; ++k) s -= A[6 * i + k] * A[6 * j + k];
      A[6 * i + j] = s / d;
    }
  }
  for (int i = 0; i < 6; ++i) {
    double s = g[i];
    for (int k = 0; k < i; ++k) s -= A[6 * i + k] * g[k];
    g[i] = s / A[6 * i + i];
  }
  for (int i = 5; i >= 0; --i) {
    double s = g[i];
    for (int k = i + 1; k < 6; ++k) s -= A[6 * k + i] * g[k];
    g[i] = s / A[6 * i + i];
  }
  const double wx = g[0], wy = g[1], wz = g[2];
  const double th2 = wx * wx + wy * wy + wz * wz, th = sqrt(th2);
  double ka, kb;  // exp(w) = I + ka [w]x + kb [w]x^2
  if (th < 1e-8) { ka = 1.0; kb = 0.5; }
  else { ka = sin(th) / th; kb = (1.0 - cos(th)) / th2; }
  const double Kx[9] = {0.0, -wz, wy, wz, 0.0, -wx, -wy, wx, 0.0};
  double E[9];
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) {
      double k2 = 0.0;
      for (int k = 0; k < 3; ++k) k2 += Kx[3 * r + k] * Kx[3 * k + c];
      E[3 * r + c] = (r == c ? 1.0 : 0.0) + ka * Kx[3 * r + c] + kb * k2;
    }
  double Rn[9];
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) Rn[3 * r + c] = E[3 * r] * P->R[c] + E[3 * r + 1] * P->R[3 + c] + E[3 * r + 2] * P->R[6 + c];
  for (int i = 0; i < 9; ++i) P->R[i] = Rn[i];
  for (int i = 0; i < 3; ++i) P->t[i] += g[3 + i];
}

// The rotation nearest a 3 x 3 matrix as the reference projects it: U diag(1, 1, det(U V^T)) V^T of its SVD, the SVD by
// kJacobiSweeps sweeps of one-sided Jacobi rotations; the factor det goes to the smallest singular value.
GSR_HD void project_so3(const double Ain[9], double Rout[9]) {
  double A[9], V[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
  for (int i = 0; i < 9; ++i) A[i] = Ain[i];
  for (int sweep = 0; sweep < kJacobiSweeps; ++sweep)
    for (int p = 0; p < 2; ++p)
      for (int q = p + 1; q < 3; ++q) {
        double al = 0.0, be = 0.0, ga = 0.0;
        for (int i = 0; i < 3; ++i) { al += A[3 * i + p] * A[3 * i + p]; be += A[3 * i + q] * A[3 * i + q]; ga += A[3 * i + p] * A[3 * i + q]; }
        if (ga == 0.0) continue;
        const double zeta = (be - al) / (2.0 * ga);
        const double t = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
        const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
        for (int i = 0; i < 3; ++i) {
          const double ap = A[3 * i + p], aq = A[3 * i + q];
          A[3 * i + p] = c * ap - s * aq; A[3 * i + q] = s * ap + c * aq;
          const double vp = V[3 * i + p], vq = V[3 * i + q];
          V[3 * i + p] = c * vp - s * vq; V[3 * i + q] = s * vp + c * vq;
        }
      }
  double sig[3], U[9];
  for (int j = 0; j < 3; ++j) {
    sig[j] = sqrt(A[j] * A[j] + A[3 + j] * A[3 + j] + A[6 + j] * A[6 + j]);
    for (int i = 0; i < 3; ++i) U[3 * i + j] = sig[j] > 0.0 ? A[3 * i + j] / sig[j] : 0.0;
  }
  double M[9];
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) M[3 * r + c] = U[3 * r] * V[3 * c] + U[3 * r + 1] * V[3 * c + 1] + U[3 * r + 2] * V[3 * c + 2];
  const double det = M[0] * (M[4] * M[8] - M[5] * M[7]) - M[1] * (M[3] * M[8] - M[5] * M[6]) + M[2] * (M[3] * M[7] - M[4] * M[6]);
  int lo = 0;
  if (sig[1] < sig[lo]) lo = 1;
  if (sig[2] < sig[lo]) lo = 2;
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) Rout[3 * r + c] = M[3 * r + c] + (det - 1.0) * U[3 * r + lo] * V[3 * c + lo];
}

}  // namespace pnp
}  // namespace gsr
