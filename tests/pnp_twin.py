"""The definition of gsr_pnp_ransac (include/gsr.h, items 1-4) restated for the host, one list at a time: a small C++ wrapper around
pf3plat_amd/csrc/gsr_pnp_solver.h - the solver's arithmetic is shared with the library on purpose, it is tested against numpy in
float64 by test_host_build_of_the_solver_in_float64 - built with the host compiler, and the Python side that fetches a list's points
(clamping the ids as the definition promises), decides the winner and assembles what a call must return.  What this checks is the
code in gsr_coarse_pose.h: draws, indices, staging, reductions, winner decoding, output layout.  Nothing here touches a device.

The device scores in fp32 and may contract a * b + c; the twin therefore scores every hypothesis twice, with the squared threshold
(and the depth test) shrunk and widened by a relative 1e-3, and calls a winner DECIDED only if no rounding inside that band could
change it."""
from __future__ import annotations

import ctypes
import os
import shutil
import subprocess
from dataclasses import dataclass

import numpy as np

from tests import pnp_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOLVER = os.path.join(ROOT, "pf3plat_amd", "csrc", "gsr_pnp_solver.h")
BAND = 1e-3            # relative, on the squared threshold
THREADS = 256          # the refinement's sums: lane tid takes matches tid, tid + 256, ..., then a binary tree over the lanes
STATUS_OK, STATUS_TOO_FEW_MATCHES, STATUS_NO_CONSENSUS, STATUS_NOT_FINITE = 0, 1, 2, 3

WRAPPER = r"""
#include "%s"
using namespace gsr::pnp;

static bool solve(int n, const float* X, const float* u, const double* K, uint32_t seed, int l, int t, Pose* P, int* drawn) {
  double XX[4][3], uu[4][2];
  for (int slot = 0; slot < 4; ++slot) {
    const int k = (int)(draw(seed, (uint32_t)l, (uint32_t)t, (uint32_t)slot) %% (uint32_t)n);
    if (drawn) drawn[slot] = k;
    for (int c = 0; c < 3; ++c) XX[slot][c] = X[3 * k + c];
    uu[slot][0] = u[2 * k]; uu[slot][1] = u[2 * k + 1];
  }
  Camera cam{K[0], K[1], K[2], K[3]};
  return hypothesis(XX, uu, cam, P);
}

// item 1: the four indices of hypothesis t
extern "C" void twin_draws(int n, uint32_t seed, int l, int t, int* out) {
  for (int slot = 0; slot < 4; ++slot) out[slot] = (int)(draw(seed, (uint32_t)l, (uint32_t)t, (uint32_t)slot) %% (uint32_t)n);
}

// items 1 + 2 for t = 0 .. hyp - 1: whether a pose was found, and its fp32 score under the shrunk and the widened test
extern "C" void twin_hypotheses(int n, const float* X, const float* u, const double* K, uint32_t seed, int l, int hyp, float thr,
                                double band, int* found, int* lo, int* hi) {
  const float fx = (float)K[0], fy = (float)K[1], cx = (float)K[2], cy = (float)K[3];
  const float thr2 = thr * thr, thr_lo = (float)(thr2 * (1.0 - band)), thr_hi = (float)(thr2 * (1.0 + band)), zband = (float)band;
  for (int t = 0; t < hyp; ++t) {
    Pose P;
    found[t] = solve(n, X, u, K, seed, l, t, &P, nullptr) ? 1 : 0;
    lo[t] = hi[t] = 0;
    if (!found[t]) continue;
    float R[9], T[3];
    for (int i = 0; i < 9; ++i) R[i] = (float)P.R[i];
    for (int i = 0; i < 3; ++i) T[i] = (float)P.t[i];
    for (int k = 0; k < n; ++k) {
      const float x = X[3 * k], y = X[3 * k + 1], z = X[3 * k + 2];
      const float Y0 = R[0] * x + R[1] * y + R[2] * z + T[0], Y1 = R[3] * x + R[4] * y + R[5] * z + T[1], Y2 = R[6] * x + R[7] * y + R[8] * z + T[2];
      const float dx = fx * Y0 / Y2 + cx - u[2 * k], dy = fy * Y1 / Y2 + cy - u[2 * k + 1];
      const float e2 = dx * dx + dy * dy;
      lo[t] += (Y2 > zband && e2 < thr_lo) ? 1 : 0;
      hi[t] += (Y2 > -zband && e2 < thr_hi) ? 1 : 0;
    }
  }
}

static double consensus(int n, const float* X, const float* u, const Camera& cam, const Pose& P, double thr, unsigned char* in,
                        double* margin) {
  const double thr2 = thr * thr;
  for (int k = 0; k < n; ++k) {
    const double Xd[3] = {X[3 * k], X[3 * k + 1], X[3 * k + 2]}, ud[2] = {u[2 * k], u[2 * k + 1]};
    double z;
    const double e2 = reproj2(P, cam, Xd, ud, &z);
    in[k] = (z > 0.0 && e2 < thr2) ? 1 : 0;
    const double d = fabs(sqrt(e2) - thr);
    if (d < *margin) *margin = d;  // (a NaN fails the comparison)
  }
  return *margin;
}

// items 3 + 4 for the winner t.  out: [0..15] the rigid inverse (row-major), [16] status, [17] inlier count, [18] the smallest
// distance (px) of a match's reprojection error under the FINAL pose from the threshold, [19] the same over the consensus tests of
// all rounds; acc: the 27 sums of the last Gauss-Newton step.
extern "C" void twin_refine(int n, const float* X, const float* u, const double* K, uint32_t seed, int l, int t, float thr_f,
                            unsigned char* mask, double* out, double* acc_out) {
  const double thr = (double)thr_f;
  Camera cam{K[0], K[1], K[2], K[3]};
  Pose P;
  for (int i = 0; i < 20; ++i) out[i] = 0.0;
  for (int i = 0; i < 27; ++i) acc_out[i] = 0.0;
  for (int k = 0; k < n; ++k) mask[k] = 0;
  for (int i = 0; i < 16; ++i) out[i] = (i %% 5 == 0) ? 1.0 : 0.0;
  out[18] = out[19] = 1.7e308;
  if (!solve(n, X, u, K, seed, l, t, &P, nullptr)) { out[16] = 2; return; }
  double rounds_margin = 1.7e308;
  for (int round = 0; round < kRefineRounds; ++round) {
    consensus(n, X, u, cam, P, thr, mask, &rounds_margin);
    for (int step = 0; step < kGnSteps; ++step) {
      static double part[%d][27];
      for (int lane = 0; lane < %d; ++lane) {
        for (int i = 0; i < 27; ++i) part[lane][i] = 0.0;
        for (int k = lane; k < n; k += %d) {
          if (!mask[k]) continue;
          const double Xd[3] = {X[3 * k], X[3 * k + 1], X[3 * k + 2]}, ud[2] = {u[2 * k], u[2 * k + 1]};
          gn_accumulate(P, cam, Xd, ud, part[lane]);
        }
      }
      for (int w = %d / 2; w > 0; w >>= 1)
        for (int lane = 0; lane < w; ++lane)
          for (int i = 0; i < 27; ++i) part[lane][i] += part[lane + w][i];
      for (int i = 0; i < 27; ++i) acc_out[i] = part[0][i];
      gn_step(&P, part[0]);
    }
  }
  if (!pose_finite(P)) {
    for (int k = 0; k < n; ++k) mask[k] = 0;
    out[16] = 3;
    return;
  }
  double final_margin = 1.7e308;
  consensus(n, X, u, cam, P, thr, mask, &final_margin);
  if (final_margin < rounds_margin) rounds_margin = final_margin;
  int count = 0;
  for (int k = 0; k < n; ++k) count += mask[k];
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) out[4 * r + c] = P.R[3 * c + r];
    out[4 * r + 3] = -(P.R[r] * P.t[0] + P.R[3 + r] * P.t[1] + P.R[6 + r] * P.t[2]);
  }
  out[12] = out[13] = out[14] = 0.0; out[15] = 1.0;
  out[16] = 0; out[17] = count; out[18] = final_margin; out[19] = rounds_margin;
}
""" % (SOLVER, THREADS, THREADS, THREADS, THREADS)


@dataclass
class Expected:
    """What a call must return for one list, and how firmly."""
    status: int
    inliers: int
    mask: np.ndarray       # (n,) bool
    pairwise: np.ndarray   # (4, 4) float64: the rigid inverse, or the identity
    winner: int            # the winning hypothesis, -1 where there is none
    score: int             # its fp32 score (shrunk = widened when decided)
    decided: bool          # no rounding inside the band changes the winner
    margin: float          # px: the nearest final reprojection error to the threshold
    rounds_margin: float   # px: the same over every consensus test of the refinement
    condition: float       # of the last step's normal matrix (2-norm, float64)


class Twin:
    def __init__(self, lib):
        self.lib = lib
        lib.twin_draws.restype = lib.twin_hypotheses.restype = lib.twin_refine.restype = None

    @staticmethod
    def fetch(sc, ls, xyz=None):
        """The list's 3-D points (n, 3) float32 at its ids_j CLAMPED into the image, its 2-D points (n, 2) float32 and the first
        view's (fx, fy, cx, cy) float64; `xyz`: in place of the scene's."""
        xyz = sc.xyz if xyz is None else xyz
        ids = np.clip(ls.ids_j, 0, ref.H * ref.W - 1)
        X = np.ascontiguousarray(xyz[ls.scene, ls.pair[1]].reshape(3, -1)[:, ids].T.astype(np.float32))
        u = np.ascontiguousarray(ls.points_2d.astype(np.float32))
        return X, u, np.array(sc.cam(ls), dtype=np.float64)

    def draws(self, n, seed, l, t):
        out = np.zeros(4, dtype=np.int32)
        self.lib.twin_draws(int(n), ctypes.c_uint32(seed & 0xffffffff), int(l), int(t), _ptr(out))
        return out

    def hypotheses(self, X, u, K, seed, l, hyp, thr=ref.THRESHOLD):
        """-> (found, shrunk score, widened score), each (hyp,) int32."""
        found, lo, hi = (np.zeros(hyp, dtype=np.int32) for _ in range(3))
        self.lib.twin_hypotheses(int(X.shape[0]), _ptr(X), _ptr(u), _ptr(K), ctypes.c_uint32(seed & 0xffffffff), int(l), int(hyp),
                                 ctypes.c_float(thr), ctypes.c_double(BAND), _ptr(found), _ptr(lo), _ptr(hi))
        return found, lo, hi

    @staticmethod
    def winner(found, lo, hi):
        """The winner by "highest score, then lowest t" -> (t, score, decided); t = -1: no hypothesis scores MIN_MATCHES (status 2),
        decided when none reaches it under the widened test either."""
        lo, hi = np.where(found > 0, lo, 0), np.where(found > 0, hi, 0)
        if lo.max(initial=0) < 4:
            return -1, int(lo.max(initial=0)), bool(hi.max(initial=0) < 4)
        w = int(np.argmax(lo))  # (the first of equals)
        decided = lo[w] == hi[w] and (hi[:w] < lo[w]).all() and (hi[w + 1:] <= lo[w]).all()
        return w, int(lo[w]), bool(decided)

    def refine(self, X, u, K, seed, l, t, thr=ref.THRESHOLD):
        n = X.shape[0]
        mask, out, acc = np.zeros(max(n, 1), dtype=np.uint8), np.zeros(20), np.zeros(27)
        self.lib.twin_refine(int(n), _ptr(X), _ptr(u), _ptr(K), ctypes.c_uint32(seed & 0xffffffff), int(l), int(t), ctypes.c_float(thr),
                             _ptr(mask), _ptr(out), _ptr(acc))
        A = np.zeros((6, 6))
        A[np.triu_indices(6)] = acc[:21]
        A = A + A.T - np.diag(np.diag(A))
        cond = float(np.linalg.cond(A)) if out[16] == 0 and np.isfinite(A).all() else np.inf
        return int(out[16]), int(out[17]), mask[:n].astype(bool), out[:16].reshape(4, 4).copy(), float(out[18]), float(out[19]), cond

    def expect(self, sc, l, seed, hyp, thr=ref.THRESHOLD, xyz=None):
        ls = sc.lists[l]
        n = ls.ids_i.size
        failure = lambda st, w, score, decided: Expected(st, 0, np.zeros(n, dtype=bool), np.eye(4), w, score, decided, np.inf, np.inf, np.inf)
        if n < 4:
            return failure(STATUS_TOO_FEW_MATCHES, -1, 0, True)
        X, u, K = self.fetch(sc, ls, xyz)
        w, score, decided = self.winner(*self.hypotheses(X, u, K, seed, l, hyp, thr))
        if w < 0:
            return failure(STATUS_NO_CONSENSUS, -1, score, decided)
        status, count, mask, pw, margin, rounds, cond = self.refine(X, u, K, seed, l, w, thr)
        if status != STATUS_OK:
            return failure(status, w, score, decided)
        return Expected(status, count, mask, pw, w, score, decided, margin, rounds, cond)


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


_BUILT = {}


def build_in(directory) -> Twin:
    """Compile the wrapper into `directory` (once per process) with the flags of the solver's own host test."""
    if "twin" not in _BUILT:
        cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
        assert cxx, "no C++ compiler (the build needs one as well)"
        src, lib_path = os.path.join(str(directory), "pnp_twin.cpp"), os.path.join(str(directory), "pnp_twin.so")
        with open(src, "w") as f:
            f.write(WRAPPER)
        subprocess.run([cxx, "-O1", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", src, "-o", lib_path], check=True)
        _BUILT["twin"] = Twin(ctypes.CDLL(lib_path))
    return _BUILT["twin"]


def built() -> Twin:
    assert "twin" in _BUILT, "pnp_twin.twin(tmp_path_factory) builds it first"
    return _BUILT["twin"]


def twin(tmp_path_factory) -> Twin:
    """The twin, built once per test session under pytest's temporary directory."""
    if "twin" not in _BUILT:
        build_in(tmp_path_factory.mktemp("pnp_twin"))
    return _BUILT["twin"]
