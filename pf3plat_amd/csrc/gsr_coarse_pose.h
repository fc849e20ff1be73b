#pragma once
#include "gsr_common.h"
#include "gsr_pnp_solver.h"
#include "gsr_pose_loss.h"  // pose_affine_inverse (k_pose_errors)

// ------------------------------------------------------------------------------------------------
// Coarse camera poses, device side (gsr_pnp_solver.h states the method and holds the solver): the PnP RANSAC kernels, k_camera_sync and
// the entry points gsr_pnp_ransac / gsr_camera_sync.  Below them, in a section of its own: the refinement of these poses by the pose
// head's residual and the pose errors (k_pose_ops: k_pose_refine_fwd / k_pose_refine_bwd / k_pose_errors; gsr_pose_refine* / gsr_pose_errors).
// ------------------------------------------------------------------------------------------------
namespace gsr {

struct PnpArgs {
  int B, V, H, W, L, hyp, nblk;
  const float* xyz; const float* intr; const int64_t* ids_i; const int64_t* ids_j; const float* wgt; const float* pts2d;
  const int32_t* offs;
  uint32_t seed; float thr; float conf_min;
  unsigned long long* best;
  float* pairwise; int32_t* inliers; int32_t* status; float* conf; uint8_t* mask;
};

constexpr int kPnpThreads = 256;
constexpr int kPnpStage = 1024;  // matches per LDS stage of the scoring kernel: 20 bytes each

// List l -> its pair (i, j) and scene.
__device__ inline void pnp_list_views(int l, int B, int V, int* s, int* pi, int* pj, int* pair) {
  const int p = l / B;
  *s = l - p * B; *pair = p;
  int i = 0, left = p;
  while (i < V - 2 && left >= V - 1 - i) { left -= V - 1 - i; ++i; }  // (at most V - 2 trips)
  *pi = i; *pj = i + 1 + left;
}

struct PnpList {
  const float* x; const int64_t* ids_i; const int64_t* ids_j; const float* pts2d;  // the second view's points; the list's entries
  int64_t hw; int W;
};

__device__ inline void pnp_fetch(const PnpList& ls, int k, float X[3], float u[2]) {
  int64_t idj = ls.ids_j[k];
  idj = idj < 0 ? 0 : (idj >= ls.hw ? ls.hw - 1 : idj);  // (an id outside the image is the caller's error; it is not followed out of the array)
  X[0] = ls.x[idj]; X[1] = ls.x[ls.hw + idj]; X[2] = ls.x[2 * ls.hw + idj];
  if (ls.pts2d) { u[0] = ls.pts2d[2 * (int64_t)k]; u[1] = ls.pts2d[2 * (int64_t)k + 1]; }
  else { const int64_t idi = ls.ids_i[k]; u[0] = (float)(idi % ls.W); u[1] = (float)(idi / ls.W); }
}

__device__ inline PnpList pnp_list(const PnpArgs& a, int l, int* s_out, int* far_out, pnp::Camera* K, int* begin, int* n) {
  int s, pi, pj, pair;
  pnp_list_views(l, a.B, a.V, &s, &pi, &pj, &pair);
  const int64_t hw = (int64_t)a.H * a.W;
  const int off = a.offs[l];
  PnpList ls;
  ls.x = a.xyz + ((int64_t)s * a.V + pj) * 3 * hw;
  ls.ids_i = a.ids_i + off; ls.ids_j = a.ids_j + off; ls.pts2d = a.pts2d ? a.pts2d + 2 * (int64_t)off : nullptr;
  ls.hw = hw; ls.W = a.W;
  const float* k = a.intr + ((int64_t)s * a.V + pi) * 9;
  K->fx = k[0]; K->fy = k[4]; K->cx = k[2]; K->cy = k[5];
  *s_out = s; *far_out = (pj - pi > 1); *begin = off; *n = a.offs[l + 1] - off;
  return ls;
}

__device__ inline bool pnp_solve_hypothesis(const PnpList& ls, const pnp::Camera& K, uint32_t seed, int l, int t, int n, pnp::Pose* P) {
  double X[4][3], u[4][2];
  for (int slot = 0; slot < 4; ++slot) {
    const int k = (int)(pnp::draw(seed, (uint32_t)l, (uint32_t)t, (uint32_t)slot) % (uint32_t)n);
    float Xf[3], uf[2];
    pnp_fetch(ls, k, Xf, uf);
    for (int c = 0; c < 3; ++c) X[slot][c] = Xf[c];
    u[slot][0] = uf[0]; u[slot][1] = uf[1];
  }
  return pnp::hypothesis(X, u, K, P);
}

// Launch 1: workgroup (list, block of 256 hypotheses).  A lane solves its hypothesis in fp64; the workgroup then walks the list in
// LDS stages, every lane counting the matches its own pose explains (fp32; all lanes read the same match: an LDS broadcast).
__global__ void __launch_bounds__(kPnpThreads) k_pnp_hypotheses(PnpArgs a) {
  __shared__ float stage[kPnpStage * 5];
  __shared__ unsigned long long red[kPnpThreads];
  const int tid = threadIdx.x, l = blockIdx.x / a.nblk, hb = blockIdx.x - l * a.nblk;
  int s, far, begin, n;
  pnp::Camera K;
  const PnpList ls = pnp_list(a, l, &s, &far, &K, &begin, &n);
  if (n < pnp::kMinMatches) {  // (uniform over the workgroup)
    if (tid == 0) a.best[blockIdx.x] = 0ull;
    return;
  }
  const int t = hb * kPnpThreads + tid;
  pnp::Pose P;
  bool ok = false;
  if (t < a.hyp) ok = pnp_solve_hypothesis(ls, K, a.seed, l, t, n, &P);
  float R[9], T[3];
  for (int i = 0; i < 9; ++i) R[i] = (float)P.R[i];
  for (int i = 0; i < 3; ++i) T[i] = (float)P.t[i];
  const float fx = (float)K.fx, fy = (float)K.fy, cx = (float)K.cx, cy = (float)K.cy, thr2 = a.thr * a.thr;
  unsigned count = 0;
  for (int base = 0; base < n; base += kPnpStage) {
    const int m = min(kPnpStage, n - base);
    __syncthreads();
    for (int k = tid; k < m; k += kPnpThreads) {
      float X[3], u[2];
      pnp_fetch(ls, base + k, X, u);
      stage[5 * k] = X[0]; stage[5 * k + 1] = X[1]; stage[5 * k + 2] = X[2]; stage[5 * k + 3] = u[0]; stage[5 * k + 4] = u[1];
    }
    __syncthreads();
    if (ok)
      for (int k = 0; k < m; ++k) {
        const float x = stage[5 * k], y = stage[5 * k + 1], z = stage[5 * k + 2];
        const float Y0 = R[0] * x + R[1] * y + R[2] * z + T[0], Y1 = R[3] * x + R[4] * y + R[5] * z + T[1], Y2 = R[6] * x + R[7] * y + R[8] * z + T[2];
        const float dx = fx * Y0 / Y2 + cx - stage[5 * k + 3], dy = fy * Y1 / Y2 + cy - stage[5 * k + 4];
        count += (Y2 > 0.f && dx * dx + dy * dy < thr2) ? 1u : 0u;
      }
  }
  red[tid] = ok ? (((unsigned long long)count << 32) | (unsigned)(a.hyp - 1 - t)) : 0ull;
  __syncthreads();
  for (int w = kPnpThreads / 2; w > 0; w >>= 1) {
    if (tid < w) red[tid] = max(red[tid], red[tid + w]);
    __syncthreads();
  }
  if (tid == 0) a.best[blockIdx.x] = red[0];
}

// Launch 2: one workgroup per list.  The winner is solved again from its index (the same arithmetic: the same pose), refined, and
// the list's row of every output written.
__global__ void __launch_bounds__(kPnpThreads) k_pnp_refine(PnpArgs a) {
  __shared__ double red[27 * kPnpThreads];
  __shared__ pnp::Pose pose, pose0;
  __shared__ int state;
  const int tid = threadIdx.x, l = blockIdx.x;
  int s, far, begin, n;
  pnp::Camera K;
  const PnpList ls = pnp_list(a, l, &s, &far, &K, &begin, &n);
  const double thr2 = (double)a.thr * (double)a.thr;

  // the confidence: the mean score in fp64, in a fixed order
  {
    double sum = 0.0;
    for (int k = tid; k < n; k += kPnpThreads) sum += (double)a.wgt[begin + k];
    red[tid] = sum;
    __syncthreads();
    for (int w = kPnpThreads / 2; w > 0; w >>= 1) {
      if (tid < w) red[tid] += red[tid + w];
      __syncthreads();
    }
    if (tid == 0) {
      float c = n > 0 ? (float)(red[0] / (double)n) : 0.f;
      if (far) c = fmaxf(c - a.conf_min, 0.f) / (1.f - a.conf_min);
      a.conf[l] = c;
    }
    __syncthreads();
  }

  if (tid == 0) {
    int st = 0;
    if (n < pnp::kMinMatches) st = 1;
    else {
      unsigned long long best = 0ull;
      for (int k = 0; k < a.nblk; ++k) best = max(best, a.best[(int64_t)l * a.nblk + k]);
      if ((unsigned)(best >> 32) < (unsigned)pnp::kMinMatches) st = 2;
      else {
        const int t = a.hyp - 1 - (int)(unsigned)(best & 0xffffffffull);
        pnp::Pose P;
        if (!pnp_solve_hypothesis(ls, K, a.seed, l, t, n, &P)) st = 2;
        pose = P;
      }
    }
    state = st;
  }
  __syncthreads();
  int st = state;

  if (st == 0) {
    for (int round = 0; round < pnp::kRefineRounds; ++round) {
      if (tid == 0) pose0 = pose;
      __syncthreads();
      for (int step = 0; step < pnp::kGnSteps; ++step) {
        double acc[27];
        for (int i = 0; i < 27; ++i) acc[i] = 0.0;
        for (int k = tid; k < n; k += kPnpThreads) {
          float Xf[3], uf[2];
          pnp_fetch(ls, k, Xf, uf);
          const double X[3] = {Xf[0], Xf[1], Xf[2]}, u[2] = {uf[0], uf[1]};
          double z;
          const double e2 = pnp::reproj2(pose0, K, X, u, &z);
          if (z > 0.0 && e2 < thr2) pnp::gn_accumulate(pose, K, X, u, acc);
        }
        __syncthreads();  // (everybody has read `pose`; `red` is free)
        for (int i = 0; i < 27; ++i) red[i * kPnpThreads + tid] = acc[i];
        __syncthreads();
        for (int w = kPnpThreads / 2; w > 0; w >>= 1) {
          if (tid < w)
            for (int i = 0; i < 27; ++i) red[i * kPnpThreads + tid] += red[i * kPnpThreads + tid + w];
          __syncthreads();
        }
        if (tid == 0) {
          double sum[27];
          for (int i = 0; i < 27; ++i) sum[i] = red[i * kPnpThreads];
          pnp::Pose P = pose;
          pnp::gn_step(&P, sum);
          pose = P;
        }
        __syncthreads();
      }
    }
    if (!pnp::pose_finite(pose)) st = 3;
  }

  // the consensus set under the final pose
  int count = 0;
  for (int k = tid; k < n; k += kPnpThreads) {
    bool in = false;
    if (st == 0) {
      float Xf[3], uf[2];
      pnp_fetch(ls, k, Xf, uf);
      const double X[3] = {Xf[0], Xf[1], Xf[2]}, u[2] = {uf[0], uf[1]};
      double z;
      const double e2 = pnp::reproj2(pose, K, X, u, &z);
      in = z > 0.0 && e2 < thr2;
    }
    if (a.mask) a.mask[begin + k] = in ? 1 : 0;
    count += in ? 1 : 0;
  }
  __syncthreads();
  int* ired = reinterpret_cast<int*>(red);
  ired[tid] = count;
  __syncthreads();
  for (int w = kPnpThreads / 2; w > 0; w >>= 1) {
    if (tid < w) ired[tid] += ired[tid + w];
    __syncthreads();
  }
  if (tid == 0) {
    a.inliers[l] = ired[0];
    a.status[l] = st;
    const int pairs = a.V * (a.V - 1) / 2, p = l / a.B;
    float* o = a.pairwise + ((int64_t)s * pairs + p) * 16;
    if (st != 0) {
      for (int i = 0; i < 16; ++i) o[i] = (i % 5 == 0) ? 1.f : 0.f;
    } else {  // the rigid inverse [R^T | -R^T t]
      for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) o[4 * r + c] = (float)pose.R[3 * c + r];
        o[4 * r + 3] = (float)(-(pose.R[r] * pose.t[0] + pose.R[3 + r] * pose.t[1] + pose.R[6 + r] * pose.t[2]));
      }
      o[12] = 0.f; o[13] = 0.f; o[14] = 0.f; o[15] = 1.f;
    }
  }
}

struct SyncArgs {
  int B, V;
  const float* pairwise; const float* conf; float* out;
};

// Launch 3: one workgroup per scene; the (4 v)^2 matrix and its square in LDS, fp64.  The matrix is formed in fp32 as the reference
// forms it (it converts to fp64 afterwards), in the reference's order of operations.
__global__ void __launch_bounds__(256) k_camera_sync(SyncArgs a) {
  constexpr int MV = pnp::kMaxViews, MN = 4 * MV;
  __shared__ double Lm[2][MN * MN];
  __shared__ int chain;
  const int tid = threadIdx.x, s = blockIdx.x, V = a.V, N = 4 * V, pairs = V * (V - 1) / 2;
  const float* Ps = a.pairwise + (int64_t)s * pairs * 16;
  float* out = a.out + (int64_t)s * V * 16;
  if (tid == 0) chain = (V == 2) ? 1 : 0;
  for (int e = tid; e < N * N; e += 256) Lm[0][e] = 0.0;
  __syncthreads();
  if (V > 2) {
    if (tid == 0) {
      float conf[MV][MV];
      for (int i = 0; i < V; ++i)
        for (int j = 0; j < V; ++j) conf[i][j] = 0.f;
      int p = 0;
      for (int i = 0; i < V; ++i)
        for (int j = i + 1; j < V; ++j, ++p) {
          const float c = a.conf[(int64_t)p * a.B + s];
          conf[i][j] = c; conf[j][i] = c;
          conf[i][i] = conf[i][i] + c / 2.f; conf[j][j] = conf[j][j] + c / 2.f;
        }
      for (int j = 0; j < V; ++j) {
        // The column sum in the order of the reference's `conf.sum(dim=1)` (torch's CPU kernel, which the records are of): row by
        // row for columns in groups of four; four interleaved partial sums over the rows 4 m + k - the rows left over added to the
        // first, then ((p0 + p1) + p2) + p3 - for the columns left over at V = 5, 6, 7 and for all columns at V = 8.  Up to V = 4
        // both are the sum in order.  (One fp32 ulp here moves the result by about 1e-6.)
        float part[4] = {0.f, 0.f, 0.f, 0.f};
        if (V == 8 || j >= 4) {
          for (int m = 0; m < V / 4; ++m)
            for (int k = 0; k < 4; ++k) part[k] += conf[4 * m + k][j];
          for (int i = 4 * (V / 4); i < V; ++i) part[0] += conf[i][j];
        } else {
          for (int i = 0; i < V; ++i) part[0] += conf[i][j];
        }
        float sum = ((part[0] + part[1]) + part[2]) + part[3];
        sum = fmaxf(sum, 1e-9f);
        for (int i = 0; i < V; ++i) conf[i][j] = conf[i][j] / sum;
      }
      for (int i = 0; i < V; ++i)
        for (int k = 0; k < 4; ++k) Lm[0][(4 * i + k) * N + 4 * i + k] = (double)conf[i][i];
      p = 0;
      for (int i = 0; i < V; ++i)
        for (int j = i + 1; j < V; ++j, ++p) {
          const float* P = Ps + p * 16;
          float inv[16];
          for (int r = 0; r < 3; ++r) {
            for (int c = 0; c < 3; ++c) inv[4 * r + c] = P[4 * c + r];
            float acc = (-1.f * P[r]) * P[3];           // ((-1 R^T) t)_r = sum_k (-R[k][r]) t_k
            acc += (-1.f * P[4 + r]) * P[7];
            acc += (-1.f * P[8 + r]) * P[11];
            inv[4 * r + 3] = acc;
          }
          for (int c = 0; c < 4; ++c) inv[12 + c] = P[12 + c];
          const float cij = conf[i][j], cji = conf[j][i];
          for (int r = 0; r < 4; ++r)
            for (int c = 0; c < 4; ++c) {
              Lm[0][(4 * i + r) * N + 4 * j + c] = (double)(cij * inv[4 * r + c]);
              Lm[0][(4 * j + r) * N + 4 * i + c] = (double)(cji * P[4 * r + c]);
            }
        }
    }
    __syncthreads();
    int cur = 0;
    for (int sq = 0; sq < pnp::kSquarings; ++sq) {
      for (int e = tid; e < N * N; e += 256) {
        const int r = e / N, c = e - r * N;
        double acc = 0.0;
        for (int k = 0; k < N; ++k) acc += Lm[cur][r * N + k] * Lm[cur][k * N + c];
        Lm[cur ^ 1][e] = acc;
      }
      __syncthreads();
      cur ^= 1;
    }
    // (kSquarings is even: the result is in Lm[0])
    if (tid == 0) {
      int zero = 0;
      for (int i = 0; i < V; ++i) zero |= (Lm[0][(4 * i + 3) * N + 3] == 0.0) ? 1 : 0;
      chain = zero;
    }
    __syncthreads();
    if (!chain && tid < V) {
      const int i = tid;
      const double mass = fmax(Lm[0][(4 * i + 3) * N + 3], 1e-9);
      double blk[16], Rp[9], R[9];
      for (int r = 0; r < 4; ++r)
        for (int c = 0; c < 4; ++c) blk[4 * r + c] = Lm[0][(4 * i + r) * N + c] / mass;
      for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) Rp[3 * r + c] = blk[4 * r + c];
      pnp::project_so3(Rp, R);
      for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) blk[4 * r + c] = R[3 * r + c];
      for (int e = 0; e < 16; ++e) out[16 * i + e] = (float)blk[e];
    }
  }
  if (chain && tid == 0) {  // camera_chaining: identity, then P(i, i + 1) times the one before, in fp32
    float cur[16];
    for (int e = 0; e < 16; ++e) { cur[e] = (e % 5 == 0) ? 1.f : 0.f; out[e] = cur[e]; }
    int p = 0;
    for (int i = 0; i + 1 < V; ++i) {
      const float* P = Ps + p * 16;
      float nxt[16];
      for (int r = 0; r < 4; ++r)
        for (int c = 0; c < 4; ++c) {
          float acc = P[4 * r] * cur[c];
          for (int k = 1; k < 4; ++k) acc += P[4 * r + k] * cur[4 * k + c];
          nxt[4 * r + c] = acc;
        }
      for (int e = 0; e < 16; ++e) { cur[e] = nxt[e]; out[16 * (i + 1) + e] = nxt[e]; }
      p += V - 1 - i;  // pair (i + 1, i + 2) follows the V - 1 - i pairs that begin with i
    }
  }
}

static bool pnp_offsets_ok(int L, const int32_t* offsets) {
  if (!offsets || offsets[0] < 0) return false;
  for (int l = 0; l < L; ++l)
    if (offsets[l + 1] < offsets[l]) return false;
  return true;
}

static bool pnp_sizes_ok(int B, int V, int pairs, int hyp) {
  if (B < 0 || V < 2 || V > pnp::kMaxViews || (int64_t)V * (V - 1) / 2 != pairs || hyp < 1 || hyp > (1 << 24)) return false;
  const int64_t nblk = (hyp + kPnpThreads - 1) / kPnpThreads;
  return (int64_t)B * pairs * nblk <= 0x7fffffff;
}

}  // namespace gsr

extern "C" {

int gsr_pnp_min_matches(void) { return gsr::pnp::kMinMatches; }

size_t gsr_pnp_ransac_scratch_bytes(int num_scenes, int num_views, int hypotheses) {
  const int pairs = num_views * (num_views - 1) / 2;
  if (num_views < 2 || !gsr::pnp_sizes_ok(num_scenes, num_views, pairs, hypotheses)) return 0;
  return (size_t)num_scenes * pairs * ((hypotheses + gsr::kPnpThreads - 1) / gsr::kPnpThreads) * sizeof(unsigned long long);
}

int gsr_pnp_ransac(int num_scenes, int num_views, int height, int width, int num_pairs, const float* xyz, const float* intrinsics_px,
                   const int64_t* ids_i, const int64_t* ids_j, const float* weights, const float* points_2d, const int32_t* offsets,
                   const int32_t* offsets_device, int hypotheses, float reprojection_error, float confidence_min, uint32_t seed,
                   void* scratch, float* pairwise, int32_t* inliers, int32_t* status, float* confidence, uint8_t* mask, void* stream_) {
  using namespace gsr;
  if (!pnp_sizes_ok(num_scenes, num_views, num_pairs, hypotheses)) return GSR_ERR_INVALID_ARGUMENT;
  if (height <= 0 || width <= 0 || (int64_t)height * width > 0x7fffffff) return GSR_ERR_INVALID_ARGUMENT;
  const int L = num_scenes * num_pairs;
  if (!pnp_offsets_ok(L, offsets)) return GSR_ERR_INVALID_ARGUMENT;
  if (!(reprojection_error > 0.f) || !(confidence_min < 1.f)) return GSR_ERR_INVALID_ARGUMENT;
  if (L == 0) return GSR_OK;
  if (!xyz || !intrinsics_px || !offsets_device || !scratch || !pairwise || !inliers || !status || !confidence) return GSR_ERR_INVALID_ARGUMENT;
  if (offsets[L] > offsets[0] && (!ids_i || !ids_j || !weights)) return GSR_ERR_INVALID_ARGUMENT;
  hipStream_t st = static_cast<hipStream_t>(stream_);
  PnpArgs a{};
  a.B = num_scenes; a.V = num_views; a.H = height; a.W = width; a.L = L; a.hyp = hypotheses;
  a.nblk = (hypotheses + kPnpThreads - 1) / kPnpThreads;
  a.xyz = xyz; a.intr = intrinsics_px; a.ids_i = ids_i; a.ids_j = ids_j; a.wgt = weights; a.pts2d = points_2d; a.offs = offsets_device;
  a.seed = seed; a.thr = reprojection_error; a.conf_min = confidence_min;
  a.best = static_cast<unsigned long long*>(scratch);
  a.pairwise = pairwise; a.inliers = inliers; a.status = status; a.conf = confidence; a.mask = mask;
  hipLaunchKernelGGL(k_pnp_hypotheses, dim3((unsigned)(L * a.nblk)), dim3(kPnpThreads), 0, st, a);
  GSR_CHECK(hipGetLastError());
  hipLaunchKernelGGL(k_pnp_refine, dim3((unsigned)L), dim3(kPnpThreads), 0, st, a);
  GSR_CHECK(hipGetLastError());
  return GSR_OK;
}

int gsr_camera_sync(int num_scenes, int num_views, const float* pairwise, const float* confidence, float* absolute, void* stream_) {
  using namespace gsr;
  if (num_scenes < 0 || num_views < 2 || num_views > pnp::kMaxViews) return GSR_ERR_INVALID_ARGUMENT;
  if (num_scenes == 0) return GSR_OK;
  if (!pairwise || !confidence || !absolute) return GSR_ERR_INVALID_ARGUMENT;
  SyncArgs a{num_scenes, num_views, pairwise, confidence, absolute};
  hipLaunchKernelGGL(k_camera_sync, dim3((unsigned)num_scenes), dim3(256), 0, static_cast<hipStream_t>(stream_), a);
  GSR_CHECK(hipGetLastError());
  return GSR_OK;
}

}  // extern "C"

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
enum { kPoseOpRefineFwd = 0, kPoseOpRefineBwd = 1, kPoseOpErrors = 2 };
struct PoseOpArgs {
  int op;
  RefineArgs r;
  PoseErrArgs e;
};

template <int kThreads>
__global__ __launch_bounds__(kRefineThreads) void k_pose_ops(const PoseOpArgs a) {
  __shared__ double part[kThreads];
  const int item = blockIdx.x * kThreads + threadIdx.x;
  if (a.op == kPoseOpRefineFwd) k_pose_refine_fwd(a.r, item);
  else if (a.op == kPoseOpRefineBwd) k_pose_refine_bwd<kThreads>(a.r, part);
  else k_pose_errors(a.e, item);
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
