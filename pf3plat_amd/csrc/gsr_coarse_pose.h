#pragma once
#include "gsr_common.h"
#include "gsr_pnp_solver.h"

// ------------------------------------------------------------------------------------------------
// Coarse camera poses, device side (gsr_pnp_solver.h states the method and holds the solver): the PnP RANSAC kernels, k_camera_sync and
// the entry points gsr_pnp_ransac / gsr_camera_sync.  gsr_pose_refine.h refines these poses by the pose head's residual.
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
