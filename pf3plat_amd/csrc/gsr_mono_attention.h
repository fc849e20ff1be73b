#pragma once
#include "gsr_common.h"

// ------------------------------------------------------------------------------------------------
// Mono-guided attention over the cost volume (reference src/model/encoder/costvolume/depth_predictor_multiview.py:360-366;
// definition: include/gsr.h): out[b, c, i] = sum_j softmax_j(sum_e q[b, e, i] k[b, e, j]) v[b, c, j], all arrays channel-major;
// `v` is the 1 x 1 convolution of the cost volume's features.  Nothing of L x L floats exists: the scores are formed, used and dropped 32 x 32 at a time, in the registers of one wave.
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
