#pragma once
#include "gsr_common.h"
#include "gsr_mono_attention.h"  // the MFMA tile helpers it shares: ma_f16, ma_row, ma_mfma, ma_zero, kMaOwn, kMaTile

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

// ------------------------------------------------------------------------------------------------
// Ragged multi-head attention (the attention of LightGlue's matcher transformer, reference lightglue.py:133-256 as
// src/model/encoder/encoder_costvolume.py:79, 334-337 builds and calls it; definition: include/gsr.h): k_mha_fwd's tile scheme - four
// waves, a wave owns 32 queries, key tiles of 32 through two LDS buffers, the score tile in registers as the next product's B operand -
// with what the matcher needs and the pose transformer has not:
//   UNITS: a workgroup is (unit, block of 128 queries, head); a unit is a query row range and a key row range of ONE packed row space
//     of T rows, read from the device copies of the four arrays (clamped to [0, T]: a wrong device copy reads nothing outside the
//     operands).  The grid is sized on the host from the host copies; a workgroup finds its unit by a wave scan over the units' block
//     counts, 64 units a step (rg_find): no table, no launch in front, no host read.
//   HEADS OF 64: channels 32 .. 63 are a second half - the score tile sums over up to 32 channel pairs, the owned q is 32 registers,
//     there are two 32 x 32 output accumulators; the half is skipped where D <= 32 (launch-uniform).
//   ROTARY AT LOAD: with `rot` the rows of q and k are rotated while they are staged: the fetch takes x, cos and sin into registers
//     (one tile ahead, as the keys themselves), the partner channel comes from the neighbouring lane (the lane index of a load runs
//     along the channels) when the registers go to LDS; x cos + (-+ partner) sin in the reference's order of operations.
// LDS: the owned image [64][129], K tiles 2 x [64][33], V tiles 2 x [32][72]: 68 352 bytes, two workgroups on a CU.  ds_read_b32 and
// ds_write_b32 bank by address mod 32 within a half wave: the K and owned images are filled by channel (line strides 33 and 129: odd)
// and read by token, the V image is filled and read by channel; a half wave never meets a bank twice.
// A unit without keys writes out = 0, lse = -inf.  No atomics, every trip count fixed by the arrays: the same bits on every call.
// ------------------------------------------------------------------------------------------------
namespace gsr {
constexpr int kRgChan = 64;                       // the most channels per head
constexpr int kRgOwnS = kMaOwn + 1;               // line stride of the owned [c][query] image
constexpr int kRgOwnFloats = kRgChan * kRgOwnS;   // ... which after the loop holds four [token][33] output tiles
constexpr int kRgKFloats = kRgChan * 33;          // a key tile's [c][33] image
constexpr int kRgVS = 72;                         // line stride of the [key][channel] value image
constexpr int kRgVFloats = 32 * kRgVS;
constexpr int kRgLdsFloats = kRgOwnFloats + 2 * kRgKFloats + 2 * kRgVFloats;
static_assert(kRgOwnFloats >= 4 * 32 * 33, "the output tiles live in the owned image");

struct RaggedArgs {
  int U, T, H, D;
  float scale;
  const int32_t *qb, *qc, *kb, *kc;  // the device copies: a unit's first query row, its queries, its first key row, its keys
  const float *q, *k, *v, *rot;      // rot: (2, T, D) cosines then sines, or NULL
  int64_t qs[3], ks[3], vs[3];       // element strides: token, head, channel
  float *out, *lse;                  // (T, H, D), (H, T)
};

__device__ __forceinline__ int rg_clamp(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// The unit that holds query block `g` of the call (blocks of 128 queries, unit after unit) and the block's index inside it; false
// past the last block.  Every lane of the wave calls it and gets the same answer.
__device__ __forceinline__ bool rg_find(const RaggedArgs& a, int g, int lane, int* unit, int* blk) {
  int base = 0;
  for (int u0 = 0; u0 < a.U; u0 += 64) {
    const int u = u0 + lane;
    const int nb = u < a.U ? (rg_clamp(a.qc[u], a.T) + kMaOwn - 1) / kMaOwn : 0;
    const int inc = (int)wave_inclusive_scan_u32((uint32_t)nb);
    const unsigned long long hit = __ballot(base + inc > g);
    if (hit) {
      const int first = __ffsll((long long)hit) - 1;
      *unit = u0 + first;
      *blk = g - base - __shfl(inc - nb, first);
      return true;
    }
    base += __shfl(inc, 63);
  }
  return false;
}

// Rows [tok0, tok0 + 32) of a range of ntok rows x channels [c0, c0 + 32) of a strided operand into 4 registers of each of 256
// threads, mh_fetch's element order; `base` is the range's first row at the head; zero outside [0, ntok) x [0, D).
__device__ __forceinline__ void rg_fetch(const float* base, int64_t st, int64_t sc, int D, int ntok, int tok0, int c0, int tid, float* regs) {
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int idx = tid + 256 * u, tok = tok0 + (idx >> 5), c = c0 + (idx & 31);
    regs[u] = (c < D && tok < ntok) ? base[(int64_t)tok * st + (int64_t)c * sc] : 0.f;
  }
}

// apply_cached_rotary_emb on a staged element: (x cos) + (rotate_half(x) sin), rotate_half(x)[2 p] = -x[2 p + 1], [2 p + 1] = x[2 p];
// the partner channel is the neighbouring lane's.  Every lane of the wave calls it.
__device__ __forceinline__ float rg_rotate(float x, float cs, float sn, int tid) {
  const float xp = __shfl_xor(x, 1);
  return x * cs + ((tid & 1) ? xp : -xp) * sn;
}

template <bool kRot>
__device__ __forceinline__ void k_ragged_fwd(const RaggedArgs& a, float* lds) {
  constexpr int VS = kRgVS;
  float* Qs = lds;
  float(*Ks)[kRgKFloats] = reinterpret_cast<float(*)[kRgKFloats]>(lds + kRgOwnFloats);
  float(*Vs)[kRgVFloats] = reinterpret_cast<float(*)[kRgVFloats]>(lds + kRgOwnFloats + 2 * kRgKFloats);
  const int tid = threadIdx.x, lane = tid & 63, x = lane & 31, h = lane >> 5, wv = tid >> 6;
  const int H = a.H, D = a.D, T = a.T;
  const int g = (int)blockIdx.x / H, hd = (int)blockIdx.x - g * H;
  int unit, blk;
  if (!rg_find(a, g, lane, &unit, &blk)) return;  // (workgroup-uniform)
  const int q0 = rg_clamp(a.qb[unit], T), nq = rg_clamp(a.qc[unit], T - q0);
  const int k0 = rg_clamp(a.kb[unit], T), nk = rg_clamp(a.kc[unit], T - k0);
  const int i0 = blk * kMaOwn, DP = (D + 1) / 2, NT = (nk + kMaTile - 1) / kMaTile;
  const bool two = D > 32;  // (launch-uniform)
  const float* qh = a.q + (int64_t)q0 * a.qs[0] + (int64_t)hd * a.qs[1];
  const float* kh = a.k + (int64_t)k0 * a.ks[0] + (int64_t)hd * a.ks[1];
  const float* vh = a.v + (int64_t)k0 * a.vs[0] + (int64_t)hd * a.vs[1];
  const float *qcos = nullptr, *qsin = nullptr, *kcos = nullptr, *ksin = nullptr;
  if (kRot) {
    qcos = a.rot + (int64_t)q0 * D; qsin = qcos + (int64_t)T * D;
    kcos = a.rot + (int64_t)k0 * D; ksin = kcos + (int64_t)T * D;
  }
  float kp[8], vp[8], cp[8], sp[8];  // a tile one ahead: k, v and (kRot) k's cosines and sines; registers 4 half + u
  auto fetch = [&](int tok0) {
#pragma unroll
    for (int half = 0; half < 2; ++half)
      if (half == 0 || two) {
        rg_fetch(kh, a.ks[0], a.ks[2], D, nk, tok0, 32 * half, tid, kp + 4 * half);
        rg_fetch(vh, a.vs[0], a.vs[2], D, nk, tok0, 32 * half, tid, vp + 4 * half);
        if (kRot) {
          rg_fetch(kcos, D, 1, D, nk, tok0, 32 * half, tid, cp + 4 * half);
          rg_fetch(ksin, D, 1, D, nk, tok0, 32 * half, tid, sp + 4 * half);
        }
      }
  };
  auto put = [&](int buf) {
#pragma unroll
    for (int half = 0; half < 2; ++half)
      if (half == 0 || two) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int idx = tid + 256 * u, tok = idx >> 5, c = 32 * half + (idx & 31);
          const float kv = kRot ? rg_rotate(kp[4 * half + u], cp[4 * half + u], sp[4 * half + u], tid) : kp[4 * half + u];
          Ks[buf][c * 33 + tok] = kv;
          Vs[buf][tok * VS + c] = vp[4 * half + u];
        }
      }
  };
  // the owned queries, rotated, as [c][kRgOwnS]
#pragma unroll
  for (int half = 0; half < 2; ++half)
    if (half == 0 || two) {
#pragma unroll 4
      for (int idx = tid; idx < 32 * kMaOwn; idx += 256) {
        const int t = idx >> 5, c = 32 * half + (idx & 31), tok = i0 + t;
        const bool ok = c < D && tok < nq;
        float xv = ok ? qh[(int64_t)tok * a.qs[0] + (int64_t)c * a.qs[2]] : 0.f;
        if (kRot) {
          const float cs = ok ? qcos[(int64_t)tok * D + c] : 0.f, sn = ok ? qsin[(int64_t)tok * D + c] : 0.f;
          xv = rg_rotate(xv, cs, sn, tid);
        }
        Qs[c * kRgOwnS + t] = xv;
      }
    }
  fetch(0);
  put(0);
  __syncthreads();
  float qreg[32];  // q'[c = 2 p + h][i]
#pragma unroll
  for (int p = 0; p < 32; ++p) qreg[p] = p < DP ? Qs[(2 * p + h) * kRgOwnS + wv * 32 + x] : 0.f;
  ma_f16 acc0 = ma_zero(), acc1 = ma_zero();
  float m = -INFINITY, l = 0.f;
  for (int tile = 0; tile < NT; ++tile) {
    const int cur = tile & 1, nxt = cur ^ 1, j0 = tile * kMaTile;
    const bool more = tile + 1 < NT;
    if (more) fetch(j0 + kMaTile);
    ma_f16 s = ma_zero();  // S^T[j][i]
#pragma unroll
    for (int p = 0; p < 32; ++p)
      if (p < DP) s = ma_mfma(Ks[cur][(2 * p + h) * 33 + x], qreg[p], s);
    float mx = -INFINITY;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      s[r] = j0 + ma_row(r, h) < nk ? s[r] * a.scale : -INFINITY;
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
    acc0 *= alpha;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc0 = ma_mfma(Vs[cur][ma_row(r, h) * VS + x], s[r], acc0);
    if (two) {
      acc1 *= alpha;
#pragma unroll
      for (int r = 0; r < 16; ++r) acc1 = ma_mfma(Vs[cur][ma_row(r, h) * VS + 32 + x], s[r], acc1);
    }
    if (more) put(nxt);
    __syncthreads();
  }
  if (nk > 0) {  // (no keys: the accumulators are the zeros they began as)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      acc0[r] = acc0[r] / l;
      acc1[r] = acc1[r] / l;
    }
  }
  // a wave's accumulators (register r = channel ma_row(r, h) of the half, of the lane's query) through its [token][33] tile of the
  // owned image, then up to 32 contiguous floats per token and half
  float* os = Qs + wv * 32 * 33;
  float* dst = a.out + ((int64_t)q0 * H + hd) * D;
  const int64_t hdD = (int64_t)H * D;
#pragma unroll
  for (int half = 0; half < 2; ++half)
    if (half == 0 || two) {
      __syncthreads();  // (the owned image, or the half stored before this one, has been read)
#pragma unroll
      for (int r = 0; r < 16; ++r) os[x * 33 + ma_row(r, h)] = half == 0 ? acc0[r] : acc1[r];
      __syncthreads();
#pragma unroll
      for (int u = 0; u < 16; ++u) {
        const int idx = lane + 64 * u, t = idx >> 5, c = 32 * half + (idx & 31), tok = i0 + wv * 32 + t;
        if (c < D && tok < nq) dst[(int64_t)tok * hdD + c] = os[t * 33 + (idx & 31)];
      }
    }
  const int i = i0 + wv * 32 + x;
  if (i < nq && h == 0) a.lse[(int64_t)hd * T + q0 + i] = nk > 0 ? m + logf(l) : -INFINITY;
}

// A kernel of its own, and a template instance so that it follows every plain kernel and none of them moves (the comment above
// k_mha_ops): 68 KB of LDS and two accumulators are not what k_mha_ops' three waves per SIMD, or k_pose_ops' one-workgroup routines,
// should be sized by.  Two workgroups on a CU: the LDS allows no more.
template <int kThreads>
__global__ __launch_bounds__(kThreads, 2) void k_ragged_ops(const RaggedArgs a) {
  __shared__ float lds[kRgLdsFloats];
  if (a.rot) k_ragged_fwd<true>(a, lds);
  else k_ragged_fwd<false>(a, lds);
}

// The limits of a call, from the host copies; on success the number of query blocks of 128 over all units.
static bool rg_sizes_ok(int U, int T, int H, int D, float scale, bool with_rot, const int32_t* qb, const int32_t* qc, const int32_t* kb,
                        const int32_t* kc, int64_t* blocks) {
  if (U < 1 || T < 1 || H < 1 || D < 1 || D > kRgChan || !std::isfinite(scale) || (with_rot && (D & 1))) return false;
  if (!qb || !qc || !kb || !kc) return false;
  const int64_t lim = 0x7fffffff;
  if ((int64_t)T * H > lim / D) return false;  // (T H D <= 2^31 - 1)
  int64_t nb = 0;
  for (int u = 0; u < U; ++u) {
    if (qb[u] < 0 || qc[u] < 0 || kb[u] < 0 || kc[u] < 0) return false;
    if ((int64_t)qb[u] + qc[u] > T || (int64_t)kb[u] + kc[u] > T) return false;
    nb += (qc[u] + kMaOwn - 1) / kMaOwn;
  }
  if (nb * H > lim) return false;  // (the grid; only overlapping query ranges can reach it)
  *blocks = nb;
  return true;
}
}  // namespace gsr

extern "C" {

size_t gsr_ragged_attention_scratch_bytes(int U, int T, int H, int D, const int32_t* q_begin_host, const int32_t* q_count_host,
                                          const int32_t* k_begin_host, const int32_t* k_count_host) {
  int64_t blocks;
  if (!gsr::rg_sizes_ok(U, T, H, D, 1.f, false, q_begin_host, q_count_host, k_begin_host, k_count_host, &blocks)) return 0;
  return 16;  // (a workgroup SEARCHES its unit: no table; never 0 for an accepted call)
}

int gsr_ragged_attention(int U, int T, int H, int D, float scale, const int32_t* q_begin_host, const int32_t* q_begin_device,
                         const int32_t* q_count_host, const int32_t* q_count_device, const int32_t* k_begin_host,
                         const int32_t* k_begin_device, const int32_t* k_count_host, const int32_t* k_count_device, const float* q,
                         const int64_t* q_strides, const float* k, const int64_t* k_strides, const float* v, const int64_t* v_strides,
                         const float* rot, float* out, float* lse, void* scratch, void* stream_) {
  using namespace gsr;
  int64_t blocks;
  if (!rg_sizes_ok(U, T, H, D, scale, rot != nullptr, q_begin_host, q_count_host, k_begin_host, k_count_host, &blocks))
    return GSR_ERR_INVALID_ARGUMENT;
  if (!q_begin_device || !q_count_device || !k_begin_device || !k_count_device || !q || !q_strides || !k || !k_strides || !v ||
      !v_strides || !out || !lse || !scratch)
    return GSR_ERR_INVALID_ARGUMENT;
  if (blocks == 0) return GSR_OK;  // (no unit has a query: nothing to write)
  RaggedArgs a{};
  a.U = U; a.T = T; a.H = H; a.D = D; a.scale = scale;
  a.qb = q_begin_device; a.qc = q_count_device; a.kb = k_begin_device; a.kc = k_count_device;
  a.q = q; a.k = k; a.v = v; a.rot = rot; a.out = out; a.lse = lse;
  for (int s = 0; s < 3; ++s) { a.qs[s] = q_strides[s]; a.ks[s] = k_strides[s]; a.vs[s] = v_strides[s]; }
  hipLaunchKernelGGL(k_ragged_ops<256>, dim3((unsigned)(blocks * H)), dim3(256), 0, static_cast<hipStream_t>(stream_), a);
  GSR_CHECK(hipGetLastError());
  return GSR_OK;
}

}  // extern "C"

// ------------------------------------------------------------------------------------------------
// Match assignment (LightGlue's MatchAssignment.forward, sigmoid_log_double_softmax and filter_matches, reference lightglue.py:259-312
// and the list building of :586-597; definition: include/gsr.h): L ragged lists in one chain of three launches - the passes of
// k_match_ops, below -, nothing of m x n elements anywhere.  The two streaming passes share one device function, k_match_stream:
//   A workgroup is four waves and OWNS 128 keypoints of one image of one list (a wave 32, the lane column, as above); the owned
//   descriptors - up to 256 channels - live in REGISTERS (128 per lane: channel 2 p + h of the lane's keypoint, read from global
//   memory once), because at d = 256 their LDS image would be 128 KB.  The other image's descriptors are streamed in tiles of 32
//   keypoints x all channels through two LDS buffers ([c][33], 33 KB each at d = 256), fetched one tile ahead into registers; the
//   lane index of a load runs along the channels.  The score tile is mh_scores' product over all channel pairs in channel order, times
//   `scale` once.  Rows of the grid (blockIdx.y) are (list, side): side 0 owns the first image's keypoints and streams the second's,
//   side 1 is the MIRRORED pass.  a b = b a, so s[i][j] has the same bits on both sides and in both passes.
//   pass kMtStats:  log sum_streamed exp s by the online log-sum-exp, kept as (maximum, log of the sum): lr on side 0, lc on side 1.
//   pass kMtArgmax: best[own] = the lowest streamed index that maximises 2 s + (ls(z) - lse)[streamed], and s there.  A lane keeps
//                   the first maximum of its registers, which ascend in the streamed index; the two lane halves meet once, at the end.
//   pass kMtFilter: one workgroup per list: the mutual checks, max0 in the reference's order of float32 operations
//                   (((s - max_r) - log sum_r) + ((s - max_c) - log sum_c)) + (ls(z0) + ls(z1)), expf, the threshold, the dense outputs and - rows in ascending chunks
//                   of 256, ranked by wave ballots and four wave totals in LDS - the compact entries and count[l].
// No atomics, no sum across workgroups, every loop's trip count fixed by the offsets: the same bits on every run.
// ------------------------------------------------------------------------------------------------
namespace gsr {
constexpr int kMtChan = 256;                  // the most channels
constexpr int kMtTileFloats = kMtChan * 33;   // a streamed tile's [c][33] image
constexpr int kMtLdsFloats = 2 * kMtTileFloats + 2 * 32;
enum { kMtStats = 0, kMtArgmax = 1, kMtFilter = 2 };

struct MatchArgs {
  int op, L, d, width, grid_rows;  // width 0: no keypoints; grid_rows: the grid's y extent of a streaming pass
  float scale, threshold;
  const float *desc[2], *z[2], *kpts[2];  // side 0: the first image, side 1: the second
  const int32_t* off[2];                  // the device copies of the offsets
  float *lmax[2], *lsum[2], *sbest[2];    // scratch, by packed keypoint: lr / lc as (running maximum, log of the sum), and s at the arg-maximum
  int32_t* best[2];                       // m0 / m1, local to the list
  int32_t* matches[2];
  float* mscores[2];
  int32_t *idx0, *idx1, *count;
  float *score, *points;
  int64_t *ids_i, *ids_j;
};

__device__ __forceinline__ float mt_logsigmoid(float z) { return fminf(z, 0.f) - log1pf(expf(-fabsf(z))); }

// Keypoints [tok0, tok0 + 32) x every channel of the streamed (ns, d) descriptors into 4 registers per chunk of 32 channels: element
// idx = tid + 256 u of chunk cb is keypoint idx >> 5, channel 32 cb + (idx & 31); zero outside [0, ns) x [0, d).
__device__ __forceinline__ void mt_fetch(const float* sd, int d, int NC, int ns, int tok0, int tid, float* regs) {
#pragma unroll
  for (int cb = 0; cb < kMtChan / 32; ++cb)
    if (cb < NC) {
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int idx = tid + 256 * u, tok = tok0 + (idx >> 5), c = 32 * cb + (idx & 31);
        regs[4 * cb + u] = (c < d && tok < ns) ? sd[(int64_t)tok * d + c] : 0.f;
      }
    }
}

// ... to LDS as [channel][33].
__device__ __forceinline__ void mt_put(float* dst, int NC, int tid, const float* regs) {
#pragma unroll
  for (int cb = 0; cb < kMtChan / 32; ++cb)
    if (cb < NC) {
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int idx = tid + 256 * u;
        dst[(32 * cb + (idx & 31)) * 33 + (idx >> 5)] = regs[4 * cb + u];
      }
    }
}

template <bool kArg>
__device__ __forceinline__ void k_match_stream(const MatchArgs& a, float* lds) {
  float(*Ts)[kMtTileFloats] = reinterpret_cast<float(*)[kMtTileFloats]>(lds);
  float(*Ws)[32] = reinterpret_cast<float(*)[32]>(lds + 2 * kMtTileFloats);
  const int tid = threadIdx.x, lane = tid & 63, x = lane & 31, h = lane >> 5, wv = tid >> 6;
  const int d = a.d, DP = (d + 1) / 2, NC = (d + 31) / 32;
  const int own0 = (int)blockIdx.x * kMaOwn;
  for (int64_t row = blockIdx.y; row < 2 * (int64_t)a.L; row += a.grid_rows) {  // (list, side); every test below is workgroup-uniform
    const int l = (int)(row >> 1), side = (int)(row & 1);
    const int o0 = a.off[side][l], no = a.off[side][l + 1] - o0;
    const int t0 = a.off[side ^ 1][l], ns = a.off[side ^ 1][l + 1] - t0;
    if (no <= 0 || ns <= 0 || own0 >= no) continue;
    const float* od = a.desc[side] + (int64_t)o0 * d;
    const float* sd = a.desc[side ^ 1] + (int64_t)t0 * d;
    const float* zs = a.z[side ^ 1] + t0;
    const float *lm = a.lmax[side ^ 1] + t0, *ls = a.lsum[side ^ 1] + t0;
    const int own = own0 + wv * 32 + x, T = (ns + kMaTile - 1) / kMaTile;
    float oreg[kMtChan / 2];  // channel 2 p + h of the lane's keypoint
#pragma unroll
    for (int p = 0; p < kMtChan / 2; ++p) {
      const int c = 2 * p + h;
      oreg[p] = (p < DP && c < d && own < no) ? od[(int64_t)own * d + c] : 0.f;
    }
    float tp[kMtChan / 8], wp = 0.f;
    mt_fetch(sd, d, NC, ns, 0, tid, tp);
    if (kArg && tid < 32) wp = tid < ns ? mt_logsigmoid(zs[tid]) - (lm[tid] + ls[tid]) : 0.f;
    mt_put(Ts[0], NC, tid, tp);
    if (kArg && tid < 32) Ws[0][tid] = wp;
    __syncthreads();
    float mrun = -INFINITY, lrun = 0.f;    // kMtStats
    float bv = -INFINITY, bs = 0.f;        // kMtArgmax
    int bi = 0;
    for (int tile = 0; tile < T; ++tile) {
      const int cur = tile & 1, nxt = cur ^ 1, j0 = tile * kMaTile;
      const bool more = tile + 1 < T;
      if (more) {
        mt_fetch(sd, d, NC, ns, j0 + kMaTile, tid, tp);
        if (kArg && tid < 32) wp = j0 + kMaTile + tid < ns ? mt_logsigmoid(zs[j0 + kMaTile + tid]) - (lm[j0 + kMaTile + tid] + ls[j0 + kMaTile + tid]) : 0.f;
      }
      ma_f16 s = ma_zero();  // S^T[streamed][own]
#pragma unroll
      for (int p = 0; p < kMtChan / 2; ++p)
        if (p < DP) s = ma_mfma(Ts[cur][(2 * p + h) * 33 + x], oreg[p], s);
      if (!kArg) {
        float mx = -INFINITY;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          s[r] = j0 + ma_row(r, h) < ns ? s[r] * a.scale : -INFINITY;
          mx = fmaxf(mx, s[r]);
        }
        mx = fmaxf(mx, __shfl_xor(mx, 32));
        const float m_new = fmaxf(mrun, mx);  // (every tile holds a keypoint: m_new is finite; exp(-inf) = 0)
        float sum = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) sum += expf(s[r] - m_new);
        sum += __shfl_xor(sum, 32);
        lrun = lrun * expf(mrun - m_new) + sum;
        mrun = m_new;
      } else {
#pragma unroll
        for (int r = 0; r < 16; ++r) {  // (ascending streamed index: the first maximum is the lowest)
          const int rr = ma_row(r, h);
          const float sv = s[r] * a.scale, v = fmaf(2.f, sv, Ws[cur][rr]);
          if (j0 + rr < ns && v > bv) {
            bv = v;
            bs = sv;
            bi = j0 + rr;
          }
        }
      }
      if (more) {
        mt_put(Ts[nxt], NC, tid, tp);
        if (kArg && tid < 32) Ws[nxt][tid] = wp;
      }
      __syncthreads();
    }
    if (!kArg) {
      if (own < no && h == 0) {  // (kept apart: s - maximum is exact where the row is peaked, as in torch's log_softmax)
        a.lmax[side][o0 + own] = mrun;
        a.lsum[side][o0 + own] = logf(lrun);
      }
    } else {
      const float ov = __shfl_xor(bv, 32), os = __shfl_xor(bs, 32);
      const int oi = __shfl_xor(bi, 32);
      if (ov > bv || (ov == bv && oi < bi)) {
        bs = os;
        bi = oi;
      }
      if (own < no && h == 0) {
        a.best[side][o0 + own] = bi;
        a.sbest[side][o0 + own] = bs;
      }
    }
  }
}

// exp of the reference's scores[i, j] at a mutual pair: row g0 and column g1 are packed indices, s = s[i][j] as pass 2 kept it.
__device__ __forceinline__ float mt_mutual_score(const MatchArgs& a, int g0, int g1) {
  const float s = a.sbest[0][g0];
  const float row = (s - a.lmax[0][g0]) - a.lsum[0][g0], col = (s - a.lmax[1][g1]) - a.lsum[1][g1];  // log_softmax's own order
  return expf((row + col) + (mt_logsigmoid(a.z[0][g0]) + mt_logsigmoid(a.z[1][g1])));
}

__device__ __forceinline__ void k_match_filter(const MatchArgs& a, float* lds) {
  int* totals = reinterpret_cast<int*>(lds);
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  {
    const int l = blockIdx.x;  // (the grid is the lists)
    const int o0 = a.off[0][l], m = a.off[0][l + 1] - o0, o1 = a.off[1][l], n = a.off[1][l + 1] - o1;
    const bool any = m > 0 && n > 0;  // (an empty side: no matches, and the scratch of this list was never written)
    for (int j = tid; j < n; j += 256) {
      int match = -1;
      float sc = 0.f;
      if (any) {
        const int i = a.best[1][o1 + j];
        if (a.best[0][o0 + i] == j) {  // mutual1 (then mutual0 of row i holds as well, and mscores0[i] is this value)
          sc = mt_mutual_score(a, o0 + i, o1 + j);
          if (sc > a.threshold) match = i;
        }
      }
      a.matches[1][o1 + j] = match;
      a.mscores[1][o1 + j] = sc;
    }
    int base = 0;
    for (int i0 = 0; i0 < m; i0 += 256) {
      const int i = i0 + tid;
      int j = -1;
      float sc = 0.f;
      bool valid = false;
      if (any && i < m) {
        j = a.best[0][o0 + i];
        if (a.best[1][o1 + j] == i) {
          sc = mt_mutual_score(a, o0 + i, o1 + j);
          valid = sc > a.threshold;
        }
      }
      if (i < m) {
        a.matches[0][o0 + i] = valid ? j : -1;
        a.mscores[0][o0 + i] = sc;
      }
      const unsigned long long vote = __ballot(valid);
      const int rank = __popcll(vote & ((1ull << lane) - 1ull));
      if (lane == 0) totals[wv] = __popcll(vote);
      __syncthreads();
      int before = 0, total = 0;
#pragma unroll
      for (int w = 0; w < 4; ++w) {
        const int t = totals[w];
        before += w < wv ? t : 0;
        total += t;
      }
      __syncthreads();
      if (valid) {
        const int k = o0 + base + before + rank;  // (at most m entries: inside the list's own stretch)
        a.idx0[k] = i;
        a.idx1[k] = j;
        a.score[k] = sc;
        if (a.width > 0) {
          const float x0 = a.kpts[0][2 * (int64_t)(o0 + i)], y0 = a.kpts[0][2 * (int64_t)(o0 + i) + 1];
          const float x1 = a.kpts[1][2 * (int64_t)(o1 + j)], y1 = a.kpts[1][2 * (int64_t)(o1 + j) + 1];
          a.ids_i[k] = (int64_t)truncf(y0) * a.width + (int64_t)truncf(x0);
          a.ids_j[k] = (int64_t)truncf(y1) * a.width + (int64_t)truncf(x1);
          a.points[2 * (int64_t)k] = x0;
          a.points[2 * (int64_t)k + 1] = y0;
        }
      }
      base += total;
    }
    if (tid == 0) a.count[l] = base;
  }
}

// The three passes, switched by the launch-uniform a.op.  They are NOT a kernel of their own: a kernel costs about 1.3 KB of note, symbols
// and descriptor in front of .text (half of it the hidden arguments that reading gridDim brings), the code object's read-only segment
// had 512 bytes left in its last page, and a fourth page there moves .text - every kernel of the library - by 4096 bytes, which has
// cost the rasterizer's headline forward 0.5 us before (docs/KERNEL_HISTORY.md).  They are routines of k_pose_ops<256>
// (gsr_pose_refine.h), whose launch-bound one-workgroup routines do not feel the registers and the LDS these passes take; the grid's
// extent comes in the arguments, not from gridDim.
__device__ __forceinline__ void k_match_ops(const MatchArgs& a, float* lds) {
  switch (a.op) {
    case kMtStats: k_match_stream<false>(a, lds); break;
    case kMtArgmax: k_match_stream<true>(a, lds); break;
    default: k_match_filter(a, lds); break;
  }
}

static int match_op_launch(const MatchArgs& a, dim3 grid, void* stream_);  // (gsr_pose_refine.h, next to the kernel)

// The limits of a call; on success the two totals (the last offsets) and the longest side of a list that has both sides.
static bool mt_sizes_ok(int L, const int32_t* off_m, const int32_t* off_n, int d, int64_t* total_m, int64_t* total_n, int* longest) {
  if (L < 1 || d < 1 || d > kMtChan || !off_m || !off_n) return false;
  int longest_ = 0;
  if (off_m[0] < 0 || off_n[0] < 0) return false;
  for (int l = 0; l < L; ++l) {
    const int64_t m = (int64_t)off_m[l + 1] - off_m[l], n = (int64_t)off_n[l + 1] - off_n[l];
    if (m < 0 || n < 0) return false;
    if (m > 0 && n > 0 && (m > n ? m : n) > longest_) longest_ = (int)(m > n ? m : n);
  }
  const int64_t lim = 0x7fffffff;
  if (off_m[L] > lim / d || off_n[L] > lim / d) return false;
  *total_m = off_m[L];
  *total_n = off_n[L];
  *longest = longest_;
  return true;
}
}  // namespace gsr

extern "C" {

size_t gsr_match_assignment_scratch_bytes(int L, const int32_t* offsets_m_host, const int32_t* offsets_n_host, int d) {
  int64_t tm, tn;
  int longest;
  if (!gsr::mt_sizes_ok(L, offsets_m_host, offsets_n_host, d, &tm, &tn, &longest)) return 0;
  return (size_t)(tm + tn + 1) * 16;  // (maximum, log-sum, s at the arg-maximum, the arg-maximum; one spare record: never 0 for an accepted call)
}

int gsr_match_assignment(int L, int d, float scale, float threshold, int width, const float* mdesc0, const float* mdesc1, const float* z0,
                         const float* z1, const int32_t* offsets_m_host, const int32_t* offsets_m_device, const int32_t* offsets_n_host,
                         const int32_t* offsets_n_device, const float* kpts0, const float* kpts1, void* scratch, int32_t* matches0,
                         int32_t* matches1, float* mscores0, float* mscores1, int32_t* idx0, int32_t* idx1, float* score, int64_t* ids_i,
                         int64_t* ids_j, float* points, int32_t* count, void* stream_) {
  using namespace gsr;
  int64_t tm, tn;
  int longest;
  if (!mt_sizes_ok(L, offsets_m_host, offsets_n_host, d, &tm, &tn, &longest)) return GSR_ERR_INVALID_ARGUMENT;
  if (!std::isfinite(scale) || !std::isfinite(threshold)) return GSR_ERR_INVALID_ARGUMENT;
  const bool with_kpts = kpts0 || kpts1;
  if (with_kpts && (!kpts0 || !kpts1 || width < 1 || !ids_i || !ids_j || !points)) return GSR_ERR_INVALID_ARGUMENT;
  if (!mdesc0 || !mdesc1 || !z0 || !z1 || !offsets_m_device || !offsets_n_device || !scratch || !matches0 || !matches1 || !mscores0 ||
      !mscores1 || !idx0 || !idx1 || !score || !count)
    return GSR_ERR_INVALID_ARGUMENT;
  MatchArgs a{};
  a.L = L; a.d = d; a.width = with_kpts ? width : 0; a.scale = scale; a.threshold = threshold;
  a.desc[0] = mdesc0; a.desc[1] = mdesc1; a.z[0] = z0; a.z[1] = z1; a.kpts[0] = kpts0; a.kpts[1] = kpts1;
  a.off[0] = offsets_m_device; a.off[1] = offsets_n_device;
  float* f = static_cast<float*>(scratch);
  const int64_t tt = tm + tn;
  a.lmax[0] = f; a.lmax[1] = f + tm; a.lsum[0] = f + tt; a.lsum[1] = f + tt + tm; a.sbest[0] = f + 2 * tt; a.sbest[1] = f + 2 * tt + tm;
  a.best[0] = reinterpret_cast<int32_t*>(f + 3 * tt); a.best[1] = a.best[0] + tm;
  a.matches[0] = matches0; a.matches[1] = matches1; a.mscores[0] = mscores0; a.mscores[1] = mscores1;
  a.idx0 = idx0; a.idx1 = idx1; a.count = count; a.score = score; a.points = points; a.ids_i = ids_i; a.ids_j = ids_j;
  if (longest > 0) {
    const int64_t rows = 2 * (int64_t)L;
    a.grid_rows = (int)(rows < 65535 ? rows : 65535);
    const dim3 grid((unsigned)((longest + kMaOwn - 1) / kMaOwn), (unsigned)a.grid_rows);
    a.op = kMtStats;
    if (int rc = match_op_launch(a, grid, stream_)) return rc;
    a.op = kMtArgmax;
    if (int rc = match_op_launch(a, grid, stream_)) return rc;
  }
  a.op = kMtFilter;
  return match_op_launch(a, dim3((unsigned)L), stream_);
}

}  // extern "C"

// ------------------------------------------------------------------------------------------------
// Keypoint extraction (SuperPoint.forward after its last two convolutions, reference src/model/LightGlue/lightglue/superpoint.py:52-95,
// 171-227, with the rescale of utils.py:146; definition: include/gsr.h): a batch of images in one chain of up to six launches - the
// passes of k_keypoint_ops, below, routines of k_pose_ops like the match assignment's and for the same reason.  This section stands
// in this header, behind the matcher's tail, because tests/test_abi.py pins the library's set of files by name.
//   pass kKpScores: a thread per 8 x 8 cell: the 65-way softmax (maximum, expf, the sum in channel order, one division per pixel) and
//                   the depth-to-space store of its 64 scores - the ONE dense float array of the chain, (B, H, W).  The softmax is not
//                   folded into the NMS tile load: a 32-pixel tile with its 20-pixel halo is 5.06 tiles of reads, which the score map
//                   serves from L2 as 4 bytes per pixel, while the logits would be read, and their expf evaluated, five times over.
//   pass kKpNms:    a workgroup per tile of kKpTile x kKpTile pixels.  The tile and a halo of 5 r pixels (simple_nms chains five
//                   max-pools of radius r) are loaded into LDS, -inf outside the image as max_pool2d pads; the pools are separable (a
//                   row pass into a second float array, a column pass out of it); the four masks are byte arrays and the suppressed
//                   scores are formed from scores and mask where they are read: nothing but the tile's keep bits leaves the chip, one
//                   32-bit word per tile row.  The region's rim computes with clipped windows: what is wrong there moves inward by r per
//                   pool and after five pools has not reached the tile.
//   pass kKpScan:   a workgroup per image: the words' population counts in row-major order of (row, word of the row) - which IS the
//                   row-major order of the pixels -, an exclusive scan in chunks of 2048 words, counts[b].
//   pass kKpWrite:  a thread per word: its kept pixels to rows base(b) + offset .. of the packed outputs, or, for an image that the
//                   top-k pass will order, to that image's staging rows.
//   pass kKpTopk:   (only with max_num_keypoints) a workgroup per image, nothing to do unless k < count <= capacity: rank by
//                   counting - a row's rank is the number of rows with a higher score, or an equal one and a lower row-major index -
//                   with the scores staged through LDS; rows of rank < k go to base(b) + rank.
//   pass kKpDesc:   a wave per keypoint: the four corner columns read through the descriptors' strides (lane = channel, so a
//                   channels_last map is read in full lines), their four norms and the blend's norm as xor-butterfly wave sums.
// base(b) = sum over the images before b of stored(count) = min(count, capacity), or k where the top-k cut applies: every pass forms
// it from counts on the device.  No atomics, no order that depends on scheduling: the same bits on every call.
// ------------------------------------------------------------------------------------------------
namespace gsr {
constexpr int kKpTile = 32;                                // a tile row is one word of the keep mask
constexpr int kKpMaxRadius = 4;
constexpr int kKpRegion = kKpTile + 10 * kKpMaxRadius;     // the tile with its halo of 5 r on either side
constexpr int kKpCells = kKpRegion * kKpRegion;
constexpr int kKpChan = 256;                               // the most descriptor channels
constexpr int kKpTopkChunk = 8192;                         // scores staged per round of the rank count
static_assert(3 * kKpCells <= kMtLdsFloats && kKpTopkChunk <= kMtLdsFloats, "the keypoint passes live in k_pose_ops' arena");
enum { kKpScores = 0, kKpNms = 1, kKpScan = 2, kKpWrite = 3, kKpTopk = 4, kKpDesc = 5 };

struct KeypointArgs {
  int op, B, H, W, C, r, border, k, cap, words;  // words: 32-bit mask words per image row
  float threshold;
  const float *logits, *desc, *scales;
  int64_t ds[4];                    // the descriptors' element strides (B, C, h, w)
  float* smap;                      // (B, H, W): written by kKpScores, or the caller's scores (then only read)
  uint32_t *mask, *woff, *rank;     // scratch: keep words and their exclusive offsets (B, H, words); the staging rows' ranks (B, cap)
  int32_t* spix;                    // scratch: staging rows (B, cap): flat pixel y W + x, and its score
  float* sscore;
  float *kpts, *kscores, *kdesc;
  int32_t *pixels, *counts;
};

// rows an image keeps: its count, cut to k where the top-k pass runs, to the capacity where it overflows
__device__ __forceinline__ int kp_stored(int cnt, int cap, int k) { return cnt > cap ? cap : (k > 0 && cnt > k ? k : cnt); }
__device__ __forceinline__ bool kp_staged(int cnt, int cap, int k) { return k > 0 && cnt > k && cnt <= cap; }
// base(b), the first packed row of image b: EVERY thread of the workgroup calls it (two barriers); the images before b are summed
// 256 at a time, so a thread reads b / 256 counts; lds: 4 words, free again on return
__device__ __forceinline__ int64_t kp_base(const KeypointArgs& a, int b, float* lds, int tid) {
  uint32_t* tot = reinterpret_cast<uint32_t*>(lds);
  uint32_t mine = 0;  // (the batch's rows are at most 2^31 - 1)
  for (int i = tid; i < b; i += 256) mine += (uint32_t)kp_stored(a.counts[i], a.cap, a.k);
  const uint32_t inc = wave_inclusive_scan_u32(mine);
  if ((tid & 63) == 63) tot[tid >> 6] = inc;
  __syncthreads();
  const int64_t base = (int64_t)tot[0] + tot[1] + tot[2] + tot[3];
  __syncthreads();
  return base;
}
__device__ __forceinline__ void kp_emit(const KeypointArgs& a, int b, int64_t g, int x, int y, float s) {
  a.pixels[2 * g] = x;
  a.pixels[2 * g + 1] = y;
  a.kscores[g] = s;
  float kx = (float)x, ky = (float)y;
  if (a.scales) {  // the preprocessor's rescale: (pixel + 0.5) / scale - 0.5
    kx = (kx + 0.5f) / a.scales[2 * b] - 0.5f;
    ky = (ky + 0.5f) / a.scales[2 * b + 1] - 0.5f;
  }
  a.kpts[2 * g] = kx;
  a.kpts[2 * g + 1] = ky;
}

// pass kKpScores: a thread per cell
__device__ __forceinline__ void k_keypoint_scores(const KeypointArgs& a, int tid) {
  const int h = a.H / 8, w = a.W / 8;
  const int64_t hw = (int64_t)h * w, item = (int64_t)blockIdx.x * 256 + tid;
  if (item >= (int64_t)a.B * hw) return;
  const int b = (int)(item / hw), cell = (int)(item - (int64_t)b * hw), i = cell / w, j = cell - i * w;
  const float* p = a.logits + (int64_t)b * 65 * hw + cell;
  float v[65];
  float mx = -INFINITY;
#pragma unroll
  for (int c = 0; c < 65; ++c) { v[c] = p[c * hw]; mx = fmaxf(mx, v[c]); }
  float sum = 0.f;
#pragma unroll
  for (int c = 0; c < 65; ++c) { v[c] = expf(v[c] - mx); sum += v[c]; }
  float* out = a.smap + ((int64_t)b * a.H + 8 * i) * a.W + 8 * j;  // (32-byte aligned: W is a multiple of 8)
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    float4* row = reinterpret_cast<float4*>(out + (int64_t)q * a.W);
    row[0] = make_float4(v[8 * q] / sum, v[8 * q + 1] / sum, v[8 * q + 2] / sum, v[8 * q + 3] / sum);
    row[1] = make_float4(v[8 * q + 4] / sum, v[8 * q + 5] / sum, v[8 * q + 6] / sum, v[8 * q + 7] / sum);
  }
}

// The cells e = tid, tid + 256, ... of the R x R region with their row and column, which are carried along, not divided out.
struct KpWalk {
  int R, n, e0, ly0, lx0, sy, sx;  // a step of 256 cells is sy rows and sx < R columns
};
template <class F>
__device__ __forceinline__ void kp_cells(const KpWalk& w, F f) {
  int ly = w.ly0, lx = w.lx0;
  for (int e = w.e0; e < w.n; e += 256) {
    f(e, ly, lx);
    lx += w.sx;
    ly += w.sy;
    if (lx >= w.R) { lx -= w.R; ++ly; }
  }
}
// T[e] = the maximum of src over e's row window, clipped to the region
template <class Src>
__device__ __forceinline__ void kp_pool_rows(Src src, float* T, const KpWalk& w, int r) {
  kp_cells(w, [&](int e, int ly, int lx) {
    const int lo = lx - r < 0 ? 0 : lx - r, hi = lx + r > w.R - 1 ? w.R - 1 : lx + r;
    float m = src(e - lx + lo);
    for (int c = e - lx + lo + 1; c <= e - lx + hi; ++c) m = fmaxf(m, src(c));
    T[e] = m;
  });
}
// the maximum of T over e's column window
__device__ __forceinline__ float kp_pool_col(const float* T, int R, int r, int ly, int lx) {
  const int lo = ly - r < 0 ? 0 : ly - r, hi = ly + r > R - 1 ? R - 1 : ly + r;
  float m = T[lo * R + lx];
  for (int y = lo + 1; y <= hi; ++y) m = fmaxf(m, T[y * R + lx]);
  return m;
}

// pass kKpNms: a workgroup per tile; lds: 2 kKpCells floats and 4 kKpCells bytes
__device__ __forceinline__ void k_keypoint_nms(const KeypointArgs& a, float* lds, int tid) {
  const int r = a.r, halo = 5 * r, R = kKpTile + 2 * halo;
  const int tx = blockIdx.x, ty = blockIdx.y, b = blockIdx.z;
  const int x0 = tx * kKpTile - halo, y0 = ty * kKpTile - halo;
  KpWalk w;
  w.R = R; w.n = R * R; w.e0 = tid; w.ly0 = tid / R; w.lx0 = tid - w.ly0 * R; w.sy = 256 / R; w.sx = 256 - w.sy * R;
  float* S = lds;
  float* T = lds + kKpCells;
  uint8_t* M = reinterpret_cast<uint8_t*>(lds + 2 * kKpCells);  // max_mask
  uint8_t* P = M + kKpCells;                                    // a mask's row pass
  uint8_t* Q = P + kKpCells;                                    // supp_mask
  uint8_t* I = Q + kKpCells;                                    // inside the image
  const float* img = a.smap + (int64_t)b * a.H * a.W;
  kp_cells(w, [&](int e, int ly, int lx) {
    const int gy = y0 + ly, gx = x0 + lx;
    const bool in = gy >= 0 && gy < a.H && gx >= 0 && gx < a.W;
    I[e] = in;
    S[e] = in ? img[(int64_t)gy * a.W + gx] : -INFINITY;  // as max_pool2d pads
  });
  __syncthreads();
  kp_pool_rows([&](int e) { return S[e]; }, T, w, r);
  __syncthreads();
  kp_cells(w, [&](int e, int ly, int lx) { M[e] = I[e] && S[e] == kp_pool_col(T, R, r, ly, lx); });
  __syncthreads();
  for (int round = 0; round < 2; ++round) {  // two rounds, not "until stable": the definition
    kp_cells(w, [&](int e, int ly, int lx) {
      const int lo = lx - r < 0 ? 0 : lx - r, hi = lx + r > R - 1 ? R - 1 : lx + r;
      uint8_t any = 0;
      for (int c = e - lx + lo; c <= e - lx + hi; ++c) any |= M[c];
      P[e] = any;
    });
    __syncthreads();
    kp_cells(w, [&](int e, int ly, int lx) {
      const int lo = ly - r < 0 ? 0 : ly - r, hi = ly + r > R - 1 ? R - 1 : ly + r;
      uint8_t any = 0;
      for (int y = lo; y <= hi; ++y) any |= P[y * R + lx];
      Q[e] = any;
    });
    __syncthreads();
    // supp_scores: 0 where suppressed, the score elsewhere; outside the image the pool's padding
    auto supp = [&](int e) { return !I[e] ? -INFINITY : (Q[e] ? 0.f : S[e]); };
    kp_pool_rows(supp, T, w, r);
    __syncthreads();
    kp_cells(w, [&](int e, int ly, int lx) {
      if (!Q[e] && I[e] && S[e] == kp_pool_col(T, R, r, ly, lx)) M[e] = 1;  // (not suppressed: its supp_score is its score)
    });
    __syncthreads();
  }
  const int wv = tid >> 6, lane = tid & 63;
  for (int q = 0; q < kKpTile / 8; ++q) {  // a wave: two tile rows at a time
    const int ly = 2 * (wv * (kKpTile / 8) + q) + (lane >> 5), lx = lane & 31;
    const int e = (ly + halo) * R + lx + halo, gy = ty * kKpTile + ly, gx = tx * kKpTile + lx;
    const bool keep = gy >= a.border && gy < a.H - a.border && gx >= a.border && gx < a.W - a.border && M[e] && S[e] > a.threshold;
    const unsigned long long vote = __ballot(keep);
    if (lx == 0 && gy < a.H) a.mask[((int64_t)b * a.H + gy) * a.words + tx] = (uint32_t)(vote >> (lane & 32));
  }
}

// pass kKpScan: a workgroup per image; lds: 4 words
__device__ __forceinline__ void k_keypoint_scan(const KeypointArgs& a, float* lds, int tid) {
  uint32_t* tot = reinterpret_cast<uint32_t*>(lds);
  const int b = blockIdx.x, wv = tid >> 6, lane = tid & 63;
  const int64_t nw = (int64_t)a.H * a.words;
  const uint32_t* mask = a.mask + b * nw;
  uint32_t* woff = a.woff + b * nw;
  uint32_t running = 0;
  for (int64_t base = 0; base < nw; base += 2048) {
    const int64_t i0 = base + tid * 8;
    uint32_t c[8], mine = 0;
#pragma unroll
    for (int q = 0; q < 8; ++q) { c[q] = i0 + q < nw ? (uint32_t)__popc(mask[i0 + q]) : 0u; mine += c[q]; }
    const uint32_t inc = wave_inclusive_scan_u32(mine);
    if (lane == 63) tot[wv] = inc;
    __syncthreads();
    uint32_t pre = running + inc - mine, all = 0;
#pragma unroll
    for (int v = 0; v < 4; ++v) { if (v < wv) pre += tot[v]; all += tot[v]; }
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      if (i0 + q < nw) woff[i0 + q] = pre;
      pre += c[q];
    }
    running += all;
    __syncthreads();
  }
  if (tid == 0) a.counts[b] = (int32_t)running;
}

// pass kKpWrite: a thread per word
__device__ __forceinline__ void k_keypoint_write(const KeypointArgs& a, float* lds, int tid) {
  const int b = blockIdx.y;
  const int64_t nw = (int64_t)a.H * a.words, idx = (int64_t)blockIdx.x * 256 + tid;
  const bool staged = kp_staged(a.counts[b], a.cap, a.k);                        // (uniform over the workgroup)
  const int64_t base = staged ? (int64_t)b * a.cap : kp_base(a, b, lds, tid);  // (before any thread leaves)
  if (idx >= nw) return;
  uint32_t word = a.mask[b * nw + idx];
  if (!word) return;
  uint32_t off = a.woff[b * nw + idx];
  const int y = (int)(idx / a.words), wc = (int)(idx - (int64_t)y * a.words);
  for (; word && off < (uint32_t)a.cap; word &= word - 1, ++off) {  // NOTHING past the image's capacity rows
    const int x = wc * 32 + __ffs((int)word) - 1;
    const float s = a.smap[((int64_t)b * a.H + y) * a.W + x];
    if (staged) {
      a.spix[base + off] = y * a.W + x;
      a.sscore[base + off] = s;
    } else {
      kp_emit(a, b, base + off, x, y, s);
    }
  }
}

// pass kKpTopk: a workgroup per image; lds: kKpTopkChunk floats
__device__ __forceinline__ void k_keypoint_topk(const KeypointArgs& a, float* lds, int tid) {
  const int b = blockIdx.x, cnt = a.counts[b];
  if (!kp_staged(cnt, a.cap, a.k)) return;  // (uniform over the workgroup)
  const float* sc = a.sscore + (int64_t)b * a.cap;
  const int32_t* px = a.spix + (int64_t)b * a.cap;
  uint32_t* rank = a.rank + (int64_t)b * a.cap;  // (a thread reads back only what it wrote)
  for (int c0 = 0; c0 < cnt; c0 += kKpTopkChunk) {
    const int m = cnt - c0 < kKpTopkChunk ? cnt - c0 : kKpTopkChunk;
    for (int j = tid; j < m; j += 256) lds[j] = sc[c0 + j];
    __syncthreads();
    for (int i = tid; i < cnt; i += 256) {
      const float s = sc[i];
      uint32_t rk = c0 ? rank[i] : 0u;
      for (int j = 0; j < m; ++j) rk += (lds[j] > s) || (lds[j] == s && c0 + j < i);  // ties: the lower row-major index first
      rank[i] = rk;
    }
    __syncthreads();
  }
  const int64_t base = kp_base(a, b, lds, tid);
  for (int i = tid; i < cnt; i += 256)
    if (rank[i] < (uint32_t)a.k) kp_emit(a, b, base + rank[i], px[i] % a.W, px[i] / a.W, sc[i]);
}

// pass kKpDesc: a wave per keypoint
__device__ __forceinline__ void k_keypoint_desc(const KeypointArgs& a, float* lds, int tid) {
  const int b = blockIdx.y, lane = tid & 63, j = blockIdx.x * 4 + (tid >> 6), stored = kp_stored(a.counts[b], a.cap, a.k);
  if ((int)blockIdx.x * 4 >= stored) return;  // (uniform over the workgroup: most of the grid leaves here, before the base)
  const int64_t g = kp_base(a, b, lds, tid) + j;
  if (j >= stored) return;  // (uniform over the wave)
  const int h = a.H / 8, w = a.W / 8;
  const float ix = ((float)a.pixels[2 * g] - 3.5f) / ((float)(8 * w) - 4.5f) * (float)(w - 1);
  const float iy = ((float)a.pixels[2 * g + 1] - 3.5f) / ((float)(8 * h) - 4.5f) * (float)(h - 1);
  const float fx0 = floorf(ix), fy0 = floorf(iy), tx = ix - fx0, ty = iy - fy0;
  const int cx = (int)fx0, cy = (int)fy0;
  const float wt[4] = {(1.f - tx) * (1.f - ty), tx * (1.f - ty), (1.f - tx) * ty, tx * ty};
  const float* d = a.desc + b * a.ds[0];
  float v[4][kKpChan / 64], nrm[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int xi = cx + (q & 1), yi = cy + (q >> 1);
    const bool in = xi >= 0 && xi < w && yi >= 0 && yi < h;  // zeros outside, as grid_sample pads
    float ss = 0.f;
#pragma unroll
    for (int i = 0; i < kKpChan / 64; ++i) {
      const int c = lane + 64 * i;
      v[q][i] = in && c < a.C ? d[c * a.ds[1] + yi * a.ds[2] + xi * a.ds[3]] : 0.f;
      ss += v[q][i] * v[q][i];
    }
    nrm[q] = fmaxf(sqrtf(wave_sum(ss)), 1e-12f);
  }
  float o[kKpChan / 64], ss = 0.f;
#pragma unroll
  for (int i = 0; i < kKpChan / 64; ++i) {
    o[i] = ((wt[0] * (v[0][i] / nrm[0]) + wt[1] * (v[1][i] / nrm[1])) + wt[2] * (v[2][i] / nrm[2])) + wt[3] * (v[3][i] / nrm[3]);
    ss += o[i] * o[i];
  }
  const float n = fmaxf(sqrtf(wave_sum(ss)), 1e-12f);
#pragma unroll
  for (int i = 0; i < kKpChan / 64; ++i)
    if (lane + 64 * i < a.C) a.kdesc[g * a.C + lane + 64 * i] = o[i] / n;
}

// The six passes as routines of k_pose_ops (gsr_pose_refine.h), op kPoseOpKeypoints, switched by the launch-uniform a.op.
__device__ __forceinline__ void k_keypoint_ops(const KeypointArgs& a, float* lds) {
  const int tid = threadIdx.x;
  switch (a.op) {
    case kKpScores: k_keypoint_scores(a, tid); break;
    case kKpNms: k_keypoint_nms(a, lds, tid); break;
    case kKpScan: k_keypoint_scan(a, lds, tid); break;
    case kKpWrite: k_keypoint_write(a, lds, tid); break;
    case kKpTopk: k_keypoint_topk(a, lds, tid); break;
    default: k_keypoint_desc(a, lds, tid); break;
  }
}

static int keypoint_op_launch(const KeypointArgs& a, dim3 grid, void* stream_);  // (gsr_pose_refine.h, next to the kernel)

// The limits of a call.  C == 0: no descriptors.
static bool kp_sizes_ok(int mode, int B, int H, int W, int C, int cap) {
  if (B < 1 || B > 65535 || H < 1 || W < 1 || C < 0 || C > kKpChan || cap < 1) return false;
  if ((mode == GSR_KEYPOINTS_FROM_LOGITS || C > 0) && (H % 8 || W % 8)) return false;
  const int64_t lim = 0x7fffffff;
  if ((int64_t)H * W > lim / B || (int64_t)cap * (C > 2 ? C : 2) > lim / B) return false;
  return (H + kKpTile - 1) / kKpTile <= 65535;
}
static int64_t kp_words(int H, int W) { return (int64_t)H * ((W + kKpTile - 1) / kKpTile); }
}  // namespace gsr

extern "C" {

int gsr_keypoints_tile(void) { return gsr::kKpTile; }

size_t gsr_keypoints_scratch_bytes(int B, int height, int width, int C, int capacity) {
  if (!gsr::kp_sizes_ok(GSR_KEYPOINTS_FROM_SCORES, B, height, width, C, capacity)) return 0;
  return (size_t)B * (2 * (size_t)gsr::kp_words(height, width) + 3 * (size_t)capacity) * 4;
}

int gsr_keypoints(int mode, int B, int height, int width, int C, int nms_radius, float threshold, int remove_borders, int max_num_keypoints,
                  int capacity, const float* logits, float* scores, const float* descriptors, const int64_t* descriptor_strides,
                  const float* scales, void* scratch, float* keypoints, int32_t* pixels, float* keypoint_scores, float* out_descriptors,
                  int32_t* counts, void* stream_) {
  using namespace gsr;
  if (mode != GSR_KEYPOINTS_FROM_LOGITS && mode != GSR_KEYPOINTS_FROM_SCORES) return GSR_ERR_INVALID_ARGUMENT;
  if (!kp_sizes_ok(mode, B, height, width, C, capacity)) return GSR_ERR_INVALID_ARGUMENT;
  if (nms_radius < 0 || nms_radius > kKpMaxRadius || remove_borders < 0 || max_num_keypoints < 0) return GSR_ERR_INVALID_ARGUMENT;
  if (!std::isfinite(threshold) || threshold < 0.f) return GSR_ERR_INVALID_ARGUMENT;
  if (!scores || !scratch || !keypoints || !pixels || !keypoint_scores || !counts) return GSR_ERR_INVALID_ARGUMENT;
  if (mode == GSR_KEYPOINTS_FROM_LOGITS && !logits) return GSR_ERR_INVALID_ARGUMENT;
  if (C > 0 && (!descriptors || !descriptor_strides || !out_descriptors)) return GSR_ERR_INVALID_ARGUMENT;
  KeypointArgs a{};
  a.B = B; a.H = height; a.W = width; a.C = C; a.r = nms_radius; a.border = remove_borders; a.k = max_num_keypoints; a.cap = capacity;
  a.words = (width + kKpTile - 1) / kKpTile;
  a.threshold = threshold; a.logits = logits; a.desc = descriptors; a.scales = scales; a.smap = scores;
  if (C > 0)
    for (int s = 0; s < 4; ++s) a.ds[s] = descriptor_strides[s];
  const int64_t nw = kp_words(height, width);
  uint32_t* u = static_cast<uint32_t*>(scratch);
  a.mask = u; a.woff = u + B * nw; a.rank = u + 2 * B * nw;
  a.spix = reinterpret_cast<int32_t*>(a.rank + (int64_t)B * capacity);
  a.sscore = reinterpret_cast<float*>(a.spix + (int64_t)B * capacity);
  a.kpts = keypoints; a.pixels = pixels; a.kscores = keypoint_scores; a.kdesc = out_descriptors; a.counts = counts;
  if (mode == GSR_KEYPOINTS_FROM_LOGITS) {
    a.op = kKpScores;
    if (int rc = keypoint_op_launch(a, dim3((unsigned)(((int64_t)B * (height / 8) * (width / 8) + 255) / 256)), stream_)) return rc;
  }
  a.op = kKpNms;
  if (int rc = keypoint_op_launch(a, dim3((unsigned)a.words, (unsigned)((height + kKpTile - 1) / kKpTile), (unsigned)B), stream_)) return rc;
  a.op = kKpScan;
  if (int rc = keypoint_op_launch(a, dim3((unsigned)B), stream_)) return rc;
  a.op = kKpWrite;
  if (int rc = keypoint_op_launch(a, dim3((unsigned)((nw + 255) / 256), (unsigned)B), stream_)) return rc;
  if (max_num_keypoints > 0) {
    a.op = kKpTopk;
    if (int rc = keypoint_op_launch(a, dim3((unsigned)B), stream_)) return rc;
  }
  if (C > 0) {
    a.op = kKpDesc;
    if (int rc = keypoint_op_launch(a, dim3((unsigned)((capacity + 3) / 4), (unsigned)B), stream_)) return rc;
  }
  return GSR_OK;
}

}  // extern "C"
