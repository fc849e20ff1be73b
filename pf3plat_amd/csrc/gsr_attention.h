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
