#pragma once
// B1 / B2 backward and the pose reductions.
#include "gsr_common.h"
#include "gsr_tiles_fwd.h"

namespace gsr {

// ------------------------------------------------------------------------------------------------
// B1: backward blend ([EXT] backward.cu renderCUDA; oracle blend_backward).  One workgroup of four wavefronts per 8x8 tile.
// The reference replays the list back to front with T <- T/(1-alpha) and accum <- alpha c + (1-alpha) accum.  With
// Q = (accum . dL/dpixel) - the blended contribution of everything DEEPER than the splat, normalised by the transmittance
// behind it; behind the last splat Q = bg . dL/dpixel - that is
//     dL/dalpha = T (c.g - Q),          Q <- alpha (c.g) + (1 - alpha) Q,          T <- T / (1 - alpha)
// Q's recurrence is linear in Q and T's a plain product, so - exactly as in the forward kernel - the list is cut into batches
// of kBB entries (walked back to front) and every batch into four SEGMENTS of 8 consecutive entries, one per wave, and the only
// division left is ONE reciprocal per segment (the product P of its (1 - alpha)); inside a segment T runs front to back by
// products.  (Until late in round 2 the kernel carried Bg = T Q instead and paid a reciprocal of (1 - alpha) per entry.)
//   stage E (batch it+1), lane = pixel: G = exp2(power) and alpha (both 0 unless the forward blended this splat at this
//            pixel: not skipped and index < the pixel's last contributor), c.g and 1 - alpha into REGISTERS, and the segment's
//            own replay of Q from 0: (1 / P, P, q') -> LDS;
//   stage A (batch it),   lane = pixel: every wave reads the four triples and forms T in front of its segment and Q at its
//            back end by the same chain as every other wave, then runs its 8 entries - T front to back, Q back to front: w and
//            G dL/dalpha go to a per-wave LDS tile (no barrier: written and read by the same wave);
//   stage R (batch it),   lane = (entry 0..7, pixel row 0..7): per-splat gradients.  Each lane sums its row of 8 pixels
//            in registers - only q, q dx, q dx^2 and w g need per-pixel work, dy is constant along a row - a 3-step DPP
//            all-reduce over the 8 lanes of an entry finishes the sums, and two atomic instructions - four whole rows each,
//            one fabric transaction per row (see `scatter`) - add 8 splats x 10 values into the per-(view, Gaussian)
//            screen-space accumulator:
//              scratch[.. * 12 + {0,1: dmean2D  2,3,4: dconic  5: dopacity  6,7,8: dcolor  9: dextra}]
// Gather pipeline: the list ids of a batch are requested four iterations ahead, its records three ahead, and they are parked in
// LDS two ahead (by the wave that requested them, before that iteration's atomics).  One barrier per batch.  SQ counters of the previous shape (one chain wave + three helpers exchanging alpha, c.g, w and
// dL/dalpha through LDS, exp2 evaluated again in the reduction): 88 VALU instructions per entry and tile, VALU-issue bound.
// ------------------------------------------------------------------------------------------------
constexpr int kBS = 8;                       // entries per wave per batch = entries per reduction pass
constexpr int kBwdWaves = 4;
constexpr int kBB = kBS * kBwdWaves;         // 32 list entries per batch
constexpr int kBwdThreads = 64 * kBwdWaves;  // 256

template <int CTRL>
__device__ __forceinline__ float dpp_row_add(float v) {
  return v + __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xf, 0xf, false));
}
// Sum over the 16 lanes of a DPP row, result in every lane of the row.
__device__ __forceinline__ float row_allreduce(float v) {
  v = dpp_row_add<0x128>(v);  // row_ror:8
  v = dpp_row_add<0x124>(v);  // row_ror:4
  v = dpp_row_add<0x122>(v);  // row_ror:2
  v = dpp_row_add<0x121>(v);  // row_ror:1
  return v;
}
// Sum over aligned groups of 8 lanes, result in every lane of the group.
__device__ __forceinline__ float oct_allreduce(float v) {
  v = dpp_row_add<0x141>(v);  // row_half_mirror: i <-> 7 - i
  v = dpp_row_add<0xB1>(v);   // quad_perm [1,0,3,2]
  v = dpp_row_add<0x4E>(v);   // quad_perm [2,3,0,1]
  return v;
}

// Fixed-point form of a gradient contribution (GSR_FLAG_DETERMINISTIC): 2^-32 resolution, clamped to +-2^30 so that the
// 64-bit sum of any realistic number of contributions cannot wrap.  Integer adds commute: the sum does not depend on order.
constexpr float kFixScale = 4294967296.f, kFixInv = 1.f / 4294967296.f;
__device__ __forceinline__ unsigned long long to_fixed(float v) {
  v = fminf(fmaxf(v, -1073741824.f), 1073741824.f);
  return (unsigned long long)(long long)__float2ll_rn(v * kFixScale);
}
__device__ __forceinline__ float from_fixed(long long x) { return (float)x * kFixInv; }
// The fixed step is absolute, the cotangents of a training loss are not of order one (a mean over the pixels of a batch hands
// back 1e-7 and less per pixel): the deterministic instances work in units of the view's largest cotangent.  One word per view
// behind the accumulator rows (both homes of the rows: the caller's scratch, geom under GSR_FLAG_BACKWARD_FOLLOWS) holds the float
// bits of the largest finite |value| of the view's cotangent images (k_cotangent_max: an integer max, order-free).  k_blend_bwd
// multiplies what it loads by 2^e, k_preprocess_bwd_det the sums it reads back by 2^-e, with max 2^e in [1, 2): both exact.  A zero or
// subnormal maximum gives e = 0; the biased exponent is held to 1..253 so that 2^e and 2^-e are both normal floats.
__device__ __forceinline__ const uint32_t* det_max_words(const Params& p) {
  return reinterpret_cast<const uint32_t*>(reinterpret_cast<const long long*>(p.scratch) +
                                           (size_t)p.d.num_views * p.d.num_gaussians * GSR_SCREEN_GRAD_FLOATS);
}
__device__ __forceinline__ float det_scale_up(uint32_t max_bits) {
  const uint32_t ef = min(max_bits >> 23, 253u);
  return ef == 0u ? 1.f : __uint_as_float((254u - ef) << 23);
}
__device__ __forceinline__ float det_scale_down(uint32_t max_bits) {
  const uint32_t ef = min(max_bits >> 23, 253u);
  return ef == 0u ? 1.f : __uint_as_float(ef << 23);
}
// grid (views, blocks): every block folds its share of the view's cotangent images into the view's word (zero-filled by the call).
// Non-finite entries (an all-ones exponent) are passed over.
__global__ __launch_bounds__(256) void k_cotangent_max(const Params p, uint32_t* words) {
  const int v = blockIdx.x;
  const size_t HW = (size_t)p.g.H * p.g.W;
  const float* img[3] = {p.dL_dcolor + (size_t)v * 3 * HW, p.dL_dextra_img ? p.dL_dextra_img + (size_t)v * HW : nullptr,
                         p.dL_dalpha_img ? p.dL_dalpha_img + (size_t)v * HW : nullptr};
  const size_t len[3] = {3 * HW, HW, HW};
  uint32_t m = 0;
  auto take = [&](float x) {
    const uint32_t b = __float_as_uint(x) & 0x7fffffffu;
    m = b < 0x7f800000u ? max(m, b) : m;
  };
  const size_t tid = (size_t)blockIdx.y * 256 + threadIdx.x, nthr = (size_t)gridDim.y * 256;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    if (!img[k]) continue;
    const size_t n4 = (reinterpret_cast<uintptr_t>(img[k]) & 15) == 0 ? len[k] >> 2 : 0;
    for (size_t i = tid; i < n4; i += nthr) {
      const float4 q = reinterpret_cast<const float4*>(img[k])[i];
      take(q.x); take(q.y); take(q.z); take(q.w);
    }
    for (size_t i = (n4 << 2) + tid; i < len[k]; i += nthr) take(img[k][i]);
  }
  // one atomic per workgroup, and only where it can still raise the word: atomics on one address are serialised on the memory side
  // (blend_bwd stage of the deterministic mode, 3 views of 256 x 256, 100.3 us without this launch: 132.8 with one atomic per wave of
  // 192 workgroups per view, 117.8 with 64 workgroups, 111.1 as it is - what is left is the launch itself and the zero-fill of the words)
  __shared__ uint32_t part[4];
  m = wave_max_u32(m);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
    m = max(max(part[0], part[1]), max(part[2], part[3]));
    if (m > __hip_atomic_load(words + v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(words + v, m);
  }
}

// Which tile a workgroup of k_blend_bwd takes.  A compute unit holds four workgroups of the launch (blocks b, b + 256, b + 512,
// b + 768 of the first round: HW_ID stamps) and, VALU-bound, is busy for the SUM of their tiles' batches (least squares over
// the 256 CUs of the 300 k / 256 x 256 workload: end = 0.93 us x sum + 0.0 x max); with the tiles in image order the heaviest
// CU carried 48 batches against a mean of 39.5.  The tiles of an XCD stay on that XCD (their records are in ITS L2: handing
// tiles out across the whole chip by load was measured - the gathers then miss, prologue 3.0 -> 4.1 us, no gain), but inside
// the XCD they are dealt to its 32 CUs heaviest first, every other round mirrored.  Work of a tile = list entries the forward
// walked (Params::tile_total); every workgroup finds its own tile: a selection by bisection over the <= 256 keys of its XCD, one wave, ballots only.
// (kBalanceMax, deal_key, deal_position: beside xcd_remap, shared with the forward's deal.)

// kAlpha (GsrBackwardOptions.dL_dalpha_img): a loss on the accumulated alpha A = 1 - T_final.  dA/dalpha_j = T_final / (1 - alpha_j) is the
// background term's derivative with the sign turned, so dL/dA enters where the background does: Q starts from bg.g - g_A.
template <bool kExtra, bool kDet, bool kAlpha = false>
__global__ __launch_bounds__(kBwdThreads, 4) void k_blend_bwd(const Params p) {
  __shared__ __attribute__((aligned(16))) float sW[kBwdWaves][kBS][64];  // A -> R, per wave: blend weight w
  __shared__ __attribute__((aligned(16))) float sQ[kBwdWaves][kBS][64];  // A -> R, per wave: G dL/dalpha
  __shared__ float sR[2][kBwdWaves][64], sP[2][kBwdWaves][64], sB[2][kBwdWaves][64];  // E -> A: segment (1/P, P, q') of iteration it in [it & 1]
  __shared__ float4 sGeo[4][kBB];   // x, y, a2, b2
  __shared__ float4 sGeo2[4][kBB];  // c2, opacity, id bits, 0
  __shared__ float4 sCol[4][kBB];   // r, g, b, extra
  __shared__ __attribute__((aligned(16))) float sG[4][64];  // dL/dpixel (r, g, b, extra) of the tile's 64 pixels
  const Grid& g = p.g;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int v = blockIdx.y;
  int t = xcd_remap(blockIdx.x, g.T);
  {
    __shared__ int sPick;
    const int xcd = (int)blockIdx.x & 7, k = (int)blockIdx.x >> 3, q8 = g.T >> 3, r8 = g.T & 7;
    const int cnt = q8 + (xcd < r8 ? 1 : 0), base = t - k;  // this XCD's tiles: [base, base + cnt)
    if (cnt <= kBalanceMax) {
      if (wave == 0) {
        // keys (deal_key): up to four per lane; a bijection of the XCD's tiles whatever tile_total holds
        const uint32_t* tot = p.tile_total + (size_t)v * g.T + base;
        uint32_t key[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const int i = lane + 64 * c;
          key[c] = i < cnt ? deal_key(tot[i], i) : 0u;
        }
        const int want = deal_position(k, cnt);  // position of this block in heaviest-first order
        // the key at that position: the largest X with more than `want` keys >= X, bit by bit from the top bit of the largest key
        const uint32_t top = wave_max_u32(max(max(key[0], key[1]), max(key[2], key[3])));
        uint32_t X = 0;
        for (int bit = 31 - __builtin_clz(top | 1u); bit >= 0; --bit) {
          const uint32_t cand = X | (1u << bit);
          int n = __builtin_popcountll(__ballot(key[0] >= cand)) + __builtin_popcountll(__ballot(key[1] >= cand));
          if (cnt > 128) n += __builtin_popcountll(__ballot(key[2] >= cand)) + __builtin_popcountll(__ballot(key[3] >= cand));
          X = n > want ? cand : X;
        }
        if (lane == 0) sPick = 255 - (int)(X & 255u);
      }
      __syncthreads();
      t = base + sPick;
    }
  }
  const int tx = t % g.sgx, ty = t / g.sgx;
#ifdef GSR_BWD_LONE  // measurement aid: one workgroup per CU (how fast is a tile that has its SIMDs to itself?)
  if (blockIdx.x >= 256 * GSR_BWD_LONE) return;
#endif
  const bool dbg = GSR_ABL(p.d.flags, GSR_FLAG_DEBUG_TIMING) && threadIdx.x == 0;  // measurement aid (tools/bwd_timeline.py)
  unsigned long long* stamp = p.keys + ((size_t)v * g.T + blockIdx.x) * 4;          // the forward's keys are dead by now
  if (dbg) stamp[0] = __builtin_amdgcn_s_memrealtime();
  const uint2 rg = p.ranges[(size_t)v * g.T + t];
  const uint32_t n = rg.y - rg.x;
  const size_t HW = (size_t)g.H * g.W;
  const GeomRec* geom = p.geom + (size_t)v * p.d.num_gaussians;
  const float4* rgbc = p.rgbc + (size_t)v * p.d.num_gaussians;
  const uint32_t* plist = p.point_list + rg.x;
  float* scratch = p.scratch + (size_t)v * p.d.num_gaussians * GSR_SCREEN_GRAD_FLOATS;
  const GsrView& cam = p.views[v];
  const float* dcol = p.dL_dcolor + (size_t)v * 3 * HW;
  const float* dext = kExtra ? p.dL_dextra_img + (size_t)v * HW : nullptr;
  (void)n;

  // ---- lane = pixel view (stages E, A)
  const int pxi = tx * 8 + (lane & 7), pyi = ty * 8 + (lane >> 3);
  const bool inside = pxi < g.W && pyi < g.H;
  const float pxf = (float)pxi, pyf = (float)pyi;
  const size_t pix = (size_t)pyi * g.W + pxi;
  const uint32_t my_last = inside ? p.n_contrib[(size_t)v * HW + pix] : 0u;
  const uint32_t nmax = wave_max_u32(my_last);
  if (nmax == 0) return;  // uniform over the workgroup: every wave holds the same 64 pixels
  float g0 = 0, g1 = 0, g2 = 0, ge = 0;
  if (inside) {
    g0 = dcol[pix]; g1 = dcol[HW + pix]; g2 = dcol[2 * HW + pix];
    if (kExtra) ge = dext[pix];
  }
  const float up = kDet ? det_scale_up(det_max_words(p)[v]) : 1.f;  // (det_max_words: the view's cotangents in units of their largest)
  if (kDet) { g0 *= up; g1 *= up; g2 *= up; ge *= up; }
  // ---- lane = (entry, pixel row) view (stage R): dL/dpixel of this lane's row of 8 pixels
  const int er = lane >> 3, pr = lane & 7;
  const int rpy = ty * 8 + pr, rpx0 = tx * 8;
  // dL/dpixel of the tile for that view, by channel, in LDS (1 KB): 24 - 32 registers per lane as arrays
  if (wave == 0) {
    sG[0][lane] = g0; sG[1][lane] = g1; sG[2][lane] = g2;
    if (kExtra) sG[3][lane] = ge;
  }
  // workgroup-uniform: held in scalar registers (the kExtra instances are at the 128-register limit)
  const float hW = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(0.5f * (float)g.W)));
  const float hH = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(0.5f * (float)g.H)));
  const float cpr = pr == 0 ? hW * kLn2 : pr == 1 ? hH * kLn2 : -0.5f;  // stage R: what float pr of a row is scaled by (besides the opacity)

  const uint32_t nbat = (nmax + kBB - 1) / kBB;
  // iteration `it` works on batch nbat-1-it; ring slots are indexed by the iteration number
  auto batch_of = [&](uint32_t it) { return nbat - 1 - it; };

  // the lane number formed where it is used (two instructions) rather than held in a register across the loop: the kExtra
  // instances sit at the 128-register limit and this was the value the compiler chose to spill
  auto lane_now = [&]() -> uint32_t {
    if (!kExtra) return (uint32_t)lane;
    uint32_t z = 0;
    asm volatile("" : "+v"(z));
    return __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, z));
  };
  // lane = entry.  The gather is ISSUED at the top of an iteration and its values are first touched (exp2-domain scaling, LDS
  // write) by park() at the end: arithmetic on them right behind the loads made the staging wave - and through the batch's
  // barrier the whole tile - wait a full memory round trip at the top of every iteration.
  auto stage = [&](uint32_t it, float4& r0, float4& r1, float4& rc, uint32_t id) {
    r0 = make_float4(0, 0, 0, 0); r1 = r0; rc = r0;
    const uint32_t ln = lane_now();
    const uint32_t idx = batch_of(it) * kBB + ln;
    if (ln < kBB && idx < nmax) {
      const GeomRec* r = geom + id;
      r0 = r->q0; r1 = r->q1;
      rc = rgbc[id];
    }
  };
  auto park = [&](int ring, float4 q0, float4 q1, const float4 col, uint32_t id) {  // lanes past the list hold zeros (id 0)
    const float ex = kExtra ? q1.z : 0.f;
    to_exp2_domain(q0, q1);
    if (lane_now() < kBB) {
      const uint32_t ln = lane_now();
      sGeo[ring][ln] = q0; sGeo2[ring][ln] = make_float4(q1.x, q1.y, __uint_as_float(id), 0.f);
      sCol[ring][ln] = make_float4(col.x, col.y, col.z, ex);
    }
  };
  auto load_ids = [&](uint32_t it) -> uint32_t {
    if (it >= nbat) return 0u;
    const uint32_t ln = lane_now();
    const uint32_t idx = batch_of(it) * kBB + ln;
    return (ln < kBB && idx < nmax) ? plist[idx] : 0u;
  };

  float al[kBS], Gc[kBS], cgv[kBS], om[kBS];  // this wave's segment of the batch about to be replayed (om = 1 - alpha)
  const int e0 = wave * kBS;
  auto eval = [&](uint32_t it) {  // stage E
    const int ring = it & 3;
    const uint32_t base = batch_of(it) * kBB + e0;
    // entry u of the segment is in front of the pixel's last one <=> u < rem.  (A wave-uniform second copy of the loop for segments
    // in front of EVERY pixel's last contributor, its index tests folded away, costs more instruction fetch than it saves: DESIGN 8)
    const uint32_t rem = my_last > base ? my_last - base : 0u;
    int es = e0;  // opaque copy: the three LDS addresses are then formed here, per batch, instead of living in three registers
    if (kExtra) asm volatile("" : "+v"(es));  // across the whole loop (the kExtra instances spilled exactly those)
    {
#pragma unroll
      for (int u = 0; u < kBS; ++u) {
        const float4 a = sGeo[ring][es + u], a2 = sGeo2[ring][es + u], c = sCol[ring][es + u];
        const float dx = a.x - pxf, dy = a.y - pyf;
        const float p2 = splat_p2(a.z, a.w, a2.x, dx, dy);
        const float G = __builtin_amdgcn_exp2f(p2);
        const float og = a2.y * G;
        const bool contrib = (uint32_t)u < rem && !(p2 > 0.f) && !(og < 1.0f / 255.0f);  // alpha < 1/255 <=> o G < 1/255
        al[u] = contrib ? fminf(0.99f, og) : 0.f;
        Gc[u] = contrib ? G : 0.f;
        float cg = c.x * g0;
        cg = __builtin_fmaf(c.y, g1, cg);
        cg = __builtin_fmaf(c.z, g2, cg);
        if (kExtra) cg = __builtin_fmaf(c.w, ge, cg);
        cgv[u] = cg;
        om[u] = 1.f - al[u];
      }
    }
    float Pl = 1.f, ql = 0.f;  // the segment's own product of (1 - alpha) and its replay of Q from 0, back to front
#pragma unroll
    for (int u = kBS - 1; u >= 0; --u) {
      Pl *= om[u];
      ql = __builtin_fmaf(om[u], ql, al[u] * cgv[u]);
    }
    sR[it & 1][wave][lane] = __builtin_amdgcn_rcpf(Pl);  // the one division of the segment
    sP[it & 1][wave][lane] = Pl;
    sB[it & 1][wave][lane] = ql;
  };
  auto replay = [&](float T, float q) {  // stage A: T in FRONT of this wave's segment, Q at its back end
#pragma unroll
    for (int u = 0; u < kBS; ++u) {  // front to back: the transmittance in front of every splat, by products only
      sW[wave][u][lane] = al[u] * T;
      Gc[u] *= T;
      T *= om[u];
    }
#pragma unroll
    for (int u = kBS - 1; u >= 0; --u) {  // back to front: Q, and G dL/dalpha = G T (c.g - Q)
      const float d = cgv[u] - q;
      sQ[wave][u][lane] = Gc[u] * d;
      q = __builtin_fmaf(al[u], d, q);  // alpha c.g + (1 - alpha) Q = Q + alpha (c.g - Q): the difference is already there
    }
  };
  struct RowSum { float val, tail; uint32_t id; };
  auto reduce = [&](uint32_t it) -> RowSum {  // stage R: entry e0 + er of iteration it, pixel row pr
    const int ring = it & 3;
    const float4 w0 = *reinterpret_cast<const float4*>(&sW[wave][er][8 * pr]);
    const float4 w1 = *reinterpret_cast<const float4*>(&sW[wave][er][8 * pr + 4]);
    const float4 q0 = *reinterpret_cast<const float4*>(&sQ[wave][er][8 * pr]);
    const float4 q1 = *reinterpret_cast<const float4*>(&sQ[wave][er][8 * pr + 4]);
    const float4 a = sGeo[ring][e0 + er], a2 = sGeo2[ring][e0 + er];
    const float wk[8] = {w0.x, w0.y, w0.z, w0.w, w1.x, w1.y, w1.z, w1.w};
    const float qk[8] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w};
    auto row8 = [&](int c, float (&o)[8]) {
      const float4 x = *reinterpret_cast<const float4*>(&sG[c][8 * pr]), y = *reinterpret_cast<const float4*>(&sG[c][8 * pr + 4]);
      o[0] = x.x; o[1] = x.y; o[2] = x.z; o[3] = x.w; o[4] = y.x; o[5] = y.y; o[6] = y.z; o[7] = y.w;
    };
    float rg0[8], rg1[8], rg2[8];
    row8(0, rg0); row8(1, rg1); row8(2, rg2);
    // Only the moments of q = G dL/dalpha are accumulated per pixel; opacity and conic enter after the reduction because
    // dL/dG = o dL/dalpha and dG/ddelx = ln2 (2 a2 gdx + b2 gdy), dG/ddely = ln2 (2 c2 gdy + b2 gdx) are linear in them.
    // (Two pixels per packed-fp32 instruction was tried here: 5 % fewer instructions, but the register pairs it needs push
    // the kernel past its 128 registers - the spills cost more than the packing saves.)
    float v6 = 0, v7 = 0, v8 = 0, v9 = 0;
    // moments of q along the row about the row's CENTRE (pixel 3.5), shifted to the splat centre afterwards:
    // sum q (dxc - j)^n, j = k - 3.5, for n = 1, 2 from S0, S1 = sum j q, S2 = sum j^2 q.  The weights pair up (j = -+3.5, -+2.5,
    // -+1.5, -+0.5), so the four pair sums feed S0 and S2 and the four pair differences S1: 19 instructions, as many as about the
    // row's first pixel (round 3) - but the terms that cancel in the shift are a quarter the size (|j| <= 3.5 instead of 7: for
    // the narrowest splats, whose centre lies inside the row, that is two more bits of the conic gradient)
    const float dxc = a.x - ((float)rpx0 + 3.5f), dy = a.y - (float)rpy;
    const float p07 = qk[0] + qk[7], p16 = qk[1] + qk[6], p25 = qk[2] + qk[5], p34 = qk[3] + qk[4];
    const float m70 = qk[7] - qk[0], m61 = qk[6] - qk[1], m52 = qk[5] - qk[2], m43 = qk[4] - qk[3];
    const float S0 = (p07 + p16) + (p25 + p34);
    const float S1 = __builtin_fmaf(m70, 3.5f, __builtin_fmaf(m61, 2.5f, __builtin_fmaf(m52, 1.5f, 0.5f * m43)));
    const float S2 = __builtin_fmaf(p07, 12.25f, __builtin_fmaf(p16, 6.25f, __builtin_fmaf(p25, 2.25f, 0.25f * p34)));
    float Sx = __builtin_fmaf(dxc, S0, -S1);               // sum q (dxc - j)
    float Sxx = __builtin_fmaf(dxc, Sx - S1, S2);          // sum q (dxc - j)^2 = dxc (dxc S0 - 2 S1) + S2
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      v6 = __builtin_fmaf(wk[k], rg0[k], v6);
      v7 = __builtin_fmaf(wk[k], rg1[k], v7);
      v8 = __builtin_fmaf(wk[k], rg2[k], v8);
    }
    if (kExtra) {  // the fourth channel in a pass of its own: its row of dL/dpixel is live only here (register budget)
      float rge[8];
      row8(3, rge);
#pragma unroll
      for (int k = 0; k < 8; ++k) v9 = __builtin_fmaf(wk[k], rge[k], v9);
    }
    const float Sy = dy * S0, Sxy = dy * Sx, Syy = dy * Sy;
    // The eight values a row receives from this entry are LINEAR in the sums, so every lane forms its share of all eight first -
    // conic (A,B,C) = (-2 ln2 a2, -ln2 b2, -2 ln2 c2):  dG/ddelx = -gdx A - gdy B,  dG/ddely = -gdy C - gdx B - and the eight
    // lanes of the entry then reduce-SCATTER them: three exchange steps in which a lane keeps the half of its values that its
    // own float index selects and hands the other half to its partner (i <-> 7 - i, i ^ 2, i ^ 1), 4 + 2 + 1 adds, and lane pr ends
    // with the complete value pr - instead of ten all-reduces (30 adds) followed by a selection of one of eight results.
    float F[8] = {__builtin_fmaf(a.w, Sy, (a.z + a.z) * Sx), __builtin_fmaf(a.w, Sx, (a2.x + a2.x) * Sy), Sxx, Sxy, Syy, S0, v6, v7};
    auto dpp_add = [](float keep, float send, auto ctrl_c) {
      return keep + __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(send), ctrl_c(), 0xf, 0xf, false));
    };
    const bool b2 = (pr & 4) != 0, b1 = (pr & 2) != 0, b0 = (pr & 1) != 0;
    float K[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) K[k] = dpp_add(b2 ? F[k + 4] : F[k], b2 ? F[k] : F[k + 4], [] { return 0x141; });  // row_half_mirror
    float L[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) L[k] = dpp_add(b1 ? K[k + 2] : K[k], b1 ? K[k] : K[k + 2], [] { return 0x4E; });   // quad_perm [2,3,0,1]
    float val = dpp_add(b0 ? L[1] : L[0], b0 ? L[0] : L[1], [] { return 0xB1; });                                   // quad_perm [1,0,3,2]
    val *= pr < 5 ? a2.y * cpr : 1.f;  // opacity and the constant of the float: hW ln2, hH ln2, -1/2, -1/2, -1/2 | 1, 1, 1
    v8 = oct_allreduce(v8);
    if (kExtra) v9 = oct_allreduce(v9);
    RowSum r;
    r.val = val; r.tail = pr == 0 ? v8 : v9;
    r.id = !GSR_ABL(p.d.flags, GSR_FLAG_ABLATE_BWD_NO_ATOMIC) ? __float_as_uint(a2.z) : 0xffffffffu;
    return r;
  };
  // The segment's sums into the accumulator rows of their splats.  Device-scope atomics are executed on the memory side of the
  // fabric (the L2s of the XCDs are not coherent with each other: TCC_EA0_ATOMIC = TCC_ATOMIC), one transaction per REQUEST the
  // lanes of an instruction coalesce into - and at 15 requests per wave and batch (floats 0-7 of eight rows, then floats 8 (9)
  // of the same rows from eight lanes of a second instruction) the launch ran at the rate of those transactions: 42.9 us, 33.8
  // without the second instruction, 34.3 with both on rows nobody else touches.  Now a row's 9 (10) values leave together:
  // the lanes of a DPP row are two entries' groups of eight; the first instruction carries the even entries - floats 0-7 from
  // their own lanes, floats 8 (9) from the first lanes of the odd neighbour's group, which fetch value and row id across the
  // row (row_ror:8) - the second instruction the odd entries the same way: 9-10 adjacent lanes, 36-40 contiguous bytes, one
  // request (two where the 48-byte row straddles a 64-byte line; 64-byte rows measured the same, the launch is no longer bound
  // by the transactions).  TCC_ATOMIC per launch 601 k -> 267-400 k, k_blend_bwd 42.9 -> 34.6 us.
  auto ror8 = [](uint32_t x) { return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x128, 0xf, 0xf, false); };
  auto scatter = [&](const RowSum& r) {
    const uint32_t o_id = ror8(r.id);
    const float o_tail = __uint_as_float(ror8(__float_as_uint(r.tail)));
    const bool odd = (er & 1) != 0, tail_lane = pr < (kExtra ? 2 : 1);
#pragma unroll
    for (int pass = 0; pass < 2; ++pass) {  // pass 0: even entries, pass 1: odd entries
      const bool own = odd == (pass == 1);
      const uint32_t id = own ? r.id : o_id;
      const float x = own ? r.val : o_tail;
      const int slot = own ? pr : 8 + pr;
      // (a lane whose value is an exact zero - a splat that no pixel of the tile blended, or whose pixels carry no gradient - adds nothing)
      if (id != 0xffffffffu && (own || tail_lane) && x != 0.f) {
        if (kDet) {
          unsigned long long* dst = reinterpret_cast<unsigned long long*>(p.scratch) +
                                    ((size_t)v * p.d.num_gaussians + id) * GSR_SCREEN_GRAD_FLOATS;
          atomicAdd(dst + slot, to_fixed(x));
        } else {
          unsafeAtomicAdd(scratch + (size_t)id * GSR_SCREEN_GRAD_FLOATS + slot, x);
        }
      }
    }
  };

  // ---- prologue: waves 0 / 1 stage and park batches 0 / 1, wave 2 requests batch 2 (parked in iteration 0), wave 3 fetches the
  // list ids of batch 3; everyone evaluates batch 0.
  // Gather pipeline of the loop, iteration `it`: wave (it+3)&3 requests the records of batch it+3 (ids in hand since it-1), wave
  // it&3 requests the list ids of batch it+4, wave (it+2)&3 parks the records it requested in iteration it-1 - more than one
  // whole iteration after the request, and BEFORE this iteration's atomics (a wave's memory counter is in order: behind its
  // atomics it would wait until the fabric has acknowledged them).
  float4 sg = make_float4(0, 0, 0, 0), sg2 = sg, sc = sg;
  uint32_t id_next = 0;
  if (wave == 0 || (wave == 1 && nbat > 1)) {
    const uint32_t it0 = (uint32_t)wave;
    const uint32_t id0 = load_ids(it0);
    stage(it0, sg, sg2, sc, id0);
    park((int)it0, sg, sg2, sc, id0);
  } else if (wave == 2) {
    id_next = load_ids(2);
    if (2 < nbat) stage(2, sg, sg2, sc, id_next);
  } else {
    id_next = load_ids(3);
  }
  __syncthreads();
  eval(0);
  __syncthreads();
  const float T_final = inside ? p.final_T[(size_t)v * HW + pix] : 0.f;
  float Tb = T_final;                                              // (T, Q) at the back end of the batch: the same in all four
  float Qb = cam.bg[0] * g0 + cam.bg[1] * g1 + cam.bg[2] * g2;    // waves (behind the last splat Q = Bg / T_final = bg.g)
  if (kAlpha) {
    Qb -= inside ? (kDet ? up * p.dL_dalpha_img[(size_t)v * HW + pix] : p.dL_dalpha_img[(size_t)v * HW + pix]) : 0.f;
    asm volatile("" : "+v"(Qb));  // (arrived before the loop, like T_final below)
  }
  if (dbg) stamp[1] = __builtin_amdgcn_s_memrealtime();
  // T_final has to have ARRIVED before the loop: a load still counted as pending at the loop's entry makes the compiler wait
  // for "everything" at the first use of Tb inside the loop - on every iteration, right behind the gather just issued
  asm volatile("" : "+v"(Tb));
  for (uint32_t it = 0; it < nbat; ++it) {
    if (wave == (int)((it + 3) & 3) && it + 3 < nbat) stage(it + 3, sg, sg2, sc, id_next);  // global gather in flight
    if (wave == (int)(it & 3)) id_next = load_ids(it + 4);
    // back to front: wave 3's segment is the deepest.  The same chain in every wave: (t, q) = transmittance and Q at the BACK end
    // of segment k; the front of segment k is the back of segment k - 1.  One segment's three values at a time (register budget).
    float t = Tb, q = Qb, Tf = 0.f, Qk = 0.f;
#pragma unroll
    for (int k = kBwdWaves - 1; k >= 0; --k) {
      const float Rk = sR[it & 1][k][lane], Pk = sP[it & 1][k][lane], Bk = sB[it & 1][k][lane];
      Qk = wave == k ? q : Qk;
      t *= Rk;
      Tf = wave == k ? t : Tf;
      q = __builtin_fmaf(Pk, q, Bk);
      asm volatile("" ::: "memory");
    }
    Tb = t; Qb = q;
    replay(Tf, Qk);
    RowSum rs = reduce(it);
    // the sums are FINISHED here, in the reduction's own basic block: left to itself the compiler sinks the last step of the
    // DPP all-reduce below the branch that follows, where a cross-lane move can no longer be folded into its add (+18 VALU)
    asm volatile("" : "+v"(rs.val), "+v"(rs.tail), "+v"(rs.id));
    // every wave: nothing of its own is in flight past this point except the atomics that follow (an explicit wait the compiler
    // sees: without it, it has to assume at the top of the loop that a request of an earlier iteration may still be pending on
    // the registers the next one writes, and waits there for the previous iteration's ATOMICS)
    __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0)
    if (wave == (int)((it + 2) & 3) && it + 2 < nbat) park((int)((it + 2) & 3), sg, sg2, sc, id_next);
    asm volatile("" ::: "memory");
    scatter(rs);
    if (it + 1 < nbat) eval(it + 1);
    __syncthreads();
  }
  if (dbg) {
    const unsigned hw = (__builtin_amdgcn_s_getreg(4 | (0 << 6) | (15 << 11)) & 0xffffu) |
                        ((__builtin_amdgcn_s_getreg(20 | (0 << 6) | (15 << 11)) & 0xfu) << 16);
    stamp[2] = __builtin_amdgcn_s_memrealtime();
    stamp[3] = ((unsigned long long)hw << 32) | ((unsigned long long)nbat << 16) | (unsigned)t;
  }
}

// ------------------------------------------------------------------------------------------------
// B2: backward preprocess — conic -> cov2D -> cov3D/mean, projection, SH ([EXT] backward.cu
// computeCov2DCUDA + preprocessCUDA; oracle preprocess_backward).  One wavefront per 64 Gaussians of a SET;
// loops over the set's views so SH is read once and every gradient is written once.
// ------------------------------------------------------------------------------------------------
constexpr int kPoseFloats = 35;  // dL/d viewmatrix (16), projmatrix (16), campos (3) of a view
// kJ: the forward saved d rgb / d direction of every (view, Gaussian) (Params::shj, GSR_FLAG_BACKWARD_FOLLOWS): the harmonics
// themselves are then not read here at all - 300 B per Gaussian less of the kernel's ~750.
// kPose: 0 no camera gradient; 1 all of it (35 floats per view); 2 only what the built-in depth channel contributes - the four
// entries 2, 6, 10, 14 of the view matrix that form z: the ONE camera gradient the reference's own graph carries (its depth render
// reads extrinsics.inverse() in torch, cuda_splatting.py:239-242; nothing reaches a camera through the rasterizer);
// 3 all of it and the two tan-fov columns (below)
// kShFrame: GSR_FLAG_SH_IN_FRAME - dL/dsh is evaluated at the direction carried into the Gaussian's frame, and the direction
// gradient of the recomputing form goes back to world coordinates before the chain into dL/dmeans and dL/dcampos (the saved
// Jacobian of the kJ form is in world coordinates already: color_eval_lane).  The flag-off instances are the code as it was.
constexpr int kPoseZFloats = 4;
// kPose == 3 (GSR_FLAG_FOV_GRADIENT): everything kPose == 1 does, and dL/dtanfovx, dL/dtanfovy behind the 35 - what the EWA Jacobian
// reads of the two fields (fx, fy and the 1.3 tanfov clamp limit); rows of 37 floats, summed by k_pose_reduce<37>.
constexpr int kPoseFovFloats = kPoseFloats + 2;
// The kernel's text is csrc/preprocess_bwd.inc, compiled twice: k_preprocess_bwd, and k_preprocess_bwd_det for GSR_FLAG_DETERMINISTIC.
#define GSR_PBWD_KERNEL k_preprocess_bwd
#define GSR_PBWD_UNIT 0
#include "preprocess_bwd.inc"
#undef GSR_PBWD_KERNEL
#undef GSR_PBWD_UNIT
#define GSR_PBWD_KERNEL k_preprocess_bwd_det
#define GSR_PBWD_UNIT 1
#include "preprocess_bwd.inc"
#undef GSR_PBWD_KERNEL
#undef GSR_PBWD_UNIT

// Sum of camera-gradient rows, two levels, fixed order (deterministic).  Block (v, b) adds rows [b * per, (b + 1) * per) of view
// v: with kCols = 35, 245 threads = 7 rows x 35 columns per step, so a step reads 980 consecutive bytes; with kCols = 37 (the rows
// with the tan-fov columns) 222 threads = 6 rows x 37.  Level 1: the rows k_preprocess_bwd wrote -> kPoseBlocks rows per view;
// level 2 (one block per view): those -> the (V, 48) output record (zeros behind [kCols]).
constexpr int kPoseBlocks = 256;
template <int kCols>
__global__ __launch_bounds__(256) void k_pose_reduce(const float* in, int rows, float* out, int out_stride, int out_rows) {
  constexpr int kRows = 256 / kCols;  // rows a step covers
  __shared__ float part[kRows][kCols];
  const int v = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  const int per = (rows + (int)gridDim.y - 1) / (int)gridDim.y;
  const int r_begin = b * per, r_end = min(rows, r_begin + per);
  const int k = tid % kCols, r0 = tid / kCols;
  const float* base = in + (size_t)v * rows * kCols;
  float acc = 0.f;
  if (r0 < kRows) {
    int r = r_begin + r0;
    for (; r + 3 * kRows < r_end; r += 4 * kRows) {  // four independent loads in flight, added in a fixed order
      const float a0 = base[(size_t)r * kCols + k], a1 = base[(size_t)(r + kRows) * kCols + k];
      const float a2 = base[(size_t)(r + 2 * kRows) * kCols + k], a3 = base[(size_t)(r + 3 * kRows) * kCols + k];
      acc += a0; acc += a1; acc += a2; acc += a3;
    }
    for (; r < r_end; r += kRows) acc += base[(size_t)r * kCols + k];
    part[r0][k] = acc;
  }
  __syncthreads();
  float* dst = out + ((size_t)v * out_rows + b) * out_stride;
  if (tid < out_stride) {
    float sum = 0.f;
    if (tid < kCols)
      for (int j = 0; j < kRows; ++j) sum += part[j][tid];
    dst[tid] = sum;
  }
}

// The same for the four-float rows of the depth-only camera gradient (kPose == 2): 256 threads = 64 rows x 4 columns per step.
// `final`: write the (V, 48) record - the sums at floats 2, 6, 10, 14 (the z row of the transposed view matrix), zeros elsewhere.
__global__ __launch_bounds__(256) void k_pose_reduce_z(const float* in, int rows, float* out, int final) {
  __shared__ float part[64][kPoseZFloats];
  const int v = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  const int per = (rows + (int)gridDim.y - 1) / (int)gridDim.y;
  const int r_begin = b * per, r_end = min(rows, r_begin + per);
  const int k = tid & 3, r0 = tid >> 2;
  const float* base = in + (size_t)v * rows * kPoseZFloats;
  float acc = 0.f;
  for (int r = r_begin + r0; r < r_end; r += 64) acc += base[(size_t)r * kPoseZFloats + k];
  part[r0][k] = acc;
  __syncthreads();
  if (tid < kPoseZFloats) {
    float sum = 0.f;
    for (int j = 0; j < 64; ++j) sum += part[j][tid];  // fixed order: deterministic
    part[0][tid] = sum;
  }
  __syncthreads();
  if (final) {
    if (tid < 48) out[(size_t)v * 48 + tid] = ((tid & 3) == 2 && tid < 16) ? part[0][tid >> 2] : 0.f;
  } else if (tid < kPoseZFloats) {
    out[((size_t)v * gridDim.y + b) * kPoseZFloats + tid] = part[0][tid];
  }
}

}  // namespace gsr
