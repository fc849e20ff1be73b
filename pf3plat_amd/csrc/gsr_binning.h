#pragma once
// K1 (projection, binning, colour pass) and the windowed binning chain.
#include "gsr_common.h"

namespace gsr {

// ------------------------------------------------------------------------------------------------
// K1: preprocess ([EXT] forward.cu preprocessCUDA; oracle preprocess()), split in two parts that have nothing in common
// but the means:
//   geometry (k_preprocess / k_preprocess_bin, feeds the binning chain): projection, EWA covariance, conic, radius,
//       reference rect and the 64-bit 8x8-tile hit mask - 40 B in, 64 B out per (view, Gaussian), VALU-bound;
//   colour (k_color / color_unit, further down: the first launch of the chain): SH -> RGB (+0.5, clamp mask) for every view
//       of a set - 300 of the 352 input bytes per Gaussian, HBM-bound.
// ------------------------------------------------------------------------------------------------
constexpr int kPreThreads = 256;

// Everything preprocess does for Gaussian i of view v; `hit(tile)` is called once per (8x8 tile, splat) pair it lists.
// Footprints wider than the 8x8-tile mask window are handed to `big(i, foot)` (the caller walks them).
// The inputs of one Gaussian as they sit in memory (the binning launch asks for the next iteration's before it works on this one's)
struct GaussIn {
  float m[3], cov6[6], op;
};
__device__ __forceinline__ GaussIn load_gauss(const Params& p, int v, int i) {
  const int set = v / p.d.views_per_set;
  const size_t gi = (size_t)set * p.d.num_gaussians + i;
  GaussIn in;
  in.m[0] = p.means[3 * gi + 0]; in.m[1] = p.means[3 * gi + 1]; in.m[2] = p.means[3 * gi + 2];
  load_covariance(p, set, i, gi, in.cov6);
  in.op = p.opac[gi];
  return in;
}
template <class F, class B>
__device__ __forceinline__ PreRec preprocess_one(const Params& p, int v, int i, const GaussIn& in, F&& hit, B&& big) {
  const int N = p.d.num_gaussians;
  // (per-lane loads of the uniform record: held in scalar registers - view_const, as k_preprocess_bwd does - the ~30 registers spill in
  // the binning kernels, forward +0.6 us)
  const GsrView& cam = p.views[v];
  const Grid& g = p.g;
  const size_t oi = (size_t)v * N + i;

  const float mx = in.m[0] * cam.scale, my = in.m[1] * cam.scale, mz = in.m[2] * cam.scale;
  float cov6[6];
#pragma unroll
  for (int k = 0; k < 6; ++k) cov6[k] = in.cov6[k] * cam.scale2;
  const float op = in.op;
  const float* vm = cam.viewmatrix;
  const float* pm = cam.projmatrix;
  const float pvz = vm[2] * mx + vm[6] * my + vm[10] * mz + vm[14];
  bool vis = !(pvz <= kNear);
  const float ph0 = pm[0] * mx + pm[4] * my + pm[8] * mz + pm[12];
  const float ph1 = pm[1] * mx + pm[5] * my + pm[9] * mz + pm[13];
  const float ph3 = pm[3] * mx + pm[7] * my + pm[11] * mz + pm[15];
  const float p_w = 1.0f / (ph3 + 0.0000001f);
  const float ppx = ph0 * p_w, ppy = ph1 * p_w;
  Cov2D c2;
  cov2d_parts(mx, my, mz, cov6, cam, g.W, g.H, c2);
  const float det = c2.a * c2.c - c2.b * c2.b;
  vis = vis && !(det == 0.f);
  const float det_inv = 1.f / det;
  const float conA = c2.c * det_inv, conB = -c2.b * det_inv, conC = c2.a * det_inv;
  const float mid = 0.5f * (c2.a + c2.c);
  const float root = sqrtf(fmaxf(0.1f, mid * mid - det));
  const float lambda1 = mid + root, lambda2 = mid - root;
  const float my_radius = ceilf(3.f * sqrtf(fmaxf(lambda1, lambda2)));
  const float px = ((ppx + 1.0f) * (float)g.W - 1.0f) * 0.5f;
  const float py = ((ppy + 1.0f) * (float)g.H - 1.0f) * 0.5f;
  vis = vis && (fabsf(px) < 3.0e38f) && (fabsf(py) < 3.0e38f) && (my_radius < 16777216.f) && (pvz < 3.0e38f);
  if (vis) {
    int rx0, ry0, rx1, ry1;
    ref_rect16(px, py, my_radius, g, rx0, ry0, rx1, ry1);
    vis = (rx1 - rx0) * (ry1 - ry0) != 0;
  }
  const int radius = vis ? (int)my_radius : 0;
  p.radii[oi] = radius;
  PreRec rec;
  const int emode = (p.d.flags >> 4) & 7;
  float ex = 0.f;
  if (vis && p.d.has_extra) {
    float dfdz;
    ex = emode == 0 ? p.extra[oi] : extra_from_depth(emode, pvz / cam.scale, cam.reserved[0], cam.reserved[1], dfdz);
  }
  rec.q0 = vis ? make_float4(px, py, conA, conB) : make_float4(0, 0, 0, 0);
  rec.q1 = vis ? make_float4(conC, op, ex, __uint_as_float((uint32_t)radius)) : make_float4(0, 0, 0, 0);
  unsigned long long mask = 0ull;
  uint32_t origin = 0u;
  if (vis && !GSR_ABL(p.d.flags, GSR_FLAG_ABLATE_NO_COUNT)) {
    const Foot f = make_foot(px, py, conA, conB, conC, op, my_radius, g);
    if (f.sx1 > f.sx0 && f.sy1 > f.sy0) {
      origin = (uint32_t)f.sx0 | ((uint32_t)f.sy0 << 12);
      if (f.sx1 - f.sx0 <= 8 && f.sy1 - f.sy0 <= 8) {
        for (int sy = f.sy0; sy < f.sy1; ++sy) mask |= (unsigned long long)row_hit_bits(f, sy, g) << ((sy - f.sy0) * 8);
        unsigned long long m = mask;
        while (m) {
          const int b = __ffsll((long long)m) - 1;
          m &= m - 1;
          hit((f.sy0 + (b >> 3)) * g.sgx + f.sx0 + (b & 7));
        }
      } else {
        origin |= 0x80000000u;
        big(i, f, pvz);
      }
    }
  }
  rec.q3 = make_float4(__uint_as_float((uint32_t)mask), __uint_as_float((uint32_t)(mask >> 32)), __uint_as_float(origin),
                       vis ? pvz : 0.f);
  return rec;
}

// The wave's 64 records are 2 KB of consecutive memory.  Written lane by lane they are 16-byte requests at a 32-byte
// stride - half of what the CU's store path carries per request, and the record store was the longest part of preprocess
// when it was done that way.  Through a per-wave LDS transpose (2 KB; 2-way conflicts on the write, none on the read) every
// store instruction covers 1 KB of consecutive bytes instead.  `valid` = records of this wave that exist.
__device__ __forceinline__ void store_records_wave(GeomRec* dst, int valid, const PreRec& rec, float4* lds, int lane) {
  lds[lane * 2 + 0] = rec.q0;
  lds[lane * 2 + 1] = rec.q1;
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  float4* out = reinterpret_cast<float4*>(dst);
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const int c = k * 64 + lane;
    const float4 x = lds[c];
    if ((c >> 1) < valid) out[c] = x;
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// The same through a 1 KB stage (thirty-two records at a time): k_preprocess_bin<true, .> keeps its LDS for the colour waves' unit buffers.
__device__ __forceinline__ void store_records_wave_1k(GeomRec* dst, int valid, const PreRec& rec, float4* lds, int lane) {
  const int l = lane & 31;
  float4* out = reinterpret_cast<float4*>(dst);
#pragma unroll
  for (int pass = 0; pass < 2; ++pass) {
    if ((lane >> 5) == pass) {
      lds[l * 2 + 0] = rec.q0;
      lds[l * 2 + 1] = rec.q1;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    const float4 x = lds[lane];  // record (lane >> 1) of this pass
    if (pass * 32 + (lane >> 1) < valid) out[pass * 64 + lane] = x;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
  }
}

// GSR_FLAG_BACKWARD_FOLLOWS: the backward's accumulator rows of a wave's (up to) 64 Gaussians of view v start at zero.  Done by
// the geometry kernels - VALU-bound, their memory pipes idle - rather than by the colour pass, which lives on memory bandwidth.
__device__ __forceinline__ void zero_rows_wave(const Params& p, int v, int first, int valid, int lane) {
  const int row4 = (p.d.flags & GSR_FLAG_DETERMINISTIC) ? 2 * GSR_SCREEN_GRAD_FLOATS / 4 : GSR_SCREEN_GRAD_FLOATS / 4;
  float4* rows = p.grad_rows + ((size_t)v * p.d.num_gaussians + first) * row4;
  const int n4 = min(valid, 64) * row4;
  for (int k = lane; k < n4; k += 64) rows[k] = make_float4(0.f, 0.f, 0.f, 0.f);
}

__global__ __launch_bounds__(kPreThreads) void k_preprocess(const Params p) {
  __shared__ float4 stage[kPreThreads / 64][128];
  const int i = blockIdx.x * kPreThreads + threadIdx.x, N = p.d.num_gaussians, v = blockIdx.y;
  const int lane = threadIdx.x & 63, first = i - lane;
  if (first >= N) return;
  PreRec rec{};
  if (i < N) rec = preprocess_one(p, v, i, load_gauss(p, v, i), [](int) {}, [](int, const Foot&, float) {});
  if (!GSR_ABL(p.d.flags, GSR_FLAG_ABLATE_NO_GEOM_STORE)) {
    store_records_wave(p.geom + (size_t)v * N + first, N - first, rec, stage[threadIdx.x >> 6], lane);
    if (i < N && p.aux) p.aux[(size_t)v * N + i] = rec.q3;  // 1 KB of consecutive bytes per wave as it is
  }
  if (p.grad_rows) zero_rows_wave(p, v, first, N - first, lane);
}

// Preprocess and count in one launch (images of up to kTileWindow 8x8 tiles): the workgroup owns the `chunk` Gaussians of
// one row of the count matrix, histograms their pairs in LDS while it projects them and stores the row at the end -
// k_count's result without a second pass over the records and without its launch.
// Pages of the key pool come from bump counters in the status block: one for the binning launch (lower half of the pool: regions
// of workgroups that list more than their fixed slot holds), one for the tile launch (upper half: scratch of lists too long for
// the LDS sort).  A counter carries the tag of the call that last touched it in its upper half: a value left by any other call
// (or never initialised) counts as zero, so the workspace needs no zeroing.  A replay of the very same call (HIP graph: same
// tag) must find both at zero again: each counter is put back by the OTHER launch of the chain - the binning launch resets
// the tile launch's at its start, the tile launch the binning's - so no reset ever runs beside a taker of the same counter.
// Only the rare workgroup that outgrows its fixed slot / the rare list longer than the LDS sort comes here.
__device__ __forceinline__ uint32_t take_pages(unsigned long long* counter, uint32_t call_tag, uint32_t n) {
  const unsigned long long tag = (unsigned long long)call_tag << 32;
  // Once the counter carries this call's tag it keeps it until the launch is over (the reset is the OTHER launch's): from then on a
  // taker is ONE fetch-add.  Only the takers that still see a foreign tag compete with compare-and-swap - one of them installs the
  // tag, the others see it in what their failed attempt returns.  (Round 5 looped on compare-and-swap throughout: on the pixel-aligned
  // scene a third of the 246 binning workgroups of a configs[3] call outgrow their slot within the same microsecond, every failed
  // attempt is a round trip to the memory side of the fabric, and the workgroups spent 28-38 us here - profiles/r06_a_stamps_*.)
  unsigned long long cur = __hip_atomic_load(counter, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  while (true) {
    if ((cur >> 32) == (tag >> 32)) return (uint32_t)atomicAdd(counter, (unsigned long long)n);
    const unsigned long long seen = atomicCAS(counter, cur, tag + n);
    if (seen == cur) return 0u;
    cur = seen;
  }
}

// Measurement aid: eight 64-bit stamps per slot at the very end of the key buffer (pages handed out last, so unused in
// any run that does not overflow).
__device__ __forceinline__ unsigned long long* dbg_stamps(const Params& p, size_t slot) {
  return p.keys + (size_t)p.pool_off + (size_t)p.key_pages * kPage - (slot + 1) * 8;  // (the padding lies behind)
}
// (in a kernel that has `dbg`, `tid` and its slot `stamp` / a second slot `stamp2`)
#define GSR_STAMP(k) do { if (dbg && tid == 0) stamp[k] = __builtin_amdgcn_s_memrealtime(); } while (0)
#define GSR_STAMP2(k) do { if (dbg && tid == 0) stamp2[k] = __builtin_amdgcn_s_memrealtime(); } while (0)

__device__ __forceinline__ Foot foot_from_lds(const float* b, const Grid& g) {
  Foot f;
  f.cx = b[0]; f.cy = b[1]; f.A = b[2]; f.B = b[3]; f.C = b[4]; f.tau = b[5];
  f.nBiC = -f.B * __builtin_amdgcn_rcpf(f.C); f.nBiA = -f.B * __builtin_amdgcn_rcpf(f.A);
  const int xs = __float_as_int(b[6]), ys = __float_as_int(b[7]);
  f.sx0 = xs & 0xffff; f.sx1 = xs >> 16; f.sy0 = ys & 0xffff; f.sy1 = ys >> 16;
  const float detc = f.A * f.C - f.B * f.B;
  f.convex = (f.A > 0.f) && (f.C > 0.f) && (detc > 0.f) && (detc < 3.0e38f);
  f.detc = detc; f.hx = 0.f; f.hy = 0.f;
  return f;
}

// Colour role: SH -> RGB (+0.5, clamp mask) of one 64-Gaussian unit for every view of its set, by a group of kColorThreads
// threads.  All of them request the unit's 64 x 3M SH floats (19 200 B at M = 25) as 16-byte coalesced loads, park them in
// LDS (row stride 3M floats, odd => conflict-free) and wave w evaluates views w, w + 4, ... with lane = Gaussian (the SH of a
// set is read ONCE however many views it has).  The colour pass is HBM-bound (300 of the 352 input bytes per Gaussian): a
// launch of its own (k_color), eight workgroups per CU, ~4.6 TB/s.  (Measured alternatives, all slower: colour workgroups
// beside or behind the per-tile sorts in one launch - the sorts' scattered gathers and the stream only lose to each other,
// whatever the order; beside the binning workgroups - with 19 KB of LDS per unit in flight a CU holds too few units to
// cover their latency once their waves share SIMDs with VALU-bound ones; a second stream - 6 us per event.)
constexpr int kColorThreads = 256;
constexpr int kShPre = 5;  // float4 registers per thread that hold the unit's SH rows (64 * 75 / 4 / 256 = 4.7)
constexpr int kColorLdsFloats = 64 * 75;  // a full unit at M = 25 (row stride 75: odd)

// Colour (+0.5, clamp mask; kJ: d rgb / d direction as well) of Gaussian i of `set` - this lane - for the views vbegin,
// vbegin + vstep, ... of the set, from its SH row `sh` (LDS).  Same expression tree as the oracle: rgb bit-exact.
// kFull: the active degree is 4 and all 25 coefficients are in memory (PF3plat's and the benchmark's case), known at compile time -
// the band tests and the `k < M` tests fold away, the 75 LDS reads of a row sit in ONE basic block (the compiler can then request
// them ahead of the arithmetic instead of three at a time between branches) - same expression tree, same bits.
// The camera of a view is wave-uniform: its scale and centre are fetched with scalar loads (readfirstlane on the view index), not
// with a per-lane global load that every unit's evaluation then waits a full memory round trip for, under the colour stream.
// kShFrame (GSR_FLAG_SH_IN_FRAME): the harmonics are in the Gaussian's frame - evaluated at the direction carried into it
// (load_dir_frame); the saved Jacobian (kJ) is carried back to world coordinates here, so the backward's direction chain reads it
// as it reads the plain one.  The flag-off instances are the code as it was.
template <bool kJ, bool kFull, bool kShFrame>
__device__ __forceinline__ void color_eval_lane(const Params& p, int set, int i, const float* sh, int vbegin, int vstep, int vend,
                                                float rmx, float rmy, float rmz, const CamLite& cam0) {
  const int N = p.d.num_gaussians, Vs = p.d.views_per_set, M = kFull ? 25 : p.d.sh_coeffs;
  const int deg = kFull ? 4 : min(p.d.sh_degree, p.d.max_sh_eval);
  float T[9];
  if (kShFrame) load_dir_frame(p, set, i, T);
  // coefficient k of channel c sits at k * ks + c * cs: (3, 1) for (N, M, 3), (1, M) for the planar (N, 3, M) layout.  The
  // common layouts get compile-time strides (one base register + immediate offsets); computed per coefficient at run time
  // the 75 LDS addresses occupied 75 registers.
  auto eval_views = [&](auto ks_c, auto cs_c) {
    const int ks = ks_c(), cs = cs_c();
    for (int vv = vbegin; vv < vend; vv += vstep) {
      const int v = __builtin_amdgcn_readfirstlane(set * Vs + vv);
      CamLite cam = cam0;
      if (vv != vbegin) cam = cam_lite(p.views, v);
      const float mx = rmx * cam.scale, my = rmy * cam.scale, mz = rmz * cam.scale;
      float dx = mx - cam.cx, dy = my - cam.cy, dz = mz - cam.cz;
      const float len = sqrtf(dx * dx + dy * dy + dz * dz);
      dx = dx / len; dy = dy / len; dz = dz / len;
      if (kShFrame) dir_to_frame(T, dx, dy, dz);
      float cr = 0, cg = 0, cb = 0;
      float jx[3] = {0, 0, 0}, jy[3] = {0, 0, 0}, jz[3] = {0, 0, 0};
      if (kJ) {  // a backward follows: d rgb / d direction as well, from the coefficients that are in LDS right now
        sh_visit(deg, dx, dy, dz, [&](int k, float bk, float bx, float by, float bz) {
          if (kFull || k < M) {
            // (compile-time instance: a scheduling fence in front of every band keeps the compiler from requesting all 75
            // coefficients at once - with the twelve accumulators of this variant that spilled)
            if (kFull && (k == 1 || k == 4 || k == 9 || k == 16 || k == 20)) __builtin_amdgcn_sched_barrier(0);
            const float s0 = sh[k * ks + 0 * cs], s1 = sh[k * ks + 1 * cs], s2 = sh[k * ks + 2 * cs];
            cr += bk * s0; cg += bk * s1; cb += bk * s2;
            jx[0] += bx * s0; jx[1] += bx * s1; jx[2] += bx * s2;
            jy[0] += by * s0; jy[1] += by * s1; jy[2] += by * s2;
            jz[0] += bz * s0; jz[1] += bz * s1; jz[2] += bz * s2;
          }
        });
      } else {
        sh_visit(deg, dx, dy, dz, [&](int k, float bk, float, float, float) {
          if (kFull || k < M) {
            cr += bk * sh[k * ks + 0 * cs]; cg += bk * sh[k * ks + 1 * cs]; cb += bk * sh[k * ks + 2 * cs];
          }
        });
      }
      cr += 0.5f; cg += 0.5f; cb += 0.5f;
      const uint32_t clampbits = (cr < 0.f ? 1u : 0u) | (cg < 0.f ? 2u : 0u) | (cb < 0.f ? 4u : 0u);
      if (kJ) {  // rows x, y, z of the Jacobian; the clamp mask rides in the spare slot (the backward then needs nothing else from here)
        if (kShFrame)
#pragma unroll
          for (int c = 0; c < 3; ++c) grad_to_world(T, jx[c], jy[c], jz[c]);
        float4* o = p.shj + ((size_t)v * N + i) * 3;
        o[0] = make_float4(jx[0], jx[1], jx[2], __uint_as_float(clampbits));
        o[1] = make_float4(jy[0], jy[1], jy[2], 0.f); o[2] = make_float4(jz[0], jz[1], jz[2], 0.f);
      }
      p.rgbc[(size_t)v * N + i] = make_float4(fmaxf(cr, 0.f), fmaxf(cg, 0.f), fmaxf(cb, 0.f), __uint_as_float(clampbits));
    }
  };
  const bool planar = (p.d.flags & GSR_FLAG_SH_PLANAR) != 0;
  if (!planar) eval_views([] { return 3; }, [] { return 1; });
  else if (kFull || M == 25) eval_views([] { return 1; }, [] { return 25; });
  else eval_views([] { return 1; }, [&] { return M; });
}
// wave-uniform choice of the instance.  kAllowFull: only the colour waves of the binning launch in inference take the compile-time
// instance - with its loads hoisted it needs ~40 registers more, which the Jacobian variant (twelve accumulators) and the
// stand-alone k_color (eight workgroups per CU) do not have; nor does the frame's direction transform (kShFrame: 28 bytes of
// scratch per lane with it).
template <bool kJ, bool kAllowFull, bool kShFrame>
__device__ __forceinline__ void color_eval(const Params& p, int set, int i, const float* sh, int vbegin, int vstep, int vend,
                                           float rmx, float rmy, float rmz, const CamLite& cam0) {
  if (kAllowFull && !kShFrame && p.d.sh_coeffs == 25 && min(p.d.sh_degree, p.d.max_sh_eval) == 4) color_eval_lane<kJ, true, kShFrame>(p, set, i, sh, vbegin, vstep, vend, rmx, rmy, rmz, cam0);
  else color_eval_lane<kJ, false, kShFrame>(p, set, i, sh, vbegin, vstep, vend, rmx, rmy, rmz, cam0);
}

// `tid` = thread within the group (0 .. kColorThreads - 1), `lds` = the group's 19 200 B; the one barrier inside is the
// workgroup's, so every group of a workgroup must come here together - a group without a unit passes valid = false.
template <bool kJ, bool kShFrame>
__device__ __forceinline__ void color_unit(const Params& p, uint32_t cu, bool valid, float* lds, int tid) {
  const unsigned long long t_start = __builtin_amdgcn_s_memrealtime();
  const int lane = tid & 63, wave = tid >> 6;
  // Few waves, little arithmetic, but every cycle a unit waits keeps 19 KB of LDS from the next one: issue ahead of the
  // VALU-bound waves this workgroup shares its SIMDs with
  __builtin_amdgcn_s_setprio(3);
  if (!valid) cu = 0;
  const int set = (int)(cu / p.color_units), unit = (int)(cu - (uint32_t)set * p.color_units);
  const int N = p.d.num_gaussians, Vs = p.d.views_per_set;
  const int g0 = unit * 64;
  const int i = g0 + lane;
  const bool in_range = i < N;
  const size_t gi = (size_t)set * N + (in_range ? i : 0);
  const int M = p.d.sh_coeffs;
  if (M == 0) {  // precomputed colours: copy through (no clamp)
    if (in_range && wave == 0 && valid)
      for (int vv = 0; vv < Vs; ++vv)
        p.rgbc[(size_t)(set * Vs + vv) * N + i] = make_float4(p.colors[3 * gi], p.colors[3 * gi + 1], p.colors[3 * gi + 2], 0.f);
    return;
  }
  const int rowf = 3 * M, ldstride = rowf | 1;
  const int cnt = min(64, N - g0);
  const float* sh_src = p.colors + ((size_t)set * N + g0) * rowf;
  const int sh_total = cnt * rowf, sh_n4 = sh_total >> 2;
  const bool sh_fast = (ldstride == rowf) && ((((uintptr_t)sh_src) & 15) == 0);
  if (!valid) {
  } else if (sh_fast) {
    float4 pre[kShPre];
#pragma unroll
    for (int q = 0; q < kShPre; ++q) {
      const int k = tid + kColorThreads * q;
      pre[q] = (k < sh_n4) ? reinterpret_cast<const float4*>(sh_src)[k] : make_float4(0, 0, 0, 0);
    }
#pragma unroll
    for (int q = 0; q < kShPre; ++q) {
      const int k = tid + kColorThreads * q;
      if (k < sh_n4) reinterpret_cast<float4*>(lds)[k] = pre[q];
    }
    for (int k = (sh_n4 << 2) + tid; k < sh_total; k += kColorThreads) lds[k] = sh_src[k];
  } else {
    for (int k = tid; k < sh_total; k += kColorThreads) {
      const int row = k / rowf;
      lds[row * ldstride + (k - row * rowf)] = sh_src[k];
    }
  }
  float rmx = 0, rmy = 0, rmz = 0;
  if (valid && in_range && wave < Vs) { rmx = p.means[3 * gi + 0]; rmy = p.means[3 * gi + 1]; rmz = p.means[3 * gi + 2]; }
  __syncthreads();
  if (!in_range || !valid) return;
  const bool dbg = GSR_ABL(p.d.flags, GSR_FLAG_DEBUG_TIMING) && set == 0 && tid == 0;
  if (dbg) dbg_stamps(p, 16384 + unit)[0] = t_start;
  // (the stand-alone colour launch lives on bandwidth at eight workgroups per CU: the compile-time instance buys it nothing)
  color_eval<kJ, false, kShFrame>(p, set, i, lds + lane * ldstride, wave, kColorThreads / 64, Vs, rmx, rmy, rmz,
                        cam_lite(p.views, __builtin_amdgcn_readfirstlane(set * Vs + min(wave, Vs - 1))));
  if (dbg) dbg_stamps(p, 16384 + unit)[1] = __builtin_amdgcn_s_memrealtime();
}

// The same unit of work by ONE wavefront (the colour waves of k_preprocess_bin): the unit's rows come in by LDS-DMA (1 KB per
// instruction, lane l's 16 bytes land at base + 16 l; nothing passes through registers), the wave waits for them and evaluates
// every view of the set, lane = Gaussian.  `lds`: this wave's own kColorLdsFloats floats - no barrier, no other wave involved.
template <bool kJ, bool kShFrame>
__device__ __forceinline__ void color_unit_wave(const Params& p, int set, int unit, float* lds, int lane, int vbegin, int vend) {
  const int N = p.d.num_gaussians, Vs = p.d.views_per_set, M = p.d.sh_coeffs;
  const int g0 = unit * 64, i = g0 + lane;
  const bool in_range = i < N;
  const size_t gi = (size_t)set * N + (in_range ? i : 0);
  if (M == 0) {  // precomputed colours: copy through (no clamp)
    if (in_range)
      for (int vv = vbegin; vv < vend; ++vv)
        p.rgbc[(size_t)(set * Vs + vv) * N + i] = make_float4(p.colors[3 * gi], p.colors[3 * gi + 1], p.colors[3 * gi + 2], 0.f);
    return;
  }
  const int rowf = 3 * M, ldstride = rowf | 1;
  const int cnt = min(64, N - g0);
  const float* sh_src = p.colors + ((size_t)set * N + g0) * rowf;
  const int sh_total = cnt * rowf, sh_n4 = sh_total >> 2;
  const bool dbg = GSR_ABL(p.d.flags, GSR_FLAG_DEBUG_TIMING) && set == 0 && lane == 0;
  unsigned long long* stamp = dbg_stamps(p, 16384 + unit);
  if (dbg) stamp[0] = __builtin_amdgcn_s_memrealtime();
  // the means and the view's parameters are asked for FIRST: vector loads return in order, so they are there when the rows (requested
  // behind them, 3 us of issuing against the stream's back-pressure) are - asked for last, the evaluation waited a round trip for them
  float rmx = 0, rmy = 0, rmz = 0;
  if (in_range) { rmx = p.means[3 * gi + 0]; rmy = p.means[3 * gi + 1]; rmz = p.means[3 * gi + 2]; }
  const CamLite cam0 = cam_lite(p.views, __builtin_amdgcn_readfirstlane(set * Vs + vbegin));
  __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0): the previous unit's LDS reads have returned before its rows are overwritten
  if ((ldstride == rowf) && ((((uintptr_t)sh_src) & 15) == 0)) {
    typedef __attribute__((address_space(3))) void* lds_ptr_t;
    for (int j = 0; 64 * j < sh_n4; ++j) {
      const int k = 64 * j + lane;
      if (k < sh_n4)
        __builtin_amdgcn_global_load_lds(reinterpret_cast<const float4*>(sh_src) + k, (lds_ptr_t)(reinterpret_cast<float4*>(lds) + 64 * j), 16, 0, 0);
    }
    for (int k = (sh_n4 << 2) + lane; k < sh_total; k += 64) lds[k] = sh_src[k];
  } else {
    for (int k = lane; k < sh_total; k += 64) {
      const int row = k / rowf;
      lds[row * ldstride + (k - row * rowf)] = sh_src[k];
    }
  }
  if (dbg) stamp[1] = __builtin_amdgcn_s_memrealtime();
  __builtin_amdgcn_s_waitcnt(0);  // the DMA writes count as vector memory operations (vmcnt); the plain LDS stores as lgkmcnt
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  if (dbg) stamp[2] = __builtin_amdgcn_s_memrealtime();
  __builtin_amdgcn_s_setprio(2);
  if (in_range) color_eval<kJ, true, kShFrame>(p, set, i, lds + lane * ldstride, vbegin, 1, vend, rmx, rmy, rmz, cam0);
  __builtin_amdgcn_s_setprio(0);
  if (dbg) stamp[3] = __builtin_amdgcn_s_memrealtime();
}

// The colour pass as a launch of its own (independent of the binning; images too large for k_preprocess_bin<true, .>).
// kShFrame: GSR_FLAG_SH_IN_FRAME (see color_eval_lane).
template <bool kJ, bool kShFrame>  // kJ: a backward was announced and the colours are harmonics - also save d rgb / d direction (Params::shj)
__global__ __launch_bounds__(kColorThreads) void k_color(const Params p) {
  __shared__ __attribute__((aligned(16))) float lds[kColorLdsFloats];
  color_unit<kJ, kShFrame>(p, blockIdx.x, true, lds, (int)threadIdx.x);
}

// K1 (images of up to kTileWindow tiles): preprocess AND the whole binning of this workgroup's `chunk` Gaussians.
//   1. preprocess the Gaussians; histogram their (tile, splat) pairs per tile in LDS; records leave through the transpose;
//   2. exclusive scan of the histogram over the tiles = where each tile's pairs start INSIDE this workgroup's own region
//      of the key buffer; the row (offset, count) per tile goes to the pair matrix [view][row][tile];
//   3. the region itself is the workgroup's own fixed slot of kStagePairs keys (no atomics at all), or - for the rare workgroup
//      that lists more - a run of pages taken from a bump counter (one device atomic);
//   4. the pairs are walked again from the hit masks still in registers, take their slot with an LDS atomic and are
//      collected in LDS (the 64 KB transpose area, free by now) so that the region is written by one linear copy - keys
//      stored pair by pair are 64 separate 8-byte requests per instruction and were the longest phase of the old emit.
// Nothing here depends on another workgroup: no count matrix prefix, no tile scan, no second pass over the records.
// sort_tile<true> (k_tile_fwd) later collects a tile's list from the <= rows regions (column (v, :, t) of the pair matrix).
// (Same-address device atomics cost ~17 ns each on this chip, one after the other:
// a counter hit by every workgroup of a launch is a serial section, hence the fixed slots here and in the sort.)
// kColor: the colour pass of the workgroup's own Gaussians runs INSIDE this launch - the last five of the sixteen waves
// stream the harmonics of the chunk's 64-Gaussian units through LDS (color_unit_wave: LDS-DMA, 19 KB per wave
// in flight) and evaluate them while the other eleven project and count, then scan, walk the pairs and copy them out - all of
// it under the stream (see the body).  The binning alone is VALU-bound with idle memory pipes, the colour pass a memory stream
// with idle ALUs: together the launch runs at the stream's rate, the separate colour launch (17 us) and its launch boundary are
// gone.  Six / five / four colour waves: 64.2 / 63.8 / 65.7 us for the forward (eleven binning waves put at most five of the
// chunk's 19 units on a SIMD, ten put six).  kJ: see color_eval_lane.
// With V views per set the units of a row are dealt out to the row's V workgroups (one per view), each evaluating all V views.
#ifndef GSR_BIN_CW
#define GSR_BIN_CW 5
#endif
#ifndef GSR_BIN_CB
#define GSR_BIN_CB (GSR_BIN_CW + 1)
#endif
constexpr int kColorViewGroup = 4;  // views a colour task of the binning launch evaluates for its unit
constexpr int kBinColorWaves = GSR_BIN_CW, kBinColorBufs = GSR_BIN_CB;  // unit buffers: one per colour wave + one for the staged pairs
#ifndef GSR_CIB_MAX_TILES
#define GSR_CIB_MAX_TILES 4608
#endif
// images of up to this many tiles take the colour pass inside the binning launch (measured range: 512 x 512 = 4096 tiles take
// 114.8 us that way, 118.8 with the colour pass as a launch of its own)
constexpr int kColorBinMaxTiles = GSR_CIB_MAX_TILES;
constexpr int kBinStageBytes = (kBinThreads / 64 - kBinColorWaves) * 1024;  // kColor: 1 KB of record transpose per binning wave
// dynamic LDS.  Plain: [0, 64 KB) record transpose per wave (4 KB each), later the pair staging; then the T tile counters.
// kColor: [0, 11 KB) record transpose of the eleven binning waves (1 KB each), later the chunk's depth table; the T tile counters;
// five 19 200-byte unit buffers of the colour waves and a sixth for the staged pairs (2 bytes each).
constexpr size_t bin_lds_bytes(int T, bool color) {
  return color ? (size_t)kBinStageBytes + (((size_t)T * 4 + 15) & ~(size_t)15) + (size_t)kBinColorBufs * kColorLdsFloats * 4
               : (size_t)(kBinThreads / 64) * 4096 + (size_t)T * 4;
}
// kMaxT: most tiles of the image the instance is built for.  The plain launch (no colour waves) of an image of at most
// kBinTwoMaxT tiles needs 78-80 KB of LDS, so TWO of its workgroups fit a CU - if they also fit its registers: that instance is
// built for eight waves per SIMD (64 VGPRs; with the per-thread tile counters sized for its own image it does not spill), and the
// VALU-bound launch (0.20 of 0.25 at one workgroup per CU) runs 15 % faster: 8 views 39.1 -> 37.3 us per view, 48 views 23.3 -> 22.2.
// Larger images have room for one workgroup per CU whatever the registers: the 85-register instance (at 64 it spills: one
// 1024 x 1024 view 182 -> 201 us).
constexpr int kBinTwoMaxT = 2048;
static bool bin_two_per_cu(const Grid& g, bool color_in_bin) {
  return GSR_BIN_TWO && !color_in_bin && g.T <= kBinTwoMaxT && 2 * align_up(bin_lds_bytes(g.T, false) + 10400, 1280) <= (size_t)160 * 1024;
}
static bool color_in_bin_by_dims(const GsrDims& d, const Grid& g) {
  // (views_per_set: one colour wave evaluates every view of its unit, so with many views a workgroup's 19 / V units are a few long
  // tasks for its five colour waves - 8 views in one chain were 7 % slower that way than with the separate launch; colour tasks in
  // groups of <= 4 views exist - colour_role - but measured no better than the colour pass as a launch of its own: 352.9 vs 342.2 us)
  const bool fused_bin = g.T <= kFusedMaxTiles && !GSR_ABL(d.flags, GSR_FLAG_ABLATE_NO_COUNT) && !(d.flags & GSR_FLAG_WINDOWED_BINNING);
  return fused_bin && !GSR_ABL(d.flags, GSR_FLAG_ABLATE_NO_SH) && d.views_per_set <= GSR_CIB_MAX_VPS &&
         g.T <= kColorBinMaxTiles && bin_lds_bytes(g.T, true) + 10400u <= 160u * 1024u;  // (+ 10.1 KB static)
}
// kShFrame: the colour waves evaluate harmonics given in their group's frame (GSR_FLAG_SH_IN_FRAME; only with kColor)
template <bool kColor, bool kJ, int kMaxT = kFusedMaxTiles, bool kShFrame = false>
__global__ __launch_bounds__(kBinThreads, (!kColor && kMaxT == kBinTwoMaxT) ? 8 : 4) void k_preprocess_bin(const Params p) {
  extern __shared__ float4 dyn_stage[];  // kBinThreads / 64 waves x 4 KB: record transpose, then pair staging; then T counters;
                                         // then (kColor) one 19 200-byte unit buffer per colour wave
  uint32_t* hist = reinterpret_cast<uint32_t*>(dyn_stage + (kColor ? kBinStageBytes / 16 : (kBinThreads / 64) * 256));
  constexpr int kWavesA = kBinThreads / 64 - (kColor ? kBinColorWaves : 0);  // waves that project and count (phase 1)
  __shared__ float bigs[kBigList][10];
  __shared__ uint32_t nbig, wtot[kBinThreads / 64], sBase, next_unit, bin_bar;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, row = blockIdx.x, v = blockIdx.y;
  const int T = p.g.T, N = p.d.num_gaussians;
  if constexpr (kColor) {
    if (row >= p.rows) {  // (workgroup-uniform) one of the kDealBlocks workgroups behind the rows: the tile launch's deal, nothing else
      const bool dbg = GSR_ABL(p.d.flags, GSR_FLAG_DEBUG_TIMING);  // (stamp slots rows ... rows + 7: behind the binning workgroups')
      unsigned long long* stamp = dbg_stamps(p, (size_t)row);
      GSR_STAMP(0);
      build_tile_order(p, row - p.rows, w, lane);
      GSR_STAMP(1);
      return;
    }
  }
  const bool dbg = GSR_ABL(p.d.flags, GSR_FLAG_DEBUG_TIMING);
  unsigned long long* stamp = dbg_stamps(p, (size_t)(blockIdx.y * p.rows + blockIdx.x));
  GSR_STAMP(0);
  for (int k = tid; k < T; k += kBinThreads) hist[k] = 0;
  if (tid == 0) {
    nbig = 0;
    next_unit = 0;
    bin_bar = 0;
    if (row == 0 && v == 0) {  // only the tile launch touches these, and it runs after this kernel
      p.status->overflow = 0; p.status->max_list = 0; *p.tail_counter = 0u;
      *p.page_counter_tiles = (unsigned long long)p.call_tag << 32;
    }
  }
  __syncthreads();
  const int end = min(N, (row + 1) * p.chunk);
  float4* stage = kColor ? dyn_stage + w * 64 : dyn_stage + w * 256;  // this wave's record-transpose area (kColor: 1 KB)
  constexpr int kIters = (kChunkMax + kWavesA * 64 - 1) / (kWavesA * 64);
  float4 q3s[kIters];
  uint32_t inl = 0;  // bit it: this lane's wide footprint of iteration it did not fit the deferred list
  auto count = [&](int t) { atomicAdd(&hist[t], 1u); };
  // Gaussians of this wave in iteration it (the colour waves have none: `end` for them)
  auto first_of = [&](int it) { return w < kWavesA ? row * p.chunk + w * 64 + it * kWavesA * 64 : end; };
  float* const colbufs = reinterpret_cast<float*>(hist + ((T + 3) & ~3));  // (kColor) the unit buffers; later the pair staging
  // A colour task = one unit of the row x one group of up to kColorViewGroup views of the set.  The row's tasks with task number
  // = vv (mod Vs) are this workgroup's; its colour waves take them as they get free.  Up to four views per set that is "the
  // row's units dealt to the row's workgroups, every view of the set per unit" (the harmonics of a set are read once); with more
  // views a wave that evaluated ALL of them for its unit was a few long tasks for five colour waves (8 views: 379 us against 334
  // with the colour pass as a launch of its own) - in groups of four a workgroup has ~4.75 tasks whatever Vs is, and the unit's
  // rows are read once per group (the repeats come out of L2 / the Infinity Cache: the row's workgroups run side by side).
  // Round 4 measured that form for 8 views (GSR_CIB_MAX_VPS 16): 352.9 us against 342.2 with the separate launch - the binning
  // launch WITHOUT colour waves has sixteen projecting waves instead of eleven, which is worth more than the launch it saves; the
  // limit stays at four views per set.
  auto colour_role = [&](int cbuf) {
    float* buf = colbufs + (size_t)cbuf * kColorLdsFloats;
    const int Vs = p.d.views_per_set, set = v / Vs, vv = v - set * Vs;
    const int u0 = row * p.chunk / 64, u1 = (end + 63) / 64;
    const int groups = (Vs + kColorViewGroup - 1) / kColorViewGroup, ntasks = (u1 - u0) * groups;
    while (true) {
      uint32_t k = 0;
      if (lane == 0) k = atomicAdd(&next_unit, 1u);
      const int t = vv + Vs * (int)__builtin_amdgcn_readfirstlane((int)k);
      if (t >= ntasks) break;
      const int u = u0 + t / groups, g0v = (t - (t / groups) * groups) * kColorViewGroup;
      color_unit_wave<kJ, kShFrame>(p, set, u, buf, lane, g0v, min(Vs, g0v + kColorViewGroup));
    }
  };  // (s_setprio 3 for these waves, or for the binning waves: no gain once the binning waves no longer wait for them)
  if (kColor && w >= kWavesA) colour_role(w - kWavesA);
  // the next unit's inputs are requested before this unit's arithmetic: under the colour stream a trip to memory takes
  // microseconds, and the record stores in between keep the compiler from moving the loads up by itself.  (Two units ahead:
  // no further gain.  Units handed out from an LDS counter instead of in fixed order: +0.5 us)
  GaussIn nxt{};
  if (first_of(0) + lane < end) nxt = load_gauss(p, v, first_of(0) + lane);
#pragma unroll
  for (int it = 0; it < kIters; ++it) {
    const int first = first_of(it);
    q3s[it] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (first >= end) continue;  // wave-uniform
    const int i = first + lane;
    const GaussIn cur = nxt;
    if (it + 1 < kIters && first_of(it + 1) + lane < end) nxt = load_gauss(p, v, first_of(it + 1) + lane);
    PreRec rec{};
    if (i < end) {
      rec = preprocess_one(p, v, i, cur, count, [&](int gi, const Foot& f, float depth) {
        const uint32_t slot = atomicAdd(&nbig, 1u);
        if (slot < (uint32_t)kBigList) {
          float* b = bigs[slot];
          b[0] = f.cx; b[1] = f.cy; b[2] = f.A; b[3] = f.B; b[4] = f.C; b[5] = f.tau;
          b[6] = __int_as_float(f.sx0 | (f.sx1 << 16)); b[7] = __int_as_float(f.sy0 | (f.sy1 << 16));
          b[8] = __int_as_float(gi); b[9] = depth;
        } else {
          inl |= 1u << it;
          big_walk_lane(f, p.g, count);
        }
      });
      q3s[it] = rec.q3;
    }
    if (!GSR_ABL(p.d.flags, GSR_FLAG_ABLATE_NO_GEOM_STORE)) {
      if (kColor) store_records_wave_1k(p.geom + (size_t)v * N + first, end - first, rec, stage, lane);
      else store_records_wave(p.geom + (size_t)v * N + first, end - first, rec, stage, lane);
    }
    if (p.grad_rows) zero_rows_wave(p, v, first, end - first, lane);
  }
  if constexpr (kColor) {
    // ---- steps 2-4 by the binning waves ALONE, under the colour stream.  The colour waves need ~25 us for the chunk's units, the
    // binning waves (which yield the SIMDs to them) are through with the projection after ~20: they go on to the scan, the region
    // and the pair walk at once instead of waiting at a workgroup barrier for the last unit, synchronising among themselves
    // through an LDS counter (s_barrier is workgroup-wide).  The pair staging cannot have the unit buffers now, so a staged pair is
    // 2 bytes - the Gaussian's index inside the chunk - in a unit buffer of their own, and the copy-out rebuilds the key from a depth
    // table of the chunk kept in the (by then idle) transpose area: full lines leave, as before.  (Pairs stored straight from
    // the walk - 8-byte stores - were tried: the launch then ends 5 us later, draining partial lines.)
    constexpr int kBinW = kWavesA, kBinT = kBinW * 64;
    static_assert((kTileWindow / kBinThreads) * kBinT >= kColorBinMaxTiles, "tile counters owned per thread");
    static_assert(kStagePairs * 2 <= kColorLdsFloats * 4 && kChunkMax * 4 <= kBinStageBytes, "staging fits a unit buffer, depths the transpose area");
    auto arrive = [&]() {
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
      if (lane == 0) __hip_atomic_fetch_add(&bin_bar, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    };
    auto wait_for = [&](uint32_t target) {
      while (__hip_atomic_load(&bin_bar, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) < target) __builtin_amdgcn_s_sleep(1);
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    };
    if (w >= kWavesA) return;  // colour waves: done (their units were taken above)
    uint32_t bar = 0;
    auto group_barrier = [&]() { arrive(); bar += kBinW; wait_for(bar); };
    group_barrier();  // every pair of the small footprints is in the histogram, every record has left the transpose area
    float* dtab = reinterpret_cast<float*>(dyn_stage);
    const int chunk0 = row * p.chunk;
#pragma unroll
    for (int it = 0; it < kIters; ++it) {
      const int i = first_of(it) + lane;
      if (i < end) dtab[i - chunk0] = q3s[it].w;
    }
    const int nb = (int)min(nbig, (uint32_t)kBigList);
    for (int e = w; e < nb; e += kBinW)  // wide footprints: one wave each, 64 candidate tiles per step
      big_walk_wave(foot_from_lds(bigs[e], p.g), p.g, lane, count);
    group_barrier();
    GSR_STAMP(1);
    const int per = (T + kBinT - 1) / kBinT;
    const int b0 = tid * per;
    uint32_t cnt[kTileWindow / kBinThreads], sum = 0;
#pragma unroll
    for (int q = 0; q < kTileWindow / kBinThreads; ++q) {
      cnt[q] = (q < per && b0 + q < T) ? hist[b0 + q] : 0u;
      sum += cnt[q];
    }
    const uint32_t incl = wave_inclusive_scan_u32(sum);
    if (lane == 63) wtot[w] = incl;
    group_barrier();  // also: every histogram counter has been read
    uint32_t basew = 0, total = 0;
#pragma unroll
    for (int k = 0; k < kBinW; ++k) {
      const uint32_t x = wtot[k];
      basew += (k < w) ? x : 0u;
      total += x;
    }
    if (tid == 0) {
      const size_t blk = (size_t)v * p.rows + row;
      uint32_t base = (uint32_t)(blk * kSlotStride);
      if (total > (uint32_t)kStagePairs) {
        const uint32_t npages = (total + kPage - 1) / kPage;
        const uint32_t first = take_pages(p.page_counter, p.call_tag, npages), half = p.key_pages / 2;  // lower half of the pool
        base = (first <= half && npages <= half - first) ? p.pool_off + first * (uint32_t)kPage : 0xffffffffu;
      }
      sBase = base;
      p.blk_base[blk] = base;
      p.blk_total[blk] = total;
    }
    uint2* mrow = p.pair_mat + ((size_t)v * p.rows + row) * (T + 8);
    uint32_t run = basew + incl - sum;
#pragma unroll
    for (int q = 0; q < kTileWindow / kBinThreads; ++q)
      if (q < per && b0 + q < T) {
        mrow[b0 + q] = make_uint2(run, cnt[q]);
        hist[b0 + q] = run;  // from here on: the tile's cursor inside the region
        run += cnt[q];
      }
    group_barrier();
    GSR_STAMP(2);
    const uint32_t base = sBase;
    if (base == 0xffffffffu || total == 0) return;
    const bool staged = total <= (uint32_t)kStagePairs;
    unsigned long long* region = p.keys + base;
    unsigned short* st16 = reinterpret_cast<unsigned short*>(colbufs + (size_t)(kBinColorBufs - 1) * kColorLdsFloats);
    auto put = [&](int gi, int t, float depth) {
      const uint32_t slot = atomicAdd(&hist[t], 1u);
      if (staged) st16[slot] = (unsigned short)(gi - chunk0);
      else region[slot] = ((unsigned long long)__float_as_uint(depth) << 32) | (uint32_t)gi;
    };
#pragma unroll
    for (int it = 0; it < kIters; ++it) {
      const int i = first_of(it) + lane;
      if (i >= end) continue;
      walk_pairs(p, q3s[it], i, 0, T, put, [&](int gi) {
        if (!((inl >> it) & 1u)) return;  // deferred: walked by a whole wave below
        const Foot ft = foot_of_record(p.geom + (size_t)v * N + gi, p.g);  // this wave's own store (complete since the first barrier)
        const float depth = q3s[it].w;
        big_walk_lane(ft, p.g, [&](int t) { put(gi, t, depth); });
      });
    }
    for (int e = w; e < nb; e += kBinW) {
      const float* b = bigs[e];
      const int gi = __float_as_int(b[8]);
      const float depth = b[9];
      big_walk_wave(foot_from_lds(b, p.g), p.g, lane, [&](int t) { put(gi, t, depth); });
    }
    GSR_STAMP(3);
    if (staged) {
      group_barrier();
      for (uint32_t k = tid; k < total; k += kBinT) {
        const uint32_t loc = st16[k];
        region[k] = ((unsigned long long)__float_as_uint(dtab[loc]) << 32) | (uint32_t)(chunk0 + (int)loc);
      }
    }
    GSR_STAMP(4);
    return;
  }
  __syncthreads();
  const int nb = (int)min(nbig, (uint32_t)kBigList);
  for (int e = w; e < nb; e += kBinThreads / 64)  // wide footprints: one wave each, 64 candidate tiles per step
    big_walk_wave(foot_from_lds(bigs[e], p.g), p.g, lane, count);
  __syncthreads();
  GSR_STAMP(1);
  // ---- 2. exclusive scan of the histogram over the tiles (thread t owns `per` consecutive tiles)
  const int per = (T + kBinThreads - 1) / kBinThreads;  // <= kMaxT / kBinThreads
  const int b0 = tid * per;
  uint32_t cnt[kMaxT / kBinThreads], sum = 0;
#pragma unroll
  for (int q = 0; q < kMaxT / kBinThreads; ++q) {
    cnt[q] = (q < per && b0 + q < T) ? hist[b0 + q] : 0u;
    sum += cnt[q];
  }
  const uint32_t incl = wave_inclusive_scan_u32(sum);
  if (lane == 63) wtot[w] = incl;
  __syncthreads();  // also: every histogram counter has been read
  uint32_t basew = 0, total = 0;
#pragma unroll
  for (int k = 0; k < kBinThreads / 64; ++k) {
    const uint32_t x = wtot[k];
    basew += (k < w) ? x : 0u;
    total += x;
  }
  // ---- 3. this workgroup's region of the key buffer: its own fixed slot, or (more than kStagePairs pairs) pool pages
  if (tid == 0) {
    const size_t blk = (size_t)v * p.rows + row;
    uint32_t base = (uint32_t)(blk * kSlotStride);
    if (total > (uint32_t)kStagePairs) {
      const uint32_t npages = (total + kPage - 1) / kPage;
      const uint32_t first = take_pages(p.page_counter, p.call_tag, npages), half = p.key_pages / 2;  // lower half of the pool
      base = (first <= half && npages <= half - first) ? p.pool_off + first * (uint32_t)kPage : 0xffffffffu;
    }
    sBase = base;
    p.blk_base[blk] = base;
    p.blk_total[blk] = total;
  }
  uint2* mrow = p.pair_mat + ((size_t)v * p.rows + row) * (T + 8);  // + 8: a column must not sit on one memory channel
  uint32_t run = basew + incl - sum;
#pragma unroll
  for (int q = 0; q < kMaxT / kBinThreads; ++q)
    if (q < per && b0 + q < T) {
      mrow[b0 + q] = make_uint2(run, cnt[q]);
      hist[b0 + q] = run;  // from here on: the tile's cursor inside the region
      run += cnt[q];
    }
  __syncthreads();
  GSR_STAMP(2);
  const uint32_t base = sBase;
  if (base == 0xffffffffu || total == 0) return;  // key buffer too small (the tile launch reports it) / nothing to list
  // ---- 4. the pairs, again, now to their slots
  const bool staged = total <= (uint32_t)kStagePairs;
  unsigned long long* lds_keys = kColor ? reinterpret_cast<unsigned long long*>(colbufs) : reinterpret_cast<unsigned long long*>(dyn_stage);
  unsigned long long* region = p.keys + base;
  auto put = [&](int gi, int t, float depth) {
    const uint32_t slot = atomicAdd(&hist[t], 1u);
    const unsigned long long key = ((unsigned long long)__float_as_uint(depth) << 32) | (uint32_t)gi;
    if (staged) lds_keys[slot] = key;
    else region[slot] = key;
  };
#pragma unroll
  for (int it = 0; it < kIters; ++it) {
    const int i = first_of(it) + lane;
    if (i >= end) continue;
    walk_pairs(p, q3s[it], i, 0, T, put, [&](int gi) {
      if (!((inl >> it) & 1u)) return;  // deferred: walked by a whole wave below
      const Foot ft = foot_of_record(p.geom + (size_t)v * N + gi, p.g);  // this wave's own store, complete since the barriers
      const float depth = q3s[it].w;
      big_walk_lane(ft, p.g, [&](int t) { put(gi, t, depth); });
    });
  }
  for (int e = w; e < nb; e += kBinThreads / 64) {
    const float* b = bigs[e];
    const int gi = __float_as_int(b[8]);
    const float depth = b[9];
    big_walk_wave(foot_from_lds(b, p.g), p.g, lane, [&](int t) { put(gi, t, depth); });
  }
  GSR_STAMP(3);
  if (staged) {
    __syncthreads();
    for (uint32_t k = tid; k < total; k += kBinThreads) region[k] = lds_keys[k];
  }
  GSR_STAMP(4);
}

// ------------------------------------------------------------------------------------------------
// WINDOWED binning path (images of more than kTileWindow tiles, or GSR_FLAG_WINDOWED_BINNING): counting sort of (8x8 tile,
// splat) pairs by tile with exact global offsets and WITHOUT global atomics (device-scope atomics measured ~25 G/s on
// MI355X: 50 us per pass at 1.25 M pairs).  A workgroup owns a chunk of `chunk` Gaussians of one view and histograms its
// pairs per tile in LDS, one window of kTileWindow tiles at a time:
//   k_count       : counts[v][chunk][tile] = pairs of this chunk in this tile     (LDS atomics, coalesced row store)
//   k_tile_prefix : per (v, tile) exclusive scan down the chunk rows, tile totals  (column scan)
//   k_tile_scan   : exclusive scan over all (v, tile) totals -> list ranges, pair total, overflow flag (or inside k_emit)
//   k_emit        : LDS cursors start at range.x + row prefix; each pair takes its slot with one LDS atomic
// Count and emit walk the same footprints with the same code, so slots match counts exactly.  Images of up to kTileWindow
// tiles take k_preprocess_bin + the gathering sort of k_tile_fwd instead (above / below).
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBinThreads) void k_count(const Params p) {
  __shared__ uint32_t hist[kTileWindow];
  const int tid = threadIdx.x, row = blockIdx.x, v = blockIdx.y;
  const int T = p.g.T;
  uint32_t* out = p.counts + ((size_t)v * p.rows + row) * T;
  for (int t0 = 0; t0 < T; t0 += kTileWindow) {
    const int t1 = min(T, t0 + kTileWindow);
    for (int k = tid; k < t1 - t0; k += kBinThreads) hist[k] = 0;
    __syncthreads();
    if (!GSR_ABL(p.d.flags, GSR_FLAG_ABLATE_NO_COUNT))
      for_each_pair(p, v, row, tid, t0, t1, [&](int, int t, float) { atomicAdd(&hist[t - t0], 1u); });
    __syncthreads();
    for (int k = tid; k < t1 - t0; k += kBinThreads) out[t0 + k] = hist[k];
    __syncthreads();
  }
}

// Column prefix of the count matrix.  One workgroup = 16 consecutive (view, tile) columns x 64 row groups (a 64-byte
// segment of every row), so a 1024-tile image spreads over 64 workgroups; a thread keeps its <= kPrefixRegs rows in
// registers between the sum and the write-back (one trip to memory), partial sums are exchanged through LDS.
constexpr int kPrefixRegs = 8;
#ifndef GSR_TP_WAVES
#define GSR_TP_WAVES 8
#endif
__global__ __launch_bounds__(1024, GSR_TP_WAVES) void k_tile_prefix(const Params p) {
  __shared__ uint32_t part[64][17];
  const int cx = threadIdx.x & 15, rg = threadIdx.x >> 4;
  const size_t VT = (size_t)p.d.num_views * p.g.T;
  const size_t col = (size_t)blockIdx.x * 16 + cx;
  const int R = p.rows, T = p.g.T;
  const int rpg = (R + 63) / 64, r0 = rg * rpg, r1 = min(R, r0 + rpg);
  const bool ok = col < VT;
  const size_t v = ok ? col / T : 0, t = ok ? col - v * T : 0;
  uint32_t* base = p.counts + (v * R) * (size_t)T + t;
  const bool in_regs = rpg <= kPrefixRegs;
  uint32_t c[kPrefixRegs];
  uint32_t sum = 0;
  if (in_regs) {
#pragma unroll
    for (int k = 0; k < kPrefixRegs; ++k) {
      c[k] = (ok && r0 + k < r1) ? base[(size_t)(r0 + k) * T] : 0u;
      sum += c[k];
    }
  } else if (ok) {
#pragma unroll 8
    for (int r = r0; r < r1; ++r) sum += base[(size_t)r * T];
  }
  part[rg][cx] = sum;
  __syncthreads();
  uint32_t run = 0, total = 0;
#pragma unroll 16
  for (int k = 0; k < 64; ++k) {
    const uint32_t x = part[k][cx];
    run += (k < rg) ? x : 0u;
    total += x;
  }
  if (ok) {
    if (in_regs) {
#pragma unroll
      for (int k = 0; k < kPrefixRegs; ++k)
        if (r0 + k < r1) {
          base[(size_t)(r0 + k) * T] = run;
          run += c[k];
        }
    } else {
#pragma unroll 8
      for (int r = r0; r < r1; ++r) {
        const uint32_t x = base[(size_t)r * T];
        base[(size_t)r * T] = run;
        run += x;
      }
    }
    if (rg == 0) p.tile_total[col] = total;
  }
}

// One workgroup per chunk of consecutive (view, tile) totals (a multiple of 1024; at most kTileScanBlocks workgroups).  Every workgroup
// reads ALL the totals once, coalesced (a few hundred KB out of L2) and so knows the grand total - which decides the overflow flag
// every range depends on - and the sum in front of its own chunk without waiting for anybody; then an exclusive scan of its chunk,
// 1024 totals at a time.  (Until round 4 this was ONE workgroup whose threads each walked 64 consecutive totals - uncoalesced -
// twice: 115 us for the 65 536 tiles of a 2048 x 2048 image, a fifth of that call.  The number of workgroups is capped because the
// redundant read grows with workgroups x totals: 48 views of 2048 x 2048 are 3 M totals - one workgroup per 1024 of them would move
// 36 GB through the L2s, 128 workgroups move 1.5 GB.)
constexpr int kTileScanBlocks = 128;
static inline unsigned tile_scan_blocks(size_t n) { return (unsigned)std::min<size_t>((n + 1023) / 1024, (size_t)kTileScanBlocks); }
__global__ __launch_bounds__(1024) void k_tile_scan(const Params p) {
  __shared__ unsigned long long sTot[16], sBefore[16], sScan[16];
  __shared__ uint32_t sMax[16];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const size_t n = (size_t)p.d.num_views * p.g.T;
  const size_t chunk = ((n + gridDim.x - 1) / gridDim.x + 1023) / 1024 * 1024;
  const size_t c0 = (size_t)blockIdx.x * chunk, c1 = c0 + chunk < n ? c0 + chunk : n;  // this workgroup's chunk: [c0, c1)
  unsigned long long tot = 0, before = 0;
  uint32_t mx = 0;
  for (size_t k = tid; k < n; k += 1024) {
    const uint32_t t = p.tile_total[k];
    tot += t;
    before += k < c0 ? t : 0u;
    mx = t > mx ? t : mx;
  }
  for (int o = 32; o > 0; o >>= 1) {
    tot += __shfl_down(tot, o, 64);
    before += __shfl_down(before, o, 64);
    mx = max(mx, (uint32_t)__shfl_down((int)mx, o, 64));
  }
  if (lane == 0) { sTot[w] = tot; sBefore[w] = before; sMax[w] = mx; }
  __syncthreads();
  unsigned long long total = 0, carry = 0;
  uint32_t gmax = 0;
#pragma unroll
  for (int q = 0; q < 16; ++q) {
    total += sTot[q];
    carry += sBefore[q];
    gmax = max(gmax, sMax[q]);
  }
  const bool overflow = total > (unsigned long long)p.d.pair_capacity;
  for (size_t s0 = c0; s0 < c1; s0 += 1024) {  // (workgroup-uniform bounds)
    const size_t k = s0 + tid;
    const uint32_t mine = k < n ? p.tile_total[k] : 0u;
    // inclusive scan inside the wave (64-bit: 1024 long lists can pass 2^32 only in theory, the running sum can)
    unsigned long long incl = mine;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const uint32_t lo = (uint32_t)__shfl_up((int)(uint32_t)incl, o, 64), hi = (uint32_t)__shfl_up((int)(uint32_t)(incl >> 32), o, 64);
      if (lane >= o) incl += ((unsigned long long)hi << 32) | lo;
    }
    if (lane == 63) sScan[w] = incl;
    __syncthreads();
    unsigned long long run = carry, step = 0;
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      run += q < w ? sScan[q] : 0ull;
      step += sScan[q];
    }
    run += incl - mine;
    if (k < n) p.ranges[k] = overflow ? make_uint2(0u, 0u) : make_uint2((uint32_t)run, (uint32_t)(run + mine));
    carry += step;
    __syncthreads();  // sScan is written again by the next 1024 totals
  }
  if (blockIdx.x == 0 && tid == 0) {
    p.status->num_pairs = total;
    p.status->overflow = overflow ? 1u : 0u;
    p.status->max_list = gmax;
  }
}

// With kScan the workgroup computes the list ranges itself (exclusive scan of all V*T tile totals, <= kEmitScanMax of
// them) instead of reading them from a separate k_tile_scan launch: ~2 us of redundant work per workgroup buys one kernel
// boundary (~6.5 us at 1024 tiles).  Block (0,0) publishes ranges + status for the kernels that follow.
constexpr int kEmitScanMax = 8192;

template <bool kScan>
__global__ __launch_bounds__(kBinThreads) void k_emit(const Params p) {
  __shared__ uint32_t cursor[kTileWindow];
  __shared__ unsigned long long wtot[kBinThreads / 64];
  __shared__ uint32_t smax, nbig;
  __shared__ int bigs[kBigList];
  const int tid = threadIdx.x, row = blockIdx.x, v = blockIdx.y;
  const int T = p.g.T;
  const uint32_t* rowp = p.counts + ((size_t)v * p.rows + row) * T;
  const uint32_t cap = (uint32_t)p.d.pair_capacity;
  const bool dbg = GSR_ABL(p.d.flags, GSR_FLAG_DEBUG_TIMING);
  unsigned long long* stamp = p.keys + (size_t)cap - (size_t)(blockIdx.x + 1) * 8;
  GSR_STAMP(0);
  if (kScan) {
    const int VT = p.d.num_views * T;
    const int per = (VT + kBinThreads - 1) / kBinThreads;  // <= 8
    const int b = tid * per, e = min(VT, b + per);
    const int lo_t = v * T, hi_t = lo_t + min(T, kTileWindow);  // kScan implies T <= kEmitScanMax <= kTileWindow: one window
    const int N = p.d.num_gaussians, gend = min(N, (row + 1) * p.chunk);
    // every global read of this workgroup is issued up front (tile totals, this row's prefixes, the records of the
    // Gaussians it will walk) so that one memory latency covers them all
    uint32_t tot[kEmitScanMax / kBinThreads], rowv[kEmitScanMax / kBinThreads];
    float4 q3r[kChunkMax / kBinThreads];
#pragma unroll
    for (int q = 0; q < kEmitScanMax / kBinThreads; ++q) {
      const bool on = q < per && b + q < e;
      tot[q] = on ? p.tile_total[b + q] : 0u;
      rowv[q] = (on && b + q >= lo_t && b + q < hi_t) ? rowp[b + q - lo_t] : 0u;
    }
#pragma unroll
    for (int u = 0; u < kChunkMax / kBinThreads; ++u) {
      const int i = row * p.chunk + tid + u * kBinThreads;
      q3r[u] = i < gend ? p.aux[(size_t)v * N + i] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    unsigned long long sum = 0;
    uint32_t mx = 0;
#pragma unroll
    for (int q = 0; q < kEmitScanMax / kBinThreads; ++q) {
      sum += tot[q];
      mx = max(mx, tot[q]);
    }
    GSR_STAMP(1);
    // block exclusive scan of the 64-bit per-thread sums: wave scan (shuffles) + 16 wave totals through LDS
    const int lane = tid & 63, w = tid >> 6;
    unsigned long long incl = sum;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const uint32_t lo = (uint32_t)__shfl_up((int)(uint32_t)incl, o, 64), hi = (uint32_t)__shfl_up((int)(uint32_t)(incl >> 32), o, 64);
      if (lane >= o) incl += ((unsigned long long)hi << 32) | lo;
    }
    if (tid == 0) { smax = 0; nbig = 0; }
    if (lane == 63) wtot[w] = incl;
    __syncthreads();
    unsigned long long basew = 0, total = 0;
#pragma unroll
    for (int k = 0; k < kBinThreads / 64; ++k) {
      const unsigned long long x = wtot[k];
      basew += (k < w) ? x : 0ull;
      total += x;
    }
    GSR_STAMP(2);
    const bool publish = (row == 0 && v == 0);
    if (publish) {
      mx = wave_max_u32(mx);
      if (lane == 0) atomicMax(&smax, mx);
    }
    const bool overflow = total > (unsigned long long)cap;
    unsigned long long run = basew + incl - sum;
#pragma unroll
    for (int q = 0; q < kEmitScanMax / kBinThreads; ++q) {
      const int k = b + q;
      if (q < per && k < e) {
        if (publish) p.ranges[k] = overflow ? make_uint2(0u, 0u) : make_uint2((uint32_t)run, (uint32_t)(run + tot[q]));
        if (k >= lo_t && k < hi_t) cursor[k - lo_t] = (uint32_t)run + rowv[q];
        run += tot[q];
      }
    }
    __syncthreads();
    if (publish && tid == 0) {
      p.status->num_pairs = total;
      p.status->overflow = overflow ? 1u : 0u;
      p.status->max_list = smax;
    }
    if (overflow) return;
    GSR_STAMP(3);
    auto put = [&](int gi, int t, float depth) {
      const uint32_t slot = GSR_ABL(p.d.flags, GSR_FLAG_ABLATE_EMIT_NO_ATOMIC) ? cursor[t] : atomicAdd(&cursor[t], 1u);
      if (slot < cap && !GSR_ABL(p.d.flags, GSR_FLAG_ABLATE_EMIT_NO_STORE))
        p.keys[slot] = ((unsigned long long)__float_as_uint(depth) << 32) | (uint32_t)gi;
    };
#pragma unroll
    for (int u = 0; u < kChunkMax / kBinThreads; ++u) {
      const int i = row * p.chunk + tid + u * kBinThreads;
      if (i < gend)
        walk_pairs(p, q3r[u], i, 0, T, put, [&](int gi) {
          const uint32_t slot = atomicAdd(&nbig, 1u);
          if (slot < (uint32_t)kBigList) {
            bigs[slot] = gi;
          } else {
            const Foot ft = foot_of_record(p.geom + (size_t)v * N + gi, p.g);
            big_walk_lane(ft, p.g, [&](int t) { put(gi, t, q3r[u].w); });
          }
        });
    }
    __syncthreads();
    {  // wide footprints: one wave each, 64 candidate tiles per step
      const int nb = (int)min(nbig, (uint32_t)kBigList);
      for (int e = w; e < nb; e += kBinThreads / 64) {
        const int gi = bigs[e];
        const GeomRec* rec = p.geom + (size_t)v * N + gi;
        const Foot ft = foot_of_record(rec, p.g);
        const float depth = p.aux[(size_t)v * N + gi].w;
        big_walk_wave(ft, p.g, lane, [&](int t) { put(gi, t, depth); });
      }
    }
    GSR_STAMP(4);
    return;
  }
  if (p.status->overflow) return;
  const uint2* rng = p.ranges + (size_t)v * T;
  for (int t0 = 0; t0 < T; t0 += kTileWindow) {
    const int t1 = min(T, t0 + kTileWindow);
    for (int k = tid; k < t1 - t0; k += kBinThreads) cursor[k] = rng[t0 + k].x + rowp[t0 + k];
    __syncthreads();
    for_each_pair(p, v, row, tid, t0, t1, [&](int i, int t, float depth) {
      const uint32_t slot = GSR_ABL(p.d.flags, GSR_FLAG_ABLATE_EMIT_NO_ATOMIC) ? cursor[t - t0] : atomicAdd(&cursor[t - t0], 1u);
      if (slot < cap && !GSR_ABL(p.d.flags, GSR_FLAG_ABLATE_EMIT_NO_STORE))
        p.keys[slot] = ((unsigned long long)__float_as_uint(depth) << 32) | (uint32_t)i;
    });
    __syncthreads();
  }
}

}  // namespace gsr
