#pragma once
#include "gsr_common.h"

// ------------------------------------------------------------------------------------------------
// Gaussian adapter: the step right in front of the raster path - per-pixel network outputs to means,
// scale + quaternion records and masked harmonics (reference src/model/encoder/common/gaussian_adapter.py:60-87 with
// get_world_rays of projection.py) - as ONE launch in each direction instead of the ~25 elementwise torch kernels, the per-Gaussian
// 3 x 3 solve and the split / broadcast copies of pf3plat_amd/adapter.py.  A workgroup takes kAdaptBlock consecutive Gaussians of
// ONE group (scene x source view): every thread builds the group's K^-1, R, t and scale multiplier from uniform loads (in fp64:
// a few dozen operations per thread against ~340 B of traffic per Gaussian); the block's raw rows - one contiguous stretch of
// the input when the row stride is the row width or the 84 of the encoder's `gaussians[..., 2:]` slice - are staged in LDS with
// 16-byte loads (the LDS image is shifted by the stretch's misalignment so both sides stay aligned), the 7-float heads are read
// from there by the block's first wave, and the 3 M harmonics floats of the block leave as one contiguous stream of 16-byte
// stores, the band mask chosen by column.  The backward recomputes everything from the forward's inputs (nothing is saved),
// assembles the block's dL/draw rows in LDS and writes them with streaming 16-byte stores; the camera-to-world gradient is one
// wave-reduced row of 12 floats per workgroup, added up in a fixed order by k_adapt_pose_reduce: the same bits on every run.
// When the intrinsics want a gradient (gsr_adapt_backward_ex with dL_dintrinsics) a second instance of the backward appends ten
// sums to that row - the cotangents of K^-1 (9) and of the scale multiplier (1) - and k_adapt_camera_reduce, launched in place of
// k_adapt_pose_reduce, carries them back to K in fp64 (formulas: include/gsr.h).  Still two launches.
// ------------------------------------------------------------------------------------------------
namespace gsr {
constexpr int kAdaptBlock = 64;       // Gaussians per workgroup
constexpr int kAdaptThreads = 256;
constexpr int kAdaptPoseFloats = 12;  // sum of dmean (x) (depth ray) (9), sum of dmean (3)
constexpr int kAdaptIntrFloats = 10;  // behind them when intrinsics want a gradient: sum of d_p (x) (u, v, 1) (9), cotangent of AdaptGroup::mult (1)
constexpr int kAdaptSlack = 8;        // a row stride of up to this many floats over the row width is streamed gaps included

struct AdaptArgs {
  int G, P, stride, lstride, height, width;
  float lo, hi, eps;
  const float *ext, *intr, *coords, *depths, *raw;
  float *means, *scale_rot, *harm;
  const float *d_means, *d_sr, *d_harm;
  float *d_raw, *d_depths, *d_coords, *partials;
};

struct AdaptGroup {
  float kinv[9], rot[9], t[3], mult;
};

// K^-1 (adjugate / determinant), camera-to-world rotation and centre, and 0.1 x sum(K[:2, :2]^-1 (1 / w, 1 / h)) of one group
__device__ __forceinline__ AdaptGroup adapt_group(const float* __restrict__ e, const float* __restrict__ k, int h, int w) {
  AdaptGroup o;
  const double a = k[0], b = k[1], c = k[2], d = k[3], ee = k[4], f = k[5], g = k[6], hh = k[7], i = k[8];
  const double c00 = ee * i - f * hh, c01 = c * hh - b * i, c02 = b * f - c * ee;
  const double c10 = f * g - d * i, c11 = a * i - c * g, c12 = c * d - a * f;
  const double c20 = d * hh - ee * g, c21 = b * g - a * hh, c22 = a * ee - b * d;
  const double inv = 1.0 / (a * c00 + b * c10 + c * c20);
  o.kinv[0] = (float)(c00 * inv); o.kinv[1] = (float)(c01 * inv); o.kinv[2] = (float)(c02 * inv);
  o.kinv[3] = (float)(c10 * inv); o.kinv[4] = (float)(c11 * inv); o.kinv[5] = (float)(c12 * inv);
  o.kinv[6] = (float)(c20 * inv); o.kinv[7] = (float)(c21 * inv); o.kinv[8] = (float)(c22 * inv);
  const double px = (double)(1.0f / (float)w), py = (double)(1.0f / (float)h);
  o.mult = (float)(0.1 * ((ee * px - b * py) + (a * py - d * px)) / c22);
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    o.rot[3 * r] = e[4 * r]; o.rot[3 * r + 1] = e[4 * r + 1]; o.rot[3 * r + 2] = e[4 * r + 2];
    o.t[r] = e[4 * r + 3];
  }
  return o;
}

// band l of the harmonics is scaled by 0.1 x 0.25^l, the DC term by 1 (gaussian_adapter.py:40-44); m: coefficient index in [0, 25)
__device__ __forceinline__ float adapt_mask(int m) {
  return m == 0 ? 1.f : m < 4 ? 0.1f * 0.25f : m < 9 ? 0.1f * 0.0625f : m < 16 ? 0.1f * 0.015625f : 0.1f * 0.00390625f;
}

// The per-Gaussian arithmetic both directions share: unit ray through the pixel, the sigmoid of the scale features, quaternion norm
struct AdaptPoint {
  float p[3], n, denom, ray[3], sig[3], qn, qd;
};
__device__ __forceinline__ AdaptPoint adapt_point(const AdaptGroup& grp, float u, float v, const float* head) {
  AdaptPoint o;
#pragma unroll
  for (int r = 0; r < 3; ++r) o.p[r] = grp.kinv[3 * r] * u + grp.kinv[3 * r + 1] * v + grp.kinv[3 * r + 2];
  o.n = sqrtf(o.p[0] * o.p[0] + o.p[1] * o.p[1] + o.p[2] * o.p[2]);
  o.denom = fmaxf(o.n, 1e-12f);  // F.normalize
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    o.ray[r] = o.p[r] / o.denom;
    o.sig[r] = 1.f / (1.f + expf(-head[r]));
  }
  o.qn = sqrtf(head[3] * head[3] + head[4] * head[4] + head[5] * head[5] + head[6] * head[6]);
  return o;
}

template <int D>
__global__ __launch_bounds__(kAdaptThreads) void k_adapt_fwd(const AdaptArgs a) {
  constexpr int M = (D + 1) * (D + 1), C = 3 * M, ROWF = 7 + C;
  extern __shared__ __attribute__((aligned(16))) float adapt_lds[];
  const int nb = (a.P + kAdaptBlock - 1) / kAdaptBlock;
  const int g = (int)blockIdx.x / nb, r0 = ((int)blockIdx.x - g * nb) * kAdaptBlock;
  const int cnt = min(kAdaptBlock, a.P - r0), tid = threadIdx.x;
  const size_t first = (size_t)g * a.P + r0;
  const float* __restrict__ src = a.raw + first * (size_t)a.stride;
  int sh = 0;
  if (a.lstride == a.stride) {  // the block's rows as one stretch of the input, gaps between rows included
    sh = (int)(((uintptr_t)src >> 2) & 3);
    float* img = adapt_lds + sh;
    const int total = (cnt - 1) * a.stride + ROWF;  // ends with the last row: nothing behind it is read
    const int head = min(total, (4 - sh) & 3);
    if (tid < head) img[tid] = src[tid];
    const int n4 = (total - head) >> 2;
    const float4* __restrict__ s4 = reinterpret_cast<const float4*>(src + head);
    float4* d4 = reinterpret_cast<float4*>(img + head);
#pragma unroll 6
    for (int k = tid; k < n4; k += kAdaptThreads) d4[k] = s4[k];
    for (int k = head + (n4 << 2) + tid; k < total; k += kAdaptThreads) img[k] = src[k];
  } else {  // rows far apart: row by row into a compact image
    for (int e = tid; e < cnt * ROWF; e += kAdaptThreads) {
      const int row = e / ROWF, col = e - row * ROWF;
      adapt_lds[e] = src[(size_t)row * a.stride + col];
    }
  }
  const AdaptGroup grp = adapt_group(a.ext + (size_t)g * 16, a.intr + (size_t)g * 9, a.height, a.width);
  __syncthreads();
  const float* img = adapt_lds + sh;
  if (tid < cnt) {
    const float* head = img + tid * a.lstride;
    const size_t gi = first + tid;
    const float u = a.coords[2 * gi], v = a.coords[2 * gi + 1], dep = a.depths[gi];
    float hd[7];
#pragma unroll
    for (int k = 0; k < 7; ++k) hd[k] = head[k];
    const AdaptPoint pt = adapt_point(grp, u, v, hd);
    const float fp = dep * grp.mult, qd = pt.qn + a.eps;
    float* mo = a.means + 3 * gi;
    float* so = a.scale_rot + 7 * gi;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      const float dir = grp.rot[3 * r] * pt.ray[0] + grp.rot[3 * r + 1] * pt.ray[1] + grp.rot[3 * r + 2] * pt.ray[2];
      mo[r] = grp.t[r] + dir * dep;
      so[r] = (a.lo + (a.hi - a.lo) * pt.sig[r]) * fp;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) so[3 + k] = hd[3 + k] / qd;
  }
  // the block's harmonics: cnt x 3 M consecutive output floats
  float* __restrict__ out = a.harm + first * C;
  const int total = cnt * C;
  const auto value = [&](int e) {
    const int row = e / C, col = e - row * C;
    return img[row * a.lstride + 7 + col] * adapt_mask(col % M);
  };
  if ((((uintptr_t)out) & 15) == 0) {
    const int n4 = total >> 2;
    for (int k = tid; k < n4; k += kAdaptThreads)
      reinterpret_cast<float4*>(out)[k] = make_float4(value(4 * k), value(4 * k + 1), value(4 * k + 2), value(4 * k + 3));
    for (int e = (n4 << 2) + tid; e < total; e += kAdaptThreads) out[e] = value(e);
  } else {
    for (int e = tid; e < total; e += kAdaptThreads) out[e] = value(e);
  }
}

// KG: the intrinsics want a gradient - the partial row is kAdaptPoseFloats + kAdaptIntrFloats wide; everything else is the same code
template <int D, bool KG>
__global__ __launch_bounds__(kAdaptThreads) void k_adapt_bwd(const AdaptArgs a) {
  constexpr int M = (D + 1) * (D + 1), C = 3 * M, ROWF = 7 + C;
  constexpr int PARTF = kAdaptPoseFloats + (KG ? kAdaptIntrFloats : 0);
  __shared__ __attribute__((aligned(16))) float rows[kAdaptBlock * ROWF];  // the block's dL/draw rows
  const int nb = (a.P + kAdaptBlock - 1) / kAdaptBlock;
  const int g = (int)blockIdx.x / nb, blk = (int)blockIdx.x - g * nb, r0 = blk * kAdaptBlock;
  const int cnt = min(kAdaptBlock, a.P - r0), tid = threadIdx.x;
  const size_t first = (size_t)g * a.P + r0;
  // harmonics: dL/draw = mask x dL/dharmonics (zeros without a cotangent), one contiguous input stream
  const int total = cnt * C;
  const float* __restrict__ gh = a.d_harm ? a.d_harm + first * C : nullptr;
  const auto put = [&](int e, float x) {
    const int row = e / C, col = e - row * C;
    rows[row * ROWF + 7 + col] = x * adapt_mask(col % M);
  };
  if (gh && (((uintptr_t)gh) & 15) == 0) {
    const int n4 = total >> 2;
#pragma unroll 5
    for (int k = tid; k < n4; k += kAdaptThreads) {
      const float4 x = reinterpret_cast<const float4*>(gh)[k];
      put(4 * k, x.x); put(4 * k + 1, x.y); put(4 * k + 2, x.z); put(4 * k + 3, x.w);
    }
    for (int e = (n4 << 2) + tid; e < total; e += kAdaptThreads) put(e, gh[e]);
  } else {
    for (int e = tid; e < total; e += kAdaptThreads) put(e, gh ? gh[e] : 0.f);
  }
  if (tid < 64) {  // one wave: the 7-float heads, depth, pixel offsets, and the group's camera gradient
    float pose[kAdaptPoseFloats];
#pragma unroll
    for (int k = 0; k < kAdaptPoseFloats; ++k) pose[k] = 0.f;
    float kg[kAdaptIntrFloats];  // (dead code without KG)
#pragma unroll
    for (int k = 0; k < kAdaptIntrFloats; ++k) kg[k] = 0.f;
    if (tid < cnt) {
      const AdaptGroup grp = adapt_group(a.ext + (size_t)g * 16, a.intr + (size_t)g * 9, a.height, a.width);
      const size_t gi = first + tid;
      const float* __restrict__ head = a.raw + gi * (size_t)a.stride;
      float hd[7], gs[7], gm[3];
#pragma unroll
      for (int k = 0; k < 7; ++k) {
        hd[k] = head[k];
        gs[k] = a.d_sr ? a.d_sr[7 * gi + k] : 0.f;
      }
#pragma unroll
      for (int k = 0; k < 3; ++k) gm[k] = a.d_means ? a.d_means[3 * gi + k] : 0.f;
      const float u = a.coords[2 * gi], v = a.coords[2 * gi + 1], dep = a.depths[gi];
      const AdaptPoint pt = adapt_point(grp, u, v, hd);
      const float fp = dep * grp.mult, range = a.hi - a.lo;
      float* row = rows + tid * ROWF;
      float d_dep = 0.f, d_ray[3] = {0.f, 0.f, 0.f};
#pragma unroll
      for (int r = 0; r < 3; ++r) {
        const float dir = grp.rot[3 * r] * pt.ray[0] + grp.rot[3 * r + 1] * pt.ray[1] + grp.rot[3 * r + 2] * pt.ray[2];
        d_dep += gm[r] * dir + gs[r] * (a.lo + range * pt.sig[r]) * grp.mult;
        row[r] = gs[r] * fp * range * (pt.sig[r] * (1.f - pt.sig[r]));
        const float d_dir = gm[r] * dep;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          d_ray[c] += grp.rot[3 * r + c] * d_dir;
          pose[3 * r + c] = gm[r] * (dep * pt.ray[c]);
        }
        pose[9 + r] = gm[r];
      }
      a.d_depths[gi] = d_dep;
      // through the normalisation (the norm's own gradient is taken as 0 where it was clamped, as torch does) and K^-1
      const float along = pt.n > 1e-12f ? pt.ray[0] * d_ray[0] + pt.ray[1] * d_ray[1] + pt.ray[2] * d_ray[2] : 0.f;
      float d_u = 0.f, d_v = 0.f;
#pragma unroll
      for (int r = 0; r < 3; ++r) {
        const float d_p = (d_ray[r] - pt.ray[r] * along) / pt.denom;
        d_u += d_p * grp.kinv[3 * r];
        d_v += d_p * grp.kinv[3 * r + 1];
        if constexpr (KG) {
          kg[3 * r] = d_p * u; kg[3 * r + 1] = d_p * v; kg[3 * r + 2] = d_p;
        }
      }
      if constexpr (KG) {
        float d_fp = 0.f;
#pragma unroll
        for (int r = 0; r < 3; ++r) d_fp += gs[r] * (a.lo + range * pt.sig[r]);
        kg[9] = dep * d_fp;
      }
      a.d_coords[2 * gi] = d_u;
      a.d_coords[2 * gi + 1] = d_v;
      // q / (|q| + eps): a zero quaternion takes the norm's gradient as 0 (torch's norm backward)
      const float qd = pt.qn + a.eps;
      const float qg = hd[3] * gs[3] + hd[4] * gs[4] + hd[5] * gs[5] + hd[6] * gs[6];
      const float back = pt.qn > 0.f ? qg / (qd * qd * pt.qn) : 0.f;
#pragma unroll
      for (int k = 0; k < 4; ++k) row[3 + k] = gs[3 + k] / qd - hd[3 + k] * back;
    }
    if (a.partials) {
#pragma unroll
      for (int k = 0; k < kAdaptPoseFloats; ++k) pose[k] = wave_sum(pose[k]);
      if (tid < kAdaptPoseFloats) {
        float mine = 0.f;
#pragma unroll
        for (int k = 0; k < kAdaptPoseFloats; ++k) mine = tid == k ? pose[k] : mine;
        a.partials[((size_t)g * nb + blk) * PARTF + tid] = mine;
      }
      if constexpr (KG) {
#pragma unroll
        for (int k = 0; k < kAdaptIntrFloats; ++k) kg[k] = wave_sum(kg[k]);
        if (tid >= kAdaptPoseFloats && tid < PARTF) {
          float mine = 0.f;
#pragma unroll
          for (int k = 0; k < kAdaptIntrFloats; ++k) mine = tid == kAdaptPoseFloats + k ? kg[k] : mine;
          a.partials[((size_t)g * nb + blk) * PARTF + tid] = mine;
        }
      }
    }
  }
  __syncthreads();
  // streaming stores, like the dense gradients of k_preprocess_bwd (unstage_rows): written once, read next by autograd
  float* __restrict__ dst = a.d_raw + first * ROWF;
  const int out_total = cnt * ROWF;
  if ((((uintptr_t)dst) & 15) == 0) {
    typedef float f4v_ __attribute__((ext_vector_type(4)));
    const int n4 = out_total >> 2;
    for (int k = tid; k < n4; k += kAdaptThreads) {
      const float4 x = reinterpret_cast<const float4*>(rows)[k];
      __builtin_nontemporal_store(f4v_{x.x, x.y, x.z, x.w}, reinterpret_cast<f4v_*>(dst) + k);
    }
    for (int k = (n4 << 2) + tid; k < out_total; k += kAdaptThreads) dst[k] = rows[k];
  } else {
    for (int k = tid; k < out_total; k += kAdaptThreads) dst[k] = rows[k];
  }
}

// dL/dextrinsics (G, 4, 4) from the per-workgroup rows: block g adds the nb rows of group g in a fixed order (252 threads = 21 rows x
// 12 columns per step, then the 21 partial rows one after the other).  Rows 0-2 x columns 0-2: sum of dmean (x) (depth ray); column 3:
// sum of dmean; bottom row zero.
__global__ __launch_bounds__(256) void k_adapt_pose_reduce(const float* __restrict__ partials, int nb, float* __restrict__ d_ext) {
  __shared__ float part[21][kAdaptPoseFloats];
  const int g = blockIdx.x, tid = threadIdx.x, k = tid % kAdaptPoseFloats, r = tid / kAdaptPoseFloats;
  const float* base = partials + (size_t)g * nb * kAdaptPoseFloats;
  if (r < 21) {
    float acc = 0.f;
    for (int i = r; i < nb; i += 21) acc += base[(size_t)i * kAdaptPoseFloats + k];
    part[r][k] = acc;
  }
  __syncthreads();
  if (tid < 16) {
    const int row = tid >> 2, col = tid & 3;
    float sum = 0.f;
    if (row < 3) {
      const int idx = col < 3 ? 3 * row + col : 9 + row;
      for (int j = 0; j < 21; ++j) sum += part[j][idx];
    }
    d_ext[(size_t)g * 16 + tid] = sum;
  }
}

// The same sum over rows of kAdaptPoseFloats + kAdaptIntrFloats floats (k_adapt_bwd<D, true>): dL/dextrinsics from the first 12
// columns in exactly k_adapt_pose_reduce's order (the same bits), and dL/dintrinsics (G, 3, 3) from the other ten, added up in
// fp64 in the same fixed order and carried through K^-1 and the scale multiplier of adapt_group in fp64:
//   dL/dK = -K^-T Ginv K^-T,   dL/dK[:2, :2] += -0.1 g_mult (K2^-T 1) (K2^-1 q)^T,   K2 = K[:2, :2], q = (1 / w, 1 / h)
__global__ __launch_bounds__(256) void k_adapt_camera_reduce(const float* __restrict__ partials, int nb, const float* __restrict__ intr, int h, int w,
                                                             float* __restrict__ d_ext, float* __restrict__ d_intr) {
  constexpr int PARTF = kAdaptPoseFloats + kAdaptIntrFloats;
  __shared__ float part[21][kAdaptPoseFloats];
  __shared__ double parti[21][kAdaptIntrFloats];
  __shared__ double tot[kAdaptIntrFloats];
  const int g = blockIdx.x, tid = threadIdx.x, k = tid % kAdaptPoseFloats, r = tid / kAdaptPoseFloats;
  const float* base = partials + (size_t)g * nb * PARTF;
  if (r < 21) {
    float acc = 0.f;
    for (int i = r; i < nb; i += 21) acc += base[(size_t)i * PARTF + k];
    part[r][k] = acc;
    if (k < kAdaptIntrFloats) {
      double wide = 0.0;
      for (int i = r; i < nb; i += 21) wide += (double)base[(size_t)i * PARTF + kAdaptPoseFloats + k];
      parti[r][k] = wide;
    }
  }
  __syncthreads();
  if (tid < 16) {
    const int row = tid >> 2, col = tid & 3;
    float sum = 0.f;
    if (row < 3) {
      const int idx = col < 3 ? 3 * row + col : 9 + row;
      for (int j = 0; j < 21; ++j) sum += part[j][idx];
    }
    d_ext[(size_t)g * 16 + tid] = sum;
  } else if (tid >= 64 && tid < 64 + kAdaptIntrFloats) {
    double sum = 0.0;
    for (int j = 0; j < 21; ++j) sum += parti[j][tid - 64];
    tot[tid - 64] = sum;
  }
  __syncthreads();
  if (tid < 9) {
    const float* kk = intr + (size_t)g * 9;
    const double a = kk[0], b = kk[1], c = kk[2], d = kk[3], ee = kk[4], f = kk[5], gg = kk[6], hh = kk[7], i = kk[8];
    double inv[9] = {ee * i - f * hh, c * hh - b * i, b * f - c * ee, f * gg - d * i, a * i - c * gg, c * d - a * f,
                     d * hh - ee * gg, b * gg - a * hh, a * ee - b * d};
    const double det2 = inv[8], rdet = 1.0 / (a * inv[0] + b * inv[3] + c * inv[6]);
#pragma unroll
    for (int j = 0; j < 9; ++j) inv[j] *= rdet;
    const int row = tid / 3, col = tid - 3 * row;
    // -(K^-T Ginv K^-T)[row][col] = -sum_rc K^-1[r][row] Ginv[r][c] K^-1[col][c]
    double sum = 0.0;
#pragma unroll
    for (int rr = 0; rr < 3; ++rr) {
      double t = 0.0;
#pragma unroll
      for (int cc = 0; cc < 3; ++cc) t += tot[3 * rr + cc] * inv[3 * col + cc];
      sum += inv[3 * rr + row] * t;
    }
    sum = -sum;
    if (row < 2 && col < 2) {
      const double px = (double)(1.0f / (float)w), py = (double)(1.0f / (float)h);
      const double ones[2] = {(ee - d) / det2, (a - b) / det2};               // K2^-T (1, 1)
      const double q[2] = {(ee * px - b * py) / det2, (a * py - d * px) / det2};  // K2^-1 (1 / w, 1 / h)
      sum -= 0.1 * tot[9] * ones[row] * q[col];
    }
    d_intr[(size_t)g * 9 + tid] = (float)sum;
  }
}

static bool adapt_sizes_ok(int G, int P, int sh_degree, int64_t stride, int height, int width) {
  if (G < 0 || P < 0 || sh_degree < 0 || sh_degree > 4 || height <= 0 || width <= 0) return false;
  const int rowf = 7 + 3 * (sh_degree + 1) * (sh_degree + 1);
  if (stride < rowf || stride > (int64_t)1 << 24) return false;
  const int64_t blocks = (int64_t)G * (((int64_t)P + kAdaptBlock - 1) / kAdaptBlock);
  return blocks <= 0x7fffffff;
}

template <template <int> class Launch>
static void adapt_dispatch(int degree, const AdaptArgs& a, hipStream_t st) {
  switch (degree) {
    case 0: Launch<0>::go(a, st); break;
    case 1: Launch<1>::go(a, st); break;
    case 2: Launch<2>::go(a, st); break;
    case 3: Launch<3>::go(a, st); break;
    default: Launch<4>::go(a, st); break;
  }
}
static unsigned adapt_grid(const AdaptArgs& a) { return (unsigned)a.G * (unsigned)((a.P + kAdaptBlock - 1) / kAdaptBlock); }
template <int D>
struct AdaptFwdLaunch {
  static void go(const AdaptArgs& a, hipStream_t st) {
    constexpr int ROWF = 7 + 3 * (D + 1) * (D + 1);
    const size_t floats = a.lstride == a.stride ? (size_t)(kAdaptBlock - 1) * a.stride + ROWF + 4 : (size_t)kAdaptBlock * ROWF;
    hipLaunchKernelGGL(k_adapt_fwd<D>, dim3(adapt_grid(a)), dim3(kAdaptThreads), floats * sizeof(float), st, a);
  }
};
template <int D>
struct AdaptBwdLaunch {
  static void go(const AdaptArgs& a, hipStream_t st) {
    hipLaunchKernelGGL((k_adapt_bwd<D, false>), dim3(adapt_grid(a)), dim3(kAdaptThreads), 0, st, a);
  }
};
template <int D>
struct AdaptBwdIntrLaunch {
  static void go(const AdaptArgs& a, hipStream_t st) {
    hipLaunchKernelGGL((k_adapt_bwd<D, true>), dim3(adapt_grid(a)), dim3(kAdaptThreads), 0, st, a);
  }
};
}  // namespace gsr

extern "C" {

size_t gsr_adapt_partials_bytes_ex(int num_groups, int gaussians_per_group, int with_intrinsics) {
  if (num_groups <= 0 || gaussians_per_group <= 0) return 0;
  const int rowf = gsr::kAdaptPoseFloats + (with_intrinsics ? gsr::kAdaptIntrFloats : 0);
  return (size_t)num_groups * (size_t)((gaussians_per_group + gsr::kAdaptBlock - 1) / gsr::kAdaptBlock) * rowf * sizeof(float);
}
size_t gsr_adapt_partials_bytes(int num_groups, int gaussians_per_group) { return gsr_adapt_partials_bytes_ex(num_groups, gaussians_per_group, 0); }

int gsr_adapt(int num_groups, int gaussians_per_group, int sh_degree, const float* extrinsics, const float* intrinsics,
              const float* coordinates, const float* depths, const float* raw, int64_t raw_row_stride, float scale_min,
              float scale_max, int height, int width, float eps, float* means, float* scale_rot, float* harmonics, void* stream_) {
  using namespace gsr;
  if (!adapt_sizes_ok(num_groups, gaussians_per_group, sh_degree, raw_row_stride, height, width)) return GSR_ERR_INVALID_ARGUMENT;
  if (num_groups == 0 || gaussians_per_group == 0) return GSR_OK;
  if (!extrinsics || !intrinsics || !coordinates || !depths || !raw || !means || !scale_rot || !harmonics) return GSR_ERR_INVALID_ARGUMENT;
  const int rowf = 7 + 3 * (sh_degree + 1) * (sh_degree + 1);
  AdaptArgs a{};
  a.G = num_groups; a.P = gaussians_per_group; a.stride = (int)raw_row_stride;
  a.lstride = raw_row_stride - rowf <= kAdaptSlack ? (int)raw_row_stride : rowf;
  a.height = height; a.width = width; a.lo = scale_min; a.hi = scale_max; a.eps = eps;
  a.ext = extrinsics; a.intr = intrinsics; a.coords = coordinates; a.depths = depths; a.raw = raw;
  a.means = means; a.scale_rot = scale_rot; a.harm = harmonics;
  adapt_dispatch<AdaptFwdLaunch>(sh_degree, a, static_cast<hipStream_t>(stream_));
  GSR_CHECK(hipGetLastError());
  return GSR_OK;
}

int gsr_adapt_backward(int num_groups, int gaussians_per_group, int sh_degree, const float* extrinsics, const float* intrinsics,
                       const float* coordinates, const float* depths, const float* raw, int64_t raw_row_stride, float scale_min,
                       float scale_max, int height, int width, float eps, const float* dL_dmeans, const float* dL_dscale_rot,
                       const float* dL_dharmonics, float* dL_draw, float* dL_ddepths, float* dL_dcoordinates, float* dL_dextrinsics,
                       float* partials, void* stream_) {
  return gsr_adapt_backward_ex(num_groups, gaussians_per_group, sh_degree, extrinsics, intrinsics, coordinates, depths, raw, raw_row_stride, scale_min,
                               scale_max, height, width, eps, dL_dmeans, dL_dscale_rot, dL_dharmonics, dL_draw, dL_ddepths, dL_dcoordinates,
                               dL_dextrinsics, nullptr, partials, stream_);
}

int gsr_adapt_backward_ex(int num_groups, int gaussians_per_group, int sh_degree, const float* extrinsics, const float* intrinsics,
                          const float* coordinates, const float* depths, const float* raw, int64_t raw_row_stride, float scale_min,
                          float scale_max, int height, int width, float eps, const float* dL_dmeans, const float* dL_dscale_rot,
                          const float* dL_dharmonics, float* dL_draw, float* dL_ddepths, float* dL_dcoordinates, float* dL_dextrinsics,
                          float* dL_dintrinsics, float* partials, void* stream_) {
  using namespace gsr;
  if (!adapt_sizes_ok(num_groups, gaussians_per_group, sh_degree, raw_row_stride, height, width)) return GSR_ERR_INVALID_ARGUMENT;
  if (num_groups == 0 || gaussians_per_group == 0) return GSR_OK;
  if (!extrinsics || !intrinsics || !coordinates || !depths || !raw || !dL_draw || !dL_ddepths || !dL_dcoordinates || !dL_dextrinsics || !partials)
    return GSR_ERR_INVALID_ARGUMENT;
  hipStream_t st = static_cast<hipStream_t>(stream_);
  AdaptArgs a{};
  a.G = num_groups; a.P = gaussians_per_group; a.stride = (int)raw_row_stride; a.lstride = a.stride;
  a.height = height; a.width = width; a.lo = scale_min; a.hi = scale_max; a.eps = eps;
  a.ext = extrinsics; a.intr = intrinsics; a.coords = coordinates; a.depths = depths; a.raw = raw;
  a.d_means = dL_dmeans; a.d_sr = dL_dscale_rot; a.d_harm = dL_dharmonics;
  a.d_raw = dL_draw; a.d_depths = dL_ddepths; a.d_coords = dL_dcoordinates; a.partials = partials;
  const int nb = (gaussians_per_group + kAdaptBlock - 1) / kAdaptBlock;
  if (dL_dintrinsics) {
    adapt_dispatch<AdaptBwdIntrLaunch>(sh_degree, a, st);
    GSR_CHECK(hipGetLastError());
    hipLaunchKernelGGL(k_adapt_camera_reduce, dim3((unsigned)num_groups), dim3(256), 0, st, partials, nb, intrinsics, height, width, dL_dextrinsics,
                       dL_dintrinsics);
  } else {
    adapt_dispatch<AdaptBwdLaunch>(sh_degree, a, st);
    GSR_CHECK(hipGetLastError());
    hipLaunchKernelGGL(k_adapt_pose_reduce, dim3((unsigned)num_groups), dim3(256), 0, st, partials, nb, dL_dextrinsics);
  }
  GSR_CHECK(hipGetLastError());
  return GSR_OK;
}

}  // extern "C"
