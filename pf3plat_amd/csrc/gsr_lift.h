#pragma once
#include "gsr_common.h"
#include "gsr_cost_volume.h"  // cv_lin
#include "gsr_pose_loss.h"    // pose_inv3

// ------------------------------------------------------------------------------------------------
// Depth lift (reference src/model/encoder/encoder_costvolume.py:265, 287-307, 506, 525-528; definition: include/gsr.h): the mono-depth
// network's output -> the refined depth, the per-pixel points and the one-hot mono cue, one launch; and the Pluecker ray map
// (:211-221, 387-392).  The cue is the cost volume's neighbour in the depth predictor's input: it shares the volume's (v b) row
// order and its candidates (cv_lin).
// One grid, two kinds of workgroup, told apart by blockIdx (uniform):
//   cue   - 64 consecutive quarter-resolution pixels of one image.  Wave 0 forms `down`, torch's bilinear resize, from taps that are
//           recomputed from depth_raw and shift (the `depth` output is never read back: no ordering inside the launch); thread
//           (part, q) scans a quarter of the candidates for pixel q - a full first-minimum scan, strict <, so ties go to the lowest
//           channel and a NaN or an infinite `down` leaves channel 0 -; the four parts are merged in ascending order.  Then the
//           workgroup writes its 64-pixel segment of every channel row once: a lane holds four pixels' channels and stores
//           float4(ch == d), a wave instruction four rows x 256 contiguous bytes.  No zero-fill, no scatter, no volume but the output.
//   full  - 1024 consecutive pixels of one image, four per thread (float4 where h w is a multiple of 4 and the arrays are 16-byte
//           aligned): depth = clamp(clamp(raw) + shift), one fp32 rounding; the ray K^-1 (u, v, 1) is affine in (x, y) with fp64
//           coefficients formed once per thread from the full fp64 inverse, rounded once to fp32 and multiplied by the depth.
// Backward: the full partition again; m1, m2 and the ray are recomputed.  The intrinsics gradient, on request, is G = sum_p g_xyz
// (u, v, 1)^T depth per image: fp64 per thread, xor tree per wave, waves in order -> 9 doubles per workgroup in the caller's scratch;
// a finishing launch adds an image's workgroups in order and forms -K^-T G K^-T.  No atomics: the same bits on every run.
// ------------------------------------------------------------------------------------------------
namespace gsr {
constexpr int kLiftPix = 1024;  // full-resolution pixels of a workgroup
constexpr int kLiftQ = 64;      // quarter-resolution pixels of a cue workgroup

struct LiftArgs {
  int B, V, H, W, D, Hq, Wq;
  int full_chunks, cue_chunks;  // workgroups per image of each kind
  int vec_full, vec_cue;        // float4 accesses are aligned
  const float *raw, *shift, *near, *far, *intr, *lin;
  float *depth, *xyz, *cue;
  const float *g_depth, *g_xyz;  // backward
  float *d_raw, *d_shift, *d_intr;
  double* partials;  // (images, full_chunks, 9)
};

// torch's clamp(x, lo, hi) = min(max(x, lo), hi) as comparisons: a NaN x fails both and stays.
__device__ __forceinline__ float lift_clamp(float x, float lo, float hi) {
  const float t = x < lo ? lo : x;
  return hi < t ? hi : t;
}

// The refined depth of one pixel; m1, m2: whether the first and the second clamp pass a gradient (inclusive at the bounds).
__device__ __forceinline__ float lift_depth_of(float raw, float shift, float lo, float hi, bool& m1, bool& m2) {
  const float t = lift_clamp(raw, lo, hi) + shift;
  m1 = raw >= lo && raw <= hi;
  m2 = t >= lo && t <= hi;
  return lift_clamp(t, lo, hi);
}

// K^-1 of one image in fp64 (all nine entries, by cofactors) and the ray of pixel (x, y)'s centre as an affine map:
// ray_c = R[3 c] x + R[3 c + 1] y + R[3 c + 2].
__device__ __forceinline__ void lift_rays(const float* Kn, int W, int H, double* Ki, double* R) {
  double K[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) K[k] = (double)Kn[k];
  pose_inv3(K, Ki);
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    R[3 * c] = Ki[3 * c] / (double)W;
    R[3 * c + 1] = Ki[3 * c + 1] / (double)H;
    R[3 * c + 2] = 0.5 * R[3 * c] + 0.5 * R[3 * c + 1] + Ki[3 * c + 2];
  }
}

// One axis of torch's bilinear resize (align_corners = False): the two source indices and the weight of the second.
__device__ __forceinline__ void lift_resize_axis(int dst, int in, int out, int& i0, int& i1, float& l1) {
  const float scale = (float)in / (float)out;
  float src = scale * ((float)dst + 0.5f) - 0.5f;
  src = src < 0.f ? 0.f : src;
  i0 = min((int)src, in - 1);
  i1 = i0 + (i0 < in - 1 ? 1 : 0);
  l1 = src - (float)i0;
}

__device__ __forceinline__ void lift_cue_block(const LiftArgs& a, int blk) {
  __shared__ float down_s[kLiftQ];
  __shared__ float best_v[4][kLiftQ];
  __shared__ int best_i[4][kLiftQ];
  const int Q = a.Hq * a.Wq;
  const int img = blk / a.cue_chunks, q0 = (blk - img * a.cue_chunks) * kLiftQ;
  const int s = img / a.V, i = img - s * a.V;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int q = q0 + lane;
  if (wv == 0) {
    float down = 0.f;
    if (q < Q) {
      const int qy = q / a.Wq, qx = q - qy * a.Wq;
      int x0, x1, y0, y1;
      float lx, ly;
      lift_resize_axis(qx, a.W, a.Wq, x0, x1, lx);
      lift_resize_axis(qy, a.H, a.Hq, y0, y1, ly);
      const float lo = a.near[img], hi = a.far[img];
      const size_t base = (size_t)img * a.H * a.W;
      const size_t r0 = base + (size_t)y0 * a.W, r1 = base + (size_t)y1 * a.W;
      bool m1, m2;
      const float v00 = lift_depth_of(a.raw[r0 + x0], a.shift[r0 + x0], lo, hi, m1, m2);
      const float v01 = lift_depth_of(a.raw[r0 + x1], a.shift[r0 + x1], lo, hi, m1, m2);
      const float v10 = lift_depth_of(a.raw[r1 + x0], a.shift[r1 + x0], lo, hi, m1, m2);
      const float v11 = lift_depth_of(a.raw[r1 + x1], a.shift[r1 + x1], lo, hi, m1, m2);
      down = (1.f - ly) * ((1.f - lx) * v00 + lx * v01) + ly * ((1.f - lx) * v10 + lx * v11);
    }
    down_s[lane] = down;
  }
  __syncthreads();
  {  // the scan of candidates [wv per, (wv + 1) per) for pixel `lane`: the hypotheses of scene 0, view 0, INVERSE depths against a depth
    const float lo_h = 1.f / a.far[0], step = 1.f / a.near[0] - lo_h;
    const float down = down_s[lane];
    const int per = (a.D + 3) / 4, d_end = min(a.D, (wv + 1) * per);
    float best = INFINITY;
    int at = 0;
    for (int d = wv * per; d < d_end; ++d) {
      const float lin = a.lin ? a.lin[d] : cv_lin(d, a.D);
      const float diff = fabsf(down - (lo_h + lin * step));
      if (diff < best) { best = diff; at = d; }
    }
    best_v[wv][lane] = best;
    best_i[wv][lane] = at;
  }
  __syncthreads();
  const size_t row = (size_t)i * a.B + s;  // view-major, as the cost volume's rows
  float* out = a.cue + row * (size_t)a.D * Q;
  if (a.vec_cue) {  // (Q is a multiple of 4: a float4 is inside the image or outside it)
    const int qq = (lane & 15) * 4;
    int ch[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      float best = best_v[0][qq + k];
      ch[k] = best_i[0][qq + k];
#pragma unroll
      for (int part = 1; part < 4; ++part)
        if (best_v[part][qq + k] < best) { best = best_v[part][qq + k]; ch[k] = best_i[part][qq + k]; }
    }
    if (q0 + qq < Q)
      for (int d = wv * 4 + (lane >> 4); d < a.D; d += 16)
        *reinterpret_cast<float4*>(out + (size_t)d * Q + q0 + qq) =
            make_float4(ch[0] == d ? 1.f : 0.f, ch[1] == d ? 1.f : 0.f, ch[2] == d ? 1.f : 0.f, ch[3] == d ? 1.f : 0.f);
  } else {
    float best = best_v[0][lane];
    int ch = best_i[0][lane];
#pragma unroll
    for (int part = 1; part < 4; ++part)
      if (best_v[part][lane] < best) { best = best_v[part][lane]; ch = best_i[part][lane]; }
    if (q < Q)
      for (int d = wv; d < a.D; d += 4) out[(size_t)d * Q + q] = ch == d ? 1.f : 0.f;
  }
}

__device__ __forceinline__ void lift_full_block(const LiftArgs& a, int blk) {
  const int HW = a.H * a.W;
  const int img = blk / a.full_chunks, p0 = (blk - img * a.full_chunks) * kLiftPix + (int)threadIdx.x * 4;
  if (p0 >= HW) return;
  const int n = min(4, HW - p0);
  double Ki[9], R[9];
  lift_rays(a.intr + (size_t)img * 9, a.W, a.H, Ki, R);
  const float lo = a.near[img], hi = a.far[img];
  const size_t at = (size_t)img * HW + p0, at3 = (size_t)img * 3 * HW + p0;
  float raw[4] = {0.f, 0.f, 0.f, 0.f}, sh[4] = {0.f, 0.f, 0.f, 0.f}, dep[4], pt[3][4];
  if (a.vec_full) {
    const float4 r4 = *reinterpret_cast<const float4*>(a.raw + at), s4 = *reinterpret_cast<const float4*>(a.shift + at);
    raw[0] = r4.x; raw[1] = r4.y; raw[2] = r4.z; raw[3] = r4.w;
    sh[0] = s4.x; sh[1] = s4.y; sh[2] = s4.z; sh[3] = s4.w;
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (k < n) { raw[k] = a.raw[at + k]; sh[k] = a.shift[at + k]; }
  }
  int y = p0 / a.W, x = p0 - y * a.W;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    bool m1, m2;
    dep[k] = lift_depth_of(raw[k], sh[k], lo, hi, m1, m2);
#pragma unroll
    for (int c = 0; c < 3; ++c) pt[c][k] = (float)(R[3 * c] * (double)x + R[3 * c + 1] * (double)y + R[3 * c + 2]) * dep[k];
    if (++x == a.W) { x = 0; ++y; }
  }
  if (a.vec_full) {
    *reinterpret_cast<float4*>(a.depth + at) = make_float4(dep[0], dep[1], dep[2], dep[3]);
#pragma unroll
    for (int c = 0; c < 3; ++c) *reinterpret_cast<float4*>(a.xyz + at3 + (size_t)c * HW) = make_float4(pt[c][0], pt[c][1], pt[c][2], pt[c][3]);
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (k < n) {
        a.depth[at + k] = dep[k];
#pragma unroll
        for (int c = 0; c < 3; ++c) a.xyz[at3 + (size_t)c * HW + k] = pt[c][k];
      }
  }
}

__global__ __launch_bounds__(256) void k_lift_fwd(const LiftArgs a) {
  const int cue_blocks = a.B * a.V * a.cue_chunks;  // (the cue, most of the traffic, first)
  if ((int)blockIdx.x < cue_blocks) lift_cue_block(a, (int)blockIdx.x);
  else lift_full_block(a, (int)blockIdx.x - cue_blocks);
}

template <bool kIntr>
__global__ __launch_bounds__(256) void k_lift_bwd(const LiftArgs a) {
  __shared__ double red[4][9];
  const int HW = a.H * a.W;
  const int img = (int)blockIdx.x / a.full_chunks, p0 = ((int)blockIdx.x - img * a.full_chunks) * kLiftPix + (int)threadIdx.x * 4;
  const int n = max(0, min(4, HW - p0));
  double G[9] = {0., 0., 0., 0., 0., 0., 0., 0., 0.};
  if (n > 0) {
    double Ki[9], R[9];
    lift_rays(a.intr + (size_t)img * 9, a.W, a.H, Ki, R);
    const float lo = a.near[img], hi = a.far[img];
    const size_t at = (size_t)img * HW + p0, at3 = (size_t)img * 3 * HW + p0;
    float raw[4] = {0.f, 0.f, 0.f, 0.f}, sh[4] = {0.f, 0.f, 0.f, 0.f}, gd[4] = {0.f, 0.f, 0.f, 0.f}, gx[3][4] = {};
    float ds[4], dr[4];
    if (a.vec_full) {
      const float4 r4 = *reinterpret_cast<const float4*>(a.raw + at), s4 = *reinterpret_cast<const float4*>(a.shift + at);
      raw[0] = r4.x; raw[1] = r4.y; raw[2] = r4.z; raw[3] = r4.w;
      sh[0] = s4.x; sh[1] = s4.y; sh[2] = s4.z; sh[3] = s4.w;
      if (a.g_depth) {
        const float4 g4 = *reinterpret_cast<const float4*>(a.g_depth + at);
        gd[0] = g4.x; gd[1] = g4.y; gd[2] = g4.z; gd[3] = g4.w;
      }
      if (a.g_xyz) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const float4 g4 = *reinterpret_cast<const float4*>(a.g_xyz + at3 + (size_t)c * HW);
          gx[c][0] = g4.x; gx[c][1] = g4.y; gx[c][2] = g4.z; gx[c][3] = g4.w;
        }
      }
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (k < n) {
          raw[k] = a.raw[at + k];
          sh[k] = a.shift[at + k];
          if (a.g_depth) gd[k] = a.g_depth[at + k];
          if (a.g_xyz) {
#pragma unroll
            for (int c = 0; c < 3; ++c) gx[c][k] = a.g_xyz[at3 + (size_t)c * HW + k];
          }
        }
    }
    int y = p0 / a.W, x = p0 - y * a.W;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      bool m1, m2;
      const float dep = lift_depth_of(raw[k], sh[k], lo, hi, m1, m2);
      double g = (double)gd[k];
#pragma unroll
      for (int c = 0; c < 3; ++c) g += (double)gx[c][k] * (R[3 * c] * (double)x + R[3 * c + 1] * (double)y + R[3 * c + 2]);
      ds[k] = m2 ? (float)g : 0.f;
      dr[k] = m1 ? ds[k] : 0.f;
      if (kIntr && k < n) {
        const double u = ((double)x + 0.5) / (double)a.W, v = ((double)y + 0.5) / (double)a.H;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const double gz = (double)gx[c][k] * (double)dep;
          G[3 * c] += gz * u; G[3 * c + 1] += gz * v; G[3 * c + 2] += gz;
        }
      }
      if (++x == a.W) { x = 0; ++y; }
    }
    if (a.vec_full) {
      if (a.d_shift) *reinterpret_cast<float4*>(a.d_shift + at) = make_float4(ds[0], ds[1], ds[2], ds[3]);
      if (a.d_raw) *reinterpret_cast<float4*>(a.d_raw + at) = make_float4(dr[0], dr[1], dr[2], dr[3]);
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (k < n) {
          if (a.d_shift) a.d_shift[at + k] = ds[k];
          if (a.d_raw) a.d_raw[at + k] = dr[k];
        }
    }
  }
  if (kIntr) {  // (every thread of the workgroup arrives here)
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
#pragma unroll
    for (int k = 0; k < 9; ++k) G[k] = wave_sum_f64(G[k]);
    if (lane == 0) {
#pragma unroll
      for (int k = 0; k < 9; ++k) red[wv][k] = G[k];
    }
    __syncthreads();
    if (tid < 9) a.partials[(size_t)blockIdx.x * 9 + tid] = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
  }
}

// One workgroup of 64 per image: lane k < 9 adds entry k of the image's workgroups in order; dK = -K^-T G K^-T.
__global__ __launch_bounds__(64) void k_lift_intr_finish(const LiftArgs a) {
  __shared__ double Gs[9];
  const int img = blockIdx.x, tid = threadIdx.x;
  if (tid < 9) {
    double sum = 0.;
    for (int c = 0; c < a.full_chunks; ++c) sum += a.partials[((size_t)img * a.full_chunks + c) * 9 + tid];
    Gs[tid] = sum;
  }
  __syncthreads();
  if (tid < 9) {
    double Ki[9], R[9];
    lift_rays(a.intr + (size_t)img * 9, a.W, a.H, Ki, R);
    const int r = tid / 3, c = tid - 3 * r;
    double sum = 0.;
    for (int m = 0; m < 3; ++m)
      for (int n = 0; n < 3; ++n) sum += Ki[3 * m + r] * Gs[3 * m + n] * Ki[3 * c + n];
    a.d_intr[(size_t)img * 9 + tid] = (float)(-sum);
  }
}

struct PluckerArgs {
  int images, H, W;
  const float *c2w, *intr;
  float* out;
};

// A thread per pixel; everything in fp64 (the map is small), rounded once.  Six coalesced plane stores.
__global__ __launch_bounds__(256) void k_plucker_rays(const PluckerArgs a) {
  const int HW = a.H * a.W, chunks = (HW + 255) / 256;
  const int img = (int)blockIdx.x / chunks, p = ((int)blockIdx.x - img * chunks) * 256 + (int)threadIdx.x;
  if (p >= HW) return;
  double Ki[9], R[9];
  lift_rays(a.intr + (size_t)img * 9, a.W, a.H, Ki, R);
  const int y = p / a.W, x = p - y * a.W;
  double d[3], wd[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) d[c] = R[3 * c] * (double)x + R[3 * c + 1] * (double)y + R[3 * c + 2];
  const double rn = 1.0 / sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
  const float* E = a.c2w + (size_t)img * 16;
#pragma unroll
  for (int c = 0; c < 3; ++c) wd[c] = ((double)E[4 * c] * d[0] + (double)E[4 * c + 1] * d[1] + (double)E[4 * c + 2] * d[2]) * rn;
  const double o[3] = {(double)E[3], (double)E[7], (double)E[11]};
  float* out = a.out + (size_t)img * 6 * HW + p;
  out[0] = (float)wd[0];
  out[(size_t)HW] = (float)wd[1];
  out[(size_t)2 * HW] = (float)wd[2];
  out[(size_t)3 * HW] = (float)(o[1] * wd[2] - o[2] * wd[1]);
  out[(size_t)4 * HW] = (float)(o[2] * wd[0] - o[0] * wd[2]);
  out[(size_t)5 * HW] = (float)(o[0] * wd[1] - o[1] * wd[0]);
}

// The checks of the lift's entry points; D = 1 for the calls that have no cue.
static bool lift_sizes_ok(int B, int V, int H, int W, int D) {
  if (B < 0 || V < 1 || H < 4 || W < 4 || D < 1) return false;
  const int64_t lim = 0x7fffffff, rows = (int64_t)B * V, hw = (int64_t)H * W, q = (int64_t)(H / 4) * (W / 4);
  return rows <= lim && hw <= lim && rows * hw <= lim && rows * hw * 3 <= lim && rows * q <= lim && rows * q * (int64_t)D <= lim;
}

static bool lift_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

static void lift_fill(LiftArgs& a, int B, int V, int H, int W, int D) {
  a.B = B; a.V = V; a.H = H; a.W = W; a.D = D; a.Hq = H / 4; a.Wq = W / 4;
  a.full_chunks = (int)(((int64_t)H * W + kLiftPix - 1) / kLiftPix);
  a.cue_chunks = (int)(((int64_t)a.Hq * a.Wq + kLiftQ - 1) / kLiftQ);
}
}  // namespace gsr

extern "C" {

size_t gsr_lift_scratch_bytes(int num_scenes, int num_views, int height, int width) {
  if (!gsr::lift_sizes_ok(num_scenes, num_views, height, width, 1)) return 0;
  const int64_t chunks = ((int64_t)height * width + gsr::kLiftPix - 1) / gsr::kLiftPix;
  return (size_t)num_scenes * num_views * (size_t)chunks * 9 * sizeof(double);
}

int gsr_lift_depth(int num_scenes, int num_views, int height, int width, int num_depth_candidates, const float* depth_raw,
                   const float* shift, const float* near, const float* far, const float* intrinsics, const float* lin, float* depth,
                   float* xyz, float* cue, void* stream_) {
  using namespace gsr;
  if (!lift_sizes_ok(num_scenes, num_views, height, width, num_depth_candidates)) return GSR_ERR_INVALID_ARGUMENT;
  if (!depth_raw || !shift || !near || !far || !intrinsics || !depth || !xyz || !cue) return GSR_ERR_INVALID_ARGUMENT;
  if (num_scenes == 0) return GSR_OK;
  LiftArgs a{};
  lift_fill(a, num_scenes, num_views, height, width, num_depth_candidates);
  a.raw = depth_raw; a.shift = shift; a.near = near; a.far = far; a.intr = intrinsics; a.lin = lin;
  a.depth = depth; a.xyz = xyz; a.cue = cue;
  a.vec_full = (height * width) % 4 == 0 && lift_aligned16(depth_raw) && lift_aligned16(shift) && lift_aligned16(depth) && lift_aligned16(xyz);
  a.vec_cue = (a.Hq * a.Wq) % 4 == 0 && lift_aligned16(cue);
  const int64_t blocks = (int64_t)num_scenes * num_views * ((int64_t)a.full_chunks + a.cue_chunks);
  if (blocks > 0x7fffffff) return GSR_ERR_INVALID_ARGUMENT;
  hipLaunchKernelGGL(k_lift_fwd, dim3((unsigned)blocks), dim3(256), 0, static_cast<hipStream_t>(stream_), a);
  GSR_CHECK(hipGetLastError());
  return GSR_OK;
}

int gsr_lift_depth_backward(int num_scenes, int num_views, int height, int width, const float* depth_raw, const float* shift,
                            const float* near, const float* far, const float* intrinsics, const float* dL_ddepth, const float* dL_dxyz,
                            float* dL_ddepth_raw, float* dL_dshift, float* dL_dintrinsics, void* scratch, void* stream_) {
  using namespace gsr;
  if (!lift_sizes_ok(num_scenes, num_views, height, width, 1)) return GSR_ERR_INVALID_ARGUMENT;
  if (!depth_raw || !shift || !near || !far || !intrinsics || (dL_dintrinsics && !scratch)) return GSR_ERR_INVALID_ARGUMENT;
  if (num_scenes == 0) return GSR_OK;
  hipStream_t st = static_cast<hipStream_t>(stream_);
  LiftArgs a{};
  lift_fill(a, num_scenes, num_views, height, width, 1);
  a.raw = depth_raw; a.shift = shift; a.near = near; a.far = far; a.intr = intrinsics;
  a.g_depth = dL_ddepth; a.g_xyz = dL_dxyz; a.d_raw = dL_ddepth_raw; a.d_shift = dL_dshift; a.d_intr = dL_dintrinsics;
  a.partials = static_cast<double*>(scratch);
  a.vec_full = (height * width) % 4 == 0 && lift_aligned16(depth_raw) && lift_aligned16(shift) && lift_aligned16(dL_ddepth) &&
               lift_aligned16(dL_dxyz) && lift_aligned16(dL_ddepth_raw) && lift_aligned16(dL_dshift);
  const int64_t blocks = (int64_t)num_scenes * num_views * a.full_chunks;
  if (dL_dintrinsics) {
    hipLaunchKernelGGL(k_lift_bwd<true>, dim3((unsigned)blocks), dim3(256), 0, st, a);
    GSR_CHECK(hipGetLastError());
    hipLaunchKernelGGL(k_lift_intr_finish, dim3((unsigned)(num_scenes * num_views)), dim3(64), 0, st, a);
  } else {
    hipLaunchKernelGGL(k_lift_bwd<false>, dim3((unsigned)blocks), dim3(256), 0, st, a);
  }
  GSR_CHECK(hipGetLastError());
  return GSR_OK;
}

int gsr_plucker_rays(int num_scenes, int num_views, int height, int width, const float* c2w, const float* intrinsics, float* out,
                     void* stream_) {
  using namespace gsr;
  if (num_scenes < 0 || num_views < 1 || height < 1 || width < 1 || !c2w || !intrinsics || !out) return GSR_ERR_INVALID_ARGUMENT;
  const int64_t lim = 0x7fffffff, rows = (int64_t)num_scenes * num_views, hw = (int64_t)height * width;
  if (rows > lim || hw > lim || rows * hw > lim || rows * hw * 6 > lim) return GSR_ERR_INVALID_ARGUMENT;
  if (num_scenes == 0) return GSR_OK;
  PluckerArgs a{(int)rows, height, width, c2w, intrinsics, out};
  hipLaunchKernelGGL(k_plucker_rays, dim3((unsigned)(rows * ((hw + 255) / 256))), dim3(256), 0, static_cast<hipStream_t>(stream_), a);
  GSR_CHECK(hipGetLastError());
  return GSR_OK;
}

}  // extern "C"
