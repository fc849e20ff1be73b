#pragma once
#include "gsr_common.h"

// ------------------------------------------------------------------------------------------------
// Image losses next to the raster path: the reference's photometric terms - LossMse (src/loss/loss_mse.py:23-36:
// weight x mean squared error), LossMultiSSIM (src/loss/loss_multissim.py:24-83: weight x (1 - mean SSIM map), 11 x 11 Gaussian
// window, sigma 1.5, zero padding, C1 = 0.01^2, C2 = 0.03^2) and the clipped squared error behind compute_psnr
// (src/evaluation/metrics.py:11-19) - evaluated in ONE launch that also writes dL/dprediction in the (image, 3, H, W) layout
// gsr_backward reads as dL_dcolor.  In torch the SSIM term alone is five depthwise convolutions forward and their
// transposes backward (dozens of launches on images this small).
//   SSIM map S = A B / (C D),  A = 2 mu1 mu2 + C1,  B = 2 sigma12 + C2,  C = mu1^2 + mu2^2 + C1,  D = sigma1^2 + sigma2^2 + C2,
//   with mu = w * x, sigma1^2 = w * x1^2 - mu1^2, sigma12 = w * x1 x2 - mu1 mu2 (w * . = windowed mean).  For the prediction x1:
//   dS/dx1(p) = [w * dmu](p) + 2 x1(p) [w * a](p) + x2(p) [w * b](p)   (the window is symmetric), where at every map position
//   a = dS/d(w*x1^2) = -A B / (C D^2),  b = dS/d(w*x1x2) = 2 A / (C D),
//   dmu = dS/dmu1 = 2 mu2 (B - A) / (C D) - 2 mu1 A B / (C^2 D) + 2 mu1 A B / (C D^2).
// One workgroup = one 16 x 16 tile of one channel of one image: inputs on the 36 x 36 halo region -> five windowed means on
// 26 x 26 (separable) -> S, a, b, dmu there (zero outside the image: those map positions do not exist) -> three windowed sums
// back on 16 x 16.  Partial sums (squared error, clipped squared error, SSIM map) go to one slot per workgroup: the caller adds
// them up (deterministic).
// ------------------------------------------------------------------------------------------------
namespace gsr {
constexpr int kLossTile = 16, kLossR = 5, kLossMid = kLossTile + 2 * kLossR, kLossIn = kLossTile + 4 * kLossR;  // 16, 26, 36

// LDS planes, row strides multiples of four floats so that a thread reads the 14 inputs of FOUR adjacent outputs of an 11-tap pass
// as four 16-byte words (the first form read every tap as a float of its own: 80 k LDS reads per workgroup, 33 us for three
// 256 x 256 images): inputs 36 x 40 (two planes), first horizontal pass 36 x 28 (five planes), a / b / dmu 26 x 28 (three planes,
// over the inputs - dead by then, a thread keeps its own pixel's two values), second horizontal pass 26 x 16 (three planes, over
// the first one's).  31.7 KB: five workgroups per CU.
constexpr int kLossXS = 40, kLossHS = 28, kLossBS = 16;
__global__ __launch_bounds__(256) void k_image_loss(int H, int W, const float* __restrict__ pred, const float* __restrict__ target,
                                                    float mse_scale, float ssim_scale, float* __restrict__ grad, float* __restrict__ partials) {
  __shared__ __attribute__((aligned(16))) float sX[2 * kLossIn * kLossXS];
  __shared__ __attribute__((aligned(16))) float sH[5 * kLossIn * kLossHS];
  static_assert(3 * kLossMid * kLossHS <= 2 * kLossIn * kLossXS && 3 * kLossMid * kLossBS <= 5 * kLossIn * kLossHS, "aliased planes fit");
  float* const x1 = sX;
  float* const x2 = sX + kLossIn * kLossXS;
  auto hz = [&](int k, int r) { return sH + (k * kLossIn + r) * kLossHS; };   // x1, x2, x1^2, x2^2, x1 x2 after the horizontal pass
  auto mp = [&](int k, int r) { return sX + (k * kLossMid + r) * kLossHS; };  // a, b, dmu on the 26 x 26 region
  auto hb = [&](int k, int r) { return sH + (k * kLossMid + r) * kLossBS; };  // their horizontal pass
  __shared__ float red[3][4];
  const int tid = threadIdx.x, img_c = blockIdx.z;   // image * 3 + channel
  const int ox = blockIdx.x * kLossTile, oy = blockIdx.y * kLossTile;
  const float* p1 = pred + (size_t)img_c * H * W;
  const float* p2 = target + (size_t)img_c * H * W;
  // window: exp(-(k - 5)^2 / (2 sigma^2)) normalised, sigma = 1.5 (loss_multissim.py:50-52), as the reference computes it in fp32
  float wgt[11];
  {
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < 11; ++k) { wgt[k] = expf(-(float)((k - 5) * (k - 5)) / 4.5f); s += wgt[k]; }
#pragma unroll
    for (int k = 0; k < 11; ++k) wgt[k] /= s;
  }
  for (int e = tid; e < kLossIn * kLossXS; e += 256) {
    const int r = e / kLossXS, c = e - r * kLossXS, y = oy - 2 * kLossR + r, x = ox - 2 * kLossR + c;
    const bool in = c < kLossIn && x >= 0 && x < W && y >= 0 && y < H;
    x1[e] = in ? p1[(size_t)y * W + x] : 0.f;
    x2[e] = in ? p2[(size_t)y * W + x] : 0.f;
  }
  __syncthreads();
  // ---- horizontal pass of the five products: row r, output columns 4 j .. 4 j + 3 (columns 26, 27 are padding)
  if (tid < kLossIn * (kLossHS / 4)) {
    const int r = tid / (kLossHS / 4), j = tid - r * (kLossHS / 4);
    float a[16], b[16];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const float4 va = *reinterpret_cast<const float4*>(x1 + r * kLossXS + 4 * j + 4 * q);
      const float4 vb = *reinterpret_cast<const float4*>(x2 + r * kLossXS + 4 * j + 4 * q);
      a[4 * q] = va.x; a[4 * q + 1] = va.y; a[4 * q + 2] = va.z; a[4 * q + 3] = va.w;
      b[4 * q] = vb.x; b[4 * q + 1] = vb.y; b[4 * q + 2] = vb.z; b[4 * q + 3] = vb.w;
    }
    float o[5][4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      float s1 = 0, s2 = 0, s11 = 0, s22 = 0, s12 = 0;
#pragma unroll
      for (int k = 0; k < 11; ++k) {
        const float av = a[u + k], bv = b[u + k], w = wgt[k];
        s1 += w * av; s2 += w * bv; s11 += w * (av * av); s22 += w * (bv * bv); s12 += w * (av * bv);
      }
      o[0][u] = s1; o[1][u] = s2; o[2][u] = s11; o[3][u] = s22; o[4][u] = s12;
    }
#pragma unroll
    for (int k = 0; k < 5; ++k) *reinterpret_cast<float4*>(hz(k, r) + 4 * j) = make_float4(o[k][0], o[k][1], o[k][2], o[k][3]);
  }
  // this thread's own pixel of the tile (the last phase needs it; the inputs' planes are overwritten before)
  const float own1 = x1[(tid / kLossTile + 2 * kLossR) * kLossXS + tid % kLossTile + 2 * kLossR];
  const float own2 = x2[(tid / kLossTile + 2 * kLossR) * kLossXS + tid % kLossTile + 2 * kLossR];
  __syncthreads();
  // ---- vertical pass + the SSIM terms: column c, output rows 4 g .. 4 g + 3 (rows >= 26 do not exist)
  float sum_s = 0.f;
  constexpr float C1 = 0.01f * 0.01f, C2 = 0.03f * 0.03f;
  if (tid < ((kLossMid + 3) / 4) * kLossMid) {
    const int g = tid / kLossMid, c = tid - g * kLossMid;
    float acc[5][4];
#pragma unroll
    for (int k = 0; k < 5; ++k) {
      float col[14];
#pragma unroll
      for (int q = 0; q < 14; ++q) col[q] = hz(k, min(4 * g + q, kLossIn - 1))[c];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        float t = 0.f;
#pragma unroll
        for (int q = 0; q < 11; ++q) t += wgt[q] * col[u + q];
        acc[k][u] = t;
      }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int r = 4 * g + u, y = oy - kLossR + r, x = ox - kLossR + c;
      if (r >= kLossMid) continue;
      const float mu1 = acc[0][u], mu2 = acc[1][u], s11 = acc[2][u], s22 = acc[3][u], s12 = acc[4][u];
      float a = 0.f, b = 0.f, dmu = 0.f;
      if (x >= 0 && x < W && y >= 0 && y < H) {
        const float A = 2.f * mu1 * mu2 + C1, B = 2.f * (s12 - mu1 * mu2) + C2;
        const float C = mu1 * mu1 + mu2 * mu2 + C1, D = (s11 - mu1 * mu1) + (s22 - mu2 * mu2) + C2;
        const float iC = 1.f / C, iD = 1.f / D, AB = A * B;
        a = -AB * iC * iD * iD;
        b = 2.f * A * iC * iD;
        dmu = 2.f * mu2 * (B - A) * iC * iD - 2.f * mu1 * AB * iC * iC * iD + 2.f * mu1 * AB * iC * iD * iD;
        if (r >= kLossR && r < kLossR + kLossTile && c >= kLossR && c < kLossR + kLossTile) sum_s += AB * iC * iD;  // this tile's own pixels
      }
      mp(0, r)[c] = a; mp(1, r)[c] = b; mp(2, r)[c] = dmu;
    }
  }
  __syncthreads();
  // ---- horizontal pass of a, b, dmu: row r, output columns 4 j .. 4 j + 3 (hb lies over hz: dead since the barrier)
  if (tid < kLossMid * (kLossTile / 4)) {
    const int r = tid / (kLossTile / 4), j = tid - r * (kLossTile / 4);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      float v[16];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const float4 t = *reinterpret_cast<const float4*>(mp(k, r) + 4 * j + 4 * q);
        v[4 * q] = t.x; v[4 * q + 1] = t.y; v[4 * q + 2] = t.z; v[4 * q + 3] = t.w;
      }
      float o[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        float t = 0.f;
#pragma unroll
        for (int q = 0; q < 11; ++q) t += wgt[q] * v[u + q];
        o[u] = t;
      }
      *reinterpret_cast<float4*>(hb(k, r) + 4 * j) = make_float4(o[0], o[1], o[2], o[3]);
    }
  }
  __syncthreads();
  float sum_se = 0.f, sum_ce = 0.f;
  {
    const int r = tid / kLossTile, c = tid - r * kLossTile, y = oy + r, x = ox + c;
    if (x < W && y < H) {
      float wa = 0, wb = 0, wm = 0;
#pragma unroll
      for (int k = 0; k < 11; ++k) { const float w = wgt[k]; wa += w * hb(0, r + k)[c]; wb += w * hb(1, r + k)[c]; wm += w * hb(2, r + k)[c]; }
      const float v1 = own1, v2 = own2;
      const float d = v1 - v2;
      sum_se = d * d;
      const float dc = fminf(fmaxf(v2, 0.f), 1.f) - fminf(fmaxf(v1, 0.f), 1.f);
      sum_ce = dc * dc;
      if (grad) grad[(size_t)img_c * H * W + (size_t)y * W + x] = mse_scale * 2.f * d - ssim_scale * (wm + 2.f * v1 * wa + v2 * wb);
    }
  }
  sum_se = wave_sum(sum_se); sum_ce = wave_sum(sum_ce); sum_s = wave_sum(sum_s);
  if ((tid & 63) == 0) { red[0][tid >> 6] = sum_se; red[1][tid >> 6] = sum_ce; red[2][tid >> 6] = sum_s; }
  __syncthreads();
  if (tid < 3) {
    const size_t slot = ((size_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
    partials[slot * 4 + tid] = red[tid][0] + red[tid][1] + red[tid][2] + red[tid][3];
    if (tid == 0) partials[slot * 4 + 3] = 0.f;
  }
}

// The slots of k_image_loss added up in a fixed order by ONE workgroup (a few thousand slots: a 256 x 256 image has 768): per image
// (sums[i][0..3]: squared error, clipped squared error, SSIM map, 0) and over the batch -> totals[0..2] = loss, mean squared
// error, mean SSIM.  No atomics, nothing between workgroups: the result is the same bits every time.
__global__ __launch_bounds__(1024) void k_image_loss_finish(int slots_per_image, int num_images, const float* __restrict__ partials,
                                                            float mse_weight, float ssim_weight, float inv_count, float* __restrict__ sums,
                                                            float* __restrict__ totals) {
  __shared__ float red[3][16];
  const int tid = threadIdx.x;
  float se = 0.f, sm = 0.f;
  for (int img = 0; img < num_images; ++img) {
    const float* ps = partials + (size_t)img * slots_per_image * 4;
    float a0 = 0.f, a1 = 0.f, a2 = 0.f;
    for (int k = tid; k < slots_per_image; k += 1024) {
      const float4 v = *reinterpret_cast<const float4*>(ps + 4 * k);
      a0 += v.x; a1 += v.y; a2 += v.z;
    }
    a0 = wave_sum(a0); a1 = wave_sum(a1); a2 = wave_sum(a2);
    if ((tid & 63) == 0) { red[0][tid >> 6] = a0; red[1][tid >> 6] = a1; red[2][tid >> 6] = a2; }
    __syncthreads();
    if (tid == 0) {
      float t[3];
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        float x = 0.f;
#pragma unroll
        for (int q = 0; q < 16; ++q) x += red[c][q];
        t[c] = x;
        sums[img * 4 + c] = x;
      }
      sums[img * 4 + 3] = 0.f;
      se += t[0]; sm += t[2];
    }
    __syncthreads();
  }
  if (tid == 0) {
    const float mse = se * inv_count, ssim = sm * inv_count;
    totals[0] = mse_weight * mse + ssim_weight * (1.f - ssim);
    totals[1] = mse;
    totals[2] = ssim;
    totals[3] = 0.f;
  }
}

// ------------------------------------------------------------------------------------------------
// Evaluation metrics (reference src/evaluation/metrics.py:11-19 compute_psnr and :36-52 compute_ssim): the SSIM there is
// skimage.metrics.structural_similarity(gt, hat, win_size=11, gaussian_weights=True, channel_axis=0, data_range=1.0) per image,
// NOT the loss's SSIM above.  Same window (11 taps, sigma 1.5, separable), but: the image is extended by reflection about its
// edge (index -1 - j reads j, H + j reads H - 1 - j; scipy's mode="reflect") instead of zeros; the covariances are the sample ones,
// cn = 121 / 120 times the population ones; the map S = (2 ux uy + C1)(2 vxy + C2) / ((ux^2 + uy^2 + C1)(vx + vy + C2)) is averaged
// over the interior 5 <= row < H - 5, 5 <= col < W - 5 of each channel, and an image's value is the mean of its three channels'.
// Forward only: one workgroup = one 16 x 16 tile of one channel of one image; both images on the 26 x 26 halo region through the
// reflected index -> the five products' horizontal 11-tap pass on 26 x 16 -> the vertical pass, S and the tile's interior sum by the
// first wave.  Slots as k_image_loss writes them: squared error, squared error of the inputs clipped to [0, 1], sum of S over the
// tile's interior pixels, 0.
// LDS: inputs 26 rows x 48 floats (a 16-lane group of the 16-byte reads covers rows r, r + 3, r + 5, r + 6 or r + 1, r + 2,
// r + 4, r + 7, four lanes and 16 floats each: at 48 floats a row those start 0, 16, 48, 32 or 48, 32, 0, 16 floats into the 64
// banks - no conflict; at 28 they would overlap); horizontal pass 26 rows x 20 floats (a 32-lane half of the column reads is two
// row groups, 4 x 20 = 80 floats = 16 banks of 32 apart).  20.4 KB and 88 VGPRs: five workgroups per CU, by the registers.
// ------------------------------------------------------------------------------------------------
constexpr int kMetXS = 48, kMetHS = 20;
__global__ __launch_bounds__(256) void k_image_metrics(int H, int W, const float* __restrict__ truth, const float* __restrict__ pred,
                                                       float* __restrict__ smap, float* __restrict__ partials) {
  __shared__ __attribute__((aligned(16))) float sX[2 * kLossMid * kMetXS];
  __shared__ __attribute__((aligned(16))) float sH[5 * kLossMid * kMetHS];
  static_assert(kMetXS % 4 == 0 && kMetHS % 4 == 0 && kMetXS >= kLossMid + 2 && kMetHS >= kLossTile, "16-byte rows");
  float* const x1 = sX;
  float* const x2 = sX + kLossMid * kMetXS;
  auto hz = [&](int k, int r) { return sH + (k * kLossMid + r) * kMetHS; };  // x, y, x^2, y^2, x y after the horizontal pass
  __shared__ float red[3][4];
  const int tid = threadIdx.x, img_c = blockIdx.z;  // image * 3 + channel
  const int ox = blockIdx.x * kLossTile, oy = blockIdx.y * kLossTile;
  const float* p1 = truth + (size_t)img_c * H * W;
  const float* p2 = pred + (size_t)img_c * H * W;
  float wgt[11];  // the window of k_image_loss
  {
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < 11; ++k) { wgt[k] = expf(-(float)((k - 5) * (k - 5)) / 4.5f); s += wgt[k]; }
#pragma unroll
    for (int k = 0; k < 11; ++k) wgt[k] /= s;
  }
  // Both images are staged minus ONE number, the ground truth at the tile's centre: the variances and the covariance do not
  // depend on it, and where the image is nearly constant around the tile (rendered backgrounds) uxx - ux^2 no longer cancels
  // seven digits against C2 = 9e-4 - the float32 rounding that costs the unshifted form 1e-4 per pixel of S there.
  const float shift = p1[(size_t)min(oy + kLossTile / 2, H - 1) * W + min(ox + kLossTile / 2, W - 1)];
  // Rows of 28: columns 26, 27 are read by the 16-byte loads and never used.  One reflection lands inside the image for every tap
  // of a pixel inside it (H, W >= 11); the taps of the tile's pixels beyond the image's edge may not, hence the clamp.
  for (int e = tid; e < kLossMid * (kLossMid + 2); e += 256) {
    const int r = e / (kLossMid + 2), c = e - r * (kLossMid + 2);
    int y = oy - kLossR + r, x = ox - kLossR + c;
    y = y < 0 ? -1 - y : (y >= H ? 2 * H - 1 - y : y);
    x = x < 0 ? -1 - x : (x >= W ? 2 * W - 1 - x : x);
    y = min(max(y, 0), H - 1);
    x = min(max(x, 0), W - 1);
    const bool in = c < kLossMid;
    x1[r * kMetXS + c] = in ? p1[(size_t)y * W + x] - shift : 0.f;
    x2[r * kMetXS + c] = in ? p2[(size_t)y * W + x] - shift : 0.f;
  }
  __syncthreads();
  // ---- horizontal pass of the five products: row r, output columns 4 j .. 4 j + 3
  if (tid < kLossMid * (kLossTile / 4)) {
    const int r = tid / (kLossTile / 4), j = tid - r * (kLossTile / 4);
    float a[16], b[16];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const float4 va = *reinterpret_cast<const float4*>(x1 + r * kMetXS + 4 * j + 4 * q);
      const float4 vb = *reinterpret_cast<const float4*>(x2 + r * kMetXS + 4 * j + 4 * q);
      a[4 * q] = va.x; a[4 * q + 1] = va.y; a[4 * q + 2] = va.z; a[4 * q + 3] = va.w;
      b[4 * q] = vb.x; b[4 * q + 1] = vb.y; b[4 * q + 2] = vb.z; b[4 * q + 3] = vb.w;
    }
    float o[5][4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      float s1 = 0, s2 = 0, s11 = 0, s22 = 0, s12 = 0;
#pragma unroll
      for (int k = 0; k < 11; ++k) {
        const float av = a[u + k], bv = b[u + k], w = wgt[k];
        s1 += w * av; s2 += w * bv; s11 += w * (av * av); s22 += w * (bv * bv); s12 += w * (av * bv);
      }
      o[0][u] = s1; o[1][u] = s2; o[2][u] = s11; o[3][u] = s22; o[4][u] = s12;
    }
#pragma unroll
    for (int k = 0; k < 5; ++k) *reinterpret_cast<float4*>(hz(k, r) + 4 * j) = make_float4(o[k][0], o[k][1], o[k][2], o[k][3]);
  }
  // ---- the two squared errors of this thread's own pixel
  float sum_se = 0.f, sum_ce = 0.f;
  {
    const int r = tid / kLossTile, c = tid - r * kLossTile;
    if (ox + c < W && oy + r < H) {  // (from memory, not from the shifted planes: the same bits as k_image_loss's)
      const float v1 = p1[(size_t)(oy + r) * W + ox + c], v2 = p2[(size_t)(oy + r) * W + ox + c];
      const float d = v1 - v2;
      sum_se = d * d;
      const float dc = fminf(fmaxf(v2, 0.f), 1.f) - fminf(fmaxf(v1, 0.f), 1.f);
      sum_ce = dc * dc;
    }
  }
  __syncthreads();
  // ---- vertical pass + S: column c, output rows 4 g .. 4 g + 3 of the tile (the first wave)
  float sum_s = 0.f;
  if (tid < kLossTile * (kLossTile / 4)) {
    constexpr float C1 = 0.01f * 0.01f, C2 = 0.03f * 0.03f, cn = 121.f / 120.f;
    const int g = tid / kLossTile, c = tid - g * kLossTile;
    float acc[5][4];
#pragma unroll
    for (int k = 0; k < 5; ++k) {
      float col[14];
#pragma unroll
      for (int q = 0; q < 14; ++q) col[q] = hz(k, 4 * g + q)[c];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        float t = 0.f;
#pragma unroll
        for (int q = 0; q < 11; ++q) t += wgt[q] * col[u + q];
        acc[k][u] = t;
      }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int y = oy + 4 * g + u, x = ox + c;
      if (x >= W || y >= H) continue;
      const float sx = acc[0][u], sy = acc[1][u], ux = sx + shift, uy = sy + shift;
      const float vx = cn * (acc[2][u] - sx * sx), vy = cn * (acc[3][u] - sy * sy), vxy = cn * (acc[4][u] - sx * sy);
      const float S = ((2.f * ux * uy + C1) * (2.f * vxy + C2)) / ((ux * ux + uy * uy + C1) * (vx + vy + C2));
      if (smap) smap[((size_t)img_c * H + y) * W + x] = S;
      if (y >= kLossR && y < H - kLossR && x >= kLossR && x < W - kLossR) sum_s += S;
    }
  }
  sum_se = wave_sum(sum_se); sum_ce = wave_sum(sum_ce); sum_s = wave_sum(sum_s);
  if ((tid & 63) == 0) { red[0][tid >> 6] = sum_se; red[1][tid >> 6] = sum_ce; red[2][tid >> 6] = sum_s; }
  __syncthreads();
  if (tid < 3) {
    const size_t slot = ((size_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
    partials[slot * 4 + tid] = red[tid][0] + red[tid][1] + red[tid][2] + red[tid][3];
    if (tid == 0) partials[slot * 4 + 3] = 0.f;
  }
}

// The slots of k_image_metrics added up as k_image_loss_finish adds them (one workgroup, fixed order, an image's sums independent
// of the other images) and finished: metrics (4, num_images) = SSIM (the interior sum / interior_count), PSNR
// (-10 log10(clipped squared error / pixel_count), +inf for equal images), the interior sum of S, the clipped squared error.
__global__ __launch_bounds__(1024) void k_image_metrics_finish(int slots_per_image, int num_images, const float* __restrict__ partials,
                                                               float interior_count, float pixel_count, float* __restrict__ metrics) {
  __shared__ float red[2][16];
  const int tid = threadIdx.x;
  for (int img = 0; img < num_images; ++img) {
    const float* ps = partials + (size_t)img * slots_per_image * 4;
    float a1 = 0.f, a2 = 0.f;
    for (int k = tid; k < slots_per_image; k += 1024) {
      const float4 v = *reinterpret_cast<const float4*>(ps + 4 * k);
      a1 += v.y; a2 += v.z;
    }
    a1 = wave_sum(a1); a2 = wave_sum(a2);
    if ((tid & 63) == 0) { red[0][tid >> 6] = a1; red[1][tid >> 6] = a2; }
    __syncthreads();
    if (tid == 0) {
      float ce = 0.f, s = 0.f;
#pragma unroll
      for (int q = 0; q < 16; ++q) { ce += red[0][q]; s += red[1][q]; }
      metrics[img] = s / interior_count;
      metrics[num_images + img] = -10.f * log10f(ce / pixel_count);
      metrics[2 * (size_t)num_images + img] = s;
      metrics[3 * (size_t)num_images + img] = ce;
    }
    __syncthreads();
  }
}
}  // namespace gsr

extern "C" {

size_t gsr_image_loss_partials(int num_images, int height, int width) {
  if (num_images <= 0 || height <= 0 || width <= 0) return 0;
  return (size_t)num_images * 3 * ((height + gsr::kLossTile - 1) / gsr::kLossTile) * ((width + gsr::kLossTile - 1) / gsr::kLossTile);
}

int gsr_image_loss(int num_images, int height, int width, const float* prediction, const float* target, float mse_weight,
                   float ssim_weight, float* dL_dprediction, float* partials, void* stream_) {
  if (num_images < 0 || height <= 0 || width <= 0) return GSR_ERR_INVALID_ARGUMENT;
  if (num_images == 0) return GSR_OK;
  if (!prediction || !target || !partials || (size_t)num_images * 3 > 65535) return GSR_ERR_INVALID_ARGUMENT;
  const double count = (double)num_images * 3.0 * height * width;  // both reference losses average over every element
  const dim3 grid((unsigned)((width + gsr::kLossTile - 1) / gsr::kLossTile), (unsigned)((height + gsr::kLossTile - 1) / gsr::kLossTile),
                  (unsigned)num_images * 3u);
  hipLaunchKernelGGL(gsr::k_image_loss, grid, dim3(256), 0, static_cast<hipStream_t>(stream_), height, width, prediction, target,
                     (float)(mse_weight / count), (float)(ssim_weight / count), dL_dprediction, partials);
  GSR_CHECK(hipGetLastError());
  return GSR_OK;
}

int gsr_image_loss_finish(int num_images, int height, int width, const float* partials, float mse_weight, float ssim_weight,
                          float* sums, float* totals, void* stream_) {
  if (num_images <= 0 || height <= 0 || width <= 0 || !partials || !sums || !totals) return GSR_ERR_INVALID_ARGUMENT;
  const int slots = (int)(gsr_image_loss_partials(num_images, height, width) / (size_t)num_images);
  const double count = (double)num_images * 3.0 * height * width;
  hipLaunchKernelGGL(gsr::k_image_loss_finish, dim3(1), dim3(1024), 0, static_cast<hipStream_t>(stream_), slots, num_images,
                     partials, mse_weight, ssim_weight, (float)(1.0 / count), sums, totals);
  GSR_CHECK(hipGetLastError());
  return GSR_OK;
}

size_t gsr_image_metrics_partials(int num_images, int height, int width) {
  if (num_images <= 0 || height < 2 * gsr::kLossR + 1 || width < 2 * gsr::kLossR + 1 || (size_t)num_images * 3 > 65535) return 0;
  return gsr_image_loss_partials(num_images, height, width);
}

int gsr_image_metrics(int num_images, int height, int width, const float* ground_truth, const float* prediction, float* ssim_map,
                      float* partials, void* stream_) {
  if (num_images < 0 || height < 2 * gsr::kLossR + 1 || width < 2 * gsr::kLossR + 1) return GSR_ERR_INVALID_ARGUMENT;
  if (num_images == 0) return GSR_OK;
  if (!ground_truth || !prediction || !partials || (size_t)num_images * 3 > 65535) return GSR_ERR_INVALID_ARGUMENT;
  const dim3 grid((unsigned)((width + gsr::kLossTile - 1) / gsr::kLossTile), (unsigned)((height + gsr::kLossTile - 1) / gsr::kLossTile),
                  (unsigned)num_images * 3u);
  hipLaunchKernelGGL(gsr::k_image_metrics, grid, dim3(256), 0, static_cast<hipStream_t>(stream_), height, width, ground_truth,
                     prediction, ssim_map, partials);
  GSR_CHECK(hipGetLastError());
  return GSR_OK;
}

int gsr_image_metrics_finish(int num_images, int height, int width, const float* partials, float* metrics, void* stream_) {
  const size_t total = gsr_image_metrics_partials(num_images, height, width);
  if (total == 0 || !partials || !metrics) return GSR_ERR_INVALID_ARGUMENT;
  const double interior = 3.0 * (height - 2 * gsr::kLossR) * (double)(width - 2 * gsr::kLossR);
  hipLaunchKernelGGL(gsr::k_image_metrics_finish, dim3(1), dim3(1024), 0, static_cast<hipStream_t>(stream_),
                     (int)(total / (size_t)num_images), num_images, partials, (float)interior, (float)(3.0 * height * width), metrics);
  GSR_CHECK(hipGetLastError());
  return GSR_OK;
}

}  // extern "C"
