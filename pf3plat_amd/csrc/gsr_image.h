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

// ------------------------------------------------------------------------------------------------
// The perceptual distance's head (lpips.LPIPS(net="vgg") after its convolutions; definition: include/gsr.h): per layer the two
// feature maps normalised along their channels, the weighted squared difference, the spatial mean - and its gradient.  Purely
// memory-bound: 64 MB per 256 x 256 image pair, read ONCE in either direction.
// A unit of work = (layer, image, run of P consecutive pixels) = one workgroup of 256 threads, thread = (channel group g, pixel p),
// tid = g P + p: lanes run along consecutive pixels (a wave-instruction reads 64 / min(P, 64) channels' runs of min(P, 64) floats
// each), the channel stride is h w.  The layer's C channels are dealt over G = 256 / P groups, channel s G + g in slot s of group g;
// G is the smallest power of two that leaves a thread at most kLpSlots = 64 channels: C <= 64 -> one group, runs of 256 pixels;
// C = 512 -> 8 groups, runs of 32 (128-byte rows); C = 1024 -> 16 groups, runs of 16.  A thread holds its slots of a, b AND the
// weights in registers (192 of them: the arrays are indexed by unrolled loops only), so the two trips over the channels the
// definition forces - the norms, then the differences a^_c - b^_c - and the gradient's third read memory once; every load of a
// unit is issued before the first is used (up to 128 KB of features in flight per CU - what one workgroup per CU needs to keep the
// memory busy).  Channel sums across the groups go through LDS and are added by every thread of a pixel in group order; a unit's
// value by a wave butterfly and four LDS words; one float per workgroup leaves, and lpips_finish adds an image's slots in a fixed
// order, a wave per image: no atomics, the same bits on every call, an image's value independent of the batch around it.
// The gradient recomputes everything from the same registers, in the projection form given at its code, and stores dL/da, dL/db
// (either optional per layer) at the addresses it read; a vector with r = 0 stores exact zeros (the stated departure from
// autograd's NaN).
// These are routines of k_pose_ops (gsr_pose_refine.h gives the reason: a kernel of its own would move .text), op kPoseOpLpips; its
// registers - one workgroup per CU - are what the register-resident unit wants anyway.  Loads are one dword per lane: 16-byte loads
// would need h w a multiple of four and a second path for every other size (not built).
// ------------------------------------------------------------------------------------------------
namespace gsr {
constexpr int kLpSlots = 64;        // channels a thread holds
constexpr int kLpThreads = 256;     // = kRefineThreads (static_assert next to the kernel)
constexpr int kLpMaxChannels = 1024;
constexpr uint32_t kLpMaxUnits = 0xffffffffu / kLpThreads;  // a launch takes at most 2^32 - 1 threads: 16 777 215 workgroups of 256
constexpr float kLpEps = 1e-10f;
enum { kLpForward = 0, kLpFinish = 1, kLpBackward = 2 };

struct LpLayer {
  const float *a, *b, *w;
  float *da, *db;     // backward: either may be null
  int C, hw;
  int lg;             // log2 of the channel groups G; P = 256 >> lg pixels per unit
  uint32_t upi, base; // units per image; the layer's first unit
  float inv_hw;
};
struct LpipsArgs {
  int op, N, L;
  LpLayer layer[GSR_LPIPS_MAX_LAYERS];
  const float* g;        // backward: (N)
  float* partials;       // forward: one float per unit; finish reads them
  float *values, *per_layer;
};

__host__ __device__ inline int lp_log_groups(int C) {
  int lg = 0;
  while (((C + (1 << lg) - 1) >> lg) > kLpSlots) ++lg;
  return lg;
}

// the layer of unit u and the unit's place in it (uniform over the workgroup; selects, so that the table stays in scalar registers)
__device__ __forceinline__ LpLayer lp_layer_of(const LpipsArgs& A, uint32_t u) {
  LpLayer y = A.layer[0];
#pragma unroll
  for (int l = 1; l < GSR_LPIPS_MAX_LAYERS; ++l)
    if (l < A.L && u >= A.layer[l].base) y = A.layer[l];
  return y;
}

template <bool kBackward>
__device__ __forceinline__ void lpips_unit(const LpipsArgs& A, float* lds) {
  const int tid = threadIdx.x;
  const uint32_t u = blockIdx.x;
  const LpLayer y = lp_layer_of(A, u);
  const uint32_t local = u - y.base, img = local / y.upi, run = local - img * y.upi;
  const int G = 1 << y.lg, P = kLpThreads >> y.lg;
  const int g = tid >> (8 - y.lg), p = tid & (P - 1);
  const int64_t pix = (int64_t)run * P + p;
  const bool valid = pix < (int64_t)y.hw;
  const int C = y.C;
  const size_t hw = (size_t)y.hw, off = ((size_t)img * C + g) * hw + (size_t)(valid ? pix : 0), step = (size_t)G * hw;
  const float* pa = y.a + off;
  const float* pb = y.b + off;
  const bool want_a = kBackward && y.da != nullptr, want_b = kBackward && y.db != nullptr;
  if (kBackward && !want_a && !want_b) return;  // (uniform: before any barrier)
  float va[kLpSlots], vb[kLpSlots], vw[kLpSlots];
  // every load of the unit, before anything is used; blocks of 8 slots past the layer's channels are skipped by a uniform branch
#pragma unroll
  for (int sb = 0; sb < kLpSlots / 8; ++sb) {
    if ((sb * 8) * G < C) {
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const int s = sb * 8 + k, c = s * G + g;
        const bool ok = valid && c < C;
        va[s] = ok ? pa[(size_t)s * step] : 0.f;
        vb[s] = ok ? pb[(size_t)s * step] : 0.f;
        vw[s] = c < C ? y.w[c] : 0.f;
      }
    } else {
#pragma unroll
      for (int k = 0; k < 8; ++k) { va[sb * 8 + k] = 0.f; vb[sb * 8 + k] = 0.f; vw[sb * 8 + k] = 0.f; }
    }
  }
  // ---- first trip: the squared norms, this thread's slots in order, then the groups of the pixel in order
  float sa = 0.f, sb2 = 0.f;
#pragma unroll
  for (int sb = 0; sb < kLpSlots / 8; ++sb) {
    if ((sb * 8) * G < C) {
#pragma unroll
      for (int k = 0; k < 8; ++k) { const int s = sb * 8 + k; sa += va[s] * va[s]; sb2 += vb[s] * vb[s]; }
    }
  }
  float* const la = lds;                    // four arrays of kLpThreads floats
  float* const lb = lds + kLpThreads;
  float* const ls = lds + 2 * kLpThreads;
  float* const lt = lds + 3 * kLpThreads;
  la[tid] = sa; lb[tid] = sb2;
  __syncthreads();
  float ra2 = 0.f, rb2 = 0.f;
  for (int q = 0; q < G; ++q) { ra2 += la[q * P + p]; rb2 += lb[q * P + p]; }
  const float ra = sqrtf(ra2), rb = sqrtf(rb2), na = ra + kLpEps, nb = rb + kLpEps;
  const float ia = 1.f / na, ib = 1.f / nb;
  if (!kBackward) {
    // ---- second trip: the weighted squared differences of the normalised vectors
    float t = 0.f;
#pragma unroll
    for (int sb = 0; sb < kLpSlots / 8; ++sb) {
      if ((sb * 8) * G < C) {
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          const int s = sb * 8 + k;
          const float d = va[s] * ia - vb[s] * ib;
          t += vw[s] * (d * d);
        }
      }
    }
    t = wave_sum(t);
    if ((tid & 63) == 0) ls[tid >> 6] = t;
    __syncthreads();
    if (tid == 0) A.partials[u] = ((ls[0] + ls[1]) + ls[2]) + ls[3];
  } else {
    // The gradient in its projection form.  With t = a / r_a (a unit vector), q = sum_c u_c t_c and r_a / n_a = 1 - eps / n_a,
    //   dL/da_c = u_c / n_a - a_c s / (r_a n_a^2) = (u_c - t_c q) / n_a + t_c q eps / n_a^2,   u_c = k w_c (a^_c - b^_c), k = 2 g_n / (h w):
    // the first form subtracts two terms that agree to eps / n_a when u is parallel to a (always at C = 1, where float32 then returns
    // noise 1e3 times the gradient); the second cancels exactly there - t = a / r_a by IEEE division is +-1 at C = 1 - and leaves the
    // eps term.  dL/db the same with the sign of u flipped.  The sides that want no gradient skip their divisions (uniform).
    const bool za = ra == 0.f, zb = rb == 0.f;
    float rho_a = ia, rho_b = ib;  // a^_c = va rho_a, whether va holds a_c or t_c
    if (want_a) {
      rho_a = ra * ia;
#pragma unroll
      for (int sb = 0; sb < kLpSlots / 8; ++sb) {
        if ((sb * 8) * G < C) {
#pragma unroll
          for (int k = 0; k < 8; ++k) va[sb * 8 + k] = za ? 0.f : va[sb * 8 + k] / ra;
        }
      }
    }
    if (want_b) {
      rho_b = rb * ib;
#pragma unroll
      for (int sb = 0; sb < kLpSlots / 8; ++sb) {
        if ((sb * 8) * G < C) {
#pragma unroll
          for (int k = 0; k < 8; ++k) vb[sb * 8 + k] = zb ? 0.f : vb[sb * 8 + k] / rb;
        }
      }
    }
    // ---- second trip: q_a = sum_c u_c ta_c, q_b = sum_c u_c tb_c
    const float kk = 2.f * A.g[img] * y.inv_hw;
    float ta = 0.f, tb = 0.f;
#pragma unroll
    for (int sb = 0; sb < kLpSlots / 8; ++sb) {
      if ((sb * 8) * G < C) {
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          const int s = sb * 8 + k;
          const float uc = kk * vw[s] * (va[s] * rho_a - vb[s] * rho_b);
          ta += uc * va[s]; tb += uc * vb[s];
        }
      }
    }
    ls[tid] = ta; lt[tid] = tb;
    __syncthreads();
    float q_a = 0.f, q_b = 0.f;
    for (int q = 0; q < G; ++q) { q_a += ls[q * P + p]; q_b += lt[q * P + p]; }
    const float e_a = q_a * (kLpEps * ia) * ia, e_b = q_b * (kLpEps * ib) * ib;
    // ---- third trip: the stores; an all-zero vector: exact zeros
    float* const qa = want_a ? y.da + off : nullptr;
    float* const qb = want_b ? y.db + off : nullptr;
#pragma unroll
    for (int sb = 0; sb < kLpSlots / 8; ++sb) {
      if ((sb * 8) * G < C) {
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          const int s = sb * 8 + k, c = s * G + g;
          if (valid && c < C) {
            const float uc = kk * vw[s] * (va[s] * rho_a - vb[s] * rho_b);
            if (want_a) qa[(size_t)s * step] = za ? 0.f : (uc - va[s] * q_a) * ia + va[s] * e_a;
            if (want_b) qb[(size_t)s * step] = zb ? 0.f : (vb[s] * q_b - uc) * ib - vb[s] * e_b;
          }
        }
      }
    }
  }
}

// One workgroup: wave v takes the images v, v + 4, ...; per layer the image's slots lane by lane in steps of 64, a butterfly, the
// layer's 1 / (h w); the value is the layers' sum in layer order.
__device__ __forceinline__ void lpips_finish(const LpipsArgs& A) {
  const int lane = threadIdx.x & 63;
  for (int n = threadIdx.x >> 6; n < A.N; n += kLpThreads / 64) {
    float value = 0.f;
#pragma unroll
    for (int l = 0; l < GSR_LPIPS_MAX_LAYERS; ++l) {
      float d = 0.f;
      if (l < A.L) {
        const LpLayer& y = A.layer[l];
        const float* ps = A.partials + y.base + (size_t)n * y.upi;
        float t = 0.f;
        for (uint32_t k = lane; k < y.upi; k += 64) t += ps[k];
        d = wave_sum(t) * y.inv_hw;
        value += d;
      }
      if (lane == 0) A.per_layer[(size_t)n * GSR_LPIPS_MAX_LAYERS + l] = d;
    }
    if (lane == 0) A.values[n] = value;
  }
}

__device__ __forceinline__ void k_lpips_ops(const LpipsArgs& A, float* lds) {
  if (A.op == kLpForward) lpips_unit<false>(A, lds);
  else if (A.op == kLpBackward) lpips_unit<true>(A, lds);
  else lpips_finish(A);
}

static int lpips_op_launch(const LpipsArgs& a, unsigned blocks, void* stream_);  // (gsr_pose_refine.h, next to the kernel)

// The table as the kernels take it; false for what the launch refuses.  *units: the workgroups of the forward and the backward.
static bool lpips_table(int N, const GsrLpipsLayers& t, LpipsArgs* out, uint64_t* units) {
  if (N < 1 || t.num_layers < 1 || t.num_layers > GSR_LPIPS_MAX_LAYERS) return false;
  LpipsArgs A{};
  A.N = N; A.L = t.num_layers;
  uint64_t base = 0;
  for (int l = 0; l < t.num_layers; ++l) {
    const GsrLpipsLayer& s = t.layer[l];
    if (s.channels < 1 || s.channels > kLpMaxChannels || s.height < 1 || s.width < 1) return false;
    const int64_t hw = (int64_t)s.height * s.width;
    if (hw > 0x7fffffffll) return false;
    LpLayer& y = A.layer[l];
    y.a = s.a; y.b = s.b; y.w = s.weight;
    y.C = s.channels; y.hw = (int)hw;
    y.lg = lp_log_groups(s.channels);
    const int64_t P = kLpThreads >> y.lg;
    y.upi = (uint32_t)((hw + P - 1) / P);
    y.base = (uint32_t)base;
    y.inv_hw = (float)(1.0 / (double)hw);
    base += (uint64_t)y.upi * (uint64_t)N;
    if (base > (uint64_t)kLpMaxUnits) return false;
  }
  *out = A;
  *units = base;
  return true;
}

}  // namespace gsr

extern "C" {

int gsr_lpips_head_channel_slots(void) { return gsr::kLpSlots; }

int gsr_lpips_head_pixel_run(int channels) {
  if (channels < 1 || channels > gsr::kLpMaxChannels) return 0;
  return gsr::kLpThreads >> gsr::lp_log_groups(channels);
}

size_t gsr_lpips_head_partials(int num_images, GsrLpipsLayers layers) {
  gsr::LpipsArgs A;
  uint64_t units = 0;
  return gsr::lpips_table(num_images, layers, &A, &units) ? (size_t)units : 0;
}

int gsr_lpips_head(int num_images, GsrLpipsLayers layers, float* partials, void* stream_) {
  gsr::LpipsArgs A;
  uint64_t units = 0;
  if (!gsr::lpips_table(num_images, layers, &A, &units) || !partials) return GSR_ERR_INVALID_ARGUMENT;
  for (int l = 0; l < A.L; ++l)
    if (!A.layer[l].a || !A.layer[l].b || !A.layer[l].w) return GSR_ERR_INVALID_ARGUMENT;
  A.op = gsr::kLpForward;
  A.partials = partials;
  return gsr::lpips_op_launch(A, (unsigned)units, stream_);
}

int gsr_lpips_head_finish(int num_images, GsrLpipsLayers layers, const float* partials, float* values, float* per_layer, void* stream_) {
  gsr::LpipsArgs A;
  uint64_t units = 0;
  if (!gsr::lpips_table(num_images, layers, &A, &units) || !partials || !values || !per_layer) return GSR_ERR_INVALID_ARGUMENT;
  A.op = gsr::kLpFinish;
  A.partials = const_cast<float*>(partials);
  A.values = values; A.per_layer = per_layer;
  return gsr::lpips_op_launch(A, 1u, stream_);
}

int gsr_lpips_head_backward(int num_images, GsrLpipsLayers layers, const float* g, float* const* dL_da, float* const* dL_db, void* stream_) {
  gsr::LpipsArgs A;
  uint64_t units = 0;
  if (!gsr::lpips_table(num_images, layers, &A, &units) || !g) return GSR_ERR_INVALID_ARGUMENT;
  bool any = false;
  for (int l = 0; l < A.L; ++l) {
    if (!A.layer[l].a || !A.layer[l].b || !A.layer[l].w) return GSR_ERR_INVALID_ARGUMENT;
    A.layer[l].da = dL_da ? dL_da[l] : nullptr;
    A.layer[l].db = dL_db ? dL_db[l] : nullptr;
    any = any || A.layer[l].da || A.layer[l].db;
  }
  if (!any) return GSR_OK;
  A.op = gsr::kLpBackward;
  A.g = g;
  return gsr::lpips_op_launch(A, (unsigned)units, stream_);
}

}  // extern "C"
