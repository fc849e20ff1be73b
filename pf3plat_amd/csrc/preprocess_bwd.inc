// The text of k_preprocess_bwd, included twice by gsr_hip.hip (inside namespace gsr, where its comments are):
//   GSR_PBWD_KERNEL k_preprocess_bwd,     GSR_PBWD_UNIT 0 - every mode but the deterministic one; its instances are the code they were
//   GSR_PBWD_KERNEL k_preprocess_bwd_det, GSR_PBWD_UNIT 1 - GSR_FLAG_DETERMINISTIC: the rows are fixed-point sums in units of their view's
//                                                          largest cotangent (det_max_words) and are read back through 2^-e of that view
// (a shared __device__ body was tried first: inlined into the kernel it did not compile to the instructions of the kernel it came from)
template <int kPose, bool kJ, bool kShFrame = false>
__global__ __launch_bounds__(64) void GSR_PBWD_KERNEL(const Params p) {
  constexpr bool kCam = kPose == 1 || kPose == 3;                 // the whole camera gradient (kPose == 3: with the two tan-fov columns)
  constexpr int kRow = kPose == 3 ? kPoseFovFloats : kPoseFloats;  // floats of a partial row
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int lane = threadIdx.x, set = blockIdx.y;
  const int N = p.d.num_gaussians, Vs = p.d.views_per_set;
  const int g0 = blockIdx.x * 64;
  const int i = g0 + lane;
  const bool in_range = i < N;
  const size_t gi = (size_t)set * N + (in_range ? i : 0);
  const Grid& g = p.g;
  const int M = p.d.sh_coeffs;
  const int rowf = 3 * M, ldstride = rowf | 1;
  const int cnt = min(64, N - g0);
  // One LDS buffer of 64 SH rows: it holds the coefficients while the views are walked (the mean gradient needs them),
  // then each lane zeroes its own row and a second, cheap walk over the views accumulates dL/dsh into it (rows are
  // private to their lane, so no barrier is needed in between) before the cooperative store.  Half the LDS of an
  // in + out pair => twice the resident waves for this latency-bound kernel.
  float* sh_in = lds;
  const bool dbg = GSR_ABL(p.d.flags, GSR_FLAG_DEBUG_TIMING) && p.dL_dmeans2D != nullptr;
  unsigned long long stamps[5] = {0, 0, 0, 0, 0};
  if (dbg) stamps[0] = __builtin_amdgcn_s_memrealtime();
  // this lane's own inputs are requested before the (long) SH staging so that one memory latency covers both
  float rmx = 0, rmy = 0, rmz = 0, rcov[6] = {0, 0, 0, 0, 0, 0};
#if GSR_PBWD_UNIT
  const bool det = true;
#else
  const bool det = (p.d.flags & GSR_FLAG_DETERMINISTIC) != 0;
#endif
  auto load_row = [&](int vv, float (&sg)[12]) {  // screen-space gradient row of (view, Gaussian): 48 B, three 16-byte loads
    if (det) {  // 12 fixed-point sums of 8 bytes
      const longlong2* s = reinterpret_cast<const longlong2*>(reinterpret_cast<const long long*>(p.scratch) +
                                                              ((size_t)(set * Vs + vv) * N + i) * GSR_SCREEN_GRAD_FLOATS);
#pragma unroll
      for (int k = 0; k < 6; ++k) { const longlong2 x = s[k]; sg[2 * k] = from_fixed(x.x); sg[2 * k + 1] = from_fixed(x.y); }
#if GSR_PBWD_UNIT
      const float dn = det_scale_down(det_max_words(p)[set * Vs + vv]);
#pragma unroll
      for (int k = 0; k < 12; ++k) sg[k] *= dn;
#endif
      return;
    }
    const float4* s = reinterpret_cast<const float4*>(p.scratch + ((size_t)(set * Vs + vv) * N + i) * GSR_SCREEN_GRAD_FLOATS);
    const float4 s0 = s[0], s1 = s[1], s2 = s[2];
    sg[0] = s0.x; sg[1] = s0.y; sg[2] = s0.z; sg[3] = s0.w; sg[4] = s1.x; sg[5] = s1.y; sg[6] = s1.z; sg[7] = s1.w;
    sg[8] = s2.x; sg[9] = s2.y; sg[10] = s2.z; sg[11] = s2.w;
  };
  float sg_first[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  if (in_range) {
    rmx = p.means[3 * gi + 0]; rmy = p.means[3 * gi + 1]; rmz = p.means[3 * gi + 2];
    load_covariance(p, set, i, gi, rcov);
    load_row(0, sg_first);
  }
  float T[9];  // kShFrame: the direction transform of this lane's group, loaded where it is used (L1-resident: the lanes share it)
  if (M > 0 && !kJ) {
    const float* sh_src = p.colors + ((size_t)set * N + g0) * rowf;
    const int sh_total = cnt * rowf, sh_n4 = sh_total >> 2;
    if (ldstride == rowf && ((((uintptr_t)sh_src) & 15) == 0)) {
      // all of the wave's 64 x 3M floats requested before the first one is parked in LDS: one memory latency, not nineteen
      constexpr int kPre = 19;  // 64 * 75 / 4 / 64 = 18.75
      float4 pre[kPre];
#pragma unroll
      for (int q = 0; q < kPre; ++q) {
        const int k = lane + 64 * q;
        pre[q] = (k < sh_n4) ? reinterpret_cast<const float4*>(sh_src)[k] : make_float4(0, 0, 0, 0);
      }
#pragma unroll
      for (int q = 0; q < kPre; ++q) {
        const int k = lane + 64 * q;
        if (k < sh_n4) reinterpret_cast<float4*>(sh_in)[k] = pre[q];
      }
      for (int k = (sh_n4 << 2) + lane; k < sh_total; k += 64) sh_in[k] = sh_src[k];
    } else {
      stage_rows(sh_in, sh_src, cnt, rowf, ldstride, lane);
    }
    __syncthreads();
  }
  // With one view per set the SH gradient of coefficient k can take the LDS slot of coefficient k as soon as the mean
  // gradient has used it: one walk.  With several views the coefficients must survive all of them: two walks (below).
  const bool one_walk = (Vs == 1) || kJ;  // (kJ: the rows are free from the start - zeroed here, accumulated into over the views)
  if (kJ && M > 0) {
    float* dsh0 = sh_in + lane * ldstride;  // this lane's own row
    for (int k = 0; k < rowf; ++k) dsh0[k] = 0.f;
  }
  if (dbg) stamps[1] = __builtin_amdgcn_s_memrealtime();
  float dmean[3] = {0, 0, 0}, dcov[6] = {0, 0, 0, 0, 0, 0}, dop = 0, dcol[3] = {0, 0, 0};
  bool seen = false;
  for (int vv = 0; vv < Vs; ++vv) {
    const int v = set * Vs + vv;
    const GsrView cam = view_const(p.views, v);  // the view record in scalar registers: -2 us (the per-lane loads of the uniform record held ~35 VGPRs)
    const size_t oi = (size_t)v * N + (in_range ? i : 0);
    float sg[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) sg[k] = sg_first[k];
    if (vv > 0) {
#pragma unroll
      for (int k = 0; k < 12; ++k) sg[k] = 0.f;
      if (in_range) load_row(vv, sg);
    }
    // A (view, Gaussian) the blend never touched (culled, off screen, or simply unseen) has an all-zero row and adds
    // nothing below - and for a culled one the projection math is not even defined - so the row itself is the test.
    bool vis = false;
#pragma unroll
    for (int k = 0; k < 10; ++k) vis = vis || (sg[k] != 0.f);
    uint32_t bits = 0;
    float4 jx = make_float4(0, 0, 0, 0), jy = jx, jz = jx;  // kJ: d rgb / d direction, clamp mask in jx.w
    if (vis && M > 0) {
      if (kJ) {
        const float4* j = p.shj + oi * 3;
        jx = j[0]; jy = j[1]; jz = j[2];
        bits = __float_as_uint(jx.w) << 28;
      } else {
        bits = __float_as_uint(p.rgbc[oi].w) << 28;
      }
    }
    if (in_range) {
      if (p.dL_dextra) p.dL_dextra[oi] = sg[9];
      if (p.dL_dmeans2D) { p.dL_dmeans2D[3 * oi + 0] = sg[0]; p.dL_dmeans2D[3 * oi + 1] = sg[1]; p.dL_dmeans2D[3 * oi + 2] = 0.f; }
    }
    // Camera gradients (SURVEY 8f-3, opt-in): what this (view, Gaussian) contributes to dL/d viewmatrix [0..16), projmatrix
    // [16..32) and campos [32..35) - every place the forward reads them: t = V p and M = J Wr in the EWA covariance, the
    // projection p_hom = F p, the view direction of the harmonics, the depth of the built-in extra channel.  Summed over
    // the wave below, one partial row per (view, workgroup); k_pose_reduce adds the rows up.  kPose == 3: tanfovx, tanfovy too [35, 37).
    float pose[kCam ? kRow : kPoseZFloats];
    if (kPose) {
#pragma unroll
      for (int k = 0; k < (kCam ? kRow : kPoseZFloats); ++k) pose[k] = 0.f;
    }
    if (vis) {
    seen = true;
    const float mx = rmx * cam.scale, my = rmy * cam.scale, mz = rmz * cam.scale;
    float cov6[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) cov6[k] = rcov[k] * cam.scale2;
    dop += sg[5];
    // --- computeCov2DCUDA
    Cov2D c2;
    cov2d_parts(mx, my, mz, cov6, cam, g.W, g.H, c2);
    const float a = c2.a, b = c2.b, c = c2.c;
    const float dA = sg[2], dB = sg[3], dC = sg[4];
    const float denom = a * c - b * b;
    const float denom2inv = 1.0f / ((denom * denom) + 0.0000001f);
    float dL_da = 0, dL_db = 0, dL_dc = 0;
    float dcv[6] = {0, 0, 0, 0, 0, 0};
    const float* Mm = c2.M;
    if (denom2inv != 0.f) {
      dL_da = denom2inv * (-c * c * dA + 2.f * b * c * dB + (denom - a * c) * dC);
      dL_dc = denom2inv * (-a * a * dC + 2.f * a * b * dB + (denom - a * c) * dA);
      dL_db = denom2inv * 2.f * (b * c * dA - (denom + 2.f * b * b) * dB + a * b * dC);
      dcv[0] = Mm[0] * Mm[0] * dL_da + Mm[0] * Mm[3] * dL_db + Mm[3] * Mm[3] * dL_dc;
      dcv[3] = Mm[1] * Mm[1] * dL_da + Mm[1] * Mm[4] * dL_db + Mm[4] * Mm[4] * dL_dc;
      dcv[5] = Mm[2] * Mm[2] * dL_da + Mm[2] * Mm[5] * dL_db + Mm[5] * Mm[5] * dL_dc;
      dcv[1] = 2.f * Mm[0] * Mm[1] * dL_da + (Mm[0] * Mm[4] + Mm[1] * Mm[3]) * dL_db + 2.f * Mm[3] * Mm[4] * dL_dc;
      dcv[2] = 2.f * Mm[0] * Mm[2] * dL_da + (Mm[0] * Mm[5] + Mm[2] * Mm[3]) * dL_db + 2.f * Mm[3] * Mm[5] * dL_dc;
      dcv[4] = 2.f * Mm[2] * Mm[1] * dL_da + (Mm[1] * Mm[5] + Mm[2] * Mm[4]) * dL_db + 2.f * Mm[4] * Mm[5] * dL_dc;
    }
    const float S[9] = {cov6[0], cov6[1], cov6[2], cov6[1], cov6[3], cov6[4], cov6[2], cov6[4], cov6[5]};
    float dM[6];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const float m0s = Mm[0] * S[0 * 3 + j] + Mm[1] * S[1 * 3 + j] + Mm[2] * S[2 * 3 + j];
      const float m1s = Mm[3] * S[0 * 3 + j] + Mm[4] * S[1 * 3 + j] + Mm[5] * S[2 * 3 + j];
      dM[j] = 2.f * m0s * dL_da + m1s * dL_db;
      dM[3 + j] = 2.f * m1s * dL_dc + m0s * dL_db;
    }
    const float* vw = cam.viewmatrix;
    const float dJ00 = vw[0] * dM[0] + vw[4] * dM[1] + vw[8] * dM[2];
    const float dJ02 = vw[2] * dM[0] + vw[6] * dM[1] + vw[10] * dM[2];
    const float dJ11 = vw[1] * dM[3] + vw[5] * dM[4] + vw[9] * dM[5];
    const float dJ12 = vw[2] * dM[3] + vw[6] * dM[4] + vw[10] * dM[5];
    const float tz = 1.f / c2.t2, tz2 = tz * tz, tz3 = tz2 * tz;
    const float xg = c2.xcl ? 0.f : 1.f, yg = c2.ycl ? 0.f : 1.f;
    const float dtx = xg * -c2.fx * tz2 * dJ02;
    const float dty = yg * -c2.fy * tz2 * dJ12;
    const float dtz = -c2.fx * tz2 * dJ00 - c2.fy * tz2 * dJ11 + (2.f * c2.fx * c2.t0) * tz3 * dJ02 +
                      (2.f * c2.fy * c2.t1) * tz3 * dJ12;
    float dm[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) dm[j] = vw[4 * j + 0] * dtx + vw[4 * j + 1] * dty + vw[4 * j + 2] * dtz;
    if (kCam) {
      const float mj[4] = {mx, my, mz, 1.f}, dt[3] = {dtx, dty, dtz};
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int k = 0; k < 3; ++k) pose[4 * j + k] += dt[k] * mj[j];  // t_k = sum_j V[4j + k] m_j
      const float J00 = c2.fx * tz, J02 = -(c2.fx * c2.t0) * tz2, J11 = c2.fy * tz, J12 = -(c2.fy * c2.t1) * tz2;
#pragma unroll
      for (int j = 0; j < 3; ++j) {  // M[0][j] = J00 V[4j] + J02 V[4j+2],  M[1][j] = J11 V[4j+1] + J12 V[4j+2]
        pose[4 * j + 0] += dM[j] * J00;
        pose[4 * j + 1] += dM[3 + j] * J11;
        pose[4 * j + 2] += dM[j] * J02 + dM[3 + j] * J12;
      }
    }
    if (kPose == 3) {  // tan-fov (GSR_FLAG_FOV_GRADIENT): fx = W / (2 tanfovx) in J00 and J02, and the limit 1.3 tanfovx a clamped t0 sits on
      const float gfx = dJ00 * tz - dJ02 * c2.t0 * tz2, gfy = dJ11 * tz - dJ12 * c2.t1 * tz2;  // dL/dfx, dL/dfy at the clamped t
      float gx = gfx * (-c2.fx / cam.tanfovx), gy = gfy * (-c2.fy / cam.tanfovy);
      // clamped: t0 = +-1.3 tanfovx t2, the sign that of t0 / t2;  J02 = -fx t0 / t2^2
      if (c2.xcl) gx += (-c2.fx * tz2 * dJ02) * ((c2.t0 * tz < 0.f ? -1.3f : 1.3f) * c2.t2);
      if (c2.ycl) gy += (-c2.fy * tz2 * dJ12) * ((c2.t1 * tz < 0.f ? -1.3f : 1.3f) * c2.t2);
      pose[kPoseFloats] += gx; pose[kPoseFloats + 1] += gy;
    }
    // --- projection
    const float* pr = cam.projmatrix;
    const float mh3 = pr[3] * mx + pr[7] * my + pr[11] * mz + pr[15];
    const float m_w = 1.0f / (mh3 + 0.0000001f);
    const float mul1 = (pr[0] * mx + pr[4] * my + pr[8] * mz + pr[12]) * m_w * m_w;
    const float mul2 = (pr[1] * mx + pr[5] * my + pr[9] * mz + pr[13]) * m_w * m_w;
    dm[0] += (pr[0] * m_w - pr[3] * mul1) * sg[0] + (pr[1] * m_w - pr[3] * mul2) * sg[1];
    dm[1] += (pr[4] * m_w - pr[7] * mul1) * sg[0] + (pr[5] * m_w - pr[7] * mul2) * sg[1];
    dm[2] += (pr[8] * m_w - pr[11] * mul1) * sg[0] + (pr[9] * m_w - pr[11] * mul2) * sg[1];
    if (kCam) {  // p_hom_k = sum_j F[4j + k] m_j;  ndc = p_hom.xy / (p_hom.w + eps)
      const float mj[4] = {mx, my, mz, 1.f};
      const float gk[4] = {sg[0] * m_w, sg[1] * m_w, 0.f, -(sg[0] * mul1 + sg[1] * mul2)};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        pose[16 + 4 * j + 0] += gk[0] * mj[j];
        pose[16 + 4 * j + 1] += gk[1] * mj[j];
        pose[16 + 4 * j + 3] += gk[3] * mj[j];
      }
    }
    // --- SH
    if (M > 0) {
      const float ox = mx - cam.campos[0], oy = my - cam.campos[1], oz = mz - cam.campos[2];
      const float len = sqrtf(ox * ox + oy * oy + oz * oz);
      float x = ox / len, y = oy / len, z = oz / len;
      if (kShFrame) { load_dir_frame(p, set, i, T); dir_to_frame(T, x, y, z); }
      const uint32_t cl = bits >> 28;
      const float d0 = (cl & 1u) ? 0.f : sg[6], d1 = (cl & 2u) ? 0.f : sg[7], d2 = (cl & 4u) ? 0.f : sg[8];
      const float* sh = sh_in + lane * ldstride;
      float ddx = 0, ddy = 0, ddz = 0;
      const int deg = min(p.d.sh_degree, p.d.max_sh_eval);
      float* shw = sh_in + lane * ldstride;
      // compile-time strides for the common layouts (see color_unit): run-time ones cost a register per LDS address
      auto sh_block = [&](auto ks_c, auto cs_c) {
        const int ks = ks_c(), cs = cs_c();
        if (kJ) {  // direction gradient from the saved Jacobian; dL/dsh accumulated over the views into the zeroed row
          ddx = jx.x * d0 + jx.y * d1 + jx.z * d2;
          ddy = jy.x * d0 + jy.y * d1 + jy.z * d2;
          ddz = jz.x * d0 + jz.y * d1 + jz.z * d2;
          sh_visit(deg, x, y, z, [&](int k, float bk, float, float, float) {
            if (k < M) { shw[k * ks + 0 * cs] += bk * d0; shw[k * ks + 1 * cs] += bk * d1; shw[k * ks + 2 * cs] += bk * d2; }
          });
          return;
        }
        sh_visit(deg, x, y, z, [&](int k, float bk, float bx, float by, float bz) {
          if (k < M) {
            const float sd = sh[k * ks + 0 * cs] * d0 + sh[k * ks + 1 * cs] * d1 + sh[k * ks + 2 * cs] * d2;
            ddx += bx * sd; ddy += by * sd; ddz += bz * sd;
            if (one_walk) { shw[k * ks + 0 * cs] = bk * d0; shw[k * ks + 1 * cs] = bk * d1; shw[k * ks + 2 * cs] = bk * d2; }
          }
        });
        if (one_walk)  // coefficients above the evaluated degree get no gradient
          for (int k = (deg + 1) * (deg + 1); k < M; ++k) { shw[k * ks + 0 * cs] = 0.f; shw[k * ks + 1 * cs] = 0.f; shw[k * ks + 2 * cs] = 0.f; }
      };
      if (!(p.d.flags & GSR_FLAG_SH_PLANAR)) sh_block([] { return 3; }, [] { return 1; });
      else if (M == 25) sh_block([] { return 1; }, [] { return 25; });
      else sh_block([] { return 1; }, [&] { return M; });
      if (kShFrame && !kJ) grad_to_world(T, ddx, ddy, ddz);
      const float sum2 = ox * ox + oy * oy + oz * oz;
      const float invsum32 = 1.0f / sqrtf(sum2 * sum2 * sum2);
      const float gdir0 = ((sum2 - ox * ox) * ddx - oy * ox * ddy - oz * ox * ddz) * invsum32;
      const float gdir1 = (-ox * oy * ddx + (sum2 - oy * oy) * ddy - oz * oy * ddz) * invsum32;
      const float gdir2 = (-ox * oz * ddx - oy * oz * ddy + (sum2 - oz * oz) * ddz) * invsum32;
      dm[0] += gdir0; dm[1] += gdir1; dm[2] += gdir2;
      if (kCam) { pose[32] -= gdir0; pose[33] -= gdir1; pose[34] -= gdir2; }  // direction = mean - campos
    } else {
      dcol[0] += sg[6]; dcol[1] += sg[7]; dcol[2] += sg[8];
    }
#pragma unroll
    for (int j = 0; j < 3; ++j) dmean[j] += dm[j] * cam.scale;
    const int emode = (p.d.flags >> 4) & 7;
    if (emode != 0 && p.d.has_extra) {  // built-in extra channel: dL/dextra flows to the mean through z (un-normalised units)
      const float z = (vw[2] * mx + vw[6] * my + vw[10] * mz + vw[14]) / cam.scale;
      float dfdz;
      (void)extra_from_depth(emode, z, cam.reserved[0], cam.reserved[1], dfdz);
      const float gz = sg[9] * dfdz;
      dmean[0] += gz * vw[2]; dmean[1] += gz * vw[6]; dmean[2] += gz * vw[10];
      if (kCam) { const float gs = gz / cam.scale; pose[2] += gs * mx; pose[6] += gs * my; pose[10] += gs * mz; pose[14] += gs; }
      if (kPose == 2) { const float gs = gz / cam.scale; pose[0] += gs * mx; pose[1] += gs * my; pose[2] += gs * mz; pose[3] += gs; }
    }
#pragma unroll
    for (int k = 0; k < 6; ++k) dcov[k] += dcv[k] * cam.scale2;
    }  // vis
    if (kCam) {  // sums over the four 16-lane DPP rows (4 DPP adds per value; a full wave sum costs 6 LDS permutes): 4 partial rows
      float* row = p.pose_partials + (((size_t)v * gridDim.x + blockIdx.x) * 4 + (lane >> 4)) * kRow;
#pragma unroll
      for (int k = 0; k < kRow; ++k) {
        const float s = row_allreduce(pose[k]);
        if ((lane & 15) == 0) row[k] = s;
      }
    }
    if (kPose == 2) {  // four values only: the whole wave's sum (DPP rows, then the four row results through scalar registers): ONE row
      float* row = p.pose_partials + ((size_t)v * gridDim.x + blockIdx.x) * kPoseZFloats;
#pragma unroll
      for (int k = 0; k < kPoseZFloats; ++k) {
        const float s = row_allreduce(pose[k]);
        auto at = [&](int l) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(s), l)); };
        const float tot = (at(0) + at(16)) + (at(32) + at(48));
        if (lane == 0) row[k] = tot;
      }
    }
  }
  if (dbg) stamps[2] = __builtin_amdgcn_s_memrealtime();
  if (in_range) {
#pragma unroll
    for (int j = 0; j < 3; ++j) p.dL_dmeans[3 * gi + j] = dmean[j];
    if (p.scale_rot) {
      const float* F = p.frames ? p.frames + ((size_t)set * p.num_frames + (size_t)i / (size_t)(N / p.num_frames)) * 9 : nullptr;
      float dsr[7];
      sr_backward(p.cov6 + 7 * gi, F, dcov, dsr);
#pragma unroll
      for (int k = 0; k < 7; ++k) p.dL_dcov6[7 * gi + k] = dsr[k];
    } else if (p.d.flags & GSR_FLAG_COV_3X3) {
      float* o = p.dL_dcov6 + 9 * gi;
      o[0] = dcov[0]; o[1] = dcov[1]; o[2] = dcov[2]; o[3] = 0.f; o[4] = dcov[3]; o[5] = dcov[4]; o[6] = 0.f; o[7] = 0.f; o[8] = dcov[5];
    } else {
#pragma unroll
      for (int k = 0; k < 6; ++k) p.dL_dcov6[6 * gi + k] = dcov[k];
    }
    p.dL_dopac[gi] = dop;
    if (M == 0) { p.dL_dcolors[3 * gi + 0] = dcol[0]; p.dL_dcolors[3 * gi + 1] = dcol[1]; p.dL_dcolors[3 * gi + 2] = dcol[2]; }
  }
  if (dbg) stamps[3] = __builtin_amdgcn_s_memrealtime();
  if (M > 0 && one_walk) {
    if (!seen && !kJ) {  // this lane's Gaussian received no gradient: its row still holds the coefficients
      float* dsh = sh_in + lane * ldstride;
      for (int k = 0; k < rowf; ++k) dsh[k] = 0.f;
    }
    __syncthreads();
    unstage_rows(p.dL_dcolors + ((size_t)set * N + g0) * rowf, sh_in, cnt, rowf, ldstride, lane);
  } else if (M > 0) {
    float* dsh = sh_in + lane * ldstride;  // this lane's row: the coefficients are no longer needed
    for (int k = 0; k < rowf; ++k) dsh[k] = 0.f;
    const int deg = min(p.d.sh_degree, p.d.max_sh_eval);
    if (kShFrame) load_dir_frame(p, set, i, T);
    auto second_walk = [&](auto ks_c, auto cs_c) {
    const int ks = ks_c(), cs = cs_c();
    for (int vv = 0; vv < Vs && in_range; ++vv) {
      const int v = set * Vs + vv;
      const GsrView& cam = p.views[v];
      const size_t oi = (size_t)v * N + i;
      float c0, c1, c2;
      if (det) {
        const long long* sgi = reinterpret_cast<const long long*>(p.scratch) + oi * GSR_SCREEN_GRAD_FLOATS;
        c0 = from_fixed(sgi[6]); c1 = from_fixed(sgi[7]); c2 = from_fixed(sgi[8]);
#if GSR_PBWD_UNIT
        { const float dn = det_scale_down(det_max_words(p)[v]); c0 *= dn; c1 *= dn; c2 *= dn; }
#endif
      } else {
        const float* sgp = p.scratch + oi * GSR_SCREEN_GRAD_FLOATS;
        c0 = sgp[6]; c1 = sgp[7]; c2 = sgp[8];
      }
      if (c0 == 0.f && c1 == 0.f && c2 == 0.f) continue;
      const uint32_t cl = __float_as_uint(p.rgbc[oi].w);
      const float d0 = (cl & 1u) ? 0.f : c0, d1 = (cl & 2u) ? 0.f : c1, d2 = (cl & 4u) ? 0.f : c2;
      const float ox = rmx * cam.scale - cam.campos[0], oy = rmy * cam.scale - cam.campos[1], oz = rmz * cam.scale - cam.campos[2];
      const float len = sqrtf(ox * ox + oy * oy + oz * oz);
      float x = ox / len, y = oy / len, z = oz / len;
      if (kShFrame) dir_to_frame(T, x, y, z);
      sh_visit(deg, x, y, z, [&](int k, float bk, float, float, float) {
        if (k < M) { dsh[k * ks + 0 * cs] += bk * d0; dsh[k * ks + 1 * cs] += bk * d1; dsh[k * ks + 2 * cs] += bk * d2; }
      });
    }
    };
    if (!(p.d.flags & GSR_FLAG_SH_PLANAR)) second_walk([] { return 3; }, [] { return 1; });
    else if (M == 25) second_walk([] { return 1; }, [] { return 25; });
    else second_walk([] { return 1; }, [&] { return M; });
    __syncthreads();
    unstage_rows(p.dL_dcolors + ((size_t)set * N + g0) * rowf, sh_in, cnt, rowf, ldstride, lane);
  }
  if (dbg && lane == 0) {  // measurement aid: phase stamps (100 MHz) over this workgroup's first dL/dmeans2D entries
    stamps[4] = __builtin_amdgcn_s_memrealtime();
    unsigned long long* o = reinterpret_cast<unsigned long long*>(p.dL_dmeans2D + 3 * ((size_t)set * Vs * N + g0));
    for (int q = 0; q < 5; ++q) o[q] = stamps[q];
  }
}
