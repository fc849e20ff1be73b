#pragma once
// K5 per-tile sort, K6 / K2 forward tile kernels.  (gsr_binning.h: take_pages.)
#include "gsr_common.h"
#include "gsr_binning.h"

namespace gsr {

// ------------------------------------------------------------------------------------------------
// K5: per-tile depth sort, kSortThreads threads per tile.  Bitonic network in its all-ascending (mirror)
// form so that a list of any length sorts with virtual +inf padding; <= kLds keys sort in LDS, longer
// lists in place in global memory.  Within a substep all compare-exchanges are disjoint, so each thread
// loads a batch of pairs before storing any (LDS latency paid once per batch, not once per pair).
// Writes the sorted Gaussian indices (the reference's point_list).
// ------------------------------------------------------------------------------------------------
template <bool kFlip, class KeyPtr>
__device__ __forceinline__ void bitonic_substep(KeyPtr a, int n, int half, int lg, int tid) {
  // kFlip: pairs (blk*2^(lg+1) + off, blk*2^(lg+1) + 2^(lg+1) - 1 - off); else (i, i + 2^lg), off < 2^lg
  constexpr int U = 4;
  const int w = 1 << lg;
  for (int tb = tid; tb < half; tb += kSortThreads * U) {
    int ii[U], jj[U];
    unsigned long long x[U], y[U];
    bool act[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int t = tb + u * kSortThreads;
      const int blk = t >> lg, off = t & (w - 1);
      ii[u] = (blk << (lg + 1)) + off;
      jj[u] = kFlip ? (blk << (lg + 1)) + 2 * w - 1 - off : ii[u] + w;
      act[u] = (t < half) && (jj[u] < n);
      x[u] = act[u] ? a[ii[u]] : 0ull;
      y[u] = act[u] ? a[jj[u]] : 0ull;
    }
#pragma unroll
    for (int u = 0; u < U; ++u)
      if (act[u] && x[u] > y[u]) { a[ii[u]] = y[u]; a[jj[u]] = x[u]; }
  }
}

template <class KeyPtr>
__device__ __forceinline__ void bitonic_block(KeyPtr a, int n, int lgnp, int tid) {
  const int half = 1 << (lgnp - 1);
  for (int lk = 1; lk <= lgnp; ++lk) {
    bitonic_substep<true>(a, n, half, lk - 1, tid);
    __syncthreads();
    for (int lj = lk - 2; lj >= 0; --lj) {
      bitonic_substep<false>(a, n, half, lj, tid);
      __syncthreads();
    }
  }
}

constexpr int kSpanMax = 48;      // most keys in one depth bucket the rank finish accepts (else bitonic fallback)

// Exclusive scan over the kSortThreads per-thread values of a workgroup (wave scan + 4 wave totals through LDS).
// Workgroup-wide OR of a predicate with its barrier (four waves).  Own version of __syncthreads_or: the device library's keeps a
// 256-byte LDS scratch per kernel and k_tile_fwd_prefix sits 120 bytes above the size at which five workgroups share a CU (LDS is
// handed out in 1280-byte units on gfx950).  `slot`: four LDS words of this call site's own.
__device__ __forceinline__ bool block_any(const bool pred, uint32_t* slot) {
  const bool w = __any((int)pred) != 0;
  if ((threadIdx.x & 63) == 0) slot[threadIdx.x >> 6] = w ? 1u : 0u;
  __syncthreads();
  return (slot[0] | slot[1] | slot[2] | slot[3]) != 0u;
}

__device__ __forceinline__ uint32_t block_exclusive_scan(uint32_t v, uint32_t* wave_tot /*[4] LDS*/, int tid, uint32_t& total) {
  const int lane = tid & 63, w = tid >> 6;
  const uint32_t s = wave_inclusive_scan_u32(v);
  if (lane == 63) wave_tot[w] = s;
  __syncthreads();
  uint32_t basew = 0;
  total = 0;
#pragma unroll
  for (int k = 0; k < kSortThreads / 64; ++k) {
    const uint32_t x = wave_tot[k];
    basew += (k < w) ? x : 0u;
    total += x;
  }
  return basew + s - v;
}

// Per-tile depth sort, kSortThreads threads per tile; writes the sorted Gaussian indices (the reference's point_list).
// Lists of up to kLds keys: LDS bucket sort - keys stay in registers, one LDS-atomic histogram over the buckets of the
// tile's own depth range (float bits are monotonic for positive depths), exclusive scan, LDS-atomic scatter into bucket
// order, then every key ranks itself among the few keys of its own bucket with the full 64-bit (depth, index) compare and
// goes to its final place.  ~40 B of LDS traffic per key instead of ~800 B for an in-LDS bitonic network.  Degenerate depth
// distributions (a bucket of more than kSpanMax keys) fall back to the bitonic network on the same LDS array; lists longer
// than kLds sort in place in global memory with the same network.
// kGather = false: the tile's keys are a contiguous range (ranges[]) written by k_emit.
// kGather = true : the tile's keys sit in up to `rows` runs, one per binning workgroup (k_preprocess_bin): column
//   (view, :, tile) of the pair matrix says where and how many.  The workgroup sums the column, copies the runs into LDS in
//   row order - after which everything is as in the contiguous case - and writes the sorted indices into the tile's own
//   fixed slot of the index list (`stride` = pair_capacity / (2 x views x tiles) entries; a longer list takes a run of the
//   shared second half from a bump counter: correct for any distribution as long as pair_capacity >= 2 x pairs, and free of
//   shared counters when pair_capacity >= 2 x views x tiles x longest list).
// LDS of a per-tile sort: kLds keys (8 B) then the bucket counters (4 B), in 8-byte words
template <int kLds>
struct SortLds {
  // depth buckets: one per key slot in the 2048-key variant (a dense depth cluster otherwise makes buckets of 20-30 entries and
  // ranking inside a bucket is quadratic: forward -1.1 us), a quarter of that in the 4096-key variant (LDS: four workgroups / CU)
  static constexpr int kBuckets = kLds == 2048 ? 2048 : 1024, kBucketBits = kLds == 2048 ? 11 : 10;
  static constexpr int kWords = kLds + kBuckets / 2;
};

// The sort of one tile's list: returns the tile's range of the index list (empty when the tile has no entry or the list did
// not fit: then status->overflow is set).  All `return`s are workgroup-uniform.  The caller provides `smem`
// (SortLds<kLds>::kWords 8-byte words, 16-byte aligned), red[8] and sInfo[4] in LDS, and (kGather) `tg`, the (view, tile) this
// workgroup takes: the caller decides it once - xcd_remap's image order or the deal - for the sort and the blend alike.
template <bool kGather, int kLds>
__device__ __forceinline__ uint2 sort_tile(const Params& p, const uint32_t bid, const int tg, unsigned long long* smem, uint32_t* red,
                                           uint32_t* sInfo) {
  // kLds keys sort in LDS over SortLds<kLds>::kBuckets depth buckets
  constexpr int kBk = SortLds<kLds>::kBuckets, kBkBits = SortLds<kLds>::kBucketBits, kBpt = kBk / kSortThreads;
  static_assert(kLds == 4096 || kLds == 2048, "bucket geometry");
  unsigned long long* sk = smem;
  uint32_t* hist = reinterpret_cast<uint32_t*>(smem + kLds);  // counts, then (same storage) scatter cursors
  uint32_t* cur = hist;
  const int tid = threadIdx.x;
  const bool dbg = GSR_ABL(p.d.flags, GSR_FLAG_DEBUG_TIMING);
  unsigned long long* stamp = dbg_stamps(p, 8192 + bid);
  unsigned long long* stamp2 = dbg_stamps(p, 8192 + p.sort_blocks + bid);
  GSR_STAMP(0);
  int n;
  uint32_t obase = 0;  // where the tile's list starts in the index list
  unsigned long long* keys;  // global memory: contiguous keys (kGather: only for lists longer than the LDS sort)
  uint32_t* out;
  if (kGather) {
    const int T = p.g.T, R = p.rows;
    // XCD-aware order: neighbouring tiles' runs share cache lines in every region, so give each XCD (= each L2) a contiguous
    // range of tiles (the caller's `tg`)
    const int v = tg / T, t = tg - v * T;
    // De-phase the first resident round.  All its workgroups start together and would gather together (memory-bound, CUs
    // idle: 250 k small reads take 11 us when issued at once, 2-4 us per workgroup when spread out), then sort together
    // (LDS-bound, memory idle).  Four groups 2 us apart let one group's gather overlap another's bucket sort (none at all:
    // forward +12 us).  The group is the workgroup's residency slot on its CU (workgroups b, b + 256, b + 512, b + 768 share
    // a CU - HW_ID stamps, tools/tile_timeline.py): the four tiles of a CU are then out of phase with EACH OTHER, one blends
    // while the next still sorts (grouping neighbouring CUs instead: +0.8 us).  Later rounds start whenever a slot frees up.
    if (bid < 1024u) {
      for (int q = 0; q < (int)((bid >> kDephaseShift) % kDephaseGroups); ++q) __builtin_amdgcn_s_sleep(64);
    }
    const uint2* col = p.pair_mat + (size_t)v * R * (T + 8) + t;
    const size_t cstride = (size_t)T + 8;
    const uint32_t* bb = p.blk_base + (size_t)v * R;
    // the length of the list, and whether every run was stored.  With up to kSortThreads rows (the usual case) a thread keeps
    // its row's (offset, count) and region base in registers; with more the column is read again for the copy.
    const bool one_stride = R <= kSortThreads;
    uint2 e0 = make_uint2(0u, 0u);
    uint32_t bb0 = 0, cnt_sum = 0, missing = 0;
    if (one_stride) {
      if (tid < R) { e0 = col[(size_t)tid * cstride]; bb0 = bb[tid]; }
      cnt_sum = e0.y;
      missing = (e0.y != 0u && bb0 == 0xffffffffu) ? 1u : 0u;
    } else {
      for (int r = tid; r < R; r += kSortThreads) {
        const uint32_t c = col[(size_t)r * cstride].y;
        cnt_sum += c;
        missing |= (c != 0u && bb[r] == 0xffffffffu) ? 1u : 0u;
      }
    }
    GSR_STAMP2(0);
    uint32_t total;
    const uint32_t start0 = block_exclusive_scan(cnt_sum, red, tid, total);
    __shared__ uint32_t sAnyMissing[kSortThreads / 64];
    const bool any_missing = block_any(missing, sAnyMissing);
    n = (int)total;
    // The tile's range of the index list: its own fixed slot of `stride` entries (no counter shared with other tiles), or -
    // a list longer than that - a run of the tail region behind the slots, taken from a bump counter.  The usual case
    // (every run stored, list fits its slot and the LDS sort) needs no decision by one thread and no barrier.
    const bool plain = !any_missing && (uint32_t)n <= p.stride && n <= kLds;
    // (the longest list so far, statistics.  Two ways of taking this read off wave 1's path were tried - asked for at the kernel's start:
    // it reads 0 in every tile and a thousand same-address atomics follow, +2 us; asked for here and compared after the run copy: +11 us)
    // Round 4: for the usual tile (`plain`) the statistic is updated by k_tile_fwd AFTER the tile's image is written - here it sat
    // in front of a barrier, and a barrier waits for the wave's outstanding memory operations: the load of a word every tile of
    // the launch goes for and, for the first tiles to arrive, a device-scope atomic queued behind hundreds of others (see
    // k_tile_fwd_prefix).  A tile that may fail to place its list keeps the early update: the caller sizes its retry from it.
    if (!plain && tid == 64 && (uint32_t)n > p.status->max_list) atomicMax(&p.status->max_list, (uint32_t)n);
    if (plain) {
      if (tid == 0) p.ranges[tg] = make_uint2((uint32_t)tg * p.stride, (uint32_t)tg * p.stride + (uint32_t)n);
    } else if (tid == 0) {
      uint32_t rbase = (uint32_t)tg * p.stride, ok = any_missing ? 0u : 1u, scratch = 0;
      if (ok && (uint32_t)n > p.stride) {
        const uint32_t at = atomicAdd(p.tail_counter, (uint32_t)n);
        if (at <= p.tail_cap && (uint32_t)n <= p.tail_cap - at) rbase = p.tail_off + at;
        else ok = 0;
      }
      if (ok && n > kLds) {  // contiguous scratch for the in-place global sort, from the page pool
        const uint32_t np = ((uint32_t)n + kPage - 1) / kPage;
        const uint32_t first = take_pages(p.page_counter_tiles, p.call_tag, np), half = p.key_pages / 2;  // upper half of the pool
        if (first <= p.key_pages - half && np <= p.key_pages - half - first) scratch = p.pool_off + (half + first) * (uint32_t)kPage;
        else ok = 0;
      }
      if (!ok) p.status->overflow = 1u;
      p.ranges[tg] = ok ? make_uint2(rbase, rbase + (uint32_t)n) : make_uint2(0u, 0u);
      sInfo[0] = rbase; sInfo[1] = ok; sInfo[2] = scratch;
    }
    if (bid == 0) {  // total pair count = sum of the binning workgroups' totals
      unsigned long long part = 0;
      for (int k = tid; k < p.d.num_views * R; k += kSortThreads) part += p.blk_total[k];
      for (int o = 32; o > 0; o >>= 1) part += __shfl_down(part, o, 64);
      __shared__ unsigned long long sPart[kSortThreads / 64];
      if ((tid & 63) == 0) sPart[tid >> 6] = part;
      __syncthreads();
      if (tid == 0) p.status->num_pairs = sPart[0] + sPart[1] + sPart[2] + sPart[3];
    }
    uint32_t rbase = (uint32_t)tg * p.stride, scratch = 0;
    if (!plain) {  // workgroup-uniform
      __syncthreads();
      if (!sInfo[1]) return make_uint2(0u, 0u);
      rbase = sInfo[0]; scratch = sInfo[2];
    }
    obase = rbase;
    if (n == 0) return make_uint2(obase, obase);
    GSR_STAMP2(1);
    out = p.point_list + rbase;
    keys = p.keys + scratch;
    unsigned long long* dst = n > kLds ? keys : sk;
    // copy the runs, in row order: six keys per step as three 16-byte loads issued together (runs are ~5 keys long; a lane's
    // request is what the memory pipeline counts, so 16 bytes per lane halve the cost of this scattered read).  The loads may
    // run one key past the run: still inside the key buffer (it is padded).
    auto copy_run = [&](const unsigned long long* src, uint32_t cnt, uint32_t start) {
      for (uint32_t j = 0; j < cnt; j += 6) {
        const ull2 a = *reinterpret_cast<const ull2*>(src + j);
        ull2 b = {0ull, 0ull}, c = {0ull, 0ull};
        if (j + 2 < cnt) b = *reinterpret_cast<const ull2*>(src + j + 2);
        if (j + 4 < cnt) c = *reinterpret_cast<const ull2*>(src + j + 4);
        unsigned long long* d = dst + start + j;
        d[0] = a.x;
        if (j + 1 < cnt) d[1] = a.y;
        if (j + 2 < cnt) d[2] = b.x;
        if (j + 3 < cnt) d[3] = b.y;
        if (j + 4 < cnt) d[4] = c.x;
        if (j + 5 < cnt) d[5] = c.y;
      }
    };
    if (one_stride) {
      if (e0.y) copy_run(p.keys + bb0 + e0.x, e0.y, start0);
      __syncthreads();
      GSR_STAMP2(2);
    } else {
      uint32_t carry = 0;
      for (int r0 = 0; r0 < R; r0 += kSortThreads) {
        const int r = r0 + tid;
        const uint2 e = r < R ? col[(size_t)r * cstride] : make_uint2(0u, 0u);
        uint32_t tot;
        const uint32_t start = carry + block_exclusive_scan(e.y, red, tid, tot);
        carry += tot;
        if (e.y) copy_run(p.keys + bb[r] + e.x, e.y, start);
        __syncthreads();  // red[] is reused by the next stride
      }
    }
    if (n == 1) {
      if (tid == 0) out[0] = (uint32_t)dst[0];
      return make_uint2(obase, obase + 1u);
    }
  } else {
    const uint2 rg = p.ranges[bid];
    n = (int)(rg.y - rg.x);
    obase = rg.x;
    if (n == 0) return rg;
    keys = p.keys + rg.x;
    out = p.point_list + rg.x;
    if (n == 1) {
      if (tid == 0) out[0] = (uint32_t)keys[0];
      return rg;
    }
  }
  int lgnp = 1;
  while ((1 << lgnp) < n) ++lgnp;
  if (n > kLds) {
    __syncthreads();
    bitonic_block(keys, n, lgnp, tid);
    for (int k = tid; k < n; k += kSortThreads) out[k] = (uint32_t)keys[k];
    return make_uint2(obase, obase + (uint32_t)n);
  }
  constexpr int Q = kLds / kSortThreads;
  unsigned long long kreg[Q];
  uint32_t lo = 0xffffffffu, hi = 0u;
#pragma unroll
  for (int q = 0; q < Q; ++q) {
    const int k = tid + q * kSortThreads;
    kreg[q] = (k < n) ? (kGather ? sk[k] : keys[k]) : ~0ull;
    if (k < n) {
      const uint32_t d = (uint32_t)(kreg[q] >> 32);
      lo = d < lo ? d : lo;
      hi = d > hi ? d : hi;
    }
  }
  GSR_STAMP(1);
  for (int k = tid; k < kBk; k += kSortThreads) hist[k] = 0;
  // block min / max of the depth bits
  hi = wave_max_u32(hi);
  lo = ~wave_max_u32(~lo);
  if ((tid & 63) == 0) { red[tid >> 6] = lo; red[4 + (tid >> 6)] = hi; }
  __syncthreads();
  lo = min(min(red[0], red[1]), min(red[2], red[3]));
  hi = max(max(red[4], red[5]), max(red[6], red[7]));
  const uint32_t range = hi - lo;
  const int shift = range < (uint32_t)kBk ? 0 : (32 - __clz((int)range)) - kBkBits;
#pragma unroll
  for (int q = 0; q < Q; ++q)
    if (tid + q * kSortThreads < n) atomicAdd(&hist[((uint32_t)(kreg[q] >> 32) - lo) >> shift], 1u);
  __syncthreads();
  GSR_STAMP(2);
  // exclusive scan of the bucket counts: thread t owns kBpt consecutive buckets
  uint32_t c[kBpt], span = 0, cmax = 0;
#pragma unroll
  for (int q = 0; q < kBpt; ++q) { c[q] = hist[kBpt * tid + q]; span += c[q]; cmax = max(cmax, c[q]); }
  uint32_t total;
  uint32_t start = block_exclusive_scan(span, red, tid, total);
#pragma unroll
  for (int q = 0; q < kBpt; ++q) { cur[kBpt * tid + q] = start; start += c[q]; }
  __shared__ uint32_t sAnyBig[kSortThreads / 64];
  const bool big = block_any(cmax > (uint32_t)kSpanMax, sAnyBig);
  GSR_STAMP(3);
  // scatter into bucket order
#pragma unroll
  for (int q = 0; q < Q; ++q)
    if (tid + q * kSortThreads < n) {
      const uint32_t slot = atomicAdd(&cur[((uint32_t)(kreg[q] >> 32) - lo) >> shift], 1u);
      sk[slot] = kreg[q];
    }
  __syncthreads();
  GSR_STAMP(4);
  if (!big) {
    // finish by ranking: every entry counts the smaller keys of its own bucket (keys are unique: they carry the
    // Gaussian index) and goes straight to its final slot in the global list.  The loads are independent, unlike
    // the dependent chain of an insertion sort.  After the scatter cur[b] is the END of bucket b.
    for (int k = tid; k < n; k += kSortThreads) {
      const unsigned long long key = sk[k];
      const uint32_t b = ((uint32_t)(key >> 32) - lo) >> shift;
      const int bs = b ? (int)cur[b - 1] : 0, be = (int)cur[b];
      int rank = bs;
      // four members per step, requested together (a dense depth cluster makes buckets of 20-30 entries: the chain of
      // dependent LDS reads is what this loop costs)
      for (int j = bs; j < be; j += 4) {
        const unsigned long long k0 = sk[j], k1 = sk[min(j + 1, be - 1)], k2 = sk[min(j + 2, be - 1)], k3 = sk[min(j + 3, be - 1)];
        rank += (k0 < key ? 1 : 0) + ((j + 1 < be && k1 < key) ? 1 : 0) + ((j + 2 < be && k2 < key) ? 1 : 0) +
                ((j + 3 < be && k3 < key) ? 1 : 0);
      }
      out[rank] = (uint32_t)key;
    }
    GSR_STAMP(5);
    GSR_STAMP(6);
    return make_uint2(obase, obase + (uint32_t)n);
  }
  bitonic_block(sk, n, lgnp, tid);
  __syncthreads();
  GSR_STAMP(5);
  for (int k = tid; k < n; k += kSortThreads) out[k] = (uint32_t)sk[k];
  GSR_STAMP(6);
  return make_uint2(obase, obase + (uint32_t)n);
}


// ------------------------------------------------------------------------------------------------
// Blend helpers shared by the forward and backward blend kernels (both must take the same skip decisions).
// At staging time (lane = splat) the conic is moved to the exp2 domain: a2 = -0.5 log2e A, b2 = -log2e B,
// c2 = -0.5 log2e C, so that per pixel  G = exp(power) = 2^(a2 dx^2 + b2 dx dy + c2 dy^2)  costs two multiplies,
// two FMAs and one v_exp_f32.
// ------------------------------------------------------------------------------------------------
constexpr float kLog2e = 1.4426950408889634f;
constexpr float kLn2 = 0.6931471805599453f;

__device__ __forceinline__ void to_exp2_domain(float4& q0, float4& q1) {
  q0.z = (-0.5f * kLog2e) * q0.z;
  q0.w = (-kLog2e) * q0.w;
  q1.x = (-0.5f * kLog2e) * q1.x;
}
__device__ __forceinline__ float splat_p2(float a2, float b2, float c2, float dx, float dy) {
  const float t = __builtin_fmaf(b2, dy, a2 * dx);
  return __builtin_fmaf(c2 * dy, dy, t * dx);
}

// ------------------------------------------------------------------------------------------------
// K6: forward blend ([EXT] forward.cu renderCUDA; oracle blend_forward).  One workgroup of four wavefronts per 8x8 tile,
// lane = pixel in every wave; the depth-ordered list is cut into batches of kFB entries and every batch into four
// SEGMENTS of kFS consecutive entries, one per wave.  The only dependence between entries is the transmittance
// T <- T (1 - alpha), a product - so a segment needs from its predecessors nothing but the product of their (1 - alpha):
//   stage E (batch i+1): the wave evaluates alpha(pixel, splat) of its segment into REGISTERS (0 where the reference
//                        skips: power > 0 or alpha < 1/255) and publishes the segment product P = prod (1 - alpha);
//   stage A (batch i)  : every wave reads the four products of the batch, forms the transmittance at the start of its
//                        own segment (Tb P0 .. P(w-1), the same multiplication chain in every wave, so all waves hold
//                        bit-identical values), then runs the reference's per-entry loop over its kFS entries from
//                        there: test T (1 - alpha) < 1e-4, weight alpha T, colour / extra accumulation, last contributor.
// Since T never increases, "the reference loop has stopped" <=> T (1 - alpha) < 1e-4 now, so the free-running product
// decides per entry exactly what the sequential loop decides; the reported final T is the smallest T that passed.
// Per-pixel arithmetic is the reference's except that T crosses a segment boundary as T_start x (segment product) rather
// than entry by entry (an fp32 re-association, ~1e-7 relative), and the colour sum is split in four partial sums.
// Wave (b mod 4) gathers the records of batch b: list ids three iterations ahead, records two ahead, LDS one ahead.
// Why this shape: a lone wavefront issues one VALU instruction per ~6 cycles on MI355X (measured) and a 256x256 view
// only has 1024 tiles for 1024 SIMDs, so a tile needs several waves; with segments no wave carries a sequential chain
// longer than kFS entries and no alpha travels through LDS.
// ------------------------------------------------------------------------------------------------
// Four waves per workgroup = one per SIMD: with a fifth wave every workgroup puts two waves on the same SIMD and the
// per-SIMD register file then admits only 3 workgroups per CU (768 of the 1024 tiles of a 256x256 view; measured).
typedef float f2 __attribute__((ext_vector_type(2)));
constexpr int kFwdWaves = 4;
#ifndef GSR_KFS
#define GSR_KFS 8
#endif
constexpr int kFS = GSR_KFS;                  // entries per wave per batch (even)
constexpr int kFB = kFS * kFwdWaves;          // 32 list entries per batch
constexpr int kFwdThreads = 64 * kFwdWaves;   // 256

__device__ __forceinline__ void stage_batch(const GeomRec* geom, const float4* rgbc, uint32_t n, uint32_t base, int lane,
                                            uint32_t id, bool want_extra, float4& g, float2& g2, float4& c) {
  // lane = splat; null record (opacity 0) past the end of the list
  g = make_float4(0, 0, 0, 0); g2 = make_float2(0, 0); c = make_float4(0, 0, 0, 0);
  if (base + lane < n) {
    // loads only - no arithmetic on the values here, so that nothing waits for them before they are parked (put_records
    // moves the conic to the exp2 domain)
    const GeomRec* r = geom + id;
    const float4 q0 = r->q0, q1 = r->q1;
    const float4 col = rgbc[id];
    const float ex = want_extra ? q1.z : 0.f;
    g = q0; g2 = make_float2(q1.x, q1.y); c = make_float4(col.x, col.y, col.z, ex);
  }
}

struct BlendLds {
  // records of a batch, laid out for PAIRS of consecutive entries (e, e+1) so that one ds_read_b128 yields the two
  // operands of two packed-fp32 instructions: [x x' y y'], [a2 a2' b2 b2'], [c2 c2' o o'], [r r' g g'], [b b' ex ex']
  float4 sXY[4][kFB / 2], sAB[4][kFB / 2], sCO[4][kFB / 2], sRG[4][kFB / 2], sBE[4][kFB / 2];
  float sP[2][kFwdWaves][64];  // segment products of batch b in sP[b & 1]
};
// One record into entry e of slot sb, conic moved to the exp2 domain: blend_range's put_records for any entry instead of "lane =
// entry" (the rank pass of k_tile_fwd_prefix: e = the entry's position in the list).  put_records keeps its own text: written through
// this function the blend of EVERY tile kernel compiled to other instructions, and k_tile_fwd and the 80-register instances are to
// stay the code they were.
__device__ __forceinline__ void park_record(BlendLds& lds, const int sb, const int e, float4 q, float2 q2, const float4& c) {
  q.z = (-0.5f * kLog2e) * q.z; q.w = (-kLog2e) * q.w; q2.x = (-0.5f * kLog2e) * q2.x;  // to_exp2_domain
  const int o = (e >> 1) * 4 + (e & 1);
  float* xy = reinterpret_cast<float*>(lds.sXY[sb]); float* ab = reinterpret_cast<float*>(lds.sAB[sb]);
  float* co = reinterpret_cast<float*>(lds.sCO[sb]); float* rg2 = reinterpret_cast<float*>(lds.sRG[sb]);
  float* be = reinterpret_cast<float*>(lds.sBE[sb]);
  xy[o] = q.x; xy[o + 2] = q.y; ab[o] = q.z; ab[o + 2] = q.w; co[o] = q2.x; co[o + 2] = q2.y;
  rg2[o] = c.x; rg2[o + 2] = c.y; be[o] = c.z; be[o + 2] = c.w;
}
// k_tile_fwd_prefix hands the first batches of a list to its blend through LDS (blend_range, `primed`): the ids of the first
// kPrimedIds positions - what the prologue reads for batches 0 ... 9 - lie over sP, which nobody touches before the first eval
constexpr int kPrimedIds = 10 * kFB;
static_assert(sizeof(uint32_t) * kPrimedIds <= sizeof(BlendLds::sP), "the handed-over ids fit the segment products' area");
// the four waves' partial results on their way to wave 0 (blend_finish): used once, after the last batch - k_tile_fwd_prefix lays
// it over its key array, which is dead by then (6 KB less: five workgroups per CU instead of four)
struct BlendFin {
  float sPart[kFwdWaves][5][64];
  uint32_t sLast[kFwdWaves][64];
};

// What a tile's blend carries from one range of its list to the next (k_tile_fwd_prefix blends the ranked prefix of the list
// first and comes back for the rest only if some pixel is still open): the free-running transmittance at the start of the
// next batch (the same bits in all four waves), and this wave's partial results.
struct BlendAcc {
  float Tb;     // free-running transmittance at the start of the batch (same in all waves)
  float Tmin;   // smallest transmittance that passed the test in this wave's segments
  f2 CR, CG, CB, CE;  // colour sums over even / odd entries
  uint32_t last, consumed;
};

// Batches [b0, nbat) of the list `plist` (entries at positions >= n read as null records), 256 threads.  Returns true when every
// pixel's loop has stopped (workgroup-uniform: the decision is taken on bit-identical values in all four waves).
// kPrimed (k_tile_fwd_prefix, the first pass of a list its rank pass has just ranked: b0 == 0): the records of batches 0 and 1 are
// parked already and the ids of positions < kPrimedIds lie over sP - the prologue reads no id from memory and requests only the
// batches it holds in registers; the state at the loop's entry is the ordinary prologue's.
template <bool kExtra, bool kTight = false, bool kPrimed = false>  // kTight: an instance built for 80 registers (see put_records)
__device__ __forceinline__ bool blend_range(const GeomRec* geom, const float4* rgbc, const uint32_t* plist, const uint32_t n,
                                            const uint32_t b0, const uint32_t nbat, BlendLds& lds, BlendAcc& s, const float pxf,
                                            const float pyf) {
  auto& sXY = lds.sXY; auto& sAB = lds.sAB; auto& sCO = lds.sCO; auto& sRG = lds.sRG; auto& sBE = lds.sBE;
  auto& sP = lds.sP;
  // (the wave's number in a SCALAR register: as `threadIdx.x >> 6` it lives in a vector register, and the choice of this wave's starting
  // transmittance among Tb, t1, t2, t3 - wave-uniform - compiled into exec-mask branches and vector compares in every iteration)
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int lane = threadIdx.x & 63;
  float Tb = s.Tb, Tmin = s.Tmin;
  f2 al[kFS / 2];                               // alphas of this wave's segment of the batch about to be accumulated
  uint32_t last = s.last, consumed = s.consumed;
  const int e0 = wave * kFS;

  const f2 px2 = {pxf, pxf}, py2 = {pyf, pyf};
  f2 om[kFS / 2];                               // 1 - alpha of the same entries (kept: stage A needs both)
  auto eval = [&](uint32_t b) {  // stage E, two entries per step (v_pk_*_f32: same rounding per component as scalar code)
    const int gb = b & 3;
    f2 P2 = {1.f, 1.f};
#pragma unroll
    for (int u = 0; u < kFS; u += 2) {
      const float4 xy = sXY[gb][(e0 + u) >> 1], ab = sAB[gb][(e0 + u) >> 1], co = sCO[gb][(e0 + u) >> 1];
      const f2 dx = f2{xy.x, xy.y} - px2, dy = f2{xy.z, xy.w} - py2;
      const f2 a2 = {ab.x, ab.y}, b2 = {ab.z, ab.w}, c2 = {co.x, co.y}, o = {co.z, co.w};
      const f2 t = __builtin_elementwise_fma(b2, dy, a2 * dx);
      const f2 p2 = __builtin_elementwise_fma(c2 * dy, dy, t * dx);
      const f2 ao = o * f2{__builtin_amdgcn_exp2f(p2.x), __builtin_amdgcn_exp2f(p2.y)};
      const float alpha0 = fminf(0.99f, ao.x), alpha1 = fminf(0.99f, ao.y);
      const bool keep0 = !(p2.x > 0.f) && !(alpha0 < 1.0f / 255.0f), keep1 = !(p2.y > 0.f) && !(alpha1 < 1.0f / 255.0f);
      al[u >> 1] = f2{keep0 ? alpha0 : 0.f, keep1 ? alpha1 : 0.f};
      om[u >> 1] = f2{1.f, 1.f} - al[u >> 1];
      P2 *= om[u >> 1];
    }
    sP[b & 1][wave][lane] = P2.x * P2.y;
  };
  f2 CR = s.CR, CG = s.CG, CB = s.CB, CE = s.CE;  // colour sums over even / odd entries
  // Stage A; Tf = transmittance at the start of this wave's segment.  A pixel's loop has stopped <=> T (1 - alpha) < 1e-4, and T
  // only falls: within the entries a wave sees, "alive" is a PREFIX.  So a pixel that is dead on entry (Tf < 1e-4: it died at an
  // earlier entry) is given T = 0 - every weight of the segment is then 0 by itself - and only a segment INSIDE which some pixel
  // of the tile dies needs the per-entry tests (weights masked from the dying entry on, the last transmittance that passed, the
  // number of entries gone through); for the others - all 8 entries alive, or none - one test per lane settles all three.
  auto accum = [&](uint32_t b, float Tf) {
    const int cb = b & 3;
    const bool alive_in = !(Tf < 0.0001f);
    float T = alive_in ? Tf : 0.f;
    float Tn[kFS];
    f2 w[kFS / 2];
    float Tp = T;
#pragma unroll
    for (int u = 0; u < kFS; u += 2) {
      Tn[u] = Tp * om[u >> 1].x;
      Tn[u + 1] = Tn[u] * om[u >> 1].y;
      Tp = Tn[u + 1];
    }
    const bool alive_out = !(Tp < 0.0001f);
    // The weights alpha x (transmittance in front of the entry) are formed AFTER the decision, by the same packed multiply on either
    // side: masked after the fact (a select per weight into fresh values) the two sides met with the weights in different registers
    // and the USUAL side paid four 64-bit register copies per iteration for it.  alpha x 0 = +0 exactly: the same bits as the select.
    if (__any(alive_in && !alive_out)) {  // wave-uniform: some pixel's loop stops inside this segment
      float Tq = T;
#pragma unroll
      for (int u = 0; u < kFS; u += 2) {
        const bool alive0 = !(Tn[u] < 0.0001f), alive1 = !(Tn[u + 1] < 0.0001f);
        w[u >> 1] = al[u >> 1] * f2{alive0 ? Tq : 0.f, alive1 ? Tn[u] : 0.f};
        Tq = Tn[u + 1];
        Tmin = alive0 ? Tn[u] : Tmin;
        Tmin = alive1 ? Tn[u + 1] : Tmin;
        last += (uint32_t)alive0 + (uint32_t)alive1;  // entries this pixel's loop went through (a prefix of the list)
      }
    } else {
      float Tq = T;
#pragma unroll
      for (int u = 0; u < kFS; u += 2) {
        w[u >> 1] = al[u >> 1] * f2{Tq, Tn[u]};
        Tq = Tn[u + 1];
      }
      Tmin = alive_out ? Tp : Tmin;
      last += alive_out ? (uint32_t)kFS : 0u;
    }
#pragma unroll
    for (int u = 0; u < kFS; u += 2) {
      const float4 rg = sRG[cb][(e0 + u) >> 1], be = sBE[cb][(e0 + u) >> 1];
      CR = __builtin_elementwise_fma(f2{rg.x, rg.y}, w[u >> 1], CR);
      CG = __builtin_elementwise_fma(f2{rg.z, rg.w}, w[u >> 1], CG);
      CB = __builtin_elementwise_fma(f2{be.x, be.y}, w[u >> 1], CB);
      if (kExtra) CE = __builtin_elementwise_fma(f2{be.z, be.w}, w[u >> 1], CE);
    }
    // keep stage A where it is written: its sums are not needed before the next iteration, and left alone the compiler sinks this
    // arithmetic below stage E - the old and the new alphas of the segment are then alive together and the loop pays sixteen
    // register copies per iteration for it
    asm volatile("" : "+v"(CR), "+v"(CG), "+v"(CB), "+v"(Tmin), "+v"(last));
    if (kExtra) asm volatile("" : "+v"(CE));
  };
  auto put_records = [&](int sb, float4 q, float2 q2, const float4& c) {  // lane = entry of the batch (park_record: any entry)
    q.z = (-0.5f * kLog2e) * q.z; q.w = (-kLog2e) * q.w; q2.x = (-0.5f * kLog2e) * q2.x;  // to_exp2_domain
    // (kTight: the offset formed here, from an opaque copy of the lane number, every time - held across the loops it was the one
    // value the 80-register instance spilled, and its reload a trip to memory in every tile's blend prologue)
    int ln = lane;
    if (kTight) asm volatile("" : "+v"(ln));
    const int o = (ln >> 1) * 4 + (ln & 1);
    float* xy = reinterpret_cast<float*>(sXY[sb]); float* ab = reinterpret_cast<float*>(sAB[sb]);
    float* co = reinterpret_cast<float*>(sCO[sb]); float* rg2 = reinterpret_cast<float*>(sRG[sb]);
    float* be = reinterpret_cast<float*>(sBE[sb]);
    xy[o] = q.x; xy[o + 2] = q.y; ab[o] = q.z; ab[o + 2] = q.w; co[o] = q2.x; co[o + 2] = q2.y;
    rg2[o] = c.x; rg2[o + 2] = c.y; be[o] = c.z; be[o + 2] = c.w;
  };

  bool done = false;
  if (nbat > b0) {
    // ---- gather pipeline: the wave with (wave - b) % 4 == 0 brings in batch b.  The records of a batch are requested FOUR iterations
    // before they are parked in LDS (and its list ids four iterations before that): a tile that is left alone on its SIMDs runs
    // an iteration in ~0.4 us, less than one trip to HBM - with the loads issued only one iteration ahead the last tiles of
    // every CU ran at memory latency (1.4 us per batch, measured) exactly when nothing else was there to cover it.
    // Prologue (w = the wave's number relative to the first batch): w = 0 / 1 stage batches b0 / b0 + 1 at once and request
    // b0 + 4 / b0 + 5; w = 2 / 3 request b0 + 2 / b0 + 3; everyone evaluates batch b0.
    float4 sg = make_float4(0, 0, 0, 0), sc = sg;
    float2 sg2 = make_float2(0, 0);
    uint32_t id_next = 0;
    // (kTight: the lane number from an opaque copy where the prologue needs it, so that it does not occupy a register across the loop)
    int lp = lane;
    if (kTight) asm volatile("" : "+v"(lp));
    const auto list_id = [&](uint32_t b) { return (b * kFB + lp < n) ? plist[b * kFB + lp] : 0u; };
    if constexpr (kPrimed) {  // w = 0 / 1 request b0 + 4 / b0 + 5, w = 2 / 3 request b0 + 2 / b0 + 3
      if (lp < kFB) {
        const uint32_t* sid = reinterpret_cast<const uint32_t*>(&sP[0][0][0]);
        const auto handed_id = [&](uint32_t b) { return (b * kFB + lp < n) ? sid[b * kFB + lp] : 0u; };
        const uint32_t w = (uint32_t)(wave - (int)b0) & 3u, bq = b0 + (w < 2 ? w + 4 : w);
        const uint32_t idq = handed_id(bq);
        id_next = handed_id(bq + 4);
        stage_batch(geom, rgbc, n, bq * kFB, lane, idq, kExtra, sg, sg2, sc);
      }
    } else if (lp < kFB) {
      const uint32_t w = (uint32_t)(wave - (int)b0) & 3u, bw = b0 + w;
      if (w < 2) {
        const uint32_t id0 = list_id(bw), id4 = list_id(bw + 4);
        id_next = list_id(bw + 8);
        if (bw < nbat) {
          stage_batch(geom, rgbc, n, bw * kFB, lane, id0, kExtra, sg, sg2, sc);
          put_records((int)(bw & 3), sg, sg2, sc);
        }
        stage_batch(geom, rgbc, n, (bw + 4) * kFB, lane, id4, kExtra, sg, sg2, sc);
      } else {
        const uint32_t id2 = list_id(bw);
        id_next = list_id(bw + 4);
        stage_batch(geom, rgbc, n, bw * kFB, lane, id2, kExtra, sg, sg2, sc);
      }
    }
    __syncthreads();
    eval(b0);
    __syncthreads();
    // ---- steady state, iteration i: A(i), E(i+1) | batch i+2 parked in LDS, batch i+6 requested, ids of batch i+10 requested
    for (uint32_t i = b0; i < nbat; ++i) {
      const float P0 = sP[i & 1][0][lane], P1 = sP[i & 1][1][lane], P2 = sP[i & 1][2][lane], P3 = sP[i & 1][3][lane];
      const uint32_t bs = i + 2;
      const bool duty = (wave == (int)(bs & 3)) && (lane < kFB);
      const float t1 = Tb * P0, t2 = t1 * P1, t3 = t2 * P2, t4 = t3 * P3;  // the same chain in every wave
      const bool last_batch = __all(t4 < 0.0001f);  // every pixel has stopped by the end of this batch: no need to evaluate the next
      accum(i, wave == 0 ? Tb : wave == 1 ? t1 : wave == 2 ? t2 : t3);
      if (i + 1 < nbat && !last_batch) eval(i + 1);
      if (duty) {
        if (bs < nbat) put_records((int)(bs & 3), sg, sg2, sc);
        if (bs + 4 < nbat) stage_batch(geom, rgbc, n, (bs + 4) * kFB, lane, id_next, kExtra, sg, sg2, sc);
        id_next = list_id(bs + 8);
      }
      Tb = t4;
      consumed = (i + 1) * kFB;
      __syncthreads();
      if (__all(Tb < 0.0001f)) { done = true; break; }  // bit-identical Tb in all four waves: a workgroup-uniform decision
    }
  }
  s.Tb = Tb; s.Tmin = Tmin; s.CR = CR; s.CG = CG; s.CB = CB; s.CE = CE; s.last = last; s.consumed = consumed;
  return done;
}

// Pair workspace too small (status->overflow): nothing was binned.  Poison the outputs so the condition cannot go unnoticed
// even when the caller defers reading the status block.  Workgroup-uniform result: true = poisoned, nothing to blend.
template <bool kExtra, bool kAlpha = false>
__device__ __forceinline__ bool blend_poisoned(const Params& p, const int v, const int pxi, const int pyi, const bool inside,
                                               const bool known = false) {
  // (the flag may be raised by another tile while this workgroup's waves read it: the decision is taken once for the workgroup)
  __shared__ uint32_t sAnyOverflow[kFwdThreads / 64];
  if (!known && !block_any(p.status->overflow != 0u, sAnyOverflow)) return false;
  const Grid& g = p.g;
  if (threadIdx.x < 64 && inside) {
    const size_t HW = (size_t)g.H * g.W, pix = (size_t)pyi * g.W + pxi;
    const float qnan = __uint_as_float(0x7fc00000u);
    float* oc = p.out_color + (size_t)v * 3 * HW;
    oc[pix] = qnan; oc[HW + pix] = qnan; oc[2 * HW + pix] = qnan;
    if (kExtra) p.out_extra[(size_t)v * HW + pix] = qnan;
    if (kAlpha) p.out_alpha[(size_t)v * HW + pix] = qnan;
    p.final_T[(size_t)v * HW + pix] = 1.f;
    p.n_contrib[(size_t)v * HW + pix] = 0u;
  }
  return true;
}

// The four waves' partial results -> the pixel: image, final transmittance, contributor count; the entries the tile walked.
// kAlpha (GsrForwardOptions.out_alpha): also the accumulated alpha A = 1 - final_T, from the value that is stored - one subtraction and
// one store per pixel in instances of their own; the kAlpha = false instances are the code they were.
template <bool kExtra, bool kAlpha = false>
__device__ __forceinline__ void blend_finish(const Params& p, const int v, const int t, const uint32_t n, BlendFin& lds, const BlendAcc& s,
                                             const int pxi, const int pyi, const bool inside, const float bg0, const float bg1,
                                             const float bg2) {
  auto& sPart = lds.sPart; auto& sLast = lds.sLast;
  const Grid& g = p.g;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  float C0 = s.CR.x + s.CR.y, C1 = s.CG.x + s.CG.y, C2 = s.CB.x + s.CB.y, E = s.CE.x + s.CE.y;  // this wave's partial colour sums
  sPart[wave][0][lane] = C0; sPart[wave][1][lane] = C1; sPart[wave][2][lane] = C2;
  if (kExtra) sPart[wave][3][lane] = E;
  sPart[wave][4][lane] = s.Tmin;
  sLast[wave][lane] = s.last;
  __syncthreads();
  if (wave == 0) {
    if (lane == 0) p.tile_total[(size_t)v * g.T + t] = min(s.consumed, n);  // statistics: list entries this tile walked
    if (inside) {
      float T = s.Tmin;
      uint32_t last = s.last;
#pragma unroll
      for (int h = 1; h < kFwdWaves; ++h) {
        C0 += sPart[h][0][lane]; C1 += sPart[h][1][lane]; C2 += sPart[h][2][lane];
        if (kExtra) E += sPart[h][3][lane];
        T = fminf(T, sPart[h][4][lane]);
        last += sLast[h][lane];
      }
      const size_t HW = (size_t)g.H * g.W, pix = (size_t)pyi * g.W + pxi;
      p.final_T[(size_t)v * HW + pix] = T;
      if (kAlpha) p.out_alpha[(size_t)v * HW + pix] = 1.f - T;
      // the pixel's loop ran through `last` entries before it stopped (every splat it blended has a smaller index; the reference
      // stores the index of the last one it blended - the entries in between are skipped by the alpha < 1/255 test either way)
      p.n_contrib[(size_t)v * HW + pix] = min(last, n);  // (the padding of the last batch counts as alive)
      float* oc = p.out_color + (size_t)v * 3 * HW;
      oc[pix] = C0 + T * bg0;
      oc[HW + pix] = C1 + T * bg1;
      oc[2 * HW + pix] = C2 + T * bg2;
      if (kExtra) p.out_extra[(size_t)v * HW + pix] = E;
    }
  }
}

// The blend of tile t of view v over the index-list range rg (256 threads; `lds` may alias anything the workgroup is done with)
template <bool kExtra, bool kAlpha = false>
__device__ __forceinline__ void blend_tile(const Params& p, const int v, const int t, const uint2 rg, BlendLds& lds) {
  const Grid& g = p.g;
  const int lane = threadIdx.x & 63;
  const int tx = t % g.sgx, ty = t / g.sgx;
  const int pxi = tx * 8 + (lane & 7), pyi = ty * 8 + (lane >> 3);
  const bool inside = pxi < g.W && pyi < g.H;
  const uint32_t n = rg.y - rg.x;
  // the view's background through scalar loads, asked for now: read as `p.views[v].bg` where it is used - in the tile's last
  // instructions - every tile ended with a memory round trip
  typedef const __attribute__((address_space(4))) float* cfptr;
  cfptr camc = reinterpret_cast<cfptr>(reinterpret_cast<uintptr_t>(p.views + __builtin_amdgcn_readfirstlane(v)));
  const float bg0 = camc[37], bg1 = camc[38], bg2 = camc[39];  // GsrView::bg
  if (blend_poisoned<kExtra, kAlpha>(p, v, pxi, pyi, inside)) return;
  const bool dbg = GSR_ABL(p.d.flags, GSR_FLAG_DEBUG_TIMING);
  unsigned long long tm0 = 0, rt0 = 0;
  if (dbg) { tm0 = __builtin_readcyclecounter(); rt0 = __builtin_amdgcn_s_memrealtime(); }
  BlendAcc acc;
  acc.Tb = inside ? 1.f : 0.f; acc.Tmin = 1.f;
  acc.CR = f2{0.f, 0.f}; acc.CG = acc.CR; acc.CB = acc.CR; acc.CE = acc.CR;
  acc.last = 0; acc.consumed = 0;
  (void)blend_range<kExtra>(p.geom + (size_t)v * p.d.num_gaussians, p.rgbc + (size_t)v * p.d.num_gaussians, p.point_list + rg.x, n, 0u,
                            (n + kFB - 1) / kFB, lds, acc, (float)pxi, (float)pyi);
  if (dbg && threadIdx.x == 0) {
    unsigned long long* o = dbg_stamps(p, 24576 + (size_t)v * g.T + t);  // (NOT over the binning workgroups' key slots: with more than one
    //                                        resident round a later tile still gathers from them when an earlier one stamps)
    // where it ran: HW_ID (id 4: wave, simd, pipe, cu, sh, se ...) and XCC_ID (id 20), 16 bits each
    const unsigned hw = (__builtin_amdgcn_s_getreg(4 | (0 << 6) | (15 << 11)) & 0xffffu) |
                        ((__builtin_amdgcn_s_getreg(20 | (0 << 6) | (15 << 11)) & 0xfu) << 16);
    o[0] = tm0; o[1] = ((unsigned long long)hw << 32); o[2] = __builtin_readcyclecounter();
    o[3] = (rt0 << 32) | (__builtin_amdgcn_s_memrealtime() & 0xffffffffull);  // 100 MHz wall clock: start | end
  }
  blend_finish<kExtra, kAlpha>(p, v, t, n, *reinterpret_cast<BlendFin*>(&lds + 1), acc, pxi, pyi, inside, bg0, bg1, bg2);
}

// One launch per tile for both: the tile's sort (its gather latency under the blend arithmetic of the other tiles of the CU),
// then - the index list written and a barrier later - its blend, over the same LDS.
#ifndef GSR_TF_WAVES
#define GSR_TF_WAVES 6
#endif
#ifndef GSR_WINDOWED_SHORT
#define GSR_WINDOWED_SHORT 600  // pair capacity per tile up to which the windowed chain sorts with the 2048-key variant
#endif
template <bool kGather, int kLds, bool kExtra, bool kAlpha = false>
__global__ __launch_bounds__(kFwdThreads, (kLds == 2048 && kGather && !kExtra) ? GSR_TF_WAVES : 4) void k_tile_fwd(const Params p) {
  static_assert(kSortThreads == kFwdThreads, "one workgroup shape for the two phases");
  constexpr int kSortWords = SortLds<kLds>::kWords, kBlendWords = (int)((sizeof(BlendLds) + sizeof(BlendFin) + 7) / 8);
  __shared__ __attribute__((aligned(16))) unsigned long long smem[kSortWords > kBlendWords ? kSortWords : kBlendWords];
  __shared__ uint32_t red[8];
  __shared__ uint32_t sInfo[4];
  const uint32_t bid = blockIdx.x;
  // The sort phase is a chain of short instruction bursts between trips to memory and LDS; the blend phase of the other tiles of
  // the CU (de-phased: they are up to 5 us ahead) keeps the SIMDs issuing every cycle.  A wave in its sort phase goes first
  // when both are ready: its next request leaves at once and the blend waves lose nothing they would not lose later (-0.7 us).
  const int tg = kGather ? fwd_tile_of(p, fwd_tile_word(p, bid)) : (int)bid;  // (one place for the sort and the blend)
  __builtin_amdgcn_s_setprio(2);
  const uint2 rg = sort_tile<kGather, kLds>(p, bid, tg, smem, red, sInfo);
  __builtin_amdgcn_s_setprio(0);
  if (bid == 0 && threadIdx.x == 0) *p.page_counter = (unsigned long long)p.call_tag << 32;  // the binning launch's (take_pages)
  __syncthreads();  // the list is this workgroup's own: its stores are visible to its waves from here on; the keys are dead
  const int v = tg / p.g.T;
  blend_tile<kExtra, kAlpha>(p, v, tg - v * p.g.T, rg, *reinterpret_cast<BlendLds*>(smem));
  if (kGather && threadIdx.x == 64 && rg.y - rg.x > p.status->max_list) atomicMax(&p.status->max_list, rg.y - rg.x);
}

// ------------------------------------------------------------------------------------------------
// K2 for the usual case (round 4): fused binning, at most kSortThreads binning rows, lists that sit in their slots of at most 2048
// entries.  Same results as k_tile_fwd<true, 2048, .>, two things done differently:
//   * gather without the scan over the rows: a row's run takes its place in the LDS key array with one LDS atomic on a cursor
//     (the order of the runs does not matter - the sort that follows is total), the depth range of the tile is taken from the keys
//     as they pass through the copying thread's registers, and the bucket histogram is filled in the pass that brings the keys
//     back into registers: two block-wide phases (and four barriers) fewer than sort_tile before the first key is in its bucket;
//   * PREFIX RANK.  A tile of the 300 k / 256 x 256 workload lists ~1220 splats and its blend walks 224-448 of them (measured:
//     every pixel's transmittance is below 1e-4 by then; tools/sim_tiles.py replays it on the CPU).  Buckets are in depth order,
//     so after the scatter the first kPrefix positions of the key array hold exactly the kPrefix nearest splats: only those are
//     ranked (the quadratic-in-bucket-size part of the sort) and written to the index list before the blend starts.  The key
//     array and the bucket cursors stay in LDS beside the blend's own area; a tile whose pixels are still open when the prefix is
//     used up ranks the rest then and goes on (an outer loop around the blend's range, the batch loop itself is untouched).  The
//     backward reads a tile's list up to the largest contributor count of its pixels, which lies inside what was ranked.
//     GSR_FLAG_FULL_LISTS ranks everything at once (tests that look at the whole list).
// Everything unusual - a run that was not stored, a list longer than its slot or than the LDS array, a degenerate depth
// distribution - goes through sort_tile<true, 2048> as before (the workgroup starts over: rare).
// ------------------------------------------------------------------------------------------------
#ifndef GSR_PREFIX
#define GSR_PREFIX 512
#endif
#ifndef GSR_DEPHASE_SLEEP
#define GSR_DEPHASE_SLEEP 16  // s_sleep argument between the four de-phase groups of k_tile_fwd_prefix's first resident round (~0.5 us).
#endif                        // Round 6, 0 / 8 / 16 / 32 / 48: headline 52.55 / 52.5 / 52.3 / 52.4 / 52.5 us, one 131 072-Gaussian view
                              // 41.7 / 41.65 / 41.4 / 42.0 / 42.3, the same on the pixel-aligned scene 47.9 / 47.8 / 48.2 / 49.2 / 49.5
#ifndef GSR_LONG_RUN
#define GSR_LONG_RUN 24  // runs of more keys than this are copied by the whole workgroup (k_tile_fwd_prefix)
#endif
#ifndef GSR_RUN_STEP
#define GSR_RUN_STEP 18  // keys of a short run requested together (k_tile_fwd_prefix, the instances built for four waves per SIMD)
#endif
constexpr int kPrefix = GSR_PREFIX;  // list positions ranked before the blend starts (a multiple of kFB)
static_assert(kPrefix % kFB == 0 && kPrefix >= 2 * kFB, "the prefix is whole batches");

// The rare paths of k_tile_fwd_prefix (inlined: as real calls - `noinline` - `Params` travels by reference, 480 B of scratch per lane
// and 108-112 VGPRs for a path that is almost never taken: forward 84 us)
__device__ __forceinline__ uint2 sort_tile_general_2048(const Params& p, const uint32_t bid, const int tg, unsigned long long* smem, uint32_t* red, uint32_t* sInfo) {
  return sort_tile<true, 2048>(p, bid, tg, smem, red, sInfo);
}
__device__ __forceinline__ void bitonic_whole_list(unsigned long long* sk, uint32_t* out, const int n) {
  int lgnp = 1;
  while ((1 << lgnp) < n) ++lgnp;
  bitonic_block(sk, n, lgnp, (int)threadIdx.x);
  for (int k = threadIdx.x; k < n; k += kSortThreads) out[k] = (uint32_t)sk[k];
}

#ifndef GSR_PF_COMPACT_MIN_TILES
#define GSR_PF_COMPACT_MIN_TILES (5 * kCUs)  // calls with more tiles than this take the compact instance
#endif
// kCompact (calls with more tiles than the chip holds at once: many views): 1024 depth buckets instead of 2048, their counters /
// cursors packed two to a 32-bit word (a cursor is at most 2048: sixteen bits; the LDS atomic adds 1 or 1 << 16) - 25.7 KB of LDS
// instead of 31.9, and the instance is built for six waves per SIMD (80 VGPRs): SIX workgroups per CU instead of five.  The single
// view (1024 tiles = four per CU) has nothing to gain from that and keeps its instance untouched.
template <bool kExtra, bool kCompact, bool kAlpha = false>
__global__ __launch_bounds__(kFwdThreads, kCompact ? 6 : 4) void k_tile_fwd_prefix(const Params p) {
  constexpr int kLds = 2048;
  constexpr int kBk = kCompact ? 1024 : SortLds<kLds>::kBuckets, kBkBits = kCompact ? 10 : SortLds<kLds>::kBucketBits, kBpt = kBk / kSortThreads;
  constexpr int Q = kLds / kSortThreads;
  // keys | bucket counters, then cursors | (kCompact) the blend's area - one array, so that the general path (sort_tile: 24 KB from
  // the start, its blend over its dead keys) finds its room in it
  constexpr int kCounterWords = kCompact ? kBk / 4 : kBk / 2;  // 8-byte words
  constexpr int kBlendWordsP = (int)((sizeof(BlendLds) + 7) / 8);
  constexpr int kFastWords = kLds + kCounterWords + (kCompact ? kBlendWordsP : 0);
  __shared__ __attribute__((aligned(16))) unsigned long long smem[kFastWords > SortLds<kLds>::kWords ? kFastWords : SortLds<kLds>::kWords];
  // NOT over the keys: a tile may come back to rank the rest of its list
  __shared__ __attribute__((aligned(16))) unsigned long long blds_own[kCompact ? 2 : kBlendWordsP];
  BlendLds& blds = *reinterpret_cast<BlendLds*>(kCompact ? smem + kLds + kCounterWords : blds_own);
  __shared__ uint32_t red[8];
  __shared__ uint32_t sInfo[4];
  __shared__ uint32_t sCount, sLongRuns, sLongKeys;
  const uint32_t bid = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  // the workgroup's tile, asked for as the kernel's first memory operation: a word of its own, on its way while the de-phase
  // groups sleep.  (The compact instance takes calls of more than one resident round: image order.)
  const uint32_t tile_word = kCompact ? (uint32_t)xcd_remap((int)bid, (int)p.sort_blocks) : fwd_tile_word(p, bid);
  // (overflow is raised by tiles of THIS launch only - a tile that cannot place its list - and such a tile poisons its own pixels
  // whatever it read here; for everybody else the flag is a courtesy whose outcome depends on timing either way)
  uint32_t overflow_early = 0;
  if (tid == 0) overflow_early = p.status->overflow;  // (asked for at the kernel's start, not between the sort and the blend)
  unsigned long long* sk = smem;
  uint32_t* hist = reinterpret_cast<uint32_t*>(smem + kLds);
  uint32_t* cur = hist;
  // bucket b's counter / cursor: a word of its own, or (kCompact) half of word b >> 1
  auto bump = [&](uint32_t b) -> uint32_t {  // returns the value before
    if (!kCompact) return atomicAdd(&cur[b], 1u);
    const uint32_t sh = (b & 1u) * 16u;
    return (atomicAdd(&cur[b >> 1], 1u << sh) >> sh) & 0xffffu;
  };
  auto cur_of = [&](uint32_t b) -> uint32_t { return kCompact ? (cur[b >> 1] >> ((b & 1u) * 16u)) & 0xffffu : cur[b]; };
  const bool dbg = GSR_ABL(p.d.flags, GSR_FLAG_DEBUG_TIMING);
  unsigned long long* stamp = dbg_stamps(p, 8192 + bid);
  unsigned long long* stamp2 = dbg_stamps(p, 8192 + p.sort_blocks + bid);
  __builtin_amdgcn_s_setprio(2);
  GSR_STAMP(0);
  const int T = p.g.T, R = p.rows;
  // (de-phasing of the first resident round: see sort_tile.  With this kernel's shorter gather 1 us between the four groups is
  // enough: sleeps of 16 / 24 / 32 / 40 / 64 gave 53.0 / 52.9 / 53.0 / 53.0 / 53.9 us for the forward; round 6: 16 - GSR_DEPHASE_SLEEP)
  if (bid < 1024u)
    for (int q = 0; q < (int)((bid >> kDephaseShift) % kDephaseGroups); ++q) __builtin_amdgcn_s_sleep(GSR_DEPHASE_SLEEP);
  const int tg = fwd_tile_of(p, tile_word);
  const int v = tg / T, t = tg - v * T;
  // ---- gather: column (v, :, t) of the pair matrix, one row per thread
  uint2 e0 = make_uint2(0u, 0u);
  uint32_t bb0 = 0;
  if (tid < R) {
    e0 = p.pair_mat[((size_t)v * R + tid) * ((size_t)T + 8) + t];
    bb0 = p.blk_base[(size_t)v * R + tid];
  }
  for (int k = tid; k < (kCompact ? kBk / 2 : kBk); k += kSortThreads) hist[k] = 0;  // (while the column is on its way)
  if (tid == 0) { sCount = 0; sLongRuns = 0; sLongKeys = 0; }
  __syncthreads();
  GSR_STAMP2(0);
  const bool has = e0.y != 0u, miss = has && bb0 == 0xffffffffu;
  // a run's place in the key array: the wave's runs side by side (DPP scan of the counts), the wave's block from ONE atomic on
  // the cursor - 247 lanes adding to the same LDS word are processed one lane after the other and hold up the LDS pipeline of
  // the whole CU while they are (measured: the per-lane form made every LDS phase of every tile on the CU 2-3 x slower)
  const uint32_t incl = wave_inclusive_scan_u32(e0.y);
  uint32_t wbase = 0;
  if (lane == 63 && incl) wbase = atomicAdd(&sCount, incl);
  wbase = (uint32_t)__builtin_amdgcn_readlane((int)wbase, 63);
  const uint32_t start0 = wbase + incl - e0.y;
  const bool fits = start0 + e0.y <= (uint32_t)kLds;
  GSR_STAMP2(1);
  uint32_t lo = 0xffffffffu, hi = 0u;
  auto take = [&](unsigned long long* d, unsigned long long key) {
    *d = key;
    const uint32_t dep = (uint32_t)(key >> 32);
    lo = dep < lo ? dep : lo;
    hi = dep > hi ? dep : hi;
  };
  // LONG runs (round 6).  Gaussians that arrive in the raster order of the images they were predicted from - what PF3plat's encoder
  // emits - put a binning workgroup's whole chunk into a narrow band of the target view: a tile then draws its list from a handful of
  // rows, 50-200 keys each, and one thread copying such a run six keys per round trip was the longest phase of the tile (10.4 us
  // "runs to LDS" against 1.4-2.0 on the independently drawn scene: profiles/r06_a_stamps_config4_structured.txt).  A run of more
  // than kLongRun keys is therefore not copied by its thread: the thread leaves a descriptor (source, place, length, running total)
  // in LDS - the blend's area, idle until the blend - and behind the barrier all 256 threads copy the long runs' keys side by side,
  // every load of a thread requested before its first store.  Short runs (every run of the independently drawn scenes) go as before.
  constexpr uint32_t kLongRun = GSR_LONG_RUN;
  uint4* ldesc = reinterpret_cast<uint4*>(&blds);  // up to kLds / kLongRun descriptors of 16 bytes
  static_assert(sizeof(BlendLds) >= (size_t)(kLds / GSR_LONG_RUN + 1) * 16, "descriptors of the long runs fit the blend's area");
  const bool is_long = has && !miss && fits && e0.y > kLongRun;
  if (__any((int)is_long)) {  // wave-uniform
    const uint32_t lcnt = is_long ? e0.y : 0u;
    const uint32_t lincl = wave_inclusive_scan_u32(lcnt);
    const unsigned long long lmask = __ballot((int)is_long);
    uint32_t kbase = 0, dbase = 0;
    if (lane == 63) {
      kbase = atomicAdd(&sLongKeys, lincl);
      dbase = atomicAdd(&sLongRuns, (uint32_t)__popcll(lmask));
    }
    kbase = (uint32_t)__builtin_amdgcn_readlane((int)kbase, 63);
    dbase = (uint32_t)__builtin_amdgcn_readlane((int)dbase, 63);
    if (is_long)
      ldesc[dbase + (uint32_t)__popcll(lmask & ((1ull << lane) - 1ull))] = make_uint4(bb0 + e0.x, start0, e0.y, kbase + lincl - lcnt);
  }
  if (!kCompact && has && !miss && fits && !is_long) {
    // kRunStep keys per step as 16-byte loads ALL requested before the first key is parked: a step is one round trip to
    // memory (~1 us under this launch's load) and the four resident tiles of a CU are in this phase together, with nothing to hide
    // it.  Runs average 5 keys but one in four is longer than 6: at six keys per step practically every wave made two dependent
    // trips and half the tiles three.  The loads may run one key past the run (the buffer is padded), never further.
    constexpr uint32_t kRunStep = GSR_RUN_STEP;
    static_assert(kRunStep % 2 == 0 && kRunStep >= 6, "whole 16-byte loads");
    const unsigned long long* src = p.keys + bb0 + e0.x;
    unsigned long long* d0 = sk + start0;
    for (uint32_t j = 0; j < e0.y; j += kRunStep) {
      ull2 r[kRunStep / 2];
#pragma unroll
      for (uint32_t u = 0; u < kRunStep / 2; ++u) {
        r[u] = ull2{0ull, 0ull};
        if (j + 2 * u < e0.y) r[u] = *reinterpret_cast<const ull2*>(src + j + 2 * u);
      }
      unsigned long long* d = d0 + j;
#pragma unroll
      for (uint32_t u = 0; u < kRunStep / 2; ++u) {
        if (j + 2 * u < e0.y) take(d + 2 * u, r[u].x);
        if (j + 2 * u + 1 < e0.y) take(d + 2 * u + 1, r[u].y);
      }
    }
  }
  if (kCompact && has && !miss && fits && !is_long) {  // (the 80-register instance: six keys per step, as it was)
    // six keys per step as three 16-byte loads issued together; the loads may run one key past the run (the buffer is padded)
    const unsigned long long* src = p.keys + bb0 + e0.x;
    unsigned long long* d0 = sk + start0;
    for (uint32_t j = 0; j < e0.y; j += 6) {
      const ull2 a = *reinterpret_cast<const ull2*>(src + j);
      ull2 b = {0ull, 0ull}, c = {0ull, 0ull};
      if (j + 2 < e0.y) b = *reinterpret_cast<const ull2*>(src + j + 2);
      if (j + 4 < e0.y) c = *reinterpret_cast<const ull2*>(src + j + 4);
      unsigned long long* d = d0 + j;
      take(d, a.x);
      if (j + 1 < e0.y) take(d + 1, a.y);
      if (j + 2 < e0.y) take(d + 2, b.x);
      if (j + 3 < e0.y) take(d + 3, b.y);
      if (j + 4 < e0.y) take(d + 4, c.x);
      if (j + 5 < e0.y) take(d + 5, c.y);
    }
  }
  hi = wave_max_u32(hi);
  lo = ~wave_max_u32(~lo);
  if (lane == 0) { red[wave] = lo; red[4 + wave] = hi; }
  if (tid == 0) sInfo[3] = overflow_early;
  __shared__ uint32_t sAnyBad[kSortThreads / 64];
  const bool bad = block_any(miss || (has && !fits), sAnyBad);
  if (sLongRuns != 0u) {  // workgroup-uniform (written before the barrier inside block_any)
    const uint32_t nruns = sLongRuns, nkeys = sLongKeys;
    // flat index f over the long runs' keys -> (run, position): the descriptors carry their running total; a thread's up to Q keys are
    // independent loads, all requested before the first of them is stored
    constexpr int QL = kLds / kSortThreads;
    unsigned long long kv[QL];
    uint32_t dst[QL];
    uint32_t r = 0;
    uint4 dsc = ldesc[0];
#pragma unroll
    for (int q = 0; q < QL; ++q) {
      const uint32_t f = (uint32_t)tid + (uint32_t)q * kSortThreads;
      dst[q] = 0xffffffffu;
      kv[q] = 0ull;
      if (f < nkeys) {
        // (descriptor slots were handed out wave by wave, so their running totals are not sorted: search them all - there are few)
        if (!(f >= dsc.w && f - dsc.w < dsc.z)) {
          for (r = 0; r < nruns; ++r) {
            dsc = ldesc[r];
            if (f >= dsc.w && f - dsc.w < dsc.z) break;
          }
        }
        kv[q] = p.keys[(size_t)dsc.x + (f - dsc.w)];
        dst[q] = dsc.y + (f - dsc.w);
      }
    }
    uint32_t lo2 = 0xffffffffu, hi2 = 0u;
#pragma unroll
    for (int q = 0; q < QL; ++q)
      if (dst[q] != 0xffffffffu) {
        sk[dst[q]] = kv[q];
        const uint32_t dep = (uint32_t)(kv[q] >> 32);
        lo2 = dep < lo2 ? dep : lo2;
        hi2 = dep > hi2 ? dep : hi2;
      }
    hi2 = wave_max_u32(hi2);
    lo2 = ~wave_max_u32(~lo2);
    if (lane == 0) { red[wave] = min(red[wave], lo2); red[4 + wave] = max(red[4 + wave], hi2); }  // (this lane wrote them above)
    __syncthreads();  // the long runs' keys are in place, the depth range covers them
  }
  GSR_STAMP2(2);
  GSR_STAMP(1);
  uint32_t n = sCount, ranked = 0, obase = (uint32_t)tg * p.stride;
  uint32_t dlo = 0;
  int shift = 0;
  bool fast_path = false;
  bool bucketed = false;  // the keys sit in bucket order in `sk`, cur[b] = end of bucket b: positions are ranked on demand
  if (bad || n > p.stride) {  // workgroup-uniform: the general path, from the start
    __syncthreads();
    const uint2 rg = sort_tile_general_2048(p, bid, tg, smem, red, sInfo);
    obase = rg.x; n = rg.y - rg.x; ranked = n;
  } else {
    if (tid == 0) p.ranges[tg] = make_uint2(obase, obase + n);
    fast_path = true;
    uint32_t* out = p.point_list + obase;
    if (n == 1) {
      if (tid == 0) out[0] = (uint32_t)sk[0];
      ranked = 1;
    } else if (n > 1) {
      dlo = min(min(red[0], red[1]), min(red[2], red[3]));
      const uint32_t dhi = max(max(red[4], red[5]), max(red[6], red[7]));
      const uint32_t range = dhi - dlo;
      shift = range < (uint32_t)kBk ? 0 : (32 - __clz((int)range)) - kBkBits;
      unsigned long long kreg[Q];
#pragma unroll
      for (int q = 0; q < Q; ++q) {
        const int k = tid + q * kSortThreads;
        kreg[q] = (k < (int)n) ? sk[k] : ~0ull;
        if (k < (int)n) (void)bump(((uint32_t)(kreg[q] >> 32) - dlo) >> shift);
      }
      __syncthreads();
      GSR_STAMP(2);
      // exclusive scan of the bucket counts: thread t owns kBpt consecutive buckets
      uint32_t c[kBpt], span = 0, cmax = 0;
#pragma unroll
      for (int q = 0; q < kBpt; ++q) { c[q] = cur_of((uint32_t)(kBpt * tid + q)); span += c[q]; cmax = max(cmax, c[q]); }
      uint32_t total;
      uint32_t start = block_exclusive_scan(span, red, tid, total);
      if (kCompact) {  // (a thread's kBpt buckets are whole words; nobody else touches them between the two barriers)
#pragma unroll
        for (int q = 0; q < kBpt; q += 2) {
          const uint32_t s0 = start, s1 = start + c[q];
          cur[(kBpt * tid + q) >> 1] = s0 | (s1 << 16);
          start = s1 + c[q + 1];
        }
      } else {
#pragma unroll
        for (int q = 0; q < kBpt; ++q) { cur[kBpt * tid + q] = start; start += c[q]; }
      }
      __shared__ uint32_t sAnyBig2[kSortThreads / 64];
      const bool big = block_any(cmax > (uint32_t)kSpanMax, sAnyBig2);
      GSR_STAMP(3);
      if (big) {  // degenerate depth distribution: the bitonic network on the same array, whole list
        bitonic_whole_list(sk, out, (int)n);
        ranked = n;
      } else {
        // scatter into bucket order (every key is in a register: in place)
#pragma unroll
        for (int q = 0; q < Q; ++q)
          if (tid + q * kSortThreads < (int)n) {
            const uint32_t slot = bump(((uint32_t)(kreg[q] >> 32) - dlo) >> shift);
            sk[slot] = kreg[q];
          }
        __syncthreads();
        GSR_STAMP(4);
        // after the scatter cur[b] is the END of bucket b.  Rank the buckets that reach into the first kPrefix positions
        ranked = n;
        if (!(p.d.flags & GSR_FLAG_FULL_LISTS) && n > (uint32_t)(kPrefix + kPrefix / 4))
          ranked = cur_of(((uint32_t)(sk[kPrefix - 1] >> 32) - dlo) >> shift);
        bucketed = true;
      }
    }
  }
  // finish by ranking: every entry counts the smaller keys of its own bucket (keys are unique: they carry the Gaussian index) and goes
  // straight to its final slot in the global list; four bucket members per step, requested together
  // `prime` (the first rank pass of the instances built for four waves per SIMD): the pass knows every entry's final position
  // and its Gaussian in the same thread, so what the blend's prologue would fetch through the list goes to it through LDS - the
  // ids of positions < kPrimedIds, and the RECORDS of batches 0 and 1, requested here (their trip to memory runs under the rest of
  // this pass) and parked where put_records parks them; positions from k1 on inside those two batches get the null record.
  // A position below 2 kFB is ranked by a thread's FIRST key: a key and its rank lie in the same bucket of at most kSpanMax keys.
  static_assert(kSpanMax + 2 * kFB <= kSortThreads, "a thread holds at most one record of batches 0 and 1");
  auto rank_positions = [&](uint32_t k0, uint32_t k1, const bool prime) {
    const GeomRec* geom = p.geom + (size_t)v * p.d.num_gaussians;  // (used under `prime` only)
    const float4* rgbc = p.rgbc + (size_t)v * p.d.num_gaussians;
    uint32_t* out = p.point_list + obase;
    uint32_t* sid = reinterpret_cast<uint32_t*>(&blds.sP[0][0][0]);
    float4 hg = make_float4(0, 0, 0, 0), hc = hg;
    float2 hg2 = make_float2(0, 0);
    int held = -1;
    for (int k = (int)k0 + tid; k < (int)k1; k += kSortThreads) {
      const unsigned long long key = sk[k];
      const uint32_t b = ((uint32_t)(key >> 32) - dlo) >> shift;
      const int bs = b ? (int)cur_of(b - 1) : 0, be = (int)cur_of(b);
      int rank = bs;
      for (int j = bs; j < be; j += 4) {
        const unsigned long long k0_ = sk[j], k1_ = sk[min(j + 1, be - 1)], k2_ = sk[min(j + 2, be - 1)], k3_ = sk[min(j + 3, be - 1)];
        rank += (k0_ < key ? 1 : 0) + ((j + 1 < be && k1_ < key) ? 1 : 0) + ((j + 2 < be && k2_ < key) ? 1 : 0) +
                ((j + 3 < be && k3_ < key) ? 1 : 0);
      }
      out[rank] = (uint32_t)key;
      if (prime) {
        if (rank < kPrimedIds) sid[rank] = (uint32_t)key;
        if (rank < 2 * kFB) {
          stage_batch(geom, rgbc, 1u, 0u, 0, (uint32_t)key, kExtra, hg, hg2, hc);
          held = rank;
        }
      }
    }
    if (prime) {
      if (held >= 0) park_record(blds, held / kFB, held % kFB, hg, hg2, hc);
      if (tid < 2 * kFB && tid >= (int)k1) park_record(blds, tid / kFB, tid % kFB, make_float4(0, 0, 0, 0), make_float2(0, 0), make_float4(0, 0, 0, 0));
    }
  };
  const bool primed = !kCompact && bucketed;  // workgroup-uniform
  if (bucketed) rank_positions(0u, ranked, primed);
  GSR_STAMP(5);
  GSR_STAMP(6);
  __builtin_amdgcn_s_setprio(0);
  if (bid == 0 && tid == 0) *p.page_counter = (unsigned long long)p.call_tag << 32;  // the binning launch's (take_pages)
  __syncthreads();  // the list is this workgroup's own: its stores are visible to its waves from here on
  // ---- blend: the ranked prefix (whole batches of it), then - only if some pixel is still open - the rest
  const Grid& g = p.g;
  const int tx = t % g.sgx, ty = t / g.sgx;
  const int pxi = tx * 8 + (lane & 7), pyi = ty * 8 + (lane >> 3);
  const bool inside = pxi < g.W && pyi < g.H;
  typedef const __attribute__((address_space(4))) float* cfptr;
  cfptr camc = reinterpret_cast<cfptr>(reinterpret_cast<uintptr_t>(p.views + __builtin_amdgcn_readfirstlane(v)));
  const float bg0 = camc[37], bg1 = camc[38], bg2 = camc[39];  // GsrView::bg
  // the longest list so far (statistics for the caller's sizing): as the tile's LAST memory operation.  Where sort_tile has it -
  // between the gather and the next barrier - a barrier's wait for outstanding memory operations includes this load and, for the
  // first tiles to arrive, a device-scope atomic on an address every tile of the launch goes for
  auto report_length = [&]() {
    if (fast_path && tid == 64 && n > p.status->max_list) atomicMax(&p.status->max_list, n);
    if (fast_path && bid == 0) {  // total pair count = sum of the binning workgroups' totals (a general-path tile has done it in sort_tile)
      unsigned long long part = 0;
      for (int k = tid; k < p.d.num_views * R; k += kSortThreads) part += p.blk_total[k];
      for (int o = 32; o > 0; o >>= 1) part += __shfl_down(part, o, 64);
      __shared__ unsigned long long sPartSum[kSortThreads / 64];
      if (lane == 0) sPartSum[wave] = part;
      __syncthreads();
      if (tid == 0) p.status->num_pairs = sPartSum[0] + sPartSum[1] + sPartSum[2] + sPartSum[3];
    }
  };
  // (usual path: the flag as thread 0 read it at the kernel's start, handed round through LDS - the same value in every wave)
  if (fast_path ? (sInfo[3] != 0u && blend_poisoned<kExtra, kAlpha>(p, v, pxi, pyi, inside, true))
                                          : blend_poisoned<kExtra, kAlpha>(p, v, pxi, pyi, inside)) {
    report_length();
    return;
  }
  unsigned long long tm0 = 0, rt0 = 0;
  if (dbg) { tm0 = __builtin_readcyclecounter(); rt0 = __builtin_amdgcn_s_memrealtime(); }
  BlendAcc acc;
  acc.Tb = inside ? 1.f : 0.f; acc.Tmin = 1.f;
  acc.CR = f2{0.f, 0.f}; acc.CG = acc.CR; acc.CB = acc.CR; acc.CE = acc.CR;
  acc.last = 0; acc.consumed = 0;
  const GeomRec* geom = p.geom + (size_t)v * p.d.num_gaussians;
  const float4* rgbc = p.rgbc + (size_t)v * p.d.num_gaussians;
  const uint32_t* plist = p.point_list + obase;
  const uint32_t nbat = (n + kFB - 1) / kFB;
  uint32_t b0 = 0;
#pragma clang loop unroll(disable)
  for (int pass = 0; pass < 2; ++pass) {
    // pass 0: the whole batches inside the ranked prefix (all of the list when everything was ranked); pass 1: from there to the end
    const bool whole = ranked >= n;
    const uint32_t b1 = whole ? nbat : ranked / kFB;
    // (the primed entry as an instantiation of its own beside the ordinary one, which the second pass takes: the ordinary one is
    // also k_tile_fwd's, and stays the code it was)
    const uint32_t nb = whole ? n : b1 * kFB;
    bool done = (primed && pass == 0) ? blend_range<kExtra, kCompact, !kCompact>(geom, rgbc, plist, nb, b0, b1, blds, acc, (float)pxi, (float)pyi)
                                      : blend_range<kExtra, kCompact>(geom, rgbc, plist, nb, b0, b1, blds, acc, (float)pxi, (float)pyi);
    done = done || whole || __all(acc.Tb < 0.0001f);  // (Tb: the same bits in all four waves)
    if (done) break;
    __builtin_amdgcn_s_setprio(2);
    rank_positions(ranked, n, false);
    __builtin_amdgcn_s_setprio(0);
    ranked = n;
    b0 = b1;
    __syncthreads();
  }
  if (dbg && tid == 0) {
    unsigned long long* o = dbg_stamps(p, 24576 + (size_t)v * g.T + t);  // (NOT over the binning workgroups' key slots: with more than one
    //                                        resident round a later tile still gathers from them when an earlier one stamps)
    const unsigned hw = (__builtin_amdgcn_s_getreg(4 | (0 << 6) | (15 << 11)) & 0xffffu) |
                        ((__builtin_amdgcn_s_getreg(20 | (0 << 6) | (15 << 11)) & 0xfu) << 16);
    o[0] = tm0; o[1] = ((unsigned long long)hw << 32); o[2] = __builtin_readcyclecounter();
    o[3] = (rt0 << 32) | (__builtin_amdgcn_s_memrealtime() & 0xffffffffull);  // 100 MHz wall clock: start | end
  }
  // (the keys are dead: their last reader is rank_positions, a barrier ago at least)
  if (kCompact) {  // the pixel's coordinates formed again (opaque lane number) instead of held across the loops: 80 registers
    int ln = lane;
    asm volatile("" : "+v"(ln));
    const int qx = tx * 8 + (ln & 7), qy = ty * 8 + (ln >> 3);
    blend_finish<kExtra, kAlpha>(p, v, t, n, *reinterpret_cast<BlendFin*>(smem), acc, qx, qy, qx < g.W && qy < g.H, bg0, bg1, bg2);
  } else {
    blend_finish<kExtra, kAlpha>(p, v, t, n, *reinterpret_cast<BlendFin*>(smem), acc, pxi, pyi, inside, bg0, bg1, bg2);
  }
  report_length();
  (void)sInfo;
}

}  // namespace gsr
