// Exact softmax sampling over the whole catalog without a [B, N] matrix (gfx950).
//
//   BaseRetriever.sampling(method='brute')    baseretriever.py:299-328
//   RetrieverSampler.forward                  recstudio/ann/sampler.py:61-78 (goes through the first)
//
// The reference scores into [B, N-1], divides by t, takes the softmax, pads to [B, N], optionally scatters zeros over the user's
// history, draws with torch.multinomial and takes log(gather(...)).  Here the same distribution is drawn by a two-level inverse
// CDF over item BLOCKS of SS_G consecutive ids (block g = items 1 + g * SS_G ...), and whatever is needed twice is recomputed
// instead of stored: the extra memory is 16 bytes per (query, block).
//
//   1. ss_block_kernel   one fp32-MFMA pass over the catalog, the orientation of fullscore_kernel (items = A operand, queries = B
//                        operand, a lane owns one query column, K permuted so that a lane's operands are contiguous floats, 32-item
//                        tiles staged through LDS and shared by the 4 waves of a 128-query workgroup).  The tile epilogue turns the
//                        dot products into the score (cosine / Euclidean as RSA_SCORE_COS / RSA_SCORE_EUC of rsa_fullscore, then
//                        * inv_t) and keeps an online (max, sum exp) per lane that is folded and written every SS_G items: one
//                        record (m_g, s_g) per (query, block).  ONE pass: the logsumexp falls out of the records, so the second
//                        product a "known lse first" form needs is saved; the records cost two registers, no wave is lost.
//   2. ss_merge_kernel   one wave per query, fixed order: M = max m_g, lse = M + log(sum s_g exp(m_g - M)), mass[g] = s_g exp(m_g - lse).
//   3. ss_hist_kernel    (history given) one wave per (query, history slot); the first slot of every block the history touches
//                        re-sums that block with the in-block routine below, the history items left out -- no subtraction of p_h
//                        (cancellation; a duplicated id would count twice).  A block wholly inside the history sums to exactly 0.
//   4. ss_scan_kernel    cum[g] = running sum of mass, taken in fixed point (a power-of-two unit chosen per row so that the row's
//                        total lies below 2^62): integer addition is associative, so the wave scan is exact, the table is
//                        monotone, two runs are bit-equal, and a block of mass 0 NEVER moves the sum (an fp32 tree scan can, by
//                        an ulp -- and would hand out a block with nothing in it).  Rounded to fp32 once per entry.  (A block
//                        whose mass is below 2^-62 n_blocks times the row's largest is never drawn.)
//   5. ss_draw_kernel    one wave per draw, two uniforms.  thr = fl32(u1 * cum[last]); block = the first g with cum[g] > thr (a
//                        64-way search: three probes at N = 1e6); when rounding leaves none (u1 -> 1), the first g with cum[g] ==
//                        cum[last].  In-block routine: lane l re-scores rows l * R .. l * R + R - 1 of the block (R = SS_G / 64)
//                        with a plain sequential fp32 fma chain over k, w_i = exp(s_i - m) relative to the block's maximum m over
//                        the items that count (history, id 0 and ids >= N weigh 0), taken in 2^-40 fixed point (exact wave scan
//                        again: an item of weight 0 is never the first to exceed anything); item = the first i whose running sum
//                        exceeds floor(u2 * total) (the product in double).  w_i = exp(s_i - lse) of the reference differs from
//                        this by the factor exp(m - lse) common to the block, which the ratio to the block's own total removes.
//                        neg_logp = s_id - lse: the log of the masked, NOT renormalised row, as the reference takes it.
//   6. ss_pos_kernel     pos_logp = s_pos - lse, -inf for the padding id (log(gather(pad(softmax)))) and for ids outside the table.
//
// A row whose every item weighs 0 (cum[last] == 0: all of the catalog in the history, or NaN scores) gets id 0 with log-prob -inf;
// the host-side checks cannot see that without a synchronisation and the entry points never synchronise.
// The uniforms are elements (q * num_neg + j) * 2 + {0, 1} of ONE torch.rand(n_query, num_neg, 2) on the device stream.  The ids
// are NOT those torch.multinomial returns for the same seed; the distribution and the log-probabilities are the same.
#include "rsa_launch.hpp"

#ifndef RSA_SS_G
#define RSA_SS_G 128     // items per block: 64, 128 or 256.  Measured at B = 2048, d = 128, n = 64 (ms, without / with a 100-id
                         // history; tables) at N = 1e6: 64 -> 6.1 / 7.6, 512 MB; 128 -> 6.5 / 9.1, 256 MB; 256 -> 9.5 / 16.8,
                         // 128 MB; at N = 1e7: 64 -> 53 / 54, 128 -> 49 / 52, 256 -> 51 / 58.  A draw and a touched block cost G
                         // rows each, the record and table traffic of the other passes 1 / G: 128 is where the headline
                         // catalog is fastest, at half the memory of 64
#endif

namespace rsa {

typedef float ss_f32x16 __attribute__((ext_vector_type(16)));

constexpr int SS_G = RSA_SS_G;
static_assert(SS_G == 64 || SS_G == 128 || SS_G == 256, "RSA_SS_G: 64, 128 or 256");
constexpr int SS_QB = 128;             // queries per workgroup of the block pass (4 waves x 32)
constexpr int SS_TI = 32;              // items per MFMA tile
constexpr int SS_TPB = SS_G / SS_TI;   // tiles per block
constexpr int SS_R = SS_G / 64;        // rows per lane of the in-block routine
constexpr float SS_FIX_ITEM = 0x1p40f, SS_UNFIX_ITEM = 0x1p-40f;

__device__ __forceinline__ float ss_finish(float dot, int mode, float item_aux, float query_aux, float inv_t) {
  float s = dot;
  if (mode == RSA_SCORE_COS) s = dot * item_aux * query_aux;
  else if (mode == RSA_SCORE_EUC) s = __fmaf_rn(2.f, dot, -item_aux) - query_aux;
  return s * inv_t;
}

__device__ __forceinline__ uint64_t ss_shfl_up(uint64_t v, int off) {
  const uint32_t lo = __shfl_up((uint32_t)v, off, 64), hi = __shfl_up((uint32_t)(v >> 32), off, 64);
  return ((uint64_t)hi << 32) | lo;
}
__device__ __forceinline__ uint64_t ss_shfl(uint64_t v, int src) {
  const uint32_t lo = __shfl((uint32_t)v, src, 64), hi = __shfl((uint32_t)(v >> 32), src, 64);
  return ((uint64_t)hi << 32) | lo;
}
// inclusive sums over the lanes of a wave, exact (integers)
__device__ __forceinline__ uint64_t ss_wave_scan(uint64_t v, int lane) {
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const uint64_t o = ss_shfl_up(v, off);
    if (lane >= off) v += o;
  }
  return v;
}

// ------------------------------------------------------------------ 1. block pass
template <int D, int MODE>
__global__ __launch_bounds__(256) void ss_block_kernel(const float* __restrict__ item_table, int64_t n_items,
                                                       const float* __restrict__ query, int64_t n_query,
                                                       const float* __restrict__ item_aux, const float* __restrict__ query_aux,
                                                       float inv_t, int64_t n_blocks, int64_t blocks_per_split,
                                                       float2* __restrict__ rec) {
  constexpr int KH = D / 2;         // k values per lane half
  constexpr int LD = D + 4;         // padded LDS row stride (floats): conflict-free 16-byte reads
  constexpr int V4 = D / 4;         // float4 per row
  constexpr int LOADS = (SS_TI * V4) / 256;
  static_assert((SS_TI * V4) % 256 == 0, "a tile must split evenly over the workgroup");
  __shared__ __attribute__((aligned(16))) float tile[2][SS_TI * LD];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int j = lane & 31, h = lane >> 5;
  const int64_t q = (int64_t)blockIdx.y * SS_QB + wave * 32 + j;
  const bool qv = q < n_query;

  const int64_t g_begin = (int64_t)blockIdx.x * blocks_per_split;
  int64_t g_end = g_begin + blocks_per_split;
  if (g_end > n_blocks) g_end = n_blocks;
  if (g_begin >= g_end) return;                              // (workgroup-uniform, before any barrier)
  const int64_t i_begin = 1 + g_begin * SS_G;
  int64_t i_end = 1 + g_end * SS_G;
  if (i_end > n_items) i_end = n_items;
  const int n_tiles = (int)((i_end - i_begin + SS_TI - 1) / SS_TI);

  float bq[KH];
  {
    const float4* src = reinterpret_cast<const float4*>(query + (size_t)(qv ? q : 0) * D + h * KH);
#pragma unroll
    for (int c = 0; c < KH / 4; ++c) {
      float4 v = src[c];
      if (!qv) v = make_float4(0.f, 0.f, 0.f, 0.f);
      bq[4 * c + 0] = v.x; bq[4 * c + 1] = v.y; bq[4 * c + 2] = v.z; bq[4 * c + 3] = v.w;
    }
  }
  float q_aux = 0.f;
  if constexpr (MODE != 0) q_aux = query_aux[qv ? q : 0];

  float4 stage[LOADS];
  auto fetch = [&](int t) __attribute__((always_inline)) {   // rows past the range: a valid row is read and zeroed
#pragma unroll
    for (int f = 0; f < LOADS; ++f) {
      const int idx = f * 256 + tid;
      const int row = idx / V4, c4 = idx - row * V4;
      int64_t item = i_begin + (int64_t)t * SS_TI + row;
      const bool ok = item < i_end;
      item = item < n_items ? item : n_items - 1;
      const float4 v = reinterpret_cast<const float4*>(item_table + (size_t)item * D)[c4];
      stage[f] = ok ? v : make_float4(0.f, 0.f, 0.f, 0.f);
    }
  };
  auto commit = [&](int buf) __attribute__((always_inline)) {
#pragma unroll
    for (int f = 0; f < LOADS; ++f) {
      const int idx = f * 256 + tid;
      const int row = idx / V4, c4 = idx - row * V4;
      *reinterpret_cast<float4*>(&tile[buf][row * LD + c4 * 4]) = stage[f];
    }
  };
  auto mfma_tile = [&](int buf) __attribute__((always_inline)) -> ss_f32x16 {
    ss_f32x16 acc = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    const float* arow = &tile[buf][j * LD + h * KH];          // the lane's item row of the tile, its k half
#pragma unroll
    for (int c = 0; c < KH / 4; ++c) {
      const float4 a = *reinterpret_cast<const float4*>(arow + 4 * c);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, bq[4 * c + 0], acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, bq[4 * c + 1], acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, bq[4 * c + 2], acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, bq[4 * c + 3], acc, 0, 0, 0);
    }
    return acc;   // acc[r] = <item (i0 + row(r)), query q>, row(r) = (r & 3) + 8 * (r >> 2) + 4 * h
  };

  float run_m = -INFINITY, run_s = 0.f;
  // the epilogue of tile t: scores, the lane's online (max, sum exp) of the current block, and the block's record at its end
  auto epilogue = [&](const ss_f32x16& acc, int t) __attribute__((always_inline)) {
    const int64_t i0 = i_begin + (int64_t)t * SS_TI;
    const bool partial = i0 + SS_TI > i_end;                  // only the last tile of the catalog
    float v[16];
#pragma unroll
    for (int g4 = 0; g4 < 4; ++g4) {
      float xs[4] = {0.f, 0.f, 0.f, 0.f};
      if constexpr (MODE != 0) {
        // the lane's 16 rows are 4 runs of 4 consecutive items: one aligned 16-byte load each (item_aux carries 64 floats
        // of padding for the rows of the last tile that lie past the table; they are masked below)
        const float4 xa = *reinterpret_cast<const float4*>(item_aux + (i0 - 1 + 8 * g4 + 4 * h));
        xs[0] = xa.x; xs[1] = xa.y; xs[2] = xa.z; xs[3] = xa.w;
      }
#pragma unroll
      for (int r4 = 0; r4 < 4; ++r4) {
        const int r = 4 * g4 + r4;
        float s = ss_finish(acc[r], MODE, xs[r4], q_aux, inv_t);
        if (partial && !(i0 + (r & 3) + 8 * (r >> 2) + 4 * h < i_end)) s = -INFINITY;
        v[r] = s;
      }
    }
    float tmax = fmaxf(fmaxf(v[0], v[1]), v[2]);
#pragma unroll
    for (int r = 3; r < 15; r += 2) tmax = fmaxf(fmaxf(tmax, v[r]), v[r + 1]);
    tmax = fmaxf(tmax, v[15]);
    const float m_new = fmaxf(run_m, tmax);
    const float m_safe = m_new == -INFINITY ? 0.f : m_new;   // nothing seen yet: exp(-inf - 0) = 0 everywhere
    constexpr float LOG2E = 1.4426950408889634f;
    const float c = m_safe * LOG2E;
    float sum = run_s * __builtin_amdgcn_exp2f(__fmaf_rn(run_m, LOG2E, -c));
#pragma unroll
    for (int r = 0; r < 16; ++r) sum += __builtin_amdgcn_exp2f(__fmaf_rn(v[r], LOG2E, -c));
    run_m = m_new;
    run_s = sum;
    if ((t + 1) % SS_TPB == 0 || t == n_tiles - 1) {          // (workgroup-uniform) the block ends with this tile
      // fold the two lane halves' item subsets (lanes j and j + 32 hold the same query)
      const float om = __shfl_xor(run_m, 32, 64), os = __shfl_xor(run_s, 32, 64);
      const float m = fmaxf(run_m, om);
      float s = 0.f;
      if (m > -INFINITY) s = run_s * __expf(run_m - m) + os * __expf(om - m);
      if (h == 0 && qv) rec[(size_t)q * n_blocks + g_begin + t / SS_TPB] = make_float2(m, s);
      run_m = -INFINITY;
      run_s = 0.f;
    }
  };

  // tile t is multiplied out of buffer t & 1 while tile t + 1 travels through registers into the other one; the epilogue of
  // tile t - 1 is independent VALU work the scheduler places under the MFMA chain of tile t
  fetch(0);
  commit(0);
  __syncthreads();
  fetch(1);
  ss_f32x16 acc_prev = mfma_tile(0);
  commit(1);
  __syncthreads();
  for (int t = 1; t < n_tiles; ++t) {
    fetch(t + 1);
    const ss_f32x16 acc = mfma_tile(t & 1);
    epilogue(acc_prev, t - 1);
    commit((t + 1) & 1);
    __syncthreads();
    acc_prev = acc;
  }
  epilogue(acc_prev, n_tiles - 1);
}

// ------------------------------------------------------------------ 2. logsumexp and block masses from the records
__global__ __launch_bounds__(256) void ss_merge_kernel(const float2* __restrict__ rec, int64_t n_query, int64_t n_blocks,
                                                       float* __restrict__ lse, float* __restrict__ mass) {
  const int lane = threadIdx.x & 63;
  const int64_t q = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (q >= n_query) return;
  const float2* row = rec + (size_t)q * n_blocks;
  float m = -INFINITY;
  for (int64_t g = lane; g < n_blocks; g += 64) m = fmaxf(m, row[g].x);
  m = wave_max(m);
  float acc = 0.f;                                            // lane l: blocks l, l + 64, ... in that order, then a fixed butterfly
  for (int64_t g = lane; g < n_blocks; g += 64) {
    const float2 p = row[g];
    if (p.x > -INFINITY) acc += p.y * __expf(p.x - m);
  }
  acc = group_sum<64>(acc);
  const float l = m + logf(acc);
  if (lane == 0) lse[q] = l;
  for (int64_t g = lane; g < n_blocks; g += 64) {
    const float2 p = row[g];
    const float v = p.y * __expf(p.x - l);
    mass[(size_t)q * n_blocks + g] = v > 0.f ? v : 0.f;       // (NaN -> 0)
  }
}

// ------------------------------------------------------------------ the in-block routine
// Lane l of the wave re-scores rows l * SS_R .. of block g for the query row q4 (plain sequential fma chain over k), marks the
// ones that weigh 0 (past the table, in the history), and takes w = exp(s - m) in 2^-40 fixed point against the maximum m of the
// rest.  -> s[r] the scores, w[r] the weights, excl the sum of the weights in front of the lane's first row, total, m.
template <int D>
__device__ __forceinline__ void ss_block_weights(const float* __restrict__ item_table, int64_t n_items, int mode,
                                                 const float* __restrict__ item_aux, float q_aux, float inv_t,
                                                 const float4* __restrict__ q4, const int64_t* __restrict__ hist, int hist_len,
                                                 int64_t g, int lane, float (&s)[SS_R], uint64_t (&w)[SS_R], uint64_t& excl,
                                                 uint64_t& total, float& m) {
  const int64_t first = 1 + g * SS_G;
  bool ok[SS_R];
  float acc[SS_R];
  const float4* rows[SS_R];
  int64_t item[SS_R];
#pragma unroll
  for (int r = 0; r < SS_R; ++r) {
    item[r] = first + lane * SS_R + r;
    ok[r] = item[r] < n_items;
    if (!ok[r]) item[r] = n_items - 1;                        // a valid row is read, its weight is 0
    rows[r] = reinterpret_cast<const float4*>(item_table + (size_t)item[r] * D);
    acc[r] = 0.f;
  }
#pragma unroll 4
  for (int c = 0; c < D / 4; ++c) {
    const float4 qq = q4[c];
#pragma unroll
    for (int r = 0; r < SS_R; ++r) {
      const float4 x = rows[r][c];
      acc[r] = __fmaf_rn(x.w, qq.w, __fmaf_rn(x.z, qq.z, __fmaf_rn(x.y, qq.y, __fmaf_rn(x.x, qq.x, acc[r]))));
    }
  }
#pragma unroll
  for (int r = 0; r < SS_R; ++r) {
    const float ia = mode != RSA_SCORE_IP ? item_aux[item[r] - 1] : 0.f;
    s[r] = ss_finish(acc[r], mode, ia, q_aux, inv_t);
  }
  // the history ids inside this block (0-padded, duplicates allowed): 64 slots per trip, the hits handed round by ballot
  for (int l0 = 0; l0 < hist_len; l0 += 64) {
    const int l = l0 + lane;
    const int64_t off = (l < hist_len ? hist[l] : 0) - first;
    unsigned long long hits = __ballot(off >= 0 && off < SS_G);
    while (hits) {
      const int src = __ffsll((long long)hits) - 1;
      hits &= hits - 1;
      const int o = __shfl((int)off, src, 64);
#pragma unroll
      for (int r = 0; r < SS_R; ++r)
        if (o == lane * SS_R + r) ok[r] = false;
    }
  }
  float mx = -INFINITY;
#pragma unroll
  for (int r = 0; r < SS_R; ++r)
    if (ok[r]) mx = fmaxf(mx, s[r]);
  m = wave_max(mx);
  uint64_t mine = 0;
#pragma unroll
  for (int r = 0; r < SS_R; ++r) {
    const float e = ok[r] ? __expf(s[r] - m) : 0.f;
    w[r] = e > 0.f ? (uint64_t)(e * SS_FIX_ITEM) : 0ull;      // (NaN -> 0)
    mine += w[r];
  }
  const uint64_t incl = ss_wave_scan(mine, lane);
  excl = incl - mine;
  total = ss_shfl(incl, 63);
}

// ------------------------------------------------------------------ 3. blocks the history touches, re-summed without it
template <int D>
__global__ __launch_bounds__(256) void ss_hist_kernel(const float* __restrict__ item_table, int64_t n_items, int mode,
                                                      const float* __restrict__ item_aux, const float* __restrict__ query_aux,
                                                      float inv_t, const float* __restrict__ query, int64_t n_query,
                                                      const int64_t* __restrict__ user_hist, int hist_len, int64_t n_blocks,
                                                      const float* __restrict__ lse, float* __restrict__ mass) {
  const int lane = threadIdx.x & 63;
  const int64_t e = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (e >= n_query * hist_len) return;
  const int64_t q = e / hist_len;
  const int l = (int)(e - q * hist_len);
  const int64_t* hist = user_hist + (size_t)q * hist_len;
  const int64_t id = hist[l];
  if (id < 1 || id >= n_items) return;                        // padding (wave-uniform)
  const int64_t g = (id - 1) / SS_G;
  bool dup = false;                                           // an earlier slot already stands for this block
  for (int l2 = lane; l2 < l; l2 += 64) {
    const int64_t h2 = hist[l2];
    dup |= h2 >= 1 && h2 < n_items && (h2 - 1) / SS_G == g;
  }
  if (__ballot(dup) != 0ull) return;
  float s[SS_R], m;
  uint64_t w[SS_R], excl, total;
  ss_block_weights<D>(item_table, n_items, mode, item_aux, mode != RSA_SCORE_IP ? query_aux[q] : 0.f, inv_t,
                      reinterpret_cast<const float4*>(query + (size_t)q * D), hist, hist_len, g, lane, s, w, excl, total, m);
  if (lane == 0) {
    float v = 0.f;
    if (total != 0ull) v = (float)total * SS_UNFIX_ITEM * __expf(m - lse[q]);
    mass[(size_t)q * n_blocks + g] = v > 0.f ? v : 0.f;
  }
}

// ------------------------------------------------------------------ 4. running sum of the block masses
__global__ __launch_bounds__(256) void ss_scan_kernel(const float* __restrict__ mass, int64_t n_query, int64_t n_blocks,
                                                      float* __restrict__ cum) {
  const int lane = threadIdx.x & 63;
  const int64_t q = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (q >= n_query) return;
  const float* row = mass + (size_t)q * n_blocks;
  float* out = cum + (size_t)q * n_blocks;
  // the fixed point sits 62 bits above the row's total at most: with the largest mass < 2^e and n_blocks <= 2^lb the sum stays
  // below 2^(e + lb), so masses are taken in units of 2^-(62 - e - lb) -- a power of two, the scaling is exact -- whatever the
  // history has left of the row
  float mx = 0.f;
  for (int64_t g = lane; g < n_blocks; g += 64) {
    const float v = row[g];
    if (v > 0.f && v < INFINITY) mx = fmaxf(mx, v);
  }
  mx = wave_max(mx);
  int e = 0;
  frexpf(mx, &e);
  const int sh = 62 - e - (64 - __clzll((long long)n_blocks));
  uint64_t carry = 0;
  for (int64_t g0 = 0; g0 < n_blocks; g0 += 64) {             // (wave-uniform trip count)
    const int64_t g = g0 + lane;
    const float v = g < n_blocks ? row[g] : 0.f;
    const uint64_t x = (v > 0.f && v < INFINITY) ? (uint64_t)ldexpf(v, sh) : 0ull;
    const uint64_t incl = ss_wave_scan(x, lane) + carry;
    if (g < n_blocks) out[g] = ldexpf((float)incl, -sh);
    carry = ss_shfl(incl, 63);
  }
}

// ------------------------------------------------------------------ 5. the draw
// first g in [0, n) with pred(row[g]); the caller knows pred(row[n - 1]) holds and pred is monotone along the row
template <class P>
__device__ __forceinline__ int64_t ss_first(const float* __restrict__ row, int64_t n, int lane, P pred) {
  int64_t lo = 0, len = n;
  while (len > 1) {                                           // (wave-uniform)
    const int64_t step = (len + 63) / 64;
    int64_t idx = lo + (lane + 1) * step - 1;
    if (idx > lo + len - 1) idx = lo + len - 1;
    const unsigned long long hit = __ballot(pred(row[idx]));  // never 0: the last probe is row[lo + len - 1]
    const int f = hit ? __ffsll((long long)hit) - 1 : 63;
    const int64_t nlo = lo + f * step;
    int64_t nend = nlo + step;
    if (nend > lo + len) nend = lo + len;
    len = nend - nlo;
    lo = nlo;
    if (len < 1) len = 1;
  }
  return lo;
}

template <int D, bool FROM_U>
__global__ __launch_bounds__(256) void ss_draw_kernel(const float* __restrict__ item_table, int64_t n_items, int mode,
                                                      const float* __restrict__ item_aux, const float* __restrict__ query_aux,
                                                      float inv_t, const float* __restrict__ query, int64_t n_query, int num_neg,
                                                      const int64_t* __restrict__ user_hist, int hist_len, int64_t n_blocks,
                                                      const float* __restrict__ lse, const float* __restrict__ cum,
                                                      const float* __restrict__ u_in, float* __restrict__ u_out, PhiloxCall pc,
                                                      int64_t* __restrict__ neg_ids, float* __restrict__ neg_logp) {
  const int lane = threadIdx.x & 63;
  const int64_t e = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (e >= n_query * num_neg) return;
  const int64_t q = e / num_neg;
  float u1, u2;
  if constexpr (FROM_U) {
    u1 = u_in[2 * e];
    u2 = u_in[2 * e + 1];
  } else {
    u1 = torch_rand_element(pc, (uint64_t)(2 * e));
    u2 = torch_rand_element(pc, (uint64_t)(2 * e + 1));
    if (u_out != nullptr && lane == 0) {
      u_out[2 * e] = u1;
      u_out[2 * e + 1] = u2;
    }
  }
  const float* crow = cum + (size_t)q * n_blocks;
  const float last = crow[n_blocks - 1];
  int64_t id = 0;
  float lp = -INFINITY;
  if (last > 0.f) {                                           // (wave-uniform) else: every item of the row weighs 0
    const float thr = u1 * last;
    const int64_t g = last > thr ? ss_first(crow, n_blocks, lane, [thr](float c) { return c > thr; })
                                 : ss_first(crow, n_blocks, lane, [last](float c) { return c >= last; });
    float s[SS_R], m;
    uint64_t w[SS_R], excl, total;
    ss_block_weights<D>(item_table, n_items, mode, item_aux, mode != RSA_SCORE_IP ? query_aux[q] : 0.f, inv_t,
                        reinterpret_cast<const float4*>(query + (size_t)q * D),
                        hist_len > 0 ? user_hist + (size_t)q * hist_len : nullptr, hist_len, g, lane, s, w, excl, total, m);
    const uint64_t T = (uint64_t)((double)u2 * (double)total);        // floor; < total because u2 < 1
    int cand = -1;
    float sv = 0.f;
    uint64_t run = excl;
#pragma unroll
    for (int r = 0; r < SS_R; ++r) {
      run += w[r];
      if (cand < 0 && run > T) {
        cand = r;
        sv = s[r];
      }
    }
    const unsigned long long hit = __ballot(cand >= 0);
    if (hit != 0ull) {                                        // (0 only when total == 0: nothing in the block counts)
      const int f = __ffsll((long long)hit) - 1;
      id = 1 + g * SS_G + (int64_t)f * SS_R + __shfl(cand, f, 64);
      lp = __shfl(sv, f, 64) - lse[q];
    }
  }
  if (lane == 0) {
    neg_ids[e] = id;
    neg_logp[e] = lp;
  }
}

// ------------------------------------------------------------------ 6. log-probabilities of given ids
__global__ __launch_bounds__(256) void ss_pos_kernel(const float* __restrict__ item_table, int64_t n_items, int dim, int mode,
                                                     const float* __restrict__ item_aux, const float* __restrict__ query_aux,
                                                     float inv_t, const float* __restrict__ query, int64_t n_query, int n_pos,
                                                     const int64_t* __restrict__ pos_ids, const float* __restrict__ lse,
                                                     float* __restrict__ pos_logp) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n_query * n_pos) return;
  const int64_t q = e / n_pos, id = pos_ids[e];
  float lp = -INFINITY;
  if (id >= 1 && id < n_items) {
    const float4* x = reinterpret_cast<const float4*>(item_table + (size_t)id * dim);
    const float4* qq = reinterpret_cast<const float4*>(query + (size_t)q * dim);
    float acc = 0.f;
    for (int c = 0; c < dim / 4; ++c) {
      const float4 a = x[c], b = qq[c];
      acc = __fmaf_rn(a.w, b.w, __fmaf_rn(a.z, b.z, __fmaf_rn(a.y, b.y, __fmaf_rn(a.x, b.x, acc))));
    }
    const bool aux = mode != RSA_SCORE_IP;
    lp = ss_finish(acc, mode, aux ? item_aux[id - 1] : 0.f, aux ? query_aux[q] : 0.f, inv_t) - lse[q];
  }
  pos_logp[e] = lp;
}

}  // namespace rsa

using namespace rsa;

// Item ranges of the block pass: ~4 workgroups per CU in flight, a multiple of 8 ranges so that all query groups of one range
// land on one XCD and share its L2 (the policy of rsa_fullscore), whole blocks per range.
struct SsPlan {
  int64_t n_blocks, blocks_per_split, splits;
};
static SsPlan ss_plan(int64_t n_query, int64_t n_items) {
  SsPlan p;
  p.n_blocks = (n_items - 1 + SS_G - 1) / SS_G;
  const int64_t groups = (n_query + SS_QB - 1) / SS_QB;
  int64_t splits = (1024 + groups - 1) / groups;
  if (splits >= 8) splits = (splits + 7) / 8 * 8;
  if (splits > p.n_blocks) splits = p.n_blocks;
  if (splits < 1) splits = 1;
  p.blocks_per_split = (p.n_blocks + splits - 1) / splits;
  p.splits = (p.n_blocks + p.blocks_per_split - 1) / p.blocks_per_split;
  return p;
}

struct SsLayout {
  float2* rec;       // [n_query, n_blocks] (max, sum exp) of every block
  float* mass;       // [n_query, n_blocks]
  float* cum;        // [n_query, n_blocks]
};
static SsLayout carve_ss(Carver& ws, int64_t n_query, int64_t n_blocks) {
  SsLayout L;
  L.rec = ws.take<float2>(n_query * n_blocks);
  L.mass = ws.take<float>(n_query * n_blocks);
  L.cum = ws.take<float>(n_query * n_blocks);
  return L;
}

extern "C" int64_t rsa_softmax_sample_workspace_bytes(int64_t n_query, int64_t n_items) {
  if (n_query <= 0 || n_items <= 1) return 0;
  Carver sizing(nullptr);
  carve_ss(sizing, n_query, ss_plan(n_query, n_items).n_blocks);
  return align256(sizing.bytes()) + 256;
}

extern "C" int32_t rsa_softmax_sample_block(void) { return SS_G; }

template <bool U_GIVEN>
static int ss_entry(const rsa_softmax_sample_args* args, rsa_stream_t stream, const char* fn) {
  rsa_softmax_sample_args a;
  if (int rc = load_args(a, args, fn)) return rc;
  RSA_CHECK_ARG(a.n_query >= 0 && a.n_items >= 2 && a.n_items <= (1ll << 36), "%s: need 2 <= n_items <= 2^36", fn);
  RSA_CHECK_ARG(a.num_neg >= 0 && a.n_pos >= 0 && a.hist_len >= 0, "%s: num_neg / n_pos / hist_len must not be negative", fn);
  RSA_CHECK_ARG(a.inv_t > 0.f && a.inv_t < INFINITY, "%s: inv_t = 1 / t must be positive and finite", fn);
  RSA_CHECK_ARG(a.score_mode >= RSA_SCORE_IP && a.score_mode <= RSA_SCORE_EUC, "%s: unknown score_mode %d", fn, a.score_mode);
  if (a.n_query == 0) return RSA_OK;
  RSA_CHECK_ARG(a.item_table && a.query, "%s: item_table/query is null", fn);
  RSA_CHECK_ARG(a.lse != nullptr, "%s: lse is null", fn);
  RSA_CHECK_ARG(a.num_neg == 0 || (a.neg_ids && a.neg_logp), "%s: neg_ids/neg_logp is null", fn);
  RSA_CHECK_ARG(a.n_pos == 0 || (a.pos_ids && a.pos_logp), "%s: pos_ids/pos_logp is null", fn);
  RSA_CHECK_ARG(a.hist_len == 0 || a.user_hist, "%s: user_hist is null", fn);
  RSA_CHECK_ARG(a.score_mode == RSA_SCORE_IP || (a.item_aux && a.query_aux && ((uintptr_t)a.item_aux & 15) == 0),
                "%s: cosine / Euclidean scores need item_aux (16-byte aligned) and query_aux", fn);
  RSA_CHECK_ARG(a.n_query * (int64_t)a.num_neg <= (1ll << 32) && a.n_query * (int64_t)a.hist_len <= (1ll << 32) &&
                    a.n_query * (int64_t)a.n_pos <= (1ll << 32), "%s: more than 2^32 draws / history slots / positives", fn);
  if (a.num_neg > 0) {
    if (U_GIVEN) RSA_CHECK_ARG(a.u_in != nullptr, "%s: u_in is null", fn);
    else RSA_CHECK_ARG(a.grid_threads > 0 && (a.offset & 3) == 0, "%s: bad philox state", fn);
  }
  if (a.dim != 32 && a.dim != 64 && a.dim != 128) {
    rsa::set_error("%s: dim=%d: the MFMA block pass is built for dim in {32, 64, 128}", fn, a.dim);
    return RSA_ERR_UNSUPPORTED;
  }
  const int64_t need = rsa_softmax_sample_workspace_bytes(a.n_query, a.n_items);
  RSA_CHECK_ARG(a.workspace != nullptr && a.workspace_bytes >= need, "%s: workspace too small (%lld < %lld)", fn,
                (long long)a.workspace_bytes, (long long)need);
  hipStream_t s = (hipStream_t)stream;
  const SsPlan pl = ss_plan(a.n_query, a.n_items);
  Carver ws(a.workspace);
  const SsLayout W = carve_ss(ws, a.n_query, pl.n_blocks);
  float* mass = a.mass ? a.mass : W.mass;
  float* cum = a.cum ? a.cum : W.cum;
  const int64_t nq = a.n_query, nb = pl.n_blocks;
  const unsigned groups = (unsigned)((nq + SS_QB - 1) / SS_QB), per_wave = (unsigned)((nq + 3) / 4);

  dispatch_dim<32, 64, 128>(a.dim, [&](auto D) {
    dispatch_int<RSA_SCORE_IP, RSA_SCORE_COS, RSA_SCORE_EUC>(a.score_mode, [&](auto MODE) {
      hipLaunchKernelGGL((ss_block_kernel<D(), MODE()>), dim3((unsigned)pl.splits, groups), dim3(256), 0, s, a.item_table, a.n_items,
                         a.query, nq, a.item_aux, a.query_aux, a.inv_t, nb, pl.blocks_per_split, W.rec);
    });
  });
  RSA_CHECK_LAUNCH("rsa_softmax_sample(block pass)");
  hipLaunchKernelGGL(ss_merge_kernel, dim3(per_wave), dim3(256), 0, s, W.rec, nq, nb, a.lse, mass);
  RSA_CHECK_LAUNCH("rsa_softmax_sample(merge)");
  if (a.n_pos > 0) {
    const int64_t total = nq * a.n_pos;
    hipLaunchKernelGGL(ss_pos_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, a.item_table, a.n_items, (int)a.dim,
                       (int)a.score_mode, a.item_aux, a.query_aux, a.inv_t, a.query, nq, (int)a.n_pos, a.pos_ids, a.lse, a.pos_logp);
    RSA_CHECK_LAUNCH("rsa_softmax_sample(positives)");
  }
  if (a.num_neg == 0 && !a.mass && !a.cum) return RSA_OK;
  if (a.hist_len > 0) {
    const int64_t total = nq * a.hist_len;
    dispatch_dim<32, 64, 128>(a.dim, [&](auto D) {
      hipLaunchKernelGGL((ss_hist_kernel<D()>), dim3((unsigned)((total + 3) / 4)), dim3(256), 0, s, a.item_table, a.n_items,
                         (int)a.score_mode, a.item_aux, a.query_aux, a.inv_t, a.query, nq, a.user_hist, (int)a.hist_len, nb, a.lse, mass);
    });
    RSA_CHECK_LAUNCH("rsa_softmax_sample(history)");
  }
  hipLaunchKernelGGL(ss_scan_kernel, dim3(per_wave), dim3(256), 0, s, mass, nq, nb, cum);
  RSA_CHECK_LAUNCH("rsa_softmax_sample(scan)");
  if (a.num_neg > 0) {
    const int64_t total = nq * a.num_neg;
    const PhiloxCall pc{a.seed, a.offset >> 2, a.grid_threads ? a.grid_threads : 1, a.elem_base};
    dispatch_dim<32, 64, 128>(a.dim, [&](auto D) {
      hipLaunchKernelGGL((ss_draw_kernel<D(), U_GIVEN>), dim3((unsigned)((total + 3) / 4)), dim3(256), 0, s, a.item_table, a.n_items,
                         (int)a.score_mode, a.item_aux, a.query_aux, a.inv_t, a.query, nq, (int)a.num_neg, a.user_hist, (int)a.hist_len,
                         nb, a.lse, cum, a.u_in, U_GIVEN ? nullptr : a.u_out, pc, a.neg_ids, a.neg_logp);
    });
    RSA_CHECK_LAUNCH("rsa_softmax_sample(draw)");
  }
  return RSA_OK;
}

extern "C" int rsa_softmax_sample(const rsa_softmax_sample_args* args, rsa_stream_t stream) {
  return ss_entry<false>(args, stream, "rsa_softmax_sample");
}

extern "C" int rsa_softmax_lookup(const rsa_softmax_sample_args* args, rsa_stream_t stream) {
  return ss_entry<true>(args, stream, "rsa_softmax_lookup");
}
