// Adaptive (model-based) negative samplers on a k-means codebook (gfx950).
//
// rsa_midx_sample / rsa_midx_lookup : MIDXSamplerUniform / ClusterSamplerUniform .forward + .compute_item_p
//                                     recstudio/ann/sampler.py:308-388, :460-510
// rsa_kmeans_step                   : one assignment pass of kmeans()      recstudio/ann/sampler.py:19-31
//
// DRAW.  One wave64 per query, one lane per cluster (K <= 64), the codebooks and wkk in LDS.
//   r_p[k]  = <q_p, c_p[k]>                      four interleaved FMA chains (elements i % 4), summed (x + y) + (z + w)
//   e_p[k]  = expf(r_p[k] - max_k r_p[k])
//   MIDX:    w0[k0] = e_0[k0] * t[k0],  t[k0] = sum_k1 wkk[k0][k1] * e_1[k1]   (ascending k1, product rounded, then added)
//            w1[k1 | k0] = wkk[k0][k1] * e_1[k1]
//   Cluster: w0[k] = wkk[k] * e_0[k]
//   A draw with uniform u over weights w[0..K): S = w[0] + w[1] + ... (ascending, fp32), target = fl(u * S), the answer is the
//   FIRST k with w[k] > 0 whose running sum (the same additions) exceeds the target.
// TIE RULE.  A bucket of weight 0 adds nothing to the running sum, so it is never the first to exceed anything; the test
// `w[k] > 0` makes that explicit.  When no running sum exceeds the target (u * S rounded up to S: u = 1 - 2^-24), the answer is the
// LAST k with w[k] > 0.  When every weight underflowed to 0 the answer is the first k whose bucket (MIDX, first stage: whose
// row of wkk) holds an item.  An empty bucket (wkk == 0) is therefore never returned, whatever u is.
// The item: idx = min(floor(float(cnt) * u2), cnt - 1) inside bucket k0 * K + k1, id = indices[indptr[b] + idx] + 1.
// Uniforms: element ((q * n + j) * 3 + t) of ONE torch.rand(M, n, 3) on the device stream (Cluster: (M, n, 2)).
// WEIGHTED ITEM (MIDXSamplerPop / ClusterSamplerPop; cp and item_logp given).  Inside bucket [start, end) the item sits at the FIRST
// position with cp[pos] > u2: an upper-bound binary search over the bucket's slice of cp.  cp is non-decreasing and stays where it
// is across an item of weight 0 (rsa_midx_weights), so such an item is never the first to exceed anything.  When no position
// exceeds u2 (a bucket of weight 0 chosen because every weight is 0) the answer is the last position whose cp exceeds its
// predecessor's, the first position when there is none.  id = indices[pos] + 1, log-prob = fl(fl(r0 + r1) + item_logp[id]);
// compute_item_p adds item_logp[pos_id] the same way (0 for the padding id).
// With a CosineScorer the query is divided by max(||q||, 1e-12) first (the sum of squares in double, one rounding per element).
//
// LLOYD STEP.  One pass over the rows for 1 or 2 parts (column halves): tiles of 16 rows are staged in LDS, a wave scores 4 rows
// against the K centres (lane = centre, argmin of ||c||^2 - 2 <x, c>, the lowest k on a tie), and per-cluster sums are then
// accumulated by one thread per COLUMN walking the tile's rows in order -- no float atomics, no [N, K] matrix.  Every workgroup
// leaves its partial sums / counts / loss in the workspace; a second launch adds the partials in workgroup order (in double).
// The grid is a function of the row count alone, so two runs over the same input are bit-equal.
#include "rsa_internal.hpp"
#include "rsa_lds.hpp"

namespace rsa {

constexpr int MIDX_MAX_K = 64, MIDX_MAX_DIM = 256;
constexpr int KM_TILE = 16;             // rows per tile of the Lloyd step (4 per wave)
constexpr int KM_MAX_GRID = 512;

extern __shared__ __attribute__((aligned(16))) float midx_smem[];

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}

__device__ __forceinline__ void stage_centres(float* cs, const float* __restrict__ centres, int rows, int dsub) {
  const int q4 = dsub >> 2, stride = dsub + CPAD;
  for (int i = threadIdx.x; i < rows * q4; i += blockDim.x) {
    const int r = i / q4, c = i - r * q4;
    *reinterpret_cast<float4*>(cs + r * stride + c * 4) = reinterpret_cast<const float4*>(centres)[i];
  }
}

// x / max(||x||, 1e-12) for a row held one float4 per lane (lanes past the row hold zeros)
__device__ __forceinline__ float4 normalize_row(float4 v) {
  const double ss = wave_sum_f64((double)v.x * v.x + (double)v.y * v.y + (double)v.z * v.z + (double)v.w * v.w);
  const double nrm = fmax(sqrt(ss), 1e-12);
  return make_float4((float)((double)v.x / nrm), (float)((double)v.y / nrm), (float)((double)v.z / nrm), (float)((double)v.w / nrm));
}

// ---------------------------------------------------------------- draw
struct MidxParams {
  const float* query;
  int64_t n_queries;
  int dim, parts, K, cosine;
  const float* centres;
  const float* wkk;
  const int32_t* indptr;
  const int32_t* indices;
  int64_t n_items;
  const int32_t* cd0;
  const int32_t* cd1;
  int num_neg, n_pos;
  const int64_t* pos_ids;
  const float* u_in;
  int64_t* neg_ids;
  float* neg_logp;
  float* pos_logp;
  float* u_out;
  PhiloxCall pc;
  const float* cp;
  const float* item_logp;
};

// first k with w(k) > 0 whose running sum exceeds `target` (see TIE RULE above); w(k) / has(k): weight / "holds an item"
template <class W, class H>
__device__ __forceinline__ int pick_cluster(int K, float target, W&& w, H&& has) {
  int sel = -1, last = -1, first_has = -1;
  float run = 0.f;
  for (int k = 0; k < K; ++k) {
    const float wk = w(k);
    run = run + wk;
    if (first_has < 0 && has(k)) first_has = k;
    if (wk > 0.f) {
      last = k;
      if (sel < 0 && run > target) sel = k;
    }
  }
  return sel >= 0 ? sel : (last >= 0 ? last : (first_has >= 0 ? first_has : 0));
}

// first position of [start, end) with cp[pos] > u (see WEIGHTED ITEM above)
__device__ __forceinline__ int32_t pick_weighted(const float* __restrict__ cp, int32_t start, int32_t end, float u) {
  int32_t lo = start, hi = end;
  while (lo < hi) {
    const int32_t mid = lo + ((hi - lo) >> 1);
    if (cp[mid] > u) hi = mid;
    else lo = mid + 1;
  }
  if (lo < end) return lo;
  const float top = cp[end - 1];                           // nothing exceeds u: the first position that reaches the last value
  if (!(top > 0.f)) return start;
  lo = start, hi = end - 1;
  while (lo < hi) {
    const int32_t mid = lo + ((hi - lo) >> 1);
    if (cp[mid] >= top) hi = mid;
    else lo = mid + 1;
  }
  return lo;
}

template <bool FROM_U, bool WEIGHTED>
__global__ __launch_bounds__(256) void midx_draw_kernel(const MidxParams p) {
  const int K = p.K, d = p.dim, parts = p.parts, dsub = d / parts, stride = dsub + CPAD;
  const int wrow = parts == 2 ? K + 1 : 1;                 // MIDX: row k0 of wkk, then the row's sum
  float* cs = midx_smem;                                   // [parts * K][dsub + CPAD]
  float* wk = cs + parts * K * stride;                     // MIDX [K][K + 1], Cluster [K]
  float* qb = wk + ((K * wrow + 3) & ~3);                  // [4][d]
  float* rr = qb + 4 * d;                                  // [4][2][64]  logits
  float* ee = rr + 4 * 2 * 64;                             // [4][2][64]  exponentials
  float* ww = ee + 4 * 2 * 64;                             // [4][64]     first-stage weights
  const int lane = lane_id(), wave = threadIdx.x >> 6;
  stage_centres(cs, p.centres, parts * K, dsub);
  if (p.wkk != nullptr) {
    if (parts == 2) {
      for (int i = threadIdx.x; i < K * K; i += blockDim.x) wk[(i / K) * wrow + (i % K)] = p.wkk[i];
    } else {
      for (int i = threadIdx.x; i < K; i += blockDim.x) wk[i] = p.wkk[i];
    }
  } else {
    for (int i = threadIdx.x; i < K * wrow; i += blockDim.x) wk[i] = 0.f;
  }
  __syncthreads();
  if (parts == 2 && (int)threadIdx.x < K) {                // "row k0 holds an item"
    float s = 0.f;
    for (int k1 = 0; k1 < K; ++k1) s += wk[threadIdx.x * wrow + k1];
    wk[threadIdx.x * wrow + K] = s;
  }
  float* q_w = qb + wave * d;
  float *r0 = rr + wave * 128, *r1 = r0 + 64, *e0 = ee + wave * 128, *e1 = e0 + 64, *w0 = ww + wave * 64;
  const int n = p.num_neg, T = p.n_pos, nu = parts + 1;
  const int64_t per_pass = (int64_t)gridDim.x * 4;
  for (int64_t q0 = (int64_t)blockIdx.x * 4; q0 < p.n_queries; q0 += per_pass) {     // block-uniform trip count
    const int64_t q = q0 + wave;
    const bool act = q < p.n_queries;
    __syncthreads();                                       // the previous query's LDS slots are free (and wk is complete)
    if (act) {
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (lane < (d >> 2)) v = reinterpret_cast<const float4*>(p.query + q * d)[lane];
      if (p.cosine) v = normalize_row(v);
      if (lane < (d >> 2)) reinterpret_cast<float4*>(q_w)[lane] = v;
    }
    __syncthreads();
    if (act) {
      const int kc = lane < K ? lane : K - 1;
      for (int part = 0; part < parts; ++part) {
        const float* c = cs + (part * K + kc) * stride;
        const float* x = q_w + part * dsub;
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int i = 0; i < dsub; i += 4)
          fma4(acc, *reinterpret_cast<const float4*>(x + i), *reinterpret_cast<const float4*>(c + i));
        const float r = sum4(acc);
        const float m = wave_max(lane < K ? r : -INFINITY);
        (part ? r1 : r0)[lane] = r;
        (part ? e1 : e0)[lane] = lane < K ? expf(r - m) : 0.f;
      }
    }
    __syncthreads();
    if (act) {
      float w = 0.f;
      if (lane < K) {
        if (parts == 2) {
          float t = 0.f;
          for (int k1 = 0; k1 < K; ++k1) t = t + wk[lane * wrow + k1] * e1[k1];
          w = e0[lane] * t;
        } else {
          w = wk[lane] * e0[lane];
        }
      }
      w0[lane] = w;
    }
    __syncthreads();
    if (act) {
      float S0 = 0.f;
      for (int k = 0; k < K; ++k) S0 = S0 + w0[k];
      for (int j = lane; j < n; j += 64) {
        const int64_t e = (q * n + j) * nu;
        float u[3];
        for (int t = 0; t < nu; ++t) u[t] = FROM_U ? p.u_in[e + t] : torch_rand_element(p.pc, (uint64_t)(e + t));
        int k0, bucket;
        float logp;
        if (parts == 2) {
          k0 = pick_cluster(K, u[0] * S0, [&](int k) { return w0[k]; }, [&](int k) { return wk[k * wrow + K] > 0.f; });
          const float* row = wk + k0 * wrow;
          float S1 = 0.f;
          for (int k1 = 0; k1 < K; ++k1) S1 = S1 + row[k1] * e1[k1];
          const int k1 = pick_cluster(K, u[1] * S1, [&](int k) { return row[k] * e1[k]; }, [&](int k) { return row[k] > 0.f; });
          bucket = k0 * K + k1;
          logp = r0[k0] + r1[k1];
        } else {
          k0 = pick_cluster(K, u[0] * S0, [&](int k) { return w0[k]; }, [&](int k) { return wk[k] > 0.f; });
          bucket = k0;
          logp = r0[k0];
        }
        const int32_t start = p.indptr[bucket], cnt = p.indptr[bucket + 1] - start;
        int64_t id = 0;                                    // (an index without items: the padding id, nothing is read)
        if (WEIGHTED) {
          const int32_t lim = (int32_t)p.n_items;          // (a bucket is a range of positions: never read past the tables)
          const int32_t s0 = start < 0 ? 0 : (start > lim ? lim : start);
          const int32_t e0 = start + cnt > lim ? lim : start + cnt;
          if (e0 > s0) {
            id = (int64_t)p.indices[pick_weighted(p.cp, s0, e0, u[nu - 1])] + 1;
            id = id < 1 ? 1 : (id > p.n_items ? p.n_items : id);
            logp = logp + p.item_logp[id];
          }
        } else if (cnt > 0) {
          int32_t idx = (int32_t)floorf((float)cnt * u[nu - 1]);
          idx = idx < 0 ? 0 : (idx > cnt - 1 ? cnt - 1 : idx);
          const int64_t at = (int64_t)start + idx;
          id = (int64_t)p.indices[at < p.n_items ? at : p.n_items - 1] + 1;
        }
        p.neg_ids[q * n + j] = id;
        if (p.neg_logp) p.neg_logp[q * n + j] = logp;
        if (!FROM_U && p.u_out)
          for (int t = 0; t < nu; ++t) p.u_out[e + t] = u[t];
      }
      for (int t = lane; t < T; t += 64) {                 // compute_item_p: the padding id reads the zero row
        int64_t id = p.pos_ids[q * T + t];
        id = id < 0 ? 0 : (id > p.n_items ? p.n_items : id);
        int32_t a = p.cd0[id];
        a = a < 0 ? 0 : (a > K ? K : a);
        float v = a > 0 ? r0[a - 1] : 0.f;
        if (parts == 2) {
          int32_t b = p.cd1[id];
          b = b < 0 ? 0 : (b > K ? K : b);
          v = v + (b > 0 ? r1[b - 1] : 0.f);
        }
        if (WEIGHTED) v = v + p.item_logp[id];
        p.pos_logp[q * T + t] = v;
      }
    }
  }
}

static int64_t draw_lds_bytes(int dim, int parts, int K) {
  const int dsub = dim / parts, wrow = parts == 2 ? K + 1 : 1;
  return 4ll * (parts * K * (dsub + CPAD) + ((K * wrow + 3) & ~3) + 4 * dim + 2 * 4 * 2 * 64 + 4 * 64);
}

// ---------------------------------------------------------------- Lloyd step
struct KmeansParams {
  const float* x;            // first row
  int64_t n_rows, row_stride;
  int dim, parts, K, normalize;
  const float* centres;
  int32_t* assign;           // [parts][n_rows]
  float* part_sums;          // [grid][K * dim]
  int32_t* part_counts;      // [grid][parts * 64]
  double* part_loss;         // [grid][parts]
};

__global__ __launch_bounds__(256) void kmeans_step_kernel(const KmeansParams p) {
  const int K = p.K, d = p.dim, parts = p.parts, dsub = d / parts, stride = dsub + CPAD, q4 = d >> 2;
  float* cs = midx_smem;                                   // [parts * K][dsub + CPAD]
  float* cn = cs + parts * K * stride;                     // [parts][64]  ||c||^2
  float* sums = cn + 128;                                  // [parts][K][dsub]
  float* xt = sums + K * d;                                // [KM_TILE][d]
  int32_t* cnt = reinterpret_cast<int32_t*>(xt + KM_TILE * d);   // [parts][64]
  int32_t* ta = cnt + 128;                                 // [parts][KM_TILE]
  double* wl = reinterpret_cast<double*>(ta + 2 * KM_TILE);      // [4][2]
  const int lane = lane_id(), wave = threadIdx.x >> 6;
  stage_centres(cs, p.centres, parts * K, dsub);
  for (int i = threadIdx.x; i < K * d; i += blockDim.x) sums[i] = 0.f;
  if (threadIdx.x < 128) cnt[threadIdx.x] = 0;
  __syncthreads();
  if ((int)threadIdx.x < parts * 64) {
    const int part = threadIdx.x >> 6, k = threadIdx.x & 63;
    double s = 0.0;
    if (k < K)
      for (int i = 0; i < dsub; ++i) s += (double)cs[(part * K + k) * stride + i] * cs[(part * K + k) * stride + i];
    cn[threadIdx.x] = (float)s;
  }
  double wloss[2] = {0.0, 0.0};
  const int64_t n_tiles = (p.n_rows + KM_TILE - 1) / KM_TILE;
  for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const int64_t row0 = tile * KM_TILE;
    const int rows = (int)(p.n_rows - row0 < KM_TILE ? p.n_rows - row0 : KM_TILE);
    __syncthreads();                                       // the previous tile has been consumed (and cn is complete)
    for (int i = threadIdx.x; i < KM_TILE * q4; i += blockDim.x) {
      const int r = i / q4, c = i - r * q4;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (r < rows) v = *reinterpret_cast<const float4*>(p.x + (row0 + r) * p.row_stride + c * 4);
      reinterpret_cast<float4*>(xt)[i] = v;
    }
    __syncthreads();
    if (p.normalize) {                                     // block-uniform
      for (int r = wave * 4; r < wave * 4 + 4; ++r) {
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (lane < q4) v = reinterpret_cast<const float4*>(xt + r * d)[lane];
        v = normalize_row(v);
        if (lane < q4) reinterpret_cast<float4*>(xt + r * d)[lane] = v;
      }
      __syncthreads();
    }
    const int kc = lane < K ? lane : K - 1;
    for (int part = 0; part < parts; ++part) {
      const float* c = cs + (part * K + kc) * stride;
      const float* x = xt + (wave * 4) * d + part * dsub;
      float4 acc[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[r] = make_float4(0.f, 0.f, 0.f, 0.f);
      for (int i = 0; i < dsub; i += 4) {
        const float4 cv = *reinterpret_cast<const float4*>(c + i);
#pragma unroll
        for (int r = 0; r < 4; ++r) fma4(acc[r], *reinterpret_cast<const float4*>(x + r * d + i), cv);
      }
      const float cnk = cn[part * 64 + kc];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = wave * 4 + r;
        if (row >= rows) continue;                         // wave-uniform
        float s = lane < K ? __fmaf_rn(-2.f, sum4(acc[r]), cnk) : INFINITY;
        int k = lane;
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
          const float os = __shfl_xor(s, m, 64);
          const int ok = __shfl_xor(k, m, 64);
          if (os < s || (os == s && ok < k)) {
            s = os;
            k = ok;
          }
        }
        k = k < K ? k : 0;                                 // (all-NaN scores)
        double dd = 0.0;
        if (lane < (dsub >> 2)) {
          const float4 xv = *reinterpret_cast<const float4*>(xt + row * d + part * dsub + lane * 4);
          const float4 cv = *reinterpret_cast<const float4*>(cs + (part * K + k) * stride + lane * 4);
          const double a = (double)xv.x - cv.x, b = (double)xv.y - cv.y, e = (double)xv.z - cv.z, f = (double)xv.w - cv.w;
          dd = a * a + b * b + e * e + f * f;
        }
        wloss[part] += wave_sum_f64(dd);
        if (lane == 0) {
          p.assign[(int64_t)part * p.n_rows + row0 + row] = k;
          ta[part * KM_TILE + row] = k;
          atomicAdd(&cnt[part * 64 + k], 1);
        }
      }
    }
    __syncthreads();
    if ((int)threadIdx.x < d) {                            // one thread per column, the tile's rows in order
      const int part = threadIdx.x / dsub, col = threadIdx.x - part * dsub;
      for (int r = 0; r < rows; ++r) {
        const int a = ta[part * KM_TILE + r];
        float* s = sums + (part * K + a) * dsub + col;
        *s = *s + xt[r * d + threadIdx.x];
      }
    }
  }
  __syncthreads();
  if (lane == 0) {
    wl[wave * 2] = wloss[0];
    wl[wave * 2 + 1] = wloss[1];
  }
  for (int i = threadIdx.x; i < K * d; i += blockDim.x) p.part_sums[(int64_t)blockIdx.x * K * d + i] = sums[i];
  if (threadIdx.x < 128) p.part_counts[(int64_t)blockIdx.x * 128 + threadIdx.x] = cnt[threadIdx.x];
  __syncthreads();
  if ((int)threadIdx.x < parts)
    p.part_loss[(int64_t)blockIdx.x * 2 + threadIdx.x] =
        ((wl[threadIdx.x] + wl[2 + threadIdx.x]) + wl[4 + threadIdx.x]) + wl[6 + threadIdx.x];
}

// the workgroups' partials added in workgroup order
__global__ __launch_bounds__(256) void kmeans_reduce_kernel(const KmeansParams p, int grid, float* __restrict__ sums,
                                                            int32_t* __restrict__ counts, double* __restrict__ loss) {
  const int kd = p.K * p.dim;
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e < kd) {
    double s = 0.0;
    for (int b = 0; b < grid; ++b) s += (double)p.part_sums[(int64_t)b * kd + e];
    sums[e] = (float)s;
  } else if (e < kd + p.parts * p.K) {
    const int i = e - kd, part = i / p.K, k = i - part * p.K;
    int32_t c = 0;
    for (int b = 0; b < grid; ++b) c += p.part_counts[(int64_t)b * 128 + part * 64 + k];
    counts[i] = c;
  } else if (e < kd + p.parts * p.K + p.parts) {
    const int part = e - kd - p.parts * p.K;
    double s = 0.0;
    for (int b = 0; b < grid; ++b) s += p.part_loss[(int64_t)b * 2 + part];
    loss[part] = s;
  }
}

static int64_t kmeans_lds_bytes(int dim, int parts, int K) {
  const int dsub = dim / parts;
  return 4ll * (parts * K * (dsub + CPAD) + 128 + K * dim + KM_TILE * dim + 128 + 2 * KM_TILE) + 8 * 8;
}

static unsigned kmeans_grid(int64_t n_rows) { return grid_1d(n_rows, KM_TILE, KM_MAX_GRID); }

struct KmeansLayout {
  float* sums;
  int32_t* counts;
  double* loss;
  int64_t bytes;
};
static KmeansLayout kmeans_layout(void* base, int64_t n_rows, int dim, int K) {
  Carver c(base);
  const int64_t g = kmeans_grid(n_rows > 0 ? n_rows : 1);
  KmeansLayout L;
  L.sums = c.take<float>(g * K * dim);
  L.counts = c.take<int32_t>(g * 128);
  L.loss = c.take<double>(g * 2);
  L.bytes = c.bytes();
  return L;
}

// ---------------------------------------------------------------- per-epoch tables of the popularity-in-bucket form
struct WeightParams {
  const float* pop;
  const float* x;            // first row, or null
  int64_t n_items, row_stride;
  int dim;
  const int32_t* indptr;
  const int32_t* indices;
  float* p;
  float* item_logp;
  float* wkk;
  float* cp;
};

// ROW PASS.  One wave per item (a lane per float4 of its row): w = pop, times exp(-||x||^2 / 2) in double; p and log p.
__global__ __launch_bounds__(256) void midx_weight_rows_kernel(const WeightParams p) {
  const int lane = lane_id(), q4 = p.dim >> 2;
  const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6), n_waves = (int64_t)gridDim.x * 4;
  if (wave == 0 && lane == 0) {
    p.p[0] = 1.f;
    p.item_logp[0] = 0.f;
  }
  if (p.x == nullptr) {                                    // no rows to read: a lane per item
    for (int64_t i = wave * 64 + lane; i < p.n_items; i += n_waves * 64) {
      const float w = p.pop[i];
      p.p[i + 1] = w;
      p.item_logp[i + 1] = (float)log((double)w);
    }
    return;
  }
  for (int64_t i = wave; i < p.n_items; i += n_waves) {
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (lane < q4) v = reinterpret_cast<const float4*>(p.x + i * p.row_stride)[lane];
    const double ss = wave_sum_f64((double)v.x * v.x + (double)v.y * v.y + (double)v.z * v.z + (double)v.w * v.w);
    if (lane == 0) {
      const float w = (float)((double)p.pop[i] * exp(-0.5 * ss));
      p.p[i + 1] = w;
      p.item_logp[i + 1] = (float)log((double)w);
    }
  }
}

// BUCKET PASS.  One workgroup of 1024 threads per bucket walks its positions in chunks of 8192, a thread 8 consecutive ones.  The
// running sum of position (chunk, wave, lane, j) is  B[wave] + (E[lane] + L[j])  in double, with
//   L[j]   the thread's own weights added one by one,
//   E[l+1] = E[l] + L[7] of lane l      (sequential over the wave's lanes, E[0] = 0),
//   B[w+1] = B[w] + E[64] of wave w     (sequential over the waves, B[0] = the previous chunk's B[16]).
// Every level only ever adds, so the sums never decrease, and an item of weight 0 gets EXACTLY its predecessor's sum also across
// a thread, wave or chunk boundary (the last sum of a thread is by construction the E of the next one, and so on up).  The first
// walk leaves the bucket's total T (the sum at its last position), the second writes cp = fl32(sum / T), which ends at 1.  The
// order of the additions is a function of the bucket's start and length alone.
constexpr int WB_THREADS = 1024, WB_ITEMS = 8;

template <bool WRITE>
__device__ __forceinline__ double bucket_walk(const WeightParams& p, int32_t start, int32_t end, double total, double* tot,
                                              double* wbase) {
  const int lane = lane_id(), wave = threadIdx.x >> 6;
  double carry = 0.0;
  for (int64_t c0 = start; c0 < end; c0 += WB_THREADS * WB_ITEMS) {
    const int64_t at = (int64_t)c0 + (int64_t)threadIdx.x * WB_ITEMS;
    double L[WB_ITEMS];
#pragma unroll
    for (int j = 0; j < WB_ITEMS; ++j) {
      double w = 0.0;
      if (at + j < end) {
        int32_t it = p.indices[at + j];
        it = it < 0 ? 0 : (it >= p.n_items ? (int32_t)p.n_items - 1 : it);
        w = (double)p.p[it + 1];
      }
      L[j] = w;
    }
#pragma unroll
    for (int j = 1; j < WB_ITEMS; ++j) L[j] = L[j - 1] + L[j];
    __syncthreads();                                       // the previous chunk's tot / wbase have been read
    tot[threadIdx.x] = L[WB_ITEMS - 1];
    __syncthreads();
    if (lane == 0) {                                       // E of this wave's lanes, in place
      double e = 0.0;
      for (int l = 0; l < 64; ++l) {
        const double t = tot[wave * 64 + l];
        tot[wave * 64 + l] = e;
        e = e + t;
      }
      wbase[wave] = e;
    }
    __syncthreads();
    if (threadIdx.x == 0) {                                // B of the waves, in place
      double b = carry;
      for (int w = 0; w < WB_THREADS / 64; ++w) {
        const double t = wbase[w];
        wbase[w] = b;
        b = b + t;
      }
      wbase[WB_THREADS / 64] = b;
    }
    __syncthreads();
    carry = wbase[WB_THREADS / 64];
    if (WRITE) {
      const double B = wbase[wave], E = tot[threadIdx.x];
#pragma unroll
      for (int j = 0; j < WB_ITEMS; ++j)
        if (at + j < end) p.cp[at + j] = total > 0.0 ? (float)((B + (E + L[j])) / total) : 0.f;
    }
  }
  return carry;
}

__global__ __launch_bounds__(WB_THREADS) void midx_weight_buckets_kernel(const WeightParams p) {
  __shared__ double tot[WB_THREADS];
  __shared__ double wbase[WB_THREADS / 64 + 1];
  const int b = blockIdx.x;
  const int32_t lim = (int32_t)p.n_items;
  int32_t start = p.indptr[b], end = p.indptr[b + 1];
  start = start < 0 ? 0 : (start > lim ? lim : start);
  end = end > lim ? lim : end;
  const double total = end > start ? bucket_walk<false>(p, start, end, 0.0, tot, wbase) : 0.0;
  if (threadIdx.x == 0) p.wkk[b] = (float)total;
  if (end > start) bucket_walk<true>(p, start, end, total, tot, wbase);
}

static int check_codebook(const char* fn, int dim, int parts, int K) {
  RSA_CHECK_ARG(parts == 1 || parts == 2, "%s: n_parts must be 1 (Cluster) or 2 (MIDX), got %d", fn, parts);
  RSA_CHECK_ARG(K >= 2 && K <= MIDX_MAX_K, "%s: n_clusters must be in [2, %d], got %d", fn, MIDX_MAX_K, K);
  RSA_CHECK_ARG(dim >= 8 && dim <= MIDX_MAX_DIM && dim % 8 == 0, "%s: dim must be a multiple of 8 in [8, %d], got %d", fn,
                MIDX_MAX_DIM, dim);
  return RSA_OK;
}

template <bool U_GIVEN>
static int midx_entry(const rsa_midx_args* args, rsa_stream_t stream, const char* fn) {
  rsa_midx_args a;
  if (int rc = load_args(a, args, fn)) return rc;
  if (int rc = check_codebook(fn, a.dim, a.n_parts, a.n_clusters)) return rc;
  RSA_CHECK_ARG(a.n_queries >= 0 && a.num_neg >= 0 && a.n_pos >= 0, "%s: negative size", fn);
  RSA_CHECK_ARG(a.score_mode == RSA_SCORE_IP || a.score_mode == RSA_SCORE_COS, "%s: score_mode must be inner product or cosine", fn);
  if (a.n_queries == 0 || (a.num_neg == 0 && a.n_pos == 0)) return RSA_OK;
  RSA_CHECK_ARG(a.query && a.centres, "%s: query/centres is null", fn);
  RSA_CHECK_ARG(((uintptr_t)a.query & 15) == 0 && ((uintptr_t)a.centres & 15) == 0, "%s: query/centres must be 16-byte aligned", fn);
  RSA_CHECK_ARG(a.n_items >= 1 && a.n_items < (1ll << 31) - 1, "%s: n_items out of range", fn);
  if (a.num_neg > 0) {
    RSA_CHECK_ARG(a.wkk && a.indptr && a.indices, "%s: wkk/indptr/indices is null", fn);
    RSA_CHECK_ARG(a.neg_ids != nullptr, "%s: neg_ids is null", fn);
    RSA_CHECK_ARG(a.n_queries <= (1ll << 62) / ((int64_t)a.num_neg * 3), "%s: too many draws", fn);
    if (U_GIVEN) RSA_CHECK_ARG(a.u_in != nullptr, "%s: u_in is null", fn);
    else RSA_CHECK_ARG(a.grid_threads > 0 && (a.offset & 3) == 0, "%s: bad philox state", fn);
  }
  if (a.n_pos > 0) {
    RSA_CHECK_ARG(a.pos_ids && a.pos_logp && a.cd0 && (a.n_parts == 1 || a.cd1), "%s: pos_ids/pos_logp/cd is null", fn);
  }
  RSA_CHECK_ARG((a.cp != nullptr) == (a.item_logp != nullptr), "%s: cp and item_logp go together (both set or both null)", fn);
  const bool weighted = a.cp != nullptr;
  const int64_t lds = draw_lds_bytes(a.dim, a.n_parts, a.n_clusters);
  RSA_CHECK_ARG(lds <= LDS_LIMIT, "%s: codebook does not fit the LDS", fn);
  MidxParams p{a.query, a.n_queries, a.dim, a.n_parts, a.n_clusters, a.score_mode == RSA_SCORE_COS, a.centres, a.wkk, a.indptr,
               a.indices, a.n_items, a.cd0, a.cd1, a.num_neg, a.n_pos, a.pos_ids, a.u_in, a.neg_ids, a.neg_logp, a.pos_logp,
               U_GIVEN ? nullptr : a.u_out, PhiloxCall{a.seed, a.offset >> 2, a.grid_threads ? a.grid_threads : 1, a.elem_base},
               a.cp, a.item_logp};
  if (int rc = weighted ? allow_lds<midx_draw_kernel<U_GIVEN, true>>(lds, fn) : allow_lds<midx_draw_kernel<U_GIVEN, false>>(lds, fn))
    return rc;
  // the codebook is staged once per workgroup, so at most 1024 workgroups stride over the queries: 4 per CU, of which the
  // LDS lets 2 be resident at K = 64, d = 128 (58 KB each) and 1 at d = 256 (93 KB)
  const dim3 grid(grid_1d(a.n_queries, 4, 1024));
  if (weighted) hipLaunchKernelGGL((midx_draw_kernel<U_GIVEN, true>), grid, dim3(256), (size_t)lds, (hipStream_t)stream, p);
  else hipLaunchKernelGGL((midx_draw_kernel<U_GIVEN, false>), grid, dim3(256), (size_t)lds, (hipStream_t)stream, p);
  RSA_CHECK_LAUNCH(fn);
  return RSA_OK;
}

}  // namespace rsa

using namespace rsa;

extern "C" int rsa_midx_sample(const rsa_midx_args* args, rsa_stream_t stream) {
  return midx_entry<false>(args, stream, "rsa_midx_sample");
}

extern "C" int rsa_midx_lookup(const rsa_midx_args* args, rsa_stream_t stream) {
  return midx_entry<true>(args, stream, "rsa_midx_lookup");
}

extern "C" int rsa_midx_weights(const rsa_midx_weights_args* args, rsa_stream_t stream) {
  const char* fn = "rsa_midx_weights";
  rsa_midx_weights_args a;
  if (int rc = load_args(a, args, fn)) return rc;
  if (int rc = check_codebook(fn, a.dim, a.n_parts, a.n_clusters)) return rc;
  RSA_CHECK_ARG(a.n_items >= 1 && a.n_items < (1ll << 31) - 1, "%s: n_items out of range", fn);
  RSA_CHECK_ARG(a.pop && a.indptr && a.indices && a.p && a.item_logp && a.wkk && a.cp, "%s: null pointer", fn);
  const float* x = nullptr;
  if (a.table != nullptr) {
    RSA_CHECK_ARG(a.row_stride >= a.dim && a.row_stride % 4 == 0 && a.row_offset >= 0, "%s: row_stride must be a multiple of 4 >= dim, row_offset >= 0", fn);
    x = a.table + a.row_offset * a.row_stride;
    RSA_CHECK_ARG(((uintptr_t)x & 15) == 0, "%s: table must be 16-byte aligned", fn);
  }
  WeightParams p{a.pop, x, a.n_items, a.row_stride, a.dim, a.indptr, a.indices, a.p, a.item_logp, a.wkk, a.cp};
  const int64_t per_block = x ? 4 : 256;
  hipLaunchKernelGGL(midx_weight_rows_kernel, dim3(grid_1d(a.n_items, per_block, 8192)), dim3(256), 0, (hipStream_t)stream, p);
  RSA_CHECK_LAUNCH("rsa_midx_weights (row pass)");
  const int buckets = a.n_parts == 2 ? a.n_clusters * a.n_clusters : a.n_clusters;
  hipLaunchKernelGGL(midx_weight_buckets_kernel, dim3(buckets), dim3(WB_THREADS), 0, (hipStream_t)stream, p);
  RSA_CHECK_LAUNCH("rsa_midx_weights (bucket pass)");
  return RSA_OK;
}

extern "C" int64_t rsa_kmeans_workspace_bytes(int64_t n_rows, int32_t dim, int32_t n_clusters) {
  const int d = dim < 8 ? 8 : (dim > MIDX_MAX_DIM ? MIDX_MAX_DIM : dim);
  const int K = n_clusters < 2 ? 2 : (n_clusters > MIDX_MAX_K ? MIDX_MAX_K : n_clusters);
  return kmeans_layout(nullptr, n_rows, d, K).bytes + 256;
}

extern "C" int rsa_kmeans_step(const rsa_kmeans_args* args, rsa_stream_t stream) {
  const char* fn = "rsa_kmeans_step";
  rsa_kmeans_args a;
  if (int rc = load_args(a, args, fn)) return rc;
  if (int rc = check_codebook(fn, a.dim, a.n_parts, a.n_clusters)) return rc;
  RSA_CHECK_ARG(a.n_rows >= 1 && a.n_rows < (1ll << 31) - 1, "%s: n_rows out of range", fn);
  RSA_CHECK_ARG(a.table && a.centres && a.assign && a.sums && a.counts && a.loss, "%s: null pointer", fn);
  RSA_CHECK_ARG(a.row_stride >= a.dim && a.row_stride % 4 == 0 && a.row_offset >= 0, "%s: row_stride must be a multiple of 4 >= dim, row_offset >= 0", fn);
  const float* x = a.table + a.row_offset * a.row_stride;
  RSA_CHECK_ARG(((uintptr_t)x & 15) == 0 && ((uintptr_t)a.centres & 15) == 0, "%s: table/centres must be 16-byte aligned", fn);
  const KmeansLayout L = kmeans_layout(a.workspace, a.n_rows, a.dim, a.n_clusters);
  RSA_CHECK_ARG(a.workspace != nullptr && a.workspace_bytes >= L.bytes + 255, "%s: workspace too small (rsa_kmeans_workspace_bytes)", fn);
  const int64_t lds = kmeans_lds_bytes(a.dim, a.n_parts, a.n_clusters);
  RSA_CHECK_ARG(lds <= LDS_LIMIT, "%s: codebook does not fit the LDS", fn);
  if (int rc = allow_lds<kmeans_step_kernel>(lds, fn)) return rc;
  const unsigned grid = kmeans_grid(a.n_rows);
  KmeansParams p{x, a.n_rows, a.row_stride, a.dim, a.n_parts, a.n_clusters, a.normalize != 0, a.centres, a.assign, L.sums, L.counts, L.loss};
  hipLaunchKernelGGL(kmeans_step_kernel, dim3(grid), dim3(256), (size_t)lds, (hipStream_t)stream, p);
  RSA_CHECK_LAUNCH("rsa_kmeans_step (assignment pass)");
  const int outs = a.n_clusters * a.dim + a.n_parts * a.n_clusters + a.n_parts;
  hipLaunchKernelGGL(kmeans_reduce_kernel, dim3((outs + 255) / 256), dim3(256), 0, (hipStream_t)stream, p, (int)grid, a.sums, a.counts, a.loss);
  RSA_CHECK_LAUNCH("rsa_kmeans_step (reduction)");
  return RSA_OK;
}
