// LSH negative sampler: sign-random-projection hash, and the collision-weighted draw over the query's buckets (gfx950).
//
// rsa_lsh_hash                    : LSHSampler.update, the codes      recstudio/ann/sampler.py:600-604
// rsa_lsh_sample / rsa_lsh_lookup : LSHSampler.forward                recstudio/ann/sampler.py:609-677
//
// HASH.  The projections W [d, K, L] sit in LDS transposed, [K * L][d + CPAD]; lane c = k * L + l of a wave owns projection
// (k, l), so with K * L <= 64 one wave scores a row against all of them and the ballot of `dot > 0` is every sign bit at once.
//   dot = <x, W[:, k, l]>:  four interleaved FMA chains (chain m takes the elements i % 4 == m in ascending i, starting from 0),
//   summed (x + y) + (z + w) -- fma4 / sum4 of rsa_lds.hpp.  A term goes through at most d / 4 + 2 roundings, so
//   |dot - exact| <= gamma(d / 4 + 2) * sum |x_i w_i|; the referee (tests/lsh_referee.py) is written against this order.
//   code[l] = sum_k bit(k * L + l) << (K - 1 - k)   (the reference's K_base_vec: the first bit is the most significant).
// The hash pass stages tiles of 32 rows in LDS, a wave scores 8 of them (4 at a time), the tile's codes leave through LDS so
// that a table's 32 codes are one 128-byte store.  Nothing is accumulated across rows: two runs are bit-equal whatever the grid.
//
// DRAW.  One wave per query.  The query is hashed as above; lanes l < L read their bucket [start_l, start_l + cnt_l) from indptr,
// a wave prefix sum gives cum_l (inclusive, 64 bits) and len = cum_{L-1}.  Draw j of query q, with u = element q * n + j of ONE
// torch.rand(n_queries, n) (lane j % 64 of pass j / 64):
//   r = floor(fl32(u * fl32(len))), one IEEE multiply, clamped to len - 1      (fl32(len) may exceed len above 2^24)
//   t = #{l : cum_l <= r}: the upper bound of r in cum.  An empty table repeats its predecessor's cum and is never the first
//       to exceed r, so it is never chosen; r < len = cum_{L-1} keeps t < L.
//   item = indices[t][start_t + (r - cum_{t-1})],  id = item + 1.
// The wave then reads the snapshot row of every draw of the pass cooperatively (a float4 per lane, two batches of 8 rows in
// flight) and reduces <q, x> and ||x||^2; ||q||^2 once per query.  All three in fp32: a lane's four elements by dot4 (x0 y0, then
// three FMAs: 4 roundings), the lanes by six pairwise levels, nearest lanes first (wave_sum_near_first: 6 roundings; lanes past
// the row add exact zeros) -- 10 roundings at most on any term, whatever d.  From there on in double, one lane per draw:
//   c = dot / sqrt(||q||^2 ||x||^2) clamped to [-1, 1] (0 when a norm is 0),  p = 1 - acos(c) / pi,
//   w = -expm1(L * log1p(-p^K))   (= 1 - (1 - p^K)^L without the cancellation; p^K by K - 1 multiplications),
//   log-prob = fl32(log(w / len + log_eps)).
// A query whose buckets are all empty (len == 0) reads no row: id = 1 + min(floor(fl32(u * fl32(n_items))), n_items - 1) from
// the same uniform, log-prob 0.
#include "rsa_internal.hpp"
#include "rsa_lds.hpp"

namespace rsa {

constexpr int LSH_MAX_DIM = 256, LSH_MAX_BITS = 16, LSH_MAX_PROJ = 64;
constexpr int HASH_TILE = 32;           // rows per tile of the hash pass (8 per wave)
constexpr int HASH_MAX_GRID = 2048;
constexpr int DRAW_ROWS = 8;             // snapshot rows a wave reads per batch of the draw

extern __shared__ __attribute__((aligned(16))) float lsh_smem[];

// W [d][C] (C = K * L, column c = k * L + l) -> LDS [C][d + CPAD]
__device__ __forceinline__ void stage_projections(float* ws, const float* __restrict__ W, int C, int d) {
  const int stride = d + CPAD;
  for (int i = threadIdx.x; i < d * C; i += blockDim.x) {
    const int r = i / C, c = i - r * C;
    ws[c * stride + r] = W[i];
  }
}

// the code of table `l` from the wave's sign bits (bit k * L + l = projection (k, l))
__device__ __forceinline__ int32_t code_of(uint64_t bits, int l, int K, int L) {
  int32_t code = 0;
  for (int k = 0; k < K; ++k) code = (code << 1) | (int32_t)((bits >> (k * L + l)) & 1);
  return code;
}

// ---------------------------------------------------------------- hash pass
struct LshHashParams {
  const float* x;            // first row
  int64_t n_rows, row_stride;
  int dim, K, L;
  const float* W;
  int32_t* codes;            // [L][n_rows]
};

__global__ __launch_bounds__(256) void lsh_hash_kernel(const LshHashParams p) {
  const int K = p.K, L = p.L, C = K * L, d = p.dim, stride = d + CPAD, q4 = d >> 2;
  float* ws = lsh_smem;                                    // [C][d + CPAD]
  float* xt = ws + C * stride;                             // [HASH_TILE][d]
  int32_t* ct = reinterpret_cast<int32_t*>(xt + HASH_TILE * d);   // [L][HASH_TILE]
  const int lane = lane_id(), wave = threadIdx.x >> 6;
  stage_projections(ws, p.W, C, d);
  const int cc = lane < C ? lane : C - 1;
  const int64_t n_tiles = (p.n_rows + HASH_TILE - 1) / HASH_TILE;
  for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const int64_t row0 = tile * HASH_TILE;
    const int rows = (int)(p.n_rows - row0 < HASH_TILE ? p.n_rows - row0 : HASH_TILE);
    __syncthreads();                                       // the previous tile has been consumed (and ws is complete)
    for (int i = threadIdx.x; i < HASH_TILE * q4; i += blockDim.x) {
      const int r = i / q4, c = i - r * q4;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (r < rows) v = *reinterpret_cast<const float4*>(p.x + (row0 + r) * p.row_stride + c * 4);
      reinterpret_cast<float4*>(xt)[i] = v;
    }
    __syncthreads();
    const float* w = ws + cc * stride;
#pragma unroll
    for (int g = 0; g < 2; ++g) {
      const int rbase = wave * 8 + g * 4;
      const float* x = xt + rbase * d;
      float4 acc[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[r] = make_float4(0.f, 0.f, 0.f, 0.f);
      for (int i = 0; i < d; i += 4) {
        const float4 wv = *reinterpret_cast<const float4*>(w + i);
#pragma unroll
        for (int r = 0; r < 4; ++r) fma4(acc[r], *reinterpret_cast<const float4*>(x + r * d + i), wv);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const uint64_t bits = __ballot(lane < C && sum4(acc[r]) > 0.f);
        if (lane < L) ct[lane * HASH_TILE + rbase + r] = code_of(bits, lane, K, L);
      }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < L * HASH_TILE; i += blockDim.x) {
      const int l = i / HASH_TILE, r = i - l * HASH_TILE;
      if (r < rows) p.codes[(int64_t)l * p.n_rows + row0 + r] = ct[i];
    }
  }
}

static int64_t hash_lds_bytes(int dim, int C, int L) { return 4ll * (C * (dim + CPAD) + HASH_TILE * dim + L * HASH_TILE); }

// ---------------------------------------------------------------- draw
template <int CTRL>
__device__ __forceinline__ float dpp_move(float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xf, 0xf, false));
}

// Sum over the wave, every lane gets it.  Six pairwise levels, nearest lanes first: lane ^ 1, lane ^ 2 (quad permutes), the other
// quad of the 8 (row_half_mirror), the other 8 of the 16 (row_mirror) -- all DPP, no LDS traffic --, then lane ^ 16, lane ^ 32.
__device__ __forceinline__ float wave_sum_near_first(float v) {
  v += dpp_move<0xB1>(v);                                  // quad_perm [1, 0, 3, 2]
  v += dpp_move<0x4E>(v);                                  // quad_perm [2, 3, 0, 1]
  v += dpp_move<0x141>(v);                                 // row_half_mirror
  v += dpp_move<0x140>(v);                                 // row_mirror
  v += __shfl_xor(v, 16, 64);
  v += __shfl_xor(v, 32, 64);
  return v;
}

struct LshParams {
  const float* query;
  int64_t n_queries;
  int dim, K, L;
  const float* W;
  const int32_t* indptr;
  const int32_t* indices;
  const float* items;
  int64_t n_items;
  int num_neg;
  const float* u_in;
  int64_t* neg_ids;
  float* neg_logp;
  int32_t* codes_out;
  float* u_out;
  double log_eps;
  PhiloxCall pc;
};

// log(w / len + log_eps) of the header, from the fp32 reductions
__device__ __forceinline__ float collision_logp(float dot, float qq, float xx, int K, int L, int64_t len, double log_eps) {
  const double den = (double)qq * (double)xx;
  double c = den > 0.0 ? (double)dot / sqrt(den) : 0.0;
  c = c > 1.0 ? 1.0 : (c < -1.0 ? -1.0 : c);               // (a NaN row stays NaN)
  const double pr = 1.0 - acos(c) / 3.14159265358979323846;
  double pk = pr;
  for (int k = 1; k < K; ++k) pk *= pr;
  const double w = -expm1((double)L * log1p(-pk));
  return (float)log(w / (double)len + log_eps);
}

template <bool FROM_U>
__global__ __launch_bounds__(256) void lsh_draw_kernel(const LshParams p) {
  const int K = p.K, L = p.L, C = K * L, d = p.dim, stride = d + CPAD, q4 = d >> 2, n = p.num_neg;
  const int64_t N = p.n_items;
  float* ws = lsh_smem;                                    // [C][d + CPAD]
  float* qb = ws + C * stride;                             // [4][d]
  int64_t* cumb = reinterpret_cast<int64_t*>(qb + 4 * d);  // [4][64]  inclusive prefix of the bucket sizes
  int32_t* startb = reinterpret_cast<int32_t*>(cumb + 4 * 64);   // [4][64]  first position of the bucket
  const int lane = lane_id(), wave = threadIdx.x >> 6;
  stage_projections(ws, p.W, C, d);
  float* q_w = qb + wave * d;
  int64_t* cum_w = cumb + wave * 64;
  int32_t* start_w = startb + wave * 64;
  const int cc = lane < C ? lane : C - 1;
  const int64_t per_pass = (int64_t)gridDim.x * 4;
  for (int64_t q0 = (int64_t)blockIdx.x * 4; q0 < p.n_queries; q0 += per_pass) {     // block-uniform trip count
    const int64_t q = q0 + wave;
    const bool act = q < p.n_queries;
    float4 qv = make_float4(0.f, 0.f, 0.f, 0.f);
    float qq = 0.f;
    int64_t len = 0;
    __syncthreads();                                       // the previous query's LDS slots are free (and ws is complete)
    if (act) {
      if (lane < q4) {
        qv = reinterpret_cast<const float4*>(p.query + q * d)[lane];
        reinterpret_cast<float4*>(q_w)[lane] = qv;
      }
      qq = wave_sum_near_first(dot4(qv, qv));
    }
    __syncthreads();
    if (act) {
      const float* w = ws + cc * stride;
      float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
      for (int i = 0; i < d; i += 4) fma4(acc, *reinterpret_cast<const float4*>(q_w + i), *reinterpret_cast<const float4*>(w + i));
      const uint64_t bits = __ballot(lane < C && sum4(acc) > 0.f);
      int32_t start = 0, cnt = 0;
      if (lane < L) {
        const int32_t code = code_of(bits, lane, K, L);
        const int32_t* ip = p.indptr + (int64_t)lane * ((1 << K) + 1) + code;
        const int32_t lim = (int32_t)N;                    // (a bucket is a range of positions: never read past the table)
        const int32_t s = ip[0], e = ip[1];
        start = s < 0 ? 0 : (s > lim ? lim : s);
        cnt = (e > lim ? lim : e) - start;
        cnt = cnt < 0 ? 0 : cnt;
        if (p.codes_out) p.codes_out[q * L + lane] = code;
      }
      long long cum = cnt;
#pragma unroll
      for (int off = 1; off < 64; off <<= 1) {
        const long long t = __shfl_up(cum, off, 64);
        if (lane >= off) cum += t;
      }
      cum_w[lane] = cum;                                   // (lanes past L repeat the total)
      start_w[lane] = start;
      len = __shfl(cum, 63, 64);
    }
    __syncthreads();
    if (act) {
      for (int jb = 0; jb < n; jb += 64) {
        const int j = jb + lane;
        const bool have = j < n;
        float u = 0.f;
        if (have) u = FROM_U ? p.u_in[q * n + j] : torch_rand_element(p.pc, (uint64_t)(q * n + j));
        int32_t item = 0;
        int64_t id;
        if (len > 0) {
          int64_t r = (int64_t)floorf(__fmul_rn(u, (float)len));
          r = r < 0 ? 0 : (r > len - 1 ? len - 1 : r);
          int lo = 0, hi = L;
          while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (cum_w[mid] <= r) lo = mid + 1;
            else hi = mid;
          }
          const int t = lo < L ? lo : L - 1;
          int64_t pos = (int64_t)start_w[t] + (r - (t > 0 ? cum_w[t - 1] : 0));
          pos = pos < 0 ? 0 : (pos > N - 1 ? N - 1 : pos);
          item = p.indices[(int64_t)t * N + pos];
          item = item < 0 ? 0 : (item > (int32_t)N - 1 ? (int32_t)N - 1 : item);
          id = (int64_t)item + 1;
        } else {
          int64_t r = (int64_t)floorf(__fmul_rn(u, (float)N));
          r = r < 0 ? 0 : (r > N - 1 ? N - 1 : r);
          id = r + 1;
        }
        float logp = 0.f;
        if (len > 0) {                                     // wave-uniform
          float dot = 0.f, xx = 0.f;
          const int cnt_b = n - jb < 64 ? n - jb : 64;
          // (lanes past the last draw hold item 0: a row that exists)
          auto load_rows = [&](int jj, float4 (&x)[DRAW_ROWS]) {
#pragma unroll
            for (int r = 0; r < DRAW_ROWS; ++r) {
              const int32_t it = __shfl(item, (jj + r) & 63, 64);
              x[r] = make_float4(0.f, 0.f, 0.f, 0.f);
              if (lane < q4) x[r] = reinterpret_cast<const float4*>(p.items + (int64_t)it * d)[lane];
            }
          };
          auto reduce_rows = [&](int jj, const float4 (&x)[DRAW_ROWS]) {
#pragma unroll
            for (int r = 0; r < DRAW_ROWS; ++r) {
              const float dt = wave_sum_near_first(dot4(qv, x[r]));
              const float xs = wave_sum_near_first(dot4(x[r], x[r]));
              if (lane == jj + r) {
                dot = dt;
                xx = xs;
              }
            }
          };
          float4 xa[DRAW_ROWS], xb[DRAW_ROWS];             // two batches of rows in flight
          load_rows(0, xa);
          for (int jj = 0; jj < cnt_b; jj += 2 * DRAW_ROWS) {
            if (jj + DRAW_ROWS < cnt_b) load_rows(jj + DRAW_ROWS, xb);
            reduce_rows(jj, xa);
            if (jj + 2 * DRAW_ROWS < cnt_b) load_rows(jj + 2 * DRAW_ROWS, xa);
            if (jj + DRAW_ROWS < cnt_b) reduce_rows(jj + DRAW_ROWS, xb);
          }
          if (have) logp = collision_logp(dot, qq, xx, K, L, len, p.log_eps);
        }
        if (have) {
          p.neg_ids[q * n + j] = id;
          p.neg_logp[q * n + j] = logp;
          if (!FROM_U && p.u_out) p.u_out[q * n + j] = u;
        }
      }
    }
  }
}

static int64_t draw_lds_bytes(int dim, int C) { return 4ll * (C * (dim + CPAD) + 4 * dim) + 4 * 64 * (8 + 4); }

static int check_hash_shape(const char* fn, int dim, int K, int L) {
  RSA_CHECK_ARG(dim >= 8 && dim <= LSH_MAX_DIM && dim % 8 == 0, "%s: dim must be a multiple of 8 in [8, %d], got %d", fn, LSH_MAX_DIM, dim);
  RSA_CHECK_ARG(K >= 1 && K <= LSH_MAX_BITS, "%s: n_bits must be in [1, %d], got %d", fn, LSH_MAX_BITS, K);
  RSA_CHECK_ARG(L >= 1 && (int64_t)K * L <= LSH_MAX_PROJ, "%s: n_bits * n_table must be in [1, %d] (one lane per projection), got %d * %d",
                fn, LSH_MAX_PROJ, K, L);
  return RSA_OK;
}

template <bool U_GIVEN>
static int lsh_entry(const rsa_lsh_args* args, rsa_stream_t stream, const char* fn) {
  rsa_lsh_args a;
  if (int rc = load_args(a, args, fn)) return rc;
  if (int rc = check_hash_shape(fn, a.dim, a.n_bits, a.n_table)) return rc;
  RSA_CHECK_ARG(a.n_queries >= 0 && a.num_neg >= 0, "%s: negative size", fn);
  RSA_CHECK_ARG(a.log_eps >= 0.0, "%s: log_eps must not be negative", fn);
  if (a.n_queries == 0 || a.num_neg == 0) return RSA_OK;
  RSA_CHECK_ARG(a.query && a.weight_vectors && a.indptr && a.indices && a.item_embs, "%s: query/weight_vectors/indptr/indices/item_embs is null", fn);
  RSA_CHECK_ARG(a.neg_ids && a.neg_logp, "%s: neg_ids/neg_logp is null", fn);
  RSA_CHECK_ARG(((uintptr_t)a.query & 15) == 0 && ((uintptr_t)a.item_embs & 15) == 0, "%s: query/item_embs must be 16-byte aligned", fn);
  RSA_CHECK_ARG(a.n_items >= 1 && a.n_items < (1ll << 31) - 1, "%s: n_items out of range", fn);
  RSA_CHECK_ARG(a.n_queries <= (1ll << 62) / a.num_neg, "%s: too many draws", fn);
  if (U_GIVEN) RSA_CHECK_ARG(a.u_in != nullptr, "%s: u_in is null", fn);
  else RSA_CHECK_ARG(a.grid_threads > 0 && (a.offset & 3) == 0, "%s: bad philox state", fn);
  const int C = a.n_bits * a.n_table;
  const int64_t lds = draw_lds_bytes(a.dim, C);
  RSA_CHECK_ARG(lds <= LDS_LIMIT, "%s: the projections do not fit the LDS", fn);
  LshParams p{a.query, a.n_queries, a.dim, a.n_bits, a.n_table, a.weight_vectors, a.indptr, a.indices, a.item_embs, a.n_items,
              a.num_neg, a.u_in, a.neg_ids, a.neg_logp, a.codes_out, U_GIVEN ? nullptr : a.u_out, a.log_eps,
              PhiloxCall{a.seed, a.offset >> 2, a.grid_threads ? a.grid_threads : 1, a.elem_base}};
  if (int rc = allow_lds<lsh_draw_kernel<U_GIVEN>>(lds, fn)) return rc;
  // the projections are staged once per workgroup, so at most 1024 workgroups stride over the queries (rsa_midx.hip)
  hipLaunchKernelGGL((lsh_draw_kernel<U_GIVEN>), dim3(grid_1d(a.n_queries, 4, 1024)), dim3(256), (size_t)lds, (hipStream_t)stream, p);
  RSA_CHECK_LAUNCH(fn);
  return RSA_OK;
}

}  // namespace rsa

using namespace rsa;

extern "C" int rsa_lsh_sample(const rsa_lsh_args* args, rsa_stream_t stream) { return lsh_entry<false>(args, stream, "rsa_lsh_sample"); }

extern "C" int rsa_lsh_lookup(const rsa_lsh_args* args, rsa_stream_t stream) { return lsh_entry<true>(args, stream, "rsa_lsh_lookup"); }

extern "C" int rsa_lsh_hash(const rsa_lsh_hash_args* args, rsa_stream_t stream) {
  const char* fn = "rsa_lsh_hash";
  rsa_lsh_hash_args a;
  if (int rc = load_args(a, args, fn)) return rc;
  if (int rc = check_hash_shape(fn, a.dim, a.n_bits, a.n_table)) return rc;
  RSA_CHECK_ARG(a.n_rows >= 1 && a.n_rows < (1ll << 31) - 1, "%s: n_rows out of range", fn);
  RSA_CHECK_ARG(a.table && a.weight_vectors && a.codes, "%s: table/weight_vectors/codes is null", fn);
  RSA_CHECK_ARG(a.row_stride >= a.dim && a.row_stride % 4 == 0 && a.row_offset >= 0, "%s: row_stride must be a multiple of 4 >= dim, row_offset >= 0", fn);
  const float* x = a.table + a.row_offset * a.row_stride;
  RSA_CHECK_ARG(((uintptr_t)x & 15) == 0, "%s: table must be 16-byte aligned", fn);
  const int C = a.n_bits * a.n_table;
  const int64_t lds = hash_lds_bytes(a.dim, C, a.n_table);
  RSA_CHECK_ARG(lds <= LDS_LIMIT, "%s: the projections do not fit the LDS", fn);
  if (int rc = allow_lds<lsh_hash_kernel>(lds, fn)) return rc;
  LshHashParams p{x, a.n_rows, a.row_stride, a.dim, a.n_bits, a.n_table, a.weight_vectors, a.codes};
  // the grid is a function of the row count alone
  hipLaunchKernelGGL(lsh_hash_kernel, dim3(grid_1d(a.n_rows, HASH_TILE, HASH_MAX_GRID)), dim3(256), (size_t)lds, (hipStream_t)stream, p);
  RSA_CHECK_LAUNCH(fn);
  return RSA_OK;
}
