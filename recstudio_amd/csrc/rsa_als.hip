// WRMF's alternating-least-squares row solve (recstudio/model/mf/wrmf.py): for every requested CSR row r with index multiset S_r
//   A = alpha * sum_{e in S_r} y_e y_e^T + gram + lambda I        b = (1 + alpha) * sum_e rated_e y_e        x = A^-1 b
//   loss_r = (1 + alpha) * sum_e (rated_e - <x, y_e>)^2 - sum_e <x, y_e>^2 + x^T gram x                      (optional)
// y_e = table[indices[e]], gram = table^T table (the caller's GEMM, once per half-epoch).  Nothing of size B Lmax d or B d d ever
// reaches memory: a row's d x d system lives in the LDS of the workgroup that solves it.
//
// GRAM (als_gram_chunk).  v_mfma_f32_32x32x2f32 with the POSITIONS as the K dimension: a step takes two positions, lane (j, hh) reads
// position 2 t + hh and loads y[32 bi + j] for every 32-column block bi -- each half-wave reads one row's contiguous floats -- and
// tile (bi, bj), bi <= bj, is mfma(y[32 bi + j], y[32 bj + j]): both operands from the same registers.  Only the upper block triangle
// is computed: 1 / 3 / 10 tiles at d = 32 / 64 / 128.  b rides along as one multiply-add per block and lane.  The four waves of a
// workgroup take the steps t = w, w + 4, ... (ALS_UNROLL steps' loads in flight); positions past the end load the chunk's first
// row and multiply it by zero.  The waves' tiles and b meet in LDS in wave order 0, 1, 2, 3 (a wave without a step adds nothing).
//
// LONG ROWS.  A row of more than ALS_CHUNK positions is cut into ceil(K / ALS_CHUNK) parts.  als_parts_scan (one workgroup)
// counts the parts of every CSR row (slot of part c of row r = goff[r] + c) and of every requested row (work item list of the
// call); als_chunk_kernel strides over the work items, finds (row, part) of an item by two rounds of 256 compares, and leaves the
// part's (S, b) in its slot; the solving workgroup adds a row's parts in part order.  No float atomics, no host synchronisation, and
// a row's bits depend on that row alone: not on the batch, the grid or the run.  A repeated row writes the same bits to the same
// slots twice.  The slots (max_parts of them) are the caller's bound; a row whose parts lie past it gets status -1 and NaN.
//
// SOLVE (als_solve_kernel, one 256-thread workgroup per requested row).  A (upper triangle) and b as column d sit in LDS with a row
// stride of d + 1 floats (odd: a column walk touches every bank): 4.2 / 16.6 / 66 KB.  Right-looking Cholesky A = R^T R, two barriers
// per column: every thread reads the pivot, the row is divided by its root (the root itself goes to a side array, so no thread
// races the pivot read), then wave w updates the rows k + 1 + w, k + 5 + w, ... of the trailing triangle, a lane per column, the
// loads of four rows issued before the first store.  Carrying b as a column makes the forward solve R^T z = b part of the same
// sweep.  Wave 0 then solves R x = z by columns with z in registers (a readlane per column, no barrier).  The first non-positive (or NaN) pivot k sets status = k + 1 and the row
// writes NaN; nothing traps.
//
// LOSS.  A second pass over the row's positions in the direct form: d / 4 lanes per position (16-byte loads), the groups' sums in
// group order, the waves' in wave order, x^T gram x by a wave per gram row.  loss_only skips the solve and reads x from the caller.
#include "rsa_internal.hpp"
#include "rsa_lds.hpp"

namespace rsa {

using f32x16 = float __attribute__((ext_vector_type(16)));

constexpr int ALS_CHUNK = 1024;        // positions per part of a long row
constexpr int ALS_THREADS = 256;
constexpr int ALS_WAVES = ALS_THREADS / WAVE;
constexpr int ALS_UNROLL = 4;          // position pairs of a wave with their loads in flight
constexpr int ALS_SCAN_THREADS = 1024;
constexpr int ALS_CHUNK_GRID = 8192;

__device__ __forceinline__ int als_row32(int r, int hh) { return (r & 3) + 8 * (r >> 2) + 4 * hh; }
__host__ __device__ constexpr int als_ld(int d) { return d + 1; }
// LDS floats of a workgroup: the matrix with b as column d, the roots, x, the reduction words
__host__ __device__ constexpr int als_lds_floats(int d) { return d * als_ld(d) + 2 * d + 64; }
__host__ __device__ constexpr int64_t als_part_floats(int d) { return (int64_t)d * d + d; }

__device__ __forceinline__ int32_t als_parts(int64_t len) { return len > ALS_CHUNK ? (int32_t)((len + ALS_CHUNK - 1) / ALS_CHUNK) : 0; }

struct AlsParams {
  const int64_t* indptr;
  const int32_t* indices;
  const float* rated;
  const int64_t* rows;
  const float* table;
  const float* gram;
  int64_t n_csr, n_solve, max_parts;
  float alpha, lam;
  int32_t loss_only, chunked;
  float* x;
  float* loss;
  int32_t* status;
  int32_t *goff, *gbase, *boff, *bbase;      // parts before CSR row r / requested row b, and before every run of the scan
  float* parts;
};

// off[i] = parts of the entries before i (entry i = CSR row rows[i], or i), off[n] = their total; base[t] = off[t * per], per =
// ceil(n / ALS_SCAN_THREADS): the first level of the chunk kernel's search.  One workgroup, a contiguous run per thread.
__global__ __launch_bounds__(ALS_SCAN_THREADS) void als_parts_scan(const int64_t* __restrict__ indptr, const int64_t* __restrict__ rows,
                                                                   int64_t n, int32_t* __restrict__ off, int32_t* __restrict__ base) {
  __shared__ int32_t s_sum[ALS_SCAN_THREADS];
  const int t = threadIdx.x;
  const int64_t per = (n + ALS_SCAN_THREADS - 1) / ALS_SCAN_THREADS;
  const int64_t lo = t * per < n ? t * per : n, hi = lo + per < n ? lo + per : n;
  int32_t sum = 0;
  for (int64_t i = lo; i < hi; ++i) {
    const int64_t r = rows ? rows[i] : i;
    sum += als_parts(indptr[r + 1] - indptr[r]);
  }
  s_sum[t] = sum;
  __syncthreads();
  if (t == 0) {
    int32_t run = 0;
    for (int i = 0; i < ALS_SCAN_THREADS; ++i) {
      const int32_t v = s_sum[i];
      s_sum[i] = run;
      run += v;
    }
    off[n] = run;
    base[ALS_SCAN_THREADS] = run;
  }
  __syncthreads();
  int32_t run = s_sum[t];
  base[t] = run;
  for (int64_t i = lo; i < hi; ++i) {
    const int64_t r = rows ? rows[i] : i;
    off[i] = run;
    run += als_parts(indptr[r + 1] - indptr[r]);
  }
}

// (S, b) of the n >= 1 positions from edge s0 on, into the LDS matrix: S over the upper block triangle, b as column D.  Ends
// behind a barrier.
template <int D>
__device__ __forceinline__ void als_gram_chunk(const AlsParams& p, int64_t s0, int n, float* A) {
  constexpr int NB = D / 32, LD = als_ld(D);
  const int lane = lane_id(), wave = threadIdx.x >> 6, j = lane & 31, hh = lane >> 5;
  f32x16 acc[NB * (NB + 1) / 2];
#pragma unroll
  for (int t = 0; t < NB * (NB + 1) / 2; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
  float bacc[NB];
#pragma unroll
  for (int b = 0; b < NB; ++b) bacc[b] = 0.f;
  const int n_steps = (n + 1) >> 1;
  for (int q0 = wave; q0 < n_steps; q0 += ALS_WAVES * ALS_UNROLL) {
    float v[ALS_UNROLL][NB], w[ALS_UNROLL];
#pragma unroll
    for (int u = 0; u < ALS_UNROLL; ++u) {
      const int e = 2 * (q0 + u * ALS_WAVES) + hh;
      const bool ok = e < n;
      const int64_t at = s0 + (ok ? e : 0);
      const float* y = p.table + (size_t)p.indices[at] * (size_t)D + j;
      w[u] = p.rated ? p.rated[at] : 1.f;
#pragma unroll
      for (int b = 0; b < NB; ++b) v[u][b] = y[32 * b];
      if (!ok) {
        w[u] = 0.f;
#pragma unroll
        for (int b = 0; b < NB; ++b) v[u][b] = 0.f;
      }
    }
#pragma unroll
    for (int u = 0; u < ALS_UNROLL; ++u) {
      if (q0 + u * ALS_WAVES < n_steps) {            // wave-uniform
        int t = 0;
#pragma unroll
        for (int bi = 0; bi < NB; ++bi) {
          bacc[bi] += w[u] * v[u][bi];
#pragma unroll
          for (int bj = bi; bj < NB; ++bj, ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(v[u][bi], v[u][bj], acc[t], 0, 0, 0);
        }
      }
    }
  }
#pragma unroll
  for (int b = 0; b < NB; ++b) bacc[b] += __shfl_xor(bacc[b], 32, 64);      // the odd positions' half: a + b on both sides
  const int phases = n_steps < ALS_WAVES ? n_steps : ALS_WAVES;
  for (int ph = 0; ph < phases; ++ph) {
    if (wave == ph) {
      int t = 0;
#pragma unroll
      for (int bi = 0; bi < NB; ++bi) {
#pragma unroll
        for (int bj = bi; bj < NB; ++bj, ++t)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            float* at = A + (32 * bi + als_row32(r, hh)) * LD + 32 * bj + j;
            *at = ph == 0 ? acc[t][r] : *at + acc[t][r];
          }
        if (hh == 0) {
          float* at = A + (32 * bi + j) * LD + D;
          *at = ph == 0 ? bacc[bi] : *at + bacc[bi];
        }
      }
    }
    __syncthreads();
  }
}

// element idx of a part: [0, D * D) the matrix row-major, then b; false for the block rows below the diagonal (never written)
template <int D>
__device__ __forceinline__ bool als_part_elem(int idx, int& at) {
  const int i = idx < D * D ? idx / D : idx - D * D, c = idx < D * D ? idx - i * D : D;
  at = i * als_ld(D) + c;
  return c == D || (i >> 5) <= (c >> 5);
}

template <int D>
__global__ __launch_bounds__(ALS_THREADS) void als_chunk_kernel(const AlsParams p) {
  extern __shared__ __attribute__((aligned(16))) float als_smem[];
  __shared__ int64_t s_found[2];
  float* A = als_smem;
  const int t = threadIdx.x;
  const int32_t total = p.boff[p.n_solve];
  const int64_t per = (p.n_solve + ALS_SCAN_THREADS - 1) / ALS_SCAN_THREADS;
  for (int32_t item = (int32_t)blockIdx.x; item < total; item += (int32_t)gridDim.x) {
    // the run, then the entry, whose parts hold this item: exactly one non-empty [off[i], off[i + 1]) does
    for (int i = t; i < ALS_SCAN_THREADS; i += ALS_THREADS)
      if (p.bbase[i] <= item && item < p.bbase[i + 1]) s_found[0] = i;
    __syncthreads();
    const int64_t lo = s_found[0] * per, hi = lo + per < p.n_solve ? lo + per : p.n_solve;
    for (int64_t i = lo + t; i < hi; i += ALS_THREADS)
      if (p.boff[i] <= item && item < p.boff[i + 1]) s_found[1] = i;
    __syncthreads();
    const int64_t b = s_found[1];
    const int64_t r = p.rows ? p.rows[b] : b;
    const int32_t c = item - p.boff[b];
    const int64_t slot = (int64_t)p.goff[r] + c;
    if (slot < p.max_parts) {                      // workgroup-uniform
      const int64_t s = p.indptr[r], len = p.indptr[r + 1] - s;
      const int64_t left = len - (int64_t)c * ALS_CHUNK;
      als_gram_chunk<D>(p, s + (int64_t)c * ALS_CHUNK, (int)(left < ALS_CHUNK ? left : ALS_CHUNK), A);
      float* out = p.parts + (size_t)slot * (size_t)als_part_floats(D);
      for (int idx = t; idx < D * D + D; idx += ALS_THREADS) {
        int at;
        if (als_part_elem<D>(idx, at)) out[idx] = A[at];
      }
    }
    __syncthreads();                               // s_found and A are reused by the next item
  }
}

template <int D>
__global__ __launch_bounds__(ALS_THREADS) void als_solve_kernel(const AlsParams p) {
  extern __shared__ __attribute__((aligned(16))) float als_smem[];
  constexpr int LD = als_ld(D), NZ = (D + 63) / 64;
  float* A = als_smem;
  float* diag = A + D * LD;
  float* xs = diag + D;
  float* red = xs + D;
  const int t = threadIdx.x, lane = lane_id(), wave = t >> 6;
  const int64_t b = blockIdx.x;
  const int64_t r = p.rows ? p.rows[b] : b;
  const int64_t s = p.indptr[r], len = p.indptr[r + 1] - s;
  int32_t status = 0;
  if (p.loss_only) {
    if (t < D) xs[t] = p.x[(size_t)b * D + t];
    __syncthreads();
  } else if (len == 0) {                           // b = 0: x = 0
    if (t < D) p.x[(size_t)b * D + t] = 0.f;
    if (t == 0) {
      p.status[b] = 0;
      if (p.loss) p.loss[b] = 0.f;
    }
    return;
  } else {
    const int32_t n_parts = als_parts(len);
    if (n_parts == 0) {
      als_gram_chunk<D>(p, s, (int)len, A);
    } else if (!p.chunked || (int64_t)p.goff[r] + n_parts > p.max_parts) {
      status = -1;                                 // the caller's max_parts does not hold this row's parts
    } else {
      const float* part = p.parts + (size_t)p.goff[r] * (size_t)als_part_floats(D);
      for (int idx = t; idx < D * D + D; idx += ALS_THREADS) {
        int at;
        if (!als_part_elem<D>(idx, at)) continue;
        float v = part[idx];
        for (int32_t c = 1; c < n_parts; ++c) v += part[(size_t)c * (size_t)als_part_floats(D) + idx];
        A[at] = v;
      }
      __syncthreads();
    }
    if (status == 0) {
      const float one_alpha = 1.f + p.alpha;
      for (int idx = t; idx < D * D + D; idx += ALS_THREADS) {
        int at;
        if (!als_part_elem<D>(idx, at)) continue;
        if (idx < D * D) {
          const int i = idx / D, c = idx - i * D;
          if (c >= i) A[at] = (p.alpha * A[at] + p.gram[idx]) + (c == i ? p.lam : 0.f);
        } else {
          A[at] = one_alpha * A[at];
        }
      }
      __syncthreads();
      // ---- A = R^T R in place (upper triangle), z = R^-T b in column D
      for (int k = 0; k < D; ++k) {
        const float pivot = A[k * LD + k];
        if (!(pivot > 0.f) && status == 0) status = k + 1;
        const float root = sqrtf(pivot);
        if (t == 0) diag[k] = root;
        if (t < D - k) A[k * LD + k + 1 + t] = A[k * LD + k + 1 + t] / root;      // columns k + 1 .. D
        __syncthreads();
        // a lane keeps its column: row k's element is read once, and four rows' loads are issued before the first store (a load
        // behind a store to the same array waits for it: one row at a time was one LDS round trip per row)
        for (int c = k + 1 + lane; c <= D; c += WAVE) {
          const float rkc = A[k * LD + c];
          for (int i0 = k + 1 + wave; i0 < D && i0 <= c; i0 += ALS_WAVES * ALS_UNROLL) {
            float v[ALS_UNROLL], rki[ALS_UNROLL];
#pragma unroll
            for (int u = 0; u < ALS_UNROLL; ++u) {
              const int i = i0 + ALS_WAVES * u;
              const bool ok = i < D && i <= c;
              v[u] = A[(ok ? i : k) * LD + c];
              rki[u] = A[k * LD + (ok ? i : c)];
            }
#pragma unroll
            for (int u = 0; u < ALS_UNROLL; ++u) {
              const int i = i0 + ALS_WAVES * u;
              if (i < D && i <= c) A[i * LD + c] = v[u] - rki[u] * rkc;
            }
          }
        }
        __syncthreads();
      }
      // ---- R x = z by columns: lane i keeps z[i], z[64 + i]
      if (wave == 0) {
        float z[NZ];
#pragma unroll
        for (int q = 0; q < NZ; ++q) z[q] = 64 * q + lane < D ? A[(64 * q + lane) * LD + D] : 0.f;
#pragma unroll
        for (int q = NZ - 1; q >= 0; --q) {
          const int top = D - 64 * q < 64 ? D - 64 * q : 64;
          for (int kk = top - 1; kk >= 0; --kk) {
            const int k = 64 * q + kk;
            const float xk = __shfl(z[q], kk, 64) / diag[k];
            if (lane == 0) xs[k] = xk;
#pragma unroll
            for (int q2 = 0; q2 <= q; ++q2) {
              const int i = 64 * q2 + lane;
              if (i < k) z[q2] = z[q2] - A[i * LD + k] * xk;
            }
          }
        }
      }
      __syncthreads();
    }
    if (status != 0 && t < D) xs[t] = __builtin_nanf("");
    __syncthreads();
    if (t < D) p.x[(size_t)b * D + t] = xs[t];
    if (t == 0) p.status[b] = status;
  }
  if (p.loss == nullptr) return;
  // ---- the loss, in the direct form, with the x of xs
  constexpr int LP = D / 4, G = WAVE / LP;         // lanes per position, positions per wave and step
  const int grp = lane / LP, col = lane - grp * LP;
  const float4 x4 = *reinterpret_cast<const float4*>(xs + 4 * col);
  float t1 = 0.f, t2 = 0.f;
  for (int64_t e0 = 0; e0 < len; e0 += ALS_WAVES * G) {
    const int64_t e = e0 + wave * G + grp;
    const bool ok = e < len;
    const int64_t at = s + (ok ? e : 0);
    const float4 y4 = *reinterpret_cast<const float4*>(p.table + (size_t)p.indices[at] * (size_t)D + 4 * col);
    const float w = p.rated ? p.rated[at] : 1.f;
    const float dot = group_sum<LP>(dot4(x4, y4));
    const float diff = w - dot;
    t1 += ok ? diff * diff : 0.f;
    t2 += ok ? dot * dot : 0.f;
  }
  float w1 = 0.f, w2 = 0.f;
#pragma unroll
  for (int g = 0; g < G; ++g) {                    // the groups' sums in group order
    w1 += __shfl(t1, g * LP, 64);
    w2 += __shfl(t2, g * LP, 64);
  }
  float quad = 0.f;                                // x^T gram x: wave w takes the gram rows w, w + 4, ...
  for (int i = wave; i < D; i += ALS_WAVES) {
    float part = 0.f;
#pragma unroll
    for (int q = 0; q < NZ; ++q) {
      const int c = 64 * q + lane;
      if (c < D) part += p.gram[i * D + c] * xs[c];
    }
    quad += xs[i] * group_sum<64>(part);
  }
  if (lane == 0) red[3 * wave] = w1, red[3 * wave + 1] = w2, red[3 * wave + 2] = quad;
  __syncthreads();
  if (t == 0) {
    float s1 = 0.f, s2 = 0.f, sq = 0.f;
    for (int wv = 0; wv < ALS_WAVES; ++wv) s1 += red[3 * wv], s2 += red[3 * wv + 1], sq += red[3 * wv + 2];
    p.loss[b] = ((1.f + p.alpha) * s1 - s2) + sq;
  }
}

struct AlsLayout {
  int32_t *goff, *gbase, *boff, *bbase;
  float* parts;
};

static AlsLayout als_layout(Carver& cv, int64_t n_csr, int64_t n_solve, int64_t max_parts, int32_t d) {
  AlsLayout y{};
  y.goff = cv.take<int32_t>(n_csr + 1);
  y.gbase = cv.take<int32_t>(ALS_SCAN_THREADS + 1);
  y.boff = cv.take<int32_t>(n_solve + 1);
  y.bbase = cv.take<int32_t>(ALS_SCAN_THREADS + 1);
  y.parts = cv.take<float>(max_parts * als_part_floats(d));
  return y;
}

static bool als_sizes_ok(int64_t n_csr, int64_t n_solve, int64_t max_parts, int32_t d) {
  return n_csr >= 0 && n_csr < (1ll << 31) && n_solve >= 0 && n_solve < (1ll << 31) && max_parts >= 0 && max_parts < (1ll << 31) &&
         (d == 32 || d == 64 || d == 128);
}

template <int D>
static int als_launch(AlsParams& p, const rsa_als_args& a, hipStream_t s, const char* fn) {
  const int64_t lds = (int64_t)als_lds_floats(D) * (int64_t)sizeof(float);
  static_assert((int64_t)als_lds_floats(128) * 4 <= LDS_LIMIT, "the d = 128 system must fit the LDS of one workgroup");
  if (int rc = allow_lds<als_solve_kernel<D>>(lds, fn)) return rc;
  if (p.chunked && !p.loss_only) {
    if (int rc = allow_lds<als_chunk_kernel<D>>(lds, fn)) return rc;
    hipLaunchKernelGGL(als_parts_scan, dim3(1), dim3(ALS_SCAN_THREADS), 0, s, p.indptr, (const int64_t*)nullptr, p.n_csr, p.goff, p.gbase);
    RSA_CHECK_LAUNCH(fn);
    if (p.rows) {
      hipLaunchKernelGGL(als_parts_scan, dim3(1), dim3(ALS_SCAN_THREADS), 0, s, p.indptr, p.rows, p.n_solve, p.boff, p.bbase);
      RSA_CHECK_LAUNCH(fn);
    } else {
      p.boff = p.goff, p.bbase = p.gbase;
    }
    hipLaunchKernelGGL(als_chunk_kernel<D>, dim3(grid_1d(p.max_parts, 1, ALS_CHUNK_GRID)), dim3(ALS_THREADS), (size_t)lds, s, p);
    RSA_CHECK_LAUNCH(fn);
  }
  hipLaunchKernelGGL(als_solve_kernel<D>, dim3((unsigned)p.n_solve), dim3(ALS_THREADS), (size_t)lds, s, p);
  RSA_CHECK_LAUNCH(fn);
  return RSA_OK;
}

}  // namespace rsa

using namespace rsa;

extern "C" int64_t rsa_als_workspace_bytes(int64_t n_csr_rows, int64_t n_solve, int64_t max_parts, int32_t d) {
  if (!als_sizes_ok(n_csr_rows, n_solve, max_parts, d)) return -1;
  Carver cv(nullptr);
  als_layout(cv, n_csr_rows, n_solve, max_parts, d);
  return cv.bytes() + 256;
}

extern "C" int rsa_als_solve(const rsa_als_args* args, rsa_stream_t stream) {
  const char* fn = "rsa_als_solve";
  rsa_als_args a;
  if (int rc = load_args(a, args, fn)) return rc;
  RSA_CHECK_ARG(a.d == 32 || a.d == 64 || a.d == 128, "%s: d = %d is not 32, 64 or 128", fn, a.d);
  RSA_CHECK_ARG(als_sizes_ok(a.n_csr_rows, a.n_solve, a.max_parts, a.d), "%s: n_csr_rows = %lld, n_solve = %lld, max_parts = %lld out of "
                "range (each must stay below 2^31)", fn, (long long)a.n_csr_rows, (long long)a.n_solve, (long long)a.max_parts);
  RSA_CHECK_ARG(a.nnz >= 0 && a.n_table >= 1 && a.n_table < (1ll << 31), "%s: nnz = %lld, n_table = %lld out of range", fn,
                (long long)a.nnz, (long long)a.n_table);
  RSA_CHECK_ARG(a.rows != nullptr || a.n_solve == a.n_csr_rows, "%s: rows is null, so n_solve = %lld must be n_csr_rows = %lld", fn,
                (long long)a.n_solve, (long long)a.n_csr_rows);
  RSA_CHECK_ARG(a.loss_only == 0 || a.loss != nullptr, "%s: loss_only without loss", fn);
  if (a.n_solve == 0) return RSA_OK;
  RSA_CHECK_ARG(a.indptr != nullptr, "%s: indptr is null", fn);
  RSA_CHECK_ARG(a.nnz == 0 || a.indices != nullptr, "%s: indices is null", fn);
  RSA_CHECK_ARG(a.table && ((uintptr_t)a.table & 15) == 0, "%s: table is null or not 16-byte aligned", fn);
  RSA_CHECK_ARG(a.gram != nullptr, "%s: gram is null", fn);
  RSA_CHECK_ARG(a.x != nullptr, "%s: x is null", fn);
  RSA_CHECK_ARG(a.loss_only != 0 || a.status != nullptr, "%s: status is null", fn);
  AlsParams p{};
  p.indptr = a.indptr, p.indices = a.indices, p.rated = a.rated, p.rows = a.rows, p.table = a.table, p.gram = a.gram;
  p.n_csr = a.n_csr_rows, p.n_solve = a.n_solve, p.max_parts = a.max_parts, p.alpha = a.alpha, p.lam = a.lam;
  p.loss_only = a.loss_only, p.chunked = a.max_parts > 0, p.x = a.x, p.loss = a.loss, p.status = a.status;
  if (p.chunked && !p.loss_only) {
    RSA_CHECK_ARG(a.workspace != nullptr, "%s: workspace is null (max_parts = %lld parts of long rows live in it)", fn, (long long)a.max_parts);
    const int64_t need = rsa_als_workspace_bytes(a.n_csr_rows, a.n_solve, a.max_parts, a.d);
    RSA_CHECK_ARG(a.workspace_bytes >= need, "%s: the workspace is too small: %lld bytes, need %lld", fn, (long long)a.workspace_bytes,
                  (long long)need);
    Carver cv(a.workspace);
    const AlsLayout y = als_layout(cv, a.n_csr_rows, a.n_solve, a.max_parts, a.d);
    p.goff = y.goff, p.gbase = y.gbase, p.boff = y.boff, p.bbase = y.bbase, p.parts = y.parts;
  }
  hipStream_t s = (hipStream_t)stream;
  int rc = RSA_ERR_UNSUPPORTED;
  dispatch_dim<32, 64, 128>(a.d, [&](auto D) { rc = als_launch<D()>(p, a, s, fn); });
  return rc;
}
