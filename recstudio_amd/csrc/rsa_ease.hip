// EASE (recstudio/model/mf/ease.py) on gfx950, all float64: the Gram matrix G = R^T R + lambda I from integer LDS counts
// (rsa_ease_gram), P = G^-1 by a blocked Cholesky factorisation, triangular inverse and W^T W on v_mfma_f64_16x16x4_f64
// (rsa_spd_inverse_f64), B = P / (-diag P) with the closed-form epoch loss (rsa_ease_weights) and history x B scores
// (rsa_ease_score).  include/recstudio_amd.h states the contract, DESIGN.md 4.23 the design.
//
// INVERSE.  Blocks of 64, every launch on the caller's stream.  Two device functions carry it:
//   diag_block   one workgroup, the 64 x 64 diagonal block in LDS: unblocked Cholesky (column scale, then a rank-1 update of the
//                trailing triangle by all 256 threads), the factor written back, then the in-place triangular inverse by columns
//                from the last to the first (x = -X[j+1:, j+1:] l / l_jj, four threads per row), written to the side array.
//   tile_gemm    acc[64 x 64] = sum over k in [k0, k1) of opA[m, k] opB[n, k]: 256 threads, wave w owns the 32 x 32 quadrant
//                (w / 2, w % 2) as 2 x 2 MFMA tiles (16 accumulator doubles per lane).  K goes through LDS in slabs of 32, two
//                buffers per operand: the next slab's global loads (16 bytes per lane where the alignment allows) are in flight
//                while the MFMAs read the current one, one barrier per slab.  An operand whose k runs along memory is kept
//                [64][34] in LDS, one whose m runs along memory [32][80]: in either the 16 rows x 4 k of one MFMA operand are one
//                ds_read_b64 per lane and a half-wave touches every bank once.  Elements outside the matrix read as zero.
// The callers give tile_gemm only the k blocks that the triangular structure leaves:
//   factor   column k:  A[i, k] -= sum_{p < k} L[i, p] L[k, p]^T  (i >= k, k blocks);  diag_block;  L[i, k] = A[i, k] L_kk^-T
//   invert   row i:     T[j] = sum_{j <= p < i} L[i, p] W[p, j] to the row panel (tile j' still reads the L[i, j] that W[i, j]
//                       replaces);  W[i, j] = -L_ii^-1 T[j],  W[i, i] = L_ii^-1
//   product  P[i, j] = sum_{p >= i} W[p, i]^T W[p, j]  (j <= i), staged in LDS and stored with its transpose.
#include <cmath>

#include "rsa_csr.hpp"
#include "rsa_launch.hpp"
#include "rsa_lds.hpp"

namespace rsa {

typedef double f64x4 __attribute__((ext_vector_type(4)));

constexpr int SPD_NB = RSA_SPD_BLOCK, SPD_THREADS = 256, SPD_SLAB = 32;
constexpr int SPD_LD_KC = SPD_SLAB + 2;                  // [64][34]: k along a row
constexpr int SPD_LD_MC = SPD_NB + 16;                   // [32][80]: m along a row
constexpr int SPD_SLAB_DOUBLES = SPD_SLAB * SPD_LD_MC;   // the larger of the two
constexpr int SPD_TS = SPD_NB + 1;                       // a staged 64 x 64 tile, row stride 65
constexpr int64_t SPD_GEMM_LDS = 4ll * SPD_SLAB_DOUBLES * 8;
static_assert(SPD_NB * SPD_LD_KC <= SPD_SLAB_DOUBLES, "either slab layout fits one buffer");
static_assert(SPD_NB * SPD_TS <= 4 * SPD_SLAB_DOUBLES, "the staged output tile reuses the slab buffers");
static_assert(SPD_GEMM_LDS <= LDS_LIMIT, "the slab buffers fit the LDS of one workgroup");
static_assert(SPD_NB == 64 && SPD_THREADS == 256 && SPD_SLAB == 32, "the index arithmetic below is written for these");

// One GEMM operand: element (m, k) lives at p[m * sm + k * sk] (one of the strides is 1) and reads as 0 unless m < m_lim and
// k < k_lim.  vec: p is 16-byte aligned and the other stride is even, so two neighbours along the unit stride are one load.
struct SpdOperand {
  const double* p;
  int64_t sm, sk, m_lim, k_lim;
  bool vec;
};

// thread t's four pairs of a 64 x 32 slab: pair idx = t + 256 q; KC: (m = idx / 16, k = 2 (idx % 16)); MC: (k = idx / 32, m = 2 (idx % 32))
template <bool KC>
__device__ __forceinline__ void spd_slab_load(const SpdOperand& o, int64_t k0, int t, double2 (&r)[4]) {
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int idx = t + SPD_THREADS * q;
    const int64_t m = KC ? (idx >> 4) : ((idx & 31) * 2);
    const int64_t k = k0 + (KC ? ((idx & 15) * 2) : (idx >> 5));
    const bool in0 = m < o.m_lim && k < o.k_lim;
    const bool in1 = KC ? (m < o.m_lim && k + 1 < o.k_lim) : (m + 1 < o.m_lim && k < o.k_lim);
    const double* src = o.p + m * o.sm + k * o.sk;
    if (in1 && o.vec) {
      r[q] = *reinterpret_cast<const double2*>(src);
    } else {
      r[q].x = in0 ? src[0] : 0.0;
      r[q].y = in1 ? src[1] : 0.0;
    }
  }
}

template <bool KC>
__device__ __forceinline__ void spd_slab_store(double* lds, int t, const double2 (&r)[4]) {
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int idx = t + SPD_THREADS * q;
    const int at = KC ? ((idx >> 4) * SPD_LD_KC + (idx & 15) * 2) : ((idx >> 5) * SPD_LD_MC + (idx & 31) * 2);
    *reinterpret_cast<double2*>(lds + at) = r[q];
  }
}

template <bool KC>
__device__ __forceinline__ double spd_slab_at(const double* lds, int m, int k) {
  return KC ? lds[m * SPD_LD_KC + k] : lds[k * SPD_LD_MC + m];
}

// The operand and result layout of v_mfma_f64_16x16x4_f64 (pinned by tests/test_gpu_ease.py at n = 16): lane l gives
// A[l % 16][l / 16] and B[l / 16][l % 16] and receives D[4 r + l / 16][l % 16] in element r (the fp32 16x16x4 form has
// D[4 (l / 16) + r] there: measured, the first version of this file assumed it).
template <bool AKC, bool BKC>
__device__ __forceinline__ void spd_slab_mma(const double* la, const double* lb, int wm, int wn, int lane, f64x4 (&acc)[2][2]) {
  const int l16 = lane & 15, lk = lane >> 4;
#pragma unroll
  for (int ks = 0; ks < SPD_SLAB; ks += 4) {
    double a[2], b[2];
#pragma unroll
    for (int x = 0; x < 2; ++x) {
      a[x] = spd_slab_at<AKC>(la, wm + 16 * x + l16, ks + lk);
      b[x] = spd_slab_at<BKC>(lb, wn + 16 * x + l16, ks + lk);
    }
#pragma unroll
    for (int x = 0; x < 2; ++x)
#pragma unroll
      for (int y = 0; y < 2; ++y) acc[x][y] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[x], b[y], acc[x][y], 0, 0, 0);
  }
}

// acc = sum_{k0 <= k < k1} A(m, k) B(n, k); k1 - k0 is a multiple of the slab.  All threads of the workgroup call it together; the
// LDS is free again on return.
template <bool AKC, bool BKC>
__device__ __forceinline__ void tile_gemm(const SpdOperand& A, const SpdOperand& B, int64_t k0, int64_t k1, double* lds,
                                          f64x4 (&acc)[2][2]) {
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int wm = (wave >> 1) * 32, wn = (wave & 1) * 32;
#pragma unroll
  for (int x = 0; x < 2; ++x)
#pragma unroll
    for (int y = 0; y < 2; ++y) acc[x][y] = f64x4{0.0, 0.0, 0.0, 0.0};
  if (k0 >= k1) return;
  double2 ra[4], rb[4];
  spd_slab_load<AKC>(A, k0, t, ra);
  spd_slab_load<BKC>(B, k0, t, rb);
  spd_slab_store<AKC>(lds, t, ra);
  spd_slab_store<BKC>(lds + SPD_SLAB_DOUBLES, t, rb);
  __syncthreads();
  int buf = 0;
  for (int64_t k = k0; k < k1; k += SPD_SLAB) {
    const bool more = k + SPD_SLAB < k1;
    double* cur = lds + buf * 2 * SPD_SLAB_DOUBLES;
    double* nxt = lds + (buf ^ 1) * 2 * SPD_SLAB_DOUBLES;
    if (more) {
      spd_slab_load<AKC>(A, k + SPD_SLAB, t, ra);
      spd_slab_load<BKC>(B, k + SPD_SLAB, t, rb);
    }
    spd_slab_mma<AKC, BKC>(cur, cur + SPD_SLAB_DOUBLES, wm, wn, lane, acc);
    if (more) {
      spd_slab_store<AKC>(nxt, t, ra);
      spd_slab_store<BKC>(nxt + SPD_SLAB_DOUBLES, t, rb);
    }
    __syncthreads();
    buf ^= 1;
  }
}

// f(row, col, value) for the 16 elements of the 64 x 64 tile that this lane holds
template <class F>
__device__ __forceinline__ void spd_each(const f64x4 (&acc)[2][2], F&& f) {
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int wm = (wave >> 1) * 32, wn = (wave & 1) * 32;
#pragma unroll
  for (int x = 0; x < 2; ++x)
#pragma unroll
    for (int y = 0; y < 2; ++y)
#pragma unroll
      for (int r = 0; r < 4; ++r) f(wm + 16 * x + 4 * r + (lane >> 4), wn + 16 * y + (lane & 15), acc[x][y][r]);
}

struct SpdParams {
  double *a, *p, *linv, *panel;
  int32_t* status;
  int64_t n, ld, ldp, npad;
  int32_t nb, k;       // the block column (factor) or block row (invert) of this launch
  bool vec;            // a's rows can be read 16 bytes at a time
};

__device__ __forceinline__ SpdOperand spd_rows_of_a(const SpdParams& p, int64_t row_block) {       // (m, k) = a[64 rb + m][k]
  return SpdOperand{p.a + row_block * SPD_NB * p.ld, p.ld, 1, p.n - row_block * SPD_NB, p.n, p.vec};
}
__device__ __forceinline__ SpdOperand spd_cols_of_a(const SpdParams& p, int64_t col_block) {       // (m, k) = a[k][64 cb + m]
  return SpdOperand{p.a + col_block * SPD_NB, 1, p.ld, p.n - col_block * SPD_NB, p.n, p.vec};
}
__device__ __forceinline__ SpdOperand spd_linv(const SpdParams& p, int64_t block) {                // (m, k) = L_bb^-1[m][k]
  return SpdOperand{p.linv + block * SPD_NB * SPD_NB, SPD_NB, 1, SPD_NB, SPD_NB, true};
}

// factor, step 1: A[i, k] -= L[i, :k] L[k, :k]^T for i = k + blockIdx.x
__global__ __launch_bounds__(SPD_THREADS) void spd_update_kernel(const SpdParams p) {
  extern __shared__ double spd_lds[];
  const int64_t i = p.k + (int64_t)blockIdx.x, k = p.k;
  f64x4 acc[2][2];
  tile_gemm<true, true>(spd_rows_of_a(p, i), spd_rows_of_a(p, k), 0, k * SPD_NB, spd_lds, acc);
  spd_each(acc, [&](int r, int c, double v) {
    const int64_t gr = i * SPD_NB + r, gc = k * SPD_NB + c;
    if (gr < p.n && gc < p.n) p.a[gr * p.ld + gc] -= v;
  });
}

// factor, step 2: the diagonal block k: L_kk in place (lower triangle), L_kk^-1 (full, zeros above the diagonal) to the side array
__global__ __launch_bounds__(SPD_THREADS) void spd_diag_kernel(const SpdParams p) {
  __shared__ double S[SPD_NB * SPD_TS];
  __shared__ double col[SPD_NB];
  const int t = threadIdx.x;
  const int64_t base = (int64_t)p.k * SPD_NB;
  if (p.k == 0 && t == 0) *p.status = 0;
  for (int idx = t; idx < SPD_NB * SPD_NB; idx += SPD_THREADS) {
    const int r = idx >> 6, c = idx & 63;
    const int64_t gr = base + r, gc = base + c;
    S[r * SPD_TS + c] = (gr < p.n && gc < p.n) ? p.a[gr * p.ld + gc] : (r == c ? 1.0 : 0.0);     // a ragged block: the identity
  }
  __syncthreads();
  const int row = t >> 2, part = t & 3;
  int bad = -1;
  for (int c = 0; c < SPD_NB; ++c) {
    const double pivot = S[c * SPD_TS + c];
    if (!(pivot > 0.0)) {                            // the same LDS word for every thread: uniform
      bad = c;
      break;
    }
    const double d = sqrt(pivot);
    __syncthreads();
    if (t == c) S[c * SPD_TS + c] = d;
    else if (t > c && t < SPD_NB) S[t * SPD_TS + c] = S[t * SPD_TS + c] / d;
    __syncthreads();
    if (row > c) {
      const double lrc = S[row * SPD_TS + c];
      for (int q = c + 1 + part; q <= row; q += 4) S[row * SPD_TS + q] -= lrc * S[q * SPD_TS + c];
    }
    __syncthreads();
  }
  double* linv = p.linv + (int64_t)p.k * SPD_NB * SPD_NB;
  if (bad >= 0) {                                    // first bad pivot wins; the block and what follows from it is NaN
    if (t == 0) atomicCAS(p.status, 0, (int32_t)(base + bad + 1));
    const double nan = __builtin_nan("");
    for (int idx = t; idx < SPD_NB * SPD_NB; idx += SPD_THREADS) {
      const int r = idx >> 6, c = idx & 63;
      const int64_t gr = base + r, gc = base + c;
      if (c <= r && gr < p.n) p.a[gr * p.ld + gc] = nan;
      linv[idx] = nan;
    }
    return;
  }
  for (int idx = t; idx < SPD_NB * SPD_NB; idx += SPD_THREADS) {
    const int r = idx >> 6, c = idx & 63;
    const int64_t gr = base + r, gc = base + c;
    if (c <= r && gr < p.n) p.a[gr * p.ld + gc] = S[r * SPD_TS + c];
  }
  // X = L^-1 in place, columns from the last: X[j][j] = 1 / l_jj, X[r][j] = -X[j][j] sum_{j < q <= r} X[r][q] l_qj
  for (int j = SPD_NB - 1; j >= 0; --j) {
    const double djj = 1.0 / S[j * SPD_TS + j];
    if (t > j && t < SPD_NB) col[t] = S[t * SPD_TS + j];
    __syncthreads();
    double s = 0.0;
    if (row > j)
      for (int q = j + 1 + part; q <= row; q += 4) s += S[row * SPD_TS + q] * col[q];
    s += __shfl_xor(s, 1, 64);
    s += __shfl_xor(s, 2, 64);                       // (s0 + s1) + (s2 + s3) in every lane of the four
    if (part == 0 && row > j) S[row * SPD_TS + j] = -(djj * s);
    if (t == 0) S[j * SPD_TS + j] = djj;
    __syncthreads();
  }
  for (int idx = t; idx < SPD_NB * SPD_NB; idx += SPD_THREADS) {
    const int r = idx >> 6, c = idx & 63;
    linv[idx] = c <= r ? S[r * SPD_TS + c] : 0.0;
  }
}

// factor, step 3: L[i, k] = A[i, k] L_kk^-T for i = k + 1 + blockIdx.x (the tile reads only itself: in place)
__global__ __launch_bounds__(SPD_THREADS) void spd_panel_kernel(const SpdParams p) {
  extern __shared__ double spd_lds[];
  const int64_t i = p.k + 1 + (int64_t)blockIdx.x, k = p.k;
  SpdOperand A = spd_rows_of_a(p, i);
  A.p += k * SPD_NB, A.k_lim = p.n - k * SPD_NB;
  f64x4 acc[2][2];
  tile_gemm<true, true>(A, spd_linv(p, k), 0, SPD_NB, spd_lds, acc);
  spd_each(acc, [&](int r, int c, double v) {
    const int64_t gr = i * SPD_NB + r, gc = k * SPD_NB + c;
    if (gr < p.n && gc < p.n) p.a[gr * p.ld + gc] = v;
  });
}

// invert, step 1: panel[:, j] = sum_{j <= q < i} L[i, q] W[q, j] for j = blockIdx.x < i = p.k
__global__ __launch_bounds__(SPD_THREADS) void spd_trow_kernel(const SpdParams p) {
  extern __shared__ double spd_lds[];
  const int64_t i = p.k, j = blockIdx.x;
  f64x4 acc[2][2];
  tile_gemm<true, false>(spd_rows_of_a(p, i), spd_cols_of_a(p, j), j * SPD_NB, i * SPD_NB, spd_lds, acc);
  spd_each(acc, [&](int r, int c, double v) { p.panel[(int64_t)r * p.npad + j * SPD_NB + c] = v; });
}

// invert, step 2: W[i, j] = -L_ii^-1 panel[:, j] for j = blockIdx.x < i; the workgroup j == i copies L_ii^-1 into the diagonal block
__global__ __launch_bounds__(SPD_THREADS) void spd_wrow_kernel(const SpdParams p) {
  extern __shared__ double spd_lds[];
  const int64_t i = p.k, j = blockIdx.x;
  if (j == i) {
    const double* linv = p.linv + i * SPD_NB * SPD_NB;
    for (int idx = threadIdx.x; idx < SPD_NB * SPD_NB; idx += SPD_THREADS) {
      const int64_t gr = i * SPD_NB + (idx >> 6), gc = i * SPD_NB + (idx & 63);
      if (gr < p.n && gc < p.n) p.a[gr * p.ld + gc] = linv[idx];
    }
    return;
  }
  const SpdOperand T{p.panel + j * SPD_NB, 1, p.npad, SPD_NB, SPD_NB, true};
  f64x4 acc[2][2];
  tile_gemm<true, false>(spd_linv(p, i), T, 0, SPD_NB, spd_lds, acc);
  spd_each(acc, [&](int r, int c, double v) {
    const int64_t gr = i * SPD_NB + r, gc = j * SPD_NB + c;
    if (gr < p.n && gc < p.n) p.a[gr * p.ld + gc] = -v;
  });
}

// product: P[i, j] = sum_{q >= i} W[q, i]^T W[q, j] for (j, i) = (blockIdx.x, blockIdx.y), j <= i, and its transpose
__global__ __launch_bounds__(SPD_THREADS) void spd_wtw_kernel(const SpdParams p) {
  extern __shared__ double spd_lds[];
  const int64_t j = blockIdx.x, i = blockIdx.y;
  if (j > i) return;
  f64x4 acc[2][2];
  tile_gemm<false, false>(spd_cols_of_a(p, i), spd_cols_of_a(p, j), i * SPD_NB, p.npad, spd_lds, acc);
  spd_each(acc, [&](int r, int c, double v) { spd_lds[r * SPD_TS + c] = v; });
  __syncthreads();
  for (int idx = threadIdx.x; idx < SPD_NB * SPD_NB; idx += SPD_THREADS) {
    const int r = idx >> 6, c = idx & 63;
    const int64_t gr = i * SPD_NB + r, gc = j * SPD_NB + c;
    // a diagonal tile takes its upper triangle from its lower one
    if (gr < p.n && gc < p.n) p.p[gr * p.ldp + gc] = (i == j && c > r) ? spd_lds[c * SPD_TS + r] : spd_lds[r * SPD_TS + c];
    const int64_t tr = j * SPD_NB + r, tc = i * SPD_NB + c;
    if (i != j && tr < p.n && tc < p.n) p.p[tr * p.ldp + tc] = spd_lds[c * SPD_TS + r];
  }
}

struct SpdLayout {
  double *linv, *panel;
};

static SpdLayout spd_layout(Carver& cv, int64_t n) {
  const int64_t nb = (n + SPD_NB - 1) / SPD_NB;
  SpdLayout y{};
  y.linv = cv.take<double>(nb * SPD_NB * SPD_NB);
  y.panel = cv.take<double>(nb * SPD_NB * SPD_NB);
  return y;
}

// ---------------------------------------------------------------- Gram, weights, score
constexpr int GRAM_THREADS = 512, GRAM_WAVES = GRAM_THREADS / WAVE, GRAM_TILE = 8192, GRAM_MAX_TILE = RSA_EASE_MAX_TILE;

struct GramParams {
  const int64_t *u_indptr, *i_indptr;
  const int32_t *u_items, *i_users;
  int64_t n_users, n_items, ld;
  double lam;
  int32_t tile, n_tiles;
  double* g;
};

__global__ __launch_bounds__(GRAM_THREADS) void ease_gram_kernel(const GramParams p) {
  extern __shared__ uint32_t gram_cnt[];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int64_t i = (int64_t)blockIdx.x / p.n_tiles;
  const int32_t tl = (int32_t)((int64_t)blockIdx.x - i * p.n_tiles);
  const int32_t lo = tl * p.tile;
  const int32_t span = (int32_t)((p.n_items - lo < p.tile) ? p.n_items - lo : p.tile);
  for (int x = t; x < span; x += GRAM_THREADS) gram_cnt[x] = 0u;
  __syncthreads();
  const int64_t is = p.i_indptr[i], ie = p.i_indptr[i + 1];
  for (int64_t k = is + wave; k < ie; k += GRAM_WAVES) {
    const int32_t u = p.i_users[k];
    if ((uint64_t)(uint32_t)u >= (uint64_t)p.n_users) continue;
    int64_t s = p.u_indptr[u];
    const int64_t e = p.u_indptr[u + 1];
    if (p.n_tiles > 1) s = knn_lower_bound(p.u_items, s, e, lo);
    for (int64_t q = s + lane; q < e; q += WAVE) {
      const uint32_t off = (uint32_t)(p.u_items[q] - lo);
      if (off >= (uint32_t)span) break;             // the row is sorted: past the tile
      atomicAdd(&gram_cnt[off], 1u);
    }
  }
  __syncthreads();
  double* row = p.g + i * p.ld + lo;
  for (int x = t; x < span; x += GRAM_THREADS) row[x] = (double)gram_cnt[x] + ((int64_t)lo + x == i ? p.lam : 0.0);
}

constexpr int WT_THREADS = 256, WT_COLS = 64, WT_CHAINS = WT_THREADS / WT_COLS;

// one workgroup per 64 columns: thread (chain g, column c) walks the rows g, g + 4, ... of its column
__global__ __launch_bounds__(WT_THREADS) void ease_weights_kernel(const double* p, double* b, double* terms, int64_t n, int64_t ld,
                                                                  int64_t ldb, double lam) {
  __shared__ double part[WT_CHAINS][WT_COLS];
  const int c = threadIdx.x & (WT_COLS - 1), g = threadIdx.x / WT_COLS;
  const int64_t col = (int64_t)blockIdx.x * WT_COLS + c;
  const bool ok = col < n;
  const double d = ok ? p[col * ld + col] : 1.0;
  __syncthreads();                                  // b may be p: every diagonal of the tile is read before one is overwritten
  double s = 0.0;
  if (ok)
    for (int64_t r = g; r < n; r += WT_CHAINS) {
      const double v = p[r * ld + col];
      s += v * v;
      b[r * ldb + col] = r == col ? 0.0 : -v / d;
    }
  part[g][c] = s;
  __syncthreads();
  if (g == 0 && ok) {
    const double sq = (part[0][c] + part[1][c]) + (part[2][c] + part[3][c]);
    terms[col] = 1.0 / d - lam * sq / (d * d);
  }
}

// loss = sqrt(sum of the terms): thread t sums the terms t, t + 256, ... ascending, then a fixed tree
__global__ __launch_bounds__(WT_THREADS) void ease_loss_kernel(const double* terms, int64_t n, double* loss) {
  __shared__ double red[WT_THREADS];
  double s = 0.0;
  for (int64_t i = threadIdx.x; i < n; i += WT_THREADS) s += terms[i];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int w = WT_THREADS / 2; w >= 1; w >>= 1) {
    if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) loss[0] = sqrt(red[0] > 0.0 ? red[0] : 0.0);
}

constexpr int SC_THREADS = 256, SC_TILE = 2 * SC_THREADS, SC_UNROLL = 4;

struct ScoreParams {
  const int64_t *users, *u_indptr;
  const int32_t* u_items;
  const double* b;
  int64_t n_users, n_items, ld;
  int32_t n_tiles;
  bool vec;
  float* out;
};

// one workgroup per (user, 512 columns of B starting at an even column); thread t owns the columns c0 = 512 tile + 2 t and c0 + 1
__global__ __launch_bounds__(SC_THREADS) void ease_score_kernel(const ScoreParams p) {
  const int64_t bq = (int64_t)blockIdx.x / p.n_tiles;
  const int64_t tl = (int64_t)blockIdx.x - bq * p.n_tiles;
  const int64_t c0 = tl * SC_TILE + 2 * (int64_t)threadIdx.x;
  const bool have0 = c0 < p.n_items, have1 = c0 + 1 < p.n_items;
  const int64_t u = p.users[bq];
  const bool ok = u >= 0 && u < p.n_users;
  const int64_t s = ok ? p.u_indptr[u] : 0, e = ok ? p.u_indptr[u + 1] : 0;
  double a0 = 0.0, a1 = 0.0;
  for (int64_t k = s; k < e; k += SC_UNROLL) {        // stored order: the order of every sum
    double2 v[SC_UNROLL];
#pragma unroll
    for (int q = 0; q < SC_UNROLL; ++q) {
      v[q] = make_double2(0.0, 0.0);
      const int32_t j = k + q < e ? p.u_items[k + q] : -1;
      if ((uint64_t)(uint32_t)j >= (uint64_t)p.n_items) continue;
      const double* src = p.b + (int64_t)j * p.ld + c0;
      if (p.vec && have1) {
        v[q] = *reinterpret_cast<const double2*>(src);
      } else {
        if (have0) v[q].x = src[0];
        if (have1) v[q].y = src[1];
      }
    }
#pragma unroll
    for (int q = 0; q < SC_UNROLL; ++q) a0 += v[q].x, a1 += v[q].y;
  }
  float* row = p.out + bq * (p.n_items - 1);
  if (have0 && c0 >= 1) row[c0 - 1] = (float)a0;       // column 0 is the padding item: no output
  if (have1) row[c0] = (float)a1;
}

static bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace rsa

using namespace rsa;

extern "C" int rsa_ease_gram(const rsa_ease_gram_args* args, rsa_stream_t stream) {
  const char* fn = "rsa_ease_gram";
  rsa_ease_gram_args a;
  if (int rc = load_args(a, args, fn)) return rc;
  if (a.tile == 0) a.tile = GRAM_TILE;
  RSA_CHECK_ARG(a.tile >= 1 && a.tile <= GRAM_MAX_TILE, "%s: tile = %d is outside 1 .. %d", fn, a.tile, GRAM_MAX_TILE);
  RSA_CHECK_ARG(a.n_items >= 1 && a.n_items < (1ll << 31) && a.n_users >= 1 && a.n_users < (1ll << 31) && a.nnz >= 0,
                "%s: n_users = %lld, n_items = %lld, nnz = %lld out of range (n >= 1)", fn, (long long)a.n_users, (long long)a.n_items,
                (long long)a.nnz);
  RSA_CHECK_ARG(a.ld >= a.n_items, "%s: ld = %lld is below n_items = %lld", fn, (long long)a.ld, (long long)a.n_items);
  RSA_CHECK_ARG(std::isfinite(a.lam), "%s: lambda is not finite", fn);
  const int64_t n_tiles = (a.n_items + a.tile - 1) / a.tile;
  RSA_CHECK_ARG(a.n_items * n_tiles < (1ll << 31), "%s: n_items * tiles = %lld workgroups do not fit one launch", fn,
                (long long)(a.n_items * n_tiles));
  RSA_CHECK_ARG(a.u_indptr != nullptr, "%s: u_indptr is null", fn);
  RSA_CHECK_ARG(a.i_indptr != nullptr, "%s: i_indptr is null", fn);
  RSA_CHECK_ARG(a.nnz == 0 || a.u_items != nullptr, "%s: u_items is null", fn);
  RSA_CHECK_ARG(a.nnz == 0 || a.i_users != nullptr, "%s: i_users is null", fn);
  RSA_CHECK_ARG(a.g != nullptr, "%s: g is null", fn);
  GramParams p{};
  p.u_indptr = a.u_indptr, p.i_indptr = a.i_indptr, p.u_items = a.u_items, p.i_users = a.i_users;
  p.n_users = a.n_users, p.n_items = a.n_items, p.ld = a.ld, p.lam = a.lam, p.tile = a.tile, p.n_tiles = (int32_t)n_tiles, p.g = a.g;
  const int64_t lds = (a.n_items < a.tile ? a.n_items : (int64_t)a.tile) * 4;
  if (int rc = allow_lds<ease_gram_kernel>(lds, fn)) return rc;
  hipLaunchKernelGGL(ease_gram_kernel, dim3((unsigned)(a.n_items * n_tiles)), dim3(GRAM_THREADS), (size_t)lds, (hipStream_t)stream, p);
  RSA_CHECK_LAUNCH(fn);
  return RSA_OK;
}

extern "C" int64_t rsa_spd_inverse_f64_workspace_bytes(int64_t n) {
  if (n < 1 || n >= (1ll << 31)) return -1;
  Carver cv(nullptr);
  spd_layout(cv, n);
  return cv.bytes() + 256;
}

extern "C" int rsa_spd_inverse_f64(const rsa_spd_inverse_args* args, rsa_stream_t stream) {
  const char* fn = "rsa_spd_inverse_f64";
  rsa_spd_inverse_args a;
  if (int rc = load_args(a, args, fn)) return rc;
  RSA_CHECK_ARG(a.n >= 1 && a.n < (1ll << 31), "%s: n = %lld is out of range (n >= 1)", fn, (long long)a.n);
  RSA_CHECK_ARG((a.n + SPD_NB - 1) / SPD_NB <= 65535, "%s: n = %lld needs more than 65535 block rows", fn, (long long)a.n);
  RSA_CHECK_ARG(a.ld >= a.n, "%s: ld = %lld is below n = %lld", fn, (long long)a.ld, (long long)a.n);
  RSA_CHECK_ARG(a.ldp >= a.n, "%s: ldp = %lld is below n = %lld", fn, (long long)a.ldp, (long long)a.n);
  RSA_CHECK_ARG(a.a != nullptr, "%s: a is null", fn);
  RSA_CHECK_ARG(a.p != nullptr, "%s: p is null", fn);
  RSA_CHECK_ARG(a.a != a.p, "%s: p must not be a (a holds W while p is written)", fn);
  RSA_CHECK_ARG(a.status != nullptr, "%s: status is null", fn);
  RSA_CHECK_ARG(a.workspace != nullptr, "%s: workspace is null", fn);
  const int64_t need = rsa_spd_inverse_f64_workspace_bytes(a.n);
  RSA_CHECK_ARG(a.workspace_bytes >= need, "%s: the workspace is too small: %lld bytes, need %lld", fn, (long long)a.workspace_bytes,
                (long long)need);
  Carver cv(a.workspace);
  const SpdLayout y = spd_layout(cv, a.n);
  SpdParams p{};
  p.a = a.a, p.p = a.p, p.linv = y.linv, p.panel = y.panel, p.status = a.status, p.n = a.n, p.ld = a.ld, p.ldp = a.ldp;
  p.nb = (int32_t)((a.n + SPD_NB - 1) / SPD_NB), p.npad = (int64_t)p.nb * SPD_NB;
  p.vec = aligned16(a.a) && a.ld % 2 == 0;
  hipStream_t s = (hipStream_t)stream;
  if (int rc = allow_lds<spd_update_kernel>(SPD_GEMM_LDS, fn)) return rc;
  if (int rc = allow_lds<spd_panel_kernel>(SPD_GEMM_LDS, fn)) return rc;
  if (int rc = allow_lds<spd_trow_kernel>(SPD_GEMM_LDS, fn)) return rc;
  if (int rc = allow_lds<spd_wrow_kernel>(SPD_GEMM_LDS, fn)) return rc;
  if (int rc = allow_lds<spd_wtw_kernel>(SPD_GEMM_LDS, fn)) return rc;
  const dim3 block(SPD_THREADS);
  for (int32_t k = 0; k < p.nb; ++k) {               // factor, left-looking
    p.k = k;
    if (k > 0) hipLaunchKernelGGL(spd_update_kernel, dim3((unsigned)(p.nb - k)), block, (size_t)SPD_GEMM_LDS, s, p);
    hipLaunchKernelGGL(spd_diag_kernel, dim3(1), block, 0, s, p);
    if (k + 1 < p.nb) hipLaunchKernelGGL(spd_panel_kernel, dim3((unsigned)(p.nb - k - 1)), block, (size_t)SPD_GEMM_LDS, s, p);
    RSA_CHECK_LAUNCH(fn);
  }
  for (int32_t i = 0; i < p.nb; ++i) {               // W = L^-1 by block rows
    p.k = i;
    if (i > 0) hipLaunchKernelGGL(spd_trow_kernel, dim3((unsigned)i), block, (size_t)SPD_GEMM_LDS, s, p);
    hipLaunchKernelGGL(spd_wrow_kernel, dim3((unsigned)(i + 1)), block, (size_t)SPD_GEMM_LDS, s, p);
    RSA_CHECK_LAUNCH(fn);
  }
  hipLaunchKernelGGL(spd_wtw_kernel, dim3((unsigned)p.nb, (unsigned)p.nb), block, (size_t)SPD_GEMM_LDS, s, p);
  RSA_CHECK_LAUNCH(fn);
  return RSA_OK;
}

extern "C" int rsa_ease_weights(const rsa_ease_weights_args* args, rsa_stream_t stream) {
  const char* fn = "rsa_ease_weights";
  rsa_ease_weights_args a;
  if (int rc = load_args(a, args, fn)) return rc;
  RSA_CHECK_ARG(a.n >= 1 && a.n < (1ll << 31), "%s: n = %lld is out of range (n >= 1)", fn, (long long)a.n);
  RSA_CHECK_ARG(a.ld >= a.n, "%s: ld = %lld is below n = %lld", fn, (long long)a.ld, (long long)a.n);
  RSA_CHECK_ARG(a.ldb >= a.n, "%s: ldb = %lld is below n = %lld", fn, (long long)a.ldb, (long long)a.n);
  RSA_CHECK_ARG(std::isfinite(a.lam), "%s: lambda is not finite", fn);
  RSA_CHECK_ARG(a.p != nullptr, "%s: p is null", fn);
  RSA_CHECK_ARG(a.b != nullptr, "%s: b is null", fn);
  RSA_CHECK_ARG(a.b != a.p || a.ldb == a.ld, "%s: b is p but ldb = %lld is not ld = %lld", fn, (long long)a.ldb, (long long)a.ld);
  RSA_CHECK_ARG(a.terms != nullptr, "%s: terms is null", fn);
  RSA_CHECK_ARG(a.loss != nullptr, "%s: loss is null", fn);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(ease_weights_kernel, dim3((unsigned)((a.n + WT_COLS - 1) / WT_COLS)), dim3(WT_THREADS), 0, s, a.p, a.b, a.terms, a.n,
                     a.ld, a.ldb, a.lam);
  hipLaunchKernelGGL(ease_loss_kernel, dim3(1), dim3(WT_THREADS), 0, s, a.terms, a.n, a.loss);
  RSA_CHECK_LAUNCH(fn);
  return RSA_OK;
}

extern "C" int rsa_ease_score(const rsa_ease_score_args* args, rsa_stream_t stream) {
  const char* fn = "rsa_ease_score";
  rsa_ease_score_args a;
  if (int rc = load_args(a, args, fn)) return rc;
  RSA_CHECK_ARG(a.n_batch >= 0 && a.n_users >= 1 && a.n_users < (1ll << 31) && a.n_items >= 1 && a.n_items < (1ll << 31),
                "%s: n_batch = %lld, n_users = %lld, n_items = %lld out of range (n >= 1)", fn, (long long)a.n_batch, (long long)a.n_users,
                (long long)a.n_items);
  RSA_CHECK_ARG(a.ld >= a.n_items, "%s: ld = %lld is below n_items = %lld", fn, (long long)a.ld, (long long)a.n_items);
  const int64_t n_tiles = (a.n_items + SC_TILE - 1) / SC_TILE;
  RSA_CHECK_ARG(a.n_batch * n_tiles < (1ll << 31), "%s: n_batch * tiles = %lld workgroups do not fit one launch", fn,
                (long long)(a.n_batch * n_tiles));
  RSA_CHECK_ARG(a.users != nullptr, "%s: users is null", fn);
  RSA_CHECK_ARG(a.u_indptr != nullptr, "%s: u_indptr is null", fn);
  RSA_CHECK_ARG(a.b != nullptr, "%s: b is null", fn);
  RSA_CHECK_ARG(a.out != nullptr, "%s: out is null", fn);
  if (a.n_batch == 0 || a.n_items == 1) return RSA_OK;
  ScoreParams p{};
  p.users = a.users, p.u_indptr = a.u_indptr, p.u_items = a.u_items, p.b = a.b, p.n_users = a.n_users, p.n_items = a.n_items, p.ld = a.ld;
  p.n_tiles = (int32_t)n_tiles, p.vec = aligned16(a.b) && a.ld % 2 == 0, p.out = a.out;
  hipLaunchKernelGGL(ease_score_kernel, dim3((unsigned)(a.n_batch * n_tiles)), dim3(SC_THREADS), 0, (hipStream_t)stream, p);
  RSA_CHECK_LAUNCH(fn);
  return RSA_OK;
}
