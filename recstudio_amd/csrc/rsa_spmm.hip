// CSR sparse x dense product with a fused layer-mean epilogue: the propagation of the graph retrievers (gfx950).
//
// rsa_spmm_csr : LightGCNNet.forward, one layer      recstudio/model/module/graphmodule.py:168-198 (mess_norm 'both')
//                SimGCLNet.forward, one layer        recstudio/model/graph/simgcl.py:14-26 (the same with noise: NOISE below)
//
//   y[r, :] = row_scale[r] * sum_e values[e] * x[indices[e], :],   acc_out[r, :] = acc_scale * (acc_in[r, :] + y[r, :])
//
// The product is a row gather with a running sum.  A neighbour row of d floats is d / 4 float4 pieces; G = the power of two
// >= d / 4 lanes read one neighbour row, so a wave-instruction covers 64 / G neighbour rows in whole 16-byte pieces (d = 64:
// 16 lanes x float4 = one 256-byte row, 4 neighbours per load; columns past d / 4 of a group idle).  A wave takes 64 edges at a
// time: lane l reads indices[b + l] and values[b + l] (two coalesced, nontemporal loads), and step t hands edge t * (64 / G) +
// slot to the lane group `slot` by a wave shuffle.  SPMM_UNROLL steps are issued before their products are added, so a wave
// keeps that many row loads in flight.
//
// ORDER.  Slot j of a wave adds the edges j, j + 64 / G, j + 2 * 64 / G, ... of its range in ascending order, each product
// rounded once, each addition rounded once (-ffp-contract=off); the slots are then added pairwise, nearest first (xor G, 2 G,
// ... 32).  Padding lanes add exact zeros.  A row of K edges therefore goes through a summation tree with K - 1 rounded additions
// and K rounded products: |sum - exact| <= gamma(K) * sum |v_e x|, whatever the tree (tests/spmm_referee.py).
//
// SKEW.  Degrees follow a power law (items with 1e4 - 1e5 neighbours against a user median of tens); a wave per row runs as long
// as its longest row.  Rows longer than the plan's chunk are cut into pieces of `chunk` edges (include/recstudio_amd.h, "THE
// PLAN"): piece p is one wave's work like any short row and lands in partials[p, :] unscaled; spmm_finish_kernel adds a split
// row's partials in ascending p -- a fixed order -- and applies row_scale and the accumulation.  The pieces are the FIRST work
// items of the gather launch, so the long rows start before the short ones.  No atomics anywhere.
//
// Every index read from memory is clamped into its array before it is followed (indptr into [0, nnz], indices into [0, n_cols),
// plan rows into [0, n_rows), plan pieces into [0, n_parts]).
//
// NOISE (SimGCLNet.forward, recstudio/model/graph/simgcl.py:14-26; include/recstudio_amd.h, "THE PERTURBED FORM").  With
// noise_eps != 0 the launches are OTHER kernels (spmm_gather_noise_kernel<LG>, spmm_finish_noise_kernel) around the same
// wave_gather_sum; the plain path runs the kernels it ran before, with the kernel arguments it had.  The row's sum after
// row_scale sits in the float4 of the d / 4 writer lanes; before store_row writes it, finish_row_noise adds sgn(s_c) * (u_c / q) * eps (the moves: row_moves),
// q = max(||u||_2, 1e-12):
//   * DRAWS.  u_c is element r * d + c of one torch.rand call (torch_rand_element): a ten-round Philox evaluation per element,
//     three of its four words unused.  The d draws of a row are spread over the wave's 64 lanes -- lane l draws the columns
//     l, l + 64, l + 128, l + 192 below d, so d <= 64 costs ONE evaluation of wave time, d = 256 four -- and handed to the
//     writer lanes by shuffles (writer w takes columns 4 w .. 4 w + 3).  The other form, every writer lane drawing its own four
//     columns (4 evaluations of wave time at any d, on d / 4 lanes), was not built.  The same lanes write noise_u, coalesced.
//     The moves of a row need no sum, so the gather launch computes them BEFORE its gather loop, where the Philox rounds run
//     under the loads of the other waves instead of after the wave's last load: 4.31 ms against 4.39 ms per layer at d = 64,
//     7.89 against 7.91 at d = 128, alternating processes on one device.
//   * ORDER OF sum u^2.  Lane l adds the squares of its columns in ascending order onto +0 (each square rounded once, each
//     addition rounded once; a lane without a column keeps +0); the 64 lane sums are added by the xor butterfly 1, 2, 4, 8,
//     16, 32, which gives every lane the same bits.  sqrt and the division are the correctly rounded ones.
//   * SPLIT ROWS get the perturbation once, on the row's total: spmm_finish_noise_kernel gives a split row a WAVE, not d / 4
//     threads -- lane w < d / 4 adds column w of the row's partials in ascending piece order exactly as spmm_finish_kernel
//     does, then the wave runs the same row_moves: the row norm is reduced across the wave's lanes, not recomputed per
//     thread, and a row's uniforms, q and perturbation are by construction those it would get unsplit.
#include "rsa_internal.hpp"

namespace rsa {

constexpr int SPMM_MAX_DIM = 256;
constexpr int SPMM_UNROLL = 4;          // row loads a wave issues before it adds their products

struct SpmmParams {
  const int64_t* indptr;
  const int32_t* indices;
  const float* values;
  int64_t n_rows, n_cols, nnz;
  int dim, d4;                          // d4 = dim / 4: float4 pieces per row
  const float* x;
  const float* row_scale;
  float* y;
  const float* acc_in;
  float* acc_out;
  float acc_scale;
  int64_t chunk, n_split, n_parts;
  const int64_t *split_row, *split_part, *part_row, *part_edge;
  float* partials;
};

__device__ __forceinline__ int64_t clamp64(int64_t v, int64_t lo, int64_t hi) { return v < lo ? lo : (v > hi ? hi : v); }

__device__ __forceinline__ void add_scaled(float4& acc, float v, const float4& x) {
  acc.x += v * x.x;
  acc.y += v * x.y;
  acc.z += v * x.z;
  acc.w += v * x.w;
}

// sum_e values[e] * x[indices[e], 4 col .. 4 col + 3] over e in [s, e): every lane of column `col` gets the total
template <int LG>
__device__ __forceinline__ float4 wave_gather_sum(const SpmmParams& p, int64_t s, int64_t e, int lane) {
  constexpr int G = 1 << LG, NB = 64 >> LG;
  const int slot = lane >> LG, col = lane & (G - 1);
  const bool col_ok = col < p.d4;
  // (a lane without a piece or without an edge still loads -- column 0 of a row that exists -- and drops what it read: a
  // predicated load would make the compiler wait for every load before it issues the next)
  const float* xc = p.x + (col_ok ? col : 0) * 4;
  const int32_t last_col = (int32_t)(p.n_cols - 1);
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int64_t b = s; b < e; b += 64) {
    const int cnt = (int)(e - b < 64 ? e - b : 64);
    int32_t idx = 0;
    float val = 0.f;
    if (lane < cnt) {
      idx = __builtin_nontemporal_load(p.indices + b + lane);
      val = p.values ? __builtin_nontemporal_load(p.values + b + lane) : 1.f;
      idx = idx < 0 ? 0 : (idx > last_col ? last_col : idx);
    }
    const int steps = (cnt + NB - 1) >> (6 - LG);
    for (int t = 0; t < steps; t += SPMM_UNROLL) {
      float4 xr[SPMM_UNROLL];
      float v[SPMM_UNROLL];
      bool ok[SPMM_UNROLL];
#pragma unroll
      for (int u = 0; u < SPMM_UNROLL; ++u) {
        const int src = (t + u) * NB + slot;
        const int32_t j = __shfl(idx, src & 63, 64);              // (idx is 0 on the lanes past cnt: row 0 exists)
        v[u] = __shfl(val, src & 63, 64);
        ok[u] = col_ok && src < cnt;
        xr[u] = *reinterpret_cast<const float4*>(xc + (int64_t)j * p.dim);
      }
#pragma unroll
      for (int u = 0; u < SPMM_UNROLL; ++u) {
        if (!ok[u]) {                                             // adds an exact zero (0 * inf of a row nobody asked for stays out)
          v[u] = 0.f;
          xr[u] = make_float4(0.f, 0.f, 0.f, 0.f);
        }
        add_scaled(acc, v[u], xr[u]);
      }
    }
  }
#pragma unroll
  for (int m = G; m < 64; m <<= 1) {
    acc.x += __shfl_xor(acc.x, m, 64);
    acc.y += __shfl_xor(acc.y, m, 64);
    acc.z += __shfl_xor(acc.z, m, 64);
    acc.w += __shfl_xor(acc.w, m, 64);
  }
  return acc;
}

__device__ __forceinline__ float4 scale_row(const SpmmParams& p, int64_t r, float4 sum) {
  if (p.row_scale) {
    const float sc = p.row_scale[r];
    sum = make_float4(sc * sum.x, sc * sum.y, sc * sum.z, sc * sum.w);
  }
  return sum;
}

// row r, columns 4 col .. 4 col + 3: y and the accumulation from the row's scaled sum
__device__ __forceinline__ void store_row(const SpmmParams& p, int64_t r, int col, float4 sum) {
  const int64_t at = r * p.dim + col * 4;
  if (p.y) *reinterpret_cast<float4*>(p.y + at) = sum;
  if (p.acc_out) {
    const float4 a = *reinterpret_cast<const float4*>(p.acc_in + at);
    const float k = p.acc_scale;
    *reinterpret_cast<float4*>(p.acc_out + at) = make_float4(k * (a.x + sum.x), k * (a.y + sum.y), k * (a.z + sum.z), k * (a.w + sum.w));
  }
}

// row r, columns 4 col .. 4 col + 3: row_scale, y and the accumulation from the row's unscaled sum
__device__ __forceinline__ void finish_row(const SpmmParams& p, int64_t r, int col, float4 sum) {
  store_row(p, r, col, scale_row(p, r, sum));
}

struct SpmmNoise {
  float eps;
  PhiloxCall pc;
  float* u;                             // nullable [n_rows, dim]
};

// The whole wave: the moves of row r, (u_c / q) * eps for the columns 4 lane .. 4 lane + 3 (file header, NOISE).  Needs no sum.
__device__ __forceinline__ float4 row_moves(const SpmmParams& p, const SpmmNoise& nz, int64_t r, int lane) {
  const uint64_t base = (uint64_t)r * (uint64_t)p.dim;
  float u[4], sq = 0.f;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int c = lane + 64 * k;
    u[k] = 0.f;
    if (k * 64 < p.dim) {                                         // (uniform over the wave)
      if (c < p.dim) {
        u[k] = torch_rand_element(nz.pc, base + (uint64_t)c);
        if (nz.u) nz.u[base + c] = u[k];
      }
      sq += u[k] * u[k];
    }
  }
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) sq += __shfl_xor(sq, m, 64);
  const float q = fmaxf(sqrtf(sq), 1e-12f);
  float un[4];                                                    // the uniforms of columns 4 lane .. 4 lane + 3
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int c = (4 * lane + j) & (SPMM_MAX_DIM - 1);            // (lanes >= d4 fetch something and drop it)
    un[j] = __shfl(u[0], c & 63, 64);
#pragma unroll
    for (int k = 1; k < 4; ++k) {
      if (k * 64 < p.dim) {
        const float v = __shfl(u[k], c & 63, 64);
        if ((c >> 6) == k) un[j] = v;
      }
    }
  }
  return make_float4((un[0] / q) * nz.eps, (un[1] / q) * nz.eps, (un[2] / q) * nz.eps, (un[3] / q) * nz.eps);
}

// s + sgn(s) * t, sgn = torch.sign: a zero stays where it is
__device__ __forceinline__ float moved(float s, float t) { return s + (s > 0.f ? t : (s < 0.f ? -t : 0.f)); }

// finish_row on the perturbed row: row_scale, the move by `mv` (row_moves), y and the accumulation
__device__ __forceinline__ void finish_row_noise(const SpmmParams& p, int64_t r, int col, float4 sum, const float4& mv) {
  sum = scale_row(p, r, sum);
  store_row(p, r, col, make_float4(moved(sum.x, mv.x), moved(sum.y, mv.y), moved(sum.z, mv.z), moved(sum.w, mv.w)));
}

// One wave per work item; items [0, n_parts) are the pieces of the split rows, items n_parts + r the rows.
template <int LG>
__global__ __launch_bounds__(256) void spmm_gather_kernel(const SpmmParams p) {
  const int lane = lane_id();
  const int64_t item = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (item >= p.n_parts + p.n_rows) return;
  const bool writer = lane < (1 << LG) && lane < p.d4;          // slot 0 holds the row
  if (item < p.n_parts) {
    const int64_t r = clamp64(p.part_row[item], 0, p.n_rows - 1);
    const int64_t row_end = clamp64(p.indptr[r + 1], 0, p.nnz);
    const int64_t s = clamp64(p.part_edge[item], 0, row_end);
    const int64_t e = row_end - s < p.chunk ? row_end : s + p.chunk;
    const float4 sum = wave_gather_sum<LG>(p, s, e, lane);
    if (writer) *reinterpret_cast<float4*>(p.partials + item * p.dim + lane * 4) = sum;
    return;
  }
  const int64_t r = item - p.n_parts;
  const int64_t s = clamp64(p.indptr[r], 0, p.nnz);
  const int64_t e = clamp64(p.indptr[r + 1], s, p.nnz);
  if (e - s > p.chunk) return;                                    // a split row: its pieces above, its sum below
  const float4 sum = wave_gather_sum<LG>(p, s, e, lane);
  if (writer) finish_row(p, r, lane, sum);
}

// One thread per (split row, float4 column): the row's partials added in ascending piece order, SPMM_UNROLL loads in flight.
__global__ __launch_bounds__(256) void spmm_finish_kernel(const SpmmParams p) {
  const int64_t tid = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t s = tid / p.d4;
  if (s >= p.n_split) return;
  const int col = (int)(tid - s * p.d4);
  const int64_t p0 = clamp64(p.split_part[s], 0, p.n_parts);
  const int64_t p1 = clamp64(p.split_part[s + 1], p0, p.n_parts);
  const float* part = p.partials + col * 4;
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int64_t q = p0; q < p1; q += SPMM_UNROLL) {
    float4 v[SPMM_UNROLL];
#pragma unroll
    for (int u = 0; u < SPMM_UNROLL; ++u) v[u] = *reinterpret_cast<const float4*>(part + (q + u < p1 ? q + u : p1 - 1) * p.dim);
#pragma unroll
    for (int u = 0; u < SPMM_UNROLL; ++u) {
      if (q + u >= p1) v[u] = make_float4(0.f, 0.f, 0.f, 0.f);
      add_scaled(acc, 1.f, v[u]);
    }
  }
  finish_row(p, clamp64(p.split_row[s], 0, p.n_rows - 1), col, acc);
}

// The perturbed form of the gather kernel: the same work items, the same sums, row_moves and finish_row_noise in place of finish_row.
template <int LG>
__global__ __launch_bounds__(256) void spmm_gather_noise_kernel(const SpmmParams p, const SpmmNoise nz) {
  const int lane = lane_id();
  const int64_t item = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (item >= p.n_parts + p.n_rows) return;
  const bool writer = lane < (1 << LG) && lane < p.d4;
  if (item < p.n_parts) {
    const int64_t r = clamp64(p.part_row[item], 0, p.n_rows - 1);
    const int64_t row_end = clamp64(p.indptr[r + 1], 0, p.nnz);
    const int64_t s = clamp64(p.part_edge[item], 0, row_end);
    const int64_t e = row_end - s < p.chunk ? row_end : s + p.chunk;
    const float4 sum = wave_gather_sum<LG>(p, s, e, lane);
    if (writer) *reinterpret_cast<float4*>(p.partials + item * p.dim + lane * 4) = sum;
    return;
  }
  const int64_t r = item - p.n_parts;
  const int64_t s = clamp64(p.indptr[r], 0, p.nnz);
  const int64_t e = clamp64(p.indptr[r + 1], s, p.nnz);
  if (e - s > p.chunk) return;
  const float4 mv = row_moves(p, nz, r, lane);                    // (before the gather: measured against after it, file header)
  const float4 sum = wave_gather_sum<LG>(p, s, e, lane);
  if (writer) finish_row_noise(p, r, lane, sum, mv);
}

// One WAVE per split row: lane w < d4 adds column w of the row's partials in ascending piece order (the additions of
// spmm_finish_kernel), then the wave perturbs the total.
__global__ __launch_bounds__(256) void spmm_finish_noise_kernel(const SpmmParams p, const SpmmNoise nz) {
  const int lane = lane_id();
  const int64_t s = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (s >= p.n_split) return;
  const bool writer = lane < p.d4;
  const int64_t p0 = clamp64(p.split_part[s], 0, p.n_parts);
  const int64_t p1 = clamp64(p.split_part[s + 1], p0, p.n_parts);
  const float* part = p.partials + (writer ? lane : 0) * 4;
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int64_t q = p0; q < p1; q += SPMM_UNROLL) {
    float4 v[SPMM_UNROLL];
#pragma unroll
    for (int u = 0; u < SPMM_UNROLL; ++u) v[u] = *reinterpret_cast<const float4*>(part + (q + u < p1 ? q + u : p1 - 1) * p.dim);
#pragma unroll
    for (int u = 0; u < SPMM_UNROLL; ++u) {
      if (q + u >= p1) v[u] = make_float4(0.f, 0.f, 0.f, 0.f);
      add_scaled(acc, 1.f, v[u]);
    }
  }
  const int64_t r = clamp64(p.split_row[s], 0, p.n_rows - 1);
  const float4 mv = row_moves(p, nz, r, lane);
  if (writer) finish_row_noise(p, r, lane, acc, mv);
}

}  // namespace rsa

using namespace rsa;

extern "C" int rsa_spmm_csr(const rsa_spmm_args* args, rsa_stream_t stream) {
  const char* fn = "rsa_spmm_csr";
  rsa_spmm_args a;
  if (int rc = load_args(a, args, fn)) return rc;
  RSA_CHECK_ARG(a.dim >= 4 && a.dim <= SPMM_MAX_DIM && a.dim % 4 == 0, "%s: dim must be a multiple of 4 in [4, %d], got %d", fn,
                SPMM_MAX_DIM, a.dim);
  RSA_CHECK_ARG(a.n_rows >= 0 && a.n_cols >= 0 && a.nnz >= 0, "%s: negative size (n_rows %lld, n_cols %lld, nnz %lld)", fn,
                (long long)a.n_rows, (long long)a.n_cols, (long long)a.nnz);
  RSA_CHECK_ARG(a.n_cols < (1ll << 31), "%s: n_cols must fit the int32 column indices", fn);
  RSA_CHECK_ARG(a.nnz == 0 || a.n_cols >= 1, "%s: edges into an empty x", fn);
  RSA_CHECK_ARG(a.chunk >= 1, "%s: the plan's chunk must be at least 1, got %lld", fn, (long long)a.chunk);
  RSA_CHECK_ARG(a.n_split >= 0 && a.n_split <= a.n_rows && a.n_parts >= 0 && a.n_parts <= a.nnz && a.n_parts >= 2 * a.n_split,
                "%s: a plan of %lld pieces for %lld split rows cannot belong to a matrix of %lld rows and %lld edges", fn,
                (long long)a.n_parts, (long long)a.n_split, (long long)a.n_rows, (long long)a.nnz);
  RSA_CHECK_ARG(a.n_split == 0 || a.plan != nullptr, "%s: plan is null", fn);
  RSA_CHECK_ARG(a.n_split == 0 || a.plan_len >= 2 * a.n_split + 1 + 2 * a.n_parts,
                "%s: the plan is too small: %lld entries, %lld split rows and %lld pieces need %lld", fn, (long long)a.plan_len,
                (long long)a.n_split, (long long)a.n_parts, (long long)(2 * a.n_split + 1 + 2 * a.n_parts));
  RSA_CHECK_ARG(a.n_parts == 0 || a.partials != nullptr, "%s: partials is null", fn);
  RSA_CHECK_ARG(a.partials_bytes >= a.n_parts * a.dim * 4, "%s: the partials workspace is too small: %lld bytes, %lld pieces need %lld",
                fn, (long long)a.partials_bytes, (long long)a.n_parts, (long long)(a.n_parts * a.dim * 4));
  RSA_CHECK_ARG(std::isfinite(a.noise_eps), "%s: noise_eps must be finite", fn);
  const bool noise = a.noise_eps != 0.f;
  RSA_CHECK_ARG(!noise || (a.noise_grid_threads > 0 && a.noise_grid_threads % 256 == 0 && (a.noise_offset & 3) == 0),
                "%s: bad philox state for the noise (grid_threads %u must be a positive multiple of 256, offset a multiple of 4)", fn,
                a.noise_grid_threads);
  RSA_CHECK_ARG(noise || a.noise_u == nullptr, "%s: noise_u without noise_eps", fn);
  RSA_CHECK_ARG(((uintptr_t)a.noise_u & 15) == 0, "%s: noise_u must be 16-byte aligned", fn);
  RSA_CHECK_ARG(a.y != nullptr || a.acc_out != nullptr, "%s: y and acc_out are both null", fn);
  RSA_CHECK_ARG(a.acc_out == nullptr || a.acc_in != nullptr, "%s: acc_out without acc_in", fn);
  if (a.n_rows == 0) return RSA_OK;
  RSA_CHECK_ARG(a.indptr != nullptr, "%s: indptr is null", fn);
  RSA_CHECK_ARG(a.nnz == 0 || (a.indices != nullptr && a.x != nullptr), "%s: indices/x is null", fn);
  RSA_CHECK_ARG((((uintptr_t)a.x | (uintptr_t)a.y | (uintptr_t)a.acc_in | (uintptr_t)a.acc_out | (uintptr_t)a.partials) & 15) == 0,
                "%s: x, y, acc_in, acc_out and partials must be 16-byte aligned", fn);
  RSA_CHECK_ARG((a.n_parts + a.n_rows + 3) / 4 < (1ll << 31), "%s: too many rows for one launch", fn);
  SpmmParams p{};
  p.indptr = a.indptr, p.indices = a.indices, p.values = a.values;
  p.n_rows = a.n_rows, p.n_cols = a.n_cols, p.nnz = a.nnz;
  p.dim = a.dim, p.d4 = a.dim / 4;
  p.x = a.x, p.row_scale = a.row_scale, p.y = a.y, p.acc_in = a.acc_in, p.acc_out = a.acc_out, p.acc_scale = a.acc_scale;
  p.chunk = a.chunk, p.n_split = a.n_split, p.n_parts = a.n_split ? a.n_parts : 0;
  if (a.n_split) {
    p.split_row = a.plan;
    p.split_part = a.plan + a.n_split;
    p.part_row = a.plan + 2 * a.n_split + 1;
    p.part_edge = p.part_row + a.n_parts;
  }
  p.partials = a.partials;
  int lg = 0;                                                    // lanes per neighbour row: the power of two >= dim / 4
  while ((1 << lg) < p.d4) ++lg;
  const unsigned blocks = (unsigned)((p.n_parts + p.n_rows + 3) / 4);
  if (noise) {
    const SpmmNoise nz{a.noise_eps, PhiloxCall{a.noise_seed, a.noise_offset >> 2, a.noise_grid_threads, a.noise_elem_base}, a.noise_u};
    dispatch_int<0, 1, 2, 3, 4, 5, 6>(lg, [&](auto LG) {
      hipLaunchKernelGGL((spmm_gather_noise_kernel<LG()>), dim3(blocks), dim3(256), 0, (hipStream_t)stream, p, nz);
    });
    RSA_CHECK_LAUNCH(fn);
    if (p.n_split) {
      hipLaunchKernelGGL(spmm_finish_noise_kernel, dim3((unsigned)((p.n_split + 3) / 4)), dim3(256), 0, (hipStream_t)stream, p, nz);
      RSA_CHECK_LAUNCH(fn);
    }
    return RSA_OK;
  }
  dispatch_int<0, 1, 2, 3, 4, 5, 6>(lg, [&](auto LG) {
    hipLaunchKernelGGL((spmm_gather_kernel<LG()>), dim3(blocks), dim3(256), 0, (hipStream_t)stream, p);
  });
  RSA_CHECK_LAUNCH(fn);
  if (p.n_split) {
    const int64_t threads = p.n_split * p.d4;
    hipLaunchKernelGGL(spmm_finish_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, (hipStream_t)stream, p);
    RSA_CHECK_LAUNCH(fn);
  }
  return RSA_OK;
}
