// CSR sparse x dense product with a fused layer-mean epilogue: the propagation of the graph retrievers (gfx950).
//
// rsa_spmm_csr : LightGCNNet.forward, one layer      recstudio/model/module/graphmodule.py:168-198 (mess_norm 'both')
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

// row r, columns 4 col .. 4 col + 3: row_scale, y and the accumulation from the row's unscaled sum
__device__ __forceinline__ void finish_row(const SpmmParams& p, int64_t r, int col, float4 sum) {
  if (p.row_scale) {
    const float sc = p.row_scale[r];
    sum = make_float4(sc * sum.x, sc * sum.y, sc * sum.z, sc * sum.w);
  }
  const int64_t at = r * p.dim + col * 4;
  if (p.y) *reinterpret_cast<float4*>(p.y + at) = sum;
  if (p.acc_out) {
    const float4 a = *reinterpret_cast<const float4*>(p.acc_in + at);
    const float k = p.acc_scale;
    *reinterpret_cast<float4*>(p.acc_out + at) = make_float4(k * (a.x + sum.x), k * (a.y + sum.y), k * (a.z + sum.z), k * (a.w + sum.w));
  }
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
