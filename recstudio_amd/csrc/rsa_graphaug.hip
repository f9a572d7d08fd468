// Per-step graph augmentation of the self-supervised graph retrievers (gfx950): thin a symmetric CSR and renormalise it.
//
// rsa_graph_dropout : EdgeDropout / NodeDropout       recstudio/model/module/data_augmentation.py:229-304 (the dgl branch)
//                     + GraphConv(norm = 'both')      recstudio/model/module/graphmodule.py:176-188 on the thinned graph
//
//   keep[e]     = floor(u_e + keep_prob) != 0  &&  !node_drop[row(e)]  &&  !node_drop[indices[e]]      u = torch.rand(nnz)
//   in_deg[r]   = #{e in row r : keep[e]}                 out_deg[r] = #{e in row r : keep[rev[e]]}
//   values[e]   = keep[e]      ? (float)(f(out_deg[indices[e]]) * f(in_deg[r]))  : 0     f(k) = 1.0 / sqrt((double)k)
//   t_values[e] = keep[rev[e]] ? (float)(f(out_deg[r]) * f(in_deg[indices[e]]))  : 0     ( = values[rev[e]] )
//
// WHY NOTHING IS GATHERED BUT TWO DEGREES.  keep[e] is a function of e's own uniform and of the flags of its two end nodes; the
// reverse edge rev[e] joins the same two nodes, so keep[rev[e]] is recomputed from element rev[e] of the Philox stream (a few
// hundred integer instructions) instead of being read back from a byte array at a random address.  out_deg[c], the number of kept
// edges LEAVING c, is then a sum over c's own row (the base structure is symmetric), and values[rev[e]] is the same double
// product with the roles of the two ends exchanged: both outputs of an edge come from what its row's wave already holds plus
// in_deg / out_deg of the other end (two 4-byte gathers from tables that stay in cache).
//
// Half of the time of a first version went into the Philox rounds (32-bit multiplies at a quarter of the rate): four draws per
// edge, two in each launch.  The first launch now parks its two decisions in values[e] (two bits of the word the second launch
// overwrites with the weight), which halves them for 8 more bytes of traffic per edge.
//
// WORK ITEMS.  One wave per item, two launches over the same items (counts, then values):
//   items [0, n_rows)         row r, when it has at most `long_row` edges: the wave walks the row 64 edges at a time, counts with
//                             ballots and STORES the two degrees -- no atomic;
//   items n_rows + w          the window [w * long_row, (w + 1) * long_row) of the edge array: the wave finds the first row that
//                             reaches into it (binary search over indptr), then looks at 64 rows at a time and takes the part of
//                             every LONG row inside its window.  A long row of K edges meets at most floor((K - 2) / long_row) + 2
//                             windows and gets one integer atomic per counter from each: with long_row >= 128 and K > long_row
//                             that is at most ceil(K / 64) (at 64 a row of 66 edges could meet three windows: hence the 128).
//                             Integer sums do not depend on their order, so two runs are bit-equal.
// The degrees are zeroed by a memset on the stream ahead of the first launch; nothing is allocated, nothing synchronises.
//
// Every index read from memory is clamped into its array before it is followed (indptr into [0, nnz], indices into [0, n_rows),
// rev into [0, nnz)).  Edge offsets are 64-bit.
#include "rsa_internal.hpp"

namespace rsa {

constexpr int64_t GD_LONG_ROW = 2048;      // default length above which a row is shared between windows

struct GraphDropParams {
  const int64_t* indptr;
  const int32_t* indices;
  const int64_t* rev;
  const uint8_t* node_drop;
  int64_t n_rows, nnz, long_row, n_windows;
  float keep_prob;
  bool draw;                               // keep_prob < 1: the uniforms are consumed
  PhiloxCall pc;
  uint8_t* keep;
  int32_t *in_deg, *out_deg;
  float *values, *t_values;
};

__device__ __forceinline__ int64_t gd_clamp(int64_t v, int64_t lo, int64_t hi) { return v < lo ? lo : (v > hi ? hi : v); }

// philox4x32_10 (rsa_common.hpp) with each round's two 32 x 32 products taken as ONE 64-bit multiply each: the high and the low
// word come out of the same quarter-rate instruction, 20 of them per draw instead of 40.  The same words bit for bit.
__device__ __forceinline__ uint4 gd_philox(uint4 c, uint2 k) {
  constexpr uint64_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u;
  constexpr uint32_t W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = M0 * c.x, p1 = M1 * c.z;
    c = make_uint4((uint32_t)(p1 >> 32) ^ c.y ^ k.x, (uint32_t)p1, (uint32_t)(p0 >> 32) ^ c.w ^ k.y, (uint32_t)p0);
    k.x += W0;
    k.y += W1;
  }
  return c;
}

// == torch_rand_element (rsa_common.hpp): element li of torch.rand(nnz), on gd_philox
__device__ __forceinline__ float gd_uniform(const PhiloxCall& pc, uint64_t li) {
  li += pc.elem_base;
  const uint64_t j = li < pc.grid_threads ? 0 : ((li >> 32) == 0 ? (uint32_t)li / pc.grid_threads : li / pc.grid_threads);
  const uint64_t idx = li - j * pc.grid_threads, ctr = pc.offset4 + (j >> 2);
  const uint4 v = gd_philox(make_uint4((uint32_t)ctr, (uint32_t)(ctr >> 32), (uint32_t)idx, (uint32_t)(idx >> 32)),
                            make_uint2((uint32_t)pc.seed, (uint32_t)(pc.seed >> 32)));
  const float inv = 2.3283064e-10f;                                          // 2^-32
  const float u = __fmaf_rn((float)pick(v, (int)(j & 3)), inv, inv);
  return u == 1.0f ? 0.0f : u;
}

// the draw of edge e alone (the node flags are the caller's)
__device__ __forceinline__ bool gd_drawn(const GraphDropParams& p, int64_t e) {
  if (!p.draw) return true;
  const float t = gd_uniform(p.pc, (uint64_t)e) + p.keep_prob;               // one fp32 addition, as the reference's
  return floorf(t) != 0.f;
}

__device__ __forceinline__ double gd_norm(int32_t k) { return 1.0 / sqrt((double)k); }

// edges [s, e) of row r.  PASS 0: the two counts, stored when `whole` (the wave has the whole row), else added atomically.
// PASS 1: values and t_values.
template <int PASS>
__device__ __forceinline__ void gd_row_range(const GraphDropParams& p, int64_t r, int64_t s, int64_t e, bool whole, int lane) {
  const bool row_ok = !(p.node_drop && p.node_drop[r]);
  const int32_t last = (int32_t)(p.n_rows - 1);
  int32_t n_in = 0, n_out = 0;
  double fin_r = 0.0, fout_r = 0.0;
  if (PASS == 1) {
    fin_r = gd_norm(p.in_deg[r]);          // (inf for a row without kept edges: then no edge below selects it)
    fout_r = gd_norm(p.out_deg[r]);
  }
  for (int64_t b = s; b < e; b += 64) {
    const int64_t at = b + lane;
    const bool have = at < e;
    if (PASS == 0) {
      bool k_in = false, k_out = false;
      if (have) {
        int32_t c = __builtin_nontemporal_load(p.indices + at);
        c = c < 0 ? 0 : (c > last ? last : c);
        const int64_t rv = gd_clamp(__builtin_nontemporal_load(p.rev + at), 0, p.nnz - 1);
        const bool ends_ok = row_ok && !(p.node_drop && p.node_drop[c]);
        k_in = ends_ok && gd_drawn(p, at);
        k_out = ends_ok && gd_drawn(p, rv);
        if (p.keep) p.keep[at] = k_in ? 1 : 0;
        p.values[at] = __int_as_float((k_in ? 1 : 0) | (k_out ? 2 : 0));     // the two draws, parked for pass 1
      }
      n_in += __popcll(__ballot(k_in));
      n_out += __popcll(__ballot(k_out));
    } else if (have) {
      int32_t c = __builtin_nontemporal_load(p.indices + at);
      c = c < 0 ? 0 : (c > last ? last : c);
      const int drawn = __float_as_int(p.values[at]);
      const bool k_in = drawn & 1, k_out = drawn & 2;
      float v = 0.f, tv = 0.f;
      if (k_in) v = (float)(gd_norm(p.out_deg[c]) * fin_r);
      if (k_out) tv = (float)(fout_r * gd_norm(p.in_deg[c]));
      p.values[at] = v;
      if (p.t_values) p.t_values[at] = tv;
    }
  }
  if (PASS == 0 && lane == 0) {
    if (whole) {
      p.in_deg[r] = n_in;
      p.out_deg[r] = n_out;
    } else {
      if (n_in) atomicAdd(p.in_deg + r, n_in);
      if (n_out) atomicAdd(p.out_deg + r, n_out);
    }
  }
}

template <int PASS>
__global__ __launch_bounds__(256) void graph_dropout_kernel(const GraphDropParams p) {
  const int lane = lane_id();
  const int64_t item = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (item >= p.n_rows + p.n_windows) return;
  if (item < p.n_rows) {
    const int64_t s = gd_clamp(p.indptr[item], 0, p.nnz);
    const int64_t e = gd_clamp(p.indptr[item + 1], s, p.nnz);
    if (e - s > p.long_row) return;                                 // a long row: the windows take it
    gd_row_range<PASS>(p, item, s, e, true, lane);
    return;
  }
  const int64_t wb = (item - p.n_rows) * p.long_row;
  const int64_t we = wb + p.long_row < p.nnz ? wb + p.long_row : p.nnz;
  // the last row whose first edge is not behind wb (rows before it end at or before wb when indptr ascends)
  int64_t lo = 0, hi = p.n_rows;
  while (hi - lo > 1) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (gd_clamp(p.indptr[mid], 0, p.nnz) <= wb) lo = mid; else hi = mid;
  }
  for (int64_t r0 = lo; r0 < p.n_rows; r0 += 64) {
    const int64_t r = r0 + lane;
    int64_t s = 0, e = 0;
    bool behind = true;                                             // rows past the matrix or past the window end the walk
    if (r < p.n_rows) {
      s = gd_clamp(p.indptr[r], 0, p.nnz);
      e = gd_clamp(p.indptr[r + 1], s, p.nnz);
      behind = s >= we;
    }
    const bool mine = !behind && e - s > p.long_row && e > wb;
    unsigned long long todo = __ballot(mine);
    while (todo) {
      const int j = __ffsll(todo) - 1;
      todo &= todo - 1;
      const int64_t sj = __shfl(s, j, 64), ej = __shfl(e, j, 64);
      gd_row_range<PASS>(p, r0 + j, sj > wb ? sj : wb, ej < we ? ej : we, false, lane);
    }
    if (__ballot(behind)) break;
  }
}

}  // namespace rsa

using namespace rsa;

extern "C" int rsa_graph_dropout(const rsa_graph_dropout_args* args, rsa_stream_t stream) {
  const char* fn = "rsa_graph_dropout";
  rsa_graph_dropout_args a;
  if (int rc = load_args(a, args, fn)) return rc;
  RSA_CHECK_ARG(a.n_rows >= 0 && a.nnz >= 0, "%s: negative size (n_rows %lld, nnz %lld)", fn, (long long)a.n_rows, (long long)a.nnz);
  RSA_CHECK_ARG(a.n_rows < (1ll << 31), "%s: n_rows must fit the int32 column indices", fn);
  RSA_CHECK_ARG(a.keep_prob >= 0.f && a.keep_prob <= 1.f, "%s: keep_prob must lie in [0, 1], got %g", fn, (double)a.keep_prob);
  RSA_CHECK_ARG(a.long_row == 0 || a.long_row >= 128, "%s: long_row must be at least 128 (0: the default), got %lld", fn,
                (long long)a.long_row);
  RSA_CHECK_ARG(a.nnz == 0 || a.n_rows >= 1, "%s: edges without rows", fn);
  if (a.n_rows == 0) return RSA_OK;
  RSA_CHECK_ARG(a.indptr != nullptr, "%s: indptr is null", fn);
  RSA_CHECK_ARG(a.in_deg != nullptr && a.out_deg != nullptr, "%s: in_deg/out_deg is null", fn);
  RSA_CHECK_ARG(a.nnz == 0 || (a.indices != nullptr && a.rev != nullptr), "%s: indices/rev is null", fn);
  RSA_CHECK_ARG(a.nnz == 0 || a.values != nullptr, "%s: values is null", fn);
  GraphDropParams p{};
  p.indptr = a.indptr, p.indices = a.indices, p.rev = a.rev, p.node_drop = a.node_drop;
  p.n_rows = a.n_rows, p.nnz = a.nnz;
  p.long_row = a.long_row ? a.long_row : GD_LONG_ROW;
  p.n_windows = (a.nnz + p.long_row - 1) / p.long_row;
  p.keep_prob = a.keep_prob, p.draw = a.keep_prob < 1.f;
  p.pc = PhiloxCall{a.seed, a.offset >> 2, a.grid_threads ? a.grid_threads : 1, a.elem_base};
  p.keep = a.keep, p.in_deg = a.in_deg, p.out_deg = a.out_deg, p.values = a.values, p.t_values = a.t_values;
  const int64_t blocks = (p.n_rows + p.n_windows + 3) / 4;
  RSA_CHECK_ARG(blocks < (1ll << 31), "%s: too many rows for one launch", fn);
  hipStream_t s = (hipStream_t)stream;
  if (hipMemsetAsync(a.in_deg, 0, (size_t)a.n_rows * 4, s) != hipSuccess || hipMemsetAsync(a.out_deg, 0, (size_t)a.n_rows * 4, s) != hipSuccess) {
    set_error("%s: clearing the degree counters failed: %s", fn, hipGetErrorString(hipGetLastError()));
    return RSA_ERR_HIP;
  }
  hipLaunchKernelGGL(graph_dropout_kernel<0>, dim3((unsigned)blocks), dim3(256), 0, s, p);
  RSA_CHECK_LAUNCH(fn);
  if (a.nnz) {
    hipLaunchKernelGGL(graph_dropout_kernel<1>, dim3((unsigned)blocks), dim3(256), 0, s, p);
    RSA_CHECK_LAUNCH(fn);
  }
  return RSA_OK;
}
