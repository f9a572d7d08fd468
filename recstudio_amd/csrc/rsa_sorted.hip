// Atomics-free, deterministic row scatter-add:  target[id] += scale * sum_{e : id_e = id} d_e * query[qrow_e]
// over the B*(1+n) (positive and negative) elements of a step.
//
// embedding_dense_backward / index_add_ of the reference (recstudio/model/basemodel/recommender.py:636-639 via
// autograd) is an atomic scatter in ATen and in rsa_fused_backward's dense mode.  Float atomics from 8 XCDs to
// one table are performed at the memory side, a dword at a time: 537 M of them cost 2.5 ms per step at
// B = 65536, n = 64, d = 128.  Here the elements are sorted by item id first (the in-tree LSD radix sort of packed (id,
// element) pairs, rsa_radix.hpp, stable), every wave sums its 64 sorted elements run by run in element order, and every row is read-modified-
// written once with full-line accesses: no atomics, bit-reproducible, ~2x faster.  A run that crosses chunk
// boundaries (rare and short for item ids; the RULE when the key is a query index -- the owner side of the sharded
// backward sums ~1000 item rows per query) is not walked by one wave: each chunk leaves the partial sum of its
// leading / trailing open segment in the workspace and a second kernel adds a run's partials in chunk order.
// `target` may be a zeroed dense gradient (== the reference's weight.grad) or the weight table itself with
// scale = -lr (plain SGD applied in place).  With optimizer state the same passes apply a rule to every touched row instead of
// adding: lazy Adam (exp_avg / exp_avg_sq: torch.optim.SparseAdam, two state rows per row: AdamRule) or torch.optim.Adagrad
// (state_sum: one state row per row, `learner: adagrad` of the reference, recommender.py:466-467: AdagradRule).  The passes
// are written once (sorted_apply_frame, sorted_finish_frame); the kernels are those frames under a rule.
#include "rsa_common.hpp"
#include "rsa_radix.hpp"
#include "rsa_internal.hpp"
#include <cstring>
#include <type_traits>

// rows requested ahead by the apply pass.  4: 78 VGPRs at d = 128 = 6 waves/SIMD; 8: 110 = 4 waves.  In-process A/B
// (tools/exp_sorted_ab.py, us per launch, 4 vs 8): headline shape all elements 836.2 / 837.7, solo rows skipped 343.7 / 350.4;
// the sharded backward's scatters onto 4096 query rows 476.5 / 485.5 and onto item rows 839.9 / 843.0; 16 (179 VGPRs): 2-3 x slower
#ifndef RSA_SORTED_UNROLL
#define RSA_SORTED_UNROLL 4
#endif
// Target rows (and the lazy-Adam state rows) are touched ONCE per pass; the query rows are re-read once per element.  With
// streaming (nontemporal) accesses for the former the latter keep their L2 lines: the 2 MB of a 4096-query step's rows were
// otherwise re-fetched per ELEMENT under the 5 GB row stream (2.05 GB of 3.87 GB fetched).
// 0: never, 1: always, 2 (default): when the target table is larger than 512 MB
#ifndef RSA_SORTED_NT
#define RSA_SORTED_NT 2
#endif

namespace rsa {

template <bool NT>
__device__ __forceinline__ float ld_row(const float* p) {
  if constexpr (NT) return __builtin_nontemporal_load(p);
  return *p;
}
template <bool NT>
__device__ __forceinline__ void st_row(float* p, float v) {
  if constexpr (NT) __builtin_nontemporal_store(v, p);
  else *p = v;
}

// ---- the rules: what a touched row becomes, given the run's sum.  The two passes below (sorted_apply_frame,
// sorted_finish_frame) are written once over a rule: NS state rows travel with a target row, state(s) is the table of the
// s-th, and apply_run read-modify-writes target[cur] and its state rows ONCE from `acc`; trow / srow are the rows' current
// values (requested earlier, at the head of the run).

// Plain accumulate (exp_avg == nullptr, decided at run time: SGD and Adam share their instantiations) or lazy Adam.
struct AdamRule {
  static constexpr int NS = 2;
  static constexpr const char* who = "rsa_rows_update_sorted(apply)";
  AdamArgs a;
  __device__ __forceinline__ bool has_state() const { return a.exp_avg != nullptr; }
  __device__ __forceinline__ float* state(int s) const { return s == 0 ? a.exp_avg : a.exp_avg_sq; }
  template <int NDW, bool NT>
  __device__ __forceinline__ void apply_run(float* __restrict__ target, int32_t cur, float scale, int lane, const float (&acc)[NDW],
                                            const float (&trow)[NDW], const float (&srow)[NS][NDW]) const {
    constexpr int D = 64 * NDW;
    float* row = target + (size_t)cur * D;
    if (a.exp_avg == nullptr) {
#pragma unroll
      for (int k = 0; k < NDW; ++k) st_row<NT>(row + k * 64 + lane, trow[k] + scale * acc[k]);
      return;
    }
    // lazy Adam on the touched row (torch.optim.SparseAdam's update, torch/optim/_functional.py sparse_adam):
    // m += (g - m)(1 - b1); v += (g^2 - v)(1 - b2); w -= step_size * m / (sqrt(v) + eps)
    float* mrow = a.exp_avg + (size_t)cur * D;
    float* vrow = a.exp_avg_sq + (size_t)cur * D;
#pragma unroll
    for (int k = 0; k < NDW; ++k) {
      const int c = k * 64 + lane;
      const float g = scale * acc[k];
      const float m0 = srow[0][k], v0 = srow[1][k];
      const float m1 = m0 + (g - m0) * a.one_minus_beta1;
      const float v1 = v0 + (g * g - v0) * a.one_minus_beta2;
      st_row<NT>(mrow + c, m1);
      st_row<NT>(vrow + c, v1);
      st_row<NT>(row + c, trow[k] - a.step_size * (m1 / (sqrtf(v1) + a.eps)));
    }
  }
};

// rsa_rows_update_args.rule == RSA_ROWS_ADAGRAD: torch.optim.Adagrad on the touched rows
//     g = upstream * run sum;   s' = s + g g;   w' = w - clr (g / (sqrt(s') + eps))
// with ONE state table.  A row without a kept element has g = 0, for which torch's dense pass changes neither s nor w
// (0 / (sqrt(s) + eps) = 0): leaving such rows alone IS the dense rule, and the sparse branch of torch.optim.Adagrad squares
// the coalesced row gradient -- the run sum these passes hold in registers.
// Every rounding is spelled out so that tests/adagrad_referee.py can follow it operation for operation:
//     g   = fl(scale * acc)
//     s'  = fl(g * g + s)                 FUSED: one rounding
//     den = fl(fl(sqrt(s')) + eps)        sqrtf and the division are the correctly rounded ones (hipcc's default)
//     q   = fl(g / den)
//     w'  = fl(-clr * q + w)              FUSED: one rounding
// Only a step's elements are ever stepped (DecStep): exchange segments are accumulated, never stepped.
struct AdagradRule {
  static constexpr int NS = 1;
  static constexpr const char* who = "rsa_rows_update_sorted(adagrad apply)";
  AdagradArgs a;
  __device__ __forceinline__ bool has_state() const { return true; }
  __device__ __forceinline__ float* state(int) const { return a.state_sum; }
  template <int NDW, bool NT>
  __device__ __forceinline__ void apply_run(float* __restrict__ target, int32_t cur, float scale, int lane, const float (&acc)[NDW],
                                            const float (&trow)[NDW], const float (&srow)[NS][NDW]) const {
    constexpr int D = 64 * NDW;
    float* row = target + (size_t)cur * D;
    float* srow_p = a.state_sum + (size_t)cur * D;
#pragma unroll
    for (int k = 0; k < NDW; ++k) {
      const int c = k * 64 + lane;
      const float g = __fmul_rn(scale, acc[k]);
      const float s1 = __fmaf_rn(g, g, srow[0][k]);
      const float den = __fadd_rn(sqrtf(s1), a.eps);
      const float q = g / den;
      st_row<NT>(srow_p + c, s1);
      st_row<NT>(row + c, __fmaf_rn(-a.clr, q, trow[k]));
    }
  }
};

// Per-chunk record of the open segments: meta[4 c + 0] = key of the LEADING segment if it continues the previous chunk's
// run (else -1), [1] = 1 if that segment is the whole chunk, [2] = key of the TRAILING segment if its run goes on into
// the next chunk and started in this one (else -1).
enum { META_LEAD_KEY = 0, META_LEAD_FULL = 1, META_TRAIL_KEY = 2, META_STRIDE = 4 };

// What element e of the sorted pairs stands for: its query row and its coefficient d loss/d score.
struct DecStep {             // a step's [M, (1 +) n] element order: e = m * w + c
  const int64_t* query_index;
  const float* dpos;
  const float* dneg;
  int n, has_pos;
  __device__ __forceinline__ void operator()(int64_t e, int32_t& qrow, float& coef) const {
    const int w = n + has_pos;
    const int64_t m = (uint32_t)e / (uint32_t)w;
    const int c = (int)(e - m * w);
    qrow = (int32_t)(query_index ? query_index[m] : m);
    coef = (has_pos && c == 0) ? dpos[m] : dneg[m * (int64_t)n + (c - has_pos)];
  }
};
struct DecSegments {         // received exchange segments: e = slot, key = (query << 32 | row), d in slot order;
  const int64_t* keys;       // e >= slots: the positive of query e - slots (its coefficient sits behind the slots' in d)
  const float* d;
  int64_t slots;
  __device__ __forceinline__ void operator()(int64_t e, int32_t& qrow, float& coef) const {
    qrow = e >= slots ? (int32_t)(e - slots) : (int32_t)((keys[e] >> 32) & 0x7fffffffll);
    coef = d[e];
  }
};

// The apply pass, one wave per chunk: NDW dwords per lane per row (D = 64 * NDW); NT: streaming accesses to the target (and
// state) rows.
template <int NDW, bool NT, class RULE, class DEC>
__device__ __forceinline__ void sorted_apply_frame(const uint64_t* __restrict__ pairs, int64_t total, const float* __restrict__ query,
                                                   const DEC& dec, const float* __restrict__ upstream, int32_t pad_row,
                                                   int32_t drop_key, float* __restrict__ target, const RULE& rule,
                                                   float* __restrict__ lead_part, float* __restrict__ trail_part,
                                                   int32_t* __restrict__ meta, int32_t key_base, int32_t elem_base,
                                                   int32_t chunk_elems) {
  constexpr int D = 64 * NDW, NS = RULE::NS;
  const int lane = lane_id();
  const int64_t chunk = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  // chunk_elems = 64, or 16 for a small pass (sorted_chunk_elems): a wave walks its elements a few at a time, one round trip
  // per group -- the 65 536 user rows of the headline step as 1024 waves x 16 groups took 30 us of latency for 100 MB
  const int64_t begin = chunk * chunk_elems;
  if (begin >= total) return;
  const float scale = upstream ? upstream[0] : 1.f;
  // this lane's element of the chunk: key, query row, coefficient (all lanes in parallel)
  const int64_t i = begin + lane;
  const bool in = lane < chunk_elems && i < total;
  const uint64_t pr = in ? pairs[i] : 0ull;
  // key_base / elem_base (0 but for the user part of a merged step sort, sort_step_all): what the part's keys and element
  // numbers are offset by inside the common sort
  const int32_t key = in ? (int32_t)(rdx_key(pr) - (uint32_t)key_base) : -1;
  int32_t qrow = 0;
  float coef = 0.f;
  bool solo = false;                  // flagged by classify_solo_kernel: the row has been applied by the forward
  if (in && key != drop_key) {        // empty slots: nothing is read for them (their query index is -1)
    int32_t e = (int32_t)rdx_val(pr);
    solo = e < 0;
    e = (e & 0x7fffffff) - elem_base;
    if (!solo) dec((int64_t)e, qrow, coef);
  }
  const int cnt = (int)(total - begin < chunk_elems ? total - begin : chunk_elems);
  const int32_t prev = begin > 0 ? (int32_t)(rdx_key(pairs[begin - 1]) - (uint32_t)key_base) : -1;                     // key in front of the chunk
  const int32_t next = begin + cnt < total ? (int32_t)(rdx_key(pairs[begin + cnt]) - (uint32_t)key_base) : -1;         // key behind it
  float acc[NDW];
  float trow[NDW], srow[NS][NDW];     // the current run's target (and state) rows, requested at its head
#pragma unroll
  for (int k = 0; k < NDW; ++k) {
    acc[k] = trow[k] = 0.f;
#pragma unroll
    for (int s = 0; s < NS; ++s) srow[s][k] = 0.f;
  }
  int32_t cur = -1;           // id of the run being accumulated (-1: none)
  bool leading = false;       // accumulating the segment that continues the previous chunk's run
  int32_t lead_key = -1;
  auto close_segment = [&]() {        // a new run begins (or the chunk ends closed): what has been summed so far is complete
    if (leading) {
#pragma unroll
      for (int k = 0; k < NDW; ++k) lead_part[(size_t)chunk * D + k * 64 + lane] = acc[k];
      leading = false;
    } else if (cur >= 0) {
      rule.template apply_run<NDW, NT>(target, cur, scale, lane, acc, trow, srow);
    }
#pragma unroll
    for (int k = 0; k < NDW; ++k) acc[k] = 0.f;
  };
  // Only the elements with work are visited: not the dropped ones (empty slots), not the padding row's, not the ones a
  // forward has applied itself (solo) -- in a step whose solo rows are applied in the forward half of a chunk is such,
  // and a pass that walked them anyway (redirected to row 0) ran no faster than the full one.  None of them can sit
  // INSIDE a run that has work (a run is one key), so skipping them leaves every run's element order untouched, and rows
  // without a kept element are neither read nor written.
  uint64_t work = __ballot(in && !solo && key != drop_key && key != pad_row);
  int last_t = -1;
  // The query rows AND the target (and state) rows of U elements are requested together before the (serial) run logic
  // consumes them.  Round 1 loaded one query row per iteration and read-modified-wrote the target row inside flush(): every
  // element waited for its own round trip and every run for an HBM read in the middle of the serial chain (VERDICT r1:
  // 0.9 ms of the 1.7 ms SGD step).  A target row belongs to exactly one run and a closed run to exactly one wave, so
  // reading it at the head of the run instead of at its end sees the same value.  Slots past the last element with
  // work request row 0, always readable.
  constexpr int U = RSA_SORTED_UNROLL;
  while (work) {
    int ts[U];
    int nu = 0;
#pragma unroll
    for (int u = 0; u < U; ++u) {
      ts[u] = 63;
      if (work) {
        ts[u] = __ffsll((unsigned long long)work) - 1;
        work &= work - 1;
        nu = u + 1;
      }
    }
    float qv[U][NDW], tv[U][NDW], sv[U][NS][NDW];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int32_t qr = u < nu ? __builtin_amdgcn_readlane(qrow, ts[u]) : 0;
      const int32_t kr = u < nu ? __builtin_amdgcn_readlane(key, ts[u]) : 0;
      const float* qp = query + (size_t)qr * D;
      const float* tp = target + (size_t)kr * D;
#pragma unroll
      for (int k = 0; k < NDW; ++k) {
        qv[u][k] = qp[k * 64 + lane];
        tv[u][k] = ld_row<NT>(tp + k * 64 + lane);
      }
      if (rule.has_state()) {
#pragma unroll
        for (int k = 0; k < NDW; ++k) {
#pragma unroll
          for (int s = 0; s < NS; ++s) sv[u][s][k] = ld_row<NT>(rule.state(s) + (size_t)kr * D + k * 64 + lane);
        }
      } else {
#pragma unroll
        for (int k = 0; k < NDW; ++k) {
#pragma unroll
          for (int s = 0; s < NS; ++s) sv[u][s][k] = 0.f;
        }
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (u >= nu) break;
      const int t = ts[u];
      const int32_t kt = __builtin_amdgcn_readlane(key, t);
      const int32_t before = t == 0 ? prev : __builtin_amdgcn_readlane(key, t - 1);
      const bool head = kt != before;
      if (head) {
        close_segment();
        cur = kt;
#pragma unroll
        for (int k = 0; k < NDW; ++k) {
          trow[k] = tv[u][k];
#pragma unroll
          for (int s = 0; s < NS; ++s) srow[s][k] = sv[u][s][k];
        }
      } else if (t == 0) {            // the chunk opens inside a run that began in an earlier chunk
        leading = true;
        cur = lead_key = kt;
      }
      const float cf = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(coef), t));   // bit pattern, not a value cast
#pragma unroll
      for (int k = 0; k < NDW; ++k) acc[k] = __fmaf_rn(cf, qv[u][k], acc[k]);
      last_t = t;
    }
    // vmcnt(0): the rows requested above that nothing read (an element that is not its run's head, a slot past the last
    // element) have landed.  Left outstanding, they make the compiler wait for them in the middle of the next requests.
    __builtin_amdgcn_s_waitcnt(0x0f70);
  }
  // the chunk's last segment: still the leading one (the whole chunk lies inside one run), open towards the next chunk,
  // or closed
  const bool whole = leading;
  int32_t trail_key = -1;
  if (leading) {
    close_segment();                                  // -> lead_part
  } else if (cur >= 0 && last_t == cnt - 1 && next == cur) {
    trail_key = cur;                                  // the run goes on: the finish pass owns its row
#pragma unroll
    for (int k = 0; k < NDW; ++k) trail_part[(size_t)chunk * D + k * 64 + lane] = acc[k];
  } else {
    close_segment();
  }
  if (lane == 0) {
    meta[chunk * META_STRIDE + META_LEAD_KEY] = lead_key;
    meta[chunk * META_STRIDE + META_LEAD_FULL] = whole ? 1 : 0;
    meta[chunk * META_STRIDE + META_TRAIL_KEY] = trail_key;
  }
}

// The finish pass, one wave per chunk whose trailing segment opened a run: adds the leading partials of the following chunks
// in chunk order (a chunk that lies wholly inside the run passes the walk on) and applies the row once.  Plain accesses (a
// few rows per pass).
template <int NDW, class RULE>
__device__ __forceinline__ void sorted_finish_frame(int64_t n_chunks, const float* __restrict__ upstream, int32_t pad_row,
                                                    float* __restrict__ target, const RULE& rule,
                                                    const float* __restrict__ lead_part, const float* __restrict__ trail_part,
                                                    const int32_t* __restrict__ meta) {
  constexpr int D = 64 * NDW, NS = RULE::NS;
  const int lane = lane_id();
  const int64_t chunk = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (chunk >= n_chunks) return;
  const int32_t cur = meta[chunk * META_STRIDE + META_TRAIL_KEY];
  if (cur < 0 || cur == pad_row) return;
  const float scale = upstream ? upstream[0] : 1.f;
  float acc[NDW], trow[NDW], srow[NS][NDW];
#pragma unroll
  for (int k = 0; k < NDW; ++k) {
    acc[k] = trail_part[(size_t)chunk * D + k * 64 + lane];
    trow[k] = target[(size_t)cur * D + k * 64 + lane];
#pragma unroll
    for (int s = 0; s < NS; ++s) srow[s][k] = rule.has_state() ? rule.state(s)[(size_t)cur * D + k * 64 + lane] : 0.f;
  }
  for (int64_t c2 = chunk + 1; c2 < n_chunks; ++c2) {
    if (meta[c2 * META_STRIDE + META_LEAD_KEY] != cur) break;
#pragma unroll
    for (int k = 0; k < NDW; ++k) acc[k] += lead_part[(size_t)c2 * D + k * 64 + lane];
    if (!meta[c2 * META_STRIDE + META_LEAD_FULL]) break;
  }
  rule.template apply_run<NDW, false>(target, cur, scale, lane, acc, trow, srow);
}

// The kernels: the two frames under a rule.  One wave per chunk of 64 sorted elements; runs that begin and end inside the
// chunk are applied by the apply kernel, the open leading / trailing segments leave their partial sums in lead_part /
// trail_part [chunk, D] for the finish kernel.
#ifndef RSA_SORTED_MIN_WAVES
#define RSA_SORTED_MIN_WAVES 1
#endif
template <int NDW, class DEC, bool NT>
__global__ __launch_bounds__(256, RSA_SORTED_MIN_WAVES) void sorted_apply_kernel(const uint64_t* __restrict__ pairs,
                                                           int64_t total, const float* __restrict__ query, const DEC dec,
                                                           const float* __restrict__ upstream, int32_t pad_row,
                                                           int32_t drop_key, float* __restrict__ target, AdamArgs adam,
                                                           float* __restrict__ lead_part, float* __restrict__ trail_part,
                                                           int32_t* __restrict__ meta, int32_t key_base, int32_t elem_base,
                                                           int32_t chunk_elems) {
  sorted_apply_frame<NDW, NT>(pairs, total, query, dec, upstream, pad_row, drop_key, target, AdamRule{adam}, lead_part, trail_part,
                              meta, key_base, elem_base, chunk_elems);
}

template <int NDW>
__global__ __launch_bounds__(256) void sorted_finish_kernel(int64_t n_chunks, const float* __restrict__ upstream,
                                                            int32_t pad_row, float* __restrict__ target, AdamArgs adam,
                                                            const float* __restrict__ lead_part,
                                                            const float* __restrict__ trail_part,
                                                            const int32_t* __restrict__ meta) {
  sorted_finish_frame<NDW>(n_chunks, upstream, pad_row, target, AdamRule{adam}, lead_part, trail_part, meta);
}

template <int NDW, bool NT>
__global__ __launch_bounds__(256, RSA_SORTED_MIN_WAVES) void sorted_apply_adagrad_kernel(
    const uint64_t* __restrict__ pairs, int64_t total, const float* __restrict__ query, const DecStep dec,
    const float* __restrict__ upstream, int32_t pad_row, int32_t drop_key, float* __restrict__ target, AdagradArgs ada,
    float* __restrict__ lead_part, float* __restrict__ trail_part, int32_t* __restrict__ meta, int32_t chunk_elems) {
  sorted_apply_frame<NDW, NT>(pairs, total, query, dec, upstream, pad_row, drop_key, target, AdagradRule{ada}, lead_part,
                              trail_part, meta, 0, 0, chunk_elems);
}

template <int NDW>
__global__ __launch_bounds__(256) void sorted_finish_adagrad_kernel(int64_t n_chunks, const float* __restrict__ upstream,
                                                                    int32_t pad_row, float* __restrict__ target, AdagradArgs ada,
                                                                    const float* __restrict__ lead_part,
                                                                    const float* __restrict__ trail_part,
                                                                    const int32_t* __restrict__ meta) {
  sorted_finish_frame<NDW>(n_chunks, upstream, pad_row, target, AdagradRule{ada}, lead_part, trail_part, meta);
}

// After the sort: an element whose key differs from both neighbours is the ONLY element of the step on its row ("solo").
// solo[e] (element order) <- 1 for such elements unless the row is the padding row / a dropped id, and bit 31 of the
// element number in `vals` is set so that the apply kernel leaves the row alone: a forward that updates solo rows
// itself (rsa_fused_args.solo_flags) has already applied them.
constexpr int32_t SOLO_BIT = (int32_t)0x80000000;
// MOSTLY_SOLO: the flags were preset to 1 and the elements that are NOT solo store a 0 -- the scattered byte stores are the cost
// of this pass (each its own 64-byte write request: 3 M of them 38 us), so the host picks the polarity with fewer of them.
template <bool MOSTLY_SOLO>
__global__ __launch_bounds__(256) void classify_solo_kernel(uint64_t* __restrict__ pairs, int64_t total, int32_t pad_row,
                                                            int32_t drop_key, uint8_t* __restrict__ solo) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
    const uint64_t pr = pairs[i];
    const int32_t k = (int32_t)rdx_key(pr);
    const int32_t before = i > 0 ? (int32_t)rdx_key(pairs[i - 1]) : -1, after = i + 1 < total ? (int32_t)rdx_key(pairs[i + 1]) : -1;
    const uint32_t e = rdx_val(pr);
    if (k != before && k != after && k != pad_row && k != drop_key) {
      if (!MOSTLY_SOLO) solo[e] = 1;                     // (the flags were zeroed: only the ones are stored)
      pairs[i] = pr | (uint64_t)(uint32_t)SOLO_BIT;      // (only the payload word changes: a neighbour reading the key races on nothing)
    } else if (MOSTLY_SOLO) {
      solo[e] = 0;
    }
  }
}

// ---- the workspace of a sorted scatter over `max_total` elements: two packed-pair buffers, the radix sort's counters,
// per 64-element chunk two partial rows (sized for dim = 256) and the segment record
// Chunks of the apply pass: 64 sorted elements per wave, 16 for a pass over at most SMALL_TOTAL elements (a function of the
// pass's total ALONE, so that two passes over the same elements sum in the same order wherever they run).  The workspace holds
// per-chunk records for ANY total <= max_total (callers size it for their largest step): the bound below is monotone.
constexpr int64_t SORTED_SMALL_TOTAL = 1 << 18;
int sorted_chunk_elems(int64_t total) { return total <= SORTED_SMALL_TOTAL ? 16 : 64; }
static int64_t sorted_max_chunks(int64_t max_total) {
  const int64_t by64 = (max_total + 63) / 64;
  const int64_t small = max_total < SORTED_SMALL_TOTAL ? max_total : SORTED_SMALL_TOTAL;
  const int64_t by16 = (small + 15) / 16;
  return by64 > by16 ? by64 : by16;
}

static SortedLayout carve_sorted(Carver& ws, int64_t max_total) {
  const int64_t chunks = sorted_max_chunks(max_total);
  SortedLayout L;
  L.pairs_a = ws.take<uint64_t>(max_total);
  L.pairs_b = ws.take<uint64_t>(max_total);
  L.temp = ws.take<char>(radix_temp_bytes(max_total));
  L.lead_part = ws.take<float>(chunks * 256);
  L.trail_part = ws.take<float>(chunks * 256);
  L.meta = ws.take<int32_t>(chunks * META_STRIDE);
  return L;
}

int64_t sorted_workspace_bytes(int64_t max_total) {
  Carver sizing(nullptr);
  carve_sorted(sizing, max_total);
  return align256(sizing.bytes()) + 256;
}

SortedLayout sorted_layout(void* workspace, int64_t max_total) {
  Carver ws(workspace);
  return carve_sorted(ws, max_total);
}

int classify_solo(uint64_t* pairs, int64_t total, int64_t pad_row, int64_t drop_key, uint8_t* solo, hipStream_t s, const char* who) {
  const int32_t pad = (int32_t)(pad_row < 0 || pad_row >= (1ll << 31) ? -2 : pad_row);
  // `total` draws over `drop_key` rows (drop_key = the row count): under a uniform draw a row is alone with probability
  // exp(-total / rows), i.e. most elements are solo below total / rows = ln 2.  A skewed draw has fewer solo elements than that;
  // the guess only decides which of the two polarities stores fewer bytes.
  const bool mostly_solo = (double)total < 0.69 * (double)drop_key;
  RSA_CHECK_HIP(hipMemsetAsync(solo, mostly_solo ? 1 : 0, (size_t)total, s), who);
  dispatch_bool(mostly_solo, [&](auto MOSTLY_SOLO) {
    hipLaunchKernelGGL(classify_solo_kernel<MOSTLY_SOLO()>, dim3(grid_1d(total, 256, 8192)), dim3(256), 0, s, pairs, total, pad,
                       (int32_t)drop_key, solo);
  });
  RSA_CHECK_LAUNCH(who);
  return RSA_OK;
}

// the apply + finish passes over sorted pairs.  The Adagrad kernels exist for a step's elements only (DEC = DecStep, no
// key_base / elem_base).
template <class RULE, class DEC>
static int apply_sorted_pairs(const uint64_t* pairs, int64_t total, const float* query, int32_t dim, const DEC& dec,
                              const float* upstream, int64_t drop_key, int64_t pad_row, float* target, const RULE& rule,
                              const SortedLayout& L, hipStream_t s, int64_t key_base = 0, int64_t elem_base = 0) {
  constexpr bool ADAGRAD = std::is_same_v<RULE, AdagradRule>;
  const int ce = sorted_chunk_elems(total);
  const unsigned chunks = (unsigned)((total + ce - 1) / ce);
  dim3 grid((chunks + 3) / 4), block(256);
  const int32_t pad = (int32_t)(pad_row < 0 || pad_row >= (1ll << 31) ? -2 : pad_row);
  // (drop_key = the table's row count; the state tables stream with the target)
  const bool nt = RSA_SORTED_NT == 1 || (RSA_SORTED_NT == 2 && streams_past_cache(drop_key, dim));
  const bool built = dispatch_dim<64, 128, 256>(dim, [&](auto D) {
    constexpr int NDW = D() / 64;
    dispatch_bool(nt, [&](auto NT) {
      if constexpr (ADAGRAD)
        hipLaunchKernelGGL((sorted_apply_adagrad_kernel<NDW, NT()>), grid, block, 0, s, pairs, total, query, dec, upstream, pad,
                           (int32_t)drop_key, target, rule.a, L.lead_part, L.trail_part, L.meta, (int32_t)ce);
      else
        hipLaunchKernelGGL((sorted_apply_kernel<NDW, DEC, NT()>), grid, block, 0, s, pairs, total, query, dec, upstream, pad,
                           (int32_t)drop_key, target, rule.a, L.lead_part, L.trail_part, L.meta, (int32_t)key_base,
                           (int32_t)elem_base, (int32_t)ce);
    });
    if constexpr (ADAGRAD)
      hipLaunchKernelGGL(sorted_finish_adagrad_kernel<NDW>, grid, block, 0, s, (int64_t)chunks, upstream, pad, target, rule.a,
                         L.lead_part, L.trail_part, L.meta);
    else
      hipLaunchKernelGGL(sorted_finish_kernel<NDW>, grid, block, 0, s, (int64_t)chunks, upstream, pad, target, rule.a, L.lead_part,
                         L.trail_part, L.meta);
  });
  if (!built) {
    rsa::set_error("rsa_rows_update_sorted: dim=%d: built for dim in {64, 128, 256}", dim);
    return RSA_ERR_UNSUPPORTED;
  }
  RSA_CHECK_LAUNCH(RULE::who);
  return RSA_OK;
}

int apply_sorted_segments(const uint64_t* pairs, int64_t total, int64_t slots, const float* query, int32_t dim,
                          const int64_t* keys, const float* d, const float* upstream, int64_t n_rows, int64_t pad_row,
                          float* target, const SortedLayout& L, hipStream_t s) {
  const AdamRule none{{nullptr, nullptr, 0.f, 0.f, 0.f, 0.f}};
  const DecSegments dec{keys, d, slots};
  return apply_sorted_pairs(pairs, total, query, dim, dec, upstream, n_rows, pad_row, target, none, L, s);
}

// ---- the in-place SGD step (rsa_step.hip): ONE sort for the step's item elements AND its user elements (SrcStepAll)
static unsigned step_all_bits(int64_t n_items, int64_t n_users) { return radix_key_bits(n_items + n_users + 2); }

int64_t step_all_workspace_bytes(int64_t n_queries, int32_t num_neg) { return sorted_workspace_bytes(n_queries * (int64_t)(num_neg + 2)); }

int sort_step_all(const int64_t* pos_ids, int64_t* neg_ids, const int64_t* user_ids, int64_t n_queries, int32_t num_neg,
                  int64_t n_items, int64_t n_users, uint8_t* solo, void* workspace, int64_t workspace_bytes, const StepDraw* draw,
                  hipStream_t s, const char* who) {
  const int64_t t_items = n_queries * (int64_t)(num_neg + 1), total = t_items + n_queries;
  RSA_CHECK_ARG(total < (1ll << 31) && n_items + n_users + 2 < (1ll << 31), "%s: more than 2^31 elements / keys", who);
  const int64_t need = step_all_workspace_bytes(n_queries, num_neg);
  RSA_CHECK_ARG(workspace && workspace_bytes >= need, "%s: item_workspace too small (%lld < %lld = "
                "rsa_scatter_rows_sorted_workspace_bytes(n_queries, num_neg + 1, n_items): the user rows are sorted with the item rows)",
                who, (long long)workspace_bytes, (long long)need);
  const SortedLayout L = sorted_layout(workspace, total);
  const unsigned bits = step_all_bits(n_items, n_users);
  const SrcStepIds it{pos_ids, neg_ids, n_items, num_neg, num_neg + 1, 1};
  const StepDraw none{nullptr, 0, 0, PhiloxCall{0, 0, 1, 0}, 0, 0, nullptr, nullptr, nullptr};
  const SrcStepAll<false> rd{it, user_ids, t_items, n_users, (uint32_t)(n_items + 1), none};
  hipError_t err;
  if (draw != nullptr && draw->kind != 0) {
    const SrcStepAll<true> dw{it, user_ids, t_items, n_users, (uint32_t)(n_items + 1), *draw};
    err = radix_sort_pairs2(dw, rd, L.pairs_a, L.pairs_b, total, bits, L.temp, s);
  } else {
    err = radix_sort_pairs(rd, L.pairs_a, L.pairs_b, total, bits, L.temp, s);
  }
  if (err != hipSuccess) {
    rsa::set_error("%s: radix sort failed: %s", who, hipGetErrorString(hipGetLastError()));
    return RSA_ERR_HIP;
  }
  // the item part only: a user row is never updated by the forward
  return classify_solo(radix_result(L.pairs_a, L.pairs_b, bits), t_items, 0, n_items, solo, s, who);
}

// the shared item rows (users == false) or the user rows (users == true) of the step sorted by sort_step_all
int apply_step_all(bool users, const float* query, const int64_t* query_index, int32_t dim, int64_t n_queries, int32_t num_neg,
                   const float* dpos, const float* dneg, const float* upstream, int64_t n_items, int64_t n_users, float* target,
                   void* workspace, hipStream_t s) {
  const int64_t t_items = n_queries * (int64_t)(num_neg + 1), total = t_items + n_queries;
  const SortedLayout L = sorted_layout(workspace, total);
  const uint64_t* sorted = radix_result(L.pairs_a, L.pairs_b, step_all_bits(n_items, n_users));
  const AdamRule none{{nullptr, nullptr, 0.f, 0.f, 0.f, 0.f}};
  if (!users) {
    const DecStep dec{query_index, dpos, dneg, (int)num_neg, 1};
    return apply_sorted_pairs(sorted, t_items, query, dim, dec, upstream, n_items, 0, target, none, L, s);
  }
  const DecStep dec{nullptr, nullptr, dneg, 1, 0};      // element m: query row m of `query`, coefficient dneg[m]
  return apply_sorted_pairs(sorted + t_items, n_queries, query, dim, dec, upstream, n_users, 0, target, none, L, s, n_items + 1, t_items);
}

}  // namespace rsa

using namespace rsa;

extern "C" int64_t rsa_scatter_rows_sorted_workspace_bytes(int64_t n_queries, int32_t num_neg, int64_t n_items) {
  if (n_queries <= 0 || num_neg < 0 || n_items < 1) return 0;
  return sorted_workspace_bytes(n_queries * (int64_t)(num_neg + 1));     // sized for the with-positives layout
}

// where the sorted pairs of a step live in its workspace (a function of the sizes alone: the sort and the apply are
// separate entry points)
static uint64_t* step_sorted(const SortedLayout& L, int64_t n_items) {
  return radix_result(L.pairs_a, L.pairs_b, radix_key_bits(n_items + 1));      // ids 0 .. n_items-1 and the drop key n_items
}

// Read-only: where a sort leaves its pairs, as a byte offset from the workspace pointer rounded up to 256 bytes (Carver's rule).
// Laid out over a made-up base (layout_probe_base) by the very calls the sorts make, so the two cannot disagree.
extern "C" int64_t rsa_scatter_rows_sorted_pairs_offset(int64_t n_queries, int32_t num_neg, int64_t n_items) {
  if (n_queries <= 0 || num_neg < 0 || n_items < 1 || n_items >= (1ll << 31)) return -1;
  const SortedLayout L = sorted_layout(layout_probe_base(), n_queries * (int64_t)(num_neg + 1));
  return layout_probe_offset(step_sorted(L, n_items));
}

extern "C" int64_t rsa_bpr_sgd_pairs_offset(int64_t n_queries, int32_t num_neg, int64_t n_items, int64_t n_users) {
  if (n_queries <= 0 || num_neg < 0 || n_items < 1 || n_users < 1 || n_items + n_users + 2 >= (1ll << 31)) return -1;
  const int64_t total = n_queries * (int64_t)(num_neg + 1) + n_queries;      // sort_step_all's
  const SortedLayout L = sorted_layout(layout_probe_base(), total);
  return layout_probe_offset(radix_result(L.pairs_a, L.pairs_b, step_all_bits(n_items, n_users)));
}

// (item id, element) pairs of a step, radix-sorted by id into the workspace; with `solo` also the classification pass
static int sort_step_elements(const rsa_rows_update_args& a, uint8_t* solo, hipStream_t s, const char* who) {
  RSA_CHECK_ARG(a.n_queries >= 0 && a.num_neg >= 1 && a.n_items >= 1 && a.n_items < (1ll << 31), "%s: bad sizes", who);
  if (a.n_queries == 0) return RSA_OK;
  RSA_CHECK_ARG(a.neg_ids != nullptr, "%s: neg_ids is null", who);
  const int has_pos = a.pos_ids != nullptr ? 1 : 0;
  const int64_t total = a.n_queries * (int64_t)(a.num_neg + has_pos);
  RSA_CHECK_ARG(total < (1ll << 31), "%s: more than 2^31 elements", who);
  const int64_t need = rsa_scatter_rows_sorted_workspace_bytes(a.n_queries, a.num_neg, a.n_items);
  RSA_CHECK_ARG(a.workspace && a.workspace_bytes >= need, "%s: workspace too small (%lld < %lld)", who, (long long)a.workspace_bytes,
                (long long)need);
  const SortedLayout L = sorted_layout(a.workspace, a.n_queries * (int64_t)(a.num_neg + 1));
  // pass 0 of the sort reads the id tensors themselves (no key-extraction launch, no id round trip)
  const SrcStepIds src{a.pos_ids, a.neg_ids, a.n_items, a.num_neg, a.num_neg + has_pos, has_pos};
  if (radix_sort_pairs(src, L.pairs_a, L.pairs_b, total, radix_key_bits(a.n_items + 1), L.temp, s) != hipSuccess) {
    rsa::set_error("%s: radix sort failed: %s", who, hipGetErrorString(hipGetLastError()));
    return RSA_ERR_HIP;
  }
  if (solo != nullptr) return classify_solo(step_sorted(L, a.n_items), total, a.pad_row, a.n_items, solo, s, who);
  return RSA_OK;
}

// The caller's hyper-parameters arrive as doubles (ABI 12): 1 - beta and the bias corrections are taken from THOSE values, as
// torch.optim.SparseAdam takes them from its Python floats, and each kernel constant is rounded to fp32 once.  (As floats,
// 1.f - float(0.999) = 0.0009999871: exp_avg_sq of every touched row 1.29e-5 short, the step size ~6e-6 off in one direction.)
static AdamRule adam_of(const rsa_rows_update_args& a) {
  if (a.exp_avg == nullptr) return AdamRule{{nullptr, nullptr, 0.f, 0.f, 0.f, 0.f}};
  const double bc1 = 1.0 - pow(a.beta1, (double)a.step), bc2 = 1.0 - pow(a.beta2, (double)a.step);
  return AdamRule{{a.exp_avg, a.exp_avg_sq, (float)(1.0 - a.beta1), (float)(1.0 - a.beta2), (float)a.eps,
                   (float)(a.lr * sqrt(bc2) / bc1)}};
}

static int check_adam(const rsa_rows_update_args& a, const char* who) {
  if (a.exp_avg == nullptr && a.exp_avg_sq == nullptr) return RSA_OK;
  RSA_CHECK_ARG(a.exp_avg && a.exp_avg_sq && a.step >= 1 && a.beta1 >= 0.0 && a.beta1 < 1.0 && a.beta2 >= 0.0 && a.beta2 < 1.0,
                "%s: bad optimizer state / hyper-parameters", who);
  return RSA_OK;
}

// Adagrad's constants as adam_of takes Adam's: clr = lr / (1 + (step - 1) lr_decay) (torch.optim.Adagrad, step 1-based) in
// double from the caller's doubles, each rounded to fp32 once.
static AdagradRule adagrad_of(const rsa_rows_update_args& a) {
  return AdagradRule{{a.state_sum, (float)(a.lr / (1.0 + (double)(a.step - 1) * a.lr_decay)), (float)a.eps}};
}

// Which rule the block asks for, and that rule's fields; before any HIP call.  rule 0 is the block as it was before `rule`
// existed (an older, shorter block reads 0): plain accumulate or lazy Adam, decided by exp_avg (check_adam).
static int check_rule(const rsa_rows_update_args& a, const char* who) {
  if (a.rule == 0) return check_adam(a, who);
  RSA_CHECK_ARG(a.rule == RSA_ROWS_ADAGRAD, "%s: unknown rule %d (0: accumulate / lazy Adam by exp_avg, %d: RSA_ROWS_ADAGRAD)", who,
                (int)a.rule, (int)RSA_ROWS_ADAGRAD);
  RSA_CHECK_ARG(a.state_sum != nullptr, "%s: Adagrad needs state_sum", who);
  RSA_CHECK_ARG(a.exp_avg == nullptr && a.exp_avg_sq == nullptr, "%s: Adagrad takes no exp_avg / exp_avg_sq (state_sum is its only state)", who);
  RSA_CHECK_ARG(a.step >= 1 && a.eps >= 0.0 && a.lr_decay >= 0.0, "%s: bad Adagrad hyper-parameters (step >= 1, eps >= 0, lr_decay >= 0)", who);
  return RSA_OK;
}

// the apply + finish passes over the sorted pairs in the workspace
static int apply_step_elements(const rsa_rows_update_args& a, int has_pos, hipStream_t s) {
  RSA_CHECK_ARG(a.n_queries >= 0 && a.num_neg >= 1 && a.n_items >= 1 && a.n_items < (1ll << 31), "rsa_rows_update_sorted: bad sizes");
  if (a.n_queries == 0) return RSA_OK;
  RSA_CHECK_ARG(a.query && a.dneg && a.target, "rsa_rows_update_sorted: null pointer");
  RSA_CHECK_ARG(!has_pos || a.dpos != nullptr, "rsa_rows_update_sorted: pos_ids without dpos");
  RSA_CHECK_ARG(a.query_index != nullptr || a.n_query_rows >= a.n_queries, "rsa_rows_update_sorted: query has fewer rows than n_queries");
  const int64_t total = a.n_queries * (int64_t)(a.num_neg + has_pos);
  const int64_t need = rsa_scatter_rows_sorted_workspace_bytes(a.n_queries, a.num_neg, a.n_items);
  RSA_CHECK_ARG(a.workspace && a.workspace_bytes >= need, "rsa_rows_update_sorted: workspace too small (%lld < %lld)",
                (long long)a.workspace_bytes, (long long)need);
  const SortedLayout L = sorted_layout(a.workspace, a.n_queries * (int64_t)(a.num_neg + 1));
  const DecStep dec{a.query_index, a.dpos, a.dneg, (int)a.num_neg, has_pos};
  auto apply = [&](const auto& rule) {
    return apply_sorted_pairs(step_sorted(L, a.n_items), total, a.query, a.dim, dec, a.upstream, a.n_items, a.pad_row, a.target, rule, L, s);
  };
  return a.rule == RSA_ROWS_ADAGRAD ? apply(adagrad_of(a)) : apply(adam_of(a));
}

extern "C" int rsa_sort_step_elements(const rsa_rows_update_args* args, rsa_stream_t stream) {
  rsa_rows_update_args a;
  if (int rc = load_args(a, args, "rsa_sort_step_elements")) return rc;
  return sort_step_elements(a, a.solo, (hipStream_t)stream, "rsa_sort_step_elements");
}

extern "C" int rsa_rows_update_presorted(const rsa_rows_update_args* args, rsa_stream_t stream) {
  rsa_rows_update_args a;
  if (int rc = load_args(a, args, "rsa_rows_update_presorted")) return rc;
  if (int rc = check_rule(a, "rsa_rows_update_presorted")) return rc;
  return apply_step_elements(a, a.has_pos != 0, (hipStream_t)stream);
}

extern "C" int rsa_rows_update_sorted(const rsa_rows_update_args* args, rsa_stream_t stream) {
  rsa_rows_update_args a;
  if (int rc = load_args(a, args, "rsa_rows_update_sorted")) return rc;
  if (int rc = check_rule(a, "rsa_rows_update_sorted")) return rc;
  RSA_CHECK_ARG(a.pos_ids == nullptr || a.dpos != nullptr, "rsa_rows_update_sorted: pos_ids without dpos");
  if (a.dim != 64 && a.dim != 128 && a.dim != 256) {      // before the sort is issued
    rsa::set_error("rsa_rows_update_sorted: dim=%d: built for dim in {64, 128, 256}", a.dim);
    return RSA_ERR_UNSUPPORTED;
  }
  if (int rc = sort_step_elements(a, nullptr, (hipStream_t)stream, "rsa_rows_update_sorted")) return rc;
  return apply_step_elements(a, a.pos_ids != nullptr, (hipStream_t)stream);
}
