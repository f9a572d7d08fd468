// NCF's pair scorers, fused (gfx950): MLPScorer and FusionMFMLPScorer over (query, item id) pairs, forward and backward.
//
// rsa_pair_mlp / rsa_pair_mlp_backward : recstudio/model/scorer.py:37-56 (MLPScorer), :92-113 (FusionMFMLPScorer) over
//                                        MLPModule (recstudio/model/module/layers.py:150-222), as NCF builds them (mf/ncf.py)
//
//   pair m = (b, slot), id i = ids[b, slot] (or c0 + slot in RANGE mode), u = query[b], x = table[i]
//   in  = [u | x] * keep0 / q                                    (2d columns)
//   h1  = relu(W1 in + b1),  h2 = relu(W2 (h1 * keep1 / q) + b2) (one or two hidden layers, K = 1 or 2)
//   fusion : s = relu(w_mf . (u * x) + w_h . h_K)                (no bias; h_K and u * x are not dropped)
//   mlp    : s = relu(w_h . (h_K * keep_K / q) + b_out)
//
// TILE.  A wave owns 32 pairs and all columns of them; a workgroup is four such waves that share nothing but the weights, and
// strides over the pair tiles.  Every product runs on v_mfma_f32_32x32x2_f32, taken TRANSPOSED as in rsa_combine.hip: the weight
// matrix is the A operand (M = output column), the pairs are the B operand (N = pair), so lane (j, hh) ends up with pair j of the
// tile in its registers, column 32 cb + row32(r, hh) in register r of accumulator block cb.  Bias, ReLU, the mask, the operand
// of the next layer and the final dot product never leave the lane: register r of block cb is, as it stands, the B operand of
// K step (cb, r) of the next product (the two halves hh supply the two columns of the K pair), and the score needs one shuffle
// across the halves.  Neither [M, 2d] nor any [M, H] exists in memory: a pair costs its 8-byte id, 4 d bytes of the item row and
// 4 bytes of score.
//
// LOADS.  u and x are read in 16-byte pieces straight from the query matrix and the embedding table (lane (j, hh) reads the
// pieces at columns 8 t + 4 hh of its pair's two rows; one trip of the K loop feeds the u half AND the x half of W1, which is
// also where u * x of the fusion term comes from).  Consecutive slots of one query sit in neighbouring lanes and ask for the
// same 16 bytes of u: they share the cache line in the load unit, nothing is staged for it.  All offsets are 64-bit.  An id is
// clamped into the table: a bad id reads a wrong row, never another allocation.
//
// WEIGHTS IN LDS.  W1 [H1, 2d] at a row stride of 2d + 4 floats, W2 [H2, H1] at H1 + 4, then b1, b2, w_mf, w_h, b_out: staged
// once per workgroup.  "Lane j reads 16 bytes of row j" with a stride that is 4 mod 8 floats is conflict-free (rsa_combine.hip);
// the backward's W^T products read W[c][32 kb + j], 32 consecutive floats per half-wave.  d = 64, [128, 64]: 102 KB of the
// 160 KB, so one workgroup (four waves) per CU; every (d, hidden) in {32, 64, 128} whose padded matrices fit is accepted and the
// host check names the limit (at d = 128 a first layer of 128 fits alone or with a second of 32 -- 135 and 152 KB --, not with
// 64 or 128).  Registers: forward 16 H1 / 32 + 16 H2 / 32 accumulators (96 at the default, no scratch) -- h1 is overwritten in
// place.  The backward keeps h and dpre of both layers (192) and, in the weights pass, 8 blocks of dW (128) next to the operands
// the unrolled products hold: both backward kernels compile to all 512 registers of one wave per SIMD (which the LDS footprint
// allows anyway) and spill -- at the default shape 0.6 KB per lane in the rows pass and 2.1 KB in the weights pass, up to 1.3 and
// 3.3 KB at [128, 128] -- a cost in time only.
//
// DROPOUT.  q = fp32(1 - p).  Element (m, c) is kept iff u[m C + c] < q and is then DIVIDED by q; u = that element of ONE
// torch.rand([M, C]) call (torch_rand_element), C = the masked columns in layer order: 2d, H1 when something follows it (always in
// mlp mode), H2 in mlp mode.  p = 0 draws nothing.  The mask follows torch.rand, not nn.Dropout's kernel (as rsa_combine.hip).
//
// BACKWARD.  Nothing is saved: both passes recompute the layers and regenerate the mask (kept as bits: 64 per layer and lane).
//   rows pass     g = upstream * (s > 0) (0 for a masked positive), dpre_K = g w_h gate_K, dh1 = W2^T dpre2, din = W1^T dpre1 --
//                 all as transposed products, so the ReLU / mask gates apply inside the lane and din leaves in 16-byte pieces: the
//                 u half (+ g w_mf x) per PAIR into the workspace, the x half (+ g w_mf u) as the per-slot item row [M, d]
//                 (the caller's row scatter drops the padding row).  pm_dq_kernel then adds the slots of a query in ascending order into dq [B, d].
//   weights pass  dW contracts over PAIRS, which needs the operands with the column on the lane and the pairs in the registers.
//                 A 32 x 32 block held in the accumulator layout is moved there THROUGH THE MATRIX UNIT (16 MFMAs against the
//                 identity: exact).  blockIdx.y picks one block of 32 output columns of W1 or W2; a wave recomputes the pair
//                 tile, transposes that dpre block and every block of the layer's masked input, and keeps dW [32, fan-in] in
//                 accumulators over all its tiles; db, dw_h, dw_mf and db_out are sums over the registers of such transposed
//                 blocks.  Every wave leaves its sums in its own slot of the workspace.
//   reduce        one thread per parameter adds the slots in ascending order.  No float atomics: two runs are bit-equal.
// flops per pair: forward 2 (2d H1 + H1 H2); rows pass 2x that again; weights pass (H1 + H2) / 32 recomputations + the dW products.
#include <utility>

#include "rsa_lds.hpp"

namespace rsa {

using f32x16 = float __attribute__((ext_vector_type(16)));

constexpr int PM_WEIGHT_GROUPS = 96;         // workgroups per column block of the weights pass: 4 * 96 partial slots at most
constexpr int PM_MAX_KB = 8;                 // blocks of 32 input columns of a layer: 2d / 32 <= 8

extern __shared__ __attribute__((aligned(16))) float pm_smem[];

struct PmParams {
  const float *query, *table;
  const int64_t* ids;
  int64_t n_query, n_slots, n_items, c0, n_pairs, n_tiles;
  int d, h1, h2, hk, mode, mask_slot0, drop, drop_k;   // hk: width of the last hidden layer; drop_k: h_K is masked (mlp mode)
  int ld1, ld2, ctot;                                  // LDS row strides of W1, W2; masked columns per pair
  const float *w1, *b1, *w2, *b2, *w_mf, *w_h, *b_out;
  float q;
  PhiloxCall pc;
  float* scores;
  const float* g;
  float *dqp, *dq, *drows, *dparams, *pw;
  int64_t n_params, o_w2, o_b1, o_b2, o_wh, o_wmf, o_bout;   // layout of dparams and of a partial slot (o_w1 = 0)
  int n_wslots;
};

struct PmSmem {
  float *w1, *w2, *b1, *b2, *wmf, *wh, *bout;
};

template <class F, int... I>
__device__ __forceinline__ void pm_each(F&& f, std::integer_sequence<int, I...>) {
  (f(std::integral_constant<int, I>{}), ...);
}
// f(integral_constant<int, 0>) ... f(integral_constant<int, N - 1>): separate pieces of code per accumulator block (rsa_combine.hip)
template <int N, class F>
__device__ __forceinline__ void pm_blocks(F&& f) {
  pm_each(static_cast<F&&>(f), std::make_integer_sequence<int, N>{});
}

__device__ __forceinline__ int pm_row32(int r, int hh) { return (r & 3) + 8 * (r >> 2) + 4 * hh; }
__device__ __forceinline__ f32x16 pm_zero() { return f32x16{0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}; }

static inline int64_t pm_lds_floats(int d, int h1, int h2) {
  const int hk = h2 ? h2 : h1;
  return (int64_t)h1 * (2 * d + 4) + (int64_t)h2 * (h1 + 4) + h1 + h2 + d + hk + 4;
}

__device__ __forceinline__ PmSmem pm_carve(const PmParams& p) {
  PmSmem s;
  s.w1 = pm_smem;
  s.w2 = s.w1 + p.h1 * p.ld1;
  s.b1 = s.w2 + p.h2 * p.ld2;
  s.b2 = s.b1 + p.h1;
  s.wmf = s.b2 + p.h2;
  s.wh = s.wmf + p.d;
  s.bout = s.wh + p.hk;
  return s;
}

// every weight into LDS (the 4 padding floats of a matrix row are never read); ends with a barrier
__device__ __forceinline__ void pm_stage(const PmParams& p, const PmSmem& s) {
  const int k1 = (2 * p.d) >> 2, k2 = p.h1 >> 2;
  for (int i = threadIdx.x; i < p.h1 * k1; i += blockDim.x) {
    const int r = i / k1, k = (i - r * k1) * 4;
    *reinterpret_cast<float4*>(s.w1 + r * p.ld1 + k) = *reinterpret_cast<const float4*>(p.w1 + (int64_t)r * 2 * p.d + k);
  }
  for (int i = threadIdx.x; i < p.h2 * k2; i += blockDim.x) {
    const int r = i / k2, k = (i - r * k2) * 4;
    *reinterpret_cast<float4*>(s.w2 + r * p.ld2 + k) = *reinterpret_cast<const float4*>(p.w2 + (int64_t)r * p.h1 + k);
  }
  for (int i = threadIdx.x; i < p.h1; i += blockDim.x) s.b1[i] = p.b1[i];
  for (int i = threadIdx.x; i < p.h2; i += blockDim.x) s.b2[i] = p.b2[i];
  for (int i = threadIdx.x; i < p.d; i += blockDim.x) s.wmf[i] = p.mode == 0 ? p.w_mf[i] : 0.f;
  for (int i = threadIdx.x; i < p.hk; i += blockDim.x) s.wh[i] = p.w_h[i];
  if (threadIdx.x == 0) s.bout[0] = p.mode == 1 ? p.b_out[0] : 0.f;
  __syncthreads();
}

// What a lane knows of its pair.
struct PmPair {
  int64_t m, id;               // pair index (clamped to one that exists), item id (clamped into the table)
  const float *ur, *xr;
  bool ok, masked;             // the pair exists; it is a positive with id 0 (scores -inf, passes no gradient)
};

__device__ __forceinline__ PmPair pm_pair(const PmParams& p, int64_t row0, int j) {
  PmPair pr;
  const int64_t m = row0 + j;
  pr.ok = m < p.n_pairs;
  pr.m = pr.ok ? m : p.n_pairs - 1;
  const int64_t b = pr.m / p.n_slots, slot = pr.m - b * p.n_slots;
  int64_t id = p.ids ? p.ids[pr.m] : p.c0 + slot;
  id = id < 0 ? 0 : (id >= p.n_items ? p.n_items - 1 : id);
  pr.id = id;
  pr.masked = p.mask_slot0 && slot == 0 && id == 0;
  pr.ur = p.query + b * (int64_t)p.d;
  pr.xr = p.table + id * (int64_t)p.d;
  return pr;
}

__device__ __forceinline__ bool pm_keep(const PmParams& p, int64_t m, int col) {
  return torch_rand_element(p.pc, (uint64_t)m * (uint64_t)p.ctot + (uint64_t)col) < p.q;
}

// The four input elements at columns k0 .. k0 + 3 of the u half (part 0) or the x half (part 1), masked; the mask bits of the lane
// are kept at (k0 >> 3) * 4 + i of keep[part] (a lane owns the pieces at k0 = 8 t + 4 hh: at most 64 elements per half).
template <bool RECORD>
__device__ __forceinline__ void pm_mask4(const PmParams& p, const PmPair& pr, int part, int k0, float (&v)[4], uint64_t (&keep)[2]) {
  if (!p.drop) return;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int bit = (k0 >> 3) * 4 + i;
    bool kept;
    if constexpr (RECORD) {
      kept = pm_keep(p, pr.m, part * p.d + k0 + i);
      if (kept) keep[part] |= 1ull << bit;
    } else {
      kept = (keep[part] >> bit) & 1;
    }
    v[i] = kept ? v[i] / p.q : 0.f;
  }
}

// bias, ReLU and mask of one layer's accumulators, in place: acc <- the layer's output as the next product reads it.
// gate: bit cb * 16 + r set where the output passes a gradient (pre-activation > 0 and kept).
template <int NCB>
__device__ __forceinline__ void pm_activate(const PmParams& p, const PmPair& pr, const float* bias, int col0, bool masked, int hh,
                                            f32x16 (&acc)[NCB], uint64_t& gate) {
  gate = 0;
  pm_blocks<NCB>([&](auto CB) {
    constexpr int cb = decltype(CB)::value;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int c = cb * 32 + pm_row32(r, hh);
      const float pre = acc[cb][r] + bias[c];
      bool on = pre > 0.f;
      float hv = on ? pre : 0.f;
      if (masked) {
        const bool kept = pm_keep(p, pr.m, col0 + c);
        hv = kept ? hv / p.q : 0.f;
        on = on && kept;
      }
      if (on) gate |= 1ull << (cb * 16 + r);
      acc[cb][r] = hv;
    }
  });
}

// The layers of one pair tile.  a1 / a2: the outputs of layer 1 / 2 as the next product reads them (masked where the rule masks
// them); keep0: the input mask; gate1 / gate2; returns the score's pre-activation z (both halves of a pair hold it).
template <int NCB1, int NCB2>
__device__ __forceinline__ float pm_layers(const PmParams& p, const PmSmem& s, const PmPair& pr, int lane, f32x16 (&a1)[NCB1],
                                           f32x16 (&a2)[NCB2 ? NCB2 : 1], uint64_t (&keep0)[2], uint64_t& gate1, uint64_t& gate2) {
  const int j = lane & 31, hh = lane >> 5;
#pragma unroll
  for (int cb = 0; cb < NCB1; ++cb) a1[cb] = pm_zero();
  keep0[0] = keep0[1] = 0;
  float dot = 0.f;
  for (int k0 = 4 * hh; k0 < p.d; k0 += 8) {
    const float4 u4 = *reinterpret_cast<const float4*>(pr.ur + k0);
    const float4 x4 = *reinterpret_cast<const float4*>(pr.xr + k0);
    float uv[4] = {u4.x, u4.y, u4.z, u4.w}, xv[4] = {x4.x, x4.y, x4.z, x4.w};
    const float4 m4 = *reinterpret_cast<const float4*>(s.wmf + k0);        // (zeros in mlp mode)
    dot += m4.x * (uv[0] * xv[0]) + m4.y * (uv[1] * xv[1]) + m4.z * (uv[2] * xv[2]) + m4.w * (uv[3] * xv[3]);
    pm_mask4<true>(p, pr, 0, k0, uv, keep0);
    pm_mask4<true>(p, pr, 1, k0, xv, keep0);
#pragma unroll
    for (int cb = 0; cb < NCB1; ++cb) {
      const float4 wa = *reinterpret_cast<const float4*>(s.w1 + (cb * 32 + j) * p.ld1 + k0);
      const float4 wb = *reinterpret_cast<const float4*>(s.w1 + (cb * 32 + j) * p.ld1 + p.d + k0);
      const float wu[4] = {wa.x, wa.y, wa.z, wa.w}, wx[4] = {wb.x, wb.y, wb.z, wb.w};
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        a1[cb] = __builtin_amdgcn_mfma_f32_32x32x2f32(wu[i], uv[i], a1[cb], 0, 0, 0);
        a1[cb] = __builtin_amdgcn_mfma_f32_32x32x2f32(wx[i], xv[i], a1[cb], 0, 0, 0);
      }
    }
  }
  pm_activate<NCB1>(p, pr, s.b1, 2 * p.d, p.drop && (NCB2 > 0 || p.drop_k), hh, a1, gate1);
  gate2 = 0;
  if constexpr (NCB2 > 0) {
#pragma unroll
    for (int cb = 0; cb < NCB2; ++cb) a2[cb] = pm_zero();
#pragma unroll
    for (int c1 = 0; c1 < NCB1; ++c1)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int k0 = c1 * 32 + 8 * g + 4 * hh;
#pragma unroll
        for (int cb = 0; cb < NCB2; ++cb) {
          const float4 w4 = *reinterpret_cast<const float4*>(s.w2 + (cb * 32 + j) * p.ld2 + k0);
          const float wv[4] = {w4.x, w4.y, w4.z, w4.w};
#pragma unroll
          for (int i = 0; i < 4; ++i) a2[cb] = __builtin_amdgcn_mfma_f32_32x32x2f32(wv[i], a1[c1][4 * g + i], a2[cb], 0, 0, 0);
        }
      }
    pm_activate<NCB2>(p, pr, s.b2, 2 * p.d + p.h1, p.drop && p.drop_k, hh, a2, gate2);
#pragma unroll
    for (int cb = 0; cb < NCB2; ++cb)
#pragma unroll
      for (int r = 0; r < 16; ++r) dot += s.wh[cb * 32 + pm_row32(r, hh)] * a2[cb][r];
  } else {
#pragma unroll
    for (int cb = 0; cb < NCB1; ++cb)
#pragma unroll
      for (int r = 0; r < 16; ++r) dot += s.wh[cb * 32 + pm_row32(r, hh)] * a1[cb][r];
  }
  dot += __shfl_xor(dot, 32, 64);
  return dot + s.bout[0];
}

template <int NCB1, int NCB2>
__global__ __launch_bounds__(256) void pm_forward_kernel(const PmParams p) {
  const PmSmem s = pm_carve(p);
  pm_stage(p, s);
  const int lane = lane_id(), wave = threadIdx.x >> 6, j = lane & 31, hh = lane >> 5;
  for (int64_t tile = (int64_t)blockIdx.x * 4 + wave; tile < p.n_tiles; tile += (int64_t)gridDim.x * 4) {
    const PmPair pr = pm_pair(p, tile * 32, j);
    f32x16 a1[NCB1], a2[NCB2 ? NCB2 : 1];
    uint64_t keep0[2], gate1, gate2;
    const float z = pm_layers<NCB1, NCB2>(p, s, pr, lane, a1, a2, keep0, gate1, gate2);
    if (pr.ok && hh == 0) p.scores[pr.m] = pr.masked ? -INFINITY : (z > 0.f ? z : 0.f);
  }
}

// The gradients of both layers' pre-activations, in the forward's layout: d1 / d2 (d2 only with two layers).  Returns g, the
// gradient at the score's pre-activation.
template <int NCB1, int NCB2>
__device__ __forceinline__ float pm_dpre(const PmParams& p, const PmSmem& s, const PmPair& pr, int lane, float z, uint64_t gate1,
                                         uint64_t gate2, f32x16 (&d1)[NCB1], f32x16 (&d2)[NCB2 ? NCB2 : 1]) {
  const int j = lane & 31, hh = lane >> 5;
  const float g = (pr.ok && !pr.masked && z > 0.f) ? p.g[pr.m] : 0.f;
  const bool scale_k = p.drop && p.drop_k;
  if constexpr (NCB2 > 0) {
#pragma unroll
    for (int cb = 0; cb < NCB2; ++cb)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        float v = g * s.wh[cb * 32 + pm_row32(r, hh)];
        if (scale_k) v = v / p.q;
        d2[cb][r] = ((gate2 >> (cb * 16 + r)) & 1) ? v : 0.f;
      }
#pragma unroll
    for (int c1 = 0; c1 < NCB1; ++c1) {
      f32x16 acc = pm_zero();
#pragma unroll
      for (int cb = 0; cb < NCB2; ++cb)
#pragma unroll
        for (int r = 0; r < 16; ++r)
          acc = __builtin_amdgcn_mfma_f32_32x32x2f32(s.w2[(cb * 32 + pm_row32(r, hh)) * p.ld2 + c1 * 32 + j], d2[cb][r], acc, 0, 0, 0);
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        float v = acc[r];
        if (p.drop) v = v / p.q;
        d1[c1][r] = ((gate1 >> (c1 * 16 + r)) & 1) ? v : 0.f;
      }
    }
  } else {
#pragma unroll
    for (int cb = 0; cb < NCB1; ++cb)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        float v = g * s.wh[cb * 32 + pm_row32(r, hh)];
        if (scale_k) v = v / p.q;
        d1[cb][r] = ((gate1 >> (cb * 16 + r)) & 1) ? v : 0.f;
      }
  }
  return g;
}

template <int NCB1, int NCB2>
__global__ __launch_bounds__(256) void pm_rows_kernel(const PmParams p) {
  const PmSmem s = pm_carve(p);
  pm_stage(p, s);
  const int lane = lane_id(), wave = threadIdx.x >> 6, j = lane & 31, hh = lane >> 5;
  for (int64_t tile = (int64_t)blockIdx.x * 4 + wave; tile < p.n_tiles; tile += (int64_t)gridDim.x * 4) {
    const PmPair pr = pm_pair(p, tile * 32, j);
    f32x16 a1[NCB1], a2[NCB2 ? NCB2 : 1], d1[NCB1], d2[NCB2 ? NCB2 : 1];
    uint64_t keep0[2], gate1, gate2;
    const float z = pm_layers<NCB1, NCB2>(p, s, pr, lane, a1, a2, keep0, gate1, gate2);
    const float g = pm_dpre<NCB1, NCB2>(p, s, pr, lane, z, gate1, gate2, d1, d2);
    // ---- din = W1^T dpre1, one block of 32 input columns at a time; columns [0, d) are du, [d, 2d) are dx
    for (int kb = 0; kb < (2 * p.d) / 32; ++kb) {
      f32x16 acc = pm_zero();
#pragma unroll
      for (int cb = 0; cb < NCB1; ++cb)
#pragma unroll
        for (int r = 0; r < 16; ++r)
          acc = __builtin_amdgcn_mfma_f32_32x32x2f32(s.w1[(cb * 32 + pm_row32(r, hh)) * p.ld1 + kb * 32 + j], d1[cb][r], acc, 0, 0, 0);
      const int part = kb * 32 >= p.d;
#pragma unroll
      for (int g4 = 0; g4 < 4; ++g4) {
        const int k0 = kb * 32 - part * p.d + 8 * g4 + 4 * hh;            // column inside the half
        float v[4] = {acc[4 * g4], acc[4 * g4 + 1], acc[4 * g4 + 2], acc[4 * g4 + 3]};
        pm_mask4<false>(p, pr, part, k0, v, keep0);
        if (p.mode == 0) {                                                 // the u * x term of the fusion scorer
          const float4 o4 = *reinterpret_cast<const float4*>((part ? pr.ur : pr.xr) + k0);
          const float4 m4 = *reinterpret_cast<const float4*>(s.wmf + k0);
          v[0] += g * m4.x * o4.x, v[1] += g * m4.y * o4.y, v[2] += g * m4.z * o4.z, v[3] += g * m4.w * o4.w;
        }
        if (pr.ok) {
          *reinterpret_cast<float4*>((part ? p.drows : p.dqp) + pr.m * (int64_t)p.d + k0) = make_float4(v[0], v[1], v[2], v[3]);
        }
      }
    }
  }
}

// dq[b] = the per-pair du of the slots of b, added in ascending slot order; one thread per 16 bytes of dq
__global__ __launch_bounds__(256) void pm_dq_kernel(const PmParams p) {
  const int64_t tid = (int64_t)blockIdx.x * 256 + threadIdx.x, d4 = p.d >> 2;
  if (tid >= p.n_query * d4) return;
  const int64_t b = tid / d4, k = (tid - b * d4) * 4;
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int64_t sl = 0; sl < p.n_slots; ++sl) {
    const float4 v = *reinterpret_cast<const float4*>(p.dqp + (b * p.n_slots + sl) * p.d + k);
    acc.x += v.x, acc.y += v.y, acc.z += v.z, acc.w += v.w;
  }
  *reinterpret_cast<float4*>(p.dq + b * p.d + k) = acc;
}

// A 32 x 32 block from the accumulator layout (lane = pair j, register r = column row32(r, hh)) to lane = column j, register r =
// pair row32(r, hh): the product with the identity, exact.
__device__ __forceinline__ f32x16 pm_transpose(const f32x16& v, int j, int hh) {
  f32x16 o = pm_zero();
#pragma unroll
  for (int r = 0; r < 16; ++r) o = __builtin_amdgcn_mfma_f32_32x32x2f32(v[r], j == pm_row32(r, hh) ? 1.f : 0.f, o, 0, 0, 0);
  return o;
}

__device__ __forceinline__ float pm_regsum(const f32x16& t) {
  float sum = 0.f;
#pragma unroll
  for (int r = 0; r < 16; ++r) sum += t[r];
  return sum + __shfl_xor(sum, 32, 64);
}

// dW [32, 32 nkb] += dpre block^T (already transposed: dt) x the layer's input blocks; in_block(kb) returns block kb of the input in the
// accumulator layout
template <class F>
__device__ __forceinline__ void pm_dw_accumulate(const f32x16& dt, int nkb, int j, int hh, f32x16 (&dw)[PM_MAX_KB], F&& in_block) {
#pragma unroll
  for (int kb = 0; kb < PM_MAX_KB; ++kb) {
    if (kb < nkb) {
      const f32x16 it = pm_transpose(in_block(kb), j, hh);
#pragma unroll
      for (int t = 0; t < 16; ++t) dw[kb] = __builtin_amdgcn_mfma_f32_32x32x2f32(dt[t], it[t], dw[kb], 0, 0, 0);
    }
  }
}

template <int NCB1, int NCB2>
__global__ __launch_bounds__(256) void pm_weights_kernel(const PmParams p) {
  const PmSmem s = pm_carve(p);
  pm_stage(p, s);
  const int lane = lane_id(), wave = threadIdx.x >> 6, j = lane & 31, hh = lane >> 5;
  const int y = blockIdx.y;                       // [0, NCB1): a column block of W1; then the column blocks of W2
  const bool last1 = NCB2 == 0;                   // layer 1 is the last hidden layer
  f32x16 dw[PM_MAX_KB];
#pragma unroll
  for (int kb = 0; kb < PM_MAX_KB; ++kb) dw[kb] = pm_zero();
  float dmf[4] = {0.f, 0.f, 0.f, 0.f};             // dw_mf of column 32 kb + j (y == 0 only)
  float db = 0.f, dwh = 0.f, dbout = 0.f;
  for (int64_t tile = (int64_t)blockIdx.x * 4 + wave; tile < p.n_tiles; tile += (int64_t)gridDim.x * 4) {
    const PmPair pr = pm_pair(p, tile * 32, j);
    f32x16 a1[NCB1], a2[NCB2 ? NCB2 : 1], d1[NCB1], d2[NCB2 ? NCB2 : 1];
    uint64_t keep0[2], gate1, gate2;
    const float z = pm_layers<NCB1, NCB2>(p, s, pr, lane, a1, a2, keep0, gate1, gate2);
    const float g = pm_dpre<NCB1, NCB2>(p, s, pr, lane, z, gate1, gate2, d1, d2);
    if (y < NCB1) {
      pm_blocks<NCB1>([&](auto CB) {
        constexpr int cb = decltype(CB)::value;
        if (cb != y) return;
        const f32x16 dt = pm_transpose(d1[cb], j, hh);
        db += pm_regsum(dt);
        if (last1) {
          f32x16 gh;
#pragma unroll
          for (int r = 0; r < 16; ++r) gh[r] = g * a1[cb][r];
          dwh += pm_regsum(pm_transpose(gh, j, hh));
        }
        pm_dw_accumulate(dt, (2 * p.d) / 32, j, hh, dw, [&](int kb) {
          const int part = kb * 32 >= p.d;
          f32x16 blk;
#pragma unroll
          for (int g4 = 0; g4 < 4; ++g4) {
            const int k0 = kb * 32 - part * p.d + 8 * g4 + 4 * hh;
            const float4 v4 = *reinterpret_cast<const float4*>((part ? pr.xr : pr.ur) + k0);
            float v[4] = {v4.x, v4.y, v4.z, v4.w};
            pm_mask4<false>(p, pr, part, k0, v, keep0);
            blk[4 * g4] = v[0], blk[4 * g4 + 1] = v[1], blk[4 * g4 + 2] = v[2], blk[4 * g4 + 3] = v[3];
          }
          return blk;
        });
      });
    }
    if constexpr (NCB2 > 0) {
      if (y >= NCB1) {
        pm_blocks<NCB2>([&](auto CB) {
          constexpr int cb = decltype(CB)::value;
          if (cb != y - NCB1) return;
          const f32x16 dt = pm_transpose(d2[cb], j, hh);
          db += pm_regsum(dt);
          f32x16 gh;
#pragma unroll
          for (int r = 0; r < 16; ++r) gh[r] = g * a2[cb][r];
          dwh += pm_regsum(pm_transpose(gh, j, hh));
          // (kb is a literal after unrolling: a1 is indexed statically)
#pragma unroll
          for (int kb = 0; kb < NCB1; ++kb) {
            const f32x16 it = pm_transpose(a1[kb], j, hh);
#pragma unroll
            for (int t = 0; t < 16; ++t) dw[kb] = __builtin_amdgcn_mfma_f32_32x32x2f32(dt[t], it[t], dw[kb], 0, 0, 0);
          }
        });
      }
    }
    if (y == 0) {
      if (hh == 0) dbout += g;
      if (p.mode == 0) {
#pragma unroll
        for (int kb = 0; kb < 4; ++kb) {
          if (kb * 32 < p.d) {
            f32x16 blk;
#pragma unroll
            for (int g4 = 0; g4 < 4; ++g4) {
              const int k0 = kb * 32 + 8 * g4 + 4 * hh;
              const float4 u4 = *reinterpret_cast<const float4*>(pr.ur + k0);
              const float4 x4 = *reinterpret_cast<const float4*>(pr.xr + k0);
              blk[4 * g4] = g * (u4.x * x4.x), blk[4 * g4 + 1] = g * (u4.y * x4.y);
              blk[4 * g4 + 2] = g * (u4.z * x4.z), blk[4 * g4 + 3] = g * (u4.w * x4.w);
            }
            dmf[kb] += pm_regsum(pm_transpose(blk, j, hh));
          }
        }
      }
    }
  }
  // ---- the wave's partial sums, in its own slot (a wave without a tile writes zeros)
  float* slot = p.pw + ((int64_t)blockIdx.x * 4 + wave) * p.n_params;
  const bool first = y < NCB1;
  const int cbk = first ? y : y - NCB1, fan = first ? 2 * p.d : p.h1;
  float* w = slot + (first ? 0 : p.o_w2);
#pragma unroll
  for (int kb = 0; kb < PM_MAX_KB; ++kb)
    if (kb * 32 < fan) {
#pragma unroll
      for (int r = 0; r < 16; ++r) w[(int64_t)(cbk * 32 + pm_row32(r, hh)) * fan + kb * 32 + j] = dw[kb][r];
    }
  if (hh == 0) {
    slot[(first ? p.o_b1 : p.o_b2) + cbk * 32 + j] = db;
    if (first == last1) slot[p.o_wh + cbk * 32 + j] = dwh;
  }
  if (y == 0) {
    if (p.mode == 0) {
#pragma unroll
      for (int kb = 0; kb < 4; ++kb)
        if (kb * 32 < p.d) {
          if (hh == 0) slot[p.o_wmf + kb * 32 + j] = dmf[kb];
        }
    } else {
#pragma unroll
      for (int m = 32; m >= 1; m >>= 1) dbout += __shfl_xor(dbout, m, 64);
      if (lane == 0) slot[p.o_bout] = dbout;
    }
  }
}

// One thread per parameter: the slots added in ascending order, eight loads in flight.
__global__ __launch_bounds__(256) void pm_reduce_kernel(const PmParams p) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= p.n_params) return;
  const float* src = p.pw + e;
  float acc = 0.f;
  for (int sl = 0; sl < p.n_wslots; sl += 8) {
    float v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = src[(int64_t)(sl + u < p.n_wslots ? sl + u : p.n_wslots - 1) * p.n_params];
#pragma unroll
    for (int u = 0; u < 8; ++u) acc += sl + u < p.n_wslots ? v[u] : 0.f;
  }
  p.dparams[e] = acc;
}

static inline int64_t pm_tiles(int64_t n_pairs) { return (n_pairs + 31) / 32; }
static inline bool pm_width_ok(int v) { return v == 32 || v == 64 || v == 128; }

// dparams and every partial slot: W1 [h1, 2d], W2 [h2, h1], b1, b2, w_h [hk], then w_mf [d] (fusion) or b_out [1] (mlp)
static inline void pm_param_layout(PmParams& p) {
  p.o_w2 = (int64_t)p.h1 * 2 * p.d;
  p.o_b1 = p.o_w2 + (int64_t)p.h2 * p.h1;
  p.o_b2 = p.o_b1 + p.h1;
  p.o_wh = p.o_b2 + p.h2;
  p.o_wmf = p.o_bout = p.o_wh + p.hk;
  p.n_params = p.o_wmf + (p.mode == 0 ? p.d : 1);
}

struct PmLayout {
  float *dqp, *pw;
  unsigned groups;
};

static inline PmLayout pm_layout(Carver& cv, int64_t n_pairs, int d, int h1, int h2) {
  PmLayout L;
  const int hk = h2 ? h2 : h1;
  const int64_t n_params = (int64_t)h1 * 2 * d + (int64_t)h2 * h1 + h1 + h2 + hk + d;      // (the larger of the two modes)
  L.groups = grid_1d(pm_tiles(n_pairs), 4, PM_WEIGHT_GROUPS);
  L.dqp = cv.take<float>(n_pairs * d);
  L.pw = cv.take<float>((int64_t)L.groups * 4 * n_params);
  return L;
}

static int pm_check(const rsa_pair_mlp_args& a, const char* fn, PmParams& p) {
  RSA_CHECK_ARG(a.n_query >= 0 && a.n_slots >= 0 && a.n_items >= 1, "%s: bad sizes (n_query %lld, n_slots %lld, n_items %lld)", fn,
                (long long)a.n_query, (long long)a.n_slots, (long long)a.n_items);
  RSA_CHECK_ARG(pm_width_ok(a.d) && pm_width_ok(a.h1) && (a.h2 == 0 || pm_width_ok(a.h2)),
                "%s: d and the hidden widths must be 32, 64 or 128 (one or two hidden layers), got d %d, hidden %d, %d", fn, a.d, a.h1, a.h2);
  RSA_CHECK_ARG(pm_lds_floats(a.d, a.h1, a.h2) * 4 <= LDS_LIMIT,
                "%s: d %d, hidden %d, %d: the padded weights are kept in LDS and need %lld bytes of %lld", fn, a.d, a.h1, a.h2,
                (long long)(pm_lds_floats(a.d, a.h1, a.h2) * 4), (long long)LDS_LIMIT);
  RSA_CHECK_ARG(a.mode == 0 || a.mode == 1, "%s: mode must be 0 (fusion) or 1 (mlp), got %d", fn, a.mode);
  RSA_CHECK_ARG(a.p >= 0.0 && a.p < 1.0, "%s: the dropout probability must lie in [0, 1), got %g", fn, a.p);
  RSA_CHECK_ARG(a.p == 0.0 || (a.grid_threads > 0 && a.grid_threads % 256 == 0 && (a.offset & 3) == 0),
                "%s: bad philox state for the dropout (grid_threads %u must be a positive multiple of 256, offset a multiple of 4)",
                fn, a.grid_threads);
  RSA_CHECK_ARG(a.ids != nullptr || (a.c0 >= 0 && a.c0 + a.n_slots <= a.n_items),
                "%s: range mode [%lld, %lld) leaves the table of %lld rows", fn, (long long)a.c0, (long long)(a.c0 + a.n_slots),
                (long long)a.n_items);
  if (a.n_query == 0 || a.n_slots == 0) return RSA_OK;
  RSA_CHECK_ARG(a.query && a.table && a.w1 && a.b1 && a.w_h, "%s: query, table, w1, b1 or w_h is null", fn);
  RSA_CHECK_ARG(a.h2 == 0 || (a.w2 && a.b2), "%s: two hidden layers need w2 and b2", fn);
  RSA_CHECK_ARG(a.mode == 0 ? a.w_mf != nullptr : a.b_out != nullptr, "%s: fusion mode needs w_mf, mlp mode b_out", fn);
  RSA_CHECK_ARG((((uintptr_t)a.query | (uintptr_t)a.table | (uintptr_t)a.w1 | (uintptr_t)a.w2) & 15) == 0,
                "%s: query, table, w1 and w2 must be 16-byte aligned", fn);
  RSA_CHECK_ARG(a.n_query <= (1ll << 40) / a.n_slots && pm_tiles(a.n_query * a.n_slots) < (1ll << 31), "%s: too many pairs for one launch", fn);
  p.query = a.query, p.table = a.table, p.ids = a.ids;
  p.n_query = a.n_query, p.n_slots = a.n_slots, p.n_items = a.n_items, p.c0 = a.c0;
  p.n_pairs = a.n_query * a.n_slots, p.n_tiles = pm_tiles(p.n_pairs);
  p.d = a.d, p.h1 = a.h1, p.h2 = a.h2, p.hk = a.h2 ? a.h2 : a.h1, p.mode = a.mode, p.mask_slot0 = a.mask_slot0 != 0;
  p.drop = a.p != 0.0, p.drop_k = a.mode == 1;
  p.ld1 = 2 * a.d + 4, p.ld2 = a.h1 + 4;
  p.ctot = 2 * a.d + ((a.h2 || a.mode == 1) ? a.h1 : 0) + (a.mode == 1 ? a.h2 : 0);
  p.w1 = a.w1, p.b1 = a.b1, p.w2 = a.w2, p.b2 = a.b2, p.w_mf = a.w_mf, p.w_h = a.w_h, p.b_out = a.b_out;
  p.q = (float)(1.0 - a.p);
  p.pc = PhiloxCall{a.seed, a.offset >> 2, a.grid_threads, a.elem_base};
  pm_param_layout(p);
  return RSA_OK;
}

// f(NCB1, NCB2) for the hidden widths of `p`
template <class F>
static inline void pm_dispatch(const PmParams& p, F&& f) {
  dispatch_int<1, 2, 4>(p.h1 / 32, [&](auto N1) { dispatch_int<0, 1, 2, 4>(p.h2 / 32, [&](auto N2) { f(N1, N2); }); });
}

}  // namespace rsa

using namespace rsa;

extern "C" int64_t rsa_pair_mlp_workspace_bytes(int64_t n_pairs, int32_t d, int32_t h1, int32_t h2) {
  if (n_pairs < 0 || !pm_width_ok(d) || !pm_width_ok(h1) || !(h2 == 0 || pm_width_ok(h2))) return -1;
  Carver cv(nullptr);
  pm_layout(cv, n_pairs, d, h1, h2);
  return cv.bytes() + 256;
}

extern "C" int rsa_pair_mlp(const rsa_pair_mlp_args* args, rsa_stream_t stream) {
  const char* fn = "rsa_pair_mlp";
  rsa_pair_mlp_args a;
  if (int rc = load_args(a, args, fn)) return rc;
  PmParams p{};
  if (int rc = pm_check(a, fn, p)) return rc;
  if (a.n_query == 0 || a.n_slots == 0) return RSA_OK;
  RSA_CHECK_ARG(a.scores != nullptr, "%s: scores is null", fn);
  p.scores = a.scores;
  const int64_t lds = pm_lds_floats(a.d, a.h1, a.h2) * 4;
  const unsigned blocks = grid_1d(p.n_tiles, 4, 1024);
  int rc = RSA_OK;
  pm_dispatch(p, [&](auto N1, auto N2) {
    rc = allow_lds<pm_forward_kernel<N1(), N2()>>(lds, fn);
    if (rc == RSA_OK) hipLaunchKernelGGL((pm_forward_kernel<N1(), N2()>), dim3(blocks), dim3(256), (size_t)lds, (hipStream_t)stream, p);
  });
  if (rc) return rc;
  RSA_CHECK_LAUNCH(fn);
  return RSA_OK;
}

extern "C" int rsa_pair_mlp_backward(const rsa_pair_mlp_args* args, rsa_stream_t stream) {
  const char* fn = "rsa_pair_mlp_backward";
  rsa_pair_mlp_args a;
  if (int rc = load_args(a, args, fn)) return rc;
  PmParams p{};
  if (int rc = pm_check(a, fn, p)) return rc;
  RSA_CHECK_ARG(a.n_query > 0 && a.n_slots > 0, "%s: no pairs", fn);
  RSA_CHECK_ARG(a.g && a.dq && a.drows && a.dparams, "%s: g, dq, drows or dparams is null", fn);
  RSA_CHECK_ARG((((uintptr_t)a.dq | (uintptr_t)a.drows) & 15) == 0, "%s: dq and drows must be 16-byte aligned", fn);
  RSA_CHECK_ARG(a.workspace != nullptr, "%s: workspace is null", fn);
  const int64_t need = rsa_pair_mlp_workspace_bytes(p.n_pairs, a.d, a.h1, a.h2);
  RSA_CHECK_ARG(a.workspace_bytes >= need, "%s: the workspace is too small: %lld bytes, need %lld", fn, (long long)a.workspace_bytes,
                (long long)need);
  Carver cv(a.workspace);
  const PmLayout L = pm_layout(cv, p.n_pairs, a.d, a.h1, a.h2);
  p.g = a.g, p.dq = a.dq, p.drows = a.drows, p.dparams = a.dparams;
  p.dqp = L.dqp, p.pw = L.pw, p.n_wslots = (int)L.groups * 4;
  hipStream_t s = (hipStream_t)stream;
  const int64_t lds = pm_lds_floats(a.d, a.h1, a.h2) * 4;
  const unsigned blocks = grid_1d(p.n_tiles, 4, 1024);
  const unsigned ny = (unsigned)((a.h1 + a.h2) / 32);
  int rc = RSA_OK;
  pm_dispatch(p, [&](auto N1, auto N2) {
    rc = allow_lds<pm_rows_kernel<N1(), N2()>>(lds, fn);
    if (rc == RSA_OK) rc = allow_lds<pm_weights_kernel<N1(), N2()>>(lds, fn);
    if (rc != RSA_OK) return;
    hipLaunchKernelGGL((pm_rows_kernel<N1(), N2()>), dim3(blocks), dim3(256), (size_t)lds, s, p);
    hipLaunchKernelGGL((pm_weights_kernel<N1(), N2()>), dim3(L.groups, ny), dim3(256), (size_t)lds, s, p);
  });
  if (rc) return rc;
  RSA_CHECK_LAUNCH(fn);
  hipLaunchKernelGGL(pm_dq_kernel, dim3((unsigned)((p.n_query * (a.d / 4) + 255) / 256)), dim3(256), 0, s, p);
  hipLaunchKernelGGL(pm_reduce_kernel, dim3((unsigned)((p.n_params + 255) / 256)), dim3(256), 0, s, p);
  RSA_CHECK_LAUNCH(fn);
  return RSA_OK;
}
