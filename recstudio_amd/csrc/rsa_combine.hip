// NGCF's BiCombiner layer, fused (gfx950): forward and backward.
//
// rsa_bi_combine / rsa_bi_combine_backward : BiCombiner.forward   recstudio/model/module/graphmodule.py:70-86
//                                            + the normalise of NGCF's layer loop, recstudio/model/graph/ngcf.py:63-86
//
//   s = LeakyReLU((x + m) W1^T + b1),  p = LeakyReLU((x * m) W2^T + b2),  h = dropout(s + p),  n = h / max(||h||_2, 1e-12)
//
// TILE.  A wave owns 32 rows and all d_out columns of them; a workgroup is four such waves that share nothing but the weights.
// Both products run on v_mfma_f32_32x32x2_f32 (fp32 in, fp32 out, as rsa_fullscore.hip / rsa_dx.hip).  The forward and the row
// pass of the backward take the products TRANSPOSED -- the weight matrix is the A operand (M = output column), the row tile the B
// operand (N = row) -- so that lane (j, hh) of the wave ends up with row j of the tile in its registers, column
// 32 cb + (r & 3) + 8 (r >> 2) + 4 hh in register r of accumulator block cb.  Everything per row then happens inside a lane: the
// bias, both LeakyReLUs, the sum, the dropout, and the row's sum of squares, which needs ONE shuffle (the two halves hh) instead
// of a butterfly over the 32 lanes that the untransposed layout spreads a row over.  The price is the store: four consecutive
// registers are 16 contiguous bytes of a row, so a wave-instruction writes 16 bytes to each of 32 rows (and 16 more from the other
// half next to them) and L2 puts the rows' lines together.  The operands x and m are read the same way, 16 bytes per lane.
//
// K ORDER.  Step 4 u + i of the K loop multiplies the pair k = 8 u + i (lanes hh = 0) and k = 8 u + 4 + i (hh = 1): a lane reads
// ONE 16-byte piece of its x row, its m row and each weight row per four steps.  d_in is padded to a multiple of 8 with zeros (in
// LDS for the weights, in registers for x and m), d_out to a multiple of 32 with zero weight rows and zero biases: the padding
// columns come out as exact zeros and are never stored.
//
// WEIGHTS IN LDS.  Both matrices are staged once per workgroup, row c at c * (KP + 4) floats (KP = d_in rounded up to 8), and a
// workgroup strides over row tiles.  The A / B operand read is "lane j reads 16 bytes of row j": ds_read_b128 serves 16 lanes at a
// time, and with a row stride that is 4 mod 8 floats the 16 rows of every such group start in 16 different 4-bank slots -- no
// conflict.  The second product of the backward reads W[c][32 kb + j], one float per lane, 32 consecutive floats per half-wave:
// conflict-free as well.  Bytes: 2 * DOP * (KP + 4) * 4 + 2 * DOP * 4 (DOP = d_out rounded up to 32) -- 34 KB at 64 x 64, where LDS
// would let four workgroups share a CU but the registers allow two (the forward at two column blocks compiles to 166 VGPRs + 64
// accumulator registers: two waves per SIMD), 133 KB at 128 x 128 (one workgroup, four waves per CU: the kernel then lives on
// the loads its K loop keeps in flight).  d_in, d_out <= 128 is what the accumulators allow (2 * 4 blocks of 16 registers per
// lane), and barely: the rows pass of the backward at d_out > 96 uses all 512 registers and spills 20 bytes per lane to scratch
// (a cost in time only).  The host check names both limits.
//
// DROPOUT.  q = fp32(1 - p).  Element (r, c) is kept iff u[r * d_out + c] < q and is then DIVIDED by q (one rounding), u = that
// element of one torch.rand call (torch_rand_element: a ten-round Philox evaluation per element, as in the SimGCL noise).  p = 0
// draws nothing.
//
// BACKWARD.  Nothing is saved: both passes recompute the pre-activations from x and m and regenerate the mask.
//   rows pass     (bc_rows_kernel, the forward's layout)  per row: ss = sum h^2, c = max(sqrt(ss), 1e-12), t = (sum h g_n) / c
//                 (0 when the clamp is active: clamp_min passes no gradient below its bound), dh = g_h + (g_n - (h / c) t) / c,
//                 dsum = keep ? dh / q : 0, ds = dsum * slope(s), dp = dsum * slope(p).  ds / dp are then in the A-operand layout
//                 of the next product (M = row j, the K pair of step t = the two columns register t holds): da = ds W1, db = dp
//                 W2 come out with N = input column on the lanes, so dx = da + db * m and dm = da + db * x are written in whole
//                 128-byte pieces.  {c, t} of every row go to the workspace.
//   weights pass  (bc_weights_kernel)  dW1 = ds^T (x + m), dW2 = dp^T (x * m) contract over ROWS, which needs ds with M = output
//                 column and the rows as the K pairs -- the layout the UNTRANSPOSED product leaves.  A wave takes one block of 32
//                 output columns (blockIdx.y), recomputes that block of S for its row tiles the other way round, rebuilds ds / dp
//                 from the row scalars of the rows pass, and keeps dW1 / dW2 [32, d_in] in accumulators over all its tiles.
//                 Recomputing the product costs 2 d_in d_out flops per row and matrix; passing ds between the layouts through
//                 LDS would need 2 * 16 KB per wave at d_out = 128 next to 133 KB of weights.
//   reduce        (bc_reduce_kernel)  every wave of the weights pass leaves its partial sums in its own slot of the workspace; one
//                 thread per output element adds the slots in ascending order.  No atomics anywhere: two runs are bit-equal.
// OCCUPANCY.  With up to two accumulator blocks per product (d <= 64) the two backward kernels are held to 256 registers
// (__launch_bounds__(256, 2)): two waves per SIMD instead of one took the rows pass from 2.9 to 1.9 ms and the weights pass from
// 3.7 to 2.5 ms on 2^21 rows at 64 x 64 (the epilogue's Philox rounds and divisions and the weights pass's operand loads wait
// under the other wave's MFMAs); wider layers need the registers for their accumulators.  The weights pass runs 256 workgroups
// per column block, 1024 partial slots at most, which the reduce adds in 0.07 ms.  (These per-kernel figures are readings of two
// kernel traces of five calls each, taken once while the kernels were written; no file in profiles/ holds them.  What
// tools/bench_ngcf.py records is the whole backward: 6.7 ms before, 4.5 ms after.)
// flops per row: forward 4 d_in d_out; backward 16 d_in d_out.  Bytes per row (d = 64): forward 512 read + 512 written; backward
// 2 * 1024 read (both passes read x, m, g_h, g_n) + 512 written.
#include <utility>

#include "rsa_lds.hpp"

namespace rsa {

using f32x16 = float __attribute__((ext_vector_type(16)));

constexpr int BC_MAX_DIM = 128;
constexpr int BC_WEIGHT_GROUPS = 256;        // workgroups per column block of the weights pass: 4 * 256 partial slots at most

extern __shared__ __attribute__((aligned(16))) float bc_smem[];

struct BcParams {
  const float *x, *m, *w1, *w2, *b1, *b2;
  int64_t n_rows, n_tiles;
  int d_in, d_out, kp, ldw, dop, kb32;        // kp: d_in rounded up to 8; ldw = kp + 4; dop: d_out rounded up to 32; kb32 = ceil(d_in / 32)
  float slope, q;
  int drop;
  PhiloxCall pc;
  float* h;
  float* n;                                   // already at the block's first column
  int64_t n_stride;
  const float* g_h;
  const float* g_n;                           // already at the block's first column
  int64_t g_n_stride;
  float *dx, *dm;
  float2* rowsc;                              // [n_rows] {c, t} of the rows pass
  float *pw, *pb;                             // [slots][2][dop][32 kb32], [slots][2][dop]
  int n_slots;
  float *dw1, *dw2, *db1, *db2;
};

// f(integral_constant<int, 0>) ... f(integral_constant<int, N - 1>): a loop over accumulator blocks whose trips are separate pieces of
// code (one `#pragma unroll` loop over 4 x 16 elements with a Philox evaluation each is past what the compiler unrolls, and an
// accumulator indexed by a run-time block number goes to scratch)
template <class F, int... I>
__device__ __forceinline__ void bc_each(F&& f, std::integer_sequence<int, I...>) {
  (f(std::integral_constant<int, I>{}), ...);
}
template <int N, class F>
__device__ __forceinline__ void bc_blocks(F&& f) {
  bc_each(static_cast<F&&>(f), std::make_integer_sequence<int, N>{});
}

__device__ __forceinline__ int row32(int r, int hh) { return (r & 3) + 8 * (r >> 2) + 4 * hh; }
__device__ __forceinline__ float bc_leaky(float v, float slope) { return v > 0.f ? v : v * slope; }
__device__ __forceinline__ float bc_slope(float v, float slope) { return v > 0.f ? 1.f : slope; }
// d loss / d h of one element: the gradient arriving at h plus the normalise backward (file header, BACKWARD)
__device__ __forceinline__ float bc_dh(float hv, float gh, float gn, float cn, float t) { return gh + (gn - (hv / cn) * t) / cn; }

// rows [c0, c0 + rows) of both weight matrices and biases into LDS, zero-padded; ends with a barrier
__device__ __forceinline__ void bc_stage(const BcParams& p, int c0, int rows, float* w1s, float* w2s, float* b1s, float* b2s) {
  const int k4 = p.ldw >> 2;
  for (int i = threadIdx.x; i < rows * k4; i += blockDim.x) {
    const int r = i / k4, k = (i - r * k4) * 4, c = c0 + r;
    float4 a = make_float4(0.f, 0.f, 0.f, 0.f), b = a;
    if (c < p.d_out && k < p.d_in) {
      a = *reinterpret_cast<const float4*>(p.w1 + (int64_t)c * p.d_in + k);
      b = *reinterpret_cast<const float4*>(p.w2 + (int64_t)c * p.d_in + k);
    }
    *reinterpret_cast<float4*>(w1s + r * p.ldw + k) = a;
    *reinterpret_cast<float4*>(w2s + r * p.ldw + k) = b;
  }
  for (int i = threadIdx.x; i < rows; i += blockDim.x) {
    const int c = c0 + i;
    b1s[i] = c < p.d_out ? p.b1[c] : 0.f;
    b2s[i] = c < p.d_out ? p.b2[c] : 0.f;
  }
  __syncthreads();
}

// Both products of the rows row0 .. row0 + 31 against the NCB staged column blocks, without the biases.
// ROWS_N: sa[cb][r] of lane (j, hh) = column 32 cb + row32(r, hh) of row row0 + j; otherwise row row0 + row32(r, hh), column 32 cb + j.
template <int NCB, bool ROWS_N>
__device__ __forceinline__ void bc_products(const BcParams& p, const float* w1s, const float* w2s, int64_t row0, int lane,
                                            f32x16 (&sa)[NCB], f32x16 (&pa)[NCB]) {
  const int j = lane & 31, hh = lane >> 5;
  int64_t row = row0 + j;
  if (row >= p.n_rows) row = p.n_rows - 1;                         // (a row that exists; its results are not stored)
  const float* xr = p.x + row * p.d_in;
  const float* mr = p.m + row * p.d_in;
#pragma unroll
  for (int cb = 0; cb < NCB; ++cb) {
    sa[cb] = f32x16{0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    pa[cb] = f32x16{0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  }
  for (int k0 = 4 * hh; k0 < p.kp; k0 += 8) {                      // (kp is a multiple of 8: both halves make kp / 8 trips)
    float4 xv = make_float4(0.f, 0.f, 0.f, 0.f), mv = xv;
    if (k0 < p.d_in) {
      xv = *reinterpret_cast<const float4*>(xr + k0);
      mv = *reinterpret_cast<const float4*>(mr + k0);
    }
    const float av[4] = {xv.x + mv.x, xv.y + mv.y, xv.z + mv.z, xv.w + mv.w};
    const float pv[4] = {xv.x * mv.x, xv.y * mv.y, xv.z * mv.z, xv.w * mv.w};
#pragma unroll
    for (int cb = 0; cb < NCB; ++cb) {
      const float4 wa = *reinterpret_cast<const float4*>(w1s + (cb * 32 + j) * p.ldw + k0);
      const float4 wb = *reinterpret_cast<const float4*>(w2s + (cb * 32 + j) * p.ldw + k0);
      const float w1v[4] = {wa.x, wa.y, wa.z, wa.w}, w2v[4] = {wb.x, wb.y, wb.z, wb.w};
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        if constexpr (ROWS_N) {
          sa[cb] = __builtin_amdgcn_mfma_f32_32x32x2f32(w1v[i], av[i], sa[cb], 0, 0, 0);
          pa[cb] = __builtin_amdgcn_mfma_f32_32x32x2f32(w2v[i], pv[i], pa[cb], 0, 0, 0);
        } else {
          sa[cb] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[i], w1v[i], sa[cb], 0, 0, 0);
          pa[cb] = __builtin_amdgcn_mfma_f32_32x32x2f32(pv[i], w2v[i], pa[cb], 0, 0, 0);
        }
      }
    }
  }
}

// h of element (row, c) from its two pre-activations; `kept` receives the mask
__device__ __forceinline__ float bc_h(const BcParams& p, float pre_s, float pre_p, int64_t row, int c, bool& kept) {
  float v = bc_leaky(pre_s, p.slope) + bc_leaky(pre_p, p.slope);
  kept = true;
  if (p.drop) {
    const float u = torch_rand_element(p.pc, (uint64_t)row * (uint64_t)p.d_out + (uint64_t)c);
    kept = u < p.q;
    v = kept ? v / p.q : 0.f;
  }
  return v;
}

template <int NCB>
__global__ __launch_bounds__(256) void bc_forward_kernel(const BcParams p) {
  float* w1s = bc_smem;
  float* w2s = w1s + p.dop * p.ldw;
  float* b1s = w2s + p.dop * p.ldw;
  float* b2s = b1s + p.dop;
  bc_stage(p, 0, p.dop, w1s, w2s, b1s, b2s);
  const int lane = lane_id(), wave = threadIdx.x >> 6, j = lane & 31, hh = lane >> 5;
  for (int64_t tile = (int64_t)blockIdx.x * 4 + wave; tile < p.n_tiles; tile += (int64_t)gridDim.x * 4) {
    const int64_t row0 = tile * 32, row = row0 + j;
    const bool row_ok = row < p.n_rows;
    const int64_t rowc = row_ok ? row : p.n_rows - 1;
    f32x16 sa[NCB], pa[NCB];
    bc_products<NCB, true>(p, w1s, w2s, row0, lane, sa, pa);
    float ss = 0.f;
    bc_blocks<NCB>([&](auto CB) {
      constexpr int cb = decltype(CB)::value;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int c = cb * 32 + row32(r, hh);
        float hv = 0.f;
        if (c < p.d_out) {
          bool kept;
          hv = bc_h(p, sa[cb][r] + b1s[c], pa[cb][r] + b2s[c], rowc, c, kept);
        }
        sa[cb][r] = hv;
        ss += hv * hv;
      }
    });
    ss += __shfl_xor(ss, 32, 64);
    const float cn = fmaxf(sqrtf(ss), 1e-12f);
    if (!row_ok) continue;
#pragma unroll
    for (int cb = 0; cb < NCB; ++cb)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int c = cb * 32 + 8 * g + 4 * hh;
        if (c < p.d_out) {
          const float4 hv = make_float4(sa[cb][4 * g], sa[cb][4 * g + 1], sa[cb][4 * g + 2], sa[cb][4 * g + 3]);
          if (p.h) *reinterpret_cast<float4*>(p.h + row * p.d_out + c) = hv;
          if (p.n) *reinterpret_cast<float4*>(p.n + row * p.n_stride + c) = make_float4(hv.x / cn, hv.y / cn, hv.z / cn, hv.w / cn);
        }
      }
  }
}

template <int NCB>
__global__ __launch_bounds__(256, NCB <= 2 ? 2 : 1) void bc_rows_kernel(const BcParams p) {
  float* w1s = bc_smem;
  float* w2s = w1s + p.dop * p.ldw;
  float* b1s = w2s + p.dop * p.ldw;
  float* b2s = b1s + p.dop;
  bc_stage(p, 0, p.dop, w1s, w2s, b1s, b2s);
  const int lane = lane_id(), wave = threadIdx.x >> 6, j = lane & 31, hh = lane >> 5;
  for (int64_t tile = (int64_t)blockIdx.x * 4 + wave; tile < p.n_tiles; tile += (int64_t)gridDim.x * 4) {
    const int64_t row0 = tile * 32, row = row0 + j;
    const bool row_ok = row < p.n_rows;
    const int64_t rowc = row_ok ? row : p.n_rows - 1;
    f32x16 sa[NCB], pa[NCB];
    bc_products<NCB, true>(p, w1s, w2s, row0, lane, sa, pa);
    // ---- the row's scalars: sum h^2 and sum h g_n, the mask kept as one bit per element
    uint64_t keep = 0;
    float ss = 0.f, dot = 0.f;
    bc_blocks<NCB>([&](auto CB) {
      constexpr int cb = decltype(CB)::value;
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int c0 = cb * 32 + 8 * g + 4 * hh;
        if (c0 < p.d_out) {
          float4 gn4 = make_float4(0.f, 0.f, 0.f, 0.f);
          if (p.g_n) gn4 = *reinterpret_cast<const float4*>(p.g_n + rowc * p.g_n_stride + c0);
          const float gn[4] = {gn4.x, gn4.y, gn4.z, gn4.w};
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const int r = 4 * g + i;
            bool kept;
            const float hv = bc_h(p, sa[cb][r] + b1s[c0 + i], pa[cb][r] + b2s[c0 + i], rowc, c0 + i, kept);
            if (kept) keep |= 1ull << (cb * 16 + r);
            ss += hv * hv;
            dot += hv * gn[i];
          }
        }
      }
    });
    ss += __shfl_xor(ss, 32, 64);
    dot += __shfl_xor(dot, 32, 64);
    const float nrm = sqrtf(ss), cn = fmaxf(nrm, 1e-12f);
    const float t = nrm >= 1e-12f ? dot / cn : 0.f;
    if (row_ok && hh == 0) p.rowsc[row] = make_float2(cn, t);
    // ---- ds, dp in place of the pre-activations
    bc_blocks<NCB>([&](auto CB) {
      constexpr int cb = decltype(CB)::value;
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int c0 = cb * 32 + 8 * g + 4 * hh;
        float4 gn4 = make_float4(0.f, 0.f, 0.f, 0.f), gh4 = gn4;
        if (c0 < p.d_out) {
          if (p.g_n) gn4 = *reinterpret_cast<const float4*>(p.g_n + rowc * p.g_n_stride + c0);
          if (p.g_h) gh4 = *reinterpret_cast<const float4*>(p.g_h + rowc * p.d_out + c0);
        }
        const float gn[4] = {gn4.x, gn4.y, gn4.z, gn4.w}, gh[4] = {gh4.x, gh4.y, gh4.z, gh4.w};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int r = 4 * g + i;
          float ds = 0.f, dp = 0.f;
          if (c0 < p.d_out) {
            const float pre_s = sa[cb][r] + b1s[c0 + i], pre_p = pa[cb][r] + b2s[c0 + i];
            const bool kept = (keep >> (cb * 16 + r)) & 1;
            float hv = bc_leaky(pre_s, p.slope) + bc_leaky(pre_p, p.slope);
            if (p.drop) hv = kept ? hv / p.q : 0.f;
            float dsum = bc_dh(hv, gh[i], gn[i], cn, t);
            if (p.drop) dsum = kept ? dsum / p.q : 0.f;
            ds = dsum * bc_slope(pre_s, p.slope);
            dp = dsum * bc_slope(pre_p, p.slope);
          }
          sa[cb][r] = ds;
          pa[cb][r] = dp;
        }
      }
    });
    // ---- da = ds W1, db = dp W2, one block of 32 input columns at a time
    for (int kb = 0; kb < p.kb32; ++kb) {
      const int kin = kb * 32 + j, kl = kin < p.kp ? kin : 0;       // (a column past the staged ones reads column 0 and is not stored)
      f32x16 da = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, db = da;
#pragma unroll
      for (int cb = 0; cb < NCB; ++cb)
#pragma unroll
        for (int t2 = 0; t2 < 16; ++t2) {
          const int c = cb * 32 + row32(t2, hh);
          da = __builtin_amdgcn_mfma_f32_32x32x2f32(sa[cb][t2], w1s[c * p.ldw + kl], da, 0, 0, 0);
          db = __builtin_amdgcn_mfma_f32_32x32x2f32(pa[cb][t2], w2s[c * p.ldw + kl], db, 0, 0, 0);
        }
      if (kin < p.d_in) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int64_t rr = row0 + row32(r, hh);
          if (rr < p.n_rows) {
            const int64_t at = rr * p.d_in + kin;
            const float xv = p.x[at], mv = p.m[at];
            p.dx[at] = da[r] + db[r] * mv;
            p.dm[at] = da[r] + db[r] * xv;
          }
        }
      }
    }
  }
}

template <int KB32>
__global__ __launch_bounds__(256, KB32 <= 2 ? 2 : 1) void bc_weights_kernel(const BcParams p) {
  float* w1s = bc_smem;
  float* w2s = w1s + 32 * p.ldw;
  float* b1s = w2s + 32 * p.ldw;
  float* b2s = b1s + 32;
  const int cb = blockIdx.y;
  bc_stage(p, cb * 32, 32, w1s, w2s, b1s, b2s);
  const int lane = lane_id(), wave = threadIdx.x >> 6, j = lane & 31, hh = lane >> 5;
  const int c = cb * 32 + j;
  const bool c_ok = c < p.d_out;
  f32x16 dw1[KB32], dw2[KB32];
#pragma unroll
  for (int kb = 0; kb < KB32; ++kb) {
    dw1[kb] = f32x16{0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    dw2[kb] = f32x16{0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  }
  float db1 = 0.f, db2 = 0.f;
  for (int64_t tile = (int64_t)blockIdx.x * 4 + wave; tile < p.n_tiles; tile += (int64_t)gridDim.x * 4) {
    const int64_t row0 = tile * 32;
    f32x16 sa[1], pa[1];
    bc_products<1, false>(p, w1s, w2s, row0, lane, sa, pa);
    float ds[16], dp[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int64_t rr = row0 + row32(r, hh);
      ds[r] = 0.f;
      dp[r] = 0.f;
      if (c_ok && rr < p.n_rows) {
        const float pre_s = sa[0][r] + b1s[j], pre_p = pa[0][r] + b2s[j];
        bool kept;
        const float hv = bc_h(p, pre_s, pre_p, rr, c, kept);
        const float2 sc = p.rowsc[rr];
        const float gh = p.g_h ? p.g_h[rr * p.d_out + c] : 0.f;
        const float gn = p.g_n ? p.g_n[rr * p.g_n_stride + c] : 0.f;
        float dsum = bc_dh(hv, gh, gn, sc.x, sc.y);
        if (p.drop) dsum = kept ? dsum / p.q : 0.f;
        ds[r] = dsum * bc_slope(pre_s, p.slope);
        dp[r] = dsum * bc_slope(pre_p, p.slope);
      }
      db1 += ds[r];
      db2 += dp[r];
    }
#pragma unroll
    for (int t = 0; t < 16; ++t) {
      const int64_t rr = row0 + row32(t, hh);
#pragma unroll
      for (int kb = 0; kb < KB32; ++kb) {
        const int kin = kb * 32 + j;
        float xv = 0.f, mv = 0.f;
        if (rr < p.n_rows && kin < p.d_in) {
          xv = p.x[rr * p.d_in + kin];
          mv = p.m[rr * p.d_in + kin];
        }
        dw1[kb] = __builtin_amdgcn_mfma_f32_32x32x2f32(ds[t], xv + mv, dw1[kb], 0, 0, 0);
        dw2[kb] = __builtin_amdgcn_mfma_f32_32x32x2f32(dp[t], xv * mv, dw2[kb], 0, 0, 0);
      }
    }
  }
  // the wave's partial sums, in its own slot (a wave without a tile writes zeros)
  db1 += __shfl_xor(db1, 32, 64);
  db2 += __shfl_xor(db2, 32, 64);
  const int64_t slot = (int64_t)blockIdx.x * 4 + wave, kw = 32 * p.kb32;
  float* pw1 = p.pw + (slot * 2 + 0) * p.dop * kw;
  float* pw2 = p.pw + (slot * 2 + 1) * p.dop * kw;
#pragma unroll
  for (int kb = 0; kb < KB32; ++kb)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int64_t at = (int64_t)(cb * 32 + row32(r, hh)) * kw + kb * 32 + j;
      pw1[at] = dw1[kb][r];
      pw2[at] = dw2[kb][r];
    }
  if (hh == 0) {
    p.pb[(slot * 2 + 0) * p.dop + cb * 32 + j] = db1;
    p.pb[(slot * 2 + 1) * p.dop + cb * 32 + j] = db2;
  }
}

// One thread per element of dW1, dW2, db1, db2: the slots added in ascending order, eight loads in flight.
__global__ __launch_bounds__(256) void bc_reduce_kernel(const BcParams p) {
  const int64_t tid = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t nw = (int64_t)p.d_out * p.d_in, kw = 32 * p.kb32;
  const float* src;
  float* dst;
  int64_t stride;
  if (tid < 2 * nw) {
    const int mat = tid >= nw;
    const int64_t rem = tid - mat * nw, c = rem / p.d_in, k = rem - c * p.d_in;
    src = p.pw + ((int64_t)mat * p.dop + c) * kw + k;
    stride = 2 * (int64_t)p.dop * kw;
    dst = (mat ? p.dw2 : p.dw1) + rem;
  } else if (tid < 2 * nw + 2 * p.d_out) {
    const int64_t e = tid - 2 * nw;
    const int mat = e >= p.d_out;
    const int64_t c = e - (int64_t)mat * p.d_out;
    src = p.pb + (int64_t)mat * p.dop + c;
    stride = 2 * (int64_t)p.dop;
    dst = (mat ? p.db2 : p.db1) + c;
  } else {
    return;
  }
  float acc = 0.f;
  for (int s = 0; s < p.n_slots; s += 8) {
    float v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = src[(int64_t)(s + u < p.n_slots ? s + u : p.n_slots - 1) * stride];
#pragma unroll
    for (int u = 0; u < 8; ++u) acc += s + u < p.n_slots ? v[u] : 0.f;
  }
  *dst = acc;
}

struct BcLayout {
  float2* rowsc;
  float *pw, *pb;
  unsigned groups;
  int slots;
};

static inline int64_t bc_tiles(int64_t n_rows) { return (n_rows + 31) / 32; }

static inline BcLayout bc_layout(Carver& cv, int64_t n_rows, int d_in, int d_out) {
  BcLayout L;
  const int64_t dop = (d_out + 31) / 32 * 32, kw = (d_in + 31) / 32 * 32;
  L.groups = grid_1d(bc_tiles(n_rows), 4, BC_WEIGHT_GROUPS);
  L.slots = (int)L.groups * 4;
  L.rowsc = cv.take<float2>(n_rows);
  L.pw = cv.take<float>((int64_t)L.slots * 2 * dop * kw);
  L.pb = cv.take<float>((int64_t)L.slots * 2 * dop);
  return L;
}

static inline int64_t bc_lds_bytes(int d_in, int rows) {
  const int64_t ldw = (d_in + 7) / 8 * 8 + 4;
  return (2 * rows * ldw + 2 * rows) * 4;
}

// the checks both entry points share (everything but the outputs); fills the shared part of `p`
static int bc_check(const rsa_bi_combine_args& a, const char* fn, BcParams& p) {
  RSA_CHECK_ARG(a.n_rows >= 0, "%s: negative n_rows %lld", fn, (long long)a.n_rows);
  RSA_CHECK_ARG(a.d_in >= 4 && a.d_out >= 4 && a.d_in % 4 == 0 && a.d_out % 4 == 0,
                "%s: d_in and d_out must be multiples of 4 and at least 4, got %d and %d", fn, a.d_in, a.d_out);
  RSA_CHECK_ARG(a.d_in <= BC_MAX_DIM && a.d_out <= BC_MAX_DIM && bc_lds_bytes(a.d_in, (a.d_out + 31) / 32 * 32) <= LDS_LIMIT,
                "%s: d_in %d, d_out %d: both weight matrices are kept in LDS (%lld bytes of %lld) and in 2 x 4 accumulator blocks: "
                "at most %d each", fn, a.d_in, a.d_out, (long long)bc_lds_bytes(a.d_in, (a.d_out + 31) / 32 * 32),
                (long long)LDS_LIMIT, BC_MAX_DIM);
  RSA_CHECK_ARG(std::isfinite(a.negative_slope), "%s: negative_slope must be finite", fn);
  RSA_CHECK_ARG(a.p >= 0.0 && a.p < 1.0, "%s: the dropout probability must lie in [0, 1), got %g", fn, a.p);
  RSA_CHECK_ARG(a.p == 0.0 || (a.grid_threads > 0 && a.grid_threads % 256 == 0 && (a.offset & 3) == 0),
                "%s: bad philox state for the dropout (grid_threads %u must be a positive multiple of 256, offset a multiple of 4)",
                fn, a.grid_threads);
  if (a.n_rows == 0) return RSA_OK;
  RSA_CHECK_ARG(a.x && a.m && a.w1 && a.w2 && a.b1 && a.b2, "%s: x, m, w1, w2, b1 or b2 is null", fn);
  RSA_CHECK_ARG((((uintptr_t)a.x | (uintptr_t)a.m | (uintptr_t)a.w1 | (uintptr_t)a.w2) & 15) == 0,
                "%s: x, m, w1 and w2 must be 16-byte aligned", fn);
  RSA_CHECK_ARG(bc_tiles(a.n_rows) < (1ll << 31), "%s: too many rows for one launch", fn);
  p.x = a.x, p.m = a.m, p.w1 = a.w1, p.w2 = a.w2, p.b1 = a.b1, p.b2 = a.b2;
  p.n_rows = a.n_rows, p.n_tiles = bc_tiles(a.n_rows);
  p.d_in = a.d_in, p.d_out = a.d_out;
  p.kp = (a.d_in + 7) / 8 * 8, p.ldw = p.kp + 4, p.dop = (a.d_out + 31) / 32 * 32, p.kb32 = (a.d_in + 31) / 32;
  p.slope = a.negative_slope;
  p.q = (float)(1.0 - a.p);
  p.drop = a.p != 0.0;
  p.pc = PhiloxCall{a.seed, a.offset >> 2, a.grid_threads, a.elem_base};
  return RSA_OK;
}

// a column block of a wider table: base, row stride and first column (floats)
static int bc_check_block(const float* base, int64_t stride, int64_t col, int d_out, const char* fn, const char* name) {
  RSA_CHECK_ARG(stride % 4 == 0 && col % 4 == 0 && col >= 0 && col + d_out <= stride && ((uintptr_t)base & 15) == 0,
                "%s: %s must be 16-byte aligned with a row stride and a column offset that are multiples of 4 and col + d_out <= "
                "stride (stride %lld, col %lld)", fn, name, (long long)stride, (long long)col);
  return RSA_OK;
}

}  // namespace rsa

using namespace rsa;

extern "C" int64_t rsa_bi_combine_workspace_bytes(int64_t n_rows, int32_t d_in, int32_t d_out) {
  if (n_rows < 0 || d_in < 4 || d_out < 4 || d_in > BC_MAX_DIM || d_out > BC_MAX_DIM) return -1;
  Carver cv(nullptr);
  bc_layout(cv, n_rows, d_in, d_out);
  return cv.bytes() + 256;
}

extern "C" int rsa_bi_combine(const rsa_bi_combine_args* args, rsa_stream_t stream) {
  const char* fn = "rsa_bi_combine";
  rsa_bi_combine_args a;
  if (int rc = load_args(a, args, fn)) return rc;
  BcParams p{};
  if (int rc = bc_check(a, fn, p)) return rc;
  RSA_CHECK_ARG(a.h != nullptr || a.n != nullptr, "%s: h and n are both null", fn);
  RSA_CHECK_ARG(((uintptr_t)a.h & 15) == 0, "%s: h must be 16-byte aligned", fn);
  if (a.n)
    if (int rc = bc_check_block(a.n, a.n_stride, a.n_col, a.d_out, fn, "n")) return rc;
  if (a.n_rows == 0) return RSA_OK;
  p.h = a.h;
  p.n = a.n ? a.n + a.n_col : nullptr;
  p.n_stride = a.n_stride;
  const int64_t lds = bc_lds_bytes(a.d_in, p.dop);
  const unsigned blocks = grid_1d(p.n_tiles, 4, 2048);
  int rc = RSA_OK;
  dispatch_int<1, 2, 3, 4>(p.dop / 32, [&](auto NCB) {
    rc = allow_lds<bc_forward_kernel<NCB()>>(lds, fn);
    if (rc == RSA_OK) hipLaunchKernelGGL((bc_forward_kernel<NCB()>), dim3(blocks), dim3(256), (size_t)lds, (hipStream_t)stream, p);
  });
  if (rc) return rc;
  RSA_CHECK_LAUNCH(fn);
  return RSA_OK;
}

extern "C" int rsa_bi_combine_backward(const rsa_bi_combine_args* args, rsa_stream_t stream) {
  const char* fn = "rsa_bi_combine_backward";
  rsa_bi_combine_args a;
  if (int rc = load_args(a, args, fn)) return rc;
  BcParams p{};
  if (int rc = bc_check(a, fn, p)) return rc;
  RSA_CHECK_ARG(a.g_h != nullptr || a.g_n != nullptr, "%s: g_h and g_n are both null", fn);
  RSA_CHECK_ARG(((uintptr_t)a.g_h & 15) == 0, "%s: g_h must be 16-byte aligned", fn);
  if (a.g_n)
    if (int rc = bc_check_block(a.g_n, a.g_n_stride, a.g_n_col, a.d_out, fn, "g_n")) return rc;
  if (a.n_rows == 0) return RSA_OK;
  RSA_CHECK_ARG(a.dx && a.dm && a.dw1 && a.dw2 && a.db1 && a.db2, "%s: dx, dm, dw1, dw2, db1 or db2 is null", fn);
  RSA_CHECK_ARG(a.workspace != nullptr, "%s: workspace is null", fn);
  const int64_t need = rsa_bi_combine_workspace_bytes(a.n_rows, a.d_in, a.d_out);
  RSA_CHECK_ARG(a.workspace_bytes >= need, "%s: the workspace is too small: %lld bytes, need %lld", fn, (long long)a.workspace_bytes,
                (long long)need);
  Carver cv(a.workspace);
  const BcLayout L = bc_layout(cv, a.n_rows, a.d_in, a.d_out);
  p.g_h = a.g_h;
  p.g_n = a.g_n ? a.g_n + a.g_n_col : nullptr;
  p.g_n_stride = a.g_n_stride;
  p.dx = a.dx, p.dm = a.dm, p.dw1 = a.dw1, p.dw2 = a.dw2, p.db1 = a.db1, p.db2 = a.db2;
  p.rowsc = L.rowsc, p.pw = L.pw, p.pb = L.pb, p.n_slots = L.slots;
  hipStream_t s = (hipStream_t)stream;
  const int64_t lds = bc_lds_bytes(a.d_in, p.dop);
  const unsigned blocks = grid_1d(p.n_tiles, 4, 2048);
  int rc = RSA_OK;
  dispatch_int<1, 2, 3, 4>(p.dop / 32, [&](auto NCB) {
    rc = allow_lds<bc_rows_kernel<NCB()>>(lds, fn);
    if (rc == RSA_OK) hipLaunchKernelGGL((bc_rows_kernel<NCB()>), dim3(blocks), dim3(256), (size_t)lds, s, p);
  });
  if (rc) return rc;
  RSA_CHECK_LAUNCH(fn);
  dispatch_int<1, 2, 3, 4>(p.kb32, [&](auto KB32) {
    hipLaunchKernelGGL((bc_weights_kernel<KB32()>), dim3(L.groups, (unsigned)(p.dop / 32)), dim3(256), (size_t)bc_lds_bytes(a.d_in, 32), s, p);
  });
  RSA_CHECK_LAUNCH(fn);
  const int64_t outs = 2 * (int64_t)a.d_out * a.d_in + 2 * a.d_out;
  hipLaunchKernelGGL(bc_reduce_kernel, dim3((unsigned)((outs + 255) / 256)), dim3(256), 0, s, p);
  RSA_CHECK_LAUNCH(fn);
  return RSA_OK;
}
