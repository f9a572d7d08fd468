// Hierarchical gating of the sequence tower HGN, fused (gfx950): forward and backward.
//
// rsa_hgn_gating / rsa_hgn_gating_backward : HGNQueryEncoder.forward between the gathers and `U +`   recstudio/model/seq/hgn.py:31-43
//
//   f_bl = sigmoid(W1 s_bl + ug_b)   sf_bl = s_bl (.) f_bl   w_bl = sigmoid(w3 . sf_bl + ui_bl)   si_bl = sf_bl w_bl
//   mean: pooled_b = sum_l si_bl / sum_l w_bl     max: pooled_b[c] = max_l si_bl[c]     out_b = pooled_b + sum_l s_bl
//
// ug = W_g_2 U + b_g [B, D] and ui = U W_g_4.weight[:L]^T [B, L] are the caller's small GEMMs; W1 = W_g_1.weight [D, D] is read
// through a row stride; D is 32, 64 or 128.  There is no mask: a padded position is a zero row, it counts in sum_l w and takes
// part in the max with si = +0.
//
// TILE, as in rsa_ffattn.hip: the rows are the B * L positions, 32 to a wave, the product W1 s runs on v_mfma_f32_32x32x2_f32 in
// one of two layouts.  ROWS ON LANES (the transposed product: W1 is the A operand): lane (j, hh) holds row j of the tile, channel
// 32 cb + (r & 3) + 8 (r >> 2) + 4 hh in register r of accumulator block cb; sums over channels happen inside a lane plus one
// shuffle.  CHANNELS ON LANES (the rows are the A operand): lane (j, hh) holds channel 32 cb + j of rows row32(r, hh); sums over
// rows happen inside a lane plus one shuffle.  W1 sits in LDS at a row stride of D + 4 floats, w3 behind it (rsa_ffattn.hip,
// "WEIGHTS IN LDS").
//
// FORWARD (hg_forward_kernel), channels on lanes, because everything it writes but `w` is a sum (or a max) over the ROWS of a
// sequence.  A WAVE owns whole sequences -- floor(32 / L) of them in one tile when L <= 32, one sequence of ceil(L / 32) tiles
// otherwise -- so sum si, sum w, sum s and the max with its index stay in the wave's registers: no atomics, no slots, no barrier
// after the staging.  The one sum over channels, w3 . sf, takes the lanes' 16 partial sums through 16 MFMAs against a 0 / 1 matrix
// that TRANSPOSE them (exact products): lane j then holds the 32 partials of row j.  The rows of a tile are told apart by their
// sequence slot; a slot's rows are added in ascending order, the two halves hh last.  On exact ties the max keeps the lowest l.
//
// BACKWARD.  f and sf are recomputed; the forward's w (and arg) are read.
//   stats   (hg_stats_kernel, mean only, rows on lanes)  q_bl = g_b . sf_bl to the workspace
//   seq     (hg_seq_kernel, mean only)  one thread per sequence: den_b = sum_l w_bl, gp_b = (sum_l w_bl q_bl) / den_b = g_b . pooled_b
//   rows    (hg_rows_kernel, rows on lanes)  dsi, dw, dz = dui, dsf; t = dsf (.) f and dpre in registers.  dpre is the A operand
//           of W1^T dpre, which comes out with the key column on the lanes; t joins it there through one more MFMA chain per
//           column block against the 0 / 1 matrix "this channel is this column" (exact), and ds = g_b + (t + W1^T dpre) is
//           written in 128-byte pieces.
//   weights (hg_weights_kernel, channels on lanes, one block of 32 channels per blockIdx.y)  rebuilds dpre from dui, w, g and
//           den / arg; dW1 [32, D] stays in accumulators over the wave's tiles, dw3 in a register; dug goes through the 0 / 1
//           matrix "row belongs to the j-th sequence of this tile" to slot (tile + b) of the workspace, as rsa_ffattn.hip's dqh.
//   reduce  (hg_reduce_kernel)  adds the waves' slots of dW1 and dw3 and the pair slots of dug in ascending order.
// No float atomics anywhere: two runs are bit-equal.  All element offsets are 64-bit.
//
// flops per row: forward 2 D^2; backward 3 * 2 D^2 (three products; two for max pooling) + 2 D^2 (W1^T dpre) + 2 D^2 (dW1).
// Bytes per row: forward 4 D read + 4 written; backward about 3 * 4 D read + 4 D written.
// REGISTERS (profiles/hgn_resources.txt).  Forward at D = 32 / 64 / 128 (mean): 228 / 256 / 256 VGPRs + 16 / 33 / 116 accumulator
// registers, 2 / 1 / 1 waves per SIMD, no scratch.  Rows pass: 167 / 256 / 256 (+ 256 accumulator registers at D = 128); with dpre
// and t side by side it spills 176 bytes per lane at D = 64 and 716 (mean) / 856 (max) at D = 128 (a cost in time only).  Weights
// pass: 160 / 176 / 158 + 0 / 0 / 80, no scratch.
// MEASURED (tools/bench_hgn.py, B = 8192, mean pooling): forward 0.40 ms and forward + backward 2.28 ms at L = 50, D = 128 -- 0.22 and
// 0.23 of the fp32-matrix floor, 0.07 and 0.06 of the 8 TB/s byte model: at neither floor.
#include <utility>

#include "rsa_lds.hpp"

namespace rsa {

using f32x16 = float __attribute__((ext_vector_type(16)));

constexpr int HG_FORWARD_GRID = 2048;
constexpr int HG_ROWS_GRID = 2048;
constexpr int HG_WEIGHT_GROUPS = 128;        // workgroups per channel block of the weights pass: 4 * 128 partial slots at most

extern __shared__ __attribute__((aligned(16))) float hg_smem[];

struct HgParams {
  const float *s, *ug, *ui, *w1, *w3, *g;
  int64_t w1_stride;
  int64_t B, n_rows, n_tiles, n_units;
  int L, D, ldw, spu;                         // ldw = D + 4; spu: sequences per forward unit
  float *out, *w;
  int32_t* arg;
  float *ds, *dug, *dui, *dw1, *dw3;
  float *q, *den, *gp;                        // [n_rows], [B], [B]
  float *pw, *pw3;                            // [slots][D][D], [slots][D]
  float* pq;                                  // [n_tiles + B][D]
  int n_slots;
};

__device__ __forceinline__ int hg_row32(int r, int hh) { return (r & 3) + 8 * (r >> 2) + 4 * hh; }
__device__ __forceinline__ float hg_sigmoid(float x) { return 1.f / (1.f + expf(-x)); }
__device__ __forceinline__ float4 hg_ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ f32x16 hg_zero() { return f32x16{0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}; }

template <class F, int... I>
__device__ __forceinline__ void hg_each(F&& f, std::integer_sequence<int, I...>) {
  (f(std::integral_constant<int, I>{}), ...);
}
template <int N, class F>
__device__ __forceinline__ void hg_blocks(F&& f) {
  hg_each(static_cast<F&&>(f), std::make_integer_sequence<int, N>{});
}

// rows [c0, c0 + rows) of W1 and of w3 into LDS; ends with a barrier
__device__ __forceinline__ void hg_stage(const HgParams& p, int c0, int rows, float* ws, float* w3s) {
  const int k4 = p.D >> 2;
  for (int i = threadIdx.x; i < rows * k4; i += blockDim.x) {
    const int r = i / k4, k = (i - r * k4) * 4;
    *reinterpret_cast<float4*>(ws + r * p.ldw + k) = hg_ld4(p.w1 + (int64_t)(c0 + r) * p.w1_stride + k);
  }
  for (int i = threadIdx.x; i < rows; i += blockDim.x) w3s[i] = p.w3[c0 + i];
  __syncthreads();
}

// W1 s of the 32 rows the lanes' pointers `kr` name (lane (j, hh): row j), against the NCB staged channel blocks.
// ROWS_N: sa[cb][r] of lane (j, hh) = channel 32 cb + row32(r, hh) of row j; otherwise row row32(r, hh), channel 32 cb + j.
template <int NCB, bool ROWS_N>
__device__ __forceinline__ void hg_product(const HgParams& p, const float* ws, const float* kr, int lane, f32x16 (&sa)[NCB]) {
  const int j = lane & 31, hh = lane >> 5;
#pragma unroll
  for (int cb = 0; cb < NCB; ++cb) sa[cb] = hg_zero();
  for (int k0 = 4 * hh; k0 < p.D; k0 += 8) {
    const float4 kv4 = hg_ld4(kr + k0);
    const float kv[4] = {kv4.x, kv4.y, kv4.z, kv4.w};
#pragma unroll
    for (int cb = 0; cb < NCB; ++cb) {
      const float4 w4 = hg_ld4(ws + (cb * 32 + j) * p.ldw + k0);
      const float wv[4] = {w4.x, w4.y, w4.z, w4.w};
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        if constexpr (ROWS_N) sa[cb] = __builtin_amdgcn_mfma_f32_32x32x2f32(wv[i], kv[i], sa[cb], 0, 0, 0);
        else sa[cb] = __builtin_amdgcn_mfma_f32_32x32x2f32(kv[i], wv[i], sa[cb], 0, 0, 0);
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------- forward
template <int NCB, bool MAXP>
__global__ __launch_bounds__(256) void hg_forward_kernel(const HgParams p) {
  float* ws = hg_smem;
  float* w3s = ws + p.D * p.ldw;
  hg_stage(p, 0, p.D, ws, w3s);
  const int lane = lane_id(), wave = threadIdx.x >> 6, j = lane & 31, hh = lane >> 5;
  for (int64_t u = (int64_t)blockIdx.x * 4 + wave; u < p.n_units; u += (int64_t)gridDim.x * 4) {
    const int64_t b0 = u * p.spu;
    const int nb = (int)(b0 + p.spu <= p.B ? p.spu : p.B - b0);            // sequences of this unit (>= 1)
    const int64_t row_base = b0 * p.L;
    const int64_t rows_total = (int64_t)nb * p.L;                          // <= 32 when spu > 1
    const int64_t n_t = (rows_total + 31) / 32;
    float a_si[NCB], a_s[NCB], mx[NCB];
    int ag[NCB];
    float den = 0.f;
#pragma unroll
    for (int cb = 0; cb < NCB; ++cb) a_si[cb] = 0.f, a_s[cb] = 0.f, mx[cb] = -INFINITY, ag[cb] = 0;
    for (int64_t t = 0; t < n_t; ++t) {
      const int64_t tr0 = 32 * t;                                          // the tile's first row, counted inside the unit
      const bool ok = tr0 + j < rows_total;
      const int64_t row = row_base + (ok ? tr0 + j : rows_total - 1);      // (a row that exists; its result is not stored)
      f32x16 sa[NCB];
      hg_product<NCB, false>(p, ws, p.s + row * p.D, lane, sa);
      // ---- the 16 rows this lane holds: sequence slot (-1: no row), position, element offsets
      int sq[16], pos[16];
      int64_t so[16], bo[16];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int64_t off = tr0 + hg_row32(r, hh);
        const bool valid = off < rows_total;
        const int64_t offc = valid ? off : rows_total - 1;
        const int slot = p.spu > 1 ? (int)((unsigned)offc / (unsigned)p.L) : 0;
        sq[r] = valid ? slot : -1;
        pos[r] = (int)(offc - (int64_t)slot * p.L);
        so[r] = (row_base + offc) * p.D + j;
        bo[r] = (b0 + slot) * p.D + j;
      }
      // ---- f, sf in place of the pre-activations; s kept; the lane's share of w3 . sf
      f32x16 sn[NCB];
      float part[16];
#pragma unroll
      for (int r = 0; r < 16; ++r) part[r] = 0.f;
      hg_blocks<NCB>([&](auto CB) {
        constexpr int cb = decltype(CB)::value;
        const float w3c = w3s[cb * 32 + j];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const float sv = p.s[so[r] + cb * 32];
          const float f = hg_sigmoid(sa[cb][r] + p.ug[bo[r] + cb * 32]);
          const float sf = sv * f;
          sn[cb][r] = sv;
          sa[cb][r] = sf;
          part[r] += w3c * sf;
        }
      });
      // ---- transposed through the matrix unit: lane (n, hh) gets the partials of row n from lanes row32(r, hh)
      f32x16 tp = hg_zero();
#pragma unroll
      for (int r = 0; r < 16; ++r) tp = __builtin_amdgcn_mfma_f32_32x32x2f32(part[r], j == hg_row32(r, hh) ? 1.f : 0.f, tp, 0, 0, 0);
      float e = 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) e += tp[r];
      e += __shfl_xor(e, 32, 64);
      const float wl = hg_sigmoid(e + p.ui[row]);
      if (ok && hh == 0) p.w[row] = wl;
      float wr[16];
#pragma unroll
      for (int r = 0; r < 16; ++r) wr[r] = __shfl(wl, hg_row32(r, hh), 64);
      // ---- pooling, one sequence slot at a time
      const int nq = p.spu > 1 ? nb : 1;
      for (int q = 0; q < nq; ++q) {
#pragma unroll
        for (int r = 0; r < 16; ++r) den += sq[r] == q ? wr[r] : 0.f;
        hg_blocks<NCB>([&](auto CB) {
          constexpr int cb = decltype(CB)::value;
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const bool in = sq[r] == q;
            const float si = sa[cb][r] * wr[r];
            a_si[cb] += in ? si : 0.f;
            a_s[cb] += in ? sn[cb][r] : 0.f;
            if constexpr (MAXP) {
              if (in && si > mx[cb]) mx[cb] = si, ag[cb] = pos[r];
            }
          }
        });
        if (t == n_t - 1) {                                               // the sequence ends here: b0 + q
          const float dn = den + __shfl_xor(den, 32, 64);
          den = 0.f;
          hg_blocks<NCB>([&](auto CB) {
            constexpr int cb = decltype(CB)::value;
            const float ssum = a_s[cb] + __shfl_xor(a_s[cb], 32, 64);
            float pooled;
            int am = 0;
            if constexpr (MAXP) {
              const float om = __shfl_xor(mx[cb], 32, 64);
              const int oa = __shfl_xor(ag[cb], 32, 64);
              const bool other = om > mx[cb] || (om == mx[cb] && oa < ag[cb]);
              pooled = other ? om : mx[cb];
              am = other ? oa : ag[cb];
            } else {
              pooled = (a_si[cb] + __shfl_xor(a_si[cb], 32, 64)) / dn;
            }
            if (hh == 0) {
              const int64_t o = (b0 + q) * p.D + cb * 32 + j;
              p.out[o] = pooled + ssum;
              if constexpr (MAXP) p.arg[o] = am;
            }
            a_si[cb] = 0.f, a_s[cb] = 0.f, mx[cb] = -INFINITY, ag[cb] = 0;
          });
        }
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------- backward
// mean pooling: q_bl = g_b . sf_bl
template <int NCB>
__global__ __launch_bounds__(256) void hg_stats_kernel(const HgParams p) {
  float* ws = hg_smem;
  float* w3s = ws + p.D * p.ldw;
  hg_stage(p, 0, p.D, ws, w3s);
  const int lane = lane_id(), wave = threadIdx.x >> 6, j = lane & 31, hh = lane >> 5;
  for (int64_t tile = (int64_t)blockIdx.x * 4 + wave; tile < p.n_tiles; tile += (int64_t)gridDim.x * 4) {
    const int64_t row = tile * 32 + j;
    const bool ok = row < p.n_rows;
    const int64_t rowc = ok ? row : p.n_rows - 1;
    const int64_t b = rowc / p.L;
    const float* sr = p.s + rowc * p.D;
    f32x16 sa[NCB];
    hg_product<NCB, true>(p, ws, sr, lane, sa);
    float dot = 0.f;
    hg_blocks<NCB>([&](auto CB) {
      constexpr int cb = decltype(CB)::value;
#pragma unroll
      for (int g4 = 0; g4 < 4; ++g4) {
        const int c0 = cb * 32 + 8 * g4 + 4 * hh;
        const float4 u4 = hg_ld4(p.ug + b * p.D + c0), s4 = hg_ld4(sr + c0), gq = hg_ld4(p.g + b * p.D + c0);
        const float uv[4] = {u4.x, u4.y, u4.z, u4.w}, sv[4] = {s4.x, s4.y, s4.z, s4.w}, gv[4] = {gq.x, gq.y, gq.z, gq.w};
#pragma unroll
        for (int i = 0; i < 4; ++i) dot += gv[i] * (sv[i] * hg_sigmoid(sa[cb][4 * g4 + i] + uv[i]));
      }
    });
    dot += __shfl_xor(dot, 32, 64);
    if (ok && hh == 0) p.q[row] = dot;
  }
}

// mean pooling: den_b and gp_b = g_b . pooled_b, one thread per sequence, ascending l
__global__ __launch_bounds__(256) void hg_seq_kernel(const HgParams p) {
  const int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (b >= p.B) return;
  const float* wb = p.w + b * p.L;
  const float* qb = p.q + b * p.L;
  float den = 0.f, num = 0.f;
  for (int l = 0; l < p.L; ++l) {
    den += wb[l];
    num += wb[l] * qb[l];
  }
  p.den[b] = den;
  p.gp[b] = num / den;
}

template <int NCB, bool MAXP>
__global__ __launch_bounds__(256, NCB <= 2 ? 2 : 1) void hg_rows_kernel(const HgParams p) {
  float* ws = hg_smem;
  float* w3s = ws + p.D * p.ldw;
  hg_stage(p, 0, p.D, ws, w3s);
  const int lane = lane_id(), wave = threadIdx.x >> 6, j = lane & 31, hh = lane >> 5;
  for (int64_t tile = (int64_t)blockIdx.x * 4 + wave; tile < p.n_tiles; tile += (int64_t)gridDim.x * 4) {
    const int64_t row0 = tile * 32, row = row0 + j;
    const bool ok = row < p.n_rows;
    const int64_t rowc = ok ? row : p.n_rows - 1;
    const int64_t bq = row0 / p.L;                                // the tile's first sequence, and where in it the tile starts
    const unsigned rem = (unsigned)(row0 - bq * p.L);
    const int64_t b = rowc / p.L;
    const int l = (int)(rowc - b * p.L);
    const float* sr = p.s + rowc * p.D;
    const float* gr = p.g + b * p.D;
    const int32_t* ar = MAXP ? p.arg + b * p.D : nullptr;
    const float wv = p.w[rowc];
    float den = 1.f, gp = 0.f;
    if constexpr (!MAXP) den = p.den[b], gp = p.gp[b];
    f32x16 sa[NCB], tt[NCB];
    hg_product<NCB, true>(p, ws, sr, lane, sa);
    // ---- f in place of the pre-activations; dsi . sf
    float dot = 0.f;
    hg_blocks<NCB>([&](auto CB) {
      constexpr int cb = decltype(CB)::value;
#pragma unroll
      for (int g4 = 0; g4 < 4; ++g4) {
        const int c0 = cb * 32 + 8 * g4 + 4 * hh;
        const float4 u4 = hg_ld4(p.ug + b * p.D + c0), s4 = hg_ld4(sr + c0), gq = hg_ld4(gr + c0);
        const float uv[4] = {u4.x, u4.y, u4.z, u4.w}, sv[4] = {s4.x, s4.y, s4.z, s4.w}, gv[4] = {gq.x, gq.y, gq.z, gq.w};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const float f = hg_sigmoid(sa[cb][4 * g4 + i] + uv[i]);
          float dsi;
          if constexpr (MAXP) dsi = ar[c0 + i] == l ? gv[i] : 0.f;
          else dsi = gv[i] / den;
          sa[cb][4 * g4 + i] = f;
          dot += dsi * (sv[i] * f);
        }
      }
    });
    dot += __shfl_xor(dot, 32, 64);
    const float dw = MAXP ? dot : dot - gp / den;
    const float dz = dw * wv * (1.f - wv);
    if (ok && hh == 0) p.dui[row] = dz;
    // ---- dpre in place of f, t = dsf (.) f beside it
    hg_blocks<NCB>([&](auto CB) {
      constexpr int cb = decltype(CB)::value;
#pragma unroll
      for (int g4 = 0; g4 < 4; ++g4) {
        const int c0 = cb * 32 + 8 * g4 + 4 * hh;
        const float4 s4 = hg_ld4(sr + c0), gq = hg_ld4(gr + c0), w4 = hg_ld4(w3s + c0);
        const float sv[4] = {s4.x, s4.y, s4.z, s4.w}, gv[4] = {gq.x, gq.y, gq.z, gq.w}, w3v[4] = {w4.x, w4.y, w4.z, w4.w};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const float f = sa[cb][4 * g4 + i];
          float dsi;
          if constexpr (MAXP) dsi = ar[c0 + i] == l ? gv[i] : 0.f;
          else dsi = gv[i] / den;
          const float dsf = dsi * wv + dz * w3v[i];
          tt[cb][4 * g4 + i] = dsf * f;
          sa[cb][4 * g4 + i] = (dsf * sv[i]) * (f * (1.f - f));
        }
      }
    });
    // ---- the sequence of each of the 16 rows this lane stores
    int sq[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) sq[r] = (int)((rem + (unsigned)hg_row32(r, hh)) / (unsigned)p.L);
    // ---- ds = g + (t + W1^T dpre), one block of 32 key columns at a time
    hg_blocks<NCB>([&](auto KB) {
      constexpr int kb = decltype(KB)::value;
      const int kin = kb * 32 + j;
      f32x16 da = hg_zero();
#pragma unroll
      for (int cb = 0; cb < NCB; ++cb)
#pragma unroll
        for (int t2 = 0; t2 < 16; ++t2)
          da = __builtin_amdgcn_mfma_f32_32x32x2f32(sa[cb][t2], ws[(cb * 32 + hg_row32(t2, hh)) * p.ldw + kin], da, 0, 0, 0);
#pragma unroll
      for (int t2 = 0; t2 < 16; ++t2)
        da = __builtin_amdgcn_mfma_f32_32x32x2f32(tt[kb][t2], hg_row32(t2, hh) == j ? 1.f : 0.f, da, 0, 0, 0);
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int64_t rr = row0 + hg_row32(r, hh);
        if (rr < p.n_rows) p.ds[rr * p.D + kin] = p.g[(bq + sq[r]) * p.D + kin] + da[r];
      }
    });
  }
}

template <int KB32, bool MAXP>
__global__ __launch_bounds__(256, KB32 <= 2 ? 2 : 1) void hg_weights_kernel(const HgParams p) {
  float* ws = hg_smem;
  float* w3s = ws + 32 * p.ldw;
  const int cb = blockIdx.y;
  hg_stage(p, cb * 32, 32, ws, w3s);
  const int lane = lane_id(), wave = threadIdx.x >> 6, j = lane & 31, hh = lane >> 5;
  const int c = cb * 32 + j;
  const float w3c = w3s[j];
  f32x16 dw[KB32];
#pragma unroll
  for (int kb = 0; kb < KB32; ++kb) dw[kb] = hg_zero();
  float dw3 = 0.f;
  for (int64_t tile = (int64_t)blockIdx.x * 4 + wave; tile < p.n_tiles; tile += (int64_t)gridDim.x * 4) {
    const int64_t row0 = tile * 32;
    const int64_t rowc = row0 + j < p.n_rows ? row0 + j : p.n_rows - 1;
    const int64_t bq = row0 / p.L;
    const unsigned rem = (unsigned)(row0 - bq * p.L);
    f32x16 sa[1];
    hg_product<1, false>(p, ws, p.s + rowc * p.D, lane, sa);
    float ds[16];
    int sq[16];                                                   // which of the tile's sequences the row belongs to; -1: no row
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int off = hg_row32(r, hh);
      const int64_t rr = row0 + off;
      ds[r] = 0.f;
      sq[r] = -1;
      if (rr < p.n_rows) {
        const int slot = (int)((rem + (unsigned)off) / (unsigned)p.L);
        const int l = (int)(rem + (unsigned)off) - slot * p.L;
        const int64_t bc = (bq + slot) * p.D + c;
        const float f = hg_sigmoid(sa[0][r] + p.ug[bc]);
        const float sv = p.s[rr * p.D + c];
        const float dz = p.dui[rr], wv = p.w[rr], gv = p.g[bc];
        float dsi;
        if constexpr (MAXP) dsi = p.arg[bc] == l ? gv : 0.f;
        else dsi = gv / p.den[bq + slot];
        const float dsf = dsi * wv + dz * w3c;
        ds[r] = (dsf * sv) * (f * (1.f - f));
        dw3 += dz * (sv * f);
        sq[r] = slot;
      }
    }
    f32x16 dq = hg_zero();
#pragma unroll
    for (int t = 0; t < 16; ++t) {
      const int64_t rr = row0 + hg_row32(t, hh);
#pragma unroll
      for (int kb = 0; kb < KB32; ++kb) {
        const float kv = rr < p.n_rows ? p.s[rr * p.D + kb * 32 + j] : 0.f;
        dw[kb] = __builtin_amdgcn_mfma_f32_32x32x2f32(ds[t], kv, dw[kb], 0, 0, 0);
      }
      dq = __builtin_amdgcn_mfma_f32_32x32x2f32(ds[t], sq[t] == j ? 1.f : 0.f, dq, 0, 0, 0);
    }
    // the tile's share of dug of its j-th sequence: channel 32 cb + row32(r, hh) in register r
    const int64_t last = row0 + 31 < p.n_rows ? row0 + 31 : p.n_rows - 1;
    const int last_slot = (int)((rem + (unsigned)(last - row0)) / (unsigned)p.L);
    if (j <= last_slot) {
      float* dst = p.pq + (tile + bq + j) * p.D + cb * 32;
#pragma unroll
      for (int r = 0; r < 16; ++r) dst[hg_row32(r, hh)] = dq[r];
    }
  }
  // the wave's partial sums, in its own slot (a wave without a tile writes zeros)
  dw3 += __shfl_xor(dw3, 32, 64);
  const int64_t slot = (int64_t)blockIdx.x * 4 + wave;
  float* pw = p.pw + slot * p.D * p.D;
#pragma unroll
  for (int kb = 0; kb < KB32; ++kb)
#pragma unroll
    for (int r = 0; r < 16; ++r) pw[(int64_t)(cb * 32 + hg_row32(r, hh)) * p.D + kb * 32 + j] = dw[kb][r];
  if (hh == 0) p.pw3[slot * p.D + c] = dw3;
}

// One thread per element of dW1 and dw3 (the waves' slots added in ascending order, eight loads in flight) and of dug (the
// pair slots of the sequence's tiles, ascending).
__global__ __launch_bounds__(256) void hg_reduce_kernel(const HgParams p) {
  const int64_t tid = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t nw = (int64_t)p.D * p.D;
  const float* src;
  float* dst;
  int64_t stride;
  if (tid < nw) {
    src = p.pw + tid, stride = nw, dst = p.dw1 + tid;
  } else if (tid < nw + p.D) {
    src = p.pw3 + (tid - nw), stride = p.D, dst = p.dw3 + (tid - nw);
  } else {
    const int64_t e = tid - (nw + p.D);
    if (e >= p.B * p.D) return;
    const int64_t b = e / p.D, m = e - b * p.D;
    const int64_t t0 = b * p.L / 32, t1 = ((b + 1) * p.L - 1) / 32;
    float acc = 0.f;
    for (int64_t t = t0; t <= t1; ++t) acc += p.pq[(t + b) * p.D + m];
    p.dug[e] = acc;
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

struct HgLayout {
  float *q, *den, *gp, *pw, *pw3, *pq;
  unsigned groups;
  int slots;
};

static inline bool hg_dim_ok(int d) { return d == 32 || d == 64 || d == 128; }
static inline int64_t hg_tiles(int64_t n_rows) { return (n_rows + 31) / 32; }

static inline HgLayout hg_layout(Carver& cv, int64_t n_seq, int64_t seq_len, int d) {
  HgLayout L;
  const int64_t n_rows = n_seq * seq_len, n_tiles = hg_tiles(n_rows);
  L.groups = grid_1d(n_tiles, 4, HG_WEIGHT_GROUPS);
  L.slots = (int)L.groups * 4;
  L.q = cv.take<float>(n_rows);
  L.den = cv.take<float>(n_seq);
  L.gp = cv.take<float>(n_seq);
  L.pw = cv.take<float>((int64_t)L.slots * d * d);
  L.pw3 = cv.take<float>((int64_t)L.slots * d);
  L.pq = cv.take<float>((n_tiles + n_seq) * d);
  return L;
}

static inline int64_t hg_lds_bytes(int d, int rows) { return ((int64_t)rows * (d + 4) + rows) * 4; }

// the checks both entry points share (everything but the outputs); fills the shared part of `p`
static int hg_check(const rsa_hgn_gating_args& a, const char* fn, HgParams& p) {
  RSA_CHECK_ARG(a.n_seq >= 0, "%s: negative n_seq %lld", fn, (long long)a.n_seq);
  RSA_CHECK_ARG(a.seq_len >= 1, "%s: seq_len must be at least 1, got %d", fn, a.seq_len);
  RSA_CHECK_ARG(hg_dim_ok(a.d), "%s: d must be 32, 64 or 128 (W_g_1 is kept in LDS and in at most 4 accumulator blocks), got %d",
                fn, a.d);
  RSA_CHECK_ARG(a.pooling == 0 || a.pooling == 1, "%s: pooling must be 0 (mean) or 1 (max), got %d", fn, a.pooling);
  RSA_CHECK_ARG(a.n_seq <= (1ll << 40) / a.seq_len, "%s: n_seq * seq_len is too large", fn);
  if (a.n_seq == 0) return RSA_OK;
  RSA_CHECK_ARG(a.s && a.ug && a.ui && a.w1 && a.w3, "%s: s, ug, ui, w1 or w3 is null", fn);
  RSA_CHECK_ARG((((uintptr_t)a.s | (uintptr_t)a.ug | (uintptr_t)a.w1) & 15) == 0 && a.w1_stride % 4 == 0 && a.w1_stride >= a.d,
                "%s: s, ug and w1 must be 16-byte aligned, the row stride of w1 a multiple of 4 and at least d (stride %lld)", fn,
                (long long)a.w1_stride);
  RSA_CHECK_ARG(a.w != nullptr, "%s: w is null", fn);
  RSA_CHECK_ARG(a.pooling == 0 || a.arg != nullptr, "%s: max pooling needs arg", fn);
  p.s = a.s, p.ug = a.ug, p.ui = a.ui, p.w1 = a.w1, p.w3 = a.w3;
  p.w1_stride = a.w1_stride;
  p.B = a.n_seq, p.L = a.seq_len, p.D = a.d, p.ldw = a.d + 4;
  p.n_rows = a.n_seq * a.seq_len, p.n_tiles = hg_tiles(p.n_rows);
  p.spu = a.seq_len <= 32 ? 32 / a.seq_len : 1;
  p.n_units = (a.n_seq + p.spu - 1) / p.spu;
  p.w = a.w, p.arg = a.arg;
  RSA_CHECK_ARG(p.n_tiles + a.n_seq < (1ll << 31), "%s: too many rows for one launch", fn);
  return RSA_OK;
}

}  // namespace rsa

using namespace rsa;

extern "C" int64_t rsa_hgn_gating_workspace_bytes(int64_t n_seq, int32_t seq_len, int32_t d) {
  if (n_seq < 0 || seq_len < 1 || !hg_dim_ok(d) || n_seq > (1ll << 40) / seq_len) return -1;
  Carver cv(nullptr);
  hg_layout(cv, n_seq, seq_len, d);
  return cv.bytes() + 256;
}

extern "C" int rsa_hgn_gating(const rsa_hgn_gating_args* args, rsa_stream_t stream) {
  const char* fn = "rsa_hgn_gating";
  rsa_hgn_gating_args a;
  if (int rc = load_args(a, args, fn)) return rc;
  HgParams p{};
  if (int rc = hg_check(a, fn, p)) return rc;
  if (a.n_seq == 0) return RSA_OK;
  RSA_CHECK_ARG(a.out != nullptr, "%s: out is null", fn);
  p.out = a.out;
  const int64_t lds = hg_lds_bytes(a.d, a.d);
  const unsigned blocks = grid_1d(p.n_units, 4, HG_FORWARD_GRID);
  int rc = RSA_OK;
  dispatch_int<1, 2, 4>(a.d / 32, [&](auto NCB) {
    dispatch_bool(a.pooling == 1, [&](auto MAXP) {
      rc = allow_lds<hg_forward_kernel<NCB(), MAXP()>>(lds, fn);
      if (rc == RSA_OK)
        hipLaunchKernelGGL((hg_forward_kernel<NCB(), MAXP()>), dim3(blocks), dim3(256), (size_t)lds, (hipStream_t)stream, p);
    });
  });
  if (rc) return rc;
  RSA_CHECK_LAUNCH(fn);
  return RSA_OK;
}

extern "C" int rsa_hgn_gating_backward(const rsa_hgn_gating_args* args, rsa_stream_t stream) {
  const char* fn = "rsa_hgn_gating_backward";
  rsa_hgn_gating_args a;
  if (int rc = load_args(a, args, fn)) return rc;
  HgParams p{};
  if (int rc = hg_check(a, fn, p)) return rc;
  if (a.n_seq == 0) return RSA_OK;
  RSA_CHECK_ARG(a.g_out && ((uintptr_t)a.g_out & 15) == 0, "%s: g_out is null or not 16-byte aligned", fn);
  RSA_CHECK_ARG(a.ds && a.dug && a.dui && a.dw1 && a.dw3, "%s: ds, dug, dui, dw1 or dw3 is null", fn);
  RSA_CHECK_ARG(a.workspace != nullptr, "%s: workspace is null", fn);
  const int64_t need = rsa_hgn_gating_workspace_bytes(a.n_seq, a.seq_len, a.d);
  RSA_CHECK_ARG(a.workspace_bytes >= need, "%s: the workspace is too small: %lld bytes, need %lld", fn, (long long)a.workspace_bytes,
                (long long)need);
  Carver cv(a.workspace);
  const HgLayout L = hg_layout(cv, a.n_seq, a.seq_len, a.d);
  p.g = a.g_out;
  p.ds = a.ds, p.dug = a.dug, p.dui = a.dui, p.dw1 = a.dw1, p.dw3 = a.dw3;
  p.q = L.q, p.den = L.den, p.gp = L.gp, p.pw = L.pw, p.pw3 = L.pw3, p.pq = L.pq, p.n_slots = L.slots;
  hipStream_t s = (hipStream_t)stream;
  const int64_t lds = hg_lds_bytes(a.d, a.d);
  const unsigned blocks = grid_1d(p.n_tiles, 4, HG_ROWS_GRID);
  const bool maxp = a.pooling == 1;
  int rc = RSA_OK;
  if (!maxp) {
    dispatch_int<1, 2, 4>(a.d / 32, [&](auto NCB) {
      rc = allow_lds<hg_stats_kernel<NCB()>>(lds, fn);
      if (rc == RSA_OK) hipLaunchKernelGGL((hg_stats_kernel<NCB()>), dim3(blocks), dim3(256), (size_t)lds, s, p);
    });
    if (rc) return rc;
    RSA_CHECK_LAUNCH(fn);
    hipLaunchKernelGGL(hg_seq_kernel, dim3((unsigned)((a.n_seq + 255) / 256)), dim3(256), 0, s, p);
    RSA_CHECK_LAUNCH(fn);
  }
  dispatch_int<1, 2, 4>(a.d / 32, [&](auto NCB) {
    dispatch_bool(maxp, [&](auto MAXP) {
      rc = allow_lds<hg_rows_kernel<NCB(), MAXP()>>(lds, fn);
      if (rc == RSA_OK) hipLaunchKernelGGL((hg_rows_kernel<NCB(), MAXP()>), dim3(blocks), dim3(256), (size_t)lds, s, p);
    });
  });
  if (rc) return rc;
  RSA_CHECK_LAUNCH(fn);
  dispatch_int<1, 2, 4>(a.d / 32, [&](auto KB32) {
    dispatch_bool(maxp, [&](auto MAXP) {
      hipLaunchKernelGGL((hg_weights_kernel<KB32(), MAXP()>), dim3(L.groups, (unsigned)(a.d / 32)), dim3(256),
                         (size_t)hg_lds_bytes(a.d, 32), s, p);
    });
  });
  RSA_CHECK_LAUNCH(fn);
  const int64_t outs = (int64_t)a.d * a.d + a.d + a.n_seq * a.d;
  hipLaunchKernelGGL(hg_reduce_kernel, dim3((unsigned)((outs + 255) / 256)), dim3(256), 0, s, p);
  RSA_CHECK_LAUNCH(fn);
  return RSA_OK;
}
