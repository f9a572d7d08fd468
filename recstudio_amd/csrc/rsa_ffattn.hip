// Feed-forward (additive) attention pooling of the sequence towers NARM and STAMP, fused (gfx950): forward and backward.
//
// rsa_ff_attention / rsa_ff_attention_backward : AttentionLayer(attention_type='feedforward').forward with ONE query per
//                                                sequence, softmax=False and value = key   recstudio/model/module/layers.py:322-399
//
//   hid_bs = sigmoid(qh_b + W_k k_bs)    a_bs = key_pad[b, s] ? 0 : (w2 . hid_bs + b2) * scale    out_b = sum_s a_bs k_bs
//
// qh = W1[:, :q_dim] q (+ b1) is the caller's small GEMM; W_k = W1[:, q_dim:] is handed over as a column block of W1 (pointer +
// row stride), b2 as a device pointer.  D (key width) and M (hidden width) are each 32, 64 or 128.
//
// TILE.  The rows are the B * S positions, flat.  A wave owns 32 of them and all M hidden units of them; the product runs on
// v_mfma_f32_32x32x2_f32 TRANSPOSED as in rsa_combine.hip -- W_k is the A operand (M = hidden unit), the key rows the B operand
// (N = row) -- so lane (j, hh) ends up with row j of the tile in its registers, hidden unit 32 cb + (r & 3) + 8 (r >> 2) + 4 hh in
// register r of accumulator block cb.  The bias add, the sigmoid and the dot with w2 then happen inside a lane; the row's score
// needs ONE shuffle (the two halves hh).  Step 4 u + i of the K loop multiplies k = 8 u + i (hh = 0) and k = 8 u + 4 + i (hh = 1):
// a lane reads one 16-byte piece of its key row and of each weight row per four steps.
// S is free, so a tile may hold parts of several sequences (S = 1: 32 of them) and a sequence may span several tiles: a lane finds
// its sequence as row / S and reads its own qh row (16 bytes per four registers; neighbouring lanes mostly share it).
//
// FORWARD (ff_forward_kernel).  out_b sums over the rows of a sequence, i.e. ACROSS lanes and, for S > 32, across tiles.  To do
// that without atomics and without partial slots a workgroup owns WHOLE sequences: a group of G = ceil(256 / S) of them (one when
// S >= 256), whose G S rows it cuts into 32-row tiles starting at the group's first row (the last tile of a group is partial: at
// most 31 of >= 256 rows idle).  Its four waves take the tiles in turn and write `a`; after a barrier wave w pools sequences
// w, w + 4, ... of the group: D / 4 lanes cover a row with 16-byte loads, the 64 / (D / 4) lane groups take every such-th
// position, and a fixed butterfly adds the groups.  The pooling reads the group's keys a second time, <= 256 rows (128 KB at
// D = 128) that the same compute unit loaded a few microseconds before: HBM sees the keys once.  A workgroup strides over groups,
// so W_k is staged once per workgroup.
//
// WEIGHTS IN LDS.  Row c of W_k at c * (D + 4) floats, w2 behind it: the stride is 4 mod 8 floats, so "lane j reads 16 bytes of
// row j" is conflict-free, and so is the second product's W_k[c][32 kb + j] (rsa_combine.hip, "WEIGHTS IN LDS").  Bytes:
// M (D + 4) 4 + 4 M -- 68 KB at 128 x 128 (two workgroups per CU), 17 KB at 64 x 64.
//
// BACKWARD.  Nothing is saved: hid and a are recomputed from key and qh.
//   rows pass     (ff_rows_kernel, the forward's layout, flat tiles)  per row: da = g_b . k (accumulated in the K loop from the
//                 pieces of the key row the lane holds anyway, one shuffle), de = live ? da * scale : 0, a as in the forward,
//                 dpre = (de * w2) * (hid * (1 - hid)) in place of the accumulators.  dpre is then the A operand of the second
//                 product (M = row, K pair of step t = the two hidden units register t holds): W_k^T dpre comes out with N = key
//                 column on the lanes, and dkey = a g_b + W_k^T dpre is written in 128-byte pieces, +0 at padded rows.  de of
//                 every row goes to the workspace (B S floats).
//   weights pass  (ff_weights_kernel)  dW_k = dpre^T k, dw2 = sum de hid and db2 = sum de contract over ROWS, dqh_b = sum_s dpre_bs
//                 over the rows of one sequence: all need dpre with M = hidden unit and the rows as K pairs, the layout the
//                 UNTRANSPOSED product leaves.  A wave takes one block of 32 hidden units (blockIdx.y), recomputes that block of
//                 hid for its tiles the other way round and rebuilds dpre from the rows pass's de.  dW_k [32, D] stays in
//                 accumulators over all its tiles.  dqh is one more MFMA chain per tile whose B operand is the 0 / 1 matrix "row
//                 belongs to the j-th sequence of this tile" (exact products): the result holds the tile's share of each of its
//                 <= 32 sequences and goes to slot (tile + b) of the workspace -- (tile, b) pairs are monotone in both, so the sum
//                 is a unique index, and there are fewer than n_tiles + B of them.
//   reduce        (ff_reduce_kernel)  one thread per element of dW_k, dw2, db2 adds the waves' slots in ascending order; one per
//                 element of dqh adds the pair slots of its sequence's tiles in ascending tile order.
// No float atomics anywhere: two runs are bit-equal.  All element offsets are 64-bit.
//
// flops per row: forward 2 M D (+ 2 D pooling); backward 2 M D (rows, product) + 2 M D (W_k^T dpre) + 2 M D (weights, product)
// + 2 M D (dW_k) + 64 M (dqh).  Bytes per row: forward 4 D read + 4 written (+ 4 D from cache); backward 2 * 4 D read + 4 D written.
//
// REGISTERS (profiles/ff_attention_resources.txt).  Forward at M = 32 / 64 / 128: 91 / 124 / 192 VGPRs + 16 / 32 / 64 accumulator
// registers, 4 / 3 / 2 waves per SIMD, no scratch.  Rows pass: 247 / 256 / 256 VGPRs (+ 250 accumulator registers at M = 128, one
// wave per SIMD); with up to two accumulator blocks it is held to 256 registers (__launch_bounds__(256, 2), as rsa_combine.hip's
// backward) and spills 160 bytes per lane at M = 64 (a cost in time only).  Weights pass at D = 32 / 64 / 128: 144 / 161 / 138 + 80.
// MEASURED (tools/bench_ff_attention.py, B = 8192): forward 0.41 ms and forward + backward 1.77 ms at S = 50, D = M = 128 -- 0.21 and
// 0.24 of the fp32-matrix floor, 0.07 and 0.06 of the 8 TB/s byte model: at neither floor.
#include <utility>

#include "rsa_lds.hpp"

namespace rsa {

using f32x16 = float __attribute__((ext_vector_type(16)));

constexpr int FF_GROUP_ROWS = 256;           // a forward workgroup owns ceil(256 / S) whole sequences at a time
constexpr int FF_FORWARD_GRID = 1024;
constexpr int FF_ROWS_GRID = 2048;
constexpr int FF_WEIGHT_GROUPS = 128;        // workgroups per hidden block of the weights pass: 4 * 128 partial slots at most

extern __shared__ __attribute__((aligned(16))) float ff_smem[];

struct FfParams {
  const float *key, *qh, *wk, *w2, *b2, *g;
  const uint8_t* pad;
  int64_t wk_stride;
  int64_t B, n_rows, n_tiles, n_groups;
  int S, D, M, ldw, G;                        // ldw = D + 4; G: sequences per forward group
  float scale;
  float *out, *a;
  float *dkey, *dqh, *dwk, *dw2, *db2;
  float* de;                                  // [n_rows]
  float *pw, *pw2, *pb2;                      // [slots][M][D], [slots][M], [slots]
  float* pq;                                  // [n_tiles + B][M]
  int n_slots;
};

__device__ __forceinline__ int ff_row32(int r, int hh) { return (r & 3) + 8 * (r >> 2) + 4 * hh; }
__device__ __forceinline__ float ff_sigmoid(float x) { return 1.f / (1.f + expf(-x)); }
__device__ __forceinline__ float4 ff_ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }

template <class F, int... I>
__device__ __forceinline__ void ff_each(F&& f, std::integer_sequence<int, I...>) {
  (f(std::integral_constant<int, I>{}), ...);
}
template <int N, class F>
__device__ __forceinline__ void ff_blocks(F&& f) {
  ff_each(static_cast<F&&>(f), std::make_integer_sequence<int, N>{});
}

// rows [c0, c0 + rows) of W_k and of w2 into LDS; ends with a barrier
__device__ __forceinline__ void ff_stage(const FfParams& p, int c0, int rows, float* ws, float* w2s) {
  const int k4 = p.D >> 2;
  for (int i = threadIdx.x; i < rows * k4; i += blockDim.x) {
    const int r = i / k4, k = (i - r * k4) * 4;
    *reinterpret_cast<float4*>(ws + r * p.ldw + k) = ff_ld4(p.wk + (int64_t)(c0 + r) * p.wk_stride + k);
  }
  for (int i = threadIdx.x; i < rows; i += blockDim.x) w2s[i] = p.w2[c0 + i];
  __syncthreads();
}

// W_k k of the 32 rows the lanes' pointers `kr` name (lane (j, hh): row j), against the NCB staged hidden blocks.
// ROWS_N: sa[cb][r] of lane (j, hh) = hidden unit 32 cb + row32(r, hh) of row j; otherwise row row32(r, hh), hidden unit 32 cb + j.
// WITH_G: returns the lane's half of g . k (`gr`: the row's g_out row).
template <int NCB, bool ROWS_N, bool WITH_G>
__device__ __forceinline__ float ff_product(const FfParams& p, const float* ws, const float* kr, const float* gr, int lane,
                                            f32x16 (&sa)[NCB]) {
  const int j = lane & 31, hh = lane >> 5;
#pragma unroll
  for (int cb = 0; cb < NCB; ++cb) sa[cb] = f32x16{0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  float dot = 0.f;
  for (int k0 = 4 * hh; k0 < p.D; k0 += 8) {
    const float4 kv4 = ff_ld4(kr + k0);
    const float kv[4] = {kv4.x, kv4.y, kv4.z, kv4.w};
    if constexpr (WITH_G) {
      const float4 gv = ff_ld4(gr + k0);
      dot += (kv4.x * gv.x + kv4.y * gv.y) + (kv4.z * gv.z + kv4.w * gv.w);
    }
#pragma unroll
    for (int cb = 0; cb < NCB; ++cb) {
      const float4 w4 = ff_ld4(ws + (cb * 32 + j) * p.ldw + k0);
      const float wv[4] = {w4.x, w4.y, w4.z, w4.w};
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        if constexpr (ROWS_N) sa[cb] = __builtin_amdgcn_mfma_f32_32x32x2f32(wv[i], kv[i], sa[cb], 0, 0, 0);
        else sa[cb] = __builtin_amdgcn_mfma_f32_32x32x2f32(kv[i], wv[i], sa[cb], 0, 0, 0);
      }
    }
  }
  return dot;
}

// hid in place of the pre-activations (ROWS_N layout); returns w2 . hid of the whole row
template <int NCB>
__device__ __forceinline__ float ff_hidden(const float* qr, const float* w2s, int hh, f32x16 (&sa)[NCB]) {
  float e = 0.f;
  ff_blocks<NCB>([&](auto CB) {
    constexpr int cb = decltype(CB)::value;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int c0 = cb * 32 + 8 * g + 4 * hh;
      const float4 q4 = ff_ld4(qr + c0), w4 = ff_ld4(w2s + c0);
      const float qv[4] = {q4.x, q4.y, q4.z, q4.w}, wv[4] = {w4.x, w4.y, w4.z, w4.w};
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float hid = ff_sigmoid(sa[cb][4 * g + i] + qv[i]);
        sa[cb][4 * g + i] = hid;
        e += wv[i] * hid;
      }
    }
  });
  return e + __shfl_xor(e, 32, 64);
}

template <int NCB>
__global__ __launch_bounds__(256) void ff_forward_kernel(const FfParams p) {
  float* ws = ff_smem;
  float* w2s = ws + p.M * p.ldw;
  ff_stage(p, 0, p.M, ws, w2s);
  const float b2 = p.b2[0];
  const int lane = lane_id(), wave = threadIdx.x >> 6, j = lane & 31, hh = lane >> 5;
  const int lpr = p.D >> 2, nsl = 64 / lpr, sl = lane / lpr, d0 = (lane - sl * lpr) * 4;     // the pooling's lane roles
  for (int64_t grp = blockIdx.x; grp < p.n_groups; grp += gridDim.x) {
    const int64_t b0 = grp * p.G, b1 = b0 + p.G < p.B ? b0 + p.G : p.B;
    const int64_t r0 = b0 * p.S, r1 = b1 * p.S;
    const int n_t = (int)((r1 - r0 + 31) / 32);
    for (int t = wave; t < n_t; t += 4) {
      const int64_t row = r0 + 32 * t + j;
      const bool ok = row < r1;
      const int64_t rowc = ok ? row : r1 - 1;                     // (a row that exists; its result is not stored)
      const int64_t b = b0 + (unsigned)(rowc - r0) / (unsigned)p.S;
      f32x16 sa[NCB];
      ff_product<NCB, true, false>(p, ws, p.key + rowc * p.D, nullptr, lane, sa);
      const float e = ff_hidden<NCB>(p.qh + b * p.M, w2s, hh, sa);
      const bool live = !(p.pad && p.pad[rowc]);
      if (ok && hh == 0) p.a[row] = live ? (e + b2) * p.scale : 0.f;
    }
    __syncthreads();                                              // the group's `a` is written (same CU: visible after the barrier)
    for (int64_t b = b0 + wave; b < b1; b += 4) {
      const float* kb = p.key + b * p.S * p.D + d0;
      const float* ab = p.a + b * p.S;
      float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll 4
      for (int s = sl; s < p.S; s += nsl) {
        const float av = ab[s];
        const float4 kv = ff_ld4(kb + (int64_t)s * p.D);
        acc.x += av * kv.x, acc.y += av * kv.y, acc.z += av * kv.z, acc.w += av * kv.w;
      }
      for (int m = 32; m >= lpr; m >>= 1) {
        acc.x += __shfl_xor(acc.x, m, 64), acc.y += __shfl_xor(acc.y, m, 64);
        acc.z += __shfl_xor(acc.z, m, 64), acc.w += __shfl_xor(acc.w, m, 64);
      }
      if (sl == 0) *reinterpret_cast<float4*>(p.out + b * p.D + d0) = acc;
    }
  }
}

template <int NCB>
__global__ __launch_bounds__(256, NCB <= 2 ? 2 : 1) void ff_rows_kernel(const FfParams p) {
  float* ws = ff_smem;
  float* w2s = ws + p.M * p.ldw;
  ff_stage(p, 0, p.M, ws, w2s);
  const float b2 = p.b2[0];
  const int lane = lane_id(), wave = threadIdx.x >> 6, j = lane & 31, hh = lane >> 5;
  for (int64_t tile = (int64_t)blockIdx.x * 4 + wave; tile < p.n_tiles; tile += (int64_t)gridDim.x * 4) {
    const int64_t row0 = tile * 32, row = row0 + j;
    const bool ok = row < p.n_rows;
    const int64_t rowc = ok ? row : p.n_rows - 1;
    const int64_t bq = row0 / p.S;                                // the tile's first sequence, and where in it the tile starts
    const unsigned rem = (unsigned)(row0 - bq * p.S);
    const int64_t b = rowc / p.S;
    f32x16 sa[NCB];
    float dot = ff_product<NCB, true, true>(p, ws, p.key + rowc * p.D, p.g + b * p.D, lane, sa);
    dot += __shfl_xor(dot, 32, 64);
    const float e = ff_hidden<NCB>(p.qh + b * p.M, w2s, hh, sa);
    const bool live = ok && !(p.pad && p.pad[rowc]);
    const float av = live ? (e + b2) * p.scale : 0.f;
    const float de = live ? dot * p.scale : 0.f;
    if (ok && hh == 0) p.de[row] = de;
    // ---- dpre in place of hid
    ff_blocks<NCB>([&](auto CB) {
      constexpr int cb = decltype(CB)::value;
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const float4 w4 = ff_ld4(w2s + cb * 32 + 8 * g + 4 * hh);
        const float wv[4] = {w4.x, w4.y, w4.z, w4.w};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const float hid = sa[cb][4 * g + i];
          sa[cb][4 * g + i] = (de * wv[i]) * (hid * (1.f - hid));
        }
      }
    });
    // ---- a, liveness and g row of the 16 rows this lane stores
    float ar[16];
    int sq[16];                                                   // which of the tile's sequences; < 0: a padded row (or none)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int off = ff_row32(r, hh);
      ar[r] = __shfl(av, off, 64);
      const int lv = __shfl((int)live, off, 64);
      sq[r] = lv ? (int)((rem + (unsigned)off) / (unsigned)p.S) : -1;
    }
    // ---- dkey = a g + W_k^T dpre, one block of 32 key columns at a time
    for (int kb = 0; kb < (p.D >> 5); ++kb) {
      const int kin = kb * 32 + j;
      f32x16 da = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
      for (int cb = 0; cb < NCB; ++cb)
#pragma unroll
        for (int t2 = 0; t2 < 16; ++t2)
          da = __builtin_amdgcn_mfma_f32_32x32x2f32(sa[cb][t2], ws[(cb * 32 + ff_row32(t2, hh)) * p.ldw + kin], da, 0, 0, 0);
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int64_t rr = row0 + ff_row32(r, hh);
        if (rr < p.n_rows) p.dkey[rr * p.D + kin] = sq[r] >= 0 ? ar[r] * p.g[(bq + sq[r]) * p.D + kin] + da[r] : 0.f;
      }
    }
  }
}

template <int KB32>
__global__ __launch_bounds__(256, KB32 <= 2 ? 2 : 1) void ff_weights_kernel(const FfParams p) {
  float* ws = ff_smem;
  float* w2s = ws + 32 * p.ldw;
  const int cb = blockIdx.y;
  ff_stage(p, cb * 32, 32, ws, w2s);
  const int lane = lane_id(), wave = threadIdx.x >> 6, j = lane & 31, hh = lane >> 5;
  const int c = cb * 32 + j;
  const float w2c = w2s[j];
  f32x16 dw[KB32];
#pragma unroll
  for (int kb = 0; kb < KB32; ++kb) dw[kb] = f32x16{0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  float dw2 = 0.f, db2 = 0.f;
  for (int64_t tile = (int64_t)blockIdx.x * 4 + wave; tile < p.n_tiles; tile += (int64_t)gridDim.x * 4) {
    const int64_t row0 = tile * 32;
    const int64_t rowc = row0 + j < p.n_rows ? row0 + j : p.n_rows - 1;
    const int64_t bq = row0 / p.S;
    const unsigned rem = (unsigned)(row0 - bq * p.S);
    f32x16 sa[1];
    ff_product<1, false, false>(p, ws, p.key + rowc * p.D, nullptr, lane, sa);
    float ds[16];
    int sq[16];                                                   // which of the tile's sequences the row belongs to; -1: no row
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int off = ff_row32(r, hh);
      const int64_t rr = row0 + off;
      ds[r] = 0.f;
      sq[r] = -1;
      if (rr < p.n_rows) {
        const int slot = (int)((rem + (unsigned)off) / (unsigned)p.S);
        const float hid = ff_sigmoid(sa[0][r] + p.qh[(bq + slot) * p.M + c]);
        const float de = p.de[rr];
        ds[r] = (de * w2c) * (hid * (1.f - hid));
        dw2 += de * hid;
        db2 += de;
        sq[r] = slot;
      }
    }
    f32x16 dq = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int t = 0; t < 16; ++t) {
      const int64_t rr = row0 + ff_row32(t, hh);
#pragma unroll
      for (int kb = 0; kb < KB32; ++kb) {
        const float kv = rr < p.n_rows ? p.key[rr * p.D + kb * 32 + j] : 0.f;
        dw[kb] = __builtin_amdgcn_mfma_f32_32x32x2f32(ds[t], kv, dw[kb], 0, 0, 0);
      }
      dq = __builtin_amdgcn_mfma_f32_32x32x2f32(ds[t], sq[t] == j ? 1.f : 0.f, dq, 0, 0, 0);
    }
    // the tile's share of dqh of its j-th sequence: hidden unit 32 cb + row32(r, hh) in register r
    const int64_t last = row0 + 31 < p.n_rows ? row0 + 31 : p.n_rows - 1;
    const int last_slot = (int)((rem + (unsigned)(last - row0)) / (unsigned)p.S);
    if (j <= last_slot) {
      float* dst = p.pq + (tile + bq + j) * p.M + cb * 32;
#pragma unroll
      for (int r = 0; r < 16; ++r) dst[ff_row32(r, hh)] = dq[r];
    }
  }
  // the wave's partial sums, in its own slot (a wave without a tile writes zeros)
  dw2 += __shfl_xor(dw2, 32, 64);
  db2 += __shfl_xor(db2, 32, 64);
  const int64_t slot = (int64_t)blockIdx.x * 4 + wave;
  float* pw = p.pw + slot * p.M * p.D;
#pragma unroll
  for (int kb = 0; kb < KB32; ++kb)
#pragma unroll
    for (int r = 0; r < 16; ++r) pw[(int64_t)(cb * 32 + ff_row32(r, hh)) * p.D + kb * 32 + j] = dw[kb][r];
  if (hh == 0) p.pw2[slot * p.M + c] = dw2;
  if (cb == 0 && lane == 0) p.pb2[slot] = db2;
}

// One thread per element of dW_k, dw2, db2 (the waves' slots added in ascending order, eight loads in flight) and of dqh (the
// pair slots of the sequence's tiles, ascending).
__global__ __launch_bounds__(256) void ff_reduce_kernel(const FfParams p) {
  const int64_t tid = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t nw = (int64_t)p.M * p.D;
  const float* src;
  float* dst;
  int64_t stride;
  if (tid < nw) {
    src = p.pw + tid, stride = nw, dst = p.dwk + tid;
  } else if (tid < nw + p.M) {
    src = p.pw2 + (tid - nw), stride = p.M, dst = p.dw2 + (tid - nw);
  } else if (tid == nw + p.M) {
    src = p.pb2, stride = 1, dst = p.db2;
  } else {
    const int64_t e = tid - (nw + p.M + 1);
    if (e >= p.B * p.M) return;
    const int64_t b = e / p.M, m = e - b * p.M;
    const int64_t t0 = b * p.S / 32, t1 = ((b + 1) * p.S - 1) / 32;
    float acc = 0.f;
    for (int64_t t = t0; t <= t1; ++t) acc += p.pq[(t + b) * p.M + m];
    p.dqh[e] = acc;
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

struct FfLayout {
  float *de, *pw, *pw2, *pb2, *pq;
  unsigned groups;
  int slots;
};

static inline bool ff_dim_ok(int d) { return d == 32 || d == 64 || d == 128; }
static inline int64_t ff_tiles(int64_t n_rows) { return (n_rows + 31) / 32; }

static inline FfLayout ff_layout(Carver& cv, int64_t n_seq, int64_t seq_len, int d, int m) {
  FfLayout L;
  const int64_t n_rows = n_seq * seq_len, n_tiles = ff_tiles(n_rows);
  L.groups = grid_1d(n_tiles, 4, FF_WEIGHT_GROUPS);
  L.slots = (int)L.groups * 4;
  L.de = cv.take<float>(n_rows);
  L.pw = cv.take<float>((int64_t)L.slots * m * d);
  L.pw2 = cv.take<float>((int64_t)L.slots * m);
  L.pb2 = cv.take<float>(L.slots);
  L.pq = cv.take<float>((n_tiles + n_seq) * m);
  return L;
}

static inline int64_t ff_lds_bytes(int d, int rows) { return ((int64_t)rows * (d + 4) + rows) * 4; }

// the checks both entry points share (everything but the outputs); fills the shared part of `p`
static int ff_check(const rsa_ff_attention_args& a, const char* fn, FfParams& p) {
  RSA_CHECK_ARG(a.n_seq >= 0, "%s: negative n_seq %lld", fn, (long long)a.n_seq);
  RSA_CHECK_ARG(a.seq_len >= 1, "%s: seq_len must be at least 1, got %d", fn, a.seq_len);
  RSA_CHECK_ARG(ff_dim_ok(a.d) && ff_dim_ok(a.m), "%s: d and m must each be 32, 64 or 128 (W_k is kept in LDS and in at most 4 "
                "accumulator blocks), got %d and %d", fn, a.d, a.m);
  RSA_CHECK_ARG(std::isfinite(a.scale), "%s: scale must be finite", fn);
  RSA_CHECK_ARG(a.n_seq <= (1ll << 40) / a.seq_len, "%s: n_seq * seq_len is too large", fn);
  if (a.n_seq == 0) return RSA_OK;
  RSA_CHECK_ARG(a.key && a.qh && a.w_k && a.w2 && a.b2, "%s: key, qh, w_k, w2 or b2 is null", fn);
  RSA_CHECK_ARG((((uintptr_t)a.key | (uintptr_t)a.qh | (uintptr_t)a.w_k) & 15) == 0 && a.w_k_stride % 4 == 0 && a.w_k_stride >= a.d,
                "%s: key, qh and w_k must be 16-byte aligned, the row stride of w_k a multiple of 4 and at least d (stride %lld)",
                fn, (long long)a.w_k_stride);
  p.key = a.key, p.qh = a.qh, p.wk = a.w_k, p.w2 = a.w2, p.b2 = a.b2, p.pad = a.key_pad;
  p.wk_stride = a.w_k_stride;
  p.B = a.n_seq, p.S = a.seq_len, p.D = a.d, p.M = a.m, p.ldw = a.d + 4;
  p.n_rows = a.n_seq * a.seq_len, p.n_tiles = ff_tiles(p.n_rows);
  p.G = (int)((FF_GROUP_ROWS + (int64_t)a.seq_len - 1) / a.seq_len);
  p.n_groups = (a.n_seq + p.G - 1) / p.G;
  p.scale = a.scale;
  RSA_CHECK_ARG(p.n_tiles + a.n_seq < (1ll << 31), "%s: too many rows for one launch", fn);
  return RSA_OK;
}

}  // namespace rsa

using namespace rsa;

extern "C" int64_t rsa_ff_attention_workspace_bytes(int64_t n_seq, int32_t seq_len, int32_t d, int32_t m) {
  if (n_seq < 0 || seq_len < 1 || !ff_dim_ok(d) || !ff_dim_ok(m) || n_seq > (1ll << 40) / seq_len) return -1;
  Carver cv(nullptr);
  ff_layout(cv, n_seq, seq_len, d, m);
  return cv.bytes() + 256;
}

extern "C" int rsa_ff_attention(const rsa_ff_attention_args* args, rsa_stream_t stream) {
  const char* fn = "rsa_ff_attention";
  rsa_ff_attention_args a;
  if (int rc = load_args(a, args, fn)) return rc;
  FfParams p{};
  if (int rc = ff_check(a, fn, p)) return rc;
  if (a.n_seq == 0) return RSA_OK;
  RSA_CHECK_ARG(a.out && a.a && ((uintptr_t)a.out & 15) == 0, "%s: out or a is null, or out is not 16-byte aligned", fn);
  p.out = a.out, p.a = a.a;
  const int64_t lds = ff_lds_bytes(a.d, a.m);
  const unsigned blocks = grid_1d(p.n_groups, 1, FF_FORWARD_GRID);
  int rc = RSA_OK;
  dispatch_int<1, 2, 4>(a.m / 32, [&](auto NCB) {
    rc = allow_lds<ff_forward_kernel<NCB()>>(lds, fn);
    if (rc == RSA_OK) hipLaunchKernelGGL((ff_forward_kernel<NCB()>), dim3(blocks), dim3(256), (size_t)lds, (hipStream_t)stream, p);
  });
  if (rc) return rc;
  RSA_CHECK_LAUNCH(fn);
  return RSA_OK;
}

extern "C" int rsa_ff_attention_backward(const rsa_ff_attention_args* args, rsa_stream_t stream) {
  const char* fn = "rsa_ff_attention_backward";
  rsa_ff_attention_args a;
  if (int rc = load_args(a, args, fn)) return rc;
  FfParams p{};
  if (int rc = ff_check(a, fn, p)) return rc;
  if (a.n_seq == 0) return RSA_OK;
  RSA_CHECK_ARG(a.g_out && ((uintptr_t)a.g_out & 15) == 0, "%s: g_out is null or not 16-byte aligned", fn);
  RSA_CHECK_ARG(a.dkey && a.dqh && a.dw_k && a.dw2 && a.db2, "%s: dkey, dqh, dw_k, dw2 or db2 is null", fn);
  RSA_CHECK_ARG(a.workspace != nullptr, "%s: workspace is null", fn);
  const int64_t need = rsa_ff_attention_workspace_bytes(a.n_seq, a.seq_len, a.d, a.m);
  RSA_CHECK_ARG(a.workspace_bytes >= need, "%s: the workspace is too small: %lld bytes, need %lld", fn, (long long)a.workspace_bytes,
                (long long)need);
  Carver cv(a.workspace);
  const FfLayout L = ff_layout(cv, a.n_seq, a.seq_len, a.d, a.m);
  p.g = a.g_out;
  p.dkey = a.dkey, p.dqh = a.dqh, p.dwk = a.dw_k, p.dw2 = a.dw2, p.db2 = a.db2;
  p.de = L.de, p.pw = L.pw, p.pw2 = L.pw2, p.pb2 = L.pb2, p.pq = L.pq, p.n_slots = L.slots;
  hipStream_t s = (hipStream_t)stream;
  const int64_t lds = ff_lds_bytes(a.d, a.m);
  const unsigned blocks = grid_1d(p.n_tiles, 4, FF_ROWS_GRID);
  int rc = RSA_OK;
  dispatch_int<1, 2, 4>(a.m / 32, [&](auto NCB) {
    rc = allow_lds<ff_rows_kernel<NCB()>>(lds, fn);
    if (rc == RSA_OK) hipLaunchKernelGGL((ff_rows_kernel<NCB()>), dim3(blocks), dim3(256), (size_t)lds, s, p);
  });
  if (rc) return rc;
  RSA_CHECK_LAUNCH(fn);
  dispatch_int<1, 2, 4>(a.d / 32, [&](auto KB32) {
    hipLaunchKernelGGL((ff_weights_kernel<KB32()>), dim3(L.groups, (unsigned)(a.m / 32)), dim3(256), (size_t)ff_lds_bytes(a.d, 32), s, p);
  });
  RSA_CHECK_LAUNCH(fn);
  const int64_t outs = (int64_t)a.m * a.d + a.m + 1 + a.n_seq * a.m;
  hipLaunchKernelGGL(ff_reduce_kernel, dim3((unsigned)((outs + 255) / 256)), dim3(256), 0, s, p);
  RSA_CHECK_LAUNCH(fn);
  return RSA_OK;
}
