// The attention core of the sequence towers (SASRec, BERT4Rec, CL4SRec ...), fused (gfx950): forward and backward.
//
// rsa_attention / rsa_attention_backward : the part of nn.MultiheadAttention between in_proj and out_proj, as the reference's
//                                          nn.TransformerEncoder runs it (recstudio/model/seq/sasrec.py:25-36, :60-63)
//
//   s_ij = scale <q_i, k_j>,  allowed(i, j) = (!causal or j <= i) and !key_pad[b, j],  P_i. = softmax over the allowed j,
//   Pt_ij = keep_ij P_ij / q,  out_i = sum_j Pt_ij v_j,  lse_i = log sum_allowed exp(s_ij)
//
// q, k, v are read where F.linear(x, in_proj_weight, in_proj_bias) left them: columns [0, D), [D, 2D), [2D, 3D) of qkv [B, L, 3D],
// head h in columns h dh .. (h + 1) dh of each.  No head-major copy, and nothing of size L x L ever reaches memory (the test-only
// `keep` aside).
//
// TILE.  L <= 64 fits one tile: LT = 16, 32 or 64 (the smallest that holds L) x dh = 16, 32 or 64 are template arguments.  A wave
// owns a block of 16 queries (and, in the second pass of the backward, 16 keys); a (b, h) problem is LT / 16 waves and a
// 256-thread workgroup holds 4, 2 or 1 problems -- an L = 9 batch pays for a 16 x 16 tile, not a 64 x 64 one.  One workgroup per
// 4 / 2 / 1 problems, one pass (no grid stride): the Q, K, V (and G) tiles of the problem are staged once into LDS with 16-byte
// loads (a head's row is 64-256 contiguous bytes), row r at r (dh + 4) floats, rows >= L zero; ONE barrier follows.
//
// PRODUCTS.  All on v_mfma_f32_16x16x4_f32 (fp32 in, fp32 out; 40-cycle dependent latency, which suits K loops this short).
// The forward takes the scores TRANSPOSED -- K is the A operand (M = key), Q the B operand (N = query) -- so lane (i, g) of the wave
// (i = lane & 15, g = lane >> 4) ends up with query i on the lane and keys 16 jb + 4 g + r in register r of block jb.  A softmax
// row is then spread over the registers of FOUR lanes: max and sum are two shuffles (xor 16, 32) after an in-lane pass.  And the
// result is already the B operand of the next product: out^T = V^T Pt^T sums over the ROW (register) index, step t of block jb
// takes register t -- P never goes through LDS.  out^T leaves 4 consecutive columns of a row in a lane: one 16-byte store each.
// K ORDER.  A 16-byte LDS read feeds four MFMA steps: step t multiplies elements k0 + 4 g + t of both operands (the same
// permutation on both sides, so the sum is over every k once).  Row stride dh + 4 floats = 4 mod 8: the ds_read_b128 of 16 rows
// starts in 16 different 4-bank slots.  The V^T / K^T / Q^T / G^T operands of the second products are one float per lane, 16
// consecutive floats per lane group, groups 4 rows = 16 banks apart: conflict-free.
// CAUSAL.  The key blocks above the diagonal are skipped (wave w computes w + 1 of them in the forward and the first backward
// pass, LT / 16 - w in the second: the waves of a problem do equal work).
//
// DROPOUT.  q = fp32(1 - p).  Element (b, h, i, j) is kept iff u < q, u = element ((b H + h) L + i) L + j of ONE
// torch.rand([B, H, L, L]) call (torch_rand_element), and P is then DIVIDED by q.  Disallowed positions own their index like any
// other (and are not evaluated unless `keep` is asked for).  p = 0 draws nothing.
//
// FULLY MASKED ROW.  A query without an allowed key gets out = 0, lse = -inf and passes no gradient (torch: NaN).
//
// BACKWARD.  From qkv, out, lse, g and the Philox state; S and P = exp(s - lse) are recomputed, the mask regenerated.
//   D_i = sum_c g_ic out_ic (at staging), dPt_ij = <g_i, v_j>, dS_ij = P_ij (keep_ij dPt_ij / q - D_i)
//   pass 1 (the forward's layout, the wave owns 16 queries)   dq_i = scale sum_j dS_ij k_j: dS^T is the B operand of K^T dS^T
//   pass 2 (untransposed: Q is A, K is B, the wave owns 16 keys, queries in the registers)
//                                                              dk_j = scale sum_i dS_ij q_i, dv_j = sum_i Pt_ij g_i: dS and Pt
//                                                              are the B operands of Q^T dS and G^T Pt
// Both sums run inside one wave, so there is no sum across waves: no atomics, no workspace, no P or dS in LDS (and one barrier);
// the price is that S, dPt and the mask are computed twice (7 tile products instead of 5).  Every element of dqkv is written,
// zeros where nothing flows.
//
// OCCUPANCY (LDS per workgroup: forward 3, backward 4 tiles of LT (dh + 4) floats per problem, + 2 LT floats in the backward).
//   LT 16: 4 problems per workgroup, 15-51 KB forward, 20-70 KB backward      LT 32: 2 problems, 15-51 KB, 20-70 KB
//   LT 64: 1 problem, 15 / 27 / 51 KB forward, 20 / 36 / 68 KB backward
// so at least three workgroups (12 waves) share a CU in the forward and two (8 waves) in the backward at dh = 64, more below.
// flops per problem: forward 4 L^2 dh, backward 14 L^2 dh (halved when causal).  Bytes per (b, l): forward 12 D read + 4 D
// written, backward 20 D read + 12 D written.
#include "rsa_lds.hpp"

namespace rsa {

using f32x4 = float __attribute__((ext_vector_type(4)));

constexpr int SA_MAX_L = 64;

extern __shared__ __attribute__((aligned(16))) float sa_smem[];

struct SaParams {
  const float* qkv;
  const uint8_t* key_pad;
  int64_t n_prob;                  // B * H
  int L, H, D;
  int causal, drop;
  float scale, q;
  PhiloxCall pc;
  float* out;                      // forward: written; backward: read
  float* lse;
  uint8_t* keep;
  const float* g;
  float* dqkv;
};

// rows [0, L) of one head's [L, DH] block (row stride `stride` floats) into LDS rows of DH + 4 floats; rows [L, LT) are zero
template <int LT, int DH>
__device__ __forceinline__ void sa_stage(const float* src, int64_t stride, int L, float* dst, int tp, int nthr) {
  constexpr int P4 = DH / 4, LD = DH + 4;
  for (int idx = tp; idx < LT * P4; idx += nthr) {
    const int r = idx / P4, c = (idx - r * P4) * 4;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (r < L) v = *reinterpret_cast<const float4*>(src + (int64_t)r * stride + c);
    *reinterpret_cast<float4*>(dst + r * LD + c) = v;
  }
}

// sum_k A[k] B[k] over the two staged rows: element r of the result is (row 4 g + r of the A block, the lane's row of the B block)
template <int DH>
__device__ __forceinline__ f32x4 sa_dot(const float* a_row, const float* b_row, int g) {
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int k0 = 0; k0 < DH; k0 += 16) {
    const float4 a = *reinterpret_cast<const float4*>(a_row + k0 + 4 * g);
    const float4 b = *reinterpret_cast<const float4*>(b_row + k0 + 4 * g);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, b.x, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, b.y, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, b.z, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, b.w, acc, 0, 0, 0);
  }
  return acc;
}

// acc[cb] += X_blk^T w: X_blk = 16 staged rows, w = a [16 rows, 16 lanes] tile in the accumulator layout (row 4 g + t in element t)
template <int DH>
__device__ __forceinline__ void sa_acc(const float* x_blk, const f32x4 w, f32x4 (&acc)[DH / 16], int j, int g) {
  constexpr int LD = DH + 4;
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int cb = 0; cb < DH / 16; ++cb)
      acc[cb] = __builtin_amdgcn_mfma_f32_16x16x4f32(x_blk[(4 * g + t) * LD + cb * 16 + j], w[t], acc[cb], 0, 0, 0);
}

// the dropout decision of element (i, j) of problem `pr`
__device__ __forceinline__ bool sa_kept(const SaParams& p, int64_t pr, int i, int j) {
  if (!p.drop) return true;
  return torch_rand_element(p.pc, ((uint64_t)pr * (uint64_t)p.L + (uint64_t)i) * (uint64_t)p.L + (uint64_t)j) < p.q;
}

template <int LT, int DH>
__global__ __launch_bounds__(256) void sa_forward_kernel(const SaParams p) {
  constexpr int NJB = LT / 16, NCB = DH / 16, NW = NJB, PPW = 4 / NW, LD = DH + 4, TILE = LT * LD;
  const int lane = lane_id(), wave = threadIdx.x >> 6, j16 = lane & 15, g = lane >> 4;
  const int slot = wave / NW, ib = wave % NW, tp = threadIdx.x - slot * NW * 64;
  const int64_t pr = (int64_t)blockIdx.x * PPW + slot;
  const bool live = pr < p.n_prob;
  const int64_t b = live ? pr / p.H : 0;
  const int h = live ? (int)(pr - b * p.H) : 0;
  float* qs = sa_smem + slot * 3 * TILE;
  float* ks = qs + TILE;
  float* vs = ks + TILE;
  const int64_t ld3 = 3 * (int64_t)p.D;
  if (live) {
    const float* src = p.qkv + b * p.L * ld3 + h * DH;
    sa_stage<LT, DH>(src, ld3, p.L, qs, tp, NW * 64);
    sa_stage<LT, DH>(src + p.D, ld3, p.L, ks, tp, NW * 64);
    sa_stage<LT, DH>(src + 2 * p.D, ld3, p.L, vs, tp, NW * 64);
  }
  __syncthreads();
  if (!live) return;
  const bool key_ok = lane < p.L && !(p.key_pad && p.key_pad[b * p.L + lane]);
  const uint64_t kmask = __ballot(key_ok);
  const int i = ib * 16 + j16;
  const bool i_ok = i < p.L;
  const int jb_end = p.causal ? ib + 1 : NJB;
  f32x4 s[NJB];
#pragma unroll
  for (int jb = 0; jb < NJB; ++jb)
    if (jb < jb_end) s[jb] = sa_dot<DH>(ks + (jb * 16 + j16) * LD, qs + i * LD, g);
  // ---- the row's softmax: the registers of the four lanes (i, 0..3)
  float m = -INFINITY;
#pragma unroll
  for (int jb = 0; jb < NJB; ++jb)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int j = jb * 16 + 4 * g + r;
      const bool ok = jb < jb_end && ((kmask >> j) & 1) && (!p.causal || j <= i);
      const float sv = ok ? s[jb][r] * p.scale : -INFINITY;
      s[jb][r] = sv;
      m = fmaxf(m, sv);
    }
  m = fmaxf(m, __shfl_xor(m, 16, 64));
  m = fmaxf(m, __shfl_xor(m, 32, 64));
  float sum = 0.f;
#pragma unroll
  for (int jb = 0; jb < NJB; ++jb)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float e = s[jb][r] == -INFINITY ? 0.f : expf(s[jb][r] - m);
      s[jb][r] = e;
      sum += e;
    }
  sum += __shfl_xor(sum, 16, 64);
  sum += __shfl_xor(sum, 32, 64);
  if (i_ok && g == 0) p.lse[pr * p.L + i] = sum > 0.f ? m + logf(sum) : -INFINITY;
  // ---- Pt = keep P / q, in place
#pragma unroll
  for (int jb = 0; jb < NJB; ++jb)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int j = jb * 16 + 4 * g + r;
      float pv = s[jb][r] != 0.f ? s[jb][r] / sum : 0.f;
      if (i_ok && j < p.L && (pv != 0.f || p.keep)) {
        const bool kept = sa_kept(p, pr, i, j);
        if (p.drop) pv = kept ? pv / p.q : 0.f;
        if (p.keep) p.keep[(pr * p.L + i) * p.L + j] = kept ? 1 : 0;
      }
      s[jb][r] = pv;
    }
  // ---- out^T = V^T Pt^T
  f32x4 o[NCB];
#pragma unroll
  for (int cb = 0; cb < NCB; ++cb) o[cb] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int jb = 0; jb < NJB; ++jb)
    if (jb < jb_end) sa_acc<DH>(vs + jb * 16 * LD, s[jb], o, j16, g);
  if (i_ok) {
    float* dst = p.out + (b * p.L + i) * (int64_t)p.D + h * DH + 4 * g;
#pragma unroll
    for (int cb = 0; cb < NCB; ++cb) *reinterpret_cast<float4*>(dst + cb * 16) = make_float4(o[cb][0], o[cb][1], o[cb][2], o[cb][3]);
  }
}

template <int LT, int DH>
__global__ __launch_bounds__(256) void sa_backward_kernel(const SaParams p) {
  constexpr int NJB = LT / 16, NCB = DH / 16, NW = NJB, PPW = 4 / NW, LD = DH + 4, TILE = LT * LD, P4 = DH / 4;
  constexpr int PER = 4 * TILE + 2 * LT;
  const int lane = lane_id(), wave = threadIdx.x >> 6, j16 = lane & 15, g = lane >> 4;
  const int slot = wave / NW, wb = wave % NW, tp = threadIdx.x - slot * NW * 64;
  const int64_t pr = (int64_t)blockIdx.x * PPW + slot;
  const bool live = pr < p.n_prob;
  const int64_t b = live ? pr / p.H : 0;
  const int h = live ? (int)(pr - b * p.H) : 0;
  float* qs = sa_smem + slot * PER;
  float* ks = qs + TILE;
  float* vs = ks + TILE;
  float* gs = vs + TILE;
  float* lse_s = gs + TILE;
  float* d_s = lse_s + LT;
  const int64_t ld3 = 3 * (int64_t)p.D;
  if (live) {
    const float* src = p.qkv + b * p.L * ld3 + h * DH;
    sa_stage<LT, DH>(src, ld3, p.L, qs, tp, NW * 64);
    sa_stage<LT, DH>(src + p.D, ld3, p.L, ks, tp, NW * 64);
    sa_stage<LT, DH>(src + 2 * p.D, ld3, p.L, vs, tp, NW * 64);
    // G, and D_i = <g_i, out_i>: a row is P4 consecutive lanes (LT * P4 is a multiple of 64: every lane makes every trip)
    const float* gsrc = p.g + b * p.L * (int64_t)p.D + h * DH;
    const float* osrc = p.out + b * p.L * (int64_t)p.D + h * DH;
    for (int idx = tp; idx < LT * P4; idx += NW * 64) {
      const int r = idx / P4, c = (idx - r * P4) * 4;
      float4 gv = make_float4(0.f, 0.f, 0.f, 0.f), ov = gv;
      if (r < p.L) {
        gv = *reinterpret_cast<const float4*>(gsrc + (int64_t)r * p.D + c);
        ov = *reinterpret_cast<const float4*>(osrc + (int64_t)r * p.D + c);
      }
      *reinterpret_cast<float4*>(gs + r * LD + c) = gv;
      const float di = group_sum<P4>((gv.x * ov.x + gv.y * ov.y) + (gv.z * ov.z + gv.w * ov.w));
      if (c == 0) d_s[r] = di;
    }
    for (int r = tp; r < LT; r += NW * 64) lse_s[r] = r < p.L ? p.lse[pr * p.L + r] : INFINITY;
  }
  __syncthreads();
  if (!live) return;
  const bool key_ok = lane < p.L && !(p.key_pad && p.key_pad[b * p.L + lane]);
  const uint64_t kmask = __ballot(key_ok);
  float* drow = p.dqkv + b * p.L * ld3 + h * DH + 4 * g;
  // ---- pass 1: the wave's 16 queries, keys in the registers: dq
  {
    const int i = wb * 16 + j16;
    const bool i_ok = i < p.L;
    const int jb_end = p.causal ? wb + 1 : NJB;
    const float lse_i = lse_s[i], d_i = d_s[i];
    f32x4 dq[NCB];
#pragma unroll
    for (int cb = 0; cb < NCB; ++cb) dq[cb] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int jb = 0; jb < NJB; ++jb) {
      if (jb >= jb_end) continue;
      const f32x4 sv = sa_dot<DH>(ks + (jb * 16 + j16) * LD, qs + i * LD, g);
      const f32x4 dp = sa_dot<DH>(vs + (jb * 16 + j16) * LD, gs + i * LD, g);
      f32x4 ds;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int j = jb * 16 + 4 * g + r;
        const bool ok = i_ok && ((kmask >> j) & 1) && (!p.causal || j <= i);
        float v = 0.f;
        if (ok) {
          const float pv = expf(sv[r] * p.scale - lse_i);
          float dpv = dp[r];
          if (p.drop) dpv = sa_kept(p, pr, i, j) ? dpv / p.q : 0.f;
          v = pv * (dpv - d_i);
        }
        ds[r] = v;
      }
      sa_acc<DH>(ks + jb * 16 * LD, ds, dq, j16, g);
    }
    if (i_ok) {
      float* dst = drow + (int64_t)i * ld3;
#pragma unroll
      for (int cb = 0; cb < NCB; ++cb)
        *reinterpret_cast<float4*>(dst + cb * 16) =
            make_float4(dq[cb][0] * p.scale, dq[cb][1] * p.scale, dq[cb][2] * p.scale, dq[cb][3] * p.scale);
    }
  }
  // ---- pass 2: the wave's 16 keys, queries in the registers: dk, dv
  {
    const int j = wb * 16 + j16;
    const bool j_ok = (kmask >> j) & 1;
    const int ib0 = p.causal ? wb : 0;
    f32x4 dk[NCB], dv[NCB];
#pragma unroll
    for (int cb = 0; cb < NCB; ++cb) dk[cb] = dv[cb] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ib = 0; ib < NJB; ++ib) {
      if (ib < ib0) continue;
      const f32x4 sv = sa_dot<DH>(qs + (ib * 16 + j16) * LD, ks + j * LD, g);
      const f32x4 dp = sa_dot<DH>(gs + (ib * 16 + j16) * LD, vs + j * LD, g);
      const float4 lse4 = *reinterpret_cast<const float4*>(lse_s + ib * 16 + 4 * g);
      const float4 d4 = *reinterpret_cast<const float4*>(d_s + ib * 16 + 4 * g);
      const float lse_r[4] = {lse4.x, lse4.y, lse4.z, lse4.w}, d_r[4] = {d4.x, d4.y, d4.z, d4.w};
      f32x4 ds, pt;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = ib * 16 + 4 * g + r;
        const bool ok = j_ok && i < p.L && (!p.causal || j <= i);
        float v = 0.f, w = 0.f;
        if (ok) {
          const float pv = expf(sv[r] * p.scale - lse_r[r]);
          float dpv = dp[r];
          w = pv;
          if (p.drop) {
            const bool kept = sa_kept(p, pr, i, j);
            dpv = kept ? dpv / p.q : 0.f;
            w = kept ? pv / p.q : 0.f;
          }
          v = pv * (dpv - d_r[r]);
        }
        ds[r] = v;
        pt[r] = w;
      }
      sa_acc<DH>(qs + ib * 16 * LD, ds, dk, j16, g);
      sa_acc<DH>(gs + ib * 16 * LD, pt, dv, j16, g);
    }
    if (j < p.L) {
      float* dst = drow + (int64_t)j * ld3 + p.D;
#pragma unroll
      for (int cb = 0; cb < NCB; ++cb) {
        *reinterpret_cast<float4*>(dst + cb * 16) =
            make_float4(dk[cb][0] * p.scale, dk[cb][1] * p.scale, dk[cb][2] * p.scale, dk[cb][3] * p.scale);
        *reinterpret_cast<float4*>(dst + p.D + cb * 16) = make_float4(dv[cb][0], dv[cb][1], dv[cb][2], dv[cb][3]);
      }
    }
  }
}

static inline int sa_tile(int L) { return L <= 16 ? 16 : (L <= 32 ? 32 : 64); }

// the checks both entry points share; fills the shared part of `p`
static int sa_check(const rsa_attention_args& a, const char* fn, SaParams& p) {
  RSA_CHECK_ARG(a.n_seq >= 0, "%s: negative n_seq %lld", fn, (long long)a.n_seq);
  RSA_CHECK_ARG(a.seq_len >= 1 && a.seq_len <= SA_MAX_L, "%s: seq_len must lie in [1, %d] (one tile holds the sequence), got %d", fn,
                SA_MAX_L, a.seq_len);
  RSA_CHECK_ARG(a.head_dim == 16 || a.head_dim == 32 || a.head_dim == 64, "%s: head_dim must be 16, 32 or 64, got %d", fn, a.head_dim);
  RSA_CHECK_ARG(a.n_head >= 1 && (int64_t)a.n_head * a.head_dim < (1ll << 29), "%s: bad n_head %d", fn, a.n_head);
  RSA_CHECK_ARG(std::isfinite(a.scale), "%s: scale must be finite", fn);
  RSA_CHECK_ARG(a.p >= 0.0 && a.p < 1.0, "%s: the dropout probability must lie in [0, 1), got %g", fn, a.p);
  RSA_CHECK_ARG(a.p == 0.0 || (a.grid_threads > 0 && a.grid_threads % 256 == 0 && (a.offset & 3) == 0),
                "%s: bad philox state for the dropout (grid_threads %u must be a positive multiple of 256, offset a multiple of 4)",
                fn, a.grid_threads);
  const int64_t n_prob = a.n_seq * a.n_head;
  RSA_CHECK_ARG(a.n_seq < (1ll << 40) && n_prob < (1ll << 31), "%s: too many (sequence, head) problems for one launch", fn);
  RSA_CHECK_ARG(a.p == 0.0 || n_prob * a.seq_len * a.seq_len < (1ll << 31),
                "%s: B H L L = %lld elements: torch.rand splits a call of 2^31 or more elements, the dropout mask would not be its", fn,
                (long long)(n_prob * a.seq_len * a.seq_len));
  if (a.n_seq == 0) return RSA_OK;
  RSA_CHECK_ARG(a.qkv && a.out && a.lse, "%s: qkv, out or lse is null", fn);
  RSA_CHECK_ARG((((uintptr_t)a.qkv | (uintptr_t)a.out) & 15) == 0, "%s: qkv and out must be 16-byte aligned", fn);
  p.qkv = a.qkv, p.key_pad = a.key_pad;
  p.n_prob = n_prob;
  p.L = a.seq_len, p.H = a.n_head, p.D = a.n_head * a.head_dim;
  p.causal = a.causal != 0;
  p.scale = a.scale;
  p.q = (float)(1.0 - a.p);
  p.drop = a.p != 0.0;
  p.pc = PhiloxCall{a.seed, a.offset >> 2, a.grid_threads, a.elem_base};
  p.out = a.out, p.lse = a.lse;
  return RSA_OK;
}

template <class F>
static inline bool sa_dispatch(int L, int dh, F&& f) {
  bool done = false;
  dispatch_int<16, 32, 64>(sa_tile(L), [&](auto LT) { done = dispatch_dim<16, 32, 64>(dh, [&](auto DH) { f(LT, DH); }); });
  return done;
}

}  // namespace rsa

using namespace rsa;

extern "C" int rsa_attention(const rsa_attention_args* args, rsa_stream_t stream) {
  const char* fn = "rsa_attention";
  rsa_attention_args a;
  if (int rc = load_args(a, args, fn)) return rc;
  SaParams p{};
  if (int rc = sa_check(a, fn, p)) return rc;
  if (a.n_seq == 0) return RSA_OK;
  p.keep = a.keep;
  int rc = RSA_OK;
  sa_dispatch(a.seq_len, a.head_dim, [&](auto LT, auto DH) {
    constexpr int ppw = 4 / (LT() / 16);
    const int64_t lds = (int64_t)ppw * 3 * LT() * (DH() + 4) * 4;
    rc = allow_lds<sa_forward_kernel<LT(), DH()>>(lds, fn);
    if (rc == RSA_OK)
      hipLaunchKernelGGL((sa_forward_kernel<LT(), DH()>), dim3((unsigned)((p.n_prob + ppw - 1) / ppw)), dim3(256), (size_t)lds,
                         (hipStream_t)stream, p);
  });
  if (rc) return rc;
  RSA_CHECK_LAUNCH(fn);
  return RSA_OK;
}

extern "C" int rsa_attention_backward(const rsa_attention_args* args, rsa_stream_t stream) {
  const char* fn = "rsa_attention_backward";
  rsa_attention_args a;
  if (int rc = load_args(a, args, fn)) return rc;
  SaParams p{};
  if (int rc = sa_check(a, fn, p)) return rc;
  if (a.n_seq == 0) return RSA_OK;
  RSA_CHECK_ARG(a.g_out && a.dqkv, "%s: g_out or dqkv is null", fn);
  RSA_CHECK_ARG((((uintptr_t)a.g_out | (uintptr_t)a.dqkv) & 15) == 0, "%s: g_out and dqkv must be 16-byte aligned", fn);
  p.g = a.g_out, p.dqkv = a.dqkv;
  int rc = RSA_OK;
  sa_dispatch(a.seq_len, a.head_dim, [&](auto LT, auto DH) {
    constexpr int ppw = 4 / (LT() / 16);
    const int64_t lds = (int64_t)ppw * (4 * LT() * (DH() + 4) + 2 * LT()) * 4;
    rc = allow_lds<sa_backward_kernel<LT(), DH()>>(lds, fn);
    if (rc == RSA_OK)
      hipLaunchKernelGGL((sa_backward_kernel<LT(), DH()>), dim3((unsigned)((p.n_prob + ppw - 1) / ppw)), dim3(256), (size_t)lds,
                         (hipStream_t)stream, p);
  });
  if (rc) return rc;
  RSA_CHECK_LAUNCH(fn);
  return RSA_OK;
}
