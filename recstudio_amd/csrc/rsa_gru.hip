// The GRU recurrence of the sequence towers (GRU4Rec, NARM), fused (gfx950): forward and backward.
//
// rsa_gru / rsa_gru_backward : the SEQUENTIAL part of torch.nn.GRU (one layer, one direction, batch_first) as the reference's
//                              module.GRULayer runs it (recstudio/model/seq/gru4rec.py); gate order r, z, n
//
//   gh_t = W_hh h_{t-1} (+ b_hh)     r = sigma(gi_r + gh_r)     z = sigma(gi_z + gh_z)     n = tanh(gi_n + r gh_n)
//   h_t  = (1 - z) n + z h_{t-1}
//
// gi = F.linear(x, W_ih, b_ih) [B, L, 3 H] is the caller's GEMM (parallel in time); this file walks the L dependent steps in ONE
// launch with W_hh resident on the chip.
//
// TILE.  A workgroup owns 16 batch rows and has H / 16 waves (H = 32, 64 or 128 is the template argument: 128, 256 or 512
// threads).  Wave w owns hidden units [16 w, 16 w + 16) of all three gates.  Its three 16-row blocks of W_hh are the A operand of
// v_mfma_f32_16x16x4_f32 (M = unit, K = H) and are loaded ONCE into registers: lane (j, g) (j = lane & 15, g = lane >> 4) keeps
// elements k0 + 4 g .. + 3 of row j of each block, 3 H / 4 registers (96 at H = 128; the 192 KB of W_hh do not fit the LDS).
// h_{t-1} of the tile is the B operand (N = batch row): 16 rows of H + 4 floats in LDS, double-buffered, read 16 bytes at a time
// -- step t of a 16-byte read multiplies elements k0 + 4 g + t of both operands, the same permutation on both sides (K ORDER of
// rsa_attention.hip); row stride = 4 mod 32 floats, so the 16 rows of a read start in 16 different 4-bank slots.
// The product leaves unit 16 w + 4 g + r of batch row j in element r of lane (j, g) for each gate: r, z and n of a unit meet in
// one lane.  The gate epilogue is in-lane, h_{t-1} of the lane's four units stays in its registers, h_t is one 16-byte store to
// `out` and one to the other LDS buffer, and ONE barrier closes the step.  The three gates are three independent accumulator
// chains, which covers the 40-cycle dependent latency of the instruction.  gi_{t+1} does not depend on h: its three 16-byte loads
// are issued before the products of step t.
//
// LENGTHS.  Row b stops at len_b (clamped into [0, L]; L without `lengths`): out[b, t >= len_b] = +0, and the workgroup runs to
// the longest row of its tile.  Rows past n_seq in the last tile have length 0 and touch no memory.
//
// BACKWARD.  From gi, gh = F.linear(h_prev, W_hh, b_hh) (the caller's GEMM over all positions: every h_{t-1} is in `out`), out,
// h0 and g_out, walking t = len - 1 .. 0 with dh_t = g_out_t + carry:
//   dn = dh (1 - z)(1 - n^2)     dz = dh (h_{t-1} - n) z (1 - z)     dr = dn gh_n r (1 - r)
//   dgi = [dr, dz, dn]           dgh = [dr, dz, dn r]                carry = dh z + W_hh^T dgh
// The owning lane recomputes r, z, n, does the gate backward and writes dgh of the tile to LDS (16 rows of 3 H + 4 floats,
// double-buffered; ONE barrier per step).  Wave w then forms its 16 units of W_hh^T dgh: columns [16 w, 16 w + 16) of W_hh,
// transposed, are its A operand, again 3 H / 4 registers per lane loaded once; the sum runs over 3 H inside the wave in three
// accumulator chains (k = 0, 1, 2 mod 3 blocks of 16) added (a0 + a1) + a2.  No atomics, no workspace; two runs are bit-equal.
// Every element of dgi, dgh_n and dh0 is written, +0 at t >= len.  Everything the step loads is independent of the carry, so the
// loads of step t - 1 are issued before the work of step t.
//
// flops: forward 2 * 3 H * H per (b, t), backward the same in the kernel (the other half of the backward is the caller's GEMMs).
// Bytes per (b, t): forward 12 H read + 4 H written; backward 32 H read + 16 H written.
#include "rsa_common.hpp"
#include "rsa_launch.hpp"

namespace rsa {

using f32x4 = float __attribute__((ext_vector_type(4)));

struct GruParams {
  const float* gi;
  const float* gh;
  const float* w_hh;
  const float* b_hh;
  const float* h0;
  const int64_t* lengths;
  int64_t B;
  int L;
  float* out;                      // forward: written; backward: read
  const float* g_out;
  float* dgi;
  float* dgh_n;
  float* dh0;
};

__device__ __forceinline__ float gru_sigmoid(float x) { return 1.f / (1.f + expf(-x)); }

__device__ __forceinline__ float4 gru_ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ void gru_st4(float* p, const float4& v) { *reinterpret_cast<float4*>(p) = v; }

// the row's length and the longest of the tile (the same value in every lane of every wave of the workgroup)
__device__ __forceinline__ int gru_lengths(const GruParams& p, int64_t b, int& tmax) {
  int len = 0;
  if (b < p.B) {
    len = p.L;
    if (p.lengths) {
      const int64_t v = p.lengths[b];
      len = v < 0 ? 0 : (v > p.L ? p.L : (int)v);
    }
  }
  int m = len;
#pragma unroll
  for (int s = 1; s < 16; s <<= 1) m = max(m, __shfl_xor(m, s, 64));
  tmax = m;
  return len;
}

template <int H>
__global__ __launch_bounds__(H * 4) void gru_forward_kernel(const GruParams p) {
  constexpr int NKB = H / 16, LD = H + 4;
  __shared__ __attribute__((aligned(16))) float hs[2][16 * LD];
  const int lane = lane_id(), wave = threadIdx.x >> 6, j = lane & 15, g = lane >> 4;
  const int u0 = wave * 16 + 4 * g;                       // the lane's four units
  const int64_t b = (int64_t)blockIdx.x * 16 + j;
  int tmax;
  const int len = gru_lengths(p, b, tmax);
  float4 wr[3][NKB];
#pragma unroll
  for (int q = 0; q < 3; ++q)
#pragma unroll
    for (int kb = 0; kb < NKB; ++kb) wr[q][kb] = gru_ld4(p.w_hh + (int64_t)(q * H + wave * 16 + j) * H + kb * 16 + 4 * g);
  const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
  float4 bias[3] = {zero4, zero4, zero4};
  if (p.b_hh) {
#pragma unroll
    for (int q = 0; q < 3; ++q) bias[q] = gru_ld4(p.b_hh + q * H + u0);
  }
  float4 h4 = zero4;
  if (b < p.B && p.h0) h4 = gru_ld4(p.h0 + b * H + u0);
  float h[4] = {h4.x, h4.y, h4.z, h4.w};
  gru_st4(&hs[0][j * LD + u0], h4);
  __syncthreads();
  // never dereferenced for a row past n_seq (len = 0)
  const float* gi_row = p.gi + (b < p.B ? b : 0) * p.L * (int64_t)(3 * H) + u0;
  float* out_row = p.out + (b < p.B ? b : 0) * p.L * (int64_t)H + u0;
  float4 gc[3] = {zero4, zero4, zero4};
  if (0 < len) {
#pragma unroll
    for (int q = 0; q < 3; ++q) gc[q] = gru_ld4(gi_row + q * H);
  }
  int cur = 0;
  for (int t = 0; t < tmax; ++t) {
    float4 gn[3] = {zero4, zero4, zero4};
    if (t + 1 < len) {
#pragma unroll
      for (int q = 0; q < 3; ++q) gn[q] = gru_ld4(gi_row + (int64_t)(t + 1) * (3 * H) + q * H);
    }
    const float* hb = &hs[cur][j * LD];
    f32x4 ar = {0.f, 0.f, 0.f, 0.f}, az = ar, an = ar;
#pragma unroll
    for (int kb = 0; kb < NKB; ++kb) {
      const float4 hv = gru_ld4(hb + kb * 16 + 4 * g);
      ar = __builtin_amdgcn_mfma_f32_16x16x4f32(wr[0][kb].x, hv.x, ar, 0, 0, 0);
      az = __builtin_amdgcn_mfma_f32_16x16x4f32(wr[1][kb].x, hv.x, az, 0, 0, 0);
      an = __builtin_amdgcn_mfma_f32_16x16x4f32(wr[2][kb].x, hv.x, an, 0, 0, 0);
      ar = __builtin_amdgcn_mfma_f32_16x16x4f32(wr[0][kb].y, hv.y, ar, 0, 0, 0);
      az = __builtin_amdgcn_mfma_f32_16x16x4f32(wr[1][kb].y, hv.y, az, 0, 0, 0);
      an = __builtin_amdgcn_mfma_f32_16x16x4f32(wr[2][kb].y, hv.y, an, 0, 0, 0);
      ar = __builtin_amdgcn_mfma_f32_16x16x4f32(wr[0][kb].z, hv.z, ar, 0, 0, 0);
      az = __builtin_amdgcn_mfma_f32_16x16x4f32(wr[1][kb].z, hv.z, az, 0, 0, 0);
      an = __builtin_amdgcn_mfma_f32_16x16x4f32(wr[2][kb].z, hv.z, an, 0, 0, 0);
      ar = __builtin_amdgcn_mfma_f32_16x16x4f32(wr[0][kb].w, hv.w, ar, 0, 0, 0);
      az = __builtin_amdgcn_mfma_f32_16x16x4f32(wr[1][kb].w, hv.w, az, 0, 0, 0);
      an = __builtin_amdgcn_mfma_f32_16x16x4f32(wr[2][kb].w, hv.w, an, 0, 0, 0);
    }
    if (t < len) {
      const float gir[4] = {gc[0].x, gc[0].y, gc[0].z, gc[0].w}, giz[4] = {gc[1].x, gc[1].y, gc[1].z, gc[1].w};
      const float gin[4] = {gc[2].x, gc[2].y, gc[2].z, gc[2].w};
      const float br[4] = {bias[0].x, bias[0].y, bias[0].z, bias[0].w}, bz[4] = {bias[1].x, bias[1].y, bias[1].z, bias[1].w};
      const float bn[4] = {bias[2].x, bias[2].y, bias[2].z, bias[2].w};
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float r = gru_sigmoid(gir[e] + (ar[e] + br[e]));
        const float z = gru_sigmoid(giz[e] + (az[e] + bz[e]));
        const float n = tanhf(gin[e] + r * (an[e] + bn[e]));
        h[e] = (1.f - z) * n + z * h[e];
      }
      gru_st4(out_row + (int64_t)t * H, make_float4(h[0], h[1], h[2], h[3]));
    } else if (b < p.B) {
      gru_st4(out_row + (int64_t)t * H, zero4);
    }
    gru_st4(&hs[cur ^ 1][j * LD + u0], make_float4(h[0], h[1], h[2], h[3]));
    __syncthreads();
    cur ^= 1;
#pragma unroll
    for (int q = 0; q < 3; ++q) gc[q] = gn[q];
  }
  if (b < p.B)
    for (int t = tmax; t < p.L; ++t) gru_st4(out_row + (int64_t)t * H, zero4);
}

// what a backward step reads for the lane's four units
struct GruStepIn {
  float4 gi[3], gh[3], go, hp;
};

template <int H>
__device__ __forceinline__ void gru_load_step(const GruParams& p, int64_t b, int u0, int t, GruStepIn& s) {
  const int64_t bt = b * p.L + t;
  const float* gi = p.gi + bt * (3 * H) + u0;
  const float* gh = p.gh + bt * (3 * H) + u0;
#pragma unroll
  for (int q = 0; q < 3; ++q) s.gi[q] = gru_ld4(gi + q * H), s.gh[q] = gru_ld4(gh + q * H);
  s.go = gru_ld4(p.g_out + bt * H + u0);
  if (t > 0) s.hp = gru_ld4(p.out + (bt - 1) * H + u0);
  else s.hp = p.h0 ? gru_ld4(p.h0 + b * H + u0) : make_float4(0.f, 0.f, 0.f, 0.f);
}

template <int H>
__global__ __launch_bounds__(H * 4) void gru_backward_kernel(const GruParams p) {
  constexpr int NKB = 3 * H / 16, LD = 3 * H + 4;
  static_assert(NKB % 3 == 0, "three accumulator chains");
  __shared__ __attribute__((aligned(16))) float ds[2][16 * LD];
  const int lane = lane_id(), wave = threadIdx.x >> 6, j = lane & 15, g = lane >> 4;
  const int u0 = wave * 16 + 4 * g;
  const int64_t b = (int64_t)blockIdx.x * 16 + j;
  int tmax;
  const int len = gru_lengths(p, b, tmax);
  // W_hh^T: rows = the wave's units (column 16 w + j of W_hh), K = the 3 H rows of W_hh
  float4 wt[NKB];
#pragma unroll
  for (int kb = 0; kb < NKB; ++kb) {
    const float* w = p.w_hh + (int64_t)(kb * 16 + 4 * g) * H + wave * 16 + j;
    wt[kb] = make_float4(w[0], w[H], w[2 * H], w[3 * H]);
  }
  const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
  const int64_t brow = b < p.B ? b : 0;                 // never dereferenced for a row past n_seq (len = 0)
  float carry[4] = {0.f, 0.f, 0.f, 0.f};
  GruStepIn c;
  c.go = c.hp = zero4;
#pragma unroll
  for (int q = 0; q < 3; ++q) c.gi[q] = c.gh[q] = zero4;
  if (tmax - 1 >= 0 && tmax - 1 < len) gru_load_step<H>(p, brow, u0, tmax - 1, c);
  int cur = 0;
  for (int t = tmax - 1; t >= 0; --t) {
    GruStepIn nx = c;
    if (t - 1 >= 0 && t - 1 < len) gru_load_step<H>(p, brow, u0, t - 1, nx);
    float dr[4] = {0.f, 0.f, 0.f, 0.f}, dz[4] = {0.f, 0.f, 0.f, 0.f}, dn[4] = {0.f, 0.f, 0.f, 0.f}, dnr[4] = {0.f, 0.f, 0.f, 0.f};
    float keep[4] = {0.f, 0.f, 0.f, 0.f};
    const bool on = t < len;
    if (on) {
      const float gir[4] = {c.gi[0].x, c.gi[0].y, c.gi[0].z, c.gi[0].w}, giz[4] = {c.gi[1].x, c.gi[1].y, c.gi[1].z, c.gi[1].w};
      const float gin[4] = {c.gi[2].x, c.gi[2].y, c.gi[2].z, c.gi[2].w};
      const float ghr[4] = {c.gh[0].x, c.gh[0].y, c.gh[0].z, c.gh[0].w}, ghz[4] = {c.gh[1].x, c.gh[1].y, c.gh[1].z, c.gh[1].w};
      const float ghn[4] = {c.gh[2].x, c.gh[2].y, c.gh[2].z, c.gh[2].w};
      const float go[4] = {c.go.x, c.go.y, c.go.z, c.go.w}, hp[4] = {c.hp.x, c.hp.y, c.hp.z, c.hp.w};
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float r = gru_sigmoid(gir[e] + ghr[e]);
        const float z = gru_sigmoid(giz[e] + ghz[e]);
        const float n = tanhf(gin[e] + r * ghn[e]);
        const float dh = go[e] + carry[e];
        dn[e] = (dh * (1.f - z)) * (1.f - n * n);
        dz[e] = (dh * (hp[e] - n)) * (z * (1.f - z));
        dr[e] = (dn[e] * ghn[e]) * (r * (1.f - r));
        dnr[e] = dn[e] * r;
        keep[e] = dh * z;
      }
    }
    if (b < p.B) {
      const int64_t bt = b * p.L + t;
      float* dgi = p.dgi + bt * (3 * H) + u0;
      gru_st4(dgi, make_float4(dr[0], dr[1], dr[2], dr[3]));
      gru_st4(dgi + H, make_float4(dz[0], dz[1], dz[2], dz[3]));
      gru_st4(dgi + 2 * H, make_float4(dn[0], dn[1], dn[2], dn[3]));
      gru_st4(p.dgh_n + bt * H + u0, make_float4(dnr[0], dnr[1], dnr[2], dnr[3]));
    }
    float* drow = &ds[cur][j * LD + u0];
    gru_st4(drow, make_float4(dr[0], dr[1], dr[2], dr[3]));
    gru_st4(drow + H, make_float4(dz[0], dz[1], dz[2], dz[3]));
    gru_st4(drow + 2 * H, make_float4(dnr[0], dnr[1], dnr[2], dnr[3]));
    __syncthreads();
    const float* db = &ds[cur][j * LD];
    f32x4 a0 = {0.f, 0.f, 0.f, 0.f}, a1 = a0, a2 = a0;
#pragma unroll
    for (int kb = 0; kb < NKB; kb += 3) {
      const float4 d0 = gru_ld4(db + kb * 16 + 4 * g), d1 = gru_ld4(db + (kb + 1) * 16 + 4 * g), d2 = gru_ld4(db + (kb + 2) * 16 + 4 * g);
      a0 = __builtin_amdgcn_mfma_f32_16x16x4f32(wt[kb].x, d0.x, a0, 0, 0, 0);
      a1 = __builtin_amdgcn_mfma_f32_16x16x4f32(wt[kb + 1].x, d1.x, a1, 0, 0, 0);
      a2 = __builtin_amdgcn_mfma_f32_16x16x4f32(wt[kb + 2].x, d2.x, a2, 0, 0, 0);
      a0 = __builtin_amdgcn_mfma_f32_16x16x4f32(wt[kb].y, d0.y, a0, 0, 0, 0);
      a1 = __builtin_amdgcn_mfma_f32_16x16x4f32(wt[kb + 1].y, d1.y, a1, 0, 0, 0);
      a2 = __builtin_amdgcn_mfma_f32_16x16x4f32(wt[kb + 2].y, d2.y, a2, 0, 0, 0);
      a0 = __builtin_amdgcn_mfma_f32_16x16x4f32(wt[kb].z, d0.z, a0, 0, 0, 0);
      a1 = __builtin_amdgcn_mfma_f32_16x16x4f32(wt[kb + 1].z, d1.z, a1, 0, 0, 0);
      a2 = __builtin_amdgcn_mfma_f32_16x16x4f32(wt[kb + 2].z, d2.z, a2, 0, 0, 0);
      a0 = __builtin_amdgcn_mfma_f32_16x16x4f32(wt[kb].w, d0.w, a0, 0, 0, 0);
      a1 = __builtin_amdgcn_mfma_f32_16x16x4f32(wt[kb + 1].w, d1.w, a1, 0, 0, 0);
      a2 = __builtin_amdgcn_mfma_f32_16x16x4f32(wt[kb + 2].w, d2.w, a2, 0, 0, 0);
    }
    if (on) {
#pragma unroll
      for (int e = 0; e < 4; ++e) carry[e] = keep[e] + ((a0[e] + a1[e]) + a2[e]);
    }
    cur ^= 1;
    c = nx;
  }
  if (b < p.B) {
    gru_st4(p.dh0 + b * H + u0, make_float4(carry[0], carry[1], carry[2], carry[3]));
    for (int t = tmax; t < p.L; ++t) {
      const int64_t bt = b * p.L + t;
      float* dgi = p.dgi + bt * (3 * H) + u0;
      gru_st4(dgi, zero4);
      gru_st4(dgi + H, zero4);
      gru_st4(dgi + 2 * H, zero4);
      gru_st4(p.dgh_n + bt * H + u0, zero4);
    }
  }
}

// the checks both entry points share; fills the shared part of `p`
static int gru_check(const rsa_gru_args& a, const char* fn, GruParams& p) {
  RSA_CHECK_ARG(a.n_seq >= 0, "%s: negative n_seq %lld", fn, (long long)a.n_seq);
  RSA_CHECK_ARG(a.seq_len >= 0, "%s: negative seq_len %d", fn, a.seq_len);
  if (a.lengths_host) {      // the caller's host copy of `lengths`: checked here, where the device copy cannot be read
    for (int64_t i = 0; i < a.n_seq; ++i)
      RSA_CHECK_ARG(a.lengths_host[i] >= 0 && a.lengths_host[i] <= a.seq_len, "%s: lengths[%lld] = %lld must lie in [0, seq_len = %d]", fn,
                    (long long)i, (long long)a.lengths_host[i], a.seq_len);
  }
  RSA_CHECK_ARG(a.hidden == 32 || a.hidden == 64 || a.hidden == 128, "%s: hidden must be 32, 64 or 128, got %d", fn, a.hidden);
  RSA_CHECK_ARG(a.n_seq < (1ll << 34), "%s: too many sequences for one launch", fn);
  RSA_CHECK_ARG(a.w_hh, "%s: w_hh is null", fn);
  RSA_CHECK_ARG(((uintptr_t)a.w_hh & 15) == 0 && ((uintptr_t)a.b_hh & 15) == 0 && ((uintptr_t)a.h0 & 15) == 0,
                "%s: w_hh, b_hh and h0 must be 16-byte aligned", fn);
  if (a.n_seq == 0 || a.seq_len == 0) return RSA_OK;
  RSA_CHECK_ARG(a.gi && a.out, "%s: gi or out is null", fn);
  RSA_CHECK_ARG((((uintptr_t)a.gi | (uintptr_t)a.out) & 15) == 0, "%s: gi and out must be 16-byte aligned", fn);
  p.gi = a.gi, p.w_hh = a.w_hh, p.b_hh = a.b_hh, p.h0 = a.h0, p.lengths = a.lengths;
  p.B = a.n_seq, p.L = a.seq_len;
  p.out = a.out;
  return RSA_OK;
}

}  // namespace rsa

using namespace rsa;

extern "C" int rsa_gru(const rsa_gru_args* args, rsa_stream_t stream) {
  const char* fn = "rsa_gru";
  rsa_gru_args a;
  if (int rc = load_args(a, args, fn)) return rc;
  GruParams p{};
  if (int rc = gru_check(a, fn, p)) return rc;
  if (a.n_seq == 0 || a.seq_len == 0) return RSA_OK;
  dispatch_dim<32, 64, 128>(a.hidden, [&](auto H) {
    hipLaunchKernelGGL((gru_forward_kernel<H()>), dim3((unsigned)((p.B + 15) / 16)), dim3(H() * 4), 0, (hipStream_t)stream, p);
  });
  RSA_CHECK_LAUNCH(fn);
  return RSA_OK;
}

extern "C" int rsa_gru_backward(const rsa_gru_args* args, rsa_stream_t stream) {
  const char* fn = "rsa_gru_backward";
  rsa_gru_args a;
  if (int rc = load_args(a, args, fn)) return rc;
  GruParams p{};
  if (int rc = gru_check(a, fn, p)) return rc;
  RSA_CHECK_ARG(a.n_seq == 0 || a.dh0, "%s: dh0 is null", fn);
  RSA_CHECK_ARG(((uintptr_t)a.dh0 & 15) == 0, "%s: dh0 must be 16-byte aligned", fn);
  if (a.n_seq == 0) return RSA_OK;
  if (a.seq_len == 0) {      // nothing flows: dh0 = 0
    RSA_CHECK_HIP(hipMemsetAsync(a.dh0, 0, (size_t)a.n_seq * a.hidden * sizeof(float), (hipStream_t)stream), fn);
    return RSA_OK;
  }
  RSA_CHECK_ARG(a.gh && a.g_out && a.dgi && a.dgh_n, "%s: gh, g_out, dgi or dgh_n is null", fn);
  RSA_CHECK_ARG((((uintptr_t)a.gh | (uintptr_t)a.g_out | (uintptr_t)a.dgi | (uintptr_t)a.dgh_n) & 15) == 0,
                "%s: gh, g_out, dgi and dgh_n must be 16-byte aligned", fn);
  p.gh = a.gh, p.g_out = a.g_out, p.dgi = a.dgi, p.dgh_n = a.dgh_n, p.dh0 = a.dh0;
  dispatch_dim<32, 64, 128>(a.hidden, [&](auto H) {
    hipLaunchKernelGGL((gru_backward_kernel<H()>), dim3((unsigned)((p.B + 15) / 16)), dim3(H() * 4), 0, (hipStream_t)stream, p);
  });
  RSA_CHECK_LAUNCH(fn);
  return RSA_OK;
}
