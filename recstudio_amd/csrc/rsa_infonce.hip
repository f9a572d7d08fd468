// In-batch InfoNCE of the contrastive sequence retrievers (gfx950) without anything of size B^2.
//
// rsa_batch_infonce / rsa_batch_infonce_backward : InfoNCELoss('batch_both' / 'batch_single')
//                                                  recstudio/model/module/data_augmentation.py:324-376
//
//   the logit set of row b:  s_ij[b, k] = <zi_b, zj_k> inv_t  for every k but those with k != b and labels[k] == labels[b];
//               with `both`: s_ii[b, k] = <zi_b, zi_k> inv_t  for every k != b whose label differs (no labels: every k != b)
//   forward :  lse_b = log sum exp over the set,  pos_b = s_ij[b, b]                        (the loss is mean(lse - pos), the caller's)
//   backward:  with P = exp(s - lse_b) recomputed from lse, g the upstream of lse - pos:
//     dzi_b = inv_t [ g_b (sum_k P_ij[b, k] zj_k + sum_k P_ii[b, k] zi_k - zj_b) + sum_r g_r P_ii[r, b] zi_r ]
//     dzj_k = inv_t [ sum_b g_b P_ij[b, k] zi_b - g_k zi_k ]
//
// ONE FRAME FOR ALL THREE PASSES.  A wave owns 32 STATIONARY rows (lane (j, hh) = lane & 31, lane >> 5: row s0 + j, kept in
// registers as the B operand of the fp32 32x32x2 MFMA) and streams the other matrix 32 rows at a time as the A operand:
// T[x, s] = <X_x, S_s>, register r of lane (j, hh) = streamed row x0 + row32(r, hh) against stationary row s0 + j.  Both exclusion
// rules are symmetric in (b, k), so the same compare on the two row indices (and two labels) serves whichever side is stationary.
//   forward            stationary zi_b; streams zj (ij) and, with `both`, zi (ii): every lane carries a running maximum and sum
//                      over ITS 16 entries of a tile, the two halves of a column meet once at the end.
//   backward, dzi      stationary zi_b; streams zj with w = g_b exp(t - lse_b), and zi with w = g_b exp(t - lse_b) + g_x exp(t - lse_x)
//                      (row role + key role of b in the ii block);
//   backward, dzj      stationary zj_k; streams zi with w = g_x exp(t - lse_x).
//   The weighted sum out^T[c, s] += sum_x X[x, c] w[x, s] is a second MFMA chain whose B operand at step r IS register r of the
//   weight tile (contraction index hh <-> streamed row row32(r, hh)); its accumulators stay in registers for the whole stream.
// A stationary row is summed by its own wave in a fixed order: no atomics, no workspace, two runs are bit-equal.  Rows past B are
// never read (the row index is clamped and the entry carries weight 0).
#include "rsa_internal.hpp"

namespace rsa {

typedef float inf_f32x16 __attribute__((ext_vector_type(16)));

struct InfoNceParams {
  const float *zi, *zj, *lse_in, *g;
  const int64_t* labels;
  int64_t B;
  float inv_t;
  bool both;
  float *lse, *pos, *dzi, *dzj;
};

__device__ __forceinline__ int inf_row32(int r, int hh) { return (r & 3) + 8 * (r >> 2) + 4 * hh; }

__device__ __forceinline__ float4 inf_ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }

// the stationary rows as MFMA operands: sreg[t] = columns 4 hh + 8 t .. + 3 of row s0 + j (zeros past B)
template <int D>
__device__ __forceinline__ void inf_stationary(const float* S, int64_t B, int64_t s0, int lane, float4 (&sreg)[D / 8]) {
  const int j = lane & 31, hh = lane >> 5;
  const int64_t row = s0 + j;
#pragma unroll
  for (int t = 0; t < D / 8; ++t)
    sreg[t] = row < B ? inf_ld4(S + row * D + 4 * hh + 8 * t) : make_float4(0.f, 0.f, 0.f, 0.f);
}

// T[r] of lane (j, hh) = <X_{x0 + row32(r, hh)}, S_{s0 + j}>
template <int D>
__device__ __forceinline__ inf_f32x16 inf_scores(const float* X, int64_t B, int64_t x0, const float4 (&sreg)[D / 8], int lane) {
  const int j = lane & 31, hh = lane >> 5;
  const int64_t row = x0 + j;
  inf_f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
  for (int t = 0; t < D / 8; ++t) {
    const float4 a = row < B ? inf_ld4(X + row * D + 4 * hh + 8 * t) : make_float4(0.f, 0.f, 0.f, 0.f);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, sreg[t].x, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, sreg[t].y, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, sreg[t].z, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, sreg[t].w, acc, 0, 0, 0);
  }
  return acc;
}

// whether (stationary row s, streamed row x) is in the logit set of the ij block (II = false) or of the ii block (II = true)
template <bool II>
__device__ __forceinline__ bool inf_in_set(int64_t s, int64_t x, int64_t B, const int64_t* labels, int64_t label_s) {
  if (s >= B || x >= B) return false;
  if (s == x) return !II;
  if (labels == nullptr) return true;
  return labels[x] != label_s;
}

// ---------------------------------------------------------------------------------------------------------------- forward
template <int D>
__global__ __launch_bounds__(64) void infonce_forward_kernel(const InfoNceParams p) {
  const int lane = lane_id(), j = lane & 31, hh = lane >> 5;
  const int64_t s0 = (int64_t)blockIdx.x * 32, s = s0 + j;
  float4 sreg[D / 8];
  inf_stationary<D>(p.zi, p.B, s0, lane, sreg);
  const int64_t label_s = (p.labels && s < p.B) ? p.labels[s] : 0;
  float m = -INFINITY, l = 0.f, pos = 0.f;
  for (int blk = 0; blk < (p.both ? 2 : 1); ++blk) {                          // wave-uniform
    const float* X = blk ? p.zi : p.zj;
    for (int64_t x0 = 0; x0 < p.B; x0 += 32) {
      const inf_f32x16 T = inf_scores<D>(X, p.B, x0, sreg, lane);
      float t[16];
      bool ok[16];
      float tmax = -INFINITY;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int64_t x = x0 + inf_row32(r, hh);
        ok[r] = blk ? inf_in_set<true>(s, x, p.B, p.labels, label_s) : inf_in_set<false>(s, x, p.B, p.labels, label_s);
        t[r] = T[r] * p.inv_t;
        if (ok[r]) tmax = fmaxf(tmax, t[r]);
        if (!blk && x == s && s < p.B) pos = t[r];
      }
      if (tmax > -INFINITY) {
        const float mn = fmaxf(m, tmax);
        float add = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r)
          if (ok[r]) add += expf(t[r] - mn);
        l = (m > -INFINITY ? l * expf(m - mn) : 0.f) + add;
        m = mn;
      }
    }
  }
  // the two halves of a column
  const float m2 = __shfl_xor(m, 32, 64), l2 = __shfl_xor(l, 32, 64), pos2 = __shfl_xor(pos, 32, 64);
  const float mm = fmaxf(m, m2);
  const float a = m > -INFINITY ? l * expf(m - mm) : 0.f, b = m2 > -INFINITY ? l2 * expf(m2 - mm) : 0.f;
  // (the same two terms in the same order in both halves: the lower half's first)
  const float sum = hh == 0 ? a + b : b + a;
  if (hh == 0 && s < p.B) {
    p.lse[s] = mm + logf(sum);
    p.pos[s] = pos + pos2;                                                    // one of the two is the positive, the other 0
  }
}

// ---------------------------------------------------------------------------------------------------------------- backward
// one streamed matrix into the accumulators.  ROW: w += g_s exp(t - lse_s); KEY: w += g_x exp(t - lse_x).
template <int D, bool II, bool ROW, bool KEY>
__device__ __forceinline__ void inf_stream(const InfoNceParams& p, const float* X, int64_t s0, const float4 (&sreg)[D / 8], int lane,
                                           int64_t label_s, float lse_s, float g_s, inf_f32x16 (&acc)[D / 32]) {
  const int j = lane & 31, hh = lane >> 5;
  const int64_t s = s0 + j;
  for (int64_t x0 = 0; x0 < p.B; x0 += 32) {
    const inf_f32x16 T = inf_scores<D>(X, p.B, x0, sreg, lane);
    float w[16];
    int64_t xr[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int64_t x = x0 + inf_row32(r, hh);
      xr[r] = x < p.B ? x : p.B - 1;                                          // never read past B; such an entry has w = 0
      float v = 0.f;
      if (inf_in_set<II>(s, x, p.B, p.labels, label_s)) {
        const float t = T[r] * p.inv_t;
        if (ROW) v += g_s * expf(t - lse_s);
        if (KEY) v += p.g[x] * expf(t - p.lse_in[x]);
      }
      w[r] = v;
    }
#pragma unroll
    for (int cb = 0; cb < D / 32; ++cb) {
#pragma unroll
      for (int r = 0; r < 16; ++r)
        acc[cb] = __builtin_amdgcn_mfma_f32_32x32x2f32(X[xr[r] * D + cb * 32 + j], w[r], acc[cb], 0, 0, 0);
    }
  }
}

// DZJ = false: dzi of the stationary zi rows; DZJ = true: dzj of the stationary zj rows
template <int D, bool DZJ>
__global__ __launch_bounds__(64) void infonce_backward_kernel(const InfoNceParams p) {
  const int lane = lane_id(), j = lane & 31, hh = lane >> 5;
  const int64_t s0 = (int64_t)blockIdx.x * 32, s = s0 + j;
  float4 sreg[D / 8];
  inf_stationary<D>(DZJ ? p.zj : p.zi, p.B, s0, lane, sreg);
  const bool have = s < p.B;
  const int64_t label_s = (p.labels && have) ? p.labels[s] : 0;
  const float lse_s = have ? p.lse_in[s] : 0.f, g_s = have ? p.g[s] : 0.f;
  inf_f32x16 acc[D / 32];
#pragma unroll
  for (int cb = 0; cb < D / 32; ++cb)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[cb][r] = 0.f;
  if (DZJ) {
    inf_stream<D, false, false, true>(p, p.zi, s0, sreg, lane, label_s, lse_s, g_s, acc);
  } else {
    inf_stream<D, false, true, false>(p, p.zj, s0, sreg, lane, label_s, lse_s, g_s, acc);
    if (p.both) inf_stream<D, true, true, true>(p, p.zi, s0, sreg, lane, label_s, lse_s, g_s, acc);
  }
  if (!have) return;
  const float* other = DZJ ? p.zi : p.zj;                                     // the positive's partner row
  float* out = DZJ ? p.dzj : p.dzi;
#pragma unroll
  for (int cb = 0; cb < D / 32; ++cb)
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const int c = cb * 32 + inf_row32(q, hh);
      out[s * D + c] = p.inv_t * (acc[cb][q] - g_s * other[s * D + c]);
    }
}

template <int D>
static int infonce_launch(const InfoNceParams& p, bool backward, hipStream_t st, const char* fn) {
  const unsigned blocks = (unsigned)((p.B + 31) / 32);
  if (!backward) {
    hipLaunchKernelGGL(infonce_forward_kernel<D>, dim3(blocks), dim3(64), 0, st, p);
    RSA_CHECK_LAUNCH(fn);
    return RSA_OK;
  }
  hipLaunchKernelGGL((infonce_backward_kernel<D, false>), dim3(blocks), dim3(64), 0, st, p);
  RSA_CHECK_LAUNCH(fn);
  hipLaunchKernelGGL((infonce_backward_kernel<D, true>), dim3(blocks), dim3(64), 0, st, p);
  RSA_CHECK_LAUNCH(fn);
  return RSA_OK;
}

static int infonce_entry(const rsa_batch_infonce_args* args, rsa_stream_t stream, bool backward, const char* fn) {
  rsa_batch_infonce_args a;
  if (int rc = load_args(a, args, fn)) return rc;
  RSA_CHECK_ARG(a.d == 32 || a.d == 64 || a.d == 128, "%s: d must be 32, 64 or 128, got %d", fn, (int)a.d);
  RSA_CHECK_ARG(a.n_rows >= 0 && a.n_rows < (1ll << 31) * 32, "%s: n_rows out of range (%lld)", fn, (long long)a.n_rows);
  RSA_CHECK_ARG(a.inv_t > 0.f && a.inv_t < INFINITY, "%s: inv_t must be positive and finite, got %g", fn, (double)a.inv_t);
  if (a.n_rows == 0) return RSA_OK;
  RSA_CHECK_ARG(a.zi != nullptr && a.zj != nullptr, "%s: zi/zj is null", fn);
  RSA_CHECK_ARG(((uintptr_t)a.zi | (uintptr_t)a.zj) % 16 == 0, "%s: zi/zj must be 16-byte aligned", fn);
  RSA_CHECK_ARG(a.lse != nullptr, "%s: lse is null", fn);
  if (backward) {
    RSA_CHECK_ARG(a.g != nullptr && a.dzi != nullptr && a.dzj != nullptr, "%s: g/dzi/dzj is null", fn);
    RSA_CHECK_ARG((const void*)a.dzi != (const void*)a.zi && (const void*)a.dzi != (const void*)a.zj && (const void*)a.dzj != (const void*)a.zi &&
                  (const void*)a.dzj != (const void*)a.zj && a.dzi != a.dzj, "%s: dzi/dzj must not alias the inputs or each other", fn);
  } else {
    RSA_CHECK_ARG(a.pos != nullptr, "%s: pos is null", fn);
  }
  InfoNceParams p{};
  p.zi = a.zi, p.zj = a.zj, p.labels = a.labels, p.B = a.n_rows, p.inv_t = a.inv_t, p.both = a.both != 0;
  p.lse = a.lse, p.pos = a.pos, p.lse_in = a.lse, p.g = a.g, p.dzi = a.dzi, p.dzj = a.dzj;
  hipStream_t st = (hipStream_t)stream;
  if (a.d == 32) return infonce_launch<32>(p, backward, st, fn);
  if (a.d == 64) return infonce_launch<64>(p, backward, st, fn);
  return infonce_launch<128>(p, backward, st, fn);
}

}  // namespace rsa

extern "C" int rsa_batch_infonce(const rsa_batch_infonce_args* args, rsa_stream_t stream) {
  return rsa::infonce_entry(args, stream, false, "rsa_batch_infonce");
}

extern "C" int rsa_batch_infonce_backward(const rsa_batch_infonce_args* args, rsa_stream_t stream) {
  return rsa::infonce_entry(args, stream, true, "rsa_batch_infonce_backward");
}
