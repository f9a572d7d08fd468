// SLIM (recstudio/model/mf/slim.py) on gfx950, all float64: the N elastic-net problems of the fit, one per target item j, solved by
// cyclic coordinate descent on the shared Gram matrix G = R^T R (rsa_slim_fit).  include/recstudio_amd.h states the contract,
// DESIGN.md 4.24 the design and the proof that the candidates C_j = {k != j, k >= 1 : G[k, j] > l1} carry the whole problem.
//
// STATE.  A problem keeps, per candidate, its id, the gradient g_k = q_k - (Q w)_k, the weight w_k and the diagonal Q_kk; H of the
// reference's solver is q - g and is formed only for the duality gap.  A coordinate's rule reads g_k, w_k and Q_kk alone, and an
// applied change delta of coordinate a is ONE update g_b -= Q[a][b] delta of every candidate b (a itself included).
// SWEEP.  The cyclic order is kept without one step per coordinate: every lane evaluates the rule of its coordinate from the current
// g, a ballot finds the lowest coordinate at or behind the scan position whose weight would change, that one is applied and the scan
// resumes behind it.  A coordinate that does not change leaves g alone, so what the lanes evaluated for the coordinates before the
// first changer is what the sequential loop would have found: the iterates are the sequential ones.
//   slim_wave_kernel   1 <= c <= 64: one wave per target, four targets per workgroup.  Lane b holds candidate b in registers; the
//                      c x c sub-Gram sits in LDS as fp32 (integer counts below 2^24: exact), 16 KB per wave, row a read by all
//                      lanes at once.  No barrier, no atomics.
//   slim_group_kernel  c > 64 (or every target when the caller asks): one 256-thread workgroup per target, the state in dynamic LDS
//                      (24 bytes per candidate), the scan in chunks of 256 coordinates with one LDS minimum across the four waves,
//                      the row of G behind an applied coordinate gathered from memory at the candidates' columns.
// Every reduction has a fixed shape (xor butterfly within a wave, then waves in order): two runs are bit-equal.
#include <climits>
#include <cmath>

#include "rsa_launch.hpp"
#include "rsa_lds.hpp"

namespace rsa {

constexpr int SLIM_WAVE_TARGETS = 4, SLIM_WAVE_THREADS = SLIM_WAVE_TARGETS * WAVE;
constexpr int SLIM_GROUP_THREADS = 256, SLIM_GROUP_WAVES = SLIM_GROUP_THREADS / WAVE;
constexpr int SLIM_SLOT_BYTES = 8 + 8 + 4 + 4;           // g, w (float64), id (int32), Q_kk (fp32, exact)
constexpr int SLIM_GROUP_STATIC = 1024;                   // the reduction and scan words of the workgroup kernel, rounded up
static_assert((LDS_LIMIT - SLIM_GROUP_STATIC) / SLIM_SLOT_BYTES == RSA_SLIM_MAX_CANDIDATES, "the header's limit is what the LDS holds");
static_assert(SLIM_WAVE_TARGETS * WAVE * WAVE * 4 <= LDS_STATIC_LIMIT, "four fp32 sub-Grams are the static LDS of one workgroup");

struct SlimParams {
  const double* g;
  const int32_t* order;
  int64_t n_items, ld, n_order;
  double l1, l2, tol;
  int32_t max_iter, cap;
  int32_t* nbr_id;
  double* nbr_w;
  int32_t *nbr_cnt, *n_iter;
};

// sklearn's coordinate update with positive = True, from g = q_k - H_k (H with the coordinate's own term still in it)
__device__ __forceinline__ double slim_rule(double g, double w, double d, double l1, double l2) {
  const double tmp = g + w * d;
  const double over = tmp - l1;
  return (tmp < 0.0 || !(over > 0.0)) ? 0.0 : over / (d + l2);
}

// the five wave- or workgroup-wide figures of the duality gap, in this order: sum w q, sum w H, sum w^2, sum |w|, max XtA
constexpr int SLIM_SUMS = 4, SLIM_FIGURES = 5;

__device__ __forceinline__ void slim_gap_terms(double (&f)[SLIM_FIGURES], double q, double g, double w, double l2) {
  f[0] += w * q;
  f[1] += w * (q - g);
  f[2] += w * w;
  f[3] += fabs(w);
  f[4] = fmax(f[4], g - l2 * w);
}

__device__ __forceinline__ double slim_gap(const double (&f)[SLIM_FIGURES], double yy, double l1, double l2) {
  const double r2 = yy + f[1] - 2.0 * f[0];
  double c = 1.0, gap = r2;
  if (f[4] > l1) {
    c = l1 / f[4];
    gap = 0.5 * (r2 + r2 * (c * c));
  }
  return gap + (l1 * f[3] - c * yy + c * f[0] + 0.5 * l2 * (1.0 + c * c) * f[2]);
}

__device__ __forceinline__ double slim_wave_sum(double v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}
__device__ __forceinline__ double slim_wave_max(double v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v = fmax(v, __shfl_xor(v, m, 64));
  return v;
}
__device__ __forceinline__ uint64_t slim_lanes_below(int lane) { return (1ull << lane) - 1ull; }

// ---------------------------------------------------------------- one wave per target
__global__ __launch_bounds__(SLIM_WAVE_THREADS) void slim_wave_kernel(const SlimParams p) {
  __shared__ double slim_sub[SLIM_WAVE_TARGETS][WAVE * WAVE / 2];      // per wave: 64 x 64 fp32
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t at = (int64_t)blockIdx.x * SLIM_WAVE_TARGETS + wave;
  if (at >= p.n_order) return;                                         // per wave; nothing below waits for another wave
  const int32_t j = p.order[at];
  if ((uint32_t)j >= (uint32_t)p.n_items) return;
  const double* grow = p.g + (int64_t)j * p.ld;
  float* qs = reinterpret_cast<float*>(slim_sub[wave]);
  // the candidates, ascending: the r-th one goes to lane r through the (still unused) first row of the sub-Gram
  int32_t* stage = reinterpret_cast<int32_t*>(qs);
  int c = 0;
  for (int64_t k0 = 1; k0 < p.n_items && c < WAVE; k0 += WAVE) {
    const int64_t k = k0 + lane;
    const bool is = k < p.n_items && k != j && grow[k] > p.l1;
    const uint64_t m = __ballot(is);
    const int r = c + __popcll(m & slim_lanes_below(lane));
    if (is && r < WAVE) stage[r] = (int32_t)k;
    c += __popcll(m);
  }
  c = c < WAVE ? c : WAVE;
  __builtin_amdgcn_wave_barrier();
  const bool live = lane < c;
  const int32_t id = live ? stage[lane] : 0;
  __builtin_amdgcn_wave_barrier();
  const double q = live ? grow[id] : 0.0;
  for (int r = 0; r < c; ++r) {                                         // row r of the sub-Gram: G[id_r, id_b]
    const int32_t idr = __shfl(id, r, 64);
    if (live) qs[r * WAVE + lane] = (float)p.g[(int64_t)idr * p.ld + id];
  }
  __builtin_amdgcn_wave_barrier();
  const double d = live ? (double)qs[lane * WAVE + lane] : 1.0;
  const double yy = grow[j], gap_tol = p.tol * yy;
  double w = 0.0, g = q;
  int it = 0;
  for (;;) {
    double dmax = 0.0;
    uint64_t ahead = ~0ull;                                              // the coordinates this sweep has not passed yet
    for (;;) {
      const double wn = slim_rule(g, w, d, p.l1, p.l2);
      const double delta = wn - w;
      const uint64_t m = __ballot(live && delta != 0.0) & ahead;
      if (m == 0) break;
      const int a = __ffsll((long long)m) - 1;
      const double da = __shfl(delta, a, 64);
      if (lane == a) w = wn, dmax = fmax(dmax, fabs(delta));
      if (live) g -= (double)qs[a * WAVE + lane] * da;
      if (a == WAVE - 1) break;
      ahead = ~0ull << (a + 1);
    }
    const double w_max = slim_wave_max(fabs(w)), d_w_max = slim_wave_max(dmax);
    const bool last = it == p.max_iter - 1;
    if (w_max == 0.0 || d_w_max / w_max < p.tol || last) {
      double f[SLIM_FIGURES] = {0.0, 0.0, 0.0, 0.0, 0.0};               // XtA of coordinate j itself is 0
      if (live) slim_gap_terms(f, q, g, w, p.l2);
#pragma unroll
      for (int x = 0; x < SLIM_SUMS; ++x) f[x] = slim_wave_sum(f[x]);
      f[4] = slim_wave_max(f[4]);
      if (slim_gap(f, yy, p.l1, p.l2) < gap_tol || last) break;
    }
    ++it;
  }
  const bool nz = live && w != 0.0;
  const uint64_t m = __ballot(nz);
  const int r = __popcll(m & slim_lanes_below(lane)), cnt = __popcll(m);
  if (nz && r < p.cap) {
    p.nbr_id[(int64_t)j * p.cap + r] = id;
    p.nbr_w[(int64_t)j * p.cap + r] = w;
  }
  if (lane == 0) {
    p.nbr_cnt[j] = cnt < p.cap ? cnt : p.cap;
    p.n_iter[j] = it + 1;
  }
}

// ---------------------------------------------------------------- one workgroup per target
// v[0 .. NS) are summed, v[NS .. N) maximised: butterfly within the wave, then the four waves in order.  Every thread calls it.
template <int NS, int N>
__device__ __forceinline__ void slim_group_reduce(double (&v)[N], double (*red)[SLIM_GROUP_WAVES]) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int x = 0; x < N; ++x) {
    v[x] = x < NS ? slim_wave_sum(v[x]) : slim_wave_max(v[x]);
    if (lane == 0) red[x][wave] = v[x];
  }
  __syncthreads();
#pragma unroll
  for (int x = 0; x < N; ++x)
    v[x] = x < NS ? (red[x][0] + red[x][1]) + (red[x][2] + red[x][3]) : fmax(fmax(red[x][0], red[x][1]), fmax(red[x][2], red[x][3]));
  __syncthreads();
}

// the rank of this thread's flag among the workgroup's set flags (threads ascending) and their number; every thread calls it
__device__ __forceinline__ int slim_group_rank(bool flag, int32_t* cnt, int& total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint64_t m = __ballot(flag);
  if (lane == 0) cnt[wave] = __popcll(m);
  __syncthreads();
  int r = __popcll(m & slim_lanes_below(lane));
  total = 0;
#pragma unroll
  for (int x = 0; x < SLIM_GROUP_WAVES; ++x) {
    if (x < wave) r += cnt[x];
    total += cnt[x];
  }
  __syncthreads();
  return r;
}

__global__ __launch_bounds__(SLIM_GROUP_THREADS) void slim_group_kernel(const SlimParams p) {
  extern __shared__ double slim_state[];
  __shared__ double s_red[SLIM_FIGURES][SLIM_GROUP_WAVES];
  __shared__ double s_delta[2][SLIM_GROUP_WAVES];
  __shared__ int32_t s_first[2][SLIM_GROUP_WAVES];
  __shared__ int32_t s_cnt[SLIM_GROUP_WAVES];
  static_assert(sizeof(double) * (SLIM_FIGURES + 2) * SLIM_GROUP_WAVES + 4 * 3 * SLIM_GROUP_WAVES <= SLIM_GROUP_STATIC, "the static words");
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int32_t j = p.order[blockIdx.x];
  if ((uint32_t)j >= (uint32_t)p.n_items) return;                        // the whole workgroup
  const int cap = p.cap;
  double *sg = slim_state, *sw = sg + cap;
  int32_t* sid = reinterpret_cast<int32_t*>(sw + cap);
  float* sd = reinterpret_cast<float*>(sid + cap);
  const double* grow = p.g + (int64_t)j * p.ld;
  int c = 0;
  for (int64_t k0 = 1; k0 < p.n_items; k0 += SLIM_GROUP_THREADS) {       // the candidates, ascending
    const int64_t k = k0 + t;
    const double v = k < p.n_items ? grow[k] : 0.0;
    const bool is = k < p.n_items && k != j && v > p.l1;
    int total;
    const int r = c + slim_group_rank(is, s_cnt, total);
    if (is && r < cap) sid[r] = (int32_t)k, sg[r] = v, sw[r] = 0.0;
    c += total;
  }
  c = c < cap ? c : cap;
  __syncthreads();
  for (int m = t; m < c; m += SLIM_GROUP_THREADS) sd[m] = (float)p.g[(int64_t)sid[m] * (p.ld + 1)];
  __syncthreads();
  const double yy = grow[j], gap_tol = p.tol * yy;
  int it = 0, par = 0;
  for (;;) {
    double dmax = 0.0;
    int pos = 0;
    while (pos < c) {
      const int k = pos + t;
      double wn = 0.0, delta = 0.0;
      if (k < c) {
        wn = slim_rule(sg[k], sw[k], (double)sd[k], p.l1, p.l2);
        delta = wn - sw[k];
      }
      const uint64_t m = __ballot(delta != 0.0);
      const int first = m ? __ffsll((long long)m) - 1 : -1;
      if (lane == 0 && first < 0) s_first[par][wave] = INT_MAX;
      if (lane == first) s_first[par][wave] = k, s_delta[par][wave] = delta;
      __syncthreads();
      int hit = 0;                                                       // the first wave with a changer holds the lowest one
      while (hit < SLIM_GROUP_WAVES && s_first[par][hit] == INT_MAX) ++hit;
      if (hit == SLIM_GROUP_WAVES) {                                     // nothing in these 256 changes
        pos += SLIM_GROUP_THREADS, par ^= 1;
        continue;
      }
      const int a = s_first[par][hit];
      const double da = s_delta[par][hit];
      if (k == a) sw[k] = wn, dmax = fmax(dmax, fabs(delta));
      const double* row = p.g + (int64_t)sid[a] * p.ld;
      for (int b = t; b < c; b += SLIM_GROUP_THREADS) sg[b] -= row[sid[b]] * da;
      __syncthreads();
      pos = a + 1, par ^= 1;
    }
    double mx[2] = {0.0, dmax};
    for (int b = t; b < c; b += SLIM_GROUP_THREADS) mx[0] = fmax(mx[0], fabs(sw[b]));
    slim_group_reduce<0>(mx, s_red);
    const bool last = it == p.max_iter - 1;
    if (mx[0] == 0.0 || mx[1] / mx[0] < p.tol || last) {
      double f[SLIM_FIGURES] = {0.0, 0.0, 0.0, 0.0, 0.0};
      for (int b = t; b < c; b += SLIM_GROUP_THREADS) slim_gap_terms(f, grow[sid[b]], sg[b], sw[b], p.l2);
      slim_group_reduce<SLIM_SUMS>(f, s_red);
      if (slim_gap(f, yy, p.l1, p.l2) < gap_tol || last) break;
    }
    ++it;
  }
  int cnt = 0;
  for (int b0 = 0; b0 < c; b0 += SLIM_GROUP_THREADS) {                    // the non-zeros, still ascending
    const int b = b0 + t;
    const bool nz = b < c && sw[b] != 0.0;
    int total;
    const int r = cnt + slim_group_rank(nz, s_cnt, total);
    if (nz && r < cap) {
      p.nbr_id[(int64_t)j * cap + r] = sid[b];
      p.nbr_w[(int64_t)j * cap + r] = sw[b];
    }
    cnt += total;
  }
  if (t == 0) {
    p.nbr_cnt[j] = cnt < cap ? cnt : cap;
    p.n_iter[j] = it + 1;
  }
}

}  // namespace rsa

using namespace rsa;

extern "C" int rsa_slim_fit(const rsa_slim_fit_args* args, rsa_stream_t stream) {
  const char* fn = "rsa_slim_fit";
  rsa_slim_fit_args a;
  if (int rc = load_args(a, args, fn)) return rc;
  RSA_CHECK_ARG(a.n_items >= 2 && a.n_items < (1ll << 31), "%s: n_items = %lld is out of range (n_items >= 2: item 0 is the padding)", fn,
                (long long)a.n_items);
  RSA_CHECK_ARG(a.ld >= a.n_items, "%s: ld = %lld is below n_items = %lld", fn, (long long)a.ld, (long long)a.n_items);
  RSA_CHECK_ARG(a.cap >= 1, "%s: cap = %d must be >= 1", fn, a.cap);
  RSA_CHECK_ARG(a.l1 >= 0.0 && std::isfinite(a.l1), "%s: l1 = %g must be finite and >= 0", fn, a.l1);
  RSA_CHECK_ARG(a.l2 > 0.0 && std::isfinite(a.l2), "%s: l2 = %g must be finite and > 0 (at 0 the minimiser is not unique)", fn, a.l2);
  RSA_CHECK_ARG(a.tol >= 0.0 && std::isfinite(a.tol), "%s: tol = %g must be finite and >= 0", fn, a.tol);
  RSA_CHECK_ARG(a.max_iter >= 1, "%s: max_iter = %d must be >= 1", fn, a.max_iter);
  RSA_CHECK_ARG(a.n_wave >= 0 && a.n_group >= 0 && a.n_wave + a.n_group <= a.n_items,
                "%s: n_wave = %lld, n_group = %lld out of range (together at most n_items)", fn, (long long)a.n_wave, (long long)a.n_group);
  RSA_CHECK_ARG(a.n_group == 0 || a.cap <= RSA_SLIM_MAX_CANDIDATES, "%s: cap = %d candidates do not fit the LDS of one workgroup (at "
                "most %d): raise l1 = alpha * l1_ratio * U", fn, a.cap, RSA_SLIM_MAX_CANDIDATES);
  RSA_CHECK_ARG(a.g != nullptr, "%s: g is null", fn);
  RSA_CHECK_ARG(a.n_wave == 0 || a.order_wave != nullptr, "%s: order_wave is null", fn);
  RSA_CHECK_ARG(a.n_group == 0 || a.order_group != nullptr, "%s: order_group is null", fn);
  RSA_CHECK_ARG(a.nbr_id != nullptr, "%s: nbr_id is null", fn);
  RSA_CHECK_ARG(a.nbr_w != nullptr, "%s: nbr_w is null", fn);
  RSA_CHECK_ARG(a.nbr_cnt != nullptr, "%s: nbr_cnt is null", fn);
  RSA_CHECK_ARG(a.n_iter != nullptr, "%s: n_iter is null", fn);
  SlimParams p{};
  p.g = a.g, p.n_items = a.n_items, p.ld = a.ld, p.l1 = a.l1, p.l2 = a.l2, p.tol = a.tol, p.max_iter = a.max_iter, p.cap = a.cap;
  p.nbr_id = a.nbr_id, p.nbr_w = a.nbr_w, p.nbr_cnt = a.nbr_cnt, p.n_iter = a.n_iter;
  hipStream_t s = (hipStream_t)stream;
  if (a.n_group > 0) {                                                   // the heavy targets first
    p.order = a.order_group, p.n_order = a.n_group;
    const int64_t lds = (int64_t)a.cap * SLIM_SLOT_BYTES;
    if (int rc = allow_lds<slim_group_kernel>(lds, fn)) return rc;
    hipLaunchKernelGGL(slim_group_kernel, dim3((unsigned)a.n_group), dim3(SLIM_GROUP_THREADS), (size_t)lds, s, p);
    RSA_CHECK_LAUNCH(fn);
  }
  if (a.n_wave > 0) {
    p.order = a.order_wave, p.n_order = a.n_wave;
    const unsigned blocks = (unsigned)((a.n_wave + SLIM_WAVE_TARGETS - 1) / SLIM_WAVE_TARGETS);
    hipLaunchKernelGGL(slim_wave_kernel, dim3(blocks), dim3(SLIM_WAVE_THREADS), 0, s, p);
    RSA_CHECK_LAUNCH(fn);
  }
  return RSA_OK;
}
