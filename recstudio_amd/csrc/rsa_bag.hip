// Bag sum of embedding rows straight from a padded id matrix, and its backward (MultiDAE / MultiVAE: the encoder input
// `item_embedding(ids).sum(1) / count_nonzero(ids, 1) ** 0.5` and the per-user mean of the positives' rows in the softmax loss).
//   out[b] = s_b * sum_{l : ids[b, l] live} table[ids[b, l]]      s_b = 1 | cnt_b^-1/2 | 1 / cnt_b      cnt_b = live ids of row b
//   dW[i]  = sum_{(b, l) : ids[b, l] = i} s_b * g[b]
// Nothing of size B L d exists: the forward reads the live rows only, the backward sorts the step's (item, bag) pairs.
//
// LIVE.  An id is live when it is > 0; id 0 (padding, anywhere in the row) and negative ids are skipped, NOT read.  A live id
// >= n_rows reads row n_rows - 1 (never past the table).
//
// FORWARD.  One 256-thread workgroup per (bag, chunk of BAG_CHUNK = 256 id positions).  It reads its 256 ids once, compacts the
// live ones into LDS in position order (ballot + popcount: no atomics), and sums their rows: a 16-byte column per thread,
// RP = min(256 / (d / 4), BAG_RP_MAX) row slots side by side, slot r taking live rows r, r + RP, r + 2 RP, ... in that order with
// BAG_UNROLL = 4 loads in flight, each into an accumulator of its own (row r + k RP goes to accumulator k mod 4; the tail's loads
// are issued on the chunk's last live row and dropped by a select, never predicated), paired (0 + 1) + (2 + 3) at the end; the
// slots' sums are then added in slot order through LDS.  bag_len <= BAG_CHUNK: the workgroup scales and writes
// out[b] itself (one launch).  Longer rows: every non-empty chunk leaves its sum and its count in the caller's workspace and a
// second launch adds a bag's non-empty chunks in chunk order, scales and writes.  An accumulator starts at +0 and so never holds
// -0: an all-padding chunk changes no bit, and the order of the additions depends on d and on that row's ids alone -- the same
// bag gives the same bits at any batch position, in any batch width, on any run.
//
// BACKWARD.  (1) the in-tree radix sort over all n_bags * bag_len positions, pass 0 reading the id matrix (SrcBagIds: key = the
// row, padding = key n_rows, payload = the bag); stable, so equal items stay in (bag, position) order.  (2) one thread per sorted
// pair marks where each item's run starts and ends (every item has one run: plain stores, no atomics).  (3) a wave per item with
// a run adds s_b * g[b] (s_b computed once per bag) over the run in sorted order (pair j of the run into accumulator j mod 4, paired
// (0 + 1) + (2 + 3)), 64 16-byte columns at a time, and stores the row once.
#include "rsa_internal.hpp"
#include "rsa_radix.hpp"

namespace rsa {

constexpr int BAG_CHUNK = 256;         // id positions per workgroup = threads per workgroup
constexpr int BAG_RP_MAX = 16;         // row slots side by side (narrow tables)
constexpr int BAG_UNROLL = 4;          // independent 16-byte row loads in flight per thread
constexpr int BAG_MAX_DIM = 1024;      // d / 4 <= 256 columns: one thread per column
constexpr int BAG_WALK_GRID = 1 << 16;

__device__ __forceinline__ float bag_scale(int mode, int cnt) {
  // cnt ** -0.5 through float64, rounded to fp32 ONCE (sqrtf then a divide round twice); cnt == 0: inf, and inf * 0 = NaN
  // (torch's 0 / 0)
  if (mode == RSA_BAG_RSQRT) return (float)(1.0 / sqrt((double)cnt));
  if (mode == RSA_BAG_MEAN) return 1.0f / (float)cnt;
  return 1.0f;
}

struct BagParams {
  const float* table;
  const int64_t* ids;
  int64_t ids_stride, n_rows, n_bags;
  int32_t L, d, ncol, rp, mode, n_chunks;
  float* out;
  int32_t* cnt;
  float* part;         // [n_bags, n_chunks, d]  (chunked form)
  int32_t* ccnt;       // [n_bags, n_chunks]
};

// CHUNKED = false: n_chunks == 1, the workgroup writes out / cnt.  true: it writes its partial sum (when it has live rows) and count.
template <bool CHUNKED>
__global__ __launch_bounds__(BAG_CHUNK) void bag_pool_kernel(const BagParams p) {
  __shared__ int32_t s_rows[BAG_CHUNK];
  __shared__ int32_t s_wave[4];
  __shared__ float4 s_part[BAG_CHUNK];
  const int t = threadIdx.x, lane = lane_id(), wave = t >> 6;
  const int64_t b = CHUNKED ? (int64_t)(blockIdx.x / (uint32_t)p.n_chunks) : (int64_t)blockIdx.x;
  const int chunk = CHUNKED ? (int)(blockIdx.x - (uint32_t)b * (uint32_t)p.n_chunks) : 0;
  const int pos = chunk * BAG_CHUNK + t;
  int64_t id = 0;
  if (pos < p.L) id = p.ids[b * p.ids_stride + pos];
  const bool live = id > 0;
  const int32_t row = (int32_t)(id >= p.n_rows ? p.n_rows - 1 : id);
  const uint64_t bal = __ballot(live);
  if (lane == 0) s_wave[wave] = (int32_t)__popcll(bal);
  __syncthreads();
  int base = 0, n_live = 0;
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    const int c = s_wave[w];
    if (w < wave) base += c;
    n_live += c;
  }
  if (live) s_rows[base + (int)__popcll(bal & ((1ull << lane) - 1ull))] = row;
  __syncthreads();
  if (CHUNKED) {
    if (t == 0) p.ccnt[blockIdx.x] = n_live;
    if (n_live == 0) return;                     // workgroup-uniform
  }
  const int rslot = t / p.ncol, col = t - rslot * p.ncol;
  const bool active = rslot < p.rp;
  float4 au[BAG_UNROLL];          // one accumulator per load in flight: chains a quarter as long
#pragma unroll
  for (int u = 0; u < BAG_UNROLL; ++u) au[u] = make_float4(0.f, 0.f, 0.f, 0.f);
  if (active && n_live > 0) {
    const float* tcol = p.table + (size_t)col * 4;
    const int last = n_live - 1;
    for (int j0 = rslot; j0 < n_live; j0 += BAG_UNROLL * p.rp) {
      float4 v[BAG_UNROLL];
#pragma unroll
      for (int u = 0; u < BAG_UNROLL; ++u) {
        const int j = j0 + u * p.rp;
        const int32_t r = s_rows[j < last ? j : last];
        v[u] = *reinterpret_cast<const float4*>(tcol + (size_t)r * (size_t)p.d);
      }
#pragma unroll
      for (int u = 0; u < BAG_UNROLL; ++u) {
        const bool ok = j0 + u * p.rp < n_live;
        au[u].x += ok ? v[u].x : 0.f;
        au[u].y += ok ? v[u].y : 0.f;
        au[u].z += ok ? v[u].z : 0.f;
        au[u].w += ok ? v[u].w : 0.f;
      }
    }
  }
  static_assert(BAG_UNROLL == 4, "the accumulators are paired (0 + 1) + (2 + 3)");
  float4 acc = make_float4((au[0].x + au[1].x) + (au[2].x + au[3].x), (au[0].y + au[1].y) + (au[2].y + au[3].y),
                           (au[0].z + au[1].z) + (au[2].z + au[3].z), (au[0].w + au[1].w) + (au[2].w + au[3].w));
  if (p.rp > 1) {
    if (active && rslot > 0) s_part[t] = acc;
    __syncthreads();
    if (rslot == 0) {
      const int used = n_live < p.rp ? n_live : p.rp;      // slots that added a row (the others hold +0)
      for (int r = 1; r < used; ++r) {
        const float4 o = s_part[r * p.ncol + col];
        acc.x += o.x, acc.y += o.y, acc.z += o.z, acc.w += o.w;
      }
    }
  }
  if (rslot != 0) return;
  if (CHUNKED) {
    *reinterpret_cast<float4*>(p.part + ((size_t)blockIdx.x * (size_t)p.d + (size_t)col * 4)) = acc;
  } else {
    const float s = bag_scale(p.mode, n_live);
    if (p.mode != RSA_BAG_SUM) acc.x *= s, acc.y *= s, acc.z *= s, acc.w *= s;
    *reinterpret_cast<float4*>(p.out + ((size_t)b * (size_t)p.d + (size_t)col * 4)) = acc;
    if (t == 0) p.cnt[b] = n_live;
  }
}

// one workgroup per bag: its non-empty chunks in chunk order
__global__ __launch_bounds__(BAG_CHUNK) void bag_merge_kernel(const BagParams p) {
  const int64_t b = blockIdx.x;
  const int col = threadIdx.x;
  const int32_t* cc = p.ccnt + (size_t)b * p.n_chunks;
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  int cnt = 0;
  for (int k = 0; k < p.n_chunks; ++k) {
    const int c = cc[k];                          // workgroup-uniform
    if (c > 0 && col < p.ncol) {
      const float4 o = *reinterpret_cast<const float4*>(p.part + (((size_t)b * p.n_chunks + k) * (size_t)p.d + (size_t)col * 4));
      acc.x += o.x, acc.y += o.y, acc.z += o.z, acc.w += o.w;
    }
    cnt += c;
  }
  if (col < p.ncol) {
    const float s = bag_scale(p.mode, cnt);
    if (p.mode != RSA_BAG_SUM) acc.x *= s, acc.y *= s, acc.z *= s, acc.w *= s;
    *reinterpret_cast<float4*>(p.out + ((size_t)b * (size_t)p.d + (size_t)col * 4)) = acc;
  }
  if (col == 0) p.cnt[b] = cnt;
}

// ---------------------------------------------------------------- backward
// pass-0 source of the radix sort: element e = b * L + l of the padded id matrix -> (row | n_rows for padding, bag)
struct SrcBagIds {
  const int64_t* ids;
  int64_t ids_stride, n_rows;
  Div32 by_len;
  __device__ __forceinline__ uint64_t operator()(int64_t e) const {
    const uint32_t b = by_len.div((uint32_t)e), l = (uint32_t)e - b * by_len.d;      // e < 2^31 (checked by the host)
    const int64_t id = ids[(int64_t)b * ids_stride + l];
    const uint32_t key = id > 0 ? (uint32_t)(id >= n_rows ? n_rows - 1 : id) : (uint32_t)n_rows;
    return rdx_pack(key, b);
  }
};

// run_end[i] = one past the last sorted pair of item i, run_start[i] its first (run_end is zeroed before: 0 = no run)
__global__ __launch_bounds__(256) void bag_runs_kernel(const uint64_t* __restrict__ pairs, int64_t total, uint32_t n_rows,
                                                       int32_t* __restrict__ run_start, int32_t* __restrict__ run_end) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const uint32_t k = rdx_key(pairs[i]);
  if (k >= n_rows) return;                        // padding (key n_rows): behind every run
  const uint32_t prev = i > 0 ? rdx_key(pairs[i - 1]) : 0xffffffffu;
  const uint32_t next = i + 1 < total ? rdx_key(pairs[i + 1]) : 0xffffffffu;
  if (prev != k) run_start[k] = (int32_t)i;
  if (next != k) run_end[k] = (int32_t)(i + 1);
}

// s_b of every bag, once (the walk reads it per pair)
__global__ __launch_bounds__(256) void bag_scale_kernel(const int32_t* __restrict__ cnt, int64_t n_bags, int mode, float* __restrict__ scale) {
  const int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (b < n_bags) scale[b] = bag_scale(mode, cnt[b]);
}

struct BagWalkParams {
  const uint64_t* pairs;
  const int32_t *run_start, *run_end;
  const float* scale;
  const float* g;
  float* dw;
  int64_t n_rows, n_bags;
  int32_t d, ncol;
};

__global__ __launch_bounds__(256) void bag_walk_kernel(const BagWalkParams p) {
  const int lane = lane_id();
  const int64_t n_waves = (int64_t)gridDim.x * 4;
  for (int64_t item = 1 + (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); item < p.n_rows; item += n_waves) {
    const int32_t e = p.run_end[item];            // wave-uniform
    if (e <= 0) continue;
    const int32_t s = p.run_start[item];
    for (int c0 = 0; c0 < p.ncol; c0 += 64) {
      const int col = c0 + lane < p.ncol ? c0 + lane : p.ncol - 1;      // the spare lanes redo the last column and store nothing
      const float* gcol = p.g + (size_t)col * 4;
      float4 au[BAG_UNROLL];
#pragma unroll
      for (int u = 0; u < BAG_UNROLL; ++u) au[u] = make_float4(0.f, 0.f, 0.f, 0.f);
      for (int32_t j0 = s; j0 < e; j0 += BAG_UNROLL) {
        float4 v[BAG_UNROLL];
        float sc[BAG_UNROLL];
#pragma unroll
        for (int u = 0; u < BAG_UNROLL; ++u) {
          const int32_t j = j0 + u < e ? j0 + u : e - 1;
          uint32_t b = rdx_val(p.pairs[j]);
          b = b < (uint32_t)p.n_bags ? b : (uint32_t)p.n_bags - 1;
          sc[u] = p.scale[b];
          v[u] = *reinterpret_cast<const float4*>(gcol + (size_t)b * (size_t)p.d);
        }
#pragma unroll
        for (int u = 0; u < BAG_UNROLL; ++u) {
          const bool ok = j0 + u < e;
          const float m = ok ? sc[u] : 0.f;
          au[u].x += ok ? m * v[u].x : 0.f;
          au[u].y += ok ? m * v[u].y : 0.f;
          au[u].z += ok ? m * v[u].z : 0.f;
          au[u].w += ok ? m * v[u].w : 0.f;
        }
      }
      const float4 acc = make_float4((au[0].x + au[1].x) + (au[2].x + au[3].x), (au[0].y + au[1].y) + (au[2].y + au[3].y),
                                     (au[0].z + au[1].z) + (au[2].z + au[3].z), (au[0].w + au[1].w) + (au[2].w + au[3].w));
      if (c0 + lane < p.ncol) *reinterpret_cast<float4*>(p.dw + ((size_t)item * (size_t)p.d + (size_t)col * 4)) = acc;
    }
  }
}

// ---------------------------------------------------------------- host
struct BagLayout {
  uint64_t *pairs_a, *pairs_b;
  void* temp;
  int32_t *run_start, *run_end;
  float* part;
  int32_t* ccnt;
  float* scale;
};

static inline int bag_chunks(int32_t L) { return L <= BAG_CHUNK ? 1 : (L + BAG_CHUNK - 1) / BAG_CHUNK; }

// the forward's partial sums are sized for the widest table (d = BAG_MAX_DIM): the size query does not take d
static BagLayout bag_layout(Carver& cv, int64_t B, int32_t L, int64_t N) {
  BagLayout y{};
  const int64_t total = B * (int64_t)L;
  y.pairs_a = cv.take<uint64_t>(total);
  y.pairs_b = cv.take<uint64_t>(total);
  y.temp = cv.take<char>(radix_temp_bytes(total));
  y.run_start = cv.take<int32_t>(N + 1);
  y.run_end = cv.take<int32_t>(N + 1);
  const int64_t chunks = L > BAG_CHUNK ? B * bag_chunks(L) : 0;
  y.part = cv.take<float>(chunks * BAG_MAX_DIM);
  y.ccnt = cv.take<int32_t>(chunks);
  y.scale = cv.take<float>(B);
  return y;
}

static bool bag_sizes_ok(int64_t B, int32_t L, int64_t N) {
  return B >= 0 && L >= 0 && N >= 1 && N < (1ll << 31) - 1 && B < (1ll << 31) && B * (int64_t)(L > 0 ? L : 1) < (1ll << 31) &&
         B * (int64_t)bag_chunks(L) < (1ll << 31);
}

static int bag_check(const rsa_bag_args& a, const char* fn) {
  RSA_CHECK_ARG(bag_sizes_ok(a.n_bags, a.bag_len, a.n_rows), "%s: n_bags = %lld, bag_len = %d, n_rows = %lld out of range (n_bags * bag_len "
                "and n_rows must stay below 2^31)", fn, (long long)a.n_bags, a.bag_len, (long long)a.n_rows);
  RSA_CHECK_ARG(a.d >= 4 && a.d <= BAG_MAX_DIM && a.d % 4 == 0, "%s: d = %d must be a multiple of 4 in [4, %d]", fn, a.d, BAG_MAX_DIM);
  RSA_CHECK_ARG(a.scale == RSA_BAG_SUM || a.scale == RSA_BAG_RSQRT || a.scale == RSA_BAG_MEAN, "%s: scale = %d is not RSA_BAG_SUM, "
                "RSA_BAG_RSQRT or RSA_BAG_MEAN", fn, a.scale);
  if (a.n_bags == 0) return RSA_OK;
  RSA_CHECK_ARG(a.bag_len == 0 || a.ids != nullptr, "%s: ids is null", fn);
  RSA_CHECK_ARG(a.ids_stride >= a.bag_len, "%s: ids_stride = %lld is below bag_len = %d", fn, (long long)a.ids_stride, a.bag_len);
  RSA_CHECK_ARG(a.cnt != nullptr, "%s: cnt is null", fn);
  return RSA_OK;
}

}  // namespace rsa

using namespace rsa;

extern "C" int64_t rsa_bag_pool_workspace_bytes(int64_t n_bags, int32_t bag_len, int64_t n_rows) {
  if (!bag_sizes_ok(n_bags, bag_len, n_rows)) return -1;
  Carver cv(nullptr);
  bag_layout(cv, n_bags, bag_len, n_rows);
  return cv.bytes() + 256;
}

extern "C" int rsa_bag_pool(const rsa_bag_args* args, rsa_stream_t stream) {
  const char* fn = "rsa_bag_pool";
  rsa_bag_args a;
  if (int rc = load_args(a, args, fn)) return rc;
  if (int rc = bag_check(a, fn)) return rc;
  if (a.n_bags == 0) return RSA_OK;
  RSA_CHECK_ARG(a.table && ((uintptr_t)a.table & 15) == 0, "%s: table is null or not 16-byte aligned", fn);
  RSA_CHECK_ARG(a.out && ((uintptr_t)a.out & 15) == 0, "%s: out is null or not 16-byte aligned", fn);
  BagParams p{};
  p.table = a.table, p.ids = a.ids, p.ids_stride = a.ids_stride, p.n_rows = a.n_rows, p.n_bags = a.n_bags;
  p.L = a.bag_len, p.d = a.d, p.ncol = a.d / 4, p.mode = a.scale, p.n_chunks = bag_chunks(a.bag_len);
  p.rp = BAG_CHUNK / p.ncol < BAG_RP_MAX ? BAG_CHUNK / p.ncol : BAG_RP_MAX;
  p.out = a.out, p.cnt = a.cnt;
  hipStream_t s = (hipStream_t)stream;
  if (p.n_chunks == 1) {
    hipLaunchKernelGGL((bag_pool_kernel<false>), dim3((unsigned)a.n_bags), dim3(BAG_CHUNK), 0, s, p);
    RSA_CHECK_LAUNCH(fn);
    return RSA_OK;
  }
  RSA_CHECK_ARG(a.workspace != nullptr, "%s: workspace is null (bag_len > %d sums through it)", fn, BAG_CHUNK);
  const int64_t need = rsa_bag_pool_workspace_bytes(a.n_bags, a.bag_len, a.n_rows);
  RSA_CHECK_ARG(a.workspace_bytes >= need, "%s: the workspace is too small: %lld bytes, need %lld", fn, (long long)a.workspace_bytes,
                (long long)need);
  Carver cv(a.workspace);
  const BagLayout y = bag_layout(cv, a.n_bags, a.bag_len, a.n_rows);
  p.part = y.part, p.ccnt = y.ccnt;
  hipLaunchKernelGGL((bag_pool_kernel<true>), dim3((unsigned)(a.n_bags * p.n_chunks)), dim3(BAG_CHUNK), 0, s, p);
  RSA_CHECK_LAUNCH(fn);
  hipLaunchKernelGGL(bag_merge_kernel, dim3((unsigned)a.n_bags), dim3(BAG_CHUNK), 0, s, p);
  RSA_CHECK_LAUNCH(fn);
  return RSA_OK;
}

extern "C" int rsa_bag_pool_backward(const rsa_bag_args* args, rsa_stream_t stream) {
  const char* fn = "rsa_bag_pool_backward";
  rsa_bag_args a;
  if (int rc = load_args(a, args, fn)) return rc;
  if (int rc = bag_check(a, fn)) return rc;
  const int64_t total = a.n_bags * (int64_t)a.bag_len;
  if (total == 0 || a.n_rows < 2) return RSA_OK;
  RSA_CHECK_ARG(a.g && ((uintptr_t)a.g & 15) == 0, "%s: g is null or not 16-byte aligned", fn);
  RSA_CHECK_ARG(a.dw && ((uintptr_t)a.dw & 15) == 0, "%s: dw is null or not 16-byte aligned", fn);
  RSA_CHECK_ARG(a.workspace != nullptr, "%s: workspace is null", fn);
  const int64_t need = rsa_bag_pool_workspace_bytes(a.n_bags, a.bag_len, a.n_rows);
  RSA_CHECK_ARG(a.workspace_bytes >= need, "%s: the workspace is too small: %lld bytes, need %lld", fn, (long long)a.workspace_bytes,
                (long long)need);
  Carver cv(a.workspace);
  const BagLayout y = bag_layout(cv, a.n_bags, a.bag_len, a.n_rows);
  hipStream_t s = (hipStream_t)stream;
  const unsigned bits = radix_key_bits(a.n_rows + 1);
  const SrcBagIds src{a.ids, a.ids_stride, a.n_rows, make_div32((uint64_t)a.bag_len)};
  RSA_CHECK_HIP(radix_sort_pairs(src, y.pairs_a, y.pairs_b, total, bits, y.temp, s), fn);
  const uint64_t* sorted = radix_result(y.pairs_a, y.pairs_b, bits);
  RSA_CHECK_HIP(hipMemsetAsync(y.run_end, 0, (size_t)(a.n_rows + 1) * sizeof(int32_t), s), fn);
  hipLaunchKernelGGL(bag_runs_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, sorted, total, (uint32_t)a.n_rows,
                     y.run_start, y.run_end);
  RSA_CHECK_LAUNCH(fn);
  hipLaunchKernelGGL(bag_scale_kernel, dim3((unsigned)((a.n_bags + 255) / 256)), dim3(256), 0, s, a.cnt, a.n_bags, a.scale, y.scale);
  RSA_CHECK_LAUNCH(fn);
  BagWalkParams w{};
  w.pairs = sorted, w.run_start = y.run_start, w.run_end = y.run_end, w.scale = y.scale, w.g = a.g, w.dw = a.dw;
  w.n_rows = a.n_rows, w.n_bags = a.n_bags, w.d = a.d, w.ncol = a.d / 4;
  hipLaunchKernelGGL(bag_walk_kernel, dim3(grid_1d(a.n_rows - 1, 4, BAG_WALK_GRID)), dim3(256), 0, s, w);
  RSA_CHECK_LAUNCH(fn);
  return RSA_OK;
}
