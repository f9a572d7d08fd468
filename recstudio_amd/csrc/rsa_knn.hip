// ItemKNN (recstudio/model/mf/itemknn.py) on gfx950: the knn largest similarities of every column of R^T R without the matrix
// (rsa_knn_build) and history x neighbour lists -> dense scores (rsa_knn_score).  include/recstudio_amd.h states the contract,
// DESIGN.md 4.22 the design.
//
// BUILD.  One workgroup of 1024 threads owns one (target item i, tile of `tile` consecutive item ids) pair.
//   count    wave w takes the users w, w + 16, ... of users(i); its lanes walk that user's sorted row (from the tile's lower bound,
//            found by binary search when the catalog has several tiles) and add 1 to the LDS counter of every id inside the tile:
//            32-bit integer LDS atomics, exact and order-free.
//   score    every non-zero counter but i's own is replaced by the bits of its fp32 similarity (positive floats order as unsigned
//            integers); the non-zeros are counted.
//   select   only when the tile holds more than knn non-zeros: the knn-th largest 48-bit key (score bits << 16 | 0xffff - slot)
//            by a most-significant-digit radix search, six 8-bit passes over the LDS tile, one histogram per wave.  The keys are
//            distinct, so exactly knn slots are at or above the threshold and "the lower id wins a tie" needs no pass of its own.
//   gather   the winners as 64-bit sort keys (~score bits << 32 | id), a bitonic sort in LDS: descending score, ascending id.
//   emit     a one-tile catalog writes the neighbour lists; otherwise the sorted keys go to the workspace and knn_merge_kernel
//            ranks every candidate of an item among its tiles' lists (binary searches; the keys are distinct) and writes the first knn.
// SCORE.  One workgroup of 256 threads owns one (user, tile of target items) pair with the fp32 sums in LDS; see the header.
#include "rsa_csr.hpp"
#include "rsa_launch.hpp"
#include "rsa_lds.hpp"

namespace rsa {

constexpr int KNN_THREADS = 1024, KNN_WAVES = KNN_THREADS / WAVE, KNN_MAX_K = RSA_KNN_MAX_K, KNN_MAX_TILE = RSA_KNN_MAX_TILE;
constexpr int KNN_MERGE_THREADS = 256, KNN_SCORE_THREADS = 256, KNN_SCORE_TILE = 8192;
// LDS words in front of the tile: the sort keys (64-bit, first: 8-byte aligned), one 256-bin histogram per wave, a few scalars
constexpr int KNN_CAND_WORDS = 2 * KNN_MAX_K, KNN_HIST_WORDS = KNN_WAVES * 256, KNN_MISC_WORDS = 16;
constexpr int KNN_FIXED_WORDS = KNN_CAND_WORDS + KNN_HIST_WORDS + KNN_MISC_WORDS;
static_assert(KNN_THREADS >= KNN_MAX_K, "one thread per kept neighbour in the sort and the emit");
static_assert((int64_t)(KNN_FIXED_WORDS + KNN_MAX_TILE) * 4 <= LDS_LIMIT, "the default tile must fit the LDS of one workgroup");
static_assert((int64_t)(KNN_FIXED_WORDS + 2 * KNN_MAX_TILE) * 4 > LDS_LIMIT, "a larger power of two would fit: raise RSA_KNN_MAX_TILE");
static_assert(KNN_MAX_TILE <= 65536, "the select key keeps the slot in 16 bits");
enum { MISC_NNZ = 0, MISC_DIGIT = 1, MISC_NEED = 2, MISC_SLOT = 3 };

struct KnnBuildParams {
  const int64_t *u_indptr, *i_indptr;
  const int32_t *u_items, *i_users, *order;
  int64_t n_users, n_items;
  int32_t knn, tile, n_tiles, jaccard;
  int32_t *nbr_id, *nbr_cnt;
  float* nbr_sim;
  uint64_t* ws_key;      // [n_order, n_tiles, knn] sorted keys of every (item, tile)
  int32_t* ws_cnt;       // [n_order, n_tiles]
};

// fp32, every operation rounded once (-ffp-contract=off; hipcc's correctly rounded divide and sqrt are left on): the operation
// sequence tests/itemknn_referee.py derives its tolerance from.  The integer operands are exact below 2^24.
__device__ __forceinline__ float knn_sim(int32_t c, int32_t nj, int32_t ni, bool jaccard) {
  if (jaccard) return (float)c / ((float)(nj + ni - c) + 1e-6f);
  return (float)c / (sqrtf((float)nj) * sqrtf((float)ni) + 1e-6f);
}

__device__ __forceinline__ uint64_t knn_sort_key(uint32_t bits, int32_t id) { return ((uint64_t)(~bits) << 32) | (uint32_t)id; }

__device__ __forceinline__ void knn_emit(const KnnBuildParams& p, int32_t item, int r, bool live, uint64_t key) {
  const size_t at = (size_t)item * (size_t)p.knn + (size_t)r;
  p.nbr_id[at] = live ? (int32_t)(uint32_t)key : -1;
  p.nbr_sim[at] = live ? __uint_as_float(~(uint32_t)(key >> 32)) : 0.f;
}

__global__ __launch_bounds__(KNN_THREADS) void knn_build_kernel(const KnnBuildParams p) {
  extern __shared__ uint32_t knn_lds[];
  uint64_t* cand = reinterpret_cast<uint64_t*>(knn_lds);
  uint32_t* hist = knn_lds + KNN_CAND_WORDS;
  uint32_t* misc = hist + KNN_HIST_WORDS;
  uint32_t* cnt = misc + KNN_MISC_WORDS;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int64_t slot = (int64_t)blockIdx.x / p.n_tiles;
  const int32_t tl = (int32_t)((int64_t)blockIdx.x - slot * p.n_tiles);
  const int32_t i = p.order[slot];
  const int32_t lo = tl * p.tile;
  const int32_t span = (int32_t)((p.n_items - lo < p.tile) ? p.n_items - lo : p.tile);
  for (int x = t; x < span; x += KNN_THREADS) cnt[x] = 0u;
  cand[t] = ~0ull;                                  // sorts behind every key
  if (t < KNN_MISC_WORDS) misc[t] = 0u;
  __syncthreads();

  // ---- count
  const bool item_ok = (uint32_t)i < (uint64_t)p.n_items;
  const int64_t is = item_ok ? p.i_indptr[i] : 0, ie = item_ok ? p.i_indptr[i + 1] : 0;
  const int32_t ni = (int32_t)(ie - is);
  for (int64_t k = is + wave; k < ie; k += KNN_WAVES) {
    const int32_t u = p.i_users[k];
    if ((uint64_t)(uint32_t)u >= (uint64_t)p.n_users) continue;
    int64_t s = p.u_indptr[u];
    const int64_t e = p.u_indptr[u + 1];
    if (p.n_tiles > 1) s = knn_lower_bound(p.u_items, s, e, lo);
    for (int64_t q = s + lane; q < e; q += WAVE) {
      const uint32_t off = (uint32_t)(p.u_items[q] - lo);
      if (off >= (uint32_t)span) break;             // the row is sorted: past the tile
      atomicAdd(&cnt[off], 1u);
    }
  }
  __syncthreads();

  // ---- score
  int mine = 0;
  for (int x = t; x < span; x += KNN_THREADS) {
    const uint32_t c = cnt[x];
    const int32_t j = lo + x;
    uint32_t bits = 0u;
    if (c != 0u && j != i) {
      const int32_t nj = (int32_t)(p.i_indptr[j + 1] - p.i_indptr[j]);
      bits = __float_as_uint(knn_sim((int32_t)c, nj, ni, p.jaccard != 0));
      ++mine;
    }
    cnt[x] = bits;
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) mine += __shfl_xor(mine, m, 64);
  if (lane == 0 && mine) atomicAdd(&misc[MISC_NNZ], (uint32_t)mine);
  __syncthreads();
  const int nnz = (int)misc[MISC_NNZ];
  const int keep = nnz < p.knn ? nnz : p.knn;

  // ---- select: thr = the knn-th largest 48-bit key
  uint64_t thr = 0ull;
  if (nnz > p.knn) {
    uint32_t need = (uint32_t)p.knn;
    for (int pass = 0; pass < 6; ++pass) {
      const int shift = 40 - 8 * pass;
      for (int x = t; x < KNN_HIST_WORDS; x += KNN_THREADS) hist[x] = 0u;
      __syncthreads();
      for (int x = t; x < span; x += KNN_THREADS) {
        const uint32_t bits = cnt[x];
        if (bits == 0u) continue;
        const uint64_t key = ((uint64_t)bits << 16) | (uint64_t)(0xffffu - (uint32_t)x);
        if (pass == 0 || (key >> (shift + 8)) == thr) atomicAdd(&hist[wave * 256 + (int)((key >> shift) & 255u)], 1u);
      }
      __syncthreads();
      if (t < 256) {
        uint32_t sum = 0u;
        for (int w = 0; w < KNN_WAVES; ++w) sum += hist[w * 256 + t];
        hist[t] = sum;
      }
      __syncthreads();
      if (wave == 0) {                              // lane l holds the bins 255 - 4 l .. 252 - 4 l: a scan from the top digit down
        uint32_t v[4], tot = 0u;
#pragma unroll
        for (int q = 0; q < 4; ++q) v[q] = hist[255 - 4 * lane - q], tot += v[q];
        uint32_t incl = tot;
#pragma unroll
        for (int m = 1; m < 64; m <<= 1) {
          const uint32_t up = __shfl_up(incl, m, 64);
          if (lane >= m) incl += up;
        }
        uint32_t acc = incl - tot;
        if (acc < need && need <= incl) {
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            if (need <= acc + v[q]) {
              misc[MISC_DIGIT] = (uint32_t)(255 - 4 * lane - q);
              misc[MISC_NEED] = need - acc;
              break;
            }
            acc += v[q];
          }
        }
      }
      __syncthreads();
      thr = (thr << 8) | (uint64_t)misc[MISC_DIGIT];
      need = misc[MISC_NEED];
    }
  }

  // ---- gather and sort
  for (int x = t; x < span; x += KNN_THREADS) {
    const uint32_t bits = cnt[x];
    if (bits == 0u) continue;
    const uint64_t key = ((uint64_t)bits << 16) | (uint64_t)(0xffffu - (uint32_t)x);
    if (key >= thr) {
      const uint32_t at = atomicAdd(&misc[MISC_SLOT], 1u);
      if (at < (uint32_t)KNN_MAX_K) cand[at] = knn_sort_key(bits, lo + x);
    }
  }
  __syncthreads();
  int width = 1;
  while (width < keep) width <<= 1;
  for (int k2 = 2; k2 <= width; k2 <<= 1) {
    for (int j = k2 >> 1; j > 0; j >>= 1) {
      const int other = t ^ j;
      if (t < width && other > t) {
        const uint64_t a = cand[t], b = cand[other];
        if ((a > b) == ((t & k2) == 0)) cand[t] = b, cand[other] = a;
      }
      __syncthreads();
    }
  }

  // ---- emit
  if (!item_ok) return;
  if (p.n_tiles == 1) {
    if (t < p.knn) knn_emit(p, i, t, t < keep, cand[t]);
    if (t == 0) p.nbr_cnt[i] = keep;
  } else {
    const size_t list = (size_t)slot * (size_t)p.n_tiles + (size_t)tl;
    if (t < keep) p.ws_key[list * (size_t)p.knn + (size_t)t] = cand[t];
    if (t == 0) p.ws_cnt[list] = keep;
  }
}

// One workgroup per item of the order: the rank of a candidate among all of the item's candidates is its place in its own list
// plus the number of smaller keys in every other list; ranks below knn are the result.
__global__ __launch_bounds__(KNN_MERGE_THREADS) void knn_merge_kernel(const KnnBuildParams p) {
  const int64_t slot = blockIdx.x;
  const int32_t i = p.order[slot];
  if ((uint32_t)i >= (uint64_t)p.n_items) return;
  const int32_t* cnts = p.ws_cnt + (size_t)slot * (size_t)p.n_tiles;
  const uint64_t* keys = p.ws_key + (size_t)slot * (size_t)p.n_tiles * (size_t)p.knn;
  int64_t total = 0;
  for (int tl = 0; tl < p.n_tiles; ++tl) total += cnts[tl];
  const int keep = (int)(total < p.knn ? total : p.knn);
  const int64_t slots = (int64_t)p.n_tiles * p.knn;
  for (int64_t c = threadIdx.x; c < slots; c += KNN_MERGE_THREADS) {
    const int tl = (int)(c / p.knn), r = (int)(c - (int64_t)tl * p.knn);
    if (r >= cnts[tl]) continue;
    const uint64_t key = keys[c];
    int rank = r;
    for (int o = 0; o < p.n_tiles && rank < p.knn; ++o) {
      if (o == tl) continue;
      const uint64_t* other = keys + (size_t)o * (size_t)p.knn;
      int a = 0, b = cnts[o];
      while (a < b) {
        const int mid = (a + b) >> 1;
        if (other[mid] < key) a = mid + 1; else b = mid;
      }
      rank += a;
    }
    if (rank < p.knn) knn_emit(p, i, rank, true, key);
  }
  for (int r = keep + (int)threadIdx.x; r < p.knn; r += KNN_MERGE_THREADS) knn_emit(p, i, r, false, 0ull);
  if (threadIdx.x == 0) p.nbr_cnt[i] = keep;
}

struct KnnScoreParams {
  const int64_t *users, *u_indptr, *t_indptr;
  const int32_t *u_items, *t_items;
  const float* t_sim;
  int64_t n_users, n_items;
  int32_t tile, n_tiles;
  float* out;
};

__global__ __launch_bounds__(KNN_SCORE_THREADS) void knn_score_kernel(const KnnScoreParams p) {
  extern __shared__ float knn_acc[];
  const int t = threadIdx.x;
  const int64_t b = (int64_t)blockIdx.x / p.n_tiles;
  const int32_t tl = (int32_t)((int64_t)blockIdx.x - b * p.n_tiles);
  const int32_t lo = 1 + tl * p.tile;                                   // item 0 has no column
  const int32_t span = (int32_t)((p.n_items - lo < p.tile) ? p.n_items - lo : p.tile);
  for (int x = t; x < span; x += KNN_SCORE_THREADS) knn_acc[x] = 0.f;
  __syncthreads();
  const int64_t u = p.users[b];
  const bool ok = u >= 0 && u < p.n_users;
  const int64_t s = ok ? p.u_indptr[u] : 0, e = ok ? p.u_indptr[u + 1] : 0;
  int32_t j_next = s < e ? p.u_items[s] : -1;
  for (int64_t k = s; k < e; ++k) {                                     // ascending j: the order of every sum
    const int32_t j = j_next;
    if (k + 1 < e) j_next = p.u_items[k + 1];
    if ((uint64_t)(uint32_t)j >= (uint64_t)p.n_items) continue;         // uniform over the workgroup
    int64_t a = p.t_indptr[j];
    const int64_t z = p.t_indptr[j + 1];
    if (p.n_tiles > 1) a = knn_lower_bound(p.t_items, a, z, lo);
    for (int64_t q = a + t; q < z; q += KNN_SCORE_THREADS) {
      const uint32_t off = (uint32_t)(p.t_items[q] - lo);
      if (off >= (uint32_t)span) break;                                 // targets ascend: past the tile
      knn_acc[off] += p.t_sim[q];                                       // distinct targets within one j
    }
    __syncthreads();
  }
  float* row = p.out + (size_t)b * (size_t)(p.n_items - 1) + (size_t)(lo - 1);
  for (int x = t; x < span; x += KNN_SCORE_THREADS) row[x] = knn_acc[x];
}

static bool knn_tile_ok(int32_t tile) { return tile >= 1 && tile <= KNN_MAX_TILE && (tile & (tile - 1)) == 0; }

static bool knn_build_sizes_ok(int64_t n_items, int64_t n_order, int32_t knn, int32_t tile) {
  return n_items >= 1 && n_items < (1ll << 31) && n_order >= 0 && n_order <= n_items && knn >= 1 && knn <= KNN_MAX_K && knn_tile_ok(tile);
}

struct KnnLayout {
  uint64_t* key;
  int32_t* cnt;
};

static KnnLayout knn_layout(Carver& cv, int64_t n_order, int64_t n_tiles, int32_t knn) {
  KnnLayout y{};
  y.key = cv.take<uint64_t>(n_order * n_tiles * knn);
  y.cnt = cv.take<int32_t>(n_order * n_tiles);
  return y;
}

}  // namespace rsa

using namespace rsa;

extern "C" int64_t rsa_knn_build_workspace_bytes(int64_t n_items, int64_t n_order, int32_t knn, int32_t tile) {
  if (tile == 0) tile = KNN_MAX_TILE;
  if (!knn_build_sizes_ok(n_items, n_order, knn, tile)) return -1;
  const int64_t n_tiles = (n_items + tile - 1) / tile;
  if (n_tiles == 1) return 0;
  Carver cv(nullptr);
  knn_layout(cv, n_order, n_tiles, knn);
  return cv.bytes() + 256;
}

extern "C" int rsa_knn_build(const rsa_knn_build_args* args, rsa_stream_t stream) {
  const char* fn = "rsa_knn_build";
  rsa_knn_build_args a;
  if (int rc = load_args(a, args, fn)) return rc;
  if (a.tile == 0) a.tile = KNN_MAX_TILE;
  RSA_CHECK_ARG(a.knn >= 1 && a.knn <= KNN_MAX_K, "%s: knn = %d is outside 1 .. %d", fn, a.knn, KNN_MAX_K);
  RSA_CHECK_ARG(knn_tile_ok(a.tile), "%s: tile = %d is not a power of two up to %d", fn, a.tile, KNN_MAX_TILE);
  RSA_CHECK_ARG(a.similarity == RSA_KNN_COSINE || a.similarity == RSA_KNN_JACCARD, "%s: similarity = %d is unknown", fn, a.similarity);
  RSA_CHECK_ARG(knn_build_sizes_ok(a.n_items, a.n_order, a.knn, a.tile) && a.n_users >= 1 && a.n_users < (1ll << 31) && a.nnz >= 0,
                "%s: n_users = %lld, n_items = %lld, n_order = %lld, nnz = %lld out of range", fn, (long long)a.n_users,
                (long long)a.n_items, (long long)a.n_order, (long long)a.nnz);
  RSA_CHECK_ARG(a.max_degree >= 0 && a.max_degree < (1ll << 24), "%s: max_degree = %lld: an item row must stay below 2^24 users "
                "(counts are converted to fp32 exactly)", fn, (long long)a.max_degree);
  const int64_t n_tiles = (a.n_items + a.tile - 1) / a.tile;
  RSA_CHECK_ARG(a.n_order * n_tiles < (1ll << 31), "%s: n_order * tiles = %lld workgroups do not fit one launch: build in parts of "
                "the order", fn, (long long)(a.n_order * n_tiles));
  if (a.n_order == 0) return RSA_OK;
  RSA_CHECK_ARG(a.u_indptr != nullptr, "%s: u_indptr is null", fn);
  RSA_CHECK_ARG(a.i_indptr != nullptr, "%s: i_indptr is null", fn);
  RSA_CHECK_ARG(a.nnz == 0 || a.u_items != nullptr, "%s: u_items is null", fn);
  RSA_CHECK_ARG(a.nnz == 0 || a.i_users != nullptr, "%s: i_users is null", fn);
  RSA_CHECK_ARG(a.order != nullptr, "%s: order is null", fn);
  RSA_CHECK_ARG(a.nbr_id != nullptr, "%s: nbr_id is null", fn);
  RSA_CHECK_ARG(a.nbr_sim != nullptr, "%s: nbr_sim is null", fn);
  RSA_CHECK_ARG(a.nbr_cnt != nullptr, "%s: nbr_cnt is null", fn);
  KnnBuildParams p{};
  p.u_indptr = a.u_indptr, p.i_indptr = a.i_indptr, p.u_items = a.u_items, p.i_users = a.i_users, p.order = a.order;
  p.n_users = a.n_users, p.n_items = a.n_items, p.knn = a.knn, p.tile = a.tile, p.n_tiles = (int32_t)n_tiles;
  p.jaccard = a.similarity == RSA_KNN_JACCARD, p.nbr_id = a.nbr_id, p.nbr_sim = a.nbr_sim, p.nbr_cnt = a.nbr_cnt;
  if (n_tiles > 1) {
    RSA_CHECK_ARG(a.workspace != nullptr, "%s: workspace is null (the candidates of %lld tiles per item live in it)", fn, (long long)n_tiles);
    const int64_t need = rsa_knn_build_workspace_bytes(a.n_items, a.n_order, a.knn, a.tile);
    RSA_CHECK_ARG(a.workspace_bytes >= need, "%s: the workspace is too small: %lld bytes, need %lld", fn, (long long)a.workspace_bytes,
                  (long long)need);
    Carver cv(a.workspace);
    const KnnLayout y = knn_layout(cv, a.n_order, n_tiles, a.knn);
    p.ws_key = y.key, p.ws_cnt = y.cnt;
  }
  hipStream_t s = (hipStream_t)stream;
  const int32_t span = (int32_t)(a.n_items < a.tile ? a.n_items : a.tile);       // a short catalog asks for no more LDS than it uses
  const int64_t lds = (int64_t)(KNN_FIXED_WORDS + span) * 4;
  if (int rc = allow_lds<knn_build_kernel>(lds, fn)) return rc;
  hipLaunchKernelGGL(knn_build_kernel, dim3((unsigned)(a.n_order * n_tiles)), dim3(KNN_THREADS), (size_t)lds, s, p);
  RSA_CHECK_LAUNCH(fn);
  if (n_tiles > 1) {
    hipLaunchKernelGGL(knn_merge_kernel, dim3((unsigned)a.n_order), dim3(KNN_MERGE_THREADS), 0, s, p);
    RSA_CHECK_LAUNCH(fn);
  }
  return RSA_OK;
}

extern "C" int rsa_knn_score(const rsa_knn_score_args* args, rsa_stream_t stream) {
  const char* fn = "rsa_knn_score";
  rsa_knn_score_args a;
  if (int rc = load_args(a, args, fn)) return rc;
  if (a.tile == 0) a.tile = KNN_SCORE_TILE;
  RSA_CHECK_ARG(knn_tile_ok(a.tile), "%s: tile = %d is not a power of two up to %d", fn, a.tile, KNN_MAX_TILE);
  RSA_CHECK_ARG(a.n_batch >= 0 && a.n_users >= 1 && a.n_users < (1ll << 31) && a.n_items >= 1 && a.n_items < (1ll << 31),
                "%s: n_batch = %lld, n_users = %lld, n_items = %lld out of range", fn, (long long)a.n_batch, (long long)a.n_users,
                (long long)a.n_items);
  const int64_t n_tiles = (a.n_items - 1 + a.tile - 1) / a.tile;
  RSA_CHECK_ARG(a.n_batch * n_tiles < (1ll << 31), "%s: n_batch * tiles = %lld workgroups do not fit one launch", fn,
                (long long)(a.n_batch * n_tiles));
  if (a.n_batch == 0 || n_tiles == 0) return RSA_OK;
  RSA_CHECK_ARG(a.users != nullptr, "%s: users is null", fn);
  RSA_CHECK_ARG(a.u_indptr != nullptr, "%s: u_indptr is null", fn);
  RSA_CHECK_ARG(a.t_indptr != nullptr, "%s: t_indptr is null", fn);
  RSA_CHECK_ARG(a.out != nullptr, "%s: out is null", fn);
  KnnScoreParams p{};
  p.users = a.users, p.u_indptr = a.u_indptr, p.t_indptr = a.t_indptr, p.u_items = a.u_items, p.t_items = a.t_items, p.t_sim = a.t_sim;
  p.n_users = a.n_users, p.n_items = a.n_items, p.tile = a.tile, p.n_tiles = (int32_t)n_tiles, p.out = a.out;
  const int64_t span = a.n_items - 1 < a.tile ? a.n_items - 1 : a.tile;
  const int64_t lds = span * 4;
  if (int rc = allow_lds<knn_score_kernel>(lds, fn)) return rc;
  hipLaunchKernelGGL(knn_score_kernel, dim3((unsigned)(a.n_batch * n_tiles)), dim3(KNN_SCORE_THREADS), (size_t)lds, (hipStream_t)stream, p);
  RSA_CHECK_LAUNCH(fn);
  return RSA_OK;
}
