// Per-step sequence views of the contrastive sequence retrievers (gfx950): one launch draws one augmented view of a batch.
//
// rsa_seq_augment : Item_Crop / Item_Mask / Item_Reorder   recstudio/model/module/data_augmentation.py:22-87
//
// The reference loops over the batch in Python, with a .item() per sequence and three host generators.  Here the random choices
// of a view are the elements of ONE torch.rand([n_seq, seq_len + 1]) call on the device stream (U[b, 0] draws the start,
// U[b, 1 + p] is the key of position p), and everything is integer work but the one fp32 product of the start:
//
//   len   = clamp(seqlen[b], 0, seq_len)        n_sub = clamp(sub[len], 0, len)       (sub: the host's float64 length table)
//   span  = max(len - n_sub + 1, 1)             start = min((int)(U[b, 0] * (float)span), span - 1)
//   crop    : out[b, p] = p < n_sub ? seq[b, start + p] : 0                                               new_len = n_sub
//   mask    : out[b, p] = p < len && rank(p) < n_sub ? mask_id : seq[b, p]                                new_len = len
//             rank(p) = #{q < len : key_q < key_p || (key_q == key_p && q < p)}
//   reorder : out[b, start + rank(p)] = seq[b, p] for p in [start, start + n_sub), rank among that window the same way;
//             out[b, p] = seq[b, p] elsewhere                                                             new_len = len
//   a row with len == 0 is copied, new_len = 0.
//
// seq_len <= 64: one lane per position, one wave per sequence, four sequences per workgroup.  The ranks are 64 cross-lane reads
// of the keys (no LDS, no atomics, no workspace); every lane writes exactly one element of its row, so two runs are bit-equal.
// Nothing is read outside [0, seq_len) of a row: start + p <= len - 1 by construction of span, and n_sub is clamped to len.
#include "rsa_internal.hpp"

namespace rsa {

struct SeqAugParams {
  const int64_t* seq;
  int64_t seq_stride;
  const void* seqlen;
  const int32_t* sub;
  int64_t n_seq, mask_id;
  int32_t seq_len, kind, len_i32;
  PhiloxCall pc;
  int64_t* out;
  void* new_len;
};

__global__ __launch_bounds__(256) void seq_augment_kernel(const SeqAugParams p) {
  const int lane = lane_id();
  const int64_t b = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= p.n_seq) return;                                                   // whole waves leave: the shuffles below stay full
  const int L = p.seq_len;
  const int64_t raw = p.len_i32 ? (int64_t)((const int32_t*)p.seqlen)[b] : ((const int64_t*)p.seqlen)[b];
  const int len = (int)(raw < 0 ? 0 : (raw > L ? L : raw));
  int n_sub = p.sub[len];
  n_sub = n_sub < 0 ? 0 : (n_sub > len ? len : n_sub);
  const int64_t* row = p.seq + b * p.seq_stride;
  int64_t* orow = p.out + b * (int64_t)L;
  const bool have = lane < L;
  const int64_t mine = have ? row[lane] : 0;
  const uint64_t u_base = (uint64_t)b * (uint64_t)(L + 1);

  int start = 0;
  if (p.kind != RSA_SEQAUG_MASK) {
    const int span = len - n_sub + 1 > 1 ? len - n_sub + 1 : 1;
    float u0 = 0.f;
    if (lane == 0) u0 = torch_rand_element(p.pc, u_base);
    u0 = __shfl(u0, 0, 64);
    start = (int)(u0 * (float)span);                                          // the one fp32 product shared with the twin
    start = start > span - 1 ? span - 1 : start;
  }

  int new_len = len;
  if (len == 0) {
    if (have) orow[lane] = mine;
  } else if (p.kind == RSA_SEQAUG_CROP) {
    new_len = n_sub;
    if (have) orow[lane] = lane < n_sub ? row[start + lane] : 0;              // start + lane <= len - 1
  } else {
    const int lo = p.kind == RSA_SEQAUG_MASK ? 0 : start;
    const int hi = p.kind == RSA_SEQAUG_MASK ? len : start + n_sub;           // <= len
    const bool in_set = lane >= lo && lane < hi;
    const float key = in_set ? torch_rand_element(p.pc, u_base + 1 + (uint64_t)lane) : 0.f;
    int rank = 0;
    for (int q = lo; q < hi; ++q) {                                           // wave-uniform bounds
      const float kq = __shfl(key, q, 64);
      rank += (kq < key || (kq == key && q < lane)) ? 1 : 0;
    }
    if (have) {
      if (p.kind == RSA_SEQAUG_MASK)
        orow[lane] = (in_set && rank < n_sub) ? p.mask_id : mine;
      else
        orow[in_set ? start + rank : lane] = mine;                            // a permutation of [start, start + n_sub)
    }
  }
  if (lane == 0) {
    if (p.len_i32) ((int32_t*)p.new_len)[b] = new_len;
    else ((int64_t*)p.new_len)[b] = new_len;
  }
}

}  // namespace rsa

using namespace rsa;

extern "C" int rsa_seq_augment(const rsa_seq_augment_args* args, rsa_stream_t stream) {
  const char* fn = "rsa_seq_augment";
  rsa_seq_augment_args a;
  if (int rc = load_args(a, args, fn)) return rc;
  RSA_CHECK_ARG(a.n_seq >= 0, "%s: negative n_seq (%lld)", fn, (long long)a.n_seq);
  RSA_CHECK_ARG(a.seq_len >= 1 && a.seq_len <= RSA_SEQAUG_MAX_LEN, "%s: seq_len must lie in [1, %d], got %d", fn, RSA_SEQAUG_MAX_LEN,
                (int)a.seq_len);
  RSA_CHECK_ARG(a.kind == RSA_SEQAUG_CROP || a.kind == RSA_SEQAUG_MASK || a.kind == RSA_SEQAUG_REORDER,
                "%s: kind must be 0 (crop), 1 (mask) or 2 (reorder), got %d", fn, (int)a.kind);
  RSA_CHECK_ARG(a.seqlen_bytes == 4 || a.seqlen_bytes == 8, "%s: seqlen_bytes must be 4 or 8, got %d", fn, (int)a.seqlen_bytes);
  if (a.n_seq == 0) return RSA_OK;
  RSA_CHECK_ARG(a.seq != nullptr && a.seqlen != nullptr && a.sub != nullptr, "%s: seq/seqlen/sub is null", fn);
  RSA_CHECK_ARG(a.out != nullptr && a.new_len != nullptr, "%s: out/new_len is null", fn);
  RSA_CHECK_ARG(a.seq_stride >= a.seq_len, "%s: seq_stride (%lld) is below seq_len (%d)", fn, (long long)a.seq_stride, (int)a.seq_len);
  RSA_CHECK_ARG((const void*)a.out != (const void*)a.seq, "%s: out must not alias seq (reorder scatters)", fn);
  const int64_t blocks = (a.n_seq + 3) / 4;
  RSA_CHECK_ARG(blocks < (1ll << 31), "%s: too many sequences for one launch", fn);
  SeqAugParams p{};
  p.seq = a.seq, p.seq_stride = a.seq_stride, p.seqlen = a.seqlen, p.sub = a.sub;
  p.n_seq = a.n_seq, p.mask_id = a.mask_id, p.seq_len = a.seq_len, p.kind = a.kind, p.len_i32 = a.seqlen_bytes == 4;
  p.pc = PhiloxCall{a.seed, a.offset >> 2, a.grid_threads ? a.grid_threads : 1, a.elem_base};
  p.out = a.out, p.new_len = a.new_len;
  hipLaunchKernelGGL(seq_augment_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, p);
  RSA_CHECK_LAUNCH(fn);
  return RSA_OK;
}
