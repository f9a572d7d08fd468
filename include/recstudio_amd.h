/*
 * recstudio_amd -- C ABI of the MI355X (gfx950) retriever hot path.
 *
 * One shared library, librecstudio_amd.so, built from recstudio_amd/csrc/ by
 * hipcc --offload-arch=gfx950.  Plain pointers and sizes only: every pointer
 * is a DEVICE pointer unless stated otherwise, `stream` is a hipStream_t
 * passed as void*.  Every entry point returns 0 on success or a negative
 * rsa_status; rsa_last_error() returns the thread-local message of the last
 * failure.  No entry point synchronises or allocates: the few reductions that need device scratch (mean of the
 * row losses, valid-row count of the BCE losses, arrival counter + per-workgroup partials of the in-kernel loss
 * reduction) take a caller-owned block of rsa_scratch_bytes() bytes, zero-filled ONCE by the caller and then
 * left alone (the kernels restore the words they use); one block per device and stream -- calls sharing a block
 * must be stream-ordered.
 *
 * The reference (ustcml/RecStudio) is pure Python on PyTorch; it has no native
 * boundary of its own.  Each entry point below therefore replaces a SEQUENCE
 * of ATen ops in the reference, cited as file:line under /root/reference.
 * The Python binding a maintainer would add is in INTEGRATION.md; the binding
 * this repo ships is recstudio_amd/_native.py (ctypes).
 *
 * Index convention (same as the reference): tables are row-major fp32
 * [rows, dim]; row 0 is the padding row; ids are int64.
 */
#ifndef RECSTUDIO_AMD_H
#define RECSTUDIO_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RSA_ABI_VERSION 13  /* (added without a bump, as the later entry points were: rsa_fullscore_plan, read-only: the plan of rsa_fullscore's top-k and where its select leaves thr / flags / seg_cnt / ovf_cnt in the workspace);
                               13: rsa_scatter_rows_sorted_pairs_offset / rsa_bpr_sgd_pairs_offset / rsa_shard_backward_workspace_offsets (read-only: where the sorts leave their pairs, runs and flags inside the caller's workspaces);
                               12: rsa_rows_update_args.lr / beta1 / beta2 / eps are DOUBLES (the caller's own values: 1 - beta and the bias corrections are derived from them in double and rounded to fp32 once; as floats, 1 - float(0.999) was 1.29e-5 short of 0.001 on every touched row);
                               11: rsa_bpr_sgd_prepare / _apply sort the step's user rows WITH its item rows (one radix sort; item_workspace = rsa_scatter_rows_sorted_workspace_bytes(n_queries, num_neg + 1, n_items), user_workspace unused) and draw the negatives inside that sort's first launch; sampler RSA_SAMPLER_GIVEN accepted (neg_ids is an input);
                               10: rsa_fullscore_lse_grad (flash forward: logsumexp + d/d query in one pass); rsa_fullscore_softmax_dw (d/d items of the full softmax with the softmax tile recomputed on the matrix cores: no
                               [B, N] matrix anywhere in the backward); rsa_fullscore_softmax_dq: probs may be NULL (not written);
                               9: every entry point that took more than 12 positional arguments takes ONE argument block whose first field is its
                               own size (see "Versioned argument blocks"): rsa_popular_args (rsa_sample_popular, rsa_popular_lookup), rsa_loss_args
                               (rsa_pairwise_loss -- which now covers the kinds of the former rsa_pairwise_loss_ex --, rsa_ssm_shared_loss),
                               rsa_seg_gather_args, rsa_fullscore_args, rsa_rows_update_args (rsa_sort_step_elements, rsa_rows_update_sorted,
                               rsa_rows_update_presorted: the former rsa_scatter_rows_sorted / _presorted / rsa_adam_rows_sorted / _presorted);
                               rsa_bpr_sgd_prepare / rsa_bpr_sgd_apply (the whole in-place SGD step of a BPR two-tower model as two calls);
                               8: rsa_shard_owner_bpr_args.finish_parts / forward_parts (the owner-side step in parts, for a caller with two streams);
                               7: rsa_shard_pos_score / rsa_shard_owner_bpr_forward / _finish (the BPR step evaluated on the owners: rows read
                               once per step); rsa_shard_sample_route: route_pos; rsa_shard_backward_segments (the owner side of the sharded backward in one call: in-tree radix sorts
                               straight from the received segments, one walk over the query runs that reads every item row once and
                               updates solo rows in place, sorted apply for the shared rows); the sorted scatters no longer call rocPRIM;
                               6: rsa_adam_rows_presorted; rows_per_shard == 0 = interleaved row ownership in the shard routing entry points;
                               5: version 2 of the fixed-capacity shard exchange (rsa_shard_sample_route: sampling fused into the routing
                               pass, self-describing segments with {count, dropped} headers, 32-bit slots; rsa_shard_score_segments;
                               rsa_shard_home: scatter + loss + mean + routed-order gradient in one launch; rsa_shard_unpack_segments;
                               rsa_shard_scatter_slots); rsa_sample_masked_uniform takes elem_base;
                               4: rsa_fullscore_softmax_dq (d/d query of the full softmax on the matrix cores, in the
                               recompute pass); 3: caller-owned reduction scratch (rsa_scratch_bytes; the library allocates nothing);
                               Philox element base (G-invariant sampling across ranks); bucket-line inverse CDF
                               (cdf_lines); SampledSoftmax epilogue (fused_loss = 2); cosine / Euclidean full-catalog
                               scores (rsa_row_sqnorm, rsa_fullscore score_mode); fixed-capacity shard routing
                               (rsa_shard_route_fixed, negative keys / positions = empty slot).
                               2: rsa_fused_args grew query_grad, packed_keys, offset_dev; new entry points
                               (rsa_row_topk, rsa_fullscore_softmax, rsa_pairwise_loss_ex, rsa_scatter_rows_sorted,
                               rsa_rng_advance) */

typedef void* rsa_stream_t; /* hipStream_t */

enum rsa_status {
  RSA_OK = 0,
  RSA_ERR_ARG = -1,         /* bad argument (null pointer, size, unsupported dim) */
  RSA_ERR_HIP = -2,         /* a HIP runtime call / kernel launch failed */
  RSA_ERR_UNSUPPORTED = -3  /* valid request this build does not implement */
};

enum rsa_score_mode { RSA_SCORE_IP = 0, RSA_SCORE_COS = 1, RSA_SCORE_EUC = 2 /* EuclideanScorer, scorer.py:28-34 */ };
enum rsa_sampler_kind { RSA_SAMPLER_GIVEN = 0, RSA_SAMPLER_UNIFORM = 1, RSA_SAMPLER_POPULAR = 2 };
enum rsa_loss_kind { RSA_LOSS_BPR = 0, RSA_LOSS_SSM = 1, RSA_LOSS_BCE = 2,
                     /* rsa_pairwise_loss: */ RSA_LOSS_WBPR = 3, RSA_LOSS_WBCE = 4, RSA_LOSS_HINGE = 5, RSA_LOSS_NCE = 6,
                     RSA_LOSS_CCL = 7 };

/* ---- Versioned argument blocks (ABI 9) --------------------------------------------------------------------------
 * The structs below whose FIRST field is `int64_t size` are read as follows: the caller sets size = sizeof(the struct)
 * as ITS header declares it; the library copies min(size, its own sizeof) bytes into a zero-filled block of its own.  Fields
 * are only ever appended, and 0 / NULL always means "not given": a caller compiled against an older header keeps working
 * against a newer library (the new fields read as 0), and a newer caller against an older library has its extra fields
 * ignored.  rsa_fused_args / rsa_backward_args / the rsa_shard_* blocks predate this and are covered by RSA_ABI_VERSION. */

const char* rsa_last_error(void);
int rsa_abi_version(void);
/* Size of the caller-owned reduction scratch (see above). */
int64_t rsa_scratch_bytes(void);

/* Device properties torch's distribution kernels size their grid from
 * (multiProcessorCount, maxThreadsPerMultiProcessor) -- needed to reproduce
 * the device random stream.  Host pointers. */
int rsa_device_info(int device, int32_t* cu_count, int32_t* max_threads_per_cu, int32_t* wave_size);

/* ---- Philox state ---------------------------------------------------------
 * (seed, offset) are the torch CUDA/HIP generator's philox seed and offset at
 * the moment the reference would have called torch.randint / torch.rand;
 * grid_threads is the thread count of torch's distribution grid for `numel`
 * outputs (256 * min(CUs * maxThreadsPerCU/256, ceil(numel/256))).  With
 * these, element i of the output is bit-identical to element i of
 * torch.randint(low, high, (numel,), device='cuda') / torch.rand(numel).
 * elem_base: output element i draws what element elem_base + i of the torch call would -- a rank that owns
 * rows [r*B, (r+1)*B) of a global [G*B, n] id tensor passes elem_base = r*B*n and the grid_threads of the GLOBAL
 * call, so that the negatives of a run do not depend on the number of GPUs; 0 otherwise. */

/* UniformSampler.forward -- recstudio/ann/sampler.py:86-111
 * (torch.randint(1, num_items+1, (num_queries, num_neg)), :102-104).
 * neg_ids[numel] <- low + philox % (high - low). */
int rsa_sample_uniform(int64_t* neg_ids, int64_t numel, int64_t low, int64_t high,
                       uint64_t seed, uint64_t offset, uint32_t grid_threads, uint64_t elem_base, rsa_stream_t stream);

/* MaskedUniformSampler.forward / uniform_sample_masked_hist -- recstudio/ann/sampler.py:117-147, :187-214:
 * rejection-free uniform negatives over the items NOT in each user's 0-padded history
 * user_hist [n_rows, hist_len] (hist_len <= 2048).  num_items excludes the padding id.  neg_ids
 * [n_rows, per_row] (per_row = queries-per-user x num_neg); u = torch.rand(n_rows, per_row) on the
 * device stream (elem_base as in "Philox state": a rank's rows of one job-wide call). */
int rsa_sample_masked_uniform(const int64_t* user_hist, int64_t n_rows, int32_t hist_len, int64_t num_items,
                              int32_t per_row, int64_t* neg_ids, uint64_t seed, uint64_t offset,
                              uint32_t grid_threads, uint64_t elem_base, rsa_stream_t stream);

/* PopularSamplerModel.forward -- recstudio/ann/sampler.py:243-258
 * (u = torch.rand; ids = torch.searchsorted(table, u); logp = log(pop_prob[ids])).
 * table/pop_prob: fp32 [n_items] exactly as the reference's registered buffers
 * (:239-241).  guide: int32 [2^guide_log2 + 1], guide[j] = first index with
 * table[i] >= j / 2^guide_log2, guide[2^guide_log2] = n_items (cut-point
 * acceleration, guide_log2 <= 28; returns the same index searchsorted does).  An id that would be
 * n_items (u above table[-1]) is clamped to n_items-1.  neg_logp / u_out may be
 * null.  cdf_lut / cdf_lines (nullable, see rsa_fused_args) are faster forms of the same lookup; with
 * cdf_lines the guide may be null. */
typedef struct rsa_popular_args {
  int64_t size;                /* sizeof(rsa_popular_args) */
  const float* table;          /* [n_items] CDF */
  const float* pop_prob;       /* [n_items] */
  const int32_t* guide;        /* nullable with cdf_lines */
  int64_t n_items;
  int32_t guide_log2;
  int32_t lines_log2;
  const float* cdf_lut;        /* nullable */
  const float* cdf_lines;      /* nullable */
  const float* u_in;           /* rsa_popular_lookup: the uniforms [numel]; ignored by rsa_sample_popular */
  int64_t* ids;                /* [numel] out */
  float* logp;                 /* nullable [numel] out */
  float* u_out;                /* nullable [numel] out (rsa_sample_popular: the uniforms drawn) */
  int64_t numel;
  uint64_t seed, offset;       /* "Philox state" (rsa_sample_popular) */
  uint32_t grid_threads;
  uint32_t _pad;
  uint64_t elem_base;
} rsa_popular_args;
int rsa_sample_popular(const rsa_popular_args* args, rsa_stream_t stream);

/* The same inverse-CDF lookup for caller-supplied uniforms u_in[numel] (used by the
 * parity tests to hit exact table edges). */
int rsa_popular_lookup(const rsa_popular_args* args, rsa_stream_t stream);

/* MIDXSamplerUniform / ClusterSamplerUniform .forward and .compute_item_p -- recstudio/ann/sampler.py:308-388, :460-510:
 * negatives from a proposal that follows the query through a k-means codebook.  n_parts = 2 (MIDX): the query's two halves
 * q0, q1 against centres[0], centres[1]; P(k0, k1) ~ wkk[k0][k1] * exp(<q0, c0[k0]>) * exp(<q1, c1[k1]>), k0 from its marginal,
 * k1 from the conditional, then an item uniform in bucket k0 * K + k1.  n_parts = 1 (Cluster): P(k) ~ wkk[k] * exp(<q, c[k]>).
 * RSA_SCORE_COS: the query is divided by max(||q||, 1e-12) first.  neg_logp = the (unnormalised) logits of the chosen clusters,
 * pos_logp[q][t] = the logits of the clusters of pos_ids[q][t] (0 for the padding id).  An empty bucket (wkk == 0) is never
 * returned; the exact draw and tie rule: recstudio_amd/csrc/rsa_midx.hip.  Uniforms: element ((q * num_neg + j) * (n_parts + 1)
 * + t) of ONE torch.rand(n_queries, num_neg, n_parts + 1) on the device stream ("Philox state").  num_neg = 0 with n_pos > 0 is
 * compute_item_p on its own.  Limits: dim % 8 == 0, dim <= 256, 2 <= n_clusters <= 64. */
typedef struct rsa_midx_args {
  int64_t size;                /* sizeof(rsa_midx_args) */
  const float* query;          /* [n_queries, dim] */
  int64_t n_queries;
  int32_t dim;
  int32_t n_parts;             /* 2: MIDX, 1: Cluster */
  int32_t n_clusters;          /* K */
  int32_t score_mode;          /* RSA_SCORE_IP or RSA_SCORE_COS */
  const float* centres;        /* [n_parts, K, dim / n_parts] */
  const float* wkk;            /* [K, K] (MIDX) or [K] (Cluster): items per bucket */
  const int32_t* indptr;       /* [K^n_parts + 1] bucket b holds indices[indptr[b] .. indptr[b + 1]) */
  const int32_t* indices;      /* [n_items] item ids - 1, grouped by bucket */
  int64_t n_items;             /* items WITHOUT the padding id */
  const int32_t* cd0;          /* [n_items + 1] cluster + 1 of every id in part 0, 0 for the padding id */
  const int32_t* cd1;          /* the same for part 1 (MIDX) */
  int32_t num_neg;
  int32_t n_pos;               /* positives per query (0: none) */
  const int64_t* pos_ids;      /* nullable [n_queries, n_pos] */
  const float* u_in;           /* rsa_midx_lookup: the uniforms [n_queries, num_neg, n_parts + 1] */
  int64_t* neg_ids;            /* [n_queries, num_neg] out */
  float* neg_logp;             /* nullable [n_queries, num_neg] out */
  float* pos_logp;             /* [n_queries, n_pos] out */
  float* u_out;                /* nullable out (rsa_midx_sample: the uniforms drawn) */
  uint64_t seed, offset;       /* "Philox state" (rsa_midx_sample) */
  uint32_t grid_threads;
  uint32_t _pad;
  uint64_t elem_base;
  /* Popularity-in-bucket form (MIDXSamplerPop / ClusterSamplerPop; tables of rsa_midx_weights).  Both null: the item is uniform in
   * its bucket, as above.  Both set: inside bucket [start, end) the item sits at the FIRST position with cp[pos] > u2 (the last
   * position whose cp exceeds its predecessor's when rounding leaves none), and item_logp[id] is added to neg_logp and pos_logp. */
  const float* cp;             /* nullable [n_items] in-bucket CDF by sorted position */
  const float* item_logp;      /* nullable [n_items + 1] log of the in-bucket weight of every id, 0 for the padding id */
} rsa_midx_args;
int rsa_midx_sample(const rsa_midx_args* args, rsa_stream_t stream);
/* The same draw for caller-supplied uniforms (the tests hit exact CDF edges with it). */
int rsa_midx_lookup(const rsa_midx_args* args, rsa_stream_t stream);

/* The per-epoch tables of MIDXSamplerPop / ClusterSamplerPop._update -- recstudio/ann/sampler.py:407-423, :545-559 -- from the
 * index of the last update.  Item i (id i + 1) weighs w = pop[i], times exp(-||row i||^2 / 2) when `table` is given (the
 * Euclidean scorer; norm and exp in double, the product rounded to fp32 once).  p = [1, w...], item_logp = fl(log((double)p)),
 * wkk[b] = the sum of w over bucket b and cp[pos] = prefix(pos) / wkk[b] inside each bucket, both accumulated in double in the
 * order of `indices` and rounded once; a bucket of weight 0 gets wkk = 0 and cp = 0 throughout.  The summation order depends on
 * the bucket layout alone: two runs are bit-equal.  Same limits as rsa_midx_args. */
typedef struct rsa_midx_weights_args {
  int64_t size;                /* sizeof(rsa_midx_weights_args) */
  const float* pop;            /* [n_items] popularity weight of ids 1 .. n_items */
  const float* table;          /* nullable: rows [row_offset, row_offset + n_items) give the Euclidean factor */
  int64_t n_items;             /* items WITHOUT the padding id */
  int64_t row_stride;          /* floats, a multiple of 4 */
  int64_t row_offset;
  int32_t dim;
  int32_t n_parts;
  int32_t n_clusters;
  int32_t _pad;
  const int32_t* indptr;       /* [K^n_parts + 1] */
  const int32_t* indices;      /* [n_items] */
  float* p;                    /* [n_items + 1] out */
  float* item_logp;            /* [n_items + 1] out */
  float* wkk;                  /* [K^n_parts] out */
  float* cp;                   /* [n_items] out */
} rsa_midx_weights_args;
int rsa_midx_weights(const rsa_midx_weights_args* args, rsa_stream_t stream);

/* One assignment pass of kmeans() -- recstudio/ann/sampler.py:19-31 -- over rows [row_offset, row_offset + n_rows) of `table`
 * (row_stride floats apart), for n_parts column groups at once; every row is read once.  normalize: rows are divided by
 * max(||row||, 1e-12) (whole row) first.  Per part: assign[part][row] = argmin_k ||x - c[k]||^2 (lowest k on a tie),
 * sums[part][k] = sum of the rows assigned to k, counts[part][k], loss[part] = sum of the minimal squared distances.  No
 * [n_rows, K] matrix and no float atomics: results are bit-equal run to run.  Same limits as rsa_midx_args. */
typedef struct rsa_kmeans_args {
  int64_t size;                /* sizeof(rsa_kmeans_args) */
  const float* table;
  int64_t n_rows;
  int64_t row_stride;          /* floats, a multiple of 4 */
  int64_t row_offset;          /* first row (1 for an embedding table whose row 0 is the padding row) */
  int32_t dim;
  int32_t n_parts;
  int32_t n_clusters;
  int32_t normalize;
  const float* centres;        /* [n_parts, K, dim / n_parts] */
  int32_t* assign;             /* [n_parts, n_rows] out */
  float* sums;                 /* [n_parts, K, dim / n_parts] out */
  int32_t* counts;             /* [n_parts, K] out */
  double* loss;                /* [n_parts] out */
  void* workspace;
  int64_t workspace_bytes;     /* >= rsa_kmeans_workspace_bytes(n_rows, dim, n_clusters) */
} rsa_kmeans_args;
int64_t rsa_kmeans_workspace_bytes(int64_t n_rows, int32_t dim, int32_t n_clusters);
int rsa_kmeans_step(const rsa_kmeans_args* args, rsa_stream_t stream);

/* LSHSampler.update, the hash -- recstudio/ann/sampler.py:600-604 -- over rows [row_offset, row_offset + n_rows) of `table`
 * (row_stride floats apart); every row is read once.  Bit (k, l) of a row x is <x, W[:, k, l]> > 0 (strict; the reference
 * normalises x first, which does not move the sign), codes[l][row] = sum_k bit(k, l) * 2^(n_bits - 1 - k).  The dot product's
 * summation order: recstudio_amd/csrc/rsa_lsh.hip.  No atomics and no accumulation across rows: two runs are bit-equal.
 * Limits: dim % 8 == 0, dim <= 256, 1 <= n_bits <= 16, n_bits * n_table <= 64 (one lane of a wave per projection). */
typedef struct rsa_lsh_hash_args {
  int64_t size;                /* sizeof(rsa_lsh_hash_args) */
  const float* table;
  int64_t n_rows;
  int64_t row_stride;          /* floats, a multiple of 4 */
  int64_t row_offset;          /* first row (1 for an embedding table whose row 0 is the padding row) */
  int32_t dim;
  int32_t n_bits;              /* K */
  int32_t n_table;             /* L */
  int32_t _pad;
  const float* weight_vectors; /* [dim, n_bits, n_table], LSHSampler.weight_vectors */
  int32_t* codes;              /* [n_table, n_rows] out */
} rsa_lsh_hash_args;
int rsa_lsh_hash(const rsa_lsh_hash_args* args, rsa_stream_t stream);

/* LSHSampler.forward -- recstudio/ann/sampler.py:609-677: negatives from the union (with multiplicity) of the query's buckets
 * in the n_table hash tables.  The query is hashed as above; cnt_l = size of its bucket in table l, cum = inclusive prefix of
 * cnt over l, len = cum[n_table - 1] (64 bits).  Draw j of query q with its uniform u:
 *   r = floor(fl32(u * fl32(len))) (ONE fp32 multiply), clamped to len - 1;  t = #{l : cum_l <= r} (an empty table is never
 *   chosen);  item = indices[t][indptr[t][code_t] + r - cum_{t-1}];  neg_ids = item + 1.
 *   c = cos(query, item_embs[item]) clamped to [-1, 1] (0 when either norm is 0), p = 1 - acos(c) / pi,
 *   w = 1 - (1 - p^K)^L evaluated as -expm1(L * log1p(-p^K)) in double,  neg_logp = fl32(log(w / len + log_eps)).
 * A query with len == 0: neg_ids = 1 + min(floor(fl32(u * fl32(n_items))), n_items - 1), neg_logp = 0.
 * Uniforms: element q * num_neg + j of ONE torch.rand(n_queries, num_neg) on the device stream ("Philox state").
 * Same limits as rsa_lsh_hash_args; n_items < 2^31 - 1. */
typedef struct rsa_lsh_args {
  int64_t size;                /* sizeof(rsa_lsh_args) */
  const float* query;          /* [n_queries, dim] */
  int64_t n_queries;
  int32_t dim;
  int32_t n_bits;              /* K */
  int32_t n_table;             /* L */
  int32_t num_neg;
  const float* weight_vectors; /* [dim, n_bits, n_table] */
  const int32_t* indptr;       /* [n_table, 2^n_bits + 1] bucket b of table l holds indices[l][indptr[l][b] .. indptr[l][b + 1]) */
  const int32_t* indices;      /* [n_table, n_items] item ids - 1, grouped by bucket */
  const float* item_embs;      /* [n_items, dim] the rows the index was built from (the snapshot of update) */
  int64_t n_items;             /* items WITHOUT the padding id */
  const float* u_in;           /* rsa_lsh_lookup: the uniforms [n_queries, num_neg] */
  int64_t* neg_ids;            /* [n_queries, num_neg] out */
  float* neg_logp;             /* [n_queries, num_neg] out */
  int32_t* codes_out;          /* nullable [n_queries, n_table] out: the query's codes */
  float* u_out;                /* nullable out (rsa_lsh_sample: the uniforms drawn) */
  double log_eps;              /* added inside the log: 1e-12 with pos_items in the reference, 0 without */
  uint64_t seed, offset;       /* "Philox state" (rsa_lsh_sample) */
  uint32_t grid_threads;
  uint32_t _pad;
  uint64_t elem_base;
} rsa_lsh_args;
int rsa_lsh_sample(const rsa_lsh_args* args, rsa_stream_t stream);
/* The same draw for caller-supplied uniforms (the tests hit every table boundary with it). */
int rsa_lsh_lookup(const rsa_lsh_args* args, rsa_stream_t stream);

/* PopularSamplerModel.compute_item_p -- recstudio/ann/sampler.py:257-258:
 * logp[i] = log(pop_prob[ids[i]]). */
int rsa_item_logp(const float* pop_prob, int64_t n_items, const int64_t* ids, int64_t numel,
                  float* logp, rsa_stream_t stream);

/* torch.nn.Embedding forward (F.embedding) -- baseretriever.py:153-154, :167-168,
 * :211, seq/sasrec.py:42.  out[numel, dim] <- table[ids]. */
int rsa_embedding_gather(const float* table, int64_t n_rows, int32_t dim, const int64_t* ids,
                         int64_t numel, float* out, rsa_stream_t stream);

/* Fused BaseRetriever.forward body for an Embedding item tower --
 * recstudio/model/basemodel/baseretriever.py:153-171 : sampler (S1/S2 above, or
 * ids given) -> item_encoder(neg ids) -> score_func(query, pos) and
 * score_func(query, neg) (recstudio/model/scorer.py:5-25), without materialising
 * the [M, n, dim] negative rows.
 *
 * M "queries" (B, or B*L for sequence targets), n negatives each.  Flat element
 * e = m*n + j is element e of the reference's [M, n] id tensor, so sampled ids
 * are bit-identical to the reference's device stream. */
typedef struct rsa_fused_args {
  const float* item_table;     /* [n_items, dim] */
  int64_t n_items;
  int32_t dim;                 /* multiple of 4, <= 1024 */
  int32_t score_mode;          /* rsa_score_mode */
  const float* query;          /* [n_query_rows, dim]: query vectors, or a user table */
  const int64_t* query_index;  /* nullable [M]: row of `query` for query m (user-id gather,
                                  baseretriever.py:211); null => row m */
  int64_t n_query_rows;
  const int64_t* pos_ids;      /* nullable [M] */
  int64_t n_queries;           /* M */
  int32_t num_neg;             /* n */
  int32_t sampler;             /* rsa_sampler_kind */
  int32_t mask_pad_pos;        /* !=0: pos_score = -inf where pos_ids == 0 (baseretriever.py:164-165) */
  int32_t guide_log2;
  uint64_t seed, offset;       /* philox state (sampler != GIVEN) */
  uint32_t grid_threads;
  uint32_t _pad;
  const float* table;          /* POPULAR: cdf / pop_prob / guide as in rsa_sample_popular */
  const float* pop_prob;
  const int32_t* guide;
  int64_t* neg_ids;            /* [M, n]: INPUT if sampler == GIVEN, else OUTPUT */
  float* neg_logp;             /* nullable [M, n] out (POPULAR); INPUT log-probabilities when sampler == GIVEN and
                                  fused_loss == 2 (null = 0) */
  float* pos_logp;             /* nullable [M] out (POPULAR, needs pos_ids); INPUT like neg_logp for GIVEN + fused_loss 2 */
  float* pos_score;            /* nullable [M] out (needs pos_ids) */
  float* neg_score;            /* [M, n] out; nullable with fused_loss != 0 (a training forward that keeps no scores: 4 B/triplet less) */
  const float* table_prob;     /* nullable [n_items][2]: interleaved copy {table[i], pop_prob[i]}.  When given,
                                  the CDF probes and the log-prob read share cache lines (one Infinity-Cache
                                  round trip fewer per sampled id); results are identical. */
  int32_t fused_loss;          /* 0 = none; 1 = BPRLoss (loss_func.py:55-59); 2 = SampledSoftmaxLoss (loss_func.py:80-90,
                                  one positive per row; logsumexp over the positive and all num_neg negatives of a query
                                  carried across its num_neg/64 tiles by ONE wave; inner product, dim in {32,64,128,256};
                                  a -inf positive yields NaN like the reference).  Evaluated in the kernel's epilogue:
                                  needs num_neg % 64 == 0, pos_ids, pos_score.  Outputs below. */
  int32_t _pad2;
  float* row_loss;             /* [M] out: per-query loss */
  float* loss_out;             /* nullable [1] out: mean over queries, reduced in the same launch by the last workgroup
                                  to finish (fixed summation order: reproducible run to run) */
  float* dpos;                 /* nullable [M] out: d loss_out / d pos_score */
  float* dneg;                 /* nullable [M, n] out: d loss_out / d neg_score */
  const float* cdf_lut;        /* nullable [2^guide_log2 + 1][4] fp32, one self-contained entry per guide bucket b with
                                  lo = guide[b], hi = guide[b+1]: {lo as int32 bits, bit 31 set when hi - lo >= 2;
                                  table[lo] (+inf when hi == lo); pop_prob[min(lo, n_items-1)];
                                  pop_prob[min(lo+1, n_items-1)]}.  Direct-lookup form of the inverse CDF: one 16-byte
                                  read resolves id and probability for every bucket holding <= 1 CDF boundary
                                  (one HBM line instead of three dependent round trips); identical results. */
  float* query_grad;           /* nullable [M, dim] out, fused_loss != 0 only (inner product, dim in {32,64,128,256}):
                                  d loss_out / d query row m = sum_j dneg[m,j] * item[neg_ids[m,j]] + dpos[m] * item[pos],
                                  accumulated while the rows are in registers, so that rsa_fused_backward can be
                                  called without query_grad / query_table_grad and then never reads an item row. */
  const int64_t* packed_keys;  /* nullable [M]: sampler GIVEN, num_neg == 1, no positives: element m scores query row
                                  (key >> 32) against item row (key & 0xffffffff) -- the owner side of the sharded
                                  exchange (rsa_shard_route keys) without unpacking; neg_ids / query_index unused.
                                  A negative key is an empty slot: its score is 0. */
  const uint64_t* offset_dev;  /* nullable device word: when set, the Philox offset is read from it at run time instead
                                  of `offset` (a multiple of 4, like torch's) -- lets a captured HIP graph draw fresh
                                  numbers on every replay; advance it with rsa_rng_advance in the same graph. */
  uint64_t elem_base;          /* Philox element index of flat element 0 (see "Philox state"); 0 on one GPU */
  void* reduce_scratch;        /* loss_out != null: caller-owned scratch of rsa_scratch_bytes() bytes (zeroed once) */
  const float* cdf_lines;      /* nullable [2^lines_log2 + 1][32] fp32 (128-byte aligned): BUCKET LINES, the one-HBM-line form
                                  of the inverse CDF.  Line b describes u in [b, b+1) / 2^lines_log2 through the DISTINCT
                                  CDF values inside it (items whose CDF equals their predecessor's can never be returned
                                  by searchsorted and are left out), 12 slots:
                                    words 0..11   cdf of the bucket's first distinct values, then (if fewer than 12) of the
                                                  first distinct entry ABOVE the bucket, then +inf
                                    words 12..23  pop_prob of those entries
                                    words 24..29  their ids as uint16 offsets from `base` (even slot in the low half)
                                    word  30      base id (int32 bits);  word 31: number of distinct values in the bucket
                                                  (int32; -1 = ids too far apart for 16-bit offsets)
                                  id = base + delta[#{cdf[i] < u}] -- the same comparisons torch.searchsorted makes; a
                                  draw above 12 in-bucket values (or a -1 line) is searched in `table` between this
                                  line's and the next line's base (line 2^lines_log2 is a sentinel).  Takes precedence
                                  over cdf_lut / guide. */
  int32_t lines_log2;
  int32_t _pad3;
  /* In-forward SGD (fused_loss = 1, num_neg == 64, ids GIVEN, query_grad given; ABI v5).  solo_flags: the classification
   * of the step's elements by rsa_sort_step_elements (element order m * (num_neg + 1) + c, c = 0 the positive: 1 <=> no
   * other element of the step touches that item row, and the row is not the padding row).  Such a row is rewritten by
   * the wave that has it in registers: item[id] += upd_scale[0] * d * q (d = d loss/d score of that element; upd_scale =
   * -lr is plain SGD) -- nothing else reads or writes that row in the step, so the result is the one a separate update
   * pass gives.  The other elements are applied by rsa_rows_update_presorted on the same workspace, which skips
   * exactly the flagged ones.  item_table is written. */
  const uint8_t* solo_flags;   /* nullable [M * (num_neg + 1)] */
  const float* upd_scale;      /* device scalar */
  /* A QUEUE of independent batches consumed by one resident grid (ABI 9; forward-only scoring / loss evaluation of many
   * batches: a small batch's launch is a sampling phase followed by a row phase, and in a stream of such launches the
   * first has nothing to hide under -- inside ONE grid the waves of different batches are out of phase, so one batch's
   * draw -> bucket line -> slot chain runs under another's row reads).  n_batches > 1: the n_queries queries are n_batches
   * consecutive batches of n_queries / n_batches; batch k's negatives are those of ITS OWN torch call -- (seed, offset +
   * k * batch_offset_step, grid_threads of ONE batch's numel) -- i.e. exactly what n_batches consecutive launches draw.
   * In-kernel samplers, num_neg % 64 == 0, loss_out null (row_loss holds every query's loss; the per-batch means are the
   * caller's), the BPR epilogue with num_neg == 64. */
  int32_t n_batches;           /* 0 / 1: one batch */
  int32_t _pad4;
  uint64_t batch_offset_step;  /* Philox offset consumed by one batch's torch call (multiple of 4) */
} rsa_fused_args;

int rsa_fused_sample_gather_score(const rsa_fused_args* args, rsa_stream_t stream);

/* *offset_dev += increment (one thread).  Together with rsa_fused_args.offset_dev this keeps the device copy of the
 * torch generator offset moving inside a captured graph; `increment` is what torch's distribution call would
 * consume ((numel-1)/(grid_threads*unroll)+1)*4, see "Philox state"). */
int rsa_rng_advance(uint64_t* offset_dev, uint64_t increment, rsa_stream_t stream);

/* BPRLoss.forward (recstudio/model/loss_func.py:55-59) / SampledSoftmaxLoss.forward
 * (:80-90) / BinaryCrossEntropyLoss.forward (:105-127, dns=False) on pos_score [M], neg_score [M, n] (each positive with its own n
 * negatives), value AND gradient in one pass.  pos_logp / neg_logp are nullable
 * (treated as 0; the reference's UniformSampler hands int64 zeros).  loss_out[1]
 * = mean over rows; row_loss [M] scratch/out; dpos [M] and dneg [M, n] (nullable)
 * = d loss_out / d score. */
typedef struct rsa_loss_args {
  int64_t size;                /* sizeof(rsa_loss_args) */
  int32_t loss_kind;           /* rsa_loss_kind */
  int32_t n_pos;               /* rsa_ssm_shared_loss: positives per row (L); ignored by rsa_pairwise_loss */
  const float* pos_score;      /* [n_rows] ([n_rows, n_pos] for rsa_ssm_shared_loss) */
  const float* neg_score;      /* [n_rows, num_neg] */
  const float* pos_logp;       /* nullable, like pos_score */
  const float* neg_logp;       /* nullable, like neg_score */
  int64_t n_rows;
  int32_t num_neg;
  int32_t _pad;
  float param0, param1;        /* RSA_LOSS_HINGE: margin; RSA_LOSS_CCL: margin, neg_weight */
  float* row_loss;             /* [n_rows] scratch / out */
  float* loss_out;             /* [1] out: the mean over rows */
  float* dpos;                 /* nullable out, like pos_score */
  float* dneg;                 /* nullable out, like neg_score */
  void* scratch;               /* rsa_scratch_bytes() */
} rsa_loss_args;
int rsa_pairwise_loss(const rsa_loss_args* args, rsa_stream_t stream);

/* loss_kind >= RSA_LOSS_WBPR -- the other PairwiseLoss classes of recstudio/model/loss_func.py, value + d loss/d score in
 * one pass:  RSA_LOSS_WBPR WeightedBPRLoss (:93-97; the softmax(neg - logQ) weights are differentiated
 * through, as in the reference), RSA_LOSS_WBCE WeightedBinaryCrossEntropyLoss (:135-137 on :105-127, padded -inf
 * positives dropped), RSA_LOSS_HINGE HingeLoss (:140-154, num_items=None; param0 = margin), RSA_LOSS_NCE NCELoss
 * (:163-168), RSA_LOSS_CCL CCLLoss (:171-186; param0 = margin, param1 = neg_weight).  InfoNCELoss (:157-160) is
 * RSA_LOSS_SSM with null log-probabilities.  Top1Loss (:66-78) is not offered: the reference's
 * forward modifies a sigmoid output in place and cannot be back-propagated.
 *
 * rsa_ssm_shared_loss: SampledSoftmaxLoss.forward when pos_score [B, L] and neg_score [B, n] have the SAME rank
 * (recstudio/model/loss_func.py:84-89): the L = n_pos positives of a row share its n negatives; padded
 * positives (+-inf) contribute nothing and are not counted.  Value + gradients in one pass. */
int rsa_ssm_shared_loss(const rsa_loss_args* args, rsa_stream_t stream);

/* out[0] = mean(row_loss[0..n_rows)) in a fixed summation order (two tiny launches). */
int rsa_mean_rows(const float* row_loss, int64_t n_rows, float* out, void* scratch, rsa_stream_t stream);

/* SoftmaxLoss.forward on a MATERIALISED score matrix -- recstudio/model/loss_func.py:41:
 * lse[m] = logsumexp(x[m, :]); softmax_scaled (nullable) [n_rows, n_cols] = softmax(x) * scale
 * (= d mean(lse) / d x for scale = 1/n_rows). */
int rsa_row_lse(const float* x, int64_t n_rows, int64_t n_cols, float* lse, float* softmax_scaled,
                float scale, rsa_stream_t stream);

/* Backward of the fused forward (shown for the inner-product scorer; RSA_SCORE_COS applies the cosine
 * chain rule instead) == what autograd
 * produces at recommender.py:636-639 (embedding_dense_backward + bmm backward):
 *   item_grad[neg_ids[m,j]] += up * dneg[m,j] * q_m     (skipped for id == item_pad_row: padding_idx)
 *   item_grad[pos_ids[m]]   += up * dpos[m]   * q_m
 *   query_grad[m]            = up * (dpos[m] * item[pos] + sum_j dneg[m,j] * item[neg_j])
 * item_grad: dense [n_items, dim], accumulated with atomics, caller zero-fills
 * (nullable).  item_grad_rows: nullable [M*(n+1), dim] row-sparse values, row
 * m*(n+1) = positive, m*(n+1)+1+j = negative j (COO values for ids
 * cat(pos, neg); no atomics).  query_grad: nullable [M, dim], overwritten.
 * upstream: nullable device scalar (d final / d loss), default 1. */
typedef struct rsa_backward_args {
  const float* item_table;
  int64_t n_items;
  int32_t dim;
  int32_t num_neg;
  const float* query;
  const int64_t* query_index;
  int64_t n_query_rows;
  const int64_t* pos_ids;      /* nullable */
  const int64_t* neg_ids;      /* [M, n] */
  int64_t n_queries;
  const float* dpos;           /* [M] (nullable iff pos_ids null) */
  const float* dneg;           /* [M, n] */
  const float* upstream;
  float* item_grad;
  float* item_grad_rows;
  float* query_grad;
  float* query_table_grad;     /* nullable [n_query_rows, dim], atomics, caller-zeroed: the query gradient accumulated
                                  at row query_index[m] -- the dense grad of a user-embedding query
                                  tower in the same launch; also the per-query accumulation of the sharded backward */
  int32_t query_table_pad_row; /* row of query_table_grad that receives no gradient (padding_idx; 0 for a RecStudio
                                  user table), -1 = none */
  int32_t item_pad_row;        /* item row that receives no gradient (padding_idx = 0 in RecStudio); -1 = none (an
                                  item-table shard that does not hold the global row 0) */
  int32_t score_mode;          /* rsa_score_mode: RSA_SCORE_IP (tuned kernels) or RSA_SCORE_COS / RSA_SCORE_EUC (plain kernel) */
  int32_t _pad;
} rsa_backward_args;

int rsa_fused_backward(const rsa_backward_args* args, rsa_stream_t stream);

/* Atomics-free, bit-reproducible form of the item-side scatter-add of a step:
 *     target[id] += upstream * sum_{e : id_e = id} d_e * query[qrow_e]      (rows id != pad_row)
 * over the elements of the step (with pos_ids: the positive of query m first, then its num_neg negatives; without: the
 * negatives only; d = dpos / dneg).
 * The (id, element) pairs are radix-sorted (the in-tree stable LSD sort, csrc/rsa_radix.hpp) and every run of equal ids is summed by one wave in
 * element order, then the row is read-modified-written once.  `target` [n_items, dim] is a zeroed dense gradient
 * (== the reference's weight.grad, recommender.py:636-639) or the weight table itself with upstream = -lr (plain
 * SGD in place).  dim in {64, 128, 256}; pos_ids / dpos nullable; query_index nullable (query row m);
 * upstream: nullable device scalar; pad_row < 0: none.  Elements whose id is NEGATIVE are dropped (empty slots of
 * the fixed-capacity shard exchange): nothing is read or written for them.  Workspace from the _workspace_bytes call. */
int64_t rsa_scatter_rows_sorted_workspace_bytes(int64_t n_queries, int32_t num_neg, int64_t n_items);

/* With exp_avg / exp_avg_sq given the accumulate becomes a LAZY ADAM update of every touched row (the update rule of
 * torch.optim.SparseAdam on the coalesced gradient g[id] = upstream * sum_e d_e * query[qrow_e]):
 *     m += (g - m)(1 - beta1);  v += (g^2 - v)(1 - beta2);  weight -= lr * sqrt(1 - beta2^step) / (1 - beta1^step) * m / (sqrt(v) + eps)
 * exp_avg / exp_avg_sq: [n_items, dim] optimizer state, updated in place; rows not in the step are untouched (lazy).
 * The row sums never leave registers: no gradient tensor, no coalesce pass.  step >= 1 is the 1-based step count.
 * With rule = RSA_ROWS_ADAGRAD and state_sum given it is torch.optim.Adagrad's update of every touched row (lr, eps, step as
 * above; lr_decay; exp_avg / exp_avg_sq must be null):
 *     state_sum += g^2;  weight -= lr / (1 + (step - 1) * lr_decay) * g / (sqrt(state_sum) + eps)
 * A row outside the step has g = 0, which changes neither its state_sum nor its weight under the dense rule: leaving it alone
 * is exact, not lazy.  These fields were appended without a new RSA_ABI_VERSION: a shorter block reads them as 0 = rule 0. */
#define RSA_ROWS_ADAGRAD 1
typedef struct rsa_rows_update_args {
  int64_t size;                /* sizeof(rsa_rows_update_args) */
  const float* query;          /* [n_query_rows, dim] */
  const int64_t* query_index;  /* nullable [n_queries] (null: query row m) */
  int64_t n_query_rows;
  int32_t dim;                 /* 64, 128 or 256 */
  int32_t has_pos;             /* rsa_rows_update_presorted: the workspace was sorted WITH positives (pos_ids given to the sort) */
  const int64_t* pos_ids;      /* nullable [n_queries] */
  const int64_t* neg_ids;      /* [n_queries, num_neg] */
  int64_t n_queries;
  int32_t num_neg;
  int32_t _pad;
  const float* dpos;           /* [n_queries] (nullable iff no positives) */
  const float* dneg;           /* [n_queries, num_neg] */
  const float* upstream;       /* nullable device scalar */
  int64_t n_items;             /* rows of target */
  int64_t pad_row;             /* < 0: none */
  float* target;               /* [n_items, dim]: a zeroed dense gradient, or the weight table (upstream = -lr: SGD in place) */
  float* exp_avg;              /* nullable: lazy Adam state (then target = the weights) */
  float* exp_avg_sq;
  double lr, beta1, beta2, eps; /* as the caller holds them (ABI 12): 1 - beta and the bias corrections are computed in double, rounded to fp32 once */
  int64_t step;
  uint8_t* solo;               /* rsa_sort_step_elements: nullable [n_queries * (num_neg + has_pos)] out */
  void* workspace;
  int64_t workspace_bytes;     /* >= rsa_scatter_rows_sorted_workspace_bytes(n_queries, num_neg, n_items) */
  float* state_sum;            /* RSA_ROWS_ADAGRAD: [n_items, dim] sum of squared gradients (then target = the weights), updated in place */
  double lr_decay;             /* RSA_ROWS_ADAGRAD: clr = lr / (1 + (step - 1) * lr_decay), in double, rounded to fp32 once */
  int32_t rule;                /* 0: accumulate, or lazy Adam when exp_avg is given (what a block without this field asks for); RSA_ROWS_ADAGRAD */
  int32_t _pad2;
} rsa_rows_update_args;

/* sort + apply in one call (the former rsa_scatter_rows_sorted / rsa_adam_rows_sorted) */
int rsa_rows_update_sorted(const rsa_rows_update_args* args, rsa_stream_t stream);

/* The same in two steps, for a forward that updates the rows only one element touches itself
 * (rsa_fused_args.solo_flags):
 *   rsa_sort_step_elements   sorts the step's (item id, element) pairs into `workspace` (reads pos_ids, neg_ids, n_queries,
 *     num_neg, n_items, pad_row) and, with `solo` (uint8 [n_queries * (num_neg + has_pos)], element order
 *     m * (num_neg + has_pos) + c), classifies them: solo[e] = 1 iff element e is the only one on its row and the row is
 *     neither pad_row nor a negative (dropped) id; those elements are also flagged inside the workspace;
 *   rsa_rows_update_presorted  is the apply pass over that workspace: every run of equal ids
 *     summed by one wave, the row read-modified-written once -- except the flagged elements, whose rows it leaves alone
 *     (has_pos says whether the sort saw positives; pos_ids / neg_ids are not read).  With the lazy-Adam fields: over a
 *     workspace sorted WITHOUT `solo` -- the sort does not read the weights, so a trainer can issue it, and the sampling in
 *     front of it, for the next batch on another stream while the current step runs.
 * Nothing may touch the workspace in between.  dim in {64, 128, 256}. */
int rsa_sort_step_elements(const rsa_rows_update_args* args, rsa_stream_t stream);
int rsa_rows_update_presorted(const rsa_rows_update_args* args, rsa_stream_t stream);

/* Read-only (ABI 13): byte offset of the sorted pairs -- n_queries * (num_neg + has_pos) 8-byte words (key << 32 | element),
 * ascending by key, equal keys in element order; bit 31 of the element word set on the elements flagged solo -- inside the
 * workspace of rsa_sort_step_elements / rsa_rows_update_sorted, from the workspace pointer rounded UP to 256 bytes.  Which of
 * the sort's two buffers holds the result depends on the number of passes, i.e. on n_items.  < 0: bad sizes. */
int64_t rsa_scatter_rows_sorted_pairs_offset(int64_t n_queries, int32_t num_neg, int64_t n_items);

/* ---- The whole in-place SGD training step of a BPR two-tower model (nn.Embedding user and item tables, inner product,
 * BPRLoss, num_neg == 64) as TWO calls -- what `fit(train.fused_optimizer: 'sgd')` issues per batch.  Replaces, per step of
 * recstudio/model/basemodel/recommender.py:596-646: sampler.forward (ann/sampler.py:86-111 / :243-258), the two tower
 * look-ups, score_func, BPRLoss, loss.backward() and optimizer.step() of torch.optim.SGD (no momentum / weight decay).
 *   rsa_bpr_sgd_prepare  the part that does not read the weights: the negatives (the device random stream, "Philox
 *     state"; sampler RSA_SAMPLER_UNIFORM: ids in [1, n_items); RSA_SAMPLER_POPULAR: `pop`; RSA_SAMPLER_GIVEN: neg_ids is
 *     an INPUT) and ONE radix sort of the step's (item id, element) pairs followed by its (user id, query) pairs (user keys
 *     behind the item keys; item_workspace), + the solo classification of the item part (solo).  The negatives are drawn by
 *     the sort's first launch (same ids as rsa_sample_uniform / rsa_sample_popular, stored to neg_ids).
 *     A trainer issues it for batch k + 1 on a second stream while batch k's apply runs.
 *   rsa_bpr_sgd_apply    forward + loss + update: rsa_fused_sample_gather_score with the ids given, fused BPR epilogue, user
 *     gradient accumulated in the forward, solo item rows updated in the forward; the shared item rows and the user rows by
 *     the sorted apply pass over the two parts of the sorted pairs.  loss_out = the batch's mean BPR loss.
 * Bit-identical to the same sequence issued entry point by entry point.  dim in {64, 128, 256}. */
typedef struct rsa_bpr_sgd_args {
  int64_t size;                /* sizeof(rsa_bpr_sgd_args) */
  float* item_table;           /* [n_items, dim], updated in place */
  int64_t n_items;
  float* user_table;           /* [n_users, dim], updated in place */
  int64_t n_users;
  int32_t dim;
  int32_t num_neg;             /* 64 */
  const int64_t* user_ids;     /* [n_queries] */
  const int64_t* pos_ids;      /* [n_queries] */
  int64_t n_queries;
  int32_t sampler;             /* RSA_SAMPLER_UNIFORM / RSA_SAMPLER_POPULAR / RSA_SAMPLER_GIVEN (prepare) */
  int32_t _pad;
  const rsa_popular_args* pop; /* HOST pointer, RSA_SAMPLER_POPULAR: the tables (ids / logp / numel / philox fields ignored) */
  uint64_t seed, offset;       /* "Philox state" of the draw (prepare) */
  uint32_t grid_threads;
  uint32_t _pad2;
  uint64_t elem_base;
  const float* step_scale;     /* device scalar: -lr */
  int64_t* neg_ids;            /* [n_queries, num_neg]: out of prepare (in with RSA_SAMPLER_GIVEN), in of apply */
  uint8_t* solo;               /* [n_queries, 1 + num_neg]: out of prepare, in of apply */
  void* item_workspace;        /* rsa_scatter_rows_sorted_workspace_bytes(n_queries, num_neg + 1, n_items): item AND user elements (ABI 11) */
  int64_t item_workspace_bytes;
  void* user_workspace;        /* unused since ABI 11 (nullable) */
  int64_t user_workspace_bytes;
  float* pos_score;            /* [n_queries] out */
  float* neg_score;            /* [n_queries, num_neg] out */
  float* row_loss;             /* [n_queries] out */
  float* dpos;                 /* [n_queries] out */
  float* dneg;                 /* [n_queries, num_neg] out */
  float* query_grad;           /* [n_queries, dim] out */
  const float* ones;           /* [n_queries] of 1.0f (the coefficients of the user-row apply) */
  float* loss_out;             /* [1] out */
  void* reduce_scratch;        /* rsa_scratch_bytes(), of the stream apply runs on */
  int64_t uniform_high;        /* RSA_SAMPLER_UNIFORM: ids drawn in [1, uniform_high); 0 = n_items (UniformSampler(num_items) of a
                                  model whose table has num_items rows, mf/bpr.py:24-25) */
} rsa_bpr_sgd_args;
int rsa_bpr_sgd_prepare(const rsa_bpr_sgd_args* args, rsa_stream_t stream);
int rsa_bpr_sgd_apply(const rsa_bpr_sgd_args* args, rsa_stream_t stream);
/* Read-only (ABI 13): the same for rsa_bpr_sgd_prepare's item_workspace: the n_queries * (num_neg + 1) item pairs (keys 0 ..
 * n_items) followed by the n_queries user pairs (element n_queries * (num_neg + 1) + m, key n_items + 1 + user id). */
int64_t rsa_bpr_sgd_pairs_offset(int64_t n_queries, int32_t num_neg, int64_t n_items, int64_t n_users);

/* embedding_dense_backward: dst[ids[i]] += src[i] for ids != 0 (padding_idx=0).
 * Used for the user-table gradient.  dst [n_rows, dim] caller-zeroed. */
int rsa_scatter_add_rows(const float* src, const int64_t* ids, int64_t numel, int32_t dim,
                         float* dst, int64_t n_rows, rsa_stream_t stream);

/* SeqDataset batch materialisation + item_encoder(in_item_id) --
 * recstudio/data/dataset.py:1418-1439 (ragged [start,end) slices of the user-sorted
 * item column, right-padded with 0) + recstudio/model/seq/sasrec.py:42.
 * out_ids [B, max_len] int64 (nullable), out_rows [B, max_len, dim] (nullable),
 * out_len [B] int64 (nullable).  Segments longer than max_len keep their LAST
 * max_len items (dataset.py:1400,1409 windows to the most recent max_seq_len). */
typedef struct rsa_seg_gather_args {
  int64_t size;                /* sizeof(rsa_seg_gather_args) */
  const float* item_table;     /* nullable when out_rows is null */
  int64_t n_items;
  int32_t dim;
  int32_t max_len;
  const int64_t* flat_item_ids;
  int64_t n_flat;
  const int64_t* seg_start;
  const int64_t* seg_end;
  int64_t n_seg;
  int64_t* out_ids;            /* nullable [n_seg, max_len] */
  float* out_rows;             /* nullable [n_seg, max_len, dim] */
  int64_t* out_len;            /* nullable [n_seg] */
} rsa_seg_gather_args;
int rsa_seg_gather(const rsa_seg_gather_args* args, rsa_stream_t stream);

/* aux[r] of every row of a [n_rows, dim] table, the per-row operand of the cosine / Euclidean full-catalog scores:
 * RSA_SCORE_COS -> 1 / ||row||_2 (inf for a zero row: the reference divides by zero too, scorer.py:21-24),
 * RSA_SCORE_EUC -> ||row||_2^2 (scorer.py:28-34).  dim % 4 == 0. */
int rsa_row_sqnorm(const float* table, int64_t n_rows, int32_t dim, int32_t score_mode, float* out, rsa_stream_t stream);

/* Full-catalog scoring -- InnerProductScorer / CosineScorer / EuclideanScorer ([B,d],[N,d]) case, scorer.py:16, :19-34,
 * called from baseretriever.py:183-186 (training, FullScoreLoss) and :384 (topk).
 * Scores query [B, dim] against item_table rows [1, n_items) (item_vector =
 * weight[1:], baseretriever.py:122-123) with the fp32 MFMA
 * (v_mfma_f32_32x32x2_f32), never materialising [B, N-1] unless `scores` is given.
 *   scores : nullable [B, n_items-1] out (reference-style materialisation)
 *   lse    : nullable [B] out, logsumexp over the catalog (SoftmaxLoss, loss_func.py:41)
 *   topk_val / topk_idx : nullable [B, k] out, k <= 1024: largest k scores in descending order,
 *     ids are ITEM ids (1-based, baseretriever.py:385); equal scores -> smaller id first.
 *   dim must be 32, 64 or 128 (RSA_ERR_UNSUPPORTED otherwise).
 *   score_mode RSA_SCORE_COS / RSA_SCORE_EUC: the dot products of a tile are turned into cosine / negative squared
 *     distance in the tile epilogue, before logsumexp / filter / store:  cos = dot * item_aux * query_aux,
 *     euc = 2 dot - item_aux - query_aux, with item_aux [n_items - 1 + 64] (entry i-1 belongs to item row i; 16-byte
 *     aligned; the 64 trailing floats are padding the last tile of an item range may read -- any values) and
 *     query_aux [B] from rsa_row_sqnorm of the same mode; both null for RSA_SCORE_IP.
 *   workspace: device scratch of rsa_fullscore_workspace_bytes(B, n_items, k) bytes. */
int64_t rsa_fullscore_workspace_bytes(int64_t n_query, int64_t n_items, int32_t k);
typedef struct rsa_fullscore_args {
  int64_t size;                /* sizeof(rsa_fullscore_args) */
  const float* item_table;
  int64_t n_items;
  int32_t dim;
  int32_t score_mode;
  const float* query;
  int64_t n_query;
  float* scores;               /* nullable */
  float* lse;                  /* nullable */
  float* topk_val;             /* nullable */
  int64_t* topk_idx;           /* nullable */
  int32_t k;
  int32_t _pad;
  const float* item_aux;       /* nullable */
  const float* query_aux;      /* nullable */
  void* workspace;
  int64_t workspace_bytes;
} rsa_fullscore_args;
int rsa_fullscore(const rsa_fullscore_args* args, rsa_stream_t stream);

/* What rsa_fullscore(n_query, n_items, k) will do, read-only and host-only (no device call): filled from the very code the
 * launch runs.  `k` as for rsa_fullscore_workspace_bytes (0: no top-k, or the caller's `scores` hold the rows).  The caller sets
 * out->size = sizeof(rsa_fullscore_plan_info); at most that many bytes are written.
 *   filter            1: sample GEMM + threshold + filter epilogue + candidate select; 0: dense select over materialised rows
 *   groups, j         the threshold of a query is the j-th largest (value descending, group index ascending) of `groups` group
 *                     maxima; a group is group_tiles consecutive sampled tiles and sample tile s covers catalog items
 *                     1 + s * tile_stride * 32 + [0, 32).  On a dense plan: what the planner had worked out when it turned the
 *                     filter down (all zero below the smallest filtered catalog)
 *   expect            catalog items the planner expects above the threshold
 *   splits, items_per_split   the item ranges of the full GEMM's launch: range x = items [1 + x * items_per_split, ...)
 *   n_seg             candidate segments per query = 2 * splits (one per range and lane half; a lane half owns rows 4..7, 12..15,
 *                     20..23, 28..31 of every 32-item tile when it is the upper one); 0 on a dense plan
 *   seg, ovf, cand_max        slots of a segment, of a query's overflow list, and the most candidates the select takes
 *   *_offset          byte offsets, from the workspace pointer rounded up to 256 bytes, of thr [n_query] (float), flags [n_query]
 *                     (int32, 1 = the row went to the exact recompute), seg_cnt [n_query, n_seg] (int32) and ovf_cnt [n_query]
 *                     (int32, appends to the overflow list, may exceed ovf); -1 on a dense plan. */
typedef struct rsa_fullscore_plan_info {
  int64_t size;                /* sizeof(rsa_fullscore_plan_info) */
  int32_t filter;
  int32_t j;
  int64_t groups;
  int64_t sample_tiles;
  int64_t tile_stride;
  int64_t group_tiles;
  double expect;
  int64_t splits;
  int64_t items_per_split;
  int64_t n_seg;
  int32_t seg;
  int32_t ovf;
  int32_t cand_max;
  int32_t _pad;
  int64_t thr_offset;
  int64_t flags_offset;
  int64_t seg_cnt_offset;
  int64_t ovf_cnt_offset;
} rsa_fullscore_plan_info;
int rsa_fullscore_plan(int64_t n_query, int64_t n_items, int32_t k, rsa_fullscore_plan_info* out);

/* BaseRetriever.sampling(method='brute') -- baseretriever.py:299-328 -- and RetrieverSampler (recstudio/ann/sampler.py:61-78)
 * without the [B, N] matrix: num_neg ids per query, with replacement, from softmax(score(q, .) * inv_t) over item rows
 * [1, n_items), the ids of user_hist [n_query, hist_len] (0-padded, duplicates allowed) removed when it is given.
 *   lse [n_query]        logsumexp of the scaled scores over the whole catalog (history included, as the reference's softmax).
 *   neg_logp             s_id * inv_t - lse: the log of the masked, NOT renormalised row, as the reference takes it.
 *   pos_logp [., n_pos]  the same for pos_ids; -inf for the padding id 0 (log(gather(pad(softmax)))) and for ids >= n_items.
 * Two-level inverse CDF over blocks of G consecutive items (G = 64, 128 or 256, fixed when the library is built; block g =
 * items 1 + g * G ...; n_blocks = ceil((n_items - 1) / G)), two uniforms per draw:
 *   mass[q][g] = sum over the block of exp(s - lse), from one fp32-MFMA pass over the catalog; a block that holds a history
 *                id is summed again without the history (never by subtraction), a block wholly in the history is exactly 0;
 *   cum[q][g]  = running sum of mass in fixed point (a power-of-two unit per row: exact, monotone), rounded to fp32 once per entry;
 *   block      = the first g with cum[g] > fl32(u1 * cum[last]) (when rounding leaves none: the first g with cum[g] == cum[last]);
 *   item       = the block's rows are scored again with plain fp32 FMAs, w_i = exp(s_i - max of the block) in 2^-40 fixed point
 *                (history, id 0 and ids >= n_items weigh 0): the first i whose running sum exceeds floor(u2 * total).
 * An item of weight 0 is never returned.  A row whose every item weighs 0 gets id 0 with log-prob -inf (the checks below run on
 * the host and cannot see it).  The ids are NOT those of torch.multinomial for the same seed; the distribution and the
 * log-probabilities are.  Uniforms: elements (q * num_neg + j) * 2 + {0, 1} of ONE torch.rand(n_query, num_neg, 2) on the device
 * stream ("Philox state"); rsa_softmax_lookup takes them from u_in instead.  dim must be 32, 64 or 128 (RSA_ERR_UNSUPPORTED
 * otherwise); score_mode / item_aux (64 floats of padding) / query_aux as in rsa_fullscore.  mass / cum: nullable
 * [n_query, n_blocks] outputs (the tables the draw used).  num_neg = 0 leaves lse (and pos_logp).  All arguments are checked
 * before the first HIP call; nothing is allocated and nothing synchronises.  Extra memory: 16 bytes per (query, block). */
int64_t rsa_softmax_sample_workspace_bytes(int64_t n_query, int64_t n_items);
/* G of this build (callers size mass / cum with it). */
int32_t rsa_softmax_sample_block(void);
typedef struct rsa_softmax_sample_args {
  int64_t size;                /* sizeof(rsa_softmax_sample_args) */
  const float* item_table;     /* [n_items, dim], row 0 is the padding row */
  int64_t n_items;
  int32_t dim;
  int32_t score_mode;          /* rsa_score_mode */
  float inv_t;                 /* 1 / temperature, > 0 */
  int32_t num_neg;
  const float* query;          /* [n_query, dim] */
  int64_t n_query;
  const int64_t* pos_ids;      /* nullable [n_query, n_pos] */
  int32_t n_pos;
  int32_t hist_len;            /* 0: nothing is excluded */
  const int64_t* user_hist;    /* nullable [n_query, hist_len] */
  const float* item_aux;       /* nullable */
  const float* query_aux;      /* nullable */
  uint64_t seed, offset;       /* "Philox state" (rsa_softmax_sample) */
  uint32_t grid_threads;
  uint32_t _pad;
  uint64_t elem_base;
  const float* u_in;           /* rsa_softmax_lookup: the uniforms [n_query, num_neg, 2] */
  float* u_out;                /* nullable out (rsa_softmax_sample: the uniforms drawn) */
  int64_t* neg_ids;            /* [n_query, num_neg] out */
  float* neg_logp;             /* [n_query, num_neg] out */
  float* pos_logp;             /* [n_query, n_pos] out */
  float* lse;                  /* [n_query] out */
  float* mass;                 /* nullable [n_query, n_blocks] out */
  float* cum;                  /* nullable [n_query, n_blocks] out */
  void* workspace;
  int64_t workspace_bytes;     /* >= rsa_softmax_sample_workspace_bytes(n_query, n_items) */
} rsa_softmax_sample_args;
int rsa_softmax_sample(const rsa_softmax_sample_args* args, rsa_stream_t stream);
/* The same draw for caller-supplied uniforms (the tests hit the table edges with it). */
int rsa_softmax_lookup(const rsa_softmax_sample_args* args, rsa_stream_t stream);

/* Sparse (CSR) times dense, the propagation step of the graph retrievers (LightGCN: recstudio/model/graph/lightgcn.py:51-62,
 * recstudio/model/module/graphmodule.py:168-198 with mess_norm = 'both'):
 *   y[r, :]       = row_scale[r] * sum_e values[e] * x[indices[e], :]       e in [indptr[r], indptr[r + 1]), r in [0, n_rows)
 *   acc_out[r, :] = acc_scale * (acc_in[r, :] + y[r, :])                    when acc_out is given
 * values null: all ones; row_scale null: 1.  y is nullable when acc_out is given; acc_in and acc_out may be the same buffer (x
 * must not alias y or acc_out).  fp32 throughout, every product and every sum rounded once (no FMA contraction).  dim is a
 * multiple of 4 and at most 256; x, y, acc_in, acc_out and partials are 16-byte aligned.  Row and byte offsets are 64-bit.
 * No atomics: a row is summed by one wave in an order fixed by the matrix, dim and the plan, so two runs are bit-equal.
 *
 * THE PLAN (built once per matrix; ops.spmm_plan builds it with torch ops, any caller can from indptr alone).  Rows with more
 * than `chunk` edges ("split rows") are cut into pieces of `chunk` consecutive edges (the last one shorter); a piece is summed by
 * a wave of its own into partials[p, :] and a second launch adds a split row's partials in ascending p and applies row_scale and
 * the accumulation.  Rows of at most `chunk` edges take no part in the plan.  `plan` is ONE int64 device array of
 * plan_len >= 2 * n_split + 1 + 2 * n_parts entries:
 *   [0, n_split)                         split_row[s]   the split rows, ascending
 *   [n_split, 2 n_split + 1)             split_part[s]  first piece of split row s; split_part[n_split] = n_parts
 *   [2 n_split + 1, .. + n_parts)        part_row[p]    the row of piece p (= split_row[s] for split_part[s] <= p < split_part[s + 1])
 *   [2 n_split + 1 + n_parts, .. + n_parts)  part_edge[p]  its first edge: indptr[row] + (p - split_part[s]) * chunk
 * chunk, n_split and n_parts travel in the argument block (the checks below run on the host and do not read device memory).
 * partials: caller-owned fp32 [n_parts, dim] (partials_bytes >= n_parts * dim * 4), overwritten by every call.
 * A null pointer among indptr / indices / x, neither y nor acc_out, acc_out without acc_in, a bad dim, a negative size, chunk < 1,
 * a plan_len or partials_bytes that is too small: RSA_ERR_ARG before the first HIP call.  Out-of-range entries of indptr /
 * indices / plan are clamped into the arrays, never followed.  Two launches (one when n_split == 0); nothing is allocated and
 * nothing synchronises.
 *
 * THE PERTURBED FORM (SimGCL: recstudio/model/graph/simgcl.py:14-26, feat + sign(feat) * normalize(rand_like(feat)) * eps).  With
 * noise_eps != 0 the row's sum AFTER row_scale, s, is replaced by s' before y and the accumulation see it:
 *   u_c  = element noise_elem_base + r * dim + c of ONE torch.rand call over n_rows * dim outputs ("Philox state")
 *   q    = max(sqrt(sum_c u_c * u_c), 1e-12)         the sum in fp32 in the fixed order rsa_spmm.hip states
 *   s'_c = s_c + sgn(s_c) * (u_c / q) * noise_eps    sgn = +1 / -1 / 0 for s_c > 0 / < 0 / +-0 (torch.sign, not copysign)
 * so a row without edges stays exactly 0.  A split row is perturbed once, on its total; its uniforms and q do not depend on
 * the plan.  noise_u (nullable fp32 [n_rows, dim]) receives the raw uniforms.  The uniforms are bit-equal to torch.rand_like
 * of an [n_rows, dim] tensor while n_rows * dim < 2^31 (torch splits larger calls; here the element index is 64-bit).
 * A noise_eps that is not finite, noise_eps != 0 with noise_grid_threads 0 or no multiple of 256 or a noise_offset that is
 * no multiple of 4, noise_u with noise_eps == 0, a noise_u that is not 16-byte aligned: RSA_ERR_ARG before the first HIP call.
 * The noise fields were appended without a new RSA_ABI_VERSION: a shorter or zeroed block reads noise_eps = 0 = no noise. */
typedef struct rsa_spmm_args {
  int64_t size;                /* sizeof(rsa_spmm_args) */
  const int64_t* indptr;       /* [n_rows + 1] */
  const int32_t* indices;      /* [nnz] column of every edge */
  const float* values;         /* nullable [nnz] */
  int64_t n_rows;
  int64_t n_cols;              /* rows of x */
  int64_t nnz;
  int32_t dim;
  int32_t _pad;
  const float* x;              /* [n_cols, dim] */
  const float* row_scale;      /* nullable [n_rows] */
  float* y;                    /* nullable [n_rows, dim] out */
  const float* acc_in;         /* nullable [n_rows, dim] */
  float* acc_out;              /* nullable [n_rows, dim] out (may be acc_in) */
  float acc_scale;
  float _pad2;
  int64_t chunk;               /* the plan's chunk size (>= 1) */
  int64_t n_split;             /* rows longer than chunk */
  int64_t n_parts;             /* their pieces = rows of partials */
  const int64_t* plan;         /* nullable when n_split == 0 */
  int64_t plan_len;
  float* partials;             /* nullable when n_parts == 0 */
  int64_t partials_bytes;
  float noise_eps;             /* 0: no noise */
  uint32_t noise_grid_threads; /* "Philox state" of the torch.rand(n_rows, dim) call the noise stands for */
  uint64_t noise_seed;
  uint64_t noise_offset;
  uint64_t noise_elem_base;
  float* noise_u;              /* nullable [n_rows, dim] out: the uniforms */
} rsa_spmm_args;
int rsa_spmm_csr(const rsa_spmm_args* args, rsa_stream_t stream);

/* Graph augmentation of the self-supervised graph retrievers (SGL: recstudio/model/graph/sgl.py,
 * recstudio/model/module/data_augmentation.py:229-304, the dgl branch): thin the SYMMETRIC base graph held as the CSR of
 * rsa_spmm_csr (rows = destinations, indices = sources) and renormalise it by the degrees that survive.  rev[e] is the position
 * of edge e's reverse edge (a bijection: rev[rev[e]] = e, indices[rev[e]] = row(e), row(rev[e]) = indices[e]).
 *   keep[e]     = floor(u_e + keep_prob) != 0, u_e = element e of torch.rand(nnz) for the given Philox state (one fp32 add, the
 *                 rule of data_augmentation.py:250-251); and, with node_drop, neither end of e flagged.  keep_prob >= 1 consumes
 *                 no uniforms.  The two directions of an interaction are separate edges with separate draws (dgl.DropEdge on the
 *                 bidirectional graph): the thinned matrix is NOT symmetric.
 *   in_deg[r]   = kept edges of row r;  out_deg[c] = kept edges with source c (= the count over row c of keep[rev[e]])
 *   values[e]   = keep[e] ? (float)(f(out_deg[indices[e]]) * f(in_deg[r])) : +0,  f(k) = 1.0 / sqrt((double)k); the product is
 *                 taken in double and rounded once (GraphConv norm = 'both' on the thinned graph; no 1 / keep_prob factor)
 *   t_values[e] = values[rev[e]]: the TRANSPOSED thinned matrix in the same indptr / indices (and the same rsa_spmm_csr plan)
 * No float atomics; the degrees of rows longer than long_row (0: 2048; at least 128) are integer atomic sums of per-wave counts, at
 * most ceil(K / 64) per counter for a row of K edges; two runs are bit-equal.  Entries of indptr / indices / rev are clamped into
 * their arrays, never followed out of them.  A null indptr / indices / rev / values / in_deg / out_deg, a negative size, keep_prob
 * outside [0, 1], a long_row in [1, 128): RSA_ERR_ARG before the first HIP call.  One memset and two launches on the stream;
 * nothing is allocated and nothing synchronises. */
typedef struct rsa_graph_dropout_args {
  int64_t size;                /* sizeof(rsa_graph_dropout_args) */
  const int64_t* indptr;       /* [n_rows + 1] */
  const int32_t* indices;      /* [nnz] */
  const int64_t* rev;          /* [nnz] */
  int64_t n_rows;
  int64_t nnz;
  uint64_t seed;               /* Philox state of the torch.rand(nnz) call this stands for */
  uint64_t offset;
  uint32_t grid_threads;
  float keep_prob;
  uint64_t elem_base;
  const uint8_t* node_drop;    /* nullable [n_rows]: non-zero = every edge at this node falls */
  uint8_t* keep;               /* nullable [nnz] out */
  int32_t* in_deg;             /* [n_rows] out */
  int32_t* out_deg;            /* [n_rows] out */
  float* values;               /* [nnz] out */
  float* t_values;             /* nullable [nnz] out */
  int64_t long_row;            /* 0: the default */
} rsa_graph_dropout_args;
int rsa_graph_dropout(const rsa_graph_dropout_args* args, rsa_stream_t stream);

/* NGCF's BiCombiner layer with the normalise of the layer loop, fused (recstudio/model/module/graphmodule.py:70-86,
 * recstudio/model/graph/ngcf.py:63-86).  x = the layer's input, m = the aggregated neighbours, both fp32 [n_rows, d_in]:
 *   s = LeakyReLU((x + m) W1^T + b1),  p = LeakyReLU((x * m) W2^T + b2)      W1, W2 fp32 [d_out, d_in] (nn.Linear), b fp32 [d_out]
 *   h = dropout(s + p)                                                        fp32 [n_rows, d_out], contiguous (nullable)
 *   n = h / max(||h||_2, 1e-12)                                               written to columns [n_col, n_col + d_out) of a table
 *                                                                             whose rows are n_stride floats apart (nullable)
 * fp32 throughout, both products on the fp32 matrix cores; one launch.  d_in and d_out are multiples of 4, at most 128 each
 * (both weight matrices are kept in LDS).
 * THE DROPOUT.  q = (float)(1.0 - p).  Element (r, c) is kept iff u[r * d_out + c] < q and is then divided by q; u = element
 * elem_base + r * d_out + c of ONE torch.rand call over n_rows * d_out outputs ("Philox state"), bit-equal to torch.rand_like of
 * an [n_rows, d_out] tensor as long as torch draws that tensor in one call (it splits a tensor of several GiB into calls with
 * states of their own; the element index here is 64-bit).  p == 0 reads no Philox state and draws nothing.  This is NOT the
 * stream nn.Dropout's own kernel consumes.
 * rsa_bi_combine_backward takes the same inputs and state, recomputes the pre-activations and the mask (nothing is saved), and
 * writes dx, dm [n_rows, d_in], dw1, dw2 [d_out, d_in], db1, db2 [d_out] from g_h (the gradient arriving at h, nullable) and g_n
 * (the gradient of the column block, in the same strided form as n, nullable).  The sums over the rows are per-wave partials in
 * `workspace` (rsa_bi_combine_workspace_bytes) added in a fixed order by a last launch: no atomics, two runs are bit-equal.
 * Three launches.
 * A bad d_in / d_out / p / Philox state, a null or misaligned pointer (x, m, w1, w2, h, g_h and the column blocks: 16 bytes; strides
 * and column offsets multiples of 4), neither h nor n (forward), neither g_h nor g_n (backward), a workspace that is too small:
 * RSA_ERR_ARG before the first HIP call.  n_rows == 0 returns 0 and launches nothing.  Nothing is allocated, nothing synchronises. */
typedef struct rsa_bi_combine_args {
  int64_t size;                /* sizeof(rsa_bi_combine_args) */
  const float* x;              /* [n_rows, d_in] */
  const float* m;              /* [n_rows, d_in] */
  const float* w1;             /* [d_out, d_in] linear_sum.weight */
  const float* w2;             /* [d_out, d_in] linear_product.weight */
  const float* b1;             /* [d_out] */
  const float* b2;             /* [d_out] */
  int64_t n_rows;
  int32_t d_in;
  int32_t d_out;
  float negative_slope;
  uint32_t grid_threads;       /* "Philox state" of the torch.rand(n_rows, d_out) call the dropout stands for (p != 0) */
  double p;                    /* dropout probability in [0, 1) */
  uint64_t seed;
  uint64_t offset;
  uint64_t elem_base;
  float* h;                    /* forward: nullable [n_rows, d_out] out */
  float* n;                    /* forward: nullable out, base of the wider table */
  int64_t n_stride;            /* floats between its rows */
  int64_t n_col;               /* first column of the block */
  const float* g_h;            /* backward: nullable [n_rows, d_out] */
  const float* g_n;            /* backward: nullable, base of the wider gradient table */
  int64_t g_n_stride;
  int64_t g_n_col;
  float* dx;                   /* backward: [n_rows, d_in] out */
  float* dm;                   /* backward: [n_rows, d_in] out */
  float* dw1;                  /* backward: [d_out, d_in] out */
  float* dw2;
  float* db1;                  /* backward: [d_out] out */
  float* db2;
  void* workspace;             /* backward */
  int64_t workspace_bytes;     /* >= rsa_bi_combine_workspace_bytes(n_rows, d_in, d_out) */
} rsa_bi_combine_args;
int64_t rsa_bi_combine_workspace_bytes(int64_t n_rows, int32_t d_in, int32_t d_out);
int rsa_bi_combine(const rsa_bi_combine_args* args, rsa_stream_t stream);
int rsa_bi_combine_backward(const rsa_bi_combine_args* args, rsa_stream_t stream);

/* The attention core of the sequence towers, fused: what nn.MultiheadAttention computes between in_proj and out_proj as the
 * reference's nn.TransformerEncoder calls it (recstudio/model/seq/sasrec.py:25-36, :60-63).  qkv fp32 [n_seq, seq_len, 3 D],
 * D = n_head * head_dim, exactly what F.linear(x, in_proj_weight, in_proj_bias) returns: columns [0, D) are q, [D, 2 D) k,
 * [2 D, 3 D) v, head h in columns h * head_dim .. of each.  Per sequence b and head h:
 *   s_ij  = scale * <q_i, k_j>
 *   key j is allowed for query i iff (!causal or j <= i) and !key_pad[b, j]
 *   P_i.  = softmax over the allowed j;  lse_i = log sum_allowed exp(s_ij)                  lse fp32 [n_seq, n_head, seq_len]
 *   Pt_ij = keep_ij * P_ij / q;  out_i = sum_j Pt_ij v_j                                    out fp32 [n_seq, seq_len, D], heads
 *                                                                                           concatenated (out_proj's input)
 * A query with no allowed key gets out = 0, lse = -inf and passes no gradient (torch returns NaN there).  fp32 throughout, the
 * products on the fp32 matrix cores; one launch; nothing of size seq_len^2 is written (`keep` aside) or saved.
 * 1 <= seq_len <= 64, head_dim 16, 32 or 64, any n_head >= 1, any n_seq; 64-bit element offsets.
 * THE DROPOUT.  q = (float)(1.0 - p).  Element (b, h, i, j) is kept iff u < q, u = element elem_base + ((b * n_head + h) * seq_len
 * + i) * seq_len + j of ONE torch.rand([n_seq, n_head, seq_len, seq_len]) call ("Philox state"); disallowed positions own their
 * index like any other.  p == 0 reads no Philox state and draws nothing.  n_seq * n_head * seq_len^2 >= 2^31 with p > 0 is refused
 * (torch splits that call).  This is NOT the stream nn.Dropout's or the SDPA kernels' dropout consumes.
 * rsa_attention_backward takes qkv, key_pad, out and lse as the forward left them, g_out (the gradient of out) and the same Philox
 * state; it recomputes S and P = exp(s - lse), regenerates the mask and writes EVERY element of dqkv [n_seq, seq_len, 3 D] (zeros
 * where nothing flows).  All sums run inside one wave: no atomics, no workspace, two runs are bit-equal.
 * seq_len / head_dim / n_head outside the range, p outside [0, 1), a bad Philox state, a null or non-16-byte-aligned qkv / out /
 * g_out / dqkv, a null lse: RSA_ERR_ARG before the first HIP call.  n_seq == 0 returns 0 and launches nothing.  Nothing is
 * allocated, nothing synchronises. */
typedef struct rsa_attention_args {
  int64_t size;                /* sizeof(rsa_attention_args) */
  const float* qkv;            /* [n_seq, seq_len, 3 * n_head * head_dim] */
  const uint8_t* key_pad;      /* nullable [n_seq, seq_len]: non-zero = key j of sequence b is not attended */
  int64_t n_seq;
  int32_t seq_len;
  int32_t n_head;
  int32_t head_dim;
  int32_t causal;
  float scale;                 /* 1 / sqrt(head_dim) for nn.MultiheadAttention */
  uint32_t grid_threads;       /* "Philox state" of the torch.rand([n_seq, n_head, seq_len, seq_len]) call (p != 0) */
  double p;                    /* dropout probability in [0, 1) */
  uint64_t seed;
  uint64_t offset;
  uint64_t elem_base;
  float* out;                  /* forward: out; backward: in */
  float* lse;                  /* forward: out; backward: in */
  uint8_t* keep;               /* forward: nullable [n_seq, n_head, seq_len, seq_len] out (tests) */
  const float* g_out;          /* backward: [n_seq, seq_len, D] */
  float* dqkv;                 /* backward: [n_seq, seq_len, 3 D] out */
} rsa_attention_args;
int rsa_attention(const rsa_attention_args* args, rsa_stream_t stream);
int rsa_attention_backward(const rsa_attention_args* args, rsa_stream_t stream);

/* The GRU recurrence of the sequence towers (GRU4Rec, NARM), fused: the SEQUENTIAL part of torch.nn.GRU (one layer, one
 * direction, batch_first) as the reference's module.GRULayer runs it (recstudio/model/seq/gru4rec.py).  Gate order r, z, n:
 *   gh_t = w_hh h_{t-1} (+ b_hh)    r = sigma(gi_r + gh_r)    z = sigma(gi_z + gh_z)    n = tanh(gi_n + r * gh_n)
 *   h_t  = (1 - z) * n + z * h_{t-1}                          (b_hn sits INSIDE r * (.), as in torch)
 * gi fp32 [n_seq, seq_len, 3 hidden] = F.linear(x, W_ih, b_ih) is the caller's GEMM; h_{-1} = h0 (null: 0).  out fp32
 * [n_seq, seq_len, hidden] holds every h_t.  All seq_len steps run in ONE launch with w_hh resident in registers; the products
 * run on the fp32 matrix cores.  hidden 32, 64 or 128, any seq_len, any n_seq; 64-bit element offsets.
 * LENGTHS (nullable, device int64 [n_seq]): row b stops at lengths[b]: out[b, t >= lengths[b]] is +0 (nn.GRU runs on over the
 * padding; both consumers of the reference discard those positions).  Null: every row has seq_len steps and the op is nn.GRU at
 * every position.  The entry cannot read device memory: a device value outside [0, seq_len] is clamped into it by the kernel.
 * lengths_host (nullable, HOST int64 [n_seq]) is the caller's own copy, when it has one: an entry outside [0, seq_len] is
 * RSA_ERR_ARG.
 * rsa_gru_backward takes gi, out, h0, w_hh, lengths as the forward had them, gh fp32 [n_seq, seq_len, 3 hidden] =
 * F.linear(h_prev, w_hh, b_hh) with h_prev[:, t] = h_{t-1} (the caller's GEMM over all positions: h_prev is h0 followed by
 * out[:, :-1]) and g_out, the gradient of out.  With dh_t = g_out_t + carry it walks t = seq_len - 1 .. 0:
 *   dn = dh (1 - z)(1 - n^2)    dz = dh (h_{t-1} - n) z (1 - z)    dr = dn gh_n r (1 - r)    carry = dh z + w_hh^T [dr, dz, dn r]
 * and writes EVERY element of dgi = [dr, dz, dn] [n_seq, seq_len, 3 hidden], dgh_n = dn r [n_seq, seq_len, hidden] (the r and z
 * parts of dgh equal those of dgi) and dh0 [n_seq, hidden], +0 at t >= lengths[b].  d w_hh = dgh^T h_prev, d b_hh and the input
 * Linear's gradients are the caller's GEMMs.  No atomics, no workspace; two runs are bit-equal.
 * hidden outside {32, 64, 128}, negative n_seq / seq_len, a bad lengths_host entry, a null w_hh, a null or non-16-byte-aligned
 * gi / out (/ gh / g_out / dgi / dgh_n / dh0): RSA_ERR_ARG before the first HIP call.  n_seq == 0 returns 0 and launches
 * nothing.  Nothing is allocated, nothing synchronises. */
typedef struct rsa_gru_args {
  int64_t size;                /* sizeof(rsa_gru_args) */
  const float* gi;             /* [n_seq, seq_len, 3 * hidden] */
  const float* w_hh;           /* [3 * hidden, hidden] */
  const float* b_hh;           /* nullable [3 * hidden] (forward only: the backward's gh carries it) */
  const float* h0;             /* nullable [n_seq, hidden] */
  const int64_t* lengths;      /* nullable device [n_seq] */
  const int64_t* lengths_host; /* nullable HOST [n_seq]: checked against [0, seq_len] */
  int64_t n_seq;
  int32_t seq_len;
  int32_t hidden;
  float* out;                  /* forward: out; backward: in */
  const float* gh;             /* backward: [n_seq, seq_len, 3 * hidden] */
  const float* g_out;          /* backward: [n_seq, seq_len, hidden] */
  float* dgi;                  /* backward: [n_seq, seq_len, 3 * hidden] out */
  float* dgh_n;                /* backward: [n_seq, seq_len, hidden] out */
  float* dh0;                  /* backward: [n_seq, hidden] out */
} rsa_gru_args;
int rsa_gru(const rsa_gru_args* args, rsa_stream_t stream);
int rsa_gru_backward(const rsa_gru_args* args, rsa_stream_t stream);

/* Feed-forward (additive) attention pooling of the sequence towers (NARM, STAMP), fused: the reference's
 * module.AttentionLayer(attention_type='feedforward', one hidden layer, sigmoid) with ONE query per sequence, softmax=False and
 * value = key (recstudio/model/module/layers.py:322-399):
 *   hid_bs = sigmoid(qh_b + W_k k_bs)    a_bs = key_pad[b, s] ? 0 : (w2 . hid_bs + b2) * scale    out_b = sum_s a_bs k_bs
 * key fp32 [n_seq, seq_len, d]; qh fp32 [n_seq, m] = W1[:, :q_dim] q (+ b1) is the caller's GEMM; w_k = W1[:, q_dim:] is a
 * column block of the wider W1: row c starts at w_k + c * w_k_stride; w2 [m]; b2 a DEVICE pointer to one float; key_pad nullable
 * uint8 [n_seq, seq_len] (non-zero: weight 0 -- a fill with 0, not a softmax mask).  d and m each 32, 64 or 128; any seq_len >= 1.
 * rsa_ff_attention writes out [n_seq, d] and a [n_seq, seq_len] (+0 at padded positions) in one launch and nothing else.
 * rsa_ff_attention_backward takes the same inputs and g_out [n_seq, d], recomputes hid and a (nothing is saved), and writes EVERY
 * element of dkey [n_seq, seq_len, d] (+0 at padded positions), dqh [n_seq, m], dw_k [m, d] (dense), dw2 [m] and db2 [1]:
 *   da = g_b . k_bs   de = da * scale   dpre = de * w2 (.) hid (1 - hid)   dkey = a g_b + W_k^T dpre   dqh = sum_s dpre
 *   dw_k = sum_bs dpre k^T   dw2 = sum_bs de hid   db2 = sum_bs de
 * The sums over rows go through per-wave partial slots in `workspace` (rsa_ff_attention_workspace_bytes) added in a fixed order
 * by a last launch: no atomics, two runs are bit-equal.  64-bit element offsets.
 * d or m outside {32, 64, 128}, seq_len < 1, negative n_seq, a null or misaligned (16 bytes: key, qh, w_k, out, g_out; w_k_stride
 * a multiple of 4, >= d) pointer, a workspace that is too small: RSA_ERR_ARG before the first HIP call.  n_seq == 0 returns 0 and
 * launches nothing.  Nothing is allocated, nothing synchronises. */
typedef struct rsa_ff_attention_args {
  int64_t size;                /* sizeof(rsa_ff_attention_args) */
  const float* key;            /* [n_seq, seq_len, d] */
  const float* qh;             /* [n_seq, m] */
  const float* w_k;            /* [m, d] block of a wider matrix */
  int64_t w_k_stride;          /* floats between its rows */
  const float* w2;             /* [m] */
  const float* b2;             /* device [1] */
  const uint8_t* key_pad;      /* nullable [n_seq, seq_len] */
  int64_t n_seq;
  int32_t seq_len;
  int32_t d;
  int32_t m;
  float scale;
  float* out;                  /* forward: [n_seq, d] out */
  float* a;                    /* forward: [n_seq, seq_len] out */
  const float* g_out;          /* backward: [n_seq, d] */
  float* dkey;                 /* backward: [n_seq, seq_len, d] out */
  float* dqh;                  /* backward: [n_seq, m] out */
  float* dw_k;                 /* backward: [m, d] out */
  float* dw2;                  /* backward: [m] out */
  float* db2;                  /* backward: [1] out */
  void* workspace;             /* backward */
  int64_t workspace_bytes;     /* >= rsa_ff_attention_workspace_bytes(n_seq, seq_len, d, m) */
} rsa_ff_attention_args;
int64_t rsa_ff_attention_workspace_bytes(int64_t n_seq, int32_t seq_len, int32_t d, int32_t m);
int rsa_ff_attention(const rsa_ff_attention_args* args, rsa_stream_t stream);
int rsa_ff_attention_backward(const rsa_ff_attention_args* args, rsa_stream_t stream);

/* Hierarchical gating of the sequence tower HGN, fused (recstudio/model/seq/hgn.py:31-43 between the gathers and `U +`):
 *   f_bl = sigmoid(W1 s_bl + ug_b)   sf_bl = s_bl (.) f_bl   w_bl = sigmoid(w3 . sf_bl + ui_bl)   si_bl = sf_bl w_bl
 *   mean: pooled_b = sum_l si_bl / sum_l w_bl     max: pooled_b[c] = max_l si_bl[c]     out_b = pooled_b + sum_l s_bl
 * s fp32 [n_seq, seq_len, d] (padded positions are zero ROWS: there is no mask, they count in sum_l w and take part in the max
 * with si = +0); ug fp32 [n_seq, d] = W_g_2 U + b_g and ui fp32 [n_seq, seq_len] = U W_g_4.weight[:seq_len]^T are the caller's
 * GEMMs; w1 = W_g_1.weight [d, d], row c at w1 + c * w1_stride; w3 [d].  d is 32, 64 or 128; any seq_len >= 1; pooling 0 = mean,
 * 1 = max.
 * rsa_hgn_gating writes out [n_seq, d], w [n_seq, seq_len] and, for max pooling, arg int32 [n_seq, d] (the position of the
 * maximum, the LOWEST one on exact ties) in one launch and nothing else.
 * rsa_hgn_gating_backward takes the same inputs, g_out [n_seq, d] and the forward's w (and arg for max pooling), recomputes f and
 * sf, and writes EVERY element of ds [n_seq, seq_len, d] (not zero at padded positions), dug [n_seq, d], dui [n_seq, seq_len],
 * dw1 [d, d] (dense) and dw3 [d]:
 *   mean: dsi = g_b / den_b, dw = -(g_b . pooled_b) / den_b     max: dsi[c] = l == arg_b[c] ? g_b[c] : 0, dw = 0
 *   dw += dsi . sf   dz = dw w (1 - w)   dui = dz   dsf = dsi w + dz w3   dpre = (dsf (.) s) (.) f (1 - f)
 *   ds = g_b + dsf (.) f + W1^T dpre   dug_b = sum_l dpre   dw1 = sum_bl dpre s^T   dw3 = sum_bl dz sf
 * The sums over rows go through partial slots in `workspace` (rsa_hgn_gating_workspace_bytes) added in a fixed order by a last
 * launch: no atomics, two runs are bit-equal.  64-bit element offsets.
 * d outside {32, 64, 128}, seq_len < 1, negative n_seq, pooling outside {0, 1}, a null or misaligned (16 bytes: s, w1; w1_stride
 * a multiple of 4, >= d) pointer, a workspace that is too small: RSA_ERR_ARG before the first HIP call.  n_seq == 0 returns 0 and
 * launches nothing.  Nothing is allocated, nothing synchronises. */
typedef struct rsa_hgn_gating_args {
  int64_t size;                /* sizeof(rsa_hgn_gating_args) */
  const float* s;              /* [n_seq, seq_len, d] */
  const float* ug;             /* [n_seq, d] */
  const float* ui;             /* [n_seq, seq_len] */
  const float* w1;             /* [d, d], possibly a block of a wider buffer */
  int64_t w1_stride;           /* floats between its rows */
  const float* w3;             /* [d] */
  int64_t n_seq;
  int32_t seq_len;
  int32_t d;
  int32_t pooling;             /* 0 mean, 1 max */
  int32_t reserved;            /* 0 */
  float* out;                  /* forward: [n_seq, d] out */
  float* w;                    /* [n_seq, seq_len]: forward out, backward in */
  int32_t* arg;                /* max pooling, [n_seq, d]: forward out, backward in */
  const float* g_out;          /* backward: [n_seq, d] */
  float* ds;                   /* backward: [n_seq, seq_len, d] out */
  float* dug;                  /* backward: [n_seq, d] out */
  float* dui;                  /* backward: [n_seq, seq_len] out */
  float* dw1;                  /* backward: [d, d] out */
  float* dw3;                  /* backward: [d] out */
  void* workspace;             /* backward */
  int64_t workspace_bytes;     /* >= rsa_hgn_gating_workspace_bytes(n_seq, seq_len, d) */
} rsa_hgn_gating_args;
int64_t rsa_hgn_gating_workspace_bytes(int64_t n_seq, int32_t seq_len, int32_t d);
int rsa_hgn_gating(const rsa_hgn_gating_args* args, rsa_stream_t stream);
int rsa_hgn_gating_backward(const rsa_hgn_gating_args* args, rsa_stream_t stream);

/* Bag sum of table rows straight from a padded id matrix, and its backward (MultiDAE / MultiVAE: recstudio/model/ae/multidae.py:21-23
 * `item_embedding(ids).sum(1) / count_nonzero(ids, 1) ** 0.5`, and the per-user mean of the positives' rows in the softmax loss):
 *   cnt[b] = live ids of row b     out[b] = s_b * sum_{l live} table[ids[b, l]]     s_b = 1 (RSA_BAG_SUM), 1 / sqrt(cnt[b])
 *   (RSA_BAG_RSQRT) or 1 / cnt[b] (RSA_BAG_MEAN); an empty bag gives 0 under RSA_BAG_SUM and NaN under the other two (0 * inf).
 * An id is live when it is > 0: id 0 is padding and may stand anywhere in a row; padding is skipped, not read (equal to the
 * reference whenever row 0 of the table is zero).  A live id >= n_rows reads row n_rows - 1.  table fp32 [n_rows, d], ids int64
 * [n_bags, bag_len] with ids_stride elements between rows, d a multiple of 4 in [4, 1024], any n_bags, bag_len >= 0 with
 * n_bags * bag_len < 2^31, n_rows < 2^31 - 1; element offsets are 64-bit.
 * rsa_bag_pool writes out [n_bags, d] and cnt [n_bags].  bag_len <= 256: one launch, no workspace.  Longer rows: chunks of 256
 * positions are summed by a workgroup each into `workspace` and a second launch adds a bag's non-empty chunks in chunk order.  No
 * atomics; the order of the additions depends on d and on that row of ids only (the same bag gives the same bits anywhere).
 * rsa_bag_pool_backward takes ids, the forward's cnt, g [n_bags, d] and writes dw[i] = sum_{(b, l) : ids[b, l] = i} s_b g[b] into
 * the rows i it touches of dw [n_rows, d], which the CALLER has zeroed (row 0 is never written): a stable radix sort of the
 * (row, bag) pairs in `workspace`, then a wave per touched row adds in (bag, position) order and stores the row once.  No atomics,
 * bit-equal from run to run.
 * A d, scale or size outside the above, a null or misaligned (16 bytes: table, out, g, dw) pointer, an ids_stride below bag_len, a
 * workspace that is too small: RSA_ERR_ARG before the first HIP call.  n_bags == 0 returns 0 and launches nothing.  Nothing is
 * allocated, nothing synchronises. */
#define RSA_BAG_SUM 0
#define RSA_BAG_RSQRT 1
#define RSA_BAG_MEAN 2
typedef struct rsa_bag_args {
  int64_t size;                /* sizeof(rsa_bag_args) */
  const float* table;          /* forward: [n_rows, d] */
  const int64_t* ids;          /* [n_bags, bag_len], row b at ids + b * ids_stride */
  int64_t ids_stride;          /* elements between the rows of ids, >= bag_len */
  int64_t n_rows;
  int64_t n_bags;
  int32_t bag_len;
  int32_t d;
  int32_t scale;               /* RSA_BAG_* */
  int32_t reserved;            /* 0 */
  float* out;                  /* forward: [n_bags, d] out */
  int32_t* cnt;                /* [n_bags]: forward out, backward in */
  const float* g;              /* backward: [n_bags, d] */
  float* dw;                   /* backward: [n_rows, d], zeroed by the caller */
  void* workspace;             /* forward with bag_len > 256, backward */
  int64_t workspace_bytes;     /* >= rsa_bag_pool_workspace_bytes(n_bags, bag_len, n_rows) */
} rsa_bag_args;
int64_t rsa_bag_pool_workspace_bytes(int64_t n_bags, int32_t bag_len, int64_t n_rows);
int rsa_bag_pool(const rsa_bag_args* args, rsa_stream_t stream);
int rsa_bag_pool_backward(const rsa_bag_args* args, rsa_stream_t stream);

/* One augmented view of a batch of histories for the contrastive sequence retrievers (CL4SRec: recstudio/model/seq/cl4srec.py;
 * Item_Crop / Item_Mask / Item_Reorder, recstudio/model/module/data_augmentation.py:22-87), one launch.  The random choices are
 * the elements of ONE torch.rand([n_seq, seq_len + 1]) call for the given Philox state: U[b, 0] draws the start, U[b, 1 + p] is
 * the key of position p (the same layout for all three kinds).
 *   len   = clamp(seqlen[b], 0, seq_len)      n_sub = clamp(sub[len], 0, len)      sub int32 [seq_len + 1]: the caller's length
 *           table (the reference's max(1, int(tau n)) / int(gamma n) / int(beta n), taken in float64 on the host; sub[0] = 0)
 *   span  = max(len - n_sub + 1, 1)           start = min((int)(U[b, 0] * (float)span), span - 1)    (one fp32 product)
 *   RSA_SEQAUG_CROP    out[b, p] = p < n_sub ? seq[b, start + p] : 0;                                          new_len = n_sub
 *   RSA_SEQAUG_MASK    out[b, p] = mask_id where p < len and rank(p) < n_sub, else seq[b, p];                  new_len = len
 *                      rank(p) = #{q < len : U[b, 1 + q] < U[b, 1 + p], or equal and q < p}
 *   RSA_SEQAUG_REORDER out[b, start + rank(p)] = seq[b, p] for p in [start, start + n_sub), ranked among themselves the same way;
 *                      every other position is copied;                                                         new_len = len
 *   a row with len == 0 is copied and gets new_len = 0.
 * seq int64 [n_seq, seq_len], row b at seq + b * seq_stride (right-padded with 0); seqlen / new_len [n_seq] are int32 or int64
 * (seqlen_bytes 4 or 8); out int64 [n_seq, seq_len] dense, not aliasing seq.  seq_len <= RSA_SEQAUG_MAX_LEN: one lane per position
 * and one wave per sequence; no atomics, no workspace, two runs are bit-equal; nothing outside [0, seq_len) of a row is read.
 * seq_len outside [1, 64], an unknown kind, seqlen_bytes not 4 / 8, a negative n_seq, a null pointer, seq_stride < seq_len, out ==
 * seq: RSA_ERR_ARG before the first HIP call.  n_seq == 0 returns 0 and launches nothing.  Nothing is allocated, nothing
 * synchronises. */
enum rsa_seqaug_kind { RSA_SEQAUG_CROP = 0, RSA_SEQAUG_MASK = 1, RSA_SEQAUG_REORDER = 2 };
#define RSA_SEQAUG_MAX_LEN 64
typedef struct rsa_seq_augment_args {
  int64_t size;                /* sizeof(rsa_seq_augment_args) */
  const int64_t* seq;          /* [n_seq, seq_len], possibly a block of a wider buffer */
  int64_t seq_stride;          /* elements between its rows */
  const void* seqlen;          /* [n_seq], int32 or int64 */
  const int32_t* sub;          /* [seq_len + 1] */
  int64_t n_seq;
  int64_t mask_id;
  int32_t seq_len;
  int32_t kind;                /* rsa_seqaug_kind */
  int32_t seqlen_bytes;        /* 4 or 8: the element size of seqlen and new_len */
  uint32_t grid_threads;       /* Philox state of the torch.rand([n_seq, seq_len + 1]) call this stands for */
  uint64_t seed;
  uint64_t offset;
  uint64_t elem_base;
  int64_t* out;                /* [n_seq, seq_len] out */
  void* new_len;               /* [n_seq] out, the element type of seqlen */
} rsa_seq_augment_args;
int rsa_seq_augment(const rsa_seq_augment_args* args, rsa_stream_t stream);

/* In-batch InfoNCE of the contrastive sequence retrievers (InfoNCELoss neg_type 'batch_both' / 'batch_single',
 * recstudio/model/module/data_augmentation.py:324-376) without anything of size n_rows^2.  zi, zj fp32 [n_rows, d] dense, 16-byte
 * aligned (normalised by the caller for 'cosine'); d is 32, 64 or 128; any n_rows.  The logit set of row b:
 *   s_ij[b, k] = <zi_b, zj_k> inv_t for every k except those with k != b and labels[k] == labels[b];
 *   with `both` also s_ii[b, k] = <zi_b, zi_k> inv_t for every k != b whose label differs (labels null: every k != b).
 * rsa_batch_infonce writes lse[b] = log sum exp over the set and pos[b] = s_ij[b, b]; the loss is mean(lse - pos), the caller's.
 * rsa_batch_infonce_backward takes the same inputs, the forward's lse and g [n_rows] (the upstream of lse - pos), recomputes
 * P = exp(s - lse_b) on the fp32 matrix cores and writes every element of
 *   dzi_b = inv_t [ g_b (sum_k P_ij[b, k] zj_k + sum_k P_ii[b, k] zi_k - zj_b) + sum_r g_r P_ii[r, b] zi_r ]
 *   dzj_k = inv_t [ sum_b g_b P_ij[b, k] zi_b - g_k zi_k ]
 * in two launches (rows of zi stationary, then rows of zj stationary).  Nothing is saved but lse; no atomics, no workspace, two
 * runs are bit-equal; rows past n_rows are never read.  d outside {32, 64, 128}, a negative n_rows, inv_t not positive and
 * finite, a null or misaligned zi / zj, a null lse (/ pos / g / dzi / dzj), dzi or dzj aliasing an input or each other:
 * RSA_ERR_ARG before the first HIP call.  n_rows == 0 returns 0 and launches nothing.  Nothing is allocated, nothing synchronises. */
typedef struct rsa_batch_infonce_args {
  int64_t size;                /* sizeof(rsa_batch_infonce_args) */
  const float* zi;             /* [n_rows, d] */
  const float* zj;             /* [n_rows, d] */
  const int64_t* labels;       /* nullable [n_rows] */
  int64_t n_rows;
  int32_t d;
  int32_t both;                /* non-zero: the s_ii block too ('batch_both') */
  float inv_t;                 /* 1 / temperature */
  int32_t reserved;            /* 0 */
  float* lse;                  /* [n_rows]: forward out, backward in */
  float* pos;                  /* forward: [n_rows] out */
  const float* g;              /* backward: [n_rows] */
  float* dzi;                  /* backward: [n_rows, d] out */
  float* dzj;                  /* backward: [n_rows, d] out */
} rsa_batch_infonce_args;
int rsa_batch_infonce(const rsa_batch_infonce_args* args, rsa_stream_t stream);
int rsa_batch_infonce_backward(const rsa_batch_infonce_args* args, rsa_stream_t stream);

/* Backward of logsumexp over the full catalog (SoftmaxLoss, loss_func.py:39-47, when the forward was
 * rsa_fullscore(..., lse) and [B, N-1] was never written):  probs[b, i-1] = row_scale[b] * exp(<q_b, item_i> - lse[b])
 * = row_scale[b] * softmax_i, recomputed by the same MFMA kernel.  d lse/d query = probs @ items[1:],
 * d lse/d items[1:] = probs^T @ query are then plain library GEMMs on the caller's side.
 * row_scale may be null (1).  probs: [n_query, n_items-1]. */
int rsa_fullscore_softmax(const float* item_table, int64_t n_items, int32_t dim, const float* query,
                          int64_t n_query, const float* lse, const float* row_scale, float* probs,
                          rsa_stream_t stream);

/* The same pass that ALSO leaves query_grad [n_query, dim] = probs @ items[1:] (d lse/d query times row_scale): the
 * tile of probs the epilogue has just produced is multiplied with the item tile staged in LDS on the matrix cores, so
 * one of the two backward GEMMs needs no second pass over the 4 * n_query * n_items bytes of probs.  The per-item-range
 * partial sums go through `workspace` (rsa_fullscore_softmax_dq_workspace_bytes) and are added in range order
 * (reproducible).  probs is still written (d lse/d items = probs^T @ query remains a library GEMM on the caller's side). */
int64_t rsa_fullscore_softmax_dq_workspace_bytes(int64_t n_query, int64_t n_items, int32_t dim);
int rsa_fullscore_softmax_dq(const float* item_table, int64_t n_items, int32_t dim, const float* query,
                             int64_t n_query, const float* lse, const float* row_scale, float* probs,
                             float* query_grad, void* workspace, int64_t workspace_bytes, rsa_stream_t stream);

/* probs == NULL (ABI 10): the softmax tile feeds the second product and is NOT written -- together with
 * rsa_fullscore_softmax_dw below a backward that never holds [B, N] ("only if [B, N] is never written"). */

/* FLASH forward of the full softmax (ABI 10): lse[q] = logsumexp_i <q, item_i> over rows 1 .. n_items - 1 AND
 * query_grad[q, :] = d lse[q] / d q = softmax_q @ items[1:] in ONE pass over the catalog -- the softmax tile is formed against a
 * running per-query reference that only moves when a tile's maximum exceeds it by more than 8 (the dQ accumulators and the running
 * sum are then rescaled: rare after the first tiles), per-item-range records (reference, sum, unnormalised sum P * item) are merged
 * in range order (reproducible).  A training step of SoftmaxLoss (loss_func.py:39-47 over scorer.py:16) is then this call (two
 * products of 2 B N d flop) + rsa_fullscore_softmax_dw (two more): d loss/d query = upstream[q] * query_grad[q], no [B, N] matrix,
 * no second pass for the query gradient.  workspace: rsa_fullscore_lse_grad_workspace_bytes.  dim in {32, 64, 128}. */
int64_t rsa_fullscore_lse_grad_workspace_bytes(int64_t n_query, int64_t n_items, int32_t dim);
int rsa_fullscore_lse_grad(const float* item_table, int64_t n_items, int32_t dim, const float* query, int64_t n_query,
                           float* lse, float* query_grad, void* workspace, int64_t workspace_bytes, rsa_stream_t stream);

/* d lse / d items WITHOUT probs (ABI 10): item_grad[i, :] = sum_b row_scale[b] * exp(<q_b, item_i> - lse[b]) * q_b for rows
 * i = 1 .. n_items - 1, item_grad[0, :] = 0 -- the reference's autograd through loss_func.py:39-47 over scorer.py:16.  Item-
 * stationary: a wave keeps its 32 item rows in registers, recomputes the [32 batch rows x 32 items] score tile per batch chunk
 * on the fp32 matrix cores, forms the scaled softmax in its accumulator registers and feeds them back as the operand of
 * item_grad^T += P^T Q (the accumulator layout IS the operand layout when the chunk's rows are taken in that order) -- the
 * [B, N] matrix exists nowhere, every output row is written once, no atomics.  flops 4 B N d, HBM bytes 8 N d.  row_scale may
 * be NULL (1).  item_table / query / item_grad 16-byte aligned, dim in {32, 64, 128}. */
int rsa_fullscore_softmax_dw(const float* item_table, int64_t n_items, int32_t dim, const float* query, int64_t n_query,
                             const float* lse, const float* row_scale, float* item_grad, rsa_stream_t stream);

/* The other backward GEMM, d lse / d items[1:] = probs^T @ query (ATen's mm backward of scorer.py:16 under loss_func.py:39-47),
 * item-stationary on the fp32 matrix cores: out[i, :] = sum_b probs[b, i] * query[b, :] for i in [0, n_cols) -- every output row
 * written once, no atomics, no split-K partials.  probs [n_query, ld] (ld >= n_cols: its row stride), query [n_query, dim],
 * out [n_cols, dim] (the caller passes item_grad + dim: row 1 of the table gradient; row 0 stays zero), dim in {32, 64, 128}. */
int rsa_probs_t_query(const float* probs, int64_t n_query, int64_t n_cols, int64_t ld, const float* query, int32_t dim,
                      float* out, rsa_stream_t stream);

/* torch.topk(values, k) over the last dim of a [n_rows, n_cols] matrix (k <= 1024): values in descending
 * order and their COLUMN indices (equal values -> smaller column first).  Used by the 'dns' sampling method
 * (baseretriever.py:343-347: the hardest num_neg[1] of a sampled pool of num_neg[0] negatives). */
int rsa_row_topk(const float* values, int64_t n_rows, int64_t n_cols, int32_t k, float* out_val,
                 int64_t* out_col, rsa_stream_t stream);

/* History exclusion of BaseRetriever.topk -- baseretriever.py:386-392: candidates (sorted
 * descending, [n_query, n_cand], item ids) that appear in user_hist [n_query, hist_len] (0-padded)
 * get score -inf; out = the k best survivors in order (masked ones, as -inf, fill the tail only
 * when fewer than k survive). */
int rsa_topk_mask_history(const float* cand_val, const int64_t* cand_idx, int32_t n_cand,
                          const int64_t* user_hist, int32_t hist_len, int64_t n_query, int32_t k,
                          float* out_val, int64_t* out_idx, rsa_stream_t stream);

/* ---- Row-sharded item table (BASELINE.json configs[3]; no counterpart in the reference, whose
 * only multi-device mode re-broadcasts whole tables every step, utils/data_parallel.py:106-159).
 * Shard g owns item rows [g*rows_per_shard, (g+1)*rows_per_shard); with rows_per_shard == 0 the rows
 * are INTERLEAVED instead: owner(id) = id % n_shards, local row = id / n_shards (every owner holds
 * 1/n_shards of any id range, so ids ordered by popularity do not make a hot shard).  An "element" is one (query,
 * item) pair of the [n_queries, 1+num_neg] matrix whose column 0 is pos_ids and columns 1.. are
 * neg_ids.  Elements are counting-sorted by owner into contiguous per-owner segments and travel
 * as one packed key = (query_base + query) << 32 | local_row; the fp32 scores come back in the
 * same order; `positions[i]` is the slot of element i's score in the home buffer
 * [pos_score (n_queries) | neg_score (n_queries x num_neg)], which rsa_scatter_f32 fills. */
int rsa_shard_count(const int64_t* pos_ids, const int64_t* neg_ids, int64_t n_queries, int32_t num_neg,
                    int64_t rows_per_shard, int32_t n_shards, int32_t* counts /* [n_shards] out */,
                    rsa_stream_t stream);
/* cursor [n_shards]: IN the exclusive prefix sum of counts (segment starts), clobbered. */
int rsa_shard_route(const int64_t* pos_ids, const int64_t* neg_ids, int64_t n_queries, int32_t num_neg,
                    int64_t rows_per_shard, int32_t n_shards, int64_t query_base, int32_t* cursor,
                    int64_t* keys, int64_t* positions, rsa_stream_t stream);
int rsa_shard_unpack(const int64_t* keys, int64_t numel, int64_t* local_rows, int64_t* query_index,
                     rsa_stream_t stream);
/* dst[positions[i]] = src[i] for positions[i] >= 0 (exact exchange) */
int rsa_scatter_f32(const float* src, const int64_t* positions, int64_t numel, float* dst, rsa_stream_t stream);
/* dst[i] = positions[i] >= 0 ? src[positions[i]] : 0: d loss/d score in routed order for the gradient exchange. */
int rsa_gather_f32(const float* src, const int64_t* positions, int64_t numel, float* dst, rsa_stream_t stream);

/* ---- Version 2 of the fixed-capacity exchange (ABI v5).  What changed against rsa_shard_route_fixed + rsa_scatter_f32 +
 * rsa_pairwise_loss: (a) the negatives are drawn INSIDE the routing pass (same Philox element mapping as
 * rsa_sample_uniform / rsa_sample_popular, so the ids are the ones the stand-alone samplers -- and the reference's
 * torch.randint / torch.rand + searchsorted, sampler.py:102-104, :246-258 -- produce); the [n_queries, num_neg] id tensor
 * is written only on request; (b) a segment is SELF-DESCRIBING: RSA_SHARD_HDR 8-byte header words {live keys, elements
 * the source rank dropped in this step -- in bank 0 of every (slice, owner), 0 elsewhere} precede its keys, so the slack is never filled, owners skip the tiles past the
 * count, and after the key all-to-all every rank knows the job-wide number of dropped elements of the step without a
 * collective of its own; (c) the home side keeps ONE int32 per element (slot_of: where its key sits in the send buffer
 * == where its score sits in the returned buffer; -1 = dropped) instead of an 8-byte position per slot, and gathers
 * through it inside the loss kernel (rsa_shard_home) -- no scatter pass, no separate loss / mean launches; (d) one
 * routing launch covers all pipelined query slices.
 * A DROPPED element (its owner's segment was full) has a defined outcome: no key, no score (reads as 0 where scores are
 * materialised), no term in a fused loss, d loss / d score = 0 (nothing is sent for it); and the owner-side update
 * scale of a step in which ANY rank dropped anything is 0 (rsa_shard_unpack_segments), so such a step leaves every
 * weight untouched. */
#define RSA_SHARD_HDR 2   /* 8-byte header words per segment: [0] live keys, [1] the source's dropped total of the step */

typedef struct rsa_shard_route_args {
  const int64_t* pos_ids;      /* [n_queries] global item ids (column 0 of the element matrix) */
  int64_t* neg_ids;            /* [n_queries, num_neg]: INPUT when sampler == RSA_SAMPLER_GIVEN, else nullable OUTPUT */
  float* neg_logp;             /* nullable [n_queries, num_neg] out (POPULAR): log pop_prob[id] */
  float* pos_logp;             /* nullable [n_queries] out: log pop_prob[pos_ids] (needs pop_prob) */
  int64_t n_queries;
  int32_t num_neg;
  int32_t sampler;             /* rsa_sampler_kind */
  int32_t n_slices;            /* pipelined slices (>= 1): slice c = the c-th of n_slices contiguous ranges of the launch's
                                  workgroups -- an arbitrary, run-independent partition of the step's elements */
  int32_t n_shards;            /* G <= 64 */
  int32_t n_banks;             /* >= 1: what goes to one owner in one slice is split over n_banks segments, each filled through its
                                  own cursor by its own share of the launch's workgroups (one cursor per owner makes every
                                  workgroup queue up on one atomic address); n_slices * n_shards * n_banks <= 4096 */
  int32_t _pad0;
  int64_t rows_per_shard;      /* owner(id) = min(id / rows_per_shard, G - 1); 0: interleaved, owner = id % G, row = id / G */
  int64_t query_base;          /* global index of query 0 (rank * n_queries): goes into the keys */
  int64_t capacity;            /* keys per (slice, owner, bank) segment */
  int64_t n_items;             /* catalog size: uniform ids are drawn from [1, n_items) */
  uint64_t seed, offset;       /* Philox state, see "Philox state" (sampler != GIVEN) */
  uint32_t grid_threads;
  uint32_t _pad;
  uint64_t elem_base;
  const float* table;          /* POPULAR: as in rsa_fused_args */
  const float* pop_prob;
  const int32_t* guide;
  const float* table_prob;
  const float* cdf_lut;
  const float* cdf_lines;
  int32_t guide_log2;
  int32_t lines_log2;
  int64_t* send_keys;          /* [n_slices][n_shards][n_banks][RSA_SHARD_HDR + capacity] out; key = (query_base + query) << 32 | local row.
                                  NULL: count only (nothing is sampled into the outputs, only counts_out is written) */
  int32_t* slot_of;            /* [n_queries * (1 + num_neg)] out, element e = query * (1 + num_neg) + column */
  int32_t* cursors;            /* [(n_slices * n_shards * n_banks + 33) * 32] int32 device scratch (one 128-byte line per cursor
                                  and ticket), zeroed ONCE by the caller (self-resetting) */
  int32_t* counts_out;         /* nullable [n_slices * n_shards * n_banks]: exact element counts per segment -- calibration */
  int32_t skip_pos;            /* != 0: the positives are NOT routed (slot_of of column 0 = -1): the owner-side BPR step
                                  (rsa_shard_owner_bpr_forward) scores them from the gathered ids instead */
  int32_t group_by_query;      /* != 0 (needs skip_pos, an in-kernel sampler and rsa_shard_route_query_groups(...) > 0): a workgroup's
                                  share of a segment is written query by query -- every query's elements for an owner form ONE
                                  contiguous run of the segment (rsa_shard_owner_bpr_args.keys_grouped: no sort by query there) */
  /* DETERMINISTIC slots (ABI 9): with deterministic != 0 no atomic decides where an element's key lands -- a count pass, an
   * exclusive prefix over the workgroups in launch order and the routing pass (three launches instead of one: +20-45 us at
   * 4.2 M elements): the send buffer, and with it every sum the owners form in slot order, is then bit-identical run to run.
   * wg_scratch: caller-owned, 2 * rsa_shard_route_workgroups(args) * n_shards ints (contents irrelevant). */
  int32_t deterministic;
  int32_t _pad1;
  int32_t* wg_scratch;
  int64_t wg_scratch_ints;
  int32_t* extra_dropped;      /* nullable device word: elements of this step that were dropped OUTSIDE this call (the fixed-capacity row
                                  look-up of an item-tower query encoder).  Added to the dropped total the segment headers carry -- the
                                  owners gate the step like any routing overflow -- and reset to 0 */
} rsa_shard_route_args;
int64_t rsa_shard_segment_stride(int64_t capacity);    /* RSA_SHARD_HDR + capacity: 8-byte words per segment */
int rsa_shard_sample_route(const rsa_shard_route_args* args, rsa_stream_t stream);
/* workgroups the call above launches for these arguments (host arithmetic only) */
int64_t rsa_shard_route_workgroups(const rsa_shard_route_args* args);
/* Queries per workgroup if a call with these parameters can route query-grouped (num_neg a divisor of 1024 and >= 64, the
 * random call's grid a multiple of 1024 threads, the rank's element base a multiple of num_neg; unroll = 4, or 2 for the
 * 64-bit draws of catalogs beyond 2^28 items), else 0. */
int32_t rsa_shard_route_query_groups(int32_t num_neg, uint32_t grid_threads, uint64_t elem_base, int32_t unroll,
                                     int32_t n_shards);

/* Owner side: scores[i] = <query[key_i >> 32], item_table[key_i & 0xffffffff]> for every live slot of the received
 * segments keys [n_segments][stride] (the fused gather+score kernel of rsa_fused_sample_gather_score reading the
 * segments directly; slots past a segment's count are not read and their score is not written; whole tiles past the
 * count are skipped).  step_dropped (nullable int32 device word) <- sum over the segments of header word 1 (the job-wide
 * dropped count of the step when the segments come from all ranks); overflow_sticky (nullable) += the same. */
int rsa_shard_score_segments(const float* item_table, int64_t n_rows, int32_t dim, const float* query,
                             int64_t n_query_rows, const int64_t* keys, int64_t n_segments, int64_t stride, float* scores,
                             int32_t* step_dropped, int32_t* overflow_sticky, rsa_stream_t stream);

/* Home side: gather the returned scores through slot_of and evaluate the loss in the same launch (one wave per query).
 * loss 0: pos_score / neg_score only.  loss 1: BPRLoss (loss_func.py:55-59).  loss 2: SampledSoftmaxLoss (:80-90) with
 * nullable log-probabilities.  loss_out = sum(row_loss) / mean_den (mean_den = n_queries for the local mean, the job-wide
 * query count for this rank's share of the global mean); dpos / dneg / d_send = d loss_out / d score, d_send in routed
 * order (index = slot) ready for the gradient all-to-all.  Every output is nullable except neg_score for loss 0. */
typedef struct rsa_shard_home_args {
  const float* scores;         /* returned score buffer, indexed by slot */
  const int32_t* slot_of;      /* [n_queries * (1 + num_neg)] */
  int64_t n_queries;
  int32_t num_neg;
  int32_t loss;
  const float* pos_logp;       /* loss 2, nullable [n_queries] */
  const float* neg_logp;       /* loss 2, nullable [n_queries, num_neg] */
  int64_t mean_den;
  float* pos_score;            /* nullable [n_queries] out */
  float* neg_score;            /* nullable [n_queries, num_neg] out */
  float* row_loss;             /* nullable [n_queries] out */
  float* loss_out;             /* nullable [1] out (needs reduce_scratch) */
  float* dpos;                 /* nullable [n_queries] out */
  float* dneg;                 /* nullable [n_queries, num_neg] out */
  float* d_send;               /* nullable, slot-indexed out */
  void* reduce_scratch;        /* rsa_scratch_bytes() bytes, zeroed once */
} rsa_shard_home_args;
int rsa_shard_home(const rsa_shard_home_args* args, rsa_stream_t stream);

/* d_send[slot_of[e]] = (dpos | dneg)[e] for a loss evaluated outside rsa_shard_home (dropped elements send nothing). */
int rsa_shard_scatter_slots(const float* dpos, const float* dneg, const int32_t* slot_of, int64_t n_queries,
                            int32_t num_neg, float* d_send, rsa_stream_t stream);

/* Owner side of the backward: (local row, query index) per slot of the received segments, -1 past a segment's count
 * (rsa_rows_update_sorted drops negative ids); scale_out (nullable, 2 floats) = {gate * (scale_in ? scale_in[0] : 1),
 * gate} with gate = step_dropped[0] != 0 ? 0 : 1 -- the `upstream` scalars of the item-side and the query-side
 * sorted scatter, so that a step in which any rank dropped an element updates nothing. */
int rsa_shard_unpack_segments(const int64_t* keys, int64_t n_segments, int64_t stride, int64_t* local_rows,
                              int64_t* query_index, const float* scale_in, const int32_t* step_dropped, float* scale_out,
                              rsa_stream_t stream);

/* The whole owner side of the sharded backward on received segments (replaces rsa_shard_unpack_segments + two
 * rsa_rows_update_sorted calls, i.e. the ATen sequence autograd runs for the reference's
 * item_encoder(neg ids) / score_func backward, recommender.py:636-639, on the rows this rank owns):
 *     qgrad_all[q]   += gate * sum_{slots of query q} d[slot] * item_local[row(slot)]
 *     item_target[r] += gate * item_scale * sum_{slots on row r} d[slot] * q_all[query(slot)]      (r != item_pad_row)
 * with gate = step_dropped[0] != 0 ? 0 : 1 (scale_out <- {gate * item_scale, gate}).  item_target == item_local: plain
 * SGD in place (item_scale = -lr) -- rows that ONE slot of the step touches are rewritten by the walk that reads them
 * for the query gradient, the others by the sorted apply pass; otherwise item_target is this rank's block of the dense
 * gradient.  Deterministic (no float atomics).  dim in {64, 128, 256}.  `workspace`: caller-owned,
 * rsa_shard_backward_workspace_bytes(n_segments, stride, n_query_rows) bytes. */
typedef struct rsa_shard_backward_args {
  const float* item_local;     /* [n_rows, dim] this rank's rows */
  int64_t n_rows;
  int32_t dim;
  const float* q_all;          /* [n_query_rows, dim] the gathered queries of all ranks */
  int64_t n_query_rows;
  const int64_t* keys;         /* [n_segments, stride] received segments (RSA_SHARD_HDR header words + keys) */
  int64_t n_segments;
  int64_t stride;
  const float* d_owner;        /* [n_segments * stride] d loss / d score in slot order (slack: never read) */
  float* item_target;          /* item_local itself (in-place SGD) or the [n_rows, dim] gradient block */
  const float* item_scale;     /* device scalar, nullable (1) */
  const int32_t* step_dropped; /* device word, nullable (no gate) */
  float* scale_out;            /* [2] device: {gate * item_scale, gate} */
  float* qgrad_all;            /* [n_query_rows, dim], accumulated into */
  int64_t item_pad_row;        /* row that never receives gradient (-1: none) */
  void* workspace;
  int64_t workspace_bytes;
} rsa_shard_backward_args;
int64_t rsa_shard_backward_workspace_bytes(int64_t n_segments, int64_t stride, int64_t n_query_rows);
/* Read-only (ABI 13): out5 <- byte offsets (from the workspace pointer rounded UP to 256 bytes) of what the owner entry points
 * leave in that workspace: [0] the row-sorted pairs (n_segments * stride slots + the n_query_rows positives when pos_rows is
 * given), [1] the query-sorted pairs of the slots, [2] run_start and [3] run_end (int32 [n_query_rows]), [4] the solo flags
 * (uint8, element order).  n_rows: rows of the local item table (its key width picks the buffer of [0]). */
int rsa_shard_backward_workspace_offsets(int64_t n_segments, int64_t stride, int64_t n_query_rows, int64_t n_rows, int64_t* out5);
int rsa_shard_backward_segments(const rsa_shard_backward_args* args, rsa_stream_t stream);

/* The stock BPR training step (loss_func.py:55-59 on the scores of baseretriever.py:153-171, and its backward) evaluated
 * ON THE OWNERS of the negatives -- the item rows of a step are then read once instead of twice (scoring pass + backward
 * pass), and neither scores nor score gradients cross the fabric:
 *   rsa_shard_pos_score          out[i] = q_all[i] . item_local[pos_rows[i]] for the positives this rank owns (pos_rows[i]
 *                                >= 0: the local row; < 0: another rank's; derived from the gathered global ids in the same
 *                                launch when pos_ids is given), 0 for the others -- summed over the ranks
 *                                (a 4-byte-per-query all-reduce) it is every positive's score on every rank;
 *   rsa_shard_owner_bpr_forward  over the negatives this rank received (the positives are NOT routed in this protocol):
 *                                score, loss term -logsigmoid(pos - neg) / num_neg, d = sigmoid(neg - pos) / (num_neg *
 *                                mean_den) (-> d_slots[slot]), qgrad_all[q] += gate * sum d * row, rows that one element of
 *                                the step touches updated in place (item_target == item_local, scale = gate * item_scale);
 *                                dsum_part[q] = the query's sum of d here, loss_part = this rank's share of the mean loss.
 *                                Also publishes the step's dropped total (the received headers' word 1) into step_dropped /
 *                                overflow_sticky and the update scales into scale_out, like rsa_shard_score_segments +
 *                                rsa_shard_backward_segments do in the score-at-home protocol;
 *   rsa_shard_owner_bpr_finish   with dsum_all = the ranks' dsum_part summed (second small all-reduce): the positives this
 *                                rank owns -- d loss/d pos = -dsum_all[q] (-> d_slots[slots + q]), qgrad_all[q] += gate *
 *                                dpos * row, the row updated in place when it is the positive's alone -- and then the
 *                                sorted apply pass for every row several elements (negatives or positives) touch.
 * Same workspace (rsa_shard_backward_workspace_bytes) and the same args for both calls of a step.  dim in {64, 128, 256}. */
typedef struct rsa_shard_owner_bpr_args {
  const float* item_local;     /* [n_rows, dim] */
  int64_t n_rows;
  int32_t dim;
  int32_t num_neg;             /* negatives per query of the step (the 1/n of BPRLoss) */
  const float* q_all;          /* [n_query_rows, dim] */
  int64_t n_query_rows;
  const int64_t* keys;         /* [n_segments, stride] received segments (negatives only) */
  int64_t n_segments;
  int64_t stride;
  const int64_t* pos_rows;     /* [n_query_rows] local row of each query's positive on this rank, < 0: not owned */
  const float* pos_score;      /* [n_query_rows] */
  int64_t mean_den;            /* queries of the step over all ranks (the mean of BPRLoss) */
  float* item_target;          /* item_local (SGD in place) or the [n_rows, dim] gradient block */
  const float* item_scale;     /* device scalar, nullable (1) */
  int32_t* step_dropped;       /* device word, written */
  int32_t* overflow_sticky;    /* device word, accumulated */
  float* scale_out;            /* [2] device */
  float* qgrad_all;            /* [n_query_rows, dim], accumulated into */
  float* d_slots;              /* [n_segments * stride + n_query_rows] OUT */
  float* dsum_part;            /* [n_query_rows] OUT */
  float* loss_part;            /* [1] OUT, nullable */
  void* reduce_scratch;        /* rsa_scratch_bytes() bytes, zeroed once (with loss_part) */
  int64_t item_pad_row;
  void* workspace;
  int64_t workspace_bytes;
  int32_t keys_grouped;        /* != 0: the segments were routed with group_by_query (every query's elements for this owner are
                                  one contiguous run of one segment): the sort by query is skipped */
  int32_t finish_parts;        /* rsa_shard_owner_bpr_finish only: 0 = all of it; 1 = the positives only (qgrad_all is complete
                                  after this call); 2 = only the sorted apply pass of the shared rows (after a call with 1).  A
                                  caller can then issue what depends on qgrad_all -- the reduce-scatter, the query tower's
                                  update -- on another stream, beside the apply pass */
  int32_t forward_parts;       /* rsa_shard_owner_bpr_forward only: 0 = all of it; 1 = only what reads nothing but the received
                                  keys and pos_rows -- the sort by row, the solo classification, the queries' runs -- into the
                                  workspace (q_all, pos_score, qgrad_all and the outputs may be null): a caller can issue it
                                  for the NEXT step, behind that step's key exchange, on another stream; 2 = the rest (update
                                  scales from the headers, then the pass over the rows) over a workspace a call with 1 filled */
  /* rsa_shard_owner_ssm_forward / _finish (ABI 9): */
  const float* logq_rows;      /* nullable [n_rows]: log-probability under the sampler of each LOCAL row's item (null: 0, the uniform sampler) */
  float* run_max;              /* [n_query_rows] OUT of the forward: max over this owner's slots of z = score - log q (-inf: none) */
  float* run_sum;              /* [n_query_rows] OUT: sum exp(z - run_max) */
  float* run_acc;              /* [n_query_rows, dim] OUT: sum exp(z - run_max) * row */
} rsa_shard_owner_bpr_args;
int rsa_shard_pos_score(const float* item_local, int64_t n_rows, int32_t dim, const float* q_all, int64_t n_query_rows,
                        int64_t* pos_rows, float* out, const int64_t* pos_ids, int64_t rows_per_shard, int32_t n_shards,
                        int32_t rank, rsa_stream_t stream);   /* pos_ids != NULL: GLOBAL ids in, pos_rows is written (the owner /
                                                                  local-row rule of rsa_shard_sample_route: rows_per_shard == 0 =
                                                                  interleaved rows); NULL: pos_rows is the input */
int rsa_shard_owner_bpr_forward(const rsa_shard_owner_bpr_args* args, rsa_stream_t stream);
int rsa_shard_owner_bpr_finish(const rsa_shard_owner_bpr_args* args, const float* dsum_all, rsa_stream_t stream);

/* SampledSoftmaxLoss (recstudio/model/loss_func.py:80-90, one positive per row) evaluated ON THE OWNERS of the negatives, for the
 * same routed step (positives not routed, pos_rows per rank): loss_q = logsumexp(z_pos, z_1 .. z_n) - z_pos with z = score -
 * log q spans all owners of a query's negatives, so the owner pass has two phases around an 8-byte-per-query all-reduce:
 *   rsa_shard_owner_ssm_forward  sort by row (in place, i.e. item_target == item_local: + the solo classification), the queries'
 *     runs, and ONE walk over the received negatives' rows: z per slot (d_slots), and per query over this owner's slots
 *     run_max = max z, run_sum = sum exp(z - run_max), run_acc = sum exp(z - run_max) * row (flash-attention style partials);
 *   [caller: m = max(z_pos, all-reduce-max(run_max)); s = all-reduce-sum(run_sum * exp(run_max - m));
 *            lse = m + log(s + exp(z_pos - m))]
 *   rsa_shard_owner_ssm_finish   (args.pos_score = z_pos) d = exp(z - lse) / mean_den per slot; qgrad_all += gate *
 *     exp(run_max - lse) / mean_den * run_acc -- the query gradient needs NO second pass over the rows --; the positives'
 *     owners add (softmax_pos - 1) / mean_den * row_pos; every touched item row gets gate * item_scale * sum d * q: into a
 *     gradient block through the sorted apply pass; in place, the rows ONE element of the step touches from a second walk by
 *     query (the query row in registers, d from the z phase 1 left per slot: no dot product, no query row per element) and
 *     only the rows several elements touch through the sorted apply pass -- 3 row transfers per negative and B query rows
 *     instead of one per element.
 * The loss itself is lse - z_pos on the caller's side.  No scores travel home, no score gradients travel back (8 instead of
 * 16 bytes per triplet over xGMI).  dims in {64, 128, 256}; same workspace as the BPR form. */
int rsa_shard_owner_ssm_forward(const rsa_shard_owner_bpr_args* args, rsa_stream_t stream);
int rsa_shard_owner_ssm_finish(const rsa_shard_owner_bpr_args* args, const float* lse_all, rsa_stream_t stream);

/* Placement probe (no reference counterpart: the reference allocates through torch and never looks).  On MI355X the same
 * launch runs 10-15 % slower when the buffers it WRITES live in certain physical regions of the HBM (per allocation, stable,
 * visible only under concurrent read load -- DESIGN.md 6, profiles/r05_output_placement.json).  This launch reproduces the
 * access pattern of the fused forward without its arithmetic: per tile of 64 elements 64 random 512-byte rows read from
 * `source` (any resident buffer much larger than the 256 MB Infinity Cache; its contents do not matter) and 512 + 3 x 256 + 16
 * bytes written over `region` (four arrays at quarter offsets, at most 65536 tiles).  A caller times it (events on `stream`)
 * on candidate allocations and keeps the fastest: recstudio_amd/placement.py.  region: 256-byte aligned, >= 1 MiB, OVERWRITTEN. */
int rsa_placement_probe(void* region, int64_t region_bytes, const void* source, int64_t source_bytes, uint32_t salt,
                        rsa_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* RECSTUDIO_AMD_H */
