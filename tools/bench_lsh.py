"""Times the LSH sampler's two kernels next to the reference's op sequence for the same work (torch ops on the same device, in
the same run, alternating), and the given-ids forward they feed.  Prints one JSON object and writes it to
profiles/lsh_bench.json.

    python tools/bench_lsh.py [--items 10000000 --dim 128 --bits 4 --tables 16 --queries 65536 --neg 64 --reps 10]

hash    : one rsa_lsh_hash pass over N rows (64 * d FMAs per 4 d-byte row)  vs  the reference's update with torch ops (normalise,
          one [N, d] x [d, K L] matmul, the comparison and the [N, L, K] x [K] matmul of sampler.py:601-604).  The bytes the kernel
          has to read and the FMAs it has to issue are reported next to the time, with the time each would take alone at the
          chip's peak (8 TB/s of HBM; 256 CUs x 4 SIMDs x 32 lanes x 2.4 GHz fp32 FMAs): the larger of the two bounds it.
update  : LSHSampler.update as a whole: the hash pass, the snapshot copy and the per-table stable sort / bincount on torch.
draw    : rsa_lsh_sample at B queries x n negatives (ids + log-probs in one launch)  vs  the reference's forward with torch ops
          (sampler.py:624-662: hash the queries, two gathers over indptr, cumsum, rand, searchsorted, three gathers, the embedding
          gather [B, n, d], cosine_similarity, acos, the two powers and the log).
forward : ops.fused_forward with the drawn ids given, the launch the sampler's ids go to -- its gather of the same B * n rows
          is the request-bound floor the draw is reported against.
Times are device events around each call, --reps calls after 3 warm-up calls, the two sides of a comparison interleaved
(a, b, a, b, ...); the mean is reported, and the fastest and slowest call next to it as the spread."""
import argparse
import json
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
PEAK_HBM_BYTES_PER_S = 8e12
PEAK_FP32_FMA_PER_S = 256 * 4 * 32 * 2.4e9


def torch_hash(rows, W, base):
    """The reference's update up to the codes, with torch ops -> codes [N, L] float."""
    d, K, L = W.shape
    unit = rows / (torch.norm(rows, dim=1, keepdim=True) + 1e-10)
    y = (torch.matmul(unit, W.view(d, -1)).view(rows.shape[0], K, L) > 0).type(torch.float)
    return torch.matmul(y.transpose(1, 2), base)


def torch_draw(q, W, base, indptr, indices, snapshot, n):
    """The reference's forward with torch ops -> (ids [B, n], log-probabilities [B, n]); rows without a bucket are not patched."""
    d, K, L = W.shape
    code = torch_hash(q, W, base).transpose(0, 1).type(torch.long)                 # [L, B]
    start = torch.gather(indptr, 1, code)
    count = torch.gather(indptr, 1, code + 1) - start
    total = count.sum(dim=0)
    cum = count.cumsum(dim=0).T.contiguous()
    r = torch.floor(torch.rand((q.shape[0], n), device=q.device) * total.view(-1, 1)).type(torch.long)
    r = torch.minimum(r, (total - 1).clamp_min(0).view(-1, 1))
    table = torch.searchsorted(cum, r, right=True).clamp_max(L - 1)
    before = torch.where(table > 0, torch.gather(cum, 1, (table - 1).clamp_min(0)), torch.zeros_like(r))
    pos = (torch.gather(start.T, 1, table) + r - before).clamp(0, indices.shape[1] - 1)
    item = indices[table, pos]
    cos = torch.nn.functional.cosine_similarity(q.view(q.shape[0], 1, d), snapshot[item], dim=-1)
    p = 1 - torch.acos(cos) / math.pi
    weight = 1 - (1 - p ** K) ** L
    return item + 1, torch.log(weight / total.view(-1, 1) + 1e-12)


def main():
    from bench_midx import timed
    ap = argparse.ArgumentParser()
    ap.add_argument('--items', type=int, default=10_000_000)
    ap.add_argument('--dim', type=int, default=128)
    ap.add_argument('--bits', type=int, default=4)
    ap.add_argument('--tables', type=int, default=16)
    ap.add_argument('--queries', type=int, default=65536)
    ap.add_argument('--neg', type=int, default=64)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'lsh_bench.json'))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_lsh.py measures on the GPU: none found')
    import recstudio_amd as ra
    from recstudio_amd import ops
    dev = 'cuda'
    N, d, K, L, B, n = a.items, a.dim, a.bits, a.tables, a.queries, a.neg
    torch.manual_seed(0)
    weight = torch.randn(N + 1, d, device=dev) * 0.3
    weight[0] = 0
    X = weight[1:]
    s = ra.LSHSampler(N + 1, d, K, L, device=dev, scorer_fn=ra.InnerProductScorer())
    W, base = s.weight_vectors.detach(), s.K_base_vec.detach()
    res = dict(device=torch.cuda.get_device_name(0), items=N, dim=d, n_bits=K, n_table=L, queries=B, num_neg=n, reps=a.reps)

    def row(t):
        return dict(ms=t[0], ms_min_max=t[1:])

    # ---- hash pass and update
    k_t, t_t = timed([lambda: ops.lsh_hash(X, W), lambda: torch_hash(X, W, base)], a.reps)
    nbytes, fmas = N * d * 4, N * K * L * d
    hbm_ms, valu_ms = nbytes / PEAK_HBM_BYTES_PER_S * 1e3, fmas / PEAK_FP32_FMA_PER_S * 1e3
    res['hash'] = dict(kernel=row(k_t), torch=row(t_t), speedup=t_t[0] / k_t[0], rows=N, bytes_read=nbytes, gbps=nbytes / k_t[0] / 1e6,
                       fp32_fma=fmas, tfma_per_s=fmas / k_t[0] / 1e9, hbm_floor_ms=hbm_ms, valu_floor_ms=valu_ms,
                       bound='VALU' if valu_ms > hbm_ms else 'HBM')
    print('hash', res['hash']['kernel'], file=sys.stderr, flush=True)
    torch.cuda.empty_cache()
    (u_t,) = timed([lambda: s.update(X)], max(2, a.reps // 3), warmup=1)
    res['update'] = row(u_t)
    print('update', res['update'], file=sys.stderr, flush=True)
    res['extra_memory_bytes'] = dict(snapshot=N * d * 4, indices_int64_and_int32=L * N * 12, indptr=L * ((1 << K) + 1) * 12)

    # ---- draw
    q = torch.randn(B, d, device=dev) * 0.3
    state = (W, s._indptr32, s._indices32, s.item_embs)
    k_t, t_t = timed([lambda: ops.lsh_sample(q, *state, n, eps=1e-12),
                      lambda: torch_draw(q, W, base, s.indptr, s.indices, s.item_embs, n)], a.reps)
    out = ops.lsh_sample(q, *state, n, eps=1e-12, want_codes=True)
    total = (torch.gather(s.indptr, 1, out['codes'].long().T + 1) - torch.gather(s.indptr, 1, out['codes'].long().T)).sum(0)
    res['draw'] = dict(kernel=row(k_t), torch=row(t_t), speedup=t_t[0] / k_t[0], draws=B * n, rows_gathered=B * n,
                       queries_without_a_bucket=int((total == 0).sum()), mean_candidates_per_query=float(total.double().mean()))
    print('draw', res['draw']['kernel'], file=sys.stderr, flush=True)
    pos = torch.randint(1, N + 1, (B,), device=dev)
    ids = out['neg_ids']
    (fwd, *_), = timed([lambda: ops.fused_forward(weight, q, n, neg_ids=ids, pos_ids=pos)], a.reps)
    res['forward_given_ids_ms'] = fwd
    res['draw_over_forward_given_ids'] = k_t[0] / fwd
    res['sampler_share_of_sample_plus_forward'] = k_t[0] / (k_t[0] + fwd)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')
    print(json.dumps(res))


if __name__ == '__main__':
    main()
