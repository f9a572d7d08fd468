"""Times the adaptive samplers' two kernels next to the reference's op sequence for the same work (torch ops on the same
device, in the same run, alternating), and the given-ids forward they feed.  Prints one JSON object and writes it to
profiles/midx_bench.json.

    python tools/bench_midx.py [--items 10000000 --dim 128 --clusters 64 --queries 65536 --neg 64 --reps 10]

draw    : rsa_midx_sample at B queries x n negatives (ids + log-probs in one launch)  vs  the same draw with torch ops (two
          softmaxes, the first-stage marginal, torch.multinomial twice -- the second over [B * n, K] -- and the in-bucket draw),
          the work of the reference's MIDXSamplerUniform.forward (recstudio/ann/sampler.py:308-345).
lloyd   : one rsa_kmeans_step over N rows, two halves  vs  one k-means iteration with torch ops per half (the [N, K] distance and
          membership matrices of the reference's kmeans(), sampler.py:19-31), at the largest N (<= --items, halved on
          out-of-memory) where those fit; reported per row.
forward : ops.fused_forward with the drawn ids given, the launch the sampler's ids go to.
Times are device events around each call, --reps calls after 3 warm-up calls, the two sides of a comparison interleaved
(a, b, a, b, ...); the mean is reported, and the fastest and slowest call next to it as the spread."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fns, reps, warmup=3):
    """(mean, min, max) milliseconds per call of each function, the functions called in turn (a, b, a, b, ...)."""
    for _ in range(warmup):
        for f in fns:
            f()
    torch.cuda.synchronize()
    ms = [[] for _ in fns]
    for _ in range(reps):
        for i, f in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            f()
            b.record()
            b.synchronize()
            ms[i].append(a.elapsed_time(b))
    return [(sum(t) / reps, min(t), max(t)) for t in ms]


def torch_draw(q, book0, book1, wkk, indptr, indices, n):
    """The two-stage multinomial draw with torch ops: first-stage cluster from its marginal, second-stage cluster from the
    conditional row (a [B * n, K] multinomial), a uniform position inside the bucket -> (ids [B, n], log-proposal [B, n])."""
    clusters, half = wkk.shape[0], q.shape[1] // 2
    logit0 = torch.mm(q[:, :half], book0.t())
    logit1 = torch.mm(q[:, half:], book1.t())
    pr0, pr1 = logit0.softmax(dim=1), logit1.softmax(dim=1)
    marginal = pr0 * torch.nn.functional.linear(pr1, wkk)                       # [B, K]: sum over the second cluster
    first = torch.multinomial(marginal, n, replacement=True)                    # [B, n]
    conditional = (wkk[first] * pr1[:, None, :]).flatten(0, 1)                  # [B * n, K]
    second = torch.multinomial(conditional, 1).view_as(first)
    bucket = first * clusters + second
    lo = indptr[bucket]
    size = indptr[bucket + 1] - lo
    within = (torch.rand(bucket.shape, device=q.device) * size).to(torch.int64)
    return indices[lo + within] + 1, logit0.gather(1, first) + logit1.gather(1, second)


def torch_lloyd(rows, centres):
    """One k-means iteration with torch ops and [N, K] temporaries (squared distances, membership matrix)
    -> (new centres, assignment, loss)."""
    row_sq = rows.square().sum(dim=1, keepdim=True)
    d2 = torch.addmm(row_sq + centres.square().sum(dim=1), rows, centres.t(), alpha=-2.0)    # [N, K]
    nearest = d2.argmin(dim=1)
    member = torch.zeros_like(d2).scatter_(1, nearest[:, None], 1.0)                        # [N, K]
    inertia = (rows - centres.index_select(0, nearest)).square().sum()
    return torch.mm(member.t(), rows) / member.sum(dim=0)[:, None], nearest, inertia


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--items', type=int, default=10_000_000)
    ap.add_argument('--dim', type=int, default=128)
    ap.add_argument('--clusters', type=int, default=64)
    ap.add_argument('--queries', type=int, default=65536)
    ap.add_argument('--neg', type=int, default=64)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'midx_bench.json'))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_midx.py measures on the GPU: none found')
    import recstudio_amd as ra
    from recstudio_amd import ops
    dev = 'cuda'
    N, d, K, B, n = a.items, a.dim, a.clusters, a.queries, a.neg
    torch.manual_seed(0)
    weight = torch.randn(N + 1, d, device=dev) * 0.3
    weight[0] = 0
    X = weight[1:]
    centres = torch.stack([X[torch.randperm(N, device=dev)[:K], p * (d // 2):(p + 1) * (d // 2)] for p in range(2)]).contiguous()
    res = dict(device=torch.cuda.get_device_name(0), items=N, dim=d, clusters=K, queries=B, num_neg=n, reps=a.reps)

    # ---- Lloyd step
    n_torch = N
    while True:
        try:
            halves = [X[:n_torch, :d // 2], X[:n_torch, d // 2:]]
            torch_lloyd(halves[0], centres[0])
            break
        except torch.OutOfMemoryError:
            torch.cuda.empty_cache()
            n_torch //= 2
    k_t, t_t = timed([lambda: ops.kmeans_step(X, centres), lambda: [torch_lloyd(h, c) for h, c in zip(halves, centres)]], a.reps)
    ours, ref = k_t[0], t_t[0]
    res['lloyd'] = dict(kernel_ms=ours, kernel_ms_min_max=k_t[1:], torch_ms_min_max=t_t[1:], kernel_rows=N, kernel_ns_per_row=ours * 1e6 / N, torch_ms=ref, torch_rows=n_torch,
                        torch_ns_per_row=ref * 1e6 / n_torch, speedup_per_row=(ref / n_torch) / (ours / N),
                        kernel_bytes_read=N * d * 4, kernel_gbps=N * d * 4 / ours / 1e6)
    del halves
    torch.cuda.empty_cache()

    # ---- the codebook state of one update pass, then the draw
    s = ra.MIDXSamplerUniform(N + 1, K, ra.InnerProductScorer())
    s.c0, s.c1 = centres[0].clone(), centres[1].clone()
    s.update(X, max_iter=1)
    q = torch.randn(B, d, device=dev) * 0.3
    state = (s._centres, s._wkk_dev, s._indptr32, s._indices32, s._cd32)
    k_t, t_t = timed([lambda: ops.midx_sample(q, *state, n),
                      lambda: torch_draw(q, s.c0, s.c1, s.wkk, s.indptr, s.indices, n)], a.reps)
    ours, ref = k_t[0], t_t[0]
    res['draw'] = dict(kernel_ms=ours, kernel_ms_min_max=k_t[1:], torch_ms_min_max=t_t[1:], torch_ms=ref, speedup=ref / ours, draws=B * n)
    ids = ops.midx_sample(q, *state, n)['neg_ids']
    pos = torch.randint(1, N + 1, (B,), device=dev)
    (fwd, *_), = timed([lambda: ops.fused_forward(weight, q, n, neg_ids=ids, pos_ids=pos)], a.reps)
    res['forward_given_ids_ms'] = fwd
    res['sampler_share_of_sample_plus_forward'] = ours / (ours + fwd)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')
    print(json.dumps(res))


if __name__ == '__main__':
    main()
