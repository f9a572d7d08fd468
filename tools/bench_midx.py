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
weighted: the popularity-in-bucket draw (MIDXSamplerPop: cp / item_logp given)  vs  the uniform draw of the same library  vs  the
          uniform draw of ANOTHER build of the library (--parent-lib, e.g. the parent commit's, built into a second directory with
          tools/build_variant.sh or its own make) loaded into the same process  vs  the corrected weighted draw with torch ops
          (the codebook stages as above, then one searchsorted over the bucket-offset CDF and two gathers) -- all four alternating.
weights : rsa_midx_weights (p, log p, wkk, cp of one epoch)  vs  the reference's loop over the K^2 buckets with torch ops
          (sampler.py:413-423: a cumsum and a division per bucket), and the same kernel for a Cluster index of K = 2 (two buckets of
          N / 2 items, one workgroup each) next to one Lloyd pass of that codebook.
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


def torch_weighted_draw(q, book0, book1, wkk, indptr, indices, cp_keyed, logp, n):
    """The corrected popularity-in-bucket draw with torch ops: the two codebook stages of ``torch_draw`` from the weighted wkk, then
    the first position of the bucket whose cp exceeds the uniform -- one searchsorted over ``cp_keyed`` = cp + 2 * (bucket of the
    position), which is sorted over the whole table -- the id there and its log-weight."""
    clusters, half = wkk.shape[0], q.shape[1] // 2
    logit0 = torch.mm(q[:, :half], book0.t())
    logit1 = torch.mm(q[:, half:], book1.t())
    pr0, pr1 = logit0.softmax(dim=1), logit1.softmax(dim=1)
    marginal = pr0 * torch.nn.functional.linear(pr1, wkk)
    first = torch.multinomial(marginal, n, replacement=True)
    conditional = (wkk[first] * pr1[:, None, :]).flatten(0, 1)
    second = torch.multinomial(conditional, 1).view_as(first)
    bucket = first * clusters + second
    u = torch.rand(bucket.shape, device=q.device, dtype=torch.float64)
    pos = torch.searchsorted(cp_keyed, u + 2.0 * bucket, right=True)
    pos = torch.minimum(pos, indptr[bucket + 1] - 1)
    ids = indices[pos] + 1
    return ids, logit0.gather(1, first) + logit1.gather(1, second) + logp[ids]


def torch_weights(w, indices, indptr_host, bucket_of_pos, n_buckets):
    """The reference's _update with torch ops (sampler.py:413-423): p, the weighted wkk and the per-bucket cumsum / total loop
    (the bucket bounds as host integers: no device read-back inside the loop)."""
    p = torch.cat([w.new_ones(1), w])
    cp = w[indices]
    wkk = torch.zeros(n_buckets, dtype=w.dtype, device=w.device).index_add_(0, bucket_of_pos, cp)
    for b in range(n_buckets):
        start, end = indptr_host[b], indptr_host[b + 1]
        if end > start:
            run = cp[start:end].cumsum(0)
            cp[start:end] = run / run[-1]
    return p, torch.log(p), wkk, cp


def parent_sampler(path):
    """``midx_sample`` of another build of the library (the argument block is versioned: an older build reads the fields it knows)."""
    import ctypes
    from recstudio_amd import _native as nat, ops, rng
    lib = ctypes.CDLL(path)
    lib.rsa_midx_sample.restype = ctypes.c_int
    lib.rsa_midx_sample.argtypes = [ctypes.POINTER(nat.MidxArgs), ctypes.c_void_p]

    def sample(query, centres, wkk, indptr, indices, cd, n):
        a, out = ops._midx_args(query, centres, wkk, indptr, indices, cd, n, None, False, 'parent midx_sample')
        pc = rng.reserve(a.n_queries * a.num_neg * (a.n_parts + 1), 4, query.device, None)
        a.seed, a.offset, a.grid_threads, a.elem_base = pc.seed, pc.offset, pc.grid_threads, pc.elem_base
        rc = lib.rsa_midx_sample(ctypes.byref(a), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        if rc != 0:
            raise RuntimeError(f'parent rsa_midx_sample: status {rc}')
        return out
    return sample


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--items', type=int, default=10_000_000)
    ap.add_argument('--dim', type=int, default=128)
    ap.add_argument('--clusters', type=int, default=64)
    ap.add_argument('--queries', type=int, default=65536)
    ap.add_argument('--neg', type=int, default=64)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--parent-lib', default=None, help="another build of librecstudio_amd.so: its uniform draw is timed in the same run")
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
    del s, ids
    torch.cuda.empty_cache()

    # ---- the popularity-in-bucket form: the tables of one epoch, then the four draws
    def row(t):
        return dict(ms=t[0], ms_min_max=t[1:])
    counts = torch.randint(0, 50, (N,), device=dev)
    sp = ra.MIDXSamplerPop(counts, K, ra.InnerProductScorer(), mode=1)
    sp.c0, sp.c1 = centres[0].clone(), centres[1].clone()
    sp.update(X, max_iter=1)
    pop = sp.pop_count.detach()
    bucket_of_pos = torch.repeat_interleave(torch.arange(K * K, device=dev), sp.indptr[1:] - sp.indptr[:-1])
    indptr_host = sp.indptr.tolist()
    k_t, t_t = timed([lambda: ops.midx_weights(pop, sp._indptr32, sp._indices32, K, 2),
                      lambda: torch_weights(pop, sp.indices, indptr_host, bucket_of_pos, K * K)], a.reps)
    res['weights'] = dict(kernel=row(k_t), torch_bucket_loop=row(t_t), speedup=t_t[0] / k_t[0], buckets=K * K)
    uniform_wkk = (sp.indptr[1:] - sp.indptr[:-1]).to(torch.float32)
    state_u = (sp._centres, uniform_wkk, sp._indptr32, sp._indices32, sp._cd32)
    state_w = (sp._centres, sp._wkk_dev, sp._indptr32, sp._indices32, sp._cd32)
    cp_keyed = sp.cp.double() + 2.0 * bucket_of_pos
    fns = [lambda: ops.midx_sample(q, *state_w, n, cp=sp.cp, item_logp=sp._logp), lambda: ops.midx_sample(q, *state_u, n),
           lambda: torch_weighted_draw(q, sp.c0, sp.c1, sp.wkk, sp.indptr, sp.indices, cp_keyed, sp._logp, n)]
    names = ['weighted', 'uniform', 'torch_weighted']
    if a.parent_lib:
        parent = parent_sampler(a.parent_lib)
        fns.append(lambda: parent(q, *state_u, n))
        names.append('uniform_parent_build')
    times = timed(fns, a.reps)
    res['draw_weighted'] = {k_: row(t) for k_, t in zip(names, times)}
    res['draw_weighted']['speedup_over_torch'] = times[2][0] / times[0][0]
    if a.parent_lib:
        band = times[3][2] - times[3][1]
        res['draw_weighted']['uniform_minus_parent_ms'] = times[1][0] - times[3][0]
        res['draw_weighted']['parent_band_ms'] = band
        res['draw_weighted']['uniform_within_parent_band'] = bool(times[1][0] - times[3][0] <= band)
    del sp, cp_keyed, bucket_of_pos
    torch.cuda.empty_cache()

    # ---- Cluster, K = 2: two buckets of about N / 2 items, one workgroup each, next to one Lloyd pass of that codebook
    c2 = X[torch.randperm(N, device=dev)[:2]].unsqueeze(0).contiguous()
    sc = ra.ClusterSamplerPop(counts, 2, ra.InnerProductScorer(), mode=1)
    sc.c = c2[0].clone()
    sc.update(X, max_iter=1)
    k_t, l_t = timed([lambda: ops.midx_weights(pop, sc._indptr32, sc._indices32, 2, 1), lambda: ops.kmeans_step(X, c2)], a.reps)
    res['weights_cluster_k2'] = dict(kernel=row(k_t), lloyd_pass_same_codebook=row(l_t),
                                     bucket_sizes=(sc.indptr[1:] - sc.indptr[:-1]).tolist())
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')
    print(json.dumps(res))


if __name__ == '__main__':
    main()
