"""Times the SLIM fit on the device: the fused arm (ops.ease_gram -> ops.slim_fit, rsa_slim.hip) against the torch twin
(ops.ease_gram -> models_mf.slim_torch), Gram matrix included in both, at about ml-1m's shape and the reference's defaults
(alpha 1, l1_ratio 0.1, positive_only).  One process, one device, the arms alternating, device events around every call, warm-up
first, medians; a streaming copy of 1 GiB is timed at the start and at the end as the record of the box's state.  Further alphas
(more candidates per target: the workgroup kernel) are timed for the fused arm, and for the twin where --twin-alphas names them.
Where sklearn imports, the reference's host loop (ElasticNet.fit per target on a lil_matrix whose column is zeroed and restored,
selection='random') is timed on 64 evenly spaced targets and SCALED to all targets: ``sklearn_host_loop_scaled_ms`` is an estimate
from that sample, not a measurement of the whole loop.  Prints one JSON object and writes it to profiles/slim_bench.json.

    python tools/bench_slim.py [--reps 3 --warmup 1 --alphas 1,0.1 --twin-alphas 1]

Data: dataset.synthetic_interactions (users uniform, items Zipf(1)), repeated pairs dropped: 6040 x 3706, 1e6 draws.
``fused_wins``: the fused fit ahead of the twin at the reference's alpha; FUSED_SLIM_DEFAULT is on only if that holds."""
import argparse
import json
import os
import sys
import time
import warnings

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

from bench_gru import copy_gbps                      # noqa: E402
from graph_bench import row, timed                   # noqa: E402

N_USERS, N_ITEMS, DRAWS, L1_RATIO, SAMPLE = 6040, 3706, 1_000_000, 0.1, 64


def sklearn_loop(u, i, U, N, alpha):
    """Seconds of the reference's loop over SAMPLE targets, or None without sklearn / scipy."""
    try:
        import scipy.sparse as sp
        from sklearn.exceptions import ConvergenceWarning
        from sklearn.linear_model import ElasticNet
    except ImportError:
        return None
    X = sp.csr_matrix((torch.ones(u.numel(), dtype=torch.float64).numpy(), (u.cpu().numpy(), i.cpu().numpy())), shape=(U, N)).tolil()
    model = ElasticNet(alpha=alpha, l1_ratio=L1_RATIO, positive=True, fit_intercept=False, copy_X=False, precompute=True,
                       selection='random', max_iter=100, tol=1e-4)
    t0 = time.perf_counter()
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', category=ConvergenceWarning)
        for j in range(1, N, (N - 1) // SAMPLE)[:SAMPLE]:
            r = X[:, j]
            X[:, j] = 0
            model.fit(X, r.toarray())
            model.sparse_coef_
            X[:, j] = r
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--alphas', default='1,0.1')
    ap.add_argument('--twin-alphas', default='1')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'slim_bench.json'))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_slim.py measures on the GPU: none found')
    from recstudio_amd import dataset, ops
    from recstudio_amd.models_mf import slim_torch
    dev = torch.device('cuda')
    props = torch.cuda.get_device_properties(0)
    u, i = (torch.from_numpy(t) for t in dataset.synthetic_interactions(N_USERS, N_ITEMS, DRAWS, alpha=1.0))
    U, N = N_USERS + 1, N_ITEMS + 1
    pair = torch.unique(u * N + i).to(dev)
    u, i = pair // N, pair % N
    by_item = torch.sort(i * U + u).values
    u_indptr = torch.cat([u.new_zeros(1), torch.cumsum(torch.bincount(u, minlength=U), 0)])
    i_indptr = torch.cat([u.new_zeros(1), torch.cumsum(torch.bincount(i, minlength=N), 0)])
    u_items, i_users = i.to(torch.int32), (by_item % U).to(torch.int32)
    res = dict(device=props.name, compute_units=props.multi_processor_count, torch=torch.__version__, reps=a.reps, warmup=a.warmup,
               users=U, items=N, interactions=int(pair.numel()), l1_ratio=L1_RATIO, copy_gb_per_s_before=copy_gbps(dev), alphas=[])

    def gram():
        return ops.ease_gram(u_indptr, u_items, i_indptr, i_users, 0.0)
    twin_alphas = {float(x) for x in a.twin_alphas.split(',') if x}
    for alpha in (float(x) for x in a.alphas.split(',')):
        def fused():
            return ops.slim_fit(gram(), U, alpha, L1_RATIO)

        def twin():
            return slim_torch(gram(), U, alpha, L1_RATIO)
        nbr_id, nbr_w, nbr_cnt, n_iter = fused()
        count = ((gram() > alpha * L1_RATIO * U).sum(0) - (gram().diagonal() > alpha * L1_RATIO * U).long())[1:]
        out = dict(alpha=alpha, l1=alpha * L1_RATIO * U, candidates_max=int(count.max()), candidates_mean=float(count.float().mean()),
                   targets_above_64=int((count > 64).sum()), non_zeros=int(nbr_cnt.sum()), n_iter_max=int(n_iter.max()))
        arms = dict(gram=gram, fused=fused)
        if alpha in twin_alphas:
            arms['twin'] = twin
            B, n_twin = twin()
            live = nbr_id >= 0
            tgt = torch.arange(N, device=dev)[:, None].expand_as(nbr_id)[live]
            out['twin_n_iter_equal_share'] = float((n_twin[1:] == n_iter[1:]).float().mean())
            out['twin_max_abs_weight_gap'] = float((B[nbr_id[live].long(), tgt] - nbr_w[live]).abs().max()) if live.any() else 0.0
            out['twin_non_zeros'] = int((B != 0).sum())
        ms = timed(list(arms.values()), a.reps, a.warmup)
        out['ms'] = {k: row(t) for k, t in zip(arms, ms)}
        if 'twin' in arms:
            out['fused_wins'] = out['ms']['fused']['ms'] < out['ms']['twin']['ms']
        if alpha == 1.0:
            sec = sklearn_loop(u, i, U, N, alpha)
            if sec is not None:
                out['sklearn_host_loop_sample'] = dict(targets=SAMPLE, ms=sec * 1e3)
                out['sklearn_host_loop_scaled_ms'] = sec * 1e3 * (N - 1) / SAMPLE
        res['alphas'].append(out)
        print(json.dumps(out), file=sys.stderr, flush=True)
    res['fused_wins_at_the_reference_alpha'] = any(o.get('fused_wins') for o in res['alphas'] if o['alpha'] == 1.0)
    res['copy_gb_per_s_after'] = copy_gbps(dev)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')
    print(json.dumps(res))


if __name__ == '__main__':
    main()
