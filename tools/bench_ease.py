"""Times the EASE fit (ops.ease_gram -> spd_inverse -> ease_weights, rsa_ease.hip) and one score batch (ops.ease_score) against torch
on the device: torch.linalg.inv and torch.linalg.cholesky + torch.cholesky_inverse of the same float64 Gram matrix, and the dense
R[users] @ B.  One process, one device, the arms alternating, device events around every call, warm-up first, medians; a streaming
copy of 1 GiB is timed at the start and at the end as the record of the box's state.  Prints one JSON object and writes it to
profiles/ease_bench.json.

    python tools/bench_ease.py [--reps 3 --warmup 1 --batch 512 --shapes ml-1m,ml-20m,n24576]

Data: dataset.synthetic_interactions (users uniform, items Zipf(1)), repeated pairs dropped: about ml-1m (6040 x 3706, 1e6 draws),
about ml-20m (138493 x 20000, 2e7 draws) and N = 24576 (P is 4.8 GB: byte offsets pass 4 GiB; there the torch arms and the score
are left out and the inverse is checked by max |G P e_j - e_j| on 16 sampled columns).  ``inverse_share_of_fp64_floor``: 2 n^3
flops at 78 TF/s over the measured time.  ``score_share_of_byte_floor``: the B rows a batch reads (8 N bytes per history item) at
the measured copy rate over the measured time.  ``fused_wins``: the fused fit ahead of the better torch arm that ran; FUSED_EASE_DEFAULT is
on only if that holds at both named shapes."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

from bench_gru import copy_gbps                      # noqa: E402
from graph_bench import row, timed                   # noqa: E402

SHAPES = {'ml-1m': (6040, 3706, 1_000_000), 'ml-20m': (138_493, 20_000, 20_000_000), 'n24576': (138_493, 24_575, 20_000_000)}
FP64_MATRIX_FLOPS = 78e12
LAM = 250.0


def shape(ops, dataset, name, a, dev, gbps):
    n_users, n_items, draws = SHAPES[name]
    u, i = (torch.from_numpy(t) for t in dataset.synthetic_interactions(n_users, n_items, draws, alpha=1.0))
    U, N = n_users + 1, n_items + 1
    pair = torch.unique(u * N + i).to(dev)
    u, i = pair // N, pair % N
    by_item = torch.sort(i * U + u).values
    u_indptr = torch.cat([u.new_zeros(1), torch.cumsum(torch.bincount(u, minlength=U), 0)])
    i_indptr = torch.cat([u.new_zeros(1), torch.cumsum(torch.bincount(i, minlength=N), 0)])
    u_items, i_users = i.to(torch.int32), (by_item % U).to(torch.int32)
    big = name == 'n24576'
    out = dict(shape=name, users=U, items=N, interactions=int(pair.numel()), lam=LAM)

    def gram():
        return ops.ease_gram(u_indptr, u_items, i_indptr, i_users, LAM)
    G = gram()

    def inverse():
        return ops.spd_inverse(G.clone(), overwrite=True)[0]

    def fit():
        return ops.ease_weights(ops.spd_inverse(gram(), overwrite=True)[0], LAM, overwrite=True)

    def torch_inv():
        return torch.linalg.inv(G)

    def torch_chol():
        return torch.cholesky_inverse(torch.linalg.cholesky(G))
    P = inverse()

    def weights():
        return ops.ease_weights(P, LAM)
    arms = dict(gram=gram, inverse=inverse, weights=weights, fit=fit)
    for key, fn in (() if big else (('torch_inv', torch_inv), ('torch_cholesky_inverse', torch_chol))):
        try:                                                            # a torch arm that cannot run at this size is reported, not timed
            fn()
            arms[key] = fn
        except RuntimeError as e:
            out.setdefault('torch_arm_failed', {})[key] = str(e).splitlines()[0][:200]
    ms = timed(list(arms.values()), a.reps, a.warmup)
    out['fit'] = {k: row(t) for k, t in zip(arms, ms)}
    out['inverse_share_of_fp64_floor'] = 2.0 * N ** 3 / FP64_MATRIX_FLOPS * 1e3 / out['fit']['inverse']['ms']
    cols = torch.arange(16, device=dev) * (N // 16) + 1
    E = torch.zeros(N, 16, dtype=torch.float64, device=dev)
    E[cols, torch.arange(16, device=dev)] = 1
    out['inverse_residual_16_columns'] = float((G @ P[:, cols] - E).abs().max())
    if not big:
        torch_ms = [out['fit'][k]['ms'] for k in ('torch_inv', 'torch_cholesky_inverse') if k in out['fit']]
        out['fused_wins'] = bool(torch_ms) and out['fit']['fit']['ms'] < min(torch_ms)
        B = ops.ease_weights(P, LAM)[0]
        users = torch.randint(1, U, (a.batch,), device=dev, generator=torch.Generator(device=dev).manual_seed(1))
        R = torch.zeros(a.batch, N, dtype=torch.float64, device=dev)
        deg = u_indptr[users + 1] - u_indptr[users]
        for b in range(a.batch):
            R[b, u_items[u_indptr[users[b]]:u_indptr[users[b] + 1]].long()] = 1
        ms = timed([lambda: ops.ease_score(users, u_indptr, u_items, B), lambda: (R @ B[:, 1:]).float()], a.reps, a.warmup)
        out['score'] = dict(batch=a.batch, history_items=int(deg.sum()), fused=row(ms[0]), dense=row(ms[1]))
        out['score_share_of_byte_floor'] = float(deg.sum()) * N * 8 / (gbps * 1e9) * 1e3 / out['score']['fused']['ms']
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--batch', type=int, default=512)
    ap.add_argument('--shapes', default='ml-1m,ml-20m,n24576')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'ease_bench.json'))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_ease.py measures on the GPU: none found')
    from recstudio_amd import dataset, ops
    dev = torch.device('cuda')
    props = torch.cuda.get_device_properties(0)
    gbps = copy_gbps(dev)
    res = dict(device=props.name, compute_units=props.multi_processor_count, torch=torch.__version__, reps=a.reps, warmup=a.warmup,
               fp64_matrix_flops=FP64_MATRIX_FLOPS, copy_gb_per_s_before=gbps, shapes=[])
    for name in a.shapes.split(','):
        res['shapes'].append(shape(ops, dataset, name, a, dev, gbps))
        print(json.dumps(res['shapes'][-1]), file=sys.stderr, flush=True)
        torch.cuda.empty_cache()
    named = [s for s in res['shapes'] if 'fused_wins' in s]
    res['fused_wins_at_both_named_shapes'] = len(named) >= 2 and all(s['fused_wins'] for s in named)
    res['copy_gb_per_s_after'] = copy_gbps(dev)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')
    print(json.dumps(res))


if __name__ == '__main__':
    main()
