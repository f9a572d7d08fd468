"""Times the ItemKNN neighbour build (ops.knn_build, rsa_knn.hip) and one top-k batch (ops.knn_score + ops.row_topk) against their
torch-op twins (models_mf.itemknn_torch: dense R^T R in column chunks, the formula, a stable sort; itemknn_score_torch + torch.topk).
One process, one device, the arms alternating, device events around every call, warm-up first, medians; a streaming copy of 1 GiB
is timed at the start and at the end as the record of the box's state.  Prints one JSON object and writes it to
profiles/itemknn_bench.json.

    python tools/bench_itemknn.py [--reps 5 --warmup 1 --knn 100 --batch 512 --k 100]

Data: dataset.synthetic_interactions (users uniform, items Zipf(1)), repeated pairs dropped, at two shapes: about ml-1m
(6040 users, 3706 items, 1e6 draws) and about ml-20m (138493 users, 26744 items, 2e7 draws).  ``heaviest``: the item with the largest
work sum_{u in users(i)} deg(u) is ONE workgroup per tile; its build alone is timed (a plan of that one item) and reported as a
share of the whole build, next to its share of the work.  ``fused_wins_at_the_larger_shape`` is the rule behind
models_mf.FUSED_KNN_DEFAULT: both the build and the top-k batch ahead by more than 15 %."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

from bench_gru import copy_gbps                      # noqa: E402
from graph_bench import peak_above, row, timed       # noqa: E402

SHAPES = {'ml-1m': (6040, 3706, 1_000_000), 'ml-20m': (138_493, 26_744, 20_000_000)}
MARGIN = 1.15


def shape(ops, mf, dataset, name, a, dev):
    n_users, n_items, draws = SHAPES[name]
    u, i = (torch.from_numpy(t) for t in dataset.synthetic_interactions(n_users, n_items, draws, alpha=1.0))
    U, N = n_users + 1, n_items + 1
    pair = torch.unique(u * N + i).to(dev)                                  # sorted: the user-side CSR with ascending ids
    u, i = pair // N, pair % N
    by_item = torch.sort(i * U + u).values
    u_indptr = torch.cat([u.new_zeros(1), torch.cumsum(torch.bincount(u, minlength=U), 0)])
    i_indptr = torch.cat([u.new_zeros(1), torch.cumsum(torch.bincount(i, minlength=N), 0)])
    u_items, i_users = i.to(torch.int32), (by_item % U).to(torch.int32)
    plan = ops.knn_plan(u_indptr, i_indptr, i_users)
    head = ops.KnnPlan(plan.order[:1], plan.weight, plan.max_degree)
    out = dict(shape=name, users=U, items=N, interactions=int(pair.numel()), knn=a.knn, similarity='cosine', targets=int(plan.order.numel()),
               max_degree=plan.max_degree, heaviest=dict(item=int(plan.order[0]), share_of_work=plan.heaviest_share()))

    def fused_build(p=plan):
        return ops.knn_build(u_indptr, u_items, i_indptr, i_users, a.knn, 'cosine', plan=p)

    def twin_build():
        return mf.itemknn_torch(u, i, U, N, a.knn, 'cosine')
    ms = timed([fused_build, twin_build, lambda: fused_build(head)], a.reps, a.warmup)
    out['build'] = dict(fused=row(ms[0]), twin=row(ms[1]), heaviest_alone=row(ms[2]))
    out['build']['twin_over_fused'] = out['build']['twin']['ms'] / out['build']['fused']['ms']
    out['heaviest']['share_of_build_time'] = out['build']['heaviest_alone']['ms'] / out['build']['fused']['ms']
    out['build']['peak_bytes'] = dict(fused=peak_above(fused_build), twin=peak_above(twin_build))
    nbr = fused_build()
    t_lists = ops.knn_transpose(*nbr)
    users = torch.randint(1, U, (a.batch,), device=dev, generator=torch.Generator(device=dev).manual_seed(1))

    def fused_topk():
        return ops.row_topk(ops.knn_score(users, u_indptr, u_items, *t_lists, N), a.k)

    def twin_topk():
        return torch.topk(mf.itemknn_score_torch(users, u_indptr, u_items, *t_lists, N), a.k)
    ms = timed([fused_topk, twin_topk], a.reps, a.warmup)
    out['topk'] = dict(batch=a.batch, k=a.k, fused=row(ms[0]), twin=row(ms[1]))
    out['topk']['twin_over_fused'] = out['topk']['twin']['ms'] / out['topk']['fused']['ms']
    out['topk']['peak_bytes'] = dict(fused=peak_above(fused_topk), twin=peak_above(twin_topk))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--knn', type=int, default=100)
    ap.add_argument('--batch', type=int, default=512)
    ap.add_argument('--k', type=int, default=100)
    ap.add_argument('--shapes', default='ml-1m,ml-20m')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'itemknn_bench.json'))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_itemknn.py measures on the GPU: none found')
    from recstudio_amd import dataset, models_mf, ops
    dev = torch.device('cuda')
    props = torch.cuda.get_device_properties(0)
    res = dict(device=props.name, compute_units=props.multi_processor_count, torch=torch.__version__, reps=a.reps, warmup=a.warmup,
               tile=ops.KNN_MAX_TILE, margin=MARGIN, copy_gb_per_s_before=copy_gbps(dev), shapes=[])
    for name in a.shapes.split(','):
        res['shapes'].append(shape(ops, models_mf, dataset, name, a, dev))
        print(json.dumps(res['shapes'][-1]), file=sys.stderr, flush=True)
        torch.cuda.empty_cache()
    last = res['shapes'][-1]
    res['fused_wins_at_the_larger_shape'] = last['build']['twin_over_fused'] > MARGIN and last['topk']['twin_over_fused'] > MARGIN
    res['copy_gb_per_s_after'] = copy_gbps(dev)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')
    print(json.dumps(res))


if __name__ == '__main__':
    main()
