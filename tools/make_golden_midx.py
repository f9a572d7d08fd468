"""Record tests/golden/midx.npz from the reference's own MIDXSamplerUniform / ClusterSamplerUniform (CPU, fp32).

Usage:  python tools/make_golden_midx.py        (needs the reference checkout that oracle/make_golden.py imports)

The fixture is data only: the inputs, every attribute the reference's ``update`` leaves behind, its ``compute_item_p`` and one
recorded ``forward``.  Cases (N = 301 with the padding id, d = 16, K = 4):

    midx_ip_30, midx_cos_30, cluster_ip_30      update(max_iter=30): the loop stops on its own
    midx_ip_2,  midx_cos_2,  cluster_ip_2       update(max_iter=2):  the loop runs out
    cluster_dead                                one initial centre far from every point, re-seeded under torch.manual_seed(7)

Initial centres are injected (``s.c0`` / ``s.c1``; the reference's ClusterSamplerUniform always passes K to ``kmeans``, so for
it ``kmeans`` is wrapped to receive the injected ``c`` instead).
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, 'tests', 'golden', 'midx.npz')
N_ITEMS, D, K, B, NUM_NEG = 300, 16, 4, 5, 7


def main():
    from oracle.make_golden import import_reference, np_
    S, scorer = import_reference()[:2]
    g = torch.Generator().manual_seed(20240)
    blobs = torch.randn(6, D, generator=g) * 1.5
    item_embs = blobs[torch.randint(0, 6, (N_ITEMS,), generator=g)] + 0.6 * torch.randn(N_ITEMS, D, generator=g)
    query = torch.randn(B, D, generator=g)
    pos1 = torch.randint(1, N_ITEMS + 1, (B,), generator=g)
    pos2 = torch.randint(1, N_ITEMS + 1, (B, 3), generator=g)
    pos1[1] = 0
    pos2[0, 2] = 0
    pos2[3, 0] = 0
    init_rows = item_embs[torch.randperm(N_ITEMS, generator=g)[:2 * K]]
    init_cos = torch.nn.functional.normalize(init_rows, dim=-1)
    out = dict(item_embs=np_(item_embs), query=np_(query), pos1=np_(pos1), pos2=np_(pos2), init_rows=np_(init_rows),
               init_cos=np_(init_cos))

    def record(name, s, names):
        for a in names:
            out[f'{name}.{a}'] = np_(getattr(s, a))
        out[f'{name}.p1'] = np_(s.compute_item_p(query_of(s), pos1))
        out[f'{name}.p2'] = np_(s.compute_item_p(query_of(s), pos2))

    def query_of(s):            # compute_item_p takes the query as forward hands it over: normalised for the cosine scorer
        return torch.nn.functional.normalize(query, dim=-1) if isinstance(s.scorer, scorer.CosineScorer) else query

    midx_names = ('c0', 'c1', 'c0_', 'c1_', 'cd0', 'cd1', 'indices', 'indptr', 'wkk')
    clu_names = ('c', 'c_', 'cd', 'indices', 'indptr', 'wkk')
    for it in (30, 2):
        for tag, sc, init in (('ip', scorer.InnerProductScorer(), init_rows), ('cos', scorer.CosineScorer(), init_cos)):
            s = S.MIDXSamplerUniform(N_ITEMS + 1, K, sc)
            s.c0, s.c1 = init[:K, :D // 2].clone(), init[K:, D // 2:].clone()
            s.update(item_embs, max_iter=it)
            record(f'midx_{tag}_{it}', s, midx_names)
            if tag == 'ip' and it == 30:
                torch.manual_seed(3)
                lp, neg, lnp = s.forward(query, NUM_NEG, pos2)
                out['forward.neg'], out['forward.neg_prob'], out['forward.pos_prob'] = np_(neg), np_(lnp), np_(lp)
        out['cluster_init'] = np_(init_rows[:K])

    orig = S.kmeans

    def run_cluster(name, init, it, seed=None):
        S.kmeans = lambda X, K_or_c, max_iter: orig(X, init.clone(), max_iter)
        try:
            s = S.ClusterSamplerUniform(N_ITEMS + 1, K, scorer.InnerProductScorer())
            if seed is not None:
                torch.manual_seed(seed)
            s.update(item_embs, max_iter=it)
        finally:
            S.kmeans = orig
        record(name, s, clu_names)

    run_cluster('cluster_ip_30', init_rows[:K], 30)
    run_cluster('cluster_ip_2', init_rows[:K], 2)
    dead = init_rows[:K].clone()
    dead[2] = 1000.0
    out['cluster_dead_init'] = np_(dead)
    run_cluster('cluster_dead', dead, 30, seed=7)
    np.savez_compressed(OUT, **out)
    print('wrote', OUT, os.path.getsize(OUT), 'bytes,', len(out), 'arrays')


if __name__ == '__main__':
    main()
