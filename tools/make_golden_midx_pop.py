"""Record tests/golden/midx_pop.npz from the reference's own MIDXSamplerPop / ClusterSamplerPop (CPU, fp32).

Usage:  python tools/make_golden_midx_pop.py     (needs the reference checkout that oracle/make_golden.py imports)

The fixture is data only.  Inputs are those of tests/golden/midx.npz (``item_embs``, ``query``, ``pos1``, ``pos2``, ``init_rows``,
``init_cos``; N = 300, d = 16, K = 4) plus ``pop_counts``: 300 integer counts, one per item id 1 .. 300, some of them 0.  Cases:

    midx_pop_ip_m1       inner product, mode 1
    midx_pop_cos_m0      cosine, mode 0 (a count of 0 weighs 0: log p = -inf is recorded for such a positive)
    midx_pop_euc_m2      Euclidean, mode 2, item_embs and the initial centres times EUC_SCALE so that exp(-||x||^2 / 2) stays normal
    cluster_pop_ip_m1    inner product, mode 1
    cluster_pop_euc_m1   Euclidean, mode 1, unscaled rows (weights down to 1e-30)

Per case: every attribute the reference's ``update`` leaves behind (centres, cluster maps, ``indices``, ``indptr``, ``wkk``, ``p``,
``cp``) and its ``compute_item_p`` for ``pos1`` and ``pos2``.  Initial centres are injected as tools/make_golden_midx.py does.  The
reference's ``forward`` is NOT recorded: its in-bucket draw disagrees with its own ``compute_item_p``.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SRC = os.path.join(ROOT, 'tests', 'golden', 'midx.npz')
OUT = os.path.join(ROOT, 'tests', 'golden', 'midx_pop.npz')
K, EUC_SCALE = 4, 0.3


def main():
    from oracle.make_golden import import_reference, np_
    S, scorer = import_reference()[:2]
    z = np.load(SRC)
    item_embs, query, pos1, pos2, init_rows, init_cos = (torch.from_numpy(z[k]) for k in
                                                         ('item_embs', 'query', 'pos1', 'pos2', 'init_rows', 'init_cos'))
    N, D = item_embs.shape
    g = torch.Generator().manual_seed(20241)
    counts = torch.randint(1, 60, (N,), generator=g)
    counts[torch.randperm(N, generator=g)[:25]] = 0
    zero_pos = int(pos2[pos2 > 0][0])
    counts[zero_pos - 1] = 0                                  # a positive id of weight 0 under mode 0
    out = dict(pop_counts=np_(counts), euc_scale=np.float32(EUC_SCALE))

    def record(name, s, names):
        for a in names:
            out[f'{name}.{a}'] = np_(getattr(s, a))
        q = torch.nn.functional.normalize(query, dim=-1) if isinstance(s.scorer, scorer.CosineScorer) else query
        out[f'{name}.p1'] = np_(s.compute_item_p(q, pos1))
        out[f'{name}.p2'] = np_(s.compute_item_p(q, pos2))
        assert s.p.shape == (N + 1,) and s.cp.shape == (N,)
        assert not bool(torch.isnan(s.cp).any()), f'{name}: a bucket of weight 0 (NaN in cp): choose other counts'

    midx_names = ('c0', 'c1', 'cd0', 'cd1', 'indices', 'indptr', 'wkk', 'p', 'cp')
    clu_names = ('c', 'cd', 'indices', 'indptr', 'wkk', 'p', 'cp')
    for name, sc, mode, init, scale in (('midx_pop_ip_m1', scorer.InnerProductScorer(), 1, init_rows, 1.0),
                                        ('midx_pop_cos_m0', scorer.CosineScorer(), 0, init_cos, 1.0),
                                        ('midx_pop_euc_m2', scorer.EuclideanScorer(), 2, init_rows, EUC_SCALE)):
        s = S.MIDXSamplerPop(counts.clone(), K, sc, mode=mode)
        s.c0, s.c1 = init[:K, :D // 2].clone() * scale, init[K:, D // 2:].clone() * scale
        s.update(item_embs * scale, max_iter=30)
        record(name, s, midx_names)
    assert bool(torch.isinf(torch.from_numpy(out['midx_pop_cos_m0.p2'])).any()), 'no positive id of weight 0 in the mode-0 case'

    orig = S.kmeans
    for name, sc in (('cluster_pop_ip_m1', scorer.InnerProductScorer()), ('cluster_pop_euc_m1', scorer.EuclideanScorer())):
        S.kmeans = lambda X, K_or_c, max_iter: orig(X, init_rows[:K].clone(), max_iter)
        try:
            s = S.ClusterSamplerPop(counts.clone(), K, sc, mode=1)
            s.update(item_embs, max_iter=30)
        finally:
            S.kmeans = orig
        record(name, s, clu_names)
    np.savez_compressed(OUT, **out)
    print('wrote', OUT, os.path.getsize(OUT), 'bytes,', len(out), 'arrays')


if __name__ == '__main__':
    main()
