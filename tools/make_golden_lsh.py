"""Record tests/golden/lsh.npz from the reference's own LSHSampler (CPU, fp32).

Usage:  python tools/make_golden_lsh.py        (needs the reference checkout that oracle/make_golden.py imports)

The fixture is data only.  Two cases, as (N, d, n_bits, n_table, B, num_neg):

    a   (300, 16, 4, 5, 5, 7)     every query has a bucket
    b   (41, 16, 8, 3, 64, 5)     256 buckets for 41 items: some queries find all three of theirs empty, some do not

Each records weight_vectors, item_embs, query, pos, the indptr / indices that ``update`` leaves, the uniforms of the
``torch.rand(B, num_neg)`` call inside ``forward`` (captured by wrapping ``torch.rand``), and the three outputs of
``forward(query, num_neg, pos)``.  The seed of a case is the first for which the float64 referee (tests/lsh_referee.py) calls
every sign bit of every row and query decided, so the recorded codes do not hinge on anyone's rounding.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
OUT = os.path.join(ROOT, 'tests', 'golden', 'lsh.npz')
CASES = {'a': (300, 16, 4, 5, 5, 7), 'b': (41, 16, 8, 3, 64, 5)}


def record(S, name, shape, seed):
    import lsh_referee as R
    N, d, K, L, B, n = shape
    torch.manual_seed(seed)
    s = S.LSHSampler(N + 1, d, K, L, device='cpu')
    g = torch.Generator().manual_seed(seed + 1)
    item_embs = torch.randn(N, d, generator=g)
    query = torch.randn(B, d, generator=g)
    pos = torch.randint(1, N + 1, (B,), generator=g)
    W = s.weight_vectors.detach()
    if not (bool(R.projections(item_embs, W)[1].all()) and bool(R.projections(query, W)[1].all())):
        return None
    s.update(item_embs)
    drawn = []
    orig = torch.rand

    def rand(*a, **k):
        t = orig(*a, **k)
        drawn.append(t.clone())
        return t
    torch.rand = rand
    try:
        torch.manual_seed(seed + 2)
        lp, neg, lnp = s.forward(query, n, pos)
    finally:
        torch.rand = orig
    assert len(drawn) == 1 and tuple(drawn[0].shape) == (B, n)
    qc, _ = R.hash_codes(query, W)
    ln = R.buckets(qc, s.indptr)[2]
    if name == 'b' and not (bool((ln == 0).any()) and bool((ln > 0).any())):
        return None
    if name == 'a' and bool((ln == 0).any()):
        return None
    from oracle.make_golden import np_
    return {f'{name}.{k}': np_(v) for k, v in dict(
        weight_vectors=W, item_embs=item_embs, query=query, pos=pos, indptr=s.indptr, indices=s.indices, u=drawn[0], neg=neg,
        log_neg_prob=lnp, log_pos_prob=lp, shape=np.asarray(shape), seed=np.asarray(seed)).items()}


def main():
    from oracle.make_golden import import_reference
    S = import_reference()[0]
    out = {}
    for name, shape in CASES.items():
        for seed in range(1000, 1100):
            got = record(S, name, shape, seed)
            if got is not None:
                out.update(got)
                print('case', name, 'seed', seed)
                break
        else:
            raise SystemExit(f'case {name}: no seed without an undecided bit')
    np.savez_compressed(OUT, **out)
    print('wrote', OUT, os.path.getsize(OUT), 'bytes,', len(out), 'arrays')


if __name__ == '__main__':
    main()
