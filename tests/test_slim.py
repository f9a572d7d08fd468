"""CPU: the SLIM referee against sklearn's own Gram solver in cyclic order, ``slim_torch`` against the referee, the candidate
restriction, the argument checks of ``rsa_slim_fit`` (they fire before any HIP call), the model's defaults and its names."""
import ctypes

import numpy as np
import pytest
import torch

import recstudio_amd as ra
import slim_referee as sr
from recstudio_amd import retriever

U, N, ALPHA, L1 = 40, 25, 0.05, 0.1
A, B = ALPHA * L1 * U, ALPHA * (1 - L1) * U
R = sr.make_R(U, N, 7).astype(np.float64)
G = R.T @ R


def test_referee_is_sklearn_cyclic_and_candidates_carry_the_problem():
    ElasticNet = pytest.importorskip('sklearn.linear_model').ElasticNet
    model = ElasticNet(alpha=ALPHA, l1_ratio=L1, selection='cyclic', precompute=True, positive=True, fit_intercept=False, max_iter=100,
                       tol=1e-4)
    counts = set()
    for j in range(1, N):
        X = R.copy()
        X[:, j] = 0
        model.fit(X, R[:, j])
        full = sr.enet_gram(G, j, A, B)
        assert np.abs(full[0] - model.coef_).max() <= 1e-12 and full[2] == model.n_iter_, j
        C = sr.candidates(G, j, A)
        part = sr.enet_gram(G, j, A, B, coords=C)
        assert np.array_equal(full[0], part[0]) and full[1:] == part[1:], j
        counts.add(len(C))
    assert min(counts) <= 1 and 5 <= max(counts) < N - 2              # the restriction really drops coordinates


@pytest.mark.parametrize('positive', [True, False])
def test_twin_is_the_referee(positive):
    W, n_iter = ra.slim_torch(torch.from_numpy(G), U, ALPHA, L1, positive)
    assert not W[:, 0].any() and not W[0].any() and not W.diagonal().any()
    for j in range(1, N):
        w, _, n = sr.enet_gram(G, j, A, B, positive)
        assert np.abs(W[:, j].numpy() - w).max() <= 1e-12 and int(n_iter[j]) == n, j
    assert positive or (W < 0).any()                                  # the unclamped rule is really exercised


def test_argument_checks_fire_before_any_hip_call():
    nat = ra._native
    lib = nat.lib()
    P = ctypes.c_void_p(256)
    base = dict(g=P, order_wave=P, order_group=P, nbr_id=P, nbr_w=P, nbr_cnt=P, n_iter=P, n_items=9, ld=10, n_wave=4, n_group=4,
                l1=1.0, l2=1.0, tol=1e-4, max_iter=100, cap=8)
    cases = [(b'size', dict(size=0)), (b'n_items = 1', dict(n_items=1)), (b'ld = 8', dict(ld=8)), (b'cap = 0', dict(cap=0)),
             (b'l2 = 0', dict(l2=0.0)), (b'l2 = -1', dict(l2=-1.0)), (b'l1 = -1', dict(l1=-1.0)), (b'max_iter = 0', dict(max_iter=0)),
             (b'alpha * l1_ratio * U', dict(cap=ra.ops.SLIM_MAX_CANDIDATES + 1)), (b'n_wave = 8', dict(n_wave=8))]
    cases += [(name.encode() + b' is null', {name: None}) for name in base if isinstance(base[name], ctypes.c_void_p)]
    for text, fields in cases:
        a = nat.SlimFitArgs()
        for k, v in {**base, **fields}.items():
            setattr(a, k, v)
        assert lib.rsa_slim_fit(ctypes.byref(a), None) == -1 and text in lib.rsa_last_error(), (text, lib.rsa_last_error())


def test_model_defaults_refusals_and_names():
    train = ra.SLIM().config['train']
    assert {k: train[k] for k in ('alpha', 'l1_ratio', 'positive_only', 'knn', 'epochs')} == \
        {'alpha': 1, 'l1_ratio': 0.1, 'positive_only': True, 'knn': 100, 'epochs': 1}
    assert ra.SLIM().config['model']['fused_slim'] is retriever.FUSED_SLIM_DEFAULT
    assert 'SLIM' not in retriever.__all__ and ra.SLIM is retriever.SLIM and ra.slim_torch is retriever.slim_torch
    with pytest.raises(NotImplementedError, match='sharded fit'):
        ra.SLIM().fit(None, dist=object())
    with pytest.raises(NotImplementedError, match='fused_slim'):
        ra.SLIM({'model': {'fused_slim': True}, 'train': {'positive_only': False}})._slim_build(None, 'cpu')
    with pytest.raises(ValueError, match='l1_ratio'):
        ra.ops.slim_fit(torch.zeros(3, 3, dtype=torch.float64), 5, 1.0, 1.0)
