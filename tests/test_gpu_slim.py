"""GPU: ``ops.slim_fit`` / ``SLIM`` against the float64 referee (tests/slim_referee.py), both kernels on every problem; the bounds
are stated at the assertions.  Measured worst share of the KKT bound on the MI355X: 0.125, the referee's own residual."""
import functools

import numpy as np
import pytest
import torch

import recstudio_amd as ra
import slim_referee as sr
from itemknn_referee import csrs
from recstudio_amd import ops
from test_dataset_golden import make

pytestmark = pytest.mark.gpu
# (U, N): seed, top, power of make_R and (alpha, l1_ratio), picked on the CPU for the candidate counts asserted in case()
CASES = {(2, 2): (0, 1.0, 0.0, 1.0, 0.1), (60, 40): (11, 0.6, 0.7, 1 / 6, 0.05), (300, 130): (9, 0.6, 0.7, 0.1, 0.05),
         (600, 330): (60, 0.9, 1.0, 1 / 12, 0.01)}
COUNTS = {(60, 40): {0, 1}, (300, 130): {0, 1, 64, 65}, (600, 330): {0, 1, 64, 65}}     # each also has one in 2 .. 63 and an empty item
RUNS = {'converged': dict(tol=0.0, max_iter=2000), 'default': dict(tol=1e-4, max_iter=100)}
SHAPES = list(CASES)


@functools.lru_cache(maxsize=None)
def case(U, N):
    seed, top, power, alpha, l1 = CASES[U, N]
    R = sr.make_R(U, N, seed, top, power)                                # (2, 2): the one interaction (1, 1)
    G = R.T.astype(np.float64) @ R
    a, b = alpha * l1 * U, alpha * (1 - l1) * U
    cand = [sr.candidates(G, j, a) for j in range(N)]
    counts = {len(c) for c in cand[1:]}
    if (U, N) in COUNTS:
        assert COUNTS[U, N] <= counts and any(2 <= c <= 63 for c in counts) and (G.diagonal()[1:] == 0).any(), sorted(counts)
        assert max(counts) > 256 or N < 300
    Gd = ops.ease_gram(*csrs(R, 'cuda'), 0.0)
    assert np.array_equal(Gd.cpu().numpy(), G)
    return G, Gd, alpha, l1, a, b, cand


@functools.lru_cache(maxsize=None)
def referee(U, N, run):
    G, _, _, _, a, b, _ = case(U, N)
    margins = [[] for _ in range(N)]
    return [sr.enet_gram(G, j, a, b, margins=margins[j], **RUNS[run]) + (margins[j],) for j in range(1, N)]


@functools.lru_cache(maxsize=None)
def fitted(U, N, run, wave_max):
    _, Gd, alpha, l1, _, _, _ = case(U, N)
    return tuple(t.cpu().numpy() for t in ops.slim_fit(Gd, U, alpha, l1, wave_max=wave_max, **RUNS[run]))


def dense(N, j, nbr_id, nbr_w, nbr_cnt):
    w = np.zeros(N)
    w[nbr_id[j, :nbr_cnt[j]]] = nbr_w[j, :nbr_cnt[j]]
    return w


@pytest.mark.parametrize('wave_max', [64, 0])
@pytest.mark.parametrize('U,N', SHAPES)
def test_converged_runs_meet_the_kkt_bound(U, N, wave_max):
    G, Gd, alpha, l1, a, b, cand = case(U, N)
    nbr_id, nbr_w, nbr_cnt, n_iter = fitted(U, N, 'converged', wave_max)
    other = fitted(U, N, 'converged', 64 - wave_max)
    assert nbr_cnt[0] == 0 and (n_iter[1:] == 2000).all()
    worst = 0.0
    for j in range(1, N):
        n, ids, w = nbr_cnt[j], nbr_id[j], dense(N, j, nbr_id, nbr_w, nbr_cnt)
        assert (np.diff(ids[:n]) > 0).all() and np.isin(ids[:n], cand[j]).all() and (nbr_w[j, :n] > 0).all(), j
        assert (ids[n:] == -1).all() and not nbr_w[j, n:].any(), j
        q, H = sr.problem(G, j)[0], sr.Qw(G, j, w)
        bound = np.maximum(8 * sr.kkt_violation(G, j, referee(U, N, 'converged')[j - 1][0], a, b).max(),
                           (len(cand[j]) + 2) * 2.0 ** -53 * (q + H + b * w))
        v = sr.kkt_violation(G, j, w, a, b)
        worst = max(worst, (v[bound > 0] / bound[bound > 0]).max(initial=0.0))
        assert (v <= bound).all(), (j, v.max())
        assert np.linalg.norm(w - dense(N, j, *other[:3])) <= np.linalg.norm(bound) / b, j
    print('worst share of the KKT bound', worst)
    again = ops.slim_fit(Gd, U, alpha, l1, wave_max=wave_max, **RUNS['converged'])
    assert all(np.array_equal(x, y.cpu().numpy()) for x, y in zip((nbr_id, nbr_w, nbr_cnt, n_iter), again))


@pytest.mark.parametrize('wave_max', [64, 0])
@pytest.mark.parametrize('U,N', SHAPES)
def test_default_runs_stop_where_the_referee_stops(U, N, wave_max):
    G, _, _, _, a, b, _ = case(U, N)
    nbr_id, nbr_w, nbr_cnt, n_iter = fitted(U, N, 'default', wave_max)
    tol, excluded = 1e-4, 0
    for j in range(1, N):
        (w_ref, _, n_ref, margins), (q, _, yy), w = referee(U, N, 'default')[j - 1], sr.problem(G, j), dense(N, j, nbr_id, nbr_w, nbr_cnt)
        if n_iter[j] < 100:
            assert sr.gap_of(q, sr.Qw(G, j, w), yy, w, a, b) < tol * yy * (1 + 1e-9), j
        near = any((r is not None and abs(r - tol) < 1e-9 * tol) or (g is not None and abs(g - tol * yy) < 1e-9 * tol * yy) for r, g in margins)
        excluded += near                                                  # a stop test within 1e-9 relative of its threshold
        assert near or (n_iter[j] == n_ref and (np.abs(w - w_ref) <= 1e-10 * np.abs(w_ref)).all()), j
    assert excluded <= 0.01 * (N - 1)


def test_model_on_ml100k(golden):
    ra.seed_everything(2022)
    trn, _, tst = make(ra.TripletDataset, golden('data_ml100k')).build(split_ratio=[0.8, 0.1, 0.1], shuffle=True)
    (u, i, _, (n_users, N)), _ = trn.get_graph([0])
    R = np.zeros((n_users, N))
    R[u.numpy(), i.numpy()] = 1
    G = R.T @ R
    B = np.stack([np.zeros(N)] + [sr.enet_gram(G, j, 0.1 * n_users, 0.9 * n_users)[0] for j in range(1, N)], 1)
    users = torch.arange(1, 301, device='cuda')
    want = torch.from_numpy(R[1:301] @ B[:, 1:])
    ref, metrics = torch.topk(want, 20), {}
    for fused in (True, False):
        m = ra.SLIM({'model': {'fused_slim': fused}})
        m.fit(trn)
        got = np.zeros((N, N))
        got[np.repeat(np.arange(N), np.diff(m.slim_indptr.cpu().numpy())), m.slim_items.cpu().numpy()] = m.slim_w.double().cpu().numpy()
        assert np.array_equal(got != 0, B != 0) and (np.abs(got - B) <= 2.0 ** -24 * np.abs(B) * (1 + 1e-6)).all()     # kept as fp32
        score, top = m.topk({trn.fuid: users}, 20)
        assert (score.double().cpu() - ref.values).abs().max() <= 1e-4
        assert (torch.gather(want, 1, top.cpu() - 1) - ref.values).abs().max() <= 2e-4       # ids differ only where scores tie within 1e-4
        metrics[fused] = m.evaluate(tst, verbose=False)
        fresh = ra.SLIM({'model': {'fused_slim': fused}})
        fresh.load_state_dict(m.state_dict())
        assert all(torch.equal(x, y) for x, y in zip(fresh.topk(users, 20), (score, top)))
    assert metrics[True] == metrics[False], metrics
