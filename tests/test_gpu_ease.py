"""GPU: ``ops.ease_gram`` / ``spd_inverse`` / ``ease_weights`` / ``ease_score`` and ``EASE`` against tests/ease_referee.py.
Inverse: P bit-symmetric, two runs bit-equal, every element of B within tol = 8 max(e_np, n u max|B*|) of B* (the factor 8: three
backward-stable stages in another block order against LAPACK's two; an fp32 accumulator anywhere is 1e6 times outside).
Measured on the MI355X: see test_inverse_against_the_refined_referee and test_model_on_ml100k."""
import numpy as np
import pytest
import torch

import ease_referee as er
import itemknn_referee as kr
import recstudio_amd as ra
from recstudio_amd import ops
from test_dataset_golden import make

pytestmark = pytest.mark.gpu


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def test_mfma_layout_pin_at_16():
    """136 distinct entries: a swapped operand or result index of the matrix instruction moves at least one of them."""
    A = np.zeros((16, 16))
    A[np.tril_indices(16)] = 0.01 * np.arange(1, 137)
    A = A + np.tril(A, -1).T + 20 * np.eye(16)
    P, status = ops.spd_inverse(dev(A))
    want = np.linalg.inv(A)
    err = np.abs(P.cpu().numpy() - want).max()
    assert int(status) == 0 and err <= 16 * 8 * er.U64 * np.abs(want).max()


@pytest.mark.parametrize('n_users,N,tile', [(1, 2, None), (7, 9, None), (60, 513, None), (300, 1000, None), (300, 1000, 96)])
def test_gram_is_exact(n_users, N, tile):
    R = kr.make_data(n_users, N)
    G = ops.ease_gram(*kr.csrs(R, 'cuda'), 0.75, tile=tile)
    assert np.array_equal(G.cpu().numpy(), er.gram(R, 0.75))
    assert torch.equal(G, ops.ease_gram(*kr.csrs(R, 'cuda'), 0.75, tile=tile))


@pytest.mark.parametrize('lam', [250.0, 1e-3])
@pytest.mark.parametrize('n', [1, 2, 63, 64, 65, 127, 128, 129, 257, 600])
def test_inverse_against_the_refined_referee(n, lam):
    """Measured on the MI355X: worst share of tol over the 20 cases 0.18 (n = 257, lambda = 1e-3); at lambda = 250 at most 0.03."""
    R, G, Bs, tol = er.ease_case(n, lam)
    P, status = ops.spd_inverse(dev(G))
    assert int(status) == 0 and torch.equal(P, P.T)
    assert torch.equal(P, ops.spd_inverse(dev(G), overwrite=True)[0])
    B, loss = ops.ease_weights(P, lam)
    err = np.abs(B.cpu().numpy() - Bs).max()                            # n = 1, 2: B* = 0 and tol = 0: exact or wrong
    print(f'n = {n} lambda = {lam}: worst share of tol {err / tol if tol else 0.0:.3f} (tol {tol:.3e})')
    assert err <= tol
    if n >= 63:                                                         # below, R is empty or one column: the norm is 0 or trivial
        Rd = R.astype(np.float64)
        direct = np.linalg.norm(Rd - Rd @ Bs)
        print(f'loss: relative gap to the direct norm {abs(float(loss) - direct) / direct:.2e}')
        assert abs(float(loss) - direct) <= 1e-9 * direct


def test_status_names_the_first_bad_pivot():
    rng = np.random.default_rng(3)
    L = np.tril(rng.standard_normal((130, 130)) * 0.1, -1) + np.eye(130)
    d = np.ones(130)
    assert int(ops.spd_inverse(dev((L * d) @ L.T))[1]) == 0
    d[70] = -1.0                                                        # the pivots of a Cholesky sweep are the d of L D L^T
    P, status = ops.spd_inverse(dev((L * d) @ L.T))
    assert int(status) == 71 and torch.isnan(P).all()


@pytest.mark.parametrize('n', [1, 65, 257])
def test_weights_and_loss_on_a_given_p(n):
    lam = 0.5
    P = np.linalg.inv(er.gram(er.zipf_data(80, n), lam))
    B, loss = ops.ease_weights(dev(P), lam)
    want = -P / np.diag(P)
    want[np.diag_indices(n)] = 0.0
    got = B.cpu().numpy()
    assert np.array_equal(got, want) and not np.signbit(np.diag(got)).any()
    assert abs(float(loss) - er.closed_form_loss(P, lam)) <= 1e-12 * er.closed_form_loss(P, lam)
    inplace = dev(P)
    assert torch.equal(ops.ease_weights(inplace, lam, overwrite=True)[0], B) and torch.equal(inplace, B)


@pytest.mark.parametrize('N', [600, 1025])
def test_score_against_float64_on_the_kernels_b(N):
    R, G, _, _ = er.ease_case(N, 250.0)
    B = ops.ease_weights(ops.spd_inverse(dev(G))[0], 250.0)[0]
    rng = np.random.default_rng(N)
    lengths = [0, 1, 255, 256, 257, N // 2]
    H = np.zeros((len(lengths), N), bool)
    for r, n in enumerate(lengths):
        H[r, 1 + rng.choice(N - 1, n, replace=False)] = True
    h_indptr, h_items = kr.csrs(H, 'cuda')[:2]
    Bn, Hd = B.cpu().numpy(), H.astype(np.float64)
    want, mass = (Hd @ Bn)[:, 1:], (Hd @ np.abs(Bn))[:, 1:]
    users = torch.arange(len(lengths), device='cuda')
    got = ops.ease_score(users, h_indptr, h_items, B)
    assert got.shape == (len(lengths), N - 1) and got.dtype == torch.float32 and not got[0].any()
    bound = (np.array(lengths)[:, None] + 2) * er.U64 * mass + 2.0 ** -24 * np.abs(want)
    assert (np.abs(got.double().cpu().numpy() - want) <= bound).all()
    assert torch.equal(ops.ease_score(users.repeat(50), h_indptr, h_items, B), got.repeat(50, 1))      # a batch of 300
    for r in range(len(lengths)):
        assert torch.equal(ops.ease_score(users[r:r + 1], h_indptr, h_items, B), got[r:r + 1])


def test_model_on_ml100k(golden):
    """Both arms against float64 dense scoring on the flag-on B; the bound is half a unit of the fourth printed digit.
    Measured on the MI355X: largest gap over the test metrics 0.0 for either arm."""
    ra.seed_everything(2022)
    trn, _, tst = make(ra.TripletDataset, golden('data_ml100k')).build(split_ratio=[0.8, 0.1, 0.1], shuffle=True)
    models = {}
    for fused in (True, False):
        models[fused] = m = ra.EASE({'model': {'fused_ease': fused}})
        m.fit(trn)
    on = models[True]
    assert on._get_item_vector().shape == (on.ease_B.size(0), on.ease_B.size(0) - 1)
    (u, i, _, (n_users, N)), _ = trn.get_graph([0])
    R64 = torch.zeros(n_users, N, dtype=torch.float64, device='cuda')
    R64[u.cuda(), i.cuda()] = 1

    def topk64(batch, k, user_h=None, return_query=False):
        scores = R64[batch[trn.fuid]] @ on.ease_B
        scores[:, 0] = -np.inf
        scores.scatter_(1, user_h, -np.inf)
        return torch.topk(scores, k)
    got = {fused: m.evaluate(tst, verbose=False) for fused, m in models.items()}
    on.topk = topk64
    want = on.evaluate(tst, verbose=False)
    del on.topk
    for fused, metrics in got.items():
        gaps = {k: abs(v - want[k]) for k, v in metrics.items()}
        print('fused_ease', fused, metrics, 'largest gap to float64', max(gaps.values()))
        assert max(gaps.values()) <= 5e-5
    users = torch.arange(1, 301, device='cuda')
    hist = tst.user_hist[users.cpu()].cuda()
    score, top = on.topk({trn.fuid: users}, 20, hist)
    fresh = ra.EASE({'model': {'fused_ease': True}})
    fresh.load_state_dict(on.state_dict())
    assert all(torch.equal(a, b) for a, b in zip(fresh.topk(users, 20, hist), (score, top)))
