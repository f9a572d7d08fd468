"""GPU: ``ops.knn_build`` / ``ops.knn_score`` / ``ItemKNN`` against the float64 referee (tests/itemknn_referee.py).
A column of the build passes when: its count is min(knn, nnz); every returned (id, sim) is a true off-diagonal non-zero of the
column with sim within the derived tolerance of the float64 value; ids are distinct; no unreturned j beats the smallest returned
float64 score by more than the tolerance; no higher id won an exact tie; the stored order is non-increasing in sim with ids ascending
among equal bits; unused slots hold (-1, +0).  Two runs are bit-equal and a catalog cut into tiles gives the bits of one tile.
Scores: within (K + 2) u sum |terms| of float64 on the kernel's own lists; a user's row has the same bits alone, in a batch of 300,
with another tile and on a second run.
Model, ml-100k: measured gap of the test metrics to float64 dense scoring: see test_model_on_ml100k."""
import functools

import numpy as np
import pytest
import torch

import itemknn_referee as kr
import recstudio_amd as ra
from recstudio_amd import ops
from test_dataset_golden import make

pytestmark = pytest.mark.gpu
CASES = [(1, 2, 1, None), (7, 9, 3, None), (40, 255, 5, 256), (40, 256, 5, 256), (40, 257, 5, 256), (60, 513, 5, 256),
         (300, 1000, 100, 256), (300, 1000, 100, None), (60, 300, 1024, None)]


@functools.lru_cache(maxsize=None)
def case(n_users, N):
    R = kr.make_data(n_users, N)
    return R, kr.csrs(R, 'cuda'), {s: kr.rule64(R, s) for s in kr.SIM_TOL}


@functools.lru_cache(maxsize=None)
def built(n_users, N, knn, tile, similarity):
    return ops.knn_build(*case(n_users, N)[1], knn, similarity, tile=tile)


@pytest.mark.parametrize('similarity', ['cosine', 'jaccard'])
@pytest.mark.parametrize('n_users,N,knn,tile', CASES)
def test_build_against_the_referee(n_users, N, knn, tile, similarity):
    S, cls = case(n_users, N)[2][similarity]
    out = built(n_users, N, knn, tile, similarity)
    worst = kr.judge(S, cls, *(t.cpu().numpy() for t in out), knn, kr.SIM_TOL[similarity])
    print('worst share of the similarity tolerance', worst)
    again = ops.knn_build(*case(n_users, N)[1], knn, similarity, tile=tile)
    assert all(torch.equal(a, b) for a, b in zip(out, again))
    if tile is not None:                                                # tiles + merge: the bits of the one-tile build
        assert all(torch.equal(a, b) for a, b in zip(out, built(n_users, N, knn, None, similarity)))


@pytest.mark.parametrize('n_users,N,knn,tile', CASES)
def test_score_against_float64_on_the_kernels_lists(n_users, N, knn, tile):
    nbr_id, nbr_sim, nbr_cnt = (t.cpu() for t in built(n_users, N, knn, tile, 'cosine'))
    t_lists = [t.cuda() for t in ops.knn_transpose(nbr_id, nbr_sim, nbr_cnt)]
    rng = np.random.default_rng(N)
    lengths = [min(n, N - 1) for n in (0, 1, 255, 256, 257, N // 2)]
    H = np.zeros((len(lengths), N), bool)
    for r, n in enumerate(lengths):
        H[r, 1 + rng.choice(N - 1, n, replace=False)] = True
    h_indptr, h_items = kr.csrs(H, 'cuda')[:2]
    B = np.zeros((N, N))
    for i in range(N):
        B[nbr_id[i, :nbr_cnt[i]].numpy(), i] = nbr_sim[i, :nbr_cnt[i]].double().numpy()
    Hd = H.astype(np.float64)
    want, terms = (Hd @ B)[:, 1:], (Hd @ (B > 0))[:, 1:]
    users = torch.arange(len(lengths), device='cuda')
    got = ops.knn_score(users, h_indptr, h_items, *t_lists, N, tile=tile)
    assert got.shape == (len(lengths), N - 1) and not got[0].any()                   # no history: zeros
    assert (np.abs(got.double().cpu().numpy() - want) <= kr.score_bound(terms, want)).all()
    batch = users.repeat(50)
    assert torch.equal(ops.knn_score(batch, h_indptr, h_items, *t_lists, N, tile=tile), got.repeat(50, 1))
    for r in range(len(lengths)):                                                     # alone, on the default tile
        assert torch.equal(ops.knn_score(users[r:r + 1], h_indptr, h_items, *t_lists, N), got[r:r + 1])


@pytest.fixture(scope='module')
def splits(golden):
    ra.seed_everything(2022)
    return make(ra.TripletDataset, golden('data_ml100k')).build(split_ratio=[0.8, 0.1, 0.1], shuffle=True)


def test_model_on_ml100k(splits):
    """Both arms against float64 dense scoring on the flag-on lists; the bound is half a unit of the fourth printed digit.
    Measured on the MI355X: largest gap over the 18 test metrics 0.0 for either arm."""
    trn, _, tst = splits
    models = {}
    for fused in (True, False):
        models[fused] = m = ra.ItemKNN({'model': {'fused_knn': fused}, 'train': {'knn': 100, 'similarity': 'cosine'}})
        m.fit(trn)
    (u, i, _, (n_users, N)), _ = trn.get_graph([0])
    R = np.zeros((n_users, N), bool)
    R[u.numpy(), i.numpy()] = True
    S, cls = kr.rule64(R, 'cosine')
    for m in models.values():
        kr.judge(S, cls, m.nbr_id.cpu().numpy(), m.nbr_sim.cpu().numpy(), m.nbr_cnt.cpu().numpy(), 100, kr.SIM_TOL['cosine'])
    on = models[True]
    B = torch.zeros(N, N, dtype=torch.float64, device='cuda')
    live = torch.arange(100, device='cuda')[None] < on.nbr_cnt[:, None]
    B[on.nbr_id[live].long(), torch.arange(N, device='cuda')[:, None].expand(N, 100)[live]] = on.nbr_sim[live].double()
    R64 = torch.from_numpy(R).cuda().double()

    def topk64(batch, k, user_h=None, return_query=False):
        scores = R64[batch[trn.fuid]] @ B
        scores[:, 0] = -np.inf
        scores.scatter_(1, user_h, -np.inf)
        return torch.topk(scores, k)
    got = {fused: m.evaluate(tst, verbose=False) for fused, m in models.items()}
    on.topk = topk64
    want = on.evaluate(tst, verbose=False)
    del on.topk
    for fused, metrics in got.items():
        gaps = {k: abs(v - want[k]) for k, v in metrics.items()}
        print('fused_knn', fused, metrics, 'largest gap to float64', max(gaps.values()))
        assert max(gaps.values()) <= 5e-5
    users = torch.arange(1, 301, device='cuda')
    hist = tst.user_hist[users.cpu()].cuda()
    score, top = on.topk({trn.fuid: users}, 20, hist)
    assert (top > 0).all() and not (top[:, :, None] == hist[:, None, :]).any()
    fresh = ra.ItemKNN()
    fresh.load_state_dict(on.state_dict())
    assert all(torch.equal(a, b) for a, b in zip(fresh.topk(users, 20, hist), (score, top)))
