"""CPU: the torch twin of the ItemKNN build against the float64 rule, three seeded mistakes that the column judgement must refuse, and
the argument checks of rsa_knn_build / rsa_knn_score (they fire before any HIP call)."""
import ctypes

import numpy as np
import pytest
import torch

import itemknn_referee as kr
import recstudio_amd as ra


@pytest.mark.parametrize('similarity', ['cosine', 'jaccard'])
@pytest.mark.parametrize('n_users,N,knn', [(1, 2, 1), (7, 9, 3), (40, 257, 5), (60, 300, 1024)])
def test_torch_twin_equals_float64_rule(n_users, N, knn, similarity):
    R = kr.make_data(n_users, N)
    S, cls = kr.rule64(R, similarity)
    u, i = (torch.from_numpy(t) for t in np.nonzero(R))
    ids, sims, cnt = ra.itemknn_torch(u, i, n_users, N, knn, similarity, dtype=torch.float64, chunk=100)
    want_ids, want_sims, want_cnt = kr.lists_from(S, knn)
    assert np.array_equal(ids.numpy(), want_ids) and np.array_equal(cnt.numpy(), want_cnt)       # the min(knn, nnz) branch included
    assert np.abs(sims.numpy() - want_sims).max() <= 1e-12
    kr.judge(S, cls, ids, sims, cnt, knn, 1e-12)
    t_indptr, t_items, t_sim = ra.ops.knn_transpose(ids, sims, cnt)
    u_indptr, u_items = kr.csrs(R)[:2]
    B = np.zeros((N, N))
    for t in range(N):
        B[want_ids[t, :want_cnt[t]], t] = want_sims[t, :want_cnt[t]]
    got = ra.itemknn_score_torch(torch.arange(n_users), u_indptr, u_items, t_indptr, t_items, t_sim, N)
    assert np.abs(got.numpy() - (R.astype(np.float64) @ B)[:, 1:]).max() <= 1e-12


def test_unknown_similarity_raises():
    with pytest.raises(ValueError, match='unsupported similarity metric'):
        ra.itemknn_torch(torch.ones(1, dtype=torch.int64), torch.ones(1, dtype=torch.int64), 2, 2, 1, 'dice')
    with pytest.raises(ValueError, match='unsupported similarity metric'):
        ra.ItemKNN({'train': {'similarity': 'dice'}})._knn_build(None, 'cpu')


@pytest.mark.parametrize('mistake', ['diagonal kept', 'union without c', 'smallest kept'])
def test_seeded_mistake_leaves_the_judgement(mistake):
    R = kr.make_data(40, 60)
    S, cls = kr.rule64(R, 'jaccard')
    wrong = kr.rule64(R, 'jaccard', keep_diagonal=mistake == 'diagonal kept', union_without_c=mistake == 'union without c')[0]
    kr.judge(S, cls, *kr.lists_from(S, 5), 5, kr.SIM_TOL['jaccard'])
    with pytest.raises(AssertionError):
        kr.judge(S, cls, *kr.lists_from(wrong, 5, largest=mistake != 'smallest kept'), 5, kr.SIM_TOL['jaccard'])


def test_argument_checks_fire_before_any_hip_call():
    nat = ra._native
    lib = nat.lib()
    build = [(b'size', dict(size=0)), (b'knn = 0', dict(knn=0)), (b'knn = 1025', dict(knn=1025)), (b'not a power of two', dict(tile=48)),
             (b'not a power of two', dict(tile=65536)), (b'similarity', dict(similarity=2)), (b'below 2^24', dict(max_degree=1 << 24)),
             (b'u_indptr is null', dict(u_indptr=None)), (b'i_indptr is null', dict(i_indptr=None)), (b'u_items is null', dict(u_items=None)),
             (b'i_users is null', dict(i_users=None)), (b'order is null', dict(order=None)), (b'nbr_id is null', dict(nbr_id=None)),
             (b'nbr_sim is null', dict(nbr_sim=None)), (b'nbr_cnt is null', dict(nbr_cnt=None)), (b'workspace is null', dict(tile=4)),
             (b'too small', dict(tile=4, workspace=ctypes.c_void_p(256), workspace_bytes=64))]
    for text, fields in build:
        a = nat.KnnBuildArgs()
        a.n_users, a.n_items, a.nnz, a.n_order, a.knn, a.max_degree = 3, 9, 5, 4, 3, 2
        a.u_indptr = a.u_items = a.i_indptr = a.i_users = a.order = a.nbr_id = a.nbr_sim = a.nbr_cnt = ctypes.c_void_p(256)
        for k, v in fields.items():
            setattr(a, k, v)
        assert lib.rsa_knn_build(ctypes.byref(a), None) == -1 and text in lib.rsa_last_error(), lib.rsa_last_error()
    assert lib.rsa_knn_build_workspace_bytes(9, 4, 3, 0) == 0 and lib.rsa_knn_build_workspace_bytes(9, 4, 3, 4) > 4 * 3 * 3 * 8
    assert lib.rsa_knn_build_workspace_bytes(9, 4, 0, 4) == -1 and lib.rsa_knn_build_workspace_bytes(9, 4, 3, 3) == -1
    score = [(b'size', dict(size=0)), (b'not a power of two', dict(tile=3)), (b'users is null', dict(users=None)),
             (b'u_indptr is null', dict(u_indptr=None)), (b't_indptr is null', dict(t_indptr=None)), (b'out is null', dict(out=None)),
             (b'out of range', dict(n_items=0))]
    for text, fields in score:
        a = nat.KnnScoreArgs()
        a.n_batch, a.n_users, a.n_items = 2, 3, 9
        a.users = a.u_indptr = a.u_items = a.t_indptr = a.t_items = a.t_sim = a.out = ctypes.c_void_p(256)
        for k, v in fields.items():
            setattr(a, k, v)
        assert lib.rsa_knn_score(ctypes.byref(a), None) == -1 and text in lib.rsa_last_error(), lib.rsa_last_error()
