"""CPU: the EASE referee against the reference's literal formula, the torch twins against the referee, the closed-form loss, the
argument checks of the four entry points (they fire before any HIP call), and the model's refusals."""
import ctypes

import numpy as np
import pytest
import torch

import ease_referee as er
import itemknn_referee as kr
import recstudio_amd as ra

SHAPES = [(1, 2), (7, 9), (60, 65), (300, 200)]


@pytest.mark.parametrize('n_users,N', SHAPES)
@pytest.mark.parametrize('lam', [250.0, 1e-3])
def test_referee_twins_and_closed_form_loss(n_users, N, lam):
    R, G, Bs, tol = er.ease_case(N, lam, n_users)
    literal = er.weights_from(np.linalg.inv(G))                      # ease.py in float64
    assert np.abs(literal - Bs).max() <= tol / 8
    u, i = (torch.from_numpy(t) for t in np.nonzero(R))
    B, loss = ra.ease_torch(u, i, n_users, N, lam)
    assert np.abs(B.numpy() - Bs).max() <= tol and not B.diagonal().any()
    Rd = R.astype(np.float64)
    direct = np.linalg.norm(Rd - Rd @ Bs)
    assert abs(float(loss) - direct) <= 1e-9 * direct + 1e-12
    assert abs(er.closed_form_loss(np.linalg.inv(G), lam) - direct) <= 1e-9 * direct + 1e-9
    u_indptr, u_items = kr.csrs(R)[:2]
    got = ra.ease_score_torch(torch.arange(n_users), u_indptr, u_items, B)
    want = (Rd @ Bs)[:, 1:]
    assert got.dtype == torch.float32 and np.abs(got.double().numpy() - want).max() <= 2.0 ** -23 * np.abs(want).max() + N * tol


def test_argument_checks_fire_before_any_hip_call():
    nat = ra._native
    lib = nat.lib()
    P = ctypes.c_void_p(256)

    def refuses(fn, cls, base, cases):
        for text, fields in cases:
            a = cls()
            for k, v in {**base, **fields}.items():
                setattr(a, k, v)
            assert getattr(lib, fn)(ctypes.byref(a), None) == -1 and text in lib.rsa_last_error(), (fn, text, lib.rsa_last_error())
    refuses('rsa_ease_gram', nat.EaseGramArgs,
            dict(u_indptr=P, u_items=P, i_indptr=P, i_users=P, g=P, n_users=3, n_items=9, nnz=5, ld=10, lam=1.0),
            [(b'size', dict(size=0)), (b'n >= 1', dict(n_items=0)), (b'ld = 8', dict(ld=8)), (b'not finite', dict(lam=float('nan'))),
             (b'not finite', dict(lam=float('inf'))), (b'tile', dict(tile=16385)), (b'u_indptr is null', dict(u_indptr=None)),
             (b'i_indptr is null', dict(i_indptr=None)), (b'u_items is null', dict(u_items=None)), (b'i_users is null', dict(i_users=None)),
             (b'g is null', dict(g=None))])
    need = lib.rsa_spd_inverse_f64_workspace_bytes(65)
    assert need >= 2 * 128 * 64 * 8 and lib.rsa_spd_inverse_f64_workspace_bytes(0) == -1
    refuses('rsa_spd_inverse_f64', nat.SpdInverseArgs,
            dict(a=P, p=ctypes.c_void_p(512), status=P, n=65, ld=66, ldp=65, workspace=P, workspace_bytes=need),
            [(b'size', dict(size=0)), (b'n >= 1', dict(n=0)), (b'ld = 64', dict(ld=64)), (b'ldp = 3', dict(ldp=3)), (b'a is null', dict(a=None)),
             (b'p is null', dict(p=None)), (b'p must not be a', dict(p=P)), (b'status is null', dict(status=None)),
             (b'workspace is null', dict(workspace=None)), (b'too small', dict(workspace_bytes=need - 1))])
    refuses('rsa_ease_weights', nat.EaseWeightsArgs, dict(p=P, b=P, terms=P, loss=P, n=9, ld=10, ldb=10, lam=1.0),
            [(b'size', dict(size=0)), (b'n >= 1', dict(n=0)), (b'ld = 8', dict(ld=8)), (b'ldb = 8', dict(ldb=8, b=ctypes.c_void_p(512))),
             (b'not finite', dict(lam=float('nan'))), (b'p is null', dict(p=None)), (b'b is null', dict(b=None)),
             (b'b is p', dict(ldb=12)), (b'terms is null', dict(terms=None)), (b'loss is null', dict(loss=None))])
    refuses('rsa_ease_score', nat.EaseScoreArgs, dict(users=P, u_indptr=P, u_items=P, b=P, out=P, n_batch=2, n_users=3, n_items=9, ld=10),
            [(b'size', dict(size=0)), (b'n >= 1', dict(n_items=0)), (b'ld = 8', dict(ld=8)), (b'users is null', dict(users=None)),
             (b'u_indptr is null', dict(u_indptr=None)), (b'b is null', dict(b=None)), (b'out is null', dict(out=None))])


def test_model_refusals():
    assert ra.EASE().config['train']['lambda'] == 250 and ra.EASE().config['train']['epochs'] == 1

    class Split:
        drop_dup = False
    with pytest.raises(ValueError, match='drop_dup: False'):
        ra.EASE()._ease_build(Split(), 'cpu')
    with pytest.raises(NotImplementedError, match='sharded fit'):
        ra.EASE().fit(None, dist=object())
