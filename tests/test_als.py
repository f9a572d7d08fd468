"""CPU: ALSDataset / transpose() invariants on ml-100k, the torch twin of the ALS step against the float64 rule, and the argument
checks of rsa_als_solve (they fire before any HIP call)."""
import ctypes

import numpy as np
import torch

import als_referee as ar
import recstudio_amd as ra
from test_dataset_golden import make


def test_csr_and_transpose_invariants_on_ml100k(golden):
    ra.seed_everything(2022)
    trn = make(ra.ALSDataset, golden('data_ml100k')).build(split_ratio=[0.8, 0.1, 0.1], shuffle=True)[0]
    sub = trn.inter_feat_subset
    u, i = trn.inter_feat[trn.fuid][sub], trn.inter_feat[trn.fiid][sub]
    (up, ui, _), (ip, iu, _) = trn.csr()
    assert up[-1] == ip[-1] == len(sub) == 66868                          # every train interaction once in each CSR
    assert torch.equal(up[1:] - up[:-1], torch.bincount(u, minlength=trn.num_users))
    assert torch.equal(ip[1:] - ip[:-1], torch.bincount(i, minlength=trn.num_items))
    pairs = torch.sort(u * trn.num_items + i).values
    assert torch.equal(torch.sort(torch.repeat_interleave(torch.arange(trn.num_users), up[1:] - up[:-1]) * trn.num_items + ui).values, pairs)
    assert torch.equal(torch.sort(iu.long() * trn.num_items + torch.repeat_interleave(torch.arange(trn.num_items), ip[1:] - ip[:-1])).values, pairs)
    T = trn.transpose()
    assert (T.fuid, T.fiid) == (trn.fiid, trn.fuid) and len(T.data_index) == int((ip[1:] > ip[:-1]).sum())
    for item, s, e in T.data_index.tolist():                             # row i of the transpose: the TRAIN users of item i only
        assert (T.inter_feat[trn.fiid][s:e] == item).all()
        assert torch.equal(torch.sort(T.inter_feat[trn.fuid][s:e]).values, torch.sort(iu[ip[item]:ip[item + 1]].long()).values)


def test_torch_twin_equals_float64_rule():
    indptr, indices, table, rated = ar.make_case(1, 32, 23, [3, 1, 40, 7], rated_zeros=True)
    t = torch.from_numpy(table).double()
    gram = t.T @ t
    for r in range(4):
        ids = torch.from_numpy(indices[indptr[r]:indptr[r + 1]].astype(np.int64))[None]
        x, loss = ra.als_step_torch(ids, torch.from_numpy(rated[indptr[r]:indptr[r + 1]]).double()[None], t, gram, 1.0, 0.5)
        Y, w64, G, A, b = ar.row_system(indptr, indices, table, gram.numpy(), 1.0, 0.5, rated, r)
        xs = np.linalg.solve(A, b)
        assert np.abs(x[0].numpy() - xs).max() <= 1e-10 and abs(float(loss) - ar.loss64(Y, w64, G, 1.0, xs)) <= 1e-10


def test_argument_checks_fire_before_any_hip_call():
    nat = ra._native
    lib = nat.lib()
    cases = [(b'size', dict(size=0)), (b'not 32, 64 or 128', dict(d=48)), (b'indptr is null', dict(indptr=None)),
             (b'table is null', dict(table=None)), (b'gram is null', dict(gram=None)), (b'x is null', dict(x=None)),
             (b'status is null', dict(status=None)), (b'rows is null', dict(n_solve=2)), (b'workspace is null', dict(max_parts=4, nnz=9)),
             (b'too small', dict(max_parts=4, nnz=9, workspace=ctypes.c_void_p(256), workspace_bytes=64))]
    for text, fields in cases:
        a = nat.AlsArgs()
        a.d, a.n_csr_rows, a.n_solve, a.n_table = 64, 3, 3, 5
        a.indptr = a.indices = a.table = a.gram = a.x = a.status = ctypes.c_void_p(256)
        for k, v in fields.items():
            setattr(a, k, v)
        assert lib.rsa_als_solve(ctypes.byref(a), None) == -1 and text in lib.rsa_last_error(), lib.rsa_last_error()
    assert lib.rsa_als_workspace_bytes(3, 3, 4, 48) == -1
