"""CPU: the referee of the SGL feature (tests/sgl_referee.py) against dense constructions, the seeded mistakes it must catch at
the bounds the GPU tests use, the reverse-edge map of NormAdj, NodeDropout's flags, the argument checks of rsa_graph_dropout
(they run before any HIP call) and the settings SGL takes and refuses.  No device kernel runs here."""
import ctypes

import numpy as np
import pytest
import torch

import sgl_referee as sg
import spmm_referee as sr

NU, NI, D = 41, 61, 16
N = NU + NI


@pytest.fixture(scope='module')
def ra():
    import recstudio_amd
    from recstudio_amd import _native
    import os
    if not os.path.exists(_native.LIB_PATH):
        _native.build()
    return recstudio_amd


@pytest.fixture(scope='module')
def small(ra):
    users, items = sr.random_bipartite(NU, NI, 400, seed=7)
    return ra.TripletDataset.from_mapped_ids(users, items, n_users=NU, n_items=NI)


@pytest.fixture(scope='module')
def adj(ra, small):
    return ra.graphmodule.NormAdj.from_dataset(small, chunk=8)


def masks(adj):
    """Three masks over the directed edges: edge dropout at 0.1 and 0.5 (each direction on its own), and a node dropout."""
    g = torch.Generator().manual_seed(3)
    rows, cols = sr.edge_rows(adj.indptr), adj.indices.long()
    flag = torch.zeros(N, dtype=torch.bool)
    flag[torch.tensor([1, 2, 3, 4, 5, NU + 1, NU + 2, NU + 3])] = True
    return {'ed 0.1': (torch.rand(adj.nnz, generator=g) + 0.9).floor().bool(), 'ed 0.5': (torch.rand(adj.nnz, generator=g) + 0.5).floor().bool(),
            'nd': ~(flag[rows] | flag[cols])}


def test_rev_pairs_every_edge_with_its_reverse(adj):
    rows, cols, rev = sr.edge_rows(adj.indptr), adj.indices.long(), adj.rev
    key = rows * N + cols
    assert int((torch.bincount(key) > 1).sum()) > 0                      # the graph has duplicate interactions
    assert rev.dtype == torch.int64 and rev.shape == (adj.nnz,)
    assert torch.equal(torch.sort(rev).values, torch.arange(adj.nnz))    # a bijection
    assert torch.equal(rev[rev], torch.arange(adj.nnz))
    assert torch.equal(cols[rev], rows) and torch.equal(rows[rev], cols)
    assert not torch.equal(rev, torch.arange(adj.nnz))


def test_rev_needs_a_symmetric_graph(ra):
    one_way = ra.graphmodule.NormAdj(torch.tensor([0, 1]), torch.tensor([1, 2]), 3)
    assert not one_way.symmetric
    with pytest.raises(ValueError, match='symmetric'):
        one_way.rev


@pytest.mark.parametrize('name', ['ed 0.1', 'ed 0.5', 'nd'])
def test_augment_agrees_with_the_dense_construction(adj, name):
    keep = masks(adj)[name]
    rows, cols = sr.edge_rows(adj.indptr), adj.indices.long()
    # edge dropout draws the two directions apart (the thinned matrix is not symmetric); node dropout drops both
    assert 0 < int(keep.sum()) < adj.nnz and torch.equal(keep, keep[adj.rev]) == (name == 'nd')
    out = sg.augment(adj.indptr, adj.indices, adj.rev, keep)
    want = sg.thinned_dense(cols[keep], rows[keep], N)
    got = sr.csr_dense(adj.indptr, adj.indices, out['values'], N)
    # every kept copy of a multi-edge carries the same weight rounded to fp32 once: the sum is off by at most u |want|
    assert bool(((got - want).abs() <= 1.001 * sr.U32 * want.abs()).all()) and bool(((got != 0) == (want != 0)).all())
    assert torch.equal(sr.csr_dense(adj.indptr, adj.indices, out['t_values'], N), got.t())
    mult = sr.csr_dense(adj.indptr, adj.indices, keep.float(), N).long()                    # kept copies per (dst, src)
    assert torch.equal(out['in_deg'], mult.sum(1)) and torch.equal(out['out_deg'], mult.sum(0))
    assert bool((out['values'][~keep] == 0).all())


def test_keeping_everything_gives_the_base_values(adj):
    out = sg.augment(adj.indptr, adj.indices, adj.rev, torch.ones(adj.nnz, dtype=torch.bool))
    assert torch.equal(out['values'], adj.values) and torch.equal(out['t_values'], adj.values)
    assert torch.equal(out['in_deg'], adj.in_deg) and torch.equal(out['out_deg'], adj.out_deg)


@pytest.mark.parametrize('mistake', ['base_degrees', 'rev_keep', 'inv_keep_prob'])
def test_seeded_value_mistakes_leave_one_ulp(adj, mistake):
    """The GPU test's bound on the values: 2 u |v_ref| on kept edges, exactly 0 on dropped ones."""
    keep = masks(adj)['ed 0.5']
    ref = sg.augment(adj.indptr, adj.indices, adj.rev, keep)['values'].double()
    bad = sg.augment(adj.indptr, adj.indices, adj.rev, keep, mistake=mistake, keep_prob=0.5)['values'].double()
    outside = (bad - ref).abs() > 2 * sr.U32 * ref.abs()
    assert int(outside.sum()) > 0


def _up_and_e0(seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(N, D, generator=g), torch.randn(N, D, generator=g)


@pytest.mark.parametrize('n_layers', [1, 2, 3])
def test_backward_through_the_untransposed_matrix_leaves_the_bound(adj, n_layers):
    keep = masks(adj)['ed 0.5']
    out = sg.augment(adj.indptr, adj.indices, adj.rev, keep)
    up, e0 = _up_and_e0(17)
    dense = sr.csr_dense(adj.indptr, adj.indices, out['values'], N)
    e64 = e0.double().requires_grad_(True)
    sg._mean_layers([dense] * n_layers, e64).backward(up.double())
    # one matrix for all layers: the backward is the layer mean over the transposed matrix on the incoming gradient
    want, tol = sr.propagate(adj.indptr, adj.indices, out['t_values'], up, n_layers)
    np.testing.assert_allclose(want.numpy(), e64.grad.numpy(), rtol=1e-12, atol=1e-14)
    same, _ = sg.propagate_each(adj.indptr, adj.indices, [out['t_values']] * n_layers, up)
    np.testing.assert_allclose(same.numpy(), want.numpy(), rtol=1e-14, atol=0)
    bad = sg.augment(adj.indptr, adj.indices, adj.rev, keep, mistake='t_is_values')
    wrong, _ = sr.propagate(adj.indptr, adj.indices, bad['t_values'], up, n_layers)
    assert sr.ratio(wrong, e64.grad, tol) > 1.0


@pytest.mark.parametrize('n_layers', [2, 3])
def test_one_view_per_layer_runs_backward_from_the_last_layer_down(adj, n_layers):
    g = torch.Generator().manual_seed(5)
    outs = [sg.augment(adj.indptr, adj.indices, adj.rev, (torch.rand(adj.nnz, generator=g) + 0.5).floor().bool()) for _ in range(n_layers)]
    up, e0 = _up_and_e0(23)
    dense = [sr.csr_dense(adj.indptr, adj.indices, o['values'], N) for o in outs]
    e64 = e0.double().requires_grad_(True)
    mean = sg._mean_layers(dense, e64)
    mean.backward(up.double())
    fwd, _ = sg.propagate_each(adj.indptr, adj.indices, [o['values'] for o in outs], e0)
    np.testing.assert_allclose(fwd.numpy(), mean.detach().numpy(), rtol=1e-12, atol=1e-14)
    tv = [o['t_values'] for o in outs]
    want, tol = sg.horner_each(adj.indptr, adj.indices, tv, up)
    np.testing.assert_allclose(want.numpy(), e64.grad.numpy(), rtol=1e-12, atol=1e-14)
    wrong, _ = sg.horner_each(adj.indptr, adj.indices, tv, up, mistake='up')
    assert sr.ratio(wrong, e64.grad, tol) > 1.0


@pytest.mark.parametrize('mistake', ['row0', 'raw_table', 'one_temperature'])
def test_seeded_info_nce_mistakes_leave_the_parity_bound(mistake):
    g = torch.Generator().manual_seed(11)
    table = torch.randn(NI, 64, generator=g, dtype=torch.float64)
    ids = torch.randint(1, NI, (32,), generator=g)
    other = table + 0.3 * torch.randn(NI, 64, generator=g, dtype=torch.float64)
    ref = sg.info_nce(other[ids], table[ids], table, 0.2, 'cosine')
    bad = sg.info_nce(other[ids], table[ids], table, 0.2, 'cosine', mistake=mistake)
    assert abs(float(bad - ref)) > 1e-4 * abs(float(ref))


def test_info_nce_is_the_cross_entropy_against_the_own_row():
    """With rep_j taken from the table, logsumexp - <i, j> / T is the cross entropy of the similarity row with the own id as label."""
    g = torch.Generator().manual_seed(12)
    table = torch.randn(NI, 8, generator=g, dtype=torch.float64)
    ids = torch.randint(1, NI, (16,), generator=g)
    q = torch.randn(16, 8, generator=g, dtype=torch.float64)
    got = sg.info_nce(q, table[ids], table, 0.5, 'inner_product')
    want = torch.nn.functional.cross_entropy(q @ table[1:].t() / 0.5, ids - 1)
    assert abs(float(got - want)) < 1e-12


def test_sgl_step_referee_reduces_to_lightgcn(adj):
    g = torch.Generator().manual_seed(2)
    ue, ie = 0.1 * torch.randn(NU, D, generator=g), 0.1 * torch.randn(NI, D, generator=g)
    uid, pos, neg = torch.randint(1, NU, (8,), generator=g), torch.randint(1, NI, (8,), generator=g), torch.randint(1, NI, (8, 2), generator=g)
    dense = sr.csr_dense(adj.indptr, adj.indices, adj.values, N)
    out = sg.augment(adj.indptr, adj.indices, adj.rev, masks(adj)['ed 0.5'])
    view = sr.csr_dense(adj.indptr, adj.indices, out['values'], N)
    base = sr.lightgcn_step(ue, ie, dense, 2, uid, pos, neg, 1e-4)
    off = sg.sgl_step(ue, ie, dense, [view, dense], 2, uid, pos, neg, 1e-4, 0.0, 0.2)
    on = sg.sgl_step(ue, ie, dense, [view, dense], 2, uid, pos, neg, 1e-4, 0.1, 0.2)
    assert abs(float(off['loss'] - base['loss'])) < 1e-14 and torch.allclose(off['user_grad'], base['user_grad'], rtol=0, atol=1e-16)
    assert abs(float(on['loss'] - base['loss'] - 0.1 * on['cl_loss'])) < 1e-12 and float(on['cl_loss']) > 0


def test_node_dropout_flags_are_the_references(ra):
    nd = ra.data_augmentation.NodeDropout(0.3, NU, NI)
    torch.manual_seed(77)
    got = nd.nodes_flag()
    torch.manual_seed(77)
    want = torch.tensor([False] * (NU + NI))                             # data_augmentation.py:281-285 restated
    user_drop_indices = torch.randperm(NU)[:int(NU * 0.3)]
    item_drop_indices = torch.randperm(NI)[:int(NI * 0.3)]
    want[user_drop_indices] = True
    want[item_drop_indices + NU] = True
    assert torch.equal(got, want) and int(got.sum()) == int(NU * 0.3) + int(NI * 0.3)


def test_augmentations_return_their_input_in_eval(ra, adj):
    for aug in (ra.data_augmentation.EdgeDropout(0.1, NU, NI), ra.data_augmentation.NodeDropout(0.1, NU, NI)):
        aug.eval()
        assert aug(adj) is adj
    with pytest.raises(RuntimeError, match='GPU'):
        ra.data_augmentation.EdgeDropout(0.1, NU, NI)(adj)


def test_info_nce_loss_settings(ra):
    loss = ra.data_augmentation.InfoNCELoss(0.2, 'cosine', 'batch_both')
    with pytest.raises(NotImplementedError, match='sequence models'):
        loss(torch.zeros(2, 4), torch.zeros(2, 4))
    with pytest.raises(NotImplementedError, match='sequence models'):
        ra.data_augmentation.InfoNCELoss(0.2, 'cosine', 'batch_single')(torch.zeros(2, 4), torch.zeros(2, 4))
    with pytest.raises(ValueError):
        ra.data_augmentation.InfoNCELoss(0.2, 'cosine', 'none')
    with pytest.raises(ValueError):
        ra.data_augmentation.InfoNCELoss(0.2, 'cosine', 'all')(torch.zeros(2, 4), torch.zeros(2, 4))


def test_graph_dropout_argument_validation_runs_before_any_device_call(ra):
    nat = ra._native
    lib = nat.lib()
    fake = ctypes.c_void_p(1 << 20)                           # never dereferenced: every case below fails its checks

    def args(**kw):
        a = nat.GraphDropoutArgs()
        a.indptr, a.indices, a.rev, a.values, a.t_values, a.in_deg, a.out_deg = (fake,) * 7
        a.n_rows, a.nnz, a.keep_prob = 10, 40, 0.9
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    def refused(a, text):
        assert lib.rsa_graph_dropout(ctypes.byref(a), None) == -1
        assert text in lib.rsa_last_error(), lib.rsa_last_error()

    assert lib.rsa_graph_dropout(None, None) == -1 and b'args is null' in lib.rsa_last_error()
    a = args()
    a.size = 0
    refused(a, b'size')
    refused(args(indptr=None), b'indptr is null')
    refused(args(indices=None), b'indices/rev is null')
    refused(args(rev=None), b'indices/rev is null')
    refused(args(values=None), b'values is null')
    refused(args(in_deg=None), b'in_deg/out_deg is null')
    refused(args(nnz=-1), b'negative size')
    refused(args(n_rows=-1), b'negative size')
    refused(args(n_rows=1 << 31), b'int32')
    refused(args(keep_prob=-0.1), b'keep_prob')
    refused(args(keep_prob=1.5), b'keep_prob')
    refused(args(keep_prob=float('nan')), b'keep_prob')
    refused(args(long_row=8), b'long_row')
    assert lib.rsa_graph_dropout(ctypes.byref(args(n_rows=0, nnz=0)), None) == 0
    with pytest.raises(RuntimeError, match='GPU only'):
        ra.ops.graph_dropout(torch.tensor([0, 1]), torch.zeros(1, dtype=torch.int32), torch.zeros(1, dtype=torch.int64), 0.9)


def test_spmm_acc_out_needs_acc(ra):
    with pytest.raises(RuntimeError, match='GPU only'):
        p = ra.ops.spmm_plan(torch.tensor([0, 1]))
        ra.ops.spmm_csr(torch.tensor([0, 1]), torch.zeros(1, dtype=torch.int32), None, torch.zeros(1, 4), plan=p, acc_out=torch.zeros(1, 4))


def test_sgl_defaults_and_refusals(ra, small):
    m = ra.SGL({'train': {'seed': 1}})
    model, train = m.config['model'], m.config['train']
    assert (model['aug_type'], model['n_layers'], model['l2_reg_weight'], model['ssl_ratio'], model['ssl_reg'], model['temperature']) == \
        ('ED', 3, 1e-4, 0.1, 0.1, 0.2)
    assert train['negative_count'] == 1 and train['batch_size'] == 2048
    assert ra.SGL({'train': {'batch_size': 512}}).config['train']['batch_size'] == 512
    m._init_model(small)
    assert isinstance(m.augmentaion_model.augmentation, ra.data_augmentation.EdgeDropout) and m.last_views is None
    assert abs(m.augmentaion_model.augmentation.keep_prob - 0.9) < 1e-12
    nd = ra.SGL({'model': {'aug_type': 'ND'}})
    nd._init_model(small)
    assert isinstance(nd.augmentaion_model.augmentation, ra.data_augmentation.NodeDropout)
    with pytest.raises(ValueError, match='aug_type'):
        ra.SGL({'model': {'aug_type': 'XX'}})._init_model(small)
    fused = ra.SGL({'train': {'fused_optimizer': 'sgd', 'negative_count': 64}})
    fused._init_model(small)
    with pytest.raises(NotImplementedError, match='stock BPR two-tower'):
        fused._fused_optimizer_step(fused.config['train'])
    with pytest.raises(NotImplementedError, match='ANN'):
        ra.SGL({'train': {'ann': {'index': 'IVFx,Flat'}}})
