"""CPU: the host side of the LightGCN feature -- the normalised adjacency of the ml-100k fixture, the chunk plan of
ops.spmm_csr, the argument checks of rsa_spmm_csr (they run before any HIP call) and the settings LightGCN refuses.  No device
kernel runs here."""
import ctypes

import numpy as np
import pytest
import torch

from test_dataset_golden import make


@pytest.fixture(scope='module')
def ra():
    import recstudio_amd
    from recstudio_amd import _native
    import os
    if not os.path.exists(_native.LIB_PATH):
        _native.build()
    return recstudio_amd


@pytest.fixture(scope='module')
def train(ra, golden):
    ra.seed_everything(2022)
    ds = make(ra.TripletDataset, golden('data_ml100k'))
    return ds.build(split_ratio=[0.8, 0.1, 0.1], shuffle=True)[0]


def test_get_graph_returns_the_training_edges(ra, train):
    nu, ni = train.num_users, train.num_items
    u = train.inter_feat[train.fuid][train.inter_feat_subset]
    i = train.inter_feat[train.fiid][train.inter_feat_subset]
    (rows, cols, vals, shape), n_rel = train.get_graph([0], form='coo', value_fields='inter', col_offset=[nu], bidirectional=[True],
                                                       shape=(nu + ni, nu + ni))
    assert shape == (nu + ni, nu + ni) and n_rel == 3
    assert torch.equal(rows, torch.cat([u, i + nu])) and torch.equal(cols, torch.cat([i + nu, u]))
    assert torch.equal(vals, torch.cat([torch.full((len(u),), 1), torch.full((len(u),), 2)]))
    (rows, cols, vals, shape), n_rel = train.get_graph(0, row_offset=3)
    assert torch.equal(rows, u + 3) and torch.equal(cols, i) and shape == (nu, ni) and n_rel == 0 and float(vals.min()) == 1.0
    with pytest.raises(NotImplementedError):
        train.get_graph([1])
    with pytest.raises(NotImplementedError):
        train.get_graph([0], form='dgl')
    with pytest.raises(NotImplementedError):
        train.get_graph([0, 1], shape=(5, 5))


def test_norm_adj_of_the_ml100k_fixture(ra, train):
    adj = ra.graphmodule.NormAdj.from_dataset(train)
    nu, ni = train.num_users, train.num_items
    n = nu + ni
    u = train.inter_feat[train.fuid][train.inter_feat_subset]
    i = train.inter_feat[train.fiid][train.inter_feat_subset]
    assert adj.n_nodes == n and adj.nnz == 2 * len(train) == 2 * 66868 == adj.indices.numel() == adj.values.numel()
    assert adj.indptr.dtype == torch.int64 and adj.indices.dtype == torch.int32 and adj.values.dtype == torch.float32
    # the CSR equals its transpose: the very same arrays
    assert adj.symmetric and adj.t_indptr is adj.indptr and adj.t_indices is adj.indices and adj.t_values is adj.values
    import spmm_referee as sr
    t = sr.csr_sorted_edges(*sr.csr_transpose(adj.indptr, adj.indices, adj.values, n), n)
    same = sr.csr_sorted_edges(adj.indptr, adj.indices, adj.values, n)
    assert torch.equal(t[0], same[0]) and torch.equal(t[1], same[1])
    # degrees are the bincounts of the training split; the pad nodes are empty
    deg = adj.indptr[1:] - adj.indptr[:-1]
    assert torch.equal(deg[:nu], torch.bincount(u, minlength=nu)) and torch.equal(deg[nu:], torch.bincount(i, minlength=ni))
    assert int(deg[0]) == 0 and int(deg[nu]) == 0 and not bool((adj.indices == 0).any()) and not bool((adj.indices == nu).any())
    # a user's row lists its items in interaction order, an item's row its users
    first_user = int(u[0])
    row = adj.indices[adj.indptr[first_user]:adj.indptr[first_user + 1]].long()
    assert torch.equal(row, i[u == first_user] + nu)
    # values: the float64 formula rounded once
    rows = sr.edge_rows(adj.indptr)
    want = (deg.double()[rows].pow(-0.5) * deg.double()[adj.indices.long()].pow(-0.5)).float()
    assert torch.equal(adj.values, want)
    # and the whole thing is the referee's construction
    ref = sr.norm_adj_csr(u, i, nu, ni)
    assert torch.equal(ref[0], adj.indptr) and torch.equal(ref[1], adj.indices) and torch.equal(ref[2], adj.values)
    with pytest.raises(AssertionError):
        ra.graphmodule.NormAdj(u, i + nu, n, symmetric=True)          # one direction only
    one_way = ra.graphmodule.NormAdj(u, i + nu, n)
    assert not one_way.symmetric and one_way.t_indptr is not one_way.indptr


@pytest.mark.parametrize('chunk', [1, 7, 8, 64, 512, 100000])
def test_plan_chunks_tile_every_split_row(ra, train, chunk):
    adj = ra.graphmodule.NormAdj.from_dataset(train, chunk=chunk)
    plan, indptr = adj.plan, adj.indptr
    deg = indptr[1:] - indptr[:-1]
    split = (deg > chunk).nonzero().view(-1)
    assert plan.chunk == chunk and plan.n_rows == deg.numel() and plan.nnz == adj.nnz
    assert torch.equal(plan.split_row(), split) and plan.n_split == split.numel()
    assert plan.table.numel() == 2 * plan.n_split + 1 + 2 * plan.n_parts and plan.table.dtype == torch.int64
    sp, prow, pedge = plan.split_part(), plan.part_row(), plan.part_edge()
    assert int(sp[0]) == 0 and int(sp[-1]) == plan.n_parts == int(((deg[split] + chunk - 1) // chunk).sum())
    covered = torch.zeros(adj.nnz, dtype=torch.int64)
    for p in range(plan.n_parts) if plan.n_parts <= 4000 else range(0, plan.n_parts, 37):
        r = int(prow[p])
        s, e = int(pedge[p]), min(int(pedge[p]) + chunk, int(indptr[r + 1]))
        assert int(indptr[r]) <= s < e <= int(indptr[r + 1]) and e - s <= chunk and int(deg[r]) > chunk
        covered[s:e] += 1
    if plan.n_parts <= 4000:
        in_split = torch.zeros(adj.nnz, dtype=torch.int64)
        for r in split.tolist():
            in_split[int(indptr[r]):int(indptr[r + 1])] = 1
        assert torch.equal(covered, in_split)                 # every edge of a split row exactly once, no other edge
    # vectorised: pieces of a row are consecutive, start at the row's first edge and step by chunk
    owner = torch.repeat_interleave(torch.arange(plan.n_split), sp[1:] - sp[:-1])
    assert torch.equal(prow, split[owner])
    assert torch.equal(pedge, indptr[prow] + (torch.arange(plan.n_parts) - sp[owner]) * chunk)
    assert bool((pedge < indptr[prow + 1]).all())


def test_plan_rejects_bad_input(ra):
    with pytest.raises(TypeError):
        ra.ops.spmm_plan(torch.zeros(3, dtype=torch.int32))
    with pytest.raises(ValueError):
        ra.ops.spmm_plan(torch.tensor([0, 2, 1]))
    with pytest.raises(ValueError):
        ra.ops.spmm_plan(torch.tensor([0, 2, 4]), chunk=0)
    empty = ra.ops.spmm_plan(torch.tensor([0, 2, 4]))
    assert (empty.n_split, empty.n_parts, empty.table.numel()) == (0, 0, 1)


def test_spmm_argument_validation_runs_before_any_device_call(ra):
    nat = ra._native
    lib = nat.lib()
    fake = ctypes.c_void_p(1 << 20)                           # never dereferenced: every case below fails its checks

    def args(**kw):
        a = nat.SpmmArgs()
        a.indptr, a.indices, a.x, a.y = fake, fake, fake, fake
        a.n_rows, a.n_cols, a.nnz, a.dim, a.chunk = 10, 10, 40, 64, 8
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    def refused(a, text):
        assert lib.rsa_spmm_csr(ctypes.byref(a), None) == -1
        assert text in lib.rsa_last_error(), lib.rsa_last_error()

    assert lib.rsa_spmm_csr(None, None) == -1 and b'args is null' in lib.rsa_last_error()
    a = args()
    a.size = 0
    refused(a, b'size')
    for dim in (0, 6, 260, -4):
        refused(args(dim=dim), b'multiple of 4')
    refused(args(n_rows=-1), b'negative size')
    refused(args(chunk=0), b'chunk')
    refused(args(indptr=None), b'indptr is null')
    refused(args(indices=None), b'indices/x is null')
    refused(args(x=None), b'indices/x is null')
    refused(args(y=None), b'y and acc_out are both null')
    refused(args(acc_out=fake), b'acc_out without acc_in')
    refused(args(x=ctypes.c_void_p((1 << 20) + 4)), b'16-byte aligned')
    refused(args(n_cols=1 << 31), b'int32')
    # the plan: 2 split rows cut into 5 pieces need 2 * 2 + 1 + 2 * 5 = 15 entries and 5 * 64 * 4 bytes of partials
    plan = dict(n_split=2, n_parts=5, plan=fake, plan_len=15, partials=fake, partials_bytes=5 * 64 * 4)
    refused(args(**dict(plan, plan_len=14)), b'plan is too small')
    refused(args(**dict(plan, plan=None)), b'plan is null')
    refused(args(**dict(plan, partials_bytes=5 * 64 * 4 - 1)), b'partials workspace is too small')
    refused(args(**dict(plan, partials=None)), b'partials is null')
    refused(args(**dict(plan, n_parts=3)), b'cannot belong')
    refused(args(**dict(plan, n_split=11, n_parts=22, plan_len=100, partials_bytes=1 << 20)), b'cannot belong')
    # an empty matrix is a valid no-op, also without a device
    assert lib.rsa_spmm_csr(ctypes.byref(args(n_rows=0, nnz=0)), None) == 0
    with pytest.raises(RuntimeError, match='GPU only'):
        p = ra.ops.spmm_plan(torch.tensor([0, 1]))
        ra.ops.spmm_csr(torch.tensor([0, 1]), torch.zeros(1, dtype=torch.int32), None, torch.zeros(1, 4), plan=p)


# ------------------------------------------------------------------------------------------------ what LightGCN refuses
def test_lightgcn_defaults_and_towers(ra, train):
    m = ra.LightGCN({'train': {'seed': 1}})
    assert m.config['model']['n_layers'] == 3 and m.config['model']['l2_reg_weight'] == 1e-4
    assert m.config['train']['negative_count'] == 1
    m._init_model(train)
    m._init_parameter()
    assert isinstance(m.loss_fn, ra.BPRLoss) and isinstance(m.score_func, ra.InnerProductScorer)
    assert type(m.sampler) is ra.UniformSampler
    assert isinstance(m.query_encoder, ra.graphmodule.GraphUserEncoder) and isinstance(m.item_encoder, ra.graphmodule.GraphItemEncoder)
    assert m.user_emb.padding_idx == 0 and m.item_emb.padding_idx == 0
    assert float(m.user_emb.weight.detach()[0].abs().max()) == 0 and float(m.item_emb.weight.detach()[0].abs().max()) == 0
    assert sorted(n for n, _ in m.named_parameters()) == ['item_emb.weight', 'user_emb.weight']
    assert m.adj_mat.nnz == 2 * len(train) and m.LightGCNNet.n_layers == 3
    assert m._fullscore_catalog() == train.num_items                     # evaluation selects in the MFMA kernel
    assert ra.BPR()._fullscore_catalog() is None                         # (a BPR that has not been built has no tower yet)
    assert np.isclose(float(ra.loss_func.l2_reg_loss_fn(torch.ones(2, 3), 2 * torch.ones(4, 3))), 3.0 + 12.0)


def test_lightgcn_refuses_fused_optimizer(ra, train):
    m = ra.LightGCN({'train': {'fused_optimizer': 'sgd', 'negative_count': 64}})
    m._init_model(train)
    with pytest.raises(NotImplementedError, match='stock BPR two-tower'):
        m._fused_optimizer_step(m.config['train'])


def test_lightgcn_refuses_multi_gpu_fit(ra, train):
    class TwoRanks:
        def get_rank(self):
            return 0

        def get_world_size(self):
            return 2
    m = ra.LightGCN({'train': {'negative_count': 64}})
    with pytest.raises(NotImplementedError, match='nn.Embedding item tower'):
        m.fit(train, dist=TwoRanks(), device='cpu')


def test_lightgcn_refuses_ann(ra):
    with pytest.raises(NotImplementedError, match='ANN'):
        ra.LightGCN({'train': {'ann': {'index': 'IVFx,Flat'}}})
