"""GPU: rsa_graph_dropout (ops.graph_dropout, NormAdj.augmented) against torch.rand's mask and the float64 referee of
tests/sgl_referee.py, and the propagation -- forward and backward -- through one thinned view and through one view per layer."""
import numpy as np
import pytest
import torch

import sgl_referee as sg
import spmm_referee as sr

pytestmark = pytest.mark.gpu
DEV = 'cuda'
NU, NI = 41, 61
N = NU + NI


@pytest.fixture(scope='module')
def ra():
    import recstudio_amd
    recstudio_amd._native.lib()
    torch.cuda.init()
    return recstudio_amd


@pytest.fixture(scope='module')
def adj(ra):
    users, items = sr.random_bipartite(NU, NI, 400, seed=7)
    data = ra.TripletDataset.from_mapped_ids(users, items, n_users=NU, n_items=NI)
    a = ra.graphmodule.NormAdj.from_dataset(data, chunk=8).to(DEV)
    assert a.plan.n_split > 0                                            # the propagation reaches its split path
    return a


@pytest.fixture(scope='module')
def hub(ra):
    """41 users x 13 items, 575 interactions: the busiest item has 177 edges, more than the 128 from which the dropout shares a
    row between the waves of its windows (NormAdj.augmented: max(chunk, 128)); the next ones have 91 and 66."""
    users, items = sr.random_bipartite(NU, 13, 500, seed=7)
    data = ra.TripletDataset.from_mapped_ids(users, items, n_users=NU, n_items=13)
    a = ra.graphmodule.NormAdj.from_dataset(data, chunk=8).to(DEV)
    assert int((a.indptr[1:] - a.indptr[:-1]).max()) > 128
    return a


def offset():
    return torch.cuda.default_generators[torch.cuda.current_device()].get_offset()


def check_view(adj, view, keep_prob, seed):
    """Everything the issue asks of one call whose generator state was ``torch.manual_seed(seed)``."""
    nnz = adj.nnz
    after = offset()
    torch.manual_seed(seed)
    want = torch.floor(torch.rand(nnz, device=DEV) + keep_prob).bool()
    assert offset() == after
    keep = view.keep.bool()
    assert view.keep.dtype == torch.uint8 and torch.equal(keep, want)
    ref = sg.augment(adj.indptr, adj.indices, adj.rev, keep)
    assert view.in_deg.dtype == torch.int32 and torch.equal(view.in_deg.long(), ref['in_deg']) and torch.equal(view.out_deg.long(), ref['out_deg'])
    v, v_ref = view.values, ref['values']
    assert bool(((v.double() - v_ref.double()).abs()[keep] <= 2 * sr.U32 * v_ref.double().abs()[keep]).all())
    print(f'keep_prob {keep_prob}, nnz {nnz}: {int(keep.sum())} kept, {int((v == v_ref)[keep].sum())} of their values bit-equal to the referee')
    assert bool((v[~keep].view(torch.int32) == 0).all())                 # +0, not -0
    assert torch.equal(view.t_values, v[adj.rev])
    return keep


@pytest.mark.parametrize('ssl_ratio', [0.1, 0.5])
def test_mask_degrees_and_values(ra, adj, ssl_ratio):
    keep_prob = 1.0 - ssl_ratio
    torch.manual_seed(41)
    view = adj.augmented(keep_prob)
    keep = check_view(adj, view, keep_prob, 41)
    assert 0 < int(keep.sum()) < adj.nnz
    cpu = lambda t: t.cpu()                                              # noqa: E731
    a = sr.csr_dense(cpu(adj.indptr), cpu(adj.indices), cpu(view.values), N)
    at = sr.csr_dense(cpu(adj.indptr), cpu(adj.indices), cpu(view.t_values), N)
    assert torch.equal(at, a.t()) and not torch.equal(a, at)
    torch.manual_seed(41)
    again = adj.augmented(keep_prob)
    for name in ('values', 't_values', 'in_deg', 'out_deg', 'keep'):
        assert torch.equal(getattr(view, name), getattr(again, name)), name
    # ops.graph_dropout itself: the same numbers, keep only on request, whatever the length from which rows are shared
    for long_row in (None, 128, 256):
        torch.manual_seed(41)
        out = ra.ops.graph_dropout(adj.indptr, adj.indices, adj.rev, keep_prob, long_row=long_row)
        assert len(out) == 4 and all(torch.equal(x, getattr(view, name)) for x, name in zip(out, ('values', 't_values', 'in_deg', 'out_deg')))
    g = torch.Generator(device=DEV).manual_seed(41)
    own = adj.augmented(keep_prob, generator=g)
    assert torch.equal(own.keep, view.keep) and g.get_offset() > 0


@pytest.mark.parametrize('keep_prob', [0.9, 0.5])
def test_rows_shared_between_windows(ra, hub, keep_prob):
    torch.manual_seed(43)
    view = hub.augmented(keep_prob)
    check_view(hub, view, keep_prob, 43)
    for long_row in (128, 160, 256, None):                              # shared over 2 - 3 windows, over 2, not shared
        torch.manual_seed(43)
        out = ra.ops.graph_dropout(hub.indptr, hub.indices, hub.rev, keep_prob, long_row=long_row)
        assert all(torch.equal(x, getattr(view, name)) for x, name in zip(out, ('values', 't_values', 'in_deg', 'out_deg'))), long_row
    flag = torch.zeros(hub.n_nodes, dtype=torch.bool, device=DEV)
    flag[NU + 1 + torch.topk((hub.indptr[1:] - hub.indptr[:-1])[NU + 1:], 1).indices] = True          # the hub itself dropped
    nd = hub.augmented(1.0, node_drop=flag)
    rows, cols = sr.edge_rows(hub.indptr), hub.indices.long()
    assert torch.equal(nd.keep.bool(), ~(flag[rows] | flag[cols])) and int(nd.in_deg[flag].sum()) == 0 and int(nd.out_deg[flag].sum()) == 0
    with pytest.raises(ra._native.NativeError, match='long_row'):
        ra.ops.graph_dropout(hub.indptr, hub.indices, hub.rev, keep_prob, long_row=64)


def test_second_philox_round_and_long_rows(ra):
    """nnz just above 4 * grid_threads: elements past the first round of the generator's grid; 400 items of ~5000 edges each are
    shared between windows at the default length."""
    cu, mt = ra.rng.device_props(DEV)
    m = 2 * cu * (mt // 256) * 256 + 300
    g = torch.Generator().manual_seed(1)
    users, items = torch.randint(1, 3001, (m,), generator=g), torch.randint(1, 401, (m,), generator=g)
    n_users, n_items = 3001, 401
    rows = torch.cat([users, items + n_users])
    cols = torch.cat([items + n_users, users])
    big = ra.graphmodule.NormAdj(rows, cols, n_users + n_items, symmetric=True).to(DEV)
    assert big.nnz == 2 * m and big.nnz > 4 * ra.rng.grid_threads(big.nnz, cu, mt)
    assert big.nnz - 4 * ra.rng.grid_threads(big.nnz, cu, mt) < 1000
    assert int((big.indptr[1:] - big.indptr[:-1]).max()) > ra.ops.GRAPH_DROPOUT_LONG_ROW
    rev = big.rev
    ar = torch.arange(big.nnz, device=DEV)
    assert torch.equal(rev[rev], ar) and torch.equal(big.indices.long()[rev], sr.edge_rows(big.indptr))
    torch.manual_seed(8)
    view = big.augmented(0.9)
    check_view(big, view, 0.9, 8)


def test_nothing_dropped(ra, adj):
    torch.manual_seed(3)
    before = offset()
    view = adj.augmented(1.0)
    assert offset() == before                                            # keep_prob >= 1 consumes no uniforms
    assert bool(view.keep.bool().all())
    assert torch.equal(view.in_deg.long().cpu(), adj.in_deg) and torch.equal(view.out_deg.long().cpu(), adj.out_deg)
    base = adj.values.double()
    assert bool(((view.values.double() - base).abs() <= 2 * sr.U32 * base.abs()).all())
    assert torch.equal(view.t_values, view.values[adj.rev])
    print(f'{int((view.values == adj.values).sum())} of {adj.nnz} values bit-equal to NormAdj.values')


@pytest.mark.parametrize('n_layers', [1, 3])
def test_everything_dropped(ra, adj, n_layers):
    view = adj.augmented(0.0)
    assert not bool(view.keep.any()) and not bool(view.in_deg.any()) and not bool(view.out_deg.any())
    assert bool((view.values.view(torch.int32) == 0).all()) and bool((view.t_values.view(torch.int32) == 0).all())
    e0 = torch.randn(N, 64, generator=torch.Generator().manual_seed(2)).to(DEV).requires_grad_(True)
    out = ra.graphmodule.LightGCNNet(n_layers).propagate(view, e0)
    out.sum().backward()
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(e0.grad).all())
    want = e0.detach().double() / (n_layers + 1)
    assert bool(((out.double() - want).abs() <= 2 * sr.U32 * want.abs()).all())


def test_node_drop_given(ra, adj):
    deg = adj.indptr[1:] - adj.indptr[:-1]
    busiest = torch.topk(deg[NU:], 3).indices + NU
    flag = torch.zeros(N, dtype=torch.bool, device=DEV)
    flag[1:6] = True
    flag[busiest] = True
    before = offset()
    view = adj.augmented(1.0, node_drop=flag)
    assert offset() == before
    rows, cols = sr.edge_rows(adj.indptr), adj.indices.long()
    keep = view.keep.bool()
    assert torch.equal(keep, ~(flag[rows] | flag[cols])) and torch.equal(keep, keep[adj.rev])
    ref = sg.augment(adj.indptr, adj.indices, adj.rev, keep)
    assert torch.equal(view.in_deg.long(), ref['in_deg']) and torch.equal(view.out_deg.long(), ref['out_deg'])
    assert bool(((view.values.double() - ref['values'].double()).abs() <= 2 * sr.U32 * ref['values'].double().abs()).all())
    assert bool((view.values[~keep].view(torch.int32) == 0).all()) and torch.equal(view.t_values, view.values[adj.rev])
    # with edge dropout on top: the uniforms are consumed, the flags still hold
    torch.manual_seed(6)
    both = adj.augmented(0.5, node_drop=flag.cpu())
    torch.manual_seed(6)
    drawn = torch.floor(torch.rand(adj.nnz, device=DEV) + 0.5).bool()
    assert torch.equal(both.keep.bool(), drawn & keep)
    L = 3
    e0 = torch.randn(N, 64, generator=torch.Generator().manual_seed(4)).to(DEV)
    out = ra.graphmodule.LightGCNNet(L).propagate(view, e0)
    want = e0.double() / (L + 1)
    assert bool(((out.double() - want).abs()[flag] <= 2 * sr.U32 * want.abs()[flag]).all())
    assert not bool(((out.double() - want).abs()[~flag] <= 2 * sr.U32 * want.abs()[~flag]).all())


def _tables(d, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(N, d, generator=g).to(DEV).requires_grad_(True), torch.randn(N, d, generator=g).to(DEV)


def _dense(adj, values):
    return sr.csr_dense(adj.indptr.cpu(), adj.indices.cpu(), values.cpu(), N).to(DEV)


@pytest.mark.parametrize('n_layers', [1, 2, 3])
@pytest.mark.parametrize('d', [4, 64, 128, 256])
def test_propagation_through_a_view(ra, adj, d, n_layers):
    torch.manual_seed(100 + d + n_layers)
    view = adj.augmented(0.5)
    e0, up = _tables(d, 17)
    got = ra.graphmodule.LightGCNNet(n_layers).propagate(view, e0)
    got.backward(up)
    mean, tol = sg.propagate_each(adj.indptr, adj.indices, [view.values] * n_layers, e0.detach())
    r_fwd = sr.ratio(got.detach(), mean, tol)
    dense = _dense(adj, view.values)
    e64 = e0.detach().double().requires_grad_(True)
    m64 = sg._mean_layers([dense] * n_layers, e64)
    m64.backward(up.double())
    np.testing.assert_allclose(mean.cpu().numpy(), m64.detach().cpu().numpy(), rtol=1e-12, atol=1e-14)
    # the backward's own bound: the same layer mean over the transposed thinned matrix on the incoming gradient
    want, tol_b = sr.propagate(adj.indptr, adj.indices, view.t_values, up, n_layers)
    np.testing.assert_allclose(want.cpu().numpy(), e64.grad.cpu().numpy(), rtol=1e-12, atol=1e-14)
    r_bwd = sr.ratio(e0.grad, e64.grad, tol_b)
    print(f'd = {d}, L = {n_layers}: |got - ref| / bound = {r_fwd} forward, {r_bwd} backward')
    assert r_fwd <= 1.0 and r_bwd <= 1.0


@pytest.mark.parametrize('n_layers', [1, 2, 3])
@pytest.mark.parametrize('d', [4, 64, 128, 256])
def test_propagation_through_one_view_per_layer(ra, adj, d, n_layers):
    torch.manual_seed(200 + d + n_layers)
    views = [adj.augmented(0.5) for _ in range(n_layers)]
    assert n_layers == 1 or not torch.equal(views[0].keep, views[1].keep)
    e0, up = _tables(d, 19)
    got = ra.graphmodule.LightGCNNet(n_layers).propagate(views, e0)
    got.backward(up)
    mean, tol = sg.propagate_each(adj.indptr, adj.indices, [v.values for v in views], e0.detach())
    r_fwd = sr.ratio(got.detach(), mean, tol)
    e64 = e0.detach().double().requires_grad_(True)
    m64 = sg._mean_layers([_dense(adj, v.values) for v in views], e64)
    m64.backward(up.double())
    np.testing.assert_allclose(mean.cpu().numpy(), m64.detach().cpu().numpy(), rtol=1e-12, atol=1e-14)
    want, tol_b = sg.horner_each(adj.indptr, adj.indices, [v.t_values for v in views], up)
    np.testing.assert_allclose(want.cpu().numpy(), e64.grad.cpu().numpy(), rtol=1e-12, atol=1e-14)
    r_bwd = sr.ratio(e0.grad, e64.grad, tol_b)
    print(f'd = {d}, L = {n_layers}, one view per layer: |got - ref| / bound = {r_fwd} forward, {r_bwd} backward')
    assert r_fwd <= 1.0 and r_bwd <= 1.0
    with pytest.raises(ValueError, match='graphs for'):
        ra.graphmodule.LightGCNNet(n_layers + 1).propagate(views, e0)


def test_one_matrix_for_all_layers_keeps_its_bits(ra, adj):
    """A list that names the same graph L times takes the path -- and gives the bits -- of the graph alone."""
    e0, up = _tables(64, 23)
    net = ra.graphmodule.LightGCNNet(3)
    a = net.propagate(adj, e0)
    a.backward(up)
    ga, e0.grad = e0.grad.clone(), None
    b = net.propagate([adj, adj, adj], e0)
    b.backward(up)
    assert torch.equal(a, b) and torch.equal(ga, e0.grad)


def test_spmm_acc_out_leaves_acc_alone(ra, adj):
    g = torch.Generator().manual_seed(29)
    x, acc = torch.randn(N, 64, generator=g).to(DEV), torch.randn(N, 64, generator=g).to(DEV)
    kept, out = acc.clone(), torch.empty_like(acc)
    res = ra.ops.spmm_csr(adj.indptr, adj.indices, adj.values, x, plan=adj.plan, acc=acc, acc_out=out, acc_scale=0.5)
    assert res is out and torch.equal(acc, kept)
    in_place = ra.ops.spmm_csr(adj.indptr, adj.indices, adj.values, x, plan=adj.plan, acc=acc, acc_scale=0.5)
    assert in_place is acc and torch.equal(acc, out)
    h = ra.ops.spmm_csr(adj.indptr, adj.indices, adj.values, x, plan=adj.plan, acc=x, acc_out=torch.empty_like(x))     # acc may be x
    ref = sr.referee(adj.indptr, adj.indices, adj.values, x, acc=x)
    assert sr.bound_ratios(ref, got_acc=h)[1] <= 1.0
    with pytest.raises(ValueError, match='alias'):
        ra.ops.spmm_csr(adj.indptr, adj.indices, adj.values, x, plan=adj.plan, acc=acc, acc_out=x)
    with pytest.raises(ValueError, match='without acc'):
        ra.ops.spmm_csr(adj.indptr, adj.indices, adj.values, x, plan=adj.plan, acc_out=out)
