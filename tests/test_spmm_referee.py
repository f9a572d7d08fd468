"""CPU: the float64 referee of rsa_spmm_csr (tests/spmm_referee.py) is the matrix product it claims to be, an fp32 emulation
of the kernel's order sits well inside its bound, and each of six planted mistakes leaves the bound."""
import numpy as np
import pytest
import torch

import spmm_referee as sr

NU, NI, D, CHUNK = 30, 20, 8, 8


@pytest.fixture(scope='module')
def graph():
    """A 300 x 200-interaction bipartite multigraph over 30 + 20 nodes: the popular items' rows are several chunks of 8 long."""
    users, items = sr.random_bipartite(NU, NI, 300, seed=3)
    indptr, indices, values = sr.norm_adj_csr(users, items, NU, NI)
    g = torch.Generator().manual_seed(4)
    x = torch.randn(NU + NI, D, generator=g)
    acc = torch.randn(NU + NI, D, generator=g)
    scale = torch.rand(NU + NI, generator=g) + 0.5
    deg = indptr[1:] - indptr[:-1]
    assert int(deg.max()) > 5 * CHUNK and int(deg[0]) == 0 and int(deg[NU]) == 0
    return dict(users=users, items=items, indptr=indptr, indices=indices, values=values, x=x, acc=acc, scale=scale)


def test_referee_is_the_dense_normalised_product(graph):
    g = graph
    dense = sr.dense_norm_adj(g['users'], g['items'], NU, NI)
    ref = sr.referee(g['indptr'], g['indices'], g['values'], g['x'])
    # values are the float64 formula rounded to fp32 once: the two products differ by that rounding and nothing else
    np.testing.assert_allclose(ref['y'].numpy(), (dense @ g['x'].double()).numpy(), rtol=0, atol=float(2 * sr.U32 * ref['A'].max()))
    assert torch.equal(sr.csr_dense(g['indptr'], g['indices'], g['values'], NU + NI),
                       sr.csr_dense(g['indptr'], g['indices'], g['values'], NU + NI).t())
    np.testing.assert_allclose(sr.csr_dense(g['indptr'], g['indices'], g['values'], NU + NI).numpy(), dense.numpy(), rtol=2 * sr.U32)
    # multi-edges are separate entries: as many as interactions, both directions
    assert g['indices'].numel() == 2 * g['users'].numel()
    pairs = torch.stack([sr.edge_rows(g['indptr']), g['indices'].long()])
    assert torch.unique(pairs, dim=1).shape[1] < pairs.shape[1]
    # row_scale, the all-ones values and the accumulation
    ref = sr.referee(g['indptr'], g['indices'], None, g['x'], row_scale=g['scale'], acc=g['acc'], acc_scale=0.25)
    ones = sr.csr_dense(g['indptr'], g['indices'], None, NU + NI)
    want = g['scale'].double().unsqueeze(1) * (ones @ g['x'].double())
    np.testing.assert_allclose(ref['y'].numpy(), want.numpy(), rtol=1e-13, atol=1e-13)
    np.testing.assert_allclose(ref['acc'].numpy(), (0.25 * (g['acc'].double() + want)).numpy(), rtol=1e-13, atol=1e-13)


def test_propagate_is_the_dense_layer_mean(graph):
    g = graph
    a = sr.csr_dense(g['indptr'], g['indices'], g['values'], NU + NI)
    e = g['x'].double()
    want = (e + a @ e + a @ a @ e + a @ a @ a @ e) / 4
    mean, tol = sr.propagate(g['indptr'], g['indices'], g['values'], g['x'], 3)
    np.testing.assert_allclose(mean.numpy(), want.numpy(), rtol=1e-12, atol=1e-14)
    assert float(tol.min()) >= 0 and float(tol.max()) < 1e-4


def _ratios(g, mistake=None, matrix=None, **kw):
    indptr, indices, values = matrix or (g['indptr'], g['indices'], g['values'])
    ref = sr.referee(g['indptr'], g['indices'], g['values'], g['x'], row_scale=g['scale'], acc=g['acc'], acc_scale=0.25)
    y, acc = sr.emulate_fp32(indptr, indices, values, g['x'], CHUNK, row_scale=g['scale'], acc=g['acc'], acc_scale=0.25,
                             mistake=mistake, **kw)
    return sr.bound_ratios(ref, torch.from_numpy(y), torch.from_numpy(acc))


def test_fp32_emulation_stays_within_half_the_bound(graph):
    ry, racc = _ratios(graph)
    assert 0 < ry <= 0.5 and 0 < racc <= 0.5, (ry, racc)


@pytest.mark.parametrize('mistake', ['drop_last', 'twice', 'no_scale_split', 'no_acc_scale'])
def test_planted_arithmetic_mistakes_leave_the_bound(graph, mistake):
    ry, racc = _ratios(graph, mistake)
    assert racc > 1.0, (mistake, ry, racc)
    if mistake != 'no_acc_scale':
        assert ry > 1.0, (mistake, ry, racc)


def test_collapsed_duplicate_edges_leave_the_bound(graph):
    g = graph
    rows = sr.edge_rows(g['indptr'])
    key = rows * (NU + NI) + g['indices'].long()
    first = torch.ones_like(key, dtype=torch.bool)
    order = torch.sort(key, stable=True).indices
    first[order[1:]] = key[order[1:]] != key[order[:-1]]
    keep = first.nonzero().view(-1)
    cnt = torch.bincount(rows[keep], minlength=NU + NI)
    indptr = torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(cnt, 0)])
    ry, racc = _ratios(g, matrix=(indptr, g['indices'][keep], g['values'][keep]))
    assert ry > 1.0 and racc > 1.0


def test_transposed_csr_of_a_non_symmetric_matrix_leaves_the_bound(graph):
    """The backward multiplies by the transposed matrix; for the symmetric normalised adjacency the two CSRs coincide (and the
    emulation over the transposed arrays stays inside the bound), for a one-directional graph they do not."""
    g = graph
    n = NU + NI
    t = sr.csr_transpose(g['indptr'], g['indices'], g['values'], n)
    assert all(torch.equal(a, b) for a, b in zip(sr.csr_sorted_edges(*t, n), sr.csr_sorted_edges(g['indptr'], g['indices'], g['values'], n)))
    ry, racc = _ratios(g, matrix=t)
    assert ry <= 0.5 and racc <= 0.5
    rows = g['users'].long()
    cols = g['items'].long() + NU                       # user -> item only
    order = torch.sort(cols, stable=True).indices
    cnt = torch.bincount(cols, minlength=n)
    indptr = torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(cnt, 0)])
    one_way = dict(g, indptr=indptr, indices=rows[order].int(), values=torch.rand(rows.numel(), generator=torch.Generator().manual_seed(5)))
    ry, racc = _ratios(one_way)
    assert ry <= 0.5 and racc <= 0.5
    ry, racc = _ratios(one_way, matrix=sr.csr_transpose(one_way['indptr'], one_way['indices'], one_way['values'], n))
    assert ry > 1.0 and racc > 1.0


def test_lightgcn_step_referee_matches_its_parts(graph):
    """The float64 step: BPR with one negative is -mean(logsigmoid(pos - neg)); the regulariser's gradient lands on the base rows of
    the batch only; the propagated tables are the layer mean."""
    g = graph
    adj = sr.dense_norm_adj(g['users'], g['items'], NU, NI)
    gen = torch.Generator().manual_seed(6)
    ue, ie = torch.randn(NU, D, generator=gen) * 0.1, torch.randn(NI, D, generator=gen) * 0.1
    uid, pos = torch.randint(1, NU, (16,), generator=gen), torch.randint(1, NI, (16,), generator=gen)
    neg = torch.randint(1, NI, (16, 1), generator=gen)
    out = sr.lightgcn_step(ue, ie, adj, 2, uid, pos, neg, 0.0)
    mean, _ = sr.propagate(*sr.norm_adj_csr(g['users'], g['items'], NU, NI), torch.cat([ue, ie]), 2)
    np.testing.assert_allclose(torch.cat([out['users'], out['items']]).numpy(), mean.numpy(), atol=1e-8)
    want = -torch.nn.functional.logsigmoid(out['pos_score'] - out['neg_score'][:, 0]).mean()
    np.testing.assert_allclose(float(out['loss']), float(want), rtol=1e-12)
    many = sr.lightgcn_step(ue, ie, adj, 2, uid, pos, torch.randint(1, NI, (16, 5), generator=gen), 0.0)
    want = -torch.nn.functional.logsigmoid(many['pos_score'].view(-1, 1) - many['neg_score']).mean(-1).mean()
    np.testing.assert_allclose(float(many['loss']), float(want), rtol=1e-12)
    reg = sr.lightgcn_step(ue, ie, adj, 2, uid, pos, neg, 0.5)
    extra_u = reg['user_grad'] - out['user_grad']
    want_u = torch.zeros(NU, D, dtype=torch.float64).index_add_(0, uid, 0.5 * 2 * ue[uid].double() / 16)
    np.testing.assert_allclose(extra_u.numpy(), want_u.numpy(), atol=1e-15)
