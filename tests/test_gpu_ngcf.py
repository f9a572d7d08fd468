"""GPU: NGCF (retriever.NGCF over graphmodule.LeftAdj / NGCFNet: rsa_spmm_csr + rsa_bi_combine) against the float64 referee of
tests/ngcf_referee.py: the table and the gradients of the propagation layer by layer from the kernels' own previous layer, one
training step against the dense float64 step on the mask, uniforms and negatives the kernels drew, the random streams against a
torch-op twin, evaluation, the top-k of evaluate, and a short fit next to the same model on torch ops."""
import numpy as np
import pytest
import torch

import ngcf_referee as nr
import spmm_referee as sr
from test_dataset_golden import make

pytestmark = pytest.mark.gpu
DEV = 'cuda'
NU, NI, B = 41, 61, 32
N = NU + NI
F64 = torch.float64


@pytest.fixture(scope='module')
def ra():
    import recstudio_amd
    recstudio_amd._native.lib()
    torch.cuda.init()
    return recstudio_amd


@pytest.fixture(scope='module')
def small(ra):
    users, items = sr.random_bipartite(NU, NI, 400, seed=7)
    return ra.TripletDataset.from_mapped_ids(users, items, n_users=NU, n_items=NI)


@pytest.fixture(scope='module')
def ml100k(ra, golden):
    ra.seed_everything(2022)
    return make(ra.TripletDataset, golden('data_ml100k')).build(split_ratio=[0.8, 0.1, 0.1], shuffle=True)


def generator(seed):
    gen = torch.Generator(device=DEV)
    gen.manual_seed(seed)
    return gen


def make_net(ra, layer_size, dropout, seed):
    torch.manual_seed(seed)
    layers = [ra.graphmodule.BiCombiner(a, b, dropout=dropout) for a, b in zip(layer_size[:-1], layer_size[1:])]
    for c in layers:                                   # biases away from 0, so that no pre-activation is 0 by construction
        torch.nn.init.uniform_(c.linear_sum.bias, -0.1, 0.1)
        torch.nn.init.uniform_(c.linear_product.bias, -0.1, 0.1)
    return ra.graphmodule.NGCFNet(layers).to(DEV)


def layer_params(c):
    return [c.linear_sum.weight.detach(), c.linear_sum.bias.detach(), c.linear_product.weight.detach(), c.linear_product.bias.detach()]


def dense_left(adj):
    """The float64 aggregation matrix of a LeftAdj from ITS mask (the kernel's), by the documented rule."""
    b = adj.base
    dst = sr.edge_rows(b.indptr.cpu())
    keep = None if adj.keep is None else adj.keep.cpu().bool()
    return nr.left_adjacency(dst, b.indices.cpu().long(), adj.n_nodes, keep)


@pytest.mark.parametrize('layer_size', [[64, 64, 64, 64], [64, 32, 16]], ids=str)
@pytest.mark.parametrize('node_dropout', [None, 0.2])
def test_table_and_gradient_layer_by_layer(ra, small, layer_size, node_dropout):
    gm, ops = ra.graphmodule, ra.ops
    base = gm.NormAdj.from_dataset(small, chunk=8).to(DEV)
    assert base.plan.n_split > 0                                        # one long row across the chunk boundary
    adj = gm.LeftAdj(base).to(DEV) if node_dropout is None else gm.LeftAdj.thinned(base, 1.0 - node_dropout, generator(3))
    A = dense_left(adj)
    if node_dropout is not None:
        assert not torch.equal(A, A.T) and 0 < int(adj.keep.sum()) < adj.nnz
        kept_out = torch.bincount(base.indices.long()[adj.keep.bool()], minlength=N)
        assert torch.equal(adj.out_deg.long(), kept_out) and int((kept_out == 0).sum()) >= 2     # (a degree 0 counted as 1 occurs: the padding nodes)
    p = 0.1
    net = make_net(ra, layer_size, p, seed=21)
    g_in = torch.Generator().manual_seed(5)
    x0 = (torch.rand(N, layer_size[0], generator=g_in) * 2 - 1).to(DEV).requires_grad_()
    G = torch.randn(N, sum(layer_size), generator=g_in).to(DEV)
    table = net.propagate(adj, x0, generator=generator(77))
    table.backward(G)
    # ---- the same launches one by one, from the same generator state: every layer judged on the kernels' own inputs
    gen, twin = generator(77), generator(77)
    csr = (base.indptr, base.indices)
    x, col, blocks, kept = x0.detach(), layer_size[0], [x0.detach()], []
    for k, c in enumerate(net.combiners):
        m = adj.aggregate(x)
        r = sr.bound_ratios(sr.referee(*csr, adj.values, x), got_y=m)[0]
        w1, b1, w2, b2 = layer_params(c)
        wide = torch.zeros(N, c.output_size + 4, device=DEV)
        pc = ra.rng.reserve(N * c.output_size, 4, torch.device(DEV), gen)
        h = ops.bi_combine(x, m, w1, w2, b1, b2, negative_slope=c.negative_slope, p=p, philox=pc, out=wide, col=4)
        u = torch.rand(N, c.output_size, device=DEV, generator=twin)
        args = [t.cpu() for t in (x, m, w1, b1, w2, b2)]
        f = nr.layer_forward(*args, c.negative_slope, p, u.cpu())
        fb = nr.layer_forward_bounds(*args, f)
        wh, wn = nr.worst(h, f['h'], fb['h']), nr.worst(wide[:, 4:], f['n'], fb['n'])
        print(f'layer {k + 1} {c.input_size}x{c.output_size}: |got - ref| / bound  m {r:.3f}  h {wh:.3f}  n {wn:.3f}')
        assert r <= 1 and wh <= 1 and wn <= 1
        kept.append((x, m, pc, u.cpu(), args, f, fb))
        blocks.append(wide[:, 4:])
        x = h
    assert torch.equal(table.detach(), torch.cat(blocks, 1))
    assert gen.get_offset() == twin.get_offset()
    # ---- the backward, from layer L down
    g_h, col, grads = None, sum(layer_size), {}
    for k in range(len(net.combiners) - 1, -1, -1):
        c = net.combiners[k]
        x, m, pc, u, args, f, fb = kept[k]
        col -= c.output_size
        assert nr.preact_margin(f, fb) >= 2                             # a condition on the inputs: every slope is decided
        w1, b1, w2, b2 = layer_params(c)
        got = ops.bi_combine_backward(x, m, w1, w2, b1, b2, g_h=g_h, g_out=G, col=col, negative_slope=c.negative_slope, p=p, philox=pc)
        gh_cpu = None if g_h is None else g_h.cpu()
        gn_cpu = G[:, col:col + c.output_size].cpu()
        b = nr.layer_backward(*args, f, gh_cpu, gn_cpu, c.negative_slope)
        bb = nr.layer_backward_bounds(*args, f, fb, b, gh_cpu, gn_cpu, c.negative_slope)
        names = ('dx', 'dm', 'dw1', 'dw2', 'db1', 'db2')
        ratios = {name: nr.worst(t, b[name], bb[name]) for name, t in zip(names, got)}
        dx, dm = got[0], got[1]
        want = sr.referee(*csr, adj.t_keep, dm, row_scale=adj.inv_out, acc=dx)
        g_h = adj.aggregate_grad(dm, dx.clone())
        ratios['A^T dm'] = sr.bound_ratios(want, got_acc=g_h)[1]
        print(f'layer {k + 1} backward: |got - ref| / bound ', '  '.join(f'{n} {v:.3f}' for n, v in ratios.items()))
        assert max(ratios.values()) <= 1, ratios
        grads[k] = got[2:]
    assert torch.equal(x0.grad, g_h + G[:, :layer_size[0]])
    for k, c in enumerate(net.combiners):
        dw1, dw2, db1, db2 = grads[k]
        assert torch.equal(c.linear_sum.weight.grad, dw1) and torch.equal(c.linear_product.weight.grad, dw2)
        assert torch.equal(c.linear_sum.bias.grad, db1) and torch.equal(c.linear_product.bias.grad, db2)
    # ---- and the whole propagation against float64 autograd over the dense matrix, on the same masks
    x64 = x0.detach().cpu().to(F64).requires_grad_()
    params = [tuple(t.cpu().to(F64).requires_grad_() for t in layer_params(c)) for c in net.combiners]
    ref = nr.net_forward(A, x64, params, 0.01, [p] * len(params), [kk[3] for kk in kept])
    ref.backward(G.cpu().to(F64))
    assert float((table.detach().cpu() - ref.detach()).abs().max()) <= 1e-4 * float(ref.detach().abs().max())
    assert float((x0.grad.cpu() - x64.grad).abs().max()) <= 3e-4 * float(x64.grad.abs().max())
    for c, (w1, b1, w2, b2) in zip(net.combiners, params):
        for got, want in ((c.linear_sum.weight, w1), (c.linear_sum.bias, b1), (c.linear_product.weight, w2), (c.linear_product.bias, b2)):
            assert float((got.grad.cpu() - want.grad).abs().max()) <= 3e-4 * float(want.grad.abs().max())


def build(ra, data, **model):
    cfg = {'model': dict({'spmm_chunk': 8}, **model), 'train': {'negative_count': 1}}
    m = ra.NGCF(cfg)
    m._init_model(data)
    m._init_parameter()
    return m.to(DEV)


def batch_of(data, size, seed):
    g = torch.Generator().manual_seed(seed)
    rows = data.inter_feat_subset[torch.randperm(len(data), generator=g)[:size]]
    return {data.fuid: data.inter_feat[data.fuid][rows].to(DEV), data.fiid: data.inter_feat[data.fiid][rows].to(DEV),
            data.frating: data.inter_feat[data.frating][rows].to(DEV)}


@pytest.mark.parametrize('node_dropout', [0.1, None])
def test_training_step_against_dense_float64(ra, small, node_dropout):
    """Loss within 1e-4, every parameter gradient (both tables, the Linears) within 3e-4 of its largest element, on the mask, the
    uniforms and the negatives the kernels drew; and those three against torch calls from the same seed, in the documented order."""
    m = build(ra, small, node_dropout=node_dropout)
    for c in m.combiners:
        torch.nn.init.uniform_(c.linear_sum.bias, -0.1, 0.1)
        torch.nn.init.uniform_(c.linear_product.bias, -0.1, 0.1)
    m.train()
    batch = batch_of(small, B, seed=5)
    torch.manual_seed(99)
    loss = m.training_step(batch)
    loss.backward()
    # the twin of the step's random stream: the edge mask, the L dropout calls, the negatives
    torch.manual_seed(99)
    base = m.adj_mat
    if node_dropout:
        u_e = torch.rand(base.nnz, device=DEV)
        keep = torch.floor(u_e + torch.tensor(1.0 - node_dropout, dtype=torch.float32, device=DEV)) != 0
        assert torch.equal(m.last_view.keep.bool(), keep)
        adj = m.last_view
    else:
        adj = m.left_adj
        assert m.last_view is None
    us = [torch.rand(N, c.output_size, device=DEV).cpu() for c in m.combiners]
    neg = torch.randint(1, m.num_items, (B, 1), device=DEV)
    with torch.no_grad():
        torch.manual_seed(99)
        assert torch.equal(m.forward(batch)['neg_id'], neg)
    ref = nr.ngcf_step(m.user_emb.weight.cpu(), m.item_emb.weight.cpu(), dense_left(adj), [layer_params(c) for c in m.combiners],
                       batch[small.fuid].cpu(), batch[small.fiid].cpu(), neg.cpu(), m.config['model']['l2_reg_weight'],
                       ps=[c.dropout for c in m.combiners], us=us)
    rel = abs(float(loss.detach()) - float(ref['loss'])) / abs(float(ref['loss']))
    errs = {'users': (m.user_emb.weight.grad, ref['user_grad']), 'items': (m.item_emb.weight.grad, ref['item_grad'])}
    for k, (c, lg) in enumerate(zip(m.combiners, ref['layer_grads'])):
        for name, got, want in (('w1', c.linear_sum.weight, lg[0]), ('b1', c.linear_sum.bias, lg[1]),
                                ('w2', c.linear_product.weight, lg[2]), ('b2', c.linear_product.bias, lg[3])):
            errs[f'{name}[{k}]'] = (got.grad, want)
    errs = {k: float((a.cpu().double() - b).abs().max() / b.abs().max()) for k, (a, b) in errs.items()}
    print(f'step node_dropout={node_dropout}: loss {float(loss.detach()):.7f} vs {float(ref["loss"]):.7f} (rel {rel:.2e}); grad error / largest '
          'element: ' + '  '.join(f'{k} {v:.1e}' for k, v in errs.items()))
    assert rel <= 1e-4 and max(errs.values()) <= 3e-4, errs


def test_eval_is_deterministic_and_the_full_graph(ra, small):
    m = build(ra, small)
    m.eval()
    state = torch.cuda.default_generators[torch.cuda.current_device()].get_offset()
    with torch.no_grad():
        m.update_encoders()
        first = torch.cat([m.query_encoder.user_embeddings, m.item_encoder.item_embeddings]).clone()
        m.update_encoders()
        again = torch.cat([m.query_encoder.user_embeddings, m.item_encoder.item_embeddings])
    assert torch.equal(first, again) and first.shape == (N, 256)
    assert torch.cuda.default_generators[torch.cuda.current_device()].get_offset() == state           # nothing drawn
    x0 = torch.cat([m.user_emb.weight, m.item_emb.weight]).detach().cpu().to(F64)
    ref = nr.net_forward(dense_left(m.left_adj), x0, [[t.cpu().to(F64) for t in layer_params(c)] for c in m.combiners])
    assert float((first.cpu() - ref).abs().max()) <= 1e-4 * float(ref.abs().max())
    with torch.no_grad():
        twin = m.NGCFNet.propagate_torch(m.left_adj, torch.cat([m.user_emb.weight, m.item_emb.weight]))
    assert float((first - twin).abs().max()) <= 1e-4 * float(twin.abs().max())


def test_evaluate_topk_on_the_256_wide_table(ra, ml100k, monkeypatch):
    trn, _, tst = ml100k
    m = build(ra, trn, spmm_chunk=None)
    m.eval()
    calls = []
    real = ra.ops.fullscore
    monkeypatch.setattr(ra.ops, 'fullscore', lambda *a, **kw: calls.append(kw.get('k')) or real(*a, **kw))
    monkeypatch.setattr(torch, 'topk', lambda *a, **kw: pytest.fail('the materialised torch.topk branch was taken'))
    k = 20
    batch = m._to_device(next(iter(tst.eval_loader(batch_size=64))), torch.device(DEV))
    with torch.no_grad():
        m._update_item_vector()
        score, ids = m.topk(batch, k, batch['user_hist'])
    monkeypatch.undo()
    assert calls and m.item_vector.shape == (trn.num_items - 1, 256)
    users, items = m.query_encoder.user_embeddings.double(), m.item_encoder.item_embeddings.double()
    full = users[batch[trn.fuid]] @ items.t()
    full[:, 0] = -np.inf
    full.scatter_(1, batch['user_hist'], -np.inf)
    want_s, _ = torch.topk(full, k)
    np.testing.assert_allclose(score.cpu().numpy(), want_s.cpu().numpy(), rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(torch.gather(full, 1, ids).cpu().numpy(), want_s.cpu().numpy(), rtol=1e-4, atol=1e-6)


def test_fit_next_to_torch_ops(ra, ml100k):
    """3 epochs on ml-100k (adam, lr 1e-3) next to the same model with NGCFNet.propagate_torch (torch.sparse.mm, nn.Linear,
    F.normalize, the same mask rule) and the per-plugin tail, from the same seed; judged as the LightGCN fit test judges its
    pair: every epoch's training loss within 2 % and a recall@20 above 0.05."""
    trn, val, tst = ml100k

    class TorchOps(ra.NGCF):
        def _propagate(self, e):
            self.used_torch = True
            drop = self.config['model']['node_dropout']
            adj = self.left_adj
            if self.training and drop:
                self.adj_mat.to(e.device)
                adj = ra.graphmodule.LeftAdj.thinned(self.adj_mat, 1.0 - float(drop))
            adj.to(e.device)
            return self.NGCFNet.propagate_torch(adj, e)

        def forward(self, batch, full_score=False, **kw):
            self.update_encoders()
            return self._forward_plugins(batch, full_score, False, False, False, True)

    cfg = {'train': {'epochs': 3, 'learner': 'adam', 'learning_rate': 0.001}, 'eval': {'batch_size': 256}}
    runs = {}
    for name, cls in (('hip', ra.NGCF), ('torch', TorchOps)):
        model = cls(cfg)
        model.fit(trn, val)
        assert hasattr(model, 'used_torch') == (name == 'torch')
        runs[name] = ([h['train_loss'] for h in model.history], model.evaluate(tst, verbose=False))
        print(name, runs[name][0], {k: round(v, 4) for k, v in runs[name][1].items() if k.endswith('@20') or k.endswith('@10')})
    hip, ref = runs['hip'][0], runs['torch'][0]
    assert len(hip) == 3 and all(abs(a - b) <= 0.02 * abs(b) for a, b in zip(hip, ref)), (hip, ref)
    assert hip[0] > hip[1] > hip[2]
    assert runs['hip'][1]['recall@20'] > 0.05


def test_a_step_does_not_outlive_itself(ra, small):
    """Every step's thinned view ([nnz] values, mask and degrees) and its autograd nodes are gone once the next step has replaced
    them, without a collector run: the fused score node keeps no reference to its own outputs (it once did, and every node upstream
    of it -- this model's propagation with its per-step view -- stayed alive for good, 1.1 GB per step on 2**27 edges)."""
    import gc
    import weakref
    m = build(ra, small)
    m.train()
    batch = batch_of(small, B, seed=5)
    views, tables = [], []
    gc.disable()
    try:
        for _ in range(3):
            for t in m.parameters():
                t.grad = None
            loss = m.training_step(batch)
            loss.backward()
            views.append(weakref.ref(m.last_view))
            tables.append(weakref.ref(m.query_encoder.user_embeddings))
    finally:
        gc.enable()
    assert [r() is not None for r in views] == [False, False, True]
    assert [r() is not None for r in tables] == [False, False, True]
