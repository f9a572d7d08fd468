"""GPU: LightGCN (retriever.LightGCN over graphmodule.NormAdj / rsa_spmm_csr) against the float64 referee of
tests/spmm_referee.py: the propagated tables, one training step's loss and gradients on the ids the kernel drew, the gradient
of the propagation alone, the top-k of evaluate, and a short fit next to the same model on torch.sparse.mm and the plugin tail."""
import numpy as np
import pytest
import torch

import spmm_referee as sr
from test_dataset_golden import make

pytestmark = pytest.mark.gpu
DEV = 'cuda'
NU, NI, D, B = 41, 61, 64, 32          # 40 users and 60 items behind the two padding ids


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


def build(ra, data, n_layers, n_neg, cls=None, chunk=None):
    m = (cls or ra.LightGCN)({'model': {'embed_dim': D, 'n_layers': n_layers, 'spmm_chunk': chunk}, 'train': {'negative_count': n_neg}})
    m._init_model(data)
    m._init_parameter()
    return m.to(DEV)


def batch_of(data, size, seed):
    g = torch.Generator().manual_seed(seed)
    rows = data.inter_feat_subset[torch.randperm(len(data), generator=g)[:size]]
    return {data.fuid: data.inter_feat[data.fuid][rows].to(DEV), data.fiid: data.inter_feat[data.fiid][rows].to(DEV),
            data.frating: data.inter_feat[data.frating][rows].to(DEV)}


def adjacency(m):
    a = m.adj_mat
    return a.indptr.to(DEV), a.indices.to(DEV), a.values.to(DEV)


def check_step(ra, data, n_layers, n_neg, chunk):
    m = build(ra, data, n_layers, n_neg, chunk=chunk)
    csr = adjacency(m)
    e0 = torch.cat([m.user_emb.weight, m.item_emb.weight]).detach()
    # the propagated tables, to the bound carried through the layers
    with torch.no_grad():
        m.update_encoders()
        got = torch.cat([m.query_encoder.user_embeddings, m.item_encoder.item_embeddings])
    mean, tol = sr.propagate(*csr, e0, n_layers)
    r = sr.ratio(got, mean, tol)
    print(f'propagated tables, L = {n_layers}: |got - ref| / bound = {r}')
    assert r <= 1.0
    # one training step on the ids the kernel draws for this seed
    batch = batch_of(data, B, seed=5)
    torch.manual_seed(99)
    with torch.no_grad():
        neg = m.forward(batch)['neg_id']
    assert neg.shape == (B, n_neg) and int(neg.min()) >= 1 and int(neg.max()) < m.num_items
    torch.manual_seed(99)
    loss = m.training_step(batch)
    loss.backward()
    adj = sr.csr_dense(*(t.cpu() for t in csr), m.num_users + m.num_items).to(DEV)
    ref = sr.lightgcn_step(m.user_emb.weight, m.item_emb.weight, adj, n_layers, batch[data.fuid], batch[data.fiid], neg,
                           m.config['model']['l2_reg_weight'])
    loss = loss.detach()
    rel = abs(float(loss) - float(ref['loss'])) / abs(float(ref['loss']))
    eu = float((m.user_emb.weight.grad.double() - ref['user_grad']).abs().max() / ref['user_grad'].abs().max())
    ei = float((m.item_emb.weight.grad.double() - ref['item_grad']).abs().max() / ref['item_grad'].abs().max())
    print(f'step L = {n_layers} n = {n_neg}: loss {float(loss):.7f} vs {float(ref["loss"]):.7f} (rel {rel:.2e}), '
          f'grad error / largest element: users {eu:.2e}, items {ei:.2e}')
    assert rel <= 1e-4 and eu <= 3e-4 and ei <= 3e-4
    return m


@pytest.mark.parametrize('n_layers', [1, 2, 3])
@pytest.mark.parametrize('n_neg', [1, 64])
def test_step_against_float64_small_graph(ra, small, n_layers, n_neg):
    m = check_step(ra, small, n_layers, n_neg, chunk=8)
    assert m.adj_mat.plan.n_split > 0                                   # the small graph reaches the split path


@pytest.mark.parametrize('n_neg', [1, 64])
def test_step_against_float64_ml100k(ra, ml100k, n_neg):
    check_step(ra, ml100k[0], 3, n_neg, chunk=None)


@pytest.mark.parametrize('n_layers', [1, 2, 3])
def test_gradient_of_propagate_alone(ra, small, n_layers):
    adj = ra.graphmodule.NormAdj.from_dataset(small, chunk=8)
    net = ra.graphmodule.LightGCNNet(n_layers)
    g = torch.Generator().manual_seed(17)
    e0 = torch.randn(NU + NI, D, generator=g).to(DEV).requires_grad_(True)
    up = torch.randn(NU + NI, D, generator=g).to(DEV)
    net.propagate(adj, e0).backward(up)
    csr = (adj.indptr, adj.indices, adj.values)
    dense = sr.csr_dense(*(t.cpu() for t in csr), NU + NI).to(DEV)
    e64 = e0.detach().double().requires_grad_(True)
    x = s = e64
    for _ in range(n_layers):
        x = dense @ x
        s = s + x
    (s / (n_layers + 1)).backward(up.double())
    # the referee of the backward: the same layer mean over the transposed (= the same) matrix on the incoming gradient
    want, tol = sr.propagate(*csr, up, n_layers)
    np.testing.assert_allclose(want.cpu().numpy(), e64.grad.cpu().numpy(), rtol=1e-12, atol=1e-14)
    r = sr.ratio(e0.grad, e64.grad, tol)
    print(f'propagate backward, L = {n_layers}: |got - autograd| / bound = {r}')
    assert r <= 1.0


def test_evaluate_topk_runs_the_fullscore_kernel(ra, ml100k, monkeypatch):
    trn, _, tst = ml100k
    m = build(ra, trn, 3, 1)
    m.eval()
    calls = []
    real = ra.ops.fullscore
    monkeypatch.setattr(ra.ops, 'fullscore', lambda *a, **kw: calls.append(kw.get('k')) or real(*a, **kw))
    monkeypatch.setattr(torch, 'topk', lambda *a, **kw: pytest.fail('the materialised torch.topk branch was taken'))
    k = 20
    batch = next(iter(tst.eval_loader(batch_size=64)))
    batch = m._to_device(batch, torch.device(DEV))
    with torch.no_grad():
        m._update_item_vector()
        score, ids = m.topk(batch, k, batch['user_hist'])
    monkeypatch.undo()
    assert calls and m.item_vector.shape == (trn.num_items - 1, D)
    mean, _ = sr.propagate(*adjacency(m), torch.cat([m.user_emb.weight, m.item_emb.weight]).detach(), 3)
    users, items = mean[:m.num_users], mean[m.num_users:]
    full = users[batch[trn.fuid]] @ items.t()
    full[:, 0] = -np.inf
    full.scatter_(1, batch['user_hist'], -np.inf)                        # (the padding of a history row is id 0 again)
    want_s, want_i = torch.topk(full, k)
    np.testing.assert_allclose(score.cpu().numpy(), want_s.cpu().numpy(), rtol=1e-4, atol=1e-7)
    np.testing.assert_allclose(torch.gather(full, 1, ids).cpu().numpy(), want_s.cpu().numpy(), rtol=1e-4, atol=1e-7)
    gap = torch.minimum((want_s[:, :-1] - want_s[:, 1:]), torch.cat([want_s.new_full((len(want_s), 1), np.inf),
                                                                     want_s[:, :-2] - want_s[:, 1:-1]], 1))
    clear = torch.cat([gap > 1e-5 * want_s[:, :-1].abs().clamp_min(1e-3), torch.zeros(len(want_s), 1, dtype=torch.bool, device=DEV)], 1)
    assert int(clear.sum()) > clear.numel() // 2 and torch.equal(ids[clear], want_i[clear])


def test_fit_next_to_torch_sparse_mm(ra, ml100k):
    """3 epochs on ml-100k (stock config: adam, lr 1e-3, one negative) next to the same model with torch.sparse.mm as its
    propagation and the per-plugin tail (sampler, indexing encoders, scorer), from the same seed: the same rule in another
    summation order."""
    trn, val, tst = ml100k

    class SparseMM(ra.LightGCN):
        def _propagate(self, e):
            a = self.adj_mat
            if not hasattr(self, '_coo'):
                rows = sr.edge_rows(a.indptr.cpu())
                self._coo = torch.sparse_coo_tensor(torch.stack([rows, a.indices.cpu().long()]), a.values.cpu(),
                                                    (a.n_nodes, a.n_nodes)).coalesce().to(e.device)
            x = s = e
            for _ in range(self.config['model']['n_layers']):
                x = torch.sparse.mm(self._coo, x)
                s = s + x
            return s / (self.config['model']['n_layers'] + 1)

        def forward(self, batch, full_score=False, **kw):
            self.update_encoders()
            return self._forward_plugins(batch, full_score, False, False, False, True)

    cfg = {'model': {'embed_dim': D}, 'train': {'epochs': 3, 'learner': 'adam', 'learning_rate': 0.001}, 'eval': {'batch_size': 256}}
    runs = {}
    for name, cls in (('hip', ra.LightGCN), ('torch', SparseMM)):
        model = cls(cfg)
        model.fit(trn, val)
        assert hasattr(model, '_coo') == (name == 'torch')               # the second run did propagate through torch.sparse.mm
        runs[name] = ([h['train_loss'] for h in model.history], model.evaluate(tst, verbose=False))
        print(name, runs[name][0], {k: round(v, 4) for k, v in runs[name][1].items() if k.endswith('@20')})
    hip, ref = runs['hip'][0], runs['torch'][0]
    assert len(hip) == 3 and all(abs(a - b) <= 0.02 * abs(b) for a, b in zip(hip, ref)), (hip, ref)
    assert hip[0] > hip[1] > hip[2]
    assert runs['hip'][1]['recall@20'] > 0.05
