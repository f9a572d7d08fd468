"""GPU: SimGCL (retriever.SimGCL over graphmodule.SimGCLNet / the perturbed rsa_spmm_csr and data_augmentation.SimGCLAugmentation)
against the float64 referee of tests/simgcl_referee.py: the propagation layer by layer, its gradient, one training step's loss and
gradients on the negatives and uniforms the kernels drew, the device stream of a step next to a torch-op twin, the top-k of
evaluate, and a short fit next to the same model written with torch.sparse.mm / rand_like / normalize / sign."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import simgcl_referee as sc
import spmm_referee as sr
from test_dataset_golden import make

pytestmark = pytest.mark.gpu
DEV = 'cuda'
NU, NI, D, B, EPS, CAP = 41, 61, 64, 32, 0.1, 1e-4
N = NU + NI


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
def adjs(ra, small):
    """The symmetric interaction graph (chunk 8: it has split rows) and a random non-symmetric one."""
    g = torch.Generator().manual_seed(9)
    one_way = ra.graphmodule.NormAdj(torch.randint(0, N, (700,), generator=g), torch.randint(0, N, (700,), generator=g), N, chunk=8)
    sym = ra.graphmodule.NormAdj.from_dataset(small, chunk=8)
    assert sym.symmetric and not one_way.symmetric and sym.plan.n_split > 0 and one_way.plan.n_split > 0
    return {'symmetric': sym.to(DEV), 'one-way': one_way.to(DEV)}


@pytest.fixture(scope='module')
def ml100k(ra, golden):
    ra.seed_everything(2022)
    return make(ra.TripletDataset, golden('data_ml100k')).build(split_ratio=[0.8, 0.1, 0.1], shuffle=True)


def gen():
    return torch.cuda.default_generators[torch.cuda.current_device()]


def coo_of(a, device):
    rows = sr.edge_rows(a.indptr.cpu())
    return torch.sparse_coo_tensor(torch.stack([rows, a.indices.cpu().long()]), a.values.cpu(), (a.n_nodes, a.n_nodes)).coalesce().to(device)


@pytest.mark.parametrize('d', [4, 64, 128, 256])
@pytest.mark.parametrize('n_layers', [1, 2, 3])
@pytest.mark.parametrize('perturbed', [False, True])
def test_propagate_layer_by_layer(ra, adjs, d, n_layers, perturbed):
    adj = adjs['symmetric']
    csr = (adj.indptr, adj.indices, adj.values)
    net = ra.graphmodule.SimGCLNet(n_layers, EPS)
    e0 = torch.cat(sc.tables(NU, NI, d, seed=3), 0).to(DEV)
    torch.manual_seed(21)
    before = gen().get_offset()
    noise = []
    mean = net.propagate(adj, e0, perturbed=perturbed, noise_out=noise)
    after = gen().get_offset()
    # the layers the kernel itself makes, one y-only launch each on the calls propagate handed out
    torch.manual_seed(21)
    layers, x = [], e0
    if perturbed:
        first = ra.rng.reserve(e0.numel(), 4, torch.device(DEV), repeat=n_layers)
        step = ra.rng.counter_offset(e0.numel(), first.grid_threads, 4)
        assert gen().get_offset() == after == before + n_layers * step
    else:
        assert after == before and not noise
    for k in range(n_layers):
        kw = {'noise': ra.rng.PhiloxCall(first.seed, first.offset + k * step, first.grid_threads), 'noise_eps': EPS} if perturbed else {}
        x = ra.ops.spmm_csr(*csr, x, plan=adj.plan, **kw)
        layers.append(x)
    j = sc.judge_propagation(*csr, e0, layers, mean, noise if perturbed else None, EPS)
    print(f'd = {d}, L = {n_layers}, perturbed {perturbed}: layers {j["ratio"]:.3f}, mean {j["mean_ratio"]:.3f} of the bound, ambiguous {j["share"]:.2e}')
    assert j['ratio'] <= 1.0 and j['mean_ratio'] <= 1.0 and j['share'] <= CAP
    if perturbed:                                                                   # the L tables are L consecutive rand_like calls
        torch.manual_seed(21)
        assert len(noise) == n_layers and all(torch.equal(u, torch.rand_like(e0)) for u in noise)
        assert gen().get_offset() == after
        assert bool((mean[0] == 0).all()) and bool((mean[NU] == 0).all())           # the padding rows have no edges and stay 0
        with torch.no_grad():
            assert float((mean - net.propagate(adj, e0)).abs().max()) > 0.01 * EPS


@pytest.mark.parametrize('d', [4, 64, 128, 256])
@pytest.mark.parametrize('n_layers', [1, 2, 3])
@pytest.mark.parametrize('graph', ['symmetric', 'one-way'])
def test_gradient_of_propagate_alone(ra, adjs, d, n_layers, graph):
    adj = adjs[graph]
    net = ra.graphmodule.SimGCLNet(n_layers, EPS)
    g = torch.Generator().manual_seed(17)
    e0 = torch.randn(N, d, generator=g).to(DEV)
    up = torch.randn(N, d, generator=g).to(DEV)
    want, tol = sc.propagate_grad(adj.t_indptr, adj.t_indices, adj.t_values, up, n_layers)
    if d == 64:                                                                     # the referee is the autograd gradient of the dense float64 mean
        dense = sr.csr_dense(adj.indptr.cpu(), adj.indices.cpu(), adj.values.cpu(), N).to(DEV)
        e64 = e0.double().requires_grad_(True)
        sc.perturbed_mean(dense, e64, n_layers, EPS, [torch.rand_like(e0) for _ in range(n_layers)]).backward(up.double())
        np.testing.assert_allclose(want.cpu().numpy(), e64.grad.cpu().numpy(), rtol=1e-12, atol=1e-14)
    for perturbed in (False, True):
        leaf = e0.clone().requires_grad_(True)
        net.propagate(adj, leaf, perturbed=perturbed).backward(up)
        r = sr.ratio(leaf.grad, want, tol)
        print(f'{graph} d = {d}, L = {n_layers}, perturbed {perturbed}: |got - ref| / bound = {r:.3f}')
        assert r <= 1.0


def build(ra, data, n_layers, n_neg, cls=None, **model):
    torch.manual_seed(1)
    m = (cls or ra.SimGCL)({'model': dict({'embed_dim': D, 'n_layers': n_layers, 'spmm_chunk': 8}, **model), 'train': {'negative_count': n_neg}})
    m._init_model(data)
    m._init_parameter()
    return m.to(DEV)


def batch_of(data, size, seed):
    g = torch.Generator().manual_seed(seed)
    rows = data.inter_feat_subset[torch.randperm(len(data), generator=g)[:size]]
    return {data.fuid: data.inter_feat[data.fuid][rows].to(DEV), data.fiid: data.inter_feat[data.fiid][rows].to(DEV),
            data.frating: data.inter_feat[data.frating][rows].to(DEV)}


_STEPS = {}


def one_step(ra, data, n_layers, n_neg):
    """One training step (seed 99) with its negatives and its 2 L tables of uniforms caught on the way; run once per setting."""
    key = (n_layers, n_neg)
    if key not in _STEPS:
        m = build(ra, data, n_layers, n_neg)
        batch = batch_of(data, B, seed=5)
        torch.manual_seed(99)
        with torch.no_grad():
            neg = m.forward(batch)['neg_id']
        caught, real = [], m.SimGCLNet.propagate

        def spy(adj, emb, perturbed=False, generator=None):
            out = [] if perturbed else None
            if perturbed:
                caught.append(out)
            return real(adj, emb, perturbed=perturbed, generator=generator, noise_out=out)

        m.SimGCLNet.propagate = spy
        torch.manual_seed(99)
        loss = m.training_step(batch)
        offset = gen().get_offset()
        loss.backward()
        _STEPS[key] = (m, batch, neg, caught, loss.detach(), offset)
    return _STEPS[key]


@pytest.mark.parametrize('n_layers', [1, 2, 3])
@pytest.mark.parametrize('n_neg', [1, 64])
def test_step_against_float64(ra, small, n_layers, n_neg):
    m, batch, neg, caught, loss, _ = one_step(ra, small, n_layers, n_neg)
    assert len(caught) == 2 and all(len(v) == n_layers for v in caught)
    adj = m.adj_mat
    dense = sr.csr_dense(adj.indptr.cpu(), adj.indices.cpu(), adj.values.cpu(), N).to(DEV)
    cfg = m.config['model']
    assert cfg['cl_weight'] == 0.5                                                  # accepted, and not applied: the referee adds cl_loss whole
    ref = sc.simgcl_step(m.user_emb.weight, m.item_emb.weight, dense, n_layers, cfg['eps'], batch[small.fuid], batch[small.fiid], neg,
                         caught[0], caught[1], cfg['l2_reg_weight'], cfg['temperature'])
    rel = abs(float(loss) - float(ref['loss'])) / abs(float(ref['loss']))
    eu = float((m.user_emb.weight.grad.double() - ref['user_grad']).abs().max() / ref['user_grad'].abs().max())
    ei = float((m.item_emb.weight.grad.double() - ref['item_grad']).abs().max() / ref['item_grad'].abs().max())
    print(f'L = {n_layers} n = {n_neg}: loss {float(loss):.7f} vs {float(ref["loss"]):.7f} (rel {rel:.2e}; cl {float(ref["cl_loss"]):.4f}), '
          f'grad error / largest element: users {eu:.2e}, items {ei:.2e}')
    assert rel <= 1e-4 and eu <= 3e-4 and ei <= 3e-4


@pytest.mark.parametrize('n_layers', [1, 2, 3])
@pytest.mark.parametrize('n_neg', [1, 64])
def test_the_stream_of_a_step_is_the_torch_twins(ra, small, n_layers, n_neg):
    """randint for the negatives, then L rand_like calls for view 1, then L for view 2 -- drawn by torch ops from the same seed."""
    m, batch, neg, caught, _, offset = one_step(ra, small, n_layers, n_neg)
    coo = coo_of(m.adj_mat, DEV)
    e = torch.cat([m.user_emb.weight, m.item_emb.weight]).detach()
    torch.manual_seed(99)
    twin_neg = torch.randint(1, m.sampler.num_items + 1, (B, n_neg), device=DEV)
    twin = []
    for _ in range(2):
        x, tabs = e, []
        for _ in range(n_layers):
            x = torch.sparse.mm(coo, x)
            tabs.append(torch.rand_like(x))
            x = x + torch.sign(x) * F.normalize(tabs[-1], dim=-1) * EPS
        twin.append(tabs)
    assert torch.equal(neg.view(B, n_neg), twin_neg)
    assert all(torch.equal(a, b) for va, vb in zip(caught, twin) for a, b in zip(va, vb))
    assert not torch.equal(caught[0][0], caught[1][0]) and (n_layers == 1 or not torch.equal(caught[0][0], caught[0][1]))
    assert offset == gen().get_offset()


def test_evaluate_topk_runs_the_fullscore_kernel_on_the_skip_input_table(ra, ml100k, monkeypatch):
    trn, _, tst = ml100k
    torch.manual_seed(1)
    m = ra.SimGCL({'model': {'embed_dim': D, 'n_layers': 3}})
    m._init_model(trn)
    m._init_parameter()
    m = m.to(DEV).eval()
    calls = []
    real = ra.ops.fullscore
    monkeypatch.setattr(ra.ops, 'fullscore', lambda *a, **kw: calls.append(kw.get('k')) or real(*a, **kw))
    monkeypatch.setattr(torch, 'topk', lambda *a, **kw: pytest.fail('the materialised torch.topk branch was taken'))
    k = 20
    batch = next(iter(tst.eval_loader(batch_size=64)))
    batch = m._to_device(batch, torch.device(DEV))
    before = gen().get_offset()
    with torch.no_grad():
        m._update_item_vector()
        score, ids = m.topk(batch, k, batch['user_hist'])
    monkeypatch.undo()
    assert calls and m.item_vector.shape == (trn.num_items - 1, D) and gen().get_offset() == before      # evaluation draws no noise
    a = m.adj_mat
    x, layers = torch.cat([m.user_emb.weight, m.item_emb.weight]).detach().double(), []
    for _ in range(3):
        x = sr.referee(a.indptr, a.indices, a.values.double(), x)['y']
        layers.append(x)
    mean = torch.stack(layers).mean(0)                                              # E_0 is not in it
    users, items = mean[:m.num_users], mean[m.num_users:]
    full = users[batch[trn.fuid]] @ items.t()
    full[:, 0] = -np.inf
    full.scatter_(1, batch['user_hist'], -np.inf)
    want_s, _ = torch.topk(full, k)
    np.testing.assert_allclose(score.cpu().numpy(), want_s.cpu().numpy(), rtol=1e-4, atol=1e-7)
    np.testing.assert_allclose(torch.gather(full, 1, ids).cpu().numpy(), want_s.cpu().numpy(), rtol=1e-4, atol=1e-7)


def test_fit_next_to_torch_ops(ra, ml100k):
    """3 epochs on ml-100k (the stock SimGCL settings) next to the same model whose propagation, plain and perturbed, is
    torch.sparse.mm / rand_like / normalize / sign under autograd and whose tail is the per-plugin one, from the same seed."""
    trn, val, tst = ml100k

    def layers_mean(model, e, eps):
        if not hasattr(model, '_coo'):
            model._coo = coo_of(model.adj_mat, e.device)
        outs = []
        for _ in range(model.config['model']['n_layers']):
            e = torch.sparse.mm(model._coo, e)
            if eps is not None:
                e = e + torch.sign(e) * F.normalize(torch.rand_like(e), dim=-1) * eps
            outs.append(e)
        return torch.stack(outs, dim=-2).mean(dim=-2)

    class TorchAug(ra.data_augmentation.SimGCLAugmentation):
        def get_gnn_embeddings(self, user_emb, item_emb, adj_mat, gnn_net):
            out = layers_mean(self.owner[0], torch.cat([user_emb.weight, item_emb.weight], dim=0), gnn_net.eps)
            self.torch_views = getattr(self, 'torch_views', 0) + 1
            return out[:self.num_users], out[self.num_users:]

    class TorchSimGCL(ra.SimGCL):
        def _init_model(self, train_data, drop_unused_field=True):
            super()._init_model(train_data, drop_unused_field)
            self.augmentation_model = TorchAug(self.config['model'], train_data)
            self.augmentation_model.owner = (self,)                                  # (a tuple: not a submodule)

        def _propagate(self, e):
            return layers_mean(self, e, None)

        def forward(self, batch, full_score=False, **kw):
            self.update_encoders()
            return self._forward_plugins(batch, full_score, False, False, False, True)

    cfg = {'model': {'embed_dim': D}, 'train': {'epochs': 3, 'learner': 'adam'}, 'eval': {'batch_size': 256}}
    runs = {}
    for name, cls in (('hip', ra.SimGCL), ('torch', TorchSimGCL)):
        model = cls(cfg)
        assert model.config['train']['learning_rate'] == 0.001 and model.config['train']['batch_size'] == 2048
        model.fit(trn, val)
        assert hasattr(model, '_coo') == (name == 'torch')
        if name == 'torch':
            assert model.augmentation_model.torch_views > 0
        runs[name] = ([h['train_loss'] for h in model.history], model.evaluate(tst, verbose=False))
        print(name, runs[name][0], {k: round(v, 4) for k, v in runs[name][1].items() if k.endswith('@20')})
    hip, ref = runs['hip'][0], runs['torch'][0]
    assert len(hip) == 3 and all(abs(a - b) <= 0.02 * abs(b) for a, b in zip(hip, ref)), (hip, ref)
    assert hip[0] > hip[1] > hip[2]
    assert runs['hip'][1]['recall@20'] > 0.05
