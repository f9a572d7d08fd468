"""GPU: SGL (retriever.SGL over data_augmentation.SGLAugmentation / rsa_graph_dropout) against the float64 referee of
tests/sgl_referee.py: InfoNCE over a whole table, one training step's loss and gradients on the masks and ids the kernels drew,
and a short fit next to the same model with its views rebuilt by torch ops and propagated by torch.sparse.mm."""
import pytest
import torch

import sgl_referee as sg
import spmm_referee as sr
from test_dataset_golden import make

pytestmark = pytest.mark.gpu
DEV = 'cuda'
NU, NI, D, B = 41, 61, 64, 32


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


def build(ra, data, n_layers, n_neg, cls=None, seed=1, **model):
    torch.manual_seed(seed)
    m = (cls or ra.SGL)({'model': dict({'embed_dim': D, 'n_layers': n_layers, 'spmm_chunk': 8}, **model), 'train': {'negative_count': n_neg}})
    m._init_model(data)
    m._init_parameter()
    return m.to(DEV)


def batch_of(data, size, seed):
    g = torch.Generator().manual_seed(seed)
    rows = data.inter_feat_subset[torch.randperm(len(data), generator=g)[:size]]
    return {data.fuid: data.inter_feat[data.fuid][rows].to(DEV), data.fiid: data.inter_feat[data.fiid][rows].to(DEV),
            data.frating: data.inter_feat[data.frating][rows].to(DEV)}


@pytest.mark.parametrize('sim_method', ['cosine', 'inner_product'])
def test_info_nce_over_the_whole_table(ra, sim_method):
    g = torch.Generator().manual_seed(31)
    scale = 1.0 if sim_method == 'cosine' else 0.3                       # (rows of an embedding table's size, not of unit variance)
    table = (scale * torch.randn(NI, 64, generator=g)).to(DEV).requires_grad_(True)
    other = (scale * torch.randn(NI, 64, generator=g)).to(DEV).requires_grad_(True)
    ids = torch.randint(1, NI, (B,), generator=g).to(DEV)
    loss = ra.data_augmentation.InfoNCELoss(0.2, sim_method, 'all')(other[ids], table[ids], all_reps=table)
    loss.backward()
    t64, o64 = table.detach().double().requires_grad_(True), other.detach().double().requires_grad_(True)
    ref = sg.info_nce(o64[ids], t64[ids], t64, 0.2, sim_method)
    ref.backward()
    loss, ref = loss.detach(), ref.detach()
    rel = abs(float(loss) - float(ref)) / abs(float(ref))
    et = float((table.grad.double() - t64.grad).abs().max() / t64.grad.abs().max())
    eo = float((other.grad.double() - o64.grad).abs().max() / o64.grad.abs().max())
    print(f'InfoNCE {sim_method}: loss {float(loss):.7f} vs {float(ref):.7f} (rel {rel:.2e}), grad error / largest element: table {et:.2e}, query {eo:.2e}')
    assert rel <= 1e-4 and et <= 3e-4 and eo <= 3e-4


def dense_of(adj, values):
    return sr.csr_dense(adj.indptr.cpu(), adj.indices.cpu(), values.cpu(), adj.n_nodes).to(DEV)


@pytest.mark.parametrize('n_layers', [1, 2, 3])
@pytest.mark.parametrize('n_neg', [1, 64])
@pytest.mark.parametrize('aug_type', ['ED', 'ND', 'RW'])
def test_step_against_float64(ra, small, aug_type, n_layers, n_neg):
    m = build(ra, small, n_layers, n_neg, aug_type=aug_type, ssl_ratio=0.3)
    batch = batch_of(small, B, seed=5)
    torch.manual_seed(99)
    with torch.no_grad():
        neg = m.forward(batch)['neg_id']
    torch.manual_seed(99)
    loss = m.training_step(batch)
    loss.backward()
    adj = m.adj_mat
    v1, v2 = m.last_views

    def dense_view(v):
        if isinstance(v, list):
            assert aug_type == 'RW' and len(v) == n_layers
            return [dense_view(x) for x in v]
        keep = v.keep.bool()
        assert 0 < int(keep.sum()) < adj.nnz
        return dense_of(adj, sg.augment(adj.indptr, adj.indices, adj.rev, keep)['values'])

    views = [dense_view(v1), dense_view(v2)]
    first = lambda v: v[0] if isinstance(v, list) else v                 # noqa: E731
    assert not torch.equal(first(v1).keep, first(v2).keep)
    if aug_type == 'ND':                                                # a dropped node loses both directions of all its edges
        assert torch.equal(v1.keep, v1.keep[adj.rev]) and int(v1.keep.sum()) < adj.nnz
    cfg = m.config['model']
    ref = sg.sgl_step(m.user_emb.weight, m.item_emb.weight, dense_of(adj, adj.values), views, n_layers, batch[small.fuid], batch[small.fiid],
                      neg, cfg['l2_reg_weight'], cfg['ssl_reg'], cfg['temperature'])
    loss = loss.detach()
    rel = abs(float(loss) - float(ref['loss'])) / abs(float(ref['loss']))
    eu = float((m.user_emb.weight.grad.double() - ref['user_grad']).abs().max() / ref['user_grad'].abs().max())
    ei = float((m.item_emb.weight.grad.double() - ref['item_grad']).abs().max() / ref['item_grad'].abs().max())
    print(f'{aug_type} L = {n_layers} n = {n_neg}: loss {float(loss):.7f} vs {float(ref["loss"]):.7f} (rel {rel:.2e}; cl {float(ref["cl_loss"]):.4f}), '
          f'grad error / largest element: users {eu:.2e}, items {ei:.2e}')
    assert rel <= 1e-4 and eu <= 3e-4 and ei <= 3e-4


def test_ssl_reg_zero_is_lightgcn(ra, small):
    lg = build(ra, small, 3, 1, cls=ra.LightGCN)
    m = build(ra, small, 3, 1, ssl_reg=0.0)
    m.load_state_dict(lg.state_dict())
    batch = batch_of(small, B, seed=5)
    torch.manual_seed(99)
    want = float(lg.training_step(batch).detach())
    torch.manual_seed(99)
    got = float(m.training_step(batch).detach())
    assert abs(got - want) <= 1e-6 * abs(want)
    m.config['model']['ssl_reg'] = 0.1
    torch.manual_seed(99)
    assert float(m.training_step(batch).detach()) > got + 1e-3                    # the contrast is there when asked for


def test_eval_draws_nothing(ra, small):
    m = build(ra, small, 3, 1, aug_type='RW')
    m.adj_mat.to(DEV)
    m.eval()
    gen = torch.cuda.default_generators[torch.cuda.current_device()]
    before, cpu_before = gen.get_offset(), torch.get_rng_state()
    view = m.augmentaion_model.draw_view(m.adj_mat, m.LightGCNNet)
    assert all(v is m.adj_mat for v in view)
    nd = ra.data_augmentation.NodeDropout(0.1, NU, NI).eval()
    assert nd(m.adj_mat) is m.adj_mat
    assert gen.get_offset() == before and torch.equal(torch.get_rng_state(), cpu_before)
    m.train()
    assert m.augmentaion_model.draw_view(m.adj_mat, m.LightGCNNet)[0] is not m.adj_mat and gen.get_offset() > before


def test_fit_next_to_torch_ops(ra, ml100k):
    """3 epochs on ml-100k (adam, lr 1e-3, one negative, the stock SGL settings) next to the same model whose views are rebuilt
    with torch ops -- the mask from torch.rand in the same generator state, two bincounts, pow, gathers -- and whose propagation,
    over the graph and over the views, is torch.sparse.mm under autograd; its tail is the per-plugin one."""
    trn, val, tst = ml100k

    def coo(a, values, device):
        rows = sr.edge_rows(a.indptr)
        return torch.sparse_coo_tensor(torch.stack([rows, a.indices.long()]), values, (a.n_nodes, a.n_nodes)).coalesce().to(device)

    def mean_layers(mat, e, n_layers):
        x = s = e
        for _ in range(n_layers):
            x = torch.sparse.mm(mat, x)
            s = s + x
        return s / (n_layers + 1)

    class TorchAug(ra.data_augmentation.SGLAugmentation):
        def get_gnn_embeddings(self, user_emb, item_emb, adj_mat, gnn_net):
            a = adj_mat.to(user_emb.weight.device)
            keep = torch.floor(torch.rand(a.nnz, device=a.indptr.device) + self.augmentation.keep_prob).bool()
            rows, cols = sr.edge_rows(a.indptr), a.indices.long()
            in_deg = torch.bincount(rows[keep], minlength=a.n_nodes)
            out_deg = torch.bincount(cols[keep], minlength=a.n_nodes)
            w = (out_deg.double().pow(-0.5)[cols] * in_deg.double().pow(-0.5)[rows]).float()
            values = torch.where(keep, w, torch.zeros_like(w))
            e = torch.cat([user_emb.weight, item_emb.weight], dim=0)
            out = mean_layers(coo(a, values, e.device), e, gnn_net.n_layers)
            self.torch_views = getattr(self, 'torch_views', 0) + 1
            return out[:self.num_users], out[self.num_users:], keep

    class TorchSGL(ra.SGL):
        def _init_model(self, train_data, drop_unused_field=True):
            super()._init_model(train_data, drop_unused_field)
            self.augmentaion_model = TorchAug(self.config['model'], train_data)

        def _propagate(self, e):
            if not hasattr(self, '_coo'):
                a = self.adj_mat
                self._coo = coo(a, a.values, e.device)
            return mean_layers(self._coo, e, self.config['model']['n_layers'])

        def forward(self, batch, full_score=False, **kw):
            self.update_encoders()
            return self._forward_plugins(batch, full_score, False, False, False, True)

    cfg = {'model': {'embed_dim': D}, 'train': {'epochs': 3, 'learner': 'adam', 'learning_rate': 0.001}, 'eval': {'batch_size': 256}}
    runs = {}
    for name, cls in (('hip', ra.SGL), ('torch', TorchSGL)):
        model = cls(cfg)
        model.fit(trn, val)
        if name == 'torch':
            assert model.augmentaion_model.torch_views > 0 and hasattr(model, '_coo')
        else:
            assert isinstance(model.last_views[0], ra.graphmodule.AugmentedAdj)
        runs[name] = ([h['train_loss'] for h in model.history], model.evaluate(tst, verbose=False))
        print(name, runs[name][0], {k: round(v, 4) for k, v in runs[name][1].items() if k.endswith('@20')})
    hip, ref = runs['hip'][0], runs['torch'][0]
    assert len(hip) == 3 and all(abs(a - b) <= 0.02 * abs(b) for a, b in zip(hip, ref)), (hip, ref)
    assert hip[0] > hip[1] > hip[2]
    assert runs['hip'][1]['recall@20'] > 0.05
