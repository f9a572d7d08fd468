"""GPU: the fused gating behind HGNQueryEncoder(fused_gating=True) and HGN's model.fused_gating: the recording of the reference's
encoder through the kernel, a checkpoint moving between the flag's two settings, a float64 training step on the negatives the run
drew, evaluate's top-k against dense float64 scores, and a short fit next to the torch-op model."""
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import hgn_referee as hr
import oracle
from test_dataset_golden import make
from test_hgn_twin import check_against_fixture, load_fixture

pytestmark = pytest.mark.gpu

DEV = 'cuda'


@pytest.fixture(scope='module')
def ra():
    import recstudio_amd
    recstudio_amd._native.lib()
    torch.cuda.init()
    return recstudio_amd


def close(got, want, rtol, atol):
    torch.testing.assert_close(torch.as_tensor(got).detach().cpu().double(), torch.as_tensor(want).detach().cpu().double(), rtol=rtol,
                               atol=atol)


class counted:
    """Counts the launches of the autograd node over the kernel."""

    def __enter__(self):
        from recstudio_amd import seqmodule
        self.mod, self.real, self.calls = seqmodule, seqmodule._HgnGatingFn.apply, []
        seqmodule._HgnGatingFn.apply = staticmethod(lambda *a: (self.calls.append(1), self.real(*a))[1])
        return self.calls

    def __exit__(self, *exc):
        self.mod._HgnGatingFn.apply = self.real
        return False


@pytest.mark.parametrize('pooling', hr.POOLINGS)
def test_fused_encoder_reproduces_the_recorded_encoder(ra, golden, pooling):
    """tests/golden/hgn.npz (the reference's own HGNQueryEncoder, L = 9 < max_seq_len = 12, d = 32) through the kernel: 1e-4 on the
    query, 3e-4 on every parameter gradient."""
    enc, rec = load_fixture(golden, pooling, device=DEV, fused_gating=True)
    with counted() as calls:
        check_against_fixture(enc, rec, pooling)
    assert len(calls) == 1


def _tower(N, users, d, max_len, pooling, seed, **kw):
    from recstudio_amd.retriever import HGNQueryEncoder
    torch.manual_seed(seed)
    item = torch.nn.Embedding(N, d, padding_idx=0)
    enc = HGNQueryEncoder('user_id', 'item_id', users, d, max_len, item, pooling, **kw)
    with torch.no_grad():
        item.weight[0] = 0
        enc.b_g.normal_(0.0, 0.3)
    return enc


def _batch(N, L, B, seed):
    gen = torch.Generator().manual_seed(seed)
    seqlen = torch.randint(1, L + 1, (B,), generator=gen)
    seqlen[0], seqlen[1] = L, 1
    hist = torch.randint(1, N, (B, L), generator=gen)
    hist[torch.arange(L).view(1, -1) >= seqlen.view(-1, 1)] = 0
    return hist, seqlen, torch.randint(1, N, (B,), generator=gen)


@pytest.mark.parametrize('pooling', hr.POOLINGS)
def test_a_checkpoint_moves_between_the_flag_s_settings(ra, tmp_path, pooling):
    N, users, d, max_len, L, B = 211, 40, 64, 20, 17, 19
    off = _tower(N, users, d, max_len, pooling, seed=1, fused_gating=False)
    on = _tower(N, users, d, max_len, pooling, seed=2, fused_gating=True)
    assert list(off.state_dict()) == list(on.state_dict())
    torch.save(off.state_dict(), tmp_path / 'off.pt')
    on.load_state_dict(torch.load(tmp_path / 'off.pt'))
    off.to(DEV).eval(), on.to(DEV).eval()
    hist, seqlen, _ = _batch(N, L, B, seed=3)
    batch = {'in_item_id': hist.to(DEV), 'seqlen': seqlen.to(DEV), 'user_id': torch.arange(1, B + 1).to(DEV)}
    with counted() as calls:
        got, want = on(batch), off(batch)
    assert len(calls) == 1
    close(got, want, 1e-4, 1e-5)
    torch.save(on.state_dict(), tmp_path / 'on.pt')
    back = _tower(N, users, d, max_len, pooling, seed=4, fused_gating=False)
    back.load_state_dict(torch.load(tmp_path / 'on.pt'))
    for k, v in back.state_dict().items():
        assert torch.equal(v.cpu(), off.state_dict()[k].cpu())


@pytest.fixture(scope='module')
def ml100k(ra, golden):
    return make(ra.SeqDataset, golden('data_ml100k'), max_seq_len=20).build(split_ratio=2)


def _model(ra, trn, n_neg, **model_cfg):
    cfg = {'model': dict({'embed_dim': 64}, **model_cfg), 'train': {'negative_count': n_neg, 'batch_size': 512},
           'eval': {'batch_size': 256}}
    model = ra.HGN(cfg)
    model._init_model(trn)
    model._init_parameter()
    with torch.no_grad():                      # (the 'xavier_normal' start leaves scores near 0: widen them so the step has a slope)
        for p in model.parameters():
            p.mul_(3.0)
        model.query_encoder.b_g.normal_(0.0, 0.3)
        model.item_encoder.weight[0] = 0
    return model.to(DEV)


def _query64(e, w, users, hist, pooling):
    """The float64 tower over the weights of ``e`` (a CPU double copy of the encoder) and the item table ``w``."""
    from recstudio_amd import seqmodule
    U = F.embedding(users, e.user_embedding.weight, padding_idx=0)
    S = F.embedding(hist, w, padding_idx=0)
    return U + seqmodule.hgn_gating_torch(S, e.W_g_2(U) + e.b_g, U @ e.W_g_4.weight[:hist.shape[1]].T, e.W_g_1.weight,
                                          e.w_g_3.weight, pooling)


@pytest.mark.parametrize('pooling', hr.POOLINGS)
@pytest.mark.parametrize('n_neg', [1, 64], ids=['one_negative', 'fused_bpr_tail'])
def test_one_training_step_against_float64(ra, ml100k, n_neg, pooling):
    """HGN.training_step at d = 64, L = 15 < max_seq_len = 20, B = 96.  No dropout: the sampler is the only consumer of the device
    generator, so replaying it yields the negatives.  Against the float64 step on those: 1e-4 on the loss, 3e-4 on every
    parameter gradient (with 3e-4 / 100 of the gradient's largest magnitude for the elements that cancel).  negative_count 64
    takes the single-launch fused BPR tail, 1 (the reference's default) the fused scorer and the loss kernel."""
    trn = ml100k[0]
    model = _model(ra, trn, n_neg, pooling_type=pooling, fused_gating=True)
    model.train()
    assert model._fused_train_path() == ('bpr' if n_neg == 64 else None) and model.query_encoder.fused_gating
    N, d, L, B = trn.num_items, 64, 15, 96
    hist, seqlen, pos = _batch(N, L, B, seed=4)
    users = torch.arange(1, B + 1)
    batch = {model.fiid: pos.to(DEV), 'in_' + model.fiid: hist.to(DEV), 'seqlen': seqlen.to(DEV), model.fuid: users.to(DEV),
             model.frating: torch.ones(B, device=DEV)}
    torch.manual_seed(11)
    with counted() as calls:
        loss = model.training_step(batch)
        loss.backward()
    assert len(calls) == 1
    # ---- the replay: the negatives
    torch.manual_seed(11)
    with torch.no_grad():
        _, neg = ra.retriever_scores(model.item_encoder.weight, torch.zeros(B, d, device=DEV), n_neg, pos_ids=batch[model.fiid],
                                     sampler=model.sampler)
    # ---- the float64 step
    e = copy.deepcopy(model.query_encoder).cpu().double()
    w = model.item_encoder.weight.detach().cpu().double().requires_grad_(True)
    query = _query64(e, w, users, hist, pooling)
    ps = (query * F.embedding(pos, w)).sum(-1)
    ns = (query.unsqueeze(1) * F.embedding(neg.cpu().view(B, n_neg), w)).sum(-1)
    want = oracle.bpr_loss(ps, ns)
    want.backward()
    assert abs(loss.item() - want.item()) <= 1e-4 * abs(want.item()), (loss.item(), want.item())
    got = dict(model.query_encoder.named_parameters())
    names = [n for n, _ in e.named_parameters() if not n.startswith('item_encoder')]
    assert sorted(names) == ['W_g_1.weight', 'W_g_2.weight', 'W_g_4.bias', 'W_g_4.weight', 'b_g', 'user_embedding.weight', 'w_g_3.weight']
    for name in names:
        gw = dict(e.named_parameters())[name].grad
        if name == 'W_g_4.bias':
            assert gw is None and got[name].grad is None
            continue
        close(got[name].grad, gw, 3e-4, 3e-6 * float(gw.abs().max()))
    assert not got['W_g_4.weight'].grad[L:].any() and bool(got['W_g_4.weight'].grad[:L].any())
    close(model.item_encoder.weight.grad, w.grad, 3e-4, 3e-6 * float(w.grad.abs().max()))


def test_topk_against_dense_float64_scores(ra, ml100k):
    """evaluate's selection (BaseRetriever.topk) for HGN's query: the scores within 1e-4 of the dense float64 scores of the same
    query over the catalog, every selected item's float64 score at least the k-th best (up to that tolerance), and the query
    itself within 1e-4 of the float64 tower."""
    trn = ml100k[0]
    model = _model(ra, trn, 1, fused_gating=True)
    model.eval()
    N, L, B, k = trn.num_items, 20, 64, 10
    hist, seqlen, _ = _batch(N, L, B, seed=6)
    users = torch.arange(1, B + 1)
    batch = {'in_' + model.fiid: hist.to(DEV), 'seqlen': seqlen.to(DEV), model.fuid: users.to(DEV)}
    with torch.no_grad(), counted() as calls:
        score, items, query = model.topk(batch, k, return_query=True)
    assert len(calls) == 1
    dense = query.double().cpu() @ model.item_encoder.weight.detach().double().cpu()[1:].t()
    want, _ = torch.topk(dense, k)
    close(score, want, 1e-4, 1e-6)
    picked = dense.gather(1, items.cpu() - 1)
    close(picked, want, 1e-4, 1e-6)
    assert int(items.min()) >= 1 and all(len(set(r.tolist())) == k for r in items.cpu())
    e = copy.deepcopy(model.query_encoder).cpu().double()
    ref = _query64(e, model.item_encoder.weight.detach().cpu().double(), users, hist, 'mean')
    close(query, ref, 1e-4, 1e-5)


def test_fit_next_to_the_torch_op_model(ra, ml100k):
    """3 epochs of HGN on ml-100k (embed_dim 64, mean pooling, one negative) with model.fused_gating on next to off from the same
    seed: the sampler is the only consumer of the generator, so the two runs see the same negatives and differ in rounding only.
    Every epoch's loss within 2 %.  Measured: the three epoch means (0.4677, 0.2785, 0.2594) agree to fp32 resolution, gap 0,
    and so do the test metrics."""
    trn, val, tst = ml100k
    runs = {}
    for fused in (True, False):
        cfg = {'model': {'embed_dim': 64, 'fused_gating': fused}, 'train': {'epochs': 3, 'batch_size': 512}, 'eval': {'batch_size': 256}}
        model = ra.HGN(cfg)
        with counted() as calls:
            model.fit(trn, val)
        assert model.query_encoder.fused_gating == fused and bool(calls) == fused                  # the kernel ran, or never
        runs[fused] = (model, [h['train_loss'] for h in model.history], model.evaluate(tst, verbose=False))
    hip, ref = runs[True][1], runs[False][1]
    print('fused', hip, 'torch ops', ref, 'gap', [abs(a - b) / abs(b) for a, b in zip(hip, ref)])
    print('test metrics: fused', runs[True][2], 'torch ops', runs[False][2])
    assert len(hip) == 3 and all(abs(a - b) <= 0.02 * abs(b) for a, b in zip(hip, ref)), (hip, ref)
    assert hip[0] > hip[2] and all(np.isfinite(v) for v in runs[True][2].values())
    assert list(runs[True][0].state_dict()) == list(runs[False][0].state_dict())
    runs[False][0].load_state_dict(runs[True][0].state_dict())
