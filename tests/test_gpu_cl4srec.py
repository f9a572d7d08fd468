"""GPU: retriever.CL4SRec -- one training step against the float64 restatement of tests/cl4srec_referee.py on the negatives and the
two views the run drew (replayed from the generator in the documented order through the per-sequence referee), model.fused_augment
on against off, evaluation without the mask token, and a short fit."""
import random

import numpy as np
import pytest
import torch

import cl4srec_referee as cr
from test_dataset_golden import make

pytestmark = pytest.mark.gpu
DEV = 'cuda'
B, L, D = 96, 20, 64
RATES = {'crop': 0.2, 'mask': 0.7, 'reorder': 0.2}


@pytest.fixture(scope='module')
def ra():
    import recstudio_amd
    recstudio_amd._native.lib()
    torch.cuda.init()
    return recstudio_amd


@pytest.fixture(scope='module')
def splits(ra, golden):
    return make(ra.SeqDataset, golden('data_ml100k'), max_seq_len=50).build(split_ratio=2)


def model_of(ra, data, **model_cfg):
    cfg = {'model': dict({'embed_dim': D, 'dropout_rate': 0.0}, **model_cfg), 'train': {'batch_size': B}}
    torch.manual_seed(5)
    m = ra.CL4SRec(cfg)
    m._init_model(data)
    m._init_parameter()
    with torch.no_grad():
        m.item_encoder.weight.mul_(10.0)
        m.query_encoder.mask_emb.mul_(10.0)
    return m.to(DEV).train()


def batch_of(N, seed=1):
    g = torch.Generator().manual_seed(seed)
    seqlen = torch.randint(1, L + 1, (B,), generator=g)
    seqlen[:3] = torch.tensor([L, 1, 2])
    hist = torch.randint(1, N, (B, L), generator=g) * (torch.arange(L).unsqueeze(0) < seqlen.unsqueeze(1))
    batch = {'user_id': torch.arange(1, B + 1), 'in_item_id': hist, 'seqlen': seqlen, 'item_id': torch.randint(1, N, (B,), generator=g),
             'rating': torch.ones(B)}
    return {k: v.to(DEV) for k, v in batch.items()}


def step(model, batch, seed):
    torch.manual_seed(seed)
    random.seed(seed)
    model.zero_grad(set_to_none=True)
    loss = model.training_step(batch)
    loss.backward()
    return loss


@pytest.mark.parametrize('fused_attention', [True, False], ids=['fused_tower', 'stock_tower'])
@pytest.mark.parametrize('augment_type', ['item_crop', 'item_mask', 'item_reorder', 'item_random'])
def test_one_training_step_against_float64(ra, splits, augment_type, fused_attention):
    """B = 96, L = 20 (< max_seq_len 50), d = 64, dropout 0: 1e-4 on the loss, 3e-4 on every gradient.  The generator order of a step:
    the main pass (its negatives; no dropout draws at p = 0), rand([B, L + 1]) for view i, the same for view j."""
    data = splits[0]
    N = data.num_items
    m = model_of(ra, data, augment_type=augment_type, fused_attention=fused_attention, tau=0.5 if augment_type == 'item_crop' else 0.2)
    mc = m.config['model']
    batch = batch_of(N)
    loss = step(m, batch, 31)
    # ---- the replay
    torch.manual_seed(31)
    random.seed(31)
    with torch.no_grad():
        neg = m.forward(batch, False, return_neg_id=True)['neg_id']
    uniforms = [torch.rand(B, L + 1, device=DEV), torch.rand(B, L + 1, device=DEV)]
    if augment_type == 'item_random':
        kinds = [('crop', 'mask', 'reorder')[random.randint(0, 2)] for _ in range(2)]
    else:
        kinds = [augment_type[5:]] * 2
    rates = [mc['tau'] if k == 'crop' else RATES[k] for k in kinds]
    views = cr.replay_views(batch['in_item_id'], batch['seqlen'], kinds, rates, uniforms, N)
    for (ids, ln), (want_ids, want_ln) in zip(m.last_views, views):
        assert torch.equal(ids.cpu(), want_ids) and torch.equal(ln.cpu(), want_ln)
    assert all(int(ids.max()) <= N for ids, _ in views) and (int(max(ids.max() for ids, _ in views)) == N) == ('mask' in kinds)
    want_loss, want_main, want_cl, want, want_item = cr.step(m.item_encoder.weight, m.query_encoder, batch['in_item_id'], batch['seqlen'],
                                                              batch['item_id'], neg, views, N, mc['temperature'], mc['cl_weight'])
    print(f'{augment_type} {kinds}, fused_attention {fused_attention}: loss {loss.item():.6f} (float64 {want_loss:.6f} = {want_main:.6f} + '
          f"{mc['cl_weight']} x {want_cl:.6f})")
    assert abs(loss.item() - want_loss) <= 1e-4 * abs(want_loss)
    got = dict(m.query_encoder.named_parameters())
    assert ('mask_emb' in want) == ('mask' in kinds) == bool(got['mask_emb'].grad.any())
    for name, gw in want.items():
        torch.testing.assert_close(got[name].grad.cpu().double(), gw, rtol=3e-4, atol=3e-6 * float(gw.abs().max()),
                                   msg=lambda s, n=name: f'{n}: {s}')
    gi = m.item_encoder.weight.grad.cpu().double()
    torch.testing.assert_close(gi, want_item, rtol=3e-4, atol=3e-6 * float(want_item.abs().max()))
    assert not gi[0].any()


@pytest.mark.parametrize('augment_type', ['item_crop', 'item_mask', 'item_reorder', 'item_random'])
def test_fused_augment_against_the_twin(ra, splits, augment_type):
    """model.fused_augment on against off at the same seed: the views are integer-equal, nothing else changes, the losses and the
    gradients are bit-equal."""
    data = splits[0]
    batch = batch_of(data.num_items, seed=2)
    runs = []
    for fused in (True, False):
        m = model_of(ra, data, augment_type=augment_type, fused_attention=True, fused_augment=fused)
        assert m.augmentation_model.augmentation.__class__.__name__.startswith('Item_')
        end = None
        loss = step(m, batch, 7)
        end = torch.cuda.default_generators[torch.cuda.current_device()].get_offset()
        runs.append((loss.detach().clone(), m.last_views, end, [p.grad.clone() for p in m.parameters() if p.grad is not None]))
    (la, va, ea, ga), (lb, vb, eb, gb) = runs
    assert torch.equal(la, lb) and ea == eb and len(ga) == len(gb) and all(torch.equal(x, y) for x, y in zip(ga, gb))
    for (ia, na), (ib, nb) in zip(va, vb):
        assert torch.equal(ia, ib) and torch.equal(na, nb) and na.dtype == batch['seqlen'].dtype
    assert not torch.equal(va[0][0], va[1][0])                              # two different views


@pytest.mark.parametrize('augment_type', ['item_crop', 'item_mask'])
def test_fused_infonce_against_the_twin(ra, splits, augment_type):
    """model.fused_infonce on against off at the same seed: the same views; 1e-4 on the loss, 3e-4 on every gradient (the module
    tolerances).  cl_weight 0 is SASRec's step and draws no view."""
    data = splits[0]
    batch = batch_of(data.num_items, seed=4)
    runs = []
    for fused in (True, False):
        m = model_of(ra, data, augment_type=augment_type, fused_attention=True, fused_infonce=fused, cl_weight=1.0)
        assert m.augmentation_model.InfoNCE_loss_fn.fused == fused
        loss = step(m, batch, 9)
        runs.append((loss.detach().clone(), m.last_views, {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}))
    (la, va, ga), (lb, vb, gb) = runs
    assert all(torch.equal(x[0], y[0]) and torch.equal(x[1], y[1]) for x, y in zip(va, vb))
    assert abs(float(la) - float(lb)) <= 1e-4 * abs(float(lb)) and set(ga) == set(gb)
    for n in gb:
        torch.testing.assert_close(ga[n], gb[n], rtol=3e-4, atol=3e-6 * float(gb[n].abs().max()), msg=lambda s, n=n: f'{n}: {s}')
    m0 = model_of(ra, data, augment_type=augment_type, fused_attention=True, cl_weight=0)
    l0 = step(m0, batch, 9)
    torch.manual_seed(9)
    with torch.no_grad():
        out = m0.forward(batch, False)
        want = m0.loss_fn(label=batch['rating'], **out['score'])
    assert m0.last_views is None and torch.equal(l0.detach(), want)


def test_evaluation_never_sees_the_mask_token(ra, splits):
    data = splits[0]
    N = data.num_items
    m = model_of(ra, data, augment_type='item_mask', fused_attention=True)
    batch = batch_of(N, seed=3)
    step(m, batch, 3)
    m.eval()
    with torch.no_grad():
        m._update_item_vector()
        score, items, query = m.topk(batch, 10, return_query=True)
    assert m.item_vector.shape == (N - 1, D) and int(items.max()) < N and int(items.min()) >= 1
    dense = query.cpu().double() @ m.item_encoder.weight.detach().cpu().double()[1:].T
    want, _ = dense.topk(10)
    torch.testing.assert_close(score.cpu().double(), want, rtol=1e-4, atol=1e-6)
    torch.testing.assert_close(dense.gather(1, items.cpu() - 1), want, rtol=1e-4, atol=1e-6)


def test_fit(ra, splits):
    """3 epochs on ml-100k with model.fused_augment and model.fused_infonce both on next to both off from the same seed: the epoch
    losses agree within 2 % (the tree's convention) and fall; evaluation is finite."""
    trn, val, tst = splits
    runs = {}
    for fused in (True, False):
        cfg = {'model': {'embed_dim': D, 'dropout_rate': 0.2, 'fused_attention': True, 'fused_augment': fused, 'fused_infonce': fused,
                         'augment_type': 'item_random'},
               'train': {'epochs': 3, 'batch_size': 512}, 'eval': {'batch_size': 256}}
        random.seed(1)
        model = ra.CL4SRec(cfg)
        model.fit(trn, val)
        runs[fused] = ([h['train_loss'] for h in model.history], model.evaluate(tst, verbose=False))
        assert model.item_encoder.weight.shape[0] == trn.num_items
    on, off = runs[True][0], runs[False][0]
    print('both flags on', on, 'off', off, 'gap', [abs(a - b) / abs(b) for a, b in zip(on, off)], 'test', runs[True][1])
    assert len(on) == 3 and all(abs(a - b) <= 0.02 * abs(b) for a, b in zip(on, off)), (on, off)
    assert on[0] > on[2] and all(np.isfinite(v) for v in runs[True][1].values())
