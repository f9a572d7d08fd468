"""CPU: retriever.CL4SRec without a device -- config defaults, state_dict keys, the mask token's placement, need_pooling=False, and
the step's two halves (SASRec's BCE on given negatives + cl_weight x the contrast of two views) on CPU tensors, through the twins and
the torch-op tower with dropout 0, against the float64 restatement of tests/cl4srec_referee.py."""
import random

import pytest
import torch

import cl4srec_referee as cr
import oracle
from test_dataset_golden import make

B, L = 32, 20
RATES = {'crop': 0.2, 'mask': 0.7, 'reorder': 0.2}


@pytest.fixture(scope='module')
def ra():
    import recstudio_amd
    return recstudio_amd


@pytest.fixture(scope='module')
def data(ra, golden):
    return make(ra.SeqDataset, golden('data_ml100k'), max_seq_len=L).build(split_ratio=2)[0]


def model_of(ra, data, cls=None, **model_cfg):
    cfg = {'model': dict({'embed_dim': 64, 'dropout_rate': 0.0}, **model_cfg), 'train': {'batch_size': B}}
    torch.manual_seed(5)
    m = (cls or ra.CL4SRec)(cfg)
    m._init_model(data)
    m._init_parameter()
    with torch.no_grad():
        m.item_encoder.weight.mul_(10.0)
        m.query_encoder.mask_emb.mul_(10.0) if hasattr(m.query_encoder, 'mask_emb') else None
    return m


def batch_of(N, seed=1):
    g = torch.Generator().manual_seed(seed)
    seqlen = torch.randint(1, L + 1, (B,), generator=g)
    seqlen[:3] = torch.tensor([L, 1, 2])
    hist = torch.randint(1, N, (B, L), generator=g) * (torch.arange(L).unsqueeze(0) < seqlen.unsqueeze(1))
    return {'in_item_id': hist, 'seqlen': seqlen}, torch.randint(1, N, (B,), generator=g), torch.randint(1, N, (B, 1), generator=g)


def test_defaults_and_state_dict(ra, data):
    m = ra.CL4SRec().config['model']
    assert (m['hidden_size'], m['layer_num'], m['temperature'], m['augment_type'], m['tau'], m['cl_weight']) == (64, 1, 1.0, 'item_crop', 0.2, 0.1)
    assert (m['head_num'], m['dropout_rate'], m['activation'], m['fused_attention'], m['fused_augment']) == (2, 0.5, 'gelu', False, True)
    assert m['fused_infonce'] is ra.retriever.FUSED_INFONCE_DEFAULT is False      # set by measurement
    assert ra.CL4SRec({'model': {'hidden_size': 96, 'layer_num': 2}}).config['model']['hidden_size'] == 96
    assert ra.SASRec().config['model']['hidden_size'] == 128 and 'CL4SRec' in ra.retriever.__all__
    cl, sas = model_of(ra, data), model_of(ra, data, cls=ra.SASRec, hidden_size=64, layer_num=1)
    assert set(cl.state_dict()) == set(sas.state_dict()) | {'query_encoder.mask_emb'}
    assert 'mask_emb' not in ''.join(sas.state_dict())
    for k, v in sas.state_dict().items():                                  # the mask token is drawn last: SASRec's parameters at the seed
        assert torch.equal(v, cl.state_dict()[k]), k
    assert cl.item_encoder.weight.shape == (data.num_items, 64) and cl.query_encoder.mask_emb.shape == (1, 64)
    assert cl.query_encoder.mask_id == data.num_items and bool(cl.query_encoder.mask_emb.any())
    assert cl.augmentation_model.InfoNCE_loss_fn.neg_type == 'batch_both' and cl.augmentation_model.InfoNCE_loss_fn.sim_method == 'inner_product'
    with pytest.raises(ValueError, match='augment_type'):
        model_of(ra, data, augment_type='item_insert')


@pytest.mark.parametrize('fused_attention', [True, False], ids=['twin_tower', 'stock_tower'])
def test_need_pooling(ra, data, fused_attention):
    m = model_of(ra, data, fused_attention=fused_attention)
    batch, _, _ = batch_of(data.num_items)
    out = m.query_encoder(batch, need_pooling=False)
    assert out.shape == (B, L, 64)
    last = out[torch.arange(B), batch['seqlen'] - 1]
    assert torch.equal(m.query_encoder(batch), last) and torch.equal(m.query_encoder(batch, need_pooling=True), last)
    # the mask token: its own row, attended, never a catalog id
    ids = batch['in_item_id'].clone()
    ids[:, 0] = data.num_items
    got = m.query_encoder({'in_item_id': ids, 'seqlen': batch['seqlen']}, need_pooling=False)      # (it never reaches the table)
    e = cr.copy.deepcopy(m.query_encoder).double()
    want = cr.tower(e, m.item_encoder.weight.detach().double(), ids, data.num_items)
    valid = torch.arange(L).unsqueeze(0) < batch['seqlen'].unsqueeze(1)
    assert float((got.detach().double() - want.detach())[valid].abs().max()) <= 1e-4 * float(want.detach().abs().max())


@pytest.mark.parametrize('augment_type', ['item_crop', 'item_mask', 'item_reorder', 'item_random'])
def test_step_against_float64(ra, data, augment_type):
    m = model_of(ra, data, augment_type=augment_type, fused_attention=True, tau=0.5 if augment_type == 'item_crop' else 0.2)
    m.train()
    N, mc = data.num_items, m.config['model']
    batch, pos, neg = batch_of(N)
    enc, w = m.query_encoder, m.item_encoder.weight
    query = enc(batch)
    main = oracle.bce_loss((query * w[pos]).sum(-1), (query.unsqueeze(1) * w[neg]).sum(-1))
    torch.manual_seed(21)
    random.seed(21)
    cl = m.augmentation_model(batch, enc)['cl_loss']
    loss = main + mc['cl_weight'] * cl                                       # CL4SRec.training_step's sum (its tail needs the device)
    loss.backward()
    # ---- the replay: rand([B, L + 1]) for view i, then for view j; item_random takes one randint per view
    torch.manual_seed(21)
    random.seed(21)
    uniforms = [torch.rand(B, L + 1), torch.rand(B, L + 1)]
    if augment_type == 'item_random':
        kinds = [('crop', 'mask', 'reorder')[random.randint(0, 2)] for _ in range(2)]
    else:
        kinds = [augment_type[5:]] * 2
    rates = [mc['tau'] if k == 'crop' else RATES[k] for k in kinds]
    views = cr.replay_views(batch['in_item_id'], batch['seqlen'], kinds, rates, uniforms, N)
    for (ids, ln), (want_ids, want_ln) in zip(m.last_views, views):
        assert torch.equal(ids, want_ids) and torch.equal(ln, want_ln)
    want_loss, want_main, want_cl, want, want_item = cr.step(w, enc, batch['in_item_id'], batch['seqlen'], pos, neg, views, N,
                                                              mc['temperature'], mc['cl_weight'])
    print(f'{augment_type} {kinds}: loss {loss.item():.6f} (float64 {want_loss:.6f}), main {main.item():.6f}, cl {cl.item():.6f}')
    assert abs(main.item() - want_main) <= 1e-4 * abs(want_main) and abs(cl.item() - want_cl) <= 1e-4 * abs(want_cl)
    assert abs(loss.item() - want_loss) <= 1e-4 * abs(want_loss)
    got = dict(enc.named_parameters())
    has_mask = 'mask' in kinds
    assert ('mask_emb' in want) == has_mask
    assert bool(got['mask_emb'].grad.any()) == has_mask                     # the mask token learns only under item_mask
    for name, gw in want.items():
        torch.testing.assert_close(got[name].grad.double(), gw, rtol=3e-4, atol=3e-6 * float(gw.abs().max()), msg=lambda s, n=name: f'{n}: {s}')
    torch.testing.assert_close(w.grad.double(), want_item, rtol=3e-4, atol=3e-6 * float(want_item.abs().max()))
    assert not w.grad[0].any()
