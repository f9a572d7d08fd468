"""CPU: SASRecQueryEncoder(fused_attention=True) on CPU tensors -- seqmodule.FusedTransformerEncoder's layer loop with the torch-op
twin of the attention core -- against the reference's own recorded tower (tests/golden/sasrec.npz, oracle/make_golden_sasrec.py:
d = 32, L = 9, 2 heads of 16, hidden 48, 2 layers, recorded on the CPU).  Measured: the query off by at most 7.2e-7, the loss
by nothing in fp32, the three gradients by at most 9e-8 (their largest elements 0.09 - 0.22)."""
import os

import numpy as np
import pytest
import torch

import oracle

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope='module')
def fixture():
    return np.load(os.path.join(HERE, 'golden', 'sasrec.npz'))


def build(g, **kw):
    from recstudio_amd.retriever import SASRecQueryEncoder
    N, d, L = int(g['N']), int(g['d']), int(g['L'])
    item = torch.nn.Embedding(N, d, padding_idx=0)
    enc = SASRecQueryEncoder('item_id', d, L, int(g['heads']), int(g['hidden']), 0.0, 'gelu', 1e-12, int(g['layers']), item, **kw)
    state = {k[3:]: torch.from_numpy(g[k]) for k in g.files if k.startswith('w::')}
    return item, enc, state


def within(got, ref, rtol, atol):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    excess = np.abs(got - ref) - (rtol * np.abs(ref) + atol)
    assert excess.max() <= 0, f'worst excess {excess.max():.3e} (worst |diff| {np.abs(got - ref).max():.3e})'


def test_fused_tower_twin_matches_the_reference_fixture(fixture):
    g = fixture
    item, enc, state = build(g, fused_attention=True)
    assert set(enc.state_dict()) == set(state)                   # the reference module's parameter names, one for one
    enc.load_state_dict(state)
    enc.train()
    batch = {'in_item_id': torch.from_numpy(g['hist']), 'seqlen': torch.from_numpy(g['seqlen'])}
    pos, neg = torch.from_numpy(g['pos']), torch.from_numpy(g['neg'])
    log_pos, log_neg = torch.from_numpy(g['log_pos']), torch.from_numpy(g['log_neg'])
    query = enc(batch)
    ps = (query * item(pos)).sum(-1)
    ns = (query.unsqueeze(1) * item(neg)).sum(-1)
    loss = oracle.sampled_softmax_loss(ps, log_pos, ns, log_neg)
    loss.backward()
    within(query.detach(), g['ssm_query'], 1e-4, 1e-6)
    assert abs(loss.item() - float(g['ssm_loss'])) <= 1e-5 * abs(float(g['ssm_loss']))
    for got, name in ((item.weight.grad, 'ssm_item_grad'), (enc.position_emb.weight.grad, 'ssm_posemb_grad'),
                      (enc.transformer_layer.layers[0].linear1.weight.grad, 'ssm_lin1_grad')):
        within(got, g[name], 3e-4, 3e-6 * np.abs(g[name]).max())
    assert not item.weight.grad[0].any()
    enc.eval()
    with torch.no_grad():
        within(enc(batch), g['eval_query'], 1e-4, 1e-6)


def test_state_dict_moves_between_the_two_settings(fixture):
    _, fused, state = build(fixture, fused_attention=True)
    _, stock, _ = build(fixture)
    fused.load_state_dict(state)
    stock.load_state_dict(fused.state_dict())
    assert list(stock.state_dict()) == list(fused.state_dict())
    for k, v in stock.state_dict().items():
        assert torch.equal(v, state[k])
    assert fused.fused_attention and not stock.fused_attention and not stock.bidirectional


def test_sasrec_reads_the_config_key():
    import recstudio_amd as ra
    assert ra.SASRec().config['model']['fused_attention'] is False
    assert ra.SASRec({'model': {'fused_attention': True}}).config['model']['fused_attention'] is True
