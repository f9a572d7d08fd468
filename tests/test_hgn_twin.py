"""CPU: seqmodule.hgn_gating_torch (the reference's op sequence) against the float64 rule of tests/hgn_referee.py to 1e-12, and
the twin and retriever.HGNQueryEncoder against tests/golden/hgn.npz, the recording of the reference's own HGNQueryEncoder
(tools/make_golden_hgn.py: max_seq_len 12, L = 9, d = 32, lengths 9, 1, 4, 9, 3, b_g set, both pooling types): the state dict loads
with strict=True, the query within 1e-4, every parameter gradient within 3e-4."""
import numpy as np
import pytest
import torch

import hgn_referee as hr
from recstudio_amd import seqmodule

L, MAX_LEN, D, USERS, ITEMS = 9, 12, 32, 7, 23
NAMES = ('S', 'ug', 'ui', 'w1', 'w3')


@pytest.mark.parametrize('pooling', hr.POOLINGS)
def test_twin_equals_the_float64_rule(pooling):
    k = hr.kernel_inputs(hr.make_case(5, 9, 32, pad='whole', seed=7))
    ops = [k[n].double().requires_grad_(True) for n in NAMES]
    out = seqmodule.hgn_gating_torch(*ops, pooling)
    fwd = hr.judge_forward(*(k[n] for n in NAMES), pooling, dict(sigmoid=0.0))
    assert float((out.detach() - fwd['out']).abs().max()) <= 1e-12
    grads = torch.autograd.grad((out * k['g'].double()).sum(), ops)
    # max pooling: which of the exactly tied zero rows of a padded sequence receives g is torch's choice: dS is compared at
    # unpadded positions (nothing else depends on it: s = 0 there)
    want = hr.backward(*(k[n] for n in NAMES), pooling, k['g'])
    unpadded = (k['S'].abs().sum(2, keepdim=True) > 0).double()
    for name, got in zip(('dS', 'dug', 'dui', 'dw1', 'dw3'), grads):
        w = want[name]
        if name == 'dS' and pooling == 'max':
            got, w = got * unpadded, w * unpadded
        assert float((got - w.reshape(got.shape)).abs().max()) <= 1e-12, name


def test_the_autograd_node_falls_back_to_the_twin_on_the_cpu():
    k = hr.kernel_inputs(hr.make_case(3, 5, 48, pad='suffix', seed=1))            # (d = 48: no kernel either)
    got = seqmodule.hgn_gating(*(k[n] for n in NAMES), 'mean')
    assert torch.equal(got, seqmodule.hgn_gating_torch(*(k[n] for n in NAMES), 'mean'))
    with pytest.raises(ValueError):
        seqmodule.hgn_gating(*(k[n] for n in NAMES), 'avg')


def load_fixture(golden, pooling, device='cpu', fused_gating=False):
    """-> (HGNQueryEncoder with the recorded state dict, dict of the recorded tensors on ``device``)."""
    from recstudio_amd.retriever import HGNQueryEncoder
    z = golden('hgn')
    rec = {k: torch.from_numpy(z[k]).to(device) for k in z.files}
    item = torch.nn.Embedding(ITEMS, D, padding_idx=0)
    enc = HGNQueryEncoder('user_id', 'item_id', USERS, D, MAX_LEN, item, pooling, fused_gating=fused_gating)
    enc.load_state_dict({k[3:]: v for k, v in rec.items() if k.startswith('sd.')}, strict=True)
    return enc.to(device), rec


def check_against_fixture(enc, rec, pooling):
    out = enc({'user_id': rec['user_id'], 'in_item_id': rec['in_item_id']})
    np.testing.assert_allclose(out.detach().cpu().numpy(), rec['out.' + pooling].cpu().numpy(), rtol=1e-4, atol=1e-5)
    params = dict(enc.named_parameters())
    grads = torch.autograd.grad((out * rec['g']).sum(), list(params.values()), allow_unused=True)
    for name, got in zip(params, grads):
        if name == 'W_g_4.bias':
            assert got is None                                             # never used, never trained: as in the reference
            continue
        want = rec[f'grad.{pooling}.{name}'].cpu().numpy()
        np.testing.assert_allclose(got.cpu().numpy(), want, rtol=3e-4, atol=3e-4 / 100 * float(np.abs(want).max()) + 1e-30, err_msg=name)


def test_state_dict_keys_are_the_reference_s(golden):
    enc, rec = load_fixture(golden, 'mean')
    keys = [k[3:] for k in rec if k.startswith('sd.')]
    assert list(enc.state_dict()) == keys
    assert keys == ['b_g', 'item_encoder.weight', 'user_embedding.weight', 'W_g_1.weight', 'W_g_2.weight', 'w_g_3.weight',
                    'W_g_4.weight', 'W_g_4.bias']
    assert enc.W_g_4.weight.shape == (MAX_LEN, D) and bool(rec['sd.W_g_4.bias'].abs().min() > 0) and bool(rec['sd.b_g'].any())


def test_b_g_starts_at_zero():
    """The reference's b_g is torch.empty and no initialiser touches a bare Parameter; here it starts at zero, and stays there
    through the retriever's initialiser."""
    from recstudio_amd.retriever import HGNQueryEncoder
    enc = HGNQueryEncoder('user_id', 'item_id', USERS, D, MAX_LEN, torch.nn.Embedding(ITEMS, D, padding_idx=0))
    assert not enc.b_g.any() and enc.b_g.requires_grad and enc.fused_gating


@pytest.mark.parametrize('pooling', hr.POOLINGS)
def test_module_reproduces_the_recorded_encoder(golden, pooling):
    enc, rec = load_fixture(golden, pooling)
    assert rec['in_item_id'].shape == (5, L) and L < MAX_LEN and (rec['in_item_id'] != 0).sum(1).tolist() == [9, 1, 4, 9, 3]
    check_against_fixture(enc, rec, pooling)
    fused, _ = load_fixture(golden, pooling, fused_gating=True)            # (CPU tensors: the flag falls back to the twin)
    check_against_fixture(fused, rec, pooling)


@pytest.mark.parametrize('pooling', hr.POOLINGS)
def test_twin_reproduces_the_recorded_query(golden, pooling):
    """The twin alone on the recorded weights, ug and ui by hand."""
    enc, rec = load_fixture(golden, pooling)
    U = enc.user_embedding(rec['user_id'])
    S = enc.item_encoder(rec['in_item_id'])
    out = U + seqmodule.hgn_gating_torch(S, enc.W_g_2(U) + enc.b_g, U @ enc.W_g_4.weight[:L].T, enc.W_g_1.weight, enc.w_g_3.weight,
                                         pooling)
    np.testing.assert_allclose(out.detach().numpy(), rec['out.' + pooling].numpy(), rtol=1e-4, atol=1e-5)


@pytest.mark.parametrize('mistake', [m for m in hr.FORWARD_MISTAKES])
def test_every_forward_mistake_misses_the_recording(golden, mistake):
    """The referee's rule reproduces the recorded query from the recorded parameters; each seeded mistake does not."""
    pooling = 'max' if mistake == 'max_unpadded' else 'mean'
    enc, rec = load_fixture(golden, pooling)
    sd = enc.state_dict()
    lengths = (rec['in_item_id'] != 0).sum(1)
    U = sd['user_embedding.weight'][rec['user_id']]
    args = (U, sd['item_encoder.weight'][rec['in_item_id']], sd['W_g_1.weight'], sd['W_g_2.weight'], sd['b_g'], sd['w_g_3.weight'],
            sd['W_g_4.weight'], sd['W_g_4.bias'], lengths, pooling)
    want = rec['out.' + pooling].double()
    right = U.double() + hr.layer_rule(*args)[0]
    wrong = U.double() + hr.layer_rule(*args, mistake=mistake)[0]
    assert float((right - want).abs().max()) <= 1e-5
    assert float((wrong - want).abs().max()) > 1e-2


def test_hgn_applies_the_reference_s_config():
    """hgn.yaml on top of basemodel.yaml: pooling_type mean, negative_count 1 unless the caller sets it; model.fused_gating follows
    retriever.FUSED_GATING_DEFAULT."""
    import recstudio_amd as ra
    from recstudio_amd import retriever
    m = ra.HGN()
    assert m.config['model']['pooling_type'] == 'mean' and m.config['train']['negative_count'] == 1
    assert m.config['model']['fused_gating'] is retriever.FUSED_GATING_DEFAULT
    m = ra.HGN({'model': {'pooling_type': 'max', 'fused_gating': False}, 'train': {'negative_count': 64}})
    assert (m.config['model']['pooling_type'], m.config['model']['fused_gating'], m.config['train']['negative_count']) == ('max', False, 64)
    assert ra.HGN._get_dataset_class() is ra.SeqDataset and isinstance(m._get_loss_func(), ra.BPRLoss)
