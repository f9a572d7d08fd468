"""CPU: seqmodule.caser_conv_torch (the reference's op sequence on the packed operands) against the float64 rule of
tests/caser_referee.py to 1e-12, and the twin and retriever.CaserQueryEncoder against tests/golden/caser.npz, the
recording of the reference's own CaserQueryEncoder (tools/make_golden_caser.py: L = 9, d = 32, n_v = 4, n_h = 16, lengths 9, 1, 4,
9, 3, eval mode): the state dict loads with strict=True, the query within 1e-4, every parameter gradient within 3e-4."""
import numpy as np
import torch

import caser_referee as cr
from recstudio_amd import seqmodule

L, D, N_V, N_H, USERS, ITEMS = 9, 32, 4, 16, 7, 23


def test_twin_equals_the_float64_rule():
    c = cr.make_case(5, 9, 32, 4, 16, seed=7, kind='whole')
    ops = [c[n].double().requires_grad_(True) for n in ('rows', 'w_v', 'b_v', 'w_h', 'b_h')]
    o = seqmodule.caser_conv_torch(*ops)
    fwd = cr.forward(c['rows'], c['w_v'], c['b_v'], c['w_h'], c['b_h'])
    assert float((o.detach() - fwd['o']).abs().max()) <= 1e-12
    grads = torch.autograd.grad((o * c['g'].double()).sum(), ops)
    want = cr.backward(c['rows'], c['w_v'], c['w_h'], cr.exact_idx(fwd), c['g'])
    for name, got in zip(('drows', 'dw_v', 'db_v', 'dw_h', 'db_h'), grads):
        assert float((got - want[name]).abs().max()) <= 1e-12, name


def load_fixture(golden, device='cpu'):
    """-> (CaserQueryEncoder with the recorded state dict, dict of the recorded tensors on ``device``)."""
    from recstudio_amd.retriever import CaserQueryEncoder
    z = golden('caser')
    rec = {k: torch.from_numpy(z[k]).to(device) for k in z.files}
    enc = CaserQueryEncoder('item_id', 'user_id', USERS, ITEMS, D, L, N_V, N_H, dropout=0.4)
    enc.load_state_dict({k[3:]: v for k, v in rec.items() if k.startswith('sd.')}, strict=True)
    return enc.to(device).eval(), rec


def check_against_fixture(enc, rec):
    out = enc({'user_id': rec['user_id'], 'in_item_id': rec['in_item_id']})
    np.testing.assert_allclose(out.detach().cpu().numpy(), rec['out'].cpu().numpy(), rtol=1e-4, atol=1e-5)
    params = dict(enc.named_parameters())
    grads = torch.autograd.grad((out * rec['g']).sum(), list(params.values()))
    for name, got in zip(params, grads):
        want = rec['grad.' + name].cpu().numpy()
        np.testing.assert_allclose(got.cpu().numpy(), want, rtol=3e-4, atol=3e-4 / 100 * float(np.abs(want).max()) + 1e-30, err_msg=name)


def test_state_dict_keys_are_the_reference_s(golden):
    enc, rec = load_fixture(golden)
    keys = [k[3:] for k in rec if k.startswith('sd.')]
    assert list(enc.state_dict()) == keys
    assert keys[:6] == ['user_embedding.weight', 'item_embedding.weight', 'vertical_filter.weight', 'vertical_filter.bias',
                        'horizontal_filter.0.weight', 'horizontal_filter.0.bias'] and keys[-2:] == ['fc.weight', 'fc.bias']
    assert isinstance(enc.horizontal_filter[3], torch.nn.Conv2d) and enc.horizontal_filter[3].weight.shape == (N_H, 1, 4, D)


def test_module_reproduces_the_recorded_encoder(golden):
    enc, rec = load_fixture(golden)
    assert (rec['in_item_id'] != 0).sum(1).tolist() == [9, 1, 4, 9, 3]
    check_against_fixture(enc, rec)


def test_twin_reproduces_the_recorded_features(golden):
    """The twin alone on the recorded weights: through fc by hand it gives the recorded query."""
    enc, rec = load_fixture(golden)
    rows = enc.item_embedding(rec['in_item_id'])
    o = seqmodule.caser_conv_torch(rows, *seqmodule.caser_pack(enc.vertical_filter, enc.horizontal_filter))
    z = torch.relu(enc.fc(o))
    np.testing.assert_allclose(z.detach().numpy(), rec['out'][:, :D].numpy(), rtol=1e-4, atol=1e-5)


def test_short_histories_are_padded_to_max_seq_len(golden):
    enc, rec = load_fixture(golden)
    batch = {'user_id': rec['user_id'][1:3], 'in_item_id': rec['in_item_id'][1:3, :4]}          # lengths 1 and 4, handed over at width 4
    np.testing.assert_allclose(enc(batch).detach().numpy(), rec['out'][1:3].numpy(), rtol=1e-4, atol=1e-5)
