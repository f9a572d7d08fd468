"""CPU: seqmodule.AttentionLayer against tests/golden/ff_attention.npz, the recording of the reference's own AttentionLayer
(tools/make_golden_ff_attention.py) for NARM's configuration (q = k = M = 128, no bias) and STAMP's (q = 128, k = M = 64, bias) at
B = 5, S = 9 with lengths 9, 1, 4, 9, 3: the state dict loads with strict=True, and the twin path (CPU tensors) is held to the
project's parity contract -- 1e-4 on out and the weights, 3e-4 on the gradients."""
import numpy as np
import pytest
import torch

from recstudio_amd import seqmodule

CONFIGS = {'narm': dict(q_dim=128, k_dim=None, mlp_layers=[128], bias=False),
           'stamp': dict(q_dim=128, k_dim=64, mlp_layers=[64], bias=True)}


def load_fixture(golden, name, device='cpu'):
    """-> (layer with the recorded state dict, dict of the recorded tensors on ``device``)."""
    z = golden('ff_attention')
    rec = {k[len(name) + 1:]: torch.from_numpy(z[k]).to(device) for k in z.files if k.startswith(name + '.')}
    cfg = CONFIGS[name]
    layer = seqmodule.AttentionLayer(q_dim=cfg['q_dim'], k_dim=cfg['k_dim'], mlp_layers=list(cfg['mlp_layers']), bias=cfg['bias'])
    layer.load_state_dict({k[3:]: v for k, v in rec.items() if k.startswith('sd.')}, strict=True)
    return layer.to(device), rec


def check_against_fixture(layer, rec):
    """Runs ``layer`` as NARM / STAMP call it on the recorded inputs and holds it to 1e-4 (out, weights) / 3e-4 (gradients)."""
    query, key = rec['query'].clone().requires_grad_(True), rec['key'].clone().requires_grad_(True)
    out, weight = layer(query, key, key, key_padding_mask=rec['mask'], need_weight=True)
    np.testing.assert_allclose(out.detach().cpu().numpy(), rec['out'].cpu().numpy(), rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(weight.detach().cpu().numpy(), rec['weight'].cpu().numpy(), rtol=1e-4, atol=1e-6)
    params = dict(layer.named_parameters())
    grads = torch.autograd.grad((out * rec['g']).sum(), [query, key] + list(params.values()))
    for name, got in zip(['query', 'key'] + list(params), grads):
        want = rec['grad.' + name].cpu().numpy()
        np.testing.assert_allclose(got.cpu().numpy(), want, rtol=3e-4, atol=3e-4 / 100 * float(np.abs(want).max()), err_msg=name)
    pad = rec['mask'].cpu()
    assert not weight.detach().cpu()[:, 0][pad].any() and not grads[1].cpu()[pad].any()


@pytest.mark.parametrize('name', sorted(CONFIGS))
def test_twin_reproduces_the_recorded_layer(golden, name):
    layer, rec = load_fixture(golden, name)
    assert rec['key'][rec['mask']].abs().min() > 0          # non-zero keys at the padded positions
    check_against_fixture(layer, rec)
