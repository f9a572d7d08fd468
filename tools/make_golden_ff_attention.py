"""Records tests/golden/ff_attention.npz from the reference's own AttentionLayer (recstudio/model/module/layers.py:322-399), loaded by
file path from a checkout of the reference.  Run by hand on the CPU; no test, smoke() or bench.py runs it:

    python tools/make_golden_ff_attention.py --reference /path/to/reference/checkout

For NARM's configuration (q = k = M = 128, bias=False) and STAMP's (q = 128, k = M = 64, bias=True) at B = 5, S = 9 with lengths
9, 1, 4, 9, 3 it stores, under the prefix ``narm.`` / ``stamp.``: the layer's state dict (``sd.<key>``), ``query`` [B, 1, q], ``key``
[B, S, k] (non-zero at the padded positions), ``mask`` bool [B, S], ``g`` [B, 1, k]; ``out`` and ``weight`` of
``layer(query, key, key, key_padding_mask=mask, need_weight=True)``; and the fp32 gradients of ``(out * g).sum()`` with respect
to the query, the keys and every parameter (``grad.query``, ``grad.key``, ``grad.<key>``).  Data only."""
import argparse
import importlib.util
import os

import numpy as np
import torch

CONFIGS = {'narm': dict(q_dim=128, k_dim=None, mlp_layers=[128], bias=False),
           'stamp': dict(q_dim=128, k_dim=64, mlp_layers=[64], bias=True)}
LENGTHS = (9, 1, 4, 9, 3)
S = 9


def load_layers(reference):
    path = os.path.join(reference, 'recstudio', 'model', 'module', 'layers.py')
    spec = importlib.util.spec_from_file_location('reference_layers', path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', required=True, help='a checkout of the reference (the directory that holds recstudio/)')
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tests', 'golden',
                                                  'ff_attention.npz'))
    args = ap.parse_args()
    layers = load_layers(args.reference)
    rec = {}
    for seed, (name, cfg) in enumerate(CONFIGS.items()):
        torch.manual_seed(2022 + seed)
        layer = layers.AttentionLayer(q_dim=cfg['q_dim'], k_dim=cfg['k_dim'], mlp_layers=list(cfg['mlp_layers']), bias=cfg['bias'])
        with torch.no_grad():
            layer.mlp[1].bias.fill_(0.25)                  # (away from 0: a dropped b2 must show)
        B, k_dim = len(LENGTHS), cfg['k_dim'] or cfg['q_dim']
        query = torch.randn(B, 1, cfg['q_dim'], requires_grad=True)
        key = torch.randn(B, S, k_dim, requires_grad=True)
        mask = torch.arange(S).view(1, S) >= torch.tensor(LENGTHS).view(B, 1)
        g = torch.randn(B, 1, k_dim)
        out, weight = layer(query, key, key, key_padding_mask=mask, need_weight=True)
        params = dict(layer.named_parameters())
        grads = torch.autograd.grad((out * g).sum(), [query, key] + list(params.values()))
        for k, v in layer.state_dict().items():
            rec[f'{name}.sd.{k}'] = v.numpy().copy()
        rec.update({f'{name}.query': query.detach().numpy(), f'{name}.key': key.detach().numpy(), f'{name}.mask': mask.numpy(),
                    f'{name}.g': g.numpy(), f'{name}.out': out.detach().numpy(), f'{name}.weight': weight.detach().numpy(),
                    f'{name}.grad.query': grads[0].numpy(), f'{name}.grad.key': grads[1].numpy()})
        for k, gr in zip(params, grads[2:]):
            rec[f'{name}.grad.{k}'] = gr.numpy()
    np.savez(args.out, **rec)
    print(args.out, os.path.getsize(args.out), 'bytes;', len(rec), 'arrays')


if __name__ == '__main__':
    main()
