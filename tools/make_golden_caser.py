"""Records tests/golden/caser.npz from the reference's own CaserQueryEncoder (recstudio/model/seq/caser.py:16-56), imported through
oracle/make_golden.py's ``import_reference`` recipe.  Run by hand on the CPU where a checkout of the reference is present; no
test, smoke() or bench.py runs it:

    python tools/make_golden_caser.py

For max_seq_len L = 9, embed_dim 32, n_v = 4, n_h = 16, 7 users, 23 items and a batch of B = 5 with lengths 9, 1, 4, 9, 3
in eval mode it stores: the encoder's state dict
(``sd.<key>``; the Conv2d biases redrawn as 0.25 randn so that both signs occur), ``user_id`` [B], ``in_item_id`` [B, L], ``g``
[B, 2 embed_dim]; ``out`` = ``encoder(batch)`` [B, 2 embed_dim]; and the fp32 gradients of ``(out * g).sum()`` with respect to every
parameter (``grad.<key>``).  Data only."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENGTHS = (9, 1, 4, 9, 3)
L, D, N_V, N_H, USERS, ITEMS = 9, 32, 4, 16, 7, 23


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden', 'caser.npz'))
    args = ap.parse_args()
    out_path = os.path.abspath(args.out)
    sys.path.insert(0, os.path.join(ROOT, 'oracle'))
    import make_golden
    make_golden.import_reference()
    from recstudio.model.seq.caser import CaserQueryEncoder
    torch.manual_seed(2022)
    enc = CaserQueryEncoder('item_id', 'user_id', USERS, ITEMS, D, L, N_V, N_H, dropout=0.4)
    with torch.no_grad():
        for conv in [enc.vertical_filter] + list(enc.horizontal_filter):
            conv.bias.copy_(0.25 * torch.randn(conv.bias.shape))
        enc.item_embedding.weight[0] = 0
        enc.user_embedding.weight[0] = 0
    enc.eval()
    B = len(LENGTHS)
    lengths = torch.tensor(LENGTHS)
    hist = torch.randint(1, ITEMS, (B, L))
    hist[torch.arange(L).view(1, L) >= lengths.view(B, 1)] = 0
    users = torch.randint(1, USERS, (B,))
    g = torch.randn(B, 2 * D)
    out = enc({'user_id': users, 'in_item_id': hist})
    params = dict(enc.named_parameters())
    grads = torch.autograd.grad((out * g).sum(), list(params.values()))
    rec = {f'sd.{k}': v.numpy().copy() for k, v in enc.state_dict().items()}
    rec.update(user_id=users.numpy(), in_item_id=hist.numpy(), g=g.numpy(), out=out.detach().numpy())
    for k, gr in zip(params, grads):
        rec[f'grad.{k}'] = gr.numpy()
    np.savez(out_path, **rec)
    print(out_path, os.path.getsize(out_path), 'bytes;', len(rec), 'arrays')


if __name__ == '__main__':
    main()
