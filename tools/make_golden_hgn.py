"""Records tests/golden/hgn.npz from the reference's own HGNQueryEncoder (recstudio/model/seq/hgn.py:16-44), imported through
oracle/make_golden.py's ``import_reference`` recipe.  Run by hand on the CPU where a checkout of the reference is present; no
test, smoke() or bench.py runs it:

    python tools/make_golden_hgn.py

For max_seq_len 12, embed_dim 32, 7 users, 23 items and a batch of B = 5 handed over at width L = 9 < max_seq_len (so that
``W_g_4.weight[:L]`` is a proper slice) with lengths 9, 1, 4, 9, 3 it stores: the encoder's state dict (``sd.<key>``, the shared
``item_encoder`` included; ``b_g``, which the reference leaves uninitialised, set to 0.25 randn; ``W_g_4.bias`` as nn.Linear draws
it, non-zero), ``user_id`` [B], ``in_item_id`` [B, L], ``g`` [B, embed_dim]; and per pooling type (``mean``, ``max``) ``out.<type>`` =
``encoder(batch)`` [B, embed_dim] and the fp32 gradients of ``(out * g).sum()`` with respect to every parameter that receives one
(``grad.<type>.<key>``; ``W_g_4.bias`` receives none).  Data only."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENGTHS = (9, 1, 4, 9, 3)
L, MAX_LEN, D, USERS, ITEMS = 9, 12, 32, 7, 23


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden', 'hgn.npz'))
    args = ap.parse_args()
    out_path = os.path.abspath(args.out)
    sys.path.insert(0, os.path.join(ROOT, 'oracle'))
    import make_golden
    make_golden.import_reference()
    from recstudio.model.seq.hgn import HGNQueryEncoder
    torch.manual_seed(2023)
    item = torch.nn.Embedding(ITEMS, D, padding_idx=0)
    enc = HGNQueryEncoder('user_id', 'item_id', USERS, D, MAX_LEN, item, 'mean')
    with torch.no_grad():
        enc.b_g.copy_(0.25 * torch.randn(D))
        for lin in (enc.W_g_1, enc.W_g_2, enc.w_g_3, enc.W_g_4):          # (wider than nn.Linear's start, so that the gates move)
            lin.weight.mul_(3.0)
        enc.user_embedding.weight[0] = 0
    B = len(LENGTHS)
    lengths = torch.tensor(LENGTHS)
    hist = torch.randint(1, ITEMS, (B, L))
    hist[torch.arange(L).view(1, L) >= lengths.view(B, 1)] = 0
    users = torch.randint(1, USERS, (B,))
    g = torch.randn(B, D)
    rec = {f'sd.{k}': v.numpy().copy() for k, v in enc.state_dict().items()}
    rec.update(user_id=users.numpy(), in_item_id=hist.numpy(), g=g.numpy())
    params = dict(enc.named_parameters())
    for pooling in ('mean', 'max'):
        enc.pooling_type = pooling
        out = enc({'user_id': users, 'in_item_id': hist})
        grads = torch.autograd.grad((out * g).sum(), list(params.values()), allow_unused=True)
        rec[f'out.{pooling}'] = out.detach().numpy()
        for k, gr in zip(params, grads):
            assert (gr is None) == (k == 'W_g_4.bias'), k
            if gr is not None:
                rec[f'grad.{pooling}.{k}'] = gr.numpy()
    np.savez(out_path, **rec)
    print(out_path, os.path.getsize(out_path), 'bytes;', len(rec), 'arrays')


if __name__ == '__main__':
    main()
