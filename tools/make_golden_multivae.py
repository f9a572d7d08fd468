"""Records tests/golden/multivae.npz from the reference's own MultiDAEQueryEncoder / MultiVAEQueryEncoder
(recstudio/model/ae/multidae.py:9-34, multivae.py:9-60) and its UserDataset (recstudio/data/dataset.py:1278-1366), imported
through oracle/make_golden.py's ``import_reference`` recipe.  Run by hand on the CPU where a checkout of the reference is present;
no test, smoke() or bench.py runs it:

    python tools/make_golden_multivae.py

ENCODERS.  23 items, embed_dim 8, a batch of B = 5 right-padded histories of width L = 9 with lengths 9, 1, 4, 9, 3.  Per encoder
(``dae``: encoder_dims [6, 4], decoder_dims [4, 6], relu; ``vae``: encoder_dims [6, 4], decoder_dims [4, 6], tanh) it stores the
state dict (``<enc>.sd.<key>``), ``<enc>.eval`` = the eval-mode output, ``<enc>.train`` = the training-mode output at dropout 0
under ``torch.manual_seed(77)`` (the VAE's one ``randn_like`` draw), the gradients of ``(out * g).sum()`` in that mode
(``<enc>.grad.<key>``) and, for the VAE, ``vae.kl``; shared: ``in_item_id`` [B, L], ``g`` [B, 8].

USERDATASET on the bundled ml-100k demo file, ``seed_everything(2022)`` then ``build(split_ratio=[0.8, 0.1, 0.1])``: per split
(``trn``, ``val``, ``tst``) the ``[user, start, end, user, start', end')`` index rows (``u.<split>.index``), the count
(``u.counts``), and the padded batch of the split's first 8 index rows (``u.<split>.<key>``; evaluation mode for val / tst, so
they carry ``user_hist``).  Data only."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENGTHS = (9, 1, 4, 9, 3)
L, D, ITEMS = 9, 8, 23
ENC_DIMS, DEC_DIMS = [6, 4], [4, 6]


def record_encoder(rec, name, enc, batch, g):
    rec.update({f'{name}.sd.{k}': v.numpy().copy() for k, v in enc.state_dict().items()})
    enc.eval()
    with torch.no_grad():
        rec[f'{name}.eval'] = enc(batch).numpy()
    enc.train()
    torch.manual_seed(77)
    out = enc(batch)
    params = dict(enc.named_parameters())
    grads = torch.autograd.grad((out * g).sum(), list(params.values()))
    rec[f'{name}.train'] = out.detach().numpy()
    for k, gr in zip(params, grads):
        rec[f'{name}.grad.{k}'] = gr.numpy()
    if name == 'vae':
        rec['vae.kl'] = enc.kl_loss.detach().numpy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden', 'multivae.npz'))
    args = ap.parse_args()
    out_path = os.path.abspath(args.out)
    sys.path.insert(0, os.path.join(ROOT, 'oracle'))
    import make_golden
    make_golden.import_reference()
    from recstudio.data.dataset import UserDataset
    from recstudio.model.ae.multidae import MultiDAEQueryEncoder
    from recstudio.model.ae.multivae import MultiVAEQueryEncoder
    from recstudio.utils import seed_everything

    torch.manual_seed(2023)
    B = len(LENGTHS)
    hist = torch.randint(1, ITEMS, (B, L))
    hist[torch.arange(L).view(1, L) >= torch.tensor(LENGTHS).view(B, 1)] = 0
    g = torch.randn(B, D)
    rec = dict(in_item_id=hist.numpy(), g=g.numpy())
    batch = {'in_item_id': hist}
    record_encoder(rec, 'dae', MultiDAEQueryEncoder('item_id', ITEMS, D, 0.0, ENC_DIMS, DEC_DIMS, 'relu'), batch, g)
    record_encoder(rec, 'vae', MultiVAEQueryEncoder('item_id', ITEMS, D, 0.0, ENC_DIMS, DEC_DIMS, 'tanh'), batch, g)

    seed_everything(2022)
    ds = UserDataset('ml-100k')
    splits = ds.build(split_ratio=[0.8, 0.1, 0.1], shuffle=True, split_mode='user_entry')
    rec['u.counts'] = np.array([len(s) for s in splits])
    for name, split in zip(('trn', 'val', 'tst'), splits):
        split.eval_mode = name != 'trn'
        split.use_field = {'user_id', 'item_id', 'rating'}
        rec[f'u.{name}.index'] = split.data_index.numpy().astype(np.int32)
        b = split[torch.arange(8)]
        rec[f'u.{name}.keys'] = np.array(sorted(b.keys()))
        for k in ('user_id', 'in_item_id', 'in_rating', 'item_id', 'rating', 'user_hist'):
            if k in b:
                rec[f'u.{name}.{k}'] = b[k].numpy().astype(np.float32 if 'rating' in k else np.int32)
    np.savez_compressed(out_path, **rec)
    print(out_path, os.path.getsize(out_path), 'bytes;', len(rec), 'arrays')


if __name__ == '__main__':
    main()
