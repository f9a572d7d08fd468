"""Times CL4SRec's per-step view draw (ops.seq_augment: rsa_seqaug.hip) and its in-batch InfoNCE (ops.batch_infonce /
ops.batch_infonce_backward: rsa_infonce.hip) next to their twins, and what both do to the model's step.  One process, one device, the
arms of a group alternating, device events around every call, warm-up calls first; a streaming copy of 1 GiB is timed at the start
and at the end as the record of the box's state.  Prints one JSON object and writes it to profiles/cl4srec_bench.json.

    python tools/bench_cl4srec.py [--batch 8192 --reps 20 --warmup 5]

Groups:
  (1) view_draw       one view of (B, L) = (256, 20) and (--batch, 50) for crop / mask / reorder at the default rates: the kernel
                      (Item_*(fused=True): one launch) / the twin (torch.rand([B, L + 1]) + seq_augment_torch: gathers, stable argsorts).
                      Lengths as SeqDataset's windows come out (bench_gru.window_lengths).
  (2) infonce         forward and forward + backward of the in-batch InfoNCE ('batch_both') at (B, d) = (256, 64), (--batch, 64) and
                      (--batch, 128): fused (data_augmentation.batch_infonce: the autograd node over the kernels) / twin
                      (batch_infonce_torch: the reference's op sequence), with the peak memory above the inputs (one [B, 2B] fp32
                      matrix is 512 MiB at B = 8192).
  (3) training_step   CL4SRec.training_step + backward on tools/bench_fit.py's synthetic sequences (--items items, one negative,
                      B = --batch, L = 50, d = 64, model.fused_attention on), model.fused_augment and model.fused_infonce both on,
                      both off and the view kernel alone, next to SASRec.training_step on the same batch.
Recorded: median / min / max in ms and the ratios.  ``fused_augment_wins_everywhere`` / ``fused_infonce_wins_everywhere`` are the
rules behind the defaults of model.fused_augment and model.fused_infonce (retriever.FUSED_INFONCE_DEFAULT)."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

from bench_gru import copy_gbps, window_lengths      # noqa: E402
from graph_bench import peak_above, row, timed       # noqa: E402


def view_draw(da, dev, B, L, reps, warmup):
    g = torch.Generator(device=dev).manual_seed(L)
    lengths = window_lengths(B, L, dev, g).long()
    seq = torch.randint(1, 100_000, (B, L), device=dev, generator=g) * (torch.arange(L, device=dev).view(1, L) < lengths.view(B, 1))
    out = dict(B=B, L=L, mean_length=float(lengths.float().mean()))
    for name, make in (('crop', lambda f: da.Item_Crop(0.2, fused=f)), ('mask', lambda f: da.Item_Mask(100_000, fused=f)),
                       ('reorder', lambda f: da.Item_Reorder(fused=f))):
        fused, twin = make(True), make(False)
        with torch.no_grad():
            ms = timed([lambda m=fused: m(seq, lengths), lambda m=twin: m(seq, lengths)], reps, warmup)
        med = [statistics.median(t) for t in ms]
        out[name] = dict(fused=row(ms[0]), twin=row(ms[1]), twin_over_fused=med[1] / med[0])
    return out


def infonce(da, dev, B, d, reps, warmup):
    g = torch.Generator(device=dev).manual_seed(d)
    zi = (torch.empty(B, d, device=dev).normal_(generator=g) * 0.3).requires_grad_(True)
    zj = (zi.detach() + 0.1 * torch.empty(B, d, device=dev).normal_(generator=g)).requires_grad_(True)
    forms = {'fused': lambda: da.batch_infonce(zi, zj, 1.0, True, fused=True), 'twin': lambda: da.batch_infonce_torch(zi, zj, 1.0, True)}

    def fwd(f):
        def run():
            with torch.no_grad():
                return f()
        return run

    def both(f):
        def run():
            zi.grad = zj.grad = None
            return f().mean().backward()
        return run

    ms = timed([fwd(forms['fused']), fwd(forms['twin']), both(forms['fused']), both(forms['twin'])], reps, warmup)
    med = [statistics.median(t) for t in ms]
    out = dict(B=B, d=d, one_logit_matrix_bytes=B * 2 * B * 4, forward=dict(fused=row(ms[0]), twin=row(ms[1])),
               forward_backward=dict(fused=row(ms[2]), twin=row(ms[3])),
               twin_over_fused=dict(forward=med[1] / med[0], forward_backward=med[3] / med[2]))
    out['peak_bytes'] = {n: dict(forward=peak_above(fwd(f)), forward_backward=peak_above(both(f))) for n, f in forms.items()}
    return out


def training_step(ra, dev, B, L, d, n_items, reps, warmup):
    from bench_fit import synthetic_seq_dataset
    ds = synthetic_seq_dataset(ra, dev, 40_000, n_items, max_seq_len=L)
    steps, batch = [], None
    arms = (('cl4srec_flags_on', ra.CL4SRec, dict(fused_augment=True, fused_infonce=True)),
            ('cl4srec_flags_off', ra.CL4SRec, dict(fused_augment=False, fused_infonce=False)),
            ('sasrec', ra.SASRec, dict(hidden_size=64, layer_num=1)),
            ('cl4srec_augment_only', ra.CL4SRec, dict(fused_augment=True, fused_infonce=False)))
    for _, cls, extra in arms:
        model = cls({'model': dict(embed_dim=d, fused_attention=True, **extra), 'train': {'batch_size': B}})
        model._init_model(ds)
        model._init_parameter()
        model.to(dev)
        model.train()
        if batch is None:
            for b in ds.device_train_loader(B, shuffle=True, drop_last=True, device=dev):
                if batch is None or b['in_' + ds.fiid].shape[1] > batch['in_' + ds.fiid].shape[1]:
                    batch = b                                   # the widest window of the epoch (L = max_seq_len)

        def step(model=model, batch=batch):
            for t in model.parameters():
                t.grad = None
            model.training_step(batch).backward()
        steps.append(step)
    ms = timed(steps, reps, warmup)
    med = [statistics.median(t) for t in ms]
    out = dict(B=B, L=L, d=d, n_items=n_items, augment_type='item_crop')
    out.update({name: row(t) for (name, _, _), t in zip(arms, ms)})
    out['flags_off_over_on'] = med[1] / med[0]
    out['cl4srec_over_sasrec'] = med[0] / med[2]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=8192)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--items', type=int, default=100_001, help='catalog of the training-step group')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'cl4srec_bench.json'))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_cl4srec.py measures on the GPU: none found')
    import recstudio_amd as ra
    from recstudio_amd import data_augmentation as da
    dev = torch.device('cuda')
    props = torch.cuda.get_device_properties(0)
    res = dict(device=props.name, compute_units=props.multi_processor_count, torch=torch.__version__, reps=a.reps, warmup=a.warmup,
               copy_gb_per_s_before=copy_gbps(dev))
    res['view_draw'] = [view_draw(da, dev, 256, 20, a.reps, a.warmup), view_draw(da, dev, a.batch, 50, a.reps, a.warmup)]
    print(json.dumps(res['view_draw']), file=sys.stderr, flush=True)
    res['fused_augment_wins_everywhere'] = all(v[k]['twin_over_fused'] > 1.0 for v in res['view_draw'] for k in ('crop', 'mask', 'reorder'))
    res['infonce'] = []
    for B, d in ((256, 64), (a.batch, 64), (a.batch, 128)):
        res['infonce'].append(infonce(da, dev, B, d, a.reps, a.warmup))
        torch.cuda.empty_cache()
    print(json.dumps(res['infonce']), file=sys.stderr, flush=True)
    res['fused_infonce_wins_everywhere'] = all(c['twin_over_fused'][k] >= 1.0 for c in res['infonce'] for k in ('forward', 'forward_backward'))
    res['training_step'] = training_step(ra, dev, a.batch, 50, 64, a.items, a.reps, a.warmup)
    res['copy_gb_per_s_after'] = copy_gbps(dev)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')
    print(json.dumps(res))


if __name__ == '__main__':
    main()
