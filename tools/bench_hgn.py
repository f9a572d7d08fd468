"""Times HGN's fused hierarchical gating (ops.hgn_gating / ops.hgn_gating_backward: rsa_gating.hip) and what it does to the
model's step.  One process, one device, the arms of a group alternating, device events around every call, warm-up calls first; a
streaming copy of 1 GiB is timed at the start and at the end as the record of the box's state.  Prints one JSON object and writes
it to profiles/hgn_bench.json.

    python tools/bench_hgn.py [--batch 8192 --reps 20 --warmup 5]

Groups:
  (1) core            forward and forward + backward of the gating from (S, ug, ui, W_g_1, w_g_3) at B = 8192 for (L, d) = (20, 64)
                      and (50, 128), mean and max pooling: fused (seqmodule.hgn_gating: the autograd node over the kernel) / twin
                      (seqmodule.hgn_gating_torch: the reference's op sequence).  Lengths as SeqDataset's windows over
                      ml-100k-like users come out (bench_gru.window_lengths): the padded rows are zero rows, both arms run every
                      position.  Peak memory above the inputs; the byte model (forward: S once + out + w; backward: S three times
                      more + dS + g, dui, w) at 8 TB/s and the fp32-matrix floor (2 B L d^2 flops forward, 5 times that more in the
                      backward under mean pooling) at 155 TF, and the fused arm's share of each.
  (2) training_step   HGN.training_step + backward on tools/bench_fit.py's synthetic sequences (--items = 100 001 items, one
                      negative, B = 8192; L = 20, d = 64 and L = 50, d = 128), model.fused_gating on and off.
Recorded: median / min / max in ms and the ratios.  ``fused_wins_everywhere`` is the rule behind retriever.FUSED_GATING_DEFAULT."""
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

PEAK_FLOPS = 155e12
PEAK_BYTES = 8e12


def core(seqmodule, dev, B, L, D, pooling, reps, warmup):
    g = torch.Generator(device=dev).manual_seed(L)
    k = 1.0 / D ** 0.5
    lengths = window_lengths(B, L, dev, g)
    S = torch.empty(B, L, D, device=dev).normal_(generator=g)
    S.mul_((torch.arange(L, device=dev).view(1, L) < lengths.view(B, 1)).unsqueeze(2))
    S.requires_grad_(True)
    ug = torch.empty(B, D, device=dev).normal_(generator=g).requires_grad_(True)
    ui = torch.empty(B, L, device=dev).normal_(generator=g).requires_grad_(True)
    w1 = ((torch.rand(D, D, device=dev, generator=g) * 2 - 1) * k).requires_grad_(True)
    w3 = ((torch.rand(D, device=dev, generator=g) * 2 - 1) * k).requires_grad_(True)
    g_out = torch.empty(B, D, device=dev).normal_(generator=g)
    leaves = [S, ug, ui, w1, w3]
    forms = {'fused': seqmodule.hgn_gating, 'twin': seqmodule.hgn_gating_torch}

    def fwd(f):
        def run():
            with torch.no_grad():
                return f(S, ug, ui, w1, w3, pooling)
        return run

    def both(f):
        def run():
            for t in leaves:
                t.grad = None
            return f(S, ug, ui, w1, w3, pooling).backward(g_out)
        return run

    ms = timed([fwd(forms['fused']), fwd(forms['twin']), both(forms['fused']), both(forms['twin'])], reps, warmup)
    out = dict(B=B, L=L, d=D, pooling=pooling, mean_length=float(lengths.float().mean()),
               forward=dict(fused=row(ms[0]), twin=row(ms[1])), forward_backward=dict(fused=row(ms[2]), twin=row(ms[3])))
    out['peak_bytes'] = {n: dict(forward=peak_above(fwd(f)), forward_backward=peak_above(both(f))) for n, f in forms.items()}
    rows = B * L
    bytes_f = 4 * (rows * D + B * D + 2 * rows + B * D)
    bytes_fb = bytes_f + 4 * (3 * rows * D + rows * D + 3 * rows + 3 * B * D)
    flops_f = 2 * rows * D * D
    mf, mb = out['forward']['fused']['ms'], out['forward_backward']['fused']['ms']
    n_prod = 6 if pooling == 'mean' else 5
    out['byte_model_ms'] = dict(forward=bytes_f / PEAK_BYTES * 1e3, forward_backward=bytes_fb / PEAK_BYTES * 1e3)
    out['matrix_floor_ms'] = dict(forward=flops_f / PEAK_FLOPS * 1e3, forward_backward=n_prod * flops_f / PEAK_FLOPS * 1e3)
    out['share_of_byte_model'] = dict(forward=out['byte_model_ms']['forward'] / mf,
                                      forward_backward=out['byte_model_ms']['forward_backward'] / mb)
    out['share_of_matrix_floor'] = dict(forward=out['matrix_floor_ms']['forward'] / mf,
                                        forward_backward=out['matrix_floor_ms']['forward_backward'] / mb)
    out['twin_over_fused'] = dict(forward=out['forward']['twin']['ms'] / mf, forward_backward=out['forward_backward']['twin']['ms'] / mb)
    return out


def training_step(ra, dev, B, L, d, n_items, reps, warmup):
    from bench_fit import synthetic_seq_dataset
    ds = synthetic_seq_dataset(ra, dev, 40_000, n_items, max_seq_len=L)
    steps = []
    for fused in (True, False):
        model = ra.HGN({'model': dict(embed_dim=d, fused_gating=fused), 'train': {'batch_size': B}})
        model._init_model(ds)
        model._init_parameter()
        model.to(dev)
        model.train()
        batch = None
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
    return dict(model='HGN', B=B, L=L, d=d, n_items=n_items, path=model._fused_train_path(), fused_on=row(ms[0]), fused_off=row(ms[1]),
                off_over_on=med[1] / med[0])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=8192)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--items', type=int, default=100_001, help='catalog of the training-step group')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'hgn_bench.json'))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_hgn.py measures on the GPU: none found')
    import recstudio_amd as ra
    from recstudio_amd import seqmodule
    dev = torch.device('cuda')
    props = torch.cuda.get_device_properties(0)
    res = dict(device=props.name, compute_units=props.multi_processor_count, torch=torch.__version__, reps=a.reps, warmup=a.warmup,
               copy_gb_per_s_before=copy_gbps(dev))
    res['core'] = []
    for L, D in ((20, 64), (50, 128)):
        for pooling in ('mean', 'max'):
            res['core'].append(core(seqmodule, dev, a.batch, L, D, pooling, a.reps, a.warmup))
            print(json.dumps(res['core'][-1]), file=sys.stderr, flush=True)
            torch.cuda.empty_cache()
    res['fused_wins_everywhere'] = all(c['twin_over_fused'][k] > 1.0 for c in res['core'] for k in ('forward', 'forward_backward'))
    res['training_step'] = [training_step(ra, dev, a.batch, 20, 64, a.items, a.reps, a.warmup),
                            training_step(ra, dev, a.batch, 50, 128, a.items, a.reps, a.warmup)]
    res['copy_gb_per_s_after'] = copy_gbps(dev)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')
    print(json.dumps(res))


if __name__ == '__main__':
    main()
