"""Times the fused GRU recurrence of the sequence towers (ops.gru_sequence / ops.gru_sequence_backward: rsa_gru.hip) and what it
does to the GRU4Rec step.  One process, one device, the arms of a group alternating, device events around every call, warm-up calls
first; a streaming copy of 1 GiB is timed at the start and at the end as the record of the box's state.  Prints one JSON object and
writes it to profiles/gru_bench.json.

    python tools/bench_gru.py [--batch 8192 --reps 20 --warmup 5]

Groups:
  (1) core            forward and forward + backward of the RECURRENCE from gi = W_ih x [B, L, 3 H] (the input GEMM is outside every
                      arm but nn.GRU's, whose arm is timed with it and, separately, that GEMM alone) at B = 8192, L = 50, H = 128 and
                      at L = 20, H = 64, bias=False as the reference's GRULayer: fused (seqmodule.gru_sequence: the kernel and the
                      backward's three GEMMs) / twin (seqmodule.gru_sequence_torch: the same rule in torch ops, L steps) / nn_gru
                      (torch.nn.GRU on the device over x [B, L, H]).  Lengths all L, and drawn as SeqDataset's windows over ml-100k-like
                      users come out (a user has 20 + Exp(86) interactions, a window is a uniform prefix of them cut at L); nn.GRU
                      runs every position either way.  The fp32-matrix floor: 2 * 3 H * H * B * L flops forward, twice that backward,
                      at 155 TF.  Peak memory of a forward + backward above the inputs, for each.
  (2) training_step   GRU4Rec.training_step + backward at the configs[2] shape (B = 8192, L = 50, d = 128, hidden 128, 256 negatives:
                      tools/bench_fit.py's synthetic sequences), model.fused_gru on and off, and with the recurrence taken out (out =
                      the r columns of gi): the share of the step the recurrence holds.
Recorded: median / min / max in ms and the ratios."""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

from graph_bench import peak_above, row, timed      # noqa: E402

PEAK_FLOPS = 155e12


def copy_gbps(dev):
    """A 1 GiB device-to-device copy: GB/s moved (read + written), the median of 5."""
    src = torch.empty(1 << 28, dtype=torch.float32, device=dev).normal_()
    dst = torch.empty_like(src)
    ms = timed([lambda: dst.copy_(src)], 5, 2)[0]
    return 2 * src.numel() * 4 / (statistics.median(ms) * 1e-3) / 1e9


def window_lengths(B, L, dev, g):
    """Lengths of SeqDataset windows over ml-100k-like users: n = 20 + Exp(86) interactions, a uniform prefix of 1 .. n - 1, cut at L."""
    n = 20 + torch.empty(B, device=dev).exponential_(1.0 / 86.0, generator=g)
    k = 1 + (torch.rand(B, device=dev, generator=g) * (n - 1)).floor()
    return k.clamp(max=L).long()


def core(seqmodule, dev, B, L, H, lengths_kind, reps, warmup):
    g = torch.Generator(device=dev).manual_seed(L)
    torch.manual_seed(L)
    gru = torch.nn.GRU(H, H, num_layers=1, bias=False, batch_first=True).to(dev)
    w_ih, w_hh = gru.weight_ih_l0.detach(), gru.weight_hh_l0.detach()
    x = torch.empty(B, L, H, device=dev).normal_(generator=g)
    g_out = torch.empty(B, L, H, device=dev).normal_(generator=g)
    lengths = None if lengths_kind == 'full' else window_lengths(B, L, dev, g)
    gi = F.linear(x, w_ih)
    gi_leaf, x_leaf = gi.clone().requires_grad_(True), x.clone().requires_grad_(True)
    w_leaf = w_hh.clone().requires_grad_(True)
    forms = {'fused': lambda a: seqmodule.gru_sequence(a, w_leaf, None, None, lengths),
             'twin': lambda a: seqmodule.gru_sequence_torch(a, w_leaf, None, None, lengths)}

    def fwd(f, a):
        def run():
            with torch.no_grad():
                return f(a)
        return run

    g3 = torch.empty(B, L, 3 * H, device=dev).normal_(generator=g)

    def both(f, leaf, grad=g_out):
        def run():
            leaf.grad = None
            w_leaf.grad = None
            for t in gru.parameters():
                t.grad = None
            return f(leaf).backward(grad)
        return run

    stock = lambda a: gru(a)[0]                              # noqa: E731
    gemm = lambda a: F.linear(a, gru.weight_ih_l0)           # noqa: E731
    arms = [fwd(forms['fused'], gi), fwd(forms['twin'], gi), fwd(stock, x), fwd(gemm, x),
            both(forms['fused'], gi_leaf), both(forms['twin'], gi_leaf), both(stock, x_leaf), both(gemm, x_leaf, g3)]
    ms = timed(arms, reps, warmup)
    names = ['fused', 'twin', 'nn_gru', 'input_gemm']
    out = dict(B=B, L=L, H=H, lengths=lengths_kind, mean_length=float(L if lengths is None else lengths.float().mean()),
               forward={n: row(ms[i]) for i, n in enumerate(names)}, forward_backward={n: row(ms[4 + i]) for i, n in enumerate(names)})
    out['peak_bytes'] = dict(fused=peak_above(both(forms['fused'], gi_leaf)), twin=peak_above(both(forms['twin'], gi_leaf)),
                             nn_gru=peak_above(both(stock, x_leaf)))
    steps = B * L if lengths is None else int(lengths.sum())
    flops_f = 2 * 3 * H * H * B * L
    mf, mb = out['forward']['fused']['ms'], out['forward_backward']['fused']['ms']
    out['floor_ms'] = dict(forward=flops_f / PEAK_FLOPS * 1e3, forward_backward=3 * flops_f / PEAK_FLOPS * 1e3,
                           live_share_of_steps=steps / (B * L))
    out['fused_over_floor'] = dict(forward=mf / out['floor_ms']['forward'], forward_backward=mb / out['floor_ms']['forward_backward'])
    # nn.GRU's arm holds the input GEMM; the fused and twin arms do not: both comparisons are recorded
    for n in ('twin', 'nn_gru'):
        out[n + '_over_fused'] = dict(forward=out['forward'][n]['ms'] / mf, forward_backward=out['forward_backward'][n]['ms'] / mb)
    out['nn_gru_over_fused_with_input_gemm'] = dict(
        forward=out['forward']['nn_gru']['ms'] / (mf + out['forward']['input_gemm']['ms']),
        forward_backward=out['forward_backward']['nn_gru']['ms'] / (mb + out['forward_backward']['input_gemm']['ms']))
    return out


def training_step(ra, seqmodule, dev, B, L, d, H, n, reps, warmup):
    from bench_fit import synthetic_seq_dataset
    ds = synthetic_seq_dataset(ra, dev, 40_000, 1_000_001, max_seq_len=L)
    steps = []
    real = seqmodule.gru_sequence
    for fused, core_on in ((True, True), (False, True), (True, False)):
        conf = {'model': {'embed_dim': d, 'hidden_size': H, 'fused_gru': fused}, 'train': {'negative_count': n, 'batch_size': B}}
        model = ra.GRU4Rec(conf)
        model._init_model(ds)
        model._init_parameter()
        model.to(dev)
        model.train()
        batch = None
        for b in ds.device_train_loader(B, shuffle=True, drop_last=True, device=dev):
            if batch is None or b['in_' + ds.fiid].shape[1] > batch['in_' + ds.fiid].shape[1]:
                batch = b                                   # the widest window of the epoch (L = max_seq_len)

        def step(model=model, batch=batch, core_on=core_on):
            for t in model.parameters():
                t.grad = None
            if not core_on:
                seqmodule.gru_sequence = lambda gi, w_hh, *a: gi[:, :, :w_hh.shape[1]]
            try:
                model.training_step(batch).backward()
            finally:
                seqmodule.gru_sequence = real
        steps.append(step)
    ms = timed(steps, reps, warmup)
    med = [statistics.median(t) for t in ms]
    return dict(B=B, L=L, d=d, hidden_size=H, negative_count=n, fused_gru_on=row(ms[0]), fused_gru_off=row(ms[1]),
                without_recurrence=row(ms[2]), off_over_on=med[1] / med[0], recurrence_share_on=(med[0] - med[2]) / med[0],
                recurrence_share_off=(med[1] - med[2]) / med[1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=8192)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'gru_bench.json'))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_gru.py measures on the GPU: none found')
    import recstudio_amd as ra
    from recstudio_amd import seqmodule
    dev = torch.device('cuda')
    props = torch.cuda.get_device_properties(0)
    res = dict(device=props.name, compute_units=props.multi_processor_count, torch=torch.__version__, reps=a.reps, warmup=a.warmup,
               copy_gb_per_s_before=copy_gbps(dev))
    res['core'] = []
    for L, H in ((50, 128), (20, 64)):
        for kind in ('full', 'ml100k_windows'):
            res['core'].append(core(seqmodule, dev, a.batch, L, H, kind, a.reps, a.warmup))
            print(json.dumps(res['core'][-1]), file=sys.stderr, flush=True)
            torch.cuda.empty_cache()
    res['training_step'] = training_step(ra, seqmodule, dev, a.batch, 50, 128, 128, 256, a.reps, a.warmup)
    res['copy_gb_per_s_after'] = copy_gbps(dev)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')
    print(json.dumps(res))


if __name__ == '__main__':
    main()
