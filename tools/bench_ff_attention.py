"""Times the fused feed-forward attention pooling of NARM and STAMP (ops.ff_attention_pool / ops.ff_attention_pool_backward:
rsa_ffattn.hip) and what it does to the two models' steps.  One process, one device, the arms of a group alternating, device events
around every call, warm-up calls first; a streaming copy of 1 GiB is timed at the start and at the end as the record of the box's
state.  Prints one JSON object and writes it to profiles/ff_attention_bench.json.

    python tools/bench_ff_attention.py [--batch 8192 --reps 20 --warmup 5]

Groups:
  (1) core            forward and forward + backward of the pooling from (query, key, W1, b1, w2, b2, key_pad) at B = 8192 for NARM's
                      shape (S = 50, D = M = q = 128, no bias) and STAMP's (S = 20, D = M = 64, q = 128, bias): fused
                      (seqmodule.ff_attention_pool: the kernel and the small GEMMs on the query side) / twin
                      (seqmodule.ff_attention_pool_torch: the reference's op sequence).  Lengths all S, and drawn as SeqDataset's
                      windows over ml-100k-like users come out (bench_gru.window_lengths); both arms run every position either way.
                      Peak memory above the inputs; the byte model (forward: the keys once + out + a; backward: the keys twice more +
                      g + dkey) at 8 TB/s and the fp32-matrix floor (2 B S M D flops forward, 4 times that more in the backward) at
                      155 TF, and the fused arm's share of each.
  (2) training_step   NARM.training_step and STAMP.training_step + backward on tools/bench_fit.py's synthetic sequences over --items
                      = 100 001 items (the full softmax over the 1 000 001 of configs[2] would bury the tower; B = 8192; NARM:
                      L = 50, d = 128, hidden 128; STAMP: L = 20, d = 64), model.fused_attention_pool on and off, and with the
                      pooling taken out (out = the first key row): the share of the step the pooling holds.
Recorded: median / min / max in ms and the ratios."""
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


def core(seqmodule, dev, name, B, S, D, M, q_dim, bias, lengths_kind, reps, warmup):
    g = torch.Generator(device=dev).manual_seed(S)
    torch.manual_seed(S)
    layer = seqmodule.AttentionLayer(q_dim=q_dim, k_dim=D, mlp_layers=[M], bias=bias).to(dev)
    w1, b1, w2, b2 = layer._one_sigmoid_layer()
    params = [t for t in (w1, b1, w2, b2) if t is not None]
    query = torch.empty(B, q_dim, device=dev).normal_(generator=g).requires_grad_(True)
    key = torch.empty(B, S, D, device=dev).normal_(generator=g).requires_grad_(True)
    g_out = torch.empty(B, D, device=dev).normal_(generator=g)
    lengths = torch.full((B,), S, device=dev) if lengths_kind == 'full' else window_lengths(B, S, dev, g)
    pad = torch.arange(S, device=dev).view(1, S) >= lengths.view(B, 1)
    forms = {'fused': seqmodule.ff_attention_pool, 'twin': seqmodule.ff_attention_pool_torch}

    def fwd(f):
        def run():
            with torch.no_grad():
                return f(query, key, w1, b1, w2, b2, pad)[0]
        return run

    def both(f):
        def run():
            for t in [query, key] + params:
                t.grad = None
            return f(query, key, w1, b1, w2, b2, pad)[0].backward(g_out)
        return run

    ms = timed([fwd(forms['fused']), fwd(forms['twin']), both(forms['fused']), both(forms['twin'])], reps, warmup)
    out = dict(shape=name, B=B, S=S, D=D, M=M, q_dim=q_dim, bias=bias, lengths=lengths_kind, mean_length=float(lengths.float().mean()),
               forward=dict(fused=row(ms[0]), twin=row(ms[1])), forward_backward=dict(fused=row(ms[2]), twin=row(ms[3])))
    out['peak_bytes'] = {n: dict(forward=peak_above(fwd(f)), forward_backward=peak_above(both(f))) for n, f in forms.items()}
    rows = B * S
    bytes_f = 4 * (rows * D + B * D + rows)
    bytes_fb = bytes_f + 4 * (2 * rows * D + B * D + rows * D + 2 * rows)
    flops_f = 2 * rows * M * D
    mf, mb = out['forward']['fused']['ms'], out['forward_backward']['fused']['ms']
    out['byte_model_ms'] = dict(forward=bytes_f / PEAK_BYTES * 1e3, forward_backward=bytes_fb / PEAK_BYTES * 1e3)
    out['matrix_floor_ms'] = dict(forward=flops_f / PEAK_FLOPS * 1e3, forward_backward=5 * flops_f / PEAK_FLOPS * 1e3)
    out['share_of_byte_model'] = dict(forward=out['byte_model_ms']['forward'] / mf,
                                      forward_backward=out['byte_model_ms']['forward_backward'] / mb)
    out['share_of_matrix_floor'] = dict(forward=out['matrix_floor_ms']['forward'] / mf,
                                        forward_backward=out['matrix_floor_ms']['forward_backward'] / mb)
    out['twin_over_fused'] = dict(forward=out['forward']['twin']['ms'] / mf, forward_backward=out['forward_backward']['twin']['ms'] / mb)
    return out


def training_step(ra, seqmodule, dev, cls, B, L, d, model_cfg, n_items, reps, warmup):
    from bench_fit import synthetic_seq_dataset
    ds = synthetic_seq_dataset(ra, dev, 40_000, n_items, max_seq_len=L)
    steps = []
    for fused, core_on in ((True, True), (False, True), (True, False)):
        conf = {'model': dict(model_cfg, embed_dim=d, fused_attention_pool=fused), 'train': {'batch_size': B}}
        model = getattr(ra, cls)(conf)
        model._init_model(ds)
        model._init_parameter()
        model.to(dev)
        model.train()
        batch = None
        for b in ds.device_train_loader(B, shuffle=True, drop_last=True, device=dev):
            if batch is None or b['in_' + ds.fiid].shape[1] > batch['in_' + ds.fiid].shape[1]:
                batch = b                                   # the widest window of the epoch (L = max_seq_len)
        layer = model.query_encoder.attn_layer if cls == 'NARM' else model.query_encoder.attention_layer
        real = layer.forward

        def step(model=model, batch=batch, core_on=core_on, layer=layer, real=real):
            for t in model.parameters():
                t.grad = None
            if not core_on:
                layer.forward = lambda query, key, value, **kw: key[:, :1]
            try:
                model.training_step(batch).backward()
            finally:
                layer.forward = real
        steps.append(step)
    ms = timed(steps, reps, warmup)
    med = [statistics.median(t) for t in ms]
    return dict(model=cls, B=B, L=L, d=d, n_items=n_items, config=model_cfg, path=model._fused_train_path(), fused_on=row(ms[0]),
                fused_off=row(ms[1]), without_pooling=row(ms[2]), off_over_on=med[1] / med[0],
                pooling_share_on=(med[0] - med[2]) / med[0], pooling_share_off=(med[1] - med[2]) / med[1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=8192)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--items', type=int, default=100_001, help='catalog of the training-step group (full softmax over it)')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'ff_attention_bench.json'))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_ff_attention.py measures on the GPU: none found')
    import recstudio_amd as ra
    from recstudio_amd import seqmodule
    dev = torch.device('cuda')
    props = torch.cuda.get_device_properties(0)
    res = dict(device=props.name, compute_units=props.multi_processor_count, torch=torch.__version__, reps=a.reps, warmup=a.warmup,
               copy_gb_per_s_before=copy_gbps(dev))
    res['core'] = []
    for name, S, D, M, q_dim, bias in (('narm', 50, 128, 128, 128, False), ('stamp', 20, 64, 64, 128, True)):
        for kind in ('full', 'ml100k_windows'):
            res['core'].append(core(seqmodule, dev, name, a.batch, S, D, M, q_dim, bias, kind, a.reps, a.warmup))
            print(json.dumps(res['core'][-1]), file=sys.stderr, flush=True)
            torch.cuda.empty_cache()
    res['training_step'] = [training_step(ra, seqmodule, dev, 'NARM', a.batch, 50, 128, {'hidden_size': 128}, a.items, a.reps, a.warmup),
                            training_step(ra, seqmodule, dev, 'STAMP', a.batch, 20, 64, {}, a.items, a.reps, a.warmup)]
    res['copy_gb_per_s_after'] = copy_gbps(dev)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')
    print(json.dumps(res))


if __name__ == '__main__':
    main()
