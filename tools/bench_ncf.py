"""Times NCF's pair scorer kernel (ops.pair_mlp / ops.pair_mlp_backward: rsa_pairmlp.hip) next to its torch-op twin and what it
does to the model's step.  One process, one device, the arms of a group alternating, device events around every call, warm-up
calls first; a streaming copy of 1 GiB is timed at the start and at the end as the record of the box's state.  Prints one JSON
object and writes it to profiles/ncf_bench.json.

    python tools/bench_ncf.py [--reps 20 --warmup 5 --items 100001]

Groups:
  (1) core            FusionMFMLPScorer and MLPScorer (d = 64, hidden [128, 64], dropout 0.1, training mode) from (query [B, d], the
                      table, ids [B, 1 + n]) to the scores, forward and forward + backward (to the query, the table and every
                      weight), at (B, n) = (65 536, 1) and (16 384, 64): fused (scorer.score_ids: the autograd node over the kernels)
                      / twin (F.embedding + scorer.pair_mlp_torch: the reference's op sequence with torch.rand masks).  Peak memory
                      above the inputs; the fp32-matrix floor 2 (2d H1 + H1 H2) M flops at 155 TF (three times that more in the
                      backward: the rows pass's two transposed products and the dW products, no recomputation counted) and the
                      byte model (forward: id + item row + score per pair and the queries; backward: the same read again twice,
                      the upstream gradient, du and the item row written per pair) at 8 TB/s, and the fused arm's share of each.
  (2) topk            NCF.topk (k = 100, no history) over --items items at B = 2048 with model.fused_scorer on: the range mode in
                      chunks of eval.pair_chunk.  The twin would first build [B, N, 2d] fp32 (the figure is recorded, not tried).
  (3) training_step   NCF.training_step + backward (yaml defaults, BCE, uniform negatives) at (B, n) = (65 536, 1) and
                      (16 384, 64), model.fused_scorer on and off.
Recorded: median / min / max in ms and the ratios.  ``fused_wins_everywhere`` (both training shapes, both directions, both
scorers) is the rule behind models_mf.FUSED_SCORER_DEFAULT."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

from bench_gru import copy_gbps                       # noqa: E402
from graph_bench import peak_above, row, timed       # noqa: E402

PEAK_FLOPS = 155e12
PEAK_BYTES = 8e12
D, HIDDEN, DROPOUT = 64, [128, 64], 0.1


def make_scorer(ra, mode, dev):
    torch.manual_seed(7)
    if mode == 'mlp':
        s = ra.MLPScorer(ra.MLPModule([2 * D] + HIDDEN + [1], 'relu', DROPOUT))
    else:
        s = ra.FusionMFMLPScorer(D, HIDDEN[-1], ra.MLPModule([2 * D] + HIDDEN, 'relu', DROPOUT))
    s.fused = True
    return s.to(dev).train()


def core(ra, dev, mode, B, n, n_items, reps, warmup):
    g = torch.Generator(device=dev).manual_seed(B + n)
    scorer = make_scorer(ra, mode, dev)
    table = (torch.empty(n_items, D, device=dev).normal_(generator=g) * 0.1).requires_grad_(True)
    query = (torch.empty(B, D, device=dev).normal_(generator=g) * 0.1).requires_grad_(True)
    ids = torch.randint(1, n_items, (B, 1 + n), device=dev, generator=g)
    g_out = torch.empty(B, 1 + n, device=dev).normal_(generator=g)
    leaves = [table, query] + list(scorer.parameters())

    def fused():
        return scorer.score_ids(query, table, ids)

    def twin():
        return scorer._flat_scores(query.unsqueeze(1).expand(B, 1 + n, D), torch.nn.functional.embedding(ids, table, padding_idx=0))

    def fwd(f):
        def run():
            with torch.no_grad():
                return f()
        return run

    def both(f):
        def run():
            for t in leaves:
                t.grad = None
            return f().backward(g_out)
        return run

    assert fused() is not None
    ms = timed([fwd(fused), fwd(twin), both(fused), both(twin)], reps, warmup)
    out = dict(scorer=mode, B=B, n=n, d=D, hidden=HIDDEN, dropout=DROPOUT, pairs=B * (1 + n), n_items=n_items,
               forward=dict(fused=row(ms[0]), twin=row(ms[1])), forward_backward=dict(fused=row(ms[2]), twin=row(ms[3])))
    out['peak_bytes'] = {name: dict(forward=peak_above(fwd(f)), forward_backward=peak_above(both(f)))
                         for name, f in (('fused', fused), ('twin', twin))}
    M = B * (1 + n)
    flops_f = 2 * (2 * D * HIDDEN[0] + HIDDEN[0] * HIDDEN[1]) * M
    bytes_f = M * (8 + 4 * D + 4) + 4 * B * D
    bytes_fb = 3 * bytes_f + M * (4 + 2 * 4 * D) + 4 * B * D
    mf, mb = out['forward']['fused']['ms'], out['forward_backward']['fused']['ms']
    out['matrix_floor_ms'] = dict(forward=flops_f / PEAK_FLOPS * 1e3, forward_backward=4 * flops_f / PEAK_FLOPS * 1e3)
    out['byte_model_ms'] = dict(forward=bytes_f / PEAK_BYTES * 1e3, forward_backward=bytes_fb / PEAK_BYTES * 1e3)
    out['share_of_matrix_floor'] = dict(forward=out['matrix_floor_ms']['forward'] / mf,
                                        forward_backward=out['matrix_floor_ms']['forward_backward'] / mb)
    out['share_of_byte_model'] = dict(forward=out['byte_model_ms']['forward'] / mf,
                                      forward_backward=out['byte_model_ms']['forward_backward'] / mb)
    out['twin_over_fused'] = dict(forward=out['forward']['twin']['ms'] / mf, forward_backward=out['forward_backward']['twin']['ms'] / mb)
    return out


def make_model(ra, dev, n_items, n_users, n_neg, fused):
    g = torch.Generator().manual_seed(1)
    ds = ra.TripletDataset.from_mapped_ids(torch.randint(1, n_users, (4096,), generator=g).numpy(),
                                           torch.randint(1, n_items, (4096,), generator=g).numpy(), n_users=n_users, n_items=n_items)
    model = ra.NCF({'model': {'fused_scorer': fused}, 'train': {'negative_count': n_neg}})
    model._init_model(ds)
    model._init_parameter()
    return model.to(dev)


def topk(ra, dev, n_items, B, reps, warmup):
    model = make_model(ra, dev, n_items, B + 1, 1, True).eval()
    batch = {model.fuid: torch.arange(1, B + 1, device=dev)}

    def run():
        with torch.no_grad():
            return model.topk(batch, 100)
    ms = timed([run], reps, warmup)[0]
    return dict(B=B, n_items=n_items, k=100, chunk=model.config['eval'].get('pair_chunk', 8192), fused=row(ms),
                peak_bytes_fused=peak_above(run), twin_first_tensor_bytes=B * (n_items - 1) * 2 * D * 4,
                matrix_floor_ms=2 * (2 * D * HIDDEN[0] + HIDDEN[0] * HIDDEN[1]) * B * (n_items - 1) / PEAK_FLOPS * 1e3)


def training_step(ra, dev, n_items, B, n_neg, reps, warmup):
    steps = []
    for fused in (True, False):
        model = make_model(ra, dev, n_items, 100_001, n_neg, fused).train()
        g = torch.Generator().manual_seed(2)
        batch = {model.fuid: torch.randint(1, 100_001, (B,), generator=g).to(dev),
                 model.fiid: torch.randint(1, n_items, (B,), generator=g).to(dev), model.frating: torch.ones(B, device=dev)}

        def step(model=model, batch=batch):
            for t in model.parameters():
                t.grad = None
            model.training_step(batch).backward()
        steps.append(step)
    ms = timed(steps, reps, warmup)
    med = [statistics.median(t) for t in ms]
    return dict(model='NCF', score_mode='fusion', B=B, n=n_neg, n_items=n_items, fused_on=row(ms[0]), fused_off=row(ms[1]),
                off_over_on=med[1] / med[0], peak_bytes=dict(fused_on=peak_above(steps[0]), fused_off=peak_above(steps[1])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--items', type=int, default=100_001)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'ncf_bench.json'))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_ncf.py measures on the GPU: none found')
    import recstudio_amd as ra
    dev = torch.device('cuda')
    props = torch.cuda.get_device_properties(0)
    res = dict(device=props.name, compute_units=props.multi_processor_count, torch=torch.__version__, reps=a.reps, warmup=a.warmup,
               copy_gb_per_s_before=copy_gbps(dev))
    res['core'] = []
    for mode in ('fusion', 'mlp'):
        for B, n in ((65_536, 1), (16_384, 64)):
            res['core'].append(core(ra, dev, mode, B, n, a.items, a.reps, a.warmup))
            print(json.dumps(res['core'][-1]), file=sys.stderr, flush=True)
            torch.cuda.empty_cache()
    res['fused_wins_everywhere'] = all(c['twin_over_fused'][k] > 1.0 for c in res['core'] for k in ('forward', 'forward_backward'))
    res['topk'] = topk(ra, dev, a.items, 2048, max(a.reps // 4, 3), 2)
    print(json.dumps(res['topk']), file=sys.stderr, flush=True)
    res['training_step'] = [training_step(ra, dev, a.items, 65_536, 1, a.reps, a.warmup),
                            training_step(ra, dev, a.items, 16_384, 64, a.reps, a.warmup)]
    res['copy_gb_per_s_after'] = copy_gbps(dev)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')
    print(json.dumps(res))


if __name__ == '__main__':
    main()
