"""Times the user-history bag kernel pair (ops.bag_pool / ops.bag_pool_backward: rsa_bag.hip) against the reference's op sequence
and torch's own bag, and what the pair does to MultiDAE's and MultiVAE's step.  One process, one device, the arms of a group
alternating, device events around every call, warm-up calls first; a streaming copy of 1 GiB is timed at the start and at the end
as the record of the box's state.  Prints one JSON object and writes it to profiles/multivae_bench.json.

    python tools/bench_multivae.py [--reps 20 --warmup 5]

Shapes: the reference's two configurations, B = 500, d = 600 (MultiVAE) and B = 256, d = 200 (MultiDAE), over N = 20 000 items.
Bag lengths (``bag_lengths``): round(exp(normal(log(140) - 0.5, 1))) clamped to [1, 3000] under torch.Generator seed 11, bag 0 set
to 3000 -- long-tailed, mean about 140; ids uniform in [1, N), right-padded to the longest bag.
Groups:
  (1) core            'rsqrt' bag sums, forward and forward + backward (the gradient of the table from a given g [B, d]):
                        fused           seqmodule.bag_pool: the autograd node over the kernel pair
                        twin            seqmodule.bag_pool_torch: embedding [B, L, d] -> sum -> divide
                        embedding_bag   F.embedding_bag(ids [B, L], mode='sum', padding_idx=0) then the divide: torch's own bag on
                                        the same padded matrix
                        embedding_bag_offsets   the same op on the compacted ids with offsets (built outside the timing): torch's
                                        bag at its best
                      Peak memory above the inputs; the byte model (live rows * 4 d + 8 B L of ids + 4 B d of output; backward: as
                      much again for dW's touched rows, + g) at 8 TB/s and the fused arm's share of it.
  (2) training_step   MultiDAE (B = 256, d = 200) and MultiVAE (B = 500, d = 600) .training_step + backward on a synthetic
                      UserDataset with the same length law, model.fused_bag on and off.
``fused_wins_everywhere``: the pair beats the twin AND both embedding_bag forms forward + backward at both shapes by more than 15 %
(the box-to-box spread DESIGN.md works with) -- the rule behind retriever.FUSED_BAG_DEFAULT."""
import argparse
import json
import math
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

from bench_gru import copy_gbps                      # noqa: E402
from graph_bench import peak_above, row, timed       # noqa: E402

PEAK_BYTES = 8e12
N_ITEMS = 20_000
LENGTH_LAW = dict(kind='round(exp(normal(mu, sigma))) clamped, bag 0 = hi', mu=math.log(140) - 0.5, sigma=1.0, lo=1, hi=3000, seed=11)
MARGIN = 1.15


def bag_lengths(B, scale=1.0):
    gen = torch.Generator().manual_seed(LENGTH_LAW['seed'])
    n = torch.empty(B).normal_(LENGTH_LAW['mu'], LENGTH_LAW['sigma'], generator=gen).exp().round().clamp(LENGTH_LAW['lo'], LENGTH_LAW['hi'])
    n[0] = LENGTH_LAW['hi']
    return (n * scale).round().long()


def padded_ids(lengths, N, seed=12):
    gen = torch.Generator().manual_seed(seed)
    L = int(lengths.max())
    ids = torch.randint(1, N, (len(lengths), L), generator=gen)
    return ids * (torch.arange(L).view(1, L) < lengths.view(-1, 1))


def core(seqmodule, dev, B, d, reps, warmup):
    lengths = bag_lengths(B)
    ids = padded_ids(lengths, N_ITEMS).to(dev)
    L = ids.shape[1]
    gen = torch.Generator(device=dev).manual_seed(d)
    w = torch.empty(N_ITEMS, d, device=dev).normal_(0, 0.1, generator=gen)
    w[0] = 0
    w.requires_grad_(True)
    g_out = torch.empty(B, d, device=dev).normal_(generator=gen)
    live = ids != 0
    flat = ids[live]
    offsets = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), live.sum(1).cumsum(0)[:-1]])
    root = live.sum(1, keepdim=True).float().pow(0.5)

    forms = {
        'fused': lambda: seqmodule.bag_pool(w, ids, 'rsqrt', fused=True),
        'twin': lambda: seqmodule.bag_pool_torch(w, ids, 'rsqrt'),
        'embedding_bag': lambda: F.embedding_bag(ids, w, mode='sum', padding_idx=0) / root,
        'embedding_bag_offsets': lambda: F.embedding_bag(flat, w, offsets, mode='sum') / root,
    }

    def fwd(f):
        def run():
            with torch.no_grad():
                return f()
        return run

    def both(f):
        def run():
            w.grad = None
            return f().backward(g_out)
        return run

    names = list(forms)
    ms = timed([fwd(forms[n]) for n in names] + [both(forms[n]) for n in names], reps, warmup)
    out = dict(B=B, d=d, L=L, n_items=N_ITEMS, live_rows=int(live.sum()), mean_length=float(lengths.float().mean()),
               forward={n: row(ms[i]) for i, n in enumerate(names)},
               forward_backward={n: row(ms[len(names) + i]) for i, n in enumerate(names)})
    out['peak_bytes'] = {n: dict(forward=peak_above(fwd(f)), forward_backward=peak_above(both(f))) for n, f in forms.items()}
    bytes_f = out['live_rows'] * 4 * d + 8 * B * L + 4 * B * d
    touched = int(torch.unique(flat).numel())
    bytes_fb = bytes_f + 8 * B * L + out['live_rows'] * 4 * d + touched * 4 * d
    mf, mb = out['forward']['fused']['ms'], out['forward_backward']['fused']['ms']
    out['byte_model_ms'] = dict(forward=bytes_f / PEAK_BYTES * 1e3, forward_backward=bytes_fb / PEAK_BYTES * 1e3)
    out['share_of_byte_model'] = dict(forward=out['byte_model_ms']['forward'] / mf, forward_backward=out['byte_model_ms']['forward_backward'] / mb)
    out['over_fused'] = {n: dict(forward=out['forward'][n]['ms'] / mf, forward_backward=out['forward_backward'][n]['ms'] / mb)
                         for n in names if n != 'fused'}
    return out


def training_step(ra, dev, cls, B, d, reps, warmup):
    lengths = bag_lengths(B, scale=1.25)                     # the train cut is 0.8 of a user's interactions
    users = torch.repeat_interleave(torch.arange(1, B + 1), lengths)
    items = torch.randint(1, N_ITEMS, (len(users),), generator=torch.Generator().manual_seed(13))
    ds = ra.UserDataset.from_mapped_ids(users, items, n_users=B + 1, n_items=N_ITEMS)
    trn = ds.build(shuffle=False)[0]
    steps, models = [], []
    for fused in (True, False):
        model = cls({'model': dict(embed_dim=d, fused_bag=fused), 'train': {'batch_size': B}})
        model._init_model(trn)
        model._init_parameter()
        model.to(dev)
        model.train()
        trn.eval_mode = False
        batch = {k: v.to(dev) for k, v in trn[torch.arange(len(trn))].items()}

        def step(model=model, batch=batch):
            for t in model.parameters():
                t.grad = None
            model.training_step(batch).backward()
        steps.append(step)
        models.append(model)
    ms = timed(steps, reps, warmup)
    med = [statistics.median(t) for t in ms]
    return dict(model=cls.__name__, B=len(trn), d=d, L=int(batch[ds.fiid].shape[1]), n_items=N_ITEMS, fused_on=row(ms[0]),
                fused_off=row(ms[1]), off_over_on=med[1] / med[0],
                peak_bytes=dict(fused_on=peak_above(steps[0]), fused_off=peak_above(steps[1])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'multivae_bench.json'))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_multivae.py measures on the GPU: none found')
    import recstudio_amd as ra
    from recstudio_amd import seqmodule
    dev = torch.device('cuda')
    props = torch.cuda.get_device_properties(0)
    res = dict(device=props.name, compute_units=props.multi_processor_count, torch=torch.__version__, reps=a.reps, warmup=a.warmup,
               length_law=LENGTH_LAW, copy_gb_per_s_before=copy_gbps(dev))
    res['core'] = []
    for B, d in ((500, 600), (256, 200)):
        res['core'].append(core(seqmodule, dev, B, d, a.reps, a.warmup))
        print(json.dumps(res['core'][-1]), file=sys.stderr, flush=True)
        torch.cuda.empty_cache()
    res['margin'] = MARGIN
    res['fused_wins_everywhere'] = all(v['forward_backward'] > MARGIN for c in res['core'] for v in c['over_fused'].values())
    res['training_step'] = [training_step(ra, dev, ra.MultiVAE, 500, 600, a.reps, a.warmup),
                            training_step(ra, dev, ra.MultiDAE, 256, 200, a.reps, a.warmup)]
    res['copy_gb_per_s_after'] = copy_gbps(dev)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')
    print(json.dumps(res))


if __name__ == '__main__':
    main()
