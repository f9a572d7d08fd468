"""Times the whole Adagrad training step (fused.FusedBPRAdagrad.step) next to the lazy-Adam step (fused.FusedBPRAdam.step) and the
all-sorted in-place SGD step (fused.bpr_sgd_step(in_forward=False): the same forward and the same sorted apply passes with no state
table) at the headline shape, in one process on one device, the three alternating (a, b, c, a, b, c, ...), device events around
every call, warm-up calls first; prints one JSON object and writes it to profiles/adagrad_step_bench.json.

    python tools/bench_adagrad_step.py [--items 10000001 --users 1000001 --dim 128 --batch 65536 --neg 64 --reps 15 --warmup 5]

Per step: median / min / max in ms and the fraction of the 8 TB/s peak on the byte model of DESIGN 4.3 -- per (query, negative)
pair the forward's bytes plus one read-modify-write of a d-float row per table the rule keeps (SGD: the weights; Adagrad: weights
and state_sum; lazy Adam: weights, exp_avg, exp_avg_sq), and the same per query for the user side:
    bytes = B n (forward + T (2 * 4d) (1 + 1 / n)),   T = 1 / 2 / 3,   forward = 556 B at d = 128, n = 64.
``adagrad_not_slower_than_adam`` is the one condition the model implies: fewer bytes through the same passes."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_BYTES_PER_S = 8e12
FORWARD_BYTES = 556          # per (query, negative) pair at d = 128, n = 64 (1596 = forward + 2 * 4d + 2 * 4d / n)


def timed(fns, reps, warmup):
    """[ms per call] per function, the functions called in turn."""
    for _ in range(warmup):
        for f in fns:
            f()
    torch.cuda.synchronize()
    ms = [[] for _ in fns]
    for _ in range(reps):
        for i, f in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            f()
            b.record()
            b.synchronize()
            ms[i].append(a.elapsed_time(b))
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--items', type=int, default=10_000_001)
    ap.add_argument('--users', type=int, default=1_000_001)
    ap.add_argument('--dim', type=int, default=128)
    ap.add_argument('--batch', type=int, default=65_536)
    ap.add_argument('--neg', type=int, default=64)
    ap.add_argument('--reps', type=int, default=15)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'adagrad_step_bench.json'))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_adagrad_step.py measures on the GPU: none found')
    import recstudio_amd as ra
    from recstudio_amd import fused
    dev = 'cuda'
    N, U, d, B, n = a.items, a.users, a.dim, a.batch, a.neg
    g = torch.Generator(device=dev).manual_seed(12)
    iw = torch.empty(N, d, device=dev).normal_(0, 0.1, generator=g)
    iw[0] = 0
    uw = torch.empty(U, d, device=dev).normal_(0, 0.1, generator=g)
    counts = (torch.rand(N, generator=torch.Generator().manual_seed(2)) ** 8 * 1e4).long()
    sampler = ra.PopularSamplerModel(counts).to(dev)
    # a few batches in turn, so that no step finds the previous call's rows in the cache
    batches = [(torch.randint(1, U, (B,), device=dev, generator=g), torch.randint(1, N, (B,), device=dev, generator=g)) for _ in range(4)]
    turn = {'k': 0}

    def batch():
        turn['k'] += 1
        return batches[turn['k'] % len(batches)]

    # one pair of weight tables under all three rules (a step's time does not depend on the values; small rates keep them finite)
    adagrad = fused.FusedBPRAdagrad(iw, uw, lr=1e-3)
    adam = fused.FusedBPRAdam(iw, uw, lr=1e-4)

    def step_adagrad():
        uid, pos = batch()
        adagrad.step(n, user_ids=uid, pos_ids=pos, sampler=sampler)

    def step_adam():
        uid, pos = batch()
        adam.step(n, user_ids=uid, pos_ids=pos, sampler=sampler)

    def step_sgd():
        uid, pos = batch()
        fused.bpr_sgd_step(iw, uw, n, 1e-3, user_ids=uid, pos_ids=pos, sampler=sampler, in_forward=False)

    names = ('adagrad', 'adam', 'sgd_all_sorted')
    tables = {'adagrad': 2, 'adam': 3, 'sgd_all_sorted': 1}
    ms = timed([step_adagrad, step_adam, step_sgd], a.reps, a.warmup)
    res = dict(device=torch.cuda.get_device_name(0), items=N, users=U, dim=d, batch=B, num_neg=n, sampler='popular', reps=a.reps,
               warmup=a.warmup, peak_bytes_per_s=PEAK_BYTES_PER_S, forward_bytes_per_pair=FORWARD_BYTES if (d, n) == (128, 64) else None)
    for name, t in zip(names, ms):
        med = statistics.median(t)
        row = dict(ms=med, ms_min_max=(min(t), max(t)), tables_per_row=tables[name])
        if (d, n) == (128, 64):
            row['bytes_per_pair'] = FORWARD_BYTES + tables[name] * 2 * 4 * d * (1 + 1 / n)
            row['fraction_of_peak'] = B * n * row['bytes_per_pair'] / (med * 1e-3) / PEAK_BYTES_PER_S
        res[name] = row
    res['adagrad_not_slower_than_adam'] = res['adagrad']['ms'] <= res['adam']['ms']
    res['finite'] = bool(torch.isfinite(iw).all()) and bool(torch.isfinite(uw).all())
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')
    print(json.dumps(res))
    if not res['adagrad_not_slower_than_adam']:
        raise SystemExit('the Adagrad step is slower than the lazy-Adam step of the same run: fewer bytes through the same passes, so something is wrong')


if __name__ == '__main__':
    main()
