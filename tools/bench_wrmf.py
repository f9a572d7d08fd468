"""Times one WRMF half-epoch through ops.als_solve (rsa_als.hip) against the reference's op sequence (padded gather, two bmm,
torch.linalg.solve, the loss pass: models_mf.als_step_torch).  One process, one device, the arms alternating, device events around
every half-epoch, warm-up first; a streaming copy of 1 GiB is timed at the start and at the end as the record of the box's state.
Prints one JSON object and writes it to profiles/wrmf_bench.json.

    python tools/bench_wrmf.py [--reps 20 --warmup 2 --users 1048576 --items 262144 --inter 16777216]

Data: dataset.synthetic_interactions (users uniform, items Zipf(1)), tables N(0, 0.1^2) with row 0 zero, alpha 1, lambda 0.5,
d = 64 and 128, the user side (rows = users, table = items) and the item side.
Arms, each a whole half-epoch with the loss:
  (a) fused      gram = table^T table, then ONE ops.als_solve over every row, max_parts exact (als_max_parts of the host indptr)
  (b) ref_100    als_step_torch over length-sorted batches of the reference's batch_size 100, ids padded on the device from the CSR;
                 a batch whose [B, L, d] gather would pass --budget bytes is cut into smaller ones (at the head of the item side)
  (b) ref_big    the same with the largest batches the budget holds, at most MAX_BATCH = 65536 rows (hipBLAS's batched LU behind
                 torch.linalg.solve fails to allocate above that)
Peak memory above the inputs for each arm.  Floors for (a): 2 d^2 nnz + rows d^3 / 3 flops at 155 TF (fp32 matrix), and
nnz (2 * 4 d + 12) + rows * 8 d bytes at 8 TB/s (every history row read by the Gram pass and again by the loss pass, ids and ratings,
x and the gram read per row from cache not counted); ``nearer`` names the floor the measured time is closer to.
``fused_wins_everywhere``: (a) beats both (b) arms on both sides at both widths by more than 15 % -- the rule behind
models_mf.FUSED_ALS_DEFAULT."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

from bench_gru import copy_gbps                      # noqa: E402
from graph_bench import peak_above, row, timed       # noqa: E402

PEAK_FLOPS, PEAK_BYTES, MARGIN = 155e12, 8e12, 1.15
ALPHA, LAM = 1.0, 0.5
MAX_BATCH = 1 << 16


def csr(key, val, n, dev):
    order = torch.sort(key, stable=True).indices
    indptr = torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(torch.bincount(key, minlength=n), 0)])
    return indptr, val[order].to(torch.int32).to(dev)


def batches(deg_sorted, d, batch, budget):
    """[start, end) over the length-sorted rows: at most ``batch`` rows (None: as many as fit), B * L * d * 4 <= budget (one row always
    goes).  The rows are sorted by descending length, so a batch's L is its first row's."""
    out, s, n = [], 0, len(deg_sorted)
    while s < n:
        L = max(int(deg_sorted[s]), 1)
        fit = max(int(budget // (L * d * 4)), 1)
        e = min(n, s + min(batch or MAX_BATCH, fit))
        out.append((s, e, L))
        s = e
    return out


def padded_sweep(als_step_torch, indptr_dev, indices, order_dev, plan, table, nnz):
    def run():
        gram = table.T @ table
        total = torch.zeros((), device=table.device)
        for s, e, L in plan:
            rows = order_dev[s:e]
            start, deg = indptr_dev[rows], indptr_dev[rows + 1] - indptr_dev[rows]
            pos = torch.arange(L, device=table.device)
            live = pos[None] < deg[:, None]
            ids = torch.where(live, indices[(start[:, None] + pos[None]).clamp(max=nnz - 1)].long(), 0)
            x, loss = als_step_torch(ids, live.float(), table, gram, ALPHA, LAM)
            total += loss.sum()
        return total
    return run


def side(ops, als_step_torch, name, indptr, indices, table, d, reps, warmup, budget):
    dev = table.device
    nnz, rows = indices.numel(), indptr.numel() - 1
    deg = indptr[1:] - indptr[:-1]
    order = torch.sort(deg, descending=True, stable=True).indices
    order = order[deg[order] > 0]                                       # the loaders hold the rows with a training interaction
    deg_sorted = deg[order].tolist()
    indptr_dev, order_dev = indptr.to(dev), order.to(dev)
    max_parts = ops.als_max_parts(indptr)

    def fused():
        return ops.als_solve(indptr_dev, indices, table, table.T @ table, ALPHA, LAM, want_loss=True, max_parts=max_parts)

    plans = dict(ref_100=batches(deg_sorted, d, 100, budget), ref_big=batches(deg_sorted, d, None, budget))
    arms = dict(fused=fused, **{k: padded_sweep(als_step_torch, indptr_dev, indices, order_dev, p, table, nnz) for k, p in plans.items()})
    names = list(arms)
    ms = timed([arms[n] for n in names], reps, warmup)
    out = dict(side=name, d=d, rows=rows, rows_solved=len(deg_sorted), nnz=nnz, longest_row=deg_sorted[0], max_parts=max_parts,
               batches={k: len(p) for k, p in plans.items()}, largest_batch={k: max(e - s for s, e, _ in p) for k, p in plans.items()},
               **{n: row(ms[i]) for i, n in enumerate(names)})
    out['peak_bytes'] = {n: peak_above(f) for n, f in arms.items()}
    a = out['fused']['ms']
    out['over_fused'] = {n: out[n]['ms'] / a for n in names if n != 'fused'}
    flop_ms = (2.0 * d * d * nnz + len(deg_sorted) * d ** 3 / 3.0) / PEAK_FLOPS * 1e3
    byte_ms = (nnz * (8.0 * d + 12) + rows * 8.0 * d) / PEAK_BYTES * 1e3
    out['floors'] = dict(matrix_ms=flop_ms, byte_ms=byte_ms, share_of_matrix_floor=flop_ms / a, share_of_byte_model=byte_ms / a,
                         nearer='matrix' if flop_ms > byte_ms else 'bytes')
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--users', type=int, default=1 << 20)
    ap.add_argument('--items', type=int, default=1 << 18)
    ap.add_argument('--inter', type=int, default=1 << 24)
    ap.add_argument('--budget', type=int, default=8 << 30, help='bytes of the [B, L, d] gather of one padded batch')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'wrmf_bench.json'))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_wrmf.py measures on the GPU: none found')
    from recstudio_amd import dataset, ops
    from recstudio_amd.models_mf import als_step_torch
    dev = torch.device('cuda')
    props = torch.cuda.get_device_properties(0)
    res = dict(device=props.name, compute_units=props.multi_processor_count, torch=torch.__version__, reps=a.reps, warmup=a.warmup,
               users=a.users, items=a.items, inter=a.inter, budget=a.budget, alpha=ALPHA, lam=LAM, chunk=ops.ALS_CHUNK, margin=MARGIN,
               copy_gb_per_s_before=copy_gbps(dev), sides=[])
    u, i = (torch.from_numpy(t) for t in dataset.synthetic_interactions(a.users, a.items, a.inter, alpha=1.0))
    by_user, by_item = csr(u, i, a.users + 1, dev), csr(i, u, a.items + 1, dev)
    for d in (64, 128):
        gen = torch.Generator(device=dev).manual_seed(d)
        tables = [torch.empty(n + 1, d, device=dev).normal_(0, 0.1, generator=gen) for n in (a.users, a.items)]
        for t in tables:
            t[0] = 0
        for name, (indptr, indices), table in (('users', by_user, tables[1]), ('items', by_item, tables[0])):
            res['sides'].append(side(ops, als_step_torch, name, indptr, indices, table, d, a.reps, a.warmup, a.budget))
            print(json.dumps(res['sides'][-1]), file=sys.stderr, flush=True)
            torch.cuda.empty_cache()
    res['fused_wins_everywhere'] = all(v > MARGIN for s in res['sides'] for v in s['over_fused'].values())
    res['copy_gb_per_s_after'] = copy_gbps(dev)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')
    print(json.dumps(res))


if __name__ == '__main__':
    main()
