"""Times SGL's per-step graph augmentation (ops.graph_dropout / rsa_graph_dropout) on the graph of tools/bench_lightgcn.py: next to
one propagation layer and next to the same augmentation written with torch ops, inside a whole SGL training step next to LightGCN's,
and the price of propagating over a thinned view without compacting it.  One process, one device, the arms of a group alternating,
device events around every call, warm-up calls first.  Prints one JSON object and writes it to profiles/sgl_bench.json.

    python tools/bench_sgl.py [--users 1048576 --items 1048576 --inter 67108864 --dim 64 --batch 2048 --layers 3 --reps 10 --warmup 3]

Arms:
  (a) dropout        ops.graph_dropout at ssl_ratio 0.1: mask, both degree vectors, values and t_values
      layer          ops.spmm_csr, one middle layer of LightGCN at --dim over the base values
      torch_ops      the augmentation with torch ops: rand, floor, two bincounts over the kept edges, pow, two gathers and the product,
                     and the gather through rev for the transposed weights (no re-sort, the edge rows precomputed outside the clock)
  (b) sgl_step       SGL.training_step + backward at --batch, --layers layers ('ED'), next to LightGCN.training_step on the same graph
  (c) layer_view     the layer of (a) over the values of a view at ssl_ratio 0.1 and 0.5, next to the base values: the dropped edges
                     are still gathered (their products are exact zeros), which is what compacting the views would save
Recorded: median / min / max in ms; for (a) the byte model  nnz (4 indices + 8 rev + 4 values + 4 t_values) + 2 passes over them for the
inputs, and the ratios dropout / layer and dropout / torch_ops."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from graph_bench import row, timed, zipf_graph      # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--users', type=int, default=1 << 20)
    ap.add_argument('--items', type=int, default=1 << 20)
    ap.add_argument('--inter', type=int, default=1 << 26)
    ap.add_argument('--dim', type=int, default=64)
    ap.add_argument('--batch', type=int, default=2048)
    ap.add_argument('--layers', type=int, default=3)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'sgl_bench.json'))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_sgl.py measures on the GPU: none found')
    import recstudio_amd as ra
    from recstudio_amd import ops
    dev = torch.device('cuda')
    nu, ni = a.users + 1, a.items + 1
    n = nu + ni
    adj, users, items = zipf_graph(a.users, a.items, a.inter, dev)
    nnz, rev = adj.nnz, adj.rev
    torch.cuda.empty_cache()
    deg = adj.indptr[1:] - adj.indptr[:-1]
    res = dict(device=torch.cuda.get_device_name(0), users=a.users, items=a.items, interactions=a.inter, rows=n, nnz=nnz,
               degree_max=int(deg.max()), long_row=ops.GRAPH_DROPOUT_LONG_ROW, long_rows=int((deg > ops.GRAPH_DROPOUT_LONG_ROW).sum()),
               chunk=adj.plan.chunk, dim=a.dim, reps=a.reps, warmup=a.warmup)
    print(f'graph built: {n} rows, {nnz} non-zeros', file=sys.stderr, flush=True)
    g = torch.Generator(device=dev).manual_seed(3)
    d = a.dim
    x = torch.empty(n, d, device=dev).normal_(0, 0.1, generator=g)
    y, acc = torch.empty_like(x), torch.zeros_like(x)

    # (a)
    rows, cols = torch.repeat_interleave(torch.arange(n, device=dev), deg), adj.indices.long()
    keep_prob = 0.9

    def torch_ops():
        keep = torch.floor(torch.rand(nnz, device=dev) + keep_prob).bool()
        in_deg = torch.bincount(rows[keep], minlength=n)
        out_deg = torch.bincount(cols[keep], minlength=n)
        w = (out_deg.double().pow(-0.5)[cols] * in_deg.double().pow(-0.5)[rows]).float()
        values = torch.where(keep, w, torch.zeros_like(w))
        return values, values[rev], in_deg, out_deg

    arm_drop = lambda: ops.graph_dropout(adj.indptr, adj.indices, rev, keep_prob)                                          # noqa: E731
    arm_layer = lambda: ops.spmm_csr(adj.indptr, adj.indices, adj.values, x, plan=adj.plan, y=y, acc=acc)                 # noqa: E731
    ms = timed([arm_drop, arm_layer, torch_ops], a.reps, a.warmup)
    torch.manual_seed(11)
    mine = arm_drop()
    torch.manual_seed(11)
    theirs = torch_ops()
    same = bool(torch.equal(mine[2].long(), theirs[2]) and torch.equal(mine[3].long(), theirs[3]))
    worst = float(((mine[0].double() - theirs[0].double()).abs() / theirs[0].double().abs().clamp_min(1e-300)).max())
    del theirs
    bytes_a = nnz * (2 * (4 + 8) + 4 + 4)
    res['augmentation'] = dict(ssl_ratio=0.1, dropout=dict(row(ms[0]), model_bytes=bytes_a, bytes_per_s=bytes_a / (statistics.median(ms[0]) * 1e-3)),
                               layer=row(ms[1]), torch_ops=row(ms[2]), dropout_over_layer=statistics.median(ms[0]) / statistics.median(ms[1]),
                               dropout_over_torch_ops=statistics.median(ms[0]) / statistics.median(ms[2]),
                               degrees_equal_torch_ops=same, values_max_relative_difference_to_torch_ops=worst)
    print(json.dumps(res['augmentation']), file=sys.stderr, flush=True)
    del rows, cols
    torch.cuda.empty_cache()

    # (c)
    v01, v05 = mine[0], ops.graph_dropout(adj.indptr, adj.indices, rev, 0.5)[0]
    del mine
    fns = [lambda v=v: ops.spmm_csr(adj.indptr, adj.indices, v, x, plan=adj.plan, y=y, acc=acc) for v in (adj.values, v01, v05)]
    ms = timed(fns, a.reps, a.warmup)
    res['layer_over_view'] = dict(base=row(ms[0]), ssl_ratio_0_1=row(ms[1]), ssl_ratio_0_5=row(ms[2]),
                                  kept_0_1=float((v01 != 0).float().mean()), kept_0_5=float((v05 != 0).float().mean()))
    print(json.dumps(res['layer_over_view']), file=sys.stderr, flush=True)
    del v01, v05, fns, x, y, acc
    torch.cuda.empty_cache()

    # (b)
    class LightGCNOnDevice(ra.LightGCN):
        def _get_graph(self, train_data):
            return adj

    class SGLOnDevice(ra.SGL):
        def _get_graph(self, train_data):
            return adj

    data = ra.TripletDataset.from_mapped_ids(users, items, n_users=nu, n_items=ni)
    cfg = {'model': {'embed_dim': d, 'n_layers': a.layers}, 'train': {'negative_count': 1}}
    steps = []
    for cls in (SGLOnDevice, LightGCNOnDevice):
        m = cls(cfg)
        m._init_model(data)
        m._init_parameter()
        m.to(dev)
        gb = torch.Generator(device=dev).manual_seed(5)
        pick = [torch.randint(0, a.inter, (a.batch,), device=dev, generator=gb).cpu() for _ in range(4)]
        batches = [{data.fuid: users[p].to(dev), data.fiid: items[p].to(dev), data.frating: torch.ones(a.batch, device=dev)} for p in pick]
        turn = {'k': 0}

        def step(m=m, batches=batches, turn=turn):
            turn['k'] += 1
            for p in m.parameters():
                p.grad = None
            m.training_step(batches[turn['k'] % len(batches)]).backward()
        steps.append(step)
    ms = timed(steps, a.reps, a.warmup)
    res['training_step'] = dict(batch=a.batch, layers=a.layers, dim=d, aug_type='ED', ssl_ratio=0.1, sgl=row(ms[0]), lightgcn=row(ms[1]),
                                sgl_over_lightgcn=statistics.median(ms[0]) / statistics.median(ms[1]))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')
    print(json.dumps(res))


if __name__ == '__main__':
    main()
