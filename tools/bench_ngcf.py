"""Times NGCF's fused BiCombiner layer (ops.bi_combine / ops.bi_combine_backward: rsa_combine.hip) on the graph of
tools/bench_lightgcn.py: forward and backward next to the same layer in torch ops (BiCombiner.forward_torch and its autograd
backward) and next to one plain ops.spmm_csr layer; the [nnz] pass that forms the per-edge values of a thinned view; a whole NGCF
training step next to LightGCN's; and the peak memory of a layer in both forms.  One process, one device, the arms of a group
alternating, device events around every call, warm-up calls first.  Prints one JSON object and writes it to
profiles/ngcf_bench.json.

    python tools/bench_ngcf.py [--users 1048576 --items 1048576 --inter 67108864 --dim 64 --batch 2048 --layers 3 --reps 10 --warmup 3]

Arms:
  (a) forward        fused (h and the normalised block written into a 4 d wide table) / torch_form (forward_torch: the same mask rule)
      backward       fused (ops.bi_combine_backward from g_h and the table's gradient) / torch_form (autograd through forward_torch,
                     timed as forward + backward minus the forward above) / spmm (one plain ops.spmm_csr layer, y only)
      the yardstick for "the fusion paid" is fused <= torch_form in both; achieved bytes/s against the model of 1 KB per row
      (forward: read x, m, write h, n) and 2.5 KB per row (backward: both passes read x, m, g_h, g_n; dx, dm written)
  (b) values pass    keep * inv_out[indices] and t_values != 0 over [nnz] (what LeftAdj.thinned adds to ops.graph_dropout), next to
                     ops.graph_dropout itself
  (c) peak memory    one layer forward + backward in both forms: bytes allocated above the inputs
  (d) training_step  NGCF.training_step + backward at --batch, --layers (layer_size [dim] * (layers + 1)), next to LightGCN's
Recorded: median / min / max in ms and the ratios."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from graph_bench import peak_above, row, timed, zipf_graph      # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--users', type=int, default=1 << 20)
    ap.add_argument('--items', type=int, default=1 << 20)
    ap.add_argument('--inter', type=int, default=1 << 26)
    ap.add_argument('--dim', type=int, default=64)
    ap.add_argument('--batch', type=int, default=2048)
    ap.add_argument('--layers', type=int, default=3)
    ap.add_argument('--dropout', type=float, default=0.1)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'ngcf_bench.json'))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_ngcf.py measures on the GPU: none found')
    import recstudio_amd as ra
    from recstudio_amd import graphmodule, ops, rng
    dev = torch.device('cuda')
    d, p = a.dim, a.dropout
    nu, ni = a.users + 1, a.items + 1
    n = nu + ni
    adj, users, items = zipf_graph(a.users, a.items, a.inter, dev)
    torch.cuda.empty_cache()
    res = dict(device=torch.cuda.get_device_name(0), users=a.users, items=a.items, interactions=a.inter, rows=n, nnz=adj.nnz, dim=d,
               dropout=p, chunk=adj.plan.chunk, reps=a.reps, warmup=a.warmup)
    print(f'graph built: {n} rows, {adj.nnz} non-zeros', file=sys.stderr, flush=True)

    # (a)
    g = torch.Generator(device=dev).manual_seed(3)
    x = torch.empty(n, d, device=dev).normal_(0, 0.1, generator=g)
    m = torch.empty(n, d, device=dev).normal_(0, 0.1, generator=g)
    g_h = torch.empty(n, d, device=dev).normal_(0, 0.1, generator=g)
    table, g_table = torch.empty(n, 4 * d, device=dev), torch.empty(n, 4 * d, device=dev).normal_(0, 0.1, generator=g)
    layer = graphmodule.BiCombiner(d, d, dropout=p).to(dev)
    w1, b1, w2, b2 = (t.detach() for t in (layer.linear_sum.weight, layer.linear_sum.bias, layer.linear_product.weight,
                                           layer.linear_product.bias))
    state = {}

    def fused_forward():
        state['pc'] = rng.reserve(n * d, 4, dev)
        return ops.bi_combine(x, m, w1, w2, b1, b2, p=p, philox=state['pc'], out=table, col=d)

    def torch_forward():
        with torch.no_grad():
            return layer.forward_torch(x, m)

    def fused_backward():
        return ops.bi_combine_backward(x, m, w1, w2, b1, b2, g_h=g_h, g_out=g_table, col=d, p=p, philox=state['pc'])

    xg, mg = x.clone().requires_grad_(), m.clone().requires_grad_()

    def torch_forward_backward():
        for t in (xg, mg, *layer.parameters()):
            t.grad = None
        h, nrm = layer.forward_torch(xg, mg)
        torch.autograd.backward([h, nrm], [g_h, g_table[:, d:2 * d]])

    y = torch.empty_like(x)

    def spmm():
        ops.spmm_csr(adj.indptr, adj.indices, adj.values, x, plan=adj.plan, y=y)

    ms = timed([fused_forward, torch_forward, fused_backward, torch_forward_backward, spmm], a.reps, a.warmup)
    med = [statistics.median(t) for t in ms]
    torch_bwd = med[3] - med[1]
    res['layer'] = dict(
        forward=dict(fused=row(ms[0]), torch_form=row(ms[1]), torch_form_over_fused=med[1] / med[0],
                     model_bytes_per_row=16 * d, fused_bytes_per_s=16 * d * n / (med[0] * 1e-3)),
        backward=dict(fused=row(ms[2]), torch_forward_plus_backward=row(ms[3]), torch_form_ms=torch_bwd, torch_form_over_fused=torch_bwd / med[2],
                      model_bytes_per_row=40 * d, fused_bytes_per_s=40 * d * n / (med[2] * 1e-3)),
        spmm_layer=row(ms[4]), fused_forward_over_spmm=med[0] / med[4], fused_backward_over_spmm=med[2] / med[4])
    print(json.dumps(res['layer']), file=sys.stderr, flush=True)

    # (c)
    def fused_both():
        fused_forward()
        return fused_backward()

    res['layer_peak_bytes'] = dict(table_bytes=n * d * 4, fused=peak_above(fused_both), torch_form=peak_above(torch_forward_backward))
    res['layer_peak_bytes']['saved'] = res['layer_peak_bytes']['torch_form'] - res['layer_peak_bytes']['fused']
    print(json.dumps(res['layer_peak_bytes']), file=sys.stderr, flush=True)
    for t in (xg, mg, *layer.parameters()):
        t.grad = None
    del x, m, g_h, table, g_table, xg, mg, y
    torch.cuda.empty_cache()

    # (b)
    adj.rev                                                                    # (built before the clock)
    view = {}

    def dropout_kernel():
        view['v'] = ops.graph_dropout(adj.indptr, adj.indices, adj.rev, 0.9, want_keep=True)

    def values_pass():
        _, t_values, _, out_deg, keep = view['v']
        inv_out = (1.0 / out_deg.clamp_min(1).double()).to(torch.float32)
        return keep.to(torch.float32) * inv_out[adj.indices.long()], (t_values != 0).to(torch.float32)

    ms = timed([dropout_kernel, values_pass], a.reps, a.warmup)
    med = [statistics.median(t) for t in ms]
    res['thinned_view'] = dict(graph_dropout=row(ms[0]), values_pass=row(ms[1]), values_pass_over_graph_dropout=med[1] / med[0])
    print(json.dumps(res['thinned_view']), file=sys.stderr, flush=True)
    view.clear()
    torch.cuda.empty_cache()

    # (d)
    def on_device(cls):
        class OnDevice(cls):
            def _get_graph(self, train_data):
                return adj
        return OnDevice

    data = ra.TripletDataset.from_mapped_ids(users, items, n_users=nu, n_items=ni)
    cfgs = {ra.NGCF: {'model': {'embed_dim': d, 'layer_size': [d] * (a.layers + 1), 'mess_dropout': [p] * a.layers, 'node_dropout': 0.1},
                      'train': {'negative_count': 1}},
            ra.LightGCN: {'model': {'embed_dim': d, 'n_layers': a.layers}, 'train': {'negative_count': 1}}}
    steps = []
    for cls, cfg in cfgs.items():
        model = on_device(cls)(cfg)
        model._init_model(data)
        model._init_parameter()
        model.to(dev)
        model.train()
        gb = torch.Generator(device=dev).manual_seed(5)
        pick = [torch.randint(0, a.inter, (a.batch,), device=dev, generator=gb).cpu() for _ in range(4)]
        batches = [{data.fuid: users[q].to(dev), data.fiid: items[q].to(dev), data.frating: torch.ones(a.batch, device=dev)} for q in pick]
        turn = {'k': 0}

        def step(model=model, batches=batches, turn=turn):
            turn['k'] += 1
            for t in model.parameters():
                t.grad = None
            model.training_step(batches[turn['k'] % len(batches)]).backward()
        steps.append(step)
    ms = timed(steps, a.reps, a.warmup)
    med = [statistics.median(t) for t in ms]
    res['training_step'] = dict(batch=a.batch, layers=a.layers, dim=d, ngcf=row(ms[0]), lightgcn=row(ms[1]), ngcf_over_lightgcn=med[0] / med[1])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')
    print(json.dumps(res))


if __name__ == '__main__':
    main()
