"""Times SimGCL's perturbed propagation layer (ops.spmm_csr(noise=...): the noise added in the epilogue of rsa_spmm_csr) on the graph
of tools/bench_lightgcn.py: next to a plain layer, next to the same layer written as a plain layer plus torch ops, and inside a
whole SimGCL training step next to LightGCN's and SGL's; and the peak memory of a perturbed propagation in both forms.  One process,
one device, the arms of a group alternating, device events around every call, warm-up calls first.  Prints one JSON object and
writes it to profiles/simgcl_bench.json.

    python tools/bench_simgcl.py [--users 1048576 --items 1048576 --inter 67108864 --dims 64,128 --batch 2048 --layers 3 --reps 10 --warmup 3]

Arms, per dim:
  (a) plain          ops.spmm_csr, one middle layer: y written, the running sum updated in place
      perturbed      the same launch with noise: rng.reserve for one rand_like, the draws, the row norm and the move in the epilogue
      torch_form     the plain layer with y only, then rand_like / F.normalize / sign / mul / add on y and the add into the running sum
      the yardstick for "the fusion paid" is perturbed < torch_form; perturbed / plain is what the noise costs on top of a layer
  (b) peak memory    SimGCLNet.propagate(perturbed=True) at --layers next to the same propagation in the torch form (no autograd):
                     bytes allocated above the inputs
  (c) training_step  (first dim only) SimGCL.training_step + backward at --batch, --layers, next to LightGCN's and SGL's ('ED')
Recorded: median / min / max in ms and the ratios; the largest difference between the two forms of the layer on the same uniforms."""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from graph_bench import peak_above, row, timed, zipf_graph      # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--users', type=int, default=1 << 20)
    ap.add_argument('--items', type=int, default=1 << 20)
    ap.add_argument('--inter', type=int, default=1 << 26)
    ap.add_argument('--dims', default='64,128')
    ap.add_argument('--batch', type=int, default=2048)
    ap.add_argument('--layers', type=int, default=3)
    ap.add_argument('--eps', type=float, default=0.1)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'simgcl_bench.json'))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_simgcl.py measures on the GPU: none found')
    import recstudio_amd as ra
    from recstudio_amd import graphmodule, ops, rng
    dev = torch.device('cuda')
    dims = [int(s) for s in a.dims.split(',')]
    nu, ni = a.users + 1, a.items + 1
    n = nu + ni
    adj, users, items = zipf_graph(a.users, a.items, a.inter, dev)
    torch.cuda.empty_cache()
    deg = adj.indptr[1:] - adj.indptr[:-1]
    res = dict(device=torch.cuda.get_device_name(0), users=a.users, items=a.items, interactions=a.inter, rows=n, nnz=adj.nnz,
               degree_max=int(deg.max()), chunk=adj.plan.chunk, split_rows=adj.plan.n_split, eps=a.eps, reps=a.reps, warmup=a.warmup, layer={},
               propagation_peak_bytes={})
    print(f'graph built: {n} rows, {adj.nnz} non-zeros', file=sys.stderr, flush=True)
    csr = (adj.indptr, adj.indices, adj.values)
    eps = a.eps

    for d in dims:
        g = torch.Generator(device=dev).manual_seed(3)
        x = torch.empty(n, d, device=dev).normal_(0, 0.1, generator=g)
        y, acc = torch.empty_like(x), torch.zeros_like(x)

        def plain():
            ops.spmm_csr(*csr, x, plan=adj.plan, y=y, acc=acc)

        def perturbed():
            ops.spmm_csr(*csr, x, plan=adj.plan, y=y, acc=acc, noise=rng.reserve(x.numel(), 4, dev), noise_eps=eps)

        def torch_form():
            ops.spmm_csr(*csr, x, plan=adj.plan, y=y)
            moved = y + torch.sign(y) * F.normalize(torch.rand_like(y), dim=-1) * eps
            acc.add_(moved)
            return moved

        ms = timed([plain, perturbed, torch_form], a.reps, a.warmup)
        torch.manual_seed(11)
        perturbed()
        mine = y.clone()
        torch.manual_seed(11)
        theirs = torch_form()
        worst = float((mine - theirs).abs().max())
        del mine, theirs
        med = [statistics.median(t) for t in ms]
        res['layer'][str(d)] = dict(plain=row(ms[0]), perturbed=row(ms[1]), torch_form=row(ms[2]), perturbed_over_plain=med[1] / med[0],
                                    torch_form_over_perturbed=med[2] / med[1], noise_ms=med[1] - med[0], torch_epilogue_ms=med[2] - med[0],
                                    max_abs_difference_to_torch_form=worst)
        print(d, json.dumps(res['layer'][str(d)]), file=sys.stderr, flush=True)
        del y, acc
        torch.cuda.empty_cache()

        # (b)
        net = graphmodule.SimGCLNet(a.layers, eps)

        def torch_propagate():
            e, outs = x, []
            for _ in range(a.layers):
                e = ops.spmm_csr(*csr, e, plan=adj.plan)
                e = e + torch.sign(e) * F.normalize(torch.rand_like(e), dim=-1) * eps
                outs.append(e)
            return torch.stack(outs, dim=-2).mean(dim=-2)

        with torch.no_grad():
            net.propagate(adj, x, perturbed=True)                                     # (the partials workspace exists before the clock)
            fused, torch_ops = peak_above(lambda: net.propagate(adj, x, perturbed=True)), peak_above(torch_propagate)
        res['propagation_peak_bytes'][str(d)] = dict(layers=a.layers, table_bytes=x.numel() * 4, fused=fused, torch_form=torch_ops,
                                                     saved=torch_ops - fused)
        print(d, json.dumps(res['propagation_peak_bytes'][str(d)]), file=sys.stderr, flush=True)
        del x
        torch.cuda.empty_cache()

    # (c)
    def on_device(cls):
        class OnDevice(cls):
            def _get_graph(self, train_data):
                return adj
        return OnDevice

    d = dims[0]
    data = ra.TripletDataset.from_mapped_ids(users, items, n_users=nu, n_items=ni)
    cfg = {'model': {'embed_dim': d, 'n_layers': a.layers}, 'train': {'negative_count': 1}}
    steps = []
    for cls in (ra.SimGCL, ra.LightGCN, ra.SGL):
        m = on_device(cls)(cfg)
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
    med = [statistics.median(t) for t in ms]
    res['training_step'] = dict(batch=a.batch, layers=a.layers, dim=d, simgcl=row(ms[0]), lightgcn=row(ms[1]), sgl=row(ms[2]),
                                simgcl_over_lightgcn=med[0] / med[1], simgcl_over_sgl=med[0] / med[2])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')
    print(json.dumps(res))


if __name__ == '__main__':
    main()
