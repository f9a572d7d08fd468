#!/usr/bin/env python3
"""Every output of the tile kernels' and the sorted row update's entry points on seeded inputs, as .npy files: two builds of
the library compute the same bits exactly when the two directories compare equal.

    RSA_LIB=/path/to/old/librecstudio_amd.so python tools/kernel_outputs.py OUT_A      # needs the GPU; one fresh process
    RSA_LIB=/path/to/new/librecstudio_amd.so python tools/kernel_outputs.py OUT_B      # per library
    python tools/kernel_outputs.py --compare OUT_A OUT_B                               # CPU only

Cases: the fused forward with the BPR epilogue (every lane-group width, a last workgroup with idle waves, the three
samplers, with and without the query gradient, one tile and 2 / 5 tiles per query), the SampledSoftmax epilogue, the
in-place SGD step (rows nearly all shared / nearly all solo), the streaming instantiations (a table beyond 512 MiB), the
sorted row update under its three rules (accumulate, lazy Adam at step 7, Adagrad with lr_decay at step 7, the last two from
a nonzero state) called directly in its sorted and presorted forms at d = 64 / 128 / 256 -- 16-element chunks: 601 x 33
elements on 3 rows (every row through the finish kernel) and 777 x 65 on 3001 with mixed duplication; 64-element chunks: 4033
x 65 on 40 rows and on 300 007 with all rows distinct; with and without positives, query_index and upstream, padding row 0
and an interior one, dropped ids, and the apply pass after a sort that flagged the solo elements --, one FusedBPRAdam /
FusedBPRAdagrad step on 1000 and 200 000 items, the streaming form of both rules, and at
world size 1 with the deterministic router: the BPR and SampledSoftmax steps on the owners (gradient block and in place),
and their score-at-home forms (segment scoring, the home kernels, backward_segments), query-grouped (n = 64) and through
the sort by query (n = 50).  ``--compare`` demands np.array_equal on every file (NaN == NaN: a padded positive's
SampledSoftmax row is NaN by contract); there is no tolerance.
"""
import os
import socket
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))


def compare(a, b):
    fa, fb = sorted(os.listdir(a)), sorted(os.listdir(b))
    if fa != fb:
        print('different sets of files:', sorted(set(fa) ^ set(fb))[:10])
        return 1
    bad = 0
    for f in fa:
        x, y = np.load(os.path.join(a, f)), np.load(os.path.join(b, f))
        same = x.shape == y.shape and x.dtype == y.dtype and np.array_equal(x, y, equal_nan=x.dtype.kind == 'f')
        if not same:
            bad += 1
            where = np.flatnonzero(~((x == y) | ((x != x) & (y != y))).reshape(-1))[:3] if x.shape == y.shape else []
            print(f'DIFFERS {f}: first at {list(where)}')
    print(f'{len(fa)} files, {bad} differing')
    return 1 if bad else 0


def main(outdir):
    import torch
    import torch.distributed as dist
    import recstudio_amd as ra
    from recstudio_amd import _native as nat, fused, ops
    from recstudio_amd.shard import RowShardPlan, ShardedItemTable, ShardedRetriever
    os.makedirs(outdir, exist_ok=True)
    dev = torch.device('cuda', 0)
    count = [0]

    def save(case, **arrays):
        for k, v in arrays.items():
            if v is None:
                continue
            v = v.detach() if torch.is_tensor(v) else torch.as_tensor(v)
            np.save(os.path.join(outdir, f'{case}.{k}.npy'), v.cpu().numpy())
            count[0] += 1

    def save_dict(case, out):
        save(case, **{k: v for k, v in out.items() if torch.is_tensor(v)})

    def inputs(N, d, B, U=300, seed=0):
        g = torch.Generator().manual_seed(seed + d + B)
        item = torch.randn(N, d, generator=g) * 0.2
        item[0] = 0
        user = torch.randn(U, d, generator=g) * 0.2
        uid = torch.randint(1, U, (B,), generator=g)
        pos = torch.randint(1, N, (B,), generator=g)
        pos[B // 2] = 0                                               # a padded positive
        counts = (torch.rand(N, generator=g) ** 3 * 50).long() + 1
        return item.to(dev), user.to(dev), uid.to(dev), pos.to(dev), counts, g

    def sampler_kw(kind, N, B, n, counts, g):
        if kind == 'uniform':
            return nat.SAMPLER_UNIFORM, {}
        if kind == 'popular':
            return nat.SAMPLER_POPULAR, ra.PopularSamplerModel(counts).to(dev).lookup_kwargs()
        return nat.SAMPLER_GIVEN, {'neg_ids': torch.randint(1, N, (B, n), generator=g).to(dev)}

    # ---- the fused forward: BPR epilogue, one tile per query (n = 64) and the walk (n = 128, 320)
    N = 20_011
    for d in (32, 64, 128, 256):
        for kind in ('uniform', 'popular', 'given'):
            item, user, uid, pos, counts, g = inputs(N, d, 37)
            sk, kw = sampler_kw(kind, N, 37, 64, counts, g)
            torch.manual_seed(11)
            out = ops.fused_forward(item, user, 64, query_index=uid, pos_ids=pos, sampler=sk, fused_bpr=True,
                                    want_query_grad=True, **kw)
            save_dict(f'fwd_bpr_qg_d{d}_{kind}', out)
    for n in (128, 320):
        for qg in (False, True):
            for kind in ('uniform', 'popular', 'given'):
                item, user, uid, pos, counts, g = inputs(N, 128, 37)
                sk, kw = sampler_kw(kind, N, 37, n, counts, g)
                torch.manual_seed(12)
                out = ops.fused_forward(item, user, n, query_index=uid, pos_ids=pos, sampler=sk, fused_bpr=True,
                                        want_query_grad=qg, **kw)
                save_dict(f'fwd_bpr_n{n}_qg{int(qg)}_{kind}', out)
    # ---- the SampledSoftmax epilogue, with log-probabilities (popularity: drawn; given ids: inputs)
    for d in (32, 64, 128, 256):
        for n in (64, 192):
            for qg in (False, True):
                for kind in ('uniform', 'popular', 'given'):
                    item, user, uid, pos, counts, g = inputs(N, d, 37)
                    sk, kw = sampler_kw(kind, N, 37, n, counts, g)
                    if kind == 'given':
                        kw['pos_logp'] = (torch.rand(37, generator=g) - 2).to(dev)
                        kw['neg_logp'] = (torch.rand(37, n, generator=g) - 2).to(dev)
                    torch.manual_seed(13)
                    out = ops.fused_forward(item, user, n, query_index=uid, pos_ids=pos, sampler=sk, fused_loss='ssm',
                                            want_query_grad=qg, **kw)
                    save_dict(f'fwd_ssm_d{d}_n{n}_qg{int(qg)}_{kind}', out)
    # ---- the in-place SGD step: rows nearly all shared (N = 1000) / nearly all solo (N = 200 000)
    for d in (64, 128, 256):
        for N2 in (1_000, 200_000):
            item, user, uid, pos, counts, g = inputs(N2, d, 300)
            pos = pos.clamp(min=1)
            torch.manual_seed(14)
            step = fused.BPRSGDStep(item, user, 64, 0.05, ra.UniformSampler(N2), 'u', 'i', False)
            loss = step({'u': uid, 'i': pos})
            rows = torch.unique(torch.cat([pos, torch.arange(0, N2, 97, device=dev)]))      # every positive's row + a sample
            save(f'sgd_d{d}_N{N2}', loss=loss, user=user, rows=item[rows], checksum=item.double().sum(0))
    # ---- the streaming instantiations: a table of more than 512 MiB
    N3, d = 1_100_000, 128
    g = torch.Generator().manual_seed(3)
    item = torch.empty(N3, d, device=dev).normal_(0, 0.2, generator=torch.Generator(device=dev).manual_seed(3))
    item[0] = 0
    user = (torch.randn(300, d, generator=g) * 0.2).to(dev)
    uid, pos = torch.randint(1, 300, (300,), generator=g).to(dev), torch.randint(1, N3, (300,), generator=g).to(dev)
    torch.manual_seed(15)
    save_dict('stream_fwd_bpr_qg', ops.fused_forward(item, user, 64, query_index=uid, pos_ids=pos, sampler=nat.SAMPLER_UNIFORM,
                                                     fused_bpr=True, want_query_grad=True))
    torch.manual_seed(15)
    save_dict('stream_fwd_ssm_qg', ops.fused_forward(item, user, 192, query_index=uid, pos_ids=pos, sampler=nat.SAMPLER_UNIFORM,
                                                     fused_loss='ssm', want_query_grad=True))
    torch.manual_seed(15)
    save_dict('stream_fwd_walk_qg', ops.fused_forward(item, user, 128, query_index=uid, pos_ids=pos, sampler=nat.SAMPLER_UNIFORM,
                                                      fused_bpr=True, want_query_grad=True))
    torch.manual_seed(16)
    step = fused.BPRSGDStep(item, user, 64, 0.05, ra.UniformSampler(N3), 'u', 'i', False)
    loss = step({'u': uid, 'i': pos})
    rows = torch.unique(torch.cat([pos, torch.arange(0, N3, 997, device=dev)]))
    save('stream_sgd', loss=loss, user=user, rows=item[rows], checksum=item.double().sum(0))

    # ---- the sorted row update (accumulate, lazy Adam, Adagrad): direct calls, sorted and presorted forms, whole steps
    def tables(rule, N, d, seed, weight=None):
        """weight (drawn here unless given) and the rule's state tables, nonzero"""
        gd = torch.Generator(device=dev).manual_seed(seed)
        t = [torch.empty(N, d, device=dev).normal_(0, 0.3, generator=gd) if weight is None else weight]
        if rule == 'adam':
            t += [torch.empty(N, d, device=dev).normal_(0, 0.1, generator=gd),
                  torch.empty(N, d, device=dev).uniform_(1e-4, 1e-2, generator=gd)]
        elif rule == 'adagrad':
            t.append(torch.empty(N, d, device=dev).uniform_(0.5, 1.5, generator=gd))
        return t

    RULES = {'acc': (ops.scatter_rows_sorted, ops.scatter_rows_presorted, {}),
             'adam': (ops.adam_rows_sorted, ops.adam_rows_presorted, dict(lr=0.05, betas=(0.9, 0.999), eps=1e-8, step=7)),
             'adagrad': (ops.adagrad_rows_sorted, ops.adagrad_rows_presorted, dict(lr=0.5, lr_decay=0.01, eps=1e-10, step=7))}

    def save_tables(case, t, rows):
        """the touched rows of every table (an even sample of 1024 where there are more) and a float64 column sum of all of it"""
        rows = rows[::max(1, rows.numel() // 1024)]
        save(case, **{f'rows{j}': x[rows] for j, x in enumerate(t)}, **{f'checksum{j}': x.double().sum(0) for j, x in enumerate(t)})

    def rows_case(name, d, M, w, N, layout, pos, qi, up, pad, drop, seed):
        g = torch.Generator().manual_seed(seed + d)
        total = M * w
        if layout == 'distinct':
            ids = torch.randperm(N, generator=g)[:total]
        elif layout == 'few':
            ids = torch.randint(0, N, (total,), generator=g)
        else:                                                         # mixed: a third of the elements on five rows
            ids = torch.randint(0, N, (total,), generator=g)
            hot = torch.rand(total, generator=g) < 0.33
            ids[hot] = torch.randint(0, 5, (total,), generator=g)[hot] * 19 + 17
        if drop:
            ids[torch.rand(total, generator=g) < 0.05] = -1           # sorted behind every row (key == n_rows), never applied
        ids = ids.view(M, w)
        coef = torch.randn(M, w, generator=g)
        p, neg = (ids[:, 0].contiguous().to(dev), ids[:, 1:].contiguous().to(dev)) if pos else (None, ids.to(dev))
        dpos, dneg = (coef[:, 0].contiguous().to(dev), coef[:, 1:].contiguous().to(dev)) if pos else (None, coef.to(dev))
        query = torch.randn(257 if qi else M, d, generator=g).to(dev)
        index = torch.randint(0, 257, (M,), generator=g).to(dev) if qi else None
        upstream = None if up is None else torch.tensor([up], device=dev)
        rows = torch.unique(ids[ids >= 0]).to(dev)
        for rule, (sorted_, presorted, hp) in RULES.items():
            t = tables(rule, N, d, seed)
            sorted_(*t, query, neg, dneg, query_index=index, pos_ids=p, dpos=dpos, upstream=upstream, pad_row=pad, **hp)
            save_tables(f'rows_{name}_d{d}_{rule}_sorted', t, rows)
            t = tables(rule, N, d, seed)
            _, ws = ops.sort_step_elements(p, neg, N, pad_row=pad, want_solo=False)
            presorted(*t, query, ws, M, neg.shape[1], dneg, query_index=index, dpos=dpos, upstream=upstream, pad_row=pad, **hp)
            save_tables(f'rows_{name}_d{d}_{rule}_presorted', t, rows)
        if layout == 'mixed':                                         # the solo-skip path: flagged elements are left alone
            t = tables('acc', N, d, seed)
            solo, ws = ops.sort_step_elements(p, neg, N, pad_row=pad, want_solo=True)
            ops.scatter_rows_presorted(*t, query, ws, M, neg.shape[1], dneg, query_index=index, dpos=dpos, upstream=upstream, pad_row=pad)
            save(f'rows_{name}_d{d}_solo', solo=solo)
            save_tables(f'rows_{name}_d{d}_solo', t, rows)

    for d in (64, 128, 256):
        # chunks of 16 elements: every row through the finish kernel; mixed duplication (interior padding row, row 0)
        rows_case('finish3', d, 601, 33, 3, 'few', pos=True, qi=False, up=0.37, pad=1, drop=False, seed=21)
        rows_case('mixed', d, 777, 65, 3001, 'mixed', pos=True, qi=True, up=0.37, pad=17, drop=True, seed=22)
        rows_case('mixed_nopos', d, 777, 65, 3001, 'mixed', pos=False, qi=True, up=None, pad=0, drop=True, seed=23)
        # chunks of 64 elements (more than 2^18 of them): 40 rows, all rows distinct
        rows_case('finish40', d, 4033, 65, 40, 'few', pos=True, qi=True, up=None, pad=0, drop=True, seed=24)
        rows_case('distinct', d, 4033, 65, 300_007, 'distinct', pos=False, qi=False, up=-0.73, pad=0, drop=False, seed=25)
        for N2 in (1_000, 200_000):
            for oname, opt in (('adam', fused.FusedBPRAdam), ('adagrad', fused.FusedBPRAdagrad)):
                it, us, uid2, pos2, counts, g = inputs(N2, d, 300)
                torch.manual_seed(17)
                o = opt(it, us)
                loss, neg = o.step(64, user_ids=uid2, pos_ids=pos2.clamp(min=1), sampler=ra.UniformSampler(N2))
                rows = torch.unique(torch.cat([pos2, neg.reshape(-1)[::7]]))
                save(f'step_{oname}_d{d}_N{N2}', loss=loss, neg=neg, rows=it[rows], checksum=it.double().sum(0), user=us,
                     **{k: v[rows] for k, v in o.state.items() if k[0] == 'i'},
                     **{k + '_checksum': v.double().sum(0) for k, v in o.state.items()})
    # the streaming instantiations of the Adam and Adagrad forms, on the table above
    g = torch.Generator().manual_seed(18)
    neg = torch.randint(1, N3, (300, 64), generator=g).to(dev)
    dpos, dneg = torch.randn(300, generator=g).to(dev), torch.randn(300, 64, generator=g).to(dev)
    rows = torch.unique(torch.cat([pos, neg.reshape(-1)]))
    for rule in ('adam', 'adagrad'):
        t = tables(rule, N3, 128, 19, weight=item)
        RULES[rule][0](*t, user, neg, dneg, query_index=uid, pos_ids=pos, dpos=dpos, pad_row=0, **RULES[rule][2])
        save_tables(f'stream_rows_{rule}', t, rows)
        del t
    del item
    torch.cuda.empty_cache()

    # ---- world size 1, the deterministic router
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        os.environ['MASTER_PORT'] = str(s.getsockname()[1])
    dist.init_process_group('gloo', rank=0, world_size=1)
    try:
        N, U, B = 20_011, 300, 37
        for d in (64, 128, 256):
            for n in (64, 50):
                item0, user0, uid, pos, counts, g = inputs(N, d, B, U)
                pos = pos.clamp(min=1)
                for lname, loss_mod in (('bpr', ra.BPRLoss), ('ssm', ra.SampledSoftmaxLoss)):
                    for sname in ('uniform', 'popular'):
                        smp = ra.UniformSampler(N) if sname == 'uniform' else ra.PopularSamplerModel(counts).to(dev)
                        for home in (False, True):
                            for lr in (None, 0.3):
                                item = item0.clone()
                                tower = torch.nn.Embedding(U, d).to(dev)
                                with torch.no_grad():
                                    tower.weight.copy_(user0)
                                table = ShardedItemTable(item, RowShardPlan(N, 1), 0, dist, check_every=0, sample_seed=9,
                                                         deterministic=True, owner_loss=not home)
                                kw = {} if lr is None else {'item_sgd_lr': lr, 'query_sgd_lr': lr}
                                tr = ShardedRetriever(table, tower, smp, loss_mod(), n, sparse_query_rows=True, keep_neg_ids=True,
                                                      owner_ssm=not home, **kw)
                                loss = tr.training_step(uid, pos)
                                case = f'w1_{lname}_d{d}_n{n}_{sname}_{"home" if home else "own"}_{"grad" if lr is None else "sgd"}'
                                it = table.item_local
                                save(case, loss=loss, neg=tr.last_neg, rows=it[torch.unique(tr.last_neg)], checksum=it.double().sum(0),
                                     user=tower.weight,
                                     item_grad=tr.item_grad_local if lr is None else None,
                                     query_grad=tr.query_grad_dense() if lr is None else None)
    finally:
        dist.destroy_process_group()
    torch.cuda.synchronize()
    print(f'{count[0]} arrays written to {outdir} by {nat.LIB_PATH}')
    return 0


if __name__ == '__main__':
    if len(sys.argv) == 4 and sys.argv[1] == '--compare':
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1]))
