"""GPU: the Adagrad row update (rsa_rows_update_sorted / rsa_rows_update_presorted with rule = RSA_ROWS_ADAGRAD: apply_run_adagrad,
sorted_apply_adagrad_kernel, sorted_finish_adagrad_kernel, adagrad_of) against a float64 referee on weight AND state_sum, at the
bound derived in tests/adagrad_referee.py (no element of any case may exceed it), the untouched-rows / reproducibility / error
contracts around it, FusedBPRAdagrad, and ``fit`` with ``train.fused_optimizer: 'learner'``.  The referee is pinned to
torch.optim.Adagrad (both gradient branches) by tests/test_adagrad_referee.py."""
import ctypes

import numpy as np
import pytest
import torch

import adagrad_referee as gr
import adam_referee as ar
from test_gpu_adam_rows import DEV, LAYOUTS, SMALL_TOTAL

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ra():
    import recstudio_amd
    recstudio_amd._native.lib()
    return recstudio_amd


def make_case(c):
    """Inputs of one direct call from the case description (see _cases) -> (call kwargs, hyper-parameters, start tables)."""
    d, M, w, N = c['d'], c['M'], c['w'], c['N']
    g = torch.Generator(device=DEV).manual_seed(c['seed'])
    total = M * w
    ids = LAYOUTS[c['layout']](g, total, N)
    if c.get('drop'):
        ids[torch.rand(total, device=DEV, generator=g) < 0.05] = -1
    ids = ids.view(M, w)
    has_pos = c['pos']
    pos, neg = (ids[:, 0].contiguous(), ids[:, 1:].contiguous()) if has_pos else (None, ids)
    coef = torch.randn(M, w, device=DEV, generator=g)
    dpos, dneg = (coef[:, 0].contiguous(), coef[:, 1:].contiguous()) if has_pos else (None, coef)
    if c['qi']:
        query = torch.randn(c.get('U', 257), d, device=DEV, generator=g)
        qi = torch.randint(0, query.shape[0], (M,), device=DEV, generator=g)
    else:
        query, qi = torch.randn(M, d, device=DEV, generator=g), None
    up = torch.tensor([c['up']], device=DEV) if c.get('up') is not None else None
    kw = dict(query=query, neg_ids=neg, dneg=dneg, query_index=qi, pos_ids=pos, dpos=dpos, upstream=up, pad_row=c['pad'])
    hp = dict(lr=c.get('lr', 0.5), lr_decay=c.get('lr_decay', 0.0), eps=c.get('eps', 1e-10), step=c['step'])
    return kw, hp, conditioned_tables(g, N, d, kw, zero_state=c['zero'])


def conditioned_tables(g, N, d, kw, zero_state):
    """Weights of order 0.3; a prior state that makes the weights a real test: state_sum in [0.5, 1.5] x the row's mean g^2 (rows the
    step does not touch: of order 1, so that they are checked on live values).  A zero state at step 1 gives g / sqrt(g^2) =
    sign(g): any error in g cancels in the weights -- those cases are there for the state."""
    w = torch.randn(N, d, device=DEV, generator=g) * 0.3
    if zero_state:
        return w, torch.zeros(N, d, device=DEV)
    grad = ar.row_gradients(kw['query'], kw['neg_ids'], kw['dneg'], query_index=kw['query_index'], pos_ids=kw['pos_ids'],
                            dpos=kw['dpos'], upstream=kw['upstream'], pad_row=-1)
    scale = torch.ones(N, 1, device=DEV)
    scale[grad['rows']] = grad['g'].pow(2).mean(1, keepdim=True).clamp_min(1e-20).float()
    return w, (0.5 + torch.rand(N, d, device=DEV, generator=g)) * scale


def run_sorted(ra, tables, kw, hp):
    w, s = (t.clone() for t in tables)
    ra.ops.adagrad_rows_sorted(w, s, kw['query'], kw['neg_ids'], kw['dneg'], query_index=kw['query_index'], pos_ids=kw['pos_ids'],
                               dpos=kw['dpos'], upstream=kw['upstream'], pad_row=kw['pad_row'], **hp)
    return w, s


def run_presorted(ra, tables, kw, hp):
    w, s = (t.clone() for t in tables)
    M, n = kw['neg_ids'].shape
    _, ws = ra.ops.sort_step_elements(kw['pos_ids'], kw['neg_ids'], w.shape[0], pad_row=kw['pad_row'], want_solo=False)
    ra.ops.adagrad_rows_presorted(w, s, kw['query'], ws, M, n, kw['dneg'], query_index=kw['query_index'], dpos=kw['dpos'],
                                  upstream=kw['upstream'], pad_row=kw['pad_row'], **hp)
    return w, s


def check_against_referee(got, tables, kw, hp, rows=None, label=''):
    """Every element of every touched row of both tables within the derived bound (the share of elements allowed outside it is
    0); -> the referee (for its row set) and the two max ratios."""
    ref = gr.referee(*tables, kw['query'], kw['neg_ids'], kw['dneg'], query_index=kw['query_index'], pos_ids=kw['pos_ids'],
                     dpos=kw['dpos'], upstream=kw['upstream'], pad_row=kw['pad_row'], rows=rows, **hp)
    r = ref['rows']
    ratios = gr.bound_ratios(ref, got[0][r], got[1][r])
    print(f'{label}: rows {r.numel()}, K max {int(ref["K"].max()) if r.numel() else 0}, error / bound: weight {ratios[0]:.3f} '
          f'state_sum {ratios[1]:.3f}')
    assert max(ratios) <= 1.0, (label, ratios)
    return ref, ratios


# ------------------------------------------------------------------------------------------------------------------ the direct calls
# total = M * w elements (w = num_neg + 1 with positives).  Chunk regime '16': total <= 2^18, '64': total > 2^18.
#   2^18 - 1 = 4161 * 63, 2^18 = 4096 * 64, 2^18 + 1 = 4033 * 65
def _cases():
    out = []
    for d in (64, 128, 256):
        for ce in (16, 64):
            big = ce == 64
            s = d * 10 + ce

            def add(name, **c):
                c.update(d=d, ce=ce, seed=s * 100 + len(out) + 7)
                out.append(pytest.param(c, id=f'd{d}-chunk{ce}-{name}'))
            # (a) all rows distinct; the exact SORTED_SMALL_TOTAL edges
            if big:
                add('distinct-total2^18+1-zero-step1', layout='distinct', M=4033, w=65, N=300_007, pos=True, qi=True, up=None, pad=-1,
                    step=1, zero=True)
                add('distinct-total2^18+1-nopos-up-decay-step1000', layout='distinct', M=4033, w=65, N=300_007, pos=False, qi=True,
                    up=-0.73, pad=0, step=1000, zero=False, lr_decay=0.01)
            else:
                add('distinct-total2^18-1-zero-step1', layout='distinct', M=4161, w=63, N=300_007, pos=False, qi=True, up=None, pad=-1,
                    step=1, zero=True)
                add('distinct-total2^18-nopos-noqi-up-decay-step1000', layout='distinct', M=4096, w=64, N=300_007, pos=False, qi=False,
                    up=-0.73, pad=0, step=1000, zero=False, lr_decay=0.01)
                add('small-total37', layout='few', M=37, w=1, N=11, pos=False, qi=True, up=None, pad=-1, step=2, zero=False, drop=True,
                    lr_decay=0.5)
            # (b) 1, 2, 3, 40 rows with thousands of elements each: every row goes through sorted_finish_adagrad_kernel
            M, w = (4033, 65) if big else (601, 33)
            add('rows1-pos-qi-up-step1000', layout='few', M=M, w=w, N=1, pos=True, qi=True, up=0.37, pad=-1, step=1000, zero=False,
                lr_decay=0.001)
            add('rows2-pad0-eps1e-2-step2', layout='few', M=M, w=w, N=2, pos=False, qi=True, up=None, pad=0, step=2, zero=False,
                eps=1e-2, drop=True)
            add('rows3-padinterior-noqi-step1', layout='few', M=M, w=w, N=3, pos=True, qi=False, up=0.37, pad=1, step=1, zero=False)
            add('rows40-pad0-drop-zero-step1', layout='few', M=M, w=w, N=40, pos=True, qi=True, up=None, pad=0, step=1, zero=True, drop=True)
            # (c) runs that start and end exactly on chunk borders
            M, w = (4100, 65) if big else (1531, 33)
            add('aligned-pad0-decay-step2', layout='aligned', M=M, w=w, N=200_003, pos=True, qi=True, up=None, pad=0, step=2, zero=False,
                lr_decay=0.25)
            add('aligned-nopad-noqi-up-zero-step1', layout='aligned', M=M, w=w - 1, N=200_003, pos=False, qi=False, up=-2.5, pad=-1,
                step=1, zero=True)
            # (d) mixed duplication, an interior padding row with many elements, dropped ids
            M, w = (4201, 65) if big else (777, 65)
            add('mixed-padinterior-drop-up-decay-step1000', layout='mixed', M=M, w=w, N=3001, pos=True, qi=True, up=0.37, pad=17, step=1000,
                zero=False, drop=True, lr_decay=0.01)
            add('mixed-pad0-lr1e-2-step1', layout='mixed', M=M, w=w - 1, N=3001, pos=False, qi=True, up=None, pad=0, step=1,
                zero=False, lr=1e-2, drop=True)
    return out


@pytest.mark.parametrize('c', _cases())
def test_adagrad_rows_sorted_and_presorted_vs_float64_referee(ra, c):
    """ops.adagrad_rows_sorted called directly: weight and state_sum of every touched row within the derived bound of the float64
    referee; rows without a kept element (padding row, rows only dropped ids name, everything else) bit-unchanged in both tables; a
    second call from the same start state and the sort_step_elements(want_solo=False) + adagrad_rows_presorted form equal the first
    bit for bit."""
    kw, hp, tables = make_case(c)
    total = c['M'] * c['w']
    assert (total > SMALL_TOTAL) == (c['ce'] == 64)          # the case runs in the chunk regime its id names
    got = run_sorted(ra, tables, kw, hp)
    again = run_sorted(ra, tables, kw, hp)
    pre = run_presorted(ra, tables, kw, hp)
    torch.cuda.synchronize()
    for a, b, p in zip(got, again, pre):
        assert torch.equal(a, b) and torch.equal(a, p)
    ref, _ = check_against_referee(got, tables, kw, hp, label=str(c['layout']))
    assert gr.untouched_equal(ref, tables, got)
    assert ref['rows'].numel() > 0
    assert not torch.equal(got[0][ref['rows']], tables[0][ref['rows']]) and not torch.equal(got[1][ref['rows']], tables[1][ref['rows']])
    if c['pad'] >= 0:
        assert not bool((ref['rows'] == c['pad']).any())
        if c['layout'] != 'distinct':
            ids = torch.cat([kw['neg_ids'].reshape(-1)] + ([kw['pos_ids']] if kw['pos_ids'] is not None else []))
            assert int((ids == c['pad']).sum()) > (0 if c['N'] > 1000 else 30)          # the padding row really has elements
    if c['layout'] == 'few' and c['N'] <= 40 and total > 1000:
        assert int(ref['K'].min()) > 16 * 8          # every row spans many chunks: all of them through the finish kernel


@pytest.mark.parametrize('d', [64, 128, 256])
@pytest.mark.parametrize('M,U', [(5000, 1201), (270_001, 50_021)])
@pytest.mark.parametrize('zero,step', [(False, 7), (True, 1)])
def test_adagrad_user_side_form(ra, d, M, U, zero, step):
    """The call FusedBPRAdagrad makes for the user table: neg_ids = user_ids.view(M, 1), coefficients of ones, query = the block of
    per-query gradients, no query_index, duplicate users in the batch; 16-element chunks (M <= 2^18) and 64-element chunks."""
    g = torch.Generator(device=DEV).manual_seed(d + M)
    uid = torch.randint(1, U, (M,), device=DEV, generator=g)
    uid[:64] = uid[64:128]
    qgrad = torch.randn(M, d, device=DEV, generator=g) * 1e-3
    kw = dict(query=qgrad, neg_ids=uid.view(M, 1), dneg=torch.ones(M, 1, device=DEV), query_index=None, pos_ids=None, dpos=None,
              upstream=None, pad_row=0)
    hp = dict(lr=0.5, lr_decay=0.1, eps=1e-10, step=step)
    tables = conditioned_tables(g, U, d, kw, zero_state=zero)
    got, again, pre = run_sorted(ra, tables, kw, hp), run_sorted(ra, tables, kw, hp), run_presorted(ra, tables, kw, hp)
    for a, b, p in zip(got, again, pre):
        assert torch.equal(a, b) and torch.equal(a, p)
    ref, _ = check_against_referee(got, tables, kw, hp, label=f'user side d={d} M={M}')
    assert gr.untouched_equal(ref, tables, got)
    assert int(ref['K'].max()) > 1 and torch.equal(got[0][0], tables[0][0])


def _hot_ids(g, total, lo, hi, n_hot=10, share=0.15):
    ids = torch.randint(lo, hi, (total,), device=DEV, generator=g)
    hot = torch.randint(lo, hi, (n_hot,), device=DEV, generator=g)
    sel = torch.rand(total, device=DEV, generator=g) < share
    ids[sel] = hot[torch.randint(0, n_hot, (int(sel.sum()),), device=DEV, generator=g)]
    ids[torch.rand(total, device=DEV, generator=g) < 0.05] = -1
    return ids


def test_adagrad_streaming_form_table_over_512_mb(ra):
    """A table over 512 MB (N = 1 100 000, d = 128: 563 MB) takes the streaming (nontemporal) form of sorted_apply_adagrad_kernel for
    the weight AND state_sum, while sorted_finish_adagrad_kernel reads and writes the same tables with plain accesses: total >
    2^18, most rows with one or two elements, ten hot rows with runs of thousands (finish kernel).  Referee on the touched rows;
    every other row of both tables bit-unchanged."""
    N, d, M, w = 1_100_000, 128, 5000, 65
    assert N * d * 4 > (512 << 20)
    g = torch.Generator(device=DEV).manual_seed(77)
    ids = _hot_ids(g, M * w, 1, N).view(M, w)
    coef = torch.randn(M, w, device=DEV, generator=g)
    query = torch.randn(999, d, device=DEV, generator=g)
    qi = torch.randint(0, 999, (M,), device=DEV, generator=g)
    kw = dict(query=query, neg_ids=ids[:, 1:].contiguous(), dneg=coef[:, 1:].contiguous(), query_index=qi, pos_ids=ids[:, 0].contiguous(),
              dpos=coef[:, 0].contiguous(), upstream=torch.tensor([0.61], device=DEV), pad_row=0)
    hp = dict(lr=0.5, lr_decay=0.05, eps=1e-10, step=3)
    tables = conditioned_tables(g, N, d, kw, zero_state=False)
    got = run_sorted(ra, tables, kw, hp)
    pre = run_presorted(ra, tables, kw, hp)
    for a, p in zip(got, pre):
        assert torch.equal(a, p)
    ref, _ = check_against_referee(got, tables, kw, hp, label='streaming')
    assert int(ref['K'].max()) > 3000 and ref['rows'].numel() > 150_000
    assert gr.untouched_equal(ref, tables, got)


def test_adagrad_rows_past_byte_offset_4_gib(ra):
    """N = 9 000 001, d = 128: every touched row lies past byte offset 4 GiB (row 8 388 608) in the weight table AND in state_sum --
    a row offset computed in 32 bits would land in the lower part.  The lower part of both tables holds a constant and must still
    hold it; the upper part is compared row for row (referee on the touched rows, everything else bit-unchanged)."""
    N, d, M, w = 9_000_001, 128, 3001, 65
    first = (4 << 30) // (d * 4)
    assert first == 8_388_608 and first < N
    g = torch.Generator(device=DEV).manual_seed(41)
    ids = _hot_ids(g, M * w, first + 1, N, n_hot=4, share=0.05).view(M, w)
    ids[0, 1], ids[0, 2] = N - 1, first + 1                     # the last row and the first one wholly past the border
    coef = torch.randn(M, w, device=DEV, generator=g)
    query = torch.randn(999, d, device=DEV, generator=g)
    qi = torch.randint(0, 999, (M,), device=DEV, generator=g)
    kw = dict(query=query, neg_ids=ids[:, 1:].contiguous(), dneg=coef[:, 1:].contiguous(), query_index=qi, pos_ids=ids[:, 0].contiguous(),
              dpos=coef[:, 0].contiguous(), upstream=None, pad_row=0)
    hp = dict(lr=0.5, lr_decay=0.0, eps=1e-10, step=2)
    wt, st = torch.empty(N, d, device=DEV), torch.empty(N, d, device=DEV)
    wt[:first], st[:first] = 0.25, 0.5
    wt[first:].normal_(0, 0.3, generator=g)
    grad = ar.row_gradients(query, kw['neg_ids'], kw['dneg'], query_index=qi, pos_ids=kw['pos_ids'], dpos=kw['dpos'], pad_row=0)
    st[first:] = 1.0
    st[grad['rows']] = ((0.5 + torch.rand(grad['rows'].numel(), d, device=DEV, generator=g)).double()
                        * grad['g'].pow(2).mean(1, keepdim=True)).float()
    assert int(grad['rows'].min()) == first + 1 and int(grad['rows'].max()) == N - 1
    hi0 = (wt[first:].clone(), st[first:].clone())
    ra.ops.adagrad_rows_sorted(wt, st, query, kw['neg_ids'], kw['dneg'], query_index=qi, pos_ids=kw['pos_ids'], dpos=kw['dpos'],
                               pad_row=0, **hp)
    torch.cuda.synchronize()
    assert bool((wt[:first] == 0.25).all()) and bool((st[:first] == 0.5).all())
    # the referee and the untouched-rows check on the upper part, re-based to row 0
    shift = lambda t: None if t is None else torch.where(t >= 0, t - first, t)      # noqa: E731
    kw_hi = dict(kw, neg_ids=shift(kw['neg_ids']), pos_ids=shift(kw['pos_ids']), pad_row=-1)
    ref, _ = check_against_referee((wt[first:], st[first:]), hi0, kw_hi, hp, label='past 4 GiB')
    assert ref['rows'].numel() == grad['rows'].numel() > 100_000 and int(ref['K'].max()) > 1000
    assert gr.untouched_equal(ref, hi0, (wt[first:], st[first:]))


# ------------------------------------------------------------------------------------------------------------- FusedBPRAdagrad
def _torch_bpr_trajectory(dtype, iw0, uw0, batches, hp):
    """torch.optim.Adagrad on sparse embeddings, BPR loss (-mean logsigmoid(pos - neg)) by autograd on ITS OWN weights; CPU (its
    index_add is sequential: the run is reproducible)."""
    iw = torch.nn.Parameter(iw0.cpu().to(dtype).clone())
    uw = torch.nn.Parameter(uw0.cpu().to(dtype).clone())
    opt = torch.optim.Adagrad([iw, uw], **hp)
    F = torch.nn.functional
    for uid, pos, neg in batches:
        opt.zero_grad()
        q = F.embedding(uid.cpu(), uw, sparse=True)
        ps = (q * F.embedding(pos.cpu(), iw, sparse=True)).sum(-1)
        ns = (q.unsqueeze(1) * F.embedding(neg.cpu(), iw, sparse=True)).sum(-1)
        (-F.logsigmoid(ps.unsqueeze(1) - ns).mean()).backward()
        opt.step()
    return [iw.data, opt.state[iw]['sum'], uw.data, opt.state[uw]['sum']]


def test_adagrad_trajectory_of_20_steps_vs_float64_torch_adagrad(ra):
    """20 FusedBPRAdagrad.step calls (the setting of test_adam_trajectory_of_20_steps_vs_float64_sparse_adam: N = 6001, U = 701,
    d = 128, B = 512, n = 64, given negatives; items 1 .. 399 recur in every step, items of the upper half are touched in ONE step
    and then rest, users recur) against torch.optim.Adagrad on float64 CPU copies fed the float64 gradients of the same loss on its
    own weights.  Two trajectories drift apart, so no derived bound applies: the yardstick is that test's own -- the distance of
    the SAME torch run in fp32 from the float64 run, times 4, per table, in the maximum norm and in the rms.  Row 0 stays untouched."""
    N, U, d, B, n, steps = 6001, 701, 128, 512, 64, 20
    hp = dict(lr=0.05, lr_decay=0.01, initial_accumulator_value=1e-6, eps=1e-10)
    g = torch.Generator().manual_seed(21)
    iw0 = torch.randn(N, d, generator=g) * 0.3
    iw0[0] = 0
    uw0 = torch.randn(U, d, generator=g) * 0.3
    batches = []
    for k in range(steps):
        uid = torch.randint(1, U, (B,), generator=g)
        pos = torch.randint(1, 400, (B,), generator=g)
        neg = torch.randint(1, 400, (B, n), generator=g)
        lo = 3000 + k * 150                                          # this step's own slice of the upper half: touched once, then resting
        neg[:, ::16] = torch.randint(lo, lo + 150, (B, n // 16), generator=g)
        batches.append((uid, pos, neg))
    want = _torch_bpr_trajectory(torch.float64, iw0, uw0, batches, hp)
    t32 = _torch_bpr_trajectory(torch.float32, iw0, uw0, batches, hp)
    iw, uw = iw0.to(DEV), uw0.to(DEV)
    fa = ra.fused.FusedBPRAdagrad(iw, uw, **hp)
    for uid, pos, neg in batches:
        fa.step(n, user_ids=uid.to(DEV), pos_ids=pos.to(DEV), neg_ids=neg.to(DEV))
    torch.cuda.synchronize()
    assert fa.t == steps
    got = [iw, fa.state['is'], uw, fa.state['us']]
    acc0 = torch.tensor(hp['initial_accumulator_value'], dtype=torch.float32)
    assert not iw[0].any() and bool((fa.state['is'][0].cpu() == acc0).all()) and torch.equal(uw[0].cpu(), uw0[0])
    bad = []
    for name, a, b, w in zip(('item weight', 'item state_sum', 'user weight', 'user state_sum'), got, t32, want):
        ek, et = (a.cpu().double() - w).abs(), (b.double() - w).abs()
        print(f'{name}: max |kernel - f64| {float(ek.max()):.3e} |torch fp32 - f64| {float(et.max()):.3e}   rms {float(ek.pow(2).mean().sqrt()):.3e}'
              f' / {float(et.pow(2).mean().sqrt()):.3e}')
        if not (float(ek.max()) <= 4 * float(et.max()) and float(ek.pow(2).mean().sqrt()) <= 4 * float(et.pow(2).mean().sqrt())):
            bad.append(name)
    assert not bad, bad


@pytest.mark.parametrize('kind', ['uniform', 'popular'])
def test_prefetched_adagrad_steps_equal_the_plain_sequence(ra, kind):
    """FusedBPRAdagrad.prepare / step_prepared (sampling and the two sorts one batch ahead on a side stream, apply passes through
    rsa_rows_update_presorted) == the same sequence of FusedBPRAdagrad.step calls: losses, negatives, weights and both state_sum
    tables bit for bit."""
    N, U, d, B, n, steps = 50_021, 3001, 128, 4096, 64, 4
    g = torch.Generator().manual_seed(8)
    iw = torch.randn(N, d, generator=g) * 0.3
    iw[0] = 0
    uw = torch.randn(U, d, generator=g) * 0.3
    batches = [(torch.randint(1, U, (B,), generator=g).to(DEV), torch.randint(1, N, (B,), generator=g).to(DEV)) for _ in range(steps)]
    if kind == 'uniform':
        sampler = ra.UniformSampler(N)
    else:
        sampler = ra.PopularSamplerModel((torch.rand(N, generator=g) ** 6 * 1000).long()).to(DEV)
    hp = dict(lr=0.05, lr_decay=0.1)
    item0, user0 = iw.to(DEV).clone(), uw.to(DEV).clone()
    torch.manual_seed(6)
    plain = ra.fused.FusedBPRAdagrad(item0, user0, **hp)
    want = [plain.step(n, user_ids=u, pos_ids=p, sampler=sampler) for u, p in batches]
    want = [(l.clone(), i.clone()) for l, i in want]
    item1, user1 = iw.to(DEV).clone(), uw.to(DEV).clone()
    torch.manual_seed(6)
    ahead = ra.fused.FusedBPRAdagrad(item1, user1, **hp)
    ticket = ahead.prepare(n, user_ids=batches[0][0], pos_ids=batches[0][1], sampler=sampler)
    for k in range(steps):
        nxt = ahead.prepare(n, user_ids=batches[k + 1][0], pos_ids=batches[k + 1][1], sampler=sampler) if k + 1 < steps else None
        loss, ids = ahead.step_prepared(ticket)
        assert torch.equal(ids, want[k][1]) and torch.equal(loss, want[k][0])
        ticket = nxt
    torch.cuda.synchronize()
    assert torch.equal(item1, item0) and torch.equal(user1, user0) and not torch.equal(item0, iw.to(DEV))
    assert ahead.t == plain.t == steps
    for k in ('is', 'us'):
        assert torch.equal(ahead.state[k], plain.state[k]) and bool(ahead.state[k].any())


# ---------------------------------------------------------------------------------------------------------------- loud errors
def test_adagrad_errors_are_loud_and_touch_nothing(ra):
    """Bad arguments raise an exception that names the entry point, before any launch: both tables are bit-unchanged."""
    g = torch.Generator(device=DEV).manual_seed(1)
    N, d, M, n = 101, 128, 40, 8
    w0, s0 = torch.randn(N, d, device=DEV, generator=g), torch.rand(N, d, device=DEV, generator=g)
    query = torch.randn(M, d, device=DEV, generator=g)
    neg = torch.randint(0, N, (M, n), device=DEV, generator=g)
    dneg = torch.randn(M, n, device=DEV, generator=g)
    _, ws = ra.ops.sort_step_elements(None, neg, N, pad_row=0, want_solo=False)

    def sorted_(w, s, q=query, **hp):
        ra.ops.adagrad_rows_sorted(w, s, q, neg, dneg, **{'lr': 0.1, **hp})

    def presorted(w, s, q=query, ws=ws, **hp):
        ra.ops.adagrad_rows_presorted(w, s, q, ws, M, n, dneg, **{'lr': 0.1, **hp})

    nat, ops = ra._native, ra.ops
    for call, entry in ((sorted_, 'rsa_rows_update_sorted'), (presorted, 'rsa_rows_update_presorted')):
        for hp in (dict(step=0), dict(eps=-1e-3), dict(lr_decay=-0.5)):
            w, s = w0.clone(), s0.clone()
            with pytest.raises(nat.NativeError, match=entry + ': bad Adagrad hyper-parameters'):
                call(w, s, **hp)
            torch.cuda.synchronize()
            assert torch.equal(w, w0) and torch.equal(s, s0)
        # no state_sum: refused by the binding ...
        w = w0.clone()
        with pytest.raises(TypeError, match='adagrad_rows_(pre)?sorted: state_sum'):
            call(w, None)
        assert torch.equal(w, w0)
        # embed_dim 100: not built
        w, s = (t[:, :100].contiguous() for t in (w0, s0))
        keep = (w.clone(), s.clone())
        with pytest.raises(nat.NativeError, match=entry + r'.*dim=100'):
            call(w, s, q=query[:, :100].contiguous())
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip((w, s), keep))
    # ... and by the library itself: no state_sum, Adam's state next to the Adagrad rule, an unknown rule
    for change, words in ((dict(state_sum=None), 'Adagrad needs state_sum'), (dict(exp_avg=nat.ptr(s0), exp_avg_sq=nat.ptr(s0)), 'no exp_avg'),
                          (dict(rule=5), 'unknown rule 5')):
        w, s = w0.clone(), s0.clone()
        a = ops._rows_update_args(w, query, None, M, n, None, dneg, None, 0)
        a.neg_ids, a.workspace, a.workspace_bytes = nat.ptr(neg), nat.ptr(ws), ws.numel()
        a.rule, a.state_sum, a.lr, a.eps, a.step = nat.ROWS_ADAGRAD, nat.ptr(s), 0.1, 1e-10, 1
        for k, v in change.items():
            setattr(a, k, v)
        for entry in ('rsa_rows_update_sorted', 'rsa_rows_update_presorted'):
            with pytest.raises(nat.NativeError, match=entry + ': .*' + words):
                nat.check(getattr(nat.lib(), entry)(ctypes.byref(a), ops._stream()), entry)
        torch.cuda.synchronize()
        assert torch.equal(w, w0) and torch.equal(s, s0)
    # a workspace too small for the presorted form
    w, s = w0.clone(), s0.clone()
    with pytest.raises(nat.NativeError, match='rsa_rows_update_presorted.*workspace too small'):
        presorted(w, s, ws=ws[:ws.numel() // 2])
    torch.cuda.synchronize()
    assert torch.equal(w, w0) and torch.equal(s, s0)


# ------------------------------------------------------------------------------------------------------------------------- fit
def test_bpr_fit_with_the_learners_adagrad_in_the_kernels(ra, golden):
    """BaseRetriever.fit on the ml-100k fixture (d = 64, n = 64, batch 512, learner: 'adagrad', 6 epochs) with
    train.fused_optimizer: 'learner' against the same configuration without it (autograd + torch.optim.Adagrad): the fused run's
    train loss at each of the six epochs within 2 % of the plain run's (the band tests/test_gpu_round4.py holds the reference's own
    trajectory to: other random streams, same data, same rule); final loss < 0.68 and recall@20 > 0.05 (the thresholds of
    test_bpr_fit_with_fused_optimizer); with train.fused_prefetch: 'adagrad' the model is bit-equal to the run without."""
    from test_dataset_golden import make
    ds = make(ra.TripletDataset, golden('data_ml100k'))
    trn, val, tst = ds.build(split_ratio=[0.8, 0.1, 0.1], shuffle=True)
    train = {'epochs': 6, 'negative_count': 64, 'batch_size': 512, 'learner': 'adagrad', 'learning_rate': 0.05, 'init_method': 'normal'}
    cfg = {'model': {'embed_dim': 64}, 'train': dict(train, fused_optimizer='learner'), 'eval': {'batch_size': 256}}
    model = ra.BPR(cfg)
    model.fit(trn, val)
    assert type(model._fused_step) is ra.fused.BPRAdagradStep and model._fused_step.stepper is None
    res = model.evaluate(tst)
    plain = ra.BPR({**cfg, 'train': train})
    plain.fit(trn, val)
    assert plain._fused_step is None
    got = np.array([h['train_loss'] for h in model.history])
    want = np.array([h['train_loss'] for h in plain.history])
    print('train loss per epoch, fused :', np.round(got, 5), '\n                      plain :', np.round(want, 5), '\nrecall@20', res['recall@20'])
    assert len(got) == len(want) == 6
    np.testing.assert_allclose(got, want, rtol=0.02)
    assert np.isfinite(got[-1]) and got[-1] < 0.68 and model.logged_metrics['train_loss'] == got[-1]
    assert res['recall@20'] > 0.05
    ahead = ra.BPR({**cfg, 'train': dict(cfg['train'], fused_prefetch='adagrad')})
    ahead.fit(trn, val)
    assert ahead._fused_step.stepper is ahead._fused_step
    assert torch.equal(ahead.item_encoder.weight, model.item_encoder.weight)
    assert torch.equal(ahead.query_encoder.weight, model.query_encoder.weight)
    assert ahead.logged_metrics['train_loss'] == model.logged_metrics['train_loss']
