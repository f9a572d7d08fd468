"""GPU: the lazy-Adam row update (rsa_rows_update_sorted / rsa_rows_update_presorted with exp_avg set: apply_run,
sorted_apply_kernel, sorted_finish_kernel, adam_of) against a float64 referee on weight, exp_avg AND exp_avg_sq, at the bound
derived in tests/adam_referee.py (no element of any case may exceed it), and the laziness / reproducibility / error contracts
around it.  The referee is pinned to torch.optim.SparseAdam by tests/test_adam_referee.py."""
import ctypes

import pytest
import torch

import adam_referee as ar

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SMALL_TOTAL = 1 << 18          # SORTED_SMALL_TOTAL of rsa_sorted.hip: at most this many elements -> 16-element chunks, else 64


@pytest.fixture(scope='module')
def ra():
    import recstudio_amd
    recstudio_amd._native.lib()
    return recstudio_amd


# ------------------------------------------------------------------------------------------------ id layouts (flat, element order)
def ids_distinct(g, total, N):
    return torch.randperm(N, device=DEV, generator=g)[:total]


def ids_few_rows(g, total, N):
    return torch.randint(0, N, (total,), device=DEV, generator=g)


def ids_mixed(g, total, N):
    """test_sorted_scatter_equals_atomic_backward_and_is_reproducible's duplication: every other element on one of 40 rows."""
    ids = torch.randint(0, 40, (total,), device=DEV, generator=g)
    ids[::2] = torch.randint(0, N, ((total + 1) // 2,), device=DEV, generator=g)
    return ids


def ids_chunk_aligned(g, total, N):
    """Runs laid out so that sorted positions that are multiples of the chunk size ARE run heads and run ends: whole-chunk runs, runs
    of 2 and 3 chunks (the middle chunk lies wholly inside: META_LEAD_FULL), runs that end exactly on a border after starting
    mid-chunk, a border crossed by one element on either side, single elements in the first / last slot of a chunk.  Row 0 (a
    padding row in some cases) leads with exactly one chunk."""
    ce = 16 if total <= SMALL_TOTAL else 64
    pattern = [ce, ce, 2 * ce, 3, ce - 3, 1, ce - 1, 3 * ce, ce - 1, 1, ce - 1, 2, ce - 1, ce + 1, ce - 1, ce - 5, 2 * ce + 5, 5, 2 * ce - 5]
    assert sum(pattern) % ce == 0          # (every group of the pattern ends on a border: the layout never drifts off it)
    lens, left = [], total
    while left > 0:
        for p in pattern:
            p = min(p, left)
            if p > 0:
                lens.append(p)
                left -= p
    assert len(lens) <= N
    rows = torch.arange(len(lens), device=DEV) * (N // len(lens))          # increasing ids with gaps: sorted order = this order
    ids = torch.repeat_interleave(rows, torch.tensor(lens, device=DEV))
    return ids[torch.randperm(total, device=DEV, generator=g)]


LAYOUTS = {'distinct': ids_distinct, 'few': ids_few_rows, 'mixed': ids_mixed, 'aligned': ids_chunk_aligned}


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
    hp = dict(lr=c.get('lr', 0.5), betas=c.get('betas', (0.9, 0.999)), eps=c.get('eps', 1e-8), step=c['step'])
    return kw, hp, conditioned_tables(g, N, d, kw, zero_state=c['zero'])


def conditioned_tables(g, N, d, kw, zero_state):
    """Weights of order 0.3; a nonzero prior state that makes the weights a real test: exp_avg random of the order of the row's
    gradient, exp_avg_sq in [0.5, 1.5] x the row's mean g^2 (bounded away from 0; rows the step does not touch: of order 1, so
    that laziness is checked on live values).  A zero state at step 1 gives m / sqrt(v) = sign(g) x a constant: any error in g
    cancels in the weights -- those cases are there for the moments."""
    w = torch.randn(N, d, device=DEV, generator=g) * 0.3
    if zero_state:
        return w, torch.zeros(N, d, device=DEV), torch.zeros(N, d, device=DEV)
    grad = ar.row_gradients(kw['query'], kw['neg_ids'], kw['dneg'], query_index=kw['query_index'], pos_ids=kw['pos_ids'],
                            dpos=kw['dpos'], upstream=kw['upstream'], pad_row=-1)
    scale = torch.ones(N, 1, device=DEV)
    scale[grad['rows']] = grad['g'].pow(2).mean(1, keepdim=True).clamp_min(1e-20).float()
    m = torch.randn(N, d, device=DEV, generator=g) * scale.sqrt()
    v = (0.5 + torch.rand(N, d, device=DEV, generator=g)) * scale
    return w, m, v


def run_sorted(ra, tables, kw, hp):
    w, m, v = (t.clone() for t in tables)
    ra.ops.adam_rows_sorted(w, m, v, kw['query'], kw['neg_ids'], kw['dneg'], query_index=kw['query_index'], pos_ids=kw['pos_ids'],
                            dpos=kw['dpos'], upstream=kw['upstream'], pad_row=kw['pad_row'], **hp)
    return w, m, v


def run_presorted(ra, tables, kw, hp):
    w, m, v = (t.clone() for t in tables)
    M, n = kw['neg_ids'].shape
    _, ws = ra.ops.sort_step_elements(kw['pos_ids'], kw['neg_ids'], w.shape[0], pad_row=kw['pad_row'], want_solo=False)
    ra.ops.adam_rows_presorted(w, m, v, kw['query'], ws, M, n, kw['dneg'], query_index=kw['query_index'], dpos=kw['dpos'],
                               upstream=kw['upstream'], pad_row=kw['pad_row'], **hp)
    return w, m, v


def check_against_referee(got, tables, kw, hp, rows=None, label=''):
    """Every element of every touched row of the three tables within the derived bound (the cap on the share of elements outside
    it is 0); -> the referee (for its row set) and the three max ratios."""
    ref = ar.referee(*tables, kw['query'], kw['neg_ids'], kw['dneg'], query_index=kw['query_index'], pos_ids=kw['pos_ids'],
                     dpos=kw['dpos'], upstream=kw['upstream'], pad_row=kw['pad_row'], rows=rows, **hp)
    r = ref['rows']
    ratios = ar.bound_ratios(ref, got[0][r], got[1][r], got[2][r])
    print(f'{label}: rows {r.numel()}, K max {int(ref["K"].max()) if r.numel() else 0}, error / bound: weight {ratios[0]:.3f} '
          f'exp_avg {ratios[1]:.3f} exp_avg_sq {ratios[2]:.3f}')
    assert max(ratios) <= 1.0, (label, ratios)
    return ref, ratios


def check_lazy(got, tables, touched_rows):
    rest = torch.ones(tables[0].shape[0], dtype=torch.bool, device=DEV)
    rest[touched_rows] = False
    for a, b in zip(got, tables):
        assert torch.equal(a[rest], b[rest])


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
                c.update(d=d, ce=ce, seed=s * 100 + len(out))
                out.append(pytest.param(c, id=f'd{d}-chunk{ce}-{name}'))
            # (a) all rows distinct; the exact SORTED_SMALL_TOTAL edges
            if big:
                add('distinct-total2^18+1-zero-step1', layout='distinct', M=4033, w=65, N=300_007, pos=True, qi=True, up=None, pad=-1,
                    step=1, zero=True)
                add('distinct-total300007-nopos-noqi-up-step1000', layout='distinct', M=300_007, w=1, N=400_009, pos=False, qi=False,
                    up=-0.73, pad=0, step=1000, zero=False)
            else:
                add('distinct-total2^18-1-zero-step1', layout='distinct', M=4161, w=63, N=300_007, pos=False, qi=True, up=None, pad=-1,
                    step=1, zero=True)
                add('distinct-total2^18-nopos-noqi-up-step1000', layout='distinct', M=4096, w=64, N=300_007, pos=False, qi=False, up=-0.73,
                    pad=0, step=1000, zero=False)
                add('small-total37', layout='few', M=37, w=1, N=11, pos=False, qi=True, up=None, pad=-1, step=2, zero=False, drop=True)
                add('ragged-total5003', layout='mixed', M=5003, w=1, N=997, pos=False, qi=True, up=1.7, pad=0, step=1, zero=False,
                    drop=True)
            # (b) 1, 2, 3, 40 rows with thousands of elements each: every row goes through sorted_finish_kernel
            M, w = (4033, 65) if big else (601, 33)
            add('rows1-pos-qi-up-step1000', layout='few', M=M, w=w, N=1, pos=True, qi=True, up=0.37, pad=-1, step=1000, zero=False)
            add('rows2-pad0-betas.5.9-step2', layout='few', M=M, w=w, N=2, pos=False, qi=True, up=None, pad=0, step=2, zero=False,
                betas=(0.5, 0.9), drop=True)
            add('rows3-padinterior-noqi-step1', layout='few', M=M, w=w, N=3, pos=True, qi=False, up=0.37, pad=1, step=1, zero=False)
            add('rows40-pad0-drop-zero-step2', layout='few', M=M, w=w, N=40, pos=True, qi=True, up=None, pad=0, step=2, zero=True, drop=True)
            # (c) runs that start and end exactly on chunk borders
            M, w = (4100, 65) if big else (1531, 33)
            add('aligned-pad0-step2', layout='aligned', M=M, w=w, N=200_003, pos=True, qi=True, up=None, pad=0, step=2, zero=False)
            add('aligned-nopad-noqi-up-zero-step1000', layout='aligned', M=M, w=w - 1, N=200_003, pos=False, qi=False, up=-2.5, pad=-1,
                step=1000, zero=True)
            # (d) mixed duplication, an interior padding row with many elements, dropped ids
            M, w = (4201, 65) if big else (777, 65)
            add('mixed-padinterior-drop-up-step1000', layout='mixed', M=M, w=w, N=3001, pos=True, qi=True, up=0.37, pad=17, step=1000,
                zero=False, drop=True)
            add('mixed-pad0-betas.5.9-lr1e-3-step1', layout='mixed', M=M, w=w - 1, N=3001, pos=False, qi=True, up=None, pad=0, step=1,
                zero=False, betas=(0.5, 0.9), lr=1e-3, drop=True)
    return out


@pytest.mark.parametrize('c', _cases())
def test_adam_rows_sorted_and_presorted_vs_float64_referee(ra, c):
    """ops.adam_rows_sorted called directly: weight, exp_avg, exp_avg_sq of every touched row within the derived bound of the float64
    referee; rows without a kept element (padding row, rows only dropped ids name, everything else) bit-unchanged in all three
    tables; a second call from the same start state and the sort_step_elements(want_solo=False) + adam_rows_presorted form equal
    the first bit for bit."""
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
    check_lazy(got, tables, ref['rows'])
    assert ref['rows'].numel() > 0
    if c['pad'] >= 0:
        assert not bool((ref['rows'] == c['pad']).any())
        if c['layout'] != 'distinct':
            ids = torch.cat([kw['neg_ids'].reshape(-1)] + ([kw['pos_ids']] if kw['pos_ids'] is not None else []))
            assert int((ids == c['pad']).sum()) > (0 if c['N'] > 1000 else 30)          # the padding row really has elements
    if c['layout'] == 'few' and c['N'] <= 40 and total > 1000:
        assert int(ref['K'].min()) > 16 * 8          # every row spans many chunks: all of them through the finish kernel


@pytest.mark.parametrize('d,M,U', [(64, 5000, 1201), (128, 65536, 20_011), (256, 5000, 1201), (64, 270_001, 50_021), (128, 270_001, 50_021),
                                   (256, 270_001, 50_021)])
@pytest.mark.parametrize('zero,step', [(False, 7), (True, 1)])
def test_adam_user_side_form(ra, d, M, U, zero, step):
    """The call FusedBPRAdam makes for the user table: neg_ids = user_ids.view(M, 1), coefficients of ones, query = the block of
    per-query gradients, no query_index, duplicate users in the batch; 16-element chunks (M <= 2^18) and 64-element chunks."""
    g = torch.Generator(device=DEV).manual_seed(d + M)
    uid = torch.randint(1, U, (M,), device=DEV, generator=g)
    uid[:64] = uid[64:128]
    qgrad = torch.randn(M, d, device=DEV, generator=g) * 1e-3
    kw = dict(query=qgrad, neg_ids=uid.view(M, 1), dneg=torch.ones(M, 1, device=DEV), query_index=None, pos_ids=None, dpos=None,
              upstream=None, pad_row=0)
    hp = dict(lr=0.5, betas=(0.9, 0.999), eps=1e-8, step=step)
    tables = conditioned_tables(g, U, d, kw, zero_state=zero)
    got, again, pre = run_sorted(ra, tables, kw, hp), run_sorted(ra, tables, kw, hp), run_presorted(ra, tables, kw, hp)
    for a, b, p in zip(got, again, pre):
        assert torch.equal(a, b) and torch.equal(a, p)
    ref, _ = check_against_referee(got, tables, kw, hp, label=f'user side d={d} M={M}')
    check_lazy(got, tables, ref['rows'])
    assert int(ref['K'].max()) > 1 and torch.equal(got[0][0], tables[0][0])


def test_adam_streaming_form_table_over_512_mb(ra):
    """A table over 512 MB (N = 1 100 000, d = 128: 563 MB) takes the streaming (nontemporal) form of sorted_apply_kernel for the
    weight AND both state tables, while sorted_finish_kernel reads and writes the same tables with plain accesses: total > 2^18,
    most rows with one or two elements, ten rows with runs of thousands (finish kernel).  Referee on the touched rows; every
    other row of the three tables bit-unchanged."""
    N, d, M, w = 1_100_000, 128, 5000, 65
    assert N * d * 4 > (512 << 20)
    g = torch.Generator(device=DEV).manual_seed(77)
    ids = torch.randint(1, N, (M * w,), device=DEV, generator=g)
    hot = torch.randint(1, N, (10,), device=DEV, generator=g)
    sel = torch.rand(M * w, device=DEV, generator=g) < 0.15
    ids[sel] = hot[torch.randint(0, 10, (int(sel.sum()),), device=DEV, generator=g)]
    ids[torch.rand(M * w, device=DEV, generator=g) < 0.05] = -1
    ids = ids.view(M, w)
    coef = torch.randn(M, w, device=DEV, generator=g)
    query = torch.randn(999, d, device=DEV, generator=g)
    qi = torch.randint(0, 999, (M,), device=DEV, generator=g)
    kw = dict(query=query, neg_ids=ids[:, 1:].contiguous(), dneg=coef[:, 1:].contiguous(), query_index=qi, pos_ids=ids[:, 0].contiguous(),
              dpos=coef[:, 0].contiguous(), upstream=torch.tensor([0.61], device=DEV), pad_row=0)
    hp = dict(lr=0.5, betas=(0.9, 0.999), eps=1e-8, step=3)
    tables = conditioned_tables(g, N, d, kw, zero_state=False)
    got = run_sorted(ra, tables, kw, hp)
    pre = run_presorted(ra, tables, kw, hp)
    for a, p in zip(got, pre):
        assert torch.equal(a, p)
    ref, _ = check_against_referee(got, tables, kw, hp, label='streaming')
    assert int(ref['K'].max()) > 3000 and ref['rows'].numel() > 150_000
    check_lazy(got, tables, ref['rows'])


# ------------------------------------------------------------------------------------------------------------- FusedBPRAdam
def _bpr_referee_inputs(ra, iw0, uw0, n, uid, pos, neg):
    """dpos / dneg / per-query gradients of the step on the START weights, from a plain fused_forward (the loss tests pin it to the
    oracle): the item gradient needs the pre-update user rows."""
    o = ra.ops.fused_forward(iw0, uw0, n, query_index=uid, pos_ids=pos, neg_ids=neg, sampler=ra._native.SAMPLER_GIVEN, want_logp=False,
                             fused_bpr=True, want_query_grad=True)
    return o['dpos'].clone(), o['dneg'].clone(), o['query_grad'].clone()


def test_adam_step_headline_shape(ra):
    """FusedBPRAdam.step at BASELINE configs[1]'s size (N = 1e7 + 1, U = 1e6 + 1, d = 128, B = 65 536, n = 64, popularity
    sampler), a conditioned nonzero state, t preset to 41 so that the step is the 42nd: negatives == torch's stream; touched item
    and user rows moved and no other row of any of the six tables, row 0 untouched; a seeded sample of 4096 touched item rows (half
    of them with more than one element) and 4096 user rows within the derived bound of the float64 referee on weight, exp_avg
    and exp_avg_sq; two runs bit-equal."""
    N, U, d, B, n, lr = 10_000_001, 1_000_001, 128, 65536, 64, 0.05
    g = torch.Generator(device=DEV).manual_seed(12)
    iw0 = torch.empty(N, d, device=DEV).normal_(0, 0.1, generator=g)
    iw0[0] = 0
    uw0 = torch.empty(U, d, device=DEV).normal_(0, 0.1, generator=g)
    counts = (torch.rand(N, generator=torch.Generator().manual_seed(2)) ** 8 * 1e4).long()
    ps = ra.PopularSamplerModel(counts).to(DEV)
    uid = torch.randint(1, U, (B,), device=DEV, generator=g)
    uid[:64] = uid[64:128]
    pos = torch.randint(1, N, (B,), device=DEV, generator=g)
    torch.manual_seed(5)
    want_ids = torch.searchsorted(ps.table, torch.rand(B, n, device=DEV)).clamp_(max=N - 1)
    dpos, dneg, qgrad = _bpr_referee_inputs(ra, iw0, uw0, n, uid, pos, want_ids)
    # the state: of the order of a typical one-element gradient (coefficient x user row), exp_avg_sq bounded away from 0
    g_typ = float(dneg.abs().mean()) * 0.1
    u_typ = float(qgrad.abs().mean())
    state0 = {'im': torch.empty(N, d, device=DEV).normal_(0, g_typ, generator=g),
              'iv': torch.empty(N, d, device=DEV).uniform_(0.5, 1.5, generator=g) * g_typ ** 2,
              'um': torch.empty(U, d, device=DEV).normal_(0, u_typ, generator=g),
              'uv': torch.empty(U, d, device=DEV).uniform_(0.5, 1.5, generator=g) * u_typ ** 2}
    runs = []
    for _ in range(2):
        iw, uw = iw0.clone(), uw0.clone()
        fa = ra.fused.FusedBPRAdam(iw, uw, lr=lr)
        fa.state = {k: v.clone() for k, v in state0.items()}
        fa.t = 41
        torch.manual_seed(5)
        loss, ids = fa.step(n, user_ids=uid, pos_ids=pos, sampler=ps)
        torch.cuda.synchronize()
        runs.append((loss.clone(), ids.clone(), iw, uw, fa.state))
        assert fa.t == 42
    (l1, i1, it1, us1, st1), (l2, i2, it2, us2, st2) = runs
    assert torch.equal(i1, want_ids) and torch.equal(i2, want_ids)
    assert torch.equal(l1, l2) and torch.equal(it1, it2) and torch.equal(us1, us2)
    assert all(torch.equal(st1[k], st2[k]) for k in st1)
    del runs, it2, us2, st2
    touched = torch.zeros(N, dtype=torch.bool, device=DEV)
    touched[pos] = True
    touched[i1.reshape(-1)] = True
    touched[0] = False
    um = torch.zeros(U, dtype=torch.bool, device=DEV)
    um[uid] = True
    um[0] = False
    for got, start, mask in ((it1, iw0, touched), (st1['im'], state0['im'], touched), (st1['iv'], state0['iv'], touched),
                             (us1, uw0, um), (st1['um'], state0['um'], um), (st1['uv'], state0['uv'], um)):
        moved = (got != start).any(1)
        assert not bool((moved & ~mask).any()) and not bool(moved[0])
        assert int((mask & ~moved).sum()) <= 8          # (an update that rounds to nothing on all 128 components: practically never)
    # a seeded sample: 2048 rows with one element, 2048 with more; 4096 user rows
    cnt = torch.bincount(torch.cat([pos, i1.reshape(-1)]), minlength=N)
    cnt[0] = 0
    gs = torch.Generator(device=DEV).manual_seed(99)
    one, many = (cnt == 1).nonzero().view(-1), (cnt > 1).nonzero().view(-1)
    rows = torch.cat([one[torch.randperm(one.numel(), device=DEV, generator=gs)[:2048]],
                      many[torch.randperm(many.numel(), device=DEV, generator=gs)[:2048]]])
    assert rows.numel() == 4096
    hp = dict(lr=lr, betas=(0.9, 0.999), eps=1e-8, step=42)
    kw = dict(query=uw0, neg_ids=i1, dneg=dneg, query_index=uid, pos_ids=pos, dpos=dpos, upstream=None, pad_row=0)
    ref, _ = check_against_referee((it1, st1['im'], st1['iv']), (iw0, state0['im'], state0['iv']), kw, hp, rows=rows, label='headline items')
    assert ref['rows'].numel() == 4096 and int((ref['K'] > 1).sum()) == 2048
    urows = um.nonzero().view(-1)
    urows = torch.cat([uid[:64].unique(), urows[torch.randperm(urows.numel(), device=DEV, generator=gs)[:4096]]]).unique()
    kw = dict(query=qgrad, neg_ids=uid.view(B, 1), dneg=torch.ones(B, 1, device=DEV), query_index=None, pos_ids=None, dpos=None,
              upstream=None, pad_row=0)
    ref, _ = check_against_referee((us1, st1['um'], st1['uv']), (uw0, state0['um'], state0['uv']), kw, hp, rows=urows, label='headline users')
    assert ref['rows'].numel() >= 4096 and int(ref['K'].max()) > 1


def _torch_bpr_trajectory(dtype, iw0, uw0, batches, lr):
    """torch.optim.SparseAdam on sparse embeddings, BPR loss (-mean logsigmoid(pos - neg)) by autograd on ITS OWN weights; CPU (its
    index_add is sequential: the run is reproducible)."""
    iw = torch.nn.Parameter(iw0.cpu().to(dtype).clone())
    uw = torch.nn.Parameter(uw0.cpu().to(dtype).clone())
    opt = torch.optim.SparseAdam([iw, uw], lr=lr)
    F = torch.nn.functional
    for uid, pos, neg in batches:
        opt.zero_grad()
        q = F.embedding(uid.cpu(), uw, sparse=True)
        ps = (q * F.embedding(pos.cpu(), iw, sparse=True)).sum(-1)
        ns = (q.unsqueeze(1) * F.embedding(neg.cpu(), iw, sparse=True)).sum(-1)
        (-F.logsigmoid(ps.unsqueeze(1) - ns).mean()).backward()
        opt.step()
    return [iw.data, opt.state[iw]['exp_avg'], opt.state[iw]['exp_avg_sq'], uw.data, opt.state[uw]['exp_avg'], opt.state[uw]['exp_avg_sq']]


def test_adam_trajectory_of_20_steps_vs_float64_sparse_adam(ra):
    """20 FusedBPRAdam.step calls (d = 128, B = 512, n = 64, given negatives; items 1 .. 399 recur in every step, items of the upper
    half are touched in ONE step and then rest, users recur) against torch.optim.SparseAdam on float64 copies fed the float64
    gradients of the same loss on its own weights.  Two trajectories drift apart, so no derived bound applies: the yardstick is
    the reference's own fp32 error -- the distance of the SAME torch run in fp32 from the float64 run -- times 4 (two independent
    fp32 runs differ from each other by about that distance; 4 leaves room for another summation order), per table, in the
    maximum norm and in the rms.  Row 0 stays 0 / untouched.
    Measured on an MI355X, max |.| (rms) of kernel - float64 against torch fp32 - float64:
        item weight 1.14e-6 (1.05e-8) / 5.35e-7 (1.06e-8)   exp_avg 1.12e-10 (3.1e-12) / 1.33e-10 (5.6e-12)   exp_avg_sq 3.6e-15 (9.6e-17) / 8.3e-15 (1.9e-16)
        user weight 1.05e-6 (2.49e-8) / 5.87e-7 (2.47e-8)   exp_avg 1.37e-10 (1.1e-11) / 9.7e-11 (1.1e-11)   exp_avg_sq 3.7e-15 (2.2e-16) / 4.6e-15 (2.3e-16)
    (with the hyper-parameters rounded to fp32 first, as before ABI 12: exp_avg_sq 1.9e-13 / 1.5e-13 -- 23 and 32 x torch's own fp32 distance)."""
    N, U, d, B, n, lr, steps = 6001, 701, 128, 512, 64, 0.01, 20
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
    want = _torch_bpr_trajectory(torch.float64, iw0, uw0, batches, lr)
    t32 = _torch_bpr_trajectory(torch.float32, iw0, uw0, batches, lr)
    iw, uw = iw0.to(DEV), uw0.to(DEV)
    fa = ra.fused.FusedBPRAdam(iw, uw, lr=lr)
    for uid, pos, neg in batches:
        fa.step(n, user_ids=uid.to(DEV), pos_ids=pos.to(DEV), neg_ids=neg.to(DEV))
    torch.cuda.synchronize()
    got = [iw, fa.state['im'], fa.state['iv'], uw, fa.state['um'], fa.state['uv']]
    assert not iw[0].any() and not fa.state['im'][0].any() and not fa.state['iv'][0].any()
    bad = []
    for name, a, b, w in zip(('item weight', 'item exp_avg', 'item exp_avg_sq', 'user weight', 'user exp_avg', 'user exp_avg_sq'), got, t32, want):
        ek, et = (a.cpu().double() - w).abs(), (b.double() - w).abs()
        print(f'{name}: max |kernel - f64| {float(ek.max()):.3e} |torch fp32 - f64| {float(et.max()):.3e}   rms {float(ek.pow(2).mean().sqrt()):.3e}'
              f' / {float(et.pow(2).mean().sqrt()):.3e}')
        if not (float(ek.max()) <= 4 * float(et.max()) and float(ek.pow(2).mean().sqrt()) <= 4 * float(et.pow(2).mean().sqrt())):
            bad.append(name)
    assert not bad, bad


# ---------------------------------------------------------------------------------------------------------------- loud errors
def test_adam_errors_are_loud_and_touch_nothing(ra):
    """Bad arguments raise an exception that names the entry point, before any launch: the three tables are bit-unchanged."""
    g = torch.Generator(device=DEV).manual_seed(1)
    N, d, M, n = 101, 128, 40, 8
    w0, m0, v0 = (torch.randn(N, d, device=DEV, generator=g) for _ in range(3))
    v0 = v0.abs()
    query = torch.randn(M, d, device=DEV, generator=g)
    neg = torch.randint(0, N, (M, n), device=DEV, generator=g)
    dneg = torch.randn(M, n, device=DEV, generator=g)
    _, ws = ra.ops.sort_step_elements(None, neg, N, pad_row=0, want_solo=False)

    def sorted_(w, m, v, q=query, **hp):
        ra.ops.adam_rows_sorted(w, m, v, q, neg, dneg, **{'lr': 0.1, **hp})

    def presorted(w, m, v, q=query, ws=ws, **hp):
        ra.ops.adam_rows_presorted(w, m, v, q, ws, M, n, dneg, **{'lr': 0.1, **hp})

    for call, entry in ((sorted_, 'rsa_rows_update_sorted'), (presorted, 'rsa_rows_update_presorted')):
        for hp in (dict(step=0), dict(betas=(1.0, 0.999)), dict(betas=(0.9, 1.5)), dict(betas=(-0.1, 0.999))):
            w, m, v = w0.clone(), m0.clone(), v0.clone()
            with pytest.raises(ra._native.NativeError, match=entry):
                call(w, m, v, **hp)
            torch.cuda.synchronize()
            assert torch.equal(w, w0) and torch.equal(m, m0) and torch.equal(v, v0)
        # exp_avg without exp_avg_sq: refused by the binding ...
        w, m = w0.clone(), m0.clone()
        with pytest.raises(TypeError, match='adam_rows_(pre)?sorted: exp_avg_sq'):
            call(w, m, None)
        assert torch.equal(w, w0) and torch.equal(m, m0)
        # embed_dim 100: not built
        w, m, v = (t[:, :100].contiguous() for t in (w0, m0, v0))
        keep = (w.clone(), m.clone(), v.clone())
        with pytest.raises(ra._native.NativeError, match=entry + r'.*dim=100'):
            call(w, m, v, q=query[:, :100].contiguous())
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip((w, m, v), keep))
    # ... and by the library itself
    nat, ops = ra._native, ra.ops
    w, m = w0.clone(), m0.clone()
    a = ops._rows_update_args(w, query, None, M, n, None, dneg, None, 0)
    a.neg_ids, a.workspace, a.workspace_bytes = nat.ptr(neg), nat.ptr(ws), ws.numel()
    a.exp_avg, a.lr, a.beta1, a.beta2, a.eps, a.step = nat.ptr(m), 0.1, 0.9, 0.999, 1e-8, 1
    for fn, entry in ((nat.lib().rsa_rows_update_sorted, 'rsa_rows_update_sorted'), (nat.lib().rsa_rows_update_presorted, 'rsa_rows_update_presorted')):
        with pytest.raises(nat.NativeError, match=entry + ': bad optimizer state'):
            nat.check(fn(ctypes.byref(a), ops._stream()), entry)
    torch.cuda.synchronize()
    assert torch.equal(w, w0) and torch.equal(m, m0)
    # a workspace too small for the presorted form
    w, m, v = w0.clone(), m0.clone(), v0.clone()
    with pytest.raises(nat.NativeError, match='rsa_rows_update_presorted.*workspace too small'):
        presorted(w, m, v, ws=ws[:ws.numel() // 2])
    torch.cuda.synchronize()
    assert torch.equal(w, w0) and torch.equal(m, m0) and torch.equal(v, v0)
