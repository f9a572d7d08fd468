"""GPU: the in-place BPR SGD step -- fused.bpr_sgd_step all-sorted and in-forward (rsa_bpr_sgd_prepare / rsa_bpr_sgd_apply), fused.PrefetchedBPRSGD,
and the float-atomic forms outside the stock dims -- against the float64 referee of tests/sgd_referee.py, on the UPDATE: every
element of every touched item and user row within Stage A (the update arithmetic from the kernel's own coefficients) and
within the end-to-end bound (the float64 step), every other row bit-unchanged, the loss against float64 at 1e-5, a second run
bit-equal.  Learning rates are batch-sized (lr = c B, BPRLoss being a mean over B n terms): each case asserts from the referee
alone that the median |update| / |weight| of the touched rows exceeds 1e-3, so an error of first OR second order in the update
is far above the bounds.  The referee is pinned to torch.optim.SGD and its bounds to the mistakes they must catch by
tests/test_sgd_referee.py.

The sigmoid allowance of Stage B is measured where the test runs: twice the worst error of torch's fp32 sigmoid(x) / n / M on
this device (sgd_referee.torch_sigmoid_allowance).  Measured on an MI355X: torch's maximum 2.4 .. 3.9 u (by M), the allowance
4.9 .. 7.9 u; the kernel's bpr_dneg up to 9.97 u at |x| = 7.3 -- above the allowance, and growing with |x|: the argument
error of the hardware exp, which Stage B carries as the derived term 2u |x| (sgd_referee.py); with it the kernel is at
<= 0.56 of the sigmoid bound.  Every test prints its error / bound figures (run with -s)."""
import pytest
import torch

import sgd_referee as sr
from sgd_step_forms import FORMS
from test_gpu_adam_rows import ids_chunk_aligned, SMALL_TOTAL

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
RDX_TILE = 4096          # rsa_radix.hpp: at most this many sort elements (B * 66) -> the one-workgroup sort, the stand-alone sampler


@pytest.fixture(scope='module')
def ra():
    import recstudio_amd
    recstudio_amd._native.lib()
    return recstudio_amd


# --------------------------------------------------------------------------------------------------------------------- the cases
def _tables(g, N, U, d):
    iw = torch.randn(N, d, device=DEV, generator=g) * 0.3
    iw[0] = 0
    uw = torch.randn(U, d, device=DEV, generator=g) * 0.3
    uw[0] = 0
    return iw, uw


def make_case(ra, c):
    """-> dict(iw0, uw0, uid, pos, sampler | None, neg | None, lr, n)."""
    d, B, N, n = c['d'], c['B'], c['N'], 64
    U = c.get('U', 211)
    g = torch.Generator(device=DEV).manual_seed(c['seed'])
    iw0, uw0 = _tables(g, N, U, d)
    uid = torch.randint(1, U, (B,), device=DEV, generator=g)
    pos = torch.randint(1, N, (B,), device=DEV, generator=g)
    sampler = neg = None
    s = c['sampler']
    if s == 'uniform':
        sampler = ra.UniformSampler(N)
    elif s == 'popular':          # a hot head: a handful of rows take most of the draws, the tail is touched once or never
        counts = (torch.rand(N, generator=torch.Generator().manual_seed(c['seed'])) ** 8 * 1e4).long()
        sampler = ra.PopularSamplerModel(counts).to(DEV)
    elif s == 'given-solo':       # every id once: every row solo, the apply pass has nothing to do
        ids = (torch.randperm(N - 1, device=DEV, generator=g)[:B * (n + 1)] + 1).view(B, n + 1)
        pos, neg = ids[:, 0].contiguous(), ids[:, 1:].contiguous()
        uid = torch.randperm(U - 1, device=DEV, generator=g)[:B] + 1
        uid[B // 2:B // 2 + 8] = uid[:8]          # (eight users twice)
    elif s == 'given-planted':
        neg = torch.randint(1, N, (B, n), device=DEV, generator=g)
        pos[11] = 0                               # a padding positive
        neg[:, 0] = pos.roll(1)                   # a negative that is another query's positive
        neg[::3, 1] = 0                           # padding ids among the negatives
        neg[::5, 2] = neg[::5, 3]                 # the same negative twice in one query
        neg[::7, 4] = pos[::7]                    # a negative equal to its own positive
        uid[5] = 0                                # user id 0
        uid[20:24] = uid[19]                      # a user five times
    elif s == 'given-aligned':                    # runs laid on the chunk borders of the item part of the sort
        ids = ids_chunk_aligned(g, B * (n + 1), N).view(B, n + 1)
        pos, neg = ids[:, 0].contiguous(), ids[:, 1:].contiguous()
    else:
        raise KeyError(s)
    users = c.get('users')
    if users == 'hot':                            # one user in more than 200 queries: long runs in the user part of the sort
        uid[torch.randperm(B, device=DEV, generator=g)[:max(201, B // 3)]] = 7
        uid[3] = 0
    elif users == 'one':
        uid[:] = 5
    return dict(iw0=iw0, uw0=uw0, uid=uid, pos=pos, sampler=sampler, neg=neg, lr=float(c.get('c', 1.0) * B), n=n)


def _cases():
    out = []

    def add(name, **c):
        c['seed'] = 1000 + len(out)
        out.append(pytest.param(c, id=name))
    for d in (64, 128, 256):
        a, b = ('uniform', 'popular') if d != 128 else ('popular', 'uniform')
        add(f'd{d}-B1-{a}', d=d, B=1, N=211, sampler=a)
        # B * 66 sort elements around RDX_TILE: the one-workgroup sort + stand-alone sampler (62) / the draw inside the sort's first launch (63)
        add(f'd{d}-B62-{a}', d=d, B=62, N=2003, sampler=a)
        add(f'd{d}-B63-{a}', d=d, B=63, N=2003, sampler=a)
        add(f'd{d}-B63-{b}', d=d, B=63, N=2003, sampler=b, c=2.0)
        # B * 65 item elements around SORTED_SMALL_TOTAL: 16- / 64-element chunks
        add(f'd{d}-B4032-{a}', d=d, B=4032, N=200_003, U=3001, sampler=a)
        add(f'd{d}-B4033-{a}', d=d, B=4033, N=200_003, U=3001, sampler=a)
        add(f'd{d}-B4033-{b}', d=d, B=4033, N=50_021, U=3001, sampler=b, c=0.5)
        add(f'd{d}-B5003-ragged-{b}', d=d, B=5003, N=50_021, U=1201, sampler=b, c=0.5)
        add(f'd{d}-N2-one-live-row', d=d, B=257, N=2, sampler='uniform')
        add(f'd{d}-N97-nearly-all-shared', d=d, B=700, N=97, sampler='uniform', c=2.0)
        add(f'd{d}-all-solo', d=d, B=300, N=40_009, U=401, sampler='given-solo')
        add(f'd{d}-planted', d=d, B=300, N=40_009, sampler='given-planted')
        add(f'd{d}-aligned-chunk16', d=d, B=1531, N=200_003, U=1201, sampler='given-aligned')
        add(f'd{d}-aligned-chunk64', d=d, B=4100, N=400_009, U=1201, sampler='given-aligned', c=0.5)
        add(f'd{d}-hot-user-{a}', d=d, B=700, N=3001, sampler=a, users='hot')
        add(f'd{d}-one-user-{b}', d=d, B=300, N=3001, sampler=b, users='one')
    return out


def _judge_form(ra, label, case, res, f64, in_table_atomics=False):
    """One form's result against Stage A (its own coefficients), Stage B (the coefficients against float64) and the end-to-end bound
    -> dict of the error / bound ratios, all asserted <= 1; rows that must not move: 0."""
    loss, neg, coef, iw, uw = res
    iw0, uw0, uid, pos, lr = case['iw0'], case['uw0'], case['uid'], case['pos'], case['lr']
    c, it64, us64, allow, torch_max = f64
    M, n = neg.shape
    it = sr.item_update(iw0, uw0, uid, pos, neg, coef['dpos'], coef['dneg'], lr, in_table_atomics=in_table_atomics)
    us = sr.user_update(uw0, uid, coef['query_grad'], lr, in_table_atomics=in_table_atomics)
    (a_item, moved_i), (a_user, moved_u) = sr.judge(it, iw, iw0), sr.judge(us, uw, uw0)
    a_qg = sr.query_grad_ratio(iw0, pos, neg, coef['dpos'], coef['dneg'], coef['query_grad'])
    # Stage B.  The sigmoid evaluation at the kernel's own fp32 argument (x = neg_score - pos_score, the difference it forms)
    x32 = coef['neg_score'] - coef['pos_score'].view(M, 1)
    units = sr.sigmoid_units(coef['dneg'], x32, 1.0 / (M * n))
    derived = 2.0 * x32.double().abs() * (1.0 - torch.sigmoid(x32.double()))          # the exp-argument term, in the same units
    sig_raw, sig_ratio = float(units.max()), float((units / (allow + derived)).max())
    small = x32.abs() < 0.5
    sig_small = float(units[small].max()) if bool(small.any()) else 0.0
    tn, tp = sr.coefficient_tolerances(c, allow)
    b_neg = float(((coef['dneg'].double() - c['dneg']).abs() / tn).max())
    b_pos = float(((coef['dpos'].double() - c['dpos']).abs() / tp).max())
    (e_item, m_i), (e_user, m_u) = sr.judge(it64, iw, iw0), sr.judge(us64, uw, uw0)
    loss_rel = abs(float(loss) - c['loss']) / abs(c['loss'])
    r = dict(a_item=a_item, a_user=a_user, a_qg=a_qg, sigmoid=sig_ratio, b_dneg=b_neg, b_dpos=b_pos, e_item=e_item, e_user=e_user)
    print(f'{label}: error / bound  Stage A items {a_item:.3f} users {a_user:.3f} query_grad {a_qg:.3f} | Stage B dneg {b_neg:.3f} dpos {b_pos:.3f} '
          f'| end to end items {e_item:.3f} users {e_user:.3f} | sigmoid: kernel max {sig_raw:.2f} u (max |x| {float(x32.abs().max()):.1f}; {sig_small:.2f} u over |x| < 0.5), torch max '
          f'{torch_max:.2f} u, allowance {allow:.2f} u, kernel / (allowance + 2|x|(1 - s)) {sig_ratio:.3f} | loss rel {loss_rel:.1e} | K max items '
          f'{int(it["K"].max())} users {int(us["K"].max())}')
    assert moved_i == 0 and moved_u == 0 and m_i == 0 and m_u == 0, (label, moved_i, moved_u)
    assert all(v <= 1.0 for v in r.values()), (label, r)          # (not max(): a NaN ratio must fail, and max(0.5, nan) is 0.5)
    assert loss_rel <= 1e-5, (label, loss_rel)
    return r


def _float64_side(case, neg, in_table_atomics=False):
    iw0, uw0, uid, pos, lr = case['iw0'], case['uw0'], case['uid'], case['pos'], case['lr']
    M, n = neg.shape
    c = sr.coefficients(iw0, uw0, uid, pos, neg)
    allow, torch_max = sr.torch_sigmoid_allowance(DEV, M, n)
    it64, us64 = sr.end_to_end(iw0, uw0, uid, pos, neg, lr, c, allow, in_table_atomics=in_table_atomics)
    return c, it64, us64, allow, torch_max


def _run(ra, form, case, seed, **kw):
    iw, uw = case['iw0'].clone(), case['uw0'].clone()
    torch.manual_seed(seed)
    loss, neg, coef = FORMS[form](ra, iw, uw, case['n'], case['lr'], case['uid'], case['pos'], case['sampler'], case['neg'], **kw)
    torch.cuda.synchronize()
    return loss, neg, coef, iw, uw


@pytest.mark.parametrize('c', _cases())
def test_sgd_step_vs_float64_referee(ra, c):
    """Every form that accepts the case (all-sorted; the two-call in-forward form; PrefetchedBPRSGD for the in-kernel samplers), d in
    {64, 128, 256}, samplers uniform / popular (hot head) / given.  Sizes: B = 1; B * 66 sort elements just below and above
    RDX_TILE (62, 63); B * 65 item elements on either side of SORTED_SMALL_TOTAL (4032, 4033); a ragged 5003.  Catalogs: N = 2
    (one live row, one run of 65 B elements -- there every query's update cancels exactly, so that case judges the long sum
    against its absolute terms and is the one case without the update-scale assertion), N = 97, every row solo, a hot head.
    Planted ids: a negative equal to its own positive, the same negative twice, another query's positive, padding negatives, a
    padding positive, runs on chunk borders.  Users: twice, one user in > 200 queries, the whole batch one user, user 0.
    Per form: Stage A on every element of every touched row of both tables and on query_grad, Stage B on the coefficients,
    the end-to-end bound, no other row changed by a bit, loss to 1e-5 of float64, a second run bit-equal; the forms draw the
    same negatives.

    Measured on an MI355X, the maximum of error / bound over the 48 cases and their forms (129 runs): Stage A items 0.668, users
    0.498, query_grad 0.121; Stage B dneg 0.262, dpos 0.020; end to end items 0.497, users 0.050.  The sigmoid: torch's maximum
    2.43 .. 3.94 u (by M), the allowance 4.85 .. 7.89 u, the kernel 9.97 u at most (3.99 u over |x| < 0.5), 0.556 of its bound with
    the exp-argument term.  All three forms write bit-equal dpos, dneg and query_grad (asserted)."""
    case = make_case(ra, c)
    forms = ['all-sorted', 'two-calls'] + (['prefetched'] if case['sampler'] is not None else [])
    total_sort, total_items = c['B'] * 66, c['B'] * 65
    if c['B'] in (62, 63):
        assert (total_sort > RDX_TILE) == (c['B'] == 63)
    if c['B'] in (4032, 4033):
        assert (total_items > SMALL_TOTAL) == (c['B'] == 4033)
    f64 = neg0 = coef0 = None
    for form in forms:
        res = _run(ra, form, case, seed=c['seed'])
        again = _run(ra, form, case, seed=c['seed'])
        assert torch.equal(res[0], again[0]) and torch.equal(res[1], again[1]) and torch.equal(res[3], again[3]) and torch.equal(res[4], again[4]), form
        if f64 is None:
            neg0 = res[1]
            f64 = _float64_side(case, neg0)
            c64, it64, us64 = f64[:3]
            if c['N'] > 2:
                si, su = sr.update_scale(it64), sr.update_scale(us64)
                print(f'median |update| / |weight|: items {si:.2e} users {su:.2e}; touched rows items {it64["rows"].numel()} users {us64["rows"].numel()}')
                assert si > 1e-3 and su > 1e-3
            if case['neg'] is not None:
                assert torch.equal(neg0, case['neg'])
        assert torch.equal(res[1], neg0), form          # the forms draw the same negatives
        if coef0 is None:
            coef0 = res[2]
        for k in ('dpos', 'dneg', 'query_grad'):        # ... and write the same coefficients, bit for bit (see _coefficients_of)
            assert torch.equal(res[2][k], coef0[k]), (form, k, float((res[2][k] - coef0[k]).abs().max()))
        _judge_form(ra, form, case, res, f64)
    K = it64['K']
    s = c['sampler']
    if s == 'given-solo':
        assert int(K.max()) == 1 and int(us64['K'].max()) == 2
    if s == 'given-planted':
        assert 0 not in it64['rows'].tolist() and 0 not in us64['rows'].tolist() and int((neg0 == 0).sum()) >= 100 and int(us64['K'].max()) >= 5
    if c['N'] == 2:
        assert it64['rows'].tolist() == [1] and int(K[0]) == 65 * c['B']
    if c.get('users') == 'hot':
        assert int(us64['K'].max()) > 200
    if c.get('users') == 'one':
        assert us64['rows'].tolist() == [5] and int(us64['K'][0]) == c['B']


# --------------------------------------------------------------------------------------- outside the stock dims: float atomics
@pytest.mark.parametrize('d,atomics,catalog', [(64, True, 'solo'), (128, True, 'solo'), (128, True, 'shared'), (32, False, 'solo'),
                                                (32, False, 'shared'), (32, True, 'shared'), (128, True, 'middle'), (32, False, 'middle')])
def test_sgd_step_float_atomic_forms_vs_float64_referee(ra, d, atomics, catalog):
    """bpr_sgd_step(atomics=True) and embed_dim 32: the item update goes through fused_backward(item_grad_out=weight) and, at d = 32,
    the user update through scatter_add_rows(out=weight) -- float atomics that accumulate IN the weight row, in a free order.  Same
    referee, no bit-reproducibility claim.  An in-table atomic rounds at the weight's magnitude once PER ELEMENT, where the
    2u |W'| of Stage A allows for one read-modify-write; whether (K + 2) u A + 2u |W'| still covers a correct implementation
    depends on the run length K (tests/test_sgd_referee.py shows it on an exact fp32 emulation, from both sides):
    * 'solo' (every item row one element, users once or twice): K <= 2, the plain bound, nothing added;
    * 'shared' (N = 97): the item rows, runs of more than 100 elements, are ASSERTED inside the plain Stage-A bound ((K + 2) u A has
      outgrown K u |W|); the user rows (1 .. 8 elements) carry the derived term (K - 2) u (|W| + |lr| A) of sgd_referee._finish --
      measured over the plain bound they reach 0.80 in one run and 0.60 in the next, the order of the atomics being free;
    * 'middle' (N = 1201, item runs of 3 .. 32 elements): the regime the plain bound cannot cover -- the kernels measure 2.91
      (d = 128) and 2.55 (d = 32) times it, the CPU emulation 2.3 to 2.9 -- judged with the term: items 0.63 / 0.61.
    Measured on an MI355X, Stage A items / users at most: solo 0.58 / 0.61, shared (items plain, users with the term) 0.25 / 0.61,
    middle 0.63 / 0.61; end to end at most 0.50."""
    B, n = 300, 64
    in_table = catalog != 'solo'
    c = dict(d=d, B=B, N={'solo': 40_009, 'shared': 97, 'middle': 1201}[catalog], U=401 if catalog == 'solo' else 211,
             sampler='given-solo' if catalog == 'solo' else 'uniform', seed=77 + d)
    case = make_case(ra, c)
    res = _run(ra, 'all-sorted', case, seed=3, atomics=atomics)
    f64 = _float64_side(case, res[1], in_table_atomics=in_table)
    assert sr.update_scale(f64[1]) > 1e-3 and sr.update_scale(f64[2]) > 1e-3
    _judge_form(ra, f'd{d} atomics={atomics} {catalog}', case, res, f64, in_table_atomics=in_table)
    K = f64[1]['K']
    plain = sr.item_update(case['iw0'], case['uw0'], case['uid'], case['pos'], res[1], res[2]['dpos'], res[2]['dneg'], case['lr'])
    plain_u = sr.user_update(case['uw0'], case['uid'], res[2]['query_grad'], case['lr'])
    plain_i, plain_us = sr.bound_ratio(plain, res[3]), sr.bound_ratio(plain_u, res[4])
    print(f'   over the plain Stage-A bound: items {plain_i:.3f} users {plain_us:.3f}; item runs of {int(K.min())} .. {int(K.max())} elements')
    if catalog == 'solo':
        assert int(K.max()) == 1 and int(f64[2]['K'].max()) == 2
    elif catalog == 'shared':
        assert int(K.min()) > 100 and plain_i <= 1.0, (int(K.min()), plain_i)
    else:
        assert 8 <= int(K.median()) and int(K.max()) <= 40


def test_sgd_step_errors_are_loud_and_touch_nothing(ra):
    """Bad arguments are refused by the host before any launch, with both tables bit-unchanged: embed_dim 100 (no query-gradient
    forward is built for it), num_neg = 32 for the in-forward form, ids of the wrong type, a workspace too small."""
    g = torch.Generator(device=DEV).manual_seed(2)
    N, U, B, n = 301, 53, 40, 64
    uid = torch.randint(1, U, (B,), device=DEV, generator=g)
    pos = torch.randint(1, N, (B,), device=DEV, generator=g)
    neg = torch.randint(1, N, (B, n), device=DEV, generator=g)

    def untouched(call, exc, match, d=128):
        iw0, uw0 = _tables(g, N, U, d)
        iw, uw = iw0.clone(), uw0.clone()
        with pytest.raises(exc, match=match):
            call(iw, uw)
        torch.cuda.synchronize()
        assert torch.equal(iw, iw0) and torch.equal(uw, uw0)

    untouched(lambda iw, uw: ra.fused.bpr_sgd_step(iw, uw, n, 1.0, user_ids=uid, pos_ids=pos, neg_ids=neg), (ValueError, ra._native.NativeError), 'query_grad', d=100)
    untouched(lambda iw, uw: ra.fused.bpr_sgd_step(iw, uw, 32, 1.0, user_ids=uid, pos_ids=pos, neg_ids=neg[:, :32].contiguous(), in_forward=True),
              ra._native.NativeError, 'rsa_bpr_sgd_prepare.*num_neg')
    untouched(lambda iw, uw: ra.fused.bpr_sgd_step(iw, uw, n, 1.0, user_ids=uid.int(), pos_ids=pos, neg_ids=neg, in_forward=True), TypeError,
              'bpr_sgd_step')

    def small_workspace(iw, uw):
        step = torch.full((1,), -1.0, device=DEV)
        b = ra.fused._sgd_step_block(iw, uw, n, B, ra._native.SAMPLER_GIVEN, None, step, neg=neg)
        a = b['args']
        a.user_ids, a.pos_ids = uid.data_ptr(), pos.data_ptr()
        a.item_workspace_bytes = a.item_workspace_bytes // 2
        ra._native.check(ra._native.lib().rsa_bpr_sgd_prepare(b['ref'], torch.cuda.current_stream().cuda_stream), 'rsa_bpr_sgd_prepare')
    untouched(small_workspace, ra._native.NativeError, 'rsa_bpr_sgd_prepare: item_workspace holds')


# ------------------------------------------------------------------------------------------------------------------- trajectory
def _torch_sgd_trajectory(dtype, iw0, uw0, batches, lrs):
    """torch.optim.SGD on two nn.Embedding(padding_idx=0)-like tables, BPR loss by autograd on ITS OWN weights, dense gradients with
    row 0 zeroed; CPU (sequential index_add: reproducible)."""
    iw = torch.nn.Parameter(iw0.cpu().to(dtype).clone())
    uw = torch.nn.Parameter(uw0.cpu().to(dtype).clone())
    opt = torch.optim.SGD([iw, uw], lr=lrs[0])
    F = torch.nn.functional
    for (uid, pos, neg), lr in zip(batches, lrs):
        for grp in opt.param_groups:
            grp['lr'] = lr
        opt.zero_grad()
        q = F.embedding(uid, uw, padding_idx=0)
        ps = (q * F.embedding(pos, iw, padding_idx=0)).sum(-1)
        ns = (q.unsqueeze(1) * F.embedding(neg, iw, padding_idx=0)).sum(-1)
        (-F.logsigmoid(ps.unsqueeze(1) - ns).mean()).backward()
        opt.step()
    return [iw.data, uw.data]


def test_sgd_trajectory_of_20_prefetched_steps_vs_float64_torch_sgd(ra):
    """20 PrefetchedBPRSGD steps (d = 128, B = 512, n = 64, popularity sampler with a hot head over N = 60 001: the head recurs in
    every step, rows of the tail are touched once and then rest; positives 1 .. 399 and 700 users recur), lr = B / 4 with
    set_lr(B / 8) after ten steps, against torch.optim.SGD on float64 copies fed its own float64 gradients on the negatives the
    stepper drew.  Trajectories drift, so no derived bound applies: the yardstick is the reference's own fp32 distance from
    float64 (the same torch run in fp32) times 4, per table, in the maximum norm and in the rms
    (test_adam_trajectory_of_20_steps_vs_float64_sparse_adam's argument).  Rows 0 stay 0.
    Not that test's batches themselves: PrefetchedBPRSGD draws its negatives with an in-kernel sampler and takes no given ids, so
    the structure of those batches is reproduced with a hot-head popularity sampler and ASSERTED on what was drawn (more than 20
    item rows touched in every step, more than 500 touched exactly once; the 700 users recur by construction).
    Measured on an MI355X, kernel - float64 against torch fp32 - float64 (largest movement of a weight over the run: 0.74 / 0.69):
    item weight max 4.020e-07 / 4.020e-07, rms 2.034e-08 / 2.035e-08; user weight max 2.284e-07 / 2.270e-07, rms 2.643e-08 / 2.685e-08
    -- the kernels are as far from float64 as torch's own fp32 run, to two digits."""
    N, U, d, B, n, steps = 60_001, 701, 128, 512, 64, 20
    g = torch.Generator().manual_seed(31)
    iw0 = torch.randn(N, d, generator=g) * 0.3
    iw0[0] = 0
    uw0 = torch.randn(U, d, generator=g) * 0.3
    uw0[0] = 0
    counts = (torch.rand(N, generator=g) ** 8 * 1e4).long()
    sampler = ra.PopularSamplerModel(counts).to(DEV)
    users = [torch.randint(1, U, (B,), generator=g) for _ in range(steps)]
    poss = [torch.randint(1, 400, (B,), generator=g) for _ in range(steps)]
    lrs = [B / 4.0] * (steps // 2) + [B / 8.0] * (steps - steps // 2)
    iw, uw = iw0.to(DEV), uw0.to(DEV)
    torch.manual_seed(17)
    stepper = ra.fused.PrefetchedBPRSGD(iw, uw, n, lrs[0], sampler)
    dev_batches = [(u.to(DEV), p.to(DEV)) for u, p in zip(users, poss)]
    batches = []
    ticket = stepper.prepare(*dev_batches[0])
    for k in range(steps):
        nxt = stepper.prepare(*dev_batches[k + 1]) if k + 1 < steps else None
        if k == steps // 2:
            stepper.set_lr(lrs[k])
        _, ids = stepper.step(ticket)
        batches.append((users[k], poss[k], ids.cpu()))
        ticket = nxt
    torch.cuda.synchronize()
    touched = torch.zeros(N, dtype=torch.int64)
    for _, p, ids in batches:
        t = torch.zeros(N, dtype=torch.bool)
        t[p] = True
        t[ids.reshape(-1)] = True
        touched += t
    assert int((touched == steps).sum()) > 20 and int((touched == 1).sum()) > 500          # rows that recur in every step, rows touched once
    want = _torch_sgd_trajectory(torch.float64, iw0, uw0, batches, lrs)
    t32 = _torch_sgd_trajectory(torch.float32, iw0, uw0, batches, lrs)
    assert not iw[0].any() and not uw[0].any()
    bad = []
    for name, a, b, w, start in zip(('item weight', 'user weight'), (iw, uw), t32, want, (iw0, uw0)):
        ek, et = (a.cpu().double() - w).abs(), (b.double() - w).abs()
        moved = float((w - start.double()).abs().max())
        print(f'{name}: max |kernel - f64| {float(ek.max()):.3e} |torch fp32 - f64| {float(et.max()):.3e}   rms {float(ek.pow(2).mean().sqrt()):.3e}'
              f' / {float(et.pow(2).mean().sqrt()):.3e}   (largest movement of a weight over the run {moved:.2f})')
        if not (float(ek.max()) <= 4 * float(et.max()) and float(ek.pow(2).mean().sqrt()) <= 4 * float(et.pow(2).mean().sqrt())):
            bad.append(name)
    assert not bad, bad
