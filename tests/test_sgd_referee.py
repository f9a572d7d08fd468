"""CPU: the float64 referee of the in-place BPR SGD step (tests/sgd_referee.py) is loss.backward() + torch.optim.SGD's own arithmetic,
an fp32 emulation of the kernels' arithmetic stays within half of the Stage-A bound the GPU tests apply, and each mistake in the
order or the bookkeeping of the update passes lands outside it at the learning rates the GPU cases use."""
import pytest
import torch

import sgd_referee as sr


def _torch_sgd_step(iw, uw, uid, pos, neg, lr):
    """float64 dense autograd + torch.optim.SGD on two nn.Embedding(padding_idx=0) tables -> (loss, W', U')."""
    item = torch.nn.Embedding(*iw.shape, padding_idx=0).double()
    user = torch.nn.Embedding(*uw.shape, padding_idx=0).double()
    with torch.no_grad():
        item.weight.copy_(iw.double())
        user.weight.copy_(uw.double())
    opt = torch.optim.SGD(list(item.parameters()) + list(user.parameters()), lr=lr)
    q = user(uid)
    loss = -torch.nn.functional.logsigmoid((q * item(pos)).sum(-1, keepdim=True) - (q.unsqueeze(1) * item(neg)).sum(-1)).mean(-1).mean()
    loss.backward()
    opt.step()
    return float(loss.detach()), item.weight.data, user.weight.data


def test_referee_equals_float64_autograd_plus_torch_sgd():
    """A case with duplicated users, a negative equal to its own positive, the same negative twice in a query, a padding id among
    the negatives, a padding positive, user id 0, and NONZERO rows 0 (the tables' values are used, their gradients dropped): the
    referee's float64 step == float64 dense autograd + torch.optim.SGD to 1e-12 on every row of both tables (the rows it does
    not name: unchanged), the loss included; the Stage-A form fed the float64 coefficients is the same step."""
    g = torch.Generator().manual_seed(4)
    N, U, d, M, n, lr = 50, 9, 8, 12, 6, 12.0
    iw, uw = torch.randn(N, d, generator=g), torch.randn(U, d, generator=g)
    uid = torch.randint(1, U, (M,), generator=g)
    uid[3], uid[7], uid[5] = uid[2], uid[2], 0
    pos = torch.randint(1, N, (M,), generator=g)
    neg = torch.randint(1, N, (M, n), generator=g)
    neg[1, 2] = pos[1]
    neg[4, 0] = neg[4, 5]
    neg[6, 3], neg[5, 1] = 0, 0
    pos[8] = 0
    neg[9, 4] = pos[10]
    loss, w_t, u_t = _torch_sgd_step(iw, uw, uid, pos, neg, lr)
    c = sr.coefficients(iw, uw, uid, pos, neg)
    it, us = sr.end_to_end(iw, uw, uid, pos, neg, lr, c, allow=4.0)
    assert abs(c['loss'] - loss) <= 1e-12
    w_r, u_r = iw.double().clone(), uw.double().clone()
    w_r[it['rows']] = it['w']
    u_r[us['rows']] = us['w']
    assert float((w_r - w_t).abs().max()) <= 1e-12 and float((u_r - u_t).abs().max()) <= 1e-12
    assert 0 not in it['rows'].tolist() and 0 not in us['rows'].tolist()
    assert torch.equal(w_t[0], iw[0].double()) and torch.equal(u_t[0], uw[0].double())
    assert int(it['K'].sum()) == int((pos != 0).sum() + (neg != 0).sum()) and int(us['K'].max()) >= 3
    a_it = sr.item_update(iw, uw, uid, pos, neg, c['dpos'], c['dneg'], lr)
    a_us = sr.user_update(uw, uid, c['qg'], lr)
    assert torch.equal(a_it['w'], it['w']) and torch.equal(a_us['w'], us['w'])
    assert bool((it['tol'] >= a_it['tol']).all()) and bool((us['tol'] >= a_us['tol']).all())


def _case(kind, seed=1, d=8):
    """Step inputs at the GPU cases' conditioning (weights of order 0.3, lr = M): 'solo' every item row one element; 'mixed' hot rows
    with runs across chunk borders next to solo rows, padding ids, duplicated users and user 0; 'long' two live item rows and
    two users: runs of about two thousand elements."""
    g = torch.Generator().manual_seed(seed)
    n = 64
    if kind == 'solo':
        N, U, M = 4000, 60, 40
        ids = (torch.randperm(N - 1, generator=g)[:M * (n + 1)] + 1).view(M, n + 1)
        pos, neg = ids[:, 0].contiguous(), ids[:, 1:].contiguous()
        uid = torch.randperm(U - 1, generator=g)[:M] + 1
    elif kind == 'mixed':
        N, U, M = 600, 20, 48
        pos = torch.randint(1, N, (M,), generator=g)
        neg = torch.randint(1, N, (M, n), generator=g)
        neg[:, ::2] = torch.randint(1, 6, (M, n // 2), generator=g)
        neg[::7, 3] = 0
        neg[:, 1] = pos.roll(1)
        pos[5] = 0
        uid = torch.randint(1, U, (M,), generator=g)
        uid[9] = 0
    else:
        N, U, M = 3, 3, 64          # (two live rows, not one: with a single live item row every query's update cancels to zero)
        pos = torch.randint(1, N, (M,), generator=g)
        neg = torch.randint(1, N, (M, n), generator=g)
        uid = torch.randint(1, U, (M,), generator=g)
    iw, uw = torch.randn(N, d, generator=g) * 0.3, torch.randn(U, d, generator=g) * 0.3
    iw[0] = 0
    uw[0] = 0
    return iw, uw, uid, pos, neg, float(M)


def _stage_a(case, chunk, mutant=None):
    iw, uw, uid, pos, neg, lr = case
    dpos, dneg, qg = sr.emulate_coefficients_fp32(iw, uw, uid, pos, neg)
    w1, u1 = sr.emulate_step_fp32(iw, uw, uid, pos, neg, dpos, dneg, qg, lr, chunk=chunk, mutant=mutant)
    it = sr.item_update(iw, uw, uid, pos, neg, dpos, dneg, lr)
    us = sr.user_update(uw, uid, qg, lr)
    (ri, mi), (ru, mu) = sr.judge(it, w1, iw), sr.judge(us, u1, uw)
    return dict(item=ri, user=ru, moved=mi + mu, qg=sr.query_grad_ratio(iw, pos, neg, dpos, dneg, qg), it=it, us=us, w1=w1, u1=u1,
                coef=(dpos, dneg, qg))


def _cpu_sigmoid_allowance(M=48, n=64):
    """twice the worst error, in units of u x the result, of torch's CPU fp32 sigmoid(x) / n / M (the GPU test: the device's)"""
    x = torch.linspace(-16, 16, 1 << 16)
    d32 = (torch.sigmoid(x) * torch.tensor(1.0 / n)) * torch.tensor(1.0 / M)
    return 2 * float(sr.sigmoid_units(d32, x, 1.0 / (M * n)).max())


@pytest.mark.parametrize('kind', ['solo', 'mixed', 'long'])
@pytest.mark.parametrize('chunk', [16, 64])
def test_fp32_emulation_stays_within_half_the_bound(kind, chunk):
    """An fp32 emulation of the kernels' arithmetic (stable sort by id, 16- and 64-element chunks with partials, one rounding per
    multiply-add, upstream * sum then one add, solo rows as row + scale * (d * q)) stays within HALF the Stage-A bound on both
    tables and on query_grad: single-element rows, runs across chunk borders, runs of about two thousand elements; and within the end-to-end bound with the sigmoid allowance taken from torch's CPU fp32 sigmoid the way the GPU test
    takes it from the device's.  The learning rate is batch-sized (lr = M): the median update is more than 1e-3 of the weight."""
    case = _case(kind)
    r = _stage_a(case, chunk)
    print(f'{kind} chunk {chunk}: error / Stage-A bound: items {r["item"]:.3f} users {r["user"]:.3f} query_grad {r["qg"]:.3f}; '
          f'K max {int(r["it"]["K"].max())}')
    assert r['item'] <= 0.5 and r['user'] <= 0.5 and r['qg'] <= 0.5 and r['moved'] == 0, r
    assert sr.update_scale(r['it']) > 1e-3 and sr.update_scale(r['us']) > 1e-3
    if kind == 'long':
        assert int(r['it']['K'].min()) > 1500 and int(r['us']['K'].min()) > 20
    if kind == 'solo':
        assert int(r['it']['K'].max()) == 1
    iw, uw, uid, pos, neg, lr = case
    c = sr.coefficients(iw, uw, uid, pos, neg)
    it, us = sr.end_to_end(iw, uw, uid, pos, neg, lr, c, allow=_cpu_sigmoid_allowance())
    ei, eu = sr.judge(it, r['w1'], iw)[0], sr.judge(us, r['u1'], uw)[0]
    print(f'   error / end-to-end bound: items {ei:.3f} users {eu:.3f}')
    assert ei <= 1.0 and eu <= 1.0
    dpos, dneg, _ = r['coef']
    tn, tp = sr.coefficient_tolerances(c, _cpu_sigmoid_allowance())
    assert bool(((dneg.double() - c['dneg']).abs() <= tn).all()) and bool(((dpos.double() - c['dpos']).abs() <= tp).all())


@pytest.mark.parametrize('mutant', sr.MUTANTS)
def test_every_planted_mistake_is_outside_the_bound(mutant):
    """Each of these lands OUTSIDE the Stage-A bound (or moves a row that must not move) on the 'mixed' case at lr = M, in both chunk
    regimes, and outside the end-to-end bound as well: the item apply reading post-update user rows; the user apply issued
    before the shared item rows were applied (solo rows already done by the forward); a solo row updated twice (in the
    forward and again in the apply pass); a solo row not updated; one element dropped from the longest run; a duplicated
    user's gradients applied once; the padding row moved; the step scale applied to every chunk partial and again to the
    total.  Nobody widens the bound without this test noticing."""
    case = _case('mixed')
    iw, uw, uid, pos, neg, lr = case
    c = sr.coefficients(iw, uw, uid, pos, neg)
    it, us = sr.end_to_end(iw, uw, uid, pos, neg, lr, c, allow=_cpu_sigmoid_allowance())
    for chunk in (16, 64):
        r = _stage_a(case, chunk, mutant)
        worst = max(r['item'], r['user'])
        (ei, mi), (eu, mu) = sr.judge(it, r['w1'], iw), sr.judge(us, r['u1'], uw)
        print(f'{mutant} chunk {chunk}: error / Stage-A bound items {r["item"]:.3g} users {r["user"]:.3g}, rows moved that must not '
              f'{r["moved"]}; error / end-to-end bound {max(ei, eu):.3g}')
        if mutant == 'padding_row_moved':
            assert r['moved'] == 1 and mi == 1 and r['w1'][0].any()
        else:
            assert worst > 1.0, (mutant, chunk, r['item'], r['user'])
            assert max(ei, eu) > 1.0
        if mutant == 'duplicate_user_once':
            assert r['user'] > 1.0 and r['item'] <= 0.5
        if mutant in ('solo_twice', 'solo_skipped', 'drop_one_of_long_run', 'scale_per_partial'):
            assert r['item'] > 1.0 and r['user'] <= 0.5


# ------------------------------------------------------------------------------------------- the float-atomic forms' in-table term
IN_TABLE_CATALOGS = {'N97': 97, 'N600': 600, 'N1500': 1500}          # item runs of about 135, 22 and 9 elements; users 1 .. 10 times


def _shared_case(N, seed=3, d=32, M=200):
    """The GPU cases' 'shared' conditioning (weights of order 0.3, lr = M, uniform negatives, recurring users, padding ids, user 0)."""
    g = torch.Generator().manual_seed(seed)
    U, n = 60, 64
    pos = torch.randint(1, N, (M,), generator=g)
    neg = torch.randint(1, N, (M, n), generator=g)
    neg[::7, 3] = 0
    uid = torch.randint(1, U, (M,), generator=g)
    uid[9] = 0
    iw, uw = torch.randn(N, d, generator=g) * 0.3, torch.randn(U, d, generator=g) * 0.3
    iw[0] = 0
    uw[0] = 0
    return iw, uw, uid, pos, neg, float(M)


def _in_table(case, order_seed, mutant=None):
    iw, uw, uid, pos, neg, lr = case
    dpos, dneg, qg = sr.emulate_coefficients_fp32(iw, uw, uid, pos, neg)
    w1, u1 = sr.emulate_in_table_fp32(iw, uw, uid, pos, neg, dpos, dneg, qg, lr, order_seed=order_seed, mutant=mutant)
    out = {}
    for name, flag in (('plain', False), ('wide', True)):
        it = sr.item_update(iw, uw, uid, pos, neg, dpos, dneg, lr, in_table_atomics=flag)
        us = sr.user_update(uw, uid, qg, lr, in_table_atomics=flag)
        (ri, mi), (ru, mu) = sr.judge(it, w1, iw), sr.judge(us, u1, uw)
        out[name] = dict(item=ri, user=ru, moved=mi + mu, it=it, us=us)
    return out


@pytest.mark.parametrize('catalog', list(IN_TABLE_CATALOGS))
def test_in_table_accumulation_needs_its_term_and_stays_within_it(catalog):
    """The float-atomic forms add every element INTO the weight row: K roundings at the weight's magnitude, where Stage A's 2u |W'|
    allows for one read-modify-write.  An fp32 emulation of exactly that (row = fl(row + fl(fl(scale * d) * q)) element by
    element, in element order and in three shuffled orders: the order of atomics is free) at lr = M, against the plain
    Stage-A bound and against the one with the derived term (K - 2) u (|W| + |lr| A) of sgd_referee._finish:

    * runs of about 9 and about 22 elements (N = 1500, 600) are OUTSIDE the plain bound -- the sum is small against the weight, so
      (K + 2) u A does not cover K roundings of |W|; measured 2.3 and 2.9 times it -- and inside the bound with the term;
    * runs of more than fifty elements (N = 97, the GPU cases' sharing) sit inside both on the item rows: there (K + 2) u A has
      grown past K u |W|;
    * the term is a worst case of K roundings of u (|W| + |lr| A) each, no more: at K >= 8 the emulation is within HALF of the bound
      (measured 0.39 at N = 600, 0.09 at N = 97), with runs of 3 and more (N = 1500) it uses 0.83 of it -- three half-ulps of a row leave no factor two;
    * rows of K <= 2 get no term: there the two bounds are the same number."""
    case = _shared_case(IN_TABLE_CATALOGS[catalog])
    for order_seed in (None, 0, 1, 2):
        r = _in_table(case, order_seed)
        p, w = r['plain'], r['wide']
        print(f'in-table {catalog}, order {order_seed}: error / plain Stage-A bound items {p["item"]:.3f} users {p["user"]:.3f}; error / bound '
              f'with the in-table term items {w["item"]:.3f} users {w["user"]:.3f}; K items {int(w["it"]["K"].min())} .. {int(w["it"]["K"].max())} '
              f'users up to {int(w["us"]["K"].max())}')
        assert w['moved'] == 0 and w['item'] <= 1.0 and w['user'] <= 1.0
        if catalog != 'N97':
            assert p['item'] > 1.0, p['item']
        if catalog != 'N1500':
            assert int(w['it']['K'].min()) >= 8 and w['item'] <= 0.5
    assert sr.update_scale(w['it']) > 1e-3 and sr.update_scale(w['us']) > 1e-3
    few = w['us']['K'] <= 2
    assert bool(few.any()) and torch.equal(w['us']['tol'][few], p['us']['tol'][few]) and bool((w['us']['tol'][~few] > p['us']['tol'][~few]).all())


@pytest.mark.parametrize('mutant', sr.IN_TABLE_MUTANTS)
def test_every_planted_mistake_is_outside_the_bound_with_the_in_table_term(mutant):
    """The mistakes of order and bookkeeping the float-atomic forms can make -- the item pass reading post-update user rows, one
    element dropped from the longest run, one element added twice, a duplicated user's gradients applied once, the padding row
    moved -- land OUTSIDE the bound WITH the in-table term (or move a row that must not move) at N = 600 and at N = 97, in element
    order and in a shuffled one.  (The solo-row and per-partial mistakes of the sorted forms do not exist here: there is no
    forward update and no partial.)"""
    for catalog in ('N600', 'N97'):
        case = _shared_case(IN_TABLE_CATALOGS[catalog])
        for order_seed in (None, 1):
            r = _in_table(case, order_seed, mutant)['wide']
            print(f'in-table {catalog} {mutant}, order {order_seed}: error / bound with the in-table term items {r["item"]:.3g} users {r["user"]:.3g}, '
                  f'rows moved that must not {r["moved"]}')
            if mutant == 'padding_row_moved':
                assert r['moved'] == 1
            elif mutant == 'duplicate_user_once':
                assert r['user'] > 1.0 and r['item'] <= 0.5
            else:
                assert r['item'] > 1.0, (mutant, catalog, order_seed, r['item'])
