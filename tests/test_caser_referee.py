"""CPU: the float64 referee of Caser's convolutions (tests/caser_referee.py) judged on itself -- an fp32 emulation of a fused
kernel's order of operations inside half its bounds, thirteen seeded mistakes outside them, the exact-tie constructions.  No device
kernel runs here.  Measured: see test_fp32_emulation_stays_within_half_of_every_bound's docstring."""
import functools

import pytest
import torch

import caser_referee as cr

# (B, L, d, n_v, n_h, kind, seed)
CASES = [(5, 9, 32, 4, 16, 'whole', 1), (4, 9, 32, 4, 16, 'const', 2), (3, 17, 32, 2, 16, 'suffix', 3), (2, 5, 64, 8, 32, 'full', 4)]


@functools.lru_cache(maxsize=None)
def judged(case):
    B, L, d, n_v, n_h, kind, seed = case
    c = cr.make_case(B, L, d, n_v, n_h, seed=seed, kind=kind)
    args = (c['rows'], c['w_v'], c['b_v'], c['w_h'], c['b_h'])
    fwd = cr.forward(*args)
    o32, idx32, grads32 = cr.emulate_fp32(*args, c['g'])
    bwd = cr.backward(c['rows'], c['w_v'], c['w_h'], idx32, c['g'])
    exact = cr.exact_idx(fwd)
    return dict(c=c, args=args, fwd=fwd, o32=o32, idx32=idx32, grads32=grads32, bwd=bwd, exact=exact,
                bwd_exact=cr.backward(c['rows'], c['w_v'], c['w_h'], exact, c['g']))


@pytest.mark.parametrize('case', CASES, ids=str)
def test_fp32_emulation_stays_within_half_of_every_bound(case):
    """Measured (worst over the four cases): o 0.23, drows 0.19, dw_v 0.02, db_v 0.01, dw_h 0.45, db_h 0.25 of the bound; the
    emulation's idx is valid everywhere and equals the float64 argmax in all four.  dw_h is the largest because its sums have one
    or two terms here (B <= 5): one rounding against a bound of 3 u; the others are small because the (n + 2) u sum |terms| rule
    is a worst case over n roundings of one sign."""
    j = judged(case)
    ratios = dict(o=cr.worst_ratio(j['o32'], j['fwd']['o'], j['fwd']['tol_o']))
    for name in cr.GRADS:
        ratios[name] = cr.worst_ratio(j['grads32'][name], j['bwd'][name], j['bwd']['tol_' + name])
    differ = int((j['idx32'] != j['exact']).sum())
    print(case, {k: round(v, 3) for k, v in ratios.items()}, 'idx differs from the float64 argmax at', differ, 'of', j['exact'].numel())
    assert max(ratios.values()) <= 0.5, ratios
    assert not cr.idx_violations(j['idx32'], j['fwd']).any()
    assert not cr.tie_checks(j['idx32'], j['c'])


def test_the_tie_constructions_fire_both_ways():
    """The padded-whole sequence has filters on both sides of 0, the constant one active and inactive filters, and suffix-padded
    sequences point at their first all-zero window somewhere."""
    j = judged(CASES[0])
    idx, c = j['idx32'].long(), j['c']
    assert not c['rows'][0].any() and (idx[0] == 0).any() and (idx[0] == 255).any()
    assert torch.equal(idx[0] == 0, c['b_h'] > 0)
    hits = sum(int(((idx[b] == int(c['lengths'][b])) & (c['lengths'][b] > 0)).sum()) for b in range(1, idx.shape[0])
               if c['lengths'][b] < idx.shape[1])
    assert hits > 0
    k = judged(CASES[1])
    assert set(k['idx32'][0].unique().tolist()) == {0, 255}
    assert not cr.tie_checks(j['exact'], c) and not cr.idx_violations(j['exact'], j['fwd']).any()


def _leaves(diff, tol):
    return bool((diff.abs() > tol).any())


@pytest.mark.parametrize('mistake', cr.FORWARD_MISTAKES)
@pytest.mark.parametrize('case', CASES[:3], ids=str)
def test_forward_mistakes_leave_the_bounds(case, mistake):
    j = judged(case)
    wrong = cr.forward(*j['args'], mistake=mistake)
    assert _leaves(wrong['o'] - j['fwd']['o'], j['fwd']['tol_o']), mistake


@pytest.mark.parametrize('mistake', cr.IDX_MISTAKES)
@pytest.mark.parametrize('case', CASES[:2], ids=str)
def test_idx_mistakes_are_caught(case, mistake):
    """A gradient sent to the LAST maximal window (on the tie constructions, where there are several) or passed at a maximum <= 0:
    the idx is refused as such, the tie checks fail for the former, and the gradients taken from it leave the bounds of the
    gradients from the valid idx."""
    j = judged(case)
    c = j['c']
    idx = cr.last_max_idx(j['fwd']) if mistake == 'grad_to_last_max' else cr.exact_idx(j['fwd'], pass_nonpositive=True)
    assert (idx != j['exact']).any()
    assert cr.idx_violations(idx, j['fwd']).any() or cr.tie_checks(idx, c)
    if mistake == 'grad_to_last_max':
        assert cr.tie_checks(idx, c)
    wrong = cr.backward(c['rows'], c['w_v'], c['w_h'], idx, c['g'])
    good = j['bwd_exact']
    assert any(_leaves(wrong[n] - good[n], good['tol_' + n]) for n in ('drows', 'dw_h', 'db_h')), mistake


@pytest.mark.parametrize('mistake', cr.BACKWARD_MISTAKES)
@pytest.mark.parametrize('case', CASES[:3], ids=str)
def test_backward_mistakes_leave_the_bounds(case, mistake):
    j = judged(case)
    c = j['c']
    wrong = cr.backward(c['rows'], c['w_v'], c['w_h'], j['exact'], c['g'], mistake=mistake)
    name = {'dE_at_tstar_only': 'drows', 'dWh_from_E_tstar': 'dw_h', 'dbh_over_inactive': 'db_h', 'dE_without_vertical': 'drows'}[mistake]
    good = j['bwd_exact']
    assert _leaves(wrong[name] - good[name], good['tol_' + name]), mistake


def test_thirteen_mistakes_are_seeded():
    assert len(cr.FORWARD_MISTAKES) + len(cr.IDX_MISTAKES) + len(cr.BACKWARD_MISTAKES) == 13
