"""The word layout of reduce_mean_loss (recstudio_amd/csrc/rsa_common.hpp) replayed in integers (tests/mean_referee.replay), for every
grid size at which the sub-word membership arithmetic differs and for the largest grid any caller launches, in random and
adversarial arrival orders: exactly one workgroup writes, the value is the float64 sum within the quantisation bound the comment
above the function states (or the documented saturation), and every word is zero afterwards.  The same model with the first
layout (2^-38 fixed point, count at bit 50) reproduces the defect that layout had: a wrong finite loss for a mean of 5000 over 256
workgroups, and a residue in the scratch that the following launches inherit.  No GPU."""
import math
import os
import re

import numpy as np
import pytest

import mean_referee as mr

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'recstudio_amd', 'csrc')

# the layout, restated: 2^-34 fixed point, count at bit 56, 32 sub-words, shares below 2^10 - 2^-35
FRAC_BITS, COUNT_SHIFT, SUBWORDS, SHARE_BITS = 34, 56, 32, 10
SHARE_CAP = 2.0 ** SHARE_BITS - 2.0 ** -(FRAC_BITS + 1)
NEW = mr.Layout(FRAC_BITS, COUNT_SHIFT, SHARE_CAP, SUBWORDS)
OLD = mr.Layout(38, 50, 1024.0, 32)          # the layout before: totals of 2^12 and more carried into the count


def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _const(text, name):
    m = re.search(r'\b' + name + r'\s*=\s*([0-9]+)\b', text)
    assert m, name
    return int(m.group(1))


def caller_grid_caps():
    """the grid caps of the callers of reduce_mean_loss, read from the host launch code"""
    m = re.search(r'#define\s+RSA_FWD_GRID_CAP\s+\(([0-9]+)\s*\*\s*([0-9]+)\)', _src('rsa_fused.hip'))
    assert m, 'RSA_FWD_GRID_CAP'
    caps = {'fused': int(m.group(1)) * int(m.group(2)),
            'home': _const(_src('rsa_shard.hip'), 'HOME_GRID_CAP'),
            'owner_walk': _const(_src('rsa_launch.hpp'), 'OWNER_WALK_GRID_CAP')}
    assert 'grid_1d(h.n_queries, 4 * qpw, HOME_GRID_CAP)' in _src('rsa_shard.hip')
    assert 'grid_1d(n_queries, 4 >> wpq_log2, OWNER_WALK_GRID_CAP)' in _src('rsa_launch.hpp')
    assert _src('rsa_fused.hip').count('RSA_FWD_GRID_CAP)), block(256)') == 3         # walk, ssm, fwd
    return caps


LARGEST_GRID = max(caller_grid_caps().values())
GRIDS = sorted({1, 2, 31, 32, 33, 64, 2048, LARGEST_GRID})


def test_restated_layout_is_the_header_s():
    h = _src('rsa_common.hpp')
    assert (_const(h, 'LOSS_FRAC_BITS'), _const(h, 'LOSS_COUNT_SHIFT'), _const(h, 'LOSS_SUBWORDS'), _const(h, 'LOSS_SHARE_BITS')) == \
        (FRAC_BITS, COUNT_SHIFT, SUBWORDS, SHARE_BITS)
    assert 'LOSS_SHARE_CAP = (double)(1 << LOSS_SHARE_BITS) - 1.0 / (double)(1ll << (LOSS_FRAC_BITS + 1))' in h
    assert '!(fabs(share) < LOSS_SHARE_CAP)' in h
    assert 'LOSS_MAX_GRID = SCRATCH_MAX_GRID' in h and _const(h, 'SCRATCH_MAX_GRID') >= LARGEST_GRID
    # the quantisation bound the tests use is the one the comment states
    assert 'Quantisation: every share is rounded to nearest, <= grid * 2^-35 absolute' in h
    assert NEW.quantisation(7) == 7 * 2.0 ** -35
    # capped shares of the largest grid cannot carry, and the counts fit
    assert LARGEST_GRID * (2 ** (FRAC_BITS + SHARE_BITS) - 1) < 2 ** COUNT_SHIFT
    assert math.ceil(LARGEST_GRID / SUBWORDS) < 2 ** (64 - COUNT_SHIFT) and SUBWORDS < 2 ** (64 - COUNT_SHIFT)
    assert int(round(math.nextafter(SHARE_CAP, 0.0) * 2.0 ** FRAC_BITS)) == 2 ** (FRAC_BITS + SHARE_BITS) - 1


def _orders(grid, shares, rng):
    big = int(np.nanargmax(np.where(np.isfinite(shares), shares, -1.0))) if grid else 0
    rest = [b for b in range(grid) if b != big]
    last_sub = (grid - 1) % SUBWORDS
    out = {'in order': list(range(grid)), 'reversed': list(range(grid - 1, -1, -1)),
           'one sub-word last': [b for b in range(grid) if b % SUBWORDS != last_sub] + [b for b in range(grid) if b % SUBWORDS == last_sub],
           'sub-word 0 last': [b for b in range(grid) if b % SUBWORDS != 0] + [b for b in range(grid) if b % SUBWORDS == 0],
           'largest share first': [big] + rest, 'largest share last': rest + [big]}
    for k in range(3):
        out[f'random {k}'] = [int(b) for b in rng.permutation(grid)]
    return out


def _share_sets(grid, rng):
    below_cap = math.nextafter(SHARE_CAP, 0.0)
    one_large = rng.random(grid)
    one_large[rng.integers(grid)] = 1023.9
    sets = {'zeros': np.zeros(grid), 'tiny': np.full(grid, 1e-12), 'O(1) mean': rng.random(grid) * 2.0 / grid,
            'mean 5000 or the cap': np.full(grid, min(5000.0 / grid, below_cap)), 'all at the cap': np.full(grid, below_cap),
            'one large': one_large, 'half ulps': (rng.integers(0, 1000, grid) + 0.5) * 2.0 ** -FRAC_BITS}
    over = rng.random(grid)
    over[rng.integers(grid)] = SHARE_CAP
    sets['one at the cap: +inf'] = over
    inf = rng.random(grid)
    inf[rng.integers(grid)] = np.inf
    sets['one inf'] = inf
    nan = rng.random(grid)
    nan[rng.integers(grid)] = np.nan
    if grid > 1:
        nan[(int(np.flatnonzero(np.isnan(nan))[0]) + 1) % grid] = 5000.0       # NaN wins over +inf
    sets['one NaN'] = nan
    return sets


@pytest.mark.parametrize('grid', GRIDS)
def test_one_writer_right_value_zero_words(grid):
    rng = np.random.default_rng(grid)
    for sname, shares in _share_sets(grid, rng).items():
        want_nan = bool(np.isnan(shares).any())
        want_inf = not want_nan and bool((~(np.abs(shares) < SHARE_CAP)).any())
        total = None if (want_nan or want_inf) else mr.exact_sum(shares)
        values = set()
        for oname, order in _orders(grid, shares, rng).items():
            assert sorted(order) == list(range(grid))
            out = mr.replay(NEW, shares, order)
            what = f'grid {grid}, shares {sname}, order {oname}'
            assert len(out['writes']) == 1, what                              # exactly one workgroup writes
            wg, loss = out['writes'][0]
            assert wg == order[-1] or grid > SUBWORDS, what                   # (two levels: the last of the last sub-word)
            assert mr.words_are_zero(out['words']), what
            if want_nan:
                assert np.isnan(loss), what
            elif want_inf:
                assert np.isposinf(loss), what
            else:
                # quantisation (comment of reduce_mean_loss) + the one fp32 rounding of the result
                bound = NEW.quantisation(grid) + 2.0 ** -24 * total
                assert abs(float(loss) - total) <= bound, (what, float(loss), total, bound)
                values.add(float(loss))
        assert len(values) <= 1, (grid, sname, values)                        # integer addition: the order does not matter


def test_consecutive_launches_share_the_words():
    """the scratch block lives as long as the process: a saturated launch leaves nothing for the next one"""
    words = mr.fresh_words(NEW)
    rng = np.random.default_rng(5)
    for grid, mean in ((256, 3000.0), (256, 5000.0), (33, 20000.0), (2048, np.inf), (31, np.nan), (LARGEST_GRID, 1023.0 * LARGEST_GRID), (256, 0.7)):
        shares = np.full(grid, mean / grid)
        out = mr.replay(NEW, shares, [int(b) for b in rng.permutation(grid)], words)
        assert len(out['writes']) == 1 and mr.words_are_zero(words), (grid, mean)
        loss = float(out['writes'][0][1])
        if np.isfinite(mean):
            assert abs(loss - mean) <= NEW.quantisation(grid) + 2.0 ** -24 * mean, (grid, mean, loss)
        else:
            assert (np.isnan(loss) and np.isnan(mean)) or loss == mean


def test_first_layout_wrote_a_wrong_finite_loss_and_left_a_residue():
    """256 workgroups, equal shares, arrivals in order, launches on one scratch block: the layout before this one (2^-38, count at
    bit 50) is right at a mean of 3000, writes 747.75 for a mean of 5000 (the total passes 2^50, carries into the count, workgroup
    254 takes itself for the last of the top word) and leaves the true last arrival's words behind; the next launch then reports
    156.93 for 0.7.  The current layout reports every mean and leaves zeros."""
    grid = 256
    means = (3000.0, 5000.0, 0.7, 0.7, 0.7)
    words, got, residue = mr.fresh_words(OLD), [], []
    for mean in means:
        out = mr.replay(OLD, np.full(grid, mean / grid), None, words)
        got.append([float(v) for _, v in out['writes']])
        residue.append(not mr.words_are_zero(words))
    assert got[0] == [3000.0] and not residue[0]
    assert len(got[1]) == 1 and abs(got[1][0] - 747.75) < 0.01 and residue[1]                  # finite and wrong
    assert len(got[2]) == 1 and abs(got[2][0] - 156.93) < 0.01 and residue[2]                  # inherited
    assert all(len(g) == 1 and np.isfinite(g[0]) for g in got[3:]) and all(residue[3:])       # the residue never leaves
    words = mr.fresh_words(NEW)
    for mean in means:
        out = mr.replay(NEW, np.full(grid, mean / grid), None, words)
        assert len(out['writes']) == 1 and mr.words_are_zero(words)
        assert abs(float(out['writes'][0][1]) - mean) <= NEW.quantisation(grid) + 2.0 ** -24 * mean


def test_referee_rows_carry_the_kernels_semantics():
    s = np.array([[0.0, 1.0, -1.0, 2.0], [-np.inf, 0.0, 0.0, 0.0], [1.0, 1.0, 1.0, 1.0]])
    live_neg = np.array([[True, False, True], [True, True, True], [True, True, True]])
    live_pos = np.array([True, True, False])
    row, dpos, dneg = mr.bpr_rows(s, mean_den=6, live_neg=live_neg, live_pos=live_pos)
    sp = lambda x: math.log1p(math.exp(x))
    assert abs(row[0] - (sp(1.0) + sp(2.0)) / 3) < 1e-15 and dneg[0, 1] == 0.0                # a dropped negative: the 1 / n stays
    assert abs(dneg[0, 0] - 1 / (1 + math.exp(-1.0)) / 18) < 1e-17 and abs(dpos[0] + dneg[0].sum()) < 1e-17
    assert row[2] == 0.0 and dpos[2] == 0.0 and not dneg[2].any()                             # a dropped positive
    row, dpos, dneg = mr.ssm_rows(s, mean_den=6, live_neg=live_neg, live_pos=live_pos)
    assert abs(row[0] - math.log(1 + math.e + math.e ** 2)) < 1e-15 and dneg[0, 1] == 0.0
    assert abs(dpos[0] - (1 / (1 + math.e + math.e ** 2) - 1) / 6) < 1e-15
    assert np.isnan(row[1]) and np.isnan(dpos[1]) and np.isnan(dneg[1]).all()                 # a padded positive
    assert row[2] == 0.0 and dpos[2] == 0.0 and not dneg[2].any()
    lp, ln = np.array([-1.0, 0.0, 0.0]), np.full((3, 3), -2.0)
    row, _, _ = mr.ssm_rows(s[[0]], pos_logp=lp[[0]], neg_logp=ln[[0]])
    assert abs(row[0] - (math.log(math.e + math.e ** 3 + math.e + math.e ** 4) - 1.0)) < 1e-14


def test_realised_scores_are_exact_and_the_sets_are_what_they_say():
    for name, make in mr.SCORE_SETS.items():
        for n in (7, 64, 200):
            s = mr.tile_rows(make(n), 10)
            table, query, pos, neg = mr.realise(s)
            assert table.shape[1] == mr.REALISE_DIM and (pos >= 1).all() and (neg >= 1).all()
            got = np.concatenate([(query * table[pos]).sum(1)[:, None], np.einsum('bd,bnd->bn', query, table[neg])], 1)
            assert got.dtype == np.float32 and np.array_equal(got, s), name
    g = mr.set_gaps(64)
    assert (g[:, 0] == 0).all() and {abs(float(v)) for v in g[0, 1:]} == set(float(np.float32(v)) for v in mr.GAP_VALUES)
    s = mr.set_range(64, 2047.0)
    s[0, 0] = -np.inf
    assert mr.realise(s)[2][0] == 0
    # exact rows: the float64 referee returns the wanted values bit for bit
    want = np.array([0.0, 2.0, 3.5, 1000.0 * 8196])
    assert np.array_equal(mr.bpr_rows(mr.scores_for_rows(want, 64, 'bpr'))[0], want)
    want = np.array([0.0, 40.0, 64.0, 1000.0 * 8196])
    assert np.array_equal(mr.ssm_rows(mr.scores_for_rows(want, 192, 'ssm'))[0], want)
    assert mr.round_sig(8196 * 1000.0 / 3) * 1024 == float(np.float32(mr.round_sig(8196 * 1000.0 / 3) * 1024))
