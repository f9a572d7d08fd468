"""The in-launch mean loss (reduce_mean_loss, rsa_common.hpp) of every caller -- the fused BPR epilogue (n = 64), the BPR walk
(n = 128, 320, 1024), the fused SampledSoftmax kernel, both home kernels (small: QPW 8 / 4 / 2, large) and the owner BPR walk --
against the float64 referee (tests/mean_referee.py) over its whole range, and the row arithmetic of the same kernels on adversarial
score gaps.

Launch sizes.  Every caller gives a workgroup ``rpw`` consecutive queries and strides over the rest: query m belongs to workgroup
(m // rpw) % grid, grid = min(ceil(B / rpw), cap).  From the host launch code: fused_fwd_kernel (n = 64: one tile per query, 4 waves)
and fused_ssm_kernel (one wave per query) rpw = 4; fused_bpr_walk_kernel rpw = 4 >> wpq_log2 = 2 (n = 128), 1 (n >= 256); the home
kernels rpw = 4 * QPW = 32 (n <= 64), 16 (n <= 128), 8 (n <= 256), 4 (above); cap = RSA_FWD_GRID_CAP = HOME_GRID_CAP = 2048.  B = rpw * g
gives g = 1, 31, 32, 33 workgroups, B = rpw + 1 two, and B = rpw * (cap + 1) runs the grid-stride loop at the capped grid (one such
case per kernel; for rpw = 4: B = 4, 5, 124, 128, 132 and 8196).

Bands of the mean (reference: the float64 mean of the referee's float64 rows).  The rows of bands (b) to (e) are exact in float32
(mean_referee.scores_for_rows: one negative at X >= 40, the others 5000 below the positive), so what is compared is the reduction:
  (a) all rows below 1e-6 (every negative 40 below the positive: rows of 4e-18 n)                      the mean within the bound
  (b) O(1) to O(10), several nonzero rows per workgroup                                                   the mean within the bound
  (c) just under 2^11 = the workgroups' shares add up to 2040 (one workgroup: 1020, under the share cap)  the mean within the bound
  (d) in [2^12, 2^10 grid): every share 1000, grids of 31 and more                                        the mean, or +inf
  (e) one workgroup's share 1500                                                                          +inf
  (f) one padded (-inf) positive, SampledSoftmax                                                          NaN
Bound of (a) - (d): grid * 2^-35 (the quantisation stated above reduce_mean_loss) + 2^-24 |ref| (the one fp32 rounding of the
result); where 1 / n is not a power of two (BPR, n = 7, 100, 200, 320) the rows themselves carry fl(1 / n) and one product, and a
workgroup's fp32 sum of r rows r - 1 additions: (r + 5) 2^-24 |ref| more.  After EVERY launch the flag word (byte 0) and the 33
reduction words (byte 256, 128 bytes apart) of ops._scratch() must be zero, and after (d), (e), (f) a band-(b) launch on the same
stream must return its own mean.  The two forms of a launch (with / without the query gradient) return bit-equal ``loss``.

Row values: row_loss, dpos, dneg of every caller on the sets of mean_referee (gaps, equal, dominant, trained; SampledSoftmax also
with log-probabilities in [-40, 0]), every element, NaN positions exactly, bound rtol |ref| + atol + 2 |torch_fp32 - ref| with
row_loss 1e-5 / 1e-7 and dpos, dneg 1e-4 / 1e-8 (the bounds test_gpu_round4.py / test_gpu_parity.py hold these outputs to);
torch_fp32 is the reference formula in torch fp32 ops on the same device.  The kernels' outputs enter no bound.

Measured on an MI355X, worst error / bound per kernel family (run with -s for every caller, size and band; 0.000 omitted):
  fused BPR (n = 64 and the walk)  mean (b) 0.286  (c) 0.016  (d) 0.096   row_loss gaps 0.009  trained 0.074   dpos, dneg <= 0.001
  fused SampledSoftmax             mean (b) 0.386  (c) 0.016  (d) 0.096   row_loss trained 0.374  trained+logQ 0.487  dominant+logQ 0.144
                                   dpos trained 0.346  trained+logQ 0.483   dneg gaps 0.373  gaps+logQ 0.238  equal+logQ 0.030
  home BPR (QPW 8 / 4 / 2, large)  mean (b) 0.348  (c) 0.260  (d) 0.662   row_loss equal 0.009  gaps 0.009  trained 0.074   dpos, dneg <= 0.001
  home SampledSoftmax              mean (b) 0.846  (c) 0.260  (d) 0.662   row_loss trained+logQ 0.485  dominant+logQ 0.344  gaps+logQ 0.119
                                   dpos trained+logQ 0.479  dominant+logQ 0.111   dneg gaps 0.410  gaps+logQ 0.410  equal+logQ 0.030
  owner BPR walk                   summed loss_part 0.75326252 / 1900.0 / +inf for a float64 mean of 0.75326252 / 1899.99990 / 39999.9998
Band (a) is a loss of exactly 0 for a float64 mean of 4e-18 n everywhere; (e) +inf and (f) NaN everywhere; no word was left in the
scratch by any launch.  No row-value case came near its bound: no kernel defect besides the one below.
With the word layout before this one (2^-38 fixed point, count at bit 50) band (d) failed for EVERY caller -- first at 31 workgroups
(fused n = 64 B = 124, walk B = 62 / 31, SampledSoftmax B = 124, home B = 992 / 496 / 248 / 124): the top word 0x009a460000000000 (or a
neighbour) was left in the scratch, and the launches after it in the process reported foreign losses -- and nothing else failed."""
import math

import numpy as np
import pytest
import torch

import mean_referee as mr
import owner_referee as orf

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
CAP = 2048                      # RSA_FWD_GRID_CAP, HOME_GRID_CAP (tests/test_mean_referee.py reads them from the host code)
QUANT = 2.0 ** -35              # per workgroup: "Quantisation: every share is rounded to nearest, <= grid * 2^-35 absolute"
U = 2.0 ** -24
TOL = {'row_loss': (1e-5, 1e-7), 'dpos': (1e-4, 1e-8), 'dneg': (1e-4, 1e-8)}
WORST = {}


@pytest.fixture(scope='module')
def ra():
    import recstudio_amd
    recstudio_amd._native.lib()
    return recstudio_amd


@pytest.fixture(scope='module')
def be(ra):
    from recstudio_amd.shard import HipBackend
    return HipBackend()


@pytest.fixture(autouse=True)
def clean_scratch(ra):
    """every test starts from zeroed words, so that words one test finds left behind (and reports) do not fail the tests after it"""
    ra.ops._scratch().zero_()
    torch.cuda.synchronize()


def _t(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(DEV)


# ---------------------------------------------------------------------------------------------------------- the callers
class Caller:
    """one kernel family at one n: ``run(scores, ...)`` launches it on float32 scores [B, 1 + n] and returns its outputs"""

    def __init__(self, kind, loss, n, qg=False, den_mult=1):
        self.kind, self.loss, self.n, self.qg, self.den_mult = kind, loss, n, qg, den_mult
        if kind == 'home':
            self.rpw = 4 * (8 if n <= 64 else 4 if n <= 128 else 2 if n <= 256 else 1)
        elif loss == 'bpr' and n != 64:
            T = n // 64
            self.rpw = 4 >> (2 if T >= 4 else 1 if T >= 2 else 0)
        else:
            self.rpw = 4
        self.name = f'{kind}-{loss}-n{n}' + ('-qg' if qg else '') + (f'-den{den_mult}B' if den_mult != 1 else '')

    def grid(self, B):
        return min(-(-B // self.rpw), CAP)

    def batch(self, g):
        return {1: self.rpw, 2: self.rpw + 1, 'cap': self.rpw * (CAP + 1)}.get(g) or self.rpw * g

    def den(self, B):
        return B * self.den_mult

    def run(self, ra, be, scores, pos_logp=None, neg_logp=None, live=None):
        B, n = scores.shape[0], self.n
        if self.kind == 'home':
            flat = _t(scores.reshape(-1))
            slot = np.arange(B * (n + 1), dtype=np.int32)               # identity: element e of the step sits in slot e
            if live is not None:
                slot = np.where(live.reshape(-1), slot, -1).astype(np.int32)
            return be.home(flat, _t(slot), B, n, loss=self.loss, pos_logp=None if pos_logp is None else _t(pos_logp),
                           neg_logp=None if neg_logp is None else _t(neg_logp), mean_den=self.den(B), want_scores=False, want_grad=True)
        table, query, pos, neg = mr.realise(scores)
        kw = dict(pos_ids=_t(pos), neg_ids=_t(neg), fused_loss=self.loss, want_query_grad=self.qg, mask_pad_pos=bool((pos == 0).any()))
        if pos_logp is not None:
            kw.update(pos_logp=_t(pos_logp), neg_logp=_t(neg_logp))
        return ra.ops.fused_forward(_t(table), _t(query), n, **kw)

    def reference(self, scores, pos_logp=None, neg_logp=None, live=None):
        B = scores.shape[0]
        lp, ln = (None, None) if live is None else (live[:, 0], live[:, 1:])
        if self.loss == 'bpr':
            return mr.bpr_rows(scores, mean_den=self.den(B), live_neg=ln, live_pos=lp)
        return mr.ssm_rows(scores, pos_logp, neg_logp, mean_den=self.den(B), live_neg=ln, live_pos=lp)


FUSED = [Caller('fused', 'bpr', 64), Caller('fused', 'bpr', 64, qg=True)] + \
        [Caller('fused', 'bpr', n, qg=qg) for n in (128, 320, 1024) for qg in (False, True)] + \
        [Caller('fused', 'ssm', n, qg=qg) for n in (64, 192) for qg in (False, True)]
HOME = [Caller('home', loss, n, den_mult=3 if n in (100, 256) else 1) for loss in ('bpr', 'ssm') for n in (7, 64, 100, 128, 200, 256, 320)]
CALLERS = FUSED + HOME
CAP_CASES = {'fused-bpr-n64', 'fused-bpr-n128-qg', 'fused-ssm-n64', 'fused-ssm-n192-qg', 'home-bpr-n7', 'home-ssm-n7', 'home-bpr-n320',
             'home-ssm-n320'}


def scratch_is_zero(ra):
    torch.cuda.synchronize()
    raw = ra.ops._scratch().cpu().numpy()
    flag = int(raw[0:4].view(np.uint32)[0])
    words = [int(raw[256 + 128 * k:256 + 128 * k + 8].view(np.uint64)[0]) for k in range(33)]
    return flag == 0 and not any(words), (flag, [hex(w) for w in words if w])


def _first_rows(c, B):
    wg = (np.arange(B) // c.rpw) % c.grid(B)
    return np.array([int(np.flatnonzero(wg == w)[0]) for w in range(c.grid(B))])


def band_rows(c, B, band):
    """the exact row values [B] of a band"""
    n, grid, den = c.n, c.grid(B), c.den(B)
    r = np.zeros(B)
    if band == 'b':
        if c.loss == 'bpr':
            r = max(2, -(-40 // n)) + (np.arange(B) % 3).astype(np.float64)
        else:
            r = np.where(np.arange(B) % 3 == 0, 40.0 + (np.arange(B) % 5), 0.0)
        return r
    first = _first_rows(c, B)
    if band == 'c':
        r[first] = mr.round_sig((2040.0 if grid >= 2 else 1020.0) / grid * den)
    elif band == 'd':
        r[first] = mr.round_sig(1000.0 * den)
    elif band == 'e':
        r[first] = mr.round_sig(1.0 * den) if c.loss == 'bpr' else 64.0
        r[first[grid // 2]] = mr.round_sig(1500.0 * den)
    return r


def mean_bound(c, B, ref):
    exact = c.loss == 'ssm' or (c.n & (c.n - 1)) == 0
    rows_per_wg = -(-B // c.grid(B))
    return c.grid(B) * QUANT + U * abs(ref) * (1 + (0 if exact else rows_per_wg + 5))


def launch_band(ra, be, c, B, band):
    """-> (loss, float64 reference mean, bound); asserts the words are zero after the launch"""
    if band == 'a':
        s = mr.tile_rows(mr.set_range(c.n, -40.0), B)
    else:
        s = mr.scores_for_rows(band_rows(c, B, band), c.n, c.loss)
    if band == 'f':
        s = mr.scores_for_rows(band_rows(c, B, 'b'), c.n, c.loss)
        s[B // 2, 0] = -np.inf
    out = c.run(ra, be, s)
    zero, left = scratch_is_zero(ra)
    assert zero, f'{c.name} B={B} band {band}: words left in the scratch {left}'
    rows = c.reference(s)[0]
    ref = math.fsum(rows) / c.den(B) if np.isfinite(rows).all() else float(np.sum(rows))
    if band in 'bcde':       # the rows are the wanted values: exactly, or (BPR, 1 / n no power of two) to fl(1 / n) and one product
        got = out['row_loss'].double().cpu().numpy()
        exact = c.loss == 'ssm' or (c.n & (c.n - 1)) == 0
        assert np.array_equal(got, rows) if exact else (np.abs(got - rows) <= 2 * U * rows).all(), f'{c.name} B={B} band {band}: rows'
    return float(out['loss']), ref, mean_bound(c, B, ref), out


def _note(key, ratio):
    WORST[key] = max(WORST.get(key, 0.0), ratio)


@pytest.mark.parametrize('c', CALLERS, ids=lambda c: c.name)
def test_mean_over_its_whole_range(ra, be, c):
    sizes = [1, 2, 31, 32, 33] + (['cap'] if c.name in CAP_CASES else [])
    for g in sizes:
        B = c.batch(g)
        grid = c.grid(B)
        assert grid == (CAP if g == 'cap' else g) and (g != 'cap' or B > CAP * c.rpw)
        for band in 'abcdef':
            if band == 'd' and grid * 1000.0 < 4096.0:
                continue                                   # [2^12, 2^10 grid) with every share below 2^10 needs 5 workgroups
            if band == 'f' and c.loss != 'ssm':
                continue                                   # a padded positive is NaN in SampledSoftmax only (+inf in BPR)
            loss, ref, bound, _ = launch_band(ra, be, c, B, band)
            what = f'{c.name} B={B} grid={grid} band ({band}): loss {loss!r}, float64 mean {ref!r}, bound {bound:.3e}'
            print(what + ('' if band in 'ef' else f', error / bound {abs(loss - ref) / bound:.3f}'))
            if band in 'abc':
                assert abs(loss - ref) <= bound, what
                _note((c.name, 'mean ' + band), abs(loss - ref) / bound)
                if band == 'a':
                    assert 0 < ref < 1e-6
                if band == 'c':
                    assert (2000 < ref < 2048) if grid >= 2 else (1000 < ref < 1024)
            elif band == 'd':
                assert 4096 <= ref < 1024 * grid
                assert loss == math.inf or abs(loss - ref) <= bound, what         # the mean or +inf, never another finite number
                if loss != math.inf:
                    _note((c.name, 'mean d'), abs(loss - ref) / bound)
            elif band == 'e':
                assert loss == math.inf, what
            else:
                assert math.isnan(loss) and math.isnan(ref), what
            if band in 'def':                               # an ordinary launch on the same stream returns its own mean
                loss, ref, bound, _ = launch_band(ra, be, c, B, 'b')
                assert abs(loss - ref) <= bound, f'after band ({band}): ' + what + f' -> then {loss!r} for {ref!r}'


@pytest.mark.parametrize('pair', [(a, b) for a in FUSED for b in FUSED if a.qg is False and b.qg and (a.loss, a.n) == (b.loss, b.n)],
                         ids=lambda p: p[0].name)
def test_both_forms_return_the_same_loss(ra, be, pair):
    plain, qg = pair
    for g in (2, 33):
        B = plain.batch(g)
        for band in 'bcd':
            if band == 'd' and g < 5:
                continue
            x, y = launch_band(ra, be, plain, B, band)[0], launch_band(ra, be, qg, B, band)[0]
            assert x == y, (plain.name, B, band, x, y)
    for sname, make in mr.SCORE_SETS.items():
        s = mr.tile_rows(make(plain.n), 37)
        a, b = plain.run(ra, be, s), qg.run(ra, be, s)
        assert torch.equal(a['loss'], b['loss']) and torch.equal(a['row_loss'], b['row_loss']), (plain.name, sname)


# ---------------------------------------------------------------------------------------------------------- row values
def torch_fp32_rows(c, s, pos_logp, neg_logp, live, den):
    """the reference formulas in torch fp32 ops on the device (the allowance of the bound, never the kernel's outputs)"""
    s = _t(s)
    pos, neg = s[:, 0], s[:, 1:]
    B, n = neg.shape
    ln = torch.ones_like(neg, dtype=torch.bool) if live is None else _t(live[:, 1:])
    lp = torch.ones_like(pos, dtype=torch.bool) if live is None else _t(live[:, 0])
    zero = torch.zeros((), device=DEV)
    if c.loss == 'bpr':
        x = pos[:, None] - neg
        keep = ln & lp[:, None]
        row = -(torch.where(keep, torch.nn.functional.logsigmoid(x), zero)).sum(1) / n
        dneg = torch.where(keep, torch.sigmoid(-x), zero) / (n * den)
        return row, -dneg.sum(1), dneg
    z_pos = pos - (0.0 if pos_logp is None else _t(pos_logp))
    z = neg - (0.0 if neg_logp is None else _t(neg_logp))
    z = torch.where(ln, z, torch.full_like(z, -math.inf))
    lse = torch.logsumexp(torch.cat([z_pos[:, None], z], 1), 1)
    row, dpos, dneg = lse - z_pos, (torch.exp(z_pos - lse) - 1.0) / den, torch.exp(z - lse[:, None]) / den
    dneg = torch.where(ln, dneg, zero)
    return torch.where(lp, row, zero), torch.where(lp, dpos, zero), torch.where(lp[:, None], dneg, zero)


def _drops(B, n):
    live = np.ones((B, 1 + n), dtype=bool)
    live[1, 1 + (n // 2)] = live[2, 1] = live[2, n] = live[5, 1 + n // 3] = False          # a few negatives
    live[4, 0] = False                                                                     # one positive
    return live


@pytest.mark.parametrize('c', CALLERS, ids=lambda c: c.name)
def test_rows_on_adversarial_scores(ra, be, c):
    B = 2 * c.rpw + 5
    sets = [(name, make(c.n), False) for name, make in mr.SCORE_SETS.items()]
    if c.loss == 'ssm':
        sets += [(name + '+logQ', make(c.n), True) for name, make in mr.SCORE_SETS.items()]
    for sname, rows, with_lq in sets:
        s = mr.tile_rows(rows, B)
        lqp, lqn = mr.ssm_logp(B, c.n) if with_lq else (None, None)
        live = _drops(B, c.n) if (c.kind == 'home' and sname.startswith(('gaps', 'dominant'))) else None
        if c.loss == 'ssm' and sname == 'equal':
            s[B - 1, 0] = -np.inf                                           # a padded positive among the rows: NaN, exactly there
        out = c.run(ra, be, s, lqp, lqn, live)
        zero, left = scratch_is_zero(ra)
        assert zero, (c.name, sname, left)
        ref = c.reference(s, lqp, lqn, live)
        t32 = torch_fp32_rows(c, s, lqp, lqn, live, float(c.den(B)))
        line = []
        for key, want, alt in zip(('row_loss', 'dpos', 'dneg'), ref, t32):
            got = out[key].double().cpu().numpy().reshape(want.shape)
            alt = alt.double().cpu().numpy().reshape(want.shape)
            nan = np.isnan(want)
            assert np.array_equal(np.isnan(got), nan), f'{c.name} {sname} {key}: NaN positions differ'
            fin = ~nan
            inf = fin & np.isinf(want)
            assert np.array_equal(got[inf], want[inf]), f'{c.name} {sname} {key}: infinities differ'
            fin &= ~inf
            rtol, atol = TOL[key]
            with np.errstate(invalid='ignore'):
                bound = rtol * np.abs(want[fin]) + atol + 2.0 * np.nan_to_num(np.abs(alt[fin] - want[fin]), nan=0.0, posinf=0.0)
            ratio = float((np.abs(got[fin] - want[fin]) / bound).max()) if fin.any() else 0.0
            line.append(f'{key} {ratio:.3f}')
            _note((c.name, sname + ' ' + key), ratio)
            assert ratio <= 1.0, f'{c.name} {sname} {key}: worst error / bound {ratio:.3f}'
        loss, want = float(out['loss']), ref[0]
        shares = np.bincount((np.arange(B) // c.rpw) % c.grid(B), weights=np.nan_to_num(want), minlength=c.grid(B)) / c.den(B)
        assert not 1000.0 < shares.max() < 1050.0                        # (which side of the share cap must not hang on fp32 rounding)
        if np.isnan(want).any():
            assert math.isnan(loss), (c.name, sname, loss)
        elif shares.max() >= 1024.0:                                     # rows in the thousands: a share of 2^10 and more saturates
            assert loss == math.inf, (c.name, sname, loss, shares.max())
        else:
            m = math.fsum(want) / c.den(B)
            # rows of fp32 arithmetic: each inside rtol |row| + atol of its float64 value (asserted above with the allowance)
            bound = c.grid(B) * QUANT + U * abs(m) * (B + 6) + (1e-5 * abs(m) + 1e-7) + 2.0 * abs(float(t32[0].double().sum()) / c.den(B) - m)
            assert abs(loss - m) <= bound, (c.name, sname, loss, m, bound)
        print(f'{c.name} {sname}: worst error / bound  ' + '  '.join(line))


# ---------------------------------------------------------------------------------------------------------- the owner BPR walk
def test_owner_bpr_walk_mean_in_every_band_it_can_reach(ra, be):
    """shared_small (2 owners, 8 queries, n = 64: 4 queries per workgroup, 2 workgroups per owner) with q_all scaled so that the
    float64 mean of the UNSHARDED step lands in band (b), (c) and (e); the owners' loss_part add up to it within owner_referee's
    Stage B bound plus the quantisation, or to +inf.  Band (d) needs 5 workgroups' worth of shares below 2^10: out of reach at 2."""
    from test_gpu_owner_step import LR, play_bpr
    step = orf.make_step(**orf.CASES['shared_small'], device=DEV)
    Q, n = step['Q'], step['n']
    allow = orf.allowances(DEV, Q, n)

    def scaled(cf):
        return dict(step, q_all=(step['q_all'] * cf).contiguous())

    def mean_at(cf):
        return float(orf.reference(scaled(cf), 'bpr', LR)['loss'])

    def scale_for(target):
        lo, hi = 1.0, 2.0
        while mean_at(hi) < target:
            hi *= 2.0
        for _ in range(24):
            mid = 0.5 * (lo + hi)
            lo, hi = (mid, hi) if mean_at(mid) < target else (lo, mid)
        return float(np.float32(lo))

    for band, target in (('b', None), ('c', 1900.0), ('e', 40000.0), ('b', None)):
        st = step if target is None else scaled(scale_for(target))
        ref = orf.reference(st, 'bpr', LR)
        out = play_bpr(be, st, False)
        zero, left = scratch_is_zero(ra)
        assert zero, (band, left)
        got = sum(float(oo['loss_part'].double()) for oo in out['owners'])
        want = float(ref['loss'])
        print(f'owner BPR walk band ({band}): summed loss_part {got!r}, float64 mean of the unsharded step {want!r}')
        if band == 'e':
            assert want > 2 * 2 * 1024 and got == math.inf
            continue
        tol = sum(t['tol_loss'] for t in orf.bpr_tolerances(st, ref, allow)) + len(out['owners']) * (2 * QUANT + U * want)
        assert abs(got - want) <= tol, (band, got, want, tol)
        _note(('owner-bpr-walk', 'mean ' + band), abs(got - want) / tol)
        if band == 'c':
            assert 1024 < want < 2048


def test_zz_report():
    """the worst error / bound per kernel and check, for the table in the module docstring (-s)"""
    names = sorted({k[0] for k in WORST})
    for name in names:
        print(name + ':  ' + '  '.join(f'{k[1]} {v:.3f}' for k, v in sorted(WORST.items()) if k[0] == name))
