"""Plain float64 referee of the in-launch mean loss (reduce_mean_loss, recstudio_amd/csrc/rsa_common.hpp) and of the row
arithmetic of its callers.  numpy only, no GPU.

  * ``bpr_rows`` / ``ssm_rows``: row_loss, dpos, dneg of BPRLoss (loss_func.py:55-59) and of SampledSoftmaxLoss with one
    positive (:80-90) in float64, with the kernels' stated semantics for padded and dropped elements.
  * ``realise``: an item table, query rows and ids whose inner products ARE a wanted float32 score matrix (d = 32, query rows
    e_0, item row i = v_i * e_0: one exact product, then additions of zeros), so no dot-product rounding enters a comparison.
  * named score sets (``SCORE_SETS``, ``ssm_logp``), a few rows each, tiled up to a batch.
  * ``Layout`` / ``replay``: an integer model of the reduction protocol -- the word layout is a parameter, the arrival order is
    the caller's -- that reports the loss written, which workgroup wrote it, and the words left behind.
"""
import math
from dataclasses import dataclass

import numpy as np

NEG_FAR = -5000.0        # a negative this far below the positive contributes exactly 0 to either loss, in float32 and in float64


# ---------------------------------------------------------------------------------------------------------- row losses
def _logsigmoid(x):
    with np.errstate(over='ignore', invalid='ignore'):
        return np.minimum(x, 0.0) - np.log1p(np.exp(-np.abs(x)))


def _sigmoid(x):
    with np.errstate(over='ignore', invalid='ignore'):
        e = np.exp(-np.abs(x))
        return np.where(x >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def _live(scores, live_neg, live_pos):
    s = np.asarray(scores, dtype=np.float64)
    B, n = s.shape[0], s.shape[1] - 1
    ln = np.ones((B, n), dtype=bool) if live_neg is None else np.asarray(live_neg, dtype=bool)
    lp = np.ones(B, dtype=bool) if live_pos is None else np.asarray(live_pos, dtype=bool)
    return s[:, 0], s[:, 1:], ln, lp, B, n


def bpr_rows(scores, mean_den=None, live_neg=None, live_pos=None):
    """scores [B, 1 + n] (column 0: the positive) -> float64 row_loss [B], dpos [B], dneg [B, n] of
         row = -(1/n) sum_j logsigmoid(pos - neg_j),   loss = sum(row) / mean_den
    A dropped negative (``live_neg`` false) leaves the sums and the 1/n stays; a dropped positive (``live_pos`` false, home
    kernels) gives row 0 and zero gradients.  A -inf positive gives +inf, as the formula does."""
    pos, neg, ln, lp, B, n = _live(scores, live_neg, live_pos)
    M = float(B if mean_den is None else mean_den)
    x = pos[:, None] - neg
    keep = ln & lp[:, None]
    with np.errstate(invalid='ignore'):
        row = -np.where(keep, _logsigmoid(x), 0.0).sum(1) / n
        dneg = np.where(keep, _sigmoid(-x), 0.0) / (n * M)
    return row, -dneg.sum(1), dneg


def ssm_rows(scores, pos_logp=None, neg_logp=None, mean_den=None, live_neg=None, live_pos=None):
    """SampledSoftmaxLoss with one positive: z = score - logQ, row = logsumexp(z_pos, z_1 .. z_n) - z_pos,
    dneg_j = softmax_j / mean_den, dpos = (softmax_pos - 1) / mean_den.  A padded (-inf) positive gives NaN (row, dpos and the
    gradient of every live negative: the reference divides 0 by 0); a dropped negative leaves the sums (gradient 0); a dropped
    positive gives row 0 and zero gradients."""
    pos, neg, ln, lp, B, n = _live(scores, live_neg, live_pos)
    M = float(B if mean_den is None else mean_den)
    z_pos = pos - (0.0 if pos_logp is None else np.asarray(pos_logp, dtype=np.float64))
    z = neg - (0.0 if neg_logp is None else np.asarray(neg_logp, dtype=np.float64))
    z = np.where(ln, z, -np.inf)
    bad = np.isinf(z_pos)
    zp = np.where(bad, 0.0, z_pos)
    zz = np.concatenate([zp[:, None], z], 1)
    at = zz.argmax(1)
    top = zz[np.arange(B), at]
    with np.errstate(invalid='ignore', over='ignore'):
        e = np.exp(zz - top[:, None])
        e[np.arange(B), at] = 0.0                      # the largest term is exactly 1: log1p of the others keeps rows far below 2^-53
        lse = top + np.log1p(e.sum(1))
        row = (top - zp) + np.log1p(e.sum(1))
        dneg = np.exp(z - lse[:, None]) / M
        dpos = -dneg.sum(1)                            # == (softmax_pos - 1) / M without the cancellation
    row, dpos = np.where(bad, np.nan, row), np.where(bad, np.nan, dpos)
    dneg = np.where(ln, np.where(bad[:, None], np.nan, dneg), 0.0)
    gone = ~lp
    return np.where(gone, 0.0, row), np.where(gone, 0.0, dpos), np.where(gone[:, None], 0.0, dneg)


# ---------------------------------------------------------------------------------------------------------- scores -> embeddings
REALISE_DIM = 32


def realise(scores):
    """float32 scores [B, 1 + n] -> (item_table [V, 32] f32, query [B, 32] f32, pos_ids [B] i64, neg_ids [B, n] i64) with
    <query[b], item_table[id]> == the wanted score, exactly: query rows are e_0, item row i is v_i * e_0.  Row 0 of the table is
    the padding row; a -inf positive becomes pos id 0 (launch with mask_pad_pos), every other id is >= 1."""
    s = np.asarray(scores)
    assert s.dtype == np.float32 and s.ndim == 2
    pad = np.isneginf(s[:, 0])
    assert np.isfinite(s[:, 1:]).all() and np.isfinite(s[~pad, 0]).all()
    vals, inv = np.unique(np.where(np.isfinite(s), s, np.float32(0)), return_inverse=True)
    ids = inv.reshape(s.shape).astype(np.int64) + 1
    table = np.zeros((vals.size + 1, REALISE_DIM), dtype=np.float32)
    table[1:, 0] = vals
    query = np.zeros((s.shape[0], REALISE_DIM), dtype=np.float32)
    query[:, 0] = 1.0
    pos_ids = np.where(pad, 0, ids[:, 0])
    return table, query, pos_ids, np.ascontiguousarray(ids[:, 1:])


# ---------------------------------------------------------------------------------------------------------- named score sets
GAP_VALUES = (0.0, 2.0 ** -20, 1.0, 10.0, 17.0, 30.0, 87.0, 89.0, 104.0, 5000.0)


def _cycle(values, n, start):
    v = np.asarray(values, dtype=np.float32)
    return v[(start + np.arange(n)) % v.size]


def set_gaps(n):
    """pos = 0; the negatives cycle through +-{0, 2^-20, 1, 10, 17, 30, 87, 89, 104, 5000} (three rotations)"""
    cyc = [s * g for g in GAP_VALUES for s in (1.0, -1.0)]
    rows = [np.concatenate([[np.float32(0)], _cycle(cyc, n, st)]) for st in (0, 7, 13)]
    return np.stack(rows).astype(np.float32)


def set_equal(n):
    """pos = every negative = c, c in {0, 50, -50}"""
    return np.stack([np.full(1 + n, c, dtype=np.float32) for c in (0.0, 50.0, -50.0)])


def set_dominant(n):
    """one negative at pos + 40 (first, middle, last place), the rest at pos - 40"""
    out = []
    for pos, at in ((3.0, 0), (-2.5, n // 2), (0.0, n - 1)):
        r = np.full(1 + n, pos - 40.0, dtype=np.float32)
        r[0], r[1 + at] = pos, pos + 40.0
        out.append(r)
    return np.stack(out)


def set_trained(n):
    """every negative at pos - g, g in {8, 16, 24}"""
    out = []
    for pos, g in ((1.5, 8.0), (-3.0, 16.0), (12.0, 24.0)):
        r = np.full(1 + n, pos - g, dtype=np.float32)
        r[0] = pos
        out.append(r)
    return np.stack(out)


def set_range(n, X, pos=0.0):
    """every negative at pos + X"""
    r = np.full((1, 1 + n), pos + X, dtype=np.float32)
    r[0, 0] = pos
    return r


SCORE_SETS = {'gaps': set_gaps, 'equal': set_equal, 'dominant': set_dominant, 'trained': set_trained}


def tile_rows(rows, B):
    """a few rows tiled up to B rows"""
    rows = np.asarray(rows)
    return np.ascontiguousarray(rows[np.arange(B) % rows.shape[0]])


def ssm_logp(B, n):
    """log-probabilities in [-40, 0] for the SampledSoftmax variants of the sets -> (pos_logp [B], neg_logp [B, n]) float32:
    with scores spanning +-40, z = score - logQ spans about +-80"""
    cyc = np.asarray([0.0, -40.0, -20.0, -1.0, -39.5, -7.25, -30.0, -0.5, -13.0], dtype=np.float32)
    b = np.arange(B)
    neg = cyc[(b[:, None] * 5 + np.arange(n)[None, :] * 2) % cyc.size]
    return np.ascontiguousarray(cyc[(b * 4 + 1) % cyc.size]), np.ascontiguousarray(neg)


def scores_for_rows(row_values, n, loss):
    """float32 scores whose row losses are EXACTLY ``row_values`` (each 0 or >= 40 / n for 'bpr', 0 or >= 40 for 'ssm', with at
    most 12 significant bits), in float32 as in float64: pos = 0, one negative at X and the others at NEG_FAR, where their term
    is exactly 0 -- BPR: row = softplus(X) / n = X / n for X >= 40 (log1p(exp(-40)) is below half an ulp of 40 in either format);
    SampledSoftmax without log-probabilities: row = log(exp(X) + 1 + ...) - 0 = X."""
    r = np.asarray(row_values, dtype=np.float64)
    X = r * n if loss == 'bpr' else r
    assert ((X == 0) | (X >= 40)).all()
    assert (X.astype(np.float32).astype(np.float64) == X).all()
    s = np.full((r.size, 1 + n), NEG_FAR, dtype=np.float32)
    s[:, 0] = 0.0
    s[:, 1] = np.where(X > 0, X, NEG_FAR).astype(np.float32)
    return s


def round_sig(x, bits=12):
    """x rounded to ``bits`` significant bits (so that x * n stays exact in float32 for n <= 1024)"""
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(divide='ignore'):
        e = np.where(x > 0, np.floor(np.log2(np.where(x > 0, x, 1.0))), 0.0)
    q = 2.0 ** (e - (bits - 1))
    return np.where(x > 0, np.round(x / q) * q, 0.0)


# ---------------------------------------------------------------------------------------------------------- the reduction protocol
@dataclass(frozen=True)
class Layout:
    """The word layout of reduce_mean_loss: a share is rounded to a multiple of 2^-frac_bits, the sum sits in bits
    0 .. count_shift - 1 of a 64-bit word and the arrival count above it; workgroup b adds to sub-word b % subwords; a share
    at or above share_cap (or NaN / inf) goes through the flag word instead (bit 0: NaN, bit 1: out of range)."""
    frac_bits: int
    count_shift: int
    share_cap: float
    subwords: int = 32

    def quantisation(self, grid):
        return grid * 2.0 ** -(self.frac_bits + 1)


MASK64 = (1 << 64) - 1


def fresh_words(layout):
    return {'flag': 0, 'top': 0, 'sub': [0] * layout.subwords}


def replay(layout, shares, order=None, words=None):
    """One launch of ``len(shares)`` workgroups arriving in ``order`` (a permutation of the workgroup indices; default 0, 1, ..),
    on the scratch ``words`` (default: zeroed; modified in place).  Every workgroup's tail is atomic here: the kernel's flag-or,
    add to the sub-word, reset, add to the top word are dependent steps of ONE thread, and every decision is taken on the value
    an atomic returned, so an interleaving of two tails decides as the order of their atomics on each word does.
    -> dict(writes=[(workgroup, float32 loss), ..], words=the scratch afterwards)."""
    grid = len(shares)
    words = fresh_words(layout) if words is None else words
    field, one = (1 << layout.count_shift) - 1, 1 << layout.count_shift
    n_sub = min(grid, layout.subwords)
    writes = []
    for b in (range(grid) if order is None else order):
        share = float(shares[b])
        bad = not (abs(share) < layout.share_cap)              # NaN, inf or out of the fixed-point range
        fixed = 0 if bad else int(round(share * 2.0 ** layout.frac_bits))      # round half to even, as __double2ll_rn
        add = (fixed & field) + one
        if bad:
            words['flag'] |= 1 if share != share else 2
        j = b % layout.subwords
        members = (grid - j + layout.subwords - 1) // layout.subwords
        prev = words['sub'][j]
        words['sub'][j] = (prev + add) & MASK64
        if (prev >> layout.count_shift) == members - 1:
            sub_total = (prev + add) & field
            words['sub'][j] = 0
            add2 = sub_total + one
            prev2 = words['top']
            words['top'] = (prev2 + add2) & MASK64
            if (prev2 >> layout.count_shift) == n_sub - 1:
                total = (prev2 + add2) & field
                loss = np.float32(total / 2.0 ** layout.frac_bits)
                flags = words['flag']
                if flags & 1:
                    loss = np.float32(np.nan)
                elif flags & 2:
                    loss = np.float32(np.inf)
                writes.append((b, loss))
                words['top'] = 0
                if flags:
                    words['flag'] = 0
    return dict(writes=writes, words=words)


def words_are_zero(words):
    return words['flag'] == 0 and words['top'] == 0 and not any(words['sub'])


def exact_sum(shares):
    return math.fsum(float(s) for s in shares)
