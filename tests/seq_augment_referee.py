"""Exact referee of one augmented view of a batch of histories (rsa_seq_augment / ops.seq_augment,
data_augmentation.seq_augment_torch): a plain per-sequence restatement of the rule in Python / numpy, independent of the batched
twin.  Integer work; the one piece of arithmetic is the fp32 product of the start, taken with numpy float32.

    len = clamp(seqlen[b], 0, L)      n_sub = sub[len]      span = max(len - n_sub + 1, 1)
    start = min(int(float32(U[b, 0]) * float32(span)), span - 1)
    crop    : out[p] = seq[start + p] for p < n_sub, else 0;                                       new_len = n_sub
    mask    : positions p < len ranked by (U[b, 1 + p], p); mask_id where the rank is below n_sub;  new_len = len
    reorder : positions of [start, start + n_sub) ranked among themselves the same way;
              out[start + rank(p)] = seq[p], everything else copied;                               new_len = len
    a row with len = 0 comes back unchanged with new_len = 0.

``sub_lengths`` restates the table len -> n_sub in Python float64 with the reference's expressions
(recstudio/model/module/data_augmentation.py:36, :59, :80).

Every rule takes ``mistake=`` naming one seeded mistake (tests/test_seq_augment_referee.py shows each of them leaves equality).
"""
import numpy as np

KINDS = ('crop', 'mask', 'reorder')
MISTAKES = ('ties_high', 'padded_keys', 'no_clamp', 'inverse_perm', 'crop_keeps_len', 'mask_all_L')


def sub_lengths(kind, rate, L, fp32=False):
    """[n_sub(0), ..., n_sub(L)].  ``fp32``: the seeded mistake of taking ``rate * n`` in fp32."""
    def prod(n):
        return float(np.float32(rate) * np.float32(n)) if fp32 else rate * n
    if kind == 'crop':
        return [0] + [max(1, int(prod(n))) for n in range(1, L + 1)]
    assert kind in ('mask', 'reorder')
    return [0] + [int(prod(n)) for n in range(1, L + 1)]


def _ranks(keys, positions, ties_high=False):
    """rank of every position of ``positions`` by (key, position): {position: rank}."""
    order = sorted(positions, key=lambda q: (keys[q], -q if ties_high else q))
    return {q: r for r, q in enumerate(order)}


def augment_row(row, seqlen, kind, sub, u, mask_id=0, mistake=None):
    """One sequence: ``row`` [L] ints, ``u`` [L + 1] float32 -> (out [L] list, new_len)."""
    assert kind in KINDS and (mistake is None or mistake in MISTAKES)
    L = len(row)
    ln = min(max(int(seqlen), 0), L)
    n_sub = int(sub[ln])
    if ln == 0:
        return [int(x) for x in row], 0
    span = max(ln - n_sub + 1, 1)
    start = int(np.float32(u[0]) * np.float32(span))
    if mistake != 'no_clamp':
        start = min(start, span - 1)
    keys = [float(x) for x in u[1:]]
    if kind == 'crop':
        out = [int(row[start + p]) if p < n_sub and start + p < L else 0 for p in range(L)]
        return out, (ln if mistake == 'crop_keeps_len' else n_sub)
    if kind == 'mask':
        pool = range(L) if mistake in ('padded_keys', 'mask_all_L') else range(ln)
        rank = _ranks(keys, pool, ties_high=mistake == 'ties_high')
        limit = L if mistake == 'mask_all_L' else ln
        out = [mask_id if p < limit and rank.get(p, L) < n_sub else int(row[p]) for p in range(L)]
        return out, ln
    window = [p for p in range(start, start + n_sub) if p < L]
    rank = _ranks(keys, window, ties_high=mistake == 'ties_high')
    out = [int(x) for x in row]
    for p in window:
        if mistake == 'inverse_perm':
            out[p] = int(row[start + rank[p]])            # a gather WITH the rank: the inverse permutation
        else:
            out[start + rank[p]] = int(row[p])
    return out, ln


def augment(seq, seqlen, kind, sub, U, mask_id=0, mistake=None):
    """A batch: ``seq`` [B, L], ``seqlen`` [B], ``U`` [B, L + 1] (array-likes) -> (out int64 [B, L], new_len int64 [B])."""
    seq, seqlen, U = np.asarray(seq), np.asarray(seqlen), np.asarray(U, dtype=np.float32)
    B, L = seq.shape
    assert U.shape == (B, L + 1) and len(sub) == L + 1
    out, new_len = np.zeros((B, L), dtype=np.int64), np.zeros(B, dtype=np.int64)
    for b in range(B):
        out[b], new_len[b] = augment_row(seq[b], seqlen[b], kind, sub, U[b], mask_id, mistake)
    return out, new_len
