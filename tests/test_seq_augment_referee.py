"""CPU: data_augmentation.seq_augment_torch (the batched twin of rsa_seq_augment) against the per-sequence referee of
tests/seq_augment_referee.py, the invariants of the three kinds, their distributions, the seeded mistakes, the modules and the
argument checks of rsa_seq_augment (which run before any device call)."""
import ctypes
import itertools
import math
import random

import numpy as np
import pytest
import torch

import seq_augment_referee as sa

MASK_ID = 999
LENGTHS = (1, 2, 9, 20, 50, 64, 70)
BELOW_ONE = float(np.nextafter(np.float32(1), np.float32(0)))             # the largest fp32 below 1


@pytest.fixture(scope='module')
def ra():
    import recstudio_amd
    return recstudio_amd


def batch(L, seed, B=24):
    """Histories of lengths 0, 1, L and mixed (right-padded with 0, distinct ids inside a row) and one U."""
    g = torch.Generator().manual_seed(seed)
    lens = torch.randint(0, L + 1, (B,), generator=g)
    lens[:4] = torch.tensor([0, 1, L, L])
    seq = torch.stack([torch.randperm(200, generator=g)[:L] + 1 for _ in range(B)])
    seq = seq * (torch.arange(L).unsqueeze(0) < lens.unsqueeze(1))
    U = torch.rand(B, L + 1, generator=g)
    return seq, lens, U


def twin(ra, seq, lens, kind, sub, U):
    return ra.data_augmentation.seq_augment_torch(seq, lens, kind, torch.tensor(sub, dtype=torch.int32), U, MASK_ID)


def agree(ra, seq, lens, kind, sub, U):
    out, new_len = twin(ra, seq, lens, kind, sub, U)
    want, want_len = sa.augment(seq.numpy(), lens.numpy(), kind, sub, U.numpy(), MASK_ID)
    assert out.dtype == torch.int64 and new_len.dtype == lens.dtype
    assert torch.equal(out, torch.from_numpy(want)) and torch.equal(new_len.long(), torch.from_numpy(want_len))
    return out, new_len


@pytest.mark.parametrize('L', LENGTHS)
@pytest.mark.parametrize('kind', sa.KINDS)
def test_twin_equals_referee(ra, kind, L):
    for rate in (0.2, 0.7, 1.0, 1e-3):                                    # the last: n_sub = 0 (mask, reorder) or 1 (crop)
        sub = sa.sub_lengths(kind, rate, L)
        assert sub == ra.data_augmentation.sub_lengths(kind, rate, L) and sub[0] == 0
        if rate == 1e-3:
            assert set(sub[1:]) == ({1} if kind == 'crop' else {0})
        seq, lens, U = batch(L, 100 * L + int(1000 * rate))
        agree(ra, seq, lens, kind, sub, U)
        agree(ra, seq, lens.to(torch.int32), kind, sub, U)
        # seqlen outside [0, L] is clamped
        agree(ra, seq, torch.where(lens == L, lens + 5, lens) - (lens == 0).long(), kind, sub, U)
        # constructed ties: a handful of distinct key values, so equal keys are everywhere
        Ut = U.clone()
        Ut[:, 1:] = (Ut[:, 1:] * 3).floor() / 4
        agree(ra, seq, lens, kind, sub, Ut)
        # the ends of the start's range: the largest fp32 below 1 (the last start; see test_seeded_mistakes for the clamp) and 0
        Uc = U.clone()
        Uc[:, 0] = BELOW_ONE
        agree(ra, seq, lens, kind, sub, Uc)
        Uc[:, 0] = 0.0
        agree(ra, seq, lens, kind, sub, Uc)


@pytest.mark.parametrize('L', (2, 9, 20, 64, 70))
def test_invariants(ra, L):
    for rate in (0.2, 0.7, 1.0):
        seq, lens, U = batch(L, 7 * L + int(10 * rate), B=40)
        p = torch.arange(L).unsqueeze(0)
        ln = lens.unsqueeze(1)
        # crop: a contiguous slice of the input, zeros behind it
        sub = sa.sub_lengths('crop', rate, L)
        out, new_len = twin(ra, seq, lens, 'crop', sub, U)
        assert torch.equal(new_len, torch.tensor(sub)[lens].long())
        for b in range(seq.shape[0]):
            n, row = int(new_len[b]), seq[b].tolist()
            got = out[b, :n].tolist()
            assert any(row[s:s + n] == got for s in range(int(lens[b]) - n + 1)) and not out[b, n:].any()
        # mask: exactly n_sub positions below len change, all to mask_id
        sub = sa.sub_lengths('mask', rate, L)
        out, new_len = twin(ra, seq, lens, 'mask', sub, U)
        changed = out != seq
        assert torch.equal(new_len, lens) and torch.equal(changed.sum(1), torch.tensor(sub)[lens].long())
        assert bool((out[changed] == MASK_ID).all()) and not bool((changed & (p >= ln)).any())
        assert not bool(out[p.expand_as(out) >= ln].any())
        # reorder: a permutation inside one window of n_sub positions, the identity elsewhere
        sub = sa.sub_lengths('reorder', rate, L)
        out, new_len = twin(ra, seq, lens, 'reorder', sub, U)
        assert torch.equal(new_len, lens) and torch.equal(out.sort(1).values, seq.sort(1).values)
        for b in range(seq.shape[0]):
            moved = (out[b] != seq[b]).nonzero().view(-1)
            n = sub[int(lens[b])]
            if len(moved):
                assert int(moved[-1]) - int(moved[0]) + 1 <= n and int(moved[-1]) < int(lens[b])
        assert not bool(out[p.expand_as(out) >= ln].any())


def within(count, n, prob, sigmas=5.0):
    return abs(count - n * prob) <= sigmas * math.sqrt(n * prob * (1 - prob))


def test_distributions(ra):
    n, L = 20000, 5
    g = torch.Generator().manual_seed(2024)
    seq = torch.arange(1, L + 1).repeat(n, 1)
    lens = torch.full((n,), L)
    sub3, sub2 = [0, 0, 0, 0, 0, 3], [0, 0, 0, 0, 0, 2]
    # mask, n_sub = 3: each of the 10 subsets
    out, _ = twin(ra, seq, lens, 'mask', sub3, torch.rand(n, L + 1, generator=g))
    code = ((out == MASK_ID) * (2 ** torch.arange(L))).sum(1)
    counts = torch.bincount(code, minlength=32)
    subsets = [sum(2 ** i for i in c) for c in itertools.combinations(range(L), 3)]
    assert int(counts[subsets].sum()) == n and all(within(int(counts[s]), n, 1 / 10) for s in subsets)
    # reorder, n_sub = 3: the three starts, and given the start each of the 6 orders
    U = torch.rand(n, L + 1, generator=g)
    out, _ = twin(ra, seq, lens, 'reorder', sub3, U)
    start = torch.minimum((U[:, 0] * 3.0).long(), torch.tensor(2))
    starts = torch.bincount(start, minlength=3)
    assert all(within(int(c), n, 1 / 3) for c in starts)
    for s in range(3):
        rows = out[start == s]
        assert torch.equal(rows[:, :s], seq[:len(rows), :s]) and torch.equal(rows[:, s + 3:], seq[:len(rows), s + 3:])
        orders = {}
        for w in rows[:, s:s + 3].tolist():
            orders[tuple(w)] = orders.get(tuple(w), 0) + 1
        assert len(orders) == 6 and all(within(c, len(rows), 1 / 6) for c in orders.values())
    # crop, n_sub = 2: the 4 starts
    out, new_len = twin(ra, seq, lens, 'crop', sub2, torch.rand(n, L + 1, generator=g))
    assert bool((new_len == 2).all()) and bool((out[:, 1] == out[:, 0] + 1).all()) and not bool(out[:, 2:].any())
    starts = torch.bincount(out[:, 0] - 1, minlength=4)
    assert len(starts) == 4 and all(within(int(c), n, 1 / 4) for c in starts)


def fp32_length_case(kind, rate, L=64):
    """A length at which ``int(rate * n)`` in fp32 differs from float64, or None."""
    good, bad = sa.sub_lengths(kind, rate, L), sa.sub_lengths(kind, rate, L, fp32=True)
    return next((n for n in range(L + 1) if good[n] != bad[n]), None)


def test_seeded_mistakes_leave_equality(ra):
    L = 20
    seq, lens, U = batch(L, 5, B=64)
    U[:, 1:] = (U[:, 1:] * 3).floor() / 4                                  # ties
    # The clamp of the start.  For every span below 2^24 the fp32 product (1 - 2^-24) * span lies at least half an ulp below span
    # and rounds DOWN (checked here for the spans in reach), so no value torch.rand can return needs the clamp: it guards the
    # rule against a uniform of exactly 1, and only that seeds the mistake.
    assert all(int(np.float32(BELOW_ONE) * np.float32(s)) == s - 1 for s in range(1, 66))
    U[::2, 0] = 1.0
    cases ={'ties_high': ('mask', 'reorder'), 'padded_keys': ('mask',), 'no_clamp': ('crop', 'reorder'),
             'inverse_perm': ('reorder',), 'crop_keeps_len': ('crop',), 'mask_all_L': ('mask',)}
    assert sorted(cases) == sorted(sa.MISTAKES)
    for mistake, kinds in cases.items():
        for kind in kinds:
            sub = sa.sub_lengths(kind, 0.7, L)
            out, new_len = twin(ra, seq, lens, kind, sub, U)
            bad, bad_len = sa.augment(seq.numpy(), lens.numpy(), kind, sub, U.numpy(), MASK_ID, mistake=mistake)
            assert not (np.array_equal(out.numpy(), bad) and np.array_equal(new_len.numpy(), bad_len)), (mistake, kind)
    # int(rate * len) in fp32: at the default rates (gamma 0.7, beta 0.2, tau 0.2) fp32 and float64 truncate alike for every
    # length up to 64 -- so that mistake cannot be seeded there; the first rate of 0.01 .. 0.99 at which they differ is 0.58 (length 50:
    # 29 against 28), and it is seeded there
    assert fp32_length_case('mask', 0.7) is None and fp32_length_case('reorder', 0.2) is None and fp32_length_case('crop', 0.2) is None
    rate = next((r / 100 for r in range(1, 100) if fp32_length_case('mask', r / 100) is not None), None)
    if rate is not None:
        n = fp32_length_case('mask', rate)
        sub, bad_sub = sa.sub_lengths('mask', rate, 64), sa.sub_lengths('mask', rate, 64, fp32=True)
        seq, lens, U = batch(64, 9, B=8)
        lens[:] = n
        seq = seq * (torch.arange(64).unsqueeze(0) < n) + (seq == 0) * (torch.arange(64).unsqueeze(0) < n) * 7
        out, _ = twin(ra, seq, lens, 'mask', sub, U)
        bad, _ = sa.augment(seq.numpy(), lens.numpy(), 'mask', bad_sub, U.numpy(), MASK_ID)
        assert not np.array_equal(out.numpy(), bad)
        print(f'fp32 length table differs from float64 at rate {rate}, len {n}: {bad_sub[n]} against {sub[n]}')


def test_modules(ra, monkeypatch):
    da = ra.data_augmentation
    seq, lens, _ = batch(20, 3)
    for mod, kind, rate in ((da.Item_Crop(0.3), 'crop', 0.3), (da.Item_Mask(MASK_ID), 'mask', 0.7), (da.Item_Reorder(), 'reorder', 0.2),
                            (da.Item_Crop(), 'crop', 0.2), (da.Item_Mask(MASK_ID, 0.5), 'mask', 0.5), (da.Item_Reorder(0.9), 'reorder', 0.9)):
        for training in (True, False):                                     # nothing special in eval(): the reference augments regardless
            mod.train(training)
            torch.manual_seed(11)
            out, new_len = mod(seq, lens)
            torch.manual_seed(11)
            U = torch.rand(seq.shape[0], 21)
            want, want_len = sa.augment(seq.numpy(), lens.numpy(), kind, sa.sub_lengths(kind, rate, 20), U.numpy(), MASK_ID)
            assert torch.equal(out, torch.from_numpy(want)) and torch.equal(new_len, torch.from_numpy(want_len))
    assert da.sub_table('mask', 0.7, 20) is da.sub_table('mask', 0.7, 20)          # cached
    # Item_Random: exactly one random.randint(0, 2) per call, for the whole batch
    calls = []
    real = random.randint

    def counted(a, b):
        calls.append((a, b))
        return real(a, b)
    monkeypatch.setattr(da.random, 'randint', counted)
    mod = da.Item_Random(MASK_ID, tao=0.3, gamma=0.5, beta=0.9)
    seen = set()
    for i in range(30):
        random.seed(i)
        torch.manual_seed(i)
        out, new_len = mod(seq, lens)
        assert len(calls) == i + 1 and calls[-1] == (0, 2)
        random.seed(i)
        choice = real(0, 2)
        assert mod.last_choice == choice
        seen.add(choice)
        kind, rate = (('crop', 0.3), ('mask', 0.5), ('reorder', 0.9))[choice]
        torch.manual_seed(i)
        want, want_len = sa.augment(seq.numpy(), lens.numpy(), kind, sa.sub_lengths(kind, rate, 20), torch.rand(seq.shape[0], 21).numpy(),
                                    MASK_ID)
        assert torch.equal(out, torch.from_numpy(want)) and torch.equal(new_len, torch.from_numpy(want_len))
    assert seen == {0, 1, 2}
    with pytest.raises(ValueError, match='kind'):
        da.seq_augment_torch(seq, lens, 'shuffle', torch.zeros(21, dtype=torch.int32), torch.rand(seq.shape[0], 21))
    with pytest.raises(ValueError, match='U must be'):
        da.seq_augment_torch(seq, lens, 'crop', torch.zeros(21, dtype=torch.int32), torch.rand(seq.shape[0], 20))


def test_argument_validation_runs_before_any_device_call(ra):
    nat = ra._native
    lib = nat.lib()
    p = ctypes.c_void_p(64)

    def args(**kw):
        a = nat.SeqAugmentArgs()
        a.seq, a.seqlen, a.sub, a.out, a.new_len = p, p, p, ctypes.c_void_p(128), p
        a.seq_stride, a.n_seq, a.seq_len, a.kind, a.seqlen_bytes = 20, 4, 20, 0, 8
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    for kw, msg in ((dict(seq_len=65), b'seq_len'), (dict(seq_len=0), b'seq_len'), (dict(kind=3), b'kind'), (dict(seqlen_bytes=2), b'seqlen_bytes'),
                    (dict(n_seq=-1), b'negative'), (dict(seq=None), b'null'), (dict(seqlen=None), b'null'), (dict(sub=None), b'null'),
                    (dict(out=None), b'null'), (dict(new_len=None), b'null'), (dict(seq_stride=19), b'seq_stride'), (dict(out=p), b'alias'),
                    (dict(size=0), b'size')):
        assert lib.rsa_seq_augment(ctypes.byref(args(**kw)), None) == -1, kw
        assert msg in lib.rsa_last_error(), (kw, lib.rsa_last_error())
    assert lib.rsa_seq_augment(None, None) == -1 and b'args is null' in lib.rsa_last_error()
    assert lib.rsa_seq_augment(ctypes.byref(args(n_seq=0, seq=None, out=None)), None) == 0        # nothing to do, nothing launched
    with pytest.raises(RuntimeError, match='GPU only'):
        ra.ops.seq_augment(torch.zeros(2, 5, dtype=torch.int64), torch.zeros(2, dtype=torch.int64), 'crop', torch.zeros(6, dtype=torch.int32))
    with pytest.raises(ValueError, match='kind'):
        ra.ops.seq_augment(torch.zeros(2, 5, dtype=torch.int64), torch.zeros(2, dtype=torch.int64), 'cut', torch.zeros(6, dtype=torch.int32))
