"""CPU: the exact referee of the radix sort and the solo classification (tests/sort_referee.py) equals a brute-force Python sort
on small inputs, differs from each way the kernels can go wrong without a row sum noticing (an unstable permutation, an LSD
pass that is not stable, a split run, a wrong clamp, a flag on a padding or dropped key), and its restatement of the host plan
(radix_items / radix_tiles) yields the plans the GPU cases of test_gpu_sort.py are named after.  All on CPU arrays: nothing is
planted in a kernel."""
import random

import pytest
import torch

import sort_referee as sf


def _brute_pairs(keys):
    keys = [int(k) for k in keys]
    order = sorted(range(len(keys)), key=lambda e: (keys[e], e))
    return torch.tensor([(keys[e] << 32) | e for e in order], dtype=torch.int64)


def _brute_item_key(i, n_items):
    return n_items if i < 0 else min(i, n_items - 1)


def _random_step(seed, M, n, n_items, with_pos=True):
    g = torch.Generator().manual_seed(seed)
    neg = torch.randint(0, n_items, (M, n), generator=g)
    pos = torch.randint(0, n_items, (M,), generator=g) if with_pos else None
    bad = torch.tensor([-1, -2 ** 40, n_items, n_items + 5, 2 ** 40])
    at = torch.randperm(M * n, generator=g)[:min(5, M * n)]
    neg.view(-1)[at] = bad[:at.numel()]
    return pos, neg


# ------------------------------------------------------------------ the plan
PLANS = {
    1: ('small',), 63: ('small',), 64: ('small',), 65: ('small',), 255: ('small',), 256: ('small',), 257: ('small',), 4095: ('small',),
    4096: ('small',),
    4097: ('multi', 4, 5, 'inline'), 8192: ('multi', 4, 8, 'inline'),
    8193: ('multi', 4, 9, 'scan'), 262221: ('multi', 4, 257, 'scan'), 1048576: ('multi', 4, 1024, 'scan'),
    1048577: ('multi', 5, 820, 'scan'),
    2883585: ('multi', 12, 939, 'scan'),
    4456447: ('multi', 17, 1024, 'scan'), 4456448: ('multi', 17, 1024, 'scan'),
    4456449: ('multi', 9, 1935, 'scan'),
}


def test_plan_formulas_give_the_plans_the_gpu_cases_sit_on():
    """rsa_radix.hpp's radix_items / radix_tiles as restated in sort_referee.py: every total of test_gpu_sort.py gets the plan
    it is there for -- the one-workgroup sort up to RDX_TILE, items 4 with 5 and 8 tiles (inline scan), 9, 257 and 1024 tiles
    (scan kernel), items 5, 12 and 17, the full round's last tile ragged (4456447) and full (4456448), two rounds one element
    later."""
    for total, want in PLANS.items():
        assert sf.plan(total) == want, total
    assert sf.RDX_TILE == 4096
    assert 4456448 == sf.RDX_SLOTS * 256 * sf.RDX_ITEMS_MAX and 4456447 % (256 * 17) != 0 and 4456448 % (256 * 17) == 0
    # every `items` the host can pick in one round is a distinct plan; two rounds start at items = ceil(17 / 2)
    assert sorted({sf.radix_items(t) for t in range(4097, 4456449, 4099)}) == list(range(4, 18))
    # passes: 2^8, 2^16, 2^24 key counts are the borders (n_items + 1 keys: the ids and the drop key)
    assert [sf.radix_passes(n + 1) for n in (2, 255, 256, 65535, 65536, 2 ** 24 - 1, 2 ** 24, 2 ** 31 - 1)] == [1, 1, 2, 2, 3, 3, 4, 4]
    # the polarity switch of the classification at n_items = 10000
    assert sf.mostly_solo(6899, 10000) and not sf.mostly_solo(6901, 10000)


# ------------------------------------------------------------------ the referee == brute force
@pytest.mark.parametrize('seed', range(6))
def test_step_pairs_equal_a_brute_force_sort(seed):
    rnd = random.Random(seed)
    M, n, n_items = rnd.choice([1, 3, 17]), rnd.choice([1, 2, 7]), rnd.choice([2, 5, 300])
    for with_pos in (True, False):
        pos, neg = _random_step(seed, M, n, n_items, with_pos)
        ids = []
        for m in range(M):
            ids += ([int(pos[m])] if with_pos else []) + [int(v) for v in neg[m]]
        want = _brute_pairs([_brute_item_key(i, n_items) for i in ids])
        got = sf.expected_step_pairs(pos, neg, n_items)
        assert got.dtype == torch.int64 and torch.equal(got, want)
        assert bool((got >= 0).all())


@pytest.mark.parametrize('seed', range(4))
def test_step_all_pairs_equal_a_brute_force_sort(seed):
    g = torch.Generator().manual_seed(100 + seed)
    M, n, n_items, n_users = 9, 4, 11, 6
    pos, neg = _random_step(seed, M, n, n_items)
    uid = torch.randint(0, n_users, (M,), generator=g)
    uid[0], uid[1], uid[2] = -1, n_users, n_users + 7
    keys = []
    for m in range(M):
        keys += [_brute_item_key(int(pos[m]), n_items)] + [_brute_item_key(int(v), n_items) for v in neg[m]]
    for m in range(M):
        u = int(uid[m])
        keys.append(n_items + 1 + (n_users if u < 0 else min(u, n_users - 1)))
    got = sf.expected_step_all_pairs(pos, neg, uid, n_items, n_users)
    assert torch.equal(got, _brute_pairs(keys))
    t_items = M * (n + 1)
    # the item part is what the item sort alone gives; the user part lies behind it, elements t_items + m
    assert torch.equal(got[:t_items], sf.expected_step_pairs(pos, neg, n_items))
    assert bool((sf.pair_keys(got[t_items:]) > n_items).all()) and bool((sf.pair_elems(got[t_items:]) >= t_items).all())


@pytest.mark.parametrize('by_query', [False, True])
def test_segment_pairs_equal_a_brute_force_sort(by_query):
    g = torch.Generator().manual_seed(7)
    n_seg, stride, n_rows, n_q = 5, 9, 13, 6
    cap = stride - sf.SHARD_HDR
    keys = (torch.randint(0, n_q, (n_seg, stride), generator=g) << 32) | torch.randint(0, n_rows, (n_seg, stride), generator=g)
    lives = [0, 1, cap, 3, cap]
    for s, live in enumerate(lives):
        keys[s, 0], keys[s, 1] = live, 12345
    keys[2, 3] = (3 << 32) | (n_rows + 4)              # a row beyond the table: capped
    keys[2, 4] = ((n_q + 2) << 32) | 5                 # a query beyond the batch: capped
    keys[3, 7] = -1                                    # behind the live range: never read as a key
    dead = n_q if by_query else n_rows
    extra = None if by_query else torch.tensor([4, -1, 0, n_rows - 1, -1, 4])
    want = []
    for s in range(n_seg):
        for w in range(stride):
            k = int(keys[s, w])
            if w >= 2 and w - 2 < lives[s]:
                want.append(min(((k >> 32) & 0x7fffffff) if by_query else (k & 0xffffffff), dead))
            else:
                want.append(dead)
    if extra is not None:
        want += [dead if int(r) < 0 else min(int(r), dead) for r in extra]
    got = sf.expected_segment_pairs(keys.reshape(-1), n_seg, stride, by_query, dead, extra)
    assert torch.equal(got, _brute_pairs(want))
    assert want.count(dead) >= n_seg * 2 + cap - 1


def test_solo_flags_and_runs_equal_brute_force():
    g = torch.Generator().manual_seed(3)
    n_items, pad = 40, 7
    keys = torch.randint(0, n_items + 1, (120,), generator=g)
    keys[keys == pad] = 8
    keys[5] = pad                                       # the padding id alone on its row
    keys[keys == n_items] = 9
    keys[17] = n_items                                  # one dropped element, alone on the drop key
    pairs = sf.pairs_of_keys(keys)
    for pad_row in (pad, 0, -1):
        flags, flagged = sf.expected_classified(pairs, pad_row, n_items)
        klist = [int(k) for k in keys]
        want = [int(klist.count(k) == 1 and k != n_items and not (pad_row >= 0 and k == pad_row)) for k in klist]
        assert flags.tolist() == want
        assert flags[17] == 0 and int(flags[5]) == int(pad_row != pad)
        marked = (flagged & sf.SOLO_BIT) != 0
        assert torch.equal(sf.pair_elems(flagged), sf.pair_elems(pairs)) and torch.equal(sf.pair_keys(flagged), sf.pair_keys(pairs))
        assert sorted(sf.pair_elems(flagged)[marked].tolist()) == [e for e, f in enumerate(want) if f]
    # runs of a query-sorted array: [start, end) per query, 0 / 0 for a query that has no slot, the dead key has no run
    n_q = 9
    qk = torch.randint(0, n_q + 1, (50,), generator=g)
    qk[qk == 4] = 5
    qp = sf.pairs_of_keys(qk)
    start, end = sf.expected_runs(qp, n_q)
    sk = sf.pair_keys(qp).tolist()
    for q in range(n_q):
        at = [i for i, k in enumerate(sk) if k == q]
        assert (int(start[q]), int(end[q])) == ((at[0], at[-1] + 1) if at else (0, 0))
    assert start.dtype == end.dtype == torch.int32 and int(start[4]) == int(end[4]) == 0


# ------------------------------------------------------------------ the mistakes the referee must catch
def _hot_keys(seed=11, total=3000, n_keys=37):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, n_keys, (total,), generator=g)


def _is_keyed_permutation(pairs, keys):
    """sorted by key, every element once, every element under its own key: all a row-sum test can see"""
    e = sf.pair_elems(pairs)
    k = sf.pair_keys(pairs)
    return (bool((k[1:] >= k[:-1]).all()) and torch.equal(torch.sort(e).values, torch.arange(keys.numel()))
            and torch.equal(keys[e], k))


def test_unstable_permutations_differ():
    keys = _hot_keys()
    want = sf.pairs_of_keys(keys)
    # (1) correctly keyed, every run in REVERSE element order
    order = torch.sort(keys * keys.numel() + (keys.numel() - 1 - torch.arange(keys.numel()))).indices
    rev = (keys[order] << 32) | order
    assert _is_keyed_permutation(rev, keys) and not torch.equal(rev, want)
    # (2) one pair of equal-key neighbours swapped
    i = int(torch.nonzero(sf.pair_keys(want)[1:] == sf.pair_keys(want)[:-1])[40])
    sw = want.clone()
    sw[i], sw[i + 1] = want[i + 1], want[i]
    assert _is_keyed_permutation(sw, keys) and not torch.equal(sw, want) and int((sw != want).sum()) == 2


def test_a_split_run_differs():
    """One element of a run ranked into the wrong tile position: its row's elements form two runs.  Every element is present
    and carries its own key -- a scatter over this array touches the right rows with the right terms -- but the array is not
    the referee's."""
    keys = _hot_keys()
    want = sf.pairs_of_keys(keys)
    k = sf.pair_keys(want)
    i = int(torch.nonzero(k == 5)[0])
    j = int(torch.nonzero(k == 9)[-1])
    split = torch.cat([want[:i], want[i + 1:j + 1], want[i:i + 1], want[j + 1:]])
    e = sf.pair_elems(split)
    assert torch.equal(torch.sort(e).values, torch.arange(keys.numel())) and torch.equal(keys[e], sf.pair_keys(split))
    runs = int((sf.pair_keys(split)[1:] != sf.pair_keys(split)[:-1]).sum()) + 1
    assert runs == int(keys.unique().numel()) + 1          # one row in two runs
    assert not torch.equal(split, want)


def _lsd(keys, passes, unstable_pass=None):
    """An LSD radix sort of (key, element) by 8-bit digits; in ``unstable_pass`` equal digits come out in reverse input order."""
    order = torch.arange(keys.numel())
    for p in range(passes):
        d = (keys[order] >> (8 * p)) & 255
        pos = torch.arange(keys.numel())
        if p == unstable_pass:
            pos = keys.numel() - 1 - pos
        order = order[torch.sort(d * keys.numel() + pos).indices]
    return (keys[order] << 32) | order


@pytest.mark.parametrize('n_keys', [200, 60_000, 2 ** 24 + 5])
def test_an_lsd_sort_with_one_unstable_pass_differs(n_keys):
    g = torch.Generator().manual_seed(5)
    total = 5000
    keys = torch.randint(0, n_keys, (total,), generator=g)
    keys[::7] = keys[3]                                   # a hot key: equal in every digit
    passes = sf.radix_passes(n_keys)
    want = sf.pairs_of_keys(keys)
    assert torch.equal(_lsd(keys, passes), want)
    for p in range(passes):
        bad = _lsd(keys, passes, unstable_pass=p)
        assert not torch.equal(bad, want), p
        e = sf.pair_elems(bad)        # every element once, under its own key: a scatter over it still adds every term to its row
        assert torch.equal(torch.sort(e).values, torch.arange(total)) and torch.equal(keys[e], sf.pair_keys(bad))
        if passes == 1:               # and with one pass it is even sorted by key: only the order inside the runs is off
            assert _is_keyed_permutation(bad, keys)


def test_a_wrong_clamp_differs():
    n_items = 50
    pos, neg = _random_step(2, 30, 8, n_items)
    ids = sf.step_ids(pos, neg)
    assert int((ids < 0).sum()) >= 2 and int((ids >= n_items).sum()) >= 3
    want = sf.expected_step_pairs(pos, neg, n_items)
    for wrong in (torch.where(ids < 0, n_items, ids.clamp(max=n_items)),        # too-large ids dropped instead of clamped
                  ids.clamp(min=0, max=n_items - 1),                            # negative ids sent to row 0
                  torch.where(ids < 0, n_items, ids % n_items),                 # wrapped instead of clamped
                  torch.where(ids < 0, n_items - 1, ids.clamp(max=n_items - 1))):      # empty slots on the last row
        assert not torch.equal(sf.pairs_of_keys(wrong), want)
    # the users' clamp of the all-in-one sort
    uid = torch.tensor([3, -1, 9, 12, 0])
    want = sf.expected_step_all_pairs(pos[:5], neg[:5], uid, n_items, 10)
    t = 5 * 9
    assert sf.pair_keys(want[t:]).tolist() == sorted(n_items + 1 + u for u in (3, 10, 9, 9, 0))
    assert sf.pair_keys(sf.expected_step_all_pairs(pos[:5], neg[:5], uid.clamp(min=0), n_items, 10)[t:]).tolist() != sf.pair_keys(want[t:]).tolist()


def test_a_flag_on_a_padding_or_dropped_key_differs():
    n_items, pad = 30, 4
    keys = torch.tensor([1, 1, 2, pad, 6, 6, 6, 9, n_items, 12])
    pairs = sf.pairs_of_keys(keys[torch.tensor([9, 4, 0, 3, 5, 8, 1, 7, 6, 2])])
    k = sf.pair_keys(pairs)
    alone = torch.ones_like(k, dtype=torch.bool)
    alone[1:] &= k[1:] != k[:-1]
    alone[:-1] &= k[1:] != k[:-1]
    want = sf.expected_solo(k, pad, n_items)
    assert want.tolist() == [False, False, True, False, False, False, False, True, True, False]
    assert not torch.equal(alone, want) and int(alone.sum()) == int(want.sum()) + 2
    assert not torch.equal(alone & (k != pad), want) and not torch.equal(alone & (k != n_items), want)
    flags, flagged = sf.expected_classified(pairs, pad, n_items)
    assert not torch.equal(sf.expected_flags(pairs, alone), flags) and not torch.equal(sf.expected_flagged_pairs(pairs, alone), flagged)
    # pad_row = -1: no padding row -- the padding id alone on its row IS solo
    assert int(sf.expected_solo(k, -1, n_items).sum()) == int(want.sum()) + 1


# ------------------------------------------------------------------ the accessors (host code only: no GPU call)
@pytest.fixture(scope='module')
def lib():
    import os
    from recstudio_amd import _native
    if not os.path.exists(_native.LIB_PATH):
        _native.build()
    return _native.lib()


def test_accessors_follow_the_pass_parity_and_stay_inside_the_workspace(lib):
    """The offsets the GPU tests read at: 256-byte aligned, the pairs end inside the workspace the size query reports, one of
    exactly two places (the sort's ping-pong buffers) chosen by the parity of the pass count -- and bad sizes are refused."""
    import ctypes
    for M, n in ((1, 1), (4097, 1), (63, 64), (1048577, 1)):
        ws = lib.rsa_scatter_rows_sorted_workspace_bytes(M, n, 1000)
        by_parity = {}
        for n_items in (2, 255, 256, 65535, 65536, 2 ** 24 - 1, 2 ** 24, 2 ** 31 - 1):
            off = lib.rsa_scatter_rows_sorted_pairs_offset(M, n, n_items)
            assert off >= 0 and off % 256 == 0 and off + 8 * M * (n + 1) <= ws
            by_parity.setdefault(sf.radix_passes(n_items + 1) & 1, set()).add(off)
        assert len(by_parity[0]) == len(by_parity[1]) == 1
        assert abs(min(by_parity[0]) - min(by_parity[1])) >= 8 * M * (n + 1)        # two buffers that do not overlap
    # the all-in-one step: n_items + n_users + 2 keys decide the parity
    ws = lib.rsa_scatter_rows_sorted_workspace_bytes(700, 65, 97)
    a, b = lib.rsa_bpr_sgd_pairs_offset(700, 64, 97, 100), lib.rsa_bpr_sgd_pairs_offset(700, 64, 200, 100)
    assert abs(a - b) >= 8 * 700 * 66 and a % 256 == b % 256 == 0 and 0 <= min(a, b) and max(a, b) + 8 * 700 * 66 <= ws
    assert lib.rsa_bpr_sgd_pairs_offset(700, 64, 154, 100) == a and lib.rsa_bpr_sgd_pairs_offset(700, 64, 155, 100) == b
    # the owner workspace: five regions, in the workspace, none overlapping another
    out = (ctypes.c_int64 * 5)()
    for n_seg, stride, Q, n_rows in ((4, 150, 41, 97), (7, 10_000, 4100, 65536), (1, 4097, 41, 65536)):
        ws = lib.rsa_shard_backward_workspace_bytes(n_seg, stride, Q)
        assert lib.rsa_shard_backward_workspace_offsets(n_seg, stride, Q, n_rows, out) == 0
        slots = n_seg * stride
        regions = sorted(zip(out, (8 * (slots + Q), 8 * slots, 4 * Q, 4 * Q, slots + Q)))
        assert all(o % 256 == 0 and o >= 0 for o, _ in regions) and regions[-1][0] + regions[-1][1] <= ws
        assert all(o + size <= nxt for (o, size), (nxt, _) in zip(regions, regions[1:]))
    assert lib.rsa_scatter_rows_sorted_pairs_offset(0, 1, 10) < 0 and lib.rsa_scatter_rows_sorted_pairs_offset(5, 1, 2 ** 31) < 0
    assert lib.rsa_bpr_sgd_pairs_offset(5, 64, 2 ** 30, 2 ** 30) < 0
    assert lib.rsa_shard_backward_workspace_offsets(4, 150, 41, 97, None) == -1 and b'out5' in lib.rsa_last_error()
    assert lib.rsa_shard_backward_workspace_offsets(4, 2, 41, 97, out) == -1
