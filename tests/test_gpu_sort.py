"""GPU: the in-tree LSD radix sort (csrc/rsa_radix.hpp) and classify_solo_kernel (csrc/rsa_sorted.hip) against the exact referee of
tests/sort_referee.py -- the SORTED PAIRS themselves, the solo flags, the payload marks and the owner side's query runs, every
comparison ``torch.equal``.  The pairs are found inside the callers' workspaces through the library's own accessors
(rsa_scatter_rows_sorted_pairs_offset, rsa_bpr_sgd_pairs_offset, rsa_shard_backward_workspace_offsets); no layout is restated here.

The totals sit on the borders of the host plan (sort_referee.plan, pinned to the header's formulas by test_sort_referee.py): the
one-workgroup sort up to 4096 elements, 5 / 8 tiles (inline scan), 9 / 257 / 1024 tiles (scan kernel), items 5, 12 and 17 rows per
wave, the full round with its last tile ragged and full, two rounds; the catalog sizes on the pass-count borders 2^8, 2^16, 2^24
(1 .. 4 passes: which ping-pong buffer holds the result).  All inputs are valid for the library: out-of-range ids are clamped by
the sources."""
import ctypes

import pytest
import torch

import sort_referee as sf

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


@pytest.fixture(scope='module')
def ra():
    import recstudio_amd
    recstudio_amd._native.lib()
    return recstudio_amd


def _region(ws, offset, count, dtype):
    """``count`` elements of ``dtype`` at byte ``offset`` of a workspace (the accessors' offsets are relative to the pointer rounded
    up to 256 bytes: the allocations here are aligned, so that is the pointer itself) -> CPU tensor"""
    assert ws.data_ptr() % 256 == 0 and offset >= 0
    size = torch.empty((), dtype=dtype).element_size()
    assert offset + count * size <= ws.numel()
    return ws[offset:offset + count * size].view(dtype).cpu()


# ------------------------------------------------------------------------------------------------------------------ key patterns
def _ff_id(n_items):
    """an id whose key has digit 255 in every pass, as far as the catalog allows: the drop key itself where it is 0xff..ff
    (n_items = 2^8k - 1: id -1 sorts under key n_items), else the largest 0xff..ff below n_items"""
    for k in (3, 2, 1):
        if n_items == (1 << (8 * k)) - 1:
            return -1
    for k in (3, 2, 1):
        if (1 << (8 * k)) - 1 < n_items:
            return (1 << (8 * k)) - 1
    return n_items - 1


def _pattern(name, total, n_items, g):
    e = torch.arange(total, dtype=torch.int64)
    if name == 'uniform':
        return torch.randint(0, n_items, (total,), generator=g)
    if name == 'equal':
        return torch.full((total,), n_items // 2, dtype=torch.int64)
    if name == 'top-digit':           # two keys that differ in one bit of the top digit only
        hi = n_items - 1
        lo = hi & ~(1 << (hi.bit_length() - 1)) if hi else 0
        return torch.where(torch.randint(0, 2, (total,), generator=g) == 1, hi, lo)
    if name == 'ascending':
        return e % n_items
    if name == 'descending':
        return (total - 1 - e) % n_items
    if name == 'digit-cycle':         # byte p of the key = (e >> p) & 255: every digit of every pass is hit
        return sum(((e >> p) & 255) << (8 * p) for p in range(4)) % n_items
    if name == 'ff-tail':             # digit 255 in every pass in the ragged last row of the last tile, next to the ~0 fill lanes
        ids = torch.randint(0, n_items, (total,), generator=g)
        ids[total - ((total - 1) % 64 + 1):] = _ff_id(n_items)
        ids[::997] = _ff_id(n_items)
        return ids
    if name == 'invalid':             # dropped and clamped ids among random ones, the last elements included
        ids = torch.randint(0, n_items, (total,), generator=g)
        bad = torch.tensor([-1, -2 ** 40, n_items, n_items + 5, 2 ** 40])
        at = torch.randperm(total, generator=g)[:max(total // 16, min(total, 5))]
        ids[at] = bad[torch.arange(at.numel()) % 5]
        ids[-1] = -1
        return ids
    raise KeyError(name)


PATTERNS = ('uniform', 'equal', 'top-digit', 'ascending', 'descending', 'digit-cycle', 'ff-tail', 'invalid')
PASS_BORDERS = (2, 255, 256, 65535, 65536, 2 ** 24 - 1, 2 ** 24, 2 ** 31 - 1)


def _step_element_cases():
    out = []
    for total in (4096, 4097, 8193, 1048577):
        out += [(total, n_items) for n_items in PASS_BORDERS]
    for total in (1, 63, 64, 65, 255, 256, 257, 4095, 8192, 262221, 1048576):
        out += [(total, n_items) for n_items in (2, 256, 65536, 2 ** 31 - 1)]           # 1, 2, 3 and 4 passes
    for total in (2883585, 4456447, 4456448, 4456449):
        out += [(total, n_items) for n_items in (1000, 100_000_001)]
    return out


def _sorted_pairs(ra, ws, M, n, n_items, total):
    off = int(ra._native.lib().rsa_scatter_rows_sorted_pairs_offset(M, n, n_items))
    return _region(ws, off, total, torch.int64)


# ------------------------------------------------------------------------------------------------------------ (a) step elements
@pytest.mark.parametrize('total,n_items', _step_element_cases(), ids=lambda v: str(v))
def test_step_elements_sorted_pairs(ra, total, n_items):
    """rsa_sort_step_elements without classification over ``total`` = M x 1 elements (no positives: any total can be hit), every
    key pattern: the pairs at the accessor's offset == the stable CPU sort, no payload carries bit 31."""
    assert (sf.plan(total) == ('small',)) == (total <= sf.RDX_TILE)
    g = torch.Generator().manual_seed(total % 9973 + n_items % 101)
    for name in PATTERNS:
        ids = _pattern(name, total, n_items, g).view(total, 1)
        solo, ws = ra.ops.sort_step_elements(None, ids.to(DEV), n_items, want_solo=False)
        torch.cuda.synchronize()
        got = _sorted_pairs(ra, ws, total, 1, n_items, total)
        want = sf.expected_step_pairs(None, ids, n_items)
        assert solo is None
        assert torch.equal(got, want), (name, int((got != want).sum()), int(torch.nonzero(got != want)[0]))
        assert not bool((got & sf.SOLO_BIT).any()), name
        del ws


@pytest.mark.parametrize('M,n', [(41, 64), (63, 64), (300, 64), (1000, 7)])
@pytest.mark.parametrize('n_items', [97, 2 ** 24 + 5])
def test_step_elements_with_positives(ra, M, n, n_items):
    """w = n + 1 elements per query, column 0 the positive: SrcStepIds' e / w and the positive column."""
    g = torch.Generator().manual_seed(M + n)
    total = M * (n + 1)
    for name in ('uniform', 'invalid', 'ff-tail', 'digit-cycle'):
        ids = _pattern(name, total, n_items, g).view(M, n + 1)
        pos, neg = ids[:, 0].contiguous(), ids[:, 1:].contiguous()
        _, ws = ra.ops.sort_step_elements(pos.to(DEV), neg.to(DEV), n_items, want_solo=False)
        torch.cuda.synchronize()
        got = _sorted_pairs(ra, ws, M, n, n_items, total)
        assert torch.equal(got, sf.expected_step_pairs(pos, neg, n_items)), name
        assert not bool((got & sf.SOLO_BIT).any()), name


# ------------------------------------------------------------------------------------------------------------ (b) classification
# (total, n_items, pad_row, dropped ids, the value the flags are preset to): both polarities (preset 1 below total = 0.69 n_items)
# next to the switch and far from it; the padding id is alone on its row wherever there is a padding row
CLASSIFY = [
    (4096, 10_000, 0, 'many', 1), (6899, 10_000, 5000, 'many', 1), (6901, 10_000, -1, 'one', 0), (8193, 10_000, 0, 'many', 0),
    (4096, 1_000_000, -1, 'many', 1), (8193, 100, 50, 'one', 0),
    (1048577, 300_000, 0, 'many', 0), (1048577, 2_000_000, 1_000_000, 'one', 1),
]


@pytest.mark.parametrize('total,n_items,pad_row,dropped,preset', CLASSIFY)
def test_classification_and_presorted_apply(ra, total, n_items, pad_row, dropped, preset):
    """rsa_sort_step_elements with the classification: flags == the referee's, bit 31 of the payload exactly on the solo pairs;
    then rsa_rows_update_presorted over that workspace on a zeroed [n_items, 64] target with NO forward having applied the solo
    elements: their rows stay bit-zero, every other row is bit-equal to rsa_rows_update_sorted on the same inputs."""
    g = torch.Generator().manual_seed(total + n_items)
    ids = torch.randint(0, n_items - 1, (total,), generator=g)
    if pad_row >= 0:
        ids[ids == pad_row] = pad_row + 1
    if dropped == 'many':
        ids[torch.randperm(total, generator=g)[:max(total // 50, 2)]] = -1
        ids[1] = -2 ** 40
    else:
        ids[total // 2] = -1                             # one dropped id: alone on the drop key
    ids[total // 5] = n_items - 1                        # a row with one element and a row with two, whatever the density
    ids[7], ids[total - 1] = n_items - 2, n_items - 2
    if pad_row >= 0:
        ids[total // 3] = pad_row                        # the padding id: the only element on its row
    ids = ids.view(total, 1)
    assert sf.mostly_solo(total, n_items) == bool(preset)
    ids_d = ids.to(DEV)
    solo, ws = ra.ops.sort_step_elements(None, ids_d, n_items, pad_row=pad_row, want_solo=True)
    torch.cuda.synchronize()
    want_flags, want_pairs = sf.expected_classified(sf.expected_step_pairs(None, ids, n_items), pad_row, n_items)
    got = _sorted_pairs(ra, ws, total, 1, n_items, total)
    assert torch.equal(solo.cpu().view(-1), want_flags)
    assert torch.equal(got, want_pairs)
    n_solo = int(want_flags.sum())
    assert 0 < n_solo < total
    # the apply pass over the classified workspace
    qrows = 257
    q = torch.randn(qrows, 64, generator=g).to(DEV)
    qi = (torch.arange(total) % qrows).to(DEV)
    dneg = (torch.rand(total, 1, generator=g) + 0.5).to(DEV)
    got_t = torch.zeros(n_items, 64, device=DEV)
    ra.ops.scatter_rows_presorted(got_t, q, ws, total, 1, dneg, query_index=qi, pad_row=pad_row)
    want_t = torch.zeros(n_items, 64, device=DEV)
    ra.ops.scatter_rows_sorted(want_t, q, ids_d, dneg, query_index=qi, pad_row=pad_row)
    torch.cuda.synchronize()
    solo_rows = ids.view(-1)[want_flags.bool()].to(DEV)
    is_solo_row = torch.zeros(n_items, dtype=torch.bool, device=DEV)
    is_solo_row[solo_rows] = True
    assert not bool(got_t[solo_rows].any())                                   # left alone: bit-zero
    assert bool(want_t[solo_rows].any(dim=1).all())                           # (the full pass does write them)
    assert torch.equal(got_t[~is_solo_row], want_t[~is_solo_row])
    if pad_row >= 0:
        assert not bool(want_t[pad_row].any())


# ------------------------------------------------------------------------------------------------- (c) the all-in-one step sort
def _prepare_only(ra, iw, uw, n, uid, pos, sampler, neg):
    """The block of fused._sgd_step_block filled the way fused._bpr_sgd_step_in_forward fills it; ONLY rsa_bpr_sgd_prepare runs."""
    fused, nat = ra.fused, ra._native
    M = uid.numel()
    kind, _ = fused._sampler_cfg(sampler, neg, M)
    step = torch.full((1,), -1.0, dtype=torch.float32, device=DEV)
    b = fused._sgd_step_block(iw, uw, n, M, kind, sampler, step, neg=neg.contiguous() if kind == nat.SAMPLER_GIVEN else None)
    a = b['args']
    keep = None
    if kind == nat.SAMPLER_POPULAR:
        pop, keep = fused._popular_block(sampler)
        a.pop = ctypes.pointer(pop)
    a.user_ids, a.pos_ids = uid.data_ptr(), pos.data_ptr()
    if kind != nat.SAMPLER_GIVEN:
        fused._reserve_draw(a, kind, sampler, M, n, torch.device(DEV))
    rc = nat.lib().rsa_bpr_sgd_prepare(b['ref'], torch.cuda.current_stream().cuda_stream)
    if rc != 0:
        nat.check(rc, 'rsa_bpr_sgd_prepare')
    torch.cuda.synchronize()
    del keep
    return b


@pytest.fixture(scope='module')
def step_tables():
    """item tables of the two catalogs and a user table: rsa_bpr_sgd_prepare never reads them"""
    return {N: torch.zeros(N, 64, device=DEV) for N in (97, 200_003)}, torch.zeros(1000, 64, device=DEV)


@pytest.mark.parametrize('B', [1, 62, 63, 700])
@pytest.mark.parametrize('kind', ['given', 'uniform', 'popular'])
@pytest.mark.parametrize('N', [97, 200_003])
def test_step_all_sorted_pairs(ra, step_tables, B, kind, N):
    """rsa_bpr_sgd_prepare, n = 64: 66 B elements (4092 at B = 62: the one-workgroup sort and the stand-alone sampler; 4158 at
    B = 63: the draw inside the histogram launch).  The item part and the user part == the referee on the ids the call left in
    ``neg``; those ids == the stand-alone sampler's under the same Philox state; flags and payload marks on the item part only."""
    n, U = 64, 1000
    items, uw = step_tables
    iw = items[N]
    assert (66 * B > sf.RDX_TILE) == (B >= 63)
    g = torch.Generator().manual_seed(B + N)
    sampler = None
    if kind == 'uniform':
        sampler = ra.UniformSampler(N)
    elif kind == 'popular':
        sampler = ra.PopularSamplerModel((torch.rand(N, generator=g) ** 8 * 1e4).long()).to(DEV)
    users = {'random': torch.randint(0, U, (B,), generator=g),
             'one': torch.full((B,), 5, dtype=torch.int64),
             'invalid': torch.randint(0, U, (B,), generator=g)}
    users['invalid'][::3] = torch.tensor([-1, U, U + 7, -2 ** 40])[torch.arange(len(range(0, B, 3))) % 4]
    for name, uid in users.items():
        pos = torch.randint(0, N, (B,), generator=g)
        neg = None
        if kind == 'given':
            neg = torch.randint(0, N, (B, n), generator=g)
            neg.view(-1)[::29] = torch.tensor([-1, N, N + 5, -2 ** 40, 2 ** 40])[torch.arange(len(range(0, B * n, 29))) % 5]
        torch.manual_seed(77 + B)
        b = _prepare_only(ra, iw, uw, n, uid.to(DEV), pos.to(DEV), sampler, None if neg is None else neg.to(DEV))
        ids = b['neg'].cpu().view(B, n)
        if kind == 'given':
            assert torch.equal(ids, neg)
        else:
            torch.manual_seed(77 + B)           # the stand-alone sampler under the same Philox state
            alone = sampler(torch.empty(B, 1, device=DEV), n, pos.to(DEV))[1]
            assert torch.equal(ids, alone.cpu().view(B, n)), name
        t_items, total = B * (n + 1), B * (n + 2)
        off = int(ra._native.lib().rsa_bpr_sgd_pairs_offset(B, n, N, U))
        got = _region(b['iws'], off, total, torch.int64)
        want = sf.expected_step_all_pairs(pos, ids, uid, N, U)
        flags, item_part = sf.expected_classified(want[:t_items], 0, N)
        assert torch.equal(sf.pair_keys(got), sf.pair_keys(want)) and torch.equal(sf.pair_elems(got), sf.pair_elems(want)), name
        assert torch.equal(got[:t_items], item_part), name
        assert torch.equal(got[t_items:], want[t_items:]) and not bool((got[t_items:] & sf.SOLO_BIT).any()), name
        assert torch.equal(b['solo'].cpu().view(-1), flags), name


# ------------------------------------------------------------------------------------------------ (d) owner-side sorts from segments
def _segments(g, n_seg, stride, n_rows, Q):
    """valid received segments: live counts 0, 1, capacity and random; rows and queries beyond the dead keys (capped); garbage
    behind the live ranges"""
    cap = stride - sf.SHARD_HDR
    keys = torch.full((n_seg, stride), -7, dtype=torch.int64)
    live = torch.randint(0, cap + 1, (n_seg,), generator=g)
    for s, v in zip(range(n_seg), (cap, 0, 1)):
        live[s] = v
    if n_seg == 1:
        live[0] = cap - 3
    for s in range(n_seg):
        c = int(live[s])
        keys[s, 0], keys[s, 1] = c, 3
        r = torch.randint(0, n_rows, (c,), generator=g)
        q = torch.randint(0, Q, (c,), generator=g)
        if c > 40:
            r[:4] = 0                                          # the padding row, several times
            r[5], r[6] = n_rows + 9, 2 ** 32 - 1               # rows beyond the table: capped to the dead key
            q[7], q[8] = Q + 1, 2 ** 31 - 1                    # queries beyond the batch
            r[9:12] = n_rows - 1
        keys[s, sf.SHARD_HDR:sf.SHARD_HDR + c] = (q << 32) | r
    return keys, live


@pytest.mark.parametrize('n_seg,stride', [(4, 150), (8, 512), (1, 4097), (7, 10_000)])
@pytest.mark.parametrize('n_rows,Q', [(97, 41), (65536, 4100), (97, 4100), (65536, 41)])
@pytest.mark.parametrize('pad_row', [0, -1])
def test_owner_sorts_from_segments(ra, n_seg, stride, n_rows, Q, pad_row):
    """HipBackend.owner_bpr_prepare (forward_parts = 1) in place on one GPU over synthetic received segments of 600, 4096, 4097 and
    70 000 slots: row_sorted (slots + the step's positives, owned and not) and q_sorted == the referee, run_start / run_end ==
    the runs of the query-sorted reference, flags and payload marks as the classification of the row sort."""
    from recstudio_amd.shard import HipBackend
    be = HipBackend()
    slots = n_seg * stride
    assert slots in (600, 4096, 4097, 70_000)
    g = torch.Generator().manual_seed(slots + n_rows + Q)
    keys, live = _segments(g, n_seg, stride, n_rows, Q)
    pos_rows = torch.randint(0, n_rows, (Q,), generator=g)
    pos_rows[::3] = -1                                         # owned by another rank
    pos_rows[1] = 0
    item = torch.zeros(n_rows, 64, device=DEV)
    scale = torch.full((1,), -0.5, device=DEV)
    ctx = be.owner_bpr_prepare(be.new_state(DEV), item, Q, keys.to(DEV).view(-1), n_seg, stride, pos_rows.to(DEV), 64, Q, item, scale,
                               item_pad_row=pad_row)
    torch.cuda.synchronize()
    offs = (ctypes.c_int64 * 5)()
    assert ra._native.lib().rsa_shard_backward_workspace_offsets(n_seg, stride, Q, n_rows, offs) == 0
    ws = ctx['ws']
    row_total = slots + Q
    row_sorted = _region(ws, offs[0], row_total, torch.int64)
    q_sorted = _region(ws, offs[1], slots, torch.int64)
    run_start, run_end = _region(ws, offs[2], Q, torch.int32), _region(ws, offs[3], Q, torch.int32)
    solo = _region(ws, offs[4], row_total, torch.uint8)
    flat = keys.view(-1)
    want_rows = sf.expected_segment_pairs(flat, n_seg, stride, False, n_rows, extra_rows=pos_rows)
    want_flags, want_rows = sf.expected_classified(want_rows, pad_row, n_rows)
    want_q = sf.expected_segment_pairs(flat, n_seg, stride, True, Q)
    assert torch.equal(q_sorted, want_q)
    assert torch.equal(sf.pair_keys(row_sorted), sf.pair_keys(want_rows))
    assert torch.equal(row_sorted, want_rows)
    assert torch.equal(solo, want_flags)
    ws_, we_ = sf.expected_runs(want_q, Q)
    assert torch.equal(run_start, ws_) and torch.equal(run_end, we_)
    assert int(sf.pair_keys(want_q).eq(Q).sum()) >= slots - int(live.sum())      # the dead slots sort last
