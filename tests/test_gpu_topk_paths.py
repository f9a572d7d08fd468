"""GPU: every way rsa_fullscore's top-k can produce a row, each PROVEN taken and each held to the float64 referee
(tests/topk_referee.py): the dense select, and on the filter plan the direct (bitonic only) and radix candidate selects, the
overflow list, and the exact recompute for each of its three causes -- in one call that mixes them, since the path is chosen per
row by the data.  rsa_fullscore_plan says which plan a shape gets and where the select's bookkeeping (thr / flags / seg_cnt /
ovf_cnt) lies in the workspace; the helper below calls rsa_fullscore through _native with a workspace it owns and reads it back.

Steering.  Catalog items are zero in coordinates 0..4 unless they belong to a boosted set; a boosted item is zero everywhere
EXCEPT its set's coordinate.  A query row has q0 in at most one of those coordinates, so it sees exactly one set far above every
ordinary item (in all three score modes) and the other sets far below, and sets in unsampled tiles never move a threshold:
    coordinate 0  radix      ~2000 items spread over the unsampled tiles, all equal (the k-th value lies inside a tie group)
    coordinate 1  overflow   every unsampled item of three whole item ranges, values rising with the id in levels of 16 equal
                             items: the best ones arrive last and live in the overflow list
    coordinate 2  too many   ~5000 spread items (> cand_max candidates)
    coordinate 3  list full  consecutive unsampled items, as many as push the overflow list past its slots
    coordinate 4  too few    one item in the first sampled tile of every group, all equal: the threshold IS the top score and
                             nothing is strictly above it
The sizes are checked against the referee's candidate counts before the GPU is involved (design_classes)."""
import ctypes
import math

import pytest
import torch

import topk_referee as R

pytestmark = pytest.mark.gpu
DEV = 'cuda'
MODES = {'ip': R.IP, 'cos': R.COS, 'euc': R.EUC}
CLASSES = ('direct', 'radix', 'overflow', 'too_many', 'list_full', 'too_few')
COORD = {'radix': 0, 'overflow': 1, 'too_many': 2, 'list_full': 3, 'too_few': 4}
N_SPECIAL = 5


@pytest.fixture(scope='module')
def ra():
    import recstudio_amd
    recstudio_amd._native.lib()
    torch.cuda.init()
    return recstudio_amd


def plan_of(ra, B, N, k):
    nat = ra._native
    info = nat.FullscorePlanInfo()
    nat.check(nat.lib().rsa_fullscore_plan(B, N, k, info), 'rsa_fullscore_plan')
    return info


def run_native(ra, items, query, k, mode, want_lse):
    """rsa_fullscore with a workspace this test owns -> dict(val, idx, lse, plan, and on the filter plan thr / flags / seg_cnt /
    ovf_cnt as the call left them), all on the CPU.  Operands are prepared as ops.fullscore prepares them."""
    nat, ops = ra._native, ra.ops
    B, N = query.shape[0], items.shape[0]
    ia = qa = None
    if mode != R.IP:
        ia, qa = ops.row_sqnorm(items[1:], mode, pad=64), ops.row_sqnorm(query, mode)
    items_p, query_p, dim = ops._pad_k(items, query)
    items_p, query_p = items_p.contiguous(), query_p.contiguous()
    plan = plan_of(ra, B, N, k)
    n_bytes = int(nat.lib().rsa_fullscore_workspace_bytes(B, N, k))
    ws = torch.zeros(n_bytes, dtype=torch.uint8, device=DEV)
    val = torch.empty(B, k, dtype=torch.float32, device=DEV)
    idx = torch.empty(B, k, dtype=torch.int64, device=DEV)
    lse = torch.empty(B, dtype=torch.float32, device=DEV) if want_lse else None
    a = nat.FullscoreArgs()
    a.item_table, a.n_items, a.dim, a.score_mode = nat.ptr(items_p), N, dim, mode
    a.query, a.n_query, a.k = nat.ptr(query_p), B, k
    a.lse, a.topk_val, a.topk_idx = nat.ptr(lse), nat.ptr(val), nat.ptr(idx)
    a.item_aux, a.query_aux = nat.ptr(ia), nat.ptr(qa)
    a.workspace, a.workspace_bytes = nat.ptr(ws), n_bytes
    nat.launch('rsa_fullscore', None, ctypes.byref(a))
    torch.cuda.synchronize()
    out = dict(val=val.cpu(), idx=idx.cpu(), lse=None if lse is None else lse.cpu(), plan=plan)
    if plan.filter:
        base = (-ws.data_ptr()) % 256                 # the regions start at the pointer rounded up to 256 bytes

        def region(off, count, dtype):
            return ws[base + off:base + off + 4 * count].cpu().clone().view(dtype)
        out['thr'] = region(plan.thr_offset, B, torch.float32)
        out['flags'] = region(plan.flags_offset, B, torch.int32)
        out['seg_cnt'] = region(plan.seg_cnt_offset, B * plan.n_seg, torch.int32).view(B, plan.n_seg)
        out['ovf_cnt'] = region(plan.ovf_cnt_offset, B, torch.int32)
    return out


# ------------------------------------------------------------------ inputs
def boosted_sets(plan, n_cols):
    """the columns of the five sets, from the plan: disjoint, the first four in unsampled tiles only"""
    sampled = R.sampled_mask(n_cols, plan)
    cols = torch.arange(n_cols)
    per, tiles = int(plan.items_per_split), -(-n_cols // R.TI)
    free = ~sampled
    sets = {}
    # overflow: the unsampled items of three whole item ranges
    ranges = [3, int(plan.splits) // 2, int(plan.splits) - 3]
    in_ranges = torch.zeros(n_cols, dtype=torch.bool)
    for x in ranges:
        in_ranges |= (cols // per) == x
    sets['overflow'] = cols[in_ranges & free]
    free = free & ~in_ranges
    # list full: consecutive unsampled items from range 20 on -- a segment keeps `seg`, the rest are appended: as many ranges as
    # push the appends past the list, and a few more
    unsampled_per_seg = per // R.TI * (int(plan.tile_stride) - 1) / int(plan.tile_stride) * R.TI / 2
    n_ranges = int((int(plan.ovf) + 200) / max(unsampled_per_seg - int(plan.seg), 1.0) / 2) + 2
    in_l = (cols // per >= 20) & (cols // per < 20 + n_ranges)
    sets['list_full'] = cols[in_l & free]
    free = free & ~in_l
    # spread sets: evenly over what is left, and always some in the first unsampled tile and in the last (partial) tile
    first_tile = cols[(cols // R.TI == 1) & free]
    last_tile = cols[(cols // R.TI == tiles - 1) & free]
    assert len(first_tile) == R.TI and len(last_tile) >= 1 and not bool(sampled[last_tile].any())
    edge_r = torch.cat([first_tile[:3], last_tile[-2:]])
    edge_m = torch.cat([first_tile[8:11], last_tile[:1]]) if len(last_tile) >= 3 else first_tile[8:11]
    free[edge_r] = False
    free[edge_m] = False
    rest = cols[free]
    pick_r = rest[torch.linspace(0, len(rest) - 1, 2000).long()]
    free[pick_r] = False
    rest = cols[free]
    pick_m = rest[torch.linspace(0, len(rest) - 1, 5000).long()]
    sets['radix'] = torch.cat([edge_r, pick_r]).unique()
    sets['too_many'] = torch.cat([edge_m, pick_m]).unique()
    # too few: row 5 of the first sampled tile of every group
    g = torch.arange(int(plan.groups))
    sets['too_few'] = g * int(plan.group_tiles) * int(plan.tile_stride) * R.TI + 5
    assert bool(sampled[sets['too_few']].all())
    allc = torch.cat(list(sets.values()))
    assert len(allc.unique()) == len(allc)
    return sets


def steering_inputs(plan, N, d, B, kind, classes, seed):
    """(items [N, d], query [B, d], sets, q0): row b is designed for classes[b % len(classes)]"""
    g = torch.Generator().manual_seed(seed)
    n_cols = N - 1
    if kind == 'grid':
        items = torch.randint(-2, 3, (N, d), generator=g).float()
        query = torch.randint(-2, 3, (B, d), generator=g).float()
        q0, lo = 64.0, 32.0
    else:
        sigma = 0.5 * math.sqrt(27.0 / (d - N_SPECIAL))      # |w|^2 ~ 6.75 at every d: far below q0^2 (Euclidean: a set the row
        items = torch.randn(N, d, generator=g) * sigma        # does not look at scores -q0^2 - |q|^2, below the ordinary items)
        query = torch.randn(B, d, generator=g) * sigma
        q0, lo = 4.0, 2.0
    items[0] = 9.0                                         # the padding row: never scored
    items[:, :N_SPECIAL] = 0.0
    query[:, :N_SPECIAL] = 0.0
    sets = boosted_sets(plan, n_cols)
    for name, cols in sets.items():
        items[1 + cols] = 0.0
        if name == 'overflow':                            # rising with the id in at most 32 levels of equal items, below q0
            level = torch.arange(len(cols)) // max(16, -(-len(cols) // 32))
            items[1 + cols, COORD[name]] = lo + (q0 - lo) * level.float() / 32.0
        else:
            items[1 + cols, COORD[name]] = q0
    for b in range(B):
        c = classes[b % len(classes)]
        if c != 'direct':
            query[b, COORD[c]] = q0
    return items, query, sets, q0


def design_classes(S, e, plan, k):
    """The class every row WILL take, from the referee alone, or None where the fp32 noise could decide: the candidates are
    counted twice, without and with the items within twice the row's bound of the float64 threshold, and both counts must give
    the same class.  (An item whose float64 score EQUALS the threshold is a copy of the item the threshold came from -- the same
    operands, the same fp32 bits -- and is not strictly above it under any rounding.)"""
    thr = R.threshold64(S, plan).unsqueeze(-1)
    E = e.max(-1, keepdim=True).values
    sure = S > thr + 2.0 * E
    maybe = sure | (((S - thr).abs() <= 2.0 * E) & (S != thr))
    seen = []
    for above in (sure, maybe):
        cnt = R.segment_counts_of(above, plan)
        seg = cnt.clamp(max=int(plan.seg))
        ovf = (cnt - int(plan.seg)).clamp(min=0).sum(-1)
        total = R.candidate_totals(plan, seg, ovf)
        row = []
        for tt, oo in zip(total.tolist(), ovf.tolist()):
            if oo > int(plan.ovf):
                row.append('list_full' if tt <= int(plan.cand_max) else None)
            elif tt > int(plan.cand_max):
                row.append('too_many')
            elif tt < k:
                row.append('too_few' if oo == 0 else None)
            elif oo > 0:
                row.append('overflow')
            else:
                row.append('direct' if tt <= 1024 else 'radix')
        seen.append(row)
    return [a if a == b else None for a, b in zip(*seen)]


def kernel_class(path, cause):
    if path == 'recompute':
        return cause
    return 'overflow' if path.endswith('+overflow') else path


REPORT = []


def report(line):
    REPORT.append(line)
    print('\n' + line)


def verify(ra, tag, items, query, k, mode, kind, expect_filter, designed=None, tie_sets=None):
    """(a) .. (f) of a case; returns the per-class row counts."""
    B, N, d_in = query.shape[0], items.shape[0], items.shape[1]
    d_run = 32 if d_in <= 32 else 64 if d_in <= 64 else 128
    exact = kind == 'grid' and mode != R.COS
    S = R.scores64(items, query, mode)
    e = torch.zeros_like(S) if exact else R.score_bound(items, query, mode, d_run)
    plan = plan_of(ra, B, N, k)
    # (a) the plan
    if expect_filter is not None:
        assert plan.filter == expect_filter, f'{tag}: plan.filter = {plan.filter}'
    if designed is not None:                               # the input does what it was built for -- no GPU involved yet
        assert plan.filter == 1
        assert design_classes(S, e, plan, k) == designed, tag
    it_d, q_d = items.to(DEV), query.to(DEV)
    got = run_native(ra, it_d, q_d, k, mode, want_lse=True)
    val, idx, lse = got['val'], got['idx'], got['lse']
    counts = {}
    if plan.filter:
        # (b) every row took the path it was designed for
        paths = R.classify(plan, got['flags'], got['seg_cnt'], got['ovf_cnt'], k)
        causes = R.recompute_cause(plan, got['seg_cnt'], got['ovf_cnt'], k)
        taken = [kernel_class(p, c) for p, c in zip(paths, causes)]
        for p in paths:
            counts[p] = counts.get(p, 0) + 1
        if designed is not None:
            assert taken == designed, f'{tag}: rows took {taken}'
        assert R.check_threshold(got['thr'], S, None if exact else e, plan) == [], tag
        if exact:
            assert R.check_candidates(S, got['thr'], plan, got['seg_cnt'], got['ovf_cnt']) == [], tag
    else:
        counts['dense'] = B
    # (c) the referee
    if exact:
        assert R.check_topk_exact(S, val, idx, k) == [], tag
    assert R.check_topk(S, e, val, idx, k) == [], tag
    if designed is not None and tie_sets is not None:       # a row that sees an all-equal set keeps its smallest ids, in order
        for b, c in enumerate(designed):
            if c in tie_sets and len(tie_sets[c]) >= k:
                assert idx[b].tolist() == (tie_sets[c].sort().values[:k] + 1).tolist(), f'{tag}: row {b} ({c})'
    # (d) the same bits through ops.fullscore
    _, lse_o, val_o, idx_o = ra.ops.fullscore(it_d, q_d, want_lse=True, k=k, score_mode=mode)
    assert torch.equal(val_o.cpu(), val) and torch.equal(idx_o.cpu(), idx) and torch.equal(lse_o.cpu(), lse), tag
    # (e) the same top-k with and without the fused logsumexp
    bare = run_native(ra, it_d, q_d, k, mode, want_lse=False)
    assert torch.equal(bare['val'], val) and torch.equal(bare['idx'], idx), tag
    if plan.filter:
        for name in ('thr', 'flags', 'seg_cnt', 'ovf_cnt'):
            assert torch.equal(bare[name], got[name]), f'{tag}: {name} differs without lse'
    # (f) the logsumexp
    want_lse = torch.logsumexp(S, -1)
    lb = R.lse_bound(S, e, plan)
    lse_share = float(((lse.double() - want_lse).abs() / lb).max())
    col = (idx - 1).clamp(0, N - 2)
    if exact:
        score_share = 0.0
    else:
        score_share = float(((val.double() - S.gather(1, col)).abs() / e.gather(1, col)).max())
    report(f'{tag}: plan={"filter" if plan.filter else "dense"} rows={counts} score_share={score_share:.3f} lse_share={lse_share:.4f}')
    assert lse_share <= 1.0, f'{tag}: lse off by {lse_share:.3f} of its bound'
    return counts


# ------------------------------------------------------------------ the filter plan: all paths in one call
MIXED = [
    # kind, mode, d, N, B, k
    ('gauss', 'ip', 32, 100_011, 129, 10),
    ('gauss', 'cos', 32, 100_011, 129, 10),
    ('gauss', 'euc', 32, 100_011, 129, 10),
    ('grid', 'ip', 32, 140_001, 5, 64),
    ('grid', 'euc', 32, 140_001, 5, 64),
    ('grid', 'ip', 32, 165_001, 5, 100),
    ('grid', 'ip', 32, 100_001, 129, 10),
    ('gauss', 'cos', 32, 165_001, 5, 100),
    ('grid', 'euc', 32, 100_001, 5, 1),
    ('gauss', 'ip', 128, 100_011, 5, 10),
    ('gauss', 'euc', 100, 100_001, 5, 10),
]


@pytest.mark.parametrize('kind,mode,d,N,B,k', MIXED)
def test_filter_plan_every_path_in_one_call(ra, kind, mode, d, N, B, k):
    """The smallest catalogs on the filter plan (the values come from rsa_fullscore_plan, nothing is hard-coded), d = 32 plus one
    d = 128 and one padded d = 100 -> 128; B = 129 puts one live row into a second query group; N - 1 = 100 010 and 165 000 end
    in a partial tile.  Every row's class is asserted twice: from the referee before the call (design_classes) and from the
    workspace after it.  Integer grids (inner product, Euclidean) are exact: top-k, threshold and every segment count bit for bit."""
    plan = plan_of(ra, B, N, k)
    assert plan.filter == 1                                # (nothing below can be built on a dense plan)
    # five rows: one of each class but one; 129 rows: all six in turn, row 128 (alone in the second query group) on the overflow list
    classes = list(CLASSES) if B >= 6 else ['direct', 'radix', 'overflow', 'list_full', 'too_few'] if k > 1 else \
        ['direct', 'radix', 'overflow', 'too_many', 'list_full']
    items, query, sets, _ = steering_inputs(plan, N, d, B, kind, classes, seed=N + B + k + d)
    designed = [classes[b % len(classes)] for b in range(B)]
    assert designed[-1] != 'direct' or B < 6
    ties = {c: sets[c] for c in ('radix', 'too_many', 'list_full', 'too_few')}
    counts = verify(ra, f'mixed {kind} {mode} d={d} N={N} B={B} k={k}', items, query, k, MODES[mode], kind, 1, designed, ties)
    assert counts.get('recompute', 0) >= 2 and counts.get('direct', 0) >= 1 and counts.get('radix', 0) >= 1
    assert sum(v for p, v in counts.items() if p.endswith('+overflow')) >= 1


@pytest.mark.parametrize('mode', ['ip', 'euc'])
def test_filter_plan_single_row(ra, mode):
    """B = 1: one Gaussian row on the direct path and one steered onto the overflow list, k = 1 at the smallest filtered catalog."""
    N, d, k = 100_001, 32, 1
    plan = plan_of(ra, 1, N, k)
    for cls in ('direct', 'overflow'):
        items, query, _, _ = steering_inputs(plan, N, d, 1, 'grid' if mode == 'euc' else 'gauss', [cls], seed=17)
        verify(ra, f'single {cls} {mode}', items, query, k, MODES[mode], 'grid' if mode == 'euc' else 'gauss', 1, [cls])


@pytest.mark.parametrize('mode', ['ip', 'cos', 'euc'])
def test_filter_plan_all_equal_catalog_and_zero_query(ra, mode):
    """Too few candidates the plain way: every item the same row (all scores of a query equal, in every mode), and for the inner
    product a zero query over a Gaussian catalog.  Nothing is strictly above the threshold; the exact recompute returns ids 1..k."""
    N, d, B, k = 100_001, 32, 5, 10
    g = torch.Generator().manual_seed(23)
    items = (torch.randn(1, d, generator=g) * 0.5).expand(N, d).contiguous()
    query = torch.randn(B, d, generator=g) * 0.5
    m = MODES[mode]
    tag = f'all-equal {mode}'
    got = run_native(ra, items.to(DEV), query.to(DEV), k, m, want_lse=True)
    plan = got['plan']
    assert plan.filter == 1
    assert R.classify(plan, got['flags'], got['seg_cnt'], got['ovf_cnt'], k) == ['recompute'] * B, tag
    assert R.recompute_cause(plan, got['seg_cnt'], got['ovf_cnt'], k) == ['too_few'] * B, tag
    assert int(got['seg_cnt'].sum()) == 0 and int(got['ovf_cnt'].sum()) == 0
    assert torch.equal(got['idx'], torch.arange(1, k + 1).expand(B, k)), tag
    S, e = R.scores64(items, query, m), R.score_bound(items, query, m, d)
    # one value per row; the threshold (matrix cores) and the recompute (a scalar fma chain) round it their own ways
    assert bool((got['val'] == got['val'][:, :1]).all()), tag
    assert bool(((got['thr'].double() - got['val'][:, 0].double()).abs() <= 2.0 * e.max(-1).values).all()), tag
    assert R.check_threshold(got['thr'], S, e, plan) == [], tag
    assert R.check_topk(S, e, got['val'], got['idx'], k) == [], tag
    lb = R.lse_bound(S, e, plan)
    share = float(((got['lse'].double() - torch.logsumexp(S, -1)).abs() / lb).max())
    report(f'{tag}: rows={{"recompute": {B}}} lse_share={share:.4f}')
    assert share <= 1.0
    if mode == 'ip':
        items = torch.randn(N, d, generator=g) * 0.5
        query = torch.zeros(B, d)
        query[1:] = torch.randn(B - 1, d, generator=g) * 0.5
        got = run_native(ra, items.to(DEV), query.to(DEV), k, m, want_lse=False)
        paths = R.classify(got['plan'], got['flags'], got['seg_cnt'], got['ovf_cnt'], k)
        assert paths[0] == 'recompute' and paths[1:] == ['direct'] * (B - 1), paths
        assert got['idx'][0].tolist() == list(range(1, k + 1)) and not bool(got['val'][0].any())
        assert R.check_topk(R.scores64(items, query, m), R.score_bound(items, query, m, d), got['val'], got['idx'], k) == []


# ------------------------------------------------------------------ the dense plan
@pytest.mark.parametrize('mode', ['ip', 'euc'])
@pytest.mark.parametrize('n_cols', [1, 33, 1025, 32_767, 32_768])
def test_dense_plan_integer_grid_exact(ra, n_cols, mode):
    """Integer grid, exact: catalogs up to the first size past the smallest filtered one (whatever plan it gets is asserted to be
    the plan the native seam reports, and the result is checked either way); k = 1 and the largest k; a block of identical items
    that outscores the rest for row 0, larger than k, so that the k-th value lies inside a tie group of more than k items."""
    N, d, B = n_cols + 1, 32, 5
    g = torch.Generator().manual_seed(n_cols)
    items = torch.randint(-2, 3, (N, d), generator=g).float()
    query = torch.randint(-2, 3, (B, d), generator=g).float()
    items[0] = 9.0
    hot = torch.arange(0, n_cols, 2)[:1500]               # every second item, up to 1500: identical rows
    items[1 + hot] = 2.0
    query[0] = 2.0                                         # row 0: the block scores 128, the most the grid allows
    for k in sorted({1, min(1024, n_cols)}):
        plan = plan_of(ra, B, N, k)
        if n_cols < 32_768:
            assert plan.filter == 0
        counts = verify(ra, f'dense grid {mode} N={N} k={k}', items, query, k, MODES[mode], 'grid', plan.filter)
        assert ('dense' in counts) == (plan.filter == 0)
        if len(hot) > k:                                    # (also part of check_topk_exact; spelled out)
            got = run_native(ra, items.to(DEV), query.to(DEV), k, MODES[mode], want_lse=False)
            assert got['idx'][0].tolist() == (hot[:k] + 1).tolist()


# ------------------------------------------------------------------ rsa_topk_mask_history
@pytest.mark.parametrize('kc', [1, 63, 64, 65, 200])
def test_mask_history_against_the_referee(ra, kc):
    g = torch.Generator().manual_seed(kc)
    for k in sorted({1, kc, kc - 3} - {0, -1, -2}):
        B, hl = 7, kc + 3
        cv = torch.randn(B, kc, generator=g).sort(-1, descending=True).values
        cv[:, kc // 2:kc // 2 + 2] = cv[:, kc // 2:kc // 2 + 1]                  # two equal neighbours
        ci = torch.stack([torch.randperm(5 * kc + 5, generator=g)[:kc] + 1 for _ in range(B)])
        hist = torch.zeros(B, hl, dtype=torch.int64)

        def mask(b, which):
            ids = ci[b, which]
            hist[b, torch.randperm(hl, generator=g)[:len(ids)]] = ids          # scattered over the columns, zeros between

        hist[1, 0], hist[1, 1], hist[1, hl - 1] = ci[1, 0], ci[1, kc - 1], ci[1, 0]    # first and last candidate, a repeat, zeros
        mask(2, torch.randperm(kc, generator=g)[:kc - k])                       # exactly k survivors
        mask(3, torch.randperm(kc, generator=g)[:kc - k + 1])                   # k - 1 survivors
        mask(4, torch.arange(kc))                                               # none
        mask(5, torch.randperm(kc, generator=g)[:kc // 2])
        hist[6] = 5 * kc + 100                                                  # a full history that hits nothing
        hist[6, hl - 1] = ci[6, 0]                                              # ... but for its last column
        ref = R.mask_history64(cv, ci, hist, k)
        assert [len(r[0]) for r in ref][2:5] == [k, k - 1, 0]
        ov, oi = ra.ops.topk_mask_history(cv.to(DEV), ci.to(DEV), hist.to(DEV), k)
        assert R.check_mask_history(ov.cpu(), oi.cpu(), ref) == [], f'kc={kc} k={k}'
