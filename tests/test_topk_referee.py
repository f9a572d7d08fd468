"""CPU: the top-k referee (tests/topk_referee.py) accepts a correct top-k and names the rule that catches each seeded mistake;
rsa_fullscore_plan (host only) is pinned to the plans the GPU cases of tests/test_gpu_topk_paths.py are built on."""
import math
from types import SimpleNamespace

import pytest
import torch

import topk_referee as R

# a filter plan in miniature: 2000 items, every 5th tile sampled (12 of them), groups of 2 sampled tiles, threshold = 3rd largest
# group maximum; 21 item ranges of 96 items, segments of 4 slots, an overflow list of 16, at most 64 candidates
PLAN = SimpleNamespace(filter=1, sample_tiles=12, tile_stride=5, group_tiles=2, groups=6, j=3, items_per_split=96, splits=21,
                       n_seg=42, seg=4, ovf=16, cand_max=64)
N_COLS, D, K = 2000, 32, 10


def gaussian(seed=0, B=5, n=N_COLS, d=D):
    g = torch.Generator().manual_seed(seed)
    items = torch.randn(n + 1, d, generator=g) * 0.5
    items[0] = 9.0                                    # the padding row would win every row if it were scored
    return items, torch.randn(B, d, generator=g) * 0.5


def grid(seed=0, B=5, n=N_COLS, d=D):
    g = torch.Generator().manual_seed(seed)
    items = torch.randint(-2, 3, (n + 1, d), generator=g).float()
    return items, torch.randint(-2, 3, (B, d), generator=g).float()


def fp32_scores(items, query, mode):
    """what a correct fp32 kernel computes, by the epilogue's own formulas"""
    w = items[1:]
    dot = query @ w.T
    if mode == R.IP:
        return dot
    if mode == R.COS:
        return dot * (1.0 / (w * w).sum(-1).sqrt()) * (1.0 / (query * query).sum(-1).sqrt()).unsqueeze(-1)
    return (2.0 * dot - (w * w).sum(-1)) - (query * query).sum(-1, keepdim=True)


def topk_of(scores, k, larger_id_first=False):
    """a correct select over fp32 scores: value descending, id ascending (or the seeded opposite)"""
    s = scores.flip(-1) if larger_id_first else scores
    order = torch.sort(s, dim=-1, descending=True, stable=True).indices[:, :k]
    if larger_id_first:
        order = scores.shape[1] - 1 - order
    return scores.gather(1, order), order + 1


@pytest.mark.parametrize('mode', [R.IP, R.COS, R.EUC])
def test_correct_topk_is_accepted_and_the_bound_holds(mode):
    items, q = gaussian(mode)
    S, e = R.scores64(items, q, mode), R.score_bound(items, q, mode, D)
    got = fp32_scores(items, q, mode)
    share = ((got.double() - S).abs() / e).max()
    assert 0 < share <= 1.0                            # a bound, and not a vacuous one for torch's own fp32 arithmetic
    assert float(e.max()) < 1e-4
    val, idx = topk_of(got, K)
    assert R.check_topk(S, e, val, idx, K) == []
    assert R.check_threshold(R.threshold64(got.double(), PLAN).float(), S, e, PLAN) == []
    lse = torch.logsumexp(got, -1)
    assert bool(((lse.double() - torch.logsumexp(S, -1)).abs() <= R.lse_bound(S, e, PLAN)).all())
    assert float(R.lse_bound(S, e, PLAN).max()) < 1e-4


def test_scores64_is_the_oracle():
    import oracle
    items, q = gaussian(7)
    for mode, fn in ((R.IP, oracle.inner_product_score), (R.COS, oracle.cosine_score), (R.EUC, oracle.euclidean_score)):
        torch.testing.assert_close(R.scores64(items, q, mode), fn(q.double(), items[1:].double()), rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize('mode', [R.IP, R.EUC])
def test_integer_grid_scores_are_exact_in_fp32(mode):
    items, q = grid(1)
    S = R.scores64(items, q, mode)
    got = fp32_scores(items, q, mode)
    assert torch.equal(got.double(), S)                # integers below 2^24: any summation order gives these bits
    val, idx = topk_of(got, K)
    assert R.check_topk_exact(S, val, idx, K) == []
    assert R.check_topk(S, torch.zeros_like(S), val, idx, K) == []
    assert int((val[:, 1:] == val[:, :-1]).sum()) > 0  # the grid is full of ties
    assert R.check_threshold(R.threshold64(got.double(), PLAN).float(), S, None, PLAN) == []


# ------------------------------------------------------------------ seeded mistakes, each caught by the rule aimed at it
def test_mistake_ties_broken_by_larger_id():
    items, q = grid(2)
    S = R.scores64(items, q, R.IP)
    val, idx = topk_of(S.float(), K, larger_id_first=True)
    assert 'ids_exact' in R.check_topk_exact(S, val, idx, K) and 'values_exact' not in R.check_topk_exact(S, val, idx, K)
    assert 'tie_order' in R.check_topk(S, torch.zeros_like(S), val, idx, K)


def test_mistake_winner_dropped_from_a_full_segment():
    items, q = gaussian(3)
    q[:, 0] = q[:, 0].abs() + 0.5
    # six items of one segment (tile 1 is not sampled; rows 0..3, 8, 9 belong to lane half 0), the best one last in id order
    cols = torch.tensor([32, 33, 34, 35, 40, 41])
    items[1 + cols] = 0.0
    items[1 + cols, 0] = torch.tensor([20., 21., 22., 23., 24., 25.])
    S, e = R.scores64(items, q, R.IP), R.score_bound(items, q, R.IP, D)
    got = fp32_scores(items, q, R.IP)
    thr = R.threshold64(S, PLAN)
    assert bool((got[:, cols] > thr.float().unsqueeze(-1)).all()) and bool((got.argmax(-1) == 41).all())
    # a segment that has `seg` slots and no overflow list loses its later candidates
    lossy = got.clone()
    lossy[:, cols[PLAN.seg:]] = -math.inf
    val, idx = topk_of(lossy, K)
    assert 'winners_present' in R.check_topk(S, e, val, idx, K)
    # ... and the bookkeeping check sees a segment that reports fewer candidates than it has
    want = R.segment_counts64(S, thr, PLAN)
    seg_cnt, ovf = want.clamp(max=PLAN.seg), (want - PLAN.seg).clamp(min=0).sum(-1)
    assert R.check_candidates(S, thr, PLAN, seg_cnt, ovf) == []
    busy = int(want[0].argmax())
    seg_cnt[0, busy] -= 1
    assert R.check_candidates(S, thr, PLAN, seg_cnt, ovf) == ['segment_counts']
    seg_cnt[0, busy] += 1
    assert R.check_candidates(S, thr, PLAN, seg_cnt, ovf + 1) == ['overflow_count']


def test_mistake_greater_equal_at_the_threshold_with_a_tie_at_kth():
    items, q = grid(4)
    S = R.scores64(items, q, R.IP)
    wv, wi = R.stable_topk(S, K)
    vk = wv[:, -1:]
    longer = (S == vk).sum(-1) > (wv == vk).sum(-1)                      # rows whose k-th value lies inside a longer tie group
    assert int(longer.sum()) >= 2
    # select: every key >= the k-th key taken as a winner, the first k in sorted order kept -- the ties of the k-th value come out
    # in the order the collection found them (here: from the end of the row), not the smallest ids
    val, idx = wv.clone().float(), wi.clone()
    for b in longer.nonzero().flatten().tolist():
        ties = (S[b] == vk[b]).nonzero().flatten() + 1
        n_tie = int((wv[b] == vk[b]).sum())
        idx[b, K - n_tie:] = ties[-n_tie:]
    assert R.check_topk_exact(S, val, idx, K) == ['ids_exact']
    assert R.check_topk(S, torch.zeros_like(S), val, idx, K) == []       # (a tolerance rule cannot see it: the exact referee must)
    # filter: score >= thr emits the threshold's own tie group as candidates
    thr = R.threshold64(S, PLAN)
    ge = torch.zeros(S.shape[0], PLAN.n_seg, dtype=torch.int64)
    c = torch.arange(N_COLS)
    seg = (c // PLAN.items_per_split) * 2 + (((c % R.TI) >> 2) & 1)
    ge.scatter_add_(1, seg.expand_as(S), (S >= thr.unsqueeze(-1)).long())
    assert 'segment_counts' in R.check_candidates(S, thr, PLAN, ge.clamp(max=PLAN.seg), (ge - PLAN.seg).clamp(min=0).sum(-1))


def test_mistake_item_id_off_by_one():
    items, q = gaussian(5)
    S, e = R.scores64(items, q, R.IP), R.score_bound(items, q, R.IP, D)
    val, idx = topk_of(fp32_scores(items, q, R.IP), K)
    assert 'values_match' in R.check_topk(S, e, val, idx - 1, K)          # column reported instead of item id
    items, q = grid(5)
    S = R.scores64(items, q, R.IP)
    val, idx = topk_of(S.float(), K)
    assert R.check_topk_exact(S, val, idx - 1, K) == ['ids_exact']


def test_mistake_padding_row_scored():
    items, q = gaussian(6)
    q = q.abs()                                                           # the padding row (all 9) then beats every item
    S, e = R.scores64(items, q, R.IP), R.score_bound(items, q, R.IP, D)
    with_pad = q @ items.T                                                # column c = item id c
    val, idx = topk_of(with_pad, K)
    idx = idx - 1
    assert bool((idx[:, 0] == 0).all())
    assert 'ids_in_range' in R.check_topk(S, e, val, idx, K)


def test_mistake_last_partial_tile_skipped():
    items, q = gaussian(8)
    assert N_COLS % R.TI != 0
    last = N_COLS // R.TI * R.TI
    items[1 + last:] *= 3.0
    items[1 + last:, 0] = q[:, 0].sign().mode().values * 4.0
    S, e = R.scores64(items, q, R.IP), R.score_bound(items, q, R.IP, D)
    got = fp32_scores(items, q, R.IP)
    assert bool((got.argmax(-1) >= last).any())                           # some row's best item lives in the partial tile
    val, idx = topk_of(got[:, :last], K)
    assert 'winners_present' in R.check_topk(S, e, val, idx, K)


def test_mistake_value_of_the_neighbouring_id():
    items, q = gaussian(9)
    S, e = R.scores64(items, q, R.IP), R.score_bound(items, q, R.IP, D)
    got = fp32_scores(items, q, R.IP)
    val, idx = topk_of(got, K)
    val = got.gather(1, idx.clamp(max=N_COLS - 1))                        # column idx = item idx + 1
    assert 'values_match' in R.check_topk(S, e, val, idx, K)


@pytest.mark.parametrize('mode', [R.COS, R.EUC])
def test_mistake_recompute_forgets_query_aux(mode):
    items, q = gaussian(10)
    S, e = R.scores64(items, q, mode), R.score_bound(items, q, mode, D)
    w = items[1:]
    dot = q @ w.T
    wrong = dot * (1.0 / (w * w).sum(-1).sqrt()) if mode == R.COS else 2.0 * dot - (w * w).sum(-1)
    val, idx = topk_of(wrong, K)                                           # the ranking of a row is still right ...
    assert R.check_topk(S, e, fp32_scores(items, q, mode).gather(1, idx - 1), idx, K) == []
    assert 'values_match' in R.check_topk(S, e, val, idx, K)               # ... the values are not


def test_mistake_threshold_at_rank_j_plus_one():
    items, q = gaussian(11)
    S, e = R.scores64(items, q, R.IP), R.score_bound(items, q, R.IP, D)
    gm = R.group_maxima64(S, PLAN)
    off = torch.sort(gm, dim=-1, descending=True).values[:, PLAN.j]
    assert R.check_threshold(off.float(), S, e, PLAN) == ['threshold']
    items, q = grid(11)
    S = R.scores64(items, q, R.IP)
    gm = R.group_maxima64(S, PLAN)
    srt = torch.sort(gm, dim=-1, descending=True).values
    if bool((srt[:, PLAN.j] != srt[:, PLAN.j - 1]).any()):
        assert R.check_threshold(srt[:, PLAN.j].float(), S, None, PLAN) == ['threshold']
    assert R.check_threshold(srt[:, PLAN.j - 1].float(), S, None, PLAN) == []


def test_group_maxima_cover_exactly_the_sampled_tiles():
    S = torch.zeros(1, N_COLS, dtype=torch.float64)
    sampled = R.sampled_mask(N_COLS, PLAN)
    assert int(sampled.sum()) == PLAN.sample_tiles * R.TI
    S[0, ~sampled] = 5.0                                # unsampled items never move a group maximum
    assert torch.equal(R.group_maxima64(S, PLAN), torch.zeros(1, PLAN.groups, dtype=torch.float64))
    for s in range(PLAN.sample_tiles):
        S.zero_()
        S[0, s * PLAN.tile_stride * R.TI + 31] = 1.0
        gm = R.group_maxima64(S, PLAN)
        assert gm[0].tolist() == [1.0 if g == s // PLAN.group_tiles else 0.0 for g in range(PLAN.groups)]


def test_mask_history_rule_and_the_mistake_that_misses_the_last_column():
    kc, k = 9, 6
    cv = torch.arange(kc, 0, -1).float().unsqueeze(0).repeat(4, 1)
    ci = torch.arange(10, 10 + kc).unsqueeze(0).repeat(4, 1)
    hist = torch.tensor([[0, 0, 0, 0],               # nothing masked
                         [10, 18, 0, 10],            # first and last candidate, a repeat, padding
                         [11, 12, 13, 14],           # kc - 4 = 5 survivors < k: one masked id in the tail
                         [99, 0, 0, 17]])            # only the last column hits
    ref = R.mask_history64(cv, ci, hist, k)

    def apply(h):
        ov, oi = torch.empty(4, k), torch.empty(4, k, dtype=torch.int64)
        for b in range(4):
            m = (ci[b].unsqueeze(-1) == h[b]).any(-1)
            v = torch.where(m, torch.tensor(-math.inf), cv[b])
            tv, sel = torch.sort(v, descending=True, stable=True)
            ov[b], oi[b] = tv[:k], ci[b][sel[:k]]
        return ov, oi
    ov, oi = apply(hist)
    assert R.check_mask_history(ov, oi, ref) == []
    assert oi[1].tolist() == [11, 12, 13, 14, 15, 16] and oi[2, :5].tolist() == [10, 15, 16, 17, 18] and ov[2, 5] == -math.inf
    bad_v, bad_i = apply(hist[:, :-1])
    assert 'kept_ids' in R.check_mask_history(bad_v, bad_i, ref)
    tail = oi.clone()
    tail[2, 5] = 10                                   # a survivor repeated in the tail instead of a masked id
    assert R.check_mask_history(ov, tail, ref) == ['tail_ids']
    fin = ov.clone()
    fin[2, 5] = 0.0
    assert R.check_mask_history(fin, oi, ref) == ['tail_values']


def test_classify_names_the_path_and_checks_the_flag():
    seg_cnt = torch.zeros(6, PLAN.n_seg, dtype=torch.int32)
    ovf = torch.zeros(6, dtype=torch.int32)
    seg_cnt[0, :5] = 3                                # 15 candidates
    seg_cnt[1, :] = 4
    ovf[1] = 16                                       # 42 * 4 + 16 = 184 > cand_max
    seg_cnt[2, :3] = 4
    ovf[2] = 5                                        # 17 candidates, overflow list used
    seg_cnt[3, :2] = 4                                # 8 < k
    seg_cnt[4, :4] = 4
    ovf[4] = 17                                       # list past its 16 slots
    seg_cnt[5, :16] = 4                               # 64 = cand_max: still selected
    flags = torch.tensor([0, 1, 0, 1, 1, 0])
    assert R.classify(PLAN, flags, seg_cnt, ovf, K) == ['direct', 'recompute', 'direct+overflow', 'recompute', 'recompute', 'direct']
    assert R.recompute_cause(PLAN, seg_cnt, ovf, K) == [None, 'too_many', None, 'too_few', 'list_full', None]
    with pytest.raises(AssertionError):
        R.classify(PLAN, torch.zeros(6, dtype=torch.int64), seg_cnt, ovf, K)
    big = SimpleNamespace(**{**vars(PLAN), 'seg': 32, 'ovf': 1024, 'cand_max': 4096})
    seg_cnt[0, :] = 30                                # 1260 candidates
    assert R.classify(big, torch.zeros(1), seg_cnt[:1], ovf[:1], K) == ['radix']


# ------------------------------------------------------------------ the native plan (host only: runs without a GPU)
@pytest.fixture(scope='module')
def nat():
    from recstudio_amd import _native
    if not __import__('os').path.exists(_native.LIB_PATH):
        _native.build()
    return _native


def native_plan(nat, B, N, k):
    info = nat.FullscorePlanInfo()
    nat.check(nat.lib().rsa_fullscore_plan(B, N, k, info), 'rsa_fullscore_plan')
    return info


def test_native_plan_matches_the_launch_arithmetic(nat):
    """The shapes the GPU path tests stand on, and the ones whose docstrings name a plan."""
    for B, N, k, filt in ((1, 100_001, 1, 1), (129, 100_001, 10, 1), (5, 140_001, 64, 1), (5, 165_001, 100, 1),
                          (2048, 300_001, 500, 0), (200, 40_000, 100, 0), (33, 5_000, 10, 0), (130, 70_001, 50, 0),
                          (4, 200_001, 100, 1), (512, 1_000_001, 100, 1), (5, 32_769, 1, 0), (5, 34, 1, 0)):
        p = native_plan(nat, B, N, k)
        assert p.filter == filt, (B, N, k)
        assert (p.seg, p.ovf, p.cand_max, p.group_tiles) == (32, 1024, 4096, 8)
        assert p.items_per_split % 32 == 0 and (p.splits - 1) * p.items_per_split < N - 1 <= p.splits * p.items_per_split
        if filt:
            assert p.n_seg == 2 * p.splits and 1 <= p.j <= p.groups // 2 and p.groups == -(-p.sample_tiles // 8)
            assert p.sample_tiles * p.tile_stride <= -(-(N - 1) // 32) and p.tile_stride >= 4
            offs = [p.thr_offset, p.flags_offset, p.seg_cnt_offset, p.ovf_cnt_offset]
            assert all(o >= 0 and o % 256 == 0 for o in offs) and offs == sorted(offs)
            assert p.flags_offset - p.thr_offset >= 4 * B and p.ovf_cnt_offset - p.seg_cnt_offset >= 4 * B * p.n_seg
            assert p.ovf_cnt_offset + 4 * B <= nat.lib().rsa_fullscore_workspace_bytes(B, N, k)
        else:
            assert p.n_seg == 0 and (p.thr_offset, p.flags_offset, p.seg_cnt_offset, p.ovf_cnt_offset) == (-1, -1, -1, -1)
    assert native_plan(nat, 2048, 300_001, 500).j == 84 and native_plan(nat, 2048, 300_001, 500).groups == 128
    assert native_plan(nat, 512, 1_000_001, 100).j == 14 and native_plan(nat, 4, 200_001, 100).j == 56
    # no top-k: only the launch's ranges
    p = native_plan(nat, 129, 100_001, 0)
    assert p.filter == 0 and p.splits == native_plan(nat, 129, 100_001, 10).splits


def test_native_plan_argument_checks(nat):
    lib = nat.lib()
    assert lib.rsa_fullscore_plan(1, 100, 1, None) == -1 and b'out is null' in lib.rsa_last_error()
    info = nat.FullscorePlanInfo()
    info.size = 0
    assert lib.rsa_fullscore_plan(1, 100, 1, info) == -1 and b'size' in lib.rsa_last_error()
    info = nat.FullscorePlanInfo()
    assert lib.rsa_fullscore_plan(1, 1, 1, info) == -1
    # an older, shorter struct: only its bytes are written
    info = nat.FullscorePlanInfo()
    info.size = nat.FullscorePlanInfo.thr_offset.offset
    info.thr_offset = 12345
    assert lib.rsa_fullscore_plan(4, 200_001, 100, info) == 0
    assert info.filter == 1 and info.cand_max == 4096 and info.thr_offset == 12345 and info.size == nat.FullscorePlanInfo.thr_offset.offset
