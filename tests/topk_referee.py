"""Float64 referee of the full-catalog top-k (csrc/rsa_fullscore.hip) and of rsa_topk_mask_history: the scores of the three
scorers from the oracle's formulas, a worst-case bound on what the fp32 kernels may differ from them by, the acceptance rules of
a top-k result (with that bound, and bit for bit where the scores are exact in fp32), the threshold of the filter plan, the
per-segment candidate counts, the path a row took as the select's bookkeeping records it, and the history mask.

Everything is plain torch in float64 / int64 and runs on whatever device its inputs live on.  A *plan* is anything with the
fields of ``rsa_fullscore_plan_info`` (the ctypes struct itself, in the tests).  ``items`` always carries the padding row 0;
score column c belongs to item id c + 1.  The checkers return the NAMES of the rules a result breaks (an empty list: accepted),
so that tests/test_topk_referee.py can ask which rule catches which mistake."""
import math

import torch

IP, COS, EUC = 0, 1, 2          # rsa_score_mode
TI = 32                         # items per MFMA tile
U = 2.0 ** -24                  # unit roundoff of fp32, round to nearest


def gamma(n):
    """Higham's gamma_n = n u / (1 - n u): (1 + d_1) ... (1 + d_n) = 1 + theta with |theta| <= gamma_n when every |d_i| <= u."""
    return n * U / (1.0 - n * U)


def sqnorm_roundings(dim):
    """Roundings a term x_c^2 passes through in row_sqnorm_kernel (csrc/rsa_misc.hip): dot4 is one rounded product and three
    fmas (4), the lane adds its ceil(dim / 4 / 64) dot4 values (one rounding each), the 64-lane butterfly adds six times."""
    return 4 + -(-(dim // 4) // 64) + 6


# ------------------------------------------------------------------ scores and their fp32 error bound
def _operands(items, query):
    w, q = items[1:].double(), query.double()
    return w, q, q @ w.T, (w * w).sum(-1), (q * q).sum(-1)


def scores64(items, query, mode):
    """[B, N - 1] float64 scores of ``query`` against rows 1.. of ``items``: inner product (scorer.py:16), cosine = <q, w> /
    |w| / |q| (scorer.py:19-25), Euclidean = -(-2 <q, w> + |w|^2 + |q|^2) (scorer.py:28-34)."""
    w, q, dot, wn, qn = _operands(items, query)
    if mode == IP:
        return dot
    if mode == COS:
        return dot / wn.sqrt() / qn.sqrt().unsqueeze(-1)
    return -(-2.0 * dot + wn + qn.unsqueeze(-1))


def score_bound(items, query, mode, d):
    """[B, N - 1] float64 bound on |fp32 kernel score - scores64| per element.  ``d``: the accumulation length of the kernel's
    dot product (the padded dim it runs at); the squared norms are taken by rsa_row_sqnorm over the columns ``items`` has.

    Inner product.  The kernel's dot is a sum of d products in which a term passes through at most d roundings whatever the
    order of the FMA / MFMA accumulation, so |dot^ - dot| <= eps := gamma_d * sum_c |q_c w_c|  (Higham, Accuracy and Stability,
    3.1; zero padding adds exact zeros).  The scalar chain of the exact recompute obeys the same bound.

    Squared norms.  n^ = |x|^2 (1 + t), |t| <= gamma_m with m = sqnorm_roundings(dim).

    Cosine.  aux^ = 1 / sqrt(n^): a correctly rounded sqrt and a correctly rounded division on top of (1 + t)^(-1/2), whose
    distance from 1 is below gamma_m: aux^ = aux (1 + t'), |t'| <= gamma_{m + 2}.  The epilogue multiplies twice (dot * item_aux *
    query_aux): score^ = (dot + e) * ia * qa * (1 + T), |T| <= gamma_{2 (m + 2) + 2}, hence
        |score^ - score| <= ia qa (eps (1 + gamma_T) + |dot| gamma_T).

    Euclidean.  t1 = fma(2, dot^, -I^) and score^ = t1 - Q^, one rounding each, I^ = I (1 + t_i), Q^ = Q (1 + t_q):
        e1 = 2 eps + gamma_m I;   |t1 - (2 dot - I)| <= e1' := e1 + u (|2 dot - I| + e1)
        |score^ - score| <= e2 + u (|score| + e2),   e2 = e1' + gamma_m Q."""
    w, q, dot, wn, qn = _operands(items, query)
    eps = gamma(d) * (q.abs() @ w.abs().T)
    if mode == IP:
        return eps
    m = sqnorm_roundings(items.shape[1])
    if mode == COS:
        g = gamma(2 * (m + 2) + 2)
        scale = 1.0 / wn.sqrt() / qn.sqrt().unsqueeze(-1)
        return scale * (eps * (1.0 + g) + dot.abs() * g)
    qn = qn.unsqueeze(-1)
    e1 = 2.0 * eps + gamma(m) * wn
    e1 = e1 + U * ((2.0 * dot - wn).abs() + e1)
    e2 = e1 + gamma(m) * qn
    return e2 + U * ((2.0 * dot - wn - qn).abs() + e2)


def lse_bound(S, e, plan):
    """[B] bound on |fp32 logsumexp - logsumexp(S)| of the kernel's online logsumexp, from the score bound ``e`` and the launch
    (plan.items_per_split, plan.splits).

    Moving every score by at most E = max e moves the logsumexp by at most E.  On top of that the kernel evaluates
    m + log(sum_i 2^((s_i - m) log2 e)) in fp32; with R the spread of the row's scores (max - min, + 2 E) and M = max |s| + E,
    the relative error of a term of the sum is, to first order, u times
        2 + (2 R + M)         v_exp_f32 (1 ulp = 2 u) and its argument fma(s, L, -fl(m L)) with L = fl(log2 e)
      + T (4 + 2 R + M)       the T = items_per_split / 32 later tiles of its lane: a rescale by exp2 of such an argument, a
                              multiply, an add
      + items_per_split / 2   the adds inside the tiles (a lane half owns 16 of a tile's 32 items)
      + 5 + 2 R               folding the two lane halves: __expf(run_m - m), multiply, add
      + splits + 3 + R        lse_merge_kernel: expf(p.x - m), multiply, `splits` sequential adds
    =: rho / u; log moves by at most rho / (1 - rho).  logf (1 ulp) and the final add cost 2 u ln N + u |lse|."""
    B, n = S.shape
    E = e.max(-1).values
    smax, smin = S.max(-1).values, S.min(-1).values
    R = smax - smin + 2.0 * E
    M = torch.maximum(smax.abs(), smin.abs()) + E
    per, splits = float(plan.items_per_split), float(plan.splits)
    T = per / TI
    rho = U * (2.0 + (2.0 * R + M) + T * (4.0 + 2.0 * R + M) + per / 2.0 + (5.0 + 2.0 * R) + (splits + 3.0 + R))
    lse = torch.logsumexp(S, -1)
    return E + rho / (1.0 - rho) + 2.0 * U * math.log(max(n, 2)) + U * (lse.abs() + E)


# ------------------------------------------------------------------ acceptance rules of a top-k result
def stable_topk(S, k):
    """(values, item ids) of the k largest per row in the order the kernels promise: value descending, id ascending."""
    order = torch.sort(S, dim=-1, descending=True, stable=True).indices[:, :k]
    return S.gather(1, order), order + 1


def check_topk(S, e, val, idx, k):
    """The rules a top-k result (val [B, k] float32, idx [B, k] int64 item ids) must obey given float64 scores S [B, N - 1]
    and the per-element bound e [B, N - 1] on the kernel's score error.  With v_k the k-th largest of S in a row and E the row's
    largest bound -- the kernel's k-th value lies within E of v_k, and it ranks by scores that are each within E of S:
      ids_in_range     ids lie in [1, N)
      ids_distinct
      values_match     |val - S[idx]| <= e[idx]
      sorted           val is non-increasing
      tie_order        equal neighbouring val have ascending ids
      winners_present  every item with S > v_k + 2 E is present
      no_losers        no item with S < v_k - 2 E is present"""
    B, n = S.shape
    failed = []
    idx = idx.long()
    val = val.double()
    in_range = (idx >= 1) & (idx <= n)
    if not bool(in_range.all()):
        failed.append('ids_in_range')
    col = (idx - 1).clamp(0, n - 1)
    if bool((torch.sort(idx, dim=-1).values.diff(dim=-1) == 0).any()):
        failed.append('ids_distinct')
    if not bool(((val - S.gather(1, col)).abs() <= e.gather(1, col)).all()):
        failed.append('values_match')
    if k > 1:
        dv = val.diff(dim=-1)
        if bool((dv > 0).any()):
            failed.append('sorted')
        if bool(((dv == 0) & (idx.diff(dim=-1) <= 0)).any()):
            failed.append('tie_order')
    vk = torch.topk(S, k, dim=-1).values[:, -1:]
    E = e.max(-1, keepdim=True).values
    present = torch.zeros(B, n, dtype=torch.bool, device=S.device)
    present.scatter_(1, col, in_range)
    if bool(((S > vk + 2.0 * E) & ~present).any()):
        failed.append('winners_present')
    if bool(((S < vk - 2.0 * E) & present).any()):
        failed.append('no_losers')
    return failed


def check_topk_exact(S, val, idx, k):
    """For scores that are exact in fp32 (integer-valued inputs): there is one right answer.
      values_exact   val == the k largest of S, bit for bit
      ids_exact      idx == their ids in (value descending, id ascending) order"""
    wv, wi = stable_topk(S, k)
    failed = []
    if not torch.equal(val.double(), wv):
        failed.append('values_exact')
    if not torch.equal(idx.long(), wi):
        failed.append('ids_exact')
    return failed


# ------------------------------------------------------------------ the filter plan: threshold, candidates, paths
def group_maxima64(S, plan):
    """[B, plan.groups] maxima of the sample pass: group g = sampled tiles [g * group_tiles, (g + 1) * group_tiles) (the last
    group may be shorter), sample tile s = items 1 + s * tile_stride * 32 + [0, 32), i.e. score columns from s * tile_stride * 32."""
    B, n = S.shape
    st, ts, gt, groups = int(plan.sample_tiles), int(plan.tile_stride), int(plan.group_tiles), int(plan.groups)
    assert groups == -(-st // gt)
    start = torch.arange(st, device=S.device) * (ts * TI)
    cols = start.unsqueeze(-1) + torch.arange(TI, device=S.device)            # [st, 32]
    assert int(cols.max()) < n, 'a sampled tile reaches past the catalog'
    tile_max = S[:, cols.reshape(-1)].reshape(B, st, TI).max(-1).values       # [B, st]
    pad = groups * gt - st
    if pad:
        tile_max = torch.cat([tile_max, tile_max.new_full((B, pad), -math.inf)], -1)
    return tile_max.reshape(B, groups, gt).max(-1).values


def threshold64(S, plan):
    """[B] the plan.j-th largest group maximum, ranked (value descending, group index ascending) as group_threshold_kernel does
    (the index only orders equal values: the VALUE at rank j is what a sort gives)."""
    gm = group_maxima64(S, plan)
    return torch.sort(gm, dim=-1, descending=True, stable=True).values[:, int(plan.j) - 1]


def check_threshold(thr, S, e, plan):
    """threshold: |thr - threshold64| <= the row's largest bound (a rank statistic moves by at most what its elements move by);
    pass e = None for exact scores: bit-equal."""
    want = threshold64(S, plan)
    if e is None:
        return [] if torch.equal(thr.double(), want) else ['threshold']
    return [] if bool(((thr.double() - want).abs() <= e.max(-1).values).all()) else ['threshold']


def sampled_mask(n_cols, plan, device=None):
    """[n_cols] bool: the score column lies in a sampled tile"""
    tile = torch.arange(n_cols, device=device) // TI
    return (tile % int(plan.tile_stride) == 0) & (tile // int(plan.tile_stride) < int(plan.sample_tiles))


def segment_counts_of(above, plan):
    """[B, plan.n_seg] how many of the columns marked in ``above`` [B, N - 1] each (item range, lane half) segment sees: item
    column c lies in range c // items_per_split, and row r = c % 32 of its tile belongs to lane half (r >> 2) & 1 (ranges are
    whole tiles)."""
    B, n = above.shape
    c = torch.arange(n, device=above.device)
    seg = (c // int(plan.items_per_split)) * 2 + (((c % TI) >> 2) & 1)
    cnt = torch.zeros(B, int(plan.n_seg), dtype=torch.int64, device=above.device)
    cnt.scatter_add_(1, seg.expand(B, n), above.long())
    return cnt


def segment_counts64(S, thr, plan):
    """the candidates (score > thr, strictly) of every segment"""
    return segment_counts_of(S > thr.double().unsqueeze(-1), plan)


def check_candidates(S, thr, plan, seg_cnt, ovf_cnt):
    """For exact scores: the filter epilogue's bookkeeping has one right value.
      segment_counts   seg_cnt == min(candidates of the segment, seg)
      overflow_count   ovf_cnt == the candidates that did not fit their segments"""
    want = segment_counts64(S, thr, plan)
    failed = []
    if not torch.equal(seg_cnt.long(), want.clamp(max=int(plan.seg))):
        failed.append('segment_counts')
    if not torch.equal(ovf_cnt.long(), (want - int(plan.seg)).clamp(min=0).sum(-1)):
        failed.append('overflow_count')
    return failed


def candidate_totals(plan, seg_cnt, ovf_cnt):
    """[B] candidates the select compacts: the segments' (at most seg each) plus the overflow list's (at most ovf)"""
    return seg_cnt.long().clamp(max=int(plan.seg)).sum(-1) + ovf_cnt.long().clamp(max=int(plan.ovf))


def classify(plan, flags, seg_cnt, ovf_cnt, k):
    """The path of every row of a filter-plan call, from what the select left in the workspace: 'recompute' (flagged), else
    'direct' (at most 1024 candidates: bitonic sort only) or 'radix' (1025 .. cand_max), with '+overflow' appended when the
    row's overflow list was used.  The flag itself is checked against the rule that sets it."""
    total = candidate_totals(plan, seg_cnt, ovf_cnt).tolist()
    out = []
    for f, t, o in zip(flags.tolist(), total, ovf_cnt.tolist()):
        bad = o > int(plan.ovf) or t < k or t > int(plan.cand_max)
        assert bool(f) == bad, f'flag {f} but {t} candidates, {o} overflow appends, k = {k}'
        if bad:
            out.append('recompute')
        else:
            out.append(('direct' if t <= 1024 else 'radix') + ('+overflow' if o > 0 else ''))
    return out


def recompute_cause(plan, seg_cnt, ovf_cnt, k):
    """why each row would be flagged: 'list_full', 'too_few', 'too_many' or None"""
    total = candidate_totals(plan, seg_cnt, ovf_cnt).tolist()
    return ['list_full' if o > int(plan.ovf) else 'too_few' if t < k else 'too_many' if t > int(plan.cand_max) else None
            for t, o in zip(total, ovf_cnt.tolist())]


# ------------------------------------------------------------------ history mask
def mask_history64(cand_val, cand_idx, hist, k):
    """BaseRetriever.topk's rule (baseretriever.py:386-392) for candidates sorted descending: a candidate found in the row's
    history gets -inf, the k best survivors come first in order, masked ids fill the tail only when fewer than k survive.
    Per row: (kept values, kept ids) of the min(k, survivors) leading slots and the masked ids, in candidate order."""
    rows = []
    for v, i, h in zip(cand_val, cand_idx, hist):
        masked = (i.unsqueeze(-1) == h.unsqueeze(0)).any(-1)
        rows.append((v[~masked][:k], i[~masked][:k], i[masked]))
    return rows


def check_mask_history(out_val, out_idx, ref):
    """kept_values / kept_ids: exact.  tail_values: -inf.  tail_ids: distinct masked candidates (all of them when they all fit:
    the reference's topk over equal -inf scores picks no particular ones either)."""
    failed = set()
    k = out_val.shape[1]
    for ov, oi, (kv, ki, masked) in zip(out_val, out_idx, ref):
        s = len(kv)
        if not torch.equal(ov[:s], kv):
            failed.add('kept_values')
        if not torch.equal(oi[:s], ki):
            failed.add('kept_ids')
        if s < k:
            if not bool((ov[s:] == -math.inf).all()):
                failed.add('tail_values')
            tail, pool = sorted(oi[s:].tolist()), sorted(masked.tolist())
            ok = len(set(tail)) == len(tail) and set(tail) <= set(pool) and (len(pool) > k - s or tail == pool)
            if not ok:
                failed.add('tail_ids')
    return sorted(failed)
