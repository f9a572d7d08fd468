"""Float64 referee of the user-history bag sum (``ops.bag_pool`` / ``ops.bag_pool_backward``, recstudio_amd/csrc/rsa_bag.hip).

THE RULE (recstudio/model/ae/multidae.py:29-31 and the per-user mean of the positives in the softmax loss), in float64:

    cnt_b = #{l : ids[b, l] != 0}        out_b = s_b * sum_{l : ids[b, l] != 0} table[ids[b, l]]
    s_b = 1 ('sum'),  cnt_b ** -0.5 ('rsqrt'),  1 / cnt_b ('mean')
    dW_i = sum_{(b, l) : ids[b, l] = i} s_b * g_b          (i != 0; an item twice in one bag counts twice)

An empty bag gives 0 under 'sum' and NaN (0 * inf, torch's 0 / 0) under the other two.  Padding is SKIPPED: the rule equals the
reference's ``embedding(ids).sum(1)`` whenever row 0 of the table is zero.

THE BOUNDS are derived, u = 2^-24 (half an ulp of fp32), first order, no fitted constant:

  * out:  (cnt + 3) u * s * sum_l |e_l| per element.  Any order of adding cnt fp32 numbers errs by at most (cnt - 1) u sum|e|;
    the square root, the reciprocal (or divide) and the final multiply are correctly rounded, u each.
  * dW_i: (m + 3) u * sum |s_b g_b| over the item's m occurrences: u each for the square root, the reciprocal and the product
    s_b * g_b of every term, (m - 1) u for the additions.
  * cnt is an integer and must be exact.

A bound of 0 (all rows of a bag zero in a column) demands the exact value.  ``emulate_fp32`` repeats the kernel's own order of
additions in fp32 torch ops on the CPU (tests/test_bag_referee.py keeps it inside HALF of every bound); ``MISTAKES`` are seeded
errors of the rule, each of which must leave a bound.
"""
import torch

U = 2.0 ** -24
F64 = torch.float64
SCALES = ('sum', 'rsqrt', 'mean')
PADS = (None, 'suffix', 'holes', 'whole')
FORWARD_MISTAKES = ('pad_read', 'cnt_pad', 'mean_for_rsqrt', 'dup_once', 'last_dropped')
BACKWARD_MISTAKES = ('scale_twice', 'row0_grad', 'neighbour', 'dup_once_bwd', 'cnt_pad_bwd')
MISTAKES = FORWARD_MISTAKES + BACKWARD_MISTAKES

CHUNK, RP_MAX = 256, 16          # rsa_bag.hip: BAG_CHUNK, BAG_RP_MAX


def f64(t):
    return t.detach().cpu().to(F64)


def _scale(cnt, scale):
    """s_b in float64 from the float64 counts; cnt == 0 -> inf for 'rsqrt' / 'mean'."""
    if scale == 'sum':
        return torch.ones_like(cnt)
    return cnt.pow(-0.5) if scale == 'rsqrt' else 1.0 / cnt


def _pairs(ids, mistake=None):
    """(bag, row) of the occurrences the rule adds, in (bag, position) order."""
    ids = ids.detach().cpu()
    live = ids != 0
    if mistake in ('pad_read', 'row0_grad'):
        live = torch.ones_like(live)
    if mistake == 'last_dropped':
        pos = torch.arange(ids.shape[1]).expand_as(ids)
        last = torch.where(live, pos, torch.full_like(pos, -1)).max(1, keepdim=True).values
        live = live & (pos != last)
    if mistake in ('dup_once', 'dup_once_bwd'):
        srt, order = ids.sort(dim=1, stable=True)
        first = torch.ones_like(live)
        first[:, 1:] = srt[:, 1:] != srt[:, :-1]
        live = live & torch.zeros_like(live).scatter(1, order, first)
    bag, pos = live.nonzero(as_tuple=True)
    return bag, ids[bag, pos]


def _counts(ids, mistake=None):
    ids = ids.detach().cpu()
    if mistake in ('cnt_pad', 'cnt_pad_bwd'):
        return torch.full((ids.shape[0],), ids.shape[1], dtype=F64)
    return (ids != 0).sum(1).to(F64)


def forward(table, ids, scale, mistake=None):
    """-> dict(out [B, d] float64 (NaN rows for empty bags under 'rsqrt' / 'mean'), cnt int64 [B], tol [B, d]).  ``table`` may live
    on any device: only the referenced rows are fetched, a block of bags at a time."""
    B, d = ids.shape[0], table.shape[1]
    bag, row = _pairs(ids, mistake)
    cnt = _counts(ids, mistake)
    tot, mag = torch.zeros(B, d, dtype=F64), torch.zeros(B, d, dtype=F64)
    step = max(1, (1 << 22) // d)
    for at in range(0, bag.numel(), step):
        e = f64(table[row[at:at + step].to(table.device)])
        tot.index_add_(0, bag[at:at + step], e)
        mag.index_add_(0, bag[at:at + step], e.abs())
    s = _scale(cnt, 'mean' if mistake == 'mean_for_rsqrt' and scale == 'rsqrt' else scale).unsqueeze(1)
    empty = (cnt == 0).unsqueeze(1)
    out = torch.where(empty & (scale != 'sum'), torch.full_like(tot, float('nan')), tot * torch.where(empty, torch.ones_like(s), s))
    tol = (cnt.unsqueeze(1) + 3) * U * torch.where(empty, torch.zeros_like(s), s) * mag
    return dict(out=out, cnt=cnt.to(torch.int64), tol=tol)


def backward(ids, g, scale, mistake=None):
    """-> dict(items int64 [T] (the touched rows, ascending), dW [T, d] float64, tol [T, d], m [T]).  Every other row of the dense
    gradient is exactly zero."""
    g = f64(g)
    bag, row = _pairs(ids, mistake)
    s = _scale(_counts(ids, mistake), scale)
    if mistake == 'scale_twice':
        s = s * s
    src = bag
    if mistake == 'neighbour':
        src = (bag + 1) % g.shape[0]
    items, inv = torch.unique(row, return_inverse=True)
    term = s[bag].unsqueeze(1) * g[src]
    dW = torch.zeros(items.numel(), g.shape[1], dtype=F64).index_add_(0, inv, term)
    mag = torch.zeros_like(dW).index_add_(0, inv, term.abs())
    m = torch.zeros(items.numel(), dtype=F64).index_add_(0, inv, torch.ones(inv.numel(), dtype=F64))
    return dict(items=items, dW=dW, tol=(m.unsqueeze(1) + 3) * U * mag, m=m)


def worst_ratio(got, want, tol):
    """max |got - want| / tol.  Where the bound is 0 the value must be exact; where the rule gives NaN the result must be NaN (a
    miss of either is inf)."""
    got = f64(got)
    nan = want.isnan()
    if bool((got.isnan() != nan).any()):
        return float('inf')
    diff = torch.where(nan, torch.zeros_like(want), (got - want).abs())
    tol = torch.where(nan, torch.ones_like(tol), tol)
    if bool(((tol == 0) & (diff != 0)).any()):
        return float('inf')
    return float((diff / tol.clamp_min(1e-300)).max()) if diff.numel() else 0.0


def dense(judged, n_rows):
    """The dense float64 [n_rows, d] gradient of ``backward``'s result (small tables only)."""
    out = torch.zeros(n_rows, judged['dW'].shape[1], dtype=F64)
    out[judged['items']] = judged['dW']
    return out


# ---------------------------------------------------------------- the kernel's order in fp32
def _scale32(cnt, scale):
    c = torch.tensor(float(cnt), dtype=torch.float32)
    one = torch.tensor(1.0, dtype=torch.float32)
    if scale == 'rsqrt':           # through float64, rounded to fp32 once
        return (1.0 / torch.tensor(float(cnt), dtype=F64).sqrt()).to(torch.float32)
    return one / c if scale == 'mean' else one


def emulate_fp32(table, ids, scale, g=None):
    """The kernel pair's own sequence of fp32 operations -> (out [B, d], cnt int32 [B], dW [N, d] or None).  Forward: a chunk of
    256 positions at a time, its live rows dealt round-robin to RP = min(256 // (d / 4), 16) slots, every slot adding its rows in
    order from +0, the slots added in slot order, the non-empty chunks in chunk order, one multiply by s (cnt ** -0.5 taken in float64 and rounded once).
    Backward: an item's occurrences in (bag, position) order, every term the fp32 product s_b * g_b."""
    N, d = table.shape
    B, L = ids.shape
    rp = min(CHUNK // (d // 4), RP_MAX)
    out = torch.zeros(B, d, dtype=torch.float32)
    cnt = torch.zeros(B, dtype=torch.int32)
    for b in range(B):
        acc, n = torch.zeros(d, dtype=torch.float32), 0
        for c0 in range(0, L, CHUNK):
            rows = [min(int(i), N - 1) for i in ids[b, c0:c0 + CHUNK] if int(i) > 0]
            if not rows:
                continue
            slots = []
            for r in range(min(rp, len(rows))):
                a = [torch.zeros(d, dtype=torch.float32) for _ in range(4)]
                for k, j in enumerate(range(r, len(rows), rp)):
                    a[k % 4] = a[k % 4] + table[rows[j]]
                slots.append((a[0] + a[1]) + (a[2] + a[3]))
            part = slots[0]
            for a in slots[1:]:
                part = part + a
            acc = acc + part
            n += len(rows)
        cnt[b] = n
        out[b] = acc * _scale32(n, scale) if scale != 'sum' else acc
    if g is None:
        return out, cnt, None
    acc = torch.zeros(N, 4, d, dtype=torch.float32)       # occurrence j of an item goes to its accumulator j mod 4
    seen = [0] * N
    s = [_scale32(int(c), scale) for c in cnt]
    for b in range(B):
        for i in ids[b]:
            if int(i) > 0:
                i = min(int(i), N - 1)
                acc[i, seen[i] % 4] += s[b] * g[b]
                seen[i] += 1
    return out, cnt, (acc[:, 0] + acc[:, 1]) + (acc[:, 2] + acc[:, 3])


# ---------------------------------------------------------------- cases
def make_ids(B, L, N, pad, gen, repeat=True, common=False):
    """int64 [B, L] of ids in [1, N).  ``pad``: None; 'suffix' (right-padded, lengths 1 and L included); 'holes' (zeros anywhere);
    'whole' ('suffix' with the LAST bag padded whole).  ``repeat``: bag 0 holds its first item twice (when it has two live
    positions).  ``common``: item 1 stands in every non-empty bag."""
    ids = torch.randint(1, N, (B, L), generator=gen)
    if pad in ('suffix', 'whole'):
        lengths = torch.randint(1, L + 1, (B,), generator=gen)
        lengths[0] = L
        if B > 1:
            lengths[1] = 1
        if pad == 'whole':
            lengths[B - 1] = 0
        ids = ids * (torch.arange(L).unsqueeze(0) < lengths.unsqueeze(1))
    elif pad == 'holes':
        ids = ids * (torch.rand(B, L, generator=gen) >= 0.3)
        ids[0, 0] = ids[0, 0].clamp_min(1)
    if repeat and L >= 2 and int(ids[0, 0]) > 0:
        ids[0, L - 1] = ids[0, 0]
    if common:
        has = (ids != 0).any(1)
        first = (ids != 0).int().argmax(1)
        ids[has, first[has]] = 1
    return ids


def make_case(B, L, d, N=23, *, pad=None, seed=0, row0=False, common=False):
    """A seeded case -> dict(table [N, d], ids [B, L], g [B, d]) of CPU tensors.  ``row0``: row 0 of the table is NOT zero (the
    rule never reads it)."""
    gen = torch.Generator().manual_seed(seed)
    table = torch.randn(N, d, generator=gen)
    if not row0:
        table[0] = 0
    return dict(table=table, ids=make_ids(B, L, N, pad, gen, common=common), g=torch.randn(B, d, generator=gen))
