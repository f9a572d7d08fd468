"""Float64 referee of the lazy-Adam row update (rsa_rows_update_sorted / _presorted with exp_avg set), the error bound a correct
fp32 implementation stays inside, and an fp32 emulation of the kernel's arithmetic.  Test code only: nothing here calls
recstudio_amd.  Runs on whatever device its tensors live on.

    g[id]   = upstream * sum over kept elements e with id_e = id of coef_e * query[qrow_e]          (float64)
    kept    = id >= 0 and id != pad_row;  touched = ids with at least one kept element
    m' = m + (g - m)(1 - b1);  v' = v + (g^2 - v)(1 - b2)
    w' = w - lr * sqrt(1 - b2^step) / (1 - b1^step) * m' / (sqrt(v') + eps)          on touched rows only

lr, b1, b2, eps are the Python doubles the caller passed (0.999, not float32(0.999)): what torch.optim.SparseAdam computes
from (torch/optim/_functional.py sparse_adam; tests/test_adam_referee.py pins this file to it).
"""
import math

import numpy as np
import torch

U32 = 2.0 ** -24          # unit roundoff of fp32


def step_size(lr, betas, step):
    return lr * math.sqrt(1.0 - betas[1] ** step) / (1.0 - betas[0] ** step)


def flat_elements(neg_ids, dneg, query_index=None, pos_ids=None, dpos=None):
    """The step's elements in the kernels' element order e = m * w + c (column 0 = the positive when given)
    -> (ids, qrow, coef), each [M * w]."""
    M = neg_ids.shape[0]
    ids, coef = neg_ids.reshape(M, -1), dneg.reshape(M, -1)
    if pos_ids is not None:
        ids = torch.cat([pos_ids.view(M, 1), ids], 1)
        coef = torch.cat([dpos.view(M, 1), coef], 1)
    q = query_index if query_index is not None else torch.arange(M, device=ids.device)
    qrow = q.view(M, 1).expand_as(ids)
    return ids.reshape(-1), qrow.reshape(-1), coef.reshape(-1)


def row_gradients(query, neg_ids, dneg, *, query_index=None, pos_ids=None, dpos=None, upstream=None, pad_row=0, rows=None,
                  block=1 << 16):
    """-> dict(rows [R] sorted touched ids, g [R, d] float64, A [R, d] = |upstream| * sum |coef_e * query[qrow_e]|, K [R] element
    counts, a_total = max column of the sum of A over all rows).  ``rows``: only these ids (a sample of a large step)."""
    ids, qrow, coef = flat_elements(neg_ids, dneg, query_index, pos_ids, dpos)
    keep = (ids >= 0) & (ids != pad_row)
    if rows is not None:
        keep &= torch.isin(ids, rows)
    ids, qrow, coef = ids[keep], qrow[keep], coef[keep]
    uniq, inv = torch.unique(ids, return_inverse=True)
    R, d = uniq.numel(), query.shape[1]
    g = torch.zeros(R, d, dtype=torch.float64, device=query.device)
    A = torch.zeros_like(g)
    for lo in range(0, ids.numel(), block):           # (blocks: the [elements, d] float64 products never exist at once)
        c = coef[lo:lo + block].double().unsqueeze(1) * query[qrow[lo:lo + block]].double()
        if R <= 64:           # few rows with thousands of elements each: a 0/1 matrix product instead of contended atomic adds
            sel = torch.nn.functional.one_hot(inv[lo:lo + block], R).to(torch.float64).t()
            g += sel @ c
            A += sel @ c.abs()
        else:
            g.index_add_(0, inv[lo:lo + block], c)
            A.index_add_(0, inv[lo:lo + block], c.abs())
    up = 1.0 if upstream is None else float(upstream.double().reshape(-1)[0])
    g *= up
    A *= abs(up)
    K = torch.bincount(inv, minlength=R)
    a_total = float(A.sum(0).max()) if R else 0.0
    return {'rows': uniq, 'g': g, 'A': A, 'K': K, 'a_total': a_total}


def adam_update(grad, weight, exp_avg, exp_avg_sq, *, lr, betas, eps, step):
    """The update of the touched rows ``grad['rows']`` from the fp32 (or float64) tables -> grad + dict(w0, m0, v0, w, m, v
    [R, d] float64, ss)."""
    r, g = grad['rows'], grad['g']
    b1, b2 = betas
    w0, m0, v0 = weight[r].double(), exp_avg[r].double(), exp_avg_sq[r].double()
    m = m0 + (g - m0) * (1.0 - b1)
    v = v0 + (g * g - v0) * (1.0 - b2)
    ss = step_size(lr, betas, step)
    w = w0 - ss * m / (v.sqrt() + eps)
    return dict(grad, w0=w0, m0=m0, v0=v0, w=w, m=m, v=v, ss=ss, betas=betas, eps=eps)


def referee(weight, exp_avg, exp_avg_sq, query, neg_ids, dneg, *, lr, betas=(0.9, 0.999), eps=1e-8, step=1, query_index=None,
            pos_ids=None, dpos=None, upstream=None, pad_row=0, rows=None):
    grad = row_gradients(query, neg_ids, dneg, query_index=query_index, pos_ids=pos_ids, dpos=dpos, upstream=upstream,
                         pad_row=pad_row, rows=rows)
    return adam_update(grad, weight, exp_avg, exp_avg_sq, lr=lr, betas=betas, eps=eps, step=step)


def tolerances(ref):
    """What an fp32 implementation of the update may differ by from ``ref`` (elementwise, [R, d] each) -> (tol_w, tol_m, tol_v).

    u = 2^-24.  A row's gradient is a sum of K products: any fp32 summation order with fused multiply-adds, per-chunk partials
    included, and the final product with `upstream` satisfy |g32 - g| <= (K + 2) u A to first order (A = the sum of the
    absolute terms).  Long runs are not judged more loosely than the SGD mode of the same kernels already is
    (test_sorted_scatter_long_runs: 1e-5 |g| + 1e-6 max(1, max column of the summed |terms|)): the smaller bound holds.
        tol_m = (1 - b1) tol_g + 4u (|m'| + |m|)
        tol_v = (1 - b2) (2|g| + tol_g) tol_g + 4u (|v'| + (1 - b2) g^2)
        tol_w = 4u |w| + ss (tol_m / den + |m'| tol_v / (2 sqrt(v') den^2)) + 4u ss |m'| / den,      den = sqrt(v') + eps
    The first term of tol_m / tol_v carries the gradient's error through the (linear resp. quadratic) moment update, the first
    bracket of tol_w carries the moments' errors through m' / den (d sqrt(v) = dv / (2 sqrt(v))); every 4u term allows the
    handful of correctly rounded operations of the update itself (sub, mul, add; sqrt, add, div, mul, sub) and the one
    rounding of each constant.  No fitted constant anywhere."""
    g, A, K = ref['g'], ref['A'], ref['K'].double().unsqueeze(1)
    b1, b2 = ref['betas']
    u = U32
    tol_g = torch.minimum((K + 2.0) * u * A, 1e-5 * g.abs() + 1e-6 * max(1.0, ref['a_total']))
    tol_m = (1.0 - b1) * tol_g + 4 * u * (ref['m'].abs() + ref['m0'].abs())
    tol_v = (1.0 - b2) * (2 * g.abs() + tol_g) * tol_g + 4 * u * (ref['v'].abs() + (1.0 - b2) * g * g)
    root = ref['v'].sqrt()
    den = root + ref['eps']
    ss, m1 = ref['ss'], ref['m'].abs()
    # (v' == 0 only where g == 0 on a zero state: m' is 0 there too and the term vanishes)
    tol_w = 4 * u * ref['w0'].abs() + ss * (tol_m / den + m1 * tol_v / (2 * root.clamp_min(1e-300) * den * den)) + 4 * u * ss * m1 / den
    return tol_w, tol_m, tol_v


def bound_ratios(ref, got_w, got_m, got_v):
    """max over all elements of |got - referee| / tolerance for (weight, exp_avg, exp_avg_sq); got_*: [R, d] rows ``ref['rows']`` of
    the tables under test.  An element the referee fixes exactly (tolerance 0) must match exactly."""
    out = []
    for got, want, tol in zip((got_w, got_m, got_v), (ref['w'], ref['m'], ref['v']), tolerances(ref)):
        err = (got.double() - want).abs()
        ratio = torch.where(err == 0, torch.zeros_like(err), err / tol.clamp_min(1e-300))
        out.append(float(ratio.max()) if ratio.numel() else 0.0)
    return tuple(out)


# ---------------------------------------------------------------------------------------------------------------------------
def emulate_run_sums(query, neg_ids, dneg, n_rows, *, query_index=None, pos_ids=None, dpos=None, pad_row=0, chunk=16,
                      drop_element_of=None, partial_scale=None):
    """The run sums of the sorted apply pass in numpy fp32, operation for operation: elements stably sorted by id, every chunk of
    `chunk` sorted elements summed run by run in element order with one rounding per multiply-add, a run that crosses chunk
    borders = trailing partial + leading partials in chunk order.  -> ({row: fp32 sum [d]}, {row: element count}).
    Two planted mistakes for the tests of the bounds: ``drop_element_of`` = a row whose last element is left out;
    ``partial_scale`` = a factor wrongly applied to every partial of a run of more than one segment.
    The coefficients are rounded to fp32 first, as the query rows are: the kernels read fp32 coefficients.  A float64 ``dneg`` is
    therefore NOT multiplied at double precision (every caller passes fp32, for which the cast changes nothing)."""
    f32 = np.float32
    ids, qrow, coef = (t.cpu().numpy() for t in flat_elements(neg_ids, dneg, query_index, pos_ids, dpos))
    q = query.cpu().numpy().astype(f32)
    coef = coef.astype(f32)
    key = np.where(ids < 0, n_rows, ids)
    order = np.argsort(key, kind='stable')
    key = key[order]

    def fma(c, x, acc):                                   # fl32(c * x + acc): the product of two fp32 numbers is exact in float64
        return (np.float64(c) * x.astype(np.float64) + acc.astype(np.float64)).astype(f32)

    sums, counts = {}, {}
    pos = 0
    while pos < len(key):
        end = pos
        while end < len(key) and key[end] == key[pos]:
            end += 1
        k = int(key[pos])
        if k != n_rows and k != pad_row:
            total = None
            lo = pos
            last = end - 1 if (drop_element_of is not None and k == drop_element_of) else end
            segments = (last - 1) // chunk - pos // chunk + 1
            while lo < last:                              # the run's segments, chunk by chunk
                hi = min(last, (lo // chunk + 1) * chunk)
                acc = np.zeros(q.shape[1], f32)
                for i in range(lo, hi):
                    e = order[i]
                    acc = fma(coef[e], q[qrow[e]], acc)
                if partial_scale is not None and segments > 1:
                    acc = (f32(partial_scale) * acc).astype(f32)
                total = acc if total is None else (total + acc).astype(f32)
                lo = hi
            if total is not None:
                sums[k], counts[k] = total, last - pos
        pos = end
    return sums, counts


def emulate_fp32(weight, exp_avg, exp_avg_sq, query, neg_ids, dneg, *, lr, betas, eps, step, query_index=None, pos_ids=None,
                 dpos=None, upstream=None, pad_row=0, chunk=16, float_betas=False):
    """The sorted kernels' arithmetic in numpy fp32, operation for operation: the run sums of emulate_run_sums, g = upstream * sum,
    then the update of apply_run.
    ``float_betas``: the hyper-parameters carried as fp32 and 1 - beta taken in fp32 (the ABI 11 form) instead of the
    caller's doubles.  -> (rows, w, m, v) fp32 arrays of the touched rows."""
    f32 = np.float32
    up = f32(1.0) if upstream is None else f32(upstream.cpu().numpy().reshape(-1)[0])
    sums, _ = emulate_run_sums(query, neg_ids, dneg, weight.shape[0], query_index=query_index, pos_ids=pos_ids, dpos=dpos,
                               pad_row=pad_row, chunk=chunk)
    d = query.shape[1]
    rows = np.array(sorted(sums), dtype=np.int64)
    b1, b2 = betas
    if float_betas:
        omb1, omb2 = f32(1.0) - f32(b1), f32(1.0) - f32(b2)
        ss = f32(float(f32(lr)) * math.sqrt(1.0 - float(f32(b2)) ** step) / (1.0 - float(f32(b1)) ** step))
    else:
        omb1, omb2 = f32(1.0 - b1), f32(1.0 - b2)
        ss = f32(step_size(lr, betas, step))
    epsf = f32(eps)
    w0, m0, v0 = (t[torch.as_tensor(rows)].cpu().numpy().astype(f32) for t in (weight, exp_avg, exp_avg_sq))
    g = np.stack([up * sums[int(r)] for r in rows]).astype(f32) if len(rows) else np.zeros((0, d), f32)
    m1 = (m0 + ((g - m0).astype(f32) * omb1).astype(f32)).astype(f32)
    v1 = (v0 + (((g * g).astype(f32) - v0).astype(f32) * omb2).astype(f32)).astype(f32)
    w1 = (w0 - (ss * (m1 / (np.sqrt(v1).astype(f32) + epsf).astype(f32)).astype(f32)).astype(f32)).astype(f32)
    return rows, w1, m1, v1
