"""Float64 referee of the Adagrad row update (rsa_rows_update_sorted / _presorted with rule = RSA_ROWS_ADAGRAD), the error bound a
correct fp32 implementation stays inside, and an fp32 emulation of the kernel's arithmetic with the mistakes the bound must
catch.  Test code only: nothing here calls recstudio_amd.  Runs on whatever device its tensors live on.

    g[id] = adam_referee.row_gradients (the coalesced row gradient of the kept elements, float64)
    clr   = lr / (1 + (step - 1) lr_decay)
    s'    = s + g^2;   w' = w - clr g / (sqrt(s') + eps)          on touched rows only

A row without a kept element has g = 0, for which the dense rule gives s' = s and w' = w: updating the touched rows alone is
torch.optim.Adagrad on dense AND on sparse gradients (tests/test_adagrad_referee.py pins this file to both branches).
lr, lr_decay, eps are the Python doubles the caller passed.
"""
import numpy as np
import torch

import adam_referee as ar

U32 = ar.U32


def clr_of(lr, lr_decay, step):
    return lr / (1.0 + (step - 1) * lr_decay)


def adagrad_update(grad, weight, state_sum, *, lr, lr_decay, eps, step):
    """The update of the touched rows ``grad['rows']`` from the fp32 (or float64) tables -> grad + dict(w0, s0, w, s [R, d]
    float64, clr, eps)."""
    r, g = grad['rows'], grad['g']
    w0, s0 = weight[r].double(), state_sum[r].double()
    clr = clr_of(lr, lr_decay, step)
    s = s0 + g * g
    w = w0 - clr * (g / (s.sqrt() + eps))
    return dict(grad, w0=w0, s0=s0, w=w, s=s, clr=clr, eps=eps)


def referee(weight, state_sum, query, neg_ids, dneg, *, lr, lr_decay=0.0, eps=1e-10, step=1, query_index=None, pos_ids=None,
            dpos=None, upstream=None, pad_row=0, rows=None):
    grad = ar.row_gradients(query, neg_ids, dneg, query_index=query_index, pos_ids=pos_ids, dpos=dpos, upstream=upstream,
                            pad_row=pad_row, rows=rows)
    return adagrad_update(grad, weight, state_sum, lr=lr, lr_decay=lr_decay, eps=eps, step=step)


def tolerances(ref):
    """What an fp32 implementation of the update may differ by from ``ref`` (elementwise, [R, d] each) -> (tol_w, tol_s).
    Derived as adam_referee.tolerances with m' replaced by g (u = 2^-24):
        tol_g as there: min((K + 2) u A, 1e-5 |g| + 1e-6 max(1, max column of the summed |terms|))
        tol_s = (2|g| + tol_g) tol_g + 4u (s' + g^2)
        tol_w = 4u |w| + clr (tol_g / den + |g| tol_s / (2 sqrt(s') den^2)) + 4u clr |g| / den,      den = sqrt(s') + eps
    The first term of tol_s carries the gradient's error through the square; the bracket of tol_w carries the errors of g and s'
    through g / den (d sqrt(s) = ds / (2 sqrt(s))); every 4u term allows the handful of correctly rounded operations of the update
    itself (mul, fma; sqrt, add, div, fma) and the one rounding of each constant.  No fitted constant."""
    g, A, K = ref['g'], ref['A'], ref['K'].double().unsqueeze(1)
    u = U32
    tol_g = torch.minimum((K + 2.0) * u * A, 1e-5 * g.abs() + 1e-6 * max(1.0, ref['a_total']))
    ga = g.abs()
    tol_s = (2 * ga + tol_g) * tol_g + 4 * u * (ref['s'] + g * g)
    root = ref['s'].sqrt()
    den = root + ref['eps']
    clr = ref['clr']
    # (s' == 0 only where g == 0 on a zero state: the term vanishes with |g|; den == 0 needs eps == 0 on top, where the update
    # itself is 0 / 0 in torch as well -- no case here has it)
    tol_w = 4 * u * ref['w0'].abs() + clr * (tol_g / den.clamp_min(1e-300) + ga * tol_s / (2 * root.clamp_min(1e-300) * (den * den).clamp_min(1e-300))) \
        + 4 * u * clr * ga / den.clamp_min(1e-300)
    return tol_w, tol_s


def bound_ratios(ref, got_w, got_s):
    """max over all elements of |got - referee| / tolerance for (weight, state_sum); got_*: [R, d] rows ``ref['rows']`` of the
    tables under test.  An element the referee fixes exactly (tolerance 0) must match exactly."""
    out = []
    for got, want, tol in zip((got_w, got_s), (ref['w'], ref['s']), tolerances(ref)):
        err = (got.double() - want).abs()
        ratio = torch.where(err == 0, torch.zeros_like(err), err / tol.clamp_min(1e-300))
        out.append(float(ratio.max()) if ratio.numel() else 0.0)
    return tuple(out)


def untouched_equal(ref, before, after):
    """Every row outside ``ref['rows']`` of every table bit-unchanged (the tolerance of an untouched element is 0)."""
    rest = torch.ones(before[0].shape[0], dtype=torch.bool, device=before[0].device)
    rest[ref['rows']] = False
    return all(torch.equal(a[rest], b[rest]) for a, b in zip(after, before))


# ---------------------------------------------------------------------------------------------------------------------------
MISTAKES = ('per_element_squares', 'old_state', 'eps_in_root', 'no_lr_decay')


def emulate_fp32(weight, state_sum, query, neg_ids, dneg, *, lr, lr_decay=0.0, eps=1e-10, step=1, query_index=None, pos_ids=None,
                 dpos=None, upstream=None, pad_row=0, chunk=16, mistake=None, drop_element_of=None, partial_scale=None):
    """The sorted kernels' arithmetic in numpy fp32, operation for operation: the run sums of adam_referee.emulate_run_sums, then
    apply_run_adagrad's
        g = fl(up * sum);  s' = fl(g g + s) [fused];  den = fl(fl(sqrt(s')) + eps);  q = fl(g / den);  w' = fl(-clr q + w) [fused]
    with clr and eps rounded to fp32 once.  -> (rows, w, s) fp32 arrays of the touched rows.
    Planted mistakes (``mistake``): 'per_element_squares' = s' = s + sum of the squared elements instead of the squared row sum;
    'old_state' = the division taken with sqrt(s); 'eps_in_root' = sqrt(s' + eps); 'no_lr_decay' = clr = lr.
    ``drop_element_of`` / ``partial_scale``: adam_referee.emulate_run_sums' (a run's last element dropped, a chunk partial scaled)."""
    assert mistake is None or mistake in MISTAKES
    f32, f64 = np.float32, np.float64
    up = f32(1.0) if upstream is None else f32(upstream.cpu().numpy().reshape(-1)[0])
    sums, _ = ar.emulate_run_sums(query, neg_ids, dneg, weight.shape[0], query_index=query_index, pos_ids=pos_ids, dpos=dpos,
                                  pad_row=pad_row, chunk=chunk, drop_element_of=drop_element_of, partial_scale=partial_scale)
    d = query.shape[1]
    rows = np.array(sorted(sums), dtype=np.int64)
    clr = f32(lr if mistake == 'no_lr_decay' else clr_of(lr, lr_decay, step))
    epsf = f32(eps)
    w0, s0 = (t[torch.as_tensor(rows)].cpu().numpy().astype(f32) for t in (weight, state_sum))
    g = np.stack([(up * sums[int(r)]).astype(f32) for r in rows]) if len(rows) else np.zeros((0, d), f32)
    if mistake == 'per_element_squares':
        ids, qrow, coef = (t.cpu().numpy() for t in ar.flat_elements(neg_ids, dneg, query_index, pos_ids, dpos))
        terms = (f64(up) * coef.astype(f64)[:, None] * query.cpu().numpy().astype(f64)[qrow]) ** 2
        sq = np.zeros((weight.shape[0], d), f64)
        keep = (ids >= 0) & (ids != pad_row)
        np.add.at(sq, ids[keep], terms[keep])
        s1 = (s0.astype(f64) + sq[rows]).astype(f32)
    else:
        s1 = (g.astype(f64) * g.astype(f64) + s0.astype(f64)).astype(f32)              # fused: one rounding
    if mistake == 'old_state':
        den = (np.sqrt(s0).astype(f32) + epsf).astype(f32)
    elif mistake == 'eps_in_root':
        den = np.sqrt((s1 + epsf).astype(f32)).astype(f32)
    else:
        den = (np.sqrt(s1).astype(f32) + epsf).astype(f32)
    q = (g / den).astype(f32)
    w1 = (-f64(clr) * q.astype(f64) + w0.astype(f64)).astype(f32)                      # fused: one rounding
    return rows, w1, s1
