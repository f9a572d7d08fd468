"""Float64 referee of the in-place BPR SGD step (fused.bpr_sgd_step in both forms, fused.PrefetchedBPRSGD, rsa_bpr_sgd_prepare /
rsa_bpr_sgd_apply), the error bounds a correct fp32 implementation stays inside, and an fp32 emulation of the kernels'
arithmetic with the mistakes the bounds must catch.  Test code only: nothing here calls recstudio_amd.  Runs on whatever
device its tensors live on.

The step is ``loss.backward(); torch.optim.SGD(lr).step()`` on two nn.Embedding(padding_idx=0) tables W (items) and U (users) with
BPRLoss (loss_func.py:55-59); M queries, n negatives each, every gradient taken from the PRE-step tables, rows 0 receive nothing:

    x[m, j]  = <U[uid_m], W[neg_mj]> - <U[uid_m], W[pos_m]>
    dneg     = sigmoid(x) / (M n)          dpos[m] = -sum_j dneg[m, j]          loss = mean softplus(x)
    W'[id]   = W[id] - lr * sum over elements e on row id of d_e * U[uid_e]          (d_e = dpos of the positive, dneg of a negative)
    qg[m]    = dpos[m] W[pos_m] + sum_j dneg[m, j] W[neg_mj]
    U'[u]    = U[u] - lr * sum over queries m of user u of qg[m]

Two stages, so that a failure names its cause (u = 2^-24):

Stage A -- the update arithmetic, given the kernel's OWN fp32 coefficients (dpos, dneg as it wrote them; query_grad for the users):
    |W'32 - W'| <= |lr| tol_g + 2u |W'|,        tol_g = min((K + 2) u A, cap)          (adam_referee.tolerances' tol_g, same cap)
A = the sum of the absolute terms of the row's run, K its length.  (K + 2) u A covers any fp32 summation order with fused
multiply-adds (K roundings, K - 1 of them additions of partial sums, per-chunk partials included: any tree has depth <= K) and the
product with the step scale; 2u |W'| the single read-modify-write.  query_grad[m] itself: (n + 3) u x the sum of the absolute
terms (n + 1 fused multiply-adds, the negation of dpos and its wave sum one unit each: the kernel multiplies by -tg, a sum of its
own).  No fitted constant.

Stage B -- the coefficients against float64 scores of the pre-step tables:
    |dneg32 - dneg| <= dneg ((1 - sigmoid(x)) (e_x + 2u |x|) + allow u)
    |dpos32 - dpos| <= sum_j (that) + (n - 1) u |dpos|
e_x = (d + 1) u (sum_i |u_i w_neg,i| + sum_i |u_i w_pos,i|) is the error of the two fp32 dot products and their difference;
d sigmoid / dx = sigmoid (1 - sigmoid).  2u |x|: a hardware exp evaluates 2^(x log2 e), the rounded product with the rounded
constant is an argument error of 2u |x| -- derived, and reported separately by the GPU test (it asserts the kernel with AND
records it without that term).  ``allow``: the error of the sigmoid evaluation itself, in units of u x the result, is nothing
arithmetic gives; the GPU test measures it for torch's fp32 sigmoid on the same device and allows twice that
(test_gpu_sgd_step.py: sigmoid_allowance).

End to end = Stage B carried through Stage A's sums: the float64 step from float64 coefficients, tolerance
    |lr| (tol_g + sum_e |delta d_e| |q_e|) + 2u |W'|
and for the users |lr| ((K + 2) u A + sum_m tol_qg[m]) + 2u |U'| with tol_qg = (n + 3) u terms + |delta dpos| |W[pos]| + sum_j |delta dneg_j| |W[neg_j]|.
"""
import numpy as np
import torch

import adam_referee as ar

U32 = ar.U32


# ------------------------------------------------------------------------------------------------------------ float64 coefficients
def coefficients(iw, uw, uid, pos, neg, block=512):
    """Float64 BPR coefficients of the step on the pre-step tables -> dict(x [M, n] = s_neg - s_pos, sig = sigmoid(x), dneg, dpos,
    loss, ex [M, n] = the derived fp32 score-difference error, qg [M, d] = d loss / d query row, qabs [M, d] = the sum of the
    absolute terms of qg)."""
    M, n = neg.shape
    d = iw.shape[1]
    dev = iw.device
    x = torch.empty(M, n, dtype=torch.float64, device=dev)
    ex = torch.empty_like(x)
    for lo in range(0, M, block):
        q = uw[uid[lo:lo + block]].double()
        wp = iw[pos[lo:lo + block]].double()
        wn = iw[neg[lo:lo + block]].double()
        x[lo:lo + block] = (q.unsqueeze(1) * wn).sum(-1) - (q * wp).sum(-1, keepdim=True)
        ex[lo:lo + block] = (d + 1) * U32 * ((q.unsqueeze(1) * wn).abs().sum(-1) + (q * wp).abs().sum(-1, keepdim=True))
    sig = torch.sigmoid(x)
    dneg = sig / (M * n)
    dpos = -dneg.sum(1)
    loss = float(torch.nn.functional.softplus(x).mean())
    qg = torch.empty(M, d, dtype=torch.float64, device=dev)
    qabs = torch.empty_like(qg)
    for lo in range(0, M, block):
        wp = iw[pos[lo:lo + block]].double()
        wn = iw[neg[lo:lo + block]].double()
        t = dneg[lo:lo + block].unsqueeze(-1) * wn
        p = dpos[lo:lo + block].unsqueeze(-1) * wp
        qg[lo:lo + block] = t.sum(1) + p
        qabs[lo:lo + block] = t.abs().sum(1) + p.abs()
    return dict(x=x, sig=sig, dneg=dneg, dpos=dpos, loss=loss, ex=ex, qg=qg, qabs=qabs, n=n, M=M)


def coefficient_tolerances(c, allow, exp_argument_term=True):
    """Stage B -> (tol_dneg [M, n], tol_dpos [M])."""
    arg = c['ex'] + (2 * U32 * c['x'].abs() if exp_argument_term else 0.0)
    tol_dneg = c['dneg'] * ((1.0 - c['sig']) * arg + allow * U32)
    tol_dpos = tol_dneg.sum(1) + (c['n'] - 1) * U32 * c['dpos'].abs()
    return tol_dneg, tol_dpos


def sigmoid_units(d32, x32, scale):
    """|d32 - sigmoid64(x32) scale| / (u sigmoid64(x32) scale) elementwise: the error of an fp32 evaluation of scale * sigmoid at
    the fp32 argument it was given, in units of u x the result."""
    want = torch.sigmoid(x32.double()) * scale
    return (d32.double() - want).abs() / (U32 * want)


def torch_sigmoid_allowance(device, M, n):
    """-> (allowance, torch's measured maximum): the worst error of torch's fp32 ``sigmoid(x) * (1 / n) * (1 / M)`` on ``device``
    against float64 ``sigmoid(x) / (M n)`` at the same fp32 arguments (2^20 of them: a grid over [-20, 20] and normal draws of
    widths 0.1, 1 and 4), in units of u x the result; the allowance is twice that (two equally legitimate evaluations of the
    exponential differ by about their own error).  Measured where the test runs, not fixed in advance."""
    g = torch.Generator(device=device).manual_seed(0)
    k = 1 << 18
    x = torch.cat([torch.linspace(-20, 20, k, device=device)] +
                  [torch.randn(k, device=device, generator=g) * w for w in (0.1, 1.0, 4.0)])
    inv_n = torch.tensor(1.0 / n, dtype=torch.float32, device=device)
    inv_m = torch.tensor(1.0 / M, dtype=torch.float32, device=device)
    worst = float(sigmoid_units((torch.sigmoid(x) * inv_n) * inv_m, x, 1.0 / (M * n)).max())
    return 2.0 * worst, worst


# ----------------------------------------------------------------------------------------------------------------- the row updates
def _ratio(got, want, tol):
    err = (got.double() - want).abs()
    r = torch.where(err == 0, torch.zeros_like(err), err / tol.clamp_min(1e-300))
    return float(r.max()) if r.numel() else 0.0


def _tol_g(grad):
    K = grad['K'].double().unsqueeze(1)
    return torch.minimum((K + 2.0) * U32 * grad['A'], 1e-5 * grad['g'].abs() + 1e-6 * max(1.0, grad['a_total']))


def _finish(grad, table, lr, in_table_atomics):
    w0 = table[grad['rows']].double()
    w = w0 - float(lr) * grad['g']
    tol = abs(float(lr)) * _tol_g(grad) + 2 * U32 * w.abs()
    if in_table_atomics:
        # float atomics that accumulate IN the weight row round K times at the weight's magnitude, not once: every add rounds a
        # value of at most |W| + |lr| A.  Two of those roundings are the 2u |W'| above.
        tol = tol + (grad['K'].double().unsqueeze(1) - 2).clamp_min(0) * U32 * (w0.abs() + abs(float(lr)) * grad['A'])
    return dict(grad, w0=w0, w=w, tol=tol)


def item_update(iw, uw, uid, pos, neg, dpos, dneg, lr, rows=None, in_table_atomics=False):
    """W' of the touched item rows from the given coefficients (the kernel's fp32 ones: Stage A; float64 ones: the float64 step)
    -> row_gradients' dict + w0, w [R, d] float64, tol [R, d] (Stage A).  ``in_table_atomics``: the bound of the forms that add
    every element into the weight row with a float atomic (bpr_sgd_step(atomics=True), embed_dim outside {64, 128, 256})."""
    grad = ar.row_gradients(uw, neg, dneg, query_index=uid, pos_ids=pos, dpos=dpos, pad_row=0, rows=rows)
    return _finish(grad, iw, lr, in_table_atomics)


def user_update(uw, uid, qgrad, lr, rows=None, in_table_atomics=False):
    """U' of the touched user rows from the per-query gradients (coefficient 1 each) -> as item_update."""
    M = uid.numel()
    ones = torch.ones(M, 1, dtype=qgrad.dtype, device=qgrad.device)
    grad = ar.row_gradients(qgrad, uid.view(M, 1), ones, pad_row=0, rows=rows)
    return _finish(grad, uw, lr, in_table_atomics)


def query_grad_ratio(iw, pos, neg, dpos, dneg, qgrad, block=512):
    """max |qgrad32[m] - (dpos[m] W[pos] + sum_j dneg[m, j] W[neg_j])| / ((n + 3) u sum of the absolute terms), the sums in float64
    from the SAME fp32 coefficients."""
    M, n = neg.shape
    worst = 0.0
    for lo in range(0, M, block):
        wp = iw[pos[lo:lo + block]].double()
        wn = iw[neg[lo:lo + block]].double()
        t = dneg[lo:lo + block].double().unsqueeze(-1) * wn
        p = dpos[lo:lo + block].double().unsqueeze(-1) * wp
        worst = max(worst, _ratio(qgrad[lo:lo + block], t.sum(1) + p, (n + 3) * U32 * (t.abs().sum(1) + p.abs())))
    return worst


def end_to_end(iw, uw, uid, pos, neg, lr, c, allow, item_rows=None, user_rows=None, in_table_atomics=False):
    """The float64 step and the end-to-end tolerances of both tables -> (item dict, user dict) as item_update / user_update."""
    tol_dneg, tol_dpos = coefficient_tolerances(c, allow)
    it = item_update(iw, uw, uid, pos, neg, c['dpos'], c['dneg'], lr, rows=item_rows, in_table_atomics=in_table_atomics)
    slack = ar.row_gradients(uw, neg, tol_dneg, query_index=uid, pos_ids=pos, dpos=tol_dpos, pad_row=0, rows=item_rows)
    assert torch.equal(slack['rows'], it['rows'])
    it['tol'] = it['tol'] + abs(float(lr)) * slack['A']
    us = user_update(uw, uid, c['qg'], lr, rows=user_rows, in_table_atomics=in_table_atomics)
    n = c['n']
    tol_qg = (n + 3) * U32 * c['qabs']
    block = 512
    for lo in range(0, c['M'], block):
        wp = iw[pos[lo:lo + block]].double().abs()
        wn = iw[neg[lo:lo + block]].double().abs()
        tol_qg[lo:lo + block] += tol_dpos[lo:lo + block].unsqueeze(-1) * wp + (tol_dneg[lo:lo + block].unsqueeze(-1) * wn).sum(1)
    M = uid.numel()
    slack = ar.row_gradients(tol_qg, uid.view(M, 1), torch.ones(M, 1, dtype=torch.float64, device=uw.device), pad_row=0, rows=user_rows)
    assert torch.equal(slack['rows'], us['rows'])
    us['tol'] = us['tol'] + abs(float(lr)) * slack['A']
    return it, us


def update_scale(ref):
    """median over the elements of the touched rows of |update| / |weight| (elements with a zero weight left out)."""
    w0 = ref['w0']
    live = w0 != 0
    return float(((ref['w'] - w0).abs()[live] / w0.abs()[live]).median()) if bool(live.any()) else float('inf')


def bound_ratio(ref, table_after):
    """max |got - referee| / tolerance over every element of the referee's rows (a ``rows=`` sample included)."""
    return _ratio(table_after[ref['rows']], ref['w'], ref['tol'])


def judge(ref, table_after, table_before):
    """-> (max |got - referee| / tolerance over every element of the referee's rows, the number of OTHER rows of the table that
    are not bit-equal to the start table).  ``ref`` covers all touched rows (no ``rows=`` sample)."""
    r = ref['rows']
    ratio = _ratio(table_after[r], ref['w'], ref['tol'])
    rest = torch.ones(table_before.shape[0], dtype=torch.bool, device=table_before.device)
    rest[r] = False
    moved = int((table_after[rest] != table_before[rest]).any(1).sum())
    return ratio, moved


# --------------------------------------------------------------------------------------------------- fp32 emulation and its mutants
IN_TABLE_MUTANTS = ('item_from_updated_users', 'drop_one_of_long_run', 'duplicate_user_once', 'padding_row_moved', 'element_twice')


def emulate_in_table_fp32(iw, uw, uid, pos, neg, dpos, dneg, qgrad, lr, order_seed=0, mutant=None):
    """The float-atomic forms in numpy fp32 (bpr_sgd_step(atomics=True), embed_dim outside the stock dims): every element is added
    INTO its weight row on its own, row = fl(row + fl(fl(scale * d) * q)) for the items from the pre-update user rows, then
    row = fl(row + fl(scale * qgrad[m])) for the users -- K read-modify-writes of a K-element row where the sorted forms make one.
    The order of the atomics is free: ``order_seed`` None = element order, otherwise a seeded permutation.  ``mutant``: one of
    IN_TABLE_MUTANTS (the mistakes of order and bookkeeping this form can make).  -> (W', U') fp32 tensors."""
    assert mutant is None or mutant in IN_TABLE_MUTANTS
    f32 = np.float32
    W, Uq = iw.cpu().numpy().astype(f32).copy(), uw.cpu().numpy().astype(f32).copy()
    scale = f32(-float(lr))
    M, n = neg.shape
    ids, qrow, coef = (t.cpu().numpy() for t in ar.flat_elements(neg, dneg, uid, pos, dpos))
    coef = coef.astype(f32)
    qg = qgrad.cpu().numpy().astype(f32)
    uidn = uid.cpu().numpy()
    rng = np.random.default_rng(order_seed) if order_seed is not None else None

    def users(target):
        seen = set()
        for m in (rng.permutation(M) if rng is not None else range(M)):
            u = int(uidn[m])
            if u == 0 or (mutant == 'duplicate_user_once' and u in seen):
                continue
            seen.add(u)
            target[u] = (target[u] + (scale * qg[m]).astype(f32)).astype(f32)

    src = Uq
    if mutant == 'item_from_updated_users':
        src = Uq.copy()
        users(src)
    live = ids[ids > 0]
    longest = int(np.bincount(live).argmax()) if live.size else -1
    planted = False
    for e in (rng.permutation(len(ids)) if rng is not None else range(len(ids))):
        k = int(ids[e])
        if k < 0 or (k == 0 and mutant != 'padding_row_moved'):
            continue
        if mutant == 'drop_one_of_long_run' and k == longest and not planted:
            planted = True
            continue
        t = ((scale * coef[e]).astype(f32) * src[qrow[e]]).astype(f32)
        for _ in range(2 if (mutant == 'element_twice' and k == longest and not planted) else 1):
            W[k] = (W[k] + t).astype(f32)
        if mutant == 'element_twice' and k == longest:
            planted = True
    if mutant == 'item_from_updated_users':
        Uq = src
    else:
        users(Uq)
    return torch.from_numpy(W), torch.from_numpy(Uq)


MUTANTS = ('item_from_updated_users', 'users_before_shared_items', 'solo_twice', 'solo_skipped', 'drop_one_of_long_run',
           'duplicate_user_once', 'padding_row_moved', 'scale_per_partial')


def emulate_coefficients_fp32(iw, uw, uid, pos, neg, with_scores=False):
    """The forward's coefficients in numpy fp32: the dot products one rounding per multiply-add in component order, the sigmoid as
    bpr_dneg forms it (t = exp(-|x|), r = 1 / (1 + t), x >= 0 ? t r : r, then the two scalings), query_grad one rounding per
    multiply-add over the negatives in order, the positive last.  -> (dpos [M], dneg [M, n], qgrad [M, d]) fp32 tensors
    (``with_scores``: + pos_score [M], neg_score [M, n])."""
    f32, f64 = np.float32, np.float64
    W, Uq = iw.cpu().numpy().astype(f32), uw.cpu().numpy().astype(f32)
    uidn, posn, negn = uid.cpu().numpy(), pos.cpu().numpy(), neg.cpu().numpy()
    M, n = negn.shape
    d = W.shape[1]
    q = Uq[uidn]
    sp = np.zeros(M, f32)
    sn = np.zeros((M, n), f32)
    for i in range(d):
        sp = (q[:, i].astype(f64) * W[posn, i] + sp).astype(f32)
        sn = (q[:, i:i + 1].astype(f64) * W[negn, i] + sn).astype(f32)
    xd = (sp[:, None] - sn).astype(f32)
    t = np.exp(-np.abs(xd)).astype(f32)
    r = (f32(1.0) / (f32(1.0) + t).astype(f32)).astype(f32)
    sg = np.where(xd >= 0, (t * r).astype(f32), r)
    dneg = ((sg * f32(1.0 / n)).astype(f32) * f32(1.0 / M)).astype(f32)
    dpos = np.zeros(M, f32)
    for j in range(n):
        dpos = (dpos + dneg[:, j]).astype(f32)
    dpos = -dpos
    qg = np.zeros((M, d), f32)
    for j in range(n):
        qg = (dneg[:, j:j + 1].astype(f64) * W[negn[:, j]] + qg).astype(f32)
    qg = (dpos[:, None].astype(f64) * W[posn] + qg).astype(f32)
    out = (torch.from_numpy(dpos), torch.from_numpy(dneg), torch.from_numpy(qg))
    return out + (torch.from_numpy(sp), torch.from_numpy(sn)) if with_scores else out


def _apply_fp32(table, query, neg_ids, coef, scale, *, query_index=None, pos_ids=None, dpos=None, pad_row=0, chunk=16,
                drop_element_of=None, scale_partials=False, skip=(), twice=()):
    """target[id] = fl(target[id] + fl(scale * run sum)) for every touched row (adam_referee.emulate_run_sums: sorted order,
    per-chunk partials).  In place on the numpy fp32 ``table``.  The switches are the mutants of emulate_step_fp32."""
    f32 = np.float32
    sums, K = ar.emulate_run_sums(query, neg_ids, coef, table.shape[0], query_index=query_index, pos_ids=pos_ids, dpos=dpos,
                                  pad_row=pad_row, chunk=chunk, drop_element_of=drop_element_of,
                                  partial_scale=f32(scale) if scale_partials else None)
    for k, total in sums.items():
        if k in skip:
            continue
        for _ in range(2 if k in twice else 1):
            table[k] = (table[k] + (f32(scale) * total).astype(f32)).astype(f32)
    return K


def emulate_step_fp32(iw, uw, uid, pos, neg, dpos, dneg, qgrad, lr, chunk=16, mutant=None):
    """The step's update passes in numpy fp32 from the given fp32 coefficients, in the kernels' order: solo item rows in the forward
    (row + scale * (d * q): the same roundings as a run of one), the shared item rows from the PRE-update user rows, then the user
    rows (users sorted, duplicates summed, one read-modify-write).  ``mutant``: one of MUTANTS.  -> (W', U') fp32 tensors."""
    assert mutant is None or mutant in MUTANTS
    f32 = np.float32
    W, Uq = iw.cpu().numpy().astype(f32).copy(), uw.cpu().numpy().astype(f32).copy()
    scale = f32(-float(lr))
    M, n = neg.shape
    ids_all = torch.cat([pos.view(M, 1), neg], 1).reshape(-1)
    cnt = torch.bincount(ids_all[ids_all > 0], minlength=W.shape[0])
    solo = set(int(k) for k in (cnt == 1).nonzero().view(-1))
    longest = int(cnt.argmax())
    ones = torch.ones(M, 1)

    def users(target):
        qi = uid.view(M, 1)
        if mutant == 'duplicate_user_once':          # only the first query of every user counts
            first = torch.zeros(M, dtype=torch.bool)
            seen = set()
            for m, u in enumerate(uid.tolist()):
                first[m] = u not in seen
                seen.add(u)
            qi = torch.where(first, uid, torch.full_like(uid, -1)).view(M, 1)
        _apply_fp32(target, qgrad, qi, ones, scale, pad_row=0, chunk=chunk)

    U_items = Uq
    if mutant in ('item_from_updated_users', 'users_before_shared_items'):
        U_new = Uq.copy()
        users(U_new)
        if mutant == 'item_from_updated_users':
            U_items = U_new
    kw = dict(query_index=uid, pos_ids=pos, dpos=dpos, chunk=chunk)
    if mutant == 'users_before_shared_items':
        # the forward (solo rows) read the pre-update user rows, the apply pass (shared rows) the updated ones
        shared = set(int(k) for k in (cnt > 1).nonzero().view(-1))
        _apply_fp32(W, torch.from_numpy(Uq), neg, dneg, scale, skip=shared, **kw)
        _apply_fp32(W, torch.from_numpy(U_new), neg, dneg, scale, skip=solo, **kw)
    else:
        _apply_fp32(W, torch.from_numpy(U_items), neg, dneg, scale,
                    pad_row=-1 if mutant == 'padding_row_moved' else 0,
                    drop_element_of=longest if mutant == 'drop_one_of_long_run' else None,
                    scale_partials=mutant == 'scale_per_partial',
                    skip=solo if mutant == 'solo_skipped' else (), twice=solo if mutant == 'solo_twice' else (), **kw)
    if mutant in ('item_from_updated_users', 'users_before_shared_items'):
        Uq = U_new
    else:
        users(Uq)
    return torch.from_numpy(W), torch.from_numpy(Uq)
