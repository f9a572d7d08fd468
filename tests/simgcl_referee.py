"""Float64 referee of the perturbed form of rsa_spmm_csr, of SimGCLNet's propagation and its gradient and of one SimGCL training
step, the error bounds a correct fp32 implementation stays inside, and an fp32 emulation with seeded mistakes.  Test code only:
nothing here calls recstudio_amd.  Runs on whatever device its tensors live on.

THE RULE (simgcl.py:14-26 and :72-100, data_augmentation.py:524-570; dgl is not installed where this project is developed, so the
referee is pinned to the rule the source spells out).  With s the row's sum after row_scale (tests/spmm_referee.py) and u the
row's d uniforms, the fp32 numbers the kernel itself drew:

    q    = max(sqrt(sum_c u_c^2), 1e-12)
    dl_c = (u_c / q) * eps                    >= 0
    s'_c = s_c + sgn(s_c) * dl_c              sgn = torch.sign: 0 at 0
    acc' = k * (acc + s')

THE BOUND per element (u = 2^-24, contraction off), a sum of three terms:
  1. tol_s = (K + 2) u |s_r| sum |v_e x|: the product's own bound, spmm_referee.tolerances.
  2. tol_dl = (d / 2 + 4) u dl_c.  The fp32 sum of squares rounds each of the d squares once and sends every term through at most
     d - 1 additions IN ANY ORDER; all terms are positive, so it is off by at most d u relatively.  The square root halves a
     relative error and is rounded once (d / 2 + 1), the maximum is exact, the division is rounded once (d / 2 + 2), the product
     with eps once (d / 2 + 3); the product with the sign is exact.  First order; the + 1 is the slack, as in tol_s.
  3. u (|s'| + tol_s + tol_dl): the final addition is rounded once, on operands that are off by the first two terms.
and the accumulation costs |k| times that plus 2 u |acc'|, as in spmm_referee.  There is no fitted constant.

SIGN AMBIGUITY.  Where 0 < tol_s and |s_c| <= tol_s the fp32 sum may have either sign or be zero: such an element is accepted
when it is within the bound of s + dl, s - dl or s.  ``judge`` reports their share among the elements of rows WITH edges; the
tests cap it at 1e-4.  A row without edges has s = 0 exactly and tol_s = 0: it is not ambiguous and must come out as exactly 0.

SEVERAL LAYERS are judged layer by layer, each from the implementation's OWN previous layer (a flipped sign moves an element by
2 dl, which no bound carried through the layers would survive), and the mean is judged from the implementation's own layers:
(y_1 + ... + y_L) / L in fp32 is L - 1 additions, the product with 1 / L and that constant's own rounding: (L + 1) u sum |y_k| / L.
"""
import numpy as np
import torch
import torch.nn.functional as F

import sgl_referee as sg
import spmm_referee as sr

U32 = sr.U32


def deltas(u, eps):
    """(dl float64 [R, d] = u / max(||u||, 1e-12) * eps with eps as the fp32 the argument block carries, tol_dl)."""
    u = u.double()
    q = u.pow(2).sum(-1, keepdim=True).sqrt().clamp_min(1e-12)
    dl = u / q * float(np.float32(eps))
    return dl, (u.shape[1] / 2.0 + 4.0) * U32 * dl.abs()


def layer(indptr, indices, values, x, u, eps, row_scale=None, acc=None, acc_scale=1.0):
    """One perturbed layer -> dict(s, tol_s, dl, tol_dl, K, acc, k): everything ``judge`` needs."""
    ref = sr.referee(indptr, indices, values, x, row_scale=row_scale)
    tol_s, _ = sr.tolerances(ref)
    dl, tol_dl = deltas(u, eps)
    k = float(np.float32(acc_scale))
    return {'s': ref['y'], 'tol_s': tol_s, 'dl': dl, 'tol_dl': tol_dl, 'K': ref['K'], 'acc': None if acc is None else acc.double(), 'k': k}


def _candidate(ref, sgn):
    """(y', tol_y', acc', tol_acc') for the sign pattern ``sgn`` (a tensor of -1 / 0 / +1)."""
    y = ref['s'] + sgn * ref['dl']
    moved = (sgn != 0).double()
    tol = ref['tol_s'] + moved * ref['tol_dl']
    tol = tol + moved * U32 * (y.abs() + tol)          # (an element that is not moved takes no final addition: s + 0 is exact)
    if ref['acc'] is None:
        return y, tol, None, None
    a = ref['k'] * (ref['acc'] + y)
    return y, tol, a, abs(ref['k']) * tol + 2.0 * U32 * a.abs()


def _ratio(got, want, tol):
    err = (got.double().to(want.device) - want).abs()
    return torch.where(err == 0, torch.zeros_like(err), err / tol.clamp_min(1e-300))


def judge(ref, got_y=None, got_acc=None):
    """-> dict(ratio: the largest |got - want| / bound over all elements, an ambiguous element judged against the best of its
    three candidates (<= 1 passes); share: ambiguous elements / elements of rows with edges; n_ambiguous)."""
    s, tol_s = ref['s'], ref['tol_s']
    amb = (tol_s > 0) & (s.abs() <= tol_s)
    per_sign = []
    for sgn in (torch.sign(s), -torch.sign(s), torch.zeros_like(s), torch.ones_like(s), -torch.ones_like(s)):
        y, tol, a, tol_a = _candidate(ref, sgn)
        r = torch.zeros_like(s)
        if got_y is not None:
            r = torch.maximum(r, _ratio(got_y, y, tol))
        if got_acc is not None:
            r = torch.maximum(r, _ratio(got_acc, a, tol_a))
        per_sign.append(r)
    best = torch.stack(per_sign).min(0).values         # (y and acc of one element must agree on ONE sign: the maximum is inside)
    worst = torch.where(amb, best, per_sign[0])
    with_edges = int((ref['K'] > 0).sum()) * s.shape[1]
    return {'ratio': float(worst.max()) if worst.numel() else 0.0, 'n_ambiguous': int(amb.sum()),
            'share': int(amb.sum()) / max(with_edges, 1)}


def ambiguous_share(indptr, indices, values, x, row_scale=None):
    """The share ``judge`` would report, from the float64 data alone."""
    ref = sr.referee(indptr, indices, values, x, row_scale=row_scale)
    tol_s, _ = sr.tolerances(ref)
    amb = (tol_s > 0) & (ref['y'].abs() <= tol_s)
    return int(amb.sum()) / max(int((ref['K'] > 0).sum()) * x.shape[1], 1)


def judge_propagation(indptr, indices, values, e0, layers, mean, uniforms=None, eps=0.0):
    """SimGCLNet's forward from the implementation's own layer outputs ``layers`` (fp32 [n, d] each) and its ``mean``: layer k
    against the referee of layer k on layers[k - 1] (e0 for the first) and ``uniforms[k]`` (None: unperturbed), the mean against
    the float64 mean of ``layers``.  -> dict(ratio: the worst layer ratio, share: the largest ambiguous share, mean_ratio)."""
    L = len(layers)
    out = {'ratio': 0.0, 'share': 0.0}
    x = e0
    for k in range(L):
        u = torch.zeros_like(layers[k]) if uniforms is None else uniforms[k]
        j = judge(layer(indptr, indices, values, x, u, eps if uniforms is not None else 0.0), got_y=layers[k])
        out['ratio'], out['share'] = max(out['ratio'], j['ratio']), max(out['share'], j['share'] if uniforms is not None else 0.0)
        x = layers[k]
    stack = torch.stack([y.double() for y in layers])
    out['mean_ratio'] = float(_ratio(mean, stack.sum(0) / L, (L + 1.0) * U32 * stack.abs().sum(0) / L).max())
    return out


def propagate_grad(t_indptr, t_indices, t_values, g, n_layers, mistake=None):
    """d mean(E'_1 .. E'_L) / d E_0 applied to g -- (A^T g + ... + (A^T)^L g) / L, perturbed or not -- over the TRANSPOSED matrix,
    with the bound of the fp32 recurrence h <- g + A^T h (L - 1 times, the last scaled by 1 / L), out = A^T h: a step costs the
    product's (K + 2) u |A^T| (|h| + t) on top of the carried |A^T| t and two roundings of the result (three with the constant
    1 / L), as sgl_referee.horner_each.  ``mistake='lightgcn'``: LightGCN's backward (the g term, / (L + 1)).  -> (grad, tol)."""
    L = int(n_layers)
    g = g.double()
    K2 = ((t_indptr[1:] - t_indptr[:-1]).double() + 2.0).unsqueeze(1) * U32
    absv = None if t_values is None else t_values.abs()
    mul = lambda v, x: sr.referee(t_indptr, t_indices, v, x)['y']                    # noqa: E731
    if mistake == 'lightgcn':
        h = s = g
        for _ in range(L):
            h = mul(t_values, h)
            s = s + h
        return s / (L + 1), None
    h, t = g.clone(), torch.zeros_like(g)
    for j in range(L - 1):
        scale = 1.0 / L if j == L - 2 else 1.0
        carried, local = mul(absv, t), K2 * mul(absv, h.abs() + t)
        h = scale * (g + mul(t_values, h))
        t = scale * (carried + local) + (3.0 if j == L - 2 else 2.0) * U32 * h.abs()
    return mul(t_values, h), mul(absv, t) + K2 * mul(absv, h.abs() + t)


# --------------------------------------------------------------------------------------------------------------------------- inputs
RAGGED = [0, 1, 7, 8, 9, 16, 17, 0, 3, 33, 5, 12, 25, 2, 8, 64, 1, 0, 15, 24]


def ragged_case(d, seed=0, n_cols=53, integer=False):
    """The matrix of the kernel tests: rows of 0, 1, 7, 8, 9, 16, 17, ... edges (around a chunk of 8) and one last row holding half
    of all edges; random columns (duplicates included), normal weights, x = 0.1 * normal [n_cols, d], row_scale in [0.5, 1.5) with a
    negative entry, acc normal.  ``integer``: x of small integers and no weights, so that every sum is exact in fp32.
    -> dict(indptr, indices, values, x, row_scale, acc) on the CPU."""
    g = torch.Generator().manual_seed(1000 * d + seed)
    lengths = RAGGED + [sum(RAGGED)]
    indptr = torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(torch.tensor(lengths), 0)])
    nnz, R = int(indptr[-1]), len(lengths)
    indices = torch.randint(0, n_cols, (nnz,), generator=g).int()
    if integer:
        return {'indptr': indptr, 'indices': indices, 'values': None, 'x': torch.randint(-8, 9, (n_cols, d), generator=g).float(),
                'row_scale': None, 'acc': torch.randint(-8, 9, (R, d), generator=g).float()}
    row_scale = 0.5 + torch.rand(R, generator=g)
    row_scale[3] = -row_scale[3]
    return {'indptr': indptr, 'indices': indices, 'values': torch.randn(nnz, generator=g), 'x': 0.1 * torch.randn(n_cols, d, generator=g),
            'row_scale': row_scale, 'acc': torch.randn(R, d, generator=g)}


def tables(n_users, n_items, d, seed):
    """Base tables of the propagation tests: 0.1 * normal, the two padding rows zero."""
    g = torch.Generator().manual_seed(seed)
    ue, ie = 0.1 * torch.randn(n_users, d, generator=g), 0.1 * torch.randn(n_items, d, generator=g)
    ue[0], ie[0] = 0.0, 0.0
    return ue, ie


# --------------------------------------------------------------------------------------------------------------------------- the step
def perturbed_mean(adj, e, n_layers, eps, uniforms=None, mistake=None):
    """mean(E'_1 .. E'_L) in dense float64 torch under autograd (``adj`` [n, n], ``uniforms``: L tables or None).  Mistakes:
    'e0_in_mean' (LightGCN's mean)."""
    outs = [e] if mistake == 'e0_in_mean' else []
    for k in range(int(n_layers)):
        e = adj @ e
        if uniforms is not None:
            e = e + torch.sign(e).detach() * F.normalize(uniforms[k].double(), dim=-1) * eps
        outs.append(e)
    return torch.stack(outs).mean(0)


def simgcl_step(user_emb, item_emb, adj, n_layers, eps, uid, pos, neg, uniforms1, uniforms2, l2_reg_weight, temperature):
    """One SimGCL training step in dense float64 torch on given negatives and uniforms: BPR on the unperturbed skip-input mean,
    l2_reg of the base rows, plus (weight 1) InfoNCE of the unique users + InfoNCE of the unique items between the two perturbed
    propagations.  -> dict(loss, user_grad, item_grad, cl_loss, users, items)."""
    ue = user_emb.detach().double().clone().requires_grad_(True)
    ie = item_emb.detach().double().clone().requires_grad_(True)
    nu = ue.shape[0]
    e = torch.cat([ue, ie], 0)
    s = perturbed_mean(adj, e, n_layers, eps)
    users, items = s[:nu], s[nu:]
    q = users[uid]
    pos_score = (q * items[pos]).sum(-1)
    neg_score = (q.unsqueeze(1) * items[neg]).sum(-1)
    w = torch.softmax(torch.ones_like(neg_score), -1)
    bpr = -torch.mean((F.logsigmoid(pos_score.view(-1, 1) - neg_score) * w).sum(-1))
    loss = bpr + l2_reg_weight * sr.l2_reg(ue[uid], ie[pos], ie[neg.reshape(-1)])
    v1, v2 = perturbed_mean(adj, e, n_layers, eps, uniforms1), perturbed_mean(adj, e, n_layers, eps, uniforms2)
    u_idx, i_idx = torch.unique(uid), torch.unique(pos)
    cl = sg.info_nce(v1[:nu][u_idx], v2[:nu][u_idx], v2[:nu], temperature, 'cosine') + \
        sg.info_nce(v1[nu:][i_idx], v2[nu:][i_idx], v2[nu:], temperature, 'cosine')
    loss = loss + cl
    loss.backward()
    return {'loss': loss.detach(), 'user_grad': ue.grad, 'item_grad': ie.grad, 'cl_loss': cl.detach(), 'users': users.detach(),
            'items': items.detach()}


# --------------------------------------------------------------------------------------------------------------------------- emulation
def emulate_layer(indptr, indices, values, x, chunk, u, eps, row_scale=None, mistake=None):
    """The perturbed layer in numpy fp32 with a sequential order (spmm_referee.emulate_fp32's: chunks of ``chunk`` edges summed edge
    by edge, a row's partials added in chunk order, row_scale), then q from the squares added left to right, the division, the
    product with eps, the sign and the addition, each rounded once.  -> y' fp32 [R, d].  ``mistake`` plants one bug:
      'copysign'    copysign(1, s) for sign(s): a row without edges moves
      'table_norm'  the noise normalised over the whole table instead of the row
      'centred'     u - 0.5 for u
      'no_sign'     dl added whatever the sign of s
      'per_piece'   every piece of a split row perturbed (with the row's uniforms) before the pieces are added"""
    f32 = np.float32
    ptr, idx = indptr.cpu().numpy(), indices.cpu().numpy()
    val = None if values is None else values.cpu().numpy().astype(f32)
    xs, us = x.cpu().numpy().astype(f32), u.cpu().numpy().astype(f32)
    if mistake == 'centred':
        us = (us - f32(0.5)).astype(f32)
    R, d = len(ptr) - 1, xs.shape[1]
    eps = f32(eps)
    table_q = max(f32(np.sqrt((us.astype(np.float64) ** 2).sum())), f32(1e-12))

    def moved(s, r):
        sq = f32(0)
        for c in range(d):
            sq = f32(sq + f32(us[r, c] * us[r, c]))
        q = table_q if mistake == 'table_norm' else max(f32(np.sqrt(sq)), f32(1e-12))
        dl = ((us[r] / q).astype(f32) * eps).astype(f32)
        sgn = np.copysign(f32(1), s) if mistake == 'copysign' else (np.ones(d, f32) if mistake == 'no_sign' else np.sign(s))
        return (s + (sgn * dl).astype(f32)).astype(f32)

    y = np.zeros((R, d), f32)
    for r in range(R):
        total, s = np.zeros(d, f32), int(ptr[r])
        pieces = (int(ptr[r + 1]) - s + chunk - 1) // chunk
        while s < ptr[r + 1]:
            e = min(s + chunk, int(ptr[r + 1]))
            part = np.zeros(d, f32)
            for j in range(s, e):
                prod = xs[idx[j]] if val is None else (val[j] * xs[idx[j]]).astype(f32)
                part = (part + prod).astype(f32)
            if mistake == 'per_piece' and pieces > 1:
                part = moved(part, r)
            total = (total + part).astype(f32)
            s = e
        if row_scale is not None:
            total = (f32(row_scale[r]) * total).astype(f32)
        y[r] = total if (mistake == 'per_piece' and pieces > 1) else moved(total, r)
    return torch.from_numpy(y)


def emulate_propagation(indptr, indices, values, e0, chunk, n_layers, uniforms=None, eps=0.0, mistake=None):
    """SimGCLNet's forward on ``emulate_layer`` -> (layers, mean) fp32.  ``uniforms`` None: unperturbed.  Mistakes, besides those of
    ``emulate_layer``: 'e0_in_mean' (LightGCN's mean), 'not_fed' (the next layer reads the UNPERTURBED output), 'same_uniforms' (the
    first layer's uniforms for every layer)."""
    L = int(n_layers)
    x, layers = e0.float(), []
    zero = torch.zeros_like(x)
    for k in range(L):
        u = zero if uniforms is None else uniforms[0 if mistake == 'same_uniforms' else k]
        e = eps if uniforms is not None else 0.0
        layer_mistake = mistake if mistake in ('copysign', 'table_norm', 'centred', 'no_sign', 'per_piece') and uniforms is not None else None
        y = emulate_layer(indptr, indices, values, x, chunk, u, e, mistake=layer_mistake)
        layers.append(y)
        x = emulate_layer(indptr, indices, values, x, chunk, zero, 0.0) if mistake == 'not_fed' else y
    acc = layers[0].numpy().copy()
    for y in layers[1:]:
        acc = (acc + y.numpy()).astype(np.float32)
    if mistake == 'e0_in_mean':
        acc = ((acc + e0.float().numpy()).astype(np.float32) * np.float32(1.0 / (L + 1))).astype(np.float32)
    elif L > 1:
        acc = (acc * np.float32(1.0 / L)).astype(np.float32)
    return layers, torch.from_numpy(acc)
