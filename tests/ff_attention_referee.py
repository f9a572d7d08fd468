"""Float64 referee of the fused feed-forward attention pooling (rsa_ff_attention / rsa_ff_attention_backward,
recstudio_amd/csrc/rsa_ffattn.hip) with the error bounds the fp32 kernel is held to.  Test code only: it calls nothing of
recstudio_amd.

THE RULE (recstudio/model/module/layers.py:322-399, AttentionLayer(q_dim, k_dim, mlp_layers=[M], activation='sigmoid') with
attention_type='feedforward', ONE query per sequence, softmax=False, value = key).  W1 [M, q_dim + k_dim], b1 [M] or none,
w2 [1, M], b2 [1]:
    qh_b   = W1[:, :q_dim] q_b (+ b1)                         [B, M]     an INPUT of the kernel
    hid_bs = sigmoid(qh_b + W1[:, q_dim:] k_bs)               [B, S, M]
    a_bs   = key_pad[b, s] ? 0 : (w2 . hid_bs + b2) * scale   [B, S]     scale = 1 / sqrt(q_dim)
    out_b  = sum_s a_bs k_bs                                  [B, D]
The divisor is sqrt(q_dim) (not k_dim, not q_dim + k_dim); the mask fills with 0 and there is no softmax; b2 reaches every live
position.  `scale` enters as the exact fp32 value handed to the kernel.
Backward from g_b = d/d out_b, at live positions (everything is 0 at padded ones):
    da = g_b . k_bs     de = da * scale     dpre = (de * w2) * (hid (1 - hid))
    dkey = a g_b + W_k^T dpre     dqh_b = sum_s dpre_bs     dW_k = sum_bs dpre k^T     dw2 = sum_bs de hid     db2 = sum_bs de

THE BOUNDS (u = 2**-24, first order in u, one rounding per fp32 operation; no constant is fitted).  A rounded sum or product s adds
u |s|; a product a b of operands with tolerances carries |a| tol_b + |b| tol_a; n accumulated products carry the terms' tolerances
+ (n + 2) u sum |terms|.
  FORWARD, judged from the kernel's own inputs (key, qh, W_k, w2, b2, key_pad: exact):
    p = W_k k       e_p = (D + 2) u sum_k |w k|
    x = qh + p      e_x = e_p + u |x|
    hid             sigma' <= 1/4; the evaluation of 1 / (1 + exp(-x)) adds an ALLOWANCE arithmetic does not give -- twice the
                    absolute error torch's own fp32 sigmoid shows against float64 where the test runs (`sigmoid_allowance`) -- and
                    the kernel's rounded sum and quotient:   e_h = e_x / 4 + allow + 2 u hid
    e = w2 . hid + b2       e_e = sum_m |w2| e_h + (M + 2) u sum_m |w2 hid| + u |e|
    a = e * scale           e_a = |scale| e_e + u |a|          (padded: a = 0 exactly, bound TINY)
    out = sum_s a k         sum_s |k| e_a + (S + 2) u sum_s |a k|
  BACKWARD, judged against the float64 gradients of the same inputs (g exact):
    da = g . k      t_da = (D + 2) u sum |g k|          de = da * scale     t_de = |scale| t_da + u |de|
    m = de * w2     t_m = |w2| t_de + u |m|             c = 1 - hid         e_c = e_h + u c
    s = hid * c     e_s = c e_h + hid e_c + u s         dpre = m * s        t_dpre = s t_m + |m| e_s + u |dpre|
    dkey            |g| e_a + u |a g| + sum_m |w| t_dpre + (M + 2) u sum_m |w dpre| + u |dkey|
    dqh             sum_s t_dpre + (S + 2) u sum_s |dpre|
    dW_k            sum_bs |k| t_dpre + (B S + 2) u sum_bs |dpre k|
    dw2             sum_bs (hid t_de + |de| e_h) + (B S + 2) u sum_bs |de hid|
    db2             sum_bs t_de + (B S + 2) u sum_bs |de|
  Every bound gets TINY = (B S + M + D) 2**-126 on top.  Elements at padded positions have bound TINY and must come out as 0.
"""
import math

import torch

U = 2.0 ** -24
F64 = torch.float64

FORWARD_MISTAKES = ('div_sqrt_k_dim', 'div_sqrt_q_plus_k', 'w1_halves_swapped', 'b2_dropped', 'b1_dropped', 'mask_ignored',
                    'mask_inf_softmax')
BACKWARD_MISTAKES = ('dkey_without_ag', 'dkey_without_wdpre', 'slope_missing', 'dqh_over_padded')


def f64(t):
    return None if t is None else t.detach().cpu().to(F64)


def fp32_scale(q_dim):
    """The fp32 value of 1 / sqrt(q_dim) the kernel is handed, as a Python float."""
    return float(torch.tensor(1.0 / math.sqrt(q_dim), dtype=torch.float32))


def live_of(key_pad, B, S):
    if key_pad is None:
        return torch.ones(B, S, dtype=torch.bool)
    return ~key_pad.detach().cpu().bool()


def layer_rule(query, key, w1, b1, w2, b2, key_pad=None, mistake=None):
    """The float64 rule from the LAYER's parameters -> (out [B, D], a [B, S]).  ``mistake``: one of FORWARD_MISTAKES."""
    query, key, w1, b1, w2, b2 = f64(query), f64(key), f64(w1), f64(b1), f64(w2), f64(b2)
    B, S, D = key.shape
    q_dim = query.shape[1]
    w_q, w_k = w1[:, :q_dim], w1[:, q_dim:]
    if mistake == 'w1_halves_swapped':                     # cat(key, query) instead of cat(query, key)
        w_k, w_q = w1[:, :D], w1[:, D:]
    qh = query @ w_q.t()
    if b1 is not None and mistake != 'b1_dropped':
        qh = qh + b1
    hid = torch.sigmoid(qh.view(B, 1, -1) + key @ w_k.t())
    e = hid @ w2.reshape(-1)
    if mistake != 'b2_dropped':
        e = e + b2.reshape(())
    div = {'div_sqrt_k_dim': D, 'div_sqrt_q_plus_k': q_dim + D}.get(mistake, q_dim) ** 0.5
    a = e / div
    live = live_of(key_pad, B, S)
    if mistake == 'mask_inf_softmax':
        a = torch.softmax(a.masked_fill(~live, float('-inf')), dim=1)
    elif mistake != 'mask_ignored':
        a = a * live.to(F64)
    return (a.unsqueeze(1) @ key).squeeze(1), a


def sigmoid_allowance(device, points=None):
    """-> dict(sigmoid, measured): the worst ABSOLUTE error of torch's own fp32 sigmoid on ``device`` against float64 on the same
    fp32 arguments (a fixed grid over [-16, 16] and ``points``, the case's own pre-activations), and twice that."""
    x = torch.linspace(-16.0, 16.0, 1 << 15, dtype=torch.float32)
    if points is not None:
        x = torch.cat([x, points.detach().cpu().float().reshape(-1)])
    es = float((torch.sigmoid(x.to(device)).double().cpu() - torch.sigmoid(x.double())).abs().max())
    return dict(sigmoid=2.0 * es, measured=es)


def _hidden(key, qh, w_k, allow):
    """hid [B, S, M] and its tolerance e_h."""
    B, S, D = key.shape
    p = key @ w_k.t()
    x = qh.view(B, 1, -1) + p
    hid = torch.sigmoid(x)
    e_x = (D + 2) * U * (key.abs() @ w_k.abs().t()) + U * x.abs()
    return hid, e_x / 4 + allow['sigmoid'] + 2 * U * hid, x


def _weights(key, qh, w_k, w2, b2, live, scale, allow):
    hid, e_h, x = _hidden(key, qh, w_k, allow)
    M = w_k.shape[0]
    e = hid @ w2 + b2
    e_e = e_h @ w2.abs() + (M + 2) * U * (hid @ w2.abs()) + U * e.abs()
    a = e * scale
    e_a = abs(scale) * e_e + U * a.abs()
    lf = live.to(F64)
    return hid, e_h, a * lf, e_a * lf, x


def judge_forward(key, qh, w_k, w2, b2, key_pad, scale, allow):
    """From the kernel's inputs -> dict(out, a, tol_out, tol_a) in float64."""
    key, qh, w_k, w2, b2 = f64(key), f64(qh), f64(w_k), f64(w2).reshape(-1), f64(b2).reshape(())
    B, S, D = key.shape
    M = w_k.shape[0]
    tiny = (B * S + M + D) * 2.0 ** -126
    live = live_of(key_pad, B, S)
    hid, e_h, a, e_a, _ = _weights(key, qh, w_k, w2, b2, live, scale, allow)
    out = (a.unsqueeze(1) @ key).squeeze(1)
    tol_out = (e_a.unsqueeze(1) @ key.abs()).squeeze(1) + (S + 2) * U * (a.abs().unsqueeze(1) @ key.abs()).squeeze(1)
    return dict(out=out, a=a, tol_out=tol_out + tiny, tol_a=e_a + tiny)


def backward(key, qh, w_k, w2, b2, key_pad, scale, g, allow=None, mistake=None):
    """The float64 gradients of the kernel's inputs -> dict(dkey, dqh, dw_k, dw2, db2) and, with ``allow``, tol_* of each.
    ``mistake``: one of BACKWARD_MISTAKES."""
    key, qh, w_k, w2, b2, g = f64(key), f64(qh), f64(w_k), f64(w2).reshape(-1), f64(b2).reshape(()), f64(g)
    B, S, D = key.shape
    M = w_k.shape[0]
    N = B * S
    tiny = (N + M + D) * 2.0 ** -126
    live = live_of(key_pad, B, S)
    lf = live.to(F64)
    al = allow if allow is not None else dict(sigmoid=0.0)
    hid, e_h, a, e_a, _ = _weights(key, qh, w_k, w2, b2, live, scale, al)
    da = (key * g.view(B, 1, D)).sum(2)
    de_all = da * scale
    de = de_all * lf
    m = de.unsqueeze(2) * w2
    c = 1.0 - hid
    s = torch.ones_like(hid) if mistake == 'slope_missing' else hid * c
    dpre = m * s
    ag = a.unsqueeze(2) * g.view(B, 1, D)
    wd = dpre @ w_k
    dkey = (wd if mistake == 'dkey_without_ag' else ag if mistake == 'dkey_without_wdpre' else ag + wd) * lf.unsqueeze(2)
    dpre_q = (de_all.unsqueeze(2) * w2) * s if mistake == 'dqh_over_padded' else dpre
    res = dict(dkey=dkey, dqh=dpre_q.sum(1), dw_k=dpre.reshape(N, M).t() @ key.reshape(N, D), dw2=(de.unsqueeze(2) * hid).sum((0, 1)),
               db2=de.sum().reshape(1))
    if allow is None:
        return res
    t_da = (D + 2) * U * (key.abs() * g.abs().view(B, 1, D)).sum(2)
    t_de = (abs(scale) * t_da + U * de.abs()) * lf
    t_m = t_de.unsqueeze(2) * w2.abs() + U * m.abs()
    e_c = e_h + U * c
    e_s = c * e_h + hid * e_c + U * s
    t_dpre = s * t_m + m.abs() * e_s + U * dpre.abs()
    wa = w_k.abs()
    t_dkey = (g.abs().view(B, 1, D) * e_a.unsqueeze(2) + U * ag.abs() + t_dpre @ wa + (M + 2) * U * (dpre.abs() @ wa) + U * dkey.abs())
    res['tol_dkey'] = t_dkey * lf.unsqueeze(2) + tiny
    res['tol_dqh'] = t_dpre.sum(1) + (S + 2) * U * dpre.abs().sum(1) + tiny
    ka = key.abs().reshape(N, D)
    res['tol_dw_k'] = t_dpre.reshape(N, M).t() @ ka + (N + 2) * U * (dpre.abs().reshape(N, M).t() @ ka) + tiny
    res['tol_dw2'] = ((hid * t_de.unsqueeze(2) + de.abs().unsqueeze(2) * e_h).sum((0, 1))
                      + (N + 2) * U * (de.abs().unsqueeze(2) * hid).sum((0, 1)) + tiny)
    res['tol_db2'] = (t_de.sum() + (N + 2) * U * de.abs().sum()).reshape(1) + tiny
    return res


def emulate_fp32(key, qh, w_k, w2, b2, key_pad, scale, g=None):
    """The kernel's sequence of operations in fp32 torch ops on the CPU -> (out, a, (dkey, dqh, dw_k, dw2, db2) or None): the
    product, qh + p, 1 / (1 + exp(-x)), the dot with w2 in ascending hidden order, (e + b2) * scale, the pooling position by
    position; the backward with its products grouped as the kernel groups them."""
    f = lambda t: None if t is None else t.detach().cpu().float()     # noqa: E731
    key, qh, w_k, w2, b2 = f(key), f(qh), f(w_k), f(w2).reshape(-1), f(b2).reshape(())
    B, S, D = key.shape
    M = w_k.shape[0]
    one = torch.ones((), dtype=torch.float32)
    sc = torch.tensor(scale, dtype=torch.float32)
    live = live_of(key_pad, B, S)
    hid = one / (one + torch.exp(-(qh.view(B, 1, M) + key @ w_k.t())))
    e = torch.zeros(B, S)
    for mm in range(M):
        e = e + w2[mm] * hid[:, :, mm]
    a = torch.where(live, (e + b2) * sc, torch.zeros(()))
    out = torch.zeros(B, D)
    for s in range(S):
        out = out + a[:, s].view(B, 1) * key[:, s]
    if g is None:
        return out, a, None
    g = f(g)
    da = torch.zeros(B, S)
    for d in range(D):
        da = da + key[:, :, d] * g[:, d].view(B, 1)
    de = torch.where(live, da * sc, torch.zeros(()))
    dpre = (de.unsqueeze(2) * w2) * (hid * (one - hid))
    dkey = torch.where(live.unsqueeze(2), a.unsqueeze(2) * g.view(B, 1, D) + dpre @ w_k, torch.zeros(()))
    dqh = torch.zeros(B, M)
    for s in range(S):
        dqh = dqh + dpre[:, s]
    dw_k = dpre.reshape(B * S, M).t() @ key.reshape(B * S, D)
    dw2 = (de.unsqueeze(2) * hid).reshape(B * S, M).sum(0)
    db2 = de.sum().reshape(1)
    return out, a, (dkey, dqh, dw_k, dw2, db2)


def worst_ratio(got, want, tol):
    """max |got - want| / tol."""
    return float(((got.detach().cpu().to(F64) - want).abs() / tol).max())


PADS = (None, 'suffix', 'holes', 'whole')


def make_pad(B, S, kind, g):
    """bool [B, S] or None.  'suffix': right-padded, lengths 1 and S included; 'holes': scattered; 'whole': as 'suffix' with one
    sequence padded whole."""
    if kind is None:
        return None
    if kind == 'holes':
        pad = torch.rand(B, S, generator=g) < 0.3
        pad[0, 0] = S > 1                                  # (at least one padded position whenever there is room for a live one)
        return pad
    lens = torch.randint(1, S + 1, (B,), generator=g)
    lens[0] = 1
    if B > 1:
        lens[1] = S
    if kind == 'whole':
        lens[B - 1] = 0
    return torch.arange(S).view(1, S) >= lens.view(B, 1)


def make_case(B, S, D, M, *, q_dim=None, bias=True, pad=None, seed=0):
    """A seeded layer-level case -> dict(query, key, w1, b1, w2, b2, key_pad, g) of fp32 / bool CPU tensors.  The keys are
    NON-ZERO at padded positions (a leaked weight must show); weights as nn.Linear initialises them, b2 well away from 0."""
    q_dim = D if q_dim is None else q_dim
    g = torch.Generator().manual_seed(1000 * seed + 131 * B + 17 * S + 3 * D + M)
    k1, k2 = 1.0 / (q_dim + D) ** 0.5, 1.0 / M ** 0.5
    return dict(query=torch.randn(B, q_dim, generator=g), key=torch.randn(B, S, D, generator=g),
                w1=(torch.rand(M, q_dim + D, generator=g) * 2 - 1) * k1 * 2.0,
                b1=(torch.rand(M, generator=g) * 2 - 1) * 0.5 if bias else None,
                w2=(torch.rand(1, M, generator=g) * 2 - 1) * k2 * 2.0, b2=torch.tensor([0.37]),
                key_pad=make_pad(B, S, pad, g), g=torch.randn(B, D, generator=g))


def kernel_inputs(case):
    """What the kernel is handed for a layer-level case: dict(key, qh, w_k, w2, b2, key_pad, scale, g); qh as the fp32 GEMM
    leaves it."""
    q_dim = case['query'].shape[1]
    qh = torch.nn.functional.linear(case['query'], case['w1'][:, :q_dim], case['b1'])
    return dict(key=case['key'], qh=qh, w_k=case['w1'][:, q_dim:], w2=case['w2'].reshape(-1), b2=case['b2'], key_pad=case['key_pad'],
                scale=fp32_scale(q_dim), g=case['g'])
