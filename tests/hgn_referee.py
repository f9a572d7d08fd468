"""Float64 referee of HGN's fused hierarchical gating (rsa_hgn_gating / rsa_hgn_gating_backward,
recstudio_amd/csrc/rsa_gating.hip) with the error bounds the fp32 kernel is held to.  Test code only: it calls nothing of
recstudio_amd.

THE RULE (recstudio/model/seq/hgn.py:31-43).  S = item_encoder(in_item_id) [B, L, d] with the zero row at padded positions and NO
mask anywhere; U = user_embedding(user_id) [B, d]; L = in_item_id.size(1) <= max_seq_len:
    ug_b  = W_g_2 U_b + b_g                    [B, d]   an INPUT of the kernel
    ui_bl = U_b . W_g_4.weight[l]   (l < L)    [B, L]   an INPUT of the kernel; W_g_4.bias is never used
    f_bl  = sigmoid(W_g_1 s_bl + ug_b)         sf_bl = s_bl (.) f_bl
    w_bl  = sigmoid(w_g_3 . sf_bl + ui_bl)     si_bl = sf_bl w_bl
    mean: pooled_b = sum_l si_bl / sum_l w_bl  (padded positions have si = 0 but w = sigmoid(ui) > 0: they count in the denominator)
    max : pooled_b[c] = max_l si_bl[c]         (padded positions take part with si = +0)
    out_b = pooled_b + sum_l s_bl              query = U + out
Backward from g_b = d/d out_b:
    mean: dsi = g_b / den_b, dw = -(g_b . pooled_b) / den_b          max: dsi[c] = l == arg_b[c] ? g_b[c] : 0, dw = 0
    dw += dsi . sf     dz = dw w (1 - w)     dui = dz     dw3 = sum_bl dz sf
    dsf = dsi w + dz w3     dpre = (dsf (.) s) (.) f (1 - f)
    dug_b = sum_l dpre     dW1 = sum_bl dpre s^T     dS = g_b + dsf (.) f + W1^T dpre      (NOT zero at padded positions)

THE BOUNDS (u = 2**-24, first order in u, one rounding per fp32 operation; no constant is fitted).  A rounded sum or product s adds
u |s|; a product a b of operands with tolerances carries |a| tol_b + |b| tol_a; a quotient a / b carries tol_a / |b| +
|a| tol_b / b^2; EVERY sum of n terms -- the two-term ones too -- carries the terms' tolerances + (n + 2) u sum |terms|, in
whatever order they are added (so a + b is charged 4 u (|a| + |b|): one rounding of a sum can use up all of u |a + b|).
  FORWARD, judged from the kernel's own inputs (S, ug, ui, W1, w3: exact):
    p = W1 s        e_p = (d + 2) u sum_k |w s|            x = p + ug      e_x = e_p + 4 u (|p| + |ug|)
    f = sigmoid(x)  sigma' <= 1/4; the evaluation of 1 / (1 + exp(-x)) adds an ALLOWANCE arithmetic does not give -- twice the
                    absolute error torch's own fp32 sigmoid shows against float64 where the test runs
                    (ff_attention_referee.sigmoid_allowance) -- and the kernel's rounded sum and quotient:
                    e_f = e_x / 4 + allow + 2 u f
    sf = s f        e_sf = |s| e_f + u |sf|                (a zero row: sf = 0 exactly, e_sf = 0)
    y = w3 . sf     e_y = sum_c |w3| e_sf + (d + 2) u sum_c |w3 sf|           z = y + ui    e_z = e_y + 4 u (|y| + |ui|)
    w = sigmoid(z)  e_w = e_z / 4 + allow + 2 u w
    si = sf w       e_si = |sf| e_w + w e_sf + u |si|
    mean: num = sum_l si   e_num = sum_l e_si + (L + 2) u sum_l |si|          den = sum_l w   e_den = sum_l e_w + (L + 2) u den
          pooled = num / den       e_pool = e_num / den + |num| e_den / den^2 + u |pooled|
    max:  a maximum moves by no more than its operands do:   e_pool = max_l e_si
          arg is VALID when si[arg] >= max_l si - (e_si[arg] + e_si[argmax]), and must be the lowest index among exact ties
    ss = sum_l s    e_ss = (L + 2) u sum_l |s|             out = pooled + ss       e_out = e_pool + e_ss + 4 u (|pooled| + |ss|)
  BACKWARD, judged against the float64 gradients of the same inputs (g exact); the kernel reads its OWN forward w (within e_w) and,
  for max pooling, its own arg, which the referee is handed:
    mean: q = g . sf      t_q = sum_c |g| e_sf + (d + 2) u sum_c |g sf|
          wq = w q        t_wq = |q| e_w + w t_q + u |wq|        n2 = sum_l wq    t_n2 = sum_l t_wq + (L + 2) u sum_l |wq|
          gp = n2 / den   t_gp = t_n2 / den + |n2| e_den / den^2 + u |gp|          (= g . pooled)
          dsi = g / den   t_dsi = |g| e_den / den^2 + u |dsi|
          gpd = gp / den  t_gpd = t_gp / den + |gp| e_den / den^2 + u |gpd|
    max:  dsi is g or 0 exactly: t_dsi = 0, gpd = 0
    dot = dsi . sf        t_dot = sum_c (|dsi| e_sf + |sf| t_dsi) + (d + 2) u sum_c |dsi sf|
    dw = dot - gpd        t_dw = t_dot + t_gpd + 4 u (|dot| + |gpd|)
    a = dw w              t_a = |dw| e_w + w t_dw + u |a|        c1 = 1 - w       t_c1 = e_w + 4 u (1 + w)
    dz = a c1             t_dz = |a| t_c1 + c1 t_a + u |dz|                         (dui)
    dsf = dsi w + dz w3   t_dsf = |dsi| e_w + w t_dsi + u |dsi w| + |w3| t_dz + u |dz w3| + 4 u (|dsi w| + |dz w3|)
    t = dsf f             t_t = |dsf| e_f + f t_dsf + u |t|      m = dsf s        t_m = |s| t_dsf + u |m|
    cf = 1 - f            e_cf = e_f + 4 u (1 + f)                     sl = f cf        e_sl = cf e_f + f e_cf + u sl
    dpre = m sl           t_dpre = sl t_m + |m| e_sl + u |dpre|
    acc = t + W1^T dpre   t_acc = t_t + sum_c |w1| t_dpre + (d + 3) u (|t| + sum_c |w1 dpre|)
    dS = g + acc          t_acc + 4 u (|g| + |acc|)
    dug                   sum_l t_dpre + (L + 2) u sum_l |dpre|
    dW1                   sum_bl |s| t_dpre + (B L + 2) u sum_bl |dpre s|
    dw3                   sum_bl (|sf| t_dz + |dz| e_sf) + (B L + 2) u sum_bl |dz sf|
  Every bound gets TINY = (B L + 2 d) 2**-126 on top.
"""
import torch

from ff_attention_referee import sigmoid_allowance, worst_ratio   # noqa: F401  (re-exported for the tests)

U = 2.0 ** -24
F64 = torch.float64

FORWARD_MISTAKES = ('den_unpadded', 'div_by_L', 'w1_transposed', 'bg_dropped', 'w4_bias_added', 'w4_last_rows', 'gate_from_S',
                    'ssum_missing', 'max_unpadded')
BACKWARD_MISTAKES = ('no_pooled_term', 'no_dz_w3', 'slope_missing', 'ds_without_g')
POOLINGS = ('mean', 'max')


def f64(t):
    return None if t is None else t.detach().cpu().to(F64)


def layer_rule(user, S, w1, w2, b_g, w3, w4, b4, lengths=None, pooling='mean', mistake=None):
    """The float64 rule from the ENCODER's parameters -> (out [B, d] = query - U, w [B, L]).  ``w4`` [max_seq_len, d], ``b4``
    [max_seq_len] (never used by the rule), ``lengths`` [B] (only the mistakes look at them).  ``mistake``: one of
    FORWARD_MISTAKES."""
    user, S, w1, w2, b_g, w3, w4, b4 = (f64(t) for t in (user, S, w1, w2, b_g, w3, w4, b4))
    w3 = w3.reshape(-1)
    B, L, d = S.shape
    real = torch.ones(B, L, dtype=torch.bool) if lengths is None else torch.arange(L).view(1, L) < lengths.cpu().view(B, 1)
    ug = user @ w2.t()
    if mistake != 'bg_dropped':
        ug = ug + b_g
    w4l = w4[-L:] if mistake == 'w4_last_rows' else w4[:L]
    ui = user @ w4l.t()
    if mistake == 'w4_bias_added':
        ui = ui + b4[:L]
    f = torch.sigmoid(S @ (w1 if mistake == 'w1_transposed' else w1.t()) + ug.view(B, 1, d))
    sf = S * f
    w = torch.sigmoid((S if mistake == 'gate_from_S' else sf) @ w3 + ui)
    si = sf * w.unsqueeze(2)
    if pooling == 'mean':
        if mistake == 'den_unpadded':
            den = (w * real.to(F64)).sum(1, keepdim=True)
        elif mistake == 'div_by_L':
            den = torch.full((B, 1), float(L), dtype=F64)
        else:
            den = w.sum(1, keepdim=True)
        pooled = si.sum(1) / den
    else:
        pooled = (si.masked_fill(~real.unsqueeze(2), float('-inf')) if mistake == 'max_unpadded' else si).max(1).values
    return (pooled if mistake == 'ssum_missing' else pooled + S.sum(1)), w


def _gates(S, ug, ui, w1, w3, allow):
    """f, sf, w, si and their tolerances, from the kernel's inputs in float64."""
    B, L, d = S.shape
    a = allow['sigmoid']
    p = S @ w1.t()
    x = p + ug.view(B, 1, d)
    e_x = (d + 2) * U * (S.abs() @ w1.abs().t()) + 4 * U * (p.abs() + ug.abs().view(B, 1, d))
    f = torch.sigmoid(x)
    e_f = e_x / 4 + a + 2 * U * f
    sf = S * f
    e_sf = S.abs() * e_f + U * sf.abs()
    y = sf @ w3
    z = y + ui
    e_z = e_sf @ w3.abs() + (d + 2) * U * (sf.abs() @ w3.abs()) + 4 * U * (y.abs() + ui.abs())
    w = torch.sigmoid(z)
    e_w = e_z / 4 + a + 2 * U * w
    si = sf * w.unsqueeze(2)
    e_si = sf.abs() * e_w.unsqueeze(2) + w.unsqueeze(2) * e_sf + U * si.abs()
    return dict(x=x, f=f, e_f=e_f, sf=sf, e_sf=e_sf, w=w, e_w=e_w, si=si, e_si=e_si)


def _mean_parts(G, L):
    num, den = G['si'].sum(1), G['w'].sum(1, keepdim=True)
    e_num = G['e_si'].sum(1) + (L + 2) * U * G['si'].abs().sum(1)
    e_den = G['e_w'].sum(1, keepdim=True) + (L + 2) * U * den
    pooled = num / den
    return num, den, e_den, pooled, e_num / den + num.abs() * e_den / den ** 2 + U * pooled.abs()


def judge_forward(S, ug, ui, w1, w3, pooling, allow):
    """From the kernel's inputs -> dict(out, w, tol_out, tol_w, si, e_si) in float64."""
    S, ug, ui, w1, w3 = f64(S), f64(ug), f64(ui), f64(w1), f64(w3).reshape(-1)
    B, L, d = S.shape
    tiny = (B * L + 2 * d) * 2.0 ** -126
    G = _gates(S, ug, ui, w1, w3, allow)
    if pooling == 'mean':
        _, _, _, pooled, e_pool = _mean_parts(G, L)
    else:
        pooled, e_pool = G['si'].max(1).values, G['e_si'].max(1).values
    ss = S.sum(1)
    out = pooled + ss
    tol_out = e_pool + (L + 2) * U * S.abs().sum(1) + 4 * U * (pooled.abs() + ss.abs())
    return dict(out=out, w=G['w'], tol_out=tol_out + tiny, tol_w=G['e_w'] + tiny, si=G['si'], e_si=G['e_si'])


def arg_problems(judged, arg):
    """Max pooling: the (b, c) at which the kernel's ``arg`` is out of range, names a position whose float64 si is more than
    e_si[arg] + e_si[argmax] below the float64 maximum, or is not the lowest index among exactly equal float64 values."""
    si, e_si = judged['si'], judged['e_si']
    B, L, d = si.shape
    arg = arg.detach().cpu().long()
    bad = (arg < 0) | (arg >= L)
    a = arg.clamp(0, L - 1).view(B, 1, d)
    at, e_at = si.gather(1, a).squeeze(1), e_si.gather(1, a).squeeze(1)
    top = si.max(1)
    e_top = e_si.gather(1, top.indices.view(B, 1, d)).squeeze(1)
    bad |= top.values - at > e_at + e_top
    lower = torch.arange(L).view(1, L, 1) < a
    bad |= ((si == at.unsqueeze(1)) & lower).any(1)
    return bad.nonzero()


def backward(S, ug, ui, w1, w3, pooling, g, arg=None, allow=None, mistake=None):
    """The float64 gradients of the kernel's inputs -> dict(dS, dug, dui, dw1, dw3) and, with ``allow``, tol_* of each.  Max pooling
    routes through ``arg`` [B, d] (the kernel's own; the float64 argmax when None).  ``mistake``: one of BACKWARD_MISTAKES."""
    S, ug, ui, w1, w3, g = f64(S), f64(ug), f64(ui), f64(w1), f64(w3).reshape(-1), f64(g)
    B, L, d = S.shape
    N = B * L
    tiny = (N + 2 * d) * 2.0 ** -126
    G = _gates(S, ug, ui, w1, w3, allow if allow is not None else dict(sigmoid=0.0))
    f, e_f, sf, e_sf, w, e_w = G['f'], G['e_f'], G['sf'], G['e_sf'], G['w'], G['e_w']
    gb, w_, e_w_ = g.view(B, 1, d), w.unsqueeze(2), e_w.unsqueeze(2)
    zero = torch.zeros(B, L, dtype=F64)
    if pooling == 'mean':
        _, den, e_den, pooled, _ = _mean_parts(G, L)
        q = (gb * sf).sum(2)
        t_q = (gb.abs() * e_sf).sum(2) + (d + 2) * U * (gb * sf).abs().sum(2)
        wq = w * q
        t_wq = q.abs() * e_w + w * t_q + U * wq.abs()
        n2 = wq.sum(1, keepdim=True)
        t_n2 = t_wq.sum(1, keepdim=True) + (L + 2) * U * wq.abs().sum(1, keepdim=True)
        gp = n2 / den
        t_gp = t_n2 / den + n2.abs() * e_den / den ** 2 + U * gp.abs()
        dsi = (g / den).view(B, 1, d).expand(B, L, d)
        t_dsi = (g.abs() * e_den / den ** 2 + U * (g / den).abs()).view(B, 1, d).expand(B, L, d)
        gpd = (gp / den).expand(B, L)
        t_gpd = (t_gp / den + gp.abs() * e_den / den ** 2 + U * (gp / den).abs()).expand(B, L)
        if mistake == 'no_pooled_term':
            gpd = zero
    else:
        idx = G['si'].max(1).indices if arg is None else arg.detach().cpu().long()
        dsi = torch.zeros(B, L, d, dtype=F64).scatter_(1, idx.view(B, 1, d), gb)
        t_dsi = torch.zeros(B, L, d, dtype=F64)
        gpd, t_gpd = zero, zero
    dot = (dsi * sf).sum(2)
    dw = dot - gpd
    a = dw * w
    c1 = 1.0 - w
    dz = a * c1
    dz_ = dz.unsqueeze(2)
    dsf = dsi * w_ if mistake == 'no_dz_w3' else dsi * w_ + dz_ * w3
    t = dsf * f
    m = dsf * S
    cf = 1.0 - f
    sl = torch.ones_like(f) if mistake == 'slope_missing' else f * cf
    dpre = m * sl
    acc = t + dpre @ w1
    dS = acc if mistake == 'ds_without_g' else gb + acc
    res = dict(dS=dS, dug=dpre.sum(1), dui=dz, dw1=dpre.reshape(N, d).t() @ S.reshape(N, d), dw3=(dz_ * sf).sum((0, 1)))
    if allow is None:
        return res
    t_dot = (dsi.abs() * e_sf + sf.abs() * t_dsi).sum(2) + (d + 2) * U * (dsi * sf).abs().sum(2)
    t_dw = t_dot + t_gpd + 4 * U * (dot.abs() + gpd.abs())
    t_a = dw.abs() * e_w + w * t_dw + U * a.abs()
    t_c1 = e_w + 4 * U * (1.0 + w)
    t_dz = a.abs() * t_c1 + c1 * t_a + U * dz.abs()
    t_dz_ = t_dz.unsqueeze(2)
    t_dsf = (dsi.abs() * e_w_ + w_ * t_dsi + U * (dsi * w_).abs() + w3.abs() * t_dz_ + U * (dz_ * w3).abs() + 4 * U * ((dsi * w_).abs() + (dz_ * w3).abs()))
    t_t = dsf.abs() * e_f + f * t_dsf + U * t.abs()
    t_m = S.abs() * t_dsf + U * m.abs()
    e_cf = e_f + 4 * U * (1.0 + f)
    e_sl = cf * e_f + f * e_cf + U * sl
    t_dpre = sl * t_m + m.abs() * e_sl + U * dpre.abs()
    wa = w1.abs()
    res['tol_dS'] = (t_t + t_dpre @ wa + (d + 3) * U * (t.abs() + dpre.abs() @ wa)
                     + 4 * U * (gb.abs() + acc.abs()) + tiny)
    res['tol_dug'] = t_dpre.sum(1) + (L + 2) * U * dpre.abs().sum(1) + tiny
    res['tol_dui'] = t_dz + tiny
    sa = S.abs().reshape(N, d)
    res['tol_dw1'] = t_dpre.reshape(N, d).t() @ sa + (N + 2) * U * (dpre.abs().reshape(N, d).t() @ sa) + tiny
    res['tol_dw3'] = ((sf.abs() * t_dz_ + dz_.abs() * e_sf).sum((0, 1)) + (N + 2) * U * (dz_ * sf).abs().sum((0, 1)) + tiny)
    return res


def emulate_fp32(S, ug, ui, w1, w3, pooling, g=None):
    """The kernel's sequence of operations in fp32 torch ops on the CPU -> (out, w, arg or None, (dS, dug, dui, dw1, dw3) or None):
    the product, + ug, 1 / (1 + exp(-x)), the dot with w3 channel by channel, the pooling position by position (strict > for the
    max: the lowest index wins ties); the backward with its products grouped as the kernel groups them."""
    c = lambda t: t.detach().cpu().float()     # noqa: E731
    S, ug, ui, w1, w3 = c(S), c(ug), c(ui), c(w1), c(w3).reshape(-1)
    B, L, d = S.shape
    one = torch.ones((), dtype=torch.float32)
    f = one / (one + torch.exp(-(S @ w1.t() + ug.view(B, 1, d))))
    sf = S * f
    y = torch.zeros(B, L)
    for k in range(d):
        y = y + w3[k] * sf[:, :, k]
    w = one / (one + torch.exp(-(y + ui)))
    num, den, ss = torch.zeros(B, d), torch.zeros(B, 1), torch.zeros(B, d)
    mx, arg = torch.full((B, d), float('-inf')), torch.zeros(B, d, dtype=torch.int32)
    for l in range(L):
        si = sf[:, l] * w[:, l].view(B, 1)
        num, den, ss = num + si, den + w[:, l].view(B, 1), ss + S[:, l]
        up = si > mx
        mx, arg = torch.where(up, si, mx), torch.where(up, torch.full_like(arg, l), arg)
    out = (num / den if pooling == 'mean' else mx) + ss
    arg = arg if pooling == 'max' else None
    if g is None:
        return out, w, arg, None
    g = c(g)
    gb = g.view(B, 1, d)
    if pooling == 'mean':
        q = torch.zeros(B, L)
        for k in range(d):
            q = q + g[:, k].view(B, 1) * sf[:, :, k]
        n2 = torch.zeros(B, 1)
        for l in range(L):
            n2 = n2 + (w[:, l] * q[:, l]).view(B, 1)
        gp = n2 / den
        dsi = (g / den).view(B, 1, d).expand(B, L, d)
        gpd = (gp / den).expand(B, L)
    else:
        dsi = torch.zeros(B, L, d).scatter_(1, arg.long().view(B, 1, d), gb)
        gpd = torch.zeros(B, L)
    dot = torch.zeros(B, L)
    for k in range(d):
        dot = dot + dsi[:, :, k] * sf[:, :, k]
    dw = dot - gpd if pooling == 'mean' else dot
    dz = dw * w * (one - w)
    dsf = dsi * w.unsqueeze(2) + dz.unsqueeze(2) * w3
    dpre = (dsf * S) * (f * (one - f))
    dS = gb + (dsf * f + dpre @ w1)
    dug = torch.zeros(B, d)
    for l in range(L):
        dug = dug + dpre[:, l]
    dw1 = dpre.reshape(B * L, d).t() @ S.reshape(B * L, d)
    dw3 = (dz.unsqueeze(2) * sf).reshape(B * L, d).sum(0)
    return out, w, arg, (dS, dug, dz, dw1, dw3)


PADS = (None, 'suffix', 'whole')


def make_lengths(B, L, kind, gen):
    """int64 [B]: the number of real (non-zero) rows of each right-padded sequence.  None: all L.  'suffix': random, lengths 1
    and L included.  'whole': as 'suffix' with the last sequence padded whole."""
    if kind is None:
        return torch.full((B,), L, dtype=torch.int64)
    lens = torch.randint(1, L + 1, (B,), generator=gen)
    lens[0] = 1
    if B > 1:
        lens[1] = L
    if kind == 'whole':
        lens[B - 1] = 0
    return lens


def make_case(B, L, d, *, pad=None, max_seq_len=None, seed=0, lengths=None):
    """A seeded encoder-level case -> dict(user, S, w1, w2, b_g, w3, w4, b4, lengths, g) of fp32 CPU tensors.  S has ZERO rows at
    l >= lengths[b]; weights as nn.Linear initialises them (scaled up so that the gates move), b_g and W_g_4.bias well away
    from 0, max_seq_len > L so that W_g_4.weight[:L] is a proper slice."""
    max_seq_len = L + 3 if max_seq_len is None else max_seq_len
    gen = torch.Generator().manual_seed(1000 * seed + 131 * B + 17 * L + 3 * d)
    k = 1.0 / d ** 0.5
    r = lambda *s: (torch.rand(*s, generator=gen) * 2 - 1)     # noqa: E731
    lens = make_lengths(B, L, pad, gen) if lengths is None else torch.as_tensor(lengths, dtype=torch.int64)
    S = torch.randn(B, L, d, generator=gen) * (torch.arange(L).view(1, L, 1) < lens.view(B, 1, 1))
    return dict(user=torch.randn(B, d, generator=gen), S=S, w1=r(d, d) * k * 2.0, w2=r(d, d) * k * 2.0, b_g=r(d) * 0.5 + 0.25,
                w3=r(1, d) * k * 2.0, w4=r(max_seq_len, d) * k * 2.0, b4=r(max_seq_len) * 0.5 + 1.0, lengths=lens,
                g=torch.randn(B, d, generator=gen))


def kernel_inputs(case):
    """What the kernel is handed for an encoder-level case: dict(S, ug, ui, w1, w3, g); ug and ui as the fp32 GEMMs leave them."""
    L = case['S'].shape[1]
    ug = torch.nn.functional.linear(case['user'], case['w2']) + case['b_g']
    ui = case['user'] @ case['w4'][:L].t()
    return dict(S=case['S'], ug=ug, ui=ui, w1=case['w1'], w3=case['w3'].reshape(-1), g=case['g'])
