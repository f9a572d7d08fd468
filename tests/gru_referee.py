"""Float64 referee of the fused GRU recurrence (rsa_gru / rsa_gru_backward, recstudio_amd/csrc/rsa_gru.hip) with the error bounds
the fp32 kernel is held to.  Test code only: it calls nothing of recstudio_amd.

THE RULE (torch.nn.GRU, one layer, one direction, batch_first, gate order r, z, n; the reference's module.GRULayer is that
module).  gi [B, L, 3 H] = W_ih x (+ b_ih) is an INPUT here, as it is for the kernel.
    gh_t = W_hh h_{t-1} (+ b_hh)     r = sigma(gi_r + gh_r)     z = sigma(gi_z + gh_z)     n = tanh(gi_n + r gh_n)
    h_t  = (1 - z) n + z h_{t-1}
With `lengths` row b stops at lengths[b]: out[b, t >= lengths[b]] = 0 (a stated deviation: nn.GRU runs on over the padding).
    dh_t = g_out_t + carry_t     dn = dh (1 - z)(1 - n^2)     dz = dh (h_{t-1} - n) z (1 - z)     dr = dn gh_n r (1 - r)
    dgi = [dr, dz, dn]     dgh = [dr, dz, dn r]     carry_{t-1} = dh z + W_hh^T dgh     dh0 = carry_{-1}

THE BOUNDS (u = 2**-24, first order in u, one rounding per fp32 operation, no FMA contraction beyond the matrix cores' one rounding
per accumulated product; no constant is fitted).  Rules used throughout: a rounded sum or product s adds u |s|; a product a b of
operands with tolerances carries |a| tol_b + |b| tol_a; n accumulated products carry the terms' tolerances + (n + 2) u sum |terms|.
  FORWARD, judged STEP BY STEP from the kernel's own h_{t-1} (out[:, t - 1] as the kernel wrote it, exact as an input):
    gh            e_gh  = (H + 2) u sum_k |w_k h_k|  (+ u |gh| for the addition of b_hh)
    r, z          the pre-activation x = gi + gh is rounded once: e_x = e_gh + u |x|.  sigma' <= 1/4, and the evaluation of
                  1 / (1 + exp(-x)) adds an ALLOWANCE arithmetic does not give -- twice the absolute error torch's own fp32 sigmoid
                  shows against float64, measured where the test runs (`activation_allowance`) -- and the kernel's rounded sum
                  and quotient, 2 u sigma:
                      e_s = e_x / 4 + allow_sigmoid + 2 u sigma
    n             x_n = gi_n + r gh_n:  e_xn = |gh_n| e_r + |r| e_ghn + u |r gh_n| + u |x_n|;  tanh' <= 1:
                      e_n = e_xn + allow_tanh
    blend         a = 1 - z: e_a = e_z + u |a|;  a n: |n| e_a + |a| e_n + u |a n|;  z h: |h| e_z + u |z h|;  the sum: + u |h_t|
  BACKWARD, judged against the float64 BPTT of the kernel's own inputs (gi, gh, out, h0, g_out: all exact as inputs), the tolerances
  carried backwards through time with the values:
    r, z, n       as above with e_gh = 0 (gh is an input): e_x = u |x|
    dh            tol_dh = tol_carry + u |dh|
    dn            = (dh (1 - z)) (1 - n n):  m = dh a: |a| tol_dh + |dh| e_a + u |m|;  c = 1 - n n: 2 |n| e_n + u n^2 + u |c|;
                  tol_dn = |c| tol_m + |m| e_c + u |dn|
    dz            = (dh (h_{t-1} - n)) (z (1 - z)):  d = h_{t-1} - n: e_n + u |d|;  m = dh d: |d| tol_dh + |dh| e_d + u |m|;
                  s = z a: |a| e_z + |z| e_a + u |s|;  tol_dz = |s| tol_m + |m| e_s + u |dz|
    dr            = (dn gh_n) (r (1 - r)):  m = dn gh_n: |gh_n| tol_dn + u |m|;  s = r (1 - r) as for z;
                  tol_dr = |s| tol_m + |m| e_s + u |dr|
    dgh_n         = dn r:  |r| tol_dn + |dn| e_r + u |dn r|
    carry         = dh z + W_hh^T dgh:  |z| tol_dh + |dh| e_z + u |dh z|, the 3 H accumulated products
                  sum_m |w_mu| tol_dgh_m + (3 H + 2) u sum_m |w_mu dgh_m|, and the sum: + u |carry|
  Every bound gets TINY = L 2**-126 on top (results below the smallest normal fp32 number carry an absolute error).  An element at
  t >= lengths[b] has bound TINY and must come out as 0 (the tests assert exact zeros there).
"""
import torch

U = 2.0 ** -24
F64 = torch.float64

FORWARD_MISTAKES = ('gate_order_zrn', 'w_hn_of_rh', 'b_hn_outside', 'blend_swapped', 'w_transposed', 'past_len')
BACKWARD_MISTAKES = ('dz_from_h_t', 'carry_without_dh_z', 'past_len', 'dgh_n_without_r')


def f64(t):
    return None if t is None else t.detach().cpu().to(F64)


def live_mask(lengths, B, L):
    """bool [B, L]: t < lengths[b] (all true without lengths)."""
    if lengths is None:
        return torch.ones(B, L, dtype=torch.bool)
    return torch.arange(L).view(1, L) < lengths.detach().cpu().view(B, 1)


def gates(gi, gh, h_prev, mistake=None, w_hh=None, b_hh=None):
    """One step (or all steps at once: any leading shape) from the pre-activations -> dict.  ``gh`` includes b_hh."""
    H = h_prev.shape[-1]
    i_r, i_z, i_n = gi.split(H, dim=-1)
    h_r, h_z, h_n = gh.split(H, dim=-1)
    if mistake == 'gate_order_zrn':
        i_r, i_z, h_r, h_z = i_z, i_r, h_z, h_r
    r = torch.sigmoid(i_r + h_r)
    z = torch.sigmoid(i_z + h_z)
    if mistake == 'w_hn_of_rh':
        h_n = (r * h_prev) @ w_hh[2 * H:].t() + (b_hh[2 * H:] if b_hh is not None else 0.0)
        x_n = i_n + h_n
    elif mistake == 'b_hn_outside' and b_hh is not None:
        x_n = i_n + r * (h_n - b_hh[2 * H:]) + b_hh[2 * H:]
    else:
        x_n = i_n + r * h_n
    n = torch.tanh(x_n)
    h = z * n + (1.0 - z) * h_prev if mistake == 'blend_swapped' else (1.0 - z) * n + z * h_prev
    return dict(r=r, z=z, n=n, h=h, x_r=i_r + h_r, x_z=i_z + h_z, x_n=x_n, gh_n=h_n)


def hidden_product(h, w_hh, b_hh, mistake=None):
    H = h.shape[-1]
    w = w_hh
    if mistake == 'w_transposed':
        w = torch.cat([blk.t() for blk in w_hh.split(H, dim=0)], dim=0)
    gh = h @ w.t()
    return gh + b_hh if b_hh is not None else gh


def forward(gi, w_hh, b_hh=None, h0=None, lengths=None, mistake=None):
    """The free-running float64 recurrence -> out [B, L, H].  ``mistake``: one of FORWARD_MISTAKES (None: the rule)."""
    gi, w_hh, b_hh, h0 = f64(gi), f64(w_hh), f64(b_hh), f64(h0)
    B, L, H3 = gi.shape
    H = H3 // 3
    on = live_mask(None if mistake == 'past_len' else lengths, B, L)
    h = h0 if h0 is not None else torch.zeros(B, H, dtype=F64)
    out = torch.zeros(B, L, H, dtype=F64)
    for t in range(L):
        s = gates(gi[:, t], hidden_product(h, w_hh, b_hh, mistake), h, mistake, w_hh, b_hh)
        m = on[:, t].view(B, 1)
        h = torch.where(m, s['h'], h)
        out[:, t] = torch.where(m, s['h'], torch.zeros_like(h))
    return out


def previous_states(out, h0):
    """h_prev [B, L, H]: h0 (or 0) followed by out[:, :-1]."""
    B, L, H = out.shape
    first = h0.view(B, 1, H) if h0 is not None else torch.zeros(B, 1, H, dtype=out.dtype)
    return torch.cat([first, out[:, :-1]], dim=1)


def _grid():
    return torch.linspace(-16.0, 16.0, 1 << 15, dtype=torch.float32)


def activation_allowance(device, points=None):
    """-> dict(sigmoid, tanh, measured_sigmoid, measured_tanh): the worst ABSOLUTE error of torch's own fp32 sigmoid / tanh on
    ``device`` against float64 on the same fp32 arguments (a fixed grid over [-16, 16] and ``points``, the case's own
    pre-activations), and twice that."""
    x = _grid() if points is None else torch.cat([_grid(), points.detach().cpu().float().reshape(-1)])
    xd = x.to(device)
    es = float((torch.sigmoid(xd).double().cpu() - torch.sigmoid(x.double())).abs().max())
    et = float((torch.tanh(xd).double().cpu() - torch.tanh(x.double())).abs().max())
    return dict(sigmoid=2.0 * es, tanh=2.0 * et, measured_sigmoid=es, measured_tanh=et)


def _sigmoid_tol(e_x, s, allow):
    return e_x / 4 + allow['sigmoid'] + 2 * U * s


def judge_forward(out_k, gi, w_hh, b_hh, h0, lengths, allow):
    """The kernel's ``out_k`` judged step by step from its own h_{t-1} -> (want, tol) [B, L, H] in float64: ``want[:, t]`` is the
    float64 step from ``out_k[:, t - 1]``; zeros with tol TINY at t >= lengths[b]."""
    out_k, gi, w_hh, b_hh, h0 = f64(out_k), f64(gi), f64(w_hh), f64(b_hh), f64(h0)
    B, L, H = out_k.shape
    tiny = L * 2.0 ** -126
    hp = previous_states(out_k, h0)
    gh = hidden_product(hp, w_hh, b_hh)
    s = gates(gi, gh, hp)
    e_gh = (H + 2) * U * (hp.abs() @ w_hh.abs().t())
    if b_hh is not None:
        e_gh = e_gh + U * gh.abs()
    e_r_gh, e_z_gh, e_n_gh = e_gh.split(H, dim=-1)
    r, z, n = s['r'], s['z'], s['n']
    e_r = _sigmoid_tol(e_r_gh + U * s['x_r'].abs(), r, allow)
    e_z = _sigmoid_tol(e_z_gh + U * s['x_z'].abs(), z, allow)
    gh_n = s['gh_n']
    e_n = gh_n.abs() * e_r + r * e_n_gh + U * (r * gh_n).abs() + U * s['x_n'].abs() + allow['tanh']
    a = 1.0 - z
    e_a = e_z + U * a
    tol = (n.abs() * e_a + a * e_n + U * (a * n).abs()) + (hp.abs() * e_z + U * (z * hp).abs()) + U * s['h'].abs() + tiny
    on = live_mask(lengths, B, L).unsqueeze(2)
    want = torch.where(on, s['h'], torch.zeros_like(s['h']))
    tol = torch.where(on, tol, torch.full_like(tol, tiny))
    return want, tol


def backward(gi, gh, out, w_hh, h0, g_out, lengths=None, allow=None, mistake=None):
    """The float64 BPTT of the kernel's own inputs -> dict(dgi, dgh_n, dh0) and, with ``allow``, their tolerances
    (tol_dgi, tol_dgh_n, tol_dh0).  ``mistake``: one of BACKWARD_MISTAKES or 'w_untransposed'."""
    gi, gh, out, w_hh, h0, g_out = f64(gi), f64(gh), f64(out), f64(w_hh), f64(h0), f64(g_out)
    B, L, H = out.shape
    tiny = L * 2.0 ** -126
    hp_all = previous_states(out, h0)
    on_all = live_mask(None if mistake == 'past_len' else lengths, B, L)
    wa = w_hh.abs()
    w_back = w_hh
    if mistake == 'w_untransposed':
        w_back = torch.cat([blk.t() for blk in w_hh.split(H, dim=0)], dim=0)
    carry = torch.zeros(B, H, dtype=F64)
    tol_carry = torch.zeros(B, H, dtype=F64)
    dgi, dgh_n = torch.zeros(B, L, 3 * H, dtype=F64), torch.zeros(B, L, H, dtype=F64)
    tol_dgi, tol_dgh_n = torch.full((B, L, 3 * H), tiny, dtype=F64), torch.full((B, L, H), tiny, dtype=F64)
    zero = torch.zeros(B, H, dtype=F64)
    for t in range(L - 1, -1, -1):
        on = on_all[:, t].view(B, 1)
        hp = hp_all[:, t]
        s = gates(gi[:, t], gh[:, t], hp)
        r, z, n, gh_n = s['r'], s['z'], s['n'], s['gh_n']
        dh = g_out[:, t] + carry
        a = 1.0 - z
        c = 1.0 - n * n
        m_n = dh * a
        dn = m_n * c
        d = (s['h'] if mistake == 'dz_from_h_t' else hp) - n
        m_z = dh * d
        s_z = z * a
        dz = m_z * s_z
        m_r = dn * gh_n
        s_r = r * (1.0 - r)
        dr = m_r * s_r
        dnr = dn if mistake == 'dgh_n_without_r' else dn * r
        keep = zero if mistake == 'carry_without_dh_z' else dh * z
        dgh = torch.cat([dr, dz, dnr], dim=1)
        new = keep + dgh @ w_back
        dgi[:, t] = torch.where(on, torch.cat([dr, dz, dn], dim=1), torch.zeros(B, 3 * H, dtype=F64))
        dgh_n[:, t] = torch.where(on, dnr, zero)
        if allow is not None:
            tol_dh = tol_carry + U * dh.abs()
            e_r = _sigmoid_tol(U * s['x_r'].abs(), r, allow)
            e_z = _sigmoid_tol(U * s['x_z'].abs(), z, allow)
            e_n = gh_n.abs() * e_r + U * (r * gh_n).abs() + U * s['x_n'].abs() + allow['tanh']
            e_a = e_z + U * a
            t_mn = a * tol_dh + dh.abs() * e_a + U * m_n.abs()
            e_c = 2 * n.abs() * e_n + U * n * n + U * c.abs()
            t_dn = c.abs() * t_mn + m_n.abs() * e_c + U * dn.abs()
            e_d = e_n + U * d.abs()
            t_mz = d.abs() * tol_dh + dh.abs() * e_d + U * m_z.abs()
            e_sz = a * e_z + z * e_a + U * s_z
            t_dz = s_z * t_mz + m_z.abs() * e_sz + U * dz.abs()
            t_mr = gh_n.abs() * t_dn + U * m_r.abs()
            ar = 1.0 - r
            e_sr = ar * e_r + r * (e_r + U * ar) + U * s_r
            t_dr = s_r * t_mr + m_r.abs() * e_sr + U * dr.abs()
            t_dnr = r * t_dn + dn.abs() * e_r + U * dnr.abs()
            t_keep = z * tol_dh + dh.abs() * e_z + U * keep.abs()
            t_dgh = torch.cat([t_dr, t_dz, t_dnr], dim=1)
            t_new = t_keep + t_dgh @ wa + (3 * H + 2) * U * (dgh.abs() @ wa) + U * new.abs()
            tol_dgi[:, t] = torch.where(on, torch.cat([t_dr, t_dz, t_dn], dim=1) + tiny, torch.full((B, 3 * H), tiny, dtype=F64))
            tol_dgh_n[:, t] = torch.where(on, t_dnr + tiny, torch.full((B, H), tiny, dtype=F64))
            tol_carry = torch.where(on, t_new, tol_carry)
        carry = torch.where(on, new, carry)
    res = dict(dgi=dgi, dgh_n=dgh_n, dh0=carry)
    if allow is not None:
        res.update(tol_dgi=tol_dgi, tol_dgh_n=tol_dgh_n, tol_dh0=tol_carry + tiny)
    return res


def emulate_fp32(gi, w_hh, b_hh=None, h0=None, lengths=None, g_out=None):
    """The kernel's sequence of operations in fp32 torch ops on the CPU -> (out, gh, (dgi, dgh_n, dh0) or None): the product,
    (acc + b), gi + gh, 1 / (1 + exp(-x)), tanh, (1 - z) n + z h; the backward with its products grouped as the kernel groups
    them and the carry as dh z + ((a0 + a1) + a2) over K blocks 0, 1, 2 mod 3."""
    f = lambda t: None if t is None else t.detach().cpu().float()     # noqa: E731
    gi, w_hh, b_hh, h0 = f(gi), f(w_hh), f(b_hh), f(h0)
    B, L, H3 = gi.shape
    H = H3 // 3
    on_all = live_mask(lengths, B, L)
    one = torch.ones((), dtype=torch.float32)
    sig = lambda x: one / (one + torch.exp(-x))                       # noqa: E731
    h = h0 if h0 is not None else torch.zeros(B, H)
    out = torch.zeros(B, L, H)
    for t in range(L):
        acc = h @ w_hh.t()
        gh = acc + b_hh if b_hh is not None else acc
        i_r, i_z, i_n = gi[:, t].split(H, 1)
        h_r, h_z, h_n = gh.split(H, 1)
        r, z = sig(i_r + h_r), sig(i_z + h_z)
        n = torch.tanh(i_n + r * h_n)
        new = (one - z) * n + z * h
        m = on_all[:, t].view(B, 1)
        h = torch.where(m, new, h)
        out[:, t] = torch.where(m, new, torch.zeros(()))
    hp_all = previous_states(out, h0)
    gh_all = hp_all @ w_hh.t()
    if b_hh is not None:
        gh_all = gh_all + b_hh
    if g_out is None:
        return out, gh_all, None
    g_out = f(g_out)
    carry = torch.zeros(B, H)
    dgi, dgh_n = torch.zeros(B, L, 3 * H), torch.zeros(B, L, H)
    blocks = [torch.cat([torch.arange(kb * 16, kb * 16 + 16) for kb in range(c, 3 * H // 16, 3)]) for c in range(3)]
    for t in range(L - 1, -1, -1):
        m = on_all[:, t].view(B, 1)
        hp = hp_all[:, t]
        i_r, i_z, i_n = gi[:, t].split(H, 1)
        h_r, h_z, h_n = gh_all[:, t].split(H, 1)
        r, z = sig(i_r + h_r), sig(i_z + h_z)
        n = torch.tanh(i_n + r * h_n)
        dh = g_out[:, t] + carry
        dn = (dh * (one - z)) * (one - n * n)
        dz = (dh * (hp - n)) * (z * (one - z))
        dr = (dn * h_n) * (r * (one - r))
        dnr = dn * r
        dgh = torch.cat([dr, dz, dnr], 1)
        a0, a1, a2 = (dgh[:, idx] @ w_hh[idx] for idx in blocks)
        new = dh * z + ((a0 + a1) + a2)
        dgi[:, t] = torch.where(m, torch.cat([dr, dz, dn], 1), torch.zeros(()))
        dgh_n[:, t] = torch.where(m, dnr, torch.zeros(()))
        carry = torch.where(m, new, carry)
    return out, gh_all, (dgi, dgh_n, carry)


def worst_ratio(got, want, tol):
    """max |got - want| / tol."""
    return float(((got.detach().cpu().to(F64) - want).abs() / tol).max())


def make_case(B, L, H, *, bias, with_h0, lengths, seed=0):
    """A seeded case -> dict(gi, w_hh, b_hh, h0, lengths, g_out) of fp32 / int64 CPU tensors.  ``lengths``: None, 'ones', 'full' or
    'mixed' (mixed: lengths differ inside a tile, one row is empty, and EVERY row of the first tile of 16 is shorter than L when
    L > 1, so that tile stops early).  Weights as nn.GRU initialises them (uniform in +-1 / sqrt(H)); gi as a Linear of unit-scale
    rows leaves it."""
    g = torch.Generator().manual_seed(1000 * seed + 31 * B + 7 * L + H)
    k = 1.0 / H ** 0.5
    gi = torch.randn(B, L, 3 * H, generator=g)
    w_hh = (torch.rand(3 * H, H, generator=g) * 2 - 1) * k * 2.0
    b_hh = (torch.rand(3 * H, generator=g) * 2 - 1) * 0.5 if bias else None
    h0 = torch.tanh(torch.randn(B, H, generator=g)) if with_h0 else None
    g_out = torch.randn(B, L, H, generator=g)
    if lengths is None:
        lens = None
    elif lengths == 'ones':
        lens = torch.ones(B, dtype=torch.int64)
    elif lengths == 'full':
        lens = torch.full((B,), L, dtype=torch.int64)
    else:
        lens = torch.randint(0, L + 1, (B,), generator=g)
        if L > 1:
            lens[:16] = torch.randint(0, L, (min(B, 16),), generator=g)
        if B > 1:
            lens[1] = 0
        lens[0] = max(L - 1, 1) if L > 1 else 1
    return dict(gi=gi, w_hh=w_hh, b_hh=b_hh, h0=h0, lengths=lens, g_out=g_out)
