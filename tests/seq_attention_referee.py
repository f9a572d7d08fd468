"""Float64 referee of the fused attention core (rsa_attention / rsa_attention_backward, recstudio_amd/csrc/rsa_attention.hip) with
the error bounds the fp32 kernel is held to.  Test code only: it calls nothing of recstudio_amd.

THE RULE (what nn.MultiheadAttention computes between in_proj and out_proj under the reference's bool causal mask and key-padding
mask, recstudio/model/seq/sasrec.py:44-53).  qkv [B, L, 3 D] = q | k | v, head h in columns h dh .. of each.
    s_ij  = scale <q_i, k_j>                       allowed(i, j) = (not causal or j <= i) and not key_pad[b, j]
    P_i.  = softmax over the allowed j             lse_i = log sum_allowed exp(s_ij)
    Pt_ij = keep_ij P_ij / q                       out_i = sum_j Pt_ij v_j
A query without an allowed key: out = 0, lse = -inf, no gradient (a stated deviation: torch gives NaN).  The dropout is NOT
nn.Dropout's stream: q = fp32(1 - p), keep = torch.rand([B, H, L, L]) < q, the kept probability DIVIDED by q.
    D_i = sum_c g_ic out_ic     dPt_ij = <g_i, v_j>     dS_ij = P_ij (keep_ij dPt_ij / q - D_i)
    dq_i = scale sum_j dS_ij k_j     dk_j = scale sum_i dS_ij q_i     dv_j = sum_i Pt_ij g_i

THE BOUNDS (u = 2**-24, no FMA contraction assumed beyond the matrix cores' one rounding per accumulated product, first order in u;
no constant is fitted).
  scores     dh products and dh accumulations, the product with `scale`, and the hardware exponential's argument (2^(x log2 e): the
             rounded product with the rounded constant is an argument error of 2 u |x|):
                 e_s = (dh + 2) u scale sum_c |q_ic k_jc| + 2 u |s_ij|
  softmax    P_ij = exp(s_ij - m) / sum_k exp(s_ik - m) moves by at most e_s(ij) + max_k e_s(ik) relative, the sum of at most L
             terms and the quotient add (L + 4) u, and the evaluation of exp itself adds an ALLOWANCE that arithmetic does not
             give: twice the error torch's own fp32 softmax shows against float64 on the same fp32 scores, measured where the
             test runs (`softmax_allowance`, in units of u):
                 rel_P(i) = 2 max_j e_s(ij) + (L + 4 + allow) u
  out        the division by q and the L accumulated products:
                 tol_out = (rel_P(i) + (L + 2) u) sum_j |Pt_ij v_jc|
  lse        m + log(sum): the maximum carries e_s, the sum (L + 4 + allow) u relative = absolute in the logarithm, the logarithm
             and the addition are rounded once each, and so was s - m inside the exponentials:
                 tol_lse = max_j e_s(ij) + (L + 4 + allow) u + u (2 |lse - m| + |m| + |lse|)
  backward   P is recomputed as exp(s - lse32) from the forward's fp32 lse:
                 rel_Pb(ij) = e_s(ij) + tol_lse(i) + 2 u |s_ij - lse_i| + allow u
             and every further quantity carries the tolerance of its operands through the first-order rules (product a b:
             |a| tol_b + |b| tol_a + u |a b|; n accumulated products: the terms' tolerances + (n + 2) u sum |terms|):
                 tol_D   = sum_c |g_ic| tol_out(ic) + (dh + 2) u sum_c |g_ic out_ic|
                 tol_dPt = (dh + 2) u sum_c |g_ic v_jc|
                 a = keep dPt / q: tol_a = keep (tol_dPt / q + u |a|);   t = a - D: tol_t = tol_a + tol_D + u |t|
                 tol_dS  = P tol_t + |t| P rel_Pb + u |dS|
                 tol_dq  = scale (sum_j tol_dS |k_jc| + (L + 2) u sum_j |dS_ij k_jc|) + u |dq|        (dk alike, over i)
                 tol_dv  = sum_i Pt_ij (rel_Pb + u) |g_ic| + (L + 2) u sum_i |Pt_ij g_ic|
  Every bound gets TINY = L 2**-126 on top: results below the smallest normal fp32 number carry an absolute, not a relative,
  error.  An element through which nothing flows has bound TINY and must come out as 0 (the tests assert exact zeros there).
"""
import math

import torch

U = 2.0 ** -24
F64 = torch.float64


def q_of(p):
    """fp32(1 - p) as a python float; 1.0 for p == 0."""
    return float(torch.tensor(1.0 - float(p), dtype=torch.float32)) if p else 1.0


def split(qkv, H, layout='3hd'):
    """qkv [B, L, 3 D] -> q, k, v [B, H, L, dh] (views in qkv's dtype).  ``layout='h3d'`` is the seeded mistake that reads a row as
    [H, 3, dh]."""
    B, L, D3 = qkv.shape
    dh = D3 // 3 // H
    if layout == '3hd':
        t = qkv.reshape(B, L, 3, H, dh).permute(2, 0, 3, 1, 4)
    else:
        t = qkv.reshape(B, L, H, 3, dh).permute(3, 0, 2, 1, 4)
    return t[0], t[1], t[2]


def allowed(key_pad, causal, B, L, mistake=None):
    """bool [B, 1, L, L]."""
    ok = torch.ones(L, L, dtype=torch.bool)
    if causal:
        ok = torch.tril(ok, diagonal=-1 if mistake == 'causal_strict' else 0)
    ok = ok.view(1, 1, L, L).expand(B, 1, L, L)
    if key_pad is not None:
        kp = key_pad.bool().cpu()
        ok = ok & (~kp.view(B, 1, L, 1) if mistake == 'pad_on_queries' else ~kp.view(B, 1, 1, L))
    return ok


def forward(qkv, key_pad, causal, H, keep=None, p=0.0, scale=None, mistake=None):
    """The forward in float64 -> dict.  ``keep`` bool / uint8 [B, H, L, L] when p != 0.  ``mistake``: one of the seeded mistakes of
    tests/test_seq_attention_referee.py (None: the rule)."""
    qkv = qkv.detach().cpu().to(F64)
    B, L, D3 = qkv.shape
    D = D3 // 3
    dh = D // H
    q, k, v = split(qkv, H, 'h3d' if mistake == 'layout' else '3hd')
    scale = 1.0 / math.sqrt(dh) if scale is None else float(scale)
    s = (q @ k.transpose(2, 3)) * (1.0 if mistake == 'no_scale' else scale)
    ok = allowed(key_pad, causal, B, L, mistake).expand(B, H, L, L)
    some = ok.any(3, keepdim=True)
    if mistake == 'uniform_masked_row':
        ok = ok | ~some
        s = torch.where(some, s, torch.zeros_like(s))
        some = torch.ones_like(some)
    sm = s.masked_fill(~ok, float('-inf'))
    m = torch.where(some, sm.amax(3, keepdim=True), torch.zeros_like(sm[..., :1]))
    e = torch.where(ok, (s - m).exp(), torch.zeros_like(s))
    tot = e.sum(3, keepdim=True)
    lse = torch.where(some, m + tot.clamp_min(1e-300).log(), torch.full_like(m, float('-inf')))
    P = torch.where(some, e / tot.clamp_min(1e-300), torch.zeros_like(e))
    qd = q_of(p)
    kp = torch.ones_like(ok) if not p else keep.cpu().bool()
    if mistake == 'no_rescale':
        Pt = torch.where(kp, P, torch.zeros_like(P))
    elif mistake == 'drop_before_norm':
        ek = torch.where(kp, e, torch.zeros_like(e))
        Pt = ek / ek.sum(3, keepdim=True).clamp_min(1e-300)
    else:
        Pt = torch.where(kp, P / qd, torch.zeros_like(P))
    out = (Pt @ v).transpose(1, 2).reshape(B, L, D)
    return dict(q=q, k=k, v=v, s=s, ok=ok, some=some, m=m, lse=lse.squeeze(3), P=P, Pt=Pt, keep=kp, qd=qd, out=out, scale=scale, H=H,
                dh=dh, L=L)


def heads(t, H):
    """[B, L, D] -> [B, H, L, dh]"""
    B, L, D = t.shape
    return t.reshape(B, L, H, D // H).transpose(1, 2)


def unheads(q, k, v):
    """three [B, H, L, dh] -> [B, L, 3 D]"""
    B, H, L, dh = q.shape
    return torch.cat([t.transpose(1, 2).reshape(B, L, H * dh) for t in (q, k, v)], dim=2)


def backward(f, g, mistake=None):
    """The float64 gradients from the forward ``f`` and g [B, L, D] -> dict(D, dPt, a, t, dS, dq, dk, dv, dqkv)."""
    g = heads(g.detach().cpu().to(F64), f['H'])
    q, k, v, P, Pt, keep, qd, scale = f['q'], f['k'], f['v'], f['P'], f['Pt'], f['keep'], f['qd'], f['scale']
    dPt = g @ v.transpose(2, 3)
    D = ((P if mistake == 'D_from_P' else Pt) * dPt).sum(3, keepdim=True)         # == sum_c g_ic out_ic
    a = torch.where(keep, dPt / qd, torch.zeros_like(dPt))
    t = a - D
    dS = P * t
    dq = scale * (dS @ k)
    dk = scale * ((dS if mistake == 'dk_untransposed' else dS.transpose(2, 3)) @ q)
    dv = Pt.transpose(2, 3) @ g
    return dict(g=g, D=D, dPt=dPt, a=a, t=t, dS=dS, dq=dq, dk=dk, dv=dv, dqkv=unheads(dq, dk, dv))


def softmax_allowance(s32, ok):
    """-> (allowance, measured): the worst relative error, in units of u, of torch's own fp32 softmax on the device of ``s32`` against
    the float64 softmax of the SAME fp32 scores (disallowed positions at -inf; rows without a key left out), and twice that."""
    ok = ok.to(s32.device)
    rows = ok.any(-1)
    x = s32.masked_fill(~ok, float('-inf'))[rows]
    got = torch.softmax(x, dim=-1).double().cpu()
    want = torch.softmax(x.double().cpu(), dim=-1)
    live = want > 2.0 ** -100
    worst = float(((got - want).abs()[live] / (U * want[live])).max()) if bool(live.any()) else 0.0
    return 2.0 * worst, worst


def forward_bounds(f, allow):
    """-> dict(e_s, rel_P, out [B, L, D], lse [B, H, L]) for ``f`` = forward(...); ``allow`` in units of u."""
    q, k, v, s, ok, L, dh = f['q'], f['k'], f['v'], f['s'], f['ok'], f['L'], f['dh']
    tiny = L * 2.0 ** -126
    e_s = (dh + 2) * U * f['scale'] * (q.abs() @ k.abs().transpose(2, 3)) + 2 * U * s.abs()
    e_max = torch.where(ok, e_s, torch.zeros_like(e_s)).amax(3, keepdim=True)
    rel_P = 2 * e_max + (L + 4 + allow) * U
    B, H = q.shape[:2]
    mag = (f['Pt'].abs() @ v.abs())
    tol_out = ((rel_P + (L + 2) * U) * mag).transpose(1, 2).reshape(B, L, H * dh) + tiny
    lse = f['lse'].unsqueeze(3)
    fin = torch.where(f['some'], lse, torch.zeros_like(lse))
    tol_lse = torch.where(f['some'], e_max + (L + 4 + allow) * U + U * (2 * (fin - f['m']).abs() + f['m'].abs() + fin.abs()),
                          torch.zeros_like(lse))
    return dict(e_s=e_s, rel_P=rel_P, out=tol_out, lse=tol_lse.squeeze(3), out_heads=heads(tol_out, H))


def backward_bounds(f, fb, b, allow):
    """-> the tolerance of dqkv [B, L, 3 D] for ``b`` = backward(f, g)."""
    q, k, v, s, P, Pt, keep, qd, scale, L, dh = (f[n] for n in ('q', 'k', 'v', 's', 'P', 'Pt', 'keep', 'qd', 'scale', 'L', 'dh'))
    g, t, dS = b['g'], b['t'], b['dS']
    tiny = L * 2.0 ** -126
    lse = f['lse'].unsqueeze(3)
    fin = torch.where(f['some'], lse, torch.zeros_like(lse))
    rel_Pb = fb['e_s'] + fb['lse'].unsqueeze(3) + 2 * U * (s - fin).abs() + allow * U
    out_h = heads(f['out'], f['H'])
    tol_D = (g.abs() * fb['out_heads']).sum(3, keepdim=True) + (dh + 2) * U * (g * out_h).abs().sum(3, keepdim=True)
    tol_dPt = (dh + 2) * U * (g.abs() @ v.abs().transpose(2, 3))
    tol_a = torch.where(keep, tol_dPt / qd + U * b['a'].abs(), torch.zeros_like(tol_dPt))
    tol_t = tol_a + tol_D + U * t.abs()
    tol_dS = P * tol_t + t.abs() * P * rel_Pb + U * dS.abs()
    tol_dq = scale * (tol_dS @ k.abs() + (L + 2) * U * (dS.abs() @ k.abs())) + U * b['dq'].abs()
    tol_dk = scale * (tol_dS.transpose(2, 3) @ q.abs() + (L + 2) * U * (dS.abs().transpose(2, 3) @ q.abs())) + U * b['dk'].abs()
    tol_dv = (Pt * (rel_Pb + U)).transpose(2, 3) @ g.abs() + (L + 2) * U * (Pt.transpose(2, 3) @ g.abs())
    return unheads(tol_dq, tol_dk, tol_dv) + tiny


def emulate_fp32(qkv, key_pad, causal, H, keep=None, p=0.0, g=None):
    """The kernel's sequence of operations in fp32 torch ops on the CPU -> (out, lse, dqkv or None, s32 [B, H, L, L]): scores,
    row maximum, exp, sum, P = e / sum, Pt = P / q, out; backward with P recomputed as exp(s - lse) from the fp32 lse."""
    qkv = qkv.detach().cpu().float()
    B, L, D3 = qkv.shape
    D = D3 // 3
    dh = D // H
    q, k, v = split(qkv, H)
    scale = torch.tensor(1.0 / math.sqrt(dh), dtype=torch.float32)
    ok = allowed(key_pad, causal, B, L).expand(B, H, L, L)
    some = ok.any(3, keepdim=True)
    s = (q @ k.transpose(2, 3)) * scale
    m = torch.where(some, s.masked_fill(~ok, float('-inf')).amax(3, keepdim=True), torch.zeros(()))
    e = torch.where(ok, (s - m).exp(), torch.zeros(()))
    tot = e.sum(3, keepdim=True)
    lse = torch.where(some, m + tot.clamp_min(1e-37).log(), torch.full_like(m, float('-inf')))
    P = torch.where(some, e / tot.clamp_min(1e-37), torch.zeros(()))
    qf = torch.tensor(q_of(p), dtype=torch.float32)
    kp = torch.ones_like(ok) if not p else keep.cpu().bool()
    Pt = torch.where(kp, P / qf, torch.zeros(())) if p else P
    out_h = Pt @ v
    out = out_h.transpose(1, 2).reshape(B, L, D)
    if g is None:
        return out, lse.squeeze(3), None, s
    gh = heads(g.detach().cpu().float(), H)
    Pb = torch.where(ok, (s - torch.where(some, lse, torch.zeros(()))).exp(), torch.zeros(()))
    Dv = (gh * out_h).sum(3, keepdim=True)
    dPt = gh @ v.transpose(2, 3)
    a = torch.where(kp, dPt / qf, torch.zeros(())) if p else dPt
    dS = Pb * (a - Dv)
    Ptb = torch.where(kp, Pb / qf, torch.zeros(())) if p else Pb
    dq, dk, dv = (dS @ k) * scale, (dS.transpose(2, 3) @ q) * scale, Ptb.transpose(2, 3) @ gh
    return out, lse.squeeze(3), unheads(dq, dk, dv), s


def worst_ratio(got, want, tol):
    """max |got - want| / tol."""
    return float(((got.detach().cpu().to(F64) - want).abs() / tol).max())


def pad_suffix(seqlen, L):
    """bool [B, L]: the right-padded suffix of sequences of the given lengths."""
    return torch.arange(L).view(1, L) >= torch.as_tensor(seqlen).view(-1, 1)
