"""Float64 referee of NGCF's BiCombiner layer and of the NGCF propagation, with the error bounds the fp32 kernels are held to.
Test code only: it calls nothing of recstudio_amd.

WHAT IT IS PINNED TO.  dgl is not installed where this project is built, so nothing of the reference's NGCF can be run and
recorded.  The referee follows the rule the reference's source spells out --
  recstudio/model/module/graphmodule.py:70-86   BiCombiner: act(linear_sum(x + m)) + act(linear_product(x * m)), then dropout
  recstudio/model/module/graphmodule.py:201-229 the layer loop: m = GraphConv(norm)(x), x <- combiner(x, m), the list of
                                                normalize(x) with the input first
  recstudio/model/graph/ngcf.py:63-86           act = LeakyReLU(), normalize = 2, mess_norm = 'left', cat over the list
-- plus dgl's documented norm = 'left' ("divide the outgoing messages of a node by its out-degree", a degree of 0 counted as 1):
  m[dst] = sum over the kept edges src -> dst of x[src] / max(out_deg_kept(src), 1).
The dropout is NOT nn.Dropout's stream: with q = fp32(1 - p) element (r, c) is kept iff u[r, c] < q, u = torch.rand, and the kept
element is divided by q (a stated deviation of the fused layer).

THE BOUNDS (u = 2**-24, no FMA contraction assumed, first order in u: the dropped products of two error terms are below N u < 1e-3
of the bound at the sizes used).  No constant below is fitted; g(n) = n u / (1 - n u).
  pre-activation   pre_j = sum_k a_k W_jk + b_j, a = x + m or x * m rounded once, the d_in products rounded once each, the sum in
                   ANY order (d_in - 1 additions on the longest path, or fewer), the bias added last:
                       tol_pre = g(d_in + 3) (sum_k |a_k| |W_jk| + |b_j|)
  activation       LeakyReLU is 1-Lipschitz (|slope| <= 1) and its product with the slope is rounded once:  tol_act = tol_pre + u |act|
  h                v = s + p rounded once, h = v / q rounded once; a dropped element is exactly 0:
                       tol_h = (tol_s + tol_p) / q + 2 u |h|
  n = h / c        c = max(||h||, 1e-12).  The squares are rounded once each and added along a path of at most d_out / 2 + 1
                   additions, the root is rounded once: |dc| <= ||tol_h||_2 + g(d_out / 2 + 3) c;  the quotient is rounded once:
                       tol_n = tol_h / c + |n| ||tol_h||_2 / c + g(d_out / 2 + 3) |n|
  backward         every quantity of   t = (sum_c h g_n) / c,  dh = g_h + (g_n - (h / c) t) / c,  dsum = keep ? dh / q : 0,
                   ds = dsum * slope(s),  da = ds W1,  dx = da + db * m,  dW1 = ds^T (x + m),  db1 = sum_r ds   carries the
                   tolerance of its operands through the same first-order rules (a product a b: |a| tol_b + |b| tol_a + u |a b|;
                   a quotient a / c: tol_a / c + |a / c| tol_c / c + u |a / c|; an n-term sum in any order: the sum of the terms'
                   tolerances + g(n) sum |terms|): `layer_backward_bounds` spells each step out.  A sum over the N rows therefore
                   gets g(N + 3) sum |terms|.
The slope of LeakyReLU jumps at 0: a backward is only decidable where no float64 pre-activation lies within its own forward
tolerance of 0 -- `preact_margin` returns min |pre| / tol_pre, and every backward test first asserts that it is at least 2 (a
condition on the INPUTS, checked on the referee).  The forward has no such ambiguity, and keep / drop compares bit-equal uniforms.
"""
import torch

U = 2.0 ** -24
EPS = 1e-12
F64 = torch.float64


def g(n):
    return n * U / (1.0 - n * U)


def q_of(p):
    """fp32(1 - p) as a python float; 1.0 for p == 0."""
    return float(torch.tensor(1.0 - float(p), dtype=torch.float32)) if p else 1.0


def leaky(v, slope):
    return torch.where(v > 0, v, v * slope)


def slope_of(pre, slope):
    """LeakyReLU's derivative at ``pre``, in the dtype of ``pre``."""
    return torch.where(pre > 0, torch.ones_like(pre), torch.full_like(pre, slope))


def layer_forward(x, m, w1, b1, w2, b2, slope=0.01, p=0.0, u=None):
    """Everything of one layer in float64 -> dict(pre_s, pre_p, s, p, keep, q, h, c, n).  ``u``: the uniforms (fp32 or float64
    holding fp32 values) when p != 0."""
    x, m, w1, b1, w2, b2 = (t.to(F64) for t in (x, m, w1, b1, w2, b2))
    pre_s = (x + m) @ w1.T + b1
    pre_p = (x * m) @ w2.T + b2
    s, pp = leaky(pre_s, slope), leaky(pre_p, slope)
    q = q_of(p)
    keep = torch.ones_like(s, dtype=torch.bool) if not p else (u.to(F64) < q)
    h = torch.where(keep, (s + pp) / q, torch.zeros_like(s))
    c = h.norm(dim=1, keepdim=True).clamp_min(EPS)
    return dict(pre_s=pre_s, pre_p=pre_p, s=s, p=pp, keep=keep, q=q, h=h, c=c, n=h / c)


def layer_forward_bounds(x, m, w1, b1, w2, b2, f):
    """-> dict(pre_s, pre_p, h, n): the tolerances of the header for the forward ``f`` = layer_forward(...)."""
    x, m, w1, b1, w2, b2 = (t.to(F64) for t in (x, m, w1, b1, w2, b2))
    d_in, d_out = w1.shape[1], w1.shape[0]
    tol_pre_s = g(d_in + 3) * ((x + m).abs() @ w1.abs().T + b1.abs())
    tol_pre_p = g(d_in + 3) * ((x * m).abs() @ w2.abs().T + b2.abs())
    tol_s, tol_p = tol_pre_s + U * f['s'].abs(), tol_pre_p + U * f['p'].abs()
    tol_h = torch.where(f['keep'], (tol_s + tol_p) / f['q'] + 2 * U * f['h'].abs(), torch.zeros_like(tol_s))
    th2 = tol_h.norm(dim=1, keepdim=True)
    tol_c = th2 + g(d_out / 2 + 3) * f['c']
    tol_n = tol_h / f['c'] + f['n'].abs() * th2 / f['c'] + g(d_out / 2 + 3) * f['n'].abs()
    return dict(pre_s=tol_pre_s, pre_p=tol_pre_p, h=tol_h, c=tol_c, n=tol_n)


def preact_margin(f, fb):
    """min over both pre-activations of |pre| / tol_pre: the backward is decidable when this is at least 2."""
    return float(torch.minimum((f['pre_s'].abs() / fb['pre_s']).min(), (f['pre_p'].abs() / fb['pre_p']).min()))


def layer_backward(x, m, w1, b1, w2, b2, f, g_h=None, g_n=None, slope=0.01):
    """The float64 gradients of one layer from its forward ``f`` -> dict(t, dh, ds, dp, da, db, dx, dm, dw1, dw2, db1, db2)."""
    x, m, w1, w2 = (t.to(F64) for t in (x, m, w1, w2))
    zero = torch.zeros_like(f['h'])
    g_h = zero if g_h is None else g_h.to(F64)
    g_n = zero if g_n is None else g_n.to(F64)
    c = f['c']
    active = f['h'].norm(dim=1, keepdim=True) >= EPS               # clamp_min passes its gradient only at or above the bound
    t = torch.where(active, (f['h'] * g_n).sum(1, keepdim=True) / c, torch.zeros_like(c))
    dh = g_h + (g_n - (f['h'] / c) * t) / c
    dsum = torch.where(f['keep'], dh / f['q'], zero)
    ds = dsum * slope_of(f['pre_s'], slope)
    dp = dsum * slope_of(f['pre_p'], slope)
    da, db = ds @ w1, dp @ w2
    return dict(t=t, dh=dh, dsum=dsum, ds=ds, dp=dp, da=da, db=db, dx=da + db * m, dm=da + db * x,
                dw1=ds.T @ (x + m), dw2=dp.T @ (x * m), db1=ds.sum(0), db2=dp.sum(0))


def layer_backward_bounds(x, m, w1, b1, w2, b2, f, fb, b, g_h=None, g_n=None, slope=0.01):
    """-> dict(dx, dm, dw1, dw2, db1, db2): the tolerances of the gradients ``b`` = layer_backward(...), step by step."""
    x, m, w1, w2 = (t.to(F64) for t in (x, m, w1, w2))
    N, d_in, d_out = x.shape[0], w1.shape[1], w1.shape[0]
    zero = torch.zeros_like(f['h'])
    g_n = zero if g_n is None else g_n.to(F64)
    h, c, q, t = f['h'], f['c'], f['q'], b['t']
    tol_h, tol_c = fb['h'], fb['c']
    hg = h * g_n
    tol_dot = (tol_h * g_n.abs()).sum(1, keepdim=True) + g(d_out / 2 + 3) * hg.abs().sum(1, keepdim=True)
    tol_t = tol_dot / c + t.abs() * tol_c / c + U * t.abs()
    hn = h / c
    tol_hn = tol_h / c + hn.abs() * tol_c / c + U * hn.abs()
    w = hn * t
    tol_w = tol_hn * t.abs() + hn.abs() * tol_t + U * w.abs()
    e = g_n - w
    tol_e = tol_w + U * e.abs()
    fq = e / c
    tol_f = tol_e / c + fq.abs() * tol_c / c + U * fq.abs()
    tol_dh = tol_f + U * b['dh'].abs()
    tol_dsum = torch.where(f['keep'], tol_dh / q + U * b['dsum'].abs(), zero)
    sl_s, sl_p = slope_of(f['pre_s'], abs(slope)), slope_of(f['pre_p'], abs(slope))
    tol_ds, tol_dp = tol_dsum * sl_s + U * b['ds'].abs(), tol_dsum * sl_p + U * b['dp'].abs()
    tol_da = tol_ds @ w1.abs() + g(d_out + 2) * (b['ds'].abs() @ w1.abs())
    tol_db = tol_dp @ w2.abs() + g(d_out + 2) * (b['dp'].abs() @ w2.abs())
    tol_dx = tol_da + m.abs() * tol_db + 2 * U * (b['da'].abs() + (b['db'] * m).abs())
    tol_dm = tol_da + x.abs() * tol_db + 2 * U * (b['da'].abs() + (b['db'] * x).abs())
    a1, a2 = (x + m).abs(), (x * m).abs()
    tol_dw1 = tol_ds.T @ a1 + (U + g(N + 3)) * (b['ds'].abs().T @ a1)
    tol_dw2 = tol_dp.T @ a2 + (U + g(N + 3)) * (b['dp'].abs().T @ a2)
    tol_db1 = tol_ds.sum(0) + g(N + 2) * b['ds'].abs().sum(0)
    tol_db2 = tol_dp.sum(0) + g(N + 2) * b['dp'].abs().sum(0)
    return dict(dx=tol_dx, dm=tol_dm, dw1=tol_dw1, dw2=tol_dw2, db1=tol_db1, db2=tol_db2)


def layer_fp32(x, m, w1, b1, w2, b2, slope=0.01, p=0.0, u=None, g_h=None, g_n=None):
    """The kernel's arithmetic step by step in fp32 torch ops on the CPU (the library's own summation orders inside the two
    products and the sums; every other operation rounded where the kernel rounds it) -> the forward and backward quantities."""
    f32 = torch.float32
    x, m, w1, b1, w2, b2 = (t.to(f32) for t in (x, m, w1, b1, w2, b2))
    sl = torch.tensor(slope, dtype=f32)
    pre_s, pre_p = (x + m) @ w1.T + b1, (x * m) @ w2.T + b2
    h = torch.where(pre_s > 0, pre_s, pre_s * sl) + torch.where(pre_p > 0, pre_p, pre_p * sl)
    q = torch.tensor(q_of(p), dtype=f32)
    keep = torch.ones_like(h, dtype=torch.bool) if not p else (u.to(f32) < q)
    if p:
        h = torch.where(keep, h / q, torch.zeros_like(h))
    ss = (h * h).sum(1, keepdim=True)
    nrm = ss.sqrt()
    c = nrm.clamp_min(EPS)
    out = dict(h=h, n=h / c)
    if g_h is None and g_n is None:
        return out
    zero = torch.zeros_like(h)
    g_h = zero if g_h is None else g_h.to(f32)
    g_n = zero if g_n is None else g_n.to(f32)
    t = torch.where(nrm >= EPS, (h * g_n).sum(1, keepdim=True) / c, torch.zeros_like(c))
    dsum = g_h + (g_n - (h / c) * t) / c
    if p:
        dsum = torch.where(keep, dsum / q, zero)
    ds = dsum * torch.where(pre_s > 0, torch.ones_like(sl), sl)
    dp = dsum * torch.where(pre_p > 0, torch.ones_like(sl), sl)
    da, db = ds @ w1, dp @ w2
    out.update(dx=da + db * m, dm=da + db * x, dw1=ds.T @ (x + m), dw2=dp.T @ (x * m), db1=ds.sum(0), db2=dp.sum(0))
    return out


def worst(got, want, tol):
    """max |got - want| / tol over the elements (0 / 0 counts as 0; a non-finite value as inf)."""
    got, want, tol = got.detach().cpu().to(F64), want.detach().cpu().to(F64), tol.detach().cpu().to(F64)
    if not bool(torch.isfinite(got).all()):
        return float('inf')
    err = (got - want).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / tol)
    return float(ratio.max()) if ratio.numel() else 0.0


def layer_inputs(N, d_in, d_out, seed, p=0.0, slope=0.01, margin=3.0):
    """Inputs of one layer, on the CPU: x, m in [-1, 1), weights of nn.Linear's scale, biases of +-0.1, the uniforms of the
    dropout and two gradients.  Rows with a float64 pre-activation closer to 0 than ``margin`` times its tolerance are drawn again
    (a few of some ten thousand), so that `preact_margin` of the result is at least ``margin``: the LeakyReLU slope of every
    element is then decided.  -> dict(x, m, w1, b1, w2, b2, u, g_h, g_n)."""
    gen = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.rand(*s, generator=gen) * 2 - 1      # noqa: E731
    x, m = r(N, d_in), r(N, d_in)
    k = d_in ** -0.5
    w1, w2, b1, b2 = r(d_out, d_in) * k, r(d_out, d_in) * k, r(d_out) * 0.1, r(d_out) * 0.1
    for _ in range(50):
        f = layer_forward(x, m, w1, b1, w2, b2, slope)
        fb = layer_forward_bounds(x, m, w1, b1, w2, b2, f)
        bad = ((f['pre_s'].abs() < margin * fb['pre_s']) | (f['pre_p'].abs() < margin * fb['pre_p'])).any(1)
        if not bool(bad.any()):
            break
        n_bad = int(bad.sum())
        x[bad], m[bad] = r(n_bad, d_in), r(n_bad, d_in)
    u = torch.rand(N, d_out, generator=gen)
    return dict(x=x, m=m, w1=w1, b1=b1, w2=w2, b2=b2, u=u, g_h=torch.randn(N, d_out, generator=gen),
                g_n=torch.randn(N, d_out, generator=gen))


# ---------------------------------------------------------------------------------------------------------------- the net
def left_adjacency(dst, src, n, keep=None, norm='left', degrees_of=None, zero_degree_as_one=True):
    """Dense float64 [n, n] matrix A with m = A x the aggregation over the edges src -> dst that ``keep`` (bool per edge) leaves.
    'left': every edge weighs 1 / max(out_deg_kept(src), 1); 'both': out_deg^-1/2 in_deg^-1/2 (the LightGCN rule, for the seeded
    mistake).  ``degrees_of``: a keep mask to count the degrees on instead (the seeded mistake 'the base graph's degrees').
    ``zero_degree_as_one=False`` (the seeded mistake): the per-edge values in the form keep[e] / out_deg[src], unclamped."""
    dst, src = dst.long(), src.long()
    keep = torch.ones_like(dst, dtype=torch.bool) if keep is None else keep.bool()
    count = keep if degrees_of is None else degrees_of.bool()
    out_deg = torch.zeros(n, dtype=F64).index_add_(0, src[count], torch.ones(int(count.sum()), dtype=F64))
    in_deg = torch.zeros(n, dtype=F64).index_add_(0, dst[count], torch.ones(int(count.sum()), dtype=F64))
    if zero_degree_as_one:
        out_deg, in_deg = out_deg.clamp_min(1.0), in_deg.clamp_min(1.0)
    w = 1.0 / out_deg[src] if norm == 'left' else out_deg[src].pow(-0.5) * in_deg[dst].pow(-0.5)
    A = torch.zeros(n, n, dtype=F64)
    if zero_degree_as_one:
        A.index_put_((dst[keep], src[keep]), w[keep], accumulate=True)
    else:       # the form a kernel computes, values[e] = keep[e] * inv_out[src]: a source that lost every edge gives 0 * inf
        A.index_put_((dst, src), keep.to(F64) * w, accumulate=True)
    return A


def net_forward(A, x0, layers, slope=0.01, ps=None, us=None, feed_normalised=False, with_input=True):
    """The float64 NGCF table cat(x_0, n_1, ..., n_L) over the dense aggregation matrix ``A`` (autograd-capable: ``x0`` and the
    layer parameters may require grad).  ``layers``: [(w1, b1, w2, b2)]; ``ps`` / ``us``: dropout probability and uniforms per
    layer.  ``feed_normalised`` / ``with_input=False``: seeded mistakes."""
    x = x0
    blocks = [x0] if with_input else []
    for k, (w1, b1, w2, b2) in enumerate(layers):
        m = A @ x
        pre_s, pre_p = (x + m) @ w1.T + b1, (x * m) @ w2.T + b2
        h = leaky(pre_s, slope) + leaky(pre_p, slope)
        p = ps[k] if ps is not None else 0.0
        if p:
            q = q_of(p)
            h = torch.where(us[k].to(F64) < q, h / q, torch.zeros_like(h))
        nk = h / h.norm(dim=1, keepdim=True).clamp_min(EPS)
        blocks.append(nk)
        x = nk if feed_normalised else h
    return torch.cat(blocks, dim=1)


def ngcf_step(user_emb, item_emb, A, layers, uid, pos, neg, l2_reg_weight, slope=0.01, ps=None, us=None):
    """One NGCF training step in dense float64 torch on given masks, uniforms and ids (ngcf.py:77-86): the table over ``A``, BPR
    on its rows (loss_func.py:55-59: -mean over the batch of the average logsigmoid(pos - neg) over the negatives) plus
    l2_reg_weight * l2_reg of the BASE rows of the batch's users, positives and negatives (loss_func.py:189-193: the sum over the
    three of mean_b ||row_b||^2).  -> dict(loss, user_grad, item_grad, layer_grads [(dw1, db1, dw2, db2)], table)."""
    dev = A.device
    ue = user_emb.detach().to(dev, F64).clone().requires_grad_(True)
    ie = item_emb.detach().to(dev, F64).clone().requires_grad_(True)
    params = [tuple(t.detach().to(dev, F64).clone().requires_grad_(True) for t in layer) for layer in layers]
    table = net_forward(A, torch.cat([ue, ie], 0), params, slope, ps, us)
    users, items = table[:ue.shape[0]], table[ue.shape[0]:]
    q = users[uid]
    pos_score = (q * items[pos]).sum(-1)
    neg_score = (q.unsqueeze(1) * items[neg]).sum(-1)
    bpr = -torch.mean(torch.nn.functional.logsigmoid(pos_score.view(-1, 1) - neg_score).mean(-1))
    reg = sum(torch.mean(torch.sum(e * e, dim=-1)) for e in (ue[uid], ie[pos], ie[neg.reshape(-1)]))
    loss = bpr + l2_reg_weight * reg
    loss.backward()
    return dict(loss=loss.detach(), user_grad=ue.grad, item_grad=ie.grad, layer_grads=[tuple(t.grad for t in layer) for layer in params],
                table=table.detach())
