"""Float64 referee of exact softmax sampling over the whole catalog (rsa_softmax_sample / rsa_softmax_lookup, ops.softmax_sample,
``sampling(method='brute')`` with ``train.brute_stream``), the bounds a correct fp32 implementation stays inside, and an fp32
emulation of the three steps with seeded mistakes.  Test code only: nothing here calls recstudio_amd.

Semantics (recstudio/model/basemodel/baseretriever.py:299-328).  Item ids run 1 .. N - 1 (row 0 of the table is the padding row):

    s_i      = score(q, x_i) / t       inner product, cosine (dot / (|q| |x|)) or Euclidean (2 dot - |x|^2 - |q|^2), scorer.py:5-34
    lse      = log sum_i exp(s_i)      over ALL items, history included (the reference's softmax comes before the mask)
    w_i      = exp(s_i - lse)          0 for the ids of the user's history, for id 0 and for ids >= N
    draw     P(id) = w_id / sum w      (torch.multinomial normalises the masked row)
    log-prob s_id - lse                the log of the masked, NOT renormalised row;  -inf for a given id that is 0

The sampler under test draws by a two-level inverse CDF with two uniforms: blocks of G consecutive ids (block g = ids 1 + g G ..),
mass_g = sum of w over the block, F(g) = (mass_0 + .. + mass_g) / sum w;  u1 picks the first block with F(g) > u1, u2 the first item
of it whose in-block CDF f(i) = (w_first + .. + w_i) / mass_g exceeds u2.  A draw (id, u1, u2) is therefore judged by

    w64[id] > 0                                        exact: an item of weight 0 is never returned
    F64(g - 1) - tol1 <= u1 <= F64(g) + tol1           g the block of id
    f64(id - 1) - tol2 <= u2 <= f64(id) + tol2         (f64 = 0 in front of the block's first item)
    |logp - (s64_id - lse64)| <= tol_lp

BOUNDS, with u = 2^-24, d the embedding width, A_i = sum_k |q_k x_ik|.

Score.  An fp32 dot product of d terms, in any order, fused or not, is within d u A_i of the exact one (the standard gamma_d bound
at first order).  Inner product: one more rounding for the product with 1 / t and one for fl(1 / t) itself:
    eps_i = (d + 2) u A_i / t.
Cosine, s = dot * fl(1 / |x|) * fl(1 / |q|) / t: each inverse norm carries the (d + 1) u of its sum of squares halved by the square
root, plus the square root and the division (2 u each when correctly rounded; 4 u allowed); two products and the two roundings
of 1 / t:  eps_i = (d A_i / (|q| |x|) + (d + 13) |cos_i|) u / t.
Euclidean, s = (fl(2 dot - fl|x|^2) - fl|q|^2) / t: the dot's error doubled, (d + 1) u on each squared norm, one rounding for each
of the two subtractions (their results are at most 2 A + |x|^2 + |q|^2 in size) and the two of 1 / t:
    eps_i = (2 d A_i + (d + 1) (|x|^2 + |q|^2) + 2 (2 A_i + |x|^2 + |q|^2) + 2 |t s_i|) u / t.

exp.  The hardware exponential is 2^(x log2 e): the product rounds the ARGUMENT, u |x| in x, the subtraction that formed x another
u |x|, and the instruction itself is good to 1 ulp = 2 u; a term below e^-104 is 0 in fp32, so |x| <= 104 for every term that
counts:  rel_exp = (2 * 104 + 2) u.

Sums.  An fp32 sum of n non-negative terms, in any order, is within (n + 2) u of the exact one, relatively (n - 1 additions and
room for a scaling product): (G + 2) u for a block, (n_blocks + 2) u for the sum over the blocks and for the running sum.

lse.  Every term of the sum carries at most max_i eps_i + rel_exp relatively, the two levels of summation (G + n_blocks + 4) u, and
the log and the addition of the maximum 2 u |lse|:
    eps_lse = max_i eps_i + rel_exp + (G + n_blocks + 4) u + 2 u |lse64|.
Log-probability: the score, the lse, and the subtraction's rounding:  tol_lp = eps_id + eps_lse + u (|s64_id| + |lse64|).

Block CDF.  mass_g = s_g exp(m_g - lse): the terms' max_i eps_i + rel_exp, eps_lse through the exponent, the block sum (G + 2) u and the
product u -- rho_m; the running sum adds (n_blocks + 2) u.  F = C_g / C_last is a ratio of two such values, at most 1:
    tol1 = 2 (rho_m + (n_blocks + 2) u) + 2 u           (the last 2 u: the fp32 product u1 * C_last and the table's own rounding)
In-block CDF.  Weights relative to one another inside a block: 2 max_i eps_i + rel_exp (the block's common factor cancels), the
block sum (G + 2) u, a ratio again:
    tol2 = 2 (2 max_i eps_i + rel_exp + (G + 2) u) + 2 u
max_i runs over the whole row in both: simpler than per block, never smaller.

Own tables.  Given the sampler's OWN fp32 running sums cum[b] the block is exact: searchsorted(cum[b], fl32(u1 * cum[b, -1]),
right=True); where rounding leaves no entry above the threshold (u1 next to 1), the first entry equal to cum[b, -1].
"""
import torch

U32 = 2.0 ** -24
REL_EXP = (2 * 104 + 2) * U32
IP, COS, EUC = 0, 1, 2


def scores64(W, Q, t, mode):
    """(s [M, N - 1] float64 for ids 1 .. N - 1, eps [M, N - 1] the bound on an fp32 score) on the device of W."""
    X, q = W[1:].double(), Q.double().to(W.device)
    d = W.shape[1]
    dot, A = q @ X.t(), q.abs() @ X.abs().t()
    if mode == IP:
        return dot / t, (d + 2) * U32 * A / t
    if mode == COS:
        den = q.norm(dim=1, keepdim=True) * X.norm(dim=1)
        c = dot / den
        return c / t, (d * A / den + (d + 13) * c.abs()) * U32 / t
    x2, q2 = (X * X).sum(1), (q * q).sum(1, keepdim=True)
    s = (2 * dot - x2 - q2) / t
    return s, (2 * d * A + (d + 1) * (x2 + q2) + 2 * (2 * A + x2 + q2) + 2 * (s * t).abs()) * U32 / t


def tables64(W, Q, t, mode, G, hist=None):
    """Everything the judges need, in float64: dict(s, eps [M, N - 1]; lse, eps_lse [M]; w [M, N] by id (0 at id 0 and over the
    history); F [M, nb] the block CDF, fin [M, N] the in-block CDF by id, tol1, tol2 [M], G, N)."""
    s, eps = scores64(W, Q, t, mode)
    M, n = s.shape
    N, nb = n + 1, (n + G - 1) // G
    lse = torch.logsumexp(s, dim=1)
    eps_max = eps.max(dim=1).values
    eps_lse = eps_max + REL_EXP + (G + nb + 4) * U32 + 2 * U32 * lse.abs()
    w = torch.cat([s.new_zeros(M, 1), torch.exp(s - lse.view(-1, 1))], dim=1)
    if hist is not None:
        h = hist.to(w.device).long()
        w.scatter_(1, torch.where((h >= 1) & (h < N), h, torch.zeros_like(h)), 0.0)      # (ids outside the table: column 0, already 0)
    wp = torch.cat([w[:, 1:], w.new_zeros(M, nb * G - n)], dim=1).view(M, nb, G)
    mass = wp.sum(2)
    total = mass.sum(1, keepdim=True)
    F = mass.cumsum(1) / total.clamp_min(1e-300)
    safe = torch.where(mass > 0, mass, torch.ones_like(mass)).unsqueeze(2)
    fin = torch.cat([w.new_zeros(M, 1), (wp.cumsum(2) / safe).reshape(M, nb * G)[:, :n]], dim=1)
    rho_m = eps_max + REL_EXP + eps_lse + (G + 3) * U32
    return dict(s=s, eps=eps, lse=lse, eps_lse=eps_lse, w=w, mass=mass, total=total.view(-1), F=F.clamp(0, 1), fin=fin.clamp(0, 1),
                tol1=2 * (rho_m + (nb + 2) * U32) + 2 * U32, tol2=2 * (2 * eps_max + REL_EXP + (G + 2) * U32) + 2 * U32,
                G=G, N=N, nb=nb)


def judge_draws(T, ids, u, logp, scale=1.0):
    """Every draw ids [M, n] (uniforms u [M, n, 2], log-probabilities logp [M, n]) -> dict of violation COUNTS (all must be 0) and the
    worst excess over each interval in units of its tolerance.  ``scale`` shrinks every tolerance (the emulation must stay
    inside half of them)."""
    dev = T['w'].device
    ids, u, logp = ids.to(dev).long(), u.to(dev).double(), logp.to(dev).double()
    N, G = T['N'], T['G']
    inside = (ids >= 1) & (ids < N)
    idc = ids.clamp(1, N - 1)
    res = dict(outside=int((~inside).sum()), zero_weight=int((T['w'].gather(1, idc) <= 0)[inside].sum()))
    g = (idc - 1) // G
    Fp = torch.cat([T['F'].new_zeros(T['F'].shape[0], 1), T['F']], dim=1)
    lo, hi = Fp.gather(1, g), Fp.gather(1, g + 1)
    tol1 = (T['tol1'] * scale).view(-1, 1)
    ex1 = torch.maximum(lo - u[..., 0], u[..., 0] - hi).clamp_min(0) / tol1
    res['block'], res['block_ratio'] = int((ex1 > 1).sum()), float(ex1.max()) if ex1.numel() else 0.0
    first = (idc - 1) % G == 0
    f_lo = torch.where(first, torch.zeros_like(lo), T['fin'].gather(1, idc - 1))
    f_hi = T['fin'].gather(1, idc)
    tol2 = (T['tol2'] * scale).view(-1, 1)
    ex2 = torch.maximum(f_lo - u[..., 1], u[..., 1] - f_hi).clamp_min(0) / tol2
    res['item'], res['item_ratio'] = int((ex2 > 1).sum()), float(ex2.max()) if ex2.numel() else 0.0
    res['logp'], res['logp_ratio'] = judge_logp(T, ids, logp, scale)
    return res


def judge_logp(T, ids, logp, scale=1.0):
    """Log-probabilities of ids [M, T] (0 = the padding id: exactly -inf) against s64 - lse64 -> (count, worst ratio)."""
    dev = T['w'].device
    ids, logp = ids.to(dev).long(), logp.to(dev).double()
    idc = ids.clamp(1, T['N'] - 1)
    s, eps = T['s'].gather(1, idc - 1), T['eps'].gather(1, idc - 1)
    lse, eps_lse = T['lse'].view(-1, 1), T['eps_lse'].view(-1, 1)
    tol = (eps + eps_lse + U32 * (s.abs() + lse.abs())) * scale
    ex = (logp - (s - lse)).abs() / tol
    ex = torch.where(ids == 0, torch.where(logp == float('-inf'), 0.0, float('inf')).double(), ex)
    ex = torch.where(torch.isnan(ex), torch.full_like(ex, float('inf')), ex)
    return int((ex > 1).sum()), float(ex.max()) if ex.numel() else 0.0


def judge_lse(T, lse, scale=1.0):
    ex = (lse.to(T['lse'].device).double() - T['lse']).abs() / (T['eps_lse'] * scale)
    return int((ex > 1).sum()), float(ex.max())


def own_block(cum, u1):
    """The exact block of every draw given the sampler's own fp32 running sums cum [M, nb]: see "Own tables"."""
    cum = cum.float().contiguous()
    last = cum[:, -1:]
    thr = (u1.to(cum.device).float() * last).contiguous()                  # ONE fp32 product
    blk = torch.searchsorted(cum, thr, right=True)
    first_full = torch.searchsorted(cum, last.expand_as(thr).contiguous(), right=False)
    return torch.where(blk >= cum.shape[1], first_full, blk)


def edge_uniforms(T, n, generator):
    """u [M, n, 2] on the device of the tables: about half the slots sit at the fp32 neighbours below / at / above values of the
    block CDF (slot 0) and of the in-block CDF (slot 1), at 0 and at 1 - 2^-24; the rest are uniform."""
    dev = T['w'].device
    M = T['F'].shape[0]
    top = 1.0 - 2.0 ** -24
    u = torch.rand(M, n, 2, generator=generator).to(dev)
    for slot, cdf in ((0, T['F']), (1, T['fin'][:, 1:])):
        c = cdf.float()
        zero, two = torch.zeros_like(c), torch.full_like(c, 2.0)
        edges = torch.cat([c, torch.nextafter(c, zero), torch.nextafter(c, two), c.new_zeros(M, 1), c.new_full((M, 1), top)], dim=1)
        pick = torch.randint(0, edges.shape[1], (M, n), generator=generator).to(dev)
        use = (torch.rand(M, n, generator=generator) < 0.5).to(dev)
        u[..., slot] = torch.where(use, edges.gather(1, pick).clamp(0.0, top), u[..., slot])
    return u.contiguous()


# ------------------------------------------------------------------------------------------------- fp32 emulation
MISTAKES = ('zero_based', 'hist_ignored_in_block', 'ph_subtracted_per_duplicate', 'temperature_on_lse_only', 'last_block_full',
            'u1_reused', 'total_one', 'ip_lse_with_cosine')


def _scores32(W, Q, t, mode):
    X, q = W.float(), Q.float()
    dot = q @ X.t()
    if mode == COS:
        dot = dot * (1.0 / X.norm(dim=1)) * (1.0 / q.norm(dim=1, keepdim=True))
    elif mode == EUC:
        dot = 2 * dot - (X * X).sum(1) - (q * q).sum(1, keepdim=True)
    return dot * torch.tensor(1.0 / t, dtype=torch.float32)


def emulate(W, Q, t, mode, G, u, hist=None, pos=None, mistake=None):
    """fp32 emulation (CPU torch) of the three steps -> (ids [M, n], logp [M, n] fp32, pos_logp or None, lse [M]).  ``mistake``:
      zero_based                   the catalog is rows 0 .. N - 2 and the row index is returned
      hist_ignored_in_block        the block masses leave the history out, the in-block scan does not
      ph_subtracted_per_duplicate  a touched block's mass = its full mass minus p_h once per history SLOT
      temperature_on_lse_only      lse from s / t, weights and log-probabilities from s
      last_block_full              the last block sums G rows (the rows past the table read as the last row)
      u1_reused                    u2 = u1
      total_one                    u1 is searched against 1 instead of the masked total
      ip_lse_with_cosine           lse from the inner products, everything else from the scores of the mode"""
    W, Q, u = W.float().cpu(), Q.float().cpu(), u.float().cpu()
    M, N = Q.shape[0], W.shape[0]
    rows = W[:-1] if mistake == 'zero_based' else W[1:]
    s = _scores32(rows, Q, t, mode)                                   # [M, n], column c = id c + 1
    n_cols = s.shape[1]
    nb = (n_cols + G - 1) // G
    s_lse = s
    if mistake == 'ip_lse_with_cosine':
        s_lse = _scores32(rows, Q, t, IP)
    s_w = _scores32(rows, Q, 1.0, mode) if mistake == 'temperature_on_lse_only' else s
    lse = torch.logsumexp(s_lse, dim=1)
    w = torch.exp(s_w - lse.view(-1, 1))
    full = w.clone()
    masked = torch.zeros_like(w, dtype=torch.bool)
    if hist is not None:
        h = hist.cpu().long()
        valid = (h >= 1) & (h < N)
        col = (h - 1).clamp(0, n_cols - 1)
        masked = torch.zeros(w.shape, dtype=torch.int32).scatter_add_(1, col, valid.int()) > 0
        w = torch.where(masked, torch.zeros_like(w), w)
    pad = nb * G - n_cols
    fill = (lambda x: torch.cat([x, x[:, -1:].expand(-1, pad)], dim=1)) if mistake == 'last_block_full' else \
        (lambda x: torch.cat([x, x.new_zeros(M, pad)], dim=1))
    mass = fill(w).view(M, nb, G).sum(2)
    if mistake == 'ph_subtracted_per_duplicate' and hist is not None:
        mass = fill(full).view(M, nb, G).sum(2)
        ph = torch.where(valid, full.gather(1, col), torch.zeros_like(col, dtype=torch.float32))
        mass = (mass - torch.zeros_like(mass).scatter_add_(1, col // G, ph)).clamp_min(0)
    cum = mass.cumsum(1)
    u1 = u[..., 0]
    u2 = u1 if mistake == 'u1_reused' else u[..., 1]
    if mistake == 'total_one':
        blk = torch.searchsorted(cum.contiguous(), u1.contiguous(), right=True).clamp_max(nb - 1)
    else:
        blk = own_block(cum, u1)
    w_in = fill(full if mistake == 'hist_ignored_in_block' else w).view(M, nb, G)
    wb = w_in.gather(1, blk.unsqueeze(2).expand(-1, -1, G))              # [M, n, G]
    run = wb.cumsum(2)
    thr = (u2 * run[..., -1]).unsqueeze(2)
    off = (run <= thr).sum(2)
    off = torch.where(off >= G, (run < run[..., -1:]).sum(2), off).clamp_max(G - 1)    # nothing above: where the sum is complete
    col = (blk * G + off).clamp_max(n_cols - 1)
    ids = col + (0 if mistake == 'zero_based' else 1)
    logp = s_w.gather(1, col) - lse.view(-1, 1)
    pos_logp = None
    if pos is not None:
        p = pos.cpu().long()
        pos_logp = torch.where(p == 0, torch.full(p.shape, float('-inf')), s_w.gather(1, (p - 1).clamp(0, n_cols - 1)) - lse.view(-1, 1))
    return ids, logp, pos_logp, lse
