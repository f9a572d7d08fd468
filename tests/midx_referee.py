"""Float64 referee of the adaptive samplers (rsa_midx_sample / rsa_midx_lookup, rsa_kmeans_step, MIDXSamplerUniform /
ClusterSamplerUniform.update), the bounds a correct fp32 implementation stays inside, and an fp32 emulation of the draw.
Test code only: nothing here calls recstudio_amd.  Runs on whatever device its tensors live on.

Semantics (recstudio/ann/sampler.py:261-510, uniform-in-bucket forms; P = 2 halves for MIDX, P = 1 for Cluster):

    qh        = q / max(||q||, 1e-12) with a CosineScorer, q otherwise
    r_p[k]    = <qh_p, c_p[k]>
    MIDX      P(k0, k1) ~ wkk[k0, k1] e^{r_0[k0]} e^{r_1[k1]};   F0 = CDF of the marginal of k0, F1(. | k0) of k1 given k0
    Cluster   P(k) ~ wkk[k] e^{r[k]}
    item      idx = min(floor(float32(cnt) * u2), cnt - 1) in bucket k0 * K + k1,  id = indices[indptr[b] + idx] + 1
    log-prob  r_0[k0] + r_1[k1]   (unnormalised, as the reference returns it); compute_item_p the same for the clusters of an id

BOUNDS, with u = 2^-24 and gamma(n) = n u / (1 - n u).

Logit.  The kernel sums a half's dsub products on four interleaved FMA chains (dsub / 4 FMAs each, the product inside an FMA is
not rounded) and adds the chains as (x + y) + (z + w): a product passes through at most dsub / 4 + 2 roundings.  With a cosine
scorer every element of qh carries one more (the sum of squares is taken in double, the quotient rounded once).  Hence
    |r^ - r| <= eps_r[k] = gamma(dsub / 4 + 3) * sum_i |qh_i c_k,i|
-- tighter than a sequential sum's (dsub + 1) u.  A returned log-prob adds the halves: one more rounding, u |r_0 + r_1|.

CDF.  A weight is wkk * e^{r - m} (m any constant per half: it cancels in the ratio).  Relative error of a computed weight:
exponent eps_r[k] + u |r - m| (the rounding of the subtraction), expf 1 ulp = 2 u per exponential (two of them in MIDX's first
stage), the products wkk * e, e_0 * t: 1 u each, the K-term sum t: K u.  A running sum of K weights adds K u.  So numerator and
denominator of a CDF value each carry at most
    eta = sum over the halves involved (max_k eps_r[k] + u max_k |r[k] - m|) + (2 K + 8) u
and the comparison `running sum > fl(u0 * S)` one more u (inside the 8): a draw u0 that returned k satisfies
    F[k - 1] - tol <= u0 <= F[k] + tol,      tol = 2 (e^eta - 1).
The first stage of MIDX involves both halves, F1(. | k0) only half 1, Cluster its single part.
Against the simpler form 2 (2 eps' + (2 K + 8) u) with eps' = (d / 2 + 1) u max_k sum_i |q_i c_k,i| per half: with S = that sum and
|r - m| <= 2 S, a half contributes here at most (dsub / 4 + 3 + 2) u S = (d / 8 + 5) u S against (d / 2 + 1) u S there.  That is
tighter from d = 16 on (7 against 9, then 13 against 33 at d = 64, ...).  Only at the smallest shape, d = 8 (dsub = 4), can it be
wider, 6 u S against 5 u S in the worst case, up to 20 %: the term u |r - m| is a rounding the kernel really commits (the
subtraction of the row maximum), which the simpler form does not count, so it stays.

Lloyd step.  Score s_k = fl(||c_k||^2 - 2 <x, c_k>) with ||c||^2 rounded once from double and the last operation an FMA:
    |s^_k - s_k| <= E_k = 2 gamma(dsub / 4 + 3) sum_i |x_i c_k,i| + u ||c_k||^2 + u |s_k|
(the + 3 covers the rounding of a normalised row).  A row is DECIDED when its best score beats every other by more than the two
bounds together; only undecided rows may differ from the float64 assignment.  Sums: a cluster's rows are added one by one in fp32
inside a workgroup and the workgroups' partials in double: at most count + 1 roundings, judged at (count + 2) u sum |x|.
"""
import numpy as np
import torch

U32 = 2.0 ** -24


def gamma(n):
    return n * U32 / (1.0 - n * U32)


def normalize64(x):
    x = x.double()
    return x / x.norm(dim=-1, keepdim=True).clamp_min(1e-12)


def logits(query, centres, cosine):
    """query [M, d], centres [P, K, dsub] -> (r [P, M, K], eps_r [P, M, K]) float64."""
    P, K, dsub = centres.shape
    q = normalize64(query) if cosine else query.double()
    c = centres.double()
    r, a = [], []
    for p in range(P):
        qp = q[:, p * dsub:(p + 1) * dsub]
        r.append(qp @ c[p].t())
        a.append(qp.abs() @ c[p].abs().t())
    r, a = torch.stack(r), torch.stack(a)
    return r, gamma(dsub // 4 + 3) * a


def tables(query, centres, wkk, cosine):
    """Everything a draw is judged against: r, eps [P, M, K]; F0 [M, K]; F1 [M, K, K] (MIDX; rows of empty k0 are NaN);
    tol0, tol1 [M]."""
    P, K, _ = centres.shape
    r, eps = logits(query, centres, cosine)
    w = wkk.double()
    m = r.max(dim=2, keepdim=True)[0]
    e = torch.exp(r - m)
    spread = (r - m).abs().max(dim=2)[0]                        # [P, M]
    eta_p = eps.max(dim=2)[0] + U32 * spread                    # [P, M]
    fixed = (2 * K + 8) * U32
    out = dict(r=r, eps=eps)
    if P == 2:
        v = e[1].unsqueeze(1) * w.unsqueeze(0)                  # [M, K0, K1]
        t = v.sum(2)
        w0 = e[0] * t
        out['F0'] = w0.cumsum(1) / w0.sum(1, keepdim=True)
        out['F1'] = v.cumsum(2) / t.unsqueeze(2)
        out['tol0'] = 2 * torch.expm1(eta_p[0] + eta_p[1] + fixed)
        out['tol1'] = 2 * torch.expm1(eta_p[1] + fixed)
    else:
        w0 = e[0] * w.view(1, K)
        out['F0'] = w0.cumsum(1) / w0.sum(1, keepdim=True)
        out['tol0'] = 2 * torch.expm1(eta_p[0] + fixed)
    return out


def item_logp(tab, cd, ids):
    """compute_item_p: ids [M, T] (0 = padding) -> (value [M, T] float64, bound [M, T])."""
    r, eps = tab['r'], tab['eps']
    val = torch.zeros(ids.shape, dtype=torch.float64, device=ids.device)
    bound = torch.zeros_like(val)
    for p, c in enumerate(cd):
        k = c.to(ids.device)[ids]                               # 0 = padding -> the zero row
        rp = torch.cat([r[p].new_zeros(r[p].shape[0], 1), r[p]], 1)
        ep = torch.cat([eps[p].new_zeros(eps[p].shape[0], 1), eps[p]], 1)
        val += rp.gather(1, k)
        bound += ep.gather(1, k)
    return val, bound + U32 * val.abs()


def build_index(cd, K):
    """cd: list of P int64 arrays [N] (clusters without the shift) -> (indices, indptr, wkk) as construct_index builds them."""
    P = len(cd)
    bucket = cd[0] * K + cd[1] if P == 2 else cd[0]
    bucket = torch.as_tensor(bucket).cpu()
    indices = torch.sort(bucket, stable=True)[1]
    count = torch.bincount(bucket, minlength=K ** P)
    indptr = torch.cat([count.new_zeros(1), count.cumsum(0)])
    wkk = count.float().view(K, K) if P == 2 else count.float()
    return indices, indptr, wkk


def judge_draws(tab, wkk, indptr, indices, cd, ids, u, logp=None):
    """Every draw of ids [M, n] (uniforms u [M, n, P + 1]) against the intervals above.  -> dict of violation COUNTS (all must be
    0) and of the worst excess over each tolerance, in units of the tolerance (``*_ratio`` <= 1 passes)."""
    P = len(cd)
    dev = ids.device
    M, n = ids.shape
    K = tab['F0'].shape[1]
    N = indices.numel()
    wkk, indptr, indices = wkk.to(dev), indptr.to(dev).long(), indices.to(dev).long()
    res = dict(id_range=int(((ids < 1) | (ids > N)).sum()))
    idc = ids.clamp(1, N)
    k = [c.to(dev)[idc] - 1 for c in cd]
    bucket = k[0] * K + k[1] if P == 2 else k[0]
    res['empty_bucket'] = int((wkk.reshape(-1)[bucket] <= 0).sum())
    inv = torch.empty(N, dtype=torch.long, device=dev)
    inv[indices] = torch.arange(N, device=dev)
    idx = inv[idc - 1] - indptr[bucket]
    cnt = indptr[bucket + 1] - indptr[bucket]
    want = torch.floor(cnt.float() * u[..., P].float()).long()
    want = torch.minimum(want, cnt - 1).clamp_min(0)
    res['item_index'] = int((idx != want).sum())

    def interval(F, kk, uu, tol):
        hi = F.gather(1, kk)
        lo = torch.where(kk > 0, F.gather(1, (kk - 1).clamp_min(0)), torch.zeros_like(hi))
        excess = torch.maximum(lo - uu, uu - hi).clamp_min(0) / tol.view(-1, 1)
        excess = torch.where(torch.isnan(excess), torch.full_like(excess, float('inf')), excess)
        return int((excess > 1).sum()), float(excess.max())

    res['cdf0'], res['cdf0_ratio'] = interval(tab['F0'], k[0], u[..., 0].double(), tab['tol0'])
    if P == 2:
        F1 = tab['F1'].gather(1, k[0].view(M, n, 1).expand(M, n, K))          # [M, n, K]: the row of each draw's k0
        hi = F1.gather(2, k[1].unsqueeze(2)).squeeze(2)
        lo = torch.where(k[1] > 0, F1.gather(2, (k[1] - 1).clamp_min(0).unsqueeze(2)).squeeze(2), torch.zeros_like(hi))
        uu = u[..., 1].double()
        excess = torch.maximum(lo - uu, uu - hi).clamp_min(0) / tab['tol1'].view(-1, 1)
        excess = torch.where(torch.isnan(excess), torch.full_like(excess, float('inf')), excess)
        res['cdf1'], res['cdf1_ratio'] = int((excess > 1).sum()), float(excess.max())
    if logp is not None:
        val, bound = item_logp(tab, cd, idc)
        ex = (logp.double() - val).abs() / bound.clamp_min(1e-300)
        res['logp'], res['logp_ratio'] = int((ex > 1).sum()), float(ex.max())
    return res


def violations(res):
    return {k: v for k, v in res.items() if not k.endswith('_ratio') and v}


# ------------------------------------------------------------------------------------------------- fp32 emulation of the draw
def _pick(w, target):
    """First k with w[k] > 0 whose fp32 running sum exceeds target; the last such k when none does (rsa_midx.hip, TIE RULE)."""
    run = torch.cumsum(w, 0, dtype=torch.float32)
    pos = w > 0
    hit = torch.nonzero(pos & (run > target)).flatten()
    if hit.numel():
        return int(hit[0])
    return int(torch.nonzero(pos).flatten()[-1])


def emulate_draws(query, centres, wkk, indptr, indices, u, cosine, mistake=None):
    """fp32 emulation (CPU, draw by draw) of the kernel's arithmetic -> (ids [M, n] int64, logp [M, n] fp32).  ``mistake``: one of
    the seeded errors a referee must catch ('wkk_transposed', 'wkk_ignored', 'halves_swapped', 'no_normalize', 'no_plus_one',
    'empty_bucket')."""
    P, K, dsub = centres.shape
    M, n = u.shape[:2]
    q = query.float()
    if cosine and mistake != 'no_normalize':
        q = (q.double() / q.double().norm(dim=-1, keepdim=True).clamp_min(1e-12)).float()
    w = wkk.float()
    if mistake == 'wkk_transposed':
        w = w.t().contiguous()
    if mistake == 'wkk_ignored':
        w = torch.ones_like(w)
    ids = torch.zeros(M, n, dtype=torch.int64)
    logp = torch.zeros(M, n, dtype=torch.float32)
    for b in range(M):
        halves = [q[b, p * dsub:(p + 1) * dsub] for p in range(P)]
        if mistake == 'halves_swapped' and P == 2:
            halves = halves[::-1]
        r = [(centres[p].float() * halves[p]).sum(1, dtype=torch.float32) for p in range(P)]
        e = [torch.exp(x - x.max()) for x in r]
        for j in range(n):
            if P == 2:
                t = torch.cumsum(w * e[1].view(1, K), 1, dtype=torch.float32)[:, -1]
                w0 = e[0] * t
                k0 = _pick(w0, u[b, j, 0] * torch.cumsum(w0, 0, dtype=torch.float32)[-1])
                v = w[k0] * e[1]
                if mistake == 'empty_bucket':
                    v = torch.where(wkk[k0].float() > 0, torch.zeros_like(v), e[1])
                    if not (v > 0).any():
                        v = w[k0] * e[1]
                k1 = _pick(v, u[b, j, 1] * torch.cumsum(v, 0, dtype=torch.float32)[-1])
                bucket, lp = k0 * K + k1, r[0][k0] + r[1][k1]
            else:
                w0 = w * e[0]
                if mistake == 'empty_bucket' and (wkk <= 0).any():
                    w0 = torch.where(wkk.float() > 0, torch.zeros_like(w0), e[0])
                k0 = _pick(w0, u[b, j, 0] * torch.cumsum(w0, 0, dtype=torch.float32)[-1])
                bucket, lp = k0, r[0][k0]
            start, cnt = int(indptr[bucket]), int(indptr[bucket + 1] - indptr[bucket])
            if cnt <= 0:                       # (only a seeded mistake gets here: any id of another bucket)
                ids[b, j] = int(indices[0]) + 1
            else:
                idx = min(int(torch.floor(torch.tensor(float(cnt), dtype=torch.float32) * u[b, j, P].float())), cnt - 1)
                ids[b, j] = int(indices[start + idx]) + (0 if mistake == 'no_plus_one' else 1)
            logp[b, j] = lp
    return ids, logp


# ------------------------------------------------------------------------------------------------- k-means
def kmeans_scores(X, centres, normalize):
    """-> (x64 [N, d] the rows as clustered, s [P, N, K] = ||c||^2 - 2 <x, c>, E [P, N, K] the bound on a computed score)."""
    P, K, dsub = centres.shape
    x = normalize64(X) if normalize else X.double()
    c = centres.double()
    s, E = [], []
    for p in range(P):
        xp = x[:, p * dsub:(p + 1) * dsub]
        cn = (c[p] * c[p]).sum(1)
        sp = cn.view(1, K) - 2 * (xp @ c[p].t())
        s.append(sp)
        E.append(2 * gamma(dsub // 4 + 3) * (xp.abs() @ c[p].abs().t()) + U32 * cn.view(1, K) + U32 * sp.abs())
    return x, torch.stack(s), torch.stack(E)


def decided_rows(s, E):
    """assign [P, N] = float64 argmin, decided [P, N] = no other cluster within the two error bounds of the best."""
    best = s.argmin(2)
    top = (s + E).gather(2, best.unsqueeze(2)).squeeze(2)
    low = (s - E).scatter(2, best.unsqueeze(2), float('inf')).min(2)[0]
    return best, low > top


def cluster_sums(x, assign, K, dsub):
    """Float64 sums over a GIVEN assignment [P, N] -> (sums [P, K, dsub], abs sums, counts [P, K], loss [P] given centres later)."""
    P, N = assign.shape
    sums = torch.zeros(P, K, dsub, dtype=torch.float64, device=x.device)
    asum = torch.zeros_like(sums)
    counts = torch.zeros(P, K, dtype=torch.int64, device=x.device)
    for p in range(P):
        xp = x[:, p * dsub:(p + 1) * dsub]
        sums[p].index_add_(0, assign[p], xp)
        asum[p].index_add_(0, assign[p], xp.abs())
        counts[p] = torch.bincount(assign[p], minlength=K)
    return sums, asum, counts


def cluster_loss(x, assign, centres, normalize):
    """(loss [P] float64 over the given assignment, its bound): the kernel takes the squared distances in double from the fp32
    rows -- a normalised row carries one rounding per element, u |x_i|, which moves (x_i - c_i)^2 by at most 2 u |x_i| |x_i - c_i|
    (+ second order); the double sums themselves add (N + dsub) 2^-53 relative."""
    P, K, dsub = centres.shape
    c = centres.double()
    loss, bound = [], []
    for p in range(P):
        xp = x[:, p * dsub:(p + 1) * dsub]
        diff = xp - c[p][assign[p]]
        lp = (diff * diff).sum()
        b = (xp.shape[0] + dsub) * 2.0 ** -52 * lp
        if normalize:
            b = b + 2.0 * gamma(2) * (xp.abs() * diff.abs()).sum()
        loss.append(lp)
        bound.append(b)
    return torch.stack(loss), torch.stack(bound)


def lloyd(X, centres, normalize, max_iter=30, K=None):
    """kmeans() of the reference (sampler.py:9-35) per part in float64 from given centres [P, K, dsub]; dead clusters re-seeded
    from X[torch.randperm(N)[:ndead]] on the CPU generator.  -> (centres [P, K, dsub] float64, assign [P, N], counts_last)."""
    P, K, dsub = centres.shape
    x = normalize64(X) if normalize else X.double()
    N = x.shape[0]
    C_out, A_out = [], []
    for p in range(P):
        xp = x[:, p * dsub:(p + 1) * dsub]
        C = centres[p].double().clone()
        prev = np.inf
        assign = None
        for _ in range(max_iter):
            dist = (C * C).sum(1).view(1, K) - 2 * (xp @ C.t())
            assign = dist.argmin(1)
            loss = float(((xp - C[assign]) ** 2).sum())
            if (prev - loss) < prev * 1e-6:
                break
            prev = loss
            count = torch.bincount(assign, minlength=K)
            C = torch.zeros_like(C).index_add_(0, assign, xp) / count.double().view(K, 1)
            dead = count == 0
            if int(dead.sum()):
                C[dead] = xp[torch.randperm(N)[:int(dead.sum())].to(xp.device)]
        C_out.append(C)
        A_out.append(assign)
    return torch.stack(C_out), torch.stack(A_out)


def centre_bound(x, assign, centres):
    """A centre is an fp32 mean of its rows: (count + 2) u sum|x| / count from the sum (above) + u |c| from the division --
    doubled when two fp32 implementations (the recorded reference and the kernel path) are compared with each other."""
    P, K, dsub = centres.shape
    _, asum, counts = cluster_sums(x, assign, K, dsub)
    cnt = counts.double().clamp_min(1).unsqueeze(2)
    return ((cnt + 2) * U32 * asum / cnt + U32 * centres.double().abs())


def edge_uniforms(tab, n, parts, generator):
    """u [M, n, parts + 1] fp32 on the tables' device: random uniforms with, in about half the slots, an exact edge -- 0,
    1 - 2^-24, or an fp32 neighbour (below / at / above) of a float64 CDF boundary of that query."""
    F = tab['F0']
    M, dev = F.shape[0], F.device
    cand = [F]
    if parts == 2:
        cand.append(tab['F1'].reshape(M, -1))
    f32 = torch.nan_to_num(torch.cat(cand, 1), nan=0.5).clamp(0.0, 1.0).float()
    zero, two = torch.zeros_like(f32), torch.full_like(f32, 2.0)
    top = 1.0 - 2.0 ** -24
    edges = torch.cat([f32, torch.nextafter(f32, zero), torch.nextafter(f32, two), torch.zeros(M, 1, device=dev),
                       torch.full((M, 1), top, device=dev)], 1).clamp(0.0, top)
    g = generator
    u = torch.rand(M, n, parts + 1, generator=g).to(dev)
    pick = torch.randint(0, edges.shape[1], (M, n * (parts + 1)), generator=g).to(dev)
    use = (torch.rand(M, n, parts + 1, generator=g) < 0.5).to(dev)
    return torch.where(use, edges.gather(1, pick).view(M, n, parts + 1), u).contiguous()
