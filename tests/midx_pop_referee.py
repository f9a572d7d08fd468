"""Float64 referee of the popularity-in-bucket samplers (rsa_midx_weights, the weighted draw of rsa_midx_sample / rsa_midx_lookup,
MIDXSamplerPop / ClusterSamplerPop), the bounds a correct fp32 implementation stays inside, and an fp32 emulation of the new step
with seeded mistakes.  Test code only: nothing here calls recstudio_amd.  The codebook stages are midx_referee's, unchanged.

Semantics (recstudio/ann/sampler.py:391-423, :533-559 for the tables; the draw is the one that agrees with compute_item_p, not
the reference's _sample_item_with_pop, :349-365).  Item ids run 1 .. N, positions 0 .. N - 1 in ``indices`` order:

    w_i       = pop[i - 1]  (* exp(-||x_i||^2 / 2) with a EuclideanScorer; norm and exp in double, ONE rounding to fp32)
    p         = [1, w_1 .. w_N],   logp = fl32(log(double(p)))       (entry 0 is 0, a weight of 0 gives -inf)
    wkk[b]    = fl32(sum of w over bucket b)                          (summed in double)
    cp[pos]   = fl32(prefix64(pos) / total64(b)) inside its bucket;   a bucket of total 0: cp = 0, wkk = 0
    draw      pos = first position of the bucket with cp[pos] > u2;   id = indices[pos] + 1
    log-prob  fl(fl(r_0[k0] + r_1[k1]) + logp[id]);   compute_item_p the same for a given id (the padding id gives 0)

BOUNDS, with u = 2^-24.

Weight.  One rounding of the double value: |w - w64| <= u |w64| + 2^-150 (the second term is half the smallest fp32 subnormal: the
rounding error below the normal range), plus what two correct double evaluations may differ by: the d-term sum of squares
carries (d + 1) 2^-53 relative, which moves the exponent ||x||^2 / 2 by that much of its size, and exp and the product 2^-52 more:
(((d + 1) ||x||^2 / 2 + 4) 2^-53) |w64|.

wkk.  One rounding of a double sum of the fp32 weights: u S, plus cnt 2^-53 S for the order of the double additions.

cp.  One rounding of a value <= 1: |cp - cp64| <= u (+ 2 N 2^-53 for the double sums, the referee's own included).  A draw that returned position pos must
therefore satisfy  cp64[pos - 1] - u' <= u2 <= cp64[pos] + u'  (cp64 = 0 before the bucket's first position), u' = that bound.
A position of weight 0 has cp64[pos - 1] = cp64[pos]: only a u2 within u' of that value could excuse it, and the count of drawn
zero-weight items is reported on its own and must be 0.

In-bucket index.  Given the sampler's OWN cp table the position is exact: searchsorted(cp[start:end], u2, right=True).

Log-probabilities.  midx_referee's logit bound (eps_r per half + u |r_0 + r_1|), plus u |logp| for the rounding of the table entry,
plus 2^-52 |logp| for the double log it is rounded from, plus u |sum| for the final addition.  The table entry is judged from the
sampler's own fp32 p (log(double(p))): p has its own bound above.

Fixture comparison (the recorded tables are the reference's fp32 ones: a matmul / cumsum over a bucket's cnt weights): an fp32 sum
of cnt terms is within (cnt + 2) u S of the exact one, as midx_referee.centre_bound argues; doubled for two fp32 implementations.
wkk: 2 (cnt + 2) u S.  cp = prefix / total, both sums carrying that relative error, then one division: 2 (2 (cnt + 2) + 1) u.
p: the constructor's transform is torch's fp32 log / pow, 1 ulp = 2 u, plus u for mode 1's addition: two machines' values are
within 6 u relative of each other (TRANSFORM_REL), and wkk / cp / log p inherit that.  With a Euclidean scorer, on top: the reference takes sum(x^2) in fp32, (d + 1) u relative, so exp's argument moves by (d + 1) u ||x||^2 / 2;
exp, the product and our own rounding add 4 u:  |p - p_ref| <= (expm1((d + 1) u ||x||^2 / 2) + 4 u) p.
"""
import torch

import midx_referee as R

U32 = R.U32
TINY = 2.0 ** -150
# two fp32 evaluations of the constructor's transform (log or pow at 1 ulp = 2 u, mode 1's addition u) on different machines
TRANSFORM_REL = 6 * U32


def transform(counts, mode):
    """The constructor's transform of the raw counts (sampler.py:399-404), in fp32 as torch computes it there."""
    c = counts.float()
    if mode == 0:
        return torch.log(c + 1)
    if mode == 1:
        return torch.log(c + 1) + 1e-6
    if mode == 2:
        return c ** 0.75
    return c


def weights64(pop, X=None):
    """(w64 [N] the exact weight in double, bound [N] on an fp32 weight computed as described above)."""
    w = pop.double()
    if X is None:
        return w, torch.zeros_like(w)                            # the weight IS the fp32 popularity
    ss = (X.double() ** 2).sum(1)
    w = w * torch.exp(-0.5 * ss)
    d = X.shape[1]
    return w, U32 * w + TINY + ((d + 1) * 0.5 * ss + 4) * 2.0 ** -53 * w


def bucket_of_position(indptr):
    """[N] the bucket every sorted position lies in."""
    indptr = indptr.long()
    cnt = indptr[1:] - indptr[:-1]
    return torch.repeat_interleave(torch.arange(cnt.numel(), device=indptr.device), cnt)


def tables64(w, indices, indptr):
    """Float64 tables from weights w [N] (by item) and the index -> dict(p [N + 1], logp [N + 1], wkk [B], cp [N], cp_prev [N] the
    CDF before each position, cnt [B], bucket [N] of each position, wpos [N] the weight at each position)."""
    dev = w.device
    indices, indptr = indices.to(dev).long(), indptr.to(dev).long()
    w = w.double()
    wpos = w[indices]
    bucket = bucket_of_position(indptr)
    nb = indptr.numel() - 1
    wkk = torch.zeros(nb, dtype=torch.float64, device=dev).index_add_(0, bucket, wpos)
    # every weight as a share of its bucket FIRST, then one running sum over the whole table minus its value in front of the bucket:
    # the shares are at most 1 and the sum at most the number of buckets, so the subtraction costs N 2^-53 absolute whatever the
    # weights' range is (buckets of total 1e-40 next to buckets of total 1e3)
    tot = wkk[bucket]
    share = torch.where(tot > 0, wpos / torch.where(tot > 0, tot, torch.ones_like(tot)), torch.zeros_like(wpos))
    run = share.cumsum(0)
    before = torch.cat([run.new_zeros(1), run])[indptr[:-1]]      # the running sum in front of each bucket
    cp = run - before[bucket]
    cp_prev = torch.where(share > 0, cp - share, cp)              # (a weight of 0 leaves the CDF where it is, exactly)
    p = torch.cat([w.new_ones(1), w])
    return dict(p=p, logp=torch.log(p), wkk=wkk, cp=cp.clamp(0, 1), cp_prev=cp_prev.clamp(0, 1), cnt=indptr[1:] - indptr[:-1],
                bucket=bucket, wpos=wpos)


def cp_bound(t):
    """[N]: |cp - cp64| per position (the second term: the referee's own running sum over all N positions, see tables64)."""
    return U32 + 2.0 * t['bucket'].numel() * 2.0 ** -53 + 0.0 * t['cp']


def wkk_bound(t):
    return (U32 + t['cnt'].double() * 2.0 ** -53) * t['wkk']


def own_index(cp, indptr, bucket, u2):
    """The exact position given the sampler's own fp32 cp: start + searchsorted(cp[start:end], u2, right=True) for draws in
    ``bucket`` [..] with uniforms ``u2`` [..] (a vectorised bisection); end where no position exceeds u2."""
    indptr = indptr.long()
    lo, hi = indptr[bucket].clone(), indptr[bucket + 1].clone()
    cp = torch.cat([cp.float(), cp.new_zeros(1).float()])
    for _ in range(33):
        live = lo < hi
        mid = (lo + hi) // 2
        up = cp[mid.clamp_max(cp.numel() - 1)] > u2.float()
        hi = torch.where(live & up, mid, hi)
        lo = torch.where(live & ~up, mid + 1, lo)
    return lo


def judge_items(t, cp_own, indptr, indices, cd, K, ids, u2):
    """The in-bucket stage of every draw ids [M, n] (uniforms u2 [M, n]) -> dict of violation COUNTS (all must be 0) and
    ``inbucket_ratio`` (the worst excess over the interval, in units of its tolerance).
      zero_weight   the drawn item weighs 0
      own_index     the position differs from searchsorted(own cp of the bucket, u2, right=True)
      inbucket      u2 outside [cp64[pos - 1] - tol, cp64[pos] + tol]"""
    dev = ids.device
    indices, indptr = indices.to(dev).long(), indptr.to(dev).long()
    N = indices.numel()
    idc = ids.clamp(1, N)
    k = [c.to(dev)[idc] - 1 for c in cd]
    bucket = k[0] * K + k[1] if len(cd) == 2 else k[0]
    inv = torch.empty(N, dtype=torch.long, device=dev)
    inv[indices] = torch.arange(N, device=dev)
    pos = inv[idc - 1]
    res = dict(zero_weight=int((t['wpos'][pos] <= 0).sum()))
    want = own_index(cp_own.to(dev), indptr, bucket, u2)
    res['own_index'] = int((want != pos).sum())
    tol = cp_bound(t)[pos]
    uu = u2.double()
    excess = torch.maximum(t['cp_prev'][pos] - uu, uu - t['cp'][pos]).clamp_min(0) / tol
    res['inbucket'], res['inbucket_ratio'] = int((excess > 1).sum()), float(excess.max())
    return res


def judge_logp(tab, logp_own, cd, ids, got):
    """Log-probabilities ``got`` of ids [M, T] (0 = padding) against logits64 + log(double(own p)) -> (count, worst ratio);
    infinities (a weight of 0) must agree exactly."""
    val, bound = R.item_logp(tab, cd, ids)
    lp = logp_own.double().to(ids.device)[ids]
    fin = torch.isfinite(lp)
    lpf = torch.where(fin, lp, torch.zeros_like(lp))
    want = val + lpf
    bound = bound + (U32 + 2.0 ** -52) * lpf.abs() + U32 * want.abs()
    got = got.double()
    ex = torch.where(fin, (got - want).abs() / bound.clamp_min(1e-300), torch.where(got == lp, 0.0, float('inf')).double())
    ex = torch.where(torch.isnan(ex), torch.full_like(ex, float('inf')), ex)
    return int((ex > 1).sum()), float(ex.max()) if ex.numel() else 0.0


def judge_all(query, centres, wkk_own, cp_own, logp_own, w_own, indptr, indices, cd, ids, u, logp, cosine):
    """Every stage of weighted draws ids [M, n] (uniforms u [M, n, P + 1]): the codebook stages by midx_referee.judge_draws against
    the CDFs of the sampler's OWN fp32 wkk (what the kernel is handed; ``wkk_own`` counts the entries of that table outside their
    own bound), the in-bucket stage and the log-probabilities by the judges above, from the sampler's own fp32 weights."""
    P, K = centres.shape[0], centres.shape[1]
    t = tables64(w_own, indices, indptr)
    wkk = wkk_own.double().to(t['wkk'].device)
    wkk = wkk.reshape(K, K) if P == 2 else wkk.reshape(K)
    tab = R.tables(query, centres, wkk, cosine)
    res = R.judge_draws(tab, wkk, indptr, indices, cd, ids, u)
    del res['item_index']                                        # (the uniform forms' in-bucket rule)
    res.update(judge_items(t, cp_own, indptr, indices, cd, K, ids, u[..., P]))
    res['logp'], res['logp_ratio'] = judge_logp(tab, logp_own, cd, ids.clamp(1, indices.numel()), logp)
    res['wkk_own'] = int(((wkk_own.double().reshape(-1).to(t['wkk'].device) - t['wkk']).abs() > wkk_bound(t)).sum())
    return res


def edge_uniforms(tab, t, indptr, n, parts, generator):
    """midx_referee.edge_uniforms, with the in-bucket slot's edges taken from the float64 in-bucket CDF: the fp32 neighbours below /
    at / above cp values, 0 and 1 - 2^-24, in about half the slots."""
    u = R.edge_uniforms(tab, n, parts, generator)
    M, dev = u.shape[0], u.device
    cp = t['cp'].float().to(dev)
    zero, two = torch.zeros_like(cp), torch.full_like(cp, 2.0)
    top = 1.0 - 2.0 ** -24
    edges = torch.cat([cp, torch.nextafter(cp, zero), torch.nextafter(cp, two), cp.new_zeros(1), cp.new_full((1,), top)]).clamp(0.0, top)
    pick = torch.randint(0, edges.numel(), (M, n), generator=generator).to(dev)
    use = (torch.rand(M, n, generator=generator) < 0.5).to(dev)
    u[..., parts] = torch.where(use, edges[pick], torch.rand(M, n, generator=generator).to(dev))
    return u.contiguous()


# ------------------------------------------------------------------------------------------------- fp32 emulation
def emulate_tables(w, indices, indptr):
    """The fp32 tables as the kernel builds them (double sums in ``indices`` order, one rounding): (p, logp, wkk, cp) on the CPU."""
    t = tables64(w.float().cpu(), indices.cpu(), indptr.cpu())
    return t['p'].float(), t['logp'].float(), t['wkk'].float(), t['cp'].float()


MISTAKES = ('p_by_position', 'no_plus_one', 'uniform_in_bucket', 'logp_missing', 'wkk_counts', 'zero_weight_drawn')


def emulate_draws(query, centres, counts_wkk, indptr, indices, cd, w, u, cosine, mistake=None):
    """fp32 emulation (CPU, draw by draw) of the weighted draw -> (ids [M, n], logp [M, n] fp32).  The codebook stages are
    midx_referee.emulate_draws' (its uniform item tells the bucket it chose).  ``mistake``: one of MISTAKES --
      p_by_position      log p read at the sorted position + 1 (the reference's indexing, sampler.py:364)
      no_plus_one        id = indices[pos] (sampler.py:362)
      uniform_in_bucket  the item uniform in its bucket
      logp_missing       log p not added
      wkk_counts         the codebook stages weigh a bucket by its item count
      zero_weight_drawn  the LAST position of a run of equal cp values instead of the first"""
    P, K, _ = centres.shape
    p, logp_tab, wkk, cp = emulate_tables(w, indices, indptr)
    wkk = wkk.view(K, K) if P == 2 else wkk
    stage_wkk = counts_wkk.float() if mistake == 'wkk_counts' else wkk
    ids_u, lp = R.emulate_draws(query, centres, stage_wkk, indptr, indices, u, cosine)
    k = [c[ids_u] - 1 for c in cd]
    bucket = k[0] * K + k[1] if P == 2 else k[0]
    M, n = ids_u.shape
    ids = torch.zeros_like(ids_u)
    out = torch.zeros(M, n, dtype=torch.float32)
    for b in range(M):
        for j in range(n):
            start, end = int(indptr[bucket[b, j]]), int(indptr[bucket[b, j] + 1])
            seg = cp[start:end]
            off = int(torch.searchsorted(seg, u[b, j, P].float().view(1), right=True))
            if off >= end - start:                              # nothing exceeds u2: the last position whose cp exceeds its predecessor's
                off = int(torch.searchsorted(seg, seg[-1:], right=False)) if float(seg[-1]) > 0 else 0
            if mistake == 'zero_weight_drawn':
                off = int(torch.searchsorted(seg, seg[off:off + 1], right=True)) - 1
            pos = start + off
            item = int(indices[pos]) + (0 if mistake == 'no_plus_one' else 1)
            if mistake == 'uniform_in_bucket':
                item = int(ids_u[b, j])
            ids[b, j] = item
            lw = logp_tab[pos + 1] if mistake == 'p_by_position' else logp_tab[min(max(item, 0), indices.numel())]
            out[b, j] = lp[b, j] if mistake == 'logp_missing' else lp[b, j] + lw
    return ids, out
