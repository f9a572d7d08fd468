"""Float64 rule of the in-batch InfoNCE (data_augmentation.batch_infonce_torch, BatchInfoNCELoss: neg_type 'batch_both' /
'batch_single'), forward and backward, written from what the reference's source spells out
(recstudio/model/module/data_augmentation.py:324-376) with explicit sums -- no autograd, no cross_entropy.  The reference's module
cannot be imported where faiss is missing, so nothing is recorded.

The logit set of row b:
    always   s_ij[b, k] = <zi_b, zj_k> inv_t   for every k except those with k != b and labels[k] == labels[b];
    `both`   s_ii[b, k] = <zi_b, zi_k> inv_t   for every k != b whose label differs from labels[b] (without labels: every k != b).
    lse_b = log sum exp over the set;  pos_b = s_ij[b, b];  the loss is mean(lse - pos).
Backward from g [B] on lse - pos, with P = exp(s - lse_b) on the set and 0 off it:
    dzi_b = inv_t [ g_b (sum_k P_ij[b, k] zj_k + sum_k P_ii[b, k] zi_k - zj_b) + sum_r g_r P_ii[r, b] zi_r ]
    dzj_k = inv_t [ sum_b g_b P_ij[b, k] zi_b - g_k zi_k ]

``mistake=`` names one seeded mistake (tests/test_batch_infonce_referee.py shows that each of them leaves a bound).

THE BOUNDS (``judge``; u = 2^-24, every sum of n fp32 terms within (n + 2) u sum|terms|, no fitted constant).
  s       a d-term dot product on the matrix cores, then one product with inv_t:
              e_s = inv_t (d + 2) u sum_c |zi_bc z_kc| + u |s|
  exp/log ``allowance(device)``: twice the worst RELATIVE error torch's own fp32 exp shows on the device against float64 on a grid
          over [-60, 0] (a_e), and twice the worst ABSOLUTE error of its fp32 log on [1, 2^18] (a_l) -- measured the way
          ff_attention_referee.sigmoid_allowance measures the sigmoid's.
  lse     the kernel keeps, per lane, a running maximum m and a running sum over its 16 entries of every 32-row tile, rescales the sum
          by exp(m_old - m_new) when the maximum moves, and merges the two halves of a column at the end.  With NT tiles streamed
          (ceil(B / 32), twice that with `both`), R = max_k t_k - min_k t_k over the row's set and P the softmax over the set:
              term k      relative  e_s[k] + u |t_k - m| + a_e              (argument error through exp's slope 1, the exp itself)
              rescales    at most NT + 1 of them, each relative  a_e + u R + 2 u
              the sum     17 additions per tile in a lane's chain:  (17 NT + 4) u  relative (all terms positive)
              rel   = sum_k P_k (e_s[k] + u R) + a_e + (17 NT + 4) u + (NT + 1) (a_e + u R + 2 u)
              e_lse = rel + a_l + 2 u |lse|                                 (log's slope on a relative error is 1; m + log rounded)
  pos     e_pos = e_s[b, b]
  P       recomputed as exp(t - lse) from the kernel's own fp32 lse:  rho_bk = e_s[b, k] + e_lse[b] + u |t_k - lse_b| + a_e (relative)
  weights w = g P (one product; two of them and a sum in the ii block):  e_w = |g| P (rho + 3 u)
  dz      out_c = sum_x X_xc w_x accumulated over all n streamed rows (n = B, or 2 B for dzi with `both`) in one chain, then
          (acc - g other) inv_t:
              tol = inv_t [ sum_x |X_xc| e_w[x] + (n + 4) u (sum_x |X_xc w_x| + |g other_c|) ] + 2 u |dz_c|
``emulate_fp32`` walks the kernel's tiles in fp32 on the CPU; it stays inside half of every bound.
"""
import math

import torch

U = 2.0 ** -24

MISTAKES = ('ii_diagonal_kept', 'ij_diagonal_dropped', 'labels_on_ii_only', 'times_t', 'single_with_ii', 'dzj_no_pos', 'dzi_no_key_role',
            'lse_without_exclusions')


def keep_masks(B, both, labels=None, mistake=None):
    """(keep_ij, keep_ii) bool [B, B]: the logit set."""
    eye = torch.eye(B, dtype=torch.bool)
    same = eye.clone() if labels is None else labels.view(-1, 1) == labels.view(1, -1)
    keep_ij = ~(same & ~eye)
    keep_ii = ~(same | eye)
    if mistake == 'ii_diagonal_kept':
        keep_ii = ~(same & ~eye)
    if mistake == 'ij_diagonal_dropped' and labels is not None:
        keep_ij = ~same
    if mistake == 'labels_on_ii_only':
        keep_ij = torch.ones(B, B, dtype=torch.bool)
    if not both and mistake != 'single_with_ii':
        keep_ii = torch.zeros(B, B, dtype=torch.bool)
    return keep_ij, keep_ii


def rule(zi, zj, inv_t, both=True, labels=None, g=None, mistake=None):
    """-> dict(lse, pos [B]; with ``g`` also dzi, dzj [B, d]) in float64."""
    assert mistake is None or mistake in MISTAKES
    zi, zj = zi.detach().cpu().double(), zj.detach().cpu().double()
    labels = None if labels is None else labels.cpu()
    B = zi.shape[0]
    scale = 1.0 / float(inv_t) if mistake == 'times_t' else float(inv_t)
    s_ij, s_ii = (zi @ zj.T) * scale, (zi @ zi.T) * scale
    keep_ij, keep_ii = keep_masks(B, both, labels, mistake)
    neg_inf = torch.full((), float('-inf'), dtype=torch.float64)
    logits = torch.cat([torch.where(keep_ij, s_ij, neg_inf), torch.where(keep_ii, s_ii, neg_inf)], dim=1)
    m = logits.max(dim=1).values
    m = torch.where(torch.isfinite(m), m, torch.zeros_like(m))
    lse = m + torch.log(torch.exp(logits - m.unsqueeze(1)).sum(1))
    pos = s_ij.diagonal().clone()
    out = dict(lse=lse, pos=pos)
    if g is None:
        return out
    g = g.detach().cpu().double()
    lse_p = lse
    if mistake == 'lse_without_exclusions':
        full = torch.cat([s_ij, s_ii] if both else [s_ij], dim=1)
        lse_p = torch.logsumexp(full, dim=1)
    p_ij = torch.where(keep_ij, torch.exp(s_ij - lse_p.unsqueeze(1)), torch.zeros_like(s_ij))
    p_ii = torch.where(keep_ii, torch.exp(s_ii - lse_p.unsqueeze(1)), torch.zeros_like(s_ii))
    gi = g.unsqueeze(1)
    dzi = gi * (p_ij @ zj + p_ii @ zi - zj)
    if mistake != 'dzi_no_key_role':
        dzi = dzi + (gi * p_ii).T @ zi
    dzj = (gi * p_ij).T @ zi
    if mistake != 'dzj_no_pos':
        dzj = dzj - gi * zi
    out.update(dzi=dzi * scale, dzj=dzj * scale)
    return out


def loss(zi, zj, inv_t, both=True, labels=None):
    r = rule(zi, zj, inv_t, both, labels)
    return float((r['lse'] - r['pos']).mean())


# ---------------------------------------------------------------------------------------------------------------- bounds
def allowance(device='cpu'):
    """-> dict(exp = a_e relative, log = a_l absolute, measured = (exp, log)): twice what torch's own fp32 exp / log show on ``device``."""
    x = torch.linspace(-60.0, 0.0, 1 << 15, dtype=torch.float32)
    ex = torch.exp(x.double())
    m_e = float(((torch.exp(x.to(device)).double().cpu() - ex).abs() / ex).max())
    y = torch.logspace(0.0, math.log2(2.0 ** 18), 1 << 15, base=2.0, dtype=torch.float64).float()
    m_l = float((torch.log(y.to(device)).double().cpu() - torch.log(y.double())).abs().max())
    return dict(exp=2.0 * m_e, log=2.0 * m_l, measured=(m_e, m_l))


def judge(zi, zj, inv_t, both=True, labels=None, g=None, allow=None):
    """The float64 rule and the tolerance of every element: dict(lse, pos[, dzi, dzj], tol_lse, tol_pos[, tol_dzi, tol_dzj])."""
    allow = allow if allow is not None else allowance()
    a_e, a_l = allow['exp'], allow['log']
    out = rule(zi, zj, inv_t, both, labels, g)
    zi, zj = zi.detach().cpu().double(), zj.detach().cpu().double()
    labels = None if labels is None else labels.cpu()
    B, d = zi.shape
    inv_t = float(inv_t)
    s_ij, s_ii = (zi @ zj.T) * inv_t, (zi @ zi.T) * inv_t
    e_ij = inv_t * (d + 2) * U * (zi.abs() @ zj.abs().T) + U * s_ij.abs()
    e_ii = inv_t * (d + 2) * U * (zi.abs() @ zi.abs().T) + U * s_ii.abs()
    keep_ij, keep_ii = keep_masks(B, both, labels)
    keep = torch.cat([keep_ij, keep_ii], 1)
    t, e_s = torch.cat([s_ij, s_ii], 1), torch.cat([e_ij, e_ii], 1)
    lse = out['lse']
    P = torch.where(keep, torch.exp(t - lse.unsqueeze(1)), torch.zeros_like(t))
    big = torch.where(keep, t, torch.full_like(t, float('-inf'))).max(1).values
    small = torch.where(keep, t, torch.full_like(t, float('inf'))).min(1).values
    R = big - small
    NT = (2 if both else 1) * ((B + 31) // 32)
    rel = (P * (e_s + U * R.unsqueeze(1))).sum(1) + a_e + (17 * NT + 4) * U + (NT + 1) * (a_e + U * R + 2 * U)
    out['tol_lse'] = rel + a_l + 2 * U * lse.abs()
    out['tol_pos'] = e_ij.diagonal().clone()
    if g is None:
        return out
    g = g.detach().cpu().double()
    rho = e_s + out['tol_lse'].unsqueeze(1) + U * (t - lse.unsqueeze(1)).abs() + a_e + 3 * U
    W = g.unsqueeze(1) * P                                     # [B, 2B]: g_b P[b, k]
    E = g.abs().unsqueeze(1) * P * rho
    W_ij, W_ii, E_ij, E_ii = W[:, :B], W[:, B:], E[:, :B], E[:, B:]
    n_i = (2 if both else 1) * B
    acc_i = W_ij.abs() @ zj.abs() + (W_ii.abs() + W_ii.abs().T) @ zi.abs() + (g.unsqueeze(1) * zj).abs()
    out['tol_dzi'] = inv_t * (E_ij @ zj.abs() + (E_ii + E_ii.T) @ zi.abs() + (n_i + 4) * U * acc_i) + 2 * U * out['dzi'].abs()
    acc_j = W_ij.abs().T @ zi.abs() + (g.unsqueeze(1) * zi).abs()
    out['tol_dzj'] = inv_t * (E_ij.T @ zi.abs() + (B + 4) * U * acc_j) + 2 * U * out['dzj'].abs()
    return out


NAMES = ('lse', 'pos', 'dzi', 'dzj')


def shares(got, ref):
    """{name: max |got - ref| / tol} for the names both hold."""
    return {n: float(((got[n].detach().cpu().double() - ref[n]).abs() / ref['tol_' + n]).max()) for n in NAMES if n in got and n in ref}


# ---------------------------------------------------------------------------------------------------------------- fp32 emulation
def _row32(r, hh):
    return (r & 3) + 8 * (r >> 2) + 4 * hh


def emulate_fp32(zi, zj, inv_t, both=True, labels=None, g=None):
    """The kernel's tile order in fp32 on the CPU: 32 stationary rows against 32 streamed rows at a time; per (column, half) a running
    maximum and sum over its 16 entries of a tile, the halves merged at the end; the backward's weighted sums accumulated tile after
    tile in fp32.  -> dict(lse, pos[, dzi, dzj]) in fp32."""
    f = torch.float32
    zi, zj = zi.detach().cpu().to(f), zj.detach().cpu().to(f)
    B, d = zi.shape
    labels = None if labels is None else labels.cpu()
    keep_ij, keep_ii = keep_masks(B, both, labels)
    inv = torch.tensor(float(inv_t), dtype=f)
    halves = [torch.tensor([_row32(r, hh) for r in range(16)]) for hh in (0, 1)]
    m = torch.full((2, B), float('-inf'), dtype=f)
    l = torch.zeros(2, B, dtype=f)
    streams = [(zj, keep_ij)] + ([(zi, keep_ii)] if both else [])
    for X, keep in streams:
        for x0 in range(0, B, 32):
            T = (zi @ X[x0:x0 + 32].T) * inv                     # [B, <= 32]
            for hh in (0, 1):
                rows = halves[hh][halves[hh] + x0 < B]
                if not len(rows):
                    continue
                t, ok = T[:, rows], keep[:, x0 + rows]
                tmax = torch.where(ok, t, torch.full_like(t, float('-inf'))).max(1).values
                mn = torch.maximum(m[hh], tmax)
                live = mn > float('-inf')
                add = torch.zeros(B, dtype=f)
                for c in range(len(rows)):                        # the lane's own order
                    add = add + torch.where(ok[:, c] & live, torch.exp(t[:, c] - mn), torch.zeros(B, dtype=f))
                scale = torch.where(m[hh] > float('-inf'), torch.exp(m[hh] - mn), torch.zeros(B, dtype=f))
                l[hh] = torch.where(tmax > float('-inf'), l[hh] * scale + add, l[hh])
                m[hh] = torch.where(tmax > float('-inf'), mn, m[hh])
    mm = torch.maximum(m[0], m[1])
    parts = [torch.where(m[h] > float('-inf'), l[h] * torch.exp(m[h] - mm), torch.zeros(B, dtype=f)) for h in (0, 1)]
    lse = mm + torch.log(parts[0] + parts[1])
    out = dict(lse=lse, pos=((zi * zj).sum(1)) * inv)
    if g is None:
        return out
    g = g.detach().cpu().to(f)

    def stream(S, X, keep, row, key):
        acc = torch.zeros(B, d, dtype=f)
        for x0 in range(0, B, 32):
            t = (S @ X[x0:x0 + 32].T) * inv
            w = torch.zeros_like(t)
            if row:
                w = w + g.unsqueeze(1) * torch.exp(t - lse.unsqueeze(1))
            if key:
                w = w + g[x0:x0 + 32].unsqueeze(0) * torch.exp(t - lse[x0:x0 + 32].unsqueeze(0))
            acc = acc + torch.where(keep[:, x0:x0 + 32], w, torch.zeros_like(w)) @ X[x0:x0 + 32]
        return acc
    acc = stream(zi, zj, keep_ij, True, False)
    if both:
        acc = acc + stream(zi, zi, keep_ii, True, True)
    out['dzi'] = inv * (acc - g.unsqueeze(1) * zj)
    out['dzj'] = inv * (stream(zj, zi, keep_ij.T, False, True) - g.unsqueeze(1) * zi)
    return out
