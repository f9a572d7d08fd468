"""Float64 referee of rsa_graph_dropout, of the propagation over thinned graphs (one matrix for all layers, or one per layer)
and of one SGL training step.  Test code only: nothing here calls recstudio_amd.  Runs on whatever device its tensors live on.

THE RULE (sgl.py:34-114, data_augmentation.py:229-450 on the dgl branch, graphmodule.py:176-188 with norm 'both'): a view keeps a
subset of the DIRECTED edges of the bidirectional interaction graph; with in_deg(r) the kept edges of row (destination) r and
out_deg(c) the kept edges with source c,

    values[e]   = keep[e] ? fp32(out_deg(c_e)^-1/2 * in_deg(r_e)^-1/2)  (the product in float64, rounded once) : 0
    t_values[e] = values[rev[e]]                        the transposed thinned matrix in the same CSR layout

The propagation bound is tests/spmm_referee.py's, (K + 2) u |s_r| sum |v_e x| per layer with K the BASE row length (the kernel
adds the zero products of the dropped edges too), carried through the layers.  ``mistake`` plants one bug for the tests of the
bounds.  dgl is not installed where this project is developed: the referee is pinned to the rule the source spells out.
"""
import torch
import torch.nn.functional as F

import spmm_referee as sr

U32 = sr.U32


def augment(indptr, indices, rev, keep, mistake=None, keep_prob=None):
    """-> dict(in_deg, out_deg int64 [n], values, t_values fp32 [nnz]) for the mask ``keep`` (bool [nnz]).  Mistakes:
      'base_degrees'  the degrees of the unthinned graph
      'rev_keep'      the forward value masked by keep[rev[e]]
      't_is_values'   t_values = values (backward through A' instead of its transpose)
      'inv_keep_prob' the 1 / keep_prob factor of the reference's COO branch"""
    n = indptr.numel() - 1
    keep = keep.bool()
    rows, cols = sr.edge_rows(indptr), indices.long()
    in_deg = torch.bincount(rows[keep], minlength=n)
    out_deg = torch.bincount(cols[keep], minlength=n)
    di, do = (torch.bincount(rows, minlength=n), torch.bincount(cols, minlength=n)) if mistake == 'base_degrees' else (in_deg, out_deg)
    norm = lambda d: torch.where(d > 0, d.double().pow(-0.5), torch.zeros(n, dtype=torch.float64, device=d.device))      # noqa: E731
    w = norm(do)[cols] * norm(di)[rows]
    if mistake == 'inv_keep_prob':
        w = w / keep_prob
    mask = keep[rev] if mistake == 'rev_keep' else keep
    values = torch.where(mask, w, torch.zeros_like(w)).float()
    t_values = values.clone() if mistake == 't_is_values' else values[rev]
    return {'in_deg': in_deg, 'out_deg': out_deg, 'values': values, 't_values': t_values}


def propagate_each(indptr, indices, values_per_layer, e0):
    """mean(E_0 .. E_L) with E_k = A_k E_{k-1} in float64 and the bound of an fp32 implementation that keeps E_k and the running
    sum in fp32 (spmm_referee.propagate with one weight array per layer).  -> (mean, tol) float64 [n, d]."""
    L = len(values_per_layer)
    e = e0.double()
    s, t, ts = e.clone(), torch.zeros_like(e), torch.zeros_like(e)
    K2 = ((indptr[1:] - indptr[:-1]).double() + 2.0).unsqueeze(1) * U32
    for k, values in enumerate(values_per_layer):
        absv = values.abs()
        carried = sr.referee(indptr, indices, absv, t)['y']
        local = K2 * sr.referee(indptr, indices, absv, e.abs() + t)['y']
        e = sr.referee(indptr, indices, values, e)['y']
        t = carried + local
        s = s + e
        ts = ts + t + (3.0 if k == L - 1 else 1.0) * U32 * s.abs()
    return s / (L + 1), ts / (L + 1)


def horner_each(indptr, indices, t_values_per_layer, g, mistake=None):
    """The gradient of ``propagate_each``'s mean for the incoming gradient g: (g + A_1^T (g + A_2^T (... A_L^T g))) / (L + 1), run
    as h <- g + A_k^T h from k = L down to 1, and its bound: a step costs the product's (K + 2) u |A^T| (|h| + t) on top of the
    carried |A^T| t, and two roundings of the result (three on the last: the constant 1 / (L + 1) is rounded to fp32 as well).
    ``mistake='up'``: the recurrence run from layer 1 up.  -> (grad, tol)."""
    L = len(t_values_per_layer)
    g = g.double()
    h, t = g.clone(), torch.zeros_like(g)
    K2 = ((indptr[1:] - indptr[:-1]).double() + 2.0).unsqueeze(1) * U32
    order = range(L) if mistake == 'up' else range(L - 1, -1, -1)
    for j, k in enumerate(order):
        values = t_values_per_layer[k]
        absv = values.abs()
        scale = 1.0 / (L + 1) if j == L - 1 else 1.0
        carried = sr.referee(indptr, indices, absv, t)['y']
        local = K2 * sr.referee(indptr, indices, absv, h.abs() + t)['y']
        h = scale * (g + sr.referee(indptr, indices, values, h)['y'])
        t = scale * (carried + local) + (3.0 if j == L - 1 else 2.0) * U32 * h.abs()
    return h, t


def thinned_dense(src, dst, n):
    """The thinned, normalised matrix [n, n] (row = destination) from its kept DIRECTED edges src -> dst by way of
    ``spmm_referee.dense_norm_adj``: on the bipartite graph whose 'users' are the n nodes as sources and whose 'items' are the n
    nodes as destinations, a user's degree is its out-degree and an item's its in-degree, so the item x user block of that
    graph's normalised adjacency is in_deg(dst)^-1/2 * count * out_deg(src)^-1/2."""
    return sr.dense_norm_adj(src, dst, n, n)[n:, :n]


def info_nce(rep_i, rep_j, table, temperature, sim_method, mistake=None):
    """data_augmentation.py:378-398 in the dtype of its inputs: ``table`` is the WHOLE table, its padding row 0 is no negative.
    Mistakes: 'row0' (row 0 among the negatives), 'raw_table' (the table left unnormalised under 'cosine'), 'one_temperature' (the
    temperature on the logsumexp term only)."""
    reps = table if mistake == 'row0' else table[1:]
    if sim_method == 'cosine':
        rep_i, rep_j = F.normalize(rep_i, p=2, dim=-1), F.normalize(rep_j, p=2, dim=-1)
        if mistake != 'raw_table':
            reps = F.normalize(reps, p=2, dim=-1)
    sim_ij = rep_i @ reps.t() / temperature
    sim_ii = (rep_i * rep_j).sum(-1) / (1.0 if mistake == 'one_temperature' else temperature)
    return torch.mean(torch.logsumexp(sim_ij, dim=-1) - sim_ii)


def _mean_layers(mats, e):
    s = e
    for a in mats:
        e = a @ e
        s = s + e
    return s / (len(mats) + 1)


def sgl_step(user_emb, item_emb, adj, views, n_layers, uid, pos, neg, l2_reg_weight, ssl_reg, temperature, mistake=None):
    """One SGL training step in dense float64 torch: spmm_referee.lightgcn_step's loss over ``adj`` (dense [n, n]) plus
    ssl_reg * (InfoNCE of the users + InfoNCE of the items) between the two ``views`` -- each a dense [n, n] matrix or a list of
    n_layers of them (RW).  -> dict(loss, user_grad, item_grad, cl_loss)."""
    ue = user_emb.detach().double().clone().requires_grad_(True)
    ie = item_emb.detach().double().clone().requires_grad_(True)
    nu = ue.shape[0]
    e = torch.cat([ue, ie], 0)
    s = _mean_layers([adj] * int(n_layers), e)
    users, items = s[:nu], s[nu:]
    q = users[uid]
    pos_score = (q * items[pos]).sum(-1)
    neg_score = (q.unsqueeze(1) * items[neg]).sum(-1)
    w = torch.softmax(torch.ones_like(neg_score), -1)
    bpr = -torch.mean((F.logsigmoid(pos_score.view(-1, 1) - neg_score) * w).sum(-1))
    loss = bpr + l2_reg_weight * sr.l2_reg(ue[uid], ie[pos], ie[neg.reshape(-1)])
    tabs = [_mean_layers(v if isinstance(v, (list, tuple)) else [v] * int(n_layers), e) for v in views]
    (u1, i1), (u2, i2) = ((t[:nu], t[nu:]) for t in tabs)
    cl = info_nce(u1[uid], u2[uid], u2, temperature, 'cosine', mistake) + info_nce(i1[pos], i2[pos], i2, temperature, 'cosine', mistake)
    loss = loss + ssl_reg * cl
    loss.backward()
    return {'loss': loss.detach(), 'user_grad': ue.grad, 'item_grad': ie.grad, 'cl_loss': cl.detach()}
