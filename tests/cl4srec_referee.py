"""Float64 restatement of one CL4SRec training step (retriever.CL4SRec: recstudio/model/seq/cl4srec.py:48-53,
recstudio/model/module/data_augmentation.py:591-606) with dropout 0, on given negatives and given views: the SASRec tower (the
gather with the mask token as the encoder's own row, learned positions, post-norm transformer layers), last-position pooling and BCE
for the main pass; for each view the tower without pooling, the mean over its first ``new_len`` positions, and the in-batch InfoNCE
('inner_product', 'batch_both') by the explicit rule of tests/batch_infonce_referee.py's logit set, here under autograd in float64.
The views themselves come from tests/seq_augment_referee.py fed the uniforms the run consumed."""
import copy

import torch
import torch.nn.functional as F

import oracle
import seq_attention_referee as sr
import seq_augment_referee as sa
import batch_infonce_referee as br


def tower(e, w, ids, mask_id, causal=True):
    """``e``: a float64 CPU copy of the SASRecQueryEncoder; ``w`` the float64 item table -> [B, L, D].  An id equal to ``mask_id``
    takes ``e.mask_emb`` and is attended; padding is ``ids == 0``."""
    B, L = ids.shape
    masked = ids == mask_id
    rows = F.embedding(torch.where(masked, torch.zeros_like(ids), ids), w, padding_idx=0)
    if masked.any():
        rows = rows + masked.unsqueeze(-1).double() * e.mask_emb
    x = rows + e.position_emb.weight[:L].unsqueeze(0)
    pad = ids == 0
    for layer in e.transformer_layer.layers:
        mha = layer.self_attn
        H = mha.num_heads
        qh, kh, vh = sr.split(F.linear(x, mha.in_proj_weight, mha.in_proj_bias), H)
        s = (qh @ kh.transpose(2, 3)) * (qh.shape[-1] ** -0.5)
        ok = sr.allowed(pad, causal, B, L).expand(B, H, L, L)
        pr = torch.softmax(s.masked_fill(~ok, float('-inf')), dim=3)
        pr = torch.where(ok.any(3, keepdim=True), pr, torch.zeros_like(pr))      # a query without keys: zeros, not NaN
        a = (pr @ vh).transpose(1, 2).reshape(B, L, -1)
        x = layer.norm1(x + mha.out_proj(a))
        x = layer.norm2(x + layer.linear2(F.gelu(layer.linear1(x))))
    return x


def mean_pool(out, ln):
    keep = (torch.arange(out.shape[1]).unsqueeze(0) < ln.unsqueeze(1)).unsqueeze(-1).double()
    return (out * keep).sum(1) / ln.unsqueeze(-1).double()


def infonce(zi, zj, inv_t, both=True, labels=None):
    """mean(lse - pos) over the logit set of batch_infonce_referee.keep_masks, under autograd."""
    keep_ij, keep_ii = br.keep_masks(zi.shape[0], both, labels)
    neg_inf = torch.full((), float('-inf'), dtype=torch.float64)
    s_ij, s_ii = (zi @ zj.T) * inv_t, (zi @ zi.T) * inv_t
    logits = torch.cat([torch.where(keep_ij, s_ij, neg_inf), torch.where(keep_ii, s_ii, neg_inf)], dim=1)
    return (torch.logsumexp(logits, dim=1) - s_ij.diagonal()).mean()


def replay_views(hist, seqlen, kinds, rates, uniforms, mask_id):
    """The two views through the per-sequence referee: ``kinds`` / ``rates`` / ``uniforms`` one entry per view."""
    L = hist.shape[1]
    views = []
    for kind, rate, U in zip(kinds, rates, uniforms):
        out, new_len = sa.augment(hist.cpu().numpy(), seqlen.cpu().numpy(), kind, sa.sub_lengths(kind, rate, L), U.cpu().numpy(), mask_id)
        views.append((torch.from_numpy(out), torch.from_numpy(new_len)))
    return views


def step(item_w, enc, hist, seqlen, pos, neg, views, mask_id, temperature, cl_weight, causal=True):
    """-> (loss, main loss, cl loss, {encoder parameter name: gradient}, item-table gradient), all float64 on the CPU."""
    e = copy.deepcopy(enc).cpu().double()
    e.item_encoder = None
    w = item_w.detach().cpu().double().requires_grad_(True)
    hist, seqlen, pos, neg = hist.cpu(), seqlen.cpu(), pos.cpu(), neg.cpu()
    x = tower(e, w, hist, mask_id, causal)
    query = x.gather(1, (seqlen - 1).clamp(min=0).view(-1, 1, 1).expand(-1, 1, x.shape[-1])).squeeze(1)
    ps = (query * F.embedding(pos, w)).sum(-1)
    ns = (query.unsqueeze(1) * F.embedding(neg, w)).sum(-1)
    main = oracle.bce_loss(ps, ns)
    reps = [mean_pool(tower(e, w, ids, mask_id, causal), ln) for ids, ln in views]
    cl = infonce(reps[0], reps[1], 1.0 / temperature)
    loss = main + cl_weight * cl
    loss.backward()
    grads = {n: p.grad for n, p in e.named_parameters() if p.grad is not None}
    return loss.item(), main.item(), cl.item(), grads, w.grad
