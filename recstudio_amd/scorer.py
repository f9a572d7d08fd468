"""Score functions -- host-side mirror of ``recstudio.model.scorer`` (InnerProduct, Cosine).

``forward(query, items)`` keeps the reference's five shape cases and its dispatch
rule (recstudio/model/scorer.py:5-25, including the ``query.size(0) == items.size(0)``
quirk); the arithmetic runs in HIP.  Inside ``BaseRetriever`` the scorer objects act
as *selectors* for the fused kernel (no [B, n, d] tensor is ever built); calling them
directly scores already-materialised vectors through the same kernels.
"""
import os

import torch

from . import _native as nat
from . import ops

__all__ = ['InnerProductScorer', 'CosineScorer', 'EuclideanScorer']


class _RowScoreFn(torch.autograd.Function):
    """scores of materialised item vectors [M, n, d] against queries [M, d] through the gather+score
    kernel (the vectors are addressed as rows 0..M*n-1 of a table).  The backward of this
    compatibility path is two broadcast products in torch."""

    @staticmethod
    def forward(ctx, q2, rows, n, cosine):
        ids = torch.arange(rows.shape[0], device=rows.device, dtype=torch.int64)
        out = ops.fused_forward(rows, q2, n, neg_ids=ids, sampler=nat.SAMPLER_GIVEN, cosine=cosine,
                                n_queries=q2.shape[0])['neg_score']
        ctx.save_for_backward(q2, rows)
        ctx.n, ctx.cosine = n, cosine
        return out

    @staticmethod
    def backward(ctx, g):
        q2, rows = ctx.saved_tensors
        M, d = q2.shape
        ids = torch.arange(rows.shape[0], device=rows.device, dtype=torch.int64).view(M, ctx.n)
        _, grows, gq = ops.fused_backward(rows, q2, ids, g.reshape(M, ctx.n).contiguous(), dense_item_grad=False,
                                          row_item_grad=True, want_query_grad=True, item_pad_row=-1,
                                          cosine=ctx.cosine)
        # row-sparse layout is [M, 1 + n, d] with an (unused) positive slot per query
        gr = grows.view(M, ctx.n + 1, d)[:, 1:].reshape(-1, d)
        return (gq if ctx.needs_input_grad[0] else None), (gr if ctx.needs_input_grad[1] else None), None, None


class InnerProductScorer(torch.nn.Module):
    cosine = False

    def forward(self, query, items):
        if query.size(0) == items.size(0):
            if query.dim() < items.dim():                 # ([B,D],[B,n,D]) / ([B,L,D],[B,L,n,D])
                n = items.shape[-2]
                lead = items.shape[:-2]
            else:                                         # ([B,D],[B,D]) / ([B,L,D],[B,L,D])
                n = 1
                lead = items.shape[:-1]
            d = items.shape[-1]
            out = _RowScoreFn.apply(query.reshape(-1, d).contiguous(), items.reshape(-1, d).contiguous(), n,
                                    self.cosine)
            return out.view(*lead, n) if query.dim() < items.dim() else out.view(*lead)
        # ([B,D],[N,D]): full-catalog scores
        return full_scores(query, items, self.cosine)


class CosineScorer(InnerProductScorer):
    cosine = True


class EuclideanScorer(InnerProductScorer):
    """recstudio/model/scorer.py:28-34: -(|items|^2 + |query|^2 - 2 <query, items>)."""
    cosine = nat.SCORE_EUC      # the `cosine` slot carries the rsa_score_mode


class NormScorer(EuclideanScorer):
    """recstudio/model/scorer.py:56-66 for p = 2: -||query - items||_2, evaluated as -sqrt of the Euclidean mode of
    the gather+score kernel (|q|^2 + |x|^2 - 2 <q, x>, clamped at 0); gradients flow through that kernel's backward."""

    def __init__(self, p=2):
        super().__init__()
        if p != 2:
            raise NotImplementedError('NormScorer: only p = 2 maps onto the dot-product kernels')
        self.p = p

    def forward(self, query, items):
        return -torch.sqrt(torch.clamp(-super().forward(query, items), min=0.0))


class GMFScorer(InnerProductScorer):
    """recstudio/model/scorer.py:69-86: act(W (query * item) + b) = act(<query * w, item> + b) -- the learned
    weights fold into the query, so scoring (and its backward) is the inner-product kernel."""

    def __init__(self, emb_dim, bias=False, activation='relu'):
        super().__init__()
        self.emb_dim = emb_dim
        self.W = torch.nn.Linear(emb_dim, 1, bias=bias)
        acts = {'relu': torch.relu, 'sigmoid': torch.sigmoid, 'tanh': torch.tanh, 'identity': lambda x: x,
                'gelu': torch.nn.functional.gelu, 'leakyrelu': torch.nn.functional.leaky_relu}
        if activation not in acts:
            raise ValueError(f'GMFScorer: unknown activation {activation!r}')
        self.activation = acts[activation]

    def forward(self, query, key):
        assert query.dim() <= key.dim(), 'query dim must be smaller than or euqal to key dim'
        s = super().forward(query * self.W.weight.view(-1), key)
        if self.W.bias is not None:
            s = s + self.W.bias
        return self.activation(s)


class _FullScoreFn(torch.autograd.Function):
    """[B, N] scores of every query against every item with the fp32-MFMA kernel (inner product, or cosine /
    Euclidean applied in the tile epilogue); the backward GEMMs of this MATERIALISED compatibility path are plain
    library GEMMs (rocBLAS through torch.matmul) plus, for cosine / Euclidean, the chain rule of the norms."""

    @staticmethod
    def forward(ctx, query, items, mode):
        ctx.mode = mode
        out = ops.fullscore(items, query, want_scores=True, items_without_pad=True, score_mode=mode)[0]
        ctx.save_for_backward(query, items, out if mode == nat.SCORE_COS else None)
        return out

    @staticmethod
    def backward(ctx, g):
        query, items, out = ctx.saved_tensors
        need_q, need_i = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if ctx.mode == nat.SCORE_IP:
            return (g @ items if need_q else None), (g.t() @ query if need_i else None), None
        if ctx.mode == nat.SCORE_EUC:        # s = 2 q.x - |x|^2 - |q|^2
            gq = 2.0 * (g @ items - g.sum(1, keepdim=True) * query) if need_q else None
            gi = 2.0 * (g.t() @ query - g.sum(0).unsqueeze(1) * items) if need_i else None
            return gq, gi, None
        # cosine: s = q.x / (|q||x|);  ds/dq = x / (|q||x|) - s q / |q|^2  (and symmetrically for x)
        qn, xn = query.norm(dim=1, keepdim=True), items.norm(dim=1, keepdim=True)
        gs = g * out
        gq = ((g / xn.t()) @ items / qn - gs.sum(1, keepdim=True) * query / (qn * qn)) if need_q else None
        gi = ((g / qn).t() @ query / xn - gs.sum(0).unsqueeze(1) * items / (xn * xn)) if need_i else None
        return gq, gi, None


def full_scores(query, items, cosine=False):
    """([B,D],[N,D]) case of the scorers (scorer.py:16, :19-25, :28-34): items has no padding row here."""
    return _FullScoreFn.apply(query, items.contiguous(), ops._score_mode(cosine))


# Full-catalog logsumexp under autograd, three forms (RSA_FULL_SOFTMAX_BACKWARD):
#   'flash' (default)  the forward is the FLASH pass: logsumexp AND d lse/d query = softmax @ items from one walk over the catalog
#                      (rsa_fullscore_lse_grad); the backward multiplies that [B, d] block by the upstream gradient and runs ONE
#                      item-stationary recompute pass for d/d items (rsa_fullscore_softmax_dw).  Four GEMMs of 2 B N d flop per
#                      training step, 8 N d bytes of HBM traffic per pass, NO [B, N] matrix at any batch size.
#   'recompute'        lse-only forward; d/d query from a query-stationary recompute pass (softmax tile not written), d/d items as
#                      above: five GEMMs, no [B, N] either (what runs when the query needs no gradient costs one GEMM less).
#   'store'            the round-5 form: the recompute pass writes the scaled softmax once ([B, N-1] fp32: 8 GB at B = 2048,
#                      N = 1e6, written and read back) and d/d items is a GEMM over it -- four GEMMs + 16 GB of traffic.
FULL_SOFTMAX_BACKWARD = os.environ.get('RSA_FULL_SOFTMAX_BACKWARD', 'flash')


class _FullLseFn(torch.autograd.Function):
    """logsumexp_i <query_b, weight_i> over item rows 1..N-1 WITHOUT writing [B, N], forward and backward (the reference:
    loss_func.py:39-47 over the scorer.py:16 matmul, under autograd) -- see FULL_SOFTMAX_BACKWARD."""

    @staticmethod
    def forward(ctx, query, weight):
        ctx.mode = FULL_SOFTMAX_BACKWARD if weight.shape[1] <= 128 else 'store'
        gq_unit = None
        if ctx.mode == 'flash' and ctx.needs_input_grad[0]:
            lse, gq_unit = ops.fullscore_lse_grad(weight, query)
        else:
            lse = ops.fullscore(weight, query, want_lse=True)[1]
        ctx.save_for_backward(query, weight, lse, gq_unit)
        return lse

    @staticmethod
    def backward(ctx, g):
        query, weight, lse, gq_unit = ctx.saved_tensors
        need_q, need_w = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        g = g.contiguous()
        if ctx.mode == 'store':
            return _full_lse_backward_stored(query, weight, lse, g, need_q, need_w)
        gq = None
        if need_q:
            gq = g.unsqueeze(1) * gq_unit if gq_unit is not None else \
                ops.fullscore_softmax(weight, query, lse, g, want_query_grad=True, want_probs=False)[1]
        gw = ops.fullscore_softmax_dw(weight, query, lse, g, out=torch.empty_like(weight)) if need_w else None
        return gq, gw


def _full_lse_backward_stored(query, weight, lse, g, need_q, need_w):
    """the round-5 backward: one [B, N-1] write of the scaled softmax (+ d/d query in the same pass), d/d items = probs^T query"""
    if need_q:     # d/d query leaves the recompute pass itself (second MFMA product per tile)
        probs, gq = ops.fullscore_softmax(weight, query, lse, g, want_query_grad=True)
    else:
        probs, gq = ops.fullscore_softmax(weight, query, lse, g), None
    gw = None
    if need_w:
        gw = torch.empty_like(weight)
        gw[0].zero_()
        if weight.shape[1] <= 128:         # in-tree item-stationary MFMA kernel (rounds 1-4: torch.matmul -> rocBLAS)
            ops.probs_t_query(probs, query, out=gw[1:])
        else:
            torch.matmul(probs.t(), query, out=gw[1:])
    return gq, gw


def full_lse(query, item_weight):
    """logsumexp over the whole catalog of <query, item> (padding row 0 excluded), differentiable."""
    return _FullLseFn.apply(query.contiguous(), item_weight)
