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
from . import ops, rng

__all__ = ['InnerProductScorer', 'CosineScorer', 'EuclideanScorer', 'MLPScorer', 'FusionMFMLPScorer']


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


# ------------------------------------------------------------------ NCF's pair scorers
PAIR_MLP_RANGE_CHUNK = 4096          # items per range-mode launch of the ([B, D], [N, D]) case


def _plain_relu_mlp(mlp):
    """(the Linear layers, the dropout probability) of an ``MLPModule`` that is Dropout / Linear(bias) / ReLU per layer and nothing
    else -- what ``pair_mlp_torch`` and the kernel evaluate --, or None."""
    seq = getattr(mlp, 'model', None)
    if not isinstance(seq, torch.nn.Sequential) or len(seq) == 0 or len(seq) % 3:
        return None
    linears = []
    for drop, lin, act in zip(seq[0::3], seq[1::3], seq[2::3]):
        if not (isinstance(drop, torch.nn.Dropout) and isinstance(lin, torch.nn.Linear) and lin.bias is not None
                and isinstance(act, torch.nn.ReLU)):
            return None
        linears.append(lin)
    return linears, float(seq[0].p)


def pair_mlp_torch(query, items, hidden, w_h, *, w_mf=None, b_out=None, p=0.0, u=None):
    """The reference's op sequence for one score per row (scorer.py:37-56 / :92-113 over MLPModule), with an EXPLICIT uniform
    tensor in place of nn.Dropout: ``query``, ``items`` [M, d] (already broadcast against each other), ``hidden`` the ``(W, b)``
    of the hidden layers, ``w_h`` the H_K output weights, and ``w_mf`` [d] (FusionMFMLPScorer) or ``b_out`` (MLPScorer).  ``u``
    [M, C] (``ops.pair_mlp_masked_columns``): column c of the masked columns is kept iff ``u[:, c] < fp32(1 - p)`` and divided by
    it -- the rule of ``ops.pair_mlp``, so one ``torch.rand`` replays the kernel's mask.  Any dtype; this is the CPU path, the
    fallback and the parity twin."""
    q = torch.tensor(1.0 - float(p), dtype=torch.float32).to(query.dtype)
    at = 0

    def drop(h):
        nonlocal at
        if p == 0.0:
            return h
        keep = u[:, at:at + h.shape[1]] < q.to(u.dtype)
        at += h.shape[1]
        return torch.where(keep, h / q, torch.zeros_like(h))

    h = drop(torch.cat([query, items], dim=-1))
    for k, (w, b) in enumerate(hidden):
        h = torch.relu(torch.nn.functional.linear(h, w, b))
        if k + 1 < len(hidden) or b_out is not None:
            h = drop(h)
    if w_mf is not None:
        return torch.relu((query * items) @ w_mf.reshape(-1) + h @ w_h.reshape(-1))
    return torch.relu(h @ w_h.reshape(-1) + b_out.reshape(()))


class _PairMlpFn(torch.autograd.Function):
    """scores [M, S] of ``ops.pair_mlp`` under autograd.  cfg: ``p``, ``mask_slot0``, ``fusion``, ``sparse_grad``, ``rows`` (the table
    is the pairs' own materialised rows: its gradient is ``drows`` as it stands).  The item rows' gradients reach the table through
    the sorted row scatter the gather+score kernel's rows take (``fused._ScoreFn``) at the widths it serves, d = 64 and 128; at
    d = 32 they go through ``ops.scatter_add_rows``, whose float atomics make a DENSE table gradient with repeated ids the one
    output of this node that is not bit-equal from run to run (``train.sparse_grad`` has no such sum)."""

    @staticmethod
    def forward(ctx, query, table, ids, cfg, w1, b1, w2, b2, w_out, b_out):
        d = table.shape[1]
        hidden = [w1.shape[0]] + ([w2.shape[0]] if w2 is not None else [])
        philox = None
        if cfg['p'] != 0.0:
            C = ops.pair_mlp_masked_columns(d, hidden, 'fusion' if cfg['fusion'] else 'mlp')
            philox = rng.reserve(ids.numel() * C, 4, query.device)
        ctx.cfg, ctx.philox = cfg, philox
        ctx.save_for_backward(query, table, ids, w1, b1, w2, b2, w_out, b_out)
        return ops.pair_mlp(query, table, ids, w1, b1, w2, b2, **_PairMlpFn._tail(cfg, w_out, b_out, d), p=cfg['p'],
                            philox=philox, mask_slot0=cfg['mask_slot0'])

    @staticmethod
    def _tail(cfg, w_out, b_out, d):
        if cfg['fusion']:
            return {'w_h': w_out[0, d:], 'w_mf': w_out[0, :d]}
        return {'w_h': w_out[0], 'b_out': b_out}

    @staticmethod
    def backward(ctx, g):
        query, table, ids, w1, b1, w2, b2, w_out, b_out = ctx.saved_tensors
        cfg, d = ctx.cfg, table.shape[1]
        dq, drows, gr = ops.pair_mlp_backward(query, table, ids, w1, b1, w2, b2, g=g.contiguous(),
                                              **_PairMlpFn._tail(cfg, w_out, b_out, d), p=cfg['p'], philox=ctx.philox,
                                              mask_slot0=cfg['mask_slot0'])
        g_table = None
        if ctx.needs_input_grad[1]:
            rows = drows.view(-1, d)
            if cfg.get('rows'):
                g_table = rows
            elif cfg.get('sparse_grad'):
                g_table = torch.sparse_coo_tensor(ids.reshape(1, -1), rows * (ids.reshape(-1, 1) != 0), table.shape)
            elif d in (64, 128, 256):
                g_table = ops.scatter_rows_sorted(torch.zeros_like(table), rows, ids.reshape(-1, 1),
                                                  torch.ones(rows.shape[0], 1, dtype=torch.float32, device=rows.device), pad_row=0)
            else:
                g_table = ops.scatter_add_rows(rows, ids.reshape(-1), table.shape[0])
        g_out = torch.cat([gr['w_mf'], gr['w_h']]).view(1, -1) if cfg['fusion'] else gr['w_h'].view(1, -1)
        return (dq if ctx.needs_input_grad[0] else None, g_table, None, None, gr['w1'], gr['b1'], gr.get('w2'), gr.get('b2'),
                g_out, gr.get('b_out'))


class _PairScorer(torch.nn.Module):
    """What MLPScorer and FusionMFMLPScorer share: the reference's five shape cases (scorer.py:42-56, :102-109) over one
    score-per-pair rule.  ``self.fused`` (a plain attribute, OFF unless set: the rule of ``models_mf.FUSED_SCORER_DEFAULT``) lets
    the HIP kernel run where ``ops.pair_mlp_kernel_ok`` accepts the tensors; everything else -- CPU tensors, another activation,
    batch norm, more than two hidden layers -- runs the torch ops."""
    fused = False

    def _parts(self):
        """(hidden Linear layers, p, output weight, output bias or None, fusion?) when the scorer is a plain relu MLP, else None."""
        raise NotImplementedError

    def _torch_scores(self, query, items):
        """the reference's own modules on materialised, broadcast [..., d] tensors"""
        raise NotImplementedError

    def _kernel_parts(self, query, table):
        parts = self._parts()
        if parts is None or not self.fused:
            return None
        hidden = [lin.out_features for lin in parts[0]]
        return parts if ops.pair_mlp_kernel_ok(query, table, hidden) else None

    def _p(self, parts):
        return parts[1] if self.training else 0.0

    def _fn_args(self, parts):
        lin, _, w_out, b_out, _ = parts
        w2, b2 = (lin[1].weight, lin[1].bias) if len(lin) > 1 else (None, None)
        return lin[0].weight, lin[0].bias, w2, b2, w_out, b_out

    def score_ids(self, query, table, ids, mask_slot0=False, sparse_grad=False):
        """scores [M, S] of the queries [M, d] against the rows ``ids`` [M, S] of ``table`` through the kernel (no [M, S, d] tensor);
        None when the kernel does not serve this scorer or these tensors."""
        parts = self._kernel_parts(query, table)
        if parts is None:
            return None
        cfg = {'p': self._p(parts), 'mask_slot0': bool(mask_slot0), 'fusion': parts[4], 'sparse_grad': sparse_grad}
        return _PairMlpFn.apply(query.contiguous(), table, ids.contiguous(), cfg, *self._fn_args(parts))

    def score_range(self, query, table, c0, count):
        """scores [B, count] of every query against rows c0 .. c0 + count - 1 of ``table``: the kernel's range mode, no autograd."""
        lin, _, w_out, b_out, fusion = self._parts()
        w1, b1, w2, b2, _, _ = self._fn_args((lin, 0.0, w_out, b_out, fusion))
        with torch.no_grad():
            return ops.pair_mlp(query.contiguous(), table, None, w1, b1, w2, b2, item_range=(c0, count),
                                **_PairMlpFn._tail({'fusion': fusion}, w_out, b_out, table.shape[1]))

    def forward(self, query, items):
        assert query.dim() <= items.dim(), 'query dim must be smaller than or euqal to key dim'
        d = items.shape[-1]
        if query.size(0) != items.size(0):                     # ([B, D], [N, D])
            need_grad = torch.is_grad_enabled() and (query.requires_grad or items.requires_grad
                                                     or any(p.requires_grad for p in self.parameters()))
            if not (need_grad or self.training) and self._kernel_parts(query, items) is not None:
                out = torch.empty(query.shape[0], items.shape[0], dtype=torch.float32, device=query.device)
                for c0 in range(0, items.shape[0], PAIR_MLP_RANGE_CHUNK):
                    c = min(PAIR_MLP_RANGE_CHUNK, items.shape[0] - c0)
                    out[:, c0:c0 + c] = self.score_range(query, items, c0, c)
                return out
            B, N = query.shape[0], items.shape[0]
            return self._flat_scores(query.unsqueeze(1).expand(B, N, d), items.unsqueeze(0).expand(B, N, d))
        if query.dim() < items.dim():                          # ([B, D], [B, n, D]) / ([B, L, D], [B, L, n, D])
            n = items.shape[-2]
            if self._kernel_parts(query, items.reshape(-1, d)) is not None:
                rows = items.reshape(-1, d).contiguous()
                ids = torch.arange(rows.shape[0], device=rows.device).view(-1, n)
                return self._rows_scores(query.reshape(-1, d), rows, ids).view(items.shape[:-1])
            return self._flat_scores(query.unsqueeze(-2).expand_as(items), items)
        if self._kernel_parts(query, items.reshape(-1, d)) is not None:      # ([B, D], [B, D]) / ([B, L, D], [B, L, D])
            rows = items.reshape(-1, d).contiguous()
            ids = torch.arange(rows.shape[0], device=rows.device).view(-1, 1)
            return self._rows_scores(query.reshape(-1, d), rows, ids).view(items.shape[:-1])
        return self._flat_scores(query, items)

    def _rows_scores(self, q2, rows, ids):
        parts = self._kernel_parts(q2, rows)
        cfg = {'p': self._p(parts), 'mask_slot0': False, 'fusion': parts[4], 'rows': True}
        return _PairMlpFn.apply(q2.contiguous(), rows, ids, cfg, *self._fn_args(parts))

    def _flat_scores(self, query, items):
        """torch ops over broadcast tensors of one shape [..., d] -> [...]"""
        parts = self._parts()
        if parts is None:
            return self._torch_scores(query, items)
        lin, p, w_out, b_out, fusion = parts
        d = items.shape[-1]
        q2, x2 = query.reshape(-1, d), items.reshape(-1, d)
        p = self._p(parts)
        hidden = [l.out_features for l in lin]
        u = None
        if p != 0.0:
            u = torch.rand(q2.shape[0], ops.pair_mlp_masked_columns(d, hidden, 'fusion' if fusion else 'mlp'), device=q2.device)
        tail = {'w_h': w_out[0, d:], 'w_mf': w_out[0, :d]} if fusion else {'w_h': w_out[0], 'b_out': b_out}
        return pair_mlp_torch(q2, x2, [(l.weight, l.bias) for l in lin], p=p, u=u, **tail).view(items.shape[:-1])


class MLPScorer(_PairScorer):
    """recstudio/model/scorer.py:37-56: ``transform(cat(query, items))`` with ``transform`` an ``MLPModule`` over
    ``[2d] + hidden + [1]`` (state_dict ``trans.model.1.weight`` ...).  Dropout masks follow ``torch.rand`` (one call per scorer
    call), not nn.Dropout's kernel."""

    def __init__(self, transform):
        super().__init__()
        self.trans = transform

    def _parts(self):
        got = _plain_relu_mlp(self.trans)
        if got is None or len(got[0]) < 2 or got[0][-1].out_features != 1:
            return None
        lin, p = got
        return lin[:-1], p, lin[-1].weight, lin[-1].bias, False

    def _torch_scores(self, query, items):
        return self.trans(torch.cat((query, items), dim=-1)).squeeze(-1)


class FusionMFMLPScorer(_PairScorer):
    """recstudio/model/scorer.py:92-113: ``act(W cat(query * key, mlp(cat(query, key))))`` with ``W`` a bias-free
    ``Linear(emb_dim + hidden_size, 1)`` (state_dict ``W.weight``, ``mlp.model.1.weight`` ...)."""

    def __init__(self, emb_dim, hidden_size, mlp, bias=False, activation='relu'):
        super().__init__()
        self.emb_dim = emb_dim
        self.hidden_size = hidden_size
        self.bias = bias
        self.W = torch.nn.Linear(self.emb_dim + self.hidden_size, 1, bias=False)
        from .seqmodule import get_act
        self.activation_name = str(activation).lower()
        self.activation = get_act(activation)
        self.mlp = mlp

    def _parts(self):
        got = _plain_relu_mlp(self.mlp)
        if got is None or self.activation_name != 'relu' or got[0][-1].out_features != self.hidden_size:
            return None
        return got[0], got[1], self.W.weight, None, True

    def _torch_scores(self, query, key):
        h = torch.cat([query * key, self.mlp(torch.cat([query, key], dim=-1))], dim=-1)
        return self.activation(self.W(h).squeeze(-1))


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
