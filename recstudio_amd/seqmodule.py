"""The sequence towers' encoders with their cores as fused kernels: the Transformer encoder's attention (SASRec) and the GRU
recurrence (GRU4Rec; below, "THE GRU").

recstudio/model/seq/sasrec.py:19-33 builds the tower from ``torch.nn.TransformerEncoder`` (post-norm, batch-first) and calls it
with a bool causal mask and a key-padding mask (:44-53).  ``FusedTransformerEncoder`` runs the same layers over the SAME
parameters -- the ``nn.TransformerEncoder`` stays the parameter container, so ``state_dict`` keys are the reference's -- with what
``nn.MultiheadAttention`` does between ``in_proj`` and ``out_proj`` replaced by ``ops.seq_attention`` (``rsa_attention``,
recstudio_amd/csrc/rsa_attention.hip): no head-major copies, no ``[B, H, L, L]`` tensor.  The Linears, LayerNorms, the
activation and the three ``nn.Dropout`` s of a layer stay torch ops.

THE MASK RULE.  Key j is allowed for query i iff ``(not causal or j <= i) and not key_pad[b, j]`` -- what torch's merged float
mask amounts to.  A query without an allowed key gets ``out = 0`` and passes no gradient; torch returns NaN for it.  (A
right-padded history under the causal mask has no such query; a fully padded sequence without the causal mask has.)

THE DROPOUT on the attention probabilities follows the project's rule (graphmodule.BiCombiner), not ``nn.Dropout`` 's kernel:
with q = fp32(1 - p), element (b, h, i, j) is kept iff ``torch.rand(B, H, L, L)[b, h, i, j] < q`` and divided by q -- ONE
``torch.rand`` call on the device generator per attention call.  In train mode a layer therefore consumes the generator in
this order: the attention's ``rand``, ``dropout1``, ``dropout`` (inside the feed-forward), ``dropout2``.

``seq_attention_torch`` is the same rule in plain torch ops: the path for CPU tensors, and the twin the tests and the timings
compare the kernel with.

THE GRU.  recstudio/model/module/layers.py:225-244 (``GRULayer``) is a ``torch.nn.GRU`` (``bias=False``, ``batch_first=True``);
recstudio/model/seq/gru4rec.py puts it under last-position pooling.  ``FusedGRU`` runs a stock ``nn.GRU`` 's layers over the SAME
parameters with the split of labour of DESIGN.md 4.14: what is parallel in time stays a torch GEMM (``gi = F.linear(x, W_ih,
b_ih)``; in the backward ``gh = F.linear(h_prev, W_hh, b_hh)`` over all positions, ``dW_hh = dgh^T h_prev``, ``db_hh``), the L
dependent steps are ONE launch of ``ops.gru_sequence`` (``rsa_gru``, recstudio_amd/csrc/rsa_gru.hip) per direction.
``lengths``: row b stops at ``lengths[b]``; ``out[b, t >= lengths[b]]`` is 0 and ``h_n[b]`` is the state at ``lengths[b] - 1``
(``nn.GRU`` runs on over the padding; the reference's consumers discard those positions).  ``gru_sequence_torch`` is the twin.

THE FEED-FORWARD ATTENTION POOLING (NARM, STAMP).  recstudio/model/module/layers.py:322-399 (``AttentionLayer``) with
``attention_type='feedforward'`` scores every position of the history against ONE query vector per sequence through a
one-hidden-layer MLP and returns the weighted sum of the history rows.  ``MLPModule`` and ``AttentionLayer`` here take the
reference's constructor arguments and hold its parameters under its ``state_dict`` keys (``mlp.0.model.1.weight`` = ``W1``
[M, q_dim + k_dim], ``mlp.0.model.1.bias`` = ``b1`` with ``bias=True``, ``mlp.1.weight`` = ``w2`` [1, M], ``mlp.1.bias`` = ``b2``).
The rule, with ``softmax=False`` and value = key (the only way the two models call it):

    qh_b = W1[:, :q_dim] q_b (+ b1)        hid_bs = sigmoid(qh_b + W1[:, q_dim:] k_bs)
    a_bs = key_pad[b, s] ? 0 : (w2 . hid_bs + b2) / sqrt(q_dim)        out_b = sum_s a_bs k_bs

The divisor is ``sqrt(q_dim)`` (the reference reads ``.size(-1)`` of the EXPANDED query, before the concatenation); the mask
fills with 0 -- there is no softmax --; ``b2`` reaches every live position.  ``qh`` stays a torch GEMM; everything per position is
ONE launch of ``ops.ff_attention_pool`` (``rsa_ff_attention``, recstudio_amd/csrc/rsa_ffattn.hip), which never writes the
``[B, S, q_dim + k_dim]`` concatenation or the ``[B, S, M]`` hidden layer, and whose backward recomputes instead of saving.
``ff_attention_pool_torch`` is the twin: the reference's op sequence literally.

THE CONVOLUTIONS OF CASER.  recstudio/model/seq/caser.py:36-56 runs, on the gathered history rows ``E`` [B, L, d] (right-padded
with zero rows to ``L = max_seq_len``; there is no mask), one ``Conv2d(1, n_v, (L, 1))`` and L ``Conv2d(1, n_h, (h, d))``, h = 1 ..
L, each of the latter under ``relu``, ``max_pool1d`` over its L - h + 1 windows and ``squeeze``, and two ``cat`` s:

    o_v[b, c d + k] = b_v[c] + sum_t W_v[c, t] E[b, t, k]            o_h[b, (h - 1) n_h + c] = max(0, max_t conv_h[b, t, c])
    conv_h[b, t, c] = b_h[c] + sum_{j < h} sum_k W_h[c, j, k] E[b, t + j, k]            o = cat(o_v, o_h)   [B, n_v d + L n_h]

``caser_conv_torch`` is that op sequence on the filters PACKED: ``w_h`` = the L ``Conv2d.weight.reshape(-1)`` concatenated in
height order (block h, [n_h, h, d], at element ``n_h d h (h - 1) / 2``), ``b_h`` [L, n_h] the biases alike -- one ``torch.cat`` each
per call (``caser_pack``), whose own backward hands the slices of the gradient back to the L modules.  It is the operand layout a
fused kernel would take; no such kernel ships, so the tower runs on torch ops.

THE GATES OF HGN.  recstudio/model/seq/hgn.py:34-43 runs, on the gathered history rows ``S`` [B, L, d] (padded positions are the
zero row; there is NO mask) and the user row ``U`` [B, d]:

    f = sigmoid(W_g_1 s + ug)      sf = s * f      w = sigmoid(w_g_3 . sf + ui)      si = sf * w
    mean: pooled = sum_l si / sum_l w        max: pooled[c] = max_l si[c]        out = pooled + sum_l s        query = U + out

with ``ug = W_g_2 U + b_g`` [B, d] and ``ui = U W_g_4.weight[:L]^T`` [B, L] (``W_g_4.bias`` is never used).  Padded positions
have ``si = 0`` but ``w = sigmoid(ui) > 0``: they count in the mean's denominator and take part in the max.  ``ug`` and ``ui``
stay torch GEMMs; everything per position is ONE launch of ``ops.hgn_gating`` (``rsa_hgn_gating``,
recstudio_amd/csrc/rsa_gating.hip), which writes ``out``, ``w`` [B, L] and the max's positions and none of the reference's eight
``[B, L, d]`` temporaries; the backward recomputes the gates.  ``hgn_gating_torch`` is the twin: the reference's op sequence.

USER-HISTORY BAGS.  The autoencoder retrievers (recstudio/model/ae/multidae.py:29-31, multivae.py:33-35) start from

    seq_emb = item_embedding(ids).sum(1) / ids.count_nonzero(1) ** 0.5          ids [B, L], 0 = padding

and their softmax loss needs, per user, the mean of the positives' rows.  ``bag_pool(weight, ids, scale)`` is both: ONE bag sum
straight from the padded id matrix (``ops.bag_pool``, ``rsa_bag_pool``, recstudio_amd/csrc/rsa_bag.hip) with the scale 'sum',
'rsqrt' or 'mean', and a sorted, atomic-free backward into the dense table gradient; no ``[B, L, d]`` tensor exists in either
direction.  Deviation: padding is skipped, not read -- equal to the reference whenever row 0 of the table is zero, which
``padding_idx=0`` guarantees.  ``bag_pool_torch`` is the twin: the reference's op sequence (it DOES read row 0).
"""
import math

import torch
import torch.nn.functional as F

from . import ops, rng

__all__ = ['seq_attention', 'seq_attention_torch', 'FusedTransformerEncoder', 'gru_sequence', 'gru_sequence_torch', 'FusedGRU',
           'ff_attention_pool', 'ff_attention_pool_torch', 'MLPModule', 'AttentionLayer', 'caser_conv_torch', 'caser_pack',
           'hgn_gating', 'hgn_gating_torch', 'bag_pool', 'bag_pool_torch']


def allowed_keys(key_pad, causal, B, L, device):
    """bool [B, 1, L, L]: key j allowed for query i."""
    ok = torch.ones(L, L, dtype=torch.bool, device=device)
    if causal:
        ok = torch.tril(ok)
    ok = ok.view(1, 1, L, L).expand(B, 1, L, L)
    if key_pad is not None:
        ok = ok & ~key_pad.bool().view(B, 1, 1, L)
    return ok


def seq_attention_torch(qkv, key_pad, causal, H, p=0.0, generator=None, want_keep=False):
    """The attention core in torch ops, under the mask and dropout rules of the module docstring.  ``qkv`` [B, L, 3 D] ->
    ``out`` [B, L, D] (and the bool keep mask [B, H, L, L] with ``want_keep``).  ``generator``: the generator of ``qkv`` 's
    device the one ``torch.rand`` call draws from (None: the default one)."""
    B, L, D3 = qkv.shape
    D = D3 // 3
    dh = D // H
    q, k, v = (t.reshape(B, L, H, dh).transpose(1, 2) for t in qkv.split(D, dim=2))
    s = (q @ k.transpose(2, 3)) * (1.0 / math.sqrt(dh))
    ok = allowed_keys(key_pad, causal, B, L, qkv.device)
    some = ok.any(dim=3, keepdim=True)
    s = torch.where(some, s.masked_fill(~ok, float('-inf')), torch.zeros((), dtype=s.dtype, device=s.device))
    pr = torch.softmax(s, dim=3) * some.to(s.dtype)
    keep = None
    if p > 0.0:
        qf = torch.tensor(1.0 - p, dtype=torch.float32).item()
        keep = torch.rand(B, H, L, L, device=qkv.device, dtype=torch.float32, generator=generator) < qf
        pr = pr * keep.to(pr.dtype) / qf
    out = (pr @ v).transpose(1, 2).reshape(B, L, D)
    return (out, keep) if want_keep else out


class _SeqAttentionFn(torch.autograd.Function):
    """``ops.seq_attention`` / ``ops.seq_attention_backward`` as one autograd node.  Saved: ``qkv``, ``out``, ``lse`` and the
    Philox state -- nothing of size L x L."""

    @staticmethod
    def forward(ctx, qkv, key_pad, causal, n_head, p, generator):
        qkv = qkv.detach().contiguous()
        B, L, _ = qkv.shape
        pc = rng.reserve(B * n_head * L * L, 4, qkv.device, generator) if p > 0.0 else None
        out, lse = ops.seq_attention(qkv, key_pad, n_head, causal=causal, p=p, philox=pc)
        ctx.save_for_backward(qkv, out, lse)
        ctx.key_pad, ctx.causal, ctx.n_head, ctx.p, ctx.pc = key_pad, causal, n_head, p, pc
        return out

    @staticmethod
    def backward(ctx, g_out):
        qkv, out, lse = ctx.saved_tensors
        dqkv = ops.seq_attention_backward(qkv, ctx.key_pad, ctx.n_head, out, lse, g_out.contiguous(), causal=ctx.causal, p=ctx.p,
                                          philox=ctx.pc)
        return dqkv, None, None, None, None, None


def seq_attention(qkv, key_pad, causal, n_head, p=0.0, generator=None):
    """``out`` [B, L, D] of the attention core: the fused kernel for device tensors, ``seq_attention_torch`` for CPU tensors."""
    if qkv.is_cuda:
        if key_pad is not None and key_pad.dtype == torch.bool:
            key_pad = key_pad.contiguous().view(torch.uint8)
        return _SeqAttentionFn.apply(qkv, key_pad, bool(causal), int(n_head), float(p), generator)
    return seq_attention_torch(qkv, key_pad, causal, n_head, p, generator)


class FusedTransformerEncoder:
    """The layers of ``encoder`` (a post-norm, batch-first ``torch.nn.TransformerEncoder``) with the fused attention core.  It
    owns no parameter: every weight is read from ``encoder`` at call time, so the module that holds ``encoder`` keeps its
    ``state_dict``, its optimizer groups and its ``.to()`` / ``.train()`` behaviour, and a checkpoint moves freely between this
    path and ``encoder(...)`` itself.

    Per layer:  ``a = attention(F.linear(x, in_proj_weight, in_proj_bias))``,  ``x = norm1(x + dropout1(out_proj(a)))``,
    ``x = norm2(x + dropout2(linear2(dropout(activation(linear1(x))))))``; ``encoder.norm`` (when there is one) closes the stack.
    """

    def __init__(self, encoder, max_seq_len, generator=None):
        if not isinstance(encoder, torch.nn.TransformerEncoder):
            raise TypeError(f'FusedTransformerEncoder: expected a torch.nn.TransformerEncoder, got {type(encoder)}')
        if int(max_seq_len) > ops.SEQ_ATTENTION_MAX_LEN:
            raise ValueError(f'FusedTransformerEncoder: max_seq_len {max_seq_len} > {ops.SEQ_ATTENTION_MAX_LEN}: one tile of the '
                             'fused attention holds the whole sequence (longer histories: fused_attention = False)')
        for k, layer in enumerate(encoder.layers):
            mha = layer.self_attn
            if layer.norm_first:
                raise ValueError(f'FusedTransformerEncoder: layer {k} has norm_first=True; only the post-norm layer the reference '
                                 'builds is implemented')
            if not mha.batch_first or not mha._qkv_same_embed_dim or mha.in_proj_bias is None or mha.bias_k is not None \
                    or mha.add_zero_attn:
                raise ValueError(f'FusedTransformerEncoder: layer {k}: the attention must be batch_first, with one in_proj of q, k '
                                 'and v with a bias, and without bias_k / add_zero_attn')
            if mha.head_dim not in ops.SEQ_ATTENTION_HEAD_DIMS:
                raise ValueError(f'FusedTransformerEncoder: layer {k}: head_dim = embed_dim / n_head = {mha.head_dim} must be one '
                                 f'of {ops.SEQ_ATTENTION_HEAD_DIMS}')
        self.encoder = encoder
        self.generator = generator

    def __call__(self, src, key_pad=None, causal=True):
        """``src`` [B, L, d]; ``key_pad`` bool [B, L] or None (True: that key is not attended) -> [B, L, d]."""
        x = src
        for layer in self.encoder.layers:
            mha = layer.self_attn
            qkv = F.linear(x, mha.in_proj_weight, mha.in_proj_bias)
            p = float(mha.dropout) if layer.training else 0.0
            a = seq_attention(qkv, key_pad, causal, mha.num_heads, p, self.generator)
            x = layer.norm1(x + layer.dropout1(mha.out_proj(a)))
            x = layer.norm2(x + layer.dropout2(layer.linear2(layer.dropout(layer.activation(layer.linear1(x))))))
        if self.encoder.norm is not None:
            x = self.encoder.norm(x)
        return x


def gru_sequence_torch(gi, w_hh, b_hh=None, h0=None, lengths=None):
    """The GRU recurrence in torch ops (any float dtype), gate order r, z, n, ``b_hn`` inside ``r * (.)``: ``gi`` [B, L, 3 H] ->
    ``out`` [B, L, H].  With ``lengths`` (int64 [B]) row b stops at ``lengths[b]`` and ``out[b, t >= lengths[b]]`` is 0."""
    B, L, H3 = gi.shape
    H = H3 // 3
    h = h0 if h0 is not None else gi.new_zeros(B, H)
    outs = []
    for t in range(L):
        i_r, i_z, i_n = gi[:, t].split(H, dim=1)
        h_r, h_z, h_n = F.linear(h, w_hh, b_hh).split(H, dim=1)
        r = torch.sigmoid(i_r + h_r)
        z = torch.sigmoid(i_z + h_z)
        n = torch.tanh(i_n + r * h_n)
        new = (1.0 - z) * n + z * h
        if lengths is None:
            h = new
            outs.append(new)
        else:
            on = (lengths > t).view(B, 1)
            h = torch.where(on, new, h)
            outs.append(torch.where(on, new, torch.zeros_like(new)))
    return torch.stack(outs, dim=1) if L else gi.new_zeros(B, 0, H)


class _GruFn(torch.autograd.Function):
    """``ops.gru_sequence`` / ``ops.gru_sequence_backward`` and the three GEMMs of the backward that are parallel in time as one
    autograd node.  Saved: the inputs and ``out`` -- every ``h_{t-1}`` is in ``out``."""

    @staticmethod
    def forward(ctx, gi, w_hh, b_hh, h0, lengths):
        gi = gi.detach().contiguous()
        out = ops.gru_sequence(gi, w_hh.detach(), b_hh=None if b_hh is None else b_hh.detach(),
                               h0=None if h0 is None else h0.detach(), lengths=lengths)
        ctx.save_for_backward(gi, w_hh, b_hh, h0, lengths, out)
        return out

    @staticmethod
    def backward(ctx, g_out):
        gi, w_hh, b_hh, h0, lengths, out = ctx.saved_tensors
        B, L, H = out.shape
        first = h0.view(B, 1, H) if h0 is not None else out.new_zeros(B, 1, H)
        h_prev = torch.cat([first, out[:, :-1]], dim=1)
        gh = F.linear(h_prev, w_hh, b_hh)
        dgi, dgh_n, dh0 = ops.gru_sequence_backward(gi, gh, out, w_hh, g_out.contiguous(), h0=h0, lengths=lengths)
        del gh
        hp, drz = h_prev.view(B * L, H), dgi.view(B * L, 3 * H)[:, :2 * H]
        dw = db = None
        if ctx.needs_input_grad[1]:
            dw = torch.cat([drz.t() @ hp, dgh_n.view(B * L, H).t() @ hp], dim=0)
        if b_hh is not None and ctx.needs_input_grad[2]:
            db = torch.cat([drz.sum(0), dgh_n.view(B * L, H).sum(0)], dim=0)
        return dgi, dw, db, (dh0 if h0 is not None else None), None


def gru_sequence(gi, w_hh, b_hh=None, h0=None, lengths=None):
    """``out`` [B, L, H] of the GRU recurrence: the fused kernel for fp32 device tensors, ``gru_sequence_torch`` for CPU tensors."""
    if gi.is_cuda:
        return _GruFn.apply(gi, w_hh, b_hh, h0, lengths)
    return gru_sequence_torch(gi, w_hh, b_hh, h0, lengths)


class FusedGRU:
    """The layers of ``gru`` (a stock ``torch.nn.GRU``) with the recurrence as one fused kernel per layer.  It owns no parameter:
    every weight is read from ``gru`` at call time, so the module that holds ``gru`` keeps its ``state_dict``, its optimizer
    groups and its ``.to()`` / ``.train()`` behaviour, and a checkpoint moves freely between this path and ``gru(...)`` itself.

    ``num_layers >= 1`` is a chain of calls; ``bias`` true or false.  A bidirectional, time-major or projected GRU, inter-layer
    dropout in train mode, a hidden size outside ``ops.GRU_HIDDEN_SIZES`` or a device dtype other than fp32 falls back to ``gru``
    itself: with ``lengths`` its ``out`` is zeroed at ``t >= lengths[b]``, and ``h_n`` is the wrapped module's (the state after all
    L steps)."""

    def __init__(self, gru):
        if not isinstance(gru, torch.nn.GRU):
            raise TypeError(f'FusedGRU: expected a torch.nn.GRU, got {type(gru)}')
        self.gru = gru

    def fused(self, x):
        """Whether a call on ``x`` takes the fused path (the kernel, or its twin on CPU tensors)."""
        g = self.gru
        return (g.batch_first and not g.bidirectional and getattr(g, 'proj_size', 0) == 0 and g.hidden_size in ops.GRU_HIDDEN_SIZES
                and not (g.training and g.dropout > 0 and g.num_layers > 1) and x.dim() == 3
                and (x.dtype == torch.float32 or (not x.is_cuda and x.is_floating_point())))

    def __call__(self, x, h0=None, lengths=None, want_state=True):
        """``x`` [B, L, input_size], ``h0`` [num_layers, B, H] or None, ``lengths`` int64 [B] or None ->
        ``(out [B, L, H], h_n [num_layers, B, H])`` as ``nn.GRU`` returns them (``h_n`` None without ``want_state``: a caller that
        pools ``out`` itself saves the gathers)."""
        g = self.gru
        B, L = x.shape[0], x.shape[1]
        if not self.fused(x):
            out, h_n = g(x, h0)
            if lengths is None or not g.batch_first:
                return out, h_n
            on = (torch.arange(L, device=x.device).view(1, L) < lengths.view(B, 1)).unsqueeze(2)
            return out * on.to(out.dtype), h_n
        finals = []
        for k in range(g.num_layers):
            w_ih, w_hh = getattr(g, f'weight_ih_l{k}'), getattr(g, f'weight_hh_l{k}')
            b_ih, b_hh = (getattr(g, f'bias_ih_l{k}'), getattr(g, f'bias_hh_l{k}')) if g.bias else (None, None)
            first = None if h0 is None else h0[k]
            x = gru_sequence(F.linear(x, w_ih, b_ih), w_hh, b_hh, first, lengths)
            if want_state:
                finals.append(last_state(x, first, lengths))
        return x, (torch.stack(finals, dim=0) if want_state else None)


def last_state(out, h0, lengths):
    """``h`` [B, H] after the last step of each row: ``out[b, lengths[b] - 1]`` (``out[:, -1]`` without ``lengths``; ``h0`` or 0
    for an empty row)."""
    B, L, H = out.shape
    if lengths is None:
        if L:
            return out[:, -1]
        return h0 if h0 is not None else out.new_zeros(B, H)
    idx = (lengths - 1).clamp(min=0, max=max(L - 1, 0)).view(B, 1, 1).expand(B, 1, H)
    last = out.gather(1, idx).squeeze(1) if L else out.new_zeros(B, H)
    empty = (lengths <= 0).view(B, 1)
    return torch.where(empty, h0 if h0 is not None else torch.zeros_like(last), last)


def ff_attention_pool_torch(query, key, w1, b1, w2, b2, key_pad=None):
    """The feed-forward attention pooling in the reference's own op sequence (recstudio/model/module/layers.py:371-389 around
    the MLP of :346-354), any float dtype: ``query`` [B, q_dim], ``key`` [B, S, k_dim], ``w1`` [M, q_dim + k_dim], ``b1`` [M] or
    None, ``w2`` [1, M], ``b2`` [1], ``key_pad`` bool [B, S] or None -> ``(out [B, k_dim], a [B, S])``."""
    q = query.unsqueeze(1)                                                       # the caller's query.unsqueeze(1): B x 1 x q_dim
    q = q.unsqueeze(2).expand(-1, -1, key.size(1), -1)                           # layers.py:371
    k = key.unsqueeze(1).expand(-1, q.size(1), -1, -1)                           # layers.py:372
    x = torch.cat((q, k), dim=-1)                                                # layers.py:374
    hid = torch.sigmoid(F.linear(x, w1, b1))                                     # MLPModule: Dropout(0), Linear, Sigmoid (:198-205)
    w = F.linear(hid, w2, b2).squeeze(-1)                                        # layers.py:353, :374   B x 1 x S
    w = w / (q.size(-1) ** 0.5)                                                  # layers.py:378
    if key_pad is not None:
        w = w.masked_fill(key_pad.bool().unsqueeze(1).expand(-1, q.size(1), -1), 0.0)   # layers.py:380-384 (softmax=False)
    out = w @ key                                                                # layers.py:389   B x 1 x D
    return out.squeeze(1), w.squeeze(1)


class _FfAttentionFn(torch.autograd.Function):
    """``ops.ff_attention_pool`` / ``ops.ff_attention_pool_backward`` and the small GEMMs on the query side as one autograd node.
    Saved: the inputs and ``qh`` [B, M] -- nothing of size B S M; the backward recomputes the hidden layer and the weights."""

    @staticmethod
    def forward(ctx, query, key, w1, b1, w2, b2, key_pad):
        query, key = query.detach().contiguous(), key.detach().contiguous()
        w1, w2, b2 = w1.detach(), w2.detach(), b2.detach()
        q_dim = query.shape[1]
        qh = F.linear(query, w1[:, :q_dim], None if b1 is None else b1.detach())
        scale = 1.0 / math.sqrt(q_dim)
        out, a = ops.ff_attention_pool(key, qh, w1[:, q_dim:], w2, b2, key_pad, scale=scale)
        ctx.save_for_backward(query, key, w1, w2, b2, key_pad, qh)
        ctx.scale, ctx.has_b1 = scale, b1 is not None
        ctx.mark_non_differentiable(a)
        return out, a

    @staticmethod
    def backward(ctx, g_out, _g_a):
        query, key, w1, w2, b2, key_pad, qh = ctx.saved_tensors
        q_dim = query.shape[1]
        dkey, dqh, dw_k, dw2, db2 = ops.ff_attention_pool_backward(key, qh, w1[:, q_dim:], w2, b2, key_pad, g_out.contiguous(),
                                                                   scale=ctx.scale)
        dquery = dqh @ w1[:, :q_dim] if ctx.needs_input_grad[0] else None
        dw1 = torch.cat([dqh.t() @ query, dw_k], dim=1) if ctx.needs_input_grad[2] else None
        db1 = dqh.sum(0) if ctx.has_b1 and ctx.needs_input_grad[3] else None
        return dquery, dkey, dw1, db1, dw2.view_as(w2), db2.view_as(b2), None


def ff_attention_kernel_ok(query, key, w1):
    """Whether ``ops.ff_attention_pool`` takes these tensors: fp32 on the device, key width and hidden width in
    ``ops.FF_ATTENTION_DIMS``, and ``W1[:, q_dim:]`` a 16-byte aligned column block."""
    return (key.is_cuda and query.is_cuda and w1.is_cuda and key.dtype == query.dtype == w1.dtype == torch.float32
            and query.dim() == 2 and key.dim() == 3 and key.shape[1] >= 1 and key.shape[2] in ops.FF_ATTENTION_DIMS
            and w1.shape[0] in ops.FF_ATTENTION_DIMS and query.shape[1] % 4 == 0 and w1.is_contiguous()
            and w1.shape[1] == query.shape[1] + key.shape[2] and w1.data_ptr() % 16 == 0)


def ff_attention_pool(query, key, w1, b1, w2, b2, key_pad=None):
    """``(out [B, k_dim], a [B, S])`` of the feed-forward attention pooling: the fused kernel where ``ff_attention_kernel_ok``,
    ``ff_attention_pool_torch`` otherwise (CPU tensors: the parity path)."""
    if ff_attention_kernel_ok(query, key, w1):
        if key_pad is not None and key_pad.dtype == torch.bool:
            key_pad = key_pad.contiguous().view(torch.uint8)
        return _FfAttentionFn.apply(query, key, w1, b1, w2, b2, key_pad)
    return ff_attention_pool_torch(query, key, w1, b1, w2, b2, key_pad)


def hgn_gating_torch(S, ug, ui, w1, w3, pooling='mean'):
    """HGN's gates, pooling and item-item sum in the reference's own op sequence (recstudio/model/seq/hgn.py:34-43), any float
    dtype: ``S`` [B, L, d], ``ug`` [B, d] = ``W_g_2(U) + b_g``, ``ui`` [B, L] = ``U @ W_g_4.weight[:L].T``, ``w1`` [d, d], ``w3``
    [1, d] -> ``out`` [B, d] = the query without its ``U +``."""
    S_F = S * torch.sigmoid(F.linear(S, w1) + ug.view(ug.size(0), 1, -1))        # hgn.py:34
    weight = torch.sigmoid(F.linear(S_F, w3.view(1, -1)) + ui.view(ui.size(0), -1, 1))   # hgn.py:35   B x L x 1
    S_I = S_F * weight                                                           # hgn.py:36
    if pooling == 'mean':
        s = S_I.sum(1) / weight.sum(1)                                           # hgn.py:38
    elif pooling == 'max':
        s = torch.max(S_I, dim=1).values                                         # hgn.py:40
    else:
        raise ValueError("`pooling_type` only support `avg` and `max`")          # hgn.py:42
    return s + S.sum(1)                                                          # hgn.py:43


class _HgnGatingFn(torch.autograd.Function):
    """``ops.hgn_gating`` / ``ops.hgn_gating_backward`` as one autograd node.  Saved: the inputs, ``w`` [B, L] and (max) ``arg``
    [B, d] -- nothing of size B L d beyond ``S`` itself; the backward recomputes the gates."""

    @staticmethod
    def forward(ctx, S, ug, ui, w1, w3, pooling):
        S, ug, ui = S.detach().contiguous(), ug.detach().contiguous(), ui.detach().contiguous()
        w1, w3 = w1.detach(), w3.detach()
        out, w, arg = ops.hgn_gating(S, ug, ui, w1, w3, pooling)
        ctx.save_for_backward(S, ug, ui, w1, w3, w, arg)
        ctx.pooling = pooling
        return out

    @staticmethod
    def backward(ctx, g_out):
        S, ug, ui, w1, w3, w, arg = ctx.saved_tensors
        dS, dug, dui, dw1, dw3 = ops.hgn_gating_backward(S, ug, ui, w1, w3, w, arg, g_out.contiguous(), ctx.pooling)
        return dS, dug, dui, dw1, dw3.view_as(w3), None


def hgn_gating_kernel_ok(S, ug, ui, w1, w3):
    """Whether ``ops.hgn_gating`` takes these tensors: fp32 on the device, width in ``ops.HGN_GATING_DIMS``, ``L >= 1``."""
    return (all(t.is_cuda and t.dtype == torch.float32 for t in (S, ug, ui, w1, w3)) and S.dim() == 3 and S.shape[1] >= 1
            and S.shape[2] in ops.HGN_GATING_DIMS and w1.stride(1) == 1 and w1.stride(0) % 4 == 0 and w1.data_ptr() % 16 == 0)


def hgn_gating(S, ug, ui, w1, w3, pooling='mean'):
    """``out`` [B, d] of HGN's gating: the fused kernel where ``hgn_gating_kernel_ok``, ``hgn_gating_torch`` otherwise (CPU
    tensors: the parity path; widths the kernel does not take)."""
    if pooling not in ('mean', 'max'):
        raise ValueError("`pooling_type` only support `avg` and `max`")
    if hgn_gating_kernel_ok(S, ug, ui, w1, w3):
        return _HgnGatingFn.apply(S, ug, ui, w1, w3, pooling)
    return hgn_gating_torch(S, ug, ui, w1, w3, pooling)


BAG_SCALES = ('sum', 'rsqrt', 'mean')


def bag_pool_torch(weight, ids, scale='sum'):
    """The bag sum in the reference's own op sequence (recstudio/model/ae/multidae.py:29-31), any float dtype: gather
    ``[B, L, d]``, sum over L, divide by ``count_nonzero ** 0.5`` ('rsqrt') or ``count_nonzero`` ('mean').  An empty bag divides
    0 by 0 (NaN), as the reference does."""
    if scale not in BAG_SCALES:
        raise ValueError(f'scale must be one of {BAG_SCALES}, got {scale!r}')
    out = F.embedding(ids, weight, padding_idx=0).sum(1)        # nn.Embedding(.., padding_idx=0): row 0 is read, and gets no gradient
    if scale == 'sum':
        return out
    non_zero_num = ids.count_nonzero(dim=1).unsqueeze(-1).to(out.dtype)      # (the reference's int64 .pow(0.5) is fp32: the same in fp32)
    return out / (non_zero_num.pow(0.5) if scale == 'rsqrt' else non_zero_num)


class _BagPoolFn(torch.autograd.Function):
    """``ops.bag_pool`` / ``ops.bag_pool_backward`` as one autograd node: linear in ``weight``, no gradient to ``ids``.  Saved:
    ``ids`` and ``cnt`` [B]."""

    @staticmethod
    def forward(ctx, weight, ids, scale):
        out, cnt = ops.bag_pool(weight.detach(), ids, scale)
        ctx.save_for_backward(ids, cnt)
        ctx.scale, ctx.n_rows = scale, weight.shape[0]
        return out

    @staticmethod
    def backward(ctx, g_out):
        ids, cnt = ctx.saved_tensors
        return ops.bag_pool_backward(ids, cnt, g_out.contiguous(), ctx.n_rows, ctx.scale), None, None


def bag_pool_kernel_ok(weight, ids):
    """Whether ``ops.bag_pool`` takes these tensors: an fp32 table and int64 ids on the device, a width that is a multiple of 4
    up to ``ops.BAG_MAX_DIM``."""
    return (weight.is_cuda and ids.is_cuda and weight.dtype == torch.float32 and ids.dtype == torch.int64 and weight.dim() == 2
            and ids.dim() == 2 and weight.shape[1] % 4 == 0 and 4 <= weight.shape[1] <= ops.BAG_MAX_DIM)


def bag_pool(weight, ids, scale='sum', fused=True):
    """``[B, d]`` bag sums of the rows ``weight[ids]`` (see the module docstring): the kernel pair where ``fused`` and
    ``bag_pool_kernel_ok``, ``bag_pool_torch`` otherwise (CPU tensors: the parity path; widths the kernel does not take)."""
    if scale not in BAG_SCALES:
        raise ValueError(f'scale must be one of {BAG_SCALES}, got {scale!r}')
    if fused and bag_pool_kernel_ok(weight, ids):
        return _BagPoolFn.apply(weight, ids, scale)
    return bag_pool_torch(weight, ids, scale)


def caser_pack(vertical_filter, horizontal_filter):
    """``(w_v [n_v, L], b_v [n_v], w_h packed, b_h [L, n_h])`` of Caser's ``Conv2d`` modules: views for the vertical filter, ONE
    ``torch.cat`` for the horizontal weights and one for their biases (``CatBackward`` hands the slices of the gradients back)."""
    w_v = vertical_filter.weight.reshape(vertical_filter.weight.shape[0], -1)
    w_h = torch.cat([conv.weight.reshape(-1) for conv in horizontal_filter])
    b_h = torch.cat([conv.bias for conv in horizontal_filter]).view(len(horizontal_filter), -1)
    return w_v, vertical_filter.bias, w_h, b_h


def caser_conv_torch(rows, w_v, b_v, w_h, b_h):
    """Caser's convolutions in the reference's own op sequence (recstudio/model/seq/caser.py:41-53) on the packed operands, any
    float dtype: ``rows`` [B, L, d], ``w_v`` [n_v, L], ``b_v`` [n_v], ``w_h`` packed, ``b_h`` [L, n_h] -> ``o`` [B, n_v d + L n_h]."""
    B, L, d = rows.shape
    n_v, n_h = w_v.shape[0], b_h.shape[1]
    x = rows.view(-1, 1, L, d)                                                   # caser.py:41
    o_v = F.conv2d(x, w_v.view(n_v, 1, L, 1), b_v)                               # caser.py:43
    o_v = o_v.reshape(o_v.size(0), -1)                                           # caser.py:44
    o_h, at = [], 0
    for i in range(L):                                                           # caser.py:47-50
        h = i + 1
        w = w_h[at:at + n_h * h * d].view(n_h, 1, h, d)
        at += n_h * h * d
        conv_out = torch.relu(F.conv2d(x, w, b_h[i]).squeeze(3))
        pool_out = F.max_pool1d(conv_out, conv_out.size(2))
        o_h.append(pool_out.squeeze(2))
    return torch.cat((o_v, torch.cat(o_h, dim=1)), dim=1)                        # caser.py:51-53


def get_act(activation, dim=None):
    """recstudio/model/module/layers.py:22-47, the activations the sequence towers name."""
    if activation is None or isinstance(activation, torch.nn.Module):
        return activation
    if not isinstance(activation, str):
        raise ValueError('"activation_func" must be a str or a instance of torch.nn.Module. ')
    table = {'relu': torch.nn.ReLU, 'sigmoid': torch.nn.Sigmoid, 'tanh': torch.nn.Tanh, 'leakyrelu': torch.nn.LeakyReLU,
             'gelu': torch.nn.GELU, 'identity': torch.nn.Identity}
    if activation.lower() not in table:
        raise ValueError(f'activation function type "{activation}"  is not supported, check spelling or pass in a instance of '
                         'torch.nn.Module.')
    return table[activation.lower()]()


class MLPModule(torch.nn.Module):
    """recstudio/model/module/layers.py:150-222: per layer ``Dropout``, ``Linear``, (``BatchNorm1d``,) activation, in one
    ``nn.Sequential`` named ``model`` -- the first Linear is ``model.1``."""

    def __init__(self, mlp_layers, activation_func='ReLU', dropout=0.0, bias=True, batch_norm=False, last_activation=True,
                 last_bn=True):
        super().__init__()
        self.mlp_layers = mlp_layers
        self.batch_norm = batch_norm
        self.bias = bias
        self.dropout = dropout
        self.activation_func = activation_func
        layers = []
        last_bn = self.batch_norm and last_bn
        n = len(mlp_layers) - 2
        for idx, (d_in, d_out) in enumerate(zip(mlp_layers[:-1], mlp_layers[1:])):
            layers.append(torch.nn.Dropout(dropout))
            layers.append(torch.nn.Linear(d_in, d_out, bias=bias))
            if (idx == n and last_bn) or (idx < n and batch_norm):
                layers.append(torch.nn.BatchNorm1d(d_out))
            if activation_func is not None and (idx < n or last_activation):
                layers.append(get_act(activation_func, dim=d_out))
        self.model = torch.nn.Sequential(*layers)

    def add_modules(self, *args):
        for block in args:
            assert isinstance(block, torch.nn.Module)
        for block in args:
            self.model.add_module(str(len(self.model._modules)), block)

    def forward(self, input):
        return self.model(input)


class AttentionLayer(torch.nn.Module):
    """recstudio/model/module/layers.py:322-399, same constructor arguments, same ``state_dict``.  ``forward`` takes the fused
    pooling (``ff_attention_pool``) when ``self.fused`` (default True; a plain attribute, not a parameter) and the call is the one
    NARM and STAMP make -- ``attention_type='feedforward'``, one hidden layer with a sigmoid, query length 1, ``value is key``,
    ``softmax=False`` -- on tensors ``ff_attention_kernel_ok`` accepts; every other call runs the reference's op sequence
    (``ff_attention_pool_torch`` for the feed-forward type).  On CPU tensors that twin is the parity path."""

    def __init__(self, q_dim, k_dim=None, v_dim=None, mlp_layers=[], activation='sigmoid', n_head=1, dropout=0.0, bias=True,
                 attention_type='feedforward', batch_first=True):
        super().__init__()
        assert attention_type in ('feedforward', 'multi-head', 'scaled-dot-product'), \
            'expecting attention_type to be one of [feedforeard, multi-head, scaled-dot-product]'
        self.attention_type = attention_type
        self.fused = True
        if k_dim is None:
            k_dim = q_dim
        if v_dim is None:
            v_dim = k_dim
        if attention_type == 'feedforward':
            mlp_layers = [q_dim + k_dim] + list(mlp_layers) + [1]
            self.mlp = torch.nn.Sequential(MLPModule(mlp_layers=mlp_layers[:-1], activation_func=activation, bias=bias),
                                           torch.nn.Linear(mlp_layers[-2], mlp_layers[-1]))
        elif attention_type == 'multi-head':
            self.attn_layer = torch.nn.MultiheadAttention(embed_dim=q_dim, num_heads=n_head, dropout=dropout, bias=bias, kdim=k_dim,
                                                          vdim=v_dim, batch_first=batch_first)
        else:
            assert q_dim == k_dim, 'expecting q_dim is equal to k_dim in scaled-dot-product attention'

    def _one_sigmoid_layer(self):
        """(W1, b1, w2, b2) when the MLP is Dropout(0) / Linear / Sigmoid + Linear(M, 1), else None."""
        if self.attention_type != 'feedforward':
            return None
        body = self.mlp[0].model
        if len(body) != 3 or not isinstance(body[1], torch.nn.Linear) or not isinstance(body[2], torch.nn.Sigmoid) \
                or (body[0].p != 0.0 and self.training):
            return None
        return body[1].weight, body[1].bias, self.mlp[1].weight, self.mlp[1].bias

    def forward(self, query, key, value, key_padding_mask=None, need_weight=False, attn_mask=None, softmax=False,
                average_attn_weights=True):
        # query: B x L x D1; key: B x S x D2; value: B x S x D; key_padding_mask: B x S
        if self.attention_type == 'multi-head':
            attn_output, attn_output_weight = self.attn_layer(query, key, value, key_padding_mask, True, attn_mask,
                                                              average_attn_weights)
            return (attn_output, attn_output_weight) if need_weight else attn_output
        params = self._one_sigmoid_layer()
        if params is not None and query.dim() == 3 and query.shape[1] == 1 and value is key and not softmax:
            pool = ff_attention_pool if self.fused else ff_attention_pool_torch
            out, w = pool(query[:, 0], key, *params, key_padding_mask)
            return (out.unsqueeze(1), w.unsqueeze(1)) if need_weight else out.unsqueeze(1)
        if self.attention_type == 'feedforward':
            query = query.unsqueeze(2).expand(-1, -1, key.size(1), -1)
            key = key.unsqueeze(1).expand(-1, query.size(1), -1, -1)
            attn_output_weight = self.mlp(torch.cat((query, key), dim=-1)).squeeze(-1)      # B x L x S
        else:
            attn_output_weight = query @ key.transpose(1, 2)
        attn_output_weight = attn_output_weight / (query.size(-1) ** 0.5)
        if key_padding_mask is not None:
            key_padding_mask = key_padding_mask.unsqueeze(1).expand(-1, query.size(1), -1)
            attn_output_weight = attn_output_weight.masked_fill(key_padding_mask, -torch.inf if softmax else 0.0)
        if softmax:
            attn_output_weight = torch.softmax(attn_output_weight, dim=-1)
        attn_output = attn_output_weight @ value                                             # B x L x D
        return (attn_output, attn_output_weight) if need_weight else attn_output
