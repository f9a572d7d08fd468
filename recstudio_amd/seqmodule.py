"""The sequence towers' Transformer encoder with the attention core as one fused kernel.

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
"""
import math

import torch
import torch.nn.functional as F

from . import ops, rng

__all__ = ['seq_attention', 'seq_attention_torch', 'FusedTransformerEncoder']


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
