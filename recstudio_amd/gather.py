"""The row gathers of the towers as autograd nodes -- HIP gather forward, sorted row scatter backward -- and the two helpers
every sequence tower is built on: ``_history_rows`` (``item_encoder(in_item_id)``) and ``_last_position``.  Imports ``torch`` and
``ops`` only, so the model families and ``data_augmentation`` can all import it."""
import torch

from . import ops


def _embedding_grad(g, ids, n_rows):
    """Dense ``weight.grad`` of an item-row gather (embedding_dense_backward with padding_idx = 0): rows sorted by item id
    and summed run by run without atomics (``rsa_rows_update_sorted``; bit-reproducible) for the stock dims, the
    float-atomic scatter otherwise."""
    d = g.shape[-1]
    rows = g.reshape(-1, d).contiguous()
    flat_ids = ids.reshape(-1, 1).contiguous()
    if d in (64, 128, 256) and rows.shape[0] > 0:
        ones = torch.ones(rows.shape[0], 1, dtype=torch.float32, device=g.device)
        return ops.scatter_rows_sorted(torch.zeros(n_rows, d, dtype=torch.float32, device=g.device), rows, flat_ids, ones, pad_row=0)
    return ops.scatter_add_rows(rows, flat_ids.view(-1), n_rows)


class _EmbedFn(torch.autograd.Function):
    """item_encoder(ids) with the HIP gather forward and the HIP row scatter-add backward."""

    @staticmethod
    def forward(ctx, weight, ids):
        ctx.save_for_backward(ids)
        ctx.n_rows = weight.shape[0]
        return ops.embedding_gather(weight, ids)

    @staticmethod
    def backward(ctx, g):
        (ids,) = ctx.saved_tensors
        return _embedding_grad(g, ids, ctx.n_rows), None


class _SegEmbedFn(torch.autograd.Function):
    """item_encoder(in_item_id) straight from the CSR view of the interaction column (dataset.py:1418-1439 +
    seq/sasrec.py:42): ``rsa_seg_gather`` reads ``[start, end)`` of the flat item column and writes the right-padded
    ``[B, L, d]`` rows -- no ``[B, L]`` id tensor is re-read; the backward is the sorted, atomics-free row scatter."""

    @staticmethod
    def forward(ctx, weight, flat, start, end, max_len, ids):
        ctx.save_for_backward(ids)
        ctx.n_rows = weight.shape[0]
        return ops.seg_gather(weight, flat, start, end, int(max_len), want_rows=True, want_ids=False)[1]

    @staticmethod
    def backward(ctx, g):
        (ids,) = ctx.saved_tensors
        return _embedding_grad(g, ids, ctx.n_rows), None, None, None, None, None


def _history_rows(item_encoder, ids, seg=None):
    """``item_encoder(ids)`` [B, L, d] of a sequence tower: the HIP gather for an ``nn.Embedding`` on device tensors -- from the
    device loader's CSR view ``seg`` = (flat item column, start, end) when the batch carries one (``ids`` then
    only serves the backward) --, the module itself otherwise (a sharded catalog: ids out, rows back; CPU tensors: the torch-op
    twins of the fused towers, parity checks without a device)."""
    if not isinstance(item_encoder, torch.nn.Embedding) or not ids.is_cuda:
        return item_encoder(ids)
    if seg is not None:
        flat, start, end = seg
        return _SegEmbedFn.apply(item_encoder.weight, flat, start, end, ids.shape[1], ids)
    return _EmbedFn.apply(item_encoder.weight, ids)


def _last_position(out, seqlen):
    """SeqPoolingLayer(pooling_type='last'): ``out[b, seqlen[b] - 1]``."""
    last = (seqlen - 1).clamp(min=0).view(-1, 1, 1).expand(-1, 1, out.shape[-1])
    return out.gather(1, last).squeeze(1)
