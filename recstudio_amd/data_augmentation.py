"""Graph augmentation -- host-side mirror of the graph half of ``recstudio.model.module.data_augmentation`` (:229-450 for SGL,
:524-570 for SimGCL, whose views are not thinned graphs but noise in the propagation: ``graphmodule.SimGCLNet``).

The reference copies its ``dgl`` graph and thins the copy once per view per step (``copy.deepcopy`` + ``dgl.DropEdge`` /
``remove_edges``); here a view is ``NormAdj.augmented``: one ``rsa_graph_dropout`` call that draws the mask, counts the
surviving degrees and writes the weights of the thinned, renormalised matrix and of its transpose into the base graph's CSR
layout, so the propagation over a view is the propagation kernel of LightGCN on other weights.

Which edges fall is defined by the device ``torch.rand`` stream in CSR edge order, not by ``dgl.DropEdge``'s stream (which
cannot be reproduced without dgl); the distribution is the same: every directed edge is dropped independently with
``dropout_prob``.

The sequence half (the views of CL4SRec, :22-97, the in-batch InfoNCE, :324-376, and ``CL4SRecAugmentation``, :573-606) is at the
end of this file, under "sequence views".
"""
import random

import torch
import torch.nn.functional as F

from .gather import _EmbedFn
from .scorer import full_lse

__all__ = ['EdgeDropout', 'NodeDropout', 'InfoNCELoss', 'SGLAugmentation', 'SimGCLAugmentation', 'Item_Crop', 'Item_Mask',
           'Item_Reorder', 'Item_Random', 'seq_augment_torch', 'sub_lengths', 'sub_table', 'batch_infonce', 'batch_infonce_torch', 'batch_infonce_kernel_ok',
           'BatchInfoNCELoss', 'seq_mean_pool', 'CL4SRecAugmentation']


class EdgeDropout(torch.nn.Module):
    """data_augmentation.py:229-263 on a ``graphmodule.NormAdj``: every directed edge falls with ``dropout_prob``; the result
    is a ``graphmodule.AugmentedAdj``.  In ``eval()`` the input comes back, as in the reference."""

    def __init__(self, dropout_prob, num_users, num_items):
        super().__init__()
        self.keep_prob = 1.0 - dropout_prob

    def forward(self, X, generator=None):
        if not self.training:
            return X
        return X.augmented(self.keep_prob, generator=generator)


class NodeDropout(torch.nn.Module):
    """data_augmentation.py:265-304: ``int(num_users * p)`` users and ``int(num_items * p)`` items, chosen by two
    ``torch.randperm`` calls on the CPU generator exactly as the reference chooses them, lose every edge."""

    def __init__(self, dropout_prob, num_users, num_items):
        super().__init__()
        self.num_users, self.num_items, self.dropout_prob = num_users, num_items, dropout_prob

    def nodes_flag(self):
        flag = torch.zeros(self.num_users + self.num_items, dtype=torch.bool)
        user_drop_indices = torch.randperm(self.num_users)[:int(self.num_users * self.dropout_prob)]
        item_drop_indices = torch.randperm(self.num_items)[:int(self.num_items * self.dropout_prob)]
        flag[user_drop_indices] = True
        flag[item_drop_indices + self.num_users] = True
        return flag

    def forward(self, X):
        if not self.training:
            return X
        return X.augmented(1.0, node_drop=self.nodes_flag())


class InfoNCELoss(torch.nn.Module):
    """data_augmentation.py:307-400 for ``neg_type='all'`` (what the graph models use):
    ``mean(logsumexp_n <i, all_n> / T - <i, j> / T)``, under ``'cosine'`` on the normalised rows.  The logsumexp runs over a whole
    table without the [B, N] matrix (``scorer.full_lse``, forward and backward); ``all_reps`` is therefore given as the WHOLE
    table, whose row 0 -- the padding row -- ``full_lse`` skips: the reference's ``all_reps=table[1:]``."""

    def __init__(self, temperature=1.0, sim_method='inner_product', neg_type='batch_both'):
        super().__init__()
        if sim_method not in ('inner_product', 'cosine'):
            raise ValueError(f"InfoNCELoss: sim_method must be 'inner_product' or 'cosine', got {sim_method!r}")
        if neg_type not in ('batch_both', 'batch_single', 'all'):
            raise ValueError(f'{neg_type} is not supported, neg_type should be "batch" or "all".')
        self.temperature, self.sim_method, self.neg_type = temperature, sim_method, neg_type

    def forward(self, augmented_rep_i, augmented_rep_j, instance_labels=None, all_reps=None):
        if self.neg_type != 'all':
            raise NotImplementedError(f"InfoNCELoss: neg_type {self.neg_type!r} contrasts inside the batch; it belongs to the "
                                      "sequence models (CL4SRec, ICLRec, CoSeRec), which this package does not have yet")
        if all_reps is None or instance_labels is not None:
            raise ValueError("InfoNCELoss: neg_type 'all' takes all_reps (the whole table) and no instance_labels")
        if self.sim_method == 'cosine':
            augmented_rep_i = F.normalize(augmented_rep_i, p=2, dim=-1)
            augmented_rep_j = F.normalize(augmented_rep_j, p=2, dim=-1)
            all_reps = F.normalize(all_reps, p=2, dim=-1)
        query = augmented_rep_i / self.temperature
        sim_ii = (query * augmented_rep_j).sum(dim=-1)
        return torch.mean(full_lse(query, all_reps.contiguous()) - sim_ii)


def _contrast(loss_fn, view1, view2, uid, iid):
    """``view1`` / ``view2``: the (user table, item table) of the two propagations -> the InfoNCE of the rows ``uid`` of the
    user tables plus that of the rows ``iid`` of the item tables, each against the whole second table (its row 0 is skipped)."""
    # the batch rows through the gather / sorted-scatter node, not index_add
    user_cl_loss, item_cl_loss = (loss_fn(_EmbedFn.apply(t1, idx), _EmbedFn.apply(t2, idx), all_reps=t2)
                                  for t1, t2, idx in zip(view1, view2, (uid, iid)))
    return user_cl_loss + item_cl_loss


class SGLAugmentation(torch.nn.Module):
    """data_augmentation.py:403-450: two views of the graph per step (``aug_type`` 'ED' edge dropout, 'ND' node dropout, 'RW' one
    edge-dropout graph per layer), the base tables propagated through each, and InfoNCE (cosine, all nodes as negatives)
    between the two views of the batch's users and of its items.  ``last_views`` keeps the step's two views."""

    def __init__(self, config, train_data):
        super().__init__()
        self.config = config
        self.fiid, self.fuid = train_data.fiid, train_data.fuid
        self.num_users, self.num_items = train_data.num_users, train_data.num_items
        aug_type = self.config['aug_type']
        if aug_type in ('ED', 'RW'):
            self.augmentation = EdgeDropout(self.config['ssl_ratio'], self.num_users, self.num_items)
        elif aug_type == 'ND':
            self.augmentation = NodeDropout(self.config['ssl_ratio'], self.num_users, self.num_items)
        else:
            raise ValueError(f"SGLAugmentation: aug_type must be 'ED', 'ND' or 'RW', got {aug_type!r}")
        self.InfoNCELoss_fn = InfoNCELoss(temperature=self.config['temperature'], sim_method='cosine', neg_type='all')
        self.last_views = None

    def draw_view(self, adj_mat, gnn_net):
        if self.config['aug_type'] == 'RW':
            return [self.augmentation(adj_mat) for _ in range(gnn_net.n_layers)]
        return self.augmentation(adj_mat)

    def get_gnn_embeddings(self, user_emb, item_emb, adj_mat, gnn_net):
        adj_mat.to(user_emb.weight.device)
        view = self.draw_view(adj_mat, gnn_net)
        embeddings = torch.cat([user_emb.weight, item_emb.weight], dim=0)
        all_embeddings = gnn_net.propagate(view, embeddings)
        return all_embeddings[:self.num_users], all_embeddings[self.num_users:], view

    def forward(self, batch, user_emb, item_emb, adj_mat, gnn_net):
        *tables1, view1 = self.get_gnn_embeddings(user_emb, item_emb, adj_mat, gnn_net)
        *tables2, view2 = self.get_gnn_embeddings(user_emb, item_emb, adj_mat, gnn_net)
        self.last_views = (view1, view2)
        return {'cl_loss': _contrast(self.InfoNCELoss_fn, tables1, tables2, batch[self.fuid], batch[self.fiid])}


class SimGCLAugmentation(torch.nn.Module):
    """data_augmentation.py:524-570: two PERTURBED propagations of the base tables over the full graph
    (``graphmodule.SimGCLNet.propagate(perturbed=True)``: every layer output moved by ``eps`` along a random direction of its own
    sign pattern), and InfoNCE (cosine, all nodes as negatives) between the two views of the batch's unique users and of its
    unique items.  The device stream takes L ``rand_like`` calls for view 1, then L for view 2.  Only ``cl_neg_type: 'all'``
    exists here; the in-batch forms of ``InfoNCELoss`` are not implemented and are refused at construction.  ``torch.unique`` is
    the reference's semantics (its host sync is accepted)."""

    def __init__(self, config, train_data):
        super().__init__()
        self.config = config
        self.fiid, self.fuid = train_data.fiid, train_data.fuid
        self.num_users, self.num_items = train_data.num_users, train_data.num_items
        if self.config['cl_neg_type'] != 'all':
            raise NotImplementedError(f"SimGCLAugmentation: cl_neg_type {self.config['cl_neg_type']!r} contrasts inside the batch; only "
                                      "'all' (every node as a negative) is implemented")
        self.InfoNCELoss_fn = InfoNCELoss(temperature=self.config['temperature'], sim_method='cosine', neg_type='all')

    def get_gnn_embeddings(self, user_emb, item_emb, adj_mat, gnn_net):
        adj_mat.to(user_emb.weight.device)
        embeddings = torch.cat([user_emb.weight, item_emb.weight], dim=0)
        all_embeddings = gnn_net.propagate(adj_mat, embeddings, perturbed=True)
        return all_embeddings[:self.num_users], all_embeddings[self.num_users:]

    def forward(self, batch, user_emb, item_emb, adj_mat, gnn_net):
        device = user_emb.weight.device
        u_idx = torch.unique(batch[self.fuid]).to(device)
        i_idx = torch.unique(batch[self.fiid]).to(device)
        tables1 = self.get_gnn_embeddings(user_emb, item_emb, adj_mat, gnn_net)
        tables2 = self.get_gnn_embeddings(user_emb, item_emb, adj_mat, gnn_net)
        return {'cl_loss': _contrast(self.InfoNCELoss_fn, tables1, tables2, u_idx, i_idx)}


# ---------------------------------------------------------------------------------------------------------------- sequence views
# Host-side mirror of the sequence half of the reference's data_augmentation (:22-97 the augmentations, :307-376 the in-batch
# InfoNCE, :573-606 CL4SRecAugmentation).
#
# THE RULE OF A VIEW (``ops.seq_augment`` / ``rsa_seq_augment`` in one launch; ``seq_augment_torch`` is the same rule in batched torch
# ops).  ``U = torch.rand([B, L + 1])`` on the device generator; ``U[b, 0]`` draws the start, ``U[b, 1 + p]`` is the key of position p.
#   len = clamp(seqlen[b], 0, L)   n_sub = sub[len]   span = max(len - n_sub + 1, 1)   start = min(int(U[b, 0] * float(span)), span - 1)
#   crop    : out[b, p] = seq[b, start + p] for p < n_sub, else 0;                                            new_len = n_sub
#   mask    : positions p < len ranked by their keys (ties to the lower position); mask_id where rank < n_sub;  new_len = len
#   reorder : the positions of [start, start + n_sub) ranked among themselves; out[b, start + rank(p)] = seq[b, p]; new_len = len
#   a row with len = 0 comes back unchanged with new_len = 0.
# ``sub`` is the table len -> n_sub, built in Python float64 with the reference's own expressions (``sub_table``).
#
# TWO DELIBERATE DEVIATIONS.  (1) The random choices follow the device ``torch.rand`` stream, not the reference's three host
# generators (``torch.randint`` on the CPU, ``np.random.choice``, ``random.shuffle``) behind a ``.item()`` per sequence: 2 B
# device synchronisations per step for the two views.  The distributions are the same: a uniform start, a uniform subset, a uniform
# order.  (2) A cropped batch keeps its width L where ``pad_sequence`` narrows it to the longest crop; the encoder's output on
# the kept positions is the same (padded keys are masked, positions count from 0).
SEQ_AUGMENT_KINDS = ('crop', 'mask', 'reorder')
_SUB_TABLES = {}


def sub_lengths(kind, rate, L):
    """``[n_sub(0), ..., n_sub(L)]`` as Python ints, in float64 with the reference's expressions: crop ``max(1, int(tau n))``
    (data_augmentation.py:36), mask ``int(gamma n)`` (:59), reorder ``int(beta n)`` (:80); ``n_sub(0) = 0``."""
    if kind not in SEQ_AUGMENT_KINDS:
        raise ValueError(f"sub_lengths: kind must be one of {SEQ_AUGMENT_KINDS}, got {kind!r}")
    rate = float(rate)
    if kind == 'crop':
        return [0] + [min(n, max(1, int(rate * n))) for n in range(1, int(L) + 1)]
    return [0] + [min(n, max(0, int(rate * n))) for n in range(1, int(L) + 1)]


def sub_table(kind, rate, L, device='cpu'):
    """``sub_lengths`` as an int32 tensor on ``device``, cached per (kind, rate, L, device)."""
    device = torch.device(device)
    if device.type == 'cuda' and device.index is None:
        device = torch.device('cuda', torch.cuda.current_device())
    key = (kind, float(rate), int(L), device)
    t = _SUB_TABLES.get(key)
    if t is None:
        if len(_SUB_TABLES) >= 64:
            _SUB_TABLES.clear()
        t = _SUB_TABLES[key] = torch.tensor(sub_lengths(kind, rate, L), dtype=torch.int32, device=device)
    return t


def seq_augment_torch(seq, seqlen, kind, sub, U, mask_id=0):
    """The rule above in batched torch ops (no Python loop over B, no synchronisation), on whatever device the tensors live.
    ``seq`` int64 [B, L], ``seqlen`` [B], ``sub`` int [L + 1], ``U`` fp32 [B, L + 1] -> ``(out [B, L], new_len [B])``."""
    if kind not in SEQ_AUGMENT_KINDS:
        raise ValueError(f"seq_augment_torch: kind must be one of {SEQ_AUGMENT_KINDS}, got {kind!r}")
    B, L = seq.shape
    if tuple(U.shape) != (B, L + 1) or sub.numel() != L + 1:
        raise ValueError(f'seq_augment_torch: U must be [{B}, {L + 1}] and sub hold {L + 1} entries')
    ln = seqlen.long().clamp(0, L)
    n_sub = torch.minimum(sub.long()[ln].clamp(min=0), ln)
    span = (ln - n_sub + 1).clamp(min=1)
    start = torch.minimum((U[:, 0] * span.to(torch.float32)).long(), span - 1)          # one fp32 product, truncated
    p = torch.arange(L, device=seq.device).unsqueeze(0)
    ln_, n_, st_ = ln.unsqueeze(1), n_sub.unsqueeze(1), start.unsqueeze(1)
    inf = torch.full((), float('inf'), dtype=U.dtype, device=U.device)
    if kind == 'crop':
        out = torch.where(p < n_, seq.gather(1, (st_ + p).clamp(max=L - 1)), torch.zeros_like(seq))
        out = torch.where(ln_ == 0, seq, out)
        return out, n_sub.to(seqlen.dtype)
    if kind == 'mask':
        keys = torch.where(p < ln_, U[:, 1:], inf)                                      # padded positions take no part
        rank = keys.argsort(dim=1, stable=True).argsort(dim=1, stable=True)             # ties to the lower position
        out = torch.where((p < ln_) & (rank < n_), torch.full_like(seq, mask_id), seq)
        return out, ln.to(seqlen.dtype)
    in_win = (p >= st_) & (p < st_ + n_)
    order = torch.where(in_win, U[:, 1:], inf).argsort(dim=1, stable=True)              # order[b, r]: the position of rank r
    src = torch.where(in_win, order.gather(1, (p - st_).clamp(0, L - 1)), p.expand(B, L))
    return seq.gather(1, src), ln.to(seqlen.dtype)


class _ItemAugment(torch.nn.Module):
    """One view per call: the kernel (``fused``, device tensors, L <= 64) or the twin fed ``torch.rand([B, L + 1])`` from the same
    generator state -- the same view either way.  Nothing special happens in ``eval()``: the reference augments regardless."""
    kind = None

    def __init__(self, rate, mask_id=0, fused=True):
        super().__init__()
        self.rate, self.mask_id, self.fused = rate, mask_id, bool(fused)

    def forward(self, sequences, seq_lens, generator=None):
        from . import ops
        B, L = sequences.shape
        sub = sub_table(self.kind, self.rate, L, sequences.device)
        if self.fused and sequences.is_cuda and 1 <= L <= ops.SEQ_AUGMENT_MAX_LEN:
            return ops.seq_augment(sequences, seq_lens, self.kind, sub, self.mask_id, generator=generator)
        U = torch.rand(B, L + 1, device=sequences.device, generator=generator)
        return seq_augment_torch(sequences, seq_lens, self.kind, sub, U, self.mask_id)


class Item_Crop(_ItemAugment):
    """data_augmentation.py:22-42: a contiguous slice of ``max(1, int(tao len))`` items from a uniform start."""
    kind = 'crop'

    def __init__(self, tao=0.2, fused=True):
        super().__init__(tao, fused=fused)
        self.tao = tao


class Item_Mask(_ItemAugment):
    """data_augmentation.py:45-63: a uniform subset of ``int(gamma len)`` positions becomes ``mask_id``."""
    kind = 'mask'

    def __init__(self, mask_id, gamma=0.7, fused=True):
        super().__init__(gamma, mask_id=mask_id, fused=fused)
        self.gamma = gamma


class Item_Reorder(_ItemAugment):
    """data_augmentation.py:66-87: a window of ``int(beta len)`` items from a uniform start, in a uniform order."""
    kind = 'reorder'

    def __init__(self, beta=0.2, fused=True):
        super().__init__(beta, fused=fused)
        self.beta = beta


class Item_Random(torch.nn.Module):
    """data_augmentation.py:89-97: one of the three per CALL (the whole batch), chosen by Python's ``random.randint(0, 2)`` on
    the host exactly as the reference chooses it."""

    def __init__(self, mask_id, tao=0.2, gamma=0.7, beta=0.2, fused=True):
        super().__init__()
        self.mask_id = mask_id
        self.augmentation_methods = torch.nn.ModuleList([Item_Crop(tao, fused), Item_Mask(mask_id, gamma, fused),
                                                         Item_Reorder(beta, fused)])
        self.last_choice = None

    @property
    def kind(self):
        """The kind of the LAST call."""
        return None if self.last_choice is None else self.augmentation_methods[self.last_choice].kind

    def forward(self, sequences, seq_lens, generator=None):
        self.last_choice = random.randint(0, len(self.augmentation_methods) - 1)
        return self.augmentation_methods[self.last_choice](sequences, seq_lens, generator=generator)


# ---------------------------------------------------------------------------------------------------------------- in-batch InfoNCE
def batch_infonce_torch(zi, zj, inv_t, both=True, labels=None):
    """The reference's op sequence for ``neg_type`` 'batch_both' / 'batch_single' (data_augmentation.py:324-376): matmuls, ``-inf``
    fill, ``cat``, ``cross_entropy`` -> the per-row ``lse - pos`` [B] (its mean is the loss).  Row b's logits are
    ``<zi_b, zj_k> inv_t`` for every k but those with ``k != b`` and ``labels[k] == labels[b]``, and with ``both`` also
    ``<zi_b, zi_k> inv_t`` for every ``k != b`` whose label differs (without labels: every ``k != b``).  Materialises [B, 2B]."""
    B = zi.shape[0]
    sim_ij = torch.matmul(zi, zj.T) * inv_t
    eye = torch.eye(B, dtype=torch.bool, device=zi.device)
    same = eye if labels is None else torch.eq(labels.unsqueeze(-1), labels)
    if labels is not None:
        sim_ij = sim_ij.masked_fill(same & ~eye, float('-inf'))
    logits = sim_ij
    if both:
        sim_ii = (torch.matmul(zi, zi.T) * inv_t).masked_fill(same | eye, float('-inf'))
        logits = torch.cat([sim_ij, sim_ii], dim=-1)
    target = torch.arange(B, dtype=torch.long, device=zi.device)
    return F.cross_entropy(logits, target, reduction='none')


class _BatchInfoNceFn(torch.autograd.Function):
    """``ops.batch_infonce`` / ``ops.batch_infonce_backward`` as one autograd node -> ``lse - pos`` [B].  Saved: the inputs and
    ``lse`` [B]; the backward recomputes the softmax."""

    @staticmethod
    def forward(ctx, zi, zj, inv_t, both, labels):
        from . import ops
        zi, zj = zi.contiguous(), zj.contiguous()
        lse, pos = ops.batch_infonce(zi, zj, inv_t, both, labels)
        ctx.save_for_backward(zi, zj, lse, *(() if labels is None else (labels,)))
        ctx.inv_t, ctx.both = inv_t, both
        return lse - pos

    @staticmethod
    def backward(ctx, g):
        from . import ops
        zi, zj, lse, *rest = ctx.saved_tensors
        dzi, dzj = ops.batch_infonce_backward(zi, zj, ctx.inv_t, ctx.both, rest[0] if rest else None, lse, g.contiguous())
        return dzi, dzj, None, None, None


def batch_infonce_kernel_ok(zi, zj):
    """Whether ``ops.batch_infonce`` takes these tensors: fp32 [B, d] on the device, d in ``ops.BATCH_INFONCE_DIMS``, B >= 1."""
    from . import ops
    return (zi.is_cuda and zj.is_cuda and zi.dtype == zj.dtype == torch.float32 and zi.dim() == 2 and zi.shape == zj.shape
            and zi.shape[1] in ops.BATCH_INFONCE_DIMS and zi.shape[0] >= 1)


def batch_infonce(zi, zj, inv_t, both=True, labels=None, fused=True):
    """The per-row in-batch InfoNCE ``lse - pos`` [B]: the fused kernels where ``fused`` and ``batch_infonce_kernel_ok`` (nothing
    of size B^2, forward or backward), ``batch_infonce_torch`` otherwise (CPU tensors, other widths, float64)."""
    if fused and batch_infonce_kernel_ok(zi, zj):
        return _BatchInfoNceFn.apply(zi, zj, float(inv_t), bool(both), labels)
    return batch_infonce_torch(zi, zj, inv_t, both, labels)


class BatchInfoNCELoss(torch.nn.Module):
    """data_augmentation.py:307-376 for ``neg_type`` 'batch_both' / 'batch_single': the contrast inside the batch that
    ``InfoNCELoss`` here refuses.  ``instance_labels`` ([B] int64, ICLRec's de-noising): rows with the same label are not each
    other's negatives.  ``fused``: the HIP kernels (``batch_infonce``: no [B, 2B] matrix, forward or backward) where they take the
    tensors; off by default, as ``model.fused_infonce`` is (slower than the op sequence at B = 8192)."""

    def __init__(self, temperature=1.0, sim_method='inner_product', neg_type='batch_both', fused=False):
        super().__init__()
        self.fused = bool(fused)
        if sim_method not in ('inner_product', 'cosine'):
            raise ValueError(f"BatchInfoNCELoss: sim_method must be 'inner_product' or 'cosine', got {sim_method!r}")
        if neg_type not in ('batch_both', 'batch_single'):
            raise ValueError(f"BatchInfoNCELoss: neg_type must be 'batch_both' or 'batch_single', got {neg_type!r} "
                             "('all' is InfoNCELoss)")
        if not float(temperature) > 0:
            raise ValueError(f'BatchInfoNCELoss: temperature must be positive, got {temperature}')
        self.temperature, self.sim_method, self.neg_type = float(temperature), sim_method, neg_type

    def forward(self, augmented_rep_i, augmented_rep_j, instance_labels=None, all_reps=None):
        if all_reps is not None:
            raise ValueError("BatchInfoNCELoss: all_reps belongs to neg_type 'all' (InfoNCELoss)")
        if augmented_rep_i.dim() != 2 or augmented_rep_i.shape != augmented_rep_j.shape:
            raise ValueError('BatchInfoNCELoss: the two views must be [B, d] of one shape, got '
                             f'{tuple(augmented_rep_i.shape)} and {tuple(augmented_rep_j.shape)}')
        if instance_labels is not None and tuple(instance_labels.shape) != (augmented_rep_i.shape[0],):
            raise ValueError('BatchInfoNCELoss: instance_labels must hold one label per row')
        if self.sim_method == 'cosine':
            augmented_rep_i = F.normalize(augmented_rep_i, p=2, dim=-1)
            augmented_rep_j = F.normalize(augmented_rep_j, p=2, dim=-1)
        return batch_infonce(augmented_rep_i, augmented_rep_j, 1.0 / self.temperature, self.neg_type == 'batch_both',
                             instance_labels, fused=self.fused).mean()


def seq_mean_pool(out, seq_len):
    """``seq_pooling_function(..., 'mean')`` (recstudio/model/module/functional.py): positions ``>= len`` zeroed, summed, divided
    by ``len`` (a row of length 0 divides by zero, as in the reference)."""
    L = out.shape[1]
    keep = torch.arange(L, device=out.device).unsqueeze(0) < seq_len.unsqueeze(1)
    return (out * keep.unsqueeze(-1).to(out.dtype)).sum(1) / seq_len.unsqueeze(-1).to(out.dtype)


class CL4SRecAugmentation(torch.nn.Module):
    """data_augmentation.py:573-606: two views of every history (both drawn before either is encoded, as in the reference), each
    through the query encoder without pooling, mean-pooled over its ``new_len`` positions, and the in-batch InfoNCE
    ('inner_product', 'batch_both') between the two.  ``mask_id = num_items``.  ``last_views`` keeps the step's
    ``((seq_i, len_i), (seq_j, len_j))``."""

    def __init__(self, config, train_data):
        super().__init__()
        self.config = config
        self.fiid = train_data.fiid
        fused = bool(config.get('fused_augment', True))
        kind = config['augment_type']
        if kind == 'item_crop':
            self.augmentation = Item_Crop(config['tau'], fused=fused)
        elif kind == 'item_mask':
            self.augmentation = Item_Mask(mask_id=train_data.num_items, fused=fused)
        elif kind == 'item_reorder':
            self.augmentation = Item_Reorder(fused=fused)
        elif kind == 'item_random':
            self.augmentation = Item_Random(mask_id=train_data.num_items, tao=config['tau'], fused=fused)
        else:
            raise ValueError(f"CL4SRecAugmentation: augment_type must be 'item_crop', 'item_mask', 'item_reorder' or 'item_random', "
                             f"got {kind!r}")
        self.InfoNCE_loss_fn = BatchInfoNCELoss(temperature=config['temperature'], sim_method='inner_product', neg_type='batch_both',
                                                fused=bool(config.get('fused_infonce', False)))
        self.last_views = None

    def forward(self, batch, query_encoder):
        seq, seqlen = batch['in_' + self.fiid], batch['seqlen']
        views = []
        for _ in range(2):
            ids, ln = self.augmentation(seq, seqlen)
            views.append((ids, ln))
        self.last_views = tuple(views)
        reps = []
        for ids, ln in views:
            # (the encoder swaps mask_id for its own mask_emb row: no id outside the catalog reaches the gather)
            out = query_encoder({'in_' + self.fiid: ids, 'seqlen': ln}, need_pooling=False)
            reps.append(seq_mean_pool(out, ln))
        return {'cl_loss': self.InfoNCE_loss_fn(reps[0], reps[1])}
