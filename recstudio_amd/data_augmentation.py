"""Graph augmentation -- host-side mirror of the graph half of ``recstudio.model.module.data_augmentation`` (:229-450 for SGL,
:524-570 for SimGCL, whose views are not thinned graphs but noise in the propagation: ``graphmodule.SimGCLNet``).

The reference copies its ``dgl`` graph and thins the copy once per view per step (``copy.deepcopy`` + ``dgl.DropEdge`` /
``remove_edges``); here a view is ``NormAdj.augmented``: one ``rsa_graph_dropout`` call that draws the mask, counts the
surviving degrees and writes the weights of the thinned, renormalised matrix and of its transpose into the base graph's CSR
layout, so the propagation over a view is the propagation kernel of LightGCN on other weights.

Which edges fall is defined by the device ``torch.rand`` stream in CSR edge order, not by ``dgl.DropEdge``'s stream (which
cannot be reproduced without dgl); the distribution is the same: every directed edge is dropped independently with
``dropout_prob``.
"""
import torch
import torch.nn.functional as F

from .scorer import full_lse

__all__ = ['EdgeDropout', 'NodeDropout', 'InfoNCELoss', 'SGLAugmentation', 'SimGCLAugmentation']


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
    from .retriever import _EmbedFn
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
