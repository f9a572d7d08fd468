"""The matrix-factorisation family beyond BPR: NCF, WRMF, ItemKNN, EASE."""
import time

import torch

from . import ops
from .dataset import ALSDataset

from .loss_func import BinaryCrossEntropyLoss
from .retriever import BaseRetriever
from .sampler import UniformSampler
from .scorer import FusionMFMLPScorer, GMFScorer, InnerProductScorer, MLPScorer
from .seqmodule import MLPModule

__all__ = ['NCF', 'FUSED_SCORER_DEFAULT', 'WRMF', 'FUSED_ALS_DEFAULT', 'als_step_torch', 'ItemKNN', 'FUSED_KNN_DEFAULT',
           'itemknn_torch', 'itemknn_score_torch', 'EASE', 'FUSED_EASE_DEFAULT', 'ease_torch', 'ease_score_torch']

# model.fused_scorer: the pair scorers run in rsa_pair_mlp (forward, backward, range-mode top-k) instead of torch ops.  Off:
# tools/bench_ncf.py (profiles/ncf_bench.json) has the kernel ahead in every forward and behind in every forward + backward.
FUSED_SCORER_DEFAULT = False


class NCF(BaseRetriever):
    """recstudio/model/mf/ncf.py:6-45, recstudio/model/mf/config/ncf.yaml (activation relu, dropout 0.1, mlp_hidden_size
    [128, 64], score_mode fusion, negative_count 1, excluding_hist False).  ``score_mode`` 'mlp' -> ``MLPScorer`` over
    ``MLPModule([2d] + hidden + [1])``, 'mf' -> ``GMFScorer``, 'fusion' -> ``FusionMFMLPScorer``; BinaryCrossEntropyLoss over
    uniform negatives.  With ``model.fused_scorer`` the positives' and negatives' ids go to the pair kernel as given ids (no
    [B, n, d] tensor) and ``topk`` walks the catalog through its range mode.

    The device generator of a training step is consumed in this order: the negatives, then ONE ``torch.rand([B (1 + n), C])`` for
    every dropout mask of the step (the reference draws its masks with nn.Dropout's kernel, separately for the positives and the
    negatives: which elements fall differs, how many does not)."""

    config_defaults = {'model': {'activation': 'relu', 'dropout': 0.1, 'mlp_hidden_size': [128, 64], 'score_mode': 'fusion',
                                 'fused_scorer': FUSED_SCORER_DEFAULT},
                       'train': {'negative_count': 1, 'excluding_hist': False}}

    def _get_item_encoder(self, train_data):
        return torch.nn.Embedding(train_data.num_items, self.embed_dim, padding_idx=0)

    def _get_query_encoder(self, train_data):
        return torch.nn.Embedding(train_data.num_users, self.embed_dim, padding_idx=0)

    def _get_score_func(self):
        model = self.config['model']
        mode = model['score_mode']
        assert mode in ('mlp', 'mf', 'fusion'), "Only 3 score modes are supported for NCF: ['mlp', 'mf', 'fusion']"
        hidden = list(model['mlp_hidden_size'])
        if mode == 'mf':
            return GMFScorer(self.embed_dim, activation=model['activation'])
        if mode == 'mlp':
            scorer = MLPScorer(MLPModule([self.embed_dim * 2] + hidden + [1], model['activation'], model['dropout']))
        else:
            mlp = MLPModule([self.embed_dim * 2] + hidden, model['activation'], model['dropout'])
            scorer = FusionMFMLPScorer(self.embed_dim, hidden[-1], mlp, activation=model['activation'])
        scorer.fused = bool(model.get('fused_scorer', FUSED_SCORER_DEFAULT))
        return scorer

    def _get_loss_func(self):
        return BinaryCrossEntropyLoss()

    def _get_sampler(self, train_data):
        return UniformSampler(train_data.num_items)


# model.fused_als: the half-epochs run in rsa_als_solve instead of the padded gather / bmm / torch.linalg.solve sequence.  Off:
# tools/bench_wrmf.py (profiles/wrmf_bench.json) has the kernel ahead at d = 64 and behind the large-batch reference at d = 128.
FUSED_ALS_DEFAULT = False


def als_step_torch(ids, ratings, table, gram, alpha, lam, item_bias=False):
    """The reference's op sequence for one padded batch (recstudio/model/mf/wrmf.py:53-80): ``ids`` [B, L] (0 pads, and row 0 of the
    table is read for them as the reference does), ``ratings`` [B, L] -> ``(x [B, d], loss [B])``."""
    rated = (ratings > 0).to(table.dtype)
    emb = table[ids]                                                            # B x L x d
    eye = lam * torch.eye(table.shape[1], dtype=table.dtype, device=table.device)
    A = torch.bmm(emb.transpose(1, 2), emb) * alpha + (gram + eye)
    r = torch.bmm(emb.transpose(1, 2), rated.unsqueeze(-1)).squeeze(-1)
    x = torch.linalg.solve(A, r * (alpha + 1))
    if item_bias:
        x[:, -1] = 1.0
    pred = (x.unsqueeze(1) * emb).sum(-1)
    loss = ((rated - pred) ** 2).sum(-1) * (alpha + 1) - (pred ** 2).sum(-1) + ((x @ gram) * x).sum(-1)
    return x, loss


class WRMF(BaseRetriever):
    """recstudio/model/mf/wrmf.py, recstudio/model/mf/config/wrmf.yaml (alpha 1, lambda 0.5, batch_size 100): implicit-feedback
    alternating least squares.  Both towers are frozen ``nn.Embedding`` tables; there is no sampler, loss function or optimizer.
    Even epochs solve every user against the item table, odd epochs every item against the user table (the reference's
    ``nepoch % 2`` loader choice); ``gram`` is recomputed at the start of each epoch and the reported loss is the mean of the rows'
    losses.  ``model.fused_als``: a half-epoch is ONE ``ops.als_solve`` over the CSR of the train split (the other table is fixed
    within an epoch, so the rows are independent); off, it is ``als_step_torch`` over the padded host batches.  Rows without a
    training interaction keep their initial values on both paths.  ``model.item_bias``: the last column of the solved user rows
    is set to 1 and the loss is taken with that x (wrmf.py:61-63)."""

    config_defaults = {'model': {'item_bias': False, 'fused_als': FUSED_ALS_DEFAULT},
                       'train': {'alpha': 1.0, 'lambda': 0.5, 'batch_size': 100}}

    @staticmethod
    def _get_dataset_class():
        return ALSDataset

    def _get_item_encoder(self, train_data):
        return torch.nn.Embedding(train_data.num_items, self.embed_dim, padding_idx=0)

    def _get_query_encoder(self, train_data):
        return torch.nn.Embedding(train_data.num_users, self.embed_dim, padding_idx=0)

    def _get_score_func(self):
        return InnerProductScorer()

    def _get_loss_func(self):
        return None

    def _get_sampler(self, train_data):
        return None

    def _init_parameter(self):
        super()._init_parameter()
        self.query_encoder.weight.requires_grad = False
        self.item_encoder.weight.requires_grad = False

    def _als_setup(self, train_data, device):
        self._als_data = train_data
        if self.config['model']['fused_als']:
            self._als_csr = [tuple(t.to(device) for t in side) + (ops.als_max_parts(side[0]),) for side in train_data.csr()]
        else:
            self._als_loaders = [train_data, train_data.transpose()]

    def _als_half_epoch(self, nepoch):
        """Solves the users (even ``nepoch``) or the items (odd) against the other table; -> the mean row loss."""
        tr, users = self.config['train'], nepoch % 2 == 0
        bias = bool(self.config['model']['item_bias']) and users
        target = (self.query_encoder if users else self.item_encoder).weight.data
        table = (self.item_encoder if users else self.query_encoder).weight.data
        gram = table.T @ table
        if self.config['model']['fused_als']:
            indptr, ids, ratings, max_parts = self._als_csr[nepoch % 2]
            rated = (ratings > 0).float()
            x, loss, _ = ops.als_solve(indptr, ids, table, gram, tr['alpha'], tr['lambda'], rated=rated, want_loss=not bias,
                                       max_parts=max_parts)
            if bias:
                x[:, -1] = 1.0
                loss = ops.als_solve(indptr, ids, table, gram, tr['alpha'], tr['lambda'], rated=rated, x=x)[1]
            seen = indptr[1:] > indptr[:-1]
            target[seen] = x[seen]
            return float(loss[seen].mean())
        data = self._als_loaders[nepoch % 2]
        losses = []
        for batch in data.train_loader(batch_size=tr['batch_size'], shuffle=True, drop_last=False):
            batch = self._to_device(batch, table.device)
            x, loss = als_step_torch(batch[data.fiid], batch[data.frating], table, gram, tr['alpha'], tr['lambda'], bias)
            target[batch[data.fuid]] = x
            losses.append(loss)
        return float(torch.cat(losses).mean())

    def fit(self, train_data, val_data=None, run_mode='light', config=None, **kwargs):
        if config is not None:
            self.config.update(config)
        if self._dist_context(kwargs) is not None:
            raise NotImplementedError('WRMF: the sharded fit is not covered (an ALS half-epoch needs the whole other table on one device)')
        self._init_model(train_data)
        self._init_parameter()
        device = self._device()
        self.to(device)
        if val_data is not None:
            val_data.use_field = train_data.use_field
        self._als_setup(train_data, device)
        epoch = [0]

        def train_epoch():
            epoch[0] += 1
            return self._als_half_epoch(epoch[0] - 1)

        def validate():
            t1 = time.time()
            metrics = self._eval_epoch(val_data, self.validation_step, device)
            return dict(metrics, valid_time=time.time() - t1)

        return self._run_epochs(train_epoch, None, validate if val_data is not None else None, log=self.logger.info)


# model.fused_knn: the neighbour build and the scores run in rsa_knn_build / rsa_knn_score instead of itemknn_torch /
# itemknn_score_torch.  On: tools/bench_itemknn.py (profiles/itemknn_bench.json) at about ml-20m's shape has the build at 10.9 ms
# against 1856 ms and a top-k batch (B = 512, k = 100) at 1.03 ms against 56.7 ms; at about ml-1m's 0.34 / 2.12 and 0.28 / 11.2 ms.
FUSED_KNN_DEFAULT = True
_KNN_BUFFERS = ('nbr_id', 'nbr_sim', 'nbr_cnt', 't_indptr', 't_items', 't_sim', 'user_indptr', 'user_items')


def _interaction_csrs(train_data, device, who):
    """The unit-valued interaction graph of a train split on ``device``: ``(users, items, n_users, n_items, (u_indptr, u_items),
    (i_indptr, i_users))``, both CSRs with int64 row pointers and int32 ids ascending within a row."""
    if not train_data.drop_dup:
        raise ValueError(f'{who}: the interaction graph is unit-valued; drop_dup: False (repeated pairs) is not covered')
    (users, items, _, (n_users, n_items)), _ = train_data.get_graph([0])
    users, items = users.to(device), items.to(device)

    def csr(key, val, n):                                            # ids ascending within a row
        order = torch.sort(key * (int(val.max()) + 1 if val.numel() else 1) + val).indices
        return torch.cat([key.new_zeros(1), torch.cumsum(torch.bincount(key, minlength=n), 0)]), val[order].to(torch.int32)
    return users, items, n_users, n_items, csr(users, items, n_users), csr(items, users, n_items)


def itemknn_torch(users, items, n_users, n_items, knn, similarity, dtype=torch.float32, chunk=2048):
    """The torch-op twin of ``ops.knn_build`` (recstudio/model/mf/itemknn.py:12-41): the dense ``R^T R`` in column chunks, the same
    formula in ``dtype``, and the ``min(knn, nnz)`` largest of each column.  ``users`` / ``items``: the interactions, one id pair each,
    no duplicates.  A stable descending sort stands where the reference has ``argpartition``: it is what decides ties by the lower
    id.  -> ``(nbr_id int32 [N, knn], nbr_sim dtype [N, knn], nbr_cnt int32 [N])`` as the kernel lays them out."""
    if similarity not in ops.KNN_SIMILARITIES:
        raise ValueError('unsupported similarity metric')
    dev = users.device
    R = torch.zeros(n_users, n_items, dtype=dtype, device=dev)
    R[users.long(), items.long()] = 1
    n = R.sum(0)
    root = torch.sqrt(n)
    width = min(int(knn), n_items)
    nbr_id = torch.full((n_items, knn), -1, dtype=torch.int32, device=dev)
    nbr_sim = torch.zeros(n_items, knn, dtype=dtype, device=dev)
    nbr_cnt = torch.zeros(n_items, dtype=torch.int32, device=dev)
    for s in range(0, n_items, chunk):
        e = min(s + chunk, n_items)
        c = R[:, s:e].T @ R                                            # [C, N]: row r is column s + r of the Gram matrix
        c[torch.arange(e - s, device=dev), torch.arange(s, e, device=dev)] = 0
        if similarity == 'cosine':
            sim = c / (root[None] * root[s:e, None] + 1e-6)
        else:
            sim = c / (n[None] + n[s:e, None] - c + 1e-6)
        val, idx = torch.sort(sim, dim=1, descending=True, stable=True)
        val, idx = val[:, :width], idx[:, :width]
        live = val > 0
        nbr_cnt[s:e] = live.sum(1).to(torch.int32)
        nbr_id[s:e, :width] = torch.where(live, idx, -1).to(torch.int32)
        nbr_sim[s:e, :width] = val
    nbr_cnt[0], nbr_id[0], nbr_sim[0] = 0, -1, 0                       # the padding item is nobody's target
    return nbr_id, nbr_sim, nbr_cnt


def itemknn_score_torch(users, indptr, items, t_indptr, t_items, t_sim, n_items):
    """The torch-op twin of ``ops.knn_score``: every (user, history item j, target of row j) triple is expanded and summed with
    ``index_put_(accumulate=True)``.  Same values up to the order of the sums."""
    users = users.long()
    start, deg = indptr[users], indptr[users + 1] - indptr[users]
    b = torch.repeat_interleave(torch.arange(users.numel(), device=users.device), deg)
    pos = torch.arange(b.numel(), device=users.device) - torch.repeat_interleave(torch.cumsum(deg, 0) - deg, deg)
    j = items[start[b] + pos].long()
    t_start, t_deg = t_indptr[j], t_indptr[j + 1] - t_indptr[j]
    bb = torch.repeat_interleave(b, t_deg)
    at = torch.repeat_interleave(t_start, t_deg) + (torch.arange(bb.numel(), device=users.device)
                                                    - torch.repeat_interleave(torch.cumsum(t_deg, 0) - t_deg, t_deg))
    out = torch.zeros(users.numel(), n_items, dtype=t_sim.dtype, device=users.device)
    out.index_put_((bb, t_items[at].long()), t_sim[at], accumulate=True)
    return out[:, 1:]


class ItemKNN(BaseRetriever):
    """recstudio/model/mf/itemknn.py, recstudio/model/mf/config/itemknn.yaml (knn 100, similarity cosine | jaccard): the item-based
    neighbourhood baseline.  There is nothing to learn: ``fit`` builds, once, the ``knn`` most similar items of every item from the
    co-occurrence counts of the train split, and a user's score of item i is the sum of sim(j -> i) over the user's train items j
    that are among i's neighbours.  No sampler, loss, optimizer or encoder; the neighbour lists, their transpose and the user-side
    CSR are buffers, so ``state_dict`` carries the fitted model.  ``model.fused_knn``: ``ops.knn_build`` / ``ops.knn_score``; off,
    ``itemknn_torch`` / ``itemknn_score_torch``.  Where the reference's ``argpartition`` leaves ties open, the lower item id wins."""

    config_defaults = {'model': {'fused_knn': FUSED_KNN_DEFAULT}, 'train': {'knn': 100, 'similarity': 'cosine', 'epochs': 1}}

    def _get_item_encoder(self, train_data):
        return None

    def _get_query_encoder(self, train_data):
        return None

    def _get_loss_func(self):
        return None

    def _get_sampler(self, train_data):
        return None

    def _update_item_vector(self):
        pass                                                              # the "item vector" is the sparse neighbour matrix

    def _knn_build(self, train_data, device):
        tr = self.config['train']
        if tr['similarity'] not in ops.KNN_SIMILARITIES:
            raise ValueError('unsupported similarity metric')
        users, items, n_users, n_items, (u_indptr, u_items), (i_indptr, i_users) = _interaction_csrs(train_data, device, 'ItemKNN')
        if self.config['model']['fused_knn']:
            nbr = ops.knn_build(u_indptr, u_items, i_indptr, i_users, tr['knn'], tr['similarity'])
        else:
            nbr = itemknn_torch(users, items, n_users, n_items, tr['knn'], tr['similarity'])
        for name, t in zip(_KNN_BUFFERS, nbr + ops.knn_transpose(*nbr) + (u_indptr, u_items)):
            self.register_buffer(name, t)

    def load_state_dict(self, state_dict, strict=True):
        for name in _KNN_BUFFERS:                                        # a fresh model has no lists yet: take their shapes from the state
            if name in state_dict:
                self.register_buffer(name, torch.empty_like(state_dict[name]))
        return super().load_state_dict(state_dict, strict)

    def topk(self, batch, k, user_h=None, return_query=False):
        """baseretriever.py:374-397 over the neighbour scores: top (k + |hist|), ids + 1, the history dropped, top k."""
        users = (batch[self.fuid] if isinstance(batch, dict) else batch).to(self.nbr_cnt.device)
        n_items = self.nbr_cnt.numel()
        score_fn = ops.knn_score if self.config['model']['fused_knn'] else itemknn_score_torch
        scores = score_fn(users, self.user_indptr, self.user_items, self.t_indptr, self.t_items, self.t_sim, n_items)
        kc = min(k + (user_h.size(1) if user_h is not None else 0), n_items - 1)
        score, topk_items = ops.row_topk(scores, kc) if kc <= ops.FULLSCORE_MAX_K else torch.topk(scores, kc)
        topk_items = topk_items + 1
        if user_h is not None:
            score, topk_items = ops.topk_mask_history(score, topk_items, user_h, min(k, kc))
        return (score, topk_items, scores) if return_query else (score, topk_items)

    def fit(self, train_data, val_data=None, run_mode='light', config=None, **kwargs):
        if config is not None:
            self.config.update(config)
        if self._dist_context(kwargs) is not None:
            raise NotImplementedError('ItemKNN: the sharded fit is not covered (the build needs both CSRs of the whole split on one device)')
        self._init_model(train_data)
        device = self._device()
        self.to(device)
        if val_data is not None:
            val_data.use_field = train_data.use_field

        def train_epoch():
            self._knn_build(train_data, device)
            return 0.0                                                   # itemknn.py:46

        def validate():
            t1 = time.time()
            metrics = self._eval_epoch(val_data, self.validation_step, device)
            return dict(metrics, valid_time=time.time() - t1)

        return self._run_epochs(train_epoch, None, validate if val_data is not None else None, log=self.logger.info)

    def evaluate(self, test_data, verbose=True, **kwargs):
        test_data.use_field = self.fields
        out = self._eval_epoch(test_data, self.test_step, self.nbr_cnt.device)
        if verbose:
            self.logger.info(str(out))
        return out


# model.fused_ease: the fit and the scores run in rsa_ease_gram / rsa_spd_inverse_f64 / rsa_ease_weights / rsa_ease_score instead of
# ease_torch / ease_score_torch.  Off: tools/bench_ease.py (profiles/ease_bench.json, medians of 3) at about ml-1m's shape has the fused
# fit at 19.8 ms against 15.6 ms for torch.linalg.cholesky + cholesky_inverse (torch.linalg.inv 40.5 ms); at about ml-20m's
# (N = 20001) the fused fit takes 545 ms (37 % of the fp64 matrix floor) and BOTH torch arms fail inside hipBLAS / hipSOLVER, so
# there is no second win to count; a score batch (B = 512) is ahead at both, 0.15 / 0.30 ms and 1.07 / 6.64 ms.
FUSED_EASE_DEFAULT = False
_EASE_BUFFERS = ('ease_B', 'user_indptr', 'user_items')


def ease_torch(users, items, n_users, n_items, lam):
    """The reference's op sequence (recstudio/model/mf/ease.py) in torch ops on the device of ``users``: dense float64 ``R``,
    ``G = R^T R + lam I``, ``P = inv(G)``, ``B = P / (-diag P)`` with a zero diagonal, and the loss ``||R - R B||_F``.
    -> ``(B float64 [N, N], loss float64 scalar tensor)``."""
    R = torch.zeros(n_users, n_items, dtype=torch.float64, device=users.device)
    R[users.long(), items.long()] = 1
    G = R.T @ R
    G.diagonal().add_(lam)
    P = torch.linalg.inv(G)
    B = P / (-P.diagonal())
    B.diagonal().zero_()
    return B, torch.linalg.norm(R - R @ B)


def ease_score_torch(users, indptr, items, B):
    """The torch-op twin of ``ops.ease_score``: the dense float64 rows ``R[users]`` times ``B[:, 1:]``, as fp32."""
    users = users.long()
    deg = indptr[users + 1] - indptr[users]
    b = torch.repeat_interleave(torch.arange(users.numel(), device=users.device), deg)
    pos = torch.arange(b.numel(), device=users.device) - torch.repeat_interleave(torch.cumsum(deg, 0) - deg, deg)
    R = torch.zeros(users.numel(), B.size(0), dtype=torch.float64, device=users.device)
    R[b, items[indptr[users][b] + pos].long()] = 1
    return (R @ B[:, 1:]).float()


class EASE(BaseRetriever):
    """recstudio/model/mf/ease.py, recstudio/model/mf/config/ease.yaml (lambda 250): Embarrassingly Shallow Autoencoders.  There is
    nothing to iterate: ``fit`` computes, once, ``B = P / (-diag P)`` with a zero diagonal from ``P = (R^T R + lambda I)^-1`` in
    float64, and a user's score of item i is the sum of ``B[j, i]`` over the user's train items j.  No sampler, loss function,
    optimizer or encoder; ``ease_B`` [N, N] float64 and the user-side CSR are buffers, so ``state_dict`` carries the fitted model.
    ``model.fused_ease``: ``ops.ease_gram`` / ``spd_inverse`` / ``ease_weights`` / ``ease_score``; off, ``ease_torch`` /
    ``ease_score_torch``.  The epoch loss is the reference's ``||R - R B||_F`` (with the flag on, its closed form from ``P``).
    Two deviations from the reference: it sets ``config['train']['gpu']`` to None (its only path is numpy on the host); this
    model leaves the config alone and runs on the configured device.  Its ``state_dict`` carries the whole dense ``R``
    (``user_item_matrix``); this one carries the CSR of R."""

    config_defaults = {'model': {'fused_ease': FUSED_EASE_DEFAULT}, 'train': {'lambda': 250, 'epochs': 1}}

    def _get_item_encoder(self, train_data):
        return None

    def _get_query_encoder(self, train_data):
        return None

    def _get_loss_func(self):
        return None

    def _get_sampler(self, train_data):
        return None

    def _update_item_vector(self):
        pass                                                              # the "item vector" is ease_B itself

    def _get_item_vector(self):
        return self.ease_B[:, 1:]                                         # ease.py: item_vector = B[:, 1:]

    def _ease_build(self, train_data, device):
        lam = self.config['train']['lambda']
        users, items, n_users, n_items, (u_indptr, u_items), (i_indptr, i_users) = _interaction_csrs(train_data, device, 'EASE')
        if self.config['model']['fused_ease']:
            P, status = ops.spd_inverse(ops.ease_gram(u_indptr, u_items, i_indptr, i_users, lam), overwrite=True)
            if int(status) != 0:
                raise ValueError(f'EASE: R^T R + lambda I is not positive definite at item {int(status) - 1} (lambda = {lam}; it must be > 0)')
            B, loss = ops.ease_weights(P, lam, overwrite=True)
        else:
            if not lam > 0:
                raise ValueError(f'EASE: lambda = {lam} must be > 0 (item 0 has no interactions: its column is singular)')
            B, loss = ease_torch(users, items, n_users, n_items, lam)
        for name, t in zip(_EASE_BUFFERS, (B, u_indptr, u_items)):
            self.register_buffer(name, t)
        return float(loss)

    def load_state_dict(self, state_dict, strict=True):
        for name in _EASE_BUFFERS:                                       # a fresh model has no weights yet: take their shapes from the state
            if name in state_dict:
                self.register_buffer(name, torch.empty_like(state_dict[name]))
        return super().load_state_dict(state_dict, strict)

    def topk(self, batch, k, user_h=None, return_query=False):
        """baseretriever.py:374-397 over the EASE scores: top (k + |hist|), ids + 1, the history dropped, top k."""
        users = (batch[self.fuid] if isinstance(batch, dict) else batch).to(self.ease_B.device)
        n_items = self.ease_B.size(0)
        score_fn = ops.ease_score if self.config['model']['fused_ease'] else ease_score_torch
        scores = score_fn(users, self.user_indptr, self.user_items, self.ease_B)
        kc = min(k + (user_h.size(1) if user_h is not None else 0), n_items - 1)
        score, topk_items = ops.row_topk(scores, kc) if kc <= ops.FULLSCORE_MAX_K else torch.topk(scores, kc)
        topk_items = topk_items + 1
        if user_h is not None:
            score, topk_items = ops.topk_mask_history(score, topk_items, user_h, min(k, kc))
        return (score, topk_items, scores) if return_query else (score, topk_items)

    def fit(self, train_data, val_data=None, run_mode='light', config=None, **kwargs):
        if config is not None:
            self.config.update(config)
        if self._dist_context(kwargs) is not None:
            raise NotImplementedError('EASE: the sharded fit is not covered (the dense N x N inverse lives on one device)')
        self._init_model(train_data)
        device = self._device()
        self.to(device)
        if val_data is not None:
            val_data.use_field = train_data.use_field

        def train_epoch():
            return self._ease_build(train_data, device)

        def validate():
            t1 = time.time()
            metrics = self._eval_epoch(val_data, self.validation_step, device)
            return dict(metrics, valid_time=time.time() - t1)

        return self._run_epochs(train_epoch, None, validate if val_data is not None else None, log=self.logger.info)

    def evaluate(self, test_data, verbose=True, **kwargs):
        test_data.use_field = self.fields
        out = self._eval_epoch(test_data, self.test_step, self.ease_B.device)
        if verbose:
            self.logger.info(str(out))
        return out


# model.fused_slim: the fit runs in rsa_slim_fit instead of slim_torch (scores: rsa_knn_score instead of itemknn_score_torch).
# On: tools/bench_slim.py (profiles/slim_bench.json, medians of 3) at about ml-1m's shape (6041 x 3707) and the reference's alpha 1,
# l1_ratio 0.1 has the fused fit, Gram included, at 2.0 ms against 1035 ms for slim_torch (same n_iter on every target, weights
# within 1.5e-15); sklearn's host loop took 1.65 s for 64 sampled targets, about 96 s scaled to all.  At alpha 0.1 (up to 1892
# candidates, 467 targets in the workgroup kernel) the fused fit takes 6.7 ms.
FUSED_SLIM_DEFAULT = True
_SLIM_BUFFERS = ('slim_indptr', 'slim_items', 'slim_w', 'user_indptr', 'user_items')


def slim_torch(G, n_rows, alpha, l1_ratio, positive=True, max_iter=100, tol=1e-4):
    """The torch-op twin of ``ops.slim_fit`` and the only path for ``positive_only: False``: sklearn's Gram coordinate descent in
    cyclic order for ALL targets at once in float64, one coordinate per step across all columns.  Column j of ``g`` is target j's
    ``q - Q w`` and of ``W`` its weights; a column that met its stop test is frozen by a ``done`` mask.
    -> ``(B float64 [N, N] with B[:, j] = w of target j (column 0 zero), n_iter int64 [N])``."""
    N = G.size(0)
    a, b = alpha * l1_ratio * int(n_rows), alpha * (1.0 - l1_ratio) * int(n_rows)
    G = G.contiguous()
    diag = G.diagonal().clone()
    eye = torch.eye(N, dtype=torch.bool, device=G.device)
    g = G.masked_fill(eye, 0.0)                                       # q: column j of G without its own entry
    W = torch.zeros_like(g)
    done = torch.zeros(N, dtype=torch.bool, device=G.device)
    done[0] = True                                                    # the padding item is nobody's target
    n_iter = torch.full((N,), int(max_iter), dtype=torch.int64, device=G.device)
    n_iter[0] = 0
    live = diag != 0                                                  # a zero diagonal is skipped (item 0, empty items)
    if positive:
        live &= (g > a).any(1)                                        # G[k, j] <= a for every j: coordinate k never leaves 0
    coords = torch.nonzero(live).flatten().tolist()
    for it in range(int(max_iter)):
        d_w_max = torch.zeros(N, dtype=torch.float64, device=G.device)
        for k in coords:
            tmp = g[k] + W[k] * diag[k]
            if positive:
                wn = torch.where(tmp < 0, torch.zeros_like(tmp), (tmp - a).clamp_min(0.0) / (diag[k] + b))
            else:
                wn = torch.sign(tmp) * (tmp.abs() - a).clamp_min(0.0) / (diag[k] + b)
            delta = torch.where(done | eye[k], torch.zeros_like(tmp), wn - W[k])        # target k has no coordinate k
            W[k] += delta
            g.addr_(G[:, k], delta, alpha=-1.0)
            d_w_max = torch.maximum(d_w_max, delta.abs())
        w_max = W.abs().amax(0)
        check = (w_max == 0) | (d_w_max / w_max < tol)
        if it == max_iter - 1:
            check = torch.ones_like(check)
        gm = g.masked_fill(eye, 0.0)                                  # row j of target j belongs to the zeroed row of Q
        q = G.masked_fill(eye, 0.0)
        q_dot_w, w_h = (W * q).sum(0), (W * (q - gm)).sum(0)
        xta = gm - b * W
        dual = xta.amax(0) if positive else xta.abs().amax(0)
        r2 = diag + w_h - 2.0 * q_dot_w
        c = torch.where(dual > a, a / dual, torch.ones_like(dual))
        gap = torch.where(dual > a, 0.5 * (r2 + r2 * c * c), r2)
        gap = gap + (a * W.abs().sum(0) - c * diag + c * q_dot_w + 0.5 * b * (1.0 + c * c) * (W * W).sum(0))
        stop = check & (gap < tol * diag) & ~done
        n_iter[stop] = it + 1
        done |= stop
        if bool(done.all()):
            break
    W[:, 0] = 0.0
    return W, n_iter


class SLIM(EASE):
    """recstudio/model/mf/slim.py, recstudio/model/mf/config/slim.yaml (alpha 1, l1_ratio 0.1, positive_only True, knn 100): Sparse
    Linear Methods.  ``fit`` solves, once, one elastic-net problem per target item on the float64 Gram matrix of the train split --
    sklearn's ``ElasticNet(precompute=True, fit_intercept=False, max_iter=100, tol=1e-4)`` rule, ``a = alpha l1_ratio U`` and
    ``b = alpha (1 - l1_ratio) U`` with U the rows of R, the padding user included -- and keeps the non-zero weights as a sparse
    item-item matrix; a user's score of item i is the sum of ``B[j, i]`` over the user's train items j.  The sparse matrix (by
    neighbour: ``slim_indptr`` / ``slim_items`` / ``slim_w``) and the user-side CSR are buffers, so ``state_dict`` carries the fitted
    model.  ``model.fused_slim``: ``ops.slim_fit`` / ``ops.knn_score``; off, ``slim_torch`` / ``itemknn_score_torch``.
    ``train.knn`` is accepted and unused, as in the reference.  ONE deviation from the reference: a sweep visits the coordinates
    in cyclic ascending order, where the reference asks for ``selection='random'`` driven by sklearn's private ``rand_r`` stream,
    which cannot be followed; for b > 0 both orders converge to the same unique minimiser.  The weights are kept in fp32 for
    scoring, as ItemKNN's similarities are."""

    config_defaults = {'model': {'fused_slim': FUSED_SLIM_DEFAULT},
                       'train': {'alpha': 1, 'l1_ratio': 0.1, 'positive_only': True, 'knn': 100, 'epochs': 1}}

    def _update_item_vector(self):
        pass                                                              # the "item vector" is the sparse weight matrix

    def _get_item_vector(self):
        raise NotImplementedError('SLIM: the item vector is the sparse matrix slim_indptr / slim_items / slim_w, not a dense one')

    def _slim_build(self, train_data, device):
        tr, fused = self.config['train'], self.config['model']['fused_slim']
        if fused and not tr['positive_only']:
            raise NotImplementedError('SLIM: model.fused_slim covers positive_only: True only (the candidate bound of rsa_slim_fit '
                                      'rests on w >= 0); set fused_slim: False')
        _, _, n_users, n_items, (u_indptr, u_items), (i_indptr, i_users) = _interaction_csrs(train_data, device, 'SLIM')
        G = ops.ease_gram(u_indptr, u_items, i_indptr, i_users, 0.0)
        if fused:
            nbr_id, nbr_w, nbr_cnt, _ = ops.slim_fit(G, n_users, tr['alpha'], tr['l1_ratio'])
        else:
            B, _ = slim_torch(G, n_users, tr['alpha'], tr['l1_ratio'], tr['positive_only'])
            live = (B != 0).T                                            # row j: the neighbours of target j, ascending
            nbr_cnt = live.sum(1).to(torch.int32)
            cap = max(1, int(nbr_cnt.max()))
            rank = torch.cumsum(live, 1) - 1
            tgt, nb = torch.nonzero(live, as_tuple=True)
            nbr_id = torch.full((n_items, cap), -1, dtype=torch.int32, device=device)
            nbr_w = torch.zeros(n_items, cap, dtype=torch.float64, device=device)
            nbr_id[tgt, rank[tgt, nb]], nbr_w[tgt, rank[tgt, nb]] = nb.to(torch.int32), B[nb, tgt]
        for name, t in zip(_SLIM_BUFFERS, ops.knn_transpose(nbr_id, nbr_w.float(), nbr_cnt) + (u_indptr, u_items)):
            self.register_buffer(name, t)
        return 0.0                                                        # slim.py: training_epoch returns 0

    def load_state_dict(self, state_dict, strict=True):
        for name in _SLIM_BUFFERS:                                       # a fresh model has no weights yet: take their shapes from the state
            if name in state_dict:
                self.register_buffer(name, torch.empty_like(state_dict[name]))
        return BaseRetriever.load_state_dict(self, state_dict, strict)

    def topk(self, batch, k, user_h=None, return_query=False):
        """baseretriever.py:374-397 over the SLIM scores: top (k + |hist|), ids + 1, the history dropped, top k."""
        users = (batch[self.fuid] if isinstance(batch, dict) else batch).to(self.slim_w.device)
        n_items = self.slim_indptr.numel() - 1
        score_fn = ops.knn_score if self.config['model']['fused_slim'] else itemknn_score_torch
        scores = score_fn(users, self.user_indptr, self.user_items, self.slim_indptr, self.slim_items, self.slim_w, n_items)
        kc = min(k + (user_h.size(1) if user_h is not None else 0), n_items - 1)
        score, topk_items = ops.row_topk(scores, kc) if kc <= ops.FULLSCORE_MAX_K else torch.topk(scores, kc)
        topk_items = topk_items + 1
        if user_h is not None:
            score, topk_items = ops.topk_mask_history(score, topk_items, user_h, min(k, kc))
        return (score, topk_items, scores) if return_query else (score, topk_items)

    def fit(self, train_data, val_data=None, run_mode='light', config=None, **kwargs):
        if config is not None:
            self.config.update(config)
        if self._dist_context(kwargs) is not None:
            raise NotImplementedError('SLIM: the sharded fit is not covered (the dense N x N Gram matrix lives on one device)')
        self._init_model(train_data)
        device = self._device()
        self.to(device)
        if val_data is not None:
            val_data.use_field = train_data.use_field

        def train_epoch():
            return self._slim_build(train_data, device)

        def validate():
            t1 = time.time()
            metrics = self._eval_epoch(val_data, self.validation_step, device)
            return dict(metrics, valid_time=time.time() - t1)

        return self._run_epochs(train_epoch, None, validate if val_data is not None else None, log=self.logger.info)

    def evaluate(self, test_data, verbose=True, **kwargs):
        test_data.use_field = self.fields
        out = self._eval_epoch(test_data, self.test_step, self.slim_w.device)
        if verbose:
            self.logger.info(str(out))
        return out
