"""The matrix-factorisation family beyond BPR: NCF, WRMF."""
import time

import torch

from . import ops
from .dataset import ALSDataset

from .loss_func import BinaryCrossEntropyLoss
from .retriever import BaseRetriever
from .sampler import UniformSampler
from .scorer import FusionMFMLPScorer, GMFScorer, InnerProductScorer, MLPScorer
from .seqmodule import MLPModule

__all__ = ['NCF', 'FUSED_SCORER_DEFAULT', 'WRMF', 'FUSED_ALS_DEFAULT', 'als_step_torch']

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
