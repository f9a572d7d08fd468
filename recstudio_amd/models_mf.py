"""The matrix-factorisation family beyond BPR: NCF."""
import torch

from .loss_func import BinaryCrossEntropyLoss
from .retriever import BaseRetriever
from .sampler import UniformSampler
from .scorer import FusionMFMLPScorer, GMFScorer, MLPScorer
from .seqmodule import MLPModule

__all__ = ['NCF', 'FUSED_SCORER_DEFAULT']

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
