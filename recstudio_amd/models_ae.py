"""The autoencoder family: the two towers over a user's bag of items and MultiDAE / MultiVAE on them.  The bag pooling is
``seqmodule.bag_pool`` (the kernel pair of rsa_bag.hip on the device)."""
import torch

from .dataset import UserDataset
from .loss_func import SoftmaxLoss
from .retriever import BaseRetriever, _BatchQueryFeat
from .scorer import InnerProductScorer, full_lse
from .seqmodule import MLPModule, bag_pool

__all__ = ['MultiDAEQueryEncoder', 'MultiVAEQueryEncoder', 'MultiDAE', 'MultiVAE']

# MultiDAE / MultiVAE: the bag kernel pair (rsa_bag.hip) for the encoder input and the positives' mean -- see DESIGN.md 4.19 for the
# measurement this default follows from
FUSED_BAG_DEFAULT = True


class _BagQueryEncoder(torch.nn.Module):
    """What the two autoencoder towers share (recstudio/model/ae/multidae.py:10-32, multivae.py:10-36): the item table, the
    dropout and ``h = dropout(item_embedding(ids).sum(1) / count_nonzero(ids, 1) ** 0.5)`` -- one ``seqmodule.bag_pool`` call
    (``fused_bag``: the kernel pair on the device; off, or on CPU tensors: the reference's op sequence)."""

    def __init__(self, fiid, num_items, embed_dim, dropout_rate, encoder_dims, decoder_dims, fused_bag):
        super().__init__()
        assert encoder_dims[-1] == decoder_dims[0], 'expecting the output size of' \
            'encoder is equal to the input size of decoder.'
        assert encoder_dims[0] == decoder_dims[-1], 'expecting the output size of' \
            'decoder is equal to the input size of encoder.'
        self.fiid = fiid
        self.fused_bag = fused_bag
        self.item_embedding = torch.nn.Embedding(num_items, embed_dim, 0)
        self.dropout = torch.nn.Dropout(p=dropout_rate)

    def pooled(self, batch):
        return self.dropout(bag_pool(self.item_embedding.weight, batch['in_' + self.fiid], 'rsqrt', fused=self.fused_bag))


class MultiDAEQueryEncoder(_BagQueryEncoder):
    """recstudio/model/ae/multidae.py:9-34, same constructor arguments (plus ``fused_bag``), submodules and ``state_dict`` keys
    (``item_embedding``, ``encoder_decoder``)."""

    def __init__(self, fiid, num_items, embed_dim, dropout_rate, encoder_dims, decoder_dims, activation='relu',
                 fused_bag=FUSED_BAG_DEFAULT):
        super().__init__(fiid, num_items, embed_dim, dropout_rate, encoder_dims, decoder_dims, fused_bag)
        self.encoder_decoder = torch.nn.Sequential(
            MLPModule([embed_dim] + encoder_dims + decoder_dims[1:], activation),
            torch.nn.Linear(decoder_dims[-1], embed_dim))

    def forward(self, batch):
        return self.encoder_decoder(self.pooled(batch))


class MultiVAEQueryEncoder(_BagQueryEncoder):
    """recstudio/model/ae/multivae.py:9-60, same constructor arguments (plus ``fused_bag``), submodules and ``state_dict`` keys
    (``item_embedding``, ``encoders``, ``decoders``).  ``kl_loss`` is set by every training-mode forward."""

    def __init__(self, fiid, num_items, embed_dim, dropout_rate, encoder_dims, decoder_dims, activation='relu',
                 fused_bag=FUSED_BAG_DEFAULT):
        super().__init__(fiid, num_items, embed_dim, dropout_rate, encoder_dims, decoder_dims, fused_bag)
        self.encoders = torch.nn.Sequential(
            MLPModule([embed_dim] + encoder_dims[:-1], activation),
            torch.nn.Linear(([embed_dim] + encoder_dims[:-1])[-1], encoder_dims[-1] * 2))
        self.decoders = torch.nn.Sequential(
            MLPModule(decoder_dims, activation),
            torch.nn.Linear(decoder_dims[-1], embed_dim))
        self.kl_loss = 0.0

    def forward(self, batch):
        encoder_h = self.encoders(self.pooled(batch))
        mu, logvar = encoder_h.tensor_split(2, dim=-1)
        z = self.reparameterize(mu, logvar)
        decoder_z = self.decoders(z)
        if self.training:
            self.kl_loss = self.kl_loss_func(mu, logvar)
        return decoder_z

    def reparameterize(self, mu, logvar):
        if self.training:
            std = torch.exp(0.5 * logvar)
            eps = torch.randn_like(std)
            return eps.mul(std).add_(mu)
        return mu

    def kl_loss_func(self, mu, logvar):
        return -0.5 * torch.mean(torch.sum(1 + logvar - mu.pow(2) - logvar.exp(), dim=1))


class _BagSoftmaxRetriever(_BatchQueryFeat, BaseRetriever):
    """What MultiDAE and MultiVAE share: one sample per user (``UserDataset``, whose batches are assembled on the host), no
    sampler, full softmax over the catalog.  With ``model.fused_bag`` the training step is
    ``mean_b(lse_b - <q_b, mean_l item[pos_bl]>)`` -- the reference's second ``SoftmaxLoss`` branch (loss_func.py:39-47) reduced
    per user -- with the positives' mean one ``bag_pool`` over the item table: no ``[B, L, d]`` gather of the positives, no
    ``[B, L]`` scores.  ``lse`` comes from ``scorer.full_lse`` (no ``[B, N]`` scores) where the fused full softmax applies (an
    nn.Embedding catalog up to 128 wide), else from ``torch.logsumexp`` over the scorer's full scores.  With the flag off the
    step is the stock plugin path over the torch twin."""

    config_defaults = {'model': {'fused_bag': FUSED_BAG_DEFAULT}, 'train': {'device_loader': False}}

    def _get_dataset_class():
        return UserDataset

    def _get_sampler(self, train_data):
        return None

    def _get_loss_func(self):
        return SoftmaxLoss()

    def _bag_step_ok(self, batch):
        return (self.config['model'].get('fused_bag', False) and type(self.loss_fn) is SoftmaxLoss and self.sampler is None
                and type(self.score_func) is InnerProductScorer and isinstance(self.item_encoder, torch.nn.Embedding)
                and batch[self.fiid].dim() == 2 and batch[self.fiid].is_cuda)

    def training_step(self, batch):
        if not self._bag_step_ok(batch):
            return super().training_step(batch)
        query = self.query_encoder(self._get_query_feat(batch))
        weight = self.item_encoder.weight
        pos = (bag_pool(weight, batch[self.fiid], 'mean') * query).sum(-1)
        if weight.shape[1] <= 128 and self.config['train'].get('fused_full_softmax', True):
            lse = full_lse(query, weight)
        else:
            lse = torch.logsumexp(self.score_func(query, self._get_item_vector()), dim=-1)
        return (lse - pos).mean()


class MultiDAE(_BagSoftmaxRetriever):
    """recstudio/model/ae/multidae.py:37-67, recstudio/model/ae/config/multidae.yaml."""

    config_defaults = {'model': {'embed_dim': 200, 'dropout': 0.5, 'encoder_dims': [64, 32], 'decoder_dims': [32, 64],
                                 'activation': 'relu'},
                       'train': {'batch_size': 256, 'learning_rate': 0.01, 'weight_decay': 1e-5}}

    def _get_query_encoder(self, train_data):
        m = self.config['model']
        return MultiDAEQueryEncoder(train_data.fiid, train_data.num_items, self.embed_dim, m['dropout'], m['encoder_dims'],
                                    m['decoder_dims'], m['activation'], fused_bag=m['fused_bag'])


class MultiVAE(_BagSoftmaxRetriever):
    """recstudio/model/ae/multivae.py:63-105, recstudio/model/ae/config/multivae.yaml: the shared step plus ``anneal * kl_loss``,
    the weight rising by ``1 / train.anneal_total_step`` per step up to ``train.anneal_max`` (:97-105)."""

    config_defaults = {'model': {'embed_dim': 600, 'dropout_rate': 0.5, 'encoder_dims': [200], 'decoder_dims': [200],
                                 'activation': 'tanh'},
                       'train': {'batch_size': 500, 'learning_rate': 0.001, 'weight_decay': 1e-5, 'anneal_max': 0.2,
                                 'anneal_total_step': 2000000, 'early_stop_patience': 100}}

    def _get_query_encoder(self, train_data):
        m = self.config['model']
        return MultiVAEQueryEncoder(train_data.fiid, train_data.num_items, self.embed_dim, m['dropout_rate'], m['encoder_dims'],
                                    m['decoder_dims'], m['activation'], fused_bag=m['fused_bag'])

    def training_step(self, batch):
        loss = super().training_step(batch)
        if not hasattr(self, 'anneal'):
            setattr(self, 'anneal', 0)
        tr = self.config['train']
        anneal = min(tr['anneal_max'], self.anneal)
        self.anneal = min(tr['anneal_max'], self.anneal + (1.0 / tr['anneal_total_step']))
        return loss + anneal * self.query_encoder.kl_loss
