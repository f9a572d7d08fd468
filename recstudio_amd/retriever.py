"""``BaseRetriever`` -- host-side mirror of recstudio/model/basemodel/baseretriever.py (the class the
reference's READMEs call TwoTowerRecommender / ItemTowerRecommender) with its forward dispatched to
the fused HIP path.

Kept from the reference: constructor kwargs (``item_encoder``, ``query_encoder``, ``scorer``,
``sampler``, ``loss``; baseretriever.py:14-43, recommender.py:48-56), the overridable hooks
(``_get_dataset_class``, ``_get_item_encoder``, ``_get_query_encoder``, ``_get_score_func``,
``_get_loss_func``, ``_get_sampler``, ``_set_data_field``), ``forward`` with its ``return_*`` flags
and output dict layout (:142-192), ``sampling`` / ``_sample`` for ``method='none'`` (:204-278),
``topk`` (:374-397), ``training_step`` / ``validation_step`` / ``test_step`` / ``_test_step``
(:399-431), ``fit`` / ``evaluate`` and the config keys read on the path.  The train/eval loop around
it is a minimal compatible one (the reference's Recommender loop is out of scope).
"""
import copy
import inspect
import logging
import math
import os
import time
from typing import Dict

import numpy as np
import torch

from . import _native as nat
from . import eval as rs_eval
from . import ops
from .dataset import SeqDataset, TripletDataset, UserDataset
from .fused import BPRAdagradStep, BPRAdamStep, BPRSGDStep, fused_bpr_loss, fused_ssm_loss, retriever_scores
from .loss_func import (BinaryCrossEntropyLoss, BPRLoss, FullScoreLoss, PairwiseLoss, PointwiseLoss, SampledSoftmaxLoss,
                        SoftmaxLoss)
from .sampler import PopularSamplerModel, Sampler, UniformSampler
from .scorer import CosineScorer, EuclideanScorer, InnerProductScorer, full_lse
from .seqmodule import AttentionLayer, FusedGRU, FusedTransformerEncoder, MLPModule, caser_conv_torch, caser_pack
from .seqmodule import hgn_gating, hgn_gating_torch
from .seqmodule import bag_pool

__all__ = ['BaseRetriever', 'TwoTowerRecommender', 'ItemTowerRecommender', 'BPR', 'SASRec', 'CL4SRec', 'GRU4Rec', 'NARM', 'STAMP', 'HGN', 'MultiDAE', 'MultiVAE', 'LightGCN', 'SGL',
           'SimGCL', 'default_config', 'seed_everything']

# ``model.fused_attention_pool`` of NARM and STAMP (the attention pooling as one HIP kernel): on where the kernel beat the
# reference's op sequence in the same run, forward and forward + backward, at both models' shapes
FUSED_ATTENTION_POOL_DEFAULT = True
# ``model.fused_infonce`` of CL4SRec (the in-batch InfoNCE as HIP kernels without [B, 2B]): OFF.  The rule is on only where the kernels
# are not slower than the reference's op sequence at every measured shape in both directions (tools/bench_cl4srec.py,
# ``fused_infonce_wins_everywhere``); they win at B = 256 and lose at B = 8192 (2.11 against 1.19 ms forward, 6.07 against 2.30 ms
# forward + backward at d = 64), where what they buy is memory: 1.7 GB less
FUSED_INFONCE_DEFAULT = False
# ``model.fused_gating`` of HGN (both gates, the pooling and the item-item sum as one HIP kernel): on where the kernel beat the
# reference's op sequence in the same run, forward and forward + backward, at both measured shapes
FUSED_GATING_DEFAULT = True
# MultiDAE / MultiVAE: the bag kernel pair (rsa_bag.hip) for the encoder input and the positives' mean -- see DESIGN.md 4.19 for the
# measurement this default follows from
FUSED_BAG_DEFAULT = True


def default_config():
    """recstudio/model/basemodel/basemodel.yaml."""
    return {
        'data': {'binarized_rating_thres': None, 'fm_eval': False, 'neg_count': 0, 'sampler': None, 'shuffle': True,
                 'split_mode': 'user_entry', 'split_ratio': [0.8, 0.1, 0.1]},
        'model': {'embed_dim': 64, 'item_bias': False},
        'train': {'accelerator': 'gpu', 'ann': None, 'batch_size': 512, 'early_stop_mode': 'max',
                  'early_stop_patience': 10, 'epochs': 1000, 'gpu': 1, 'grad_clip_norm': None,
                  'init_method': 'xavier_normal', 'item_batch_size': 1024, 'learner': 'adam', 'learning_rate': 0.001,
                  'num_threads': 10, 'sampling_method': 'none', 'sampler': 'uniform', 'negative_count': 0,
                  'excluding_hist': False, 'scheduler': None, 'seed': 2022, 'weight_decay': 0.0,
                  'tensorboard_path': None, 'sparse_grad': False, 'device_loader': True, 'fused_optimizer': None,
                  'shard_slices': 1, 'shard_layout': 'block', 'shard_owner_loss': True, 'shard_init': 'auto',
                  'shard_lookahead': False, 'shard_deterministic': True, 'shard_rows_share': None,
                  'fused_prefetch': True, 'brute_stream': False},
        'eval': {'batch_size': 128, 'cutoff': [5, 10, 20], 'val_metrics': ['ndcg', 'recall'], 'val_n_epoch': 1,
                 'test_metrics': ['ndcg', 'recall', 'precision', 'map', 'mrr', 'hit'], 'topk': 100,
                 'save_path': './saved/'},
    }


def seed_everything(seed):
    """recstudio/utils/utils.py:334-381: python / numpy / torch CPU + all device generators."""
    import random
    random.seed(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)
    return seed


def _device_init_block(plan, rank, n_items, d, seed, method, device, rows_per_chunk=1 << 16):
    """This rank's rows of an [n_items, d] embedding table initialised as recstudio/model/init.py does (xavier_normal /
    xavier_uniform over the FULL shape, normal(0.02)) WITHOUT ever holding the full table: the table is defined chunk by
    chunk of ``rows_per_chunk`` GLOBAL rows, chunk c drawn from its own generator stream (seed, c) on the device, and a
    rank generates the chunks its rows fall into and keeps those rows.  The table is therefore a function of (seed, shape)
    alone: any world size, either row layout, gives the rows of the same table (at 1e8 x 128 the host copy the
    slice-after-init form needs is 51 GB per rank)."""
    n_local = plan.n_local(rank)
    out = torch.empty(n_local, d, dtype=torch.float32, device=device)
    gen = torch.Generator(device=device)
    if method == 'xavier_uniform':
        bound = (6.0 / (n_items + d)) ** 0.5
    std = (2.0 / (n_items + d)) ** 0.5 if method == 'xavier_normal' else 0.02
    R, G = int(rows_per_chunk), plan.world
    lo, hi = (0, n_items) if plan.interleaved else plan.bounds(rank)
    for c in range(lo // R, (max(hi, lo + 1) - 1) // R + 1):
        a, b = c * R, min((c + 1) * R, n_items)
        if b <= a:
            break
        gen.manual_seed((int(seed) * 1_000_003 + c) & 0x7fffffffffffffff)
        if method == 'xavier_uniform':
            vals = (torch.rand(R, d, generator=gen, device=device) * 2 - 1) * bound
        else:
            vals = torch.randn(R, d, generator=gen, device=device) * std
        if plan.interleaved:
            first = (rank - a) % G                     # first row of the chunk this rank owns
            rows = vals[first:b - a:G]
            at = (a + first - rank) // G
            out[at:at + rows.shape[0]] = rows
        else:
            u, v = max(a, lo), min(b, hi)
            if v > u:
                out[u - lo:v - lo] = vals[u - a:v - a]
    return out


def _init_weights(module, method):
    """recstudio/model/init.py: xavier_normal / xavier_uniform / normal(0.02); the padding row is zeroed."""
    if isinstance(module, torch.nn.Embedding) and module.weight.is_meta:
        return          # a sharded catalog: its rows are drawn on the owners' devices (_device_init_block)
    if isinstance(module, (torch.nn.Embedding, torch.nn.Linear)):
        if method == 'xavier_normal':
            torch.nn.init.xavier_normal_(module.weight.data)
        elif method == 'xavier_uniform':
            torch.nn.init.xavier_uniform_(module.weight.data)
        else:
            module.weight.data.normal_(mean=0.0, std=0.02)
        if isinstance(module, torch.nn.Linear) and module.bias is not None:
            torch.nn.init.constant_(module.bias.data, 0)
        elif getattr(module, 'padding_idx', None) is not None:
            torch.nn.init.constant_(module.weight.data[module.padding_idx], 0.)
    elif isinstance(module, torch.nn.LayerNorm):
        module.bias.data.zero_()
        module.weight.data.fill_(1.0)


def _stock_forward(scorer, sampler, item_embedding, n_item_fields, sampling_method, neg_count, **train_only):
    """Dispatch rule (mirrors the reference's own check at baseretriever.py:122), on plain values: the fused kernels are used
    when the item tower is a plain ``nn.Embedding`` over the item id, the scorer's TYPE is exactly one of the stock scorers, the
    sampler's exactly UniformSampler / PopularSamplerModel (None: no sampler, full-score losses) and ``sampling_method`` is
    'none'; anything else goes through the per-plugin path (sampler / scorer / loss objects called one by one, like the
    reference does).  ``train_only``: what only ``_stock_train_path`` looks at."""
    return (item_embedding and n_item_fields == 1 and scorer in (InnerProductScorer, CosineScorer, EuclideanScorer)
            and (sampler is None or sampler in (UniformSampler, PopularSamplerModel)) and sampling_method == 'none'
            and not isinstance(neg_count, (list, tuple)))


def _stock_train_path(loss, dim, fused_ssm=True, fused_full_softmax=True, **fwd):
    """The fused training path of a stock configuration, on plain values (``fwd``: ``_stock_forward``'s; ``dim``: the width of
    an nn.Embedding item tower): 'bpr' / 'ssm' -- stock BPRLoss / SampledSoftmaxLoss on whole 64-negative tiles, one launch --,
    'full_softmax' -- stock SoftmaxLoss without the [B, N] score matrix --, or None: the per-plugin path."""
    ip, n = fwd['scorer'] is InnerProductScorer, fwd['neg_count']
    if fwd['sampler'] is None:
        full = (loss is SoftmaxLoss and ip and fwd['item_embedding'] and fwd['n_item_fields'] == 1 and dim <= 128
                and fused_full_softmax)
        return 'full_softmax' if full else None
    if not (_stock_forward(**fwd) and ip and n and n % 64 == 0):
        return None
    if loss is SampledSoftmaxLoss and dim in (32, 64, 128, 256) and fused_ssm:
        return 'ssm'
    return 'bpr' if loss is BPRLoss else None


def _stand_in_optimizer(lr):
    """Carries a learning rate and nothing else: the reference's scheduler objects drive it when the update runs in the
    kernels, and the rate they set is handed to the kernels after every epoch."""
    opt = torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=lr)
    opt.step()                                   # (a no-op; the schedulers warn when they step first)
    return opt


def _one_ahead(batches, step, prepare=None):
    """``[step(b, prepare(b)) for b in batches]`` with the prepare calls issued one batch ahead: prepare(b0), prepare(b1),
    step(b0), prepare(b2), step(b1), ..., step(b_last); they consume the generator in batch order, so the draws are those of
    the plain sequence.  ``prepare`` None: no look-ahead, every ticket is None."""
    if prepare is None:
        return [step(batch, None) for batch in batches]
    out, ticket = [], None
    for k, (batch, batch_next) in enumerate(_with_next(batches)):
        if k == 0:
            ticket = prepare(batch)
        ticket_next = prepare(batch_next) if batch_next is not None else None
        out.append(step(batch, ticket))
        ticket = ticket_next
    return out


class BaseRetriever(torch.nn.Module):
    def __init__(self, config: Dict = None, **kwargs):
        super().__init__()
        self.config = default_config()
        if config is not None:
            for group, values in config.items():
                if isinstance(values, dict) and group in self.config:
                    self.config[group].update(values)
                else:
                    self.config[group] = values
        if self.config['train']['seed'] is not None:
            seed_everything(self.config['train']['seed'])          # recommender.py:34-35
        self.embed_dim = self.config['model']['embed_dim']
        self.logged_metrics = {}
        self.logger = logging.getLogger('recstudio_amd')
        for key, attr in (('item_encoder', 'item_encoder'), ('query_encoder', 'query_encoder')):
            if key in kwargs:
                assert isinstance(kwargs[key], torch.nn.Module), f'{key} must be torch.nn.Module'
                setattr(self, attr, kwargs[key])
            else:
                setattr(self, attr, None)
        if 'scorer' in kwargs:
            assert isinstance(kwargs['scorer'], torch.nn.Module), 'scorer must be torch.nn.Module'
            self.score_func = kwargs['scorer']
        else:
            self.score_func = self._get_score_func()
        if 'sampler' in kwargs:
            assert isinstance(kwargs['sampler'], Sampler), 'sampler must be recstudio_amd.Sampler'
            self.sampler = kwargs['sampler']
        else:
            self.sampler = None
        if 'loss' in kwargs:
            assert isinstance(kwargs['loss'], (FullScoreLoss, PairwiseLoss, PointwiseLoss)), \
                'loss should be a FullScoreLoss, PairwiseLoss or PointwiseLoss'
            self.loss_fn = kwargs['loss']
        else:
            self.loss_fn = None
        if self.config['train']['ann'] is not None:
            raise NotImplementedError('ANN indexes (train.ann) are outside the path this package covers')
        self.use_index = False
        self.ckpt_path = None

    # ------------------------------------------------------------------ hooks (reference API)
    def _get_dataset_class():
        return TripletDataset

    def _set_data_field(self, data):
        data.use_field = set([data.fuid, data.fiid, data.frating])

    def _get_item_encoder(self, train_data):
        return torch.nn.Embedding(train_data.num_items, self.embed_dim, padding_idx=0)

    def _get_query_encoder(self, train_data):
        if self.fuid in self.query_fields:
            return torch.nn.Embedding(train_data.num_users, self.embed_dim, padding_idx=0)
        raise ValueError('query_encoder missing.')

    def _get_score_func(self):
        return InnerProductScorer()

    def _get_loss_func(self):
        return None

    def _get_sampler(self, train_data):
        return UniformSampler(train_data.num_items)

    # ------------------------------------------------------------------ model set-up
    def _init_model(self, train_data, drop_unused_field=True):
        self._set_data_field(train_data)
        self.fields = train_data.use_field
        self.frating = train_data.frating
        assert self.frating in self.fields, 'rating field is required.'
        if drop_unused_field:
            train_data.drop_feat(self.fields)
        self.fiid, self.fuid = train_data.fiid, train_data.fuid
        self.item_fields = {self.fiid} & set(self.fields)
        assert self.fiid in self.item_fields, 'item id is required to use.'
        self.query_fields = {self.fuid} & set(self.fields)
        if isinstance(train_data, SeqDataset):
            self.query_fields = self.query_fields | {'in_' + f for f in self.item_fields} | {'seqlen'}
        self.neg_count = self.config['train']['negative_count']
        if self.loss_fn is None:
            if 'train_data' in inspect.signature(self._get_loss_func).parameters:
                self.loss_fn = self._get_loss_func(train_data)
            else:
                self.loss_fn = self._get_loss_func()
        if not self.item_encoder and getattr(self, '_item_table_on_meta', False):
            # multi-GPU fit over a big catalog: the [N, d] table is never materialised on the host -- its shape only (a
            # meta tensor); every rank fills its own rows on its device (_setup_shard, _device_init_block)
            with torch.device('meta'):
                self.item_encoder = self._get_item_encoder(train_data)
        self.item_encoder = self._get_item_encoder(train_data) if not self.item_encoder else self.item_encoder
        self.query_encoder = self._get_query_encoder(train_data) if not self.query_encoder else self.query_encoder
        self.sampler = self._get_sampler(train_data) if not self.sampler else self.sampler

    def _init_parameter(self):
        method = self.config['train']['init_method']
        for _, module in self.named_children():
            module.apply(lambda m: _init_weights(m, method))

    def _get_item_feat(self, data):
        return data[self.fiid] if isinstance(data, dict) else data

    def _get_query_feat(self, data):
        if isinstance(data, dict):
            if len(self.query_fields) == 1:
                return data[list(self.query_fields)[0]]
            return {f: v for f, v in data.items() if f in self.query_fields}
        return data

    def _get_item_vector(self):
        if len(self.item_fields) == 1 and isinstance(self.item_encoder, torch.nn.Embedding):
            return self.item_encoder.weight[1:]                        # baseretriever.py:122-123
        raise NotImplementedError('item towers other than nn.Embedding over the item id are not covered')

    def _update_item_vector(self):
        item_vector = self._get_item_vector()
        if not hasattr(self, 'item_vector'):
            self.register_buffer('item_vector', item_vector.detach().clone())
        else:
            self.item_vector = item_vector

    # ------------------------------------------------------------------ forward
    def _stock_values(self):
        """What ``_stock_forward`` / ``_stock_train_path`` decide on."""
        tr, embedding = self.config['train'], isinstance(self.item_encoder, torch.nn.Embedding)
        return dict(loss=type(self.loss_fn), scorer=type(self.score_func), item_embedding=embedding,
                    sampler=None if self.sampler is None else type(self.sampler), neg_count=getattr(self, 'neg_count', None),
                    n_item_fields=len(getattr(self, 'item_fields', ())), sampling_method=tr.get('sampling_method', 'none'),
                    dim=self.item_encoder.weight.shape[1] if embedding else None, fused_ssm=tr.get('fused_ssm', True),
                    fused_full_softmax=tr.get('fused_full_softmax', True))

    def _fused_ok(self):
        return _stock_forward(**self._stock_values())

    def _fused_train_path(self, batch=None):
        """'bpr' | 'ssm' | 'full_softmax' | None: the fused training path this model (and, if given, this batch) takes."""
        path = _stock_train_path(**self._stock_values())
        return path if batch is None or batch[self.fiid].dim() == 1 else None

    def _query_source(self, qfeat, gather_in_kernel=True):
        """For the fused kernels: (user table, ids) when the kernel can gather the user rows itself, else (encoded queries, None)."""
        if gather_in_kernel and isinstance(self.query_encoder, torch.nn.Embedding) and isinstance(qfeat, torch.Tensor) \
                and qfeat.dim() == 1:
            return self.query_encoder.weight, qfeat
        return self.query_encoder(qfeat), None

    def forward(self, batch: Dict, full_score: bool = False, return_query: bool = False, return_item: bool = False,
                return_neg_item: bool = False, return_neg_id: bool = False):
        if self.sampler is None or not self._fused_ok():      # (without a sampler there is nothing to fuse: one scorer call)
            return self._forward_plugins(batch, full_score, return_query, return_item, return_neg_item, return_neg_id)
        output = {}
        pos_items = self._get_item_feat(batch)
        cosine = self.score_func.cosine      # False / True / rsa_score_mode of the Euclidean scorer
        query = None
        if self.neg_count is None:
            raise ValueError('`negative_count` value is required when `sampler` is not none.')
        qsrc, qidx = self._query_source(self._get_query_feat(batch), pos_items.dim() == 1 and not return_query)
        if qidx is None:
            query, qsrc = qsrc, qsrc.reshape(-1, qsrc.shape[-1])
        lead = tuple(pos_items.shape)
        score, neg_ids = retriever_scores(
            self.item_encoder.weight, qsrc, self.neg_count, query_index=qidx, pos_ids=pos_items.reshape(-1),
            sampler=self.sampler, cosine=cosine, mask_pad_pos=pos_items.dim() > 1,
            sparse_grad=self.config['train'].get('sparse_grad', False))
        n = self.neg_count
        output['score'] = {
            'pos_score': score['pos_score'].view(lead), 'log_pos_prob': score['log_pos_prob'].view(lead).detach(),
            'neg_score': score['neg_score'].view(*lead, n), 'log_neg_prob': score['log_neg_prob'].view(*lead, n).detach()}
        neg_ids = neg_ids.view(*lead, n)
        if return_neg_item:
            output['neg_item'] = self.item_encoder(neg_ids)
        if return_neg_id:
            output['neg_id'] = neg_ids
        if return_query:
            output['query'] = query
        if return_item:
            output['item'] = self.item_encoder(pos_items)
        return output

    def _forward_plugins(self, batch, full_score, return_query, return_item, return_neg_item, return_neg_id):
        """baseretriever.py:142-192 step by step: sampler -> item_encoder -> score_func."""
        output = {}
        pos_items = self._get_item_feat(batch)
        pos_item_vec = None
        if self.sampler is not None:
            (log_pos_prob, neg_item_idx, log_neg_prob), query = self.sampling(
                batch=batch, num_neg=self.neg_count, excluding_hist=self.config['train'].get('excluding_hist', False),
                method=self.config['train'].get('sampling_method', 'none'), return_query=True)
            if (isinstance(self.item_encoder, torch.nn.Embedding) and len(self.item_fields) == 1
                    and type(self.score_func) in (InnerProductScorer, CosineScorer, EuclideanScorer)
                    and isinstance(pos_items, torch.Tensor) and isinstance(neg_item_idx, torch.Tensor)
                    and neg_item_idx.shape[:-1] == pos_items.shape and not return_neg_item and query.is_cuda):
                # Any sampler plugin / sampling method over an nn.Embedding catalog with a stock scorer: its ids go to
                # the gather+score kernel as GIVEN ids -- no [B, n, d] tensor of negative rows, and the backward is the
                # sorted row scatter instead of torch's atomic embedding backward (MaskedUniformSampler with
                # excluding_hist, B = 16384, n = 64: step + backward 3.1 -> 0.6 ms)
                n = neg_item_idx.shape[-1]
                score, _ = retriever_scores(
                    self.item_encoder.weight, query.reshape(-1, query.shape[-1]), n, pos_ids=pos_items.reshape(-1),
                    neg_ids=neg_item_idx.reshape(-1, n), cosine=self.score_func.cosine, mask_pad_pos=pos_items.dim() > 1,
                    sparse_grad=self.config['train'].get('sparse_grad', False))
                pos_score = score['pos_score'].view(pos_items.shape)
                neg_score = score['neg_score'].view(*pos_items.shape, n)
            else:
                pos_item_vec = self.item_encoder(pos_items)
                pos_score = self.score_func(query, pos_item_vec)
                if batch[self.fiid].dim() > 1:
                    pos_score = pos_score.masked_fill(batch[self.fiid] == 0, -float('inf'))
                neg_item_vec = self.item_encoder(self._get_item_feat(neg_item_idx))
                neg_score = self.score_func(query, neg_item_vec)
                if return_neg_item:
                    output['neg_item'] = neg_item_vec
            output['score'] = {'pos_score': pos_score, 'log_pos_prob': log_pos_prob, 'neg_score': neg_score,
                               'log_neg_prob': log_neg_prob}
            if return_neg_id:
                output['neg_id'] = neg_item_idx
        else:
            pos_item_vec = self.item_encoder(pos_items)
            query = self.query_encoder(self._get_query_feat(batch))
            pos_score = self.score_func(query, pos_item_vec)
            if batch[self.fiid].dim() > 1:
                pos_score = pos_score.masked_fill(batch[self.fiid] == 0, -float('inf'))
            output['score'] = {'pos_score': pos_score}
            if full_score:
                output['score']['all_score'] = self.score_func(query, self._get_item_vector())
        if return_query:
            output['query'] = query
        if return_item:
            output['item'] = pos_item_vec if pos_item_vec is not None else self.item_encoder(pos_items)
        return output

    def _sample(self, batch, neg: int = 1, excluding_hist: bool = False, return_query: bool = True):
        query = self.query_encoder(self._get_query_feat(batch))
        pos_items = batch.get(self.fiid, None)
        user_hist = batch.get('user_hist', batch.get(self.fiid, None)) if excluding_hist else None
        if not isinstance(self.sampler, Sampler):
            raise TypeError('`sampler` only support Sampler type.')
        kwargs = {'num_neg': neg, 'pos_items': pos_items}
        params = inspect.signature(self.sampler.forward).parameters      # baseretriever.py:225-228
        if 'excluding_hist' in params:
            kwargs['excluding_hist'] = excluding_hist
        if 'user_hist' in params:
            kwargs['user_hist'] = user_hist
        kwargs['query'] = query
        pos_prob, neg_id, neg_prob = self.sampler(**kwargs)
        return (pos_prob, neg_id, neg_prob, query) if return_query else (pos_prob, neg_id, neg_prob)

    def _pool_scores(self, query, pool):
        """Scores of every query against its own pool of item ids [.., n0] with the gather+score kernel (ids
        given, no [B, n0, d] tensor) -- no autograd, as in the reference's sampling() (which detaches)."""
        if not (isinstance(self.item_encoder, torch.nn.Embedding)
                and type(self.score_func) in (InnerProductScorer, CosineScorer, EuclideanScorer)):
            raise NotImplementedError("this sampling_method needs an nn.Embedding item tower and a stock scorer")
        n0 = pool.shape[-1]
        with torch.no_grad():
            q2 = query.reshape(-1, query.shape[-1]).contiguous()
            s = ops.fused_forward(self.item_encoder.weight, q2, n0, neg_ids=pool.reshape(-1, n0).contiguous(),
                                  cosine=self.score_func.cosine)['neg_score']
        return s.view(*pool.shape)

    def sampling(self, batch, num_neg, method='none', excluding_hist=False, t=1, return_query=False, query=None):
        """baseretriever.py:248-369, all six methods.  'none' is the sampler plugin; 'dns' / 'sir' (:330-355) draw a
        pool of num_neg[0] ids, score it with the gather+score kernel and keep the num_neg[1] best (`rsa_row_topk`) /
        resample by softmax weight; 'toprand' / 'top&rand' (:280-298) start from the full-catalog top-k (MFMA
        kernel); 'brute' (:300-328) samples from the softmax over the whole catalog.  The random draws of the
        non-default methods are the reference's own torch ops on the device (torch.randint / torch.multinomial),
        so they consume the generator exactly as the reference does."""
        if method not in ('none', 'dns', 'sir', 'toprand', 'top&rand', 'brute'):
            raise NotImplementedError('sampling method only support one of none/brute/sir/dns/toprand/top&rand')
        if isinstance(num_neg, int):
            num_neg = [num_neg, num_neg]
        elif not isinstance(num_neg, (list, tuple)):
            raise TypeError('num_neg only support int and List/Tuple type.')
        assert len(num_neg) == 2 and num_neg[0] >= num_neg[1], 'negative_count must be [pool, kept] with pool >= kept'
        fiid_val = batch.get(self.fiid)
        user_hist = batch.get('user_hist', fiid_val)
        if user_hist is not None and user_hist.dim() == 1:
            user_hist = user_hist.view(-1, 1)          # the positives play the history's role (:259-261)
        if method == 'none':
            assert self.sampler is not None, 'excepted sampler of retriever to be Sampler, but get None.'
            log_pos_prob, neg_id, log_neg_prob, query = self._sample(batch, num_neg[1], excluding_hist, True)
        elif method in ('dns', 'sir'):
            assert self.sampler is not None, 'excepted sampler of retriever to be Sampler, but get None.'
            _, pool, _, query = self._sample(batch, num_neg[0], excluding_hist, True)
            scores = self._pool_scores(query, pool)
            if method == 'dns':
                _, cols = ops.row_topk(scores, num_neg[1])
                neg_id = torch.gather(pool, -1, cols)
                log_neg_prob = torch.zeros_like(neg_id)
                log_pos_prob = torch.zeros_like(fiid_val)
            else:
                with torch.no_grad():
                    log_pos_prob = self.score_func(query, self.item_encoder(self._get_item_feat(batch)))      # :349-351
                    probs = torch.softmax(scores + torch.finfo(torch.float32).eps, dim=-1)
                    resampled = torch.multinomial(probs.reshape(-1, probs.shape[-1]), num_neg[1],
                                                  replacement=True).view(*probs.shape[:-1], num_neg[1])
                neg_id = torch.gather(pool, -1, resampled)
                log_neg_prob = torch.gather(scores, -1, resampled)
        elif method == 'toprand':
            _, topk_items, query = self.topk(batch, k=num_neg[0], user_h=user_hist, return_query=True)
            rand_idx = torch.randint(0, num_neg[0], (topk_items.size(0), num_neg[1]), device=topk_items.device)
            neg_id = torch.gather(topk_items, -1, rand_idx)
            log_neg_prob = torch.zeros_like(neg_id)
            log_pos_prob = torch.zeros_like(fiid_val)
        elif method == 'top&rand':
            k0 = num_neg[1] // 2
            _, neg_id, query = self.topk(batch, k=k0, user_h=user_hist, return_query=True)
            n_q = int(np.prod(query.shape[:-1]))
            rand_ids = torch.randint(1, self.item_vector.size(0) + 1, size=(n_q, num_neg[1] - k0), device=query.device)
            neg_id = torch.cat((neg_id, rand_ids), dim=-1)
            log_neg_prob = torch.zeros_like(neg_id)
            log_pos_prob = torch.zeros_like(fiid_val)
        else:                                                        # 'brute': softmax over the whole catalog
            query = self.query_encoder(self._get_query_feat(batch)) if query is None else query
            pos2 = fiid_val.view(-1, 1) if fiid_val.dim() == 1 else fiid_val
            if self.config['train'].get('brute_stream', False):
                # the same distribution and log-probabilities without the [B, N] matrices (ops.softmax_sample); the ids
                # are not torch.multinomial's for the same seed
                if not isinstance(self.item_encoder, torch.nn.Embedding):
                    raise NotImplementedError("train.brute_stream needs an nn.Embedding item tower (the kernel reads the table's rows)")
                if type(self.score_func) not in (InnerProductScorer, CosineScorer, EuclideanScorer):
                    raise NotImplementedError('train.brute_stream needs a stock InnerProduct / Cosine / Euclidean scorer, got '
                                              f'{type(self.score_func).__name__}')
                if query.dim() != 2:
                    raise NotImplementedError(f'train.brute_stream needs a 2-D query [B, d], got {tuple(query.shape)}')
                out = ops.softmax_sample(self.item_vector.detach(), query.detach(), num_neg[1] * pos2.size(-1), t=t,
                                         score_mode=self.score_func.cosine, pos_ids=pos2,
                                         user_hist=user_hist if excluding_hist else None, items_without_pad=True)
                log_pos_prob, neg_id, log_neg_prob = out['pos_logp'], out['neg_ids'], out['neg_logp']
                result = (log_pos_prob.view_as(fiid_val).detach(), neg_id, log_neg_prob.detach())
                return (result, query) if return_query else (result, None)
            with torch.no_grad():
                all_score = self.score_func(query, self.item_vector) / t
                all_prob = torch.nn.functional.pad(torch.softmax(all_score, dim=-1), pad=(1, 0))
                log_pos_prob = torch.log(torch.gather(all_prob, dim=-1, index=pos2))
                sampling_prob = all_prob
                if excluding_hist:
                    sampling_prob = all_prob.scatter(-1, user_hist, 0.0)        # utils.mask_with_hist(dist, hist, 0)
                neg_id = torch.multinomial(sampling_prob, num_neg[1] * pos2.size(-1), replacement=True)
                log_neg_prob = torch.log(torch.gather(sampling_prob, dim=-1, index=neg_id))
        log_pos_prob = log_pos_prob.view_as(fiid_val)
        result = (log_pos_prob.detach(), neg_id, log_neg_prob.detach())
        return (result, query) if return_query else (result, None)

    def _fullscore_catalog(self):
        """The catalog size (padding row included) when ``topk`` can run the MFMA kernel over ``item_vector`` -- a stock scorer
        over an nn.Embedding item tower --, else None: scores are materialised and ``torch.topk`` selects."""
        if type(self.score_func) in (InnerProductScorer, CosineScorer, EuclideanScorer) \
                and isinstance(self.item_encoder, torch.nn.Embedding):
            return self.item_encoder.weight.shape[0]
        return None

    def topk(self, batch, k, user_h=None, return_query=False):
        """baseretriever.py:374-397: full-catalog scores -> top (k + |hist|) -> drop history -> top k."""
        query = self.query_encoder(self._get_query_feat(batch))
        if getattr(self, '_shard', None) is not None:
            return self._topk_sharded(query, k, user_h, return_query)
        more = user_h.size(1) if user_h is not None else 0
        n_items = self._fullscore_catalog()
        if n_items is not None:
            # the MFMA kernel: scores + exact top-(k + more) without the [B, N] matrix (cosine / Euclidean: the tile
            # epilogue applies the norms, scorer.py:19-34); embed_dim > 128 or k + more > 1024 (a user whose history
            # is longer than that, e.g. ml-1m) are composed from the same kernel on materialised scores (ops.fullscore)
            kc = min(k + more, n_items - 1)
            table = self.item_vector if hasattr(self, 'item_vector') else self._get_item_vector()
            q = query.detach().contiguous()
            in_kernel = min(512, n_items - 1)     # a selection the threshold-filter pass of the kernel still makes (k <= 656)
            if user_h is not None and kc > 1024 and 2 * k <= in_kernel and table.shape[1] <= 128:
                # A history longer than 1024 - k (ml-1m: ~1.8 k) pushes k + |hist| past the in-kernel select and onto
                # materialised scores + torch.topk (25 ms instead of 5.5 at B = 2048, N = 1e6).  The k best items
                # outside the history are among the 512 best overall unless more than 512 - k history items outrank
                # them: select 512 in the kernel, drop the history, and only the rows left with fewer than k survivors
                # (heavy users of a model that ranks their own history first) go through the wide path.
                _, _, score, topk_items = ops.fullscore(table.detach(), q, k=in_kernel, items_without_pad=True,
                                                        score_mode=self.score_func.cosine)
                score, topk_items = ops.topk_mask_history(score, topk_items, user_h, k)
                short = torch.isinf(score[:, k - 1]).nonzero().view(-1)
                if short.numel():
                    _, _, s2, i2 = ops.fullscore(table.detach(), q[short].contiguous(), k=kc, items_without_pad=True,
                                                 score_mode=self.score_func.cosine)
                    s2, i2 = ops.topk_mask_history(s2, i2, user_h[short].contiguous(), k)
                    score[short], topk_items[short] = s2, i2
                return (score, topk_items, query) if return_query else (score, topk_items)
            _, _, score, topk_items = ops.fullscore(table.detach(), q, k=kc,
                                                    items_without_pad=True, score_mode=self.score_func.cosine)
        else:
            score, topk_items = torch.topk(self.score_func(query, self.item_vector), k + more)
            topk_items = topk_items + 1
        if user_h is not None:
            score, topk_items = ops.topk_mask_history(score, topk_items, user_h, min(k, score.shape[1]))
        return (score, topk_items, query) if return_query else (score, topk_items)

    # ------------------------------------------------------------------ steps
    def training_step(self, batch):
        path = self._fused_train_path(batch)
        if path in ('bpr', 'ssm'):
            # single launch: stock BPRLoss / SampledSoftmaxLoss (configs[2]) on the fused kernels with a whole number of
            # 64-negative tiles; the SampledSoftmax logsumexp over the positive and the negatives of a query is carried through
            # its tiles by one wave, the query gradient is accumulated in the forward
            qsrc, qidx = self._query_source(self._get_query_feat(batch))
            fused_loss = fused_bpr_loss if path == 'bpr' else fused_ssm_loss
            loss, _ = fused_loss(self.item_encoder.weight, qsrc, self.neg_count, query_index=qidx, pos_ids=batch[self.fiid],
                                 sampler=self.sampler, sparse_grad=self.config['train'].get('sparse_grad', False))
            return loss
        if path == 'full_softmax':
            # full softmax without the [B, N] score matrix: stock SoftmaxLoss over an nn.Embedding catalog
            output = self.forward(batch, False, return_query=True)
            lse = full_lse(output['query'], self.item_encoder.weight)
            return (lse - output['score']['pos_score']).mean()       # loss_func.py:39-47, first branch
        output = self.forward(batch, isinstance(self.loss_fn, FullScoreLoss))
        score = output['score']
        score['label'] = batch[self.frating]
        return self.loss_fn(**score)

    def _cutoffs(self):
        cutoff = self.config['eval']['cutoff']
        return cutoff if isinstance(cutoff, list) else [cutoff]

    def validation_step(self, batch):
        return self._test_step(batch, self.config['eval']['val_metrics'], self._cutoffs()[:1])

    def test_step(self, batch):
        return self._test_step(batch, self.config['eval']['test_metrics'], self._cutoffs())

    def _test_step(self, batch, metric, cutoffs):
        rank_m = rs_eval.get_rank_metrics(metric)
        topk = self.config['eval']['topk']
        bs = batch[self.frating].size(0)
        assert len(rank_m) > 0
        score, topk_items = self.topk(batch, topk, batch['user_hist'])
        n_valid = batch.get('_n_valid')
        if n_valid is not None and n_valid < bs:
            # this rank's part of a global evaluation batch the world size did not divide: the trailing rows are padding
            # (dataset.rank_part) -- they took part in the (collective) top-k above and are dropped from the metrics
            if n_valid == 0:
                return {f'{name}@{cutoff}': 0.0 for cutoff in cutoffs for name, _ in rank_m}, 0
            bs = n_valid
            topk_items = topk_items[:bs]
            batch = dict(batch, **{self.fiid: batch[self.fiid][:bs], self.frating: batch[self.frating][:bs]})
        if batch[self.fiid].dim() > 1:
            target, _ = batch[self.fiid].sort()
            idx_ = torch.searchsorted(target, topk_items)
            idx_[idx_ == target.size(1)] = target.size(1) - 1
            label = torch.gather(target, 1, idx_) == topk_items
            pos_rating = batch[self.frating]
        else:
            label = batch[self.fiid].view(-1, 1) == topk_items
            pos_rating = batch[self.frating].view(-1, 1)
        return {f'{name}@{cutoff}': func(label, pos_rating, cutoff) for cutoff in cutoffs for name, func in rank_m}, bs

    # ------------------------------------------------------------------ minimal fit / evaluate loop
    def _device(self):
        if not torch.cuda.is_available():
            raise RuntimeError('recstudio_amd trains on a ROCm GPU only (no CPU fallback)')
        gpu = self.config['train'].get('gpu', 1)
        idx = gpu[0] if isinstance(gpu, (list, tuple)) and gpu else 0
        return torch.device('cuda', int(idx) if isinstance(idx, int) and idx < torch.cuda.device_count() else 0)

    def _get_optimizer(self):
        tr = self.config['train']
        name, lr = tr['learner'].lower(), tr['learning_rate']
        params = [p for p in self.parameters() if p.requires_grad]
        if tr.get('sparse_grad', False):
            return torch.optim.SparseAdam(params, lr=lr) if name == 'adam' else torch.optim.SGD(params, lr=lr)
        return self._make_optimizer(params)

    def _get_scheduler(self, optimizer):
        """recommender.py:476-494: ``train.scheduler`` = 'exponential' (gamma 0.98) | 'onplateau' | None, stepped once
        per epoch (the plateau scheduler on the monitored validation metric, else on the training loss)."""
        name = self.config['train'].get('scheduler')
        if name is None or optimizer is None:
            return None
        if name.lower() == 'exponential':
            return torch.optim.lr_scheduler.ExponentialLR(optimizer, gamma=0.98)
        if name.lower() == 'onplateau':
            return torch.optim.lr_scheduler.ReduceLROnPlateau(optimizer, mode=self.config['train'].get('early_stop_mode', 'max'))
        return None

    def _step_scheduler(self, scheduler, log):
        if scheduler is None:
            return
        if isinstance(scheduler, torch.optim.lr_scheduler.ReduceLROnPlateau):
            scheduler.step(log.get(getattr(self, 'val_metric', None), log['train_loss']))
        else:
            scheduler.step()
        log['lr'] = float(scheduler.optimizer.param_groups[0]['lr'])

    def _to_device(self, batch, device):
        def move(v):
            if isinstance(v, torch.Tensor):
                return v.to(device, non_blocking=True)
            if isinstance(v, tuple):
                return tuple(move(x) for x in v)
            return v
        return {k: move(v) for k, v in batch.items()}

    # ------------------------------------------------------------------ multi-GPU fit / evaluate (row-sharded item table)
    def _dist_context(self, kwargs):
        """The process group this ``fit`` runs in when it is ONE RANK of a multi-process job: ``fit(..., dist=...)`` (a
        torch.distributed look-alike; forces the sharded path at any world size), an initialised torch.distributed
        with more than one rank, or a launcher environment (WORLD_SIZE > 1: the group is created here, RCCL, one rank
        per GPU).  None: single-process training.  Replaces recommender.py:608-612, :716-742 (``data_parallel`` /
        ``_accelerate``: every parameter re-broadcast to a gpu list each step; the ddp branch raises)."""
        dist = kwargs.get('dist')
        if dist is not None:
            return dist
        import torch.distributed as td
        if not td.is_available():
            return None
        if not td.is_initialized() and int(os.environ.get('WORLD_SIZE', '1')) > 1:
            local = int(os.environ.get('LOCAL_RANK', '0'))
            os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
            torch.cuda.set_device(local)
            td.init_process_group('nccl', device_id=torch.device('cuda', local))
        if td.is_initialized() and td.get_world_size() > 1:
            return td
        gpu = self.config['train'].get('gpu', 1)
        n_gpu = len(gpu) if isinstance(gpu, (list, tuple)) else (gpu if isinstance(gpu, int) else 1)
        if n_gpu > 1:
            # the reference would now replicate the model over the gpu list inside this process (accelerator 'dp') or raise
            # ('ddp'); here multi-GPU training is one process per GPU
            self.logger.warning(f"train.gpu asks for {n_gpu} GPUs but this is a single process: training on one GPU.  Start the "
                                f"same script with `python -m torch.distributed.run --nproc-per-node {n_gpu} --master-addr "
                                f"127.0.0.1 script.py` and fit() shards the item table over the ranks.")
        return None

    def _setup_shard(self, train_data, dist, backend=None, device=None):
        """Row-shard the item table over the ranks of ``dist``: rank r keeps rows [lo, hi) -- with ``train.shard_layout:
        'interleaved'`` rows r, r + G, ... -- of ``item_encoder.weight`` (and,
        through the optimizer, of its Adam state) as an ``nn.Embedding`` of its own block; sampler and query tower are
        replicated.  Every rank initialises the full model from the same seed first (recommender.py:34-35), so the
        shards are the rows of the very table a single process would train."""
        from . import shard
        rank, world = dist.get_rank(), dist.get_world_size()
        if not (isinstance(self.item_encoder, torch.nn.Embedding) and len(self.item_fields) == 1
                and type(self.score_func) is InnerProductScorer and isinstance(self.loss_fn, PairwiseLoss)
                and self.sampler is not None and self.config['train'].get('sampling_method', 'none') == 'none'
                and isinstance(self.neg_count, int) and self.neg_count > 0):
            raise NotImplementedError('multi-GPU fit covers the two-tower configuration: nn.Embedding item tower over the item '
                                      'id, InnerProductScorer, a PairwiseLoss, a Sampler with sampling_method "none"')
        if device is None:
            if backend is not None:
                raise ValueError('a non-default shard backend needs an explicit device')
            device = torch.device('cuda', int(os.environ.get('LOCAL_RANK', torch.cuda.current_device())))
        device = torch.device(device)
        n_items, d = self.item_encoder.weight.shape
        plan = shard.RowShardPlan(n_items, world, layout=self.config['train'].get('shard_layout', 'block'))
        if self.item_encoder.weight.is_meta:
            rows = _device_init_block(plan, rank, n_items, d, self.config['train']['seed'] or 2022,
                                      self.config['train']['init_method'], device)
            if rank == 0 and self.item_encoder.padding_idx is not None:
                rows[self.item_encoder.padding_idx] = 0
        else:
            rows = plan.take(self.item_encoder.weight.detach(), rank).clone()
        block = torch.nn.Embedding(plan.n_local(rank), d, padding_idx=0 if rank == 0 else None, _weight=rows)
        # An ITEM-TOWER query encoder (SASRec: seq/sasrec.py:14, :42, :107) embeds its input with the very table the
        # model scores against.  Every place the tower holds that module is re-pointed at the sharded table below
        # (shard.ShardedRows: ids out, rows back, gradients to the owners), so the embedding stays tied and no rank
        # keeps -- or dense-all-reduces the gradient of -- a replica of the catalog.
        full = self.item_encoder
        tied = []
        if isinstance(self.query_encoder, torch.nn.Module):
            tied = [(mod, name) for mod in self.query_encoder.modules() for name, child in mod._modules.items() if child is full]
            for mod, name in tied:
                mod._modules[name] = None
            if any(p is full.weight for p in self.query_encoder.parameters()):
                for mod, name in tied:
                    mod._modules[name] = full
                raise NotImplementedError('multi-GPU fit: the query tower uses item_encoder.weight outside the item_encoder '
                                          'module itself; only towers that call their item_encoder submodule can be sharded')
        self.item_encoder = block                      # the full table is dropped: this rank keeps its rows only
        lo, hi = (None, None) if plan.interleaved else plan.bounds(rank)
        if hasattr(self, 'item_vector'):
            del self.item_vector
        self.to(device)
        table = shard.ShardedItemTable(self.item_encoder.weight.data, plan, rank, dist, backend=backend,
                                       sample_seed=self.config['train']['seed'] or 2022,
                                       chunks=int(self.config['train'].get('shard_slices', 1)),
                                       owner_loss=bool(self.config['train'].get('shard_owner_loss', True)),
                                       deterministic=bool(self.config['train'].get('shard_deterministic', True)),
                                       rows_share=self.config['train'].get('shard_rows_share'))
        self._shard = {'table': table, 'dist': dist, 'rank': rank, 'world': world, 'lo': lo, 'hi': hi, 'device': device,
                       'n_items': n_items, 'plan': plan, 'tower_rows': None}
        if tied:
            rows = shard.ShardedRows(table)
            for mod, name in tied:
                mod._modules[name] = rows
            self._shard['tower_rows'] = rows
        return self._shard

    def _topk_sharded(self, query, k, user_h, return_query):
        """``topk`` over the sharded catalog: per-shard MFMA pass + exchange of the (value, id) partials
        (ShardedItemTable.full_lse_topk), then the history exclusion of baseretriever.py:386-392.  The candidate count is
        k + the width of the WHOLE history table (the same on every rank: the collectives need equal shapes) -- at least
        as many candidates as the single-process path keeps, so the k survivors are the same."""
        sh = self._shard
        table, be = sh['table'], sh['table'].backend
        more = sh.get('hist_width', user_h.size(1) if user_h is not None else 0)
        kc = min(k + more, sh['n_items'] - 1)
        mask = be.mask_history if hasattr(be, 'mask_history') else ops.topk_mask_history
        q = query.detach().contiguous()
        narrow = min(sh.get('topk_narrow', 512), sh['n_items'] - 1)
        if user_h is not None and kc > ops.FULLSCORE_MAX_K and 2 * k <= narrow:
            # a history longer than 1024 - k (ml-1m: ~1.8 k): the single-process strategy (``topk`` above) with
            # rank-uniform shapes -- 512 candidates over the whole catalog, history dropped; only if ANY row of ANY rank is
            # left with fewer than k survivors (one flag, all-reduced: every rank takes the same branch) does the batch
            # go through the wide pass
            _, score, topk_items = table.full_lse_topk(q, narrow, want_lse=False)
            score, topk_items = mask(score, topk_items, user_h, k)
            short = torch.isinf(score[:, k - 1]).any().to(torch.int32).reshape(1)
            table._all_reduce_max(short)
            if not int(short):
                return (score, topk_items, query) if return_query else (score, topk_items)
        _, score, topk_items = table.full_lse_topk(q, kc, want_lse=False)
        if user_h is not None:
            score, topk_items = mask(score, topk_items, user_h, min(k, score.shape[1]))
        else:
            score, topk_items = score[:, :k], topk_items[:, :k]
        return (score, topk_items, query) if return_query else (score, topk_items)

    def _prepared_batches(self, loader, device):
        for batch in loader:
            batch = self._to_device(batch, device)
            batch.pop('_n_valid', None)
            yield batch

    def _fit_sharded(self, train_data, val_data, dist, backend=None, device=None):
        """One process per GPU, item table row-sharded, query tower replicated (``shard.ShardedRetriever``): rank r trains on
        its contiguous 1/G of every global batch (``train.batch_size`` is per rank), the negatives come from one job-wide
        stream, the loss is the global mean -- a G-rank run reproduces the single-process run on the global batch up to
        fp32 summation order.  The optimizer is the reference's (``train.learner``) on this rank's parameters: its own
        row block (with its block of the optimizer state) and its replica of the tower, whose gradients are summed over
        the ranks first; ``train.fused_optimizer: 'sgd'`` applies plain SGD inside the exchange instead."""
        from . import shard
        # train.shard_init: 'host' = every rank initialises the full table as a single process would and keeps its rows
        # (bit-equal to the unsharded model's initial weights); 'device' = the rows are drawn on the owner's device, the
        # full table never exists anywhere (_device_init_block); 'auto' (default): 'device' once the table exceeds 2 GiB
        mode = self.config['train'].get('shard_init', 'auto')
        self._item_table_on_meta = mode == 'device' or (mode == 'auto' and not self.item_encoder and
                                                          train_data.num_items * self.embed_dim * 4 > (2 << 30))
        self._init_model(train_data)
        self._init_parameter()
        sh = self._setup_shard(train_data, dist, backend, device)
        table, rank, world, device = sh['table'], sh['rank'], sh['world'], sh['device']
        if hasattr(self.sampler, 'to'):
            self.sampler.to(device)
        if getattr(type(self.sampler), 'update', Sampler.update) is not Sampler.update:
            raise NotImplementedError('multi-GPU fit: samplers with a per-epoch update() are not covered')
        if val_data is not None:
            val_data.use_field = train_data.use_field
        tr = self.config['train']
        if hasattr(train_data, 'user_hist') and train_data.user_hist is not None:
            sh['hist_width'] = int(max(train_data.user_hist.shape[1], getattr(val_data, 'user_hist', train_data.user_hist).shape[1]))
        fused = tr.get('fused_optimizer')
        if fused not in (None, 'sgd'):
            raise NotImplementedError("multi-GPU fit: train.fused_optimizer must be None or 'sgd'")
        lr = tr['learning_rate']
        embed_tower = isinstance(self.query_encoder, torch.nn.Embedding)
        trainer = shard.ShardedRetriever(table, self.query_encoder, self.sampler, self.loss_fn, self.neg_count,
                                         item_sgd_lr=lr if fused else None,
                                         query_sgd_lr=lr if (fused and embed_tower) else None)
        optimizer = None
        if not fused or not embed_tower:
            params = [p for p in self.parameters() if p.requires_grad and not (fused and p is self.item_encoder.weight)]
            optimizer = self._make_optimizer(params) if params else None
        if not fused:
            self.item_encoder.weight.grad = trainer.item_grad_local       # the exchange accumulates into the block's .grad
        scheduler = self._get_scheduler(_stand_in_optimizer(lr) if fused and embed_tower and tr.get('scheduler') else optimizer)
        sh['trainer'] = trainer
        trainer.table.defer_overflow = True          # report a capacity overflow after the step instead of raising inside it
        if sh['tower_rows'] is not None:
            sh['tower_rows'].bind(trainer)
        on_gpu = device.type == 'cuda'
        self.train_losses = []
        prepare = lambda batch: trainer.prepare_step(self._get_query_feat(batch), batch[self.fiid])      # noqa: E731

        def step(batch, ticket):
            if optimizer is not None:
                optimizer.zero_grad(set_to_none=False)
            loss = trainer.training_step(self._get_query_feat(batch), batch[self.fiid], batch[self.frating], ticket=ticket)
            if optimizer is not None:
                if tr['grad_clip_norm'] is not None:
                    self._clip_grad_norm_sharded(params, tr['grad_clip_norm'], dist)
                optimizer.step()
            # an id distribution that outgrew the calibrated segment capacity: the poll (every rank sees the job-wide
            # sticky count at the same step) reports it HERE, after the whole step -- the steps in which elements were
            # dropped updated nothing (their scale was 0 on the device), the step the lagging poll landed in is a healthy
            # one and has run to its end, the capacity is recalibrated on the next step; carry on
            msg = trainer.table.take_overflow()
            if msg:
                self.logger.warning(msg)
            return loss.detach().reshape(1)

        def train_epoch():
            # train.shard_lookahead: the weight-independent half of the NEXT batch's step (negatives, routing, key exchange,
            # the owner's sorts) is issued on a second stream before the current batch is stepped (ShardedRetriever.prepare_step)
            ahead = bool(tr.get('shard_lookahead', False)) and trainer.can_prepare()
            self._shard['lookahead'] = ahead
            if on_gpu and tr.get('device_loader', True) and hasattr(train_data, 'device_train_loader'):
                loader = train_data.device_train_loader(tr['batch_size'], shuffle=True, drop_last=False, device=device, ddp=True,
                                                        rank=rank, world=world)
                # the rank parts of one global batch: every rank's history window has the same shape, so a tower's row
                # look-ups can travel in fixed-capacity segments (no host round trip per step).  NOT with look-ahead: a
                # fixed-capacity look-up hands its dropped count to the NEXT routing launch, which with look-ahead belongs to a
                # batch prepared one or two steps earlier on the other stream -- the step whose look-up overflowed would run
                # ungated.  The variable-split look-up cannot drop anything.
                trainer.table.uniform_lookups = not ahead
            else:
                loader = train_data.train_loader(batch_size=tr['batch_size'], shuffle=True, drop_last=False, ddp=True,
                                                 rank=rank, world=world)
            with _above_second_stream(ahead and on_gpu, device, self._shard):
                losses = _one_ahead(self._prepared_batches(loader, device), step, prepare if ahead else None)
            step_losses = torch.cat(losses)                     # this rank's shares of the global mean losses
            dist.all_reduce(step_losses)      # (the all-reduced loss / metric: the same scheduler decision on every rank)
            self.train_losses.append(step_losses.cpu())
            return float(step_losses.mean())

        validate = (lambda: self._eval_epoch(val_data, self.validation_step, device)) if val_data is not None else None
        return self._run_epochs(train_epoch, scheduler, validate, on_lr=trainer.set_sgd_lr if fused else None,
                                log=self.logger.info if rank == 0 else None,
                                after_restore=lambda: setattr(table, 'item_local', self.item_encoder.weight.data))

    def _run_epochs(self, train_epoch, scheduler, validate=None, on_lr=None, log=None, after_restore=None):
        """The epoch loop of ``fit``, single-process and sharded: ``train_epoch() -> loss`` every epoch, ``validate() -> metrics``
        every ``eval.val_n_epoch`` epochs (None: no validation data), early stopping on ``self.val_metric``, one scheduler step per
        epoch with the new rate handed to ``on_lr``, one ``history`` entry and one ``log(line)`` per epoch (``log`` None: this
        process does not log); at the end the best state is restored and ``after_restore()`` called.  Returns the best metric."""
        tr, val_metrics = self.config['train'], self.config['eval']['val_metrics']
        self.val_metric = f"{(val_metrics[0] if isinstance(val_metrics, list) else val_metrics)}@{self._cutoffs()[0]}"
        best, best_state, bad = None, None, 0
        self.history = []                                  # one dict per epoch: what the reference logs (recommender.py:249-270)
        for epoch in range(tr['epochs']):
            t0 = time.time()
            self.train()
            entry = {'epoch': epoch, 'train_loss': train_epoch(), 'train_time': time.time() - t0}
            if validate is not None and (epoch + 1) % self.config['eval']['val_n_epoch'] == 0:
                entry.update(validate())
                cur = entry[self.val_metric]
                better = best is None or (cur > best if tr['early_stop_mode'] == 'max' else cur < best)
                if better:
                    best, best_state, bad = cur, copy.deepcopy(self.state_dict()), 0
                else:
                    bad += 1
            self._step_scheduler(scheduler, entry)
            if on_lr is not None and scheduler is not None:
                on_lr(entry['lr'])
            self.logged_metrics = entry
            self.history.append(dict(entry))
            if log is not None:
                log(' '.join(f'{k}={v:.4f}' if isinstance(v, float) else f'{k}={v}' for k, v in entry.items()))
            if validate is not None and bad >= tr['early_stop_patience']:
                break
        if best_state is not None:
            self.load_state_dict(best_state)
            if after_restore is not None:
                after_restore()
        return best

    def _clip_grad_norm_sharded(self, params, max_norm, dist):
        """``torch.nn.utils.clip_grad_norm_`` (recommender.py training loop) over a model whose item table is split over the
        ranks: the squared norm of this rank's row block is summed over the ranks, the replicated tower's gradients
        (already summed, identical everywhere) count once; every rank scales by the same coefficient."""
        block = self.item_encoder.weight
        sq_block = torch.zeros((), device=block.device)
        sq_rest = torch.zeros((), device=block.device)
        for p in params:
            if p.grad is None:
                continue
            if p is block:
                sq_block = sq_block + p.grad.float().pow(2).sum()
            else:
                sq_rest = sq_rest + p.grad.float().pow(2).sum()
        dist.all_reduce(sq_block)
        total = (sq_block + sq_rest).sqrt()
        coef = torch.clamp(max_norm / (total + 1e-6), max=1.0)
        for p in params:
            if p.grad is not None:
                p.grad.mul_(coef)
        return total

    def _make_optimizer(self, params):
        tr = self.config['train']
        name, lr, wd = tr['learner'].lower(), tr['learning_rate'], tr['weight_decay']
        table = {'adam': torch.optim.Adam, 'sgd': torch.optim.SGD, 'adagrad': torch.optim.Adagrad,
                 'rmsprop': torch.optim.RMSprop}
        return table.get(name, torch.optim.Adam)(params, lr=lr, weight_decay=wd)

    def fit(self, train_data, val_data=None, run_mode='light', config: Dict = None, **kwargs):
        if config is not None:
            self.config.update(config)
        dist = self._dist_context(kwargs)
        if dist is not None:
            return self._fit_sharded(train_data, val_data, dist, kwargs.get('shard_backend'), kwargs.get('device'))
        self._init_model(train_data)
        self._init_parameter()
        device = self._device()
        self.to(device)
        if val_data is not None:
            val_data.use_field = train_data.use_field
        optimizer = self._get_optimizer()
        tr = self.config['train']
        fused_step = self._fused_step = self._fused_optimizer_step(tr)
        scheduler = self._get_scheduler(_stand_in_optimizer(tr['learning_rate']) if fused_step is not None else optimizer)
        # the device-resident loader is built once: its columns are uploaded once, every epoch re-draws the order
        dev_loader = train_data.device_train_loader(tr['batch_size'], shuffle=True, drop_last=False, device=device) \
            if tr.get('device_loader', True) and hasattr(train_data, 'device_train_loader') else None
        prepare = None
        if fused_step is not None and fused_step.stepper is not None:
            # one batch of look-ahead: the next step's negatives are drawn and sorted on a side stream while this
            # step's forward and apply passes run (fused.PrefetchedBPRSGD; same weights bit for bit)
            stepper = fused_step.stepper
            prepare = lambda batch: stepper.prepare(batch[self.fuid], batch[self.fiid])      # noqa: E731
            step = lambda batch, ticket: stepper.step(ticket)[0]                               # noqa: E731
        else:
            def step(batch, ticket):
                if fused_step is not None and batch[self.fiid].dim() == 1:
                    return fused_step(batch)        # forward + loss + optimizer update in the kernels
                optimizer.zero_grad()
                loss = self.training_step(batch)
                loss.backward()
                if tr['grad_clip_norm'] is not None:
                    torch.nn.utils.clip_grad_norm_(self.parameters(), tr['grad_clip_norm'])
                optimizer.step()
                return loss.detach()

        def train_epoch():
            self._update_item_vector()
            if self.sampler is not None:
                self.sampler.update(item_embs=self.item_vector)                 # recommender.py:564-570
            loader = dev_loader if dev_loader is not None else \
                train_data.train_loader(batch_size=tr['batch_size'], shuffle=True, drop_last=False)
            losses = _one_ahead((self._to_device(batch, device) for batch in loader), step, prepare)
            return float(torch.stack(losses).mean())

        def validate():
            t1 = time.time()
            metrics = self._eval_epoch(val_data, self.validation_step, device)
            return dict(metrics, valid_time=time.time() - t1)     # the reference logs both times (recommender.py:262-266)

        return self._run_epochs(train_epoch, scheduler, validate if val_data is not None else None,
                                on_lr=fused_step.set_lr if fused_step is not None else None, log=self.logger.info)

    def _fused_optimizer_step(self, tr):
        """``train.fused_optimizer: 'sgd' | 'adam' | 'learner'`` (default None = the reference's torch optimizer on autograd
        gradients): for the stock BPR two-tower configuration (nn.Embedding towers, InnerProductScorer, BPRLoss,
        Uniform / Popular sampler, negative_count % 64 == 0, embed_dim in {64, 128, 256}) run the whole step --
        sampling, scoring, loss, and the SGD / lazy-Adam update of the touched rows -- in the kernels, with no gradient
        tensors (fused.bpr_sgd_step / fused.FusedBPRAdam).  'adam' follows torch.optim.SparseAdam (rows outside the
        batch keep their state), which differs from the dense Adam the reference runs by default.  'learner' runs the rule
        ``train.learner`` names: 'sgd' as above, 'adagrad' = torch.optim.Adagrad with its defaults (fused.FusedBPRAdagrad; exact,
        not lazy: a zero gradient changes neither a row's state_sum nor its weight); any other learner is refused."""
        kind = tr.get('fused_optimizer')
        if not kind:
            return None
        conf = lambda k: tr[k] if k in tr else self.config['train'][k]      # noqa: E731  (a partial ``tr``: the model's own settings)
        if not (self._fused_train_path() == 'bpr' and isinstance(self.neg_count, int)
                and isinstance(self.query_encoder, torch.nn.Embedding) and self.item_encoder.weight.shape[1] in (64, 128, 256)
                and not tr.get('weight_decay') and tr.get('grad_clip_norm') is None):
            raise NotImplementedError("train.fused_optimizer needs the stock BPR two-tower configuration "
                                      "(see BaseRetriever._fused_optimizer_step)")
        if kind not in ('sgd', 'adam', 'learner'):
            raise ValueError(f"train.fused_optimizer must be 'sgd' or 'adam', or 'learner' (the rule train.learner names), got {kind!r}")
        if kind == 'learner':
            # the reference's own learner inside the kernels: the two whose row-sparse step IS the dense rule (a zero gradient moves
            # neither the weight nor Adagrad's state_sum).  Dense Adam moves every row in every step: 'adam' above is SparseAdam.
            kind = str(conf('learner')).lower()
            if kind not in ('sgd', 'adagrad'):
                raise NotImplementedError(f"train.fused_optimizer: 'learner' covers train.learner 'sgd' and 'adagrad', got {kind!r}")
        # look-ahead: 'sgd' only on the in-forward step (one 64-negative tile); it does not pay for lazy Adam -- in-process A/B
        # at the headline shape: 2.61 ms plain, 2.68 ms one batch ahead: the draw leaves the forward for the stand-alone sampler
        # and the apply pass is the step -- so there it is opt-in: train.fused_prefetch: 'adam'
        prefetch = tr.get('fused_prefetch', True)
        # (Adagrad's step has Adam's shape -- stand-alone sampler, two sorts, two apply passes: opt-in too, train.fused_prefetch: 'adagrad')
        ahead = bool(self.neg_count == 64 and prefetch and self.fiid is not None) if kind == 'sgd' else prefetch == kind
        cls = {'sgd': BPRSGDStep, 'adam': BPRAdamStep, 'adagrad': BPRAdagradStep}[kind]
        return cls(self.item_encoder.weight, self.query_encoder.weight, self.neg_count, conf('learning_rate'), self.sampler,
                   self.fuid, self.fiid, ahead)

    @torch.no_grad()
    def _eval_epoch(self, data, step, device):
        self.eval()
        sh = getattr(self, '_shard', None)
        if sh is None:
            self._update_item_vector()
            loader = data.eval_loader(batch_size=self.config['eval']['batch_size'])
        else:       # this rank's contiguous part of every global evaluation batch (dataset.py:1141-1142)
            loader = data.eval_loader(batch_size=self.config['eval']['batch_size'], ddp=True, rank=sh['rank'], world=sh['world'])
        total, rows, sizes = 0, [], []
        for batch in self._eval_batches(data, loader, device, cache=sh is None):
            metrics, bs = step(batch)
            # per-batch values stay on the device until the epoch ends: float(v) here was one host synchronisation per
            # metric per batch (most of an ml-100k validation epoch)
            rows.append(metrics)
            sizes.append(bs)
            total += bs
        acc = {}
        if rows:
            keys = list(rows[0])
            vals = torch.stack([torch.stack([torch.as_tensor(m[k], dtype=torch.float32, device=device) for k in keys])
                                for m in rows]).double().cpu()
            for r, bs in enumerate(sizes):                                         # weighted mean, recommender.py:308-324
                for c, k in enumerate(keys):
                    acc[k] = acc.get(k, 0.0) + float(vals[r, c]) * bs
        if sh is not None:                                                     # sums over the ranks' parts
            keys = sorted(acc)
            t = torch.tensor([acc[k] for k in keys] + [float(total)], dtype=torch.float64, device=device)
            if t.device.type == 'cuda':
                t = t.float()
            sh['dist'].all_reduce(t)
            acc, total = {k: float(v) for k, v in zip(keys, t[:-1])}, float(t[-1])
        return {k: v / max(total, 1) for k, v in acc.items()}

    EVAL_CACHE_BYTES = 1 << 30

    def _eval_batches(self, data, loader, device, cache=True):
        """The evaluation batches of ``data`` on the device.  An evaluation split does not change between epochs, so the
        host loader's work (per-user ragged slices, ``pad_sequence``, the history rows, the uploads) is done once: the
        device-resident batches of a split are kept (up to EVAL_CACHE_BYTES over all splits) and replayed every epoch."""
        store = self.__dict__.setdefault('_eval_cache', {})
        key = (id(data), self.config['eval']['batch_size'], str(device), len(data))
        hit = store.get(key)
        if hit is not None and hit[0] is data:
            yield from hit[1]
            return
        kept, size = [], 0
        budget = self.EVAL_CACHE_BYTES - sum(v[2] for v in store.values())
        for batch in loader:
            batch = self._to_device(batch, device)
            if cache and kept is not None:
                size += sum(v.numel() * v.element_size() for v in batch.values() if isinstance(v, torch.Tensor))
                if size > budget:
                    kept = None
                else:
                    kept.append(batch)
            yield batch
        if cache and kept is not None:
            store[key] = (data, kept, size)

    def evaluate(self, test_data, verbose=True, **kwargs):
        test_data.use_field = self.fields
        sh = getattr(self, '_shard', None)
        if sh is not None and getattr(test_data, 'user_hist', None) is not None:
            sh['hist_width'] = max(sh.get('hist_width', 0), int(test_data.user_hist.shape[1]))
        out = self._eval_epoch(test_data, self.test_step, next(self.parameters()).device)
        if verbose:
            self.logger.info(str(out))
        return out


TwoTowerRecommender = BaseRetriever      # README.md:29-31 names
ItemTowerRecommender = BaseRetriever


class BPR(BaseRetriever):
    """recstudio/model/mf/bpr.py:7-25, recstudio/model/mf/config/bpr.yaml (negative_count: 1)."""

    def __init__(self, config=None, **kwargs):
        super().__init__(config, **kwargs)
        if 'negative_count' not in (config or {}).get('train', {}):
            self.config['train']['negative_count'] = 1

    def _get_dataset_class():
        return TripletDataset

    def _get_item_encoder(self, train_data):
        return torch.nn.Embedding(train_data.num_items, self.embed_dim, padding_idx=0)

    def _get_query_encoder(self, train_data):
        return torch.nn.Embedding(train_data.num_users, self.embed_dim, padding_idx=0)

    def _get_score_func(self):
        return InnerProductScorer()

    def _get_loss_func(self):
        return BPRLoss()

    def _get_sampler(self, train_data):
        return UniformSampler(train_data.num_items)


class LightGCN(BaseRetriever):
    """recstudio/model/graph/lightgcn.py:14-84, recstudio/model/graph/config/{all,lightgcn}.yaml (n_layers 3, l2_reg_weight 1e-4,
    negative_count 1).  The base tables ``user_emb`` / ``item_emb`` are propagated over the normalised interaction graph
    (``graphmodule.NormAdj``, ``rsa_spmm_csr``); everything behind the propagation is the fused path: the propagated item table is
    the ``item_weight`` of ``fused.retriever_scores``, the propagated user table its ``query_src`` with the batch's user ids as
    ``query_index`` -- the negatives are drawn in the kernel (the ids ``UniformSampler`` gives for the seed), no [B, n, d] tensor
    exists, and the dense table gradients flow back into the propagation's backward.  The towers are not nn.Embedding modules,
    so ``train.fused_optimizer``, multi-GPU ``fit`` and ``train.ann`` refuse this model as they refuse any such tower."""

    def __init__(self, config=None, **kwargs):
        super().__init__(config, **kwargs)
        self.config['model'].setdefault('n_layers', 3)
        self.config['model'].setdefault('l2_reg_weight', 1e-4)
        given = config or {}
        for group, key, value in (('train', 'negative_count', 1), ('train', 'early_stop_patience', 100), ('eval', 'cutoff', [20, 10, 5])):
            if key not in given.get(group, {}):
                self.config[group][key] = value

    def _init_model(self, train_data, drop_unused_field=True):
        from . import graphmodule
        super()._init_model(train_data, drop_unused_field)
        self.num_users, self.num_items = train_data.num_users, train_data.num_items
        self.user_emb = torch.nn.Embedding(self.num_users, self.embed_dim, padding_idx=0)
        self.item_emb = torch.nn.Embedding(self.num_items, self.embed_dim, padding_idx=0)
        net = self._get_gnn_net()
        setattr(self, type(net).__name__, net)
        self.adj_mat = self._get_graph(train_data)

    def _get_gnn_net(self):
        """The propagation module; ``_init_model`` registers it under its class name."""
        from . import graphmodule
        return graphmodule.LightGCNNet(self.config['model']['n_layers'])

    def _get_graph(self, train_data):
        """The normalised adjacency of the training interactions (``model.spmm_chunk``: the chunk size of its plan, default
        ``ops.SPMM_CHUNK``)."""
        from . import graphmodule
        return graphmodule.NormAdj.from_dataset(train_data, chunk=self.config['model'].get('spmm_chunk'))

    def _get_dataset_class():
        return TripletDataset

    def _get_loss_func(self):
        return BPRLoss()

    def _get_score_func(self):
        return InnerProductScorer()

    def _get_sampler(self, train_data):
        return UniformSampler(train_data.num_items)

    def _get_query_encoder(self, train_data):
        from . import graphmodule
        return graphmodule.GraphUserEncoder()

    def _get_item_encoder(self, train_data):
        from . import graphmodule
        return graphmodule.GraphItemEncoder()

    def _propagate(self, embeddings):
        return self.LightGCNNet.propagate(self.adj_mat, embeddings)

    def update_encoders(self):
        embeddings = torch.cat([self.user_emb.weight, self.item_emb.weight], dim=0)
        all_embeddings = self._propagate(embeddings)
        self.query_encoder.user_embeddings, self.item_encoder.item_embeddings = \
            all_embeddings[:self.num_users], all_embeddings[self.num_users:]

    def forward(self, batch, full_score=False, return_query=True, return_item=True, return_neg_item=False, return_neg_id=True):
        self.update_encoders()
        users, items = self.query_encoder.user_embeddings, self.item_encoder.item_embeddings
        pos_items, uid = self._get_item_feat(batch), batch[self.fuid]
        if self.neg_count is None or isinstance(self.neg_count, (list, tuple)) or type(self.score_func) is not InnerProductScorer \
                or self.config['train'].get('sampling_method', 'none') != 'none' or pos_items.dim() != 1:
            return self._forward_plugins(batch, full_score, return_query, return_item, return_neg_item, return_neg_id)
        n = self.neg_count
        score, neg_ids = retriever_scores(items, users, n, query_index=uid, pos_ids=pos_items, sampler=self.sampler)
        output = {'score': {'pos_score': score['pos_score'], 'log_pos_prob': score['log_pos_prob'].detach(),
                            'neg_score': score['neg_score'].view(-1, n), 'log_neg_prob': score['log_neg_prob'].view(-1, n).detach()}}
        if return_neg_id:
            output['neg_id'] = neg_ids.view(-1, n)
        if return_neg_item:
            output['neg_item'] = self.item_encoder(neg_ids.view(-1, n))
        if return_query:
            output['query'] = self.query_encoder(uid)
        if return_item:
            output['item'] = self.item_encoder(pos_items)
        return output

    def training_step(self, batch):
        from .loss_func import l2_reg_loss_fn
        output = self.forward(batch, isinstance(self.loss_fn, FullScoreLoss), return_query=False, return_item=False, return_neg_id=True)
        score = dict(output['score'], label=batch[self.frating])
        # the regulariser sees the BASE rows of the batch (lightgcn.py:72-73), through the gather / sorted-scatter autograd node
        reg = l2_reg_loss_fn(_EmbedFn.apply(self.user_emb.weight, batch[self.fuid]),
                             _EmbedFn.apply(self.item_emb.weight, batch[self.fiid]),
                             _EmbedFn.apply(self.item_emb.weight, output['neg_id'].reshape(-1)))
        return self.loss_fn(**score) + self.config['model']['l2_reg_weight'] * reg

    def _get_item_vector(self):
        if self.item_encoder.item_embeddings is None:
            return self.item_emb.weight[1:].detach().clone()
        return self.item_encoder.item_embeddings[1:].detach().clone()

    @torch.no_grad()
    def _update_item_vector(self):
        self.update_encoders()
        super()._update_item_vector()

    def _fullscore_catalog(self):
        # ``item_vector`` is a plain fp32 table (the propagated item rows): the MFMA top-k reads it as it reads an nn.Embedding's
        return self.num_items if type(self.score_func) in (InnerProductScorer, CosineScorer, EuclideanScorer) else None


class SGL(LightGCN):
    """recstudio/model/graph/sgl.py:34-114, recstudio/model/graph/config/sgl.yaml (aug_type 'ED', n_layers 3, l2_reg_weight 1e-4,
    ssl_ratio 0.1, ssl_reg 0.1, temperature 0.2, negative_count 1, batch_size 2048): LightGCN's step plus ``ssl_reg`` times the
    InfoNCE contrast (users and items) between two randomly thinned views of the graph, drawn afresh every step
    (``data_augmentation.SGLAugmentation`` on ``rsa_graph_dropout``).  ``last_views`` holds the last step's two views (their
    masks and degrees; ``ssl_reg: 0`` draws none and is LightGCN's step).  Evaluation propagates over the full graph and is
    LightGCN's.

    Two deliberate deviations from the reference.  (1) sgl.py:101-103 ends a line with a stray comma, so ``training_step``
    returns a tuple and ``Recommender.training_epoch`` (recommender.py:615-639) runs no backward at all; here the loss is the sum
    those three lines plainly intend.  (2) Which edges fall is defined by the device ``torch.rand`` stream in CSR edge order, not
    by ``dgl.DropEdge``'s stream, which cannot be reproduced without dgl; the distribution is the same."""

    def __init__(self, config=None, **kwargs):
        super().__init__(config, **kwargs)
        for key, value in (('aug_type', 'ED'), ('ssl_ratio', 0.1), ('ssl_reg', 0.1), ('temperature', 0.2)):
            self.config['model'].setdefault(key, value)
        if 'batch_size' not in (config or {}).get('train', {}):
            self.config['train']['batch_size'] = 2048

    def _init_model(self, train_data, drop_unused_field=True):
        from . import data_augmentation
        super()._init_model(train_data, drop_unused_field)
        self.augmentaion_model = data_augmentation.SGLAugmentation(self.config['model'], train_data)

    @property
    def last_views(self):
        return self.augmentaion_model.last_views

    def training_step(self, batch):
        loss = super().training_step(batch)
        if not self.config['model']['ssl_reg']:
            return loss
        cl_output = self.augmentaion_model(batch, self.user_emb, self.item_emb, self.adj_mat, self.LightGCNNet)
        return loss + self.config['model']['ssl_reg'] * cl_output['cl_loss']


class SimGCL(LightGCN):
    """recstudio/model/graph/simgcl.py:35-110, recstudio/model/graph/config/simgcl.yaml (eps 0.1, n_layers 3, l2_reg_weight 1e-4,
    cl_neg_type 'all', temperature 0.2, batch_size 2048, learning_rate 0.001, negative_count 1): LightGCN's step -- BPR on
    uniform negatives plus the l2 regulariser of the base rows -- over ``graphmodule.SimGCLNet``, whose layer mean SKIPS the
    input (mean(E_1 .. E_L), which ``evaluate`` / ``topk`` use as well), plus the InfoNCE contrast between two noise-perturbed
    propagations of the same graph (``data_augmentation.SimGCLAugmentation``; the noise is added inside ``rsa_spmm_csr``).  The
    device stream of a step: the negatives first, then the L ``rand_like`` calls of view 1, then those of view 2.

    ``model.cl_weight`` (0.5 in simgcl.yaml) is accepted and NOT applied: nothing in the reference reads it, simgcl.py:98 adds
    ``cl_loss`` with weight 1, and so does this class."""

    def __init__(self, config=None, **kwargs):
        super().__init__(config, **kwargs)
        for key, value in (('eps', 0.1), ('cl_weight', 0.5), ('cl_neg_type', 'all'), ('temperature', 0.2)):
            self.config['model'].setdefault(key, value)
        given = (config or {}).get('train', {})
        for key, value in (('batch_size', 2048), ('learning_rate', 0.001)):
            if key not in given:
                self.config['train'][key] = value

    def _init_model(self, train_data, drop_unused_field=True):
        from . import data_augmentation
        super()._init_model(train_data, drop_unused_field)
        self.augmentation_model = data_augmentation.SimGCLAugmentation(self.config['model'], train_data)

    def _get_gnn_net(self):
        from . import graphmodule
        return graphmodule.SimGCLNet(self.config['model']['n_layers'], self.config['model']['eps'])

    def _propagate(self, embeddings):
        return self.SimGCLNet.propagate(self.adj_mat, embeddings)

    def training_step(self, batch):
        loss = super().training_step(batch)                    # the negatives are drawn here, before the noise
        cl_output = self.augmentation_model(batch, self.user_emb, self.item_emb, self.adj_mat, self.SimGCLNet)
        return loss + cl_output['cl_loss']


class NGCF(LightGCN):
    """recstudio/model/graph/ngcf.py:14-96, recstudio/model/graph/config/ngcf.yaml (layer_size [64, 64, 64, 64], mess_dropout
    [0.1, 0.1, 0.1], node_dropout 0.1 -- ``None`` switches it off --, l2_reg_weight 1e-5, batch_size 2048, learning_rate 1e-4,
    negative_count 1).  The base tables are propagated by ``graphmodule.NGCFNet``: per layer one ``rsa_spmm_csr`` over the
    left-normalised graph (``graphmodule.LeftAdj``) and one fused ``BiCombiner`` (``rsa_bi_combine``); the result is
    ``cat(x_0, normalize(h_1), ..., normalize(h_L))``, sum(layer_size) wide (at most 256, the widest table the fused BPR tail and
    the MFMA top-k take), and everything behind it -- the fused forward, ``training_step`` (BPR plus the l2 regulariser of the BASE
    rows), ``evaluate`` / ``topk`` -- is LightGCN's.  ``embed_dim`` must equal ``layer_size[0]``.  Evaluation propagates over
    the full graph without any dropout.

    The device generator of a training step is consumed in this order: the edge mask (``torch.rand(nnz)``, with ``node_dropout``),
    then the L message-dropout calls in layer order (``torch.rand(n_nodes, layer_size[k])``), then the negatives.

    Two deliberate deviations from the reference, both in WHICH elements fall, neither in how many.  (1) ``node_dropout`` is an
    edge dropout in the reference too (``EdgeDropout`` -> ``dgl.DropEdge``); here the kept edges are defined by the device
    ``torch.rand`` stream in CSR edge order (``rsa_graph_dropout``), as for SGL.  (2) The message dropout keeps element (r, c)
    iff ``torch.rand_like(h)[r, c] < fp32(1 - p)`` and divides by that; ``nn.Dropout``'s kernel walks the same Philox stream in
    another layout (``graphmodule.BiCombiner``)."""

    MAX_WIDTH = 256

    def __init__(self, config=None, **kwargs):
        super().__init__(config, **kwargs)
        model, given = self.config['model'], config or {}
        for key, value in (('layer_size', [64, 64, 64, 64]), ('node_dropout', 0.1)):
            model.setdefault(key, value)
        model['n_layers'] = len(model['layer_size']) - 1
        model.setdefault('mess_dropout', [0.1] * (len(model['layer_size']) - 1))
        if 'l2_reg_weight' not in given.get('model', {}):
            model['l2_reg_weight'] = 1e-5
        for key, value in (('batch_size', 2048), ('learning_rate', 1e-4)):
            if key not in given.get('train', {}):
                self.config['train'][key] = value
        layers = [int(v) for v in model['layer_size']]
        if len(layers) < 2 or len(model['mess_dropout']) != len(layers) - 1:
            raise ValueError(f'NGCF: layer_size {layers} needs at least one layer and one mess_dropout per layer, got '
                             f'{model["mess_dropout"]}')
        if self.embed_dim != layers[0]:
            raise ValueError(f'NGCF: embed_dim ({self.embed_dim}) must equal layer_size[0] ({layers[0]})')
        if sum(layers) > self.MAX_WIDTH:
            raise ValueError(f'NGCF: the concatenated table is sum(layer_size) = {sum(layers)} wide; the fused BPR tail and the '
                             f'top-k kernels take tables of at most {self.MAX_WIDTH} columns')
        drop = model['node_dropout']
        if drop is not None and not 0.0 <= float(drop) < 1.0:
            raise ValueError(f'NGCF: node_dropout must be None or lie in [0, 1), got {drop}')

    def _init_model(self, train_data, drop_unused_field=True):
        from . import graphmodule
        super()._init_model(train_data, drop_unused_field)
        self.left_adj = graphmodule.LeftAdj(self.adj_mat)
        self.last_view = None

    def _get_gnn_net(self):
        from . import graphmodule
        model = self.config['model']
        layers = [int(v) for v in model['layer_size']]
        self.combiners = torch.nn.ModuleList(graphmodule.BiCombiner(a, b, dropout=float(p))
                                             for a, b, p in zip(layers[:-1], layers[1:], model['mess_dropout']))
        return graphmodule.NGCFNet(self.combiners, len(layers) - 1)

    def _propagate(self, embeddings):
        from . import graphmodule
        drop = self.config['model']['node_dropout']
        adj = self.left_adj
        if self.training and drop:
            self.adj_mat.to(embeddings.device)
            adj = self.last_view = graphmodule.LeftAdj.thinned(self.adj_mat, 1.0 - float(drop))
        return self.NGCFNet.propagate(adj, embeddings)


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


class _above_second_stream:
    """``with`` block whose work runs on a HIGH-priority stream (entered after, left before, the stream that was current):
    the look-ahead's second stream then sits below the steps it runs under and fills their gaps instead of competing with
    them (sharded training step one batch ahead, in process: 1.166 ms with both at the default priority, 1.136 ms so)."""

    def __init__(self, on, device, cache):
        self.on, self.device, self.cache = bool(on), device, cache

    def __enter__(self):
        if self.on:
            self.prev = torch.cuda.current_stream(self.device)
            hi = self.cache.get('hi_stream')
            if hi is None:
                hi = self.cache['hi_stream'] = torch.cuda.Stream(device=self.device, priority=-1)
            hi.wait_stream(self.prev)
            torch.cuda.set_stream(hi)
            self.hi = hi
        return self

    def __exit__(self, *exc):
        if self.on:
            self.prev.wait_stream(self.hi)
            torch.cuda.set_stream(self.prev)
        return False


def _with_next(it):
    """(x0, x1), (x1, x2), ..., (x_last, None)"""
    it = iter(it)
    cur = next(it, None)
    while cur is not None:
        nxt = next(it, None)
        yield cur, nxt
        cur = nxt


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


class SASRecQueryEncoder(torch.nn.Module):
    """recstudio/model/seq/sasrec.py:8-67: item-embedding gather of the history (HIP) + learned positions
    + nn.TransformerEncoder (causal unless ``bidirectional``) + last-position pooling.  The encoder is stock PyTorch-ROCm by
    default; with ``fused_attention`` its layers run through ``seqmodule.FusedTransformerEncoder`` (the attention core as one
    HIP kernel) over the same parameters: ``state_dict`` is the same either way.

    ``need_pooling=False`` returns the tower's ``[B, L, D]`` (what CL4SRec's views are mean-pooled from).  With ``mask_id`` (CL4SRec:
    ``num_items``) the encoder owns ``mask_emb`` [1, D], the row of the mask token: the ids
    equal to ``mask_id`` are gathered as row 0 (the zero padding row) through the same gather node and ``mask_emb`` is added at those
    positions, while ``key_pad`` stays ``ids == 0`` on the ORIGINAL ids, so masked positions are attended.  The catalog table keeps
    its ``num_items`` rows (the reference widens it by one, cl4srec.py:33-34): ``mask_id`` never reaches the gather, the sampler or
    ``topk``."""

    def __init__(self, fiid, embed_dim, max_seq_len, n_head, hidden_size, dropout, activation, layer_norm_eps, n_layer,
                 item_encoder, bidirectional=False, fused_attention=False, mask_id=None):
        super().__init__()
        self.fiid = fiid
        self.mask_id = mask_id
        if mask_id is not None:
            self.mask_emb = torch.nn.Parameter(torch.zeros(1, embed_dim))
        self.item_encoder = item_encoder
        self.bidirectional = bool(bidirectional)
        self.fused_attention = bool(fused_attention)
        self.position_emb = torch.nn.Embedding(max_seq_len, embed_dim)
        layer = torch.nn.TransformerEncoderLayer(d_model=embed_dim, nhead=n_head, dim_feedforward=hidden_size,
                                                 dropout=dropout, activation=activation, layer_norm_eps=layer_norm_eps,
                                                 batch_first=True, norm_first=False)
        self.transformer_layer = torch.nn.TransformerEncoder(layer, num_layers=n_layer)
        self.dropout = torch.nn.Dropout(p=dropout)
        # (no parameters of its own: it reads transformer_layer's at call time)
        self._fused = FusedTransformerEncoder(self.transformer_layer, max_seq_len) if self.fused_attention else None

    def forward(self, batch, need_pooling=True):
        user_hist = batch['in_' + self.fiid]
        B, L = user_hist.shape
        positions = torch.arange(L, dtype=torch.long, device=user_hist.device).unsqueeze(0).expand(B, L)
        seg = batch.get('_seg')
        masked = None
        ids = user_hist
        if self.mask_id is not None and seg is None:
            # any ids handed over as a tensor (a view of CL4SRec): the mask token is no catalog row.  (The CSR view of the loader
            # gathers from the dataset's own item column, which holds no mask token.)
            masked = user_hist == self.mask_id
            ids = torch.where(masked, torch.zeros_like(user_hist), user_hist)
        if not isinstance(self.item_encoder, torch.nn.Embedding):
            # the row-sharded catalog (shard.ShardedRows put here by BaseRetriever._setup_shard): ids out, rows back
            rows = self.item_encoder(ids)
        elif not user_hist.is_cuda and (self._fused is not None or self.mask_id is not None):
            # the torch-op twin of the fused tower (seqmodule.seq_attention_torch) on CPU tensors: parity checks without a device
            rows = self.item_encoder(ids)
        elif seg is not None and user_hist.is_cuda:
            # the device loader handed over the CSR view (flat item column, start, end): the fused segment gather emits
            # [B, L, d] directly; ``in_item_id`` only serves the padding mask and the backward
            flat, start, end = seg
            rows = _SegEmbedFn.apply(self.item_encoder.weight, flat, start, end, L, user_hist)
        else:
            rows = _EmbedFn.apply(self.item_encoder.weight, ids)
        if masked is not None:
            rows = rows + masked.unsqueeze(-1).to(rows.dtype) * self.mask_emb
        seq = rows + self.position_emb(positions)
        if self._fused is not None:
            out = self._fused(self.dropout(seq), key_pad=user_hist == 0, causal=not self.bidirectional)
        else:
            if self.bidirectional:
                mask = torch.zeros(L, L, dtype=torch.bool, device=user_hist.device)
            else:
                mask = torch.triu(torch.ones(L, L, dtype=torch.bool, device=user_hist.device), 1)
            out = self.transformer_layer(self.dropout(seq), mask=mask, src_key_padding_mask=user_hist == 0)
        if not need_pooling:
            return out
        last = (batch['seqlen'] - 1).clamp(min=0).view(-1, 1, 1).expand(-1, 1, out.shape[-1])
        return out.gather(1, last).squeeze(1)


class SASRec(BaseRetriever):
    """recstudio/model/seq/sasrec.py:70-123 with the retriever tail on the fused path."""

    def __init__(self, config=None, **kwargs):
        # recstudio/model/seq/config/sasrec.yaml on top of basemodel.yaml; the caller's config wins
        user = config or {}
        super().__init__(config, **kwargs)
        m = self.config['model']
        for k, v in (('hidden_size', 128), ('layer_num', 2), ('head_num', 2), ('dropout_rate', 0.5),
                     ('activation', 'gelu'), ('layer_norm_eps', 1e-12), ('fused_attention', False)):
            m.setdefault(k, v)
        for k, v in (('negative_count', 1), ('init_method', 'normal')):
            if k not in user.get('train', {}):
                self.config['train'][k] = v

    def _get_dataset_class():
        return SeqDataset

    def _get_query_encoder(self, train_data):
        m = self.config['model']
        return SASRecQueryEncoder(self.fiid, self.embed_dim, train_data.config['max_seq_len'], m['head_num'],
                                  m['hidden_size'], m['dropout_rate'], m['activation'], m['layer_norm_eps'],
                                  m['layer_num'], self.item_encoder, fused_attention=m['fused_attention'])

    def _get_query_feat(self, data):
        return data if isinstance(data, dict) else super()._get_query_feat(data)

    def _get_loss_func(self):
        return BinaryCrossEntropyLoss()         # sasrec.py:117-119

    def _get_sampler(self, train_data):
        return UniformSampler(train_data.num_items)


class CL4SRec(SASRec):
    """recstudio/model/seq/cl4srec.py:13-53, recstudio/model/seq/config/cl4srec.yaml (hidden_size 64, layer_num 1, temperature 1.0,
    augment_type 'item_crop', tau 0.2, cl_weight 0.1) on top of SASRec's: SASRec's step plus ``cl_weight`` times the in-batch InfoNCE
    between two augmented views of every history, drawn afresh every step (``data_augmentation.CL4SRecAugmentation``).  The tower
    runs three times per step: the main pass and one pass per view.  ``last_views`` holds the last step's two views.

    A view is ONE launch of ``rsa_seq_augment`` with ``model.fused_augment`` (default on: faster than the twin at every measured shape), the same rule in batched torch ops
    (``seq_augment_torch``) without it, on CPU tensors or above 64 positions -- the same view either way.  The in-batch InfoNCE is
    ``rsa_batch_infonce`` / ``rsa_batch_infonce_backward`` with ``model.fused_infonce`` (nothing of size B^2, forward or backward;
    off by default: slower than the op sequence at B = 8192, see ``FUSED_INFONCE_DEFAULT``), the reference's op sequence
    (``batch_infonce_torch``, which holds [B, 2B]) without it, on CPU tensors or at other widths.

    THE GENERATOR ORDER OF A STEP (device stream): the main pass (the tower's dropouts, then the negatives), ``rand([B, L + 1])`` for
    view i, the same for view j, the tower's dropouts for view i, then those for view j.  ``item_random`` also takes one
    ``random.randint(0, 2)`` per view from Python's generator.

    Deliberate deviations from the reference.  (1) The views follow the device ``torch.rand`` stream, not the reference's three host
    generators behind one ``.item()`` per sequence (2 B synchronisations per step).  (2) A cropped batch keeps its width L
    (``pad_sequence`` narrows it); the encoder's output on the kept positions is the same.  (3) The mask token is not row
    ``num_items`` of a widened item table (cl4srec.py:33-34, which the reference's evaluation then scores like an item) but the
    query encoder's own ``mask_emb`` [1, d]: the catalog table keeps ``num_items`` rows, so the sampler, the fused tail, ``topk``
    and ``evaluate`` run unchanged and never see ``num_items``; a reference checkpoint's trailing row is ``mask_emb``.  (4) The
    training form is this tree's SASRec's (``SeqDataset``, last-position pooling, BCE with one negative); the reference's uses
    ``SeqToSeqDataset`` with a loss at every position."""

    def __init__(self, config=None, **kwargs):
        user = (config or {}).get('model', {})
        super().__init__(config, **kwargs)
        m = self.config['model']
        for k, v in (('hidden_size', 64), ('layer_num', 1)):
            if k not in user:
                m[k] = v
        for k, v in (('temperature', 1.0), ('augment_type', 'item_crop'), ('tau', 0.2), ('cl_weight', 0.1), ('fused_augment', True),
                     ('fused_infonce', FUSED_INFONCE_DEFAULT)):
            m.setdefault(k, v)

    def _init_model(self, train_data, drop_unused_field=True):
        from . import data_augmentation
        super()._init_model(train_data, drop_unused_field)
        self.augmentation_model = data_augmentation.CL4SRecAugmentation(self.config['model'], train_data)

    def _get_query_encoder(self, train_data):
        m = self.config['model']
        return SASRecQueryEncoder(self.fiid, self.embed_dim, train_data.config['max_seq_len'], m['head_num'],
                                  m['hidden_size'], m['dropout_rate'], m['activation'], m['layer_norm_eps'],
                                  m['layer_num'], self.item_encoder, fused_attention=m['fused_attention'],
                                  mask_id=train_data.num_items)

    def _init_parameter(self):
        super()._init_parameter()
        # the mask token like a row of the item table (recstudio/model/init.py on the reference's [num_items + 1, d] table); drawn
        # last, so every other parameter is SASRec's at the same seed
        w = self.query_encoder.mask_emb.data
        method, (n, d) = self.config['train']['init_method'], self.item_encoder.weight.shape
        if method == 'xavier_normal':
            w.normal_(mean=0.0, std=math.sqrt(2.0 / (n + 1 + d)))
        elif method == 'xavier_uniform':
            bound = math.sqrt(6.0 / (n + 1 + d))
            w.uniform_(-bound, bound)
        else:
            w.normal_(mean=0.0, std=0.02)

    @property
    def last_views(self):
        return self.augmentation_model.last_views

    def training_step(self, batch):
        loss = super().training_step(batch)
        if not self.config['model']['cl_weight']:
            return loss
        cl_output = self.augmentation_model(batch, self.query_encoder)
        return loss + self.config['model']['cl_weight'] * cl_output['cl_loss']


class GRU4RecQueryEncoder(torch.nn.Module):
    """recstudio/model/seq/gru4rec.py:36-53: item-embedding gather of the history (HIP) + nn.Dropout + module.GRULayer (an
    ``nn.GRU`` with ``bias=False``, ``batch_first=True``) + last-position pooling + nn.Linear(hidden_size, embed_dim).  With
    ``fused_gru`` the GRU runs through ``seqmodule.FusedGRU`` (the recurrence as one HIP kernel, stopped at ``seqlen``) over the
    same parameters: ``state_dict`` is the same either way.  In train mode the device generator is consumed once per call, by
    the ``nn.Dropout`` on the gathered rows."""

    def __init__(self, fiid, embed_dim, hidden_size, dropout, n_layer, item_encoder, fused_gru=True):
        super().__init__()
        self.fiid = fiid
        self.item_encoder = item_encoder
        self.fused_gru = bool(fused_gru)
        self.dropout = torch.nn.Dropout(p=dropout)
        self.gru = torch.nn.GRU(input_size=embed_dim, hidden_size=hidden_size, num_layers=n_layer, bias=False, batch_first=True,
                                bidirectional=False)
        self.dense = torch.nn.Linear(hidden_size, embed_dim)
        # (no parameters of its own: it reads gru's at call time)
        self._fused = FusedGRU(self.gru) if self.fused_gru else None

    def forward(self, batch):
        user_hist = batch['in_' + self.fiid]
        L = user_hist.shape[1]
        seg = batch.get('_seg')
        if not isinstance(self.item_encoder, torch.nn.Embedding) or not user_hist.is_cuda:
            # the row-sharded catalog (shard.ShardedRows put here by BaseRetriever._setup_shard): ids out, rows back; or CPU
            # tensors (the torch-op twin of the fused recurrence: parity checks without a device)
            rows = self.item_encoder(user_hist)
        elif seg is not None:
            flat, start, end = seg
            rows = _SegEmbedFn.apply(self.item_encoder.weight, flat, start, end, L, user_hist)
        else:
            rows = _EmbedFn.apply(self.item_encoder.weight, user_hist)
        seqlen = batch['seqlen']
        if self._fused is not None:
            out, _ = self._fused(self.dropout(rows), lengths=seqlen, want_state=False)
        else:
            out, _ = self.gru(self.dropout(rows))
        last = (seqlen - 1).clamp(min=0).view(-1, 1, 1).expand(-1, 1, out.shape[-1])
        return self.dense(out.gather(1, last).squeeze(1))


class GRU4Rec(BaseRetriever):
    """recstudio/model/seq/gru4rec.py:17-63 with the retriever tail on the fused BPR path."""

    def __init__(self, config=None, **kwargs):
        # recstudio/model/seq/config/gru4rec.yaml on top of basemodel.yaml; the caller's config wins
        user = config or {}
        super().__init__(config, **kwargs)
        m = self.config['model']
        for k, v in (('hidden_size', 128), ('dropout_rate', 0.3), ('layer_num', 1), ('fused_gru', True)):
            m.setdefault(k, v)
        if 'negative_count' not in user.get('train', {}):
            self.config['train']['negative_count'] = 1

    def _get_dataset_class():
        return SeqDataset

    def _get_query_encoder(self, train_data):
        m = self.config['model']
        return GRU4RecQueryEncoder(self.fiid, self.embed_dim, m['hidden_size'], m['dropout_rate'], m['layer_num'],
                                   self.item_encoder, fused_gru=m['fused_gru'])

    def _get_query_feat(self, data):
        return data if isinstance(data, dict) else super()._get_query_feat(data)

    def _get_score_func(self):
        return InnerProductScorer()

    def _get_loss_func(self):
        return BPRLoss()

    def _get_sampler(self, train_data):
        return UniformSampler(train_data.num_items)


def _history_rows(item_encoder, batch, fiid):
    """``item_encoder(in_item_id)`` [B, L, d] of a sequence tower: the HIP gather (from the device loader's CSR view when the
    batch carries one) for an ``nn.Embedding`` on device tensors, the module itself otherwise (a sharded catalog; CPU tensors)."""
    user_hist = batch['in_' + fiid]
    seg = batch.get('_seg')
    if not isinstance(item_encoder, torch.nn.Embedding) or not user_hist.is_cuda:
        return item_encoder(user_hist)
    if seg is not None:
        flat, start, end = seg
        return _SegEmbedFn.apply(item_encoder.weight, flat, start, end, user_hist.shape[1], user_hist)
    return _EmbedFn.apply(item_encoder.weight, user_hist)


def _last_position(out, seqlen):
    """SeqPoolingLayer(pooling_type='last'): ``out[b, seqlen[b] - 1]``."""
    last = (seqlen - 1).clamp(min=0).view(-1, 1, 1).expand(-1, 1, out.shape[-1])
    return out.gather(1, last).squeeze(1)


class NARMQueryEncoder(torch.nn.Module):
    """recstudio/model/seq/narm.py:15-47: item-embedding gather of the history (HIP) + nn.Dropout + module.GRULayer (an ``nn.GRU``
    with ``bias=False``) -> ``c_global`` = the state at the last position; ``c_local`` = ``AttentionLayer(q_dim=hidden_size,
    mlp_layers=[hidden_size], bias=False)`` of that state over every GRU state (``seqmodule.AttentionLayer``: the pooling as one
    HIP kernel with ``fused_attention_pool``); ``fc`` = nn.Dropout + nn.Linear(2 hidden_size, embed_dim, bias=False) of their
    concatenation.  The GRU sits under ``gru_layer.2.gru`` as in the reference; with ``fused_gru`` it runs through
    ``seqmodule.FusedGRU``.  ``state_dict`` is the same whichever flags are set.
    In train mode the device generator is consumed TWICE per call, in this order: the ``nn.Dropout`` on the gathered rows
    (``gru_layer.1``), then the ``nn.Dropout`` on ``cat(c_global, c_local)`` (``fc.0``).
    The fused GRU writes zeros at ``t >= seqlen`` where ``nn.GRU`` runs on; the padding mask gives those positions weight 0 and
    gradient 0 either way, so the query is the same."""

    def __init__(self, fiid, embed_dim, hidden_size, layer_num, dropout_rate, item_encoder=None, fused_gru=True,
                 fused_attention_pool=True):
        super().__init__()
        self.fiid = fiid
        self.item_encoder = item_encoder
        self.fused_gru = bool(fused_gru)
        gru_layer = torch.nn.Module()
        gru_layer.gru = torch.nn.GRU(input_size=embed_dim, hidden_size=hidden_size, num_layers=layer_num, bias=False,
                                     batch_first=True, bidirectional=False)
        # (the reference's Sequential(item_encoder, Dropout, GRULayer): the item encoder is registered once, above)
        self.gru_layer = torch.nn.ModuleDict({'1': torch.nn.Dropout(dropout_rate[0]), '2': gru_layer})
        self.attn_layer = AttentionLayer(q_dim=hidden_size, mlp_layers=[hidden_size], bias=False)
        self.attn_layer.fused = bool(fused_attention_pool)
        self.fc = torch.nn.Sequential(torch.nn.Dropout(dropout_rate[1]), torch.nn.Linear(hidden_size * 2, embed_dim, bias=False))
        self._fused = FusedGRU(gru_layer.gru) if self.fused_gru else None

    def forward(self, batch):
        user_hist = batch['in_' + self.fiid]
        rows = self.gru_layer['1'](_history_rows(self.item_encoder, batch, self.fiid))
        seqlen = batch['seqlen']
        if self._fused is not None:
            gru_vec, _ = self._fused(rows, lengths=seqlen, want_state=False)
        else:
            gru_vec, _ = self.gru_layer['2'].gru(rows)
        c_global = h_t = _last_position(gru_vec, seqlen)                                           # B x H
        c_local = self.attn_layer(query=h_t.unsqueeze(1), key=gru_vec, value=gru_vec, key_padding_mask=user_hist == 0,
                                  need_weight=False).squeeze(1)                                    # B x H
        return self.fc(torch.cat((c_global, c_local), dim=1))                                      # B x D


class _SeqSoftmaxRetriever(BaseRetriever):
    """What NARM and STAMP share: SeqDataset, InnerProductScorer, SoftmaxLoss and no sampler -- ``training_step`` takes the
    'full_softmax' path, which never holds [B, N]."""

    def _get_dataset_class():
        return SeqDataset

    def _get_query_feat(self, data):
        return data if isinstance(data, dict) else super()._get_query_feat(data)

    def _get_score_func(self):
        return InnerProductScorer()

    def _get_loss_func(self):
        return SoftmaxLoss()

    def _get_sampler(self, train_data):
        return None


class NARM(_SeqSoftmaxRetriever):
    """recstudio/model/seq/narm.py:50-88 with the retriever tail on the fused full-softmax path."""

    def __init__(self, config=None, **kwargs):
        # recstudio/model/seq/config/narm.yaml on top of basemodel.yaml; the caller's config wins
        super().__init__(config, **kwargs)
        m = self.config['model']
        for k, v in (('hidden_size', 128), ('dropout_rate', [0.25, 0.5]), ('layer_num', 1), ('fused_gru', True),
                     ('fused_attention_pool', FUSED_ATTENTION_POOL_DEFAULT)):
            m.setdefault(k, v)

    def _get_dataset_class():
        return SeqDataset

    def _get_query_encoder(self, train_data):
        m = self.config['model']
        return NARMQueryEncoder(self.fiid, self.embed_dim, m['hidden_size'], m['layer_num'], m['dropout_rate'], self.item_encoder,
                                fused_gru=m['fused_gru'], fused_attention_pool=m['fused_attention_pool'])


class STAMPQueryEncoder(torch.nn.Module):
    """recstudio/model/seq/stamp.py:6-32: ``m_t`` = the last item's embedding, ``m_s`` = the mean of the history's, ``m_a`` =
    ``AttentionLayer(q_dim=2 embed_dim, k_dim=embed_dim, mlp_layers=[embed_dim])`` of ``cat(m_t, m_s)`` over the history rows
    (``seqmodule.AttentionLayer``: one HIP kernel with ``fused_attention_pool``), query = ``mlpA(m_a) * mlpB(m_t)`` (two
    ``MLPModule([embed_dim, embed_dim], Tanh)``).  No dropout is active: the generator is not consumed."""

    def __init__(self, fiid, embed_dim, item_encoder, fused_attention_pool=True):
        super().__init__()
        self.fiid = fiid
        self.item_encoder = item_encoder
        self.attention_layer = AttentionLayer(q_dim=2 * embed_dim, k_dim=embed_dim, mlp_layers=[embed_dim])
        self.attention_layer.fused = bool(fused_attention_pool)
        self.mlpA = MLPModule([embed_dim, embed_dim], torch.nn.Tanh())
        self.mlpB = MLPModule([embed_dim, embed_dim], torch.nn.Tanh())

    def forward(self, batch):
        user_hist = batch['in_' + self.fiid]
        seq_emb = _history_rows(self.item_encoder, batch, self.fiid)
        m_t = _last_position(seq_emb, batch['seqlen'])
        m_s = seq_emb.sum(dim=1) / batch['seqlen'].unsqueeze(1).float()                            # B x D
        query = torch.cat((m_t, m_s), dim=1)                                                       # B x 2D
        m_a = self.attention_layer(query.unsqueeze(1), seq_emb, seq_emb, key_padding_mask=(user_hist == 0)).squeeze(1)
        return self.mlpA(m_a) * self.mlpB(m_t)


class STAMP(_SeqSoftmaxRetriever):
    """recstudio/model/seq/stamp.py:35-61 with the retriever tail on the fused full-softmax path."""

    def __init__(self, config=None, **kwargs):
        # recstudio/model/seq/config/stamp.yaml (embed_dim 64) on top of basemodel.yaml; the caller's config wins
        super().__init__(config, **kwargs)
        self.config['model'].setdefault('fused_attention_pool', FUSED_ATTENTION_POOL_DEFAULT)

    def _get_dataset_class():
        return SeqDataset

    def _get_query_encoder(self, train_data):
        return STAMPQueryEncoder(self.fiid, self.embed_dim, self.item_encoder,
                                 fused_attention_pool=self.config['model']['fused_attention_pool'])


class CaserQueryEncoder(torch.nn.Module):
    """recstudio/model/seq/caser.py:16-56, same constructor arguments, same submodules (``user_embedding``, ``item_embedding`` --
    the tower's OWN [num_items, embed_dim] table, not the item encoder --, ``vertical_filter``, ``horizontal_filter.{i}``, ``fc``)
    and so the same ``state_dict``.  The history ids are padded to ``max_seq_len`` (:39) and gathered through ``_history_rows``;
    everything between that gather and the dropout in front of ``fc`` is ``seqmodule.caser_conv_torch``, the reference's op
    sequence over the ``Conv2d`` modules' own parameters; then ``nn.Dropout``, ``relu(fc(.))`` and ``cat((z, P_u))``: a query of
    width 2 embed_dim.  In train mode the generator is consumed ONCE per call, by that ``nn.Dropout`` on ``o`` [B, n_v d + L n_h].
    The tower only: no retriever is built on it while its convolutions have no kernel."""

    def __init__(self, fiid, fuid, num_users, num_items, embed_dim, max_seq_len, n_v, n_h, dropout=0.2) -> None:
        super().__init__()
        self.fiid = fiid
        self.fuid = fuid
        self.max_seq_len = max_seq_len
        self.user_embedding = torch.nn.Embedding(num_users, embed_dim, 0)
        self.item_embedding = torch.nn.Embedding(num_items, embed_dim, 0)
        self.dropout = torch.nn.Dropout(p=dropout)
        self.vertical_filter = torch.nn.Conv2d(in_channels=1, out_channels=n_v, kernel_size=(self.max_seq_len, 1))
        self.horizontal_filter = torch.nn.ModuleList([
            torch.nn.Conv2d(in_channels=1, out_channels=n_h, kernel_size=(h, embed_dim)) for h in range(1, max_seq_len + 1)])
        self.fc = torch.nn.Linear(n_v * embed_dim + n_h * max_seq_len, embed_dim, bias=True)

    def conv_features(self, batch):
        """``o`` [B, n_v d + L n_h]: what goes into the dropout."""
        item_seq = batch['in_' + self.fiid]
        if item_seq.size(1) < self.max_seq_len:
            item_seq = torch.nn.functional.pad(item_seq, (0, self.max_seq_len - item_seq.size(1)))      # caser.py:39
            batch = {k: v for k, v in batch.items() if k != '_seg'}
            batch['in_' + self.fiid] = item_seq
        rows = _history_rows(self.item_embedding, batch, self.fiid)
        return caser_conv_torch(rows, *caser_pack(self.vertical_filter, self.horizontal_filter))

    def forward(self, batch):
        P_u = self.user_embedding(batch[self.fuid])
        o = self.dropout(self.conv_features(batch))
        z = torch.relu(self.fc(o))
        return torch.cat((z, P_u), dim=1)


class HGNQueryEncoder(torch.nn.Module):
    """recstudio/model/seq/hgn.py:16-44, same constructor arguments, same submodules (``user_embedding``, ``W_g_1``, ``W_g_2``,
    ``b_g``, ``w_g_3``, ``W_g_4`` and the shared ``item_encoder``) and so the same ``state_dict``.  The history rows are gathered
    through ``_history_rows``; ``ug = W_g_2(U) + b_g`` and ``ui = U @ W_g_4.weight[:L].T`` are torch GEMMs; everything per position
    -- the feature gate, the instance gate, the pooling and ``S.sum(1)`` -- is ONE launch of ``seqmodule.hgn_gating`` with
    ``fused_gating`` (a plain attribute, not a parameter), the reference's op sequence ``hgn_gating_torch`` without it or on CPU
    tensors.  Two facts of the reference: ``b_g`` is ``torch.empty`` there and no initialiser touches a bare ``Parameter``, so it
    trains from uninitialised memory -- here it starts at ZERO; ``W_g_4.bias`` exists, is saved and loaded, and
    never receives a gradient.  No dropout: the generator is not consumed."""

    def __init__(self, fuid, fiid, num_users, embed_dim, max_seq_len, item_encoder, pooling_type='mean', fused_gating=True) -> None:
        super().__init__()
        self.fuid = fuid
        self.fiid = fiid
        self.item_encoder = item_encoder
        self.pooling_type = pooling_type
        self.fused_gating = bool(fused_gating)
        self.user_embedding = torch.nn.Embedding(num_users, embed_dim, 0)
        self.W_g_1 = torch.nn.Linear(embed_dim, embed_dim, bias=False)
        self.W_g_2 = torch.nn.Linear(embed_dim, embed_dim, bias=False)
        self.b_g = torch.nn.Parameter(torch.zeros(embed_dim), requires_grad=True)
        self.w_g_3 = torch.nn.Linear(embed_dim, 1, bias=False)
        self.W_g_4 = torch.nn.Linear(embed_dim, max_seq_len)

    def forward(self, batch):
        if self.pooling_type not in ('mean', 'max'):
            raise ValueError("`pooling_type` only support `avg` and `max`")                           # hgn.py:42
        U = self.user_embedding(batch[self.fuid])                                                     # B x D
        S = _history_rows(self.item_encoder, batch, self.fiid)                                        # B x L x D
        ug = self.W_g_2(U) + self.b_g
        ui = U @ self.W_g_4.weight[:S.size(1)].T                                                      # B x L
        gate = hgn_gating if self.fused_gating else hgn_gating_torch
        return U + gate(S, ug, ui, self.W_g_1.weight, self.w_g_3.weight.view(-1), self.pooling_type)


class HGN(BaseRetriever):
    """recstudio/model/seq/hgn.py:47-68 with the retriever tail on the fused BPR path."""

    def __init__(self, config=None, **kwargs):
        # recstudio/model/seq/config/hgn.yaml on top of basemodel.yaml; the caller's config wins
        user = config or {}
        super().__init__(config, **kwargs)
        m = self.config['model']
        for k, v in (('pooling_type', 'mean'), ('fused_gating', FUSED_GATING_DEFAULT)):
            m.setdefault(k, v)
        if 'negative_count' not in user.get('train', {}):
            self.config['train']['negative_count'] = 1

    def _get_dataset_class():
        return SeqDataset

    def _get_query_encoder(self, train_data):
        m = self.config['model']
        return HGNQueryEncoder(self.fuid, self.fiid, train_data.num_users, self.embed_dim, train_data.config['max_seq_len'],
                               self.item_encoder, m['pooling_type'], fused_gating=m['fused_gating'])

    def _get_query_feat(self, data):
        return data if isinstance(data, dict) else super()._get_query_feat(data)

    def _get_score_func(self):
        return InnerProductScorer()

    def _get_loss_func(self):
        return BPRLoss()

    def _get_sampler(self, train_data):
        return UniformSampler(train_data.num_items)


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


class MultiDAE(BaseRetriever):
    """recstudio/model/ae/multidae.py:37-67: one sample per user (``UserDataset``), no sampler, full softmax over the catalog.
    With ``model.fused_bag`` the training step is ``mean_b(lse_b - <q_b, mean_l item[pos_bl]>)`` -- the reference's second
    ``SoftmaxLoss`` branch (loss_func.py:39-47) reduced per user -- with the positives' mean one ``bag_pool`` over the item table:
    no ``[B, L, d]`` gather of the positives, no ``[B, L]`` scores.  ``lse`` comes from ``scorer.full_lse`` (no ``[B, N]`` scores)
    where the fused full softmax applies (an nn.Embedding catalog up to 128 wide), else from ``torch.logsumexp`` over the
    scorer's full scores.  With the flag off the step is the stock plugin path over the torch twin."""

    _model_defaults = (('dropout', 0.5), ('encoder_dims', [64, 32]), ('decoder_dims', [32, 64]), ('activation', 'relu'))
    _train_defaults = (('batch_size', 256), ('learning_rate', 0.01), ('weight_decay', 1e-5))

    def __init__(self, config=None, **kwargs):
        # recstudio/model/ae/config/multidae.yaml (multivae.yaml) on top of basemodel.yaml; the caller's config wins
        user = config or {}
        super().__init__(config, **kwargs)
        m = self.config['model']
        if 'embed_dim' not in user.get('model', {}):
            m['embed_dim'] = self.embed_dim = self._embed_dim_default
        for k, v in self._model_defaults + (('fused_bag', FUSED_BAG_DEFAULT),):
            m.setdefault(k, v)
        for k, v in self._train_defaults + (('device_loader', False),):        # UserDataset batches are assembled on the host
            if k not in user.get('train', {}):
                self.config['train'][k] = v

    _embed_dim_default = 200

    def _get_dataset_class():
        return UserDataset

    def _get_item_encoder(self, train_data):
        return torch.nn.Embedding(train_data.num_items, self.embed_dim, 0)

    def _get_query_encoder(self, train_data):
        m = self.config['model']
        return MultiDAEQueryEncoder(train_data.fiid, train_data.num_items, self.embed_dim, m['dropout'], m['encoder_dims'],
                                    m['decoder_dims'], m['activation'], fused_bag=m['fused_bag'])

    def _get_query_feat(self, data):
        return data if isinstance(data, dict) else super()._get_query_feat(data)

    def _get_score_func(self):
        return InnerProductScorer()

    def _get_sampler(self, train_data):
        return None

    def _get_loss_func(self):
        return SoftmaxLoss()

    def _bag_step_ok(self, batch):
        return (self.config['model'].get('fused_bag', False) and type(self.loss_fn) is SoftmaxLoss and self.sampler is None
                and type(self.score_func) is InnerProductScorer and isinstance(self.item_encoder, torch.nn.Embedding)
                and batch[self.fiid].dim() == 2 and batch[self.fiid].is_cuda)

    def _softmax_step(self, batch):
        if not self._bag_step_ok(batch):
            return BaseRetriever.training_step(self, batch)
        query = self.query_encoder(self._get_query_feat(batch))
        weight = self.item_encoder.weight
        pos = (bag_pool(weight, batch[self.fiid], 'mean') * query).sum(-1)
        if weight.shape[1] <= 128 and self.config['train'].get('fused_full_softmax', True):
            lse = full_lse(query, weight)
        else:
            lse = torch.logsumexp(self.score_func(query, self._get_item_vector()), dim=-1)
        return (lse - pos).mean()

    def training_step(self, batch):
        return self._softmax_step(batch)


class MultiVAE(MultiDAE):
    """recstudio/model/ae/multivae.py:63-105: MultiDAE's step plus ``anneal * kl_loss``, the weight rising by
    ``1 / train.anneal_total_step`` per step up to ``train.anneal_max`` (:97-105)."""

    _model_defaults = (('dropout_rate', 0.5), ('encoder_dims', [200]), ('decoder_dims', [200]), ('activation', 'tanh'))
    _train_defaults = (('batch_size', 500), ('learning_rate', 0.001), ('weight_decay', 1e-5), ('anneal_max', 0.2),
                       ('anneal_total_step', 2000000), ('early_stop_patience', 100))
    _embed_dim_default = 600

    def _get_query_encoder(self, train_data):
        m = self.config['model']
        return MultiVAEQueryEncoder(train_data.fiid, train_data.num_items, self.embed_dim, m['dropout_rate'], m['encoder_dims'],
                                    m['decoder_dims'], m['activation'], fused_bag=m['fused_bag'])

    def training_step(self, batch):
        loss = self._softmax_step(batch)
        if not hasattr(self, 'anneal'):
            setattr(self, 'anneal', 0)
        tr = self.config['train']
        anneal = min(tr['anneal_max'], self.anneal)
        self.anneal = min(tr['anneal_max'], self.anneal + (1.0 / tr['anneal_total_step']))
        return loss + anneal * self.query_encoder.kl_loss
