"""The sequence family: the towers over a user's history (SASRec, GRU4Rec, NARM, STAMP, Caser, HGN) and the retrievers built
on them.  Every tower gathers its history rows through ``gather._history_rows``; the fused cores are in ``seqmodule``."""
import math

import torch

from . import data_augmentation
from .dataset import SeqDataset
from .gather import _history_rows, _last_position
from .loss_func import BinaryCrossEntropyLoss, BPRLoss, SoftmaxLoss
from .retriever import BaseRetriever, _BatchQueryFeat
from .seqmodule import (AttentionLayer, FusedGRU, FusedTransformerEncoder, MLPModule, caser_conv_torch, caser_pack, hgn_gating,
                        hgn_gating_torch)

__all__ = ['SeqRetriever', 'SASRecQueryEncoder', 'SASRec', 'CL4SRec', 'GRU4RecQueryEncoder', 'GRU4Rec', 'NARMQueryEncoder', 'NARM',
           'STAMPQueryEncoder', 'STAMP', 'CaserQueryEncoder', 'HGNQueryEncoder', 'HGN']

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


class SeqRetriever(_BatchQueryFeat, BaseRetriever):
    """What every sequence retriever shares: ``SeqDataset``, and a query tower that takes the whole batch dict."""

    def _get_dataset_class():
        return SeqDataset


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
        if self.mask_id is not None and seg is None:
            # any ids handed over as a tensor (a view of CL4SRec): the mask token is no catalog row.  (The CSR view of the loader
            # gathers from the dataset's own item column, which holds no mask token.)
            masked = user_hist == self.mask_id
            rows = _history_rows(self.item_encoder, torch.where(masked, torch.zeros_like(user_hist), user_hist))
            rows = rows + masked.unsqueeze(-1).to(rows.dtype) * self.mask_emb
        else:
            rows = _history_rows(self.item_encoder, user_hist, seg)
        seq = rows + self.position_emb(positions)
        if self._fused is not None:
            out = self._fused(self.dropout(seq), key_pad=user_hist == 0, causal=not self.bidirectional)
        else:
            if self.bidirectional:
                mask = torch.zeros(L, L, dtype=torch.bool, device=user_hist.device)
            else:
                mask = torch.triu(torch.ones(L, L, dtype=torch.bool, device=user_hist.device), 1)
            out = self.transformer_layer(self.dropout(seq), mask=mask, src_key_padding_mask=user_hist == 0)
        return _last_position(out, batch['seqlen']) if need_pooling else out


class SASRec(SeqRetriever):
    """recstudio/model/seq/sasrec.py:70-123, recstudio/model/seq/config/sasrec.yaml, with the retriever tail on the fused path."""

    config_defaults = {'model': {'hidden_size': 128, 'layer_num': 2, 'head_num': 2, 'dropout_rate': 0.5, 'activation': 'gelu',
                                 'layer_norm_eps': 1e-12, 'fused_attention': False},
                       'train': {'negative_count': 1, 'init_method': 'normal'}}

    def _get_query_encoder(self, train_data):
        m = self.config['model']
        return SASRecQueryEncoder(self.fiid, self.embed_dim, train_data.config['max_seq_len'], m['head_num'],
                                  m['hidden_size'], m['dropout_rate'], m['activation'], m['layer_norm_eps'],
                                  m['layer_num'], self.item_encoder, fused_attention=m['fused_attention'])

    def _get_loss_func(self):
        return BinaryCrossEntropyLoss()         # sasrec.py:117-119


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

    config_defaults = {'model': {'hidden_size': 64, 'layer_num': 1, 'temperature': 1.0, 'augment_type': 'item_crop', 'tau': 0.2,
                                 'cl_weight': 0.1, 'fused_augment': True, 'fused_infonce': FUSED_INFONCE_DEFAULT}}

    def _init_model(self, train_data, drop_unused_field=True):
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
        rows = _history_rows(self.item_encoder, batch['in_' + self.fiid], batch.get('_seg'))
        seqlen = batch['seqlen']
        if self._fused is not None:
            out, _ = self._fused(self.dropout(rows), lengths=seqlen, want_state=False)
        else:
            out, _ = self.gru(self.dropout(rows))
        return self.dense(_last_position(out, seqlen))


class GRU4Rec(SeqRetriever):
    """recstudio/model/seq/gru4rec.py:17-63, recstudio/model/seq/config/gru4rec.yaml, with the retriever tail on the fused BPR
    path."""

    config_defaults = {'model': {'hidden_size': 128, 'dropout_rate': 0.3, 'layer_num': 1, 'fused_gru': True},
                       'train': {'negative_count': 1}}

    def _get_query_encoder(self, train_data):
        m = self.config['model']
        return GRU4RecQueryEncoder(self.fiid, self.embed_dim, m['hidden_size'], m['dropout_rate'], m['layer_num'],
                                   self.item_encoder, fused_gru=m['fused_gru'])

    def _get_loss_func(self):
        return BPRLoss()


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
        rows = self.gru_layer['1'](_history_rows(self.item_encoder, user_hist, batch.get('_seg')))
        seqlen = batch['seqlen']
        if self._fused is not None:
            gru_vec, _ = self._fused(rows, lengths=seqlen, want_state=False)
        else:
            gru_vec, _ = self.gru_layer['2'].gru(rows)
        c_global = h_t = _last_position(gru_vec, seqlen)                                           # B x H
        c_local = self.attn_layer(query=h_t.unsqueeze(1), key=gru_vec, value=gru_vec, key_padding_mask=user_hist == 0,
                                  need_weight=False).squeeze(1)                                    # B x H
        return self.fc(torch.cat((c_global, c_local), dim=1))                                      # B x D


class _SeqSoftmaxRetriever(SeqRetriever):
    """What NARM and STAMP add to it: SoftmaxLoss and no sampler -- ``training_step`` takes the 'full_softmax' path, which never
    holds [B, N]."""

    def _get_loss_func(self):
        return SoftmaxLoss()

    def _get_sampler(self, train_data):
        return None


class NARM(_SeqSoftmaxRetriever):
    """recstudio/model/seq/narm.py:50-88, recstudio/model/seq/config/narm.yaml, with the retriever tail on the fused full-softmax
    path."""

    config_defaults = {'model': {'hidden_size': 128, 'dropout_rate': [0.25, 0.5], 'layer_num': 1, 'fused_gru': True,
                                 'fused_attention_pool': FUSED_ATTENTION_POOL_DEFAULT}}

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
        seq_emb = _history_rows(self.item_encoder, user_hist, batch.get('_seg'))
        m_t = _last_position(seq_emb, batch['seqlen'])
        m_s = seq_emb.sum(dim=1) / batch['seqlen'].unsqueeze(1).float()                            # B x D
        query = torch.cat((m_t, m_s), dim=1)                                                       # B x 2D
        m_a = self.attention_layer(query.unsqueeze(1), seq_emb, seq_emb, key_padding_mask=(user_hist == 0)).squeeze(1)
        return self.mlpA(m_a) * self.mlpB(m_t)


class STAMP(_SeqSoftmaxRetriever):
    """recstudio/model/seq/stamp.py:35-61, recstudio/model/seq/config/stamp.yaml (embed_dim 64), with the retriever tail on the
    fused full-softmax path."""

    config_defaults = {'model': {'fused_attention_pool': FUSED_ATTENTION_POOL_DEFAULT}}

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
        item_seq, seg = batch['in_' + self.fiid], batch.get('_seg')
        if item_seq.size(1) < self.max_seq_len:
            # caser.py:39; the CSR view would give the unpadded width, so the padded ids are gathered as ids
            item_seq, seg = torch.nn.functional.pad(item_seq, (0, self.max_seq_len - item_seq.size(1))), None
        rows = _history_rows(self.item_embedding, item_seq, seg)
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
        S = _history_rows(self.item_encoder, batch['in_' + self.fiid], batch.get('_seg'))             # B x L x D
        ug = self.W_g_2(U) + self.b_g
        ui = U @ self.W_g_4.weight[:S.size(1)].T                                                      # B x L
        gate = hgn_gating if self.fused_gating else hgn_gating_torch
        return U + gate(S, ug, ui, self.W_g_1.weight, self.w_g_3.weight.view(-1), self.pooling_type)


class HGN(SeqRetriever):
    """recstudio/model/seq/hgn.py:47-68, recstudio/model/seq/config/hgn.yaml, with the retriever tail on the fused BPR path."""

    config_defaults = {'model': {'pooling_type': 'mean', 'fused_gating': FUSED_GATING_DEFAULT},
                       'train': {'negative_count': 1}}

    def _get_query_encoder(self, train_data):
        m = self.config['model']
        return HGNQueryEncoder(self.fuid, self.fiid, train_data.num_users, self.embed_dim, train_data.config['max_seq_len'],
                               self.item_encoder, m['pooling_type'], fused_gating=m['fused_gating'])

    def _get_loss_func(self):
        return BPRLoss()
