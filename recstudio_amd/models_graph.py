"""The graph family: LightGCN and what derives from it (SGL, SimGCL, NGCF).  The propagation modules are in ``graphmodule``,
the views in ``data_augmentation``; everything behind the propagation is ``BaseRetriever``'s fused path."""
import torch

from . import data_augmentation, graphmodule
from .fused import retriever_scores
from .gather import _EmbedFn
from .loss_func import BPRLoss, FullScoreLoss, l2_reg_loss_fn
from .retriever import BaseRetriever
from .scorer import CosineScorer, EuclideanScorer, InnerProductScorer

__all__ = ['LightGCN', 'SGL', 'SimGCL', 'NGCF']


class LightGCN(BaseRetriever):
    """recstudio/model/graph/lightgcn.py:14-84, recstudio/model/graph/config/{all,lightgcn}.yaml (n_layers 3, l2_reg_weight 1e-4,
    negative_count 1).  The base tables ``user_emb`` / ``item_emb`` are propagated over the normalised interaction graph
    (``graphmodule.NormAdj``, ``rsa_spmm_csr``); everything behind the propagation is the fused path: the propagated item table is
    the ``item_weight`` of ``fused.retriever_scores``, the propagated user table its ``query_src`` with the batch's user ids as
    ``query_index`` -- the negatives are drawn in the kernel (the ids ``UniformSampler`` gives for the seed), no [B, n, d] tensor
    exists, and the dense table gradients flow back into the propagation's backward.  The towers are not nn.Embedding modules,
    so ``train.fused_optimizer``, multi-GPU ``fit`` and ``train.ann`` refuse this model as they refuse any such tower."""

    config_defaults = {'model': {'n_layers': 3, 'l2_reg_weight': 1e-4},
                       'train': {'negative_count': 1, 'early_stop_patience': 100},
                       'eval': {'cutoff': [20, 10, 5]}}

    def _init_model(self, train_data, drop_unused_field=True):
        super()._init_model(train_data, drop_unused_field)
        self.num_users, self.num_items = train_data.num_users, train_data.num_items
        self.user_emb = torch.nn.Embedding(self.num_users, self.embed_dim, padding_idx=0)
        self.item_emb = torch.nn.Embedding(self.num_items, self.embed_dim, padding_idx=0)
        net = self._get_gnn_net()
        setattr(self, type(net).__name__, net)
        self.adj_mat = self._get_graph(train_data)

    def _get_gnn_net(self):
        """The propagation module; ``_init_model`` registers it under its class name."""
        return graphmodule.LightGCNNet(self.config['model']['n_layers'])

    def _get_graph(self, train_data):
        """The normalised adjacency of the training interactions (``model.spmm_chunk``: the chunk size of its plan, default
        ``ops.SPMM_CHUNK``)."""
        return graphmodule.NormAdj.from_dataset(train_data, chunk=self.config['model'].get('spmm_chunk'))

    def _get_loss_func(self):
        return BPRLoss()

    def _get_query_encoder(self, train_data):
        return graphmodule.GraphUserEncoder()

    def _get_item_encoder(self, train_data):
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

    config_defaults = {'model': {'aug_type': 'ED', 'ssl_ratio': 0.1, 'ssl_reg': 0.1, 'temperature': 0.2},
                       'train': {'batch_size': 2048}}

    def _init_model(self, train_data, drop_unused_field=True):
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

    config_defaults = {'model': {'eps': 0.1, 'cl_weight': 0.5, 'cl_neg_type': 'all', 'temperature': 0.2},
                       'train': {'batch_size': 2048, 'learning_rate': 0.001}}

    def _init_model(self, train_data, drop_unused_field=True):
        super()._init_model(train_data, drop_unused_field)
        self.augmentation_model = data_augmentation.SimGCLAugmentation(self.config['model'], train_data)

    def _get_gnn_net(self):
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
    config_defaults = {'model': {'layer_size': [64, 64, 64, 64], 'node_dropout': 0.1, 'l2_reg_weight': 1e-5},
                       'train': {'batch_size': 2048, 'learning_rate': 1e-4}}

    def __init__(self, config=None, **kwargs):
        super().__init__(config, **kwargs)
        model = self.config['model']
        # derived from layer_size, whoever set it: the layer count, and one mess_dropout per layer unless the caller gave them
        model['n_layers'] = len(model['layer_size']) - 1
        model.setdefault('mess_dropout', [0.1] * model['n_layers'])
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
        super()._init_model(train_data, drop_unused_field)
        self.left_adj = graphmodule.LeftAdj(self.adj_mat)
        self.last_view = None

    def _get_gnn_net(self):
        model = self.config['model']
        layers = [int(v) for v in model['layer_size']]
        self.combiners = torch.nn.ModuleList(graphmodule.BiCombiner(a, b, dropout=float(p))
                                             for a, b, p in zip(layers[:-1], layers[1:], model['mess_dropout']))
        return graphmodule.NGCFNet(self.combiners, len(layers) - 1)

    def _propagate(self, embeddings):
        drop = self.config['model']['node_dropout']
        adj = self.left_adj
        if self.training and drop:
            self.adj_mat.to(embeddings.device)
            adj = self.last_view = graphmodule.LeftAdj.thinned(self.adj_mat, 1.0 - float(drop))
        return self.NGCFNet.propagate(adj, embeddings)
