"""Graph modules -- host-side mirror of ``recstudio.model.module.graphmodule`` for LightGCN, with the propagation on
``rsa_spmm_csr`` (recstudio_amd/csrc/rsa_spmm.hip) instead of dgl message passing.

``NormAdj`` is what the reference holds as a ``dgl.graph`` plus the two degree-norm vectors of ``LightGCNNet.forward``
(graphmodule.py:176-188, mess_norm 'both'): the normalised adjacency ``D^-1/2 A D^-1/2`` in CSR with the norms folded into the edge
values.  ``LightGCNNet`` is graphmodule.py:190-198 with ``LightGCNCombiner`` (:89-94, the identity on the neighbour message) and
the layer mean of lightgcn.py:56-60 in one autograd node.  ``GraphUserEncoder`` / ``GraphItemEncoder``: graphmodule.py:97-111.
"""
import torch

from . import ops

__all__ = ['NormAdj', 'LightGCNNet', 'GraphUserEncoder', 'GraphItemEncoder']


def _csr_by(key, other, weights, n):
    """CSR of the edges grouped by ``key`` (stable: a row's edges keep their input order) -> (indptr int64 [n + 1], other[order]
    int32, weights[order])."""
    order = torch.sort(key, stable=True).indices
    count = torch.bincount(key, minlength=n)
    indptr = torch.cat([count.new_zeros(1), torch.cumsum(count, 0)])
    return indptr, other[order].to(torch.int32), weights[order]


class NormAdj:
    """Normalised adjacency of a graph given as edges ``rows -> cols`` over ``n_nodes`` nodes (duplicates are multi-edges, as in
    ``dgl.graph``): ``y = adj @ x`` is ``y[dst] = in_deg(dst)^-1/2 * sum over edges src -> dst of out_deg(src)^-1/2 * x[src]``, a
    degree of 0 giving the factor 0.  Stored as the CSR over destination rows -- ``indptr`` int64 [n + 1], ``indices`` int32 [nnz]
    (the sources), ``values`` fp32 [nnz] = the product of the two factors taken in float64 and rounded once -- with the chunk
    ``plan`` of ``ops.spmm_csr``.  The transposed CSR is built as well: the backward of the product multiplies by it.  For the
    bidirectional interaction graph the matrix is symmetric and the two are the SAME arrays, which ``from_dataset`` asserts."""

    def __init__(self, rows, cols, n_nodes, chunk=None, symmetric=False):
        rows, cols = torch.as_tensor(rows, dtype=torch.int64), torch.as_tensor(cols, dtype=torch.int64)
        n = int(n_nodes)
        if rows.shape != cols.shape or rows.dim() != 1:
            raise ValueError('NormAdj: rows and cols must be 1-D id columns of the same length')
        if n >= 1 << 31:
            raise ValueError('NormAdj: the node count must fit int32 column indices')
        if rows.numel() and (int(min(rows.min(), cols.min())) < 0 or int(max(rows.max(), cols.max())) >= n):
            raise ValueError(f'NormAdj: node ids must lie in [0, {n})')
        out_deg, in_deg = torch.bincount(rows, minlength=n), torch.bincount(cols, minlength=n)
        norm = lambda deg: torch.where(deg > 0, deg.double().pow(-0.5), deg.new_zeros(n, dtype=torch.float64))      # noqa: E731
        weights = (norm(out_deg)[rows] * norm(in_deg)[cols]).to(torch.float32)
        chunk = ops.SPMM_CHUNK if chunk is None else int(chunk)
        self.n_nodes, self.nnz, self.chunk = n, int(rows.numel()), chunk
        self.in_deg, self.out_deg = in_deg, out_deg
        self.indptr, self.indices, self.values = _csr_by(cols, rows, weights, n)
        t = _csr_by(rows, cols, weights, n)
        self.symmetric = all(torch.equal(a, b) for a, b in zip(t, (self.indptr, self.indices, self.values)))
        if symmetric and not self.symmetric:
            raise AssertionError('NormAdj: the graph was declared symmetric but its CSR differs from its transposed CSR')
        self.plan = ops.spmm_plan(self.indptr, chunk)
        if self.symmetric:
            self.t_indptr, self.t_indices, self.t_values, self.t_plan = self.indptr, self.indices, self.values, self.plan
        else:
            self.t_indptr, self.t_indices, self.t_values = t
            self.t_plan = ops.spmm_plan(self.t_indptr, chunk)

    @classmethod
    def from_dataset(cls, train_data, chunk=None):
        """The graph lightgcn.py:29-31 builds: every training interaction (u, i) as u -> num_users + i and back; the two padding
        nodes (0 and num_users) have no edges."""
        n = train_data.num_users + train_data.num_items
        (rows, cols, _, shape), _ = train_data.get_graph([0], form='coo', value_fields='inter', col_offset=[train_data.num_users],
                                                         bidirectional=[True], shape=(n, n))
        return cls(rows, cols, shape[0], chunk=chunk, symmetric=True)

    def to(self, device):
        device = torch.device(device)
        if self.indptr.device != device:
            for name in ('indptr', 'indices', 'values') + (() if self.symmetric else ('t_indptr', 't_indices', 't_values')):
                setattr(self, name, getattr(self, name).to(device))
            if self.symmetric:
                self.t_indptr, self.t_indices, self.t_values = self.indptr, self.indices, self.values
            self.plan.to(device)
            self.t_plan.to(device)
        return self

    def csr(self, transposed=False):
        return (self.t_indptr, self.t_indices, self.t_values, self.t_plan) if transposed else \
            (self.indptr, self.indices, self.values, self.plan)


def _layer_mean(csr, e0, n_layers):
    """(E_0 + A E_0 + ... + A^L E_0) / (L + 1): L launches of ``ops.spmm_csr``, each adding its layer to the running sum in its
    epilogue; the last one writes no layer output and scales the sum."""
    indptr, indices, values, plan = csr
    L = int(n_layers)
    acc = e0.detach().clone(memory_format=torch.contiguous_format)
    x, spare = e0.detach().contiguous(), [None, None]
    for k in range(L):
        last = k == L - 1
        y = None
        if not last:
            y = spare[k % 2] = torch.empty_like(acc) if spare[k % 2] is None else spare[k % 2]
        ops.spmm_csr(indptr, indices, values, x, plan=plan, y=y, acc=acc, acc_scale=1.0 / (L + 1) if last else 1.0)
        x = y
    return acc


class _PropagateFn(torch.autograd.Function):
    """The layers are linear, so no layer output is kept: the backward is the same L launches, with the transposed matrix, on
    the incoming gradient -- dE_0 = 1 / (L + 1) * sum_k (A^T)^k g."""

    @staticmethod
    def forward(ctx, e0, adj, n_layers):
        ctx.adj, ctx.n_layers = adj, n_layers
        return _layer_mean(adj.csr(), e0, n_layers)

    @staticmethod
    def backward(ctx, g):
        return _layer_mean(ctx.adj.csr(transposed=True), g, ctx.n_layers), None, None


class LightGCNNet(torch.nn.Module):
    def __init__(self, n_layers):
        super().__init__()
        if int(n_layers) < 0:
            raise ValueError('LightGCNNet: n_layers must not be negative')
        self.n_layers = int(n_layers)

    def propagate(self, adj, embeddings):
        """``embeddings`` fp32 [n_nodes, d] (d a multiple of 4, at most 256) -> the mean over the layers E_0 .. E_L."""
        if embeddings.shape[0] != adj.n_nodes:
            raise ValueError(f'LightGCNNet: {embeddings.shape[0]} embedding rows for a graph of {adj.n_nodes} nodes')
        adj.to(embeddings.device)
        if self.n_layers == 0:
            return embeddings
        return _PropagateFn.apply(embeddings, adj, self.n_layers)

    forward = propagate


class GraphItemEncoder(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.item_embeddings = None

    def forward(self, batch_data):
        return self.item_embeddings[batch_data]


class GraphUserEncoder(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.user_embeddings = None

    def forward(self, batch_data):
        return self.user_embeddings[batch_data]
