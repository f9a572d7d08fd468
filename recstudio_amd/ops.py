"""Tensor-level wrappers over the C ABI (include/recstudio_amd.h).

PyTorch is used for device memory, streams and the generator state only; every
computation below happens in the HIP kernels of librecstudio_amd.so.  All
tensors must live on a ROCm device -- there is no CPU path.
"""
import ctypes
import functools
import math

import torch

from . import _native as nat
from . import placement, rng
from ._native import ptr


# Integer all-zero log-probabilities (what the reference's UniformSampler hands out, sampler.py:113-114) come from a
# small cache of persistent zero buffers (one per element count and device) and are recognised by address, not by
# reading them back: the losses would otherwise need a host sync per step to learn that there is nothing to subtract
# (and the sampler a memset per step).  They are constants: nothing in the package or in the reference writes to them.
_ZERO_LOGP = {}


def zero_logp_like(ids):
    """An int64 all-zero tensor shaped like ``ids`` (a view of a cached constant buffer)."""
    return zero_logp(ids.shape, ids.device)


def zero_logp(shape, device):
    """The same constant for a shape / device instead of a template tensor."""
    shape = tuple(int(x) for x in shape)
    numel = 1
    for x in shape:
        numel *= x
    device = torch.device(device)
    if device.type == 'cuda' and device.index is None:
        device = torch.device('cuda', torch.cuda.current_device())
    key = (numel, device)
    z = _ZERO_LOGP.get(key)
    if z is None:
        if len(_ZERO_LOGP) >= 16:              # a handful of batch shapes at most; do not grow without bound
            _ZERO_LOGP.clear()
        z = _ZERO_LOGP[key] = torch.zeros(numel, dtype=torch.int64, device=device)
    return z.view(shape)


def is_known_zero(t):
    if t.is_floating_point():
        return False
    z = _ZERO_LOGP.get((t.numel(), t.device))
    return z is not None and z.data_ptr() == t.data_ptr()


# Every native launch runs on the CURRENT STREAM OF THE DEVICE ITS TENSORS LIVE ON, with that device made current
# for the duration of the call (torch.cuda.device guard): a model on cuda:1 while cuda:0 is the process's current
# device (BaseRetriever honours train.gpu = [1] without calling set_device) must not launch on device 0's stream
# against device-1 pointers.  All tensor arguments of one call must share the device.
_LAUNCH_DEV = []


def _raw_stream(dev=None):
    """hipStream_t (as an int) of the current stream of ``dev``.  torch.cuda.current_stream() builds a Stream object
    (6 us a call, seven calls per sharded step); the raw getter is a plain C call."""
    index = dev.index if dev is not None and dev.index is not None else torch.cuda.current_device()
    return torch._C._cuda_getCurrentRawStream(index)


def _stream():
    return ctypes.c_void_p(_raw_stream(_LAUNCH_DEV[-1] if _LAUNCH_DEV else None))


def _launch(name, *args):
    """``nat.launch`` on the current stream of the launch device: every one-shot native call of ops.py and shard.py."""
    nat.launch(name, _stream(), *args)


def _tensor_device(args, kwargs):
    dev = None
    for a in list(args) + list(kwargs.values()):
        if isinstance(a, torch.Tensor) and a.is_cuda:
            if dev is None:
                dev = a.device
            elif a.device != dev:
                raise RuntimeError(f'recstudio_amd: tensors of one call live on different devices ({dev} and {a.device})')
    return dev


def _on_device(fn):
    """Run ``fn`` under the device guard of its tensor arguments (see above)."""
    @functools.wraps(fn)
    def wrapped(*args, **kwargs):
        dev = _tensor_device(args, kwargs)
        if dev is None:
            d = kwargs.get('device')
            if d is None:
                d = next((a for a in args if isinstance(a, (torch.device, str))), None)
            dev = torch.device(d) if d is not None else None
            if dev is not None and dev.type == 'cuda' and dev.index is None:
                dev = torch.device('cuda', torch.cuda.current_device())
        if dev is None or dev.type != 'cuda':
            return fn(*args, **kwargs)       # CPU tensors: the op's own _need() raises the "GPU only" error
        _LAUNCH_DEV.append(dev)
        try:
            if dev.index == torch.cuda.current_device():
                return fn(*args, **kwargs)
            with torch.cuda.device(dev):
                return fn(*args, **kwargs)
        finally:
            _LAUNCH_DEV.pop()
    return wrapped


# Caller-owned reduction scratch of the C ABI (rsa_scratch_bytes(): arrival counter + partial sums of the in-kernel
# loss reduction, rsa_mean_rows' partials, the BCE valid-row counter): one zero-filled block per (device, stream),
# so that launches on different streams or devices never share words.
_SCRATCH = {}


def _scratch():
    dev = _LAUNCH_DEV[-1] if _LAUNCH_DEV else torch.device('cuda', torch.cuda.current_device())
    return _scratch_for(dev, _raw_stream(dev))


def _scratch_for(dev, raw_stream):
    key = (dev.index, raw_stream)
    t = _SCRATCH.get(key)
    if t is None:
        if len(_SCRATCH) >= 64:          # short-lived streams: forget the oldest blocks (a block is only ever used on its stream)
            for old in list(_SCRATCH)[:32]:
                del _SCRATCH[old]
        t = _SCRATCH[key] = torch.zeros(int(nat.lib().rsa_scratch_bytes()), dtype=torch.uint8, device=dev)
    return t


def _need_view(t, dtype, name):
    """The checks of ``_need`` for a tensor that the kernel reads in place through its strides (no contiguous copy)."""
    if not isinstance(t, torch.Tensor):
        raise TypeError(f'{name}: expected a tensor, got {type(t)}')
    if not t.is_cuda:
        raise RuntimeError(f'{name}: recstudio_amd runs on the GPU only (got a {t.device} tensor); '
                           'there is no CPU fallback')
    if t.dtype != dtype:
        raise TypeError(f'{name}: expected {dtype}, got {t.dtype}')
    return t


def _need(t, dtype, name):
    t = _need_view(t, dtype, name)
    return t if t.is_contiguous() else t.contiguous()


def _need_opt(t, dtype, name):
    return None if t is None else _need(t, dtype, name)


def _workspace_bytes(sizer, *dims):
    """(what the size query ``sizer`` returns for ``dims`` -- the ``workspace_bytes`` the library is told --, the bytes to set
    aside for it: never an empty buffer).  Callers that carve the workspace out of an arena use this directly."""
    nbytes = int(getattr(nat.lib(), sizer)(*dims))
    return nbytes, max(nbytes, 8)


def _workspace(dev, sizer, *dims):
    """(uint8 workspace tensor on ``dev``, workspace_bytes) for the size query ``sizer``."""
    nbytes, alloc = _workspace_bytes(sizer, *dims)
    return torch.empty(alloc, dtype=torch.uint8, device=dev), nbytes


def _score_mode(cosine):
    """rsa_score_mode from the wrappers' ``cosine`` argument: a bool (inner product / cosine) or the mode itself."""
    return int(cosine) if not isinstance(cosine, bool) else (nat.SCORE_COS if cosine else nat.SCORE_IP)


# ------------------------------------------------------------------ samplers
@_on_device
def sample_uniform(numel, low, high, device, generator=None):
    """int64 [numel], == torch.randint(low, high, (numel,), device=device) incl. generator advance."""
    out = torch.empty(int(numel), dtype=torch.int64, device=device)
    if numel == 0:
        return out
    pc = rng.reserve(numel, rng.randint_unroll(low, high), device, generator)
    _launch('rsa_sample_uniform', ptr(out), int(numel), int(low), int(high), pc.seed, pc.offset, pc.grid_threads, pc.elem_base)
    return out


@_on_device
def sample_masked_uniform(user_hist, num_items, per_row, generator=None):
    """int64 [B, per_row]: uniform over [1, num_items] minus each row's history (sampler.py:117-147)."""
    user_hist = _need(user_hist, torch.int64, 'user_hist')
    B, Lh = user_hist.shape
    out = torch.empty(B, int(per_row), dtype=torch.int64, device=user_hist.device)
    if B * per_row:
        pc = rng.reserve(B * per_row, 4, user_hist.device, generator)
        _launch('rsa_sample_masked_uniform', ptr(user_hist), B, Lh, int(num_items), int(per_row), ptr(out),
                pc.seed, pc.offset, pc.grid_threads, pc.elem_base)
    return out


def popular_args(table, pop_prob, guide, guide_log2, cdf_lut=None, cdf_lines=None, lines_log2=0):
    """rsa_popular_args with the sampler's tables filled in (checked device fp32 / int32 tensors)"""
    a = nat.PopularArgs()
    a.table, a.pop_prob, a.guide = ptr(table), ptr(pop_prob), ptr(guide)
    a.n_items, a.guide_log2, a.lines_log2 = table.numel(), int(guide_log2), int(lines_log2)
    a.cdf_lut = ptr(_need_opt(cdf_lut, torch.float32, 'cdf_lut'))
    a.cdf_lines = ptr(_need_opt(cdf_lines, torch.float32, 'cdf_lines'))
    return a


@_on_device
def sample_popular(table, pop_prob, guide, guide_log2, numel, generator=None, want_u=False, cdf_lut=None,
                   cdf_lines=None, lines_log2=0):
    table = _need(table, torch.float32, 'table')
    pop_prob = _need(pop_prob, torch.float32, 'pop_prob')
    guide = _need_opt(guide, torch.int32, 'guide')
    dev = table.device
    ids = torch.empty(int(numel), dtype=torch.int64, device=dev)
    logp = torch.empty(int(numel), dtype=torch.float32, device=dev)
    u = torch.empty(int(numel), dtype=torch.float32, device=dev) if want_u else None
    if numel:
        pc = rng.reserve(numel, 4, dev, generator)
        a = popular_args(table, pop_prob, guide, guide_log2, cdf_lut, cdf_lines, lines_log2)
        a.ids, a.logp, a.u_out, a.numel = ptr(ids), ptr(logp), ptr(u), int(numel)
        a.seed, a.offset, a.grid_threads, a.elem_base = pc.seed, pc.offset, pc.grid_threads, pc.elem_base
        _launch('rsa_sample_popular', ctypes.byref(a))
    return (ids, logp, u) if want_u else (ids, logp)


@_on_device
def popular_lookup(table, pop_prob, guide, guide_log2, u, cdf_lut=None, cdf_lines=None, lines_log2=0):
    table = _need(table, torch.float32, 'table')
    pop_prob = _need(pop_prob, torch.float32, 'pop_prob')
    guide = _need_opt(guide, torch.int32, 'guide')
    u = _need(u, torch.float32, 'u')
    ids = torch.empty(u.numel(), dtype=torch.int64, device=u.device)
    logp = torch.empty(u.numel(), dtype=torch.float32, device=u.device)
    a = popular_args(table, pop_prob, guide, guide_log2, cdf_lut, cdf_lines, lines_log2)
    a.u_in, a.ids, a.logp, a.numel = ptr(u), ptr(ids), ptr(logp), u.numel()
    _launch('rsa_popular_lookup', ctypes.byref(a))
    return ids.view(u.shape), logp.view(u.shape)


@_on_device
def item_logp(pop_prob, ids):
    pop_prob = _need(pop_prob, torch.float32, 'pop_prob')
    ids = _need(ids, torch.int64, 'ids')
    out = torch.empty(ids.shape, dtype=torch.float32, device=ids.device)
    _launch('rsa_item_logp', ptr(pop_prob), pop_prob.numel(), ptr(ids), ids.numel(), ptr(out))
    return out


def _codebook_shape(centres, who):
    """(n_parts, K, d_sub) of a stacked codebook [n_parts, K, d_sub], with the limits of rsa_midx_args checked."""
    if centres.dim() != 3 or centres.shape[0] not in (1, 2):
        raise ValueError(f'{who}: centres must be [n_parts (1 or 2), K, dim / n_parts], got {tuple(centres.shape)}')
    parts, K, dsub = (int(v) for v in centres.shape)
    dim = parts * dsub
    if not 2 <= K <= 64:
        raise ValueError(f'{who}: the number of clusters must be in [2, 64], got {K}')
    if dim % 8 or dim > 256:
        raise ValueError(f'{who}: embed_dim must be a multiple of 8 and at most 256, got {dim}')
    return parts, K, dsub


@_on_device
def kmeans_step(table, centres, *, normalize=False):
    """rsa_kmeans_step: one assignment pass of k-means over the rows of ``table`` [N, d] (any row stride: ``weight[1:]`` is
    read in place) against ``centres`` [n_parts, K, d / n_parts] -> (assign int32 [n_parts, N], sums fp32 [n_parts, K, d_sub],
    counts int32 [n_parts, K], loss float64 [n_parts]).  ``normalize``: rows divided by max(||row||, 1e-12) first."""
    centres = _need(centres, torch.float32, 'centres')
    table = _need_view(table, torch.float32, 'table')
    parts, K, dsub = _codebook_shape(centres, 'kmeans_step')
    dim = parts * dsub
    if table.dim() != 2 or table.shape[1] != dim or table.shape[0] < 1:
        raise ValueError(f'kmeans_step: table must be [N >= 1, {dim}], got {tuple(table.shape)}')
    base, stride, skip, table = _table_view(table, dim)
    n, dev = table.shape[0], table.device
    assign = torch.empty(parts, n, dtype=torch.int32, device=dev)
    sums = torch.empty(parts, K, dsub, dtype=torch.float32, device=dev)
    counts = torch.empty(parts, K, dtype=torch.int32, device=dev)
    loss = torch.empty(parts, dtype=torch.float64, device=dev)
    a = nat.KmeansArgs()
    a.table, a.n_rows, a.row_stride, a.row_offset = base, n, stride, skip
    a.dim, a.n_parts, a.n_clusters, a.normalize = dim, parts, K, int(bool(normalize))
    a.centres, a.assign, a.sums, a.counts, a.loss = ptr(centres), ptr(assign), ptr(sums), ptr(counts), ptr(loss)
    ws, a.workspace_bytes = _workspace(dev, 'rsa_kmeans_workspace_bytes', n, dim, K)
    a.workspace = ptr(ws)
    _launch('rsa_kmeans_step', ctypes.byref(a))
    return assign, sums, counts, loss


def _table_view(table, dim):
    """(base pointer, row stride, row offset, the tensor to keep alive) of a row table read in place: a view that starts a whole
    number of rows into its storage (``weight[1:]``) goes down as base pointer + row offset; anything the kernels cannot stride
    over is copied."""
    if table.stride(1) != 1 or table.stride(0) % 4 or table.stride(0) < dim or table.data_ptr() % 16:
        table = table.contiguous()
    stride = table.stride(0)
    skip = table.storage_offset() // stride if table.storage_offset() % stride == 0 else 0
    return table.data_ptr() - skip * stride * 4, stride, skip, table


@_on_device
def midx_weights(pop, indptr, indices, n_clusters, n_parts, *, table=None, dim=8):
    """rsa_midx_weights: the per-epoch tables of the popularity-in-bucket samplers from ``pop`` [N] (the weight of ids 1 .. N) and
    the index of the last update (int32 ``indptr`` [K^n_parts + 1], ``indices`` [N]).  ``table`` [N, d] (any row stride): the
    weight is multiplied by exp(-||row||^2 / 2), the Euclidean scorer's form.
    -> (p [N + 1], item_logp [N + 1], wkk [K^n_parts], cp [N]), all fp32."""
    pop = _need(pop, torch.float32, 'pop')
    indptr, indices = _need(indptr, torch.int32, 'indptr'), _need(indices, torch.int32, 'indices')
    K, parts, n = int(n_clusters), int(n_parts), pop.numel()
    if parts not in (1, 2) or not 2 <= K <= 64:
        raise ValueError(f'midx_weights: n_parts must be 1 or 2 and the number of clusters in [2, 64], got {parts}, {K}')
    if n < 1 or pop.dim() != 1 or indices.numel() != n or indptr.numel() != K ** parts + 1:
        raise ValueError(f'midx_weights: pop [N >= 1], indices [N] and indptr [K^n_parts + 1] do not match (N = {n}, K = {K})')
    dev = pop.device
    a = nat.MidxWeightsArgs()
    if table is not None:
        table = _need_view(table, torch.float32, 'table')
        dim = int(table.shape[1]) if table.dim() == 2 else 0
        if table.dim() != 2 or table.shape[0] != n or dim % 8 or not 8 <= dim <= 256:
            raise ValueError(f'midx_weights: table must be [{n}, d] with d a multiple of 8 and at most 256, got {tuple(table.shape)}')
        base, a.row_stride, a.row_offset, table = _table_view(table, dim)
        a.table = base
    out = carve(dev, [('p', (n + 1,), torch.float32), ('logp', (n + 1,), torch.float32), ('wkk', (K ** parts,), torch.float32),
                      ('cp', (n,), torch.float32)])
    a.pop, a.n_items, a.dim, a.n_parts, a.n_clusters = ptr(pop), n, int(dim), parts, K
    a.indptr, a.indices = ptr(indptr), ptr(indices)
    a.p, a.item_logp, a.wkk, a.cp = ptr(out['p']), ptr(out['logp']), ptr(out['wkk']), ptr(out['cp'])
    _launch('rsa_midx_weights', ctypes.byref(a))
    return out['p'], out['logp'], out['wkk'], out['cp']


def _midx_args(query, centres, wkk, indptr, indices, cd, num_neg, pos_ids, cosine, who, cp=None, item_logp=None):
    query = _need(query, torch.float32, 'query')
    centres = _need(centres, torch.float32, 'centres')
    parts, K, dsub = _codebook_shape(centres, who)
    dim = parts * dsub
    if query.dim() != 2 or query.shape[1] != dim:
        raise ValueError(f'{who}: query must be [M, {dim}], got {tuple(query.shape)}')
    M, n = query.shape[0], int(num_neg)
    a = nat.MidxArgs()
    a.query, a.n_queries, a.dim, a.n_parts, a.n_clusters = ptr(query), M, dim, parts, K
    a.score_mode = nat.SCORE_COS if cosine else nat.SCORE_IP
    a.centres, a.num_neg = ptr(centres), n
    if len(cd) != parts:
        raise ValueError(f'{who}: one cluster map per part')
    cd = [_need(c, torch.int32, 'cd') for c in cd]
    a.n_items = cd[0].numel() - 1
    a.cd0, a.cd1 = ptr(cd[0]), ptr(cd[1] if parts == 2 else None)
    if n:
        wkk, indptr, indices = _need(wkk, torch.float32, 'wkk'), _need(indptr, torch.int32, 'indptr'), _need(indices, torch.int32, 'indices')
        if wkk.numel() != K ** parts or indptr.numel() != K ** parts + 1 or indices.numel() != a.n_items:
            raise ValueError(f'{who}: wkk / indptr / indices do not match K = {K}, n_items = {a.n_items}')
        a.wkk, a.indptr, a.indices = ptr(wkk), ptr(indptr), ptr(indices)
    dev = query.device
    out = dict(neg_ids=torch.empty(M, n, dtype=torch.int64, device=dev), neg_logp=torch.empty(M, n, dtype=torch.float32, device=dev))
    if n:
        a.neg_ids, a.neg_logp = ptr(out['neg_ids']), ptr(out['neg_logp'])
    if pos_ids is not None:
        pos_ids = _need(pos_ids, torch.int64, 'pos_ids')
        if pos_ids.dim() != 2 or pos_ids.shape[0] != M:
            raise ValueError(f'{who}: pos_ids must be [M, T]')
        out['pos_logp'] = torch.empty(pos_ids.shape, dtype=torch.float32, device=dev)
        a.n_pos, a.pos_ids, a.pos_logp = pos_ids.shape[1], ptr(pos_ids), ptr(out['pos_logp'])
    if cp is not None or item_logp is not None:
        if cp is None or item_logp is None:
            raise ValueError(f'{who}: cp and item_logp go together')
        cp, item_logp = _need(cp, torch.float32, 'cp'), _need(item_logp, torch.float32, 'item_logp')
        if cp.numel() != a.n_items or item_logp.numel() != a.n_items + 1:
            raise ValueError(f'{who}: cp must hold n_items = {a.n_items} entries and item_logp one more')
        a.cp, a.item_logp = ptr(cp), ptr(item_logp)
    return a, out


@_on_device
def midx_sample(query, centres, wkk, indptr, indices, cd, num_neg, *, pos_ids=None, cosine=False, generator=None,
                want_u=False, cp=None, item_logp=None):
    """rsa_midx_sample: negatives of MIDXSamplerUniform (``centres`` [2, K, d / 2]) / ClusterSamplerUniform ([1, K, d]) for
    ``query`` [M, d], the uniforms those of ``torch.rand(M, num_neg, n_parts + 1)`` on the device generator (advanced as that
    call would).  ``cd``: the int32 cluster maps [N + 1] per part; ``pos_ids`` [M, T]: also their ``compute_item_p``.
    ``cp`` [N] / ``item_logp`` [N + 1] (``midx_weights``): the item is drawn from the bucket's CDF instead of uniformly, and its
    log-weight is added to both log-probabilities (MIDXSamplerPop / ClusterSamplerPop).
    -> dict(neg_ids [M, n] int64, neg_logp [M, n], pos_logp [M, T], u [M, n, n_parts + 1] with ``want_u``)."""
    a, out = _midx_args(query, centres, wkk, indptr, indices, cd, num_neg, pos_ids, cosine, 'midx_sample', cp, item_logp)
    numel = a.n_queries * a.num_neg * (a.n_parts + 1)
    if numel:
        pc = rng.reserve(numel, 4, query.device, generator)
        a.seed, a.offset, a.grid_threads, a.elem_base = pc.seed, pc.offset, pc.grid_threads, pc.elem_base
        if want_u:
            out['u'] = torch.empty(a.n_queries, a.num_neg, a.n_parts + 1, dtype=torch.float32, device=query.device)
            a.u_out = ptr(out['u'])
    _launch('rsa_midx_sample', ctypes.byref(a))
    return out


@_on_device
def midx_lookup(query, centres, wkk, indptr, indices, cd, u, *, pos_ids=None, cosine=False, cp=None, item_logp=None):
    """rsa_midx_lookup: the draw of ``midx_sample`` for caller-supplied uniforms ``u`` [M, n, n_parts + 1]."""
    u = _need(u, torch.float32, 'u')
    if u.dim() != 3:
        raise ValueError('midx_lookup: u must be [M, n, n_parts + 1]')
    a, out = _midx_args(query, centres, wkk, indptr, indices, cd, u.shape[1], pos_ids, cosine, 'midx_lookup', cp, item_logp)
    if u.shape[0] != a.n_queries or u.shape[2] != a.n_parts + 1:
        raise ValueError('midx_lookup: u must be [M, n, n_parts + 1]')
    a.u_in = ptr(u)
    _launch('rsa_midx_lookup', ctypes.byref(a))
    return out


def _hash_shape(weight_vectors, who):
    """(dim, n_bits, n_table) of ``LSHSampler.weight_vectors`` [d, K, L], with the limits of rsa_lsh_hash_args checked."""
    if weight_vectors.dim() != 3:
        raise ValueError(f'{who}: weight_vectors must be [dim, n_bits, n_table], got {tuple(weight_vectors.shape)}')
    dim, K, L = (int(v) for v in weight_vectors.shape)
    if dim % 8 or not 8 <= dim <= 256:
        raise ValueError(f'{who}: embed_dim must be a multiple of 8 and at most 256, got {dim}')
    if not 1 <= K <= 16:
        raise ValueError(f'{who}: n_bits must be in [1, 16], got {K}')
    if L < 1 or K * L > 64:
        raise ValueError(f'{who}: n_bits * n_table must be at most 64 (one lane of a wave per projection), got {K} * {L}')
    return dim, K, L


@_on_device
def lsh_hash(table, weight_vectors):
    """rsa_lsh_hash: the LSH codes of the rows of ``table`` [N, d] (any row stride: ``weight[1:]`` is read in place) under the
    projections ``weight_vectors`` [d, K, L] -> int32 [L, N]; bit (k, l) is ``<row, W[:, k, l]> > 0``, the first bit the most
    significant."""
    weight_vectors = _need(weight_vectors, torch.float32, 'weight_vectors')
    table = _need_view(table, torch.float32, 'table')
    dim, K, L = _hash_shape(weight_vectors, 'lsh_hash')
    if table.dim() != 2 or table.shape[1] != dim or table.shape[0] < 1:
        raise ValueError(f'lsh_hash: table must be [N >= 1, {dim}], got {tuple(table.shape)}')
    base, stride, skip, table = _table_view(table, dim)
    n = table.shape[0]
    codes = torch.empty(L, n, dtype=torch.int32, device=table.device)
    a = nat.LshHashArgs()
    a.table, a.n_rows, a.row_stride, a.row_offset = base, n, stride, skip
    a.dim, a.n_bits, a.n_table = dim, K, L
    a.weight_vectors, a.codes = ptr(weight_vectors), ptr(codes)
    _launch('rsa_lsh_hash', ctypes.byref(a))
    return codes


def _lsh_args(query, weight_vectors, indptr, indices, item_embs, num_neg, eps, want_codes, who):
    query = _need(query, torch.float32, 'query')
    weight_vectors = _need(weight_vectors, torch.float32, 'weight_vectors')
    dim, K, L = _hash_shape(weight_vectors, who)
    if query.dim() != 2 or query.shape[1] != dim:
        raise ValueError(f'{who}: query must be [M, {dim}], got {tuple(query.shape)}')
    indptr, indices = _need(indptr, torch.int32, 'indptr'), _need(indices, torch.int32, 'indices')
    item_embs = _need(item_embs, torch.float32, 'item_embs')
    if item_embs.dim() != 2 or item_embs.shape[1] != dim or item_embs.shape[0] < 1:
        raise ValueError(f'{who}: item_embs must be [N >= 1, {dim}], got {tuple(item_embs.shape)}')
    N = item_embs.shape[0]
    if tuple(indptr.shape) != (L, (1 << K) + 1) or tuple(indices.shape) != (L, N):
        raise ValueError(f'{who}: indptr must be [{L}, {(1 << K) + 1}] and indices [{L}, {N}], got {tuple(indptr.shape)} and '
                         f'{tuple(indices.shape)}')
    if eps < 0:
        raise ValueError(f'{who}: eps must not be negative')
    M, n, dev = query.shape[0], int(num_neg), query.device
    out = dict(neg_ids=torch.empty(M, n, dtype=torch.int64, device=dev), neg_logp=torch.empty(M, n, dtype=torch.float32, device=dev))
    a = nat.LshArgs()
    a.query, a.n_queries, a.dim, a.n_bits, a.n_table, a.num_neg = ptr(query), M, dim, K, L, n
    a.weight_vectors, a.indptr, a.indices, a.item_embs, a.n_items = ptr(weight_vectors), ptr(indptr), ptr(indices), ptr(item_embs), N
    a.neg_ids, a.neg_logp, a.log_eps = ptr(out['neg_ids']), ptr(out['neg_logp']), float(eps)
    if want_codes:
        out['codes'] = torch.empty(M, L, dtype=torch.int32, device=dev)
        a.codes_out = ptr(out['codes'])
    return a, out, (query, weight_vectors, indptr, indices, item_embs)


@_on_device
def lsh_sample(query, weight_vectors, indptr, indices, item_embs, num_neg, *, eps=0.0, generator=None, want_u=False,
               want_codes=False):
    """rsa_lsh_sample: negatives of LSHSampler for ``query`` [M, d] from the index ``indptr`` int32 [L, 2^K + 1] / ``indices``
    int32 [L, N] over the snapshot ``item_embs`` [N, d]; the uniforms are those of ``torch.rand(M, num_neg)`` on the device
    generator (advanced as that call would).  ``eps`` is added inside the log (1e-12 with pos_items in the reference, 0 without).
    -> dict(neg_ids [M, n] int64, neg_logp [M, n], u [M, n] with ``want_u``, codes int32 [M, L] with ``want_codes``)."""
    a, out, keep = _lsh_args(query, weight_vectors, indptr, indices, item_embs, num_neg, eps, want_codes, 'lsh_sample')
    numel = a.n_queries * a.num_neg
    if numel:
        pc = rng.reserve(numel, 4, query.device, generator)
        a.seed, a.offset, a.grid_threads, a.elem_base = pc.seed, pc.offset, pc.grid_threads, pc.elem_base
    if want_u:
        out['u'] = torch.empty(a.n_queries, a.num_neg, dtype=torch.float32, device=query.device)
        a.u_out = ptr(out['u'])
    _launch('rsa_lsh_sample', ctypes.byref(a))
    return out


@_on_device
def lsh_lookup(query, weight_vectors, indptr, indices, item_embs, u, *, eps=0.0, want_codes=False):
    """rsa_lsh_lookup: the draw of ``lsh_sample`` for caller-supplied uniforms ``u`` [M, n]."""
    u = _need(u, torch.float32, 'u')
    if u.dim() != 2 or u.shape[0] != query.shape[0]:
        raise ValueError('lsh_lookup: u must be [M, n]')
    a, out, keep = _lsh_args(query, weight_vectors, indptr, indices, item_embs, u.shape[1], eps, want_codes, 'lsh_lookup')
    a.u_in = ptr(u)
    _launch('rsa_lsh_lookup', ctypes.byref(a))
    return out


# ------------------------------------------------------------------ gathers
@_on_device
def embedding_gather(table, ids):
    table = _need(table, torch.float32, 'table')
    ids = _need(ids, torch.int64, 'ids')
    n_rows, dim = table.shape
    out = torch.empty(*ids.shape, dim, dtype=torch.float32, device=table.device)
    _launch('rsa_embedding_gather', ptr(table), n_rows, dim, ptr(ids), ids.numel(), ptr(out))
    return out


@_on_device
def scatter_add_rows(src, ids, n_rows, out=None):
    """dst[ids[i]] += src[i] for ids != 0 (embedding_dense_backward with padding_idx = 0).  ``out``: accumulate
    into an existing [n_rows, dim] tensor instead of a fresh zero one."""
    src = _need(src, torch.float32, 'src')
    ids = _need(ids, torch.int64, 'ids')
    dim = src.shape[-1]
    dst = _need(out, torch.float32, 'out') if out is not None else torch.zeros(n_rows, dim, dtype=torch.float32,
                                                                                device=src.device)
    _launch('rsa_scatter_add_rows', ptr(src), ptr(ids), ids.numel(), dim, ptr(dst), n_rows)
    return dst


@_on_device
def seg_gather(item_table, flat_item_ids, seg_start, seg_end, max_len, want_rows=True, want_ids=True):
    flat = _need(flat_item_ids, torch.int64, 'flat_item_ids')
    s = _need(seg_start, torch.int64, 'seg_start')
    e = _need(seg_end, torch.int64, 'seg_end')
    dev = flat.device
    B = s.numel()
    tab = _need(item_table, torch.float32, 'item_table') if want_rows else None
    dim = tab.shape[1] if tab is not None else 4
    n_items = tab.shape[0] if tab is not None else 1
    ids = torch.empty(B, max_len, dtype=torch.int64, device=dev) if want_ids else None
    rows = torch.empty(B, max_len, dim, dtype=torch.float32, device=dev) if want_rows else None
    lens = torch.empty(B, dtype=torch.int64, device=dev)
    a = nat.SegGatherArgs()
    a.item_table, a.n_items, a.dim, a.max_len = ptr(tab), n_items, dim, int(max_len)
    a.flat_item_ids, a.n_flat, a.seg_start, a.seg_end, a.n_seg = ptr(flat), flat.numel(), ptr(s), ptr(e), B
    a.out_ids, a.out_rows, a.out_len = ptr(ids), ptr(rows), ptr(lens)
    _launch('rsa_seg_gather', ctypes.byref(a))
    return ids, rows, lens


def carve(dev, specs, align=4096):
    """``{key: tensor}`` for ``specs = [(key, shape, dtype), ...]``, every tensor a view of ONE allocation.

    Why: the buffers a launch WRITES must not come from separate allocations.  The headline launch (four [B, n] output arrays,
    84 MB of the 2.8 GB it moves) ran 404-409 us on every one of 31 layouts of those arrays inside one allocation (any skew
    between them, any shift, arenas of 86 MB .. 1 GB) and 443-471 us on 5 of 9 sets of separately allocated arrays of the same
    shapes in the same processes (profiles/r05_output_placement.json; moving any ONE of the four into an arena did not help).
    The class belongs to the allocation; with ``RSA_PLACEMENT=1`` (opt-in) ``placement.pick`` probes candidates and returns one of
    the fast class -- by default the arena is one plain ``torch.empty``."""
    offs, total = [], 0
    for _, shape, dtype in specs:
        cnt = 1
        for v in shape:
            cnt *= int(v)
        offs.append((total, cnt))
        total += (cnt * torch.empty((), dtype=dtype).element_size() + align - 1) // align * align
    arena = placement.pick(max(total, align), dev)          # plain torch.empty unless placement was asked for
    out = {}
    for (key, shape, dtype), (off, cnt) in zip(specs, offs):
        nb = cnt * torch.empty((), dtype=dtype).element_size()
        out[key] = arena[off:off + nb].view(dtype).view(tuple(int(v) for v in shape))
    return out


# ------------------------------------------------------------------ fused forward / backward
@_on_device
def fused_forward(item_table, query, num_neg, *, query_index=None, pos_ids=None, neg_ids=None,
                  sampler=nat.SAMPLER_GIVEN, cosine=False, mask_pad_pos=False,
                  table=None, pop_prob=None, guide=None, guide_log2=0, generator=None, n_queries=None,
                  out=None, want_logp=True, table_prob=None, fused_bpr=False, want_mean=True, cdf_lut=None,
                  want_query_grad=False, rng_state=None, cdf_lines=None, lines_log2=0, fused_loss=None,
                  pos_logp=None, neg_logp=None, _plan=None, inplace_update=None, n_batches=1, want_scores=True):
    """One launch of rsa_fused_sample_gather_score.  Returns a dict with
    neg_ids [M,n] int64, neg_score [M,n], pos_score [M] (if pos_ids), and for the
    popularity sampler neg_logp [M,n], pos_logp [M].  ``out``: a dict returned by an earlier
    call with the same shapes, whose buffers are overwritten instead of allocating.
    ``want_logp=False`` skips the log-probability outputs of the popularity sampler (BPR ignores
    them, loss_func.py:55-59).  ``fused_bpr=True`` (needs num_neg % 64 == 0 and pos_ids) evaluates
    BPRLoss in the kernel's epilogue: adds ``loss`` (scalar), ``row_loss [M]``, ``dpos [M]``,
    ``dneg [M, n]`` to the result; with ``want_query_grad`` (inner product, dim in {32, 64, 128, 256}) also
    ``query_grad [M, d]`` = d loss / d query row, accumulated while the rows are in registers.
    ``fused_loss='ssm'`` (same conditions, inner product, dim in {32, 64, 128, 256}): SampledSoftmaxLoss in the
    epilogue instead (one wave per query carries the logsumexp over its num_neg / 64 tiles); with ids given,
    ``pos_logp`` / ``neg_logp`` are the INPUT log-probabilities.  ``cdf_lines`` / ``lines_log2``: the bucket-line
    form of the popularity sampler's inverse CDF (PopularSamplerModel.cdf_lines).
    ``want_scores=False`` (with a loss the kernel fuses): ``neg_score`` is not written and not returned -- a training forward
    needs d loss/d score, not the scores (4 B/triplet less).
    ``n_batches`` = S > 1: a QUEUE of S independent batches consumed by one launch -- ``query_index`` / ``pos_ids`` hold the
    S batches back to back ([S * B]); the outputs are those of S consecutive ``fused_forward`` calls over B queries each,
    concatenated (every batch draws its negatives from its own torch call: the generator is advanced S times), ``loss``
    is the [S] vector of the batches' mean losses.  In-kernel samplers only."""
    item_table = _need(item_table, torch.float32, 'item_table')
    query = _need(query, torch.float32, 'query')
    dev = item_table.device
    n_items, dim = item_table.shape
    if query.dim() != 2 or query.shape[1] != dim:
        raise ValueError(f'query must be [rows, {dim}], got {tuple(query.shape)}')
    query_index = _need_opt(query_index, torch.int64, 'query_index')
    pos_ids = _need_opt(pos_ids, torch.int64, 'pos_ids')
    if n_queries is None:
        n_queries = query_index.numel() if query_index is not None else query.shape[0]
    M, n = int(n_queries), int(num_neg)
    if pos_ids is not None and pos_ids.numel() != M:
        raise ValueError('pos_ids must have one id per query')
    a = nat.FusedArgs()
    # (None: the launch does not consume the torch generator -- nothing for ``FusedStep`` to reserve per step)
    unroll = None if sampler == nat.SAMPLER_GIVEN or rng_state is not None else rng.sampler_unroll(sampler, n_items)
    if sampler == nat.SAMPLER_GIVEN:
        neg_ids = _need(neg_ids, torch.int64, 'neg_ids')
        if neg_ids.numel() != M * n:
            raise ValueError('neg_ids must be [M, num_neg]')
    else:
        neg_ids = out['neg_ids'] if out is not None else None          # (allocated with the other outputs below)
        if rng_state is not None:
            # graph-capturable form: (seed, device int64 tensor holding the offset); the caller advances it
            # (rsa_rng_advance) and mirrors the consumption into the torch generator afterwards
            seed, offset_dev = rng_state
            cu, mt = rng.device_props(dev)
            a.seed, a.offset, a.grid_threads = int(seed) & 0xFFFFFFFFFFFFFFFF, 0, rng.grid_threads(M * n, cu, mt)
            a.offset_dev = ptr(offset_dev)
        elif n_batches > 1:
            if M % n_batches:
                raise ValueError('n_batches must divide the number of queries')
            per = M // int(n_batches) * n
            pc = rng.reserve(per, unroll, dev, generator, repeat=int(n_batches))
            if pc.elem_base:
                raise NotImplementedError('fused_forward(n_batches=...) inside rng.sharded_stream')
            a.seed, a.offset, a.grid_threads, a.elem_base = pc.seed, pc.offset, pc.grid_threads, 0
            a.n_batches, a.batch_offset_step = int(n_batches), rng.counter_offset(per, pc.grid_threads, unroll)
            want_mean = False
        else:
            pc = rng.reserve(M * n, unroll, dev, generator)
            a.seed, a.offset, a.grid_threads, a.elem_base = pc.seed, pc.offset, pc.grid_threads, pc.elem_base
    reuse = out is not None        # caller-provided output buffers (same keys/shapes as returned)
    if fused_loss is None and fused_bpr:
        fused_loss = 'bpr'
    score_mode = _score_mode(cosine)
    composed = fused_loss == 'bpr' and n != 64 and (dim not in (32, 64, 128, 256) or score_mode != nat.SCORE_IP)
    keep_scores = want_scores or fused_loss not in ('bpr', 'ssm') or composed
    f32 = torch.float32
    loss_specs = []
    if fused_loss in ('bpr', 'ssm'):
        loss_specs = [('dneg', (M, n), f32), ('loss', (), f32), ('row_loss', (M,), f32), ('dpos', (M,), f32)]
        if want_query_grad:
            loss_specs.append(('query_grad', (M, dim), f32))
    if reuse:
        missing = [spec for spec in loss_specs if spec[0] not in out]      # a dict of an earlier call without this loss
        if missing:
            out.update(carve(dev, missing))
    else:
        # every output of the launch out of ONE allocation (carve): see there for why
        specs = [('neg_score', (M, n), f32)] if keep_scores else []
        if sampler != nat.SAMPLER_GIVEN:
            specs.insert(0, ('neg_ids', (M, n), torch.int64))
        if pos_ids is not None:
            specs.append(('pos_score', (M,), f32))
        if sampler == nat.SAMPLER_POPULAR and want_logp:
            specs.append(('neg_logp', (M, n), f32))
            if pos_ids is not None:
                specs.append(('pos_logp', (M,), f32))
        out = carve(dev, specs + loss_specs)
        if sampler != nat.SAMPLER_GIVEN:
            neg_ids = out['neg_ids']
    out['neg_ids'] = neg_ids.view(M, n)
    if sampler == nat.SAMPLER_POPULAR:
        table = _need(table, torch.float32, 'table')
        pop_prob = _need(pop_prob, torch.float32, 'pop_prob')
        guide = _need_opt(guide, torch.int32, 'guide')
    a.item_table, a.n_items, a.dim = ptr(item_table), n_items, dim
    a.score_mode = score_mode
    a.query, a.query_index, a.n_query_rows = ptr(query), ptr(query_index), query.shape[0]
    a.pos_ids, a.n_queries, a.num_neg = ptr(pos_ids), M, n
    a.sampler, a.mask_pad_pos, a.guide_log2 = int(sampler), int(bool(mask_pad_pos)), int(guide_log2)
    a.table, a.pop_prob, a.guide = ptr(table), ptr(pop_prob), ptr(guide)
    a.table_prob = ptr(_need_opt(table_prob, torch.float32, 'table_prob'))
    a.cdf_lut = ptr(_need_opt(cdf_lut, torch.float32, 'cdf_lut'))
    a.cdf_lines, a.lines_log2 = ptr(_need_opt(cdf_lines, torch.float32, 'cdf_lines')), int(lines_log2)
    if sampler == nat.SAMPLER_GIVEN and fused_loss == 'ssm' and (pos_logp is not None or neg_logp is not None):
        # ids given: the log-probabilities are INPUTS of the SampledSoftmax epilogue
        a.neg_logp, a.pos_logp = ptr(_need_opt(neg_logp, torch.float32, 'neg_logp')), ptr(_need_opt(pos_logp, torch.float32, 'pos_logp'))
        a.neg_ids = ptr(neg_ids)
    else:
        a.neg_ids, a.neg_logp, a.pos_logp = ptr(neg_ids), ptr(out.get('neg_logp')), ptr(out.get('pos_logp'))
    a.pos_score, a.neg_score = ptr(out.get('pos_score')), ptr(out['neg_score'] if keep_scores else None)
    if composed:
        # queries longer than one tile are walked by one workgroup (no atomics): that kernel covers the stock dims and
        # the inner product; anything else runs the loss as its own (equally deterministic) launch
        if want_query_grad:
            raise ValueError('want_query_grad needs the inner-product scorer and dim in {32, 64, 128, 256}')
        if n_batches > 1:
            raise ValueError('fused_forward(n_batches=...) with a fused BPR loss needs num_neg == 64, or the inner-product scorer '
                             'and dim in {32, 64, 128, 256} (this configuration is composed of two launches)')
        _launch('rsa_fused_sample_gather_score', ctypes.byref(a))
        out['loss'], out['dpos'], out['dneg'], out['row_loss'] = pairwise_loss(nat.LOSS_BPR, out['pos_score'], out['neg_score'])
        return out
    if fused_loss is not None:
        if fused_loss not in ('bpr', 'ssm'):
            raise ValueError("fused_loss must be None, 'bpr' or 'ssm'")
        a.fused_loss = (nat.LOSS_BPR if fused_loss == 'bpr' else nat.LOSS_SSM) + 1
        a.row_loss, a.loss_out = ptr(out['row_loss']), ptr(out['loss'] if want_mean else None)
        if want_mean:
            a.reduce_scratch = ptr(_scratch())
        a.dpos, a.dneg = ptr(out['dpos']), ptr(out['dneg'])
        if want_query_grad:
            a.query_grad = ptr(out['query_grad'])
        if inplace_update is not None:
            # (solo_flags, scale): rows touched by exactly one element of the step (sort_step_elements) are updated inside
            # the forward: item_table += scale * d * q
            solo_flags, upd_scale = inplace_update
            a.solo_flags, a.upd_scale = ptr(_need(solo_flags, torch.uint8, 'solo_flags')), ptr(_need(upd_scale, torch.float32, 'upd_scale'))
    elif want_query_grad:
        raise ValueError('want_query_grad needs a fused loss (fused_bpr=True / fused_loss=...)')
    if n_batches > 1 and (sampler == nat.SAMPLER_GIVEN or rng_state is not None):
        raise ValueError('fused_forward(n_batches=...) draws its negatives in the kernel from the torch generator')
    _launch('rsa_fused_sample_gather_score', ctypes.byref(a))
    if n_batches > 1 and fused_loss is not None:
        _queue_losses(out, int(n_batches))
    if _plan is not None:
        _plan.update(args=a, out=out, device=dev, generator=generator, numel=M * n, n_batches=int(n_batches), unroll=unroll,
                     keep=(item_table, query, query_index, pos_ids, neg_ids, table, pop_prob, guide))
    return out


def _queue_losses(out, n_batches):
    """out['loss'] [S] <- the per-batch means of a queue launch's row losses (the kernel's own mean is per LAUNCH and is off for a
    queue), written IN PLACE into one persistent buffer: ``FusedStep`` hands out the same dict on every call."""
    cur = out.get('loss')
    if cur is None or cur.dim() != 1 or cur.numel() != n_batches:
        out['loss'] = torch.empty(n_batches, dtype=torch.float32, device=out['row_loss'].device)
    torch.mean(out['row_loss'].view(n_batches, -1), dim=1, out=out['loss'])


class FusedStep:
    """A ``fused_forward`` call frozen into its argument block: ``step()`` re-launches the same kernel on the same
    buffers, drawing fresh negatives (the generator is advanced exactly as a ``fused_forward`` call would).  What it
    saves is host time only -- tensor checks, the ctypes struct fill: ~35 us of Python per call, more than a B = 4096
    launch runs on the GPU.  The outputs are the dict of the first call (overwritten in place by every step)."""

    def __init__(self, item_table, query, num_neg, **kw):
        if kw.get('out') is not None or kw.get('rng_state') is not None:
            raise ValueError('FusedStep owns its output buffers and reads the torch generator')
        self._p = {}
        self.out = fused_forward(item_table, query, num_neg, _plan=self._p, **kw)
        if 'args' not in self._p:
            raise ValueError('this configuration is composed of several launches: call fused_forward')
        self._fn = nat.lib().rsa_fused_sample_gather_score
        self._ref = ctypes.byref(self._p['args'])

    def __call__(self):
        p = self._p
        if p['unroll'] is not None:
            nb = p.get('n_batches', 1)
            pc = rng.reserve(p['numel'] // nb, p['unroll'], p['device'], p['generator'], repeat=nb)
            a = p['args']
            a.seed, a.offset, a.grid_threads, a.elem_base = pc.seed, pc.offset, pc.grid_threads, pc.elem_base
        rc = self._fn(self._ref, ctypes.c_void_p(_raw_stream(p['device'])))
        if rc != 0:
            nat.check(rc, 'rsa_fused_sample_gather_score')
        if p.get('n_batches', 1) > 1 and 'row_loss' in self.out:      # a queue's per-batch losses are the host side's
            with torch.cuda.device(p['device']):
                _queue_losses(self.out, p['n_batches'])
        return self.out


@_on_device
def score_packed_keys(item_table, query, keys):
    """Scores of (query row, item row) pairs packed as (qrow << 32) | irow (rsa_shard_route's keys): the fused
    gather+score kernel reading the pairs directly."""
    item_table = _need(item_table, torch.float32, 'item_table')
    query = _need(query, torch.float32, 'query')
    keys = _need(keys, torch.int64, 'keys')
    m = keys.numel()
    out = torch.empty(m, dtype=torch.float32, device=keys.device)
    if m == 0:
        return out
    a = nat.FusedArgs()
    a.item_table, a.n_items, a.dim = ptr(item_table), item_table.shape[0], item_table.shape[1]
    a.query, a.n_query_rows = ptr(query), query.shape[0]
    a.n_queries, a.num_neg, a.sampler = m, 1, nat.SAMPLER_GIVEN
    a.packed_keys, a.neg_score = ptr(keys), ptr(out)
    _launch('rsa_fused_sample_gather_score', ctypes.byref(a))
    return out


def _loss(who, kind, pos_score, neg_score, pos_logp, neg_logp, want_grad=True, shared=False, param0=0.0, param1=0.0):
    """The one body of the loss wrappers -> (loss, dpos, dneg, row_loss).  ``shared``: rsa_ssm_shared_loss over pos_score [B, L]
    and neg_score [B, n]; otherwise rsa_pairwise_loss over one positive and n negatives per row."""
    pos_score = _need(pos_score, torch.float32, 'pos_score')
    neg_score = _need(neg_score, torch.float32, 'neg_score')
    if shared:
        (M, n_pos), n = pos_score.shape, neg_score.shape[1]
    else:
        M, n_pos = pos_score.numel(), 0
        n = neg_score.numel() // max(M, 1)
        if neg_score.numel() != M * n or M == 0 or n == 0:
            raise ValueError(f'{who}: pos {tuple(pos_score.shape)} vs neg {tuple(neg_score.shape)}')
    pos_logp = _need_opt(pos_logp, torch.float32, 'pos_logp')
    neg_logp = _need_opt(neg_logp, torch.float32, 'neg_logp')
    dev = pos_score.device
    row = torch.empty(M, dtype=torch.float32, device=dev)
    loss = torch.empty((), dtype=torch.float32, device=dev)
    dpos = torch.empty_like(pos_score) if want_grad else None
    dneg = torch.empty_like(neg_score) if want_grad else None
    a = nat.LossArgs()
    a.loss_kind, a.n_rows, a.num_neg, a.n_pos = int(kind), M, n, n_pos
    a.pos_score, a.neg_score, a.pos_logp, a.neg_logp = ptr(pos_score), ptr(neg_score), ptr(pos_logp), ptr(neg_logp)
    a.row_loss, a.loss_out, a.dpos, a.dneg, a.scratch = ptr(row), ptr(loss), ptr(dpos), ptr(dneg), ptr(_scratch())
    a.param0, a.param1 = float(param0), float(param1)
    _launch('rsa_ssm_shared_loss' if shared else 'rsa_pairwise_loss', ctypes.byref(a))
    return loss, dpos, dneg, row


@_on_device
def pairwise_loss(kind, pos_score, neg_score, pos_logp=None, neg_logp=None, want_grad=True):
    """(loss [scalar tensor], dpos [M] | None, dneg [M,n] | None, row_loss [M])."""
    return _loss('pairwise_loss', kind, pos_score, neg_score, pos_logp, neg_logp, want_grad)


@_on_device
def pairwise_loss_ex(kind, pos_score, neg_score, pos_logp=None, neg_logp=None, param0=0.0, param1=0.0):
    """rsa_pairwise_loss, kinds WeightedBPR / WeightedBCE / Hinge / NCE / CCL: (loss, dpos, dneg)."""
    if not nat.LOSS_WBPR <= int(kind) <= nat.LOSS_CCL:
        raise ValueError(f'pairwise_loss_ex: unknown loss kind {kind}')
    return _loss('pairwise_loss_ex', kind, pos_score, neg_score, pos_logp, neg_logp, param0=param0, param1=param1)[:3]


@_on_device
def ssm_shared_loss(pos_score, neg_score, pos_logp=None, neg_logp=None):
    """rsa_ssm_shared_loss: pos_score [B, L], neg_score [B, n].  Returns (loss, dpos, dneg)."""
    return _loss('ssm_shared_loss', nat.LOSS_SSM, pos_score, neg_score, pos_logp, neg_logp, shared=True)[:3]


@_on_device
def fused_backward(item_table, query, neg_ids, dneg, *, query_index=None, pos_ids=None, dpos=None, upstream=None,
                   dense_item_grad=True, row_item_grad=False, want_query_grad=True, query_table_grad=None,
                   item_grad_out=None, query_table_pad_row=0, item_pad_row=0, cosine=False):
    """rsa_fused_backward.  Returns (item_grad [N,d] | None, item_grad_rows [M*(n+1), d] | None,
    query_grad [M,d] | None)."""
    item_table = _need(item_table, torch.float32, 'item_table')
    query = _need(query, torch.float32, 'query')
    neg_ids = _need(neg_ids, torch.int64, 'neg_ids')
    dneg = _need(dneg, torch.float32, 'dneg')
    query_index = _need_opt(query_index, torch.int64, 'query_index')
    pos_ids = _need_opt(pos_ids, torch.int64, 'pos_ids')
    dpos = _need_opt(dpos, torch.float32, 'dpos')
    upstream = _need_opt(upstream, torch.float32, 'upstream')
    dev = item_table.device
    n_items, dim = item_table.shape
    M = query_index.numel() if query_index is not None else query.shape[0]
    n = neg_ids.numel() // M
    if item_grad_out is not None:          # accumulate into a caller-provided (zeroed or running) dense buffer
        item_grad = _need(item_grad_out, torch.float32, 'item_grad_out')
    else:
        item_grad = torch.zeros(n_items, dim, dtype=torch.float32, device=dev) if dense_item_grad else None
    bufs = carve(dev, ([('rows', (M * (n + 1), dim), torch.float32)] if row_item_grad else []) +
                 ([('qgrad', (M, dim), torch.float32)] if want_query_grad else []))
    rows, qgrad = bufs.get('rows'), bufs.get('qgrad')
    if rows is not None and pos_ids is None:
        rows.zero_()
    a = nat.BackwardArgs()
    a.item_table, a.n_items, a.dim, a.num_neg = ptr(item_table), n_items, dim, n
    a.query, a.query_index, a.n_query_rows = ptr(query), ptr(query_index), query.shape[0]
    a.pos_ids, a.neg_ids, a.n_queries = ptr(pos_ids), ptr(neg_ids), M
    a.dpos, a.dneg, a.upstream = ptr(dpos), ptr(dneg), ptr(upstream)
    a.item_grad, a.item_grad_rows, a.query_grad = ptr(item_grad), ptr(rows), ptr(qgrad)
    a.query_table_grad = ptr(_need_opt(query_table_grad, torch.float32, 'query_table_grad'))
    a.query_table_pad_row = int(query_table_pad_row)
    a.item_pad_row = int(item_pad_row)
    a.score_mode = _score_mode(cosine)
    _launch('rsa_fused_backward', ctypes.byref(a))
    return item_grad, rows, qgrad


def _rows_update_args(target, query, query_index, n_queries, num_neg, dpos, dneg, upstream, pad_row):
    a = nat.RowsUpdateArgs()
    a.query, a.query_index, a.n_query_rows = ptr(query), ptr(_need_opt(query_index, torch.int64, 'query_index')), query.shape[0]
    a.dim, a.n_queries, a.num_neg = target.shape[1], int(n_queries), int(num_neg)
    a.dpos, a.dneg = ptr(_need_opt(dpos, torch.float32, 'dpos')), ptr(dneg)
    a.upstream = ptr(_need_opt(upstream, torch.float32, 'upstream'))
    a.n_items, a.pad_row, a.target = target.shape[0], int(pad_row), ptr(target)
    return a


def _rule_fields(a, rule, who):
    """``rule``: ('adam', exp_avg, exp_avg_sq, lr, betas, eps, step) or ('adagrad', state_sum, lr, lr_decay, eps, step) -> its fields of
    the block.  Doubles, as the caller holds them: the library derives 1 - beta and the bias corrections (ABI 12), or clr = lr /
    (1 + (step - 1) lr_decay), from these and rounds each kernel constant to fp32 once."""
    kind, *state, lr, hp, eps, step = rule
    if kind == 'adam':
        a.exp_avg = ptr(_need(state[0], torch.float32, who + ': exp_avg'))
        a.exp_avg_sq = ptr(_need(state[1], torch.float32, who + ': exp_avg_sq'))
        a.beta1, a.beta2 = float(hp[0]), float(hp[1])
    else:
        a.rule, a.state_sum, a.lr_decay = nat.ROWS_ADAGRAD, ptr(_need(state[0], torch.float32, who + ': state_sum')), float(hp)
    a.lr, a.eps, a.step = float(lr), float(eps), int(step)


@_on_device
def sort_step_elements(pos_ids, neg_ids, n_items, pad_row=0, want_solo=True):
    """rsa_sort_step_elements: the step's (item id, element) pairs sorted by id in a workspace, and the classification
    ``solo [M, 1 + n]`` uint8 (column 0 = the positive): 1 where no other element of the step touches that item row.
    -> (solo, workspace) for ``fused_forward(inplace_update=...)`` + ``scatter_rows_presorted``.
    The sorted pairs (int64 ``key << 32 | element``, bit 31 of the element word set on the solo ones) start
    ``rsa_scatter_rows_sorted_pairs_offset(M, n, n_items)`` bytes into ``workspace``."""
    neg_ids = _need(neg_ids, torch.int64, 'neg_ids')
    pos_ids = _need_opt(pos_ids, torch.int64, 'pos_ids')
    M = pos_ids.numel() if pos_ids is not None else neg_ids.shape[0]
    n = neg_ids.numel() // max(M, 1)
    w = n + (1 if pos_ids is not None else 0)
    ws_bytes, ws_alloc = _workspace_bytes('rsa_scatter_rows_sorted_workspace_bytes', M, n, int(n_items))
    bufs = carve(neg_ids.device, [('ws', (ws_alloc,), torch.uint8)] + ([('solo', (M, w), torch.uint8)] if want_solo else []))
    solo, ws = bufs.get('solo'), bufs['ws']                     # solo None: sort only, nothing flagged
    a = nat.RowsUpdateArgs()
    a.pos_ids, a.neg_ids, a.n_queries, a.num_neg, a.n_items, a.pad_row = ptr(pos_ids), ptr(neg_ids), M, n, int(n_items), int(pad_row)
    a.solo, a.workspace, a.workspace_bytes = ptr(solo), ptr(ws), ws_bytes
    _launch('rsa_sort_step_elements', ctypes.byref(a))
    return solo, ws


def _rows_update(who, target, query, dneg, *, neg_ids=None, workspace=None, n_queries=None, num_neg=None, rule=None,
                 query_index=None, pos_ids=None, dpos=None, upstream=None, pad_row=0):
    """The one body of the rows-update wrappers.  No ``workspace``: sort + apply over ``neg_ids`` / ``pos_ids``
    (rsa_rows_update_sorted; queries and negatives per query derived here, the workspace allocated here).  ``workspace`` given:
    the apply pass over the pairs ``sort_step_elements`` left in it (rsa_rows_update_presorted).  ``rule``: the optimizer applied to
    the touched rows (``_rule_fields``); None: plain accumulate."""
    presorted = workspace is not None
    target = _need(target, torch.float32, 'weight' if rule else 'target')
    query = _need(query, torch.float32, 'query')
    neg_ids = None if presorted else _need(neg_ids, torch.int64, 'neg_ids')
    dneg = _need(dneg, torch.float32, 'dneg')
    query_index = _need_opt(query_index, torch.int64, 'query_index')
    pos_ids = _need_opt(pos_ids, torch.int64, 'pos_ids')
    dpos = _need_opt(dpos, torch.float32, 'dpos')
    upstream = _need_opt(upstream, torch.float32, 'upstream')
    if presorted:
        M, n = n_queries, num_neg
    else:
        M = query_index.numel() if query_index is not None else query.shape[0]
        if M == 0:
            return target
        n = neg_ids.numel() // M
    a = _rows_update_args(target, query, query_index, M, n, dpos, dneg, upstream, pad_row)
    if rule:
        _rule_fields(a, rule, who)
    if presorted:
        a.has_pos, a.workspace_bytes = int(dpos is not None), workspace.numel()
    else:
        a.pos_ids, a.neg_ids = ptr(pos_ids), ptr(neg_ids)
        workspace, a.workspace_bytes = _workspace(target.device, 'rsa_scatter_rows_sorted_workspace_bytes', M, n, target.shape[0])
    a.workspace = ptr(workspace)
    _launch('rsa_rows_update_presorted' if presorted else 'rsa_rows_update_sorted', ctypes.byref(a))
    return target


@_on_device
def scatter_rows_sorted(target, query, neg_ids, dneg, *, query_index=None, pos_ids=None, dpos=None, upstream=None,
                        pad_row=0):
    """rsa_rows_update_sorted: target[id] += upstream * sum_e d_e * query[qrow_e], sorted by id, no atomics.
    ``target``: [n_items, d] (a zeroed dense gradient, or the weight table with upstream = -lr)."""
    return _rows_update('scatter_rows_sorted', target, query, dneg, neg_ids=neg_ids, query_index=query_index, pos_ids=pos_ids,
                        dpos=dpos, upstream=upstream, pad_row=pad_row)


@_on_device
def adam_rows_sorted(weight, exp_avg, exp_avg_sq, query, neg_ids, dneg, *, lr, betas=(0.9, 0.999), eps=1e-8, step=1,
                     query_index=None, pos_ids=None, dpos=None, upstream=None, pad_row=0):
    """rsa_rows_update_sorted with the lazy-Adam state: lazy Adam (torch.optim.SparseAdam's rule) on the rows touched by the step, from the
    factored gradient (ids, coefficients, query rows) -- no gradient tensor."""
    return _rows_update('adam_rows_sorted', weight, query, dneg, neg_ids=neg_ids, rule=('adam', exp_avg, exp_avg_sq, lr, betas, eps, step),
                        query_index=query_index, pos_ids=pos_ids, dpos=dpos, upstream=upstream, pad_row=pad_row)


@_on_device
def scatter_rows_presorted(target, query, workspace, n_queries, num_neg, dneg, *, query_index=None, dpos=None, upstream=None,
                           pad_row=0):
    """rsa_rows_update_presorted: the apply pass of scatter_rows_sorted over the pairs ``sort_step_elements`` left in
    ``workspace`` (elements flagged solo there are skipped: the forward has applied them)."""
    return _rows_update('scatter_rows_presorted', target, query, dneg, workspace=workspace, n_queries=n_queries, num_neg=num_neg,
                        query_index=query_index, dpos=dpos, upstream=upstream, pad_row=pad_row)


@_on_device
def adam_rows_presorted(weight, exp_avg, exp_avg_sq, query, workspace, n_queries, num_neg, dneg, *, lr, betas=(0.9, 0.999),
                        eps=1e-8, step=1, query_index=None, dpos=None, upstream=None, pad_row=0):
    """rsa_rows_update_presorted with the lazy-Adam state: the apply pass of adam_rows_sorted over the pairs ``sort_step_elements(want_solo=False)``
    left in ``workspace``."""
    return _rows_update('adam_rows_presorted', weight, query, dneg, workspace=workspace, n_queries=n_queries, num_neg=num_neg,
                        rule=('adam', exp_avg, exp_avg_sq, lr, betas, eps, step), query_index=query_index, dpos=dpos, upstream=upstream,
                        pad_row=pad_row)


@_on_device
def adagrad_rows_sorted(weight, state_sum, query, neg_ids, dneg, *, lr, lr_decay=0.0, eps=1e-10, step=1, query_index=None,
                        pos_ids=None, dpos=None, upstream=None, pad_row=0):
    """rsa_rows_update_sorted with rule = RSA_ROWS_ADAGRAD: torch.optim.Adagrad's update (state_sum += g^2; weight -= lr / (1 +
    (step - 1) lr_decay) * g / (sqrt(state_sum) + eps)) on the rows touched by the step, from the factored gradient -- no gradient
    tensor.  A row outside the step has a zero gradient, which the dense rule leaves as it is: this IS torch.optim.Adagrad."""
    return _rows_update('adagrad_rows_sorted', weight, query, dneg, neg_ids=neg_ids, rule=('adagrad', state_sum, lr, lr_decay, eps, step),
                        query_index=query_index, pos_ids=pos_ids, dpos=dpos, upstream=upstream, pad_row=pad_row)


@_on_device
def adagrad_rows_presorted(weight, state_sum, query, workspace, n_queries, num_neg, dneg, *, lr, lr_decay=0.0, eps=1e-10, step=1,
                           query_index=None, dpos=None, upstream=None, pad_row=0):
    """rsa_rows_update_presorted with rule = RSA_ROWS_ADAGRAD: the apply pass of adagrad_rows_sorted over the pairs
    ``sort_step_elements(want_solo=False)`` left in ``workspace``."""
    return _rows_update('adagrad_rows_presorted', weight, query, dneg, workspace=workspace, n_queries=n_queries, num_neg=num_neg,
                        rule=('adagrad', state_sum, lr, lr_decay, eps, step), query_index=query_index, dpos=dpos, upstream=upstream,
                        pad_row=pad_row)


# ------------------------------------------------------------------ full catalog
@_on_device
def row_lse(x, want_softmax=False, scale=1.0):
    x = _need(x, torch.float32, 'x')
    M, n = x.shape
    lse = torch.empty(M, dtype=torch.float32, device=x.device)
    sm = torch.empty_like(x) if want_softmax else None
    _launch('rsa_row_lse', ptr(x), M, n, ptr(lse), ptr(sm), float(scale))
    return lse, sm


def _pad_k(*mats):
    """The MFMA kernel is built for d in {32, 64, 128}: zero-pad the k dimension of ``mats`` [.., d] at smaller dims (a copy --
    only for unusual dims; the dot products are unchanged) -> (*mats, the dim they have now).  d > 128 is handled by the
    callers (k split into chunks)."""
    dim = mats[0].shape[1]
    if dim in (32, 64, 128):
        return (*mats, dim)
    if dim > 128:
        raise NotImplementedError(f'one MFMA pass covers embed_dim <= 128, got {dim} (ops.fullscore splits it)')
    pad = (32 if dim < 32 else 64 if dim < 64 else 128) - dim
    return (*(torch.nn.functional.pad(m, (0, pad)) for m in mats), dim + pad)


def _unpad(res, d_in, out=None):
    """The other end of ``_pad_k``: ``res`` [.., dim] of a launch at the padded k -> its first ``d_in`` columns, copied into ``out``
    when given.  Stock dims: no copy -- ``res`` itself (``out`` when the launch wrote straight into it)."""
    if res.shape[1] == d_in:
        return res if out is None else out
    res = res[:, :d_in]
    return res.contiguous() if out is None else out.copy_(res)


@_on_device
def row_sqnorm(table, score_mode, pad=0):
    """rsa_row_sqnorm: per-row operand of the cosine (1 / ||row||) or Euclidean (||row||^2) full-catalog scores.
    ``pad`` extra (zero) entries are appended (the MFMA kernel reads up to a tile past the last item)."""
    table = _need(table, torch.float32, 'table')
    n, d = table.shape
    out = torch.zeros(n + pad, dtype=torch.float32, device=table.device) if pad else \
        torch.empty(n, dtype=torch.float32, device=table.device)
    _launch('rsa_row_sqnorm', ptr(table), n, d, int(score_mode), ptr(out))
    return out


FULLSCORE_MAX_K = 1024


@_on_device
def fullscore(item_table, query, *, want_scores=False, want_lse=False, k=0, items_without_pad=False, score_mode=0):
    """rsa_fullscore: scores of query [B,d] against rows 1.. of item_table [N,d].
    ``items_without_pad``: ``item_table`` is the reference's ``item_vector`` (= weight[1:], no padding
    row); the kernel never touches row 0, so the base pointer is simply moved one row back.
    ``score_mode``: rsa_score_mode (inner product / cosine / Euclidean, scorer.py:5-34).
    Shapes outside the single-pass kernel are composed from it: embed_dim > 128 accumulates materialised scores
    over 128-wide slices of k; top-k beyond 1024 runs on materialised scores (torch.topk)."""
    item_table = _need(item_table, torch.float32, 'item_table')
    query = _need(query, torch.float32, 'query')
    score_mode = _score_mode(score_mode)
    dim0 = item_table.shape[1]
    if dim0 > 128 or k > FULLSCORE_MAX_K:
        return _fullscore_composed(item_table, query, want_scores, want_lse, k, items_without_pad, score_mode)
    dev = item_table.device
    n_items, dim = item_table.shape
    ia = qa = None
    if score_mode != nat.SCORE_IP:       # per-item / per-query operands from the UNPADDED rows
        rows = item_table if items_without_pad else item_table[1:]
        ia = row_sqnorm(rows, score_mode, pad=64)
        qa = row_sqnorm(query, score_mode)
    item_table, query, dim = _pad_k(item_table, query)
    table_ptr = ptr(item_table)
    if items_without_pad:
        n_items += 1
        table_ptr = ctypes.c_void_p(item_table.data_ptr() - dim * 4)
    B = query.shape[0]
    scores = torch.empty(B, n_items - 1, dtype=torch.float32, device=dev) if want_scores else None
    lse = torch.empty(B, dtype=torch.float32, device=dev) if want_lse else None
    tv = torch.empty(B, k, dtype=torch.float32, device=dev) if k else None
    ti = torch.empty(B, k, dtype=torch.int64, device=dev) if k else None
    a = nat.FullscoreArgs()
    a.item_table, a.n_items, a.dim, a.score_mode = table_ptr, n_items, dim, score_mode
    a.query, a.n_query, a.k = ptr(query), B, int(k)
    a.scores, a.lse, a.topk_val, a.topk_idx = ptr(scores), ptr(lse), ptr(tv), ptr(ti)
    a.item_aux, a.query_aux = ptr(ia), ptr(qa)
    ws, a.workspace_bytes = _workspace(dev, 'rsa_fullscore_workspace_bytes', B, n_items, int(k))
    a.workspace = ptr(ws)
    _launch('rsa_fullscore', ctypes.byref(a))
    return scores, lse, tv, ti


def _fullscore_composed(item_table, query, want_scores, want_lse, k, items_without_pad, score_mode):
    """embed_dim > 128 and / or k > 1024 (the reference has neither limit, scorer.py:16, baseretriever.py:385):
    inner products accumulated over <= 128-wide column slices through the MFMA kernel into one materialised
    [B, N-1] matrix, the cosine / Euclidean operands applied to it, then logsumexp (rsa_row_lse) and top-k
    (rsa_row_topk up to 1024, torch.topk beyond)."""
    rows = item_table if items_without_pad else item_table[1:]
    d = rows.shape[1]
    scores = None
    for c0 in range(0, d, 128):
        part = fullscore(rows[:, c0:c0 + 128].contiguous(), query[:, c0:c0 + 128].contiguous(), want_scores=True,
                         items_without_pad=True)[0]
        scores = part if scores is None else scores.add_(part)
    if score_mode == nat.SCORE_COS:
        scores.mul_(row_sqnorm(rows, score_mode)).mul_(row_sqnorm(query, score_mode).view(-1, 1))
    elif score_mode == nat.SCORE_EUC:
        scores.mul_(2.0).sub_(row_sqnorm(rows, score_mode)).sub_(row_sqnorm(query, score_mode).view(-1, 1))
    lse = row_lse(scores)[0] if want_lse else None
    tv = ti = None
    if k:
        if k <= FULLSCORE_MAX_K:
            tv, ti = row_topk(scores, k)
        else:
            tv, ti = torch.topk(scores, k, dim=-1)
        ti = ti + 1
    return (scores if want_scores else None), lse, tv, ti


@_on_device
def fullscore_softmax(item_table, query, lse, row_scale=None, want_query_grad=False, want_probs=True):
    """rsa_fullscore_softmax: probs[b, i-1] = row_scale[b] * exp(<query_b, item_i> - lse[b]) over rows 1.. of
    ``item_table`` (dims in {32, 64, 128}).  ``want_query_grad``: -> (probs, probs @ item_table[1:]), the product
    accumulated on the matrix cores in the same pass (rsa_fullscore_softmax_dq); with ``want_probs=False`` the [B, N-1]
    matrix is neither allocated nor written (-> (None, query_grad))."""
    item_table = _need(item_table, torch.float32, 'item_table')
    query = _need(query, torch.float32, 'query')
    lse = _need(lse, torch.float32, 'lse')
    d_in = query.shape[1]
    item_table, query, dim = _pad_k(item_table, query)
    n_items = item_table.shape[0]
    B = query.shape[0]
    if not want_probs and not want_query_grad:
        raise ValueError('fullscore_softmax: nothing to compute (want_probs=False needs want_query_grad=True)')
    probs = torch.empty(B, n_items - 1, dtype=torch.float32, device=item_table.device) if want_probs else None
    if want_query_grad:
        qgrad = torch.empty(B, dim, dtype=torch.float32, device=item_table.device)
        ws, ws_bytes = _workspace(item_table.device, 'rsa_fullscore_softmax_dq_workspace_bytes', B, n_items, dim)
        _launch('rsa_fullscore_softmax_dq', ptr(item_table), n_items, dim, ptr(query), B, ptr(lse),
                ptr(_need_opt(row_scale, torch.float32, 'row_scale')), ptr(probs), ptr(qgrad), ptr(ws), ws_bytes)
        return probs, _unpad(qgrad, d_in)
    _launch('rsa_fullscore_softmax', ptr(item_table), n_items, dim, ptr(query), B, ptr(lse),
            ptr(_need_opt(row_scale, torch.float32, 'row_scale')), ptr(probs))
    return probs


@_on_device
def fullscore_lse_grad(item_table, query):
    """rsa_fullscore_lse_grad: (lse [B], d lse/d query [B, d] = softmax @ item_table[1:]) in ONE pass over the catalog (the flash
    forward of the full softmax).  embed_dim <= 128."""
    item_table = _need(item_table, torch.float32, 'item_table')
    query = _need(query, torch.float32, 'query')
    d_in = query.shape[1]
    tab, q, dim = _pad_k(item_table, query)
    n_items, B, dev = tab.shape[0], q.shape[0], tab.device
    lse = torch.empty(B, dtype=torch.float32, device=dev)
    gq = torch.empty(B, dim, dtype=torch.float32, device=dev)
    ws, ws_bytes = _workspace(dev, 'rsa_fullscore_lse_grad_workspace_bytes', B, n_items, dim)
    _launch('rsa_fullscore_lse_grad', ptr(tab), n_items, dim, ptr(q), B, ptr(lse), ptr(gq), ptr(ws), ws_bytes)
    return lse, _unpad(gq, d_in)


@_on_device
def fullscore_softmax_dw(item_table, query, lse, row_scale=None, out=None):
    """rsa_fullscore_softmax_dw: d/d item_table of sum_b row_scale[b] * logsumexp_i <query_b, item_i> (rows 1.. of the table; row
    0 of the result is zero) with the softmax tile recomputed on the matrix cores -- no [B, N] matrix.  embed_dim <= 128."""
    item_table = _need(item_table, torch.float32, 'item_table')
    query = _need(query, torch.float32, 'query')
    lse = _need(lse, torch.float32, 'lse')
    d_in = item_table.shape[1]
    tab, q, dim = _pad_k(item_table, query)
    n_items, B = tab.shape[0], q.shape[0]
    res = out if dim == d_in and out is not None else torch.empty(n_items, dim, dtype=torch.float32, device=tab.device)
    res = _need(res, torch.float32, 'out')
    if res.shape != (n_items, dim):
        raise ValueError(f'fullscore_softmax_dw: out must be [{n_items}, {dim}]')
    _launch('rsa_fullscore_softmax_dw', ptr(tab), n_items, dim, ptr(q), B, ptr(lse),
            ptr(_need_opt(row_scale, torch.float32, 'row_scale')), ptr(res))
    return _unpad(res, d_in, out)


@_on_device
def probs_t_query(probs, query, out=None):
    """rsa_probs_t_query: ``probs.t() @ query`` ([B, n] x [B, d] -> [n, d]) on the fp32 matrix cores, item-stationary -- the
    d/d items GEMM of the full-softmax backward.  d in {32, 64, 128} (other dims: zero-padded columns, sliced off)."""
    probs = _need(probs, torch.float32, 'probs')
    query = _need(query, torch.float32, 'query')
    B, n = probs.shape
    d = query.shape[1]
    if query.shape[0] != B:
        raise ValueError('probs_t_query: probs [B, n] and query [B, d] must share B')
    if d > 128:
        raise NotImplementedError('probs_t_query: embed_dim <= 128')
    q, dim = _pad_k(query)
    if out is None or dim != d:
        res = torch.empty(n, dim, dtype=torch.float32, device=probs.device)
    elif tuple(out.shape) != (n, d) or not out.is_contiguous() or out.dtype != torch.float32:
        raise ValueError('probs_t_query: out must be a contiguous fp32 [n, d] tensor')
    else:
        res = out
    _launch('rsa_probs_t_query', ptr(probs), B, n, probs.stride(0), ptr(q), dim, ptr(res))
    return _unpad(res, d, out)


SOFTMAX_SAMPLE_MAX_DIM = 128


def softmax_sample_block():
    """Items per block of the two-level draw (the library's compile-time G): ``mass`` / ``cum`` hold ceil((N - 1) / G) columns."""
    return int(nat.lib().rsa_softmax_sample_block())


def _softmax_sample_args(item_table, query, num_neg, t, score_mode, pos_ids, user_hist, want_tables, items_without_pad, who):
    item_table = _need(item_table, torch.float32, 'item_table')
    query = _need(query, torch.float32, 'query')
    if item_table.dim() != 2 or query.dim() != 2 or query.shape[1] != item_table.shape[1]:
        raise ValueError(f'{who}: item_table must be [N, d] and query [M, d], got {tuple(item_table.shape)} and {tuple(query.shape)}')
    d = item_table.shape[1]
    if d > SOFTMAX_SAMPLE_MAX_DIM or d % 4:
        raise NotImplementedError(f'{who}: embed_dim must be a multiple of 4 and at most {SOFTMAX_SAMPLE_MAX_DIM} '
                                  f'(one MFMA pass over k), got {d}')
    if not float(t) > 0.0:
        raise ValueError(f'{who}: the temperature t must be positive, got {t}')
    n = int(num_neg)
    if n < 0:
        raise ValueError(f'{who}: num_neg must not be negative')
    score_mode = _score_mode(score_mode)
    n_items = item_table.shape[0] + (1 if items_without_pad else 0)
    if n_items < 2:
        raise ValueError(f'{who}: the catalog is empty')
    dev, M = query.device, query.shape[0]
    ia = qa = None
    if score_mode != nat.SCORE_IP:       # per-item / per-query operands from the UNPADDED rows
        ia = row_sqnorm(item_table if items_without_pad else item_table[1:], score_mode, pad=64)
        qa = row_sqnorm(query, score_mode)
    item_table, query, dim = _pad_k(item_table, query)
    # (rows without the padding row: the kernels never touch row 0, so the base pointer is moved one row back)
    table_ptr = ctypes.c_void_p(item_table.data_ptr() - dim * 4) if items_without_pad else ptr(item_table)
    out = dict(neg_ids=torch.empty(M, n, dtype=torch.int64, device=dev), neg_logp=torch.empty(M, n, dtype=torch.float32, device=dev),
               pos_logp=None, lse=torch.empty(M, dtype=torch.float32, device=dev))
    a = nat.SoftmaxSampleArgs()
    a.item_table, a.n_items, a.dim, a.score_mode, a.inv_t = table_ptr, n_items, dim, score_mode, 1.0 / float(t)
    a.query, a.n_query, a.num_neg = ptr(query), M, n
    a.item_aux, a.query_aux, a.lse = ptr(ia), ptr(qa), ptr(out['lse'])
    if n:
        a.neg_ids, a.neg_logp = ptr(out['neg_ids']), ptr(out['neg_logp'])
    if pos_ids is not None:
        pos_ids = _need(pos_ids, torch.int64, 'pos_ids')
        if pos_ids.dim() != 2 or pos_ids.shape[0] != M:
            raise ValueError(f'{who}: pos_ids must be [M, T]')
        out['pos_logp'] = torch.empty(pos_ids.shape, dtype=torch.float32, device=dev)
        a.n_pos, a.pos_ids, a.pos_logp = pos_ids.shape[1], ptr(pos_ids), ptr(out['pos_logp'])
    if user_hist is not None:
        user_hist = _need(user_hist, torch.int64, 'user_hist')
        if user_hist.dim() != 2 or user_hist.shape[0] != M:
            raise ValueError(f'{who}: user_hist must be [M, L]')
        if user_hist.shape[1]:
            a.hist_len, a.user_hist = user_hist.shape[1], ptr(user_hist)
    if want_tables:
        G = softmax_sample_block()
        nb = (n_items - 1 + G - 1) // G
        out['mass'] = torch.empty(M, nb, dtype=torch.float32, device=dev)
        out['cum'] = torch.empty(M, nb, dtype=torch.float32, device=dev)
        a.mass, a.cum = ptr(out['mass']), ptr(out['cum'])
    ws, a.workspace_bytes = _workspace(dev, 'rsa_softmax_sample_workspace_bytes', M, n_items)
    a.workspace = ptr(ws)
    return a, out, (item_table, query, ia, qa, pos_ids, user_hist, ws)


@_on_device
def softmax_sample(item_table, query, num_neg, *, t=1.0, score_mode=0, pos_ids=None, user_hist=None, generator=None, want_u=False,
                   want_tables=False, items_without_pad=False):
    """rsa_softmax_sample: ``num_neg`` ids per query, with replacement, from softmax(score(query, .) / t) over rows 1.. of
    ``item_table`` [N, d] -- the draw of ``sampling(method='brute')`` without the [M, N] matrix (two-level inverse CDF over item
    blocks, include/recstudio_amd.h).  ``user_hist`` [M, L] (0-padded): those ids are never drawn.  ``pos_ids`` [M, T]: also their
    log-probabilities (-inf for the padding id).  The uniforms are those of ``torch.rand(M, num_neg, 2)`` on the device generator
    (advanced as that call would); the ids are NOT torch.multinomial's for the same seed.  ``items_without_pad``: ``item_table`` is
    weight[1:].  -> dict(neg_ids [M, n] int64, neg_logp [M, n] = score / t - lse (the masked row is not renormalised), pos_logp
    [M, T] or None, lse [M], u [M, n, 2] with ``want_u``, mass / cum [M, ceil((N - 1) / G)] with ``want_tables``)."""
    a, out, keep = _softmax_sample_args(item_table, query, num_neg, t, score_mode, pos_ids, user_hist, want_tables,
                                        items_without_pad, 'softmax_sample')
    numel = a.n_query * a.num_neg * 2
    if numel:
        pc = rng.reserve(numel, 4, query.device, generator)
        a.seed, a.offset, a.grid_threads, a.elem_base = pc.seed, pc.offset, pc.grid_threads, pc.elem_base
    if want_u:
        out['u'] = torch.empty(a.n_query, a.num_neg, 2, dtype=torch.float32, device=query.device)
        a.u_out = ptr(out['u'])
    _launch('rsa_softmax_sample', ctypes.byref(a))
    return out


@_on_device
def softmax_lookup(item_table, query, u, *, t=1.0, score_mode=0, pos_ids=None, user_hist=None, want_tables=False,
                   items_without_pad=False):
    """rsa_softmax_lookup: the draw of ``softmax_sample`` for caller-supplied uniforms ``u`` [M, n, 2]."""
    u = _need(u, torch.float32, 'u')
    if u.dim() != 3 or u.shape[0] != query.shape[0] or u.shape[2] != 2:
        raise ValueError('softmax_lookup: u must be [M, n, 2]')
    a, out, keep = _softmax_sample_args(item_table, query, u.shape[1], t, score_mode, pos_ids, user_hist, want_tables,
                                        items_without_pad, 'softmax_lookup')
    a.u_in = ptr(u)
    _launch('rsa_softmax_lookup', ctypes.byref(a))
    return out


@_on_device
def topk_mask_history(cand_val, cand_idx, user_hist, k):
    """baseretriever.py:386-392 on sorted candidates: drop history items, keep the k best."""
    cand_val = _need(cand_val, torch.float32, 'cand_val')
    cand_idx = _need(cand_idx, torch.int64, 'cand_idx')
    user_hist = _need(user_hist, torch.int64, 'user_hist')
    B, kc = cand_val.shape
    out_v = torch.empty(B, k, dtype=torch.float32, device=cand_val.device)
    out_i = torch.empty(B, k, dtype=torch.int64, device=cand_val.device)
    _launch('rsa_topk_mask_history', ptr(cand_val), ptr(cand_idx), kc, ptr(user_hist), user_hist.shape[1], B, int(k),
            ptr(out_v), ptr(out_i))
    return out_v, out_i


@_on_device
def row_topk(values, k):
    """torch.topk(values, k) over the last dim (k <= 1024) -> (values, column indices)."""
    values = _need(values, torch.float32, 'values')
    lead, n = values.shape[:-1], values.shape[-1]
    v2 = values.reshape(-1, n)
    out_v = torch.empty(v2.shape[0], k, dtype=torch.float32, device=values.device)
    out_i = torch.empty(v2.shape[0], k, dtype=torch.int64, device=values.device)
    _launch('rsa_row_topk', ptr(v2), v2.shape[0], n, int(k), ptr(out_v), ptr(out_i))
    return out_v.view(*lead, k), out_i.view(*lead, k)


@_on_device
def rng_advance(offset_dev, increment):
    """*offset_dev += increment on the stream (rsa_rng_advance): the device copy of the generator offset."""
    _launch('rsa_rng_advance', ptr(offset_dev), int(increment))


# ------------------------------------------------------------------ sparse x dense (graph propagation)
SPMM_MAX_DIM = 256
# Rows longer than this are cut into pieces summed by separate waves (include/recstudio_amd.h, "THE PLAN").  Measured on the
# Zipf graph of tools/bench_lightgcn.py: 128 / 256 / 512 / 1024 / 2048 edges -> 8.5 / 6.1 / 4.9 / 4.3 / 4.0 ms per layer.
SPMM_CHUNK = 2048


class SpmmPlan:
    """The chunk list of one CSR matrix for ``spmm_csr`` (``spmm_plan`` builds it, once per matrix): ``table`` is the int64 array
    rsa_spmm_args.plan describes -- split_row [n_split], split_part [n_split + 1], part_row [n_parts], part_edge [n_parts] --, and
    the partials workspace [n_parts, d] is kept here between calls."""

    def __init__(self, chunk, n_rows, nnz, n_split, n_parts, table):
        self.chunk, self.n_rows, self.nnz, self.n_split, self.n_parts, self.table = chunk, n_rows, nnz, n_split, n_parts, table
        self._partials = None

    def to(self, device):
        if self.table.device != torch.device(device):
            self.table, self._partials = self.table.to(device), None
        return self

    def split_row(self):
        return self.table[:self.n_split]

    def split_part(self):
        return self.table[self.n_split:2 * self.n_split + 1]

    def part_row(self):
        return self.table[2 * self.n_split + 1:2 * self.n_split + 1 + self.n_parts]

    def part_edge(self):
        return self.table[2 * self.n_split + 1 + self.n_parts:]

    def partials(self, dim, device):
        need = self.n_parts * dim
        if self._partials is None or self._partials.numel() < need or self._partials.device != device:
            self._partials = torch.empty(max(need, 4), dtype=torch.float32, device=device)
        return self._partials


def spmm_plan(indptr, chunk=SPMM_CHUNK):
    """The plan of ``spmm_csr`` for the matrix whose row pointer is ``indptr`` int64 [R + 1] (host or device; the plan lives where
    ``indptr`` does): rows of more than ``chunk`` edges are cut into pieces of ``chunk`` consecutive edges."""
    if not isinstance(indptr, torch.Tensor) or indptr.dtype != torch.int64 or indptr.dim() != 1 or indptr.numel() < 1:
        raise TypeError('spmm_plan: indptr must be an int64 tensor [R + 1]')
    chunk = int(chunk)
    if chunk < 1:
        raise ValueError(f'spmm_plan: chunk must be at least 1, got {chunk}')
    deg = indptr[1:] - indptr[:-1]
    if deg.numel() and int(deg.min()) < 0:
        raise ValueError('spmm_plan: indptr must not decrease')
    split = (deg > chunk).nonzero().view(-1)
    pieces = (deg[split] + chunk - 1) // chunk
    split_part = torch.cat([pieces.new_zeros(1), torch.cumsum(pieces, 0)])
    n_split, n_parts = int(split.numel()), int(split_part[-1])
    owner = torch.repeat_interleave(torch.arange(n_split, device=indptr.device), pieces)
    part_row = split[owner]
    part_edge = indptr[part_row] + (torch.arange(n_parts, device=indptr.device) - split_part[owner]) * chunk
    table = torch.cat([split, split_part, part_row, part_edge]).contiguous()
    return SpmmPlan(chunk, int(deg.numel()), int(indptr[-1]) if indptr.numel() else 0, n_split, n_parts, table)


@_on_device
def spmm_csr(indptr, indices, values, x, *, plan, row_scale=None, y=None, acc=None, acc_scale=1.0, acc_out=None,
             noise=None, noise_eps=0.0, noise_out=None):
    """rsa_spmm_csr: ``y[r] = row_scale[r] * sum_e values[e] * x[indices[e]]`` over the edges ``[indptr[r], indptr[r + 1])`` of
    row r -- ``indptr`` int64 [R + 1], ``indices`` int32 [nnz], ``values`` fp32 [nnz] or None (all ones), ``x`` fp32 [C, d] with d
    a multiple of 4 and at most 256, ``row_scale`` fp32 [R] or None, ``plan`` = ``spmm_plan(indptr)``.  No atomics; bit-equal
    from run to run.
    ``acc`` fp32 [R, d]: also ``acc <- acc_scale * (acc + y)`` IN PLACE, in the same pass (the running layer sum of LightGCN; the
    last layer's ``acc_scale = 1 / (L + 1)`` makes it the mean).  With ``acc`` and without ``y`` the product itself is not written.
    ``acc_out`` fp32 [R, d] (with ``acc``): the accumulation is written THERE and ``acc`` is only read -- one step of a Horner
    recurrence ``h' = acc_scale * (g + A h)`` with g = ``acc``, h = ``x``, h' = ``acc_out``.
    Without ``acc``, ``y`` None allocates the result.  Returns ``y`` when it was written, else ``acc_out`` / ``acc``.
    ``noise`` (a ``rng.PhiloxCall`` reserved for ONE ``torch.rand`` call over ``R * d`` outputs) with ``noise_eps != 0``: SimGCL's
    perturbed layer.  Row r's sum after ``row_scale``, s, becomes ``s + sign(s) * u / max(||u||_2, 1e-12) * noise_eps`` before
    ``y`` and the accumulation see it, ``u`` = elements ``[r d, (r + 1) d)`` of that call (``torch.sign``: a zero stays zero, so
    rows without edges stay 0).  ``noise_out`` fp32 [R, d]: receives the uniforms.  They are bit-equal to ``torch.rand_like`` of
    an [R, d] tensor in the generator state ``noise`` was reserved in while ``R * d < 2**31``; torch splits larger calls in two,
    here a larger table still draws the elements of one call indexed with 64 bits.  ``noise_eps == 0`` is the plain product and
    takes neither ``noise`` nor ``noise_out``."""
    indptr = _need(indptr, torch.int64, 'indptr')
    indices = _need(indices, torch.int32, 'indices')
    values = _need_opt(values, torch.float32, 'values')
    x = _need(x, torch.float32, 'x')
    row_scale = _need_opt(row_scale, torch.float32, 'row_scale')
    if not isinstance(plan, SpmmPlan):
        raise TypeError('spmm_csr: plan must come from spmm_plan(indptr)')
    R, nnz = indptr.numel() - 1, indices.numel()
    if x.dim() != 2 or x.shape[1] % 4 or not 4 <= x.shape[1] <= SPMM_MAX_DIM:
        raise ValueError(f'spmm_csr: x must be [C, d] with d a multiple of 4 and at most {SPMM_MAX_DIM}, got {tuple(x.shape)}')
    C, d = x.shape
    if plan.n_rows != R or plan.nnz != nnz:
        raise ValueError(f'spmm_csr: the plan was built for {plan.n_rows} rows / {plan.nnz} edges, the matrix has {R} / {nnz}')
    if values is not None and values.numel() != nnz:
        raise ValueError('spmm_csr: values must hold one weight per edge')
    if row_scale is not None and row_scale.numel() != R:
        raise ValueError('spmm_csr: row_scale must hold one factor per row')
    dev = x.device
    plan.to(dev)
    if acc_out is not None and acc is None:
        raise ValueError('spmm_csr: acc_out without acc')
    for name, t in (('y', y), ('acc', acc), ('acc_out', acc_out)):
        if t is not None:
            _need_view(t, torch.float32, name)
            if tuple(t.shape) != (R, d) or not t.is_contiguous():
                raise ValueError(f'spmm_csr: {name} must be a contiguous [{R}, {d}] tensor')
            # (acc may be x when the sum goes to acc_out: it is then only read)
            if t.data_ptr() == x.data_ptr() and t.numel() and not (name == 'acc' and acc_out is not None):
                raise ValueError(f'spmm_csr: {name} must not alias x')
    noise_eps = float(noise_eps)
    if not math.isfinite(noise_eps):
        raise ValueError(f'spmm_csr: noise_eps must be finite, got {noise_eps}')
    if noise_eps != 0.0:
        if not isinstance(noise, rng.PhiloxCall):
            raise TypeError('spmm_csr: noise_eps needs noise, a rng.PhiloxCall (rng.reserve(R * d, 4, device))')
        if noise.grid_threads <= 0 or noise.grid_threads % rng.BLOCK or noise.offset % 4:
            raise ValueError(f'spmm_csr: bad philox state for the noise: {noise}')
    elif noise is not None or noise_out is not None:
        raise ValueError('spmm_csr: noise / noise_out without noise_eps')
    if noise_out is not None:
        _need_view(noise_out, torch.float32, 'noise_out')
        if tuple(noise_out.shape) != (R, d) or not noise_out.is_contiguous() or noise_out.data_ptr() % 16:
            raise ValueError(f'spmm_csr: noise_out must be a contiguous, 16-byte aligned [{R}, {d}] tensor')
    if y is None and acc is None:
        y = torch.empty(R, d, dtype=torch.float32, device=dev)
    partials = plan.partials(d, dev) if plan.n_parts else None
    a = nat.SpmmArgs()
    a.indptr, a.indices, a.values = ptr(indptr), ptr(indices), ptr(values)
    a.n_rows, a.n_cols, a.nnz, a.dim = R, C, nnz, d
    a.x, a.row_scale, a.y = ptr(x), ptr(row_scale), ptr(y)
    a.acc_in, a.acc_out, a.acc_scale = ptr(acc), ptr(acc if acc_out is None else acc_out), float(acc_scale)
    a.chunk, a.n_split, a.n_parts = plan.chunk, plan.n_split, plan.n_parts
    if plan.n_split:
        a.plan, a.plan_len = ptr(plan.table), plan.table.numel()
        a.partials, a.partials_bytes = ptr(partials), partials.numel() * 4
    if noise_eps != 0.0:
        a.noise_eps, a.noise_u = noise_eps, ptr(noise_out)
        a.noise_seed, a.noise_offset, a.noise_grid_threads, a.noise_elem_base = noise.seed, noise.offset, noise.grid_threads, noise.elem_base
    _launch('rsa_spmm_csr', ctypes.byref(a))
    return y if y is not None else (acc if acc_out is None else acc_out)


GRAPH_DROPOUT_LONG_ROW = 2048      # rows longer than this are counted by several waves (rsa_graphaug.hip, "WORK ITEMS")


@_on_device
def graph_dropout(indptr, indices, rev, keep_prob, *, node_drop=None, generator=None, want_keep=False, long_row=None):
    """rsa_graph_dropout: thin the symmetric CSR graph (``indptr`` int64 [n + 1], ``indices`` int32 [nnz], ``rev`` int64 [nnz] =
    the position of every edge's reverse edge) and renormalise it by the surviving degrees.  Edge e is kept iff
    ``floor(u_e + keep_prob) != 0`` for ``u = torch.rand(nnz, device=...)`` on the device generator (advanced as that call would;
    not touched when ``keep_prob >= 1``) and, with ``node_drop`` (bool / uint8 [n]), neither of its ends is flagged.
    -> ``(values, t_values, in_deg, out_deg[, keep])``: fp32 [nnz] weights ``in_deg(dst)^-1/2 out_deg(src)^-1/2`` of the kept
    edges (0 on the dropped ones) and the same for the transposed thinned matrix (``t_values == values[rev]``), both in the layout
    -- and for the ``spmm_plan`` -- of the base graph; int32 [n] degrees; ``keep`` uint8 [nnz] with ``want_keep``.  ``long_row``
    (default 2048, at least 128): rows longer than this are counted by the waves of the edge windows they reach into.  No float
    atomics; bit-equal from run to run."""
    indptr = _need(indptr, torch.int64, 'indptr')
    indices = _need(indices, torch.int32, 'indices')
    rev = _need(rev, torch.int64, 'rev')
    n, nnz = indptr.numel() - 1, indices.numel()
    if indptr.dim() != 1 or n < 0 or rev.numel() != nnz:
        raise ValueError('graph_dropout: indptr must be [n + 1] and rev must hold one position per edge')
    keep_prob = float(keep_prob)
    if not 0.0 <= keep_prob <= 1.0:
        raise ValueError(f'graph_dropout: keep_prob must lie in [0, 1], got {keep_prob}')
    if node_drop is not None:
        if node_drop.dtype == torch.bool:
            node_drop = node_drop.view(torch.uint8)
        node_drop = _need(node_drop, torch.uint8, 'node_drop')
        if node_drop.numel() != n:
            raise ValueError('graph_dropout: node_drop must hold one flag per node')
    dev = indptr.device
    values = torch.empty(nnz, dtype=torch.float32, device=dev)
    t_values = torch.empty(nnz, dtype=torch.float32, device=dev)
    in_deg = torch.empty(n, dtype=torch.int32, device=dev)
    out_deg = torch.empty(n, dtype=torch.int32, device=dev)
    keep = torch.empty(nnz, dtype=torch.uint8, device=dev) if want_keep else None
    a = nat.GraphDropoutArgs()
    a.indptr, a.indices, a.rev, a.n_rows, a.nnz = ptr(indptr), ptr(indices), ptr(rev), n, nnz
    a.keep_prob, a.node_drop, a.keep = keep_prob, ptr(node_drop), ptr(keep)
    a.in_deg, a.out_deg, a.values, a.t_values = ptr(in_deg), ptr(out_deg), ptr(values), ptr(t_values)
    a.long_row = GRAPH_DROPOUT_LONG_ROW if long_row is None else int(long_row)
    if keep_prob < 1.0 and nnz:
        pc = rng.reserve(nnz, 4, dev, generator)
        a.seed, a.offset, a.grid_threads, a.elem_base = pc.seed, pc.offset, pc.grid_threads, pc.elem_base
    _launch('rsa_graph_dropout', ctypes.byref(a))
    return (values, t_values, in_deg, out_deg) + ((keep,) if want_keep else ())


# ------------------------------------------------------------------ NGCF's BiCombiner layer
BI_COMBINE_MAX_DIM = 128          # both weight matrices are kept in LDS (rsa_combine.hip, "WEIGHTS IN LDS")


def _bi_combine_args(who, x, m, w1, w2, b1, b2, negative_slope, p, philox):
    x, m = _need(x, torch.float32, 'x'), _need(m, torch.float32, 'm')
    w1, w2 = _need(w1, torch.float32, 'w1'), _need(w2, torch.float32, 'w2')
    b1, b2 = _need(b1, torch.float32, 'b1'), _need(b2, torch.float32, 'b2')
    if x.dim() != 2 or m.shape != x.shape:
        raise ValueError(f'{who}: x and m must be [N, d_in] tensors of one shape, got {tuple(x.shape)} and {tuple(m.shape)}')
    N, d_in = x.shape
    if w1.dim() != 2 or w1.shape[1] != d_in or w2.shape != w1.shape:
        raise ValueError(f'{who}: w1 and w2 must be [d_out, {d_in}] (nn.Linear layout), got {tuple(w1.shape)} and {tuple(w2.shape)}')
    d_out = w1.shape[0]
    if tuple(b1.shape) != (d_out,) or tuple(b2.shape) != (d_out,):
        raise ValueError(f'{who}: b1 and b2 must be [{d_out}]')
    for name, d in (('d_in', d_in), ('d_out', d_out)):
        if d % 4 or not 4 <= d <= BI_COMBINE_MAX_DIM:
            raise ValueError(f'{who}: {name} must be a multiple of 4 in [4, {BI_COMBINE_MAX_DIM}] (the weights are kept in LDS), got {d}')
    p = float(p)
    if not 0.0 <= p < 1.0:
        raise ValueError(f'{who}: the dropout probability must lie in [0, 1), got {p}')
    a = nat.BiCombineArgs()
    a.x, a.m, a.w1, a.w2, a.b1, a.b2 = ptr(x), ptr(m), ptr(w1), ptr(w2), ptr(b1), ptr(b2)
    a.n_rows, a.d_in, a.d_out, a.negative_slope, a.p = N, d_in, d_out, float(negative_slope), p
    if p != 0.0:
        if not isinstance(philox, rng.PhiloxCall):
            raise TypeError(f'{who}: dropout needs philox, a rng.PhiloxCall (rng.reserve(N * d_out, 4, device))')
        a.seed, a.offset, a.grid_threads, a.elem_base = philox.seed, philox.offset, philox.grid_threads, philox.elem_base
    elif philox is not None:
        raise ValueError(f'{who}: philox without dropout (p = 0 draws nothing)')
    return a, (x, m, w1, w2, b1, b2), N, d_in, d_out


def _column_block(who, name, table, col, N, d_out):
    """(table, row stride, col) of the [N, d_out] block at column ``col`` of the wider fp32 table ``table``."""
    _need_view(table, torch.float32, name)
    col = int(col)
    if table.dim() != 2 or table.shape[0] != N or table.stride(1) != 1 or table.stride(0) % 4 or col % 4 or col < 0 \
            or col + d_out > table.shape[1] or table.data_ptr() % 16:
        raise ValueError(f'{who}: {name} must be a 16-byte aligned [{N}, >= col + {d_out}] table with unit column stride and a row '
                         f'stride and column offset that are multiples of 4 (got {tuple(table.shape)}, strides {table.stride()}, col {col})')
    return table, table.stride(0), col


@_on_device
def bi_combine(x, m, w1, w2, b1, b2, *, negative_slope=0.01, p=0.0, philox=None, want_h=True, out=None, col=0):
    """rsa_bi_combine: NGCF's BiCombiner layer in one launch.  ``x``, ``m`` fp32 [N, d_in]; ``w1``, ``w2`` fp32 [d_out, d_in]
    (``nn.Linear`` layout), ``b1``, ``b2`` fp32 [d_out]; d_in, d_out multiples of 4, at most 128.
    ``h = dropout(LeakyReLU((x + m) w1^T + b1) + LeakyReLU((x * m) w2^T + b2))`` -> fp32 [N, d_out] (``want_h``), and
    ``h / max(||h||_2, 1e-12)`` into columns ``[col, col + d_out)`` of the wider table ``out`` (fp32 [N, >= col + d_out]) when it is
    given; the other columns of ``out`` are not touched.  -> ``h`` (None without ``want_h``).
    Dropout with probability ``p``: with q = fp32(1 - p), element (r, c) is kept iff ``u[r, c] < q`` and divided by q, ``u`` =
    ``torch.rand(N, d_out)`` in the generator state ``philox`` (``rng.reserve(N * d_out, 4, device)``) was reserved in -- bit-equal
    to ``torch.rand_like(h)`` as long as torch draws ``h`` in one call (it splits a tensor of several GiB; the element index here
    is 64-bit).  ``p == 0`` takes no ``philox``."""
    a, keep, N, d_in, d_out = _bi_combine_args('bi_combine', x, m, w1, w2, b1, b2, negative_slope, p, philox)
    if not want_h and out is None:
        raise ValueError('bi_combine: neither h nor a table for the normalised block was asked for')
    h = torch.empty(N, d_out, dtype=torch.float32, device=keep[0].device) if want_h else None
    a.h = ptr(h)
    if out is not None:
        out, a.n_stride, a.n_col = _column_block('bi_combine', 'out', out, col, N, d_out)
        a.n = ptr(out)
    _launch('rsa_bi_combine', ctypes.byref(a))
    return h


@_on_device
def bi_combine_backward(x, m, w1, w2, b1, b2, *, g_h=None, g_out=None, col=0, negative_slope=0.01, p=0.0, philox=None):
    """rsa_bi_combine_backward: the gradients of ``bi_combine`` from ``g_h`` (fp32 [N, d_out], the gradient arriving at ``h``)
    and / or ``g_out`` (the gradient of the wider table; its columns ``[col, col + d_out)`` are the gradient of the normalised
    block).  The layer is recomputed from ``x``, ``m`` and the mask regenerated from ``philox`` (the state the forward was given):
    nothing the forward produced is read.  -> ``(dx, dm, dw1, dw2, db1, db2)``.  No atomics; bit-equal from run to run."""
    a, keep, N, d_in, d_out = _bi_combine_args('bi_combine_backward', x, m, w1, w2, b1, b2, negative_slope, p, philox)
    if g_h is None and g_out is None:
        raise ValueError('bi_combine_backward: neither g_h nor g_out is given')
    dev = keep[0].device
    if g_h is not None:
        g_h = _need(g_h, torch.float32, 'g_h')
        if tuple(g_h.shape) != (N, d_out):
            raise ValueError(f'bi_combine_backward: g_h must be [{N}, {d_out}]')
        a.g_h = ptr(g_h)
    if g_out is not None:
        g_out, a.g_n_stride, a.g_n_col = _column_block('bi_combine_backward', 'g_out', g_out, col, N, d_out)
        a.g_n = ptr(g_out)
    dx, dm = torch.empty(N, d_in, dtype=torch.float32, device=dev), torch.empty(N, d_in, dtype=torch.float32, device=dev)
    if N == 0:
        z = lambda *s: torch.zeros(*s, dtype=torch.float32, device=dev)      # noqa: E731
        return dx, dm, z(d_out, d_in), z(d_out, d_in), z(d_out), z(d_out)
    dw = torch.empty(2, d_out, d_in, dtype=torch.float32, device=dev)
    db = torch.empty(2, d_out, dtype=torch.float32, device=dev)
    ws, a.workspace_bytes = _workspace(dev, 'rsa_bi_combine_workspace_bytes', N, d_in, d_out)
    a.workspace = ptr(ws)
    a.dx, a.dm, a.dw1, a.dw2, a.db1, a.db2 = ptr(dx), ptr(dm), ptr(dw[0]), ptr(dw[1]), ptr(db[0]), ptr(db[1])
    _launch('rsa_bi_combine_backward', ctypes.byref(a))
    return dx, dm, dw[0], dw[1], db[0], db[1]


# ------------------------------------------------------------------ the attention core of the sequence towers
SEQ_ATTENTION_MAX_LEN = 64             # one tile holds the sequence (rsa_attention.hip, "TILE")
SEQ_ATTENTION_HEAD_DIMS = (16, 32, 64)


def _seq_attention_args(who, qkv, key_pad, n_head, causal, scale, p, philox):
    qkv = _need(qkv, torch.float32, 'qkv')
    n_head = int(n_head)
    if qkv.dim() != 3 or n_head < 1 or qkv.shape[2] % (3 * n_head):
        raise ValueError(f'{who}: qkv must be [B, L, 3 * n_head * head_dim] (n_head {n_head}), got {tuple(qkv.shape)}')
    B, L, D3 = qkv.shape
    D = D3 // 3
    dh = D // n_head
    if dh not in SEQ_ATTENTION_HEAD_DIMS:
        raise ValueError(f'{who}: head_dim must be one of {SEQ_ATTENTION_HEAD_DIMS}, got {dh}')
    if not 1 <= L <= SEQ_ATTENTION_MAX_LEN:
        raise ValueError(f'{who}: the sequence length must lie in [1, {SEQ_ATTENTION_MAX_LEN}] (one tile holds it), got {L}')
    if key_pad is not None:
        if key_pad.dtype == torch.bool:
            key_pad = key_pad.view(torch.uint8) if key_pad.is_contiguous() else key_pad.contiguous().view(torch.uint8)
        key_pad = _need(key_pad, torch.uint8, 'key_pad')
        if tuple(key_pad.shape) != (B, L):
            raise ValueError(f'{who}: key_pad must be [{B}, {L}], got {tuple(key_pad.shape)}')
    p = float(p)
    if not 0.0 <= p < 1.0:
        raise ValueError(f'{who}: the dropout probability must lie in [0, 1), got {p}')
    a = nat.AttentionArgs()
    a.qkv, a.key_pad = ptr(qkv), ptr(key_pad)
    a.n_seq, a.seq_len, a.n_head, a.head_dim, a.causal = B, L, n_head, dh, 1 if causal else 0
    a.scale = 1.0 / math.sqrt(dh) if scale is None else float(scale)
    a.p = p
    if p != 0.0:
        if not isinstance(philox, rng.PhiloxCall):
            raise TypeError(f'{who}: dropout needs philox, a rng.PhiloxCall (rng.reserve(B * n_head * L * L, 4, device))')
        if B * n_head * L * L >= 1 << 31:
            raise ValueError(f'{who}: B * n_head * L * L = {B * n_head * L * L} >= 2^31: torch.rand splits such a call, the mask '
                             'would not be its')
        a.seed, a.offset, a.grid_threads, a.elem_base = philox.seed, philox.offset, philox.grid_threads, philox.elem_base
    elif philox is not None:
        raise ValueError(f'{who}: philox without dropout (p = 0 draws nothing)')
    return a, (qkv, key_pad), B, L, D


@_on_device
def seq_attention(qkv, key_pad, n_head, *, causal=True, scale=None, p=0.0, philox=None, want_keep=False):
    """rsa_attention: the attention core of ``nn.MultiheadAttention`` in one launch.  ``qkv`` fp32 [B, L, 3 D] =
    ``F.linear(x, in_proj_weight, in_proj_bias)`` (q, k, v side by side, head h in columns ``h * dh ..`` of each); ``key_pad``
    bool / uint8 [B, L] or None (non-zero: that key is not attended); L <= 64, dh = D / n_head in {16, 32, 64}.
    Key j is allowed for query i iff ``(not causal or j <= i) and not key_pad[b, j]``; ``P`` = softmax of ``scale * q k^T`` over
    the allowed keys (``scale`` defaults to ``1 / sqrt(dh)``), ``out = (keep * P / q) v``.
    -> ``(out [B, L, D], lse [B, n_head, L][, keep uint8 [B, n_head, L, L]])``.  A query without an allowed key gets ``out = 0``
    and ``lse = -inf`` (torch: NaN).
    Dropout with probability ``p``: with q = fp32(1 - p), element (b, h, i, j) is kept iff ``u[b, h, i, j] < q``, ``u`` =
    ``torch.rand(B, n_head, L, L)`` in the generator state ``philox`` (``rng.reserve(B * n_head * L * L, 4, device)``) was reserved
    in.  ``p == 0`` takes no ``philox``."""
    a, keepalive, B, L, D = _seq_attention_args('seq_attention', qkv, key_pad, n_head, causal, scale, p, philox)
    dev = keepalive[0].device
    out = torch.empty(B, L, D, dtype=torch.float32, device=dev)
    lse = torch.empty(B, a.n_head, L, dtype=torch.float32, device=dev)
    keep = torch.empty(B, a.n_head, L, L, dtype=torch.uint8, device=dev) if want_keep else None
    a.out, a.lse, a.keep = ptr(out), ptr(lse), ptr(keep)
    _launch('rsa_attention', ctypes.byref(a))
    return (out, lse) + ((keep,) if want_keep else ())


@_on_device
def seq_attention_backward(qkv, key_pad, n_head, out, lse, g_out, *, causal=True, scale=None, p=0.0, philox=None):
    """rsa_attention_backward: ``dqkv`` [B, L, 3 D] of ``seq_attention`` from ``g_out`` (the gradient of ``out``), the forward's
    ``out`` and ``lse`` and the Philox state the forward was given.  The scores and the mask are recomputed; every element is
    written (zeros where nothing flows).  No atomics; bit-equal from run to run."""
    a, keepalive, B, L, D = _seq_attention_args('seq_attention_backward', qkv, key_pad, n_head, causal, scale, p, philox)
    out, lse, g_out = _need(out, torch.float32, 'out'), _need(lse, torch.float32, 'lse'), _need(g_out, torch.float32, 'g_out')
    if tuple(out.shape) != (B, L, D) or tuple(g_out.shape) != (B, L, D) or tuple(lse.shape) != (B, a.n_head, L):
        raise ValueError(f'seq_attention_backward: out and g_out must be [{B}, {L}, {D}] and lse [{B}, {a.n_head}, {L}], got '
                         f'{tuple(out.shape)}, {tuple(g_out.shape)}, {tuple(lse.shape)}')
    dqkv = torch.empty(B, L, 3 * D, dtype=torch.float32, device=out.device)
    a.out, a.lse, a.g_out, a.dqkv = ptr(out), ptr(lse), ptr(g_out), ptr(dqkv)
    _launch('rsa_attention_backward', ctypes.byref(a))
    return dqkv


# ------------------------------------------------------------------ the GRU recurrence of the sequence towers
GRU_HIDDEN_SIZES = (32, 64, 128)


def _gru_args(who, gi, w_hh, h0, lengths):
    gi, w_hh = _need(gi, torch.float32, 'gi'), _need(w_hh, torch.float32, 'w_hh')
    if gi.dim() != 3 or w_hh.dim() != 2 or w_hh.shape[0] != 3 * w_hh.shape[1] or gi.shape[2] != w_hh.shape[0]:
        raise ValueError(f'{who}: gi must be [B, L, 3 H] and w_hh [3 H, H], got {tuple(gi.shape)} and {tuple(w_hh.shape)}')
    B, L, H3 = gi.shape
    H = H3 // 3
    if H not in GRU_HIDDEN_SIZES:
        raise ValueError(f'{who}: the hidden size must be one of {GRU_HIDDEN_SIZES}, got {H}')
    if h0 is not None:
        h0 = _need(h0, torch.float32, 'h0')
        if tuple(h0.shape) != (B, H):
            raise ValueError(f'{who}: h0 must be [{B}, {H}], got {tuple(h0.shape)}')
    lengths_host = None
    if lengths is not None:
        if lengths.dtype != torch.int64 or tuple(lengths.shape) != (B,):
            raise ValueError(f'{who}: lengths must be int64 [{B}], got {lengths.dtype} {tuple(lengths.shape)}')
        if not lengths.is_cuda:
            # a host copy: the native entry checks it against [0, L]; the device copy is what the kernel reads
            lengths_host = lengths.contiguous()
            lengths = lengths_host.to(gi.device)
        lengths = _need(lengths, torch.int64, 'lengths')
    a = nat.GruArgs()
    a.gi, a.w_hh, a.h0, a.lengths = ptr(gi), ptr(w_hh), ptr(h0), ptr(lengths)
    a.lengths_host = lengths_host.data_ptr() if lengths_host is not None else None
    a.n_seq, a.seq_len, a.hidden = B, L, H
    return a, (gi, w_hh, h0, lengths, lengths_host), B, L, H


@_on_device
def gru_sequence(gi, w_hh, *, b_hh=None, h0=None, lengths=None):
    """rsa_gru: the sequential part of a one-layer, batch-first ``nn.GRU`` in one launch.  ``gi`` fp32 [B, L, 3 H] =
    ``F.linear(x, W_ih, b_ih)`` (gates r | z | n), ``w_hh`` [3 H, H], ``b_hh`` [3 H] or None (``b_hn`` inside ``r * (.)``),
    ``h0`` [B, H] or None (zeros), ``lengths`` int64 [B] or None; H in {32, 64, 128}.
    -> ``out`` [B, L, H], every ``h_t``.  With ``lengths`` row b stops at ``lengths[b]`` and ``out[b, t >= lengths[b]]`` is 0
    (values outside [0, L] are clamped on the device; a CPU ``lengths`` tensor is checked instead and raises)."""
    a, keepalive, B, L, H = _gru_args('gru_sequence', gi, w_hh, h0, lengths)
    if b_hh is not None:
        b_hh = _need(b_hh, torch.float32, 'b_hh')
        if tuple(b_hh.shape) != (3 * H,):
            raise ValueError(f'gru_sequence: b_hh must be [{3 * H}], got {tuple(b_hh.shape)}')
    out = torch.empty(B, L, H, dtype=torch.float32, device=keepalive[0].device)
    a.b_hh, a.out = ptr(b_hh), ptr(out)
    _launch('rsa_gru', ctypes.byref(a))
    return out


@_on_device
def gru_sequence_backward(gi, gh, out, w_hh, g_out, *, h0=None, lengths=None):
    """rsa_gru_backward: ``(dgi [B, L, 3 H], dgh_n [B, L, H], dh0 [B, H])`` of ``gru_sequence`` from ``g_out`` (the gradient of
    ``out``), the forward's ``out`` and ``gh = F.linear(h_prev, w_hh, b_hh)`` with ``h_prev = cat(h0, out[:, :-1])``.  The r and z
    parts of ``dgh`` are those of ``dgi``; ``dgh_n`` is its n part.  Every element is written (zeros at ``t >= lengths[b]``).
    No atomics; bit-equal from run to run."""
    a, keepalive, B, L, H = _gru_args('gru_sequence_backward', gi, w_hh, h0, lengths)
    gh, out, g_out = _need(gh, torch.float32, 'gh'), _need(out, torch.float32, 'out'), _need(g_out, torch.float32, 'g_out')
    if tuple(gh.shape) != (B, L, 3 * H) or tuple(out.shape) != (B, L, H) or tuple(g_out.shape) != (B, L, H):
        raise ValueError(f'gru_sequence_backward: gh must be [{B}, {L}, {3 * H}] and out, g_out [{B}, {L}, {H}], got '
                         f'{tuple(gh.shape)}, {tuple(out.shape)}, {tuple(g_out.shape)}')
    dev = out.device
    dgi = torch.empty(B, L, 3 * H, dtype=torch.float32, device=dev)
    dgh_n = torch.empty(B, L, H, dtype=torch.float32, device=dev)
    dh0 = torch.empty(B, H, dtype=torch.float32, device=dev)
    a.gh, a.out, a.g_out, a.dgi, a.dgh_n, a.dh0 = ptr(gh), ptr(out), ptr(g_out), ptr(dgi), ptr(dgh_n), ptr(dh0)
    _launch('rsa_gru_backward', ctypes.byref(a))
    return dgi, dgh_n, dh0


# ------------------------------------------------------------------ feed-forward attention pooling (NARM, STAMP)
FF_ATTENTION_DIMS = (32, 64, 128)      # key width and hidden width: W_k is kept in LDS (rsa_ffattn.hip, "WEIGHTS IN LDS")


def _ff_attention_args(who, key, qh, w_k, w2, b2, key_pad, scale):
    key, qh = _need(key, torch.float32, 'key'), _need(qh, torch.float32, 'qh')
    w_k = _need_view(w_k, torch.float32, 'w_k')
    w2, b2 = _need(w2, torch.float32, 'w2'), _need(b2, torch.float32, 'b2')
    if key.dim() != 3 or key.shape[1] < 1:
        raise ValueError(f'{who}: key must be [B, S, D] with S >= 1, got {tuple(key.shape)}')
    B, S, D = key.shape
    if w_k.dim() != 2 or w_k.shape[1] != D:
        raise ValueError(f'{who}: w_k must be [M, {D}] (the key columns of the hidden Linear), got {tuple(w_k.shape)}')
    M = w_k.shape[0]
    for name, d in (('D', D), ('M', M)):
        if d not in FF_ATTENTION_DIMS:
            raise ValueError(f'{who}: {name} must be one of {FF_ATTENTION_DIMS}, got {d}')
    if w_k.stride(1) != 1 or w_k.stride(0) % 4 or w_k.stride(0) < D or w_k.data_ptr() % 16:
        raise ValueError(f'{who}: w_k must be a 16-byte aligned column block with unit column stride and a row stride that is a '
                         f'multiple of 4 (got strides {w_k.stride()}, offset {w_k.storage_offset()})')
    if tuple(qh.shape) != (B, M):
        raise ValueError(f'{who}: qh must be [{B}, {M}], got {tuple(qh.shape)}')
    if w2.numel() != M or b2.numel() != 1:
        raise ValueError(f'{who}: w2 must hold {M} elements and b2 one, got {tuple(w2.shape)} and {tuple(b2.shape)}')
    if key_pad is not None:
        if key_pad.dtype == torch.bool:
            key_pad = key_pad.view(torch.uint8) if key_pad.is_contiguous() else key_pad.contiguous().view(torch.uint8)
        key_pad = _need(key_pad, torch.uint8, 'key_pad')
        if tuple(key_pad.shape) != (B, S):
            raise ValueError(f'{who}: key_pad must be [{B}, {S}], got {tuple(key_pad.shape)}')
    scale = float(scale)
    if not math.isfinite(scale):
        raise ValueError(f'{who}: scale must be finite, got {scale}')
    a = nat.FfAttentionArgs()
    a.key, a.qh, a.w_k, a.w_k_stride, a.w2, a.b2, a.key_pad = ptr(key), ptr(qh), ptr(w_k), w_k.stride(0), ptr(w2), ptr(b2), ptr(key_pad)
    a.n_seq, a.seq_len, a.d, a.m, a.scale = B, S, D, M, scale
    return a, (key, qh, w_k, w2, b2, key_pad), B, S, D, M


@_on_device
def ff_attention_pool(key, qh, w_k, w2, b2, key_pad=None, *, scale):
    """rsa_ff_attention: the reference's feed-forward ``AttentionLayer`` with one query per sequence, ``softmax=False`` and
    value = key, in one launch.  ``key`` fp32 [B, S, D]; ``qh`` fp32 [B, M] = ``F.linear(query, W1[:, :q_dim], b1)``; ``w_k`` fp32
    [M, D] = ``W1[:, q_dim:]``, read in place through its row stride (a column block of ``W1``: no copy); ``w2`` fp32 [M] (or
    [1, M]); ``b2`` fp32 [1] on the device; ``key_pad`` bool / uint8 [B, S] or None; D, M in {32, 64, 128}, any S >= 1.
    ``a[b, s] = 0 if key_pad[b, s] else (w2 . sigmoid(qh[b] + w_k key[b, s]) + b2) * scale`` (``scale`` as fp32: the reference's
    ``1 / sqrt(q_dim)``), ``out[b] = sum_s a[b, s] key[b, s]``.  -> ``(out [B, D], a [B, S])``; nothing of size B S M is written.
    A sequence that is padded whole gets ``out = 0``; B = 0 returns empty tensors without a launch."""
    a, keepalive, B, S, D, M = _ff_attention_args('ff_attention_pool', key, qh, w_k, w2, b2, key_pad, scale)
    dev = keepalive[0].device
    out = torch.empty(B, D, dtype=torch.float32, device=dev)
    w = torch.empty(B, S, dtype=torch.float32, device=dev)
    if B == 0:
        return out, w
    a.out, a.a = ptr(out), ptr(w)
    _launch('rsa_ff_attention', ctypes.byref(a))
    return out, w


@_on_device
def ff_attention_pool_backward(key, qh, w_k, w2, b2, key_pad, g_out, *, scale):
    """rsa_ff_attention_backward: the gradients of ``ff_attention_pool`` from ``g_out`` (fp32 [B, D], the gradient of ``out``).
    The hidden layer and the weights are recomputed from ``key`` and ``qh``: nothing the forward produced is read.
    -> ``(dkey [B, S, D], dqh [B, M], dw_k [M, D], dw2 [M], db2 [1])``; every element is written, +0 at padded positions.  The
    gradients of the query and of ``W1[:, :q_dim]`` / ``b1`` follow from ``dqh`` on the caller's side.  No atomics; bit-equal from
    run to run."""
    a, keepalive, B, S, D, M = _ff_attention_args('ff_attention_pool_backward', key, qh, w_k, w2, b2, key_pad, scale)
    g_out = _need(g_out, torch.float32, 'g_out')
    if tuple(g_out.shape) != (B, D):
        raise ValueError(f'ff_attention_pool_backward: g_out must be [{B}, {D}], got {tuple(g_out.shape)}')
    dev = keepalive[0].device
    dkey = torch.empty(B, S, D, dtype=torch.float32, device=dev)
    dqh = torch.empty(B, M, dtype=torch.float32, device=dev)
    if B == 0:
        z = lambda *s: torch.zeros(*s, dtype=torch.float32, device=dev)      # noqa: E731
        return dkey, dqh, z(M, D), z(M), z(1)
    dw_k = torch.empty(M, D, dtype=torch.float32, device=dev)
    dw2 = torch.empty(M + 1, dtype=torch.float32, device=dev)
    ws, a.workspace_bytes = _workspace(dev, 'rsa_ff_attention_workspace_bytes', B, S, D, M)
    a.workspace, a.g_out = ptr(ws), ptr(g_out)
    a.dkey, a.dqh, a.dw_k, a.dw2, a.db2 = ptr(dkey), ptr(dqh), ptr(dw_k), ptr(dw2[:M]), ptr(dw2[M:])
    _launch('rsa_ff_attention_backward', ctypes.byref(a))
    return dkey, dqh, dw_k, dw2[:M], dw2[M:]


# ------------------------------------------------------------------ hierarchical gating (HGN)
HGN_GATING_DIMS = (32, 64, 128)        # the embedding width: W_g_1 is kept in LDS (rsa_gating.hip)
HGN_POOLING = {'mean': 0, 'max': 1}


def _hgn_gating_args(who, S, ug, ui, w1, w3, pooling):
    S, ug, ui = _need(S, torch.float32, 'S'), _need(ug, torch.float32, 'ug'), _need(ui, torch.float32, 'ui')
    w1, w3 = _need_view(w1, torch.float32, 'w1'), _need(w3, torch.float32, 'w3')
    if pooling not in HGN_POOLING:
        raise ValueError(f'{who}: pooling must be one of {tuple(HGN_POOLING)}, got {pooling!r}')
    if S.dim() != 3 or S.shape[1] < 1:
        raise ValueError(f'{who}: S must be [B, L, D] with L >= 1, got {tuple(S.shape)}')
    B, L, D = S.shape
    if D not in HGN_GATING_DIMS:
        raise ValueError(f'{who}: D must be one of {HGN_GATING_DIMS}, got {D}')
    if tuple(w1.shape) != (D, D):
        raise ValueError(f'{who}: w1 must be [{D}, {D}], got {tuple(w1.shape)}')
    if w1.stride(1) != 1 or w1.stride(0) % 4 or w1.stride(0) < D or w1.data_ptr() % 16:
        raise ValueError(f'{who}: w1 must be 16-byte aligned with unit column stride and a row stride that is a multiple of 4 '
                         f'(got strides {w1.stride()}, offset {w1.storage_offset()})')
    if tuple(ug.shape) != (B, D) or tuple(ui.shape) != (B, L) or w3.numel() != D:
        raise ValueError(f'{who}: ug must be [{B}, {D}], ui [{B}, {L}] and w3 hold {D} elements, got {tuple(ug.shape)}, '
                         f'{tuple(ui.shape)}, {tuple(w3.shape)}')
    a = nat.HgnGatingArgs()
    a.s, a.ug, a.ui, a.w1, a.w1_stride, a.w3 = ptr(S), ptr(ug), ptr(ui), ptr(w1), w1.stride(0), ptr(w3)
    a.n_seq, a.seq_len, a.d, a.pooling = B, L, D, HGN_POOLING[pooling]
    return a, (S, ug, ui, w1, w3), B, L, D


@_on_device
def hgn_gating(S, ug, ui, w1, w3, pooling='mean'):
    """rsa_hgn_gating: HGN's feature gate, instance gate, pooling and item-item sum in one launch.  ``S`` fp32 [B, L, D] (padded
    positions are zero rows: there is no mask); ``ug`` fp32 [B, D] = ``W_g_2(U) + b_g``; ``ui`` fp32 [B, L] =
    ``U @ W_g_4.weight[:L].T``; ``w1`` fp32 [D, D] = ``W_g_1.weight``, read in place through its row stride; ``w3`` fp32 [D] (or
    [1, D]); D in {32, 64, 128}, any L >= 1.  ``f = sigmoid(S w1^T + ug)``, ``sf = S * f``, ``w = sigmoid(sf . w3 + ui)``,
    ``si = sf * w``; ``out = si.sum(1) / w.sum(1) + S.sum(1)`` ('mean') or ``si.max(1) + S.sum(1)`` ('max').
    -> ``(out [B, D], w [B, L], arg)``: ``arg`` int32 [B, D], the position of the maximum (the lowest on exact ties), None for
    'mean'.  Nothing of size B L D is written.  B = 0 returns empty tensors without a launch."""
    a, keepalive, B, L, D = _hgn_gating_args('hgn_gating', S, ug, ui, w1, w3, pooling)
    dev = keepalive[0].device
    out = torch.empty(B, D, dtype=torch.float32, device=dev)
    w = torch.empty(B, L, dtype=torch.float32, device=dev)
    arg = torch.empty(B, D, dtype=torch.int32, device=dev) if pooling == 'max' else None
    if B == 0:
        return out, w, arg
    a.out, a.w, a.arg = ptr(out), ptr(w), ptr(arg)
    _launch('rsa_hgn_gating', ctypes.byref(a))
    return out, w, arg


@_on_device
def hgn_gating_backward(S, ug, ui, w1, w3, w, arg, g_out, pooling='mean'):
    """rsa_hgn_gating_backward: the gradients of ``hgn_gating`` from ``g_out`` (fp32 [B, D], the gradient of ``out``), the forward's
    ``w`` [B, L] and, for 'max', its ``arg``.  The gates are recomputed from ``S`` and ``ug``.
    -> ``(dS [B, L, D], dug [B, D], dui [B, L], dw1 [D, D], dw3 [D])``; every element is written; ``dS`` is NOT zero at padded
    positions (the gather's backward drops them).  The gradients of ``W_g_2``, ``b_g``, ``W_g_4.weight[:L]`` and ``U`` follow from
    ``dug`` and ``dui`` on the caller's side.  No atomics; bit-equal from run to run."""
    a, keepalive, B, L, D = _hgn_gating_args('hgn_gating_backward', S, ug, ui, w1, w3, pooling)
    g_out, w = _need(g_out, torch.float32, 'g_out'), _need(w, torch.float32, 'w')
    if tuple(g_out.shape) != (B, D) or tuple(w.shape) != (B, L):
        raise ValueError(f'hgn_gating_backward: g_out must be [{B}, {D}] and w [{B}, {L}], got {tuple(g_out.shape)}, {tuple(w.shape)}')
    if pooling == 'max':
        arg = _need(arg, torch.int32, 'arg')
        if tuple(arg.shape) != (B, D):
            raise ValueError(f'hgn_gating_backward: arg must be [{B}, {D}], got {tuple(arg.shape)}')
    else:
        arg = None
    dev = keepalive[0].device
    dS = torch.empty(B, L, D, dtype=torch.float32, device=dev)
    dug = torch.empty(B, D, dtype=torch.float32, device=dev)
    dui = torch.empty(B, L, dtype=torch.float32, device=dev)
    if B == 0:
        return dS, dug, dui, torch.zeros(D, D, dtype=torch.float32, device=dev), torch.zeros(D, dtype=torch.float32, device=dev)
    dw1 = torch.empty(D, D, dtype=torch.float32, device=dev)
    dw3 = torch.empty(D, dtype=torch.float32, device=dev)
    ws, a.workspace_bytes = _workspace(dev, 'rsa_hgn_gating_workspace_bytes', B, L, D)
    a.workspace, a.g_out, a.w, a.arg = ptr(ws), ptr(g_out), ptr(w), ptr(arg)
    a.ds, a.dug, a.dui, a.dw1, a.dw3 = ptr(dS), ptr(dug), ptr(dui), ptr(dw1), ptr(dw3)
    _launch('rsa_hgn_gating_backward', ctypes.byref(a))
    return dS, dug, dui, dw1, dw3


# ------------------------------------------------------------------ sequence views (CL4SRec)
SEQ_AUGMENT_MAX_LEN = 64          # one lane per position, one wave per sequence (rsa_seqaug.hip)
SEQ_AUGMENT_KINDS = {'crop': 0, 'mask': 1, 'reorder': 2}


def seq_augment(seq, seqlen, kind, sub, mask_id=0, generator=None):
    """rsa_seq_augment: one augmented view of the histories ``seq`` (int64 [B, L], right-padded with 0, read in place through its
    row stride; L <= 64) of lengths ``seqlen`` ([B] int32 / int64, clamped into [0, L] by the kernel) in one launch.  ``kind`` is
    'crop', 'mask' or 'reorder'; ``sub`` (int32 [L + 1] on the device) is the table ``len -> n_sub``.  The random choices are
    ``U = torch.rand([B, L + 1], device=...)`` on the device generator, which is advanced as that call would advance it: ``U[b, 0]``
    draws the start, ``U[b, 1 + p]`` is the key of position p (``data_augmentation.seq_augment_torch`` is the rule in torch ops).
    -> ``(out int64 [B, L], new_len [B] in seqlen's dtype)``.  No atomics; bit-equal from run to run."""
    if kind not in SEQ_AUGMENT_KINDS:
        raise ValueError(f"seq_augment: kind must be 'crop', 'mask' or 'reorder', got {kind!r}")
    return _seq_augment(seq, seqlen, SEQ_AUGMENT_KINDS[kind], sub, int(mask_id), generator)


@_on_device
def _seq_augment(seq, seqlen, kind, sub, mask_id, generator):
    seq = _need_view(seq, torch.int64, 'seq')
    if seq.dim() != 2:
        raise ValueError(f'seq_augment: seq must be [B, L], got {tuple(seq.shape)}')
    B, L = seq.shape
    if not 1 <= L <= SEQ_AUGMENT_MAX_LEN:
        raise ValueError(f'seq_augment: L must lie in [1, {SEQ_AUGMENT_MAX_LEN}], got {L}')
    if B and (seq.stride(1) != 1 or seq.stride(0) < L):
        seq = seq.contiguous()
    if seqlen.dtype not in (torch.int32, torch.int64):
        raise TypeError(f'seq_augment: seqlen must be int32 or int64, got {seqlen.dtype}')
    seqlen = _need(seqlen, seqlen.dtype, 'seqlen')
    sub = _need(sub, torch.int32, 'sub')
    if seqlen.numel() != B or sub.numel() != L + 1:
        raise ValueError(f'seq_augment: seqlen must hold {B} lengths and sub {L + 1} entries, got {seqlen.numel()} and {sub.numel()}')
    out = torch.empty(B, L, dtype=torch.int64, device=seq.device)
    new_len = torch.empty(B, dtype=seqlen.dtype, device=seq.device)
    if B == 0:
        return out, new_len
    pc = rng.reserve(B * (L + 1), 4, seq.device, generator)
    a = nat.SeqAugmentArgs()
    a.seq, a.seq_stride, a.seqlen, a.sub, a.n_seq, a.mask_id = ptr(seq), seq.stride(0), ptr(seqlen), ptr(sub), B, int(mask_id)
    a.seq_len, a.kind, a.seqlen_bytes = L, kind, seqlen.element_size()
    a.seed, a.offset, a.grid_threads, a.elem_base = pc.seed, pc.offset, pc.grid_threads, pc.elem_base
    a.out, a.new_len = ptr(out), ptr(new_len)
    _launch('rsa_seq_augment', ctypes.byref(a))
    return out, new_len


# ------------------------------------------------------------------ in-batch InfoNCE (CL4SRec)
BATCH_INFONCE_DIMS = (32, 64, 128)


def _batch_infonce_args(who, zi, zj, inv_t, both, labels):
    zi, zj = _need(zi, torch.float32, 'zi'), _need(zj, torch.float32, 'zj')
    if zi.dim() != 2 or zi.shape != zj.shape:
        raise ValueError(f'{who}: zi and zj must be [B, d] of one shape, got {tuple(zi.shape)} and {tuple(zj.shape)}')
    B, d = zi.shape
    if d not in BATCH_INFONCE_DIMS:
        raise ValueError(f'{who}: d must be one of {BATCH_INFONCE_DIMS}, got {d}')
    labels = _need_opt(labels, torch.int64, 'labels')
    if labels is not None and tuple(labels.shape) != (B,):
        raise ValueError(f'{who}: labels must hold one label per row')
    a = nat.BatchInfoNceArgs()
    a.zi, a.zj, a.labels, a.n_rows, a.d, a.both, a.inv_t = ptr(zi), ptr(zj), ptr(labels), B, d, int(bool(both)), float(inv_t)
    return a, (zi, zj, labels), B, d


@_on_device
def batch_infonce(zi, zj, inv_t, both=True, labels=None):
    """rsa_batch_infonce: ``lse`` [B] and ``pos`` [B] of the in-batch InfoNCE of ``zi``, ``zj`` (fp32 [B, d], d in 32 / 64 / 128;
    normalised by the caller for 'cosine') without a [B, 2B] matrix.  Row b's logits are ``<zi_b, zj_k> inv_t`` for every k but those
    with ``k != b`` and ``labels[k] == labels[b]`` and, with ``both``, ``<zi_b, zi_k> inv_t`` for every ``k != b`` whose label differs
    (no ``labels``: every ``k != b``); ``pos_b = <zi_b, zj_b> inv_t``.  The loss is ``mean(lse - pos)``."""
    a, keepalive, B, d = _batch_infonce_args('batch_infonce', zi, zj, inv_t, both, labels)
    lse = torch.empty(B, dtype=torch.float32, device=keepalive[0].device)
    pos = torch.empty(B, dtype=torch.float32, device=keepalive[0].device)
    a.lse, a.pos = ptr(lse), ptr(pos)
    _launch('rsa_batch_infonce', ctypes.byref(a))
    return lse, pos


@_on_device
def batch_infonce_backward(zi, zj, inv_t, both, labels, lse, g):
    """rsa_batch_infonce_backward: ``(dzi, dzj)`` from the forward's ``lse`` and ``g`` [B], the upstream of ``lse - pos``; the
    softmax is recomputed from ``lse`` on the matrix cores (a row-stationary and a key-stationary pass).  No float atomics; two runs
    are bit-equal."""
    a, keepalive, B, d = _batch_infonce_args('batch_infonce_backward', zi, zj, inv_t, both, labels)
    lse, g = _need(lse, torch.float32, 'lse'), _need(g, torch.float32, 'g')
    if tuple(lse.shape) != (B,) or tuple(g.shape) != (B,):
        raise ValueError(f'batch_infonce_backward: lse and g must be [{B}], got {tuple(lse.shape)} and {tuple(g.shape)}')
    dzi, dzj = torch.empty_like(keepalive[0]), torch.empty_like(keepalive[1])
    a.lse, a.g, a.dzi, a.dzj = ptr(lse), ptr(g), ptr(dzi), ptr(dzj)
    _launch('rsa_batch_infonce_backward', ctypes.byref(a))
    return dzi, dzj


# ------------------------------------------------------------------ user-history bags (MultiDAE / MultiVAE)
BAG_MAX_DIM = 1024                # one thread per 16-byte column of a row (rsa_bag.hip)
BAG_SCALES = {'sum': 0, 'rsqrt': 1, 'mean': 2}


def _bag_args(who, ids, N, d, scale):
    ids = _need_view(ids, torch.int64, 'ids')
    if scale not in BAG_SCALES:
        raise ValueError(f'{who}: scale must be one of {tuple(BAG_SCALES)}, got {scale!r}')
    if ids.dim() != 2:
        raise ValueError(f'{who}: ids must be [B, L], got {tuple(ids.shape)}')
    if d % 4 or not 4 <= d <= BAG_MAX_DIM:
        raise ValueError(f'{who}: the row width must be a multiple of 4 in [4, {BAG_MAX_DIM}], got {d}')
    B, L = ids.shape
    if B > 0 and L > 0 and (ids.stride(1) != 1 or ids.stride(0) < L):
        ids = ids.contiguous()
    a = nat.BagArgs()
    a.ids, a.ids_stride = ptr(ids), (ids.stride(0) if B > 0 and L > 0 else L)
    a.n_rows, a.n_bags, a.bag_len, a.d, a.scale = N, B, L, d, BAG_SCALES[scale]
    return a, ids, B, L


@_on_device
def bag_pool(table, ids, scale='sum'):
    """rsa_bag_pool: ``out[b] = s_b * table[ids[b, live]].sum(0)`` straight from the padded id matrix.  ``table`` fp32 [N, d], d
    a multiple of 4 up to 1024; ``ids`` int64 [B, L], read in place through its row stride; an id is live when it is > 0 (0 is
    padding, anywhere in the row; it is skipped, not read).  ``scale``: 'sum' (s = 1), 'rsqrt' (s = cnt ** -0.5) or 'mean'
    (s = 1 / cnt); an empty bag gives 0 under 'sum' and NaN under the other two.
    -> ``(out [B, d], cnt int32 [B])``.  Nothing of size B L d is read, written or allocated; no atomics; the same bag gives the
    same bits at any batch position."""
    table = _need(table, torch.float32, 'table')
    if table.dim() != 2:
        raise ValueError(f'bag_pool: table must be [N, d], got {tuple(table.shape)}')
    N, d = table.shape
    a, ids, B, L = _bag_args('bag_pool', ids, N, d, scale)
    dev = table.device
    out = torch.empty(B, d, dtype=torch.float32, device=dev)
    cnt = torch.empty(B, dtype=torch.int32, device=dev)
    if B == 0:
        return out, cnt
    ws = None
    if L > 256:
        ws, a.workspace_bytes = _workspace(dev, 'rsa_bag_pool_workspace_bytes', B, L, N)
    a.table, a.out, a.cnt, a.workspace = ptr(table), ptr(out), ptr(cnt), ptr(ws)
    _launch('rsa_bag_pool', ctypes.byref(a))
    return out, cnt


@_on_device
def bag_pool_backward(ids, cnt, g, n_rows, scale='sum', out=None):
    """rsa_bag_pool_backward: the gradient of ``bag_pool`` to its table, ``dW[i] = sum over the occurrences (b, l) of item i of
    s_b * g[b]`` (an item twice in one bag counts twice; row 0 and padding receive nothing), from ``ids``, the forward's ``cnt``
    and ``g`` fp32 [B, d].  -> dense ``dW`` fp32 [n_rows, d] (``out``: a ZEROED tensor to write into).  The (item, bag) pairs
    are sorted by the in-tree radix sort and every touched row is written once: no atomics, two runs are bit-equal."""
    g = _need(g, torch.float32, 'g')
    cnt = _need(cnt, torch.int32, 'cnt')
    if g.dim() != 2:
        raise ValueError(f'bag_pool_backward: g must be [B, d], got {tuple(g.shape)}')
    d = g.shape[1]
    a, ids, B, L = _bag_args('bag_pool_backward', ids, int(n_rows), d, scale)
    if g.shape[0] != B or tuple(cnt.shape) != (B,):
        raise ValueError(f'bag_pool_backward: g must be [{B}, {d}] and cnt [{B}], got {tuple(g.shape)}, {tuple(cnt.shape)}')
    dev = g.device
    if out is None:
        out = torch.zeros(int(n_rows), d, dtype=torch.float32, device=dev)
    else:
        out = _need_view(out, torch.float32, 'out')
        if tuple(out.shape) != (int(n_rows), d) or not out.is_contiguous():
            raise ValueError(f'bag_pool_backward: out must be a contiguous [{int(n_rows)}, {d}] tensor, got {tuple(out.shape)}')
    if B == 0 or L == 0:
        return out
    ws, a.workspace_bytes = _workspace(dev, 'rsa_bag_pool_workspace_bytes', B, L, int(n_rows))
    a.cnt, a.g, a.dw, a.workspace = ptr(cnt), ptr(g), ptr(out), ptr(ws)
    _launch('rsa_bag_pool_backward', ctypes.byref(a))
    return out
