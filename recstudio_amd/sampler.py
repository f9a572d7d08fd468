"""Negative samplers -- host-side mirror of ``recstudio.ann.sampler`` for the graded samplers.

Same class names, constructor arguments, ``forward`` signature and return
conventions as recstudio/ann/sampler.py:48-58 (Sampler), :81-114
(UniformSampler) and :224-258 (PopularSamplerModel); the sampling itself runs in
HIP (``rsa_sample_uniform`` / ``rsa_sample_popular``) on the torch device Philox
stream, so the ids equal what the reference's ``torch.randint`` / ``torch.rand``
+ ``torch.searchsorted`` produce on the same device for the same seed.
"""
from typing import Optional, Union

import numpy as np
import torch
from torch import Tensor

from . import _native as nat
from . import ops

__all__ = ['Sampler', 'UniformSampler', 'MaskedUniformSampler', 'PopularSamplerModel', 'build_guide_table',
           'build_cdf_lines', 'MIDXSamplerUniform', 'ClusterSamplerUniform', 'MIDXSamplerPop', 'ClusterSamplerPop', 'LSHSampler']


class Sampler(torch.nn.Module):
    """recstudio/ann/sampler.py:48-58."""

    def __init__(self, num_items, scorer_fn=None):
        super().__init__()
        self.num_items = num_items - 1   # remove padding (sampler.py:51)
        self.scorer = scorer_fn

    def update(self, item_embs, max_iter=30):
        pass

    def compute_item_p(self, query, pos_items):
        pass


def _query_shape(query, pos_items, device):
    if isinstance(query, int):                      # sampler.py:91-94
        dev = pos_items.device if pos_items is not None else device
        return (query,), dev
    if isinstance(query, Tensor):                   # sampler.py:95-99
        return tuple(query.shape[:-1]), query.device
    raise TypeError('`query` must be an int or a Tensor')


class UniformSampler(Sampler):
    """recstudio/ann/sampler.py:81-114: ids uniform in [1, num_items], int64 zero "log-probs"."""

    def forward(self, query: Union[Tensor, int], num_neg: int, pos_items: Optional[Tensor] = None,
                device: Optional[torch.device] = None):
        shape, dev = _query_shape(query, pos_items, device)
        nq = int(np.prod(shape))
        with torch.no_grad():
            neg = ops.sample_uniform(nq * num_neg, 1, self.num_items + 1, dev)
            neg = neg.view(*shape, num_neg)
            neg_prob = self.compute_item_p(None, neg)
            if pos_items is not None:
                return self.compute_item_p(None, pos_items), neg, neg_prob
            return neg, neg_prob

    def compute_item_p(self, query, pos_items):
        return ops.zero_logp_like(pos_items)        # sampler.py:113-114


class MaskedUniformSampler(Sampler):
    """recstudio/ann/sampler.py:187-214: uniform negatives excluding each user's history (rejection-free).
    BaseRetriever passes ``user_hist`` because the parameter is named in ``forward`` (baseretriever.py:225-228)."""

    def forward(self, query, num_neg, pos_items=None, user_hist=None):
        with torch.no_grad():
            if query.dim() == 2:
                neg = ops.sample_masked_uniform(user_hist, self.num_items, num_neg)
            elif query.dim() == 3:
                nq = query.size(1)
                neg = ops.sample_masked_uniform(user_hist, self.num_items, nq * num_neg).view(query.size(0), nq, num_neg)
            else:
                raise ValueError('`query` need to be 2-dimensional or 3-dimensional.')
            neg_prob = self.compute_item_p(query, neg)
            if pos_items is not None:
                return self.compute_item_p(query, pos_items), neg, neg_prob
            return neg, neg_prob

    def compute_item_p(self, query, pos_items):
        return ops.zero_logp_like(pos_items)            # -log(1), int64 like the reference (sampler.py:213-214)


def build_guide_table(table: Tensor, guide_log2: Optional[int] = None):
    """Cut-point ("guide") table for the fp32 CDF ``table``: guide[j] = first index i with
    table[i] >= j / K, K = 2**guide_log2, guide[K] = N.  Searching only inside
    [guide[b], guide[b+1]] for b = floor(u*K) returns exactly torch.searchsorted(table, u)
    (sampler.py:247): u*K is exact in fp32 (power-of-two scale) and the cut points j/K are compared with the
    fp32 CDF in float64, where both are exact."""
    n = table.numel()
    if guide_log2 is None:
        # ~1 item per bucket; LUT = 16 B per bucket: 134 MB at N = 1e7, 537 MB (the cap) at N = 1e8 -- measured best
        # of 2^23..2^26 there; 2^24 at N = 1e7 is slower than 2^23 (fewer searches but a wider random footprint)
        guide_log2 = int(min(25, max(4, int(np.ceil(np.log2(max(n, 2)))) - 1)))
    K = 1 << guide_log2
    cuts = torch.arange(K + 1, dtype=torch.float64) / K
    guide = torch.searchsorted(table.detach().cpu().to(torch.float64).contiguous(), cuts)
    guide[K] = n
    return guide.to(torch.int32), guide_log2


LINE_SLOTS = 12     # entry slots of one bucket line (rsa_common.hpp)


def build_cdf_lines(table: Tensor, pop_prob: Tensor, lines_log2: Optional[int] = None, max_bytes: int = 2 << 30,
                    overflow_target: float = 1e-2):
    """BUCKET LINES: the one-HBM-line form of ``torch.searchsorted(table, u)`` (layout: include/recstudio_amd.h,
    ``rsa_fused_args.cdf_lines``).  Bucket b covers u in [b, b+1) / 2**lines_log2; its 128-byte line lists the bucket's
    first distinct CDF values, then -- when there is room -- the first distinct entry ABOVE the bucket, each with its
    probability and its id as a 16-bit offset from the line's base id: 12 slots of {cdf fp32, prob fp32, delta u16} +
    base + count = 128 bytes.  The slot of a draw is #{cdf[i] < u}.  Items whose CDF value equals their predecessor's
    (zero probability, or a probability the fp32 cumsum absorbed) can never be returned by a lower-bound search and are
    left out, so a catalog where most items were never seen does not crowd the lines.  Cut points are compared in
    float64, where the fp32 CDF and b / 2**g are both exact -- same argument as ``build_guide_table``.

    ``lines_log2`` None: the smallest size (>= 2**4 buckets) for which at most ``overflow_target`` of the buckets
    (= of the draws, u being uniform) hold more than 11 distinct values (a 12th leaves no room for the entry above the
    bucket; a draw beyond the 12th falls back to a binary search), capped at ``max_bytes``.
    Returns (lines [2**g + 1, 32] float32 -- the last line is a sentinel closing the fallback ranges --, g)."""
    t = table.detach().cpu().to(torch.float32).contiguous()
    pp = pop_prob.detach().cpu().to(torch.float32).contiguous()
    n = t.numel()
    distinct = torch.ones(n, dtype=torch.bool)
    distinct[1:] = t[1:] > t[:-1]
    ids = torch.nonzero(distinct).flatten()                    # first index of every run of equal CDF values
    cdf = t[ids]
    nd = ids.numel()
    cdf64 = cdf.to(torch.float64)

    def cuts_of(g):
        K = 1 << g
        gd = torch.searchsorted(cdf64, torch.arange(K + 1, dtype=torch.float64) / K)     # first entry >= b / K
        gd[K] = nd
        return gd

    def crowded(g):
        c = cuts_of(g)
        return float(((c[1:] - c[:-1]) > LINE_SLOTS - 1).double().mean())

    if lines_log2 is None:
        g_max = max(4, int(np.floor(np.log2(max_bytes / 128))))
        g = int(min(g_max, max(4, int(np.ceil(np.log2(max(nd, 2) / 4.0))))))            # ~4 entries per bucket
        while g > 4 and crowded(g - 1) <= overflow_target:       # as small as the overflow target allows
            g -= 1
        while g < g_max and crowded(g) > overflow_target:
            g += 1
        lines_log2 = g
    gd = cuts_of(lines_log2)
    K = 1 << lines_log2
    lo, hi = gd[:-1], gd[1:]
    cnt = hi - lo
    last = n - 1
    as_f = lambda x: x.to(torch.int32).view(torch.float32)       # noqa: E731  int32 bit patterns in a float tensor
    lines = torch.zeros(K + 1, 32, dtype=torch.float32)
    slot_id = torch.zeros(K, LINE_SLOTS, dtype=torch.int64)
    for k in range(LINE_SLOTS):
        e = lo + k
        used = e <= hi                                            # real entries (e < hi) and the one above the bucket (e == hi)
        past = e >= nd                                            # nothing above: searchsorted returns n -> clamped to n - 1
        ec = e.clamp(max=nd - 1)
        idk = torch.where(past, torch.full_like(e, last), ids[ec])
        slot_id[:, k] = torch.where(used, idk, torch.zeros_like(idk))
        lines[:K, k] = torch.where(used & ~past, cdf[ec], torch.full((K,), float('inf')))
        lines[:K, 12 + k] = torch.where(used, pp[idk], torch.zeros(K))
    base = slot_id[:, 0]
    used_cols = torch.arange(LINE_SLOTS).view(1, -1) <= cnt.view(-1, 1)
    delta = torch.where(used_cols, slot_id - base.view(-1, 1), torch.zeros_like(slot_id))
    wide = (delta > 0xffff).any(1)                                # ids too far apart for 16-bit offsets: searched instead
    delta = delta.clamp(min=0, max=0xffff)
    packed = (delta[:, 0::2] | (delta[:, 1::2] << 16))            # two uint16 per word, even slot in the low half
    packed = torch.where(packed >= (1 << 31), packed - (1 << 32), packed)
    lines[:K, 24:30] = packed.to(torch.int32).view(torch.float32)
    # fallback range in `table`: [first id at or above the bucket's lower cut, the next line's]
    first = torch.where(lo < nd, ids[lo.clamp(max=nd - 1)], torch.full_like(lo, last))
    lines[:K, 30] = as_f(torch.where(wide, first, base))
    lines[:K, 31] = as_f(torch.where(wide, torch.full_like(cnt, -1), cnt))
    lines[K, 30] = as_f(torch.tensor([last]))[0]
    lines[K, :12] = float('inf')
    return lines, lines_log2


def _rebuild_derived(module, incompatible_keys):
    """load_state_dict post-hook of PopularSamplerModel (a module-level function: a lambda in the hook dict would make the
    module unpicklable -- torch.save(model), mp.spawn arguments)."""
    module._register_pairs()


class PopularSamplerModel(Sampler):
    """recstudio/ann/sampler.py:224-258.  The fp32 tables are built with the very same torch
    CPU ops as the reference's constructor (so they are bit-identical to its registered
    buffers) and uploaded with the module; a guide table accelerates the inverse-CDF search."""

    # derived lookup structures: rebuilt from pop_prob / table, never part of the state dict (the reference's
    # checkpoint holds exactly `pop_prob` and `table`, sampler.py:239-241)
    LINES_MIN_ITEMS = 1 << 16        # below this the tables live in L2 and every form costs the same

    def __init__(self, pop_count, scorer=None, mode=0, guide_log2=None, lookup='auto', lines_log2=None):
        """``lookup``: 'lines' (bucket lines, one HBM line per draw), 'lut' (16-byte direct-lookup table + 4-wide
        probe), 'guide' (guide table + binary search) or 'auto' (lines for catalogs of LINES_MIN_ITEMS items or
        more).  All return torch.searchsorted's index."""
        super().__init__(pop_count.shape[0], scorer)
        self.lookup, self._guide_log2_arg, self._lines_log2_arg = lookup, guide_log2, lines_log2
        with torch.no_grad():
            pop_count = torch.as_tensor(pop_count).detach().to('cpu', torch.float)
            if mode == 0:
                pop_count = torch.log(pop_count + 1)
            elif mode == 1:
                pop_count = torch.log(pop_count + 1) + 1e-6
            elif mode == 2:
                pop_count = pop_count ** 0.75
            pop_count[0] = 1                                              # sampler.py:237
            self.register_buffer('pop_prob', pop_count / pop_count.sum())
            self.register_buffer('table', torch.cumsum(self.pop_prob, dim=0))
            self.pop_prob[-1] = 1.0                                       # sampler.py:241
            self._register_pairs()
        self.register_load_state_dict_post_hook(_rebuild_derived)

    def _load_from_state_dict(self, state_dict, prefix, *args, **kwargs):
        # checkpoints of an earlier revision carried the derived `guide` buffer: not part of the state any more
        state_dict.pop(prefix + 'guide', None)
        super()._load_from_state_dict(state_dict, prefix, *args, **kwargs)

    def _use_lines(self):
        if self.lookup == 'auto':
            return self.table.numel() >= self.LINES_MIN_ITEMS
        return self.lookup == 'lines'

    @torch.no_grad()
    def _register_pairs(self):
        """(Re)build every derived buffer from ``table`` / ``pop_prob`` -- also after ``load_state_dict`` replaced them,
        so that the kernels never sample from a stale structure while ``compute_item_p`` reads the new ``pop_prob``.
        None of them is persistent: the state dict is the reference's (``pop_prob``, ``table``)."""
        dev = self.table.device
        table, prob = self.table.detach().cpu(), self.pop_prob.detach().cpu()
        # interleaved {table[i], pop_prob[i]} copy (binary-search fallbacks share cache lines with the probability)
        self.register_buffer('table_prob', torch.stack([table, prob], 1).contiguous().to(dev), persistent=False)
        guide = lut = lines = None
        self.guide_log2 = self.lines_log2 = 0
        if self._use_lines():
            lines, self.lines_log2 = build_cdf_lines(table, prob, self._lines_log2_arg)
        else:
            guide, self.guide_log2 = build_guide_table(table, self._guide_log2_arg)
            if self.lookup in ('auto', 'lut'):
                # direct-lookup table, one self-contained 16-B entry per guide bucket (layout: rsa_common.hpp,
                # cdf_lookup_lut): {lo | search bit, table[lo] or +inf, pop_prob[lo], pop_prob[lo+1]}
                last = table.numel() - 1
                lo = guide.to(torch.int64)
                hi = torch.cat([lo[1:], lo[-1:]])
                span = hi - lo
                g0, g1 = lo.clamp(max=last), (lo + 1).clamp(max=last)
                x = (lo - (span >= 2).to(torch.int64) * (1 << 31)).to(torch.int32)
                y = torch.where(span == 0, torch.full_like(table[g0], float('inf')), table[g0])
                lut = torch.stack([x.view(torch.float32), y, prob[g0], prob[g1]], 1).contiguous()
        for name, t in (('guide', guide), ('cdf_lut', lut), ('cdf_lines', lines)):
            self.register_buffer(name, None if t is None else t.to(dev), persistent=False)

    @classmethod
    def from_tables(cls, pop_prob, table, guide_log2=None, lookup='auto', lines_log2=None):
        """Build from already-computed reference buffers (e.g. a loaded RecStudio checkpoint's
        ``sampler.pop_prob`` / ``sampler.table``) instead of recomputing them from counts."""
        self = cls.__new__(cls)
        Sampler.__init__(self, table.numel(), None)
        self.lookup, self._guide_log2_arg, self._lines_log2_arg = lookup, guide_log2, lines_log2
        self.register_buffer('pop_prob', pop_prob.detach().clone().to(torch.float32))
        self.register_buffer('table', table.detach().clone().to(torch.float32))
        self._register_pairs()
        self.register_load_state_dict_post_hook(_rebuild_derived)
        return self

    def lookup_kwargs(self):
        """The popularity tables as keyword arguments of ``ops.fused_forward`` / ``ops.sample_popular``."""
        return dict(table=self.table, pop_prob=self.pop_prob, guide=self.guide, guide_log2=self.guide_log2,
                    table_prob=getattr(self, 'table_prob', None), cdf_lut=getattr(self, 'cdf_lut', None),
                    cdf_lines=getattr(self, 'cdf_lines', None), lines_log2=getattr(self, 'lines_log2', 0))

    def forward(self, query, num_neg, pos_items=None):
        with torch.no_grad():
            shape = tuple(query.shape[:-1])
            nq = int(np.prod(shape))
            neg, neg_prob = ops.sample_popular(self.table, self.pop_prob, self.guide, self.guide_log2, nq * num_neg,
                                               cdf_lut=getattr(self, 'cdf_lut', None),
                                               cdf_lines=getattr(self, 'cdf_lines', None),
                                               lines_log2=getattr(self, 'lines_log2', 0))
            neg = neg.view(*shape, num_neg)
            neg_prob = neg_prob.view(*shape, num_neg)
            if pos_items is not None:
                return self.compute_item_p(query, pos_items), neg, neg_prob
            return neg, neg_prob

    def compute_item_p(self, query, pos_items):
        return ops.item_logp(self.pop_prob, pos_items)                    # sampler.py:257-258


class MIDXSamplerUniform(Sampler):
    """recstudio/ann/sampler.py:261-388: negatives from a proposal that follows the query through two k-means half-codebooks,
    the final item uniform inside the chosen bucket.  ``update`` (once per epoch) runs the reference's Lloyd loop on
    ``rsa_kmeans_step``; ``forward`` is one launch of ``rsa_midx_sample`` (ids, log_neg_prob and log_pos_prob).  The uniforms are
    those of one ``torch.rand(M, n, 3)`` on the device generator, so the ids are distribution-equal to the reference's
    ``torch.multinomial`` draws, not stream-equal."""

    N_PARTS = 2
    EUCLIDEAN = False            # the Euclidean scorer weighs the items inside a bucket: the Pop classes

    def __init__(self, num_items, num_clusters, scorer_fn=None):
        from .scorer import CosineScorer, EuclideanScorer, InnerProductScorer
        allowed = (InnerProductScorer, CosineScorer) + ((EuclideanScorer,) if self.EUCLIDEAN else ())
        if scorer_fn is not None and type(scorer_fn) not in allowed:
            names = ', '.join(c.__name__ for c in allowed)
            raise NotImplementedError(f'{type(self).__name__}: scorer must be None or one of {names} (got {type(scorer_fn).__name__}'
                                      '; the Euclidean form draws by weight inside a bucket: MIDXSamplerPop / ClusterSamplerPop)')
        super().__init__(num_items, scorer_fn)
        if not 2 <= int(num_clusters) <= 64:
            raise ValueError(f'{type(self).__name__}: num_clusters must be in [2, 64], got {num_clusters}')
        self.K = int(num_clusters)
        self._cosine = isinstance(scorer_fn, CosineScorer)

    # -------------------------------------------------------------- update
    def _centre_names(self):
        return ('c0', 'c1')

    @torch.no_grad()
    def _rows(self, X, idx):
        """Rows ``idx`` of the (normalised, for the cosine scorer) table, as the Lloyd loop seeds centres from them."""
        rows = X[idx.to(X.device)]
        return torch.nn.functional.normalize(rows, dim=-1) if self._cosine else rows

    @torch.no_grad()
    def update(self, item_embs, max_iter=30):
        X = item_embs.detach()
        if not X.is_cuda or X.dtype != torch.float32 or X.dim() != 2:
            raise RuntimeError(f'{type(self).__name__}.update: item_embs must be an fp32 [N, d] tensor on the GPU')
        N, d = X.shape
        P, K = self.N_PARTS, self.K
        if d % 8 or d > 256:
            raise ValueError(f'{type(self).__name__}: embed_dim must be a multiple of 8 and at most 256, got {d}')
        dsub = d // P
        names = self._centre_names()
        C = []
        for p, name in enumerate(names):                       # kmeans(): given centres, or K random rows (half 0 first)
            if hasattr(self, name):
                C.append(getattr(self, name).detach().to(X.device, torch.float32))
            else:
                C.append(self._rows(X, torch.randperm(N)[:K])[:, p * dsub:(p + 1) * dsub])
        C = torch.stack(C).contiguous()
        prev = [np.inf] * P
        live = [True] * P
        assign = torch.empty(P, N, dtype=torch.int32, device=X.device)
        for _ in range(max_iter):
            a, sums, counts, loss = ops.kmeans_step(X, C, normalize=self._cosine)
            loss = loss.tolist()
            counts_f = counts.to(torch.float32)
            C_next = C.clone()
            for p in range(P):
                if not live[p]:
                    continue
                assign[p] = a[p]
                if (prev[p] - loss[p]) < prev[p] * 1e-6:        # sampler.py:27: centres and assignment of this pass
                    live[p] = False
                    continue
                prev[p] = loss[p]
                C_next[p] = sums[p] / counts_f[p].unsqueeze(-1)
                dead = counts[p] == 0
                ndead = int(dead.sum())
                if ndead:                                       # sampler.py:32-34, ascending cluster order
                    C_next[p][dead] = self._rows(X, torch.randperm(N)[:ndead])[:, p * dsub:(p + 1) * dsub]
            C = C_next
            if not any(live):
                break
        self._build_index(C, assign.to(torch.int64))
        self._update(X)

    def _update(self, X):
        """What follows the index in the reference's ``_update``: nothing for the uniform forms (``wkk`` is the bucket counts)."""

    def _draw_tables(self):
        """The in-bucket tables handed to the draw kernel: none, the item is uniform in its bucket."""
        return {}

    @torch.no_grad()
    def _build_index(self, C, cd):
        """The reference's attributes (names, dtypes) from the centres [P, K, d_sub] and assignments [P, N], plus the compact
        device copies the kernel reads (derived, rebuilt by every update)."""
        P, K = self.N_PARTS, self.K
        dev = C.device
        for p, name in enumerate(self._centre_names()):
            setattr(self, name, C[p].clone())
            setattr(self, name + '_', torch.cat([C.new_zeros(1, C.shape[2]), C[p]], dim=0))
        shifted = [torch.cat([cd.new_zeros(1), cd[p] + 1]) for p in range(P)]
        if P == 2:
            self.cd0, self.cd1 = shifted
            bucket = cd[0] * K + cd[1]
        else:
            self.cd, = shifted
            bucket = cd[0]
        nb = K ** P
        self.indices = torch.sort(bucket, stable=True)[1]                      # construct_index, sampler.py:38-45
        count = torch.bincount(bucket, minlength=nb)
        self.indptr = torch.cat([count.new_zeros(1), count.cumsum(0)])
        self.wkk = count.to(torch.float32).view(K, K) if P == 2 else count.to(torch.float32)
        self._centres = C.contiguous()
        self._cd32 = [c.to(torch.int32) for c in shifted]
        self._indices32, self._indptr32 = self.indices.to(torch.int32), self.indptr.to(torch.int32)
        self._wkk_dev = self.wkk.to(dev).contiguous()

    # -------------------------------------------------------------- draw
    def _check_ready(self):
        if not hasattr(self, '_centres'):
            raise RuntimeError(f'{type(self).__name__}: call update(item_embs) before sampling (fit does, once per epoch)')

    def forward(self, query, num_neg, pos_items=None):
        self._check_ready()
        with torch.no_grad():
            if query.dim() not in (2, 3):
                raise ValueError('`query` need to be 2-dimensional or 3-dimensional.')
            if query.dim() == 3 and pos_items is not None:
                raise ValueError(f'{type(self).__name__}: a 3-dimensional query takes no pos_items (the reference fails in view_as)')
            lead = tuple(query.shape[:-1])
            pos2 = None
            if pos_items is not None:
                if pos_items.dim() not in (1, 2) or pos_items.shape[0] != query.shape[0]:
                    raise ValueError('`pos_items` must be [B] or [B, T]')
                pos2 = pos_items.reshape(query.shape[0], -1)
            out = ops.midx_sample(query.detach().reshape(-1, query.shape[-1]), self._centres, self._wkk_dev, self._indptr32,
                                  self._indices32, self._cd32, int(num_neg), pos_ids=pos2, cosine=self._cosine,
                                  **self._draw_tables())
            neg, neg_prob = out['neg_ids'].view(*lead, num_neg), out['neg_logp'].view(*lead, num_neg)
            if pos_items is not None:
                return out['pos_logp'].view(pos_items.shape), neg, neg_prob
            return neg, neg_prob

    def compute_item_p(self, query, pos_items):
        """log-proposal (unnormalised) of ``pos_items`` [B] / [B, T] under ``query`` [B, d]: the draw kernel with no draws."""
        self._check_ready()
        with torch.no_grad():
            q = query.detach().reshape(-1, query.shape[-1])
            out = ops.midx_sample(q, self._centres, None, None, None, self._cd32, 0, pos_ids=pos_items.reshape(q.shape[0], -1),
                                  cosine=self._cosine, **self._draw_tables())
            return out['pos_logp'].view(pos_items.shape)


class ClusterSamplerUniform(MIDXSamplerUniform):
    """recstudio/ann/sampler.py:426-510: the same with ONE codebook over the whole vector (``c``, ``cd``, ``wkk`` [K])."""

    N_PARTS = 1

    def _centre_names(self):
        return ('c',)


class _PopInBucket:
    """The popularity-in-bucket form shared by ``MIDXSamplerPop`` and ``ClusterSamplerPop`` (recstudio/ann/sampler.py:391-423,
    :533-559): the final item is drawn inside the chosen bucket in proportion to a weight -- the transformed popularity, times
    exp(-||x||^2 / 2) with an ``EuclideanScorer`` -- and ``log`` of that weight enters both log-probabilities.

    ``pop_count`` holds N entries, the counts of ids 1 .. N (``item_freq[1:]``, no padding entry), as the reference's ``_update``
    requires; ``num_items`` is therefore N - 1 as in the reference (where nothing reads it either).  ``update`` builds the
    reference's ``p`` [N + 1], ``cp`` [N] and weighted ``wkk`` on ``rsa_midx_weights``.

    DEVIATION: the draw is the one that agrees with ``compute_item_p`` -- position = first with ``cp > u`` inside the bucket,
    ``id = indices[pos] + 1``, ``log_neg_prob = logits + log p[id]`` -- not the reference's ``_sample_item_with_pop``
    (``sampler.py:349-365``), which returns ids without the ``+ 1``, reads ``p`` at the sorted position and clamps an in-bucket
    offset against an absolute position."""

    EUCLIDEAN = True

    def __init__(self, pop_count: Tensor, num_clusters, scorer=None, mode=1):
        super().__init__(pop_count.shape[0], num_clusters, scorer)
        from .scorer import EuclideanScorer
        self._euclidean = isinstance(scorer, EuclideanScorer)
        if mode == 0:                                           # sampler.py:399-404
            pop_count = torch.log(pop_count + 1)
        elif mode == 1:
            pop_count = torch.log(pop_count + 1) + 1e-6
        elif mode == 2:
            pop_count = pop_count ** 0.75
        self.pop_count = torch.nn.Parameter(pop_count, requires_grad=False)

    @torch.no_grad()
    def update(self, item_embs, max_iter=30):
        if item_embs.dim() == 2 and self.pop_count.shape[0] != item_embs.shape[0]:
            raise ValueError(f'{type(self).__name__}: pop_count has {self.pop_count.shape[0]} entries for {item_embs.shape[0]} rows '
                             'of item_embs; it takes one count per item id 1 .. N and none for the padding id: item_freq[1:]')
        super().update(item_embs, max_iter)

    @torch.no_grad()
    def _update(self, X):
        P, K = self.N_PARTS, self.K
        pop = self.pop_count.detach().to(X.device, torch.float32)
        self.p, self._logp, wkk, self.cp = ops.midx_weights(pop, self._indptr32, self._indices32, K, P,
                                                            table=X if self._euclidean else None, dim=X.shape[1])
        self.wkk = wkk.view(K, K) if P == 2 else wkk
        self._wkk_dev = wkk

    def _draw_tables(self):
        return dict(cp=self.cp, item_logp=self._logp)


class MIDXSamplerPop(_PopInBucket, MIDXSamplerUniform):
    """recstudio/ann/sampler.py:391-423: ``MIDXSamplerUniform`` with the popularity-weighted item inside the bucket."""


class ClusterSamplerPop(_PopInBucket, ClusterSamplerUniform):
    """recstudio/ann/sampler.py:533-559: ``ClusterSamplerUniform`` with the popularity-weighted item inside the bucket."""


class LSHSampler(UniformSampler):
    """recstudio/ann/sampler.py:562-707: negatives from the union of the query's buckets in ``n_table`` sign-random-projection
    hash tables of ``n_bits`` bits each, with the collision probability ``1 - (1 - p^K)^L`` in the log-proposal.  ``update`` (once
    per epoch) hashes the table on ``rsa_lsh_hash`` and builds the reference's ``indices`` [L, N] / ``indptr`` [L, 2^K + 1] (int64,
    a stable sort per table); ``forward`` is one launch of ``rsa_lsh_sample``.  The uniforms are those of the reference's one
    ``torch.rand(B, num_neg)`` on the device generator, so a query with a non-empty bucket gets the reference's ids.

    DEVIATIONS:
    * a query whose buckets are all empty draws uniformly over 1 .. N from its own uniforms of that call (log-probability 0);
      the reference spends a separate ``torch.randint`` on those rows, which shifts the stream -- distribution-equal;
    * without ``pos_items`` the reference returns the ids before that patch and ``log(inf)`` for such rows; here both forms
      return the patched ids and 0;
    * the cosine is clamped to [-1, 1] (the reference's ``acos`` returns NaN past it), and the position ``floor(u * len)`` to
      ``len - 1`` also where ``float(len)`` rounds above ``len``;
    * ``1 - (1 - p^K)^L`` is evaluated as ``-expm1(L * log1p(-p^K))`` in double, without the reference's fp32 cancellation."""

    def __init__(self, num_items: int, n_dims: int, n_bits: int = 4, n_table: int = 16, device='cuda', scorer_fn=None):
        from .scorer import InnerProductScorer
        if scorer_fn is not None and type(scorer_fn) is not InnerProductScorer:
            raise NotImplementedError(f'LSHSampler: scorer must be None or InnerProductScorer, got {type(scorer_fn).__name__}')
        super().__init__(num_items, scorer_fn)
        n_dims, n_bits, n_table = int(n_dims), int(n_bits), int(n_table)
        if n_dims % 8 or not 8 <= n_dims <= 256:
            raise ValueError(f'LSHSampler: n_dims must be a multiple of 8 and at most 256, got {n_dims}')
        if not 1 <= n_bits <= 16 or n_table < 1 or n_bits * n_table > 64:
            raise ValueError(f'LSHSampler: n_bits must be in [1, 16] and n_bits * n_table at most 64, got {n_bits} * {n_table}')
        self.n_dims, self.n_bits, self.n_table, self.device = n_dims, n_bits, n_table, device
        w = torch.rand(n_dims, n_bits, n_table)                                 # sampler.py:680-683, the CPU generator
        self.weight_vectors = torch.nn.Parameter((w / torch.norm(w, dim=0, keepdim=True)).to(device), requires_grad=False)
        base = torch.from_numpy(1 << np.arange(n_bits - 1, -1, -1)).type(torch.float).to(device)
        self.K_base_vec = torch.nn.Parameter(base, requires_grad=False)
        self.indptr, self.indices = None, None
        self.item_embs = None

    @torch.no_grad()
    def update(self, item_embs):
        X = item_embs.detach()
        if not X.is_cuda or X.dtype != torch.float32 or X.dim() != 2 or X.shape[1] != self.n_dims:
            raise RuntimeError(f'LSHSampler.update: item_embs must be an fp32 [N, {self.n_dims}] tensor on the GPU')
        W = self.weight_vectors.detach().to(X.device)
        codes = ops.lsh_hash(X, W).to(torch.int64)                              # [L, N]
        self.item_embs = X.clone()
        # construct_index per table (sampler.py:38-45, :686-707)
        self.indices = torch.sort(codes, dim=1, stable=True)[1]
        nb = 1 << self.n_bits
        rows = torch.arange(self.n_table, device=X.device).unsqueeze(1)
        count = torch.bincount((codes + rows * nb).flatten(), minlength=self.n_table * nb).view(self.n_table, nb)
        self.indptr = torch.cat([count.new_zeros(self.n_table, 1), count.cumsum(1)], dim=1)
        self._indices32, self._indptr32 = self.indices.to(torch.int32), self.indptr.to(torch.int32)

    def forward(self, query, num_neg, pos_items=None):
        if self.item_embs is None:
            raise RuntimeError('LSHSampler: call update(item_embs) before sampling (fit does, once per epoch)')
        if not isinstance(query, Tensor) or query.dim() != 2:
            raise ValueError('LSHSampler: `query` need to be 2-dimensional.')
        with torch.no_grad():
            out = ops.lsh_sample(query.detach(), self.weight_vectors.detach(), self._indptr32, self._indices32, self.item_embs,
                                 int(num_neg), eps=1e-12 if pos_items is not None else 0.0)
            if pos_items is not None:
                return ops.zero_logp_like(pos_items), out['neg_ids'], out['neg_logp']
            return out['neg_ids'], out['neg_logp']


def sampler_kind(sampler):
    """rsa_sampler_kind of the plugin the kernels draw from themselves, None for every other one.  Exact types only: a
    subclass may override ``forward``, and must then go through the plugin path."""
    if type(sampler) is UniformSampler:
        return nat.SAMPLER_UNIFORM
    if type(sampler) is PopularSamplerModel:
        return nat.SAMPLER_POPULAR
    return None


class RetrieverSampler(Sampler):
    """recstudio/ann/sampler.py:61-78 (IRGAN): negatives drawn by ANOTHER retriever's ``sampling(method=...)`` --
    by default from its softmax over the whole catalog ('brute'), scored on the full-score kernels."""

    def __init__(self, num_items, retriever=None, method='brute', t=1):
        super().__init__(num_items)
        self.retriever, self.method, self.T = retriever, method, t

    def update(self, item_embs, max_iter=30):
        self.retriever._update_item_vector()

    def forward(self, batch, num_neg, pos_items=None, excluding_hist=False):
        (log_pos_prob, neg_id, log_neg_prob), _ = self.retriever.sampling(
            batch=batch, num_neg=num_neg, excluding_hist=excluding_hist, method=self.method, return_query=False, t=self.T)
        return log_pos_prob.detach(), neg_id.detach(), log_neg_prob.detach()
