"""CPU: the referee of the LSH sampler (tests/lsh_referee.py) is pinned to the reference's own recorded behaviour
(tests/golden/lsh.npz, tools/make_golden_lsh.py), five seeded mistakes land outside its judgement, and the new entry points are
declared, bound and validate their arguments without a GPU."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import lsh_referee as R

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CASES = ['a', 'b']


@pytest.fixture(scope='module')
def gold():
    z = np.load(os.path.join(HERE, 'golden', 'lsh.npz'))
    return {k: torch.from_numpy(z[k]) for k in z.files}


def case(gold, name):
    g = {k.split('.', 1)[1]: v for k, v in gold.items() if k.startswith(name + '.')}
    g['N'], g['d'], g['K'], g['L'], g['B'], g['n'] = (int(v) for v in g['shape'])
    return g


def recorded_codes(indptr, indices):
    """Item codes [N, L] read back from the recorded index: the bucket that holds the item."""
    L, N = indices.shape
    codes = torch.empty(N, L, dtype=torch.int64)
    for l in range(L):
        codes[indices[l], l] = torch.searchsorted(indptr[l].contiguous(), torch.arange(N), right=True) - 1
    return codes


def loop_draw(qcodes, indptr, indices, u, n_items, strict=False, tables=None, plus_one=True):
    """The draw rule of include/recstudio_amd.h, one element at a time; the keyword arguments seed the mistakes below."""
    M, n = u.shape
    L = qcodes.shape[1]
    ids = torch.zeros(M, n, dtype=torch.int64)
    lens = torch.zeros(M, dtype=torch.int64)
    for m in range(M):
        start = [int(indptr[l, qcodes[m, l]]) for l in range(L)]
        cnt = [int(indptr[l, qcodes[m, l] + 1]) - start[l] for l in range(L)]
        cum = np.cumsum(cnt).tolist()
        ln = sum(cnt[l] for l in (tables if tables is not None else range(L)))
        lens[m] = ln
        for j in range(n):
            uj = np.float32(u[m, j].item())
            if ln == 0:
                ids[m, j] = 1 + min(int(np.floor(np.float32(uj * np.float32(n_items)))), n_items - 1)
                continue
            r = min(int(np.floor(np.float32(uj * np.float32(ln)))), ln - 1)
            t = sum(1 for l in range(L) if (cum[l] < r if strict else cum[l] <= r))
            t = min(t, L - 1)
            pos = start[t] + r - (cum[t - 1] if t > 0 else 0)
            ids[m, j] = int(indices[t, max(0, min(pos, n_items - 1))]) + (1 if plus_one else 0)
    return ids, lens


# ---------------------------------------------------------------- surface
def test_sampler_is_exported():
    import recstudio_amd as ra
    from recstudio_amd import sampler
    assert 'LSHSampler' in sampler.__all__ and ra.LSHSampler is sampler.LSHSampler
    s = ra.LSHSampler(101, 16, 4, 5, device='cpu')
    assert tuple(s.weight_vectors.shape) == (16, 4, 5) and not s.weight_vectors.requires_grad
    assert torch.equal(s.K_base_vec.data, torch.tensor([8., 4., 2., 1.]))
    assert list(s.state_dict()) == ['weight_vectors', 'K_base_vec'] and s.num_items == 100
    assert s.indptr is None and s.indices is None and s.item_embs is None
    torch.manual_seed(5)
    a = ra.LSHSampler(101, 16, 4, 5, device='cpu').weight_vectors
    torch.manual_seed(5)
    w = torch.rand(16, 4, 5)
    assert torch.equal(a.data, w / torch.norm(w, dim=0, keepdim=True))          # the reference's construction, same stream
    with pytest.raises(RuntimeError, match='update'):
        s(torch.zeros(2, 16), 3)
    with pytest.raises(NotImplementedError, match='InnerProductScorer'):
        ra.LSHSampler(101, 16, scorer_fn=ra.CosineScorer())
    ra.LSHSampler(101, 16, device='cpu', scorer_fn=ra.InnerProductScorer())
    with pytest.raises(ValueError, match='n_bits'):
        ra.LSHSampler(101, 16, 5, 13, device='cpu')


def test_entry_points_are_declared_and_bound():
    from recstudio_amd import _native as nat
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'recstudio_amd.h')).read(), flags=re.S)
    for name in ('rsa_lsh_hash', 'rsa_lsh_sample', 'rsa_lsh_lookup'):
        assert re.search(r'\b' + name + r'\s*\(', text) and name in nat.SIGNATURES
    assert 'rsa_lsh_hash_args' in nat.STRUCTS and 'rsa_lsh_args' in nat.STRUCTS
    assert 'log_eps' in [f[0] for f in nat.LshArgs._fields_]
    assert nat.lib().rsa_abi_version() == 13


def test_arguments_are_validated_without_a_gpu():
    from recstudio_amd import _native as nat
    lib = nat.lib()
    for fn, cls in ((lib.rsa_lsh_sample, nat.LshArgs), (lib.rsa_lsh_lookup, nat.LshArgs), (lib.rsa_lsh_hash, nat.LshHashArgs)):
        a = cls()
        a.size = 0
        assert fn(ctypes.byref(a), None) == -1 and b'size' in lib.rsa_last_error()
        a = cls()
        a.dim, a.n_bits, a.n_table = 16, 5, 13
        assert fn(ctypes.byref(a), None) == -1 and b'n_bits * n_table' in lib.rsa_last_error()
        a.n_bits, a.n_table = 17, 1
        assert fn(ctypes.byref(a), None) == -1 and b'n_bits must be in [1, 16]' in lib.rsa_last_error()
        a.n_bits, a.n_table = 0, 1
        assert fn(ctypes.byref(a), None) == -1 and b'n_bits' in lib.rsa_last_error()
        for dim in (12, 264, 0):
            a.dim, a.n_bits, a.n_table = dim, 4, 16
            assert fn(ctypes.byref(a), None) == -1 and b'dim must be a multiple of 8' in lib.rsa_last_error()
    a = nat.LshArgs()
    a.dim, a.n_bits, a.n_table, a.n_queries, a.num_neg, a.n_items = 16, 4, 16, 2, 3, 10
    assert lib.rsa_lsh_sample(ctypes.byref(a), None) == -1 and b'is null' in lib.rsa_last_error()
    a.num_neg = 0                                             # nothing to draw: no pointer is needed
    assert lib.rsa_lsh_sample(ctypes.byref(a), None) == 0
    h = nat.LshHashArgs()
    h.dim, h.n_bits, h.n_table, h.n_rows = 16, 4, 16, 5
    assert lib.rsa_lsh_hash(ctypes.byref(h), None) == -1 and b'is null' in lib.rsa_last_error()
    h.n_rows = 0
    assert lib.rsa_lsh_hash(ctypes.byref(h), None) == -1 and b'n_rows' in lib.rsa_last_error()


# ---------------------------------------------------------------- the recorded reference
@pytest.mark.parametrize('name', CASES)
def test_referee_reproduces_the_recorded_index(gold, name):
    g = case(gold, name)
    codes, decided = R.hash_codes(g['item_embs'], g['weight_vectors'])
    assert bool(decided.all()) and bool(R.projections(g['query'], g['weight_vectors'])[1].all())    # the fixture's promise
    assert torch.equal(codes, recorded_codes(g['indptr'], g['indices']))
    indptr, indices = R.build_index(codes, g['K'])
    assert indptr.dtype == torch.int64 and indices.dtype == torch.int64
    assert torch.equal(indptr, g['indptr']) and torch.equal(indices, g['indices'])
    assert R.judge_codes(codes, g['item_embs'], g['weight_vectors']) == (0, 0.0)


@pytest.mark.parametrize('name', CASES)
def test_referee_reproduces_the_recorded_draw(gold, name):
    g = case(gold, name)
    N, d, K, L = g['N'], g['d'], g['K'], g['L']
    qcodes, _ = R.hash_codes(g['query'], g['weight_vectors'])
    ids, items, ln, _ = R.draw(qcodes, g['indptr'], g['indices'], g['u'], N)
    full = ln > 0
    if name == 'b':
        assert int(full.sum()) > 0 and int((~full).sum()) > 0
    else:
        assert bool(full.all())
    assert torch.equal(ids[full], g['neg'][full])
    assert torch.equal(ids, loop_draw(qcodes, g['indptr'], g['indices'], g['u'], N)[0])
    assert bool(((ids >= 1) & (ids <= N)).all())
    # rows without a bucket: the reference's own uniform ids and log-probability 0
    assert bool(((g['neg'][~full] >= 1) & (g['neg'][~full] <= N)).all()) and bool((g['log_neg_prob'][~full] == 0).all())
    assert g['log_pos_prob'].dtype == torch.int64 and bool((g['log_pos_prob'] == 0).all())
    # the recorded log-probabilities are the reference's fp32 evaluation: R.reference_logp_interval derives their bound
    lo, hi, slack, small = R.reference_logp_interval(g['query'], g['item_embs'], items, ln, K, L, 1e-12)
    got = g['log_neg_prob'].double()
    assert float(small.double().mean()) <= 0.10               # what is not compared may cover at most a tenth of a case
    ok = R.inside(got, lo, hi, slack(got)) | small
    print(name, 'skipped share', float(small.double().mean()), 'widest interval', float((hi - lo)[~small].max()))
    assert bool(ok[full].all())


# ---------------------------------------------------------------- seeded mistakes
def test_mistakes_land_outside_the_judgement(gold):
    g = case(gold, 'a')
    N, K, L, W = g['N'], g['K'], g['L'], g['weight_vectors']
    X = g['item_embs'].clone()
    X[7] = 0                                                  # a row whose every projection is exactly 0
    s, decided = R.projections(X, W)
    assert bool(decided.all())
    good = R.codes_of_bits(s > 0)
    assert R.judge_codes(good, X, W)[0] == 0 and bool((good[7] == 0).all())
    # 1. bit order reversed (the first bit taken as the least significant)
    assert R.judge_codes(R.codes_of_bits((s > 0).flip(1)), X, W)[0] > 0
    # 2. >= for >
    assert R.judge_codes(R.codes_of_bits(s >= 0), X, W)[0] == K * L
    # the draw, on uniforms that sit on every table boundary
    indptr, indices = g['indptr'], g['indices']
    qcodes, _ = R.hash_codes(g['query'], W)
    start, cum, ln = R.buckets(qcodes, indptr)
    rows = []
    for m in range(qcodes.shape[0]):
        us, rs = R.boundary_uniforms(ln[m], cum[m])
        assert len(us) >= 2
        rows.append(us)
    n = min(len(r) for r in rows)
    u = torch.tensor([r[:n] for r in rows], dtype=torch.float32)
    ids, items, ln2, t = R.draw(qcodes, indptr, indices, u, N)
    assert torch.equal(ids, loop_draw(qcodes, indptr, indices, u, N)[0]) and int(t.max()) > 0
    # 3. cum_l < r for <=
    assert not torch.equal(ids, loop_draw(qcodes, indptr, indices, u, N, strict=True)[0])
    # 4. the id without the + 1
    assert not torch.equal(ids, loop_draw(qcodes, indptr, indices, u, N, plus_one=False)[0])
    # 5. len over the wrong set of tables: other ids, and a log-probability outside every interval
    wrong_ids, wrong_len = loop_draw(qcodes, indptr, indices, g['u'], N, tables=range(L - 1))
    ids_u, items_u, ln_u, _ = R.draw(qcodes, indptr, indices, g['u'], N)
    assert bool((wrong_len < ln_u).all()) and not torch.equal(wrong_ids, ids_u)
    lo, hi, c = R.logp_interval(g['query'], g['item_embs'], items_u, ln_u, K, L, 0.0)
    mistaken = R.F(c, K, L, wrong_len.view(-1, 1), 0.0)
    assert not bool(R.inside(mistaken, lo, hi, 1e-5).any())
    assert bool(R.inside(R.F(c, K, L, ln_u.view(-1, 1), 0.0), lo, hi, 0.0).all())


def test_boundary_uniforms_hit_their_targets():
    cum = torch.tensor([3, 3, 10, 17, 17])
    us, rs = R.boundary_uniforms(17, cum)
    assert rs == [2, 3, 9, 10, 16]
    for u, r in zip(us, rs):
        assert 0 <= u < 1 and int(np.floor(np.float32(np.float32(u) * np.float32(17)))) == r
    assert R.boundary_uniforms(0, torch.tensor([0, 0])) == ([], [])


def test_weight_is_monotone_and_free_of_cancellation():
    c = torch.linspace(-1, 1, 2001, dtype=torch.float64)
    for K, L in ((4, 16), (1, 1), (16, 4), (2, 32)):
        w = R.collision_weight(c, K, L)
        assert bool((w[1:] >= w[:-1]).all()) and float(w[0]) == 0.0 and float(w[-1]) == 1.0
        p = 1 - torch.acos(c) / math.pi
        tiny = p ** K < 1e-9
        assert bool(((w[tiny] - L * p[tiny] ** K).abs() <= 1e-6 * L * p[tiny] ** K + 1e-300).all())
