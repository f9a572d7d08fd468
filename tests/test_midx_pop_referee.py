"""CPU: the float64 referee of the popularity-in-bucket samplers (tests/midx_pop_referee.py) is pinned to the reference's own
recorded tables and compute_item_p (tests/golden/midx_pop.npz, tools/make_golden_midx_pop.py), an fp32 emulation of the new step
stays within half of every bound, six seeded mistakes land far outside, an exact tie takes the next positive-weight position, and
the new ABI fields, rsa_midx_weights and the classes' surface are checked without a GPU."""
import ctypes
import inspect
import os

import numpy as np
import pytest
import torch

import midx_referee as R
import midx_pop_referee as PR

HERE = os.path.dirname(os.path.abspath(__file__))
K = 4
# (case, parts, scorer, mode)
CASES = [('midx_pop_ip_m1', 2, 'ip', 1), ('midx_pop_cos_m0', 2, 'cos', 0), ('midx_pop_euc_m2', 2, 'euc', 2),
         ('cluster_pop_ip_m1', 1, 'ip', 1), ('cluster_pop_euc_m1', 1, 'euc', 1)]


@pytest.fixture(scope='module')
def gold():
    z = np.load(os.path.join(HERE, 'golden', 'midx.npz'))
    out = {k: torch.from_numpy(z[k]) for k in z.files}
    z = np.load(os.path.join(HERE, 'golden', 'midx_pop.npz'))
    out.update({k: torch.from_numpy(z[k]) for k in z.files})
    return out


def case_inputs(gold, name, parts, scorer, mode):
    """(X as clustered and weighed, pop fp32 [N], centres, cd, indices, indptr) of a recorded case."""
    X = gold['item_embs'] * (float(gold['euc_scale']) if name == 'midx_pop_euc_m2' else 1.0)
    pop = PR.transform(gold['pop_counts'], mode)
    if parts == 2:
        c, cd = torch.stack([gold[f'{name}.c0'], gold[f'{name}.c1']]), [gold[f'{name}.cd0'], gold[f'{name}.cd1']]
    else:
        c, cd = gold[f'{name}.c'].unsqueeze(0), [gold[f'{name}.cd']]
    return X, pop, c, cd, gold[f'{name}.indices'], gold[f'{name}.indptr']


def recorded_item_p(gold, name, key, ids):
    """The recorded compute_item_p in the shape of ``ids``.  The reference's ClusterSamplerPop returns [B, B] for a 1-D pos_items
    (sampler.py:487-499: r is reshaped to [B] and then added to log p of the [B, 1] view); entry [i, i] is id i's own value."""
    got = gold[f'{name}.{key}'].double()
    if got.numel() != ids.numel():
        assert got.shape == (ids.numel(), ids.numel())
        got = got.diagonal()
    return got.reshape(ids.shape)


def fixture_bounds(t, X, euclid):
    """(wkk bound [B], cp bound [N], relative p bound [N]) between two fp32 implementations (the referee's docstring).  The
    recorded popularity transform is torch's fp32 log / pow on the CPU that recorded it; another CPU's vector math library may
    round the last bit the other way, so the transform itself is compared at TRANSFORM_REL, not bit for bit."""
    cnt = t['cnt'].double()
    wkk_b = 2 * (cnt + 2) * R.U32 * t['wkk']
    cp_b = 2 * (2 * (cnt[t['bucket']] + 2) + 1) * R.U32
    if euclid:
        ss = (X.double() ** 2).sum(1)
        p_rel = torch.expm1((X.shape[1] + 1) * R.U32 * 0.5 * ss) + 4 * R.U32
    else:
        p_rel = torch.zeros(X.shape[0], dtype=torch.float64)
    return wkk_b, cp_b, p_rel + PR.TRANSFORM_REL


@pytest.mark.parametrize('name,parts,scorer,mode', CASES)
def test_referee_reproduces_the_recorded_tables(gold, name, parts, scorer, mode):
    X, pop, c, cd, indices, indptr = case_inputs(gold, name, parts, scorer, mode)
    w64, _ = PR.weights64(pop, X if scorer == 'euc' else None)
    t = PR.tables64(w64, indices, indptr)
    wkk_b, cp_b, p_rel = fixture_bounds(t, X, scorer == 'euc')
    p_ref, cp_ref, wkk_ref = gold[f'{name}.p'].double(), gold[f'{name}.cp'].double(), gold[f'{name}.wkk'].double().reshape(-1)
    assert p_ref.shape == (X.shape[0] + 1,) and float(p_ref[0]) == 1.0
    if scorer != 'euc':                                                      # the transform itself
        assert bool(((gold[f'{name}.p'][1:].double() - pop.double()).abs() <= PR.TRANSFORM_REL * pop.double()).all())
    assert bool(((p_ref[1:] - w64).abs() <= p_rel * w64 + PR.TINY).all())
    err = (wkk_ref - t['wkk']).abs()
    print(name, 'wkk error / bound', float((err / wkk_b.clamp_min(1e-300)).max()))
    assert bool((err <= wkk_b + (p_rel.max() * t['wkk'])).all())
    err = (cp_ref - t['cp']).abs()
    print(name, 'cp error / bound', float((err / cp_b).max()))
    assert bool((err <= cp_b + 2 * p_rel.max()).all())
    assert int((t['wkk'] == 0).sum()) == int((wkk_ref == 0).sum())           # empty buckets only: no NaN was recorded


@pytest.mark.parametrize('name,parts,scorer,mode', CASES)
def test_referee_reproduces_compute_item_p(gold, name, parts, scorer, mode):
    X, pop, c, cd, indices, indptr = case_inputs(gold, name, parts, scorer, mode)
    w64, _ = PR.weights64(pop, X if scorer == 'euc' else None)
    t = PR.tables64(w64, indices, indptr)
    _, _, p_rel = fixture_bounds(t, X, scorer == 'euc')
    tab = R.tables(gold['query'], c, t['wkk'].view(K, K) if parts == 2 else t['wkk'], scorer == 'cos')
    dsub = c.shape[2]
    seen_inf = 0
    for key, ids in (('p1', gold['pos1'].view(-1, 1)), ('p2', gold['pos2'])):
        val, bound = R.item_logp(tab, cd, ids)
        bound = bound * (R.gamma(dsub + 2) / R.gamma(dsub // 4 + 3))          # the recorded side is a sequential fp32 sum
        lp = t['logp'][ids]
        fin = torch.isfinite(lp)
        lpf = torch.where(fin, lp, torch.zeros_like(lp))
        rel = torch.cat([p_rel.new_zeros(1), p_rel])[ids]
        # log of a p that is off by rel, torch.log at 1 ulp (2 u |log|), and the final addition
        bound = bound + rel + 2 * R.U32 * lpf.abs() + R.U32 * (val + lpf).abs()
        got = recorded_item_p(gold, name, key, ids)
        assert bool(((got - (val + lpf)).abs()[fin] <= bound[fin]).all())
        assert bool((got[~fin] == -np.inf).all())
        seen_inf += int((~fin).sum())
        assert bool((got[ids == 0] == 0).all()) and int((ids == 0).sum()) > 0
    if mode == 0:
        assert seen_inf > 0                                                    # a positive id of weight 0 was recorded


EMU = [c for c in CASES if c[0] != 'cluster_pop_euc_m1'] + [CASES[4]]


def emu_inputs(gold, name, parts, scorer, mode, n, seed, edges=True):
    X, pop, c, cd, indices, indptr = case_inputs(gold, name, parts, scorer, mode)
    w64, wb = PR.weights64(pop, X if scorer == 'euc' else None)
    w = w64.float()
    assert bool(((w.double() - w64).abs() <= wb).all())
    t = PR.tables64(w, indices, indptr)
    wkk64 = t['wkk'].view(K, K) if parts == 2 else t['wkk']
    q = gold['query']
    tab = R.tables(q, c, wkk64, scorer == 'cos')
    g = torch.Generator().manual_seed(seed)
    u = PR.edge_uniforms(tab, t, indptr, n, parts, g) if edges else torch.rand(q.shape[0], n, parts + 1, generator=g)
    counts = R.build_index([x[1:] - 1 for x in cd], K)[2]
    return q, c, cd, indices, indptr, w, counts, u


@pytest.mark.parametrize('name,parts,scorer,mode', EMU)
def test_fp32_emulation_stays_within_half_of_every_bound(gold, name, parts, scorer, mode):
    q, c, cd, indices, indptr, w, counts, u = emu_inputs(gold, name, parts, scorer, mode, 24, 31)
    ids, logp = PR.emulate_draws(q, c, counts, indptr, indices, cd, w, u, scorer == 'cos')
    p, logp_tab, wkk, cp = PR.emulate_tables(w, indices, indptr)
    t = PR.tables64(w, indices, indptr)
    assert bool(((cp.double() - t['cp']).abs() <= 0.5 * PR.cp_bound(t)).all())
    # (wkk is ONE rounding of its double sum, and the bound is that rounding's own worst case, u relative: nothing correct can
    # promise half of it, so the whole bound is asked here; cp rounds a value below 1 against an absolute u, which leaves half)
    assert bool(((wkk.double() - t['wkk']).abs() <= PR.wkk_bound(t)).all())
    res = PR.judge_all(q, c, wkk, cp, logp_tab, w, indptr, indices, cd, ids, u, logp, scorer == 'cos')
    print(name, res)
    assert not R.violations(res)
    # (the edges are exact ties of a float64 boundary: the excess there is 0, every other draw keeps half a tolerance)
    assert all(v <= 0.5 for k_, v in res.items() if k_.endswith('_ratio'))


@pytest.mark.parametrize('mistake,check', [
    ('p_by_position', ('logp',)), ('no_plus_one', ('cdf0', 'cdf1', 'inbucket', 'own_index')),
    ('uniform_in_bucket', ('inbucket', 'own_index')), ('logp_missing', ('logp',)), ('wkk_counts', ('cdf0', 'cdf1')),
    ('zero_weight_drawn', ('zero_weight', 'inbucket'))])
@pytest.mark.parametrize('name,parts,scorer,mode', [CASES[1], ('cluster_pop_ip_m1', 1, 'ip', 0)])    # (mode 0: weights of 0)
def test_seeded_mistakes_land_far_outside(gold, name, parts, scorer, mode, mistake, check):
    q, c, cd, indices, indptr, w, counts, u = emu_inputs(gold, name, parts, scorer, mode, 40, 13, edges=False)
    ids, logp = PR.emulate_draws(q, c, counts, indptr, indices, cd, w, u, scorer == 'cos', mistake=mistake)
    p, logp_tab, wkk, cp = PR.emulate_tables(w, indices, indptr)
    res = PR.judge_all(q, c, wkk, cp, logp_tab, w, indptr, indices, cd, ids.clamp(0, indices.numel()), u, logp, scorer == 'cos')
    print(mistake, res)
    bad = R.violations(res)
    assert any(key in bad for key in check), (mistake, res)
    # at least 10x outside some bound
    assert max(res.get(key + '_ratio', 0.0) for key in check) >= 10, (mistake, res)


def test_a_tie_takes_the_next_positive_weight_position():
    """u2 exactly equal to a cp value: the upper bound, the next position of positive weight; zero weights are never returned,
    at u2 = 0 and u2 = 1 - 2^-24 either."""
    w = torch.tensor([0.0, 2.0, 0.0, 0.0, 1.0, 1.0, 0.0])                   # one bucket: cp = 0 .5 .5 .5 .75 1 1
    indices, indptr = torch.arange(7), torch.tensor([0, 7, 7])
    centres = torch.zeros(1, 2, 8)
    cd = [torch.tensor([0, 1, 1, 1, 1, 1, 1, 1])]
    top = 1.0 - 2.0 ** -24
    u2 = torch.tensor([0.0, 0.25, 0.5, float(np.nextafter(np.float32(0.5), np.float32(0))), 0.75, top])
    u = torch.stack([torch.full_like(u2, 0.3), u2], 1).view(1, -1, 2)
    ids, _ = PR.emulate_draws(torch.zeros(1, 8), centres, torch.tensor([7.0, 0.0]), indptr, indices, cd, w, u, False)
    assert ids.view(-1).tolist() == [2, 2, 5, 2, 6, 6]
    p, logp_tab, wkk, cp = PR.emulate_tables(w, indices, indptr)
    assert cp.tolist() == [0.0, 0.5, 0.5, 0.5, 0.75, 1.0, 1.0] and wkk.tolist() == [4.0, 0.0]
    t = PR.tables64(w, indices, indptr)
    res = PR.judge_items(t, cp, indptr, indices, cd, 2, ids, u[..., 1])
    assert not R.violations(res), res
    got = PR.own_index(cp, indptr, torch.zeros(6, dtype=torch.long), u2)
    assert got.tolist() == [1, 1, 4, 1, 5, 5]


# ------------------------------------------------------------------------------------------------- ABI, no GPU
@pytest.fixture(scope='module')
def nat():
    from recstudio_amd import _native
    if not os.path.exists(_native.LIB_PATH):
        _native.build()
    return _native


def midx_block(nat, **kw):
    a = nat.MidxArgs()
    p = ctypes.c_void_p(4096)
    a.query = a.centres = a.wkk = a.indptr = a.indices = a.cd0 = a.cd1 = a.neg_ids = a.u_in = p
    a.n_queries, a.dim, a.n_parts, a.n_clusters, a.num_neg, a.n_items, a.grid_threads = 4, 16, 2, 4, 3, 100, 256
    for k_, v in kw.items():
        setattr(a, k_, v)
    return a


@pytest.mark.parametrize('entry', ['rsa_midx_sample', 'rsa_midx_lookup'])
def test_cp_and_item_logp_go_together(nat, entry):
    lib = nat.lib()
    assert nat.MidxArgs._fields_[-2:] == [('cp', ctypes.c_void_p), ('item_logp', ctypes.c_void_p)]
    assert nat.ABI_VERSION == 13
    for kw in (dict(cp=4096), dict(item_logp=4096)):
        assert getattr(lib, entry)(ctypes.byref(midx_block(nat, **kw)), None) == -1
        assert b'cp' in lib.rsa_last_error()
    # the other checks still come first with both set
    assert getattr(lib, entry)(ctypes.byref(midx_block(nat, cp=4096, item_logp=4096, n_clusters=65)), None) == -1
    assert b'n_clusters' in lib.rsa_last_error()


def weights_block(nat, **kw):
    a = nat.MidxWeightsArgs()
    p = ctypes.c_void_p(4096)
    a.pop = a.table = a.indptr = a.indices = a.p = a.item_logp = a.wkk = a.cp = p
    a.n_items, a.row_stride, a.dim, a.n_parts, a.n_clusters = 100, 16, 16, 2, 4
    for k_, v in kw.items():
        setattr(a, k_, v)
    return a


@pytest.mark.parametrize('kw,msg', [(dict(n_clusters=65), b'n_clusters'), (dict(n_clusters=1), b'n_clusters'), (dict(dim=12), b'dim'),
                                    (dict(dim=264), b'dim'), (dict(size=0), b'size'), (dict(n_parts=3), b'n_parts'),
                                    (dict(pop=None), b'null'), (dict(indices=None), b'null'), (dict(indptr=None), b'null'),
                                    (dict(p=None), b'null'), (dict(item_logp=None), b'null'), (dict(wkk=None), b'null'),
                                    (dict(cp=None), b'null'), (dict(row_stride=18), b'row_stride'), (dict(row_stride=8), b'row_stride'),
                                    (dict(row_offset=-1), b'row_offset'), (dict(n_items=0), b'n_items'),
                                    (dict(n_items=2 ** 31), b'n_items'), (dict(table=4100), b'aligned')])
def test_weights_entry_validates_before_any_launch(nat, kw, msg):
    lib = nat.lib()
    assert lib.rsa_midx_weights(ctypes.byref(weights_block(nat, **kw)), None) == -1
    assert msg in lib.rsa_last_error()
    assert lib.rsa_midx_weights(None, None) == -1
    assert nat.MidxWeightsArgs._fields_[0] == ('size', ctypes.c_int64)


# ------------------------------------------------------------------------------------------------- class surface
def test_classes_follow_the_reference_surface(gold):
    import recstudio_amd as ra
    from recstudio_amd import sampler
    counts = gold['pop_counts']
    for cls, base in ((ra.MIDXSamplerPop, ra.MIDXSamplerUniform), (ra.ClusterSamplerPop, ra.ClusterSamplerUniform)):
        assert cls.__name__ in sampler.__all__ and issubclass(cls, base)
        assert list(inspect.signature(cls.__init__).parameters) == ['self', 'pop_count', 'num_clusters', 'scorer', 'mode']
        assert inspect.signature(cls.__init__).parameters['scorer'].default is None
        assert inspect.signature(cls.__init__).parameters['mode'].default == 1
        s = cls(counts.clone(), 4)
        assert s.num_items == counts.numel() - 1 and s.K == 4 and sampler.sampler_kind(s) is None        # N - 1, as the reference
        assert isinstance(s.pop_count, torch.nn.Parameter) and not s.pop_count.requires_grad
        assert [n for n, _ in s.named_parameters()] == ['pop_count']
        c = counts.float()
        for mode, want in ((0, torch.log(c + 1)), (1, torch.log(c + 1) + 1e-6), (2, c ** 0.75), (3, counts)):
            got = cls(counts.clone(), 4, mode=mode).pop_count
            assert torch.equal(got.data, want) and (mode == 3 or got.dtype == torch.float32)
        for sc in (ra.InnerProductScorer(), ra.CosineScorer(), ra.EuclideanScorer()):
            cls(counts.clone(), 4, sc)
            cls(counts.clone(), 4, scorer=sc, mode=0)
        with pytest.raises(NotImplementedError):
            cls(counts.clone(), 4, object())
        with pytest.raises(NotImplementedError):
            base(counts.numel() + 1, 4, ra.EuclideanScorer())                  # the uniform forms still refuse it
        with pytest.raises(ValueError):
            cls(counts.clone(), 65)
        with pytest.raises(RuntimeError, match='update'):
            s(torch.zeros(2, 16), 3)
        with pytest.raises(RuntimeError, match='update'):
            s.compute_item_p(torch.zeros(2, 16), torch.ones(2, dtype=torch.long))
        long = cls(torch.cat([counts.new_zeros(1), counts]), 4)                # item_freq with the padding entry
        with pytest.raises(ValueError, match=r'item_freq\[1:\]'):
            long.update(torch.zeros(counts.numel(), 16))
