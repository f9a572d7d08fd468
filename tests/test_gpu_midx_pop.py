"""GPU: the popularity-in-bucket samplers (rsa_midx_weights, the weighted draw of rsa_midx_sample / rsa_midx_lookup, MIDXSamplerPop /
ClusterSamplerPop) against the float64 referee of tests/midx_pop_referee.py: the per-epoch tables, EVERY draw inside its float64
intervals (codebook stages and in-bucket stage) with exact edges in half the uniforms, the recorded reference tables through
``update``, the device random stream, the untouched uniform path, and two epochs of ``fit``."""
import os

import numpy as np
import pytest
import torch

import midx_referee as R
import midx_pop_referee as PR
from test_gpu_midx import Book, queries, synthetic_book
from test_midx_pop_referee import CASES, case_inputs, fixture_bounds, recorded_item_p

pytestmark = pytest.mark.gpu
DEV = 'cuda'
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope='module')
def ra():
    import recstudio_amd
    recstudio_amd._native.lib()
    torch.cuda.init()
    return recstudio_amd


@pytest.fixture(scope='module')
def gold():
    out = {}
    for f in ('midx.npz', 'midx_pop.npz'):
        z = np.load(os.path.join(HERE, 'golden', f))
        out.update({k: torch.from_numpy(z[k]) for k in z.files})
    return out


def mode0_weights(book, seed):
    """log(count + 1) over counts with zeros, and one non-empty bucket (not the only one) whose items all weigh 0."""
    g = torch.Generator().manual_seed(seed)
    counts = torch.randint(0, 6, (book.n_items,), generator=g)
    cnt = (book.indptr[1:] - book.indptr[:-1]).cpu()
    full = torch.nonzero(cnt > 0).flatten()
    assert full.numel() >= 2
    b = int(full[full.numel() // 2])
    planted = book.indices[int(book.indptr[b]):int(book.indptr[b + 1])].cpu()
    counts[planted] = 0
    assert int((counts == 0).sum()) > planted.numel()
    return PR.transform(counts, 0).to(DEV), b


def own_tables(book, w, table=None):
    from recstudio_amd import ops
    return ops.midx_weights(w, book.indptr.int(), book.indices.int(), book.K, book.P, table=table)


def judge_pop(book, query, w, own, ids, u, logp, cosine=False):
    p, logp_tab, wkk, cp = own
    res = PR.judge_all(query, book.centres, wkk, cp, logp_tab, w, book.indptr, book.indices, book.cd, ids, u, logp, cosine)
    assert not R.violations(res), res
    return res


# (parts, d, K, M, n, N with the padding id)
SHAPES = [(2, 8, 2, 3, 5, 50), (1, 16, 4, 7, 70, 301), (2, 128, 64, 257, 64, 100003), (1, 64, 2, 33, 100, 20011),
          (2, 256, 64, 5, 3, 5001)]


@pytest.mark.parametrize('parts,d,K,M,n,N', SHAPES)
def test_every_weighted_draw_inside_its_float64_intervals(ra, parts, d, K, M, n, N):
    from recstudio_amd import ops
    book = synthetic_book(parts, d, K, N - 1, seed=d + K)
    w, planted = mode0_weights(book, N)
    own = own_tables(book, w)
    p, logp_tab, wkk, cp = own
    assert float(wkk[planted]) == 0.0 and int(book.wkk.reshape(-1)[planted]) > 0       # a non-empty bucket of weight 0
    q = queries(M, d, 3)
    t = PR.tables64(w, book.indices, book.indptr)
    tab = R.tables(q, book.centres, (wkk.view(K, K) if parts == 2 else wkk), False)
    u = PR.edge_uniforms(tab, t, book.indptr, n, parts, torch.Generator().manual_seed(K * 1000 + n))
    on_cp = torch.isin(u[..., parts], cp)
    print('in-bucket uniforms at 0 / top / on a cp value', int((u[..., parts] == 0).sum()), int((u[..., parts] == 1 - 2.0 ** -24).sum()),
          int(on_cp.sum()), 'of', M * n)
    edge = on_cp | (u[..., parts] == 0) | (u[..., parts] == 1 - 2.0 ** -24)            # (a bucket's last cp, 1, is clamped to the top)
    assert int(edge.sum()) >= M * n // 8                                               # half the slots, a third of the edges
    g = torch.Generator().manual_seed(N)
    pos = torch.randint(0, N, (M, 3), generator=g).to(DEV)
    pos[0, 0] = 0
    pos[0, 1] = int(book.indices[int(book.indptr[planted])]) + 1                       # a positive of weight 0: -inf
    out = ops.midx_lookup(q, *book.kernel_args()[:1], wkk, *book.kernel_args()[2:], u, pos_ids=pos, cp=cp, item_logp=logp_tab)
    res = judge_pop(book, q, w, own, out['neg_ids'], u, out['neg_logp'])
    print((parts, d, K, M, n, N), res)
    assert bool(torch.isfinite(out['neg_logp']).all())
    bad, ratio = PR.judge_logp(tab, logp_tab, book.cd, pos, out['pos_logp'])
    assert bad == 0, ratio
    assert float(out['pos_logp'][0, 0]) == 0.0 and float(out['pos_logp'][0, 1]) == -np.inf


# ------------------------------------------------------------------------------------------------- rsa_midx_weights
def explicit_book(parts, K, sizes, d, seed):
    """A codebook state whose buckets have the given sizes (in bucket order), the items shuffled over them."""
    g = torch.Generator().manual_seed(seed)
    bucket = torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes))
    bucket = bucket[torch.randperm(bucket.numel(), generator=g)]
    assign = [bucket // K, bucket % K] if parts == 2 else [bucket]
    return Book(torch.randn(parts, K, d // parts, generator=g), assign)


def check_tables(book, w, own, X=None):
    """p, logp, wkk, cp of the kernel against float64, and the exact properties the draw relies on."""
    p, logp_tab, wkk, cp = own
    N = book.n_items
    w64, wb = PR.weights64(w, X)
    assert p.shape == (N + 1,) and logp_tab.shape == (N + 1,) and cp.shape == (N,) and wkk.numel() == book.K ** book.P
    assert float(p[0]) == 1.0 and float(logp_tab[0]) == 0.0
    err = (p[1:].double() - w64).abs()
    print('weight error / bound', float((err / wb.clamp_min(1e-300)).max()) if X is not None else 0.0)
    assert bool((err <= wb).all())
    lp = torch.log(p.double())
    fin = torch.isfinite(lp)
    assert torch.equal(logp_tab[~fin].double(), lp[~fin])                              # log 0 = -inf, as the reference's
    assert bool(((logp_tab.double() - lp).abs()[fin] <= ((R.U32 + 2.0 ** -52) * lp.abs() + PR.TINY)[fin]).all())
    t = PR.tables64(p[1:], book.indices, book.indptr)                                   # from the kernel's OWN fp32 weights
    err = (wkk.double() - t['wkk']).abs()
    assert bool((err <= PR.wkk_bound(t)).all())
    err = (cp.double() - t['cp']).abs()
    print('cp error / bound', float((err / PR.cp_bound(t)).max()))
    assert bool((err <= PR.cp_bound(t)).all())
    # exact: a bucket's cp never decreases, stays put across a weight of 0, ends at 1; a bucket of weight 0 is 0 throughout
    indptr = book.indptr.long()
    first = torch.zeros(N, dtype=torch.bool, device=DEV)
    first[indptr[:-1][indptr[:-1] < N]] = True
    prev = torch.where(first, torch.zeros_like(cp), torch.cat([cp.new_zeros(1), cp[:-1]]))
    assert bool((cp >= prev).all())
    zero = t['wpos'] == 0
    assert bool((cp[zero] == prev[zero]).all()) and int(zero.sum()) > 0
    last = indptr[1:][indptr[1:] > indptr[:-1]] - 1
    tot = t['wkk'][t['bucket'][last]]
    assert bool((cp[last][tot > 0] == 1).all()) and bool((cp[last][tot == 0] == 0).all())
    assert bool((wkk[t['wkk'] == 0] == 0).all())
    return t


# (parts, K, d, bucket sizes or N, what)
def weight_cases():
    many = [0, 5, 1, 0, 300, 64, 0, 2, 8192, 8193, 0, 16385, 1, 0, 0, 7]              # the chunk of 8192 positions: at, over, two over
    return [('small', 2, 4, 16, many, False, False), ('euclid', 2, 4, 16, many, True, False),
            ('euclid_view', 1, 16, 64, many, True, True), ('cluster2', 1, 2, 8, [10000, 10010], False, False)]


@pytest.mark.parametrize('name,parts,K,d,sizes,euclid,view', weight_cases())
def test_midx_weights_against_float64(ra, name, parts, K, d, sizes, euclid, view):
    book = explicit_book(parts, K, sizes, d, seed=len(sizes) + d)
    N = book.n_items
    g = torch.Generator().manual_seed(N)
    counts = torch.randint(0, 9, (N,), generator=g)
    if len(sizes) > 4:
        counts[book.indices[int(book.indptr[4]):int(book.indptr[5])].cpu()] = 0       # a non-empty bucket of weight 0
    w = PR.transform(counts, 0 if not euclid else 2).to(DEV)
    X = None
    if euclid:
        W = torch.randn(N + 1, d, generator=g)
        W = W / W.norm(dim=1, keepdim=True) * torch.sqrt(torch.rand(N + 1, 1, generator=g) * 250.0)       # ||x||^2 in [0, 250)
        W = W.to(DEV)
        X = W[1:] if view else W[1:].clone()
        if view:
            assert X.data_ptr() != X._base.data_ptr()
        ss = (X.double() ** 2).sum(1)
        assert float(ss.max()) > 240 and int((ss < 5).sum()) > 0
    own = own_tables(book, w, X)
    again = own_tables(book, w, X)
    for a, b in zip(own, again):
        assert torch.equal(a, b), 'two runs differ'
    check_tables(book, w, own, X)
    if euclid:
        under = (own[0][1:] == 0) & (w > 0)
        print('weights that underflowed', int(under.sum()), 'subnormal', int(((own[0] > 0) & (own[0] < 2.0 ** -126)).sum()))
        assert int(under.sum()) > 0


# ------------------------------------------------------------------------------------------------- update, recorded reference
@pytest.mark.parametrize('name,parts,scorer,mode', CASES)
def test_update_against_the_recorded_reference(ra, gold, name, parts, scorer, mode):
    X, pop, c_ref, cd_ref, indices_ref, indptr_ref = case_inputs(gold, name, parts, scorer, mode)
    Xd = X.to(DEV)
    d = X.shape[1]
    K = 4
    sc = dict(ip=ra.InnerProductScorer, cos=ra.CosineScorer, euc=ra.EuclideanScorer)[scorer]()
    cls = ra.MIDXSamplerPop if parts == 2 else ra.ClusterSamplerPop
    s = cls(gold['pop_counts'].clone(), K, sc, mode=mode).to(DEV)
    assert torch.equal(s.pop_count.cpu(), pop)
    scale = float(gold['euc_scale']) if name == 'midx_pop_euc_m2' else 1.0
    init = gold['init_cos' if scorer == 'cos' else 'init_rows'] * scale
    if parts == 1:
        s.c = init[:K].clone()
    else:
        s.c0, s.c1 = init[:K, :d // 2].clone(), init[K:, d // 2:].clone()
    s.update(Xd, max_iter=30)
    for a in (('cd0', 'cd1') if parts == 2 else ('cd',)) + ('indices', 'indptr'):
        assert torch.equal(getattr(s, a).cpu(), gold[f'{name}.{a}']), a
    w64, wb = PR.weights64(pop, X if scorer == 'euc' else None)
    t = PR.tables64(w64, indices_ref, indptr_ref)
    wkk_b, cp_b, p_rel = fixture_bounds(t, X, scorer == 'euc')
    assert s.p.shape == gold[f'{name}.p'].shape and s.cp.shape == gold[f'{name}.cp'].shape and s.wkk.shape == gold[f'{name}.wkk'].shape
    assert s.p.dtype == s.cp.dtype == s.wkk.dtype == torch.float32
    p, cp, wkk = s.p.cpu().double(), s.cp.cpu().double(), s.wkk.cpu().double().reshape(-1)
    if scorer != 'euc':                                          # the kernel hands the weights on as they are
        assert torch.equal(s.p[1:].cpu(), s.pop_count.detach().cpu()) and float(s.p[0]) == 1.0
    assert bool(((p[1:] - w64).abs() <= wb).all())
    assert bool(((p - gold[f'{name}.p'].double()).abs()[1:] <= (p_rel + R.U32) * w64 + PR.TINY).all())
    err = (wkk - gold[f'{name}.wkk'].double().reshape(-1)).abs()
    print(name, 'wkk error / bound', float((err / wkk_b.clamp_min(1e-300)).max()))
    assert bool((err <= wkk_b + p_rel.max() * t['wkk']).all())
    err = (cp - gold[f'{name}.cp'].double()).abs()
    print(name, 'cp error / bound', float((err / cp_b).max()))
    assert bool((err <= cp_b + 2 * p_rel.max()).all())
    # compute_item_p: ours within the kernel's bound of the float64 value, the recorded one within the reference's
    q = gold['query'].to(DEV)
    centres = torch.stack([getattr(s, n_) for n_ in (('c0', 'c1') if parts == 2 else ('c',))])
    tab = R.tables(q, centres, s.wkk, scorer == 'cos')
    cd = [c.to(DEV) for c in cd_ref]
    dsub = centres.shape[2]
    # our centres are an fp32 mean of their own: within twice centre_bound of the recorded ones, which moves a logit by |q| . bound
    x64 = R.normalize64(X) if scorer == 'cos' else X.double()
    cb = 2 * R.centre_bound(x64, torch.stack([c[1:] - 1 for c in cd_ref]), c_ref)
    assert bool(((centres.cpu().double() - c_ref.double()).abs() <= cb).all())
    qh = (R.normalize64(q) if scorer == 'cos' else q.double()).abs()
    moved = [torch.cat([qh.new_zeros(qh.shape[0], 1), qh[:, p_ * dsub:(p_ + 1) * dsub] @ cb[p_].t().to(DEV)], 1) for p_ in range(parts)]
    for key, ids in (('p1', gold['pos1']), ('p2', gold['pos2'])):
        got = s.compute_item_p(q, ids.to(DEV))
        assert got.shape == ids.shape
        ids2 = ids.view(ids.shape[0], -1).to(DEV)
        bad, ratio = PR.judge_logp(tab, s._logp, cd, ids2, got.view(ids2.shape))
        assert bad == 0, ratio
        ref = recorded_item_p(gold, name, key, ids2.cpu()).to(DEV)
        val, bound = R.item_logp(tab, cd, ids2)
        lp = s._logp.double()[ids2]
        fin = torch.isfinite(lp)
        lpf = torch.where(fin, lp, torch.zeros_like(lp))
        rel = torch.cat([p_rel.new_zeros(1), p_rel]).to(DEV)[ids2]
        shift = sum(m.gather(1, c[ids2]) for m, c in zip(moved, cd))
        # ours + the recorded side's logits, log p of two weights u (+ rel) apart, two logs, two additions
        both = bound * (1 + R.gamma(dsub + 2) / R.gamma(dsub // 4 + 3)) + shift + rel + R.U32 + 4 * R.U32 * lpf.abs() \
            + 2 * R.U32 * (val + lpf).abs()
        assert bool(((got.view(ids2.shape).double() - ref).abs()[fin] <= both[fin]).all())
        assert torch.equal(got.view(ids2.shape)[~fin].double(), ref[~fin])
        assert bool((got.view(ids2.shape)[ids2 == 0] == 0).all())
    if mode == 0:
        assert bool(torch.isinf(s.compute_item_p(q, gold['pos2'].to(DEV))).any())


# ------------------------------------------------------------------------------------------------- stream, classes
@pytest.mark.parametrize('parts,scorer', [(2, 'ip'), (1, 'cos'), (2, 'euc'), (1, 'euc')])
def test_sample_follows_the_device_stream_and_agrees_with_compute_item_p(ra, gold, parts, scorer):
    from recstudio_amd import ops
    X = (gold['item_embs'] * (0.3 if scorer == 'euc' else 1.0)).to(DEV)
    sc = dict(ip=ra.InnerProductScorer, cos=ra.CosineScorer, euc=ra.EuclideanScorer)[scorer]()
    cls = ra.MIDXSamplerPop if parts == 2 else ra.ClusterSamplerPop
    s = cls(gold['pop_counts'].clone(), 4, sc, mode=0).to(DEV)
    torch.manual_seed(0)
    s.update(X)
    M, n = 9, 37
    q = queries(M, 16, 8)
    state = (s._centres, s._wkk_dev, s._indptr32, s._indices32, s._cd32)
    gen = torch.cuda.default_generators[torch.cuda.current_device()]
    torch.manual_seed(17)
    before = gen.get_state()
    out = ops.midx_sample(q, *state, n, cosine=scorer == 'cos', want_u=True, cp=s.cp, item_logp=s._logp)
    end = gen.get_offset()
    gen.set_state(before)
    want_u = torch.rand(M, n, parts + 1, device=DEV)
    assert torch.equal(out['u'], want_u), 'uniforms differ from torch.rand(M, n, P + 1) on the device stream'
    assert gen.get_offset() == end, 'the generator does not end where the torch call ends'
    gen.set_state(before)
    neg, lp = s(q, n)                                           # the class draws the same ids from the same state
    assert torch.equal(neg, out['neg_ids']) and torch.equal(lp, out['neg_logp']) and gen.get_offset() == end
    twin = ops.midx_lookup(q, *state, out['u'], cosine=scorer == 'cos', cp=s.cp, item_logp=s._logp)
    assert torch.equal(twin['neg_ids'], neg) and torch.equal(twin['neg_logp'], lp)
    book = Book(s._centres.cpu(), [c[1:].cpu().long() - 1 for c in s._cd32])
    w = s.p[1:]
    res = judge_pop(book, q, w, (s.p, s._logp, s.wkk, s.cp), neg, out['u'], lp, cosine=scorer == 'cos')
    print(parts, scorer, res)
    assert int(neg.min()) >= 1 and int(neg.max()) <= X.shape[0] and bool((s.p[neg] > 0).all())
    # the consistency the reference lacks: log_neg_prob IS compute_item_p of the drawn ids
    again = s.compute_item_p(q, neg)
    tab = R.tables(q, book.centres, s.wkk, scorer == 'cos')
    bad, ratio = PR.judge_logp(tab, s._logp, book.cd, neg, again)
    assert bad == 0, ratio                                      # (lp itself was judged against the same values above)
    print('log_neg_prob == compute_item_p bit for bit:', bool(torch.equal(again, lp)))
    # shapes and restrictions of the uniform classes
    q3 = q[:6].view(2, 3, 16)
    neg3, lp3 = s(q3, 5)
    assert neg3.shape == (2, 3, 5) and lp3.shape == (2, 3, 5)
    with pytest.raises(ValueError):
        s(q3, 5, torch.ones(2, 3, dtype=torch.long, device=DEV))
    pos1 = torch.tensor([0, 5, 300, 7, 0, 1, 2, 3, 4], device=DEV)
    lpp, neg, lp = s(q, 4, pos1)
    assert lpp.shape == (M,) and float(lpp[0]) == 0.0 and torch.equal(lpp, s.compute_item_p(q, pos1))


@pytest.mark.parametrize('parts', [2, 1])
def test_uniform_path_is_untouched(ra, gold, parts):
    """cp / item_logp null: rsa_midx_lookup returns what the Uniform class returns for the same uniforms, bit for bit."""
    from recstudio_amd import ops
    X = gold['item_embs'].to(DEV)
    cls = ra.MIDXSamplerUniform if parts == 2 else ra.ClusterSamplerUniform
    s = cls(X.shape[0] + 1, 4, ra.InnerProductScorer())
    torch.manual_seed(0)
    s.update(X)
    q = queries(9, 16, 8)
    pos = torch.randint(0, 301, (9, 2), generator=torch.Generator().manual_seed(1)).to(DEV)
    torch.manual_seed(23)
    lpp, neg, lp = s(q, 37, pos)
    torch.manual_seed(23)
    u = torch.rand(9, 37, parts + 1, device=DEV)
    out = ops.midx_lookup(q, s._centres, s._wkk_dev, s._indptr32, s._indices32, s._cd32, u, pos_ids=pos, cp=None, item_logp=None)
    assert torch.equal(out['neg_ids'], neg) and torch.equal(out['neg_logp'], lp) and torch.equal(out['pos_logp'], lpp)
    tab = R.tables(q, s._centres, s.wkk, False)
    book = Book(s._centres.cpu(), [c[1:].cpu().long() - 1 for c in s._cd32])
    res = R.judge_draws(tab, book.wkk, book.indptr, book.indices, book.cd, neg, u, lp)
    assert not R.violations(res), res                           # (item_index: the uniform in-bucket rule, exact)
    with pytest.raises(ValueError, match='cp'):
        ops.midx_lookup(q, s._centres, s._wkk_dev, s._indptr32, s._indices32, s._cd32, u, cp=torch.zeros(300, device=DEV))


# ------------------------------------------------------------------------------------------------- end to end
def test_fit_two_epochs_with_the_midx_pop_sampler(ra, golden):
    """BPR's towers with SampledSoftmaxLoss and MIDXSamplerPop over item_freq[1:] on ml-100k (the uniform form's test with the
    popularity-weighted bucket): finite losses, the second epoch's lower, every id in 1 .. N."""
    from test_dataset_golden import make
    import logging
    g = golden('data_ml100k')
    ds = make(ra.TripletDataset, g)
    trn, val, _ = ds.build(split_ratio=[0.8, 0.1, 0.1], shuffle=True)
    cfg = {'train': {'epochs': 2, 'negative_count': 16, 'batch_size': 512, 'learning_rate': 0.001},
           'eval': {'batch_size': 256}, 'model': {'embed_dim': 64}}
    freq = trn.item_freq[1:]
    assert freq.numel() == trn.num_items - 1
    sampler = ra.MIDXSamplerPop(freq, 8, ra.InnerProductScorer(), mode=1)
    tables = []
    plain_update = sampler.update

    def update(item_embs, max_iter=30):
        plain_update(item_embs, max_iter)
        tables.append((sampler.c0.clone(), sampler.cp.clone()))
    sampler.update = update
    model = ra.BPR(cfg, loss=ra.SampledSoftmaxLoss(), sampler=sampler)
    losses = []

    class Grab(logging.Handler):
        def emit(self, record):
            if 'train_loss=' in record.getMessage():
                losses.append(float(record.getMessage().split('train_loss=')[1].split()[0]))
    model.logger.addHandler(Grab())
    model.logger.setLevel(logging.INFO)
    model.fit(trn, val)
    print('epoch losses', losses)
    assert len(losses) == 2 and all(np.isfinite(losses)) and losses[1] < losses[0]
    assert len(tables) == 2 and not torch.equal(tables[0][0], tables[1][0])
    batch = next(iter(trn.train_loader(batch_size=64, shuffle=False)))
    batch = model._to_device(batch, next(model.parameters()).device)
    out = model.forward(batch, return_query=True, return_neg_id=True)
    lp = out['score']['log_neg_prob']
    assert bool(torch.isfinite(lp).all()) and int(out['neg_id'].min()) >= 1 and int(out['neg_id'].max()) <= trn.num_items - 1
    assert torch.equal(lp, sampler.compute_item_p(out['query'], out['neg_id']))
    assert not sampler.pop_count.requires_grad and torch.equal(sampler.pop_count.cpu(), torch.log(freq.float() + 1) + 1e-6)
