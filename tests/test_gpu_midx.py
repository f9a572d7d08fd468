"""GPU: the adaptive samplers (rsa_midx_sample / rsa_midx_lookup, rsa_kmeans_step, MIDXSamplerUniform / ClusterSamplerUniform)
against the float64 referee of tests/midx_referee.py: the device random stream, the twin entry, EVERY draw inside its float64
interval, the Lloyd step, ``update`` against the recorded reference, and two epochs of ``fit``."""
import os

import numpy as np
import pytest
import torch

import midx_referee as R

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
    z = np.load(os.path.join(HERE, 'golden', 'midx.npz'))
    return {k: torch.from_numpy(z[k]) for k in z.files}


class Book:
    """A codebook state on the device, as ``update`` leaves it: centres [P, K, dsub], cd (int64 [N + 1] per part), index."""

    def __init__(self, centres, assign):
        P, K, _ = centres.shape
        self.P, self.K = P, K
        self.centres = centres.float().contiguous().to(DEV)
        assign = [a.cpu().long() for a in assign]
        self.indices, self.indptr, self.wkk = (t.to(DEV) for t in R.build_index(assign, K))
        self.cd = [torch.cat([a.new_zeros(1), a + 1]).to(DEV) for a in assign]
        self.n_items = assign[0].numel()

    def kernel_args(self):
        return (self.centres, self.wkk.contiguous(), self.indptr.int(), self.indices.int(), [c.int() for c in self.cd])


def synthetic_book(parts, d, K, n_items, seed, scale=1.0, one_bucket=False):
    g = torch.Generator().manual_seed(seed)
    X = torch.randn(n_items, d, generator=g)
    dsub = d // parts
    centres = torch.stack([X[torch.randperm(n_items, generator=g)[:K], p * dsub:(p + 1) * dsub] for p in range(parts)])
    if one_bucket:
        assign = [torch.full((n_items,), K - 2, dtype=torch.long) for _ in range(parts)]
    else:
        assign = list(R.kmeans_scores(X.to(DEV), centres.to(DEV), False)[1].argmin(2).cpu())
    return Book(centres * scale, assign)


def recorded_book(gold, name, parts):
    if parts == 2:
        c = torch.stack([gold[f'{name}.c0'], gold[f'{name}.c1']])
        cd = [gold[f'{name}.cd0'], gold[f'{name}.cd1']]
    else:
        c, cd = gold[f'{name}.c'].unsqueeze(0), [gold[f'{name}.cd']]
    return Book(c, [x[1:] - 1 for x in cd])


def judge(ra, book, query, n, cosine, seed, pos=None):
    """The whole battery for one codebook / query batch: stream, twin, every draw judged, the edges through the twin."""
    from recstudio_amd import ops
    M = query.shape[0]
    args = book.kernel_args()
    gen = torch.cuda.default_generators[torch.cuda.current_device()]
    torch.manual_seed(seed)
    state = gen.get_state()
    out = ops.midx_sample(query, *args, n, pos_ids=pos, cosine=cosine, want_u=True)
    end = gen.get_offset()
    gen.set_state(state)
    want_u = torch.rand(M, n, book.P + 1, device=DEV)
    assert torch.equal(out['u'], want_u), 'uniforms differ from torch.rand(M, n, P + 1) on the device stream'
    assert gen.get_offset() == end, 'the generator does not end where the torch call ends'
    twin = ops.midx_lookup(query, *args, out['u'], pos_ids=pos, cosine=cosine)
    assert torch.equal(twin['neg_ids'], out['neg_ids']) and torch.equal(twin['neg_logp'], out['neg_logp'])
    tab = R.tables(query, book.centres, book.wkk, cosine)
    assert bool(torch.isfinite(tab['F0']).all()) and bool(torch.isfinite(out['neg_logp']).all())
    res = R.judge_draws(tab, book.wkk, book.indptr, book.indices, book.cd, out['neg_ids'], out['u'], out['neg_logp'])
    print('stream draws', res)
    assert not R.violations(res), res
    u = R.edge_uniforms(tab, max(n, 16), book.P, torch.Generator().manual_seed(seed + 1))
    edge = ops.midx_lookup(query, *args, u, cosine=cosine)
    res = R.judge_draws(tab, book.wkk, book.indptr, book.indices, book.cd, edge['neg_ids'], u, edge['neg_logp'])
    print('edge draws', res)
    assert not R.violations(res), res
    if pos is not None:
        val, bound = R.item_logp(tab, book.cd, pos)
        assert bool(((out['pos_logp'].double() - val).abs() <= bound).all())
        assert torch.equal(twin['pos_logp'], out['pos_logp'])
        assert bool((out['pos_logp'][pos == 0] == 0).all())
    return out


def queries(M, d, seed, scale=1.0):
    return (torch.randn(M, d, generator=torch.Generator().manual_seed(seed)) * scale).to(DEV)


# (parts, d, K, M, n, N with the padding id)
SHAPES = [(2, 8, 2, 3, 5, 50), (2, 64, 16, 1000, 1, 5001), (2, 128, 64, 257, 64, 100003), (2, 256, 64, 33, 100, 20011),
          (2, 32, 5, 17, 9, 500), (2, 64, 37, 9, 33, 3000), (2, 16, 8, 11, 13, 41),
          (1, 8, 2, 3, 5, 50), (1, 64, 16, 1000, 1, 5001), (1, 128, 64, 257, 64, 100003), (1, 256, 64, 33, 100, 20011),
          (1, 32, 5, 17, 9, 500), (1, 64, 37, 9, 33, 3000)]


@pytest.mark.parametrize('parts,d,K,M,n,N', SHAPES)
def test_every_draw_inside_its_float64_interval(ra, parts, d, K, M, n, N):
    book = synthetic_book(parts, d, K, N - 1, seed=d + K)
    if (d, K, N) == (16, 8, 41):
        assert int((book.wkk == 0).sum()) > 32          # more than half of the 64 buckets are empty
    g = torch.Generator().manual_seed(N)
    pos = torch.randint(0, N, (M, 3), generator=g).to(DEV)
    pos[0, 0] = 0
    judge(ra, book, queries(M, d, 3), n, False, seed=K * 1000 + n, pos=pos)


@pytest.mark.parametrize('name,parts,cosine', [('midx_ip_30', 2, False), ('midx_cos_30', 2, True), ('cluster_ip_30', 1, False),
                                               ('midx_ip_2', 2, False)])
def test_recorded_codebooks(ra, gold, name, parts, cosine):
    """The fixture's shape (16, 4, 5, 7, 301): empty buckets, and (MIDX) a bucket holding exactly one item."""
    book = recorded_book(gold, name, parts)
    assert torch.equal(book.wkk.cpu(), gold[f'{name}.wkk']) and torch.equal(book.indices.cpu(), gold[f'{name}.indices'])
    if parts == 2:
        assert int((book.wkk == 1).sum()) >= 1 or name != 'midx_ip_30'
    q = gold['query'].to(DEV)
    out = judge(ra, book, q, 7, cosine, seed=5, pos=gold['pos2'].to(DEV))
    ref = gold[f'{name}.p2'].double().to(DEV)
    tab = R.tables(q, book.centres, book.wkk, cosine)
    _, bound = R.item_logp(tab, book.cd, gold['pos2'].to(DEV))
    scale = R.gamma(book.centres.shape[2] + 2) / R.gamma(book.centres.shape[2] // 4 + 3)     # the recorded side is a sequential fp32 sum
    assert bool(((out['pos_logp'].double() - ref).abs() <= bound * (1 + scale)).all())


@pytest.mark.parametrize('parts', [2, 1])
def test_all_items_in_one_bucket(ra, parts):
    book = synthetic_book(parts, 32, 6, 200, seed=1, one_bucket=True)
    out = judge(ra, book, queries(7, 32, 4), 19, False, seed=21)
    assert int((book.wkk > 0).sum()) == 1 and int(out['neg_ids'].min()) >= 1


@pytest.mark.parametrize('parts,cosine', [(2, False), (1, False), (2, True), (1, True)])
def test_logits_of_sixty_and_the_cosine_scorer(ra, parts, cosine):
    """Centres scaled so that the logits reach about +-60 (cosine: |logit| <= ||c||): no inf, no NaN, every draw judged."""
    book = synthetic_book(parts, 64, 16, 2000, seed=9, scale=60.0 / 8.0 if not cosine else 8.0)
    q = queries(33, 64, 6, scale=1.0 if not cosine else 5.0)
    tab = R.tables(q, book.centres, book.wkk, cosine)
    if not cosine:
        assert float(tab['r'].abs().max()) > 60.0
    judge(ra, book, q, 12, cosine, seed=77)


# ------------------------------------------------------------------------------------------------- Lloyd step
def lloyd_inputs(N, dsub, K, parts, seed, with_pad_row=False):
    g = torch.Generator().manual_seed(seed)
    d = dsub * parts
    W = torch.randn(N + 1, d, generator=g).to(DEV)
    X = W[1:] if with_pad_row else W[1:].clone()
    rows = torch.randperm(N, generator=g)[:K]
    centres = torch.stack([W[1:][rows.to(DEV), p * dsub:(p + 1) * dsub] for p in range(parts)])
    centres = centres + 0.05 * torch.randn(centres.shape, generator=g).to(DEV)
    return X, centres.contiguous()


LLOYD = [(300, 4, 2, 2, False, False), (300, 8, 5, 1, False, False), (300, 8, 5, 2, True, True),
         (4099, 64, 64, 2, False, False), (4099, 128, 5, 1, True, False), (4099, 128, 64, 2, False, True),
         (4099, 64, 5, 1, False, True), (200003, 64, 64, 2, True, False), (200003, 128, 64, 1, False, False)]


@pytest.mark.parametrize('N,dsub,K,parts,view,normalize', LLOYD)
def test_lloyd_step_against_float64(ra, N, dsub, K, parts, view, normalize):
    from recstudio_amd import ops
    X, centres = lloyd_inputs(N, dsub, K, parts, seed=N + dsub + K, with_pad_row=view)
    if view:
        assert X.data_ptr() != X._base.data_ptr()                  # a table view with a base offset (weight[1:])
    x64, s, E = R.kmeans_scores(X, centres, normalize)
    want, decided = R.decided_rows(s, E)
    undecided = 1.0 - float(decided.double().mean())
    print('undecided rows', undecided)
    assert undecided <= 0.002                                      # asserted on the input, before the kernel runs
    assign, sums, counts, loss = ops.kmeans_step(X, centres, normalize=normalize)
    again = ops.kmeans_step(X, centres, normalize=normalize)
    for a, b in zip((assign, sums, counts, loss), again):
        assert torch.equal(a, b), 'two runs differ'
    assign = assign.long()
    assert int(assign.min()) >= 0 and int(assign.max()) < K
    assert torch.equal(assign[decided], want[decided])
    ref_sums, abs_sums, ref_counts = R.cluster_sums(x64, assign, K, dsub)
    assert torch.equal(counts.long(), ref_counts)
    bound = (ref_counts.double().unsqueeze(2) + 2) * R.U32 * abs_sums
    err = (sums.double() - ref_sums).abs()
    print('sums error / bound', float((err / bound.clamp_min(1e-300)).max()))
    assert bool((err <= bound).all())
    ref_loss, loss_bound = R.cluster_loss(x64, assign, centres, normalize)
    print('loss error / bound', ((loss - ref_loss).abs() / loss_bound).tolist())
    assert bool(((loss - ref_loss).abs() <= loss_bound).all())


# ------------------------------------------------------------------------------------------------- update
UPDATE_CASES = [('midx_ip_30', 2, False, 30), ('midx_cos_30', 2, True, 30), ('cluster_ip_30', 1, False, 30),
                ('midx_ip_2', 2, False, 2), ('midx_cos_2', 2, True, 2), ('cluster_ip_2', 1, False, 2),
                ('cluster_dead', 1, False, 30)]


@pytest.mark.parametrize('name,parts,cosine,max_iter', UPDATE_CASES)
def test_update_against_the_recorded_reference(ra, gold, name, parts, cosine, max_iter):
    X = gold['item_embs'].to(DEV)
    K, d = 4, X.shape[1]
    cls = ra.MIDXSamplerUniform if parts == 2 else ra.ClusterSamplerUniform
    s = cls(X.shape[0] + 1, K, ra.CosineScorer() if cosine else ra.InnerProductScorer())
    init = gold['init_cos' if cosine else 'init_rows']
    if name == 'cluster_dead':
        s.c = gold['cluster_dead_init'].clone()
        torch.manual_seed(7)
    elif parts == 1:
        s.c = init[:K].clone()
    else:
        s.c0, s.c1 = init[:K, :d // 2].clone(), init[K:, d // 2:].clone()
    s.update(X, max_iter=max_iter)
    ints = ('cd0', 'cd1', 'indices', 'indptr') if parts == 2 else ('cd', 'indices', 'indptr')
    for a in ints:
        got = getattr(s, a)
        assert got.dtype == torch.int64 and torch.equal(got.cpu(), gold[f'{name}.{a}']), a
    assert s.wkk.dtype == torch.float32 and torch.equal(s.wkk.cpu(), gold[f'{name}.wkk'])
    x64 = R.normalize64(gold['item_embs']) if cosine else gold['item_embs'].double()
    names = ('c0', 'c1') if parts == 2 else ('c',)
    c_ref = torch.stack([gold[f'{name}.{n}'] for n in names])
    assign = torch.stack([gold[f'{name}.{a}'][1:] - 1 for a in (('cd0', 'cd1') if parts == 2 else ('cd',))])
    bound = 2 * R.centre_bound(x64, assign, c_ref)
    for p, n in enumerate(names):
        err = (getattr(s, n).cpu().double() - c_ref[p].double()).abs()
        print(name, n, 'centre error / bound', float((err / bound[p].clamp_min(1e-300)).max()))
        assert bool((err <= bound[p]).all())
        pad = getattr(s, n + '_')
        assert pad.shape[0] == K + 1 and bool((pad[0] == 0).all()) and torch.equal(pad[1:], getattr(s, n))


def test_class_forward_shapes_and_errors(ra, gold):
    X = gold['item_embs'].to(DEV)
    for cls in (ra.MIDXSamplerUniform, ra.ClusterSamplerUniform):
        s = cls(X.shape[0] + 1, 4, ra.InnerProductScorer())
        torch.manual_seed(0)
        s.update(X)
        q3 = queries(6, 16, 2).view(2, 3, 16)
        neg, lp = s(q3, 5)
        assert neg.shape == (2, 3, 5) and lp.shape == (2, 3, 5) and neg.dtype == torch.int64
        flat = s.compute_item_p(q3.view(6, 16), neg.view(6, 5))
        assert torch.equal(flat.view(2, 3, 5), lp)
        with pytest.raises(ValueError):
            s(q3, 5, torch.ones(2, 3, dtype=torch.long, device=DEV))
        q = q3.view(6, 16)
        pos1 = torch.tensor([0, 5, 300, 7, 0, 1], device=DEV)
        lpp, neg, lp = s(q, 4, pos1)
        assert lpp.shape == (6,) and neg.shape == (6, 4) and float(lpp[0]) == 0.0 and float(lpp[4]) == 0.0
        assert torch.equal(lpp, s.compute_item_p(q, pos1))
        lpp, _, _ = s(q, 4, pos1.view(6, 1).expand(6, 3).contiguous())
        assert lpp.shape == (6, 3)
        neg, lp = s(q, 0)                                      # no draws: empty results, not an error
        assert neg.shape == (6, 0) and lp.shape == (6, 0) and neg.dtype == torch.int64
        with pytest.raises(ValueError):
            cls(301, 4).update(torch.randn(300, 12, device=DEV))
        with pytest.raises(NotImplementedError):
            cls(301, 4, ra.EuclideanScorer())


# ------------------------------------------------------------------------------------------------- end to end
def test_fit_two_epochs_with_the_midx_sampler(ra, golden):
    """BPR's towers with SampledSoftmaxLoss and the MIDX sampler on ml-100k, at the stock learning rate (0.001, as
    test_bpr_fit_ml100k).  The sampled-softmax loss is measured AGAINST the proposal, which is rebuilt from the trained embeddings
    every epoch: where the proposal approaches the model's own softmax the loss tends to log(n + 1) whatever the model has learnt,
    so the falling loss says little by itself and the test also asks that the model ranks held-out items above chance."""
    from test_dataset_golden import make
    import logging
    g = golden('data_ml100k')
    ds = make(ra.TripletDataset, g)
    trn, val, _ = ds.build(split_ratio=[0.8, 0.1, 0.1], shuffle=True)
    cfg = {'train': {'epochs': 2, 'negative_count': 16, 'batch_size': 512, 'learning_rate': 0.001},
           'eval': {'batch_size': 256}, 'model': {'embed_dim': 64}}
    sampler = ra.MIDXSamplerUniform(trn.num_items, 8, ra.InnerProductScorer())
    centres = []
    plain_update = sampler.update

    def update(item_embs, max_iter=30):
        plain_update(item_embs, max_iter)
        centres.append(sampler.c0.clone())
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
    assert len(centres) == 2 and not torch.equal(centres[0], centres[1])
    batch = next(iter(trn.train_loader(batch_size=64, shuffle=False)))
    batch = model._to_device(batch, next(model.parameters()).device)
    out = model.forward(batch, return_query=True, return_neg_id=True)
    lp = out['score']['log_neg_prob']
    assert torch.equal(lp, sampler.compute_item_p(out['query'], out['neg_id']))
    assert bool(torch.isfinite(lp).all()) and int(out['neg_id'].min()) >= 1 and int(out['neg_id'].max()) < trn.num_items
    recall = model.evaluate(val)['recall@20']
    print('recall@20', recall, 'chance', 20 / (trn.num_items - 1))
    assert recall > 20 / (trn.num_items - 1)               # a ranking that has learnt nothing hits 20 of the items at random
