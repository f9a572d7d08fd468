"""GPU: BaseRetriever (the reference's plugin surface) on the fused path -- _test_step against the
recorded reference outputs, and short end-to-end fits of BPR (TripletDataset) and SASRec (SeqDataset)
on the ml-100k fixture."""
import numpy as np
import pytest
import torch

import oracle
from test_dataset_golden import make

pytestmark = pytest.mark.gpu
T = torch.from_numpy
DEV = 'cuda'


@pytest.fixture(scope='module')
def ra():
    import recstudio_amd
    recstudio_amd._native.lib()
    torch.cuda.init()
    return recstudio_amd


def _retriever(ra, g, **kw):
    N, d = g['item_w'].shape
    U = g['user_w'].shape[0]
    item = torch.nn.Embedding(N, d, padding_idx=0)
    user = torch.nn.Embedding(U, d, padding_idx=0)
    with torch.no_grad():
        item.weight.copy_(T(g['item_w']))
        user.weight.copy_(T(g['user_w']))
    m = ra.BaseRetriever(None, item_encoder=item, query_encoder=user, scorer=ra.InnerProductScorer(), **kw)
    m.fiid, m.fuid, m.frating = 'item_id', 'user_id', 'rating'
    m.item_fields, m.query_fields = {'item_id'}, {'user_id'}
    return m.to(DEV)


def test_topk_and_test_step_golden(ra, golden):
    g = golden('topk')
    k = g['items'].shape[1]
    m = _retriever(ra, g)
    m.config['eval']['topk'] = k
    m._update_item_vector()
    uid, hist = T(g['uid']).to(DEV), T(g['hist']).to(DEV)
    with torch.no_grad():
        score, items = m.topk({'user_id': uid, 'user_hist': hist}, k, hist)
        assert np.array_equal(items.cpu().numpy(), g['items'])
        np.testing.assert_allclose(score.cpu().numpy(), g['score'], rtol=1e-5)
        metrics = ['ndcg', 'recall', 'precision', 'map', 'mrr', 'hit']
        b1 = {'user_id': uid, 'user_hist': hist, 'item_id': T(g['tgt1']).to(DEV), 'rating': torch.ones(len(uid), device=DEV)}
        b2 = {'user_id': uid, 'user_hist': hist, 'item_id': T(g['tgt2']).to(DEV), 'rating': T(g['rat2']).to(DEV)}
        for batch, pre in ((b1, 'm1_'), (b2, 'm2_')):
            out, bs = m._test_step(batch, metrics, [5, 10])
            assert bs == len(uid)
            for key, v in out.items():
                np.testing.assert_allclose(float(v), g[pre + key], rtol=1e-5, err_msg=pre + key)


def test_training_step_golden_through_baseretriever(ra, golden):
    """BaseRetriever.training_step + backward == the reference's, with a sampler plugin that returns
    fixed ids (so it goes down the per-plugin path) AND with given ids through the fused path."""
    g = golden('forward')
    for tag, loss in (('bpr_ip', 'BPRLoss'), ('ssm_ip', 'SampledSoftmaxLoss')):
        gg = {'item_w': g[tag + '_item_w'], 'user_w': g[tag + '_user_w']}
        neg, lpp, lnp = T(g[tag + '_neg']).to(DEV), T(g[tag + '_lpp']).to(DEV), T(g[tag + '_lnp']).to(DEV)

        class Fixed(ra.Sampler):
            def forward(self, query, num_neg, pos_items=None):
                return lpp, neg, lnp
        m = _retriever(ra, gg, sampler=Fixed(gg['item_w'].shape[0]), loss=getattr(ra, loss)())
        m.neg_count = neg.shape[1]
        batch = {'user_id': T(g[tag + '_uid']).to(DEV), 'item_id': T(g[tag + '_pos']).to(DEV),
                 'rating': torch.ones(neg.shape[0], device=DEV)}
        assert not m._fused_ok()
        out = m.forward(batch)
        np.testing.assert_allclose(out['score']['neg_score'].detach().cpu(), g[tag + '_neg_score'], rtol=1e-4, atol=1e-6)
        lossv = m.training_step(batch)
        np.testing.assert_allclose(lossv.item(), g[tag + '_loss'], rtol=1e-5)
        lossv.backward()
        np.testing.assert_allclose(m.item_encoder.weight.grad.cpu(), g[tag + '_item_grad'], rtol=1e-4, atol=1e-7)
        np.testing.assert_allclose(m.query_encoder.weight.grad.cpu(), g[tag + '_user_grad'], rtol=1e-4, atol=1e-7)
    # full-score branch with SoftmaxLoss (sampler None)
    tag = 'softmax_ip'
    gg = {'item_w': g[tag + '_item_w'], 'user_w': g[tag + '_user_w']}
    m = _retriever(ra, gg, loss=ra.SoftmaxLoss())
    batch = {'user_id': T(g[tag + '_uid']).to(DEV), 'item_id': T(g[tag + '_pos']).to(DEV),
             'rating': torch.ones(len(g[tag + '_uid']), device=DEV)}
    lossv = m.training_step(batch)
    np.testing.assert_allclose(lossv.item(), g[tag + '_loss'], rtol=1e-5)
    lossv.backward()
    np.testing.assert_allclose(m.item_encoder.weight.grad.cpu(), g[tag + '_item_grad'], rtol=1e-4, atol=1e-7)


def test_fused_forward_through_baseretriever_matches_device_reference_ops(ra):
    """Fused dispatch: the score dict equals what the reference's op sequence (torch.randint ->
    F.embedding -> matmul) gives on this device under the same seed."""
    N, U, d, B, n = 3001, 200, 64, 300, 8
    m = ra.BaseRetriever({'model': {'embed_dim': d}, 'train': {'negative_count': n}},
                         item_encoder=torch.nn.Embedding(N, d, padding_idx=0),
                         query_encoder=torch.nn.Embedding(U, d, padding_idx=0), sampler=ra.UniformSampler(N),
                         loss=ra.BPRLoss())
    m.fiid, m.fuid, m.frating = 'item_id', 'user_id', 'rating'
    m.item_fields, m.query_fields, m.neg_count = {'item_id'}, {'user_id'}, n
    m._init_parameter()
    m.to(DEV)
    assert m._fused_ok() and not m.item_encoder.weight[0].any()
    batch = {'user_id': torch.randint(1, U, (B,), device=DEV), 'item_id': torch.randint(1, N, (B,), device=DEV),
             'rating': torch.ones(B, device=DEV)}
    torch.manual_seed(5)
    out = m.forward(batch, return_neg_id=True, return_query=True, return_item=True)
    torch.manual_seed(5)
    neg = torch.randint(1, N, (B, n), device=DEV)
    assert torch.equal(out['neg_id'], neg)
    q = m.query_encoder(batch['user_id'])
    want = torch.matmul(m.item_encoder(neg), q.unsqueeze(-1)).squeeze(-1)
    np.testing.assert_allclose(out['score']['neg_score'].detach().cpu(), want.detach().cpu(), rtol=1e-4, atol=1e-6)
    assert torch.equal(out['query'], q) and out['score']['log_neg_prob'].dtype == torch.int64
    assert set(out['score']) == {'pos_score', 'log_pos_prob', 'neg_score', 'log_neg_prob'}


def test_bpr_fit_ml100k(ra, golden):
    """BASELINE.json configs[0] shape: BPR, d = 64, UniformSampler n = 1 on ml-100k.  The reference logs
    train_loss_0 = 0.6931 (README.md:198) and reaches ndcg@10 ~0.24 after ~35 epochs; a few epochs
    must start at ln 2 and move the right way."""
    g = golden('data_ml100k')
    cfg = {'train': {'epochs': 6, 'negative_count': 1, 'batch_size': 512, 'learning_rate': 0.001},
           'eval': {'batch_size': 256}}
    model = ra.BPR(cfg)
    ds = make(ra.TripletDataset, g)
    trn, val, tst = ds.build(split_ratio=[0.8, 0.1, 0.1], shuffle=True)
    losses = []
    import logging

    class Grab(logging.Handler):
        def emit(self, record):
            losses.append(record.getMessage())
    model.logger.addHandler(Grab())
    model.logger.setLevel(logging.INFO)
    best = model.fit(trn, val)
    first = float(losses[0].split('train_loss=')[1].split()[0])
    last = float(losses[-1].split('train_loss=')[1].split()[0])
    assert abs(first - 0.6931) < 2e-3 and last < first - 0.02
    res = model.evaluate(tst)
    assert set(res) >= {'ndcg@10', 'recall@10', 'mrr@20', 'hit@5'}
    assert res['recall@20'] > 0.05 and best > 0.01          # far above chance (20 / 1574 items)


@pytest.mark.parametrize('name,lrs', [('exponential', [0.01 * 0.98, 0.01 * 0.98 ** 2, 0.01 * 0.98 ** 3]), ('onplateau', None)])
def test_fit_steps_the_configured_scheduler(ra, golden, name, lrs):
    """train.scheduler (recommender.py:476-494: 'exponential' = ExponentialLR(gamma 0.98), 'onplateau' = ReduceLROnPlateau),
    stepped once per epoch; weight decay and gradient clipping go to the torch optimizer as in the reference."""
    g = golden('data_ml100k')
    cfg = {'train': {'epochs': 3, 'negative_count': 64, 'batch_size': 2048, 'learning_rate': 0.01, 'scheduler': name,
                     'weight_decay': 1e-6, 'grad_clip_norm': 5.0}, 'eval': {'batch_size': 256}}
    model = ra.BPR(cfg)
    trn, val, _ = make(ra.TripletDataset, g).build(split_ratio=[0.8, 0.1, 0.1], shuffle=True)
    seen = []
    import logging

    class Grab(logging.Handler):
        def emit(self, record):
            seen.append(record.getMessage())
    model.logger.addHandler(Grab())
    model.logger.setLevel(logging.INFO)
    model.fit(trn, val)
    got = [float(m.split('lr=')[1].split()[0]) for m in seen if 'lr=' in m]
    assert len(got) == 3
    if lrs is not None:
        np.testing.assert_allclose(got, lrs, rtol=6e-3)        # (the log prints four decimals)
    else:
        assert all(abs(v - 0.01) < 1e-9 for v in got)          # three improving epochs: the plateau scheduler holds the rate
    with pytest.raises(NotImplementedError):                   # the in-kernel optimizer steps: no weight decay / clipping
        ra.BPR({'train': dict(cfg['train'], fused_optimizer='sgd')}).fit(trn, val)
    # ... but they follow the scheduler: the rate of the stand-in optimizer is handed to the kernels after every epoch
    if name == 'exponential':
        base = dict(cfg['train'], fused_optimizer='sgd', weight_decay=0.0, grad_clip_norm=None, learning_rate=20.0, epochs=2)
        seen.clear()
        sched = ra.BPR({'train': base, 'eval': cfg['eval']})
        if not any(isinstance(h, Grab) for h in sched.logger.handlers):      # (the models share one logger)
            sched.logger.addHandler(Grab())
        sched.logger.setLevel(logging.INFO)
        sched.fit(trn, val)
        got = [float(m.split('lr=')[1].split()[0]) for m in seen if 'lr=' in m]
        np.testing.assert_allclose(got, [19.6, 19.208], rtol=1e-4)
        const = ra.BPR({'train': dict(base, scheduler=None), 'eval': cfg['eval']})
        const.fit(trn, val)
        # epoch 0 ran at the same rate in both; epoch 1 at 19.6 vs 20: different weights, same order of magnitude
        diff = (sched.item_encoder.weight - const.item_encoder.weight).detach().abs().max()
        assert 0 < float(diff) < 0.1 * float(const.item_encoder.weight.abs().max())


def test_sasrec_fit_ml100k(ra, golden):
    """BASELINE.json configs[2] shape (scaled down): SASRec on SeqDataset, d = 64, L <= 50,
    SampledSoftmax with the popularity sampler, n = 64."""
    g = golden('data_ml100k')
    sq = make(ra.SeqDataset, g, max_seq_len=50)
    trn, val, tst = sq.build(split_ratio=2)
    cfg = {'model': {'embed_dim': 64, 'dropout_rate': 0.2}, 'train': {'epochs': 2, 'negative_count': 64,
           'batch_size': 512, 'learning_rate': 0.002, 'init_method': 'normal'}, 'eval': {'batch_size': 256}}
    model = ra.SASRec(cfg, loss=ra.SampledSoftmaxLoss(), sampler=ra.PopularSamplerModel(trn.item_freq))
    best = model.fit(trn, val)
    res = model.evaluate(tst)
    assert np.isfinite(model.logged_metrics['train_loss']) and res['recall@20'] > 0.02


def test_sasrec_stock_defaults_fit_ml100k(ra, golden):
    """Stock SASRec as the reference configures it (sasrec.py:117-123, seq/config/sasrec.yaml): BinaryCrossEntropyLoss,
    UniformSampler, negative_count = 1, normal init -- no plugin kwargs."""
    g = golden('data_ml100k')
    sq = make(ra.SeqDataset, g, max_seq_len=50)
    trn, val, tst = sq.build(split_ratio=2)
    model = ra.SASRec({'model': {'embed_dim': 64}, 'train': {'epochs': 2, 'batch_size': 512}, 'eval': {'batch_size': 256}})
    model.fit(trn, val)
    assert type(model.loss_fn) is ra.BinaryCrossEntropyLoss and model.neg_count == 1
    assert model.config['train']['init_method'] == 'normal'
    res = model.evaluate(tst)
    assert np.isfinite(model.logged_metrics['train_loss']) and res['recall@20'] > 0.02


def test_device_loaders_match_host_loaders(ra, golden):
    """Loader fast path: batches assembled on the GPU (SeqDataset through rsa_seg_gather) equal the host
    loader's batches (which are pinned to the reference in tests/test_dataset_golden.py)."""
    g = golden('data_ml100k')
    ds = make(ra.TripletDataset, g)
    trn, _, _ = ds.build(split_ratio=[0.8, 0.1, 0.1], shuffle=True)
    trn.drop_feat(trn.use_field)
    host = list(trn.train_loader(512, shuffle=False))
    dev = list(trn.device_train_loader(512, shuffle=False, device=DEV))
    assert len(host) == len(dev) == 131
    for hb, db in zip(host[:3] + host[-1:], dev[:3] + dev[-1:]):
        assert sorted(hb) == sorted(db)
        for k in hb:
            assert db[k].is_cuda and torch.equal(hb[k], db[k].cpu()) and hb[k].dtype == db[k].dtype
    sq = make(ra.SeqDataset, g, max_seq_len=50)
    strn, _, _ = sq.build(split_ratio=2)
    strn.drop_feat(strn.use_field)
    host = list(zip(range(4), strn.train_loader(64, shuffle=False)))
    dev = list(zip(range(4), strn.device_train_loader(64, shuffle=False, device=DEV)))
    for (_, hb), (_, db) in zip(host, dev):
        flat, st, en = db['_seg']                              # the CSR view rides along (for towers that gather from it)
        assert sorted(hb) == sorted(k for k in db if not k.startswith('_'))
        for k in hb:
            assert torch.equal(hb[k], db[k].cpu()), k
        assert torch.equal(en - st, db['seqlen']) and torch.equal(flat[en], db['item_id'])
    # shuffled epochs cover every sample exactly once
    seen = torch.cat([b['user_id'] * 0 + 1 for b in trn.device_train_loader(4096, shuffle=True, device=DEV)])
    assert int(seen.sum()) == len(trn)


def test_dns_sampling_method(ra):
    """sampling_method='dns' (baseretriever.py:330-347): the reference's op sequence on this device --
    randint pool -> embedding -> matmul -> topk -> gather -- against the kernel path, same seed."""
    N, U, d, B, n0, n1 = 4001, 100, 64, 70, 32, 4
    m = ra.BaseRetriever({'model': {'embed_dim': d}, 'train': {'negative_count': [n0, n1], 'sampling_method': 'dns'}},
                         item_encoder=torch.nn.Embedding(N, d, padding_idx=0),
                         query_encoder=torch.nn.Embedding(U, d, padding_idx=0), sampler=ra.UniformSampler(N),
                         loss=ra.BPRLoss())
    m.fiid, m.fuid, m.frating = 'item_id', 'user_id', 'rating'
    m.item_fields, m.query_fields, m.neg_count = {'item_id'}, {'user_id'}, [n0, n1]
    m._init_parameter()
    m.to(DEV)
    assert not m._fused_ok()
    batch = {'user_id': torch.randint(1, U, (B,), device=DEV), 'item_id': torch.randint(1, N, (B,), device=DEV),
             'rating': torch.ones(B, device=DEV)}
    torch.manual_seed(9)
    out = m.forward(batch, return_neg_id=True)
    torch.manual_seed(9)
    pool = torch.randint(1, N, (B, n0), device=DEV)
    q = m.query_encoder(batch['user_id'])
    s = torch.matmul(m.item_encoder(pool), q.unsqueeze(-1)).squeeze(-1)
    want = torch.gather(pool, -1, torch.topk(s, n1).indices)
    assert torch.equal(out['neg_id'], want)
    np.testing.assert_allclose(out['score']['neg_score'].detach().cpu(), torch.topk(s, n1).values.detach().cpu(),
                               rtol=1e-4, atol=1e-6)
    loss = m.training_step(batch)
    loss.backward()
    assert torch.isfinite(loss) and m.item_encoder.weight.grad is not None and not m.item_encoder.weight.grad[0].any()
    v, c = ra.ops.row_topk(s.detach(), 7)
    wv, wc = torch.topk(s.detach(), 7)
    assert torch.equal(v, wv) and torch.equal(c, wc)


def test_bpr_sgd_step_equals_autograd_plus_torch_sgd(ra):
    """fused.bpr_sgd_step (no gradient tensors: updates applied by the kernels) == loss.backward() +
    torch.optim.SGD.step() on dense gradients, same sampled negatives."""
    torch.manual_seed(6)
    N, U, d, B, n, lr = 4001, 301, 64, 257, 64, 0.05
    item = torch.nn.Embedding(N, d, padding_idx=0).to(DEV)
    user = torch.nn.Embedding(U, d, padding_idx=0).to(DEV)
    item2 = torch.nn.Embedding(N, d, padding_idx=0).to(DEV)
    user2 = torch.nn.Embedding(U, d, padding_idx=0).to(DEV)
    item2.load_state_dict(item.state_dict())
    user2.load_state_dict(user.state_dict())
    uid = torch.randint(1, U, (B,), device=DEV)
    pos = torch.randint(1, N, (B,), device=DEV)
    iw0, uw0 = item.weight.detach().clone(), user.weight.detach().clone()
    torch.manual_seed(8)
    loss, neg = ra.fused.bpr_sgd_step(item.weight, user.weight, n, lr, user_ids=uid, pos_ids=pos,
                                      sampler=ra.UniformSampler(N))
    opt = torch.optim.SGD(list(item2.parameters()) + list(user2.parameters()), lr=lr)
    q = user2(uid)
    ref = -torch.nn.functional.logsigmoid((q * item2(pos)).sum(-1, keepdim=True)
                                          - (q.unsqueeze(1) * item2(neg)).sum(-1)).mean(-1).mean()
    ref.backward()
    opt.step()
    np.testing.assert_allclose(loss.item(), ref.item(), rtol=1e-5)
    np.testing.assert_allclose(item.weight.detach().cpu(), item2.weight.detach().cpu(), rtol=1e-4, atol=1e-7)
    np.testing.assert_allclose(user.weight.detach().cpu(), user2.weight.detach().cpu(), rtol=1e-4, atol=1e-7)
    assert not item.weight[0].any() and not user.weight[0].any()
    # The assertions above judge the WEIGHT (weights N(0, 1), lr = 0.05: the median update is 3.9e-6 of the weight, their
    # tolerance 25 times that).  The UPDATE: W' - W and U' - U against the float64 step within the end-to-end bound of
    # tests/sgd_referee.py on every element of every touched row (2u |W'| for the read-modify-write + the gradient's own
    # bound), no other row moved; and against torch's fp32 update within twice that bound (torch's fp32 autograd + SGD is
    # one more fp32 implementation of the same step).
    import sgd_referee as sr
    c = sr.coefficients(iw0, uw0, uid, pos, neg)
    allow, _ = sr.torch_sigmoid_allowance(iw0.device, B, n)
    for ref, got, theirs, start in zip(sr.end_to_end(iw0, uw0, uid, pos, neg, lr, c, allow), (item.weight.data, user.weight.data),
                                       (item2.weight.data, user2.weight.data), (iw0, uw0)):
        ratio, moved = sr.judge(ref, got, start)
        r = ref['rows']
        upd, upd_t, want = got[r].double() - ref['w0'], theirs[r].double() - ref['w0'], ref['w'] - ref['w0']
        vs_torch = float(((upd - upd_t).abs() / (2 * ref['tol'])).max())
        print(f'update against float64: error / bound {ratio:.3f}; against torch fp32: {vs_torch:.3f} of twice the bound; median |update| / |weight| '
              f'{sr.update_scale(ref):.1e}; max |update - float64 update| / |update| at the median row '
              f'{float(((upd - want).abs().sum(1) / want.abs().sum(1)).median()):.1e}')
        assert ratio <= 1.0 and moved == 0 and vs_torch <= 1.0


@pytest.mark.parametrize('kind', ['uniform', 'popular'])
def test_device_side_philox_offset_is_graph_capturable(ra, kind):
    """``rsa_fused_args.offset_dev`` + ``rsa_rng_advance``: the Philox offset read from, and advanced in, a device word -- the
    hooks a host needs to capture the step in its own hipGraph.  A captured (forward, advance) pair replayed three times
    draws what three eager launches draw from the torch generator, losses included.  (The package itself replays nothing:
    a graph replay of the step measured slower than its eager launches -- 72 vs 65 us, DESIGN appendix A -- and the wrapper
    class that did was removed in round 5.)"""
    from recstudio_amd import rng
    nat = ra._native
    torch.manual_seed(1)
    N, U, d, B, n = 6001, 401, 128, 192, 64
    item = torch.randn(N, d, device=DEV) * 0.2
    item[0] = 0
    user = torch.randn(U, d, device=DEV) * 0.2
    kw = {'sampler': nat.SAMPLER_UNIFORM}
    if kind == 'popular':
        kw = dict(ra.PopularSamplerModel((torch.rand(N) ** 2 * 90).long()).to(DEV).lookup_kwargs(), sampler=nat.SAMPLER_POPULAR)
    batches = [(torch.randint(1, U, (B,), device=DEV), torch.randint(1, N, (B,), device=DEV)) for _ in range(3)]
    gen = torch.cuda.default_generators[torch.cuda.current_device()]
    torch.manual_seed(77)
    eager = []
    for uid, pos in batches:
        o = ra.ops.fused_forward(item, user, n, query_index=uid, pos_ids=pos, fused_bpr=True, want_logp=False, **kw)
        eager.append((float(o['loss']), o['neg_ids'].clone()))
    torch.manual_seed(77)
    seed, offset0 = int(gen.initial_seed()), int(gen.get_offset())
    unroll = 4 if kind == 'popular' else rng.randint_unroll(1, N)
    cu, mt = rng.device_props(torch.device(DEV))
    increment = rng.counter_offset(B * n, rng.grid_threads(B * n, cu, mt), unroll)
    offset_dev = torch.tensor([offset0], dtype=torch.int64, device=DEV)
    uid_s, pos_s = batches[0][0].clone(), batches[0][1].clone()
    box = {}

    def body():
        box['o'] = ra.ops.fused_forward(item, user, n, query_index=uid_s, pos_ids=pos_s, out=box.get('o'), fused_bpr=True,
                                        want_logp=False, rng_state=(seed, offset_dev), **kw)
        ra.ops.rng_advance(offset_dev, increment)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side), torch.no_grad():
        body()                                        # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    offset_dev.fill_(offset0)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph), torch.no_grad():
        body()
    for (uid, pos), (want_loss, want_neg) in zip(batches, eager):
        uid_s.copy_(uid)
        pos_s.copy_(pos)
        graph.replay()
        assert torch.equal(box['o']['neg_ids'], want_neg)
        np.testing.assert_allclose(float(box['o']['loss']), want_loss, rtol=1e-6)
    assert int(offset_dev) == offset0 + 3 * increment


def _sampling_model(ra, N, U, d, n0, n1, method):
    m = ra.BaseRetriever({'model': {'embed_dim': d}, 'train': {'negative_count': [n0, n1], 'sampling_method': method}},
                         item_encoder=torch.nn.Embedding(N, d, padding_idx=0),
                         query_encoder=torch.nn.Embedding(U, d, padding_idx=0), sampler=ra.UniformSampler(N),
                         loss=ra.BPRLoss())
    m.fiid, m.fuid, m.frating = 'item_id', 'user_id', 'rating'
    m.item_fields, m.query_fields, m.neg_count = {'item_id'}, {'user_id'}, [n0, n1]
    m._init_parameter()
    m.to(DEV)
    with torch.no_grad():
        m.item_encoder.weight.mul_(30)          # spread the scores so that softmax / top-k are not degenerate
        m.item_encoder.weight[0] = 0
    m._update_item_vector()
    return m


@pytest.mark.parametrize('method', ['sir', 'toprand', 'top&rand', 'brute'])
def test_other_sampling_methods_follow_the_reference_op_sequence(ra, method):
    """baseretriever.py:280-355 restated with stock torch ops on this device (F.embedding, matmul, topk,
    softmax, multinomial, randint) under the same seed == BaseRetriever.sampling(method=...)."""
    N, U, d, B, n0, n1 = 3001, 100, 64, 50, 24, 6
    m = _sampling_model(ra, N, U, d, n0, n1, method)
    uid = torch.randint(1, U, (B,), device=DEV)
    pos = torch.randint(1, N, (B,), device=DEV)
    batch = {'user_id': uid, 'item_id': pos, 'rating': torch.ones(B, device=DEV)}
    torch.manual_seed(21)
    (lpp, neg, lnp), query = m.sampling(batch, [n0, n1], method=method, return_query=True)
    W = m.item_encoder.weight.detach()
    q = m.query_encoder(uid).detach()
    torch.manual_seed(21)
    if method == 'sir':
        pool = torch.randint(1, N, (B, n0), device=DEV)
        s = torch.matmul(W[pool], q.unsqueeze(-1)).squeeze(-1)
        probs = torch.softmax(s + torch.finfo(torch.float32).eps, -1)
        # the kernel's scores differ from matmul's in the last bits; feed multinomial the kernel's probabilities
        kernel_probs = torch.softmax(m._pool_scores(q, pool) + torch.finfo(torch.float32).eps, -1)
        np.testing.assert_allclose(kernel_probs.cpu(), probs.cpu(), rtol=2e-4, atol=1e-7)
        res = torch.multinomial(kernel_probs, n1, replacement=True)
        assert torch.equal(neg, torch.gather(pool, -1, res))
        np.testing.assert_allclose(lnp.cpu(), torch.gather(s, -1, res).cpu(), rtol=1e-4, atol=1e-5)
        np.testing.assert_allclose(lpp.cpu(), (q * W[pos]).sum(-1).cpu(), rtol=1e-4, atol=1e-5)
    elif method in ('toprand', 'top&rand'):
        k = n0 if method == 'toprand' else n1 // 2
        full = q @ W[1:].T
        sc, it = torch.topk(full, k + 1)
        it = it + 1
        keep = it != pos.view(-1, 1)                       # the positive plays the history's role
        top = torch.stack([row[kp][:k] for row, kp in zip(it, keep)])
        if method == 'toprand':
            idx = torch.randint(0, n0, (B, n1), device=DEV)
            assert torch.equal(neg, torch.gather(top, -1, idx))
        else:
            rnd = torch.randint(1, N, size=(B, n1 - k), device=DEV)
            assert torch.equal(neg, torch.cat((top, rnd), -1))
        assert not lnp.any() and not lpp.any()
    else:
        all_prob = torch.nn.functional.pad(torch.softmax(m.score_func(q, m.item_vector), -1), (1, 0))
        want = torch.multinomial(all_prob, n1, replacement=True)
        assert torch.equal(neg, want)
        np.testing.assert_allclose(lnp.cpu(), torch.log(torch.gather(all_prob, -1, want)).cpu(), rtol=1e-5)
        np.testing.assert_allclose(lpp.cpu(), torch.log(torch.gather(all_prob, -1, pos.view(-1, 1))).view(-1).cpu(), rtol=1e-5)
    # and the training step runs through it
    loss = m.training_step(batch)
    loss.backward()
    assert torch.isfinite(loss)


def test_retriever_sampler_wraps_another_retrievers_sampling(ra):
    """sampler.py:61-78: the generator retriever's brute-force softmax sampling behind the Sampler interface."""
    N, U, d, B = 2001, 80, 64, 30
    gen = _sampling_model(ra, N, U, d, 8, 5, 'brute')
    rs = ra.RetrieverSampler(N, retriever=gen, method='brute', t=1)
    assert isinstance(rs, ra.Sampler)
    batch = {'user_id': torch.randint(1, U, (B,), device=DEV), 'item_id': torch.randint(1, N, (B,), device=DEV)}
    torch.manual_seed(3)
    lpp, neg, lnp = rs(batch, 5)
    torch.manual_seed(3)
    (lpp2, neg2, lnp2), _ = gen.sampling(batch, 5, method='brute')
    assert torch.equal(neg, neg2) and torch.equal(lnp, lnp2) and torch.equal(lpp, lpp2)
    assert neg.shape == (B, 5) and int(neg.min()) >= 1 and int(neg.max()) < N


@pytest.mark.parametrize('d', [64, 128, 256])
def test_sorted_scatter_equals_atomic_backward_and_is_reproducible(ra, d):
    """rsa_rows_update_sorted (radix sort by item id + one RMW per row) == the dense atomic scatter of
    rsa_fused_backward, twice bit-identical, padding row untouched, heavy duplication included."""
    torch.manual_seed(d)
    N, U, M, n = 3001, 500, 777, 64
    item = torch.randn(N, d, device=DEV)
    user = torch.randn(U, d, device=DEV)
    uid = torch.randint(1, U, (M,), device=DEV)
    pos = torch.randint(0, N, (M,), device=DEV)
    neg = torch.randint(0, 40, (M, n), device=DEV)             # ~1200 copies of each id: long runs crossing chunks
    neg[:, ::2] = torch.randint(0, N, (M, n // 2), device=DEV)
    dpos, dneg = torch.randn(M, device=DEV), torch.randn(M, n, device=DEV)
    up = torch.tensor([0.37], device=DEV)
    ref = ra.ops.fused_backward(item, user, neg, dneg, query_index=uid, pos_ids=pos, dpos=dpos, upstream=up,
                                want_query_grad=False)[0]
    a = ra.ops.scatter_rows_sorted(torch.zeros(N, d, device=DEV), user, neg, dneg, query_index=uid, pos_ids=pos,
                                   dpos=dpos, upstream=up)
    b = ra.ops.scatter_rows_sorted(torch.zeros(N, d, device=DEV), user, neg, dneg, query_index=uid, pos_ids=pos,
                                   dpos=dpos, upstream=up)
    assert torch.equal(a, b) and not a[0].any()
    np.testing.assert_allclose(a.cpu(), ref.cpu(), rtol=2e-4, atol=2e-4)
    q = user[uid].double()
    want = torch.zeros(N, d, dtype=torch.float64, device=DEV)
    want.index_add_(0, pos, dpos.double().unsqueeze(1) * q)
    want.index_add_(0, neg.reshape(-1), (dneg.double().unsqueeze(-1) * q.unsqueeze(1)).reshape(-1, d))
    want[0] = 0
    np.testing.assert_allclose(a.cpu(), (want * 0.37).float().cpu(), rtol=1e-4, atol=1e-4)


@pytest.mark.parametrize('M,n,with_pos', [(1, 1, True), (3, 5, False), (130, 7, True), (64, 1, False)])
def test_sorted_scatter_small_and_ragged_shapes(ra, M, n, with_pos):
    torch.manual_seed(M * 10 + n)
    N, U, d = 37, 20, 128
    user = torch.randn(U, d, device=DEV)
    uid = torch.randint(0, U, (M,), device=DEV)
    pos = torch.randint(0, N, (M,), device=DEV) if with_pos else None
    neg = torch.randint(0, N, (M, n), device=DEV)
    dpos = torch.randn(M, device=DEV) if with_pos else None
    dneg = torch.randn(M, n, device=DEV)
    got = ra.ops.scatter_rows_sorted(torch.ones(N, d, device=DEV), user, neg, dneg, query_index=uid, pos_ids=pos, dpos=dpos,
                                     pad_row=-1)
    q = user[uid].double()
    want = torch.ones(N, d, dtype=torch.float64, device=DEV)
    if with_pos:
        want.index_add_(0, pos, dpos.double().unsqueeze(1) * q)
    want.index_add_(0, neg.reshape(-1), (dneg.double().unsqueeze(-1) * q.unsqueeze(1)).reshape(-1, d))
    np.testing.assert_allclose(got.cpu(), want.float().cpu(), rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize('N,M,n,d', [(5, 700, 64, 128), (3, 9000, 5, 64), (40, 3000, 33, 256), (2, 64, 1, 128), (1, 129, 1, 128)])
def test_sorted_scatter_long_runs(ra, N, M, n, d):
    """Few target rows, thousands of elements each (the owner side of the sharded backward sorts by QUERY index: runs of
    ~1000): runs that span many 64-element chunks are summed from per-chunk partials in chunk order -- equal to a float64
    index_add, bit-identical from call to call, empty slots (negative ids) dropped, with and without a padding row."""
    g = torch.Generator(device=DEV).manual_seed(N * 1000 + M)
    U = 50
    src = torch.randn(U, d, device=DEV, generator=g)
    uid = torch.randint(0, U, (M,), device=DEV, generator=g)
    ids = torch.randint(0, N, (M, n), device=DEV, generator=g)
    ids[torch.rand(M, n, device=DEV, generator=g) < 0.05] = -1                   # empty slots
    dn = torch.randn(M, n, device=DEV, generator=g)
    for pad_row in (-1, 0):
        base = torch.randn(N, d, device=DEV, generator=g)
        got = ra.ops.scatter_rows_sorted(base.clone(), src, ids, dn, query_index=uid, pad_row=pad_row)
        keep = ids.reshape(-1) >= 0
        want = base.double()
        contrib = (dn.double().unsqueeze(-1) * src[uid].double().unsqueeze(1)).reshape(-1, d)
        want.index_add_(0, ids.reshape(-1)[keep], contrib[keep])
        if pad_row >= 0:
            want[pad_row] = base[pad_row].double()
        scale = float(contrib.abs().sum(0).max())
        np.testing.assert_allclose(got.cpu(), want.float().cpu(), rtol=1e-5, atol=1e-6 * max(1.0, scale))
        again = ra.ops.scatter_rows_sorted(base.clone(), src, ids, dn, query_index=uid, pad_row=pad_row)
        assert torch.equal(got, again)


def test_fused_adam_step_equals_sparse_grads_plus_torch_sparse_adam(ra):
    """fused.FusedBPRAdam (no gradient tensors; lazy Adam applied by rsa_rows_update_sorted) == loss.backward() with
    COO gradients + torch.optim.SparseAdam.step(), three steps, same sampled negatives."""
    torch.manual_seed(7)
    N, U, d, B, n, lr = 4001, 301, 64, 200, 64, 0.01
    item = torch.nn.Embedding(N, d, padding_idx=0).to(DEV)
    user = torch.nn.Embedding(U, d, padding_idx=0).to(DEV)
    with torch.no_grad():
        item.weight.mul_(0.3)
        user.weight.mul_(0.3)
    item2 = torch.nn.Embedding(N, d, padding_idx=0).to(DEV)
    user2 = torch.nn.Embedding(U, d, padding_idx=0).to(DEV)
    item2.load_state_dict(item.state_dict())
    user2.load_state_dict(user.state_dict())
    opt = torch.optim.SparseAdam(list(item2.parameters()) + list(user2.parameters()), lr=lr)
    fa = ra.fused.FusedBPRAdam(item.weight, user.weight, lr=lr)
    sampler = ra.UniformSampler(N)
    batches = [(torch.randint(1, U, (B,), device=DEV), torch.randint(1, N, (B,), device=DEV)) for _ in range(3)]
    batches[1] = (batches[0][0], batches[0][1])                  # repeated rows: state carried over
    for step, (uid, pos) in enumerate(batches):
        torch.manual_seed(50 + step)
        loss, neg = fa.step(n, user_ids=uid, pos_ids=pos, sampler=sampler)
        opt.zero_grad()
        ref, _ = ra.fused.fused_bpr_loss(item2.weight, user2.weight, n, query_index=uid, pos_ids=pos, neg_ids=neg,
                                         sparse_grad=True)
        ref.backward()
        opt.step()
        np.testing.assert_allclose(float(loss), float(ref.detach()), rtol=1e-5)
    np.testing.assert_allclose(item.weight.detach().cpu(), item2.weight.detach().cpu(), rtol=2e-4, atol=2e-6)
    np.testing.assert_allclose(user.weight.detach().cpu(), user2.weight.detach().cpu(), rtol=2e-4, atol=2e-6)
    assert not item.weight[0].any()


@pytest.mark.parametrize('kind', ['adam', 'sgd'])
def test_bpr_fit_with_fused_optimizer(ra, golden, kind):
    """BaseRetriever.fit with train.fused_optimizer: the whole step (sampling, scoring, loss, optimizer update) in the
    kernels; BPR on the ml-100k fixture still learns."""
    g = golden('data_ml100k')
    ds = make(ra.TripletDataset, g)
    trn, val, tst = ds.build(split_ratio=[0.8, 0.1, 0.1], shuffle=True)
    lr = 0.003 if kind == 'adam' else 30.0            # plain SGD on a mean-reduced loss needs a batch-sized rate
    cfg = {'model': {'embed_dim': 64}, 'train': {'epochs': 6, 'negative_count': 64, 'batch_size': 512, 'learning_rate': lr,
           'fused_optimizer': kind, 'init_method': 'normal'}, 'eval': {'batch_size': 256}}
    if kind == 'adam':
        cfg['train']['fused_prefetch'] = 'adam'       # (the look-ahead is opt-in for the lazy-Adam step: it does not pay there)
    model = ra.BPR(cfg)
    model.fit(trn, val)
    res = model.evaluate(tst)
    assert np.isfinite(model.logged_metrics['train_loss']) and model.logged_metrics['train_loss'] < 0.68
    assert res['recall@20'] > 0.05
    if True:
        # the default run above drew and sorted every step's negatives one batch ahead on a side stream
        # (fused.PrefetchedBPRSGD / FusedBPRAdam.prepare); without the look-ahead: the same model bit for bit
        plain = ra.BPR({**cfg, 'train': dict(cfg['train'], fused_prefetch=False)})
        plain.fit(trn, val)
        assert torch.equal(plain.item_encoder.weight, model.item_encoder.weight)
        assert torch.equal(plain.query_encoder.weight, model.query_encoder.weight)
        assert plain.logged_metrics['train_loss'] == model.logged_metrics['train_loss']
