"""GPU: exact softmax sampling over the whole catalog without [B, N] (rsa_softmax_sample / rsa_softmax_lookup, ops.softmax_sample,
``sampling(method='brute')`` with ``train.brute_stream``) against the float64 referee of tests/softmax_draw_referee.py: EVERY draw
inside its two CDF intervals with an exact block given the kernel's own table, the log-probabilities, the device random stream,
the history, spiky rows, the distribution, the existing torch path, and the catalog size the torch path cannot hold."""
import ctypes

import pytest
import torch

import softmax_draw_referee as R

pytestmark = pytest.mark.gpu
DEV = 'cuda'
COUNTS = ('outside', 'zero_weight', 'block', 'item', 'logp')


@pytest.fixture(scope='module')
def ra():
    import recstudio_amd
    recstudio_amd._native.lib()
    torch.cuda.init()
    return recstudio_amd


@pytest.fixture(scope='module')
def G(ra):
    return ra.ops.softmax_sample_block()


def catalog(n_cols, d, M, seed, scale=0.4):
    g = torch.Generator().manual_seed(seed)
    W = torch.randn(n_cols + 1, d, generator=g) * scale
    W[0] = 0
    Q = torch.randn(M, d, generator=g) * 0.6
    pos = torch.randint(0, n_cols + 1, (M, 2), generator=g)
    return W.to(DEV), Q.to(DEV), pos.to(DEV), g


def check(T, out, u, G, pos=None, what=''):
    res = R.judge_draws(T, out['neg_ids'], u, out['neg_logp'])
    assert not {k: res[k] for k in COUNTS if res[k]}, (what, res)
    assert torch.equal(R.own_block(out['cum'], u[..., 0]), (out['neg_ids'] - 1) // G), what
    assert R.judge_lse(T, out['lse'])[0] == 0, what
    if pos is not None:
        assert R.judge_logp(T, pos, out['pos_logp'])[0] == 0, what
        assert bool(torch.isneginf(out['pos_logp'][pos == 0]).all())
    return res


# (mode, d, t, N - 1 in units chosen below, B, n)
SHAPES = [(R.IP, 32, 1.0, 'five', 1, 5), (R.IP, 64, 0.5, 'G-1', 130, 1), (R.COS, 128, 4.0, 'G', 1, 64), (R.EUC, 48, 1.0, '3G+5', 130, 5),
          (R.IP, 128, 4.0, '3G+5', 130, 64), (R.COS, 48, 0.5, '3G+5', 1, 5), (R.EUC, 64, 0.5, 'G-1', 1, 64), (R.COS, 32, 1.0, 'five', 130, 1),
          (R.IP, 128, 1.0, '40000', 130, 5), (R.EUC, 32, 4.0, '40000', 1, 64), (R.COS, 64, 1.0, '40000', 130, 1)]


@pytest.mark.parametrize('mode,d,t,size,B,n', SHAPES)
def test_every_draw_is_inside_its_intervals(ra, G, mode, d, t, size, B, n):
    """softmax_lookup on uniforms at the CDF edges and softmax_sample on the device stream, every draw judged; two calls on one
    seed are bit-equal, sample == lookup fed with its own uniforms, and the generator ends where torch.rand(M, n, 2) leaves it."""
    ops = ra.ops
    n_cols = {'five': 5, 'G-1': G - 1, 'G': G, '3G+5': 3 * G + 5, '40000': 40000}[size]
    W, Q, pos, g = catalog(n_cols, d, B, seed=n_cols + d)
    T = R.tables64(W, Q, t, mode, G)
    if size == '40000':
        # more than one item range in the block pass: the host deals ~1024 workgroups over ceil(B / 128) query groups, whole
        # blocks per range, at most one range per block (ss_plan, rsa_softmax_sample.hip)
        n_blocks, groups = (n_cols + G - 1) // G, (B + 127) // 128
        assert min((1024 + groups - 1) // groups, n_blocks) > 1
    u = R.edge_uniforms(T, n, g)
    out = ops.softmax_lookup(W, Q, u, t=t, score_mode=mode, pos_ids=pos, want_tables=True)
    check(T, out, u, G, pos, 'lookup')
    gen = torch.cuda.default_generators[torch.cuda.current_device()]
    torch.manual_seed(77)
    want_u = torch.rand(B, n, 2, device=DEV)
    want_offset = gen.get_offset()
    torch.manual_seed(77)
    a = ops.softmax_sample(W, Q, n, t=t, score_mode=mode, pos_ids=pos, want_u=True, want_tables=True)
    assert gen.get_offset() == want_offset
    assert torch.equal(a['u'], want_u)
    check(T, a, a['u'], G, pos, 'sample')
    torch.manual_seed(77)
    b = ops.softmax_sample(W, Q, n, t=t, score_mode=mode, pos_ids=pos, want_u=True, want_tables=True)
    c = ops.softmax_lookup(W, Q, a['u'], t=t, score_mode=mode, pos_ids=pos, want_tables=True)
    for other in (b, c):
        for k in ('neg_ids', 'neg_logp', 'pos_logp', 'lse', 'mass', 'cum'):
            assert torch.equal(a[k], other[k]), k


@pytest.mark.parametrize('mode,d,t', [(R.IP, 64, 1.0), (R.COS, 128, 0.5), (R.EUC, 48, 4.0)])
def test_history_is_never_drawn(ra, G, mode, d, t):
    """0-padding, duplicated ids, one block wholly inside the history, and a row whose history is everything but one item."""
    ops = ra.ops
    n_cols, B, n = 3 * G + 5, 6, 64
    W, Q, pos, g = catalog(n_cols, d, B, seed=11)
    L = n_cols + 3
    hist = torch.zeros(B, L, dtype=torch.int64)
    keep = 2 * G + 7                                                # row 0: every id but this one
    hist[0, :n_cols - 1] = torch.tensor([i for i in range(1, n_cols + 1) if i != keep])
    for b in range(1, B):
        some = torch.randint(1, n_cols + 1, (20,), generator=g)
        row = torch.cat([some, some[:6], torch.arange(G + 1, 2 * G + 1)])          # duplicates, and block 1 whole
        hist[b, 1:1 + row.numel()] = row                                          # (slot 0 and the tail stay 0)
    hist = hist.to(DEV)
    T = R.tables64(W, Q, t, mode, G, hist)
    u = R.edge_uniforms(T, n, g)
    out = ops.softmax_lookup(W, Q, u, t=t, score_mode=mode, pos_ids=pos, user_hist=hist, want_tables=True)
    check(T, out, u, G, pos, 'lookup')
    torch.manual_seed(5)
    smp = ops.softmax_sample(W, Q, n, t=t, score_mode=mode, user_hist=hist, want_u=True, want_tables=True)
    check(T, smp, smp['u'], G, None, 'sample')
    for o in (out, smp):
        assert not bool((o['neg_ids'].unsqueeze(2) == hist.unsqueeze(1)).any())
        assert bool((o['neg_ids'][0] == keep).all())
        assert float(o['mass'][1:, 1].abs().max()) == 0.0            # the block wholly in the history: exactly 0
        assert float(o['mass'][0, :2].abs().max()) == 0.0 and float(o['mass'][0, 3].abs().max()) == 0.0


def test_spiky_rows(ra, G):
    """One item 200 above the rest: it is the only id drawn (the others' weights underflow) -- and with that item in the history the
    draw goes on over the rest."""
    ops = ra.ops
    n_cols, d, B, n = 3 * G + 5, 64, 3, 64
    W, Q, _, g = catalog(n_cols, d, B, seed=3, scale=0.05)
    spike = torch.tensor([G, G + 1, n_cols])                        # last of block 0, first of block 1, the last item
    Q[:] = 0
    Q[:, 0] = 10.0
    W[:, 0] = 0
    for b in range(B):
        Q[b, 1 + b] = 1.0                                           # rows differ
    W[spike.to(DEV), 0] = 20.0                                      # score 200 against |others| < 1
    hist = spike.to(DEV).view(1, -1).expand(B, -1).contiguous()
    T = R.tables64(W, Q, 1.0, R.IP, G)
    u = R.edge_uniforms(T, n, g)
    out = ops.softmax_lookup(W, Q, u, want_tables=True)
    check(T, out, u, G, None, 'spiky')
    assert bool(torch.isin(out['neg_ids'], spike.to(DEV)).all())
    # the spikes in the history: every other weight is exp(-200) = 0 in fp32 (the reference's masked row is all zero as well and
    # torch.multinomial refuses it) -- the documented answer is id 0 with log-probability -inf
    out = ops.softmax_lookup(W, Q, u, user_hist=hist, want_tables=True)
    assert not bool(out['neg_ids'].any()) and bool(torch.isneginf(out['neg_logp']).all()) and not bool(out['cum'].any())
    # 30 above the rest: with the spikes in the history the draw goes on over the others
    W[spike.to(DEV), 0] = 3.0
    T = R.tables64(W, Q, 1.0, R.IP, G, hist)
    u = R.edge_uniforms(T, n, g)
    out = ops.softmax_lookup(W, Q, u, user_hist=hist, want_tables=True)
    check(T, out, u, G, None, 'spiky, history')
    assert not bool(torch.isin(out['neg_ids'], spike.to(DEV)).any())


def test_distribution(ra, G):
    """N - 1 = 37, one query 4096 times, n = 64: every item's count c_i within 6 sigma (+ 1) of M p_i, p from the referee; the rule
    itself is confirmed on torch.multinomial (CPU) first."""
    ops = ra.ops
    n_cols, d, B, n = 37, 32, 4096, 64
    W, Q, _, g = catalog(n_cols, d, 1, seed=8, scale=1.0)
    hist = torch.tensor([[3, 3, 0, 17]], device=DEV)
    T = R.tables64(W, Q, 2.0, R.IP, G, hist)
    p = (T['w'][0] / T['total'][0]).cpu()
    M = B * n

    def inside(counts):
        dev = (counts.double() - M * p).abs()
        return bool((dev <= 6 * torch.sqrt(M * p * (1 - p)) + 1).all())
    torch.manual_seed(1)
    assert inside(torch.bincount(torch.multinomial(p.float(), M, replacement=True), minlength=n_cols + 1))
    torch.manual_seed(1234)
    out = ops.softmax_sample(W, Q.expand(B, -1).contiguous(), n, t=2.0, user_hist=hist.expand(B, -1).contiguous())
    counts = torch.bincount(out['neg_ids'].view(-1).cpu(), minlength=n_cols + 1)
    assert int(counts[0]) == 0 and int(counts[3]) == 0 and int(counts[17]) == 0
    assert inside(counts), (counts.tolist(), (M * p).tolist())


def _sampling_model(ra, N, U, d, n0, n1, scorer=None, stream=False):
    m = ra.BaseRetriever({'model': {'embed_dim': d}, 'train': {'negative_count': [n0, n1], 'sampling_method': 'brute',
                                                                'brute_stream': stream}},
                         item_encoder=torch.nn.Embedding(N, d, padding_idx=0), query_encoder=torch.nn.Embedding(U, d, padding_idx=0),
                         sampler=ra.UniformSampler(N), loss=ra.BPRLoss(), **({'scorer': scorer} if scorer is not None else {}))
    m.fiid, m.fuid, m.frating = 'item_id', 'user_id', 'rating'
    m.item_fields, m.query_fields, m.neg_count = {'item_id'}, {'user_id'}, [n0, n1]
    m._init_parameter()
    m.to(DEV)
    with torch.no_grad():
        m.item_encoder.weight.mul_(30)          # spread the scores so that the softmax is not flat
        m.item_encoder.weight[0] = 0
    m._update_item_vector()
    return m


@pytest.mark.parametrize('excluding_hist', [False, True])
def test_streaming_brute_agrees_with_the_torch_path(ra, G, excluding_hist):
    N, U, d, B, n1, t = 3001, 100, 64, 50, 6, 2
    m = _sampling_model(ra, N, U, d, 8, n1)
    assert m.config['train']['brute_stream'] is False and ra.retriever.default_config()['train']['brute_stream'] is False
    uid = torch.randint(1, U, (B,), device=DEV)
    pos = torch.randint(1, N, (B,), device=DEV)
    hist = torch.randint(0, N, (B, 9), device=DEV)
    batch = {'user_id': uid, 'item_id': pos, 'rating': torch.ones(B, device=DEV), 'user_hist': hist}
    torch.manual_seed(4)
    (lpp0, neg0, lnp0), _ = m.sampling(batch, [8, n1], method='brute', excluding_hist=excluding_hist, t=t)
    m.config['train']['brute_stream'] = True
    torch.manual_seed(4)
    (lpp1, neg1, lnp1), q1 = m.sampling(batch, [8, n1], method='brute', excluding_hist=excluding_hist, t=t, return_query=True)
    assert (lpp0.shape, neg0.shape, lnp0.shape) == (lpp1.shape, neg1.shape, lnp1.shape)
    assert (lpp0.dtype, neg0.dtype, lnp0.dtype) == (lpp1.dtype, neg1.dtype, lnp1.dtype)
    assert not lpp1.requires_grad and not lnp1.requires_grad and q1 is not None
    W, q = m.item_encoder.weight.detach(), m.query_encoder(uid).detach()
    T = R.tables64(W, q, float(t), R.IP, G, hist if excluding_hist else None)
    assert R.judge_logp(T, pos.view(-1, 1), lpp1.view(-1, 1))[0] == 0
    tol = (T['eps'].gather(1, pos.view(-1, 1) - 1).view(-1) + T['eps_lse'] + R.U32 * (T['s'].gather(1, pos.view(-1, 1) - 1).view(-1).abs()
                                                                                     + T['lse'].abs()))
    assert bool(((lpp1.double() - lpp0.double()).abs() <= 2 * tol).all())        # two fp32 evaluations, each within tol_lp
    # the streaming ids' log-probabilities == the default path's log(all_prob) gathered at those ids
    all_prob = torch.nn.functional.pad(torch.softmax(m.score_func(q, m.item_vector) / t, dim=-1), pad=(1, 0))
    if excluding_hist:
        all_prob = all_prob.scatter(-1, hist, 0.0)
        assert not bool((neg1.unsqueeze(2) == hist.unsqueeze(1)).any())
    want = torch.log(torch.gather(all_prob, -1, neg1))
    assert bool(torch.isfinite(want).all())
    assert R.judge_logp(T, neg1, lnp1)[0] == 0 and R.judge_logp(T, neg1, want)[0] == 0
    assert int(neg1.min()) >= 1 and int(neg1.max()) < N
    # RetrieverSampler gets the streaming path through retriever.sampling
    rs = ra.RetrieverSampler(N, retriever=m, method='brute', t=1)
    torch.manual_seed(3)
    a = rs(batch, 5)
    torch.manual_seed(3)
    (b, _) = m.sampling(batch, 5, method='brute')
    assert all(torch.equal(x, y) for x, y in zip(a, b)) and a[1].shape == (B, 5)
    # and a training step runs through it
    loss = m.training_step({k: v for k, v in batch.items() if k != 'user_hist'})
    loss.backward()
    assert torch.isfinite(loss)


def test_streaming_brute_says_what_it_cannot_do(ra):
    m = _sampling_model(ra, 301, 20, 32, 4, 2, stream=True)
    batch = {'user_id': torch.randint(1, 20, (4,), device=DEV), 'item_id': torch.randint(1, 301, (4,), device=DEV)}
    m.score_func = ra.scorer.GMFScorer(32).to(DEV)
    with pytest.raises(NotImplementedError, match='stock'):
        m.sampling(batch, 2, method='brute')
    m.score_func = ra.InnerProductScorer()
    with pytest.raises(NotImplementedError, match='2-D'):
        m.sampling(batch, 2, method='brute', query=torch.zeros(4, 3, 32, device=DEV))


def test_big_catalog_stays_far_below_one_score_matrix(ra, G):
    """train.brute_stream at N = 10^6 + 1, B = 256, d = 128, n = 64 with a 50-id history: 4096 draws judged by the referee on their
    rows, and the call's peak memory rises by less than one eighth of ONE [B, N - 1] fp32 matrix (the torch path holds three to
    four of them; with G >= 64 the tables are at most a sixteenth, so this is a condition, not a measurement)."""
    N, U, d, B, n, L = 1_000_001, 300, 128, 256, 64, 50
    m = ra.BaseRetriever({'model': {'embed_dim': d}, 'train': {'negative_count': [n, n], 'sampling_method': 'brute', 'brute_stream': True}},
                         item_encoder=torch.nn.Embedding(N, d, padding_idx=0), query_encoder=torch.nn.Embedding(U, d, padding_idx=0),
                         sampler=ra.UniformSampler(N), loss=ra.BPRLoss())
    m.fiid, m.fuid, m.frating = 'item_id', 'user_id', 'rating'
    m.item_fields, m.query_fields, m.neg_count = {'item_id'}, {'user_id'}, [n, n]
    m.to(DEV)
    g = torch.Generator(device=DEV).manual_seed(0)
    with torch.no_grad():
        m.item_encoder.weight.normal_(0, 0.3, generator=g)
        m.item_encoder.weight[0] = 0
        m.query_encoder.weight.normal_(0, 0.3, generator=g)
    m._update_item_vector()
    uid = torch.randint(1, U, (B,), device=DEV, generator=g)
    pos = torch.randint(1, N, (B,), device=DEV, generator=g)
    hist = torch.randint(0, N, (B, L), device=DEV, generator=g)
    hist[:, :4] = hist[:, 4:8]                                       # duplicates
    batch = {'user_id': uid, 'item_id': pos, 'user_hist': hist}
    query = m.query_encoder(uid).detach()
    gen = torch.cuda.default_generators[torch.cuda.current_device()]
    torch.manual_seed(9)
    off0 = gen.get_offset()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    (lpp, neg, lnp), _ = m.sampling(batch, n, method='brute', excluding_hist=True, query=query)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    assert rise < 4 * B * (N - 1) // 8, rise
    assert neg.shape == (B, n) and lpp.shape == (B,)
    assert not bool((neg.unsqueeze(2) == hist.unsqueeze(1)).any())
    # the uniforms of the call, from the stream it consumed
    torch.manual_seed(9)
    assert gen.get_offset() == off0
    u = torch.rand(B, n, 2, device=DEV)
    rows = torch.arange(0, B, 4, device=DEV)                         # 64 rows x 64 draws
    W = m.item_encoder.weight.detach()
    T = R.tables64(W, query[rows], 1.0, R.IP, G, hist[rows])
    res = R.judge_draws(T, neg[rows], u[rows], lnp[rows])
    assert not {k: res[k] for k in COUNTS if res[k]}, res
    assert R.judge_logp(T, pos[rows].view(-1, 1), lpp[rows].view(-1, 1))[0] == 0


def test_argument_errors(ra, G):
    ops, nat = ra.ops, ra._native
    W, Q, pos, _ = catalog(50, 32, 3, seed=1)
    out = ops.softmax_sample(W, Q, 0, pos_ids=pos)                   # num_neg = 0: empty outputs, lse and pos_logp still there
    assert out['neg_ids'].shape == (3, 0) and out['neg_logp'].shape == (3, 0) and out['neg_ids'].dtype == torch.int64
    T = R.tables64(W, Q, 1.0, R.IP, G)
    assert R.judge_lse(T, out['lse'])[0] == 0 and R.judge_logp(T, pos, out['pos_logp'])[0] == 0
    for bad_t in (0.0, -1.0):
        with pytest.raises(ValueError, match='temperature'):
            ops.softmax_sample(W, Q, 2, t=bad_t)
    with pytest.raises(NotImplementedError, match='128'):
        ops.softmax_sample(torch.zeros(10, 256, device=DEV), torch.zeros(2, 256, device=DEV), 2)
    with pytest.raises(ValueError, match='u must be'):
        ops.softmax_lookup(W, Q, torch.zeros(3, 4, device=DEV))
    # the C ABI itself: every check runs before the first HIP call
    lib = nat.lib()
    lse = torch.empty(3, device=DEV)
    ws = torch.empty(int(lib.rsa_softmax_sample_workspace_bytes(3, 51)), dtype=torch.uint8, device=DEV)

    def block(**kw):
        a = nat.SoftmaxSampleArgs()
        a.item_table, a.n_items, a.dim, a.inv_t, a.query, a.n_query = nat.ptr(W), 51, 32, 1.0, nat.ptr(Q), 3
        a.num_neg, a.grid_threads, a.lse, a.workspace, a.workspace_bytes = 2, 256, nat.ptr(lse), nat.ptr(ws), ws.numel()
        ids, lp = torch.empty(3, 2, dtype=torch.int64, device=DEV), torch.empty(3, 2, device=DEV)
        a.neg_ids, a.neg_logp = nat.ptr(ids), nat.ptr(lp)
        for k, v in kw.items():
            setattr(a, k, v)
        return a, (ids, lp)
    for kw, status, text in ((dict(neg_ids=None), -1, b'neg_ids'), (dict(lse=None), -1, b'lse is null'), (dict(dim=36), -3, b'dim=36'),
                             (dict(inv_t=0.0), -1, b'inv_t'), (dict(inv_t=-2.0), -1, b'inv_t'), (dict(workspace_bytes=8), -1, b'workspace'),
                             (dict(n_pos=1), -1, b'pos_ids'), (dict(hist_len=3), -1, b'user_hist'), (dict(score_mode=1), -1, b'item_aux')):
        a, keep = block(**kw)
        assert lib.rsa_softmax_sample(ctypes.byref(a), None) == status, kw
        assert text in lib.rsa_last_error(), (kw, lib.rsa_last_error())
    a, keep = block()
    assert lib.rsa_softmax_lookup(ctypes.byref(a), None) == -1 and b'u_in' in lib.rsa_last_error()
