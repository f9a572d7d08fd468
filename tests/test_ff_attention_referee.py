"""CPU: the float64 referee of the fused feed-forward attention pooling (tests/ff_attention_referee.py) judged on itself -- an fp32
emulation of the kernel's order of operations inside half its bounds, eleven seeded mistakes outside them --, the argument checks
of rsa_ff_attention / rsa_ff_attention_backward (they run before any HIP call), the torch-op twin against the float64 rule, and
AttentionLayer / NARM / STAMP query encoders on CPU tensors.  No device kernel runs here.  Measured: see
test_fp32_emulation_stays_within_half_of_every_bound's docstring."""
import ctypes
import functools

import pytest
import torch

import ff_attention_referee as fr

# (B, S, D, M, q_dim, bias, pad, seed): NARM's configuration (q = k = M, no bias) and STAMP's (q = 2 k, bias); padded cases carry
# non-zero keys at the padded positions
CASES = [(5, 9, 32, 32, 32, False, 'whole', 1), (5, 9, 32, 32, 64, True, 'whole', 2), (4, 33, 64, 64, 128, True, 'holes', 3),
         (3, 20, 64, 128, 64, True, 'suffix', 4), (2, 40, 128, 128, 128, False, None, 5)]


@pytest.fixture(scope='module')
def nat():
    import os
    from recstudio_amd import _native
    if not os.path.exists(_native.LIB_PATH):
        _native.build()
    return _native


@functools.lru_cache(maxsize=None)
def judged(case):
    B, S, D, M, q_dim, bias, pad, seed = case
    c = fr.make_case(B, S, D, M, q_dim=q_dim, bias=bias, pad=pad, seed=seed)
    k = fr.kernel_inputs(c)
    args = (k['key'], k['qh'], k['w_k'], k['w2'], k['b2'], k['key_pad'], k['scale'])
    out32, a32, grads32 = fr.emulate_fp32(*args, k['g'])
    pre = k['qh'].view(B, 1, M) + k['key'] @ k['w_k'].t()
    allow = fr.sigmoid_allowance('cpu', pre)
    fwd = fr.judge_forward(*args, allow)
    bwd = fr.backward(*args, k['g'], allow)
    return dict(c=c, k=k, args=args, out32=out32, a32=a32, grads32=grads32, allow=allow, fwd=fwd, bwd=bwd)


NAMES = ('dkey', 'dqh', 'dw_k', 'dw2', 'db2')


@pytest.mark.parametrize('case', CASES, ids=str)
def test_fp32_emulation_stays_within_half_of_every_bound(case):
    """Measured (worst over the five cases): out 0.014, a 0.014, dkey 0.016, dqh 0.018, dw_k 0.015, dw2 0.007, db2 0.003 of the
    bound, with torch's CPU sigmoid measuring 1.5 u (allowance 3.0 u).  The shares are small because the (n + 2) u sum |terms|
    rule is a worst case over n roundings of one sign, where the roundings of a real sum largely cancel."""
    j = judged(case)
    ratios = dict(out=fr.worst_ratio(j['out32'], j['fwd']['out'], j['fwd']['tol_out']),
                  a=fr.worst_ratio(j['a32'], j['fwd']['a'], j['fwd']['tol_a']))
    for name, got in zip(NAMES, j['grads32']):
        ratios[name] = fr.worst_ratio(got, j['bwd'][name], j['bwd']['tol_' + name])
    print(case, {k: round(v, 3) for k, v in ratios.items()}, j['allow'])
    assert max(ratios.values()) <= 0.5, ratios
    assert not torch.isnan(j['out32']).any() and not torch.isnan(j['grads32'][0]).any()


def test_padded_positions_are_exact_zeros_in_the_referee():
    j = judged(CASES[0])
    pad = j['c']['key_pad']
    assert pad.any() and pad[-1].all() and j['c']['key'][pad].abs().min() > 0
    assert not j['fwd']['a'][pad].any() and not j['bwd']['dkey'][pad].any()
    assert not j['fwd']['out'][-1].any() and not j['bwd']['dqh'][-1].any()
    assert not j['a32'][pad].any() and not j['grads32'][0][pad].any()


def _leaves(diff, tol):
    return bool((diff.abs() > tol).any())


# the cases with a bias and padded positions (non-zero keys there) show every mistake
@pytest.mark.parametrize('mistake', fr.FORWARD_MISTAKES)
@pytest.mark.parametrize('case', [CASES[1], CASES[2]], ids=str)
def test_forward_mistakes_leave_the_bounds(case, mistake):
    j = judged(case)
    c = j['c']
    out, a = fr.layer_rule(c['query'], c['key'], c['w1'], c['b1'], c['w2'], c['b2'], c['key_pad'], mistake)
    assert _leaves(a - j['fwd']['a'], j['fwd']['tol_a']), mistake
    assert _leaves(out - j['fwd']['out'], j['fwd']['tol_out']), mistake


@pytest.mark.parametrize('mistake', fr.BACKWARD_MISTAKES)
@pytest.mark.parametrize('case', [CASES[1], CASES[2]], ids=str)
def test_backward_mistakes_leave_the_bounds(case, mistake):
    j = judged(case)
    wrong = fr.backward(*j['args'], j['k']['g'], None, mistake)
    name = 'dqh' if mistake == 'dqh_over_padded' else 'dkey'
    if mistake == 'slope_missing':
        assert all(_leaves(wrong[n] - j['bwd'][n], j['bwd']['tol_' + n]) for n in ('dkey', 'dqh', 'dw_k')), mistake
    assert _leaves(wrong[name] - j['bwd'][name], j['bwd']['tol_' + name]), mistake


def test_the_rule_itself_stays_inside_the_bounds():
    """The layer-level float64 rule and the kernel-level one agree to far less than any bound (qh is rounded to fp32 between them)."""
    for case in CASES:
        j = judged(case)
        c = j['c']
        out, a = fr.layer_rule(c['query'], c['key'], c['w1'], c['b1'], c['w2'], c['b2'], c['key_pad'])
        assert not _leaves(a - j['fwd']['a'], j['fwd']['tol_a'] + 1e-6) and not _leaves(out - j['fwd']['out'], j['fwd']['tol_out'] + 1e-5)


@pytest.mark.parametrize('bias', [False, True])
def test_twin_equals_the_float64_rule(bias):
    from recstudio_amd import seqmodule
    c = fr.make_case(5, 9, 32, 64, q_dim=64, bias=bias, pad='whole', seed=7)
    d = {k: (v.double() if v is not None and v.is_floating_point() else v) for k, v in c.items()}
    leaves = [d[n].requires_grad_(True) for n in ('query', 'key', 'w1', 'w2', 'b2')] + ([d['b1'].requires_grad_(True)] if bias else [])
    out, a = seqmodule.ff_attention_pool_torch(d['query'], d['key'], d['w1'], d['b1'], d['w2'], d['b2'], d['key_pad'])
    want_out, want_a = fr.layer_rule(c['query'], c['key'], c['w1'], c['b1'], c['w2'], c['b2'], c['key_pad'])
    assert float((out.detach() - want_out).abs().max()) <= 1e-12 and float((a.detach() - want_a).abs().max()) <= 1e-12
    grads = torch.autograd.grad((out * d['g']).sum(), leaves)
    # the kernel-level float64 gradients, from a float64 qh, and the query side's chain rule
    q_dim = 64
    qh = torch.nn.functional.linear(d['query'], d['w1'][:, :q_dim], d['b1']).detach()
    b = fr.backward(d['key'], qh, d['w1'][:, q_dim:], d['w2'], d['b2'], d['key_pad'], 1.0 / q_dim ** 0.5, d['g'])
    want = [b['dqh'] @ d['w1'][:, :q_dim].detach(), b['dkey'], torch.cat([b['dqh'].t() @ d['query'].detach(), b['dw_k']], 1),
            b['dw2'].view(1, -1), b['db2']] + ([b['dqh'].sum(0)] if bias else [])
    for got, w in zip(grads, want):
        assert float((got - w).abs().max()) <= 1e-12


def test_attention_layer_state_dict_and_paths():
    from recstudio_amd import seqmodule
    narm = seqmodule.AttentionLayer(q_dim=128, mlp_layers=[128], bias=False)
    stamp = seqmodule.AttentionLayer(q_dim=128, k_dim=64, mlp_layers=[64])
    assert {k: tuple(v.shape) for k, v in narm.state_dict().items()} == {
        'mlp.0.model.1.weight': (128, 256), 'mlp.1.weight': (1, 128), 'mlp.1.bias': (1,)}
    assert {k: tuple(v.shape) for k, v in stamp.state_dict().items()} == {
        'mlp.0.model.1.weight': (64, 192), 'mlp.0.model.1.bias': (64,), 'mlp.1.weight': (1, 64), 'mlp.1.bias': (1,)}
    g = torch.Generator().manual_seed(3)
    q, k = torch.randn(4, 1, 128, generator=g), torch.randn(4, 7, 64, generator=g)
    pad = torch.arange(7).view(1, 7) >= torch.tensor([7, 1, 4, 0]).view(4, 1)
    out, w = stamp(q, k, k, key_padding_mask=pad, need_weight=True)
    sd = stamp.state_dict()
    want_out, want_w = fr.layer_rule(q[:, 0], k, sd['mlp.0.model.1.weight'], sd['mlp.0.model.1.bias'], sd['mlp.1.weight'],
                                     sd['mlp.1.bias'], pad)
    assert out.shape == (4, 1, 64) and w.shape == (4, 1, 7)
    out, w = out.detach(), w.detach()
    assert float((out[:, 0].double() - want_out).abs().max()) < 1e-5 and float((w[:, 0].double() - want_w).abs().max()) < 1e-5
    # the general path (a copy of the key as the value: not the fused call) gives the same
    out2 = stamp(q, k, k.clone(), key_padding_mask=pad)
    assert torch.allclose(out, out2, atol=1e-6)
    # softmax=True: the reference's -inf fill + softmax
    live = pad[:3]
    out3, w3 = stamp(q[:3], k[:3], k[:3], key_padding_mask=live, need_weight=True, softmax=True)
    assert torch.allclose(w3.sum(-1), torch.ones(3, 1), atol=1e-6) and not w3[:, 0][live].any()


def test_native_argument_checks(nat):
    lib = nat.lib()
    a = nat.FfAttentionArgs()
    a.n_seq, a.seq_len, a.d, a.m, a.scale = 4, 9, 48, 64, 0.1
    assert lib.rsa_ff_attention(ctypes.byref(a), None) == -1          # d outside {32, 64, 128}
    a.d, a.seq_len = 64, 0
    assert lib.rsa_ff_attention(ctypes.byref(a), None) == -1          # seq_len < 1
    a.seq_len, a.n_seq = 9, -1
    assert lib.rsa_ff_attention_backward(ctypes.byref(a), None) == -1
    a.n_seq = 4
    assert lib.rsa_ff_attention(ctypes.byref(a), None) == -1          # null pointers
    a.n_seq = 0
    assert lib.rsa_ff_attention(ctypes.byref(a), None) == 0 and lib.rsa_ff_attention_backward(ctypes.byref(a), None) == 0
    assert lib.rsa_ff_attention_workspace_bytes(4, 9, 48, 64) == -1
    small, big = lib.rsa_ff_attention_workspace_bytes(4, 9, 64, 64), lib.rsa_ff_attention_workspace_bytes(4000, 50, 128, 128)
    assert 0 < small < big
    # the workspace holds nothing of size B S M: B S floats, the waves' slots and fewer than n_tiles + B rows of M
    assert big < 4 * (4000 * 50 + 512 * (128 * 128 + 129) + (4000 * 50 // 32 + 4001) * 128) + 8 * 256


def _cpu_batch(n_items, B, L, seed):
    g = torch.Generator().manual_seed(seed)
    lens = torch.randint(1, L + 1, (B,), generator=g)
    lens[0], lens[1] = L, 1
    ids = torch.randint(1, n_items, (B, L), generator=g) * (torch.arange(L).view(1, L) < lens.view(B, 1))
    return {'in_item_id': ids, 'seqlen': lens}


def test_narm_and_stamp_build_on_ml100k(golden):
    import recstudio_amd as ra
    from recstudio_amd import retriever
    from test_dataset_golden import make
    m = ra.NARM().config['model']
    assert (m['hidden_size'], m['dropout_rate'], m['layer_num'], m['fused_gru']) == (128, [0.25, 0.5], 1, True)
    assert m['fused_attention_pool'] is retriever.FUSED_ATTENTION_POOL_DEFAULT
    assert ra.STAMP().config['model']['embed_dim'] == 64
    assert ra.NARM({'model': {'fused_attention_pool': False}}).config['model']['fused_attention_pool'] is False
    trn, _, _ = make(ra.SeqDataset, golden('data_ml100k'), max_seq_len=20).build(split_ratio=2)
    for cls, flag in ((ra.NARM, True), (ra.NARM, False), (ra.STAMP, True), (ra.STAMP, False)):
        model = cls({'model': {'embed_dim': 64, 'fused_attention_pool': flag}, 'train': {'batch_size': 64}})
        model._init_model(trn)
        model._init_parameter()
        assert isinstance(model.loss_fn, ra.SoftmaxLoss) and isinstance(model.score_func, ra.InnerProductScorer)
        assert model.sampler is None and model._fused_train_path() == 'full_softmax'
        layer = model.query_encoder.attn_layer if cls is ra.NARM else model.query_encoder.attention_layer
        assert isinstance(layer, ra.AttentionLayer) and layer.fused is flag
        batch = _cpu_batch(trn.num_items, 8, 20, 2)
        assert model.query_encoder(batch).shape == (8, 64)


def test_query_encoders_on_cpu_follow_the_reference_graph():
    """NARM's and STAMP's encoders on CPU tensors (the twin path) against the reference's forward written out in float64."""
    from recstudio_amd import retriever
    torch.manual_seed(5)
    emb = torch.nn.Embedding(50, 32, padding_idx=0)
    batch = _cpu_batch(50, 6, 8, 1)
    pad = batch['in_item_id'] == 0
    last = (batch['seqlen'] - 1).view(-1, 1, 1)

    narm = retriever.NARMQueryEncoder('item_id', 32, 64, 1, [0.25, 0.5], emb).eval()
    keys = set(narm.state_dict())
    assert {'item_encoder.weight', 'gru_layer.2.gru.weight_ih_l0', 'gru_layer.2.gru.weight_hh_l0', 'attn_layer.mlp.0.model.1.weight',
            'attn_layer.mlp.1.weight', 'attn_layer.mlp.1.bias', 'fc.1.weight'} == keys
    q = narm(batch)
    sd = {k: v.double() for k, v in narm.state_dict().items()}
    gru = torch.nn.GRU(32, 64, 1, bias=False, batch_first=True).double()
    gru.load_state_dict({'weight_ih_l0': sd['gru_layer.2.gru.weight_ih_l0'], 'weight_hh_l0': sd['gru_layer.2.gru.weight_hh_l0']})
    gv = gru(sd['item_encoder.weight'][batch['in_item_id']])[0]
    h_t = gv.gather(1, last.expand(-1, 1, 64)).squeeze(1)
    c_local, _ = fr.layer_rule(h_t, gv, sd['attn_layer.mlp.0.model.1.weight'], None, sd['attn_layer.mlp.1.weight'],
                               sd['attn_layer.mlp.1.bias'], pad)
    want = torch.cat([h_t, c_local], 1) @ sd['fc.1.weight'].t()
    assert float((q.detach().double() - want).abs().max()) < 1e-5

    stamp = retriever.STAMPQueryEncoder('item_id', 32, emb).eval()
    q = stamp(batch)
    sd = {k: v.double() for k, v in stamp.state_dict().items()}
    rows = sd['item_encoder.weight'][batch['in_item_id']]
    m_t = rows.gather(1, last.expand(-1, 1, 32)).squeeze(1)
    m_s = rows.sum(1) / batch['seqlen'].view(-1, 1).double()
    m_a, _ = fr.layer_rule(torch.cat([m_t, m_s], 1), rows, sd['attention_layer.mlp.0.model.1.weight'],
                           sd['attention_layer.mlp.0.model.1.bias'], sd['attention_layer.mlp.1.weight'],
                           sd['attention_layer.mlp.1.bias'], pad)
    lin = lambda x, n: torch.tanh(x @ sd[n + '.model.1.weight'].t() + sd[n + '.model.1.bias'])     # noqa: E731
    want = lin(m_a, 'mlpA') * lin(m_t, 'mlpB')
    assert float((q.detach().double() - want).abs().max()) < 1e-5
