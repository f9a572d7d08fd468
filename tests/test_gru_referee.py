"""CPU: the float64 referee of the fused GRU recurrence (tests/gru_referee.py) judged on itself -- an fp32 emulation of the kernel's
order of operations inside half its bounds, eleven seeded mistakes outside them --, the argument checks of rsa_gru / rsa_gru_backward
(they run before any HIP call), the torch-op twin against nn.GRU in float64, FusedGRU on CPU tensors and one CPU training step of
GRU4Rec.  No device kernel runs here.  Measured: the emulation within 0.21 of the bounds of out, 0.24 of those of dgi, 0.19 of
those of dgh_n and 0.01 of those of dh0 in all five cases, with torch's CPU sigmoid measuring 1.5 u and its tanh 0.5 u (allowances of
3.0 u and 1.1 u)."""
import ctypes
import functools

import pytest
import torch

import gru_referee as gr
import oracle
from test_dataset_golden import make

# (B, L, H, bias, h0, lengths, seed): lengths mixed and h0 non-zero in the cases the mistakes are shown in
CASES = [(5, 9, 32, True, True, 'mixed', 1), (19, 12, 64, True, True, 'mixed', 2), (4, 20, 128, False, True, 'mixed', 3),
         (3, 7, 32, False, False, None, 4), (18, 5, 64, True, False, 'full', 5)]


@pytest.fixture(scope='module')
def nat():
    import os
    from recstudio_amd import _native
    if not os.path.exists(_native.LIB_PATH):
        _native.build()
    return _native


@functools.lru_cache(maxsize=None)
def judged(case):
    B, L, H, bias, with_h0, lengths, seed = case
    c = gr.make_case(B, L, H, bias=bias, with_h0=with_h0, lengths=lengths, seed=seed)
    out32, gh32, (dgi32, dghn32, dh032) = gr.emulate_fp32(c['gi'], c['w_hh'], c['b_hh'], c['h0'], c['lengths'], c['g_out'])
    allow = gr.activation_allowance('cpu', torch.cat([c['gi'].reshape(-1), gh32.reshape(-1)]))
    want, tol = gr.judge_forward(out32, c['gi'], c['w_hh'], c['b_hh'], c['h0'], c['lengths'], allow)
    b = gr.backward(c['gi'], gh32, out32, c['w_hh'], c['h0'], c['g_out'], c['lengths'], allow)
    return dict(c=c, out32=out32, gh32=gh32, dgi32=dgi32, dghn32=dghn32, dh032=dh032, allow=allow, want=want, tol=tol, b=b)


@pytest.mark.parametrize('case', CASES, ids=str)
def test_fp32_emulation_stays_within_half_of_every_bound(case):
    j = judged(case)
    b = j['b']
    ratios = dict(out=gr.worst_ratio(j['out32'], j['want'], j['tol']), dgi=gr.worst_ratio(j['dgi32'], b['dgi'], b['tol_dgi']),
                  dgh_n=gr.worst_ratio(j['dghn32'], b['dgh_n'], b['tol_dgh_n']), dh0=gr.worst_ratio(j['dh032'], b['dh0'], b['tol_dh0']))
    print(case, ratios, j['allow'])
    assert max(ratios.values()) <= 0.5, ratios
    assert not torch.isnan(j['out32']).any() and not torch.isnan(j['dgi32']).any()


def test_positions_past_the_length_are_exact_zeros_in_the_referee():
    j = judged(CASES[0])
    c, b = j['c'], j['b']
    dead = ~gr.live_mask(c['lengths'], 5, 9)
    assert dead.any() and (c['lengths'] == 0).any()
    full = gr.forward(c['gi'], c['w_hh'], c['b_hh'], c['h0'], c['lengths'])
    assert not full[dead].any() and not j['want'][dead].any() and not b['dgi'][dead].any() and not b['dgh_n'][dead].any()
    assert not j['out32'][dead].any() and not j['dgi32'][dead].any() and not j['dghn32'][dead].any()
    assert float(j['tol'][dead].max()) < 1e-35 and float(b['tol_dgi'][dead].max()) < 1e-35
    empty = c['lengths'] == 0                       # nothing flows into h0 of an empty row
    assert not b['dh0'][empty].any() and not j['dh032'][empty].any()


def _judge_a_mistake(j, mistake):
    """The mistake made in float64 (no rounding of its own), judged as a kernel's output would be -> the worst share of a bound."""
    c = j['c']
    if mistake in gr.FORWARD_MISTAKES and not mistake.endswith('@backward'):
        out_m = gr.forward(c['gi'], c['w_hh'], c['b_hh'], c['h0'], c['lengths'], mistake=mistake)
        want, tol = gr.judge_forward(out_m, c['gi'], c['w_hh'], c['b_hh'], c['h0'], c['lengths'], j['allow'])
        return gr.worst_ratio(out_m, want, tol)
    mistake = mistake.replace('@backward', '')
    b, m = j['b'], gr.backward(c['gi'], j['gh32'], j['out32'], c['w_hh'], c['h0'], c['g_out'], c['lengths'], mistake=mistake)
    return max(gr.worst_ratio(m['dgi'], b['dgi'], b['tol_dgi']), gr.worst_ratio(m['dgh_n'], b['dgh_n'], b['tol_dgh_n']),
               gr.worst_ratio(m['dh0'], b['dh0'], b['tol_dh0']))


MISTAKES = ['gate_order_zrn', 'w_hn_of_rh', 'b_hn_outside', 'blend_swapped', 'w_transposed', 'past_len', 'dz_from_h_t',
            'carry_without_dh_z', 'past_len@backward', 'dgh_n_without_r', 'w_untransposed@backward']


@pytest.mark.parametrize('mistake', MISTAKES)
def test_a_seeded_mistake_leaves_a_bound(mistake):
    """Each mistake leaves a bound in every case with mixed lengths and a non-zero h0 (b_hn outside r * (.) needs a bias)."""
    shown = 0
    for case in CASES[:3]:
        if mistake == 'b_hn_outside' and not case[3]:
            continue
        worst = _judge_a_mistake(judged(case), mistake)
        assert worst > 1.0, (mistake, case, worst)
        shown += 1
    assert shown >= 2


# ---------------------------------------------------------------------------------------------------------------- the C ABI
def _block(nat, n_seq=8, L=20, H=64):
    a = nat.GruArgs()
    for name in ('gi', 'w_hh', 'b_hh', 'h0', 'lengths', 'out', 'gh', 'g_out', 'dgi', 'dgh_n', 'dh0'):
        setattr(a, name, 4096)
    a.n_seq, a.seq_len, a.hidden = n_seq, L, H
    return a


@pytest.mark.parametrize('entry', ['rsa_gru', 'rsa_gru_backward'])
def test_argument_checks_run_before_any_hip_call(nat, entry):
    lib = nat.lib()
    fn = getattr(lib, entry)

    def refused(a, text):
        assert fn(ctypes.byref(a), None) == -1
        assert text in lib.rsa_last_error(), lib.rsa_last_error()

    assert fn(None, None) == -1
    a = _block(nat)
    a.size = 0
    refused(a, b'size')
    for H in (0, 16, 48, 96, 256):
        refused(_block(nat, H=H), b'hidden')
    refused(_block(nat, n_seq=-1), b'negative')
    refused(_block(nat, L=-1), b'negative')
    for bad in (-1, 21):                                                   # a negative length, and one above L
        lens = (ctypes.c_int64 * 8)(20, 1, 0, 5, bad, 7, 20, 3)
        a = _block(nat)
        a.lengths_host = ctypes.addressof(lens)
        refused(a, b'lengths[4]')
    fields = ('w_hh', 'gi', 'out') + (('gh', 'g_out', 'dgi', 'dgh_n', 'dh0') if entry == 'rsa_gru_backward' else ())
    for field in fields:
        a = _block(nat)
        setattr(a, field, None)
        refused(a, b'null')
        setattr(a, field, 4104)
        refused(a, b'16-byte aligned')
    assert fn(ctypes.byref(_block(nat, n_seq=0)), None) == 0               # nothing to do: no launch, no HIP call
    assert lib.rsa_abi_version() == 13


def test_ops_refuse_mismatched_shapes_without_a_device():
    from recstudio_amd import ops
    gi, w = torch.zeros(2, 3, 96), torch.zeros(96, 32)
    with pytest.raises(RuntimeError, match='GPU only'):
        ops.gru_sequence(gi, w)
    assert ops.GRU_HIDDEN_SIZES == (32, 64, 128)


# ---------------------------------------------------------------------------------------------------------------- the twin
def _stock(I, H, layers, bias, seed):
    torch.manual_seed(seed)
    return torch.nn.GRU(input_size=I, hidden_size=H, num_layers=layers, bias=bias, batch_first=True).double()


@pytest.mark.parametrize('bias', [False, True], ids=['nobias', 'bias'])
def test_the_torch_twin_is_nn_gru_in_float64(bias):
    import torch.nn.functional as F
    from recstudio_amd import seqmodule
    B, L, I, H = 4, 11, 24, 32
    gru = _stock(I, H, 1, bias, 3)
    gen = torch.Generator().manual_seed(5)
    x = torch.randn(B, L, I, dtype=torch.float64, generator=gen)
    h0 = torch.randn(B, H, dtype=torch.float64, generator=gen)
    b_ih, b_hh = (gru.bias_ih_l0, gru.bias_hh_l0) if bias else (None, None)
    gi = F.linear(x, gru.weight_ih_l0, b_ih)
    for first in (None, h0):
        want, _ = gru(x, None if first is None else first.unsqueeze(0))
        got = seqmodule.gru_sequence_torch(gi, gru.weight_hh_l0, b_hh, first)
        torch.testing.assert_close(got, want, rtol=1e-12, atol=1e-12)
        torch.testing.assert_close(got, gr.forward(gi, gru.weight_hh_l0, b_hh, first), rtol=1e-12, atol=1e-12)
    lengths = torch.tensor([11, 1, 0, 6])
    want, _ = gru(x, h0.unsqueeze(0))
    got = seqmodule.gru_sequence_torch(gi, gru.weight_hh_l0, b_hh, h0, lengths)
    on = gr.live_mask(lengths, B, L)
    torch.testing.assert_close(got[on], want[on], rtol=1e-12, atol=1e-12)
    assert not got[~on].any()
    torch.testing.assert_close(got, gr.forward(gi, gru.weight_hh_l0, b_hh, h0, lengths), rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize('bias', [False, True], ids=['nobias', 'bias'])
def test_two_layers_of_the_twin_are_nn_gru_in_float64(bias):
    from recstudio_amd import seqmodule
    B, L, I, H = 3, 8, 16, 32
    gru = _stock(I, H, 2, bias, 9)
    gen = torch.Generator().manual_seed(6)
    x = torch.randn(B, L, I, dtype=torch.float64, generator=gen)
    h0 = torch.randn(2, B, H, dtype=torch.float64, generator=gen)
    fused = seqmodule.FusedGRU(gru)
    assert fused.fused(x)
    for first in (None, h0):
        (got, got_n), (want, want_n) = fused(x, first), gru(x, first)
        torch.testing.assert_close(got, want, rtol=1e-12, atol=1e-12)
        torch.testing.assert_close(got_n, want_n, rtol=1e-12, atol=1e-12)


def test_the_twins_autograd_is_the_referees_bptt():
    import torch.nn.functional as F
    from recstudio_amd import seqmodule
    j = judged(CASES[0])
    c = j['c']
    gi, w, b, h0 = (c[k].double().requires_grad_(True) for k in ('gi', 'w_hh', 'b_hh', 'h0'))
    out = seqmodule.gru_sequence_torch(gi, w, b, h0, c['lengths'])
    out.backward(c['g_out'].double())
    gh = F.linear(gr.previous_states(out.detach(), h0.detach()), w.detach(), b.detach())
    ref = gr.backward(gi, gh, out, w, h0, c['g_out'], c['lengths'])
    torch.testing.assert_close(gi.grad, ref['dgi'], rtol=1e-11, atol=1e-13)
    torch.testing.assert_close(h0.grad, ref['dh0'], rtol=1e-11, atol=1e-13)


@pytest.mark.parametrize('bias', [False, True], ids=['nobias', 'bias'])
def test_fused_gru_on_cpu_tensors_goes_through_the_twin(bias, monkeypatch):
    """Two layers, float32, against the wrapped nn.GRU (out, h_n and every gradient); state_dict keys are the wrapped module's."""
    from recstudio_amd import seqmodule
    B, L, I, H = 5, 9, 16, 32
    torch.manual_seed(7)
    gru = torch.nn.GRU(I, H, num_layers=2, bias=bias, batch_first=True)
    holder = torch.nn.Module()
    holder.gru = gru
    holder.fused = seqmodule.FusedGRU(gru)
    assert list(holder.state_dict()) == ['gru.' + k for k in gru.state_dict()]
    calls = []
    real = seqmodule.gru_sequence_torch
    monkeypatch.setattr(seqmodule, 'gru_sequence_torch', lambda *a: (calls.append(1), real(*a))[1])
    x = torch.randn(B, L, I, requires_grad=True)
    h0 = torch.randn(2, B, H)
    out, h_n = holder.fused(x, h0)
    assert len(calls) == 2 and holder.fused.fused(x)
    g = torch.randn(B, L, H)
    (out * g).sum().backward()
    got = [x.grad.clone()] + [p.grad.clone() for p in gru.parameters()]
    x.grad = None
    gru.zero_grad()
    want, want_n = gru(x, h0)
    (want * g).sum().backward()
    torch.testing.assert_close(out, want, rtol=1e-4, atol=1e-6)
    torch.testing.assert_close(h_n, want_n, rtol=1e-4, atol=1e-6)
    for a, b in zip(got, [x.grad] + [p.grad for p in gru.parameters()]):
        torch.testing.assert_close(a, b, rtol=3e-4, atol=3e-6 * float(b.abs().max()))
    # lengths: nn.GRU at t < len, zeros beyond, h_n the state at len - 1
    lengths = torch.tensor([9, 1, 4, 9, 2])
    out, h_n = holder.fused(x, h0, lengths)
    on = gr.live_mask(lengths, B, L)
    torch.testing.assert_close(out[on], want[on], rtol=1e-4, atol=1e-6)
    assert not out[~on].any()
    torch.testing.assert_close(h_n[1], out[torch.arange(B), lengths - 1], rtol=0, atol=0)
    # what the kernel cannot do falls back to the wrapped module
    for other in (torch.nn.GRU(I, 48, batch_first=True), torch.nn.GRU(I, H, batch_first=True, bidirectional=True),
                  torch.nn.GRU(I, H)):
        f = seqmodule.FusedGRU(other)
        assert not f.fused(x)
        a, b = f(x.detach()), other(x.detach())
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    with pytest.raises(TypeError):
        seqmodule.FusedGRU(torch.nn.LSTM(I, H))


def test_gru4rec_builds_on_ml100k_and_takes_a_cpu_step(golden):
    import recstudio_amd as ra
    assert ra.GRU4Rec().config['model']['fused_gru'] is True
    m = ra.GRU4Rec().config
    assert (m['model']['hidden_size'], m['model']['dropout_rate'], m['model']['layer_num'], m['train']['negative_count']) == \
        (128, 0.3, 1, 1)
    trn, val, tst = make(ra.SeqDataset, golden('data_ml100k'), max_seq_len=20).build(split_ratio=2)
    model = ra.GRU4Rec({'model': {'embed_dim': 64, 'hidden_size': 64}, 'train': {'batch_size': 64}})
    model._init_model(trn)
    model._init_parameter()
    enc = model.query_encoder
    assert enc._fused is not None and isinstance(enc.gru, torch.nn.GRU) and not enc.gru.bias and enc.gru.batch_first
    assert [k for k in enc.state_dict() if k.startswith('gru.')] == ['gru.weight_ih_l0', 'gru.weight_hh_l0']
    assert isinstance(model.loss_fn, ra.BPRLoss) and isinstance(model.score_func, ra.InnerProductScorer)
    assert isinstance(model.sampler, ra.UniformSampler)
    gen = torch.Generator().manual_seed(0)
    B, L, N = 32, 20, trn.num_items
    seqlen = torch.randint(1, L + 1, (B,), generator=gen)
    hist = torch.randint(1, N, (B, L), generator=gen)
    hist[torch.arange(L).view(1, -1) >= seqlen.view(-1, 1)] = 0
    pos, neg = torch.randint(1, N, (B,), generator=gen), torch.randint(1, N, (B, 1), generator=gen)
    model.train()
    query = enc({'in_' + model.fiid: hist, 'seqlen': seqlen})
    ps = (query * model.item_encoder(pos)).sum(-1)
    ns = (query.unsqueeze(1) * model.item_encoder(neg)).sum(-1)
    loss = oracle.bpr_loss(ps, ns)              # the rule of BPRLoss in torch ops (the package's loss kernels need a device)
    loss.backward()
    assert torch.isfinite(loss) and all(torch.isfinite(p.grad).all() for p in enc.gru.parameters())
    assert enc.gru.weight_hh_l0.grad.abs().max() > 0
