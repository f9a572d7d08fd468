"""GPU: the fused GRU recurrence (ops.gru_sequence / ops.gru_sequence_backward: rsa_gru.hip) against the float64 referee
(tests/gru_referee.py).  The forward is judged step by step from the kernel's own h_{t-1}, the backward against the float64 BPTT of
the kernel's own inputs; every element of out, dgi, dgh_n and dh0 inside its bound, exact zeros at t >= len, two runs bit-equal, 64-bit
offsets, peak memory, and the autograd node against the torch-op twin.

Measured on an MI355X over the 8 shapes x 4 length forms x h0 x bias: out within 0.26, dgi 0.33, dgh_n 0.25 and dh0 0.02 of their
bounds (past 4 GiB: 0.02, 0.19, 0.17, 0.004), with torch's device sigmoid measuring 1.5 u and its tanh 1.3 u against float64
(allowances of 3.0 u and 2.6 u); the forward's peak memory is exactly out, the backward's exactly its three outputs.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

import gru_referee as gr

pytestmark = pytest.mark.gpu

DEV = 'cuda'
SHAPES = [(1, 1, 32), (3, 9, 32), (15, 2, 64), (16, 20, 64), (17, 20, 64), (33, 50, 128), (5, 70, 128), (300, 20, 128)]
LENGTHS = [None, 'ones', 'full', 'mixed']
WORST = {}


@pytest.fixture(scope='module')
def ops():
    import recstudio_amd
    recstudio_amd._native.lib()
    torch.cuda.init()
    return recstudio_amd.ops


@functools.lru_cache(maxsize=None)
def device_allowance():
    """torch's own fp32 sigmoid / tanh on this device against float64, over the fixed grid and the range the cases' pre-activations
    lie in (a denser grid over [-8, 8]): measured once, shared by every case."""
    return gr.activation_allowance(DEV, torch.linspace(-8.0, 8.0, 1 << 18))


def dev(t):
    return None if t is None else t.to(DEV)


def run_and_judge(ops, c, rows=None):
    """One forward and one backward of the kernels on the case ``c``; judged on ``rows`` (a slice of the batch; None: all).
    -> the worst share of a bound per output."""
    allow = device_allowance()
    gi, w, b, h0, lens, g_out = (dev(c[k]) for k in ('gi', 'w_hh', 'b_hh', 'h0', 'lengths', 'g_out'))
    B, L, H = g_out.shape
    out = ops.gru_sequence(gi, w, b_hh=b, h0=h0, lengths=lens)
    first = h0.view(B, 1, H) if h0 is not None else out.new_zeros(B, 1, H)
    gh = F.linear(torch.cat([first, out[:, :-1]], dim=1), w, b)
    dgi, dgh_n, dh0 = ops.gru_sequence_backward(gi, gh, out, w, g_out, h0=h0, lengths=lens)
    again = ops.gru_sequence(gi, w, b_hh=b, h0=h0, lengths=lens)
    again_b = ops.gru_sequence_backward(gi, gh, out, w, g_out, h0=h0, lengths=lens)
    assert torch.equal(out, again) and all(torch.equal(x, y) for x, y in zip((dgi, dgh_n, dh0), again_b))     # bit-equal
    sl = slice(None) if rows is None else rows
    cut = lambda t: None if t is None else t[sl].cpu()              # noqa: E731
    want, tol = gr.judge_forward(cut(out), cut(gi), w, b, cut(h0), cut(lens), allow)
    ref = gr.backward(cut(gi), cut(gh), cut(out), w, cut(h0), cut(g_out), cut(lens), allow)
    ratios = dict(out=gr.worst_ratio(cut(out), want, tol), dgi=gr.worst_ratio(cut(dgi), ref['dgi'], ref['tol_dgi']),
                  dgh_n=gr.worst_ratio(cut(dgh_n), ref['dgh_n'], ref['tol_dgh_n']),
                  dh0=gr.worst_ratio(cut(dh0), ref['dh0'], ref['tol_dh0']))
    n = want.shape[0]
    dead = ~gr.live_mask(cut(lens), n, L)
    for name, t in (('out', out), ('dgi', dgi), ('dgh_n', dgh_n)):
        assert not cut(t)[dead].any(), f'{name} is not exactly 0 at t >= len'
        assert not torch.signbit(cut(t)[dead]).any(), f'{name} holds -0 at t >= len'
    if lens is not None:
        assert not cut(dh0)[cut(lens) == 0].any()
    assert not torch.isnan(out).any() and not torch.isnan(dgi).any() and not torch.isnan(dh0).any()
    return ratios


@pytest.mark.parametrize('lengths', LENGTHS, ids=lambda v: f'len_{v}')
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_every_element_within_its_bound(ops, shape, lengths):
    """With and without h0, with and without b_hh; 'mixed' has lengths that differ inside a tile, an empty row, and a first tile
    whose rows are all shorter than L (the early stop)."""
    B, L, H = shape
    for with_h0 in (False, True):
        for bias in (False, True):
            c = gr.make_case(B, L, H, bias=bias, with_h0=with_h0, lengths=lengths, seed=3)
            if lengths == 'mixed' and L > 1:
                assert int(c['lengths'][:16].max()) < L
            ratios = run_and_judge(ops, c)
            print(shape, lengths, 'h0' if with_h0 else '-', 'bias' if bias else '-', {k: round(v, 3) for k, v in ratios.items()})
            for k, v in ratios.items():
                WORST[k] = max(WORST.get(k, 0.0), v)
            assert max(ratios.values()) <= 1.0, ratios
    print('worst so far', {k: round(v, 3) for k, v in WORST.items()}, device_allowance())


def test_offsets_past_4_gib(ops):
    """B = 140 005, L = 20, H = 128: gi, gh and dgi are 4.3 GB each, so the rows from 139 811 on lie past byte offset 2^32; the last
    tile (five rows: 140 000 ..) is judged against the referee, mixed lengths."""
    B, L, H = 140_005, 20, 128
    g = torch.Generator(device=DEV).manual_seed(5)
    k = 2.0 / H ** 0.5
    c = dict(gi=torch.empty(B, L, 3 * H, device=DEV).normal_(generator=g),
             w_hh=(torch.rand(3 * H, H, device=DEV, generator=g) * 2 - 1) * k,
             b_hh=torch.rand(3 * H, device=DEV, generator=g) - 0.5,
             h0=torch.tanh(torch.empty(B, H, device=DEV).normal_(generator=g)),
             lengths=torch.randint(0, L + 1, (B,), device=DEV, generator=g),
             g_out=torch.empty(B, L, H, device=DEV).normal_(generator=g))
    c['lengths'][-1], c['lengths'][-2] = L, 1
    assert (B - 5) * L * 3 * H * 4 > 1 << 32
    ratios = run_and_judge(ops, c, rows=slice(B - 5, B))
    print('past 4 GiB', ratios)
    assert max(ratios.values()) <= 1.0, ratios


def _peak_above(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    keep = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del keep
    return peak


def test_peak_memory_is_the_outputs(ops):
    B, L, H = 4096, 20, 128
    c = {k: dev(v) for k, v in gr.make_case(B, L, H, bias=True, with_h0=True, lengths='mixed', seed=1).items()}
    out = ops.gru_sequence(c['gi'], c['w_hh'], b_hh=c['b_hh'], h0=c['h0'], lengths=c['lengths'])
    gh = F.linear(torch.cat([c['h0'].view(B, 1, H), out[:, :-1]], dim=1), c['w_hh'], c['b_hh'])
    fwd = _peak_above(lambda: ops.gru_sequence(c['gi'], c['w_hh'], b_hh=c['b_hh'], h0=c['h0'], lengths=c['lengths']))
    bwd = _peak_above(lambda: ops.gru_sequence_backward(c['gi'], gh, out, c['w_hh'], c['g_out'], h0=c['h0'], lengths=c['lengths']))
    print('peak bytes: forward', fwd, 'of', out.nbytes, 'backward', bwd, 'of', (4 * B * L * H + B * H) * 4)
    assert fwd <= out.nbytes + (1 << 20)
    assert bwd <= (4 * B * L * H + B * H) * 4 + (1 << 20)


@pytest.mark.parametrize('bias,with_h0,lengths', [(True, True, 'mixed'), (False, False, None)], ids=['bias_h0_mixed', 'plain'])
def test_autograd_node_against_the_twin(ops, bias, with_h0, lengths):
    """seqmodule._GruFn (the kernels and the backward's three GEMMs) against seqmodule.gru_sequence_torch in float64 under autograd:
    1e-4 on out, 3e-4 on the gradients of gi, w_hh, b_hh and h0 (with 3e-4 / 100 of a gradient's largest magnitude for the elements
    that cancel)."""
    from recstudio_amd import seqmodule
    B, L, H = 37, 20, 64
    c = gr.make_case(B, L, H, bias=bias, with_h0=with_h0, lengths=lengths, seed=8)
    names = [k for k in ('gi', 'w_hh', 'b_hh', 'h0') if c[k] is not None]
    leaves = {k: c[k].to(DEV).requires_grad_(True) for k in names}
    out = seqmodule.gru_sequence(leaves['gi'], leaves['w_hh'], leaves.get('b_hh'), leaves.get('h0'), dev(c['lengths']))
    assert out.grad_fn is not None and type(out.grad_fn).__name__ == '_GruFnBackward'
    out.backward(c['g_out'].to(DEV))
    ref = {k: c[k].double().requires_grad_(True) for k in names}
    want = seqmodule.gru_sequence_torch(ref['gi'], ref['w_hh'], ref.get('b_hh'), ref.get('h0'), c['lengths'])
    want.backward(c['g_out'].double())
    torch.testing.assert_close(out.detach().cpu().double(), want.detach(), rtol=1e-4, atol=1e-6)
    for k in names:
        g = ref[k].grad
        torch.testing.assert_close(leaves[k].grad.cpu().double(), g, rtol=3e-4, atol=3e-6 * float(g.abs().max()))


def test_ops_refuse_what_the_kernel_cannot_do(ops):
    gi, w = torch.zeros(2, 3, 96, device=DEV), torch.zeros(96, 32, device=DEV)
    with pytest.raises(ValueError, match='hidden size'):
        ops.gru_sequence(torch.zeros(2, 3, 144, device=DEV), torch.zeros(144, 48, device=DEV))
    with pytest.raises(ValueError, match='gi must be'):
        ops.gru_sequence(gi, torch.zeros(96, 64, device=DEV))
    with pytest.raises(ValueError, match='h0 must be'):
        ops.gru_sequence(gi, w, h0=torch.zeros(3, 32, device=DEV))
    with pytest.raises(ValueError, match='lengths must be'):
        ops.gru_sequence(gi, w, lengths=torch.zeros(3, dtype=torch.int64, device=DEV))
    with pytest.raises(Exception, match=r'lengths\[1\]'):
        ops.gru_sequence(gi, w, lengths=torch.tensor([1, 4]))                       # a host tensor is checked by the entry
    out = ops.gru_sequence(gi, w, lengths=torch.tensor([1, 3]))
    assert out.shape == (2, 3, 32) and not out.any()
    assert ops.gru_sequence(gi[:0], w).shape == (0, 3, 32)
