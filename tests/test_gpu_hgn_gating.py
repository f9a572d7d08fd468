"""GPU: ops.hgn_gating / ops.hgn_gating_backward (rsa_gating.hip) against the float64 referee (tests/hgn_referee.py): every
element of out, w, dS, dug, dui, dW1 and dw3 inside its bound at the tile edges (L = 31, 32, 33), with a sequence across several
tiles (L = 50, 70), several sequences in one tile (L = 1, 9, 20) and more than one workgroup (B = 300), under no padding, a
zero-row suffix and one sequence padded whole, for mean and max pooling; W_g_1 is always a view inside a wider NaN-filled buffer.
Worst shares of the bounds over the 54 cases, as printed by test_every_element_within_its_bound on the MI355X:
    out 0.069   w 0.235   dS 0.244   dug 0.014   dui 0.015   dW1 0.014   dw3 0.007
with the device's own fp32 sigmoid measuring 1.5 u against float64 (allowance 3.0 u).  w and dS come closest because their bounds
are the shortest: at a padded position w = sigmoid(ui) carries little more than the allowance, and dS there is g + dsf f, two
roundings against 4 u (|g| + |acc|).  The case past 4 GiB: out 0.003, w 0.220, dS 0.236, dug 0.001, dui 0.002.
"""
import pytest
import torch

import hgn_referee as hr

pytestmark = pytest.mark.gpu

DEV = 'cuda'
SHAPES = [(1, 1, 32), (3, 9, 32), (2, 31, 64), (2, 32, 64), (2, 33, 64), (3, 20, 64), (5, 50, 128), (2, 70, 128), (300, 20, 64)]
NAMES = ('dS', 'dug', 'dui', 'dw1', 'dw3')
WORST = {}


@pytest.fixture(scope='module')
def ops():
    import recstudio_amd
    recstudio_amd._native.lib()
    torch.cuda.init()
    return recstudio_amd.ops


def device_inputs(k):
    """The kernel's inputs on the device; w1 as rows [1, 1 + d), columns [8, 8 + d) of a wider NaN-filled matrix."""
    d = k['w1'].shape[0]
    wide = torch.full((d + 2, d + 12), float('nan'))
    wide[1:1 + d, 8:8 + d] = k['w1']
    wide = wide.to(DEV)
    return dict(S=k['S'].to(DEV), ug=k['ug'].to(DEV), ui=k['ui'].to(DEV), w1=wide[1:1 + d, 8:8 + d], w3=k['w3'].to(DEV),
                g=k['g'].to(DEV), wide=wide)


def allowance(k):
    """The device's sigmoid against float64 on the fixed grid and on the case's own arguments of both gates."""
    B, L, D = k['S'].shape
    pre = k['ug'].view(B, 1, D) + k['S'] @ k['w1'].t()
    z = (k['S'] * torch.sigmoid(pre)) @ k['w3'] + k['ui']
    return hr.sigmoid_allowance(DEV, torch.cat([pre.reshape(-1), z.reshape(-1)]))


def run(ops, d, pooling):
    out, w, arg = ops.hgn_gating(d['S'], d['ug'], d['ui'], d['w1'], d['w3'], pooling)
    grads = ops.hgn_gating_backward(d['S'], d['ug'], d['ui'], d['w1'], d['w3'], w, arg, d['g'], pooling)
    return out, w, arg, grads


@pytest.mark.parametrize('pooling', hr.POOLINGS)
@pytest.mark.parametrize('pad', hr.PADS, ids=str)
@pytest.mark.parametrize('shape', SHAPES, ids=str)
def test_every_element_within_its_bound(ops, shape, pad, pooling):
    """Measured on the MI355X: the worst shares of the bounds are in the module docstring."""
    B, L, D = shape
    c = hr.make_case(B, L, D, pad=pad, seed=3)
    k = hr.kernel_inputs(c)
    d = device_inputs(k)
    assert d['w1'].stride(0) == D + 12 and d['w1'].data_ptr() == d['wide'].data_ptr() + 4 * (D + 12 + 8)   # read in place
    out, w, arg, grads = run(ops, d, pooling)
    out2, w2, arg2, grads2 = run(ops, d, pooling)
    torch.cuda.synchronize()
    allow = allowance(k)
    args = (k['S'], k['ug'], k['ui'], k['w1'], k['w3'], pooling)
    fwd = hr.judge_forward(*args, allow)
    bwd = hr.backward(*args, k['g'], arg=arg, allow=allow)
    ratios = dict(out=hr.worst_ratio(out, fwd['out'], fwd['tol_out']), w=hr.worst_ratio(w, fwd['w'], fwd['tol_w']))
    for name, got in zip(NAMES, grads):
        assert got.shape == bwd[name].shape, name
        ratios[name] = hr.worst_ratio(got, bwd[name], bwd['tol_' + name])
    for n, v in ratios.items():
        WORST[n] = max(WORST.get(n, 0.0), v)
    print(shape, pad, pooling, {n: round(v, 3) for n, v in ratios.items()}, 'worst so far',
          {n: round(v, 3) for n, v in WORST.items()}, allow)
    for t in (out, w) + tuple(grads):
        assert not torch.isnan(t).any()                                    # nothing of the NaN frame around W_g_1 leaks
    assert max(ratios.values()) <= 1.0, ratios
    if pooling == 'max':
        assert arg.dtype == torch.int32 and arg.shape == (B, D)
        assert hr.arg_problems(fwd, arg).numel() == 0
    else:
        assert arg is None
    # two runs are bit-equal
    for x, y in zip((out, w) + tuple(grads), (out2, w2) + tuple(grads2)):
        assert torch.equal(x, y)
    if pooling == 'max':
        assert torch.equal(arg, arg2)
    # a sequence padded whole: out is exactly 0 under mean, arg is 0 everywhere under max
    if pad == 'whole':
        assert not c['S'][B - 1].any()
        if pooling == 'mean':
            assert not out[B - 1].view(torch.int32).any()
        else:
            assert not arg[B - 1].any() and not out[B - 1].any()
    assert torch.isnan(d['wide'][0]).all() and torch.isnan(d['wide'][:, :8]).all() and torch.isnan(d['wide'][:, 8 + D:]).all()


def test_b_zero_and_refused_width(ops):
    z = lambda *s: torch.zeros(*s, device=DEV)         # noqa: E731
    for pooling in hr.POOLINGS:
        out, w, arg = ops.hgn_gating(z(0, 5, 32), z(0, 32), z(0, 5), z(32, 32), z(32), pooling)
        assert out.shape == (0, 32) and w.shape == (0, 5) and (arg is None) == (pooling == 'mean')
        dS, dug, dui, dw1, dw3 = ops.hgn_gating_backward(z(0, 5, 32), z(0, 32), z(0, 5), z(32, 32), z(32), w, arg, z(0, 32), pooling)
        assert dS.shape == (0, 5, 32) and dug.shape == (0, 32) and dui.shape == (0, 5) and not dw1.any() and not dw3.any()
    with pytest.raises(ValueError):
        ops.hgn_gating(z(2, 5, 48), z(2, 48), z(2, 5), z(48, 48), z(48), 'mean')
    with pytest.raises(ValueError):
        ops.hgn_gating(z(2, 5, 32), z(2, 32), z(2, 5), z(32, 32), z(32), 'avg')


def test_offsets_past_four_gib(ops):
    """S and dS of B = 16448, L = 512, d = 128 end past byte offset 4 GiB: the last two sequences, which lie there, are judged
    against the referee of those sequences alone (out, w, dS, dug and dui are per-sequence), mean pooling."""
    B, L, D, T = 16448, 512, 128, 2
    assert B * L * D * 4 > 1 << 32 and (B - T) * L * D * 4 > 1 << 32
    gen = torch.Generator(device=DEV).manual_seed(9)
    S = torch.randn(B, L, D, device=DEV, generator=gen)
    lens = torch.randint(1, L + 1, (B,), device=DEV, generator=gen)
    S.mul_((torch.arange(L, device=DEV).view(1, L) < lens.view(B, 1)).unsqueeze(2))
    ug = torch.randn(B, D, device=DEV, generator=gen)
    ui = torch.randn(B, L, device=DEV, generator=gen)
    g = torch.randn(B, D, device=DEV, generator=gen)
    w1 = (torch.rand(D, D, device=DEV, generator=gen) * 2 - 1) * 0.15
    w3 = (torch.rand(D, device=DEV, generator=gen) * 2 - 1) * 0.15
    out, w, arg = ops.hgn_gating(S, ug, ui, w1, w3, 'mean')
    dS, dug, dui, dw1, dw3 = ops.hgn_gating_backward(S, ug, ui, w1, w3, w, arg, g, 'mean')
    torch.cuda.synchronize()
    tS, tug, tui, tg = [t[B - T:].cpu() for t in (S, ug, ui, g)]
    allow = allowance(dict(S=tS, ug=tug, ui=tui, w1=w1.cpu(), w3=w3.cpu()))
    args = (tS, tug, tui, w1.cpu(), w3.cpu(), 'mean')
    fwd = hr.judge_forward(*args, allow)
    bwd = hr.backward(*args, tg, allow=allow)
    ratios = dict(out=hr.worst_ratio(out[B - T:], fwd['out'], fwd['tol_out']), w=hr.worst_ratio(w[B - T:], fwd['w'], fwd['tol_w']),
                  dS=hr.worst_ratio(dS[B - T:], bwd['dS'], bwd['tol_dS']), dug=hr.worst_ratio(dug[B - T:], bwd['dug'], bwd['tol_dug']),
                  dui=hr.worst_ratio(dui[B - T:], bwd['dui'], bwd['tol_dui']))
    print(ratios)
    assert max(ratios.values()) <= 1.0, ratios
    assert not torch.isnan(dw1).any() and not torch.isnan(dw3).any()


def test_peak_memory(ops):
    """At B = 1024, L = 64, d = 64 one [B, L, d] tensor is 16 MiB.  The forward's peak above its inputs is at most out + w + arg +
    1 MiB; the backward's at most its outputs + the workspace + 1 MiB."""
    import recstudio_amd
    B, L, D = 1024, 64, 64
    assert B * L * D * 4 == 16 << 20
    k = hr.kernel_inputs(hr.make_case(B, L, D, pad='suffix', seed=5))
    d = device_inputs(k)
    mib = 1 << 20
    for pooling in hr.POOLINGS:
        run(ops, d, pooling)                                                # (the LDS grant and the library load are behind us)
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        res = ops.hgn_gating(d['S'], d['ug'], d['ui'], d['w1'], d['w3'], pooling)
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - base
        outs = 4 * (B * D + B * L + (B * D if pooling == 'max' else 0))
        print(pooling, 'forward peak', peak, 'out + w + arg', outs)
        assert peak <= outs + mib
        w, arg = res[1], res[2]
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        grads = ops.hgn_gating_backward(d['S'], d['ug'], d['ui'], d['w1'], d['w3'], w, arg, d['g'], pooling)
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - base
        ws = recstudio_amd._native.lib().rsa_hgn_gating_workspace_bytes(B, L, D)
        outs = 4 * (B * L * D + B * D + B * L + D * D + D)
        print(pooling, 'backward peak', peak, 'outputs', outs, 'workspace', ws)
        assert peak <= outs + ws + mib
        del res, grads


def separated_case(B, L, D, allow):
    """An encoder-level case with one sequence padded whole in which, on the referee, the two largest si of every (b, c) among
    the real positions -- and the zero of the padded ones, where there are any -- differ by more than four tolerances: the first
    seed at which that holds."""
    for seed in range(8, 40):
        c = hr.make_case(B, L, D, pad='whole', seed=seed)
        k = hr.kernel_inputs(c)
        j = hr.judge_forward(k['S'], k['ug'], k['ui'], k['w1'], k['w3'], 'max', allow)
        real = (torch.arange(L).view(1, L) < c['lengths'].view(B, 1)).unsqueeze(2)
        first_pad = (torch.arange(L).view(1, L) == c['lengths'].view(B, 1)).unsqueeze(2)       # one zero stands for all of them
        si = j['si'].masked_fill(~(real | first_pad), float('-inf'))
        top = si.topk(min(2, L), dim=1)
        if L < 2:
            return c, k
        tol = j['e_si'].max(1).values
        gap = top.values[:, 0] - top.values[:, 1]
        if bool((gap > 4 * tol).all()):
            return c, k
    raise AssertionError('no seed separates the two largest si')


@pytest.mark.parametrize('cfg', [(37, 20, 64, 'mean'), (19, 50, 128, 'mean'), (23, 12, 64, 'max'), (7, 40, 32, 'max')], ids=str)
def test_autograd_node_against_the_twin(ops, cfg):
    """seqmodule.hgn_gating (the autograd node over the kernel) against hgn_gating_torch (the reference's op sequence) under
    autograd on the device: 1e-4 forward, 3e-4 on the gradients of S, ug, ui and both weights, with 3e-4 / 100 of a gradient's
    largest magnitude for the elements that cancel.  Max pooling: the case separates the two largest si of every (b, c) by more
    than four tolerances (asserted), and dS is compared at unpadded positions only -- which of several exactly tied padded rows
    receives g is torch's choice, and the gather's backward drops those rows anyway."""
    from recstudio_amd import seqmodule
    B, L, D, pooling = cfg
    allow = hr.sigmoid_allowance(DEV)
    if pooling == 'max':
        c, k = separated_case(B, L, D, allow)
        j = hr.judge_forward(k['S'], k['ug'], k['ui'], k['w1'], k['w3'], 'max', allow)
        real = (torch.arange(L).view(1, L) < c['lengths'].view(B, 1)).unsqueeze(2)
        first_pad = (torch.arange(L).view(1, L) == c['lengths'].view(B, 1)).unsqueeze(2)
        top = j['si'].masked_fill(~(real | first_pad), float('-inf')).topk(2, dim=1).values
        assert bool((top[:, 0] - top[:, 1] > 4 * j['e_si'].max(1).values).all())
    else:
        c = hr.make_case(B, L, D, pad='whole', seed=8)
        k = hr.kernel_inputs(c)
    names = ['S', 'ug', 'ui', 'w1', 'w3']
    res = {}
    calls = []
    real_apply = seqmodule._HgnGatingFn.apply
    seqmodule._HgnGatingFn.apply = staticmethod(lambda *a: (calls.append(1), real_apply(*a))[1])
    try:
        for which, fn in (('fused', seqmodule.hgn_gating), ('twin', seqmodule.hgn_gating_torch)):
            t = {n: k[n].to(DEV).requires_grad_(True) for n in names}
            out = fn(t['S'], t['ug'], t['ui'], t['w1'], t['w3'], pooling)
            grads = torch.autograd.grad((out * k['g'].to(DEV)).sum(), [t[n] for n in names])
            res[which] = (out.detach(), grads)
    finally:
        seqmodule._HgnGatingFn.apply = real_apply
    assert len(calls) == 1                                                  # the kernel ran for the fused arm, and only for it
    close = lambda x, y, rtol, atol: torch.testing.assert_close(x.double().cpu(), y.double().cpu(), rtol=rtol, atol=atol)   # noqa: E731
    close(res['fused'][0], res['twin'][0], 1e-4, 1e-5)
    unpadded = (torch.arange(L).view(1, L) < c['lengths'].view(B, 1)).view(B, L, 1).to(DEV)
    for n, x, y in zip(names, res['fused'][1], res['twin'][1]):
        assert x.shape == y.shape, n
        if n == 'S' and pooling == 'max':
            x, y = x * unpadded, y * unpadded
        close(x, y, 3e-4, 3e-6 * float(y.abs().max()))
