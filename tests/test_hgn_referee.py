"""CPU: the float64 referee of HGN's gating (tests/hgn_referee.py) -- its backward formulas against autograd, an fp32 emulation of
the kernel's order inside half of every bound, and every seeded mistake outside a bound."""
import pytest
import torch

import hgn_referee as hr

SHAPES = [(1, 1, 32), (3, 9, 32), (2, 33, 64), (5, 50, 128)]
NAMES = ('dS', 'dug', 'dui', 'dw1', 'dw3')


@pytest.fixture(scope='module')
def allow():
    return hr.sigmoid_allowance('cpu')


@pytest.mark.parametrize('pooling', hr.POOLINGS)
@pytest.mark.parametrize('pad', hr.PADS, ids=str)
def test_backward_formulas_agree_with_autograd(pad, pooling):
    c = hr.make_case(4, 9, 32, pad=pad, seed=1)
    k = {n: hr.f64(v) for n, v in hr.kernel_inputs(c).items()}
    t = {n: k[n].clone().requires_grad_(True) for n in ('S', 'ug', 'ui', 'w1', 'w3')}
    B, L, d = t['S'].shape
    f = torch.sigmoid(t['S'] @ t['w1'].t() + t['ug'].view(B, 1, d))
    sf = t['S'] * f
    w = torch.sigmoid(sf @ t['w3'] + t['ui'])
    si = sf * w.unsqueeze(2)
    top = si.max(1)
    pooled = si.sum(1) / w.sum(1, keepdim=True) if pooling == 'mean' else top.values
    out = pooled + t['S'].sum(1)
    grads = torch.autograd.grad((out * k['g']).sum(), [t[n] for n in ('S', 'ug', 'ui', 'w1', 'w3')])
    # (autograd's own choice among the tied zeros of padded rows is handed over: the formulas are judged, not the tie-break)
    res = hr.backward(k['S'], k['ug'], k['ui'], k['w1'], k['w3'], pooling, k['g'], arg=top.indices if pooling == 'max' else None)
    for name, want in zip(NAMES, grads):
        assert float((res[name] - want).abs().max()) <= 1e-13 * max(1.0, float(want.abs().max())), name
    fwd = hr.judge_forward(k['S'], k['ug'], k['ui'], k['w1'], k['w3'], pooling, dict(sigmoid=0.0))
    assert float((fwd['out'] - out.detach()).abs().max()) <= 1e-13


@pytest.mark.parametrize('pooling', hr.POOLINGS)
@pytest.mark.parametrize('pad', hr.PADS, ids=str)
@pytest.mark.parametrize('shape', SHAPES, ids=str)
def test_fp32_emulation_inside_half_of_every_bound(allow, shape, pad, pooling):
    B, L, d = shape
    k = hr.kernel_inputs(hr.make_case(B, L, d, pad=pad, seed=2))
    out, w, arg, grads = hr.emulate_fp32(k['S'], k['ug'], k['ui'], k['w1'], k['w3'], pooling, k['g'])
    args = (k['S'], k['ug'], k['ui'], k['w1'], k['w3'], pooling)
    fwd = hr.judge_forward(*args, allow)
    bwd = hr.backward(*args, k['g'], arg=arg, allow=allow)
    ratios = dict(out=hr.worst_ratio(out, fwd['out'], fwd['tol_out']), w=hr.worst_ratio(w, fwd['w'], fwd['tol_w']))
    for name, got in zip(NAMES, grads):
        ratios[name] = hr.worst_ratio(got, bwd[name], bwd['tol_' + name])
    assert max(ratios.values()) <= 0.5, ratios
    if pooling == 'max':
        assert hr.arg_problems(fwd, arg).numel() == 0
        if pad == 'whole':
            assert not arg[B - 1].any()
    elif pad == 'whole':
        assert not out[B - 1].any()


def test_arg_judgement_catches_a_wrong_or_late_index(allow):
    k = hr.kernel_inputs(hr.make_case(3, 9, 32, pad='suffix', seed=2))
    fwd = hr.judge_forward(k['S'], k['ug'], k['ui'], k['w1'], k['w3'], 'max', allow)
    good = fwd['si'].max(1).indices
    assert hr.arg_problems(fwd, good).numel() == 0
    low = fwd['si'].min(1).indices                               # sequence 1 has no padding: its minimum is no maximum
    assert hr.arg_problems(fwd, low).numel() > 0
    # sequence 0 has one real position: wherever the zero of the padded rows wins, only the FIRST padded row (l = 1) is right
    late = good.clone()
    late[0][good[0] == 1] = 2
    assert (good[0] == 1).any() and hr.arg_problems(fwd, late).numel() > 0


@pytest.mark.parametrize('mistake', hr.FORWARD_MISTAKES)
def test_every_forward_mistake_leaves_a_bound(allow, mistake):
    pooling = 'max' if mistake == 'max_unpadded' else 'mean'
    c = hr.make_case(5, 9, 32, pad='suffix', seed=4)
    k = hr.kernel_inputs(c)
    fwd = hr.judge_forward(k['S'], k['ug'], k['ui'], k['w1'], k['w3'], pooling, allow)
    enc = (c['user'], c['S'], c['w1'], c['w2'], c['b_g'], c['w3'], c['w4'], c['b4'], c['lengths'], pooling)
    right, _ = hr.layer_rule(*enc)
    wrong, _ = hr.layer_rule(*enc, mistake=mistake)
    # the rule from the encoder's parameters is the rule from the kernel's inputs up to the fp32 rounding of ug and ui ...
    assert float((right - fwd['out']).abs().max()) <= 1e-5
    # ... and the mistake is far outside the bound
    assert float(((wrong - fwd['out']).abs() / fwd['tol_out']).max()) > 100.0
    if mistake == 'max_unpadded':
        real = torch.arange(9).view(1, 9, 1) < c['lengths'].view(5, 1, 1)
        assert bool((fwd['si'].masked_fill(~real, float('-inf')).max(1).values[0] < 0).any())   # all real si[c] negative somewhere


@pytest.mark.parametrize('mistake,pooling', [(m, p) for m in hr.BACKWARD_MISTAKES for p in hr.POOLINGS
                                             if (m, p) != ('no_pooled_term', 'max')])       # (max pooling has no such term)
def test_every_backward_mistake_leaves_a_bound(allow, mistake, pooling):
    k = hr.kernel_inputs(hr.make_case(5, 9, 32, pad='suffix', seed=4))
    args = (k['S'], k['ug'], k['ui'], k['w1'], k['w3'], pooling, k['g'])
    right = hr.backward(*args, allow=allow)
    wrong = hr.backward(*args, mistake=mistake)
    worst = max(float(((wrong[n] - right[n]).abs() / right['tol_' + n]).max()) for n in NAMES)
    assert worst > 100.0
