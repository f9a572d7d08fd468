"""CPU: the float64 referee of the user-history bag sum (tests/bag_referee.py) -- the torch twin against the rule, the rule's
backward against autograd, an fp32 emulation of the kernel pair's order inside half of every bound, and every seeded mistake
outside a bound."""
import pytest
import torch

import bag_referee as br
from recstudio_amd import seqmodule

SHAPES = [(1, 1, 4), (5, 9, 8), (3, 33, 200), (2, 300, 64), (2, 520, 260)]


@pytest.mark.parametrize('scale', br.SCALES)
@pytest.mark.parametrize('pad', br.PADS, ids=str)
def test_twin_agrees_with_the_rule_in_float64(pad, scale):
    c = br.make_case(5, 9, 8, pad=pad, seed=1, common=True)
    w = c['table'].to(br.F64).requires_grad_(True)
    got = seqmodule.bag_pool(w, c['ids'], scale)
    want = br.forward(c['table'], c['ids'], scale)
    live = ~want['out'].isnan()
    assert bool((got.isnan() == ~live).all())
    assert float((got.detach() - want['out'])[live].abs().max()) <= 1e-12
    rows = (c['ids'] != 0).any(1)
    (got[rows] * c['g'].to(br.F64)[rows]).sum().backward()
    ids = c['ids'] * rows.unsqueeze(1)
    bwd = br.backward(ids[rows], c['g'][rows], scale)
    assert float((w.grad[1:] - br.dense(bwd, w.shape[0])[1:]).abs().max()) <= 1e-12
    assert bwd['items'].min() >= 1


def test_twin_reads_row_zero_and_the_rule_does_not():
    c = br.make_case(4, 6, 8, pad='suffix', seed=3, row0=True)
    twin = seqmodule.bag_pool_torch(c['table'].to(br.F64), c['ids'], 'sum')
    n_pad = (c['ids'] == 0).sum(1, keepdim=True).to(br.F64)
    want = br.forward(c['table'], c['ids'], 'sum')['out']
    assert float((twin - n_pad * c['table'][0].to(br.F64) - want).abs().max()) <= 1e-12


@pytest.mark.parametrize('scale', br.SCALES)
@pytest.mark.parametrize('pad', br.PADS, ids=str)
@pytest.mark.parametrize('shape', SHAPES, ids=str)
def test_fp32_emulation_inside_half_of_every_bound(shape, pad, scale):
    B, L, d = shape
    c = br.make_case(B, L, d, N=41, pad=pad, seed=2, row0=True, common=True)
    out, cnt, dW = br.emulate_fp32(c['table'], c['ids'], scale, c['g'])
    fwd = br.forward(c['table'], c['ids'], scale)
    bwd = br.backward(c['ids'], c['g'], scale)
    assert torch.equal(cnt.to(torch.int64), fwd['cnt'])
    assert br.worst_ratio(out, fwd['out'], fwd['tol']) <= 0.5
    assert br.worst_ratio(dW[bwd['items']], bwd['dW'], bwd['tol']) <= 0.5
    assert int(dW.count_nonzero()) == int(dW[bwd['items']].count_nonzero())


@pytest.mark.parametrize('mistake', br.MISTAKES)
def test_every_seeded_mistake_leaves_a_bound(mistake):
    scale = 'mean' if mistake in ('scale_twice', 'cnt_pad_bwd') else 'rsqrt'
    c = br.make_case(5, 9, 8, pad='suffix', seed=4, row0=True, common=True)
    N = c['table'].shape[0]
    if mistake in br.FORWARD_MISTAKES:
        want, bad = br.forward(c['table'], c['ids'], scale), br.forward(c['table'], c['ids'], scale, mistake)
        ratio = br.worst_ratio(bad['out'], want['out'], want['tol'])
        assert ratio > 1 or not torch.equal(bad['cnt'], want['cnt'])
        if mistake != 'cnt_pad':
            assert ratio > 1
    else:
        want, bad = br.backward(c['ids'], c['g'], scale), br.backward(c['ids'], c['g'], scale, mistake)
        tol = torch.zeros(N, c['g'].shape[1], dtype=br.F64)
        tol[want['items']] = want['tol']
        assert br.worst_ratio(br.dense(bad, N), br.dense(want, N), tol) > 1


def test_worst_ratio_demands_exact_zeros_and_nans():
    want = torch.tensor([[0.0, float('nan')]], dtype=br.F64)
    tol = torch.zeros(1, 2, dtype=br.F64)
    assert br.worst_ratio(torch.tensor([[0.0, float('nan')]]), want, tol) == 0.0
    assert br.worst_ratio(torch.tensor([[1e-30, float('nan')]]), want, tol) == float('inf')
    assert br.worst_ratio(torch.tensor([[0.0, 0.0]]), want, tol) == float('inf')
