"""GPU: ops.bag_pool / ops.bag_pool_backward (rsa_bag.hip) against the float64 referee (tests/bag_referee.py): every element of
out, cnt and dW inside its bound for d = 4 .. 1024 (1, 16, 50, 64, 65, 150 and 256 16-byte columns), L = 1 .. 300 and the lengths
either side of the long-bag switch (256 | 257: one launch | chunks of 256 positions merged by a second; 512 | 513: two | three
chunks), B = 1, 5 and 300, under no padding, a right-padded mix, interior zeros and one bag padded whole, for the three scales.
Every case has a table whose row 0 is not zero, an item repeated inside bag 0, item 1 in every bag, and ids read in place from a
wider buffer filled with an out-of-range id.  Two runs are bit-equal, and so is the same bag one position further down a batch
that is 7 columns wider (which crosses the switch at L = 256).
Worst shares of the bounds, as printed by test_every_element_within_its_bound on the MI355X:
    out 0.405   dW 0.557        (the case past 4 GiB: out 0.189, dW 0.417)
dW comes closest where an item occurs once or twice: its bound is then 4 or 5 u of one or two products, of which the rounding of
s_b, the product and one addition can use up to 3.
"""
import pytest
import torch

import bag_referee as br

pytestmark = pytest.mark.gpu

DEV = 'cuda'
SHAPES = [(1, 1, 4), (5, 2, 64), (5, 9, 200), (300, 33, 256), (5, 70, 260), (300, 70, 600), (5, 300, 1024), (1, 300, 600),
          (300, 300, 64), (5, 256, 200), (5, 257, 200), (5, 512, 600), (5, 513, 600), (1, 9, 1024)]
WORST = {}
BIG_ID = 1 << 40


@pytest.fixture(scope='module')
def ops():
    import recstudio_amd
    recstudio_amd._native.lib()
    torch.cuda.init()
    return recstudio_amd.ops


def strided_ids(ids):
    """``ids`` on the device as rows [1, 1 + B), columns [3, 3 + L) of a wider buffer filled with an out-of-range id."""
    B, L = ids.shape
    wide = torch.full((B + 2, L + 5), BIG_ID, dtype=torch.int64, device=DEV)
    wide[1:1 + B, 3:3 + L] = ids.to(DEV)
    return wide[1:1 + B, 3:3 + L]


def bits(t):
    return t.view(torch.int32)


def judge(table, ids, g, scale, out, cnt, dW):
    fwd, bwd = br.forward(table, ids, scale), br.backward(ids, g, scale)
    assert torch.equal(cnt.cpu().to(torch.int64), fwd['cnt'])
    ratios = dict(out=br.worst_ratio(out, fwd['out'], fwd['tol']), dW=br.worst_ratio(dW[bwd['items'].to(DEV)], bwd['dW'], bwd['tol']))
    assert int(dW.count_nonzero()) == int(dW[bwd['items'].to(DEV)].count_nonzero())      # no other row is written (row 0 among them)
    return fwd, ratios


@pytest.mark.parametrize('pad', br.PADS, ids=str)
@pytest.mark.parametrize('shape', SHAPES, ids=str)
def test_every_element_within_its_bound(ops, shape, pad):
    """Measured on the MI355X: the worst shares of the bounds are in the module docstring."""
    B, L, d = shape
    N = 23 if B * L < 500 else 997
    c = br.make_case(B, L, d, N, pad=pad, seed=5, row0=True, common=True)
    table, g, ids = c['table'].to(DEV), c['g'].to(DEV), strided_ids(c['ids'])
    assert L == 1 or ids.stride(0) == L + 5                       # read in place
    wider = torch.cat([c['ids'].roll(1, 0), torch.zeros(B, 7, dtype=torch.int64)], 1).to(DEV)
    for scale in br.SCALES:
        out, cnt = ops.bag_pool(table, ids, scale)
        dW = ops.bag_pool_backward(ids, cnt, g, N, scale)
        out2, cnt2 = ops.bag_pool(table, ids, scale)
        dW2 = ops.bag_pool_backward(ids, cnt2, g, N, scale)
        out3, cnt3 = ops.bag_pool(table, wider, scale)
        torch.cuda.synchronize()
        fwd, ratios = judge(c['table'], c['ids'], c['g'], scale, out, cnt, dW)
        for n, v in ratios.items():
            WORST[n] = max(WORST.get(n, 0.0), v)
        print(shape, pad, scale, {n: round(v, 3) for n, v in ratios.items()}, 'worst so far', {n: round(v, 3) for n, v in WORST.items()})
        assert max(ratios.values()) <= 1.0, ratios
        assert torch.equal(bits(out), bits(out2)) and torch.equal(cnt, cnt2) and torch.equal(bits(dW), bits(dW2))
        assert torch.equal(bits(out3), bits(out.roll(1, 0))) and torch.equal(cnt3, cnt.roll(1, 0))
        if pad == 'whole':
            empty = fwd['cnt'] == 0
            assert int(empty.sum()) == 1 and bool(empty[B - 1])
            row_nan = out.isnan().all(1).cpu()
            assert torch.equal(row_nan, empty if scale != 'sum' else torch.zeros_like(empty))
            assert scale != 'sum' or not bool(out[B - 1].any())
            assert not bool(dW.isnan().any())                 # no gradient from the empty bag


def test_table_past_4_gib(ops):
    """64-bit offsets: a [1 100 000, 1024] table (4.5 GB), allocated uninitialised, with only the referenced rows written -- some of
    them the top rows."""
    N, d, B, L = 1_100_000, 1024, 5, 9
    gen = torch.Generator().manual_seed(7)
    pool = torch.tensor([1, 2, 77, 524_288, 1_048_575, 1_048_576, 1_048_577, N - 3, N - 2, N - 1])
    ids = pool[torch.randint(0, pool.numel(), (B, L), generator=gen)]
    ids[1, 1:] = 0
    ids[2, 3] = 0
    table = torch.empty(N, d, device=DEV)
    table[pool.to(DEV)] = torch.randn(pool.numel(), d, generator=gen).to(DEV)
    g = torch.randn(B, d, generator=gen).to(DEV)
    for scale in ('rsqrt', 'mean'):
        out, cnt = ops.bag_pool(table, ids.to(DEV), scale)
        dW = ops.bag_pool_backward(ids.to(DEV), cnt, g, N, scale)
        torch.cuda.synchronize()
        _, ratios = judge(table, ids, g, scale, out, cnt, dW)
        print('past 4 GiB', scale, {n: round(v, 3) for n, v in ratios.items()})
        assert max(ratios.values()) <= 1.0, ratios
        del dW


def test_refusals(ops):
    ids = torch.tensor([[1, 2, 0]], device=DEV)
    for d in (6, 1028):
        with pytest.raises(ValueError, match='multiple of 4'):
            ops.bag_pool(torch.zeros(5, d, device=DEV), ids)
        with pytest.raises(ValueError, match='multiple of 4'):
            ops.bag_pool_backward(ids, torch.ones(1, dtype=torch.int32, device=DEV), torch.zeros(1, d, device=DEV), 5)
    with pytest.raises(RuntimeError, match='GPU only'):
        ops.bag_pool(torch.zeros(5, 8), ids.cpu())
    with pytest.raises(RuntimeError, match='GPU only'):
        ops.bag_pool(torch.zeros(5, 8, device=DEV), ids.cpu())
    with pytest.raises(TypeError, match='int64'):
        ops.bag_pool(torch.zeros(5, 8, device=DEV), ids.int())
    with pytest.raises(ValueError, match='scale'):
        ops.bag_pool(torch.zeros(5, 8, device=DEV), ids, 'max')


def test_autograd_node_matches_the_twin(ops):
    from recstudio_amd import seqmodule
    c = br.make_case(5, 9, 200, pad='suffix', seed=9)
    ids = c['ids'].to(DEV)
    for scale in br.SCALES:
        w = c['table'].to(DEV).requires_grad_(True)
        out = seqmodule.bag_pool(w, ids, scale)
        (out * c['g'].to(DEV)).sum().backward()
        w2 = c['table'].to(DEV).requires_grad_(True)
        out_t = seqmodule.bag_pool(w2, ids, scale, fused=False)
        (out_t * c['g'].to(DEV)).sum().backward()
        # both are fp32 sums of the same terms in some order: each inside the referee's bound, so at most two bounds apart
        fwd, bwd = br.forward(c['table'], c['ids'], scale), br.backward(c['ids'], c['g'], scale)
        assert bool(((out - out_t).detach().cpu().to(br.F64).abs() <= 2 * fwd['tol']).all())
        assert not bool(w.grad[0].any())
        diff = (w.grad - w2.grad).cpu().to(br.F64).abs()
        assert bool((diff[bwd['items']] <= 2 * bwd['tol']).all()) and int(diff.count_nonzero()) == int(diff[bwd['items']].count_nonzero())
