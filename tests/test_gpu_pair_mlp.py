"""GPU: ops.pair_mlp / ops.pair_mlp_backward (rsa_pairmlp.hip) against a float64 restatement of the scorers' formulas.

Inputs lie on a grid (embeddings k/16, W k/16, b1 odd/512, b2 odd/2^14, output weights k/4, b_out odd/2^17, p = 0.5 so 1/q = 2):
every sum of the forward is exact in fp32 in any order, so the scores must EQUAL the float64 referee and every ReLU decision of
the backward is the referee's.  Gradients are sums that are not exact: |got - ref| <= 3e-4 |ref| + 3e-6 max|ref| per tensor."""
import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 32, [32]), (5, 2, 32, [64, 32]), (8, 3, 64, [128, 64]), (11, 2, 64, [128, 64]), (31, 0, 64, [128, 64]),
          (300, 1, 64, [128, 64]), (7, 4, 128, [64, 32])]
N_ITEMS = 41


def grid_inputs(B, n, d, hidden, mode, seed=0):
    g = torch.Generator().manual_seed(seed)
    ri = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=g).double()      # noqa: E731
    odd = lambda *s: 2 * torch.randint(-8, 8, s, generator=g).double() + 1           # noqa: E731
    t = {'query': ri(-8, 8, B, d) / 16, 'table': ri(-8, 8, N_ITEMS, d) / 16,
         'w1': ri(-4, 4, hidden[0], 2 * d) / 16, 'b1': odd(hidden[0]) / 512, 'w2': None, 'b2': None}
    if len(hidden) > 1:
        t['w2'], t['b2'] = ri(-4, 4, hidden[1], hidden[0]) / 16, odd(hidden[1]) / 2 ** 14
    t['w_h'] = ri(-2, 2, hidden[-1]) / 4
    t['w_mf'] = ri(-2, 2, d) / 4 if mode == 'fusion' else None
    t['b_out'] = odd(1) / 2 ** 17 if mode == 'mlp' else None
    ids = torch.randint(1, N_ITEMS, (B, 1 + n), generator=g)
    ids[:, -1] = ids[:, 0] if n > 1 else ids[:, -1]          # repeated ids inside a query
    if n > 0:
        ids[0, -1] = 0                                       # id 0 among the negatives
    if B > 1:
        ids[1, 0] = 0                                        # a positive id of 0: scores -inf
    return t, ids


def referee(t, ids, p, u, mask_slot0=True, steps=None):
    """float64: the formulas of the issue, pair by pair.  ``steps``: asserts sum|terms| / grid step < 2^24 for every sum."""
    B, S = ids.shape
    d = t['query'].shape[1]
    q = float(torch.tensor(1.0 - p, dtype=torch.float32))
    at = 0

    def drop(h):
        nonlocal at
        if p == 0.0:
            return h
        keep = u[:, at:at + h.shape[1]].double() < q
        at += h.shape[1]
        return torch.where(keep, h / q, torch.zeros_like(h))

    def exact(x, w, b, step):
        if steps is not None:
            total = x.detach().abs() @ w.detach().abs().reshape(-1, x.shape[1]).t()
            total = total + (b.detach().abs() if b is not None else 0)
            assert float(total.max()) / step < 2 ** 24

    uq = t['query'].repeat_interleave(S, dim=0)
    x = t['table'][ids.reshape(-1)].clone().requires_grad_(t['query'].requires_grad)      # the per-slot item rows
    h = drop(torch.cat([uq, x], 1))
    layers = [(t['w1'], t['b1'], 2.0 ** -9)] + ([(t['w2'], t['b2'], 2.0 ** -14)] if t['w2'] is not None else [])
    for k, (w, b, step) in enumerate(layers):
        exact(h, w, b, step)
        pre = h @ w.t() + b
        assert float(pre.detach().abs().min()) >= 2.0 ** -14
        h = torch.relu(pre)
        if k + 1 < len(layers) or t['b_out'] is not None:
            h = drop(h)
    if t['w_mf'] is not None:
        exact(torch.cat([uq * x, h], 1), torch.cat([t['w_mf'], t['w_h']]), None, 2.0 ** -17)
        z = (uq * x) @ t['w_mf'] + h @ t['w_h']
    else:
        exact(h, t['w_h'], t['b_out'], 2.0 ** -17)
        z = h @ t['w_h'] + t['b_out']
    s = torch.relu(z).view(B, S)
    if mask_slot0:
        s = torch.where((ids == 0) & (torch.arange(S) == 0), torch.full_like(s, -float('inf')), s)
    return s, x


def close(got, ref):
    got, ref = got.detach().double().cpu(), ref.detach().double()
    bound = 3e-4 * ref.abs() + 3e-6 * ref.abs().max()
    return bool(((got - ref).abs() <= bound).all())


def on_gpu(t):
    return {k: None if v is None else v.float().cuda() for k, v in t.items()}


@pytest.mark.parametrize('mode', ['fusion', 'mlp'])
@pytest.mark.parametrize('p', [0.0, 0.5])
@pytest.mark.parametrize('B,n,d,hidden', SHAPES)
def test_pair_mlp_matches_referee(B, n, d, hidden, p, mode):
    from recstudio_amd import ops, rng
    t, ids = grid_inputs(B, n, d, hidden, mode)
    dv, idv = on_gpu(t), ids.cuda()
    M, C = ids.numel(), ops.pair_mlp_masked_columns(d, hidden, mode)
    gen = torch.cuda.default_generators[torch.cuda.current_device()]
    torch.manual_seed(1234)
    off0 = gen.get_offset()
    u = torch.rand(M, C, device='cuda').cpu() if p else None
    off1 = gen.get_offset()
    gen.set_offset(off0)
    philox = rng.reserve(M * C, 4, 'cuda') if p else None
    assert gen.get_offset() == off1                      # the state handed to the kernel is that call's, and as long
    table0 = dv['table'].clone()
    args = (dv['query'], dv['table'], idv, dv['w1'], dv['b1'], dv['w2'], dv['b2'], dv['w_h'])
    kw = dict({k: dv[k] for k in ('w_mf', 'b_out') if dv[k] is not None}, p=p, philox=philox, mask_slot0=True)
    got = ops.pair_mlp(*args, **kw)
    leaves = {k: v.clone().requires_grad_(True) for k, v in t.items() if v is not None and k != 'table'}
    ref, rows = referee(dict(t, **leaves), ids, p, u, steps=True)
    assert torch.equal(got.cpu(), ref.detach().float())
    assert torch.equal(got, ops.pair_mlp(*args, **kw)) and torch.equal(dv['table'], table0)
    up = torch.randn(B, 1 + n, generator=torch.Generator().manual_seed(5)).double()
    torch.where(torch.isinf(ref), torch.zeros_like(ref), ref).mul(up).sum().backward()
    dq, drows, grads = ops.pair_mlp_backward(*args, up.float().cuda(), **kw)
    dq2, drows2, grads2 = ops.pair_mlp_backward(*args, up.float().cuda(), **kw)
    assert torch.equal(dq, dq2) and torch.equal(drows, drows2) and all(torch.equal(grads[k], grads2[k]) for k in grads)
    assert close(dq, leaves['query'].grad)
    assert close(drows.view(M, d), rows.grad)
    assert sorted(grads) == sorted(k for k in leaves if k != 'query')
    for k in grads:
        assert close(grads[k], leaves[k].grad), k


def test_range_mode_equals_given_ids():
    from recstudio_amd import ops
    t, _ = grid_inputs(9, 1, 64, [128, 64], 'fusion')
    dv = on_gpu(t)
    c0, C = 3, 35
    ids = torch.arange(c0, c0 + C).repeat(9, 1).cuda()
    args = (dv['w1'], dv['b1'], dv['w2'], dv['b2'], dv['w_h'])
    given = ops.pair_mlp(dv['query'], dv['table'], ids, *args, w_mf=dv['w_mf'])
    ranged = ops.pair_mlp(dv['query'], dv['table'], None, *args, w_mf=dv['w_mf'], item_range=(c0, C))
    assert torch.equal(given, ranged) and float(given.max()) > 0


def test_table_ending_past_4_gib():
    """rows addressed with 64-bit offsets: the last rows of a 4.25 GiB table score what the same rows score in a small one"""
    from recstudio_amd import ops
    t, _ = grid_inputs(4, 1, 128, [64, 32], 'mlp')
    dv = on_gpu(t)
    n_rows = (17 << 28) // (128 * 4)                                   # 4.25 GiB of fp32 rows of 128
    big = torch.zeros(n_rows, 128, device='cuda')
    big[-N_ITEMS:] = dv['table']
    ids = torch.randint(1, N_ITEMS, (4, 3), generator=torch.Generator().manual_seed(3)).cuda()
    args = (dv['w1'], dv['b1'], dv['w2'], dv['b2'], dv['w_h'])
    small = ops.pair_mlp(dv['query'], dv['table'], ids, *args, b_out=dv['b_out'])
    assert torch.equal(ops.pair_mlp(dv['query'], big, ids + (n_rows - N_ITEMS), *args, b_out=dv['b_out']), small)


def test_forward_peak_memory_is_the_scores():
    from recstudio_amd import ops
    t, _ = grid_inputs(4096, 7, 64, [128, 64], 'fusion')               # M = 32768 pairs: [M, H1] would be 16 MiB
    dv = on_gpu(t)
    ids = torch.randint(1, N_ITEMS, (4096, 8), device='cuda')
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    s = ops.pair_mlp(dv['query'], dv['table'], ids, dv['w1'], dv['b1'], dv['w2'], dv['b2'], dv['w_h'], w_mf=dv['w_mf'])
    torch.cuda.synchronize()
    assert torch.cuda.max_memory_allocated() - base <= s.numel() * 4 + (1 << 20)
