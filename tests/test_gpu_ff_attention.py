"""GPU: ops.ff_attention_pool / ops.ff_attention_pool_backward (rsa_ffattn.hip) against the float64 referee
(tests/ff_attention_referee.py): every element of out, a, dkey, dqh, dW_k, dw2 and db2 inside its bound at the tile edges (S = 31,
32, 33), with a sequence across several tiles (S = 50, 70), several sequences in one tile (S = 1, 9, 20), D != M both ways and more
than one workgroup (B = 300), under no mask, a right-padded suffix, scattered holes and one sequence padded whole -- the keys are
non-zero at the padded positions, and W_k is always a column block of a wider matrix whose other columns are NaN.
Worst shares of the bounds over the 36 cases, as printed by test_every_element_within_its_bound on the MI355X:
    out 0.005   a 0.008   dkey 0.009   dqh 0.018   dW_k 0.021   dw2 0.022   db2 0.012
with the device's own fp32 sigmoid measuring 1.5 u against float64 (allowance 3.0 u).  The shares are small because the
(n + 2) u sum |terms| rule charges every rounding of a sum with one sign; the seeded mistakes of tests/test_ff_attention_referee.py
still leave these bounds by orders of magnitude.  The case past 4 GiB: out 0.001, a 0.003, dkey 0.003, dqh 0.0001.
"""
import pytest
import torch

import ff_attention_referee as fr

pytestmark = pytest.mark.gpu

DEV = 'cuda'
SHAPES = [(1, 1, 32, 32), (3, 9, 32, 64), (2, 31, 64, 64), (2, 32, 64, 64), (2, 33, 64, 64), (3, 20, 64, 128), (5, 50, 128, 128),
          (2, 70, 128, 128), (300, 20, 64, 64)]
NAMES = ('dkey', 'dqh', 'dw_k', 'dw2', 'db2')
WORST = {}


@pytest.fixture(scope='module')
def ops():
    import recstudio_amd
    recstudio_amd._native.lib()
    torch.cuda.init()
    return recstudio_amd.ops


def device_inputs(k):
    """The kernel's inputs on the device; w_k as columns [q, q + D) of a wider matrix whose first q = 8 columns are NaN."""
    M, D = k['w_k'].shape
    wide = torch.full((M, 8 + D), float('nan'))
    wide[:, 8:] = k['w_k']
    wide = wide.to(DEV)
    pad = None if k['key_pad'] is None else k['key_pad'].to(DEV)
    return dict(key=k['key'].to(DEV), qh=k['qh'].to(DEV), w_k=wide[:, 8:], w2=k['w2'].to(DEV), b2=k['b2'].to(DEV), key_pad=pad,
                g=k['g'].to(DEV), wide=wide)


def run(ops, d, scale):
    out, a = ops.ff_attention_pool(d['key'], d['qh'], d['w_k'], d['w2'], d['b2'], d['key_pad'], scale=scale)
    grads = ops.ff_attention_pool_backward(d['key'], d['qh'], d['w_k'], d['w2'], d['b2'], d['key_pad'], d['g'], scale=scale)
    return out, a, grads


@pytest.mark.parametrize('pad', fr.PADS, ids=str)
@pytest.mark.parametrize('shape', SHAPES, ids=str)
def test_every_element_within_its_bound(ops, shape, pad):
    """Measured on the MI355X: the worst shares of the bounds are in the module docstring."""
    B, S, D, M = shape
    c = fr.make_case(B, S, D, M, q_dim=D, bias=True, pad=pad, seed=3)
    k = fr.kernel_inputs(c)
    d = device_inputs(k)
    assert d['w_k'].stride(0) == D + 8 and d['w_k'].data_ptr() == d['wide'].data_ptr() + 32      # read in place: no copy
    out, a, grads = run(ops, d, k['scale'])
    out2, a2, grads2 = run(ops, d, k['scale'])
    torch.cuda.synchronize()
    pre = k['qh'].view(B, 1, M) + k['key'] @ k['w_k'].t()
    allow = fr.sigmoid_allowance(DEV, pre)
    args = (k['key'], k['qh'], k['w_k'], k['w2'], k['b2'], k['key_pad'], k['scale'])
    fwd = fr.judge_forward(*args, allow)
    bwd = fr.backward(*args, k['g'], allow)
    ratios = dict(out=fr.worst_ratio(out, fwd['out'], fwd['tol_out']), a=fr.worst_ratio(a, fwd['a'], fwd['tol_a']))
    for name, got in zip(NAMES, grads):
        assert got.shape == bwd[name].shape, name
        ratios[name] = fr.worst_ratio(got, bwd[name], bwd['tol_' + name])
    for n, v in ratios.items():
        WORST[n] = max(WORST.get(n, 0.0), v)
    print(shape, pad, {n: round(v, 3) for n, v in ratios.items()}, 'worst so far', {n: round(v, 3) for n, v in WORST.items()}, allow)
    for t in (out, a) + tuple(grads):
        assert not torch.isnan(t).any()                                    # nothing of the NaN columns next to W_k leaks
    assert max(ratios.values()) <= 1.0, ratios
    # two runs are bit-equal
    for x, y in zip((out, a) + tuple(grads), (out2, a2) + tuple(grads2)):
        assert torch.equal(x, y)
    # padded positions are exactly +0 (the sign bit too), a sequence padded whole is exactly 0
    if k['key_pad'] is not None:
        padd = d['key_pad']
        assert padd.any() or S == 1
        assert not a[padd].view(torch.int32).any() and not grads[0][padd].view(torch.int32).any()
    if pad == 'whole':
        assert not out[B - 1].any() and not grads[1][B - 1].any() and not grads[0][B - 1].any()
    assert torch.isnan(d['wide'][:, :8]).all()


def test_b_zero_launches_nothing(ops):
    z = lambda *s: torch.zeros(*s, device=DEV)         # noqa: E731
    out, a = ops.ff_attention_pool(z(0, 5, 32), z(0, 64), z(64, 32), z(64), z(1), None, scale=0.1)
    assert out.shape == (0, 32) and a.shape == (0, 5)
    dkey, dqh, dw, dw2, db2 = ops.ff_attention_pool_backward(z(0, 5, 32), z(0, 64), z(64, 32), z(64), z(1), None, z(0, 32), scale=0.1)
    assert dkey.shape == (0, 5, 32) and dqh.shape == (0, 64) and not dw.any() and not dw2.any() and not db2.any()
    with pytest.raises(ValueError):
        ops.ff_attention_pool(z(2, 5, 48), z(2, 64), z(64, 48), z(64), z(1), None, scale=0.1)


def test_offsets_past_four_gib(ops):
    """key and dkey of B = 16448, S = 512, D = 128 (M = 32) end past byte offset 4 GiB: the last two sequences, which lie there,
    are judged against the referee of those sequences alone (out, a, dkey, dqh are per-sequence)."""
    B, S, D, M, T = 16448, 512, 128, 32, 2
    assert B * S * D * 4 > 1 << 32 and (B - T) * S * D * 4 > 1 << 32
    gen = torch.Generator(device=DEV).manual_seed(9)
    key = torch.randn(B, S, D, device=DEV, generator=gen)
    qh = torch.randn(B, M, device=DEV, generator=gen)
    g = torch.randn(B, D, device=DEV, generator=gen)
    w_k = (torch.rand(M, D, device=DEV, generator=gen) * 2 - 1) * 0.15
    w2 = (torch.rand(M, device=DEV, generator=gen) * 2 - 1) * 0.3
    b2 = torch.tensor([0.37], device=DEV)
    pad = torch.rand(B, S, device=DEV, generator=gen) < 0.2
    scale = fr.fp32_scale(128)
    out, a = ops.ff_attention_pool(key, qh, w_k, w2, b2, pad, scale=scale)
    dkey, dqh, dw_k, dw2, db2 = ops.ff_attention_pool_backward(key, qh, w_k, w2, b2, pad, g, scale=scale)
    torch.cuda.synchronize()
    tail = [t[B - T:].cpu() for t in (key, qh, pad, g)]
    allow = fr.sigmoid_allowance(DEV, tail[1].view(T, 1, M) + tail[0] @ w_k.cpu().t())
    args = (tail[0], tail[1], w_k.cpu(), w2.cpu(), b2.cpu(), tail[2], scale)
    fwd = fr.judge_forward(*args, allow)
    bwd = fr.backward(*args, tail[3], allow)
    ratios = dict(out=fr.worst_ratio(out[B - T:], fwd['out'], fwd['tol_out']), a=fr.worst_ratio(a[B - T:], fwd['a'], fwd['tol_a']),
                  dkey=fr.worst_ratio(dkey[B - T:], bwd['dkey'], bwd['tol_dkey']),
                  dqh=fr.worst_ratio(dqh[B - T:], bwd['dqh'], bwd['tol_dqh']))
    print(ratios)
    assert max(ratios.values()) <= 1.0, ratios
    assert not torch.isnan(dw_k).any() and not torch.isnan(dw2).any() and not torch.isnan(db2).any()
    assert not dkey[B - T:][pad[B - T:]].any()


def test_peak_memory(ops):
    """At B = 1024, S = 32, D = 64, M = 128 the hidden layer [B, S, M] would be 16 MiB.  The forward's peak above its inputs is at
    most out + a + 1 MiB; the backward's at most its outputs + the workspace + 1 MiB."""
    import recstudio_amd
    B, S, D, M = 1024, 32, 64, 128
    assert B * S * M * 4 == 16 << 20
    c = fr.make_case(B, S, D, M, q_dim=D, bias=False, pad='suffix', seed=5)
    k = fr.kernel_inputs(c)
    d = device_inputs(k)
    run(ops, d, k['scale'])                                                 # (the LDS grant and the library load are behind us)
    torch.cuda.synchronize()
    mib = 1 << 20
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    res = ops.ff_attention_pool(d['key'], d['qh'], d['w_k'], d['w2'], d['b2'], d['key_pad'], scale=k['scale'])
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    print('forward peak', peak, 'out + a', 4 * (B * D + B * S))
    assert peak <= 4 * (B * D + B * S) + mib
    del res
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    res = ops.ff_attention_pool_backward(d['key'], d['qh'], d['w_k'], d['w2'], d['b2'], d['key_pad'], d['g'], scale=k['scale'])
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    ws = recstudio_amd._native.lib().rsa_ff_attention_workspace_bytes(B, S, D, M)
    outs = 4 * (B * S * D + B * M + M * D + M + 1)
    print('backward peak', peak, 'outputs', outs, 'workspace', ws)
    assert peak <= outs + ws + mib


@pytest.mark.parametrize('cfg', [(37, 20, 64, 64, 128, True), (19, 50, 128, 128, 128, False)], ids=['stamp', 'narm'])
def test_autograd_node_against_the_twin(ops, cfg):
    """seqmodule.ff_attention_pool (the autograd node over the kernel) against ff_attention_pool_torch (the reference's op
    sequence) under autograd on the device: 1e-4 forward, 3e-4 on the gradients of the query, the keys and every parameter, with
    3e-4 / 100 of a gradient's largest magnitude for the elements that cancel."""
    from recstudio_amd import seqmodule
    B, S, D, M, q_dim, bias = cfg
    c = fr.make_case(B, S, D, M, q_dim=q_dim, bias=bias, pad='whole', seed=8)
    names = ['query', 'key', 'w1', 'w2', 'b2'] + (['b1'] if bias else [])
    res = {}
    calls = []
    real = seqmodule._FfAttentionFn.apply
    seqmodule._FfAttentionFn.apply = staticmethod(lambda *a: (calls.append(1), real(*a))[1])
    try:
        for which, fn in (('fused', seqmodule.ff_attention_pool), ('twin', seqmodule.ff_attention_pool_torch)):
            t = {n: (c[n].to(DEV).requires_grad_(True) if n in names else (None if c[n] is None else c[n].to(DEV))) for n in c}
            out, a = fn(t['query'], t['key'], t['w1'], t['b1'], t['w2'], t['b2'], t['key_pad'])
            grads = torch.autograd.grad((out * t['g']).sum(), [t[n] for n in names])
            res[which] = (out.detach(), a.detach(), grads)
    finally:
        seqmodule._FfAttentionFn.apply = real
    assert len(calls) == 1                                                  # the kernel ran for the fused arm, and only for it
    close = lambda x, y, rtol, atol: torch.testing.assert_close(x.double().cpu(), y.double().cpu(), rtol=rtol, atol=atol)   # noqa: E731
    close(res['fused'][0], res['twin'][0], 1e-4, 1e-5)
    close(res['fused'][1], res['twin'][1], 1e-4, 1e-6)
    for n, x, y in zip(names, res['fused'][2], res['twin'][2]):
        assert x.shape == y.shape, n
        close(x, y, 3e-4, 3e-6 * float(y.abs().max()))
