"""GPU: rsa_bi_combine / rsa_bi_combine_backward (ops.bi_combine, ops.bi_combine_backward, graphmodule.BiCombiner) against the
float64 layer of tests/ngcf_referee.py, every element inside the bounds its header derives."""
import functools

import pytest
import torch

import ngcf_referee as nr

pytestmark = pytest.mark.gpu

DEV = 'cuda'
SLOPE = 0.01
PARAMS = ('x', 'm', 'w1', 'b1', 'w2', 'b2')
SHAPES = [(4, 4), (36, 20), (64, 64), (64, 32), (32, 64), (128, 128)]
SIZES = [1, 31, 32, 33, 257, 1000]            # 1000 = 7 workgroups of 128 rows and a last one of 104 (3 full waves and one of 8 rows)
PS = [0.0, 0.1, 0.5]


@pytest.fixture(scope='module')
def ra():
    import recstudio_amd
    return recstudio_amd


@functools.lru_cache(maxsize=None)
def inputs(N, d_in, d_out):
    """CPU inputs of one shape, shared by the tests below and never written to."""
    return nr.layer_inputs(N, d_in, d_out, seed=1000 * d_in + d_out + N)


def on_gpu(inp):
    return [inp[k].to(DEV) for k in ('x', 'm', 'w1', 'w2', 'b1', 'b2')]


def reserve(ra, N, d_out, p, gen):
    return ra.rng.reserve(N * d_out, 4, torch.device(DEV), gen) if p else None


def generator(seed, burn=0):
    gen = torch.Generator(device=DEV)
    gen.manual_seed(seed)
    if burn:
        torch.rand(burn, device=DEV, generator=gen)
    return gen


@pytest.mark.parametrize('d_in,d_out', SHAPES)
def test_forward_within_the_bound(ra, d_in, d_out):
    ops = ra.ops
    for N in SIZES:
        inp = inputs(N, d_in, d_out)
        dev = on_gpu(inp)
        args = [inp[k] for k in PARAMS]
        for p in PS:
            gen, twin = generator(5, burn=3), generator(5, burn=3)
            state = gen.get_offset()
            wide = torch.full((N, d_out + 12), 7.5, device=DEV)
            h = ops.bi_combine(*dev, negative_slope=SLOPE, p=p, philox=reserve(ra, N, d_out, p, gen), out=wide, col=8)
            u = torch.rand(N, d_out, device=DEV, generator=twin)
            if p:
                assert gen.get_offset() == twin.get_offset()
                # (no sum of two activations is exactly 0 on these inputs: an element is 0 exactly where it was dropped)
                assert torch.equal(h != 0, u < torch.tensor(1.0 - p, dtype=torch.float32, device=DEV))
                f = nr.layer_forward(*args, SLOPE, p, u.cpu())
            else:
                assert gen.get_offset() == state                      # p = 0 draws nothing
                f = nr.layer_forward(*args, SLOPE)
            fb = nr.layer_forward_bounds(*args, f)
            wh, wn = nr.worst(h, f['h'], fb['h']), nr.worst(wide[:, 8:8 + d_out], f['n'], fb['n'])
            print(f'forward {d_in}x{d_out} N={N} p={p}: worst error / bound  h {wh:.3f}  n {wn:.3f}')
            assert wh <= 1 and wn <= 1
            assert bool((wide[:, :8] == 7.5).all()) and bool((wide[:, 8 + d_out:] == 7.5).all())      # the neighbours bit-unchanged
            # every nullable output, and a second run
            gen2 = generator(5, burn=3)
            h_only = ops.bi_combine(*dev, negative_slope=SLOPE, p=p, philox=reserve(ra, N, d_out, p, gen2))
            gen3 = generator(5, burn=3)
            wide2 = torch.full((N, d_out + 12), 7.5, device=DEV)
            assert ops.bi_combine(*dev, negative_slope=SLOPE, p=p, philox=reserve(ra, N, d_out, p, gen3), want_h=False, out=wide2, col=8) is None
            assert torch.equal(h_only, h) and torch.equal(wide2, wide)


def test_mask_is_torch_rand_past_the_first_philox_round(ra):
    """N * d_out above grid_threads * 4: elements of the second and third round of the torch.rand call."""
    N, d_in, d_out, p = 32769, 64, 128, 0.1
    gen_in = torch.Generator(device=DEV).manual_seed(1)
    x, m = (torch.rand(N, d_in, device=DEV, generator=gen_in) + 0.5 for _ in range(2))
    w = torch.full((d_out, d_in), 0.01, device=DEV)            # every pre-activation positive: h != 0 exactly where kept
    b = torch.full((d_out,), 0.1, device=DEV)
    gen, twin = generator(9, burn=1000), generator(9, burn=1000)
    pc = reserve(ra, N, d_out, p, gen)
    assert N * d_out > 2 * 4 * pc.grid_threads
    h = ra.ops.bi_combine(x, m, w, w, b, b, negative_slope=SLOPE, p=p, philox=pc)
    u = torch.rand(N, d_out, device=DEV, generator=twin)
    assert torch.equal(h != 0, u < torch.tensor(1.0 - p, dtype=torch.float32, device=DEV))
    assert gen.get_offset() == twin.get_offset()


def test_forward_past_4_gib(ra):
    """x, m and h past byte offset 4 GiB (N = 2**24 + 33 at d = 64); the referee runs on the first and the last 1024 rows.
    torch.rand itself splits a tensor of this size (4 GiB) into several calls with states of their own, so its result is not
    the uniforms of ONE call (the bit-equality with torch.rand is checked below that size, above); the uniforms here come from the
    other kernel that draws the elements of one call with a 64-bit index, the SimGCL noise of ops.spmm_csr (noise_out) on a
    graph without edges."""
    ops = ra.ops
    N, d, p = (1 << 24) + 33, 64, 0.1
    gen_in = torch.Generator(device=DEV).manual_seed(2)
    x = torch.rand(N, d, device=DEV, generator=gen_in) * 2 - 1
    m = torch.rand(N, d, device=DEV, generator=gen_in) * 2 - 1
    small = inputs(33, d, d)
    w1, w2, b1, b2 = (small[k].to(DEV) for k in ('w1', 'w2', 'b1', 'b2'))
    pc = reserve(ra, N, d, p, generator(4))
    wide = torch.empty(N, d, device=DEV)
    h = ops.bi_combine(x, m, w1, w2, b1, b2, negative_slope=SLOPE, p=p, philox=pc, out=wide)
    indptr = torch.zeros(N + 1, dtype=torch.int64, device=DEV)
    u = torch.empty(N, d, device=DEV)
    ops.spmm_csr(indptr, torch.empty(0, dtype=torch.int32, device=DEV), None, torch.zeros(1, d, device=DEV),
                 plan=ops.spmm_plan(indptr), noise=pc, noise_eps=1.0, noise_out=u)
    for rows in (slice(0, 1024), slice(N - 1024, N)):
        args = [x[rows].cpu(), m[rows].cpu(), small['w1'], small['b1'], small['w2'], small['b2']]
        f = nr.layer_forward(*args, SLOPE, p, u[rows].cpu())
        fb = nr.layer_forward_bounds(*args, f)
        wh, wn = nr.worst(h[rows], f['h'], fb['h']), nr.worst(wide[rows], f['n'], fb['n'])
        print(f'forward past 4 GiB rows {rows.start}..: worst error / bound  h {wh:.3f}  n {wn:.3f}')
        assert wh <= 1 and wn <= 1


# every shape at every N of the forward list up to 257 (a lone row, a tile one short, full and one over, several workgroups) and at
# 4099, where the dW reduction spans several workgroups
BACKWARD = [(d_in, d_out, N) for d_in, d_out in SHAPES for N in (1, 31, 32, 33, 257, 4099)]


@pytest.mark.parametrize('d_in,d_out,N', BACKWARD)
def test_backward_within_the_bound(ra, d_in, d_out, N):
    ops = ra.ops
    inp = inputs(N, d_in, d_out)
    dev = on_gpu(inp)
    args = [inp[k] for k in PARAMS]
    names = ('dx', 'dm', 'dw1', 'dw2', 'db1', 'db2')
    for p in (0.0, 0.1):
        for use_h, use_n in ((True, True), (True, False), (False, True)):
            g_h = inp['g_h'] if use_h else None
            g_n = inp['g_n'] if use_n else None
            g_wide = None
            if use_n:
                g_wide = torch.full((N, d_out + 8), float('nan'), device=DEV)          # (the other columns are never read)
                g_wide[:, 4:4 + d_out] = g_n.to(DEV)
            gen, twin = generator(6), generator(6)
            pc = reserve(ra, N, d_out, p, gen)
            u = torch.rand(N, d_out, device=DEV, generator=twin).cpu()
            f = nr.layer_forward(*args, SLOPE, p, u)
            fb = nr.layer_forward_bounds(*args, f)
            assert nr.preact_margin(f, fb) >= 2                    # a condition on the inputs: every slope is decided
            b = nr.layer_backward(*args, f, g_h, g_n, SLOPE)
            bb = nr.layer_backward_bounds(*args, f, fb, b, g_h, g_n, SLOPE)
            kw = dict(g_h=g_h.to(DEV) if use_h else None, g_out=g_wide, col=4, negative_slope=SLOPE, p=p, philox=pc)
            got = ops.bi_combine_backward(*dev, **kw)
            ratios = {name: nr.worst(t, b[name], bb[name]) for name, t in zip(names, got)}
            print(f'backward {d_in}x{d_out} N={N} p={p} g_h={use_h} g_n={use_n}: worst error / bound ',
                  '  '.join(f'{k} {v:.3f}' for k, v in ratios.items()))
            assert max(ratios.values()) <= 1, ratios
            again = ops.bi_combine_backward(*dev, **kw)
            assert all(torch.equal(a, c) for a, c in zip(got, again))


@pytest.mark.parametrize('d_in,d_out,N', [(64, 64, 257), (64, 32, 1000), (36, 20, 33)])
def test_module_against_its_torch_twin(ra, d_in, d_out, N):
    """graphmodule.BiCombiner under autograd next to forward_torch from the same generator state: the parity contract of the
    other fused paths (1e-4 on the scalar, 3e-4 of the largest element on every gradient)."""
    inp = inputs(N, d_in, d_out)
    torch.manual_seed(8)
    layer = ra.graphmodule.BiCombiner(d_in, d_out, dropout=0.1).to(DEV)
    G_h, G_n = inp['g_h'].to(DEV), inp['g_n'].to(DEV)
    grads = []
    for fused in (True, False):
        layer.zero_grad()
        x, m = inp['x'].to(DEV).requires_grad_(), inp['m'].to(DEV).requires_grad_()
        gen = generator(12)
        if fused:
            wide = torch.zeros(N, d_out + 4, device=DEV)
            h, wide = layer(x, m, out=wide, col=4, generator=gen)
            n = wide[:, 4:]
        else:
            h, n = layer.forward_torch(x, m, generator=gen)
        loss = (h * G_h).sum() + (n * G_n).sum()
        loss.backward()
        grads.append([float(loss.detach())] + [t.grad.clone() for t in (x, m, *layer.parameters())])
    (l0, *g0), (l1, *g1) = grads
    assert abs(l0 - l1) <= 1e-4 * abs(l1)
    for a, c in zip(g0, g1):
        assert float((a - c).abs().max()) <= 3e-4 * float(c.abs().max())
    layer.eval()
    x, m = inp['x'].to(DEV), inp['m'].to(DEV)
    gen = generator(12)
    with torch.no_grad():
        h_eval = layer(x, m, generator=gen)
        assert gen.get_offset() == generator(12).get_offset()               # eval: no dropout, nothing drawn
        assert torch.equal(h_eval, layer(x, m))
        assert float((h_eval - layer.forward_torch(x, m)[0]).abs().max()) <= 3e-4 * float(h_eval.abs().max())
