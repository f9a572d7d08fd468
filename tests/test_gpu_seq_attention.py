"""GPU: rsa_attention / rsa_attention_backward (ops.seq_attention, ops.seq_attention_backward, seqmodule._SeqAttentionFn) against
the float64 referee of tests/seq_attention_referee.py: every element of out, lse and dqkv inside the bound its header derives."""
import ctypes
import functools

import pytest
import torch

import seq_attention_referee as sr

pytestmark = pytest.mark.gpu

DEV = 'cuda'
# (B, H, L, dh): every tile (16, 32, 64) at and next to its edges, every head width, one wave .. four waves per problem, and a last
# workgroup that is not full (B H not a multiple of the 4 / 2 problems a workgroup holds at the small tiles)
SHAPES = [(3, 2, 9, 16), (2, 1, 1, 16), (5, 2, 16, 16), (5, 2, 17, 32), (3, 4, 31, 16), (3, 2, 32, 32), (2, 2, 33, 64), (2, 2, 50, 64),
          (2, 2, 63, 32), (2, 2, 64, 64), (300, 2, 20, 32)]
PADS = ['none', 'suffix', 'holes', 'full']
PS = [0.0, 0.1, 0.5]


@pytest.fixture(scope='module')
def ra():
    import recstudio_amd
    return recstudio_amd


def generator(seed, burn=0):
    gen = torch.Generator(device=DEV)
    gen.manual_seed(seed)
    if burn:
        torch.rand(burn, device=DEV, generator=gen)
    return gen


@functools.lru_cache(maxsize=None)
def inputs(B, H, L, dh):
    """CPU inputs of one shape, shared by the tests below and never written to."""
    gen = torch.Generator().manual_seed(1000 * L + 10 * dh + H + B)
    D = H * dh
    qkv, g = torch.randn(B, L, 3 * D, generator=gen), torch.randn(B, L, D, generator=gen)
    seqlen = torch.randint(1, L + 1, (B,), generator=gen)
    seqlen[0], seqlen[B - 1] = L, 1
    suffix = sr.pad_suffix(seqlen, L)
    holes = torch.rand(B, L, generator=gen) < 0.3
    full = suffix.clone()
    full[B // 2] = True
    return dict(qkv=qkv, g=g, none=None, suffix=suffix, holes=holes, full=full)


def judge(ra, qkv, g, pad, causal, H, p, gen_seed=5):
    """One forward and backward on the device against the referee -> the worst ratios (out, lse, dqkv)."""
    ops = ra.ops
    B, L, D3 = qkv.shape
    dev_q, dev_g = qkv.to(DEV), g.to(DEV)
    dev_pad = None if pad is None else pad.to(DEV)
    gen, twin = generator(gen_seed, burn=3), generator(gen_seed, burn=3)
    before = gen.get_offset()
    pc = ra.rng.reserve(B * H * L * L, 4, torch.device(DEV), gen) if p else None
    out, lse, keep = ops.seq_attention(dev_q, dev_pad, H, causal=causal, p=p, philox=pc, want_keep=True)
    if p:
        want_keep = torch.rand(B, H, L, L, device=DEV, generator=twin) < sr.q_of(p)
        assert torch.equal(keep.bool(), want_keep)
        assert gen.get_offset() == twin.get_offset()
    else:
        assert gen.get_offset() == before and bool(keep.all())       # p = 0 draws nothing
    out2, lse2 = ops.seq_attention(dev_q, dev_pad, H, causal=causal, p=p, philox=pc)      # (the path that skips blocks and draws)
    assert torch.equal(out, out2) and torch.equal(lse, lse2)
    dqkv = ops.seq_attention_backward(dev_q, dev_pad, H, out, lse, dev_g, causal=causal, p=p, philox=pc)
    again = ops.seq_attention_backward(dev_q, dev_pad, H, out, lse, dev_g, causal=causal, p=p, philox=pc)
    assert torch.equal(dqkv, again)                                  # no atomics: bit-equal
    for t in (out, dqkv):
        assert not torch.isnan(t).any()
    assert not torch.isnan(lse).any()
    f = sr.forward(qkv, pad, causal, H, keep.cpu(), p)
    dh = D3 // 3 // H
    qh, kh, _ = sr.split(dev_q, H)
    s32 = (qh @ kh.transpose(2, 3)) * torch.tensor(dh ** -0.5, dtype=torch.float32, device=DEV)
    allow, measured = sr.softmax_allowance(s32, f['ok'])
    fb = sr.forward_bounds(f, allow)
    b = sr.backward(f, g)
    tol = sr.backward_bounds(f, fb, b, allow)
    some = f['some'].squeeze(3)
    lse_c = lse.cpu()
    assert torch.equal(torch.isneginf(lse_c), ~some)
    r_lse = float(((lse_c.double() - f['lse']).abs()[some] / fb['lse'][some]).max()) if bool(some.any()) else 0.0
    dead = ~some.transpose(1, 2).reshape(B, L, H, 1).expand(B, L, H, dh).reshape(B, L, H * dh)      # queries without a key
    assert not out.cpu()[dead].any() and not dqkv.cpu()[:, :, :H * dh][dead].any()                 # exact zeros
    return sr.worst_ratio(out, f['out'], fb['out']), r_lse, sr.worst_ratio(dqkv, b['dqkv'], tol), measured


@pytest.mark.parametrize('shape', SHAPES, ids=str)
def test_forward_and_backward_within_the_bounds(ra, shape):
    B, H, L, dh = shape
    inp = inputs(*shape)
    for causal in (True, False):
        for pad in PADS:
            for p in PS:
                r_out, r_lse, r_dqkv, measured = judge(ra, inp['qkv'], inp['g'], inp[pad], causal, H, p)
                print(f'{shape} causal={causal} pad={pad} p={p}: out {r_out:.3f} lse {r_lse:.3f} dqkv {r_dqkv:.3f} of the bound '
                      f"(torch's softmax: {measured:.2f} u)")
                assert r_out <= 1.0 and r_lse <= 1.0 and r_dqkv <= 1.0, (shape, causal, pad, p, r_out, r_lse, r_dqkv)


def test_padded_keys_receive_exact_zeros(ra):
    B, H, L, dh = 5, 2, 17, 32
    inp = inputs(B, H, L, dh)
    D = H * dh
    pad = inp['full']
    out, lse = ra.ops.seq_attention(inp['qkv'].to(DEV), pad.to(DEV), H, causal=False)
    dqkv = ra.ops.seq_attention_backward(inp['qkv'].to(DEV), pad.to(DEV), H, out, lse, inp['g'].to(DEV), causal=False).cpu()
    assert not dqkv[:, :, D:][pad].any()                               # dk and dv of a padded key
    assert not out.cpu()[B // 2].any() and torch.isneginf(lse[B // 2]).all() and not dqkv[B // 2].any()


def test_mask_is_torch_rand_past_the_first_philox_round(ra):
    B, H, L, dh = 300, 2, 64, 16                                      # 2.46 M uniforms: more than one per thread of torch's grid
    qkv = torch.randn(B, L, 3 * H * dh, device=DEV)
    for p in (0.1, 0.5):
        gen, twin = generator(9, burn=5), generator(9, burn=5)
        pc = ra.rng.reserve(B * H * L * L, 4, torch.device(DEV), gen)
        assert B * H * L * L > pc.grid_threads
        keep = ra.ops.seq_attention(qkv, None, H, causal=True, p=p, philox=pc, want_keep=True)[2]
        assert torch.equal(keep.bool(), torch.rand(B, H, L, L, device=DEV, generator=twin) < sr.q_of(p))
        assert gen.get_offset() == twin.get_offset()


def test_offsets_past_4_gib(ra):
    H, L, dh, p = 2, 64, 64, 0.1
    D = H * dh
    B = (1 << 32) // (L * 3 * D * 4) + 40                             # qkv and dqkv end 3.9 MB past byte offset 4 GiB
    gen0 = generator(21)
    qkv = torch.randn(B, L, 3 * D, device=DEV, generator=gen0)
    g = torch.randn(B, L, D, device=DEV, generator=gen0)
    pad = torch.zeros(B, L, dtype=torch.bool, device=DEV)
    pad[-3, 40:] = True
    assert (B - 8) * L * 3 * D * 4 > 1 << 32                           # the judged sequences lie past it
    gen, twin = generator(22), generator(22)
    pc = ra.rng.reserve(B * H * L * L, 4, torch.device(DEV), gen)
    out, lse = ra.ops.seq_attention(qkv, pad, H, causal=True, p=p, philox=pc)
    dqkv = ra.ops.seq_attention_backward(qkv, pad, H, out, lse, g, causal=True, p=p, philox=pc)
    keep = (torch.rand(B, H, L, L, device=DEV, generator=twin) < sr.q_of(p))[-8:].cpu()
    tq, tg, tp = qkv[-8:].cpu(), g[-8:].cpu(), pad[-8:].cpu()
    f = sr.forward(tq, tp, True, H, keep, p)
    qh, kh, _ = sr.split(qkv[-8:], H)
    allow, _ = sr.softmax_allowance((qh @ kh.transpose(2, 3)) * torch.tensor(dh ** -0.5, device=DEV), f['ok'])
    fb = sr.forward_bounds(f, allow)
    b = sr.backward(f, tg)
    assert sr.worst_ratio(out[-8:], f['out'], fb['out']) <= 1.0
    assert sr.worst_ratio(dqkv[-8:], b['dqkv'], sr.backward_bounds(f, fb, b, allow)) <= 1.0
    assert float((lse[-8:].cpu().double() - f['lse']).abs().max()) <= float(fb['lse'].max())


def test_no_l2_tensor_is_allocated(ra):
    B, H, L, dh = 256, 4, 64, 16
    D = H * dh
    qkv = torch.randn(B, L, 3 * D, device=DEV)
    g = torch.randn(B, L, D, device=DEV)
    pad = torch.zeros(B, L, dtype=torch.bool, device=DEV).view(torch.uint8)
    gen = generator(3)
    pc = ra.rng.reserve(B * H * L * L, 4, torch.device(DEV), gen)
    ra.ops.seq_attention(qkv, pad, H, p=0.5, philox=pc)                # (first call: anything set up once)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out, lse = ra.ops.seq_attention(qkv, pad, H, p=0.5, philox=pc)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    assert peak <= out.numel() * 4 + lse.numel() * 4 + (1 << 20), peak          # any [B, H, L, L] fp32 tensor is 16 MiB
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    dqkv = ra.ops.seq_attention_backward(qkv, pad, H, out, lse, g, p=0.5, philox=pc)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    assert peak <= dqkv.numel() * 4 + (1 << 20), peak


def test_bad_arguments_are_refused(ra):
    nat = ra._native
    lib = nat.lib()

    def status(L=20, dh=32, shift=0):
        H = 2
        buf = torch.zeros(4 * L * 3 * H * dh + 8, device=DEV)
        out, lse = torch.zeros(4 * L * H * dh, device=DEV), torch.zeros(4 * H * L, device=DEV)
        a = nat.AttentionArgs()
        a.qkv, a.out, a.lse = buf.data_ptr() + shift, out.data_ptr(), lse.data_ptr()
        a.n_seq, a.seq_len, a.n_head, a.head_dim, a.causal, a.scale = 4, L, H, dh, 1, 0.25
        return lib.rsa_attention(ctypes.byref(a), None)

    assert status() == 0
    assert status(L=65) == -1 and status(dh=24) == -1 and status(shift=4) == -1
    torch.cuda.synchronize()
    qkv = torch.zeros(2, 65, 3 * 32, device=DEV)
    with pytest.raises(ValueError, match='sequence length'):
        ra.ops.seq_attention(qkv, None, 2)
    with pytest.raises(ValueError, match='head_dim'):
        ra.ops.seq_attention(torch.zeros(2, 9, 3 * 48, device=DEV), None, 2)
    with pytest.raises(TypeError, match='philox'):
        ra.ops.seq_attention(torch.zeros(2, 9, 3 * 32, device=DEV), None, 2, p=0.5)


def test_autograd_node_against_the_twin(ra):
    """seqmodule._SeqAttentionFn next to seq_attention_torch under autograd, from the same seed at p = 0.5 (they draw the same
    torch.rand): the parity contract, 1e-4 on out and 3e-4 on dqkv.  Elementwise rtol plus rtol / 100 of the largest magnitude: an
    element is a sum of up to L products whose fp32 error scales with the sum of their magnitudes, not with the element."""
    from recstudio_amd import seqmodule
    B, H, L, dh = 64, 2, 20, 32
    gen0 = torch.Generator().manual_seed(77)
    qkv = torch.randn(B, L, 3 * H * dh, generator=gen0).to(DEV)
    g = torch.randn(B, L, H * dh, generator=gen0).to(DEV)
    pad = sr.pad_suffix(torch.randint(1, L + 1, (B,), generator=gen0), L).to(DEV)
    for causal in (True, False):
        a, b = qkv.clone().requires_grad_(True), qkv.clone().requires_grad_(True)
        gen, twin = generator(31), generator(31)
        out = seqmodule.seq_attention(a, pad, causal, H, 0.5, gen)
        ref = seqmodule.seq_attention_torch(b, pad, causal, H, 0.5, twin)
        assert gen.get_offset() == twin.get_offset()
        out.backward(g)
        ref.backward(g)
        for got, want, rtol in ((out, ref, 1e-4), (a.grad, b.grad, 3e-4)):
            torch.testing.assert_close(got.detach(), want.detach(), rtol=rtol, atol=rtol * 1e-2 * float(want.detach().abs().max()))
