"""CPU: the float64 referee of the fused attention core (tests/seq_attention_referee.py) judged on itself -- an fp32 emulation of the
kernel's order of operations inside half its bounds, nine seeded mistakes outside them -- and the argument checks of rsa_attention
/ rsa_attention_backward (they run before any HIP call).  No device kernel runs here.  Measured: the emulation within 0.03 of the bounds
of out and dqkv in all five cases, with torch's CPU softmax measuring 3.9 - 5.7 u (an allowance of 7.8 - 11.3 u)."""
import ctypes
import functools

import pytest
import torch

import seq_attention_referee as sr

# (B, H, L, dh, causal, p, seed)
CASES = [(4, 2, 9, 16, True, 0.0, 1), (4, 2, 9, 16, False, 0.5, 2), (3, 2, 20, 32, True, 0.5, 3), (3, 1, 33, 64, False, 0.1, 4),
         (3, 2, 17, 16, True, 0.1, 5)]

MISTAKES = ['causal_strict', 'pad_on_queries', 'no_scale', 'no_rescale', 'drop_before_norm', 'layout', 'D_from_P', 'dk_untransposed',
            'uniform_masked_row']


@pytest.fixture(scope='module')
def nat():
    import os
    from recstudio_amd import _native
    if not os.path.exists(_native.LIB_PATH):
        _native.build()
    return _native


def make_inputs(B, H, L, dh, seed, full_pad=True):
    """qkv, g, key_pad (a suffix with lengths 1 and L, a scattered hole, and -- ``full_pad`` -- the last sequence padded whole)"""
    gen = torch.Generator().manual_seed(seed)
    D = H * dh
    qkv = torch.randn(B, L, 3 * D, generator=gen)
    g = torch.randn(B, L, D, generator=gen)
    seqlen = torch.randint(1, L + 1, (B,), generator=gen)
    seqlen[0], seqlen[1 % B] = L, 1
    pad = sr.pad_suffix(seqlen, L)
    if L > 2:
        pad[0, L // 2] = True                      # a hole inside the longest sequence
    if full_pad:
        pad[B - 1] = True
    u = torch.rand(B, H, L, L, generator=gen)
    return qkv, g, pad, u


@functools.lru_cache(maxsize=None)
def judged(case):
    B, H, L, dh, causal, p, seed = case
    qkv, g, pad, u = make_inputs(B, H, L, dh, seed)
    keep = u < sr.q_of(p)
    out32, lse32, dqkv32, s32 = sr.emulate_fp32(qkv, pad, causal, H, keep, p, g)
    f = sr.forward(qkv, pad, causal, H, keep, p)
    allow, _ = sr.softmax_allowance(s32, f['ok'])
    fb = sr.forward_bounds(f, allow)
    b = sr.backward(f, g)
    tol = sr.backward_bounds(f, fb, b, allow)
    return dict(qkv=qkv, g=g, pad=pad, keep=keep, f=f, fb=fb, b=b, tol=tol, allow=allow, out32=out32, lse32=lse32, dqkv32=dqkv32)


@pytest.mark.parametrize('case', CASES, ids=str)
def test_fp32_emulation_stays_within_half_of_every_bound(case):
    j = judged(case)
    f, fb = j['f'], j['fb']
    assert sr.worst_ratio(j['out32'], f['out'], fb['out']) <= 0.5
    assert sr.worst_ratio(j['dqkv32'], j['b']['dqkv'], j['tol']) <= 0.5
    some = f['some'].squeeze(3)
    assert torch.equal(torch.isneginf(j['lse32']), ~some) and torch.equal(torch.isneginf(f['lse']), ~some)
    assert float(((j['lse32'].double() - f['lse']).abs()[some] / fb['lse'][some]).max()) <= 0.5
    assert not torch.isnan(j['out32']).any() and not torch.isnan(j['dqkv32']).any()


def test_rows_without_a_key_are_exact_zeros_in_the_referee():
    j = judged(CASES[1])                           # not causal, the last sequence padded whole
    f, b = j['f'], j['b']
    assert not f['some'][-1].any() and not f['out'][-1].any() and not b['dqkv'][-1].any()
    assert torch.isneginf(f['lse'][-1]).all()
    assert float(j['fb']['out'][-1].max()) < 1e-35 and float(j['tol'][-1].max()) < 1e-35


@pytest.mark.parametrize('mistake', MISTAKES)
def test_a_seeded_mistake_leaves_a_bound(mistake):
    """Each mistake, made in float64 (no rounding of its own), is outside the bound of ``out`` or of a gradient in every case it can
    show in: dropout mistakes need p > 0, the masked-row mistake a row without a key."""
    shown = 0
    for case in CASES:
        B, H, L, dh, causal, p, seed = case
        if mistake in ('no_rescale', 'drop_before_norm', 'D_from_P') and not p:
            continue
        if mistake == 'causal_strict' and not causal:
            continue
        if mistake == 'uniform_masked_row' and causal:
            continue
        if mistake == 'layout' and H == 1:                       # one head: the two layouts are the same
            continue
        j = judged(case)
        fwd = mistake not in ('D_from_P', 'dk_untransposed')
        f = sr.forward(j['qkv'], j['pad'], causal, H, j['keep'], p, mistake=mistake if fwd else None)
        b = sr.backward(f, j['g'], mistake=None if fwd else mistake)
        worst = max(sr.worst_ratio(f['out'], j['f']['out'], j['fb']['out']), sr.worst_ratio(b['dqkv'], j['b']['dqkv'], j['tol']))
        assert worst > 1.0, (mistake, case, worst)
        shown += 1
    assert shown >= 1


# ---------------------------------------------------------------------------------------------------------------- the C ABI
def _block(nat, n_seq=8, L=20, H=2, dh=32, p=0.0):
    a = nat.AttentionArgs()
    for name in ('qkv', 'key_pad', 'out', 'lse', 'g_out', 'dqkv'):
        setattr(a, name, 4096)
    a.n_seq, a.seq_len, a.n_head, a.head_dim, a.causal, a.scale, a.p = n_seq, L, H, dh, 1, 0.25, p
    return a


@pytest.mark.parametrize('entry', ['rsa_attention', 'rsa_attention_backward'])
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
    refused(_block(nat, L=65), b'seq_len')
    refused(_block(nat, L=0), b'seq_len')
    refused(_block(nat, dh=24), b'head_dim')
    refused(_block(nat, dh=128), b'head_dim')
    refused(_block(nat, H=0), b'n_head')
    refused(_block(nat, n_seq=-1), b'negative')
    refused(_block(nat, p=1.0), b'[0, 1)')
    refused(_block(nat, p=0.1), b'philox')             # grid_threads 0
    a = _block(nat, p=0.1)
    a.grid_threads, a.offset = 256, 2
    refused(a, b'philox')
    a = _block(nat, n_seq=1 << 19, L=64, p=0.5)        # 2^19 * 2 * 64 * 64 = 2^32 uniforms
    a.grid_threads = 256
    refused(a, b'torch.rand splits')
    for field in ('qkv', 'out', 'lse'):
        a = _block(nat)
        setattr(a, field, None)
        refused(a, b'is null')
    for field in ('qkv', 'out'):
        a = _block(nat)
        setattr(a, field, 4100)
        refused(a, b'16-byte aligned')
    if entry == 'rsa_attention_backward':
        for field in ('g_out', 'dqkv'):
            a = _block(nat)
            setattr(a, field, None)
            refused(a, b'is null')
            setattr(a, field, 4104)
            refused(a, b'16-byte aligned')
    assert fn(ctypes.byref(_block(nat, n_seq=0)), None) == 0            # nothing to do: no launch, no HIP call
    assert lib.rsa_abi_version() == 13


def test_ops_refuse_what_the_kernel_cannot_do():
    from recstudio_amd import seqmodule
    enc = lambda d, h, **kw: torch.nn.TransformerEncoder(                # noqa: E731
        torch.nn.TransformerEncoderLayer(d_model=d, nhead=h, dim_feedforward=16, batch_first=True, **kw), num_layers=1)
    seqmodule.FusedTransformerEncoder(enc(32, 2), 64)
    with pytest.raises(ValueError, match='max_seq_len'):
        seqmodule.FusedTransformerEncoder(enc(32, 2), 65)
    with pytest.raises(ValueError, match='head_dim'):
        seqmodule.FusedTransformerEncoder(enc(48, 2), 20)
    with pytest.raises(ValueError, match='norm_first'):
        seqmodule.FusedTransformerEncoder(enc(32, 2, norm_first=True), 20)


def test_the_torch_twin_follows_the_referee():
    """seqmodule.seq_attention_torch (the CPU path and the GPU tests' twin) in float64 against the referee, autograd included."""
    from recstudio_amd import seqmodule
    for case in CASES[:3]:
        B, H, L, dh, causal, p, seed = case
        j = judged(case)
        gen = torch.Generator().manual_seed(seed)
        x = j['qkv'].double().requires_grad_(True)
        out, keep = seqmodule.seq_attention_torch(x, j['pad'], causal, H, p, gen, want_keep=True)
        if p:
            gen2 = torch.Generator().manual_seed(seed)
            assert torch.equal(keep, torch.rand(B, H, L, L, generator=gen2) < sr.q_of(p))
        f = sr.forward(j['qkv'], j['pad'], causal, H, keep, p)
        b = sr.backward(f, j['g'])
        out.backward(j['g'].double())
        torch.testing.assert_close(out.detach(), f['out'], rtol=1e-12, atol=1e-13)
        torch.testing.assert_close(x.grad, b['dqkv'], rtol=1e-11, atol=1e-13)
