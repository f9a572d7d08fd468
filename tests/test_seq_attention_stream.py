"""CPU: the streaming attention pair (rsa_attention_stream / rsa_attention_stream_backward): their argument checks (before any HIP
call), the constructor limits of FusedTransformerEncoder(stream=True), and an fp32 emulation of the kernels' order of operations --
64-key blocks under the RUNNING softmax, the form that ships -- against the float64 referee of tests/seq_attention_referee.py.
Measured (worst ratio to the bound over the three cases): out 0.015, lse 0.042, dqkv 0.022, with torch's CPU softmax at 6.2 - 8.1 u:
the running form needs no second sweep."""
import ctypes

import pytest
import torch

import seq_attention_referee as sr
from test_seq_attention_referee import _block, make_inputs, nat      # noqa: F401  (nat: the fixture that builds the library)

# (B, H, L, dh, causal, p, seed)
CASES = [(2, 2, 65, 16, True, 0.0, 1), (2, 1, 130, 64, False, 0.5, 2), (2, 2, 200, 32, True, 0.5, 3)]
NEG = float('-inf')


def emulate_stream(qkv, key_pad, causal, H, keep, p, g):
    """The streaming kernels' order in fp32 torch ops -> (out, lse, dqkv, s32): per 64-key block m' = max(m, block max), alpha =
    exp(m - m') (0 while m = -inf), l = l alpha + sum e, o = o alpha + (keep e / q) v; P = exp(s - lse) and block sums backward."""
    B, L, D3 = qkv.shape
    dh = D3 // 3 // H
    q, k, v = sr.split(qkv.float(), H)
    ok = sr.allowed(key_pad, causal, B, L).expand(B, H, L, L)
    s = (q @ k.transpose(2, 3)) * torch.tensor(dh ** -0.5, dtype=torch.float32)
    qf = torch.tensor(sr.q_of(p), dtype=torch.float32)
    kp = keep.float() / qf if p else torch.ones_like(s)
    zero = torch.zeros(())
    m, l, o = torch.full((B, H, L, 1), NEG), torch.zeros(B, H, L, 1), torch.zeros(B, H, L, dh)
    blocks = [slice(j0, min(j0 + 64, L)) for j0 in range(0, L, 64)]
    for blk in blocks:
        sb = s[..., blk].masked_fill(~ok[..., blk], NEG)
        m_new = torch.maximum(m, sb.amax(3, keepdim=True))
        alpha = torch.where(torch.isneginf(m), zero, (m - m_new).exp())
        e = torch.where(torch.isneginf(sb), zero, (sb - m_new).exp())
        l = l * alpha + e.sum(3, keepdim=True)
        o = o * alpha + (e * kp[..., blk]) @ v[:, :, blk]
        m = m_new
    some = l > 0
    out_h = torch.where(some, o / l, zero)
    lse = torch.where(some, m + l.clamp_min(1e-37).log(), torch.full_like(m, NEG))
    gh = sr.heads(g.float(), H)
    Pb = torch.where(ok, (s - torch.where(some, lse, zero)).exp(), zero)
    dS = Pb * ((gh @ v.transpose(2, 3)) * kp - (gh * out_h).sum(3, keepdim=True))
    Ptb = Pb * kp
    dq = sum(dS[..., blk] @ k[:, :, blk] for blk in blocks) * (dh ** -0.5)
    dk = sum(dS[:, :, blk].transpose(2, 3) @ q[:, :, blk] for blk in blocks) * (dh ** -0.5)
    dv = sum(Ptb[:, :, blk].transpose(2, 3) @ gh[:, :, blk] for blk in blocks)
    return out_h.transpose(1, 2).reshape(B, L, H * dh), lse.squeeze(3), sr.unheads(dq, dk.float(), dv), s


@pytest.mark.parametrize('case', CASES, ids=str)
def test_running_softmax_in_fp32_stays_within_every_bound(case):
    B, H, L, dh, causal, p, seed = case
    qkv, g, pad, u = make_inputs(B, H, L, dh, seed)
    keep = u < sr.q_of(p)
    out32, lse32, dqkv32, s32 = emulate_stream(qkv, pad, causal, H, keep, p, g)
    f = sr.forward(qkv, pad, causal, H, keep, p)
    allow, measured = sr.softmax_allowance(s32, f['ok'])
    fb = sr.forward_bounds(f, allow)
    b = sr.backward(f, g)
    some = f['some'].squeeze(3)
    assert torch.equal(torch.isneginf(lse32), ~some)
    r_out = sr.worst_ratio(out32, f['out'], fb['out'])
    r_lse = float(((lse32.double() - f['lse']).abs()[some] / fb['lse'][some]).max())
    r_dqkv = sr.worst_ratio(dqkv32, b['dqkv'], sr.backward_bounds(f, fb, b, allow))
    print(f"{case}: out {r_out:.3f} lse {r_lse:.3f} dqkv {r_dqkv:.3f} of the bound (torch's softmax: {measured:.2f} u)")
    assert r_out <= 1.0 and r_lse <= 1.0 and r_dqkv <= 1.0
    assert not torch.isnan(out32).any() and not torch.isnan(dqkv32).any()


@pytest.mark.parametrize('entry', ['rsa_attention_stream', 'rsa_attention_stream_backward'])
def test_argument_checks_run_before_any_hip_call(nat, entry):    # noqa: F811
    lib = nat.lib()
    fn = getattr(lib, entry)

    def refused(a, text):
        assert fn(ctypes.byref(a), None) == -1
        assert text in lib.rsa_last_error(), lib.rsa_last_error()

    assert fn(None, None) == -1
    refused(_block(nat, L=0), b'seq_len')
    refused(_block(nat, L=1025), b'seq_len')
    refused(_block(nat, dh=24), b'head_dim')
    refused(_block(nat, L=200, p=0.1), b'philox')
    for field, bad, text in [('qkv', None, b'is null'), ('lse', None, b'is null'), ('out', 4100, b'16-byte aligned')] + \
            ([('g_out', None, b'is null'), ('dqkv', 4104, b'16-byte aligned')] if entry.endswith('backward') else []):
        a = _block(nat, L=200)
        setattr(a, field, bad)
        refused(a, text)
    assert fn(ctypes.byref(_block(nat, L=200, n_seq=0)), None) == 0      # nothing to do: no launch, no HIP call


def test_stream_encoder_limits():
    from recstudio_amd import ops, seqmodule
    enc = torch.nn.TransformerEncoder(torch.nn.TransformerEncoderLayer(d_model=32, nhead=2, dim_feedforward=16, batch_first=True), 1)
    assert ops.SEQ_ATTENTION_STREAM_MAX_LEN == 1024
    seqmodule.FusedTransformerEncoder(enc, 65, stream=True)
    seqmodule.FusedTransformerEncoder(enc, 1024, stream=True)
    with pytest.raises(ValueError, match='SEQ_ATTENTION_STREAM_MAX_LEN'):
        seqmodule.FusedTransformerEncoder(enc, 1025, stream=True)
