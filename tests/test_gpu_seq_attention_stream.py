"""GPU: rsa_attention_stream / rsa_attention_stream_backward (ops.seq_attention_stream, ops.seq_attention_stream_backward, and
seqmodule._SeqAttentionFn above 64 positions) against the float64 referee of tests/seq_attention_referee.py: every element of out,
lse and dqkv inside the bound its header derives; nothing of size L x L allocated; the SASRec tower at max_seq_len = 100."""
import functools

import pytest
import torch

import seq_attention_referee as sr
from test_gpu_seq_attention import generator, inputs as base_inputs, ra      # noqa: F401  (ra: the package fixture)
from test_gpu_seq_encoder import _batch, _tower, close

pytestmark = pytest.mark.gpu

DEV = 'cuda'
# (B, H, L, dh): one partial block, whole blocks and one row past them, 2 - 4 blocks, every head width, and 160 problems
SHAPES = [(2, 2, 17, 16), (2, 2, 64, 32), (2, 2, 65, 16), (2, 1, 80, 64), (2, 2, 127, 32), (2, 2, 128, 64), (2, 2, 129, 16),
          (3, 2, 200, 64), (40, 4, 130, 16)]
PADS = ['none', 'suffix', 'holes', 'full', 'first_block']


@functools.lru_cache(maxsize=None)
def inputs(B, H, L, dh):
    """The one-tile file's CPU inputs of the shape (never written to), and `first_block`: m stays -inf through the whole first block."""
    return dict(base_inputs(B, H, L, dh), first_block=(torch.arange(L) < 64).view(1, L).expand(B, L).contiguous())


def judge(ra, qkv, g, pad, causal, H, p, gen_seed=5):
    """One forward and backward on the device against the referee -> the worst ratios (out, lse, dqkv)."""
    ops = ra.ops
    B, L, D3 = qkv.shape
    dh = D3 // 3 // H
    dev_q, dev_g = qkv.to(DEV), g.to(DEV)
    dev_pad = None if pad is None else pad.to(DEV)
    gen, twin = generator(gen_seed, burn=3), generator(gen_seed, burn=3)
    before = gen.get_offset()
    pc = ra.rng.reserve(B * H * L * L, 4, torch.device(DEV), gen) if p else None
    out, lse, keep = ops.seq_attention_stream(dev_q, dev_pad, H, causal=causal, p=p, philox=pc, want_keep=True)
    if p:
        assert torch.equal(keep.bool(), torch.rand(B, H, L, L, device=DEV, generator=twin) < sr.q_of(p))
        assert gen.get_offset() == twin.get_offset()
    else:
        assert gen.get_offset() == before and bool(keep.all())       # p = 0 draws nothing
    out2, lse2 = ops.seq_attention_stream(dev_q, dev_pad, H, causal=causal, p=p, philox=pc)      # (the path that skips blocks)
    assert torch.equal(out, out2) and torch.equal(lse, lse2)
    dqkv = ops.seq_attention_stream_backward(dev_q, dev_pad, H, out, lse, dev_g, causal=causal, p=p, philox=pc)
    again = ops.seq_attention_stream_backward(dev_q, dev_pad, H, out, lse, dev_g, causal=causal, p=p, philox=pc)
    assert torch.equal(dqkv, again)                                  # no atomics: bit-equal
    assert not torch.isnan(out).any() and not torch.isnan(dqkv).any() and not torch.isnan(lse).any()
    f = sr.forward(qkv, pad, causal, H, keep.cpu(), p)
    qh, kh, _ = sr.split(dev_q, H)
    s32 = (qh @ kh.transpose(2, 3)) * torch.tensor(dh ** -0.5, dtype=torch.float32, device=DEV)
    allow, _ = sr.softmax_allowance(s32, f['ok'])
    fb = sr.forward_bounds(f, allow)
    b = sr.backward(f, g)
    some = f['some'].squeeze(3)
    lse_c = lse.cpu()
    assert torch.equal(torch.isneginf(lse_c), ~some)
    r_lse = float(((lse_c.double() - f['lse']).abs()[some] / fb['lse'][some]).max()) if bool(some.any()) else 0.0
    dead = ~some.transpose(1, 2).reshape(B, L, H, 1).expand(B, L, H, dh).reshape(B, L, H * dh)      # queries without a key
    assert not out.cpu()[dead].any() and not dqkv.cpu()[:, :, :H * dh][dead].any()                 # exact zeros
    return sr.worst_ratio(out, f['out'], fb['out']), r_lse, sr.worst_ratio(dqkv, b['dqkv'], sr.backward_bounds(f, fb, b, allow))


@pytest.mark.parametrize('causal', [True, False], ids=['causal', 'full'])
@pytest.mark.parametrize('shape', SHAPES, ids=str)
def test_forward_and_backward_within_the_bounds(ra, shape, causal):      # noqa: F811
    inp = inputs(*shape)
    for pad in PADS:
        for p in (0.0, 0.5):
            r_out, r_lse, r_dqkv = judge(ra, inp['qkv'], inp['g'], inp[pad], causal, shape[1], p)
            print(f'{shape} causal={causal} pad={pad} p={p}: out {r_out:.3f} lse {r_lse:.3f} dqkv {r_dqkv:.3f} of the bound')
            assert r_out <= 1.0 and r_lse <= 1.0 and r_dqkv <= 1.0, (shape, causal, pad, p, r_out, r_lse, r_dqkv)


def test_no_l2_tensor_is_allocated(ra):      # noqa: F811
    B, H, L, dh = 64, 4, 200, 16                                   # one [B, H, L, L] fp32 tensor is 39 MiB
    qkv, g = torch.randn(B, L, 3 * H * dh, device=DEV), torch.randn(B, L, H * dh, device=DEV)
    pad = torch.zeros(B, L, dtype=torch.uint8, device=DEV)
    pc = ra.rng.reserve(B * H * L * L, 4, torch.device(DEV), generator(3))

    def peak(fn):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        res = fn()
        torch.cuda.synchronize()
        return res, torch.cuda.max_memory_allocated() - base

    ra.ops.seq_attention_stream(qkv, pad, H, p=0.5, philox=pc)                # (first call: anything set up once)
    (out, lse), used = peak(lambda: ra.ops.seq_attention_stream(qkv, pad, H, p=0.5, philox=pc))
    assert used <= out.numel() * 4 + lse.numel() * 4 + (1 << 20), used
    dqkv, used = peak(lambda: ra.ops.seq_attention_stream_backward(qkv, pad, H, out, lse, g, p=0.5, philox=pc))
    assert used <= dqkv.numel() * 4 + (1 << 20), used


@pytest.mark.parametrize('bidirectional', [False, True], ids=['causal', 'bidirectional'])
def test_tower_at_100_positions_next_to_the_stock_tower(ra, bidirectional):      # noqa: F811
    """SASRecQueryEncoder(max_seq_len=100, fused_attention=True) -- refused before the streaming kernels -- next to the stock
    nn.TransformerEncoder over the same weights: the query within rtol 1e-4, atol 1e-6, parameter and item gradients within rtol 3e-4,
    atol 3e-6 max|g|, in train mode (dropout 0) and in eval mode with autograd on."""
    N, d, L, B = 503, 64, 100, 16
    item, enc = _tower(ra, N, d, L, 2, 128, 2, 0.0, seed=3, fused_attention=True, bidirectional=bidirectional)
    item2, stock = _tower(ra, N, d, L, 2, 128, 2, 0.0, seed=3, bidirectional=bidirectional)
    assert enc._fused is not None and stock._fused is None
    hist, seqlen, _ = _batch(N, L, B, seed=4)
    batch = {'in_item_id': hist.to(DEV), 'seqlen': seqlen.to(DEV)}
    w = torch.randn(B, d, generator=torch.Generator().manual_seed(5)).to(DEV)
    for train in (True, False):
        queries = []
        for e in (enc, stock):
            e.to(DEV).train(train).zero_grad()
            queries.append(e(batch))
            (queries[-1] * w).sum().backward()
        close(queries[0], queries[1], 1e-4, 1e-6)
        for a, b in zip(enc.parameters(), stock.parameters()):
            close(a.grad, b.grad, 3e-4, 3e-6 * float(b.grad.abs().max()))
