"""GPU: the fused sequence tower (seqmodule.FusedTransformerEncoder behind SASRecQueryEncoder(fused_attention=True) and
SASRec's model.fused_attention) against the reference's recorded tower, the stock nn.TransformerEncoder on this device, a float64
training step on the masks and negatives the kernels drew, and a short fit next to the stock model."""
import copy
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import oracle
import seq_attention_referee as sr
from test_dataset_golden import make

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
DEV = 'cuda'


@pytest.fixture(scope='module')
def ra():
    import recstudio_amd
    recstudio_amd._native.lib()
    torch.cuda.init()
    return recstudio_amd


def close(got, want, rtol, atol):
    torch.testing.assert_close(torch.as_tensor(got).detach().cpu().float(), torch.as_tensor(want).detach().cpu().float(), rtol=rtol,
                               atol=atol)


def fixture_tower(ra, **kw):
    from recstudio_amd.retriever import SASRecQueryEncoder
    g = np.load(os.path.join(HERE, 'golden', 'sasrec.npz'))
    N, d, L = int(g['N']), int(g['d']), int(g['L'])
    item = torch.nn.Embedding(N, d, padding_idx=0)
    enc = SASRecQueryEncoder('item_id', d, L, int(g['heads']), int(g['hidden']), 0.0, 'gelu', 1e-12, int(g['layers']), item, **kw)
    state = {k[3:]: torch.from_numpy(g[k]) for k in g.files if k.startswith('w::')}
    assert set(state) == set(enc.state_dict())
    enc.load_state_dict(state)
    return g, item, enc.to(DEV)


def test_fixture_on_the_device(ra):
    """The reference's recorded tower through fused_attention=True: (i) against the fixture at the tolerances the stock-path test
    (test_gpu_round4.test_sasrec_tower_and_tied_gradients_vs_reference) uses for its comparison (i); (ii) against the stock
    nn.TransformerEncoder over the same weights on this device, 1e-4 on the query and the loss, 3e-4 on the gradients, in train mode
    (p = 0) and in eval mode."""
    g, item, enc = fixture_tower(ra, fused_attention=True)
    _, item2, stock = fixture_tower(ra)
    hist, seqlen = torch.from_numpy(g['hist']).to(DEV), torch.from_numpy(g['seqlen']).to(DEV)
    pos, neg = torch.from_numpy(g['pos']).to(DEV), torch.from_numpy(g['neg']).to(DEV)
    log_pos, log_neg = torch.from_numpy(g['log_pos']).to(DEV), torch.from_numpy(g['log_neg']).to(DEV)
    batch = {'in_item_id': hist, 'seqlen': seqlen}
    n = neg.shape[1]
    runs = []
    for it, e in ((item, enc), (item2, stock)):
        e.train()
        query = e(batch)
        score, _ = ra.retriever_scores(it.weight, query, n, pos_ids=pos, neg_ids=neg)
        loss = ra.SampledSoftmaxLoss()(None, score['pos_score'], log_pos, score['neg_score'], log_neg)
        loss.backward()
        runs.append((query, loss, it.weight.grad, e.position_emb.weight.grad, e.transformer_layer.layers[0].linear1.weight.grad))
    (query, loss, gi, gp, gl), (q2, l2, gi2, gp2, gl2) = runs
    close(query, g['ssm_query'], 3e-3, 3e-4)
    assert abs(loss.item() - float(g['ssm_loss'])) <= 1e-3 * abs(float(g['ssm_loss']))
    close(gi, g['ssm_item_grad'], 2e-2, 3e-5)
    close(gp, g['ssm_posemb_grad'], 2e-2, 3e-5)
    assert not gi[0].any()
    close(query, q2, 1e-4, 1e-6)
    assert abs(loss.item() - l2.item()) <= 1e-4 * abs(l2.item())
    for a, b in ((gi, gi2), (gp, gp2), (gl, gl2)):
        close(a, b, 3e-4, 3e-6 * float(b.abs().max()))
    # eval mode.  With autograd on, nn.TransformerEncoder runs the layers it trains with: 1e-4.  Under no_grad it takes torch's
    # inference fast path, which is itself 2.6e-4 away from the recorded reference on this device (measured: stock 2.613e-04, fused
    # 4.768e-07, fused - stock 2.613e-04), so there the fused tower is held to the recorded reference instead, at the bound of
    # tests/test_seq_encoder_twin.py -- 300 times tighter than comparison (i)
    enc.eval(), stock.eval()
    close(enc(batch), stock(batch), 1e-4, 1e-6)
    with torch.no_grad():
        fast = float((stock(batch).cpu() - torch.from_numpy(g['eval_query'])).abs().max())
        print(f"eval, no_grad: stock fast path - fixture {fast:.3e}, fused - fixture "
              f"{float((enc(batch).cpu() - torch.from_numpy(g['eval_query'])).abs().max()):.3e}")
        close(enc(batch), g['eval_query'], 1e-4, 1e-6)


def _tower(ra, N, d, L, heads, hidden, layers, dropout, seed, **kw):
    from recstudio_amd.retriever import SASRecQueryEncoder
    torch.manual_seed(seed)
    item = torch.nn.Embedding(N, d, padding_idx=0)
    with torch.no_grad():
        item.weight.mul_(0.3)
        item.weight[0] = 0
    enc = SASRecQueryEncoder('item_id', d, L, heads, hidden, dropout, 'gelu', 1e-12, layers, item, **kw)
    return item, enc


def _batch(N, L, B, seed):
    gen = torch.Generator().manual_seed(seed)
    seqlen = torch.randint(1, L + 1, (B,), generator=gen)
    seqlen[0], seqlen[1] = L, 1
    hist = torch.randint(1, N, (B, L), generator=gen)
    hist[torch.arange(L).view(1, -1) >= seqlen.view(-1, 1)] = 0
    return hist, seqlen, torch.randint(1, N, (B,), generator=gen)


def _float64_step(item_w, enc, hist, seqlen, pos, neg, masks, keeps, causal):
    """The tower and the BCE step in float64 on the CPU, with the given nn.Dropout masks (already scaled: 0 or 1 / (1 - p)) and
    attention keep masks.  -> (loss, {parameter name: gradient}, item gradient)."""
    e = copy.deepcopy(enc).cpu().double()
    w = item_w.detach().cpu().double().requires_grad_(True)
    masks = [m.cpu().double() for m in masks]
    B, L = hist.shape
    x = (F.embedding(hist, w, padding_idx=0) + e.position_emb.weight[:L].unsqueeze(0)) * masks[0]
    pad = hist == 0
    k = 1
    for li, layer in enumerate(e.transformer_layer.layers):
        mha = layer.self_attn
        H = mha.num_heads
        qkv = F.linear(x, mha.in_proj_weight, mha.in_proj_bias)
        qh, kh, vh = sr.split(qkv, H)
        s = (qh @ kh.transpose(2, 3)) * (qh.shape[-1] ** -0.5)
        ok = sr.allowed(pad, causal, B, L).expand(B, H, L, L)
        pr = torch.softmax(s.masked_fill(~ok, float('-inf')), dim=3)
        pt = pr * keeps[li].cpu().double() / sr.q_of(mha.dropout)
        a = (pt @ vh).transpose(1, 2).reshape(B, L, -1)
        x = layer.norm1(x + mha.out_proj(a) * masks[k])
        h = layer.linear2(F.gelu(layer.linear1(x)) * masks[k + 1])
        x = layer.norm2(x + h * masks[k + 2])
        k += 3
    query = x.gather(1, (seqlen - 1).view(-1, 1, 1).expand(-1, 1, x.shape[-1])).squeeze(1)
    ps = (query * F.embedding(pos, w)).sum(-1)
    ns = (query.unsqueeze(1) * F.embedding(neg, w)).sum(-1)
    loss = oracle.bce_loss(ps, ns)
    loss.backward()
    return loss.item(), {n: p.grad for n, p in e.named_parameters() if p.grad is not None}, w.grad


@pytest.mark.parametrize('bidirectional', [False, True], ids=['causal', 'bidirectional'])
def test_one_training_step_against_float64(ra, bidirectional):
    """dropout 0.5, d = 64, L = 20, B = 64, two layers of two heads.  The generator is consumed in the documented order -- the
    input dropout, then per layer the attention's torch.rand, dropout1, the feed-forward's dropout, dropout2 -- so replaying it
    yields every mask; the negatives are the ones the fused scorer drew.  Against the float64 step on those: 1e-4 on the loss, 3e-4
    on every parameter gradient (with 3e-4 / 100 of the gradient's largest magnitude for the elements that cancel).  The order
    itself is asserted against a torch-twin tower from the same seed."""
    N, d, L, B, heads, hidden, layers, p = 503, 64, 20, 64, 2, 128, 2, 0.5
    item, enc = _tower(ra, N, d, L, heads, hidden, layers, p, seed=3, fused_attention=True, bidirectional=bidirectional)
    item.to(DEV), enc.to(DEV).train()
    hist, seqlen, pos = _batch(N, L, B, seed=4)
    batch = {'in_item_id': hist.to(DEV), 'seqlen': seqlen.to(DEV)}
    sampler = ra.UniformSampler(N - 1).to(DEV)
    torch.manual_seed(11)
    query = enc(batch)
    score, neg = ra.retriever_scores(item.weight, query, 4, pos_ids=pos.to(DEV), sampler=sampler)
    loss = ra.BinaryCrossEntropyLoss()(None, score['pos_score'], score['log_pos_prob'], score['neg_score'], score['log_neg_prob'])
    loss.backward()
    # ---- the replay
    torch.manual_seed(11)
    ones = lambda *s: torch.ones(*s, device=DEV)                  # noqa: E731
    masks, keeps = [F.dropout(ones(B, L, d), p, True)], []
    for _ in range(layers):
        keeps.append(torch.rand(B, heads, L, L, device=DEV) < sr.q_of(p))
        masks += [F.dropout(ones(B, L, d), p, True), F.dropout(ones(B, L, hidden), p, True), F.dropout(ones(B, L, d), p, True)]
    # ---- the same order in a torch-twin tower (the attention core in torch ops, everything else the same modules)
    from recstudio_amd import seqmodule
    twin = copy.deepcopy(enc)
    twin.item_encoder = item
    real = seqmodule._SeqAttentionFn.apply
    try:
        seqmodule._SeqAttentionFn.apply = staticmethod(
            lambda qkv, pad, causal, H, pp, gen: seqmodule.seq_attention_torch(qkv, pad, causal, H, pp, gen))
        torch.manual_seed(11)
        with torch.no_grad():
            q_twin = twin(batch)
    finally:
        seqmodule._SeqAttentionFn.apply = real
    close(query, q_twin, 1e-4, 1e-6)
    # ---- the float64 step
    want_loss, want, want_item = _float64_step(item.weight, enc, hist, seqlen, pos, neg.cpu(), masks, keeps, not bidirectional)
    assert abs(loss.item() - want_loss) <= 1e-4 * abs(want_loss), (loss.item(), want_loss)
    got = dict(enc.named_parameters())
    assert len(want) == 1 + 12 * layers                            # the position table and 12 tensors per layer
    for name, gw in want.items():
        if name.startswith('item_encoder'):
            continue
        close(got[name].grad, gw, 3e-4, 3e-6 * float(gw.abs().max()))
    close(item.weight.grad, want_item, 3e-4, 3e-6 * float(want_item.abs().max()))


def test_fit_next_to_the_stock_model_and_checkpoints(ra, golden):
    """3 epochs of SASRec on ml-100k with model.fused_attention next to the stock model from the same seed.  dropout_rate 0: every
    epoch's loss within 2 % (the two towers differ in rounding only.  Measured: step losses differ by at most 2.4e-7 and 130 of the
    156 of an epoch are bit-equal, the weights after an epoch by 1e-8 .. 8e-5; the three epoch means agree to fp32 resolution, gap 0).  dropout_rate 0.5 (other masks than
    nn.MultiheadAttention's): the loss falls and the metrics are finite.  A state_dict of one loads into the other."""
    from recstudio_amd import seqmodule
    g = golden('data_ml100k')
    trn, val, tst = make(ra.SeqDataset, g, max_seq_len=20).build(split_ratio=2)
    runs = {}
    for rate in (0.0, 0.5):
        for fused in (True, False):
            if rate and not fused:
                continue
            cfg = {'model': {'embed_dim': 64, 'dropout_rate': rate, 'fused_attention': fused},
                   'train': {'epochs': 3, 'batch_size': 512}, 'eval': {'batch_size': 256}}
            model = ra.SASRec(cfg)
            calls = []
            real = seqmodule._SeqAttentionFn.apply
            seqmodule._SeqAttentionFn.apply = staticmethod(lambda *a: (calls.append(1), real(*a))[1])
            try:
                model.fit(trn, val)
            finally:
                seqmodule._SeqAttentionFn.apply = real
            assert (model.query_encoder._fused is not None) == fused and bool(calls) == fused      # the kernel ran, or never
            runs[rate, fused] = (model, [h['train_loss'] for h in model.history], model.evaluate(tst, verbose=False))
    hip, ref = runs[0.0, True][1], runs[0.0, False][1]
    print('fused', hip, 'stock', ref, 'gap', [abs(a - b) / abs(b) for a, b in zip(hip, ref)])
    assert len(hip) == 3 and all(abs(a - b) <= 0.02 * abs(b) for a, b in zip(hip, ref)), (hip, ref)
    drop = runs[0.5, True]
    assert drop[1][0] > drop[1][2] and all(np.isfinite(v) for v in drop[2].values()) and all(np.isfinite(drop[1]))
    fused_model, stock_model = runs[0.0, True][0], runs[0.0, False][0]
    assert list(fused_model.state_dict()) == list(stock_model.state_dict())
    stock_model.load_state_dict(fused_model.state_dict())
    fused_model.load_state_dict(stock_model.state_dict())
