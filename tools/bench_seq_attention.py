"""Times the fused attention core of the sequence towers (ops.seq_attention / ops.seq_attention_backward: rsa_attention.hip) and
what it does to the SASRec step.  One process, one device, the arms of a group alternating, device events around every call,
warm-up calls first; a streaming copy of 1 GiB is timed at the start and at the end as the record of the box's state.  Prints one
JSON object and writes it to profiles/seq_attention_bench.json.

    python tools/bench_seq_attention.py [--batch 8192 --reps 20 --warmup 5]

Groups:
  (1) core            forward and forward + backward at configs[2] (B = 8192, H = 2, L = 50, dh = 64) and at L = 20, dh = 32, p = 0.5,
                      causal, right-padded histories: fused / twin (seqmodule.seq_attention_torch: the same rule in torch ops) / sdpa
                      (F.scaled_dot_product_attention as nn.MultiheadAttention calls it: head-major views, the merged float mask,
                      dropout_p).  Bytes by the model of the kernel's header (forward: qkv read, out written; backward: qkv, out, g
                      read, dqkv written) against the 8 TB/s peak; peak memory of a forward + backward in every form.
  (2) tower           the stock nn.TransformerEncoder (2 layers, d = 128, hidden 128, dropout 0.5) forward + backward next to
                      FusedTransformerEncoder over the same weights, and next to the same layer loop with the attention core taken
                      out (a = the v columns of qkv): what the Linears, LayerNorms, GELU and dropouts cost by themselves.
  (3) training_step   SASRec.training_step + backward at configs[2] (tools/bench_fit.py's synthetic sequences), model.fused_attention
                      on and off.
Recorded: median / min / max in ms and the ratios."""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

from graph_bench import peak_above, row, timed      # noqa: E402

PEAK_BYTES_PER_S = 8e12


def copy_gbps(dev):
    """A 1 GiB device-to-device copy: GB/s moved (read + written), the median of 5."""
    src = torch.empty(1 << 28, dtype=torch.float32, device=dev).normal_()
    dst = torch.empty_like(src)
    ms = timed([lambda: dst.copy_(src)], 5, 2)[0]
    return 2 * src.numel() * 4 / (statistics.median(ms) * 1e-3) / 1e9


def sdpa_form(qkv, key_pad, H, p):
    """The attention core as nn.MultiheadAttention runs it (need_weights=False): head-major views of q, k, v, the bool causal mask
    and the key-padding mask merged into one float mask, F.scaled_dot_product_attention with dropout_p, heads concatenated."""
    B, L, D3 = qkv.shape
    D = D3 // 3
    q, k, v = (t.reshape(B, L, H, D // H).transpose(1, 2) for t in qkv.split(D, dim=2))
    causal = torch.zeros(L, L, device=qkv.device).masked_fill(torch.triu(torch.ones(L, L, dtype=torch.bool, device=qkv.device), 1),
                                                              float('-inf'))
    pad = torch.zeros(B, L, device=qkv.device).masked_fill(key_pad, float('-inf'))
    mask = (causal.view(1, 1, L, L) + pad.view(B, 1, 1, L)).expand(B, H, L, L)
    out = F.scaled_dot_product_attention(q, k, v, attn_mask=mask, dropout_p=p)
    return out.transpose(1, 2).reshape(B, L, D)


def core(seqmodule, dev, B, H, L, dh, p, reps, warmup):
    D = H * dh
    g = torch.Generator(device=dev).manual_seed(L)
    qkv = torch.empty(B, L, 3 * D, device=dev).normal_(generator=g)
    g_out = torch.empty(B, L, D, device=dev).normal_(generator=g)
    seqlen = torch.randint(1, L + 1, (B,), device=dev, generator=g)
    key_pad = torch.arange(L, device=dev).view(1, L) >= seqlen.view(B, 1)
    leaf = qkv.clone().requires_grad_(True)
    forms = {'fused': lambda x: seqmodule.seq_attention(x, key_pad, True, H, p),
             'twin': lambda x: seqmodule.seq_attention_torch(x, key_pad, True, H, p),
             'sdpa': lambda x: sdpa_form(x, key_pad, H, p)}

    def fwd(f):
        def run():
            with torch.no_grad():
                return f(qkv)
        return run

    def both(f):
        def run():
            leaf.grad = None
            f(leaf).backward(g_out)
        return run

    names = list(forms)
    ms = timed([fwd(forms[n]) for n in names] + [both(forms[n]) for n in names], reps, warmup)
    out = dict(B=B, H=H, L=L, head_dim=dh, p=p, forward={}, forward_backward={}, peak_bytes={})
    bytes_f, bytes_b = B * L * 4 * D * 4, B * L * 8 * D * 4
    for i, n in enumerate(names):
        out['forward'][n] = row(ms[i])
        out['forward_backward'][n] = row(ms[len(names) + i])
        out['peak_bytes'][n] = peak_above(both(forms[n]))
    mf, mb = (statistics.median(ms[0]), statistics.median(ms[len(names)]))
    out['model_bytes'] = dict(forward=bytes_f, backward=bytes_b)
    out['fused_fraction_of_peak'] = dict(forward=bytes_f / (mf * 1e-3) / PEAK_BYTES_PER_S,
                                         forward_backward=(bytes_f + bytes_b) / (mb * 1e-3) / PEAK_BYTES_PER_S)
    for n in names[1:]:
        out[n + '_over_fused'] = dict(forward=out['forward'][n]['ms'] / mf, forward_backward=out['forward_backward'][n]['ms'] / mb)
    leaf.grad = None
    return out


def tower(seqmodule, dev, B, L, d, H, hidden, layers, p, reps, warmup):
    layer = torch.nn.TransformerEncoderLayer(d_model=d, nhead=H, dim_feedforward=hidden, dropout=p, activation='gelu',
                                             layer_norm_eps=1e-12, batch_first=True, norm_first=False)
    enc = torch.nn.TransformerEncoder(layer, num_layers=layers).to(dev).train()
    fused = seqmodule.FusedTransformerEncoder(enc, L)
    g = torch.Generator(device=dev).manual_seed(7)
    x = torch.empty(B, L, d, device=dev).normal_(generator=g).requires_grad_(True)
    g_out = torch.empty(B, L, d, device=dev).normal_(generator=g)
    seqlen = torch.randint(1, L + 1, (B,), device=dev, generator=g)
    key_pad = torch.arange(L, device=dev).view(1, L) >= seqlen.view(B, 1)
    causal = torch.triu(torch.ones(L, L, dtype=torch.bool, device=dev), 1)
    real = seqmodule.seq_attention

    def clear():
        x.grad = None
        for t in enc.parameters():
            t.grad = None

    def stock():
        clear()
        enc(x, mask=causal, src_key_padding_mask=key_pad).backward(g_out)

    def with_kernel():
        clear()
        fused(x, key_pad=key_pad, causal=True).backward(g_out)

    def without_core():
        clear()
        seqmodule.seq_attention = lambda qkv, *a: qkv[:, :, 2 * d:]
        try:
            fused(x, key_pad=key_pad, causal=True).backward(g_out)
        finally:
            seqmodule.seq_attention = real

    ms = timed([stock, with_kernel, without_core], reps, warmup)
    med = [statistics.median(t) for t in ms]
    clear()
    return dict(B=B, L=L, d=d, heads=H, hidden=hidden, layers=layers, p=p, stock=row(ms[0]), fused_attention=row(ms[1]),
                without_attention_core=row(ms[2]), stock_attention_core_ms=med[0] - med[2], fused_attention_core_ms=med[1] - med[2],
                stock_attention_share=(med[0] - med[2]) / med[0], stock_over_fused=med[0] / med[1])


def training_step(ra, dev, B, L, d, n, reps, warmup):
    from bench_fit import synthetic_seq_dataset
    ds = synthetic_seq_dataset(ra, dev, 40_000, 1_000_001, max_seq_len=L)
    steps = []
    for fused in (True, False):
        conf = {'model': {'embed_dim': d, 'fused_attention': fused}, 'train': {'negative_count': n, 'batch_size': B}}
        model = ra.SASRec(conf, loss=ra.SampledSoftmaxLoss(), sampler=ra.PopularSamplerModel(ds.item_freq))
        model._init_model(ds)
        model._init_parameter()
        model.to(dev)
        model.train()
        batch = None
        for b in ds.device_train_loader(B, shuffle=True, drop_last=True, device=dev):
            if batch is None or b['in_' + ds.fiid].shape[1] > batch['in_' + ds.fiid].shape[1]:
                batch = b                                   # the widest window of the epoch (L = max_seq_len)

        def step(model=model, batch=batch):
            for t in model.parameters():
                t.grad = None
            model.training_step(batch).backward()
        steps.append(step)
    ms = timed(steps, reps, warmup)
    med = [statistics.median(t) for t in ms]
    return dict(B=B, L=L, d=d, negative_count=n, fused_attention_on=row(ms[0]), fused_attention_off=row(ms[1]), off_over_on=med[1] / med[0])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=8192)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'seq_attention_bench.json'))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_seq_attention.py measures on the GPU: none found')
    import recstudio_amd as ra
    from recstudio_amd import seqmodule
    dev = torch.device('cuda')
    props = torch.cuda.get_device_properties(0)
    res = dict(device=props.name, compute_units=props.multi_processor_count, torch=torch.__version__, reps=a.reps, warmup=a.warmup,
               copy_gb_per_s_before=copy_gbps(dev))
    res['core'] = [core(seqmodule, dev, a.batch, 2, 50, 64, 0.5, a.reps, a.warmup), core(seqmodule, dev, a.batch, 2, 20, 32, 0.5, a.reps, a.warmup)]
    print(json.dumps(res['core']), file=sys.stderr, flush=True)
    torch.cuda.empty_cache()
    res['tower'] = tower(seqmodule, dev, a.batch, 50, 128, 2, 128, 2, 0.5, a.reps, a.warmup)
    print(json.dumps(res['tower']), file=sys.stderr, flush=True)
    torch.cuda.empty_cache()
    res['training_step'] = training_step(ra, dev, a.batch, 50, 128, 256, a.reps, a.warmup)
    res['copy_gb_per_s_after'] = copy_gbps(dev)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')
    print(json.dumps(res))


if __name__ == '__main__':
    main()
