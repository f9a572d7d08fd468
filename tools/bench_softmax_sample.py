"""Times exact softmax sampling over the whole catalog -- ops.softmax_sample, the streaming form of ``sampling(method='brute')`` --
next to the torch op sequence it replaces (baseretriever.py:313-328: scores, softmax, pad, scatter of the history, torch.multinomial,
two gathers and a log) on the same device, in the same process, alternating; prints one JSON object and writes it to
profiles/softmax_sample_bench.json.

    python tools/bench_softmax_sample.py [--items 1000000 --big-items 10000000 --dim 128 --queries 2048 --neg 64 --hist 100 --reps 7]
                                         [--variant-libs 64=PATH,256=PATH]

brute      : the streaming path vs the torch path at --items, with and without a --hist-id history: median / min / max of --reps calls
             after 3 warm-up calls (device events), and the peak of torch.cuda.max_memory_allocated over one call of each.
block_pass : the MFMA block pass + merge alone (num_neg = 0) vs rsa_fullscore's logsumexp alone, alternating: its floor is that one
             2 B N d product.
block_size : the streaming path of other builds of the library (--variant-libs G=PATH, built with
             ``VARIANT_FILES=rsa_softmax_sample tools/build_variant.sh g64 -DRSA_SS_G=64``) next to the default build's, alternating.
big        : the streaming path alone at --big-items; the torch path is attempted once and its OutOfMemoryError recorded as such."""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fns, reps, warmup=3):
    """dict(ms = median, ms_min_max) per function, the functions called in turn (a, b, a, b, ...)."""
    for _ in range(warmup):
        for f in fns:
            f()
    torch.cuda.synchronize()
    ms = [[] for _ in fns]
    for _ in range(reps):
        for i, f in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            f()
            b.record()
            b.synchronize()
            ms[i].append(a.elapsed_time(b))
    return [dict(ms=statistics.median(t), ms_min_max=(min(t), max(t))) for t in ms]


def peak_bytes(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    del out
    return rise


def torch_brute(item_vector, query, n, hist=None, t=1.0):
    """The reference's op sequence (baseretriever.py:313-328) with torch ops."""
    all_prob = torch.nn.functional.pad(torch.softmax(query @ item_vector.t() / t, dim=-1), pad=(1, 0))
    sampling_prob = all_prob if hist is None else all_prob.scatter(-1, hist, 0.0)
    neg_id = torch.multinomial(sampling_prob, n, replacement=True)
    return neg_id, torch.log(torch.gather(sampling_prob, dim=-1, index=neg_id))


def variant_sampler(path):
    """``softmax_sample`` of another build of the library (its own G, so its own workspace size)."""
    from recstudio_amd import _native as nat, ops, rng
    lib = ctypes.CDLL(path)
    lib.rsa_softmax_sample.restype = ctypes.c_int
    lib.rsa_softmax_sample.argtypes = [ctypes.POINTER(nat.SoftmaxSampleArgs), ctypes.c_void_p]
    lib.rsa_softmax_sample_workspace_bytes.restype = ctypes.c_int64
    lib.rsa_softmax_sample_workspace_bytes.argtypes = [ctypes.c_int64, ctypes.c_int64]
    lib.rsa_softmax_sample_block.restype = ctypes.c_int32

    def sample(item_vector, query, n, hist=None):
        a, out, keep = ops._softmax_sample_args(item_vector, query, n, 1.0, 0, None, hist, False, True, 'variant softmax_sample')
        a.workspace_bytes = lib.rsa_softmax_sample_workspace_bytes(a.n_query, a.n_items)
        ws = torch.empty(max(int(a.workspace_bytes), 8), dtype=torch.uint8, device=query.device)
        a.workspace = nat.ptr(ws)
        if n:
            pc = rng.reserve(a.n_query * n * 2, 4, query.device, None)
            a.seed, a.offset, a.grid_threads, a.elem_base = pc.seed, pc.offset, pc.grid_threads, pc.elem_base
        rc = lib.rsa_softmax_sample(ctypes.byref(a), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        if rc != 0:
            raise RuntimeError(f'variant rsa_softmax_sample: status {rc}')
        return out
    return sample, int(lib.rsa_softmax_sample_block())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--items', type=int, default=1_000_000)
    ap.add_argument('--big-items', type=int, default=10_000_000)
    ap.add_argument('--dim', type=int, default=128)
    ap.add_argument('--queries', type=int, default=2048)
    ap.add_argument('--neg', type=int, default=64)
    ap.add_argument('--hist', type=int, default=100)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--variant-libs', default='', help='G=PATH,... other builds of librecstudio_amd.so (-DRSA_SS_G=G)')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'softmax_sample_bench.json'))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_softmax_sample.py measures on the GPU: none found')
    from recstudio_amd import ops
    dev = 'cuda'
    N, d, B, n, L = a.items, a.dim, a.queries, a.neg, a.hist
    torch.manual_seed(0)
    G = ops.softmax_sample_block()
    res = dict(device=torch.cuda.get_device_name(0), items=N, dim=d, queries=B, num_neg=n, hist_len=L, reps=a.reps, block_items=G,
               score_matrix_bytes=4 * B * N)

    def setup(n_items):
        weight = torch.randn(n_items + 1, d, device=dev) * 0.3
        weight[0] = 0
        return weight, torch.randn(B, d, device=dev) * 0.3, torch.randint(1, n_items + 1, (B, L), device=dev)
    weight, q, hist = setup(N)
    X = weight[1:]

    # ---- the streaming path next to the torch path
    res['brute'] = {}
    for name, h in (('no_history', None), ('history', hist)):
        s_t, t_t = timed([lambda: ops.softmax_sample(X, q, n, user_hist=h, items_without_pad=True),
                          lambda: torch_brute(X, q, n, h)], a.reps)
        s_t['peak_bytes'] = peak_bytes(lambda: ops.softmax_sample(X, q, n, user_hist=h, items_without_pad=True))
        t_t['peak_bytes'] = peak_bytes(lambda: torch_brute(X, q, n, h))
        res['brute'][name] = dict(stream=s_t, torch=t_t, speedup=t_t['ms'] / s_t['ms'], peak_ratio=t_t['peak_bytes'] / s_t['peak_bytes'])
    torch.cuda.empty_cache()

    # ---- the block pass next to its floor
    b_t, l_t = timed([lambda: ops.softmax_sample(X, q, 0, items_without_pad=True),
                      lambda: ops.fullscore(X, q, want_lse=True, items_without_pad=True)], a.reps)
    flop = 2.0 * B * N * d
    res['block_pass'] = dict(block_pass_and_merge=b_t, fullscore_lse=l_t, lse_floor_fraction=l_t['ms'] / b_t['ms'],
                             block_pass_tflops=flop / b_t['ms'] / 1e9, fullscore_lse_tflops=flop / l_t['ms'] / 1e9)

    # ---- other block sizes
    variants = []
    if a.variant_libs:
        fns, names = [lambda: ops.softmax_sample(X, q, n, items_without_pad=True),
                      lambda: ops.softmax_sample(X, q, n, user_hist=hist, items_without_pad=True),
                      lambda: ops.softmax_sample(X, q, 0, items_without_pad=True)], [(G, 'no_history'), (G, 'history'), (G, 'block_pass')]
        for spec in a.variant_libs.split(','):
            g, path = spec.split('=', 1)
            sample, g_lib = variant_sampler(path)
            assert g_lib == int(g), (g_lib, g)
            variants.append((g_lib, sample))
            fns += [lambda s=sample: s(X, q, n), lambda s=sample: s(X, q, n, hist), lambda s=sample: s(X, q, 0)]
            names += [(g_lib, 'no_history'), (g_lib, 'history'), (g_lib, 'block_pass')]
        out = {}
        for (g, what), t in zip(names, timed(fns, a.reps)):
            out.setdefault(f'G={g}', {})[what] = t
        for g in out:
            out[g]['table_bytes'] = 16 * B * ((N + int(g[2:]) - 1) // int(g[2:]))
        res['block_size'] = out

    # ---- the headline catalog: the streaming path alone; the torch path cannot allocate
    del weight, X, q, hist
    torch.cuda.empty_cache()
    Nb = a.big_items
    weight, q, hist = setup(Nb)
    X = weight[1:]
    big = dict(items=Nb, score_matrix_bytes=4 * B * Nb)
    (big['no_history'], big['history']) = timed([lambda: ops.softmax_sample(X, q, n, items_without_pad=True),
                                                 lambda: ops.softmax_sample(X, q, n, user_hist=hist, items_without_pad=True)], a.reps)
    big['history']['peak_bytes'] = peak_bytes(lambda: ops.softmax_sample(X, q, n, user_hist=hist, items_without_pad=True))
    for g, sample in variants:
        t0, t1 = timed([lambda: sample(X, q, n), lambda: sample(X, q, n, hist)], a.reps)
        big[f'G={g}'] = dict(no_history=t0, history=t1)
    try:
        torch_brute(X, q, n, hist)
        torch.cuda.synchronize()
        big['torch'] = 'ran'
    except torch.OutOfMemoryError as e:
        big['torch'] = 'OutOfMemoryError: ' + str(e).split('.')[0]
    res['big'] = big
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')
    print(json.dumps(res))


if __name__ == '__main__':
    main()
