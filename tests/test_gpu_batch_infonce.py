"""GPU: ops.batch_infonce / ops.batch_infonce_backward (rsa_infonce.hip) against the float64 rule and the per-element bounds of
tests/batch_infonce_referee.py: every element of lse, pos, dzi and dzj within its bound; bit-equal runs; peak memory; the autograd
node against the twin on the device."""
import pytest
import torch
import torch.nn.functional as F

import batch_infonce_referee as br

pytestmark = pytest.mark.gpu
DEV = 'cuda'
SHAPES = [(1, 32), (2, 32), (31, 64), (32, 64), (33, 64), (65, 128), (257, 32), (300, 128)]
WORST = {}


@pytest.fixture(scope='module')
def ra():
    import recstudio_amd
    recstudio_amd._native.lib()
    torch.cuda.init()
    return recstudio_amd


@pytest.fixture(scope='module')
def allow(ra):
    a = br.allowance(DEV)
    print(f"device exp: worst relative error {a['measured'][0]:.3e}, log: worst absolute error {a['measured'][1]:.3e}")
    return a


def views(B, d, seed, scale=0.3):
    g = torch.Generator().manual_seed(seed)
    zi = torch.randn(B, d, generator=g) * scale
    zj = zi + 0.3 * torch.randn(B, d, generator=g) * scale
    return zi, zj, torch.rand(B, generator=g) + 0.5


def label_sets(B, seed):
    g = torch.Generator().manual_seed(seed)
    return {'absent': None, 'equal': torch.full((B,), 3), 'distinct': torch.randperm(B, generator=g) + 10,
            'repeats': torch.randint(0, max(B // 3, 1), (B,), generator=g)}


def run(ra, zi, zj, inv_t, both, labels, g):
    zi, zj, g = zi.to(DEV), zj.to(DEV), g.to(DEV)
    labels = None if labels is None else labels.to(DEV)
    lse, pos = ra.ops.batch_infonce(zi, zj, inv_t, both, labels)
    dzi, dzj = ra.ops.batch_infonce_backward(zi, zj, inv_t, both, labels, lse, g)
    return dict(lse=lse, pos=pos, dzi=dzi, dzj=dzj)


def judge(ra, allow, zi, zj, inv_t, both, labels, g, tag):
    got = run(ra, zi, zj, inv_t, both, labels, g)
    ref = br.judge(zi, zj, inv_t, both, labels, g, allow)
    worst = br.shares(got, ref)
    print(f'{tag}: worst share of each bound {({k: round(v, 3) for k, v in worst.items()})}')
    for k, v in worst.items():
        WORST[k] = max(WORST.get(k, 0.0), v)
    assert all(bool(torch.isfinite(got[k]).all()) for k in got) and all(v <= 1.0 for v in worst.values()), (tag, worst)
    return got, ref


@pytest.mark.parametrize('both', [True, False], ids=['batch_both', 'batch_single'])
@pytest.mark.parametrize('B,d', SHAPES)
def test_every_element_within_its_bound(ra, allow, B, d, both):
    zi, zj, g = views(B, d, 3 * B + d)
    outs = {}
    for name, labels in label_sets(B, 2).items():
        for inv_t in (1.0, 1 / 0.2):
            got, ref = judge(ra, allow, zi, zj, inv_t, both, labels, g, f'B {B}, d {d}, both {both}, labels {name}, inv_t {inv_t}')
            outs[name, inv_t] = got
            if name == 'equal':                                            # the positive alone is left
                assert bool(((got['lse'].cpu().double() - ref['pos']).abs() <= ref['tol_lse'] + ref['tol_pos']).all())
    for inv_t in (1.0, 1 / 0.2):                                           # all distinct == absent, bit for bit
        assert all(torch.equal(outs['distinct', inv_t][k], outs['absent', inv_t][k]) for k in br.NAMES)
    again = run(ra, zi, zj, 1.0, both, label_sets(B, 2)['repeats'], g)      # two runs bit-equal
    assert all(torch.equal(again[k], outs['repeats', 1.0][k]) for k in br.NAMES)
    if B == 1:
        assert torch.equal(outs['absent', 1.0]['lse'], outs['absent', 1.0]['pos'])   # the positive alone: lse = m + log(1)


@pytest.mark.parametrize('both', [True, False], ids=['batch_both', 'batch_single'])
def test_normalised_rows_at_temperature_0_05(ra, allow, both):
    """Scores span +-20: the running maximum matters."""
    zi, zj, g = views(257, 64, 5)
    zi, zj = torch.nn.functional.normalize(zi, dim=-1), torch.nn.functional.normalize(zj, dim=-1)
    got, ref = judge(ra, allow, zi, zj, 20.0, both, None, g, f'normalised rows, inv_t 20, both {both}')
    assert float(ref['pos'].max()) > 15 and float((zi @ zi.T).min()) * 20 < -5


def test_worst_shares(ra):
    """(runs after the cases above) the worst share of each bound over all of them."""
    print('worst share of each bound over all cases:', {k: round(v, 3) for k, v in WORST.items()})
    assert all(v <= 1.0 for v in WORST.values())


def test_peak_memory(ra):
    """B = 2048, d = 64, where one [B, 2B] matrix is 32 MiB: the forward allocates lse + pos (+ 1 MiB), the backward dzi + dzj (+ 1 MiB)."""
    B, d = 2048, 64
    zi, zj, g = (t.to(DEV) for t in views(B, d, 9))
    ra.ops.batch_infonce(zi, zj, 1.0, True)                                 # (warm: lazily loaded code objects)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    lse, pos = ra.ops.batch_infonce(zi, zj, 1.0, True)
    torch.cuda.synchronize()
    fwd = torch.cuda.max_memory_allocated() - before
    assert fwd <= 2 * B * 4 + (1 << 20), fwd
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    dzi, dzj = ra.ops.batch_infonce_backward(zi, zj, 1.0, True, None, lse, g)
    torch.cuda.synchronize()
    bwd = torch.cuda.max_memory_allocated() - before
    assert bwd <= 2 * B * d * 4 + (1 << 20), bwd
    print(f'peak above the inputs: forward {fwd} bytes, backward {bwd} bytes (one [B, 2B] matrix: {B * 2 * B * 4})')


@pytest.mark.parametrize('sim', ['inner_product', 'cosine'])
@pytest.mark.parametrize('neg_type', ['batch_both', 'batch_single'])
def test_autograd_node_against_the_twin(ra, neg_type, sim):
    """BatchInfoNCELoss(fused=True) against fused=False on the device and against float64: 1e-4 on the loss, 3e-4 on the gradients (the
    parity contract), with the kernel's derived per-element bound as the absolute term."""
    da = ra.data_augmentation
    zi, zj, _ = views(300, 64, 13)
    labels = label_sets(300, 4)['repeats'].to(DEV)
    for lab in (None, labels):
        runs = []
        for fused, dev, dt in ((True, DEV, torch.float32), (False, DEV, torch.float32), (False, 'cpu', torch.float64)):
            a, b = zi.to(dev, dt).requires_grad_(True), zj.to(dev, dt).requires_grad_(True)
            loss = da.BatchInfoNCELoss(0.5, sim, neg_type, fused=fused)(a, b, instance_labels=None if lab is None else lab.to(dev))
            loss.backward()
            runs.append((float(loss.detach()), a.grad.double().cpu(), b.grad.double().cpu()))
        (l1, ga1, gb1), (l2, ga2, gb2), (l64, ga64, gb64) = runs
        assert abs(l1 - l2) <= 1e-4 * abs(l2) and abs(l1 - l64) <= 1e-4 * abs(l64)
        # The absolute allowance for the elements that cancel is the kernel's own derived bound (batch_infonce_referee.judge, at the
        # kernel's inputs and g = 1 / B), carried through F.normalize's backward |J| for 'cosine', J_b = (I - n_b n_b^T) / ||z_b||.
        # (A flat 3e-4 / 100 of the largest gradient, 8.0e-9 here, is less than fp32 guarantees for a 600-term sum whose terms add up to
        # 1.6e-3: (n + 2) u sum|terms| = 5.8e-8.  Measured at the worst such element: kernel 1.5e-8 off float64, the twin 4e-9.)
        B = zi.shape[0]
        ki, kj = (F.normalize(z, dim=-1) for z in (zi, zj)) if sim == 'cosine' else (zi, zj)
        ref = br.judge(ki, kj, 2.0, neg_type == 'batch_both', lab, torch.full((B,), 1.0 / B), br.allowance(DEV))
        tols = []
        for z, tol in ((zi, ref['tol_dzi']), (zj, ref['tol_dzj'])):
            if sim == 'cosine':
                n, norm = F.normalize(z.double(), dim=-1), z.double().norm(dim=-1)
                J = (torch.eye(z.shape[1], dtype=torch.float64).unsqueeze(0) - n.unsqueeze(2) * n.unsqueeze(1)).abs() / norm.view(-1, 1, 1)
                tol = torch.einsum('bcd,bd->bc', J, tol)
            tols.append(tol)
        for got, twin, r64, tol in ((ga1, ga2, ga64, tols[0]), (gb1, gb2, gb64, tols[1])):
            print(f'{neg_type} {sim}: twin off float64 by {float((twin - r64).abs().max()):.3e}, fused by {float((got - r64).abs().max()):.3e}, '
                  f'fused - twin {float((got - twin).abs().max()):.3e}; largest gradient {float(r64.abs().max()):.3e}')
            assert bool(((got - r64).abs() <= 3e-4 * r64.abs() + tol).all())
            assert bool(((got - twin).abs() <= 3e-4 * twin.abs() + tol + (twin - r64).abs()).all())
    z48 = torch.randn(10, 48, device=DEV)                                   # another width: the twin
    assert torch.equal(da.batch_infonce(z48, z48, 1.0), da.batch_infonce_torch(z48, z48, 1.0))
    with pytest.raises(ValueError, match='d must be'):
        ra.ops.batch_infonce(z48, z48, 1.0)
