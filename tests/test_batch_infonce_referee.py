"""CPU: data_augmentation.batch_infonce_torch (the reference's op sequence for the in-batch InfoNCE) in float64 against the explicit
rule of tests/batch_infonce_referee.py to 1e-12, forward and backward; the seeded mistakes; BatchInfoNCELoss; and InfoNCELoss's own
batch modes, which still raise."""
import pytest
import torch

import batch_infonce_referee as br

SHAPES = [(1, 32), (2, 32), (31, 64), (33, 64), (65, 128), (40, 48)]


@pytest.fixture(scope='module')
def da():
    from recstudio_amd import data_augmentation
    return data_augmentation


def views(B, d, seed, scale=0.5):
    g = torch.Generator().manual_seed(seed)
    zi = torch.randn(B, d, generator=g, dtype=torch.float64) * scale
    zj = zi + 0.3 * torch.randn(B, d, generator=g, dtype=torch.float64) * scale
    return zi, zj, torch.rand(B, generator=g, dtype=torch.float64) + 0.5


def label_sets(B, seed):
    g = torch.Generator().manual_seed(seed)
    return {'absent': None, 'equal': torch.full((B,), 3), 'distinct': torch.randperm(B, generator=g) + 10,
            'repeats': torch.randint(0, max(B // 3, 1), (B,), generator=g)}


def twin64(da, zi, zj, inv_t, both, labels, g):
    zi, zj = zi.clone().requires_grad_(True), zj.clone().requires_grad_(True)
    rows = da.batch_infonce_torch(zi, zj, inv_t, both, labels)
    rows.backward(g)
    return rows.detach(), zi.grad, zj.grad


def close(a, b, tol=1e-12):
    assert float((a - b).abs().max()) <= tol * max(1.0, float(b.abs().max())), float((a - b).abs().max())


@pytest.mark.parametrize('both', [True, False], ids=['batch_both', 'batch_single'])
@pytest.mark.parametrize('B,d', SHAPES)
def test_twin_equals_the_rule(da, B, d, both):
    zi, zj, g = views(B, d, 7 * B + d)
    for inv_t in (1.0, 1 / 0.2):
        for name, labels in label_sets(B, B).items():
            rows, dzi, dzj = twin64(da, zi, zj, inv_t, both, labels, g)
            want = br.rule(zi, zj, inv_t, both, labels, g)
            close(rows, want['lse'] - want['pos'])
            close(dzi, want['dzi'])
            close(dzj, want['dzj'])
            if name == 'equal' and not both:
                close(want['lse'], want['pos'])                     # the positive alone is left
            if name == 'distinct':
                base = br.rule(zi, zj, inv_t, both, None, g)
                assert all(torch.equal(base[k], want[k]) for k in base)
    if B == 1:
        close(want['lse'], want['pos'])


def test_normalised_rows_at_a_low_temperature(da):
    """Scores spanning +-20: the running maximum matters."""
    zi, zj, g = views(64, 64, 3)
    zi, zj = torch.nn.functional.normalize(zi, dim=-1), torch.nn.functional.normalize(zj, dim=-1)
    rows, dzi, dzj = twin64(da, zi, zj, 20.0, True, None, g)
    want = br.rule(zi, zj, 20.0, True, None, g)
    assert float((zi @ zj.T).diagonal().min()) * 20 > 15
    close(rows, want['lse'] - want['pos'])
    close(dzi, want['dzi'])
    close(dzj, want['dzj'])


@pytest.fixture(scope='module')
def allow():
    return br.allowance('cpu')


GPU_SHAPES = [(1, 32), (2, 32), (31, 64), (32, 64), (33, 64), (65, 128), (257, 32), (300, 128)]


@pytest.mark.parametrize('both', [True, False], ids=['batch_both', 'batch_single'])
@pytest.mark.parametrize('B,d', GPU_SHAPES)
def test_fp32_emulation_stays_inside_half_of_every_bound(allow, B, d, both):
    """The kernel's tile order in fp32 (batch_infonce_referee.emulate_fp32) at the shapes of the GPU test."""
    zi, zj, g = views(B, d, 3 * B + d, scale=0.3)
    zi, zj, g = zi.float(), zj.float(), g.float()
    for inv_t, lab in ((1.0, None), (1 / 0.2, label_sets(B, 2)['repeats'])):
        ref = br.judge(zi, zj, inv_t, both, lab, g, allow)
        worst = br.shares(br.emulate_fp32(zi, zj, inv_t, both, lab, g), ref)
        assert set(worst) == set(br.NAMES) and all(v <= 0.5 for v in worst.values()), worst
    zi, zj = torch.nn.functional.normalize(zi, dim=-1), torch.nn.functional.normalize(zj, dim=-1)
    ref = br.judge(zi, zj, 20.0, both, None, g, allow)                      # temperature 0.05: the running maximum matters
    worst = br.shares(br.emulate_fp32(zi, zj, 20.0, both, None, g), ref)
    assert all(v <= 0.5 for v in worst.values()), worst


def test_seeded_mistakes_leave_a_bound(da, allow):
    B, d, inv_t = 33, 64, 1 / 0.5
    zi, zj, g = views(B, d, 11, scale=0.12)                                # scores of order 1: every logit carries weight
    zi, zj, g = zi.float(), zj.float(), g.float()
    labels = label_sets(B, 5)['repeats']
    assert int((labels.view(-1, 1) == labels.view(1, -1)).sum()) > B          # there are repeats
    for mistake in br.MISTAKES:
        both = mistake != 'single_with_ii'
        ref = br.judge(zi, zj, inv_t, both, labels, g, allow)
        bad = br.rule(zi, zj, inv_t, both, labels, g, mistake=mistake)
        worst = br.shares(bad, ref)
        assert max(worst.values()) > 1.0, (mistake, worst)
        # and the twin, in fp32, is inside every bound
        rows, dzi, dzj = twin64(da, zi, zj, inv_t, both, labels, g)
        got = dict(dzi=dzi, dzj=dzj)
        assert all(v <= 1.0 for v in br.shares(got, ref).values())
        assert bool(((rows.double() - (ref['lse'] - ref['pos'])).abs() <= ref['tol_lse'] + ref['tol_pos'] + 2 * br.U * ref['lse'].abs()).all())


def test_kernel_argument_validation_runs_before_any_device_call():
    import ctypes
    from recstudio_amd import _native as nat, ops
    lib = nat.lib()
    p, q, r, t = (ctypes.c_void_p(v) for v in (64, 128, 256, 512))

    def args(**kw):
        a = nat.BatchInfoNceArgs()
        a.zi, a.zj, a.lse, a.pos, a.g, a.dzi, a.dzj = p, q, r, r, r, t, ctypes.c_void_p(1024)
        a.n_rows, a.d, a.both, a.inv_t = 5, 64, 1, 1.0
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    for fn in (lib.rsa_batch_infonce, lib.rsa_batch_infonce_backward):
        for kw, msg in ((dict(d=48), b'd must be'), (dict(n_rows=-1), b'n_rows'), (dict(inv_t=0.0), b'inv_t'), (dict(zi=None), b'null'),
                        (dict(zj=None), b'null'), (dict(zi=ctypes.c_void_p(68)), b'aligned'), (dict(lse=None), b'lse is null'), (dict(size=0), b'size')):
            assert fn(ctypes.byref(args(**kw)), None) == -1, kw
            assert msg in lib.rsa_last_error(), (kw, lib.rsa_last_error())
        assert fn(None, None) == -1 and b'args is null' in lib.rsa_last_error()
        assert fn(ctypes.byref(args(n_rows=0, zi=None)), None) == 0
    assert lib.rsa_batch_infonce(ctypes.byref(args(pos=None)), None) == -1 and b'pos is null' in lib.rsa_last_error()
    for kw in (dict(g=None), dict(dzi=None), dict(dzj=None)):
        assert lib.rsa_batch_infonce_backward(ctypes.byref(args(**kw)), None) == -1 and b'null' in lib.rsa_last_error()
    for kw in (dict(dzi=p), dict(dzj=q), dict(dzj=t)):
        assert lib.rsa_batch_infonce_backward(ctypes.byref(args(**kw)), None) == -1 and b'alias' in lib.rsa_last_error()
    z = torch.zeros(4, 48)
    with pytest.raises(RuntimeError, match='GPU only'):
        ops.batch_infonce(z, z, 1.0)
    from recstudio_amd import data_augmentation as da
    assert not da.batch_infonce_kernel_ok(z, z)
    assert torch.equal(da.batch_infonce(z, z, 1.0), da.batch_infonce_torch(z, z, 1.0))      # CPU tensors: the twin


def test_loss_class(da):
    zi, zj, _ = views(20, 32, 2)
    zi, zj = zi.float(), zj.float()
    labels = label_sets(20, 1)['repeats']
    for neg_type, both in (('batch_both', True), ('batch_single', False)):
        for sim in ('inner_product', 'cosine'):
            fn = da.BatchInfoNCELoss(0.5, sim, neg_type)
            a, b = (torch.nn.functional.normalize(z, dim=-1) for z in (zi, zj)) if sim == 'cosine' else (zi, zj)
            for lab in (None, labels):
                got = fn(zi, zj, instance_labels=lab)
                assert abs(float(got) - br.loss(a, b, 2.0, both, lab)) <= 1e-5
    assert da.BatchInfoNCELoss().neg_type == 'batch_both' and da.BatchInfoNCELoss().temperature == 1.0
    for kw, msg in ((dict(neg_type='all'), 'neg_type'), (dict(sim_method='dot'), 'sim_method'), (dict(temperature=0.0), 'temperature')):
        with pytest.raises(ValueError, match=msg):
            da.BatchInfoNCELoss(**kw)
    fn = da.BatchInfoNCELoss()
    with pytest.raises(ValueError, match='all_reps'):
        fn(zi, zj, all_reps=zi)
    with pytest.raises(ValueError, match='one shape'):
        fn(zi, zj[:5])
    with pytest.raises(ValueError, match='one label per row'):
        fn(zi, zj, instance_labels=labels[:5])


def test_info_nce_loss_batch_modes_still_raise(da):
    zi, zj, _ = views(4, 8, 1)
    for neg_type in ('batch_both', 'batch_single'):
        with pytest.raises(NotImplementedError, match='sequence models'):
            da.InfoNCELoss(neg_type=neg_type)(zi, zj)
