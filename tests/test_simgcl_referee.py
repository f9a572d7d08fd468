"""CPU: the referee of the SimGCL feature (tests/simgcl_referee.py) against dense constructions, the fp32 emulation inside its
bounds and every seeded mistake outside them, the inputs of the GPU tests under the sign-ambiguity cap, the argument checks of the
perturbed rsa_spmm_csr (they run before any HIP call) and the settings SimGCL takes and refuses.  No device kernel runs here."""
import ctypes

import numpy as np
import pytest
import torch

import simgcl_referee as sc
import spmm_referee as sr

NU, NI, D, CHUNK, EPS = 41, 61, 16, 8, 0.1
N = NU + NI
CAP = 1e-4          # the largest share of sign-ambiguous elements among rows with edges


@pytest.fixture(scope='module')
def ra():
    import recstudio_amd
    from recstudio_amd import _native
    import os
    if not os.path.exists(_native.LIB_PATH):
        _native.build()
    return recstudio_amd


@pytest.fixture(scope='module')
def small(ra):
    users, items = sr.random_bipartite(NU, NI, 400, seed=7)
    return ra.TripletDataset.from_mapped_ids(users, items, n_users=NU, n_items=NI)


@pytest.fixture(scope='module')
def adj(ra, small):
    return ra.graphmodule.NormAdj.from_dataset(small, chunk=CHUNK)


@pytest.fixture(scope='module')
def inputs(adj):
    """(e0, [view 1's L uniform tables, view 2's]): shared by the tests below, never written to."""
    e0 = torch.cat(sc.tables(NU, NI, D, seed=3), 0)
    g = torch.Generator().manual_seed(4)
    return e0, [[torch.rand(N, D, generator=g) for _ in range(3)] for _ in range(2)]


def csr(adj):
    return adj.indptr, adj.indices, adj.values


def test_the_graph_has_split_rows_and_rows_without_edges(adj):
    deg = adj.indptr[1:] - adj.indptr[:-1]
    assert int((deg > CHUNK).sum()) > 0 and int((deg == 0).sum()) >= 2 and adj.plan.n_split > 0


@pytest.mark.parametrize('n_layers', [1, 2, 3])
@pytest.mark.parametrize('perturbed', [False, True])
def test_emulation_stays_inside_the_bounds(adj, inputs, n_layers, perturbed):
    e0, (u1, _) = inputs
    uniforms = u1[:n_layers] if perturbed else None
    layers, mean = sc.emulate_propagation(*csr(adj), e0, CHUNK, n_layers, uniforms, EPS)
    j = sc.judge_propagation(*csr(adj), e0, layers, mean, uniforms, EPS)
    print(n_layers, perturbed, j)
    assert j['ratio'] <= 1.0 and j['mean_ratio'] <= 1.0 and j['share'] <= CAP
    deg = adj.indptr[1:] - adj.indptr[:-1]
    assert all(bool((y[deg == 0] == 0).all()) for y in layers)                       # rows without edges stay exactly 0
    if perturbed:                                                                    # the perturbation is there: eps along a unit vector
        plain, _ = sc.emulate_propagation(*csr(adj), e0, CHUNK, 1)
        moved = (layers[0] - plain[0]).double().norm(dim=-1)[deg > 0]
        assert bool(((moved - EPS).abs() < 1e-5).all())


def test_emulation_agrees_with_the_dense_float64_mean(adj, inputs):
    e0, (u1, _) = inputs
    dense = sr.csr_dense(*csr(adj), N)
    for uniforms in (None, u1):
        _, mean = sc.emulate_propagation(*csr(adj), e0, CHUNK, 3, uniforms, EPS)
        want = sc.perturbed_mean(dense, e0.double(), 3, float(np.float32(EPS)), uniforms)
        # (signs of near-zero sums aside, which the data of this test has none of, the two agree to fp32 accuracy)
        assert float((mean.double() - want).abs().max()) < 1e-6


@pytest.mark.parametrize('mistake', ['e0_in_mean', 'not_fed', 'copysign', 'table_norm', 'same_uniforms', 'centred', 'no_sign', 'per_piece'])
def test_seeded_forward_mistakes_leave_the_bounds(adj, inputs, mistake):
    e0, (u1, _) = inputs
    layers, mean = sc.emulate_propagation(*csr(adj), e0, CHUNK, 3, u1, EPS, mistake=mistake)
    j = sc.judge_propagation(*csr(adj), e0, layers, mean, u1, EPS)
    print(mistake, j)
    assert max(j['ratio'], j['mean_ratio']) > 1.0


def test_copysign_moves_a_row_without_edges(adj, inputs):
    e0, (u1, _) = inputs
    deg = adj.indptr[1:] - adj.indptr[:-1]
    y = sc.emulate_layer(*csr(adj), e0, CHUNK, u1[0], EPS, mistake='copysign')
    assert bool((y[deg == 0] != 0).any())
    assert bool((sc.emulate_layer(*csr(adj), e0, CHUNK, u1[0], EPS)[deg == 0] == 0).all())


def test_the_second_views_uniforms_are_not_the_first_views(adj, inputs):
    """An implementation that perturbs both views with the same uniforms: its second view judged with the second view's own."""
    e0, (u1, u2) = inputs
    layers, mean = sc.emulate_propagation(*csr(adj), e0, CHUNK, 3, u1, EPS)
    assert sc.judge_propagation(*csr(adj), e0, layers, mean, u2, EPS)['ratio'] > 1.0


def test_an_ambiguous_sign_is_accepted_either_way_and_counted():
    """One row of two edges whose exact sum is far inside its own rounding error: +dl, -dl and 0 all pass, 2 dl off does not."""
    indptr, indices = torch.tensor([0, 2]), torch.tensor([0, 1], dtype=torch.int32)
    x = torch.tensor([[1.0] * 4, [-1.0 + 2.0 ** -24] * 4])
    u = torch.full((1, 4), 0.5)
    ref = sc.layer(indptr, indices, None, x, u, EPS)
    s, dl = ref['s'], ref['dl']
    assert abs(float(dl[0, 0]) - float(np.float32(EPS)) / 2) < 1e-12
    for sgn in (1.0, -1.0, 0.0):
        j = sc.judge(ref, got_y=(s + sgn * dl).float())
        assert j['ratio'] <= 1.0 and j['n_ambiguous'] == 4 and j['share'] == 1.0
    assert sc.judge(ref, got_y=(s + 2 * dl).float())['ratio'] > 1.0
    clear = sc.layer(indptr, indices, None, torch.tensor([[1.0] * 4, [0.5] * 4]), u, EPS)
    assert sc.judge(clear, got_y=(clear['s'] + clear['dl']).float())['ratio'] <= 1.0
    j = sc.judge(clear, got_y=(clear['s'] - clear['dl']).float())
    assert j['ratio'] > 1.0 and j['n_ambiguous'] == 0


@pytest.mark.parametrize('d', [4, 36, 64, 128, 256])
def test_kernel_test_inputs_stay_under_the_ambiguity_cap(d):
    c = sc.ragged_case(d)
    for row_scale in (None, c['row_scale']):
        assert sc.ambiguous_share(c['indptr'], c['indices'], c['values'], c['x'], row_scale) <= CAP
    lengths = c['indptr'][1:] - c['indptr'][:-1]
    assert set([0, 1, 7, 8, 9, 16, 17]) <= set(lengths.tolist()) and int(lengths[-1]) * 2 == int(c['indptr'][-1])


@pytest.mark.parametrize('d', [4, 64, 128, 256])
def test_propagation_test_inputs_stay_under_the_ambiguity_cap(adj, d):
    """The float64 layers of the tables tests/test_gpu_simgcl.py propagates (unperturbed and perturbed data differ by eps only)."""
    x = torch.cat(sc.tables(NU, NI, d, seed=3), 0)
    for _ in range(3):
        assert sc.ambiguous_share(*csr(adj), x) <= CAP
        x = sr.referee(*csr(adj), x)['y'].float()


@pytest.mark.parametrize('n_layers', [1, 2, 3])
@pytest.mark.parametrize('symmetric', [True, False])
def test_gradient_referee_and_lightgcns_backward(ra, adj, inputs, n_layers, symmetric):
    e0, (u1, _) = inputs
    if symmetric:
        a = adj
    else:
        g = torch.Generator().manual_seed(9)
        a = ra.graphmodule.NormAdj(torch.randint(0, N, (700,), generator=g), torch.randint(0, N, (700,), generator=g), N, chunk=CHUNK)
        assert not a.symmetric
    dense = sr.csr_dense(a.indptr, a.indices, a.values, N)
    up = torch.randn(N, D, generator=torch.Generator().manual_seed(10))
    for uniforms in (None, u1):
        e64 = e0.double().requires_grad_(True)
        sc.perturbed_mean(dense, e64, n_layers, EPS, uniforms).backward(up.double())
        want, tol = sc.propagate_grad(a.t_indptr, a.t_indices, a.t_values, up, n_layers)
        np.testing.assert_allclose(want.numpy(), e64.grad.numpy(), rtol=1e-12, atol=1e-14)      # the noise does not enter the gradient
    wrong, _ = sc.propagate_grad(a.t_indptr, a.t_indices, a.t_values, up, n_layers, mistake='lightgcn')
    assert sr.ratio(wrong, want, tol) > 1.0
    if not symmetric:                                                                # and the untransposed matrix is caught too
        other, _ = sc.propagate_grad(a.indptr, a.indices, a.values, up, n_layers)
        assert sr.ratio(other, want, tol) > 1.0


def test_step_referee_adds_the_contrast_with_weight_one(adj, inputs):
    e0, (u1, u2) = inputs
    g = torch.Generator().manual_seed(2)
    ue, ie = e0[:NU], e0[NU:]
    uid, pos, neg = torch.randint(1, NU, (8,), generator=g), torch.randint(1, NI, (8,), generator=g), torch.randint(1, NI, (8, 2), generator=g)
    dense = sr.csr_dense(*csr(adj), N)
    out = sc.simgcl_step(ue, ie, dense, 2, EPS, uid, pos, neg, u1[:2], u2[:2], 1e-4, 0.2)
    # the BPR + l2 part is LightGCN's on the skip-input mean: rebuild it from the returned tables
    q = out['users'][uid]
    ps, ns = (q * out['items'][pos]).sum(-1), (q.unsqueeze(1) * out['items'][neg]).sum(-1)
    bpr = -torch.nn.functional.logsigmoid(ps.view(-1, 1) - ns).mean(-1).mean()
    reg = sr.l2_reg(ue[uid].double(), ie[pos].double(), ie[neg.reshape(-1)].double())
    assert abs(float(out['loss'] - bpr - 1e-4 * reg - out['cl_loss'])) < 1e-12 and float(out['cl_loss']) > 0
    want = sc.perturbed_mean(dense, e0.double(), 2, EPS)
    assert torch.allclose(torch.cat([out['users'], out['items']]), (dense @ e0.double() + dense @ (dense @ e0.double())) / 2, rtol=0, atol=1e-15)
    assert torch.equal(torch.cat([out['users'], out['items']]), want)
    same = sc.simgcl_step(ue, ie, dense, 2, EPS, uid, pos, neg, u1[:2], u1[:2], 1e-4, 0.2)
    assert abs(float(same['cl_loss'] - out['cl_loss'])) > 1e-3                       # the two views must not share their noise


def test_spmm_noise_argument_validation_runs_before_any_device_call(ra):
    nat = ra._native
    lib = nat.lib()
    fake = ctypes.c_void_p(1 << 20)                           # never dereferenced: every case below fails its checks

    def args(**kw):
        a = nat.SpmmArgs()
        a.indptr, a.indices, a.x, a.y = (fake,) * 4
        a.n_rows, a.n_cols, a.nnz, a.dim, a.chunk = 10, 10, 40, 64, 2048
        a.noise_eps, a.noise_grid_threads = 0.1, 512
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    def refused(a, text):
        assert lib.rsa_spmm_csr(ctypes.byref(a), None) == -1
        assert text in lib.rsa_last_error(), lib.rsa_last_error()

    refused(args(noise_eps=float('nan')), b'noise_eps must be finite')
    refused(args(noise_eps=float('inf')), b'noise_eps must be finite')
    refused(args(noise_grid_threads=0), b'bad philox state for the noise')
    refused(args(noise_grid_threads=300), b'bad philox state for the noise')
    refused(args(noise_offset=6), b'bad philox state for the noise')
    refused(args(noise_eps=0.0, noise_u=fake), b'noise_u without noise_eps')
    refused(args(noise_u=ctypes.c_void_p((1 << 20) + 4)), b'noise_u must be 16-byte aligned')
    # no noise: the block of before, whatever the other noise fields hold; an empty matrix returns before any launch
    assert lib.rsa_spmm_csr(ctypes.byref(args(n_rows=0, nnz=0)), None) == 0
    assert lib.rsa_spmm_csr(ctypes.byref(args(n_rows=0, nnz=0, noise_eps=0.0, noise_grid_threads=7)), None) == 0
    short = args(n_rows=0, nnz=0, noise_eps=float('nan'))
    short.size = nat.SpmmArgs.noise_eps.offset                # a caller built against the header of before: the tail is not read
    assert lib.rsa_spmm_csr(ctypes.byref(short), None) == 0
    assert nat.SpmmArgs.noise_eps.offset == nat.SpmmArgs.partials_bytes.offset + 8
    p = ra.ops.spmm_plan(torch.tensor([0, 1]))
    with pytest.raises(RuntimeError, match='GPU only'):
        ra.ops.spmm_csr(torch.tensor([0, 1]), torch.zeros(1, dtype=torch.int32), None, torch.zeros(1, 4), plan=p, noise_eps=0.1,
                        noise=ra.rng.PhiloxCall(1, 0, 256))


def test_simgcl_defaults_and_refusals(ra, small):
    m = ra.SimGCL({'train': {'seed': 1}})
    model, train = m.config['model'], m.config['train']
    assert (model['eps'], model['n_layers'], model['l2_reg_weight'], model['cl_neg_type'], model['temperature'], model['cl_weight']) == \
        (0.1, 3, 1e-4, 'all', 0.2, 0.5)
    assert (train['batch_size'], train['learning_rate'], train['early_stop_patience'], train['negative_count']) == (2048, 0.001, 100, 1)
    assert m.config['eval']['cutoff'] == [20, 10, 5]
    assert ra.SimGCL({'train': {'batch_size': 512}}).config['train']['batch_size'] == 512
    assert issubclass(ra.SimGCL, ra.LightGCN) and 'SimGCL' in ra.retriever.__all__
    m._init_model(small)
    net = m.SimGCLNet
    assert isinstance(net, ra.graphmodule.SimGCLNet) and (net.n_layers, net.eps) == (3, 0.1) and not hasattr(m, 'LightGCNNet')
    assert isinstance(m.augmentation_model, ra.data_augmentation.SimGCLAugmentation)
    for neg_type in ('batch_both', 'batch_single'):
        with pytest.raises(NotImplementedError, match='cl_neg_type'):
            ra.SimGCL({'model': {'cl_neg_type': neg_type}})._init_model(small)
    with pytest.raises(ValueError, match='n_layers'):
        ra.SimGCL({'model': {'n_layers': 0}})._init_model(small)
    with pytest.raises(ValueError, match='n_layers'):
        ra.graphmodule.SimGCLNet(0, 0.1)
    with pytest.raises(NotImplementedError, match='ANN'):
        ra.SimGCL({'train': {'ann': {'index': 'IVFx,Flat'}}})
