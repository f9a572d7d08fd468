"""CPU: the referee of the NGCF feature (tests/ngcf_referee.py) against nn.Linear / LeakyReLU / F.normalize / autograd in float64,
the fp32 emulation inside half its bounds and every seeded mistake outside them, the argument checks of rsa_bi_combine /
rsa_bi_combine_backward (they run before any HIP call) and BiCombiner's parameters.  No device kernel runs here."""
import ctypes

import pytest
import torch

import ngcf_referee as nr

F64 = torch.float64
SLOPE = 0.01
PARAMS = ('x', 'm', 'w1', 'b1', 'w2', 'b2')


@pytest.fixture(scope='module')
def nat():
    import os
    from recstudio_amd import _native
    if not os.path.exists(_native.LIB_PATH):
        _native.build()
    return _native


@pytest.fixture(scope='module', params=[(33, 4, 4, 0.0, 1), (97, 36, 20, 0.1, 2), (130, 64, 64, 0.1, 3), (65, 32, 64, 0.5, 4)], ids=str)
def case(request):
    N, d_in, d_out, p, seed = request.param
    inp = nr.layer_inputs(N, d_in, d_out, seed)
    args = [inp[k] for k in PARAMS]
    f = nr.layer_forward(*args, SLOPE, p, inp['u'])
    fb = nr.layer_forward_bounds(*args, f)
    b = nr.layer_backward(*args, f, inp['g_h'], inp['g_n'], SLOPE)
    bb = nr.layer_backward_bounds(*args, f, fb, b, inp['g_h'], inp['g_n'], SLOPE)
    return dict(inp=inp, args=args, p=p, f=f, fb=fb, b=b, bb=bb)


def torch_layer(inp, p, slope=SLOPE, variant=None):
    """The layer from torch.nn pieces in float64 under autograd -> (h, n, leaves)."""
    leaves = {k: inp[k].to(F64).requires_grad_() for k in PARAMS}
    x, m = leaves['x'], leaves['m']
    lin = torch.nn.functional.linear
    act = torch.nn.LeakyReLU(slope)
    q = nr.q_of(p)
    keep = (inp['u'].to(F64) < q) if p else torch.ones(x.shape[0], leaves['w1'].shape[0], dtype=torch.bool)
    drop = lambda v, scale=True: torch.where(keep, v / (q if scale else 1.0), torch.zeros_like(v)) if p else v     # noqa: E731
    if variant == 'act_after_sum':
        h = drop(act(lin(x + m, leaves['w1'], leaves['b1']) + lin(x * m, leaves['w2'], leaves['b2'])))
    elif variant == 'w2_on_sum':
        h = drop(act(lin(x + m, leaves['w1'], leaves['b1'])) + act(lin(x + m, leaves['w2'], leaves['b2'])))
    elif variant == 'no_bias':
        h = drop(act(lin(x + m, leaves['w1'], leaves['b1'])) + act(lin(x * m, leaves['w2'])))
    elif variant == 'no_rescale':
        h = drop(act(lin(x + m, leaves['w1'], leaves['b1'])) + act(lin(x * m, leaves['w2'], leaves['b2'])), scale=False)
    elif variant == 'dropout_first':          # the mask and 1 / q on the products, before bias and activation
        h = act(drop(lin(x + m, leaves['w1'])) + leaves['b1']) + act(drop(lin(x * m, leaves['w2'])) + leaves['b2'])
    else:
        h = drop(act(lin(x + m, leaves['w1'], leaves['b1'])) + act(lin(x * m, leaves['w2'], leaves['b2'])))
    return h, torch.nn.functional.normalize(h, dim=-1), leaves


def test_referee_equals_torch_modules(case):
    inp, p, f, b = case['inp'], case['p'], case['f'], case['b']
    h, n, leaves = torch_layer(inp, p)
    assert torch.allclose(f['h'], h, rtol=1e-13, atol=1e-15) and torch.allclose(f['n'], n, rtol=1e-13, atol=1e-15)
    ((h * inp['g_h'].to(F64)).sum() + (n * inp['g_n'].to(F64)).sum()).backward()
    for k, name in (('x', 'dx'), ('m', 'dm'), ('w1', 'dw1'), ('w2', 'dw2'), ('b1', 'db1'), ('b2', 'db2')):
        assert torch.allclose(b[name], leaves[k].grad, rtol=1e-11, atol=1e-13), name


def test_absent_gradients(case):
    inp, p = case['inp'], case['p']
    for gh, gn in ((inp['g_h'], None), (None, inp['g_n'])):
        h, n, leaves = torch_layer(inp, p)
        (((h * gh.to(F64)).sum() if gh is not None else 0) + ((n * gn.to(F64)).sum() if gn is not None else 0)).backward()
        b = nr.layer_backward(*case['args'], case['f'], gh, gn, SLOPE)
        for k, name in (('x', 'dx'), ('m', 'dm'), ('w1', 'dw1'), ('w2', 'dw2'), ('b1', 'db1'), ('b2', 'db2')):
            assert torch.allclose(b[name], leaves[k].grad, rtol=1e-11, atol=1e-13), name


def test_inputs_decide_every_slope(case):
    assert nr.preact_margin(case['f'], case['fb']) >= 2


def test_fp32_emulation_within_half_the_bound(case):
    inp, p, f, fb, b, bb = (case[k] for k in ('inp', 'p', 'f', 'fb', 'b', 'bb'))
    e = nr.layer_fp32(*case['args'], SLOPE, p, inp['u'], inp['g_h'], inp['g_n'])
    for name in ('h', 'n'):
        assert nr.worst(e[name], f[name], fb[name]) <= 0.5, name
    for name in ('dx', 'dm', 'dw1', 'dw2', 'db1', 'db2'):
        assert nr.worst(e[name], b[name], bb[name]) <= 0.5, name


@pytest.mark.parametrize('variant', ['act_after_sum', 'w2_on_sum', 'no_bias', 'no_rescale', 'dropout_first'])
def test_seeded_layer_mistakes_leave_the_bound(case, variant):
    inp, p, f, fb, b, bb = (case[k] for k in ('inp', 'p', 'f', 'fb', 'b', 'bb'))
    h, n, leaves = torch_layer(inp, p, variant=variant)
    if variant in ('no_rescale', 'dropout_first') and not p:          # without dropout there is nothing to get wrong
        assert nr.worst(h, f['h'], fb['h']) <= 1
        return
    assert nr.worst(h, f['h'], fb['h']) > 1
    if variant != 'no_rescale':                     # (the normalised block does not see a factor common to the row)
        assert nr.worst(n, f['n'], fb['n']) > 1
    ((h * inp['g_h'].to(F64)).sum() + (n * inp['g_n'].to(F64)).sum()).backward()
    assert nr.worst(leaves['x'].grad, b['dx'], bb['dx']) > 1
    assert nr.worst(leaves['w1'].grad, b['dw1'], bb['dw1']) > 1


# ---------------------------------------------------------------------------------------------------------------- the net
NU, NI, D = 23, 31, 8
NN = NU + NI


@pytest.fixture(scope='module')
def net():
    """A small non-symmetric thinned view of a bidirectional multigraph with an isolated node, two layers with dropout."""
    gen = torch.Generator().manual_seed(11)
    users, items = torch.randint(1, NU, (150,), generator=gen), torch.randint(1, NI, (150,), generator=gen) + NU
    dst, src = torch.cat([items, users]), torch.cat([users, items])
    keep = torch.rand(dst.numel(), generator=gen) < 0.8
    keep[src == src[0]] = False                                    # one node loses every out-edge and still receives
    x0 = (torch.rand(NN, D, generator=gen, dtype=F64) * 2 - 1)
    sizes = [D, 12, 4]
    layers = []
    for a, b in zip(sizes[:-1], sizes[1:]):
        layers.append(tuple((torch.rand(*s, generator=gen, dtype=F64) * 2 - 1) * a ** -0.5 for s in ((b, a), (b,), (b, a), (b,))))
    ps = [0.1, 0.5]
    us = [torch.rand(NN, b, generator=gen) for b in sizes[1:]]
    A = nr.left_adjacency(dst, src, NN, keep)
    return dict(dst=dst, src=src, keep=keep, x0=x0, layers=layers, ps=ps, us=us, A=A, sizes=sizes)


def net_table_and_grad(net, A, A_back=None, **kw):
    """(table, d sum(table * G) / d x0); ``A_back``: the matrix whose transpose the backward goes through (a seeded mistake)."""
    x0 = net['x0'].clone().requires_grad_()
    G = torch.rand(NN, sum(net['sizes']), generator=torch.Generator().manual_seed(5), dtype=F64) - 0.5
    if A_back is None:
        table = nr.net_forward(A, x0, net['layers'], SLOPE, net['ps'], net['us'], **kw)
    else:
        class Agg(torch.autograd.Function):
            @staticmethod
            def forward(ctx, x):
                return A @ x

            @staticmethod
            def backward(ctx, gy):
                return A_back.T @ gy
        table = nr.net_forward(_Mat(Agg), x0, net['layers'], SLOPE, net['ps'], net['us'], **kw)
    if table.shape[1] != G.shape[1]:
        return table, None
    (table * G).sum().backward()
    return table, x0.grad


class _Mat:
    """``_Mat(fn) @ x`` = fn.apply(x)."""

    def __init__(self, fn):
        self.fn = fn

    def __matmul__(self, x):
        return self.fn.apply(x)


def test_left_adjacency_is_the_documented_rule(net):
    dst, src, keep, A = net['dst'], net['src'], net['keep'], net['A']
    out_deg = torch.bincount(src[keep], minlength=NN).clamp_min(1).to(F64)
    x = net['x0']
    want = torch.zeros_like(x)
    for e in range(dst.numel()):
        if keep[e]:
            want[dst[e]] += x[src[e]] / out_deg[src[e]]
    assert torch.allclose(A @ x, want, rtol=1e-13, atol=1e-15)
    assert float((A @ x)[0].abs().max()) == 0 and float((A @ x)[NU].abs().max()) == 0          # the padding nodes have no edges
    assert not torch.equal(A, A.T)


def net_table_bound(net):
    """Per element of the true table, the layer bound of its block (ngcf_referee's header) from the float64 layer inputs; block 0
    is a copy of x_0 and has tolerance 0."""
    x, tols = net['x0'], [torch.zeros(NN, D, dtype=F64)]
    for (w1, b1, w2, b2), p, u in zip(net['layers'], net['ps'], net['us']):
        m = net['A'] @ x
        f = nr.layer_forward(x, m, w1, b1, w2, b2, SLOPE, p, u)
        tols.append(nr.layer_forward_bounds(x, m, w1, b1, w2, b2, f)['n'])
        x = f['h']
    return torch.cat(tols, 1)


@pytest.mark.parametrize('mistake', ['feed_normalised', 'both', 'base_degrees', 'zero_degree', 'no_input', 'untransposed'])
def test_seeded_net_mistakes_leave_the_bound(net, mistake):
    """The table of every mistake against the float64 net, judged with the layer bound of each block (`net_table_bound`: what a
    layer may be off by on exact inputs; the true net passes it trivially, being the referee).  The gradient with respect to x_0
    has no derived bound across layers: it is judged with 1e-3 of its largest element as a stand-in, three orders above any fp32
    error and as many below what a mistake does.  'untransposed' leaves the table alone and shows in the gradient only."""
    dst, src, keep = net['dst'], net['src'], net['keep']
    table, grad = net_table_and_grad(net, net['A'])
    tol = net_table_bound(net)
    assert nr.worst(table, table, tol) == 0
    if mistake == 'feed_normalised':
        bad, bad_grad = net_table_and_grad(net, net['A'], feed_normalised=True)
    elif mistake == 'both':
        bad, bad_grad = net_table_and_grad(net, nr.left_adjacency(dst, src, NN, keep, norm='both'))
    elif mistake == 'base_degrees':
        bad, bad_grad = net_table_and_grad(net, nr.left_adjacency(dst, src, NN, keep, degrees_of=torch.ones_like(keep)))
    elif mistake == 'zero_degree':
        # a node that lost every out-edge: keep[e] * (1 / out_deg[src]) is 0 * inf on its edges
        lost = (torch.bincount(src, minlength=NN) > 0) & (torch.bincount(src[keep], minlength=NN) == 0)
        assert int(lost.sum()) >= 1
        bad, bad_grad = net_table_and_grad(net, nr.left_adjacency(dst, src, NN, keep, zero_degree_as_one=False))
        assert nr.worst(bad, table, tol) == float('inf') and not bool(torch.isfinite(bad_grad).all())
        return
    elif mistake == 'no_input':
        bad, _ = net_table_and_grad(net, net['A'], with_input=False)
        assert bad.shape[1] == table.shape[1] - D
        assert nr.worst(bad, table[:, :bad.shape[1]], tol[:, :bad.shape[1]]) > 1          # every block sits D columns early
        return
    else:
        A_sym = net['A'].T.contiguous()
        bad, bad_grad = net_table_and_grad(net, net['A'], A_back=A_sym)
        assert nr.worst(bad, table, tol) == 0
        assert float((bad_grad - grad).abs().max()) > 1e-3 * float(grad.abs().max())
        return
    assert nr.worst(bad, table, tol) > 1
    assert float((bad_grad - grad).abs().max()) > 1e-3 * float(grad.abs().max())


# ---------------------------------------------------------------------------------------------------------------- the C ABI
def _block(nat, n_rows=64, d_in=64, d_out=64, p=0.0):
    a = nat.BiCombineArgs()
    for name in ('x', 'm', 'w1', 'w2', 'b1', 'b2', 'h', 'g_h', 'dx', 'dm', 'dw1', 'dw2', 'db1', 'db2', 'workspace'):
        setattr(a, name, 4096)
    a.n_rows, a.d_in, a.d_out, a.negative_slope, a.p = n_rows, d_in, d_out, 0.01, p
    a.workspace_bytes = 1 << 40
    return a


@pytest.mark.parametrize('entry', ['rsa_bi_combine', 'rsa_bi_combine_backward'])
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
    for field in ('x', 'm', 'w1', 'w2', 'b1', 'b2'):
        a = _block(nat)
        setattr(a, field, None)
        refused(a, b'is null')
    for field in ('x', 'm', 'w1', 'w2'):
        a = _block(nat)
        setattr(a, field, 4100)
        refused(a, b'16-byte aligned')
    refused(_block(nat, d_in=6), b'multiples of 4')
    refused(_block(nat, d_out=30), b'multiples of 4')
    refused(_block(nat, d_in=0), b'multiples of 4')
    refused(_block(nat, d_in=132), b'LDS')
    refused(_block(nat, d_out=256), b'LDS')
    refused(_block(nat, n_rows=-1), b'negative')
    refused(_block(nat, p=1.0), b'[0, 1)')
    refused(_block(nat, p=0.1), b'philox')            # grid_threads 0
    a = _block(nat, p=0.1)
    a.grid_threads, a.offset = 256, 2
    refused(a, b'philox')
    a = _block(nat)
    a.h, a.g_h = None, None
    refused(a, b'both null')
    a = _block(nat)
    a.h, a.g_h, a.n, a.g_n, a.n_stride, a.g_n_stride, a.n_col, a.g_n_col = None, None, 4096, 4096, 66, 66, 0, 0
    refused(a, b'multiples of 4')
    a.n_stride = a.g_n_stride = 64
    a.n_col = a.g_n_col = 4
    refused(a, b'col + d_out')
    assert fn(ctypes.byref(_block(nat, n_rows=0)), None) == 0          # nothing to do: no launch, no HIP call


def test_backward_outputs_and_workspace_are_checked(nat):
    lib = nat.lib()
    a = _block(nat)
    a.dw2 = None
    assert lib.rsa_bi_combine_backward(ctypes.byref(a), None) == -1 and b'is null' in lib.rsa_last_error()
    a = _block(nat)
    a.workspace_bytes = 1024
    assert lib.rsa_bi_combine_backward(ctypes.byref(a), None) == -1 and b'too small' in lib.rsa_last_error()
    need = lib.rsa_bi_combine_workspace_bytes(4099, 64, 64)
    assert need >= 4099 * 8 + 2 * 64 * 64 * 4 and lib.rsa_bi_combine_workspace_bytes(1 << 21, 64, 64) >= need
    assert lib.rsa_bi_combine_workspace_bytes(-1, 64, 64) < 0 and lib.rsa_bi_combine_workspace_bytes(8, 132, 64) < 0
    assert lib.rsa_abi_version() == 13


# ---------------------------------------------------------------------------------------------------------------- the module
def test_bicombiner_parameters_are_the_references():
    from recstudio_amd import graphmodule
    layer = graphmodule.BiCombiner(64, 32, dropout=0.1)
    assert sorted(layer.state_dict()) == ['linear_product.bias', 'linear_product.weight', 'linear_sum.bias', 'linear_sum.weight']
    assert tuple(layer.linear_sum.weight.shape) == (32, 64) and layer.negative_slope == 0.01
    for bad in ((6, 64), (64, 130), (256, 64)):
        with pytest.raises(ValueError, match='multiple of 4'):
            graphmodule.BiCombiner(*bad)
    with pytest.raises(ValueError, match='dropout'):
        graphmodule.BiCombiner(64, 64, dropout=1.0)
    with pytest.raises(RuntimeError, match='GPU only'):
        layer(torch.zeros(4, 64), torch.zeros(4, 64))


def test_forward_torch_is_the_referee_layer():
    """The torch-op twin (fp32, CPU) against the float64 layer, dropout mask from the same generator state."""
    from recstudio_amd import graphmodule
    torch.manual_seed(3)
    layer = graphmodule.BiCombiner(36, 20, dropout=0.5)
    inp = nr.layer_inputs(33, 36, 20, seed=9)
    gen = torch.Generator().manual_seed(21)
    u = torch.rand(33, 20, generator=torch.Generator().manual_seed(21))
    h, n = layer.forward_torch(inp['x'], inp['m'], generator=gen)
    args = [inp['x'], inp['m'], layer.linear_sum.weight.detach(), layer.linear_sum.bias.detach(),
            layer.linear_product.weight.detach(), layer.linear_product.bias.detach()]
    f = nr.layer_forward(*args, 0.01, 0.5, u)
    fb = nr.layer_forward_bounds(*args, f)
    assert torch.equal(h != 0, f['keep'] & (f['h'] != 0))
    assert nr.worst(h, f['h'], fb['h']) <= 1 and nr.worst(n, f['n'], fb['n']) <= 1
    layer.eval()
    h_eval, _ = layer.forward_torch(inp['x'], inp['m'], generator=gen)
    f0 = nr.layer_forward(*args, 0.01)
    assert nr.worst(h_eval, f0['h'], nr.layer_forward_bounds(*args, f0)['h']) <= 1


def test_ngcf_settings_and_refusals():
    """config/ngcf.yaml's values where the caller gives none, the caller's where it does, and what the model refuses."""
    import recstudio_amd as ra
    m = ra.NGCF()
    assert m.config['model']['layer_size'] == [64, 64, 64, 64] and m.config['model']['mess_dropout'] == [0.1, 0.1, 0.1]
    assert m.config['model']['node_dropout'] == 0.1 and m.config['model']['l2_reg_weight'] == 1e-5 and m.embed_dim == 64
    assert m.config['train']['batch_size'] == 2048 and m.config['train']['learning_rate'] == 1e-4
    assert m.config['train']['negative_count'] == 1 and issubclass(ra.NGCF, ra.LightGCN)
    m = ra.NGCF({'model': {'embed_dim': 32, 'layer_size': [32, 16], 'node_dropout': None, 'l2_reg_weight': 1e-3},
                 'train': {'learning_rate': 0.01}})
    assert m.config['model']['mess_dropout'] == [0.1] and m.config['model']['node_dropout'] is None
    assert m.config['model']['l2_reg_weight'] == 1e-3 and m.config['train']['learning_rate'] == 0.01
    with pytest.raises(ValueError, match='embed_dim'):
        ra.NGCF({'model': {'embed_dim': 32}})
    with pytest.raises(ValueError, match='at most 256'):
        ra.NGCF({'model': {'layer_size': [64] * 5, 'mess_dropout': [0.1] * 4}})
    with pytest.raises(ValueError, match='mess_dropout'):
        ra.NGCF({'model': {'mess_dropout': [0.1]}})
    with pytest.raises(ValueError, match='node_dropout'):
        ra.NGCF({'model': {'node_dropout': 1.0}})
    with pytest.raises(ValueError, match='multiple of 4'):
        m = ra.NGCF({'model': {'embed_dim': 64, 'layer_size': [64, 30], 'mess_dropout': [0.1]}})
        m._init_model(_tiny_dataset(ra))


def _tiny_dataset(ra):
    import spmm_referee as sr
    users, items = sr.random_bipartite(11, 13, 60, seed=1)
    return ra.TripletDataset.from_mapped_ids(users, items, n_users=11, n_items=13)


def test_ngcf_modules_on_the_host():
    """_init_model builds the reference's modules (their state_dict keys) and the left-normalised graph; the Linears take the
    model's weight init (xavier_normal, zero biases)."""
    import recstudio_amd as ra
    m = ra.NGCF({'model': {'spmm_chunk': 8}})
    data = _tiny_dataset(ra)
    m._init_model(data)
    m._init_parameter()
    keys = set(m.state_dict())
    for k in range(3):
        for name in ('linear_sum', 'linear_product'):
            assert {f'combiners.{k}.{name}.weight', f'combiners.{k}.{name}.bias', f'NGCFNet.combiners.{k}.{name}.weight'} <= keys
    assert {'user_emb.weight', 'item_emb.weight'} <= keys and not hasattr(m, 'LightGCNNet')
    assert all(float(c.linear_sum.bias.detach().abs().max()) == 0 for c in m.combiners)
    assert m.NGCFNet.out_dim == 256 and len(list(m.parameters())) == 2 + 4 * 3
    adj = m.left_adj
    out_deg = torch.bincount(adj.base.indices.long(), minlength=adj.n_nodes).clamp_min(1)
    assert torch.equal(adj.values, (1.0 / out_deg.double()).float()[adj.base.indices.long()]) and adj.t_keep is None
    A = nr.left_adjacency(torch.repeat_interleave(torch.arange(adj.n_nodes), adj.base.indptr[1:] - adj.base.indptr[:-1]),
                          adj.base.indices.long(), adj.n_nodes)
    assert torch.allclose(A.sum(0)[out_deg > 0][1:3], torch.ones(2, dtype=F64))          # a column of A sums to 1: 'left'
    with pytest.raises(RuntimeError, match='GPU'):
        m.NGCFNet.propagate(adj, torch.zeros(adj.n_nodes, 64))
