"""CPU: the pair scorers' torch twin against the float64 rule, the reference's state_dict keys and shape cases, NCF from its yaml
defaults, and the argument checks of ops.pair_mlp (which run before any HIP call)."""
import pytest
import torch

MLP_KEYS = ['trans.model.1.weight', 'trans.model.1.bias', 'trans.model.4.weight', 'trans.model.4.bias', 'trans.model.7.weight',
            'trans.model.7.bias']
FUSION_KEYS = ['W.weight', 'mlp.model.1.weight', 'mlp.model.1.bias', 'mlp.model.4.weight', 'mlp.model.4.bias']


@pytest.fixture(scope='module')
def ra():
    import recstudio_amd
    return recstudio_amd


def scorer(ra, mode, d=8, hidden=(12, 6), dropout=0.5):
    torch.manual_seed(3)
    if mode == 'mlp':
        return ra.MLPScorer(ra.MLPModule([2 * d] + list(hidden) + [1], 'relu', dropout)).double()
    return ra.FusionMFMLPScorer(d, hidden[-1], ra.MLPModule([2 * d] + list(hidden), 'relu', dropout)).double()


def rule(q, x, lin, w_out, b_out, p, u):
    """the issue's formulas, float64, written out"""
    keep_q = float(torch.tensor(1.0 - p, dtype=torch.float32))
    d, at = q.shape[1], 0
    h = torch.cat([q, x], 1)
    masked = [h.shape[1]] + [l.out_features for l in lin]
    for k in range(len(lin) + 1):
        if k < len(lin) or b_out is not None:
            h = torch.where(u[:, at:at + masked[k]] < keep_q, h / keep_q, torch.zeros_like(h))
            at += masked[k]
        if k < len(lin):
            h = torch.relu(h @ lin[k].weight.t() + lin[k].bias)
    if b_out is None:
        return torch.relu((q * x) @ w_out[0, :d] + h @ w_out[0, d:])
    return torch.relu(h @ w_out[0] + b_out[0])


@pytest.mark.parametrize('mode', ['mlp', 'fusion'])
def test_twin_equals_the_float64_rule(ra, mode):
    s = scorer(ra, mode)
    lin, p, w_out, b_out, fusion = s._parts()
    g = torch.Generator().manual_seed(1)
    q, x = torch.randn(37, 8, generator=g).double(), torch.randn(37, 8, generator=g).double()
    C = ra.ops.pair_mlp_masked_columns(8, [12, 6], mode)
    assert C == (16 + 12 if fusion else 16 + 12 + 6) and p == 0.5
    u = torch.rand(37, C, generator=g)
    tail = {'w_h': w_out[0, 8:], 'w_mf': w_out[0, :8]} if fusion else {'w_h': w_out[0], 'b_out': b_out}
    got = ra.pair_mlp_torch(q, x, [(l.weight, l.bias) for l in lin], p=p, u=u, **tail)
    want = rule(q, x, lin, w_out, b_out, p, u)
    assert float((got - want).abs().max()) <= 1e-12 and float(want.max()) > 0
    s.eval()                                                         # eval: the modules themselves are the same function
    assert float((s(q, x) - s._torch_scores(q, x)).abs().max()) <= 1e-12


def test_state_dict_keys_are_the_reference_s(ra):
    assert list(scorer(ra, 'mlp').state_dict()) == MLP_KEYS
    assert list(scorer(ra, 'fusion').state_dict()) == FUSION_KEYS


@pytest.mark.parametrize('mode', ['mlp', 'mf', 'fusion'])
def test_ncf_builds_from_the_yaml_defaults(ra, mode):
    model = ra.NCF({'model': {'score_mode': mode}})
    cfg = model.config
    assert cfg['model']['activation'] == 'relu' and cfg['model']['dropout'] == 0.1 and cfg['model']['mlp_hidden_size'] == [128, 64]
    assert cfg['train']['negative_count'] == 1 and cfg['train']['excluding_hist'] is False and 'fused_scorer' in cfg['model']
    assert ra.NCF().config['model']['score_mode'] == 'fusion'
    assert type(model.score_func) is {'mlp': ra.MLPScorer, 'mf': ra.GMFScorer, 'fusion': ra.FusionMFMLPScorer}[mode]
    assert isinstance(model._get_loss_func(), ra.BinaryCrossEntropyLoss) and ra.NCF._get_dataset_class() is ra.TripletDataset
    keys = list(model.score_func.state_dict())
    want = {'mlp': MLP_KEYS, 'mf': ['W.weight'], 'fusion': FUSION_KEYS}[mode]
    assert keys == want
    assert sorted(k for k in model.state_dict() if k.startswith('score_func.')) == sorted('score_func.' + k for k in want)


@pytest.mark.parametrize('mode', ['mlp', 'fusion'])
def test_the_five_shape_cases(ra, mode):
    s = scorer(ra, mode).float().eval()
    B, L, n, N, d = 3, 4, 5, 7, 8
    r = lambda *shape: torch.randn(*shape)         # noqa: E731
    assert s(r(B, d), r(B, d)).shape == (B,)
    assert s(r(B, d), r(B, n, d)).shape == (B, n)
    assert s(r(B, d), r(N, d)).shape == (B, N)
    assert s(r(B, L, d), r(B, L, d)).shape == (B, L)
    assert s(r(B, L, d), r(B, L, n, d)).shape == (B, L, n)


def test_pair_mlp_checks_its_arguments_before_any_hip_call(ra):
    ops = ra.ops
    q, t, ids = torch.zeros(4, 64), torch.zeros(9, 64), torch.zeros(4, 2, dtype=torch.int64)
    w1, b1, w2, b2, wh, wmf = torch.zeros(128, 128), torch.zeros(128), torch.zeros(64, 128), torch.zeros(64), torch.zeros(64), torch.zeros(64)
    bad = [
        dict(w1=torch.zeros(128, 100)),                              # fan-in is not 2d
        dict(w1=torch.zeros(48, 128), b1=torch.zeros(48), w2=torch.zeros(64, 48)),      # a width outside 32 / 64 / 128
        dict(ids=ids.int()), dict(ids=None), dict(ids=None, item_range=(5, 9)),
        dict(w_mf=None), dict(b_out=torch.zeros(1)), dict(p=1.0), dict(p=0.5),          # (p without a philox state)
    ]
    for change in bad:
        a = dict(query=q, table=t, ids=ids, w1=w1, b1=b1, w2=w2, b2=b2, w_h=wh, w_mf=wmf)
        a.update(change)
        with pytest.raises((ValueError, TypeError)):
            ops.pair_mlp(**a)
    with pytest.raises(ValueError, match='LDS'):                     # d = 128 with [128, 128]: 200 KB of padded weights
        ops.pair_mlp(torch.zeros(4, 128), torch.zeros(9, 128), ids, torch.zeros(128, 256), b1, torch.zeros(128, 128),
                     torch.zeros(128), torch.zeros(128), w_mf=torch.zeros(128))
    with pytest.raises(RuntimeError, match='GPU only'):              # everything in order: only then is the device looked at
        ops.pair_mlp(q, t, ids, w1, b1, w2, b2, wh, w_mf=wmf)
    assert not ops.pair_mlp_kernel_ok(q, t, [128, 64]) and ops.pair_mlp_lds_bytes(64, [128, 64]) <= 160 << 10
