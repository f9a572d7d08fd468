"""GPU: NCF with model.fused_scorer (the pair kernel): one training step against a float64 step on the negatives and uniforms the
run drew, top-k against dense float64 scores, checkpoints across the flag, a short fit next to the same model on torch ops."""
import pytest
import torch

from test_dataset_golden import make
from test_gpu_pair_mlp import close

pytestmark = pytest.mark.gpu
DEV = 'cuda'
SEED = 11                     # fixed; checked below: no pre-activation of the float64 step lies within 1e-5 of 0


@pytest.fixture(scope='module')
def ra():
    import recstudio_amd
    recstudio_amd._native.lib()
    torch.cuda.init()
    return recstudio_amd


@pytest.fixture(scope='module')
def ml100k(ra, golden):
    ra.seed_everything(2022)
    return make(ra.TripletDataset, golden('data_ml100k')).build(split_ratio=[0.8, 0.1, 0.1], shuffle=True)


def build(ra, trn, mode, n_neg, fused, dropout=0.5, **train):
    model = ra.NCF({'model': {'score_mode': mode, 'dropout': dropout, 'fused_scorer': fused},
                    'train': dict({'negative_count': n_neg}, **train)})
    model._init_model(trn)
    model._init_parameter()
    torch.manual_seed(SEED)
    # random, non-grid weights.  The biases lie 0.3 .. 0.45 either side of 0 and the hidden weights are small next to them, so no
    # pre-activation of the 1e5 of a step comes within 1e-5 of 0 (float64_step asserts that); the output weights are positive, so
    # every pair passes a gradient.  The price: a hidden unit's ReLU gate is nearly the same for every pair of the step, so a
    # gate taken from the wrong PAIR would not show here -- tests/test_gpu_pair_mlp.py, whose gates vary by pair, is where it does
    for name, p in model.score_func.named_parameters():
        bound = 0.03 if name.endswith('model.4.weight') else 0.15 if name.endswith('model.1.weight') else 0.3
        torch.nn.init.uniform_(p, -bound, bound)
        with torch.no_grad():
            if name.endswith('bias'):
                p.copy_(torch.sign(p) * (0.3 + p.abs() / 2))
            elif name in ('W.weight', 'trans.model.7.weight'):
                p.uniform_(0.05, 0.3)
    return model.to(DEV)


def batch_of(trn, B, model):
    g = torch.Generator().manual_seed(4)
    users = torch.randint(1, trn.num_users, (B,), generator=g)
    items = torch.randint(1, trn.num_items, (B,), generator=g)
    return {model.fuid: users.to(DEV), model.fiid: items.to(DEV), model.frating: torch.ones(B, device=DEV)}


def float64_step(model, batch, neg, u, mode):
    """BCE over relu scores, float64, from copies of the model's parameters -> (loss, {name: grad})"""
    leaves = {k: v.detach().double().cpu().requires_grad_(True) for k, v in model.named_parameters()}
    d = model.embed_dim
    ids = torch.cat([batch[model.fiid].view(-1, 1).cpu(), neg], 1)
    S = ids.shape[1]
    q = leaves['query_encoder.weight'][batch[model.fuid].cpu()].repeat_interleave(S, dim=0)
    x = leaves['item_encoder.weight'][ids.reshape(-1)]
    keep_q = float(torch.tensor(0.5, dtype=torch.float32))
    pre = 'score_func.trans.model.' if mode == 'mlp' else 'score_func.mlp.model.'
    h, at = torch.cat([q, x], 1), 0
    for k, idx in enumerate((1, 4)):
        h = torch.where(u[:, at:at + h.shape[1]].double() < keep_q, h / keep_q, torch.zeros_like(h))
        at += h.shape[1]
        z = h @ leaves[f'{pre}{idx}.weight'].t() + leaves[f'{pre}{idx}.bias']
        assert float(z.detach().abs().min()) > 1e-5
        h = torch.relu(z)
    if mode == 'mlp':
        h = torch.where(u[:, at:at + h.shape[1]].double() < keep_q, h / keep_q, torch.zeros_like(h))
        z = h @ leaves[pre + '7.weight'][0] + leaves[pre + '7.bias'][0]
    else:
        w = leaves['score_func.W.weight'][0]
        z = (q * x) @ w[:d] + h @ w[d:]
    assert float(z.detach().abs().min()) > 1e-5
    s = torch.relu(z).view(-1, S)
    loss = (-torch.nn.functional.logsigmoid(s[:, 0]) + torch.nn.functional.softplus(s[:, 1:]).mean(1)).mean()
    loss.backward()
    return loss.detach(), {k: v.grad for k, v in leaves.items()}


@pytest.mark.parametrize('mode', ['fusion', 'mlp'])
@pytest.mark.parametrize('n_neg', [1, 4])
def test_one_training_step_against_float64(ra, ml100k, n_neg, mode):
    trn = ml100k[0]
    model = build(ra, trn, mode, n_neg, True).train()
    batch = batch_of(trn, 96, model)
    gen = torch.cuda.default_generators[torch.cuda.current_device()]
    torch.manual_seed(SEED)
    off0 = gen.get_offset()
    loss = model.training_step(batch)
    loss.backward()
    off1 = gen.get_offset()
    # the documented order: the negatives, then the one mask call
    gen.set_offset(off0)
    _, neg, _ = model.sampler(model.query_encoder(batch[model.fuid]), n_neg, batch[model.fiid])
    C = ra.ops.pair_mlp_masked_columns(64, [128, 64], mode)
    u = torch.rand(96 * (1 + n_neg), C, device=DEV).cpu()
    assert gen.get_offset() == off1
    want, grads = float64_step(model, batch, neg.cpu(), u, mode)
    assert abs(float(loss) - float(want)) <= 1e-4 * abs(float(want))
    for k, p in model.named_parameters():
        got, ref = p.grad.double().cpu(), grads[k] if grads[k] is not None else torch.zeros_like(p, dtype=torch.float64, device='cpu')
        assert bool(((got - ref).abs() <= 3e-4 * ref.abs() + 3e-6 * ref.abs().max()).all()), k
    assert float(model.item_encoder.weight.grad[0].abs().max()) == 0.0
    # the flag off at the same seed draws the same negatives
    off = build(ra, trn, mode, n_neg, False).train()
    gen.set_offset(off0)
    assert torch.equal(off.forward(batch, return_neg_id=True)['neg_id'], neg)


def test_the_generator_moves_only_for_a_training_mask(ra, ml100k):
    """eval mode and dropout 0 draw nothing; a training call with dropout advances the generator as its one torch.rand([M, C])"""
    trn = ml100k[0]
    gen = torch.cuda.default_generators[torch.cuda.current_device()]
    ids = torch.randint(1, trn.num_items, (64, 3), device=DEV)
    for dropout, train, C in ((0.5, False, 0), (0.0, True, 0), (0.5, True, 2 * 64 + 128)):
        model = build(ra, trn, 'fusion', 1, True, dropout=dropout).train(train)
        q = model.query_encoder(ids[:, 0] % trn.num_users)
        off0 = gen.get_offset()
        assert model.score_func.score_ids(q, model.item_encoder.weight, ids) is not None
        off1 = gen.get_offset()
        gen.set_offset(off0)
        if C:
            torch.rand(ids.numel(), C, device=DEV)
        assert gen.get_offset() == off1, (dropout, train)


def test_topk_against_dense_float64_scores(ra):
    g = torch.Generator().manual_seed(9)
    trn = ra.TripletDataset.from_mapped_ids(torch.randint(1, 61, (900,), generator=g).numpy(),
                                            torch.randint(1, 1683, (900,), generator=g).numpy(), n_users=61, n_items=1683)
    model = build(ra, trn, 'fusion', 1, True).eval()
    assert trn.num_items == 1683
    model.config['eval']['pair_chunk'] = 500
    users = torch.arange(1, 41, device=DEV)
    hist = torch.randint(0, trn.num_items, (40, 30), generator=torch.Generator().manual_seed(2)).to(DEV)
    score, items = model.topk({model.fuid: users}, 20, hist)
    sf = model.score_func.double().cpu()
    q, table = model.query_encoder.weight.detach().double().cpu()[users.cpu()], model.item_encoder.weight.detach().double().cpu()
    dense = sf._torch_scores(q.unsqueeze(1).expand(40, 1683, 64), table.unsqueeze(0).expand(40, 1683, 64)).detach()
    dense[:, 0] = -float('inf')
    dense.scatter_(1, hist.cpu(), -float('inf'))
    want = torch.topk(dense, 20, dim=1).values
    assert not bool((items == 0).any()) and not bool((items.unsqueeze(2) == hist.unsqueeze(1)).any())
    assert close(score, want) and close(torch.gather(dense, 1, items.cpu()), want)
    model.score_func.float().to(DEV)


def test_a_checkpoint_moves_between_the_flag_s_settings(ra, ml100k, tmp_path):
    trn = ml100k[0]
    a, b = build(ra, trn, 'fusion', 1, False).eval(), build(ra, trn, 'fusion', 1, True).eval()
    torch.save(a.state_dict(), tmp_path / 'off.pt')
    b.load_state_dict(torch.load(tmp_path / 'off.pt'))
    batch = batch_of(trn, 64, a)
    ids = torch.randint(1, trn.num_items, (64, 3), device=DEV)
    q = a.query_encoder(batch[a.fuid])
    on = b.score_func.score_ids(q, b.item_encoder.weight, ids)
    off = a.score_func(q, a.item_encoder(ids))
    assert on is not None and torch.allclose(on, off, rtol=1e-4, atol=1e-6)
    torch.save(b.state_dict(), tmp_path / 'on.pt')
    a.load_state_dict(torch.load(tmp_path / 'on.pt'))


def test_fit_next_to_the_torch_op_model(ra, ml100k):
    """3 epochs of NCF (yaml defaults) on ml-100k, model.fused_scorer on next to off, same seed: every epoch loss within 2 %"""
    trn, val, tst = ml100k
    runs = {}
    for fused in (True, False):
        model = ra.NCF({'model': {'fused_scorer': fused}, 'train': {'epochs': 3, 'batch_size': 2048}, 'eval': {'batch_size': 256}})
        model.fit(trn, val)
        runs[fused] = [h['train_loss'] for h in model.history]
        print('fused' if fused else 'torch', runs[fused])
    assert len(runs[True]) == 3 and all(abs(a - b) <= 0.02 * abs(b) for a, b in zip(runs[True], runs[False])), runs
