"""GPU: WRMF on ml-100k (d = 32, alpha 1, lambda 0.5).  One user half-epoch and one item half-epoch with model.fused_als on agree
with the flag off (the reference's padded op sequence) and with a dense float64 ALS sweep on the CPU (tests/als_referee.py: every
solved row inside the referee's forward bound, the epoch loss 1e-4 relative); model.item_bias agrees between the two arms; top-k
equals dense float64 scores; a 6-epoch fit does not raise the float64 WRMF objective beyond its fp32 rounding
(nnz + 2) u sum |terms| and ends above the untrained tables' test ndcg@10."""
import pytest
import torch

import als_referee as ar
import recstudio_amd as ra
from test_dataset_golden import make

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def splits(golden):
    ra.seed_everything(2022)
    return make(ra.ALSDataset, golden('data_ml100k')).build(split_ratio=[0.8, 0.1, 0.1], shuffle=True)


def fitted(trn, fused, epochs, item_bias=False):
    ra.seed_everything(7)
    m = ra.WRMF({'model': {'embed_dim': 32, 'fused_als': fused, 'item_bias': item_bias}, 'train': {'epochs': epochs, 'alpha': 1.0, 'lambda': 0.5}})
    m.fit(trn)
    return m


@pytest.mark.parametrize('epochs,item_bias', [(1, False), (2, False), (1, True)], ids=['users', 'items', 'users-item_bias'])
def test_half_epoch_against_flag_off_and_float64_sweep(splits, epochs, item_bias):
    trn = splits[0]
    a, b = fitted(trn, True, epochs, item_bias), fitted(trn, False, epochs, item_bias)
    for name in ('query_encoder', 'item_encoder'):
        wa, wb = getattr(a, name).weight.data.double(), getattr(b, name).weight.data.double()
        assert (wa - wb).norm() <= 1e-4 * wb.norm()
    assert abs(a.history[-1]['train_loss'] - b.history[-1]['train_loss']) <= 1e-4 * abs(b.history[-1]['train_loss'])
    if item_bias:                                                 # x is overwritten after the solve: not the solution of A x = b
        return
    users = epochs == 1                                           # the half-epoch that ran last: its other table did not change in it
    indptr, ids, ratings = trn.csr()[0 if users else 1]
    table = (a.item_encoder if users else a.query_encoder).weight.data
    x = (a.query_encoder if users else a.item_encoder).weight.data
    rows = (indptr[1:] > indptr[:-1]).nonzero().view(-1).numpy()
    worst = ar.judge(indptr.numpy(), ids.numpy(), table.cpu().numpy(), (table.T @ table).cpu().numpy(), 1.0, 0.5,
                     (ratings > 0).float().numpy(), rows, x.cpu().numpy()[rows])
    print('worst shares', worst)
    assert abs(a.history[-1]['train_loss'] - worst['mean_loss']) <= 1e-4 * abs(worst['mean_loss'])


def objective(m, trn):
    """sum_obs [(1 + alpha)(1 - p)^2 - p^2] + ||P Q^T||_F^2 + lambda (||P||^2 + ||Q||^2) in float64, and (nnz + 2) u sum |terms|."""
    P, Q = m.query_encoder.weight.data.double().cpu(), m.item_encoder.weight.data.double().cpu()
    sub = trn.inter_feat_subset
    p = (P[trn.inter_feat[trn.fuid][sub]] * Q[trn.inter_feat[trn.fiid][sub]]).sum(-1)
    dense, reg = ((P @ Q.T) ** 2).sum(), 0.5 * ((P ** 2).sum() + (Q ** 2).sum())
    return (float((2.0 * (1 - p) ** 2 - p ** 2).sum() + dense + reg),
            float((len(sub) + 2) * ar.U * ((2.0 * (1 - p) ** 2 + p ** 2).sum() + dense + reg)))


def test_fit_lowers_the_objective_ranks_and_learns(splits):
    trn, _, tst = splits
    m = fitted(trn, True, 1)
    values = [objective(m, trn)]
    for epoch in range(1, 6):
        m._als_half_epoch(epoch)
        values.append(objective(m, trn))
        assert values[-1][0] <= values[-2][0] + values[-1][1] + values[-2][1]
    scores = m.query_encoder.weight.data.double() @ m.item_encoder.weight.data.double()[1:].T
    _, top = m.topk({trn.fuid: torch.arange(1, 20, device='cuda')}, 5)
    assert torch.equal(top.cpu() - 1, scores[1:20].topk(5).indices.cpu())
    assert m.evaluate(tst, verbose=False)['ndcg@10'] > fitted(trn, True, 0).evaluate(tst, verbose=False)['ndcg@10']
