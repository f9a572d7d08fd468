"""GPU: ops.als_solve (rsa_als.hip) against the float64 referee (tests/als_referee.py): backward error, forward error and loss
inside their bounds for d = 32, 64, 128, row lengths 0, 1, 2, 31, 32, 33, d - 1, d, d + 1 (rank-deficient sums: only lam I + gram
make A definite) and C, C + 1, 2 C + 1 either side of the chunk split (C = ops.ALS_CHUNK), B = 1, 5, 300, N = 23 or 997, under
(alpha, lam) = (1, 0.5) and (40, 0.01); the latter over N = 997 at d = 32, 64 and N = 4001 at d = 128, where the referee's
kappa eta < 0.1 holds (checked on the CPU: gram over fewer rows leaves a row of about d positions with kappa eta above it).  Every
case: rated None and with zeros, an id twice in a row, indices read from a view inside a buffer of out-of-range ids, two runs
bit-equal, status 0.  A shuffled subset with repeats, rows solved alone and the loss-only form are bit-equal to / judged like the
batch of 300.  One constructed non-positive pivot between two healthy rows; one table past 4 GiB.
Worst shares of the bounds, as printed on the MI355X:
    backward 0.001   forward < 0.001   loss 0.106   (kappa eta <= 0.042; the case past 4 GiB: 5e-5, 2e-5, 0.002)"""
import numpy as np
import pytest
import torch

import als_referee as ar

pytestmark = pytest.mark.gpu
DEV = 'cuda'
CASES = [(32, 997, 300, 1.0, 0.5), (64, 997, 300, 1.0, 0.5), (128, 997, 300, 1.0, 0.5), (32, 23, 5, 1.0, 0.5), (64, 997, 1, 1.0, 0.5),
         (128, 997, 5, 1.0, 0.5), (32, 997, 300, 40.0, 0.01), (64, 997, 300, 40.0, 0.01), (128, 4001, 300, 40.0, 0.01)]


@pytest.fixture(scope='module')
def ops():
    import recstudio_amd
    recstudio_amd._native.lib()
    torch.cuda.init()
    return recstudio_amd.ops


def lengths_for(d, B, C):
    edge = [0, 1, 2, 31, 32, 33, d - 1, d, d + 1, C, C + 1, 2 * C + 1]
    return {1: [C + 1], 5: [0, 33, d, C + 1, 1]}.get(B) or edge + [int(v) for v in np.random.default_rng(d).integers(0, 40, size=B - 12)]


def upload(case):
    indptr, indices, t, rated = (None if v is None else torch.from_numpy(v).to(DEV) for v in case)
    wide = torch.full((len(indices) + 11,), 1 << 30, dtype=torch.int32, device=DEV)       # out-of-range ids around the view
    wide[7:7 + len(indices)] = indices
    return indptr, wide[7:7 + len(indices)], t, t.T @ t, rated


bits = lambda t: t.view(torch.int32)      # noqa: E731


def solve_and_judge(ops, case, dev, alpha, lam, rows=None):
    indptr, indices, table, gram, rated = dev
    rows_dev = None if rows is None else torch.as_tensor(rows, dtype=torch.int64, device=DEV)
    x, loss, status = ops.als_solve(indptr, indices, table, gram, alpha, lam, rows=rows_dev, rated=rated, want_loss=True)
    assert not status.any()
    worst = ar.judge(case[0], case[1], case[2], gram.cpu().numpy(), alpha, lam, case[3], rows, x.cpu().numpy(), loss.cpu().numpy())
    x2, loss2, _ = ops.als_solve(indptr, indices, table, gram, alpha, lam, rows=rows_dev, rated=rated, want_loss=True)
    assert torch.equal(bits(x), bits(x2)) and torch.equal(bits(loss), bits(loss2))
    return x, loss, worst


@pytest.mark.parametrize('rated_zeros', [False, True], ids=['ones', 'rated'])
@pytest.mark.parametrize('d,N,B,alpha,lam', CASES, ids=str)
def test_solve_within_bounds(ops, d, N, B, alpha, lam, rated_zeros):
    case = ar.make_case(d + B, d, N, lengths_for(d, B, ops.ALS_CHUNK), rated_zeros=rated_zeros)
    print('worst shares', solve_and_judge(ops, case, upload(case), alpha, lam)[2])


@pytest.mark.parametrize('d', [32, 64, 128])
def test_subset_rows_and_batch_independence(ops, d):
    case = ar.make_case(5, d, 997, lengths_for(d, 300, ops.ALS_CHUNK), rated_zeros=True)
    dev = upload(case)
    x_all, loss_all, _ = solve_and_judge(ops, case, dev, 1.0, 0.5)
    subset = [int(r) for r in np.random.default_rng(1).permutation(300)[:40]] + [11, 9, 11, 0]    # 9, 11: rows of C and 2 C + 1, twice
    for rows in (subset, [8], [11], [20]):                        # d + 1, 2 C + 1 and a short row, each solved alone
        x, loss, _ = solve_and_judge(ops, case, dev, 1.0, 0.5, rows=rows)
        assert torch.equal(bits(x), bits(x_all[rows])) and torch.equal(bits(loss), bits(loss_all[rows]))
    xb = x_all.clone()                                            # the loss of a caller's own x (a column overwritten): loss-only form
    xb[:, -1] = 1.0
    loss_b = ops.als_solve(*dev[:4], 1.0, 0.5, rated=dev[4], x=xb)[1]
    for r in (0, 2, 8, 11):
        Y, w, G, _, _ = ar.row_system(case[0], case[1], case[2], dev[3].cpu().numpy(), 1.0, 0.5, case[3], r)
        ar.loss_share(Y, w, G, 1.0, xb[r].double().cpu().numpy(), float(loss_b[r]), r)


def test_non_positive_pivot_is_a_status(ops):
    """lam = 0, gram = 0, d = 32: row 1 has one position with y = 1, so A = y y^T, every step is exact and pivot 1 is 0.  Rows 0 and 2
    hold 40 independent positions each: definite, and untouched by their neighbour."""
    table = torch.randn(100, 32, device=DEV) * 0.1
    table[5] = 1.0
    indptr = torch.tensor([0, 40, 41, 81], device=DEV)
    indices = torch.cat([torch.arange(10, 50), torch.tensor([5]), torch.arange(50, 90)]).to(torch.int32).to(DEV)
    gram = torch.zeros(32, 32, device=DEV)
    x, _, status = ops.als_solve(indptr, indices, table, gram, 1.0, 0.0)
    assert status.tolist() == [0, 2, 0] and torch.isnan(x[1]).all() and torch.isfinite(x[[0, 2]]).all()       # 1 + the pivot's index
    for r in (0, 2):
        alone = ops.als_solve(indptr, indices, table, gram, 1.0, 0.0, rows=torch.tensor([r], device=DEV))[0]
        assert torch.equal(bits(alone[0]), bits(x[r]))


def test_table_past_4gib(ops):
    d, N = 128, (1 << 23) + 4096                                  # N d 4 bytes > 4 GiB: the last rows lie past byte offset 2^32
    indptr, local, tail, _ = ar.make_case(3, d, 997, [0, 1, 33, d, ops.ALS_CHUNK + 1])
    table = torch.zeros(N, d, device=DEV)
    table[N - 997:] = torch.from_numpy(tail).to(DEV)
    gram = table[N - 997:].T @ table[N - 997:]
    x, loss, status = ops.als_solve(torch.from_numpy(indptr).to(DEV), torch.from_numpy(local + (N - 997)).to(DEV), table, gram, 1.0, 0.5, want_loss=True)
    assert not status.any()
    print('past 4 GiB', ar.judge(indptr, local, tail, gram.cpu().numpy(), 1.0, 0.5, None, None, x.cpu().numpy(), loss.cpu().numpy()))
