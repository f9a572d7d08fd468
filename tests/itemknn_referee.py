"""Float64 referee of ``ops.knn_build`` / ``ops.knn_score`` (rsa_knn_build, rsa_knn_score), written from
recstudio/model/mf/itemknn.py:12-41: with C = R^T R of the unit-valued R, n = diag C, for column i and every j != i with C[j, i] > 0
    cosine   s = C[j, i] / (sqrt(n_j) sqrt(n_i) + 1e-6)        jaccard   s = C[j, i] / (n_j + n_i - C[j, i] + 1e-6)
and the column keeps its min(knn, nnz) largest s.
Tolerance of ONE similarity, u = 2^-24, from the kernel's operation sequence (knn_sim in rsa_knn.hip; the build leaves hipcc's
correctly rounded fp32 divide and sqrt on and sets -ffp-contract=off, so every operation below rounds once; the integer operands
are exact below 2^24, which the host checks):
  cosine   fl(sqrt n_j), fl(sqrt n_i), their product, the sum with fl(1e-6) (the constant's own rounding perturbs a part of that
           sum), the quotient: 6 factors (1 + d), |d| <= u       ->  |s^ - s| <= gamma_6 s
  jaccard  the integer n_j + n_i - c converted (exact below 2^24, one rounding above), the sum with fl(1e-6), the quotient and the
           constant's rounding: 4 factors                       ->  |s^ - s| <= gamma_4 s
with gamma_n = n u / (1 - n u).  Two fp32 values the kernel ranks one way can therefore be the other way round in float64 by at
most tol (s_a + s_b): that is the slack of the "nothing better was left out" check; no element is exempted.
Score of one (user, item): a sum of K fp32 terms in some order, |sum^ - sum| <= (K + 2) u sum |terms| (+ what the terms carry)."""
import numpy as np
import torch

U = 2.0 ** -24
gamma = lambda n: n * U / (1.0 - n * U)      # noqa: E731
SIM_TOL = {'cosine': gamma(6), 'jaccard': gamma(4)}


def make_data(n_users, N, seed=0):
    """bool R [n_users, N] with: column 0 (padding) and one more item held by nobody, an item held by every user (two of them where
    N allows: a pair that co-occurs in every user), a user with no items, and a block of items with identical user sets (exact ties)."""
    rng = np.random.default_rng(seed)
    R = rng.random((n_users, N)) < min(0.3, 8.0 / N + 0.05)
    R[:, 1] = True
    if N > 8:
        R[:, 2] = True
        R[:, N - 2] = False
        block = np.arange(3, min(3 + max(4, N // 8), N - 2))
        R[:, block] = R[:, block[:1]]
        R[:, N - 1] = R[:, 3]                                   # the same user set once more, at the far end of the catalog
    R[:, 0] = False
    if n_users > 2:
        R[n_users - 1] = False
    return R


def csrs(R, device='cpu'):
    """(u_indptr, u_items, i_indptr, i_users): int64 row pointers, int32 ids ascending within a row."""
    def one(M):
        r, c = np.nonzero(M)
        indptr = np.concatenate([[0], np.cumsum(M.sum(1))]).astype(np.int64)
        return torch.from_numpy(indptr).to(device), torch.from_numpy(c.astype(np.int32)).to(device)
    return one(R) + one(R.T)


def rule64(R, similarity, keep_diagonal=False, union_without_c=False):
    """(S float64 [N, N] with S[j, i] the similarity of neighbour j in column i, 0 where there is none; cls int64 [N, N], equal
    exactly where two neighbours of a column have the same operands).  The two flags seed mistakes for the tests of the judgement."""
    if similarity not in SIM_TOL:
        raise ValueError('unsupported similarity metric')
    Rd = R.astype(np.float64)
    C = Rd.T @ Rd
    n = np.diag(C).copy()
    if not keep_diagonal:
        np.fill_diagonal(C, 0)
    den = np.sqrt(n)[:, None] * np.sqrt(n)[None] + 1e-6 if similarity == 'cosine' else \
        n[:, None] + n[None] - (0 if union_without_c else C) + 1e-6
    return C / den, (C * 2.0 ** 26 + n[:, None]).astype(np.int64)


def lists_from(S, knn, largest=True):
    """The neighbour lists (nbr_id int32, nbr_sim float64, nbr_cnt int32) of a dense S under the stated order: descending s, then
    ascending id (``largest`` False keeps the smallest instead: a seeded mistake)."""
    N = S.shape[0]
    ids, sims, cnt = np.full((N, knn), -1, np.int32), np.zeros((N, knn)), np.zeros(N, np.int32)
    for i in range(N):
        nz = np.flatnonzero(S[:, i])
        order = nz[np.lexsort((nz, -S[nz, i] if largest else S[nz, i]))][:knn]
        order = order[np.lexsort((order, -S[order, i]))]
        cnt[i] = len(order)
        ids[i, :len(order)], sims[i, :len(order)] = order, S[order, i]
    return ids, sims, cnt


def judge(S, cls, nbr_id, nbr_sim, nbr_cnt, knn, tol):
    """Asserts the judgement of every column (module docstring of tests/test_gpu_itemknn.py lists it); -> the worst |s^ - s| / (tol s)."""
    N, worst = S.shape[0], 0.0
    nbr_id, nbr_sim, nbr_cnt = (np.asarray(t) for t in (nbr_id, nbr_sim, nbr_cnt))
    assert nbr_id.shape == nbr_sim.shape == (N, knn) and nbr_cnt.shape == (N,)
    for i in range(N):
        col, k = S[:, i], int(nbr_cnt[i])
        nz = np.flatnonzero(col)
        assert k == min(knn, len(nz)), ('count', i, k, len(nz))
        assert (nbr_id[i, k:] == -1).all() and not nbr_sim[i, k:].any() and not np.signbit(nbr_sim[i, k:]).any(), ('unused slots', i)
        if k == 0:
            continue
        ids, sims = nbr_id[i, :k].astype(np.int64), nbr_sim[i, :k].astype(np.float64)
        assert ids.min() >= 0 and ids.max() < N and len(np.unique(ids)) == k, ('ids', i)
        assert (ids != i).all() and (col[ids] > 0).all(), ('not an off-diagonal non-zero', i)
        err = np.abs(sims - col[ids]) / col[ids]
        assert (err <= tol).all(), ('value', i, err.max(), tol)
        worst = max(worst, float(err.max()) / tol if tol else 0.0)
        rest = np.setdiff1d(nz, ids)
        if len(rest):
            low = col[ids].min()
            assert (col[rest] - low <= tol * (col[rest] + low)).all(), ('a better neighbour was left out', i)
            lost_tie = (cls[rest, i][:, None] == cls[ids, i][None]) & (ids[None] > rest[:, None])
            assert not lost_tie.any(), ('a higher id won an exact tie', i)
        step = np.diff(nbr_sim[i, :k])
        assert (step <= 0).all() and (np.diff(ids)[step == 0] > 0).all(), ('stored order', i)
    return worst


def score_bound(K, sum_abs, carried=0.0):
    return (K + 2) * U * sum_abs + carried
