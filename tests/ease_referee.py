"""The referee of the EASE kernels (helpers only): test matrices and ``B*``, the reference's B from an inverse refined in extended
precision.  ``B*``: numpy's float64 inverse of G, three Newton steps ``P <- P (2 I - G P)`` in ``np.longdouble`` (each squares the
residual: 1e-13 -> below the longdouble unit), then the reference's two lines, rounded to float64 once."""
import functools

import numpy as np

U64 = 2.0 ** -53


def zipf_data(n_users, N, seed=0):
    """bool R [n_users, N]: item i >= 1 is held with probability min(1, 6 / i) (Zipf), item 0 (padding) by nobody; the last user
    holds nothing."""
    rng = np.random.default_rng(seed + 1000 * N)
    R = rng.random((n_users, N)) < np.minimum(1.0, 6.0 / np.maximum(np.arange(N), 1))[None]
    R[:, 0] = False
    if n_users > 2:
        R[-1] = False
    return R


def gram(R, lam):
    """G = R^T R + lam I in float64: integers below 2^53 plus lam, every entry rounded at most once."""
    Rd = R.astype(np.float64)
    return Rd.T @ Rd + lam * np.eye(R.shape[1])


def spd_with_spectrum(n, cond, seed=0):
    """Q diag(s) Q^T with s log-spaced in [1, cond] and Q a random orthogonal matrix, symmetrised exactly."""
    rng = np.random.default_rng(seed)
    Q = np.linalg.qr(rng.standard_normal((n, n)))[0]
    A = (Q * np.logspace(0, np.log10(cond), n)) @ Q.T
    return (A + A.T) / 2


def weights_from(P):
    """The reference's two lines: B = P / (-diag P), B[diag] = 0."""
    B = P / (-np.diag(P))
    B[np.diag_indices_from(B)] = 0
    return B


def refined_inverse(G):
    Gl = G.astype(np.longdouble)
    P, I2 = np.linalg.inv(G).astype(np.longdouble), 2 * np.eye(len(G), dtype=np.longdouble)
    for _ in range(3):
        P = P @ (I2 - Gl @ P)
    return P


@functools.lru_cache(maxsize=None)
def ease_case(n, lam, n_users=300):
    """(R, G, B*, tol) for the Gram matrix of zipf_data at n items: tol = 8 max(e_np, n u max|B*|), e_np the error of numpy's own
    float64 inverse against B* on this matrix."""
    R = zipf_data(n_users, n)
    G = gram(R, lam)
    Bs = weights_from(refined_inverse(G)).astype(np.float64)
    e_np = np.abs(weights_from(np.linalg.inv(G)) - Bs).max()
    return R, G, Bs, 8 * max(e_np, n * U64 * np.abs(Bs).max())


def closed_form_loss(P, lam):
    d = np.diag(P)
    return np.sqrt(np.sum(1 / d - lam * (P * P).sum(0) / (d * d)))
