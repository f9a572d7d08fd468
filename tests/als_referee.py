"""Float64 referee of ``ops.als_solve`` (rsa_als_solve): per requested CSR row, from the fp32 inputs,
    A = alpha * sum_e y_e y_e^T + gram + lam I     b = (1 + alpha) * sum_e rated_e y_e     x* = A^-1 b
    loss(x) = (1 + alpha) * sum_e (rated_e - <x, y_e>)^2 - sum_e <x, y_e>^2 + x^T gram x
Bounds, from u = 2^-24 alone (gamma_n = n u / (1 - n u)), for a row of K positions and width d:
  formation   |dA| <= (K + 2) u (alpha sum_e |y_e| |y_e|^T + |gram| + lam I) =: EA,   |db| <= (K + 2) u (1 + alpha) sum_e |rated_e| |y_e| =: Eb
  Cholesky    (A + dA) x^ = b with |dA| <= gamma_{3d+1} |R^T| |R|,  || |R^T| |R| ||_2 <= d ||A||_2 / (1 - d gamma_{d+1})     (Higham, ASNA 10.4-10.6)
  eta         = max( (||EA||_F + gamma_{3d+1} d ||A||_2 / (1 - d gamma_{d+1})) / ||A||_2 ,  ||Eb||_2 / ||b||_2 )
  1. backward ||b - A x^||_2 <= eta (||A||_2 ||x^||_2 + ||b||_2)
  2. forward  ||x^ - x*||_2 / ||x*||_2 <= 2 kappa eta / (1 - kappa eta),  kappa = cond_2(A) in float64;  kappa eta < 0.1 is asserted
  3. loss     |loss^ - loss(x^)| <= u [ (K + 2) T + (d + 2) sum_e (2 (1 + alpha) |rated_e - p_e| + 2 |p_e|) <|x^|, |y_e|> + (2 d + 2) |x^|^T |gram| |x^| ],
              p_e = <x^, y_e>,  T = (1 + alpha) sum_e (rated_e - p_e)^2 + sum_e p_e^2 + |x^|^T |gram| |x^|   (the sum's own error, then the carried
              error of every p_e and of the quadratic form's 2 d products)
An empty row must give x^ = 0 exactly."""
import numpy as np

U = 2.0 ** -24


gamma = lambda n: n * U / (1.0 - n * U)      # noqa: E731

def make_case(seed, d, N, lengths, rated_zeros=False):
    """(indptr int64, indices int32, table fp32 [N, d] ~ N(0, 0.1^2), rated fp32 | None) for rows of the given lengths."""
    rng = np.random.default_rng(seed)
    table = (rng.standard_normal((N, d)) * 0.1).astype(np.float32)
    indptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    indices = rng.integers(0, N, size=int(indptr[-1])).astype(np.int32)
    for s, e in zip(indptr[:-1], indptr[1:]):
        if e - s >= 2:
            indices[s + 1] = indices[s]                       # the same id twice in one row: counts twice
    return indptr, indices, table, (rng.random(len(indices)) < 0.7).astype(np.float32) if rated_zeros else None


def row_system(indptr, indices, table, gram, alpha, lam, rated, r):
    s, e = int(indptr[r]), int(indptr[r + 1])
    Y = table[indices[s:e]].astype(np.float64)
    w = np.ones(e - s) if rated is None else rated[s:e].astype(np.float64)
    d = table.shape[1]
    G = gram.astype(np.float64)
    A = alpha * Y.T @ Y + G + lam * np.eye(d)
    b = (1.0 + alpha) * (Y * w[:, None]).sum(0)
    return Y, w, G, A, b


def loss64(Y, w, G, alpha, x):
    p = Y @ x
    return (1.0 + alpha) * ((w - p) ** 2).sum() - (p ** 2).sum() + x @ G @ x


def loss_share(Y, w, G, alpha, xh, loss_hat, where=None):
    """Asserts bound 3 for one row at the float64 copy ``xh`` of the x the loss was taken with; -> the share of the bound used."""
    K, d = len(Y), len(xh)
    p = Y @ xh
    ax = np.abs(xh)
    quad = ax @ np.abs(G) @ ax
    T = (1.0 + alpha) * ((w - p) ** 2).sum() + (p ** 2).sum() + quad
    carried = ((2 * (1.0 + alpha) * np.abs(w - p) + 2 * np.abs(p)) * (np.abs(Y) @ ax)).sum()
    tol = U * ((K + 2) * T + (d + 2) * carried + (2 * d + 2) * quad)
    err = abs(loss_hat - loss64(Y, w, G, alpha, xh))
    assert err <= tol, ('loss', where, K, err, tol)
    return err / tol if tol > 0 else 0.0


def judge(indptr, indices, table, gram, alpha, lam, rated, rows, x_hat, loss_hat=None):
    """Asserts the three bounds for every solved row; -> the worst shares of the bounds {'backward', 'forward', 'loss', 'kappa_eta'} and
    'mean_loss', the mean over the rows of loss(x*)."""
    alpha, lam = float(np.float32(alpha)), float(np.float32(lam))
    d = table.shape[1]
    rows = np.arange(len(indptr) - 1) if rows is None else np.asarray(rows)
    worst = {'backward': 0.0, 'forward': 0.0, 'loss': 0.0, 'kappa_eta': 0.0, 'mean_loss': 0.0}
    for k, r in enumerate(rows):
        Y, w, G, A, b = row_system(indptr, indices, table, gram, alpha, lam, rated, r)
        K = len(Y)
        xh = x_hat[k].astype(np.float64)
        assert np.isfinite(xh).all() and (K > 0 or not x_hat[k].any()), (k, r)
        nA = np.linalg.norm(A, 2)
        EA = (K + 2) * U * (alpha * np.abs(Y).T @ np.abs(Y) + np.abs(G) + lam * np.eye(d))
        Eb = (K + 2) * U * (1.0 + alpha) * (np.abs(Y) * np.abs(w)[:, None]).sum(0)
        nb = np.linalg.norm(b)
        eta = max((np.linalg.norm(EA) + gamma(3 * d + 1) * d * nA / (1.0 - d * gamma(d + 1))) / nA,
                  np.linalg.norm(Eb) / nb if nb > 0 else 0.0)
        kappa = np.linalg.cond(A, 2)
        assert kappa * eta < 0.1, (k, r, K, kappa, eta)
        worst['kappa_eta'] = max(worst['kappa_eta'], kappa * eta)
        resid = np.linalg.norm(b - A @ xh)
        bound = eta * (nA * np.linalg.norm(xh) + nb)
        assert resid <= bound, ('backward', k, r, K, resid, bound)
        worst['backward'] = max(worst['backward'], resid / bound if bound > 0 else 0.0)
        xs = np.linalg.solve(A, b)
        worst['mean_loss'] += loss64(Y, w, G, alpha, xs) / len(rows)
        if nb > 0:
            fwd = np.linalg.norm(xh - xs) / np.linalg.norm(xs)
            fb = 2 * kappa * eta / (1 - kappa * eta)
            assert fwd <= fb, ('forward', k, r, K, fwd, fb)
            worst['forward'] = max(worst['forward'], fwd / fb)
        if loss_hat is not None:
            worst['loss'] = max(worst['loss'], loss_share(Y, w, G, alpha, xh, float(loss_hat[k]), (k, r)))
    return worst
