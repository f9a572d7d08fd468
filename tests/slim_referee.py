"""The float64 referee of SLIM (numpy, one target at a time): sklearn's ``enet_coordinate_descent_gram`` in cyclic order on
``Q = G`` without row and column j, ``q = G[:, j]`` without j, ``y.y = G[j, j]``, over ALL coordinates, and the KKT residual of a
weight vector; tests/test_slim.py holds it to sklearn itself.  A sweep jumps to the next coordinate whose value changes (the others
leave every quantity alone); once the state (w, g) after a sweep repeats an earlier one, whole periods are skipped."""
import numpy as np


def make_R(n_users, n_items, seed, top=0.6, power=0.7):
    """Seeded Bernoulli interactions with Zipf-like column densities ``top / rank^power``; row 0 and column 0 are the padding."""
    R = np.random.default_rng(seed).random((n_users, n_items)) < top / np.arange(1, n_items + 1)[None] ** power
    R[0], R[:, 0] = False, False
    return R


def problem(G, j):
    """``(q, diag Q, y.y)`` of target j; Q itself is G with row and column j zeroed (``Qw``)."""
    q, d = G[:, j].astype(np.float64), G.diagonal().astype(np.float64)
    q[j], d[j] = 0.0, 0.0
    return q, d, float(G[j, j])


def Qw(G, j, w):
    H = G @ np.where(np.arange(len(w)) == j, 0.0, w)
    H[j] = 0.0
    return H


def candidates(G, j, a):
    return np.array([k for k in range(1, len(G)) if k != j and G[k, j] > a], dtype=np.int64)


def gap_of(q, H, yy, w, a, b, positive=True):
    """The solver's duality gap at w, ``H = Q w``."""
    xta = q - H - b * w
    dual = xta.max() if positive else np.abs(xta).max()
    q_dot_w, r2 = w @ q, yy + w @ H - 2.0 * (w @ q)
    c, gap = 1.0, r2
    if dual > a:
        c = a / dual
        gap = 0.5 * (r2 + r2 * c * c)
    return gap + a * np.abs(w).sum() - c * yy + c * q_dot_w + 0.5 * b * (1.0 + c * c) * (w @ w)


def enet_gram(G, j, a, b, positive=True, max_iter=100, tol=1e-4, coords=None, margins=None):
    """-> ``(w, gap, n_iter)``.  ``coords``: restrict the sweep to these.  ``margins`` (a list) receives, per sweep walked,
    ``(d_w_max / w_max or None, gap or None)``: what the two stop tests compared with ``tol`` and ``tol * y.y``."""
    q, d, yy = problem(G, j)
    allowed = d != 0.0
    if coords is not None:
        allowed &= np.isin(np.arange(len(q)), coords)
    w, g, gap, it = np.zeros(len(q)), q.copy(), tol + 1.0, 0
    seen = {w.tobytes() + g.tobytes(): -1}
    while True:
        d_w_max, pos = 0.0, 0
        while True:
            tmp = g + w * d
            wn = np.sign(tmp) * np.maximum(np.abs(tmp) - a, 0.0) / (d + b)
            if positive:
                wn[tmp < 0] = 0.0
            delta = np.where(allowed, wn - w, 0.0)
            ahead = np.nonzero(delta[pos:])[0]
            if not len(ahead):
                break
            k = pos + ahead[0]
            w[k], pos, d_w_max = wn[k], k + 1, max(d_w_max, abs(delta[k]))
            row = G[k].astype(np.float64)
            row[j] = 0.0
            g -= row * delta[k]
        w_max = np.abs(w).max()
        ratio = d_w_max / w_max if w_max else None
        checked = w_max == 0.0 or ratio < tol or it == max_iter - 1
        if checked:
            gap = gap_of(q, q - g, yy, w, a, b, positive)
        if margins is not None:
            margins.append((ratio, gap if checked else None))
        if (checked and gap < tol * yy) or it == max_iter - 1:
            return w, gap, it + 1
        state = w.tobytes() + g.tobytes()
        if state in seen:
            period = it - seen[state]
            it += (max_iter - 2 - it) // period * period
        seen[state] = it
        it += 1


def kkt_violation(G, j, w, a, b):
    """``|q_k - (Q w)_k - b w_k - a|`` where w_k > 0, ``max(0, q_k - (Q w)_k - a)`` where w_k = 0; ``|w - w*|_2 <= |v|_2 / b``."""
    r = problem(G, j)[0] - Qw(G, j, w) - b * w - a
    return np.where(w > 0, np.abs(r), np.maximum(r, 0.0))
