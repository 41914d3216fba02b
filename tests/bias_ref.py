"""fp64 numpy reference of biased explicit ALS, r^ = mu + b_u + c_i + x_u . theta_i (include/cumf_bias_capi.h); no code of
the repository is used.

`direct_half` solves every row's bordered (f + 1)-unknown ridge problem with its own lambda_bias; `aug_half` solves the
same row as the plain ALS update at F = f + 2 on gather rows [theta | s | 0] and residual ratings, the form the library
runs.  `run` alternates either of them from the reference's start.
"""
import numpy as np


def planted_bias_ratings(m=300, n=200, density=0.15, rank=4, seed=7, empty=True, test_share=0.2, scale=0.5):
    """(R, train mask, test mask): ratings 3.5 + b_u + c_i + u_u . v_i + 0.1 N(0, 1) with planted biases and factors of
    standard deviation 0.5 (`scale` for the factors).  empty: row 5 and column 9 have no rating at all.  The defaults give
    7 184 train and 1 757 test ratings."""
    rng = np.random.RandomState(seed)
    mask = rng.random_sample((m, n)) < density
    if empty:
        mask[5, :] = False
        mask[:, 9] = False
    U = scale * rng.standard_normal((m, rank))
    V = scale * rng.standard_normal((n, rank))
    b = 0.5 * rng.standard_normal(m)
    c = 0.5 * rng.standard_normal(n)
    R = 3.5 + b[:, None] + c[None, :] + U @ V.T + 0.1 * rng.standard_normal((m, n))
    test = mask & (rng.random_sample((m, n)) < test_share)
    train = mask & ~test
    return R, train, test


def direct_half(R, train, mu, G, g_bias, lam, lam_b):
    """One half-iteration, row by row: minimise sum_i (r - mu - g_bias_i - b - x . G_i)^2 + n_u (lam |x|^2 + lam_b b^2).
    Returns (X rows x f, b rows); rows without ratings get 0."""
    rows, f = R.shape[0], G.shape[1]
    X, b = np.zeros((rows, f)), np.zeros(rows)
    for u in range(rows):
        idx = np.flatnonzero(train[u])
        if idx.size == 0:
            continue
        Z = np.hstack([G[idx], np.ones((idx.size, 1))])
        t = R[u, idx] - mu - g_bias[idx]
        A = Z.T @ Z + idx.size * np.diag([lam] * f + [lam_b])
        z = np.linalg.solve(A, Z.T @ t)
        X[u], b[u] = z[:f], z[f]
    return X, b


def aug_half(R, train, mu, G, g_bias, lam, lam_b):
    """The same half-iteration as the plain update at F = f + 2: gather rows [G_i | s | 0], s = sqrt(lam / lam_b), ratings
    (r - mu) - g_bias_i, lam n_u on the whole diagonal; x = z[:f], b = s z[f], z[f + 1] == 0."""
    rows, f = R.shape[0], G.shape[1]
    s = np.sqrt(lam / lam_b)
    GA = np.hstack([G, np.full((G.shape[0], 1), s), np.zeros((G.shape[0], 1))])
    X, b = np.zeros((rows, f)), np.zeros(rows)
    for u in range(rows):
        idx = np.flatnonzero(train[u])
        if idx.size == 0:
            continue
        g = GA[idx]
        t = (R[u, idx] - mu) - g_bias[idx]
        z = np.linalg.solve(g.T @ g + lam * idx.size * np.eye(f + 2), g.T @ t)
        assert z[f + 1] == 0.0
        X[u], b[u] = z[:f], s * z[f]
    return X, b


def predict(mu, X, b, T, c):
    return mu + b[:, None] + c[None, :] + X @ T.T


def rmse(R, mask, P):
    return float(np.sqrt(np.mean((R[mask] - P[mask]) ** 2))) if mask.any() else 0.0


def theta0(n, f):
    """The reference's start: 0.2 * uniform[0, 1) from RandomState(0)."""
    return 0.2 * np.random.RandomState(0).random_sample((n, f))


def run(iters=10, f=8, lam=0.05, lam_b=None, data=None, half=direct_half, trace=None):
    """`iters` alternating iterations (X side, then Theta side) from theta0, X = 0 and zero biases; mu is the training mean.
    Returns a dict with mu, X, b, T, c and the (train, test) RMSE.  trace: a list that receives (X, b, T, c) copies after
    every iteration."""
    R, train, test = planted_bias_ratings() if data is None else data
    lam_b = lam if lam_b is None else lam_b
    m, n = R.shape
    mu = float(R[train].mean())
    T, c = theta0(n, f), np.zeros(n)
    X, b = np.zeros((m, f)), np.zeros(m)
    for _ in range(iters):
        X, b = half(R, train, mu, T, c, lam, lam_b)
        T, c = half(R.T, train.T, mu, X, b, lam, lam_b)
        if trace is not None:
            trace.append((X.copy(), b.copy(), T.copy(), c.copy()))
    P = predict(mu, X, b, T, c)
    return {"mu": mu, "X": X, "b": b, "T": T, "c": c, "train_rmse": rmse(R, train, P), "test_rmse": rmse(R, test, P)}
