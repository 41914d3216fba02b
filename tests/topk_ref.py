"""numpy reference of top-k recommendation and ranking metrics (include/cumf_topk_capi.h), for tests/test_topk*.py.

`chain_scores` rounds the fp64 value of s + q_j c_j to fp32 after every j.  For "dyadic" data -- values +-(1 + m/128) 2^e,
e in [-3, 3] -- every product and partial sum is exact in fp64, so this is exactly the fmaf chain the kernel computes; on
other data it can differ from fmaf in the last bit (double rounding), rarely."""
import numpy as np


def dyadic(rng, shape):
    m = rng.randint(0, 128, size=shape)
    e = rng.randint(-3, 4, size=shape)
    sign = np.where(rng.random_sample(shape) < 0.5, -1.0, 1.0)
    return (sign * (1.0 + m / 128.0) * np.exp2(e)).astype(np.float32)


def chain_scores(Q, C):
    """rows x ncand fp32: s = +0; s = fl32(s + Q[q, j] C[c, j]) for j = 0 .. f - 1."""
    Q = np.asarray(Q, np.float32)
    C = np.asarray(C, np.float32)
    s = np.zeros((Q.shape[0], C.shape[0]), np.float32)
    acc = np.empty(s.shape, np.float64)
    for j in range(Q.shape[1]):
        np.multiply.outer(Q[:, j].astype(np.float64), C[:, j].astype(np.float64), out=acc)
        acc += s
        s = acc.astype(np.float32)
    return s


def topk(scores, k, exclude=None):
    """(ids int32, scores fp32) rows x k: per row the k best non-NaN, non-excluded candidates by (score desc, index asc);
    exclude: per row an iterable of candidate indices (or None)."""
    rows, n = scores.shape
    ids = np.full((rows, k), -1, np.int32)
    out = np.full((rows, k), -np.inf, np.float32)
    for q in range(rows):
        s = scores[q]
        ok = ~np.isnan(s)
        if exclude is not None and len(exclude[q]):
            ex = np.asarray(exclude[q], np.int64)
            ex = ex[(ex >= 0) & (ex < n)]
            ok[ex] = False
        idx = np.nonzero(ok)[0]
        order = idx[np.lexsort((idx, -s[idx].astype(np.float64)))][:k]
        ids[q, :len(order)] = order
        out[q, :len(order)] = s[order]
    return ids, out


def csr_rows(rowptr, colidx):
    rowptr = np.asarray(rowptr)
    return [np.asarray(colidx[rowptr[q]:rowptr[q + 1]]) for q in range(len(rowptr) - 1)]


def ranking_metrics(ids, rowptr, colidx, val=None):
    """(count, mean precision@k, mean recall@k, mean NDCG@k) over the queries with at least one relevant held-out entry."""
    rows, k = ids.shape
    gains = 1.0 / np.log2(np.arange(k) + 2.0)
    n, p, r, g = 0, 0.0, 0.0, 0.0
    for q in range(rows):
        cols = np.asarray(colidx[rowptr[q]:rowptr[q + 1]])
        if val is not None:
            cols = cols[np.asarray(val[rowptr[q]:rowptr[q + 1]]) > 0]
        t = len(cols)
        if t == 0:
            continue
        rel = set(int(c) for c in cols)
        hit = np.array([int(i) >= 0 and int(i) in rel for i in ids[q]])
        n += 1
        p += hit.sum() / k
        r += hit.sum() / t
        g += gains[hit].sum() / gains[:min(k, t)].sum()
    if n == 0:
        return 0, 0.0, 0.0, 0.0
    return n, p / n, r / n, g / n
