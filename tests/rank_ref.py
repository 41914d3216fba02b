"""numpy reference of full-ranking evaluation (include/cumf_rank_capi.h), for tests/test_rank*.py.  Scores come from
`topk_ref.chain_scores`, so on dyadic data the ranks are exactly what the kernels must give."""
import numpy as np


def heldout_ranks(scores, test_rowptr, test_colidx, exclude=None):
    """(ranks int32 parallel to test_colidx, n_eligible int32 per row) of a rows x ncand score matrix: the rank of a held-out
    entry (q, t) is the number of eligible candidates c != t with (score desc, index asc) before t; -1 when t is outside
    the table or not eligible.  exclude: per row an iterable of candidate indices (or None)."""
    rows, n = scores.shape
    test_rowptr = np.asarray(test_rowptr, np.int64)
    ranks = np.full(len(test_colidx), -1, np.int32)
    n_eligible = np.zeros(rows, np.int32)
    for q in range(rows):
        s = scores[q]
        ok = ~np.isnan(s)
        if exclude is not None and len(exclude[q]):
            ex = np.asarray(exclude[q], np.int64)
            ok[ex[(ex >= 0) & (ex < n)]] = False
        n_eligible[q] = ok.sum()
        idx = np.nonzero(ok)[0]
        se = s[idx].astype(np.float64) + 0.0
        for e in range(test_rowptr[q], test_rowptr[q + 1]):
            t = int(test_colidx[e])
            if 0 <= t < n and ok[t]:
                st = np.float64(s[t])
                ranks[e] = int(((se > st) | ((se == st) & (idx < t))).sum())
    return ranks, n_eligible


def rank_metrics(ranks, n_eligible, test_rowptr, test_val=None, ks=()):
    """dict of the metrics of cumf_rank_metrics, accumulated in fp64 in query order."""
    rows = len(n_eligible)
    nq = na = 0
    auc = mprn = mprw = mrr = ap = 0.0
    per_k = {k: [0.0, 0.0, 0.0] for k in ks}
    for u in range(rows):
        a, b = int(test_rowptr[u]), int(test_rowptr[u + 1])
        r = np.asarray(ranks[a:b], np.int64)
        w = np.ones(b - a) if test_val is None else np.asarray(test_val[a:b], np.float64)
        keep = (r >= 0) if test_val is None else (r >= 0) & (w > 0)
        r, w = r[keep], w[keep]
        order = np.argsort(r, kind="stable")
        r, w = r[order], w[order]
        p, N = len(r), int(n_eligible[u])
        if p == 0:
            continue
        nq += 1
        j = np.arange(p)
        if N > p:
            na += 1
            auc += 1.0 - float((r - j).sum()) / (p * (N - p))
        if N > 1:
            mprn += float((w * r / (N - 1.0)).sum())
            mprw += float(w.sum())
        mrr += 1.0 / (1.0 + r[0])
        ap += float(((j + 1) / (r + 1.0)).sum()) / p
        for k in ks:
            hit = r < k
            per_k[k][0] += hit.sum() / k
            per_k[k][1] += hit.sum() / p
            per_k[k][2] += (1.0 / np.log2(r[hit] + 2.0)).sum() / (1.0 / np.log2(np.arange(min(k, p)) + 2.0)).sum()
    mean = lambda x, n: x / n if n else 0.0  # noqa: E731
    return {"queries": nq, "auc_queries": na, "auc": mean(auc, na), "mpr": mean(mprn, mprw), "mrr": mean(mrr, nq),
            "map": mean(ap, nq), "precision": {k: mean(v[0], nq) for k, v in per_k.items()},
            "recall": {k: mean(v[1], nq) for k, v in per_k.items()}, "ndcg": {k: mean(v[2], nq) for k, v in per_k.items()}}
