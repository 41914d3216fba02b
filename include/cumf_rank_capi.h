/*
 * cumf_rank_capi.h -- C ABI of full-ranking evaluation of libALS.so: the rank of every held-out entry among all eligible
 * candidates, and AUC, MPR, MRR, MAP and precision / recall / NDCG at any cut-off from those ranks.  The rows x ncand score
 * matrix is never written.
 *
 * Scores, eligibility and order are those of cumf_topk_capi.h.  A query table Q (rows x f fp32, row-major), a candidate
 * table C (ncand x f fp32), and optionally an exclusion list per query: a CSR (excl_rowptr, rows + 1 entries; excl_colidx)
 * of candidate indices, ascending within each row, duplicates allowed.  The score of candidate c for query q is the fp32
 * fmaf chain in increasing j,
 *   s = +0.0f;  for j = 0 .. f - 1:  s = fmaf(Q[q,j], C[c,j], s),
 * with -0 taken as +0.  A candidate is eligible for q when it is not in q's exclusion row and its score is not NaN.
 * Candidate a ranks before b when s_a > s_b, or s_a == s_b and a < b (a total order).
 *
 * Held-out ranks.  A held-out CSR per query (test_rowptr, rows + 1 entries; test_colidx ascending and unique within each
 * row); n_test is the number of entries of test_colidx, and the entries of the call are those from test_rowptr[0] up to
 * test_rowptr[rows] <= n_test.  cumf_heldout_ranks writes
 *   ranks       int32, parallel to test_colidx (n_test entries; those outside the call's rows are left alone): for a
 *               held-out entry (q, t) the number of eligible candidates c != t that rank before t, so the best position is
 *               rank 0; -1 when t is outside [0, ncand) or not eligible for q (excluded, or its score NaN);
 *   n_eligible  int32 per query: its eligible candidates.
 * For any k <= 128, ranks[e] == j < k exactly when cumf_topk's ids[q, j] == t.  A caller batches queries by offsetting Q, the
 * row pointers and n_eligible; test_colidx and ranks keep their base.
 *
 * Metrics.  cumf_rank_metrics reduces ranks, n_eligible, test_rowptr, the optional test_val and n_k cut-offs ks (a HOST
 * array, each >= 1, at most 16 of them, no cap of 128) to DEVICE doubles.  For query u, P_u is the set of its held-out
 * entries that are relevant (value > 0, or all when test_val is NULL) and have rank >= 0; p = |P_u|, N = n_eligible[u], and
 * r_1 < ... < r_p are the ranks of P_u in ascending order (distinct: the order is total).  Held-out entries that are not
 * relevant are ordinary candidates.
 *   queries      = #{u : p >= 1}; every mean below is over these queries, except AUC and MPR
 *   AUC_u        = 1 - sum_j (r_j - (j - 1)) / (p (N - p)); the mean is over the auc_queries = #{u : p >= 1 and N > p}
 *   MPR          = sum_{u, e in P_u} w_e r_e / (N_u - 1)  /  sum w_e, w = test_val (1 without values), the expected
 *                  percentile rank of Hu, Koren and Volinsky: 0 is best, about 0.5 random; entries of queries with
 *                  N_u <= 1 are left out
 *   MRR_u        = 1 / (1 + r_1)
 *   AP_u         = (1 / p) sum_j j / (r_j + 1); MAP is its mean
 *   per cut-off k, with h = #{j : r_j < k}:  precision@k = h / k,  recall@k = h / p,
 *                  NDCG@k = sum_{r_j < k} 1 / log2(r_j + 2)  /  sum_{j < min(k, p)} 1 / log2(j + 2)
 * out_f64 (6 + 3 n_k doubles) receives (queries, auc_queries, AUC, MPR, MRR, MAP), then (precision, recall, NDCG) per
 * cut-off in the order of ks.  Every mean is 0 when nothing counts.  fp64 accumulation, summed in query order.
 * Against cumf_ranking_metrics of cumf_topk's lists at the same k: there |T_u| counts every relevant held-out entry, here p
 * counts those with a rank, so the two differ only for held-out entries that are also excluded (train n test) or outside
 * the table.
 *
 * Conventions of cumf_als_capi.h: DEVICE pointers of the calling process unless marked HOST, `stream` a hipStream_t passed
 * as void* (NULL = the default stream), 0 on success or a HIP error code after printing the reason to stderr, no CPU
 * fallback.  Row pointers are int32 or int64, one flag per CSR.  Scope: 1 <= f <= 512, 0 <= ncand < 2^31, one GPU, any
 * number of held-out entries per query; anything else is refused.  Every result is bit-identical from run to run and does
 * not depend on how the work is cut (integer atomics only).
 */
#ifndef CUMF_RANK_CAPI_H_
#define CUMF_RANK_CAPI_H_

#ifdef __cplusplus
extern "C" {
#endif

/* 1 when cumf_heldout_ranks takes f: 1 <= f <= 512.  Host only. */
int cumf_rank_available(int f);

/* ranks (n_test) and n_eligible (rows) of the held-out CSR.  excl_rowptr and excl_colidx are both NULL when nothing is
 * excluded. */
int cumf_heldout_ranks(const float* Q, long rows, const float* C, long ncand, int f, const void* excl_rowptr,
                       int excl_rowptr_is_64, const int* excl_colidx, const void* test_rowptr, int test_rowptr_is_64,
                       const int* test_colidx, long n_test, int* ranks, int* n_eligible, void* stream);

/* The metrics of `ranks` / `n_eligible` as cumf_heldout_ranks writes them; test_val may be NULL; ks is a HOST array. */
int cumf_rank_metrics(const int* ranks, const int* n_eligible, long rows, const void* test_rowptr, int rowptr_is_64,
                      const float* test_val, long n_test, const int* ks, int n_k, double* out_f64, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CUMF_RANK_CAPI_H_ */
