/*
 * cumf_topk_capi.h -- C ABI of top-k recommendation and ranking metrics of libALS.so.
 *
 * Top-k.  A query table Q (rows x f fp32, row-major), a candidate table C (ncand x f fp32), k, and optionally an exclusion
 * list per query: a CSR (excl_rowptr, rows + 1 entries; excl_colidx) of candidate indices, ascending within each row,
 * duplicates allowed.  The score of candidate c for query q is the fp32 fmaf chain in increasing j,
 *   s = +0.0f;  for j = 0 .. f - 1:  s = fmaf(Q[q,j], C[c,j], s),
 * which v_mfma_f32_16x16x4_f32 issued in increasing j reproduces bit for bit.  A candidate is eligible for q when it is not
 * in q's exclusion row and its score is not NaN.  Candidate a ranks before b when s_a > s_b, or s_a == s_b and a < b (a total
 * order: the result does not depend on how the work is cut).  Per query, ids (int32) and scores (fp32, the chain value) of
 * its k best eligible candidates, best first, row-major rows x k; slots beyond the eligible count get id -1 and score -inf.
 * A score of -0 is reported as +0.  A caller batches queries by offsetting Q and excl_rowptr (and ids, scores).
 *
 * Ranking metrics.  `ids` (rows x k, as cumf_topk writes them) against a held-out CSR per query (test_rowptr, rows + 1
 * entries; test_colidx ascending and unique within each row; test_val optional).  An entry is relevant when its value is
 * > 0, or always when test_val is NULL.  T_u = the relevant entries of row u, L_u = its ids; for every u with |T_u| >= 1:
 *   precision@k = |L_u n T_u| / k,   recall@k = |L_u n T_u| / |T_u|,
 *   NDCG@k = sum_{j : L_u[j] in T_u} 1 / log2(j + 2)  /  sum_{j < min(k, |T_u|)} 1 / log2(j + 2).
 * out4_f64 (4 DEVICE doubles) receives (number of such queries, mean precision, mean recall, mean NDCG); the means are 0
 * when no query counts.  fp64 accumulation, summed in query order.
 *
 * Conventions of cumf_als_capi.h: DEVICE pointers of the calling process, `stream` a hipStream_t passed as void* (NULL = the
 * default stream), 0 on success or a HIP error code after printing the reason to stderr, no CPU fallback.  Row pointers are
 * int32 or int64 (rowptr_is_64), as in cumf_plan_create.  Scope: 1 <= f <= 512, 1 <= k <= 128, 0 <= ncand < 2^31, one GPU;
 * anything else is refused.  Every result is bit-identical from run to run (no float atomics).
 */
#ifndef CUMF_TOPK_CAPI_H_
#define CUMF_TOPK_CAPI_H_

#ifdef __cplusplus
extern "C" {
#endif

/* 1 when cumf_topk takes (f, k): 1 <= f <= 512 and 1 <= k <= 128.  Host only. */
int cumf_topk_available(int f, int k);

/* The k best eligible candidates of each of the `rows` queries into ids / scores (rows x k each).  excl_rowptr and
 * excl_colidx are both NULL when nothing is excluded. */
int cumf_topk(const float* Q, long rows, const float* C, long ncand, int f, const void* excl_rowptr, int rowptr_is_64,
              const int* excl_colidx, int k, int* ids, float* scores, void* stream);

/* precision@k, recall@k and NDCG@k of `ids` (rows x k) against the held-out CSR; test_val may be NULL. */
int cumf_ranking_metrics(const int* ids, long rows, int k, const void* test_rowptr, int rowptr_is_64, const int* test_colidx,
                         const float* test_val, double* out4_f64, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CUMF_TOPK_CAPI_H_ */
