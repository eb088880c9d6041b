/*
 * nsg_score.h -- per-position language-model scores for the cover-text quality guard,
 * part of `libnsgcoder.so`.
 *
 * Replaces the two Hugging Face reductions the reference's guard metrics run over a text's logits:
 *   - LMScorer.score (src/neuralstego/metrics/lm_scorer.py:121-131): `model(**inputs, labels=ids).loss`, the
 *     mean over positions t < T-1 of  -log softmax(logits[t])[ids[t+1]];
 *   - avg_entropy (src/neuralstego/metrics/entropy.py:36-46): the mean over positions t < T-1 of
 *     -sum_j p_j log(p_j + 1e-12), p = softmax(logits[t]).
 * One wavefront streams one row of V logits once (HBM-bound), keeping an online max, sum of exponentials and
 * sum of p-weighted logits per lane; nll = lse - x[label] and entropy = lse - sum_j p_j x_j are produced in
 * float64 from fp32 partials (the 1e-12 inside the reference's log changes the entropy by < 1e-9 nats).
 */
#ifndef NSG_SCORE_H
#define NSG_SCORE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* d_logits: [nrows, ld] rows of dtype (0 = fp32, 1 = fp16, NS_DTYPE_*), V <= ld valid columns, 16-byte aligned
 * rows.  d_labels: [nrows] int32 target id per row, or a negative value for "no label" (nll written as 0).
 * d_nll, d_entropy: [nrows] float64 outputs (either may be NULL).  Returns 0 or a negative NS_ERR_* code. */
int ns_score_rows(const void* d_logits, int64_t ld, int64_t nrows, int V, int dtype, const int32_t* d_labels,
                  double* d_nll, double* d_entropy, void* hip_stream);

/* The head GEMM with the row scores as its epilogue: nll / entropy of the rows of softmax(x @ wt^T) without a
 * [M, V] logits array.  d_x: fp16 [M, K] (the ln_f rows), d_wt: fp16 [V, K] (K contiguous, as ns_lm_gemm takes it),
 * both 16-byte aligned with ldx, ldw multiples of 8.  The logit of (row, column) has the bits ns_lm_gemm stores with
 * NS_LM_EPI_STORE_F32 (one canonical MFMA chain); with logits_dtype == NS_DTYPE_F16 it is rounded to fp16 and widened
 * back first, as NS_LM_EPI_STORE followed by ns_score_rows sees it.  d_labels / d_nll / d_entropy as in ns_score_rows
 * (a label < 0 or >= V gives nll 0).  A workgroup reduces 128 rows over a span of column tiles into one fp32
 * (max, sum e, sum e x) per (row, span) in d_work; a second kernel merges a row's spans in ascending order in float64.
 * The span cut and every reduction order depend on V only: a row's outputs have the same bits at M = 1 and inside any
 * batch.  d_work: 16-byte aligned, at least ns_lm_head_score_work_bytes(M, V) bytes (contents are scratch).
 * Returns NS_ERR_CONFIG for a NULL d_x / d_wt / d_work, a misaligned pointer or stride or a short d_work; NS_OK
 * without a launch for M == 0 or both outputs NULL; NS_ERR_UNSUPPORTED for a K of more than one accumulator chain
 * (K > 1024) or no multiple of 64 -- the caller then runs ns_lm_gemm + ns_score_rows. */
int ns_lm_head_score(const void* d_x, int64_t ldx, const void* d_wt, int64_t ldw, int M, int V, int K,
                     int logits_dtype, const int32_t* d_labels, double* d_nll, double* d_entropy, void* d_work,
                     int64_t work_bytes, void* hip_stream);
int64_t ns_lm_head_score_work_bytes(int M, int V);

#ifdef __cplusplus
}
#endif

#endif /* NSG_SCORE_H */
