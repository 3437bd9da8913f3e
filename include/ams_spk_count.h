/* ams_spk_count.h -- choosing the number of clusters of every segment of a ragged point set: the C ABI of libams_spk_count.so
 * (csrc/spk_count/spk_count.hip; gfx950 only).
 *
 * ams_kmr_* (include/ams_kmeans_ragged.h) cluster R segments for ONE number of clusters C.  These entry points score the clusterings of
 * SEVERAL candidate numbers c_lo .. c_hi of the same segments in one sweep over the points and pick a number per segment, with a number
 * of launches that does not depend on R.  The other headers are unchanged and keep their version numbers; the conventions are those of
 * ams.h: every entry point returns an ams_status, never allocates, never synchronises, enqueues on the given stream only; the caller owns
 * every buffer; AMS_E_INVALID_ARG is returned before anything is launched.
 *
 * Definitions.  R, p_off, xn, w, g_off, tab, Ptot, Gtot as in include/ams_kmeans_ragged.h, and
 *   candidates  k = 0 .. ncand - 1 stand for C_k = c_lo + k clusters, 2 <= c_lo <= c_hi <= 6, ncand = c_hi - c_lo + 1; pre_k = sum_{j < k} C_j
 *   cent_all    float32: for k = 0 .. ncand - 1 one after the other, the centroids [R tries, C_k, E] of every try of candidate k (what
 *               ams_kmr_iterate left); candidate k starts at float R tries E pre_k
 *   inertia_all float32 [ncand, R tries]: the inertia of every try (ams_kmr_inertia)
 *   sel_all     float32: for k one after the other, [R, C_k, E]; candidate k starts at float R E pre_k
 *   score [R, ncand] float64, tries_out [R, ncand] int32
 * Try of candidate k of segment r: the FIRST try with the smallest FINITE inertia (a NaN or infinite inertia is skipped: an empty cluster
 * leaves a NaN centroid); -1 where no try is finite: the candidate is disqualified.
 * Score of a candidate (the simplified silhouette): with the chosen try's centroids every point has s = (d2 - d1) / d2, d1 <= d2 the two
 * smallest Euclidean distances sqrt(sum_e (x_e - c_e)^2) to the C_k centroids, s = 0 where d2 == 0; score = sum w s / sum w (w = 1 without
 * weights), -infinity for a disqualified candidate and where sum w == 0.  All arithmetic in float64 on the float32 inputs, differences
 * first.  Summation order, restarted at each segment's first point: chunks of 8192 points; lane j (0 .. 255) adds its points j, j + 256,
 * .. of the chunk in order; the 256 lanes by the halving tree v[j] += v[j + s], s = 128 .. 1; the chunk totals sequentially in chunk
 * order.  No atomics on floating-point data: a segment's result does not depend on its neighbours.
 * sel_all[k][r]: the centroids of the chosen try of candidate k; for a disqualified candidate those of the try ams_kmr_select picks (the
 * first NaN inertia, else the first minimum).
 * Count of segment r (ams_spkc_choose): the candidate with the largest score, the first maximum.  Every candidate at -infinity: count 1
 * and candidate -1 if lo == 1, else count c_lo and candidate 0.  lo == 1 and the best score below *min_score: count 1, candidate -1.
 *
 * Domain: E in {40, 8}; 2 <= c_lo <= c_hi <= 6; lo == 1 (then c_lo == 2 and min_score != NULL) or lo == c_lo; R >= 1; tries >= 1;
 * R <= Gtot, 4 Gtot < 2^31; no NULL pointer except w and min_score.  A workspace below ams_spkc_workspace_bytes is
 * AMS_E_WORKSPACE_TOO_SMALL.  The kernels TRUST the device tables.
 */
#ifndef AMS_SPK_COUNT_H
#define AMS_SPK_COUNT_H
#include <stddef.h>
#include <stdint.h>
#include "ams.h" /* ams_status, AMS_OK, AMS_E_* */
#ifdef __cplusplus
extern "C" {
#endif

int ams_spkc_abi_version(void); /* 1 */

/* Bytes of workspace of ams_spkc_score: 8 Gtot (ncand + 1) (0 for arguments outside the domain). */
size_t ams_spkc_workspace_bytes(int R, long Gtot, int E, int c_lo, int c_hi);

/* score, tries_out and sel_all of every segment and candidate.  Two launches: the sweep (one workgroup per chunk of the table; every point
 * is read once for all candidates) and the finish (one workgroup per segment). */
ams_status ams_spkc_score(const float* xn, const float* w, const int32_t* tab, const int64_t* p_off, const int64_t* g_off,
                          const float* cent_all, const float* inertia_all, int R, int tries, long Gtot, int E, int c_lo, int c_hi,
                          void* ws, size_t ws_bytes, double* score, int32_t* tries_out, float* sel_all, void* stream);

/* count [R] int32, cand [R] int32 and chosen [R, c_hi, E] (the chosen candidate's sel rows; rows >= count, and every row of candidate -1,
 * are zero).  min_score: a HOST pointer to one double, read before the launch, or NULL.  One launch. */
ams_status ams_spkc_choose(const double* score, const float* sel_all, int R, int E, int lo, int c_lo, int c_hi, const double* min_score,
                           int32_t* count, int32_t* cand, float* chosen, void* stream);

/* labels [Ptot] int32 from labels_all [ncand, Ptot] (ams_kmr_labels on sel_all[k], candidate after candidate): those of the segment's
 * chosen candidate; 0 for candidate -1.  One launch. */
ams_status ams_spkc_labels(const int32_t* labels_all, const int32_t* cand, const int32_t* tab, const int64_t* p_off, int R, long Gtot,
                           long Ptot, int c_lo, int c_hi, int32_t* labels, void* stream);

#ifdef __cplusplus
}
#endif
#endif
