/* ams_kmeans_ragged_soft.h -- SOFT k-means over segments of different numbers of points: the C ABI of libams_kmeans_ragged_soft.so
 * (csrc/kmeans_ragged/kmeans_ragged_soft.hip; gfx950 only).
 *
 * ams_kmr_* (include/ams_kmeans_ragged.h) cluster R segments of any lengths with a HARD assignment; ams_kmeans_* with beta >= 0
 * (include/ams.h) run the soft assignment over b utterances of ONE common length, in a summation order that depends on b.  These entry
 * points run the soft assignment over R segments of any lengths at once, with a number of launches that does not depend on R, and every
 * segment comes out bit for bit as the same call gives it alone.  The other headers and libraries are unchanged.  The conventions are those
 * of ams.h: every entry point returns an ams_status, never allocates, never synchronises, enqueues on the given stream only; the caller owns
 * every buffer; AMS_E_INVALID_ARG is returned before anything is launched.
 *
 * Layout (that of ams_kmeans_ragged.h; the tables are the ones ams_kmr_tables builds).
 *   R >= 1 segments; segment r has P_r >= 1 points of E floats
 *   p_off [R + 1] int64   p_off[0] = 0, p_off[r + 1] = p_off[r] + P_r;  Ptot = p_off[R]
 *   xn [Ptot, E]          float32, ALREADY normalised, 16-byte aligned; segment r is rows p_off[r] .. p_off[r + 1]
 *   w [Ptot] or NULL      silence weights, laid out like the points
 *   G_r = ceil(P_r / 8192)  chunks of segment r;  g_off [R + 1] int64: g_off[r] = sum_{q < r} G_q;  Gtot = g_off[R]
 *   tab [4 Gtot, 4] int32   the work table of ams_kmr_tables; of the four rows of a chunk only the first, 4 (g_off[r] + g) = (r, g, 0, 0),
 *                           is read here
 *   init_idx [R tries, C] int32   row r tries + t: C distinct point indices RELATIVE to segment r, each in 0 .. P_r - 1
 *   centroids [R tries, C, E], inertia [R tries], best [R] int32, selected [R, C, E], masks [Ptot, C]
 * The kernels TRUST the device tables and init_idx.
 *
 * Semantics.  For every segment the run
 *     ams_kmrs_init, nb_iterations x ams_kmrs_iterate, ams_kmrs_inertia, ams_kmrs_select, ams_kmrs_masks
 * computes what oracle/kmeans.py::kmeans(X[None], idx, C, tries, iterations, beta, notsilent = w[None]) computes for it as a batch of one:
 *   labels   lab[l, c] = e_c / sum_c e_c,  e_c = exp(-beta w_l |x_l - cent_c|^2)   (no maximum is subtracted)
 *   update   cent_c = sum_l x_l w_l lab[l, c] / sum_l lab[l, c]                      (a silent point counts with 1 / C in every denominator)
 *   inertia  sum_c (sum_l |x_l - cent_c|^2 lab[l, c]) / (sum_l lab[l, c])            (labels with w, distances without)
 *   select   the FIRST minimum of the inertia over the tries; the first NaN if there is one (np.argmin)
 *   masks    assign_at_end on:  ams_kmrs_masks with w = NULL on the selected centroids
 *            assign_at_end off: ams_kmrs_masks with the run's w: the labels of the chosen try, recomputed from its centroids
 * |x - c|^2 is evaluated as |x|^2 - 2 <x, c> + |c|^2 and clamped at 0; the library is built WITH FMA contraction: like every soft mode
 * it is tolerance-tested against a float64 restatement of the oracle, not bit-specified against it.
 *
 * Summation order, restarted at each segment's first point (what makes a segment independent of its neighbours): chunks of 8192 points
 * of the segment; one workgroup of 256 lanes per (chunk, try); lane j adds its points j, j + 256, .. of the chunk in order; every wave
 * sums its 64 lanes by the halving tree v[j] += v[j + s], s = 32 .. 1; the four wave totals are added as (w0 + w1) + (w2 + w3); the
 * chunk partials are added in chunk order by the workgroup that stores the row's last partial (a ticket per row).  No atomics on
 * floating-point data, no waiting between workgroups.
 *
 * Domain: (E, C) in {40, 8} x {2 .. 6}; beta finite and >= 0; R >= 1; tries >= 1; Gtot >= R, 4 Gtot tries < 2^31; no NULL pointer except
 * w; cent_in != cent_out; AMS_E_INVALID_ARG otherwise.  A workspace below ams_kmrs_workspace_bytes is AMS_E_WORKSPACE_TOO_SMALL.
 */
#ifndef AMS_KMEANS_RAGGED_SOFT_H
#define AMS_KMEANS_RAGGED_SOFT_H
#include <stddef.h>
#include <stdint.h>
#include "ams.h" /* ams_status, AMS_OK, AMS_E_* */
#ifdef __cplusplus
extern "C" {
#endif

int ams_kmrs_abi_version(void); /* 1 */

/* Bytes of workspace of ams_kmrs_iterate / ams_kmrs_inertia: 4 tries Gtot C (E + 1) (0 for arguments outside the domain). */
size_t ams_kmrs_workspace_bytes(int R, int tries, long Gtot, int E, int C);

/* centroids[r tries + t, c, :] = xn[p_off[r] + init_idx[r tries + t, c], :].  One launch. */
ams_status ams_kmrs_init(const float* xn, const int64_t* p_off, const int32_t* init_idx, float* centroids, int R, int tries, int E, int C,
                         void* stream);

/* One soft iteration for all R tries rows: labels from cent_in, the new centroids to cent_out [R tries, C, E].  One launch.
 * tickets: R tries zeroed 32-bit words, left zero. */
ams_status ams_kmrs_iterate(const float* xn, const float* w, const int32_t* tab, const int64_t* p_off, const int64_t* g_off,
                            const float* cent_in, float* cent_out, int R, int tries, long Gtot, int E, int C, float beta, void* ws,
                            size_t ws_bytes, void* tickets, void* stream);

/* inertia [R tries] of the soft assignment to cent [R tries, C, E].  One launch.  tickets as above. */
ams_status ams_kmrs_inertia(const float* xn, const float* w, const int32_t* tab, const int64_t* p_off, const int64_t* g_off,
                            const float* cent, float* inertia, int R, int tries, long Gtot, int E, int C, float beta, void* ws,
                            size_t ws_bytes, void* tickets, void* stream);

/* best[r] = the first minimum of inertia[r tries ..]; selected[r] = centroids[r tries + best[r]].  One launch. */
ams_status ams_kmrs_select(const float* inertia, const float* centroids, int32_t* best, float* selected, int R, int tries, int E, int C,
                           void* stream);

/* masks [Ptot, C]: the soft labels of every point for cent [R, C, E] (one centroid set per segment).  One launch; nothing but the Ptot C
 * labels is written. */
ams_status ams_kmrs_masks(const float* xn, const float* w, const int32_t* tab, const int64_t* p_off, const int64_t* g_off,
                          const float* cent, float beta, float* masks, int R, long Gtot, int E, int C, void* stream);

#ifdef __cplusplus
}
#endif
#endif
