/* ams_kmeans_ragged.h -- hard k-means over segments of different numbers of points: the C ABI of libams_kmeans_ragged.so
 * (csrc/kmeans_ragged/kmeans_ragged.hip; gfx950 only).
 *
 * ams_kmeans_* (include/ams.h) cluster b utterances of ONE common length L per call.  These entry points cluster R segments of any
 * lengths at once -- the embeddings of R whole recordings, each a point set of its own -- with a number of launches that does not depend
 * on R.  include/ams.h is unchanged and keeps its own version number; the conventions are those of ams.h: every entry point returns an
 * ams_status, never allocates, never synchronises, enqueues on the given stream only; the caller owns every buffer; AMS_E_INVALID_ARG is
 * returned before anything is launched.
 *
 * Definitions.
 *   R >= 1 segments; segment r has P_r >= 1 points of E floats
 *   p_off [R + 1] int64   p_off[0] = 0, p_off[r + 1] = p_off[r] + P_r;  Ptot = p_off[R]
 *   xn [Ptot, E]          float32, ALREADY normalised (ams_kmeans_normalize is row-wise: it takes the packed layout as it is);
 *                         segment r is rows p_off[r] .. p_off[r + 1]
 *   w [Ptot] or NULL      silence weights, laid out like the points
 *   G_r = ceil(P_r / 8192)  chunks of segment r;  g_off [R + 1] int64: g_off[r] = sum_{q < r} G_q;  Gtot = g_off[R]
 *   tab [4 Gtot, 4] int32   the work table: row 4 (g_off[r] + g) + k is (r, g, k, 0) -- column k (0 .. 3: points 64 k .. 64 k + 63 of
 *                           every 256) of chunk g of segment r.  A workgroup reads its unit of work from it.
 *   init_idx [R tries, C] int32   row r tries + t: C distinct point indices RELATIVE to segment r, each in 0 .. P_r - 1
 *   centroids [R tries, C, E], inertia [R tries], best [R] int32, selected [R, C, E], labels [Ptot] int32
 * p_off, g_off and tab are device tables built on the host (ams_kmr_tables fills g_off and tab from p_off) and uploaded once per layout.
 * The kernels TRUST the device tables and init_idx: entries consistent with the definitions above and with the scalars R, Gtot, Pmax.
 *
 * Semantics: hard assignment only (the beta < 0 case of ams.h).  For every segment the run
 *     ams_kmr_init, nb_iterations x ams_kmr_iterate, ams_kmr_inertia, ams_kmr_select, ams_kmr_labels
 * gives, BIT FOR BIT, what ams_kmeans_init / _iterate / _assign / _select give for that segment alone as a batch of one (b = 1), which is
 * what oracle/kmeans.py::kmeans gives for it: the seed rows as initial centroids; one centroid update per iteration; the inertia of every
 * try and the FIRST minimum over the tries; silent points (w = 0) counted in the denominator and labelled 0; an empty cluster gives a NaN
 * centroid; the distance is the sum, left to right, of individually rounded squares (times w), compared after an IEEE sqrt, ties to the
 * lowest cluster.  The weight row of a segment is the segment's (with b = 1 the reference's weight-tile quirk does not arise).
 *   assign_at_end on:  ams_kmr_labels with w = NULL (the reference re-assigns without the silence weights)
 *   assign_at_end off: ams_kmr_labels with the run's w: the labels of the chosen try as its last pass assigned them
 * Summation order, restarted at each segment's first point: chunks of 8192 points of the segment; lane j (0 .. 255) adds its points
 * j, j + 256, .. of the chunk in order; every 64-lane column by the halving tree v[j] += v[j + s], s = 32 .. 1; the column totals are
 * added sequentially in (chunk, column) order.  No atomics on floating-point data, no waiting between workgroups: the workgroup that
 * stores a row's last partial adds the row up (a ticket per row).  The library is built with -ffp-contract=off.
 *
 * Domain: (E, C) in {40, 8} x {2 .. 6}; R >= 1; tries >= 1; 1 <= Gtot, 4 Gtot tries < 2^31; Pmax >= 1 (the largest P_r); no NULL pointer
 * except w; AMS_E_INVALID_ARG otherwise.  A workspace below ams_kmr_workspace_bytes is AMS_E_WORKSPACE_TOO_SMALL.
 * At E = 40, C = 2, tries a multiple of 5 and Pmax E 4 < 2^31, one read of a column's points serves five tries.
 */
#ifndef AMS_KMEANS_RAGGED_H
#define AMS_KMEANS_RAGGED_H
#include <stddef.h>
#include <stdint.h>
#include "ams.h" /* ams_status, AMS_OK, AMS_E_* */
#ifdef __cplusplus
extern "C" {
#endif

int ams_kmr_abi_version(void); /* 1 */

/* Host only.  Gtot for the HOST table p_off [R + 1]; -1 for R < 1, a NULL pointer, p_off[0] != 0, a segment of fewer than one point or
 * more than 2^31 - 1 chunk columns in all. */
long ams_kmr_chunks(const int64_t* p_off, int R);

/* Host only.  Fills the HOST tables g_off [R + 1] and tab [4 Gtot, 4] from the HOST table p_off; AMS_E_INVALID_ARG where ams_kmr_chunks
 * answers -1. */
ams_status ams_kmr_tables(const int64_t* p_off, int R, int64_t* g_off, int32_t* tab);

/* Bytes of workspace of ams_kmr_iterate / ams_kmr_inertia: 4 tries 4 Gtot C (E + 1) (0 for arguments outside the domain). */
size_t ams_kmr_workspace_bytes(int R, int tries, long Gtot, int E, int C);

/* centroids[r tries + t, c, :] = xn[p_off[r] + init_idx[r tries + t, c], :].  One launch. */
ams_status ams_kmr_init(const float* xn, const int64_t* p_off, const int32_t* init_idx, float* centroids, int R, int tries, int E, int C,
                        void* stream);

/* One Lloyd iteration for all R tries rows: labels from cent_in, the new centroids to cent_out [R tries, C, E].  One launch.
 * tickets: R tries zeroed 32-bit words, left zero. */
ams_status ams_kmr_iterate(const float* xn, const float* w, const int32_t* tab, const int64_t* p_off, const int64_t* g_off,
                           const float* cent_in, float* cent_out, int R, int tries, long Gtot, long Pmax, int E, int C, void* ws,
                           size_t ws_bytes, void* tickets, void* stream);

/* inertia [R tries] of the assignment to cent [R tries, C, E].  One launch. */
ams_status ams_kmr_inertia(const float* xn, const float* w, const int32_t* tab, const int64_t* p_off, const int64_t* g_off,
                           const float* cent, float* inertia, int R, int tries, long Gtot, long Pmax, int E, int C, void* ws,
                           size_t ws_bytes, void* tickets, void* stream);

/* best[r] = the first minimum of inertia[r tries ..]; selected[r] = centroids[r tries + best[r]].  One launch. */
ams_status ams_kmr_select(const float* inertia, const float* centroids, int32_t* best, float* selected, int R, int tries, int E, int C,
                          void* stream);

/* labels [Ptot] of the assignment to cent [R, C, E] (one centroid set per segment).  One launch; nothing but the Ptot labels is written. */
ams_status ams_kmr_labels(const float* xn, const float* w, const int32_t* tab, const int64_t* p_off, const int64_t* g_off,
                          const float* cent, int32_t* labels, int R, long Gtot, int E, int C, void* stream);

#ifdef __cplusplus
}
#endif
#endif
