/* ams_kmeans_seed.h -- k-means++ (D^2) seeding of every segment of a ragged point set: the C ABI of libams_kmeans_seed.so
 * (csrc/kmeans_seed/kmeans_seed.hip; gfx950 only).
 *
 * ams_kmr_* (include/ams_kmeans_ragged.h), ams_kmrs_* and ams_spkc_* start every try of a segment from C seed points the HOST names.  These
 * entry points choose such seeds on the device, try by try, by sampling in proportion to the squared distance to the seeds chosen so far,
 * with a number of launches that does not depend on R.  They only produce indices: the other headers and libraries are unchanged and keep
 * their version numbers.  The conventions are those of ams.h: every entry point returns an ams_status, never allocates, never
 * synchronises, enqueues on the given stream only; the caller owns every buffer; AMS_E_INVALID_ARG is returned before anything is launched.
 *
 * Definitions.  R, p_off, xn, w, g_off, tab, Ptot, Gtot as in include/ams_kmeans_ragged.h (w NULL: every weight is 1), and
 *   draws  uint64 [R tries, C] on the device: u[r, t, c], the one random number step c of try t of segment r consumes
 *   seeds  int32  [R tries, C] on the device: row r tries + t holds the C seeds of try t of segment r, relative to the segment
 * The sampling weights are INTEGERS, so every sum below is exact in 64 bits, no order of addition matters, and the seeds are a function of
 * the inputs alone:
 *   d(i, s)   = sum over e = 0 .. E - 1, left to right, of round(round((xn[i, e] - xn[s, e])^2) w[i]) in float32: the hard distance of
 *               oracle/kmeans.py (sqdist) of point i to point s under the weight of point i (no FMA contraction in this library)
 *   quant(v)  = 0 if v is a NaN or v <= 0, else the truncation to uint32 of min(v, 2048.0f) * 1048576.0f (a power of two: the product is
 *               exact; quant <= 2^31)
 *   q_i at step 0      = quant(w[i])    (2^20 for every point without weights)
 *   q_i at step c >= 1 = min over the c seeds s chosen so far of quant(d(i, s)), the minimum of the integers
 *               (a chosen point, its exact duplicates, every point of weight 0 and every point with a NaN coordinate have q = 0)
 *   total     = sum over the segment's points of q_i (uint64; Ptot 2^31 < 2^64)
 *   seed c    = if total > 0: with target = floor(u[r, t, c] total / 2^64), the smallest i whose inclusive prefix sum q_0 + .. + q_i
 *               exceeds target; if total == 0: the smallest index of the segment that is not among seeds 0 .. c - 1 of this (r, t)
 * The C seeds of a row are distinct and in 0 .. P_r - 1 whenever P_r >= C; a CALLER'S duty (the kernels trust the tables).  Seeds are
 * sequential: columns 0 .. C' - 1 of a seeding for C clusters are the seeding for C' clusters from draw columns 0 .. C' - 1.
 *
 * Domain: E in {40, 8}; 1 <= C <= 6; R >= 1; tries >= 1; R <= Gtot, 4 Gtot < 2^31; P_r >= C for every segment; no NULL pointer except w.
 * A workspace below ams_kms_workspace_bytes is AMS_E_WORKSPACE_TOO_SMALL.  The kernels TRUST the device tables.
 */
#ifndef AMS_KMEANS_SEED_H
#define AMS_KMEANS_SEED_H
#include <stddef.h>
#include <stdint.h>
#include "ams.h" /* ams_status, AMS_OK, AMS_E_* */
#ifdef __cplusplus
extern "C" {
#endif

int ams_kms_abi_version(void); /* 1 */

/* Bytes of workspace of ams_kms_step and ams_kms_seed: 8 Gtot tries, the exact chunk sums of every try (0 for arguments outside the
 * domain). */
size_t ams_kms_workspace_bytes(int R, int tries, long Gtot, int E, int C);

/* Step c (0 <= c < C) of every try of every segment: column c of seeds from columns 0 .. c - 1.  Two launches: the weighing (one
 * workgroup per chunk of the table; every point is read once for up to 16 tries, and the chunk's sum of q goes to the workspace by one
 * plain store per try) and the pick (one workgroup per segment and try: the chunk that holds the target from the chunk sums, that one
 * chunk's q again and a prefix scan in point order).  No atomics. */
ams_status ams_kms_step(const float* xn, const float* w, const int32_t* tab, const int64_t* p_off, const int64_t* g_off,
                        const uint64_t* draws, int R, int tries, long Gtot, int E, int C, int c, void* ws, size_t ws_bytes, int32_t* seeds,
                        void* stream);

/* Steps 0 .. C - 1 one after the other: 2 C launches. */
ams_status ams_kms_seed(const float* xn, const float* w, const int32_t* tab, const int64_t* p_off, const int64_t* g_off,
                        const uint64_t* draws, int R, int tries, long Gtot, int E, int C, void* ws, size_t ws_bytes, int32_t* seeds,
                        void* stream);

#ifdef __cplusplus
}
#endif
#endif
