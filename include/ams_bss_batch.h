/* ams_bss_batch.h -- batched BSS-eval: the C ABI of the ams_bssb_* entry points of libams_bss.so.
 *
 * include/ams_bss.h scores ONE utterance against ONE set of estimates per call.  These entry points score `nutt` utterances,
 * each against `nsets` sets of estimates, in one call: the Gram matrices depend on the references only, so they are assembled
 * and factorised once per utterance and every set of estimates enters as right-hand sides.  The factorisation is this
 * library's own batched blocked Cholesky (float64 MFMA); there is no hipSOLVER on this path.  hipFFT stays as the FFT.
 *
 * All arrays are float64 (info: int32) on the device.  One context = one geometry (max_utt, nsets, nsrc, nsampl, flen); it owns
 * the hipFFT plans, nothing else -- scratch comes from the caller.  ams_bss.h is unchanged and keeps its own version number.
 */
#ifndef AMS_BSS_BATCH_H
#define AMS_BSS_BATCH_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef struct ams_bssb_ctx ams_bssb_ctx;

/* 0 on success, <0 on error (-1 invalid argument, -2 workspace too small, -3 launch / library failure), as ams_bss.h. */
int ams_bssb_abi_version(void);
int ams_bssb_create(ams_bssb_ctx** out, int max_utt, int nsets, int nsrc, int nsampl, int flen);
void ams_bssb_destroy(ams_bssb_ctx* ctx);
size_t ams_bssb_workspace_bytes(const ams_bssb_ctx* ctx);

/* 1 <= nutt <= max_utt.  ref: [nutt, nsrc, nsampl].  est: [nutt, nsets, nsrc, nsampl].  crit: [nutt, nsets, 3, nsrc, nsrc];
 * crit[u][k] is what ams_bss_eval_pairs(ref[u], est[u][k]) returns (crit[c][jest][jtrue]).  info: [nutt]; info[u] != 0 when a
 * Gram matrix of utterance u was not positive definite (a silent reference): the criteria of THAT utterance are NaN, the
 * others are unaffected.  A result depends on its utterance's data only (no atomics, fixed summation orders). */
int ams_bssb_eval(ams_bssb_ctx* ctx, int nutt, const double* ref, const double* est, double* crit, int* info, void* ws,
                  size_t ws_bytes, void* stream);

/* The factorisation on its own: nmat column-major symmetric positive definite matrices of order n (leading dimension lda,
 * `stride` elements apart), lower triangle read, lower Cholesky factor written in place, the strict upper triangle untouched.
 * info: [nmat] on the device; info[m] = 0, or the index of the first non-positive pivot + 1 (the factor of that matrix is
 * then NaN from that column on; the other matrices are unaffected). */
int ams_bssb_potrf(double* A, int n, int lda, long stride, int nmat, int* info, void* stream);

#ifdef __cplusplus
}
#endif
#endif
