/* ams_sisdr.h -- scale-invariant SDR of R recordings of ANY lengths and track counts against K sets of estimated tracks each, with the
 * best one-to-one matching of tracks to true sources: the C ABI of libams_sisdr.so (csrc/sisdr/sisdr.hip; gfx950 only).
 *
 * ams_bssr_* (include/ams_bss_ragged.h) need one number of sources for references and estimates, shared by the whole call.  These entry
 * points take a number of references Sr_r and, per set, a number of estimated tracks Se_rk that are free per recording, in TWO launches
 * whatever R is.  The other headers are unchanged and keep their version numbers; the conventions are those of ams.h: every entry point
 * returns an ams_status, never allocates, never synchronises, enqueues on the given stream only; the caller owns every buffer;
 * AMS_E_INVALID_ARG is returned before anything is launched.
 *
 * Definitions (the float64 restatement is tests/sisdr_ref.py).  Recording r has L_r samples and nrows_r = Sr_r + 1 +
 * sum_k Se_rk rows of float32: its references, its mixture, then the tracks of set 0, set 1, ..  (1 <= Sr, Se <= 6, 1 <= K <= 8, so
 * nrows <= 55).
 *   x     float32: the packed rows
 *   rows  int64 [R, 56]: the offset (in floats) of every row of the recording in x, in the order above; unused entries are not read
 *   rec   int64 [R, 4]:  {L_r, the recording's first block in the work table, 0, 0}
 *   cnt   int32 [R, 16]: {Sr_r, nrows_r, Se_r0 .. Se_r7, 0 ..}
 *   tab   int32 [Btot, 2]: the work table, one row (recording, block) per block of AMS_SISDR_BLOCK = 4096 samples, ceil(L_r / 4096) per
 *         recording, recordings and blocks ascending
 * With zero_mean != 0 every row has its mean over L_r removed.  For an estimate e and a reference s: g = <e,s>, ee = <e,e>, ss = <s,s>,
 *   si_sdr(e, s) = 10 log10(g^2 / (ss ee - g^2));  NaN where ss <= 0 (a silent reference: bit 0 of info[r] is set);  -infinity where
 *   ee <= 0 < ss;  +infinity where ss ee - g^2 <= 0.
 * Matching of set k: n = min(Se, Sr); the candidates are, in the order of itertools.permutations, the n-tuples of distinct indices out of
 * max(Se, Sr) -- the estimate of every reference if Se >= Sr, else the reference of every estimate; a candidate's value is the sum of
 * its pairs' si_sdr, added from 0.0 in tuple order; the first candidate takes the lead and a later one takes it only with a value that
 * compares greater.  A recording with info != 0 gets no matching.
 * Outputs, every word stored:
 *   pair      float64 [R, K, 6, 6] (estimate, reference), NaN outside [Se, Sr]
 *   match_ref int32 [R, K, 6] the estimate of every reference, match_est int32 [R, K, 6] the reference of every estimate; -1 where there
 *             is none
 *   si_sdr    float64 [R, K, 6] per reference, NaN where unmatched;  si_sdri = si_sdr - base
 *   missed, spurious int32 [R, K]: Sr - n and Se - n; 0 for a recording with info != 0
 *   base      float64 [R, 6] = si_sdr(mixture, s_j), NaN for j >= Sr;  info int32 [R]
 * Arithmetic: float64 on the float32 inputs, from the Gram products <u,v> of {references, mixture, a row of ones} with every row and every
 * row's own square; centring is <u,v> - sum(u) sum(v) / L.  Summation order, restarted at each recording: per block of 4096 samples,
 * tiles of T = 1024 / G samples (G = 1, 2, 4, 8 for nrows <= 7, 14, 28, 55); within a block sample phase p = 0 .. 256/G - 1 adds its
 * samples p, p + 256/G, .. of every tile in order by fused multiply-adds; the 32 phases of a half wave by the butterfly lanes l ^ 1, 2, 4,
 * 8, 16; the half waves in order; the blocks in ascending order.  No atomics on floating-point data: a recording's result is a function
 * of its own rows only.
 *
 * Domain: R >= 1; 1 <= K <= 8; R <= Btot < 2^31.  A workspace below ams_sisdr_workspace_bytes is AMS_E_WORKSPACE_TOO_SMALL.  The kernels
 * TRUST the device tables.
 */
#ifndef AMS_SISDR_H
#define AMS_SISDR_H
#include <stddef.h>
#include <stdint.h>
#include "ams.h" /* ams_status, AMS_OK, AMS_E_* */
#ifdef __cplusplus
extern "C" {
#endif

int ams_sisdr_abi_version(void); /* 1 */

/* AMS_SISDR_BLOCK: the samples per row of the work table. */
int ams_sisdr_block(void); /* 4096 */

/* Bytes of workspace of ams_sisdr_eval: one partial of 504 float64 per block (0 for arguments outside the domain). */
size_t ams_sisdr_workspace_bytes(int R, int K, long Btot);

/* Two launches: the Gram sweep (one workgroup per row of the table; every sample is read once) and the finish (one workgroup per
 * recording and set). */
ams_status ams_sisdr_eval(const float* x, const int64_t* rows, const int64_t* rec, const int32_t* cnt, const int32_t* tab, int R, int K,
                          long Btot, int zero_mean, void* ws, size_t ws_bytes, double* pair, int32_t* match_ref, int32_t* match_est,
                          double* si_sdr, double* si_sdri, int32_t* missed, int32_t* spurious, double* base, int32_t* info,
                          void* stream);

#ifdef __cplusplus
}
#endif
#endif
