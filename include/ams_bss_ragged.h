/* ams_bss_ragged.h -- ragged BSS-eval: the C ABI of libams_bss_ragged.so (csrc/bss/bss_ragged.hip; gfx950 only).
 *
 * include/ams_bss_batch.h scores utterances of ONE common length per context and owns four hipFFT plans of that length.  These entry
 * points score R recordings of ANY lengths, each against K sets of estimates, in one call: the number of kernel launches is a function
 * of (S, K, F) only, there is no context, no FFT plan and no hipFFT / hipSOLVER on the link line.  The correlations and the projections
 * are computed in the time domain with v_mfma_f64_16x16x4_f64; the Gram matrices are factorised and solved by the batched blocked
 * Cholesky and triangular solves of csrc/bss/chol_batched.h, the header the batched path (ams_bss_batch.h) builds from too.  ams_bss.h
 * and ams_bss_batch.h are unchanged and keep their own version numbers.
 *
 * Conventions: 0 on success, <0 on error (-1 invalid argument, returned before anything is launched; -2 workspace too small, nothing
 * launched; -3 launch failure), as ams_bss_batch.h.  The entry points never allocate and never synchronise; they enqueue on the given
 * stream only; the caller owns every buffer.  All arrays are float64 (info: int32; tables: int64 / int32) on the device unless a
 * function says "host only".
 *
 * Definitions.
 *   R >= 1 recordings; recording r has L_r >= 1 samples.  S = nsrc in 1 .. 6, K = nsets in 1 .. 64, F = flen in 1 .. AMS_BSSR_MAX_FLEN.
 *   l_off [R + 1] int64    l_off[0] = 0, l_off[r + 1] = l_off[r] + L_r
 *   ref                    recording r's block [S, L_r] starts at element S l_off[r]
 *   est                    recording r's block [K, S, L_r] starts at element K S l_off[r]; estimate row e = k S + s (0 .. K S - 1)
 *   crit [R, K, 3, S, S]   crit[r][k][c][jest][jtrue], c = SDR, SIR, SAR: what ams_bssb_eval gives for recording r and set k
 *   info [R]               info[r] != 0 where a Gram matrix of recording r was not positive definite (a silent reference): the
 *                          criteria of THAT recording are NaN, the other recordings are unaffected
 *   Time is cut into blocks of AMS_BSSR_BLOCK samples; recording r has B_r = ceil((L_r + F - 1) / AMS_BSSR_BLOCK) blocks (the
 *   projections are L_r + F - 1 samples long).  b_off [R + 1] int64: b_off[r] = sum_{q < r} B_q; Btot = b_off[R] <= 2^31 - 1.
 *   tab [Btot, 2] int32    the work table: row b_off[r] + b is (r, b).  A workgroup reads its unit of work from it.
 * l_off, b_off and tab are device tables built on the host (ams_bssr_tables fills b_off and tab from l_off) and uploaded once per
 * layout.  The kernels TRUST the device tables: entries consistent with the definitions above and with the scalars R, F, Btot.
 *
 * Arithmetic per recording: oracle/bss_eval.py's, restated without the FFT (its n >= L + F - 1, so its circular correlations and
 * convolutions are the linear ones).  Samples outside 0 .. L_r - 1 are zero.
 *   Correlations  u(x, y)[m] = sum_t x[t] y[t + m], m = 0 .. F - 1, for every ordered pair of references and every (reference i,
 *                 estimate row e).  With rr_ij[m] = sum_t ref_i[t + m] ref_j[t]:  rr_ij[m] = u(ref_j, ref_i)[m] for m >= 0 and
 *                 u(ref_i, ref_j)[-m] for m < 0;  re_ie[k] = u(ref_i, est_e)[k].  Every lag of every pair is computed once and both
 *                 Gram blocks (i, j) and (j, i) are filled from it.
 *   Gram          G [S F, S F] column-major, block (i, j) element [a, b] = rr_ij[b - a];  Gj[i] = the diagonal block (i, i) [F, F];
 *                 Df[e][i F + k] = Dj[i][e][k] = re_ie[k]  -- the layouts of gram_kernel / rhs_kernel of csrc/bss/fft_path.h.
 *   Solves        Cf[e] = G^-1 Df[e] (filters of estimate e on all references), Cj[j][e] = Gj[j]^-1 Dj[j][e], in place.
 *   Projections   P_f(e)[t] = sum_i sum_k Cf_{e,i}[k] ref_i[t - k],  P_j(e)[t] = sum_k Cj_{j,e}[k] ref_j[t - k],  t = 0 .. L_r + F - 2,
 *                 never written to memory: the five sums of sums_kernel are taken where the projections are formed, through
 *                 s_true = ref_j, e_spat = P_j - s_true, e_interf = P_f - s_true - e_spat, e_artif = -s_true - e_spat - e_interf + est
 *                 (csrc/bss/criteria.h, one function for all paths).
 *   Criteria      10 log10(num / (den + 1e-12)), as crit_kernel (csrc/bss/criteria.h).
 * Summation order (fixed; no atomics on floating-point data; a result is a function of its recording's data only).
 *   Correlations: per (block, pair, tile of 256 lags) one workgroup of four waves.  The block is two halves of 2048 samples; a half is
 *   2048 / 4 + 4 MFMA steps of four consecutive tau (tau = t + lag mod 16); wave w takes the steps 129 w .. 129 w + 128 of each
 *   half, first half first, and adds its i-th step of a half (i = 0 .. 128) into accumulator i mod 4; a wave's total is
 *   (acc0 + acc1) + (acc2 + acc3); the four wave totals are added in order 0, 1, 2, 3.  The block partials of a recording are added
 *   sequentially in block order by a second launch.
 *   Projections: a tile of 256 outputs is one MFMA chain over kappa = -16 .. F - 1 in steps of four, the references in order i = 0 ..
 *   S - 1 for P_f.  Wave w takes tiles w, w + 4, w + 8, w + 12 of the block; a lane adds its 16 outputs (4 tiles x 4 registers) in that
 *   order; the 64 lanes of a wave by the halving tree v[l] += v[l + s], s = 32 .. 1; the wave totals in order; one row of five sums per
 *   (block, e, j).  The rows of a recording are added sequentially in block order by the last launch.
 */
#ifndef AMS_BSS_RAGGED_H
#define AMS_BSS_RAGGED_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define AMS_BSSR_BLOCK 4096    /* samples per block of the summation order */
#define AMS_BSSR_MAX_FLEN 1024 /* the filter and a block's halo are held in LDS */

int ams_bssr_abi_version(void); /* 1 */
int ams_bssr_block(void);       /* AMS_BSSR_BLOCK, for bindings that cannot read the macro */

/* Host only.  Btot for the HOST table l_off [R + 1] and flen; -1 for R < 1 or R > 65535, a NULL pointer, l_off[0] != 0, a recording of
 * fewer than one sample, flen outside 1 .. AMS_BSSR_MAX_FLEN, or more than 2^31 - 1 table rows in all. */
long ams_bssr_blocks(const int64_t* l_off, int R, int flen);

/* Host only.  Fills the HOST tables b_off [R + 1] and tab [Btot, 2] from the HOST table l_off; -1 where ams_bssr_blocks answers -1. */
int ams_bssr_tables(const int64_t* l_off, int R, int flen, int64_t* b_off, int32_t* tab);

/* Kernel launches of one ams_bssr_eval call: a function of (S, K, F) only -- 4 (correlations, their block sum, Gram, right-hand
 * sides) + (3 ceil(S F / 32) - 2) + (3 ceil(F / 32) - 2) (the two factorisations) + 4 (the solves) + 2 (projections and sums, criteria).
 * Two memsets of the pivot flags come on top.  -1 outside the domain. */
int ams_bssr_launches(int nsrc, int nsets, int flen);

/* Bytes of workspace for R recordings of Btot blocks in all: per recording 8 ((S F)^2 + S F^2) for the Gram matrices plus
 * 8 (2 K S^2 F + (S^2 + K S^2) F) for the right-hand sides and correlations, per block 8 ((S^2 + K S^2) F + 5 K S^2) for the partial
 * sums, each array rounded up to 256 bytes.  0 outside the domain. */
size_t ams_bssr_workspace_bytes(int R, int nsets, int nsrc, int flen, long Btot);

/* Scores R recordings.  ws: 8-byte aligned.  Counts the launches it enqueues and returns -3 if they are not ams_bssr_launches. */
int ams_bssr_eval(const double* ref, const double* est, const int64_t* l_off, const int64_t* b_off, const int32_t* tab, int R, int nsets,
                  int nsrc, int flen, long Btot, double* crit, int* info, void* ws, size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
