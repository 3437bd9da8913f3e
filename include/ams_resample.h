/* ams_resample.h -- sample-rate conversion for whole recordings: the C ABI of libams_resample.so (csrc/resample/resample.hip; gfx950
 * only).
 *
 * A rational-ratio polyphase FIR resampler, with 16-bit-PCM decoding and the channel down-mix fused into its input side.
 * include/ams.h and include/ams_stitch.h are unchanged and keep their own version numbers; the conventions are those of ams.h: every
 * entry point returns an ams_status, never allocates, never synchronises, enqueues on the given stream only; the caller owns every
 * buffer; AMS_E_INVALID_ARG is returned before anything is launched.
 *
 * Definitions (the oracle is scipy.signal.resample_poly with its defaults).  For an input rate fi and an output rate fo:
 * g = gcd(fi, fo), up = fo / g, down = fi / g, m = max(up, down), half = 10 m.
 *   taps [20 m + 1]  a sinc with cutoff 1 / m of Nyquist, times a Kaiser window (beta 5.0), normalised to unit gain at DC, times up;
 *                    designed by the CALLER in float64 and rounded once to float32; a device table
 *   M              = ceil(N up / down)                                         output samples for N input samples
 *   y[n]           = sum_k taps[n down + half - k up] x[k]                      over 0 <= k < N with 0 <= n down + half - k up <= 2 half
 * (zero padding at both ends, zero phase: y is time-aligned with x).  The sum is float32, in increasing k; the product and the add
 * may be fused.  The same arguments give the same bits.  n down + half is formed in 64 bits.
 * Limits (AMS_E_INVALID_ARG otherwise): no NULL pointer (taps may be NULL for pcm16 with up = down = 1 only); up and down in 1 .. 1024
 * with gcd(up, down) = 1; ntaps = 20 max(up, down) + 1; channels in 1 .. 8; rows in 1 .. 65535; n_in >= 1 and M <= 2^38;
 * n_out = ams_resample_out_len(n_in, up, down); a stride not shorter than its row.
 */
#ifndef AMS_RESAMPLE_H
#define AMS_RESAMPLE_H
#include <stddef.h>
#include <stdint.h>
#include "ams.h" /* ams_status, AMS_OK, AMS_E_* */
#ifdef __cplusplus
extern "C" {
#endif

int ams_resample_abi_version(void); /* 1 */

/* M = ceil(n_in up / down); 0 for arguments outside the limits. */
long ams_resample_out_len(long n_in, int up, int down);

/* y [n_out] float32 from pcm [n_in, channels]: interleaved little-endian int16 frames.  The input sample is
 *   x[k] = (float)(sum_c pcm[k, c]) / (float)(32768 channels)          an int32 sum and one IEEE division,
 * formed inside the kernel and filtered as above; no intermediate float signal is written.  up = down = 1 is a pure decode / down-mix
 * (taps may be NULL, ntaps is then not looked at).  Kernels as for ams_resample_f32 with rows = 1; the decode-only kernel has grid
 * (ceil(n_in / 256)), 256 threads, one frame per thread.  int16 loads (2 bytes per lane and channel), any 2-byte-aligned base.
 * Bytes moved: 2 channels n_in read (the decimating arm reads 20 down / 256 frames more per workgroup), 4 n_out written, the taps
 * from cache. */
ams_status ams_resample_pcm16(const int16_t* pcm, long n_in, int channels, const float* taps, int ntaps, int up, int down, float* y,
                              long n_out, void* stream);

/* y [rows, n_out] from x [rows, n_in]: rows independent float32 rows, x_stride and y_stride elements from one row to the next.
 * Grid (ceil(n_out / 256), rows), 256 threads, one output sample per thread, no workspace, no atomics.
 *   down > up (decimation, 20 down / up + 1 taps per output): the workgroup stages the input samples its 256 outputs reach in LDS,
 *     4096 at a time (16 KB; (256 down + 20 down) / up + 2 samples, one round for every standard rate), each decoded / loaded once
 *     per workgroup with coalesced dword loads; a thread then walks its own contiguous span of them.
 *   up >= down (interpolation, at most 21 taps per output): neighbouring outputs read the same few input samples and walk the phases
 *     of the filter; every thread reads its <= 21 samples straight from memory (L1 hits), no LDS.
 * The taps are read through the cache in both arms (the table is at most 82 KB).  Dword accesses, any 4-byte-aligned base and stride.
 * Bytes moved: 4 rows n_in read (decimation: times 1 + 20 / 256), 4 rows n_out written. */
ams_status ams_resample_f32(const float* x, int rows, long n_in, long x_stride, const float* taps, int ntaps, int up, int down, float* y,
                            long n_out, long y_stride, void* stream);

#ifdef __cplusplus
}
#endif
#endif
