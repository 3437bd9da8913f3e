/* ams_resample_ragged.h -- sample-rate conversion of many signals of mixed ratios in one launch: the C ABI of
 * libams_resample_ragged.so (csrc/resample/resample_ragged.hip; gfx950 only).
 *
 * ams_resample_* (include/ams_resample.h) convert ONE signal (rows of one length, one ratio) per launch.  These entry points convert J
 * signals of any lengths, ratios and channel counts in one launch.  include/ams.h and include/ams_resample.h are unchanged and keep their
 * own version numbers; the conventions are those of ams.h: every entry point returns an ams_status, never allocates, never synchronises,
 * enqueues on the given stream only; the caller owns every buffer; AMS_E_INVALID_ARG is returned before anything is launched.
 *
 * Definitions.  The arithmetic is that of include/ams_resample.h, from the same code (csrc/resample/resample_core.h):
 *   y[n] = sum_k taps[n down + half - k up] x[k], float32, in increasing k, every term one fused multiply-add; half = 10 max(up, down);
 *   a PCM frame is decoded as (float)(sum_c pcm[k, c]) / (float)(32768 channels); positions n down + half are 64-bit.
 * Every job is BIT FOR BIT what ams_resample_f32 / ams_resample_pcm16 give for that signal alone (cut to its first n_keep outputs).
 *
 * A JOB is one signal conversion: AMS_RSR_JOB_WORDS = 12 int64 words,
 *    0 src       where the signal starts: BYTES from the pointer x of the run call (any sign: a signal may lie anywhere on the device);
 *                a multiple of 4 (float32) or 2 (int16)
 *    1 n_in      input samples (frames) per row, >= 1
 *    2 rows      >= 1; 1 for int16 frames
 *    3 x_stride  elements from one input row to the next, >= n_in
 *    4 channels  0: float32 rows; 1 .. 8: interleaved little-endian int16 frames of that many channels
 *    5 up        1 .. 1024
 *    6 down      1 .. 1024, gcd(up, down) = 1
 *    7 tap_off   where this ratio's filter starts in the tap buffer: its 20 max(up, down) + 1 taps (designed as include/ams_resample.h says)
 *                lie at taps[tap_off ..] and must fit in taps_len; not looked at for up = down
 *    8 dst       where row 0 starts in the output buffer y, in floats, >= 0
 *    9 y_stride  floats from one output row to the next, >= n_keep
 *   10 n_keep    only the outputs 0 .. n_keep - 1 of every row are stored: 1 <= n_keep <= M = ceil(n_in up / down) <= 2^38
 *   11 reserved  (the device table holds ceil(n_keep / 256) here)
 * The outputs of different jobs must not overlap; every row must end inside y: dst + (rows - 1) y_stride + n_keep <= y_len.
 *
 * Work.  A workgroup (256 threads) makes 256 consecutive outputs of one row of one job; job j owns rows_j ceil(n_keep_j / 256)
 * consecutive workgroups of a 1-D grid.  The DEVICE TABLE, (J + 1) + 12 J int64 words, is
 *    prefix [J + 1]     prefix[0] = 0, prefix[j + 1] = prefix[j] + rows_j ceil(n_keep_j / 256); prefix[J] = the grid, < 2^31
 *    jobs   [J, 12]     the job records
 * built on the host by ams_rsr_tables and uploaded as ONE buffer.  A workgroup finds its job by a binary search of the prefix with
 * uniform (scalar) loads: table memory is proportional to J, never to the number of samples.  The arm is chosen per workgroup from its job:
 *    down > up   decimation: the input samples the tile's KEPT outputs reach go through LDS, 4096 per round, each loaded / decoded once
 *    up > down   interpolation: at most 21 samples per output, straight from memory
 *    up = down   int16: decode and down-mix only; float32: a copy
 * No atomics, no scratch, no workspace, and no store outside [dst, dst + n_keep) of a row.
 *
 * Limits (AMS_E_INVALID_ARG, ams_rsr_tiles: -1): J < 1; a NULL pointer; a job outside what the record above states; taps_len < 1; a tap
 * range that does not fit; a grid of 2^31 workgroups or more; for the run calls also y_len, a job of the other kind (channels = 0 for
 * ams_rsr_run_pcm16, channels >= 1 for ams_rsr_run_f32) and a src that is not a multiple of the element size.  The run calls check the
 * HOST job list and TRUST the device table to be what ams_rsr_tables made of the same list.
 */
#ifndef AMS_RESAMPLE_RAGGED_H
#define AMS_RESAMPLE_RAGGED_H
#include <stddef.h>
#include <stdint.h>
#include "ams.h" /* ams_status, AMS_OK, AMS_E_* */
#ifdef __cplusplus
extern "C" {
#endif

int ams_rsr_abi_version(void); /* 1 */

/* Host only.  The grid: sum_j rows_j ceil(n_keep_j / 256) for the HOST job list jobs [J, 12]; -1 outside the limits. */
long ams_rsr_tiles(const int64_t* jobs, int J, long taps_len);

/* Host only.  Fills the HOST buffer table [(J + 1) + 12 J] (prefix, then the records) from the HOST job list; AMS_E_INVALID_ARG where
 * ams_rsr_tiles answers -1. */
ams_status ams_rsr_tables(const int64_t* jobs, int J, long taps_len, int64_t* table);

/* One launch: every job (all of int16 frames) from x + src to y + dst.  jobs: the HOST list; table: the DEVICE copy of what
 * ams_rsr_tables made of it; taps: the DEVICE tap buffer of taps_len floats; y: y_len floats, of which only the kept outputs change.
 * Bytes moved: per job 2 channels n_in read (decimation: 20 down / 256 frames more per workgroup), 4 rows n_keep written. */
ams_status ams_rsr_run_pcm16(const int16_t* x, const float* taps, long taps_len, const int64_t* jobs, int J, const int64_t* table, float* y,
                             long y_len, void* stream);

/* One launch: every job (all of float32 rows).  Bytes moved: per job 4 rows n_in read (less where n_keep cuts the tail; decimation:
 * times 1 + 20 / 256), 4 rows n_keep written. */
ams_status ams_rsr_run_f32(const float* x, const float* taps, long taps_len, const int64_t* jobs, int J, const int64_t* table, float* y,
                           long y_len, void* stream);

#ifdef __cplusplus
}
#endif
#endif
