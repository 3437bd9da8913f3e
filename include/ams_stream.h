/* ams_stream.h -- live streams: the C ABI of libams_stream.so (csrc/stream/stream.hip; gfx950 only).
 *
 * include/ams_stitch.h cuts, tracks and cross-fades a recording that is there in full.  These entry points do the same for streams that
 * arrive block by block: what a stream needs from its past (the samples no chunk has taken yet, the tail of its last chunk's estimate and
 * the track permutation of that chunk) lives in an opaque state buffer on the device, one slot per stream, and every push serves any
 * number of streams with a fixed number of launches.  The other headers and libraries are unchanged and keep their own version numbers;
 * the conventions are those of ams.h: every entry point returns an ams_status, never allocates, never synchronises, enqueues on the given
 * stream only; the caller owns every buffer; AMS_E_INVALID_ARG is returned before anything is launched.
 *
 * Definitions, on top of those of ams_stitch.h: L, H, V = L - H, S, w_head, perms, Q, rel, trk.  For one stream:
 *   N            samples received, D chunks done: both live on the HOST only; the device sees offsets inside one push
 *   pending      x[D H .. N): fewer than L samples after every push                               state, [L]
 *   tail         est[D - 1, :, H .. L) in the model's own source order                            state, [S, V]
 *   trk          the track permutation of chunk D - 1; the identity while D == 0                  state, [S]
 * One push is described by a table of n entries of AMS_STREAM_ENTRY int32 words, one per stream that takes part, built on the host and
 * uploaded with the push:
 *   [0] slot      the stream's slot of the state, 0 .. slots - 1, no slot twice in one table
 *   [1] x_off     where its new samples start in the packed buffer x          [2] k        how many there are (>= 0)
 *   [3] pend      samples pending before this push (N - D H, < L)            [4] rows     chunks this push cuts for it (>= 0)
 *   [5] row0      its first row of mix / est: rows row0 .. row0 + rows - 1   [6] out_off  where its output starts in every row of out
 *   [7] m         output samples of this push (>= 0)                         [8] flags    AMS_STREAM_FIRST | AMS_STREAM_CLOSING
 *   [9 .. 11]     0
 * AMS_STREAM_FIRST: D == 0 before this push: row row0 is chunk 0, which has no border in front of it.  AMS_STREAM_CLOSING: the stream
 * ends with this push: its last row may be short of samples and is filled with zeros, and m reaches past the last row's hop into its
 * tail (or, without a row, into the carried tail).  ams_hip/stream.py: plan() is this arithmetic.  The kernels skip an entry whose
 * numbers point outside the buffers the scalar arguments describe; they trust it otherwise.
 *
 * Bit contract.  Q of a border is BIT-EQUAL to ams_stitch_stats on the two chunk estimates on either side: the same slab of 1024 overlap
 * positions per workgroup, the same order (1) per thread over its positions, (2) the 64 lanes by the halving shuffle tree, (3) the four
 * waves through LDS in wave order, (4) the slabs in slab order, and the same alignment arm: 16-byte loads where L % 4 == 0, H % 4 == 0 and
 * est is 16-byte aligned (the state's own tail rows always are), dword loads otherwise.  rel is ams_stitch_tracks' search (<, the lowest
 * index among equals, a NaN cost never wins, all NaN: the identity) and the cross-fade is ams_stitch_ola's two rounded products and one
 * rounded add, so the concatenated output of a stream is bit-equal to ams_stitch_ola on the stream's estimates.  No atomics anywhere; no
 * launch reads state that another workgroup of the same launch writes; the library is built with -ffp-contract=off.
 *
 * Limits, the same for every entry point that takes the argument (AMS_E_INVALID_ARG otherwise, nothing launched): 1 <= slots <= 65535;
 * S in 1 .. 6; 2 <= L <= 2^30; ceil(L / 2) <= H <= L - 1; 1 <= n <= slots; 0 <= max_rows <= min(rows, 65535), rows <= 65535 n; the packed
 * sizes of a push, x_total and S out_stride, below 2^31; P = S!; state 16-byte aligned; no NULL pointer except where stated.  row0 of
 * entry s is the sum of the rows of the entries before it, out_off likewise of their m.
 */
#ifndef AMS_STREAM_H
#define AMS_STREAM_H
#include <stddef.h>
#include <stdint.h>
#include "ams.h" /* ams_status, AMS_OK, AMS_E_* */
#ifdef __cplusplus
extern "C" {
#endif

#define AMS_STREAM_ENTRY 12   /* int32 words per table entry */
#define AMS_STREAM_FIRST 1
#define AMS_STREAM_CLOSING 2

int ams_stream_abi_version(void); /* 1 */

/* Kernel launches this library has enqueued in this process so far (a host counter: the launch counts below can be checked). */
long ams_stream_launch_count(void);

/* Bytes of the opaque state of `slots` streams: per slot ceil4(L) floats of pending samples, S ceil4(V) of tail and 8 words of trk
 * (ceil4: rounded up to a multiple of 4, so that every row starts on a 16-byte boundary).  0 for arguments outside the limits. */
size_t ams_stream_state_bytes(int slots, int S, int L, int H);

/* Re-arms slots first .. first + count - 1: pending and tail become zeros, trk the identity.  Nothing of an earlier stream survives.
 * One launch: grid (count), 256 threads. */
ams_status ams_stream_reset(void* state, int slots, int S, int L, int H, int first, int count, void* stream);

/* Appends every stream's new samples and cuts the chunks that are ready: row row0 + j of mix [rows, L] is the stream's pending samples
 * followed by its new ones, from j H on, zeros past their end (a closing chunk).  Two launches: (1) grid (ceil(L / 1024), max(max_rows, 1),
 * n), 256 threads: the rows, from the OLD pending samples and x; (2) grid (ceil(L / 1024), n): the new pending samples, from the last
 * row of mix just written and x -- or, for a stream without a row, x appended behind what is pending.  x: the packed new samples
 * [x_total] (not NULL even if x_total == 0); mix may be NULL where rows == 0.  Dword accesses, any base.
 * Bytes moved: 4 (rows L + sum k) read, 4 rows L + 4 sum min(L, pend + k) written, 48 bytes of table per workgroup from cache. */
ams_status ams_stream_feed(void* state, int slots, int S, int L, int H, const int32_t* table, int n, int rows, int max_rows,
                           const float* x, long x_total, float* mix, void* stream);

/* Bytes of workspace ams_stream_absorb needs: rows ceil(V / 1024) S S floats of slab sums and (rows + n) S words of tracks. */
size_t ams_stream_workspace_bytes(int n, int rows, int S, int L, int H);

/* Takes est [rows, S, L] of the rows ams_stream_feed cut (same table) and writes every stream's output [S, m] at out[k out_stride +
 * out_off + i].  Four launches: (1) grid (ceil(V / 1024), max(max_rows, 1), n), 256 threads: the slab sums of every row's border with
 * the row before it -- the carried tail for a stream's first row, none for chunk 0; (2) grid (n), 256 threads: a workgroup per stream
 * walks its rows: Q in slab order, the search, trk <- rel[trk], into the workspace and the state; (3) grid (max(ceil(max_m / 1024), 1),
 * n, S), 256 threads: cross-fade and copy; (4) grid (ceil(V / 1024), n, S): the new tails.  Q_rows [rows, S, S] and trk_rows [rows, S]
 * (either may be NULL) also receive every row's Q (zeros for chunk 0) and trk.  est may be NULL where rows == 0.
 * Bytes moved: 8 rows S V for the borders, 4 S (sum m + rows V) of est read, 4 S sum m of out and 4 S V per stream of tails written. */
ams_status ams_stream_absorb(void* state, int slots, int S, int L, int H, const int32_t* table, int n, int rows, int max_rows, long max_m,
                             const float* est, const int32_t* perms, int P, const float* w_head, float* out, long out_stride, void* ws,
                             size_t ws_bytes, float* Q_rows, int32_t* trk_rows, void* stream);

#ifdef __cplusplus
}
#endif
#endif
