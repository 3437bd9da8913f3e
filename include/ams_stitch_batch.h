/* ams_stitch_batch.h -- many recordings in one call: the C ABI of libams_stitch_batch.so (csrc/stitch/stitch_batch.hip; gfx950 only).
 *
 * include/ams_stitch.h cuts, tracks and cross-fades ONE recording per call.  These entry points do the same for R recordings of any
 * lengths at once: their chunks form one stream that a model separates in full batches, and every entry point uses a fixed number of
 * launches whatever R is.  include/ams.h and include/ams_stitch.h are unchanged and keep their own version numbers; the conventions are
 * those of ams.h: every entry point returns an ams_status, never allocates, never synchronises, enqueues on the given stream only; the
 * caller owns every buffer; AMS_E_INVALID_ARG is returned before anything is launched.
 *
 * Definitions, on top of those of ams_stitch.h, which hold unchanged inside every recording: L, H, V = L - H, S, mix,
 * est, Q, rel, trk, out, w_head, perms.
 *   R >= 1 recordings, n[r] >= 1 samples each
 *   C_r          = 1 + max(0, ceil((n[r] - L) / H))                     chunks of recording r
 *   c_off[r]     = sum_{q < r} C_q,  Ctot = c_off[R]                    global chunk g = c_off[r] + c;  c_off has R + 1 entries
 *   chunk_rec[g] = r                                                    [Ctot] int32
 *   x            one float32 buffer: recording r is x[x_off[r] .. x_off[r] + n[r])           x_off[r] % 4 == 0
 *   out          one float32 buffer: recording r's block [S, n[r]], row-major, is at out_off[r]   out_off[r] % 4 == 0
 *   blk_off[r]   = sum_{q < r} ceil(n[q] / 1024),  nblk = blk_off[R]    1024-sample blocks of the cross-fade;  R + 1 entries
 *   blk_rec[b]   = r                                                    [nblk] int32
 *   mix[g, l]    = x[x_off[r] + c H + l] where c H + l < n[r], else 0   [Ctot, L]
 *   Q[g]         the border between chunks g and g + 1 where chunk_rec[g] == chunk_rec[g + 1] (a real border): ams_stitch.h's
 *                Q[c] of that recording; the row of a recording's last chunk is written as exact zeros                 [Ctot, S, S]
 *   rel[g]       ams_stitch.h's rel[c] on a real border (same table, <, lowest index among equals, NaN rules); the identity on a
 *                recording's last chunk                                                                              [Ctot, S]
 *   trk[g]       trk[c_off[r], k] = k, trk[g + 1, k] = rel[g][trk[g, k]] inside recording r only: no chain crosses a recording  [Ctot, S]
 *   out block r  ams_stitch.h's cross-fade of est[c_off[r] .. c_off[r + 1]) with trk[c_off[r] ..]: out[out_off[r] + k n[r] + m]
 * n, x_off, out_off, c_off, blk_off are int64 device tables, chunk_rec and blk_rec int32 device tables; the caller knows the lengths on
 * the host, builds the tables there and uploads them once (ams_hip/stitch_batch.py: layout).  The kernels TRUST the tables: entries
 * consistent with the definitions above and with the scalar arguments R, Ctot, nblk; only the scalars are checked.
 *
 * Bit contract.  For every recording the rows of mix, Q (real borders), rel, trk and the output block are BIT-EQUAL to what
 * libams_stitch.so gives for that recording alone, on est[c_off[r] .. c_off[r + 1]), in the same alignment arm (the arm is chosen once
 * per call from L % 4, H % 4 and the base addresses; multiples of 4 as offsets keep every recording in the arm of the bases).  For Q
 * this is the summation order of ams_stitch_stats: (1) per thread over its positions of a slab in position order, (2) the 64 lanes of
 * a wave by the halving shuffle tree l += l + o, o = 32 .. 1, (3) the four waves through LDS in wave order ((w0 + w1) + w2) + w3,
 * (4) the slabs of 1024 overlap positions in slab order.  No atomics anywhere; the library is built with -ffp-contract=off.
 *
 * Limits, the same for every entry point that takes the argument (AMS_E_INVALID_ARG otherwise, nothing launched): S in 1 .. 6;
 * 2 <= L <= 2^30; ceil(L / 2) <= H <= L - 1; R >= 1; Ctot >= R; R <= nblk < 2^31; P = S!; no NULL pointer; ws_bytes at least
 * ams_stitchb_workspace_bytes (a short workspace is an invalid argument here).  Offsets and sample positions are 64-bit.
 */
#ifndef AMS_STITCH_BATCH_H
#define AMS_STITCH_BATCH_H
#include <stddef.h>
#include <stdint.h>
#include "ams.h" /* ams_status, AMS_OK, AMS_E_* */
#ifdef __cplusplus
extern "C" {
#endif

int ams_stitchb_abi_version(void); /* 1 */

/* The chunk gather with zero fill: mix [Ctot, L] from the packed x.  One launch: grid (ceil(L / 1024), min(Ctot, 65535)), 256 threads, a
 * workgroup row walks the chunks g, g + gridDim.y, ...; no LDS, no workspace.  Never reads past a recording's own n[r] samples: what lies
 * between two recordings in x is not touched.
 * L % 4 == 0 and H % 4 == 0 with x and mix 16-byte aligned: one 16-byte load and store per thread (a group that crosses n[r] is filled
 * element by element); anything else: dword accesses, any base.
 * Bytes moved: 4 sum_r (min(n[r], C_r L) + (C_r - 1) V) read, 4 Ctot L written, 12 bytes of tables per chunk from cache. */
ams_status ams_stitchb_chunks(const float* x, const int64_t* n, const int64_t* x_off, const int64_t* c_off, const int32_t* chunk_rec,
                              float* mix, int R, int Ctot, int L, int H, void* stream);

/* Bytes of workspace ams_stitchb_stats needs: Ctot ceil(V / 1024) S S 4 (0 for arguments outside the limits). */
size_t ams_stitchb_workspace_bytes(int Ctot, int S, int L, int H);

/* The border table Q [Ctot, S, S] from est [Ctot, S, L].  Two launches: (1) grid (ceil(V / 1024), min(Ctot, 65535)), 256 threads: a
 * workgroup takes one slab of 1024 overlap positions of one real border (the last chunk of a recording is skipped), S x S running sums
 * in registers, shuffle tree, LDS in wave order (576 bytes), the slab's partial sums go to ws; (2) grid (ceil(Ctot S S / 256)): one
 * thread per entry of Q adds its slab partials in slab order, or writes 0.0f on the row of a recording's last chunk.
 * L % 4 == 0 and H % 4 == 0 with est 16-byte aligned: 16-byte loads; anything else: dword loads, any base.
 * Bytes moved: 8 (Ctot - R) S V read, 4 (Ctot - R) S S 2 ceil(V / 1024) of partials, 4 Ctot S S of Q. */
ams_status ams_stitchb_stats(const float* est, const int32_t* chunk_rec, float* Q, int R, int Ctot, int S, int L, int H, void* ws,
                             size_t ws_bytes, void* stream);

/* Border permutations rel [Ctot, S] and tracks trk [Ctot, S] (int32) from Q [Ctot, S, S] and perms [P, S] (int32, lexicographic, P = S!).
 * Two launches, no signalling between workgroups: (1) grid (Ctot), 256 threads: the search of ams_stitch_tracks on a real border, the
 * identity on a recording's last chunk; (2) grid (R), 64 threads: one wave per recording stages its rows of rel through LDS (960 words
 * at a time) and lanes k < S walk the chain from the identity at chunk c_off[r].  The kernels TRUST perms: every entry in 0 .. S - 1.
 * Bytes moved: 4 Ctot (S S + 3 S) + 4 P S per border from cache. */
ams_status ams_stitchb_tracks(const float* Q, const int32_t* perms, const int64_t* c_off, const int32_t* chunk_rec, int32_t* rel,
                              int32_t* trk, int R, int Ctot, int S, int P, void* stream);

/* The cross-fade: every recording's block [S, n[r]] of the packed out from est [Ctot, S, L], trk [Ctot, S] and w_head [V].  One launch:
 * grid (nblk, S), 256 threads: workgroup (b, k) writes block b - blk_off[r] (1024 samples) of track k of recording r = blk_rec[b];
 * 64-bit sample positions, no LDS, no workspace.  Nothing is written outside the blocks: what lies between them
 * in out stays as it was.  The kernel TRUSTS trk: every entry in 0 .. S - 1 (ams_stitchb_tracks writes nothing else).
 * L % 4 == 0 and H % 4 == 0 with est, out and w_head 16-byte aligned: one group of 4 positions per thread, 16-byte loads, a 16-byte
 * store where the row of the block starts on a 16-byte boundary and 4 dword stores otherwise; the last group of a row stores its
 * m < n[r] only.  Anything else: dword accesses, any base.
 * Bytes moved: 4 S sum_r (n[r] + (C_r - 1) V) of est and 4 S sum_r n[r] of out, 36 bytes of tables per workgroup from cache. */
ams_status ams_stitchb_ola(const float* est, const int32_t* trk, const float* w_head, const int64_t* n, const int64_t* out_off,
                           const int64_t* c_off, const int32_t* blk_rec, const int64_t* blk_off, float* out, int R, int Ctot, long nblk,
                           int S, int L, int H, void* stream);

#ifdef __cplusplus
}
#endif
#endif
