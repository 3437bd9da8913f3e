/* ams_stitch.h -- whole recordings: the C ABI of libams_stitch.so (csrc/stitch/stitch.hip; gfx950 only).
 *
 * A separation model works on chunks of L samples and clusters every chunk on its own, so the order of its S outputs is arbitrary
 * from chunk to chunk.  These entry points cut a recording into overlapping chunks, decide at every chunk border which output
 * continues which, and cross-fade the pieces back into S recordings.  include/ams.h is unchanged and keeps its own version number;
 * the conventions are those of ams.h: every entry point returns an ams_status, never allocates, never synchronises, enqueues on the
 * given stream only; the caller owns every buffer; AMS_E_INVALID_ARG is returned before anything is launched.
 *
 * Definitions.  x [N] float32, N >= 1.  L = chunk length, H = hop with ceil(L / 2) <= H <= L - 1, V = L - H the
 * overlap (1 .. L / 2: no sample is covered by more than two chunks).  S = 1 .. 6 sources.
 *   C            = 1 + max(0, ceil((N - L) / H))                       chunks
 *   mix[c, l]    = x[c H + l] where c H + l < N, else 0
 *   est[C, S, L] the model's output for the C chunks
 *   Q[c, i, j]   = sum_{v < V} (est[c, i, H + v] - est[c + 1, j, v])^2      c = 0 .. C - 2, f32, fixed order, no atomics
 *   rel[c]       = perms[argmin_p sum_s Q[c, s, perms[p, s]]]              perms: the lexicographic [S!, S] table; the cost is summed in
 *                  s order in f32, compared with <, the lowest index wins among equal costs, a NaN cost never wins, and if every
 *                  cost is NaN index 0 (the identity) wins
 *   trk[0, k]    = k,   trk[c + 1, k] = rel[c][trk[c, k]]                  track k is what the model called source k in chunk 0
 *   out[k, n]    for n < N, c1 = min(n / H, C - 1), p = n - c1 H:
 *                  c1 > 0 and p < V:  fl(w_tail[p] est[c1 - 1, trk[c1 - 1, k], H + p]) + fl(w_head[p] est[c1, trk[c1, k], p])
 *                                     with w_tail[p] = 1.0f - w_head[p]: two rounded products, one rounded add, no FMA
 *                  otherwise:         est[c1, trk[c1, k], p]               (a copy)
 *   w_head[v]    = float32((v + 0.5) / V), computed by the CALLER in float64 and rounded once; a device table of V floats
 * Limits, the same for every entry point that takes the argument (AMS_E_INVALID_ARG otherwise): S in 1 .. 6; 2 <= L <= 2^30;
 * ceil(L / 2) <= H <= L - 1; N >= 1; C equal to the formula above where N is given, C >= 2 for stats and tracks; P = S!; no NULL
 * pointer.  Sample positions are 64-bit.
 */
#ifndef AMS_STITCH_H
#define AMS_STITCH_H
#include <stddef.h>
#include <stdint.h>
#include "ams.h" /* ams_status, AMS_OK, AMS_E_* */
#ifdef __cplusplus
extern "C" {
#endif

int ams_stitch_abi_version(void); /* 1 */

/* The chunk gather with zero fill: mix [C, L] from x [N].  C = 1 (N <= L) is valid.
 * Grid (ceil(L / 1024), min(C, 65535)), 256 threads, a workgroup row walks the chunks c, c + gridDim.y, ...; no LDS, no workspace.
 * L % 4 == 0 and H % 4 == 0 with x and mix 16-byte aligned: one 16-byte load and store per thread (a group that crosses N is filled
 * element by element); anything else: dword accesses (thread t takes positions t, t + 256, t + 512, t + 768 of the 1024), any base.
 * Bytes moved: 4 (min(N, C L) + (C - 1) V) read, 4 C L written. */
ams_status ams_stitch_chunks(const float* x, long N, float* mix, int C, int L, int H, void* stream);

/* Bytes of workspace ams_stitch_stats needs: (C - 1) ceil(V / 1024) S S 4 (0 for arguments outside the limits). */
size_t ams_stitch_workspace_bytes(int C, int S, int L, int H);

/* The border table Q [C - 1, S, S] from est [C, S, L], C >= 2.  Both sides of a border are read in place: the tail of chunk c and the
 * head of chunk c + 1 are strided views of est.  Two launches: (1) grid (ceil(V / 1024), min(C - 1, 65535)), 256 threads: a workgroup
 * takes one slab of 1024 overlap positions of one border, every thread holds the S x S running sums in registers (no scratch),
 * the 64 lanes of a wave are folded by a shuffle tree, the 4 waves through LDS (576 bytes) in wave order, and the slab's S S partial
 * sums go to ws; (2) grid (ceil((C - 1) S S / 256)): one thread per entry of Q adds its slab partials in slab order.  No atomics: the
 * bits of Q depend on (est, S, L, H, the alignment arm) only.
 * L % 4 == 0 and H % 4 == 0 with est 16-byte aligned: 16-byte loads; anything else: dword loads, any base.
 * AMS_E_WORKSPACE_TOO_SMALL: ws_bytes < ams_stitch_workspace_bytes(C, S, L, H).
 * Bytes moved: 8 (C - 1) S V read (each side once), 4 (C - 1) S S (2 ceil(V / 1024) + 1) of partials and Q. */
ams_status ams_stitch_stats(const float* est, float* Q, int C, int S, int L, int H, void* ws, size_t ws_bytes, void* stream);

/* Border permutations rel [C - 1, S] and tracks trk [C, S] (int32) from Q [C - 1, S, S] and perms [P, S] (int32, lexicographic,
 * P = S!), C >= 2.  Two launches, no signalling between workgroups: (1) grid (C - 1), 256 threads: lane t owns permutations t,
 * t + 256, t + 512, a 256-lane halving tree in LDS ordered by (cost, index) with the NaN rule above picks the winner and S lanes copy
 * its row of perms to rel; (2) grid (1), 64 threads: one wave stages rel through LDS (960 words at a time) and lanes k < S walk the
 * chain.  The kernel TRUSTS perms: every entry in 0 .. S - 1.  Bytes moved: 4 (C - 1) (S S + 2 S) + 4 P S per border from cache. */
ams_status ams_stitch_tracks(const float* Q, const int32_t* perms, int32_t* rel, int32_t* trk, int C, int S, int P, void* stream);

/* The cross-fade: out [S, N] from est [C, S, L], trk [C, S] and w_head [V].  C = 1 is valid (a copy of the first N samples of every
 * source; trk and w_head are still required, w_head is not read).  Nothing past out[S - 1, N - 1] is written.
 * Grid (ceil(N / 1024), S), 256 threads, 64-bit sample positions, no LDS, no workspace.  The kernel TRUSTS trk: every entry in
 * 0 .. S - 1 (ams_stitch_tracks writes nothing else).
 * L % 4 == 0 and H % 4 == 0 with est, out and w_head 16-byte aligned: one group of 4 positions per thread, 16-byte loads, a 16-byte
 * store where the row out[k] starts on a 16-byte boundary (always for N % 4 == 0) and 4 dword stores otherwise; the last group of a row
 * stores its n < N only.  Anything else: dword accesses (thread t takes positions t, t + 256, t + 512, t + 768 of the 1024), any base.
 * Bytes moved: 4 S (N + (C - 1) V) of est and 4 S N of out, plus 4 (C - 1) V of w_head per source from cache. */
ams_status ams_stitch_ola(const float* est, const int32_t* trk, const float* w_head, float* out, long N, int C, int S, int L, int H,
                          void* stream);

#ifdef __cplusplus
}
#endif
#endif
