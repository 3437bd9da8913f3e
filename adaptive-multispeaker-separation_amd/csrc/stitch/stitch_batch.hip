// Many recordings in one call (include/ams_stitch_batch.h): the stitcher over a ragged stream of chunks.
// A library of its own (libams_stitch_batch.so): ams_stitch.h and libams_stitch.so are untouched.  Built with -ffp-contract=off.  Every
// recording's results are bit-equal to libams_stitch.so's on that recording alone: the per-recording arithmetic is stitch_core.h's, the
// header that stitch.hip compiles too; what is here is where a workgroup finds its recording (chunk_rec, c_off, blk_rec, blk_off:
// device tables the caller built on the host and that the kernels trust).  Launch counts do not depend on the number of recordings.
// No MFMA, no atomics, no scratch.
#include "../../../include/ams_stitch_batch.h"
#include "stitch_core.h"

namespace {

inline ams_status check_launch() { return hipGetLastError() == hipSuccess ? AMS_OK : AMS_E_LAUNCH_FAILED; }
inline bool counts_ok(int R, int Ctot) { return R >= 1 && Ctot >= R; }

template <bool VEC>
__global__ __launch_bounds__(256) void chunks_kernel(const float* __restrict__ xp, const int64_t* __restrict__ len,
                                                     const int64_t* __restrict__ x_off, const int64_t* __restrict__ c_off,
                                                     const int* __restrict__ chunk_rec, float* __restrict__ mix, int Ctot, int L, int H) {
    for (int g = blockIdx.y; g < Ctot; g += gridDim.y) {
        const int r = chunk_rec[g];
        gather_row<VEC>(xp + x_off[r], len[r], ((long)g - c_off[r]) * H, mix + (long)g * L, L);
    }
}

// chunk g has a border behind it: the next chunk belongs to the same recording
__device__ __forceinline__ bool real_border(const int* __restrict__ chunk_rec, long g, int Ctot) {
    return g + 1 < Ctot && chunk_rec[g] == chunk_rec[g + 1];
}

template <int S, bool VEC>
__global__ __launch_bounds__(256) void stats_kernel(const float* __restrict__ est, const int* __restrict__ chunk_rec,
                                                    float* __restrict__ part, int Ctot, int L, int H) {
    const int V = L - H, nslab = gridDim.x, slab = blockIdx.x;
    const int v0 = slab * SLAB, v1 = min(V, v0 + SLAB);
    for (int c = blockIdx.y; c < Ctot; c += gridDim.y) {
        if (!real_border(chunk_rec, c, Ctot)) continue;                   // the same for the whole workgroup
        border_sums<S, VEC>(est + (long)c * S * L + H, L, est + (long)(c + 1) * S * L, L, v0, v1, part + ((long)c * nslab + slab) * (S * S));
    }
}

// Q[e] = the slab partials of entry e in slab order; exact zeros on the row of a recording's last chunk (its partials were never written)
__global__ __launch_bounds__(256) void stats_fold_kernel(const float* __restrict__ part, const int* __restrict__ chunk_rec,
                                                         float* __restrict__ Q, long total, int SS, int nslab, int Ctot) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const long c = e / SS;
    if (!real_border(chunk_rec, c, Ctot)) {
        Q[e] = 0.f;
        return;
    }
    Q[e] = slab_fold(part + c * nslab * SS + (int)(e - c * SS), nslab, SS);
}

__global__ __launch_bounds__(256) void border_perm_kernel(const float* __restrict__ Q, const int* __restrict__ perms,
                                                          const int* __restrict__ chunk_rec, int* __restrict__ rel, int Ctot, int S, int P) {
    __shared__ float q[36];
    __shared__ float sc[256];
    __shared__ int sp[256];
    const int SS = S * S, tid = threadIdx.x, c = blockIdx.x;
    if (!real_border(chunk_rec, c, Ctot)) {                          // a recording's last chunk: the identity (the whole workgroup leaves)
        if (tid < S) rel[(long)c * S + tid] = tid;
        return;
    }
    if (tid < SS) q[tid] = Q[(long)c * SS + tid];
    __syncthreads();
    const int win = best_perm(q, sc, sp, perms, S, P);
    if (tid < S) rel[(long)c * S + tid] = perms[(long)win * S + tid];
}

// one wave per recording, a fresh start at its first chunk c_off[r]
__global__ __launch_bounds__(64) void tracks_kernel(const int* __restrict__ rel_all, const int64_t* __restrict__ c_off,
                                                    int* __restrict__ trk_all, int S) {
    const long g0 = c_off[blockIdx.x];
    chain_walk(rel_all + g0 * S, trk_all + g0 * S, (int)(c_off[blockIdx.x + 1] - g0), S);
}

template <bool VEC>
__global__ __launch_bounds__(256) void ola_kernel(const float* __restrict__ est_all, const int* __restrict__ trk_all,
                                                  const float* __restrict__ w_head, const int64_t* __restrict__ len,
                                                  const int64_t* __restrict__ out_off, const int64_t* __restrict__ c_off,
                                                  const int* __restrict__ blk_rec, const int64_t* __restrict__ blk_off,
                                                  float* __restrict__ out_all, int S, int L, int H) {
    const int r = blk_rec[blockIdx.x];
    const long blk = (long)blockIdx.x - blk_off[r];                        // the 1024-sample block inside recording r
    const long N = len[r], g0 = c_off[r];
    const int C = (int)(c_off[r + 1] - g0), k = blockIdx.y;
    fade_block<VEC>(est_all + g0 * S * L, trk_all + g0 * S, w_head, out_all + out_off[r] + (long)k * N, N, C, S, L, H, k, blk);
}

}  // namespace

extern "C" {

int ams_stitchb_abi_version(void) { return 1; }

ams_status ams_stitchb_chunks(const float* x, const int64_t* n, const int64_t* x_off, const int64_t* c_off, const int32_t* chunk_rec,
                              float* mix, int R, int Ctot, int L, int H, void* stream) {
    STITCH_REQUIRE(x && n && x_off && c_off && chunk_rec && mix);
    STITCH_REQUIRE(counts_ok(R, Ctot) && geometry_ok(L, H));
    const bool vec = L % 4 == 0 && H % 4 == 0 && aligned16(x) && aligned16(mix);
    const dim3 grid((unsigned)cdiv(L, 1024), (unsigned)(Ctot < 65535 ? Ctot : 65535));
    hipStream_t st = (hipStream_t)stream;
    if (vec) hipLaunchKernelGGL(chunks_kernel<true>, grid, dim3(256), 0, st, x, n, x_off, c_off, chunk_rec, mix, Ctot, L, H);
    else hipLaunchKernelGGL(chunks_kernel<false>, grid, dim3(256), 0, st, x, n, x_off, c_off, chunk_rec, mix, Ctot, L, H);
    return check_launch();
}

size_t ams_stitchb_workspace_bytes(int Ctot, int S, int L, int H) {
    if (Ctot < 1 || !sources_ok(S) || !geometry_ok(L, H)) return 0;
    return (size_t)Ctot * (size_t)cdiv(L - H, SLAB) * (size_t)(S * S) * sizeof(float);
}

ams_status ams_stitchb_stats(const float* est, const int32_t* chunk_rec, float* Q, int R, int Ctot, int S, int L, int H, void* ws,
                             size_t ws_bytes, void* stream) {
    STITCH_REQUIRE(est && chunk_rec && Q && ws);
    STITCH_REQUIRE(sources_ok(S) && counts_ok(R, Ctot) && geometry_ok(L, H));
    STITCH_REQUIRE(ws_bytes >= ams_stitchb_workspace_bytes(Ctot, S, L, H));
    const int nslab = (int)cdiv(L - H, SLAB);
    const bool vec = L % 4 == 0 && H % 4 == 0 && aligned16(est);
    const dim3 grid((unsigned)nslab, (unsigned)(Ctot < 65535 ? Ctot : 65535));
    hipStream_t st = (hipStream_t)stream;
    float* part = (float*)ws;
    const ams_status rc = for_sources(S, [&](auto s) {
        if (vec) hipLaunchKernelGGL((stats_kernel<s(), true>), grid, dim3(256), 0, st, est, chunk_rec, part, Ctot, L, H);
        else hipLaunchKernelGGL((stats_kernel<s(), false>), grid, dim3(256), 0, st, est, chunk_rec, part, Ctot, L, H);
        return check_launch();
    });
    if (rc != AMS_OK) return rc;
    const long total = (long)Ctot * S * S;
    hipLaunchKernelGGL(stats_fold_kernel, dim3((unsigned)cdiv(total, 256)), dim3(256), 0, st, part, chunk_rec, Q, total, S * S, nslab, Ctot);
    return check_launch();
}

ams_status ams_stitchb_tracks(const float* Q, const int32_t* perms, const int64_t* c_off, const int32_t* chunk_rec, int32_t* rel,
                              int32_t* trk, int R, int Ctot, int S, int P, void* stream) {
    STITCH_REQUIRE(Q && perms && c_off && chunk_rec && rel && trk);
    STITCH_REQUIRE(sources_ok(S) && counts_ok(R, Ctot));
    STITCH_REQUIRE(perm_count_ok(S, P));
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(border_perm_kernel, dim3((unsigned)Ctot), dim3(256), 0, st, Q, perms, chunk_rec, rel, Ctot, S, P);
    ams_status rc = check_launch();
    if (rc != AMS_OK) return rc;
    hipLaunchKernelGGL(tracks_kernel, dim3((unsigned)R), dim3(64), 0, st, rel, c_off, trk, S);
    return check_launch();
}

ams_status ams_stitchb_ola(const float* est, const int32_t* trk, const float* w_head, const int64_t* n, const int64_t* out_off,
                           const int64_t* c_off, const int32_t* blk_rec, const int64_t* blk_off, float* out, int R, int Ctot, long nblk,
                           int S, int L, int H, void* stream) {
    STITCH_REQUIRE(est && trk && w_head && n && out_off && c_off && blk_rec && blk_off && out);
    STITCH_REQUIRE(sources_ok(S) && counts_ok(R, Ctot) && geometry_ok(L, H) && nblk >= R && nblk <= 0x7fffffffL);
    const bool vec = L % 4 == 0 && H % 4 == 0 && aligned16(est) && aligned16(out) && aligned16(w_head);
    const dim3 grid((unsigned)nblk, (unsigned)S);
    hipStream_t st = (hipStream_t)stream;
    if (vec) hipLaunchKernelGGL(ola_kernel<true>, grid, dim3(256), 0, st, est, trk, w_head, n, out_off, c_off, blk_rec, blk_off, out, S, L, H);
    else hipLaunchKernelGGL(ola_kernel<false>, grid, dim3(256), 0, st, est, trk, w_head, n, out_off, c_off, blk_rec, blk_off, out, S, L, H);
    return check_launch();
}

}  // extern "C"
