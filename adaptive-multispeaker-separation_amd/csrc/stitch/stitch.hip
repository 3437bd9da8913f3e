// Whole recordings (include/ams_stitch.h): chunk gather, border table, border permutations and tracks, cross-fade.
// A library of its own (libams_stitch.so): include/ams.h and libams_hip.so are untouched.  Built with -ffp-contract=off: the cross-fade
// is two rounded products and one rounded add, and the border table has one summation order per alignment arm.  All four are
// bandwidth-bound streaming / reduction kernels: no MFMA, no atomics, no scratch.  The arithmetic is stitch_core.h's, which
// libams_stitch_batch.so and libams_stream.so compile too; this file says where one recording's workgroups find their chunks.
#include "../../../include/ams_stitch.h"
#include "stitch_core.h"

namespace {

inline ams_status check_launch() { return hipGetLastError() == hipSuccess ? AMS_OK : AMS_E_LAUNCH_FAILED; }

template <bool VEC>
__global__ __launch_bounds__(256) void chunks_kernel(const float* __restrict__ x, long N, float* __restrict__ mix, int C, int L, int H) {
    for (int c = blockIdx.y; c < C; c += gridDim.y)
        gather_row<VEC>(x, N, (long)c * H, mix + (long)c * L, L);
}

template <int S, bool VEC>
__global__ __launch_bounds__(256) void stats_kernel(const float* __restrict__ est, float* __restrict__ part, int nb, int L, int H) {
    const int V = L - H, nslab = gridDim.x, slab = blockIdx.x;
    const int v0 = slab * SLAB, v1 = min(V, v0 + SLAB);
    for (int c = blockIdx.y; c < nb; c += gridDim.y)                      // est[c, i, H + v] against est[c + 1, j, v]
        border_sums<S, VEC>(est + (long)c * S * L + H, L, est + (long)(c + 1) * S * L, L, v0, v1, part + ((long)c * nslab + slab) * (S * S));
}

// Q[e] = the slab partials of entry e in slab order
__global__ __launch_bounds__(256) void stats_fold_kernel(const float* __restrict__ part, float* __restrict__ Q, long total, int SS, int nslab) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const long c = e / SS;
    Q[e] = slab_fold(part + c * nslab * SS + (int)(e - c * SS), nslab, SS);
}

__global__ __launch_bounds__(256) void border_perm_kernel(const float* __restrict__ Q, const int* __restrict__ perms, int* __restrict__ rel,
                                                          int S, int P) {
    __shared__ float q[36];
    __shared__ float sc[256];
    __shared__ int sp[256];
    const int SS = S * S, tid = threadIdx.x, c = blockIdx.x;
    if (tid < SS) q[tid] = Q[(long)c * SS + tid];
    __syncthreads();
    const int win = best_perm(q, sc, sp, perms, S, P);
    if (tid < S) rel[(long)c * S + tid] = perms[(long)win * S + tid];
}

__global__ __launch_bounds__(64) void tracks_kernel(const int* __restrict__ rel, int* __restrict__ trk, int C, int S) {
    chain_walk(rel, trk, C, S);
}

template <bool VEC>
__global__ __launch_bounds__(256) void ola_kernel(const float* __restrict__ est, const int* __restrict__ trk, const float* __restrict__ w_head,
                                                  float* __restrict__ out, long N, int C, int S, int L, int H) {
    const int k = blockIdx.y;
    fade_block<VEC>(est, trk, w_head, out + (long)k * N, N, C, S, L, H, k, blockIdx.x);
}

}  // namespace

extern "C" {

int ams_stitch_abi_version(void) { return 1; }

ams_status ams_stitch_chunks(const float* x, long N, float* mix, int C, int L, int H, void* stream) {
    STITCH_REQUIRE(x && mix);
    STITCH_REQUIRE(N >= 1 && geometry_ok(L, H) && C >= 1 && (long)C == chunks_of(N, L, H));
    const bool vec = L % 4 == 0 && H % 4 == 0 && aligned16(x) && aligned16(mix);
    const dim3 grid((unsigned)cdiv(L, 1024), (unsigned)(C < 65535 ? C : 65535));
    hipStream_t st = (hipStream_t)stream;
    if (vec) hipLaunchKernelGGL(chunks_kernel<true>, grid, dim3(256), 0, st, x, N, mix, C, L, H);
    else hipLaunchKernelGGL(chunks_kernel<false>, grid, dim3(256), 0, st, x, N, mix, C, L, H);
    return check_launch();
}

size_t ams_stitch_workspace_bytes(int C, int S, int L, int H) {
    if (C < 2 || !sources_ok(S) || !geometry_ok(L, H)) return 0;
    return (size_t)(C - 1) * (size_t)cdiv(L - H, SLAB) * (size_t)(S * S) * sizeof(float);
}

ams_status ams_stitch_stats(const float* est, float* Q, int C, int S, int L, int H, void* ws, size_t ws_bytes, void* stream) {
    STITCH_REQUIRE(est && Q && ws);
    STITCH_REQUIRE(sources_ok(S) && C >= 2 && geometry_ok(L, H));
    if (ws_bytes < ams_stitch_workspace_bytes(C, S, L, H)) return AMS_E_WORKSPACE_TOO_SMALL;
    const int nb = C - 1, nslab = (int)cdiv(L - H, SLAB);
    const bool vec = L % 4 == 0 && H % 4 == 0 && aligned16(est);
    const dim3 grid((unsigned)nslab, (unsigned)(nb < 65535 ? nb : 65535));
    hipStream_t st = (hipStream_t)stream;
    float* part = (float*)ws;
    const ams_status rc = for_sources(S, [&](auto s) {
        if (vec) hipLaunchKernelGGL((stats_kernel<s(), true>), grid, dim3(256), 0, st, est, part, nb, L, H);
        else hipLaunchKernelGGL((stats_kernel<s(), false>), grid, dim3(256), 0, st, est, part, nb, L, H);
        return check_launch();
    });
    if (rc != AMS_OK) return rc;
    const long total = (long)nb * S * S;
    hipLaunchKernelGGL(stats_fold_kernel, dim3((unsigned)cdiv(total, 256)), dim3(256), 0, st, part, Q, total, S * S, nslab);
    return check_launch();
}

ams_status ams_stitch_tracks(const float* Q, const int32_t* perms, int32_t* rel, int32_t* trk, int C, int S, int P, void* stream) {
    STITCH_REQUIRE(Q && perms && rel && trk);
    STITCH_REQUIRE(sources_ok(S) && C >= 2);
    STITCH_REQUIRE(perm_count_ok(S, P));
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(border_perm_kernel, dim3((unsigned)(C - 1)), dim3(256), 0, st, Q, perms, rel, S, P);
    ams_status rc = check_launch();
    if (rc != AMS_OK) return rc;
    hipLaunchKernelGGL(tracks_kernel, dim3(1), dim3(64), 0, st, rel, trk, C, S);
    return check_launch();
}

ams_status ams_stitch_ola(const float* est, const int32_t* trk, const float* w_head, float* out, long N, int C, int S, int L, int H,
                          void* stream) {
    STITCH_REQUIRE(est && trk && w_head && out);
    STITCH_REQUIRE(sources_ok(S) && N >= 1 && geometry_ok(L, H) && C >= 1 && (long)C == chunks_of(N, L, H));
    const bool vec = L % 4 == 0 && H % 4 == 0 && aligned16(est) && aligned16(out) && aligned16(w_head);
    const dim3 grid((unsigned)cdiv(N, 1024), (unsigned)S);
    hipStream_t st = (hipStream_t)stream;
    if (vec) hipLaunchKernelGGL(ola_kernel<true>, grid, dim3(256), 0, st, est, trk, w_head, out, N, C, S, L, H);
    else hipLaunchKernelGGL(ola_kernel<false>, grid, dim3(256), 0, st, est, trk, w_head, out, N, C, S, L, H);
    return check_launch();
}

}  // extern "C"
