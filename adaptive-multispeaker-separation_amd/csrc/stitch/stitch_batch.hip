// Many recordings in one call (include/ams_stitch_batch.h): the kernels of stitch.hip over a ragged stream of chunks.
// A library of its own (libams_stitch_batch.so): ams_stitch.h and libams_stitch.so are untouched.  Built with -ffp-contract=off.  Every
// recording's results are bit-equal to libams_stitch.so's on that recording alone: the per-recording arithmetic below IS stitch.hip's,
// statement for statement; what is new is where a workgroup finds its recording (chunk_rec, c_off, blk_rec, blk_off: device tables the
// caller built on the host and that the kernels trust).  Launch counts do not depend on the number of recordings.  No MFMA, no atomics,
// no scratch.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include "../../../include/ams_stitch_batch.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int SLAB = 1024;            // overlap positions per workgroup of the border table
constexpr int TILE = 960;             // words of rel staged per round of the chain walk: a multiple of every S in 1 .. 6

#define STITCHB_REQUIRE(cond)                  \
    do {                                       \
        if (!(cond)) return AMS_E_INVALID_ARG; \
    } while (0)

inline ams_status check_launch() { return hipGetLastError() == hipSuccess ? AMS_OK : AMS_E_LAUNCH_FAILED; }
inline long cdiv(long a, long b) { return (a + b - 1) / b; }
inline bool geometry_ok(int L, int H) { return L >= 2 && L <= (1 << 30) && H >= (L + 1) / 2 && H <= L - 1; }
inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// ------------------------------------------------------------------ chunks
template <bool VEC>
__global__ __launch_bounds__(256) void chunks_kernel(const float* __restrict__ xp, const int64_t* __restrict__ len,
                                                     const int64_t* __restrict__ x_off, const int64_t* __restrict__ c_off,
                                                     const int* __restrict__ chunk_rec, float* __restrict__ mix, int Ctot, int L, int H) {
    for (int g = blockIdx.y; g < Ctot; g += gridDim.y) {
        const int r = chunk_rec[g];
        const float* const x = xp + x_off[r];
        const long N = len[r];
        const long base = ((long)g - c_off[r]) * H;
        float* const row = mix + (long)g * L;
        if constexpr (VEC) {
            const int l = (blockIdx.x * 256 + threadIdx.x) * 4;
            if (l >= L) return;
            const long n = base + l;
            f32x4 v;
            if (n + 4 <= N) v = *(const f32x4*)(x + n);
            else {
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = n + e < N ? x[n + e] : 0.f;
            }
            *(f32x4*)(row + l) = v;
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int l = blockIdx.x * 1024 + k * 256 + threadIdx.x;
                if (l >= L) break;
                const long n = base + l;
                row[l] = n < N ? x[n] : 0.f;
            }
        }
    }
}

// ------------------------------------------------------------------ border table
// sum of the 64 lanes in lane 0, as the halving tree l += l + o (o = 32 .. 1): one fixed order
__device__ __forceinline__ float wave_fold(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}

// chunk g has a border behind it: the next chunk belongs to the same recording
__device__ __forceinline__ bool real_border(const int* __restrict__ chunk_rec, long g, int Ctot) {
    return g + 1 < Ctot && chunk_rec[g] == chunk_rec[g + 1];
}

template <int S, bool VEC>
__global__ __launch_bounds__(256) void stats_kernel(const float* __restrict__ est, const int* __restrict__ chunk_rec,
                                                    float* __restrict__ part, int Ctot, int L, int H) {
    __shared__ float sm[4][S * S];
    const int V = L - H, nslab = gridDim.x, slab = blockIdx.x, tid = threadIdx.x;
    const int v0 = slab * SLAB, v1 = min(V, v0 + SLAB);
    for (int c = blockIdx.y; c < Ctot; c += gridDim.y) {
        if (!real_border(chunk_rec, c, Ctot)) continue;                   // the same for the whole workgroup
        const float* const tail = est + (long)c * S * L + H;              // est[c, i, H + v] = tail[i L + v]
        const float* const head = est + (long)(c + 1) * S * L;            // est[c + 1, j, v] = head[j L + v]
        float acc[S][S];
#pragma unroll
        for (int i = 0; i < S; ++i)
#pragma unroll
            for (int j = 0; j < S; ++j) acc[i][j] = 0.f;
        if constexpr (VEC) {
            const int v = v0 + tid * 4;                                    // V % 4 == 0: whole groups only
            if (v < v1) {
                f32x4 a[S], b[S];
#pragma unroll
                for (int i = 0; i < S; ++i) {
                    a[i] = *(const f32x4*)(tail + (long)i * L + v);
                    b[i] = *(const f32x4*)(head + (long)i * L + v);
                }
#pragma unroll
                for (int e = 0; e < 4; ++e)
#pragma unroll
                    for (int i = 0; i < S; ++i)
#pragma unroll
                        for (int j = 0; j < S; ++j) {
                            const float d = a[i][e] - b[j][e];
                            acc[i][j] += d * d;
                        }
            }
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int v = v0 + k * 256 + tid;
                if (v < v1) {
                    float a[S], b[S];
#pragma unroll
                    for (int i = 0; i < S; ++i) {
                        a[i] = tail[(long)i * L + v];
                        b[i] = head[(long)i * L + v];
                    }
#pragma unroll
                    for (int i = 0; i < S; ++i)
#pragma unroll
                        for (int j = 0; j < S; ++j) {
                            const float d = a[i] - b[j];
                            acc[i][j] += d * d;
                        }
                }
            }
        }
#pragma unroll
        for (int i = 0; i < S; ++i)
#pragma unroll
            for (int j = 0; j < S; ++j) {
                const float s = wave_fold(acc[i][j]);
                if ((tid & 63) == 0) sm[tid >> 6][i * S + j] = s;
            }
        __syncthreads();
        if (tid < S * S) part[((long)c * nslab + slab) * (S * S) + tid] = ((sm[0][tid] + sm[1][tid]) + sm[2][tid]) + sm[3][tid];
        __syncthreads();
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
    const int ij = (int)(e - c * SS);
    const float* p = part + c * nslab * SS + ij;
    float s = p[0];
    for (int k = 1; k < nslab; ++k) s += p[(long)k * SS];
    Q[e] = s;
}

template <int S>
ams_status launch_stats(bool vec, dim3 grid, hipStream_t st, const float* est, const int* chunk_rec, float* part, int Ctot, int L, int H) {
    if (vec) hipLaunchKernelGGL((stats_kernel<S, true>), grid, dim3(256), 0, st, est, chunk_rec, part, Ctot, L, H);
    else hipLaunchKernelGGL((stats_kernel<S, false>), grid, dim3(256), 0, st, est, chunk_rec, part, Ctot, L, H);
    return check_launch();
}

// ------------------------------------------------------------------ border permutations and tracks
// (c2, p2) before (c1, p1) in the order (cost, index)?  An index >= P marks "none": a lane without a permutation, or a NaN cost.
__device__ __forceinline__ bool goes_first(float c2, int p2, float c1, int p1, int P) {
    if (p2 >= P) return false;
    if (p1 >= P) return true;
    return c2 < c1 || (c2 == c1 && p2 < p1);
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
    float best = 0.f;
    int bp = P;
    for (int p = tid; p < P; p += 256) {                             // t, t + 256, t + 512: increasing index, so < keeps the lowest
        const int* row = perms + (long)p * S;
        float cost = 0.f;
        for (int s = 0; s < S; ++s) cost += q[s * S + row[s]];
        if (cost == cost && (bp == P || cost < best)) { best = cost; bp = p; }
    }
    sc[tid] = best;
    sp[tid] = bp;
    __syncthreads();
    for (int h = 128; h >= 1; h >>= 1) {
        if (tid < h && goes_first(sc[tid + h], sp[tid + h], sc[tid], sp[tid], P)) { sc[tid] = sc[tid + h]; sp[tid] = sp[tid + h]; }
        __syncthreads();
    }
    const int win = sp[0] < P ? sp[0] : 0;                           // every cost NaN: the identity
    if (tid < S) rel[(long)c * S + tid] = perms[(long)win * S + tid];
}

// one wave per recording: trk[c_off[r], k] = k, trk[g + 1, k] = rel[g][trk[g, k]] up to the recording's last chunk; rel goes through LDS
// TILE words at a time (coalesced loads, LDS-latency chain)
__global__ __launch_bounds__(64) void tracks_kernel(const int* __restrict__ rel_all, const int64_t* __restrict__ c_off,
                                                    int* __restrict__ trk_all, int S) {
    __shared__ int sr[TILE];
    const long g0 = c_off[blockIdx.x];
    const int C = (int)(c_off[blockIdx.x + 1] - g0);
    const int* const rel = rel_all + g0 * S;
    int* const trk = trk_all + g0 * S;
    const int lane = threadIdx.x, per = TILE / S, nb = C - 1;
    int cur = lane < S ? lane : 0;
    if (lane < S) trk[lane] = cur;
    for (int b0 = 0; b0 < nb; b0 += per) {
        const int n = min(per, nb - b0);
        for (int w = lane; w < n * S; w += 64) sr[w] = rel[(long)b0 * S + w];
        __syncthreads();
        if (lane < S) {
            for (int b = 0; b < n; ++b) {
                cur = sr[b * S + cur];
                trk[(long)(b0 + b + 1) * S + lane] = cur;
            }
        }
        __syncthreads();
    }
}

// ------------------------------------------------------------------ cross-fade
__device__ __forceinline__ long chunk_of(long n, int H, int C) {
    const long c = n / H;
    return c < C - 1 ? c : C - 1;
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
    const int C = (int)(c_off[r + 1] - g0);
    const float* const est = est_all + g0 * S * L;
    const int* const trk = trk_all + g0 * S;
    const int k = blockIdx.y, V = L - H;
    float* const orow = out_all + out_off[r] + (long)k * N;
    if constexpr (VEC) {
        const long n = (blk * 256 + threadIdx.x) * 4;                      // H % 4 == 0, V % 4 == 0: a group never straddles a case
        if (n >= N) return;
        const long c1 = chunk_of(n, H, C);
        const long p = n - c1 * H;                                         // < L: inside chunk c1, and p + 3 < L
        f32x4 v = *(const f32x4*)(est + (c1 * S + trk[c1 * S + k]) * L + p);
        if (c1 > 0 && p < V) {
            const f32x4 t = *(const f32x4*)(est + ((c1 - 1) * S + trk[(c1 - 1) * S + k]) * L + H + p);
            const f32x4 wh = *(const f32x4*)(w_head + p);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float wt = 1.0f - wh[e];
                const float a = wt * t[e], b = wh[e] * v[e];
                v[e] = a + b;
            }
        }
        if (n + 4 <= N) {
            if (((uintptr_t)orow & 15) == 0) *(f32x4*)(orow + n) = v;
            else { orow[n] = v[0]; orow[n + 1] = v[1]; orow[n + 2] = v[2]; orow[n + 3] = v[3]; }
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (n + e < N) orow[n + e] = v[e];
        }
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const long n = blk * 1024 + j * 256 + threadIdx.x;
            if (n >= N) break;
            const long c1 = chunk_of(n, H, C);
            const long p = n - c1 * H;
            float v = est[(c1 * S + trk[c1 * S + k]) * L + p];
            if (c1 > 0 && p < V) {
                const float t = est[((c1 - 1) * S + trk[(c1 - 1) * S + k]) * L + H + p];
                const float wh = w_head[p];
                const float wt = 1.0f - wh;
                const float a = wt * t, b = wh * v;
                v = a + b;
            }
            orow[n] = v;
        }
    }
}

inline bool counts_ok(int R, int Ctot) { return R >= 1 && Ctot >= R; }
inline bool sources_ok(int S) { return S >= 1 && S <= 6; }

}  // namespace

extern "C" {

int ams_stitchb_abi_version(void) { return 1; }

ams_status ams_stitchb_chunks(const float* x, const int64_t* n, const int64_t* x_off, const int64_t* c_off, const int32_t* chunk_rec,
                              float* mix, int R, int Ctot, int L, int H, void* stream) {
    STITCHB_REQUIRE(x && n && x_off && c_off && chunk_rec && mix);
    STITCHB_REQUIRE(counts_ok(R, Ctot) && geometry_ok(L, H));
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
    STITCHB_REQUIRE(est && chunk_rec && Q && ws);
    STITCHB_REQUIRE(sources_ok(S) && counts_ok(R, Ctot) && geometry_ok(L, H));
    STITCHB_REQUIRE(ws_bytes >= ams_stitchb_workspace_bytes(Ctot, S, L, H));
    const int nslab = (int)cdiv(L - H, SLAB);
    const bool vec = L % 4 == 0 && H % 4 == 0 && aligned16(est);
    const dim3 grid((unsigned)nslab, (unsigned)(Ctot < 65535 ? Ctot : 65535));
    hipStream_t st = (hipStream_t)stream;
    float* part = (float*)ws;
    ams_status rc;
    switch (S) {
        case 1: rc = launch_stats<1>(vec, grid, st, est, chunk_rec, part, Ctot, L, H); break;
        case 2: rc = launch_stats<2>(vec, grid, st, est, chunk_rec, part, Ctot, L, H); break;
        case 3: rc = launch_stats<3>(vec, grid, st, est, chunk_rec, part, Ctot, L, H); break;
        case 4: rc = launch_stats<4>(vec, grid, st, est, chunk_rec, part, Ctot, L, H); break;
        case 5: rc = launch_stats<5>(vec, grid, st, est, chunk_rec, part, Ctot, L, H); break;
        default: rc = launch_stats<6>(vec, grid, st, est, chunk_rec, part, Ctot, L, H); break;
    }
    if (rc != AMS_OK) return rc;
    const long total = (long)Ctot * S * S;
    hipLaunchKernelGGL(stats_fold_kernel, dim3((unsigned)cdiv(total, 256)), dim3(256), 0, st, part, chunk_rec, Q, total, S * S, nslab, Ctot);
    return check_launch();
}

ams_status ams_stitchb_tracks(const float* Q, const int32_t* perms, const int64_t* c_off, const int32_t* chunk_rec, int32_t* rel,
                              int32_t* trk, int R, int Ctot, int S, int P, void* stream) {
    STITCHB_REQUIRE(Q && perms && c_off && chunk_rec && rel && trk);
    STITCHB_REQUIRE(sources_ok(S) && counts_ok(R, Ctot));
    int fact = 1;
    for (int s = 2; s <= S; ++s) fact *= s;
    STITCHB_REQUIRE(P == fact);
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
    STITCHB_REQUIRE(est && trk && w_head && n && out_off && c_off && blk_rec && blk_off && out);
    STITCHB_REQUIRE(sources_ok(S) && counts_ok(R, Ctot) && geometry_ok(L, H) && nblk >= R && nblk <= 0x7fffffffL);
    const bool vec = L % 4 == 0 && H % 4 == 0 && aligned16(est) && aligned16(out) && aligned16(w_head);
    const dim3 grid((unsigned)nblk, (unsigned)S);
    hipStream_t st = (hipStream_t)stream;
    if (vec) hipLaunchKernelGGL(ola_kernel<true>, grid, dim3(256), 0, st, est, trk, w_head, n, out_off, c_off, blk_rec, blk_off, out, S, L, H);
    else hipLaunchKernelGGL(ola_kernel<false>, grid, dim3(256), 0, st, est, trk, w_head, n, out_off, c_off, blk_rec, blk_off, out, S, L, H);
    return check_launch();
}

}  // extern "C"
