// The stitcher's shared device code and host helpers, stated once for its three libraries: stitch.hip (one recording),
// stitch_batch.hip (a ragged batch) and ../stream/stream.hip (live streams) are specified bit for bit against each other, and what they
// have in common -- the border sums, the fold orders, the permutation search, the chain walk, the cross-fade -- is compiled from HERE
// into each of them.  A .hip file keeps where a workgroup finds its recording or stream, and its entry points.  Every unit that
// includes this is built with -ffp-contract=off: each product and each sum below is rounded once, in the order written.  Register
// arrays stay local to ONE helper (border_sums sums, folds and stores): passed between helpers they cost registers (HISTORY.md).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include <type_traits>
#include "../../../include/ams.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int SLAB = 1024;            // overlap positions per workgroup of the border table
constexpr int TILE = 960;             // words of rel staged per round of the chain walk: a multiple of every S in 1 .. 6

#define STITCH_REQUIRE(cond)                   \
    do {                                       \
        if (!(cond)) return AMS_E_INVALID_ARG; \
    } while (0)

inline long cdiv(long a, long b) { return (a + b - 1) / b; }
inline bool geometry_ok(int L, int H) { return L >= 2 && L <= (1 << 30) && H >= (L + 1) / 2 && H <= L - 1; }
inline long chunks_of(long N, int L, int H) { return N <= L ? 1 : 1 + cdiv(N - L, H); }
inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
inline bool sources_ok(int S) { return S >= 1 && S <= 6; }
inline bool perm_count_ok(int S, int P) {
    int fact = 1;
    for (int s = 2; s <= S; ++s) fact *= s;
    return P == fact;
}

// f(std::integral_constant<int, S>) for the S in 1 .. 6 that the caller has checked: the one place that turns S into a template argument
template <typename F>
ams_status for_sources(int S, F&& f) {
    switch (S) {
        case 1: return f(std::integral_constant<int, 1>());
        case 2: return f(std::integral_constant<int, 2>());
        case 3: return f(std::integral_constant<int, 3>());
        case 4: return f(std::integral_constant<int, 4>());
        case 5: return f(std::integral_constant<int, 5>());
        default: return f(std::integral_constant<int, 6>());
    }
}

// ------------------------------------------------------------------ chunks
// this thread's share of one chunk row: row[l] = x[base + l], zero past N
template <bool VEC>
__device__ __forceinline__ void gather_row(const float* __restrict__ x, long N, long base, float* __restrict__ row, int L) {
    if constexpr (VEC) {
        const int l = (blockIdx.x * 256 + threadIdx.x) * 4;
        if (l >= L) return;
        const long n = base + l;
        f32x4 r;
        if (n + 4 <= N) r = *(const f32x4*)(x + n);
        else {
#pragma unroll
            for (int e = 0; e < 4; ++e) r[e] = n + e < N ? x[n + e] : 0.f;
        }
        *(f32x4*)(row + l) = r;
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

// ------------------------------------------------------------------ border table
// sum of the 64 lanes in lane 0, as the halving tree l += l + o (o = 32 .. 1): one fixed order
__device__ __forceinline__ float wave_fold(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}

// One workgroup of 256, one border, the slab [v0, v1) of its overlap: dst[i S + j] = sum_v (tail[i ts + v] - head[j L + v])^2, summed per
// lane in v order, per wave by wave_fold, over the four waves left to right.  The tail rows lie ts words apart: L inside est, Vp in a
// stream's carried tail.  VEC: V % 4 == 0 and 16-byte rows.  Every thread of the workgroup calls it (two barriers).
template <int S, bool VEC>
__device__ __forceinline__ void border_sums(const float* __restrict__ tail, long ts, const float* __restrict__ head, int L, int v0, int v1,
                                            float* __restrict__ dst) {
    __shared__ float sm[4][S * S];
    const int tid = threadIdx.x;
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
                a[i] = *(const f32x4*)(tail + i * ts + v);
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
                    a[i] = tail[i * ts + v];
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
    if (tid < S * S) dst[tid] = ((sm[0][tid] + sm[1][tid]) + sm[2][tid]) + sm[3][tid];
    __syncthreads();
}

// the slab partials of one entry of Q, in slab order: p[0] + p[SS] + ...
__device__ __forceinline__ float slab_fold(const float* __restrict__ p, int nslab, int SS) {
    float s = p[0];
    for (int k = 1; k < nslab; ++k) s += p[(long)k * SS];
    return s;
}

// ------------------------------------------------------------------ border permutations and tracks
// (c2, p2) before (c1, p1) in the order (cost, index)?  An index >= P marks "none": a lane without a permutation, or a NaN cost.
__device__ __forceinline__ bool goes_first(float c2, int p2, float c1, int p1, int P) {
    if (p2 >= P) return false;
    if (p1 >= P) return true;
    return c2 < c1 || (c2 == c1 && p2 < p1);
}

// One workgroup of 256: the index of the permutation with the lowest cost sum_s q[s S + perm[s]] (added in s order), the lowest index
// among equals, 0 -- the identity -- where every cost is NaN.  q [S S], sc [256], sp [256] are LDS; q is filled and the workgroup
// synchronised before the call; every thread calls it and gets the same answer.
__device__ __forceinline__ int best_perm(const float* q, float* sc, int* sp, const int* __restrict__ perms, int S, int P) {
    const int tid = threadIdx.x;
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
    return sp[0] < P ? sp[0] : 0;
}

// one wave: trk[0, k] = k, trk[c + 1, k] = rel[c][trk[c, k]] over the C chunks of one recording; rel goes through LDS TILE words at a
// time (coalesced loads, LDS-latency chain)
__device__ __forceinline__ void chain_walk(const int* __restrict__ rel, int* __restrict__ trk, int C, int S) {
    __shared__ int sr[TILE];
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
// fl(fl(fl(1 - wh) t) + fl(wh r)): the tail t of the chunk before fades out, the head r of this one fades in
__device__ __forceinline__ float fade(float wh, float t, float r) {
    const float wt = 1.0f - wh;
    const float a = wt * t, b = wh * r;
    return a + b;
}

__device__ __forceinline__ long chunk_of(long n, int H, int C) {
    const long c = n / H;
    return c < C - 1 ? c : C - 1;
}

// One workgroup of 256: samples [1024 blk, 1024 blk + 1024) of output k of one recording of N samples and C chunks: est [C, S, L] in the
// order trk [C, S], into orow [N].  VEC: H % 4 == 0, V % 4 == 0 and 16-byte est and w_head; orow may still be misaligned
template <bool VEC>
__device__ __forceinline__ void fade_block(const float* __restrict__ est, const int* __restrict__ trk, const float* __restrict__ w_head,
                                           float* __restrict__ orow, long N, int C, int S, int L, int H, int k, long blk) {
    const int V = L - H;
    if constexpr (VEC) {
        const long n = (blk * 256 + threadIdx.x) * 4;                      // H % 4 == 0, V % 4 == 0: a group never straddles a case
        if (n >= N) return;
        const long c1 = chunk_of(n, H, C);
        const long p = n - c1 * H;                                         // < L: inside chunk c1, and p + 3 < L
        f32x4 r = *(const f32x4*)(est + (c1 * S + trk[c1 * S + k]) * L + p);
        if (c1 > 0 && p < V) {
            const f32x4 t = *(const f32x4*)(est + ((c1 - 1) * S + trk[(c1 - 1) * S + k]) * L + H + p);
            const f32x4 wh = *(const f32x4*)(w_head + p);
#pragma unroll
            for (int e = 0; e < 4; ++e) r[e] = fade(wh[e], t[e], r[e]);
        }
        if (n + 4 <= N) {
            if (((uintptr_t)orow & 15) == 0) *(f32x4*)(orow + n) = r;
            else { orow[n] = r[0]; orow[n + 1] = r[1]; orow[n + 2] = r[2]; orow[n + 3] = r[3]; }
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (n + e < N) orow[n + e] = r[e];
        }
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const long n = blk * 1024 + j * 256 + threadIdx.x;
            if (n >= N) break;
            const long c1 = chunk_of(n, H, C);
            const long p = n - c1 * H;
            float r = est[(c1 * S + trk[c1 * S + k]) * L + p];
            if (c1 > 0 && p < V) r = fade(w_head[p], est[((c1 - 1) * S + trk[(c1 - 1) * S + k]) * L + H + p], r);
            orow[n] = r;
        }
    }
}

}  // namespace
