// k-means++ (D^2) seeding of every segment of a ragged point set (include/ams_kmeans_seed.h): libams_kmeans_seed.so.
//
// The sampling weights are integers (the header: quant), so every sum is exact and the seeds do not depend on who adds what first.  A
// step is two launches.  The weighing takes one chunk of 8192 points of one segment from the work table of include/ams_kmeans_ragged.h
// per workgroup, holds the seed rows chosen so far of up to TB tries of its segment in LDS, stages 256 points at a time through LDS with
// coalesced loads, lets every lane weigh one point against all of them and leaves the chunk's sum per try in the workspace: plain
// stores by one lane each, no atomics.  The pick, one workgroup per (segment, try), finds the chunk that holds the target from those
// sums, weighs that one chunk again and scans it in point order.  The distances are recomputed against all chosen seeds at every step:
// there is no [tries, Ptot] running minimum.  Compiled without FMA contraction: d is the hard distance of csrc/kmeans.hip.
#include "../common.h"
#include "../../../include/ams_kmeans_seed.h"

thread_local int g_ams_last_hip_error = 0;      // (common.h: this library keeps its own)

namespace {

constexpr int CHUNK = 8192;                     // points per chunk: the chunks of the table (ams_kmeans_ragged.h)
constexpr int LANES = 256;
constexpr int WAVES = LANES / 64;
constexpr int TB = 16;                          // tries weighed per read of the points
constexpr int MAXSEED = 5;                      // seeds chosen before the last step of C = 6
typedef unsigned long long u64;

struct KmsArgs {
    const float* xn; const float* w; const int32_t* tab; const long* p_off; const long* g_off; const u64* draws;
    int R, tries, C, c;                         // c: the step, the column of seeds to fill
    u64* part;                                  // [Gtot, tries]: the sum of q over the chunk
    int32_t* seeds;
};

__device__ __forceinline__ unsigned quant(float v) {
    if (!(v > 0.0f)) return 0u;                                    // a NaN or v <= 0
    return (unsigned)(fminf(v, 2048.0f) * 1048576.0f);            // exact: a power of two; at most 2^31
}

// oracle/kmeans.py::sqdist: left to right over e, every square rounded before it is weighted and added
template <int E, bool HAS_W>
__device__ __forceinline__ float sqdist(const float* __restrict__ x, const float* __restrict__ s, float wv) {
    float d = 0.0f;
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const float t = x[e] - s[e];
        const float sq = t * t;
        d = d + (HAS_W ? sq * wv : sq);
    }
    return d;
}

// q of a point at step c >= 1 against the c seed rows at sd
template <int E, bool HAS_W>
__device__ __forceinline__ unsigned q_point(const float* __restrict__ x, float wv, const float* __restrict__ sd, int c) {
    unsigned q = 0xFFFFFFFFu;
    for (int j = 0; j < c; ++j) {
        const unsigned v = quant(sqdist<E, HAS_W>(x, sd + j * E, wv));
        q = v < q ? v : q;
    }
    return q;
}

__device__ __forceinline__ u64 wave_sum(u64 v) {                  // lane 0 of the wavefront holds the sum
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) v += __shfl_down(v, s);
    return v;
}

// a seed read back from the buffer, held inside the segment whatever the word is: never an out-of-range row
__device__ __forceinline__ long seed_row(int s, long P) { return s < 0 ? 0 : (s >= P ? P - 1 : s); }

template <int E, bool HAS_W>
__global__ __launch_bounds__(LANES) void kms_weigh_kernel(KmsArgs a) {
    constexpr int LD = E + 1;                                      // row pitch of the staged points: lanes read rows, 41 and 9 are odd
    __shared__ float tile[LANES * LD];
    __shared__ float sd[TB * MAXSEED * E];
    __shared__ u64 wsum[TB * WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int32_t* const row = a.tab + (long)blockIdx.x * 16;      // column 0 of chunk blockIdx.x of the table
    const int r = row[0], g = row[1];
    const long p0 = a.p_off[r], P = a.p_off[r + 1] - p0;
    const long first = (long)g * CHUNK;
    const long left = P - first;
    const int n = left < CHUNK ? (int)left : CHUNK;                // points of this chunk
    const float* const base = a.xn + (p0 + first) * E;
    const float* const wb = HAS_W ? a.w + p0 + first : nullptr;
    u64* const out = a.part + (long)blockIdx.x * a.tries;
    const int c = a.c;

    if (c == 0) {                                                  // the weights themselves: one sum for every try
        u64 acc = 0;
        for (int q = tid; q < n; q += LANES) acc += HAS_W ? quant(wb[q]) : (1u << 20);
        acc = wave_sum(acc);
        if (lane == 0) wsum[wave] = acc;
        __syncthreads();
        u64 tot = 0;
#pragma unroll
        for (int k = 0; k < WAVES; ++k) tot += wsum[k];
        for (int t = tid; t < a.tries; t += LANES) out[t] = tot;
        return;
    }

    for (int t0 = 0; t0 < a.tries; t0 += TB) {
        const int nt = a.tries - t0 < TB ? a.tries - t0 : TB;
        __syncthreads();                                           // the seed rows and sums of the batch before are used up
        for (int i = tid; i < nt * c * E; i += LANES) {
            const int t = i / (c * E), j = (i / E) % c, e = i % E;
            const long s = seed_row(a.seeds[((long)r * a.tries + t0 + t) * a.C + j], P);
            sd[(t * MAXSEED + j) * E + e] = a.xn[(p0 + s) * E + e];
        }
        u64 acc[TB];
#pragma unroll
        for (int t = 0; t < TB; ++t) acc[t] = 0;
        for (int q0 = 0; q0 < n; q0 += LANES) {
            const int m = n - q0 < LANES ? n - q0 : LANES;         // points of this tile
            __syncthreads();                                       // the tile before is used up (first round: sd is written)
            for (int i = tid; i < m * E; i += LANES) tile[(i / E) * LD + i % E] = base[(long)q0 * E + i];
            __syncthreads();
            if (tid < m) {
                float x[E];
#pragma unroll
                for (int e = 0; e < E; ++e) x[e] = tile[tid * LD + e];
                const float wv = HAS_W ? wb[q0 + tid] : 1.0f;
#pragma unroll
                for (int t = 0; t < TB; ++t)
                    if (t < nt) acc[t] += q_point<E, HAS_W>(x, wv, sd + t * MAXSEED * E, c);
            }
        }
#pragma unroll
        for (int t = 0; t < TB; ++t) {
            const u64 v = wave_sum(acc[t]);
            if (lane == 0) wsum[t * WAVES + wave] = v;
        }
        __syncthreads();
        if (tid < nt) {
            u64 tot = 0;
#pragma unroll
            for (int k = 0; k < WAVES; ++k) tot += wsum[tid * WAVES + k];
            out[t0 + tid] = tot;
        }
    }
}

template <int E, bool HAS_W>
__global__ __launch_bounds__(LANES) void kms_pick_kernel(KmsArgs a) {
    constexpr int LD = E + 1;
    __shared__ float tile[LANES * LD];
    __shared__ float sd[MAXSEED * E];
    __shared__ u64 lsum[LANES];
    __shared__ u64 wsum[WAVES];
    __shared__ u64 sh_resid;
    __shared__ long sh_chunk;
    __shared__ int sh_scan;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = blockIdx.x / a.tries, t = blockIdx.x % a.tries;
    const long rowi = (long)r * a.tries + t;
    int32_t* const my = a.seeds + rowi * a.C;
    const long g0 = a.g_off[r], G = a.g_off[r + 1] - g0;
    const long p0 = a.p_off[r], P = a.p_off[r + 1] - p0;
    const int c = a.c;

    // the segment's chunk sums of this try: lane l adds chunks l k .. l k + k - 1
    const long k = (G + LANES - 1) / LANES;
    {
        u64 ls = 0;
        const long i1 = (tid + 1) * k < G ? (tid + 1) * k : G;
        for (long i = tid * k; i < i1; ++i) ls += a.part[(g0 + i) * a.tries + t];
        lsum[tid] = ls;
    }
    for (int i = tid; i < c * E; i += LANES) sd[i] = a.xn[(p0 + seed_row(my[i / E], P)) * E + i % E];
    __syncthreads();
    if (tid == 0) {
        u64 total = 0;
        for (int l = 0; l < LANES; ++l) total += lsum[l];
        if (total == 0) {                                          // nothing to sample from: the smallest index that is no seed yet
            int pick = 0;
            for (bool used = true; used;) {
                used = false;
                for (int j = 0; j < c; ++j) used = used || my[j] == pick;
                if (used) ++pick;
            }
            my[c] = pick;
            sh_scan = 0;
        } else {
            const u64 target = __umul64hi(a.draws[rowi * a.C + c], total);     // < total
            u64 pre = 0;
            int l = 0;
            while (l < LANES - 1 && pre + lsum[l] <= target) pre += lsum[l++];
            long i = l * k;
            for (; i < G - 1; ++i) {                               // (a chunk whose sum is zero is passed over)
                const u64 v = a.part[(g0 + i) * a.tries + t];
                if (pre + v > target) break;
                pre += v;
            }
            sh_chunk = i;
            sh_resid = target - pre;
            sh_scan = 1;
        }
    }
    __syncthreads();
    if (!sh_scan) return;

    // that chunk's q again, and the prefix sums in point order: the one point whose (exclusive, inclusive] sums hold the residual
    const long first = sh_chunk * CHUNK;
    const u64 resid = sh_resid;
    const long left = P - first;
    const int n = left < CHUNK ? (int)left : CHUNK;
    const float* const base = a.xn + (p0 + first) * E;
    const float* const wb = HAS_W ? a.w + p0 + first : nullptr;
    u64 running = 0;
    for (int q0 = 0; q0 < n; q0 += LANES) {
        const int m = n - q0 < LANES ? n - q0 : LANES;
        __syncthreads();                                           // the tile and the wave sums before are used up
        if (c > 0) {
            for (int i = tid; i < m * E; i += LANES) tile[(i / E) * LD + i % E] = base[(long)q0 * E + i];
            __syncthreads();
        }
        unsigned q = 0;
        if (tid < m) {
            const float wv = HAS_W ? wb[q0 + tid] : 1.0f;
            if (c == 0) q = HAS_W ? quant(wv) : (1u << 20);
            else {
                float x[E];
#pragma unroll
                for (int e = 0; e < E; ++e) x[e] = tile[tid * LD + e];
                q = q_point<E, HAS_W>(x, wv, sd, c);
            }
        }
        u64 incl = q;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const u64 o = __shfl_up(incl, d);
            if (lane >= d) incl += o;
        }
        if (lane == 63) wsum[wave] = incl;
        __syncthreads();
        u64 off = running, tot = 0;
#pragma unroll
        for (int w2 = 0; w2 < WAVES; ++w2) {
            if (w2 < wave) off += wsum[w2];
            tot += wsum[w2];
        }
        const u64 mine = off + incl;
        if (q > 0 && mine - q <= resid && resid < mine) my[c] = (int32_t)(first + q0 + tid);
        running += tot;
        if (running > resid) break;                                // (the same for every lane)
    }
}

bool kms_domain(int E, int C) { return (E == 40 || E == 8) && C >= 1 && C <= 6; }
bool kms_sizes(int R, int tries, long Gtot) { return R >= 1 && tries >= 1 && Gtot >= R && 4 * Gtot < (1L << 31) && (long)R * tries < (1L << 31); }

template <int E, bool HAS_W>
ams_status kms_launch_step(const KmsArgs& a, long Gtot, hipStream_t st) {
    hipLaunchKernelGGL((kms_weigh_kernel<E, HAS_W>), dim3((unsigned)Gtot), dim3(LANES), 0, st, a);
    ams_status s = ams_check_launch();
    if (s != AMS_OK) return s;
    hipLaunchKernelGGL((kms_pick_kernel<E, HAS_W>), dim3((unsigned)((long)a.R * a.tries)), dim3(LANES), 0, st, a);
    return ams_check_launch();
}

ams_status kms_steps(const float* xn, const float* w, const int32_t* tab, const int64_t* p_off, const int64_t* g_off, const uint64_t* draws,
                     int R, int tries, long Gtot, int E, int C, int c0, int c1, void* ws, size_t ws_bytes, int32_t* seeds, void* stream) {
    AMS_REQUIRE(xn && tab && p_off && g_off && draws && ws && seeds && kms_domain(E, C) && kms_sizes(R, tries, Gtot) && c0 >= 0 && c1 <= C);
    if (ws_bytes < ams_kms_workspace_bytes(R, tries, Gtot, E, C)) return AMS_E_WORKSPACE_TOO_SMALL;
    KmsArgs a{};
    a.xn = xn; a.w = w; a.tab = tab; a.p_off = (const long*)p_off; a.g_off = (const long*)g_off; a.draws = (const u64*)draws;
    a.R = R; a.tries = tries; a.C = C; a.part = (u64*)ws; a.seeds = seeds;
    hipStream_t st = (hipStream_t)stream;
    for (int c = c0; c < c1; ++c) {
        a.c = c;
        ams_status s;
        if (E == 40) s = w ? kms_launch_step<40, true>(a, Gtot, st) : kms_launch_step<40, false>(a, Gtot, st);
        else s = w ? kms_launch_step<8, true>(a, Gtot, st) : kms_launch_step<8, false>(a, Gtot, st);
        if (s != AMS_OK) return s;
    }
    return AMS_OK;
}

}  // namespace

extern "C" {

int ams_kms_abi_version(void) { return 1; }

size_t ams_kms_workspace_bytes(int R, int tries, long Gtot, int E, int C) {
    if (!kms_domain(E, C) || !kms_sizes(R, tries, Gtot)) return 0;
    return sizeof(u64) * (size_t)Gtot * (size_t)tries;
}

ams_status ams_kms_step(const float* xn, const float* w, const int32_t* tab, const int64_t* p_off, const int64_t* g_off,
                        const uint64_t* draws, int R, int tries, long Gtot, int E, int C, int c, void* ws, size_t ws_bytes, int32_t* seeds,
                        void* stream) {
    AMS_REQUIRE(c >= 0 && c < C);
    return kms_steps(xn, w, tab, p_off, g_off, draws, R, tries, Gtot, E, C, c, c + 1, ws, ws_bytes, seeds, stream);
}

ams_status ams_kms_seed(const float* xn, const float* w, const int32_t* tab, const int64_t* p_off, const int64_t* g_off,
                        const uint64_t* draws, int R, int tries, long Gtot, int E, int C, void* ws, size_t ws_bytes, int32_t* seeds,
                        void* stream) {
    return kms_steps(xn, w, tab, p_off, g_off, draws, R, tries, Gtot, E, C, 0, C, ws, ws_bytes, seeds, stream);
}

}  // extern "C"
