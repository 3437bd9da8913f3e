// Choosing the number of clusters of every segment of a ragged point set (include/ams_spk_count.h): libams_spk_count.so.
//
// The sweep reads every point ONCE for all candidates: a workgroup takes one chunk of 8192 points of one segment from the work table of
// include/ams_kmeans_ragged.h, picks every candidate's try from the inertias itself, keeps the chosen centroids of all candidates (at
// most 2 + 3 + 4 + 5 + 6 = 20) in LDS as float64, stages 256 points at a time through LDS with coalesced loads and lets every lane
// score one point against all of them.  The sums are float64, added in a fixed order (the header), without atomics: the chunk totals go
// to the workspace and a second launch adds them per segment.
#include "../common.h"
#include "../../../include/ams_spk_count.h"

thread_local int g_ams_last_hip_error = 0;      // (common.h: this library keeps its own)

namespace {

constexpr int CHUNK = 8192;                     // points per chunk: the chunks of the table (ams_kmeans_ragged.h)
constexpr int LANES = 256;
constexpr int MAXCAND = 5;                      // candidates 2 .. 6
constexpr int MAXCENT = 20;                     // 2 + 3 + 4 + 5 + 6

struct SpkcArgs {
    const float* xn; const float* w; const int32_t* tab; const long* p_off; const long* g_off;
    const float* cent_all; const float* inertia_all;
    int R, tries, c_lo, c_hi;
    double* part;                               // [Gtot, ncand + 1]: sum w s per candidate, then sum w
    double* score; int32_t* tries_out; float* sel_all;
};

// the first try with the smallest FINITE inertia; -1 if there is none
__device__ __forceinline__ int finite_first_min(const float* __restrict__ inertia, int tries) {
    int bt = -1;
    float bv = 0.0f;
    for (int t = 0; t < tries; ++t) {
        const float v = inertia[t];
        if (!__builtin_isfinite(v)) continue;
        if (bt < 0 || v < bv) { bv = v; bt = t; }
    }
    return bt;
}

// the try kmeans_select_kernel (csrc/kmeans.hip) picks: the first NaN if there is one, else the first minimum (np.argmin)
__device__ __forceinline__ int select_try(const float* __restrict__ inertia, int tries) {
    int bt = 0;
    float bv = inertia[0];
    for (int t = 1; t < tries; ++t) {
        const float v = inertia[t];
        if (bv == bv && !(bv <= v)) { bv = v; bt = t; }
    }
    return bt;
}

// centroid j of the c_lo + (c_lo + 1) + .. rows of all candidates -> (candidate k, rows before it, clusters of it)
__device__ __forceinline__ void which_candidate(int j, int c_lo, int& k, int& pre, int& C) {
    k = 0; pre = 0; C = c_lo;
    while (j - pre >= C) { pre += C; ++k; ++C; }
}

__device__ __forceinline__ int all_centroids(int c_lo, int c_hi) { return (c_lo + c_hi) * (c_hi - c_lo + 1) / 2; }

template <int E, bool HAS_W>
__global__ __launch_bounds__(LANES) void spkc_sweep_kernel(SpkcArgs a) {
    constexpr int LD = E + 1;                                      // row pitch of the staged points: lanes read rows, 41 and 9 are odd
    __shared__ double stage_d[(LANES * LD + 1) / 2 > (MAXCAND + 1) * LANES ? (LANES * LD + 1) / 2 : (MAXCAND + 1) * LANES];
    __shared__ double cs[MAXCENT * E];
    __shared__ int try_sh[MAXCAND];
    float* const tile = reinterpret_cast<float*>(stage_d);
    const int tid = threadIdx.x;
    const int32_t* const row = a.tab + (long)blockIdx.x * 16;      // column 0 of chunk blockIdx.x of the table
    const int r = row[0], g = row[1];
    const long p0 = a.p_off[r];
    const long first = (long)g * CHUNK;
    const long left = a.p_off[r + 1] - p0 - first;
    const int n = left < CHUNK ? (int)left : CHUNK;                // points of this chunk
    const int ncand = a.c_hi - a.c_lo + 1;
    const int nct = all_centroids(a.c_lo, a.c_hi);

    if (tid < ncand) try_sh[tid] = finite_first_min(a.inertia_all + ((long)tid * a.R + r) * a.tries, a.tries);
    __syncthreads();
    for (int i = tid; i < nct * E; i += LANES) {
        const int j = i / E, e = i % E;
        int k, pre, C;
        which_candidate(j, a.c_lo, k, pre, C);
        const int t = try_sh[k];
        // (a disqualified candidate is scored against zeros: its sums are dropped by the finish)
        cs[i] = t < 0 ? 0.0 : (double)a.cent_all[((long)a.R * a.tries * pre + ((long)r * a.tries + t) * C + (j - pre)) * E + e];
    }

    double acc[MAXCAND], accw = 0.0;
#pragma unroll
    for (int k = 0; k < MAXCAND; ++k) acc[k] = 0.0;
    const float* const base = a.xn + (p0 + first) * E;
    for (int q0 = 0; q0 < n; q0 += LANES) {
        const int m = n - q0 < LANES ? n - q0 : LANES;             // points of this tile
        __syncthreads();                                           // the tile before is used up (first round: cs is written)
        for (int i = tid; i < m * E; i += LANES) tile[(i / E) * LD + i % E] = base[(long)q0 * E + i];
        __syncthreads();
        if (tid < m) {
            double x[E];
#pragma unroll
            for (int e = 0; e < E; ++e) x[e] = (double)tile[tid * LD + e];
            const double wv = HAS_W ? (double)a.w[p0 + first + q0 + tid] : 1.0;
            const double* cc = cs;
#pragma unroll
            for (int k = 0; k < MAXCAND; ++k) {
                if (k < ncand) {
                    double m1 = __builtin_inf(), m2 = __builtin_inf();         // the two smallest squared distances
                    for (int c = 0; c < a.c_lo + k; ++c, cc += E) {
                        double da = 0.0, db = 0.0;
#pragma unroll
                        for (int e = 0; e < E; e += 2) {
                            const double ta = x[e] - cc[e], tb = x[e + 1] - cc[e + 1];
                            da = fma(ta, ta, da);
                            db = fma(tb, tb, db);
                        }
                        const double d = da + db;
                        if (d < m1) { m2 = m1; m1 = d; }
                        else if (d < m2) m2 = d;
                    }
                    const double d1 = sqrt(m1), d2 = sqrt(m2);
                    acc[k] += wv * (d2 == 0.0 ? 0.0 : (d2 - d1) / d2);
                }
            }
            accw += wv;
        }
    }

    // the 256 lanes by the halving tree, all values side by side; the staging area is free now
    __syncthreads();
    double* const red = stage_d;
#pragma unroll
    for (int k = 0; k < MAXCAND; ++k) red[k * LANES + tid] = acc[k];
    red[MAXCAND * LANES + tid] = accw;
    __syncthreads();
    for (int s = LANES / 2; s > 0; s >>= 1) {
        if (tid < s) {
#pragma unroll
            for (int k = 0; k <= MAXCAND; ++k) red[k * LANES + tid] += red[k * LANES + tid + s];
        }
        __syncthreads();
    }
    if (tid <= ncand) a.part[(long)blockIdx.x * (ncand + 1) + tid] = red[(tid < ncand ? tid : MAXCAND) * LANES];
}

// one workgroup per segment: the chunk totals in chunk order, the score, the try, the selected centroids of every candidate
__global__ __launch_bounds__(64) void spkc_finish_kernel(SpkcArgs a, int E) {
    __shared__ int try_sh[MAXCAND];
    const int r = blockIdx.x, tid = threadIdx.x;
    const int ncand = a.c_hi - a.c_lo + 1;
    if (tid < ncand) {
        const float* const in = a.inertia_all + ((long)tid * a.R + r) * a.tries;
        const int t = finite_first_min(in, a.tries);
        double sws = 0.0, sw = 0.0;
        for (long g = a.g_off[r]; g < a.g_off[r + 1]; ++g) {       // sequentially, in chunk order
            sws += a.part[g * (ncand + 1) + tid];
            sw += a.part[g * (ncand + 1) + ncand];
        }
        a.score[(long)r * ncand + tid] = (t < 0 || sw == 0.0) ? -__builtin_inf() : sws / sw;
        a.tries_out[(long)r * ncand + tid] = t;
        try_sh[tid] = t >= 0 ? t : select_try(in, a.tries);
    }
    __syncthreads();
    const int nct = all_centroids(a.c_lo, a.c_hi);
    for (int i = tid; i < nct * E; i += 64) {
        const int j = i / E, e = i % E;
        int k, pre, C;
        which_candidate(j, a.c_lo, k, pre, C);
        a.sel_all[((long)a.R * pre + (long)r * C + (j - pre)) * E + e] =
            a.cent_all[((long)a.R * a.tries * pre + ((long)r * a.tries + try_sh[k]) * C + (j - pre)) * E + e];
    }
}

__global__ __launch_bounds__(64) void spkc_choose_kernel(const double* __restrict__ score, const float* __restrict__ sel_all, int R, int E,
                                                         int lo, int c_lo, int c_hi, int has_min, double min_score,
                                                         int32_t* __restrict__ count, int32_t* __restrict__ cand,
                                                         float* __restrict__ chosen) {
    const int r = blockIdx.x, tid = threadIdx.x;
    const int ncand = c_hi - c_lo + 1;
    int kb = 0;
    double best = score[(long)r * ncand];
    for (int k = 1; k < ncand; ++k) {
        const double v = score[(long)r * ncand + k];
        if (v > best) { best = v; kb = k; }                        // the first maximum
    }
    int n, cd;
    if (best == -__builtin_inf()) {                                // every candidate is disqualified
        if (lo == 1) { n = 1; cd = -1; }
        else { n = c_lo; cd = 0; }
    } else if (lo == 1 && has_min && best < min_score) { n = 1; cd = -1; }
    else { n = c_lo + kb; cd = kb; }
    if (tid == 0) { count[r] = n; cand[r] = cd; }
    int pre = 0;
    for (int k = 0; k < cd; ++k) pre += c_lo + k;
    for (int i = tid; i < c_hi * E; i += 64) {
        const int c = i / E;
        chosen[(long)r * c_hi * E + i] = (cd >= 0 && c < n) ? sel_all[((long)R * pre + (long)r * n) * E + i] : 0.0f;
    }
}

__global__ __launch_bounds__(LANES) void spkc_labels_kernel(const int32_t* __restrict__ labels_all, const int32_t* __restrict__ cand,
                                                            const int32_t* __restrict__ tab, const long* __restrict__ p_off, long Ptot,
                                                            int32_t* __restrict__ labels) {
    const int32_t* const row = tab + (long)blockIdx.x * 16;
    const int r = row[0], g = row[1];
    const long p0 = p_off[r] + (long)g * CHUNK;
    const long left = p_off[r + 1] - p0;
    const int n = left < CHUNK ? (int)left : CHUNK;
    const int cd = cand[r];
    for (int q = threadIdx.x; q < n; q += LANES) labels[p0 + q] = cd < 0 ? 0 : labels_all[(long)cd * Ptot + p0 + q];
}

bool spkc_domain(int E, int c_lo, int c_hi) { return (E == 40 || E == 8) && c_lo >= 2 && c_lo <= c_hi && c_hi <= 6; }
bool spkc_sizes(int R, long Gtot) { return R >= 1 && Gtot >= R && 4 * Gtot < (1L << 31); }

}  // namespace

extern "C" {

int ams_spkc_abi_version(void) { return 1; }

size_t ams_spkc_workspace_bytes(int R, long Gtot, int E, int c_lo, int c_hi) {
    if (!spkc_domain(E, c_lo, c_hi) || !spkc_sizes(R, Gtot)) return 0;
    return sizeof(double) * (size_t)Gtot * (size_t)(c_hi - c_lo + 2);
}

ams_status ams_spkc_score(const float* xn, const float* w, const int32_t* tab, const int64_t* p_off, const int64_t* g_off,
                          const float* cent_all, const float* inertia_all, int R, int tries, long Gtot, int E, int c_lo, int c_hi,
                          void* ws, size_t ws_bytes, double* score, int32_t* tries_out, float* sel_all, void* stream) {
    AMS_REQUIRE(xn && tab && p_off && g_off && cent_all && inertia_all && ws && score && tries_out && sel_all && tries >= 1 &&
                spkc_domain(E, c_lo, c_hi) && spkc_sizes(R, Gtot));
    if (ws_bytes < ams_spkc_workspace_bytes(R, Gtot, E, c_lo, c_hi)) return AMS_E_WORKSPACE_TOO_SMALL;
    SpkcArgs a{};
    a.xn = xn; a.w = w; a.tab = tab; a.p_off = (const long*)p_off; a.g_off = (const long*)g_off;
    a.cent_all = cent_all; a.inertia_all = inertia_all; a.R = R; a.tries = tries; a.c_lo = c_lo; a.c_hi = c_hi;
    a.part = (double*)ws; a.score = score; a.tries_out = tries_out; a.sel_all = sel_all;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)Gtot);
    if (E == 40) {
        if (w) hipLaunchKernelGGL((spkc_sweep_kernel<40, true>), grid, dim3(LANES), 0, st, a);
        else hipLaunchKernelGGL((spkc_sweep_kernel<40, false>), grid, dim3(LANES), 0, st, a);
    } else {
        if (w) hipLaunchKernelGGL((spkc_sweep_kernel<8, true>), grid, dim3(LANES), 0, st, a);
        else hipLaunchKernelGGL((spkc_sweep_kernel<8, false>), grid, dim3(LANES), 0, st, a);
    }
    ams_status s = ams_check_launch();
    if (s != AMS_OK) return s;
    hipLaunchKernelGGL(spkc_finish_kernel, dim3((unsigned)R), dim3(64), 0, st, a, E);
    return ams_check_launch();
}

ams_status ams_spkc_choose(const double* score, const float* sel_all, int R, int E, int lo, int c_lo, int c_hi, const double* min_score,
                           int32_t* count, int32_t* cand, float* chosen, void* stream) {
    AMS_REQUIRE(score && sel_all && count && cand && chosen && R >= 1 && spkc_domain(E, c_lo, c_hi));
    AMS_REQUIRE((lo == 1 && c_lo == 2 && min_score) || lo == c_lo);
    hipLaunchKernelGGL(spkc_choose_kernel, dim3((unsigned)R), dim3(64), 0, (hipStream_t)stream, score, sel_all, R, E, lo, c_lo, c_hi,
                       min_score ? 1 : 0, min_score ? *min_score : 0.0, count, cand, chosen);
    return ams_check_launch();
}

ams_status ams_spkc_labels(const int32_t* labels_all, const int32_t* cand, const int32_t* tab, const int64_t* p_off, int R, long Gtot,
                           long Ptot, int c_lo, int c_hi, int32_t* labels, void* stream) {
    AMS_REQUIRE(labels_all && cand && tab && p_off && labels && spkc_domain(40, c_lo, c_hi) && spkc_sizes(R, Gtot) && Ptot >= R);
    hipLaunchKernelGGL(spkc_labels_kernel, dim3((unsigned)Gtot), dim3(LANES), 0, (hipStream_t)stream, labels_all, cand, tab,
                       (const long*)p_off, Ptot, labels);
    return ams_check_launch();
}

}  // extern "C"
