// Sample-rate conversion of many signals of mixed ratios in one launch (include/ams_resample_ragged.h).  A library of its
// own (libams_resample_ragged.so): include/ams_resample.h and libams_resample.so are untouched.  The arithmetic is resample_core.h's, the
// code resample.hip runs: a job is bit-equal to the single call.  One kernel per kind of input; a workgroup finds its job in the prefix of
// tile counts with scalar loads (the tables through the constant address space, as the ragged build of kmeans.hip reads its own) and
// takes the decimating, the interpolating or the copying arm -- uniformly, so the barriers of the decimating arm are safe.  One output
// sample per thread, no MFMA, no atomics, no scratch.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include "../../../include/ams_resample_ragged.h"
#include "resample_core.h"

namespace {

constexpr int JOB_WORDS = 12;
enum { J_SRC, J_NIN, J_ROWS, J_XSTRIDE, J_CH, J_UP, J_DOWN, J_TAPOFF, J_DST, J_YSTRIDE, J_NKEEP, J_TILES };
constexpr long MAX_GRID = 1L << 31;

typedef const __attribute__((address_space(4))) long rs_clong;            // the tables are uniform reads: scalar loads

inline ams_status check_launch() { return hipGetLastError() == hipSuccess ? AMS_OK : AMS_E_LAUNCH_FAILED; }

// the limits of the header for one job record; M out
inline bool job_ok(const int64_t* q, long taps_len, long* tiles) {
    const long n_in = q[J_NIN], rows = q[J_ROWS], ch = q[J_CH], up = q[J_UP], down = q[J_DOWN], n_keep = q[J_NKEEP];
    if (!ratio_ok(up, down) || ch < 0 || ch > 8 || n_in < 1 || n_in > MAX_OUT || rows < 1 || rows >= MAX_GRID) return false;
    if (ch >= 1 && rows != 1) return false;
    const long M = cdiv(n_in * up, down);                                 // <= 2^48
    if (M > MAX_OUT || n_keep < 1 || n_keep > M) return false;
    if (q[J_XSTRIDE] < n_in || q[J_YSTRIDE] < n_keep || q[J_DST] < 0) return false;
    if (q[J_SRC] % (ch ? 2 : 4)) return false;
    if (up != down) {
        const long nt = 20 * (up > down ? up : down) + 1;
        if (q[J_TAPOFF] < 0 || q[J_TAPOFF] > taps_len - nt) return false;
    }
    *tiles = rows * cdiv(n_keep, TILE);                                   // < 2^31 2^30
    return true;
}

long total_tiles(const int64_t* jobs, int J, long taps_len) {
    if (!jobs || J < 1 || taps_len < 1) return -1;
    long total = 0;
    for (int j = 0; j < J; ++j) {
        long t;
        if (!job_ok(jobs + (long)j * JOB_WORDS, taps_len, &t)) return -1;
        total += t;
        if (total >= MAX_GRID) return -1;
    }
    return total;
}

template <class Source>
struct make_source;
template <>
struct make_source<F32Source> {
    static __device__ __forceinline__ F32Source at(const void* x, long src, int) { return F32Source{(const float*)((const char*)x + src)}; }
};
template <>
struct make_source<Pcm16Source> {
    static __device__ __forceinline__ Pcm16Source at(const void* x, long src, int channels) {
        return Pcm16Source{(const int16_t*)((const char*)x + src), channels};
    }
};

// grid: prefix[J] workgroups.  table = prefix [J + 1], then the records [J, 12].
template <class Source>
__global__ __launch_bounds__(TILE) void ragged_kernel(const void* __restrict__ x, const float* __restrict__ taps, const long* __restrict__ table,
                                                      int J, float* __restrict__ y) {
    __shared__ float xs[KC];
    rs_clong* prefix = (rs_clong*)table;
    const long b = blockIdx.x;
    int lo = 0, hi = J;                                                   // prefix[lo] <= b < prefix[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (prefix[mid] <= b) lo = mid;
        else hi = mid;
    }
    rs_clong* q = prefix + (J + 1) + (long)lo * JOB_WORDS;
    const long local = b - prefix[lo], tiles = q[J_TILES];
    const long row = local / tiles, n0 = (local - row * tiles) * TILE;
    const long N = q[J_NIN], n_keep = q[J_NKEEP];
    const int up = (int)q[J_UP], down = (int)q[J_DOWN];
    Source src = make_source<Source>::at(x, q[J_SRC], (int)q[J_CH]);
    src.advance(row * q[J_XSTRIDE]);
    const float* h = taps + q[J_TAPOFF];
    float* yr = y + q[J_DST] + row * q[J_YSTRIDE];
    const int tid = threadIdx.x;
    const long n = n0 + tid;
    if (down > up) {                                                      // uniform: all 256 threads reach the barriers of decimate_tile
        const float acc = decimate_tile(src, xs, N, h, up, down, n0, n_keep, tid);
        if (n < n_keep) yr[n] = acc;
    } else if (up > down) {
        if (n < n_keep) yr[n] = interpolate_one(src, N, h, up, down, n);
    } else {
        if (n < n_keep) yr[n] = src(n);                                   // up = down = 1: the decode and down-mix, or a copy
    }
}

template <class Source>
ams_status run(const void* x, const float* taps, long taps_len, const int64_t* jobs, int J, const int64_t* table, float* y, long y_len,
               bool pcm, void* stream) {
    if (!x || !taps || !jobs || !table || !y) return AMS_E_INVALID_ARG;
    const long grid = total_tiles(jobs, J, taps_len);
    if (grid < 1) return AMS_E_INVALID_ARG;
    for (int j = 0; j < J; ++j) {
        const int64_t* q = jobs + (long)j * JOB_WORDS;
        if ((q[J_CH] >= 1) != pcm) return AMS_E_INVALID_ARG;
        // the last kept output of the last row lies inside y (y_stride and rows are bounded above: no overflow below 2^63 for y_len < 2^62)
        if (y_len < 1 || q[J_DST] > y_len - q[J_NKEEP]) return AMS_E_INVALID_ARG;
        if (q[J_ROWS] > 1 && q[J_YSTRIDE] > (y_len - q[J_NKEEP] - q[J_DST]) / (q[J_ROWS] - 1)) return AMS_E_INVALID_ARG;
    }
    hipLaunchKernelGGL(ragged_kernel<Source>, dim3((unsigned)grid), dim3(TILE), 0, (hipStream_t)stream, x, taps, (const long*)table, J, y);
    return check_launch();
}

}  // namespace

extern "C" {

int ams_rsr_abi_version(void) { return 1; }

long ams_rsr_tiles(const int64_t* jobs, int J, long taps_len) { return total_tiles(jobs, J, taps_len); }

ams_status ams_rsr_tables(const int64_t* jobs, int J, long taps_len, int64_t* table) {
    if (!table || total_tiles(jobs, J, taps_len) < 1) return AMS_E_INVALID_ARG;
    int64_t* rec = table + J + 1;
    table[0] = 0;
    for (int j = 0; j < J; ++j) {
        const int64_t* q = jobs + (long)j * JOB_WORDS;
        int64_t* r = rec + (long)j * JOB_WORDS;
        for (int w = 0; w < JOB_WORDS; ++w) r[w] = q[w];
        r[J_TILES] = cdiv(q[J_NKEEP], TILE);
        if (q[J_UP] == q[J_DOWN]) r[J_TAPOFF] = 0;                        // (not looked at: no address is formed from a stray value)
        table[j + 1] = table[j] + q[J_ROWS] * r[J_TILES];
    }
    return AMS_OK;
}

ams_status ams_rsr_run_pcm16(const int16_t* x, const float* taps, long taps_len, const int64_t* jobs, int J, const int64_t* table, float* y,
                             long y_len, void* stream) {
    return run<Pcm16Source>(x, taps, taps_len, jobs, J, table, y, y_len, true, stream);
}

ams_status ams_rsr_run_f32(const float* x, const float* taps, long taps_len, const int64_t* jobs, int J, const int64_t* table, float* y,
                           long y_len, void* stream) {
    return run<F32Source>(x, taps, taps_len, jobs, J, table, y, y_len, false, stream);
}

}  // extern "C"
