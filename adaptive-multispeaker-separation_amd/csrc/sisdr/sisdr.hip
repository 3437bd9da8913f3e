// Scale-invariant SDR with rectangular matching over a ragged set of recordings (include/ams_sisdr.h): libams_sisdr.so.
//
// Everything the definition needs of a recording follows from one Gram matrix: the products of {references, mixture, a row of ones} with
// every row, and every row's own square.  The sweep reads every float32 sample ONCE: a workgroup takes one block of 4096 samples of one
// recording from the work table, stages its rows tile by tile in LDS (plus a row of ones and a row of zeros, so that the inner loop has
// no bounds), and every thread owns a sample phase and a strip of 8 x 7 products in float64 registers (the sums of the rows are the
// products with the row of ones; a column of ones would only repeat them).  The partials of a block go to
// the workspace and the second launch adds them per recording in block order, centres, fills the pair table and searches the
// assignments.  No atomics; this translation unit is compiled without FMA contraction: the fused multiply-adds below are explicit.
#include "../common.h"
#include "../../../include/ams_sisdr.h"

thread_local int g_ams_last_hip_error = 0;      // (common.h: this library keeps its own)

namespace {

constexpr int BLOCK = 4096;                     // samples per row of the work table
constexpr int LANES = 256;
constexpr int NA = 8;                           // rows of the left factor: <= 6 references, the mixture, ones
constexpr int NC = 56;                          // columns: <= 55 rows
constexpr int GC = 7;                           // columns per thread
constexpr int PART = NA * NC + NC;              // float64 per block partial: the products [8, 56], then the squares [56]
constexpr int TILE_FLOATS = 9216;               // (nrows + 2) * T <= 9216 for every G: 9 * 1024, 16 * 512, 30 * 256, 57 * 128
constexpr int MAXS = 6;

struct SisdrArgs {
    const float* x; const long* rows; const long* rec; const int32_t* cnt; const int32_t* tab;
    int R, K, zero_mean;
    double* part;                               // [Btot, PART]
    double* pair; int32_t* match_ref; int32_t* match_est; double* si_sdr; double* si_sdri; int32_t* missed; int32_t* spurious;
    double* base; int32_t* info;
};

__device__ __forceinline__ int groups_of(int nc) { return nc <= GC ? 1 : nc <= 2 * GC ? 2 : nc <= 4 * GC ? 4 : 8; }

__global__ __launch_bounds__(LANES) void sisdr_gram_kernel(SisdrArgs a) {
    __shared__ double sh_d[TILE_FLOATS / 2];
    __shared__ long row_off[NC];                                   // the recording's row offsets: read once, not once per sample
    float* const tile = reinterpret_cast<float*>(sh_d);
    const int tid = threadIdx.x;
    const int r = a.tab[2 * (long)blockIdx.x], b = a.tab[2 * (long)blockIdx.x + 1];
    const long L = a.rec[4 * (long)r];
    const int Sr = a.cnt[16 * (long)r], nrows = a.cnt[16 * (long)r + 1];
    const int nc = nrows;                                          // one column per row
    const int G = groups_of(nc);
    const int P = LANES / G;                                       // sample phases
    const int lgT = G == 1 ? 10 : G == 2 ? 9 : G == 4 ? 8 : 7;
    const int T = 1 << lgT;                                        // samples per tile
    const int g = tid / P, p = tid % P;
    const long s0 = (long)b * BLOCK;
    const int n = L - s0 < BLOCK ? (int)(L - s0) : BLOCK;          // samples of this block
    const long* const rows = a.rows + (long)NC * r;
    const int ONES = nrows, ZEROS = nrows + 1;                     // two constant rows of the tile

    // where this thread's operands lie in a tile
    int ra[NA], rc[GC];
#pragma unroll
    for (int i = 0; i < NA; ++i) ra[i] = (i <= Sr ? i : i == Sr + 1 ? ONES : ZEROS) << lgT;
#pragma unroll
    for (int j = 0; j < GC; ++j) rc[j] = (GC * g + j < nc ? GC * g + j : ZEROS) << lgT;
    const bool upper = Sr + 2 > 4;                                 // rows 4 .. 7 of the left factor are in use

    for (int t = tid; t < T; t += LANES) { tile[(ONES << lgT) + t] = 1.0f; tile[(ZEROS << lgT) + t] = 0.0f; }
    if (tid < nrows) row_off[tid] = rows[tid] + s0;

    double acc[NA][GC], sq[GC];
#pragma unroll
    for (int j = 0; j < GC; ++j) {
        sq[j] = 0.0;
#pragma unroll
        for (int i = 0; i < NA; ++i) acc[i][j] = 0.0;
    }
    for (int t0 = 0; t0 < n; t0 += T) {
        const int m = n - t0 < T ? n - t0 : T;                     // samples of this tile
        __syncthreads();                                           // the tile before is used up
#pragma unroll 4
        for (int i = tid; i < nrows << lgT; i += LANES) {          // (independent loads: several are in flight per thread)
            const int j = i >> lgT, t = i & (T - 1);
            if (t < m) tile[i] = a.x[row_off[j] + t0 + t];
        }
        __syncthreads();
        for (int t = p; t < m; t += P) {
            double cv[GC];
#pragma unroll
            for (int j = 0; j < GC; ++j) {
                cv[j] = (double)tile[rc[j] + t];
                sq[j] = fma(cv[j], cv[j], sq[j]);
            }
#pragma unroll
            for (int i = 0; i < NA / 2; ++i) {
                const double av = (double)tile[ra[i] + t];
#pragma unroll
                for (int j = 0; j < GC; ++j) acc[i][j] = fma(av, cv[j], acc[i][j]);
            }
            if (upper) {
#pragma unroll
                for (int i = NA / 2; i < NA; ++i) {
                    const double av = (double)tile[ra[i] + t];
#pragma unroll
                    for (int j = 0; j < GC; ++j) acc[i][j] = fma(av, cv[j], acc[i][j]);
                }
            }
        }
    }

    // the 32 phases of a half wave: a butterfly that halves the values a lane carries at every step.  Lane l ends with values
    // 32 b0 + 16 b1 + 8 b2 + 4 b3 + 2 b4 + {0, 1} (b_i: bit i of l) summed over its half wave
    double v[64];
#pragma unroll
    for (int i = 0; i < NA; ++i) {
#pragma unroll
        for (int j = 0; j < GC; ++j) v[i * GC + j] = acc[i][j];
    }
#pragma unroll
    for (int j = 0; j < GC; ++j) v[NA * GC + j] = sq[j];
    v[63] = 0.0;
    int idx = 0;
#pragma unroll
    for (int bit = 0; bit < 5; ++bit) {
        const int H = 32 >> bit;
        const bool up = (tid >> bit) & 1;
        idx += up ? H : 0;
#pragma unroll
        for (int i = 0; i < H; ++i) {
            const double send = up ? v[i] : v[i + H];
            const double keep = up ? v[i + H] : v[i];
            v[i] = keep + __shfl_xor(send, 1 << bit);
        }
    }
    __syncthreads();                                               // the last tile is used up
    double* const red = sh_d;                                      // [8 half waves, 64 values]
    const int hw = tid >> 5;
    red[hw * 64 + idx] = v[0];
    red[hw * 64 + idx + 1] = v[1];
    __syncthreads();
    for (int o = tid; o < 64 * G; o += LANES) {
        const int gg = o >> 6, q = o & 63;
        const int per = 8 / G;                                     // half waves of one group of columns, in order
        double s = red[(gg * per) * 64 + q];
        for (int h = 1; h < per; ++h) s += red[(gg * per + h) * 64 + q];
        double* const out = a.part + (long)blockIdx.x * PART;
        if (q < NA * GC) {
            const int i = q / GC, c = GC * gg + q % GC;
            if (i < Sr + 2 && c < nc) out[i * NC + c] = s;
        } else if (q < NA * GC + GC) {
            const int c = GC * gg + (q - NA * GC);
            if (c < nc) out[NA * NC + c] = s;
        }
    }
}

// si_sdr from centred products: the edge rules of the header
__device__ __forceinline__ double si_sdr_of(double g, double ee, double ss) {
    if (!(ss > 0.0)) return __builtin_nan("");
    if (!(ee > 0.0)) return -__builtin_inf();
    const double g2 = g * g;
    const double den = ss * ee - g2;
    if (den <= 0.0) return g != 0.0 ? __builtin_inf() : -__builtin_inf();
    return 10.0 * log10(g2 / den);
}

// the number of q-tuples of distinct elements out of m
__device__ __forceinline__ int arrangements(int m, int q) {
    int v = 1;
    for (int i = 0; i < q; ++i) v *= m - i;
    return v;
}

// candidate c of itertools.permutations(range(big), n) -> t[0 .. n - 1]
__device__ __forceinline__ void unrank(int c, int big, int n, int* t) {
    unsigned avail = (1u << big) - 1u;
    for (int pos = 0; pos < n; ++pos) {
        const int after = arrangements(big - pos - 1, n - pos - 1);
        int d = c / after;
        c -= d * after;
        int e = 0;
        for (;; ++e) {
            if ((avail >> e) & 1u) {
                if (d == 0) break;
                --d;
            }
        }
        t[pos] = e;
        avail &= ~(1u << e);
    }
}

// one workgroup per (recording, set)
__global__ __launch_bounds__(LANES) void sisdr_finish_kernel(SisdrArgs a) {
    __shared__ double tot[PART];
    __shared__ double pv[MAXS * MAXS];
    __shared__ double bs[MAXS];
    __shared__ double cval[LANES];
    __shared__ int cidx[LANES];
    __shared__ int flag;
    const int tid = threadIdx.x;
    const int r = blockIdx.x / a.K, k = blockIdx.x % a.K;
    const long L = a.rec[4 * (long)r], b0 = a.rec[4 * (long)r + 1];
    const int nb = (int)((L + BLOCK - 1) / BLOCK);
    const int32_t* const cnt = a.cnt + 16 * (long)r;
    const int Sr = cnt[0], nrows = cnt[1], Se = cnt[2 + k];
    const int nc = nrows, na = Sr + 2;
    int e0 = Sr + 1;                                               // the first row of set k
    for (int j = 0; j < k; ++j) e0 += cnt[2 + j];
    if (tid == 0) flag = 0;

    // the block partials in ascending block order
    for (int i = tid; i < PART; i += LANES) {
        const int row = i / NC, c = i % NC;
        double s = 0.0;
        if (c < nc && (row == NA || row < na)) {
            const double* src = a.part + b0 * PART + i;
            for (int blk = 0; blk < nb; ++blk) s += src[(long)blk * PART];
        }
        tot[i] = s;
    }
    __syncthreads();

    const double len = (double)L;
    const double* const sums = tot + (Sr + 1) * NC;                // the products with the row of ones
    const double* const sqs = tot + NA * NC;
    const double qnan = __builtin_nan("");
    if (tid < MAXS * MAXS + MAXS) {
        // tid < 36: pair (estimate i, reference j); then the mixture against reference j
        const bool mix = tid >= MAXS * MAXS;
        const int i = mix ? 0 : tid / MAXS, j = mix ? tid - MAXS * MAXS : tid % MAXS;
        double val = qnan;
        if (j < Sr && (mix || i < Se)) {
            const int u = mix ? Sr : e0 + i;                       // the row of the estimate
            double g = tot[j * NC + u], ee = sqs[u], ss = sqs[j];
            if (a.zero_mean) {
                g = g - sums[j] * sums[u] / len;
                ee = ee - sums[u] * sums[u] / len;
                ss = ss - sums[j] * sums[j] / len;
            }
            val = si_sdr_of(g, ee, ss);
            if (mix && !(ss > 0.0)) atomicOr(&flag, 1);            // (an integer flag in LDS)
        }
        if (mix) {
            bs[j] = val;
            if (k == 0) a.base[(long)r * MAXS + j] = val;
        } else {
            pv[tid] = val;
            a.pair[((long)r * a.K + k) * MAXS * MAXS + tid] = val;
        }
    }
    __syncthreads();
    const int info = flag;
    if (k == 0 && tid == 0) a.info[r] = info;

    const int n = Se < Sr ? Se : Sr, big = Se < Sr ? Sr : Se;
    const int ncand = arrangements(big, n);
    // every thread: the best of its candidates tid, tid + 256, ..; a NaN value never takes the lead
    double bv = -__builtin_inf(), v0 = 0.0;
    int bi = 0x7fffffff;
    if (info == 0) {
        for (int c = tid; c < ncand; c += LANES) {
            int t[MAXS];
            unrank(c, big, n, t);
            double s = 0.0;
            for (int q = 0; q < n; ++q) s += Se >= Sr ? pv[t[q] * MAXS + q] : pv[q * MAXS + t[q]];
            if (c == 0) v0 = s;
            if (s == s && (bi == 0x7fffffff || s > bv)) { bv = s; bi = c; }
        }
    }
    cval[tid] = bv;
    cidx[tid] = bi;
    __syncthreads();
    for (int s = LANES / 2; s > 0; s >>= 1) {
        if (tid < s) {
            const double ov = cval[tid + s];
            const int oi = cidx[tid + s];
            if (oi != 0x7fffffff && (cidx[tid] == 0x7fffffff || ov > cval[tid] || (ov == cval[tid] && oi < cidx[tid]))) {
                cval[tid] = ov;
                cidx[tid] = oi;
            }
        }
        __syncthreads();
    }
    if (tid == 0) {
        // the first candidate keeps the lead if its value is NaN (nothing compares greater) and when every value is NaN
        const int best = (v0 != v0 || cidx[0] == 0x7fffffff) ? 0 : cidx[0];
        int mr[MAXS], me[MAXS];
        for (int q = 0; q < MAXS; ++q) { mr[q] = -1; me[q] = -1; }
        if (info == 0) {
            int t[MAXS];
            unrank(best, big, n, t);
            for (int q = 0; q < n; ++q) {
                if (Se >= Sr) { mr[q] = t[q]; me[t[q]] = q; }
                else { me[q] = t[q]; mr[t[q]] = q; }
            }
        }
        const long o = ((long)r * a.K + k) * MAXS;
        for (int j = 0; j < MAXS; ++j) {
            const double val = mr[j] >= 0 ? pv[mr[j] * MAXS + j] : qnan;
            a.match_ref[o + j] = mr[j];
            a.match_est[o + j] = me[j];
            a.si_sdr[o + j] = val;
            a.si_sdri[o + j] = mr[j] >= 0 ? val - bs[j] : qnan;
        }
        a.missed[(long)r * a.K + k] = info == 0 ? Sr - n : 0;
        a.spurious[(long)r * a.K + k] = info == 0 ? Se - n : 0;
    }
}

bool sisdr_domain(int R, int K, long Btot) { return R >= 1 && K >= 1 && K <= 8 && Btot >= R && Btot < (1L << 31); }

}  // namespace

extern "C" {

int ams_sisdr_abi_version(void) { return 1; }

int ams_sisdr_block(void) { return BLOCK; }

size_t ams_sisdr_workspace_bytes(int R, int K, long Btot) {
    if (!sisdr_domain(R, K, Btot)) return 0;
    return sizeof(double) * (size_t)PART * (size_t)Btot;
}

ams_status ams_sisdr_eval(const float* x, const int64_t* rows, const int64_t* rec, const int32_t* cnt, const int32_t* tab, int R, int K,
                          long Btot, int zero_mean, void* ws, size_t ws_bytes, double* pair, int32_t* match_ref, int32_t* match_est,
                          double* si_sdr, double* si_sdri, int32_t* missed, int32_t* spurious, double* base, int32_t* info,
                          void* stream) {
    AMS_REQUIRE(x && rows && rec && cnt && tab && ws && pair && match_ref && match_est && si_sdr && si_sdri && missed && spurious &&
                base && info && sisdr_domain(R, K, Btot));
    if (ws_bytes < ams_sisdr_workspace_bytes(R, K, Btot)) return AMS_E_WORKSPACE_TOO_SMALL;
    SisdrArgs a{};
    a.x = x; a.rows = (const long*)rows; a.rec = (const long*)rec; a.cnt = cnt; a.tab = tab;
    a.R = R; a.K = K; a.zero_mean = zero_mean ? 1 : 0;
    a.part = (double*)ws;
    a.pair = pair; a.match_ref = match_ref; a.match_est = match_est; a.si_sdr = si_sdr; a.si_sdri = si_sdri;
    a.missed = missed; a.spurious = spurious; a.base = base; a.info = info;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(sisdr_gram_kernel, dim3((unsigned)Btot), dim3(LANES), 0, st, a);
    ams_status s = ams_check_launch();
    if (s != AMS_OK) return s;
    hipLaunchKernelGGL(sisdr_finish_kernel, dim3((unsigned)(R * K)), dim3(LANES), 0, st, a);
    return ams_check_launch();
}

}  // extern "C"
