// Ragged BSS-eval for gfx950 (include/ams_bss_ragged.h): libams_bss_ragged.so.
//
// R recordings of any lengths x K sets of estimates in one call, no FFT.  What does not depend on a recording's length is shared with
// the batched path: the blocked f64-MFMA Cholesky and the two triangular solves over all R (1 + S) Gram matrices (chol_batched.h), the
// decomposition and the criteria (criteria.h).  What depends on the length is here, in the time domain, the unit of work (recording,
// block of AMS_BSSR_BLOCK samples) read from a host-built table:
//   bssr_corr_kernel   u(x, y)[m] = sum_t x[t] y[t + m] over one block, 256 lags per workgroup, as v_mfma_f64_16x16x4_f64 tiles:
//                      A[i][tau] = x[tau - i], B[tau][j] = y[tau + 16 j]  =>  D[i][j] = u[16 j + i]
//   bssr_csum_kernel   the block partials of a recording added in block order
//   bssr_gram_kernel / bssr_rhs_kernel   the layouts of gram_kernel / rhs_kernel of fft_path.h
//   bssr_proj_kernel   the FIR projections as the same Toeplitz product, A[i][kappa] = c[i + kappa], B[kappa][j] = x[16 j - kappa]
//                      =>  D[i][j] = P[16 j + i], and the five sums of sums_kernel in the same launch (no projection reaches memory)
//   bssr_crit_kernel   the partial rows of a recording added in block order, then the criteria of crit_kernel
// C/D lane map of the f64 MFMA as in the Cholesky: col = lane & 15, row = (lane >> 4) + 4 reg.  The B operands stride 16 samples from
// lane to lane; their LDS copies are skewed by one double per 16 (sk) so that the 16 lanes fall on different banks.
// No atomics, every sum in the order the header states: a result is a function of its recording's data only.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdlib.h>
#include "../../../include/ams_bss_ragged.h"
#include "chol_batched.h"
#include "criteria.h"

namespace {

constexpr int BLK = AMS_BSSR_BLOCK;
constexpr int MAXF = AMS_BSSR_MAX_FLEN;
constexpr int SUB = 2048;                         // samples of a block held in LDS at a time by the correlations
constexpr int CSTEPS = (SUB + 16) / 4;            // MFMA steps of a half: tau = 0 .. SUB + 15
constexpr int CW = CSTEPS / 4;                    // ... per wave (129)
constexpr int TPW = BLK / 256 / 4;                // projection tiles per wave (4)
constexpr int PXH = MAXF + 4;                     // the largest halo of the projections
constexpr int PXN = PXH + BLK + 17;
static_assert(BLK % SUB == 0 && CSTEPS % 4 == 0 && CW % 4 == 1 && TPW == 4, "the summation order of the header");

__host__ __device__ constexpr int sk(int p) { return p + (p >> 4); }

__device__ __forceinline__ d4 mfma(double a, double b, d4 c) { return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0); }

// unit u < S*S: (x, y) = (reference u / S, reference u % S);  u >= S*S: (reference q / KS, estimate row q % KS), q = u - S*S
__global__ __launch_bounds__(256) void bssr_corr_kernel(const double* __restrict__ ref, const double* __restrict__ est,
                                                        const long* __restrict__ l_off, const int* __restrict__ tab,
                                                        double* __restrict__ cpart, int S, int KS, int F) {
    __shared__ double xs[SUB + 32];               // xs[16 + v] = x[th + v], 16 zeros on either side
    __shared__ double ys[sk(SUB + 256) + 1];      // ys[sk(v)] = y[th + lag0 + v]
    __shared__ double red[4][256];
    const int row = blockIdx.x, u = blockIdx.y, lag0 = 256 * blockIdx.z;
    const int t = threadIdx.x, lane = t & 63, w = t >> 6, lr = lane & 15, lk = lane >> 4;
    const int r = tab[2 * (long)row], b = tab[2 * (long)row + 1];
    const long l0 = l_off[r], L = l_off[r + 1] - l0;
    const int NU = S * S + S * KS;
    const double* rbase = ref + (long)S * l0;
    const double *x, *y;
    if (u < S * S) {
        x = rbase + (long)(u / S) * L; y = rbase + (long)(u % S) * L;
    } else {
        const int q = u - S * S;
        x = rbase + (long)(q / KS) * L; y = est + (long)KS * l0 + (long)(q % KS) * L;
    }
    double* out = cpart + ((long)row * NU + u) * F;
    const long t0 = (long)b * BLK;
    if (t0 >= L) {                                // a block of the projections' tail: x is zero throughout
        if (lag0 + t < F) out[lag0 + t] = 0.0;
        return;
    }
    d4 a0 = {0.0, 0.0, 0.0, 0.0}, a1 = a0, a2 = a0, a3 = a0;
    for (int h = 0; h < BLK / SUB; ++h) {
        const long th = t0 + (long)h * SUB;
        if (th >= L) break;                       // (uniform; the half would add exact zeros)
        __syncthreads();
        for (int p = t; p < SUB + 32; p += 256) {
            const long tt = th + p - 16;
            xs[p] = (p >= 16 && p < 16 + SUB && tt < L) ? x[tt] : 0.0;
        }
        for (int p = t; p < SUB + 256; p += 256) {
            const long tt = th + lag0 + p;
            ys[sk(p)] = tt < L ? y[tt] : 0.0;
        }
        __syncthreads();
        const int xa = 16 + lk - lr, ya = lk + 16 * lr;
        int s = w * CW;
        for (int i = 0; i < CW - 1; i += 4, s += 4) {
            a0 = mfma(xs[xa + 4 * s], ys[sk(ya + 4 * s)], a0);
            a1 = mfma(xs[xa + 4 * s + 4], ys[sk(ya + 4 * s + 4)], a1);
            a2 = mfma(xs[xa + 4 * s + 8], ys[sk(ya + 4 * s + 8)], a2);
            a3 = mfma(xs[xa + 4 * s + 12], ys[sk(ya + 4 * s + 12)], a3);
        }
        a0 = mfma(xs[xa + 4 * s], ys[sk(ya + 4 * s)], a0);
    }
    for (int q = 0; q < 4; ++q) red[w][16 * lr + lk + 4 * q] = (a0[q] + a1[q]) + (a2[q] + a3[q]);
    __syncthreads();
    if (lag0 + t < F) out[lag0 + t] = ((red[0][t] + red[1][t]) + red[2][t]) + red[3][t];
}

// corr[r][u][m] = the partials of recording r's blocks, added in block order.  blockIdx.y = recording
__global__ void bssr_csum_kernel(const double* __restrict__ cpart, const long* __restrict__ b_off, double* __restrict__ corr, int NUF) {
    const int r = blockIdx.y;
    const long b0 = b_off[r], b1 = b_off[r + 1];
    for (int idx = blockIdx.x * blockDim.x + threadIdx.x; idx < NUF; idx += gridDim.x * blockDim.x) {
        double v = 0.0;
        for (long b = b0; b < b1; ++b) v += cpart[b * NUF + idx];
        corr[(long)r * NUF + idx] = v;
    }
}

// G block (I, J) element [a, b] = rr_IJ[b - a]: u(ref_J, ref_I)[b - a] for b >= a, u(ref_I, ref_J)[a - b] below.  Column-major, as
// gram_kernel; Gj[I] = block (I, I).  blockIdx.y = recording
__global__ void bssr_gram_kernel(const double* __restrict__ corr_, double* __restrict__ G_, double* __restrict__ Gj_, int S, int KS, int F) {
    const int N = S * F, r = blockIdx.y, NU = S * S + S * KS;
    const double* corr = corr_ + (long)r * NU * F;
    double* G = G_ + (long)r * N * N;
    double* Gj = Gj_ + (long)r * S * F * F;
    for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < (long)N * N; idx += (long)gridDim.x * blockDim.x) {
        const int row = (int)(idx / N), col = (int)(idx % N);
        const int I = row / F, a = row % F, J = col / F, b = col % F;
        const double v = b >= a ? corr[(long)(J * S + I) * F + (b - a)] : corr[(long)(I * S + J) * F + (a - b)];
        G[(long)col * N + row] = v;
        if (I == J) Gj[(long)I * F * F + (long)b * F + a] = v;
    }
}

// Df[r][e][i*F + k] = Dj[r][i][e][k] = u(ref_i, est_e)[k], as rhs_kernel.  blockIdx.y = recording
__global__ void bssr_rhs_kernel(const double* __restrict__ corr_, double* __restrict__ Df_, double* __restrict__ Dj_, int S, int KS, int F) {
    const int N = S * F, r = blockIdx.y, NU = S * S + S * KS;
    const double* corr = corr_ + (long)r * NU * F;
    double* Df = Df_ + (long)r * KS * N;
    double* Dj = Dj_ + (long)r * KS * N;
    for (int idx = blockIdx.x * blockDim.x + threadIdx.x; idx < KS * N; idx += gridDim.x * blockDim.x) {
        const int e = idx / N, q = idx % N, i = q / F, k = q % F;
        const double v = corr[(long)(S * S + i * KS + e) * F + k];
        Df[(long)e * N + q] = v;
        Dj[((long)i * KS + e) * F + k] = v;
    }
}

// One (recording, block) x estimate row e: P_f(e) over the block (kept in registers, 4 tiles of 256 outputs per wave), then for every
// j the projection P_j(e) and the five sums.  part[row][e][j][5]
__global__ __launch_bounds__(256) void bssr_proj_kernel(const double* __restrict__ ref, const double* __restrict__ est,
                                                        const long* __restrict__ l_off, const int* __restrict__ tab,
                                                        const double* __restrict__ Cf, const double* __restrict__ Cj,
                                                        double* __restrict__ part, int S, int KS, int F) {
    __shared__ double xs[sk(PXN) + 1];            // xs[sk(p)] = x[Tb - XH + p], p = 0 .. XH + BLK + 16
    __shared__ double cs[MAXF + 64];              // cs[p] = c[p - 16], zero outside 0 .. F - 1
    __shared__ double sm[4];
    const int row = blockIdx.x, e = blockIdx.y;
    const int t = threadIdx.x, lane = t & 63, w = t >> 6, lr = lane & 15, lk = lane >> 4;
    const int r = tab[2 * (long)row], b = tab[2 * (long)row + 1];
    const long l0 = l_off[r], L = l_off[r + 1] - l0, Lp = L + F - 1, Tb = (long)b * BLK;
    const int N = S * F;
    const int nsteps = (F + 16 + 3) / 4;          // kappa = -16 + 4 step + (0 .. 3)
    const int XH = 4 * nsteps - 16;               // F .. F + 3: the halo in front of the block
    const double* rbase = ref + (long)S * l0;
    const double* er = est + (long)KS * l0 + (long)e * L;
    const double* Cfr = Cf + (long)r * KS * N + (long)e * N;
    const double* Cjr = Cj + (long)r * KS * N;
    const int ca = lr + lk;                                           // cs index at step 0
    const int xb = 256 * w + XH + 16 + 16 * lr - lk;                  // xs index (unskewed) of tile w at step 0

    auto stage = [&](const double* x, const double* c) {
        __syncthreads();
        for (int p = t; p < XH + BLK + 17; p += 256) {
            const long tt = Tb - XH + p;
            xs[sk(p)] = (tt >= 0 && tt < L) ? x[tt] : 0.0;
        }
        for (int p = t; p < 4 * nsteps + 16; p += 256) cs[p] = (p >= 16 && p < 16 + F) ? c[p - 16] : 0.0;
        __syncthreads();
    };

    d4 pf[TPW];
#pragma unroll
    for (int tl = 0; tl < TPW; ++tl) pf[tl] = d4{0.0, 0.0, 0.0, 0.0};
    for (int i = 0; i < S; ++i) {                                     // i ascending, as prod_kernel
        stage(rbase + (long)i * L, Cfr + (long)i * F);
        for (int s = 0; s < nsteps; ++s) {
            const double a = cs[ca + 4 * s];
#pragma unroll
            for (int tl = 0; tl < TPW; ++tl) pf[tl] = mfma(a, xs[sk(xb + 1024 * tl - 4 * s)], pf[tl]);
        }
    }
    for (int j = 0; j < S; ++j) {
        stage(rbase + (long)j * L, Cjr + ((long)j * KS + e) * F);
        d4 pj[TPW];
#pragma unroll
        for (int tl = 0; tl < TPW; ++tl) pj[tl] = d4{0.0, 0.0, 0.0, 0.0};
        for (int s = 0; s < nsteps; ++s) {
            const double a = cs[ca + 4 * s];
#pragma unroll
            for (int tl = 0; tl < TPW; ++tl) pj[tl] = mfma(a, xs[sk(xb + 1024 * tl - 4 * s)], pj[tl]);
        }
        double s0 = 0, s1 = 0, s2 = 0, s3 = 0, s4 = 0;
#pragma unroll
        for (int tl = 0; tl < TPW; ++tl)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int o = 256 * (w + 4 * tl) + 16 * lr + lk + 4 * q;      // output D[lk + 4 q][lr] of the tile
                const long tt = Tb + o;
                if (tt < Lp) {
                    const double s_true = xs[sk(XH + o)];
                    const double ev = tt < L ? er[tt] : 0.0;
                    decompose_add(s_true, pj[tl][q], pf[tl][q], ev, s0, s1, s2, s3, s4);
                }
            }
        double* out = part + (((long)row * KS + e) * S + j) * 5;
        double v;
        v = block_sum(s0, sm); if (t == 0) out[0] = v;
        v = block_sum(s1, sm); if (t == 0) out[1] = v;
        v = block_sum(s2, sm); if (t == 0) out[2] = v;
        v = block_sum(s3, sm); if (t == 0) out[3] = v;
        v = block_sum(s4, sm); if (t == 0) out[4] = v;
    }
}

// blockIdx.x = e * S + j, blockIdx.y = recording.  crit[r][k][c][e][j]; NaN when a factorisation of THIS recording failed
__global__ void bssr_crit_kernel(const double* __restrict__ part, const long* __restrict__ b_off, const int* __restrict__ info_f,
                                 const int* __restrict__ info_j, double* __restrict__ crit, int* __restrict__ info_out, int S, int KS) {
    const int pair = blockIdx.x, r = blockIdx.y;
    if (threadIdx.x != 0) return;
    int bad = info_f[r] != 0;
    for (int i = 0; i < S; ++i) bad |= (info_j[(long)r * S + i] != 0);
    double s[5] = {0, 0, 0, 0, 0};
    for (long b = b_off[r]; b < b_off[r + 1]; ++b)
        for (int k = 0; k < 5; ++k) s[k] += part[((b * KS * S) + pair) * 5 + k];
    const int set = pair / (S * S), ej = pair % (S * S), K = KS / S;
    criteria_store(s, bad, crit + ((long)r * K + set) * 3 * S * S, S * S, ej);
    if (pair == 0) info_out[r] = bad;
}

bool bssr_domain(int S, int K, int F) { return S >= 1 && S <= 6 && K >= 1 && K <= 64 && F >= 1 && F <= MAXF; }

struct bssr_layout {
    size_t G, Gj, Df, Dj, corr, cpart, part, info, total;
};

bssr_layout bssr_offsets(int R, int K, int S, int F, long Btot) {
    const size_t d = sizeof(double), r = (size_t)R, N = (size_t)S * F, KS = (size_t)K * S, NU = (size_t)S * S + S * KS, bt = (size_t)Btot;
    bssr_layout l;
    size_t o = 0;
    l.G = o;      o = align256(o + r * N * N * d);
    l.Gj = o;     o = align256(o + r * S * F * F * d);
    l.Df = o;     o = align256(o + r * KS * N * d);
    l.Dj = o;     o = align256(o + r * KS * N * d);
    l.corr = o;   o = align256(o + r * NU * F * d);
    l.cpart = o;  o = align256(o + bt * NU * F * d);
    l.part = o;   o = align256(o + bt * KS * S * 5 * d);
    l.info = o;   o = align256(o + r * (1 + S) * sizeof(int));
    l.total = o;
    return l;
}

}  // namespace

extern "C" {

int ams_bssr_abi_version(void) { return 1; }
int ams_bssr_block(void) { return BLK; }

long ams_bssr_blocks(const int64_t* l_off, int R, int flen) {
    if (!l_off || R < 1 || R > MAXGRID || flen < 1 || flen > MAXF || l_off[0] != 0) return -1;
    long B = 0;
    for (int r = 0; r < R; ++r) {
        const long L = l_off[r + 1] - l_off[r];
        if (L < 1) return -1;
        B += (L + flen - 1 + BLK - 1) / BLK;
        if (B > 2147483647L) return -1;
    }
    return B;
}

int ams_bssr_tables(const int64_t* l_off, int R, int flen, int64_t* b_off, int32_t* tab) {
    if (!b_off || !tab || ams_bssr_blocks(l_off, R, flen) < 0) return -1;
    long B = 0;
    for (int r = 0; r < R; ++r) {
        b_off[r] = B;
        const long Br = (l_off[r + 1] - l_off[r] + flen - 1 + BLK - 1) / BLK;
        for (long b = 0; b < Br; ++b) {
            tab[2 * (B + b)] = r;
            tab[2 * (B + b) + 1] = (int32_t)b;
        }
        B += Br;
    }
    b_off[R] = B;
    return 0;
}

int ams_bssr_launches(int nsrc, int nsets, int flen) {
    if (!bssr_domain(nsrc, nsets, flen)) return -1;
    return 4 + potrf_launches(nsrc * flen) + potrf_launches(flen) + 4 + 2;
}

size_t ams_bssr_workspace_bytes(int R, int nsets, int nsrc, int flen, long Btot) {
    if (!bssr_domain(nsrc, nsets, flen) || R < 1 || R > MAXGRID || Btot < R || Btot > 2147483647L) return 0;
    return bssr_offsets(R, nsets, nsrc, flen, Btot).total;
}

int ams_bssr_eval(const double* ref, const double* est, const int64_t* l_off, const int64_t* b_off, const int32_t* tab, int R, int nsets,
                  int nsrc, int flen, long Btot, double* crit, int* info, void* ws, size_t ws_bytes, void* stream) {
    if (!ref || !est || !l_off || !b_off || !tab || !crit || !info || !ws || ((size_t)ws & 7)) return -1;
    if (!bssr_domain(nsrc, nsets, flen) || R < 1 || R > MAXGRID || Btot < R || Btot > 2147483647L) return -1;
    const int S = nsrc, K = nsets, F = flen, KS = K * S, N = S * F, NU = S * S + S * KS;
    const bssr_layout l = bssr_offsets(R, K, S, F, Btot);
    if (ws_bytes < l.total) return -2;
    hipStream_t st = (hipStream_t)stream;
    char* w = (char*)ws;
    double* G = (double*)(w + l.G);
    double* Gj = (double*)(w + l.Gj);
    double* Df = (double*)(w + l.Df);
    double* Dj = (double*)(w + l.Dj);
    double* corr = (double*)(w + l.corr);
    double* cpart = (double*)(w + l.cpart);
    double* part = (double*)(w + l.part);
    int* info_f = (int*)(w + l.info);
    int* info_j = info_f + R;
    const long* lo = (const long*)l_off;
    const long* bo = (const long*)b_off;

    hipLaunchKernelGGL(bssr_corr_kernel, dim3((unsigned)Btot, NU, (F + 255) / 256), dim3(256), 0, st, ref, est, lo, tab, cpart, S, KS, F);
    hipLaunchKernelGGL(bssr_csum_kernel, dim3((NU * F + 255) / 256, R), dim3(256), 0, st, cpart, bo, corr, NU * F);
    const long nn = (long)N * N;
    hipLaunchKernelGGL(bssr_gram_kernel, dim3((unsigned)(nn + 255 < 1024 * 256 ? (nn + 255) / 256 : 1024), R), dim3(256), 0, st, corr, G,
                       Gj, S, KS, F);
    hipLaunchKernelGGL(bssr_rhs_kernel, dim3((KS * N + 255) / 256 < 16 ? (KS * N + 255) / 256 : 16, R), dim3(256), 0, st, corr, Df, Dj, S,
                       KS, F);
    // factorise every Gram matrix once, then solve with all estimates of all sets as right-hand sides (as ams_bssb_eval)
    const int pf = potrf_batched(G, N, N, nn, R, info_f, st);
    if (pf < 0) return -3;
    const int pj = potrf_batched(Gj, F, F, (long)F * F, R * S, info_j, st);
    if (pj < 0) return -3;
    const int sf = solve_batched(G, N, N, nn, Df, N, (long)KS * N, KS, R, st);
    const int sj = solve_batched(Gj, F, F, (long)F * F, Dj, F, (long)KS * F, KS, R * S, st);
    hipLaunchKernelGGL(bssr_proj_kernel, dim3((unsigned)Btot, KS), dim3(256), 0, st, ref, est, lo, tab, Df, Dj, part, S, KS, F);
    hipLaunchKernelGGL(bssr_crit_kernel, dim3(KS * S, R), dim3(64), 0, st, part, bo, info_f, info_j, crit, info, S, KS);
    if (hipGetLastError() != hipSuccess) return -3;
    // the header's promise: this call's six launches and what the shared code reports are what ams_bssr_launches states
    return 4 + pf + pj + sf + sj + 2 == ams_bssr_launches(S, K, F) ? 0 : -3;
}

}  // extern "C"
