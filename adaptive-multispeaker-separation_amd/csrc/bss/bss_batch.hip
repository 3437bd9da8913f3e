// Batched BSS-eval for gfx950 (include/ams_bss_batch.h): nutt utterances x nsets sets of estimates in one call.
//
// Same arithmetic as bss_eval.hip, one more index.  Per call:
//   1. ONE batched real FFT of all references and all estimates of all sets;
//   2. cross-spectra -> ONE batched inverse FFT -> the auto/cross-correlations (the reference pairs once per utterance,
//      reference x estimate for every set);
//   3. per utterance ONE (nsrc*flen)^2 Gram matrix and its nsrc diagonal blocks (same block overwrite order as bss_eval.hip);
//   4. all nutt*(1+nsrc) matrices factorised by this file's batched blocked Cholesky (below), then two batched triangular
//      solves with the nsets*nsrc estimates of the utterance as right-hand sides;
//   5. the filters applied by spectral multiplication, the same two-stage float64 sums, the same criteria.
//
// Batched Cholesky (right-looking, lower, column-major, panel width NB = 32), three launches per block column, the grid of
// each spanning matrices x tiles, ordinary stream order between them:
//   potrf_diag   one workgroup per matrix: the NB x NB diagonal block factorised in LDS (unblocked, column by column);
//   potrf_panel  one workgroup per 64 rows below it: inverts the diagonal factor in LDS (each workgroup its own copy -- no
//                workspace, no cross-workgroup traffic) and forms  panel <- panel * inv(L_kk)^T  with v_mfma_f64_16x16x4_f64;
//   potrf_trail  one workgroup per 64 x 64 tile of the lower trailing matrix:  C_ij -= P_i * P_j^T  with the same instruction.
// Both products are computed TRANSPOSED (D' = B * A^T), because the f64 MFMA's C/D map is col = lane & 15,
// row = (lane >> 4) + 4 * reg: with the matrix row on `col`, 16 lanes touch 16 consecutive doubles of a column.
// A non-positive (or NaN) pivot sets info[m] once and writes NaN as the pivot; the NaN spreads through that matrix only.
// No atomics, no persistent grid, every sum in a fixed order: a factor is a function of its matrix alone.
//
// Compiled a second time by bss_ragged.hip with AMS_BSS_RAGGED (libams_bss_ragged.so): that build keeps the Cholesky, the triangular
// solves and block_sum and leaves out the exported entry points, the context and every use of hipFFT.  AMS_BSS_LAUNCH is
// hipLaunchKernelGGL unless the including file counts its launches.
#include <hip/hip_runtime.h>
#ifndef AMS_BSS_RAGGED
#include <hipfft/hipfft.h>
#endif
#include <math.h>
#include <stdlib.h>
#ifndef AMS_BSS_RAGGED
#include "../../../include/ams_bss_batch.h"
#endif
#ifndef AMS_BSS_LAUNCH
#define AMS_BSS_LAUNCH hipLaunchKernelGGL
#endif

namespace {

constexpr int RB = 256;            // blocks per (set, e, j) triple in the first reduction stage (as bss_eval.hip)
constexpr int NB = 32;             // Cholesky panel width
constexpr int TM = 64;             // rows / columns of a panel or trailing tile
constexpr int TS = 64;             // rows per step of the triangular solves
constexpr int RC = 4;              // right-hand sides per workgroup of the triangular solves
constexpr int MAXGRID = 65535;

typedef double d4 __attribute__((ext_vector_type(4)));

#ifndef AMS_BSS_RAGGED
struct plan_set {
    int nutt;                      // 0: not planned
    hipfftHandle fwd_in, inv_corr, fwd_c, inv_proj;
};
#endif

}  // namespace

#ifndef AMS_BSS_RAGGED
struct ams_bssb_ctx {
    int U, K, S, L, F, n, nc, Lp, NP, KS;
    plan_set full, part;           // plans for nutt == max_utt, and for the last other nutt asked for
    size_t ws_bytes;
    // offsets (in bytes) into the caller's workspace; `a` holds xs, then cpad, then pspec; `b` holds corr, then cspec, then proj
    size_t o_tpad, o_spec, o_a, o_b, o_G, o_Gj, o_Df, o_Dj, o_part, o_info;
};
#endif

namespace {

#ifndef AMS_BSS_RAGGED
// ---------------------------------------------------------------- assembly and reduction kernels, blockIdx.z = utterance
// rows of an utterance: [0, S) references, [S, S + K*S) estimates (set-major)
__global__ void pad_kernel(const double* __restrict__ ref, const double* __restrict__ est, double* __restrict__ tpad, int S, int KS,
                           int L, int n) {
    const int r = blockIdx.y, u = blockIdx.z;
    const double* src = r < S ? ref + ((long)u * S + r) * L : est + ((long)u * KS + (r - S)) * L;
    double* dst = tpad + ((long)u * (S + KS) + r) * n;
    for (int t = blockIdx.x * blockDim.x + threadIdx.x; t < n; t += gridDim.x * blockDim.x) dst[t] = t < L ? src[t] : 0.0;
}

// pair p < S(S+1)/2: references (i >= j), row-major over i then j;  p >= that: (reference i, estimate row ke)
__device__ __forceinline__ void pair_of(int p, int S, int KS, int& a, int& b) {
    const int nrr = S * (S + 1) / 2;
    if (p < nrr) {
        int i = 0;
        while ((i + 1) * (i + 2) / 2 <= p) ++i;
        a = i; b = p - i * (i + 1) / 2;
    } else {
        const int q = p - nrr;
        a = q / KS; b = S + q % KS;
    }
}
__global__ void cross_kernel(const hipfftDoubleComplex* __restrict__ spec, hipfftDoubleComplex* __restrict__ xs, int S, int KS, int NP,
                             int nc) {
    int a, b;
    pair_of(blockIdx.y, S, KS, a, b);
    const int u = blockIdx.z;
    const hipfftDoubleComplex* sp = spec + (long)u * (S + KS) * nc;
    hipfftDoubleComplex* out = xs + ((long)u * NP + blockIdx.y) * nc;
    for (int k = blockIdx.x * blockDim.x + threadIdx.x; k < nc; k += gridDim.x * blockDim.x) {
        const hipfftDoubleComplex x = sp[(long)a * nc + k], v = sp[(long)b * nc + k];
        out[k] = make_hipDoubleComplex(x.x * v.x + x.y * v.y, x.y * v.x - x.x * v.y);      // x * conj(v)
    }
}

__device__ __forceinline__ int rr_index(int i, int j) { return i * (i + 1) / 2 + j; }      // i >= j

// as gram_kernel of bss_eval.hip; blockIdx.y = utterance
__global__ void gram_kernel(const double* __restrict__ corr_, double* __restrict__ G_, double* __restrict__ Gj_, int S, int F, int n,
                            int NP) {
    const int N = S * F, u = blockIdx.y;
    const double* corr = corr_ + (long)u * NP * n;
    double* G = G_ + (long)u * N * N;
    double* Gj = Gj_ + (long)u * S * F * F;
    const double sc = 1.0 / n;
    for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < (long)N * N; idx += (long)gridDim.x * blockDim.x) {
        const int row = (int)(idx / N), col = (int)(idx % N);
        const int I = row / F, a = row % F, J = col / F, b = col % F;
        double v;
        if (I > J) v = corr[(long)rr_index(I, J) * n + ((b - a) % n + n) % n];
        else if (I < J) v = corr[(long)rr_index(J, I) * n + ((a - b) % n + n) % n];
        else v = corr[(long)rr_index(I, I) * n + ((a - b) % n + n) % n];
        v *= sc;
        G[(long)col * N + row] = v;
        if (I == J) Gj[(long)I * F * F + (long)b * F + a] = v;
    }
}

// Df[u][ke][i*F + k] = Dj[u][i][ke][k] = corr_(i,ke)[(n - k) mod n] / n
__global__ void rhs_kernel(const double* __restrict__ corr_, double* __restrict__ Df_, double* __restrict__ Dj_, int S, int KS, int F,
                           int n, int NP) {
    const int nrr = S * (S + 1) / 2, N = S * F, u = blockIdx.y;
    const double* corr = corr_ + (long)u * NP * n;
    double* Df = Df_ + (long)u * KS * N;
    double* Dj = Dj_ + (long)u * KS * N;
    const double sc = 1.0 / n;
    for (int idx = blockIdx.x * blockDim.x + threadIdx.x; idx < KS * N; idx += gridDim.x * blockDim.x) {
        const int e = idx / N, r = idx % N, i = r / F, k = r % F;
        const double v = corr[(long)(nrr + i * KS + e) * n + (n - k) % n] * sc;
        Df[(long)e * N + r] = v;
        Dj[((long)i * KS + e) * F + k] = v;
    }
}

// filters, zero padded: rows [0, KS*S): (full, ke, i);  rows [KS*S, 2*KS*S): (single, j, ke)
__global__ void cpad_kernel(const double* __restrict__ Cf_, const double* __restrict__ Cj_, double* __restrict__ cpad, int S, int KS,
                            int F, int n) {
    const int r = blockIdx.y, u = blockIdx.z, N = S * F;
    const double* src = r < KS * S ? Cf_ + (long)u * KS * N + (long)r * F : Cj_ + (long)u * KS * N + (long)(r - KS * S) * F;
    double* dst = cpad + ((long)u * 2 * KS * S + r) * n;
    for (int t = blockIdx.x * blockDim.x + threadIdx.x; t < n; t += gridDim.x * blockDim.x) dst[t] = t < F ? src[t] : 0.0;
}

__device__ __forceinline__ hipfftDoubleComplex cmul(hipfftDoubleComplex u, hipfftDoubleComplex v) {
    return make_hipDoubleComplex(u.x * v.x - u.y * v.y, u.x * v.y + u.y * v.x);
}
// rows [0, KS): projection of estimate ke on ALL references;  rows [KS, KS + S*KS): (single reference j, estimate ke)
__global__ void prod_kernel(const hipfftDoubleComplex* __restrict__ spec_, const hipfftDoubleComplex* __restrict__ cspec_,
                            hipfftDoubleComplex* __restrict__ pspec_, int S, int KS, int nc) {
    const int r = blockIdx.y, u = blockIdx.z;
    const hipfftDoubleComplex* spec = spec_ + (long)u * (S + KS) * nc;
    const hipfftDoubleComplex* cspec = cspec_ + (long)u * 2 * KS * S * nc;
    hipfftDoubleComplex* pspec = pspec_ + ((long)u * (KS + S * KS) + r) * nc;
    for (int k = blockIdx.x * blockDim.x + threadIdx.x; k < nc; k += gridDim.x * blockDim.x) {
        hipfftDoubleComplex acc = make_hipDoubleComplex(0.0, 0.0);
        if (r < KS) {
            for (int i = 0; i < S; ++i) {                                  // i ascending, as bss_eval.hip
                const hipfftDoubleComplex t = cmul(cspec[(long)(r * S + i) * nc + k], spec[(long)i * nc + k]);
                acc.x += t.x; acc.y += t.y;
            }
        } else {
            const int q = r - KS, j = q / KS;
            acc = cmul(cspec[(long)(KS * S + q) * nc + k], spec[(long)j * nc + k]);
        }
        pspec[k] = acc;
    }
}
#endif

__device__ __forceinline__ double block_sum(double v, double* sm) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) sm[w] = v;
    __syncthreads();
    double t = 0.0;
    if (threadIdx.x == 0) for (int i = 0; i < (int)(blockDim.x >> 6); ++i) t += sm[i];
    __syncthreads();
    return t;
}

#ifndef AMS_BSS_RAGGED
// as sums_kernel of bss_eval.hip; blockIdx.y = ke * S + j, blockIdx.z = utterance
__global__ __launch_bounds__(256) void sums_kernel(const double* __restrict__ tpad_, const double* __restrict__ proj_,
                                                   double* __restrict__ part_, int S, int KS, int n, int Lp) {
    __shared__ double sm[4];
    const int pair = blockIdx.y, ke = pair / S, j = pair % S, u = blockIdx.z;
    const double sc = 1.0 / n;
    const double* tpad = tpad_ + (long)u * (S + KS) * n;
    const double* proj = proj_ + (long)u * (KS + S * KS) * n;
    const double* ref = tpad + (long)j * n;
    const double* est = tpad + (long)(S + ke) * n;
    const double* pf = proj + (long)ke * n;
    const double* pj = proj + (long)(KS + j * KS + ke) * n;
    double a0 = 0, a1 = 0, a2 = 0, a3 = 0, a4 = 0;
    for (int t = blockIdx.x * blockDim.x + threadIdx.x; t < Lp; t += gridDim.x * blockDim.x) {
        const double s_true = ref[t];
        const double e_spat = pj[t] * sc - s_true;
        const double e_interf = pf[t] * sc - s_true - e_spat;
        const double e_artif = -s_true - e_spat - e_interf + est[t];
        const double s_filt = s_true + e_spat;
        a0 += s_filt * s_filt;
        a1 += (e_interf + e_artif) * (e_interf + e_artif);
        a2 += e_interf * e_interf;
        a3 += (s_filt + e_interf) * (s_filt + e_interf);
        a4 += e_artif * e_artif;
    }
    double* out = part_ + ((((long)u * KS * S) + pair) * RB + blockIdx.x) * 5;
    double v;
    v = block_sum(a0, sm); if (threadIdx.x == 0) out[0] = v;
    v = block_sum(a1, sm); if (threadIdx.x == 0) out[1] = v;
    v = block_sum(a2, sm); if (threadIdx.x == 0) out[2] = v;
    v = block_sum(a3, sm); if (threadIdx.x == 0) out[3] = v;
    v = block_sum(a4, sm); if (threadIdx.x == 0) out[4] = v;
}

// stage 2 + criteria.  blockIdx.x = ke * S + j, blockIdx.y = utterance.  crit[u][k][c][e][j]; NaN when a factorisation of
// THIS utterance failed (info_f[u], info_j[u*S ..]).
__global__ void crit_kernel(const double* __restrict__ part_, const int* __restrict__ info_f, const int* __restrict__ info_j,
                            double* __restrict__ crit, int* __restrict__ info_out, int S, int KS) {
    const int pair = blockIdx.x, u = blockIdx.y;
    if (threadIdx.x != 0) return;
    int bad = info_f[u] != 0;
    for (int i = 0; i < S; ++i) bad |= (info_j[u * S + i] != 0);
    const double* part = part_ + (((long)u * KS * S) + pair) * RB * 5;
    double s[5] = {0, 0, 0, 0, 0};
    for (int b = 0; b < RB; ++b)
        for (int k = 0; k < 5; ++k) s[k] += part[(long)b * 5 + k];
    const double nanv = nan("");
    const int set = pair / (S * S), ej = pair % (S * S), K = KS / S;
    double* out = crit + ((long)u * K + set) * 3 * S * S;
    out[0 * S * S + ej] = bad ? nanv : 10.0 * log10(s[0] / (s[1] + 1e-12));
    out[1 * S * S + ej] = bad ? nanv : 10.0 * log10(s[0] / (s[2] + 1e-12));
    out[2 * S * S + ej] = bad ? nanv : 10.0 * log10(s[3] / (s[4] + 1e-12));
    if (pair == 0) info_out[u] = bad;
}
#endif

// ---------------------------------------------------------------- batched blocked Cholesky
// Diagonal block [k0, k0 + nb) of every matrix, in LDS.  s[col][row]; a short last block is padded with the identity.
__global__ __launch_bounds__(256) void potrf_diag_kernel(double* __restrict__ A, int n, int lda, long stride, int nmat, int k0,
                                                         int* __restrict__ info) {
    __shared__ double s[NB][NB + 1];
    const int t = threadIdx.x, i = t & 31, g = t >> 5;
    const int nb = min(NB, n - k0);
    for (int m = blockIdx.x; m < nmat; m += gridDim.x) {
        double* Am = A + (long)m * stride + (long)k0 * lda + k0;
        for (int c = g; c < NB; c += 8) s[c][i] = (i < nb && c < nb && i >= c) ? Am[(long)c * lda + i] : (i == c ? 1.0 : 0.0);
        __syncthreads();
        for (int j = 0; j < nb; ++j) {
            const double d = s[j][j];
            const double piv = d > 0.0 ? sqrt(d) : nan("");
            if (t == 0 && !(d > 0.0) && info[m] == 0) info[m] = k0 + j + 1;
            __syncthreads();                                               // s[j][j] read by all before it is replaced
            if (g == 0 && i >= j) s[j][i] = (i == j) ? piv : s[j][i] / piv;
            __syncthreads();
            for (int c = j + 1 + g; c <= i; c += 8) s[c][i] -= s[j][i] * s[j][c];
            __syncthreads();
        }
        for (int c = g; c < NB; c += 8)
            if (i < nb && c < nb && i >= c) Am[(long)c * lda + i] = s[c][i];
        __syncthreads();
    }
}

// Rows [r0 + 64 * blockIdx.x, +64) of the panel below the diagonal block, r0 = k0 + NB:  X = P * inv(L_kk)^T.
__global__ __launch_bounds__(256) void potrf_panel_kernel(double* __restrict__ A, int n, int lda, long stride, int nmat, int k0) {
    __shared__ double sL[NB][NB + 1];      // sL[col][row] = L_kk[row][col]
    __shared__ double sI[NB][NB + 1];      // sI[p][c] = inv(L_kk)[c][p]
    __shared__ double sP[NB][TM + 1];      // sP[p][r] = P[r][p]
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int row0 = k0 + NB + TM * blockIdx.x;
    for (int m = blockIdx.y; m < nmat; m += gridDim.y) {
        double* Am = A + (long)m * stride;
        {
            const int i = t & 31, g = t >> 5;
            for (int c = g; c < NB; c += 8) {
                sL[c][i] = i >= c ? Am[(long)(k0 + c) * lda + k0 + i] : 0.0;          // k0 + NB < n here: a full block
                sI[c][i] = 0.0;
            }
            const int r = t & 63, g4 = t >> 6;
            for (int p = g4; p < NB; p += 4) sP[p][r] = row0 + r < n ? Am[(long)(k0 + p) * lda + row0 + r] : 0.0;
        }
        __syncthreads();
        if (t < NB) {                                                      // column t of the inverse: L x = e_t
            const int c = t;
            sI[c][c] = 1.0 / sL[c][c];
            for (int i = c + 1; i < NB; ++i) {
                double acc = 0.0;
                for (int p = c; p < i; ++p) acc += sL[p][i] * sI[c][p];
                sI[c][i] = -acc / sL[i][i];
            }
        }
        __syncthreads();
        // here sI[c][i] = inv[i][c]; the product wants a[cc][p] = inv[cc][p] = sI[p][cc]
        const int lr = lane & 15, lk = lane >> 4;
        for (int cb = 0; cb < NB / 16; ++cb) {
            d4 acc = {0.0, 0.0, 0.0, 0.0};
            for (int ks = 0; ks < NB / 4; ++ks) {
                const double a = sI[4 * ks + lk][16 * cb + lr];
                const double b = sP[4 * ks + lk][16 * w + lr];
                acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc, 0, 0, 0);
            }
            const int row = row0 + 16 * w + lr;
            if (row < n)
                for (int q = 0; q < 4; ++q) Am[(long)(k0 + 16 * cb + lk + 4 * q) * lda + row] = acc[q];
        }
        __syncthreads();
    }
}

// Tile (blockIdx.x >= blockIdx.y) of the lower trailing matrix:  C -= P_i * P_j^T.
__global__ __launch_bounds__(256) void potrf_trail_kernel(double* __restrict__ A, int n, int lda, long stride, int nmat, int k0) {
    __shared__ double sPi[NB][TM + 1];
    __shared__ double sPj[NB][TM + 1];
    const int ti = blockIdx.x, tj = blockIdx.y;
    if (tj > ti) return;
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int I0 = k0 + NB + TM * ti, J0 = k0 + NB + TM * tj;
    const int lr = lane & 15, lk = lane >> 4;
    for (int m = blockIdx.z; m < nmat; m += gridDim.z) {
        double* Am = A + (long)m * stride;
        {
            const int r = t & 63, g4 = t >> 6;
            for (int p = g4; p < NB; p += 4) {
                sPi[p][r] = I0 + r < n ? Am[(long)(k0 + p) * lda + I0 + r] : 0.0;
                sPj[p][r] = J0 + r < n ? Am[(long)(k0 + p) * lda + J0 + r] : 0.0;
            }
        }
        __syncthreads();
        const int row = I0 + 16 * w + lr;
        for (int jb = 0; jb < TM / 16; ++jb) {
            if (ti == tj && jb > w) break;                                 // wholly above the diagonal
            d4 acc;
            for (int q = 0; q < 4; ++q) {
                const int col = J0 + 16 * jb + lk + 4 * q;
                acc[q] = (row < n && col <= row) ? Am[(long)col * lda + row] : 0.0;
            }
            for (int ks = 0; ks < NB / 4; ++ks) {
                const double a = -sPj[4 * ks + lk][16 * jb + lr];
                const double b = sPi[4 * ks + lk][16 * w + lr];
                acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc, 0, 0, 0);
            }
            for (int q = 0; q < 4; ++q) {
                const int col = J0 + 16 * jb + lk + 4 * q;
                if (row < n && col <= row) Am[(long)col * lda + row] = acc[q];
            }
        }
        __syncthreads();
    }
}

int potrf_batched(double* A, int n, int lda, long stride, int nmat, int* info, hipStream_t st) {
    if (hipMemsetAsync(info, 0, (size_t)nmat * sizeof(int), st) != hipSuccess) return -3;
    const int gm = nmat < MAXGRID ? nmat : MAXGRID;
    for (int k0 = 0; k0 < n; k0 += NB) {
        AMS_BSS_LAUNCH(potrf_diag_kernel, dim3(gm), dim3(256), 0, st, A, n, lda, stride, nmat, k0, info);
        const int rem = n - k0 - NB;
        if (rem <= 0) break;
        const int T = (rem + TM - 1) / TM;
        AMS_BSS_LAUNCH(potrf_panel_kernel, dim3(T, gm), dim3(256), 0, st, A, n, lda, stride, nmat, k0);
        AMS_BSS_LAUNCH(potrf_trail_kernel, dim3(T, T, gm), dim3(256), 0, st, A, n, lda, stride, nmat, k0);
    }
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

// ---------------------------------------------------------------- batched triangular solves, L L^T x = b in place
// One workgroup per (matrix, group of RC right-hand sides); right-hand side r of matrix m at B + m * strideB + r * ldb.
// The factor is read once per solve; the solved part of x is read back from global memory (written by this workgroup).
__global__ __launch_bounds__(256) void solve_fwd_kernel(const double* __restrict__ Lf, int n, int lda, long strideL, double* B, int ldb,
                                                        long strideB, int R, int nmat) {
    __shared__ double sL[TS][TS + 1];      // sL[col][row]
    __shared__ double sacc[4][RC][TS];
    __shared__ double sx[RC][TS];
    const int t = threadIdx.x, row = t & 63, g = t >> 6;
    const int rbase = blockIdx.x * RC, nr = min(RC, R - rbase);
    for (int m = blockIdx.y; m < nmat; m += gridDim.y) {
        const double* Lm = Lf + (long)m * strideL;
        double* Bm = B + (long)m * strideB + (long)rbase * ldb;
        for (int i0 = 0; i0 < n; i0 += TS) {
            const int nb = min(TS, n - i0);
            double acc[RC];
            for (int r = 0; r < RC; ++r) acc[r] = 0.0;
            if (row < nb)
                for (int c = g; c < i0; c += 4) {
                    const double l = Lm[(long)c * lda + i0 + row];
                    for (int r = 0; r < RC; ++r)
                        if (r < nr) acc[r] += l * Bm[(long)r * ldb + c];
                }
            for (int r = 0; r < RC; ++r) sacc[g][r][row] = acc[r];
            for (int c = g; c < TS; c += 4) sL[c][row] = (row < nb && c < nb && row >= c) ? Lm[(long)(i0 + c) * lda + i0 + row] : (row == c ? 1.0 : 0.0);
            __syncthreads();
            // thread (row, r = g)
            double v = 0.0;
            const bool on = row < nb && g < nr;
            if (on) v = Bm[(long)g * ldb + i0 + row] - (((sacc[0][g][row] + sacc[1][g][row]) + sacc[2][g][row]) + sacc[3][g][row]);
            for (int j = 0; j < nb; ++j) {
                if (row == j) { v = v / sL[j][j]; sx[g][j] = v; }
                __syncthreads();
                if (row > j) v -= sL[j][row] * sx[g][j];
            }
            if (on) Bm[(long)g * ldb + i0 + row] = v;
            __syncthreads();
        }
    }
}

__global__ __launch_bounds__(256) void solve_bwd_kernel(const double* __restrict__ Lf, int n, int lda, long strideL, double* B, int ldb,
                                                        long strideB, int R, int nmat) {
    __shared__ double sL[TS][TS + 1];      // sL[col][row]
    __shared__ double sacc[RC][TS];
    __shared__ double sx[RC][TS];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int rbase = blockIdx.x * RC, nr = min(RC, R - rbase);
    const int nblk = (n + TS - 1) / TS;
    for (int m = blockIdx.y; m < nmat; m += gridDim.y) {
        const double* Lm = Lf + (long)m * strideL;
        double* Bm = B + (long)m * strideB + (long)rbase * ldb;
        for (int ib = nblk - 1; ib >= 0; --ib) {
            const int i0 = ib * TS, nb = min(TS, n - i0), below = i0 + nb;
            // column i0 + cc of the factor below the block, dotted with the solved part: one wave per column
            for (int cc = w; cc < nb; cc += 4) {
                double acc[RC];
                for (int r = 0; r < RC; ++r) acc[r] = 0.0;
                for (int j = below + lane; j < n; j += 64) {
                    const double l = Lm[(long)(i0 + cc) * lda + j];
                    for (int r = 0; r < RC; ++r)
                        if (r < nr) acc[r] += l * Bm[(long)r * ldb + j];
                }
                for (int r = 0; r < RC; ++r) {
                    double v = acc[r];
                    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
                    if (lane == 0) sacc[r][cc] = v;
                }
            }
            for (int c = w; c < TS; c += 4) sL[c][lane] = (lane < nb && c < nb && lane >= c) ? Lm[(long)(i0 + c) * lda + i0 + lane] : (lane == c ? 1.0 : 0.0);
            __syncthreads();
            // thread (cc = lane, r = w):  x_cc = (y_cc - sum_{j > cc} L[j][cc] x_j) / L[cc][cc]
            const int cc = lane;
            const bool on = cc < nb && w < nr;
            double v = 0.0;
            if (on) v = Bm[(long)w * ldb + i0 + cc] - sacc[w][cc];
            for (int j = nb - 1; j >= 0; --j) {
                if (cc == j) { v = v / sL[j][j]; sx[w][j] = v; }
                __syncthreads();
                if (cc < j) v -= sL[cc][j] * sx[w][j];
            }
            if (on) Bm[(long)w * ldb + i0 + cc] = v;
            __syncthreads();
        }
    }
}

void solve_batched(const double* Lf, int n, int lda, long strideL, double* B, int ldb, long strideB, int R, int nmat, hipStream_t st) {
    const dim3 grid((R + RC - 1) / RC, nmat < MAXGRID ? nmat : MAXGRID);
    AMS_BSS_LAUNCH(solve_fwd_kernel, grid, dim3(256), 0, st, Lf, n, lda, strideL, B, ldb, strideB, R, nmat);
    AMS_BSS_LAUNCH(solve_bwd_kernel, grid, dim3(256), 0, st, Lf, n, lda, strideL, B, ldb, strideB, R, nmat);
}

inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }
inline size_t max3(size_t a, size_t b, size_t c) { return a > b ? (a > c ? a : c) : (b > c ? b : c); }

#ifndef AMS_BSS_RAGGED
void destroy_plans(plan_set* p) {
    if (!p->nutt) return;
    hipfftDestroy(p->fwd_in); hipfftDestroy(p->inv_corr); hipfftDestroy(p->fwd_c); hipfftDestroy(p->inv_proj);
    p->nutt = 0;
}

bool make_plans(const ams_bssb_ctx* c, plan_set* p, int nutt) {
    destroy_plans(p);
    const int S = c->S, KS = c->KS, n = c->n;
    int made = 0;
    bool ok = hipfftPlan1d(&p->fwd_in, n, HIPFFT_D2Z, nutt * (S + KS)) == HIPFFT_SUCCESS;
    made += ok;
    ok = ok && hipfftPlan1d(&p->inv_corr, n, HIPFFT_Z2D, nutt * c->NP) == HIPFFT_SUCCESS;
    made += ok;
    ok = ok && hipfftPlan1d(&p->fwd_c, n, HIPFFT_D2Z, nutt * 2 * KS * S) == HIPFFT_SUCCESS;
    made += ok;
    ok = ok && hipfftPlan1d(&p->inv_proj, n, HIPFFT_Z2D, nutt * (KS + S * KS)) == HIPFFT_SUCCESS;
    made += ok;
    if (!ok) {
        if (made > 0) hipfftDestroy(p->fwd_in);
        if (made > 1) hipfftDestroy(p->inv_corr);
        if (made > 2) hipfftDestroy(p->fwd_c);
        return false;
    }
    p->nutt = nutt;
    return true;
}
#endif

}  // namespace

#ifndef AMS_BSS_RAGGED
extern "C" {

int ams_bssb_abi_version(void) { return 1; }

int ams_bssb_create(ams_bssb_ctx** out, int max_utt, int nsets, int nsrc, int nsampl, int flen) {
    if (!out || max_utt < 1 || max_utt > MAXGRID || nsets < 1 || nsets > 64 || nsrc < 1 || nsrc > 6 || nsampl < 1 || flen < 1) return -1;
    if ((long)max_utt * nsrc > MAXGRID) return -1;
    ams_bssb_ctx* c = (ams_bssb_ctx*)calloc(1, sizeof(ams_bssb_ctx));
    if (!c) return -3;
    const int U = max_utt, K = nsets, S = nsrc, F = flen, KS = K * S;
    c->U = U; c->K = K; c->S = S; c->L = nsampl; c->F = F; c->KS = KS;
    c->Lp = nsampl + flen - 1;
    int n = 1;
    while (n < c->Lp) n <<= 1;
    c->n = n; c->nc = n / 2 + 1;
    c->NP = S * (S + 1) / 2 + S * KS;
    if (!make_plans(c, &c->full, U)) { free(c); return -3; }
    const size_t d = sizeof(double), z = 2 * sizeof(double), nn = (size_t)n, nc = (size_t)c->nc, u = (size_t)U;
    const size_t N = (size_t)S * F;
    size_t o = 0;
    c->o_tpad = o;  o = align256(o + u * (S + KS) * nn * d);
    c->o_spec = o;  o = align256(o + u * (S + KS) * nc * z);
    c->o_a = o;     o = align256(o + u * max3((size_t)c->NP * nc * z, (size_t)2 * KS * S * nn * d, (size_t)(KS + S * KS) * nc * z));
    c->o_b = o;     o = align256(o + u * max3((size_t)c->NP * nn * d, (size_t)2 * KS * S * nc * z, (size_t)(KS + S * KS) * nn * d));
    c->o_G = o;     o = align256(o + u * N * N * d);
    c->o_Gj = o;    o = align256(o + u * S * F * F * d);
    c->o_Df = o;    o = align256(o + u * KS * N * d);
    c->o_Dj = o;    o = align256(o + u * KS * N * d);
    c->o_part = o;  o = align256(o + u * KS * S * RB * 5 * d);
    c->o_info = o;  o = align256(o + u * (1 + S) * sizeof(int));
    c->ws_bytes = o;
    *out = c;
    return 0;
}

void ams_bssb_destroy(ams_bssb_ctx* c) {
    if (!c) return;
    destroy_plans(&c->full);
    destroy_plans(&c->part);
    free(c);
}

size_t ams_bssb_workspace_bytes(const ams_bssb_ctx* c) { return c ? c->ws_bytes : 0; }

int ams_bssb_potrf(double* A, int n, int lda, long stride, int nmat, int* info, void* stream) {
    if (!A || !info || n < 1 || lda < n || nmat < 1 || (nmat > 1 && stride < (long)lda * (n - 1) + n)) return -1;
    return potrf_batched(A, n, lda, stride, nmat, info, (hipStream_t)stream);
}

int ams_bssb_eval(ams_bssb_ctx* c, int nutt, const double* ref, const double* est, double* crit, int* info, void* ws, size_t ws_bytes,
                  void* stream) {
    if (!c || !ref || !est || !crit || !info || !ws || nutt < 1 || nutt > c->U) return -1;
    if (ws_bytes < c->ws_bytes) return -2;
    plan_set* pl = &c->full;
    if (nutt != c->U) {
        pl = &c->part;
        if (pl->nutt != nutt && !make_plans(c, pl, nutt)) return -3;
    }
    hipStream_t st = (hipStream_t)stream;
    char* w = (char*)ws;
    const int S = c->S, KS = c->KS, F = c->F, n = c->n, nc = c->nc, N = S * F, NP = c->NP, U = nutt;
    double* tpad = (double*)(w + c->o_tpad);
    hipfftDoubleComplex* spec = (hipfftDoubleComplex*)(w + c->o_spec);
    hipfftDoubleComplex* xs = (hipfftDoubleComplex*)(w + c->o_a);
    double* corr = (double*)(w + c->o_b);
    double* G = (double*)(w + c->o_G);
    double* Gj = (double*)(w + c->o_Gj);
    double* Df = (double*)(w + c->o_Df);
    double* Dj = (double*)(w + c->o_Dj);
    double* cpad = (double*)(w + c->o_a);
    hipfftDoubleComplex* cspec = (hipfftDoubleComplex*)(w + c->o_b);
    hipfftDoubleComplex* pspec = (hipfftDoubleComplex*)(w + c->o_a);
    double* proj = (double*)(w + c->o_b);
    double* part = (double*)(w + c->o_part);
    int* info_f = (int*)(w + c->o_info);
    int* info_j = info_f + c->U;

    hipfftSetStream(pl->fwd_in, st); hipfftSetStream(pl->inv_corr, st); hipfftSetStream(pl->fwd_c, st); hipfftSetStream(pl->inv_proj, st);

    hipLaunchKernelGGL(pad_kernel, dim3(64, S + KS, U), dim3(256), 0, st, ref, est, tpad, S, KS, c->L, n);
    if (hipfftExecD2Z(pl->fwd_in, tpad, spec) != HIPFFT_SUCCESS) return -3;
    hipLaunchKernelGGL(cross_kernel, dim3(32, NP, U), dim3(256), 0, st, spec, xs, S, KS, NP, nc);
    if (hipfftExecZ2D(pl->inv_corr, xs, corr) != HIPFFT_SUCCESS) return -3;
    hipLaunchKernelGGL(gram_kernel, dim3(1024, U), dim3(256), 0, st, corr, G, Gj, S, F, n, NP);
    hipLaunchKernelGGL(rhs_kernel, dim3(16, U), dim3(256), 0, st, corr, Df, Dj, S, KS, F, n, NP);
    // factorise every Gram matrix once, then solve with all estimates of all sets as right-hand sides
    if (potrf_batched(G, N, N, (long)N * N, U, info_f, st) != 0) return -3;
    if (potrf_batched(Gj, F, F, (long)F * F, U * S, info_j, st) != 0) return -3;
    solve_batched(G, N, N, (long)N * N, Df, N, (long)KS * N, KS, U, st);
    solve_batched(Gj, F, F, (long)F * F, Dj, F, (long)KS * F, KS, U * S, st);
    hipLaunchKernelGGL(cpad_kernel, dim3(64, 2 * KS * S, U), dim3(256), 0, st, Df, Dj, cpad, S, KS, F, n);
    if (hipfftExecD2Z(pl->fwd_c, cpad, cspec) != HIPFFT_SUCCESS) return -3;
    hipLaunchKernelGGL(prod_kernel, dim3(32, KS + S * KS, U), dim3(256), 0, st, spec, cspec, pspec, S, KS, nc);
    if (hipfftExecZ2D(pl->inv_proj, pspec, proj) != HIPFFT_SUCCESS) return -3;
    hipLaunchKernelGGL(sums_kernel, dim3(RB, KS * S, U), dim3(256), 0, st, tpad, proj, part, S, KS, n, c->Lp);
    hipLaunchKernelGGL(crit_kernel, dim3(KS * S, U), dim3(64), 0, st, part, info_f, info_j, crit, info, S, KS);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

}  // extern "C"
#endif
