// Batched blocked Cholesky and triangular solves for gfx950, float64: shared by bss_batch.hip (libams_bss.so) and bss_ragged.hip
// (libams_bss_ragged.so).  Needs hip_runtime.h only; everything here has internal linkage.
//
// Cholesky (right-looking, lower, column-major, panel width NB = 32), three launches per block column, the grid of each spanning
// matrices x tiles, ordinary stream order between them:
//   potrf_diag   one workgroup per matrix: the NB x NB diagonal block factorised in LDS (unblocked, column by column);
//   potrf_panel  one workgroup per 64 rows below it: inverts the diagonal factor in LDS (each workgroup its own copy -- no
//                workspace, no cross-workgroup traffic) and forms  panel <- panel * inv(L_kk)^T  with v_mfma_f64_16x16x4_f64;
//   potrf_trail  one workgroup per 64 x 64 tile of the lower trailing matrix:  C_ij -= P_i * P_j^T  with the same instruction.
// Both products are computed TRANSPOSED (D' = B * A^T), because the f64 MFMA's C/D map is col = lane & 15,
// row = (lane >> 4) + 4 * reg: with the matrix row on `col`, 16 lanes touch 16 consecutive doubles of a column.
// A non-positive (or NaN) pivot sets info[m] once and writes NaN as the pivot; the NaN spreads through that matrix only.
// No atomics, no persistent grid, every sum in a fixed order: a factor is a function of its matrix alone.
// potrf_batched and solve_batched return the number of launches they enqueued, for callers that promise a launch count.
#ifndef AMS_BSS_CHOL_BATCHED_H
#define AMS_BSS_CHOL_BATCHED_H
#include <hip/hip_runtime.h>
#include <math.h>
#include <stddef.h>

namespace {

constexpr int NB = 32;             // Cholesky panel width
constexpr int TM = 64;             // rows / columns of a panel or trailing tile
constexpr int TS = 64;             // rows per step of the triangular solves
constexpr int RC = 4;              // right-hand sides per workgroup of the triangular solves
constexpr int MAXGRID = 65535;

typedef double d4 __attribute__((ext_vector_type(4)));

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

// -> the number of launches enqueued (potrf_launches(n)), or -3
int potrf_batched(double* A, int n, int lda, long stride, int nmat, int* info, hipStream_t st) {
    if (hipMemsetAsync(info, 0, (size_t)nmat * sizeof(int), st) != hipSuccess) return -3;
    const int gm = nmat < MAXGRID ? nmat : MAXGRID;
    int launches = 0;
    for (int k0 = 0; k0 < n; k0 += NB) {
        hipLaunchKernelGGL(potrf_diag_kernel, dim3(gm), dim3(256), 0, st, A, n, lda, stride, nmat, k0, info);
        ++launches;
        const int rem = n - k0 - NB;
        if (rem <= 0) break;
        const int T = (rem + TM - 1) / TM;
        hipLaunchKernelGGL(potrf_panel_kernel, dim3(T, gm), dim3(256), 0, st, A, n, lda, stride, nmat, k0);
        hipLaunchKernelGGL(potrf_trail_kernel, dim3(T, T, gm), dim3(256), 0, st, A, n, lda, stride, nmat, k0);
        launches += 2;
    }
    return hipGetLastError() == hipSuccess ? launches : -3;
}

// what potrf_batched enqueues for order n: diag for every block column, panel + trail for all but the last
inline int potrf_launches(int n) { return 3 * ((n + NB - 1) / NB) - 2; }

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

// -> the number of launches enqueued (always 2)
int solve_batched(const double* Lf, int n, int lda, long strideL, double* B, int ldb, long strideB, int R, int nmat, hipStream_t st) {
    const dim3 grid((R + RC - 1) / RC, nmat < MAXGRID ? nmat : MAXGRID);
    hipLaunchKernelGGL(solve_fwd_kernel, grid, dim3(256), 0, st, Lf, n, lda, strideL, B, ldb, strideB, R, nmat);
    hipLaunchKernelGGL(solve_bwd_kernel, grid, dim3(256), 0, st, Lf, n, lda, strideL, B, ldb, strideB, R, nmat);
    return 2;
}

inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

}  // namespace

#endif
