// The kernels of the FFT paths of BSS-eval around the hipFFT calls, in their batched form: U utterances x K sets of estimates,
// KS = K * S estimate rows per utterance.  bss_batch.hip launches them as they are; bss_eval.hip launches them with U = 1, KS = S.
// Everything here has internal linkage.
#ifndef AMS_BSS_FFT_PATH_H
#define AMS_BSS_FFT_PATH_H
#include <hip/hip_runtime.h>
#include <hipfft/hipfft.h>
#include "criteria.h"

namespace {

constexpr int RB = 256;            // blocks per (set, e, j) triple in the first reduction stage

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

// G[(I,a),(J,b)] with the reference's block overwrite order (utils/bss_eval.py:696-702: the later write wins); column-major ==
// row-major (symmetric up to rounding, and the factorisations only read the lower triangle of the column-major view = the upper
// triangle of this row-major fill): element (row, col) of the mathematical matrix lives at col*N + row.  Gj[I] = block (I, I).
// blockIdx.y = utterance
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
            for (int i = 0; i < S; ++i) {                                  // same order as :723-729 (i ascending)
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

// the decomposition of criteria.h over the Lp samples of one (estimate row ke, reference j) pair; stage 1 of 2: part[u][pair][RB][5].
// blockIdx.y = ke * S + j, blockIdx.z = utterance
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
    for (int t = blockIdx.x * blockDim.x + threadIdx.x; t < Lp; t += gridDim.x * blockDim.x)
        decompose_add(ref[t], pj[t] * sc, pf[t] * sc, est[t], a0, a1, a2, a3, a4);
    double* out = part_ + ((((long)u * KS * S) + pair) * RB + blockIdx.x) * 5;
    double v;
    v = block_sum(a0, sm); if (threadIdx.x == 0) out[0] = v;
    v = block_sum(a1, sm); if (threadIdx.x == 0) out[1] = v;
    v = block_sum(a2, sm); if (threadIdx.x == 0) out[2] = v;
    v = block_sum(a3, sm); if (threadIdx.x == 0) out[3] = v;
    v = block_sum(a4, sm); if (threadIdx.x == 0) out[4] = v;
}

// stage 2 + criteria.  blockIdx.x = ke * S + j, blockIdx.y = utterance.  crit[u][k][c][e][j]; NaN when a factorisation of
// THIS utterance failed: its flags are info_f[u] and info_j[u * nj .. (u + 1) * nj).
__global__ void crit_kernel(const double* __restrict__ part_, const int* __restrict__ info_f, const int* __restrict__ info_j, int nj,
                            double* __restrict__ crit, int* __restrict__ info_out, int S, int KS) {
    const int pair = blockIdx.x, u = blockIdx.y;
    if (threadIdx.x != 0) return;
    int bad = info_f[u] != 0;
    for (int i = 0; i < nj; ++i) bad |= (info_j[u * nj + i] != 0);
    const double* part = part_ + (((long)u * KS * S) + pair) * RB * 5;
    double s[5] = {0, 0, 0, 0, 0};
    for (int b = 0; b < RB; ++b)
        for (int k = 0; k < 5; ++k) s[k] += part[(long)b * 5 + k];
    const int set = pair / (S * S), ej = pair % (S * S), K = KS / S;
    criteria_store(s, bad, crit + ((long)u * K + set) * 3 * S * S, S * S, ej);
    if (pair == 0) info_out[u] = bad;
}

}  // namespace

#endif
