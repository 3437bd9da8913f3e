// BSS-eval (SDR / SIR / SAR) for gfx950 -- reference utils/bss_eval.py:586-748 (cupy path).
//
// The reference recomputes, for every (estimate, reference) pair, the FFTs of the references, the Toeplitz Gram matrix of
// their delayed copies (flen = 512 lags) and a dense LU solve.  None of that depends on the estimate, so here per utterance:
//   1. ONE batched real FFT of the nsrc references and nsrc estimates (zero padded to n = 2^ceil(log2(nsampl+flen-1)));
//   2. cross-spectra -> ONE batched inverse FFT -> all auto/cross-correlations (reference pairs and reference x estimate);
//   3. the (nsrc*flen)^2 Gram matrix assembled ONCE from them (its diagonal blocks are the single-reference Grams), with the
//      reference's block write order (:696-702: the later write wins) reproduced exactly;
//   4. Cholesky factorisations (hipSOLVER potrf): 1 full + nsrc single, then potrs with all estimates as right-hand sides;
//   5. the distortion filters applied by spectral multiplication (one batched FFT each way), sums of squares in float64 with a
//      fixed two-stage reduction order, criteria with the reference's 10 log10(num / (den + 1e-12)).
// float64 throughout, as the reference (:595-596).  The kernels are those of fft_path.h (shared with bss_batch.hip), launched with
// one utterance and one set of estimates: U = 1, KS = S.
#include <hip/hip_runtime.h>
#include <hipfft/hipfft.h>
#include <hipsolver/hipsolver.h>
#include <math.h>
#include <stdlib.h>
#include "../../../include/ams_bss.h"
#include "fft_path.h"

struct ams_bss_ctx {
    int S, L, F, n, nc, Lp, NP;
    hipfftHandle fwd_in, inv_corr, fwd_c, inv_proj;
    hipsolverHandle_t solver;
    int lwork;
    size_t ws_bytes;
    // offsets (in bytes) into the caller's workspace
    size_t o_tpad, o_spec, o_xs, o_corr, o_G, o_Gj, o_Df, o_Dj, o_cpad, o_cspec, o_pspec, o_proj, o_part, o_work, o_info;
};

static inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

extern "C" {

int ams_bss_abi_version(void) { return 1; }

int ams_bss_create(ams_bss_ctx** out, int nsrc, int nsampl, int flen) {
    if (!out || nsrc < 1 || nsrc > 6 || nsampl < 1 || flen < 1) return -1;
    ams_bss_ctx* c = (ams_bss_ctx*)calloc(1, sizeof(ams_bss_ctx));
    if (!c) return -3;
    c->S = nsrc; c->L = nsampl; c->F = flen;
    c->Lp = nsampl + flen - 1;
    int n = 1;
    while (n < c->Lp) n <<= 1;                                   // :689
    c->n = n; c->nc = n / 2 + 1;
    const int S = nsrc, F = flen;
    c->NP = S * (S + 1) / 2 + S * S;
    bool ok = hipfftPlan1d(&c->fwd_in, n, HIPFFT_D2Z, 2 * S) == HIPFFT_SUCCESS;
    ok = ok && hipfftPlan1d(&c->inv_corr, n, HIPFFT_Z2D, c->NP) == HIPFFT_SUCCESS;
    ok = ok && hipfftPlan1d(&c->fwd_c, n, HIPFFT_D2Z, 2 * S * S) == HIPFFT_SUCCESS;
    ok = ok && hipfftPlan1d(&c->inv_proj, n, HIPFFT_Z2D, S + S * S) == HIPFFT_SUCCESS;
    ok = ok && hipsolverCreate(&c->solver) == HIPSOLVER_STATUS_SUCCESS;
    if (!ok) { free(c); return -3; }
    int lw1 = 0, lw2 = 0, lw3 = 0, lw4 = 0;
    hipsolverDpotrf_bufferSize(c->solver, HIPSOLVER_FILL_MODE_LOWER, S * F, nullptr, S * F, &lw1);
    hipsolverDpotrf_bufferSize(c->solver, HIPSOLVER_FILL_MODE_LOWER, F, nullptr, F, &lw2);
    hipsolverDpotrs_bufferSize(c->solver, HIPSOLVER_FILL_MODE_LOWER, S * F, S, nullptr, S * F, nullptr, S * F, &lw3);
    hipsolverDpotrs_bufferSize(c->solver, HIPSOLVER_FILL_MODE_LOWER, F, S, nullptr, F, nullptr, F, &lw4);
    c->lwork = lw1;
    if (lw2 > c->lwork) c->lwork = lw2;
    if (lw3 > c->lwork) c->lwork = lw3;
    if (lw4 > c->lwork) c->lwork = lw4;
    size_t o = 0;
    const size_t d = sizeof(double), z = 2 * sizeof(double);
    c->o_tpad = o;  o = align256(o + (size_t)2 * S * n * d);
    c->o_spec = o;  o = align256(o + (size_t)2 * S * c->nc * z);
    c->o_xs = o;    o = align256(o + (size_t)c->NP * c->nc * z);
    c->o_corr = o;  o = align256(o + (size_t)c->NP * n * d);
    c->o_G = o;     o = align256(o + (size_t)S * F * S * F * d);
    c->o_Gj = o;    o = align256(o + (size_t)S * F * F * d);
    c->o_Df = o;    o = align256(o + (size_t)S * S * F * d);
    c->o_Dj = o;    o = align256(o + (size_t)S * S * F * d);
    c->o_cpad = o;  o = align256(o + (size_t)2 * S * S * n * d);
    c->o_cspec = o; o = align256(o + (size_t)2 * S * S * c->nc * z);
    c->o_pspec = o; o = align256(o + (size_t)(S + S * S) * c->nc * z);
    c->o_proj = o;  o = align256(o + (size_t)(S + S * S) * n * d);
    c->o_part = o;  o = align256(o + (size_t)S * S * RB * 5 * d);
    c->o_work = o;  o = align256(o + (size_t)(c->lwork > 0 ? c->lwork : 1) * d);
    c->o_info = o;  o = align256(o + (size_t)(2 * (1 + S)) * sizeof(int));
    c->ws_bytes = o;
    *out = c;
    return 0;
}

void ams_bss_destroy(ams_bss_ctx* c) {
    if (!c) return;
    hipfftDestroy(c->fwd_in); hipfftDestroy(c->inv_corr); hipfftDestroy(c->fwd_c); hipfftDestroy(c->inv_proj);
    hipsolverDestroy(c->solver);
    free(c);
}

size_t ams_bss_workspace_bytes(const ams_bss_ctx* c) { return c ? c->ws_bytes : 0; }

int ams_bss_eval_pairs(ams_bss_ctx* c, const double* ref, const double* est, double* crit, int* info, void* ws, size_t ws_bytes,
                       void* stream) {
    if (!c || !ref || !est || !crit || !info || !ws) return -1;
    if (ws_bytes < c->ws_bytes) return -2;
    hipStream_t st = (hipStream_t)stream;
    char* w = (char*)ws;
    const int S = c->S, F = c->F, n = c->n, nc = c->nc, N = S * F;
    double* tpad = (double*)(w + c->o_tpad);
    hipfftDoubleComplex* spec = (hipfftDoubleComplex*)(w + c->o_spec);
    hipfftDoubleComplex* xs = (hipfftDoubleComplex*)(w + c->o_xs);
    double* corr = (double*)(w + c->o_corr);
    double* G = (double*)(w + c->o_G);
    double* Gj = (double*)(w + c->o_Gj);
    double* Df = (double*)(w + c->o_Df);
    double* Dj = (double*)(w + c->o_Dj);
    double* cpad = (double*)(w + c->o_cpad);
    hipfftDoubleComplex* cspec = (hipfftDoubleComplex*)(w + c->o_cspec);
    hipfftDoubleComplex* pspec = (hipfftDoubleComplex*)(w + c->o_pspec);
    double* proj = (double*)(w + c->o_proj);
    double* part = (double*)(w + c->o_part);
    double* work = (double*)(w + c->o_work);
    int* dinfo = (int*)(w + c->o_info);

    hipfftSetStream(c->fwd_in, st); hipfftSetStream(c->inv_corr, st); hipfftSetStream(c->fwd_c, st); hipfftSetStream(c->inv_proj, st);
    hipsolverSetStream(c->solver, st);

    hipLaunchKernelGGL(pad_kernel, dim3(64, 2 * S, 1), dim3(256), 0, st, ref, est, tpad, S, S, c->L, n);
    if (hipfftExecD2Z(c->fwd_in, tpad, spec) != HIPFFT_SUCCESS) return -3;
    hipLaunchKernelGGL(cross_kernel, dim3(32, c->NP, 1), dim3(256), 0, st, spec, xs, S, S, c->NP, nc);
    if (hipfftExecZ2D(c->inv_corr, xs, corr) != HIPFFT_SUCCESS) return -3;
    hipLaunchKernelGGL(gram_kernel, dim3(1024, 1), dim3(256), 0, st, corr, G, Gj, S, F, n, c->NP);
    hipLaunchKernelGGL(rhs_kernel, dim3(16, 1), dim3(256), 0, st, corr, Df, Dj, S, S, F, n, c->NP);
    // factorise + solve: full system with the nsrc estimates as right-hand sides, then each single-reference system
    int k = 0;
    if (hipsolverDpotrf(c->solver, HIPSOLVER_FILL_MODE_LOWER, N, G, N, work, c->lwork, dinfo + k++) != HIPSOLVER_STATUS_SUCCESS) return -3;
    if (hipsolverDpotrs(c->solver, HIPSOLVER_FILL_MODE_LOWER, N, S, G, N, Df, N, work, c->lwork, dinfo + k++) != HIPSOLVER_STATUS_SUCCESS) return -3;
    for (int j = 0; j < S; ++j) {
        double* A = Gj + (long)j * F * F;
        double* B = Dj + (long)j * S * F;
        if (hipsolverDpotrf(c->solver, HIPSOLVER_FILL_MODE_LOWER, F, A, F, work, c->lwork, dinfo + k++) != HIPSOLVER_STATUS_SUCCESS) return -3;
        if (hipsolverDpotrs(c->solver, HIPSOLVER_FILL_MODE_LOWER, F, S, A, F, B, F, work, c->lwork, dinfo + k++) != HIPSOLVER_STATUS_SUCCESS) return -3;
    }
    hipLaunchKernelGGL(cpad_kernel, dim3(64, 2 * S * S, 1), dim3(256), 0, st, Df, Dj, cpad, S, S, F, n);
    if (hipfftExecD2Z(c->fwd_c, cpad, cspec) != HIPFFT_SUCCESS) return -3;
    hipLaunchKernelGGL(prod_kernel, dim3(32, S + S * S, 1), dim3(256), 0, st, spec, cspec, pspec, S, S, nc);
    if (hipfftExecZ2D(c->inv_proj, pspec, proj) != HIPFFT_SUCCESS) return -3;
    hipLaunchKernelGGL(sums_kernel, dim3(RB, S * S, 1), dim3(256), 0, st, tpad, proj, part, S, S, n, c->Lp);
    // every flag of dinfo[0 .. k) turns the result into NaN: dinfo[0] as the utterance's own, the k - 1 others behind it
    hipLaunchKernelGGL(crit_kernel, dim3(S * S, 1), dim3(64), 0, st, part, dinfo, dinfo + 1, k - 1, crit, info, S, S);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

}  // extern "C"
