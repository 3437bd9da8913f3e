// Batched BSS-eval for gfx950 (include/ams_bss_batch.h): nutt utterances x nsets sets of estimates in one call.
//
// Same arithmetic as bss_eval.hip, one more index; the kernels around the FFTs are those of fft_path.h for both.  Per call:
//   1. ONE batched real FFT of all references and all estimates of all sets;
//   2. cross-spectra -> ONE batched inverse FFT -> the auto/cross-correlations (the reference pairs once per utterance,
//      reference x estimate for every set);
//   3. per utterance ONE (nsrc*flen)^2 Gram matrix and its nsrc diagonal blocks (same block overwrite order as bss_eval.hip);
//   4. all nutt*(1+nsrc) matrices factorised by the batched blocked Cholesky of chol_batched.h, then two batched triangular
//      solves with the nsets*nsrc estimates of the utterance as right-hand sides;
//   5. the filters applied by spectral multiplication, the same two-stage float64 sums, the same criteria (criteria.h).
#include <hip/hip_runtime.h>
#include <hipfft/hipfft.h>
#include <math.h>
#include <stdlib.h>
#include "../../../include/ams_bss_batch.h"
#include "chol_batched.h"
#include "fft_path.h"

namespace {

struct plan_set {
    int nutt;                      // 0: not planned
    hipfftHandle fwd_in, inv_corr, fwd_c, inv_proj;
};

}  // namespace

struct ams_bssb_ctx {
    int U, K, S, L, F, n, nc, Lp, NP, KS;
    plan_set full, part;           // plans for nutt == max_utt, and for the last other nutt asked for
    size_t ws_bytes;
    // offsets (in bytes) into the caller's workspace; `a` holds xs, then cpad, then pspec; `b` holds corr, then cspec, then proj
    size_t o_tpad, o_spec, o_a, o_b, o_G, o_Gj, o_Df, o_Dj, o_part, o_info;
};

namespace {

inline size_t max3(size_t a, size_t b, size_t c) { return a > b ? (a > c ? a : c) : (b > c ? b : c); }

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

}  // namespace

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
    return potrf_batched(A, n, lda, stride, nmat, info, (hipStream_t)stream) < 0 ? -3 : 0;
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
    if (potrf_batched(G, N, N, (long)N * N, U, info_f, st) < 0) return -3;
    if (potrf_batched(Gj, F, F, (long)F * F, U * S, info_j, st) < 0) return -3;
    solve_batched(G, N, N, (long)N * N, Df, N, (long)KS * N, KS, U, st);
    solve_batched(Gj, F, F, (long)F * F, Dj, F, (long)KS * F, KS, U * S, st);
    hipLaunchKernelGGL(cpad_kernel, dim3(64, 2 * KS * S, U), dim3(256), 0, st, Df, Dj, cpad, S, KS, F, n);
    if (hipfftExecD2Z(pl->fwd_c, cpad, cspec) != HIPFFT_SUCCESS) return -3;
    hipLaunchKernelGGL(prod_kernel, dim3(32, KS + S * KS, U), dim3(256), 0, st, spec, cspec, pspec, S, KS, nc);
    if (hipfftExecZ2D(pl->inv_proj, pspec, proj) != HIPFFT_SUCCESS) return -3;
    hipLaunchKernelGGL(sums_kernel, dim3(RB, KS * S, U), dim3(256), 0, st, tpad, proj, part, S, KS, n, c->Lp);
    hipLaunchKernelGGL(crit_kernel, dim3(KS * S, U), dim3(64), 0, st, part, info_f, info_j, S, crit, info, S, KS);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

}  // extern "C"
