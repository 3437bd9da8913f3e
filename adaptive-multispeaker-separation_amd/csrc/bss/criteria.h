// What all three BSS-eval paths (bss_eval.hip, bss_batch.hip, bss_ragged.hip) compute identically: the block reduction, the signal
// decomposition of the reference's utils/bss_eval.py:641-663 and its criteria (:732-748).  Everything here has internal linkage.
// How the partial sums of a (estimate, reference) pair are added up stays with each path's crit kernel: that order is its contract.
#ifndef AMS_BSS_CRITERIA_H
#define AMS_BSS_CRITERIA_H
#include <hip/hip_runtime.h>
#include <math.h>

namespace {

// the sum of v over the workgroup, valid in thread 0: lanes by shuffle, then the waves in ascending order
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

// One sample: s_true the reference, p_single / p_full the estimate's projections on that reference alone / on all references
// (already scaled), est the estimate.  Adds the five squares into a0 .. a4:
//   a0 |s_filt|^2   a1 |e_interf + e_artif|^2   a2 |e_interf|^2   a3 |s_filt + e_interf|^2   a4 |e_artif|^2
__device__ __forceinline__ void decompose_add(double s_true, double p_single, double p_full, double est, double& a0, double& a1,
                                              double& a2, double& a3, double& a4) {
    const double e_spat = p_single - s_true;
    const double e_interf = p_full - s_true - e_spat;
    const double e_artif = -s_true - e_spat - e_interf + est;
    const double s_filt = s_true + e_spat;
    a0 += s_filt * s_filt;
    a1 += (e_interf + e_artif) * (e_interf + e_artif);
    a2 += e_interf * e_interf;
    a3 += (s_filt + e_interf) * (s_filt + e_interf);
    a4 += e_artif * e_artif;
}

// the five totals of a pair -> out[c * stride + at] = SDR, SIR, SAR (c = 0, 1, 2) in dB; NaN when a factorisation failed
__device__ __forceinline__ void criteria_store(const double* s, int bad, double* out, int stride, int at) {
    const double nanv = nan("");
    out[0 * stride + at] = bad ? nanv : 10.0 * log10(s[0] / (s[1] + 1e-12));
    out[1 * stride + at] = bad ? nanv : 10.0 * log10(s[0] / (s[2] + 1e-12));
    out[2 * stride + at] = bad ? nanv : 10.0 * log10(s[3] / (s[4] + 1e-12));
}

}  // namespace

#endif
