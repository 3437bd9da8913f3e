// Batched k-means mask assignment (reference models/Kmeans_2.py:86-188), HBM-bound streaming kernels.
//
// The reference tiles X nb_tries times (2.1 GB at the benchmark shape) and broadcasts a [R,L,C,E] temporary per
// label pass (4.2 GB).  Here the un-tiled, normalised embeddings are streamed: row r = b*tries + try reads x[b]
// (tries index the centroid set only), one pass computes the assignment AND the centroid numerators/denominators
// for the next iteration, and nothing larger than [R, chunks, C*(E+1)] partial sums is written.
//
// Algorithmic bytes per pass: L*E*4 per row (+ L*4 weights); x[b] is shared by the `tries` rows of an utterance
// through L2.
//
// The hard passes (per-try, grouped accumulation, five-tries, select) and the summation order they share with oracle/kmeans.py are in
// kmeans_hard.h, instantiated here with the dense geometry KmDense.  This file keeps the normalisation, the stand-alone reduce, the
// soft accumulation, the seed gather and the entry points.  Contraction is off in this unit (Makefile, and kmeans_hard.h's pragma).
#include <stdlib.h>
#include "kmeans_hard.h"

namespace {

// x [nrows, E] -> xn: x * (1/sqrt(max(sum_e x^2, 1e-12))), sequential over e (tf.nn.l2_normalize, Kmeans_2.py:40-41).
// Rows are staged through LDS in slabs of 256 so global traffic is coalesced while each thread still sums ITS row left to right
// (the order oracle/kmeans.py uses): 1.59 ms -> HBM speed for the 210 MB embedding tensor of the benchmark shape.
__global__ __launch_bounds__(256) void kmeans_normalize_kernel(const float* __restrict__ x, float* __restrict__ xn, long nrows, int E) {
    extern __shared__ float tile[];                  // [256][E + 1]
    const int LD = E + 1, tid = threadIdx.x;
    for (long r0 = (long)blockIdx.x * 256; r0 < nrows; r0 += (long)gridDim.x * 256) {
        const int nr = (int)min((long)256, nrows - r0);
        const float* src = x + r0 * E;
        __syncthreads();
        for (int i = tid; i < nr * E; i += 256) tile[(i / E) * LD + (i % E)] = src[i];
        __syncthreads();
        if (tid < nr) {
            float* p = tile + tid * LD;
            float ss = 0.f;
            for (int e = 0; e < E; ++e) ss = __fadd_rn(ss, __fmul_rn(p[e], p[e]));
            const float inv = ((1.0f) / (sqrtf(fmaxf(ss, 1e-12f))));
            for (int e = 0; e < E; ++e) p[e] = __fmul_rn(p[e], inv);
        }
        __syncthreads();
        float* dst = xn + r0 * E;
        for (int i = tid; i < nr * E; i += 256) dst[i] = tile[(i / E) * LD + (i % E)];
    }
}

// Sum the G partial rows of a row in order; ACC passes: centroid = num / den.  FINAL passes: inertia[r] = sum_c tot_c/cnt_c.
__global__ void kmeans_reduce_kernel(const float* __restrict__ part, float* __restrict__ out, float* __restrict__ den_out, int R,
                                     int G, int C, int E, int final_) {
    const int NV = final_ ? 2 * C : C * (E + 1);
    const int per = final_ ? 1 : C * E;
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long)R * per) return;
    const int r = (int)(i / per), k = (int)(i - (long)r * per);
    const float* pr = part + (long)r * G * NV;
    if (final_) {
        float inertia = 0.f;
        for (int c = 0; c < C; ++c) {
            float tot = 0.f, cnt = 0.f;
            for (int g = 0; g < G; ++g) { tot = __fadd_rn(tot, pr[(long)g * NV + c]); cnt = __fadd_rn(cnt, pr[(long)g * NV + C + c]); }
            inertia = __fadd_rn(inertia, ((tot) / (cnt)));
        }
        out[r] = inertia;
    } else {
        const int c = k / E;
        float num = 0.f, den = 0.f;
        for (int g = 0; g < G; ++g) { num = __fadd_rn(num, pr[(long)g * NV + k]); den = __fadd_rn(den, pr[(long)g * NV + C * E + c]); }
        out[(long)r * C * E + k] = ((num) / (den));
        if (den_out && (k % E) == 0) den_out[(long)r * C + c] = den;
    }
}

// ------------------------------------------------------------------------------------------------------------------------------
// SOFT_ACC the way csrc/kmeans_soft.hip runs its backward passes (round 5; E = 40, tolerance-checked like every soft mode):
//   * the row's centroids are SCALAR operands (s_load through the constant address space) of packed FMAs, not LDS broadcast reads
//     (40 ds_read_b64 per point in kmeans_pass_kernel's soft branch);
//   * d_c = w (|x|^2 - 2 <x, c> + |c|^2): one dot product per cluster (20 v_pk_fma) instead of subtract / multiply / add per element;
//   * sums as v_pk_fma with the factor w lab_c; slab j + 1 is requested while slab j is worked on; ONE resident round of workgroups
//     (512 / R chunks per row).
// ~120 vector instructions per point instead of ~480: 66 -> 42 us per pass at 64 rows x 20480 points (fine-tuning step 4.54 -> 4.33 ms).
struct KsfArgs {
    const float* xn; const float* w; const float* cent; float* part; unsigned* tickets; float* cent_out; float* den_out;
    long L; int b, tries, nG, spw, w_mod_b; float beta;
};
typedef const f2 __attribute__((address_space(4))) kt_cf2;

template <int C_, bool HAS_W>
__global__ __launch_bounds__(256) void kmeans_soft_acc_kernel(KsfArgs a) {
    constexpr int E_ = 40, CE = C_ * E_, NV = CE + C_, LD = E_ + 4, V4 = E_ / 4, H = E_ / 2;
    __shared__ __attribute__((aligned(16))) float buf[256 * LD];
    __shared__ int last_sh;
    const int r = blockIdx.y, g = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int bi = r / a.tries;
    const float* xb = a.xn + (long)bi * a.L * E_;
    const float* wb = HAS_W ? a.w + (long)(a.w_mod_b ? (r % a.b) : bi) * a.L : nullptr;
    const kt_cfloat* cen = (const kt_cfloat*)(a.cent + (long)r * CE);
    kt_cf2* cen2 = (kt_cf2*)cen;
    float cc[C_];                                               // |c|^2 (uniform: scalar operands)
#pragma unroll
    for (int c = 0; c < C_; ++c) {
        float v = 0.f;
#pragma unroll
        for (int e = 0; e < E_; ++e) v = fmaf(cen[c * E_ + e], cen[c * E_ + e], v);
        cc[c] = v;
    }
    f2 acc2[C_][H];
    float den[C_];
#pragma unroll
    for (int c = 0; c < C_; ++c) {
        den[c] = 0.f;
#pragma unroll
        for (int q = 0; q < H; ++q) acc2[c][q] = (f2){0.f, 0.f};
    }
    float4 pre[V4];
    float wpre = 1.0f;
    auto fetch = [&](int j) {
        const long q0 = ((long)g * a.spw + j) * LANES;
        const long lim = (a.L - q0) * V4;
        const float4* src = reinterpret_cast<const float4*>(xb + q0 * E_);
#pragma unroll
        for (int k = 0; k < V4; ++k) {
            const long i = tid + 256 * k;
            pre[k] = src[i < lim ? i : (lim > 0 ? lim - 1 : -q0 * V4)];       // clamped inside the utterance's rows
        }
        if (HAS_W) wpre = wb[min(q0 + tid, a.L - 1)];
    };
    fetch(0);
    for (int j = 0; j < a.spw; ++j) {
        const long p0 = ((long)g * a.spw + j) * LANES;
        const int npts = (int)max((long)0, min((long)LANES, a.L - p0));
        if (npts <= 0) break;                                   // (workgroup-uniform)
        __syncthreads();
#pragma unroll
        for (int k = 0; k < V4; ++k) {
            const int i = tid + 256 * k;
            const int row = i / V4, c4 = i - row * V4;
            *reinterpret_cast<float4*>(&buf[row * LD + c4 * 4]) = (i < npts * V4) ? pre[k] : make_float4(0.f, 0.f, 0.f, 0.f);
        }
        __syncthreads();
        const float wv = wpre;
        if (j + 1 < a.spw) fetch(j + 1);
        if (tid < npts) {
            f2 x2[H];
            f2 xs = {0.f, 0.f};
#pragma unroll
            for (int q = 0; q < V4; ++q) {
                const float4 v = *reinterpret_cast<const float4*>(&buf[tid * LD + q * 4]);
                x2[2 * q] = (f2){v.x, v.y}; x2[2 * q + 1] = (f2){v.z, v.w};
                xs = __builtin_elementwise_fma(x2[2 * q], x2[2 * q], xs);
                xs = __builtin_elementwise_fma(x2[2 * q + 1], x2[2 * q + 1], xs);
            }
            const float xx = xs[0] + xs[1];
            float lab[C_], sum = 0.f;
#pragma unroll
            for (int c = 0; c < C_; ++c) {
                f2 sd = {0.f, 0.f};
#pragma unroll
                for (int q = 0; q < H; ++q) sd = __builtin_elementwise_fma(x2[q], (f2)cen2[c * H + q], sd);
                const float d = fmaxf(xx - 2.0f * (sd[0] + sd[1]) + cc[c], 0.f) * (HAS_W ? wv : 1.0f);
                lab[c] = expf(-a.beta * d);
                sum += lab[c];
            }
            const float inv = 1.0f / sum;
#pragma unroll
            for (int c = 0; c < C_; ++c) {
                const float lb = lab[c] * inv, wl = HAS_W ? wv * lb : lb;
                const f2 wl2 = {wl, wl};
#pragma unroll
                for (int q = 0; q < H; ++q) acc2[c][q] = __builtin_elementwise_fma(x2[q], wl2, acc2[c][q]);
                den[c] += lb;
            }
        }
    }
    // workgroup sum of the NV values: a lane tree per wave (VALU), the four wave totals meet in LDS
    __syncthreads();
#pragma unroll
    for (int c = 0; c < C_; ++c) {
#pragma unroll
        for (int q = 0; q < H; ++q) {
            const float v0 = wave_sum_lane0(acc2[c][q][0]), v1 = wave_sum_lane0(acc2[c][q][1]);
            if (lane == 0) { buf[wave * NV + c * E_ + 2 * q] = v0; buf[wave * NV + c * E_ + 2 * q + 1] = v1; }
        }
        const float vd = wave_sum_lane0(den[c]);
        if (lane == 0) buf[wave * NV + CE + c] = vd;
    }
    __syncthreads();
    float* const mypart = a.part + ((long)r * a.nG + g) * NV;
    for (int i = tid; i < NV; i += 256) {
        const float v = (buf[i] + buf[NV + i]) + (buf[2 * NV + i] + buf[3 * NV + i]);
        if (a.tickets) __hip_atomic_store(mypart + i, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        else mypart[i] = v;
    }
    if (a.tickets == nullptr) return;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __syncthreads();
    if (tid == 0) {
        const int last = atomicAdd(a.tickets + r, 1u) == (unsigned)a.nG - 1u;
        if (last) __hip_atomic_store(a.tickets + r, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        last_sh = last;
    }
    __syncthreads();
    if (!last_sh || tid >= CE) return;
    const int c = tid / E_;
    float num = 0.f, dn = 0.f;
    for (int q = 0; q < a.nG; ++q) {
        num += __hip_atomic_load(a.part + ((long)r * a.nG + q) * NV + tid, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        dn += __hip_atomic_load(a.part + ((long)r * a.nG + q) * NV + CE + c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    a.cent_out[(long)r * CE + tid] = num / dn;
    if (a.den_out && (tid % E_) == 0) a.den_out[(long)r * C_ + c] = dn;
}

// centroids[r,c,:] = xn[r/tries, idx[r,c], :]                 (Kmeans_2.py:61-71)
__global__ void kmeans_init_kernel(const float* __restrict__ xn, const int32_t* __restrict__ idx, float* __restrict__ cent, int R,
                                   int C, int E, long L, int tries) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long)R * C * E) return;
    const int e = (int)(i % E);
    const long rc = i / E;
    const int r = (int)(rc / C);
    cent[i] = xn[((long)(r / tries) * L + idx[rc]) * E + e];
}

}  // namespace

extern "C" {

ams_status ams_kmeans_normalize(const float* x, float* xn, long nrows, int E, void* stream) {
    AMS_REQUIRE(x && xn && nrows > 0 && E > 0);
    AMS_REQUIRE(E <= 60);                                   // 256 x (E+1) floats of LDS
    long blocks = (nrows + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(kmeans_normalize_kernel, dim3((int)blocks), dim3(256), (size_t)256 * (E + 1) * sizeof(float), (hipStream_t)stream,
                       x, xn, nrows, E);
    return ams_check_launch();
}

#ifdef AMS_KT_DBG
static unsigned long long* g_kt_dbg = nullptr;
unsigned long long* ams_dbg_kt_buffer(size_t words) {       // device buffer the next launches write their placement / times to
    if (!g_kt_dbg) { hipMalloc((void**)&g_kt_dbg, words * 8); hipMemset(g_kt_dbg, 0, words * 8); }
    return g_kt_dbg;
}
int ams_dbg_kt_occupancy() {
    int n = -1;
    hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, kmeans_hard_tries_kernel<KmDense, false>, 640, KT_LDS_BYTES);
    return n;
}
#endif

size_t ams_kmeans_workspace_bytes(int R, long L, int E, int C) {
    const int NP = max(ceil_div(L, CHUNK_SOFT), 4 * ceil_div(L, CHUNK_HARD));      // partial rows per row, whichever mode runs
    return sizeof(float) * (size_t)R * NP * C * (E + 1);
}

ams_status ams_kmeans_init(const float* xn, const int32_t* init_idx, float* centroids, int b, int tries, long L, int E, int C,
                           void* stream) {
    AMS_REQUIRE(xn && init_idx && centroids && b > 0 && tries > 0 && L > 0);
    const long n = (long)b * tries * C * E;
    hipLaunchKernelGGL(kmeans_init_kernel, dim3(ceil_div(n, 256)), dim3(256), 0, (hipStream_t)stream, xn, init_idx, centroids,
                       b * tries, C, E, L, tries);
    return ams_check_launch();
}

// One Lloyd iteration for all R = b*tries rows: labels from `cent_in`, new centroids to `cent_out`.
// beta < 0: hard assignment (argmin), else soft assignment softmax(-beta d^2).
ams_status ams_kmeans_iterate(const float* xn, const float* w, const float* cent_in, float* cent_out, float* den_out, int b, int tries,
                              long L, int E, int C, float beta, int w_mod_b, void* ws, size_t ws_bytes, void* tickets, void* stream) {
    AMS_REQUIRE(xn && cent_in && cent_out && ws && b > 0 && tries > 0 && L > 0 && C >= 2 && C <= 6);
    const int R = b * tries;
    if (ws_bytes < ams_kmeans_workspace_bytes(R, L, E, C)) return AMS_E_WORKSPACE_TOO_SMALL;
    hipStream_t st = (hipStream_t)stream;
    KmDense::Args a{};
    a.xn = xn; a.w = w; a.cent = cent_in; a.part = (float*)ws; a.L = L; a.b = b; a.tries = tries; a.G = ceil_div(L, chunk_of(beta >= 0.f));
    a.w_mod_b = w_mod_b; a.beta = beta; a.one = 1.0f;
    a.tickets = (unsigned*)tickets; a.fin_out = cent_out; a.fin_den = den_out;
    // AMS_KM_TRIES=0: every try a workgroup of its own (kmeans_pass_kernel) also where kmeans_hard_tries_kernel applies -- same bits
    static const bool tries_kernel = [] { const char* e = getenv("AMS_KM_TRIES"); return !(e && e[0] == '0'); }();
    if (tries_kernel && beta < 0.f && E == 40 && C == 2 && tries % TQ == 0 && L * E * 4 < (1L << 31))   /* 32-bit buffer offsets */ {
        KtArgs k{};
        k.xn = xn; k.cent = cent_in; k.part = (float*)ws; k.tickets = (unsigned*)tickets; k.fin_out = cent_out; k.fin_den = den_out;
        k.L = L; k.b = b; k.tries = tries; k.G = a.G; k.w = w; k.w_mod_b = w_mod_b;
#ifdef AMS_KT_DBG
        k.dbg = g_kt_dbg;
#endif
        if (w) hipLaunchKernelGGL((kmeans_hard_tries_kernel<KmDense, true>), dim3((unsigned)(b * (tries / TQ) * 4 * a.G)), dim3(640), KT_LDS_BYTES, st, k);
        else hipLaunchKernelGGL((kmeans_hard_tries_kernel<KmDense, false>), dim3((unsigned)(b * (tries / TQ) * 4 * a.G)), dim3(640), KT_LDS_BYTES, st, k);
        ams_status s2 = ams_check_launch();
        if (s2 != AMS_OK || tickets) return s2;
        hipLaunchKernelGGL(kmeans_reduce_kernel, dim3(ceil_div((long)R * C * E, 256)), dim3(256), 0, st, (const float*)ws, cent_out, den_out, R,
                           4 * a.G, C, E, 0);
        return ams_check_launch();
    }
    // AMS_KM_SOFT=0: the soft accumulation pass of kmeans_pass_kernel also where kmeans_soft_acc_kernel applies
    static const bool soft_kernel = [] { const char* e = getenv("AMS_KM_SOFT"); return !(e && e[0] == '0'); }();
    if (soft_kernel && beta >= 0.f && E == 40) {
        KsfArgs k{};
        k.xn = xn; k.w = w; k.cent = cent_in; k.part = (float*)ws; k.tickets = (unsigned*)tickets; k.cent_out = cent_out; k.den_out = den_out;
        k.L = L; k.b = b; k.tries = tries; k.w_mod_b = w_mod_b; k.beta = beta;
        const int slabs = ceil_div(L, LANES);
        int nG = 512 / R; if (nG < 1) nG = 1; if (nG > slabs) nG = slabs;
        if (nG > a.G) nG = a.G;                                 // the workspace holds a.G partial rows per row
        k.spw = ceil_div(slabs, nG); k.nG = ceil_div(slabs, k.spw);
        const dim3 grid(k.nG, R);
#define AMS_KSF(CC) do { if (w) hipLaunchKernelGGL((kmeans_soft_acc_kernel<CC, true>), grid, dim3(256), 0, st, k); \
                         else hipLaunchKernelGGL((kmeans_soft_acc_kernel<CC, false>), grid, dim3(256), 0, st, k); } while (0)
        if (C == 2) AMS_KSF(2); else if (C == 3) AMS_KSF(3); else if (C == 4) AMS_KSF(4); else if (C == 5) AMS_KSF(5); else AMS_KSF(6);
#undef AMS_KSF
        ams_status s2 = ams_check_launch();
        if (s2 != AMS_OK || tickets) return s2;
        hipLaunchKernelGGL(kmeans_reduce_kernel, dim3(ceil_div((long)R * C * E, 256)), dim3(256), 0, st, (const float*)ws, cent_out, den_out, R,
                           k.nG, C, E, 0);
        return ams_check_launch();
    }
    ams_status s;
    if (AMS_KM_GROUPED && beta < 0.f && C > 4 && (E == 40 || E == 8)) {
        s = launch_grouped<KmDense>(a, E, C, st);
    } else {
        s = beta < 0.f ? launch_pass<KmDense, HARD_ACC>(a, R, E, C, st) : launch_pass<KmDense, SOFT_ACC>(a, R, E, C, st);
    }
    if (s != AMS_OK || tickets) return s;
    hipLaunchKernelGGL(kmeans_reduce_kernel, dim3(ceil_div((long)R * C * E, 256)), dim3(256), 0, st, (const float*)ws, cent_out, den_out, R,
                       beta < 0.f ? 4 * a.G : a.G, C, E, 0);
    return ams_check_launch();
}

// Labels for `cent` (+ per-row inertia).  hard: labels int32 [R,L]; soft: soft [R,L,C].  Either output may be NULL.
ams_status ams_kmeans_assign(const float* xn, const float* w, const float* cent, int32_t* labels, float* soft, float* inertia, int b,
                             int tries, long L, int E, int C, float beta, int w_mod_b, void* ws, size_t ws_bytes, void* tickets, void* stream) {
    AMS_REQUIRE(xn && cent && ws && b > 0 && tries > 0 && L > 0 && C >= 2 && C <= 6);
    const int R = b * tries;
    if (ws_bytes < ams_kmeans_workspace_bytes(R, L, E, C)) return AMS_E_WORKSPACE_TOO_SMALL;
    hipStream_t st = (hipStream_t)stream;
    KmDense::Args a{};
    a.xn = xn; a.w = w; a.cent = cent; a.part = (float*)ws; a.labels = labels; a.soft = soft; a.L = L; a.b = b; a.tries = tries;
    const bool labels_only = beta < 0.f && !inertia && labels;
    a.G = ceil_div(L, chunk_of(beta >= 0.f || labels_only)); a.w_mod_b = w_mod_b; a.beta = beta; a.one = 1.0f;
    a.tickets = inertia ? (unsigned*)tickets : nullptr; a.fin_out = inertia; a.fin_den = nullptr;
    static const bool tries_kernel = [] { const char* e = getenv("AMS_KM_TRIES"); return !(e && e[0] == '0'); }();
    if (tries_kernel && beta < 0.f && inertia && E == 40 && C == 2 && tries % TQ == 0 && L * E * 4 < (1L << 31))   /* 32-bit buffer offsets */ {
        KtArgs k{};
        k.xn = xn; k.cent = cent; k.part = (float*)ws; k.tickets = (unsigned*)tickets; k.fin_out = inertia; k.labels = labels;
        k.L = L; k.b = b; k.tries = tries; k.G = a.G; k.w = w; k.w_mod_b = w_mod_b;
        if (w) hipLaunchKernelGGL((kmeans_hard_tries_final_kernel<KmDense, true>), dim3((unsigned)(b * (tries / TQ) * 2 * a.G)), dim3(640), 2 * 128 * 40 * sizeof(float), st, k);
        else hipLaunchKernelGGL((kmeans_hard_tries_final_kernel<KmDense, false>), dim3((unsigned)(b * (tries / TQ) * 2 * a.G)), dim3(640), 2 * 128 * 40 * sizeof(float), st, k);
        ams_status s2 = ams_check_launch();
        if (s2 != AMS_OK || tickets) return s2;
        hipLaunchKernelGGL(kmeans_reduce_kernel, dim3(ceil_div(R, 256)), dim3(256), 0, st, (const float*)ws, inertia, (float*)nullptr, R, 4 * a.G, C, E, 1);
        return ams_check_launch();
    }
    ams_status s = labels_only ? launch_pass<KmDense, HARD_LABELS>(a, R, E, C, st)
                 : beta < 0.f ? launch_pass<KmDense, HARD_FINAL>(a, R, E, C, st) : launch_pass<KmDense, SOFT_FINAL>(a, R, E, C, st);
    if (s != AMS_OK) return s;
    if (inertia && !tickets) {
        hipLaunchKernelGGL(kmeans_reduce_kernel, dim3(ceil_div(R, 256)), dim3(256), 0, st, (const float*)ws, inertia, (float*)nullptr, R, beta < 0.f ? 4 * a.G : a.G, C, E, 1);
        s = ams_check_launch();
    }
    return s;
}

// One backward pass of the unrolled soft k-means for b rows (the selected tries, already gathered by the caller):
ams_status ams_kmeans_select(const float* inertia, const float* centroids, int32_t* best, float* selected, int b, int tries, int E,
                             int C, void* stream) {
    AMS_REQUIRE(inertia && centroids && best && selected && b > 0 && tries > 0);
    hipLaunchKernelGGL(kmeans_select_kernel, dim3(b), dim3(64), 0, (hipStream_t)stream, inertia, centroids, best, selected, b, tries, C * E);
    return ams_check_launch();
}

}  // extern "C"
