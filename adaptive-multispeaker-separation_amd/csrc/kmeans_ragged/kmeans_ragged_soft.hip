// Soft k-means over segments of different numbers of points (include/ams_kmeans_ragged_soft.h):
// libams_kmeans_ragged_soft.so.
//
// The passes have the form of kmeans_soft_acc_kernel (csrc/kmeans.hip): the row's centroids are wave-uniform loads through the constant
// address space (scalar operands of packed FMAs), d_c = w (|x|^2 - 2 <x, c> + |c|^2) clamped at 0, rows staged through LDS as 16-byte
// vectors, slab j + 1 requested while slab j is worked on.  What differs is the unit of work and the summation order: a workgroup reads
// (segment, chunk) from the host-built work table of ams_kmr_tables and the segment's own length, chunk count and place among the partial
// rows from p_off / g_off, and the order is the FIXED one of the header (chunks of 8192 points restarted at each segment), so a segment's
// sums see the same terms in the same order whatever its neighbours in the call are.  One launch per pass whatever the number of segments.
#include "../common.h"
#include "../../../include/ams_kmeans_ragged_soft.h"
#include <math.h>

thread_local int g_ams_last_hip_error = 0;      // (common.h: this library keeps its own)

namespace {

constexpr int KRS_CHUNK = 8192, KRS_LANES = 256, KRS_SLABS = KRS_CHUNK / KRS_LANES;

typedef float krs_f2 __attribute__((ext_vector_type(2)));
// wave-uniform loads through the CONSTANT address space are scalar loads.  Legal here: every centroid a kernel reads was written by an
// EARLIER launch (the previous pass's finishing workgroup included); the centroids a pass writes are read by later launches only
typedef const float __attribute__((address_space(4))) krs_cfloat;
typedef const krs_f2 __attribute__((address_space(4))) krs_cf2;

struct KrsArgs {
    const float* xn; const float* w; const int32_t* tab; const long* p_off; const long* g_off; const float* cent;
    float* part; unsigned* tickets; float* out;     // out: cent_out [R tries, C, E] | inertia [R tries] | masks [Ptot, C]
    int tries; float beta;
};

// where a workgroup works: chunk g of segment r (the first of the chunk's four table rows), its points and its row's partials
struct KrsUnit {
    int r, g, G, npc;          // segment, chunk, chunks of the segment, points of this chunk (1 .. 8192)
    long p0, g0;               // first point of the CHUNK in xn, first chunk of the segment among all chunks
};
__device__ __forceinline__ KrsUnit krs_unit(const KrsArgs& a, long u) {
    KrsUnit k;
    k.r = a.tab[16 * u];
    k.g = a.tab[16 * u + 1];
    const long s0 = a.p_off[k.r], P = a.p_off[k.r + 1] - s0;
    k.g0 = a.g_off[k.r];
    k.G = (int)(a.g_off[k.r + 1] - k.g0);
    k.p0 = s0 + (long)k.g * KRS_CHUNK;
    k.npc = (int)min((long)KRS_CHUNK, P - (long)k.g * KRS_CHUNK);
    return k;
}

// |c|^2 of the row's centroids (uniform: scalar operands)
template <int E_, int C_>
__device__ __forceinline__ void krs_cc(krs_cfloat* cen, float (&cc)[C_]) {
#pragma unroll
    for (int c = 0; c < C_; ++c) {
        float v = 0.f;
#pragma unroll
        for (int e = 0; e < E_; ++e) v = fmaf(cen[c * E_ + e], cen[c * E_ + e], v);
        cc[c] = v;
    }
}

// the soft labels of one point: d1_c = max(|x|^2 - 2 <x, c> + |c|^2, 0), lab_c = exp(-beta wv d1_c) / sum
template <int E_, int C_, bool HAS_W>
__device__ __forceinline__ void krs_labels(const krs_f2 (&x2)[E_ / 2], float xx, krs_cf2* cen2, const float (&cc)[C_], float wv, float beta,
                                           float (&lab)[C_], float (&d1)[C_]) {
    constexpr int H = E_ / 2;
    float sum = 0.f;
#pragma unroll
    for (int c = 0; c < C_; ++c) {
        krs_f2 sd = {0.f, 0.f};
#pragma unroll
        for (int q = 0; q < H; ++q) sd = __builtin_elementwise_fma(x2[q], (krs_f2)cen2[c * H + q], sd);
        d1[c] = fmaxf(xx - 2.0f * (sd[0] + sd[1]) + cc[c], 0.f);
        lab[c] = expf(-beta * (HAS_W ? d1[c] * wv : d1[c]));
        sum += lab[c];
    }
    const float inv = 1.0f / sum;
#pragma unroll
    for (int c = 0; c < C_; ++c) lab[c] *= inv;
}

// The slabs j0 .. j1 - 1 (256 points each) of a chunk of npc points at xc (weights at wc), through LDS as 16-byte vectors; slab j + 1 is
// requested into registers before slab j is worked on.  Every address is clamped inside the chunk's own npc rows (the short last slab of
// a segment reads nothing behind it); validity is applied at the LDS write.  body(j, npts, valid, x2, xx, wv) is called by EVERY thread
// (it may hold barriers); thread tid holds point 256 j + tid of the chunk, valid = tid < npts.  The caller makes sure j1 <= ceil(npc / 256).
template <int E_, bool HAS_W, typename F>
__device__ __forceinline__ void krs_slabs(const float* xc, const float* wc, int npc, int j0, int j1, float* buf, F&& body) {
    constexpr int LD = E_ + 4, V4 = E_ / 4, H = E_ / 2;
    static_assert(E_ % 4 == 0, "rows are staged as 16-byte vectors");
    const int tid = threadIdx.x;
    float4 pre[V4];
    float wpre = 1.0f;
    auto fetch = [&](int j) {
        const int q0 = j * KRS_LANES;
        const int lim = (npc - q0) * V4;                        // float4s of the chunk from this slab on: > 0 for a slab that exists
        const float4* src = reinterpret_cast<const float4*>(xc + (long)q0 * E_);
#pragma unroll
        for (int k = 0; k < V4; ++k) {
            const int i = tid + KRS_LANES * k;
            pre[k] = src[i < lim ? i : lim - 1];
        }
        if (HAS_W) wpre = wc[min(q0 + tid, npc - 1)];
    };
    if (j0 < j1) fetch(j0);
    for (int j = j0; j < j1; ++j) {
        const int npts = min(KRS_LANES, npc - j * KRS_LANES);
        __syncthreads();
#pragma unroll
        for (int k = 0; k < V4; ++k) {
            const int i = tid + KRS_LANES * k;
            const int row = i / V4, c4 = i - row * V4;
            *reinterpret_cast<float4*>(&buf[row * LD + c4 * 4]) = (i < npts * V4) ? pre[k] : make_float4(0.f, 0.f, 0.f, 0.f);
        }
        __syncthreads();
        const float wv = wpre;
        if (j + 1 < j1) fetch(j + 1);
        krs_f2 x2[H];
        krs_f2 xs = {0.f, 0.f};
#pragma unroll
        for (int q = 0; q < V4; ++q) {
            const float4 v = *reinterpret_cast<const float4*>(&buf[tid * LD + q * 4]);
            x2[2 * q] = (krs_f2){v.x, v.y}; x2[2 * q + 1] = (krs_f2){v.z, v.w};
            xs = __builtin_elementwise_fma(x2[2 * q], x2[2 * q], xs);
            xs = __builtin_elementwise_fma(x2[2 * q + 1], x2[2 * q + 1], xs);
        }
        body(j, npts, tid < npts, x2, xs[0] + xs[1], wv);
    }
}

// The workgroup's NV sums are in buf[wave NV + i] (four wave totals): store the chunk's partial (w0 + w1) + (w2 + w3), count the arrival
// and tell whether this workgroup stored the row's last partial.  Partials leave as agent-scope (write-through) stores and are read back
// the same way; the arrival is counted once every wave's stores are acknowledged.  The ticket is left zero for the next pass.
__device__ __forceinline__ bool krs_arrive(float* mypart, const float* buf, int NV, unsigned* ticket, int G, int* last_sh) {
    const int tid = threadIdx.x;
    for (int i = tid; i < NV; i += KRS_LANES)
        __hip_atomic_store(mypart + i, (buf[i] + buf[NV + i]) + (buf[2 * NV + i] + buf[3 * NV + i]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (tid == 0) {
        const int last = atomicAdd(ticket, 1u) == (unsigned)G - 1u;
        if (last) __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        *last_sh = last;
    }
    __syncthreads();
    return *last_sh != 0;
}

// One soft iteration.  grid Gtot tries (the tries of a chunk adjacent: they read the same points from L2), 256 threads.
template <int E_, int C_, bool HAS_W>
__global__ __launch_bounds__(256) void krs_acc_kernel(KrsArgs a) {
    constexpr int CE = C_ * E_, NV = CE + C_, LD = E_ + 4, H = E_ / 2;
    constexpr int BUF = 256 * LD > 4 * NV ? 256 * LD : 4 * NV;
    __shared__ __attribute__((aligned(16))) float buf[BUF];
    __shared__ int last_sh;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int t = (int)(blockIdx.x % (unsigned)a.tries);
    const KrsUnit u = krs_unit(a, (long)(blockIdx.x / (unsigned)a.tries));
    const long row = (long)u.r * a.tries + t;
    krs_cfloat* cen = (krs_cfloat*)(a.cent + row * CE);
    krs_cf2* cen2 = (krs_cf2*)cen;
    float cc[C_];
    krs_cc<E_, C_>(cen, cc);
    krs_f2 acc2[C_][H];
    float den[C_];
#pragma unroll
    for (int c = 0; c < C_; ++c) {
        den[c] = 0.f;
#pragma unroll
        for (int q = 0; q < H; ++q) acc2[c][q] = (krs_f2){0.f, 0.f};
    }
    krs_slabs<E_, HAS_W>(a.xn + u.p0 * E_, HAS_W ? a.w + u.p0 : nullptr, u.npc, 0, (u.npc + KRS_LANES - 1) / KRS_LANES, buf,
                         [&](int, int, bool valid, const krs_f2 (&x2)[H], float xx, float wv) {
        if (!valid) return;
        float lab[C_], d1[C_];
        krs_labels<E_, C_, HAS_W>(x2, xx, cen2, cc, wv, a.beta, lab, d1);
#pragma unroll
        for (int c = 0; c < C_; ++c) {
            const float wl = HAS_W ? wv * lab[c] : lab[c];
            const krs_f2 wl2 = {wl, wl};
#pragma unroll
            for (int q = 0; q < H; ++q) acc2[c][q] = __builtin_elementwise_fma(x2[q], wl2, acc2[c][q]);
            den[c] += lab[c];
        }
    });
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
    float* const prow = a.part + (u.g0 * a.tries + (long)t * u.G) * NV;          // the row's G partials, chunk after chunk
    if (!krs_arrive(prow + (long)u.g * NV, buf, NV, a.tickets + row, u.G, &last_sh) || tid >= CE) return;
    const int c = tid / E_;
    float num = 0.f, dn = 0.f;
    for (int q = 0; q < u.G; ++q) {
        num += __hip_atomic_load(prow + (long)q * NV + tid, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        dn += __hip_atomic_load(prow + (long)q * NV + CE + c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    a.out[row * CE + tid] = num / dn;
}

// The inertia of every row: labels with w, distances without.  The same grid and order; 2 C sums per workgroup.
template <int E_, int C_, bool HAS_W>
__global__ __launch_bounds__(256) void krs_inertia_kernel(KrsArgs a) {
    constexpr int CE = C_ * E_, NV = 2 * C_, LD = E_ + 4, H = E_ / 2;
    __shared__ __attribute__((aligned(16))) float buf[256 * LD];
    __shared__ int last_sh;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int t = (int)(blockIdx.x % (unsigned)a.tries);
    const KrsUnit u = krs_unit(a, (long)(blockIdx.x / (unsigned)a.tries));
    const long row = (long)u.r * a.tries + t;
    krs_cfloat* cen = (krs_cfloat*)(a.cent + row * CE);
    krs_cf2* cen2 = (krs_cf2*)cen;
    float cc[C_];
    krs_cc<E_, C_>(cen, cc);
    float num[C_], den[C_];
#pragma unroll
    for (int c = 0; c < C_; ++c) num[c] = den[c] = 0.f;
    krs_slabs<E_, HAS_W>(a.xn + u.p0 * E_, HAS_W ? a.w + u.p0 : nullptr, u.npc, 0, (u.npc + KRS_LANES - 1) / KRS_LANES, buf,
                         [&](int, int, bool valid, const krs_f2 (&x2)[H], float xx, float wv) {
        if (!valid) return;
        float lab[C_], d1[C_];
        krs_labels<E_, C_, HAS_W>(x2, xx, cen2, cc, wv, a.beta, lab, d1);
#pragma unroll
        for (int c = 0; c < C_; ++c) { num[c] = fmaf(d1[c], lab[c], num[c]); den[c] += lab[c]; }
    });
    __syncthreads();
#pragma unroll
    for (int c = 0; c < C_; ++c) {
        const float vn = wave_sum_lane0(num[c]), vd = wave_sum_lane0(den[c]);
        if (lane == 0) { buf[wave * NV + c] = vn; buf[wave * NV + C_ + c] = vd; }
    }
    __syncthreads();
    float* const prow = a.part + (u.g0 * a.tries + (long)t * u.G) * NV;
    if (!krs_arrive(prow + (long)u.g * NV, buf, NV, a.tickets + row, u.G, &last_sh) || tid != 0) return;
    float tot = 0.f;
#pragma unroll
    for (int c = 0; c < C_; ++c) {
        float sn = 0.f, sd = 0.f;
        for (int q = 0; q < u.G; ++q) {
            sn += __hip_atomic_load(prow + (long)q * NV + c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            sd += __hip_atomic_load(prow + (long)q * NV + C_ + c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        tot += sn / sd;
    }
    a.out[row] = tot;
}

// masks [Ptot, C] for one centroid set per segment: a pure stream (E 4 bytes read, C 4 bytes written per point).  grid 4 Gtot: a
// workgroup takes eight slabs of a chunk (nothing is summed, so the split is free).  The labels of a slab meet in LDS and leave as one
// contiguous run of npts C floats.
template <int E_, int C_, bool HAS_W>
__global__ __launch_bounds__(256) void krs_masks_kernel(KrsArgs a) {
    constexpr int CE = C_ * E_, LD = E_ + 4, H = E_ / 2, Q = KRS_SLABS / 4;
    __shared__ __attribute__((aligned(16))) float buf[256 * LD];
    const int tid = threadIdx.x;
    const KrsUnit u = krs_unit(a, (long)(blockIdx.x >> 2));
    const int nsl = (u.npc + KRS_LANES - 1) / KRS_LANES, j0 = (int)(blockIdx.x & 3) * Q;
    if (j0 >= nsl) return;                                      // (workgroup-uniform)
    krs_cfloat* cen = (krs_cfloat*)(a.cent + (long)u.r * CE);
    krs_cf2* cen2 = (krs_cf2*)cen;
    float cc[C_];
    krs_cc<E_, C_>(cen, cc);
    float* const mc = a.out + u.p0 * C_;
    krs_slabs<E_, HAS_W>(a.xn + u.p0 * E_, HAS_W ? a.w + u.p0 : nullptr, u.npc, j0, min(j0 + Q, nsl), buf,
                         [&](int j, int npts, bool, const krs_f2 (&x2)[H], float xx, float wv) {
        float lab[C_], d1[C_];
        krs_labels<E_, C_, HAS_W>(x2, xx, cen2, cc, wv, a.beta, lab, d1);      // (a lane without a point works on a zero row)
        __syncthreads();                                        // every lane has read its row
#pragma unroll
        for (int c = 0; c < C_; ++c) buf[tid * C_ + c] = lab[c];
        __syncthreads();
        float* const dst = mc + (long)j * KRS_LANES * C_;
        for (int i = tid; i < npts * C_; i += KRS_LANES) dst[i] = buf[i];
    });
}

// centroids[r, c, :] = xn[p_off[r / tries] + idx[r, c], :]
__global__ void krs_init_kernel(const float* __restrict__ xn, const long* __restrict__ p_off, const int32_t* __restrict__ idx,
                                float* __restrict__ cent, long n, int C, int E, int tries) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int e = (int)(i % E);
    const long rc = i / E;
    const long r = rc / C;
    cent[i] = xn[(p_off[r / tries] + idx[rc]) * E + e];
}

// best[r] = the first minimum of inertia[r tries ..], the first NaN if there is one (np.argmin; kmeans_select_kernel of csrc/kmeans.hip)
__global__ void krs_select_kernel(const float* __restrict__ inertia, const float* __restrict__ cent, int32_t* __restrict__ best,
                                  float* __restrict__ sel, int R, int tries, int CE) {
    const int r = blockIdx.x;
    if (r >= R) return;
    int bt = 0;
    float bv = inertia[(long)r * tries];
    for (int t = 1; t < tries; ++t) {
        const float v = inertia[(long)r * tries + t];
        if (bv == bv && !(bv <= v)) { bv = v; bt = t; }
    }
    if (threadIdx.x == 0) best[r] = bt;
    for (int i = threadIdx.x; i < CE; i += blockDim.x) sel[(long)r * CE + i] = cent[((long)r * tries + bt) * CE + i];
}

bool krs_pair(int E, int C) { return (E == 40 || E == 8) && C >= 2 && C <= 6; }
bool krs_sizes(int R, int tries, long Gtot) { return R >= 1 && tries >= 1 && Gtot >= R && 4 * Gtot * (long)tries < (1L << 31); }
bool krs_beta(float beta) { return isfinite(beta) && beta >= 0.f; }
bool krs_aligned(const void* p) { return ((uintptr_t)p & 15) == 0; }

// one launch of KERNEL<E, C, HAS_W> for the pair (E, C)
#define AMS_KRS_ARM(KERNEL, EE, CC) do { if (a.w) hipLaunchKernelGGL((KERNEL<EE, CC, true>), grid, dim3(256), 0, st, a); \
                                         else hipLaunchKernelGGL((KERNEL<EE, CC, false>), grid, dim3(256), 0, st, a); } while (0)
#define AMS_KRS_LAUNCH(KERNEL) do { \
        if (E == 40) { if (C == 2) AMS_KRS_ARM(KERNEL, 40, 2); else if (C == 3) AMS_KRS_ARM(KERNEL, 40, 3); else if (C == 4) AMS_KRS_ARM(KERNEL, 40, 4); \
                       else if (C == 5) AMS_KRS_ARM(KERNEL, 40, 5); else AMS_KRS_ARM(KERNEL, 40, 6); } \
        else { if (C == 2) AMS_KRS_ARM(KERNEL, 8, 2); else if (C == 3) AMS_KRS_ARM(KERNEL, 8, 3); else if (C == 4) AMS_KRS_ARM(KERNEL, 8, 4); \
               else if (C == 5) AMS_KRS_ARM(KERNEL, 8, 5); else AMS_KRS_ARM(KERNEL, 8, 6); } } while (0)

}  // namespace

extern "C" {

int ams_kmrs_abi_version(void) { return 1; }

size_t ams_kmrs_workspace_bytes(int R, int tries, long Gtot, int E, int C) {
    if (!krs_pair(E, C) || !krs_sizes(R, tries, Gtot)) return 0;
    return sizeof(float) * (size_t)tries * (size_t)Gtot * C * (E + 1);
}

ams_status ams_kmrs_init(const float* xn, const int64_t* p_off, const int32_t* init_idx, float* centroids, int R, int tries, int E, int C,
                         void* stream) {
    AMS_REQUIRE(xn && p_off && init_idx && centroids && R >= 1 && tries >= 1 && krs_pair(E, C));
    const long n = (long)R * tries * C * E;
    AMS_REQUIRE(n < (1L << 31) * 256);
    hipLaunchKernelGGL(krs_init_kernel, dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, (hipStream_t)stream, xn, (const long*)p_off,
                       init_idx, centroids, n, C, E, tries);
    return ams_check_launch();
}

ams_status ams_kmrs_iterate(const float* xn, const float* w, const int32_t* tab, const int64_t* p_off, const int64_t* g_off,
                            const float* cent_in, float* cent_out, int R, int tries, long Gtot, int E, int C, float beta, void* ws,
                            size_t ws_bytes, void* tickets, void* stream) {
    AMS_REQUIRE(xn && tab && p_off && g_off && cent_in && cent_out && cent_in != cent_out && ws && tickets && krs_pair(E, C) &&
                krs_sizes(R, tries, Gtot) && krs_beta(beta) && krs_aligned(xn));
    if (ws_bytes < ams_kmrs_workspace_bytes(R, tries, Gtot, E, C)) return AMS_E_WORKSPACE_TOO_SMALL;
    hipStream_t st = (hipStream_t)stream;
    KrsArgs a{};
    a.xn = xn; a.w = w; a.tab = tab; a.p_off = (const long*)p_off; a.g_off = (const long*)g_off; a.cent = cent_in;
    a.part = (float*)ws; a.tickets = (unsigned*)tickets; a.out = cent_out; a.tries = tries; a.beta = beta;
    const dim3 grid((unsigned)(Gtot * tries));
    AMS_KRS_LAUNCH(krs_acc_kernel);
    return ams_check_launch();
}

ams_status ams_kmrs_inertia(const float* xn, const float* w, const int32_t* tab, const int64_t* p_off, const int64_t* g_off,
                            const float* cent, float* inertia, int R, int tries, long Gtot, int E, int C, float beta, void* ws,
                            size_t ws_bytes, void* tickets, void* stream) {
    AMS_REQUIRE(xn && tab && p_off && g_off && cent && inertia && ws && tickets && krs_pair(E, C) && krs_sizes(R, tries, Gtot) &&
                krs_beta(beta) && krs_aligned(xn));
    if (ws_bytes < ams_kmrs_workspace_bytes(R, tries, Gtot, E, C)) return AMS_E_WORKSPACE_TOO_SMALL;
    hipStream_t st = (hipStream_t)stream;
    KrsArgs a{};
    a.xn = xn; a.w = w; a.tab = tab; a.p_off = (const long*)p_off; a.g_off = (const long*)g_off; a.cent = cent;
    a.part = (float*)ws; a.tickets = (unsigned*)tickets; a.out = inertia; a.tries = tries; a.beta = beta;
    const dim3 grid((unsigned)(Gtot * tries));
    AMS_KRS_LAUNCH(krs_inertia_kernel);
    return ams_check_launch();
}

ams_status ams_kmrs_select(const float* inertia, const float* centroids, int32_t* best, float* selected, int R, int tries, int E, int C,
                           void* stream) {
    AMS_REQUIRE(inertia && centroids && best && selected && R >= 1 && tries >= 1 && krs_pair(E, C));
    hipLaunchKernelGGL(krs_select_kernel, dim3(R), dim3(64), 0, (hipStream_t)stream, inertia, centroids, best, selected, R, tries, C * E);
    return ams_check_launch();
}

ams_status ams_kmrs_masks(const float* xn, const float* w, const int32_t* tab, const int64_t* p_off, const int64_t* g_off,
                          const float* cent, float beta, float* masks, int R, long Gtot, int E, int C, void* stream) {
    AMS_REQUIRE(xn && tab && p_off && g_off && cent && masks && krs_pair(E, C) && krs_sizes(R, 1, Gtot) && krs_beta(beta) && krs_aligned(xn));
    hipStream_t st = (hipStream_t)stream;
    KrsArgs a{};
    a.xn = xn; a.w = w; a.tab = tab; a.p_off = (const long*)p_off; a.g_off = (const long*)g_off; a.cent = cent;
    a.out = masks; a.tries = 1; a.beta = beta;
    const dim3 grid((unsigned)(4 * Gtot));
    AMS_KRS_LAUNCH(krs_masks_kernel);
    return ams_check_launch();
}

}  // extern "C"
