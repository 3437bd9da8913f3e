// Deep-attractor reconstruction loss of the DANet-SCE separator (reference models/SC_V2.py:44-92), the term L41ModelV2 adds to the
// source-contrastive loss of csrc/l41.hip:
//   m[b,p,s]  = (y[b,p,s] + 1) / 2  (* [log10(max_p |X[b,:]| / |X[b,p]|) < thr] with --silence_loss)       a general float weight
//   A[b,s,e]  = sum_p V[b,p,e] m[b,p,s] / (1e-12 + sum_p m[b,p,s])                                          the attractors
//   a[b,p,s]  = sigmoid(<A[b,s,:], V[b,p,:]>)
//   cost      = mean_b mean_s mean_p (X_non_mix[b,p,s] - X_input[b,p] a[b,p,s])^2
// and its gradient w.r.t. V with den = 1e-12 + sum m, r = X_input a - X_non_mix, g = 2 r X_input a (1 - a) / (B S TF):
//   dA[b,s,e] = sum_p g[b,p,s] V[b,p,e],      dV[b,p,e] = sum_s ( g[b,p,s] A[b,s,e] + m[b,p,s] dA[b,s,e] / den[b,s] )
//
// Three passes, all HBM-bound, thread-per-point over 256-point blocks like csrc/l41.hip (16-byte pieces of V through LDS):
//   attractor pass       reads V once:  block partials of sum V m and sum m  -> danet_reduce_kernel -> A
//   reconstruction pass  reads V once:  cost partials; in a training step also g [B,TF,S] (S/E of V) and block partials of dA
//   backward pass        reads NO V:    dV from g, m (again from y), A, dA/den, times the upstream scalar; written, or ADDED to the
//                        gradient the source-contrastive backward left there (one read-modify-write, no temporary); optional max |dV|
// Every sum over the bins of an utterance is two-stage: a 256-point block adds its points in a fixed order (the (feature, part) walk of
// l41_kernel's dVs sums), one wave per output adds the blocks' partials (lane-strided, then a fixed tree).  No atomics: same inputs,
// same bits.  (The 8192-point chunk of the k-means passes would leave 192 workgroups at the bench shape; the 256-point block gives
// 5120 and is the unit the L41 loss already reduces over.)
#include "common.h"

namespace {

constexpr int MAXS = 4;
constexpr int MAXE = 40;

__device__ __forceinline__ float silence_weight(const float* __restrict__ xs, const float* __restrict__ xmax, int b, long idx, float thr) {
    if (xs == nullptr) return 1.0f;
    return (log10f(xmax[b] / fabsf(xs[idx])) < thr) ? 1.0f : 0.0f;       // as weight_masks_kernel (csrc/preproc.hip); 0/0 and x/0 -> 0
}

// max_p |X[b,p]| of every utterance (the silence mask's reference level): one workgroup per utterance
__global__ __launch_bounds__(256) void danet_xmax_kernel(const float* __restrict__ X, float* __restrict__ xmax, long TF) {
    __shared__ float sm[4];
    const float* xr = X + (long)blockIdx.x * TF;
    float mx = 0.f;
    for (long i = threadIdx.x; i < TF; i += 256) mx = fmaxf(mx, fabsf(xr[i]));
    mx = wave_max(mx);
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = mx;
    __syncthreads();
    if (threadIdx.x == 0) xmax[blockIdx.x] = fmaxf(fmaxf(sm[0], sm[1]), fmaxf(sm[2], sm[3]));
}

template <int E_, bool VEC>
__device__ __forceinline__ void load_tile(float* __restrict__ tile, const float* __restrict__ eb, int npts, int tid) {
    constexpr int LD = VEC ? E_ + 4 : E_ + 1;
    if constexpr (VEC) {
        constexpr int V4 = E_ / 4;
        const float4* src = reinterpret_cast<const float4*>(eb);
#pragma unroll
        for (int k = 0; k < V4; ++k) {
            const int i = tid + 256 * k, row = i / V4, c4 = i - row * V4;
            const float4 v4 = src[min(i, npts * V4 - 1)];                    // unconditional, clamped (rows past npts are never read back)
            *reinterpret_cast<float4*>(&tile[row * LD + c4 * 4]) = v4;
        }
    } else {
        for (int i = tid; i < npts * E_; i += 256) tile[(i / E_) * LD + (i % E_)] = eb[i];
    }
}

// out[s * E + e] = sum over the block's points of sw[p, s] * tile[p, e]: thread (feature e, part) adds its part's points one after
// another, the parts meet in part order (fixed order: deterministic).  Call with all 256 threads; sw rows are MAXS wide, zero past S / npts.
template <int E_, int LD>
__device__ __forceinline__ void block_outer_sum(const float* __restrict__ tile, const float* __restrict__ sw, float* __restrict__ red,
                                                int npts, int S, int tid, float* __restrict__ out) {
    constexpr int NPART = 256 / E_;
    const int eo = tid % E_, part = tid / E_;
    if (part < NPART) {
        const int per = (256 + NPART - 1) / NPART;
        const int pa = part * per, pb = min(npts, pa + per);
        float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
        for (int p = pa; p < pb; ++p) {
            const float vv = tile[p * LD + eo];
            const float4 w4 = *reinterpret_cast<const float4*>(&sw[p * MAXS]);
            a0 += w4.x * vv; a1 += w4.y * vv; a2 += w4.z * vv; a3 += w4.w * vv;
        }
        float* const r = &red[part * (MAXS * E_)];
        r[eo] = a0; r[E_ + eo] = a1; r[2 * E_ + eo] = a2; r[3 * E_ + eo] = a3;
    }
    __syncthreads();
    if (tid < S * E_) {
        float t = 0.f;
#pragma unroll
        for (int q = 0; q < NPART; ++q) t += red[q * (MAXS * E_) + tid];
        out[tid] = t;
    }
}

// attractor pass: num_part [B, nblk, S*E], den_part [B, nblk, S]
template <int E_, bool VEC>
__global__ __launch_bounds__(256) void danet_attr_kernel(const float* __restrict__ v, const float* __restrict__ y, const float* __restrict__ xs,
                                                         const float* __restrict__ xmax, float thr, float* __restrict__ num_part,
                                                         float* __restrict__ den_part, long TF, int S, int nblk) {
    constexpr int LD = VEC ? E_ + 4 : E_ + 1;
    __shared__ __attribute__((aligned(16))) float tile[256 * LD];
    __shared__ __attribute__((aligned(16))) float sw[256 * MAXS];
    __shared__ float red[(256 / E_) * MAXS * E_];
    __shared__ float sden[4 * MAXS];
    const int b = blockIdx.y, tid = threadIdx.x;
    const long p0 = (long)blockIdx.x * 256;
    const int npts = (int)min((long)256, TF - p0);
    load_tile<E_, VEC>(tile, v + ((long)b * TF + p0) * E_, npts, tid);
    float m[MAXS] = {0.f, 0.f, 0.f, 0.f};
    if (tid < npts) {
        const long idx = (long)b * TF + p0 + tid;
        const float w = 0.5f * silence_weight(xs, xmax, b, idx, thr);
        for (int s = 0; s < S; ++s) m[s] = (y[idx * S + s] + 1.0f) * w;
    }
#pragma unroll
    for (int s = 0; s < MAXS; ++s) {
        sw[tid * MAXS + s] = m[s];
        const float t = wave_sum(m[s]);
        if ((tid & 63) == 0) sden[(tid >> 6) * MAXS + s] = t;
    }
    __syncthreads();
    const long blk = (long)b * nblk + blockIdx.x;
    if (tid < S) den_part[blk * S + tid] = ((sden[tid] + sden[MAXS + tid]) + sden[2 * MAXS + tid]) + sden[3 * MAXS + tid];
    block_outer_sum<E_, LD>(tile, sw, red, npts, S, tid, num_part + blk * (S * E_));
}

// out[b, k] = sum over the blocks of part[b, :, k] / (1e-12 + sum over the blocks of den_part[b, :, k / E]): one WAVE per output, its
// lanes take the blocks c = lane, lane + 64, ... and meet in a fixed tree (l41_dvs_final_kernel's order)
__global__ void danet_reduce_kernel(const float* __restrict__ part, const float* __restrict__ den_part, float* __restrict__ out, int nblk,
                                    int E, int S, int B) {
    const int SE = S * E;
    const int i = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (i >= B * SE) return;
    const int b = i / SE, k = i - b * SE, s = k / E;
    float t = 0.f, d = 0.f;
    for (int c = lane; c < nblk; c += 64) {
        t += part[((long)b * nblk + c) * SE + k];
        d += den_part[((long)b * nblk + c) * S + s];
    }
    t = wave_sum(t);
    d = wave_sum(d);
    if (lane == 0) out[i] = t / (1e-12f + d);
}

// reconstruction pass.  x_non_mix element (b, p, s) lies at xnm[b * S * TF + s * xss + p * xps]
template <int E_, bool TRAIN, bool VEC>
__global__ __launch_bounds__(256) void danet_recon_kernel(const float* __restrict__ v, const float* __restrict__ attr,
                                                          const float* __restrict__ xin, const float* __restrict__ xnm, long xss, long xps,
                                                          float* __restrict__ cost_part, float* __restrict__ g, float* __restrict__ da_part,
                                                          long TF, int S, int nblk, float gscale) {
    constexpr int LD = VEC ? E_ + 4 : E_ + 1;
    __shared__ __attribute__((aligned(16))) float tile[256 * LD];
    __shared__ float sa[MAXS * E_];
    __shared__ __attribute__((aligned(16))) float sw[TRAIN ? 256 * MAXS : 4];
    __shared__ float red[TRAIN ? (256 / E_) * MAXS * E_ : 4];
    __shared__ float scost[4];
    const int b = blockIdx.y, tid = threadIdx.x;
    const long p0 = (long)blockIdx.x * 256;
    const int npts = (int)min((long)256, TF - p0);
    load_tile<E_, VEC>(tile, v + ((long)b * TF + p0) * E_, npts, tid);
    for (int i = tid; i < S * E_; i += 256) sa[i] = attr[(long)b * S * E_ + i];
    __syncthreads();
    float cost = 0.f;
    float gs[MAXS] = {0.f, 0.f, 0.f, 0.f};
    if (tid < npts) {
        float vv[E_];
#pragma unroll
        for (int e = 0; e < E_; ++e) vv[e] = tile[tid * LD + e];
        const long idx = (long)b * TF + p0 + tid;
        const float xi = xin[idx];
        const float* xn = xnm + (long)b * S * TF + (p0 + tid) * xps;
        for (int s = 0; s < S; ++s) {
            float z = 0.f;
#pragma unroll
            for (int e = 0; e < E_; ++e) z += vv[e] * sa[s * E_ + e];
            const float a = 1.0f / (1.0f + expf(-z));                      // z -> -inf: exp -> inf, a -> 0; z -> +inf: a -> 1; never NaN
            const float r = xi * a - xn[s * xss];
            cost += r * r;
            if (TRAIN) {
                gs[s] = 2.0f * gscale * r * xi * a * (1.0f - a);
                g[idx * S + s] = gs[s];
            }
        }
    }
    cost = wave_sum(cost);
    if ((tid & 63) == 0) scost[tid >> 6] = cost;
    if (TRAIN) {
#pragma unroll
        for (int s = 0; s < MAXS; ++s) sw[tid * MAXS + s] = gs[s];
    }
    __syncthreads();
    const long blk = (long)b * nblk + blockIdx.x;
    if (tid == 0) cost_part[blk] = ((scost[0] + scost[1]) + scost[2]) + scost[3];
    if constexpr (TRAIN) block_outer_sum<E_, LD>(tile, sw, red, npts, S, tid, da_part + blk * (S * E_));
}

__global__ __launch_bounds__(1024) void danet_cost_final_kernel(const float* __restrict__ part, float* __restrict__ out, long n, float scale) {
    __shared__ float sm[16];
    float s = 0.f;
    for (long i = threadIdx.x; i < n; i += blockDim.x) s += part[i];
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        float t = 0.f;
        for (int w = 0; w < (int)(blockDim.x >> 6); ++w) t += sm[w];
        out[0] = t * scale;
    }
}

// backward pass: dv[b,p,:] (+)= upstream * sum_s ( g[b,p,s] A[b,s,:] + m[b,p,s] dAd[b,s,:] ),  dAd = dA / den.  V is not read.
template <bool VEC, bool ACC>
__global__ __launch_bounds__(256) void danet_bwd_kernel(const float* __restrict__ y, const float* __restrict__ xs, const float* __restrict__ xmax,
                                                        float thr, const float* __restrict__ g, const float* __restrict__ attr,
                                                        const float* __restrict__ dattr, const float* __restrict__ upstream,
                                                        float* __restrict__ dv, float* __restrict__ amax_part, long TF, int E, int S, int nblk) {
    __shared__ __attribute__((aligned(16))) float sg[256 * MAXS];
    __shared__ __attribute__((aligned(16))) float sm[256 * MAXS];
    __shared__ __attribute__((aligned(16))) float sa[MAXS * MAXE];
    __shared__ __attribute__((aligned(16))) float sd[MAXS * MAXE];
    __shared__ float smax[4];
    const int b = blockIdx.y, tid = threadIdx.x;
    const long p0 = (long)blockIdx.x * 256;
    const int npts = (int)min((long)256, TF - p0);
    for (int i = tid; i < MAXS * E; i += 256) {
        sa[i] = i < S * E ? attr[(long)b * S * E + i] : 0.f;
        sd[i] = i < S * E ? dattr[(long)b * S * E + i] : 0.f;
    }
    {
        float gg[MAXS] = {0.f, 0.f, 0.f, 0.f}, mm[MAXS] = {0.f, 0.f, 0.f, 0.f};
        if (tid < npts) {
            const long idx = (long)b * TF + p0 + tid;
            const float up = upstream[0];
            const float w = 0.5f * silence_weight(xs, xmax, b, idx, thr) * up;
            for (int s = 0; s < S; ++s) {
                gg[s] = g[idx * S + s] * up;
                mm[s] = (y[idx * S + s] + 1.0f) * w;
            }
        }
#pragma unroll
        for (int s = 0; s < MAXS; ++s) { sg[tid * MAXS + s] = gg[s]; sm[tid * MAXS + s] = mm[s]; }
    }
    __syncthreads();
    float* db = dv + ((long)b * TF + p0) * E;
    float amx = 0.f;
    if constexpr (VEC) {
        const int V4 = E >> 2, n4 = npts * V4;
        float4* dst = reinterpret_cast<float4*>(db);
        for (int i = tid; i < n4; i += 256) {
            const int row = i / V4, c = (i - row * V4) * 4;
            const float4 g4 = *reinterpret_cast<const float4*>(&sg[row * MAXS]);
            const float4 m4 = *reinterpret_cast<const float4*>(&sm[row * MAXS]);
            const float gq[MAXS] = {g4.x, g4.y, g4.z, g4.w}, mq[MAXS] = {m4.x, m4.y, m4.z, m4.w};
            float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
            for (int s = 0; s < MAXS; ++s) {                                 // rows past S hold zeros
                const float4 a4 = *reinterpret_cast<const float4*>(&sa[s * E + c]);
                const float4 d4 = *reinterpret_cast<const float4*>(&sd[s * E + c]);
                acc.x += gq[s] * a4.x + mq[s] * d4.x;
                acc.y += gq[s] * a4.y + mq[s] * d4.y;
                acc.z += gq[s] * a4.z + mq[s] * d4.z;
                acc.w += gq[s] * a4.w + mq[s] * d4.w;
            }
            if (ACC) { const float4 o = dst[i]; acc.x += o.x; acc.y += o.y; acc.z += o.z; acc.w += o.w; }
            dst[i] = acc;
            amx = fmaxf(fmaxf(amx, fmaxf(fabsf(acc.x), fabsf(acc.y))), fmaxf(fabsf(acc.z), fabsf(acc.w)));
        }
    } else {
        for (int i = tid; i < npts * E; i += 256) {
            const int row = i / E, e = i - row * E;
            float acc = 0.f;
            for (int s = 0; s < S; ++s) acc += sg[row * MAXS + s] * sa[s * E + e] + sm[row * MAXS + s] * sd[s * E + e];
            if (ACC) acc += db[i];
            db[i] = acc;
            amx = fmaxf(amx, fabsf(acc));
        }
    }
    if (amax_part != nullptr) {
        amx = wave_max(amx);
        if ((tid & 63) == 0) smax[tid >> 6] = amx;
        __syncthreads();
        if (tid == 0) amax_part[(long)b * nblk + blockIdx.x] = fmaxf(fmaxf(smax[0], smax[1]), fmaxf(smax[2], smax[3]));
    }
}

__global__ __launch_bounds__(1024) void danet_amax_final_kernel(const float* __restrict__ part, float* __restrict__ out, long n) {
    __shared__ float sm[16];
    float m = 0.f;
    for (long i = threadIdx.x; i < n; i += blockDim.x) m = fmaxf(m, part[i]);
    m = wave_max(m);
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        float t = 0.f;
        for (int w = 0; w < (int)(blockDim.x >> 6); ++w) t = fmaxf(t, sm[w]);
        out[0] = t;
    }
}

struct Ws {
    float *xmax, *den_part, *part, *cost_part, *amax_part;
    size_t floats;
};

inline Ws danet_ws(void* ws, int B, long TF, int E, int S) {
    const size_t nb = (size_t)B * ceil_div(TF, 256);
    Ws w;
    w.xmax = (float*)ws;
    w.den_part = w.xmax + (((size_t)B + 3) & ~(size_t)3);
    w.part = w.den_part + nb * S;
    w.cost_part = w.part + nb * S * E;
    w.amax_part = w.cost_part + nb;
    w.floats = (size_t)(w.amax_part + nb - (float*)ws);
    return w;
}

inline bool danet_domain(int E, int S) {                                 // the (E, S) domain of ams_l41_loss_fwd
    return S > 0 && S <= MAXS && (E == 40 || E == 32 || E == 20 || E == 16 || E == 8 || E == 4 || E == 3);
}
inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" {

size_t ams_danet_workspace_bytes(int B, long TF, int E, int S) {
    if (B <= 0 || TF <= 0 || E <= 0 || S <= 0) return 0;
    return sizeof(float) * danet_ws(nullptr, B, TF, E, S).floats;
}

#define AMS_DANET_LAUNCH(K, ...) hipLaunchKernelGGL((K), grid, dim3(256), 0, st, __VA_ARGS__)
#define AMS_DANET_ATTR_E(EE, ...)                                                                     \
    if (EE % 4 == 0 && vec) AMS_DANET_LAUNCH((danet_attr_kernel<EE, (EE % 4 == 0)>), __VA_ARGS__);      \
    else AMS_DANET_LAUNCH((danet_attr_kernel<EE, false>), __VA_ARGS__);
#define AMS_DANET_RECON_E(EE, ...)                                                                                  \
    if (train) {                                                                                                    \
        if (EE % 4 == 0 && vec) AMS_DANET_LAUNCH((danet_recon_kernel<EE, true, (EE % 4 == 0)>), __VA_ARGS__);         \
        else AMS_DANET_LAUNCH((danet_recon_kernel<EE, true, false>), __VA_ARGS__);                                    \
    } else {                                                                                                        \
        if (EE % 4 == 0 && vec) AMS_DANET_LAUNCH((danet_recon_kernel<EE, false, (EE % 4 == 0)>), __VA_ARGS__);        \
        else AMS_DANET_LAUNCH((danet_recon_kernel<EE, false, false>), __VA_ARGS__);                                   \
    }
#define AMS_DANET_DISPATCH(WHICH, ...)              \
    switch (E) {                                    \
        case 40: { WHICH(40, __VA_ARGS__) } break;  \
        case 32: { WHICH(32, __VA_ARGS__) } break;  \
        case 20: { WHICH(20, __VA_ARGS__) } break;  \
        case 16: { WHICH(16, __VA_ARGS__) } break;  \
        case 8: { WHICH(8, __VA_ARGS__) } break;    \
        case 4: { WHICH(4, __VA_ARGS__) } break;    \
        case 3: { WHICH(3, __VA_ARGS__) } break;    \
        default: return AMS_E_INVALID_ARG;          \
    }

// v [B,TF,E] embeddings (NOT normalised: models/SC_V2.py:67), y [B,TF,S] masks (m = (y + 1) / 2), x_sil [B,TF] or NULL: the input the
// silence mask is taken from (with sil_thr), x_input [B,TF], x_non_mix [B,S,TF] (xnm_rows != 0: the rows the front / STFT writes) or
// [B,TF,S] -> cost[0], attr [B,S,E].  g [B,TF,S] and dattr [B,S,E] (both or neither): what ams_danet_recon_bwd needs; NULL = cost only.
ams_status ams_danet_recon_fwd(const float* v, const float* y, const float* x_sil, float sil_thr, const float* x_input, const float* x_non_mix,
                               int xnm_rows, float* cost, float* attr, float* g, float* dattr, int B, long TF, int E, int S, void* ws,
                               size_t ws_bytes, void* stream) {
    AMS_REQUIRE(v && y && x_input && x_non_mix && cost && attr && ws && B > 0 && TF > 0 && danet_domain(E, S));
    AMS_REQUIRE((g == nullptr) == (dattr == nullptr));
    if (ws_bytes < ams_danet_workspace_bytes(B, TF, E, S)) return AMS_E_WORKSPACE_TOO_SMALL;
    hipStream_t st = (hipStream_t)stream;
    const int nblk = ceil_div(TF, 256);
    const Ws w = danet_ws(ws, B, TF, E, S);
    dim3 grid(nblk, B);
    const bool vec = aligned16(v), train = g != nullptr;
    const float* xmax = nullptr;
    if (x_sil != nullptr) {
        hipLaunchKernelGGL(danet_xmax_kernel, dim3(B), dim3(256), 0, st, x_sil, w.xmax, TF);
        xmax = w.xmax;
    }
    AMS_DANET_DISPATCH(AMS_DANET_ATTR_E, v, y, x_sil, xmax, sil_thr, w.part, w.den_part, TF, S, nblk)
    const dim3 rgrid(ceil_div((long)B * S * E, 4));
    hipLaunchKernelGGL(danet_reduce_kernel, rgrid, dim3(256), 0, st, (const float*)w.part, (const float*)w.den_part, attr, nblk, E, S, B);
    const float scale = 1.0f / ((float)B * (float)TF * (float)S);
    const long xss = xnm_rows ? TF : 1, xps = xnm_rows ? 1 : S;
    AMS_DANET_DISPATCH(AMS_DANET_RECON_E, v, (const float*)attr, x_input, x_non_mix, xss, xps, w.cost_part, g, w.part, TF, S, nblk, scale)
    hipLaunchKernelGGL(danet_cost_final_kernel, dim3(1), dim3(1024), 0, st, (const float*)w.cost_part, cost, (long)B * nblk, scale);
    if (train)
        hipLaunchKernelGGL(danet_reduce_kernel, rgrid, dim3(256), 0, st, (const float*)w.part, (const float*)w.den_part, dattr, nblk, E, S, B);
    return ams_check_launch();
}

// dv [B,TF,E] = upstream[0] * d cost / d v, from what the forward left in g, attr, dattr (and m, again from y / x_sil / sil_thr: pass
// the forward's).  accumulate != 0: ADDED to what dv holds (the source-contrastive gradient of ams_l41_loss_bwd) instead of written.
// amax_out (optional): one float that receives max |dv| as the launch leaves it (see ams_l41_loss_bwd).
ams_status ams_danet_recon_bwd(const float* y, const float* x_sil, float sil_thr, const float* g, const float* attr, const float* dattr,
                               const float* upstream, float* dv, int accumulate, float* amax_out, int B, long TF, int E, int S, void* ws,
                               size_t ws_bytes, void* stream) {
    AMS_REQUIRE(y && g && attr && dattr && upstream && dv && ws && B > 0 && TF > 0 && danet_domain(E, S));
    if (ws_bytes < ams_danet_workspace_bytes(B, TF, E, S)) return AMS_E_WORKSPACE_TOO_SMALL;
    hipStream_t st = (hipStream_t)stream;
    const int nblk = ceil_div(TF, 256);
    const Ws w = danet_ws(ws, B, TF, E, S);
    dim3 grid(nblk, B);
    const bool vec = E % 4 == 0 && aligned16(dv);
    const float* xmax = nullptr;
    if (x_sil != nullptr) {
        hipLaunchKernelGGL(danet_xmax_kernel, dim3(B), dim3(256), 0, st, x_sil, w.xmax, TF);
        xmax = w.xmax;
    }
    float* const amax_part = amax_out ? w.amax_part : nullptr;
#define AMS_DANET_BWD(V, A) \
    AMS_DANET_LAUNCH((danet_bwd_kernel<V, A>), y, x_sil, xmax, sil_thr, g, attr, dattr, upstream, dv, amax_part, TF, E, S, nblk)
    if (vec) { if (accumulate) AMS_DANET_BWD(true, true); else AMS_DANET_BWD(true, false); }
    else { if (accumulate) AMS_DANET_BWD(false, true); else AMS_DANET_BWD(false, false); }
#undef AMS_DANET_BWD
    if (amax_out) hipLaunchKernelGGL(danet_amax_final_kernel, dim3(1), dim3(1024), 0, st, (const float*)amax_part, amax_out, (long)B * nblk);
    return ams_check_launch();
}

}  // extern "C"
