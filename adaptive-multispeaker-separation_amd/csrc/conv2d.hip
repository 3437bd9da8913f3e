// The dilated 2-D convolution stack (reference models/network.py:528-551): tf.contrib.layers.conv2d, stride 1, SAME, atrous rate
// [rt, rf], bias, ReLU.  Activations are NHWC [B, T, F, C] (pixel p = (b T + t) F + f, channels fastest), weights HWIO
// [kh, kw, cin, cout] = [K, cout] with k = tap cin + ci, tap = i kw + j, tap (i, j) at offset ((i - (kh-1)/2) rt, (j - (kw-1)/2) rf).
//
// Three shape classes:
//   cin, cout >= 4 (layers 2-12, and the dX of layer 13): IMPLICIT GEMMs on the product kernel of csrc/gemm.hip (A_CONV / A_CONV_T
//     loaders, no im2col image: C % 4 == 0, so a float4 of a k-tile lies inside one tap and is all signal or all padding), in its
//     arithmetic classes (fp16x3 with both bounds, bf16x6, native f32 under ams_gemm_set_arith(0)):
//       forward  y  = relu(A_CONV(x) . W + b)                      bias + ReLU in the product's epilogue, max |y| folded by it
//       dX       dx = A_CONV(dy, mirrored taps) . W^T * (y_below > 0)   the mask of the layer below in the epilogue, max |dx| folded
//       dW, db   dW = A_CONV_T(x) . dy, db = colsum(dy)            deterministic split-K slabs, column sums from the same pass
//   cin == 1 (layer 1): a direct forward kernel (7 taps per output); dW / db from an 8-column image (taps padded to 8) and the
//     product -- 32 bytes per pixel, no dX (its input is data).
//   cout == 4 (layer 13): direct kernels for the forward (weights in LDS, one pixel per thread) and for dW / db (one workgroup per
//     tap and pixel slab, partial sums added in slab order), f32 FMA: a 128-wide product tile would be 97 % padding.
// No floating-point atomics: the folded bounds are atomicMax of the bit patterns of non-negative floats (order-independent), so two
// launches give the same bits.  As in the product kernels, fmaxf drops a NaN from a folded bound: a NaN reaches the caller through
// the output itself.
#include "common.h"
#include <algorithm>

namespace {

struct Geo {
    int B, T, F, cin, cout, kh, kw, rt, rf;
    long M() const { return long(B) * T * F; }
    int taps() const { return kh * kw; }
};

inline int log2_exact(int c) {
    int l = 0;
    while ((1 << l) < c) ++l;
    return (1 << l) == c ? l : -1;
}

inline bool geo_ok(const Geo& g) {
    return g.B > 0 && g.T > 0 && g.F > 0 && g.T < 65536 && g.F < 65536 && g.cin > 0 && g.cout > 0 && g.kh > 0 && g.kw > 0 &&
           (g.kh & 1) && (g.kw & 1) && g.rt > 0 && g.rf > 0 && (g.cout % 4 == 0) && log2_exact(g.cout) >= 2 &&
           (g.cin == 1 || log2_exact(g.cin) >= 2) && g.M() * std::max(g.cin, g.cout) < (1L << 31);
}

constexpr int SKINNY_SLABS = 1024;                     // pixel slabs of the cout == 4 weight gradient

inline size_t al256(size_t n) { return (n + 255) & ~size_t(255); }

// workspace: [A (image of layer 1 / slabs of the skinny dW) | product split-K slabs | 32 cout floats of colsum scratch | padded weights]
struct Ws {
    size_t a, slabs, bsum, wpad, total;
};

Ws ws_layout(const Geo& g) {
    Ws w{};
    const long M = g.M();
    const int K = g.taps() * g.cin;
    if (g.cin == 1) {
        w.a = al256(size_t(M) * 8 * 4);
        w.slabs = al256(ams_gemm_workspace_bytes(8, g.cout, int(M), 1, 0));
        w.wpad = al256(size_t(8) * g.cout * 4);
    } else if (g.cout == 4) {
        w.a = al256(size_t(SKINNY_SLABS) * (size_t(K) * 4 + 4) * 4);
    } else {
        w.slabs = al256(ams_detail::conv_wgrad_ws_bytes(int(M), g.cout, K));
    }
    w.bsum = al256(size_t(32) * g.cout * 4);
    w.total = w.a + w.slabs + w.bsum + w.wpad;
    return w;
}

__device__ __forceinline__ void fold_amax(float m, unsigned* amax) {
    __shared__ float sm[16];
    m = wave_max(m);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, nw = blockDim.x >> 6;
    if (lane == 0) sm[wv] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        float t = 0.f;
        for (int i = 0; i < nw; ++i) t = fmaxf(t, sm[i]);
        atomicMax(amax, __float_as_uint(t));
    }
}

// layer 1 (cin == 1): y[p, co..co+3] = relu(b + sum_tap x[p + off(tap)] w[tap, co..co+3]); one float4 of outputs per thread
__global__ __launch_bounds__(256) void conv_c1_fwd_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                          const float* __restrict__ bias, float* __restrict__ y, long M, int T, int F,
                                                          int cout, int kh, int kw, int rt, int rf, unsigned* __restrict__ amax) {
    const int c4 = cout >> 2, taps = kh * kw;
    const long n = M * c4;
    float m = 0.f;
    for (long i = blockIdx.x * long(blockDim.x) + threadIdx.x; i < n; i += long(gridDim.x) * blockDim.x) {
        const int co = int(i % c4) * 4;
        const long p = i / c4;
        const int f = int(p % F);
        const int t = int((p / F) % T);
        f32x4 acc = *reinterpret_cast<const f32x4*>(bias + co);
        for (int tap = 0; tap < taps; ++tap) {
            const int dt = (tap / kw - (kh - 1) / 2) * rt, df = (tap % kw - (kw - 1) / 2) * rf;
            if (t + dt < 0 || t + dt >= T || f + df < 0 || f + df >= F) continue;
            const float xv = x[p + long(dt) * F + df];
            const f32x4 wv = *reinterpret_cast<const f32x4*>(w + long(tap) * cout + co);
            acc += xv * wv;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[j] = acc[j] > 0.f ? acc[j] : 0.f;
        *reinterpret_cast<f32x4*>(y + p * cout + co) = acc;
        m = fmaxf(m, fmaxf(fmaxf(acc[0], acc[1]), fmaxf(acc[2], acc[3])));
    }
    if (amax) fold_amax(m, amax);
}

// layer 1 weight gradient operand: col[p, tap] = x[p + off(tap)] (0 outside), taps padded to 8 columns
__global__ void im2col_c1_kernel(const float* __restrict__ src, float* __restrict__ col, long M, int T, int F, int kh, int kw, int rt,
                                 int rf) {
    const int taps = kh * kw;
    const long n = M * 8;
    for (long i = blockIdx.x * long(blockDim.x) + threadIdx.x; i < n; i += long(gridDim.x) * blockDim.x) {
        const int tap = int(i & 7);
        const long p = i >> 3;
        float v = 0.f;
        if (tap < taps) {
            const int f = int(p % F);
            const int t = int((p / F) % T);
            const int dt = (tap / kw - (kh - 1) / 2) * rt, df = (tap % kw - (kw - 1) / 2) * rf;
            if (t + dt >= 0 && t + dt < T && f + df >= 0 && f + df < F) v = src[p + long(dt) * F + df];
        }
        col[i] = v;
    }
}

// cout == 4: y[p, 0..3] = relu(b + sum_{tap, c} x[p + off(tap), c] w[tap, c, 0..3]); weights in LDS, one pixel per thread
__global__ __launch_bounds__(256) void conv_o4_fwd_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                          const float* __restrict__ bias, float* __restrict__ y, long M, int T, int F,
                                                          int C, int kh, int kw, int rt, int rf, unsigned* __restrict__ amax) {
    extern __shared__ f32x4 wl[];                      // [taps C] rows of the 4 outputs
    const int taps = kh * kw;
    for (int i = threadIdx.x; i < taps * C; i += blockDim.x) wl[i] = reinterpret_cast<const f32x4*>(w)[i];
    __syncthreads();
    const f32x4 b = *reinterpret_cast<const f32x4*>(bias);
    float m = 0.f;
    for (long p = blockIdx.x * long(blockDim.x) + threadIdx.x; p < M; p += long(gridDim.x) * blockDim.x) {
        const int f = int(p % F);
        const int t = int((p / F) % T);
        f32x4 acc = b;
        for (int tap = 0; tap < taps; ++tap) {
            const int dt = (tap / kw - (kh - 1) / 2) * rt, df = (tap % kw - (kw - 1) / 2) * rf;
            if (t + dt < 0 || t + dt >= T || f + df < 0 || f + df >= F) continue;
            const f32x4* xs = reinterpret_cast<const f32x4*>(x + (p + long(dt) * F + df) * C);
            const f32x4* ws = wl + tap * C;
            for (int c4 = 0; c4 < (C >> 2); ++c4) {
                const f32x4 xv = xs[c4];
                acc += xv[0] * ws[4 * c4] + xv[1] * ws[4 * c4 + 1] + xv[2] * ws[4 * c4 + 2] + xv[3] * ws[4 * c4 + 3];
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[j] = acc[j] > 0.f ? acc[j] : 0.f;
        *reinterpret_cast<f32x4*>(y + p * 4) = acc;
        m = fmaxf(m, fmaxf(fmaxf(acc[0], acc[1]), fmaxf(acc[2], acc[3])));
    }
    if (amax) fold_amax(m, amax);
}

// cout == 4 weight gradient, partial sums: workgroup (tap, slab), thread c: part[slab][(tap C + c) 4 + o] = sum over the slab's pixels p
// of x[p + off(tap), c] dy[p, o]; the tap-0 workgroups' threads 0..3 also leave part[slab][taps C 4 + o] = sum_p dy[p, o]
__global__ void conv_o4_wgrad_kernel(const float* __restrict__ x, const float* __restrict__ dy, float* __restrict__ part, long M, int T,
                                     int F, int C, int kh, int kw, int rt, int rf, long per_slab) {
    const int tap = blockIdx.x, slab = blockIdx.y, taps = kh * kw;
    const long row = long(taps) * C * 4 + 4;
    const long p0 = slab * per_slab, p1 = min(M, p0 + per_slab);
    const int dt = (tap / kw - (kh - 1) / 2) * rt, df = (tap % kw - (kw - 1) / 2) * rf;
    for (int c = threadIdx.x; c < C; c += blockDim.x) {
        f32x4 acc = {0.f, 0.f, 0.f, 0.f}, db = {0.f, 0.f, 0.f, 0.f};
        const bool wdb = tap == 0 && c == 0;
        for (long p = p0; p < p1; ++p) {
            const f32x4 d = reinterpret_cast<const f32x4*>(dy)[p];
            if (wdb) db += d;
            const int f = int(p % F);
            const int t = int((p / F) % T);
            if (t + dt < 0 || t + dt >= T || f + df < 0 || f + df >= F) continue;
            acc += x[(p + long(dt) * F + df) * C + c] * d;
        }
        *reinterpret_cast<f32x4*>(part + slab * row + (long(tap) * C + c) * 4) = acc;
        if (wdb) *reinterpret_cast<f32x4*>(part + slab * row + long(taps) * C * 4) = db;
    }
}

// out[i] = sum_s part[s][i] in slab order, i < row (row % 4 == 0): dw = out[0 .. row-4), db = out[row-4 ..)
__global__ void slab_sum_kernel(const float* __restrict__ part, float* __restrict__ dw, float* __restrict__ db, long row, int slabs) {
    const long n4 = row / 4;
    for (long i = blockIdx.x * long(blockDim.x) + threadIdx.x; i < n4; i += long(gridDim.x) * blockDim.x) {
        f32x4 s = {0.f, 0.f, 0.f, 0.f};
        for (int k = 0; k < slabs; ++k) s += reinterpret_cast<const f32x4*>(part + k * row)[i];
        if (i < n4 - 1) reinterpret_cast<f32x4*>(dw)[i] = s;
        else *reinterpret_cast<f32x4*>(db) = s;
    }
}

// dst[i] = src[i] * (mask[i] > 0), n % 4 == 0; amax (optional) receives max |dst|
__global__ void relu_mask_kernel(const float* src, float* dst, const float* __restrict__ mask, long n4, unsigned* __restrict__ amax) {
    float m = 0.f;
    for (long i = blockIdx.x * long(blockDim.x) + threadIdx.x; i < n4; i += long(gridDim.x) * blockDim.x) {
        f32x4 v = reinterpret_cast<const f32x4*>(src)[i];
        const f32x4 k = reinterpret_cast<const f32x4*>(mask)[i];
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = k[j] > 0.f ? v[j] : 0.f;
        reinterpret_cast<f32x4*>(dst)[i] = v;
#pragma unroll
        for (int j = 0; j < 4; ++j) m = fmaxf(m, fabsf(v[j]));
    }
    if (amax) fold_amax(m, amax);
}

// wt[(tap, co), ci] = w[(tap, ci), co]: the weights of the dX product (W^T per tap)
__global__ void wt_kernel(const float* __restrict__ w, float* __restrict__ wt, int taps, int cin, int cout) {
    const long n = long(taps) * cin * cout;
    for (long i = blockIdx.x * long(blockDim.x) + threadIdx.x; i < n; i += long(gridDim.x) * blockDim.x) {
        const int ci = int(i % cin);
        const long tc = i / cin;
        const int co = int(tc % cout), tap = int(tc / cout);
        wt[i] = w[(long(tap) * cin + ci) * cout + co];
    }
}

inline int grid_for(long n, int per_block = 256) { return int(std::min<long>((n + per_block - 1) / per_block, 8192)); }

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

extern "C" {

size_t ams_dilated_conv2d_workspace_bytes(int B, int T, int F, int cin, int cout, int kh, int kw) {
    const Geo g{B, T, F, cin, cout, kh, kw, 1, 1};
    if (!geo_ok(g)) return 0;
    const size_t wt = al256(size_t(kh) * kw * cin * cout * 4);      // the dX launch: W^T per tap
    return std::max(ws_layout(g).total, wt);
}

ams_status ams_dilated_conv2d_fwd(const float* x, const float* w, const float* bias, float* y, int B, int T, int F, int cin, int cout,
                                  int kh, int kw, int rt, int rf, const float* amax_x, const float* amax_w, float* amax_y, void* ws,
                                  size_t ws_bytes, void* stream) {
    const Geo g{B, T, F, cin, cout, kh, kw, rt, rf};
    AMS_REQUIRE(geo_ok(g) && x && w && bias && y);
    AMS_REQUIRE(aligned16(x) && aligned16(w) && aligned16(bias) && aligned16(y));
    (void)ws; (void)ws_bytes;                           // the forward needs no workspace (kept for one signature across the three)
    hipStream_t st = (hipStream_t)stream;
    const long M = g.M();
    if (cin == 1 || cout == 4) {
        if (amax_y && hipMemsetAsync(amax_y, 0, sizeof(float), st) != hipSuccess) return ams_check_launch();
        unsigned* am = reinterpret_cast<unsigned*>(amax_y);
        if (cin == 1) {
            conv_c1_fwd_kernel<<<grid_for(M * (cout / 4)), 256, 0, st>>>(x, w, bias, y, M, T, F, cout, kh, kw, rt, rf, am);
        } else {
            const size_t lds = size_t(g.taps()) * cin * 16;
            if (lds > 64 * 1024) return AMS_E_INVALID_ARG;
            conv_o4_fwd_kernel<<<grid_for(M), 256, lds, st>>>(x, w, bias, y, M, T, F, cin, kh, kw, rt, rf, am);
        }
        return ams_check_launch();
    }
    return ams_detail::conv_fwd_or_dx(x, w, bias, y, int(M), cout, T, F, log2_exact(cin), kh, kw, rt, rf, 1, nullptr, amax_x, amax_w,
                                      amax_y, st);
}

ams_status ams_dilated_conv2d_bwd_data(const float* dy, const float* w, const float* y_below, float* dx, int B, int T, int F, int cin,
                                       int cout, int kh, int kw, int rt, int rf, const float* amax_dy, const float* amax_w,
                                       float* amax_dx, void* ws, size_t ws_bytes, void* stream) {
    const Geo g{B, T, F, cin, cout, kh, kw, rt, rf};
    AMS_REQUIRE(geo_ok(g) && cin % 4 == 0 && dy && w && dx && ws && (!amax_dx || y_below));   // the bound is folded with the mask
    AMS_REQUIRE(aligned16(dy) && aligned16(dx) && aligned16(ws) && (!y_below || aligned16(y_below)));
    if (ws_bytes < ams_dilated_conv2d_workspace_bytes(B, T, F, cin, cout, kh, kw)) return AMS_E_WORKSPACE_TOO_SMALL;
    hipStream_t st = (hipStream_t)stream;
    float* wt = static_cast<float*>(ws);
    const int taps = g.taps();
    wt_kernel<<<grid_for(long(taps) * cout * cin), 256, 0, st>>>(w, wt, taps, cin, cout);
    ams_status s = ams_check_launch();
    if (s != AMS_OK) return s;
    return ams_detail::conv_fwd_or_dx(dy, wt, nullptr, dx, int(g.M()), cin, T, F, log2_exact(cout), kh, kw, -rt, -rf, 0, y_below,
                                      amax_dy, amax_w, amax_dx, st);
}

ams_status ams_dilated_conv2d_bwd_filter(const float* x, const float* dy, float* dw, float* db, int B, int T, int F, int cin,
                                         int cout, int kh, int kw, int rt, int rf, const float* amax_x, const float* amax_dy, void* ws,
                                         size_t ws_bytes, void* stream) {
    const Geo g{B, T, F, cin, cout, kh, kw, rt, rf};
    AMS_REQUIRE(geo_ok(g) && x && dy && dw && db && ws);
    AMS_REQUIRE(aligned16(x) && aligned16(dy) && aligned16(dw) && aligned16(db) && aligned16(ws));
    const Ws L = ws_layout(g);
    if (ws_bytes < L.total) return AMS_E_WORKSPACE_TOO_SMALL;
    hipStream_t st = (hipStream_t)stream;
    char* base = static_cast<char*>(ws);
    float* a = reinterpret_cast<float*>(base);
    void* slabs = base + L.a;
    float* bsum_ws = reinterpret_cast<float*>(base + L.a + L.slabs);
    float* wpad = reinterpret_cast<float*>(base + L.a + L.slabs + L.bsum);
    const long M = g.M();
    const int K = g.taps() * cin;
    if (cin == 1) {                                     // 8-column image, the product writes 8 rows, the first K are copied out
        im2col_c1_kernel<<<grid_for(M * 8), 256, 0, st>>>(x, a, M, T, F, kh, kw, rt, rf);
        ams_status s = ams_check_launch();
        if (s != AMS_OK) return s;
        s = ams_gemm_f32_at_b_colsum(8, cout, int(M), a, 8, dy, cout, wpad, cout, 0, db, 0, bsum_ws, nullptr, nullptr, 0, slabs,
                                     L.slabs, nullptr, 0, st);
        if (s != AMS_OK) return s;
        if (hipMemcpyAsync(dw, wpad, size_t(K) * cout * 4, hipMemcpyDeviceToDevice, st) != hipSuccess) return ams_check_launch();
        return AMS_OK;
    }
    if (cout == 4) {
        const long per = (M + SKINNY_SLABS - 1) / SKINNY_SLABS;
        const int ns = int((M + per - 1) / per);
        conv_o4_wgrad_kernel<<<dim3(g.taps(), ns), dim3(std::min(cin, 256)), 0, st>>>(x, dy, a, M, T, F, cin, kh, kw, rt, rf, per);
        ams_status s = ams_check_launch();
        if (s != AMS_OK) return s;
        const long row = long(K) * 4 + 4;
        slab_sum_kernel<<<grid_for(row / 4), 256, 0, st>>>(a, dw, db, row, ns);
        return ams_check_launch();
    }
    return ams_detail::conv_wgrad(x, dy, dw, db, bsum_ws, int(M), cout, T, F, log2_exact(cin), kh, kw, rt, rf, amax_x, amax_dy, slabs,
                                  L.slabs, st);
}

ams_status ams_dilated_conv2d_relu_bwd(const float* dy, const float* y, float* dx, long n, float* amax_dx, void* stream) {
    AMS_REQUIRE(dy && y && dx && n > 0 && n % 4 == 0 && aligned16(dy) && aligned16(y) && aligned16(dx));
    hipStream_t st = (hipStream_t)stream;
    if (amax_dx && hipMemsetAsync(amax_dx, 0, sizeof(float), st) != hipSuccess) return ams_check_launch();
    relu_mask_kernel<<<grid_for(n / 4), 256, 0, st>>>(dy, dx, y, n / 4, reinterpret_cast<unsigned*>(amax_dx));
    return ams_check_launch();
}

}  // extern "C"
