// Sample-rate conversion (include/ams_resample.h): a rational-ratio polyphase FIR with 16-bit-PCM decoding and the channel
// down-mix fused into its input side.  A library of its own (libams_resample.so): include/ams.h, include/ams_stitch.h and their
// libraries are untouched.  Streaming kernels: one output sample per thread, float32 sums in increasing k, no MFMA, no atomics, no
// scratch.  y[n] = sum_k taps[n down + half - k up] x[k]; the position n down + half is 64-bit, a tap index (0 .. 2 half) is an int.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include "../../../include/ams_resample.h"

namespace {

constexpr int TILE = 256;             // output samples per workgroup, one per thread
constexpr int KC = 4096;              // input samples staged per round of the decimating arm (16 KB of LDS)
constexpr int MAX_RATIO = 1024;
constexpr long MAX_OUT = 1L << 38;

#define RESAMPLE_REQUIRE(cond)                 \
    do {                                       \
        if (!(cond)) return AMS_E_INVALID_ARG; \
    } while (0)

inline ams_status check_launch() { return hipGetLastError() == hipSuccess ? AMS_OK : AMS_E_LAUNCH_FAILED; }
inline long cdiv(long a, long b) { return (a + b - 1) / b; }
inline int gcd(int a, int b) {
    while (b) {
        const int t = a % b;
        a = b;
        b = t;
    }
    return a;
}
inline bool ratio_ok(int up, int down) { return up >= 1 && up <= MAX_RATIO && down >= 1 && down <= MAX_RATIO && gcd(up, down) == 1; }

// ------------------------------------------------------------------ the two kinds of input
struct F32Source {                    // a float32 row
    const float* x;
    __device__ __forceinline__ void advance(long off) { x += off; }
    __device__ __forceinline__ float operator()(long k) const { return x[k]; }
};

struct Pcm16Source {                  // interleaved int16 frames: the int32 sum of a frame's channels over 32768 channels, one IEEE division
    const int16_t* pcm;
    int channels;
    __device__ __forceinline__ void advance(long off) { pcm += off * channels; }
    __device__ __forceinline__ float operator()(long k) const {
        const int16_t* f = pcm + k * channels;
        int s = 0;
        for (int c = 0; c < channels; ++c) s += f[c];
        return (float)s / (float)(32768 * channels);
    }
};

// the input samples output n reaches: k_lo .. k_hi (never empty for n < M: half >= 10 up), and P = n down + half
struct Span {
    long P, lo, hi;
};

__device__ __forceinline__ Span span_of(long n, long N, int up, int down, int half) {
    Span s;
    s.P = n * down + half;
    const long q = s.P - 2L * half;                            // the lowest k has P - k up <= 2 half
    s.lo = q <= 0 ? 0 : (q + up - 1) / up;
    s.hi = s.P / up;                                           // the highest k has P - k up >= 0
    if (s.hi > N - 1) s.hi = N - 1;
    return s;
}

// ------------------------------------------------------------------ decimation: down > up
// The 256 outputs of a workgroup reach the contiguous samples k_lo(first) .. k_hi(last).  They go through LDS KC at a time, every one
// loaded (and decoded) once; a thread adds the part of its own span that lies in the round, so its sum runs in increasing k whatever
// the number of rounds.
template <class Source>
__global__ __launch_bounds__(TILE) void decimate_kernel(Source src0, long x_stride, long N, const float* __restrict__ taps, int up, int down,
                                                        float* __restrict__ y, long M, long y_stride) {
    __shared__ float xs[KC];
    const int tid = threadIdx.x, half = 10 * down;
    const long n0 = (long)blockIdx.x * TILE, n = n0 + tid;
    const long nlast = n0 + TILE - 1 < M ? n0 + TILE - 1 : M - 1;
    Source src = src0;
    src.advance((long)blockIdx.y * x_stride);
    const long wlo = span_of(n0, N, up, down, half).lo, whi = span_of(nlast, N, up, down, half).hi;
    Span s = span_of(n < M ? n : nlast, N, up, down, half);
    if (n >= M) { s.lo = 1; s.hi = 0; }
    float acc = 0.f;
    for (long c0 = wlo; c0 <= whi; c0 += KC) {
        const int cnt = (int)(whi - c0 + 1 < KC ? whi - c0 + 1 : KC);
        for (int i = tid; i < cnt; i += TILE) xs[i] = src(c0 + i);
        __syncthreads();
        const long a = s.lo > c0 ? s.lo : c0, b = s.hi < c0 + cnt - 1 ? s.hi : c0 + cnt - 1;
        if (a <= b) {
            const int i0 = (int)(a - c0), cntk = (int)(b - a + 1);
            int t = (int)(s.P - a * up);                       // 0 .. 2 half, falls by up per sample
#pragma unroll 4
            for (int j = 0; j < cntk; ++j, t -= up) acc += taps[t] * xs[i0 + j];
        }
        __syncthreads();
    }
    if (n < M) y[(long)blockIdx.y * y_stride + n] = acc;
}

// ------------------------------------------------------------------ interpolation: up >= down
// At most 21 samples per output, and neighbouring outputs share them: straight from memory.
template <class Source>
__global__ __launch_bounds__(TILE) void interpolate_kernel(Source src0, long x_stride, long N, const float* __restrict__ taps, int up, int down,
                                                           float* __restrict__ y, long M, long y_stride) {
    const long n = (long)blockIdx.x * TILE + threadIdx.x;
    if (n >= M) return;
    Source src = src0;
    src.advance((long)blockIdx.y * x_stride);
    const Span s = span_of(n, N, up, down, 10 * up);
    int t = (int)(s.P - s.lo * up);
    float acc = 0.f;
    for (long k = s.lo; k <= s.hi; ++k, t -= up) acc += taps[t] * src(k);
    y[(long)blockIdx.y * y_stride + n] = acc;
}

// ------------------------------------------------------------------ up = down = 1 on PCM: decode and down-mix only
__global__ __launch_bounds__(TILE) void decode_kernel(Pcm16Source src, long N, float* __restrict__ y) {
    const long n = (long)blockIdx.x * TILE + threadIdx.x;
    if (n < N) y[n] = src(n);
}

template <class Source>
ams_status launch(Source src, int rows, long n_in, long x_stride, const float* taps, int up, int down, float* y, long n_out, long y_stride,
                  hipStream_t st) {
    const dim3 grid((unsigned)cdiv(n_out, TILE), (unsigned)rows);
    if (down > up) hipLaunchKernelGGL(decimate_kernel<Source>, grid, dim3(TILE), 0, st, src, x_stride, n_in, taps, up, down, y, n_out, y_stride);
    else hipLaunchKernelGGL(interpolate_kernel<Source>, grid, dim3(TILE), 0, st, src, x_stride, n_in, taps, up, down, y, n_out, y_stride);
    return check_launch();
}

}  // namespace

extern "C" {

int ams_resample_abi_version(void) { return 1; }

long ams_resample_out_len(long n_in, int up, int down) {
    if (n_in < 1 || !ratio_ok(up, down) || n_in > MAX_OUT) return 0;
    const long M = cdiv(n_in * up, down);
    return M <= MAX_OUT ? M : 0;
}

ams_status ams_resample_pcm16(const int16_t* pcm, long n_in, int channels, const float* taps, int ntaps, int up, int down, float* y,
                              long n_out, void* stream) {
    RESAMPLE_REQUIRE(pcm && y);
    RESAMPLE_REQUIRE(channels >= 1 && channels <= 8 && n_in >= 1 && ratio_ok(up, down));
    const long M = ams_resample_out_len(n_in, up, down);
    RESAMPLE_REQUIRE(M >= 1 && n_out == M);
    hipStream_t st = (hipStream_t)stream;
    Pcm16Source src{pcm, channels};
    if (up == 1 && down == 1) {
        hipLaunchKernelGGL(decode_kernel, dim3((unsigned)cdiv(n_in, TILE)), dim3(TILE), 0, st, src, n_in, y);
        return check_launch();
    }
    RESAMPLE_REQUIRE(taps && ntaps == 20 * (up > down ? up : down) + 1);
    return launch(src, 1, n_in, 0, taps, up, down, y, n_out, n_out, st);
}

ams_status ams_resample_f32(const float* x, int rows, long n_in, long x_stride, const float* taps, int ntaps, int up, int down, float* y,
                            long n_out, long y_stride, void* stream) {
    RESAMPLE_REQUIRE(x && y && taps);
    RESAMPLE_REQUIRE(rows >= 1 && rows <= 65535 && n_in >= 1 && ratio_ok(up, down));
    RESAMPLE_REQUIRE(ntaps == 20 * (up > down ? up : down) + 1);
    const long M = ams_resample_out_len(n_in, up, down);
    RESAMPLE_REQUIRE(M >= 1 && n_out == M && x_stride >= n_in && y_stride >= n_out);
    return launch(F32Source{x}, rows, n_in, x_stride, taps, up, down, y, n_out, y_stride, (hipStream_t)stream);
}

}  // extern "C"
