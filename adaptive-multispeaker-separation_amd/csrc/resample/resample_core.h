// The arithmetic of the resampler, shared by resample.hip (libams_resample.so: one signal per launch) and
// resample_ragged.hip (libams_resample_ragged.so: many signals of mixed ratios per launch): the span of input samples an
// output reaches, the two kinds of input, and the two accumulation loops.  Both translation units get their sums from THESE functions, so
// a job of the ragged library is bit-equal to the single call by construction: the same terms, in the same order, each one fused
// multiply-add (written out as __builtin_fmaf: what the compiler's contraction made of `acc += h * x` in resample.hip before this header
// existed, now independent of the contraction setting and of the code around the loop).
#ifndef AMS_RESAMPLE_CORE_H
#define AMS_RESAMPLE_CORE_H
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

constexpr int TILE = 256;             // output samples per workgroup, one per thread
constexpr int KC = 4096;              // input samples staged per round of the decimating arm (16 KB of LDS)
constexpr int MAX_RATIO = 1024;
constexpr long MAX_OUT = 1L << 38;

inline long cdiv(long a, long b) { return (a + b - 1) / b; }
inline int gcd(int a, int b) {
    while (b) {
        const int t = a % b;
        a = b;
        b = t;
    }
    return a;
}
inline bool ratio_ok(long up, long down) {
    return up >= 1 && up <= MAX_RATIO && down >= 1 && down <= MAX_RATIO && gcd((int)up, (int)down) == 1;
}

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
// Output n0 + tid of a row for the whole workgroup (all 256 threads call it: it synchronises); `end` is one past the last output that is
// wanted (M, or fewer: outputs from `end` on get an empty sum and stage nothing).  The outputs n0 .. min(n0 + 255, end - 1) reach the
// contiguous samples k_lo(first) .. k_hi(last).  They go through LDS KC at a time, every one loaded (and decoded) once; a thread adds the
// part of its own span that lies in the round, so its sum runs in increasing k whatever the number of rounds and wherever the window ends.
template <class Source>
__device__ __forceinline__ float decimate_tile(const Source& src, float* xs, long N, const float* __restrict__ taps, int up, int down, long n0,
                                               long end, int tid) {
    const int half = 10 * down;
    const long n = n0 + tid;
    const long nlast = n0 + TILE - 1 < end ? n0 + TILE - 1 : end - 1;
    const long wlo = span_of(n0, N, up, down, half).lo, whi = span_of(nlast, N, up, down, half).hi;
    Span s = span_of(n < end ? n : nlast, N, up, down, half);
    if (n >= end) { s.lo = 1; s.hi = 0; }
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
            for (int j = 0; j < cntk; ++j, t -= up) acc = __builtin_fmaf(taps[t], xs[i0 + j], acc);
        }
        __syncthreads();
    }
    return acc;
}

// ------------------------------------------------------------------ interpolation: up >= down
// Output n (< M) of a row.  At most 21 samples per output, and neighbouring outputs share them: straight from memory.
template <class Source>
__device__ __forceinline__ float interpolate_one(const Source& src, long N, const float* __restrict__ taps, int up, int down, long n) {
    const Span s = span_of(n, N, up, down, 10 * up);
    int t = (int)(s.P - s.lo * up);
    float acc = 0.f;
    for (long k = s.lo; k <= s.hi; ++k, t -= up) acc = __builtin_fmaf(taps[t], src(k), acc);
    return acc;
}

}  // namespace
#endif
