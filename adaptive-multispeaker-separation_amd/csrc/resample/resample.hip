// Sample-rate conversion (include/ams_resample.h): a rational-ratio polyphase FIR with 16-bit-PCM decoding and the channel
// down-mix fused into its input side.  A library of its own (libams_resample.so): include/ams.h, include/ams_stitch.h and their
// libraries are untouched.  Streaming kernels: one output sample per thread, float32 sums in increasing k, no MFMA, no atomics, no
// scratch.  y[n] = sum_k taps[n down + half - k up] x[k]; the position n down + half is 64-bit, a tap index (0 .. 2 half) is an int.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include "../../../include/ams_resample.h"
#include "resample_core.h"                // TILE, KC, Span / span_of, the two Sources and the two accumulation loops (shared with resample_ragged.hip)

namespace {

#define RESAMPLE_REQUIRE(cond)                 \
    do {                                       \
        if (!(cond)) return AMS_E_INVALID_ARG; \
    } while (0)

inline ams_status check_launch() { return hipGetLastError() == hipSuccess ? AMS_OK : AMS_E_LAUNCH_FAILED; }

// ------------------------------------------------------------------ decimation: down > up (decimate_tile: the LDS-staged window)
template <class Source>
__global__ __launch_bounds__(TILE) void decimate_kernel(Source src0, long x_stride, long N, const float* __restrict__ taps, int up, int down,
                                                        float* __restrict__ y, long M, long y_stride) {
    __shared__ float xs[KC];
    const long n0 = (long)blockIdx.x * TILE, n = n0 + threadIdx.x;
    Source src = src0;
    src.advance((long)blockIdx.y * x_stride);
    const float acc = decimate_tile(src, xs, N, taps, up, down, n0, M, (int)threadIdx.x);
    if (n < M) y[(long)blockIdx.y * y_stride + n] = acc;
}

// ------------------------------------------------------------------ interpolation: up >= down (interpolate_one: straight from memory)
template <class Source>
__global__ __launch_bounds__(TILE) void interpolate_kernel(Source src0, long x_stride, long N, const float* __restrict__ taps, int up, int down,
                                                           float* __restrict__ y, long M, long y_stride) {
    const long n = (long)blockIdx.x * TILE + threadIdx.x;
    if (n >= M) return;
    Source src = src0;
    src.advance((long)blockIdx.y * x_stride);
    y[(long)blockIdx.y * y_stride + n] = interpolate_one(src, N, taps, up, down, n);
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
