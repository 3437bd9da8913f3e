// Batch assembly from a device-resident sample pool (include/ams.h: ams_mix_gather; data/resident.py plans the indices).
// A streaming kernel: one float4 of positions per thread and batch row; the S source chunks are loaded, stored as the rows of non_mix and
// added up in source order ((r0 + r1) + r2) ... with plain f32 adds -- the bits of np.stack(rows).sum(axis=0) -- into mix.  No LDS, no
// atomics; pool offsets are 64-bit.
#include "common.h"

namespace {

// VEC: L % 4 == 0 and 16-byte aligned mix / non_mix: 16-byte stores; a source chunk that is itself 16-byte aligned (every chunk when
// the pool's utterances start at multiples of 4 floats) is fetched as one float4, any other with four dword loads -- a branch on the
// row's address, the same for every lane of the workgroup.  !VEC: thread t handles positions t, t + 256, t + 512, t + 768 of the
// workgroup's 1024 (coalesced dwords), any L and any base.
template <int S, bool VEC>
__global__ __launch_bounds__(256) void mix_gather_kernel(const float* __restrict__ pool, const long long* __restrict__ utt_off,
                                                         const int* __restrict__ plan, const int* __restrict__ plan_keys, long first,
                                                         float* __restrict__ mix, float* __restrict__ non_mix, int* __restrict__ ind, int L) {
    const int b = blockIdx.y;
    const long j = first + b;
    const float* src[S];
#pragma unroll
    for (int s = 0; s < S; ++s) {
        const int u = plan[(j * S + s) * 2], c = plan[(j * S + s) * 2 + 1];
        src[s] = pool + (long)utt_off[u] + (long)c * L;
    }
    if (blockIdx.x == 0 && threadIdx.x < S) ind[(long)b * S + threadIdx.x] = plan_keys[j * S + threadIdx.x];
    float* const mrow = mix + (long)b * L;
    float* const nrow = non_mix + (long)b * S * L;
    if constexpr (VEC) {
        const int i = (blockIdx.x * 256 + threadIdx.x) * 4;
        if (i >= L) return;
        f32x4 r[S];
#pragma unroll
        for (int s = 0; s < S; ++s) {
            const float* p = src[s] + i;
            if (((uintptr_t)src[s] & 15) == 0) r[s] = *(const f32x4*)p;
            else { r[s][0] = p[0]; r[s][1] = p[1]; r[s][2] = p[2]; r[s][3] = p[3]; }
        }
        f32x4 acc = r[0];
#pragma unroll
        for (int s = 0; s < S; ++s) {
            *(f32x4*)(nrow + (long)s * L + i) = r[s];
            if (s > 0) acc = acc + r[s];
        }
        *(f32x4*)(mrow + i) = acc;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int i = blockIdx.x * 1024 + k * 256 + threadIdx.x;
            if (i >= L) break;
            float r[S];
#pragma unroll
            for (int s = 0; s < S; ++s) r[s] = src[s][i];
            float acc = r[0];
#pragma unroll
            for (int s = 0; s < S; ++s) {
                nrow[(long)s * L + i] = r[s];
                if (s > 0) acc = acc + r[s];
            }
            mrow[i] = acc;
        }
    }
}

template <int S>
void launch(bool vec, dim3 grid, hipStream_t st, const float* pool, const long long* utt_off, const int* plan, const int* plan_keys,
            long first, float* mix, float* non_mix, int* ind, int L) {
    if (vec) hipLaunchKernelGGL((mix_gather_kernel<S, true>), grid, dim3(256), 0, st, pool, utt_off, plan, plan_keys, first, mix, non_mix, ind, L);
    else hipLaunchKernelGGL((mix_gather_kernel<S, false>), grid, dim3(256), 0, st, pool, utt_off, plan, plan_keys, first, mix, non_mix, ind, L);
}

}  // namespace

extern "C" {

ams_status ams_mix_gather(const float* pool, const long long* utt_off, const int32_t* plan, const int32_t* plan_keys, long first,
                          float* mix, float* non_mix, int32_t* ind, int B, int S, int L, void* stream) {
    AMS_REQUIRE(pool && utt_off && plan && plan_keys && mix && non_mix && ind);
    AMS_REQUIRE(S >= 1 && S <= 6 && B >= 1 && B <= 65535 && L >= 1 && L <= (1 << 30) && first >= 0);      // 32-bit positions inside a row
    const bool vec = L % 4 == 0 && (((uintptr_t)pool | (uintptr_t)mix | (uintptr_t)non_mix) & 15) == 0;
    const dim3 grid((unsigned)ceil_div(L, 1024), (unsigned)B);
    hipStream_t st = (hipStream_t)stream;
    switch (S) {
        case 1: launch<1>(vec, grid, st, pool, utt_off, plan, plan_keys, first, mix, non_mix, ind, L); break;
        case 2: launch<2>(vec, grid, st, pool, utt_off, plan, plan_keys, first, mix, non_mix, ind, L); break;
        case 3: launch<3>(vec, grid, st, pool, utt_off, plan, plan_keys, first, mix, non_mix, ind, L); break;
        case 4: launch<4>(vec, grid, st, pool, utt_off, plan, plan_keys, first, mix, non_mix, ind, L); break;
        case 5: launch<5>(vec, grid, st, pool, utt_off, plan, plan_keys, first, mix, non_mix, ind, L); break;
        default: launch<6>(vec, grid, st, pool, utt_off, plan, plan_keys, first, mix, non_mix, ind, L); break;
    }
    return ams_check_launch();
}

}  // extern "C"
