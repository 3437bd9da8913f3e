// How an f32 operand is cut for the 16-bit matrix pipe, and the sc1 buffer accesses of the kernels that publish to each other: the ONE
// definition for csrc/gemm.hip, gemm_ps.hip, lstm_ring.hip, dpcl.hip and kmeans.hip.  The tests assert bit identity between the forms
// of a product (pre-split images against the in-product cut, path B, dX from a weight image); that identity is this file.
//
// bf16x6: a = hi + mid + lo exactly, three bf16 terms (split3); six partial products.  Needs no scale (bf16 has the f32 exponent) and
// stays the arithmetic of every launch that does not supply the bounds.
//
// fp16x3: two fp16 planes per operand instead of three bf16 planes, three products instead of six.
//   a * s = h0 + h1 + e,  h0 = fp16(a s),  h1 = fp16(a s - h0),  |e| <= 2^-22 |a s|   (both conversions round to nearest; h0 * h0' is exact in f32)
//   a.b ~ [h0.h0' + (h0.h1' + h1.h0')] / (s s')   -- dropped: h1.h1' (2^-22) and e: the same 2^-22 level as the f32 accumulation itself
// s = 2^(13 - floor(log2(amax))): the largest operand entry lands in [2^13, 2^14) (fp16 overflows at 65504), entries down to amax * 2^-17
// keep all 22 bits, smaller ones an absolute error of amax * 2^-39.
#pragma once
#include <hip/hip_runtime.h>

typedef _Float16 f16x2_t __attribute__((ext_vector_type(2)));
typedef _Float16 f16x4_t __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8_t __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));
typedef float f32x2_t __attribute__((ext_vector_type(2)));
typedef int i32x4_t __attribute__((ext_vector_type(4)));

__device__ __forceinline__ unsigned pk_bf16(float a, float b) {           // v_cvt_pk_bf16_f32: a -> bits 0..15, b -> bits 16..31
    const f32x2_t v = {a, b};
    return __builtin_bit_cast(unsigned, __builtin_convertvector(v, bf16x2_t));
}
__device__ __forceinline__ unsigned pk_f16(float a, float b) {
    const f32x2_t v = {a, b};
    return __builtin_bit_cast(unsigned, __builtin_convertvector(v, f16x2_t));
}
__device__ __forceinline__ void split2h(float a, float b, unsigned& hi, unsigned& mid) {
    hi = pk_f16(a, b);
    const f16x2_t h = __builtin_bit_cast(f16x2_t, hi);
    mid = pk_f16(a - (float)h[0], b - (float)h[1]);
}
__device__ __forceinline__ void split3(float a, float b, unsigned& hi, unsigned& mid, unsigned& lo) {
    hi = pk_bf16(a, b);
    const float ra = a - __uint_as_float(hi << 16), rb = b - __uint_as_float(hi & 0xffff0000u);
    mid = pk_bf16(ra, rb);
    const float sa = ra - __uint_as_float(mid << 16), sb = rb - __uint_as_float(mid & 0xffff0000u);
    lo = pk_bf16(sa, sb);
}
// One value as the two fp16 terms of split2h in ONE dword, hi | mid << 16: what the PRODUCER of h_t publishes in the fp16x3 forward
// ring (round 5).  A consumer then builds its MFMA operand planes with two v_perm_b32 per pair of k-slots; splitting on arrival was two
// conversions back, two subtractions and two packed conversions per pair in each of the 25 consumers' four waves, on the hand-off cycle.
__device__ __forceinline__ unsigned pack_hm(float v) {
    const _Float16 hi = (_Float16)v;
    const _Float16 mid = (_Float16)(v - (float)hi);
    return (unsigned)__builtin_bit_cast(unsigned short, hi) | ((unsigned)__builtin_bit_cast(unsigned short, mid) << 16);
}
// 2^(13 - floor(log2(amax))) for a finite positive amax; 1 for 0, denormals, Inf and NaN (which then propagate as they would in f32)
__device__ __forceinline__ float f16_scale(float amax) {
    const int e = (int)((__float_as_uint(amax) >> 23) & 0xffu);
    if (e == 0 || e == 255) return 1.0f;
    const int se = 127 + 13 - (e - 127);            // biased exponent of the scale
    return (se >= 1 && se <= 254) ? __uint_as_float((unsigned)se << 23) : 1.0f;
}
// the same scale and its exact inverse (both powers of two; (1, 1) where f16_scale gives 1)
__device__ __forceinline__ void f16_scale2(float amax, float& sc, float& inv) {
    const int e = (int)((__float_as_uint(amax) >> 23) & 0xffu);
    const int se = 127 + 13 - (e - 127);
    const bool ok = (e != 0 && e != 255 && se >= 1 && se <= 253);
    sc = ok ? __uint_as_float((unsigned)se << 23) : 1.0f;
    inv = ok ? __uint_as_float((unsigned)(254 - se) << 23) : 1.0f;
}

// Raw buffer accesses with aux bit 16 = sc1: stores write through to the memory side, loads bypass this CU's L1 and are served by the
// L2 -- the publish form of MI355X_MICROARCH.md ("publish-large": sc1 payload -> s_waitcnt vmcnt(0) -> agent-scope flag, sc1 loads on
// the reader)
__device__ __forceinline__ __amdgpu_buffer_rsrc_t make_rsrc(const void* p, unsigned bytes) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), (short)0, (int)bytes, 0x00020000);
}
__device__ __forceinline__ float4 ld16_sc1(__amdgpu_buffer_rsrc_t rs, unsigned off) {
    return __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(rs, off, 0, 16));
}
__device__ __forceinline__ float ld4_sc1(__amdgpu_buffer_rsrc_t rs, unsigned off) {
    return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs, off, 0, 16));
}
__device__ __forceinline__ void st16_sc1(__amdgpu_buffer_rsrc_t rs, unsigned off, float4 v) {
    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(i32x4_t, v), rs, off, 0, 16);
}
