// Packed 16-bit operations on the halves of a 32-bit register, shared by the general kernel's arithmetic flavours
// and the pair-table kernels.
#pragma once
#include "common.h"

namespace miopal {

typedef short s16x2 __attribute__((ext_vector_type(2)));
typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));

static __device__ __forceinline__ uint32_t pk_add_sat_i16(uint32_t a, uint32_t b) {
    s16x2 r = __builtin_elementwise_add_sat(__builtin_bit_cast(s16x2, a), __builtin_bit_cast(s16x2, b));
    return __builtin_bit_cast(uint32_t, r);
}
static __device__ __forceinline__ uint32_t pk_sub_sat_i16(uint32_t a, uint32_t b) {
    s16x2 r = __builtin_elementwise_sub_sat(__builtin_bit_cast(s16x2, a), __builtin_bit_cast(s16x2, b));
    return __builtin_bit_cast(uint32_t, r);
}
static __device__ __forceinline__ uint32_t pk_max_i16(uint32_t a, uint32_t b) {
    s16x2 r = __builtin_elementwise_max(__builtin_bit_cast(s16x2, a), __builtin_bit_cast(s16x2, b));
    return __builtin_bit_cast(uint32_t, r);
}
static __device__ __forceinline__ uint32_t pk_sub_sat_u16(uint32_t a, uint32_t b) {
    u16x2 r = __builtin_elementwise_sub_sat(__builtin_bit_cast(u16x2, a), __builtin_bit_cast(u16x2, b));
    return __builtin_bit_cast(uint32_t, r);
}
static __device__ __forceinline__ uint32_t pk_add_f16(uint32_t a, uint32_t b) {
    return __builtin_bit_cast(uint32_t, __builtin_bit_cast(f16x2, a) + __builtin_bit_cast(f16x2, b));
}
static __device__ __forceinline__ uint32_t pk_max3_f16(uint32_t a, uint32_t b, uint32_t c) {
    f16x2 r = __builtin_elementwise_maximum(
        __builtin_elementwise_maximum(__builtin_bit_cast(f16x2, a), __builtin_bit_cast(f16x2, b)),
        __builtin_bit_cast(f16x2, c));
    return __builtin_bit_cast(uint32_t, r);
}
static __device__ __forceinline__ uint32_t pk_max2_f16(uint32_t a, uint32_t b) {
    f16x2 r = __builtin_elementwise_maximum(__builtin_bit_cast(f16x2, a), __builtin_bit_cast(f16x2, b));
    return __builtin_bit_cast(uint32_t, r);
}
static __device__ __forceinline__ uint32_t pk_max_u16(uint32_t a, uint32_t b) {
    u16x2 r = __builtin_elementwise_max(__builtin_bit_cast(u16x2, a), __builtin_bit_cast(u16x2, b));
    return __builtin_bit_cast(uint32_t, r);
}
static __device__ __forceinline__ uint32_t dup16(int v) { return ((uint32_t)v & 0xffffu) * 0x00010001u; }
// the same signed value in both halves, as one integer ("biased integer halves", interseq_pair_parts.h)
// (unsigned arithmetic: the product wraps modulo 2^32 for negative or large v, no signed overflow)
static __device__ __forceinline__ uint32_t both(int v) { return (uint32_t)v * 0x00010001u; }

}  // namespace miopal
