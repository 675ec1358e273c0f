/*
 * h2y_planes.h -- what the in-place passes over a frame's three float or half planes share (k_gamut in h2y_gamut.hip, k_tonemap in
 * h2y_tonemap.hip): one 16-byte access of a plane and its samples as binary32.  Device code only; include after h2y_kernels.h.
 */
#pragma once

#define H2Y_GLOBAL __attribute__((address_space(1)))
typedef uint32_t u32x4 __attribute__((ext_vector_type(4))); /* one 16-byte access */

template <int IN> struct plane_sample;
template <> struct plane_sample<H2Y_IN_F32> {
    typedef uint32_t bits;
    static constexpr uint32_t per_group = 4; /* pixels of one 16-byte access */
    static __device__ __forceinline__ float widen(uint32_t u) { return __builtin_bit_cast(float, u); }
    static __device__ __forceinline__ uint32_t narrow(float f) { return __builtin_bit_cast(uint32_t, f); }
    static __device__ __forceinline__ void unpack(const u32x4 v, float f[4])
    {
        f[0] = widen(v.x), f[1] = widen(v.y), f[2] = widen(v.z), f[3] = widen(v.w);
    }
    static __device__ __forceinline__ u32x4 pack(const float f[4]) { return u32x4{narrow(f[0]), narrow(f[1]), narrow(f[2]), narrow(f[3])}; }
};
template <> struct plane_sample<H2Y_IN_F16> {
    typedef uint16_t bits;
    static constexpr uint32_t per_group = 8;
    static __device__ __forceinline__ float widen(uint32_t u) { return (float)__builtin_bit_cast(_Float16, (uint16_t)u); } /* exact */
    static __device__ __forceinline__ uint32_t narrow(float f) { return __builtin_bit_cast(uint16_t, (_Float16)f); } /* to nearest even; inf past 65504 */
    static __device__ __forceinline__ void unpack(const u32x4 v, float f[8])
    {
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
        for (int k = 0; k < 4; k++) f[2 * k] = widen(w[k] & 0xFFFFu), f[2 * k + 1] = widen(w[k] >> 16);
    }
    static __device__ __forceinline__ u32x4 pack(const float f[8])
    {
        uint32_t w[4];
        for (int k = 0; k < 4; k++) w[k] = narrow(f[2 * k]) | narrow(f[2 * k + 1]) << 16;
        return u32x4{w[0], w[1], w[2], w[3]};
    }
};
