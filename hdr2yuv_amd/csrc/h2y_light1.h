/*
 * h2y_light1.h -- what the kernels that measure light share (k_light in h2y_light.hip, k_lightdist in h2y_lightdist.hip): one sample's
 * light as include/hdr2yuv_hip.h defines it, and a 64-bit wave shuffle.  Device code only; include after h2y_device.h.
 */
#pragma once

/* one sample's light: normalised as matrix_convert() does, through the source transfer (TFN) by the conversion's tiers, a NaN
 * as 0, clamped to [0, 1] (+0 for anything not above 0) */
template <bool TFN>
__device__ __forceinline__ float light1(const pix_params &pp, const pq_recA *tab, int c, float v)
{
    float x = norm1<H2Y_PIPE_RUNTIME>(pp, c, v);
    if (TFN) { /* pixel_fast(), source stage */
        const float x0 = x;
        if (pp.src_fn == H2Y_TFN_RHO_H) x = (powf25(x) - 1.0f) * 0.0625f; /* RHO_GAMMA_f's inner powf, then (P - 1) / 16: both exact */
        const float xin = x;
        bool slow;
        x = tfn_fast(x, tab, tfn_cut_of(pp.src_fn), tfn_zero_bits(pp.src_fn), tfn_one_bits(pp.src_fn), &slow);
        if (__builtin_expect(__builtin_amdgcn_ballot_w64(slow) != 0, 0)) {
            x = pq_ext_gather(xin, x, slow, pp.tf_ext[0], tfn_lo_bits(pp.src_fn)); /* below the table: the full-range table */
            if (slow) x = tf_to_linear_careful(pp.src_tf, x0);
        }
    }
    return x > 0.0f ? fminf(x, 1.0f) : 0.0f;
}

__device__ __forceinline__ unsigned long long shfl_xor_u64(unsigned long long v, int o)
{
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, o, WAVE), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), o, WAVE);
    return ((unsigned long long)hi << 32) | lo;
}
