// observe_core.h — observation tensors (dg_observe_*): what a descriptor and a set of strides have to be, the clamp, the
// affine map and the narrowing store, as one body for the host path (dg_observe_host, api_scene.cpp) and the device path
// (observe_kernels.hip).  The integer value that goes in is reduce_core.h's rounded mean / luma or plane_reduce_core.h's
// representative distance: nothing of them is restated here.
#pragma once
#include "plane_reduce_core.h"
#if defined(__HIPCC__)
#include <hip/hip_fp16.h>
#endif

namespace dg {

// Channels of a source, bytes of an element.
DG_HD uint32_t obs_channels(uint32_t source) { return source == DG_OBS_RGB ? 3u : 1u; }
DG_HD uint32_t obs_element_bytes(uint32_t dtype) { return dtype == DG_OBS_U8 ? 1u : dtype == DG_OBS_F32 ? 4u : 2u; }

DG_HD uint32_t obs_f32_bits(float f) {
    union { float f; uint32_t u; } b;
    b.f = f;
    return b.u;
}
DG_HD bool obs_finite(float f) { return (obs_f32_bits(f) & 0x7F800000u) != 0x7F800000u; }

// What a descriptor has to be.
DG_HD bool obs_desc_ok(const dg_obs_desc &d) {
    if (d.fx < 1u || d.fx > REDUCE_MAX_FACTOR || d.fy < 1u || d.fy > REDUCE_MAX_FACTOR || d.reserved != 0u) return false;
    if (d.source != DG_OBS_RGB && d.source != DG_OBS_GRAY && d.source != DG_OBS_DISTANCE) return false;
    if (d.source == DG_OBS_DISTANCE ? d.rule != DG_PLANE_POINT && d.rule != DG_PLANE_NEAREST : d.rule != 0u) return false;
    if (d.dtype != DG_OBS_U8 && d.dtype != DG_OBS_F16 && d.dtype != DG_OBS_BF16 && d.dtype != DG_OBS_F32) return false;
    if (d.lo > d.hi || d.lo < -32768 || d.hi > 32767) return false;
    if (!obs_finite(d.scale) || !obs_finite(d.bias)) return false;
    if (d.dtype == DG_OBS_U8 && !(d.scale == 1.0f && d.bias == 0.0f && d.lo >= 0 && d.hi <= 255)) return false;
    return true;
}

// The stride rule.  Every stride is >= 1; over the dimensions whose extent is above 1, in the order of their strides, each stride is
// at least the one before times that one's extent, so no two elements share an address.  The products are compared as quotients
// (a b <= s  <=>  a <= floor(s / b) for positive integers), so nothing overflows; and the largest stride times its extent stays below
// 2^62 elements, so that no offset the stores compute does.
DG_HD bool obs_strides_ok(const int64_t strides[4], const uint32_t extent[4]) {
    int64_t st[4];
    uint32_t ex[4];
    uint32_t m = 0;
    for (uint32_t i = 0; i < 4u; i++) {
        if (strides[i] < 1) return false;
        if (extent[i] <= 1u) continue;
        uint32_t k = m++;
        for (; k > 0u && st[k - 1u] > strides[i]; k--) { st[k] = st[k - 1u]; ex[k] = ex[k - 1u]; }
        st[k] = strides[i]; ex[k] = extent[i];
    }
    for (uint32_t k = 1; k < m; k++)
        if (st[k] / (int64_t)ex[k - 1u] < st[k - 1u]) return false;
    return m == 0u || st[m - 1u] <= ((int64_t)1 << 62) / (int64_t)ex[m - 1u];
}

DG_HD int32_t obs_clamp(int32_t v, int32_t lo, int32_t hi) { return v < lo ? lo : v > hi ? hi : v; }

// o = fl32(fl32((float)v * scale) + bias): two roundings.  Every TU is built with -ffp-contract=off (the Makefile's FLAGS, rust_num.h),
// which forbids the fused form; the product is a statement of its own besides.  Subnormals are kept on both sides (neither build
// flushes them).
DG_HD float obs_map(int32_t v, float scale, float bias) {
    const float p = (float)v * scale;
    return p + bias;
}

// binary32 -> binary16, round to nearest even, as integer arithmetic on the bits: subnormals kept, overflow to infinity.  (A NaN cannot
// arise from finite scale and bias; it keeps its top mantissa bits and stays a NaN.)
DG_HD uint16_t obs_f16_bits(float f) {
    const uint32_t u = obs_f32_bits(f), sign = (u >> 16) & 0x8000u, a = u & 0x7FFFFFFFu;
    if (a > 0x7F800000u) {
        const uint32_t r = 0x7C00u + ((a & 0x007FFFFFu) >> 13);
        return (uint16_t)(sign + (r == 0x7C00u ? r + 1u : r));
    }
    if (a >= 0x477FF000u) return (uint16_t)(sign | 0x7C00u);          // 65520 = max + half an ulp ties to even: infinity
    if (a >= 0x38800000u) {                                            // normal: rebias the exponent (127 -> 15), round 13 bits away
        const uint32_t r = a - 0x38000000u;
        return (uint16_t)(sign | ((r + 0x0FFFu + ((r >> 13) & 1u)) >> 13));
    }
    if (a <= 0x33000000u) return (uint16_t)sign;                       // up to 2^-25, half the smallest subnormal: ties to even, 0
    const uint32_t shift = 126u - (a >> 23), m = (a & 0x007FFFFFu) | 0x00800000u;      // in units of 2^-24: m >> shift, 14 <= shift <= 24
    const uint32_t q = m >> shift, rem = m & ((1u << shift) - 1u), half = 1u << (shift - 1u);
    return (uint16_t)(sign | (q + (rem > half || (rem == half && (q & 1u)) ? 1u : 0u)));
}

// binary32 -> bfloat16, round to nearest even: the upper half of the bits after adding half an ulp less one, plus the bit that stays
// lowest.  A carry out of the mantissa is the next exponent, out of the largest exponent infinity.  (A NaN becomes the quiet 0x7FC0.)
DG_HD uint16_t obs_bf16_bits(float f) {
    const uint32_t u = obs_f32_bits(f);
    if ((u & 0x7FFFFFFFu) > 0x7F800000u) return (uint16_t)0x7FC0u;
    return (uint16_t)((u + 0x7FFFu + ((u >> 16) & 1u)) >> 16);
}

// The three narrowings of the device.  binary16: the hardware conversion, round to nearest even under the kernels' default mode;
// bfloat16: the integer form above.  The host takes the integer forms, so that it needs no _Float16.
#if defined(__HIP_DEVICE_COMPILE__)
DG_HD uint16_t obs_f16_narrow(float f) { return __half_as_ushort(__float2half_rn(f)); }
#else
DG_HD uint16_t obs_f16_narrow(float f) { return obs_f16_bits(f); }
#endif

// Element `at` of dst takes clamped value v under (scale, bias), as DTYPE.
template <uint32_t DTYPE>
DG_HD void obs_store(void *dst, int64_t at, int32_t v, float scale, float bias) {
    if (DTYPE == DG_OBS_U8) static_cast<uint8_t *>(dst)[at] = (uint8_t)v;
    else if (DTYPE == DG_OBS_F32) static_cast<float *>(dst)[at] = obs_map(v, scale, bias);
    else if (DTYPE == DG_OBS_F16) static_cast<uint16_t *>(dst)[at] = obs_f16_narrow(obs_map(v, scale, bias));
    else static_cast<uint16_t *>(dst)[at] = obs_bf16_bits(obs_map(v, scale, bias));
}

// What every store of both paths runs: the clamp, then obs_store of the descriptor's dtype.
DG_HD void obs_put(const dg_obs_desc &d, void *dst, int64_t at, int32_t v) {
    v = obs_clamp(v, d.lo, d.hi);
    switch (d.dtype) {
        case DG_OBS_U8: obs_store<DG_OBS_U8>(dst, at, v, d.scale, d.bias); break;
        case DG_OBS_F16: obs_store<DG_OBS_F16>(dst, at, v, d.scale, d.bias); break;
        case DG_OBS_BF16: obs_store<DG_OBS_BF16>(dst, at, v, d.scale, d.bias); break;
        default: obs_store<DG_OBS_F32>(dst, at, v, d.scale, d.bias); break;
    }
}

// The store phase's lane-to-element map of the colour kernel: item j of a run of np output pixels with 3 channels.  Planar
// (strides[3] == 1): channel after channel, consecutive items are consecutive pixels of one channel; otherwise consecutive items are
// the channels of consecutive pixels.  Both are one-to-one onto [0, np) x [0, 3) for j in [0, 3 np).
DG_HD void obs_item(uint32_t j, uint32_t np, bool planar, uint32_t &p, uint32_t &c) {
    if (planar) { c = j >= 2u * np ? 2u : j >= np ? 1u : 0u; p = j - c * np; }
    else { p = j / 3u; c = j - 3u * p; }
}

}  // namespace dg
