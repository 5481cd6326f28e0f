// Device helpers and host geometry shared by the tile kernels (tiles.hip, tiles_seamless.hip): the blend profile, one pixel's bytes as one load / store,
// the np2tensor / tensor2np element ops and the blend overlap.  Every rounding is explicit (__f*_rn), so the values do not depend on the including file's
// contraction setting.
#pragma once
#include "common.h"

namespace innfer {
namespace {

// torch.linspace(start, end, steps)[i] in fp32 = one fused multiply-add per element,
// counted from the nearer end (ATen RangeFactories; verified against golden G2).
__device__ __forceinline__ float lin(float start, float end, int steps, int i) {
    if (steps == 1) return start;
    const float step = __fdiv_rn(__fsub_rn(end, start), (float)(steps - 1));
    return i < steps / 2 ? __fmaf_rn(step, (float)i, start)
                         : __fmaf_rn(-step, (float)(steps - i - 1), end);
}

__device__ __forceinline__ float profile(int i, int P, int ov) {
    if (i < ov) return lin(0.1f, 1.0f, ov, i);
    if (i < P - ov) return 1.0f;
    return lin(1.0f, 0.1f, ov, i - (P - ov));
}

// C bytes (or shorts) of one pixel in one load / store: 1, 2, 4 or 8 bytes, naturally aligned
template <typename T, int C> struct alignas(sizeof(T) * C) Px { T v[C]; };

// one np2tensor element: float32(x) / maxval [-> ((x - 0.5) * 2).clamp(-1, 1)] -- the ops of k_u8_to_nchw / k_extract_u8
__device__ __forceinline__ float to_unit(float x, float maxval, int normalize) {
    float v = __fdiv_rn(x, maxval);
    if (normalize) v = fminf(fmaxf(__fmul_rn(__fsub_rn(v, 0.5f), 2.0f), -1.0f), 1.0f);
    return v;
}

// one tensor2np element (k_nchw_to_u8 / k_recompose U8OUT): [denormalise,] clip(range * v, 0, range), round half to even
__device__ __forceinline__ int quantise(float v, int denormalize, float range) {
    if (denormalize) v = fminf(fmaxf(__fdiv_rn(__fsub_rn(v, -1.0f), 2.0f), 0.0f), 1.0f);
    return __float2int_rn(fminf(fmaxf(__fmul_rn(range, v), 0.0f), range));
}

template <typename TO>
__device__ __forceinline__ TO mean3(TO y0, TO y1, TO y2) {
    return (TO)__fdiv_rn(__fadd_rn(__fadd_rn((float)y0, (float)y1), (float)y2), 3.0f);
}

inline unsigned blocks(long total, int bs) { return (unsigned)((total + bs - 1) / bs); }


// overlap = scale * int(round((1-step) * (P/scale)))  with Python's round-half-to-even (utils.py:396)
inline int blend_overlap(int P, double step, int scale) {
    const double v = (1.0 - step) * ((double)P / scale);
    double r = __builtin_rint(v);                                     // FE_TONEAREST = half to even
    return scale * (int)r;
}

}  // namespace
}  // namespace innfer
