// Device helpers and host geometry shared by the tile kernels (tiles.hip, tiles_u8.hip, tiles_tta.hip): the blend profile, one pixel's bytes as one load / store,
// the np2tensor / tensor2np element ops, the blend overlap and the blend's geometry check.  Every rounding is explicit (__f*_rn), so the values do not depend on the including file's
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

// one np2tensor element: float32(x) / maxval [-> ((x - 0.5) * 2).clamp(-1, 1)] -- the ops of k_u8_to_nchw
__device__ __forceinline__ float to_unit(float x, float maxval, int normalize) {
    float v = __fdiv_rn(x, maxval);
    if (normalize) v = fminf(fmaxf(__fmul_rn(__fsub_rn(v, 0.5f), 2.0f), -1.0f), 1.0f);
    return v;
}

// one tensor2np element (the ops of k_nchw_to_u8): [denormalise,] clip(range * v, 0, range), round half to even
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

// The blend geometry every recompose entry point checks and uses: the FH x FW blend of n tiles [.., P, P] on the lattice of the (height, width) image at
// `scale`, and cs = scale * crop, what the crop window leaves off every side.  batch: n is any multiple of the lattice (innfer_recompose), else exactly one
// image.  0 or the error already set, prefixed with the entry point's name.
struct BlendGeo { int FH, FW, ov, eff, nh, nw, cs; };
inline int blend_geo(const char* who, int n, int P, int height, int width, double step, int scale, int crop, bool batch, BlendGeo* g) {
    if (step < 0.5 || step > 1.0) return set_error(INNFER_ERR_INVALID, "%s: step must be in [0.5,1]", who);
    if (n <= 0 || P <= 0 || scale <= 0 || height <= 0 || width <= 0) return set_error(INNFER_ERR_INVALID, "%s: bad sizes", who);
    if (crop < 0 || 2L * crop >= height || 2L * crop >= width) return set_error(INNFER_ERR_INVALID, "%s: crop %d leaves nothing of %dx%d", who, crop, height, width);
    if ((long)scale * height > 0x7fffffffL / 2 || (long)scale * width > 0x7fffffffL / 2) return set_error(INNFER_ERR_INVALID, "%s: output size overflows", who);
    g->FH = scale * height; g->FW = scale * width;
    if (g->FH < P || g->FW < P) return set_error(INNFER_ERR_INVALID, "%s: patch %d larger than output %dx%d", who, P, g->FH, g->FW);
    g->ov = blend_overlap(P, step, scale);
    if (P - 2 * g->ov < 0) return set_error(INNFER_ERR_INVALID, "%s: overlap %d exceeds half of patch %d (reference raises too)", who, g->ov, P);
    g->eff = (int)(step * P);
    g->nh = 1 + (g->FH - P) / g->eff + ((g->FH - P) % g->eff != 0);
    g->nw = 1 + (g->FW - P) / g->eff + ((g->FW - P) % g->eff != 0);
    if (batch && n % (g->nh * g->nw)) return set_error(INNFER_ERR_INVALID, "%s: %d tiles is not a multiple of %dx%d", who, n, g->nh, g->nw);
    if (!batch && n != g->nh * g->nw) return set_error(INNFER_ERR_INVALID, "%s: one image of %dx%d tiles expected, got %d tiles", who, g->nh, g->nw, n);
    g->cs = scale * crop;
    return INNFER_OK;
}

// Source index of position i (relative to the image: -pad .. n + pad - 1) on an axis of n pixels; -1: outside under INNFER_BORDER_ALPHA_PAD.  Inside the
// image no division is made.  INNFER_BORDER_MIRROR needs n >= 2 (its period is 2 (n - 1)): the entry points refuse n < 2 before anything is launched.
__host__ __device__ __forceinline__ int border_index(int i, int n, int mode) {
    if ((unsigned)i < (unsigned)n) return i;
    if (mode == INNFER_BORDER_TILE) {
        const int r = i % n;
        return r < 0 ? r + n : r;
    }
    if (mode == INNFER_BORDER_MIRROR) {
        const int p = 2 * (n - 1);
        int j = i % p;
        if (j < 0) j += p;
        return j < n ? j : p - j;
    }
    if (mode == INNFER_BORDER_REPLICATE) return i < 0 ? 0 : n - 1;
    return -1;
}

// N elements in one load / store at alignment A bytes (3-channel pixels: four of them are 12 bytes at 4, one is three byte accesses)
template <typename T, int N, int A> struct alignas(A) Run { T v[N]; };

// what every entry point checks of (H, W, pad, mode); 0 or the error already set
inline int check_border(const char* who, int H, int W, int pad, int mode) {
    if (H <= 0 || W <= 0 || pad < 0) return set_error(INNFER_ERR_INVALID, "%s: bad sizes H=%d W=%d pad=%d", who, H, W, pad);
    if (mode < INNFER_BORDER_TILE || mode > INNFER_BORDER_ALPHA_PAD) return set_error(INNFER_ERR_INVALID, "%s: border mode %d (0 tile, 1 mirror, 2 replicate, 3 alpha_pad)", who, mode);
    if (mode == INNFER_BORDER_MIRROR && (H < 2 || W < 2))
        return set_error(INNFER_ERR_INVALID, "%s: mirror needs at least 2 rows and 2 columns, the image is %dx%d", who, H, W);
    if ((long)H + 2L * pad > 0x3fffffffL || (long)W + 2L * pad > 0x3fffffffL) return set_error(INNFER_ERR_INVALID, "%s: padded size overflows", who);
    return INNFER_OK;
}

}  // namespace
}  // namespace innfer
