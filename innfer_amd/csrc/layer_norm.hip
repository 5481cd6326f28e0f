// nn.LayerNorm(C) per pixel over a channel-padded fp16 slab (SwinIR: tokens = pixels): mean and biased variance over the C REAL channels of the slab's c_pad / 32 groups, eps inside
// the square root, per-channel affine.  Four lanes own a pixel: lane q holds channels 8 q .. 8 q + 7 of every group (one 16-byte load per group, at most 64 values), so both
// passes run on registers -- the sum, then the squared deviations from the mean (fp32, fixed order: the lane's groups in order, then the quad's butterfly) -- and
//   out = fp16(fma((x - mean) * rstd, gamma[c], beta[c])),  rstd = 1 / sqrtf(var + eps):  one fp16 rounding.
// Channels >= C are left out of the statistics whatever they hold and are WRITTEN as zeros.  in == out is allowed (a thread reads all it writes before it writes).
// Memory bound: 64 bytes per group in, 64 out.
// ADD (Swin2SR's res-post-norm, t = t + norm(branch)): out = fp16(res + fma((x - mean) * rstd, gamma[c], beta[c])) -- the same statistics in the same order, the sum in fp32,
// still ONE fp16 rounding; pad channels are written as zeros.  out may be res or in: a lane reads the eight channels of every group of both before it writes them.
#include "common.h"

namespace innfer {

namespace {

struct LnArgs {
    const f16* in; long in_gs;
    f16* out; long out_gs;
    const f16* res; long res_gs;     // ADD only
    const float* gamma; const float* beta;
    long npix; int C; float eps;
    int h1, ce;                      // HOLE only: the real channels are [0, C) and [h1, ce), h1 = 32 ceil(C / 32)
};

template <int NG, bool ADD, bool HOLE = false>
__global__ __launch_bounds__(256) void layer_norm_kernel(const LnArgs p) {
    auto real = [&](int c) { if constexpr (HOLE) return c < p.C || (c >= p.h1 && c < p.ce); else return c < p.C; };
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    const int q = (int)(i & 3);
    const bool live = (i >> 2) < p.npix;
    const long px = live ? (i >> 2) : p.npix - 1;          // (a quad beyond the last pixel repeats it and stores nothing: the exchanges below stay inside whole quads)
    const f16* ib = p.in + px * 32 + q * 8;
    f16x8 v[NG];
#pragma unroll
    for (int g = 0; g < NG; ++g) v[g] = *(const f16x8*)(ib + g * p.in_gs);
    f16x8 r[ADD ? NG : 1];
    if constexpr (ADD) {
        const f16* rb = p.res + px * 32 + q * 8;
#pragma unroll
        for (int g = 0; g < NG; ++g) r[g] = *(const f16x8*)(rb + g * p.res_gs);
    }
    auto quad = [](float s) { s += __shfl_xor(s, 1); return s + __shfl_xor(s, 2); };
    float s = 0.f;
#pragma unroll
    for (int g = 0; g < NG; ++g)
#pragma unroll
        for (int e = 0; e < 8; ++e)
            if (real(g * 32 + q * 8 + e)) s += (float)v[g][e];
    const float rc = 1.0f / (float)(HOLE ? p.C + p.ce - p.h1 : p.C);
    const float mu = quad(s) * rc;
    s = 0.f;
#pragma unroll
    for (int g = 0; g < NG; ++g)
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float d = (float)v[g][e] - mu;
            if (real(g * 32 + q * 8 + e)) s += d * d;
        }
    const float rstd = 1.0f / sqrtf(quad(s) * rc + p.eps);
    if (!live) return;
    f16* ob = p.out + px * 32 + q * 8;
#pragma unroll
    for (int g = 0; g < NG; ++g) {
        const int c0 = g * 32 + q * 8;
        f16x8 y;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            if constexpr (ADD) y[e] = real(c0 + e) ? (f16)((float)r[g][e] + __builtin_fmaf(((float)v[g][e] - mu) * rstd, p.gamma[c0 + e], p.beta[c0 + e])) : (f16)0.f;
            else y[e] = real(c0 + e) ? (f16)__builtin_fmaf(((float)v[g][e] - mu) * rstd, p.gamma[c0 + e], p.beta[c0 + e]) : (f16)0.f;
        }
        *(f16x8*)(ob + g * p.out_gs) = y;
    }
}

}  // namespace

// c_pad: channels of both slabs (a multiple of 64, >= C, <= MAXC: 256, or 512 in the wide form without residual): every group is read and written.  gamma / beta: device floats, at least C each (the values behind C are never read)
template <bool ADD, int MAXC = 256>
static int layer_norm_any(const f16* in, long in_gs, const f16* res, long res_gs, f16* out, long out_gs, long npix, int C, int c_pad, const float* gamma, const float* beta, float eps, hipStream_t s) {
    if (ADD && (!res || res_gs < npix * 32)) return set_error(INNFER_ERR_INVALID, "layer norm: the residual is null or its group stride below %ld pixels x 32", npix);
    if (!in || !out || !gamma || !beta || npix <= 0) return set_error(INNFER_ERR_INVALID, "layer norm: null argument or %ld pixels", npix);
    if (C < 1 || c_pad < C || c_pad > MAXC || c_pad % 64)
        return set_error(INNFER_ERR_UNSUPPORTED, MAXC == 256 ? "layer norm: C=%d in a slab of %d channels (built: slabs of 64, 128, 192 or 256 channels -- at most eight groups in a quad's registers)"
                                                             : "layer norm (wide): C=%d in a slab of %d channels (built: slabs of 64 .. 512 channels in steps of 64 -- at most sixteen groups in a quad's registers)", C, c_pad);
    if (in_gs < npix * 32 || out_gs < npix * 32) return set_error(INNFER_ERR_INVALID, "layer norm: a group stride below %ld pixels x 32", npix);
    const long nblk = (npix * 4 + 255) / 256;
    if (nblk > 0x7fffffffL) return set_error(INNFER_ERR_UNSUPPORTED, "layer norm: %ld pixels exceed the launch grid", npix);
    const int ng = c_pad / 32;
    GtScope gt(s, ADD ? "layer norm + residual (per pixel, padded slab)" : "layer norm (per pixel, padded slab)", (ADD ? 9.0 : 8.0) * C * (double)npix, (ADD ? 192.0 : 128.0) * ng * (double)npix);
    const LnArgs p{in, in_gs, out, out_gs, res, res_gs, gamma, beta, npix, C, eps, 0, 0};
    const dim3 grid((unsigned)nblk), block(256);
    switch (ng) {
        case 2: hipLaunchKernelGGL((layer_norm_kernel<2, ADD>), grid, block, 0, s, p); break;
        case 4: hipLaunchKernelGGL((layer_norm_kernel<4, ADD>), grid, block, 0, s, p); break;
        case 6: hipLaunchKernelGGL((layer_norm_kernel<6, ADD>), grid, block, 0, s, p); break;
        case 8: hipLaunchKernelGGL((layer_norm_kernel<8, ADD>), grid, block, 0, s, p); break;
        default:
            if constexpr (MAXC > 256 && !ADD) {
                switch (ng) {
                    case 10: hipLaunchKernelGGL((layer_norm_kernel<10, false>), grid, block, 0, s, p); break;
                    case 12: hipLaunchKernelGGL((layer_norm_kernel<12, false>), grid, block, 0, s, p); break;
                    case 14: hipLaunchKernelGGL((layer_norm_kernel<14, false>), grid, block, 0, s, p); break;
                    default: hipLaunchKernelGGL((layer_norm_kernel<16, false>), grid, block, 0, s, p); break;
                }
            }
            break;
    }
    INNFER_HIP(hipGetLastError());
    return INNFER_OK;
}

int layer_norm_launch(const f16* in, long in_gs, f16* out, long out_gs, long npix, int C, int c_pad, const float* gamma, const float* beta, float eps, hipStream_t s) {
    return layer_norm_any<false>(in, in_gs, nullptr, 0, out, out_gs, npix, C, c_pad, gamma, beta, eps, s);
}

// The same over slabs of up to 512 channels (DAT's ffn.sg.norm on half the hidden channels): up to sixteen groups, 128 values, in a quad's registers; in == out allowed
int layer_norm_wide_launch(const f16* in, long in_gs, f16* out, long out_gs, long npix, int C, int c_pad, const float* gamma, const float* beta, float eps, hipStream_t s) {
    return layer_norm_any<false, 512>(in, in_gs, nullptr, 0, out, out_gs, npix, C, c_pad, gamma, beta, eps, s);
}

// The HOLED form (DRCT's dense slab x | x1 | .. | x4: x in its own ceil(C / 32) groups, every x_k in one group behind them): the normalised channels are [0, C) and
// [32 ceil(C / 32), c_end) -- the hole [C, 32 ceil(C / 32)) and the channels from c_end on stay out of the statistics whatever they hold (a select, never a product) and are
// written as zeros.  gamma / beta: c_pad device floats indexed by SLAB channel.  Order: the lane's groups in order, then the quad's butterfly, as every other form.
int layer_norm_holed_launch(const f16* in, long in_gs, f16* out, long out_gs, long npix, int C, int c_end, int c_pad, const float* gamma, const float* beta, float eps, hipStream_t s) {
    if (!in || !out || !gamma || !beta || npix <= 0) return set_error(INNFER_ERR_INVALID, "layer norm (holed): null argument or %ld pixels", npix);
    const int h1 = (C + 31) / 32 * 32;
    if (C < 1 || c_end < h1 || c_pad < c_end || c_pad > 512 || c_pad % 64)
        return set_error(INNFER_ERR_UNSUPPORTED, "layer norm (holed): C=%d, channels up to %d in a slab of %d (built: c_end >= 32 ceil(C / 32), slabs of 64 .. 512 channels in steps of 64)", C, c_end, c_pad);
    if (in_gs < npix * 32 || out_gs < npix * 32) return set_error(INNFER_ERR_INVALID, "layer norm (holed): a group stride below %ld pixels x 32", npix);
    const long nblk = (npix * 4 + 255) / 256;
    if (nblk > 0x7fffffffL) return set_error(INNFER_ERR_UNSUPPORTED, "layer norm (holed): %ld pixels exceed the launch grid", npix);
    const int ng = c_pad / 32;
    GtScope gt(s, "layer norm (per pixel, dense slab with a hole)", 8.0 * (C + c_end - h1) * (double)npix, 128.0 * ng * (double)npix);
    const LnArgs p{in, in_gs, out, out_gs, nullptr, 0, gamma, beta, npix, C, eps, h1, c_end};
    const dim3 grid((unsigned)nblk), block(256);
    switch (ng) {
        case 2: hipLaunchKernelGGL((layer_norm_kernel<2, false, true>), grid, block, 0, s, p); break;
        case 4: hipLaunchKernelGGL((layer_norm_kernel<4, false, true>), grid, block, 0, s, p); break;
        case 6: hipLaunchKernelGGL((layer_norm_kernel<6, false, true>), grid, block, 0, s, p); break;
        case 8: hipLaunchKernelGGL((layer_norm_kernel<8, false, true>), grid, block, 0, s, p); break;
        case 10: hipLaunchKernelGGL((layer_norm_kernel<10, false, true>), grid, block, 0, s, p); break;
        case 12: hipLaunchKernelGGL((layer_norm_kernel<12, false, true>), grid, block, 0, s, p); break;
        case 14: hipLaunchKernelGGL((layer_norm_kernel<14, false, true>), grid, block, 0, s, p); break;
        default: hipLaunchKernelGGL((layer_norm_kernel<16, false, true>), grid, block, 0, s, p); break;
    }
    INNFER_HIP(hipGetLastError());
    return INNFER_OK;
}

// out = fp16(res + LayerNorm(C)(in)): `res` a third slab of c_pad channels; out may be res or in
int layer_norm_add_launch(const f16* in, long in_gs, const f16* res, long res_gs, f16* out, long out_gs, long npix, int C, int c_pad, const float* gamma, const float* beta, float eps, hipStream_t s) {
    return layer_norm_any<true>(in, in_gs, res, res_gs, out, out_gs, npix, C, c_pad, gamma, beta, eps, s);
}

}  // namespace innfer
