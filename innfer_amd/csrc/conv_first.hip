// First convolution of a generator: few input channels (1..8), NCHW planar input
// straight from the caller's tensor, fp16 blocked-NHWC slab output.
// Replaces `fea_conv = conv_block(in_nc, nf, 3)` (RRDBNet_arch.py:25, SRResNet_arch.py:24).
//
// 1728 MAC per pixel for 3->64: 0.01 % of an RRDBNet-23 forward, bound by its 128 B/pixel store.  On the matrix cores with split fp32 operands (first_conv_mfma
// below); the VALU kernel of round 1 it replaced (K/8 lanes per pixel) was removed in round 6: every engine's first conv has 32 or 64 outputs.
#include "common.h"
#include <type_traits>

namespace innfer {
namespace {

struct FP;
__device__ __forceinline__ float first_conv_input(const FP& p, long n, int ci, int Y, int X, long hw);

struct FP {
    const void* in; int in_f32; int Cin;
    int in_u8, in_norm, in_round16;
    const float* w; const float* bias;
    f16* out; long out_gstride; f16* out2; long out2_gstride;
    int K; long npix; int H, W; int act;
    long out_lo, out2_lo;          // != 0: fp32-accurate mode -- the lo part fp16((f - hi) * 2^11) of every value goes this many elements behind its hi part
};

// One input value of the first conv: planar fp16 / fp32, or np2tensor of a uint8 HWC image (float32(u8) / 255, BGR -> RGB flip as in
// colors.py:5-21, optional ((x - 0.5) * 2).clamp(-1, 1), optional rounding to fp16) -- bit for bit what the separate pass produces.
__device__ __forceinline__ float first_conv_input(const FP& p, long n, int ci, int Y, int X, long hw) {
    if (p.in_u8) {
        int sc = ci;
        if (p.Cin % 3 == 0) sc = p.Cin - 1 - ci; else if (p.Cin == 4 && ci < 3) sc = 2 - ci;
        float v = __fdiv_rn((float)((const uint8_t*)p.in)[(n * hw + (long)Y * p.W + X) * p.Cin + sc], 255.0f);
        if (p.in_norm) v = fminf(fmaxf(__fmul_rn(__fsub_rn(v, 0.5f), 2.0f), -1.0f), 1.0f);
        if (p.in_round16) v = (float)(f16)v;
        return v;
    }
    const long o = (n * p.Cin + ci) * hw + (long)Y * p.W + X;
    return p.in_f32 ? ((const float*)p.in)[o] : (float)((const f16*)p.in)[o];
}

// One input value behind FirstConvLaunch.in_map: operand = fp16(fma(alpha[ci], v, shift[ci])) of the value v the unmapped conv would multiply (first_conv_input).
__device__ __forceinline__ float first_conv_input_map(const FP& p, const float* map, long n, int ci, int Y, int X, long hw) {
    return (float)(f16)__builtin_fmaf(map[ci], first_conv_input(p, n, ci, Y, X, hw), map[p.Cin + ci]);
}

// The same conv on the matrix cores (K = 32 or 64 outputs): the 9 * Cin taps of a pixel are the k dimension of a 16 x 16 x 32 MFMA
// (27 of 32 for RGB; ceil(9 Cin / 32) steps), 16 consecutive pixels are its columns, 16 * NT output channels its rows.  A lane gathers
// the 8 patch values of its (pixel, k-octet) straight from the planar input -- 8 loads per lane and 16 pixels instead of the VALU
// kernel's 27 loads per lane and 8 pixels, no LDS -- and ends up with 4 * NT consecutive output channels of its pixel (rows permuted as in
// conv_pack): one or two 16-byte stores per output slab.  fp32 weights and fp32 input are split into an fp16 head and an fp16 remainder
// (w = wh + wl, x = xh + xl; wh*xh + wl*xh + wh*xl with fp32 accumulation), so the result keeps the fp32 VALU kernel's accuracy (product
// terms below 2^-22 relative dropped) although the MFMA operands are fp16.  Bound by its two 128 B/pixel stores, as it should be.
// (round 5: the walk.  The first form strode over 16-pixel groups of the flattened pixel index: two 64-bit divisions and eight bounds-tested, index-rebuilt
//  loads per lane and group -- ~500 VALU instructions for 8 MFMAs: 0.26 ms for a 1080p frame whose stores need 0.07-0.14.  Now a workgroup owns 64 columns x
//  FIRST_ROWS rows of one image, wave w its 16-column strip: a lane's eight patch offsets and column validity are fixed for the strip, a row costs eight loads
//  at base + offset, and the weight fragments are built once per FIRST_ROWS groups.  Same operands, same MFMA order: the same bits.)
constexpr int FIRST_ROWS = 16;
template <int NT, int STEPS, bool FAST16>                           // STEPS = ceil(9 Cin / 32): 1 for gray / RGB, 2 for 4..7 channels, 3 for 8; FAST16: planar fp16 input
__global__ __launch_bounds__(256) void first_conv_mfma(const FP p) {
    constexpr bool PRELU = false;
    constexpr bool IMAP = false;
    [[maybe_unused]] const float* const slope_p = nullptr;
    [[maybe_unused]] const float* const map_p = nullptr;
#include "conv_first_body.inc"
}

// act 8: f >= 0 ? f : slope[c] * f (nn.PReLU; constant slopes: ReLU, LeakyReLU(a)) -- the same body with the slopes of the lane's channels beside its biases
struct FPS { FP f; const float* slope; };
template <int NT, int STEPS, bool FAST16>
__global__ __launch_bounds__(256) void first_conv_mfma_prelu(const FPS ps) {
    constexpr bool PRELU = true;
    constexpr bool IMAP = false;
    const FP& p = ps.f;
    const float* const slope_p = ps.slope;
    [[maybe_unused]] const float* const map_p = nullptr;
#include "conv_first_body.inc"
}

// FirstConvLaunch.in_map: the operand is fp16(alpha[c] * v + shift[c]) of the loaded value v (the planar fp16 value, or np2tensor of the uint8 image) -- SPAN's
// `(x - mean) * img_range` in front of conv_1 without a pass of its own.  One fp32 fma, one rounding; a tap outside the image multiplies zero, AFTER the map (folding the
// shift into the bias would be wrong on the border ring).  The same body on its generic-input path; act 0 / 1 / 2 at run time.
struct FPM { FP f; const float* map; };
template <int NT, int STEPS, bool FAST16>
__global__ __launch_bounds__(256) void first_conv_mfma_map(const FPM pm) {
    static_assert(!FAST16, "the mapped operand is computed per value: the generic-input path");
    constexpr bool PRELU = false;
    constexpr bool IMAP = true;
    const FP& p = pm.f;
    [[maybe_unused]] const float* const slope_p = nullptr;
    const float* const map_p = pm.map;
#include "conv_first_body.inc"
}

}  // namespace

int first_conv_launch(const FirstConvLaunch& L, hipStream_t s) {
    if (L.K % 8 || L.K > 256 || L.K <= 0)
        return set_error(INNFER_ERR_UNSUPPORTED, "first conv: nf=%d must be a multiple of 8, <= 256", L.K);
    if (L.Cin < 1 || L.Cin > 8) return set_error(INNFER_ERR_UNSUPPORTED, "first conv: in_nc=%d unsupported", L.Cin);
    FP p{L.in, L.in_f32, L.Cin, L.in_u8, L.in_norm, L.in_round16, L.w, L.bias, L.out, L.out_gstride, L.out2, L.out2_gstride,
         L.K, (long)L.N * L.H * L.W, L.H, L.W, L.act, L.out_lo, L.out2_lo};
    if (L.act == 8 && (!L.slope || L.out_lo || L.out2_lo || (L.K != 32 && L.K != 64)))
        return set_error(L.slope ? INNFER_ERR_UNSUPPORTED : INNFER_ERR_INVALID, "first conv: act 8 (per-channel slope) needs the slope vector; built for 32 / 64 fp16 outputs (no split output)");
    if (L.in_map && (L.in_f32 || L.act == 8 || L.out_lo || L.out2_lo || (L.K != 32 && L.K != 64)))
        return set_error(INNFER_ERR_UNSUPPORTED, "first conv: the input map is built for fp16 or uint8 input, act 0..2 and 32 / 64 fp16 outputs (no split output)");
    const FPS ps{p, L.slope};
    const FPM pm{p, L.in_map};
    if (L.K == 32 || L.K == 64) {
        if (L.N > 65535 || (L.H + FIRST_ROWS - 1) / FIRST_ROWS > 65535) return set_error(INNFER_ERR_UNSUPPORTED, "first conv: %d images of %d rows exceed the launch grid", L.N, L.H);
        const dim3 grid((unsigned)((L.W + 63) / 64), (unsigned)((L.H + FIRST_ROWS - 1) / FIRST_ROWS), (unsigned)L.N);
        const int steps = (L.Cin * 9 + 31) / 32;
        const bool fast16 = !L.in_u8 && !L.in_f32 && (long)L.Cin * L.H * L.W < 0x7fffffffL;
        if (L.W >= (1 << 20) - 1) return set_error(INNFER_ERR_UNSUPPORTED, "first conv: %d columns", L.W);
#define FC(NT_, ST_) do { if (L.in_map) hipLaunchKernelGGL((first_conv_mfma_map<NT_, ST_, false>), grid, dim3(256), 0, s, pm); \
                          else if (L.act == 8) { if (fast16) hipLaunchKernelGGL((first_conv_mfma_prelu<NT_, ST_, true>), grid, dim3(256), 0, s, ps); \
                                              else hipLaunchKernelGGL((first_conv_mfma_prelu<NT_, ST_, false>), grid, dim3(256), 0, s, ps); } \
                          else if (fast16) hipLaunchKernelGGL((first_conv_mfma<NT_, ST_, true>), grid, dim3(256), 0, s, p); \
                          else hipLaunchKernelGGL((first_conv_mfma<NT_, ST_, false>), grid, dim3(256), 0, s, p); } while (0)
        if (L.K == 64) { if (steps == 1) FC(4, 1); else if (steps == 2) FC(4, 2); else FC(4, 3); }
        else { if (steps == 1) FC(2, 1); else if (steps == 2) FC(2, 2); else FC(2, 3); }
#undef FC
        INNFER_HIP(hipGetLastError());
        return INNFER_OK;
    }
    return set_error(INNFER_ERR_UNSUPPORTED, "first conv: K = %d (built: 32 or 64 outputs on the matrix cores)", L.K);
}

}  // namespace innfer
