// The adaptive interaction that ends both attention forms of a DAT block, on two channel-padded fp16 slabs X (gated per channel) and Y (gated per pixel):
//   s[pixel] = sigmoid(w2 . GELU(W1 X[pixel] + b1) + b2)          (spatial_interaction: 1x1 conv C -> hid, BatchNorm folded into W1 / b1 at load, exact GELU, 1x1 conv hid -> 1)
//   out      = fp16(fma(X, y[n][c], Y * s[pixel]))                (y = sigmoid(channel_interaction(mean_pixels(Y))): chan_attn.hip's pool + the GELU-hidden excite)
// ONE launch.  Four lanes own a pixel, as in layer_norm.hip: lane q holds channels 8 q .. 8 q + 7 of every group of X (at most 64 values).  Hidden unit j is the fma chain over
// the lane's channels in order (groups in order), the quad's butterfly (xor 1, then xor 2), + b1[j], GELU = f (1 + erff(f / sqrt 2)) / 2; s = 1 / (1 + expf(-(b2 + sum_j
// w2[j] h_j))) with the hidden units in order -- all fp32; the output is one fma and one fp16 rounding per value.  W1 sits in LDS ([hid][c_pad] fp32, zeros behind C: whatever
// X's pad channels hold is inert for s); channels >= C of out are written as zeros.  out may be X or Y (a lane reads all it writes before it writes).
// Memory bound: 2 x 64 bytes in, 64 out per pixel and group.
#include "common.h"

namespace innfer {

namespace {

constexpr int AIM_HID = 16;

struct AimArgs {
    const f16* x; long x_gs;
    const f16* y; long y_gs;
    f16* out; long out_gs;
    const float* gate;                   // [N][c_pad]
    const float* w1; const float* b1; const float* w2; float b2;
    long npix, HW; int C, c_pad, hid;
};

template <int NG>
__global__ __launch_bounds__(256) void aim_mix_kernel(const AimArgs p) {
    __shared__ float w1s[AIM_HID * NG * 32];
    for (int i = threadIdx.x; i < p.hid * NG * 32; i += 256) {
        const int j = i / (NG * 32), c = i - j * (NG * 32);
        w1s[i] = c < p.C ? p.w1[j * p.C + c] : 0.f;
    }
    __syncthreads();
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    const int q = (int)(i & 3);
    const bool live = (i >> 2) < p.npix;
    const long px = live ? (i >> 2) : p.npix - 1;          // (a quad beyond the last pixel repeats it and stores nothing: the exchanges below stay inside whole quads)
    const f16* xb = p.x + px * 32 + q * 8;
    float xv[NG][8];
#pragma unroll
    for (int g = 0; g < NG; ++g) {
        const f16x8 v = *(const f16x8*)(xb + g * p.x_gs);
#pragma unroll
        for (int e = 0; e < 8; ++e) xv[g][e] = g * 32 + q * 8 + e < p.C ? (float)v[e] : 0.f;
    }
    float z = p.b2;
    for (int j = 0; j < p.hid; ++j) {
        const float* wr = w1s + j * NG * 32 + q * 8;
        float a = 0.f;
#pragma unroll
        for (int g = 0; g < NG; ++g)
#pragma unroll
            for (int e = 0; e < 8; ++e) a = __builtin_fmaf(wr[g * 32 + e], xv[g][e], a);
        a += __shfl_xor(a, 1);
        a += __shfl_xor(a, 2);
        const float f = a + p.b1[j];
        const float hj = (0.5f * f) * (1.0f + erff(f * 0.70710678118654752440f));
        z = __builtin_fmaf(p.w2[j], hj, z);
    }
    const float sg = 1.0f / (1.0f + expf(-z));
    if (!live) return;
    const f16* yb = p.y + px * 32 + q * 8;
    f16* ob = p.out + px * 32 + q * 8;
    const float* gt = p.gate + (px / p.HW) * p.c_pad + q * 8;
#pragma unroll
    for (int g = 0; g < NG; ++g) {
        const f16x8 yv = *(const f16x8*)(yb + g * p.y_gs);
        f16x8 r;
#pragma unroll
        for (int e = 0; e < 8; ++e) r[e] = g * 32 + q * 8 + e < p.C ? (f16)__builtin_fmaf(xv[g][e], gt[g * 32 + e], (float)yv[e] * sg) : (f16)0.f;
        *(f16x8*)(ob + g * p.out_gs) = r;
    }
}

}  // namespace

// gate: N x c_pad device floats (the per-channel gate of every sample); w1 [hid][C], b1 [hid], w2 [hid]: device floats; c_pad a multiple of 64, <= 256; hid <= 16
int aim_mix_launch(const f16* x, long x_gs, const f16* y, long y_gs, f16* out, long out_gs, const float* gate, int N, long HW, int C, int c_pad, int hid, const float* w1,
                   const float* b1, const float* w2, float b2, hipStream_t s) {
    if (!x || !y || !out || !gate || !w1 || !b1 || !w2 || N <= 0 || HW <= 0) return set_error(INNFER_ERR_INVALID, "interaction mix: null argument or N=%d HW=%ld", N, HW);
    if (C < 1 || c_pad < C || c_pad > 256 || c_pad % 64) return set_error(INNFER_ERR_UNSUPPORTED, "interaction mix: C=%d in a slab of %d channels (built: slabs of 64, 128, 192 or 256 channels)", C, c_pad);
    if (hid < 1 || hid > AIM_HID) return set_error(INNFER_ERR_UNSUPPORTED, "interaction mix: %d hidden channels (built: 1 .. %d, C / 16 of at most 256 channels)", hid, AIM_HID);
    const long npix = (long)N * HW, nblk = (npix * 4 + 255) / 256;
    if (nblk > 0x7fffffffL) return set_error(INNFER_ERR_UNSUPPORTED, "interaction mix: %ld pixels exceed the launch grid", npix);
    if (x_gs < npix * 32 || y_gs < npix * 32 || out_gs < npix * 32) return set_error(INNFER_ERR_INVALID, "interaction mix: a group stride below %ld pixels x 32", npix);
    const int ng = c_pad / 32;
    GtScope gt(s, "interaction mix (per-pixel gate, two-branch blend)", (2.0 * C * hid + 3.0 * C) * (double)npix, 192.0 * ng * (double)npix);
    const AimArgs p{x, x_gs, y, y_gs, out, out_gs, gate, w1, b1, w2, b2, npix, HW, C, c_pad, hid};
    const dim3 grid((unsigned)nblk), block(256);
    switch (ng) {
        case 2: hipLaunchKernelGGL(aim_mix_kernel<2>, grid, block, 0, s, p); break;
        case 4: hipLaunchKernelGGL(aim_mix_kernel<4>, grid, block, 0, s, p); break;
        case 6: hipLaunchKernelGGL(aim_mix_kernel<6>, grid, block, 0, s, p); break;
        default: hipLaunchKernelGGL(aim_mix_kernel<8>, grid, block, 0, s, p); break;
    }
    INNFER_HIP(hipGetLastError());
    return INNFER_OK;
}

}  // namespace innfer
