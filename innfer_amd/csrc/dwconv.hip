// Depthwise 3 x 3 conv (groups = channels, zero padding 1) over a channel-padded fp16 slab of N x H x W pixels (DAT: attn.dwconv with its BatchNorm folded into taps and
// bias at load, and ffn.sg.conv).  A thread owns eight channels of one pixel: nine 16-byte loads (a tap outside the image is skipped: its zero adds nothing), per channel
//   f = bias[c];  f = fma(w[c][ky][kx], x[r + ky - 1][col + kx - 1][c], f)   in fp32, the taps row-major,
// then the epilogue and ONE fp16 rounding:
//   DW_NONE   f
//   DW_GELU   GELU(f), common.h fast_gelu (the exact erf form of the conv kernels' act 12)
//   DW_MUL    f * float(m[pixel][c]), m a second slab of the same shape (the gate x1 * g of DAT's feed-forward)
// Channels >= C are written as zeros whatever in, m and the parameters hold.  taps: fp32 [C][9], bias: fp32 [C].  out must not overlap in (a pixel reads its neighbours).
// A workgroup works inside ONE 32-channel group and keeps that group's taps and bias in LDS ([tap][channel]: a lane's eight channels are two 16-byte reads per tap; read
// from global memory per thread, with their stride of nine floats, the launch took 2.8 times as long).
// Memory bound: the nine loads of a pixel meet in L1 / L2; 64 bytes in (+ 64 of m), 64 out per pixel and group.
#include "common.h"

namespace innfer {

namespace {

enum { DW_NONE = 0, DW_GELU = 1, DW_MUL = 2 };

struct DwArgs {
    const f16* in; long in_gs;
    const f16* mul; long mul_gs;
    f16* out; long out_gs;
    const float* taps; const float* bias;
    long NHW; int H, W, C;
};

template <int EPI>
__global__ __launch_bounds__(256) void dwconv3x3_kernel(const DwArgs p) {
    __shared__ __attribute__((aligned(16))) float tw[10][32];          // the group's taps [tap][channel] and, in row 9, its bias: zeros behind C
    const int grp = blockIdx.y;
    for (int j = threadIdx.x; j < 320; j += 256) {
        const int k = j >> 5, ch = grp * 32 + (j & 31);
        tw[k][j & 31] = ch < p.C ? (k < 9 ? p.taps[ch * 9 + k] : p.bias[ch]) : 0.f;
    }
    __syncthreads();
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= p.NHW * 4) return;
    const int q = (int)(i & 3);
    const long px = i >> 2;
    const long hw = (long)p.H * p.W;
    const int rem = (int)(px % hw), r = rem / p.W, c = rem - r * p.W;
    const int c0 = grp * 32 + q * 8;
    f16x8 res;
    if (c0 >= p.C) {
#pragma unroll
        for (int e = 0; e < 8; ++e) res[e] = (f16)0.f;
    } else {
        float f[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) f[e] = tw[9][q * 8 + e];
        const f16* ib = p.in + grp * p.in_gs + px * 32 + q * 8;
#pragma unroll
        for (int ky = 0; ky < 3; ++ky)
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) {
                const int rr = r + ky - 1, cc = c + kx - 1;
                if (rr < 0 || rr >= p.H || cc < 0 || cc >= p.W) continue;
                const f16x8 x = *(const f16x8*)(ib + ((long)(ky - 1) * p.W + (kx - 1)) * 32);
#pragma unroll
                for (int e = 0; e < 8; ++e) f[e] = __builtin_fmaf(tw[ky * 3 + kx][q * 8 + e], (float)x[e], f[e]);
            }
        f16x8 m;
        if constexpr (EPI == DW_MUL) m = *(const f16x8*)(p.mul + grp * p.mul_gs + px * 32 + q * 8);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            float v = f[e];
            if constexpr (EPI == DW_GELU) v = fast_gelu(v);
            if constexpr (EPI == DW_MUL) v = v * (float)m[e];
            res[e] = c0 + e < p.C ? (f16)v : (f16)0.f;
        }
    }
    *(f16x8*)(p.out + grp * p.out_gs + px * 32 + q * 8) = res;
}

}  // namespace

// c_pad: channels of the slabs (a multiple of 32, >= C, <= 512); epilogue 0 none | 1 GELU | 2 times `mul`; taps [C][9] and bias [C]: device floats
int dwconv3x3_launch(const f16* in, long in_gs, const f16* mul, long mul_gs, f16* out, long out_gs, int N, int H, int W, int C, int c_pad, const float* taps, const float* bias,
                     int epilogue, hipStream_t s) {
    if (!in || !out || !taps || !bias || N <= 0 || H <= 0 || W <= 0) return set_error(INNFER_ERR_INVALID, "depthwise conv: null argument or N=%d H=%d W=%d", N, H, W);
    if (epilogue < DW_NONE || epilogue > DW_MUL) return set_error(INNFER_ERR_UNSUPPORTED, "depthwise conv: epilogue %d (built: 0 none, 1 GELU, 2 times a second slab)", epilogue);
    if (C < 1 || c_pad < C || c_pad > 512 || c_pad % 32) return set_error(INNFER_ERR_UNSUPPORTED, "depthwise conv: C=%d in a slab of %d channels (built: whole groups of 32, at most 512 channels)", C, c_pad);
    const long NHW = (long)N * H * W;
    if ((long)H * W > 0x7fffffffL || (NHW * 4 + 255) / 256 > 0x7fffffffL) return set_error(INNFER_ERR_UNSUPPORTED, "depthwise conv: %ld pixels exceed the launch grid", NHW);
    if (in_gs < NHW * 32 || out_gs < NHW * 32) return set_error(INNFER_ERR_INVALID, "depthwise conv: a group stride below N * H * W * 32");
    if (epilogue == DW_MUL && (!mul || mul_gs < NHW * 32)) return set_error(INNFER_ERR_INVALID, "depthwise conv: the multiplier slab is null or its group stride below N * H * W * 32");
    if (in == out) return set_error(INNFER_ERR_INVALID, "depthwise conv: in place (a pixel reads its neighbours)");
    const int ng = c_pad / 32;
    GtScope gt(s, epilogue == DW_GELU ? "depthwise 3x3 + GELU" : epilogue == DW_MUL ? "depthwise 3x3 x gate" : "depthwise 3x3", 18.0 * C * (double)NHW,
               (epilogue == DW_MUL ? 192.0 : 128.0) * ng * (double)NHW);
    const DwArgs p{in, in_gs, mul, mul_gs, out, out_gs, taps, bias, NHW, H, W, C};
    const dim3 grid((unsigned)((NHW * 4 + 255) / 256), (unsigned)ng), block(256);
    if (epilogue == DW_GELU) hipLaunchKernelGGL(dwconv3x3_kernel<DW_GELU>, grid, block, 0, s, p);
    else if (epilogue == DW_MUL) hipLaunchKernelGGL(dwconv3x3_kernel<DW_MUL>, grid, block, 0, s, p);
    else hipLaunchKernelGGL(dwconv3x3_kernel<DW_NONE>, grid, block, 0, s, p);
    INNFER_HIP(hipGetLastError());
    return INNFER_OK;
}

}  // namespace innfer
