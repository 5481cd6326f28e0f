// Depthwise 5 x 5 conv (groups = channels, zero padding 2) with GELU and its own input added back, over a channel-padded fp16 slab of N x H x W pixels (SRFormer's
// ConvFFN: fc2 reads h + GELU(dwconv(h))).  Per channel
//   f = bias[c];  f = fma(w[c][ky][kx], x[r + ky - 2][col + kx - 2][c], f)   in fp32, the taps row-major (a tap outside the image is a zero operand),
//   out = fp16(x[r][col][c] + GELU(f))                                       common.h fast_gelu, the sum in fp32, ONE rounding.
// Channels >= C are written as zeros whatever `in` and the parameters hold.  taps: fp32 [C][25], bias: fp32 [C].  out must not overlap in (a pixel reads its neighbours).
// A workgroup works inside ONE 32-channel group on a tile of 16 x 16 pixels: the tile and its halo of 2 (20 x 20 pixels x 32 channels, 25.6 KB) are staged in LDS with
// 16-byte loads, zeros outside the image; the group's taps [25][32] and its bias live in LDS beside it (zeros behind C).  A thread owns one channel octet of FOUR pixels of
// a column, four rows apart: a tap's eight weights are read once (two ds_read_b128) for four pixels; a quarter-wave's lanes read consecutive 16-byte pieces of a tile row.
// 25 taps read through L1 as dwconv.hip reads its nine would be 25 global loads per pixel and octet; here a pixel is loaded 1.56 times.
#include "common.h"
#include "test_entry.h"

namespace innfer {

namespace {

constexpr int DW5_T = 16, DW5_S = DW5_T + 4;       // tile side, staged side

struct Dw5Args {
    const f16* in; long in_gs;
    f16* out; long out_gs;
    const float* taps; const float* bias;
    int N, H, W, C, tx, ty;
};

__global__ __launch_bounds__(256) void dwconv5x5_gelu_add_kernel(const Dw5Args p) {
    __shared__ __attribute__((aligned(16))) f16 tile[DW5_S * DW5_S * 32];
    __shared__ __attribute__((aligned(16))) float tw[26][32];          // the group's taps [tap][channel] and, in row 25, its bias: zeros behind C
    const int grp = blockIdx.y, tid = threadIdx.x;
    const int b = blockIdx.x, bx = b % p.tx, by = (b / p.tx) % p.ty, n = b / (p.tx * p.ty);
    const int r0 = by * DW5_T, c0 = bx * DW5_T;
    for (int j = tid; j < 26 * 32; j += 256) {
        const int k = j >> 5, ch = grp * 32 + (j & 31);
        tw[k][j & 31] = ch < p.C ? (k < 25 ? p.taps[ch * 25 + k] : p.bias[ch]) : 0.f;
    }
    const f16* ib = p.in + grp * p.in_gs + (long)n * p.H * p.W * 32;
    f16x8 zero8;
#pragma unroll
    for (int e = 0; e < 8; ++e) zero8[e] = (f16)0.f;
    for (int j = tid; j < DW5_S * DW5_S * 4; j += 256) {
        const int q = j & 3, sp = j >> 2, sr = sp / DW5_S, sc = sp - sr * DW5_S;
        const int r = r0 + sr - 2, c = c0 + sc - 2;
        const bool in = r >= 0 && r < p.H && c >= 0 && c < p.W;
        *(f16x8*)(tile + sp * 32 + q * 8) = in ? *(const f16x8*)(ib + ((long)r * p.W + c) * 32 + q * 8) : zero8;
    }
    __syncthreads();
    const int q = tid & 3, col = (tid >> 2) & 15, row = tid >> 6;       // pixels (row + 4 i, col), i = 0 .. 3
    if (c0 + col >= p.W) return;
    float f[4][8];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int e = 0; e < 8; ++e) f[i][e] = tw[25][q * 8 + e];
#pragma unroll 1
    for (int ky = 0; ky < 5; ++ky)          // (a tap row per trip: unrolled over all 25 taps the compiler hoists every read and spills)
#pragma unroll
        for (int kx = 0; kx < 5; ++kx) {
            float wv[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) wv[e] = tw[ky * 5 + kx][q * 8 + e];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const f16x8 x = *(const f16x8*)(tile + ((row + 4 * i + ky) * DW5_S + col + kx) * 32 + q * 8);
#pragma unroll
                for (int e = 0; e < 8; ++e) f[i][e] = __builtin_fmaf(wv[e], (float)x[e], f[i][e]);
            }
        }
    const int ch0 = grp * 32 + q * 8;
    f16* ob = p.out + grp * p.out_gs + (long)n * p.H * p.W * 32 + q * 8;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int r = r0 + row + 4 * i;
        if (r >= p.H) continue;
        const f16x8 x = *(const f16x8*)(tile + ((row + 4 * i + 2) * DW5_S + col + 2) * 32 + q * 8);
        f16x8 res;
#pragma unroll
        for (int e = 0; e < 8; ++e) res[e] = ch0 + e < p.C ? (f16)((float)x[e] + fast_gelu(f[i][e])) : (f16)0.f;
        *(f16x8*)(ob + ((long)r * p.W + c0 + col) * 32) = res;
    }
}

int dwconv5_refuse(const void* in, long in_gs, const void* out, long out_gs, int N, int H, int W, int C, int c_pad, const void* taps, const void* bias) {
    if (!in || !out || !taps || !bias || N <= 0 || H <= 0 || W <= 0) return set_error(INNFER_ERR_INVALID, "depthwise 5x5: null argument or N=%d H=%d W=%d", N, H, W);
    if (C < 1 || c_pad < C || c_pad > 1024 || c_pad % 32) return set_error(INNFER_ERR_UNSUPPORTED, "depthwise 5x5: C=%d in a slab of %d channels (built: whole groups of 32, at most 1024 channels)", C, c_pad);
    const long NHW = (long)N * H * W;
    const long tiles = (long)N * ((H + DW5_T - 1) / DW5_T) * ((W + DW5_T - 1) / DW5_T);
    if (tiles > 0x7fffffffL) return set_error(INNFER_ERR_UNSUPPORTED, "depthwise 5x5: %ld pixels exceed the launch grid", NHW);
    if (in_gs < NHW * 32 || out_gs < NHW * 32) return set_error(INNFER_ERR_INVALID, "depthwise 5x5: a group stride below N * H * W * 32");
    const int ng = c_pad / 32;
    const f16 *i0 = (const f16*)in, *i1 = i0 + (ng - 1) * in_gs + NHW * 32, *o0 = (const f16*)out, *o1 = o0 + (ng - 1) * out_gs + NHW * 32;
    if (i0 < o1 && o0 < i1) return set_error(INNFER_ERR_INVALID, "depthwise 5x5: out overlaps in (a pixel reads its neighbours)");
    return INNFER_OK;
}

}  // namespace

// c_pad: channels of the slabs (a multiple of 32, >= C, <= 1024); taps [C][25] and bias [C]: device floats
int dwconv5x5_gelu_add_launch(const f16* in, long in_gs, f16* out, long out_gs, int N, int H, int W, int C, int c_pad, const float* taps, const float* bias, hipStream_t s) {
    if (int rc = dwconv5_refuse(in, in_gs, out, out_gs, N, H, W, C, c_pad, taps, bias)) return rc;
    const int ng = c_pad / 32, tx = (W + DW5_T - 1) / DW5_T, ty = (H + DW5_T - 1) / DW5_T;
    GtScope gt(s, "depthwise 5x5 + GELU + input", 50.0 * C * (double)N * H * W, 128.0 * ng * (double)N * H * W);
    const Dw5Args p{in, in_gs, out, out_gs, taps, bias, N, H, W, C, tx, ty};
    hipLaunchKernelGGL(dwconv5x5_gelu_add_kernel, dim3((unsigned)(N * tx * ty), (unsigned)ng), dim3(256), 0, s, p);
    INNFER_HIP(hipGetLastError());
    return INNFER_OK;
}

// The launch alone, for tests: dwconv5x5_gelu_add_launch, the code the network runs.  h_taps [C][25], h_bias [C]: host floats.  Uploads, launches, waits.
extern "C" int innfer_dwconv5x5_gelu_add(const void* d_in, int64_t in_gs, void* d_out, int64_t out_gs, int N, int H, int W, int C, int c_pad, const float* h_taps,
                                         const float* h_bias, void* stream) {
    if (int rc = dwconv5_refuse(d_in, (long)in_gs, d_out, (long)out_gs, N, H, W, C, c_pad, h_taps, h_bias)) return rc;
    Upload b("dwconv5x5_gelu_add", {{h_taps, (size_t)C * 25}, {h_bias, (size_t)C}});
    int rc = b.rc;
    if (rc == INNFER_OK) rc = dwconv5x5_gelu_add_launch((const f16*)d_in, (long)in_gs, (f16*)d_out, (long)out_gs, N, H, W, C, c_pad, b.d, b.d + (size_t)C * 25, (hipStream_t)stream);
    return finish("dwconv5x5_gelu_add", rc, stream);
}

}  // namespace innfer
