// First convolution of a BasicSR RRDBNet with scale 2 or 1 (Real-ESRGAN x2plus and kin): conv3x3(pixel_unshuffle(x, r)) of an RGB image, r = 2 | 4, with the
// unshuffle folded into the conv's addressing -- the 12- / 48-channel tensor is never written.
//
// Per colour channel c the conv is a 3r x 3r window of the full-resolution image at stride r: channel c r^2 + i r + j, tap (ky, kx) of LR pixel (Y, X) reads image
// pixel (c, r (Y + ky - 1) + i, r (X + kx - 1) + j) = (c, r Y - r + wy, r X - r + wx) with window row wy = r ky + i and window column wx = r kx + j.  The k dimension
// of the MFMA is therefore ordered (c, wy, wx) (first_unshuffle_pack permutes the weights to match): consecutive k are adjacent image pixels of one row.
// k = 27 r^2 = 108 (4 steps of v_mfma_f32_16x16x32_f16) or 432 (14 steps).  At 14 steps the hi and lo weight fragments of conv_first.hip's register-resident form
// would take ~450 VGPRs, so here the packed fragments live in LDS: [step][16-channel tile][hi | lo][lane][8 fp16] = 2 KB per (step, tile) -- 32 KB (r 2) or 112 KB
// (r 4) for 64 outputs, inside gfx950's 160 KB.  A wave's ds_read_b128 of one fragment is 64 lanes x 16 consecutive bytes: every 16-lane group covers one whole
// 256-byte bank row, conflict-free without a swizzle.
//
// Sizes that are not a multiple of r: the image is padded bottom / right to the next multiple with `reflect` (index 2 (H - 1) - y, pad <= 3) as BasicSR's inference
// tools do; the reflected index is part of the addressing here and the caller crops the result.  A tap whose LR pixel lies outside the LR grid is zero.
//
// Input kinds, output slabs ((hi, lo) pairs in the fp32-accurate mode), split arithmetic (wh xh + wl xh + wh xl, fp32 accumulation), row order of the output
// channels and the activation form are those of first_conv_mfma (conv_first.hip); so is the walk: a workgroup owns 64 columns x 16 rows of the LR grid of one image,
// wave w its 16-column strip.
#include "common.h"
#include <type_traits>

namespace innfer {
namespace {

struct UP {
    const void* in; int in_norm, in_round16;
    const f16* wpk; const float* bias;
    f16* out; long out_gstride; f16* out2; long out2_gstride;
    int H, W;                      // the image
    int h, w;                      // the LR grid: ceil(H / r) x ceil(W / r)
    int act;
    long out_lo, out2_lo;
};

constexpr int UNSH_ROWS = 16;

constexpr int unsh_steps(int r) { return (27 * r * r + 31) / 32; }

// KIND: 0 planar fp16, 1 planar fp32, 2 uint8 HWC BGR (np2tensor as the prologue, bit for bit first_conv_input's arithmetic)
template <int NT, int R, int KIND>
__global__ __launch_bounds__(256) void first_conv_unshuffle(const UP p) {
    constexpr int R3 = 3 * R, WIN = R3 * R3, NK = 3 * WIN, STEPS = unsh_steps(R);
    extern __shared__ __attribute__((aligned(16))) char smem[];
    for (int i = threadIdx.x; i < STEPS * NT * 128; i += 256) ((u32x4*)smem)[i] = ((const u32x4*)p.wpk)[i];
    __syncthreads();
    const int lane = threadIdx.x & 63, li = lane & 15, lg = lane >> 4;
    const int xs = blockIdx.x * 64 + (int)(threadIdx.x >> 6) * 16;   // the wave's strip
    if (xs >= p.w) return;                                            // (a strip beyond the grid: whole waves, behind the only barrier)
    const int X = xs + li;
    const int Y0 = blockIdx.y * UNSH_ROWS, Y1 = min(Y0 + UNSH_ROWS, p.h);
    const long n = blockIdx.z;
    const bool live = X < p.w;
    const long ihw = (long)p.H * p.W;
    const int gh = R * p.h, gw = R * p.w;                             // the padded image
    f32x4 bias[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) bias[t] = *(const f32x4*)(p.bias + 32 * (t >> 1) + 8 * lg + 4 * (t & 1));
    const bool any_lo = KIND == 1 || (KIND == 2 && !p.in_round16);
    const f16x8* frag = (const f16x8*)smem + lane;
    for (int Y = Y0; Y < Y1; ++Y) {
        f32x4 acc[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t) acc[t] = bias[t];
        // (the fragments are in LDS, so the step may be a run-time index: unrolled 14 times (r 4) the loop-invariant window coordinates of all 112 elements
        //  are hoisted and spill -- 1.2 KB of scratch per lane; rolled, a step's eight are recomputed, a few VALU operations per load, in 50 .. 90 VGPRs)
#pragma unroll 1
        for (int st = 0; st < STEPS; ++st) {
            // the lane's eight patch values of this step: unconditional loads from an address inside the image (a dead element reads pixel (0, 0) and is zeroed
            // by the select), independent of each other
            f16x8 xh, xl;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const int kk = st * 32 + lg * 8 + e;
                const int c = kk / WIN, rem = kk - c * WIN, wy = rem / R3, wx = rem - wy * R3;
                int iy = R * Y - R + wy, ix = R * X - R + wx;
                const bool ok = live && kk < NK && iy >= 0 && iy < gh && ix >= 0 && ix < gw;
                if (iy >= p.H) iy = 2 * (p.H - 1) - iy;               // reflect pad of the bottom / right rim (launch: pad < H, W)
                if (ix >= p.W) ix = 2 * (p.W - 1) - ix;
                const long px = ok ? (long)iy * p.W + ix : 0;
                const int cc = ok ? c : 0;
                float v;
                if constexpr (KIND == 0) v = (float)((const f16*)p.in)[(n * 3 + cc) * ihw + px];
                else if constexpr (KIND == 1) v = ((const float*)p.in)[(n * 3 + cc) * ihw + px];
                else {
                    v = __fdiv_rn((float)((const uint8_t*)p.in)[(n * ihw + px) * 3 + (2 - cc)], 255.0f);
                    if (p.in_norm) v = fminf(fmaxf(__fmul_rn(__fsub_rn(v, 0.5f), 2.0f), -1.0f), 1.0f);
                    if (p.in_round16) v = (float)(f16)v;
                }
                v = ok ? v : 0.f;
                const f16 hh = (f16)v;
                xh[e] = hh;
                xl[e] = KIND == 0 ? (f16)0.f : (f16)(v - (float)hh);
            }
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                const f16x8 wh = frag[((st * NT + t) * 2 + 0) * 64], wl = frag[((st * NT + t) * 2 + 1) * 64];
                acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wh, xh, acc[t], 0, 0, 0);
                acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wl, xh, acc[t], 0, 0, 0);
                if (any_lo) acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wh, xl, acc[t], 0, 0, 0);
            }
        }
        if (!live) continue;
        const long pix = (n * p.h + Y) * p.w + X;
        f16 h[4 * NT], l[4 * NT];
        auto finish = [&](auto act_tag) __attribute__((always_inline)) {
            constexpr int ACT = decltype(act_tag)::value;
#pragma unroll
            for (int t = 0; t < NT; ++t)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    float f = acc[t][j];
                    if (ACT == 1) f = __builtin_amdgcn_fmed3f(f, 0.2f * f, 3.0e38f);
                    else if (ACT == 2) f = __builtin_amdgcn_fmed3f(f, 0.f, 3.0e38f);
                    h[4 * t + j] = (f16)f;
                    l[4 * t + j] = (f16)((f - (float)h[4 * t + j]) * 2048.0f);
                }
        };
        if (p.act == 1) finish(std::integral_constant<int, 1>{}); else if (p.act == 2) finish(std::integral_constant<int, 2>{}); else finish(std::integral_constant<int, 0>{});
        const long o = pix * 32 + 8 * lg;
#pragma unroll
        for (int q = 0; q < NT / 2; ++q) {                            // plane q: tiles 2 q, 2 q + 1
            f16x8 v;
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = h[8 * q + e];
            *(f16x8*)(p.out + q * p.out_gstride + o) = v;
            if (p.out2) *(f16x8*)(p.out2 + q * p.out2_gstride + o) = v;
            if (p.out_lo) {
#pragma unroll
                for (int e = 0; e < 8; ++e) v[e] = l[8 * q + e];
                *(f16x8*)(p.out + p.out_lo + q * p.out_gstride + o) = v;
                if (p.out2) *(f16x8*)(p.out2 + p.out2_lo + q * p.out2_gstride + o) = v;
            }
        }
    }
}

template <int NT, int R, int KIND>
int launch_one(const UP& p, dim3 grid, hipStream_t s) {
    constexpr int LDS = unsh_steps(R) * NT * 2048;
    static std::atomic<unsigned long long> attr_done{0};
    INNFER_HIP(ensure_lds_attr(first_conv_unshuffle<NT, R, KIND>, LDS, attr_done));
    hipLaunchKernelGGL((first_conv_unshuffle<NT, R, KIND>), grid, dim3(256), LDS, s, p);
    INNFER_HIP(hipGetLastError());
    return INNFER_OK;
}

template <int NT, int R>
int launch_kind(const UP& p, int kind, dim3 grid, hipStream_t s) {
    if (kind == 0) return launch_one<NT, R, 0>(p, grid, s);
    if (kind == 1) return launch_one<NT, R, 1>(p, grid, s);
    return launch_one<NT, R, 2>(p, grid, s);
}

}  // namespace

size_t first_unshuffle_packed_bytes(int K, int r) { return (size_t)unsh_steps(r) * (K / 16) * 2048; }

// w [K][3 r^2][3][3] (torch's pixel_unshuffle channel order c r^2 + i r + j) -> the kernel's LDS image: [step][tile][hi | lo][lane][8], k ordered (c, wy, wx)
void first_unshuffle_pack(const float* w, int K, int r, void* packed) {
    const int NT = K / 16, R3 = 3 * r, WIN = R3 * R3, NK = 3 * WIN, steps = unsh_steps(r), Cin = 3 * r * r;
    f16* d = (f16*)packed;
    for (int st = 0; st < steps; ++st)
        for (int t = 0; t < NT; ++t)
            for (int lane = 0; lane < 64; ++lane)
                for (int e = 0; e < 8; ++e) {
                    const int li = lane & 15, lg = lane >> 4;
                    const int oc = 32 * (t >> 1) + 8 * (li >> 2) + 4 * (t & 1) + (li & 3);      // the plane row order of first_conv_mfma
                    const int kk = st * 32 + lg * 8 + e;
                    float v = 0.f;
                    if (kk < NK) {
                        const int c = kk / WIN, rem = kk - c * WIN, wy = rem / R3, wx = rem - wy * R3;
                        const int ch = c * r * r + (wy % r) * r + wx % r;
                        v = w[(((size_t)oc * Cin + ch) * 3 + wy / r) * 3 + wx / r];
                    }
                    const f16 hi = (f16)v;
                    d[(((size_t)(st * NT + t) * 2 + 0) * 64 + lane) * 8 + e] = hi;
                    d[(((size_t)(st * NT + t) * 2 + 1) * 64 + lane) * 8 + e] = (f16)(v - (float)hi);
                }
}

int first_unshuffle_launch(const FirstUnshuffleLaunch& L, hipStream_t s) {
    if (L.r != 2 && L.r != 4) return set_error(INNFER_ERR_UNSUPPORTED, "first conv (unshuffle): factor %d (built: 2, 4)", L.r);
    if (L.Cin != 3) return set_error(INNFER_ERR_UNSUPPORTED, "first conv (unshuffle): in_nc=%d (built: 3 -- 12 or 48 channels behind the unshuffle)", L.Cin);
    if (L.K != 32 && L.K != 64) return set_error(INNFER_ERR_UNSUPPORTED, "first conv (unshuffle): K = %d (built: 32 or 64 outputs on the matrix cores)", L.K);
    if (L.N <= 0 || L.H <= 0 || L.W <= 0) return set_error(INNFER_ERR_INVALID, "first conv (unshuffle): bad shape %dx%dx%d", L.N, L.H, L.W);
    const int h = (L.H + L.r - 1) / L.r, w = (L.W + L.r - 1) / L.r;
    if ((h * L.r != L.H && L.H < 4) || (w * L.r != L.W && L.W < 4))
        return set_error(INNFER_ERR_UNSUPPORTED, "first conv (unshuffle): a %d x %d image is reflect-padded to a multiple of %d, which needs at least 4 rows and columns", L.H, L.W, L.r);
    if (L.N > 65535 || (h + UNSH_ROWS - 1) / UNSH_ROWS > 65535) return set_error(INNFER_ERR_UNSUPPORTED, "first conv (unshuffle): %d images of %d rows exceed the launch grid", L.N, h);
    if ((long)L.r * w + L.r >= 0x7fffffffL / 2 || (long)L.r * h + L.r >= 0x7fffffffL / 2) return set_error(INNFER_ERR_UNSUPPORTED, "first conv (unshuffle): %d x %d image", L.H, L.W);
    UP p{L.in, L.in_norm, L.in_round16, (const f16*)L.wpk, L.bias, L.out, L.out_gstride, L.out2, L.out2_gstride, L.H, L.W, h, w, L.act, L.out_lo, L.out2_lo};
    const dim3 grid((unsigned)((w + 63) / 64), (unsigned)((h + UNSH_ROWS - 1) / UNSH_ROWS), (unsigned)L.N);
    const int kind = L.in_u8 ? 2 : L.in_f32 ? 1 : 0;
    if (L.K == 64) return L.r == 2 ? launch_kind<4, 2>(p, kind, grid, s) : launch_kind<4, 4>(p, kind, grid, s);
    return L.r == 2 ? launch_kind<2, 2>(p, kind, grid, s) : launch_kind<2, 4>(p, kind, grid, s);
}

}  // namespace innfer
