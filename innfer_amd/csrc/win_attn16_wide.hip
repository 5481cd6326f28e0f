// 16 x 16 window attention for heads WIDER than one 32-channel group (DRCT: the dense group grows the token width by 32 per block and changes the head count with it --
// C 180 / 6 heads gives head dims 30, 53, 122, 46, 77).  A head owns G = ceil(d / 32) consecutive 32-channel groups, G in {2, 3, 4}: ONE launch for all windows and heads.
//   qkv slab   3 nH G channel groups of 32: groups h G .. h G + G - 1 = q of head h (d real channels, then zeros; the d^-0.5 already inside the weights), then the nH G
//              groups of k, then those of v
//   out slab   nH G groups: head h's result at the query pixels in groups h G .. h G + G - 1, channels >= d of the head written as zeros
// Window geometry, the roll as addresses (shift 0 | 8), the mask and the dense [nH][256 query][256 key] fp32 bias as the C operand are those of win_attn16_kernel<16>
// (win_attn16.hip); the arithmetic is win_attn_core.h's.  Per block a wave issues 8 G v_mfma_f32_16x16x32_f16 for S (chained over the G channel steps in the same
// accumulator) and 8 G for O.
// Resources: 64 queries a wave would need 16 G VGPRs of Q fragments, 32 G of O accumulators and 64 of scores (352 at G = 4: one wave per SIMD).  So a workgroup is EIGHT waves
// and a wave owns 32 queries: 8 G + 16 G + 32 registers of state, which leaves every instantiation under 256 registers (two waves per SIMD from ONE workgroup) with no scratch:
// 127 / 159 / 186 VGPRs, no AGPRs, for G = 2 / 3 / 4 as the compiler reports them (tests/test_drct_host.py asserts the scratch condition at compile time).
// V^T of the window is staged once per workgroup in LDS ([32 G channels][256 slots + 8] fp16: 33.8 / 50.7 / 67.6 KB); K fragments come from the slab (L2 serves the seven
// re-reads of a window's K by the other waves).
#include "win_attn_core.h"

namespace innfer {

namespace {

struct WinAttn16W {
    const f16* qkv; long gs;
    f16* out; long out_gs;
    const float* relb;
    int N, Hp, Wp, nH, d, shift;
};

template <int G>
__global__ __launch_bounds__(512) void win_attn16_wide_kernel(const WinAttn16W p) {
    constexpr int VROW = 264;                                   // fp16 elements of a V^T row (a multiple of 8: 16-byte aligned fragments; rows start on different banks)
    extern __shared__ __attribute__((aligned(16))) f16 vt[];    // [32 G][VROW]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, lg = lane >> 4;
    const int nwx = p.Wp >> 4, nw = nwx * (p.Hp >> 4);
    const int item = blockIdx.x;
    const int w = item % nw, h = (item / nw) % p.nH, n = item / (nw * p.nH);
    const int wy = w / nwx, wx = w - wy * nwx;
    const long img = (long)n * p.Hp * p.Wp;
    // element offset of token t's pixel inside a slab group: pixel ((r + shift) mod Hp, (c + shift) mod Wp) of the stored frame
    auto pix = [&](int t) -> long {
        int r = wy * 16 + (t >> 4) + p.shift, c = wx * 16 + (t & 15) + p.shift;
        if (r >= p.Hp) r -= p.Hp;
        if (c >= p.Wp) c -= p.Wp;
        return (img + (long)r * p.Wp + c) * 32;
    };
    const long sec = (long)p.nH * G * p.gs;                      // q -> k -> v
    const f16* qb = p.qkv + (long)h * G * p.gs + 8 * lg;
    const f16* kb = qb + sec;
    const f16* vb = p.qkv + 2 * sec + (long)h * G * p.gs;
    for (int pc = tid; pc < 256 * 4 * G; pc += 512) {            // V^T into LDS: piece (key, channel octet) -> eight rows, the key's slot inside its 64-key block
        const int tok = pc / (4 * G), oct = pc - tok * (4 * G);
        wa::scatter_vt<VROW>(vt, tok, oct, *(const f16x8*)(vb + (long)(oct >> 2) * p.gs + pix(tok) + 8 * (oct & 3)));
    }
    long px[2];
    f16x8 qf[2][G];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        px[t] = pix(32 * wave + 16 * t + li);
#pragma unroll
        for (int g = 0; g < G; ++g) qf[t][g] = *(const f16x8*)(qb + (long)g * p.gs + px[t]);
    }
    __syncthreads();

    const bool masked = p.shift && (wy == (p.Hp >> 4) - 1 || wx == nwx - 1);      // (workgroup-uniform) the windows that wrap
    int lq[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) lq[t] = wa::label_sq<16>(wy, wx, 32 * wave + 16 * t + li, p.Hp, p.Wp);
    const float* rb = p.relb + (long)h * 65536 + (long)(32 * wave + li) * 256 + 4 * lg;
    const f32x4 z4 = {0.f, 0.f, 0.f, 0.f};
    float m[2], l[2];
    f32x4 o[2 * G][2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        m[t] = -3.0e38f; l[t] = 0.f;
#pragma unroll
        for (int td = 0; td < 2 * G; ++td) o[td][t] = z4;
    }
#pragma unroll 1
    for (int b = 0; b < 4; ++b) {
        long ko[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) ko[t] = pix(64 * b + 16 * t + li);
        // s[tk][tq][j]: key 64 b + 16 tk + 4 lg + j, query 32 wave + 16 tq + li
        f32x4 s[4][2];
#pragma unroll
        for (int tq = 0; tq < 2; ++tq)
#pragma unroll
            for (int tk = 0; tk < 4; ++tk) s[tk][tq] = *(const f32x4*)(rb + 16 * tq * 256 + 64 * b + 16 * tk);
#pragma unroll
        for (int g = 0; g < G; ++g) {
            f16x8 kf[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) kf[t] = *(const f16x8*)(kb + (long)g * p.gs + ko[t]);
#pragma unroll
            for (int tq = 0; tq < 2; ++tq)
#pragma unroll
                for (int tk = 0; tk < 4; ++tk) s[tk][tq] = __builtin_amdgcn_mfma_f32_16x16x32_f16(kf[tk], qf[tq][g], s[tk][tq], 0, 0, 0);
        }
        if (masked) wa::mask_block(s, lq, 64 * b + 4 * lg, [&](int key) { return wa::label_sq<16>(wy, wx, key, p.Hp, p.Wp); });
        f16x8 pf[2][2];                                  // pf[tq][ks]: the B fragment of key step ks of this block
        wa::softmax_block(s, m, l, o, pf);
        wa::pv_block<2, 2 * G, VROW>(vt + 64 * b, li, lg, pf, o);
    }
    wa::store_out(p.out + (long)h * G * p.out_gs, p.out_gs, px, o, l, p.d, lg, [](int) { return false; });
}

template <int G>
int wa16w_go(const WinAttn16W& p, unsigned total, hipStream_t s) {
    static std::atomic<unsigned long long> done{0};
    constexpr int lds = 32 * G * 264 * 2;
    INNFER_HIP(ensure_lds_attr(win_attn16_wide_kernel<G>, lds, done));
    hipLaunchKernelGGL(win_attn16_wide_kernel<G>, dim3(total), dim3(512), lds, s, p);
    INNFER_HIP(hipGetLastError());
    return INNFER_OK;
}

}  // namespace

// relb: dense fp32 [nH][256 query][256 key]; Hp, Wp multiples of 16; 32 < d <= 128; shift 0 | 8.  A refusal launches nothing.
int win_attn16_wide_launch(const f16* qkv, long gs, f16* out, long out_gs, const float* relb, int N, int Hp, int Wp, int nH, int d, int shift, hipStream_t s) {
    if (int rc = wa::refuse_frame("wide window attention 16", qkv, out, relb, N, Hp, Wp, 16)) return rc;
    if (nH < 1 || nH > 8 || d <= 32 || d > 128)
        return set_error(INNFER_ERR_UNSUPPORTED, "wide window attention 16: %d heads of %d channels (built: <= 8 heads of 33 .. 128 channels; win_attn16_launch takes d <= 32)", nH, d);
    if (shift != 0 && shift != 8) return set_error(INNFER_ERR_UNSUPPORTED, "wide window attention 16: shift %d (built: 0, 8)", shift);
    const long total = (long)N * nH * (Hp >> 4) * (Wp >> 4);
    if (int rc = wa::refuse_strides_grid("wide window attention 16", gs, out_gs, N, Hp, Wp, total, 0x7fffffffL)) return rc;
    const int g = (d + 31) / 32;
    GtScope gt(s, "window attention (16 x 16, heads of 2 .. 4 groups)", 4.0 * 256 * 256 * d * (double)total, (double)total * (256.0 * 32 * g * 2 * 4 + 65536.0 * 4));
    const WinAttn16W p{qkv, gs, out, out_gs, relb, N, Hp, Wp, nH, d, shift};
    if (g == 2) return wa16w_go<2>(p, (unsigned)total, s);
    if (g == 3) return wa16w_go<3>(p, (unsigned)total, s);
    return wa16w_go<4>(p, (unsigned)total, s);
}

}  // namespace innfer
