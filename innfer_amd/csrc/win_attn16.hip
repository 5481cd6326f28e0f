// Attention of 16 x 16 query windows over the head-padded qkv slab (HAT: the window self-attention of a HAB, and the overlapping cross-attention of an OCAB), templated on
// the side KW of the KEY window: ONE launch for all windows and heads of a batch.  The arithmetic is win_attn_core.h's; this file's own:
//   KW 16      keys = the window's own 256 tokens.  Token i of window (wy, wx) is pixel (16 wy + i / 16, 16 wx + i % 16) of the SHIFTED frame, pixel ((r + shift) mod Hp,
//              (c + shift) mod Wp) of the stored one (shift 0 | 8): the roll is the address of the gather, the roll back the address of the store.  Masked with a shift.
//   KW 24      keys = the 24 x 24 pixels from (16 wy - 4, 16 wx - 4) of the stored frame (nn.Unfold(24, stride 16, padding 4) behind the Linear): a position outside the grid
//              is a key with k = v = 0 -- its score is the bias alone and it TAKES PART in the softmax.  No shift, no mask.
//   geometry   a workgroup owns one (image, head, window); wave w its queries 64 w .. 64 w + 63.  256 x KW^2 fp32 scores do not fit registers, so a wave walks the keys in
//              blocks of 64 (4 for KW 16, 9 for KW 24) with the running softmax.  The bias is a dense [nH][256 query][KW^2 key] fp32 table.
//   V^T        of the whole key window, staged ONCE per workgroup in LDS ([32 channels][KW^2 slots + 8]: 16.5 KB / 36.5 KB); the four waves share it.  K is not staged: its
//              fragments are read once per wave from the slab (L2 serves the three re-reads).
#include "win_attn_core.h"

namespace innfer {

namespace {

struct WinAttn16 {
    const f16* qkv; long gs;
    f16* out; long out_gs;
    const float* relb;
    int N, Hp, Wp, nH, d, shift;
};

template <int KW>
__global__ __launch_bounds__(256) void win_attn16_kernel(const WinAttn16 p) {
    constexpr int NK = KW * KW, NB = NK / 64, VROW = NK + 8;      // VROW: fp16 elements of a V^T row (a multiple of 8: 16-byte aligned fragments; rows start on different banks)
    __shared__ __attribute__((aligned(16))) f16 vt[32 * VROW];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, lg = lane >> 4;
    const int nwx = p.Wp >> 4, nw = nwx * (p.Hp >> 4);
    const int item = blockIdx.x;
    const int w = item % nw, h = (item / nw) % p.nH, n = item / (nw * p.nH);
    const int wy = w / nwx, wx = w - wy * nwx;
    const long img = (long)n * p.Hp * p.Wp;
    // element offset of key j's pixel inside a slab group, -1 for a key outside the grid (KW 24 only)
    auto kpix = [&](int j) -> long {
        int r, c;
        if (KW == 16) {
            r = wy * 16 + (j >> 4) + p.shift; c = wx * 16 + (j & 15) + p.shift;
            if (r >= p.Hp) r -= p.Hp;
            if (c >= p.Wp) c -= p.Wp;
        } else {
            const int jr = j / KW;
            r = wy * 16 - 4 + jr; c = wx * 16 - 4 + (j - jr * KW);
            if (r < 0 || r >= p.Hp || c < 0 || c >= p.Wp) return -1;
        }
        return (img + (long)r * p.Wp + c) * 32;
    };
    auto qpix = [&](int t) -> long {
        int r = wy * 16 + (t >> 4) + p.shift, c = wx * 16 + (t & 15) + p.shift;
        if (r >= p.Hp) r -= p.Hp;
        if (c >= p.Wp) c -= p.Wp;
        return (img + (long)r * p.Wp + c) * 32;
    };
    f16x8 zero8;
#pragma unroll
    for (int e = 0; e < 8; ++e) zero8[e] = (f16)0.f;
    const f16* qb = p.qkv + (long)h * p.gs + 8 * lg;
    const f16* kb = qb + (long)p.nH * p.gs;
    const f16* vb = p.qkv + (long)(2 * p.nH + h) * p.gs;
    for (int pc = tid; pc < NK * 4; pc += 256) {         // V^T into LDS: piece (key, channel octet) -> eight rows, the key's slot inside its 64-key block
        const int tok = pc >> 2, oct = pc & 3;
        const long o = kpix(tok);
        wa::scatter_vt<VROW>(vt, tok, oct, o >= 0 ? *(const f16x8*)(vb + o + 8 * oct) : zero8);
    }
    long px[4];
    f16x8 qf[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        px[t] = qpix(64 * wave + 16 * t + li);
        qf[t] = *(const f16x8*)(qb + px[t]);
    }
    __syncthreads();

    const bool masked = KW == 16 && p.shift && (wy == (p.Hp >> 4) - 1 || wx == nwx - 1);      // (workgroup-uniform) the windows that wrap
    int lq[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) lq[t] = wa::label_sq<16>(wy, wx, 64 * wave + 16 * t + li, p.Hp, p.Wp);
    const float* rb = p.relb + (long)h * 256 * NK + (long)(64 * wave + li) * NK + 4 * lg;
    const f32x4 z4 = {0.f, 0.f, 0.f, 0.f};
    float m[4], l[4];
    f32x4 o[2][4];
#pragma unroll
    for (int t = 0; t < 4; ++t) { m[t] = -3.0e38f; l[t] = 0.f; o[0][t] = z4; o[1][t] = z4; }
#pragma unroll 1
    for (int b = 0; b < NB; ++b) {
        f16x8 kf[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const long ko = kpix(64 * b + 16 * t + li);
            kf[t] = ko >= 0 ? *(const f16x8*)(kb + ko) : zero8;
        }
        // s[tk][tq][j]: key 64 b + 16 tk + 4 lg + j, query 64 wave + 16 tq + li
        f32x4 s[4][4];
#pragma unroll
        for (int tq = 0; tq < 4; ++tq)
#pragma unroll
            for (int tk = 0; tk < 4; ++tk) {
                const f32x4 bias = *(const f32x4*)(rb + 16 * tq * NK + 64 * b + 16 * tk);
                s[tk][tq] = __builtin_amdgcn_mfma_f32_16x16x32_f16(kf[tk], qf[tq], bias, 0, 0, 0);
            }
        if (masked) wa::mask_block(s, lq, 64 * b + 4 * lg, [&](int key) { return wa::label_sq<16>(wy, wx, key, p.Hp, p.Wp); });
        f16x8 pf[4][2];                                  // pf[tq][ks]: the B fragment of key step ks of this block
        wa::softmax_block(s, m, l, o, pf);
        wa::pv_block<4, 2, VROW>(vt + 64 * b, li, lg, pf, o);
    }
    wa::store_out(p.out + (long)h * p.out_gs, p.out_gs, px, o, l, p.d, lg, [](int) { return false; });
}

}  // namespace

// kw 16: the window self-attention (shift 0 | 8); kw 24: the overlapping cross-attention (shift 0).  relb: dense fp32 [nH][256 query][kw^2 key]
int win_attn16_launch(const f16* qkv, long gs, f16* out, long out_gs, const float* relb, int N, int Hp, int Wp, int nH, int d, int shift, int kw, hipStream_t s) {
    if (int rc = wa::refuse_frame("window attention 16", qkv, out, relb, N, Hp, Wp, 16)) return rc;
    if (kw != 16 && kw != 24) return set_error(INNFER_ERR_UNSUPPORTED, "window attention 16: a key window of %d (built: 16, the window itself; 24, the overlapping one)", kw);
    if (nH < 1 || nH > 8 || d < 1 || d > 32) return set_error(INNFER_ERR_UNSUPPORTED, "window attention 16: %d heads of %d channels (built: <= 8 heads, <= 32 channels)", nH, d);
    if (shift != 0 && (shift != 8 || kw != 16)) return set_error(INNFER_ERR_UNSUPPORTED, "window attention 16: shift %d with a key window of %d (built: 0; 8 with 16)", shift, kw);
    const long total = (long)N * nH * (Hp >> 4) * (Wp >> 4);
    if (int rc = wa::refuse_strides_grid("window attention 16", gs, out_gs, N, Hp, Wp, total, 0x7fffffffL)) return rc;
    const double nk = (double)kw * kw;
    GtScope gt(s, kw == 16 ? "window attention (16 x 16, all heads)" : "overlapping window attention (16 x 16 on 24 x 24, all heads)", 4.0 * 256 * nk * 32 * (double)total,
               (double)total * (256 * 32 * 2 * 2 + nk * 32 * 2 * 2 + 256 * nk * 4));
    const WinAttn16 p{qkv, gs, out, out_gs, relb, N, Hp, Wp, nH, d, shift};
    if (kw == 16) hipLaunchKernelGGL(win_attn16_kernel<16>, dim3((unsigned)total), dim3(256), 0, s, p);
    else hipLaunchKernelGGL(win_attn16_kernel<24>, dim3((unsigned)total), dim3(256), 0, s, p);
    INNFER_HIP(hipGetLastError());
    return INNFER_OK;
}

}  // namespace innfer
