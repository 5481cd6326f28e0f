// Attention over RECTANGULAR windows in two head branches of transposed shape (DAT's adaptive spatial attention), over the head-padded qkv slab on the UNPADDED H x W grid:
// ONE launch for all windows, both branches and all heads of a batch.  The arithmetic is win_attn_core.h's (the running softmax over blocks of 64 keys); this file's own is
// the geometry.  split = [s0, s1] ([8, 32] | [8, 16]), T = s0 s1 tokens per window (256 | 128):
//   branch 0   heads 0 .. nH / 2 - 1: windows of s0 rows x s1 columns, shift (s0 / 2, s1 / 2)
//   branch 1   heads nH / 2 .. nH - 1: windows of s1 rows x s0 columns, shift (s1 / 2, s0 / 2)
// The frame the windows tile is Hp x Wp, H and W rounded up to multiples of s1 = max(s0, s1); it exists only as coordinates.  Token i of window (wy, wx) of a head whose
// windows are wh x ww is pixel (wh wy + i / ww, ww wx + i % ww) of the ROLLED frame, pixel ((r + shy) mod Hp, (c + shx) mod Wp) of the stored one (shy = shx = 0 when the
// block is not shifted).  A token whose stored pixel lies outside H x W is a ZERO operand (the published code pads qkv behind the Linear: q = k = v = 0): it is never read
// and never stored; as a key its score is bias + mask and it TAKES PART in the softmax, exactly as win_attn16.hip's KW-24 form treats keys outside the grid.
// Shifted: -100 (not -inf) between tokens whose labels 3 a(r) + b(c) differ, a = 0 below Hp - wh, 1 below Hp - shy, else 2 on the rolled-frame row, b likewise with Wp, ww,
// shx: anisotropic per branch, computed from the coordinates, only in the last window row / column (elsewhere every label is 0).
// The bias is a dense [nH][T][T] fp32 table (query-major), tokens row-major inside the head's OWN window shape.
// A workgroup of T threads owns one (image, head, window); wave w its queries 64 w .. 64 w + 63; V^T of the window is staged once per workgroup in LDS ([32][T + 8] fp16).
#include "win_attn_core.h"

namespace innfer {

namespace {

struct WinAttnRect {
    const f16* qkv; long gs;
    f16* out; long out_gs;
    const float* relb;
    int N, H, W, Hp, Wp, nH, d, s0, s1, shifted;
};

template <int T>
__global__ __launch_bounds__(T) void win_attn_rect_kernel(const WinAttnRect p) {
    constexpr int NB = T / 64, VROW = T + 8;
    __shared__ __attribute__((aligned(16))) f16 vt[32 * VROW];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, lg = lane >> 4;
    const int nw = (p.Hp * p.Wp) / T;                          // windows of a frame: the same for both branches
    const int item = blockIdx.x;
    const int w = item % nw, h = (item / nw) % p.nH, n = item / (nw * p.nH);
    const bool br1 = h >= (p.nH >> 1);
    const int wh = br1 ? p.s1 : p.s0, ww = br1 ? p.s0 : p.s1;
    const int shy = p.shifted ? wh >> 1 : 0, shx = p.shifted ? ww >> 1 : 0;
    const int nwx = p.Wp / ww, nwy = p.Hp / wh;
    const int wy = w / nwx, wx = w - wy * nwx;
    const long img = (long)n * p.H * p.W;
    // element offset of token j's pixel inside a slab group, -1 for a token of the pad
    auto tpix = [&](int j) -> long {
        const int jr = j / ww;
        int r = wy * wh + jr + shy, c = wx * ww + (j - jr * ww) + shx;
        if (r >= p.Hp) r -= p.Hp;
        if (c >= p.Wp) c -= p.Wp;
        if (r >= p.H || c >= p.W) return -1;
        return (img + (long)r * p.W + c) * 32;
    };
    f16x8 zero8;
#pragma unroll
    for (int e = 0; e < 8; ++e) zero8[e] = (f16)0.f;
    const f16* qb = p.qkv + (long)h * p.gs + 8 * lg;
    const f16* kb = qb + (long)p.nH * p.gs;
    const f16* vb = p.qkv + (long)(2 * p.nH + h) * p.gs;
    for (int pc = tid; pc < T * 4; pc += T) {                  // V^T into LDS: piece (key, channel octet) -> eight rows, the key's slot inside its 64-key block
        const int tok = pc >> 2, oct = pc & 3;
        const long o = tpix(tok);
        wa::scatter_vt<VROW>(vt, tok, oct, o >= 0 ? *(const f16x8*)(vb + o + 8 * oct) : zero8);
    }
    long px[4];
    f16x8 qf[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        px[t] = tpix(64 * wave + 16 * t + li);
        qf[t] = px[t] >= 0 ? *(const f16x8*)(qb + px[t]) : zero8;
    }
    __syncthreads();

    const bool masked = p.shifted && (wy == nwy - 1 || wx == nwx - 1);      // (workgroup-uniform) the windows that wrap
    auto label = [&](int j) -> int {
        const int jr = j / ww;
        return 3 * wa::band(wy * wh + jr, p.Hp, wh, shy) + wa::band(wx * ww + (j - jr * ww), p.Wp, ww, shx);
    };
    int lq[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) lq[t] = label(64 * wave + 16 * t + li);
    const float* rb = p.relb + (long)h * T * T + (long)(64 * wave + li) * T + 4 * lg;
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
            const long ko = tpix(64 * b + 16 * t + li);
            kf[t] = ko >= 0 ? *(const f16x8*)(kb + ko) : zero8;
        }
        // s[tk][tq][j]: key 64 b + 16 tk + 4 lg + j, query 64 wave + 16 tq + li
        f32x4 s[4][4];
#pragma unroll
        for (int tq = 0; tq < 4; ++tq)
#pragma unroll
            for (int tk = 0; tk < 4; ++tk) {
                const f32x4 bias = *(const f32x4*)(rb + 16 * tq * T + 64 * b + 16 * tk);
                s[tk][tq] = __builtin_amdgcn_mfma_f32_16x16x32_f16(kf[tk], qf[tq], bias, 0, 0, 0);
            }
        if (masked) wa::mask_block(s, lq, 64 * b + 4 * lg, label);
        f16x8 pf[4][2];                                  // pf[tq][ks]: the B fragment of key step ks of this block
        wa::softmax_block(s, m, l, o, pf);
        wa::pv_block<4, 2, VROW>(vt + 64 * b, li, lg, pf, o);
    }
    wa::store_out(p.out + (long)h * p.out_gs, p.out_gs, px, o, l, p.d, lg, [&](int tq) { return px[tq] < 0; });      // a pad token as a query: its result is dropped
}

}  // namespace

// relb: dense fp32 [nH][T][T], T = s0 s1.  Slabs of N x H x W pixels (no pad): every pixel of every head's group is written exactly once.
int win_attn_rect_launch(const f16* qkv, long gs, f16* out, long out_gs, const float* relb, int N, int H, int W, int nH, int d, int s0, int s1, int shifted, hipStream_t s) {
    if (!qkv || !out || !relb || N <= 0 || H <= 0 || W <= 0) return set_error(INNFER_ERR_INVALID, "rectangular window attention: null argument or N=%d H=%d W=%d", N, H, W);
    if (s0 != 8 || (s1 != 32 && s1 != 16)) return set_error(INNFER_ERR_UNSUPPORTED, "rectangular window attention: split [%d, %d] (built: [8, 32] and [8, 16])", s0, s1);
    if (nH < 2 || nH > 8 || (nH & 1) || d < 1 || d > 32)
        return set_error(INNFER_ERR_UNSUPPORTED, "rectangular window attention: %d heads of %d channels (built: 2, 4, 6 or 8 heads -- half per branch -- of <= 32 channels)", nH, d);
    if (shifted != 0 && shifted != 1) return set_error(INNFER_ERR_INVALID, "rectangular window attention: shifted is 0 or 1, not %d", shifted);
    if (H > 0x3fffffff || W > 0x3fffffff) return set_error(INNFER_ERR_UNSUPPORTED, "rectangular window attention: %d x %d pixels", H, W);
    const long G = (long)N * H * W * 32;
    if (gs < G || out_gs < G) return set_error(INNFER_ERR_INVALID, "rectangular window attention: a group stride below N * H * W * 32");
    const int Hp = (H + s1 - 1) / s1 * s1, Wp = (W + s1 - 1) / s1 * s1, T = s0 * s1;
    const long total = (long)N * nH * ((long)Hp * Wp / T);
    if ((long)Hp * Wp > 0x7fffffffL || total > 0x7fffffffL) return set_error(INNFER_ERR_UNSUPPORTED, "rectangular window attention: %ld windows x heads exceed the launch grid", total);
    GtScope gt(s, s1 == 32 ? "rectangular window attention (8 x 32 | 32 x 8, all heads)" : "rectangular window attention (8 x 16 | 16 x 8, all heads)",
               4.0 * T * T * 32 * (double)total, (double)total * (T * 32 * 2 * 4 + (double)T * T * 4));
    const WinAttnRect p{qkv, gs, out, out_gs, relb, N, H, W, Hp, Wp, nH, d, s0, s1, shifted};
    if (T == 256) hipLaunchKernelGGL(win_attn_rect_kernel<256>, dim3((unsigned)total), dim3(256), 0, s, p);
    else hipLaunchKernelGGL(win_attn_rect_kernel<128>, dim3((unsigned)total), dim3(128), 0, s, p);
    INNFER_HIP(hipGetLastError());
    return INNFER_OK;
}

}  // namespace innfer
