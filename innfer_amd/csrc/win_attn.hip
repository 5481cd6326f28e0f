// Window attention of a Swin block (SwinIR: 8 x 8 windows, shift 0 or 4) over the head-padded qkv slab: ONE launch for all windows and heads of a batch.  The arithmetic is
// win_attn_core.h's; this file's own:
//   geometry   a wave owns one (image, head, window): 64 tokens, ONE key block -- row_max and exp_sum_pack directly, no running maximum and no alpha.  Token i of window
//              (wy, wx) is pixel (8 wy + i / 8, 8 wx + i % 8) of the SHIFTED frame, pixel ((r + shift) mod Hp, (c + shift) mod Wp) of the stored one: torch.roll(u, (-shift,
//              -shift)) is the address of the gather, the roll back the address of the store.  The bias is a dense [nH][64 query][64 key] fp32 table.
//   V^T        staged once per WAVE in LDS ([32 channels][64 slots], 144-byte rows).  Bound by the gather and the exponentials, not by the 32 MFMAs: 12 KB in, 4 KB out a wave.
//   COS        (Swin2SR: the SwinV2 cosine attention) another score: S = (q^ k^T^) tau_h + B_h + M, q^ = q / max(||q||_2, 1e-12), k^ likewise.  The raw product K Q^T runs on
//              the fp16 operands AS STORED (C operand zero); the scaling follows in fp32, s = fma(raw (rq_i tau_h), rk_j, B_h[i][j]) -- normalising q or k into fp16 in front
//              of the MFMA would cost one more rounding of every operand.  r = 1 / max(sqrtf(sum of squares), 1e-12) in fp32: a lane holds eight channels of its four tokens,
//              the four lane groups of a token are two exchanges apart, so rq of query 16 tq + li is on every lane that needs it; the 64 rk go through 256 bytes of LDS per
//              wave in front of the barrier V^T needs anyway (lane l writes key l, a lane reads its four consecutive keys of a 16-key tile as one 16-byte load).  An all-zero
//              q or k row has raw = 0: its scores are the bias alone.
#include "win_attn_core.h"

namespace innfer {

namespace {

constexpr int WA_VROW = 72;          // fp16 elements of a V^T row in LDS: 64 key slots + 8 (144 bytes: a multiple of 16, rows do not all start on the same bank)

struct WinAttn {
    const f16* qkv; long gs;
    f16* out; long out_gs;
    const float* relb;
    const float* tau;                // COS: exp(min(logit_scale, ln 100)) of every head
    int N, Hp, Wp, nH, d, shift, total;
};

template <bool COS>
__global__ __launch_bounds__(256) void win_attn_kernel(const WinAttn p) {
    __shared__ __attribute__((aligned(16))) f16 vts[4][32 * WA_VROW];
    __shared__ __attribute__((aligned(16))) float rks[COS ? 4 : 1][64];      // COS: 1 / max(||k||, 1e-12) of the wave's 64 keys
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, lg = lane >> 4;
    int item = blockIdx.x * 4 + wave;
    const bool live = item < p.total;
    if (!live) item = p.total - 1;                       // (the last workgroup's spare waves repeat the last item and store nothing: the barrier below is the workgroup's)
    const int nwx = p.Wp >> 3, nw = nwx * (p.Hp >> 3);
    const int w = item % nw, h = (item / nw) % p.nH, n = item / (nw * p.nH);
    const int wy = w / nwx, wx = w - wy * nwx;
    auto pix = [&](int t) -> long {                      // element offset of token t's pixel inside a slab group
        int r = wy * 8 + (t >> 3) + p.shift, c = wx * 8 + (t & 7) + p.shift;
        if (r >= p.Hp) r -= p.Hp;
        if (c >= p.Wp) c -= p.Wp;
        return (((long)n * p.Hp + r) * p.Wp + c) * 32;
    };
    const f16* qb = p.qkv + (long)h * p.gs + 8 * lg;
    const f16* kb = qb + (long)p.nH * p.gs;
    const f16* vb = p.qkv + (long)(2 * p.nH + h) * p.gs;
    f16* vt = vts[wave];
    long px[4];
    f16x8 qf[4], kf[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        px[t] = pix(16 * t + li);
        qf[t] = *(const f16x8*)(qb + px[t]);
        kf[t] = *(const f16x8*)(kb + px[t]);
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) {                        // V^T into LDS: piece (token, channel octet) -> eight rows, the token's key slot
        const int pc = lane + 64 * c, tok = pc >> 2, oct = pc & 3;
        const f16x8 v = *(const f16x8*)(vb + pix(tok) + 8 * oct);
        wa::scatter_vt<WA_VROW>(vt, tok, oct, v);
    }
    float rq[4] = {0.f, 0.f, 0.f, 0.f};                  // COS: tau_h / max(||q||, 1e-12) of query 16 tq + li
    if constexpr (COS) {
        const float tau = p.tau[h];
        float mine = 0.f;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            float sq = 0.f, sk = 0.f;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float a = (float)qf[t][e], b = (float)kf[t][e];
                sq = __builtin_fmaf(a, a, sq);
                sk = __builtin_fmaf(b, b, sk);
            }
            sq += __shfl_xor(sq, 16); sq += __shfl_xor(sq, 32);
            sk += __shfl_xor(sk, 16); sk += __shfl_xor(sk, 32);
            rq[t] = tau / fmaxf(sqrtf(sq), 1e-12f);
            const float rk = 1.0f / fmaxf(sqrtf(sk), 1e-12f);
            if (lg == t) mine = rk;                      // (all four lane groups hold token 16 t + li's value: group t keeps it, so lane l writes key l)
        }
        rks[wave][lane] = mine;
    }
    __syncthreads();

    // s[tk][tq][j]: key 16 tk + 4 lg + j, query 16 tq + li
    const float* rb = p.relb + (long)h * 4096;
    f32x4 s[4][4];
#pragma unroll
    for (int tq = 0; tq < 4; ++tq)
#pragma unroll
        for (int tk = 0; tk < 4; ++tk) {
            const f32x4 b = *(const f32x4*)(rb + (16 * tq + li) * 64 + 16 * tk + 4 * lg);
            if constexpr (COS) {
                const f32x4 z = {0.f, 0.f, 0.f, 0.f};
                const f32x4 raw = __builtin_amdgcn_mfma_f32_16x16x32_f16(kf[tk], qf[tq], z, 0, 0, 0);
                const f32x4 rk = *(const f32x4*)(&rks[wave][16 * tk + 4 * lg]);
#pragma unroll
                for (int j = 0; j < 4; ++j) s[tk][tq][j] = __builtin_fmaf(raw[j] * rq[tq], rk[j], b[j]);
            } else
                s[tk][tq] = __builtin_amdgcn_mfma_f32_16x16x32_f16(kf[tk], qf[tq], b, 0, 0, 0);
        }
    if (p.shift && (wy == (p.Hp >> 3) - 1 || wx == nwx - 1)) {       // (wave-uniform) the windows that wrap
        int lq[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) lq[t] = wa::label_sq<8>(wy, wx, 16 * t + li, p.Hp, p.Wp);
        wa::mask_block(s, lq, 4 * lg, [&](int key) { return wa::label_sq<8>(wy, wx, key, p.Hp, p.Wp); });
    }
    float l[4];
    f16x8 pf[4][2];                                      // pf[tq][ks]: the B fragment of key step ks
#pragma unroll
    for (int tq = 0; tq < 4; ++tq) l[tq] = wa::exp_sum_pack(s, tq, wa::row_max(s, tq), pf[tq]);
    const f32x4 z4 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int td = 0; td < 2; ++td) {                     // one channel tile at a time (rows 16 td .. of V^T, channels 16 td .. of the group): its 16 accumulator registers
        f32x4 o[1][4] = {{z4, z4, z4, z4}};              // are free again at its store, which keeps the COS form at four waves a SIMD
        wa::pv_block<4, 1, WA_VROW>(vt + 16 * td * WA_VROW, li, lg, pf, o);
        wa::store_out(p.out + (long)h * p.out_gs + 16 * td, p.out_gs, px, o, l, p.d - 16 * td, lg, [&](int) { return !live; });
    }
}

}  // namespace

static int win_attn_any(const f16* qkv, long gs, f16* out, long out_gs, const float* relb, const float* tau, bool cos, int N, int Hp, int Wp, int nH, int d, int shift, hipStream_t s) {
    if (cos && !tau) return set_error(INNFER_ERR_INVALID, "window attention: the cosine form without its per-head scales");
    if (int rc = wa::refuse_frame("window attention", qkv, out, relb, N, Hp, Wp, 8)) return rc;
    if (nH < 1 || nH > 8 || d < 1 || d > 32) return set_error(INNFER_ERR_UNSUPPORTED, "window attention: %d heads of %d channels (built: <= 8 heads, <= 32 channels)", nH, d);
    if (shift != 0 && shift != 4) return set_error(INNFER_ERR_UNSUPPORTED, "window attention: shift %d (built: 0, 4)", shift);
    const long total = (long)N * nH * (Hp >> 3) * (Wp >> 3);
    if (int rc = wa::refuse_strides_grid("window attention", gs, out_gs, N, Hp, Wp, total, 0x7ffffff0L)) return rc;
    GtScope gt(s, cos ? "cosine window attention (8 x 8, all heads)" : "window attention (8 x 8, all heads)", 4.0 * 64 * 64 * 32 * (double)total, (double)total * 64 * 32 * 2 * 4 + nH * 16384.0);
    const WinAttn p{qkv, gs, out, out_gs, relb, tau, N, Hp, Wp, nH, d, shift, (int)total};
    if (cos) hipLaunchKernelGGL(win_attn_kernel<true>, dim3((unsigned)((total + 3) / 4)), dim3(256), 0, s, p);
    else hipLaunchKernelGGL(win_attn_kernel<false>, dim3((unsigned)((total + 3) / 4)), dim3(256), 0, s, p);
    INNFER_HIP(hipGetLastError());
    return INNFER_OK;
}

int win_attn_launch(const f16* qkv, long gs, f16* out, long out_gs, const float* relb, int N, int Hp, int Wp, int nH, int d, int shift, hipStream_t s) {
    return win_attn_any(qkv, gs, out, out_gs, relb, nullptr, false, N, Hp, Wp, nH, d, shift, s);
}

int win_attn_cos_launch(const f16* qkv, long gs, f16* out, long out_gs, const float* relb, const float* tau, int N, int Hp, int Wp, int nH, int d, int shift, hipStream_t s) {
    return win_attn_any(qkv, gs, out, out_gs, relb, tau, true, N, Hp, Wp, nH, d, shift, s);
}

}  // namespace innfer
