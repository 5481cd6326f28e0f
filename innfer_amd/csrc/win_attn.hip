// Window attention of a Swin block (SwinIR: 8 x 8 windows, shift 0 or 4) over the head-padded qkv slab: ONE launch for all windows and heads of a batch.
//   qkv slab   3 nH channel groups of 32: group h = q of head h (d real channels, then zeros; the d^-0.5 already inside the weights), nH + h = k, 2 nH + h = v
//   out slab   nH groups: head h's result at the same pixels, channels d .. 31 zero -- what attn.proj reads through its permuted input columns
// A wave owns one (image, head, window): 64 tokens x 32 channels.  Token i of window (wy, wx) is pixel (8 wy + i / 8, 8 wx + i % 8) of the SHIFTED frame, which is pixel
// ((r + shift) mod Hp, (c + shift) mod Wp) of the stored one: torch.roll(u, (-shift, -shift)) is the address of the gather, the roll back the address of the store.
//   S^T = K Q^T + B^T   sixteen v_mfma_f32_16x16x32_f16: A = 16 keys x 32 channels, B = 32 channels x 16 queries -- both fragments are 16-byte loads straight from the slab
//                       (lane (li, lg): token 16 t + li, channels 8 lg .. 8 lg + 7); the C operand is the relative position bias, a dense [nH][64 query][64 key] fp32
//                       table (four consecutive keys of a query per lane: one 16-byte load).  The transposed product leaves a QUERY on a lane (li) and its 64 keys in
//                       16 registers x 4 lane groups: the row maximum and the row sum are 15 register operations and two cross-lane exchanges.
//   mask                shift only, and only in the last window row / column: tokens carry the label 3 a(r) + b(c) of their shifted-frame pixel (a = 0 below Hp - 8, 1 below
//                       Hp - 4, else 2); a score whose two labels differ gets -100 added (not -inf), as the published code does.  Computed from the coordinates.
//   P                   exp(s - max) in fp32 (v_exp_f32), the row sum in fp32 over the unrounded values; P rounded to fp16 is the B operand of the second product
//   O^T = V^T P^T       sixteen MFMAs: a lane's eight P values of a 32-key step are keys 32 ks + 16 (e / 4) + 4 lg + e % 4, so V^T is staged once per wave in LDS with
//                       its keys in that order ([32 channels][64 slots], 144-byte rows): an A fragment is one ds_read_b128.  A lane ends with four consecutive channels of
//                       its query: o / sum in fp32, one rounding, one 8-byte store; channels >= d are written as zeros.
// A window of image n reads only image n.  Bound by the gather and the exponentials, not by the 32 MFMAs: 12 KB in and 4 KB out per wave.
//
// COS (Swin2SR: the SwinV2 cosine attention) is the same kernel with another score: S = (q^ k^T^) tau_h + B_h + M, q^ = q / max(||q||_2, 1e-12), k^ likewise.  The raw
// product K Q^T runs on the fp16 operands AS STORED (C operand zero); the scaling follows in fp32, s = fma(raw (rq_i tau_h), rk_j, B_h[i][j]) -- normalising q or k into fp16
// in front of the MFMA would cost one more rounding of every operand.  r = 1 / max(sqrtf(sum of squares), 1e-12) in fp32: a lane holds eight channels of its four tokens,
// the four lane groups of a token are two exchanges apart (__shfl_xor 16, 32), so rq of query 16 tq + li is on every lane that needs it; the 64 rk go through 256 bytes of
// LDS per wave in front of the barrier V^T needs anyway (lane l writes key l, a lane reads its four consecutive keys of a 16-key tile as one 16-byte load).  An all-zero q
// or k row has raw = 0: its scores are the bias alone.  Mask, maximum, exponentials, sum, P and the second product are the code above.
#include "common.h"

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

__device__ __forceinline__ int wa_band(int r, int n) { return r < n - 8 ? 0 : (r < n - 4 ? 1 : 2); }

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
        const int slot = (tok & 32) + 8 * ((tok >> 2) & 3) + 4 * ((tok >> 4) & 1) + (tok & 3);
#pragma unroll
        for (int e = 0; e < 8; ++e) vt[(8 * oct + e) * WA_VROW + slot] = v[e];
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
        int lq[4], lk[4][4];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int tq = 16 * t + li;
            lq[t] = 3 * wa_band(wy * 8 + (tq >> 3), p.Hp) + wa_band(wx * 8 + (tq & 7), p.Wp);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int tk = 16 * t + 4 * lg + j;
                lk[t][j] = 3 * wa_band(wy * 8 + (tk >> 3), p.Hp) + wa_band(wx * 8 + (tk & 7), p.Wp);
            }
        }
#pragma unroll
        for (int tq = 0; tq < 4; ++tq)
#pragma unroll
            for (int tk = 0; tk < 4; ++tk)
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (lq[tq] != lk[tk][j]) s[tk][tq][j] += -100.0f;
    }
    float inv[4];
    f16x8 pf[4][2];                                      // pf[tq][ks]: the B fragment of key step ks
#pragma unroll
    for (int tq = 0; tq < 4; ++tq) {
        float m = s[0][tq][0];
#pragma unroll
        for (int tk = 0; tk < 4; ++tk)
#pragma unroll
            for (int j = 0; j < 4; ++j) m = fmaxf(m, s[tk][tq][j]);
        m = fmaxf(m, __shfl_xor(m, 16));
        m = fmaxf(m, __shfl_xor(m, 32));
        float sum = 0.f;
#pragma unroll
        for (int tk = 0; tk < 4; ++tk)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float e = __expf(s[tk][tq][j] - m);
                sum += e;
                pf[tq][tk >> 1][4 * (tk & 1) + j] = (f16)e;
            }
        sum += __shfl_xor(sum, 16);
        sum += __shfl_xor(sum, 32);
        inv[tq] = 1.0f / sum;
    }
    const f32x4 z4 = {0.f, 0.f, 0.f, 0.f};
    f16* ob = p.out + (long)h * p.out_gs + 4 * lg;
#pragma unroll
    for (int td = 0; td < 2; ++td) {
        const f16x8 a0 = *(const f16x8*)(vt + (16 * td + li) * WA_VROW + 8 * lg), a1 = *(const f16x8*)(vt + (16 * td + li) * WA_VROW + 32 + 8 * lg);
#pragma unroll
        for (int tq = 0; tq < 4; ++tq) {
            f32x4 o = __builtin_amdgcn_mfma_f32_16x16x32_f16(a0, pf[tq][0], z4, 0, 0, 0);
            o = __builtin_amdgcn_mfma_f32_16x16x32_f16(a1, pf[tq][1], o, 0, 0, 0);
            f16x4 r;
#pragma unroll
            for (int j = 0; j < 4; ++j) r[j] = 16 * td + 4 * lg + j < p.d ? (f16)(o[j] * inv[tq]) : (f16)0.f;
            if (live) *(f16x4*)(ob + px[tq] + 16 * td) = r;
        }
    }
}

}  // namespace

static int win_attn_any(const f16* qkv, long gs, f16* out, long out_gs, const float* relb, const float* tau, bool cos, int N, int Hp, int Wp, int nH, int d, int shift, hipStream_t s) {
    if (cos && !tau) return set_error(INNFER_ERR_INVALID, "window attention: the cosine form without its per-head scales");
    if (!qkv || !out || !relb || N <= 0 || Hp <= 0 || Wp <= 0) return set_error(INNFER_ERR_INVALID, "window attention: null argument or N=%d Hp=%d Wp=%d", N, Hp, Wp);
    if ((Hp & 7) || (Wp & 7)) return set_error(INNFER_ERR_INVALID, "window attention: %d x %d is not a whole number of 8 x 8 windows (the caller pads)", Hp, Wp);
    if (nH < 1 || nH > 8 || d < 1 || d > 32) return set_error(INNFER_ERR_UNSUPPORTED, "window attention: %d heads of %d channels (built: <= 8 heads, <= 32 channels)", nH, d);
    if (shift != 0 && shift != 4) return set_error(INNFER_ERR_UNSUPPORTED, "window attention: shift %d (built: 0, 4)", shift);
    const long G = (long)N * Hp * Wp * 32;
    if (gs < G || out_gs < G) return set_error(INNFER_ERR_INVALID, "window attention: a group stride below N * Hp * Wp * 32");
    const long total = (long)N * nH * (Hp >> 3) * (Wp >> 3);
    if (total > 0x7ffffff0L) return set_error(INNFER_ERR_UNSUPPORTED, "window attention: %ld windows x heads exceed the launch grid", total);
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
