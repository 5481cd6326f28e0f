// The device code and the host refusals the window-attention kernels share (win_attn.hip, win_attn16.hip, win_attn_rect.hip, win_attn16_wide.hip), and the ONE description
// of their arithmetic -- the "declared arithmetic" the float32 models of tests/_*_ref.py restate.  A kernel file keeps its geometry (which pixel a token is, which tokens
// are zero operands), its first product, its launch bounds and its LDS; every step behind the scores is the code below, so the four kernels round alike by construction.
//   slabs       qkv: channel groups of 32 -- q of every head, then k, then v (d real channels of a head, then zeros; the d^-0.5 already inside the weights); out: the head's
//               result at the query pixels, channels >= d written as zeros.  A window of image n reads only image n.
//   lanes       lane (li, lg) = (lane & 15, lane >> 4) of a wave.  A fragment of the first product is a 16-byte load straight from the slab: token 16 t + li, channels
//               8 lg .. 8 lg + 7.
//   S^T = K Q^T + B^T   v_mfma_f32_16x16x32_f16 with A = 16 keys x 32 channels, B = 32 channels x 16 queries, C = the relative position bias (dense fp32, query-major: four
//               consecutive keys of a query per lane are one 16-byte load).  The TRANSPOSED product leaves a QUERY on a lane (li) and the 64 keys of a block in 16 registers
//               x 4 lane groups -- s[tk][tq][j] is key 16 tk + 4 lg + j of the block, query tile tq: a row maximum or a row sum is 15 register operations and two cross-lane
//               exchanges (__shfl_xor 16, 32), and every softmax factor is a per-LANE scalar.
//   mask        with a shift, in the windows of the last window row / column only: tokens carry the label 3 a(r) + b(c) of their rolled-frame pixel, a = band(r, Hp, win, shift);
//               a score whose two labels differ gets -100 added (NOT -inf, as the published code does).  Computed from the coordinates, no table.
//   softmax     keys in blocks of 64.  m' = max(m, block maximum); P = exp(s - m') in fp32 (v_exp_f32), the row sum over the UNROUNDED values; the running sum and the
//               accumulator are multiplied by alpha = exp(m - m') (first block: exp(-3e38 - m') = 0 on a zero sum and a zero accumulator).  P rounded to fp16 is the B operand
//               of the second product.  A kernel whose window is one block (win_attn.hip) uses row_max and exp_sum_pack alone: it has no alpha.
//   O^T += V^T P^T      a lane's eight P values of a 32-key step ks are keys 32 ks + 16 (e / 4) + 4 lg + e % 4.  V^T is staged in LDS ([channels][key slots + 8] fp16) with every
//               64-key block in THAT order (slot()), so an A fragment is one ds_read_b128 of slots 32 ks + 8 lg .. + 7: two reads per channel tile, two MFMAs per query tile.
//   store       a lane ends with four consecutive channels of its query: o * (1 / sum) in fp32, one rounding, one 8-byte store; channels >= d are written as zeros.
#pragma once
#include "common.h"

namespace innfer {
namespace wa {

// ---- device ----
// key slot of token tok inside its V^T row: the 64-key block stays, the key's place inside it becomes the order in which the lanes hold P
constexpr __host__ __device__ int slot(int tok) { return (tok & ~63) + (tok & 32) + 8 * ((tok >> 2) & 3) + 4 * ((tok >> 4) & 1) + (tok & 3); }

constexpr bool slot_matches_pf() {      // lane group lg's element e of pf[tq][ks] (exp_sum_pack) is the key whose slot is 32 ks + 8 lg + e: a permutation of the block, in pf's order
    for (int blk = 0; blk < 2; ++blk)
        for (int ks = 0; ks < 2; ++ks)
            for (int lg = 0; lg < 4; ++lg)
                for (int e = 0; e < 8; ++e)
                    if (slot(64 * blk + 16 * (2 * ks + (e >> 2)) + 4 * lg + (e & 3)) != 64 * blk + 32 * ks + 8 * lg + e) return false;
    return true;
}
static_assert(slot_matches_pf(), "the V^T slot order is not the key order of the P fragments");

// V^T into LDS: piece (key tok, channel octet oct) -> eight rows, the key's slot
template <int VROW>
__device__ __forceinline__ void scatter_vt(f16* vt, int tok, int oct, const f16x8& v) {
    const int sl = slot(tok);
#pragma unroll
    for (int e = 0; e < 8; ++e) vt[(8 * oct + e) * VROW + sl] = v[e];
}

__device__ __forceinline__ int band(int r, int n, int win, int sh) { return r < n - win ? 0 : (r < n - sh ? 1 : 2); }

// label of token t (row-major) of the WIN x WIN window (wy, wx) of an Hp x Wp frame rolled by WIN / 2
template <int WIN>
__device__ __forceinline__ int label_sq(int wy, int wx, int t, int Hp, int Wp) {
    return 3 * band(wy * WIN + t / WIN, Hp, WIN, WIN / 2) + band(wx * WIN + t % WIN, Wp, WIN, WIN / 2);
}

// the mask of a 64-key block whose lane holds keys key0 + 16 tk + j (key0 = 64 b + 4 lg): lq the labels of the wave's queries, label(key) the label of a key.
// (Written as a choice between two register quads, not as a conditional +=: a branch here survives into the ISA, and the compare masks then spill out of the SGPRs.)
template <int TQ, class Label>
__device__ __forceinline__ void mask_block(f32x4 (&s)[4][TQ], const int (&lq)[TQ], int key0, Label label) {
#pragma unroll
    for (int tk = 0; tk < 4; ++tk)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int lk = label(key0 + 16 * tk + j);
#pragma unroll
            for (int tq = 0; tq < TQ; ++tq) {
                f32x4 t = s[tk][tq];
                t[j] += -100.0f;
                s[tk][tq] = lq[tq] != lk ? t : s[tk][tq];
            }
        }
}

// maximum of query tile tq's 64 scores of a block
template <int TQ>
__device__ __forceinline__ float row_max(const f32x4 (&s)[4][TQ], int tq) {
    float m = s[0][tq][0];
#pragma unroll
    for (int tk = 0; tk < 4; ++tk)
#pragma unroll
        for (int j = 0; j < 4; ++j) m = fmaxf(m, s[tk][tq][j]);
    m = fmaxf(m, __shfl_xor(m, 16));
    return fmaxf(m, __shfl_xor(m, 32));
}

// exp(s - m) of query tile tq's 64 scores: their fp32 sum is returned, their fp16 roundings become pf[ks], the B fragments of the block's two 32-key steps
template <int TQ>
__device__ __forceinline__ float exp_sum_pack(const f32x4 (&s)[4][TQ], int tq, float m, f16x8 (&pf)[2]) {
    float sum = 0.f;
#pragma unroll
    for (int tk = 0; tk < 4; ++tk)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float e = __expf(s[tk][tq][j] - m);
            sum += e;
            pf[tk >> 1][4 * (tk & 1) + j] = (f16)e;
        }
    sum += __shfl_xor(sum, 16);
    return sum + __shfl_xor(sum, 32);
}

// one 64-key block of the running softmax of TQ query tiles with TD channel tiles of accumulator
template <int TQ, int TD>
__device__ __forceinline__ void softmax_block(const f32x4 (&s)[4][TQ], float (&m)[TQ], float (&l)[TQ], f32x4 (&o)[TD][TQ], f16x8 (&pf)[TQ][2]) {
#pragma unroll
    for (int tq = 0; tq < TQ; ++tq) {
        const float mn = fmaxf(m[tq], row_max(s, tq));
        const float alpha = __expf(m[tq] - mn);
        const float sum = exp_sum_pack(s, tq, mn, pf[tq]);
        l[tq] = l[tq] * alpha + sum;
        m[tq] = mn;
#pragma unroll
        for (int td = 0; td < TD; ++td)
#pragma unroll
            for (int j = 0; j < 4; ++j) o[td][tq][j] *= alpha;
    }
}

// O^T += V^T P^T of one block; vtb: the block's first slot in V^T row 0
template <int TQ, int TD, int VROW>
__device__ __forceinline__ void pv_block(const f16* vtb, int li, int lg, const f16x8 (&pf)[TQ][2], f32x4 (&o)[TD][TQ]) {
#pragma unroll
    for (int td = 0; td < TD; ++td) {
        const f16* vr = vtb + (16 * td + li) * VROW + 8 * lg;
        const f16x8 a0 = *(const f16x8*)vr, a1 = *(const f16x8*)(vr + 32);
#pragma unroll
        for (int tq = 0; tq < TQ; ++tq) {
            o[td][tq] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a0, pf[tq][0], o[td][tq], 0, 0, 0);
            o[td][tq] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a1, pf[tq][1], o[td][tq], 0, 0, 0);
        }
    }
}

// o / l of every query the lane holds (px: its pixel's offset in a group), unless skip(tq); ob: the head's first output group; channel tiles 2 g, 2 g + 1 are group g
template <int TQ, int TD, class Skip>
__device__ __forceinline__ void store_out(f16* ob, long out_gs, const long (&px)[TQ], const f32x4 (&o)[TD][TQ], const float (&l)[TQ], int d, int lg, Skip skip) {
#pragma unroll
    for (int tq = 0; tq < TQ; ++tq) {
        if (skip(tq)) continue;
        const float inv = 1.0f / l[tq];
#pragma unroll
        for (int td = 0; td < TD; ++td) {
            f16x4 r;
#pragma unroll
            for (int j = 0; j < 4; ++j) r[j] = 16 * td + 4 * lg + j < d ? (f16)(o[td][tq][j] * inv) : (f16)0.f;
            *(f16x4*)(ob + (long)(td >> 1) * out_gs + px[tq] + 16 * (td & 1) + 4 * lg) = r;
        }
    }
}

// ---- host: the refusals of a launch over a padded frame of win x win windows, under the launch's own message prefix.  They come in two halves because each file's own
// refusals (key window, heads and channels, shift) stand between them, and a call with two faults keeps reporting the one it always reported. ----
inline int refuse_frame(const char* what, const void* qkv, const void* out, const void* relb, int N, int Hp, int Wp, int win) {
    if (!qkv || !out || !relb || N <= 0 || Hp <= 0 || Wp <= 0) return set_error(INNFER_ERR_INVALID, "%s: null argument or N=%d Hp=%d Wp=%d", what, N, Hp, Wp);
    if (Hp % win || Wp % win) return set_error(INNFER_ERR_INVALID, "%s: %d x %d is not a whole number of %d x %d windows (the caller pads)", what, Hp, Wp, win, win);
    return INNFER_OK;
}
// total: windows x heads; limit: what the launch's grid takes
inline int refuse_strides_grid(const char* what, long gs, long out_gs, int N, int Hp, int Wp, long total, long limit) {
    const long G = (long)N * Hp * Wp * 32;
    if (gs < G || out_gs < G) return set_error(INNFER_ERR_INVALID, "%s: a group stride below N * Hp * Wp * 32", what);
    if (total > limit) return set_error(INNFER_ERR_UNSUPPORTED, "%s: %ld windows x heads exceed the launch grid", what, total);
    return INNFER_OK;
}

}  // namespace wa
}  // namespace innfer
