// Permuted self-attention (SRFormer's PSA) over WS x WS query windows, WS = 2 PW in {16, 22, 24}: a window has WS^2 queries but only PW^2 keys.  ONE launch for all
// windows and heads of a batch.  What follows the scores is win_attn_core.h's (slot order of V^T, the P fragments, the store); this file's own:
//   keys       key token (py, px), py, px < PW, has C channels: channel f = s (C / 4) + cc is channel cc of the kv Linear's k (or v) output at pixel (2 py + s / 2,
//              2 px + s % 2) of the window, s = 0 .. 3.  Head h owns f in [h d, (h + 1) d): its channels can straddle two pixels of the 2 x 2 patch, and not at an
//              octet, so K and V^T of the window are staged ONCE per workgroup in LDS by an ELEMENT-wise gather (thread = (key, channel): at most 160 x 32 two-byte
//              loads for each of k and v); the straddling is paid there and nowhere else.  K: [keys][32 + 8], V^T: [32][keys + 8] with the keys in slot order.
//   slabs      q: the head-padded slab (head h = group h, d real channels, then zeros; d^-0.5 inside the weights); kv: k's C / 4 channels in ceil(C / 128) groups in
//              natural order (zero pads), then v's in as many; out: the head-padded slab the proj launches read, channels >= d written as zeros.
//   roll       token (r, c) of window (wy, wx) is pixel ((WS wy + r + shift) mod Hp, (WS wx + c + shift) mod Wp) of the stored frame: the roll is the address of the
//              gathers, the roll back the address of the store.
//   bias       B[h][query (r, c)][key (py, px)] = table[h][(r / 2 - py + PW - 1)(2 PW - 1) + (c / 2 - px + PW - 1)]: the head's compact table (<= 529 floats) lives in
//              LDS; a lane's index is (its query's base) - (the key's offset), the offsets (and the keys' labels) held in registers.  It enters as the MFMA's C operand.
//   mask       (shift only, last window row / column) -100 where the labels differ.  A query's label is SwinIR's on the rolled frame (bands at Hp - WS, Hp - WS / 2);
//              a key's comes from the same construction on the half-resolution grid Hp / 2 x Wp / 2 (bands at Hp / 2 - PW, Hp / 2 - PW / 2: PW 11 gives 5, so key row 5
//              of a last-row window is label 1 although it covers query rows 10 and 11).
//   geometry   a workgroup owns one (image, head, window); its four waves walk the query tiles of 16 (16 / 31 / 36 of them) round-robin, ONE tile at a time.  A wave
//              keeps the K fragments of all key tiles in registers (16 / 32 / 36 VGPRs) and reads V^T from LDS.  Keys are padded to a multiple of 32 (64 / 128 / 160):
//              a pad key's score is -3e38 (outside the maximum; exp gives 0, outside the sum), its K row and V^T column are zeros.  The queries of the last tile beyond
//              WS^2 repeat the last query and are never stored.
//   arithmetic S^T = K Q^T + B^T by v_mfma_f32_16x16x32_f16 (one K step: d <= 32), fp32; ONE pass over all keys: maximum, P = exp(s - m) (v_exp_f32), the sum over the
//              unrounded values; P rounded to fp16 is the B operand of O^T += V^T P^T (key steps of 32, fp32 accumulation); o * (1 / sum), one rounding.
#include "win_attn_core.h"
#include "test_entry.h"

namespace innfer {

namespace {

struct WinAttnPerm {
    const f16* q; long q_gs;
    const f16* kv; long kv_gs;
    f16* out; long out_gs;
    const float* table;
    int N, Hp, Wp, C, nH, d, shift;
};

template <int PW>
__global__ __launch_bounds__(256) void win_attn_perm_kernel(const WinAttnPerm p) {
    constexpr int WS = 2 * PW, NQ = WS * WS, NK = PW * PW, NKP = (NK + 31) / 32 * 32, KT = (NK + 15) / 16, KS = NKP / 32, NT = (NQ + 15) / 16;
    constexpr int KP = 40, VROW = NKP + 8, SIDE = 2 * PW - 1, NTAB = SIDE * SIDE;      // KP, VROW: multiples of 8 (16-byte fragments) whose rows start on different banks
    __shared__ __attribute__((aligned(16))) f16 kl[NKP * KP];
    __shared__ __attribute__((aligned(16))) f16 vt[32 * VROW];
    __shared__ __attribute__((aligned(16))) int kinfo[NKP];       // key -> py SIDE + px (its offset in the table) | its label << 16
    __shared__ float tab[NTAB];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, lg = lane >> 4;
    const int nwx = p.Wp / WS, nwy = p.Hp / WS, nw = nwx * nwy;
    const int item = blockIdx.x;
    const int w = item % nw, h = (item / nw) % p.nH, n = item / (nw * p.nH);
    const int wy = w / nwx, wx = w - wy * nwx;
    const long img = (long)n * p.Hp * p.Wp;
    // element offset inside a slab group of the pixel at (r, c) of the window
    auto pix = [&](int r, int c) -> long {
        int rr = wy * WS + r + p.shift, cc = wx * WS + c + p.shift;
        if (rr >= p.Hp) rr -= p.Hp;
        if (cc >= p.Wp) cc -= p.Wp;
        return (img + (long)rr * p.Wp + cc) * 32;
    };
    {   // K and V^T of the window: thread = (key, channel e of the head); channel e is channel cc of pixel `sub` of the key's 2 x 2 patch
        const int c4 = p.C >> 2, kg = (c4 + 31) >> 5, e = tid & 31;
        const bool real = e < p.d;
        const int f = real ? h * p.d + e : 0, sub = f / c4, cc = f - sub * c4;
        const f16* kb = p.kv + (long)(cc >> 5) * p.kv_gs + (cc & 31);
        const f16* vb = kb + (long)kg * p.kv_gs;
        for (int key = tid >> 5; key < NKP; key += 8) {
            f16 kv = (f16)0.f, vv = (f16)0.f;
            if (real && key < NK) {
                const int py = key / PW, px = key - py * PW;
                const long o = pix(2 * py + (sub >> 1), 2 * px + (sub & 1));
                kv = kb[o]; vv = vb[o];
            }
            kl[key * KP + e] = kv;
            vt[e * VROW + wa::slot(key)] = vv;
        }
        for (int key = tid; key < NKP; key += 256) {
            const int py = key / PW, px = key - py * PW;
            const int lab = 3 * wa::band(wy * PW + py, p.Hp >> 1, PW, PW / 2) + wa::band(wx * PW + px, p.Wp >> 1, PW, PW / 2);
            kinfo[key] = key < NK ? (py * SIDE + px) | (lab << 16) : 0;
        }
        for (int i = tid; i < NTAB; i += 256) tab[i] = p.table[(long)h * NTAB + i];
    }
    __syncthreads();

    f16x8 kf[KT];
    int4 ki[KT];
#pragma unroll
    for (int t = 0; t < KT; ++t) {
        kf[t] = *(const f16x8*)(kl + (16 * t + li) * KP + 8 * lg);
        ki[t] = *(const int4*)(kinfo + 16 * t + 4 * lg);
    }
    const bool masked = p.shift && (wy == nwy - 1 || wx == nwx - 1);      // (workgroup-uniform) the windows that wrap
    const f16* qb = p.q + (long)h * p.q_gs + 8 * lg;
    f16* ob = p.out + (long)h * p.out_gs;
    const f32x4 z4 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
    for (int t = wave; t < NT; t += 4) {
        const int qi = 16 * t + li < NQ ? 16 * t + li : NQ - 1;
        const int r = qi / WS, c = qi - r * WS;
        const long px[1] = {pix(r, c)};
        const f16x8 qf = *(const f16x8*)(qb + px[0]);
        const int qbase = ((r >> 1) + PW - 1) * SIDE + (c >> 1) + PW - 1;
        const int lq = 3 * wa::band(wy * WS + r, p.Hp, WS, PW) + wa::band(wx * WS + c, p.Wp, WS, PW);
        // s[tk][j]: key 16 tk + 4 lg + j, query 16 t + li
        f32x4 s[KT];
#pragma unroll
        for (int tk = 0; tk < KT; ++tk) {
            const int kk[4] = {ki[tk].x, ki[tk].y, ki[tk].z, ki[tk].w};
            f32x4 bias;
#pragma unroll
            for (int j = 0; j < 4; ++j) bias[j] = tab[qbase - (kk[j] & 0xffff)];
            s[tk] = __builtin_amdgcn_mfma_f32_16x16x32_f16(kf[tk], qf, bias, 0, 0, 0);
            if (masked) {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float sm = s[tk][j] + -100.0f;
                    s[tk][j] = lq != (kk[j] >> 16) ? sm : s[tk][j];
                }
            }
            if (16 * tk + 15 >= NK) {
#pragma unroll
                for (int j = 0; j < 4; ++j) s[tk][j] = 16 * tk + 4 * lg + j < NK ? s[tk][j] : -3.0e38f;
            }
        }
        float m = s[0][0];
#pragma unroll
        for (int tk = 0; tk < KT; ++tk)
#pragma unroll
            for (int j = 0; j < 4; ++j) m = fmaxf(m, s[tk][j]);
        m = fmaxf(m, __shfl_xor(m, 16));
        m = fmaxf(m, __shfl_xor(m, 32));
        f16x8 pf[KS];
        float sum = 0.f;
#pragma unroll
        for (int tk = 0; tk < 2 * KS; ++tk)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float e = 0.f;
                if (tk < KT) { e = __expf(s[tk < KT ? tk : 0][j] - m); sum += e; }
                pf[tk >> 1][4 * (tk & 1) + j] = (f16)e;
            }
        sum += __shfl_xor(sum, 16);
        const float l[1] = {sum + __shfl_xor(sum, 32)};
        f32x4 o[2][1] = {{z4}, {z4}};
#pragma unroll
        for (int ks = 0; ks < KS; ++ks)
#pragma unroll
            for (int td = 0; td < 2; ++td) {
                const f16x8 a = *(const f16x8*)(vt + (16 * td + li) * VROW + 32 * ks + 8 * lg);
                o[td][0] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, pf[ks], o[td][0], 0, 0, 0);
            }
        wa::store_out(ob, p.out_gs, px, o, l, p.d, lg, [&](int) { return 16 * t + li >= NQ; });
    }
}

// every refusal of the launch, before anything is uploaded or launched
int win_attn_perm_refuse(const void* q, long q_gs, const void* kv, long kv_gs, const void* out, long out_gs, const void* table, int N, int Hp, int Wp, int C, int nH, int ws,
                         int shift) {
    const char* what = "permuted window attention";
    if (ws != 16 && ws != 22 && ws != 24) return set_error(INNFER_ERR_UNSUPPORTED, "%s: a window of %d (built: 16, 22, 24)", what, ws);
    if (!kv) return set_error(INNFER_ERR_INVALID, "%s: null argument", what);
    if (int rc = wa::refuse_frame(what, q, out, table, N, Hp, Wp, ws)) return rc;
    if (C < 4 || C > 256 || nH < 1 || nH > 8 || C % 4 || C % nH || C / nH > 32)
        return set_error(INNFER_ERR_UNSUPPORTED, "%s: %d channels in %d heads (built: C <= 256, C %% 4 == 0, <= 8 heads of <= 32 channels, C %% heads == 0)", what, C, nH);
    if (shift != 0 && shift != ws / 2) return set_error(INNFER_ERR_UNSUPPORTED, "%s: shift %d (built: 0, %d)", what, shift, ws / 2);
    if (kv_gs < (long)N * Hp * Wp * 32) return set_error(INNFER_ERR_INVALID, "%s: a group stride below N * Hp * Wp * 32", what);
    return wa::refuse_strides_grid(what, q_gs, out_gs, N, Hp, Wp, (long)N * nH * (Hp / ws) * (Wp / ws), 0x7fffffffL);
}

}  // namespace

// q: nH groups; kv: 2 ceil(C / 128) groups (k, then v); out: nH groups; table: compact fp32 [nH][(ws - 1)^2] (device); ws 16 | 22 | 24; shift 0 | ws / 2
int win_attn_perm_launch(const f16* q, long q_gs, const f16* kv, long kv_gs, f16* out, long out_gs, const float* table, int N, int Hp, int Wp, int C, int nH, int ws, int shift,
                         hipStream_t s) {
    if (int rc = win_attn_perm_refuse(q, q_gs, kv, kv_gs, out, out_gs, table, N, Hp, Wp, C, nH, ws, shift)) return rc;
    const long total = (long)N * nH * (Hp / ws) * (Wp / ws);
    const double nq = (double)ws * ws, nk = nq / 4;
    GtScope gt(s, "permuted window attention (all heads)", 4.0 * nq * nk * 32 * (double)total, (double)total * (nq * 32 * 2 * 2 + nk * 32 * 2 * 2 + (ws - 1.0) * (ws - 1.0) * 4));
    const WinAttnPerm p{q, q_gs, kv, kv_gs, out, out_gs, table, N, Hp, Wp, C, nH, C / nH, shift};
    if (ws == 16) hipLaunchKernelGGL(win_attn_perm_kernel<8>, dim3((unsigned)total), dim3(256), 0, s, p);
    else if (ws == 22) hipLaunchKernelGGL(win_attn_perm_kernel<11>, dim3((unsigned)total), dim3(256), 0, s, p);
    else hipLaunchKernelGGL(win_attn_perm_kernel<12>, dim3((unsigned)total), dim3(256), 0, s, p);
    INNFER_HIP(hipGetLastError());
    return INNFER_OK;
}

// The launch alone, for tests: win_attn_perm_launch, the code the network runs.  Every refusal comes before the upload; uploads the table, launches, waits.
extern "C" int innfer_window_attention_perm(const void* d_q, int64_t q_gs, const void* d_kv, int64_t kv_gs, void* d_out, int64_t out_gs, const float* h_table, int N, int Hp,
                                            int Wp, int C, int num_heads, int window, int shift, void* stream) {
    if (int rc = win_attn_perm_refuse(d_q, (long)q_gs, d_kv, (long)kv_gs, d_out, (long)out_gs, h_table, N, Hp, Wp, C, num_heads, window, shift)) return rc;
    Upload b("window_attention_perm", {{h_table, (size_t)num_heads * (window - 1) * (window - 1)}}, "bias table");
    int rc = b.rc;
    if (rc == INNFER_OK)
        rc = win_attn_perm_launch((const f16*)d_q, (long)q_gs, (const f16*)d_kv, (long)kv_gs, (f16*)d_out, (long)out_gs, b.d, N, Hp, Wp, C, num_heads, window, shift, (hipStream_t)stream);
    return finish("window_attention_perm", rc, stream);
}

}  // namespace innfer
