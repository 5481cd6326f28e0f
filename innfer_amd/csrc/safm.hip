// SAFMN's spatially-adaptive feature modulation (Sun et al. 2023) as ONE launch over channel-padded fp16 slabs of N x H x W pixels:
//   out = fp16(t + GELU(aggr(cat(s_0 .. s_3)) + b) * u),   s_i = nearest(dw3x3_i(adaptive_max_pool(u_i, (H >> i, W >> i))), (H, W)),   u_i = channels [i chunk, (i + 1) chunk)
// with chunk = dim / 4, torch's index rules (pool window of cell o: [floor(o h / ph), ceil((o + 1) h / ph)); nearest source of y: min(floorf(y * ((float)ph / (float)h)),
// ph - 1), ONE fp32 multiply; level 0 is the same rule with ph = h: the identity), zero padding of the depthwise conv ON THE POOLED GRID.  Reads u and t, writes out;
// no intermediate touches memory.  Channels >= dim are written as zeros whatever u and t hold there (selected, never multiplied).  out may be t, never u.
//   tile       a workgroup of four waves owns 16 x 16 pixels of one image.  Per level it needs the pooled cells its pixels map to -- at most 16, 9, 5, 3 a side -- and one
//              cell of halo for the depthwise conv.
//   phase 1    per level: (a) the haloed pooled grid into LDS, a thread per (cell, 16-byte channel octet), octets fastest, then cells along the row; the window comes from
//              the formula in image coordinates, a cell outside the pooled grid is zeros.  A level's channels need not start at an octet (dim 36: chunk 9): the octets
//              that overlap the level are read whole and the level's channels selected.  (b) the depthwise 3 x 3 from that grid, a thread per (cell, channel), taps and
//              bias in LDS, fp32 from the bias on with the taps row-major; s is written at POOLED resolution into the level's LDS grid as fp16 -- the one declared rounding
//              in front of the matrix product.  The up-sampled tensor never exists.
//   phase 2    out^T = Wq S^T on v_mfma_f32_16x16x32_f16: A = 16 output channels x 32 input channels of aggr's weight (from LDS while the panel fits, dim_pad <= 128: it
//              takes the place of the pooled grid; from L2 above), B = 16 pixels of a tile row x 32 channels gathered from the four LDS grids through each pixel's source
//              cell (16-byte reads where chunk % 8 == 0, element reads otherwise), K steps of 32 in natural channel order, input channels >= dim zeros.  All of s is
//              resident, so a wave finishes PT rows of the tile at a time over all K steps: PT x dim_pad / 16 accumulators, 64 .. 128 VGPRs, nothing carried between passes.
//   epilogue   a lane holds four consecutive output channels of a pixel: + bias, common.h fast_gelu, * u, + t in fp32, ONE rounding, 8-byte stores.
#include "common.h"
#include "test_entry.h"

#include <vector>

namespace innfer {

namespace {

constexpr int SAFM_T = 16, SAFM_CELLS = 256 + 81 + 25 + 9, SAFM_HALO_CELLS = 18 * 18;
__host__ __device__ constexpr int safm_mc(int i) { return i == 0 ? 16 : i == 1 ? 9 : i == 2 ? 5 : 3; }            // cells a side a tile can map to at level i
__host__ __device__ constexpr int safm_off(int i) { return i == 0 ? 0 : i == 1 ? 256 : i == 2 ? 337 : 362; }      // first cell of level i's grid of s

struct SafmArgs {
    const f16* u; long u_gs;
    const f16* t; long t_gs;
    f16* out; long out_gs;
    const f16* wq;              // aggr's weight [KP][KP] fp16, row = output channel, zeros behind dim
    const float* ab;            // aggr's bias [KP], zeros behind dim
    const float* mfr;           // taps [dim][9], then bias [dim]
    int N, H, W, dim, chunk, ng, tx, ty;
    float sy[4], sx[4];         // (float)(H >> i) / (float)H and the same for W: the scale of the nearest rule
};

__device__ __forceinline__ int safm_src(int y, float scale, int ph) {
    const int v = (int)floorf((float)y * scale);
    return v < ph - 1 ? v : ph - 1;
}
__device__ __forceinline__ int safm_clamp(int v, int hi) { return v < 0 ? 0 : v > hi ? hi : v; }
struct SafmL4 { int v0, v1, v2, v3; };
// the cell of coordinate y inside the grid of a tile that spans [y0, yl]: its source cell minus the tile's first, held inside the at most mc cells the grid has
__device__ __forceinline__ int safm_cell(int y, int y0, int yl, float scale, int ph, int mc) {
    const int first = safm_src(y0, scale, ph), n = safm_src(yl, scale, ph) - first + 1;
    return safm_clamp(safm_src(y, scale, ph) - first, (n < mc ? n : mc) - 1);
}

// halfs of the channel stride of the LDS grids: the chunk rounded up to an octet, plus one octet so that neighbouring cells start on different banks
__host__ __device__ inline int safm_cs(int chunk) { return ((chunk + 7) & ~7) + 8; }
template <int DG>
__host__ __device__ inline size_t safm_lds_bytes(int dim) {
    constexpr int KP = 32 * DG;
    const size_t cs = (size_t)safm_cs(dim / 4), halo = SAFM_HALO_CELLS * cs, panel = DG <= 4 ? (size_t)KP * (KP + 8) : 0;
    return (size_t)(10 * dim + KP) * 4 + (SAFM_CELLS * cs + (halo > panel ? halo : panel)) * 2;
}

template <int DG>
__global__ __launch_bounds__(256) void safm_kernel(const SafmArgs p) {
    constexpr int KP = 32 * DG, OT = 2 * DG, PT = DG == 8 ? 2 : 4, WP = KP + 8;
    constexpr bool WLDS = DG <= 4;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int dim = p.dim, chunk = p.chunk, CS = safm_cs(chunk), H = p.H, W = p.W;
    float* tw = (float*)smem;                    // taps [9][dim], bias [dim]
    float* abl = tw + 10 * dim;                  // aggr's bias [KP]
    f16* S = (f16*)(abl + KP);                   // s of the four levels: [SAFM_CELLS][CS]
    f16* R = S + SAFM_CELLS * CS;                // phase 1: the haloed pooled grid [(mc + 2)^2][CS]; phase 2: aggr's panel [KP][WP]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, lg = lane >> 4;
    const int blk = blockIdx.x, bx = blk % p.tx, by = (blk / p.tx) % p.ty, n = blk / (p.tx * p.ty);
    const int r0 = by * SAFM_T, c0 = bx * SAFM_T;
    const int rl = r0 + SAFM_T - 1 < H ? r0 + SAFM_T - 1 : H - 1, cl = c0 + SAFM_T - 1 < W ? c0 + SAFM_T - 1 : W - 1;
    const long img = (long)n * H * W * 32;
    for (int j = tid; j < 10 * dim; j += 256) {
        const int k = j / dim, c = j - k * dim;
        tw[j] = k < 9 ? p.mfr[c * 9 + k] : p.mfr[9 * dim + c];
    }
    for (int j = tid; j < KP; j += 256) abl[j] = p.ab[j];

    // ---- phase 1: per level the pooled grid with its halo, then the depthwise conv at pooled resolution
#pragma unroll 1
    for (int i = 0; i < 4; ++i) {
        const int ph = H >> i, pw = W >> i, mc = safm_mc(i), pitch = mc + 2;
        const float sy = i == 0 ? p.sy[0] : i == 1 ? p.sy[1] : i == 2 ? p.sy[2] : p.sy[3], sx = i == 0 ? p.sx[0] : i == 1 ? p.sx[1] : i == 2 ? p.sx[2] : p.sx[3];
        const int cy0 = safm_src(r0, sy, ph), cx0 = safm_src(c0, sx, pw);
        int ncy = safm_src(rl, sy, ph) - cy0 + 1, ncx = safm_src(cl, sx, pw) - cx0 + 1;
        ncy = ncy < mc ? ncy : mc; ncx = ncx < mc ? ncx : mc;
        const int gx = ncx + 2, clo = i * chunk, chi = clo + chunk, o0 = clo >> 3, no = ((chi - 1) >> 3) - o0 + 1;
        __syncthreads();                         // (the last level's conv has read R; i == 0: the taps are in place)
        for (int j = tid; j < (ncy + 2) * gx * no; j += 256) {
            const int oi = j % no, cell = j / no, a = cell / gx, b = cell - a * gx;
            const int cy = cy0 - 1 + a, cx = cx0 - 1 + b, ch0 = (o0 + oi) * 8;
            float m[8];
            if (cy >= 0 && cy < ph && cx >= 0 && cx < pw) {
                const int ys = (int)((long)cy * H / ph), ye = (int)(((long)(cy + 1) * H + ph - 1) / ph);
                const int xs = (int)((long)cx * W / pw), xe = (int)(((long)(cx + 1) * W + pw - 1) / pw);
#pragma unroll
                for (int e = 0; e < 8; ++e) m[e] = -INFINITY;
                const f16* ub = p.u + (long)(ch0 >> 5) * p.u_gs + img + (ch0 & 31);
                for (int y = ys; y < ye; ++y)
                    for (int x = xs; x < xe; ++x) {
                        const f16x8 v = *(const f16x8*)(ub + ((long)y * W + x) * 32);
#pragma unroll
                        for (int e = 0; e < 8; ++e) m[e] = fmaxf(m[e], (float)v[e]);
                    }
            } else {
#pragma unroll
                for (int e = 0; e < 8; ++e) m[e] = 0.f;
            }
            f16* dst = R + (a * pitch + b) * CS - clo;
#pragma unroll
            for (int e = 0; e < 8; ++e)
                if (ch0 + e >= clo && ch0 + e < chi) dst[ch0 + e] = (f16)m[e];
        }
        __syncthreads();
        for (int j = tid; j < ncy * ncx * chunk; j += 256) {
            const int k = j % chunk, cell = j / chunk, a = cell / ncx, b = cell - a * ncx, c = clo + k;
            float f = tw[9 * dim + c];
#pragma unroll
            for (int ky = 0; ky < 3; ++ky)
#pragma unroll
                for (int kx = 0; kx < 3; ++kx) f = __builtin_fmaf(tw[(ky * 3 + kx) * dim + c], (float)R[((a + ky) * pitch + b + kx) * CS + k], f);
            S[(safm_off(i) + a * mc + b) * CS + k] = (f16)f;
        }
    }
    __syncthreads();
    if (WLDS) {
        for (int j = tid; j < KP * (KP / 8); j += 256) {
            const int row = j / (KP / 8), q = j - row * (KP / 8);
            *(f16x8*)(R + row * WP + q * 8) = *(const f16x8*)(p.wq + row * KP + q * 8);
        }
        __syncthreads();
    }

    // ---- phase 2: the aggregation and the gate
    // a pixel coordinate's cell inside the tile's grid of level I (named scalars, no arrays: every index below is static)
    const int col = c0 + li < W ? c0 + li : W - 1;
#define SAFM_CELL(I, y, y0, yl, scale, h) safm_cell(y, y0, yl, scale, (h) >> I, safm_mc(I))
    const SafmL4 scx = {SAFM_CELL(0, col, c0, cl, p.sx[0], W), SAFM_CELL(1, col, c0, cl, p.sx[1], W), SAFM_CELL(2, col, c0, cl, p.sx[2], W), SAFM_CELL(3, col, c0, cl, p.sx[3], W)};
    const bool oct = (chunk & 7) == 0;
    const int kg = (dim + 31) >> 5;
    f16x8 zero8;
#pragma unroll
    for (int e = 0; e < 8; ++e) zero8[e] = (f16)0.f;
    const f32x4 z4 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
    for (int pass = 0; pass < 4 / PT; ++pass) {
        const int row0 = r0 + wave * 4 + pass * PT;
        SafmL4 cb[PT];
#pragma unroll
        for (int j = 0; j < PT; ++j) {
            const int r = row0 + j < H ? row0 + j : H - 1;
            // channel c of level l lies at S[v0 + c + (l >= 1 ? v1 : 0) + (l >= 2 ? v2 : 0) + (l >= 3 ? v3 : 0)]: differences, so that a level is three selects against
            // zero and never an index into this array
            const int b0 = (safm_off(0) + SAFM_CELL(0, r, r0, rl, p.sy[0], H) * safm_mc(0) + scx.v0) * CS;
            const int b1 = (safm_off(1) + SAFM_CELL(1, r, r0, rl, p.sy[1], H) * safm_mc(1) + scx.v1) * CS;
            const int b2 = (safm_off(2) + SAFM_CELL(2, r, r0, rl, p.sy[2], H) * safm_mc(2) + scx.v2) * CS;
            const int b3 = (safm_off(3) + SAFM_CELL(3, r, r0, rl, p.sy[3], H) * safm_mc(3) + scx.v3) * CS;
            cb[j].v0 = b0; cb[j].v1 = b1 - b0 - chunk; cb[j].v2 = b2 - b1 - chunk; cb[j].v3 = b3 - b2 - chunk;
        }
#undef SAFM_CELL
        f32x4 acc[PT][OT];
#pragma unroll
        for (int j = 0; j < PT; ++j)
#pragma unroll
            for (int ot = 0; ot < OT; ++ot) acc[j][ot] = z4;
#pragma unroll 1
        for (int ks = 0; ks < kg; ++ks) {
            const int cbase = ks * 32 + lg * 8;
            f16x8 bf[PT];
#pragma unroll
            for (int j = 0; j < PT; ++j) {
                f16x8 v = zero8;
                if (oct) {
                    if (cbase < dim) v = *(const f16x8*)(S + cb[j].v0 + cbase + (cbase >= chunk ? cb[j].v1 : 0) + (cbase >= 2 * chunk ? cb[j].v2 : 0) + (cbase >= 3 * chunk ? cb[j].v3 : 0));
                } else {
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        const int c = cbase + e;
                        const f16 x = S[c < dim ? cb[j].v0 + c + (c >= chunk ? cb[j].v1 : 0) + (c >= 2 * chunk ? cb[j].v2 : 0) + (c >= 3 * chunk ? cb[j].v3 : 0) : 0];
                        v[e] = c < dim ? x : (f16)0.f;
                    }
                }
                bf[j] = v;
            }
#pragma unroll
            for (int ot = 0; ot < OT; ++ot) {
                if (ot * 16 >= dim) continue;
                const f16x8 af = WLDS ? *(const f16x8*)(R + (ot * 16 + li) * WP + cbase) : *(const f16x8*)(p.wq + (ot * 16 + li) * KP + cbase);
#pragma unroll
                for (int j = 0; j < PT; ++j) acc[j][ot] = __builtin_amdgcn_mfma_f32_16x16x32_f16(af, bf[j], acc[j][ot], 0, 0, 0);
            }
        }
        // acc[j][ot][e]: output channel 16 ot + 4 lg + e of pixel (row0 + j, c0 + li)
        if (c0 + li >= W) continue;
#pragma unroll
        for (int j = 0; j < PT; ++j) {
            if (row0 + j >= H) continue;
            const long pix = img + ((long)(row0 + j) * W + c0 + li) * 32;
#pragma unroll
            for (int ot = 0; ot < OT; ++ot) {
                if ((ot >> 1) >= p.ng) continue;
                const long o = pix + (ot & 1) * 16 + 4 * lg;
                const int oc0 = ot * 16 + 4 * lg;
                const f16x4 uv = *(const f16x4*)(p.u + (long)(ot >> 1) * p.u_gs + o), tv = *(const f16x4*)(p.t + (long)(ot >> 1) * p.t_gs + o);
                f16x4 res;
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    res[e] = oc0 + e < dim ? (f16)((float)tv[e] + fast_gelu(acc[j][ot][e] + abl[oc0 + e]) * (float)uv[e]) : (f16)0.f;
                *(f16x4*)(p.out + (long)(ot >> 1) * p.out_gs + o) = res;
            }
        }
    }
}

template <int DG>
int safm_go(const SafmArgs& p, unsigned total, hipStream_t s) {
    static std::atomic<unsigned long long> done{0};
    INNFER_HIP(ensure_lds_attr(safm_kernel<DG>, (int)safm_lds_bytes<DG>(32 * DG), done));
    hipLaunchKernelGGL(safm_kernel<DG>, dim3(total), dim3(256), safm_lds_bytes<DG>(p.dim), s, p);
    INNFER_HIP(hipGetLastError());
    return INNFER_OK;
}

// every refusal of the launch, before anything is uploaded or launched
int safm_refuse(const void* u, long u_gs, const void* t, long t_gs, const void* out, long out_gs, int N, int H, int W, int dim, int c_pad, const void* a, const void* b,
                const void* c) {
    if (!u || !t || !out || !a || !b || !c || N <= 0 || H <= 0 || W <= 0) return set_error(INNFER_ERR_INVALID, "safm: null argument or N=%d H=%d W=%d", N, H, W);
    if (dim < 8 || dim > 256 || dim % 4 || c_pad < dim || c_pad > 256 || c_pad % 32)
        return set_error(INNFER_ERR_UNSUPPORTED, "safm: dim=%d in a slab of %d channels (built: dim a multiple of 4 in 8 .. 256, whole groups of 32)", dim, c_pad);
    if (H < 8 || W < 8) return set_error(INNFER_ERR_UNSUPPORTED, "safm: %d x %d pixels (four levels: both sides at least 8, so that the last pooled grid has a cell)", H, W);
    const long NHW = (long)N * H * W;
    if ((long)N * ((H + SAFM_T - 1) / SAFM_T) * ((W + SAFM_T - 1) / SAFM_T) > 0x7fffffffL) return set_error(INNFER_ERR_UNSUPPORTED, "safm: %ld pixels exceed the launch grid", NHW);
    if (u_gs < NHW * 32 || t_gs < NHW * 32 || out_gs < NHW * 32) return set_error(INNFER_ERR_INVALID, "safm: a group stride below N * H * W * 32");
    const int ng = c_pad / 32;
    const f16 *u0 = (const f16*)u, *u1 = u0 + (ng - 1) * u_gs + NHW * 32, *o0 = (const f16*)out, *o1 = o0 + (ng - 1) * out_gs + NHW * 32;
    if (u0 < o1 && o0 < u1) return set_error(INNFER_ERR_INVALID, "safm: out overlaps u (a pixel's pooled cells read its neighbours)");
    return INNFER_OK;
}

__global__ void slab_add_kernel(const f16* a, const f16* b, f16* out, long n8) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n8) return;
    const f16x8 x = ((const f16x8*)a)[i], y = ((const f16x8*)b)[i];
    f16x8 r;
#pragma unroll
    for (int e = 0; e < 8; ++e) r[e] = (f16)((float)x[e] + (float)y[e]);
    ((f16x8*)out)[i] = r;
}

}  // namespace

int safm_kp(int c_pad) { return c_pad <= 64 ? 64 : c_pad <= 128 ? 128 : 256; }

// aggr's weight [dim][dim] and bias [dim] as the kernel reads them: fp16 [KP][KP] (one rounding) and fp32 [KP], zeros behind dim
void safm_pack(const float* w, const float* b, int dim, int kp, f16* wq, float* ab) {
    for (int o = 0; o < kp; ++o) {
        ab[o] = o < dim && b ? b[o] : 0.f;
        for (int c = 0; c < kp; ++c) wq[(size_t)o * kp + c] = o < dim && c < dim ? (f16)w[(size_t)o * dim + c] : (f16)0.f;
    }
}

// c_pad: channels of the three slabs (a multiple of 32, dim <= c_pad <= 256); wq, ab: safm_pack's for safm_kp(c_pad), mfr: taps [dim][9] then bias [dim], all on the device
int safm_launch(const f16* u, long u_gs, const f16* t, long t_gs, f16* out, long out_gs, int N, int H, int W, int dim, int c_pad, const f16* wq, const float* ab,
                const float* mfr, hipStream_t s) {
    if (int rc = safm_refuse(u, u_gs, t, t_gs, out, out_gs, N, H, W, dim, c_pad, wq, ab, mfr)) return rc;
    SafmArgs p{u, u_gs, t, t_gs, out, out_gs, wq, ab, mfr, N, H, W, dim, dim / 4, c_pad / 32, (W + SAFM_T - 1) / SAFM_T, (H + SAFM_T - 1) / SAFM_T, {}, {}};
    for (int i = 0; i < 4; ++i) { p.sy[i] = (float)(H >> i) / (float)H; p.sx[i] = (float)(W >> i) / (float)W; }
    const unsigned total = (unsigned)(N * p.tx * p.ty);
    const double px = (double)N * H * W;
    GtScope gt(s, "safm", (2.0 * dim * dim + 18.0 * dim) * px, 6.0 * c_pad * px);
    const int kp = safm_kp(c_pad);
    return kp == 64 ? safm_go<2>(p, total, s) : kp == 128 ? safm_go<4>(p, total, s) : safm_go<8>(p, total, s);
}

// out = fp16(a + b) over n halfs (a multiple of 8): SAFMN's global skip
int slab_add_launch(const f16* a, const f16* b, f16* out, long n, hipStream_t s) {
    hipLaunchKernelGGL(slab_add_kernel, dim3((unsigned)((n / 8 + 255) / 256)), dim3(256), 0, s, a, b, out, n / 8);
    INNFER_HIP(hipGetLastError());
    return INNFER_OK;
}

// The launch alone, for tests: safm_launch, the code the network runs.  Host floats: aggr [dim][dim] and [dim], mfr taps [dim][9] and bias [dim].  Uploads, launches, waits.
extern "C" int innfer_safm(const void* d_u, int64_t u_gs, const void* d_t, int64_t t_gs, void* d_out, int64_t out_gs, int N, int H, int W, int dim, int c_pad,
                           const float* h_aggr_w, const float* h_aggr_b, const float* h_taps, const float* h_bias, void* stream) {
    if (int rc = safm_refuse(d_u, (long)u_gs, d_t, (long)t_gs, d_out, (long)out_gs, N, H, W, dim, c_pad, h_aggr_w, h_aggr_b, h_taps)) return rc;
    if (!h_bias) return set_error(INNFER_ERR_INVALID, "safm: null argument");
    const int kp = safm_kp(c_pad);
    std::vector<f16> wq((size_t)kp * kp);
    std::vector<float> ab(kp);
    safm_pack(h_aggr_w, h_aggr_b, dim, kp, wq.data(), ab.data());
    Upload b("safm", {{ab.data(), (size_t)kp}, {h_taps, (size_t)dim * 9}, {h_bias, (size_t)dim}, {(const float*)wq.data(), (size_t)kp * kp / 2}});
    int rc = b.rc;
    if (rc == INNFER_OK)
        rc = safm_launch((const f16*)d_u, (long)u_gs, (const f16*)d_t, (long)t_gs, (f16*)d_out, (long)out_gs, N, H, W, dim, c_pad, (const f16*)(b.d + kp + (size_t)dim * 10), b.d,
                         b.d + kp, (hipStream_t)stream);
    return finish("safm", rc, stream);
}

}  // namespace innfer
