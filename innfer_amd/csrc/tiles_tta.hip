// The self-ensemble on the uint8 chop path (ABI 119, `-tta`): the image runs through the network in its eight dihedral orientations and the eight results,
// turned back, are averaged before quantisation.  t_k, k = 0 .. 7: transpose if k & 4, then flip the columns if k & 1, then flip the rows if k & 2.
//   - k_extract_u8_tta / k_extract_u8_tta_t fill tiles [8 n (x 2 with alpha), C | 3, ps, ps]: slots [k n, (k + 1) n) hold the tiles of t_k(padded image) on
//     that orientation's OWN lattice (for k >= 4 that of a (W + 2 pad) x (H + 2 pad) image), every element read from the uint8 image through t_k^-1 and the
//     border index map.  Because the padding is `pad` on every side, t_k(pad(x)) == pad(t_k(x)).
//   - k_recompose_u8_tta computes, per output pixel, the blend of each orientation at the pixel's place in that orientation's frame (blend_at, the loop
//     of k_recompose_u8, rounded to TO), sums the eight in fp32 in the order k = 0 .. 7, multiplies by 0.125, rounds to TO and quantises.
// No rotated image, no per-orientation result and no accumulator image exists.  The element arithmetic IS that of tiles_u8.hip: load_run, put_run,
// blend_at and store_px of tiles_u8_common.h are the bodies of both files' kernels (k_extract_u8_tta_t keeps its own load, through LDS), and the host's
// form dispatch and refusals are that header's too.  tiles.hip deliberately shares none of it: its separate passes are what the tests hold all this to.
#include "common.h"
#include "tiles_u8_common.h"

#pragma clang fp contract(off)

namespace innfer {
namespace {

// Pixel (y, x) of t_k of an H x W image is pixel (*sy, *sx) of the image: t_k^-1 on coordinates.
__host__ __device__ __forceinline__ void dihedral_src(int k, int H, int W, int y, int x, int* sy, int* sx) {
    const int A = k & 4 ? W : H, B = k & 4 ? H : W;               // t_k of the image is A x B
    const int a = k & 2 ? A - 1 - y : y, b = k & 1 ? B - 1 - x : x;
    *sy = k & 4 ? b : a;
    *sx = k & 4 ? a : b;
}

// The gather of the orientations k = 0 .. 3 (no transpose): k_extract_u8 with the row map and the column map behind t_k^-1.  grid.y runs over the slots
// [slot_begin, ..) of [0, 4 n); slot = k n + tile.  A thread's V pixels lie along an image row, descending under a column flip: load_run is then called at
// the run's low end with `rev`.
template <typename TO, int C, int V, bool FIT>
__global__ void __launch_bounds__(256) k_extract_u8_tta(const uint8_t* img, TO* tiles, int H, int W, int pad, int mode, int ps, int R, int step_int, int nw,
                                                         int n, int slot_begin, int normalize, int alpha) {
    const int q = ps / V;
    const int t = blockIdx.x * 256 + threadIdx.x;             // over R * (ps / V)
    const int yr = t / q, y = blockIdx.z * R + yr, x = (t - yr * q) * V;
    if (yr >= R || y >= ps) return;
    const int slot = blockIdx.y + slot_begin;
    const int k = slot / n, i = slot - k * n;
    const int th = i / nw, tw = i - th * nw;
    const int HP = H + 2 * pad, WP = W + 2 * pad;
    int oy = th * step_int; if (oy > HP - ps) oy = HP - ps;
    int ox = tw * step_int; if (ox > WP - ps) ox = WP - ps;
    const bool rev = k & 1;
    const int Y = k & 2 ? HP - 1 - (oy + y) : oy + y;         // row of the padded image
    const int X0 = rev ? WP - 1 - (ox + x) - (V - 1) : ox + x; // lowest column of the run in the padded image
    Run<uint8_t, C * V, 1> p = {};
    const int sy = border_index(Y - pad, H, mode);
    if (sy >= 0) p = load_run<C, V>(img + (long)sy * W * C, X0 - pad, W, mode, rev);
    put_run<TO, C, V, FIT>(p, tiles, slot, (long)8 * n + slot, (long)ps * ps, (long)y * ps + x, normalize, alpha);
}

// The gather of the orientations k = 4 .. 7: a tile row lies along an image COLUMN.  A block moves a 32 x 32 patch of one tile through LDS so that both sides
// run along rows: in the first phase 32 consecutive lanes read 32 consecutive pixels of one image row (the patch's y direction), each pixel's C bytes as one
// dword of a [32][33] array (pitch 33: lane l writes bank l + r, reads bank l + r of the 32 ds_write_b32 / ds_read_b32 banks -- no conflict on either
// side); in the second phase 32 consecutive lanes store 32 consecutive elements of one tile row.  grid: x the patch column, y the slot of [4 n, 8 n) from
// slot_begin, z the patch row.  The lattice is that of the (W + 2 pad) x (H + 2 pad) image: nh and nw swap.
template <typename TO, int C, bool FIT>
__global__ void __launch_bounds__(256) k_extract_u8_tta_t(const uint8_t* img, TO* tiles, int H, int W, int pad, int mode, int ps, int step_int, int nh,
                                                           int n, int slot_begin, int normalize, int alpha) {
    __shared__ uint32_t lds[32][33];
    const int slot = blockIdx.y + slot_begin;
    const int k = slot / n, i = slot - k * n;
    const int th = i / nh, tw = i - th * nh;                  // nh tiles per row of this lattice
    const int A = W + 2 * pad, B = H + 2 * pad;               // t_k of the padded image is A x B
    int oy = th * step_int; if (oy > A - ps) oy = A - ps;
    int ox = tw * step_int; if (ox > B - ps) ox = B - ps;
    const int px = blockIdx.x * 32, py = blockIdx.z * 32;     // the patch's origin in the tile
    const int l = threadIdx.x & 31, g = threadIdx.x >> 5;
    constexpr int AP = C == 3 ? 1 : C;
    for (int r = g; r < 32; r += 8) {                         // lane l along the tile's y = the image's x; r along the tile's x = the image's y
        const int ty = py + l, tx = px + r;
        uint32_t v = 0;
        if (ty < ps && tx < ps) {
            const int a = k & 2 ? A - 1 - (oy + ty) : oy + ty, b = k & 1 ? B - 1 - (ox + tx) : ox + tx;
            const int sy = border_index(b - pad, H, mode), sx = border_index(a - pad, W, mode);      // the transpose: pixel (b, a) of the padded image
            if (sy >= 0 && sx >= 0) {
                const Run<uint8_t, C, AP> s = *(const Run<uint8_t, C, AP>*)(img + ((long)sy * W + sx) * C);
#pragma unroll
                for (int c = 0; c < C; ++c) v |= (uint32_t)s.v[c] << (8 * c);
            }
        }
        lds[r][l] = v;
    }
    __syncthreads();
    for (int r = g; r < 32; r += 8) {                         // lane l along the tile's x
        const int ty = py + r, tx = px + l;
        if (ty < ps && tx < ps) {
            const uint32_t v = lds[l][r];
            Run<uint8_t, C, 1> p;
#pragma unroll
            for (int c = 0; c < C; ++c) p.v[c] = (uint8_t)(v >> (8 * c));
            put_run<TO, C, 1, FIT>(p, tiles, slot, (long)8 * n + slot, (long)ps * ps, (long)ty * ps + tx, normalize, alpha);
        }
    }
}

// The blend.  Tiles [8 n, C, P, P], orientation k in slots [k n, (k + 1) n) on its own lattice (FIT: colour tiles [0, 8 n), alpha tiles [8 n, 16 n), three
// channels each).  Output pixel (Yo, Xo) is pixel (Yo + cs, Xo + cs) of the FH x FW frame; in orientation k's frame (FW x FH for k >= 4) it lies where t_k
// moves it, and its blend there is blend_at, as in k_recompose_u8: den per orientation, the quotient rounded to TO.  The eight are added as floats in
// the order k = 0 .. 7 (from 0.f: x + 0 is x), times 0.125f, rounded to TO; then store_px.  One thread per output pixel in blocks of 16 x 16 pixels: a
// block reads 16 consecutive elements of 16 tile rows in the straight and in the transposed orientations alike.  No LDS, no atomics.
template <typename TI, typename TO, int C, bool FIT>
__global__ void __launch_bounds__(256) k_recompose_u8_tta(const TI* tiles, int n, int P, int FH, int FW, int eff, int nh, int nw, int ov, int cs, int OH, int OW,
                                                           int alpha, int aconst, int denormalize, uint8_t* img) {
    const int Xo = blockIdx.x * 16 + (threadIdx.x & 15), Yo = blockIdx.y * 16 + (threadIdx.x >> 4);
    if (Xo >= OW || Yo >= OH) return;
    using F = Form<C, FIT>;
    float sum[F::NC];
#pragma unroll
    for (int c = 0; c < F::NC; ++c) sum[c] = 0.f;
    const long pp = (long)P * P;
    TO r[F::NC];
    for (int k = 0; k < 8; ++k) {
        const bool tr = k & 4;
        const int A = tr ? FW : FH, B = tr ? FH : FW;                     // orientation k: an A x B frame, its lattice nh x nw swapped with it
        int Y = tr ? Xo + cs : Yo + cs, X = tr ? Yo + cs : Xo + cs;
        if (k & 2) Y = A - 1 - Y;
        if (k & 1) X = B - 1 - X;
        blend_at<TI, TO, F::NT, F::NC>(tiles + (long)k * n * F::NT * pp, (long)8 * n * 3 * pp, alpha, P, A, B, tr ? nw : nh, tr ? nh : nw, eff, ov, Y, X, r);
#pragma unroll
        for (int c = 0; c < F::NC; ++c) sum[c] = __fadd_rn(sum[c], (float)r[c]);
    }
#pragma unroll
    for (int c = 0; c < F::NC; ++c) r[c] = (TO)__fmul_rn(sum[c], 0.125f);
    store_px<TO, C, FIT>(r, alpha, aconst, denormalize, img + ((long)Yo * OW + Xo) * C);
}

}  // namespace
}  // namespace innfer

using namespace innfer;

extern "C" int innfer_dihedral_index(int k, int H, int W, int y, int x, int* sy, int* sx) {
    if (!sy || !sx || k < 0 || k > 7 || H <= 0 || W <= 0) return set_error(INNFER_ERR_INVALID, "dihedral_index: k=%d (0 .. 7) H=%d W=%d / null argument", k, H, W);
    const int A = k & 4 ? W : H, B = k & 4 ? H : W;
    if (y < 0 || y >= A || x < 0 || x >= B) return set_error(INNFER_ERR_INVALID, "dihedral_index: pixel (%d, %d) outside the %dx%d image of orientation %d", y, x, A, B, k);
    dihedral_src(k, H, W, y, x, sy, sx);
    return INNFER_OK;
}

extern "C" int innfer_extract_tiles_u8_tta(const uint8_t* d_img, int C, int H, int W, int normalize, int patch, double step, int fit, int alpha,
                                           int pad, int mode, void* d_tiles, int tile_dtype, void* stream) {
    const char* who = "extract_tiles_u8_tta";
    if (!d_img || !d_tiles) return set_error(INNFER_ERR_INVALID, "%s: null argument", who);
    if (int rc = check_u8_form(who, fit, C, alpha, -1, false)) return rc;
    if (C > 4) return set_error(INNFER_ERR_UNSUPPORTED, "%s: %d channels (built: 1 .. 4, what innfer_recompose_u8_tta stores)", who, C);
    if (alpha && (C == 1 || !fit)) return set_error(INNFER_ERR_INVALID, "%s: alpha tiles need fit and an image with an alpha plane", who);
    if (int rc = check_border(who, H, W, pad, mode)) return rc;
    int ps, nh, nw;
    if (int rc = innfer_chop_plan(H + 2 * pad, W + 2 * pad, patch, step, &ps, &nh, &nw, nullptr, nullptr)) return rc;
    if (!is_float_dtype(tile_dtype)) return set_error(INNFER_ERR_INVALID, "%s: bad dtype %d", who, tile_dtype);
    const int step_int = (int)(ps * step);
    const long n = (long)nh * nw;
    if (16 * n > 0x7fffffffL) return set_error(INNFER_ERR_INVALID, "%s: %ld tiles per orientation overflow", who, n);
    if ((ps + 31) / 32 > 65535) return set_error(INNFER_ERR_UNSUPPORTED, "%s: patch %d exceeds the launch grid", who, ps);
    hipStream_t s = (hipStream_t)stream;
    const bool x4 = ps % 4 == 0;
    const int q = x4 ? ps / 4 : ps, R = ps < (1 << 28) / q ? ps : (1 << 28) / q;      // R * q threads per tile and block layer fit an int
    const int a = alpha ? 1 : 0, nn = (int)n;
#define EX(V) hipLaunchKernelGGL((k_extract_u8_tta<TO, CC, V, F>), g, dim3(256), 0, s, d_img, (TO*)d_tiles, H, W, pad, mode, ps, R, step_int, nw, nn, (int)b, normalize, a)
#define EXT() hipLaunchKernelGGL((k_extract_u8_tta_t<TO, CC, F>), gt, dim3(256), 0, s, d_img, (TO*)d_tiles, H, W, pad, mode, ps, step_int, nh, nn, (int)(4 * n + b), normalize, a)
    for (long b = 0; b < 4 * n; b += 65535) {                 // slots are the grid's y: at most 65535 per launch, the straight and the transposed half alike
        const unsigned cnt = (unsigned)(4 * n - b < 65535 ? 4 * n - b : 65535);
        const dim3 g(blocks((long)R * q, 256), cnt, (ps + R - 1) / R), gt((ps + 31) / 32, cnt, (ps + 31) / 32);
        with_dtype(tile_dtype, [&](auto to) { with_form(fit, C, [&](auto c, auto f) {
            using TO = decltype(to);
            constexpr int CC = decltype(c)::value;
            constexpr bool F = decltype(f)::value;
            if (x4) EX(4); else EX(1);
            EXT();
        }); });
    }
#undef EXT
#undef EX
    INNFER_HIP(hipGetLastError());
    return INNFER_OK;
}

extern "C" int innfer_recompose_u8_tta(const void* d_tiles, int dtype, int n, int C, int P, int height, int width, double step, int scale,
                                       int via_dtype, int denormalize, int fit, int alpha, int alpha_const, int crop, uint8_t* d_img, void* stream) {
    const char* who = "recompose_u8_tta";
    if (!d_tiles || !d_img) return set_error(INNFER_ERR_INVALID, "%s: null argument", who);
    if (C > 4) return set_error(INNFER_ERR_UNSUPPORTED, "%s: %d channels (built: 1 .. 4)", who, C);
    if (int rc = check_u8_form(who, fit, C, alpha, alpha_const, true)) return rc;
    BlendGeo g;
    if (int rc = blend_geo(who, n, P, height, width, step, scale, crop, false, &g)) return rc;
    if (16L * n > 0x7fffffffL) return set_error(INNFER_ERR_INVALID, "%s: %d tiles per orientation overflow", who, n);
    const int OH = g.FH - 2 * g.cs, OW = g.FW - 2 * g.cs;
    if ((OH + 15) / 16 > 65535) return set_error(INNFER_ERR_UNSUPPORTED, "%s: %d output rows exceed the launch grid", who, OH);
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((OW + 15) / 16, (OH + 15) / 16), block(256);
    const int a = alpha ? 1 : 0;
    if (!is_float_dtype(dtype) || !is_float_dtype(via_dtype)) return set_error(INNFER_ERR_INVALID, "%s: bad dtype", who);
    with_dtype(dtype, [&](auto ti) { with_dtype(via_dtype, [&](auto to) { with_form(fit, C, [&](auto c, auto f) {
        hipLaunchKernelGGL((k_recompose_u8_tta<decltype(ti), decltype(to), decltype(c)::value, decltype(f)::value>), grid, block, 0, s, (const decltype(ti)*)d_tiles, n, P,
                           g.FH, g.FW, g.eff, g.nh, g.nw, g.ov, g.cs, OH, OW, a, alpha_const, denormalize, d_img);
    }); }); });
    INNFER_HIP(hipGetLastError());
    return INNFER_OK;
}
