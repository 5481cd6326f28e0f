// The uint8 chop path (ABI 113 / 115 / 117): ONE tile gather and ONE blend serve the plain, the fit_channels, the seamless and the seamless + fit forms.
//   - k_extract_u8 reads the uint8 image through the border index map: the tiles of the image as if it had been padded by `pad` pixels with its own
//     continuation (wrap, mirror, edge replicate) or with transparent black.  pad = 0: the map is the identity -- innfer_extract_tiles_u8 / _fit.
//   - k_recompose_u8 computes and stores only the crop window of the blend, quantised to uint8.  crop = 0: the whole blend -- innfer_recompose_u8 / _fit.
//   - innfer_pad_inthwc materialises the padded image for every path that is not fused (whole-image forwards, model chains, 16-bit images).
// Neither the padded image nor the padded result ever exists on the chop path.  One read + one write per element like the kernels of tiles.hip; no LDS, no
// atomics.  The element arithmetic is the helpers of tiles_common.h in the order of the separate passes (k_u8_to_nchw + k_extract, k_recompose +
// k_nchw_to_u8 of tiles.hip), so the results are theirs bit for bit.
// The kernels' bodies -- load_run, put_run, blend_at, store_px -- and the host's form dispatch and refusals are tiles_u8_common.h, shared with the
// self-ensemble's kernels (tiles_tta.hip) and deliberately NOT with tiles.hip, whose separate passes stay the independent anchors of the tests.
#include "common.h"
#include "tiles_u8_common.h"

#pragma clang fp contract(off)

namespace innfer {
namespace {

template <typename T, int C>
__global__ void __launch_bounds__(256) k_pad_inthwc(const T* img, T* out, int H, int W, int pad, int mode, int WP) {
    const int X = blockIdx.x * 256 + threadIdx.x, Y = blockIdx.y;
    if (X >= WP) return;
    constexpr int A = C == 3 ? sizeof(T) : sizeof(T) * C;
    const int sy = border_index(Y - pad, H, mode), sx = border_index(X - pad, W, mode);
    Run<T, C, A> p;
#pragma unroll
    for (int c = 0; c < C; ++c) p.v[c] = 0;
    if (sy >= 0 && sx >= 0) p = *(const Run<T, C, A>*)(img + ((long)sy * W + sx) * C);
    *(Run<T, C, A>*)(out + ((long)Y * WP + X) * C) = p;
}

// any channel count
template <typename T>
__global__ void __launch_bounds__(256) k_pad_inthwc_n(const T* img, T* out, int H, int W, int C, int pad, int mode, int WP) {
    const int X = blockIdx.x * 256 + threadIdx.x, Y = blockIdx.y;
    if (X >= WP) return;
    const int sy = border_index(Y - pad, H, mode), sx = border_index(X - pad, W, mode);
    const bool in = sy >= 0 && sx >= 0;
    const T* src = img + ((long)sy * W + sx) * C;
    T* dst = out + ((long)Y * WP + X) * C;
    for (int c = 0; c < C; ++c) dst[c] = in ? src[c] : (T)0;
}

// The gather.  FIT false: tiles [count, C, ps, ps], channels flipped BGR(A) -> RGB(A) (np2tensor + extract_patches_2d).  FIT true: colour tile k at slot
// k - tile_begin ((g, g, g) from gray, RGB from BGRA), its alpha tile (a, a, a) at slot count + k - tile_begin when `alpha`, [3, ps, ps] each.  The lattice is
// that of the virtual padded image.  One block row of the grid per tile, V consecutive pixels of one tile row per thread, R tile rows per block layer
// (grid.z; R = ps unless ps * ps / V would overflow an int).  The row map is computed once per thread; the run along the row is load_run's, the stores
// put_run's.  Outside the image under alpha_pad every byte is 0 and takes the same arithmetic.  V = 4 needs ps % 4 == 0 (the tile stores are then aligned).
template <typename TO, int C, int V, bool FIT>
__global__ void __launch_bounds__(256) k_extract_u8(const uint8_t* img, TO* tiles, int H, int W, int pad, int mode, int ps, int R, int step_int, int nw,
                                                     int tile_begin, int count, int normalize, int alpha) {
    const int q = ps / V;
    const int t = blockIdx.x * 256 + threadIdx.x;             // over R * (ps / V)
    const int yr = t / q, y = blockIdx.z * R + yr, x = (t - yr * q) * V;
    if (yr >= R || y >= ps) return;
    const int kk = blockIdx.y, k = kk + tile_begin;
    const int th = k / nw, tw = k - th * nw;
    const int HP = H + 2 * pad, WP = W + 2 * pad;
    int oy = th * step_int; if (oy > HP - ps) oy = HP - ps;
    int ox = tw * step_int; if (ox > WP - ps) ox = WP - ps;
    Run<uint8_t, C * V, 1> p = {};
    const int sy = border_index(oy + y - pad, H, mode);
    if (sy >= 0) p = load_run<C, V>(img + (long)sy * W * C, ox + x - pad, W, mode, false);
    put_run<TO, C, V, FIT>(p, tiles, kk, count + kk, (long)ps * ps, (long)y * ps + x, normalize, alpha);
}

// any channel count (pad = 0 only): one element per thread, 3 n channels fully flipped
template <typename TO>
__global__ void k_extract_u8_n(const uint8_t* img, TO* tiles, int C, int H, int W, int ps, int step_int, int nw, int tile_begin, long total, int normalize) {
    long i = (long)blockIdx.x * blockDim.x + threadIdx.x;      // over count*C*ps*ps
    if (i >= total) return;
    const int x = (int)(i % ps);
    const int y = (int)((i / ps) % ps);
    const int c = (int)((i / ((long)ps * ps)) % C);
    const int k = (int)(i / ((long)ps * ps * C)) + tile_begin;
    const int th = k / nw, tw = k % nw;
    int oy = th * step_int; if (oy > H - ps) oy = H - ps;
    int ox = tw * step_int; if (ox > W - ps) ox = W - ps;
    const int sc = C % 3 == 0 ? C - 1 - c : c;
    tiles[i] = (TO)to_unit((float)img[((long)(oy + y) * W + ox + x) * C + sc], 255.0f, normalize);
}

// The blend: k_recompose of tiles.hip with tensor2np as the store.  FIT false: tiles [n, C, P, P], each blended channel rounded to TO (the tensor
// recompose_tensor would have returned), quantised and flipped RGB(A) -> BGR(A).  FIT true: colour tiles [0, n) and, with `alpha`, alpha tiles [n, 2 n),
// three channels each; B, G, R (C 4) or mean3 (gray) of the colour result, mean3 of the alpha result or the constant alpha `aconst` (>= 0).  Only the crop
// window is computed: output pixel (Yo, Xo) is pixel (Yo + cs, Xo + cs) of the full FH x FW blend, cs = scale * crop: blend_at there, then store_px.  One
// thread per output pixel, its C bytes in one store.
template <typename TI, typename TO, int C, bool FIT>
__global__ void __launch_bounds__(256) k_recompose_u8(const TI* tiles, int n, int P, int FH, int FW, int eff, int nh, int nw, int ov, int cs, int OW,
                                                                int alpha, int aconst, int denormalize, uint8_t* img) {
    const int Xo = blockIdx.x * 256 + threadIdx.x, Yo = blockIdx.y;
    if (Xo >= OW) return;
    using F = Form<C, FIT>;
    TO r[F::NC];
    blend_at<TI, TO, F::NT, F::NC>(tiles, (long)n * 3 * P * P, alpha, P, FH, FW, nh, nw, eff, ov, Yo + cs, Xo + cs, r);
    store_px<TO, C, FIT>(r, alpha, aconst, denormalize, img + ((long)Yo * OW + Xo) * C);
}

}  // namespace
}  // namespace innfer

using namespace innfer;

extern "C" int innfer_border_index(int i, int n, int mode) {
    if (n < 1 || mode < INNFER_BORDER_TILE || mode > INNFER_BORDER_ALPHA_PAD) {
        set_error(INNFER_ERR_INVALID, "border_index: n=%d mode=%d", n, mode);
        return INNFER_BORDER_ERROR;
    }
    if (mode == INNFER_BORDER_MIRROR && n < 2) {
        set_error(INNFER_ERR_INVALID, "border_index: mirror needs n >= 2 (period 2 (n - 1)), got n=%d", n);
        return INNFER_BORDER_ERROR;
    }
    return border_index(i, n, mode);
}

extern "C" int innfer_pad_inthwc(const void* d_img, int bits, int H, int W, int C, int pad, int mode, void* d_out, void* stream) {
    if (!d_img || !d_out || C <= 0 || (bits != 8 && bits != 16)) return set_error(INNFER_ERR_INVALID, "pad_inthwc: null argument / bits %d (8, 16) / C %d", bits, C);
    if (int rc = check_border("pad_inthwc", H, W, pad, mode)) return rc;
    const int HP = H + 2 * pad, WP = W + 2 * pad;
    if (HP > 65535) return set_error(INNFER_ERR_UNSUPPORTED, "pad_inthwc: %d rows exceed the launch grid", HP);
    hipStream_t s = (hipStream_t)stream;
    const dim3 g((WP + 255) / 256, HP), b(256);
#define PADK(T, CC) hipLaunchKernelGGL((k_pad_inthwc<T, CC>), g, b, 0, s, (const T*)d_img, (T*)d_out, H, W, pad, mode, WP)
#define PAD_T(T) do { if (C == 1) PADK(T, 1); else if (C == 2) PADK(T, 2); else if (C == 3) PADK(T, 3); else if (C == 4) PADK(T, 4); \
                      else hipLaunchKernelGGL(k_pad_inthwc_n<T>, g, b, 0, s, (const T*)d_img, (T*)d_out, H, W, C, pad, mode, WP); } while (0)
    if (bits == 8) PAD_T(uint8_t); else PAD_T(uint16_t);
#undef PAD_T
#undef PADK
    INNFER_HIP(hipGetLastError());
    return INNFER_OK;
}

// the four gathers: C and FIT pick the kernel, the rest is shared.  The plain entry points pass pad = 0 and INNFER_BORDER_REPLICATE (no division, no refusal).
static int extract_u8(const char* who, bool fit, const uint8_t* d_img, int C, int H, int W, int normalize, int patch, double step, int tile_begin,
                      int tile_count, int alpha, int pad, int mode, void* d_tiles, int tile_dtype, hipStream_t s) {
    if (!d_img || !d_tiles) return set_error(INNFER_ERR_INVALID, "%s: null argument", who);
    if (int rc = check_u8_form(who, fit, C, alpha, -1, false)) return rc;
    if (alpha && C == 1) return set_error(INNFER_ERR_INVALID, "%s: a 1-channel image has no alpha", who);
    if (C > 4 && pad > 0) return set_error(INNFER_ERR_UNSUPPORTED, "%s: %d channels with a border (built: 1 .. 4, what innfer_recompose_u8 stores)", who, C);
    if (int rc = check_border(who, H, W, pad, mode)) return rc;
    int ps, nh, nw;
    if (int rc = innfer_chop_plan(H + 2 * pad, W + 2 * pad, patch, step, &ps, &nh, &nw, nullptr, nullptr)) return rc;
    const int step_int = (int)(ps * step);
    if (tile_begin < 0 || tile_count < 0 || tile_begin + tile_count > nh * nw)
        return set_error(INNFER_ERR_INVALID, "%s: tile range [%d,+%d) outside %d tiles", who, tile_begin, tile_count, nh * nw);
    if (tile_count == 0) return INNFER_OK;
    if (!is_float_dtype(tile_dtype)) return set_error(INNFER_ERR_INVALID, "%s: bad dtype %d", who, tile_dtype);
    const long pp = (long)ps * ps;
    if (C > 4) {
        const long total = (long)tile_count * C * pp;
        if (tile_dtype == INNFER_F16)
            hipLaunchKernelGGL(k_extract_u8_n<f16>, dim3(blocks(total, 256)), dim3(256), 0, s, d_img, (f16*)d_tiles, C, H, W, ps, step_int, nw, tile_begin, total, normalize);
        else
            hipLaunchKernelGGL(k_extract_u8_n<float>, dim3(blocks(total, 256)), dim3(256), 0, s, d_img, (float*)d_tiles, C, H, W, ps, step_int, nw, tile_begin, total, normalize);
        INNFER_HIP(hipGetLastError());
        return INNFER_OK;
    }
    const bool x4 = ps % 4 == 0;
    const int q = x4 ? ps / 4 : ps, R = ps < (1 << 28) / q ? ps : (1 << 28) / q;      // R * q threads per tile and block layer fit an int
    const int a = alpha ? 1 : 0;
#define EX(V) hipLaunchKernelGGL((k_extract_u8<TO, CC, V, F>), g, dim3(256), 0, s, d_img, dst, H, W, pad, mode, ps, R, step_int, nw, tile_begin + (int)b, tile_count, normalize, a)
    for (long b = 0; b < tile_count; b += 65535) {            // tiles are the grid's y: at most 65535 per launch; `count` stays the alpha slot base
        const dim3 g(blocks((long)R * q, 256), (unsigned)(tile_count - b < 65535 ? tile_count - b : 65535), (ps + R - 1) / R);
        with_dtype(tile_dtype, [&](auto to) { with_form(fit, C, [&](auto c, auto f) {
            using TO = decltype(to);
            constexpr int CC = decltype(c)::value;
            constexpr bool F = decltype(f)::value;
            TO* dst = (TO*)d_tiles + b * Form<CC, F>::NT * pp;
            if (x4) EX(4); else EX(1);
        }); });
    }
#undef EX
    INNFER_HIP(hipGetLastError());
    return INNFER_OK;
}

extern "C" int innfer_extract_tiles_u8(const uint8_t* d_img, int C, int H, int W, int normalize, int patch, double step,
                                       int tile_begin, int tile_count, void* d_tiles, int tile_dtype, void* stream) {
    return extract_u8("extract_tiles_u8", false, d_img, C, H, W, normalize, patch, step, tile_begin, tile_count, 0, 0, INNFER_BORDER_REPLICATE, d_tiles, tile_dtype,
                      (hipStream_t)stream);
}

extern "C" int innfer_extract_tiles_u8_fit(const uint8_t* d_img, int C, int H, int W, int normalize, int patch, double step,
                                           int tile_begin, int tile_count, int alpha, void* d_tiles, int tile_dtype, void* stream) {
    return extract_u8("extract_tiles_u8_fit", true, d_img, C, H, W, normalize, patch, step, tile_begin, tile_count, alpha, 0, INNFER_BORDER_REPLICATE, d_tiles, tile_dtype,
                      (hipStream_t)stream);
}

extern "C" int innfer_extract_tiles_u8_seamless(const uint8_t* d_img, int C, int H, int W, int normalize, int patch, double step,
                                                int tile_begin, int tile_count, int pad, int mode, void* d_tiles, int tile_dtype, void* stream) {
    return extract_u8("extract_tiles_u8_seamless", false, d_img, C, H, W, normalize, patch, step, tile_begin, tile_count, 0, pad, mode, d_tiles, tile_dtype,
                      (hipStream_t)stream);
}

extern "C" int innfer_extract_tiles_u8_fit_seamless(const uint8_t* d_img, int C, int H, int W, int normalize, int patch, double step,
                                                    int tile_begin, int tile_count, int alpha, int pad, int mode, void* d_tiles, int tile_dtype, void* stream) {
    return extract_u8("extract_tiles_u8_fit_seamless", true, d_img, C, H, W, normalize, patch, step, tile_begin, tile_count, alpha, pad, mode, d_tiles, tile_dtype,
                      (hipStream_t)stream);
}

// the four blends: C and FIT pick the kernel, the rest is shared.  The plain entry points pass crop = 0.
static int recompose_u8(const char* who, bool fit, const void* d_tiles, int dtype, int n, int C, int P, int height, int width, double step, int scale,
                        int via_dtype, int denormalize, int alpha, int alpha_const, int crop, uint8_t* d_img, hipStream_t s) {
    if (!d_tiles || !d_img) return set_error(INNFER_ERR_INVALID, "%s: null argument", who);
    if (int rc = check_u8_form(who, fit, C, alpha, alpha_const, true)) return rc;
    BlendGeo g;
    if (int rc = blend_geo(who, n, P, height, width, step, scale, crop, false, &g)) return rc;
    const int OH = g.FH - 2 * g.cs, OW = g.FW - 2 * g.cs;
    if (OH > 65535) return set_error(INNFER_ERR_UNSUPPORTED, "%s: %d output rows exceed the launch grid", who, OH);
    const dim3 grid((OW + 255) / 256, OH), block(256);
    const int a = alpha ? 1 : 0;
    if (!is_float_dtype(dtype) || !is_float_dtype(via_dtype)) return set_error(INNFER_ERR_INVALID, "%s: bad dtype", who);
    with_dtype(dtype, [&](auto ti) { with_dtype(via_dtype, [&](auto to) { with_form(fit, C, [&](auto c, auto f) {
        hipLaunchKernelGGL((k_recompose_u8<decltype(ti), decltype(to), decltype(c)::value, decltype(f)::value>), grid, block, 0, s, (const decltype(ti)*)d_tiles, n, P,
                           g.FH, g.FW, g.eff, g.nh, g.nw, g.ov, g.cs, OW, a, alpha_const, denormalize, d_img);
    }); }); });
    INNFER_HIP(hipGetLastError());
    return INNFER_OK;
}

extern "C" int innfer_recompose_u8(const void* d_tiles, int dtype, int n, int C, int P, int height, int width, double step, int scale,
                                   int via_dtype, int denormalize, uint8_t* d_img, void* stream) {
    return recompose_u8("recompose_u8", false, d_tiles, dtype, n, C, P, height, width, step, scale, via_dtype, denormalize, 0, -1, 0, d_img, (hipStream_t)stream);
}

extern "C" int innfer_recompose_u8_fit(const void* d_tiles, int dtype, int n, int P, int height, int width, double step, int scale,
                                       int via_dtype, int denormalize, int C, int alpha, int alpha_const, uint8_t* d_img, void* stream) {
    return recompose_u8("recompose_u8_fit", true, d_tiles, dtype, n, C, P, height, width, step, scale, via_dtype, denormalize, alpha, alpha_const, 0, d_img,
                        (hipStream_t)stream);
}

extern "C" int innfer_recompose_u8_seamless(const void* d_tiles, int dtype, int n, int C, int P, int height, int width, double step, int scale,
                                            int via_dtype, int denormalize, int crop, uint8_t* d_img, void* stream) {
    return recompose_u8("recompose_u8_seamless", false, d_tiles, dtype, n, C, P, height, width, step, scale, via_dtype, denormalize, 0, -1, crop, d_img,
                        (hipStream_t)stream);
}

extern "C" int innfer_recompose_u8_fit_seamless(const void* d_tiles, int dtype, int n, int P, int height, int width, double step, int scale,
                                                int via_dtype, int denormalize, int C, int alpha, int alpha_const, int crop, uint8_t* d_img, void* stream) {
    return recompose_u8("recompose_u8_fit_seamless", true, d_tiles, dtype, n, C, P, height, width, step, scale, via_dtype, denormalize, alpha, alpha_const, crop, d_img,
                        (hipStream_t)stream);
}
