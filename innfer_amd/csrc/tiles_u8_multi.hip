// The uint8 chop path for MANY images at once (`-batch`, Model.run_u8_batch): one tile gather and one blend for n images of different sizes that share the
// channel count C and the tile size ps, packed in one device buffer.  The tiles of image 0 in its own innfer_chop_plan order, then image 1's, ... form ONE
// tile stream, so small images fill a network launch together instead of one launch each on a fraction of the chip.
//   - innfer_chop_multi_plan (host only) writes the geometry into caller memory: ps, tile counts, running tile counts, packed byte offsets, a per-tile table
//     for the gather (image offset, H, W, tile origin: no search and no division in the kernel) and a per-image table for the blend.  The caller uploads the
//     two tables; the library copies nothing.
//   - k_extract_u8_multi is k_extract_u8 of tiles_u8.hip with the image and the tile origin read from the table: tile first_i + k is bit for bit tile k of
//     innfer_extract_tiles_u8_seamless of image i.
//   - k_recompose_u8_multi is k_recompose_u8 with grid z = image and the frame read from the table: image i's bytes are innfer_recompose_u8_seamless's.
// Both are built from load_run, put_run, blend_at and store_px of tiles_u8_common.h, so the element arithmetic is the single-image kernels' by construction.
// One read + one write per element, 64-bit offsets, no LDS, no atomics.
#include "common.h"
#include "tiles_u8_common.h"

#pragma clang fp contract(off)

namespace innfer {
namespace {

// The gather: one block row of the grid per tile (table and tiles point at the launch's first tile), V consecutive pixels of one tile row per thread, R tile
// rows per block layer -- k_extract_u8's thread map.
template <typename TO, int C, int V>
__global__ void __launch_bounds__(256) k_extract_u8_multi(const uint8_t* imgs, const innfer_multi_tile* table, TO* tiles, int pad, int mode, int ps, int R,
                                                           int normalize) {
    const int q = ps / V;
    const int t = blockIdx.x * 256 + threadIdx.x;             // over R * (ps / V)
    const int yr = t / q, y = blockIdx.z * R + yr, x = (t - yr * q) * V;
    if (yr >= R || y >= ps) return;
    const innfer_multi_tile e = table[blockIdx.y];
    Run<uint8_t, C * V, 1> p = {};
    const int sy = border_index(e.oy + y - pad, e.H, mode);
    if (sy >= 0) p = load_run<C, V>(imgs + e.img_off + (long)sy * e.W * C, e.ox + x - pad, e.W, mode, false);
    put_run<TO, C, V, false>(p, tiles, blockIdx.y, 0, (long)ps * ps, (long)y * ps + x, normalize, 0);
}

// The blend: grid z = image (images points at the launch's first image), y = output rows from y0 up to the tallest result, x = 256 output pixels; threads
// outside their image's crop window leave.  blend_at at (Yo + cs, Xo + cs) of the image's own FH x FW frame over its own tiles, then store_px.
template <typename TI, typename TO, int C>
__global__ void __launch_bounds__(256) k_recompose_u8_multi(const TI* tiles, const innfer_multi_image* images, int P, int eff, int ov, int cs, int y0,
                                                             int denormalize, uint8_t* out) {
    const innfer_multi_image d = images[blockIdx.z];
    const int OW = d.FW - 2 * cs, OH = d.FH - 2 * cs;
    const int Xo = blockIdx.x * 256 + threadIdx.x, Yo = y0 + blockIdx.y;
    if (Xo >= OW || Yo >= OH) return;
    TO r[C];
    blend_at<TI, TO, C, C>(tiles + d.first * C * P * P, 0, 0, P, d.FH, d.FW, d.nh, d.nw, eff, ov, Yo + cs, Xo + cs, r);
    store_px<TO, C, false>(r, 0, -1, denormalize, out + d.out_off + ((long)Yo * OW + Xo) * C);
}

constexpr int64_t kPackAlign = 16;                            // every image starts on a 16-byte boundary of the packed buffers
inline int64_t pack_up(int64_t v) { return (v + kPackAlign - 1) / kPackAlign * kPackAlign; }

// What every entry point checks of the image set, and the geometry they share: ps and the tile total; 0 or the error already set.
int multi_geometry(const char* who, int n_images, const int* sizes, int C, int pad, int mode, int patch, double step, int* ps_out, long* total_out) {
    if (n_images <= 0 || !sizes) return set_error(INNFER_ERR_INVALID, "%s: %d images / null sizes", who, n_images);
    if (C < 1 || C > 4) return set_error(INNFER_ERR_INVALID, "%s: %d channels (1 .. 4)", who, C);
    int ps0 = 0;
    long total = 0;
    for (int i = 0; i < n_images; ++i) {
        const int H = sizes[2 * i], W = sizes[2 * i + 1];
        if (int rc = check_border(who, H, W, pad, mode)) return rc;
        int ps, nh, nw;
        if (int rc = innfer_chop_plan(H + 2 * pad, W + 2 * pad, patch, step, &ps, &nh, &nw, nullptr, nullptr)) return rc;
        if (i == 0) ps0 = ps;
        else if (ps != ps0)
            return set_error(INNFER_ERR_INVALID, "%s: image %d (%dx%d) has tiles of %d, image 0 of %d: one tile stream needs one tile size", who, i, H, W, ps, ps0);
        total += (long)nh * nw;
        if (total > 0x7fffffffL) return set_error(INNFER_ERR_INVALID, "%s: more than 2^31 - 1 tiles", who);
    }
    *ps_out = ps0;
    *total_out = total;
    return INNFER_OK;
}

}  // namespace
}  // namespace innfer

using namespace innfer;

extern "C" int innfer_chop_multi_plan(int n_images, const int* sizes, int C, int pad, int patch, double step, int scale, int* ps_out, int* counts, int* first,
                                      int64_t* in_off, int64_t* out_off, innfer_multi_tile* tiles, innfer_multi_image* images) {
    int ps;
    long total;
    if (int rc = multi_geometry("chop_multi_plan", n_images, sizes, C, pad, INNFER_BORDER_REPLICATE, patch, step, &ps, &total)) return rc;
    if (scale < 1) return set_error(INNFER_ERR_INVALID, "chop_multi_plan: scale %d", scale);
    const int step_int = (int)(ps * step);
    int64_t in = 0, out = 0;
    long k = 0;
    for (int i = 0; i < n_images; ++i) {
        const int H = sizes[2 * i], W = sizes[2 * i + 1], HP = H + 2 * pad, WP = W + 2 * pad;
        int nh, nw;
        innfer_chop_plan(HP, WP, patch, step, nullptr, &nh, &nw, nullptr, nullptr);
        if ((long)scale * HP > 0x7fffffffL / 2 || (long)scale * WP > 0x7fffffffL / 2) return set_error(INNFER_ERR_INVALID, "chop_multi_plan: output size overflows");
        const int64_t in_bytes = (int64_t)H * W * C, out_bytes = (int64_t)scale * H * scale * W * C;
        if (in > INT64_MAX / 4 - in_bytes || out > INT64_MAX / 4 - out_bytes) return set_error(INNFER_ERR_INVALID, "chop_multi_plan: packed size overflows");
        if (counts) counts[i] = nh * nw;
        if (first) first[i] = (int)k;
        if (in_off) in_off[i] = in;
        if (out_off) out_off[i] = out;
        if (images) images[i] = innfer_multi_image{out, (int64_t)k, scale * HP, scale * WP, nh, nw};
        if (tiles)
            for (int th = 0; th < nh; ++th)
                for (int tw = 0; tw < nw; ++tw) {
                    int oy = th * step_int; if (oy > HP - ps) oy = HP - ps;
                    int ox = tw * step_int; if (ox > WP - ps) ox = WP - ps;
                    tiles[k + (long)th * nw + tw] = innfer_multi_tile{in, H, W, oy, ox};
                }
        k += (long)nh * nw;
        in = pack_up(in + in_bytes);
        out = pack_up(out + out_bytes);
    }
    if (ps_out) *ps_out = ps;
    if (first) first[n_images] = (int)k;
    if (in_off) in_off[n_images] = in;
    if (out_off) out_off[n_images] = out;
    return INNFER_OK;
}

extern "C" int innfer_extract_tiles_u8_multi(const uint8_t* d_imgs, int n_images, const int* sizes, int C, int normalize, int patch, double step, int pad, int mode,
                                             const innfer_multi_tile* d_table, void* d_tiles, int tile_dtype, void* stream) {
    const char* who = "extract_tiles_u8_multi";
    if (!d_imgs || !d_table || !d_tiles) return set_error(INNFER_ERR_INVALID, "%s: null argument", who);
    int ps;
    long total;
    if (int rc = multi_geometry(who, n_images, sizes, C, pad, mode, patch, step, &ps, &total)) return rc;
    if (!is_float_dtype(tile_dtype)) return set_error(INNFER_ERR_INVALID, "%s: bad dtype %d", who, tile_dtype);
    hipStream_t s = (hipStream_t)stream;
    const long pp = (long)ps * ps;
    const bool x4 = ps % 4 == 0;
    const int q = x4 ? ps / 4 : ps, R = ps < (1 << 28) / q ? ps : (1 << 28) / q;      // R * q threads per tile and block layer fit an int
#define EX(V) hipLaunchKernelGGL((k_extract_u8_multi<TO, CC, V>), g, dim3(256), 0, s, d_imgs, d_table + b, (TO*)d_tiles + b * CC * pp, pad, mode, ps, R, normalize)
    for (long b = 0; b < total; b += 65535) {                 // tiles are the grid's y: at most 65535 per launch
        const dim3 g(blocks((long)R * q, 256), (unsigned)(total - b < 65535 ? total - b : 65535), (ps + R - 1) / R);
        with_dtype(tile_dtype, [&](auto to) { with_form(false, C, [&](auto c, auto) {
            using TO = decltype(to);
            constexpr int CC = decltype(c)::value;
            if (x4) EX(4); else EX(1);
        }); });
    }
#undef EX
    INNFER_HIP(hipGetLastError());
    return INNFER_OK;
}

extern "C" int innfer_recompose_u8_multi(const void* d_tiles, int dtype, int n_images, const int* sizes, int C, int P, int patch, double step, int scale,
                                         int via_dtype, int denormalize, int pad, const innfer_multi_image* d_images, uint8_t* d_out, void* stream) {
    const char* who = "recompose_u8_multi";
    if (!d_tiles || !d_images || !d_out) return set_error(INNFER_ERR_INVALID, "%s: null argument", who);
    if (P <= 0 || scale <= 0 || P % scale) return set_error(INNFER_ERR_INVALID, "%s: tiles of %d at scale %d (a positive multiple of the scale)", who, P, scale);
    int ps;
    long total;
    if (int rc = multi_geometry(who, n_images, sizes, C, pad, INNFER_BORDER_REPLICATE, patch, step, &ps, &total)) return rc;
    if (ps != P / scale) return set_error(INNFER_ERR_INVALID, "%s: tiles of %d are not the images' tile size %d x scale %d", who, P, ps, scale);
    if (!is_float_dtype(dtype) || !is_float_dtype(via_dtype)) return set_error(INNFER_ERR_INVALID, "%s: bad dtype", who);
    BlendGeo g = {};
    int max_oh = 0, max_ow = 0;
    for (int i = 0; i < n_images; ++i) {                     // every image's blend geometry is what innfer_recompose_u8_seamless checks, on the gather's lattice
        const int HP = sizes[2 * i] + 2 * pad, WP = sizes[2 * i + 1] + 2 * pad;
        int nh, nw;
        innfer_chop_plan(HP, WP, ps, step, nullptr, &nh, &nw, nullptr, nullptr);
        if (int rc = blend_geo(who, nh * nw, P, HP, WP, step, scale, pad, false, &g)) return rc;
        if (g.nh != nh || g.nw != nw) return set_error(INNFER_ERR_INVALID, "%s: image %d blends %dx%d tiles, its lattice has %dx%d", who, i, g.nh, g.nw, nh, nw);
        max_oh = max_oh > g.FH - 2 * g.cs ? max_oh : g.FH - 2 * g.cs;
        max_ow = max_ow > g.FW - 2 * g.cs ? max_ow : g.FW - 2 * g.cs;
    }
    hipStream_t s = (hipStream_t)stream;
    for (int b = 0; b < n_images; b += 65535)                 // images are the grid's z, rows its y: at most 65535 of each per launch
        for (int y0 = 0; y0 < max_oh; y0 += 65535) {
            const dim3 grid((max_ow + 255) / 256, (unsigned)(max_oh - y0 < 65535 ? max_oh - y0 : 65535), (unsigned)(n_images - b < 65535 ? n_images - b : 65535));
            with_dtype(dtype, [&](auto ti) { with_dtype(via_dtype, [&](auto to) { with_form(false, C, [&](auto c, auto) {
                hipLaunchKernelGGL((k_recompose_u8_multi<decltype(ti), decltype(to), decltype(c)::value>), grid, dim3(256), 0, s, (const decltype(ti)*)d_tiles,
                                   d_images + b, P, g.eff, g.ov, g.cs, y0, denormalize, d_out);
            }); }); });
        }
    INNFER_HIP(hipGetLastError());
    return INNFER_OK;
}
