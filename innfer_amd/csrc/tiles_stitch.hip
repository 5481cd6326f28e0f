// The stitched tile path (`-tile N -tile_pad P`, Real-ESRGAN's --tile / --tile_pad): large rectangular tiles that carry a halo of context pixels, the halo
// thrown away.  Every output pixel comes from exactly ONE tile -- its owner -- and nothing is averaged, so the network runs on 1.05 .. 1.12x the image's
// pixels where the 200 / 0.5 chop of tiles.hip / tiles_u8.hip runs it on 3.7 .. 3.9x.
//
// Lattice, per axis of A pixels with tile core T >= 1 and halo h >= 0 (plan_axis):
//   A <= T + 2h :  n = 1, P = A, origin 0
//   otherwise   :  n = ceil((A - 2h) / T);  P = ceil((A + 2h (n - 1)) / n);  S = P - 2h;  o_i = min(i S, A - P)
//   owner(y)    =  the largest i with i == 0 or o_i + h <= y
// All tiles are P_h x P_w (balanced: 1080 rows at T = 1024 are two tiles of 556 rows), lie inside the image and are in row-major order.  An owned pixel is at
// least h away from every tile edge that is not an image edge.  o_i = i S for i < n - 1 and A - P for i = n - 1, so the owner has the closed form of
// owner_of below -- one integer division; the kernels use it in output pixels (everything times the scale).
//
// Kernels: a gather and a stitch, each in a tensor form (a copy, any C, fp16 / fp32) and a uint8 form (np2tensor as the gather's load through the border map
// of the seamless modes, tensor2np as the stitch's store, C 1 .. 4; the element arithmetic is load_run / put_run / store_px of tiles_u8_common.h and nothing
// else).  One read and one write per element, no LDS, no atomics.  Consecutive lanes are consecutive pixels of one row; a thread moves V of them as one
// 16-byte (tensor forms) / 8-byte load (uint8 stitch) where the run lies in one tile and its addresses are aligned, else one by one -- balanced tile widths
// are usually odd, so the scalar path is a first-class citizen.  Every tile and image offset is 64-bit.
#include "common.h"
#include "tiles_u8_common.h"

#pragma clang fp contract(off)

namespace innfer {
namespace {

// one axis of the lattice on the host: tiles, tile length, stride P - 2h (1 where n == 1), last origin A - P
struct Axis { int n, P, S, last; };

inline void plan_axis(int A, int T, int h, Axis* a) {
    if ((long)A <= (long)T + 2L * h) { a->n = 1; a->P = A; a->S = 1; a->last = 0; return; }
    const long n = (A - 2L * h + T - 1) / T;
    const long P = (A + 2L * h * (n - 1) + n - 1) / n;
    a->n = (int)n; a->P = (int)P; a->S = (int)(P - 2L * h); a->last = (int)(A - P);
}

// one axis as the kernels see it, in units of 1 / s low-resolution pixels (s = 1: the gathers): tiles, stride, last origin, halo (0 where n == 1)
struct Ax { int n, S, last, h; };

inline Ax scaled(const Axis& a, int h, int s) { return Ax{a.n, a.S * s, a.last * s, a.n > 1 ? h * s : 0}; }

__host__ __device__ __forceinline__ int origin_of(int i, const Ax& a) { return i == a.n - 1 ? a.last : i * a.S; }

// the tile that owns position X: the last one from last + h on, the first one below h, else (X - h) / S (which is < n - 1 there, as (n - 1) S >= last)
__host__ __device__ __forceinline__ int owner_of(int X, const Ax& a) {
    if (X - a.h >= a.last) return a.n - 1;
    return X < a.h ? 0 : (X - a.h) / a.S;
}

struct Lattice { Axis y, x; };

// what every entry point checks of (H, W, tile, halo, scale) and the lattice of the H x W image; 0 or the error already set
inline int lattice(const char* who, int H, int W, int tile, int halo, int scale, Lattice* g) {
    if (H <= 0 || W <= 0 || tile <= 0 || halo < 0 || scale <= 0)
        return set_error(INNFER_ERR_INVALID, "%s: bad sizes H=%d W=%d tile=%d halo=%d scale=%d", who, H, W, tile, halo, scale);
    if ((long)scale * H > 0x3fffffffL || (long)scale * W > 0x3fffffffL) return set_error(INNFER_ERR_INVALID, "%s: output size overflows", who);
    plan_axis(H, tile, halo, &g->y);
    plan_axis(W, tile, halo, &g->x);
    return INNFER_OK;
}

template <typename T> __device__ __forceinline__ bool aligned16(const T* a, const T* b) { return (((uintptr_t)a | (uintptr_t)b) & 15) == 0; }

// The tensor gather: img [1, C, H, W] -> tiles [count, C, PH, PW] of tiles tile_begin .. of the lattice.  grid (PW / V / 256, PH, count); a thread copies V
// consecutive elements of one tile row in every channel, 16 bytes at a time where both addresses are aligned.
template <typename T, int V>
__global__ void __launch_bounds__(256) k_gather_rect(const T* img, T* tiles, int C, int H, int W, int PH, int PW, int nw, Ax ay, Ax ax, int tile_begin) {
    typedef T vt __attribute__((ext_vector_type(V)));
    const int x0 = (blockIdx.x * 256 + threadIdx.x) * V, y = blockIdx.y;
    if (x0 >= PW) return;
    const int kk = blockIdx.z, k = kk + tile_begin, th = k / nw, tw = k - th * nw;
    const T* sp = img + (long)(origin_of(th, ay) + y) * W + origin_of(tw, ax) + x0;
    T* dp = tiles + ((long)kk * C * PH + y) * PW + x0;
    const long splane = (long)H * W, dplane = (long)PH * PW;
    const int nv = min(V, PW - x0);
    for (int c = 0; c < C; ++c, sp += splane, dp += dplane) {
        if (nv == V && aligned16(sp, dp)) {
            *(vt*)dp = *(const vt*)sp;
        } else {
            for (int j = 0; j < nv; ++j) dp[j] = sp[j];
        }
    }
}

// The tensor stitch: tiles [n, C, PH, PW] (PH = s P_h ..) -> out [1, C, FH, FW], a copy from the owner tile.  grid (FW / V / 256, FH); a thread copies V
// consecutive pixels of one output row in every channel: 16 bytes at a time where they have one owner and both addresses are aligned, else one by one, each
// from its own owner.  ay / ax are in output pixels.
template <typename T, int V>
__global__ void __launch_bounds__(256) k_stitch(const T* tiles, T* out, int C, int PH, int PW, int FH, int FW, int nw, Ax ay, Ax ax) {
    typedef T vt __attribute__((ext_vector_type(V)));
    const int X0 = (blockIdx.x * 256 + threadIdx.x) * V, Y = blockIdx.y;
    if (X0 >= FW) return;
    const int ky = owner_of(Y, ay), y = Y - origin_of(ky, ay);
    const long splane = (long)PH * PW, dplane = (long)FH * FW;
    const long row = ((long)ky * nw * C * PH + y) * PW;           // of tile (ky, 0); tile (ky, k) lies k * C * splane behind
    const int nv = min(V, FW - X0), kx = owner_of(X0, ax);
    T* dp = out + (long)Y * FW + X0;
    if (nv == V && owner_of(X0 + V - 1, ax) == kx) {
        const T* sp = tiles + row + (long)kx * C * splane + (X0 - origin_of(kx, ax));
        for (int c = 0; c < C; ++c, sp += splane, dp += dplane) {
            if (aligned16(sp, dp)) {
                *(vt*)dp = *(const vt*)sp;
            } else {
#pragma unroll
                for (int j = 0; j < V; ++j) dp[j] = sp[j];
            }
        }
    } else {
        for (int j = 0; j < nv; ++j) {
            const int k = owner_of(X0 + j, ax);
            const T* sp = tiles + row + (long)k * C * splane + (X0 + j - origin_of(k, ax));
            for (int c = 0; c < C; ++c) dp[c * dplane + j] = sp[c * splane];
        }
    }
}

// The uint8 gather: the tiles [count, C, PH, PW] of the virtual (H + 2 pad) x (W + 2 pad) image, every element read from img [H, W, C] through the border
// map -- k_extract_u8 of tiles_u8.hip on the rectangular lattice: the row map once per thread, load_run along the row, put_run's stores (np2tensor: /255,
// BGR(A) -> RGB(A), normalisation, cast).  grid (PW / V / 256, PH, count).  V = 4 needs PW % 4 == 0 (put_run's vector stores are then aligned), else V = 1.
template <typename TO, int C, int V>
__global__ void __launch_bounds__(256) k_gather_u8_rect(const uint8_t* img, TO* tiles, int H, int W, int pad, int mode, int PH, int PW, int nw, Ax ay, Ax ax,
                                                         int tile_begin, int normalize) {
    const int x = (blockIdx.x * 256 + threadIdx.x) * V, y = blockIdx.y;
    if (x >= PW) return;
    const int kk = blockIdx.z, k = kk + tile_begin, th = k / nw, tw = k - th * nw;
    Run<uint8_t, C * V, 1> p = {};
    const int sy = border_index(origin_of(th, ay) + y - pad, H, mode);
    if (sy >= 0) p = load_run<C, V>(img + (long)sy * W * C, origin_of(tw, ax) + x - pad, W, mode, false);
    put_run<TO, C, V, false>(p, tiles, kk, 0, (long)PH * PW, (long)y * PW + x, normalize, 0);
}

// The uint8 stitch: tiles [n, C, PH, PW] -> img [OH, OW, C] uint8 HWC BGR(A), output pixel (Yo, Xo) = pixel (Yo + cs, Xo + cs) of the stitched frame (cs =
// scale * crop: only the seamless window is read and stored), quantised by store_px (tensor2np: denormalise, flip, clip, round half to even).  grid
// (OW / 4 / 256, OH); a thread handles 4 consecutive pixels: per channel one 8-byte (fp16) / 16-byte (fp32) load where they have one owner and the address is
// aligned, else element by element, each from its own owner; the 4 C bytes leave in one store where that is aligned, else pixel by pixel.
template <typename TI, int C>
__global__ void __launch_bounds__(256) k_stitch_u8(const TI* tiles, uint8_t* img, int PH, int PW, int nw, Ax ay, Ax ax, int cs, int OW, int denormalize) {
    constexpr int V = 4, AV = C == 3 ? 4 : 4 * C;
    typedef TI vt __attribute__((ext_vector_type(V)));
    const int Xo = (blockIdx.x * 256 + threadIdx.x) * V, Yo = blockIdx.y;
    if (Xo >= OW) return;
    const int Y = Yo + cs, X0 = Xo + cs;
    const int ky = owner_of(Y, ay), y = Y - origin_of(ky, ay);
    const long plane = (long)PH * PW;
    const long row = ((long)ky * nw * C * PH + y) * PW;
    const int nv = min(V, OW - Xo), kx = owner_of(X0, ax);
    TI r[V][C];
    if (nv == V && owner_of(X0 + V - 1, ax) == kx) {
        const TI* sp = tiles + row + (long)kx * C * plane + (X0 - origin_of(kx, ax));
#pragma unroll
        for (int c = 0; c < C; ++c, sp += plane) {
            if (((uintptr_t)sp & (sizeof(vt) - 1)) == 0) {
                const vt v = *(const vt*)sp;
#pragma unroll
                for (int j = 0; j < V; ++j) r[j][c] = v[j];
            } else {
#pragma unroll
                for (int j = 0; j < V; ++j) r[j][c] = sp[j];
            }
        }
    } else {
#pragma unroll
        for (int j = 0; j < V; ++j) {
            if (j < nv) {
                const int k = owner_of(X0 + j, ax);
                const TI* sp = tiles + row + (long)k * C * plane + (X0 + j - origin_of(k, ax));
#pragma unroll
                for (int c = 0; c < C; ++c) r[j][c] = sp[c * plane];
            }
        }
    }
    uint8_t* dst = img + ((long)Yo * OW + Xo) * C;
    if (nv == V && ((uintptr_t)dst & (AV - 1)) == 0) {
        Run<uint8_t, C * V, AV> o;
#pragma unroll
        for (int j = 0; j < V; ++j) store_px<TI, C, false>(r[j], 0, -1, denormalize, &o.v[j * C]);
        *(Run<uint8_t, C * V, AV>*)dst = o;
    } else {
#pragma unroll
        for (int j = 0; j < V; ++j)
            if (j < nv) store_px<TI, C, false>(r[j], 0, -1, denormalize, dst + j * C);
    }
}

// the tile range of a gather; 0 or the error already set
inline int check_range(const char* who, int tile_begin, int tile_count, const Lattice& g) {
    if (tile_begin < 0 || tile_count < 0 || (long)tile_begin + tile_count > (long)g.y.n * g.x.n)
        return set_error(INNFER_ERR_INVALID, "%s: tile range [%d,+%d) outside %dx%d tiles", who, tile_begin, tile_count, g.y.n, g.x.n);
    return INNFER_OK;
}

}  // namespace
}  // namespace innfer

using namespace innfer;

extern "C" int innfer_tile_plan(int H, int W, int tile, int halo, int* ph, int* pw, int* nh, int* nw, int* ys, int* xs) {
    Lattice g;
    if (int rc = lattice("tile_plan", H, W, tile, halo, 1, &g)) return rc;
    if (ph) *ph = g.y.P;
    if (pw) *pw = g.x.P;
    if (nh) *nh = g.y.n;
    if (nw) *nw = g.x.n;
    const Ax ay = scaled(g.y, halo, 1), ax = scaled(g.x, halo, 1);
    if (ys) for (int i = 0; i < g.y.n; ++i) ys[i] = origin_of(i, ay);
    if (xs) for (int i = 0; i < g.x.n; ++i) xs[i] = origin_of(i, ax);
    return INNFER_OK;
}

extern "C" int innfer_tile_owner(int A, int tile, int halo, int scale, int X, int* index, int* origin) {
    Lattice g;
    if (int rc = lattice("tile_owner", A, A, tile, halo, scale, &g)) return rc;
    if (X < 0 || X >= scale * A || !index || !origin) return set_error(INNFER_ERR_INVALID, "tile_owner: position %d outside [0, %d) / null argument", X, scale * A);
    const Ax a = scaled(g.x, halo, scale);
    *index = owner_of(X, a);
    *origin = origin_of(*index, a);
    return INNFER_OK;
}

extern "C" int innfer_extract_tiles_rect(const void* d_img, int dtype, int C, int H, int W, int tile, int halo, int tile_begin, int tile_count,
                                         void* d_tiles, void* stream) {
    const char* who = "extract_tiles_rect";
    if (!d_img || !d_tiles || C <= 0) return set_error(INNFER_ERR_INVALID, "%s: null argument / C %d", who, C);
    Lattice g;
    if (int rc = lattice(who, H, W, tile, halo, 1, &g)) return rc;
    if (int rc = check_range(who, tile_begin, tile_count, g)) return rc;
    if (tile_count == 0) return INNFER_OK;
    if (!is_float_dtype(dtype)) return set_error(INNFER_ERR_INVALID, "%s: bad dtype %d", who, dtype);
    const int PH = g.y.P, PW = g.x.P;
    if (PH > 65535) return set_error(INNFER_ERR_UNSUPPORTED, "%s: %d tile rows exceed the launch grid", who, PH);
    const Ax ay = scaled(g.y, halo, 1), ax = scaled(g.x, halo, 1);
    const long tile_elems = (long)C * PH * PW;
    hipStream_t s = (hipStream_t)stream;
    for (long b = 0; b < tile_count; b += 65535) {              // tiles are the grid's z: at most 65535 per launch
        const unsigned nz = (unsigned)(tile_count - b < 65535 ? tile_count - b : 65535);
        with_dtype(dtype, [&](auto t) {
            using T = decltype(t);
            constexpr int V = 16 / sizeof(T);
            hipLaunchKernelGGL((k_gather_rect<T, V>), dim3(blocks(PW, 256 * V), PH, nz), dim3(256), 0, s, (const T*)d_img, (T*)d_tiles + b * tile_elems, C, H, W, PH,
                               PW, g.x.n, ay, ax, tile_begin + (int)b);
        });
    }
    INNFER_HIP(hipGetLastError());
    return INNFER_OK;
}

extern "C" int innfer_extract_tiles_u8_rect(const uint8_t* d_img, int C, int H, int W, int normalize, int tile, int halo, int tile_begin, int tile_count,
                                            int pad, int mode, void* d_tiles, int tile_dtype, void* stream) {
    const char* who = "extract_tiles_u8_rect";
    if (!d_img || !d_tiles) return set_error(INNFER_ERR_INVALID, "%s: null argument", who);
    if (C < 1 || C > 4) return set_error(INNFER_ERR_INVALID, "%s: %d channels (1 .. 4)", who, C);
    if (int rc = check_border(who, H, W, pad, mode)) return rc;
    Lattice g;
    if (int rc = lattice(who, H + 2 * pad, W + 2 * pad, tile, halo, 1, &g)) return rc;
    if (int rc = check_range(who, tile_begin, tile_count, g)) return rc;
    if (tile_count == 0) return INNFER_OK;
    if (!is_float_dtype(tile_dtype)) return set_error(INNFER_ERR_INVALID, "%s: bad dtype %d", who, tile_dtype);
    const int PH = g.y.P, PW = g.x.P;
    if (PH > 65535) return set_error(INNFER_ERR_UNSUPPORTED, "%s: %d tile rows exceed the launch grid", who, PH);
    const Ax ay = scaled(g.y, halo, 1), ax = scaled(g.x, halo, 1);
    const bool x4 = PW % 4 == 0;
    hipStream_t s = (hipStream_t)stream;
#define GA(V) hipLaunchKernelGGL((k_gather_u8_rect<TO, CC, V>), dim3(blocks(PW, 256 * V), PH, nz), dim3(256), 0, s, d_img, dst, H, W, pad, mode, PH, PW, g.x.n, ay, ax, \
                                 tile_begin + (int)b, normalize)
    for (long b = 0; b < tile_count; b += 65535) {
        const unsigned nz = (unsigned)(tile_count - b < 65535 ? tile_count - b : 65535);
        with_dtype(tile_dtype, [&](auto to) { with_form(false, C, [&](auto c, auto) {
            using TO = decltype(to);
            constexpr int CC = decltype(c)::value;
            TO* dst = (TO*)d_tiles + b * CC * PH * PW;
            if (x4) GA(4); else GA(1);
        }); });
    }
#undef GA
    INNFER_HIP(hipGetLastError());
    return INNFER_OK;
}

extern "C" int innfer_stitch_tiles(const void* d_tiles, int dtype, int n, int C, int height, int width, int tile, int halo, int scale, void* d_out, void* stream) {
    const char* who = "stitch_tiles";
    if (!d_tiles || !d_out || C <= 0) return set_error(INNFER_ERR_INVALID, "%s: null argument / C %d", who, C);
    Lattice g;
    if (int rc = lattice(who, height, width, tile, halo, scale, &g)) return rc;
    if (n != (long)g.y.n * g.x.n) return set_error(INNFER_ERR_INVALID, "%s: one image of %dx%d tiles expected, got %d tiles", who, g.y.n, g.x.n, n);
    if (!is_float_dtype(dtype)) return set_error(INNFER_ERR_INVALID, "%s: bad dtype %d", who, dtype);
    const int FH = scale * height, FW = scale * width;
    if (FH > 65535) return set_error(INNFER_ERR_UNSUPPORTED, "%s: %d output rows exceed the launch grid", who, FH);
    const Ax ay = scaled(g.y, halo, scale), ax = scaled(g.x, halo, scale);
    with_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        constexpr int V = 16 / sizeof(T);
        hipLaunchKernelGGL((k_stitch<T, V>), dim3(blocks(FW, 256 * V), FH), dim3(256), 0, (hipStream_t)stream, (const T*)d_tiles, (T*)d_out, C, scale * g.y.P,
                           scale * g.x.P, FH, FW, g.x.n, ay, ax);
    });
    INNFER_HIP(hipGetLastError());
    return INNFER_OK;
}

extern "C" int innfer_stitch_tiles_u8(const void* d_tiles, int dtype, int n, int C, int height, int width, int tile, int halo, int scale, int denormalize,
                                      int crop, uint8_t* d_img, void* stream) {
    const char* who = "stitch_tiles_u8";
    if (!d_tiles || !d_img) return set_error(INNFER_ERR_INVALID, "%s: null argument", who);
    if (C < 1 || C > 4) return set_error(INNFER_ERR_INVALID, "%s: %d channels (1 .. 4)", who, C);
    Lattice g;
    if (int rc = lattice(who, height, width, tile, halo, scale, &g)) return rc;
    if (crop < 0 || 2L * crop >= height || 2L * crop >= width) return set_error(INNFER_ERR_INVALID, "%s: crop %d leaves nothing of %dx%d", who, crop, height, width);
    if (n != (long)g.y.n * g.x.n) return set_error(INNFER_ERR_INVALID, "%s: one image of %dx%d tiles expected, got %d tiles", who, g.y.n, g.x.n, n);
    if (!is_float_dtype(dtype)) return set_error(INNFER_ERR_INVALID, "%s: bad dtype %d", who, dtype);
    const int cs = scale * crop, OH = scale * height - 2 * cs, OW = scale * width - 2 * cs;
    if (OH > 65535) return set_error(INNFER_ERR_UNSUPPORTED, "%s: %d output rows exceed the launch grid", who, OH);
    const Ax ay = scaled(g.y, halo, scale), ax = scaled(g.x, halo, scale);
    with_dtype(dtype, [&](auto ti) { with_form(false, C, [&](auto c, auto) {
        using TI = decltype(ti);
        hipLaunchKernelGGL((k_stitch_u8<TI, decltype(c)::value>), dim3(blocks(OW, 1024), OH), dim3(256), 0, (hipStream_t)stream, (const TI*)d_tiles, d_img,
                           scale * g.y.P, scale * g.x.P, g.x.n, ay, ax, cs, OW, denormalize);
    }); });
    INNFER_HIP(hipGetLastError());
    return INNFER_OK;
}
