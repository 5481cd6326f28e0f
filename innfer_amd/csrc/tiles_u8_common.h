// What the uint8 chop kernels of tiles_u8.hip and tiles_tta.hip share, each body once: the row-run load through the border map (load_run), the tile
// stores of the gather (put_run), the blend of one frame at one pixel (blend_at), the quantise-and-store tail (store_px), and on the host the dispatch
// from the runtime (fit, C, dtype) to the kernels' template arguments and the channel / alpha refusals (check_u8_form).  The stitched tile path
// (tiles_stitch.hip) builds its uint8 gather and stitch from load_run, put_run and store_px too, so its conversions are these.  A header of its own rather than
// a section of tiles_common.h because tiles.hip must NOT use any of it: its k_extract, k_recompose, k_u8_to_nchw and k_nchw_to_u8 are the independent
// anchors the tests hold these kernels to, and sharing a loop with them would make those tests compare code with itself.  Every rounding is explicit.
#pragma once
#include <type_traits>
#include "tiles_common.h"

namespace innfer {
namespace {

// channels of a tile (NT) and numerators per pixel (NC: colour + alpha results under FIT with an alpha plane) of the form <C, FIT>
template <int C, bool FIT> struct Form { static constexpr int NT = FIT ? 3 : C, NC = FIT && C > 1 ? 6 : NT; };

// The V pixels (C bytes each) at positions x0 .. x0 + V - 1 of an image row of W pixels, positions relative to the image and mapped by border_index;
// with `rev` delivered in descending order.  Where the run does not cross a fold of the map (source indices m0 .. m0 + 3) and its bytes are aligned it is
// one load, else one load per pixel through the map; 0 where the map says -1.  V = 4 or 1.
template <int C, int V>
__device__ __forceinline__ Run<uint8_t, C * V, 1> load_run(const uint8_t* row, int x0, int W, int mode, bool rev) {
    constexpr int AP = C == 3 ? 1 : C, AV = C == 3 ? 4 : 4 * C;
    Run<uint8_t, C * V, 1> p;
#pragma unroll
    for (int e = 0; e < C * V; ++e) p.v[e] = 0;
    const int m0 = border_index(x0, W, mode);
    bool run = false;
    if (V == 4) run = m0 >= 0 && border_index(x0 + 3, W, mode) == m0 + 3 && ((uintptr_t)(row + (long)m0 * C) & (AV - 1)) == 0;
    if (run) {
        const Run<uint8_t, C * V, AV> r = *(const Run<uint8_t, C * V, AV>*)(row + (long)m0 * C);
#pragma unroll
        for (int j = 0; j < V; ++j) {
#pragma unroll
            for (int c = 0; c < C; ++c) p.v[j * C + c] = rev ? r.v[(V - 1 - j) * C + c] : r.v[j * C + c];
        }
    } else {
#pragma unroll
        for (int j = 0; j < V; ++j) {
            const int jj = rev ? V - 1 - j : j;
            const int m = jj == 0 ? m0 : border_index(x0 + jj, W, mode);
            if (m >= 0) {
                const Run<uint8_t, C, AP> r = *(const Run<uint8_t, C, AP>*)(row + (long)m * C);
#pragma unroll
                for (int c = 0; c < C; ++c) p.v[j * C + c] = r.v[c];
            }
        }
    }
    return p;
}

// The tile stores of the gather for V pixels p (C bytes each, image order) at offset o of the colour slot `slot` and, FIT with alpha, the alpha slot
// `aslot`.  FIT false: channels flipped BGR(A) -> RGB(A) (np2tensor).  FIT true: (g, g, g) from gray, RGB from BGRA, the alpha tile (a, a, a).
template <typename TO, int C, int V, bool FIT>
__device__ __forceinline__ void put_run(const Run<uint8_t, C * V, 1>& p, TO* tiles, long slot, long aslot, long pp, long o, int normalize, int alpha) {
    typedef TO vo __attribute__((ext_vector_type(V)));
    if constexpr (FIT) {
        vo col[3], a;
#pragma unroll
        for (int j = 0; j < V; ++j) {
#pragma unroll
            for (int c = 0; c < 3; ++c)                             // RGB from BGR(A); (g, g, g) from gray
                col[c][j] = (TO)to_unit((float)p.v[j * C + (C == 4 ? 2 - c : 0)], 255.0f, normalize);
            if (C > 1) a[j] = (TO)to_unit((float)p.v[j * C + C - 1], 255.0f, normalize);
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) *(vo*)(tiles + (slot * 3 + c) * pp + o) = col[c];
        if (C > 1 && alpha) {
#pragma unroll
            for (int c = 0; c < 3; ++c) *(vo*)(tiles + (aslot * 3 + c) * pp + o) = a;
        }
    } else {
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const int sc = C == 3 ? 2 - c : (C == 4 && c < 3 ? 2 - c : c);      // np2tensor's flip: BGR -> RGB, BGRA -> RGBA
            vo v;
#pragma unroll
            for (int j = 0; j < V; ++j) v[j] = (TO)to_unit((float)p.v[j * C + sc], 255.0f, normalize);
            *(vo*)(tiles + (slot * C + c) * pp + o) = v;
        }
    }
}

// The blend of one A x B frame of na x nb tiles [.., NT, P, P] from `base` at pixel (Y, X): k_recompose of tiles.hip -- the tiles that cover the pixel in
// (h, w) order, each tile's weight computed once for all numerators, den summed alongside -- with the quotients rounded to TO into r[NC].  NC > NT: the
// alpha tiles lie aoff elements behind the colour tiles and fill r[3 .. 5] when `alpha` (else those are 0 / den).
template <typename TI, typename TO, int NT, int NC>
__device__ __forceinline__ void blend_at(const TI* base, long aoff, int alpha, int P, int A, int B, int na, int nb, int eff, int ov, int Y, int X, TO (&r)[NC]) {
    float num[NC], den = 0.f;
#pragma unroll
    for (int c = 0; c < NC; ++c) num[c] = 0.f;
    const long pp = (long)P * P;
    const int h0 = max(0, (Y - P + eff) / eff), w0 = max(0, (X - P + eff) / eff);
    for (int h = h0; h < na; ++h) {
        const int oy = min(h * eff, A - P);
        if (oy > Y) break;
        if (Y - oy >= P) continue;
        const float wy = profile(Y - oy, P, ov);
        for (int w = w0; w < nb; ++w) {
            const int ox = min(w * eff, B - P);
            if (ox > X) break;
            if (X - ox >= P) continue;
            const float wgt = __fmul_rn(profile(X - ox, P, ov), wy);
            den = __fadd_rn(den, wgt);
            const long k = (long)h * nb + w;
            const TI* tp = base + (k * NT * P + (Y - oy)) * (long)P + (X - ox);
#pragma unroll
            for (int c = 0; c < NT; ++c) num[c] = __fadd_rn(num[c], __fmul_rn((float)tp[c * pp], wgt));
            if constexpr (NC > NT) if (alpha) {
#pragma unroll
                for (int c = 0; c < 3; ++c) num[3 + c] = __fadd_rn(num[3 + c], __fmul_rn((float)tp[aoff + c * pp], wgt));
            }
        }
    }
#pragma unroll
    for (int c = 0; c < NC; ++c) r[c] = (TO)__fdiv_rn(num[c], den);
}

// The blend's tail, tensor2np as the store: r quantised to the pixel's C bytes at dst in one store.  FIT false: flipped RGB(A) -> BGR(A).  FIT true:
// B, G, R (C 4) or mean3 (gray) of the colour result, mean3 of the alpha result or the constant alpha `aconst`.
template <typename TO, int C, bool FIT>
__device__ __forceinline__ void store_px(const TO (&r)[Form<C, FIT>::NC], int alpha, int aconst, int denormalize, uint8_t* dst) {
    constexpr int NC = Form<C, FIT>::NC;
    Run<uint8_t, C, C == 3 ? 1 : C> o;
    if constexpr (FIT) {
        if (C == 4) {
#pragma unroll
            for (int c = 0; c < 3; ++c) o.v[2 - c] = (uint8_t)quantise((float)r[c], denormalize, 255.0f);
        } else {
            o.v[0] = (uint8_t)quantise((float)mean3(r[0], r[1], r[2]), denormalize, 255.0f);
        }
        if (C > 1) o.v[C - 1] = alpha ? (uint8_t)quantise((float)mean3(r[NC - 3], r[NC - 2], r[NC - 1]), denormalize, 255.0f) : (uint8_t)aconst;
    } else {
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const int sc = (C == 3 || (C == 4 && c < 3)) ? 2 - c : c;           // tensor2np's flip: RGB -> BGR, RGBA -> BGRA
            o.v[sc] = (uint8_t)quantise((float)r[c], denormalize, 255.0f);
        }
    }
    *(Run<uint8_t, C, C == 3 ? 1 : C>*)dst = o;
}

// ---- host: the runtime (dtype, fit, C) as template arguments.  f gets a value of the element type / integral_constants <C>, <FIT>; the caller has
// refused every other dtype and channel count (check_u8_form).
inline bool is_float_dtype(int dtype) { return dtype == INNFER_F16 || dtype == INNFER_F32; }
template <typename F> inline void with_dtype(int dtype, F&& f) {
    if (dtype == INNFER_F16) f(f16{}); else f(float{});
}
template <typename F> inline void with_form(bool fit, int C, F&& f) {
    using std::integral_constant;
    using std::bool_constant;
    if (C == 1) fit ? f(integral_constant<int, 1>{}, bool_constant<true>{}) : f(integral_constant<int, 1>{}, bool_constant<false>{});
    else if (C == 2) fit ? f(integral_constant<int, 2>{}, bool_constant<true>{}) : f(integral_constant<int, 2>{}, bool_constant<false>{});
    else if (C == 3) f(integral_constant<int, 3>{}, bool_constant<false>{});
    else fit ? f(integral_constant<int, 4>{}, bool_constant<true>{}) : f(integral_constant<int, 4>{}, bool_constant<false>{});
}

// The channel and alpha refusals of a gather (blend false: any C >= 1 -- what is built beyond 4 is the entry point's to say) or a blend (C 1 .. 4; alpha
// tiles only under fit with an alpha plane, else a constant alpha in [0, 255]); 0 or the error already set.
inline int check_u8_form(const char* who, bool fit, int C, int alpha, int alpha_const, bool blend) {
    if (fit ? (C != 1 && C != 2 && C != 4) : (C < 1 || (blend && C > 4)))
        return set_error(INNFER_ERR_INVALID, "%s: %d channels (%s)", who, C, fit ? "1, 2 or 4" : blend ? "1 .. 4" : "at least 1");
    if (blend && (fit ? (C == 1 ? alpha != 0 : (!alpha && (alpha_const < 0 || alpha_const > 255))) : alpha != 0))
        return set_error(INNFER_ERR_INVALID, "%s: a %d-channel image needs %s", who, C, !fit || C == 1 ? "no alpha tiles" : "alpha tiles or a constant alpha in [0, 255]");
    return INNFER_OK;
}

}  // namespace
}  // namespace innfer
