// Antialiased separable resampler (ABI 118): the result of a network resampled to any final size before it leaves the device (`-outscale`).
//   - innfer_resample_taps / innfer_resample_plan (host only) build the per-axis tables in the Pillow / ATen antialias=True convention: for output i the
//     window [start, start + count) of source samples and its normalised weights, computed in float64 and rounded once to float32.
//   - innfer_resample_inthwc runs both passes on a uint8 / uint16 HWC image.  k_resample_fused is one launch with no global intermediate: a workgroup
//     owns TY x TX output pixels, runs the horizontal pass over the source rows its block needs into an LDS float32 image [R][TX][C] and the vertical
//     pass out of LDS.  Its plan rows live in LDS too (the horizontal ones transposed, [t][x], so that a wave reads consecutive words).  Where no block
//     fits the LDS budget (a 400x reduction needs thousands of rows) k_resample_h / k_resample_v do the same two passes through the caller's workspace.
// The arithmetic of a pass is ONE function (hpass / vpass) in both forms: acc = acc + w * x per tap in ascending order, the multiply and the add each
// rounded to float32 (no contraction), so the fused and the two-launch results are the same bytes and equal utils.resample_np.
// Indices read from the device plans are clamped (or wrapped by increment) before they address memory: a plan that does not belong to the sizes gives a
// wrong image, never an access outside the source, the workspace or LDS.
#include <cmath>

#include "common.h"

#pragma clang fp contract(off)

namespace innfer {
namespace {

constexpr int RS_THREADS = 512;
constexpr size_t RS_LDS_BUDGET = 64 * 1024;      // per workgroup: two workgroups (16 waves) per CU of 160 KiB, and no opt-in above the default dynamic limit
constexpr int RS_MAX_N = 1 << 28;                // 7 n (the widest wrapped lanczos window: -3.5 n .. 3.5 n) fits an int

// N elements in one load / store at alignment A bytes (a 3-channel pixel is three element accesses)
template <typename T, int N, int A> struct alignas(A) Run { T v[N]; };
template <typename T, int C> using Pixel = Run<T, C, C == 3 ? (int)sizeof(T) : (int)sizeof(T) * C>;

// ------------------------------------------------------------------------------------------------ host: the tables
constexpr double kPi = 3.14159265358979323846;

double filter_support(int f) { return f == INNFER_RESAMPLE_BOX ? 0.5 : f == INNFER_RESAMPLE_BILINEAR ? 1.0 : f == INNFER_RESAMPLE_BICUBIC ? 2.0 : 3.0; }

double sinc(double x) { return x == 0.0 ? 1.0 : std::sin(kPi * x) / (kPi * x); }

double filter_value(int f, double x) {
    switch (f) {
    case INNFER_RESAMPLE_BOX: return x > -0.5 && x <= 0.5 ? 1.0 : 0.0;
    case INNFER_RESAMPLE_BILINEAR: x = std::fabs(x); return x < 1.0 ? 1.0 - x : 0.0;
    case INNFER_RESAMPLE_BICUBIC: {                                     // Keys, a = -0.5
        const double a = -0.5;
        x = std::fabs(x);
        if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1.0;
        if (x < 2.0) return (((x - 5.0) * x + 8.0) * x - 4.0) * a;
        return 0.0;
    }
    default: return x >= -3.0 && x < 3.0 ? sinc(x) * sinc(x / 3.0) : 0.0;
    }
}

struct Axis { double scale, fs, support; };

Axis axis_of(int n_in, int n_out, int f) {
    Axis a;
    a.scale = (double)n_in / (double)n_out;
    a.fs = a.scale > 1.0 ? a.scale : 1.0;
    a.support = filter_support(f) * a.fs;
    return a;
}

// the window [lo, hi) of output i and its centre
void window(const Axis& a, int n_in, int i, int wrap, int* lo, int* hi, double* c) {
    *c = (i + 0.5) * a.scale;
    long l = (long)std::floor(*c - a.support + 0.5), h = (long)std::floor(*c + a.support + 0.5);
    if (!wrap) {
        if (l < 0) l = 0;
        if (h > n_in) h = n_in;
    }
    *lo = (int)l;
    *hi = (int)h;
}

int check_axis(const char* who, int n_in, int n_out, int f) {
    if (n_in < 1 || n_out < 1 || n_in > RS_MAX_N || n_out > RS_MAX_N) return set_error(INNFER_ERR_INVALID, "%s: bad sizes n_in=%d n_out=%d (1 .. 2^28)", who, n_in, n_out);
    if (f < INNFER_RESAMPLE_BOX || f > INNFER_RESAMPLE_LANCZOS) return set_error(INNFER_ERR_INVALID, "%s: filter %d (0 box, 1 bilinear, 2 bicubic, 3 lanczos)", who, f);
    return INNFER_OK;
}

// ------------------------------------------------------------------------------------------------ host: the block of the fused kernel
// The LDS budget rule.  A block of TY output rows needs at most R = Tv + ceil((TY - 1) h / oh) + 1 source rows (a window is at most Tv rows, the window
// starts of rows y and y + k are at most ceil(k h / oh) apart; + 1 for the rounding of the float64 centres), and its LDS holds the float32 image
// [R][TX][C], the horizontal plan rows [Th][TX], the vertical ones [TY][Tv] and the starts / counts.  The largest TX x TY (TX 64 .. 16, TY 32 .. 1) that
// fits RS_LDS_BUDGET is taken; none: the two-launch form.
struct Tile { int TX, TY, R; size_t lds; };

Tile pick_tile(int h, int C, int oh, int ow, int Th, int Tv) {
    Tile best = {0, 0, 0, 0};
    for (int TX = ow > 32 ? 64 : ow > 16 ? 32 : 16; TX >= 16; TX >>= 1)
        for (int TY = 32; TY >= 1; TY >>= 1) {
            if (TY > 1 && TY / 2 >= oh) continue;                     // no taller than the image needs
            const long R = (long)Tv + ((long)(TY - 1) * h + oh - 1) / oh + 1;
            const size_t lds = 4 * ((size_t)R * TX * C + (size_t)Th * TX + (size_t)TY * Tv + 2 * (size_t)TX + 2 * (size_t)TY);
            if (lds <= RS_LDS_BUDGET && TX * TY > best.TX * best.TY) best = {TX, TY, (int)R, lds};
        }
    return best;
}

// ------------------------------------------------------------------------------------------------ device: the two passes
__device__ __forceinline__ int pmod(int i, int n) {
    const int r = i % n;
    return r < 0 ? r + n : r;
}

__device__ __forceinline__ int clampi(int i, int lo, int hi) { return i < lo ? lo : i > hi ? hi : i; }

// One pixel of the horizontal pass: source row `row` (w pixels), window [start, start + count), weights wt(t).
template <typename T, int C, typename W>
__device__ __forceinline__ void hpass(const T* __restrict__ row, int w, int start, int count, int wrap, W wt, float (&acc)[C]) {
#pragma unroll
    for (int c = 0; c < C; ++c) acc[c] = 0.0f;
    int col = wrap ? pmod(start, w) : start;
    for (int t = 0; t < count; ++t) {
        const int sc = wrap ? col : clampi(col, 0, w - 1);
        const Pixel<T, C> p = *(const Pixel<T, C>*)(row + (size_t)sc * C);
        const float wgt = wt(t);
#pragma unroll
        for (int c = 0; c < C; ++c) acc[c] = __fadd_rn(acc[c], __fmul_rn(wgt, (float)p.v[c]));
        if (++col == w && wrap) col = 0;
    }
}

// One pixel of the vertical pass: px(t) points at the C floats of the intermediate at tap t.
template <int C, typename P, typename W>
__device__ __forceinline__ void vpass(int count, P px, W wt, float (&acc)[C]) {
#pragma unroll
    for (int c = 0; c < C; ++c) acc[c] = 0.0f;
    for (int t = 0; t < count; ++t) {
        const float* p = px(t);
        const float wgt = wt(t);
#pragma unroll
        for (int c = 0; c < C; ++c) acc[c] = __fadd_rn(acc[c], __fmul_rn(wgt, p[c]));
    }
}

template <typename T, int C>
__device__ __forceinline__ void store_pixel(T* dst, const float (&acc)[C]) {
    constexpr float maxval = sizeof(T) == 1 ? 255.0f : 65535.0f;
    Pixel<T, C> o;
#pragma unroll
    for (int c = 0; c < C; ++c) o.v[c] = (T)fminf(fmaxf(floorf(__fadd_rn(acc[c], 0.5f)), 0.0f), maxval);
    *(Pixel<T, C>*)dst = o;
}

template <typename T, int C>
__global__ void __launch_bounds__(RS_THREADS) k_resample_fused(const T* __restrict__ src, T* __restrict__ dst, int h, int w, int oh, int ow,
        const int* __restrict__ hs, const int* __restrict__ hc, const float* __restrict__ hw, int Th,
        const int* __restrict__ vs, const int* __restrict__ vc, const float* __restrict__ vw, int Tv, int wrap, int lTX, int TY, int Rcap, int nby) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int TX = 1 << lTX, tid = threadIdx.x;
    float* s_img = (float*)smem;                                  // [Rcap][TX][C]
    float* s_wh = s_img + (size_t)Rcap * TX * C;                  // [Th][TX]
    float* s_wv = s_wh + (size_t)Th * TX;                         // [TY][Tv]
    int* s_hs = (int*)(s_wv + (size_t)TY * Tv);                   // [TX] starts, [TX] counts, [TY] starts, [TY] counts
    int* s_hc = s_hs + TX;
    int* s_vs = s_hc + TX;
    int* s_vc = s_vs + TY;
    const int x0 = blockIdx.x * TX, nx = min(TX, ow - x0);
    for (int i = tid; i < nx * Th; i += RS_THREADS) {
        const int x = i / Th, t = i - x * Th;
        s_wh[t * TX + x] = hw[(size_t)(x0 + x) * Th + t];
    }
    for (int x = tid; x < nx; x += RS_THREADS) {
        s_hs[x] = hs[x0 + x];
        s_hc[x] = clampi(hc[x0 + x], 0, Th);
    }
    for (int by = blockIdx.y; by < nby; by += gridDim.y) {
        const int y0 = by * TY, ny = min(TY, oh - y0);
        __syncthreads();                                          // the previous block's vertical pass has read its tables
        for (int i = tid; i < ny * Tv; i += RS_THREADS) s_wv[i] = vw[(size_t)y0 * Tv + i];
        for (int y = tid; y < ny; y += RS_THREADS) {
            s_vs[y] = vs[y0 + y];
            s_vc[y] = clampi(vc[y0 + y], 0, Tv);
        }
        __syncthreads();
        const int rlo = s_vs[0], R = clampi(s_vs[ny - 1] + s_vc[ny - 1] - rlo, 0, Rcap);
        for (int item = tid; item < (R << lTX); item += RS_THREADS) {
            const int r = item >> lTX, x = item & (TX - 1);
            if (x >= nx) continue;
            const int sr = wrap ? pmod(rlo + r, h) : clampi(rlo + r, 0, h - 1);
            float acc[C];
            hpass<T, C>(src + (size_t)sr * w * C, w, s_hs[x], s_hc[x], wrap, [&](int t) { return s_wh[t * TX + x]; }, acc);
            float* o = s_img + item * C;
#pragma unroll
            for (int c = 0; c < C; ++c) o[c] = acc[c];
        }
        __syncthreads();
        for (int item = tid; item < (ny << lTX); item += RS_THREADS) {
            const int y = item >> lTX, x = item & (TX - 1);
            if (x >= nx) continue;
            const int off = s_vs[y] - rlo;
            const float* wrow = s_wv + y * Tv;
            float acc[C];
            vpass<C>(s_vc[y], [&](int t) { return s_img + (clampi(off + t, 0, Rcap - 1) * TX + x) * C; }, [&](int t) { return wrow[t]; }, acc);
            store_pixel<T, C>(dst + ((size_t)(y0 + y) * ow + (x0 + x)) * C, acc);
        }
    }
}

// the two-launch form: the float32 intermediate [h][ow][C] in the caller's workspace
template <typename T, int C>
__global__ void __launch_bounds__(256) k_resample_h(const T* __restrict__ src, float* __restrict__ ws, int h, int w, int ow,
        const int* __restrict__ hs, const int* __restrict__ hc, const float* __restrict__ hw, int Th, int wrap) {
    const int X = blockIdx.x * 256 + threadIdx.x;
    if (X >= ow) return;
    const int start = hs[X], count = clampi(hc[X], 0, Th);
    const float* wrow = hw + (size_t)X * Th;
    for (int row = blockIdx.y; row < h; row += gridDim.y) {
        float acc[C];
        hpass<T, C>(src + (size_t)row * w * C, w, start, count, wrap, [&](int t) { return wrow[t]; }, acc);
        float* o = ws + ((size_t)row * ow + X) * C;
#pragma unroll
        for (int c = 0; c < C; ++c) o[c] = acc[c];
    }
}

template <typename T, int C>
__global__ void __launch_bounds__(256) k_resample_v(const float* __restrict__ ws, T* __restrict__ dst, int h, int oh, int ow,
        const int* __restrict__ vs, const int* __restrict__ vc, const float* __restrict__ vw, int Tv, int wrap) {
    const int X = blockIdx.x * 256 + threadIdx.x;
    if (X >= ow) return;
    for (int y = blockIdx.y; y < oh; y += gridDim.y) {
        const int start = vs[y], count = clampi(vc[y], 0, Tv);
        const float* wrow = vw + (size_t)y * Tv;
        int row = wrap ? pmod(start, h) : start;
        float acc[C];
        vpass<C>(count, [&](int) {
            const int sr = wrap ? row : clampi(row, 0, h - 1);
            if (++row == h && wrap) row = 0;
            return ws + ((size_t)sr * ow + X) * C;
        }, [&](int t) { return wrow[t]; }, acc);
        store_pixel<T, C>(dst + ((size_t)y * ow + X) * C, acc);
    }
}

int check_image(const char* who, int h, int w, int C, int oh, int ow, int Th, int Tv) {
    if (C < 1 || C > 4) return set_error(INNFER_ERR_INVALID, "%s: %d channels (1 .. 4)", who, C);
    if (h < 1 || w < 1 || oh < 1 || ow < 1 || h > RS_MAX_N || w > RS_MAX_N || oh > RS_MAX_N || ow > RS_MAX_N)
        return set_error(INNFER_ERR_INVALID, "%s: bad sizes %dx%d -> %dx%d (1 .. 2^28 each)", who, h, w, oh, ow);
    if (Th < 1 || Tv < 1) return set_error(INNFER_ERR_INVALID, "%s: plan widths Th=%d Tv=%d (innfer_resample_taps)", who, Th, Tv);
    return INNFER_OK;
}

}  // namespace
}  // namespace innfer

using namespace innfer;

extern "C" int innfer_resample_taps(int n_in, int n_out, int filter) {
    if (check_axis("resample_taps", n_in, n_out, filter)) return INNFER_ERR_INVALID;
    const Axis a = axis_of(n_in, n_out, filter);
    int T = 0;
    for (int i = 0; i < n_out; ++i) {
        int lo, hi;
        double c;
        window(a, n_in, i, 1, &lo, &hi, &c);                // the wrapped window contains the truncated one
        if (hi - lo > T) T = hi - lo;
    }
    return T;
}

extern "C" int innfer_resample_plan(int n_in, int n_out, int filter, int wrap, int* start, int* count, float* weights, int T) {
    if (int rc = check_axis("resample_plan", n_in, n_out, filter)) return rc;
    if (!start || !count || !weights) return set_error(INNFER_ERR_INVALID, "resample_plan: null argument");
    const int need = innfer_resample_taps(n_in, n_out, filter);
    if (T < need) return set_error(INNFER_ERR_INVALID, "resample_plan: T=%d, the widest window has %d taps (innfer_resample_taps)", T, need);
    const Axis a = axis_of(n_in, n_out, filter);
    std::vector<double> wd((size_t)need);
    for (int i = 0; i < n_out; ++i) {
        int lo, hi;
        double c;
        window(a, n_in, i, wrap != 0, &lo, &hi, &c);
        double sum = 0.0;
        for (int j = lo; j < hi; ++j) {
            wd[j - lo] = filter_value(filter, (j - c + 0.5) / a.fs);
            sum += wd[j - lo];
        }
        float* row = weights + (size_t)i * T;
        for (int t = 0; t < T; ++t) row[t] = t < hi - lo ? (float)(sum != 0.0 ? wd[t] / sum : wd[t]) : 0.0f;
        start[i] = lo;
        count[i] = hi - lo;
    }
    return INNFER_OK;
}

extern "C" size_t innfer_resample_workspace_bytes(int h, int w, int C, int oh, int ow, int Th, int Tv) {
    if (check_image("resample_workspace_bytes", h, w, C, oh, ow, Th, Tv)) return 0;
    return pick_tile(h, C, oh, ow, Th, Tv).TX ? 0 : (size_t)h * ow * C * sizeof(float);
}

extern "C" int innfer_resample_inthwc(const void* d_src, int bits, int h, int w, int C, void* d_dst, int oh, int ow,
                                      const int* d_hstart, const int* d_hcount, const float* d_hweights, int Th,
                                      const int* d_vstart, const int* d_vcount, const float* d_vweights, int Tv,
                                      int wrap, void* d_workspace, size_t workspace_bytes, void* stream) {
    if (bits != 8 && bits != 16) return set_error(INNFER_ERR_INVALID, "resample_inthwc: bits %d (8, 16)", bits);
    if (int rc = check_image("resample_inthwc", h, w, C, oh, ow, Th, Tv)) return rc;
    if (!d_src || !d_dst || !d_hstart || !d_hcount || !d_hweights || !d_vstart || !d_vcount || !d_vweights)
        return set_error(INNFER_ERR_INVALID, "resample_inthwc: null argument");
    const Tile tile = pick_tile(h, C, oh, ow, Th, Tv);
    const size_t need = tile.TX ? 0 : (size_t)h * ow * C * sizeof(float);
    if (need && (!d_workspace || workspace_bytes < need))
        return set_error(INNFER_ERR_WORKSPACE, "resample_inthwc: workspace %zu < %zu bytes (innfer_resample_workspace_bytes)", workspace_bytes, need);
    hipStream_t s = (hipStream_t)stream;
    wrap = wrap != 0;
    GtScope gt(s, "resample", 2.0 * C * ((double)h * ow * Th + (double)oh * ow * Tv), (double)(bits / 8) * C * ((double)h * w + (double)oh * ow));
    if (tile.TX) {
        const int lTX = tile.TX == 64 ? 6 : tile.TX == 32 ? 5 : 4, nby = (oh + tile.TY - 1) / tile.TY;
        const dim3 g((ow + tile.TX - 1) / tile.TX, nby < 65535 ? nby : 65535), b(RS_THREADS);
#define FUSED(T, CC) hipLaunchKernelGGL((k_resample_fused<T, CC>), g, b, tile.lds, s, (const T*)d_src, (T*)d_dst, h, w, oh, ow, d_hstart, d_hcount, d_hweights, Th, \
                                        d_vstart, d_vcount, d_vweights, Tv, wrap, lTX, tile.TY, tile.R, nby)
#define FUSED_T(T) do { if (C == 1) FUSED(T, 1); else if (C == 2) FUSED(T, 2); else if (C == 3) FUSED(T, 3); else FUSED(T, 4); } while (0)
        if (bits == 8) FUSED_T(uint8_t); else FUSED_T(uint16_t);
#undef FUSED_T
#undef FUSED
        INNFER_HIP(hipGetLastError());
        return INNFER_OK;
    }
    float* ws = (float*)d_workspace;
    const dim3 b(256), gh((ow + 255) / 256, h < 65535 ? h : 65535), gv((ow + 255) / 256, oh < 65535 ? oh : 65535);
#define TWO(T, CC) do { hipLaunchKernelGGL((k_resample_h<T, CC>), gh, b, 0, s, (const T*)d_src, ws, h, w, ow, d_hstart, d_hcount, d_hweights, Th, wrap); \
                        hipLaunchKernelGGL((k_resample_v<T, CC>), gv, b, 0, s, (const float*)ws, (T*)d_dst, h, oh, ow, d_vstart, d_vcount, d_vweights, Tv, wrap); } while (0)
#define TWO_T(T) do { if (C == 1) TWO(T, 1); else if (C == 2) TWO(T, 2); else if (C == 3) TWO(T, 3); else TWO(T, 4); } while (0)
    if (bits == 8) TWO_T(uint8_t); else TWO_T(uint16_t);
#undef TWO_T
#undef TWO
    INNFER_HIP(hipGetLastError());
    return INNFER_OK;
}
