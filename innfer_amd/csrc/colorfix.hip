// `-cf` colour fix on the GPU: replaces color_fix (utils/utils.py:278-315) with its srgb2linear /
// linear2srgb (utils/colors.py:29-60) ends.  The reference calls OpenCV twice (cv2.resize INTER_CUBIC and
// cv2.GaussianBlur 3x3, sigma 0); OpenCV is neither vendored nor installed here, so these kernels follow
// the published float32 algorithms (oracle/colorfix.py states them) and parity with OpenCV itself is
// UNPINNED.  All images are HWC, the two uint8 inputs and the uint8 output live on the device.
//   1. lin_b = srgb2linear(B) (kept: it is needed again at the end); diff = srgb2linear(A) - cubic(lin_b -> size A)
//   2. blur  = gauss3(diff)            rows, then columns, BORDER_REFLECT_101
//   3. out   = linear2srgb(cubic(blur -> size B) + lin_b)
// HBM-bound pointwise / gather work: one thread per output element, contraction off so that the float32
// operation order is the one written down (and mirrored by the oracle).
// Further down: the two fixes that are not the reference's (`-cf_mode wavelet | adain`, innfer_color_fix_mode), whose contract is utils.color_fix_np.
#include "common.h"

#pragma clang fp contract(off)

using namespace innfer;

namespace {

// The two transfer functions as written down (colors.py:29-60 on uint8 / on the float result)...
__device__ __forceinline__ float srgb2lin_eval(uint8_t v) {
    const float l = __fdiv_rn((float)v, 255.0f);
    return l <= 0.04045f ? __fdiv_rn(l, 12.92f) : powf(__fdiv_rn(__fadd_rn(l, 0.055f), 1.055f), 2.4f);
}

__device__ __forceinline__ uint8_t lin2srgb_eval(float x) {
    float s = fminf(fmaxf(x, 0.0f), 1.0f);
    s = s <= 0.0031308f ? __fmul_rn(s, 12.92f) : __fsub_rn(__fmul_rn(1.055f, powf(s, (float)(1.0 / 2.4))), 0.055f);
    s = fminf(fmaxf(__fmul_rn(s, 255.0f), 0.0f), 255.0f);
    return (uint8_t)(int)s;
}

// ... and as the image kernels apply them: both have only 256 outcomes, so the powf leaves the per-pixel path (it was what color_fix's time went to).
// g_s2l[v] = srgb2lin_eval(v); g_thr[k] = the smallest float in [0, 1] that lin2srgb_eval maps to a code >= k (k = 1 .. 255; found by bisection over
// the float bit patterns with lin2srgb_eval itself, once per device) -- linear2srgb(x) is then the number of thresholds <= clamp(x), eight compares.
__device__ float g_s2l[256];
__device__ float g_thr[256];

__global__ void k_build_tables() {
    const int k = threadIdx.x;
    g_s2l[k] = srgb2lin_eval((uint8_t)k);
    unsigned lo = 0u, hi = 0x3F800000u;                 // bit patterns of 0.0f and 1.0f: non-negative floats order like their bits
    if (k == 0) { g_thr[0] = 0.0f; return; }
    if (lin2srgb_eval(__uint_as_float(hi)) < k) { g_thr[k] = 2.0f; return; }       // (code 255 is reached at 1.0: never taken)
    while (lo < hi) {                                   // invariant: eval(hi) >= k
        const unsigned mid = lo + ((hi - lo) >> 1);
        if (lin2srgb_eval(__uint_as_float(mid)) >= k) hi = mid; else lo = mid + 1;
    }
    g_thr[k] = __uint_as_float(hi);
}

__device__ __forceinline__ float srgb2lin(uint8_t v) { return g_s2l[v]; }

// thr: the 256 thresholds in LDS
__device__ __forceinline__ uint8_t lin2srgb(float x, const float* thr) {
    const float s = fminf(fmaxf(x, 0.0f), 1.0f);
    int code = 0;
#pragma unroll
    for (int step = 128; step >= 1; step >>= 1) code += (thr[code + step] <= s) ? step : 0;
    return (uint8_t)code;
}

// OpenCV's cubic taps for destination index d: first source index (s - 1) and the four weights
__device__ __forceinline__ void cubic_taps(int d, float scale, int& s, float w[4]) {
    const float A = -0.75f;
    float f = ((float)d + 0.5f) * scale - 0.5f;
    const float fl = floorf(f);
    s = (int)fl;
    const float t = f - fl;
    w[0] = ((A * (t + 1.f) - 5.f * A) * (t + 1.f) + 8.f * A) * (t + 1.f) - 4.f * A;
    w[1] = ((A + 2.f) * t - (A + 3.f)) * t * t + 1.f;
    w[2] = ((A + 2.f) * (1.f - t) - (A + 3.f)) * (1.f - t) * (1.f - t) + 1.f;
    w[3] = 1.f - w[0] - w[1] - w[2];
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// horizontal pass, then vertical pass, as cv2.resize does for float images
// (SRC = uint8_t: the source is an sRGB image, linearised through the table as it is read)
__device__ __forceinline__ float cs_load(const float* p, long o) { return p[o]; }
__device__ __forceinline__ float cs_load(const uint8_t* p, long o) { return srgb2lin(p[o]); }
template <typename SRC>
__device__ __forceinline__ float cubic_sample(const SRC* src, int Hs, int Ws, int C, int c, int y, int x, float sy, float sx) {
    int x0, y0;
    float wx[4], wy[4];
    cubic_taps(x, sx, x0, wx);
    cubic_taps(y, sy, y0, wy);
    float acc = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const SRC* row = src + (long)clampi(y0 - 1 + j, 0, Hs - 1) * Ws * C + c;
        float r = 0.f;
#pragma unroll
        for (int i = 0; i < 4; ++i) r = r + cs_load(row, (long)clampi(x0 - 1 + i, 0, Ws - 1) * C) * wx[i];
        acc = acc + r * wy[j];
    }
    return acc;
}

__global__ void k_lin(const uint8_t* in, float* out, long n) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = srgb2lin(in[i]);
}

// diff = srgb2linear(A) - (scaling ? cubic(srgb2linear(B) -> A's size) : srgb2linear(B)); B is linearised through the table as it is read
__global__ void k_diff(const uint8_t* a, const uint8_t* b8, int hA, int wA, int hB, int wB, int C, int scaling, float* diff) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long)hA * wA * C) return;
    const int c = (int)(i % C), x = (int)((i / C) % wA), y = (int)(i / ((long)C * wA));
    const float b = scaling ? cubic_sample(b8, hB, wB, C, c, y, x, (float)hB / (float)hA, (float)wB / (float)wA) : srgb2lin(b8[i]);
    diff[i] = srgb2lin(a[i]) - b;
}

// one pass of the [0.25, 0.5, 0.25] filter along x (dir 0) or y (dir 1), BORDER_REFLECT_101
__global__ void k_gauss3(const float* in, int H, int W, int C, int dir, float* out) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long)H * W * C) return;
    const int c = (int)(i % C), x = (int)((i / C) % W), y = (int)(i / ((long)C * W));
    const int n = dir ? H : W, p = dir ? y : x;
    int lo = p - 1, hi = p + 1;
    if (lo < 0) lo = n > 1 ? 1 : 0;
    if (hi >= n) hi = n > 1 ? n - 2 : 0;
    const long step = dir ? (long)W * C : C;
    const float* base = in + i - (long)p * step;
    (void)c;
    out[i] = in[i] * 0.5f + (base[(long)lo * step] + base[(long)hi * step]) * 0.25f;
}

// out = linear2srgb((scaling ? cubic(blur -> B's size) : blur) + srgb2linear(B))
__global__ void k_finish(const float* blur, const uint8_t* b8, int hA, int wA, int hB, int wB, int C, int scaling, uint8_t* out) {
    __shared__ float thr[256];
    thr[threadIdx.x] = g_thr[threadIdx.x];
    __syncthreads();
    // one thread per pixel: the cubic taps and weights are the same for its C channels (same arithmetic per channel as cubic_sample)
    const long pix = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (pix >= (long)hB * wB) return;
    const int x = (int)(pix % wB), y = (int)(pix / wB);
    if (!scaling) {
        for (int c = 0; c < C; ++c) out[pix * C + c] = lin2srgb(blur[pix * C + c] + srgb2lin(b8[pix * C + c]), thr);
        return;
    }
    int x0, y0;
    float wx[4], wy[4];
    cubic_taps(x, (float)wA / (float)wB, x0, wx);
    cubic_taps(y, (float)hA / (float)hB, y0, wy);
    long ro[4]; int co[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) { ro[j] = (long)clampi(y0 - 1 + j, 0, hA - 1) * wA * C; co[j] = clampi(x0 - 1 + j, 0, wA - 1) * C; }
    for (int c = 0; c < C; ++c) {
        float acc = 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float r = 0.f;
#pragma unroll
            for (int i = 0; i < 4; ++i) r = r + blur[ro[j] + co[i] + c] * wx[i];
            acc = acc + r * wy[j];
        }
        out[pix * C + c] = lin2srgb(acc + srgb2lin(b8[pix * C + c]), thr);
    }
}

// linear_resize (utils.py:267-276): out = linear2srgb(cubic(srgb2linear(img) -> (oh, ow)))
__global__ void k_resize_finish(const float* lin, int h, int w, int C, int oh, int ow, uint8_t* out) {
    __shared__ float thr[256];
    thr[threadIdx.x] = g_thr[threadIdx.x];
    __syncthreads();
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long)oh * ow * C) return;
    const int c = (int)(i % C), x = (int)((i / C) % ow), y = (int)(i / ((long)C * ow));
    out[i] = lin2srgb(cubic_sample(lin, h, w, C, c, y, x, (float)h / (float)oh, (float)w / (float)ow), thr);
}

// ---------------------------------------------------------------- `-cf_mode wavelet` (utils.color_fix_np states the contract)
// out = quantise(B + B5(up(A) - B)): B5 = five a-trous levels (dilation 1, 2, 4, 8, 16) of the [0.25, 0.5, 0.25] filter along x, then along y, replicate
// border, in code units.  One workgroup owns a WV_T x WV_T core of the SR image and, per channel, the core plus a WV_HALO = 1 + 2 + 4 + 8 + 16 px halo,
// cut to the image: two fp32 ping-pong planes in LDS (2 x 126 x 126 x 4 = 127008 B, one workgroup per CU).  The difference is computed from the two uint8
// images as the plane is filled, the ten passes run in LDS, and the core is stored as uint8: no fp32 plane of SR size exists in global memory.
// The window is cut to the IMAGE, so a clamped index of a value the core depends on is the image's own replicate index; towards a neighbouring tile the
// window's edge values are wrong, but a value at distance >= 32 - 2^(i+1) from the core stops mattering after level i, which is also why level i's
// passes run on that shrunken rectangle only (30, 28, 24, 16, 0 px around the core; the x pass on 2^i more rows, which the y pass reads).
// Lanes run along x at pitch 1 in both passes: no bank conflicts.
constexpr int WV_T = 64, WV_HALO = 31, WV_R = WV_T + 2 * WV_HALO, WV_LEVELS = 5;
constexpr int WV_TX = 64, WV_TY = 16;                   // 1024 threads: 64 lanes along x, 16 rows
constexpr int WV_LDS = 2 * WV_R * WV_R * (int)sizeof(float);

// cubic_sample of the uint8 codes themselves (no transfer function): the same taps, weights and order
__device__ __forceinline__ float cubic_sample_u8(const uint8_t* src, int Hs, int Ws, int C, int c, int y, int x, float sy, float sx) {
    int x0, y0;
    float wx[4], wy[4];
    cubic_taps(x, sx, x0, wx);
    cubic_taps(y, sy, y0, wy);
    float acc = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const uint8_t* row = src + (long)clampi(y0 - 1 + j, 0, Hs - 1) * Ws * C + c;
        float r = 0.f;
#pragma unroll
        for (int i = 0; i < 4; ++i) r = r + (float)row[(long)clampi(x0 - 1 + i, 0, Ws - 1) * C] * wx[i];
        acc = acc + r * wy[j];
    }
    return acc;
}

__device__ __forceinline__ uint8_t quant_u8(float v) { return (uint8_t)(int)fminf(fmaxf(floorf(v + 0.5f), 0.0f), 255.0f); }

__global__ __launch_bounds__(WV_TX * WV_TY) void k_wavelet(const uint8_t* a, const uint8_t* b8, int hA, int wA, int hB, int wB, int C, int scaling,
                                                           int tiles_x, uint8_t* out) {
    extern __shared__ float wv_lds[];
    float* P = wv_lds;
    float* Q = wv_lds + WV_R * WV_R;
    const int lx = threadIdx.x, ly = threadIdx.y;
    const int cy0 = ((int)blockIdx.x / tiles_x) * WV_T, cx0 = ((int)blockIdx.x % tiles_x) * WV_T;      // the core, cut to the image
    const int cy1 = min(cy0 + WV_T, hB), cx1 = min(cx0 + WV_T, wB);
    const int ry0 = max(cy0 - WV_HALO, 0), rx0 = max(cx0 - WV_HALO, 0);                                // the loaded window, cut to the image
    const int ry1 = min(cy1 + WV_HALO, hB), rx1 = min(cx1 + WV_HALO, wB);
    const float sy = (float)hA / (float)hB, sx = (float)wA / (float)wB;
    for (int c = 0; c < C; ++c) {
        // cubic_sample_u8 is separable as written: r = 0 + s0 wx0 + .. + s3 wx3 per LR row, then acc = acc + r wy[j].  The LR rows the window's taps touch
        // are a_lo .. a_lo + a_n - 1 before the clamp (the first tap's row never decreases with y); where they fit into Q, their r go there once per
        // window column and every element takes its four from LDS -- the same operations on the same values, a quarter and less of the global reads.
        int a_lo = 0, a_n = WV_R + 1;
        if (scaling) {
            float w_[4];
            int s_hi;
            cubic_taps(ry0, sy, a_lo, w_);
            cubic_taps(ry1 - 1, sy, s_hi, w_);
            a_lo -= 1;
            a_n = s_hi + 2 - a_lo + 1;
        }
        if (scaling && a_n <= WV_R) {
            for (int x = rx0 + lx; x < rx1; x += WV_TX) {
                int x0;
                float wx[4];
                cubic_taps(x, sx, x0, wx);
                int co[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) co[i] = clampi(x0 - 1 + i, 0, wA - 1) * C + c;
                for (int jr = ly; jr < a_n; jr += WV_TY) {
                    const uint8_t* row = a + (long)clampi(a_lo + jr, 0, hA - 1) * wA * C;
                    float r = 0.f;
#pragma unroll
                    for (int i = 0; i < 4; ++i) r = r + (float)row[co[i]] * wx[i];
                    Q[jr * WV_R + (x - rx0)] = r;
                }
            }
            __syncthreads();
            for (int y = ry0 + ly; y < ry1; y += WV_TY) {
                int y0;
                float wy[4];
                cubic_taps(y, sy, y0, wy);
                const int qb = (y0 - 1 - a_lo) * WV_R - rx0;
                for (int x = rx0 + lx; x < rx1; x += WV_TX) {
                    float acc = 0.f;
#pragma unroll
                    for (int j = 0; j < 4; ++j) acc = acc + Q[qb + j * WV_R + x] * wy[j];
                    P[(y - ry0) * WV_R + (x - rx0)] = acc - (float)b8[((long)y * wB + x) * C + c];
                }
            }
        } else {
            for (int y = ry0 + ly; y < ry1; y += WV_TY)
                for (int x = rx0 + lx; x < rx1; x += WV_TX) {
                    const long o = ((long)y * wB + x) * C + c;
                    const float up = scaling ? cubic_sample_u8(a, hA, wA, C, c, y, x, sy, sx) : (float)a[o];
                    P[(y - ry0) * WV_R + (x - rx0)] = up - (float)b8[o];
                }
        }
        __syncthreads();
        for (int lv = 0; lv < WV_LEVELS; ++lv) {
            const int r = 1 << lv, rem = 32 - (2 << lv);
            const int x_lo = max(cx0 - rem, rx0), x_hi = min(cx1 + rem, rx1);
            int y_lo = max(cy0 - rem - r, ry0), y_hi = min(cy1 + rem + r, ry1);
            for (int y = y_lo + ly; y < y_hi; y += WV_TY) {                                            // along x: P -> Q
                const float* row = P + (y - ry0) * WV_R;
                for (int x = x_lo + lx; x < x_hi; x += WV_TX)
                    Q[(y - ry0) * WV_R + (x - rx0)] = row[x - rx0] * 0.5f + (row[max(x - r, rx0) - rx0] + row[min(x + r, rx1 - 1) - rx0]) * 0.25f;
            }
            __syncthreads();
            y_lo = max(cy0 - rem, ry0), y_hi = min(cy1 + rem, ry1);
            for (int y = y_lo + ly; y < y_hi; y += WV_TY) {                                            // along y: Q -> P
                const int yl = max(y - r, ry0) - ry0, yh = min(y + r, ry1 - 1) - ry0;
                for (int x = x_lo + lx; x < x_hi; x += WV_TX) {
                    const int xo = x - rx0;
                    P[(y - ry0) * WV_R + xo] = Q[(y - ry0) * WV_R + xo] * 0.5f + (Q[yl * WV_R + xo] + Q[yh * WV_R + xo]) * 0.25f;
                }
            }
            __syncthreads();
        }
        for (int y = cy0 + ly; y < cy1; y += WV_TY)
            for (int x = cx0 + lx; x < cx1; x += WV_TX) {
                const long o = ((long)y * wB + x) * C + c;
                out[o] = quant_u8((float)b8[o] + P[(y - ry0) * WV_R + (x - rx0)]);
            }
        __syncthreads();                                // the next channel refills P
    }
}

// ---------------------------------------------------------------- `-cf_mode adain`
// Workspace: 16 64-bit counters [image A | B][channel 0 .. 3][S1 | S2] (zeroed on the stream), then float g[4], o[4].
constexpr int AD_THREADS = 256;
constexpr size_t AD_WS = 16 * sizeof(unsigned long long) + 8 * sizeof(float);

__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_down(v, d, 64);
    return v;
}

// exact integer sums of x and x * x per channel: a thread walks pixels, a wave adds up by shuffles, a workgroup in LDS, one atomicAdd per counter and workgroup
__global__ __launch_bounds__(AD_THREADS) void k_adain_sums(const uint8_t* img, long npix, int C, unsigned long long* cnt) {
    __shared__ unsigned long long part[AD_THREADS / 64][8];
    unsigned long long s1[4] = {0, 0, 0, 0}, s2[4] = {0, 0, 0, 0};
    for (long p = (long)blockIdx.x * AD_THREADS + threadIdx.x; p < npix; p += (long)gridDim.x * AD_THREADS) {
#pragma unroll
        for (int c = 0; c < 4; ++c)
            if (c < C) {
                const unsigned v = img[p * C + c];
                s1[c] += v;
                s2[c] += v * v;
            }
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const unsigned long long t1 = wave_sum(s1[c]), t2 = wave_sum(s2[c]);
        if (lane == 0) { part[wave][2 * c] = t1; part[wave][2 * c + 1] = t2; }
    }
    __syncthreads();
    if (threadIdx.x < 2 * C) {
        unsigned long long t = 0;
        for (int w = 0; w < AD_THREADS / 64; ++w) t += part[w][threadIdx.x];
        atomicAdd(cnt + threadIdx.x, t);
    }
}

// sums -> gain and offset per channel, float64, in the order utils.color_fix_np writes down
__global__ void k_adain_params(const unsigned long long* cnt, double nA, double nB, int C, float* go) {
    const double eps = 1e-5 * 255 * 255;
    for (int c = 0; c < C; ++c) {
        const double mA = (double)cnt[2 * c] / nA, qA = (double)cnt[2 * c + 1] / nA;
        const double mB = (double)cnt[8 + 2 * c] / nB, qB = (double)cnt[8 + 2 * c + 1] / nB;
        const double vA = nA > 1 ? fmax(qA - mA * mA, 0.0) * (nA / (nA - 1)) : 0.0;
        const double vB = nB > 1 ? fmax(qB - mB * mB, 0.0) * (nB / (nB - 1)) : 0.0;
        const double g = sqrt(vA + eps) / sqrt(vB + eps);
        go[c] = (float)g;
        go[4 + c] = (float)(mA - mB * g);
    }
}

// four values per thread; vec: both pointers are 4-byte aligned, so a full group moves as one dword
__global__ __launch_bounds__(AD_THREADS) void k_adain_apply(const uint8_t* b8, long n, int C, const float* go, int vec, uint8_t* out) {
    const long i = ((long)blockIdx.x * AD_THREADS + threadIdx.x) * 4;
    if (i >= n) return;
    int c = (int)(i % C);
    if (vec && i + 4 <= n) {
        const uchar4 v = *reinterpret_cast<const uchar4*>(b8 + i);
        const uint8_t in[4] = {v.x, v.y, v.z, v.w};
        uint8_t o[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            o[j] = quant_u8((float)in[j] * go[c] + go[4 + c]);
            c = c + 1 == C ? 0 : c + 1;
        }
        *reinterpret_cast<uchar4*>(out + i) = make_uchar4(o[0], o[1], o[2], o[3]);
        return;
    }
    for (long k = i; k < n && k < i + 4; ++k) {
        out[k] = quant_u8((float)b8[k] * go[c] + go[4 + c]);
        c = c + 1 == C ? 0 : c + 1;
    }
}

// the tables are built once per device (the first call waits for them: later calls may come on other streams)
int ensure_tables(hipStream_t s) {
    static bool built[64] = {};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0) dev = 0;
    if (!built[dev & 63]) {
        hipLaunchKernelGGL(k_build_tables, dim3(1), dim3(256), 0, s);
        INNFER_HIP(hipGetLastError());
        INNFER_HIP(hipStreamSynchronize(s));
        built[dev & 63] = true;
    }
    return INNFER_OK;
}

inline unsigned nblk(long n) { return (unsigned)((n + 255) / 256); }
inline size_t al(size_t v) { return (v + 255) & ~(size_t)255; }

}  // namespace

extern "C" size_t innfer_color_fix_workspace_bytes(int hA, int wA, int hB, int wB, int C) {
    if (hA <= 0 || wA <= 0 || hB <= 0 || wB <= 0 || C <= 0) return 0;
    (void)hB; (void)wB;                                 // two fp32 planes of A's size (difference, blur); nothing of B's size is kept
    return 2 * al((size_t)hA * wA * C * 4);
}

extern "C" int innfer_linear_resize(const uint8_t* d_img, int h, int w, int C, uint8_t* d_out, int oh, int ow, void* d_ws, size_t ws_bytes, void* stream) {
    if (!d_img || !d_out || !d_ws || h <= 0 || w <= 0 || oh <= 0 || ow <= 0 || C <= 0 || C > 4) return set_error(INNFER_ERR_INVALID, "linear_resize: bad arguments");
    if (ws_bytes < (size_t)h * w * C * 4) return set_error(INNFER_ERR_WORKSPACE, "linear_resize: workspace %zu < %zu bytes", ws_bytes, (size_t)h * w * C * 4);
    hipStream_t s = (hipStream_t)stream;
    if (int rc = ensure_tables(s)) return rc;
    const long n = (long)h * w * C, no = (long)oh * ow * C;
    hipLaunchKernelGGL(k_lin, dim3(nblk(n)), dim3(256), 0, s, d_img, (float*)d_ws, n);
    hipLaunchKernelGGL(k_resize_finish, dim3(nblk(no)), dim3(256), 0, s, (const float*)d_ws, h, w, C, oh, ow, d_out);
    INNFER_HIP(hipGetLastError());
    return INNFER_OK;
}

extern "C" int innfer_color_fix(const uint8_t* d_a, int hA, int wA, const uint8_t* d_b, int hB, int wB, int C, uint8_t* d_out,
                                void* d_ws, size_t ws_bytes, void* stream) {
    if (!d_a || !d_b || !d_out || !d_ws) return set_error(INNFER_ERR_INVALID, "color_fix: null argument");
    if (hA <= 0 || wA <= 0 || hB <= 0 || wB <= 0 || C <= 0 || C > 4) return set_error(INNFER_ERR_INVALID, "color_fix: bad shape");
    const int scaling = hA < hB && wA < wB;
    if (!scaling && (hA != hB || wA != wB))
        return set_error(INNFER_ERR_INVALID, "color_fix: images of %dx%d and %dx%d cannot be subtracted (the reference raises too)", hA, wA, hB, wB);
    if (ws_bytes < innfer_color_fix_workspace_bytes(hA, wA, hB, wB, C))
        return set_error(INNFER_ERR_WORKSPACE, "color_fix: workspace too small");
    hipStream_t s = (hipStream_t)stream;
    if (int rc = ensure_tables(s)) return rc;
    const long nA = (long)hA * wA * C, nB = (long)hB * wB * C;
    float* t0 = (float*)d_ws;                          // (the linear copy of B the first version kept is gone: B is linearised through the table where it is read)
    float* t1 = (float*)((char*)t0 + al((size_t)nA * 4));
    (void)nB;
    hipLaunchKernelGGL(k_diff, dim3(nblk(nA)), dim3(256), 0, s, d_a, d_b, hA, wA, hB, wB, C, scaling, t0);
    hipLaunchKernelGGL(k_gauss3, dim3(nblk(nA)), dim3(256), 0, s, (const float*)t0, hA, wA, C, 0, t1);
    hipLaunchKernelGGL(k_gauss3, dim3(nblk(nA)), dim3(256), 0, s, (const float*)t1, hA, wA, C, 1, t0);
    hipLaunchKernelGGL(k_finish, dim3(nblk((long)hB * wB)), dim3(256), 0, s, (const float*)t0, d_b, hA, wA, hB, wB, C, scaling, d_out);
    INNFER_HIP(hipGetLastError());
    return INNFER_OK;
}

// `-cf_mode`: 0 lowfreq (innfer_color_fix), 1 wavelet, 2 adain
extern "C" size_t innfer_color_fix_mode_workspace_bytes(int mode, int hA, int wA, int hB, int wB, int C) {
    if (hA <= 0 || wA <= 0 || hB <= 0 || wB <= 0 || C <= 0) return 0;
    if (mode == 0) return innfer_color_fix_workspace_bytes(hA, wA, hB, wB, C);
    return mode == 2 ? AD_WS : 0;                       // wavelet: everything lives in LDS; adain: the counters, the gains and the offsets
}

extern "C" int innfer_color_fix_mode(int mode, const uint8_t* d_a, int hA, int wA, const uint8_t* d_b, int hB, int wB, int C, uint8_t* d_out,
                                     void* d_ws, size_t ws_bytes, void* stream) {
    if (mode == 0) return innfer_color_fix(d_a, hA, wA, d_b, hB, wB, C, d_out, d_ws, ws_bytes, stream);
    if (mode != 1 && mode != 2) return set_error(INNFER_ERR_INVALID, "color_fix: mode %d (0 lowfreq, 1 wavelet, 2 adain)", mode);
    if (!d_a || !d_b || !d_out) return set_error(INNFER_ERR_INVALID, "color_fix: null argument");
    if (hA <= 0 || wA <= 0 || hB <= 0 || wB <= 0 || C <= 0 || C > 4) return set_error(INNFER_ERR_INVALID, "color_fix: bad shape");
    const int scaling = hA < hB && wA < wB;
    if (!scaling && (hA != hB || wA != wB))
        return set_error(INNFER_ERR_INVALID, "color_fix: images of %dx%d and %dx%d cannot be subtracted (the reference raises too)", hA, wA, hB, wB);
    const size_t need = innfer_color_fix_mode_workspace_bytes(mode, hA, wA, hB, wB, C);
    if (need && (!d_ws || ws_bytes < need)) return set_error(INNFER_ERR_WORKSPACE, "color_fix: workspace %zu < %zu bytes", d_ws ? ws_bytes : (size_t)0, need);
    hipStream_t s = (hipStream_t)stream;
    if (mode == 1) {
        static std::atomic<unsigned long long> lds_set{0};
        INNFER_HIP(ensure_lds_attr(k_wavelet, WV_LDS, lds_set));
        const int tiles_x = (wB + WV_T - 1) / WV_T, tiles_y = (hB + WV_T - 1) / WV_T;
        if ((long)tiles_x * tiles_y > 0x7fffffffL) return set_error(INNFER_ERR_INVALID, "color_fix: image too large");
        hipLaunchKernelGGL(k_wavelet, dim3((unsigned)(tiles_x * tiles_y)), dim3(WV_TX, WV_TY), WV_LDS, s, d_a, d_b, hA, wA, hB, wB, C, scaling, tiles_x, d_out);
        INNFER_HIP(hipGetLastError());
        return INNFER_OK;
    }
    if (((uintptr_t)d_ws & 7) != 0) return set_error(INNFER_ERR_INVALID, "color_fix: the workspace must be 8-byte aligned");
    unsigned long long* cnt = (unsigned long long*)d_ws;
    float* go = (float*)(cnt + 16);
    const long pA = (long)hA * wA, pB = (long)hB * wB, nB = pB * C;
    INNFER_HIP(hipMemsetAsync(d_ws, 0, AD_WS, s));
    auto blocks = [](long npix) { return (unsigned)std::min<long>((npix + AD_THREADS - 1) / AD_THREADS, 2048); };
    hipLaunchKernelGGL(k_adain_sums, dim3(blocks(pA)), dim3(AD_THREADS), 0, s, d_a, pA, C, cnt);
    hipLaunchKernelGGL(k_adain_sums, dim3(blocks(pB)), dim3(AD_THREADS), 0, s, d_b, pB, C, cnt + 8);
    hipLaunchKernelGGL(k_adain_params, dim3(1), dim3(1), 0, s, (const unsigned long long*)cnt, (double)pA, (double)pB, C, go);
    const int vec = (((uintptr_t)d_b | (uintptr_t)d_out) & 3) == 0;
    hipLaunchKernelGGL(k_adain_apply, dim3((unsigned)((nB + 4L * AD_THREADS - 1) / (4L * AD_THREADS))), dim3(AD_THREADS), 0, s, d_b, nB, C, (const float*)go, vec, d_out);
    INNFER_HIP(hipGetLastError());
    return INNFER_OK;
}
