// The channel attention that ends HAT's conv block (CAB), PER SAMPLE, on a channel-padded fp16 slab z of N x HW pixels:
//   y[n][c] = sigmoid(W2 relu(W1 mean_pixels(z[n]) + b1) + b2)      (AdaptiveAvgPool2d(1), 1x1 conv C -> hid, ReLU, 1x1 conv hid -> C, Sigmoid)
//   t       = fp16(float(t) + conv_scale * y[n][c] * float(z))      (t already holds shortcut + proj of the block)
// Three launches:
//   ca_pool       a workgroup reads a segment of CA_SEG pixels x 32 channels ONCE (16-byte loads, 16 pixels x 8 channels per thread) and writes the segment's 32 channel sums.
//                 fp32, a fixed order (the thread's pixels in order, the xor butterfly over the wave's 16 pixel lanes, the four waves in index order): deterministic, no atomics.
//   ca_excite     one workgroup per sample: thread c merges channel c's segment sums in index order, the mean is the total times 1 / HW; thread j < hid the hidden unit j
//                 (fp32 fma over the channels in order, ReLU -- or, in the GELU form of DAT's channel_interaction, f (1 + erff(f / sqrt 2)) / 2); thread c the output (fma over the hidden units in order, 1 / (1 + exp(-x))).  y of a pad channel is 0.
//   ca_scale_add  per value fmaf(conv_scale * y[n][c], z, t) in fp32 and one fp16 rounding; in place on t.  Memory bound: 2 x 64 bytes in, 64 out per pixel and group.
// Nothing crosses samples: a batch's sample equals its own forward bit for bit.
#include "common.h"

namespace innfer {

namespace {

constexpr int CA_SEG = 1024;

__global__ __launch_bounds__(256) void ca_pool_kernel(const f16* z, long gs, long HW, float* part, int nseg, int c_pad) {
    __shared__ float red[4][32];
    const int sg = blockIdx.x, grp = blockIdx.y, n = blockIdx.z;
    const int t = threadIdx.x, q = t & 3, pl = t >> 2, wv = t >> 6, lane = t & 63;
    const long p0 = (long)sg * CA_SEG;
    const int cnt = (int)min((long)CA_SEG, HW - p0);
    const f16* base = z + grp * gs + ((long)n * HW + p0) * 32 + q * 8;
    float a[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) a[e] = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int px = pl + 64 * i;
        if (px < cnt) {
            const f16x8 v = *(const f16x8*)(base + (long)px * 32);
#pragma unroll
            for (int e = 0; e < 8; ++e) a[e] += (float)v[e];
        }
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) {
#pragma unroll
        for (int m = 4; m < 64; m <<= 1) a[e] += __shfl_xor(a[e], m);
        if (lane < 4) red[wv][q * 8 + e] = a[e];
    }
    __syncthreads();
    if (t < 32) part[((long)n * nseg + sg) * c_pad + grp * 32 + t] = ((red[0][t] + red[1][t]) + red[2][t]) + red[3][t];
}

template <bool GELU>
__global__ __launch_bounds__(256) void ca_excite_kernel(const float* part, int nseg, long HW, int C, int c_pad, int hid, const float* w1, const float* b1, const float* w2,
                                                        const float* b2, float* y, float* sums) {
    __shared__ float mean[256], hv[64];
    const int n = blockIdx.x, t = threadIdx.x;
    if (t < c_pad) {
        float s = 0.f;
        for (int sg = 0; sg < nseg; ++sg) s += part[((long)n * nseg + sg) * c_pad + t];
        if (sums) sums[(long)n * c_pad + t] = s;
        mean[t] = s * (1.0f / (float)HW);
    }
    __syncthreads();
    if (t < hid) {
        float s = b1[t];
        for (int c = 0; c < C; ++c) s = __builtin_fmaf(w1[t * C + c], mean[c], s);
        if constexpr (GELU) hv[t] = (0.5f * s) * (1.0f + erff(s * 0.70710678118654752440f));
        else hv[t] = fmaxf(s, 0.f);
    }
    __syncthreads();
    if (t < c_pad) {
        float r = 0.f;
        if (t < C) {
            float s = b2[t];
            for (int j = 0; j < hid; ++j) s = __builtin_fmaf(w2[t * hid + j], hv[j], s);
            r = 1.0f / (1.0f + expf(-s));
        }
        y[(long)n * c_pad + t] = r;
    }
}

__global__ __launch_bounds__(256) void ca_scale_add_kernel(f16* t, long t_gs, const f16* z, long z_gs, const float* y, float scale, long NHW, long HW, int c_pad) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= NHW * 4 * (c_pad / 32)) return;
    const int grp = (int)(i / (NHW * 4));
    const long rem = i - grp * NHW * 4;
    const long px = rem >> 2;
    const int q = (int)(rem & 3);
    const long n = px / HW;
    const long o = px * 32 + q * 8;
    const f16x8 a = *(const f16x8*)(t + grp * t_gs + o), b = *(const f16x8*)(z + grp * z_gs + o);
    const float* yc = y + n * c_pad + grp * 32 + q * 8;
    f16x8 r;
#pragma unroll
    for (int e = 0; e < 8; ++e) r[e] = (f16)__builtin_fmaf(scale * yc[e], (float)b[e], (float)a[e]);
    *(f16x8*)(t + grp * t_gs + o) = r;
}

inline int ca_nseg(long HW) { return (int)((HW + CA_SEG - 1) / CA_SEG); }

}  // namespace

// floats of the segment sums ca_pool writes and ca_excite merges
size_t ca_work_floats(int N, long HW, int c_pad) { return (size_t)N * ca_nseg(HW) * c_pad; }

static int ca_check(const char* what, int N, long HW, int c_pad) {
    if (N <= 0 || N > 65535 || HW <= 0 || ca_nseg(HW) > 0x7fffff) return set_error(INNFER_ERR_INVALID, "channel attention (%s): N=%d HW=%ld", what, N, HW);
    if (c_pad < 64 || c_pad > 256 || c_pad % 64) return set_error(INNFER_ERR_UNSUPPORTED, "channel attention (%s): a slab of %d channels (built: 64, 128, 192, 256)", what, c_pad);
    return INNFER_OK;
}

int ca_pool_launch(const f16* z, long z_gs, int N, long HW, int c_pad, float* work, hipStream_t s) {
    if (!z || !work) return set_error(INNFER_ERR_INVALID, "channel attention (pool): null argument");
    if (int rc = ca_check("pool", N, HW, c_pad)) return rc;
    if (z_gs < (long)N * HW * 32) return set_error(INNFER_ERR_INVALID, "channel attention (pool): a group stride below N * HW * 32");
    GtScope gt(s, "channel attention: per-sample channel sums", (double)c_pad * N * (double)HW, 2.0 * c_pad * N * (double)HW);
    hipLaunchKernelGGL(ca_pool_kernel, dim3((unsigned)ca_nseg(HW), (unsigned)(c_pad / 32), (unsigned)N), dim3(256), 0, s, z, z_gs, HW, work, ca_nseg(HW), c_pad);
    INNFER_HIP(hipGetLastError());
    return INNFER_OK;
}

// w1 [hid][C], b1 [hid], w2 [C][hid], b2 [C]: device floats; y: N x c_pad floats; sums (may be null): the merged channel sums, N x c_pad floats
template <bool GELU>
static int ca_excite_any(const float* work, int N, long HW, int C, int c_pad, int hid, const float* w1, const float* b1, const float* w2, const float* b2, float* y, float* sums,
                         hipStream_t s) {
    if (!work || !w1 || !b1 || !w2 || !b2 || !y) return set_error(INNFER_ERR_INVALID, "channel attention (excite): null argument");
    if (int rc = ca_check("excite", N, HW, c_pad)) return rc;
    if (C < 1 || C > c_pad || hid < 1 || hid > 64) return set_error(INNFER_ERR_UNSUPPORTED, "channel attention (excite): C=%d of %d, %d hidden channels (built: <= 64)", C, c_pad, hid);
    GtScope gt(s, "channel attention: squeeze / excite", 4.0 * C * hid * N, 4.0 * N * ((double)ca_nseg(HW) * c_pad + c_pad) + 8.0 * C * hid);
    hipLaunchKernelGGL(ca_excite_kernel<GELU>, dim3((unsigned)N), dim3(256), 0, s, work, ca_nseg(HW), HW, C, c_pad, hid, w1, b1, w2, b2, y, sums);
    INNFER_HIP(hipGetLastError());
    return INNFER_OK;
}

int ca_excite_launch(const float* work, int N, long HW, int C, int c_pad, int hid, const float* w1, const float* b1, const float* w2, const float* b2, float* y, float* sums,
                     hipStream_t s) {
    return ca_excite_any<false>(work, N, HW, C, c_pad, hid, w1, b1, w2, b2, y, sums, s);
}

// The same with the exact GELU, f (1 + erff(f / sqrt 2)) / 2, in place of the ReLU on the hidden units (DAT's channel_interaction, its BatchNorm folded into w1 / b1 at load)
int ca_excite_gelu_launch(const float* work, int N, long HW, int C, int c_pad, int hid, const float* w1, const float* b1, const float* w2, const float* b2, float* y,
                          float* sums, hipStream_t s) {
    return ca_excite_any<true>(work, N, HW, C, c_pad, hid, w1, b1, w2, b2, y, sums, s);
}

int ca_scale_add_launch(f16* t, long t_gs, const f16* z, long z_gs, const float* y, float scale, int N, long HW, int c_pad, hipStream_t s) {
    if (!t || !z || !y) return set_error(INNFER_ERR_INVALID, "channel attention (scale-add): null argument");
    if (int rc = ca_check("scale-add", N, HW, c_pad)) return rc;
    const long NHW = (long)N * HW, nthr = NHW * 4 * (c_pad / 32);
    if (t_gs < NHW * 32 || z_gs < NHW * 32) return set_error(INNFER_ERR_INVALID, "channel attention (scale-add): a group stride below N * HW * 32");
    if ((nthr + 255) / 256 > 0x7fffffffL) return set_error(INNFER_ERR_UNSUPPORTED, "channel attention (scale-add): %ld pixels exceed the launch grid", NHW);
    GtScope gt(s, "channel attention: scale-add", 2.0 * c_pad * (double)NHW, 6.0 * c_pad * (double)NHW);
    hipLaunchKernelGGL(ca_scale_add_kernel, dim3((unsigned)((nthr + 255) / 256)), dim3(256), 0, s, t, t_gs, z, z_gs, y, scale, NHW, HW, c_pad);
    INNFER_HIP(hipGetLastError());
    return INNFER_OK;
}

}  // namespace innfer
