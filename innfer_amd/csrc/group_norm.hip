// GroupNorm over a 64-channel fp16 slab + the block's skip, PER SAMPLE: RealPLKSR's `norm(refine(..)) + x` (nn.GroupNorm(groups, 64): mean and biased variance over
// (64 / groups) x H x W of each image, eps inside the square root, per-channel affine).  Three launches:
//   gn_stats     a workgroup reads a segment of GN_SEG pixels x 32 channels ONCE (16-byte loads, 16 pixels x 8 channels per thread in registers) and writes one record
//                (count, mean, M2) per channel OCTET: the segment mean first, then the squared deviations from it -- the two-pass form on registers, as norm_stats.h.
//                Sums run in a fixed order (xor butterfly over the wave's 16 pixel lanes, the four waves in index order): deterministic, no atomics.
//   gn_finalize  one workgroup per (image, group): thread i merges records i, i + 256, .. with Chan's update (norm::chan_merge), thread 0 merges the 256 results in index
//                order; alpha[n][c] = gamma[c] / sqrt(M2 / count + eps), shift[n][c] = beta[c] - mean alpha[n][c] (norm::bn_write's transform).
//   gn_apply     out = fp16(fma(alpha[n][c], u, shift[n][c]) + skip): one fp32 fma, one fp32 add, one rounding.  Memory bound: 2 x 128 bytes in, 128 out per pixel.
// An octet never straddles two groups: groups in {1, 2, 4, 8}.
#include "common.h"
#include "norm_stats.h"

namespace innfer {

namespace {

constexpr int GN_SEG = 1024;

__global__ __launch_bounds__(256) void gn_stats_kernel(const f16* u, long gs, long HW, float* rec, int nseg) {
    __shared__ float red[4][4];
    const int sg = blockIdx.x, grp = blockIdx.y, n = blockIdx.z;
    const int t = threadIdx.x, q = t & 3, pl = t >> 2, wv = t >> 6, lane = t & 63;
    const long p0 = (long)sg * GN_SEG;
    const int cnt = (int)min((long)GN_SEG, HW - p0);
    const f16* base = u + grp * gs + ((long)n * HW + p0) * 32 + q * 8;
    f16x8 v[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int px = pl + 64 * i;
        if (px < cnt) v[i] = *(const f16x8*)(base + (long)px * 32);
        else
#pragma unroll
            for (int e = 0; e < 8; ++e) v[i][e] = (f16)0.f;
    }
    auto reduce = [&](float s) {                 // the octet's total over the workgroup, in every thread of the octet
#pragma unroll
        for (int m = 4; m < 64; m <<= 1) s += __shfl_xor(s, m);
        if (lane < 4) red[wv][q] = s;
        __syncthreads();
        const float tot = ((red[0][q] + red[1][q]) + red[2][q]) + red[3][q];
        __syncthreads();
        return tot;
    };
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        float a = 0.f;
#pragma unroll
        for (int e = 0; e < 8; ++e) a += (float)v[i][e];
        s += a;
    }
    const float count = 8.0f * (float)cnt;
    const float mu = reduce(s) / count;
    s = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        float a = 0.f;
#pragma unroll
        for (int e = 0; e < 8; ++e) { const float d = (float)v[i][e] - mu; a += d * d; }
        if (pl + 64 * i < cnt) s += a;
    }
    const float m2 = reduce(s);
    if (t < 4) {
        float* o = rec + ((((long)n * nseg + sg) * 8) + grp * 4 + q) * 3;
        o[0] = count; o[1] = mu; o[2] = m2;
    }
}

__global__ __launch_bounds__(256) void gn_finalize_kernel(const float* rec, int nseg, int groups, const float* gamma, const float* beta, float eps, float* alpha, float* shift) {
    __shared__ float sn[256], sm[256], sq[256];
    const int g = blockIdx.x, n = blockIdx.y, t = threadIdx.x;
    const int opg = 8 / groups, R = nseg * opg;
    float cnt = 0.f, mu = 0.f, m2 = 0.f;
    for (int r0 = t; r0 < R; r0 += 1024) {       // four records per trip, their loads issued together (one per trip is one exposed load latency per record: merge_group_parts)
        float v[4][3];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int r = min(r0 + 256 * j, R - 1);
            const int sg = r / opg, oi = r - sg * opg;
            const float* q = rec + ((((long)n * nseg + sg) * 8) + g * opg + oi) * 3;
            v[j][0] = r0 + 256 * j < R ? q[0] : 0.f; v[j][1] = q[1]; v[j][2] = q[2];          // (count 0: a no-op of chan_merge)
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) norm::chan_merge(cnt, mu, m2, v[j][0], v[j][1], v[j][2]);
    }
    sn[t] = cnt; sm[t] = mu; sq[t] = m2;
    __syncthreads();
    if (t == 0) {
        for (int i = 1; i < 256; ++i) norm::chan_merge(cnt, mu, m2, sn[i], sm[i], sq[i]);
        sm[0] = mu; sq[0] = 1.0f / sqrtf(m2 / cnt + eps);
    }
    __syncthreads();
    const int cpg = 8 * opg;
    if (t < cpg) {
        const int c = g * cpg + t;
        const float a = sq[0] * (gamma ? gamma[c] : 1.0f);
        alpha[n * 64 + c] = a;
        shift[n * 64 + c] = (beta ? beta[c] : 0.f) - sm[0] * a;
    }
}

__global__ __launch_bounds__(256) void gn_apply_kernel(const f16* u, long u_gs, const f16* skip, long skip_gs, f16* out, long out_gs, long NHW, long HW,
                                                       const float* alpha, const float* shift) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= NHW * 8) return;
    const int grp = (int)(i / (NHW * 4));
    const long rem = i - grp * NHW * 4;
    const long px = rem >> 2;
    const int q = (int)(rem & 3);
    const long n = px / HW;
    const long o = px * 32 + q * 8;
    const f16x8 x = *(const f16x8*)(u + grp * u_gs + o), k = *(const f16x8*)(skip + grp * skip_gs + o);
    const float* a = alpha + n * 64 + grp * 32 + q * 8;
    const float* b = shift + n * 64 + grp * 32 + q * 8;
    f16x8 y;
#pragma unroll
    for (int e = 0; e < 8; ++e) y[e] = (f16)(__builtin_fmaf(a[e], (float)x[e], b[e]) + (float)k[e]);
    *(f16x8*)(out + grp * out_gs + o) = y;
}

inline int gn_nseg(long HW) { return (int)((HW + GN_SEG - 1) / GN_SEG); }
inline size_t gn_rec_floats(int N, long HW) { return ((size_t)N * gn_nseg(HW) * 8 * 3 + 63) & ~(size_t)63; }

}  // namespace

size_t gn_work_floats(int N, long HW) { return gn_rec_floats(N, HW) + (size_t)N * 128; }

int gn_stats_launch(const f16* u, long u_gs, int N, long HW, float* work, hipStream_t s) {
    if (!u || !work || N <= 0 || N > 65535 || HW <= 0 || gn_nseg(HW) > 0x7fffff) return set_error(INNFER_ERR_INVALID, "group norm: null argument or N=%d HW=%ld", N, HW);
    GtScope gt(s, "group norm statistics (64-channel slab)", 3.0 * 64 * N * (double)HW, 128.0 * N * (double)HW);
    hipLaunchKernelGGL(gn_stats_kernel, dim3((unsigned)gn_nseg(HW), 2, (unsigned)N), dim3(256), 0, s, u, u_gs, HW, work, gn_nseg(HW));
    INNFER_HIP(hipGetLastError());
    return INNFER_OK;
}

int gn_finalize_launch(int N, long HW, int groups, const float* gamma, const float* beta, float eps, float* work, hipStream_t s) {
    if (!work || N <= 0 || N > 65535 || HW <= 0) return set_error(INNFER_ERR_INVALID, "group norm: null argument or N=%d HW=%ld", N, HW);
    if (groups != 1 && groups != 2 && groups != 4 && groups != 8) return set_error(INNFER_ERR_UNSUPPORTED, "group norm: %d groups of 64 channels (built: 1, 2, 4, 8)", groups);
    float* alpha = work + gn_rec_floats(N, HW);
    hipLaunchKernelGGL(gn_finalize_kernel, dim3((unsigned)groups, (unsigned)N), dim3(256), 0, s, (const float*)work, gn_nseg(HW), groups, gamma, beta, eps, alpha, alpha + (size_t)N * 64);
    INNFER_HIP(hipGetLastError());
    return INNFER_OK;
}

int gn_apply_launch(const f16* u, long u_gs, const f16* skip, long skip_gs, f16* out, long out_gs, int N, long HW, const float* work, hipStream_t s) {
    if (!u || !skip || !out || !work || N <= 0 || HW <= 0) return set_error(INNFER_ERR_INVALID, "group norm: null argument or N=%d HW=%ld", N, HW);
    const long NHW = (long)N * HW, nthr = NHW * 8;
    if ((nthr + 255) / 256 > 0x7fffffffL) return set_error(INNFER_ERR_UNSUPPORTED, "group norm: %ld pixels exceed the launch grid", NHW);
    const float* alpha = work + gn_rec_floats(N, HW);
    GtScope gt(s, "group norm apply + skip (64-channel slab)", 2.0 * 64 * (double)NHW, 384.0 * (double)NHW);
    hipLaunchKernelGGL(gn_apply_kernel, dim3((unsigned)((nthr + 255) / 256)), dim3(256), 0, s, u, u_gs, skip, skip_gs, out, out_gs, NHW, HW, alpha, alpha + (size_t)N * 64);
    INNFER_HIP(hipGetLastError());
    return INNFER_OK;
}

}  // namespace innfer
