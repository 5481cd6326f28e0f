// Attention ACROSS channels over all pixels of one sample (DAT's adaptive channel attention), per head, on the head-padded qkv slab of win_attn.hip (3 nH groups of 32
// channels on N x HW pixels; q and k as the Linear left them -- no scale):
//   G[x][y] = sum_n q[n][x] k[n][y],  sq[x] = sum_n q[n][x]^2,  sk[y] = sum_n k[n][y]^2
//   A[x][y] = softmax_y( (G[x][y] (rq[x] rk[y])) temperature_h ),  r = 1 / max(sqrtf(s), 1e-12)          (F.normalize over the pixels, then q k^T times temperature)
//   a[n][x] = sum_y A[x][y] v[n][y]
// Three launches, plain fp32 FMAs: the pass is memory-bound (64 bytes of q and k per pixel and head against 1024 FMAs), and the scalar form has an order of summation
// that is easy to state and to model; the matrix cores would save nothing that shows.
//   csa_gram      a workgroup owns a segment of CSA_SEG pixels of one (sample, head); it stages 64 pixels of q and k at a time in LDS as fp32 (channels >= d as ZEROS:
//                 whatever the slab's pad channels hold is inert) and thread (x, y quad) adds its four products pixel by pixel: acc = fma(q[n][x], k[n][y], acc), the
//                 segment's pixels in order.  Threads 0 .. 31 / 32 .. 63 do the same for sq / sk.  One record of 32 x 32 + 32 + 32 floats per segment: no atomics.
//   csa_softmax   one workgroup per (sample, head): every value's segment partials merged in index order (a repeat is bit-identical), the scaling above, then thread x
//                 the softmax of row x over y < d (maximum, expf, the sum in order, e / sum).  A: [N][nH][32][32] fp32; rows x >= d and columns y >= d are zeros.  A column
//                 x of q that is all zero has G = 0 on its row: the row is uniform, 1 / d.
//   csa_apply     four lanes per pixel: lane q the outputs x = 8 q .. 8 q + 7: acc = fma(A[x][y], v[n][y], acc) over y = 0 .. d - 1 in order, fp32, ONE fp16 rounding,
//                 one 16-byte store; outputs x >= d are written as zeros, v's channels >= d are never used.  A^T sits in LDS.
// Nothing crosses samples: a batch's sample equals its own launch bit for bit.
#include "common.h"

namespace innfer {

namespace {

constexpr int CSA_SEG = 1024, CSA_REC = 32 * 32 + 64;

__global__ __launch_bounds__(256) void csa_gram_kernel(const f16* qkv, long gs, long HW, int nH, int d, float* part, int nseg) {
    __shared__ float qs[64][33];
    __shared__ __attribute__((aligned(16))) float ks[64][36];
    const int sg = blockIdx.x, h = blockIdx.y, n = blockIdx.z, t = threadIdx.x;
    const int x = t >> 3, y0 = (t & 7) * 4;
    const long p0 = (long)sg * CSA_SEG;
    const int cnt = (int)min((long)CSA_SEG, HW - p0);
    const f16* qb = qkv + (long)h * gs + ((long)n * HW + p0) * 32;
    const f16* kb = qb + (long)nH * gs;
    float g[4] = {0.f, 0.f, 0.f, 0.f}, nn = 0.f;
    for (int c0 = 0; c0 < cnt; c0 += 64) {
        const int m = min(64, cnt - c0);
        __syncthreads();
        {                                                     // 64 pixels x 4 octets of q and of k: one 16-byte load each per thread
            const int px = t >> 2, oc = t & 3;
            if (px < m) {
                const f16x8 a = *(const f16x8*)(qb + (long)(c0 + px) * 32 + 8 * oc), b = *(const f16x8*)(kb + (long)(c0 + px) * 32 + 8 * oc);
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const bool real = 8 * oc + e < d;
                    qs[px][8 * oc + e] = real ? (float)a[e] : 0.f;
                    ks[px][8 * oc + e] = real ? (float)b[e] : 0.f;
                }
            }
        }
        __syncthreads();
        for (int i = 0; i < m; ++i) {
            const float qv = qs[i][x];
            const f32x4 kv = *(const f32x4*)&ks[i][y0];
#pragma unroll
            for (int j = 0; j < 4; ++j) g[j] = __builtin_fmaf(qv, kv[j], g[j]);
        }
        if (t < 64)
            for (int i = 0; i < m; ++i) {
                const float v = t < 32 ? qs[i][t] : ks[i][t - 32];
                nn = __builtin_fmaf(v, v, nn);
            }
    }
    float* rec = part + (((long)n * nH + h) * nseg + sg) * CSA_REC;
    *(f32x4*)(rec + x * 32 + y0) = f32x4{g[0], g[1], g[2], g[3]};
    if (t < 64) rec[1024 + t] = nn;
}

__global__ __launch_bounds__(256) void csa_softmax_kernel(const float* part, int nseg, int nH, int d, const float* temp, float* A, float* gram) {
    __shared__ float S[32][33], rn[64];
    const int h = blockIdx.x, n = blockIdx.y, t = threadIdx.x;
    const float* rec = part + ((long)n * nH + h) * nseg * CSA_REC;
    float g[4] = {0.f, 0.f, 0.f, 0.f}, nn = 0.f;
    for (int sg = 0; sg < nseg; ++sg) {
#pragma unroll
        for (int j = 0; j < 4; ++j) g[j] += rec[(long)sg * CSA_REC + 4 * t + j];
        if (t < 64) nn += rec[(long)sg * CSA_REC + 1024 + t];
    }
    if (t < 64) rn[t] = 1.0f / fmaxf(sqrtf(nn), 1e-12f);
    if (gram) {
        float* gr = gram + ((long)n * nH + h) * CSA_REC;
#pragma unroll
        for (int j = 0; j < 4; ++j) gr[4 * t + j] = g[j];
        if (t < 64) gr[1024 + t] = nn;
    }
    __syncthreads();
    const float tau = temp[h];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int x = (4 * t + j) >> 5, y = (4 * t + j) & 31;
        S[x][y] = (g[j] * (rn[x] * rn[32 + y])) * tau;
    }
    __syncthreads();
    float* out = A + ((long)n * nH + h) * 1024;
    if (t < 32) {
        if (t < d) {
            float m = S[t][0];
            for (int y = 1; y < d; ++y) m = fmaxf(m, S[t][y]);
            float sum = 0.f;
            for (int y = 0; y < d; ++y) { const float e = expf(S[t][y] - m); S[t][y] = e; sum += e; }
            for (int y = 0; y < 32; ++y) out[t * 32 + y] = y < d ? S[t][y] / sum : 0.f;
        } else {
            for (int y = 0; y < 32; ++y) out[t * 32 + y] = 0.f;
        }
    }
}

__global__ __launch_bounds__(256) void csa_apply_kernel(const f16* qkv, long gs, f16* out, long out_gs, const float* A, long HW, int nH, int d) {
    __shared__ __attribute__((aligned(16))) float At[32][32];          // At[y][x]
    const int h = blockIdx.y, n = blockIdx.z, t = threadIdx.x;
    const float* a = A + ((long)n * nH + h) * 1024;
    for (int i = t; i < 1024; i += 256) At[i & 31][i >> 5] = a[i];
    __syncthreads();
    const long px = (long)blockIdx.x * 64 + (t >> 2);
    const int q = t & 3;
    if (px >= HW) return;
    const f16* vb = qkv + (long)(2 * nH + h) * gs + ((long)n * HW + px) * 32;
    f16x8 v[4];
#pragma unroll
    for (int o = 0; o < 4; ++o) v[o] = *(const f16x8*)(vb + 8 * o);
    float acc[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] = 0.f;
#pragma unroll
    for (int y = 0; y < 32; ++y) {
        if (y < d) {
            const float vv = (float)v[y >> 3][y & 7];
            const f32x4 a0 = *(const f32x4*)&At[y][8 * q], a1 = *(const f32x4*)&At[y][8 * q + 4];
#pragma unroll
            for (int e = 0; e < 4; ++e) { acc[e] = __builtin_fmaf(a0[e], vv, acc[e]); acc[4 + e] = __builtin_fmaf(a1[e], vv, acc[4 + e]); }
        }
    }
    f16x8 r;
#pragma unroll
    for (int e = 0; e < 8; ++e) r[e] = 8 * q + e < d ? (f16)acc[e] : (f16)0.f;
    *(f16x8*)(out + (long)h * out_gs + ((long)n * HW + px) * 32 + 8 * q) = r;
}

inline int csa_nseg(long HW) { return (int)((HW + CSA_SEG - 1) / CSA_SEG); }

}  // namespace

// floats of the segment records csa_gram writes and csa_softmax merges
size_t csa_work_floats(int N, long HW, int nH) { return (size_t)N * nH * csa_nseg(HW) * CSA_REC; }

static int csa_check(const char* what, int N, long HW, int nH, int d) {
    if (N <= 0 || N > 65535 || HW <= 0 || csa_nseg(HW) > 0x7fffff || (HW + 63) / 64 > 0x7fffffffL) return set_error(INNFER_ERR_INVALID, "channel self-attention (%s): N=%d HW=%ld", what, N, HW);
    if (nH < 1 || nH > 8 || d < 1 || d > 32) return set_error(INNFER_ERR_UNSUPPORTED, "channel self-attention (%s): %d heads of %d channels (built: <= 8 heads, <= 32 channels)", what, nH, d);
    return INNFER_OK;
}

// work: csa_work_floats(N, HW, nH) floats; temp: nH device floats; A: N * nH * 1024 floats; gram (may be null): the merged G [32][32], sq [32], sk [32] per (sample, head)
int csa_gram_launch(const f16* qkv, long gs, int N, long HW, int nH, int d, float* work, hipStream_t s) {
    if (!qkv || !work) return set_error(INNFER_ERR_INVALID, "channel self-attention (Gram): null argument");
    if (int rc = csa_check("Gram", N, HW, nH, d)) return rc;
    if (gs < (long)N * HW * 32) return set_error(INNFER_ERR_INVALID, "channel self-attention (Gram): a group stride below N * HW * 32");
    const int nseg = csa_nseg(HW);
    GtScope gt(s, "channel self-attention: Gram and norms", 2.0 * 1088 * nH * N * (double)HW, 128.0 * nH * N * (double)HW);
    hipLaunchKernelGGL(csa_gram_kernel, dim3((unsigned)nseg, (unsigned)nH, (unsigned)N), dim3(256), 0, s, qkv, gs, HW, nH, d, work, nseg);
    INNFER_HIP(hipGetLastError());
    return INNFER_OK;
}

int csa_softmax_launch(const float* work, int N, long HW, int nH, int d, const float* temp, float* A, float* gram, hipStream_t s) {
    if (!work || !temp || !A) return set_error(INNFER_ERR_INVALID, "channel self-attention (softmax): null argument");
    if (int rc = csa_check("softmax", N, HW, nH, d)) return rc;
    const int nseg = csa_nseg(HW);
    GtScope gt(s, "channel self-attention: merge, scale, softmax", 1100.0 * nH * N * nseg, 4.0 * CSA_REC * nH * N * (double)nseg);
    hipLaunchKernelGGL(csa_softmax_kernel, dim3((unsigned)nH, (unsigned)N), dim3(256), 0, s, work, nseg, nH, d, temp, A, gram);
    INNFER_HIP(hipGetLastError());
    return INNFER_OK;
}

int csa_scores_launch(const f16* qkv, long gs, int N, long HW, int nH, int d, const float* temp, float* work, float* A, float* gram, hipStream_t s) {
    if (!temp || !A) return set_error(INNFER_ERR_INVALID, "channel self-attention (scores): null argument");
    if (int rc = csa_gram_launch(qkv, gs, N, HW, nH, d, work, s)) return rc;
    return csa_softmax_launch(work, N, HW, nH, d, temp, A, gram, s);
}

int csa_apply_launch(const f16* qkv, long gs, f16* out, long out_gs, const float* A, int N, long HW, int nH, int d, hipStream_t s) {
    if (!qkv || !out || !A) return set_error(INNFER_ERR_INVALID, "channel self-attention (apply): null argument");
    if (int rc = csa_check("apply", N, HW, nH, d)) return rc;
    if (gs < (long)N * HW * 32 || out_gs < (long)N * HW * 32) return set_error(INNFER_ERR_INVALID, "channel self-attention (apply): a group stride below N * HW * 32");
    GtScope gt(s, "channel self-attention: apply", 2.0 * 1024 * nH * N * (double)HW, 128.0 * nH * N * (double)HW);
    hipLaunchKernelGGL(csa_apply_kernel, dim3((unsigned)((HW + 63) / 64), (unsigned)nH, (unsigned)N), dim3(256), 0, s, qkv, gs, out, out_gs, A, HW, nH, d);
    INNFER_HIP(hipGetLastError());
    return INNFER_OK;
}

}  // namespace innfer
