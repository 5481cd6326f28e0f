// Pass kernels that several generator engines launch unchanged: tanh(raw + bias) as the NCHW output (UNet, ResNet).  Each translation unit that includes
// this header gets its own copy, as with norm_stats.h.  (The engines' NCHW -> slab kernels stay their own: the same copy written three ways, which the compiler
// gives three different register budgets.)
#pragma once
#include "common.h"

namespace innfer {

// raw[.., 0:C] (fp32 rows of cpad floats) + bias -> tanh -> NCHW (fp16 or fp32); one thread per pixel
static __global__ void tanh_bias_to_nchw(const float* raw, int cpad, int C, long HW, int N, const float* bias, void* out, int out_f32) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long)N * HW) return;
    const long n = i / HW, px = i % HW;
    for (int c = 0; c < C; ++c) {
        const float y = fast_tanh(raw[i * cpad + c] + bias[c]);
        const long o = (n * C + c) * HW + px;
        if (out_f32) ((float*)out)[o] = y; else ((f16*)out)[o] = (f16)y;
    }
}

inline int launch_tanh_bias_to_nchw(const float* raw, int cpad, int C, long HW, int N, const float* bias, void* out, int out_f32, hipStream_t s) {
    hipLaunchKernelGGL(tanh_bias_to_nchw, dim3((unsigned)((N * HW + 255) / 256)), dim3(256), 0, s, raw, cpad, C, HW, N, bias, out, out_f32);
    INNFER_HIP(hipGetLastError());
    return INNFER_OK;
}

}  // namespace innfer
