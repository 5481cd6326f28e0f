// The tail of BasicSR's SRVGGNetCompact: out = PixelShuffle(s)(last conv) + nearest_upsample(x, s), one pass.
//
// The last conv (nf -> C s^2, no activation) runs as an ordinary slab conv; this kernel reads its fp16 slab on the LR grid and the NETWORK'S OWN INPUT
// (planar fp16, or the uint8 HWC image exactly as the first conv reads it) and writes the result: planar fp16 / fp32, or the uint8 HWC image with
// tensor2np as the store.  Per output value: r = fp16(float(slab value) + float(fp16 base value)) -- one fp32 add, one rounding, what torch's half
// `out += base` does -- then float(r), or the quantisation of the last convs' uint8 epilogue (conv3x3_planar.h) on r.
//
// Without a base (ShuffleAddLaunch.base == nullptr) the same pass is PixelShuffle(s) alone with the same three stores: SPAN's tail.
//
// Memory bound: 2 C s^2 bytes in and at most 4 C s^2 bytes out per LR pixel.  One thread owns one LR pixel: it reads the pixel's C s^2 <= 64 channels as
// 16-byte pieces of the pixel's 64-byte run in each slab plane (consecutive lanes = consecutive pixels: a wave's loads cover whole lines) and writes, per
// output channel and row phase, its s consecutive output values as one vector store where the alignment allows -- consecutive lanes write consecutive
// pieces of one HR row, 64 s values per wave and instruction.  No LDS: the stores are contiguous as they are.
#include "common.h"

namespace innfer {
namespace {

struct SP {
    const f16* slab; long gstride;
    const void* base; int base_u8, base_norm;
    void* out; int out_denorm;
    int C; long npix; int H, W;
};

// v[0 .. n) to p: one store of n elements where ALIGNED says the address is a multiple of the run's size (n = 2, 4), element stores otherwise
template <typename T, int n, bool ALIGNED>
__device__ __forceinline__ void store_run(T* p, const T (&v)[4]) {
    if constexpr (ALIGNED && n == 4) {
        typedef T V4 __attribute__((ext_vector_type(4)));
        *(V4*)p = V4{v[0], v[1], v[2], v[3]};
    } else if constexpr (ALIGNED && n == 2) {
        typedef T V2 __attribute__((ext_vector_type(2)));
        *(V2*)p = V2{v[0], v[1]};
    } else {
#pragma unroll
        for (int i = 0; i < n; ++i) p[i] = v[i];
    }
}

// OUT: 0 fp16 planar, 1 fp32 planar, 2 uint8 HWC.  ALIGNED: `out` is aligned to S elements (planar) / to S * C bytes where that is 4, 8, 12 or 16 (uint8).
template <int S, int OUT, bool ALIGNED>
__global__ __launch_bounds__(256) void shuffle_add_kernel(const SP p) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= p.npix) return;
    constexpr int SS = S * S;
    constexpr int NV = (4 * SS + 7) / 8;                      // 16-byte pieces of the widest case (C = 4)
    const int K = p.C * SS;
    f16x8 v[NV];
#pragma unroll
    for (int q = 0; q < NV; ++q) {
        if (8 * q < K) v[q] = *(const f16x8*)(p.slab + (long)(q >> 2) * p.gstride + i * 32 + (q & 3) * 8);
        else v[q] = f16x8{0, 0, 0, 0, 0, 0, 0, 0};
    }
    const int x = (int)(i % p.W);
    const long row = i / p.W;                                 // n * H + y
    const int y = (int)(row % p.H);
    const long n = row / p.H;
    const long hw = (long)p.H * p.W;
    // the input value as the first conv sees it (conv_first.hip first_conv_input, in_round16): np2tensor's value rounded to fp16
    float b[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        b[c] = 0.f;
        if (c >= p.C || !p.base) continue;                       // (no base: PixelShuffle alone -- fp16(v + 0) is v)
        if (p.base_u8) {
            int sc = c;
            if (p.C % 3 == 0) sc = p.C - 1 - c; else if (p.C == 4 && c < 3) sc = 2 - c;
            float u = __fdiv_rn((float)((const uint8_t*)p.base)[i * p.C + sc], 255.0f);
            if (p.base_norm) u = fminf(fmaxf(__fmul_rn(__fsub_rn(u, 0.5f), 2.0f), -1.0f), 1.0f);
            b[c] = (float)(f16)u;
        } else {
            b[c] = (float)((const f16*)p.base)[(n * p.C + c) * hw + (long)y * p.W + x];
        }
    }
    const int WO = p.W * S;
    const long HO = (long)p.H * S;
#pragma unroll
    for (int a = 0; a < S; ++a) {
        const long Y = (long)y * S + a;
        [[maybe_unused]] uint8_t px[16];                      // OUT 2: the S pixels of this row phase, C bytes each
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            if (c >= p.C) continue;
            f16 r[4];
#pragma unroll
            for (int bb = 0; bb < S; ++bb) {
                const int ch = c * SS + a * S + bb;           // (compile-time after unrolling: a register of v)
                float f = (float)v[ch >> 3][ch & 7] + b[c];
                r[bb] = (f16)f;
            }
#pragma unroll
            for (int bb = S; bb < 4; ++bb) r[bb] = (f16)0.f;
            if constexpr (OUT == 0) {
                store_run<f16, S, ALIGNED>((f16*)p.out + ((n * p.C + c) * HO + Y) * WO + (long)x * S, r);
            } else if constexpr (OUT == 1) {
                const float rf[4] = {(float)r[0], (float)r[1], (float)r[2], (float)r[3]};
                store_run<float, S, ALIGNED>((float*)p.out + ((n * p.C + c) * HO + Y) * WO + (long)x * S, rf);
            } else {
                // tensor2np on the fp16 value (conv3x3_planar.h, out_round16): optional denormalisation, clip(255 x), round half to even, RGB(A) -> BGR(A)
#pragma unroll
                for (int bb = 0; bb < S; ++bb) {
                    float w = (float)r[bb];
                    if (p.out_denorm) w = fminf(fmaxf(__fdiv_rn(__fsub_rn(w, -1.0f), 2.0f), 0.0f), 1.0f);
                    w = fminf(fmaxf(__fmul_rn(255.0f, w), 0.0f), 255.0f);
                    const uint8_t q = (uint8_t)__float2int_rn(w);
                    // byte bb * C + sc of the run, sc = the channel's place in the BGR(A) pixel; C is a run-time value, every index here a compile-time one
                    if (p.C == 1) px[bb] = q;
                    else if (p.C == 2) px[bb * 2 + (c & 1)] = q;
                    else if (p.C == 3) px[bb * 3 + (c < 3 ? 2 - c : 0)] = q;
                    else px[bb * 4 + (c < 3 ? 2 - c : 3)] = q;
                }
            }
        }
        if constexpr (OUT == 2) {
            uint8_t* o = (uint8_t*)p.out + ((n * HO + Y) * WO + (long)x * S) * p.C;
            const int nb = S * p.C;                           // 1 .. 16 bytes, consecutive lanes follow each other
            if (ALIGNED && (nb & 3) == 0) {
#pragma unroll
                for (int d = 0; d < 4; ++d)
                    if (4 * d < nb) ((unsigned*)o)[d] = (unsigned)px[4 * d] | ((unsigned)px[4 * d + 1] << 8) | ((unsigned)px[4 * d + 2] << 16) | ((unsigned)px[4 * d + 3] << 24);
            } else {
#pragma unroll
                for (int d = 0; d < 16; ++d)
                    if (d < nb) o[d] = px[d];
            }
        }
    }
}

template <int S>
int launch_s(const SP& p, int out_mode, bool aligned, hipStream_t s) {
    const dim3 grid((unsigned)((p.npix + 255) / 256));
#define SA(O_) do { if (aligned) hipLaunchKernelGGL((shuffle_add_kernel<S, O_, true>), grid, dim3(256), 0, s, p); \
                    else hipLaunchKernelGGL((shuffle_add_kernel<S, O_, false>), grid, dim3(256), 0, s, p); } while (0)
    if (out_mode == 0) SA(0); else if (out_mode == 1) SA(1); else SA(2);
#undef SA
    INNFER_HIP(hipGetLastError());
    return INNFER_OK;
}

}  // namespace

int shuffle_add_launch(const ShuffleAddLaunch& L, hipStream_t s) {
    if (!L.slab || !L.out) return set_error(INNFER_ERR_INVALID, "shuffle_add: null argument");
    if (L.s < 1 || L.s > 4 || L.C < 1 || L.C > 4 || L.out_mode < 0 || L.out_mode > 2)
        return set_error(INNFER_ERR_UNSUPPORTED, "shuffle_add: scale %d (1..4), %d channels (1..4), out_mode %d (0 fp16, 1 fp32, 2 uint8 image)", L.s, L.C, L.out_mode);
    if (L.N <= 0 || L.H <= 0 || L.W <= 0) return set_error(INNFER_ERR_INVALID, "shuffle_add: bad shape %dx%dx%d", L.N, L.H, L.W);
    const long npix = (long)L.N * L.H * L.W;
    if (L.gstride < npix * 32) return set_error(INNFER_ERR_INVALID, "shuffle_add: group stride %ld < %ld (N * H * W * 32)", L.gstride, npix * 32);
    if ((npix + 255) / 256 > 0x7fffffffL) return set_error(INNFER_ERR_UNSUPPORTED, "shuffle_add: %ld pixels exceed the launch grid", npix);
    SP p{L.slab, L.gstride, L.base, L.base_u8, L.base_norm, L.out, L.out_denorm, L.C, npix, L.H, L.W};
    // a thread's s consecutive outputs start at a multiple of s elements (planar) / of s * C bytes (uint8) behind `out`: vector stores where `out` itself is aligned to that
    const size_t run = L.out_mode == 2 ? (size_t)L.s * L.C : (size_t)L.s * (L.out_mode == 1 ? 4 : 2);
    const bool aligned = L.out_mode == 2 ? (run % 4 == 0 && (uintptr_t)L.out % 4 == 0) : ((L.s == 2 || L.s == 4) && (uintptr_t)L.out % run == 0);
    switch (L.s) {
        case 1: return launch_s<1>(p, L.out_mode, aligned, s);
        case 2: return launch_s<2>(p, L.out_mode, aligned, s);
        case 3: return launch_s<3>(p, L.out_mode, aligned, s);
        default: return launch_s<4>(p, L.out_mode, aligned, s);
    }
}

}  // namespace innfer
