// plk_conv: the partial large-kernel conv of RealPLKSR (PLKConv2d) -- a k x k zero-padded conv (k odd, 3 .. 17) of the FIRST 16 channels of a 32-channel slab group;
// the group's other 16 channels pass through.  Input and output are different slab groups (other workgroups still read the halo of the input while this one stores),
// so the kernel also copies channels 16 .. 31: the result is a whole group and the next launch needs to know nothing about the split.
//
// On the matrix cores as D[16 out channels][16 pixels] += A[16][32] B[32][16] with v_mfma_f32_16x16x32_f16: one step's k dimension is TWO TAPS x 16 input channels
// (lane group lg = lane >> 4: the tap in column 2 hp + (lg >> 1) of kernel row dy, channels 8 (lg & 1) .. + 7) -- the taps of a kernel row are paired horizontally,
// (k + 1) / 2 pairs per row (the pair behind the last column has zero weights and reads the last column's pixel): 9 x 17 = 153 steps for k = 17.
//   B: a lane's eight values are 16 contiguous bytes of ONE pixel of the staged tile -- one ds_read_b128, no shuffle: the tile lies in LDS as [row][column][16 channels]
//      (32 bytes per pixel), the haloed 16 x 32 tile is (16 + 2 r) x (32 + 2 r) x 32 B = 49 152 B for r = 8, so three workgroups share a CU.
//   A: the k^2 x 16 x 16 weights do not fit beside the tile (153 KB for k = 17), so they STREAM: the panel is packed on the host as [pair][dy][lane][8] fp16 -- a wave's
//      fragment of a step is 1 KB of consecutive bytes -- and every wave reads its fragments straight from global memory (L2 hits: every workgroup of the launch reads the
//      same panel), one column pair's k fragments at a time.
// A workgroup of four waves owns a 16 x 32 tile; a wave owns four rows of it as eight 16-pixel segments (eight accumulators).  For one column pair the B fragment of
// input row iy serves the four output rows iy - dy: the wave walks the k + 3 input rows of its strip, reads each row's two fragments ONCE and multiplies them with the
// (up to) four kernel rows they meet -- 2 (k + 3) LDS reads for 8 k MFMAs per pair (40 for 136 at k = 17) instead of one read per MFMA, which had the first form of this
// kernel bound by LDS reads at 2.4 x a trunk conv's time (now 2.1 x: DESIGN.md 3.4k).  4 x 153 x 8 = 4896 MFMAs per tile against 2304 of a 64 -> 64 nine-tap launch.
// fp32 accumulation from the bias, one rounding at the store.  Ragged tiles and images smaller than the radius need nothing special: the stage reads zero outside the
// image, the stores and the copy are guarded.
#include "common.h"

namespace innfer {

namespace {

constexpr int PLK_TH = 16, PLK_TW = 32, PLK_RMAX = 8;

struct PlkP {
    const f16* in; f16* out;                      // channel 0 of the input / output group
    const f16* wpk; const float* bias;            // plk_pack panel; 16 floats
    int H, W;
};

template <int K>
__global__ __launch_bounds__(256) void plk_conv_kernel(const PlkP p) {
    constexpr int r = K / 2, TWh = PLK_TW + 2 * r, THh = PLK_TH + 2 * r, NP = (K + 1) / 2;
    __shared__ __attribute__((aligned(16))) char smem[THh * TWh * 32];
    const int tx0 = blockIdx.x * PLK_TW, ty0 = blockIdx.y * PLK_TH;
    const long img = (long)blockIdx.z * p.H * p.W;
    // the haloed tile's channels 0 .. 15: 32 bytes per pixel as two 16-byte pieces, zero outside the image
    for (int i = threadIdx.x; i < THh * TWh * 2; i += 256) {
        const int px = i >> 1, ly = px / TWh, lx = px - ly * TWh;
        const int y = ty0 - r + ly, x = tx0 - r + lx;
        f16x8 v = {0, 0, 0, 0, 0, 0, 0, 0};
        if (y >= 0 && y < p.H && x >= 0 && x < p.W) v = *(const f16x8*)(p.in + (img + (long)y * p.W + x) * 32 + (i & 1) * 8);
        *(f16x8*)(smem + i * 16) = v;
    }
    // channels 16 .. 31 of the tile's own pixels pass through
    for (int i = threadIdx.x; i < PLK_TH * PLK_TW * 2; i += 256) {
        const int px = i >> 1, y = ty0 + (px >> 5), x = tx0 + (px & 31);
        if (y < p.H && x < p.W) {
            const long o = (img + (long)y * p.W + x) * 32 + 16 + (i & 1) * 8;
            *(f16x8*)(p.out + o) = *(const f16x8*)(p.in + o);
        }
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, li = lane & 15, lg = lane >> 4;
    f32x4 acc[4][2];
    {
        const f32x4 b = *(const f32x4*)(p.bias + lg * 4);       // D row = output channel 4 lg + j, column = pixel li
#pragma unroll
        for (int ry = 0; ry < 4; ++ry) { acc[ry][0] = b; acc[ry][1] = b; }
    }
    const char* bbase = smem + ((wv * 4) * TWh + li) * 32 + (lg & 1) * 16;          // pixel (row 4 wv, column li) of the haloed tile = tap (0, 0) of output (4 wv, li)
    const f16x8* wp = (const f16x8*)p.wpk + lane;
#pragma unroll 1
    for (int hp = 0; hp < NP; ++hp) {
        const int dx = min(2 * hp + (lg >> 1), K - 1);        // (the pair behind the last column: zero weights, the last column's pixel)
        const char* bp = bbase + dx * 32;
        f16x8 a[K];
#pragma unroll
        for (int dy = 0; dy < K; ++dy) a[dy] = wp[(hp * K + dy) * 64];
#pragma unroll
        for (int iy = 0; iy < K + 3; ++iy) {                  // input row 4 wv + iy of the haloed tile meets output row ry through kernel row dy = iy - ry
            const f16x8 b0 = *(const f16x8*)(bp + iy * TWh * 32), b1 = *(const f16x8*)(bp + (iy * TWh + 16) * 32);
#pragma unroll
            for (int ry = 0; ry < 4; ++ry) {
                const int dy = iy - ry;
                if (dy >= 0 && dy < K) {
                    acc[ry][0] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a[dy], b0, acc[ry][0], 0, 0, 0);
                    acc[ry][1] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a[dy], b1, acc[ry][1], 0, 0, 0);
                }
            }
        }
    }
#pragma unroll
    for (int m = 0; m < 8; ++m) {
        const int y = ty0 + wv * 4 + (m >> 1), x = tx0 + (m & 1) * 16 + li;
        if (y < p.H && x < p.W) {
            f16x4 h;
#pragma unroll
            for (int j = 0; j < 4; ++j) h[j] = (f16)acc[m >> 1][m & 1][j];
            *(f16x4*)(p.out + (img + (long)y * p.W + x) * 32 + lg * 4) = h;
        }
    }
}

}  // namespace

size_t plk_packed_bytes(int k) { return (size_t)((k + 1) / 2) * k * 64 * 16; }

// w [16][16][k][k] fp32 (OIHW) -> [pair][dy][lane][8] fp16: lane (lg, row) of step (hp, dy) holds output channel `row`, tap (dy, 2 hp + (lg >> 1)), input channels
// 8 (lg & 1) .. + 7; zeros behind the last column
void plk_pack(const float* w, int k, void* packed) {
    f16* d = (f16*)packed;
    const int kk = k * k, np = (k + 1) / 2;
    for (int hp = 0; hp < np; ++hp)
        for (int dy = 0; dy < k; ++dy)
            for (int l = 0; l < 64; ++l) {
                const int lg = l >> 4, row = l & 15, dx = 2 * hp + (lg >> 1);
                for (int j = 0; j < 8; ++j)
                    d[(((size_t)hp * k + dy) * 64 + l) * 8 + j] = dx < k ? (f16)w[((size_t)row * 16 + (lg & 1) * 8 + j) * kk + dy * k + dx] : (f16)0.f;
            }
}

int plk_conv_launch(const PlkLaunch& L, hipStream_t s) {
    if (!L.in || !L.out || !L.wpk || !L.bias) return set_error(INNFER_ERR_INVALID, "plk_conv: null argument");
    if (L.k < 3 || L.k > 2 * PLK_RMAX + 1 || !(L.k & 1)) return set_error(INNFER_ERR_UNSUPPORTED, "plk_conv: kernel size %d (built: odd, 3 .. 17)", L.k);
    if (L.N <= 0 || L.H <= 0 || L.W <= 0) return set_error(INNFER_ERR_INVALID, "plk_conv: bad shape %dx%dx%d", L.N, L.H, L.W);
    const long G = (long)L.N * L.H * L.W * 32;
    if (L.in < L.out + G && L.out < L.in + G)
        return set_error(INNFER_ERR_INVALID, "plk_conv: the output group overlaps the input group (other workgroups still read the halo of what this one would overwrite)");
    const int gx = (L.W + PLK_TW - 1) / PLK_TW, gy = (L.H + PLK_TH - 1) / PLK_TH;
    if (L.N > 65535 || gy > 65535) return set_error(INNFER_ERR_UNSUPPORTED, "plk_conv: %d images of %d rows exceed the launch grid", L.N, L.H);
    const PlkP p{L.in, L.out, L.wpk, L.bias, L.H, L.W};
    const double px = (double)L.N * L.H * L.W;
    GtScope gt(s, "plk_conv k x k, 16 of 32 channels", 2.0 * L.k * L.k * 256.0 * px, px * 128.0 + (double)L.k * L.k * 512.0);
    const dim3 grid((unsigned)gx, (unsigned)gy, (unsigned)L.N);
    switch (L.k) {
#define PLK_K(K_) case K_: hipLaunchKernelGGL(plk_conv_kernel<K_>, grid, dim3(256), 0, s, p); break
        PLK_K(3); PLK_K(5); PLK_K(7); PLK_K(9); PLK_K(11); PLK_K(13); PLK_K(15); PLK_K(17);
#undef PLK_K
    }
    INNFER_HIP(hipGetLastError());
    return INNFER_OK;
}

}  // namespace innfer
