// first_conv_mfma: the kernel body (csrc/conv_first.hip), included textually by the two kernels that share it -- first_conv_mfma (act 0 / 1 / 2, chosen at run time) and
// first_conv_mfma_prelu (act 8: per-channel slopes, SRVGGNetCompact's body.0 + body.1) -- so that the first keeps exactly the code it had as the only kernel.  It uses the
// kernel's template parameters (NT, STEPS, FAST16), its argument block `p` (FP), the flags PRELU / IMAP and the pointers slope_p / map_p; not a stand-alone file.
// first_conv_mfma_map (IMAP: a per-input-channel affine on the loaded value, SPAN's `(x - mean) * img_range`) is the third kernel on this body.
    const int lane = threadIdx.x & 63, li = lane & 15, lg = lane >> 4;
    const int nk = p.Cin * 9;
    const int x = blockIdx.x * 64 + (threadIdx.x >> 6) * 16 + li;    // this lane's column
    const int y0 = blockIdx.y * FIRST_ROWS, y1 = min(y0 + FIRST_ROWS, p.H);
    const long n = blockIdx.z;
    if (blockIdx.x * 64 + (int)(threadIdx.x >> 6) * 16 >= p.W) return;      // (a strip beyond the image: whole waves)
    // weight fragments, once per wave: row li of sub-tile t is output channel 32 (t >> 1) + 8 (li >> 2) + 4 (t & 1) + (li & 3) (the plane row order of conv3x3.hip's
    // 64-channel kernels): lane group lg ends with channels 8 lg .. 8 lg + 7 of EACH 32-channel slab plane of its pixel, so the four groups of a pixel column write its whole
    // 64-byte line of a plane and a store instruction covers 16 pixels x 64 bytes of ONE plane (round 5, with the row walk: the stores are what is left of this kernel)
    f16x8 wh[STEPS][NT], wl[STEPS][NT];
#pragma unroll
    for (int st = 0; st < STEPS; ++st)
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const int oc = 32 * (t >> 1) + 8 * (li >> 2) + 4 * (t & 1) + (li & 3);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const int kk = st * 32 + lg * 8 + e;
                const float wv = p.w[(long)min(kk, nk - 1) * p.K + oc];          // (unconditional load, then the select: a predicated load is a branch each -- 64 of them per wave)
                const float w = kk < nk ? wv : 0.f;
                const f16 h = (f16)w;
                wh[st][t][e] = h;
                wl[st][t][e] = (f16)(w - (float)h);
            }
        }
    f32x4 bias[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) bias[t] = *(const f32x4*)(p.bias + 32 * (t >> 1) + 8 * lg + 4 * (t & 1));
    [[maybe_unused]] f32x4 slope[PRELU ? NT : 1];
    if constexpr (PRELU) {
#pragma unroll
        for (int t = 0; t < NT; ++t) slope[t] = *(const f32x4*)(slope_p + 32 * (t >> 1) + 8 * lg + 4 * (t & 1));
    }
    const long hw = (long)p.H * p.W;
    const bool live = x < p.W;
    // the lane's patch elements: (channel, row offset, column) of k = 32 st + 8 lg + e; column validity never changes along the strip, row validity only on the
    // image's first and last row (bit masks, wave-uniform tests)
    int eoff[STEPS][8];                                              // FAST16: element offset from (row y, channel 0, column 0); else (channel << 20 | column + 1) -- W < 2^20 (launch)
    unsigned xok = 0, top = 0, bot = 0;
#pragma unroll
    for (int st = 0; st < STEPS; ++st)
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int kk = st * 32 + lg * 8 + e;
            const int ci = kk / 9, tap = kk - ci * 9, r = tap / 3, sx = tap - r * 3, X = x + sx - 1;
            eoff[st][e] = FAST16 ? (int)(ci * hw) + (r - 1) * p.W + X : (ci << 20) | (X + 1);
            if (live && kk < nk && X >= 0 && X < p.W) xok |= 1u << (st * 8 + e);
            if (r == 0) top |= 1u << (st * 8 + e);
            if (r == 2) bot |= 1u << (st * 8 + e);
        }
    const bool any_lo = !FAST16 && !IMAP && (p.in_f32 != 0 || (p.in_u8 && !p.in_round16));
    [[maybe_unused]] const f16* in16 = (const f16*)p.in + n * p.Cin * hw;
    // One row of the strip: (FAST16) `raw` holds the row's 8 STEPS patch values as loaded -- requested one row ahead, first touched here.
    auto process = [&](int y, const unsigned (&raw)[STEPS][8]) __attribute__((always_inline)) {
        const unsigned ok = xok & (y == 0 ? ~top : ~0u) & (y == p.H - 1 ? ~bot : ~0u);
        f32x4 acc[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t) acc[t] = bias[t];
#pragma unroll
        for (int st = 0; st < STEPS; ++st) {             // compile-time index into the fragment arrays (a runtime one would send them to scratch)
            f16x8 xh, xl;
            if constexpr (FAST16) {                      // the values are the hi operands as they lie in memory, no lo part
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const bool o = (ok >> (st * 8 + e)) & 1;
                    xh[e] = o ? __builtin_bit_cast(f16, (unsigned short)raw[st][e]) : (f16)0.f;
                    xl[e] = (f16)0.f;
                }
            } else {
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const int kk = st * 32 + lg * 8 + e;
                    const int r = (kk - (kk / 9) * 9) / 3;
                    float v = 0.f;
                    if constexpr (IMAP) {        // the mapped operand: an fp16 value, no lo part; outside the image the operand stays zero
                        if ((ok >> (st * 8 + e)) & 1) v = first_conv_input_map(p, map_p, n, eoff[st][e] >> 20, y + r - 1, (eoff[st][e] & 0xfffff) - 1, hw);
                    } else
                    if ((ok >> (st * 8 + e)) & 1) v = first_conv_input(p, n, eoff[st][e] >> 20, y + r - 1, (eoff[st][e] & 0xfffff) - 1, hw);
                    const f16 h = (f16)v;
                    xh[e] = h;
                    xl[e] = (f16)(v - (float)h);
                }
            }
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wh[st][t], xh, acc[t], 0, 0, 0);
                acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wl[st][t], xh, acc[t], 0, 0, 0);
                if (any_lo) acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wh[st][t], xl, acc[t], 0, 0, 0);
            }
        }
        if (!live) return;
        const long pix = n * hw + (long)y * p.W + x;
        f16 h[4 * NT], l[4 * NT];
        // (the activation chosen ONCE per row: a uniform test per value is a branch per value in this unrolled code -- 16 of them, with the accumulators copied around each)
        auto finish = [&](auto act_tag) __attribute__((always_inline)) {
            constexpr int ACT = decltype(act_tag)::value;
#pragma unroll
            for (int t = 0; t < NT; ++t)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    float f = acc[t][j];
                    if (ACT == 1) f = __builtin_amdgcn_fmed3f(f, 0.2f * f, 3.0e38f);      // (one instruction behind the multiply; a finite top: conv3x3_epilogue_slab.h ACT_TOP)
                    else if (ACT == 2) f = __builtin_amdgcn_fmed3f(f, 0.f, 3.0e38f);
                    else if (ACT == 8) f = f >= 0.f ? f : slope[PRELU ? t : 0][j] * f;
                    h[4 * t + j] = (f16)f;
                    l[4 * t + j] = (f16)((f - (float)h[4 * t + j]) * 2048.0f);
                }
        };
        if constexpr (PRELU) finish(std::integral_constant<int, 8>{});
        else if (p.act == 1) finish(std::integral_constant<int, 1>{}); else if (p.act == 2) finish(std::integral_constant<int, 2>{}); else finish(std::integral_constant<int, 0>{});
        const long o = pix * 32 + 8 * lg;
#pragma unroll
        for (int q = 0; q < NT / 2; ++q) {                            // plane q: tiles 2 q, 2 q + 1
            f16x8 v;
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = h[8 * q + e];
            *(f16x8*)(p.out + q * p.out_gstride + o) = v;
            if (p.out2) *(f16x8*)(p.out2 + q * p.out2_gstride + o) = v;
            if (p.out_lo) {
#pragma unroll
                for (int e = 0; e < 8; ++e) v[e] = l[8 * q + e];
                *(f16x8*)(p.out + p.out_lo + q * p.out_gstride + o) = v;
                if (p.out2) *(f16x8*)(p.out2 + p.out2_lo + q * p.out2_gstride + o) = v;
            }
        }
    };
    if constexpr (FAST16) {
        // unconditional loads from a clamped offset (an element outside the image reads the row's own first value, zeroed when it is used): independent, all in flight
        // together, and the NEXT row's are requested before this row is multiplied and stored (two register sets used alternately, as in unet_first_mfma)
        auto request = [&](int y, unsigned (&raw)[STEPS][8]) __attribute__((always_inline)) {
            const unsigned ok = xok & (y == 0 ? ~top : ~0u) & (y == p.H - 1 ? ~bot : ~0u);
            const unsigned short* row = (const unsigned short*)in16 + (long)y * p.W;
#pragma unroll
            for (int st = 0; st < STEPS; ++st)
#pragma unroll
                for (int e = 0; e < 8; ++e) raw[st][e] = row[((ok >> (st * 8 + e)) & 1) ? eoff[st][e] : 0];
        };
        unsigned rawA[STEPS][8], rawB[STEPS][8];
        request(y0, rawA);
        int y = y0;
        for (; y + 1 < y1; y += 2) {
            request(y + 1, rawB);
            process(y, rawA);
            if (y + 2 < y1) request(y + 2, rawA);
            process(y + 1, rawB);
        }
        if (y < y1) process(y, rawA);
    } else {
        unsigned none[STEPS][8] = {};
        for (int y = y0; y < y1; ++y) process(y, none);
    }
