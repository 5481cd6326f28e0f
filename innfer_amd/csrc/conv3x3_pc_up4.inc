// conv3x3_pc, UP4 (TMF | PC_UP4): the consumer waves' own walk of the one-visit up-conv -- four phases per tile as straight-line code.
// A fragment of the BODY of conv3x3_pc (csrc/conv3x3.hip), included there textually (round 5, VERDICT r4 item 7: the kernel body was 940 lines; no functional
// change -- the device assembly of the translation unit is identical).  It uses the kernel's locals and compile-time flags; not a stand-alone file.
    if constexpr (UP4) {
        // ---- the one-pass up-conv's own walk: per tile, the four phases as straight-line code (a phase's accumulators live from its bias to its epilogue only;
        // a `switch` over the phase inside the generic step loop made the allocator carry them across all four unrolled bodies: 344 bytes of scratch per lane) ----
        // the four phases' biases (256 floats) in the 1 KB behind the weight ring: a phase starts from four ds_read_b128 instead of holding sixteen bias registers
        // across the phase before it (the kernel sits at the 168-register budget of a 12-wave workgroup)
        float* const bias_lds = (float*)(smem + L::TAIL);
        if (cw == 0) *(f32x4*)(bias_lds + 4 * lane) = *(const f32x4*)(p.bias + 4 * lane);
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
        asm volatile("s_barrier" ::: "memory");                   // both groups of the first tile and the first panel have landed
        int slot0 = 0;                                            // LDS slot of the tile's group 0: (2 T) % 3
#ifdef INNFER_ABLATE
        const bool no_mfma = (p.abl & 8) != 0;
#else
        constexpr bool no_mfma = false;
#endif
        for (int jt = j0; jt < run_len; jt += slots) {
            int kg, n, ty0, tx0;
            decode(jt, kg, n, ty0, tx0);
            // (opaque per-tile copies of the lane coordinates: otherwise the four epilogues' per-lane address parts -- a dozen 64-bit values -- are hoisted out of
            //  the tile loop and live across all of it: scratch spills at the 168-register budget of a 12-wave workgroup)
            int li_t = li, lg_t = lg;
            asm volatile("" : "+v"(li_t), "+v"(lg_t));
            auto phase = [&](auto phc) __attribute__((always_inline)) {
                constexpr int PH = decltype(phc)::value, A = PH >> 1, B = PH & 1;
                const int cbase = PH * WROWS + lane_cbase<NT, ROWP>(lg_t);
                f32x4 acc[NT][MT];
#pragma unroll
                for (int t = 0; t < NT; ++t) {
                    const f32x4 bt = *(const f32x4*)(bias_lds + cbase + toff_lin<NT, ROWP>(t));
#pragma unroll
                    for (int m = 0; m < MT; ++m) acc[t][m] = bt;
                }
#pragma unroll
                for (int cg = 0; cg < 2; ++cg) {
                    const int sl = slot0 + cg;
                    const char* st = smem + (sl >= 3 ? sl - 3 : sl) * IN_BYTES;
                    const char* sw = smem + 3 * IN_BYTES + cg * W_BYTES;              // (eight steps per tile: the step's parity is the group)
                    if (!no_mfma) four_tap(std::integral_constant<int, (TAPS_PHASE << (3 * A + B))>{}, acc, st, sw);
                    if (cg == 1) {       // the phase's 16 x 32 virtual pixels go out through the phase-lattice epilogue (tile origin shifted by (a, b))
                        if (p.act == 1) epilogue_slab<RPW, NT, 1, false, false, true, false, true, false, false, ROWP>(p, acc, n, ty0 + A, tx0 + B, cw, li_t, cbase);
                        else if (p.act == 2) epilogue_slab<RPW, NT, 2, false, false, true, false, true, false, false, ROWP>(p, acc, n, ty0 + A, tx0 + B, cw, li_t, cbase);
                        else epilogue_slab<RPW, NT, 0, false, false, true, false, true, false, false, ROWP>(p, acc, n, ty0 + A, tx0 + B, cw, li_t, cbase);
                    }
                    asm volatile("s_barrier" ::: "memory");
                }
            };
            phase(std::integral_constant<int, 0>{});
            phase(std::integral_constant<int, 1>{});
            phase(std::integral_constant<int, 2>{});
            phase(std::integral_constant<int, 3>{});
            slot0 = slot0 == 0 ? 2 : slot0 - 1;
        }
        return;
    }
