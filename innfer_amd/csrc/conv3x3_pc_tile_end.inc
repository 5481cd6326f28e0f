// conv3x3_pc: what the consumer waves do after a tile's last chunk -- the epilogue of the instantiation (split / canvas / RLDS / fused last conv / statistics / slab / planar).
// A fragment of the BODY of conv3x3_pc (csrc/conv3x3.hip), included there textually (round 5, VERDICT r4 item 7: the kernel body was 940 lines; no functional
// change -- the device assembly of the translation unit is identical).  It uses the kernel's locals and compile-time flags; not a stand-alone file.
#ifdef INNFER_GRID2_LATE
            // A/B build: the grid alone -- the residual loaded here, at the top of the epilogue, as the 8 x 1 form does
            if constexpr (GRID2 && RLDS) { if (p.res2) residual_prefetch_grid2(p, p.res2, p.res2_gstride, rpre, n, ty0, tx0, cwr, li, cbase); }
            else if constexpr (GRID2) { if (p.res1) residual_prefetch_grid2(p, p.res1, p.res1_gstride, rpre, n, ty0, tx0, cwr, li, cbase); }
#endif
            if constexpr (GRID2 && RLDS) {           // res1 is inside the accumulators (x / s1); res2, where there is one, was prefetched
                if (p.res2) epilogue_slab_grid2<0, false, true, true, 2>(p, acc, rpre, n, ty0, tx0, cwr, li, cbase);
                else epilogue_slab_grid2<0, false, false, true, 0>(p, acc, rpre, n, ty0, tx0, cwr, li, cbase);
            } else if constexpr (GRID2) {            // res1 was prefetched; a second memory residual is loaded in the epilogue
#define EPI(A, B, C) epilogue_slab_grid2<A, B, C, false, (B) ? 1 : 0>(p, acc, rpre, n, ty0, tx0, cwr, li, cbase)
            if (!p.res1) {
                if (p.act == 1) EPI(1, false, false); else if (p.act == 2) EPI(2, false, false); else EPI(0, false, false);
            } else if (!p.res2) {
                if (p.act == 1) EPI(1, true, false); else if (p.act == 2) EPI(2, true, false); else EPI(0, true, false);
            } else {
                if (p.act == 1) EPI(1, true, true); else if (p.act == 2) EPI(2, true, true); else EPI(0, true, true);
            }
#undef EPI
            } else if constexpr (OUTMODE == OUT_SLAB && SPLIT) {
#define EPI(A, B, C) epilogue_slab_split<RPW, NT, A, B, C, CV>(p, acc, n, ty0, tx0, cw, li, cbase)
            if (!p.res1) {
                if (p.act == 1) EPI(1, false, false); else if (p.act == 2) EPI(2, false, false); else EPI(0, false, false);
            } else if (!p.res2) {
                if (p.act == 1) EPI(1, true, false); else if (p.act == 2) EPI(2, true, false);
                else if (NT == 2 && TM == TAPS_1X1 && p.act == 4) EPI((NT == 2 && TM == TAPS_1X1) ? 4 : 0, true, false);         // (the PA gate: the 32-channel 1x1 kernel only)
                else if (NT == 2 && TM == TAPS_1X1 && p.act == 5) EPI((NT == 2 && TM == TAPS_1X1) ? 5 : 0, true, false);
                else EPI(0, true, false);
            } else {
                if (p.act == 1) EPI(1, true, true); else if (p.act == 2) EPI(2, true, true); else EPI(0, true, true);
            }
#undef EPI
            } else if constexpr (OUTMODE == OUT_SLAB && CV && RLDS) {
                if (p.res2) epilogue_slab_cv<RPW, NT, 0, false, true, true, ROWP>(p, acc, ty0, tx0, cw, li, cbase);
                else epilogue_slab_cv<RPW, NT, 0, false, false, true, ROWP>(p, acc, ty0, tx0, cw, li, cbase);
            } else if constexpr (OUTMODE == OUT_SLAB && RLDS) {
                if (p.res2) epilogue_slab<RPW, NT, 0, false, true, true, false, false, false, true, ROWP>(p, acc, n, ty0, tx0, cw, li, cbase, dcur);
                else epilogue_slab<RPW, NT, 0, false, false, true, false, false, false, true, ROWP>(p, acc, n, ty0, tx0, cw, li, cbase, dcur);
            } else if constexpr (OUTMODE == OUT_SLAB && CV) {
#define EPI(A, B, C) epilogue_slab_cv<RPW, NT, A, B, C, false, ROWP>(p, acc, ty0, tx0, cw, li, cbase)
            if (!p.res1) {
                if (p.act == 1) EPI(1, false, false); else if (p.act == 2) EPI(2, false, false);
                else if (NT == 4 && !ROWP && p.act == 7) EPI((NT == 4 && !ROWP) ? 7 : 0, false, false); else EPI(0, false, false);
            } else if (!p.res2) {
                if (p.act == 1) EPI(1, true, false); else if (p.act == 2) EPI(2, true, false); else EPI(0, true, false);
            } else {
                if (p.act == 1) EPI(1, true, true); else if (p.act == 2) EPI(2, true, true); else EPI(0, true, true);
            }
#undef EPI
            } else if constexpr (FUSE) {
                const int lidf = run_start + (p.rev ? run_len - 1 - (jt - slots) : (jt - slots));         // (jt was advanced above; KG == 1: the tile index)
                fused_last_epilogue<RPW, NT>(p, acc, smem + ((g & 1) * STAGE), smem + L::TAIL, n, ty0, tx0, cw, lane, lidf);
            } else if constexpr (PRELU) {
                // act 8 (SRVGGNetCompact): the lane's slopes come back from the wave's LDS copy (same channels as bias_r[t]; KG == 1); plain slab store, no residual
                f32x4 slope_r[NT];
#pragma unroll
                for (int t = 0; t < NT; ++t) slope_r[t] = *(const f32x4*)(slope_lds + lane_cbase<NT, ROWP>(lg) + toff_lin<NT, ROWP>(t));
                epilogue_slab<RPW, NT, 8, false, false, true, false, false, false, false, ROWP, false>(p, acc, n, ty0, tx0, cw, li, cbase, dcur, slope_r);
            } else if constexpr (SPAN) {
                // act 10 (the gate that ends a SPAB: res1 = the block's input, loaded hoisted) / act 9 (SiLU): plain slab store
                if (p.act == 10) epilogue_slab<RPW, NT, 10, true, false, true, false, false, false, false, ROWP, false>(p, acc, n, ty0, tx0, cw, li, cbase, dcur);
                else epilogue_slab<RPW, NT, 9, false, false, true, false, false, false, false, ROWP, false>(p, acc, n, ty0, tx0, cw, li, cbase, dcur);
            } else if constexpr (MISH) {
                // act 11 (Mish, RealPLKSR's DCCM): plain slab store, no residual
                epilogue_slab<RPW, NT, 11, false, false, true, false, false, false, false, ROWP, false>(p, acc, n, ty0, tx0, cw, li, cbase, dcur);
            } else if constexpr (GELU) {
                // act 12 (exact GELU, SwinIR's mlp.fc1): plain slab store, no residual
                epilogue_slab<RPW, NT, 12, false, false, true, false, false, false, false, false, false>(p, acc, n, ty0, tx0, cw, li, cbase, dcur);
            } else if constexpr (OUTMODE == OUT_SLAB) {
            if constexpr (STATS) {
                const int lid = run_start + (p.rev ? run_len - 1 - (jt - slots) : (jt - slots));         // (jt was advanced above)
                epilogue_stats<RPW, NT, TM == TAPS_PHASE, PAIR>(p, acc, bias_r, ty0, tx0, cw, li, cbase, lid / p.KG);
            }
#define EPI(A, B, C) epilogue_slab<RPW, NT, A, B, C, !(C), POLY, TM == TAPS_PHASE, PAIR, false, ROWP, PSH>(p, acc, n, ty0, tx0, cw, li, cbase, dcur)
            if (!p.res1) {
                if (p.act == 1) EPI(1, false, false); else if (p.act == 2) EPI(2, false, false);
                else if (NT == 4 && TM == TAPS_3X3 && !POLY && !ROWP && p.act == 7) EPI((NT == 4 && TM == TAPS_3X3 && !POLY && !ROWP) ? 7 : 0, false, false); else EPI(0, false, false);
            } else if (!p.res2) {
                if (p.act == 1) EPI(1, true, false); else if (p.act == 2) EPI(2, true, false); else if (p.act == 4) EPI(4, true, false);
                else if (p.act == 5) EPI(5, true, false); else EPI(0, true, false);
            } else {
                if (p.act == 1) EPI(1, true, true); else if (p.act == 2) EPI(2, true, true); else EPI(0, true, true);
            }
#undef EPI
            } else {
                epilogue_planar<RPW, NT>(p, acc, n, ty0, tx0, cw, li, lg, cbase);
            }
