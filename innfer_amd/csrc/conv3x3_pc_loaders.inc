// conv3x3_pc: the loader waves (LDS-DMA of halo tiles and weight panels for every loader form: plain, canvas, S9, S2, POLY, PAIR, SPLIT, UP4, RLDS order).
// A fragment of the BODY of conv3x3_pc (csrc/conv3x3.hip), included there textually (round 5, VERDICT r4 item 7: the kernel body was 940 lines; no functional
// change -- the device assembly of the translation unit is identical).  It uses the kernel's locals and compile-time flags; not a stand-alone file.
    if (wave >= NCW) {
        // ================================ loaders ================================
        // The loaders of the 16- / 32-output kernels issue at raised priority: their layers wait for the LDS-DMA stream, and a piece issued between the
        // consumers' MFMAs costs 100-185 cycles of queueing (MI355X_MICROARCH.md).  32-output layers 0.1344 -> 0.1320 ms, last conv -3 %; the 64-output
        // kernels, which wait for the matrix pipe, lose 0.5 % with it and keep the default (profiles/r3/prio_ab.txt; INNFER_PRIO: A/B builds).
#if defined(__HIP_DEVICE_COMPILE__)
#ifdef INNFER_PRIO
        __builtin_amdgcn_s_setprio(INNFER_PRIO);
#else
        if constexpr (NT <= 2 && !GRID2) __builtin_amdgcn_s_setprio(3);       // (GRID2 is a 64-output kernel: WROWS 64)
#endif
#endif
        const int lw = wave - NCW;
        int loff[KQ];
        int lpix[POLY ? KQ : 1];
        int s9_ty0 = 0, s9_tx0 = 0, s9_n = 0; bool s9_edge = false;          // S9: the current tile (edge tiles re-derive their offsets per chunk)
        constexpr bool S2PRE = S2 && RPW == 2;      // (the 24-row, 32-channel form keeps the per-chunk derivation: with the per-tile one hipcc leaves its argument struct in scratch memory)
        int s2_off[S2PRE ? KQ : 1]; unsigned s2_m0 = 0, s2_m1 = 0, s2_m2 = 0, s2_m3 = 0;   // S2 edge tiles: per-piece offsets of phase (0, 0), validity bits per phase
        static_assert(!S2 || KQ <= 32, "one validity bit per piece");
        {
            const int ypar = p.up ? ((p.y0 - 1) & 1) : 0;
#pragma unroll
            for (int k = 0; k < KQ; ++k) {
                const int px = (lw + NLW * k) * 16 + (lane >> 2);
                const int ly = px / LWP;
                int lx = px - ly * LWP;
                const bool imgb = PAIR && lx >= 18;                                       // PAIR: LDS columns 18 .. 35 are the halo row of the pair's second image
                if (imgb) lx -= 18;
                const int slot = (lane & 3) ^ (((px >> 2) & 1) << 1);
                const int ry = S2 ? 2 * ly : p.up ? (ly + ypar) >> 1 : ly;
                const int rx = S2 ? 2 * lx : p.up ? (lx + 1) >> 1 : lx;
                // only the halo rows / columns a tap of the mask reads are fetched (a 1x1 conv: none; the other lanes' pieces arrive as zeros
                // without memory traffic)
                constexpr int R0 = (TM & 0x007) ? 0 : (TM & 0x038) ? 1 : 2, R1 = (TM & 0x1C0) ? 2 : (TM & 0x038) ? 1 : 0;
                constexpr int S0 = (TM & 0x049) ? 0 : (TM & 0x092) ? 1 : 2, S1 = (TM & 0x124) ? 2 : (TM & 0x092) ? 1 : 0;
                const bool used = ly >= R0 && ly <= TH - 1 + R1 && lx >= S0 && lx <= TWI - 1 + S1;
                loff[k] = (px < NPX && lx < LVALID && used) ? ((ry * p.Ws + rx) * 32 + slot * 8) * 2 + (imgb ? (int)p.in_img_stride * 2 : 0) : OOB;
                if constexpr (POLY) {          // the tile's dilation scales the pixel part: voff = lpix * d + slot (setup)
                    lpix[k] = (px < NPX && lx < LVALID) ? (ly * p.fullW + lx) * 64 : -1;
                    loff[k] = slot * 16;
                }
            }
        }
        const int wvoff = lane * 16;
        int voff[KQ];
        const char* in_tile = nullptr;
        const char* w_tile = nullptr;
        // (always_inline: a lambda left as a call keeps the per-lane offset arrays it captures in scratch memory -- the S9 instantiation, whose
        //  issue path is the longest, ran 11 x slower that way: profiles/r2/kernel_experiments.txt 13)
        auto setup = [&](int jj) __attribute__((always_inline)) {
            int kg, n, ty0, tx0, dl = 1;
            if constexpr (POLY) decode_poly(jj, kg, n, ty0, tx0, dl);
            else decode(jj, kg, n, ty0, tx0);
            const long n0 = PAIR ? 2L * n : n;                 // PAIR: n is the pair; image 2n + 1 lies one image stride behind (loff)
            const bool no_b = PAIR && 2 * n + 1 >= p.N;        // an odd batch's last pair has no second image: its pieces stay zero
            in_tile = (const char*)(p.in + n0 * p.in_img_stride) + ((long)((ty0 - 1) >> p.up) * p.Ws + ((tx0 >> p.up) - 1)) * 64;
            w_tile = (const char*)p.wpk + (long)kg * p.nchunks * W_BYTES;
#pragma unroll
            for (int k = 0; k < KQ; ++k) voff[k] = loff[k];
            if constexpr (POLY) {
                const int d = dl, dd = d * d;
                const int nn = n / dd, ph = n - nn * dd, py = ph / d, px = ph - py * d;
                const int Hp = (p.fullH - py + d - 1) / d, Wp = (p.fullW - px + d - 1) / d;      // this component's extent
                in_tile = (const char*)(p.in + (long)nn * p.in_img_stride) + (((long)(ty0 - 1) * d + py) * p.fullW + (long)(tx0 - 1) * d + px) * 64;
                const bool edge = ty0 == 0 || ty0 + TH + 1 > Hp || tx0 == 0 || tx0 + TW + 1 > Wp;
#pragma unroll
                for (int k = 0; k < KQ; ++k) {
                    bool ok = lpix[POLY ? k : 0] >= 0;
                    if (edge) {
                        const int pxi = (lw + NLW * k) * 16 + (lane >> 2);
                        const int ly = pxi / LWP, lx = pxi - ly * LWP;
                        const int Y = ty0 - 1 + ly, X = tx0 - 1 + lx;
                        ok = ok && Y >= 0 && Y < Hp && X >= 0 && X < Wp;
                    }
                    voff[k] = ok ? lpix[POLY ? k : 0] * d + loff[k] : OOB;
                }
                return;
            }
            if constexpr (CV) {
                const int uy = ty0 - 1 + p.cv_h1, ux = tx0 - 1 + p.cv_w1;                 // first halo pixel, shifted by one cell so that it is >= 0
                const int qy = uy / p.cv_h1, qx = ux / p.cv_w1;
                const int cyA = qy - 1, yA = uy - qy * p.cv_h1, cxA = qx - 1, xA = ux - qx * p.cv_w1;
                const int nA = cyA * p.cv_gx + cxA;
                if (cyA >= 0 && cxA >= 0 && cxA < p.cv_gx && nA < p.N && yA + LH <= p.H && xA + LVALID <= p.W) {
                    in_tile = (const char*)(p.in + (long)nA * p.in_img_stride) + ((long)yA * p.Ws + xA) * 64;       // inside one image: plain path
                    return;
                }
                in_tile = (const char*)p.in;                                              // offsets from the first image's origin, per lane
#pragma unroll
                for (int k = 0; k < KQ; ++k) {
                    const int px = (lw + NLW * k) * 16 + (lane >> 2);
                    const int ly = px / LWP, lx = px - ly * LWP;
                    int y = yA + ly, cy = cyA;
                    if (y >= p.cv_h1) { y -= p.cv_h1; ++cy; }
                    int x = xA + lx, cx = cxA;
                    if (x >= p.cv_w1) { x -= p.cv_w1; ++cx; }
                    const int nn = cy * p.cv_gx + cx;
                    const bool ok = loff[k] != OOB && y < p.H && x < p.W && cy >= 0 && cx >= 0 && cy < p.cv_gy && cx < p.cv_gx && nn < p.N;
                    const int slot = (lane & 3) ^ (((px >> 2) & 1) << 1);
                    voff[k] = ok ? (((nn * p.H + y) * p.W + x) * 32 + slot * 8) * 2 : OOB;
                }
                return;
            }
            if constexpr (S9) {          // displaced reads reach 4 pixels beyond the tile: such tiles derive their offsets per chunk (issue)
                s9_ty0 = ty0; s9_tx0 = tx0; s9_n = n;
                s9_edge = ty0 < 4 || ty0 + TH + 4 > p.H || tx0 < 4 || tx0 + TW + 4 > p.W;
                return;
            }
            if constexpr (S2) {          // cells (ty0 - 1 .. ty0 + TH) x (tx0 - 1 .. tx0 + TW) of both phases: source rows 2 ty0 - 3 .. 2 (ty0 + TH)
                s9_ty0 = ty0; s9_tx0 = tx0; s9_n = (int)n0;
                s9_edge = PAIR || 2 * ty0 < 3 || 2 * (ty0 + TH) >= p.Hs || 2 * tx0 < 3 || 2 * (tx0 + TW) >= p.Ws;
                in_tile = (const char*)(p.in + n0 * p.in_img_stride) + ((long)(2 * ty0 - 3) * p.Ws + (2 * tx0 - 3)) * 64;
                if (S2PRE && s9_edge) {
                    // a tile that touches the image border: the offsets of phase (0, 0) from the image origin and one validity bit per (phase, piece),
                    // derived once per tile -- issue_to then selects; (deriving them per chunk cost the loaders ~0.7 us per step, and in the UNet's
                    // 16 x 16 .. 64 x 64 grids every tile is such a tile: profiles/r3/ablate_unet.txt)
                    s2_m0 = s2_m1 = s2_m2 = s2_m3 = 0;
#pragma unroll
                    for (int k = 0; k < KQ; ++k) {
                        const int px = (lw + NLW * k) * 16 + (lane >> 2);
                        const int ly = px / LWP;
                        int lx = px - ly * LWP;
                        const bool imgb = PAIR && lx >= 18;
                        if (imgb) lx -= 18;
                        const int Yb = 2 * (ty0 - 1 + ly) - 1, Xb = 2 * (tx0 - 1 + lx) - 1;
                        s2_off[S2PRE ? k : 0] = (Yb * p.Ws + Xb) * 64 + (loff[k] - (2 * ly * p.Ws + 2 * lx) * 64);        // (loff carries the second image's stride)
                        const bool y0 = Yb >= 0 && Yb < p.Hs, y1 = Yb + 1 >= 0 && Yb + 1 < p.Hs, x0 = Xb >= 0 && Xb < p.Ws, x1 = Xb + 1 >= 0 && Xb + 1 < p.Ws;
                        const bool lv = loff[k] != OOB && !(imgb && no_b);
                        s2_m0 |= (unsigned)(lv && y0 && x0) << k; s2_m1 |= (unsigned)(lv && y0 && x1) << k;
                        s2_m2 |= (unsigned)(lv && y1 && x0) << k; s2_m3 |= (unsigned)(lv && y1 && x1) << k;
                    }
                }
                return;
            }
            if (PAIR || ty0 == 0 || ty0 + TH + 1 > p.H || tx0 == 0 || tx0 + TW + 1 > p.W) {
#pragma unroll
                for (int k = 0; k < KQ; ++k) {
                    const int px = (lw + NLW * k) * 16 + (lane >> 2);
                    const int ly = px / LWP;
                    int lx = px - ly * LWP;
                    const bool imgb = PAIR && lx >= 18;
                    if (imgb) lx -= 18;
                    const int Y = ty0 - 1 + ly, X = tx0 - 1 + lx;
                    if (Y < 0 || Y >= p.H || X < 0 || X >= p.W || (imgb && no_b)) {
                        // reflection padding: the ring of pixels one step outside the image mirrors the pixel one step inside; farther
                        // out (tile padding of a ragged frame) only feeds outputs that are never stored
                        // (reflect 2 = nn.ReplicationPad2d(1): the ring repeats the border pixel)
                        if (p.reflect && loff[k] != OOB && Y >= -1 && Y <= p.H && X >= -1 && X <= p.W) {
                            const int in1 = p.reflect == 2 ? 0 : 1, in2 = p.reflect == 2 ? 1 : 2;
                            const int Yr = Y < 0 ? in1 : (Y >= p.H ? p.H - in2 : Y), Xr = X < 0 ? in1 : (X >= p.W ? p.W - in2 : X);
                            voff[k] = loff[k] + ((Yr - Y) * p.Ws + (Xr - X)) * 64;
                        } else {
                            voff[k] = OOB;
                        }
                    }
                }
            }
        };
        // what: 1 input pieces, 2 weight pieces, 3 both; st_i / st_w: LDS destinations; wsrc: the chunk's weight panel
        auto issue_to = [&](int c, char* st_i, char* st_w, const char* wsrc, int what) __attribute__((always_inline)) {
#if defined(__HIP_DEVICE_COMPILE__)
            const char* src = in_tile + c * p.in_gbytes;
            if constexpr (SPLIT) {               // virtual chunk -> (part, channel group): parts 0 and 2 read the hi slab, part 1 the lo slab
                const int part = c >= 2 * p.ncg ? 2 : (c >= p.ncg ? 1 : 0);
                src = in_tile + (c - part * p.ncg) * p.in_gbytes + (part == 1 ? p.in_lo_bytes : 0);
            }
            if constexpr (S9) {
                const int sub = c / p.ncg, cg = c - sub * p.ncg;
                const int sy = p.s9v ? 3 * (sub - 1) : 3 * (sub / 3 - 1), sx = p.s9v ? 0 : 3 * (sub % 3 - 1);
                if (!s9_edge) {
                    src = in_tile + cg * p.in_gbytes + ((long)sy * p.Ws + sx) * 64;        // every displaced pixel is inside the image
#pragma unroll
                    for (int k = 0; k < KQ; ++k) voff[k] = loff[k];
                } else {                                                                  // offsets from the image origin, per lane
                    src = (const char*)(p.in + (long)s9_n * p.in_img_stride) + cg * p.in_gbytes;
#pragma unroll
                    for (int k = 0; k < KQ; ++k) {
                        const int px = (lw + NLW * k) * 16 + (lane >> 2);
                        const int ly = px / LWP, lx = px - ly * LWP;
                        int Y = s9_ty0 - 1 + ly + sy, X = s9_tx0 - 1 + lx + sx;
                        if (p.reflect) {                                                  // ReflectionPad2d(3)
                            Y = Y < 0 ? -Y : (Y >= p.H ? 2 * p.H - 2 - Y : Y);
                            X = X < 0 ? -X : (X >= p.W ? 2 * p.W - 2 - X : X);
                        }
                        const bool ok = loff[k] != OOB && Y >= 0 && Y < p.H && X >= 0 && X < p.W;
                        voff[k] = ok ? (Y * p.Ws + X) * 64 + (loff[k] - (ly * p.Ws + lx) * 64) : OOB;
                    }
                }
            }
            if constexpr (S2) {
                const int ph = c / p.ncg, cg = c - ph * p.ncg, pa = ph >> 1, pb = ph & 1;
                if (!s9_edge) {
                    src = in_tile + cg * p.in_gbytes + ((long)pa * p.Ws + pb) * 64;
#pragma unroll
                    for (int k = 0; k < KQ; ++k) voff[k] = loff[k];
                } else if constexpr (S2PRE) {                                             // offsets from the image origin, per lane (setup)
                    src = (const char*)(p.in + (long)s9_n * p.in_img_stride) + cg * p.in_gbytes;
                    const int shift = (pa * p.Ws + pb) * 64;
                    const unsigned m = ph == 0 ? s2_m0 : ph == 1 ? s2_m1 : ph == 2 ? s2_m2 : s2_m3;
#pragma unroll
                    for (int k = 0; k < KQ; ++k) voff[k] = ((m >> k) & 1u) ? s2_off[S2PRE ? k : 0] + shift : OOB;
                } else {                                                                  // (24-row tiles: per chunk, as before round 3)
                    src = (const char*)(p.in + (long)s9_n * p.in_img_stride) + cg * p.in_gbytes;
#pragma unroll
                    for (int k = 0; k < KQ; ++k) {
                        const int px = (lw + NLW * k) * 16 + (lane >> 2);
                        const int ly = px / LWP, lx = px - ly * LWP;
                        const int Y = 2 * (s9_ty0 - 1 + ly) + pa - 1, X = 2 * (s9_tx0 - 1 + lx) + pb - 1;
                        const bool ok = loff[k] != OOB && Y >= 0 && Y < p.Hs && X >= 0 && X < p.Ws;
                        voff[k] = ok ? (Y * p.Ws + X) * 64 + (loff[k] - (2 * ly * p.Ws + 2 * lx) * 64) : OOB;
                    }
                }
            }
            const __amdgpu_buffer_rsrc_t ri = __builtin_amdgcn_make_buffer_rsrc((void*)src, 0, 0x7fffffff, 0x00020000);
            const __amdgpu_buffer_rsrc_t rw = __builtin_amdgcn_make_buffer_rsrc((void*)wsrc, 0, W_BYTES, 0x00020000);
#ifdef INNFER_ABLATE
            if (p.abl & 2) what &= ~2;                                   // abl 2: no weight pieces, abl 4: no input pieces
            if (p.abl & 4) what &= ~1;
#endif
            if (what & 2) {
#pragma unroll
                for (int k = 0; k < KW; ++k) {
                    const int jq = lw + NLW * k;
                    if (jq < WQ)
                        __builtin_amdgcn_raw_ptr_buffer_load_lds(rw, (__attribute__((address_space(3))) void*)(st_w + jq * 1024), 16, wvoff, jq * 1024, 0, 0);
                }
            }
            if (what & 1) {
#pragma unroll
                for (int k = 0; k < KQ; ++k) {
                    const int q = lw + NLW * k;
                    if (q < NQ)
                        __builtin_amdgcn_raw_ptr_buffer_load_lds(ri, (__attribute__((address_space(3))) void*)(st_i + q * 1024), 16, voff[k], 0, 0, INNFER_IN_AUX);
                }
            }
#else
            (void)c; (void)st_i; (void)st_w; (void)wsrc; (void)what; (void)wvoff; (void)KW; (void)in_tile; (void)w_tile; (void)s9_ty0; (void)s9_tx0; (void)s9_n; (void)s9_edge; (void)s2_off; (void)s2_m0; (void)s2_m1; (void)s2_m2; (void)s2_m3;
#endif
        };
        auto issue = [&](int c, int stage) __attribute__((always_inline)) {
            const int cg = RLDS ? (c + 2 >= p.nchunks ? c + 2 - p.nchunks : c + 2) : c;      // RLDS: groups 2, 3, .., 0, 1 -- the residual's two groups last
            issue_to(cg, smem + stage * STAGE, smem + stage * STAGE + IN_BYTES, w_tile + (long)cg * W_BYTES, 3);
        };
        if constexpr (NSI == 3) {
            // ---- ring of three input slots + two weight slots: the input cursor runs two chunks ahead of the consumers, the weight cursor one ----
            char* const wring = smem + 3 * IN_BYTES;
            const int my_in = (NQ - lw + NLW - 1) / NLW;                 // input pieces THIS wave issues per chunk (KQ or KQ - 1)
            auto wait_all_but_in = [&](bool pending) {                    // everything older than the youngest chunk's input pieces has landed
                if (!pending) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                else if (my_in == KQ) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(KQ) : "memory");
                else asm volatile("s_waitcnt vmcnt(%0)" ::"n"(KQ - 1) : "memory");
            };
            if constexpr (UP4) {
                // tile T's groups 0 / 1 live in slots (2T) % 3 and (2T + 1) % 3 for its eight steps; weights: panel (g + 1) % 8 one step ahead
                int jt_i = j0, base = 0;                                  // base: slot of the current tile's group 0
                setup(jt_i);
                issue_to(0, smem, wring, (const char*)p.wpk, 3);
                issue_to(1, smem + IN_BYTES, nullptr, nullptr, 1);
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                asm volatile("s_barrier" ::: "memory");
                for (int g = 0; g < G; ++g) {
                    const int st8 = g & 7;
                    bool pending = false;
                    if (g + 1 < G) issue_to(0, nullptr, wring + ((g + 1) & 1) * W_BYTES, (const char*)p.wpk + (long)((g + 1) & 7) * W_BYTES, 2);
                    if (st8 == 0 && g + 8 < G) {                          // next tile's group 0 -> the slot the previous tile's group 1 has left
                        jt_i += slots; setup(jt_i);
                        const int fs = base == 0 ? 2 : base - 1;          // (base + 2) % 3
                        issue_to(0, smem + fs * IN_BYTES, nullptr, nullptr, 1);
                        pending = true;
                    }
                    if (st8 == 7 && g + 1 < G) {                          // next tile's group 1 -> this tile's group-0 slot (last read in step 6)
                        issue_to(1, smem + base * IN_BYTES, nullptr, nullptr, 1);
                        pending = true;
                        base = base == 0 ? 2 : base - 1;
                    }
                    wait_all_but_in(pending);
                    asm volatile("s_barrier" ::: "memory");
                }
                return;
            }
            int jt_i = j0, c_i = 0;                                       // input cursor (setup() keeps its tile's offsets in voff / in_tile)
            int jt_w = j0, c_w = 0, kg_w;                                 // weight cursor
            { int n_, ty_, tx_; decode(jt_w, kg_w, n_, ty_, tx_); }
            setup(jt_i);
            issue_to(0, smem, wring, (const char*)p.wpk + (long)kg_w * p.nchunks * W_BYTES, 3);
            bool pending = false;
            if (G > 1) {
                if (++c_i == p.nchunks) { c_i = 0; jt_i += slots; setup(jt_i); }
                issue_to(c_i, smem + IN_BYTES, nullptr, nullptr, 1);
                pending = true;
            }
            wait_all_but_in(pending);
            asm volatile("s_barrier" ::: "memory");
            int slot = 2;                                                 // (g + 2) % 3
            for (int g = 0; g < G; ++g) {
                pending = false;
                if (g + 1 < G) {
                    if (++c_w == p.nchunks) { c_w = 0; jt_w += slots; int n_, ty_, tx_; decode(jt_w, kg_w, n_, ty_, tx_); }
                    issue_to(0, nullptr, wring + ((g + 1) & 1) * W_BYTES, (const char*)p.wpk + ((long)kg_w * p.nchunks + c_w) * W_BYTES, 2);
                }
                if (g + 2 < G) {
                    if (++c_i == p.nchunks) { c_i = 0; jt_i += slots; setup(jt_i); }
                    issue_to(c_i, smem + slot * IN_BYTES, nullptr, nullptr, 1);
                    pending = true;
                }
                slot = slot == 2 ? 0 : slot + 1;
                wait_all_but_in(pending);
                asm volatile("s_barrier" ::: "memory");
            }
            return;
        }
        int jt = j0, c = 0;
        setup(jt);
        issue(0, 0);
        if constexpr (FUSE) {                 // the last conv's four A fragments (4 KB) behind the two stages, once per workgroup
#if defined(__HIP_DEVICE_COMPILE__)
            const __amdgpu_buffer_rsrc_t rf = __builtin_amdgcn_make_buffer_rsrc((void*)p.fl_w, 0, 4096, 0x00020000);
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rf, (__attribute__((address_space(3))) void*)(smem + L::TAIL + lw * 1024), 16, lane * 16, lw * 1024, 0, 0);
#endif
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        asm volatile("s_barrier" ::: "memory");
        int cc = 0;                            // FUSE: the chunk the consumers work on in step g
        for (int g = 0; g < G; ++g) {
            PCT(l0);
            if (g + 1 < G) {
                if (++c == p.nchunks) { c = 0; jt += slots; setup(jt); }
                issue(c, (g + 1) & 1);
                PCT(l1);
#ifdef INNFER_ABLATE
                // abl 32 (with 8: no MFMA phase): FREE-RUNNING loaders -- the ceiling of this kernel's own access pattern (piece shapes, halo tiles, slab
                // stores) without the per-chunk coupling to the consumers: a loader waits only for the chunk issued BEFORE the one it has just issued (one
                // chunk always in flight) and meets the consumers once per tile (profiles/r4/access_pattern_ceiling.txt)
                if (p.abl & 32) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(KQ + KW - 2) : "memory");
                else
#endif
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                PCT(l2);
                if (lw == 0) { PCACC(3, l1, l0); PCACC(4, l2, l1); }
            }
#ifdef INNFER_ABLATE
            if ((p.abl & 32) && (g + 1) % p.nchunks != 0) continue;          // free-running: one barrier per tile
#endif
            PCT(l3);
            if constexpr (FUSE) {             // a tile's last chunk: the consumers' fused epilogue meets at two more barriers
                if (++cc == p.nchunks) {
                    cc = 0;
                    asm volatile("s_barrier" ::: "memory");
                    asm volatile("s_barrier" ::: "memory");
                }
            }
            asm volatile("s_barrier" ::: "memory");
            PCT(l4);
            if (lw == 0) PCACC(5, l4, l3);
        }
        return;
    }
