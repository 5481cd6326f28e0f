// The tap masks and mode flags that key an instantiation of conv3x3_pc (its `int TMF` template argument) -- the ONE place a value is written.
// TMF = tap mask | mode flags.  Every flag is compile-time: an instantiation contains none of the other modes' code.  The argument stays a plain int
// (the mangled kernel names carry its value).  Included by common.h inside namespace innfer.  Not a stand-alone header.

// ---- tap masks: bits 0..8, bit r * 3 + s = tap (r, s) of the 3x3 lattice; the weight panel holds the set taps in that order ----
constexpr int TAPS_3X3   = 0x1FF;   // all nine taps: the 3x3 conv (software-pipelined fragment reads); also the mask of the tap field itself
constexpr int TAPS_1X1   = 0x010;   // the centre tap: a 1x1 conv (panels from conv_pack_1x1)
constexpr int TAPS_COL   = 0x092;   // the centre column: a 7 x 1 column conv as three vertically displaced 3-tap blocks (S9, conv_pack7v)
constexpr int TAPS_PHASE = 0x01B;   // taps {0, 1}^2: one output phase of ConvTranspose2d(k, 2, 1) per channel group, on a lattice shifted by the phase
constexpr int TAPS_S2    = 0x1B0;   // taps {1, 2}^2: Conv2d(4, 2, 1) on the space-to-depth source (always with PC_S2)

// ---- mode flags ----
constexpr int PC_S2    = 0x200;       // the stride-2 gather loader: chunk = (source phase, channel group)
constexpr int PC_PAIR  = 0x400;       // grids <= 16 wide: a tile row is two images side by side (four-tap kernels)
constexpr int PC_PFX   = 0x800;       // (1x1) the operand of chunk k is LeakyReLU(running sum of chunks 0 .. k): PPON's c2
constexpr int PC_STATS = 0x1000;      // partial norm statistics out of the epilogue (epilogue_stats)
constexpr int PC_SPLIT = 0x2000;      // fp32-accurate mode: (hi, lo) fp16 operand pairs, 3 * ncg virtual chunks
constexpr int PC_FUSE  = 0x20000;     // HR_conv0 -> conv_last: the network's last conv inside this conv's epilogue (4 KB LDS tail: its panel)
constexpr int PC_RLDS  = 0x40000;     // the dense block's residual (= input groups 0, 1) from the live LDS stage; chunk order 2, 3, .., 0, 1
constexpr int PC_SGATE = 0x80000;     // out = v * sigmoid(W v + b), a 1x1 conv of the conv's own result, in the epilogue (PAN's pixel attention)
constexpr int PC_BRELU = 0x100000;    // the pixel operand is max(x, 0) of the stored slab, applied as a fragment leaves LDS
constexpr int PC_UP4   = 0x200000;    // all four phases of a 2x transposed conv in one visit of a tile (1 KB LDS tail: the phases' biases)
constexpr int PC_ROWP  = 0x400000;    // the plane row order of the 64-channel output groups (toff_slab)
constexpr int PC_PSH   = 0x800000;    // nn.PixelShuffle(2) as the store: phase-major plane-order panels (conv_pack_shuffle2)
constexpr int PC_PRELU = 0x1000000;   // act 8: per-channel slopes in the slab epilogue (LDS tail: 256 B of slopes per consumer wave)
constexpr int PC_GRID2 = 0x2000000;   // the eight consumer waves as a 2 x 4 grid (32-channel half x 4-row group; RPW 4, NT 2) over the same 16 x 32 tile and 64-row panels
constexpr int PC_MISH  = 0x8000000;   // act 11 in the slab epilogue: Mish, f * tanh(softplus(f)) (one hardware exponential + reciprocal per value; RealPLKSR's DCCM)
constexpr int PC_GELU  = 0x10000000;  // act 12 in the slab epilogue of the 64-output 1x1 conv: the exact (erf) GELU (SwinIR's mlp.fc1)
constexpr int PC_SPAN  = 0x4000000;   // act 9 / 10 in the slab epilogue: SiLU, and SPAN's gate (f + res1) * (sigmoid(f) - 0.5) (one hardware exponential + reciprocal per value)

// "tap mask + every flag below X": what an instantiation of mode X is compared against when the lower flags must all be clear
constexpr int PC_BELOW_FUSE  = PC_FUSE - 1;
constexpr int PC_BELOW_RLDS  = PC_RLDS - 1;
constexpr int PC_BELOW_SGATE = PC_SGATE - 1;
constexpr int PC_BELOW_UP4   = PC_UP4 - 1;
