"""Every form of conv3x3_pc, alone, against float64 within one fp16 rounding (needs an MI355X: `pytest -m gpu`).

conv_launch (csrc/conv3x3.hip) chooses among some thirty instantiations of one kernel body; ABI 121 (innfer_conv_args.conv1x1 / prefix_lrelu / d_gate_packed / in_relu /
conv7x7 / out_planar / planar_phases / outm, act 3 / 6) makes each of them a single launch.  The bound, the references and the roundings they mirror are in
tests/_conv_ref.py (assert_within_fp16_rounding):

    |got - ref| <= ulp16(max(|ref|, |got|)) / 2 + 8 e32 + extra          (fp32 results of >= 4096 values: 8 e32 + extra)

Shapes: the smallest at which a mechanism can fail.  Tiles are 24 x 32 (32-output and planar kernels) and 16 x 32 (64-output, 1x1, phase kernels); the grid is
min(tiles, 256) workgroups, so a workgroup meets a second tile -- the next-tile prefetch, the wrap of the three-slot ring -- beyond 256 tiles (241 x 833, 273 x 513).
Every output lies between guard bands and, in a wider slab, beside foreign groups: all of them must keep their fill value.

Measured on the MI355X (largest e32 of the family's cases; worst err / bound over every element of every case):

    family                                               e32        worst err / bound
    planar 3x3, K <= 4 (fast path)                       5.3e-07    0.994
    planar 3x3, K = 5 / 16 (generic loop)                5.5e-07    0.998
    planar 3x3, reflection padding                       1.6e-06    0.993
    planar 3x3, K = 32                                   6.4e-07    0.997
    planar 3x3, K = 64 (launch_t)                        6.9e-07    0.994
    two-workgroup kernel, slab K = 16                    5.0e-07    0.994
    two-workgroup kernel, planar K = 16, residuals       4.1e-07    0.994   (fp32 stores: 0.046 of 8 e32)
    two-workgroup kernel, planar K = 32, residuals       5.9e-07    0.993   (fp32 stores: 0.038 of 8 e32)
    planar uint8 image                                   5.4e-07    7e-5 of the codes differ (cap 1e-2), each by one, next to a boundary
    planar phase scatter                                 8.5e-07    0.998
    planar phase scatter + in_relu                       5.8e-07    0.995
    planar 7x7                                           1.3e-06    0.994
    planar 7x7, reflect                                  1.3e-06    0.994
    1x1, 32 outputs                                      1.5e-06    0.996
    1x1, 32 outputs, PA gate                             1.5e-06    0.990
    1x1, 64 outputs                                      1.9e-06    0.996
    1x1, 64 outputs, PA gate                             1.9e-06    0.990
    1x1, running-sum operand                             2.6e-06    0.996
    self gate                                            7.1e-07    0.790
    self gate, upsampled input                           6.5e-07    0.772
    up-conv phases                                       1.6e-06    0.993
    sweep: 3x3 32 outputs                                4.6e-07    0.996
    sweep: 3x3 64 outputs                                5.0e-07    0.993
    sweep: 3x3 upsampled input                           4.6e-07    0.993
    sweep: PixelShuffle(2) store                         5.0e-07    0.992
    sweep: Conv2d(4, 2, 1)                               6.4e-07    0.990
    sweep: ConvTranspose2d(k, 2, 1)                      1.2e-06    0.987
    sweep: 7x1 column conv                               4.8e-07    0.993
    sweep: dilated 3x3                                   4.5e-07    0.994

The fp16 stores sit at 0.99 because the storage rounding alone fills the bound (fp16(float32 conv) on the CPU reaches the same figures, tests/test_conv_forms_cpu.py);
the device's own share shows where nothing is rounded: the fp32 stores of >= 4096 values reach 0.34 of 8 e32 (a 4 x 4 image of the 7x7 conv, whose 48 values
understate e32, would reach 0.75: such cases keep the rounding term); with tanh / sigmoid they reach 0.19 of 8 e32 + 2^-21, so the hardware tanh / sigmoid stay
within about 1e-7, as csrc/common.h says.
The fp32-accurate forms: planar 3x3 max |err| 1.15e-6, 1x1 6.0e-7 (bound 3e-6).  Up-conv phases against the nine-tap weights' float64 result: 1.1e-3 (reported only).

tanh / sigmoid on the hardware exponential and reciprocal are allowed 2^-21 each (_conv_ref.TRANS, derived there); the uint8 image is compared in codes
(_conv_ref.assert_image_codes); the fp32-accurate forms keep the fp32 mode's 3e-6 (tests/test_gpu_fp32_mode.py).
"""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _conv_ref as R
from _conv_ref import Case

pytestmark = pytest.mark.gpu

FILL, FILL_U8, GUARD = -3.0, 171, 4096
S24 = [(1, 1, 1), (1, 24, 32), (1, 25, 33), (1, 50, 70), (3, 37, 45)]          # tiles of 24 x 32
S16 = [(1, 1, 1), (1, 16, 32), (1, 17, 33), (1, 50, 70), (3, 37, 45)]          # tiles of 16 x 32
MANY24, MANY16 = (1, 241, 833), (1, 273, 513)                                  # 11 x 27 = 297 and 18 x 17 = 306 tiles: more than the 256 workgroups


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


# ------------------------------------------------------------------------------------------------ one launch
def _pack(c, plane_rows=0):
    import innfer_amd.lib as L
    lib = L.lib
    _, w, _ = R.data(c)
    K, Cc = c.K, c.C
    if c.form == "phases":
        w, K = R.phase_conv3x3_weights(w), 4 * c.K
    wc = np.ascontiguousarray(w.numpy(), dtype=np.float32)
    size, fn = {
        "3x3": (lib.innfer_conv3x3_packed_bytes(K, Cc), lambda p: lib.innfer_pack_conv3x3_rows(wc.ctypes.data, K, Cc, plane_rows, p)),
        "shuffle": (lib.innfer_conv3x3_packed_bytes(K, Cc), lambda p: lib.innfer_pack_conv3x3(wc.ctypes.data, K, Cc, p)),
        "dil": (lib.innfer_conv3x3_packed_bytes(K, Cc), lambda p: lib.innfer_pack_conv3x3(wc.ctypes.data, K, Cc, p)),
        "phases": (lib.innfer_conv3x3_packed_bytes(K, Cc), lambda p: lib.innfer_pack_conv3x3(wc.ctypes.data, K, Cc, p)),
        "1x1": (lib.innfer_conv1x1_packed_bytes(K, Cc), lambda p: lib.innfer_pack_conv1x1(wc.ctypes.data, K, Cc, p)),
        "7x7": (lib.innfer_conv7x7_packed_bytes(K, Cc), lambda p: lib.innfer_pack_conv7x7(wc.ctypes.data, K, Cc, p)),
        "upph": (lib.innfer_convt2x_packed_bytes(K, Cc), lambda p: lib.innfer_pack_up2x_phases(wc.ctypes.data, K, Cc, plane_rows, p)),
        "t2x": (lib.innfer_convt2x_packed_bytes(K, Cc), lambda p: lib.innfer_pack_convt2x_rows(wc.ctypes.data, K, Cc, c.k, plane_rows, p)),
        "s2k4": (lib.innfer_conv4x4s2_packed_bytes(K, Cc), lambda p: lib.innfer_pack_conv4x4s2(wc.ctypes.data, K, Cc, p)),
        "7x1": (lib.innfer_conv7x1_packed_bytes(K, Cc), lambda p: lib.innfer_pack_conv7x1(wc.ctypes.data, K, Cc, p)),
    }[c.form]
    assert size > 0
    packed = np.zeros(size, dtype=np.uint8)
    L.check(fn(packed.ctypes.data))
    return packed


def _run(dev, c, out="slab", act=0, res1=None, s1=1.0, res2=None, s2=1.0, out_groups=None, out_off=0, rows=None, plane_rows=0, gate=False, expect=0, **fields):
    """One launch of the case through innfer_conv3x3_f16.  out: "slab" -> [N, channels, Ho, Wo] fp16 of the WHOLE output slab (every group); "f16" / "f32" -> the planar
    tensor; "u8" -> the image [N, H, W, K].  The output lies between guard bands that must keep their fill, like everything a refused launch (expect != 0) was given."""
    import innfer_amd.lib as L
    x, _, b = R.data(c)
    N, Cc, Hs, Ws = x.shape
    xin = R.to_slab(x, Cc // 32 + 1).to(dev)                     # (a junk group behind the input: a chunk too many would show)
    d_packed = torch.from_numpy(_pack(c, plane_rows)).to(dev)
    reps = 4 if c.form in ("phases", "upph", "t2x") else 1     # the phase forms take the biases once per phase
    bias = torch.zeros((reps * c.K + 63) // 64 * 64)
    bias[:reps * c.K] = b.repeat(reps)
    d_bias = bias.to(dev)
    two = c.form in ("upph", "t2x", "shuffle") or (c.form == "phases")
    Ho, Wo = (2 * c.H, 2 * c.W) if two else (c.H, c.W)
    Kout = c.K // 4 if c.form == "shuffle" else c.K
    if out == "slab":
        groups = out_groups or max(Kout, 32) // 32
        numel, dt, fill = groups * N * Ho * Wo * 32, torch.float16, FILL
    else:
        numel, dt, fill = N * Kout * Ho * Wo, {"f16": torch.float16, "f32": torch.float32, "u8": torch.uint8}[out], FILL_U8 if out == "u8" else FILL
    buf = torch.full((numel + 2 * GUARD,), fill, dtype=dt, device=dev)
    a = L.ConvArgs()
    a.d_in, a.in_group_stride, a.C = xin.data_ptr(), N * Hs * Ws * 32, Cc
    a.d_packed, a.d_bias = d_packed.data_ptr(), d_bias.data_ptr()
    a.d_out, a.out_group_stride, a.out_ch_off, a.K = buf.data_ptr() + GUARD * buf.element_size(), N * Ho * Wo * 32, out_off, c.K
    a.N, a.H, a.W, a.act, a.upsample2x = N, c.H, c.W, act, c.up
    a.reflect_pad, a.in_relu, a.plane_rows = c.reflect, c.in_relu, plane_rows
    a.conv1x1, a.prefix_lrelu, a.conv7x7 = int(c.form == "1x1"), c.prefix, int(c.form == "7x7")
    a.planar_phases = int(c.form == "phases")
    a.pixel_shuffle2, a.stride2_k4, a.column7 = int(c.form == "shuffle"), int(c.form == "s2k4"), int(c.form == "7x1")
    a.transposed2x = c.k if c.form == "t2x" else 4 if c.form == "upph" else 0
    a.dilation = c.dil if c.form == "dil" else 0
    a.out_planar = {"slab": 0, "f16": 1, "f32": 2, "u8": 3}[out]
    keep = []
    for name, r, sc in (("1", res1, s1), ("2", res2, s2)):
        if r is not None:
            rs = R.to_slab(F.pad(r, (0, 0, 0, 0, 0, -r.shape[1] % 32))).to(dev)      # (a residual of 16 channels lies in a 32-channel group)
            setattr(a, f"d_res{name}", rs.data_ptr()); setattr(a, f"res{name}_group_stride", N * Ho * Wo * 32); setattr(a, f"res{name}_scale", sc)
            keep.append(rs)
    if gate:
        wg, bg = R.gate_params(c)
        gp = np.zeros(2048, dtype=np.uint8)
        L.check(L.lib.innfer_pack_selfgate(np.ascontiguousarray(wg.numpy()).ctypes.data, gp.ctypes.data))
        keep += [torch.from_numpy(gp).to(dev), bg.to(dev)]
        a.d_gate_packed, a.d_gate_bias = keep[-2].data_ptr(), keep[-1].data_ptr()
    if rows:
        a.row_begin, a.row_end = rows
    for k, v in fields.items():
        assert hasattr(a, k), k
        setattr(a, k, v)
    rc = L.lib.innfer_conv3x3_f16(C.byref(a), None)
    torch.cuda.synchronize()
    raw = buf.cpu()
    if expect:
        assert rc == expect, (str(c), rc, L.last_error())
        assert bool((raw == fill).all()), f"{c}: a refused launch wrote to d_out"
        return None
    assert rc == 0, (str(c), fields, L.last_error())
    assert bool((raw[:GUARD] == fill).all()) and bool((raw[GUARD + numel:] == fill).all()), f"{c}: wrote outside the output"
    core = raw[GUARD:GUARD + numel]
    if out == "slab":
        return R.from_slab(core.reshape(groups, N, Ho, Wo, 32))
    if out == "u8":
        return core.reshape(N, Ho, Wo, Kout)
    return core.reshape(N, Kout, Ho, Wo)


def _check(dev, c, family, out="slab", act=0, outm=0, nres=0, s1=1.0, s2=1.0, out_off=0, out_groups=None, rows=None, **kw):
    """Launch, float64 reference of the same epilogue, the bound; foreign channels of the slab and rows outside the range keep the fill value."""
    y64, e32 = R.pre(c)
    r1 = R.residual(c, 1, y64.shape) if (nres >= 1 or act in (4, 5)) else None
    r2 = R.residual(c, 2, y64.shape) if nres >= 2 else None
    got = _run(dev, c, out, act=act, res1=r1, s1=s1, res2=r2, s2=s2, out_off=out_off, out_groups=out_groups, rows=rows, **({"outm": outm} if outm else {}), **kw)
    ref, ntrans = R.epilogue(y64, act, outm, r1.double() if r1 is not None else None, s1, r2.double() if r2 is not None else None, s2)
    if c.form == "shuffle":
        ref = F.pixel_shuffle(ref, 2)
    K = ref.shape[1]
    what = f"{c} {out} act {act}" + (f" outm {outm}" if outm else "") + (f" res {nres}" if nres else "") + (f" off {out_off}" if out_off else "") + (f" rows {rows}" if rows else "") + \
           "".join(f" {k}={v}" for k, v in kw.items())
    if out == "slab":
        assert bool((got[:, :out_off] == FILL).all()) and bool((got[:, out_off + K:] == FILL).all()), f"{what}: foreign channels of the slab were written"
        got = got[:, out_off:out_off + K]
    if rows:
        assert bool((got[:, :, :rows[0]] == FILL).all()) and bool((got[:, :, rows[1]:] == FILL).all()), f"{what}: rows outside the range were written"
        got, ref = got[:, :, rows[0]:rows[1]], ref[:, :, rows[0]:rows[1]]
    # an fp32 store has no storage rounding: the bound drops that term -- where the case has enough values (R.FEW) for its e32 to stand for the operation
    return R.assert_within_fp16_rounding(got, ref, e32, extra=ntrans * R.TRANS, what=what, family=family, rounding=out != "f32" or got.numel() < R.FEW)


# ------------------------------------------------------------------------------------------------ planar 3x3
@pytest.mark.parametrize("K", [1, 2, 3, 4, 5, 16])
def test_planar_3x3_k_le_16(dev, K):
    """launch_pc<3, 1, 4, OUT_NCHW>: the K <= 4 fast path and the generic loop (K = 5, 16 put values on lanes with lg != 0; every channel has its own bias, so a swapped
    channel cannot pass), fp16 and fp32 stores, act 0 / 1 / 2 / 3 / 6, outm 0 .. 4, a row range, the workgroups' second tile."""
    fam = "planar 3x3, K <= 4 (fast path)" if K <= 4 else "planar 3x3, K = 5 / 16 (generic loop)"
    sizes = S24 + ([MANY24] if K in (3, 16) else [])
    for i, (N, H, W) in enumerate(sizes):
        c = Case("3x3", N, 64 if K != 5 else 32, K, H, W, seed=K)
        for out in ("f16", "f32"):
            for act in ((0, 3) if (N, H, W) == MANY24 else (0, 1, 2, 3, 6)):
                _check(dev, c, fam, out, act=act)
        if i in (2, 4):
            for outm in (1, 2, 3, 4):
                _check(dev, c, fam, "f16", act=0, outm=outm)
            _check(dev, c, fam, "f32", act=1, outm=1)
            _check(dev, c, fam, "f32", act=3, outm=2)
        if H == 50:
            for out, act in (("f16", 0), ("f32", 3)):
                _check(dev, c, fam, out, act=act, rows=(8, 40))


@pytest.mark.parametrize("K", [3, 16])
def test_planar_3x3_reflection_padding(dev, K):
    for (N, H, W) in [(1, 2, 2), (1, 25, 33), (2, 50, 70)]:
        c = Case("3x3", N, 64, K, H, W, seed=20 + K, reflect=1)
        for out, act in (("f16", 0), ("f32", 0), ("f16", 3)):
            _check(dev, c, "planar 3x3, reflection padding", out, act=act)


@pytest.mark.parametrize("K", [32, 64])
def test_planar_3x3_k_32_and_64(dev, K):
    """K = 32: launch_pc<3, 2, 4, OUT_NCHW> (two 16-channel tiles per lane in the generic loop); K = 64: the old halo-tile kernel launch_t<2, 4, OUT_NCHW>, which has
    no tanh / sigmoid -- conv_launch refuses them, asserted here."""
    import innfer_amd.lib as L
    fam = f"planar 3x3, K = {K}"
    for (N, H, W) in S24 + [MANY24]:
        c = Case("3x3", N, 64, K, H, W, seed=30 + K)
        acts = (0, 1) if (N, H, W) == MANY24 else (0, 1, 2) if K == 64 else (0, 1, 2, 3, 6)
        for out in ("f16", "f32"):
            for act in acts:
                _check(dev, c, fam, out, act=act)
    c = Case("3x3", 1, 64, K, 25, 33, seed=30 + K)
    if K == 64:
        for act in (3, 6):
            _run(dev, c, "f16", act=act, expect=L.ERR_UNSUPPORTED)
    _run(dev, c, "f16", outm=1, expect=L.ERR_UNSUPPORTED)


@pytest.mark.parametrize("K,out", [(16, "slab"), (16, "planar"), (32, "planar")])
def test_two_workgroup_kernel_forms_without_another_test(dev, K, out):
    """conv3x3_mfma's instantiations beside <2, 4, OUT_NCHW> (the K = 64 case above) and <2, 4, OUT_SHUFFLE2> (the sweep's PixelShuffle(2) store): launch_t<4, 1, OUT_SLAB>
    (a slab of 16 channels: the other half of its 32-channel group keeps the fill), <4, 1, OUT_NCHW> and <4, 2, OUT_NCHW> (planar outputs WITH residuals; without one they
    run on conv3x3_pc).  Tiles are 16 x 32: both sizes are ragged on both axes, the second is a batch."""
    fam = f"two-workgroup kernel, {out} K = {K}"
    for (N, H, W) in [(1, 25, 33), (2, 37, 45)]:
        c = Case("3x3", N, 64, K, H, W, seed=50 + K + (out == "slab"))
        if out == "slab":
            for act in (0, 1, 2):
                _check(dev, c, fam, act=act)
        else:
            _check(dev, c, fam, "f16", act=1, nres=1, s1=0.2)
            _check(dev, c, fam, "f32", act=0, nres=2, s1=0.2, s2=0.5)
            _check(dev, c, fam, "f16", act=2, nres=2, s1=0.2, s2=0.5)


# ------------------------------------------------------------------------------------------------ the uint8 image
@pytest.mark.parametrize("K", [1, 3, 4])
def test_planar_uint8_image(dev, K):
    """tensor2np as the store (the K <= 4 uint8 twin of the fast path; with outm the generic loop's copy of it): codes against the float64 conv taken through the
    written-down steps (_conv_ref.image_codes: BGR / BGRA byte order), equal except one code next to a rounding boundary, at most 1 % of the values."""
    for (N, H, W) in [(1, 25, 33), (3, 37, 45), (1, 50, 70)] + ([MANY24] if K == 3 else []):
        for denorm in (0, 1):
            c = Case("3x3", N, 64, K, H, W, seed=40 + K, blo=-1.0 if denorm else 0.0)
            y64, e32 = R.pre(c)
            for r16 in (0, 1):
                got = _run(dev, c, "u8", out_denorm=denorm, out_round16=r16)
                R.assert_image_codes(got, y64, e32, denorm, r16, what=f"{c} denorm {denorm} round16 {r16}", family="planar uint8 image")
            if H == 25:         # clamp(0, 1) in front of the conversion: the generic loop's uint8 store
                got = _run(dev, c, "u8", out_denorm=denorm, out_round16=1, outm=4)
                R.assert_image_codes(got, y64.clamp(0, 1), e32, denorm, 1, what=f"{c} denorm {denorm} round16 1 outm 4", family="planar uint8 image")


# ------------------------------------------------------------------------------------------------ the phase scatter
@pytest.mark.parametrize("K", [3, 4])
def test_planar_phase_scatter(dev, K):
    """ConvTranspose2d(C, K, 4, 2, 1) as ONE 3x3 conv of 4 K phase channels whose epilogue scatters the phases (K = 3: the dedicated path; the operand ReLU is
    TMF 0x100000), against F.conv_transpose2d(relu(x)) in float64: ragged input grids put every phase on a tile edge."""
    for in_relu in (0, 1):
        for (N, H, W) in [(1, 1, 1), (1, 7, 9), (1, 24, 32), (1, 25, 33), (3, 37, 45)]:
            c = Case("phases", N, 64 if H != 7 else 128, K, H, W, seed=50 + K, in_relu=in_relu)
            for out, act in (("f16", 0), ("f16", 3), ("f32", 3)):
                _check(dev, c, "planar phase scatter" + (" + in_relu" if in_relu else ""), out, act=act)
    c = Case("3x3", 2, 64, 5, 25, 33, seed=59, in_relu=1)          # the operand ReLU without phases (same instantiation, generic loop)
    _check(dev, c, "planar phase scatter + in_relu", "f16", act=1)


# ------------------------------------------------------------------------------------------------ 7x7
@pytest.mark.parametrize("Cc,K", [(32, 3), (64, 3), (32, 16), (64, 16)])
def test_planar_7x7(dev, Cc, K):
    """The 7x7 conv as nine displaced 3x3 convs (S9, conv_pack7x7), zero and reflection padding; 4 x 4 is the smallest image ReflectionPad2d(3) takes."""
    for reflect in (0, 1):
        for (N, H, W) in [(1, 4, 4), (2, 7, 9), (2, 25, 33), (1, 50, 70)]:
            c = Case("7x7", N, Cc, K, H, W, seed=60 + K, reflect=reflect)
            for out, act in (("f16", 0), ("f16", 3), ("f32", 0)):
                _check(dev, c, "planar 7x7" + (", reflect" if reflect else ""), out, act=act)


# ------------------------------------------------------------------------------------------------ 1x1
@pytest.mark.parametrize("Cc,K", [(32, 32), (64, 32), (96, 32), (160, 32), (32, 64), (64, 64), (96, 64), (160, 64)])
def test_conv1x1(dev, Cc, K):
    """0x10 on the three-slot input ring (1, 2, 3 and 5 chunks: fewer and more than slots), 32- and 64-output tiles: act 0 / 1 / 2, the PA gate (act 4 / 5 times res1),
    one and two residuals, out_ch_off into a wider slab."""
    fam = f"1x1, {K} outputs"
    for (N, H, W) in S16 + ([MANY16] if Cc == 64 else []):
        c = Case("1x1", N, Cc, K, H, W, seed=70 + K + Cc)
        many = (N, H, W) == MANY16
        for act in ((1,) if many else (0, 1, 2)):
            _check(dev, c, fam, act=act)
        for act in ((4,) if many else (4, 5)):
            _check(dev, c, fam + ", PA gate", act=act)
        if not many:
            _check(dev, c, fam, act=0, nres=1, s1=0.2)
            _check(dev, c, fam, act=1, nres=2, s1=0.2, s2=0.5)
            if H in (17, 37):
                _check(dev, c, fam, act=1, out_off=32, out_groups=4)
                _check(dev, c, fam + ", PA gate", act=4, out_off=32, out_groups=4)


@pytest.mark.parametrize("Cc", [64, 256])
def test_conv1x1_running_sum_operand(dev, Cc):
    """0x810 (PPON's c2): the operand of input group g is fp16(LeakyReLU(group 0 + .. + group g)); the reference mirrors that one rounding (_conv_ref.operand) on inputs
    whose running sums are exact in fp32."""
    for (N, H, W) in S16 + ([MANY16] if Cc == 64 else []):
        c = Case("1x1", N, Cc, 64, H, W, seed=80 + Cc, prefix=1)
        for act in (0, 1):
            _check(dev, c, "1x1, running-sum operand", act=act)


def test_conv1x1_running_sum_operand_with_ppon_residuals(dev):
    """c2 exactly as PPON issues it: 1x1, 256 -> 64 on the running-sum operand, no activation, then its two residual stages (out * 0.2 + x, * 0.2 + the block's input)."""
    for (N, H, W) in S16:
        c = Case("1x1", N, 256, 64, H, W, seed=336, prefix=1)
        _check(dev, c, "1x1, running-sum operand, two residuals", act=0, nres=2, s1=0.2, s2=0.2)


@pytest.mark.parametrize("N,H,W", [(1, 1, 1), (1, 5, 3), (1, 25, 33), (2, 37, 45)])
def test_dilation_groups_one_launch(dev, N, H, W):
    """PPON's eight dilated convs (64 -> 32 each, rates 1 .. 8) as the ONE launch the network issues (dilation_groups = 8: one panel and one bias column per rate),
    each rate against its own float64 dilated conv under ulp16 / 2 + 8 e32 of that rate; 5 x 3 lies below most rates (every tap but the centre's falls outside)."""
    import innfer_amd.lib as L
    from innfer_amd import synth
    G = 8
    x = torch.from_numpy(synth.uniform((N, 64, H, W), 810 + H, -1, 1)).half()
    ws = [torch.from_numpy(synth.uniform((32, 64, 3, 3), 820 + g, -1, 1) / np.float32(24.0)) for g in range(G)]
    b = torch.from_numpy(synth.uniform((32 * G,), 830, -1, 1))
    pb = L.lib.innfer_conv3x3_packed_bytes(32, 64)
    packed = np.zeros(G * pb, dtype=np.uint8)
    for g in range(G):
        L.check(L.lib.innfer_pack_conv3x3(np.ascontiguousarray(ws[g].numpy()).ctypes.data, 32, 64, packed[g * pb:].ctypes.data))
    xin, d_packed, d_bias = R.to_slab(x, 3).to(dev), torch.from_numpy(packed).to(dev), b.to(dev)
    gs, numel = N * H * W * 32, G * N * H * W * 32
    buf = torch.full((numel + 2 * GUARD,), FILL, dtype=torch.float16, device=dev)
    a = L.ConvArgs()
    a.d_in, a.in_group_stride, a.C = xin.data_ptr(), gs, 64
    a.d_packed, a.d_bias = d_packed.data_ptr(), d_bias.data_ptr()
    a.d_out, a.out_group_stride, a.out_ch_off, a.K = buf.data_ptr() + 2 * GUARD, gs, 0, 32 * G
    a.N, a.H, a.W, a.act, a.dilation_groups = N, H, W, 0, G
    rc = L.lib.innfer_conv3x3_f16(C.byref(a), None)
    torch.cuda.synchronize()
    assert rc == 0, L.last_error()
    raw = buf.cpu()
    assert bool((raw[:GUARD] == FILL).all()) and bool((raw[GUARD + numel:] == FILL).all()), "wrote outside the output"
    got = R.from_slab(raw[GUARD:GUARD + numel].reshape(G, N, H, W, 32))
    for g in range(G):
        conv = lambda dt: F.conv2d(x.to(dt), ws[g].half().to(dt), b[32 * g:32 * g + 32].to(dt), padding=g + 1, dilation=g + 1)
        y64 = conv(torch.float64)
        e32 = (conv(torch.float32).double() - y64).abs().max().item()
        R.assert_within_fp16_rounding(got[:, 32 * g:32 * g + 32], y64, e32, what=f"dilation_groups rate {g + 1} {N}x{H}x{W}", family="dilation groups, one launch")


# ------------------------------------------------------------------------------------------------ the self gate
@pytest.mark.parametrize("Cc", [32, 64])
@pytest.mark.parametrize("up", [0, 1])
def test_self_gate(dev, Cc, up):
    """0x801FF: out = act(v sigmoid(Wg v + bg)), v = fp16(conv + bias) -- the kernel rounds v on purpose, the float64 reference does not: the allowance for it is
    computed per pixel (_conv_ref.self_gate)."""
    sizes = [(1, 2, 2), (1, 24, 32), (1, 26, 34), (1, 50, 70), (3, 38, 46)] if up else S24 + ([MANY24] if Cc == 32 else [])
    for (N, H, W) in sizes:
        c = Case("3x3", N, Cc, 32, H, W, seed=90 + Cc + up, up=up)
        y64, e32 = R.pre(c)
        for act in (0, 1):
            ref, extra = R.self_gate(c, y64, e32, act)
            got = _run(dev, c, act=act, gate=True)
            R.assert_within_fp16_rounding(got, ref, e32, extra=extra, what=f"{c} self gate act {act}", family="self gate" + (", upsampled input" if up else ""))


# ------------------------------------------------------------------------------------------------ the up-conv as four phases
@pytest.mark.parametrize("N,H,W", [(1, 5, 7), (2, 9, 13), (1, 16, 16), (1, 16, 32), (1, 17, 33), (3, 37, 45), (1, 50, 70), (1, 257, 513)])
def test_upconv_phases(dev, N, H, W):
    """nearest 2x + conv3x3 (64 -> 64) as four 2x2-tap phases over the source grid (innfer_pack_up2x_phases through transposed2x = 4): against float64 with the packer's
    own weights Wt = fp16(float32 sum of taps) (bit-compared with the packer on the CPU).  plane_rows 1 is the one-visit kernel (grids wider than 16; refused below) and
    must equal plane_rows 0 bit for bit.  The distance to the nine-tap weights' float64 result is what the fold costs: reported, not bounded here
    (test_upconv_phases_vs_nine_taps_and_oracle holds it)."""
    import innfer_amd.lib as L
    c = Case("upph", N, 64, 64, H, W, seed=100)
    y64, e32 = R.pre(c)
    ref, _ = R.epilogue(y64, 1)
    got0 = _run(dev, c, act=1, plane_rows=0)
    R.assert_within_fp16_rounding(got0, ref, e32, what=f"{c} rows 0", family="up-conv phases")
    if W > 16:
        got1 = _run(dev, c, act=1, plane_rows=1)
        assert torch.equal(got0, got1), "the one-visit form differs from one phase per visit"
    else:
        _run(dev, c, act=1, plane_rows=1, expect=L.ERR_UNSUPPORTED)
    if H <= 50:
        x, w, b = R.data(c)
        nine = F.leaky_relu(F.conv2d(F.interpolate(x.double(), scale_factor=2.0, mode="nearest"), w.half().double(), b.double(), padding=1), 0.2)
        print(f"[conv-forms] up-conv phases | {c}: max |phases - nine-tap float64| {(got0.double() - nine).abs().max().item():.2e} (reported only)")


# ------------------------------------------------------------------------------------------------ the forms that were reachable before, on record
SWEEP = [
    ("3x3 32 outputs", Case("3x3", 2, 96, 32, 37, 45, seed=110), dict(act=1)),
    ("3x3 64 outputs", Case("3x3", 2, 64, 64, 37, 45, seed=111), dict(act=1)),
    ("3x3 64 outputs", Case("3x3", 2, 64, 64, 37, 45, seed=111), dict(act=1, plane_rows=1)),
    ("3x3 64 outputs", Case("3x3", 1, 192, 64, 25, 33, seed=112), dict(act=0, nres=2, s1=0.2, s2=0.2)),
    ("3x3 32 outputs", Case("3x3", 1, 64, 32, 25, 33, seed=113), dict(act=1, nres=1, s1=0.2)),
    ("3x3 32 outputs", Case("3x3", 1, 64, 32, 25, 33, seed=114, reflect=1), dict(act=2)),
    ("3x3 upsampled input", Case("3x3", 2, 64, 64, 38, 46, seed=115, up=1), dict(act=1)),
    ("3x3 upsampled input", Case("3x3", 2, 64, 32, 38, 46, seed=116, up=1), dict(act=1)),
    ("PixelShuffle(2) store", Case("shuffle", 2, 64, 128, 25, 33, seed=117), dict(act=1)),
    ("Conv2d(4, 2, 1)", Case("s2k4", 2, 64, 64, 25, 33, seed=118), dict(act=1)),
    ("ConvTranspose2d(k, 2, 1)", Case("t2x", 2, 64, 64, 25, 33, seed=119, k=4), dict(act=2)),
    ("ConvTranspose2d(k, 2, 1)", Case("t2x", 2, 64, 64, 25, 33, seed=120, k=3), dict(act=2)),
    ("7x1 column conv", Case("7x1", 2, 96, 64, 25, 33, seed=121), dict(act=0)),
    ("7x1 column conv", Case("7x1", 2, 96, 32, 25, 33, seed=122, reflect=1), dict(act=1)),
    ("dilated 3x3", Case("dil", 1, 64, 32, 25, 33, seed=123, dil=2), dict(act=1)),
    ("dilated 3x3", Case("dil", 1, 64, 32, 25, 33, seed=124, dil=5), dict(act=1)),
]


@pytest.mark.parametrize("i", range(len(SWEEP)), ids=[f"{f} {c}".replace(" ", "_") for f, c, _ in SWEEP])
def test_reachable_forms_within_fp16_rounding(dev, i):
    """The forms tests/test_gpu_parity.py already runs alone (at a flat 4e-3 against float32), once each at a ragged size through the float64 bound."""
    fam, c, kw = SWEEP[i]
    _check(dev, c, "sweep: " + fam, **kw)


# ------------------------------------------------------------------------------------------------ the fp32-accurate forms
def _run_split(dev, c, x32, w32, out, act=0):
    """The case on (hi, lo) operand pairs: x32 / w32 fp32.  out "f32": planar [N, K, H, W]; "slab": the split slab pair read back as fp32."""
    import innfer_amd.lib as L
    N, Cc, H, W = x32.shape
    g = N * H * W * 32
    G = Cc // 32
    xin = torch.full((2, G, N, H, W, 32), 7.0, dtype=torch.float16, device=dev)
    L.check(L.lib.innfer_nchw_to_slab_split(x32.to(dev).contiguous().data_ptr(), xin.data_ptr(), g, G * g, 0, N, Cc, H, W, None))
    wc = np.ascontiguousarray(w32.numpy(), dtype=np.float32)
    if c.form == "1x1":
        packed = np.zeros(3 * L.lib.innfer_conv1x1_packed_bytes(c.K, Cc), dtype=np.uint8)
        L.check(L.lib.innfer_pack_conv1x1_split(wc.ctypes.data, c.K, Cc, packed.ctypes.data))
    else:
        packed = np.zeros(3 * L.lib.innfer_conv3x3_packed_bytes(c.K, Cc), dtype=np.uint8)
        L.check(L.lib.innfer_pack_conv3x3_split(wc.ctypes.data, c.K, Cc, packed.ctypes.data))
    d_packed = torch.from_numpy(packed).to(dev)
    bias = torch.zeros((c.K + 63) // 64 * 64)
    bias[:c.K] = R.data(c)[2]
    d_bias = bias.to(dev)
    a = L.ConvArgs()
    a.d_in, a.in_group_stride, a.C = xin.data_ptr(), g, Cc
    a.d_packed, a.d_bias = d_packed.data_ptr(), d_bias.data_ptr()
    a.K, a.N, a.H, a.W, a.act = c.K, N, H, W, act
    a.split, a.in_lo, a.conv1x1 = 1, G * g, int(c.form == "1x1")
    if out == "f32":
        numel = N * c.K * H * W
        buf = torch.full((numel + 2 * GUARD,), FILL, dtype=torch.float32, device=dev)
        a.d_out, a.out_planar = buf.data_ptr() + 4 * GUARD, 2
        L.check(L.lib.innfer_conv3x3_f16(C.byref(a), None))
        torch.cuda.synchronize()
        raw = buf.cpu()
        assert bool((raw[:GUARD] == FILL).all()) and bool((raw[GUARD + numel:] == FILL).all()), f"{c}: wrote outside the output"
        return raw[GUARD:GUARD + numel].reshape(N, c.K, H, W)
    og = c.K // 32
    o = torch.full((2, og, N, H, W, 32), FILL, dtype=torch.float16, device=dev)
    a.d_out, a.out_group_stride, a.out_lo = o.data_ptr(), g, og * g
    L.check(L.lib.innfer_conv3x3_f16(C.byref(a), None))
    torch.cuda.synchronize()
    res = torch.empty((N, c.K, H, W), dtype=torch.float32, device=dev)
    L.check(L.lib.innfer_slab_split_to_nchw(o.data_ptr(), g, og * g, 0, res.data_ptr(), N, c.K, H, W, None))
    torch.cuda.synchronize()
    return res.cpu()


def _split_operands(c):
    from innfer_amd import synth
    x = torch.from_numpy(synth.uniform((c.N, c.C, c.H, c.W), 100 * c.seed + 31, -1, 1))
    _, w, b = R.data(c)
    return x, w, b


@pytest.mark.parametrize("K", [3, 16])
def test_planar_output_in_the_fp32_mode(dev, K):
    """0x21FF with OUT_NCHW (the last conv of a network in the fp32-accurate mode): fp32 operands as (hi, lo) pairs, against float64 on the same fp32 operands at the fp32
    mode's bound of 3e-6 on O(1) outputs (tests/test_gpu_fp32_mode.py); tanh adds its 2^-21."""
    for (N, H, W) in [(1, 1, 1), (1, 25, 33), (3, 37, 45), (1, 50, 70)]:
        c = Case("3x3", N, 64, K, H, W, seed=130 + K)
        x, w, b = _split_operands(c)
        y = F.conv2d(x.double(), w.double(), b.double(), padding=1)
        for act in (0, 3):
            got = _run_split(dev, c, x, w, "f32", act=act)
            ref = torch.tanh(y) if act == 3 else y
            err = (got.double() - ref).abs().max().item()
            print(f"[conv-forms] planar 3x3, fp32 mode | {c} act {act}: max|err| {err:.2e}")
            assert err < 3e-6 + (R.TRANS if act == 3 else 0), (str(c), act, err)


@pytest.mark.parametrize("Cc,K", [(64, 32), (160, 32), (64, 64), (96, 64)])
def test_conv1x1_in_the_fp32_mode(dev, Cc, K):
    """0x2010: the 1x1 conv on (hi, lo) pairs, both tile widths, at the fp32 mode's 3e-6."""
    for (N, H, W) in [(1, 1, 1), (1, 17, 33), (3, 37, 45)]:
        c = Case("1x1", N, Cc, K, H, W, seed=140 + K)
        x, w, b = _split_operands(c)
        y = F.conv2d(x.double(), w.double()[:, :, None, None], b.double())
        for act in (0, 1):
            got = _run_split(dev, c, x, w, "slab", act=act)
            ref = F.leaky_relu(y, 0.2) if act else y
            err = (got.double() - ref).abs().max().item()
            print(f"[conv-forms] 1x1, fp32 mode | {c} act {act}: max|err| {err:.2e}")
            assert err < 3e-6, (str(c), act, err)


# ------------------------------------------------------------------------------------------------ refusals
def test_new_fields_are_refused_where_nothing_is_built(dev):
    """Each field of ABI 121 in a combination conv_launch does not build: INNFER_ERR_UNSUPPORTED / INVALID, and d_out keeps its fill (checked by _run)."""
    import innfer_amd.lib as L
    p3 = Case("3x3", 1, 64, 3, 9, 11, seed=150)
    s32 = Case("3x3", 1, 64, 32, 9, 11, seed=151)
    one32, one64 = Case("1x1", 1, 64, 32, 9, 11, seed=152), Case("1x1", 1, 64, 64, 9, 11, seed=153)
    r1 = R.residual(s32, 1, (1, 32, 9, 11))
    _run(dev, s32, "slab", act=6, expect=L.ERR_INVALID)                                  # sigmoid / tanh belong to planar outputs
    _run(dev, s32, "slab", act=3, expect=L.ERR_INVALID)
    _run(dev, s32, "slab", outm=1, expect=L.ERR_UNSUPPORTED)                             # outm: the planar last conv
    _run(dev, Case("3x3", 1, 64, 32, 9, 11, seed=151), "f16", outm=2, expect=L.ERR_UNSUPPORTED)      # ... of <= 16 channels
    _run(dev, Case("1x1", 1, 64, 32, 9, 11, seed=152, prefix=1), "slab", expect=L.ERR_UNSUPPORTED)   # the running sum is built for 64-output tiles
    _run(dev, s32, "slab", prefix_lrelu=1, expect=L.ERR_INVALID)                         # ... and for the 1x1 conv
    _run(dev, Case("3x3", 1, 64, 5, 9, 11, seed=154), "u8", expect=L.ERR_UNSUPPORTED)    # an image has <= 4 channels
    _run(dev, p3, "f16", out_denorm=1, expect=L.ERR_INVALID)                             # denormalisation belongs to the image
    _run(dev, Case("7x7", 1, 64, 3, 9, 11, seed=155), "f16", res1=R.residual(p3, 1, (1, 32, 9, 11)), expect=L.ERR_UNSUPPORTED)     # no residual on the 7x7
    _run(dev, Case("7x7", 1, 64, 32, 9, 11, seed=156), "f16", expect=L.ERR_UNSUPPORTED)  # 7x7: K <= 16
    _run(dev, Case("7x7", 1, 64, 32, 9, 11, seed=156), "slab", expect=L.ERR_UNSUPPORTED)   # ... planar only
    _run(dev, Case("7x7", 1, 64, 3, 2, 2, seed=157, reflect=1), "f16", expect=L.ERR_INVALID)   # ReflectionPad2d(3) needs 4 x 4
    _run(dev, one32, "f16", expect=L.ERR_UNSUPPORTED)                                    # 1x1: slab outputs
    _run(dev, Case("1x1", 1, 64, 16, 9, 11, seed=158), "slab", expect=L.ERR_UNSUPPORTED)   # ... of 32- / 64-channel tiles
    _run(dev, one64, "slab", act=4, expect=L.ERR_INVALID)                                # the PA gate multiplies res1
    _run(dev, s32, "slab", gate=True, res1=r1, expect=L.ERR_UNSUPPORTED)                 # the self gate: no residual,
    _run(dev, Case("3x3", 1, 64, 64, 9, 11, seed=159), "slab", gate=True, expect=L.ERR_UNSUPPORTED)    # 32 outputs,
    _run(dev, p3, "f16", gate=True, expect=L.ERR_UNSUPPORTED)                            # slab output
    _run(dev, s32, "slab", d_gate_bias=0x1000, expect=L.ERR_INVALID)                     # both pointers or none
    _run(dev, s32, "slab", in_relu=1, expect=L.ERR_UNSUPPORTED)                          # in_relu: the planar <= 16-output kernel
    _run(dev, Case("3x3", 1, 64, 32, 9, 11, seed=151, in_relu=1), "f16", expect=L.ERR_UNSUPPORTED)
    _run(dev, Case("phases", 1, 64, 3, 9, 11, seed=161), "u8", expect=L.ERR_UNSUPPORTED)       # no phases into an image
    _run(dev, p3, "f16", out_ch_off=16, expect=L.ERR_UNSUPPORTED)
    _run(dev, Case("t2x", 1, 64, 64, 9, 11, seed=162), "slab", outm=1, expect=L.ERR_UNSUPPORTED)   # the new fields do not combine with the stride-2 forms
    _run(dev, Case("7x1", 1, 64, 32, 9, 11, seed=163), "slab", conv1x1=1, expect=L.ERR_UNSUPPORTED)
