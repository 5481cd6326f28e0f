"""SwinIR on the GPU (needs an MI355X: `pytest -m gpu`): the window attention, the per-pixel LayerNorm and the GELU epilogue alone, whole networks, the Model.
Every launch writes between guard bands that must keep their fill; inputs must be unchanged.

1. innfer_window_attention against float64 on the stored fp16 operands: padded sizes 8x8, 8x16, 16x24, 24x40, each with shift 0 and shift 4 (the mask acts on the last
   window row and column; at 8x8 inside the one window, which wraps onto itself); (nH, d) = (6, 30), (6, 10), (2, 32), (8, 30); a batch of 3 whose samples differ, each
   bit-equal to its own N = 1 launch; one case with scores beyond +-40 (the row maximum must be subtracted).  The bound is tests/test_gpu_pan_fsa.py's convention,
   ulp16 / 2 + 8 e_model: e_model = max |model - exact| of a torch model of the kernel's DECLARED roundings -- float32 scores (q k^T + B, then + M), float32 maximum,
   exponentials and sum, P rounded to fp16 as the operand of P v, float32 accumulation and division -- computed on the CPU, never from the kernel.  Pad channels of the
   output are exactly zero.
2. innfer_layer_norm against float64 LayerNorm on the stored fp16 operands: C = 60, 180, 240, 64 in slabs of 64 ceil(C / 64) channels whose pad channels hold junk on
   input; 1x1, 8x8, 17x33 pixels and a batch whose pixels differ in scale and offset; in place == out of place, bit for bit.  The bound, per element, is one fp16
   rounding plus LN_STATS, what the float32 operations can cost (u = 2^-24, n = c_pad / 4 + 2 the longest chain of additions of a lane and its quad's butterfly):
     mean:  the sum's error is <= n u sum |x|, times 1 / C (its rounding and the product: 2 more):  |dmu| <= (n + 2) u A, A = max |x| of the pixel;
     var:   d = x - mu^ (one rounding), s = fma(d, d, s) along the same chain, times 1 / C, plus eps: <= (n + 5) u relative (mu's own error enters squared);
     rstd = 1 / sqrtf(var + eps): half of that and <= 2 u for each of the two operations:  <= ((n + 5) / 2 + 4) u relative;
     out = fma((x - mu^) rstd^, gamma, beta): the difference, the product and the fma, one rounding each.
   With z = (x - mu) / sigma:  LN_STATS = u [ ((n + 5) / 2 + 7) |gamma z| + (n + 2) |gamma| A / sigma + |gamma z| + |beta| ].
3. act 12 (innfer_conv3x3_f16, the 1x1 form, 64 -> 64 and 192 -> 64) against float64 GELU (erf) of the float64 conv with assert_within_fp16_rounding, extra = |f| GELU_T.
   GELU_T -- derived as MISH_T is.  common.h fast_gelu computes f - h (f >= 0) or -h, h = (|f| / 2) E, E = (q t) e^(-x^2), x = |f| / sqrt 2, t = 1 / (1 + p x), q the
   degree-4 Horner polynomial of Abramowitz & Stegun 7.1.26, whose E differs from erfc(x) by <= 1.5e-7 ABSOLUTE (their bound).  In float32 (u = 2^-24): x carries one
   rounding, which moves erfc by <= x erfc'(x) u <= 0.5 u; t one fma and a 1-ulp reciprocal (3 u relative, t <= 1); q four fmas on partial sums below 1.5 (<= 6 u); q t one
   more; e^(-x^2) = v_exp_f32 (2 u) of an argument whose rounding and log2 e scaling move it by (x^2 + 1) 2 u relative -- and (x^2 + 1) e^(-x^2) <= 1; the product: u.
   So |E^ - erfc| <= 1.5e-7 + (0.5 + 3 + 6 + 1 + 2 + 2 + 1) u = 1.5e-7 + 15.5 u = 1.08e-6, h = |f| E / 2 adds its two roundings and f - h one more (each <= u |f|):
   |error| <= |f| (0.54e-6 + 3 u) = |f| 0.72e-6 <= |f| 2^-20.  GELU_T = 2^-20 = 9.5e-7.
   One case has biases of +-60: the result stays finite (f itself above, -0 below).  The refusals: status and nothing written.
4. Networks against the float64 forward of tests/_swinir_ref.py: max |err| <= 2 x the fp16 storage model's own error on the same case and >= 99 % of the uint8 codes
   within +-1 (tests/test_swinir_host.py verifies the storage model alone on the CPU); the launch count equals the formula of DESIGN.md 3.4l; out= is honoured; a batch's
   sample equals its own forward bit for bit; forward_u8 == the separate conversions; a float32 tensor is refused.
   Measured on the MI355X, engine max |err| / storage model max |err| (100 % of the codes within +-1 in every case):
       C60 [2,2] direct x2 16x24 0.993 | direct x4 13x21 (padded) 0.897 | C180 pixelshuffle x4 16x16 1.002 | pixelshuffle x3 9x17 1.119 |
       C240 3conv nearest+conv x4 16x24 1.032 | C64 nearest+conv x2 8x8 1.000 | batch of two pixelshuffle x2 19x26 1.029 | Model chop x2 250x330 1.035
   Measured worst err / bound of the single launches: window attention 0.198 .. 0.269 (e_model 0.9e-4 .. 4.0e-4, scores up to +-289 included); layer norm 0.937 .. 0.994
   (the fp16 rounding dominates); act 12 0.865 .. 0.978 (e32 1.4e-7 .. 4.9e-6), biases of +-60 0.977.
5. Model(arch='infer', chop=True) from a .pth under params_ema (with the two buffers of a published checkpoint) against the helper run tile by tile; run_u8 plain, tta,
   seamless='tile', run_u8_batch and tile=32, tile_pad=8 against their definitions, bit for bit.
"""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _conv_ref as R
import _swinir_ref as SR
from _conv_ref import Case

pytestmark = pytest.mark.gpu

FILL, GUARD = -3.0, 4096
GELU_T = 2.0 ** -20
S16 = [(1, 1, 1), (1, 16, 32), (1, 17, 33), (1, 50, 70), (3, 37, 45)]          # the 16 x 32-tile edges, and a batch
MANY16 = (1, 273, 513)                                                         # more tiles than workgroups: a workgroup's second tile


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


# ------------------------------------------------------------------------------------------------ 1. the window attention
def _attn_data(N, Hp, Wp, nH, d, seed, gain=1.0):
    """q, k, v as fp16 [3, N, nH, d, Hp, Wp] (the values of the slab's real channels) and the dense bias table [nH, 64, 64] float32; samples of a batch differ."""
    from innfer_amd import synth
    qkv = synth.uniform((3, N, nH, d, Hp, Wp), 5000 + seed, -1, 1)
    for n in range(N):
        qkv[:, n] *= np.float32(1.0 + 0.5 * n)
    qkv[0] *= np.float32(gain)
    table = synth.uniform((nH, 64, 64), 5001 + seed, -2, 2)
    return torch.from_numpy(qkv).half(), torch.from_numpy(np.ascontiguousarray(table))


def _attn_ref(qkv, table, shift, dt, model=False):
    """softmax(q k^T + B + M) v per window and head in dtype dt through the roll; model: P rounded to fp16 in front of P v, the sum over the unrounded values."""
    _, N, nH, d, Hp, Wp = qkv.shape
    x = qkv.to(dt).reshape(3 * N, nH * d, Hp, Wp)
    if shift:
        x = torch.roll(x, (-shift, -shift), (2, 3))
    w = SR._windows(x).reshape(3, N, -1, 64, nH, d).permute(0, 1, 2, 4, 3, 5)          # [3, N, nW, nH, 64, d]
    S = w[0] @ w[1].transpose(-1, -2) + table.to(dt)
    if shift:
        S = S + SR.shift_mask(Hp, Wp).to(dt)[None, :, None]
    if model:
        e = torch.exp(S - S.amax(-1, keepdim=True))
        o = (e.half().to(dt) @ w[2]) / e.sum(-1, keepdim=True)
    else:
        o = torch.softmax(S, -1) @ w[2]
    o = SR._unwindows(o.permute(0, 1, 3, 2, 4).reshape(N, -1, 64, nH * d), Hp, Wp)
    if shift:
        o = torch.roll(o, (shift, shift), (2, 3))
    return o.reshape(N, nH, d, Hp, Wp), float(S.abs().max())


def _attn_launch(dev, qkv, table, shift):
    """innfer_window_attention from a head-padded slab of its own into [guard | nH groups | a foreign group | guard].  Returns [N, nH, 32, Hp, Wp] fp16 (cpu)."""
    import innfer_amd.lib as L
    _, N, nH, d, Hp, Wp = qkv.shape
    G = N * Hp * Wp * 32
    pad = torch.zeros(3, N, nH, 32, Hp, Wp, dtype=torch.float16)
    pad[:, :, :, :d] = qkv
    slab = pad.permute(0, 2, 1, 4, 5, 3).contiguous()                                  # [3, nH, N, Hp, Wp, 32]: group which * nH + h
    xin = slab.to(dev)
    buf = torch.full(((nH + 1) * G + 2 * GUARD,), FILL, dtype=torch.float16, device=dev)
    tb = np.ascontiguousarray(table.numpy(), np.float32)
    L.check(L.lib.innfer_window_attention(xin.data_ptr(), G, buf.data_ptr() + 2 * GUARD, G, tb.ctypes.data, N, Hp, Wp, nH, d, shift, None))
    torch.cuda.synchronize()
    raw = buf.cpu()
    assert bool((raw[:GUARD] == FILL).all()) and bool((raw[GUARD + nH * G:] == FILL).all()), "window attention wrote outside its output"
    assert torch.equal(xin.cpu(), slab), "window attention wrote to its input"
    return raw[GUARD:GUARD + nH * G].reshape(nH, N, Hp, Wp, 32).permute(1, 0, 4, 2, 3)


def _attn_check(dev, N, Hp, Wp, nH, d, shift, seed, gain=1.0, smin=0.0):
    qkv, table = _attn_data(N, Hp, Wp, nH, d, seed, gain)
    ref, smax = _attn_ref(qkv, table, shift, torch.float64)
    assert smax >= smin, (smax, smin)
    e_model = float((_attn_ref(qkv, table, shift, torch.float32, model=True)[0].double() - ref).abs().max())
    got = _attn_launch(dev, qkv, table, shift)
    assert bool((got[:, :, d:] == 0).all()), "pad channels of the attention's result are not zero"
    what = f"window attention {N}x{Hp}x{Wp} nH {nH} d {d} shift {shift}" + (f" (|S| up to {smax:.0f})" if smin else "")
    R.assert_within_fp16_rounding(got[:, :, :d], ref, e_model, what=what, family=f"window attention, shift {shift}")
    return qkv, table, got


@pytest.mark.parametrize("nH,d", [(6, 30), (6, 10), (2, 32), (8, 30)])
def test_window_attention(dev, nH, d):
    for i, (Hp, Wp) in enumerate([(8, 8), (8, 16), (16, 24), (24, 40)]):
        for shift in (0, 4):
            _attn_check(dev, 1, Hp, Wp, nH, d, shift, 100 * nH + 10 * i + shift)


def test_window_attention_batch_and_large_scores(dev):
    """A window of sample n reads only sample n: each sample of a batch of three equals its own launch bit for bit; scores beyond +-40 stay finite and inside the bound."""
    for shift in (0, 4):
        qkv, table, got = _attn_check(dev, 3, 16, 24, 6, 30, shift, 900 + shift)
        for n in range(3):
            one = _attn_launch(dev, qkv[:, n:n + 1].contiguous(), table, shift)
            assert torch.equal(one.view(torch.int16), got[n:n + 1].contiguous().view(torch.int16)), (shift, n)
        _attn_check(dev, 1, 16, 24, 2, 32, shift, 950 + shift, gain=24.0, smin=40.0)


def test_window_attention_refusals(dev):
    import innfer_amd.lib as L
    buf = torch.zeros(64 * 64 * 32 * 8, dtype=torch.float16, device=dev)
    tb = np.zeros((8, 64, 64), np.float32)
    G = 16 * 16 * 32
    call = lambda Hp, Wp, nH, d, shift: L.lib.innfer_window_attention(buf.data_ptr(), G, buf.data_ptr(), G, tb.ctypes.data, 1, Hp, Wp, nH, d, shift, None)
    assert call(16, 12, 2, 32, 0) == L.ERR_INVALID and call(16, 16, 9, 8, 0) == L.ERR_UNSUPPORTED and call(16, 16, 2, 33, 0) == L.ERR_UNSUPPORTED
    assert call(16, 16, 2, 32, 2) == L.ERR_UNSUPPORTED


# ------------------------------------------------------------------------------------------------ 2. LayerNorm
def _ln_launch(dev, x, Cc, gamma, beta, in_place=False):
    """x: fp16 [N, c_pad, H, W] whose channels >= Cc hold junk.  Returns [N, c_pad, H, W] fp16 (cpu)."""
    import innfer_amd.lib as L
    N, cp, H, W = x.shape
    G, ng = N * H * W * 32, cp // 32
    xin = R.to_slab(x).to(dev)
    g, b = np.ascontiguousarray(gamma.numpy(), np.float32), np.ascontiguousarray(beta.numpy(), np.float32)
    if in_place:
        L.check(L.lib.innfer_layer_norm(xin.data_ptr(), G, xin.data_ptr(), G, N * H * W, Cc, cp, g.ctypes.data, b.ctypes.data, 1e-5, None))
        torch.cuda.synchronize()
        return R.from_slab(xin.cpu())
    buf = torch.full(((ng + 1) * G + 2 * GUARD,), FILL, dtype=torch.float16, device=dev)
    L.check(L.lib.innfer_layer_norm(xin.data_ptr(), G, buf.data_ptr() + 2 * GUARD, G, N * H * W, Cc, cp, g.ctypes.data, b.ctypes.data, 1e-5, None))
    torch.cuda.synchronize()
    raw = buf.cpu()
    assert bool((raw[:GUARD] == FILL).all()) and bool((raw[GUARD + ng * G:] == FILL).all()), "layer norm wrote outside its output"
    assert torch.equal(xin.cpu(), R.to_slab(x)), "layer norm wrote to its input"
    return R.from_slab(raw[GUARD:GUARD + ng * G].reshape(ng, N, H, W, 32))


@pytest.mark.parametrize("Cc", [60, 180, 240, 64])
def test_layer_norm(dev, Cc):
    from innfer_amd import synth
    cp = -(-Cc // 64) * 64
    n_chain = cp // 4 + 2
    for i, (N, H, W) in enumerate([(1, 1, 1), (1, 8, 8), (1, 17, 33), (3, 17, 33)]):
        seed = 7000 + 10 * Cc + i
        x = synth.uniform((N, cp, H, W), seed, -1, 1)
        x = x * synth.uniform((N, 1, H, W), seed + 1, 0.25, 4.0) + synth.uniform((N, 1, H, W), seed + 2, -2.0, 2.0)          # pixels differ in scale and offset
        x[:, Cc:] = 7.0                                                                                                     # junk in the pad channels: ignored
        x = torch.from_numpy(np.ascontiguousarray(x, np.float32)).half()
        gamma, beta = torch.from_numpy(synth.uniform((Cc,), seed + 3, 0.5, 1.5)), torch.from_numpy(synth.uniform((Cc,), seed + 4, -0.2, 0.2))
        x64 = x[:, :Cc].double()
        ref = SR.layer_norm(x64, gamma.double(), beta.double())
        mu = x64.mean(1, keepdim=True)
        sigma = torch.sqrt(x64.var(1, unbiased=False, keepdim=True) + 1e-5)
        A = x64.abs().amax(1, keepdim=True)
        ga, be = gamma.double().abs()[None, :, None, None], beta.double().abs()[None, :, None, None]
        gz = ga * ((x64 - mu) / sigma).abs()
        ln_stats = 2.0 ** -24 * (((n_chain + 5) / 2 + 7) * gz + (n_chain + 2) * ga * A / sigma + gz + be)
        got = _ln_launch(dev, x, Cc, gamma, beta)
        assert bool((got[:, Cc:] == 0).all()), "pad channels of the layer norm's result are not zero"
        R.assert_within_fp16_rounding(got[:, :Cc], ref, 0.0, extra=ln_stats, what=f"layer norm C {Cc} {N}x{H}x{W}", family=f"layer norm, C {Cc}")
        assert torch.equal(_ln_launch(dev, x, Cc, gamma, beta, in_place=True).view(torch.int16), got.view(torch.int16)), "in place differs from out of place"


def test_layer_norm_refusals(dev):
    import innfer_amd.lib as L
    buf = torch.zeros(64 * 512, dtype=torch.float16, device=dev)
    g = np.ones(512, np.float32)
    call = lambda Cc, cp: L.lib.innfer_layer_norm(buf.data_ptr(), 64 * 32, buf.data_ptr(), 64 * 32, 64, Cc, cp, g.ctypes.data, g.ctypes.data, 1e-5, None)
    assert call(300, 320) == L.ERR_UNSUPPORTED and call(60, 48) == L.ERR_UNSUPPORTED and call(60, 32) == L.ERR_UNSUPPORTED


# ------------------------------------------------------------------------------------------------ 3. the GELU epilogue
def _launch(dev, c, expect=0, form="1x1", bias=None, res=False, off=0, **fields):
    """One launch through innfer_conv3x3_f16 with act 12 into [guard | off / 32 groups | the conv's groups | a foreign group | guard]: everything beside the result must
    keep its fill, like everything a refused launch (expect != 0) was given.  Returns [N, K, H, W] fp16 (cpu)."""
    import innfer_amd.lib as L
    lib = L.lib
    x, w, b = R.data(c)
    if bias is not None:
        b = bias
    N, Cc, H, W = x.shape
    xin = R.to_slab(x, Cc // 32 + 1).to(dev)
    wc = np.ascontiguousarray(w.numpy(), dtype=np.float32)
    if form == "1x1":
        packed = np.zeros(lib.innfer_conv1x1_packed_bytes(c.K, Cc), dtype=np.uint8)
        L.check(lib.innfer_pack_conv1x1(wc.ctypes.data, c.K, Cc, packed.ctypes.data))
    elif fields.get("split"):
        packed = np.zeros(3 * lib.innfer_conv1x1_packed_bytes(c.K, Cc), dtype=np.uint8)
        L.check(lib.innfer_pack_conv1x1_split(wc.ctypes.data, c.K, Cc, packed.ctypes.data))
    else:
        packed = np.zeros(lib.innfer_conv3x3_packed_bytes(c.K, Cc), dtype=np.uint8)
        L.check(lib.innfer_pack_conv3x3_rows(wc.ctypes.data, c.K, Cc, fields.get("plane_rows", 0), packed.ctypes.data))
    d_packed = torch.from_numpy(packed).to(dev)
    bb = torch.zeros(64); bb[:c.K] = b
    d_bias = bb.to(dev)
    groups = off // 32 + (c.K + 31) // 32 + 1
    G = N * H * W * 32
    buf = torch.full((2 * groups * G + 2 * GUARD,), FILL, dtype=torch.float16, device=dev)
    keep = []
    a = L.ConvArgs()
    a.d_in, a.in_group_stride, a.C = xin.data_ptr(), G, Cc
    a.d_packed, a.d_bias = d_packed.data_ptr(), d_bias.data_ptr()
    a.d_out, a.out_group_stride, a.K, a.out_ch_off = buf.data_ptr() + GUARD * 2, G, c.K, off
    a.N, a.H, a.W, a.act = N, H, W, 12
    a.conv1x1 = int(form == "1x1" or bool(fields.get("split")))
    if res:
        keep.append(R.to_slab(torch.zeros((N, max(c.K, 32), H, W), dtype=torch.float16)).to(dev))
        a.d_res1, a.res1_group_stride, a.res1_scale = keep[-1].data_ptr(), G, 1.0
    for k, v in fields.items():
        assert hasattr(a, k), k
        if k == "d_stats_part":
            n = N * lib.innfer_conv_stats_records(H, W, 1) * c.K * 3
            keep.append(torch.zeros(n, dtype=torch.float32, device=dev))
            a.d_stats_part, a.stats_part_floats = keep[-1].data_ptr(), n
        else:
            setattr(a, k, v)
    rc = lib.innfer_conv3x3_f16(C.byref(a), None)
    torch.cuda.synchronize()
    raw = buf.cpu()
    if expect:
        assert rc == expect, (str(c), fields, rc, L.last_error())
        assert bool((raw == FILL).all()), f"{c}: a refused launch wrote to d_out"
        return None
    assert rc == 0, (str(c), L.last_error())
    assert bool((raw[:GUARD] == FILL).all()) and bool((raw[GUARD + groups * G:] == FILL).all()), f"{c}: wrote outside the output"
    assert torch.equal(xin.cpu(), R.to_slab(x, Cc // 32 + 1)), f"{c}: wrote to its input"
    got = R.from_slab(raw[GUARD:GUARD + groups * G].reshape(groups, N, H, W, 32))
    assert bool((got[:, :off] == FILL).all()) and bool((got[:, off + c.K:] == FILL).all()), f"{c}: channels beside the conv's were written"
    return got[:, off:off + c.K]


def _gelu64(y):
    return y * 0.5 * (1.0 + torch.erf(y / np.sqrt(2.0)))


@pytest.mark.parametrize("Cin", [64, 192])
def test_gelu_epilogue(dev, Cin):
    """conv3x3_pc<2, 4, 4, OUT_SLAB, .., TAPS_1X1 | PC_GELU, false, 3>: ragged edges, a batch, a workgroup's second tile (273 x 513), a whole-group channel offset."""
    for i, (N, H, W) in enumerate(S16 + [MANY16]):
        c = Case("1x1", N, Cin, 64, H, W, seed=300 + Cin + i, blo=-3.0)
        y64, e32 = R.pre(c)
        got = _launch(dev, c, off=64 if i == 2 else 0)
        R.assert_within_fp16_rounding(got, _gelu64(y64), e32, extra=y64.abs() * GELU_T, what=f"{c} act 12", family=f"act 12, {Cin} -> 64")


def test_gelu_epilogue_large_arguments(dev):
    """Biases of +-60 (alternating by channel): e^(-1800) underflows -- the result stays finite: f itself above, (minus) zero below."""
    c = Case("1x1", 1, 64, 64, 17, 33, seed=381)
    bias = torch.tensor([60.0 if i % 2 == 0 else -60.0 for i in range(64)])
    x, w, _ = R.data(c)
    y64 = F.conv2d(x.double(), w.half().double()[:, :, None, None], bias.double())
    e32 = float((F.conv2d(x.float(), w.half().float()[:, :, None, None], bias).double() - y64).abs().max())
    got = _launch(dev, c, bias=bias)
    assert torch.isfinite(got).all() and float(y64.abs().min()) > 55
    assert bool((got[:, 1::2] == 0).all()) and bool((got[:, 0::2] > 55).all())
    R.assert_within_fp16_rounding(got, _gelu64(y64), e32, extra=y64.abs() * GELU_T, what=f"{c} act 12, biases +-60", family="act 12, large arguments")


def test_gelu_epilogue_refusals(dev):
    """act 12 on a form that does not build it is UNSUPPORTED; nothing is launched: d_out keeps its fill."""
    import innfer_amd.lib as L
    c = Case("1x1", 1, 64, 64, 16, 32, seed=395)
    c3 = Case("3x3", 1, 64, 64, 16, 32, seed=395)
    G = 16 * 32 * 32
    U = L.ERR_UNSUPPORTED
    _launch(dev, c3, form="3x3", expect=U)
    _launch(dev, c3, form="3x3", plane_rows=1, expect=U)
    _launch(dev, c, out_planar=1, expect=U)
    _launch(dev, c, split=1, in_lo=3 * G, out_lo=3 * G, expect=U)
    _launch(dev, c, d_stats_part=1, expect=U)
    _launch(dev, c, prefix_lrelu=1, expect=U)
    _launch(dev, c, upsample2x=1, expect=U)
    _launch(dev, c, reflect_pad=1, expect=U)
    _launch(dev, c, res=True, expect=U)
    _launch(dev, Case("1x1", 1, 64, 32, 16, 32, seed=396), expect=U)          # the 32-output kernel has no GELU form
    _launch(dev, Case("1x1", 1, 64, 16, 16, 32, seed=397), expect=U)


# ------------------------------------------------------------------------------------------------ 4. networks
def _net(dev, sd, wrap=True, with_buffers=False):
    from innfer_amd.architectures import get_network
    from innfer_amd.run import infer_from_state_dict
    if with_buffers:
        sd = dict(sd, **SR.buffers(sd))
    info = infer_from_state_dict({"params_ema": sd} if wrap else sd)
    net = get_network(info["net_params"])
    net.load_state_dict(info["state_dict"], strict=True)
    return net.to(dev).eval()


def _assert_like_storage_model(got, y64, ys, what):
    """max |engine - float64| <= 2 x max |storage model - float64| of the same case (computed here), and >= 99 % of the uint8 codes within +-1."""
    err, es = float((got.double() - y64).abs().max()), float((ys - y64).abs().max())
    share = SR.codes_within_one(got, y64)
    print(f"[swinir] {what}: engine max|err| {err:.2e}, storage model {es:.2e}, ratio {err / es:.3f}; codes within +-1: {share:.5f}")
    assert got.shape == y64.shape and torch.isfinite(got).all()
    assert err <= 2 * es, (what, err, es)
    assert share >= 0.99, (what, share)


def launch_formula(Cc, nH, hidden, depths, upsampler, s, resi, padded):
    """S1 + 2 + B (3 + SQ + 2 S1 + SH) + (R + 1) SR + T + 2 [padded]."""
    S1, SQ, SH = -(-Cc // 64), -(-3 * nH // 2), -(-hidden // 64)
    SR_ = S1 if resi == "1conv" else 2 * -(-Cc // 256) + S1
    lg = {2: 1, 4: 2}.get(s, 0)
    T = {"pixelshuffledirect": 2, "pixelshuffle": 4 if s == 3 else 2 + lg, "nearest+conv": 3 + lg}[upsampler]
    return S1 + 2 + sum(depths) * (3 + SQ + 2 * S1 + SH) + (len(depths) + 1) * SR_ + T + (2 if padded else 0)


def _launches(net, x):
    """Launch count of one forward (innfer_net_forward_timed)."""
    import innfer_amd.lib as L
    N, _, H, W = x.shape
    s = L.lib.innfer_net_scale(net._handle)
    out = torch.empty((N, net.out_nc, H * s, W * s), dtype=torch.float16, device=x.device)
    ws = torch.empty(L.lib.innfer_net_workspace_bytes(net._handle, N, H, W), dtype=torch.uint8, device=x.device)
    n = C.c_int()
    ms = (C.c_float * 1024)()
    L.check(L.lib.innfer_net_forward_timed(net._handle, x.data_ptr(), L.F16, out.data_ptr(), L.F16, N, H, W, ws.data_ptr(), ws.numel(), None, 1024, ms, None, None, None, C.byref(n)))
    return n.value, out


@pytest.mark.parametrize("name", list(SR.FIXTURES))
def test_network_vs_float64(dev, name):
    from innfer_amd import synth
    from innfer_amd.utils import utils as U
    Cc, nH, depths, shape, ups, s, resi, seed = SR.FIXTURES[name]
    sd, x, y64, ys = SR.case(name)
    net = _net(dev, sd, with_buffers=seed % 2 == 1)
    assert (net.nf, net.num_heads, tuple(net.depths), net.upsampler, net.upscale, net.resi_connection) == (Cc, nH, tuple(depths), ups, s, resi)
    xd = x.to(dev).half()
    y = net(xd)
    assert y.dtype == torch.float16 and net._out_shape(shape[0], shape[2], shape[3], dev) == tuple(y64.shape) == tuple(y.shape)
    _assert_like_storage_model(y.float().cpu(), y64, ys, name)
    n, yt = _launches(net, xd)
    assert n == launch_formula(Cc, nH, 2 * Cc, depths, ups, s, resi, shape[2] % 8 != 0 or shape[3] % 8 != 0) and torch.equal(yt, y), n
    buf = torch.empty(y.shape, dtype=torch.float16, device=dev)
    assert net(xd, out=buf) is buf and torch.equal(buf, y)
    if shape[0] > 1:          # nothing in SwinIR crosses samples
        assert torch.equal(net(xd[1:]), y[1:])
    img = torch.from_numpy(synth.image_u8(shape[2], shape[3], 3, s)).to(dev)
    sep = U.tensor2np(net(U.np2tensor(img.cpu().numpy(), dtype=torch.float16)))
    assert np.array_equal(net.forward_u8(img).cpu().numpy(), sep)
    with pytest.raises(NotImplementedError, match="fp16 mode"):
        net(x.to(dev))
    with pytest.raises(NotImplementedError, match="fp16 mode"):
        net.forward_u8(img, fp16=False)
    assert net.flops(1, shape[2], shape[3]) > 0 and net.tile_batch_bytes(2, 16) > 0


def test_network_refuses_sides_too_short_to_pad(dev):
    sd = SR.fixture_sd("C64 [2] nearest+conv x2 8x8")
    net = _net(dev, sd)
    with pytest.raises(NotImplementedError, match="reflection"):
        net(torch.zeros(1, 3, 4, 16, dtype=torch.float16, device=dev))
    assert tuple(net(torch.zeros(1, 3, 5, 16, dtype=torch.float16, device=dev)).shape) == (1, 3, 10, 32)


# ------------------------------------------------------------------------------------------------ 5. the Model
@pytest.fixture(scope="module")
def model(tmp_path_factory):
    from innfer_amd.run import Model
    sd = SR.fill(3, 60, (2,), 6, 2.0, 2, "pixelshuffle", "1conv", seed=8)
    path = str(tmp_path_factory.mktemp("swinir") / "2x_swinir.pth")
    torch.save({"params_ema": dict(sd, **SR.buffers(sd))}, path)
    m = Model(path, arch="infer", scale=None, device="cuda", chop=True, tile_batch=4)
    assert (m.arch, m.scale, m.in_nc, m.out_nc) == ("swinir", 2, 3, 3)
    return m, sd


def test_model_chop(dev, model):
    """250 x 330 through the chop path against the helper run tile by tile (oracle.extract_patches_2d / recompose_tensor; the storage model's blend rounded to fp16 as the
    chop path's is); run_u8 == the separate conversions; a float32 tensor is refused."""
    import oracle
    from innfer_amd import synth
    from innfer_amd.utils import utils as U
    m, sd = model
    x = torch.from_numpy(synth.uniform((1, 3, 250, 330), 52))
    y = m(x.to(dev).half()).float().cpu()
    assert tuple(y.shape) == (1, 3, 500, 660)
    tiles = oracle.extract_patches_2d(x, (200, 200), [0.5, 0.5], batch_first=True).squeeze(0)
    h64 = torch.cat([SR.forward64(sd, tiles[i:i + 1], 2, "pixelshuffle") for i in range(tiles.shape[0])], 0)
    hs = torch.cat([SR.forward_storage(sd, tiles[i:i + 1], 2, "pixelshuffle") for i in range(tiles.shape[0])], 0)
    y64 = oracle.recompose_tensor(h64, 250, 330, step=0.5, scale=2).double()
    ys = oracle.recompose_tensor(hs, 250, 330, step=0.5, scale=2).half().double()
    _assert_like_storage_model(y, y64, ys, "Model chop x2 250x330")
    img = synth.image_u8(250, 330, 3, 9)
    assert np.array_equal(m.run_u8(img), U.tensor2np(m(U.np2tensor(img, dtype=torch.float16))))
    with pytest.raises(NotImplementedError, match="fp16 mode"):
        m(x.to(dev))


def test_model_run_u8_options(dev, model):
    """plain, tile=, tta, seamless='tile' and run_u8_batch on a SwinIR model: each equals the definition its docstring gives for it, bit for bit (images <= 96 px)."""
    from innfer_amd import synth
    from innfer_amd.run import Model
    from innfer_amd.utils import utils as U
    m, sd = model
    h, w = 40, 56
    img = synth.image_u8(h, w, 3, 61)
    plain = m.run_u8(img)
    assert plain.shape == (2 * h, 2 * w, 3) and np.array_equal(plain, U.tensor2np(m(U.np2tensor(img, dtype=torch.float16))))
    got = m.run_u8(img, tta=True)
    assert np.array_equal(got, U.tensor2np(m.forward_tta(U.np2tensor(img, dtype=torch.float16))))
    got = m.run_u8(img, seamless="tile")
    want = U.tensor2np(m(U.np2tensor(U.seamless_pad_np(img, "tile"), dtype=torch.float16)))[32:-32, 32:-32]
    assert got.shape == plain.shape and np.array_equal(got, want)
    imgs = [img, synth.image_u8(33, 96, 3, 62), synth.image_u8(64, 17, 3, 63)]
    for a, b in zip(m.run_u8_batch(imgs), [m.run_u8(i) for i in imgs]):
        assert np.array_equal(a, b)
    mt = Model(None, arch="infer", scale=None, device="cuda", chop=True, tile_batch=4, state_dict={"params_ema": sd}, tile=32, tile_pad=8)
    big = synth.image_u8(70, 96, 3, 64)
    assert np.array_equal(mt.run_u8(big), U.tensor2np(mt(U.np2tensor(big, dtype=torch.float16))))
