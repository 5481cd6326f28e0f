"""The small pointwise / gather kernels around PAN, PPON, the WBC UNet and the image filters, one launch at a time, against float64 (needs an MI355X: `pytest -m gpu`).

Under test, each through a single-launch entry point that calls the launch function the forwards call (ABI 124: innfer_pan_pre / _upsample / _final / _slab_pair,
innfer_ppon_upsample3 / _axpy, innfer_wbc_pre / _upadd, innfer_f32_prefix_lrelu / _act_copy) or that was exported before (innfer_guided_filter, innfer_guided_filter_ex,
innfer_filter2d): pan_pre, pan_upsample, pan_final, pan_final_x4, pan_nchw_to_slab_pair, ppon_upsample3, ppon_axpy, wb_pre, wb_upadd, gf_ab + gf_out, gf_ab_r + gf_out_r /
gf_out_fast, k_filter2d, and the fp32 twins f32_bilinear_up, f32_nearest_up, f32_upadd, f32_axpy, f32_prefix_lrelu, f32_act_copy.  PPON's alpha is also exercised through
two whole engines.  References, models, case lists and where every bound comes from: tests/_glue_ref.py (checked on the CPU by tests/test_glue_cpu.py).

Every buffer a kernel writes is prefilled with a sentinel and sits between sentinel guards (a gap between slab groups must keep the sentinel); every input sits between
NaN guards and is compared with what was uploaded afterwards; a batch's samples differ and each is bit-equal to its own N = 1 launch.

fp32 stores carry no storage rounding, so their bound is 8 e32 + extra alone, and e32 -- a maximum over the values of a case -- understates the cost of float32 arithmetic
on a case of a few dozen values (tests/_conv_ref.py met the same).  For them e32 is therefore the largest over the family's size list at the same parameters.

Measured on the MI355X -- per family the largest e32 / e_model of its cases and the worst err / bound over every element of every case:
    family                                                      e32 / e_model   worst err / bound
    PPON alpha, network level                                   (derived)       1.000
    f32_act_copy, none / LeakyReLU / ReLU                       exact           bit-identical
    f32_act_copy, tanh / sigmoid                                6.3e-08         0.081
    f32_axpy                                                    (derived)       0.989
    f32_bilinear_up                                             2.5e-06         0.125
    f32_prefix_lrelu                                            3.6e-07         0.091
    f32_upadd                                                   1.2e-07         0.125
    guided filter ks 1 .. 7, fast                               9.2e-03         0.998
    guided filter ks 1 .. 7, regular                            4.9e-05         0.996
    guided filter r = 1 (gf_ab + gf_out)                        1.4e-06         0.997
    k_filter2d                                                  2.3e-07         0.998
    pan_final / pan_final_x4, fp16 out                          2.3e-06         1.000
    pan_final / pan_final_x4, fp32 out                          2.3e-06         0.125
    pan_final form 0 == form 1                                  exact           bit-identical
    pan_nchw_to_slab_pair                                       exact           bit-identical
    pan_pre                                                     exact           bit-identical
    pan_upsample / f32_nearest_up / ppon_upsample3, nearest     exact           bit-identical
    pan_upsample, bilinear                                      3.3e-06         1.000
    ppon_axpy                                                   (derived)       1.000
    wb_pre                                                      exact           bit-identical
    wb_upadd, pt mode                                           5.2e-08         1.000
    wb_upadd, tf mode                                           exact           bit-identical
(fp16 stores sit at 1.0 because the storage rounding alone fills the bound; '(derived)': the bound is a derived extra alone.  The fast guided filter's largest e_model is the
float32 model's own error on its worst-conditioned case, eps 1e-4; the typical figure is 1e-7 .. 1e-6.)
conv forms as PPON issues them (tests/test_gpu_conv_forms.py): c2 with its two residual stages e32 2.6e-06, worst 0.974; dilation_groups = 8, per rate, e32 5.5e-07, worst 0.997.
pytest --durations: the slowest tests of this file are test_guided_filter_ex[7-*] at 0.3 s; the file runs in 6 s; the whole GPU suite in 408 s (1188 passed).
"""
import numpy as np
import pytest
import torch

import _conv_ref as C
import _glue_ref as G
import innfer_amd.lib as L

pytestmark = pytest.mark.gpu

GUARD = 4096                  # elements of guard in front of and behind every buffer
SENT = 777.0
F16, F32 = 0, 1               # innfer_dtype
GAP = 64                      # elements between slab groups that must keep the sentinel (a multiple of 8: 16-byte accesses)
f32 = np.float32
TD = {F16: torch.float16, F32: torch.float32}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


class Out:
    """a destination of n elements: sentinel-filled, between sentinel guards"""

    def __init__(self, n, dtype, dev):
        self.n = n
        self.buf = torch.full((GUARD + n + GUARD,), SENT, dtype=dtype, device=dev)
        self.v = self.buf[GUARD:GUARD + n]
        self.ptr = self.v.data_ptr()

    def cpu(self):
        torch.cuda.synchronize()
        assert bool((self.buf[:GUARD] == SENT).all()) and bool((self.buf[GUARD + self.n:] == SENT).all()), "wrote outside its destination"
        return self.v.cpu()


class In:
    """an input on the device between NaN guards; same() tells whether the kernel left it as uploaded"""

    def __init__(self, t, dev, n=None, at=None):
        t = t.contiguous().reshape(-1)
        n = n or t.numel()
        self.buf = torch.full((GUARD + n + GUARD,), float("nan"), dtype=t.dtype, device=dev)
        self.v = self.buf[GUARD:GUARD + n]
        if at is None:
            self.v.copy_(t)
        else:
            for off, part in at:
                self.v[off:off + part.numel()].copy_(part.reshape(-1))
        self.ptr = self.v.data_ptr()
        self.keep = self.buf.clone()

    def same(self):
        torch.cuda.synchronize()
        a, b = self.buf.view(torch.int16 if self.buf.dtype == torch.float16 else torch.int32), self.keep.view(torch.int16 if self.buf.dtype == torch.float16 else torch.int32)
        return bool(torch.equal(a, b))


def bits(t):
    t = t.contiguous()
    return t.view(torch.int16 if t.dtype == torch.float16 else torch.int32)


def slab_in(slab, gs, dev):
    """[G, N, H, W, 32] fp16 -> device groups gs elements apart, NaN between and around them"""
    return In(slab, dev, n=(slab.shape[0] - 1) * gs + slab[0].numel(), at=[(g * gs, slab[g]) for g in range(slab.shape[0])])


def slab_out(flat, Gr, gs, shape):
    """the groups of a flat destination -> [G, *shape, 32]; the gaps between them must hold the sentinel"""
    n = int(np.prod(shape)) * 32
    for g in range(Gr - 1):
        assert (flat[g * gs + n:(g + 1) * gs] == SENT).all(), "wrote into the gap between two groups"
    return torch.stack([flat[g * gs:g * gs + n].view(*shape, 32) for g in range(Gr)])


def exact(family):
    C.MEASURED.setdefault("glue: " + family, [0.0, 0.0])


def within(got, ref, e32, extra, what, family, rounding):
    if not rounding and e32 == 0.0 and np.isscalar(extra) and extra == 0.0:
        # the float32 evaluation reproduces float64 on every value of the family (sums of short operands): the bound is 0 and 0 / 0 is no ratio -- the values must be equal
        assert torch.equal(got.double(), ref.double()), f"{what}: e32 0 (float32 is exact here), yet {int((got.double() != ref.double()).sum())} values differ from float64"
        exact(family)
        return 0.0
    return C.assert_within_fp16_rounding(got, ref, e32, extra=extra, what=what, family="glue: " + family, rounding=rounding)


# ------------------------------------------------------------------------------------------------ PAN: pre, upsample, final, slab pair
@pytest.mark.parametrize("Cc", (1, 3, 8))
def test_pan_pre_bit_for_bit(dev, Cc):
    def run(x, dt):
        N, _, H, W = x.shape
        xin, out = In(x, dev), Out(N * H * W * 32, torch.float16, dev)
        L.check(L.lib.innfer_pan_pre(xin.ptr, dt, N, Cc, H, W, out.ptr, None))
        got = out.cpu().view(N, H, W, 32)
        assert xin.same()
        return got
    for H, W in ((1, 1), (5, 7), (17, 33)):
        for dt in (F16, F32):
            x = G.rand((3, Cc, H, W), H * W + Cc, -4, 4).to(TD[dt])
            got = run(x, dt)
            assert torch.equal(bits(got), bits(G.to_group(x.half()))), (H, W, dt)          # (fp32 input: round to nearest even, as .half(); pad channels zero)
            for n in range(3):
                assert torch.equal(bits(run(x[n:n + 1], dt)[0]), bits(got[n])), (H, W, dt, n)
    exact("pan_pre")


def _ups16(dev, x, f, bil, gap=GAP):
    """pan_upsample on the slab of x [N, C, h, w] fp16 (C padded with zero channels to whole groups) -> [N, Gr * 32, f h, f w] fp16"""
    N, _, h, w = x.shape
    s = G.to_slab(x)
    Gr = s.shape[0]
    gi, go = N * h * w * 32 + gap, N * f * h * f * w * 32 + gap
    xin, out = slab_in(s, gi, dev), Out((Gr - 1) * go + N * f * h * f * w * 32, torch.float16, dev)
    L.check(L.lib.innfer_pan_upsample(xin.ptr, F16, N, Gr * 32, h, w, f, bil, gi, out.ptr, go, None))
    got = G.from_slab(slab_out(out.cpu(), Gr, go, (N, f * h, f * w)))
    assert xin.same()
    return got


@pytest.mark.parametrize("f", (2, 3))
@pytest.mark.parametrize("Cc", (24, 40))
def test_pan_upsample_slabs(dev, Cc, f):
    """one group (unf = 24 channels) and two (nf = 40); nearest bit for bit, bilinear under ulp16 / 2 + 8 e32"""
    for h, w in G.UPS_SIZES:
        x = G.rand((2, Cc, h, w), 100 * h + w + Cc).half()
        for bil in (0, 1):
            got = _ups16(dev, x, f, bil)
            assert (got[:, Cc:] == 0).all(), "pad channels"
            if bil:
                ref, e32, _ = G.judge_upsample(x.float(), f)
                within(got[:, :Cc], ref, e32, 0.0, f"pan_upsample bilinear x{f} C{Cc} {h}x{w}", "pan_upsample, bilinear", True)
            else:
                assert torch.equal(bits(got[:, :Cc]), bits(G.upsample_ref(x, f, False).half())), (h, w, f)
            for n in range(2):
                assert torch.equal(bits(_ups16(dev, x[n:n + 1], f, bil)[0]), bits(got[n])), (h, w, f, bil, n)
    exact("pan_upsample / f32_nearest_up / ppon_upsample3, nearest")


@pytest.mark.parametrize("f", (2, 3))
def test_pan_upsample_fp32(dev, f):
    """f32_upsample_launch: f32_nearest_up bit for bit, f32_bilinear_up under 8 e32"""
    def run(x, bil):
        N, Cc, h, w = x.shape
        xin, out = In(x, dev), Out(N * Cc * f * h * f * w, torch.float32, dev)
        L.check(L.lib.innfer_pan_upsample(xin.ptr, F32, N, Cc, h, w, f, bil, 0, out.ptr, 0, None))
        got = out.cpu().view(N, Cc, f * h, f * w)
        assert xin.same()
        return got
    xs = [G.rand((2, 5, h, w), 100 * h + w) for h, w in G.UPS_SIZES]
    e_fam = max(G.judge_upsample(x, f)[1] for x in xs)
    for x in xs:
        for bil in (0, 1):
            got = run(x, bil)
            if bil:
                within(got, G.upsample_ref(x, f, True), e_fam, 0.0, f"f32_bilinear_up x{f} {tuple(x.shape[2:])}", "f32_bilinear_up", False)
            else:
                assert torch.equal(bits(got), bits(G.upsample_ref(x, f, False).float()))
            for n in range(2):
                assert torch.equal(bits(run(x[n:n + 1], bil)[0]), bits(got[n]))


def _final(dev, raw, x, s, xdt, odt, form):
    N, Cc, H, W = x.shape
    rin, xin, out = In(raw, dev), In(x, dev), Out(N * Cc * s * H * s * W, TD[odt], dev)
    L.check(L.lib.innfer_pan_final(rin.ptr, Cc, xin.ptr, xdt, N, H, W, s, out.ptr, odt, form, None))
    got = out.cpu().view(N, Cc, s * H, s * W)
    assert rin.same() and xin.same()
    return got


@pytest.mark.parametrize("s", (1, 2, 3, 4))
def test_pan_final(dev, s):
    """pan_final / pan_final_x4: out = raw + bilinear(x, align_corners=True); where the output width is a multiple of 4 the two forms give the same bits"""
    sizes = G.FINAL_SIZES + (((3, 4),) if s == 3 else ())
    for Cc in (1, 3, 4):
        for xdt in (F16, F32):
            cases = []
            for H, W in sizes:
                x = G.rand((2, Cc, H, W), 10 * H + W + Cc).to(TD[xdt])
                raw = G.rand((2, Cc, s * H, s * W), s + Cc)
                cases.append((x, raw) + G.judge_final(raw, x.float(), s)[:2])
            e_fam = max(c[3] for c in cases)
            for x, raw, ref, e32 in cases:
                H, W = x.shape[2:]
                for odt in (F16, F32):
                    what = f"pan_final x{s} C{Cc} {H}x{W} x{'16' if xdt == F16 else '32'} out{'16' if odt == F16 else '32'}"
                    got = _final(dev, raw, x, s, xdt, odt, -1)
                    if odt == F16:
                        within(got, ref, e32, 0.0, what, "pan_final / pan_final_x4, fp16 out", True)
                    else:
                        within(got, ref, e_fam, 0.0, what, "pan_final / pan_final_x4, fp32 out", False)
                    g0 = _final(dev, raw, x, s, xdt, odt, 0)
                    if (W * s) % 4 == 0:
                        g1 = _final(dev, raw, x, s, xdt, odt, 1)
                        assert torch.equal(bits(g1), bits(got)), what + ": form -1 is not the strip form"
                        ndiff = int((bits(g0) != bits(g1)).sum())
                        assert ndiff == 0, f"{what}: the one-pixel and the strip form differ in {ndiff} of {g0.numel()} values"
                    else:
                        assert torch.equal(bits(g0), bits(got)), what + ": form -1 is not the one-pixel form"
                    for n in range(2):
                        assert torch.equal(bits(_final(dev, raw[n:n + 1], x[n:n + 1], s, xdt, odt, -1)[0]), bits(got[n])), (what, n)
    exact("pan_final form 0 == form 1")


def test_pan_slab_pair_bit_for_bit(dev):
    def run(x):
        N, Cc, H, W = x.shape
        px = N * H * W
        lo = 2 * px * 32 + GAP
        xin, out = In(x, dev), Out(lo + 2 * px * 32, torch.float16, dev)
        L.check(L.lib.innfer_pan_slab_pair(xin.ptr, N, Cc, H, W, out.ptr, lo, None))
        flat = out.cpu()
        assert xin.same() and (flat[2 * px * 32:lo] == SENT).all(), "wrote between the halves"
        return flat[:2 * px * 32].view(2, N, H, W, 32), flat[lo:].view(2, N, H, W, 32)
    for H, W in ((1, 1), (5, 7)):
        x = G.slab_pair_values((2, 40, H, W), H * W)
        hi, lo = run(x)
        rh, rl = G.slab_pair_ref(x)
        assert torch.equal(bits(hi), bits(G.to_slab(rh))) and torch.equal(bits(lo), bits(G.to_slab(rl))), (H, W)          # pad channels 40 .. 63: zero in both halves
        assert (G.from_slab(hi)[:, 40:] == 0).all() and (G.from_slab(lo)[:, 40:] == 0).all()
        for n in range(2):
            h1, l1 = run(x[n:n + 1])
            assert torch.equal(bits(h1[:, 0]), bits(hi[:, n])) and torch.equal(bits(l1[:, 0]), bits(lo[:, n]))
    exact("pan_nchw_to_slab_pair")


# ------------------------------------------------------------------------------------------------ PPON: nearest 3x, axpy, alpha
def test_ppon_upsample3_bit_for_bit(dev):
    def run(x):
        N, _, H, W = x.shape
        gi, go = N * H * W * 32 + GAP, N * 9 * H * W * 32 + GAP
        xin, out = slab_in(G.to_slab(x), gi, dev), Out(go + N * 9 * H * W * 32, torch.float16, dev)
        L.check(L.lib.innfer_ppon_upsample3(xin.ptr, gi, out.ptr, go, N, H, W, None))
        got = G.from_slab(slab_out(out.cpu(), 2, go, (N, 3 * H, 3 * W)))
        assert xin.same()
        return got
    for H, W in ((1, 1), (2, 3), (5, 7)):
        x = G.rand((2, 64, H, W), H * W).half()
        got = run(x)
        assert torch.equal(bits(got), bits(G.upsample_ref(x, 3, False).half())), (H, W)
        for n in range(2):
            assert torch.equal(bits(run(x[n:n + 1])[0]), bits(got[n]))


@pytest.mark.parametrize("dt,form", ((F16, 0), (F32, 0), (F32, 1)), ids=("ppon_axpy-fp16", "ppon_axpy-fp32", "f32_axpy"))
def test_ppon_axpy(dev, dt, form):
    """out = a x + y under u (|a x| + |a x + y|) (+ ulp16 / 2 for the fp16 store), x aliasing the output (as the forward calls it) and not"""
    for n in (1, 255, 256, 257, 3 * 10 * 12 * 16):
        x, y = G.rand((n,), n).to(TD[dt]), G.rand((n,), n + 1).to(TD[dt])
        for a in (1.0, 0.5, -0.25, 0.0):
            ref, extra = G.axpy_ref(x.float(), y.float(), a), G.axpy_extra(x.float(), y.float(), a)
            for alias in (0, 1):
                yin, out = In(y, dev), Out(n, TD[dt], dev)
                if alias:
                    out.v.copy_(x)
                    xptr = out.ptr
                else:
                    xin = In(x, dev)
                    xptr = xin.ptr
                L.check(L.lib.innfer_ppon_axpy(xptr, yin.ptr, out.ptr, a, n, dt, form, None))
                got = out.cpu()
                assert yin.same() and (alias or xin.same())
                within(got, ref, 0.0, extra, f"axpy n={n} a={a} alias={alias}", "ppon_axpy" if form == 0 else "f32_axpy", dt == F16)


@pytest.mark.parametrize("dt", (torch.float16, torch.float32), ids=("fp16", "fp32"))
def test_ppon_alpha_network_level(dev, dt):
    """Two engines with the same weights, alpha = 1 and alpha = 0.5: out_c and out_s bit-equal; out_p(0.5) - out_s against 0.5 (out_p(1) - out_s).  With p = the head's
    result, out_p(a) = store(a p + out_s): each is within u (|a p| + |a p + s|) (+ ulp16 / 2 when stored as fp16) of its exact value, and the fp16 engine's p is the
    same fp16 tensor in both, so the difference is bounded by the alpha = 0.5 launch's allowance plus half the alpha = 1 launch's."""
    from innfer_amd import synth
    from innfer_amd.architectures.PPON_arch import PPON
    outs = {}
    sd = None
    for alpha in (1.0, 0.5):
        net = PPON(3, 64, 2, 3, upscale=4, alpha=alpha)
        if sd is None:
            sd = {k: torch.from_numpy(v) for k, v in synth.fill_state_dict({k: tuple(t.shape) for k, t in net.state_dict().items()}, 5).items()}
        net.load_state_dict(sd, strict=True)
        net = net.to(dev).eval()
        x = torch.from_numpy(synth.uniform((1, 3, 10, 12), 31)).to(dev).to(dt)
        outs[alpha] = [o.cpu() for o in net(x)]
        del net
    (c1, s1, p1), (c5, s5, p5) = outs[1.0], outs[0.5]
    assert torch.equal(bits(c1), bits(c5)) and torch.equal(bits(s1), bits(s5)), "alpha changed out_c / out_s"
    assert not torch.equal(p1, p5), "alpha has no effect on out_p"
    s, p1, p5 = s1.double(), p1.double(), p5.double()
    px = p1 - s                                             # the head's result, to within the alpha = 1 launch's allowance
    r = (C.ulp16(p1) / 2 if dt == torch.float16 else 0.0), (C.ulp16(p5) / 2 if dt == torch.float16 else 0.0)
    bound = 0.5 * (r[0] + G.U * (px.abs() + p1.abs())) + r[1] + G.U * (0.5 * px.abs() + p5.abs())
    ratio = ((p5 - s) - 0.5 * px).abs() / bound
    print(f"[glue] PPON alpha, network level ({dt}): worst err / bound {ratio.max().item():.3f}")
    m = C.MEASURED.setdefault("glue: PPON alpha, network level", [0.0, 0.0])
    m[1] = max(m[1], ratio.max().item())
    assert ratio.max().item() <= 1.0, ratio.max().item()


# ------------------------------------------------------------------------------------------------ WBC UNet: pre, upadd
def test_wbc_pre_bit_for_bit(dev):
    def run(x, dt):
        N, Cc, H, W = x.shape
        xin, out = In(x, dev), Out(N * H * W * 32, torch.float16, dev)
        L.check(L.lib.innfer_wbc_pre(xin.ptr, dt, N, Cc, H, W, out.ptr, None))
        got = out.cpu().view(N, H, W, 32)
        assert xin.same()
        return got
    for W in (1, 3, 4, 7, 33):
        for H in (1, 5):
            for dt in (F16, F32):
                x = G.rand((2, 3, H, W), 10 * H + W, -4, 4).to(TD[dt])
                got = run(x, dt)
                assert torch.equal(bits(got), bits(G.wb_pre_ref(x.half()))), (H, W, dt)
                assert (got[..., 21:] == 0).all()
                for n in range(2):
                    assert torch.equal(bits(run(x[n:n + 1], dt)[0]), bits(got[n]))
    exact("wb_pre")


@pytest.mark.parametrize("Cc", (32, 64))
@pytest.mark.parametrize("tf", (0, 1), ids=("pt", "tf"))
def test_wbc_upadd_slabs(dev, tf, Cc):
    def run(src, skip):
        N, _, h, w = src.shape
        sin, kin, out = In(G.to_slab(src), dev), In(G.to_slab(skip), dev), Out(N * 4 * h * w * Cc, torch.float16, dev)
        L.check(L.lib.innfer_wbc_upadd(sin.ptr, kin.ptr, F16, N, Cc, h, w, tf, out.ptr, None))
        got = G.from_slab(out.cpu().view(Cc // 32, N, 2 * h, 2 * w, 32))
        assert sin.same() and kin.same()
        return got
    for h, w in G.UPADD_SIZES:
        src, skip = G.rand((2, Cc, h, w), 10 * h + w).half(), G.rand((2, Cc, 2 * h, 2 * w), 10 * h + w + 1).half()
        got = run(src, skip)
        if tf:
            assert torch.equal(bits(got), bits(G.upadd16_ref(src, skip, 1)[0])), (h, w)
        else:
            ref, e32, extra = G.judge_upadd_pt(src.float(), skip.float(), True)
            within(got, ref, e32, extra, f"wb_upadd pt C{Cc} {h}x{w}", "wb_upadd, pt mode", True)
        for n in range(2):
            assert torch.equal(bits(run(src[n:n + 1], skip[n:n + 1])[0]), bits(got[n]))
    if tf:
        exact("wb_upadd, tf mode")


@pytest.mark.parametrize("tf", (0, 1), ids=("pt", "tf"))
def test_wbc_upadd_fp32(dev, tf):
    def run(src, skip):
        N, Cc, h, w = src.shape
        sin, kin, out = In(src, dev), In(skip, dev), Out(N * Cc * 4 * h * w, torch.float32, dev)
        L.check(L.lib.innfer_wbc_upadd(sin.ptr, kin.ptr, F32, N, Cc, h, w, tf, out.ptr, None))
        got = out.cpu().view(N, Cc, 2 * h, 2 * w)
        assert sin.same() and kin.same()
        return got
    cases = []
    for h, w in G.UPADD_SIZES:
        src, skip = G.rand((2, 5, h, w), 10 * h + w), G.rand((2, 5, 2 * h, 2 * w), 10 * h + w + 1)
        if tf:
            ref = G.tf_up_ref(src.double()) + skip.double()
            e32 = float(((G.tf_up_ref(src) + skip).double() - ref).abs().max())
        else:
            ref, e32, _ = G.judge_upadd_pt(src, skip, False)
        cases.append((src, skip, ref, e32))
    e_fam = max(c[3] for c in cases)
    for src, skip, ref, _ in cases:
        got = run(src, skip)
        within(got, ref, e_fam, 0.0, f"f32_upadd tf={tf} {tuple(src.shape[2:])}", "f32_upadd", False)
        for n in range(2):
            assert torch.equal(bits(run(src[n:n + 1], skip[n:n + 1])[0]), bits(got[n]))


# ------------------------------------------------------------------------------------------------ fp32-mode passes
def test_f32_prefix_lrelu(dev):
    def run(t):
        N, Cc, hw = t.shape
        out = Out(t.numel(), torch.float32, dev)          # in place
        out.v.copy_(t.reshape(-1))
        L.check(L.lib.innfer_f32_prefix_lrelu(out.ptr, N, 8, Cc // 8, hw, None))
        return out.cpu().view(N, Cc, hw)
    cases = []
    for hw in (1, 35):
        t = G.rand((2, 8 * 32, hw), hw)
        t[:, ::5] = 0
        t[:, 3::32] = t[:, 3::32].abs()
        ref, extra = G.prefix_lrelu_ref(t, 8)
        cases.append((t, ref, extra, float((torch.from_numpy(G.prefix_lrelu_model(t, 8)).double() - ref).abs().max())))
    e_fam = max(c[3] for c in cases)
    for t, ref, extra, _ in cases:
        got = run(t)
        within(got, ref, e_fam, extra, f"f32_prefix_lrelu hw={t.shape[2]}", "f32_prefix_lrelu", False)
        for n in range(2):
            assert torch.equal(bits(run(t[n:n + 1])[0]), bits(got[n]))


@pytest.mark.parametrize("act", range(5))
def test_f32_act_copy(dev, act):
    """strides wider than per_image on both sides: the input's gaps are NaN, the output's must keep the sentinel"""
    N, per, ins, ons = 3, 37, 50, 45
    x = G.rand((N, per), 9 + act, -4, 4)
    x[:, ::6] = 0
    xin = In(x, dev, n=(N - 1) * ins + per, at=[(n * ins, x[n]) for n in range(N)])
    out = Out((N - 1) * ons + per, torch.float32, dev)
    L.check(L.lib.innfer_f32_act_copy(xin.ptr, ins, out.ptr, ons, per, N, act, None))
    flat = out.cpu()
    assert xin.same()
    for n in range(N - 1):
        assert (flat[n * ons + per:(n + 1) * ons] == SENT).all(), "wrote between two images"
    got = torch.stack([flat[n * ons:n * ons + per] for n in range(N)])
    if act < 3:
        assert torch.equal(bits(got), bits(G.act_ref(x, act))), act
        exact("f32_act_copy, none / LeakyReLU / ReLU")
    else:
        ref = G.act_ref(x.double(), act)
        e32 = float((G.act_ref(x, act).double() - ref).abs().max())
        within(got, ref, e32, C.TRANS, f"f32_act_copy act {act}", "f32_act_copy, tanh / sigmoid", False)


# ------------------------------------------------------------------------------------------------ guided filter
def _gf(dev, x, y, dt, N, Cc, ks, eps, xhr=None, r1=False):
    """x, y [N * C, H, W] float32 holding fp16 values; r1: innfer_guided_filter (gf_ab + gf_out), else innfer_guided_filter_ex"""
    H, W = x.shape[-2:]
    xin, yin = In(x.to(TD[dt]), dev), In(y.to(TD[dt]), dev)
    nb = L.lib.innfer_guided_filter_workspace_bytes(N, Cc, H, W)
    ws = torch.empty(nb, dtype=torch.uint8, device=dev)
    if r1:
        out = Out(x.numel(), TD[dt], dev)
        L.check(L.lib.innfer_guided_filter(xin.ptr, yin.ptr, dt, N, Cc, H, W, eps, out.ptr, ws.data_ptr(), nb, None))
        hin = None
    elif xhr is None:
        out = Out(x.numel(), TD[dt], dev)
        L.check(L.lib.innfer_guided_filter_ex(xin.ptr, yin.ptr, dt, N, Cc, H, W, ks, eps, None, 0, 0, out.ptr, ws.data_ptr(), nb, None))
        hin = None
    else:
        hin, out = In(xhr.to(TD[dt]), dev), Out(xhr.numel(), TD[dt], dev)
        L.check(L.lib.innfer_guided_filter_ex(xin.ptr, yin.ptr, dt, N, Cc, H, W, ks, eps, hin.ptr, xhr.shape[-2], xhr.shape[-1], out.ptr, ws.data_ptr(), nb, None))
    got = out.cpu().view((xhr if xhr is not None else x).shape)
    assert xin.same() and yin.same() and (hin is None or hin.same())
    return got


@pytest.mark.parametrize("dt", (F16, F32), ids=("fp16", "fp32"))
@pytest.mark.parametrize("fam", G.GF_FAMILIES)
def test_guided_filter_r1(dev, fam, dt):
    """innfer_guided_filter, the exported r = 1 entry (gf_ab + gf_out): ulp16 / 2 + 8 e_model, e_model from the float32 model in the kernel's order"""
    for eps in (5e-3, 1e-2):
        for P, N, Cc in ((1, 1, 1), (6, 2, 3)):
            cases = []
            for H, W in G.GF_SIZES:
                x, y = G.gf_operands(fam, P, H, W, 7 * H + W + P)
                cases.append((x, y) + G.judge_gf(x, y, 3, eps)[:2])
            e_fam = max(c[3] for c in cases)
            for x, y, ref, e in cases:
                got = _gf(dev, x, y, dt, N, Cc, 3, eps, r1=True)
                within(got, ref, e if dt == F16 else e_fam, 0.0, f"guided_filter r=1 {fam} {tuple(x.shape)} eps {eps}", "guided filter r = 1 (gf_ab + gf_out)", dt == F16)
                if N > 1:
                    for n in range(N):
                        assert torch.equal(bits(_gf(dev, x[n * Cc:(n + 1) * Cc], y[n * Cc:(n + 1) * Cc], dt, 1, Cc, 3, eps, r1=True)), bits(got[n * Cc:(n + 1) * Cc]))


@pytest.mark.parametrize("dt", (F16, F32), ids=("fp16", "fp32"))
@pytest.mark.parametrize("ks", (1, 3, 5, 7))
def test_guided_filter_ex(dev, ks, dt):
    """innfer_guided_filter_ex: gf_ab_r + gf_out_r (regular) and gf_ab_r + gf_out_fast (x_HR at 2H x 2W, H x W, (2H + 1) x (3W - 2) and 1 x 1)"""
    r = ks // 2
    N, Cc = 2, 2
    for fam in G.GF_FAMILIES:
        for eps in (5e-3, 1e-2, 1e-4):
            for mode in range(5):
                cases = []
                for H, W in ((r + 1, r + 1), (5, 7), (17, 23)):
                    x, y = G.gf_operands(fam, N * Cc, H, W, 7 * H + W + ks)
                    xhr = None
                    if mode:
                        Hh, Wh = ((2 * H, 2 * W), (H, W), (2 * H + 1, 3 * W - 2), (1, 1))[mode - 1]
                        xhr = G.gf_operands(fam, N * Cc, Hh, Wh, 3 * H + W + mode)[0]          # the high-resolution guidance is of the low-resolution one's kind
                    cases.append((x, y, xhr) + G.judge_gf(x, y, ks, eps, xhr)[:2])
                e_fam = max(c[4] for c in cases)
                for x, y, xhr, ref, e in cases:
                    got = _gf(dev, x, y, dt, N, Cc, ks, eps, xhr)
                    what = f"guided_filter_ex ks {ks} {fam} {tuple(x.shape[1:])} eps {eps} " + (f"fast -> {tuple(xhr.shape[1:])}" if mode else "regular")
                    within(got, ref, e if dt == F16 else e_fam, 0.0, what, "guided filter ks 1 .. 7, " + ("fast" if mode else "regular"), dt == F16)
                    if fam == "noise" and eps == 1e-2:
                        for n in range(N):
                            sl = slice(n * Cc, (n + 1) * Cc)
                            assert torch.equal(bits(_gf(dev, x[sl], y[sl], dt, 1, Cc, ks, eps, None if xhr is None else xhr[sl])), bits(got[sl])), what


# ------------------------------------------------------------------------------------------------ filter2D
@pytest.mark.parametrize("dt", (F16, F32), ids=("fp16", "fp32"))
@pytest.mark.parametrize("border", range(4), ids=G.BORDERS)
def test_filter2d(dev, border, dt):
    """k_filter2d under kH kW u sum |k v| (the fmaf chain) + 8 e32 (+ ulp16 / 2): every border mode with centred, even and off-centre kernels on small odd planes"""
    def run(x, k, pl, pt):
        P, H, W = x.shape
        xin, kin, out = In(x.to(TD[dt]), dev), In(k, dev), Out(x.numel(), TD[dt], dev)
        L.check(L.lib.innfer_filter2d(xin.ptr, dt, P, H, W, kin.ptr, k.shape[0], k.shape[1], pl, pt, border, out.ptr, None))
        got = out.cpu().view(P, H, W)
        assert xin.same() and kin.same()
        return got
    cases = [(H, W, kH, kW, pl, pt) for H, W in G.F2D_PLANES for kH, kW, pl, pt in G.F2D_KERNELS]
    if border == 3:
        cases += [(2, 2, 3, 5, 2, 1), (3, 2, 4, 5, 2, 3)]          # circular with pad == size
    ran = 0
    for H, W, kH, kW, pl, pt in cases:
        if not G.f2d_accepts(H, W, kH, kW, pl, pt, border):
            continue
        k = G.f2d_kernel(kH, kW, 8 * kH + kW)
        for P in (1, 6):
            x = G.rand((P, H, W), H * W + P).half().float()
            ref, e32, extra = G.judge_f2d(x, k, pl, pt, border)
            got = run(x, k, pl, pt)
            within(got, ref, e32, extra, f"filter2d {G.BORDERS[border]} {kH}x{kW} pad ({pl}, {pt}) on {P}x{H}x{W}", "k_filter2d", dt == F16)
            if P > 1:
                assert torch.equal(bits(run(x[2:3], k, pl, pt)[0]), bits(got[2]))
            ran += 1
    assert ran >= (30 if border != 1 else 20), ran


# ------------------------------------------------------------------------------------------------ the record
def test_report():
    """(runs last in this file) per family: the largest e32 / e_model and the worst err / bound over every element of every case"""
    rows = sorted((k[6:], v) for k, v in C.MEASURED.items() if k.startswith("glue: "))
    print("\n    family                                                      e32 / e_model   worst err / bound")
    for name, (e, w) in rows:
        print(f"    {name:<60}{(f'{e:.1e}' if e else ('exact' if not w else '(derived)')):<16}{(f'{w:.3f}' if w else 'bit-identical')}")
    assert len(rows) >= 15, [r[0] for r in rows]
