"""The pass kernels of the pix2pix UNet (csrc/unet.hip) and the CycleGAN ResNet (csrc/resnet.hip), launch by launch, against float64 (needs an MI355X:
`pytest -m gpu`).

Under test, each through its single-launch entry point of ABI 123 -- which calls the launcher the network calls, so grid, block and instantiation are the
network's: unet_pre, unet_pre_patch, rn_pre (bit for bit); unet_post, unet_post_slab, rn_post, rn_post_slab, rn_post_slab_pad + rn_zero_ring (placement bit for
bit, values under the derived bound); all five instantiations of unet_deep_post; unet_first_mfma<f16 | float>; rn_sum9_tanh, unet_final, rn_final.
References, case lists, comparators and where every bound comes from: tests/_pass_kernels_ref.py (checked on the CPU by tests/test_pass_kernels_cpu.py).

Every buffer a kernel writes is prefilled with a sentinel and sits between sentinel guards; every gathered input sits between NaN guards.

Pass kernels of the UNet / ResNet engines -- largest e32 or e_emul of the family's cases; worst err / bound over every element of every case on the MI355X:
    family                                                   e32 / e_emul     worst err / bound
    unet_pre, unet_pre_patch, rn_pre                         exact            bit-identical
    rn_post_slab_pad + rn_zero_ring, placement               exact            bit-identical
    unet_post, unet_post_slab                                (derived)        1.000
    rn_post, rn_post_slab, rn_post_slab_pad values           (derived)        1.000
    unet_deep_post, train mode (y metric, 8 x e_emul)        7.9e-07          0.115
    unet_deep_post, eval / bias / none                       (derived)        0.999
    unet_first_mfma                                          3.2e-06          0.996
    rn_sum9_tanh                                             1.6e-07          0.993
    unet_final, rn_final                                     7.3e-08          0.996
(the fp16 stores sit at 1.0 because the storage rounding alone fills the bound, as in tests/test_gpu_conv_forms.py)
"""
import numpy as np
import pytest
import torch

import _pass_kernels_ref as R
import innfer_amd.lib as L

pytestmark = pytest.mark.gpu

GUARD = 4096                  # elements of sentinel in front of and behind every buffer a kernel writes
SENT16, SENTF = 1234.0, 777.0
F16, F32 = 0, 1               # innfer_dtype


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _guarded(n, dtype, fill, dev, guard=GUARD):
    buf = torch.full((guard + n + guard,), fill, dtype=dtype, device=dev)
    return buf, buf[guard:guard + n]


def _intact(buf, n, fill, guard=GUARD):
    return bool((buf[:guard] == fill).all().item() and (buf[guard + n:] == fill).all().item())


def _f(t):
    return None if t is None else t.data_ptr()


def _input(t, dev):
    """A gathered input on the device between NaN guards (floating types)"""
    t = t.contiguous()
    _, v = _guarded(t.numel(), t.dtype, float("nan"), dev)
    v.copy_(t.reshape(-1))
    return v


def _dev(a, dev):
    return None if a is None else torch.as_tensor(a).contiguous().to(dev)


_REPORT = {}


def _note(family, ratio, e=None):
    w, we = _REPORT.get(family, (0.0, 0.0))
    _REPORT[family] = (max(w, ratio), max(we, e or 0.0))
    return ratio


class _View:
    """A destination view: C channels at channel offset coff of a `wide`-channel fp16 slab over N * HW pixels, sentinel-filled and guarded"""

    def __init__(self, dev, N, HW, Cc, coff=0, wide=None):
        self.N, self.HW, self.C, self.coff = N, HW, Cc, coff
        self.wide = wide or -(-Cc // 32) * 32
        self.gs = N * HW * 32
        self.n = (self.wide // 32) * self.gs
        self.buf, self.v = _guarded(self.n, torch.float16, SENT16, dev)

    def args(self, a):
        return [self.v.data_ptr(), self.gs, self.coff, a]

    def read(self, written=None):
        """-> what the kernel wrote [N, C, HW] (cpu fp16); the guards, the neighbouring channels and (written < C: the channels beyond) keep the sentinel"""
        assert _intact(self.buf, self.n, SENT16), "wrote outside the destination slab"
        full = R.from_slab(self.v.view(self.wide // 32, self.N, self.HW, 1, 32)).cpu()[..., 0]
        w = self.C if written is None else written
        assert (full[:, :self.coff] == SENT16).all() and (full[:, self.coff + w:] == SENT16).all(), "wrote outside its channels"
        got = full[:, self.coff:self.coff + w]
        assert (got != SENT16).all(), "left part of its output unwritten"
        return got.contiguous()


NO = [None, 0, 0, 0]


def _check_pass(got, x, alpha, shift, a, res=None, extra=0.0):
    ref, mag = R.pass_ref(x, alpha, shift, a, res)
    return R.worst_ratio(got.double().numpy(), ref, R.pass_bound(ref, got.double().numpy(), mag, extra))


# ------------------------------------------------------------------------------------------------ exact kernels
@pytest.mark.parametrize("Cc", (1, 3, 32))
def test_unet_pre_bit_for_bit(dev, Cc):
    for HW in (1, 255, 257):
        for N in (1, 3):
            for dt in (F16, F32):
                x = torch.randn(N, Cc, 1, HW, generator=torch.Generator().manual_seed(HW + N))
                x = x.half() if dt == F16 else x
                obuf, out = _guarded(N * HW * 32, torch.float16, SENT16, dev)
                xin = _input(x, dev)
                L.check(L.lib.innfer_unet_pre(xin.data_ptr(), dt, Cc, 1, HW, N, out.data_ptr(), N * HW * 32, 0, None))
                torch.cuda.synchronize()
                assert _intact(obuf, N * HW * 32, SENT16)
                assert torch.equal(R.bits16(out.view(N, HW, 32).cpu()), R.bits16(R.unet_pre_ref(x.float()).half())), (HW, N, dt)
    _note("unet_pre, unet_pre_patch, rn_pre", 0.0)


@pytest.mark.parametrize("Cc", (1, 3, 4))
def test_unet_pre_patch_bit_for_bit(dev, Cc):
    for H, W in ((2, 2), (6, 10), (32, 34)):
        for N in (1, 2):
            for dt in (F16, F32):
                x = torch.randn(N, Cc, H, W, generator=torch.Generator().manual_seed(H + W + N))
                x = x.half() if dt == F16 else x
                M = N * (H // 2) * (W // 2)
                obuf, out = _guarded(2 * M * 32, torch.float16, SENT16, dev)
                xin = _input(x, dev)
                L.check(L.lib.innfer_unet_pre(xin.data_ptr(), dt, Cc, H, W, N, out.data_ptr(), M * 32, 1, None))
                torch.cuda.synchronize()
                assert _intact(obuf, 2 * M * 32, SENT16)
                got = R.from_slab(out.view(2, N, H // 2, W // 2, 32).cpu())
                assert torch.equal(R.bits16(got), R.bits16(R.unet_patch(x.half().float()).half())), (H, W, N, dt)


@pytest.mark.parametrize("Cc,patch", ((1, 1), (3, 1), (4, 1), (5, 0), (32, 0)))
def test_resnet_pre_bit_for_bit(dev, Cc, patch):
    for H, W in ((4, 4), (5, 7), (9, 33) if patch else (3, 33)):
        for N in (1, 2):
            for dt in (F16, F32):
                x = torch.randn(N, Cc, H, W, generator=torch.Generator().manual_seed(H + W + N))
                x = x.half() if dt == F16 else x
                n = N * H * W * 32
                obuf, out = _guarded(n, torch.float16, SENT16, dev)
                xin = _input(x, dev)
                L.check(L.lib.innfer_resnet_pre(xin.data_ptr(), dt, Cc, H, W, N, out.data_ptr(), patch, None))
                torch.cuda.synchronize()
                assert _intact(obuf, n, SENT16)
                got = R.from_slab(out.view(1, N, H, W, 32).cpu())
                want = R.row_patch(x.half().float()) if patch else R.unet_pre_ref(x.half().float()).view(N, H, W, 32).permute(0, 3, 1, 2)
                assert torch.equal(R.bits16(got), R.bits16(want.half())), (H, W, N, dt)


def _run_pad(dev, H, W, Cc, N, seed=0):
    """rn_zero_ring + rn_post_slab_pad on a random slab -> (padded result [N, C, H + 8, W + 8] cpu fp16, x [N, C, H, W] float64, alpha, shift [N, C, 1, 1] float64)"""
    rng = np.random.default_rng(seed + 100 * H + W + Cc)
    x = torch.from_numpy(rng.normal(0.2, 1.0, (N, Cc, H, W))).half()
    al, sh = rng.uniform(0.5, 2.0, (N, Cc)).astype(np.float32), rng.uniform(-1, 1, (N, Cc)).astype(np.float32)
    src = _input(R.to_slab(x), dev)
    G, Hp, Wp = Cc // 32, H + 8, W + 8
    gd = N * Hp * Wp * 32
    dbuf, dst = _guarded(G * gd, torch.float16, SENT16, dev)
    ad, sd = _dev(al, dev), _dev(sh, dev)
    L.check(L.lib.innfer_resnet_post_slab_pad(src.data_ptr(), N * H * W * 32, Cc, H, W, N, ad.data_ptr(), sd.data_ptr(), 1, dst.data_ptr(), gd, None))
    torch.cuda.synchronize()
    assert _intact(dbuf, G * gd, SENT16), "wrote outside the padded slab"
    return R.from_slab(dst.view(G, N, Hp, Wp, 32).cpu()), x.double().numpy(), al.astype(np.float64)[..., None, None], sh.astype(np.float64)[..., None, None]


@pytest.mark.parametrize("H,W", ((4, 4), (4, 9), (5, 5), (7, 4), (8, 8), (16, 21)))
def test_resnet_post_slab_pad(dev, H, W):
    """Placement: every element of the (H + 8) x (W + 8) slab is the kernel's own value at the source pixel ReflectionPad2d(3) names, zero on the outer ring, no
    sentinel left; values: the image itself under the derived bound."""
    for Cc in (32, 64):
        for N in (1, 2):
            got, x, al, sh = _run_pad(dev, H, W, Cc, N)
            assert (got != SENT16).all(), "part of the padded slab was never written"
            own = got[:, :, 4:4 + H, 4:4 + W]
            assert torch.equal(R.bits16(got), R.bits16(torch.from_numpy(R.pad_ref(own.numpy())))), (H, W, Cc, N)
            assert (got[:, :, 0] == 0).all() and (got[:, :, -1] == 0).all() and (got[:, :, :, 0] == 0).all() and (got[:, :, :, -1] == 0).all()
            r = _note("rn_post, rn_post_slab, rn_post_slab_pad values", _check_pass(own, x, al, sh, 2))
            assert r <= 1.0, (H, W, Cc, N, r)
    _note("rn_post_slab_pad + rn_zero_ring, placement", 0.0)


# ------------------------------------------------------------------------------------------------ passes with given alpha / shift
def _pass_data(N, Cc, HW, seed):
    rng = np.random.default_rng(seed)
    x = rng.normal(0.0, 1.5, (N, Cc, HW)).astype(np.float32)
    al = (rng.uniform(0.5, 2.0, (N, Cc)) * rng.choice([-1.0, 1.0], (N, Cc))).astype(np.float32)
    sh = rng.uniform(-1, 1, (N, Cc)).astype(np.float32)
    res = torch.from_numpy(rng.uniform(-2, 2, (N, Cc, HW))).half()
    return x, al, sh, res


def _unet_variants(dev, N, HW, Cc):
    """(name, [first view, second view or None], (act0, act1)): one destination; two at channel offsets (0, 40) of a wider buffer (128 channels, 160 for C = 96)"""
    wide = max(128, -(-(40 + Cc) // 32) * 32)
    yield "one view", [_View(dev, N, HW, Cc), None], (2, 0)
    for acts in ((1, 2), (2, 1)):
        yield "two views %s" % (acts,), [_View(dev, N, HW, Cc, 0, wide), _View(dev, N, HW, Cc, 40, wide)], acts


def _run_unet_pass(dev, form, Cc, HW, N, nstride, null_alpha=False, ones=False):
    """One (C, HW, N, nstride) of unet_post (form 0: fp32 rows of cpad columns, NaN beyond C) or unet_post_slab (form 1); yields (what, got, x, alpha, shift, act)"""
    x, al, sh, _ = _pass_data(N, Cc, HW, 11 + Cc + HW + N)
    if nstride == 0:
        al, sh = al[:1], sh[:1]
    if ones:
        al = np.ones_like(al)
    cpad = {32: 64, 96: 128}[Cc]
    if form == 0:
        src = _input(R.to_rows(x, cpad), dev)
        x64 = x.astype(np.float64)
    else:
        xh = torch.from_numpy(x).half()
        src = _input(R.to_slab(xh.view(N, Cc, HW, 1)), dev)
        x64 = xh.double().numpy()
    ad, sd = (None, None) if null_alpha else (_dev(al, dev), _dev(sh, dev))
    a64, s64 = (None, None) if null_alpha else (al.astype(np.float64)[..., None], sh.astype(np.float64)[..., None])
    for name, views, acts in _unet_variants(dev, N, HW, Cc):
        d1 = views[1].args(acts[1]) if views[1] else NO
        if form == 0:
            L.check(L.lib.innfer_unet_post(src.data_ptr(), cpad, Cc, HW, N, _f(ad), _f(sd), nstride, *views[0].args(acts[0]), *d1, None))
        else:
            L.check(L.lib.innfer_unet_post_slab(src.data_ptr(), N * HW * 32, Cc, HW, N, _f(ad), _f(sd), nstride, *views[0].args(acts[0]), *d1, None))
        torch.cuda.synchronize()
        for v, a in zip(views, acts):
            if v:
                yield "%s act %d" % (name, a), v.read(), x64, a64, s64, a


@pytest.mark.parametrize("Cc,HW", ((32, 257), (32, 1000), (96, 257), (96, 1000)))
@pytest.mark.parametrize("form", (0, 1), ids=("unet_post", "unet_post_slab"))
def test_unet_post_vs_float64(dev, form, Cc, HW):
    """act(x alpha + shift) into one view and into two views with acts (1, 2) / (2, 1) at channel offsets (0, 40): each view carries ITS activation, the
    neighbouring channels keep their sentinel; per-image vectors (nstride = C) and shared ones (nstride = 0); the bias-only form (alpha = 1); unet_post without
    alpha / shift."""
    for N in (1, 3):
        for nstride in (Cc, 0):
            modes = [dict(), dict(ones=True)] + ([dict(null_alpha=True)] if form == 0 and nstride == 0 else [])
            for kw in modes:
                for what, got, x64, a64, s64, a in _run_unet_pass(dev, form, Cc, HW, N, nstride, **kw):
                    r = _note("unet_post, unet_post_slab", _check_pass(got, x64, a64, s64, a))
                    assert r <= 1.0, (N, nstride, kw, what, r)


@pytest.mark.parametrize("Cc,HW", ((32, 257), (32, 1000), (96, 257), (96, 1000)))
@pytest.mark.parametrize("form", (0, 1), ids=("rn_post", "rn_post_slab"))
def test_resnet_post_vs_float64(dev, form, Cc, HW):
    """[relu](x alpha + shift) [+ res], relu x residual; the slab form also in place (dst == src)"""
    cpad = {32: 64, 96: 128}[Cc]
    for N in (1, 3):
        x, al, sh, res = _pass_data(N, Cc, HW, 23 + Cc + HW + N)
        ad, sd = _dev(al, dev), _dev(sh, dev)
        a64, s64 = al.astype(np.float64)[..., None], sh.astype(np.float64)[..., None]
        resd = _input(R.to_slab(res.view(N, Cc, HW, 1)), dev)
        xh = torch.from_numpy(x).half()
        x64 = x.astype(np.float64) if form == 0 else xh.double().numpy()
        for relu in (0, 1):
            for with_res in (False, True):
                for inplace in ((False,) if form == 0 else (False, True)):
                    v = _View(dev, N, HW, Cc)
                    rp = resd.data_ptr() if with_res else None
                    if form == 0:
                        src = _input(R.to_rows(x, cpad), dev)
                        L.check(L.lib.innfer_resnet_post(src.data_ptr(), cpad, Cc, HW, N, ad.data_ptr(), sd.data_ptr(), relu, rp, v.v.data_ptr(), v.gs, None))
                    else:
                        if inplace:
                            v.v.copy_(R.to_slab(xh.view(N, Cc, HW, 1)).reshape(-1))
                            src = v.v
                        else:
                            src = _input(R.to_slab(xh.view(N, Cc, HW, 1)), dev)
                        L.check(L.lib.innfer_resnet_post_slab(src.data_ptr(), Cc, HW, N, ad.data_ptr(), sd.data_ptr(), relu, rp, v.v.data_ptr(), v.gs, None))
                    torch.cuda.synchronize()
                    r = _note("rn_post, rn_post_slab, rn_post_slab_pad values",
                              _check_pass(v.read(), x64, a64, s64, 2 if relu else 0, res.double().numpy() if with_res else None))
                    assert r <= 1.0, (N, relu, with_res, inplace, r)


# ------------------------------------------------------------------------------------------------ unet_deep_post
def _deep_launch(dev, part, ks, Cc, HW, N, params, views, acts, image=None):
    """part: device float32 [ks, Nall, HW, cpad]; image = n: that image alone (N = 1) out of the batch's buffer"""
    g, b, ea, es = params
    Nall = part.shape[1]
    ptr = part.data_ptr() + (0 if image is None else image * HW * R.DEEP_CPAD * 4)
    d1 = views[1].args(acts[1]) if views[1] else NO
    L.check(L.lib.innfer_unet_deep_post(ptr, Nall * HW * R.DEEP_CPAD, ks, R.DEEP_CPAD, Cc, HW, N, _f(g), _f(b), _f(ea), _f(es), *views[0].args(acts[0]), *d1, None))
    torch.cuda.synchronize()


def _deep_case(dev, HW, mode, Cc, ks, N, kind, two):
    """-> worst figure of the case: train mode the y excess (held to deep_bound), the other modes err / derived bound"""
    p, x64 = R.deep_data(N, Cc, HW, ks, kind)
    rows = torch.full((ks, N, HW, R.DEEP_CPAD), float("nan"), dtype=torch.float32)
    rows[..., :Cc] = torch.from_numpy(p)
    part = _input(rows, dev).view(ks, N, HW, R.DEEP_CPAD)
    hp = R.deep_params(Cc, mode)
    params = [_dev(v, dev) for v in hp]
    acts = (1, 2) if two else (2, 0)

    def views(n):
        return [_View(dev, n, HW, 64, 0), _View(dev, n, HW, 64, 40, 128) if two else None]
    vs = views(N)
    _deep_launch(dev, part, ks, Cc, HW, N, params, vs, acts)
    gots = [v.read(written=Cc) for v in vs if v]                  # C = 40: channels 40 .. 63 of the destination keep their sentinel
    if N > 1:                                                     # a batch is its batch-1 launches, bit for bit
        for n in range(N):
            v1 = views(1)
            _deep_launch(dev, part, ks, Cc, HW, 1, params, v1, acts, image=n)
            for gb, v in zip(gots, [v for v in v1 if v]):
                assert torch.equal(R.bits16(v.read(written=Cc)), R.bits16(gb[n:n + 1])), "image %d of the batch differs from its batch-1 launch" % n
    worst = 0.0
    for got, a in zip(gots, acts):
        if mode == "train":
            a64, s64 = R.bn_alpha_shift(x64, hp[0], hp[1])
            worst = max(worst, R.y_excess(got.double().numpy(), x64, a64, s64, a))
        else:
            ea = None if hp[2] is None else hp[2].astype(np.float64)[None, :, None]
            es = None if hp[3] is None else hp[3].astype(np.float64)[None, :, None]
            extra = (ks - 1) * 2.0 ** -24 * (1.0 if ea is None else np.abs(ea)) * np.abs(p.astype(np.float64)).sum(0).transpose(0, 2, 1)
            worst = max(worst, _check_pass(got, x64, ea, es, a, extra=extra))
    return worst


@pytest.mark.parametrize("mode", R.DEEP_MODES)
@pytest.mark.parametrize("HW", R.DEEP_HW)
def test_unet_deep_post_vs_float64(dev, HW, mode):
    """Split-K reduction + BatchNorm + views in one launch, every instantiation at both ends of its range: C = 32, 64 and 40 (the c < C guards) in rows of 64 with
    NaN beyond C, ks = 1 .. 17 (the 8-deep loop and its tail), batches equal to their batch-1 launches, one and two destinations."""
    inst = R.deep_inst(HW)
    bad = []
    for kind in "ac":
        bound = R.deep_bound(inst, kind) if mode == "train" else 1.0
        worst = 0.0
        for Cc in R.DEEP_C:
            for ks in R.DEEP_KS:
                for N in R.DEEP_N:
                    for two in (False, True):
                        w = _deep_case(dev, HW, mode, Cc, ks, N, kind, two)
                        fam = "unet_deep_post, train mode (y metric, 8 x e_emul)" if mode == "train" else "unet_deep_post, eval / bias / none"
                        _note(fam, w / bound, R.deep_e_emul(inst, kind) if mode == "train" else None)
                        worst = max(worst, w / bound)
                        if not w <= bound:
                            bad.append("kind %s C %d ks %d N %d two %s: %.3e > %.3e" % (kind, Cc, ks, N, two, w, bound))
        print("MEASURED unet_deep_post<%d, %d> HW %d %s kind %s: worst / bound %.3f" % (inst + (HW, mode, kind, worst)))
    assert not bad, "; ".join(bad[:8])


# ------------------------------------------------------------------------------------------------ unet_first_mfma
def _first_launch(dev, xin, dt, Cc, H, W, N, packed, bias, with_d1, image=None):
    ho, wo = H // 2, W // 2
    gs = N * ho * wo * 32
    b0, d0 = _guarded(2 * gs, torch.float16, SENT16, dev)
    b1, d1 = _guarded(2 * gs, torch.float16, SENT16, dev)
    ptr = xin.data_ptr() + (0 if image is None else image * Cc * H * W * xin.element_size())
    L.check(L.lib.innfer_unet_first_conv(ptr, dt, Cc, H, W, N, packed.data_ptr(), _f(bias), d0.data_ptr(), d1.data_ptr() if with_d1 else None, gs, None))
    torch.cuda.synchronize()
    assert _intact(b0, 2 * gs, SENT16) and _intact(b1, 2 * gs, SENT16), "wrote outside its slabs"
    g0 = R.from_slab(d0.view(2, N, ho, wo, 32).cpu())
    g1 = R.from_slab(d1.view(2, N, ho, wo, 32).cpu())
    assert (g0 != SENT16).all(), "left part of dst0 unwritten"
    assert (g1 != SENT16).all() if with_d1 else (g1 == SENT16).all(), "dst1: unwritten, or written though NULL was passed"
    return g0, g1


@pytest.mark.parametrize("N,H,W", R.FIRST_SHAPES)
def test_unet_first_conv_vs_float64(dev, N, H, W):
    """Conv2d(C, 64, 4, 2, 1) [+ bias] from the NCHW input, LeakyReLU(0.2) view and optional ReLU view: one row with both halos outside the image; two and three
    16-pixel segments (the prefetch hand-over on either register set); more output rows than the grid has waves (the grid-stride loop wraps); a batch equals its
    batch-1 launches.  The fp32 input holds values fp16 does not: its result must be, bit for bit, that of the fp16 input holding their roundings; and dst0 must
    not depend on whether dst1 is asked for."""
    for Cc in R.FIRST_C:
        for with_bias in (False, True):
            x32, x, w, b, ref, e32 = R.first_data(N, H, W, Cc, with_bias)
            packed = np.zeros(L.lib.innfer_unet_first_packed_bytes(), np.uint8)
            L.check(L.lib.innfer_pack_unet_first(np.ascontiguousarray(w.numpy()).ctypes.data, Cc, packed.ctypes.data))
            packed, bias = _dev(packed, dev), _dev(b, dev)
            want = R.act(ref.numpy(), 1)
            first = None
            for dt in (F16, F32):
                xin = _input(x.half() if dt == F16 else x32, dev)
                for with_d1 in (False, True):
                    g0, g1 = _first_launch(dev, xin, dt, Cc, H, W, N, packed, bias, with_d1)
                    if first is None:
                        first = g0
                        got = g0.double().numpy()
                        r = _note("unet_first_mfma", R.worst_ratio(got, want, R.ulp16(np.maximum(np.abs(want), np.abs(got))) / 2 + 8 * e32), e32)
                        assert r <= 1.0, (Cc, with_bias, dt, with_d1, r, e32)
                    else:
                        assert torch.equal(R.bits16(g0), R.bits16(first)), (Cc, with_bias, dt, with_d1)
                    if with_d1:
                        pos = g0 >= 0
                        assert torch.equal(g1[pos], g0[pos]) and (g1[~pos] == 0).all(), "dst1 is not relu(dst0)"
                        assert (R.bits16(g1)[pos & (g0 != 0)] == R.bits16(g0)[pos & (g0 != 0)]).all()
                    if N > 1 and with_d1:
                        for n in range(N):
                            h0, h1 = _first_launch(dev, xin, dt, Cc, H, W, 1, packed, bias, True, image=n)
                            assert torch.equal(R.bits16(h0), R.bits16(g0[n:n + 1])) and torch.equal(R.bits16(h1), R.bits16(g1[n:n + 1])), "image %d differs from its batch-1 launch" % n


# ------------------------------------------------------------------------------------------------ tanh tails
def _tanh_check(family, got, pre64, pre32, out_dt):
    ref = np.tanh(pre64)
    e32 = float(np.abs(np.tanh(pre32).astype(np.float64) - ref).max())
    g = got.double().numpy()
    bound = 8 * e32 + R.TANH_HW + (R.ulp16(np.maximum(np.abs(ref), np.abs(g))) / 2 if out_dt == F16 else 0.0)
    return _note(family, R.worst_ratio(g, ref, bound), e32)


@pytest.mark.parametrize("K", (1, 3))
def test_resnet_sum9_tanh_vs_float64(dev, K):
    for H, W in ((4, 4), (5, 9), (16, 21)):
        for N in (1, 2):
            rng = np.random.default_rng(40 + H + W + N + K)
            Q = rng.normal(0, 0.3, (N, 9 * K, H + 8, W + 8)).astype(np.float32)
            bias = rng.normal(0, 0.3, K).astype(np.float32)
            pre64 = R.sum9_ref(Q.astype(np.float64), bias, K, H, W)
            pre32 = np.broadcast_to(bias[None, :, None, None], pre64.shape).astype(np.float32).copy()
            for j in range(9):
                pre32 = pre32 + Q[:, j::9][:, :K, 3 * (j // 3) + 1:3 * (j // 3) + 1 + H, 3 * (j % 3) + 1:3 * (j % 3) + 1 + W]
            qd, bd = _input(torch.from_numpy(Q), dev), _dev(bias, dev)
            for out_dt, tdt, sent in ((F16, torch.float16, SENT16), (F32, torch.float32, SENTF)):
                n = N * K * H * W
                obuf, out = _guarded(n, tdt, sent, dev)
                L.check(L.lib.innfer_resnet_sum9_tanh(qd.data_ptr(), bd.data_ptr(), out.data_ptr(), out_dt, K, H, W, N, None))
                torch.cuda.synchronize()
                assert _intact(obuf, n, sent) and (out != sent).all()
                r = _tanh_check("rn_sum9_tanh", out.view(N, K, H, W).cpu(), pre64, pre32, out_dt)
                assert r <= 1.0, (H, W, N, out_dt, r)


@pytest.mark.parametrize("Cc", (1, 3))
@pytest.mark.parametrize("net", ("unet", "resnet"))
def test_final_vs_float64(dev, net, Cc):
    """tanh(raw + bias) -> NCHW fp16 / fp32 from rows of 4 and of 64 floats whose padding columns hold NaN"""
    fn = L.lib.innfer_unet_final if net == "unet" else L.lib.innfer_resnet_final
    for H, W in ((4, 4), (5, 9), (16, 21)):
        for N in (1, 2):
            for rs in (4, 64):
                HW = H * W
                rng = np.random.default_rng(60 + HW + N + Cc + rs)
                x = rng.normal(0, 1.0, (N, Cc, HW)).astype(np.float32)
                bias = rng.normal(0, 0.3, Cc).astype(np.float32)
                pre64 = x.astype(np.float64) + bias.astype(np.float64)[None, :, None]
                pre32 = x + bias[None, :, None]
                rd, bd = _input(R.to_rows(x, rs), dev), _dev(bias, dev)
                for out_dt, tdt, sent in ((F16, torch.float16, SENT16), (F32, torch.float32, SENTF)):
                    n = N * Cc * HW
                    obuf, out = _guarded(n, tdt, sent, dev)
                    L.check(fn(rd.data_ptr(), rs, Cc, HW, N, bd.data_ptr(), out.data_ptr(), out_dt, None))
                    torch.cuda.synchronize()
                    assert _intact(obuf, n, sent) and (out != sent).all()
                    r = _tanh_check("unet_final, rn_final", out.view(N, Cc, HW).cpu(), pre64, pre32, out_dt)
                    assert r <= 1.0, (net, H, W, N, rs, out_dt, r)


# ------------------------------------------------------------------------------------------------ the figures of the table
def test_report(dev):
    """One case per family, not bounded: prints the worst err / bound per kernel family (after the tests above in one session: over every case they ran) -- the
    figures of the module docstring and of docs/KERNELS.md."""
    got, x, al, sh = _run_pad(dev, 5, 5, 32, 2)
    _note("rn_post, rn_post_slab, rn_post_slab_pad values", _check_pass(got[:, :, 4:9, 4:9], x, al, sh, 2))
    for what, g, x64, a64, s64, a in _run_unet_pass(dev, 1, 32, 257, 3, 32):
        _note("unet_post, unet_post_slab", _check_pass(g, x64, a64, s64, a))
    for mode, fam in (("train", "unet_deep_post, train mode (y metric, 8 x e_emul)"), ("eval", "unet_deep_post, eval / bias / none")):
        w = _deep_case(dev, 65, mode, 40, 17, 3, "c", True)
        _note(fam, w / (R.deep_bound((8, 32), "c") if mode == "train" else 1.0), R.deep_e_emul((8, 32), "c") if mode == "train" else None)
    _, x, w, b, ref, e32 = R.first_data(2, 6, 64, 3, True)
    packed = np.zeros(L.lib.innfer_unet_first_packed_bytes(), np.uint8)
    L.check(L.lib.innfer_pack_unet_first(np.ascontiguousarray(w.numpy()).ctypes.data, 3, packed.ctypes.data))
    g0, _ = _first_launch(dev, _input(x.half(), dev), F16, 3, 6, 64, 2, _dev(packed, dev), _dev(b, dev), True)
    want = R.act(ref.numpy(), 1)
    _note("unet_first_mfma", R.worst_ratio(g0.double().numpy(), want, R.ulp16(np.maximum(np.abs(want), np.abs(g0.double().numpy()))) / 2 + 8 * e32), e32)
    for fam, (ratio, e) in sorted(_REPORT.items()):
        print("REPORT %-58s largest e32 / e_emul %.2e   worst err / bound %.3f" % (fam, e, ratio))
