"""The fp32 mode's generic convolution and normalisation (csrc/f32ops.hip: f32conv_launch, f32_norm_launch) held to float64, launch by launch.

The networks reach these kernels through whatever plan the shape gets (tiled kernel with its (NKT, NPT) instantiation, images per tile, channel
chunk and epilogue, or the direct large-view kernel); the network tests only meet the plans their goldens happen to take.  Here every case of
oracle/f32conv.sweep() runs through innfer_f32conv in both forms (0: the planner's kernel, 1: the direct kernel) and is compared with the layer
computed by torch.nn.functional in float64, and the sweep asserts which plans it reached.

Bound: max|got - ref| <= 1e-5 * max(1, max|ref|) (SURVEY 8c asks 1e-4 of the network output).  Bits: every element outside a launch's view keeps
the sentinel it was filled with; image i of a batch equals the N = 1 launch on that image; the register forms of the norm equal the three-pass
kernel.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import innfer_amd.lib as L
from oracle import f32conv as O

pytestmark = pytest.mark.gpu

SENT = 0x7FC0DEAD                  # a NaN no kernel computes: what the output buffers are filled with
TOL = 1e-5


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _uniform(shape, seed, lo=-1.0, hi=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(shape, generator=g, dtype=torch.float32) * (hi - lo) + lo


def _bits(t):
    return t.contiguous().view(torch.int32)


def _packed(dev, w):
    """[K][C][ntap] fp32 (numpy) -> innfer_pack_f32conv panels on the device."""
    K, Cc, nt = w.shape
    w = np.ascontiguousarray(w, dtype=np.float32)
    n = L.lib.innfer_f32conv_packed_floats(K, Cc, nt)
    out = np.empty(n, np.float32)
    L.check(L.lib.innfer_pack_f32conv(w.ctypes.data, K, Cc, nt, out.ctypes.data))
    return torch.from_numpy(out).to(dev)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


class _Run:
    """The device tensors of one case: input view inside a wider tensor, gate / residual, output tensor (or 64-float rows), panels."""

    def __init__(self, dev, case):
        self.case = c = case
        Ho, Wo = c.out_hw
        self.Ho, self.Wo = Ho, Wo
        self.x_full = _uniform((c.N, c.ctot, c.H, c.W), 10 * c.seed + 1).to(dev)
        self.mul = _uniform((c.N, c.K, Ho, Wo), 10 * c.seed + 2, -2, 2).to(dev) if c.mul else None
        self.res = _uniform((c.N, c.K, Ho, Wo), 10 * c.seed + 3).to(dev) if c.res else None
        self.bias = O.weights(c)[1].to(dev)
        self.launches = [(d, _packed(dev, w), m) for (d, w, m) in O.launches(c)]
        if c.kind == "rows":
            self.out = torch.empty((c.N, Ho * Wo, 64), device=dev)
            ns, cs, ps, base = Ho * Wo * 64, 1, 64, 0
        else:
            self.out = torch.empty((c.N, c.ktot, Ho, Wo), device=dev)
            ns, cs, ps, base = c.ktot * Ho * Wo, Ho * Wo, 1, c.koff * Ho * Wo
        self.view = (ns, cs, ps)
        n = torch.arange(c.N).view(-1, 1, 1, 1)
        k = torch.arange(c.K).view(1, -1, 1, 1)
        y = torch.arange(Ho).view(1, 1, -1, 1)
        x = torch.arange(Wo).view(1, 1, 1, -1)
        self.idx = base + n * ns + k * cs + (y * Wo + x) * ps          # [N][K][Ho][Wo] -> element of self.out

    def args(self, d, wp, form, N=None, img=0, out=None):
        """F32ConvArgs of launch d from image `img` on; `out`: a one-image output tensor of the same layout instead of self.out."""
        c, (ns, cs, ps) = self.case, self.view
        hw = c.H * c.W
        Ho, Wo = self.Ho, self.Wo
        kw = dict(d)
        taps = kw.pop("taps")
        if N is not None:
            kw["N"] = N
        o = self.out if out is None else out
        base = c.koff * Ho * Wo if c.kind != "rows" else 0
        return L.f32conv_args(
            taps, d_in=self.x_full.data_ptr() + 4 * (img * c.ctot * hw + c.coff * hw), in_nstride=c.ctot * hw, in_cstride=hw,
            d_packed=wp.data_ptr(), d_bias=self.bias.data_ptr(),
            d_out=o.data_ptr() + 4 * ((img if out is None else 0) * ns + base), out_nstride=ns, out_cstride=cs, out_pstride=ps,
            d_res=self.res.data_ptr() + 4 * img * c.K * Ho * Wo if c.res else None, res_nstride=c.K * Ho * Wo, res_cstride=Ho * Wo,
            d_mul=self.mul.data_ptr() + 4 * img * c.K * Ho * Wo if c.mul else None, mul_nstride=c.K * Ho * Wo, mul_cstride=Ho * Wo,
            form=form, **kw)

    def run(self, form):
        """All launches of the case in `form`; after each one, every element outside the views written so far still holds the sentinel."""
        c = self.case
        _bits(self.out).fill_(SENT)
        written = torch.zeros((self.Ho, self.Wo), dtype=torch.bool)
        plans = []
        for (d, wp, m) in self.launches:
            a = self.args(d, wp, form)
            plans.append(L.f32conv_plan(a))
            L.check(L.lib.innfer_f32conv(C.byref(a), _stream()))
            torch.cuda.synchronize()
            written |= torch.from_numpy(m)
            got = _bits(self.out).cpu().view(-1)
            keep = torch.ones(got.numel(), dtype=torch.bool)
            keep[self.idx[:, :, written].reshape(-1)] = False
            bad = (got[keep] != SENT).sum().item()
            assert bad == 0, f"{c.name} form {form}: {bad} elements outside the launch views were written (launch {d['ooy'], d['oox']})"
        return self.out.cpu().view(-1)[self.idx], plans


def _ref(run):
    c = run.case
    x = run.x_full[:, c.coff:c.coff + c.C].cpu()
    return O.reference(c, x, run.mul.cpu() if c.mul else None, run.res.cpu() if c.res else None)


def test_f32conv_sweep_vs_float64(dev):
    """Every case of oracle/f32conv.sweep() in both forms against float64, the sentinel outside the views, batch == its images' N = 1 launches,
    and the plans the sweep must reach: all 8 (NKT, NPT) instantiations, IMG > 1, both epilogues, a partial last chunk, the direct kernel."""
    worst = (0.0, None)
    seen, imgs, vec4, partial, direct = set(), set(), set(), 0, 0
    batch_nkt = set()
    for case in O.sweep():
        run = _Run(dev, case)
        ref = _ref(run)
        scale = max(1.0, ref.abs().max().item())
        outs = {}
        for form in (0, 1):
            got, plans = run.run(form)
            outs[form] = got.clone()
            assert torch.isfinite(got).all(), (case.name, form)
            err = (got.double() - ref).abs().max().item() / scale
            if err > worst[0]:
                worst = (err, f"{case.name} form {form} plan {plans[0]}")
            assert err <= TOL, (case.name, form, plans, err)
            for p in plans:
                if form == 0:
                    seen.add((p["NKT"], p["NPT"]))
                    imgs.add(p["IMG"])
                    vec4.add(p["vec4"])
                    partial += bool(p["CC"]) and case.C % p["CC"] != 0
                direct += p["direct"]
        if case.N > 1:                                         # image i of the batch == the N = 1 launch on image i (form 0: the planner's kernel)
            p_batch = L.f32conv_plan(run.args(*run.launches[0][:2], 0))
            for i in sorted({0, case.N - 1}):
                one = torch.empty((1,) + tuple(run.out.shape[1:]), device=dev)
                _bits(one).fill_(SENT)
                for (d, wp, _m) in run.launches:
                    a = run.args(d, wp, 0, N=1, img=i, out=one)
                    L.check(L.lib.innfer_f32conv(C.byref(a), _stream()))
                torch.cuda.synchronize()
                got1 = one.cpu().view(-1)[run.idx[:1]]
                assert torch.equal(_bits(got1), _bits(outs[0][i:i + 1])), f"{case.name}: image {i} of the batch differs from its N = 1 launch"
            batch_nkt.add(p_batch["NKT"])
    print(f"f32conv sweep: worst max|err| / max(1, max|ref|) = {worst[0]:.2e} ({worst[1]})")
    assert seen == {(nkt, npt) for nkt in (1, 2, 3, 4) for npt in (1, 4)}, sorted(seen)
    assert max(imgs) > 1 and vec4 == {0, 1} and partial > 0 and direct > 0, (imgs, vec4, partial, direct)
    assert batch_nkt == {1, 2, 3, 4}, batch_nkt


def _strided_case(dev, name, C_, H, W, K, N, ns, cs, seed, pad_mode=1):
    """A 3 x 3 conv of K outputs over the view [N][C][H][W] with strides (ns, cs, W, 1) into one flat buffer: (case, run, buffer)."""
    case = O.Case(name, N, C_, H, W, K, pad_mode=pad_mode, act=1, seed=seed)
    extent = (N - 1) * ns + (C_ - 1) * cs + H * W
    buf = torch.empty(extent, device=dev)
    view = buf.as_strided((N, C_, H, W), (ns, cs, W, 1))
    view.copy_(_uniform((N, C_, H, W), seed))
    run = _Run.__new__(_Run)
    run.case, (run.Ho, run.Wo) = case, case.out_hw
    run.mul = run.res = None
    run.bias = O.weights(case)[1].to(dev)
    run.launches = [(d, _packed(dev, w), m) for (d, w, m) in O.launches(case)]
    run.out = torch.empty((N, K, H, W), device=dev)
    run.view = (K * H * W, H * W, 1)
    run.idx = torch.arange(N * K * H * W).view(N, K, H, W)
    run.x_full = buf                                          # (args() adds the view's strides below)
    return case, run, view


def _strided_args(run, d, wp, form, ns, cs):
    a = run.args(d, wp, form)
    a.d_in, a.in_nstride, a.in_cstride = run.x_full.data_ptr(), ns, cs
    return a


def _run_strided(run, form, ns, cs):
    d, wp, _ = run.launches[0]
    a = _strided_args(run, d, wp, form, ns, cs)
    plan = L.f32conv_plan(a)
    _bits(run.out).fill_(SENT)
    L.check(L.lib.innfer_f32conv(C.byref(a), _stream()))
    torch.cuda.synchronize()
    return run.out.cpu(), plan


def test_f32conv_views_beyond_2gib(dev):
    """(a) A small image read through a channel stride that puts the view beyond 2 GiB takes the direct kernel; (b) the same shape with the tiled
    kernel's gate extent (CC in_cstride + IMG in_nstride + H W) * 4 at its last admitted value below 2^31 takes the tiled kernel, its last channel
    ~1.5 GiB into the buffer.  Whole outputs against float64."""
    T = (1 << 29) - 1                                         # the gate: extent * 4 < 0x7fffffff
    H, W, K, N = 9, 11, 16, 2
    # (a) C = 3, channel stride 2^28 + 65 floats: channel 2 starts 2 GiB + 520 B into the buffer; image 1 overlaps image 0 (read-only views may)
    cs, ns = (1 << 28) + 65, 41
    case, run, view = _strided_case(dev, "view_beyond_2gib", 3, H, W, K, N, ns, cs, 901)
    assert (2 * cs) * 4 >= 1 << 31
    ref = O.reference(case, view.cpu())
    for form in (0, 1):
        got, plan = _run_strided(run, form, ns, cs)
        assert plan["direct"] == 1, plan
        err = (got.double() - ref).abs().max().item()
        print(f"view beyond 2 GiB, form {form}: plan {plan}, max|err| {err:.2e}")
        assert err <= TOL * max(1.0, ref.abs().max().item()), err
    del run, view
    torch.cuda.empty_cache()
    # (b) C = 4 (CC 4, IMG 1 for this grid): in_cstride chosen so that the gate extent is exactly T -- the last value the tiled kernel admits
    C_ = 4
    probe = O.Case("p", N, C_, H, W, K)
    d0 = O.launches(probe)[0][0]
    kw = dict(d0)
    taps = kw.pop("taps")
    p0 = L.f32conv_plan(L.f32conv_args(taps, d_in=1 << 20, in_nstride=C_ * H * W, in_cstride=H * W, d_packed=1 << 20, d_out=1 << 20,
                                       out_nstride=K * H * W, out_cstride=H * W, out_pstride=1, **kw))
    CC, IMG = p0["CC"], p0["IMG"]
    ns = 97
    cs = (T - H * W - IMG * ns) // CC
    ns = T - H * W - CC * cs                                  # exact: CC cs + IMG ns + H W == T (IMG == 1)
    assert IMG == 1 and CC * cs + IMG * ns + H * W == T, (CC, IMG)
    case, run, view = _strided_case(dev, "view_below_2gib", C_, H, W, K, N, ns, cs, 902)
    ref = O.reference(case, view.cpu())
    got, plan = _run_strided(run, 0, ns, cs)
    assert plan["direct"] == 0, plan
    err = (got.double() - ref).abs().max().item()
    print(f"view at the gate (last channel at byte {4 * (ns + 3 * cs)}): plan {plan}, max|err| {err:.2e}")
    assert err <= TOL * max(1.0, ref.abs().max().item()), err
    del run, view
    torch.cuda.empty_cache()


def test_f32conv_4k_reflect_64ch_windows(dev):
    """A 64 -> 64 3 x 3 reflect-padded layer (CycleGAN ResnetBlock) on a 2160 x 3840 frame: its 64-channel input spans 2.1 GB, beyond the tiled
    kernel's 32-bit gate.  Corner, last-row and last-channel windows against float64 on crops plus halo."""
    H, W, Cc, K = 2160, 3840, 64, 64
    case = O.Case("resnet_block_4k", 1, Cc, H, W, K, pad_mode=1, act=2, seed=903)
    g = torch.Generator(device=dev).manual_seed(903)
    x = torch.rand((1, Cc, H, W), generator=g, device=dev) * 2 - 1
    w, b = O.weights(case)
    (d, wp, _), = O.launches(case)
    wp = _packed(dev, wp)
    out = torch.empty((1, K, H, W), device=dev)
    kw = dict(d)
    taps = kw.pop("taps")
    a = L.f32conv_args(taps, d_in=x.data_ptr(), in_nstride=Cc * H * W, in_cstride=H * W, d_packed=wp.data_ptr(), d_bias=b.to(dev).data_ptr(),
                       d_out=out.data_ptr(), out_nstride=K * H * W, out_cstride=H * W, out_pstride=1, form=0, **kw)
    plan = L.f32conv_plan(a)
    L.check(L.lib.innfer_f32conv(C.byref(a), _stream()))
    torch.cuda.synchronize()
    worst = 0.0
    for (y0, y1, x0, x1, k0, k1) in [(0, 16, 0, 16, 0, 64), (H - 16, H, W - 16, W, 0, 64), (H - 2, H, 1900, 1964, 0, 64), (1000, 1040, 0, W, 63, 64),
                                     (0, 8, W - 24, W, 60, 64), (H - 8, H, 0, 24, 0, 8)]:
        ya, yb, xa, xb = max(y0 - 1, 0), min(y1 + 1, H), max(x0 - 1, 0), min(x1 + 1, W)
        crop = x[:, :, ya:yb, xa:xb].cpu()
        pads = (int(y0 == 0), int(y1 == H), int(x0 == 0), int(x1 == W))
        ref = O.epilogue(case, O.conv_only(case, crop, w[k0:k1], pads=pads), b[k0:k1])
        got = out[:, k0:k1, y0:y1, x0:x1].cpu()
        err = (got.double() - ref).abs().max().item()
        worst = max(worst, err)
        assert err <= TOL * max(1.0, ref.abs().max().item()), ((y0, x0, k0), err)
    print(f"4K reflect 64 -> 64: plan {plan}, worst window max|err| {worst:.2e}")
    del x, out
    torch.cuda.empty_cache()


def _norm_ref(x, mode, w, b, rm, rv, act, res, eps=1e-5):
    """(float64 output, max |x alpha|): alpha = weight / sqrt(var + eps), the factor the kernels (and ATen's fp32 batch_norm_cpu_transform_input)
    apply as y = x alpha + (bias - mean alpha)."""
    x = x.double()
    if mode == 3:
        alpha = w.double().view(1, -1, 1)
        y = x * alpha + b.double().view(1, -1, 1)
    else:
        if mode == 1:
            mean, var = rm.double().view(1, -1, 1), rv.double().view(1, -1, 1)
        else:
            mean = x.mean(dim=2, keepdim=True)
            var = ((x - mean) ** 2).mean(dim=2, keepdim=True)           # biased
        alpha = 1.0 / torch.sqrt(var + eps)
        y = (x - mean) * alpha
        if mode != 2:
            alpha = alpha * w.double().view(1, -1, 1)
            y = y * w.double().view(1, -1, 1) + b.double().view(1, -1, 1)
    y = O._act(y, act)
    return (y + res.double() if res is not None else y), (x * alpha).abs().max().item()


@pytest.mark.parametrize("HW", [1, 2, 63, 64, 65, 4095, 4096, 4097, 16384, 16385])
def test_f32_norm_vs_float64(dev, HW):
    """innfer_f32_norm modes 0 .. 3 (BatchNorm2d on the image's statistics / on running statistics, InstanceNorm2d, a per-channel transform) with
    affine, activation, residual and an output channel offset, against float64; the plane-in-registers forms (65 <= HW <= 16384, modes 0 / 2) equal
    the three-pass kernel bit for bit; elements outside the output view keep the sentinel.  (HW <= 64 runs a wave per plane whose sums run in
    another order: held to float64 only.)
    Bound: 1e-5 of max(1, |y|, |x alpha|).  The kernels compute y = x alpha + (bias - mean alpha) in fp32 -- ATen's own fp32 form -- so a plane whose
    variance is ~0 (HW = 1: var = 0, alpha = weight / sqrt(eps) ~ 316 weight) cancels two terms of magnitude |x alpha| ~ 1e3 into y = bias; relative
    to |y| alone the fp32 round-off of that cancellation (3e-5 measured at HW = 1) exceeds 1e-5 though the arithmetic is the reference's."""
    N, Cc, ctot, coff = 2, 3, 5, 1
    for mode in range(4):
        for act in ((0, 1, 2, 3, 4) if HW in (64, 4097) else sorted({mode + 1, 1})):
            seed = 5000 + 37 * HW + 7 * mode + act
            xin = _uniform((N, Cc + 1, HW), seed).to(dev) * 3 + 0.5
            w = _uniform((Cc,), seed + 1, 0.5, 1.5).to(dev)
            b = _uniform((Cc,), seed + 2).to(dev)
            rm = _uniform((Cc,), seed + 3).to(dev)
            rv = _uniform((Cc,), seed + 4, 0.5, 2.0).to(dev)
            res = _uniform((N, Cc, HW), seed + 5).to(dev) if act % 2 == 0 else None
            outs = {}
            for form in (0, 1):
                out = torch.empty((N, ctot, HW), device=dev)
                _bits(out).fill_(SENT)
                L.check(L.lib.innfer_f32_norm(xin[:, 1:].data_ptr(), (Cc + 1) * HW, HW, out[:, coff:].data_ptr(), ctot * HW, HW, N, Cc, HW, mode, 1e-5,
                                              w.data_ptr(), b.data_ptr(), rm.data_ptr(), rv.data_ptr(), act,
                                              res.data_ptr() if res is not None else None, Cc * HW, HW, form, _stream()))
                torch.cuda.synchronize()
                outs[form] = out.cpu()
                ob = _bits(outs[form])
                assert (ob[:, :coff] == SENT).all() and (ob[:, coff + Cc:] == SENT).all(), (HW, mode, form)
                ref, xa = _norm_ref(xin[:, 1:].cpu(), mode, w.cpu(), b.cpu(), rm.cpu(), rv.cpu(), act, res.cpu() if res is not None else None)
                err = (outs[form][:, coff:coff + Cc].double() - ref).abs().max().item()
                assert err <= TOL * max(1.0, ref.abs().max().item(), xa), (HW, mode, act, form, err, xa)
            if mode in (0, 2) and 64 < HW <= 16384:
                assert torch.equal(_bits(outs[0]), _bits(outs[1])), f"register form != three-pass kernel (HW {HW}, mode {mode}, act {act})"
