"""CPU side of tests/test_gpu_glue_kernels.py (the pointwise / gather kernels around PAN, PPON, the WBC UNet and the image filters): every reference and model of
tests/_glue_ref.py against the torch function it restates, in float64; the refusals of the entry points of ABI 124, called with pointers nothing may dereference;
and planted faults in the numpy stand-in of each kernel, each of which must miss its comparator by >= 10x at some case of the GPU list (the factors are printed).
"""
import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import _glue_ref as G
import innfer_amd.lib as L

FAKE = 0x1000
f32, f64 = np.float32, np.float64
T = lambda a: torch.as_tensor(np.asarray(a))


# ------------------------------------------------------------------------------------------------ the references restate torch
def test_interpolation_models_are_f_interpolate():
    for h, w in G.UPS_SIZES + G.FINAL_SIZES + ((3, 4),):
        x = G.rand((2, 3, h, w), h * 31 + w).double()
        for f in (2, 3):
            want = F.interpolate(x, scale_factor=float(f), mode="bilinear", align_corners=False)
            assert (T(G.bilinear_model(x, f * h, f * w, False, f, f64)) - want).abs().max() < 1e-12, (h, w, f)
            assert torch.equal(T(G.nearest_model(x.numpy(), f)), F.interpolate(x, scale_factor=float(f), mode="nearest"))
            assert torch.equal(G.upsample_ref(x, f, True), want)
        for s in (1, 2, 3, 4):
            raw = G.rand((2, 3, s * h, s * w), 7).double()
            want = raw + (F.interpolate(x, size=(s * h, s * w), mode="bilinear", align_corners=True) if s > 1 else x)
            assert (T(G.pan_final_model(raw, x, s, f64)) - want).abs().max() < 1e-12, (h, w, s)
            assert torch.equal(G.pan_final_ref(raw, x, s), want)
        for Ho, Wo in ((2 * h, 2 * w), (h, w), (2 * h + 1, 3 * w - 2), (1, 1)):
            if Ho > 0 and Wo > 0:
                want = F.interpolate(x, size=(Ho, Wo), mode="bilinear", align_corners=True)
                assert (T(G.bilinear_model(x, Ho, Wo, True, None, f64)) - want).abs().max() < 1e-12, (h, w, Ho, Wo)


def test_wbc_references():
    for h, w in G.UPADD_SIZES:
        x = G.rand((2, 4, h, w), h + w).double()
        assert torch.equal(T(G.tf_up_model(x, f64)), G.tf_up_ref(x)), (h, w)
    for H, W in ((1, 1), (1, 3), (5, 4), (5, 7), (1, 33)):          # the row patch turns the zero-padded 7x7 conv into seven vertical taps
        x = G.rand((2, 3, H, W), H * W).double()
        conv = nn.Conv2d(3, 8, 7, padding=3).double()
        wcol = torch.zeros(8, 32, 7, 1, dtype=torch.float64)
        with torch.no_grad():
            wcol[:, :21, :, 0] = conv.weight.permute(0, 3, 1, 2).reshape(8, 21, 7)          # [co][kx * 3 + c][ky]
            got = F.conv2d(G.wb_pre_ref(x).permute(0, 3, 1, 2), wcol, conv.bias, padding=(3, 0))
            assert (got - conv(x)).abs().max() < 1e-12, (H, W)
        assert (G.wb_pre_ref(x)[..., 21:] == 0).all()


def test_pass_references():
    x = G.slab_pair_values((2, 40, 5, 7), 3)
    hi, lo = G.slab_pair_ref(x)
    mh, ml = G.slab_pair_model(x)
    assert np.array_equal(hi.numpy().view(np.int16), mh.view(np.int16)) and np.array_equal(lo.numpy().view(np.int16), ml.view(np.int16))
    assert ((hi.double() + lo.double() / 2048 - x.double()).abs() <= x.double().abs() * 2.0 ** -21 + 2.0 ** -36).all()          # the pair carries ~22 bits
    assert (x == 0).any() and (lo[x == hi.float()] == 0).all() and ((lo != 0) & (lo.abs().double() < 2.0 ** -14)).any() and x.abs().max() > 3.5
    t = G.rand((2, 8 * 4, 5), 5)
    t[:, :, 0] = 0
    ref, extra = G.prefix_lrelu_ref(t, 8)
    d = t.double().reshape(2, 8, 4, 5)
    want = F.leaky_relu(torch.cat([d[:, :k + 1].sum(1) for k in range(8)], 1), float(np.float32(0.2)))          # PPON's cat(d1, d1 + d2, ..) -> act
    assert (ref - want).abs().max() < 1e-12 and (T(G.prefix_lrelu_model(t, 8, f64)) - ref).abs().max() < 1e-12
    assert ((T(G.prefix_lrelu_model(t, 8, f32)).double() - ref).abs() <= extra).all()
    a, b = G.rand((300,), 1), G.rand((300,), 2)
    for al in (1.0, 0.5, -0.25, 0.0):
        assert torch.equal(T(G.axpy_model(a, b, al, f64)), G.axpy_ref(a, b, al))
        assert ((T(G.axpy_model(a, b, al, f32)).double() - G.axpy_ref(a, b, al)).abs() <= G.axpy_extra(a, b, al)).all()
    v = G.rand((100,), 3, -3, 3).double()
    assert torch.equal(G.act_ref(v, 2), F.relu(v)) and (G.act_ref(v, 1) - F.leaky_relu(v, 0.2)).abs().max() < 1e-8 and torch.equal(G.act_ref(v, 4), torch.sigmoid(v))


def test_filter_references():
    for fam in G.GF_FAMILIES:
        for H, W in G.GF_SIZES:
            x, y = G.gf_operands(fam, 2, H, W, 11)
            for ks in (1, 3, 5, 7):
                if H <= ks // 2 or W <= ks // 2:
                    continue
                for eps in (1e-2, 1e-4):
                    assert (T(G.gf_model(x, y, ks, eps, f64)) - G.gf_ref(x, y, ks, eps)).abs().max() < 1e-9, (fam, H, W, ks, eps)
                    xhr, _ = G.gf_operands("noise", 2, 2 * H + 1, 3 * W - 2, 12)
                    assert (T(G.gf_model(x, y, ks, eps, f64, xhr)) - G.gf_ref(x, y, ks, eps, xhr)).abs().max() < 1e-9, (fam, H, W, ks, eps)
    for H, W in G.F2D_PLANES + ((2, 2),):
        x = G.rand((2, H, W), H * W)
        for kH, kW, pl, pt in G.F2D_KERNELS:
            k = G.f2d_kernel(kH, kW, kH * 8 + kW)
            for border in range(4):
                if G.f2d_accepts(H, W, kH, kW, pl, pt, border):
                    assert (T(G.f2d_model(x, k, pl, pt, border, f64)) - G.f2d_ref(x, k, pl, pt, border)[0]).abs().max() < 1e-12, (H, W, kH, kW, border)
    x, k = G.rand((1, 2, 2), 1), G.f2d_kernel(3, 5, 2)          # circular with pad == size
    assert G.f2d_accepts(2, 2, 3, 5, 2, 1, 3) and (T(G.f2d_model(x, k, 2, 1, 3, f64)) - G.f2d_ref(x, k, 2, 1, 3)[0]).abs().max() < 1e-12


# ------------------------------------------------------------------------------------------------ refusals: nothing may launch (the pointers are never dereferenced)
def _refused(rc, *codes):
    assert rc in (codes or (L.ERR_INVALID,)), rc
    assert L.last_error()
    return True


def test_entry_points_refuse():
    assert L.ABI_VERSION == 124 == L.lib.innfer_version()
    lib, f, big = L.lib, FAKE, 1 << 30
    # innfer_pan_pre
    assert _refused(lib.innfer_pan_pre(None, 0, 1, 3, 4, 4, f, None)) and _refused(lib.innfer_pan_pre(f, 0, 1, 3, 4, 4, None, None))
    assert _refused(lib.innfer_pan_pre(f, 2, 1, 3, 4, 4, f, None))                                                  # uint8 input
    for N, Cc, H, W in ((0, 3, 4, 4), (1, 0, 4, 4), (1, 3, 0, 4), (1, 3, 4, 0)):
        assert _refused(lib.innfer_pan_pre(f, 0, N, Cc, H, W, f, None))
    assert _refused(lib.innfer_pan_pre(f, 0, 1, 33, 4, 4, f, None), L.ERR_UNSUPPORTED)                              # more than one group
    # innfer_pan_upsample
    assert _refused(lib.innfer_pan_upsample(None, 0, 1, 32, 4, 4, 2, 1, big, f, big, None)) and _refused(lib.innfer_pan_upsample(f, 0, 1, 32, 4, 4, 2, 1, big, None, big, None))
    for fac, bil in ((1, 0), (4, 1), (2, 2), (2, -1)):
        assert _refused(lib.innfer_pan_upsample(f, 0, 1, 32, 4, 4, fac, bil, big, f, big, None))
    for N, Cc, h, w in ((0, 32, 4, 4), (1, 0, 4, 4), (1, 32, 0, 4), (1, 32, 4, 0)):
        assert _refused(lib.innfer_pan_upsample(f, 1, N, Cc, h, w, 2, 1, big, f, big, None))
    for Cc in (8, 40, 96):
        assert _refused(lib.innfer_pan_upsample(f, 0, 1, Cc, 4, 4, 2, 1, big, f, big, None))                         # whole groups, one or two
    assert _refused(lib.innfer_pan_upsample(f, 0, 2, 64, 4, 4, 2, 1, 2 * 16 * 32 - 1, f, big, None))                # group strides
    assert _refused(lib.innfer_pan_upsample(f, 0, 2, 64, 4, 4, 3, 1, big, f, 2 * 9 * 16 * 32 - 1, None))
    assert _refused(lib.innfer_pan_upsample(f, 2, 1, 32, 4, 4, 2, 1, big, f, big, None))                            # dtype
    # innfer_pan_final
    for a in ((None, 3, f), (f, 3, None)):
        assert _refused(lib.innfer_pan_final(a[0], a[1], a[2], 0, 1, 4, 4, 2, f, 0, -1, None))
    assert _refused(lib.innfer_pan_final(f, 3, f, 0, 1, 4, 4, 2, None, 0, -1, None))
    for xdt, odt in ((2, 0), (0, 2)):
        assert _refused(lib.innfer_pan_final(f, 3, f, xdt, 1, 4, 4, 2, f, odt, -1, None))
    for Cc, N, H, W, s in ((0, 1, 4, 4, 2), (3, 0, 4, 4, 2), (3, 1, 0, 4, 2), (3, 1, 4, 0, 2), (3, 1, 4, 4, 0), (3, 1, 4, 4, 5)):
        assert _refused(lib.innfer_pan_final(f, Cc, f, 0, N, H, W, s, f, 0, -1, None))
    for form in (-2, 2):
        assert _refused(lib.innfer_pan_final(f, 3, f, 0, 1, 4, 4, 2, f, 0, form, None))
    assert _refused(lib.innfer_pan_final(f, 3, f, 0, 1, 4, 5, 2, f, 0, 1, None))                                    # the strip form on a width of 10
    assert _refused(lib.innfer_pan_final(f, 3, f, 0, 1, 3, 3, 3, f, 0, 1, None))
    # innfer_pan_slab_pair
    assert _refused(lib.innfer_pan_slab_pair(None, 1, 40, 4, 4, f, big, None)) and _refused(lib.innfer_pan_slab_pair(f, 1, 40, 4, 4, None, big, None))
    for N, Cc, H, W in ((0, 40, 4, 4), (1, 0, 4, 4), (1, 40, 0, 4), (1, 40, 4, 0)):
        assert _refused(lib.innfer_pan_slab_pair(f, N, Cc, H, W, f, big, None))
    assert _refused(lib.innfer_pan_slab_pair(f, 2, 40, 4, 4, f, 2 * 2 * 16 * 32 - 8, None))                         # lo inside the hi half
    assert _refused(lib.innfer_pan_slab_pair(f, 1, 40, 4, 4, f, 2 * 16 * 32 + 4, None))                             # 16-byte stores
    # innfer_ppon_upsample3 / innfer_ppon_axpy
    assert _refused(lib.innfer_ppon_upsample3(None, big, f, big, 1, 4, 4, None)) and _refused(lib.innfer_ppon_upsample3(f, big, None, big, 1, 4, 4, None))
    for N, H, W in ((0, 4, 4), (1, 0, 4), (1, 4, 0)):
        assert _refused(lib.innfer_ppon_upsample3(f, big, f, big, N, H, W, None))
    assert _refused(lib.innfer_ppon_upsample3(f, 2 * 16 * 32 - 1, f, big, 2, 4, 4, None)) and _refused(lib.innfer_ppon_upsample3(f, big, f, 2 * 9 * 16 * 32 - 1, 2, 4, 4, None))
    for a in ((None, f, f), (f, None, f), (f, f, None)):
        assert _refused(lib.innfer_ppon_axpy(a[0], a[1], a[2], 1.0, 8, 0, 0, None))
    assert _refused(lib.innfer_ppon_axpy(f, f, f, 1.0, 0, 0, 0, None)) and _refused(lib.innfer_ppon_axpy(f, f, f, 1.0, 8, 2, 0, None))
    assert _refused(lib.innfer_ppon_axpy(f, f, f, 1.0, 8, 0, 1, None)) and _refused(lib.innfer_ppon_axpy(f, f, f, 1.0, 8, 1, 2, None)) and _refused(lib.innfer_ppon_axpy(f, f, f, 1.0, 8, 1, -1, None))
    # innfer_wbc_pre / innfer_wbc_upadd
    assert _refused(lib.innfer_wbc_pre(None, 0, 1, 3, 4, 4, f, None)) and _refused(lib.innfer_wbc_pre(f, 0, 1, 3, 4, 4, None, None)) and _refused(lib.innfer_wbc_pre(f, 2, 1, 3, 4, 4, f, None))
    for N, Cc, H, W in ((0, 3, 4, 4), (1, 0, 4, 4), (1, 3, 0, 4), (1, 3, 4, 0)):
        assert _refused(lib.innfer_wbc_pre(f, 0, N, Cc, H, W, f, None))
    assert _refused(lib.innfer_wbc_pre(f, 0, 1, 5, 4, 4, f, None), L.ERR_UNSUPPORTED)                               # 35 patch channels
    for a in ((None, f, f), (f, None, f), (f, f, None)):
        assert _refused(lib.innfer_wbc_upadd(a[0], a[1], 0, 1, 32, 4, 4, 0, a[2], None))
    for N, Cc, h, w, tf in ((0, 32, 4, 4, 0), (1, 0, 4, 4, 0), (1, 32, 0, 4, 0), (1, 32, 4, 0, 0), (1, 32, 4, 4, 2), (1, 32, 4, 4, -1)):
        assert _refused(lib.innfer_wbc_upadd(f, f, 1, N, Cc, h, w, tf, f, None))
    for Cc in (8, 16, 48, 96):
        assert _refused(lib.innfer_wbc_upadd(f, f, 0, 1, Cc, 4, 4, 0, f, None))
    assert _refused(lib.innfer_wbc_upadd(f, f, 2, 1, 32, 4, 4, 0, f, None))
    # innfer_f32_prefix_lrelu / innfer_f32_act_copy
    assert _refused(lib.innfer_f32_prefix_lrelu(None, 1, 8, 32, 4, None))
    for N, g, gc, hw in ((0, 8, 32, 4), (1, 0, 32, 4), (1, 8, 0, 4), (1, 8, 32, 0)):
        assert _refused(lib.innfer_f32_prefix_lrelu(f, N, g, gc, hw, None))
    assert _refused(lib.innfer_f32_act_copy(None, 8, f, 8, 8, 1, 0, None)) and _refused(lib.innfer_f32_act_copy(f, 8, None, 8, 8, 1, 0, None))
    for ins, ons, per, N, act in ((7, 8, 8, 2, 0), (8, 7, 8, 2, 0), (8, 8, 0, 2, 0), (8, 8, 8, 0, 0), (8, 8, 8, 2, 5), (8, 8, 8, 2, -1)):
        assert _refused(lib.innfer_f32_act_copy(f, ins, f, ons, per, N, act, None))
    # innfer_filter2d: F.pad's limits (reflect with pad >= size, circular with pad > size)
    assert _refused(lib.innfer_filter2d(f, 1, 1, 2, 3, f, 5, 1, 0, 2, 1, f, None)) and _refused(lib.innfer_filter2d(f, 1, 1, 3, 2, f, 1, 5, 2, 0, 1, f, None))
    assert _refused(lib.innfer_filter2d(f, 1, 1, 2, 2, f, 7, 1, 0, 3, 3, f, None)) and _refused(lib.innfer_filter2d(f, 1, 1, 2, 2, f, 1, 7, 3, 0, 3, f, None))


# ------------------------------------------------------------------------------------------------ planted faults
def _report(name, factors):
    worst = max(factors)
    print(f"[glue-faults] {name}: clean {factors[0]:.3f}, fault misses by {worst:.1f}x at its worst case")
    assert factors[0] <= 1.0, (name, "the unfaulted stand-in misses its own comparator", factors[0])
    assert worst >= 10.0, (name, worst)


def test_planted_interpolation_faults():
    # pan_upsample (fp16 slabs) over the GPU list: the unclamped second tap, f = 3 with inv = 0.5
    clean, noclamp, inv = [], [], []
    for h, w in G.UPS_SIZES:
        src = G.rand((2, 8, h, w), h * w).half().float()
        for f in (2, 3):
            ref, e32, _ = G.judge_upsample(src, f)
            clean.append(G.ratio(G.h16(G.bilinear_model(src, f * h, f * w, False, f), f64), ref, e32))
            noclamp.append(G.ratio(G.h16(G.bilinear_model(src, f * h, f * w, False, f, fault="noclamp"), f64), ref, e32))
            if f == 3:
                inv.append(G.ratio(G.h16(G.bilinear_model(src, f * h, f * w, False, f, inv=0.5), f64), ref, e32))
    _report("pan_upsample: second tap not clamped", [max(clean)] + noclamp)
    _report("pan_upsample: f = 3 with inv = 0.5", [max(clean)] + inv)
    # pan_final: align_corners swapped, the unclamped tap (fp32 in, fp32 out: the tightest comparator)
    clean, align, noclamp = [], [], []
    for h, w in G.FINAL_SIZES:
        for s in (2, 3, 4):
            x, raw = G.rand((2, 3, h, w), h + w), G.rand((2, 3, s * h, s * w), s)
            ref, e32, _ = G.judge_final(raw, x, s)
            for lst, fault in ((clean, None), (align, "align"), (noclamp, "noclamp")):
                lst.append(G.ratio(G.h16(G.pan_final_model(raw, x, s, fault=fault), f64), ref, e32))
    _report("pan_final: align_corners swapped", [max(clean)] + align)
    _report("pan_final: second tap not clamped", [max(clean)] + noclamp)
    # nearest 3x with y / 2 (bit for bit)
    off = []
    for h, w in ((1, 1), (2, 3), (5, 7)):
        src = G.rand((2, 8, h, w), h * w).half().float().numpy()
        off.append(G.bits_off(G.nearest_model(src, 3, div=2), G.nearest_model(src, 3)))
    _report("ppon_upsample3 / nearest 3x: y / 3 -> y / 2", [0.0] + off)


def test_planted_wbc_faults():
    for name, fault in (("odd / odd takes the right neighbour", "right"), ("the border is zero, not replicated", "zero")):
        off = []
        for h, w in G.UPADD_SIZES:
            src, skip = G.rand((2, 32, h, w), h * w).half().float(), G.rand((2, 32, 2 * h, 2 * w), 9).half().float()
            want, _ = G.upadd16_ref(src, skip, 1)
            assert G.bits_off(G.upadd16_model(src, skip, 1), want.float()) == 0.0
            off.append(G.bits_off(G.upadd16_model(src, skip, 1, fault), want.float()))
        _report("wb_upadd tf mode: " + name, [0.0] + off)
    clean, bad = [], []
    for h, w in G.UPADD_SIZES:
        src, skip = G.rand((2, 32, h, w), h * w).half().float(), G.rand((2, 32, 2 * h, 2 * w), 9).half().float()
        ref, e32, extra = G.judge_upadd_pt(src, skip, True)
        clean.append(G.ratio(G.upadd16_model(src, skip, 0), ref, e32, extra))
        bad.append(G.ratio(G.upadd16_model(src, skip, 0, "noclamp"), ref, e32, extra))
    _report("wb_upadd pt mode: second tap not clamped", [max(clean)] + bad)
    for name, kw in (("offset -2 instead of -3", dict(off=-2)), ("channel order c * 7 + kx", dict(order="c*7+kx"))):
        off = []
        for H, W in ((1, 1), (1, 3), (5, 4), (5, 7), (1, 33)):
            x = G.rand((2, 3, H, W), H * W).half()
            off.append(G.bits_off(G.wb_pre_model(x, **kw).float(), G.wb_pre_ref(x).float()))
        _report("wb_pre: " + name, [0.0] + off)


def test_planted_pass_faults():
    clean, bad = [], []
    for n in (1, 255, 256, 257, 3 * 10 * 12 * 16):
        x, y = G.rand((n,), n).half().float(), G.rand((n,), n + 1).half().float()
        for a in (1.0, 0.5, -0.25, 0.0):
            ref, extra = G.axpy_ref(x, y, a), G.axpy_extra(x, y, a)
            clean.append(G.ratio(G.h16(G.axpy_model(x, y, a), f64), ref, 0.0, extra))
            bad.append(G.ratio(G.h16(G.axpy_model(x, y, a, fault="ignore_a"), f64), ref, 0.0, extra))
    _report("ppon_axpy ignores a", [max(clean)] + bad)
    x = G.slab_pair_values((2, 40, 5, 7), 3)
    hi, lo = G.slab_pair_ref(x)
    _report("pan_nchw_to_slab_pair: lo scaled by 2^10", [G.bits_off(G.slab_pair_model(x)[1].astype(f32), lo.float()), G.bits_off(G.slab_pair_model(x, 1024.0)[1].astype(f32), lo.float())])
    clean, bad = [], []
    for hw in (1, 35):
        t = G.rand((2, 8 * 32, hw), hw)
        t[:, ::5] = 0
        ref, extra = G.prefix_lrelu_ref(t, 8)
        e32 = float((T(G.prefix_lrelu_model(t, 8)).double() - ref).abs().max())
        clean.append(G.ratio(G.prefix_lrelu_model(t, 8), ref, e32, extra, rounding=False))
        bad.append(G.ratio(G.prefix_lrelu_model(t, 8, fault="feedback"), ref, e32, extra, rounding=False))
    _report("f32_prefix_lrelu feeds the activated value back", [max(clean)] + bad)


def test_planted_filter_faults():
    res = {k: [] for k in ("clean", "replicate", "b_mean_y", "no_eps", "box_ks3")}
    for fam in G.GF_FAMILIES:
        for H, W in G.GF_SIZES[1:]:
            x, y = G.gf_operands(fam, 2, H, W, 21)
            for ks in (3, 5):
                if H <= ks // 2 or W <= ks // 2:
                    continue
                ref, e, _ = G.judge_gf(x, y, ks, 1e-2)
                for fault in res:
                    if fault == "box_ks3" and ks != 5:
                        continue
                    got = G.h16(G.gf_model(x, y, ks, 1e-2, f32, fault=None if fault == "clean" else fault), f64)
                    res[fault].append((G.ratio(got, ref, e), fam, H, W, ks))
    for fault in list(res)[1:]:
        for fam in G.GF_FAMILIES:
            mine = [r[0] for r in res[fault] if r[1] == fam]
            # a flat guidance plane has cov = var = 0: A = 0 and b = mean_y whatever eps or the term A multiplies; every other family must show every fault
            if fam == "flat" and fault in ("b_mean_y", "no_eps"):
                continue
            _report(f"guided filter, {fam}: {fault}", [max(r[0] for r in res['clean'] if r[1] == fam)] + mine)
    clean, swap, circ, conv = [], [], [], []
    for H, W in G.F2D_PLANES:
        x = G.rand((2, H, W), H * W).half().float()
        for kH, kW, pl, pt in G.F2D_KERNELS:
            k = G.f2d_kernel(kH, kW, kH * 8 + kW)
            for border in range(4):
                if not G.f2d_accepts(H, W, kH, kW, pl, pt, border):
                    continue
                ref, e32, extra = G.judge_f2d(x, k, pl, pt, border)
                clean.append(G.ratio(G.h16(G.f2d_model(x, k, pl, pt, border), f64), ref, e32, extra))
                if (kH, kW) in ((4, 4), (5, 7)) and pl != pt:
                    swap.append(G.ratio(G.h16(G.f2d_model(x, k, pl, pt, border, fault="swap"), f64), ref, e32, extra))
                if border == 3 and kH * kW > 1:
                    circ.append(G.ratio(G.h16(G.f2d_model(x, k, pl, pt, border, fault="circ1"), f64), ref, e32, extra))
                if kH * kW > 1:
                    conv.append(G.ratio(G.h16(G.f2d_model(x, k, pl, pt, border, fault="conv"), f64), ref, e32, extra))
    _report("filter2d: pad_left / pad_top swapped (4 x 4, 5 x 7)", [max(clean)] + swap)
    _report("filter2d: circular off by one", [max(clean)] + circ)
    _report("filter2d: correlation turned into convolution", [max(clean)] + conv)
