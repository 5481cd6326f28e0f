"""The planner of the fp32 mode's generic convolution (csrc/f32ops.hip f32conv_plan, through the host-only innfer_f32conv_plan): the batch
invariance the kernels' bit-exactness rests on, the exact boundary of the tiled kernel's 32-bit offset gate, and the plans of 4K frames."""
import pytest

import innfer_amd.lib as L
from oracle import f32conv as O

FAKE = 1 << 20                                   # an aligned, non-null address: the planner never dereferences a pointer
GATE = (1 << 29) - 1                             # tiled iff (CC in_cstride + IMG in_nstride + Hin Win) * 4 < 0x7fffffff


def _args(case, d, N=None, in_nstride=None, in_cstride=None, form=0):
    Ho, Wo = case.out_hw
    hw = case.H * case.W
    kw = dict(d)
    taps = kw.pop("taps")
    if N is not None:
        kw["N"] = N
    rows = case.kind == "rows"
    return L.f32conv_args(
        taps, d_in=FAKE, in_nstride=case.ctot * hw if in_nstride is None else in_nstride, in_cstride=hw if in_cstride is None else in_cstride,
        d_packed=FAKE, d_bias=FAKE, d_out=FAKE,
        out_nstride=Ho * Wo * 64 if rows else case.ktot * Ho * Wo, out_cstride=1 if rows else Ho * Wo, out_pstride=64 if rows else 1,
        d_res=FAKE if case.res else None, res_nstride=case.K * Ho * Wo, res_cstride=Ho * Wo,
        d_mul=FAKE if case.mul else None, mul_nstride=case.K * Ho * Wo, mul_cstride=Ho * Wo, form=form, **kw)


def test_plan_is_batch_invariant():
    """(IMG, NPT, CC) come from a nominal batch of 64 (f32conv_plan): CC is the order of the sums, so a batch equals its images' own forwards bit for
    bit only if they do not follow N.  Every launch of the GPU sweep (oracle/f32conv.sweep), N = 1 .. 130."""
    n = 0
    for case in O.sweep():
        for d, _w, _m in O.launches(case):
            p1 = L.f32conv_plan(_args(case, d, N=1))
            assert not p1["direct"], (case.name, p1)
            for N in range(2, 131):
                p = L.f32conv_plan(_args(case, d, N=N))
                assert (p["direct"], p["IMG"], p["NPT"], p["CC"]) == (0, p1["IMG"], p1["NPT"], p1["CC"]), (case.name, N, p1, p)
                n += 1
    assert n > 10000


def test_offset_gate_boundary():
    """The tiled kernel addresses its patch with 32-bit byte offsets; f32conv_plan admits a view iff (CC in_cstride + IMG in_nstride + Hin Win) * 4
    < 2^31 - 1.  Views whose extent sits on either side of that bound, reached through in_cstride and through in_nstride, on an IMG = 1 plan and an
    IMG > 1 plan."""
    cases = [O.Case("img1", 2, 4, 9, 11, 16), O.Case("img1_c3", 1, 3, 17, 40, 24, pad_mode=1), O.Case("imgN", 65, 512, 2, 2, 512, k=4, stride=2, pad=1)]
    saw_img = set()
    for case in cases:
        d = O.launches(case)[0][0]
        hw = case.H * case.W
        p = L.f32conv_plan(_args(case, d))
        CC, IMG = p["CC"], p["IMG"]
        saw_img.add(IMG)
        assert not p["direct"] and CC > 0
        # through in_cstride (in_nstride 0: every image reads the same view)
        cs = (GATE - hw) // CC
        assert GATE - CC < CC * cs + hw <= GATE
        assert L.f32conv_plan(_args(case, d, in_nstride=0, in_cstride=cs))["direct"] == 0, case.name
        assert L.f32conv_plan(_args(case, d, in_nstride=0, in_cstride=cs + 1))["direct"] == 1, case.name
        # through in_nstride
        cs = hw
        ns = (GATE - hw - CC * cs) // IMG
        assert GATE - IMG < CC * cs + IMG * ns + hw <= GATE
        assert L.f32conv_plan(_args(case, d, in_nstride=ns, in_cstride=cs))["direct"] == 0, case.name
        assert L.f32conv_plan(_args(case, d, in_nstride=ns + 1, in_cstride=cs))["direct"] == 1, case.name
        if IMG == 1:                                           # exactly at the bound: the last admitted extent is 2^31 - 4 bytes
            ns = GATE - hw - CC * cs
            assert L.f32conv_plan(_args(case, d, in_nstride=ns, in_cstride=cs))["direct"] == 0
            assert L.f32conv_plan(_args(case, d, in_nstride=ns + 1, in_cstride=cs))["direct"] == 1
    assert 1 in saw_img and max(saw_img) > 1, saw_img


def test_4k_frame_plans():
    """What the fp32 layers of a 3840 x 2160 frame run (recorded from the planner).  The gate counts the whole first image (IMG in_nstride), so the
    CycleGAN ResNet layers that read its 64-channel full-resolution tensor (stride-2 down conv, last 7 x 7 conv, 2.1 GB per image) take the direct
    kernel; the WBC UNet's 32-channel full-resolution layers (1.06 GB) stay on the tiled kernel."""
    H, W = 2160, 3840
    expect = [
        (O.Case("resnet_down_s2", 1, 64, H, W, 128, stride=2), dict(direct=1)),                        # resnet.hip:640
        (O.Case("resnet_c7_last", 1, 64, H, W, 3, k=7, pad_mode=1, act=3), dict(direct=1)),            # resnet.hip:651
        (O.Case("resnet_block_64", 1, 64, H, W, 64, pad_mode=1), dict(direct=1)),
        (O.Case("wbc_conv8", 1, 32, H, W, 32, act=1), dict(direct=0, NKT=2, NPT=4, IMG=1, CC=8, vec4=1)),      # wbcunet.hip:445
        (O.Case("wbc_conv1_pt", 1, 32, H, W, 32, stride=2, act=1), dict(direct=0, NKT=2, NPT=4, IMG=1, CC=4, vec4=1)),     # wbcunet.hip:430
        (O.Case("wbc_conv1_tf", 1, 32, H, W, 32, stride=2, tf=True, act=1), dict(direct=0, NKT=2, NPT=4, IMG=1, CC=4, vec4=1)),
        (O.Case("wbc_conv9", 1, 32, H, W, 3, k=7), dict(direct=0, NKT=1, NPT=4, IMG=1, CC=4, vec4=1)),     # wbcunet.hip:446
    ]
    for case, want in expect:
        p = L.f32conv_plan(_args(case, O.launches(case)[0][0]))
        assert {k: p[k] for k in want} == want, (case.name, p)
        if p["direct"]:
            assert p["NKT"] == p["CC"] == p["lds"] == 0 and p["workgroups"] > 0


def test_plan_reports_errors_and_forced_direct():
    """form 1 always plans the direct kernel; bad arguments are refused without a device."""
    case = O.Case("small", 2, 20, 9, 9, 24)
    d = O.launches(case)[0][0]
    assert L.f32conv_plan(_args(case, d, form=1))["direct"] == 1
    a = _args(case, d)
    a.form = 2
    with pytest.raises(ValueError):
        L.f32conv_plan(a)
    a = _args(case, d)
    a.ntap = 0
    with pytest.raises(ValueError):
        L.f32conv_plan(a)
