"""CPU side of the first-conv and slab-pass tests (tests/test_gpu_first_conv.py holds the kernels to these on the GPU): every reference of
tests/_first_conv_ref.py against the torch module it restates; the pair term of the split output against float32 values pushed through the pair; the case list's
reach; and planted faults -- each must be rejected by the GPU test's comparator at a case of the GPU test's own list, named here, where the fault-free model of
the declared arithmetic passes.

Figures printed by test_case_errors (worst over the GPU test's cases of a kind): e32, e_split and what the same model costs with its subnormal low parts lost.
"""
import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import _first_conv_ref as R
import innfer_amd.lib as L
import oracle.convert

f16, f32, f64 = np.float16, np.float32, np.float64


# ------------------------------------------------------------------------------------------------ the references restate the modules
@pytest.mark.parametrize("a", R.ACTS)
def test_conv_reference_is_conv2d_plus_activation(a):
    g = torch.Generator().manual_seed(a)
    for Cc, K, H, W in ((1, 32, 1, 1), (3, 64, 5, 7), (8, 32, 4, 17)):
        x = torch.randn(2, Cc, H, W, generator=g, dtype=torch.float64)
        conv = nn.Conv2d(Cc, K, 3, 1, 1).double()
        prelu = nn.PReLU(K).double()
        with torch.no_grad():
            prelu.weight.copy_(torch.rand(K, generator=g, dtype=torch.float64) - 0.5)
            net = nn.Sequential(conv, {0: nn.Identity(), 1: nn.LeakyReLU(0.2), 2: nn.ReLU(), 8: prelu}[a])
            got = R.conv_ref(x.numpy(), conv.weight.numpy(), conv.bias.numpy(), a, prelu.weight.numpy())
            assert np.abs(got - net(x).numpy()).max() < 1e-12
            # the float32 twin (e32) and the fault-free model agree with it to float32 accuracy
            x32, w32, b32, s32 = x.float().numpy(), conv.weight.float().numpy(), conv.bias.float().numpy(), prelu.weight.float().numpy()
            ref = R.conv_ref(x32, w32, b32, a, s32)
            assert np.abs(R.conv_f32(x32, w32, b32, a, s32) - ref).max() < 1e-5
            assert np.abs(R.split_model(x32, w32, b32, a, s32) - ref).max() < 1e-5


def test_patches_are_unfold():
    x = torch.randn(2, 3, 5, 18, dtype=torch.float64)
    want = F.unfold(x, 3, padding=1).view(2, 3, 3, 3, 5, 18).numpy()
    assert np.array_equal(R.patches(x.numpy()), want)


@pytest.mark.parametrize("Cc", (1, 3, 4))
def test_np2tensor_restatement_is_the_projects(Cc):
    img = R.u8_images(2, 5, 7, Cc)
    for normalize in (False, True):
        want = torch.cat([oracle.convert.np2tensor(img[n], normalize=normalize) for n in range(2)])
        got = R.np2tensor_np(img, normalize, False)
        assert got.dtype == f32 and torch.equal(R.bits16(torch.from_numpy(got).view(torch.int16)), R.bits16(want.contiguous().view(torch.int16)))
        assert torch.equal(torch.from_numpy(R.np2tensor_np(img, normalize, True)), want.half().float())
    if Cc == 4:                     # alpha stays in place
        assert np.array_equal(R.np2tensor_np(img, False, False)[:, 3], img[..., 3].astype(f32) / f32(255))


def test_exact_pass_references_are_torch():
    g = torch.Generator().manual_seed(5)
    for H, W in R.SLAB_GRIDS:
        x = torch.randn(2, 72, H, W, generator=g)
        for f in (2, 3):
            assert np.array_equal(R.upsample_ref(x.numpy(), f), F.interpolate(x, scale_factor=f, mode="nearest").numpy())
        for r in (2, 3):
            assert np.array_equal(R.shuffle_ref(x.numpy(), r), F.pixel_shuffle(x, r).numpy())


def test_input_map_reference_is_norm_act():
    x, al, sh = R.map_data(40, 2, 3, 5)
    for a, mod in ((0, nn.Identity()), (1, nn.LeakyReLU(0.2)), (2, nn.ReLU())):
        ref, mag = R.pass_ref(x, al.astype(f64)[None, :, None, None], sh.astype(f64)[None, :, None, None], a)
        want = mod(torch.from_numpy(x).double() * torch.from_numpy(al).double().view(1, -1, 1, 1) + torch.from_numpy(sh).double().view(1, -1, 1, 1))
        assert np.abs(ref - want.numpy()).max() < 1e-12 and (mag >= np.abs(ref) - 1e-12).all()
    assert (np.abs(al) >= 0.5).all() and (al < 0).any() and (al > 0).any()


# ------------------------------------------------------------------------------------------------ the pair term
def test_pair_term_bounds_the_pairs_own_error():
    """float32 values of every magnitude the tests meet, pushed through (hi, lo): |hi + lo 2^-11 - v| <= pair_term(v), and the term is not slack by more than the
    rounding mode leaves (some value comes within a factor 2 of it)"""
    rng = np.random.default_rng(3)
    worst = 0.0
    for scale in (2.0 ** -20, 2.0 ** -14, 2.0 ** -8, 1e-2, 1.0, 37.0, 1000.0):
        v = (scale * rng.uniform(-1, 1, 200000)).astype(f32)
        hi, lo = R.to_pair(v)
        err = np.abs(R.pair_value(hi, lo) - v.astype(f64))
        term = R.pair_term(v.astype(f64))
        assert (err <= term).all(), scale
        worst = max(worst, float((err / term).max()))
    assert worst > 0.5, worst
    assert R.pair_term(np.array(1.0)) == 2.0 ** -22 and R.pair_term(np.array(0.0)) == 2.0 ** -36


# ------------------------------------------------------------------------------------------------ the case list
def test_case_list_reaches_every_instantiation():
    cases = R.first_cases()
    assert len(cases) == len(R.FIRST_K) * len(R.FIRST_C) * len(R.FIRST_HW) and len(R.ALL_FORMS) == 24
    assert set().union(*(R.case_forms(c) for c in cases)) == R.ALL_FORMS
    for K in R.FIRST_K:
        for Cc in R.FIRST_C:
            sub = R.first_cases(K, Cc)
            assert {(c.H, c.W) for c in sub} == set(R.FIRST_HW) and {c.act for c in sub} == set(R.ACTS) and {c.N for c in sub} == {1, 3}
            assert {(c.kind, c.act) for c in sub} == {(k, a) for k in "AB" for a in R.ACTS}
            assert any(c.kind == "B" and c.act != 8 for c in sub)                  # the sharpest check: a split-output case at kind B
    assert all(c.H <= 33 and c.W <= 130 and c.N <= 3 for c in cases)


def test_kind_b_low_parts_are_all_subnormal():
    for case in R.first_cases(64, 3)[:4]:
        x32, _, w, _, _ = R.first_data(case)
        for v in (x32, w):
            lo = R.split16(v)[1]
            if case.kind == "B":
                assert (np.abs(lo) < 2.0 ** -14).all() and (lo != 0).any()
            else:
                assert (np.abs(lo) >= 2.0 ** -14).any()


def test_case_errors():
    """e of the cases: the declared arithmetic is float32-accurate; with the subnormal low parts lost it is not, by the factors the kinds were chosen for"""
    worst = {}
    for case in R.first_cases(64, 3) + R.first_cases(32, 8):
        if case.H * case.W < 200:
            continue
        x32, _, w, b, slope = R.first_data(case)
        ref = R.conv_ref(x32, w, b, case.act, slope)
        e = R.case_e(case, 32)
        lost = float(np.abs(R.split_model(x32, w, b, case.act, slope, "flush") - ref).max())
        k = worst.setdefault(case.kind, [0.0, 0.0])
        k[0], k[1] = max(k[0], e), max(k[1], lost)
        # float32 accuracy.  Kind B: the unscaled subnormal remainders carry an ABSOLUTE 2^-25 each, which |w| ~ 0.04 over up to 72 taps (and |x| <= 2^-4 likewise)
        # turns into at most 2 * 72 * 0.06 * 2^-25 = 2.6e-7 -- still 1e-5 of the outputs
        assert e < (2e-6 if case.kind == "A" else 2.6e-7), (case, e)
    for kind, (e, lost) in sorted(worst.items()):
        print("MEASURED kind %s: largest e %.2e, low parts lost %.2e" % (kind, e, lost))
    assert worst["B"][1] > 100 * worst["B"][0]


# ------------------------------------------------------------------------------------------------ planted faults
def _find(K, Cc, pred):
    for c in R.first_cases(K, Cc):
        if pred(c):
            return c
    raise AssertionError("no such case in the GPU test's list")


def _ratios(case, which, split, fault):
    """(fault-free, faulty) worst err / bound of the model's output stored as the kernel stores it, under the GPU test's comparator"""
    x32, x16, w, b, slope = R.first_data(case)
    x = x16 if which == 16 else x32
    ref = R.conv_ref(x, w, b, case.act, slope)
    e = R.case_e(case, which)
    out = []
    for flt in (None, fault):
        v = R.split_model(x, w, b, case.act, slope, flt)
        if split:
            got = R.pair_value(*R.to_pair(v))
            out.append(R.worst_ratio(got, ref, R.pair_bound(ref, got, e)))
        else:
            got = v.astype(f16).astype(f64)
            out.append(R.worst_ratio(got, ref, R.store_bound(ref, got, e)))
    return out


FAULTS = (
    # fault, (K, in_nc), the case's predicate, input (16 | 32), split output
    ("wl_xh", (64, 3), lambda c: c.kind == "B" and c.act != 8 and c.H * c.W > 500, 32, True),
    ("wl_xh", (32, 4), lambda c: c.kind == "A" and c.act != 8 and c.H * c.W > 500, 16, False),
    ("xl_wh", (64, 8), lambda c: c.kind == "B" and c.act != 8 and c.H * c.W > 500, 32, True),
    ("xl_wh", (32, 1), lambda c: c.kind == "A" and c.act != 8 and c.H * c.W > 500, 32, True),
    ("flush", (64, 3), lambda c: c.kind == "B" and c.act != 8 and c.H * c.W > 500, 32, True),
    ("flush", (32, 7), lambda c: c.kind == "B" and c.H * c.W > 500, 16, False),
    ("taps", (64, 4), lambda c: c.H > 1 and c.W > 1, 16, False),
    ("top", (32, 3), lambda c: c.H > 1, 16, False),
    ("strip", (64, 1), lambda c: c.W > 16, 16, False),
    ("slope", (32, 8), lambda c: c.act == 8 and c.H * c.W > 16, 16, False),
    ("slope", (64, 7), lambda c: c.act == 8 and c.H * c.W > 16, 32, False),
)


@pytest.mark.parametrize("fault,kc,pred,which,split", FAULTS, ids=["%s-%d-%d-%d%s" % (f[0], f[1][0], f[1][1], f[3], "-pair" if f[4] else "") for f in FAULTS])
def test_planted_fault_is_rejected(fault, kc, pred, which, split):
    case = _find(kc[0], kc[1], pred)
    ok, bad = _ratios(case, which, split, fault)
    print("MEASURED %s at %s: fault-free %.3f, faulty %.3g" % (fault, case, ok, bad))
    assert ok <= 1.0, (case, ok)
    assert bad > 1.0, (case, bad)


def test_bgra_flipped_as_four_channels_is_rejected():
    img = R.u8_images(1, 15, 63, 4)                       # a uint8 case of the GPU test: C = 4 at 15 x 63
    assert not np.array_equal(R.np2tensor_np(img, False, True), R.np2tensor_np(img, False, True, flip="all4"))
    assert np.array_equal(R.np2tensor_np(img, False, True)[:, 1], R.np2tensor_np(img, False, True, flip="all4")[:, 2])


def test_exact_pass_faults_are_rejected():
    """At the smallest grid of the GPU test that can show them (3 x 5; at 1 x 1 nearest-up is a broadcast and cannot)"""
    x = np.arange(2 * 72 * 3 * 5, dtype=f32).reshape(2, 72, 3, 5)
    for r in (2, 3):
        assert not np.array_equal(R.shuffle_ref(x, r), R.shuffle_ref(x, r, "ij"))
    for f in (2, 3):
        assert not np.array_equal(R.upsample_ref(x, f), R.upsample_ref(x, f, "up"))
    one = x[:, :, :1, :1]
    assert np.array_equal(R.upsample_ref(one, 3), R.upsample_ref(one, 3, "up")) and not np.array_equal(R.shuffle_ref(one, 2), R.shuffle_ref(one, 2, "ij"))


def test_input_map_comparators_reject_a_neighbouring_channel():
    """alpha of channel c ^ 1, and the lo twin left out of the split form's operand"""
    x, al, sh = R.map_data(64, 2, 7, 11)
    a64, s64 = al.astype(f64)[None, :, None, None], sh.astype(f64)[None, :, None, None]
    xs = x.astype(f16).astype(f64)
    ref, mag = R.pass_ref(xs, a64, s64, 1)
    good = np.maximum(xs * a64 + s64, 0.2 * (xs * a64 + s64)).astype(f32).astype(f16).astype(f64)
    assert R.worst_ratio(good, ref, R.pass_bound(ref, good, mag)) <= 1.0
    wrong = R.pass_ref(xs, a64[:, np.arange(64) ^ 1], s64, 1)[0].astype(f16).astype(f64)
    assert R.worst_ratio(wrong, ref, R.pass_bound(ref, wrong, mag)) > 1.0
    hi, lo = R.to_pair(x)
    xp = R.pair_value(hi, lo)
    ref, mag = R.pass_ref(xp, a64, s64, 0)
    good = R.pair_value(*R.to_pair((xp * a64 + s64).astype(f32)))
    assert R.worst_ratio(good, ref, R.map_split_bound(ref, good, mag)) <= 1.0
    nolo = R.pair_value(*R.to_pair((hi.astype(f64) * a64 + s64).astype(f32)))
    assert R.worst_ratio(nolo, ref, R.map_split_bound(ref, nolo, mag)) > 1.0


# ------------------------------------------------------------------------------------------------ refusals (nothing launches: no pointer is dereferenced)
def test_entry_points_refuse():
    assert L.ABI_VERSION == 124 == L.lib.innfer_version()
    n = 0
    for what, rc, want in R.refusals(L):
        assert rc == want, (what, rc, L.last_error())
        assert L.last_error(), what
        n += 1
    assert n > 30
