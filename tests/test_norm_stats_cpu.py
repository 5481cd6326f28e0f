"""CPU side of the fp16 engine's norm-statistics tests (tests/test_gpu_norm_stats.py holds the kernels to these numbers on the GPU):
the conditions the GPU bounds rest on, proven on a float32 emulation of the device arithmetic (tests/_norm_stats_ref.py), and the host-side
plumbing of ABI 120 (innfer_conv_stats_records, the INNFER_ERR_WORKSPACE refusals).

Emulation's worst error of y = x alpha + shift against float64, relative to max(1, |y|, |x alpha|), over every case of a family (ratio = |mean - bias| / std):

    family   kind a (ratio < 1)   kind b (ratio < 7)   kind c (ratio 6 .. 10)   kind d (ratio 30, one case)
    plain        4.6e-07              4.0e-06              1.2e-05                 1.8e-05
    up           3.5e-07              3.9e-07              3.4e-06                 5.9e-06
    down         2.6e-07              2.6e-06              8.4e-06                 3.3e-05
    col          3.3e-07              2.0e-06              9.4e-06                 1.8e-05

The hard ceiling of the GPU tests is 2^-12 = 2.4e-4; a tenth of it holds on every case of kinds a .. c, so the working bound (8 x these numbers) stays below the
ceiling.  At ratio 30 the one-pass M2 = s2 - s1 * mean of (x - bias) has lost a further decimal digit against ratio 8 in the records themselves (5e-4 .. 6e-3 of M2
against 1e-4 .. 2e-4), which the merged variance averages down."""
import ctypes as C

import numpy as np
import pytest

import _norm_stats_ref as R
import innfer_amd.lib as L


@pytest.mark.parametrize("family", list(R.CASES))
def test_emulation_is_a_tenth_of_the_ceiling(family):
    """On every case the GPU test runs with kinds a .. c: kind c's ratio lies in [6, 10] on every (image, channel) with more than one pixel, the emulated records
    partition the image (counts sum to the pixels of the output), and the emulation's y error is at most CEILING / 10."""
    for c in R.CASES[family]:
        Ho, Wo = R.out_hw(c)
        _, mask = R.regions(c, np.zeros((1, 1, Ho, Wo)))
        assert mask.shape[0] == R.records_per_image(c.H, c.W, R.phases(c)) and mask.sum() == Ho * Wo, R.case_id(c)
        for kind in R.KINDS:
            d = R.data(c, kind)
            e = R.emulation_error(c, kind)
            print("%-28s %s  ratio [%.2f, %.2f]  emulation: y %.2e  records %.2e" % (R.case_id(c), kind, np.nanmin(d.ratio), np.nanmax(d.ratio), e.y, e.rec))
            if Ho * Wo > 1:
                assert np.isfinite(d.ratio).all(), (R.case_id(c), kind)
                if kind == "c":
                    assert d.ratio.min() >= 6.0 and d.ratio.max() <= 10.0, (R.case_id(c), d.ratio.min(), d.ratio.max())
                else:
                    assert d.ratio.max() <= 8.0, (R.case_id(c), kind, d.ratio.max())
            assert e.y <= R.CEILING / 10, (R.case_id(c), kind, e.y)
        assert d.y.abs().max().item() < 100.0                      # far inside fp16
    for kind in R.KINDS:
        yb, rb = R.working_bounds(family, kind)
        assert 0 < yb <= R.CEILING, (family, kind, yb)
        print("%s %s: working bounds  y %.2e  records %.2e" % (family, kind, yb, rb))


def test_emulation_at_ratio_30_is_recorded():
    """Characterisation (kind d): the emulation's error where |mean - bias| / std = 30 -- printed, and written into this file's docstring and docs/KERNELS.md 3.1;
    not held to the working bound."""
    for c in R.D_CASES:
        d = R.data(c, "d")
        e = R.emulation_error(c, "d")
        assert 25.0 <= d.ratio.min() and d.ratio.max() <= 35.0, (R.case_id(c), d.ratio.min(), d.ratio.max())
        assert np.isfinite(e.y) and np.isfinite(e.rec)
        print("%-28s d  ratio [%.1f, %.1f]  emulation: y %.2e  records %.2e" % (R.case_id(c), d.ratio.min(), d.ratio.max(), e.y, e.rec))


def test_float64_merge_of_float64_records_is_the_plane_statistics():
    """The record geometry and both merge orders, checked without rounding in the way: Chan's update over the float64 records of a ragged, phased case gives the
    plane's own mean and variance."""
    for c in (R.Case("plain", 3, 64, 64, 33, 65, 0), R.Case("up", 3, 64, 64, 7, 5, 3)):
        d = R.data(c, "b")
        y = d.y.numpy()
        vals, mask = R.regions(c, y)
        cnt, mean, M2 = R.records64(vals, mask)
        HW = y.shape[2] * y.shape[3]
        for order in (np.arange(len(cnt)), np.argsort(np.arange(len(cnt)) % 8, kind="stable")):
            n, mu, m2 = 0.0, np.zeros(mean[:, 0].shape), np.zeros(mean[:, 0].shape)
            for r in order:
                if cnt[r] == 0:
                    continue
                tot = n + cnt[r]
                dl = mean[:, r] - mu
                mu = mu + dl * (cnt[r] / tot)
                m2 = m2 + M2[:, r] + dl * dl * (n * cnt[r] / tot)
                n = tot
            assert n == HW
            assert np.abs(mu - d.mean).max() < 1e-12 and np.abs(m2 / HW - d.var).max() < 1e-12


def test_conv_stats_records_formula():
    for H in (1, 2, 15, 16, 17, 33, 37, 256):
        for W in (1, 16, 17, 31, 32, 33, 65, 70, 256):
            for ph in (1, 4):
                assert L.lib.innfer_conv_stats_records(H, W, ph) == -(-H // 16) * -(-W // 32) * ph * 8 == R.records_per_image(H, W, ph)
    assert L.lib.innfer_conv_stats_records(33, 65, 1) == 72
    for bad in ((0, 4, 1), (4, 0, 1), (4, 4, 2), (4, 4, 0)):
        assert L.lib.innfer_conv_stats_records(*bad) == L.ERR_INVALID


def test_short_statistics_buffers_are_refused_on_the_host():
    """ABI 120: a d_stats_part of fewer than N * records * channels * 3 floats is INNFER_ERR_WORKSPACE on every branch of innfer_conv3x3_f16 that takes
    statistics, before anything is launched (the pointers here are never dereferenced); likewise innfer_norm_stats' segment scratch."""
    assert L.ABI_VERSION == 124 == L.lib.innfer_version()
    fake = 0x1000
    for kw, ph in ((dict(K=64), 1), (dict(K=128), 1), (dict(K=64, stride2_k4=1), 1), (dict(K=64, transposed2x=4), 4), (dict(K=128, transposed2x=3), 4),
                   (dict(K=64, column7=1), 1)):
        a = L.ConvArgs(d_in=fake, d_packed=fake, d_bias=fake, d_out=fake, C=32, N=3, H=17, W=33, in_group_stride=1 << 20, out_group_stride=1 << 20, **kw)
        need = 3 * R.records_per_image(17, 33, ph) * kw["K"] * 3
        a.d_stats_part = fake
        for short in (0, need - 1):
            a.stats_part_floats = short
            assert L.lib.innfer_conv3x3_f16(C.byref(a), None) == L.ERR_WORKSPACE, (kw, short)
            assert "stats_part_floats" in L.last_error()
    assert L.lib.innfer_norm_stats(fake, 0, 0, 64, 1025, 1e-5, None, None, fake, fake, 40, 2, fake, 2 * 40 * 2 * 2 - 1, None) == L.ERR_WORKSPACE
    assert L.lib.innfer_norm_stats(fake, 1, 2 * 4097 * 32, 0, 4097, 1e-5, None, None, fake, fake, 40, 2, None, 0, None) == L.ERR_WORKSPACE
    assert L.lib.innfer_norm_stats(fake, 1, 2 * 4097 * 32 - 1, 0, 4097, 1e-5, None, None, fake, fake, 40, 2, fake, 1 << 20, None) == L.ERR_INVALID
    assert L.lib.innfer_norm_combine_parts(None, 8, 4, 1e-5, None, None, fake, fake, 64, 1, None) == L.ERR_INVALID
    assert L.lib.innfer_resnet_post_slab_parts(fake, 64, 48, 4, 1, fake, 8, None, None, 0, None, fake, None) == L.ERR_INVALID            # C % 32
    assert L.lib.innfer_unet_post_slab_parts(fake, 128, 64, 4, 1, fake, 8, None, None, fake, 128, 4, 1, None, 0, 0, 0, None) == L.ERR_INVALID   # offset % 8


# ------------------------------------------------------------------------------------------------ the GPU test's checks have teeth
def _emulated_run(c, kind, cnt=None, mask_of=None, merge=None, merge8=None):
    """What the device computes for (case, kind) in the form test_gpu_norm_stats._judge takes, from the float32 emulation -- with a fault planted where asked:
    cnt: the records' counts; mask_of: the validity mask; merge: chan_merge; merge8: the 8-lane merge of the in-network kernels."""
    import types

    import torch

    import test_gpu_norm_stats as T
    d = R.data(c, kind)
    ref = R.reference_records(c, kind)
    y = d.y.numpy()
    HW = y.shape[2] * y.shape[3]
    mask = ref.mask if mask_of is None else mask_of(ref.mask)
    part = R.emulate_records(ref.vals, mask, d.b.numpy(), (mask.sum(1) if mask_of is not None else None) if cnt is None else cnt)
    slab = T._to_slab(d.y.float())
    r = {"cv": types.SimpleNamespace(HW=HW), "slab0": slab, "slab": slab, "part": part}
    aff = [R.affine(c, which) for which in (0, 1)]
    _, mu, m2 = R.emulate_merge(part, 32, merge)
    r["alpha_shift"] = [R.alpha_shift32(mu, m2, HW, *aff[which]) for which in (0, 1)]
    _, mu, m2 = merge8(part) if merge8 else R.emulate_merge(part, 8, merge)
    x16 = T._from_slab(slab).float().numpy()
    r["res"] = torch.from_numpy(np.random.default_rng(7).uniform(-2, 2, y.shape).astype(np.float32)).half()
    res = r["res"].float().numpy()
    r["posts"] = {}
    for name, act, with_res, which in (("rn plain", 0, False, 0), ("rn relu+res+affine", 2, True, 1), ("unet lrelu+affine", 1, False, 1), ("unet relu", 2, False, 0)):
        a, s = R.alpha_shift32(mu, m2, HW, *aff[which])
        v = x16 * a[..., None, None] + s[..., None, None]
        v = np.maximum(v, np.float32(0.2) * v) if act == 1 else np.maximum(v, np.float32(0)) if act == 2 else v
        r["posts"][name] = (torch.from_numpy((v + res if with_res else v).astype(np.float32)).half(), act, with_res, which)
    return r


def _verdict(c, kind, **fault):
    import test_gpu_norm_stats as T
    try:
        return T._judge(c, kind, _emulated_run(c, kind, **fault))
    except AssertionError as e:
        return ["assert: " + str(e)[:80]]


def test_planted_faults_fail_the_gpu_checks():
    """test_gpu_norm_stats' verdict (_judge: assertions 1 .. 5) run on the float32 emulation in place of the device: the faithful emulation passes on a ragged case of
    every family, and each of these faults, planted into the emulation as it would sit in the kernels, fails -- named with the check that catches it:
      the `cols` clamp of epilogue_stats dropped (count = rows * 32 whatever the image's width) ............. the records' counts (every case with W % 32 != 0)
      the phase lattice's shift not taken back (`yw -= ph >> 1; x0 -= ph & 1`) ............................. the records' counts (every transposed case)
      chan_merge's n * nb / tot taken as nb ................................................................. combine_parts' y and the in-network merges' outputs
      an `rr < nper` guard dropped (the clamped record merged with its own count) .......................... the in-network merges' outputs, where nper % 32 != 0
                                                                                                             and the last record holds pixels (16 x 32; 48 x 65)
    The fifth fault of that kind, the `2 q + sg >= N` skip of the image-pair forms, writes the missing image's records behind the last image's: the N * records *
    channels * 3 floats hold what they should and the sentinel behind them (a whole image's records wide) does not -- _Conv.run's check, on the odd batches."""
    f = np.float32
    wide, up, small, trips = R.Case("plain", 3, 64, 64, 33, 65, 0), R.Case("up", 2, 64, 64, 17, 40, 3), R.Case("plain", 1, 64, 64, 16, 32, 0), R.Case("plain", 1, 64, 64, 48, 65, 0)
    for c in (wide, up, small, trips, R.Case("down", 3, 32, 64, 5, 7, 0), R.Case("col", 2, 32, 64, 23, 40, 1)):
        assert c in R.ALL_CASES
        for kind in R.KINDS:
            assert _verdict(c, kind) == [], (R.case_id(c), kind)

    # the cols clamp
    ref = R.reference_records(wide, "a")
    rows = ref.mask.reshape(-1, R.RPW, R.TW).any(2).sum(1)
    got = _verdict(wide, "a", cnt=rows * R.TW)
    assert got and "count" in got[0], got

    # the phase shift: phase (a, b) loses the pixels with y + a >= H or x + b >= W
    def shifted(mask):
        ty, tx = -(-up.H // R.TH), -(-up.W // R.TW)
        m = mask.reshape(ty, tx, 4, R.NCW, R.RPW, R.TW).copy()
        ys = (np.arange(ty)[:, None, None] * R.TH + np.arange(R.NCW)[None, :, None] * R.RPW + np.arange(R.RPW)[None, None, :])          # [ty, wave, row]
        xs = np.arange(tx)[:, None] * R.TW + np.arange(R.TW)[None, :]                                                                    # [tx, col]
        for ph in range(4):
            ok = (ys[:, None, :, :, None] + (ph >> 1) < up.H) & (xs[None, :, None, None, :] + (ph & 1) < up.W)
            m[:, :, ph] &= ok
        return m.reshape(mask.shape)
    got = _verdict(up, "a", mask_of=shifted)
    assert got and "count" in got[0], got

    # chan_merge's factor
    def merge_nb(n, mu, m2, nb, mub, m2b):
        with np.errstate(divide="ignore", invalid="ignore"):
            tot, dl = n + nb, mub - mu
            mu2, m22 = mu + dl * (nb / tot), m2 + (m2b + dl * dl * nb)
        ok = nb > 0
        return np.where(ok, tot, n).astype(f), np.where(ok, mu2, mu).astype(f), np.where(ok, m22, m2).astype(f)
    for kind in R.KINDS:
        got = _verdict(wide, kind, merge=merge_nb)
        assert any("combine_parts" in g for g in got) and any("rn " in g for g in got) and any("unet " in g for g in got), (kind, got)

    # an rr < nper guard
    def merge8_unguarded(rec):
        N, nper, K, _ = rec.shape
        lanes = []
        for lg in range(8):
            n, mu, m2 = (np.zeros((N, K), f) for _ in range(3))
            for r0 in range(lg, nper, 32):
                for j in range(4):
                    q = rec[:, min(r0 + 8 * j, nper - 1)]
                    n, mu, m2 = R._chan_merge(n, mu, m2, q[..., 0], q[..., 1], q[..., 2])
            lanes.append((n, mu, m2))
        n, mu, m2 = lanes[0]
        for ln in lanes[1:]:
            n, mu, m2 = R._chan_merge(n, mu, m2, *ln)
        return n, mu, m2
    for c in (small, trips):
        for kind in R.KINDS:
            got = _verdict(c, kind, merge8=merge8_unguarded)
            assert any("rn " in g for g in got) and any("unet " in g for g in got) and not any("combine_parts" in g for g in got), (R.case_id(c), kind, got)
    assert _verdict(wide, "a", merge8=merge8_unguarded) == []          # 33 x 65 ends in a wave outside the image: count 0, the dropped guard changes nothing there
