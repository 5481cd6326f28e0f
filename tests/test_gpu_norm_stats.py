"""The fp16 engine's norm statistics, launch by launch, against float64 (needs an MI355X: `pytest -m gpu`).

Under test: the (count, mean, M2) records the conv kernels write from their epilogue (csrc/conv3x3_stats_gate_rlds.h epilogue_stats -- all six instantiations:
plain 3x3, the stride-2 conv and the transposed conv's phases in their wide and image-pair forms, the 7 x 1 column conv), the three merges of those records
(norm::combine_parts_kernel, rn_post_slab_parts, unet_post_slab_parts) and the re-read kernels (stats_kernel<false>, stats_slab8_kernel, combine_kernel), through
the test entry points of ABI 120.  Cases, data kinds, the float64 reference and the float32 emulation the bounds come from: tests/_norm_stats_ref.py.

Metric: y = x alpha + shift at the channel's min, max and mean x, error relative to max(1, |y|, |x alpha|).  Hard ceiling 2^-12 (kinds a .. c); working bound
8 x the emulation's worst error over the family's cases of that kind (tests/test_norm_stats_cpu.py lists the emulation's numbers).

Worst error per family and data kind -- emulation / measured on an MI355X (records: mean relative to max(1, |mean|), M2 relative to max(1, M2)):
    family  kind   y: emulation / measured (working bound)    records: emulation / measured
    plain    a       4.6e-07 / 1.9e-06  (3.7e-06)               5.6e-07 / 9.2e-07
    plain    b       4.0e-06 / 6.7e-06  (3.2e-05)               2.1e-05 / 5.2e-06
    plain    c       1.2e-05 / 7.1e-06  (9.6e-05)               1.3e-04 / 3.6e-05
    up       a       3.5e-07 / 3.8e-07  (2.8e-06)               5.2e-07 / 5.4e-07
    up       b       3.9e-07 / 4.6e-07  (3.1e-06)               2.2e-05 / 6.8e-06
    up       c       3.4e-06 / 2.2e-06  (2.7e-05)               2.0e-04 / 9.0e-05
    down     a       2.6e-07 / 2.9e-07  (2.1e-06)               4.3e-07 / 5.7e-07
    down     b       2.6e-06 / 9.0e-07  (2.1e-05)               1.6e-05 / 5.9e-06
    down     c       8.4e-06 / 5.0e-06  (6.7e-05)               8.1e-05 / 3.5e-05
    col      a       3.3e-07 / 2.5e-07  (2.6e-06)               4.3e-07 / 5.1e-07
    col      b       2.0e-06 / 7.0e-07  (1.6e-05)               3.0e-05 / 8.1e-06
    col      c       9.4e-06 / 3.8e-06  (7.5e-05)               7.7e-05 / 3.9e-05
  (plain a / b: set by the 1 x 1 image -- var = 0, alpha = 1 / sqrt(eps), y cancels two terms of |x alpha| ~ 300.)
  Kind d (ratio 30; one case per family, printed, not bounded):
    plain            1.8e-05 / 4.3e-06                          5.1e-04 / 2.0e-04
    up               5.9e-06 / 2.0e-06                          6.3e-03 / 2.2e-03
    down             3.3e-05 / 8.7e-06                          3.6e-04 / 1.3e-04
    col              1.8e-05 / 4.9e-06                          9.8e-05 / 2.5e-05
  The in-network merges beyond the fp16 store's 2^-11 (y metric, worst of rn_post_slab_parts / unet_post_slab_parts): plain 6.6e-06, up 4.8e-07, down 8.3e-07,
  col 8.3e-07.  The re-read kernels: emulation 1.8e-07, bound 1.8e-06, measured 2.2e-07 (kind a) / 1.4e-07 (kind c).
"""
import ctypes as C

import numpy as np
import pytest
import torch

import _norm_stats_ref as R
import innfer_amd.lib as L

pytestmark = pytest.mark.gpu

GUARD = 4096                  # elements of sentinel in front of and behind every buffer a kernel writes
SENT16, SENTF = -3.0, 777.0


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _to_slab(x):
    """[N, C, H, W] (fp16-representable) -> the fp16 blocked-NHWC slab [C / 32, N, H, W, 32]"""
    N, Cc, H, W = x.shape
    return x.half().view(N, Cc // 32, 32, H, W).permute(1, 0, 3, 4, 2).contiguous()


def _from_slab(s):
    G, N, H, W, _ = s.shape
    return s.permute(1, 0, 4, 2, 3).reshape(N, G * 32, H, W)


def _guarded(n, dtype, fill, dev, guard=GUARD):
    buf = torch.full((guard + n + guard,), fill, dtype=dtype, device=dev)
    return buf, buf[guard:guard + n]


def _intact(buf, n, fill, guard=GUARD):
    return bool((buf[:guard] == fill).all().item() and (buf[guard + n:] == fill).all().item())


def _f(t):
    return None if t is None else t.data_ptr()


class _Conv:
    """One case's conv on the device: operands uploaded and packed once, launched with or without the statistics buffer"""

    def __init__(self, dev, c, d):
        self.c, self.dev = c, dev
        wc = np.ascontiguousarray(d.w.numpy(), np.float32)
        if c.family == "plain":
            packed = np.zeros(L.lib.innfer_conv3x3_packed_bytes(c.K, c.C), np.uint8)
            L.check(L.lib.innfer_pack_conv3x3(wc.ctypes.data, c.K, c.C, packed.ctypes.data))
        elif c.family == "up":
            packed = np.zeros(L.lib.innfer_convt2x_packed_bytes(c.K, c.C), np.uint8)
            L.check(L.lib.innfer_pack_convt2x(wc.ctypes.data, c.K, c.C, c.opt, packed.ctypes.data))
        elif c.family == "down":
            packed = np.zeros(L.lib.innfer_conv4x4s2_packed_bytes(c.K, c.C), np.uint8)
            L.check(L.lib.innfer_pack_conv4x4s2(wc.ctypes.data, c.K, c.C, packed.ctypes.data))
        else:
            packed = np.zeros(L.lib.innfer_conv7x1_packed_bytes(c.K, c.C), np.uint8)
            L.check(L.lib.innfer_pack_conv7x1(wc.ctypes.data, c.K, c.C, packed.ctypes.data))
        assert packed.size > 0
        self.packed = torch.from_numpy(packed).to(dev)
        self.packed64 = []                 # K > 64 (reachable only with statistics): the launch without statistics is one launch per 64 output channels
        if c.family == "plain" and c.K > 64:
            for k0 in range(0, c.K, 64):
                p64 = np.zeros(L.lib.innfer_conv3x3_packed_bytes(64, c.C), np.uint8)
                L.check(L.lib.innfer_pack_conv3x3(np.ascontiguousarray(wc[k0:k0 + 64]).ctypes.data, 64, c.C, p64.ctypes.data))
                self.packed64.append(torch.from_numpy(p64).to(dev))
        self.bias = (d.b.repeat(4) if c.family == "up" else d.b).contiguous().to(dev)
        self.slab = _to_slab(d.x).to(dev)
        self.Ho, self.Wo = R.out_hw(c)
        self.HW = self.Ho * self.Wo
        self.g_in = self.slab[0].numel()
        self.g_out = c.N * self.HW * 32
        self.nper = R.records_per_image(c.H, c.W, R.phases(c))
        assert self.nper == L.lib.innfer_conv_stats_records(c.H, c.W, R.phases(c))
        self.need = c.N * self.nper * c.K * 3
        self.pguard = self.nper * c.K * 3 + 1024          # a whole image's records of sentinel behind the buffer (and in front)

    def args(self, out, part=None, floats=0):
        c, a = self.c, L.ConvArgs()
        a.d_in, a.in_group_stride, a.C = self.slab.data_ptr(), self.g_in, c.C
        a.d_packed, a.d_bias = self.packed.data_ptr(), self.bias.data_ptr()
        a.d_out, a.out_group_stride, a.K = out.data_ptr(), self.g_out, c.K
        a.N, a.H, a.W, a.act = c.N, c.H, c.W, 0
        if c.family == "plain":
            a.reflect_pad = c.opt
        elif c.family == "up":
            a.transposed2x = c.opt
        elif c.family == "down":
            a.stride2_k4 = 1
        else:
            a.column7, a.reflect_pad = 1, c.opt
        if part is not None:
            a.d_stats_part, a.stats_part_floats = part.data_ptr(), floats
        return a

    def run(self, stats):
        """-> (output slab [K / 32, N, Ho, Wo, 32] fp16 on the device, records [N, nper, K, 3] float32 on the device or None); sentinels checked"""
        c = self.c
        n_out = (c.K // 32) * self.g_out
        obuf, out = _guarded(n_out, torch.float16, SENT16, self.dev)
        part = pbuf = None
        if stats:
            pbuf, part = _guarded(self.need, torch.float32, SENTF, self.dev, self.pguard)
            part.fill_(float("nan"))
            short = self.args(out, part, self.need - 1)
            assert L.lib.innfer_conv3x3_f16(C.byref(short), None) == L.ERR_WORKSPACE
        if not stats and self.packed64:
            for i, p64 in enumerate(self.packed64):
                a = self.args(out)
                a.d_packed, a.d_bias, a.K, a.out_ch_off = p64.data_ptr(), self.bias.data_ptr() + 4 * 64 * i, 64, 64 * i
                L.check(L.lib.innfer_conv3x3_f16(C.byref(a), None))
        else:
            L.check(L.lib.innfer_conv3x3_f16(C.byref(self.args(out, part, self.need)), None))
        torch.cuda.synchronize()
        assert _intact(obuf, n_out, SENT16), "the conv wrote outside its output slab"
        if stats:
            assert _intact(pbuf, self.need, SENTF, self.pguard), "the conv wrote statistics outside N * records * channels * 3 floats"
            part = part.view(c.N, self.nper, c.K, 3)
        return out.view(c.K // 32, c.N, self.Ho, self.Wo, 32), part


def _combine(dev, cv, part, gamma, beta):
    c = cv.c
    abuf, alpha = _guarded(c.N * c.K, torch.float32, SENTF, dev)
    sbuf, shift = _guarded(c.N * c.K, torch.float32, SENTF, dev)
    L.check(L.lib.innfer_norm_combine_parts(part.data_ptr(), cv.nper, cv.HW, R.EPS, _f(gamma), _f(beta), alpha.data_ptr(), shift.data_ptr(), c.K, c.N, None))
    torch.cuda.synchronize()
    assert _intact(abuf, c.N * c.K, SENTF) and _intact(sbuf, c.N * c.K, SENTF)
    return alpha.view(c.N, c.K).cpu().numpy(), shift.view(c.N, c.K).cpu().numpy()


def _posts(dev, cv, out, part, res, aff):
    """The two in-network merges on the conv's slab and records: {name: (fp16 result [N, K, Ho, Wo] on the cpu, act, residual?, affine?)}"""
    c = cv.c
    G, n = c.K // 32, (c.K // 32) * cv.g_out
    got = {}
    for name, relu, with_res, which in (("rn plain", 0, False, 0), ("rn relu+res+affine", 1, True, 1), ("rn res", 0, True, 0), ("rn relu+affine", 1, False, 1)):
        gamma, beta = aff[which]
        dbuf, dst = _guarded(n, torch.float16, SENT16, dev)
        L.check(L.lib.innfer_resnet_post_slab_parts(out.data_ptr(), cv.g_out, c.K, cv.HW, c.N, part.data_ptr(), cv.nper, _f(gamma), _f(beta), relu,
                                                    res.data_ptr() if with_res else None, dst.data_ptr(), None))
        torch.cuda.synchronize()
        assert _intact(dbuf, n, SENT16), name
        got[name] = (_from_slab(dst.view(G, c.N, cv.Ho, cv.Wo, 32)).cpu(), 2 if relu else 0, with_res, which)
    # UNet: one destination (LeakyReLU, affine), then two (ReLU at offset 0; LeakyReLU at channel offset 40 of a wider slab, no affine)
    gamma, beta = aff[1]
    dbuf, dst = _guarded(n, torch.float16, SENT16, dev)
    L.check(L.lib.innfer_unet_post_slab_parts(out.data_ptr(), cv.g_out, c.K, cv.HW, c.N, part.data_ptr(), cv.nper, _f(gamma), _f(beta),
                                              dst.data_ptr(), cv.g_out, 0, 1, None, 0, 0, 0, None))
    torch.cuda.synchronize()
    assert _intact(dbuf, n, SENT16)
    got["unet lrelu+affine"] = (_from_slab(dst.view(G, c.N, cv.Ho, cv.Wo, 32)).cpu(), 1, False, 1)
    dbuf0, dst0 = _guarded(n, torch.float16, SENT16, dev)
    n1 = (G + 2) * cv.g_out
    dbuf1, dst1 = _guarded(n1, torch.float16, SENT16, dev)
    L.check(L.lib.innfer_unet_post_slab_parts(out.data_ptr(), cv.g_out, c.K, cv.HW, c.N, part.data_ptr(), cv.nper, None, None,
                                              dst0.data_ptr(), cv.g_out, 0, 2, dst1.data_ptr(), cv.g_out, 40, 1, None))
    torch.cuda.synchronize()
    assert _intact(dbuf0, n, SENT16) and _intact(dbuf1, n1, SENT16)
    got["unet relu"] = (_from_slab(dst0.view(G, c.N, cv.Ho, cv.Wo, 32)).cpu(), 2, False, 0)
    wide = _from_slab(dst1.view(G + 2, c.N, cv.Ho, cv.Wo, 32)).cpu()
    assert (wide[:, :40] == SENT16).all() and (wide[:, 40 + c.K:] == SENT16).all(), "unet_post_slab_parts wrote outside its channels"
    got["unet lrelu at 40"] = (wide[:, 40:40 + c.K].contiguous(), 1, False, 0)
    return got


def _run_case(dev, c, kind, posts=True):
    """Everything the device computes for (case, kind), as cpu tensors"""
    d = R.data(c, kind)
    cv = _Conv(dev, c, d)
    out0, _ = cv.run(False)
    out1, part = cv.run(True)
    r = {"cv": cv, "slab0": out0.cpu(), "slab": out1.cpu(), "part": part.cpu().numpy()}
    aff = [tuple(None if v is None else torch.from_numpy(v).to(dev) for v in R.affine(c, which)) for which in (0, 1)]
    r["alpha_shift"] = [_combine(dev, cv, part, *aff[which]) for which in (0, 1)]
    if posts:
        res = torch.from_numpy(np.random.default_rng(7).uniform(-2, 2, (c.N, c.K, cv.Ho, cv.Wo)).astype(np.float32)).half()
        r["res"] = res
        r["posts"] = _posts(dev, cv, out1, part, _to_slab(res).to(dev), aff)
    return r


def _same_bits(r0, r1):
    assert torch.equal(r0["slab"], r1["slab"]), "the conv is not deterministic"
    assert np.array_equal(r0["part"].view(np.uint32), r1["part"].view(np.uint32)), "the records are not deterministic"
    for (a0, s0), (a1, s1) in zip(r0["alpha_shift"], r1["alpha_shift"]):
        assert np.array_equal(a0.view(np.uint32), a1.view(np.uint32)) and np.array_equal(s0.view(np.uint32), s1.view(np.uint32)), "combine_parts is not deterministic"
    for name in r0.get("posts", {}):
        assert torch.equal(r0["posts"][name][0].view(torch.int16), r1["posts"][name][0].view(torch.int16)), name + " is not deterministic"


def _check_records(c, kind, r, bound):
    """Assertions 1 .. 3; returns the records' worst error"""
    d = R.data(c, kind)
    ref = R.reference_records(c, kind)
    cv, part = r["cv"], r["part"]
    assert torch.equal(r["slab0"].view(torch.int16), r["slab"].view(torch.int16)), "the statistics changed the conv's result"
    got = _from_slab(r["slab"]).double()
    assert (got - d.y).abs().max().item() <= 2.0 ** -11 * d.y.abs().max().item() + 2e-3, "the conv itself is off"
    assert np.isfinite(part).all(), "records the launch never wrote: %d of %d values" % ((~np.isfinite(part)).sum(), part.size)
    assert np.array_equal(part[..., 0], np.broadcast_to(ref.cnt[None, :, None], part.shape[:3])), "a record's count is not the number of valid pixels of its wave"
    assert (part[..., 0].sum(1) == cv.HW).all()
    empty = ref.cnt == 0
    assert (part[:, empty, :, 0] == 0).all()
    err = R.record_error(part, ref.cnt, ref.mean, ref.M2)
    if bound is not None:
        assert err <= bound, "records: %.3e > %.3e" % (err, bound)
    return err


def _check_y(c, kind, r, bound):
    """Assertion 4; returns combine_parts' worst y error"""
    d = R.data(c, kind)
    xs = R.reference_records(c, kind).xs
    worst = 0.0
    for which in (0, 1):
        a64, s64 = R.alpha_shift64(d.mean, d.var, *R.affine(c, which))
        a, s = r["alpha_shift"][which]
        assert np.isfinite(a).all() and np.isfinite(s).all()
        worst = max(worst, R.y_error(a, s, a64, s64, xs))
    if bound is not None:
        assert worst <= bound and worst <= R.CEILING, "combine_parts: %.3e > %.3e" % (worst, min(bound, R.CEILING))
    return worst


def _check_posts(c, kind, r, bound):
    """Assertion 5; returns the worst excess over the fp16 store's rounding, in the y metric, and what exceeded the bound"""
    why = []
    d = R.data(c, kind)
    x16 = _from_slab(r["slab"]).double().numpy()
    worst = 0.0
    for name, (got, act, with_res, which) in r["posts"].items():
        a64, s64 = R.alpha_shift64(d.mean, d.var, *R.affine(c, which))
        xa = x16 * a64[..., None, None]
        v = xa + s64[..., None, None]
        ref = np.maximum(v, 0.2 * v) if act == 1 else np.maximum(v, 0.0) if act == 2 else v
        if with_res:
            ref = ref + r["res"].double().numpy()
        scale = np.maximum(1.0, np.maximum(np.abs(v), np.abs(xa)))
        diff = np.abs(got.double().numpy() - ref)
        excess = float((np.maximum(diff - 2.0 ** -11 * np.abs(ref) - 2.0 ** -24, 0.0) / scale).max())
        worst = max(worst, excess)
        if excess > min(bound, R.CEILING):
            why.append("%s: %.3e beyond the fp16 rounding > %.3e" % (name, excess, min(bound, R.CEILING)))
    return worst, why


def _judge(c, kind, r):
    """Assertions 1 .. 5 on one run's results (r as _run_case returns them): the geometry asserts, the figures are printed, what exceeds a bound is returned"""
    yb, rb = R.working_bounds(c.family, kind)
    er = _check_records(c, kind, r, None)
    ey = _check_y(c, kind, r, None)
    ep, why = _check_posts(c, kind, r, yb)
    print("MEASURED %s %s %s records %.3e (bound %.3e) y %.3e (bound %.3e) posts %.3e" % (c.family, kind, R.case_id(c), er, rb, ey, yb, ep))
    bad = []
    if er > rb:
        bad.append("%s records: %.3e > %.3e" % (kind, er, rb))
    if ey > min(yb, R.CEILING):
        bad.append("%s combine_parts: %.3e > %.3e" % (kind, ey, min(yb, R.CEILING)))
    return bad + ["%s %s" % (kind, w) for w in why]


@pytest.mark.parametrize("c", R.ALL_CASES, ids=R.case_id)
def test_conv_statistics_and_their_merges_vs_float64(dev, c):
    """Per case and data kind a .. c: (1) the slab written with statistics equals the slab without, bit for bit, and nothing outside the buffers is touched (a buffer
    one float short is INNFER_ERR_WORKSPACE); (2) every record is written (NaN-filled before), counts are the valid pixels of each wave's region and sum to the
    output's pixels, waves outside the image hold count 0; (3) each record's mean and M2 match float64 on its region; (4) combine_parts' y against float64; (5)
    rn_post_slab_parts (with and without relu, residual, gamma / beta) and unet_post_slab_parts (both activations, one and two destinations, a channel offset)
    against float64 act(x16 alpha + shift) [+ res], within the statistics bound plus the fp16 store's 2^-11; (6) a second run gives the same bits."""
    bad = []
    for kind in R.KINDS:
        d = R.data(c, kind)
        if kind == "c" and d.y.shape[2] * d.y.shape[3] > 1:
            assert 6.0 <= d.ratio.min() and d.ratio.max() <= 10.0
        r = _run_case(dev, c, kind)
        bad += _judge(c, kind, r)
        _same_bits(r, _run_case(dev, c, kind))
    assert not bad, "; ".join(bad)


@pytest.mark.parametrize("c", R.D_CASES, ids=R.case_id)
def test_ratio_30_is_characterised(dev, c):
    """Kind d (|mean - bias| / std = 30): the records' geometry holds as everywhere; the errors are printed (module docstring, docs/KERNELS.md 3.1), not bounded."""
    d = R.data(c, "d")
    assert 25.0 <= d.ratio.min() and d.ratio.max() <= 35.0
    r = _run_case(dev, c, "d", posts=False)
    er = _check_records(c, "d", r, None)
    ey = _check_y(c, "d", r, None)
    e = R.emulation_error(c, "d")
    print("MEASURED %s d %s records %.3e (emulation %.3e) y %.3e (emulation %.3e)" % (c.family, R.case_id(c), er, e.rec, ey, e.y))


_HWS = (1, 2, 63, 1023, 1024, 1025, 4097)
_NS, _CS = 2, 40


def _two_pass_bound():
    """One bound for both data kinds (a two-pass variance pays nothing for a large mean): 8 x the float32 emulation's worst y error over every HW and kind"""
    worst = 0.0
    for HW in _HWS:
        for kind in "ac":
            x = R.plane_data(_NS, _CS, HW, kind, 9000 + HW)
            mean, var = x.mean(2), x.var(2)
            mu, m2 = R.emulate_two_pass(x)
            for which in (0, 1):
                g, b = (None, None) if not which else R.affine(R.Case("plain", 1, 32, _CS, 1, 1, 0), 1)
                worst = max(worst, R.y_error(*R.alpha_shift32(mu, m2, HW, g, b), *R.alpha_shift64(mean, var, g, b), R.probes(x)))
    return R.MARGIN * worst


@pytest.mark.parametrize("HW", _HWS)
def test_reread_statistics_vs_float64(dev, HW):
    """innfer_norm_stats in both forms -- fp32 [N][HW][64] with 40 channels (stats_kernel<false>) and a two-group fp16 slab with junk beyond channel 40
    (stats_slab8_kernel), several segments through combine_kernel from HW = 1025 -- kinds a and c under ONE bound, with and without gamma / beta; scratch and
    outputs keep their sentinels, a second run gives the same bits."""
    bound = _two_pass_bound()
    assert bound <= R.CEILING
    N, Cc, cpad = _NS, _CS, 64
    nseg = (HW + 1023) // 1024
    for kind in "ac":
        x = R.plane_data(N, Cc, HW, kind, 9000 + HW)
        if kind == "c" and HW > 1:
            ratio = np.abs(x.mean(2)) / x.std(2)
            assert 6.0 <= ratio.min() and ratio.max() <= 10.0
        xt = torch.from_numpy(x)
        raw = torch.full((N, HW, cpad), float("nan"), dtype=torch.float32)
        raw[:, :, :Cc] = xt.permute(0, 2, 1).float()
        padded = torch.full((N, 64, HW, 1), float("nan"), dtype=torch.float64)
        padded[:, :Cc, :, 0] = xt
        slab = _to_slab(padded)
        raw, slab = raw.to(dev), slab.to(dev)
        mean, var, xs = x.mean(2), x.var(2), R.probes(x)
        for form, src, gs in ((0, raw, 0), (1, slab, N * HW * 32)):
            for which in (0, 1):
                g, b = (None, None) if not which else R.affine(R.Case("plain", 1, 32, Cc, 1, 1, 0), 1)
                gd, bd = (None, None) if not which else (torch.from_numpy(g).to(dev), torch.from_numpy(b).to(dev))
                runs = []
                for _ in range(2):
                    abuf, alpha = _guarded(N * Cc, torch.float32, SENTF, dev)
                    sbuf, shift = _guarded(N * Cc, torch.float32, SENTF, dev)
                    npart = N * Cc * nseg * 2
                    pbuf, part = _guarded(npart, torch.float32, SENTF, dev)
                    if nseg > 1:
                        assert L.lib.innfer_norm_stats(src.data_ptr(), form, gs, cpad, HW, R.EPS, _f(gd), _f(bd), alpha.data_ptr(), shift.data_ptr(), Cc, N,
                                                       part.data_ptr(), npart - 1, None) == L.ERR_WORKSPACE
                    L.check(L.lib.innfer_norm_stats(src.data_ptr(), form, gs, cpad, HW, R.EPS, _f(gd), _f(bd), alpha.data_ptr(), shift.data_ptr(), Cc, N,
                                                    part.data_ptr(), npart, None))
                    torch.cuda.synchronize()
                    assert _intact(abuf, N * Cc, SENTF) and _intact(sbuf, N * Cc, SENTF) and _intact(pbuf, npart, SENTF)
                    runs.append((alpha.view(N, Cc).cpu().numpy(), shift.view(N, Cc).cpu().numpy()))
                (a, s), (a1, s1) = runs
                assert np.array_equal(a.view(np.uint32), a1.view(np.uint32)) and np.array_equal(s.view(np.uint32), s1.view(np.uint32))
                assert np.isfinite(a).all() and np.isfinite(s).all()
                err = R.y_error(a, s, *R.alpha_shift64(mean, var, g, b), xs)
                print("MEASURED reread %s HW %d form %d affine %d y %.3e (bound %.3e)" % (kind, HW, form, which, err, bound))
                assert err <= bound, (kind, HW, form, which, err, bound)
