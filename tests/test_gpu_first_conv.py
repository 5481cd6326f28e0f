"""The first conv of the SR engine (csrc/conv_first.hip: first_conv_mfma / first_conv_mfma_prelu, 24 instantiations) and the slab passes of csrc/net.hip
(slab_upsample_nearest, slab_pixel_shuffle, slab_input_map, slab_input_map_split), launch by launch, against float64 (needs an MI355X: `pytest -m gpu`).

Each is reached through its single-launch entry point (innfer_first_conv, innfer_slab_*), which calls the launcher the networks call: grid, block, instantiation
and argument order are the network's.  References, case lists, comparators and where every bound comes from: tests/_first_conv_ref.py (checked on the CPU by
tests/test_first_conv_cpu.py, which also plants the faults these comparators must reject at cases of this list).

Every output slab is sentinel-filled between sentinel guards, its 32-channel groups a gap apart (group stride > N H W 32) and, for a split output, its lo twin
another gap behind: guards and gaps must keep the sentinel, everything else must lose it.  Every input sits between NaN guards (uint8: 255).

Largest e = max(e32, e_split) of the family's cases; worst err / bound over every element of every case on the MI355X:
    family                                                                   largest e    worst err / bound
    first_conv_mfma<NT, 1, *> fp16 store (in_nc 1, 3)                        7.5e-7       0.996
    first_conv_mfma<NT, 2, *> fp16 store (in_nc 4, 7)                        1.5e-6       0.993
    first_conv_mfma<NT, 3, *> fp16 store (in_nc 8)                           1.7e-6       0.992
    first_conv_mfma, split pair, kind A                                      1.6e-6       0.202
    first_conv_mfma, split pair, kind B (all low parts subnormal)            4.9e-8       0.157
    first_conv_mfma_prelu (act 8), fp16 store                                1.6e-6       0.997
    uint8 input, values (kind U)                                             8.6e-7       0.995
    uint8 input against the planar launch on np2tensor's tensor              exact        bit-identical
    slab_input_map                                                           derived      0.999
    slab_input_map_split                                                     derived      0.373
    slab_upsample_nearest, slab_pixel_shuffle (and their lo-twin launches)   exact        bit-identical
(the fp16 stores sit at 1.0 because the storage rounding alone fills the bound, as in tests/test_gpu_conv_forms.py; the pairs use a fifth of theirs at kind B as
at kind A: the unscaled subnormal low parts reach the MFMA intact)
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _first_conv_ref as R
import innfer_amd.lib as L

pytestmark = pytest.mark.gpu

GUARD = 4096
SENT16 = 1234.0
F16, F32, U8 = 0, 1, 2
f16, f32, f64 = np.float16, np.float32, np.float64


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _guarded(n, dtype, fill, dev):
    buf = torch.full((GUARD + n + GUARD,), fill, dtype=dtype, device=dev)
    return buf, buf[GUARD:GUARD + n]


def _input(t, dev):
    """A planar input on the device between NaN guards (uint8: 255)"""
    t = torch.as_tensor(t).contiguous()
    _, v = _guarded(t.numel(), t.dtype, 255 if t.dtype == torch.uint8 else float("nan"), dev)
    v.copy_(t.reshape(-1))
    return v


def _place(dev, parts, gs, lo=0):
    """Source slabs on the device: parts = [hi] or [hi, lo twin], each [G, n] fp16 -- group g of twin t at t * lo + g * gs; NaN in the gaps and the guards"""
    G, n = parts[0].shape
    total = (len(parts) - 1) * lo + (G - 1) * gs + n
    host = torch.full((total,), float("nan"), dtype=torch.float16)
    for t, p in enumerate(parts):
        for g in range(G):
            host[t * lo + g * gs:t * lo + g * gs + n] = p[g]
    _, v = _guarded(total, torch.float16, float("nan"), dev)
    v.copy_(host)
    return v


class _Out:
    """A destination: G groups of n elements, gs apart; twins = 2: the lo twin `lo` behind.  Sentinel-filled between sentinel guards."""

    def __init__(self, dev, G, n, gap, twins=1, lo_gap=0):
        self.G, self.n, self.gs, self.twins = G, n, n + gap, twins
        one = (G - 1) * self.gs + n
        self.lo = one + lo_gap if twins == 2 else 0
        self.total = self.lo + one
        self.buf, self.v = _guarded(self.total, torch.float16, SENT16, dev)

    @property
    def ptr(self):
        return self.v.data_ptr()

    def read(self):
        """-> the twins' [G, n] cpu tensors; guards and gaps intact, nothing inside left unwritten"""
        assert bool((self.buf[:GUARD] == SENT16).all().item() and (self.buf[GUARD + self.total:] == SENT16).all().item()), "wrote outside the slab"
        t = self.v.cpu()
        gap = torch.ones(self.total, dtype=torch.bool)
        out = []
        for tw in range(self.twins):
            idx = (tw * self.lo + torch.arange(self.G)[:, None] * self.gs + torch.arange(self.n)[None, :])
            gap[idx.reshape(-1)] = False
            out.append(t[idx])
        assert (t[gap] == SENT16).all(), "wrote into the gap between the groups / the twins"
        assert all((o != SENT16).all() for o in out), "left part of its output unwritten"
        return out


def _eq(a, b):
    return torch.equal(R.bits16(a), R.bits16(b))


_REPORT = {}
_LAUNCHED = set()


def _note(family, ratio, e=None):
    w, we = _REPORT.get(family, (0.0, 0.0))
    _REPORT[family] = (max(w, ratio), max(we, e or 0.0))
    return ratio


# ------------------------------------------------------------------------------------------------ the first conv
def _fc(dev, xin, dt, N, Cc, H, W, w, b, K, a, slope, split, with2, normalize=0, fp16_mode=1, image=None):
    """One innfer_first_conv -> ([hi] or [hi, lo] of the slab as [N, K, H, W] cpu fp16, the same of the second slab or None)"""
    n = N * H * W * 32
    o1 = _Out(dev, K // 32, n, 1056, 2 if split else 1, 544)
    o2 = _Out(dev, K // 32, n, 2080, 2 if split else 1, 96) if with2 else None
    ptr = xin.data_ptr() + (0 if image is None else image * (H * W * Cc) * xin.element_size())
    w = np.ascontiguousarray(w, f32)
    b = np.ascontiguousarray(b, f32)
    s = None if slope is None else np.ascontiguousarray(slope, f32)
    L.check(L.lib.innfer_first_conv(ptr, dt, normalize, fp16_mode, N, Cc, H, W, w.ctypes.data, b.ctypes.data, K, a, None if s is None else s.ctypes.data,
                                    o1.ptr, o1.gs, o1.lo, o2.ptr if o2 else None, o2.gs if o2 else 0, o2.lo if o2 else 0, None))
    torch.cuda.synchronize()
    _LAUNCHED.add(R.form(K, Cc, {F16: "f16", F32: "f32", U8: "u8"}[dt], a))

    def nchw(o):
        return None if o is None else [R.from_slab(p.view(K // 32, N, H, W, 32)).contiguous() for p in o.read()]
    return nchw(o1), nchw(o2)


def _store_ratio(got, ref, e):
    g = got.double().numpy()
    return R.worst_ratio(g, ref, R.store_bound(ref, g, e))


def _pair_ratio(hi, lo, ref, e):
    g = R.pair_value(hi.numpy(), lo.numpy())
    return R.worst_ratio(g, ref, R.pair_bound(ref, g, e))


def _family(case, split):
    if case.act == 8:
        return "first_conv_mfma_prelu, fp16 store"
    return "first_conv_mfma, split pair, kind %s" % case.kind if split else "first_conv_mfma, fp16 store, STEPS %d" % R.form(case.K, case.C, "f16", 0)[1]


def _first_case(dev, case, bad):
    K, Cc, H, W, N, kind, a = case
    x32, x16, w, b, slope = R.first_data(case)
    ref16, e16 = R.conv_ref(x16, w, b, a, slope), R.case_e(case, 16)
    ref32, e32 = R.conv_ref(x32, w, b, a, slope), R.case_e(case, 32)
    in16, in16f, in32 = _input(torch.from_numpy(x16).half(), dev), _input(torch.from_numpy(x16), dev), _input(torch.from_numpy(x32), dev)
    split = a != 8

    def run(xin, dt, sp, with2, **kw):
        return _fc(dev, xin, dt, kw.pop("N", N), Cc, H, W, w, b, K, a, slope, sp, with2, **kw)
    # planar fp16 input (FAST16), fp16 stores, both slabs
    (g16,), (g16b,) = run(in16, F16, False, True)
    assert _eq(g16, g16b), (case, "out2 differs from out")
    r = _note(_family(case, False), _store_ratio(g16, ref16, e16), e16)
    print("MEASURED %s f16 input, fp16 store: e %.2e err / bound %.3f" % (case, e16, r))
    if not r <= 1.0:
        bad.append("%s fp16 input: %.3f" % (case, r))
    # the same fp16-representable image as planar fp32 (the three-product form with xl = 0), one slab: the same bits
    (g16f,), _ = run(in16f, F32, False, False)
    assert _eq(g16f, g16), (case, "fp32 input of an fp16-representable image differs from its fp16 input")
    # planar fp32 input that fp16 does not hold: the (hi, lo) pair of the fp32-accurate mode -- or, act 8 (no split output), the fp16 store
    if split:
        (hi, lo), (hi2, lo2) = run(in32, F32, True, True)
        assert _eq(hi, hi2) and _eq(lo, lo2), (case, "out2 pair differs from out")
        r = _note(_family(case, True), _pair_ratio(hi, lo, ref32, e32), e32)
        big = [hi, lo]
    else:
        (g32,), (g32b,) = run(in32, F32, False, True)
        assert _eq(g32, g32b), (case, "out2 differs from out")
        r = _note(_family(case, False), _store_ratio(g32, ref32, e32), e32)
        big = [g32]
    print("MEASURED %s f32 input, %s: e %.2e err / bound %.3f" % (case, "pair" if split else "fp16 store", e32, r))
    if not r <= 1.0:
        bad.append("%s fp32 input: %.3f" % (case, r))
    if N > 1:                       # image i of a batch is the batch-1 launch on image i
        for i in range(N):
            (s16,), _ = run(in16, F16, False, False, N=1, image=i)
            assert _eq(s16, g16[i:i + 1]), (case, "image %d of the fp16 batch differs from its batch-1 launch" % i)
            s32, _ = run(in32, F32, split, False, N=1, image=i)
            assert all(_eq(p, q[i:i + 1]) for p, q in zip(s32, big)), (case, "image %d of the fp32 batch differs from its batch-1 launch" % i)


def test_case_list_launches_all_24_instantiations():
    """From the list and the launch rule (first_conv_launch: K, ceil(9 in_nc / 32), planar fp16 input, act 8) -- every case is launched with both planar kinds"""
    forms = set()
    for case in R.first_cases():
        forms |= {R.form(case.K, case.C, "f16", case.act), R.form(case.K, case.C, "f32", case.act)}
    assert forms == R.ALL_FORMS and len(forms) == 24


@pytest.mark.parametrize("Cc", R.FIRST_C)
@pytest.mark.parametrize("K", R.FIRST_K)
def test_first_conv_vs_float64(dev, K, Cc):
    """Every H x W of the list -- one row, one column, strips whose waves exit whole, a ragged last strip, last row blocks of 1, 2 and 15 rows (both tails of the
    two-row pipeline), three column blocks -- with the four activations under both data kinds, N = 1 and 3"""
    bad = []
    before = set(_LAUNCHED)
    for case in R.first_cases(K, Cc):
        _first_case(dev, case, bad)
    assert not bad, "; ".join(bad[:8])
    want = set().union(*(R.case_forms(c) for c in R.first_cases(K, Cc)))
    assert want <= _LAUNCHED and len(want) == 4, (want, _LAUNCHED - before)


@pytest.mark.parametrize("Cc", (1, 3, 4))
def test_first_conv_uint8_is_the_planar_launch_on_np2tensor(dev, Cc):
    """The uint8 HWC image (BGR -> RGB, BGRA -> RGBA with alpha in place, gray) equals, bit for bit, the planar launch on np2tensor's tensor: fp16 mode = planar
    fp16 input of the rounded tensor, fp16 stores; fp32 mode = planar fp32 input, the (hi, lo) pair"""
    i = 0
    for H, W, N in ((1, 17, 1), (15, 63, 1), (17, 65, 2)):
        img = R.u8_images(N, H, W, Cc)
        din = _input(torch.from_numpy(img), dev)
        for normalize in (0, 1):
            for fp16_mode in (1, 0):
                K, a = R.FIRST_K[i % 2], (R.ACTS if fp16_mode else R.ACTS[:3])[(i // 2) % (4 if fp16_mode else 3)]
                i += 1
                case = R.Case(K, Cc, H, W, N, "A", a)
                _, _, w, b, slope = R.first_data(case)
                t = R.np2tensor_np(img, bool(normalize), bool(fp16_mode))
                split = not fp16_mode
                got, got2 = _fc(dev, din, U8, N, Cc, H, W, w, b, K, a, slope, split, True, normalize, fp16_mode)
                pin = _input(torch.from_numpy(t).half() if fp16_mode else torch.from_numpy(t), dev)
                want, _ = _fc(dev, pin, F16 if fp16_mode else F32, N, Cc, H, W, w, b, K, a, slope, split, False)
                assert all(_eq(p, q) for p, q in zip(got, want)) and all(_eq(p, q) for p, q in zip(got2, want)), (H, W, N, normalize, fp16_mode, K, a)
                ref, e = R.conv_ref(t, w, b, a, slope), R.data_e(t, w, b, a, slope)              # and the values themselves, kind U
                r = _pair_ratio(got[0], got[1], ref, e) if split else _store_ratio(got[0], ref, e)
                assert _note("first conv, uint8 input (kind U)", r, e) <= 1.0, (H, W, N, normalize, fp16_mode, K, a, r)
    _note("first conv, uint8 input vs the planar launch", 0.0)


def test_first_conv_refusals():
    """One launch-free call each: the error code, and a message"""
    n = 0
    for what, rc, want in R.refusals(L):
        assert rc == want and L.last_error(), (what, rc, L.last_error())
        n += 1
    assert n > 30


# ------------------------------------------------------------------------------------------------ the exact passes
def _slab2d(x):
    """[N, C, H, W] fp16 -> [G, n]"""
    s = R.to_slab(x)
    return s.reshape(s.shape[0], -1)


def _twin_out(dev, G, dn, gap, src_extent, twin):
    """The destination of an exact pass and the one lo distance that serves source and destination (as in the network): behind the larger of the two hi slabs"""
    if not twin:
        return _Out(dev, G, dn, gap), 0
    dst_extent = (G - 1) * (dn + gap) + dn
    lo = max(src_extent, dst_extent) + 32
    out = _Out(dev, G, dn, gap, 2, lo - dst_extent)
    assert out.lo == lo
    return out, lo


def _rand16(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)).half()


@pytest.mark.parametrize("f,groups", R.UPSAMPLE_CASES)
def test_slab_upsample_nearest_bit_for_bit(dev, f, groups):
    for H, W in R.SLAB_GRIDS:
        for N in (1, 2):
            for twin in ((False, True) if (H, W, N) == (3, 5, 2) else (False,)):
                xs = [_rand16((N, 32 * groups, H, W), 10 * H + W + N + t) for t in range(2 if twin else 1)]
                n = N * H * W * 32
                sgs, dn = n + 96, n * f * f
                out, lo = _twin_out(dev, groups, dn, 160, (groups - 1) * sgs + n, twin)
                src = _place(dev, [_slab2d(x) for x in xs], sgs, lo)
                L.check(L.lib.innfer_slab_upsample_nearest(src.data_ptr(), sgs, out.ptr, out.gs, groups, N, H, W, f, lo, None))
                torch.cuda.synchronize()
                for x, got in zip(xs, out.read()):
                    want = F.interpolate(x.float(), scale_factor=f, mode="nearest").half()
                    assert _eq(R.from_slab(got.view(groups, N, H * f, W * f, 32)), want), (H, W, N, twin)
    _note("slab_upsample_nearest, slab_pixel_shuffle", 0.0)


@pytest.mark.parametrize("nf,r", R.SHUFFLE_CASES)
def test_slab_pixel_shuffle_bit_for_bit(dev, nf, r):
    gin, gout = nf * r * r // 32, nf // 32
    for H, W in R.SLAB_GRIDS:
        for N in (1, 2):
            for twin in ((False, True) if (H, W, N) == (3, 5, 2) else (False,)):
                xs = [_rand16((N, nf * r * r, H, W), 20 * H + W + N + t) for t in range(2 if twin else 1)]
                n = N * H * W * 32
                sgs, dn = n + 96, n * r * r
                out, lo = _twin_out(dev, gout, dn, 160, (gin - 1) * sgs + n, twin)
                src = _place(dev, [_slab2d(x) for x in xs], sgs, lo)
                L.check(L.lib.innfer_slab_pixel_shuffle(src.data_ptr(), sgs, out.ptr, out.gs, nf, N, H, W, r, lo, None))
                torch.cuda.synchronize()
                for x, got in zip(xs, out.read()):
                    want = F.pixel_shuffle(x.float(), r).half()
                    assert _eq(R.from_slab(got.view(gout, N, H * r, W * r, 32)), want), (H, W, N, twin)
    _note("slab_upsample_nearest, slab_pixel_shuffle", 0.0)


# ------------------------------------------------------------------------------------------------ the input map
def _map_case(dev, Cc, N, H, W, a, split):
    """-> worst err / bound; channels beyond C (their source holds NaN) must be written as zeros"""
    x, al, sh = R.map_data(Cc, N, H, W, a)
    G = -(-Cc // 32)
    n = N * H * W * 32
    a64, s64 = al.astype(f64)[None, :, None, None], sh.astype(f64)[None, :, None, None]

    def slab(v):
        s = R.to_slab(torch.from_numpy(v.astype(f32)), fill=float("nan"))
        return s.reshape(G, -1)
    if split:
        hi, lo = R.to_pair(x)
        lo_d = G * n + 64
        src = _place(dev, [slab(hi), slab(lo)], n, lo_d)
        out = _Out(dev, G, n, 0, 2, lo_d - G * n)
        assert out.lo == lo_d
        xs = R.pair_value(hi, lo)
    else:
        lo_d = 0
        src = _place(dev, [slab(x.astype(f16))], n)
        out = _Out(dev, G, n, 0)
        xs = x.astype(f16).astype(f64)
    L.check(L.lib.innfer_slab_input_map(src.data_ptr(), out.ptr, n, lo_d, Cc, al.ctypes.data, sh.ctypes.data, a, None))
    torch.cuda.synchronize()
    got = [R.from_slab(p.view(G, N, H, W, 32)) for p in out.read()]
    for p in got:
        assert (p[:, Cc:] == 0).all(), "channels beyond C are not zero"
    ref, mag = R.pass_ref(xs, a64, s64, a)
    if split:
        g = R.pair_value(got[0][:, :Cc].numpy(), got[1][:, :Cc].numpy())
        return R.worst_ratio(g, ref, R.map_split_bound(ref, g, mag))
    g = got[0][:, :Cc].double().numpy()
    return R.worst_ratio(g, ref, R.pass_bound(ref, g, mag))


@pytest.mark.parametrize("split", (False, True), ids=("slab_input_map", "slab_input_map_split"))
@pytest.mark.parametrize("Cc", R.MAP_C)
def test_slab_input_map_vs_float64(dev, Cc, split):
    bad = []
    for H, W in R.SLAB_GRIDS:
        for N in (1, 2):
            for a in (0, 1, 2):
                r = _note("slab_input_map_split" if split else "slab_input_map", _map_case(dev, Cc, N, H, W, a, split))
                if not r <= 1.0:
                    bad.append("%d x %d N %d act %d: %.3f" % (H, W, N, a, r))
    print("MEASURED slab_input_map%s C %d: worst err / bound %.3f" % ("_split" if split else "", Cc, _REPORT["slab_input_map_split" if split else "slab_input_map"][0]))
    assert not bad, "; ".join(bad[:8])


# ------------------------------------------------------------------------------------------------ the figures of the table
def test_report(dev):
    """One case per family, not bounded: prints the worst err / bound per kernel family (after the tests above in one session: over every case they ran) -- the
    figures of the module docstring and of docs/KERNELS.md"""
    for K, Cc in ((64, 3), (32, 4), (64, 8)):
        for case in R.first_cases(K, Cc)[3:7]:
            _first_case(dev, case, [])
    for split in (False, True):
        _note("slab_input_map_split" if split else "slab_input_map", _map_case(dev, 40, 2, 7, 11, 1, split))
    for fam, (ratio, e) in sorted(_REPORT.items()):
        print("REPORT %-48s largest e %.2e   worst err / bound %.3f" % (fam, e, ratio))
