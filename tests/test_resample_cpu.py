"""The resampler of `-outscale` without a GPU: the host tables (innfer_resample_taps / innfer_resample_plan) against a float64 restatement of their
definition written here, utils.resample_np against float64 accumulation, both against ATen's and Pillow's antialiased resize, the wrap identity, the
argument checks and the two command-line flags."""
import math

import numpy as np
import pytest
import torch

from innfer_amd import lib as L
from innfer_amd import synth
from innfer_amd.utils import utils as U

FILTERS = ("box", "bilinear", "bicubic", "lanczos")
AXES = ((37, 18), (37, 23), (40, 100), (64, 7), (5, 13), (1, 3), (33, 33), (1400, 3))
SHAPES = (((37, 52), (18, 26)), ((37, 52), (23, 31)), ((40, 64), (100, 96)), ((64, 48), (7, 5)), ((5, 7), (13, 3)), ((1, 1), (3, 3)), ((33, 47), (33, 20)))
SUPPORT = {"box": 0.5, "bilinear": 1.0, "bicubic": 2.0, "lanczos": 3.0}


# ------------------------------------------------------------------------------------------------------------------ the definition, float64
def _sinc(x):
    return 1.0 if x == 0.0 else math.sin(math.pi * x) / (math.pi * x)


def _filter(name, x):
    if name == "box":
        return 1.0 if -0.5 < x <= 0.5 else 0.0
    if name == "bilinear":
        return max(0.0, 1.0 - abs(x))
    if name == "bicubic":                                                   # Keys, a = -0.5
        x = abs(x)
        if x < 1.0:
            return (1.5 * x - 2.5) * x * x + 1.0
        return (((x - 5.0) * x + 8.0) * x - 4.0) * -0.5 if x < 2.0 else 0.0
    return _sinc(x) * _sinc(x / 3.0) if -3.0 <= x < 3.0 else 0.0


def _plan64(n_in, n_out, name, wrap):
    """[(lo, [w_j for j in lo .. hi - 1])] per output, float64, normalised, not rounded."""
    scale = n_in / n_out
    fs = max(scale, 1.0)
    support = SUPPORT[name] * fs
    rows = []
    for i in range(n_out):
        c = (i + 0.5) * scale
        lo, hi = math.floor(c - support + 0.5), math.floor(c + support + 0.5)
        if not wrap:
            lo, hi = max(lo, 0), min(hi, n_in)
        w = np.array([_filter(name, (j - c + 0.5) / fs) for j in range(lo, hi)], np.float64)
        rows.append((lo, w / w.sum()))
    return rows


def _tables64(n_in, n_out, name, wrap):
    """_plan64 in the layout of L.resample_plan, weights float64."""
    rows = _plan64(n_in, n_out, name, wrap)
    T = max(len(w) for _, w in rows)
    weights = np.zeros((n_out, T), np.float64)
    for i, (_, w) in enumerate(rows):
        weights[i, :len(w)] = w
    return np.array([lo for lo, _ in rows], np.int64), np.array([len(w) for _, w in rows], np.int64), weights


def _axis0_64(x, plan, wrap):
    """One pass along axis 0 in float64 with the given tables."""
    start, count, weights = plan
    n = x.shape[0]
    acc = np.zeros((len(start),) + x.shape[1:], np.float64)
    for t in range(weights.shape[1]):
        idx = start.astype(np.int64) + t
        idx = idx % n if wrap else np.clip(idx, 0, n - 1)
        acc += weights[:, t].astype(np.float64).reshape((-1,) + (1,) * (x.ndim - 1)) * x[idx]
    return acc


def _resample64(img, plan_h, plan_v, wrap):
    """Horizontal pass, then vertical, float64, not quantised."""
    x = np.swapaxes(_axis0_64(np.swapaxes(img.astype(np.float64), 0, 1), plan_h, wrap), 0, 1)
    return _axis0_64(x, plan_v, wrap)


def _image(h, w, C, bits, seed):
    img = synth.image_u8(h, w, C * (bits // 8), seed)
    return img if bits == 8 else img.view(np.uint16)


# ------------------------------------------------------------------------------------------------------------------ 1. the plan
@pytest.mark.parametrize("wrap", [0, 1])
@pytest.mark.parametrize("name", FILTERS)
def test_plan_is_the_float64_definition(name, wrap):
    """start and count exactly, every weight within 1e-7 (one float32 ulp near 1, and the host libm's sin), rows summing to 1 within T * 6e-8, and
    innfer_resample_taps == the widest row of either form."""
    for n_in, n_out in AXES:
        T = L.resample_taps(n_in, n_out, name)
        assert T == max(len(w) for _, w in _plan64(n_in, n_out, name, True)), (n_in, n_out)
        assert T >= max(len(w) for _, w in _plan64(n_in, n_out, name, False)), (n_in, n_out)
        start, count, weights = L.resample_plan(n_in, n_out, name, wrap)
        assert weights.shape == (n_out, T) and weights.dtype == np.float32
        rows = _plan64(n_in, n_out, name, wrap)
        assert start.tolist() == [lo for lo, _ in rows], (n_in, n_out)
        assert count.tolist() == [len(w) for _, w in rows], (n_in, n_out)
        for i, (_, w) in enumerate(rows):
            assert np.abs(weights[i, :len(w)].astype(np.float64) - w).max() <= 1e-7, (n_in, n_out, i)
            assert not weights[i, len(w):].any(), (n_in, n_out, i)
        assert np.abs(weights.astype(np.float64).sum(1) - 1.0).max() <= T * 6e-8, (n_in, n_out)
        wide = L.resample_plan(n_in, n_out, name, wrap, T=T + 3)             # a wider table is the same table, zero-padded
        assert np.array_equal(wide[2][:, :T], weights) and not wide[2][:, T:].any()
    if not wrap:
        assert (start >= 0).all() and (start + count <= n_in).all()


# ------------------------------------------------------------------------------------------------------------------ 2. float32 accumulation
@pytest.mark.parametrize("bits", [8, 16])
@pytest.mark.parametrize("name", FILTERS)
def test_resample_np_against_float64_accumulation(name, bits):
    """resample_np (float32, taps in order) against the same tables accumulated in float64: codes differ by at most 1, only where the float64 value
    lies within the forward error bound of the summation order, delta = maxval (T_h + T_v + 2) L_h L_v 2^-24, of a half-integer, and in at most 3 %
    of the codes (a cap: exact ties that float32 weight rounding breaks -- bilinear at 2.5x, box at 64 -> 7 -- are the worst cases)."""
    maxval = 255 if bits == 8 else 65535
    for k, ((h, w), (oh, ow)) in enumerate(SHAPES):
        for wrap in (False, True):
            img = _image(h, w, 3, bits, 100 + k)
            got = U.resample_np(img, oh, ow, name, wrap)
            assert got.shape == (oh, ow, 3) and got.dtype == img.dtype
            ph, pv = L.resample_plan(w, ow, name, wrap), L.resample_plan(h, oh, name, wrap)
            v = _resample64(img, ph, pv, wrap)
            want = np.clip(np.floor(v + 0.5), 0, maxval)
            diff = got.astype(np.int64) != want
            assert np.abs(got.astype(np.int64) - want).max() <= 1, (h, w, oh, ow, wrap)
            L_h, L_v = np.abs(ph[2]).sum(1).max(), np.abs(pv[2]).sum(1).max()
            delta = maxval * (ph[2].shape[1] + pv[2].shape[1] + 2) * L_h * L_v * 2.0 ** -24
            assert (np.abs(v[diff] - np.floor(v[diff]) - 0.5) <= delta).all(), (h, w, oh, ow, wrap)
            assert diff.mean() <= 0.03, (h, w, oh, ow, wrap, diff.mean())
    gray = _image(37, 52, 1, bits, 7)[:, :, 0]                                       # HW in, HW out: the HWC result of one channel
    assert np.array_equal(U.resample_np(gray, 23, 31, name), U.resample_np(gray[:, :, None], 23, 31, name)[:, :, 0])


# ------------------------------------------------------------------------------------------------------------------ 3. second opinions
@pytest.mark.parametrize("bits", [8, 16])
@pytest.mark.parametrize("name", ["bicubic", "bilinear"])
def test_definition_is_aten_antialias(name, bits):
    """The float64 form of the definition == torch.nn.functional.interpolate(antialias=True) in float64, within 1e-9 maxval."""
    import torch.nn.functional as F
    maxval = 255 if bits == 8 else 65535
    for k, ((h, w), (oh, ow)) in enumerate(SHAPES):
        img = _image(h, w, 3, bits, 200 + k)
        mine = _resample64(img, _tables64(w, ow, name, False), _tables64(h, oh, name, False), False)
        x = torch.from_numpy(img.astype(np.float64)).permute(2, 0, 1)[None]
        ref = F.interpolate(x, size=(oh, ow), mode=name, antialias=True, align_corners=False)[0].permute(1, 2, 0).numpy()
        assert np.abs(mine - ref).max() <= 1e-9 * maxval, (h, w, oh, ow, np.abs(mine - ref).max())


def test_definition_is_pillow_lanczos():
    """lanczos against Pillow's mode-F resize (float32 arithmetic): within 2e-4 of an 8-bit code."""
    Image = pytest.importorskip("PIL.Image")
    for k, ((h, w), (oh, ow)) in enumerate(SHAPES):
        img = _image(h, w, 1, 8, 300 + k)[:, :, 0]
        mine = _resample64(img, _tables64(w, ow, "lanczos", False), _tables64(h, oh, "lanczos", False), False)
        ref = np.asarray(Image.fromarray(img.astype(np.float32), mode="F").resize((ow, oh), Image.LANCZOS), np.float64)
        assert np.abs(mine - ref).max() <= 2e-4, (h, w, oh, ow, np.abs(mine - ref).max())


# ------------------------------------------------------------------------------------------------------------------ 4. wrap
@pytest.mark.parametrize("name", FILTERS)
def test_wrap_commutes_with_a_roll(name):
    """At n_in = 2 n_out on both axes every output has the same window relative to its centre: rolling the input by (2, 2) rolls the wrapped result
    by (1, 1), bit for bit -- a tileable texture stays tileable.  The truncated form does not have the property."""
    for bits in (8, 16):
        img = _image(36, 52, 3, bits, 400)
        got = U.resample_np(np.roll(img, (2, 2), (0, 1)), 18, 26, name, wrap=True)
        assert np.array_equal(got, np.roll(U.resample_np(img, 18, 26, name, wrap=True), (1, 1), (0, 1))), bits
    img = _image(36, 52, 3, 8, 400)
    assert not np.array_equal(U.resample_np(np.roll(img, (2, 2), (0, 1)), 18, 26, "lanczos"), np.roll(U.resample_np(img, 18, 26, "lanczos"), (1, 1), (0, 1)))


# ------------------------------------------------------------------------------------------------------------------ 5. refusals, the parser
def test_argument_checks_need_no_gpu():
    """Bad bits, channel counts, sizes, plan widths, null pointers and filters are INNFER_ERR_INVALID before any device call."""
    buf = np.zeros(64, np.int32)
    p = buf.ctypes.data                                                        # a host pointer: a check that let it through would fail loudly

    def call(bits=8, h=4, w=4, C=3, oh=2, ow=2, Th=3, Tv=3, src=p):
        return L.lib.innfer_resample_inthwc(src, bits, h, w, C, p, oh, ow, p, p, p, Th, p, p, p, Tv, 0, None, 0, None)
    for bad in (dict(bits=12), dict(bits=0), dict(C=0), dict(C=5), dict(h=0), dict(w=-1), dict(oh=0), dict(ow=0), dict(Th=0), dict(Tv=-2), dict(src=None)):
        assert call(**bad) == L.ERR_INVALID, bad
        assert "resample_inthwc" in L.last_error()
    assert L.lib.innfer_resample_workspace_bytes(4, 4, 5, 2, 2, 3, 3) == 0
    assert L.lib.innfer_resample_taps(4, 2, 4) == L.ERR_INVALID and L.lib.innfer_resample_taps(0, 2, 3) == L.ERR_INVALID
    s, c, w = np.zeros(2, np.int32), np.zeros(2, np.int32), np.zeros((2, 8), np.float32)
    assert L.lib.innfer_resample_plan(4, 2, -1, 0, s.ctypes.data, c.ctypes.data, w.ctypes.data, 8) == L.ERR_INVALID
    assert L.lib.innfer_resample_plan(4, 0, 3, 0, s.ctypes.data, c.ctypes.data, w.ctypes.data, 8) == L.ERR_INVALID
    assert L.lib.innfer_resample_plan(4, 2, 3, 0, s.ctypes.data, c.ctypes.data, w.ctypes.data, 2) == L.ERR_INVALID        # T below the widest window
    assert L.lib.innfer_resample_plan(4, 2, 3, 0, None, c.ctypes.data, w.ctypes.data, 8) == L.ERR_INVALID
    with pytest.raises(ValueError, match="filter"):
        L.resample_plan(4, 2, "nearest")
    with pytest.raises(ValueError, match="filter"):
        U.resample_np(np.zeros((4, 4, 3), np.uint8), 2, 2, "cubic")
    with pytest.raises(TypeError):
        U.resample_np(np.zeros((4, 4, 3), np.float32), 2, 2)
    assert U.resample_size(1080, 1920, 2.5) == (2700, 4800) and U.resample_size(3, 3, 0.1) == (1, 1) and U.resample_size(7, 9, 0.75) == (5, 6)
    for bad in (0, -1.5, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="scale"):
            U.resample_size(10, 10, bad)


def test_flags_are_absent_unless_given():
    from innfer_amd import run as R
    args = R.build_parser().parse_args(["-m", "x"])
    assert not hasattr(args, "outscale") and not hasattr(args, "outfilter")
    args = R.build_parser().parse_args(["-m", "x", "-outscale", "2.5", "-outfilter", "bicubic"])
    assert args.outscale == 2.5 and args.outfilter == "bicubic"
    with pytest.raises(SystemExit):
        R.build_parser().parse_args(["-m", "x", "-outfilter", "nearest"])
    for bad in ("0", "-2", "nan", "inf"):
        with pytest.raises(ValueError, match="scale"):
            R.main(["-m", "x", "-outscale", bad])
