"""The colour fixes that are not the reference's (`-cf_mode wavelet | adain`): their numpy contract utils.color_fix_np, the command line's flag and the
binding, without a GPU.

The wavelet fix is checked against the literal form of StableSR's wavelet_reconstruction (two decompositions: SR's high band plus the enlarged LR's low
band, 3 x 3 dilated depthwise convolutions with replicate padding), written here in torch, with the LR image enlarged by oracle.colorfix.resize_cubic.
color_fix_np computes ONE decomposition of the difference (the a-trous blur is linear), so the two differ by float32 rounding only: at most 1 code on at
most 1e-3 of the values (measured: at most 3.3e-5 at these three shapes)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from innfer_amd import synth
from innfer_amd.utils import utils as U

MODES = ("wavelet", "adain")


def _quantise(x):
    return np.clip(np.floor(x + np.float32(0.5)), 0, 255).astype(np.uint8)


def _wavelet_blur(x, radius):
    """StableSR's wavelet_blur: the 3 x 3 kernel [1, 2, 1] x [1, 2, 1] / 16 at dilation `radius` on the replicate-padded [1, C, H, W] image."""
    C = x.shape[1]
    k = torch.tensor([[0.0625, 0.125, 0.0625], [0.125, 0.25, 0.125], [0.0625, 0.125, 0.0625]], dtype=x.dtype)[None, None].repeat(C, 1, 1, 1)
    return F.conv2d(F.pad(x, (radius,) * 4, mode="replicate"), k, groups=C, dilation=radius)


def _wavelet_decomposition(x, levels=5):
    high = torch.zeros_like(x)
    for i in range(levels):
        low = _wavelet_blur(x, 2 ** i)
        high = high + (x - low)
        x = low
    return high, x


def _stablesr_wavelet(lr, sr):
    """wavelet_reconstruction(content = SR, style = LR enlarged to SR's size): content's high band + style's low band, in code units."""
    from oracle.colorfix import resize_cubic
    up = resize_cubic(lr.astype(np.float32), (sr.shape[1], sr.shape[0])) if lr.shape != sr.shape else lr.astype(np.float32)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).permute(2, 0, 1)[None]
    high, _ = _wavelet_decomposition(t(sr.astype(np.float32)))
    _, low = _wavelet_decomposition(t(up))
    return _quantise((high + low)[0].permute(1, 2, 0).numpy())


def test_identical_images_are_left_alone():
    for C, shape in ((3, (30, 41)), (1, (7, 5)), (4, (1, 1)), (2, (64, 3))):
        a = synth.image_u8(shape[0], shape[1], C, 3 + C)
        for mode in MODES:
            assert np.array_equal(U.color_fix_np(a, a, mode), a), (mode, C, shape)


@pytest.mark.parametrize("lr_shape,scale", (((25, 37), 4), ((64, 48), 2), ((9, 70), 4)), ids=("100x148", "128x96", "36x280"))
def test_wavelet_is_stablesr_wavelet_reconstruction(lr_shape, scale):
    lr = synth.image_u8(lr_shape[0], lr_shape[1], 3, 21)
    sr = synth.image_u8(lr_shape[0] * scale, lr_shape[1] * scale, 3, 22)
    got, want = U.color_fix_np(lr, sr, "wavelet"), _stablesr_wavelet(lr, sr)
    d = np.abs(got.astype(int) - want.astype(int))
    print(f"wavelet vs the literal form at SR {sr.shape[:2]}: max {d.max()} code, {np.count_nonzero(d) / d.size:.2e} of the values differ")
    assert d.max() <= 1 and np.count_nonzero(d) <= 1e-3 * d.size


def test_cubic_enlargement_is_the_oracles():
    """The enlargement inside the wavelet fix restates cubic_sample of csrc/colorfix.hip; oracle.colorfix.resize_cubic states the same scheme."""
    from oracle.colorfix import resize_cubic
    x = synth.image_u8(20, 24, 3, 5).astype(np.float32)
    for oh, ow in ((80, 96), (50, 70), (21, 25)):
        assert np.array_equal(U._cubic_enlarge_np(x, oh, ow), resize_cubic(x, (ow, oh)))


def _cast_pair():
    """(LR, SR with a colour cast).  The LR image is a gradient plus texture inside 48 .. 200, so that neither the noise nor the cast clips at 0 or 255: a
    clipped value has lost what a fix of the mean would need.  SR = LR nearest-enlarged 4x + noise of up to 12 codes, then gain and offset per channel."""
    h, w, s = 24, 31, 4
    yy, xx = np.mgrid[0:h, 0:w]
    base = np.stack([100 + 2 * xx, 70 + 4 * yy, 170 - 2 * xx - 2 * yy], -1)
    lr = (base + synth.image_u8(h, w, 3, 8).astype(int) % 40 - 12).astype(np.uint8)
    noise = synth.image_u8(h * s, w * s, 3, 9).astype(int) % 25 - 12
    sr = np.repeat(np.repeat(lr, s, 0), s, 1).astype(int) + noise
    gain, offset = np.array([0.9, 1.0, 1.1]), np.array([10, -6, 4])
    cast = np.floor(sr * gain + offset + 0.5)
    assert lr.min() >= 48 and lr.max() <= 200 and cast.min() >= 0 and cast.max() <= 255
    return lr, cast.astype(np.uint8)


def test_a_colour_cast_is_removed():
    lr, cast = _cast_pair()
    assert np.abs(cast.mean((0, 1)) - lr.mean((0, 1))).min() > 3                    # every channel is off before the fix
    for mode in MODES:
        fixed = U.color_fix_np(lr, cast, mode)
        off = np.abs(fixed.mean((0, 1)) - lr.mean((0, 1)))
        print(f"{mode}: channel means off by {off} after the fix")
        assert fixed.shape == cast.shape and fixed.dtype == np.uint8 and off.max() <= 1.0, (mode, off)
    fixed = U.color_fix_np(lr, cast, "adain")
    off = np.abs(fixed.reshape(-1, 3).std(0, ddof=1) - lr.reshape(-1, 3).std(0, ddof=1))
    print(f"adain: channel standard deviations off by {off} after the fix")
    assert off.max() <= 1.0, off


def test_channels_are_independent():
    lr, cast = _cast_pair()
    for mode in MODES:
        whole = U.color_fix_np(lr, cast, mode)
        for c in range(3):
            assert np.array_equal(U.color_fix_np(lr[:, :, c:c + 1], cast[:, :, c:c + 1], mode)[:, :, 0], whole[:, :, c]), (mode, c)


def test_refusals():
    a, b = synth.image_u8(8, 8, 3, 1), synth.image_u8(16, 16, 3, 2)
    with pytest.raises(ValueError, match="mode"):
        U.color_fix_np(a, b, "histogram")
    with pytest.raises(ValueError, match="mode"):
        U.color_fix_np(a, b, "lowfreq")                                              # the reference's fix is utils.color_fix itself: not restated
    with pytest.raises(ValueError, match="mode"):
        U.color_fix(a, b, mode="histogram")                                         # refused before anything touches the GPU
    for mode in MODES:
        with pytest.raises(ValueError, match="cannot be subtracted"):
            U.color_fix_np(b, a, mode)                                               # LR larger than SR
        with pytest.raises(ValueError, match="cannot be subtracted"):
            U.color_fix_np(a, synth.image_u8(16, 8, 3, 2), mode)                     # enlarged along one axis only
        with pytest.raises(ValueError, match="channel"):
            U.color_fix_np(a, synth.image_u8(16, 16, 4, 2), mode)
        with pytest.raises(TypeError):
            U.color_fix_np(a.astype(np.uint16), b, mode)


def test_parser():
    from innfer_amd import run as R
    p = R.build_parser()
    ns = p.parse_args(["-m", "x"])
    assert not hasattr(ns, "cf_mode") and ns.cf is False
    assert not hasattr(p.parse_args(["-m", "x", "-cf"]), "cf_mode")
    for mode in ("lowfreq", "wavelet", "adain"):
        assert p.parse_args(["-m", "x", "-cf_mode", mode]).cf_mode == mode
    action = next(a for a in p._actions if a.dest == "cf_mode")
    assert tuple(action.choices) == ("lowfreq", "wavelet", "adain") == R.CF_MODE_CHOICES == U.COLOR_FIX_MODES
    with pytest.raises(SystemExit):
        p.parse_args(["-m", "x", "-cf_mode", "histogram"])


def test_binding():
    from innfer_amd import lib as L
    assert L.COLOR_FIX_MODES == {"lowfreq": 0, "wavelet": 1, "adain": 2}
    for name in ("innfer_color_fix_mode_workspace_bytes", "innfer_color_fix_mode"):
        assert name in L.SIGNATURES and getattr(L.lib, name).argtypes is not None
    assert L.lib.innfer_version() == 124
    # the workspace of the new modes does not grow with the images; mode 0 is innfer_color_fix's
    for mode in (1, 2):
        assert L.lib.innfer_color_fix_mode_workspace_bytes(mode, 8, 8, 32, 32, 3) == L.lib.innfer_color_fix_mode_workspace_bytes(mode, 1080, 1920, 4320, 7680, 3) < 1024
    assert L.lib.innfer_color_fix_mode_workspace_bytes(0, 8, 9, 32, 36, 3) == L.lib.innfer_color_fix_workspace_bytes(8, 9, 32, 36, 3)
    # refused before anything is launched (no device is touched: these pass without a GPU)
    for args, match in (((7, 1, 8, 8, 1, 32, 32, 3, 1, None, 0), "mode"), ((1, None, 8, 8, 1, 32, 32, 3, 1, None, 0), "null"),
                        ((1, 1, 32, 32, 1, 8, 8, 3, 1, None, 0), "cannot be subtracted"), ((2, 1, 8, 8, 1, 32, 32, 5, 1, None, 0), "bad shape"),
                        ((2, 1, 8, 8, 1, 32, 32, 3, 1, 8, 16), "workspace"), ((2, 1, 8, 8, 1, 32, 32, 3, 1, None, 0), "workspace")):
        with pytest.raises(L.InnferError if match == "workspace" else ValueError, match=match):
            L.check(L.lib.innfer_color_fix_mode(*args, None))
