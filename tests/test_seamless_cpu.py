"""Seamless modes, the part that needs no GPU: the border index map of the library against np.pad, the numpy statement of the contract, the
`-seamless` flag of the command line and the refusals that are made before anything touches the GPU."""
import inspect

import numpy as np
import pytest

import innfer_amd.lib as L
from innfer_amd import run as R, synth
from innfer_amd.utils import utils as U
from innfer_amd.utils.defaults import SEAMLESS_PAD

NP_MODE = {"tile": "wrap", "mirror": "reflect", "replicate": "edge"}


@pytest.mark.parametrize("mode", sorted(NP_MODE))
def test_border_index_is_np_pad(mode):
    """innfer_border_index (the function the kernels index with) against np.pad of arange(n): n = 1 .. 39, pad 16 (less than, equal to and more than
    n: several folds) and 33."""
    for n in range(1, 40):
        if mode == "mirror" and n < 2:
            continue
        for pad in (16, 33):
            got = [L.border_index(i, n, mode) for i in range(-pad, n + pad)]
            assert got == list(np.pad(np.arange(n), pad, mode=NP_MODE[mode])), (mode, n, pad)


def test_border_index_alpha_pad_and_errors():
    for n in (1, 5, 39):
        got = [L.border_index(i, n, "alpha_pad") for i in range(-16, n + 16)]
        assert got == [-1] * 16 + list(range(n)) + [-1] * 16, n
    assert L.lib.innfer_border_index(0, 1, L.BORDER_MODES["mirror"]) < -1          # a negative error, not the alpha_pad marker
    with pytest.raises(ValueError, match="mirror"):
        L.border_index(0, 1, "mirror")
    with pytest.raises(ValueError):
        L.border_index(0, 0, "tile")
    with pytest.raises(ValueError):
        L.border_index(0, 4, 7)


def test_seamless_pad_np_states_the_contract():
    assert SEAMLESS_PAD == 16 and U.SEAMLESS_MODES == ("tile", "mirror", "replicate", "alpha_pad") == R.SEAMLESS_CHOICES
    for shape in ((5, 7, 4), (37, 52, 3), (9, 6)):
        img = synth.image_u8(shape[0], shape[1], shape[2] if len(shape) == 3 else 1, 3)
        img = img if len(shape) == 3 else img[:, :, 0]
        width = ((16, 16), (16, 16)) + ((0, 0),) * (img.ndim - 2)
        for mode, npm in NP_MODE.items():
            got = U.seamless_pad_np(img, mode)
            assert got.dtype == img.dtype and np.array_equal(got, np.pad(img, width, mode=npm)), (shape, mode)
        got = U.seamless_pad_np(img, "alpha_pad")
        assert got.shape[:2] == (shape[0] + 32, shape[1] + 32) and np.array_equal(got[16:-16, 16:-16], img), shape
        outside = got.copy()
        outside[16:-16, 16:-16] = 0
        assert not outside.any(), shape                                             # every channel, alpha included, is 0 outside the image
    img16 = synth.image_u8(6, 8, 4, 4).view(np.uint16)
    assert np.array_equal(U.seamless_pad_np(img16, "tile"), np.pad(img16, ((16, 16), (16, 16), (0, 0)), mode="wrap"))
    assert np.array_equal(U.seamless_crop(U.seamless_pad_np(img16, "mirror"), 1), img16)
    with pytest.raises(ValueError, match="mode"):
        U.seamless_pad_np(img16, "wrap")


def test_mirror_refuses_a_one_pixel_side():
    """'mirror' has period 2 (n - 1): a side of one pixel is refused with ValueError -- by the numpy statement, and by the GPU route before it
    uploads anything."""
    for img in (synth.image_u8(12, 1, 3, 5), synth.image_u8(1, 12, 3, 6)):
        with pytest.raises(ValueError, match="mirror"):
            U.seamless_pad_np(img, "mirror")
        with pytest.raises(ValueError, match="mirror"):
            U.seamless_pad(img, "mirror")
        with pytest.raises(ValueError, match="mirror"):
            U.seamless_mode("mirror", *img.shape[:2])
        assert U.seamless_pad_np(img, "tile").shape == (img.shape[0] + 32, img.shape[1] + 32, 3)


def test_flag_parses_and_is_absent_by_default():
    p = R.build_parser()
    argv = ["-m", "4x_model.pth", "-i", "in", "-o", "out", "-cf"]
    plain = p.parse_args(argv)
    assert not hasattr(plain, "seamless")
    assert vars(plain) == dict(models="4x_model.pth", arch="infer", input="in", output="out", scale="-1", cf=True, comp=False, no_gpu=True,
                               no_fp16=True, norm=False)                            # the namespace the reference's flags gave before this one existed
    for mode in R.SEAMLESS_CHOICES:
        ns = p.parse_args(argv + ["-seamless", mode])
        assert ns.seamless == mode
        d = vars(ns)
        del d["seamless"]
        assert d == vars(plain)
    with pytest.raises(SystemExit):
        p.parse_args(argv + ["-seamless", "wrap"])
    with pytest.raises(SystemExit):
        p.parse_args(argv + ["-seamless"])


def test_run_u8_signature_and_sharded_chop():
    assert inspect.signature(R.Model.run_u8).parameters["seamless"].default is None
    from innfer_amd import parallel
    with pytest.raises(NotImplementedError, match="seamless"):
        parallel.ChopRunner(lambda t: t, 2, seamless="tile")
    with pytest.raises(NotImplementedError, match="seamless"):
        parallel.run_chain([], None, seamless="tile")
