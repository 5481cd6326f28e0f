"""The self-ensemble (`-tta`), the part that needs no GPU: the orientation index map of the library against np.transpose / np.flip, utils.dihedral and its
inverse, the numpy statement of the definition (utils.tta_np), the `-tta` flag and the refusal of a CPU device."""
import inspect

import numpy as np
import pytest
import torch

import innfer_amd.lib as L
from innfer_amd import run as R, synth
from innfer_amd.utils import utils as U


def _t(a, k):
    """t_k written out: transpose if k & 4, then flip the columns if k & 1, then flip the rows if k & 2."""
    if k & 4:
        a = np.transpose(a, (1, 0) + tuple(range(2, a.ndim)))
    if k & 1:
        a = np.flip(a, 1)
    if k & 2:
        a = np.flip(a, 0)
    return a


@pytest.mark.parametrize("k", range(8))
def test_dihedral_index_is_transpose_and_flip(k):
    """innfer_dihedral_index (the map the kernels turn coordinates with) against np.transpose / np.flip of an image whose pixels are their own index."""
    for (H, W) in ((1, 1), (1, 5), (3, 4), (7, 7)):
        idx = np.arange(H * W).reshape(H, W)
        want = _t(idx, k)
        assert want.shape == ((W, H) if k & 4 else (H, W))
        for y in range(want.shape[0]):
            for x in range(want.shape[1]):
                sy, sx = L.dihedral_index(k, H, W, y, x)
                assert 0 <= sy < H and 0 <= sx < W and idx[sy, sx] == want[y, x], (k, H, W, y, x)


def test_dihedral_index_errors():
    with pytest.raises(ValueError, match="k=8"):
        L.dihedral_index(8, 3, 4, 0, 0)
    with pytest.raises(ValueError):
        L.dihedral_index(-1, 3, 4, 0, 0)
    assert L.dihedral_index(4, 3, 4, 3, 2) == (2, 3)                    # the oriented image is 4 x 3
    with pytest.raises(ValueError, match="outside"):
        L.dihedral_index(4, 3, 4, 2, 3)                                 # a pixel of the 3 x 4 image, not of its transpose
    with pytest.raises(ValueError, match="outside"):
        L.dihedral_index(0, 3, 4, 3, 0)
    with pytest.raises(ValueError, match="outside"):
        L.dihedral_index(1, 3, 4, 0, -1)


@pytest.mark.parametrize("k", range(8))
def test_dihedral_and_its_inverse(k):
    """utils.dihedral is t_k and dihedral_inv undoes it: numpy HW and HWC images, torch NCHW (and HW) tensors on the CPU; the results are contiguous."""
    for a in (synth.image_u8(5, 7, 1, 1)[:, :, 0], synth.image_u8(5, 7, 3, 2), synth.image_u8(6, 6, 4, 3).view(np.uint16)):
        b = U.dihedral(a, k)
        assert b.flags["C_CONTIGUOUS"] and b.dtype == a.dtype and np.array_equal(b, _t(a, k)), (k, a.shape)
        assert np.array_equal(U.dihedral_inv(b, k), a), (k, a.shape)
    x = torch.from_numpy(synth.uniform((2, 3, 5, 7), 4))
    y = U.dihedral(x, k)
    assert y.is_contiguous() and y.shape == ((2, 3, 7, 5) if k & 4 else (2, 3, 5, 7))
    for n in range(2):
        for c in range(3):
            assert np.array_equal(y[n, c].numpy(), _t(x[n, c].numpy(), k)), (k, n, c)
    assert torch.equal(U.dihedral_inv(y, k), x)
    assert torch.equal(U.dihedral_inv(U.dihedral(x[0, 0], k), k), x[0, 0])
    with pytest.raises(ValueError, match="0 .. 7"):
        U.dihedral(x, 8)
    with pytest.raises(TypeError):
        U.dihedral(np.zeros((2, 2, 2, 2)), 0)


def test_tta_np_of_an_equivariant_function_is_the_function():
    """fn commutes with every orientation: the eight terms are equal, their float32 sum is 8 fn and the mean is fn(img) exactly -- for uint8 and for
    float16 values, whose partial sums 2 x .. 8 x fit float32's mantissa (a float32 image's 3 x does not)."""
    fn = lambda a: a * 2
    for img in (synth.image_u8(5, 7, 3, 5), synth.uniform((6, 9), 6).astype(np.float16)):
        got = U.tta_np(fn, img)
        assert got.dtype == img.dtype and got.shape == img.shape and np.array_equal(got, fn(img))


def test_tta_np_is_the_sequential_mean_of_eight_orientations():
    """A function that does not commute (a horizontal roll): tta_np equals the loop written out -- float32, k = 0 .. 7 in order, times 0.125."""
    fn = lambda a: np.roll(a, 2, axis=1)
    img = synth.uniform((5, 7, 3), 7)
    acc = np.zeros(img.shape, np.float32)
    for k in range(8):
        term = fn(_t(img, k))
        if k & 2:
            term = np.flip(term, 0)
        if k & 1:
            term = np.flip(term, 1)
        if k & 4:
            term = np.transpose(term, (1, 0, 2))
        acc = acc + term.astype(np.float32)
    want = (acc * np.float32(0.125)).astype(img.dtype)
    got = U.tta_np(fn, img)
    assert np.array_equal(got, want)
    assert not np.array_equal(got, fn(img))                                         # the ensemble is not the single run


def test_flag_parses_and_is_absent_by_default():
    p = R.build_parser()
    argv = ["-m", "4x_model.pth", "-i", "in", "-o", "out", "-cf"]
    plain = p.parse_args(argv)
    assert not hasattr(plain, "tta")
    assert vars(plain) == dict(models="4x_model.pth", arch="infer", input="in", output="out", scale="-1", cf=True, comp=False, no_gpu=True,
                               no_fp16=True, norm=False)                            # the namespace of the reference's flags, as before
    ns = p.parse_args(argv + ["-tta"])
    assert ns.tta is True
    d = vars(ns)
    del d["tta"]
    assert d == vars(plain)
    ns = p.parse_args(["-m", "x", "-tta", "-seamless", "tile", "-fit_channels", "-outscale", "1.5"])
    assert (ns.tta, ns.seamless, ns.fit_channels, ns.outscale) == (True, "tile", True, 1.5)
    with pytest.raises(SystemExit):
        p.parse_args(argv + ["-tta", "8"])                                          # a switch: it takes no value


def test_signatures_and_cpu_refusal():
    assert inspect.signature(R.Model.run_u8).parameters["tta"].default is False
    assert list(inspect.signature(R.Model.forward_tta).parameters) == ["self", "data"]
    assert L.ABI_VERSION >= 119 and all(hasattr(L.lib, f) for f in ("innfer_dihedral_index", "innfer_extract_tiles_u8_tta", "innfer_recompose_u8_tta"))
    with pytest.raises(RuntimeError, match="cuda"):
        R.Model("nowhere.pth", arch="infer", device="cpu")
