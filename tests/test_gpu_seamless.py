"""Seamless modes on the GPU: Model.run_u8(seamless=), utils.seamless_pad and `run.py -seamless`.  Every test states one identity: the result is what
the existing pipeline returns for the numpy-padded image (utils.seamless_pad_np), with the padding cut off -- bit for bit, kernel by kernel
(innfer_pad_inthwc, the two tile gathers, the two blends) and end to end.  Only the oracle test has a tolerance.  Needs an MI355X: `pytest -m gpu`."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

MODES = ("tile", "mirror", "replicate", "alpha_pad")
PAD = 16
# image -> (padded size, ps, tiles): smaller than PAD (several folds per row); one tile row; two tile rows; a width that is a multiple of 4 (so are the
# tile origins: the four-pixel loads run, and their fold fallback)
SIZES = {(5, 7): ((37, 39), 37, (1, 2)), (37, 52): ((69, 84), 69, (1, 2)), (210, 236): ((242, 268), 200, (2, 2)), (184, 200): ((216, 232), 200, (2, 2))}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _sd(shapes, seed=0):
    from innfer_amd import synth
    return {k: torch.from_numpy(v) for k, v in synth.fill_state_dict(shapes, seed).items()}


def _model(tmp_path, chop, seed=70, scale=2, name=None):
    from innfer_amd import run as R, synth
    path = str(tmp_path / (name or f"{scale}x_seamless_{seed}.pth"))
    sd = _sd(synth.rrdbnet_shapes(nb=1, scale=scale), seed)
    torch.save(sd, path)
    return R.Model(path, "infer", scale, chop=chop), sd


def _image(h, w, C, seed):
    from innfer_amd import synth
    return synth.image_u8(h, w, C, seed)


# ------------------------------------------------------------------------------------------------------------------ 1. the pad kernel
@pytest.mark.parametrize("bits", [8, 16])
def test_pad_kernel(dev, bits):
    """innfer_pad_inthwc == seamless_pad_np for uint8 and uint16 images of 1, 3 and 4 channels, every mode, sizes from one pixel up; the bytes behind
    the output stay as they were; numpy in -> numpy out, tensor in -> tensor out."""
    from innfer_amd import lib as L
    from innfer_amd.utils import utils as U
    for (h, w) in ((1, 1), (5, 7), (37, 52)):
        for C in (1, 3, 4):
            img = _image(h, w, C * (bits // 8), 10 + C).view(np.uint8 if bits == 8 else np.uint16)
            assert img.shape == (h, w, C)
            for mode in MODES:
                if mode == "mirror" and (h, w) == (1, 1):
                    continue
                want = U.seamless_pad_np(img, mode)
                d = torch.from_numpy(img if bits == 8 else img.view(np.int16)).to(dev)
                nbytes = want.size * (bits // 8)
                buf = torch.full((nbytes + 64,), 0xA5, dtype=torch.uint8, device=dev)
                L.check(L.lib.innfer_pad_inthwc(d.data_ptr(), bits, h, w, C, PAD, L.BORDER_MODES[mode], buf.data_ptr(), _stream()))
                got = buf.cpu().numpy()
                assert np.array_equal(got[:nbytes].view(want.dtype).reshape(want.shape), want), (bits, h, w, C, mode)
                assert (got[nbytes:] == 0xA5).all(), (bits, h, w, C, mode)
                r = U.seamless_pad(img, mode)
                assert isinstance(r, np.ndarray) and r.dtype == img.dtype and np.array_equal(r, want), (bits, h, w, C, mode)
                rd = U.seamless_pad(d, mode)
                assert rd.is_cuda and np.array_equal(rd.cpu().numpy().view(want.dtype), want), (bits, h, w, C, mode)
    img = _image(9, 11, 5, 3)                                                       # any channel count
    assert np.array_equal(U.seamless_pad(img, "mirror"), U.seamless_pad_np(img, "mirror"))
    assert np.array_equal(U.seamless_crop(U.seamless_pad(torch.from_numpy(img).to(dev), "tile"), 1).cpu().numpy(), img)
    with pytest.raises(ValueError, match="mirror"):
        L.check(L.lib.innfer_pad_inthwc(d.data_ptr(), 8, 1, 9, 1, PAD, L.BORDER_MODES["mirror"], buf.data_ptr(), _stream()))


# ------------------------------------------------------------------------------------------------------------------ 2. the gathers
def _gather(d, C, h, w, normalize, dt, begin, count, mode=None, fit=False, alpha=False):
    """Tiles [count (x 2 with alpha), C | 3, ps, ps] of the [h, w, C] device image: the existing gather (mode None) or the seamless one."""
    from innfer_amd import lib as L
    pad = 0 if mode is None else PAD
    ps, ys, xs = L.chop_plan(h + 2 * pad, w + 2 * pad, 200, 0.5)
    tiles = torch.full(((2 if alpha else 1) * count, 3 if fit else C, ps, ps), 7.0, dtype=dt, device=d.device)
    code = L.F16 if dt == torch.float16 else L.F32
    head = (d.data_ptr(), C, h, w, int(normalize), 200, 0.5, begin, count)
    tail = (tiles.data_ptr(), code, _stream())
    if mode is None:
        rc = L.lib.innfer_extract_tiles_u8_fit(*head, int(alpha), *tail) if fit else L.lib.innfer_extract_tiles_u8(*head, *tail)
    elif fit:
        rc = L.lib.innfer_extract_tiles_u8_fit_seamless(*head, int(alpha), PAD, L.BORDER_MODES[mode], *tail)
    else:
        rc = L.lib.innfer_extract_tiles_u8_seamless(*head, PAD, L.BORDER_MODES[mode], *tail)
    L.check(rc)
    return tiles, (ps, len(ys), len(xs))


@pytest.mark.parametrize("fit", [False, True])
@pytest.mark.parametrize("mode", MODES)
def test_gather(dev, mode, fit):
    """The seamless gather on the image == the existing gather on the numpy-padded image, bit for bit: fp16 and fp32 tiles, normalisation off and on,
    1 / 3 / 4 channels (fit: 1 / 2 / 4, alpha tiles off and on), the four lattices of SIZES, all tiles and the sub-range that begins at tile 1 (two
    tiles where the lattice has them)."""
    from innfer_amd.utils import utils as U
    for (h, w), (padded, ps, (nh, nw)) in SIZES.items():
        for C in ((1, 2, 4) if fit else (1, 3, 4)):
            img = _image(h, w, C, 20 + C)
            ref_img = U.seamless_pad_np(img, mode)
            assert ref_img.shape[:2] == padded
            d, d_ref = torch.from_numpy(img).to(dev), torch.from_numpy(ref_img).to(dev)
            for dt in (torch.float16, torch.float32):
                for normalize in (False, True):
                    for alpha in ((False, True) if fit and C > 1 else (False,)):
                        for begin, count in ((0, nh * nw), (1, min(2, nh * nw - 1))):
                            tag = (mode, fit, h, w, C, dt, normalize, alpha, begin, count)
                            got, geo = _gather(d, C, h, w, normalize, dt, begin, count, mode, fit, alpha)
                            want, _ = _gather(d_ref, C, padded[0], padded[1], normalize, dt, begin, count, None, fit, alpha)
                            assert geo == (ps, nh, nw), tag
                            assert torch.equal(got, want), tag


def test_gather_refusals(dev):
    from innfer_amd import lib as L
    d = torch.zeros((1, 8, 3), dtype=torch.uint8, device=dev)
    t = torch.zeros((1, 3, 33, 33), dtype=torch.float16, device=dev)
    with pytest.raises(ValueError, match="mirror"):
        L.check(L.lib.innfer_extract_tiles_u8_seamless(d.data_ptr(), 3, 1, 8, 0, 200, 0.5, 0, 1, PAD, 1, t.data_ptr(), L.F16, _stream()))
    with pytest.raises(ValueError, match="mode"):
        L.check(L.lib.innfer_extract_tiles_u8_seamless(d.data_ptr(), 3, 1, 8, 0, 200, 0.5, 0, 1, PAD, 4, t.data_ptr(), L.F16, _stream()))
    with pytest.raises(ValueError, match="range"):
        L.check(L.lib.innfer_extract_tiles_u8_seamless(d.data_ptr(), 3, 1, 8, 0, 200, 0.5, 1, 2, PAD, 0, t.data_ptr(), L.F16, _stream()))
    with pytest.raises(ValueError, match="channels"):
        L.check(L.lib.innfer_extract_tiles_u8_fit_seamless(d.data_ptr(), 3, 1, 8, 0, 200, 0.5, 0, 1, 0, PAD, 0, t.data_ptr(), L.F16, _stream()))


# ------------------------------------------------------------------------------------------------------------------ 3. the blends
def _blend(tiles, n, C, P, height, width, s, denormalize, crop=None, fit=False, alpha=False, aconst=-1):
    """uint8 [s (height - 2 crop), s (width - 2 crop), C] of the existing blend (crop None) or the seamless one, between two 64-byte sentinels."""
    from innfer_amd import lib as L
    from innfer_amd.utils import utils as U
    c = crop or 0
    shape = (s * (height - 2 * c), s * (width - 2 * c), C)
    nbytes = shape[0] * shape[1] * C
    buf = torch.full((nbytes + 128,), 0xA5, dtype=torch.uint8, device=tiles.device)
    dt = U._dt(tiles)
    head = (tiles.data_ptr(), dt, n) + (() if fit else (C,)) + (P, height, width, 0.5, s, dt, int(denormalize)) + ((C, int(alpha), aconst) if fit else ())
    tail = (buf.data_ptr() + 64, _stream())
    if crop is None:
        rc = (L.lib.innfer_recompose_u8_fit if fit else L.lib.innfer_recompose_u8)(*head, *tail)
    else:
        rc = (L.lib.innfer_recompose_u8_fit_seamless if fit else L.lib.innfer_recompose_u8_seamless)(*head, crop, *tail)
    L.check(rc)
    got = buf.cpu().numpy()
    assert (got[:64] == 0xA5).all() and (got[64 + nbytes:] == 0xA5).all(), "the blend wrote outside its output"
    return got[64:64 + nbytes].reshape(shape)


@pytest.mark.parametrize("fit", [False, True])
@pytest.mark.parametrize("s", [1, 2, 4])
def test_blend(dev, s, fit):
    """innfer_recompose_u8_seamless(crop=16) == innfer_recompose_u8(...)[16 s:-16 s, 16 s:-16 s] of random fp16 / fp32 tiles: padded sizes 37 x 39 (one
    tile row) and 242 x 268 (2 x 2 tiles), 1 / 3 / 4 channels, denormalisation off and on; the fit blend with alpha tiles and with a constant alpha."""
    from innfer_amd import lib as L, synth
    for (height, width) in ((37, 39), (242, 268)):
        ps, ys, xs = L.chop_plan(height, width, 200, 0.5)
        n, P = len(ys) * len(xs), ps * s
        for dt in (torch.float16, torch.float32):
            base = torch.from_numpy(synth.uniform((2 * n, 4, P, P), 30 + s)).to(dev)
            for C in ((1, 2, 4) if fit else (1, 3, 4)):
                for denormalize in (False, True):
                    src = (base * 2.4 - 1.2) if denormalize else (base * 1.2 - 0.1)         # some values beyond the clip on both sides
                    for alpha, aconst in (((True, -1), (False, 77)) if fit and C > 1 else ((False, -1),)):
                        tiles = src[:(2 if alpha else 1) * n, :3 if fit else C].to(dt).contiguous()
                        tag = (s, fit, height, width, dt, C, denormalize, alpha)
                        full = _blend(tiles, n, C, P, height, width, s, denormalize, None, fit, alpha, aconst)
                        got = _blend(tiles, n, C, P, height, width, s, denormalize, PAD, fit, alpha, aconst)
                        assert got.shape == (s * (height - 32), s * (width - 32), C), tag
                        assert np.array_equal(got, full[PAD * s:-PAD * s, PAD * s:-PAD * s]), tag
                        if fit and C > 1 and not alpha:
                            assert (got[:, :, C - 1] == 77).all(), tag


def test_blend_refusals(dev):
    from innfer_amd import lib as L
    t = torch.zeros((2, 3, 37, 37), dtype=torch.float16, device=dev)
    o = torch.zeros((64,), dtype=torch.uint8, device=dev)
    with pytest.raises(ValueError, match="crop"):
        L.check(L.lib.innfer_recompose_u8_seamless(t.data_ptr(), L.F16, 2, 3, 37, 37, 39, 0.5, 1, L.F16, 0, 19, o.data_ptr(), _stream()))
    with pytest.raises(ValueError, match="tiles expected"):
        L.check(L.lib.innfer_recompose_u8_seamless(t.data_ptr(), L.F16, 3, 3, 37, 37, 39, 0.5, 1, L.F16, 0, PAD, o.data_ptr(), _stream()))


# ------------------------------------------------------------------------------------------------------------------ 4. end to end
@pytest.fixture(scope="module")
def models(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("seamless_models")
    return {chop: _model(tmp, chop)[0] for chop in (True, False)}


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("chop", [True, False])
def test_run_u8_is_pad_run_crop(dev, models, chop, mode):
    """run_u8(img, seamless=m) == run_u8(seamless_pad_np(img, m))[32:-32, 32:-32] for BGR images smaller and larger than a tile, fp16 and fp32,
    normalisation off and on, on the fused chop path and on the un-chopped engine path."""
    from innfer_amd.utils import utils as U
    m = models[chop]
    for (h, w, seed) in ((37, 52, 1), (210, 236, 2)):
        img = _image(h, w, 3, seed)
        ref_img = U.seamless_pad_np(img, mode)
        for fp16 in (True, False):
            for normalize in (False, True):
                got = m.run_u8(img, normalize=normalize, fp16=fp16, seamless=mode)
                want = m.run_u8(ref_img, normalize=normalize, fp16=fp16)[32:-32, 32:-32]
                assert isinstance(got, np.ndarray) and got.dtype == np.uint8 and got.shape == (2 * h, 2 * w, 3), (chop, mode, h, w, fp16, normalize)
                assert np.array_equal(got, want), (chop, mode, h, w, fp16, normalize)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("chop", [True, False])
def test_run_u8_fit_channels(dev, models, chop, mode):
    """The same identity with fit_channels=True: BGRA and gray + alpha, with a varying alpha plane, an opaque one and an all-0 one."""
    from innfer_amd.utils import utils as U
    m = models[chop]
    h, w = 37, 52
    for C in (4, 2):
        base = _image(h, w, C, 40 + C)
        for alpha in ("varying", 255, 0):
            img = base.copy()
            if alpha != "varying":
                img[:, :, C - 1] = alpha
            ref_img = U.seamless_pad_np(img, mode)
            for fp16, normalize in ((True, False), (False, True)):
                got = m.run_u8(img, normalize=normalize, fp16=fp16, fit_channels=True, seamless=mode)
                want = m.run_u8(ref_img, normalize=normalize, fp16=fp16, fit_channels=True)[32:-32, 32:-32]
                assert got.shape == (2 * h, 2 * w, C) and np.array_equal(got, want), (chop, mode, C, alpha, fp16, normalize)
                if alpha != "varying" and (mode != "alpha_pad" or alpha == 0):
                    assert (got[:, :, C - 1] == alpha).all(), (chop, mode, C, alpha)
    gray = _image(210, 236, 1, 47)[:, :, 0]                                          # a 2-D image, two tile rows
    got = m.run_u8(gray, fit_channels=True, seamless=mode)
    assert got.shape == (420, 472) and np.array_equal(got, m.run_u8(U.seamless_pad_np(gray, mode), fit_channels=True)[32:-32, 32:-32]), (chop, mode)


class _Counting:
    """Stands in for Model.model: counts the tiles it is given."""

    def __init__(self, net):
        self.net, self.seen = net, 0

    def __call__(self, x):
        self.seen += x.shape[0]
        return self.net(x)


def test_constant_alpha_shortcut(dev, models):
    """A constant alpha plane stays constant under tile / mirror / replicate and is copied (n tiles run); under alpha_pad the padding's alpha is 0, so
    only an all-0 plane is copied and an opaque one runs as 2 n tiles."""
    from innfer_amd import lib as L
    m = models[True]
    h, w = 37, 52
    _, ys, xs = L.chop_plan(h + 32, w + 32, 200, 0.5)
    n = len(ys) * len(xs)
    img = _image(h, w, 4, 50)
    net = m.model
    m.model = _Counting(net)
    try:
        for mode, value, tiles in (("tile", 255, n), ("mirror", 77, n), ("replicate", 0, n), ("alpha_pad", 0, n), ("alpha_pad", 255, 2 * n)):
            img[:, :, 3] = value
            m.model.seen = 0
            got = m.run_u8(img, fit_channels=True, seamless=mode)
            assert m.model.seen == tiles, (mode, value, m.model.seen)
            if tiles == n:
                assert (got[:, :, 3] == value).all(), (mode, value)
    finally:
        m.model = net


@pytest.mark.parametrize("chop", [True, False])
def test_device_images_out_and_default(dev, models, chop):
    """A device tensor in gives a device tensor out, `out=` (the uncropped image's shape x scale) is written and returned, seamless=None is the
    call without the keyword, and refusals are ValueErrors."""
    m = models[chop]
    h, w = 37, 52
    img = _image(h, w, 3, 60)
    want = m.run_u8(img, seamless="tile")
    d = torch.from_numpy(img).to(dev)
    r = m.run_u8(d, seamless="tile")
    assert r.is_cuda and r.is_contiguous() and np.array_equal(r.cpu().numpy(), want)
    out = torch.full((2 * h, 2 * w, 3), 9, dtype=torch.uint8, device=dev)
    r = m.run_u8(d, seamless="tile", out=out)
    assert r.data_ptr() == out.data_ptr() and np.array_equal(out.cpu().numpy(), want)
    bgra = _image(h, w, 4, 61)
    out4 = torch.full((2 * h, 2 * w, 4), 9, dtype=torch.uint8, device=dev)
    r = m.run_u8(torch.from_numpy(bgra).to(dev), fit_channels=True, seamless="mirror", out=out4)
    assert r.data_ptr() == out4.data_ptr() and np.array_equal(out4.cpu().numpy(), m.run_u8(bgra, fit_channels=True, seamless="mirror"))
    assert np.array_equal(m.run_u8(img), m.run_u8(img, seamless=None))
    assert not np.array_equal(m.run_u8(img), want)                                  # the border does change
    with pytest.raises(ValueError, match="mode"):
        m.run_u8(img, seamless="wrap")
    with pytest.raises(ValueError, match="mirror"):
        m.run_u8(_image(9, 1, 3, 62), seamless="mirror")
    with pytest.raises(ValueError, match="out"):
        m.run_u8(d, seamless="tile", out=torch.empty((2 * h + 64, 2 * w + 64, 3), dtype=torch.uint8, device=dev))


# ------------------------------------------------------------------------------------------------------------------ 5. the command line
def test_command_line(dev, tmp_path, monkeypatch):
    """`run.py -seamless tile` with one model, with a chain a>b of two 2x models (crop 64 px) and with -cf: the files written equal the explicit route --
    pad the file with numpy, run the command without the flag, crop (-cf: the colour fix of the unpadded input and the cropped output).  A pix2pix
    `resize` preset refuses the flag."""
    from innfer_amd import run as R, synth
    from innfer_amd.utils import utils as U
    for sub in ("models", "in", "in_pad"):
        (tmp_path / sub).mkdir()
    for name, seed in (("2x_a.pth", 71), ("2x_b.pth", 72)):
        torch.save(_sd(synth.rrdbnet_shapes(nb=1, scale=2), seed), str(tmp_path / "models" / name))
    img = _image(40, 56, 3, 73)
    U.save_img(img, str(tmp_path / "in" / "tex.png"))
    U.save_img(U.seamless_pad_np(img, "tile"), str(tmp_path / "in_pad" / "tex.png"))
    monkeypatch.chdir(tmp_path)
    for tag, chain, total in (("one", "2x_a", 2), ("chain", "2x_a>2x_b", 4)):
        assert R.main(["-m", chain, "-i", "in", "-o", f"out_{tag}", "-seamless", "tile"]) == 0
        assert R.main(["-m", chain, "-i", "in_pad", "-o", f"ref_{tag}"]) == 0
        got = U.read_img(str(tmp_path / f"out_{tag}" / "tex.png"))
        ref = U.seamless_crop(U.read_img(str(tmp_path / f"ref_{tag}" / "tex.png")), total)
        assert got.shape == (40 * total, 56 * total, 3) and ref.shape == got.shape, tag
        assert np.array_equal(got, ref), tag
        assert R.main(["-m", chain, "-i", "in", "-o", f"out_cf_{tag}", "-seamless", "tile", "-cf"]) == 0
        assert np.array_equal(U.read_img(str(tmp_path / f"out_cf_{tag}" / "tex.png")), U.color_fix(img, ref)), tag
    with pytest.raises(ValueError, match="-seamless"):
        R.main(["-m", "2x_a", "-a", "p2p_256", "-i", "in", "-o", "out_p2p", "-seamless", "tile"])


# ------------------------------------------------------------------------------------------------------------------ 6. the oracle
def test_against_the_oracle(dev, tmp_path):
    """fp16 run_u8(seamless='tile') of a 64 x 88 image (padded: 96 x 120) against the oracle's chop_forward of the fp32 RRDBNet on the numpy-padded image,
    cropped: >= 99 % of the uint8 codes within +-1 on every channel."""
    import oracle
    from innfer_amd.utils import utils as U
    m, sd = _model(tmp_path, True, seed=74)
    img = _image(64, 88, 3, 75)
    got = m.run_u8(img, seamless="tile").astype(np.int32)
    f = lambda t: oracle.rrdbnet_forward(sd, t, nb=1, scale=2)
    with torch.no_grad():
        ref = oracle.tensor2np(oracle.chop_forward(f, oracle.np2tensor(U.seamless_pad_np(img, "tile")), 2)).astype(np.int32)[32:-32, 32:-32]
    assert got.shape == ref.shape == (128, 176, 3)
    for c in range(3):
        assert (np.abs(got[:, :, c] - ref[:, :, c]) <= 1).mean() >= 0.99, c
