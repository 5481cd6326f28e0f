"""The self-ensemble on the GPU: innfer_extract_tiles_u8_tta, innfer_recompose_u8_tta, Model.run_u8(tta=True) and `run.py -tta`.  Every comparison is bit
for bit.  The gather is held to the existing gathers on the image turned on the host (utils.dihedral), the blend to the existing tensor blend of each
orientation's slots turned back and averaged in float32, the whole to Model.forward_tta.  Needs an MI355X: `pytest -m gpu`.

Image sizes (the smallest that reach every branch): (5, 7) under a seamless mode only (padded 37 x 39, several folds of the border map per row);
(37, 53): ps 37, the one-pixel path, a 1 x 2 lattice whose clamped last tile becomes 2 x 1 when transposed; (40, 56): ps 40, the four-pixel loads, their
reversal and their fold fallback; (210, 236): ps 200, a 2 x 2 lattice clamped on both axes."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

MODES = ("tile", "mirror", "replicate", "alpha_pad")
PAD = 16
SIZES = ((5, 7), (37, 53), (40, 56), (210, 236))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _image(h, w, C, seed):
    from innfer_amd import synth
    return synth.image_u8(h, w, C, seed)


def _sd(shapes, seed=0):
    from innfer_amd import synth
    return {k: torch.from_numpy(v) for k, v in synth.fill_state_dict(shapes, seed).items()}


def _model(tmp_path, chop, seed=80, scale=2, name=None):
    from innfer_amd import run as R, synth
    path = str(tmp_path / (name or f"{scale}x_tta_{seed}.pth"))
    torch.save(_sd(synth.rrdbnet_shapes(nb=1, scale=scale), seed), path)
    return R.Model(path, "infer", scale, chop=chop)


# ------------------------------------------------------------------------------------------------------------------ 1. the gather
def _gather_ref(d, C, h, w, normalize, dt, mode, fit, alpha, patch=200):
    """All tiles of the [h, w, C] device image by the existing gathers: [n (x 2 with alpha), C | 3, ps, ps]."""
    from innfer_amd import lib as L
    pad = 0 if mode is None else PAD
    ps, ys, xs = L.chop_plan(h + 2 * pad, w + 2 * pad, patch, 0.5)
    n = len(ys) * len(xs)
    tiles = torch.full(((2 if alpha else 1) * n, 3 if fit else C, ps, ps), 7.0, dtype=dt, device=d.device)
    head = (d.data_ptr(), C, h, w, int(normalize), patch, 0.5, 0, n)
    tail = (tiles.data_ptr(), L.F16 if dt == torch.float16 else L.F32, _stream())
    if mode is None:
        rc = L.lib.innfer_extract_tiles_u8_fit(*head, int(alpha), *tail) if fit else L.lib.innfer_extract_tiles_u8(*head, *tail)
    elif fit:
        rc = L.lib.innfer_extract_tiles_u8_fit_seamless(*head, int(alpha), PAD, L.BORDER_MODES[mode], *tail)
    else:
        rc = L.lib.innfer_extract_tiles_u8_seamless(*head, PAD, L.BORDER_MODES[mode], *tail)
    L.check(rc)
    return tiles, n, ps


@pytest.mark.parametrize("fit", [False, True])
@pytest.mark.parametrize("mode", [None] + list(MODES))
def test_gather(dev, mode, fit):
    """Slots [k n, (k + 1) n) (with alpha also [8 n + k n, ..)) of innfer_extract_tiles_u8_tta == the existing gather of utils.dihedral(img, k), for every
    k: fp16 and fp32 tiles, normalisation off and on, 1 / 3 / 4 channels (fit: 1 / 2 / 4, alpha tiles off and on), pad 0 (mode None) and pad 16 in each
    mode.  The buffer is pre-filled and the elements behind the tiles stay as they were."""
    from innfer_amd import lib as L
    from innfer_amd.utils import utils as U
    code = L.BORDER_MODES["replicate" if mode is None else mode]
    for (h, w) in SIZES:
        if mode is None and (h, w) == (5, 7):
            continue
        for C in ((1, 2, 4) if fit else (1, 3, 4)):
            img = _image(h, w, C, 20 + C)
            d = torch.from_numpy(img).to(dev)
            turned = [torch.from_numpy(U.dihedral(img, k)).to(dev) for k in range(8)]
            for dt in (torch.float16, torch.float32):
                for normalize in (False, True):
                    for alpha in ((False, True) if fit and C > 1 else (False,)):
                        tag = (mode, fit, h, w, C, dt, normalize, alpha)
                        refs = [_gather_ref(turned[k], C, turned[k].shape[0], turned[k].shape[1], normalize, dt, mode, fit, alpha) for k in range(8)]
                        n, ps = refs[0][1], refs[0][2]
                        assert all(r[1:] == (n, ps) for r in refs), tag
                        count, Ct = (16 if alpha else 8) * n, 3 if fit else C
                        numel = count * Ct * ps * ps
                        buf = torch.full((numel + 64,), 7.0, dtype=dt, device=dev)
                        L.check(L.lib.innfer_extract_tiles_u8_tta(d.data_ptr(), C, h, w, int(normalize), 200, 0.5, int(fit), int(alpha), 0 if mode is None else PAD, code,
                                                                  buf.data_ptr(), L.F16 if dt == torch.float16 else L.F32, _stream()))
                        got = buf[:numel].view(count, Ct, ps, ps)
                        assert bool((buf[numel:] == 7.0).all()), tag
                        for k in range(8):
                            assert torch.equal(got[k * n:(k + 1) * n], refs[k][0][:n]), tag + (k,)
                            if alpha:
                                assert torch.equal(got[8 * n + k * n:8 * n + (k + 1) * n], refs[k][0][n:]), tag + (k, "alpha")


def test_gather_launch_split(dev):
    """More slots than one launch takes (the grid's y ends at 65535): a 120 x 141 image of 2 channels at patch 2 is a 119 x 140 lattice, n = 16 660, so
    each half of the gather (4 n = 66 640 slots, straight and transposed) is a launch of 65 535 slots and one of 1 105 that starts at slot_begin 65 535;
    the sides differ, so the transposed lattice is 140 x 119.  The plain form and the fit form with alpha tiles, whose slot base is 8 n whatever the
    launch: fp16, every orientation's slots held to the existing gather (one launch of n tiles) of utils.dihedral(img, k), the buffer's tail untouched."""
    from innfer_amd import lib as L
    from innfer_amd.utils import utils as U
    h, w, C, patch = 120, 141, 2, 2
    ps, ys, xs = L.chop_plan(h, w, patch, 0.5)
    n = len(ys) * len(xs)
    assert (ps, len(ys), len(xs)) == (2, 119, 140) and 4 * n == 65535 + 1105
    img = _image(h, w, C, 27)
    d = torch.from_numpy(img).to(dev)
    turned = [torch.from_numpy(U.dihedral(img, k)).to(dev) for k in range(8)]
    for fit, alpha in ((False, False), (True, True)):
        refs = [_gather_ref(t, C, t.shape[0], t.shape[1], False, torch.float16, None, fit, alpha, patch) for t in turned]
        assert all(r[1:] == (n, ps) for r in refs), fit
        count, Ct = (16 if alpha else 8) * n, 3 if fit else C
        numel = count * Ct * ps * ps
        buf = torch.full((numel + 64,), 7.0, dtype=torch.float16, device=dev)
        L.check(L.lib.innfer_extract_tiles_u8_tta(d.data_ptr(), C, h, w, 0, patch, 0.5, int(fit), int(alpha), 0, L.BORDER_MODES["replicate"], buf.data_ptr(), L.F16,
                                                  _stream()))
        got = buf[:numel].view(count, Ct, ps, ps)
        assert bool((buf[numel:] == 7.0).all()), fit
        for k in range(8):
            assert torch.equal(got[k * n:(k + 1) * n], refs[k][0][:n]), (fit, k)
            if alpha:
                assert torch.equal(got[8 * n + k * n:8 * n + (k + 1) * n], refs[k][0][n:]), (fit, k, "alpha")


def test_refusals(dev):
    from innfer_amd import lib as L
    d = torch.zeros((40, 56, 5), dtype=torch.uint8, device=dev)
    t = torch.zeros((16 * 2, 5, 40, 40), dtype=torch.float16, device=dev)
    o = torch.zeros((80 * 112 * 5,), dtype=torch.uint8, device=dev)
    with pytest.raises(NotImplementedError, match="channels"):
        L.check(L.lib.innfer_extract_tiles_u8_tta(d.data_ptr(), 5, 40, 56, 0, 200, 0.5, 0, 0, 0, 2, t.data_ptr(), L.F16, _stream()))
    with pytest.raises(ValueError, match="channels"):
        L.check(L.lib.innfer_extract_tiles_u8_tta(d.data_ptr(), 3, 40, 56, 0, 200, 0.5, 1, 0, 0, 2, t.data_ptr(), L.F16, _stream()))
    with pytest.raises(ValueError, match="mirror"):
        L.check(L.lib.innfer_extract_tiles_u8_tta(d.data_ptr(), 3, 1, 56, 0, 200, 0.5, 0, 0, PAD, 1, t.data_ptr(), L.F16, _stream()))
    with pytest.raises(ValueError, match="mode"):
        L.check(L.lib.innfer_extract_tiles_u8_tta(d.data_ptr(), 3, 40, 56, 0, 200, 0.5, 0, 0, PAD, 4, t.data_ptr(), L.F16, _stream()))
    with pytest.raises(NotImplementedError, match="channels"):
        L.check(L.lib.innfer_recompose_u8_tta(t.data_ptr(), L.F16, 2, 5, 80, 40, 56, 0.5, 2, L.F16, 0, 0, 0, -1, 0, o.data_ptr(), _stream()))
    with pytest.raises(ValueError, match="tiles expected"):
        L.check(L.lib.innfer_recompose_u8_tta(t.data_ptr(), L.F16, 3, 3, 80, 40, 56, 0.5, 2, L.F16, 0, 0, 0, -1, 0, o.data_ptr(), _stream()))
    with pytest.raises(ValueError, match="crop"):
        L.check(L.lib.innfer_recompose_u8_tta(t.data_ptr(), L.F16, 2, 3, 80, 40, 56, 0.5, 2, L.F16, 0, 0, 0, -1, 20, o.data_ptr(), _stream()))
    with pytest.raises(ValueError, match="alpha"):
        L.check(L.lib.innfer_recompose_u8_tta(t.data_ptr(), L.F16, 2, 4, 80, 40, 56, 0.5, 2, L.F16, 0, 1, 0, -1, 0, o.data_ptr(), _stream()))


# ------------------------------------------------------------------------------------------------------------------ 2. the blend
def _blend_tta(tiles, n, C, P, height, width, s, via, denormalize, crop, fit=False, alpha=False, aconst=-1):
    """uint8 [s (height - 2 crop), s (width - 2 crop), C] of innfer_recompose_u8_tta between two 64-byte sentinels."""
    from innfer_amd import lib as L
    from innfer_amd.utils import utils as U
    shape = (s * (height - 2 * crop), s * (width - 2 * crop), C)
    nbytes = shape[0] * shape[1] * C
    buf = torch.full((nbytes + 128,), 0xA5, dtype=torch.uint8, device=tiles.device)
    L.check(L.lib.innfer_recompose_u8_tta(tiles.data_ptr(), U._dt(tiles), n, C, P, height, width, 0.5, s, L.F16 if via == torch.float16 else L.F32, int(denormalize),
                                          int(fit), int(alpha), aconst, crop, buf.data_ptr() + 64, _stream()))
    got = buf.cpu().numpy()
    assert (got[:64] == 0xA5).all() and (got[64 + nbytes:] == 0xA5).all(), "the blend wrote outside its output"
    return got[64:64 + nbytes].reshape(shape)


def _mean_of_blends(tiles, n, height, width, s, via):
    """The composition the blend is held to: utils.recompose_tensor of each orientation's n slots on its own frame (width x height for k >= 4), turned
    back, added as float32 in the order k = 0 .. 7, times 0.125, cast to `via`: [1, C, s height, s width]."""
    from innfer_amd.utils import utils as U
    acc = None
    for k in range(8):
        hk, wk = (width, height) if k & 4 else (height, width)
        y = U.dihedral_inv(U.recompose_tensor(tiles[k * n:(k + 1) * n], hk, wk, step=0.5, scale=s, out_dtype=via), k).float()
        acc = y if acc is None else acc + y
    return (acc * 0.125).to(via)


@pytest.mark.parametrize("dts", [(torch.float16, torch.float16), (torch.float16, torch.float32), (torch.float32, torch.float32)], ids=["h2h", "h2f", "f2f"])
def test_blend(dev, dts):
    """innfer_recompose_u8_tta of random tiles [8 n, C, P, P] == tensor2np of the mean of the eight existing tensor blends, cropped: scale 2, 1 / 3 / 4
    channels, crop 0 and 16, denormalisation off and on, lattices 1 x 1 (37 x 39), 1 x 2 (37 x 53, 40 x 56) and 2 x 2 (210 x 236).  The last orientation
    takes part: corrupting slot 7 n changes the result."""
    from innfer_amd import lib as L, synth
    from innfer_amd.utils import utils as U
    tdt, via = dts
    s = 2
    for (height, width) in ((37, 39), (37, 53), (40, 56), (210, 236)):
        ps, ys, xs = L.chop_plan(height, width, 200, 0.5)
        n, P = len(ys) * len(xs), ps * s
        base = torch.from_numpy(synth.uniform((8 * n, 4, P, P), 31 + height)).to(dev)
        for C in (1, 3, 4):
            for denormalize in (False, True):
                src = (base * 2.4 - 1.2) if denormalize else (base * 1.2 - 0.1)             # some values beyond the clip on both sides
                tiles = src[:, :C].to(tdt).contiguous()
                full = _mean_of_blends(tiles, n, height, width, s, via)
                for crop in (0, PAD):
                    tag = (dts, height, width, C, denormalize, crop)
                    c = s * crop
                    want = U.tensor2np(full[:, :, c:s * height - c, c:s * width - c], denormalize=denormalize)
                    got = _blend_tta(tiles, n, C, P, height, width, s, via, denormalize, crop)
                    assert got.shape == want.shape and np.array_equal(got, want), tag
                tiles[7 * n] = 1.0 - tiles[7 * n]
                assert not np.array_equal(_blend_tta(tiles, n, C, P, height, width, s, via, denormalize, PAD), got), (dts, height, width, C, "slot 7 n")


def test_blend_fit(dev):
    """The fit form: colour tiles [0, 8 n), alpha tiles [8 n, 16 n) -- each plane is averaged over the orientations channel by channel, then mean3 / the
    constant alpha and the quantisation (utils.fit_merge of the two means)."""
    from innfer_amd import lib as L, synth
    from innfer_amd.utils import utils as U
    s, (height, width) = 2, (40, 56)
    ps, ys, xs = L.chop_plan(height, width, 200, 0.5)
    n, P = len(ys) * len(xs), ps * s
    for dt in (torch.float16, torch.float32):
        tiles = (torch.from_numpy(synth.uniform((16 * n, 3, P, P), 41)).to(dev) * 1.2 - 0.1).to(dt).contiguous()
        y, ya = _mean_of_blends(tiles[:8 * n], n, height, width, s, dt), _mean_of_blends(tiles[8 * n:], n, height, width, s, dt)
        for C, alpha, aconst in ((1, False, -1), (2, True, -1), (4, True, -1), (4, False, 77)):
            want = U.fit_merge(y, ya if alpha else None, None if alpha or C == 1 else aconst, C).cpu().numpy()
            for crop in (0, PAD):
                got = _blend_tta(tiles, n, C, P, height, width, s, dt, False, crop, fit=True, alpha=alpha, aconst=aconst)
                c = s * crop
                assert np.array_equal(got, want[c:s * height - c, c:s * width - c]), (dt, C, alpha, crop)


# ------------------------------------------------------------------------------------------------------------------ 3. end to end
@pytest.fixture(scope="module")
def models(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("tta_models")
    return {chop: _model(tmp, chop) for chop in (True, False)}


def _want(m, img, fp16=True, normalize=False):
    """The definition: tensor2np(forward_tta(np2tensor(img)[.half()]))."""
    from innfer_amd.utils import utils as U
    x = U.np2tensor(img, normalize=normalize, dtype=torch.float16 if fp16 else torch.float32)
    return U.tensor2np(m.forward_tta(x), denormalize=normalize)


@pytest.mark.parametrize("case", [(True, (37, 53), True), (True, (40, 56), True), (True, (210, 236), True), (False, (40, 56), True), (True, (40, 56), False)],
                         ids=["chop-37x53", "chop-40x56", "chop-210x236", "whole-40x56", "chop-40x56-fp32"])
def test_run_u8_is_forward_tta(dev, models, case):
    from innfer_amd.utils import utils as U
    chop, (h, w), fp16 = case
    m = models[chop]
    img = _image(h, w, 3, 50 + h)
    for normalize in (False, True):
        got = m.run_u8(img, normalize=normalize, fp16=fp16, tta=True)
        assert isinstance(got, np.ndarray) and got.dtype == np.uint8 and got.shape == (2 * h, 2 * w, 3)
        assert np.array_equal(got, _want(m, img, fp16, normalize)), (case, normalize)


@pytest.mark.parametrize("chop", [True, False])
def test_run_u8_seamless(dev, models, chop):
    """With seamless the definition holds for the padded image, the padding cut off: a 5 x 7 image (smaller than the padding) in every mode, 40 x 56 tiled."""
    from innfer_amd.utils import utils as U
    m = models[chop]
    for (h, w), modes in (((5, 7), MODES), ((40, 56), ("tile",))):
        img = _image(h, w, 3, 60 + h)
        for mode in modes:
            got = m.run_u8(img, seamless=mode, tta=True)
            want = _want(m, U.seamless_pad_np(img, mode))[32:-32, 32:-32]
            assert got.shape == (2 * h, 2 * w, 3) and np.array_equal(got, want), (chop, h, w, mode)


@pytest.mark.parametrize("chop", [True, False])
def test_run_u8_fit_channels_outscale_and_device_input(dev, models, chop):
    """fit_channels on a BGRA image with a varying alpha plane (and seamless on top), a constant alpha, a gray image; outscale; a device tensor in."""
    from innfer_amd.utils import utils as U
    m = models[chop]
    h, w = 40, 56
    bgra = _image(h, w, 4, 71)
    assert len(np.unique(bgra[:, :, 3])) > 1
    want = U.fit_channels_forward(m.forward_tta, bgra, device=dev, dtype=torch.float16)
    got = m.run_u8(bgra, fit_channels=True, tta=True)
    assert got.shape == (2 * h, 2 * w, 4) and np.array_equal(got, want), chop
    got = m.run_u8(bgra, fit_channels=True, seamless="alpha_pad", tta=True)
    want = U.fit_channels_forward(m.forward_tta, U.seamless_pad_np(bgra, "alpha_pad"), device=dev, dtype=torch.float16)[32:-32, 32:-32]
    assert np.array_equal(got, want), chop
    opaque = bgra.copy()
    opaque[:, :, 3] = 255
    got = m.run_u8(opaque, fit_channels=True, tta=True)
    assert (got[:, :, 3] == 255).all() and np.array_equal(got, U.fit_channels_forward(m.forward_tta, opaque, device=dev, dtype=torch.float16)), chop
    gray = _image(37, 53, 1, 72)[:, :, 0]
    assert np.array_equal(m.run_u8(gray, fit_channels=True, tta=True), U.fit_channels_forward(m.forward_tta, gray, device=dev, dtype=torch.float16)), chop
    img = _image(h, w, 3, 73)
    ref = _want(m, img)
    oh, ow = U.resample_size(h, w, 1.5)
    got = m.run_u8(img, outscale=1.5, tta=True)
    assert got.shape == (oh, ow, 3) and np.array_equal(got, U.resample_np(ref, oh, ow, "lanczos")), chop
    d = torch.from_numpy(img).to(dev)
    r = m.run_u8(d, tta=True)
    assert r.is_cuda and r.is_contiguous() and r.dtype == torch.uint8 and np.array_equal(r.cpu().numpy(), ref), chop
    out = torch.full((2 * h, 2 * w, 3), 9, dtype=torch.uint8, device=dev)
    r = m.run_u8(d, tta=True, out=out)
    assert r.data_ptr() == out.data_ptr() and np.array_equal(out.cpu().numpy(), ref), chop


class _Counting:
    """Stands in for Model.model: records the tile count of every call."""

    def __init__(self, net):
        self.net, self.calls = net, []

    def __call__(self, x):
        self.calls.append(x.shape[0])
        return self.net(x)


def test_one_tile_stream_and_the_forced_fallback(dev, models, monkeypatch):
    """The chop path hands all 8 n tiles (16 n with alpha) to the network as one stream; where the buffers do not fit, the tensor path runs the eight
    orientations one after the other -- and returns the same bits, in every form."""
    from innfer_amd import lib as L
    m = models[True]
    h, w = 210, 236
    _, ys, xs = L.chop_plan(h, w, 200, 0.5)
    n = len(ys) * len(xs)
    img, bgra = _image(h, w, 3, 74), _image(40, 56, 4, 75)
    fused = m.run_u8(img, tta=True), m.run_u8(img, seamless="mirror", tta=True), m.run_u8(bgra, fit_channels=True, tta=True)
    net = m.model
    m.model = _Counting(net)
    try:
        m.run_u8(img, tta=True)
        assert sum(m.model.calls) == 8 * n and len(m.model.calls) == 1, m.model.calls
        asked = []
        monkeypatch.setattr(m, "_tta_fits", lambda nbytes, device: asked.append(nbytes) or False)
        m.model.calls = []
        slow = m.run_u8(img, tta=True), m.run_u8(img, seamless="mirror", tta=True), m.run_u8(bgra, fit_channels=True, tta=True)
        assert len(asked) == 3 and asked[0] == 8 * n * 3 * 200 * 200 * (1 + 4) * 2
        assert m.model.calls[:8] == [n] * 8, m.model.calls
    finally:
        m.model = net
    for a, b in zip(fused, slow):
        assert np.array_equal(a, b)


def test_the_ensemble_does_something_and_is_invariant(dev, models):
    """tta=True is not the single run, and it commutes with a flip of the input: the eight orientations of the flipped image are the eight orientations
    of the image (40 x 60, ps 40: the lattice is flip-symmetric as well)."""
    from innfer_amd.utils import utils as U
    m = models[True]
    img = _image(40, 60, 3, 76)
    tta = m.run_u8(img, tta=True)
    assert tta.shape == (80, 120, 3) and not np.array_equal(tta, m.run_u8(img))
    assert np.array_equal(m.run_u8(img, tta=False), m.run_u8(img))
    assert np.array_equal(m.run_u8(U.dihedral(img, 1), tta=True), U.dihedral(tta, 1))


def test_command_line(dev, tmp_path, monkeypatch):
    """`run.py -tta` on a folder of two images writes what run_u8(tta=True) returns; with -seamless and -outscale on top likewise; a chain a>b applies
    forward_tta per model in the tensor loop."""
    from innfer_amd import run as R, synth
    from innfer_amd.utils import utils as U
    for sub in ("models", "in"):
        (tmp_path / sub).mkdir()
    for name, seed in (("2x_a.pth", 81), ("2x_b.pth", 82)):
        torch.save(_sd(synth.rrdbnet_shapes(nb=1, scale=2), seed), str(tmp_path / "models" / name))
    imgs = {"one": _image(40, 56, 3, 83), "two": _image(53, 37, 3, 84)}
    for name, img in imgs.items():
        U.save_img(img, str(tmp_path / "in" / f"{name}.png"))
    monkeypatch.chdir(tmp_path)
    a, b = (R.Model(str(tmp_path / "models" / f), "infer", 2) for f in ("2x_a.pth", "2x_b.pth"))
    assert R.main(["-m", "2x_a", "-i", "in", "-o", "out", "-tta"]) == 0
    assert R.main(["-m", "2x_a", "-i", "in", "-o", "out_s", "-tta", "-seamless", "tile", "-outscale", "1.5"]) == 0
    assert R.main(["-m", "2x_a>2x_b", "-i", "in", "-o", "out_chain", "-tta"]) == 0
    for name, img in imgs.items():
        assert np.array_equal(U.read_img(str(tmp_path / "out" / f"{name}.png")), a.run_u8(img, tta=True)), name
        assert np.array_equal(U.read_img(str(tmp_path / "out_s" / f"{name}.png")), a.run_u8(img, tta=True, seamless="tile", outscale=1.5)), name
        x = U.np2tensor(img, dtype=torch.float16)
        assert np.array_equal(U.read_img(str(tmp_path / "out_chain" / f"{name}.png")), U.tensor2np(b.forward_tta(a.forward_tta(x)))), name
