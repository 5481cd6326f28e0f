"""`-outscale` on the GPU: innfer_resample_inthwc, utils.resample, Model.run_u8(outscale=) and `run.py -outscale`.  Every test states one identity:
the result is utils.resample_np (the numpy statement of the resampler, built from the same host tables) of what the pipeline returns without the
switch -- bit for bit, for the fused kernel, the two-launch form and end to end.  Needs an MI355X: `pytest -m gpu`."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

FILTERS = ("box", "bilinear", "bicubic", "lanczos")
# the shapes of the CPU tests; several blocks each way, one axis down and one up, sizes that are multiples of nothing; a 30x reduction of the rows,
# whose block is a single output row of 16 or 64 pixels
SHAPES = (((37, 52), (18, 26)), ((37, 52), (23, 31)), ((40, 64), (100, 96)), ((64, 48), (7, 5)), ((5, 7), (13, 3)), ((1, 1), (3, 3)), ((33, 47), (33, 20)),
          ((210, 236), (157, 301)), ((300, 40), (10, 40)))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _image(h, w, C, seed, bits=8):
    from innfer_amd import synth
    img = synth.image_u8(h, w, C * (bits // 8), seed)
    return img if bits == 8 else img.view(np.uint16)


_PLANS = {}


def _plan(dev, n_in, n_out, name, wrap):
    """The host tables of one axis on the device: (start, count, weights, T), uploaded once."""
    from innfer_amd import lib as L
    key = (n_in, n_out, name, wrap)
    if key not in _PLANS:
        s, c, w = L.resample_plan(n_in, n_out, name, wrap)
        _PLANS[key] = (torch.from_numpy(s).to(dev), torch.from_numpy(c).to(dev), torch.from_numpy(w).to(dev), w.shape[1])
    return _PLANS[key]


def _kernel(dev, d, bits, oh, ow, name, wrap, ws=None, ws_bytes=None):
    """innfer_resample_inthwc of the device image d into a 0xA5 buffer with 64 guard bytes: (status, result bytes, guard bytes)."""
    from innfer_amd import lib as L
    h, w, C = d.shape
    hs, hc, hw, Th = _plan(dev, w, ow, name, wrap)
    vs, vc, vw, Tv = _plan(dev, h, oh, name, wrap)
    need = L.lib.innfer_resample_workspace_bytes(h, w, C, oh, ow, Th, Tv)
    if ws is None and need:
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
    nbytes = oh * ow * C * (bits // 8)
    buf = torch.full((nbytes + 64,), 0xA5, dtype=torch.uint8, device=dev)
    rc = L.lib.innfer_resample_inthwc(d.data_ptr(), bits, h, w, C, buf.data_ptr(), oh, ow, hs.data_ptr(), hc.data_ptr(), hw.data_ptr(), Th,
                                      vs.data_ptr(), vc.data_ptr(), vw.data_ptr(), Tv, int(wrap), ws.data_ptr() if ws is not None else None,
                                      (need if ws_bytes is None else ws_bytes), _stream())
    got = buf.cpu().numpy()
    return rc, got[:nbytes], got[nbytes:], need


# ------------------------------------------------------------------------------------------------------------------ 1. the fused kernel
@pytest.mark.parametrize("bits", [8, 16])
@pytest.mark.parametrize("name", FILTERS)
def test_kernel_is_resample_np(dev, name, bits):
    """innfer_resample_inthwc == resample_np for every shape, wrap 0 and 1, 1 .. 4 channels; the bytes behind the output stay as they were; all of
    these run as the one fused launch (no workspace); tensor in -> tensor out and numpy in -> numpy out of utils.resample."""
    from innfer_amd import lib as L
    from innfer_amd.utils import utils as U
    dt = np.uint8 if bits == 8 else np.uint16
    for k, ((h, w), (oh, ow)) in enumerate(SHAPES):
        for C in (1, 2, 3, 4):
            img = _image(h, w, C, 10 * k + C, bits)
            d = torch.from_numpy(img if bits == 8 else img.view(np.int16)).to(dev)
            for wrap in (False, True):
                want = U.resample_np(img, oh, ow, name, wrap)
                rc, got, guard, need = _kernel(dev, d, bits, oh, ow, name, wrap)
                assert rc == L.OK and need == 0, (h, w, oh, ow, C, wrap, L.last_error())
                assert np.array_equal(got.view(dt).reshape(want.shape), want), (h, w, oh, ow, C, wrap)
                assert (guard == 0xA5).all(), (h, w, oh, ow, C, wrap)
                rd = U.resample(d, size=(oh, ow), filter=name, wrap=wrap)
                assert rd.is_cuda and rd.dtype == d.dtype and np.array_equal(rd.cpu().numpy().view(dt), want), (h, w, oh, ow, C, wrap)
        r = U.resample(img, size=(oh, ow), filter=name)                            # numpy in, numpy out (C = 4, truncated window)
        assert isinstance(r, np.ndarray) and r.dtype == img.dtype and np.array_equal(r, U.resample_np(img, oh, ow, name)), (h, w, oh, ow)
    gray = _image(37, 52, 1, 90, bits)[:, :, 0]                                      # HW, and scale= by Real-ESRGAN's rule
    assert np.array_equal(U.resample(gray, scale=0.75, filter=name), U.resample_np(gray, 27, 39, name))
    assert U.resample(gray, size=(37, 52), filter=name) is gray                      # the source size: no call is made


# ------------------------------------------------------------------------------------------------------------------ 2. the two-launch form
@pytest.mark.parametrize("bits", [8, 16])
def test_fallback_through_the_workspace(dev, bits):
    """(1400, 24) -> (3, 5) with lanczos: 2801-tap windows, no block fits LDS -- the two launches through the float32 intermediate give resample_np
    too; too small a workspace is INNFER_ERR_WORKSPACE and nothing is written."""
    from innfer_amd import lib as L
    from innfer_amd.utils import utils as U
    dt = np.uint8 if bits == 8 else np.uint16
    for C in (1, 3, 4):
        img = _image(1400, 24, C, 20 + C, bits)
        d = torch.from_numpy(img if bits == 8 else img.view(np.int16)).to(dev)
        for wrap in (False, True):
            want = U.resample_np(img, 3, 5, "lanczos", wrap)
            rc, got, guard, need = _kernel(dev, d, bits, 3, 5, "lanczos", wrap)
            assert need == 1400 * 5 * C * 4 and rc == L.OK, (C, wrap, need, L.last_error())
            assert np.array_equal(got.view(dt).reshape(want.shape), want) and (guard == 0xA5).all(), (C, wrap)
            assert np.array_equal(U.resample(img, size=(3, 5), wrap=wrap), want), (C, wrap)
    small = torch.empty(need - 4, dtype=torch.uint8, device=dev)
    rc, got, guard, _ = _kernel(dev, d, bits, 3, 5, "lanczos", False, ws=small, ws_bytes=need - 4)
    assert rc == L.ERR_WORKSPACE and (got == 0xA5).all() and "workspace" in L.last_error()
    rc, got, guard, _ = _kernel(dev, d, bits, 3, 5, "lanczos", False, ws=small, ws_bytes=0)
    assert rc == L.ERR_WORKSPACE and (got == 0xA5).all()


# ------------------------------------------------------------------------------------------------------------------ 3. end to end
def _sd(shapes, seed=0):
    from innfer_amd import synth
    return {k: torch.from_numpy(v) for k, v in synth.fill_state_dict(shapes, seed).items()}


@pytest.fixture(scope="module")
def models(tmp_path_factory):
    from innfer_amd import run as R, synth
    tmp = tmp_path_factory.mktemp("resample_models")
    path = str(tmp / "2x_resample_80.pth")
    torch.save(_sd(synth.rrdbnet_shapes(nb=1, scale=2), 80), path)
    return {chop: R.Model(path, "infer", 2, chop=chop) for chop in (True, False)}


@pytest.mark.parametrize("chop", [True, False])
def test_run_u8_outscale(dev, models, chop):
    """run_u8(img, outscale=F) == resample_np(run_u8(img), int(H F), int(W F)) for F above and below 1 on a 2x model, every filter once, a BGRA
    image under fit_channels, and seamless='tile' against the wrapped window; F = the model's scale is the plain result; device tensors and out=."""
    from innfer_amd.utils import utils as U
    m = models[chop]
    for (h, w, seed) in ((37, 52, 1), (210, 236, 2)):
        img = _image(h, w, 3, seed)
        plain = m.run_u8(img)
        for F, name in ((1.5, "lanczos"), (0.75, "lanczos"), (1.5, "bicubic"), (0.75, "box"), (1.5, "bilinear")):
            got = m.run_u8(img, outscale=F, outfilter=name)
            assert isinstance(got, np.ndarray) and got.dtype == np.uint8 and got.shape == (int(h * F), int(w * F), 3), (chop, h, w, F, name)
            assert np.array_equal(got, U.resample_np(plain, int(h * F), int(w * F), name)), (chop, h, w, F, name)
        assert np.array_equal(m.run_u8(img, outscale=2), plain) and np.array_equal(m.run_u8(img, outscale=None), plain)
    h, w = 37, 52
    assert np.array_equal(m.run_u8(img[:h, :w], outscale=1.5), m.run_u8(img[:h, :w], outscale=1.5, outfilter="lanczos"))      # the default filter
    bgra = _image(h, w, 4, 3)
    for F in (1.5, 0.75):
        got = m.run_u8(bgra, fit_channels=True, outscale=F)
        assert got.shape == (int(h * F), int(w * F), 4), (chop, F)
        assert np.array_equal(got, U.resample_np(m.run_u8(bgra, fit_channels=True), int(h * F), int(w * F))), (chop, F)
        tex = _image(h, w, 3, 4)
        got = m.run_u8(tex, seamless="tile", outscale=F)
        tiled = m.run_u8(tex, seamless="tile")
        assert np.array_equal(got, U.resample_np(tiled, int(h * F), int(w * F), wrap=True)), (chop, F)
        assert not np.array_equal(got, U.resample_np(tiled, int(h * F), int(w * F), wrap=False)), (chop, F)
        got = m.run_u8(tex, seamless="mirror", outscale=F)                           # the other modes: the truncated window
        assert np.array_equal(got, U.resample_np(m.run_u8(tex, seamless="mirror"), int(h * F), int(w * F))), (chop, F)
    gray = _image(h, w, 1, 5)[:, :, 0]                                               # a 2-D image comes back 2-D
    got = m.run_u8(gray, fit_channels=True, outscale=1.5)
    assert got.shape == (55, 78) and np.array_equal(got, U.resample_np(m.run_u8(gray, fit_channels=True), 55, 78))
    d = torch.from_numpy(tex).to(dev)
    want = m.run_u8(tex, outscale=1.5)
    r = m.run_u8(d, outscale=1.5)
    assert r.is_cuda and r.is_contiguous() and np.array_equal(r.cpu().numpy(), want)
    out = torch.full((55, 78, 3), 9, dtype=torch.uint8, device=dev)
    r = m.run_u8(d, outscale=1.5, out=out)
    assert r.data_ptr() == out.data_ptr() and np.array_equal(out.cpu().numpy(), want)
    r = m.run_u8(d, outscale=2)                                                     # the model's scale: its own result, untouched
    assert np.array_equal(r.cpu().numpy(), m.run_u8(tex))
    with pytest.raises(ValueError, match="out"):
        m.run_u8(d, outscale=1.5, out=torch.empty((74, 104, 3), dtype=torch.uint8, device=dev))
    with pytest.raises(ValueError, match="scale"):
        m.run_u8(tex, outscale=0)
    with pytest.raises(ValueError, match="filter"):
        m.run_u8(tex, outscale=1.5, outfilter="nearest")


# ------------------------------------------------------------------------------------------------------------------ 4. the command line
def test_command_line(dev, tmp_path, monkeypatch):
    """`run.py -outscale 1.5 -outfilter bicubic` on two files writes resample_np of what the same command writes without the flags -- on the run_u8
    route, on the host-side order of -cf (chain -> colour fix -> resample) -- and -comp saves the input beside the smaller result."""
    from innfer_amd import run as R, synth
    from innfer_amd.utils import utils as U
    for sub in ("models", "in"):
        (tmp_path / sub).mkdir()
    torch.save(_sd(synth.rrdbnet_shapes(nb=1, scale=2), 81), str(tmp_path / "models" / "2x_a.pth"))
    sizes = {"a": (40, 56), "b": (33, 47)}
    for name, (h, w) in sizes.items():
        U.save_img(_image(h, w, 3, 82 + h), str(tmp_path / "in" / f"{name}.png"))
    monkeypatch.chdir(tmp_path)
    flags = ["-outscale", "1.5", "-outfilter", "bicubic"]
    for tag, extra in (("plain", []), ("cf", ["-cf"])):
        assert R.main(["-m", "2x_a", "-i", "in", "-o", f"ref_{tag}"] + extra) == 0
        assert R.main(["-m", "2x_a", "-i", "in", "-o", f"out_{tag}"] + extra + flags) == 0
        for name, (h, w) in sizes.items():
            ref = U.read_img(str(tmp_path / f"ref_{tag}" / f"{name}.png"))
            got = U.read_img(str(tmp_path / f"out_{tag}" / f"{name}.png"))
            assert ref.shape == (2 * h, 2 * w, 3) and got.shape == (int(h * 1.5), int(w * 1.5), 3), (tag, name)
            assert np.array_equal(got, U.resample_np(ref, int(h * 1.5), int(w * 1.5), "bicubic")), (tag, name)
    assert R.main(["-m", "2x_a", "-i", "in", "-o", "out_comp", "-comp"] + flags) == 0
    for name, (h, w) in sizes.items():
        comp = U.read_img(str(tmp_path / "out_comp" / f"{name}.png"))
        assert comp.shape == (int(h * 1.5), 2 * int(w * 1.5), 3), name
        assert np.array_equal(comp[:, int(w * 1.5):], U.read_img(str(tmp_path / "out_plain" / f"{name}.png"))), name
