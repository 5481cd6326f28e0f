"""The colour fixes `-cf_mode wavelet | adain` on the GPU (csrc/colorfix.hip: innfer_color_fix_mode) and the fix inside run_u8 / run_u8_batch /
FramePipeline / the command line.

1. the kernels: utils.color_fix(a, b, mode=m) == utils.color_fix_np(a, b, m) TO THE CODE -- every operation is +, -, *, /, sqrt or floor in a stated order,
   contraction is off, the sums are integers -- at shapes that clamp both edges inside one tile, cross tile boundaries off the tile grid (SR extents T + 1 and
   2 T + 31 for the wavelet kernel's T = 64), enlarge by no factor, by 4 and by a non-integer ratio, with 1, 3 and 4 channels;
2. the definition: run_u8(img, color_fix=m) == utils.color_fix(img, run_u8(img), mode=m) [resampled] on every path, run_u8_batch == the list;
3. the command line and FramePipeline.
Every comparison is exact.  Needs an MI355X: `pytest -m gpu`."""
import numpy as np
import pytest
import torch

from test_gpu_tile import SENTINEL, _guarded, _rrdb_model, _tail_intact

pytestmark = pytest.mark.gpu

MODES = ("lowfreq", "wavelet", "adain")
NEW = MODES[1:]
T = 64                                                          # WV_T of csrc/colorfix.hip: the core of a wavelet tile (halo 31)
# (LR size, SR size, C)
SHAPES = (((9, 70), (36, 280), 3),                              # x4; SR height 36 < 2 * 31 + 1: both edges clamp inside one tile
          ((20, 30), (T + 1, 2 * T + 31), 3),                   # off the tile grid: a 1-px last tile row, three tile columns
          ((30, 30), (30, 30), 3),                              # equal sizes: nothing is enlarged
          ((17, 9), (68, 36), 1),
          ((12, 14), (48, 56), 4),
          ((20, 24), (50, 70), 3),                              # a non-integer ratio
          ((40, 50), (3 * T + 5, 3 * T + 1), 2),                # interior tiles: a core whose whole halo lies inside the image, on both axes
          ((150, 140), (152, 141), 1))                          # a ratio near 1: a window's taps touch more LR rows than the LDS plane holds (the direct form)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _pair(lr, sr, C, seed=1):
    from innfer_amd import synth
    return synth.image_u8(lr[0], lr[1], C, seed), synth.image_u8(sr[0], sr[1], C, seed + 1)


# ------------------------------------------------------------------------------------------------------------------ 1. the kernels
@pytest.mark.parametrize("mode", NEW)
@pytest.mark.parametrize("lr,sr,C", SHAPES, ids=[f"{a[0]}x{a[1]}-{b[0]}x{b[1]}-c{c}" for a, b, c in SHAPES])
def test_kernel_equals_the_contract(dev, lr, sr, C, mode):
    from innfer_amd.utils import utils as U
    a, b = _pair(lr, sr, C)
    want = U.color_fix_np(a, b, mode)
    got = U.color_fix(a, b, mode=mode)
    assert isinstance(got, np.ndarray) and got.dtype == np.uint8 and got.shape == want.shape
    d = np.abs(got.astype(int) - want.astype(int))
    print(f"{mode} {lr} -> {sr} C={C}: max {d.max()} code, {np.count_nonzero(d)} of {d.size} values differ")
    assert np.array_equal(got, want)
    # cuda tensors in, a cuda tensor out, into `out`, and nothing is written behind it
    ta, tb = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)
    buf, out = _guarded(b.shape, torch.uint8, dev)
    r = U.color_fix(ta, tb, mode=mode, out=out)
    assert r is out and _tail_intact(buf) and np.array_equal(out.cpu().numpy(), want)
    r = U.color_fix(ta, tb, mode=mode)
    assert torch.is_tensor(r) and r.is_cuda and np.array_equal(r.cpu().numpy(), want)


def test_unaligned_images_and_large_sums(dev):
    """adain moves four values per thread as one dword where both pointers allow it: an SR image and a result at odd addresses take the scalar form.
    300 x 300 values of 255 per channel: the sum of squares passes 2^32."""
    from innfer_amd import synth
    from innfer_amd.utils import utils as U
    a, b = _pair((20, 30), (65, 159), 3, seed=7)
    want = {m: U.color_fix_np(a, b, m) for m in NEW}
    ta = torch.from_numpy(a).to(dev)
    raw = torch.zeros(b.size + 64, dtype=torch.uint8, device=dev)
    tb = raw[1:1 + b.size].view(b.shape)
    tb.copy_(torch.from_numpy(b))
    buf = torch.full((b.size + 65,), SENTINEL[torch.uint8], dtype=torch.uint8, device=dev)
    out = buf[1:1 + b.size].view(b.shape)
    assert tb.data_ptr() % 4 == 1 and out.data_ptr() % 4 == 1
    for m in NEW:
        assert U.color_fix(ta, tb, mode=m, out=out) is out
        assert np.array_equal(out.cpu().numpy(), want[m]) and _tail_intact(buf) and int(buf[0]) == SENTINEL[torch.uint8], m
    a = np.full((300, 300, 3), 255, np.uint8)
    a[::2, :, 1] = 0
    b = synth.image_u8(300, 300, 3, 4)
    assert np.array_equal(U.color_fix(a, b, mode="adain"), U.color_fix_np(a, b, "adain"))


def test_mode_zero_is_innfer_color_fix_and_refusals_launch_nothing(dev):
    from innfer_amd import lib as L
    from innfer_amd.utils import utils as U
    a, b = _pair((20, 24), (50, 70), 3)
    ta, tb = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)
    assert np.array_equal(U.color_fix(a, b, mode="lowfreq"), U.color_fix(a, b))
    out = torch.full(b.shape, SENTINEL[torch.uint8], dtype=torch.uint8, device=dev)
    ws = torch.zeros(1 << 16, dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    # mode 0 through the new entry is the old entry
    L.check(L.lib.innfer_color_fix_mode(0, ta.data_ptr(), 20, 24, tb.data_ptr(), 50, 70, 3, out.data_ptr(), ws.data_ptr(), ws.numel(), stream))
    assert np.array_equal(out.cpu().numpy(), U.color_fix(a, b))
    out.fill_(SENTINEL[torch.uint8])
    ok = dict(mode=2, a=ta.data_ptr(), hA=20, wA=24, b=tb.data_ptr(), hB=50, wB=70, C=3, out=out.data_ptr(), ws=ws.data_ptr(), n=ws.numel())
    for change, exc, match in ((dict(mode=3), ValueError, "mode"), (dict(mode=-1), ValueError, "mode"), (dict(a=None), ValueError, "null"), (dict(out=None), ValueError, "null"),
                               (dict(hA=60, wA=80), ValueError, "cannot be subtracted"), (dict(hA=50, wA=24), ValueError, "cannot be subtracted"),
                               (dict(C=5), ValueError, "bad shape"), (dict(hB=0), ValueError, "bad shape"), (dict(n=8), L.InnferError, "workspace"),
                               (dict(ws=None), L.InnferError, "workspace"), (dict(mode=1, C=0), ValueError, "bad shape"), (dict(mode=1, b=None), ValueError, "null")):
        k = dict(ok, **change)
        with pytest.raises(exc, match=match):
            L.check(L.lib.innfer_color_fix_mode(k["mode"], k["a"], k["hA"], k["wA"], k["b"], k["hB"], k["wB"], k["C"], k["out"], k["ws"], k["n"], stream))
    torch.cuda.synchronize()
    assert bool((out == SENTINEL[torch.uint8]).all())
    with pytest.raises(ValueError, match="mode"):
        U.color_fix(a, b, mode="histogram")
    with pytest.raises(ValueError, match="out must"):
        U.color_fix(ta, tb, mode="adain", out=torch.empty((50, 70, 4), dtype=torch.uint8, device=dev))
    with pytest.raises(ValueError, match="out must not be"):
        U.color_fix(ta, tb, mode="wavelet", out=tb)


# ------------------------------------------------------------------------------------------------------------------ 2. the definition
@pytest.fixture(scope="module")
def rrdb(tmp_path_factory):
    return _rrdb_model(tmp_path_factory)


@pytest.fixture(scope="module")
def rrdb_whole(tmp_path_factory):
    return _rrdb_model(tmp_path_factory, chop=False)


@pytest.fixture(scope="module")
def img():
    from innfer_amd import synth
    return synth.image_u8(44, 56, 3, 31)


def _defined(m, img, mode, outscale=None, seamless=None, **kw):
    """utils.color_fix(img, run_u8(img, <the options without color_fix and outscale>), mode) [then resample_np], from the separate calls."""
    from innfer_amd.utils import utils as U
    plain = m.run_u8(img, seamless=seamless, **kw)
    flat = img.ndim == 2
    fixed = U.color_fix(img[:, :, None] if flat else img, plain[:, :, None] if flat else plain, mode=mode)
    fixed = fixed[:, :, 0] if flat else fixed
    if outscale is None:
        return fixed
    oh, ow = U.resample_size(img.shape[0], img.shape[1], outscale)
    return U.resample_np(fixed, oh, ow, "lanczos", wrap=seamless == "tile")


@pytest.mark.parametrize("mode", MODES)
def test_run_u8_color_fix_is_the_two_calls(dev, rrdb, rrdb_whole, img, mode):
    from innfer_amd import synth
    for m, kw in ((rrdb, {}), (rrdb_whole, {}), (rrdb, dict(seamless="tile")), (rrdb_whole, dict(seamless="tile")), (rrdb, dict(outscale=2.5)),
                  (rrdb, dict(seamless="tile", outscale=2.5)), (rrdb, dict(tta=True))):
        want = _defined(m, img, mode, **kw)
        got = m.run_u8(img, color_fix=mode, **kw)
        assert isinstance(got, np.ndarray) and got.dtype == np.uint8 and got.shape == want.shape and np.array_equal(got, want), (mode, kw)
    # a cuda image stays on the device, `out` is honoured
    d = torch.from_numpy(img).to(dev)
    want = _defined(rrdb, img, mode)
    out = torch.empty(want.shape, dtype=torch.uint8, device=dev)
    assert rrdb.run_u8(d, color_fix=mode, out=out) is out and np.array_equal(out.cpu().numpy(), want)
    want = _defined(rrdb, img, mode, outscale=2.5)
    out = torch.empty(want.shape, dtype=torch.uint8, device=dev)
    assert rrdb.run_u8(d, color_fix=mode, outscale=2.5, out=out) is out and np.array_equal(out.cpu().numpy(), want)
    # fit_channels: BGRA, and a 2-D image (fixed as H x W x 1)
    rgba = synth.image_u8(40, 48, 4, 32)
    for m in (rrdb, rrdb_whole):
        assert np.array_equal(m.run_u8(rgba, fit_channels=True, color_fix=mode), _defined(m, rgba, mode, fit_channels=True)), mode
    gray = synth.image_u8(40, 48, 1, 33)[:, :, 0]
    got = rrdb.run_u8(gray, fit_channels=True, color_fix=mode)
    assert got.shape == (80, 96) and np.array_equal(got, _defined(rrdb, gray, mode, fit_channels=True)), mode


def test_run_u8_color_fix_refusals(rrdb, img):
    with pytest.raises(ValueError, match="mode"):
        rrdb.run_u8(img, color_fix="histogram")
    with pytest.raises(ValueError, match="mode"):
        rrdb.run_u8_batch([img, img], color_fix="histogram")


@pytest.mark.parametrize("mode", MODES)
def test_run_u8_batch_is_the_list(dev, rrdb, mode, monkeypatch):
    from innfer_amd import synth
    imgs = [synth.image_u8(h, w, 3, 40 + i) for i, (h, w) in enumerate(((40, 56), (56, 40), (64, 50)))]      # ps 40, 40 and 50: a group of two, one alone
    for kw in ({}, dict(outscale=1.5), dict(seamless="mirror")):
        want = [rrdb.run_u8(im, color_fix=mode, **kw) for im in imgs]
        calls = []
        inner = rrdb._chop_u8_multi
        with monkeypatch.context() as mp:
            mp.setattr(rrdb, "_chop_u8_multi", lambda *a, **k: (calls.append(len(a[1])), inner(*a, **k))[1])
            got = rrdb.run_u8_batch(imgs, color_fix=mode, **kw)
            cuda = rrdb.run_u8_batch([torch.from_numpy(im).to(dev) for im in imgs], color_fix=mode, **kw)
        assert calls == [2, 2]                                                                # the fast path ran, for both forms
        for g, c, w in zip(got, cuda, want):
            assert np.array_equal(g, w) and c.is_cuda and np.array_equal(c.cpu().numpy(), w), (mode, kw)


# ------------------------------------------------------------------------------------------------------------------ 3. the command line, FramePipeline
def test_command_line(dev, tmp_path, monkeypatch):
    """`-cf_mode wavelet -outscale 2` writes what the definition gives; `-cf` alone and `-cf -outscale 2` write the files of the separate steps
    utils.resample(utils.color_fix(img, run_u8(img))); -cf_mode alone turns the fix on; -batch and -fit_channels write the same files."""
    from innfer_amd import run as R, synth
    from innfer_amd.run import Model
    from innfer_amd.utils import utils as U
    for sub in ("models", "in"):
        (tmp_path / sub).mkdir()
    torch.save({k: torch.from_numpy(v) for k, v in synth.fill_state_dict(synth.rrdbnet_shapes(nb=1, scale=4), 77).items()}, str(tmp_path / "models" / "4x_a.pth"))
    imgs = {f"tex{i}": synth.image_u8(h, w, 3, 60 + i) for i, (h, w) in enumerate(((40, 56), (48, 40), (40, 56)))}
    for name, im in imgs.items():
        U.save_img(im, str(tmp_path / "in" / f"{name}.png"))
    monkeypatch.chdir(tmp_path)
    m = Model(str(tmp_path / "models" / "4x_a.pth"), "infer", 4)
    plain = {name: m.run_u8(im) for name, im in imgs.items()}

    def files(tag, extra):
        assert R.main(["-m", "4x_a", "-i", "in", "-o", f"out_{tag}"] + extra) == 0
        return {name: U.read_img(str(tmp_path / f"out_{tag}" / f"{name}.png")) for name in imgs}

    def final(im, name):
        return U.resample(im, size=U.resample_size(*imgs[name].shape[:2], 2), filter="lanczos")
    for tag, extra, want in (("wv2", ["-cf_mode", "wavelet", "-outscale", "2"], lambda n: final(U.color_fix(imgs[n], plain[n], mode="wavelet"), n)),
                             ("cf", ["-cf"], lambda n: U.color_fix(imgs[n], plain[n])),
                             ("cf2", ["-cf", "-outscale", "2"], lambda n: final(U.color_fix(imgs[n], plain[n]), n)),
                             ("ad", ["-cf_mode", "adain"], lambda n: U.color_fix(imgs[n], plain[n], mode="adain")),
                             ("cflow", ["-cf", "-cf_mode", "lowfreq"], lambda n: U.color_fix(imgs[n], plain[n])),
                             ("wvb", ["-cf_mode", "wavelet", "-batch", "3"], lambda n: U.color_fix(imgs[n], plain[n], mode="wavelet"))):
        got = files(tag, extra)
        for name in imgs:
            assert np.array_equal(got[name], want(name)), (tag, name)
    assert not np.array_equal(files("plain", [])["tex0"], U.color_fix(imgs["tex0"], plain["tex0"]))
    # a chain is not run_u8's: the fix is the separate step behind it, as before
    torch.save({k: torch.from_numpy(v) for k, v in synth.fill_state_dict(synth.rrdbnet_shapes(nb=1, scale=2), 78).items()}, str(tmp_path / "models" / "2x_b.pth"))
    assert R.main(["-m", "2x_b+2x_b", "-i", "in", "-o", "out_chain", "-cf_mode", "adain"]) == 0
    assert R.main(["-m", "2x_b+2x_b", "-i", "in", "-o", "out_chain_plain"]) == 0
    for name in imgs:
        chain = U.read_img(str(tmp_path / "out_chain_plain" / f"{name}.png"))
        assert np.array_equal(U.read_img(str(tmp_path / "out_chain" / f"{name}.png")), U.color_fix(imgs[name], chain, mode="adain")), name


def test_frame_pipeline(dev, rrdb):
    from innfer_amd import synth
    from innfer_amd.pipeline import FramePipeline
    from innfer_amd.utils import utils as U
    frames = [synth.image_u8(40, 56, 3, 90 + i) for i in range(3)]
    plain = [rrdb.run_u8(f) for f in frames]
    for cf, mode in (("adain", "adain"), ("wavelet", "wavelet"), (True, "lowfreq"), ("lowfreq", "lowfreq")):
        got = [o.copy() for o in FramePipeline(rrdb, scale=2, device=dev, depth=2, color_fix=cf)(frames)]
        for g, f, p in zip(got, frames, plain):
            assert np.array_equal(g, U.color_fix(f, p, mode=mode)), cf
    with pytest.raises(ValueError, match="mode"):
        FramePipeline(rrdb, scale=2, device=dev, color_fix="histogram")
