"""fit_channels: gray (HW, HW1), gray + alpha (HW2) and BGRA images through an RGB (3 -> 3) network -- Model.run_u8(fit_channels=True), the
tensor path (utils.fit_channels_forward) and `run.py -fit_channels`.  The colour plane must be exactly what the 3-channel machinery returns, the
gray / alpha plane exactly mean3 of the network's result on the plane replicated to three channels; a constant alpha plane is copied and not run.
Needs an MI355X: `pytest -m gpu`."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _sd(shapes, seed=0):
    from innfer_amd import synth
    return {k: torch.from_numpy(v) for k, v in synth.fill_state_dict(shapes, seed).items()}


def _model(tmp_path, chop, seed=90, scale=2, name=None):
    from innfer_amd import run as R, synth
    path = str(tmp_path / (name or f"{scale}x_fit_{seed}.pth"))
    sd = _sd(synth.rrdbnet_shapes(nb=1, scale=scale), seed)
    torch.save(sd, path)
    return R.Model(path, "infer", scale, chop=chop), sd


def _mean3_codes(y, normalize, imtype=np.uint8):
    """The contract's mean3, computed here on the CPU: ((y0 + y1) + y2) / 3 in fp32 of the result's channels, rounded to the result dtype,
    quantised by tensor2np (a 2-D tensor: one plane, no channel flip)."""
    from innfer_amd.utils import utils as U
    yc = y.detach().float().cpu()
    m = (((yc[0, 0] + yc[0, 1]) + yc[0, 2]) / 3).to(y.dtype)
    return U.tensor2np(m.to(y.device), denormalize=normalize, data_range=255 if imtype == np.uint8 else 65535, imtype=imtype)


def _plane_codes(m, plane, normalize, dtype):
    """mean3 codes of m(np2tensor(plane replicated to three channels)): what a gray or alpha plane must come out as."""
    from innfer_amd.utils import utils as U
    rep = np.ascontiguousarray(np.repeat(plane[:, :, None], 3, axis=2))
    return _mean3_codes(m(U.np2tensor(rep, normalize=normalize, dtype=dtype)), normalize, np.uint8 if plane.dtype == np.uint8 else np.uint16)


@pytest.mark.parametrize("chop", [True, False])
def test_colour_unchanged_and_planes_exact(dev, tmp_path, chop):
    """BGRA: B, G, R bit-identical to run_u8 of the BGR image, alpha = mean3 of the network on (a, a, a).  Gray HW / HW1 / HW2: gray = mean3 of the
    network on (g, g, g), alpha as above.  fp16 and fp32 mode, [-1, 1] normalisation on and off, images smaller and larger than a 200-px tile; the
    fused chop path (tile gather / blend) and the tensor path (split / merge around the forward) agree bit for bit."""
    from innfer_amd import synth
    from innfer_amd.utils import utils as U
    m, _ = _model(tmp_path, chop)
    for (h, w, seed) in [(37, 52, 1), (210, 236, 2)]:
        bgra = synth.image_u8(h, w, 4, seed)
        gray = synth.image_u8(h, w, 1, seed + 10)[:, :, 0]
        ga = np.ascontiguousarray(np.stack([gray, bgra[:, :, 3]], axis=2))
        for fp16 in (True, False):
            dt = torch.float16 if fp16 else torch.float32
            for normalize in (False, True):
                tag = (chop, h, w, fp16, normalize)
                got = m.run_u8(bgra, normalize=normalize, fp16=fp16, fit_channels=True)
                assert got.dtype == np.uint8 and got.shape == (2 * h, 2 * w, 4), tag
                assert np.array_equal(got[:, :, :3], m.run_u8(np.ascontiguousarray(bgra[:, :, :3]), normalize=normalize, fp16=fp16)), tag
                want_a = _plane_codes(m, bgra[:, :, 3], normalize, dt)
                assert np.array_equal(got[:, :, 3], want_a), tag
                assert np.array_equal(U.fit_channels_forward(m, bgra, normalize=normalize, dtype=dt), got), tag
                want_g = _plane_codes(m, gray, normalize, dt)
                g2 = m.run_u8(gray, normalize=normalize, fp16=fp16, fit_channels=True)
                assert g2.shape == (2 * h, 2 * w) and np.array_equal(g2, want_g), tag
                g1 = m.run_u8(gray[:, :, None], normalize=normalize, fp16=fp16, fit_channels=True)
                assert g1.shape == (2 * h, 2 * w, 1) and np.array_equal(g1[:, :, 0], want_g), tag
                got_ga = m.run_u8(ga, normalize=normalize, fp16=fp16, fit_channels=True)
                assert got_ga.shape == (2 * h, 2 * w, 2), tag
                assert np.array_equal(got_ga[:, :, 0], want_g) and np.array_equal(got_ga[:, :, 1], want_a), tag
                assert np.array_equal(U.fit_channels_forward(m, ga, normalize=normalize, dtype=dt), got_ga), tag
                assert np.array_equal(U.fit_channels_forward(m, gray, normalize=normalize, dtype=dt), g2), tag
    # a device image stays on the device
    d = torch.from_numpy(bgra).to(dev)
    r = m.run_u8(d, fit_channels=True)
    assert r.is_cuda and np.array_equal(r.cpu().numpy(), m.run_u8(bgra, fit_channels=True))


def test_against_the_oracle(dev, tmp_path):
    """The oracle's chop_forward of the fp32 RRDBNet on the colour plane and on (a, a, a), mean3 and quantise: >= 99 % of the uint8 codes within +-1
     on every channel of the fp16 result."""
    import oracle
    from innfer_amd import synth
    m, sd = _model(tmp_path, True, seed=91)
    bgra = synth.image_u8(96, 120, 4, 5)
    got = m.run_u8(bgra, fit_channels=True).astype(np.int32)
    f = lambda t: oracle.rrdbnet_forward(sd, t, nb=1, scale=2)
    with torch.no_grad():
        col = oracle.tensor2np(oracle.chop_forward(f, oracle.np2tensor(np.ascontiguousarray(bgra[:, :, :3])), 2)).astype(np.int32)
        ya = oracle.chop_forward(f, oracle.np2tensor(np.ascontiguousarray(np.repeat(bgra[:, :, 3:], 3, axis=2))), 2).float()
    alpha = oracle.tensor2np(((ya[0, 0] + ya[0, 1]) + ya[0, 2]) / 3).astype(np.int32)
    for c in range(3):
        assert (np.abs(got[:, :, c] - col[:, :, c]) <= 1).mean() >= 0.99, c
    assert (np.abs(got[:, :, 3] - alpha) <= 1).mean() >= 0.99


class _Counting:
    """Stands in for Model.model: counts the tiles / images it is given."""

    def __init__(self, net):
        self.net, self.seen = net, 0

    def __call__(self, x):
        self.seen += x.shape[0]
        return self.net(x)


def test_constant_alpha_is_copied_not_run(dev, tmp_path):
    """An alpha plane of one value (0, 255, 77 in uint8; 40000 in uint16) comes out as that value exactly, and the network sees only the colour
    tiles (n, not 2n); a varying alpha plane sends 2n tiles."""
    from innfer_amd import lib as L, synth
    from innfer_amd.utils import utils as U
    m, _ = _model(tmp_path, True, seed=92)
    h, w = 150, 230
    bgra = synth.image_u8(h, w, 4, 7)
    _, ys, xs = L.chop_plan(h, w, 150, 0.5)
    n = len(ys) * len(xs)
    colour = m.run_u8(np.ascontiguousarray(bgra[:, :, :3]))
    net = m.model
    m.model, m.tile_batch = _Counting(net), 64
    try:
        for v in (0, 255, 77):
            img = bgra.copy()
            img[:, :, 3] = v
            m.model.seen = 0
            got = m.run_u8(img, fit_channels=True)
            assert m.model.seen == n, (v, m.model.seen, n)
            assert (got[:, :, 3] == v).all() and np.array_equal(got[:, :, :3], colour), v
        m.model.seen = 0
        m.run_u8(bgra, fit_channels=True)
        assert m.model.seen == 2 * n
    finally:
        m.model = net
    img16 = (synth.image_u8(h, w, 4, 8).astype(np.uint16) * 257)
    img16[:, :, 3] = 40000
    calls = []
    out16 = U.fit_channels_forward(lambda t: calls.append(t.shape) or m(t), img16, dtype=torch.float16)
    assert len(calls) == 1 and out16.dtype == np.uint16 and out16.shape == (2 * h, 2 * w, 4)
    assert (out16[:, :, 3] == 40000).all()
    want = U.tensor2np(m(U.np2tensor(np.ascontiguousarray(img16[:, :, :3]), dtype=torch.float16)), data_range=65535, imtype=np.uint16)
    assert np.array_equal(out16[:, :, :3], want)


def test_default_unchanged(dev, tmp_path):
    """Without the switch a BGRA image with a 3-channel network still raises, and a 2-D image is still refused."""
    from innfer_amd import synth
    m, _ = _model(tmp_path, False, seed=93)
    with pytest.raises(ValueError, match="4 channels"):
        m.run_u8(synth.image_u8(40, 48, 4, 9))
    with pytest.raises(TypeError):
        m.run_u8(synth.image_u8(40, 48, 1, 9)[:, :, 0])


def test_command_line(dev, tmp_path, monkeypatch):
    """`run.py -fit_channels` over a folder of RGB, RGBA, LA, L and 16-bit L files: every file gets an output of its own mode at scale x size (LA
    comes back RGBA: both readers turn it into BGRA) holding what the library calls return; an `a>b` chain and an un-chopped pix2pix model
    (`-a p2p_256`) too."""
    from PIL import Image
    from innfer_amd import run as R, synth
    from innfer_amd.architectures import get_network
    from innfer_amd.utils import utils as U
    from innfer_amd.utils.defaults import get_network_G_config
    (tmp_path / "models").mkdir(); (tmp_path / "in").mkdir(); (tmp_path / "in256").mkdir()
    for name, scale, seed in (("1x_clean.pth", 1, 94), ("2x_up.pth", 2, 95)):
        torch.save(_sd(synth.rrdbnet_shapes(nb=1, scale=scale), seed), str(tmp_path / "models" / name))
    h, w = 40, 56
    files = {
        "rgb": (Image.fromarray(synth.image_u8(h, w, 3, 20)), "RGB"),
        "rgba": (Image.fromarray(synth.image_u8(h, w, 4, 21), "RGBA"), "RGBA"),
        "la": (Image.fromarray(synth.image_u8(h, w, 2, 22), "LA"), "RGBA"),
        "l": (Image.fromarray(synth.image_u8(h, w, 1, 23)[:, :, 0], "L"), "L"),
        "l16": (Image.fromarray(synth.image_u8(h, w, 2, 24).view(np.uint16)[:, :, 0].copy()), None),
    }
    for k, (im, _) in files.items():
        im.save(str(tmp_path / "in" / f"{k}.png"))
    monkeypatch.chdir(tmp_path)
    m2 = R.Model(str(tmp_path / "models" / "2x_up.pth"), "infer", 2)
    m1 = R.Model(str(tmp_path / "models" / "1x_clean.pth"), "infer", 1)
    for tag, chain, fn in (("out", "2x_up", m2), ("out_chain", "clean>2x_up", lambda t: m2(m1(t)))):
        assert R.main(["-m", chain, "-i", "in", "-o", tag, "-fit_channels"]) == 0
        for k, (im, mode) in files.items():
            path = str(tmp_path / tag / f"{k}.png")
            with Image.open(path) as o:
                with Image.open(str(tmp_path / "in" / f"{k}.png")) as i:
                    assert o.size == (2 * w, 2 * h) and o.mode == (mode or i.mode), (tag, k, o.mode)
            src = U.read_img(str(tmp_path / "in" / f"{k}.png"))
            want = U.fit_channels_forward(fn, src, dtype=torch.float16) if src.ndim == 2 or src.shape[2] != 3 else U.tensor2np(fn(U.np2tensor(src, dtype=torch.float16)))
            assert np.array_equal(U.read_img(path), want), (tag, k)
    # un-chopped pix2pix (meval=False, normalize=True, images enlarged to a multiple of 256): the alpha plane runs as its own forward
    net = get_network(get_network_G_config("p2p_256", 1))
    shapes = {k: tuple(v.shape) for k, v in net.state_dict().items()}
    torch.save(_sd(shapes, 96), str(tmp_path / "models" / "1x_p2p.pth"))
    for k, arr, mode in (("rgba", synth.image_u8(256, 256, 4, 25), "RGBA"), ("la", synth.image_u8(256, 256, 2, 26), "LA")):
        Image.fromarray(arr, mode).save(str(tmp_path / "in256" / f"{k}.png"))
    assert R.main(["-m", "1x_p2p", "-a", "p2p_256", "-i", "in256", "-o", "out_p2p", "-fit_channels"]) == 0
    mp = R.Model(str(tmp_path / "models" / "1x_p2p.pth"), "p2p_256", 1, meval=False, chop=False)
    for k in ("rgba", "la"):
        src = U.read_img(str(tmp_path / "in256" / f"{k}.png"))
        got = U.read_img(str(tmp_path / "out_p2p" / f"{k}.png"))
        assert got.shape == (256, 256, 4) and np.array_equal(got, mp.run_u8(src, normalize=True, fit_channels=True)), k
    assert sorted(os.listdir(tmp_path / "out_p2p")) == ["la.png", "rgba.png"]
