"""The stitched tile path on the GPU (`-tile N -tile_pad P`; csrc/tiles_stitch.hip, Model.tile_forward, Model.run_u8 under Model(tile=N)).

1. the four kernels alone, bit for bit against torch / numpy slicing built from lib.tile_plan (and the separate conversions np2tensor / tensor2np);
2. no seam: with a halo no smaller than the network's receptive radius the tiled result IS the whole-image result, and with a smaller one it is not;
3. the definition: tile_forward == the batch-1 forwards of the sliced tiles stitched in torch; run_u8 == its docstring with the tiled __call__ inside;
4. 64-bit offsets: more than 2^31 elements in the image, the tile buffer and the result;
5. refusals.
Every comparison is exact.  Needs an MI355X: `pytest -m gpu`."""
import numpy as np
import pytest
import torch

import _compact_ref as CR

pytestmark = pytest.mark.gpu

SIZES = ((50, 77), (41, 23), (48, 64))          # odd widths (no row but the first is aligned), a single tile, and one where every run is aligned
LATTICES = ((32, 8), (16, 4), (16, 0))          # (tile, halo); (16, 0) on 50 x 77 gives P_w = 16: the four-pixel form of the uint8 gather
MODES = ("tile", "mirror", "replicate", "alpha_pad")
PAD = 16
SENTINEL = {torch.float16: 777.0, torch.float32: 777.0, torch.uint8: 0xA5}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _guarded(shape, dtype, dev):
    """(flat buffer with 64 sentinel elements behind the tensor, the tensor): a kernel that writes past its output changes the tail."""
    n = int(np.prod(shape))
    buf = torch.full((n + 64,), SENTINEL[dtype], dtype=dtype, device=dev)
    return buf, buf[:n].view(shape)


def _tail_intact(buf):
    return bool((buf[-64:] == SENTINEL[buf.dtype]).all())


def _rects(H, W, tile, halo, s=1):
    """[(k, oy, ox, r0, r1, c0, c1)]: tile k at origin (oy, ox) owns rows [r0, r1) and columns [c0, c1) of the s H x s W frame -- the owner rule as
    ranges: tile i of an axis owns [o_i + h, o_(i+1) + h), from 0 for the first and to the end for the last."""
    from innfer_amd import lib as L
    ph, pw, ys, xs = L.tile_plan(H, W, tile, halo)

    def spans(org, A):
        lo = [0] + [o + halo for o in org[1:]]
        return list(zip(org, lo, lo[1:] + [A]))
    return ph, pw, [(i * len(xs) + j, s * oy, s * ox, s * r0, s * r1, s * c0, s * c1)
                    for i, (oy, r0, r1) in enumerate(spans(ys, H)) for j, (ox, c0, c1) in enumerate(spans(xs, W))]


def _slice_tiles(x, tile, halo):
    """[n, C, P_h, P_w]: the tiles of x [1, C, H, W] by slicing."""
    ph, pw, rects = _rects(x.shape[2], x.shape[3], tile, halo)
    return torch.stack([x[0, :, oy:oy + ph, ox:ox + pw] for _, oy, ox, *_ in rects])


def _stitch_torch(tiles, H, W, tile, halo, s):
    """[1, C, s H, s W]: every tile's owned rectangle copied out of it."""
    out = torch.empty((1, tiles.shape[1], s * H, s * W), dtype=tiles.dtype, device=tiles.device)
    for k, oy, ox, r0, r1, c0, c1 in _rects(H, W, tile, halo, s)[2]:
        out[0, :, r0:r1, c0:c1] = tiles[k, :, r0 - oy:r1 - oy, c0 - ox:c1 - ox]
    return out


def _gather(x, tile, halo, begin=0, count=None):
    from innfer_amd import lib as L
    from innfer_amd.utils import utils as U
    _, C, H, W = x.shape
    ph, pw, ys, xs = L.tile_plan(H, W, tile, halo)
    count = len(ys) * len(xs) - begin if count is None else count
    buf, tiles = _guarded((count, C, ph, pw), x.dtype, x.device)
    L.check(L.lib.innfer_extract_tiles_rect(x.data_ptr(), U._dt(x), C, H, W, tile, halo, begin, count, buf.data_ptr(), _stream()))
    assert _tail_intact(buf)
    return tiles


def _stitch(tiles, H, W, tile, halo, s):
    from innfer_amd import lib as L
    from innfer_amd.utils import utils as U
    buf, out = _guarded((1, tiles.shape[1], s * H, s * W), tiles.dtype, tiles.device)
    L.check(L.lib.innfer_stitch_tiles(tiles.data_ptr(), U._dt(tiles), tiles.shape[0], tiles.shape[1], H, W, tile, halo, s, out.data_ptr(), _stream()))
    assert _tail_intact(buf)
    return out


def _gather_u8(d, normalize, dt, tile, halo, begin=0, count=None, pad=0, mode="replicate"):
    from innfer_amd import lib as L
    H, W, C = d.shape
    ph, pw, ys, xs = L.tile_plan(H + 2 * pad, W + 2 * pad, tile, halo)
    count = len(ys) * len(xs) - begin if count is None else count
    buf, tiles = _guarded((count, C, ph, pw), dt, d.device)
    L.check(L.lib.innfer_extract_tiles_u8_rect(d.data_ptr(), C, H, W, int(normalize), tile, halo, begin, count, pad, L.BORDER_MODES[mode], buf.data_ptr(),
                                               L.F16 if dt == torch.float16 else L.F32, _stream()))
    assert _tail_intact(buf)
    return tiles


def _stitch_u8(tiles, HP, WP, tile, halo, s, denormalize, crop=0):
    from innfer_amd import lib as L
    from innfer_amd.utils import utils as U
    buf, out = _guarded((s * (HP - 2 * crop), s * (WP - 2 * crop), tiles.shape[1]), torch.uint8, tiles.device)
    L.check(L.lib.innfer_stitch_tiles_u8(tiles.data_ptr(), U._dt(tiles), tiles.shape[0], tiles.shape[1], HP, WP, tile, halo, s, int(denormalize), crop,
                                         out.data_ptr(), _stream()))
    assert _tail_intact(buf)
    return out


def _uniform(shape, seed, dt, dev, lo=-0.25, hi=1.25):
    from innfer_amd import synth
    return torch.from_numpy(synth.uniform(shape, seed, lo, hi)).to(dev).to(dt)


# ------------------------------------------------------------------------------------------------------------------ 1. the kernels alone
@pytest.mark.parametrize("tile,halo", LATTICES)
@pytest.mark.parametrize("hw", SIZES)
def test_tensor_gather_and_stitch_equal_slicing(dev, hw, tile, halo):
    H, W = hw
    for dt in (torch.float16, torch.float32):
        for C in (1, 3, 4, 7):
            x = _uniform((1, C, H, W), 3 * C + H, dt, dev)
            want = _slice_tiles(x, tile, halo)
            n = want.shape[0]
            assert torch.equal(_gather(x, tile, halo), want), (dt, C)
            for begin, count in ((1, n - 1), (n // 2, 1), (n, 0), (0, 0)):                # ranges that do not start at 0; empty ones
                assert torch.equal(_gather(x, tile, halo, begin, count), want[begin:begin + count]), (dt, C, begin, count)
            for s in (1, 2, 3, 4):
                if C == 7 and s > 2:
                    continue
                hr = _uniform((n, C, s * want.shape[2], s * want.shape[3]), 11 * s + C, dt, dev)
                assert torch.equal(_stitch(hr, H, W, tile, halo, s), _stitch_torch(hr, H, W, tile, halo, s)), (dt, C, s)
            assert torch.equal(_stitch(want, H, W, tile, halo, 1), x), (dt, C)             # gather, then stitch at scale 1: the image itself


@pytest.mark.parametrize("tile,halo", LATTICES)
@pytest.mark.parametrize("hw", SIZES)
def test_u8_gather_and_stitch_equal_the_separate_conversions(dev, hw, tile, halo):
    """The uint8 gather == slicing np2tensor(img); the uint8 stitch == tensor2np of the stitched tensor."""
    from innfer_amd import synth
    from innfer_amd.utils import utils as U
    H, W = hw
    for C in (1, 3, 4):
        img = synth.image_u8(H, W, C, 20 + C)
        d = torch.from_numpy(img).to(dev)
        for dt in (torch.float16, torch.float32):
            for normalize in (False, True):
                want = _slice_tiles(U.np2tensor(img, normalize=normalize, device=dev, dtype=dt), tile, halo)
                n = want.shape[0]
                assert torch.equal(_gather_u8(d, normalize, dt, tile, halo), want), (C, dt, normalize)
                assert torch.equal(_gather_u8(d, normalize, dt, tile, halo, n // 2, n - n // 2), want[n // 2:]), (C, dt, normalize)
                for s in (1, 2, 3, 4):
                    lo, hi = (-1.25, 1.25) if normalize else (-0.25, 1.25)                    # values the clip has to catch on both sides
                    hr = _uniform((n, C, s * want.shape[2], s * want.shape[3]), 7 * s + C, dt, dev, lo, hi)
                    ref = U.tensor2np(_stitch_torch(hr, H, W, tile, halo, s), denormalize=normalize)
                    got = _stitch_u8(hr, H, W, tile, halo, s, normalize).cpu().numpy()
                    assert np.array_equal(got, ref), (C, dt, normalize, s)


@pytest.mark.parametrize("mode", MODES)
def test_u8_seamless_forms_equal_the_padded_image_and_the_crop(dev, mode):
    """pad / crop inside the kernels == the same kernels on seamless_pad_np(img) at pad 0, followed by the crop."""
    from innfer_amd import synth
    from innfer_amd.utils import utils as U
    for (H, W) in SIZES[:2]:
        for tile, halo in LATTICES:
            for C in (1, 3, 4):
                img = synth.image_u8(H, W, C, 40 + C)
                padded = U.seamless_pad_np(img, mode)
                HP, WP = padded.shape[:2]
                d, dp = torch.from_numpy(img).to(dev), torch.from_numpy(padded).to(dev)
                for dt, normalize in ((torch.float16, False), (torch.float32, True)):
                    want = _gather_u8(dp, normalize, dt, tile, halo)
                    n = want.shape[0]
                    assert torch.equal(_gather_u8(d, normalize, dt, tile, halo, pad=PAD, mode=mode), want), (H, W, tile, halo, C, dt)
                    assert torch.equal(_gather_u8(d, normalize, dt, tile, halo, 1, n - 1, pad=PAD, mode=mode), want[1:]), (H, W, tile, halo, C, dt)
                    for s in (1, 2, 3):
                        hr = _uniform((n, C, s * want.shape[2], s * want.shape[3]), 5 * s + C, dt, dev)
                        full = _stitch_u8(hr, HP, WP, tile, halo, s, normalize)
                        got = _stitch_u8(hr, HP, WP, tile, halo, s, normalize, crop=PAD)
                        assert got.shape == (s * H, s * W, C) and torch.equal(got, full[s * PAD:-s * PAD, s * PAD:-s * PAD]), (H, W, tile, halo, C, dt, s)


# ------------------------------------------------------------------------------------------------------------------ the models
def _compact_model(tmp_path_factory, **kw):
    """SRVGGNetCompact with num_conv = 2: four 3 x 3 convs, so a receptive radius of 4 low-resolution pixels; 2x."""
    from innfer_amd.run import Model
    path = str(tmp_path_factory.mktemp("tile") / "compact_x2.pth")
    torch.save({"params_ema": CR.fill(3, 64, 2, 2, seed=71)}, path)
    return Model(path, arch="infer", scale=None, device="cuda", **kw)


def _rrdb_model(tmp_path_factory, **kw):
    from innfer_amd import synth
    from innfer_amd.run import Model
    path = str(tmp_path_factory.mktemp("tile") / "2x_rrdb.pth")
    torch.save({k: torch.from_numpy(v) for k, v in synth.fill_state_dict(synth.rrdbnet_shapes(nb=1, scale=2), 72).items()}, path)
    return Model(path, "infer", 2, **kw)


@pytest.fixture(scope="module")
def compact(tmp_path_factory):
    return _compact_model(tmp_path_factory, tile=32, tile_pad=8)


@pytest.fixture(scope="module")
def rrdb(tmp_path_factory):
    return _rrdb_model(tmp_path_factory, tile=32, tile_pad=8)


# ------------------------------------------------------------------------------------------------------------------ 2. no seam
def test_halo_of_the_receptive_radius_leaves_no_seam(dev, compact):
    """70 x 90 at tile 32 + 8 (2 x 3 tiles of 43 x 41): every owned pixel is at least 8 >= 4 pixels from an interior tile edge, so it sees what it sees in
    the whole image -- the tiled result equals the un-tiled forward bit for bit, as tensors and as uint8 images.  With a halo of 2 it must not."""
    from innfer_amd import synth
    m = compact
    x = _uniform((1, 3, 70, 90), 81, torch.float16, dev, 0.0, 1.0)
    whole = m.model(x)
    assert m.tile == 32 and m.tile_pad == 8
    y = m.tile_forward(x)
    assert y.shape == whole.shape and torch.equal(y, whole)
    assert torch.equal(m(x), whole)                                                        # __call__ honours Model(tile=)
    img = torch.from_numpy(synth.image_u8(70, 90, 3, 82)).to(dev)
    whole_u8 = m.model.forward_u8(img)
    assert torch.equal(m.run_u8(img), whole_u8)
    assert np.array_equal(m.run_u8(img.cpu().numpy()), whole_u8.cpu().numpy())
    # teeth: 2 < 4, pixels next to the interior tile edges see the zero padding of the tile instead of the image
    assert not torch.equal(m.tile_forward(x, 32, 2), whole)
    m.tile_pad = 2
    try:
        assert not torch.equal(m.run_u8(img), whole_u8)
    finally:
        m.tile_pad = 8


# ------------------------------------------------------------------------------------------------------------------ 3. the definition
@pytest.mark.parametrize("which", ["rrdb", "compact"])
def test_tile_forward_is_the_stitch_of_the_tiles_forwards(dev, which, rrdb, compact):
    from innfer_amd import synth
    from innfer_amd.utils import utils as U
    m = rrdb if which == "rrdb" else compact
    H, W, s = 70, 90, 2
    x = _uniform((1, 3, H, W), 91, torch.float16, dev, 0.0, 1.0)
    tiles = _slice_tiles(x, 32, 8)
    want = _stitch_torch(torch.cat([m.model(tiles[i:i + 1].contiguous()) for i in range(tiles.shape[0])]), H, W, 32, 8, s)
    try:
        for tb in (1, 3, None):
            m.tile_batch = tb
            assert torch.equal(m.tile_forward(x), want), tb
    finally:
        m.tile_batch = None
    img = synth.image_u8(H, W, 3, 92)
    assert np.array_equal(m.run_u8(img), U.tensor2np(m(U.np2tensor(img, dtype=torch.float16))))
    want = U.tensor2np(m(U.np2tensor(U.seamless_pad_np(img, "tile"), dtype=torch.float16)))[s * PAD:-s * PAD, s * PAD:-s * PAD]
    got = m.run_u8(img, seamless="tile")
    assert got.shape == (s * H, s * W, 3) and np.array_equal(got, want)
    if which == "rrdb":                                                                    # the fp32-accurate engine, normalised
        assert np.array_equal(m.run_u8(img, normalize=True, fp16=False), U.tensor2np(m(U.np2tensor(img, normalize=True)), denormalize=True))


def test_run_u8_options_hold_with_the_tiled_call_inside(dev, rrdb):
    """fit_channels on a BGRA image, tta and outscale: each equals the definition run_u8's docstring gives for it, `self(...)` being tile_forward."""
    from innfer_amd import synth
    from innfer_amd.utils import utils as U
    m = rrdb
    H, W = 40, 56
    img, bgra = synth.image_u8(H, W, 3, 93), synth.image_u8(H, W, 4, 94)
    plain = m.run_u8(img)
    got = m.run_u8(bgra, fit_channels=True)
    assert got.shape == (2 * H, 2 * W, 4) and np.array_equal(got, U.fit_channels_forward(m, bgra, device=dev, dtype=torch.float16))
    assert np.array_equal(m.run_u8(img, tta=True), U.tensor2np(m.forward_tta(U.np2tensor(img, dtype=torch.float16))))
    got = m.run_u8(img, outscale=1.5)
    assert got.shape == (60, 84, 3) and np.array_equal(got, U.resample_np(plain, 60, 84))
    want = U.tensor2np(m.forward_tta(U.np2tensor(U.seamless_pad_np(img, "mirror"), dtype=torch.float16)))[2 * PAD:-2 * PAD, 2 * PAD:-2 * PAD]
    assert np.array_equal(m.run_u8(img, tta=True, seamless="mirror"), want)
    got = m.run_u8(bgra, fit_channels=True, tta=True, outscale=1.5)                        # the three together
    want = U.resample_np(U.fit_channels_forward(m.forward_tta, bgra, device=dev, dtype=torch.float16), 60, 84)
    assert got.shape == (60, 84, 4) and np.array_equal(got, want)


def test_tile_0_is_the_whole_image(dev, tmp_path_factory):
    from innfer_amd import synth
    m0, mw = _rrdb_model(tmp_path_factory, tile=0), _rrdb_model(tmp_path_factory, chop=False)
    x = _uniform((1, 3, 45, 52), 95, torch.float16, dev, 0.0, 1.0)
    assert torch.equal(m0(x), mw(x)) and torch.equal(m0(x), m0.model(x))
    img = synth.image_u8(45, 52, 3, 96)
    assert np.array_equal(m0.run_u8(img), mw.run_u8(img))
    assert np.array_equal(m0.run_u8(img, seamless="replicate"), mw.run_u8(img, seamless="replicate"))
    assert np.array_equal(m0.run_u8(img, tta=True), mw.run_u8(img, tta=True))
    with pytest.raises(ValueError, match="needs a tile size"):
        m0.tile_forward(x)

    def no_room(*a, **k):
        raise torch.OutOfMemoryError("stand-in: the allocator gave up")
    m0._predict = mw._predict = m0.model.forward_u8 = mw.model.forward_u8 = no_room        # an out-of-memory under tile=0 names the way out; chop=False stays as it was
    for call in (lambda m: m(x), lambda m: m.run_u8(img)):
        with pytest.raises(torch.OutOfMemoryError, match="-tile 1024"):
            call(m0)
        with pytest.raises(torch.OutOfMemoryError, match="^stand-in"):
            call(mw)


# ------------------------------------------------------------------------------------------------------------------ 4. 64-bit offsets
def test_offsets_past_2_to_the_31(dev):
    """1 x 3 x 27000 x 27000 fp16 at (8192, 16): 16 tiles of 6774 x 6774, 2.20e9 elements in the tile buffer and 2.19e9 in the image and the result, both
    past 2^31.  Everything is verified on the device."""
    H = W = 27000
    tile, halo = 8192, 16
    ph, pw, rects = _rects(H, W, tile, halo)
    assert (ph, pw, len(rects)) == (6774, 6774, 16) and 3 * H * W > 2 ** 31 and len(rects) * 3 * ph * pw > 2 ** 31
    rows = torch.arange(H, device=dev, dtype=torch.int32).view(H, 1)
    cols = torch.arange(W, device=dev, dtype=torch.int32).view(1, W)
    x = torch.empty((1, 3, H, W), dtype=torch.float16, device=dev)
    for c in range(3):
        x[0, c] = ((rows * 31 + cols * 17 + c * 7) % 2039).to(torch.float16)                # integers below 2048: exact in fp16, no two neighbours alike
    del rows, cols
    tiles = _gather(x, tile, halo)
    for k, oy, ox, *_ in rects:
        assert torch.equal(tiles[k], x[0, :, oy:oy + ph, ox:ox + pw]), k
    out = _stitch(tiles, H, W, tile, halo, 1)
    for k, oy, ox, r0, r1, c0, c1 in rects:
        assert torch.equal(out[0, :, r0:r1, c0:c1], tiles[k, :, r0 - oy:r1 - oy, c0 - ox:c1 - ox]), k
    assert torch.equal(out, x)


# ------------------------------------------------------------------------------------------------------------------ 5. refusals
def test_refusals(dev):
    from innfer_amd import lib as L
    a = torch.zeros(4096, dtype=torch.float16, device=dev)
    b = torch.zeros(4096, dtype=torch.uint8, device=dev)
    p, q, st = a.data_ptr(), b.data_ptr(), _stream()
    with pytest.raises(NotImplementedError, match="output rows"):                          # 80000 output rows
        L.check(L.lib.innfer_stitch_tiles(p, L.F16, 3, 1, 20000, 8, 8192, 16, 4, p, st))
    with pytest.raises(NotImplementedError, match="output rows"):
        L.check(L.lib.innfer_stitch_tiles_u8(p, L.F16, 3, 1, 20000, 8, 8192, 16, 4, 0, 0, q, st))
    with pytest.raises(NotImplementedError, match="tile rows"):                            # one tile of 70000 rows
        L.check(L.lib.innfer_extract_tiles_rect(p, L.F16, 1, 70000, 8, 100000, 0, 0, 1, p, st))
    with pytest.raises(NotImplementedError, match="tile rows"):
        L.check(L.lib.innfer_extract_tiles_u8_rect(q, 1, 70000, 8, 0, 100000, 0, 0, 1, 0, 2, p, L.F16, st))
    for C in (0, 5):                                                                       # the uint8 forms: 1 .. 4 channels
        with pytest.raises(ValueError, match="channels"):
            L.check(L.lib.innfer_extract_tiles_u8_rect(q, C, 20, 20, 0, 16, 0, 0, 1, 0, 2, p, L.F16, st))
        with pytest.raises(ValueError, match="channels"):
            L.check(L.lib.innfer_stitch_tiles_u8(p, L.F16, 4, C, 20, 20, 16, 0, 1, 0, 0, q, st))
    for begin, count in ((-1, 1), (0, 5), (4, 1), (2, -1)):                                # 20 x 20 at (16, 0): 2 x 2 tiles
        with pytest.raises(ValueError, match="tile range"):
            L.check(L.lib.innfer_extract_tiles_rect(p, L.F16, 1, 20, 20, 16, 0, begin, count, p, st))
        with pytest.raises(ValueError, match="tile range"):
            L.check(L.lib.innfer_extract_tiles_u8_rect(q, 1, 20, 20, 0, 16, 0, begin, count, 0, 2, p, L.F16, st))
    for n in (3, 5):
        with pytest.raises(ValueError, match="2x2 tiles expected"):
            L.check(L.lib.innfer_stitch_tiles(p, L.F16, n, 1, 20, 20, 16, 0, 1, p, st))
        with pytest.raises(ValueError, match="2x2 tiles expected"):
            L.check(L.lib.innfer_stitch_tiles_u8(p, L.F16, n, 1, 20, 20, 16, 0, 1, 0, 0, q, st))
    with pytest.raises(ValueError, match="crop"):
        L.check(L.lib.innfer_stitch_tiles_u8(p, L.F16, 4, 1, 20, 20, 16, 0, 1, 0, 10, q, st))
    with pytest.raises(ValueError, match="dtype"):
        L.check(L.lib.innfer_stitch_tiles(p, L.U8, 4, 1, 20, 20, 16, 0, 1, p, st))
    with pytest.raises(ValueError, match="mirror"):
        L.check(L.lib.innfer_extract_tiles_u8_rect(q, 1, 1, 20, 0, 16, 0, 0, 1, 16, L.BORDER_MODES["mirror"], p, L.F16, st))
    with pytest.raises(ValueError):
        L.check(L.lib.innfer_extract_tiles_rect(0, L.F16, 1, 20, 20, 16, 0, 0, 1, p, st))
    torch.cuda.synchronize()
    assert not a.any() and not b.any()                                                     # nothing was launched
