"""The uint8 chop path against the separate passes, kernel by kernel and bit for bit.  The plain, fit_channels and seamless entry points all launch one
gather and one blend template (csrc/tiles_u8.hip); test_gpu_seamless.py compares that template with itself at two paddings.  These tests anchor it to
kernels that share nothing with it: the whole-image converters (innfer_u8hwc_to_nchw, innfer_nchw_to_u8hwc, innfer_inthwc_to_nchw_fit,
innfer_nchw_to_inthwc_fit) around the float gather and blend (innfer_extract_tiles, innfer_recompose).  Needs an MI355X: `pytest -m gpu`."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

# the padded sizes of test_gpu_seamless.py: one tile row (ps 37, ps 69); a 2 x 2 lattice with a ragged last row and column; width and tile step multiples of 4
SIZES = ((37, 39), (69, 84), (242, 268), (216, 232))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _code(dt):
    from innfer_amd import lib as L
    return L.F16 if dt == torch.float16 else L.F32


def _device_image(img, dev, offset):
    """The HWC image on the device; offset: one pixel into a larger buffer, so that no four-pixel run of it is aligned."""
    if not offset:
        return torch.from_numpy(img).to(dev)
    C = img.shape[2]
    buf = torch.zeros((img.size + C,), dtype=torch.uint8, device=dev)
    buf[C:] = torch.from_numpy(img).to(dev).reshape(-1)
    return buf[C:]


def _tile_buffer(count, C, ps, dt, dev, fill):
    """[count, C, ps, ps] tiles filled with `fill`, with one more tile row of it behind them."""
    buf = torch.full((count * C * ps * ps + ps,), fill, dtype=dt, device=dev)
    return buf, buf[:count * C * ps * ps].view(count, C, ps, ps)


def _float_tiles(planes, h, w, patch, begin, count, ps, fill=-3.0):
    """innfer_extract_tiles of the [C, h, w] float planes."""
    from innfer_amd import lib as L
    _, want = _tile_buffer(count, planes.shape[0], ps, planes.dtype, planes.device, fill)
    L.check(L.lib.innfer_extract_tiles(planes.data_ptr(), _code(planes.dtype), planes.shape[0], h, w, patch, 0.5, begin, count, want.data_ptr(), _stream()))
    return want


def _planes(d, h, w, C, normalize, dt):
    """innfer_u8hwc_to_nchw of the device image."""
    from innfer_amd import lib as L
    x = torch.empty((C, h, w), dtype=dt, device=d.device)
    L.check(L.lib.innfer_u8hwc_to_nchw(d.data_ptr(), h, w, C, int(normalize), x.data_ptr(), _code(dt), _stream()))
    return x


def _gather_u8(d, C, h, w, normalize, dt, patch, begin, count, ps, fit=False, alpha=False):
    """innfer_extract_tiles_u8 / _fit into a sentinel-filled buffer; the tile row behind the tiles must stay as it was."""
    from innfer_amd import lib as L
    slots = (2 if alpha else 1) * count
    buf, got = _tile_buffer(slots, 3 if fit else C, ps, dt, d.device, 7.0)
    head = (d.data_ptr(), C, h, w, int(normalize), patch, 0.5, begin, count)
    tail = (got.data_ptr(), _code(dt), _stream())
    L.check(L.lib.innfer_extract_tiles_u8_fit(*head, int(alpha), *tail) if fit else L.lib.innfer_extract_tiles_u8(*head, *tail))
    assert (buf[got.numel():] == 7.0).all(), "the gather wrote behind its tiles"
    return got


# ------------------------------------------------------------------------------------------------------------------ 1. the gathers
@pytest.mark.parametrize("C", [1, 2, 3, 4, 6])
def test_gather_equals_convert_then_extract(dev, C):
    """innfer_extract_tiles_u8 == innfer_extract_tiles(innfer_u8hwc_to_nchw(img)): the four lattices and a 216 x 232 image that begins one pixel into its
    buffer (no aligned four-pixel run: the per-pixel loads), fp16 and fp32 tiles, normalisation off and on, all tiles and the sub-range from tile 1.
    C = 6 runs the any-channel-count kernel."""
    from innfer_amd import lib as L, synth
    for (h, w), offset in [(sz, False) for sz in SIZES] + [((216, 232), True)]:
        d = _device_image(synth.image_u8(h, w, C, 40 + C), dev, offset)
        ps, ys, xs = L.chop_plan(h, w, 200, 0.5)
        n = len(ys) * len(xs)
        for dt in (torch.float16, torch.float32):
            for normalize in (False, True):
                planes = _planes(d, h, w, C, normalize, dt)
                for begin, count in ((0, n), (1, min(2, n - 1))):
                    got = _gather_u8(d, C, h, w, normalize, dt, 200, begin, count, ps)
                    assert torch.equal(got, _float_tiles(planes, h, w, 200, begin, count, ps)), (h, w, offset, C, dt, normalize, begin, count)


@pytest.mark.parametrize("C", [1, 2, 4])
def test_fit_gather_equals_gather_of_the_explicit_planes(dev, C):
    """innfer_extract_tiles_u8_fit == innfer_extract_tiles_u8 (3 channels) of the (g, g, g) / BGR image in the colour slots and of the (a, a, a) image in
    the alpha slots; alpha tiles off and on."""
    from innfer_amd import lib as L, synth
    for (h, w) in SIZES:
        img = synth.image_u8(h, w, C, 50 + C)
        colour = img[:, :, :3] if C == 4 else np.repeat(img[:, :, :1], 3, axis=2)
        d, dc = torch.from_numpy(img).to(dev), torch.from_numpy(np.ascontiguousarray(colour)).to(dev)
        da = torch.from_numpy(np.ascontiguousarray(np.repeat(img[:, :, C - 1:], 3, axis=2))).to(dev)
        ps, ys, xs = L.chop_plan(h, w, 200, 0.5)
        n = len(ys) * len(xs)
        for dt in (torch.float16, torch.float32):
            for normalize in (False, True):
                for alpha in ((False, True) if C > 1 else (False,)):
                    for begin, count in ((0, n), (1, min(2, n - 1))):
                        tag = (h, w, C, dt, normalize, alpha, begin, count)
                        got = _gather_u8(d, C, h, w, normalize, dt, 200, begin, count, ps, fit=True, alpha=alpha)
                        assert torch.equal(got[:count], _gather_u8(dc, 3, h, w, normalize, dt, 200, begin, count, ps)), tag
                        if alpha:
                            assert torch.equal(got[count:], _gather_u8(da, 3, h, w, normalize, dt, 200, begin, count, ps)), tag


def test_gather_of_more_tiles_than_one_launch_holds(dev):
    """A 2-pixel patch on a 600 x 600 image: 599 x 599 = 358 801 tiles, more than five launch grids of 65 535.  The plain gather and the fit gather with
    alpha tiles (whose slot base is the call's tile count, not the launch's) equal the separate passes over all tiles and from tile 1."""
    from innfer_amd import lib as L, synth
    h = w = 600
    ps, ys, xs = L.chop_plan(h, w, 2, 0.5)
    n = len(ys) * len(xs)
    assert (ps, n) == (2, 599 * 599)
    img = synth.image_u8(h, w, 2, 60)
    d = torch.from_numpy(img).to(dev)
    dt = torch.float16
    for begin, count in ((0, n), (1, n - 1)):
        got = _gather_u8(d, 2, h, w, False, dt, 2, begin, count, ps)
        assert torch.equal(got, _float_tiles(_planes(d, h, w, 2, False, dt), h, w, 2, begin, count, ps)), (begin, count)
        colour, alpha = (torch.empty((3, h, w), dtype=dt, device=dev) for _ in range(2))
        L.check(L.lib.innfer_inthwc_to_nchw_fit(d.data_ptr(), 8, h, w, 2, 0, 255.0, colour.data_ptr(), alpha.data_ptr(), L.F16, _stream()))
        got = _gather_u8(d, 2, h, w, False, dt, 2, begin, count, ps, fit=True, alpha=True)
        assert torch.equal(got[:count], _float_tiles(colour, h, w, 2, begin, count, ps)), (begin, count)
        assert torch.equal(got[count:], _float_tiles(alpha, h, w, 2, begin, count, ps)), (begin, count)


# ------------------------------------------------------------------------------------------------------------------ 2. the blends
def _guarded(nbytes, dev):
    return torch.full((nbytes + 128,), 0xA5, dtype=torch.uint8, device=dev)


def _unguard(buf, shape):
    got = buf.cpu().numpy()
    nbytes = got.size - 128
    assert (got[:64] == 0xA5).all() and (got[64 + nbytes:] == 0xA5).all(), "the blend wrote outside its output"
    return got[64:64 + nbytes].reshape(shape)


def _float_blend(tiles, n, P, height, width, s, via):
    """innfer_recompose of tiles [n, C, P, P] into a [C, s height, s width] tensor of dtype `via`."""
    from innfer_amd import lib as L
    out = torch.empty((tiles.shape[1], s * height, s * width), dtype=via, device=tiles.device)
    L.check(L.lib.innfer_recompose(tiles.data_ptr(), _code(tiles.dtype), n, tiles.shape[1], P, height, width, 0.5, s, out.data_ptr(), _code(via), _stream()))
    return out


def _random_tiles(shape, seed, denormalize, dev):
    from innfer_amd import synth
    base = torch.from_numpy(synth.uniform(shape, seed)).to(dev)
    return (base * 2.4 - 1.2) if denormalize else (base * 1.2 - 0.1)            # some values beyond the clip on both sides


@pytest.mark.parametrize("s", [1, 2, 4])
def test_blend_equals_recompose_then_convert(dev, s):
    """innfer_recompose_u8 == innfer_nchw_to_u8hwc(innfer_recompose(tiles)): the four lattices, 1 / 3 / 4 channels, every tile dtype / via_dtype pair,
    denormalisation off and on, 64 sentinel bytes on both sides of the output."""
    from innfer_amd import lib as L
    for (height, width) in SIZES:
        ps, ys, xs = L.chop_plan(height, width, 200, 0.5)
        n, P = len(ys) * len(xs), ps * s
        FH, FW = s * height, s * width
        for denormalize in (False, True):
            src = _random_tiles((n, 4, P, P), 70 + s, denormalize, dev)
            for C in (1, 3, 4):
                for dt in (torch.float16, torch.float32):
                    tiles = src[:, :C].to(dt).contiguous()
                    for via in (torch.float16, torch.float32):
                        tag = (s, height, width, C, dt, via, denormalize)
                        got = _guarded(FH * FW * C, dev)
                        L.check(L.lib.innfer_recompose_u8(tiles.data_ptr(), _code(dt), n, C, P, height, width, 0.5, s, _code(via), int(denormalize),
                                                          got.data_ptr() + 64, _stream()))
                        want = torch.empty((FH, FW, C), dtype=torch.uint8, device=dev)
                        blended = _float_blend(tiles, n, P, height, width, s, via)
                        L.check(L.lib.innfer_nchw_to_u8hwc(blended.data_ptr(), _code(via), FH, FW, C, int(denormalize), want.data_ptr(), _stream()))
                        assert np.array_equal(_unguard(got, (FH, FW, C)), want.cpu().numpy()), tag


@pytest.mark.parametrize("s", [1, 2, 4])
def test_fit_blend_equals_recompose_then_merge(dev, s):
    """innfer_recompose_u8_fit == innfer_nchw_to_inthwc_fit(innfer_recompose(colour tiles), innfer_recompose(alpha tiles) or the constant alpha): 1 / 2 / 4
    channels, alpha tiles and a constant alpha, the lattices and dtype pairs of the plain blend."""
    from innfer_amd import lib as L
    for (height, width) in SIZES:
        ps, ys, xs = L.chop_plan(height, width, 200, 0.5)
        n, P = len(ys) * len(xs), ps * s
        FH, FW = s * height, s * width
        for denormalize in (False, True):
            src = _random_tiles((2 * n, 3, P, P), 80 + s, denormalize, dev)
            for C in (1, 2, 4):
                for alpha, aconst in (((True, -1), (False, 77)) if C > 1 else ((False, -1),)):
                    for dt in (torch.float16, torch.float32):
                        tiles = src[:(2 if alpha else 1) * n].to(dt).contiguous()
                        for via in (torch.float16, torch.float32):
                            tag = (s, height, width, C, alpha, dt, via, denormalize)
                            got = _guarded(FH * FW * C, dev)
                            L.check(L.lib.innfer_recompose_u8_fit(tiles.data_ptr(), _code(dt), n, P, height, width, 0.5, s, _code(via), int(denormalize), C,
                                                                  int(alpha), aconst, got.data_ptr() + 64, _stream()))
                            colour = _float_blend(tiles[:n], n, P, height, width, s, via)
                            a = _float_blend(tiles[n:], n, P, height, width, s, via) if alpha else None
                            want = torch.empty((FH, FW, C), dtype=torch.uint8, device=dev)
                            L.check(L.lib.innfer_nchw_to_inthwc_fit(colour.data_ptr(), a.data_ptr() if alpha else None, _code(via), FH, FW, C, int(denormalize), 8,
                                                                    aconst, want.data_ptr(), _stream()))
                            assert np.array_equal(_unguard(got, (FH, FW, C)), want.cpu().numpy()), tag
