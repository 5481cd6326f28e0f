"""BasicSR RRDBNet / Real-ESRGAN checkpoints on the HIP engine: the first conv with pixel_unshuffle folded into its addressing
(csrc/conv_first_unshuffle.hip) launch by launch, the scale-2 / scale-1 networks against the reference (G28) and the CPU oracle, Model with chop, and
the 4x form against the same weights under old-arch keys."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _np_sd(shapes, seed=0):
    from innfer_amd import synth
    return {k: torch.from_numpy(v) for k, v in synth.fill_state_dict(shapes, seed).items()}


def _basicsr(sd_old, nb):
    """old-arch state dict -> the same tensors under BasicSR's names."""
    from innfer_amd.architectures.keys import realesrgan_key_map
    return {n + "." + p: sd_old[o + "." + p] for n, o in realesrgan_key_map(nb).items() for p in ("weight", "bias")}


def oracle_realesrgan(sd_old, x, r, nb):
    """BasicSR RRDBNet(scale = 4 // r) on the CPU oracle: reflect pad bottom / right to a multiple of r, unshuffle, the 4x graph, crop."""
    import oracle
    H, W = x.shape[-2:]
    ph, pw = -H % r, -W % r
    xp = F.pad(x, (0, pw, 0, ph), mode="reflect") if ph or pw else x
    s = 4 // r
    with torch.no_grad():
        return oracle.rrdbnet_forward(sd_old, F.pixel_unshuffle(xp, r) if r > 1 else xp, nb=nb, scale=4)[:, :, :s * H, :s * W]


def _codes_within_one(dev, y, ref):
    """fraction of the final uint8 codes (tensor2np) within +-1 of the codes of the fp32 reference output."""
    from innfer_amd.utils import utils as U
    a = U.tensor2np(torch.as_tensor(np.ascontiguousarray(y), dtype=torch.float32).to(dev)).astype(np.int32)
    b = U.tensor2np(torch.as_tensor(np.ascontiguousarray(ref), dtype=torch.float32).to(dev)).astype(np.int32)
    return float((np.abs(a - b) <= 1).mean())


# ------------------------------------------------------------------ the first conv alone
def _first_conv(dev, x, w, b, r, K, act=0, fp32=False, normalize=False):
    """conv3x3(pixel_unshuffle(x, r)) through innfer_first_conv_unshuffle.  x: [N,3,H,W] float16 / float32 tensor or an [H,W,3] uint8 image (cpu).
    Returns (NCHW float32 result on the LR grid, the raw slab(s)) on the cpu; fp32: the (hi, lo) pair of the fp32-accurate mode."""
    import innfer_amd.lib as L
    u8 = x.dtype == torch.uint8
    N, (H, W) = (1, x.shape[:2]) if u8 else (x.shape[0], x.shape[2:])
    h, w_ = -(-H // r), -(-W // r)
    groups = K // 32
    g = N * h * w_ * 32
    lo = groups * g if fp32 else 0
    slab = torch.full(((2 if fp32 else 1), groups, N, h, w_, 32), 7.0, dtype=torch.float16, device=dev)
    d = x.to(dev).contiguous()
    dt = L.U8 if u8 else (L.F32 if x.dtype == torch.float32 else L.F16)
    wc, bc = np.ascontiguousarray(w.numpy(), np.float32), np.ascontiguousarray(b.numpy(), np.float32)
    L.check(L.lib.innfer_first_conv_unshuffle(d.data_ptr(), dt, int(normalize), int(not fp32), N, 3, H, W, r, wc.ctypes.data, bc.ctypes.data, K, act,
                                              slab.data_ptr(), g, lo, None))
    out = torch.empty((N, K, h, w_), dtype=torch.float32, device=dev)
    if fp32:
        L.check(L.lib.innfer_slab_split_to_nchw(slab.data_ptr(), g, lo, 0, out.data_ptr(), N, K, h, w_, None))
    else:
        L.check(L.lib.innfer_slab_to_nchw(slab.data_ptr(), g, 0, out.data_ptr(), L.F32, N, K, h, w_, None))
    torch.cuda.synchronize()
    return out.cpu(), slab.cpu()


def _operands(r, K, N, H, W, seed=0):
    from innfer_amd import synth
    cin = 3 * r * r
    x = torch.from_numpy(synth.uniform((N, 3, H, W), 11 + seed, -1, 1))
    w = torch.from_numpy(synth.uniform((K, cin, 3, 3), 12 + seed, -1, 1)) / np.sqrt(9 * cin)
    b = torch.from_numpy(synth.uniform((K,), 13 + seed, -1, 1))
    return x, w, b


def _ref_conv(x, w, b, r, act, dtype=torch.float32):
    """F.conv2d(F.pixel_unshuffle(x, r), w, b, padding=1) on the same operands (reflect pad bottom / right for ragged sizes)."""
    H, W = x.shape[-2:]
    ph, pw = -H % r, -W % r
    x = x.to(dtype)
    xp = F.pad(x, (0, pw, 0, ph), mode="reflect") if ph or pw else x
    y = F.conv2d(F.pixel_unshuffle(xp, r), w.to(dtype), b.to(dtype), padding=1)
    return F.leaky_relu(y, 0.2) if act == 1 else F.relu(y) if act == 2 else y


# image sizes: LR grids that are not multiples of 16 / 64 columns or 16 rows, one-pixel-high LR grids, several images, ragged sizes (reflect pad)
_SHAPES = {2: [(1, 32, 32), (2, 38, 90), (1, 2, 140), (1, 66, 2), (1, 31, 33), (3, 7, 201)],
           4: [(1, 32, 32), (2, 76, 180), (1, 4, 280), (1, 132, 4), (1, 31, 33), (3, 9, 402)]}


@pytest.mark.parametrize("K", [64, 32])
@pytest.mark.parametrize("r", [2, 4])
def test_first_conv_fp16_vs_conv2d(dev, r, K):
    """Planar fp16 input, fp16 engine: against F.conv2d(F.pixel_unshuffle(x, r), w, b, padding=1) in fp32 on the same (fp16-rounded) input, <= 4e-3
    (the bound of the conv tests of test_gpu_parity.py; measured maximum 9.7e-4: one rounding of O(1) values to fp16)."""
    for i, (N, H, W) in enumerate(_SHAPES[r]):
        act = i % 3
        x, w, b = _operands(r, K, N, H, W, i)
        got, _ = _first_conv(dev, x.half(), w, b, r, K, act=act)
        ref = _ref_conv(x.half().float(), w, b, r, act)
        err = (got - ref).abs().max().item()
        print(f"first conv r={r} K={K} {N}x{H}x{W} act {act} fp16: max|err| {err:.2e}")
        assert got.shape == ref.shape and err <= 4e-3, (r, K, N, H, W, err)


@pytest.mark.parametrize("K", [64, 32])
@pytest.mark.parametrize("r", [2, 4])
def test_first_conv_fp32_mode_vs_float64(dev, r, K):
    """Planar fp32 input, (hi, lo) output of the fp32-accurate mode: against the float64 conv, < 3e-6 -- the bound test_gpu_fp32_mode.py's
    test_split_conv_vs_float64_conv2d applies to the split convs with the same operand scaling (|x| <= 1, |w| <= 1 / sqrt(fan-in)) and up to 1728 terms; this
    conv sums 108 or 432, so no wider bound is needed (measured maximum over these cases: 1.03e-6 for r = 2, 1.71e-6 for r = 4)."""
    for i, (N, H, W) in enumerate(_SHAPES[r]):
        act = (i + 1) % 3
        x, w, b = _operands(r, K, N, H, W, 20 + i)
        got, _ = _first_conv(dev, x, w, b, r, K, act=act, fp32=True)
        ref = _ref_conv(x, w, b, r, act, torch.float64)
        err = (got.double() - ref).abs().max().item()
        print(f"first conv r={r} K={K} {N}x{H}x{W} act {act} fp32 mode: max|err| {err:.2e}")
        assert err < 3e-6, (r, K, N, H, W, err)


@pytest.mark.parametrize("r", [2, 4])
def test_first_conv_uint8_equals_separate_pass(dev, r):
    """uint8 HWC BGR input (np2tensor as the conv's prologue) == innfer_u8hwc_to_nchw followed by the float path, bit for bit, slab for slab: both
    `normalize` settings, the fp16 engine (values rounded to fp16) and the fp32-accurate mode, both widths, a ragged size."""
    import innfer_amd.lib as L
    from innfer_amd import synth
    for (H, W, K) in [(40, 72, 64), (31, 33, 32), (4, 132, 64)]:
        img = torch.from_numpy(synth.image_u8(H, W, 3, 5 + r))
        _, w, b = _operands(r, K, 1, H, W, 40)
        for normalize in (False, True):
            for fp32 in (False, True):
                xf = torch.empty((1, 3, H, W), dtype=torch.float32 if fp32 else torch.float16, device=dev)
                L.check(L.lib.innfer_u8hwc_to_nchw(img.to(dev).data_ptr(), H, W, 3, int(normalize), xf.data_ptr(), L.F32 if fp32 else L.F16, None))
                torch.cuda.synchronize()
                want, want_slab = _first_conv(dev, xf.cpu(), w, b, r, K, act=1, fp32=fp32)
                got, got_slab = _first_conv(dev, img, w, b, r, K, act=1, fp32=fp32, normalize=normalize)
                assert torch.equal(got_slab.view(torch.int16), want_slab.view(torch.int16)), (H, W, K, normalize, fp32)
                ref = _ref_conv(xf.cpu().float(), w, b, r, 1, torch.float64)
                assert (got.double() - ref).abs().max().item() <= (3e-6 if fp32 else 4e-3)


def test_first_conv_refuses_what_is_not_built(dev):
    import innfer_amd.lib as L
    x, w, b = _operands(2, 64, 1, 3, 3)
    with pytest.raises(NotImplementedError, match="reflect-padded"):        # a ragged 3 x 3 image: the pad needs 4 rows / columns
        _first_conv(dev, x.half(), w, b, 2, 64)
    h = C.c_void_p()
    with pytest.raises(NotImplementedError, match="unshuffle"):
        L.check(L.lib.innfer_rrdbnet_create_ex2(C.byref(h), 4, 3, 64, 1, 32, 4, 0, 3, 1, 0, 2))
    with pytest.raises(NotImplementedError, match="unshuffle 3"):
        L.check(L.lib.innfer_rrdbnet_create_ex2(C.byref(h), 3, 3, 64, 1, 32, 4, 0, 3, 1, 0, 3))


# ------------------------------------------------------------------ networks
def _net(dev, r, nb, seed, nf=64):
    from innfer_amd import synth
    from innfer_amd.architectures import get_network
    from innfer_amd.run import infer_from_state_dict
    sd_old = _np_sd(synth.rrdbnet_shapes(in_nc=3 * r * r, nf=nf, nb=nb, scale=4), seed)
    info = infer_from_state_dict({"params_ema": _basicsr(sd_old, nb)})
    assert (info["arch"], info["scale"], info["nb"], info["nf"]) == ("realesrgan", 4 // r, nb, nf)
    net = get_network(info["net_params"])
    net.load_state_dict(info["state_dict"], strict=True)
    return net.to(dev).eval(), sd_old


@pytest.mark.parametrize("r", [2, 4])
def test_network_vs_golden_g28_and_oracle(dev, golden, r):
    """RealESRGANNet (scale 4 // r) against the reference's RRDBNet(in_nc = 3 r^2) behind torch's pixel_unshuffle (G28) and against the CPU oracle: fp16 engine
    <= 1e-2 with >= 99 % of the uint8 codes within +-1, fp32-accurate mode <= 1e-4; an even and a ragged size (reflect pad + crop), C ABI u8 path included."""
    from innfer_amd import synth
    from innfer_amd.utils import utils as U
    g = golden("g28_realesrgan")
    net, sd_old = _net(dev, r, 2, r)
    s = 4 // r
    for name, shape, seed in (("32x32", (1, 3, 32, 32), 280), ("31x33", (1, 3, 31, 33), 290)):
        x = torch.from_numpy(synth.uniform(shape, seed + r))
        want = g[f"r{r}_{name}"]
        ref = oracle_realesrgan(sd_old, x, r, 2).numpy()
        assert np.abs(ref - want).max() <= 2e-6
        y16 = net(x.to(dev).half()).float().cpu().numpy()
        y32 = net(x.to(dev)).cpu().numpy()
        assert y16.shape == y32.shape == want.shape == (1, 3, s * shape[2], s * shape[3])
        e16, e32 = np.abs(y16 - want).max(), np.abs(y32 - want).max()
        print(f"realesrgan r={r} {name}: fp16 max|err| {e16:.2e}, fp32 mode {e32:.2e}")
        assert e16 <= 1e-2 and np.abs(y16 - ref).max() <= 1e-2, e16
        assert _codes_within_one(dev, y16, want) >= 0.99
        assert e32 <= 1e-4 and np.abs(y32 - ref).max() <= 1e-4, e32
        assert net._out_shape(1, shape[2], shape[3], dev) == want.shape
        # out= lands the (cropped) result in the caller's tensor
        buf = torch.empty(want.shape, dtype=torch.float16, device=dev)
        assert net(x.to(dev).half(), out=buf) is buf and np.array_equal(buf.float().cpu().numpy(), y16)
    # a batch of two images, nf 32
    net32, sd32 = _net(dev, r, 1, 7, nf=32)
    xb = torch.from_numpy(synth.uniform((2, 3, 21, 26), 300 + r))
    yb = net32(xb.to(dev).half()).float().cpu()
    assert (yb - oracle_realesrgan(sd32, xb, r, 1)).abs().max().item() <= 1e-2
    # uint8 in, uint8 out through the first / last conv == the separate conversions around the float forward
    img = torch.from_numpy(synth.image_u8(31, 33, 3, r)).to(dev)
    for fp16 in (True, False):
        sep = U.tensor2np(net(U.np2tensor(img.cpu().numpy(), dtype=torch.float16 if fp16 else torch.float32)))
        assert np.array_equal(net.forward_u8(img, fp16=fp16).cpu().numpy(), sep)
    assert net.flops(1, 31, 33) == net.flops(1, 32, 34) > 0 and net.tile_batch_bytes(1, 200) > 0


def test_model_chop_scale2(dev, tmp_path):
    """Model(chop=True) of a wrapped BasicSR checkpoint of scale 2 from a .pth file on a 250 x 330 image: 1x3x500x660, against the oracle run tile by tile
    with the bounds of test_model_chop_golden; run_u8 == tensor2np(Model(np2tensor(img))) bit for bit."""
    import oracle
    from innfer_amd import synth
    from innfer_amd.run import Model
    from innfer_amd.utils import utils as U
    r, nb = 2, 1
    sd_old = _np_sd(synth.rrdbnet_shapes(in_nc=12, nb=nb, scale=4), 21)
    path = str(tmp_path / "x2plus_like.pth")
    torch.save({"params_ema": _basicsr(sd_old, nb)}, path)
    m = Model(path, arch="infer", scale=None, device="cuda", chop=True, tile_batch=4)
    assert (m.arch, m.scale, m.in_nc, m.out_nc) == ("realesrgan", 2, 3, 3)
    x = torch.from_numpy(synth.uniform((1, 3, 250, 330), 42))
    y = m(x.to(dev).half()).float().cpu()
    assert tuple(y.shape) == (1, 3, 500, 660)
    tiles = oracle.extract_patches_2d(x, (200, 200), [0.5, 0.5], batch_first=True).squeeze(0)
    hr = torch.cat([oracle_realesrgan(sd_old, tiles[i:i + 1], r, nb) for i in range(tiles.shape[0])], 0)
    ref = oracle.recompose_tensor(hr, 250, 330, step=0.5, scale=2)
    err = (y - ref).abs().max().item()
    print(f"Model chop scale 2, 250x330: max|err| {err:.2e}")
    assert err < 1e-2
    assert _codes_within_one(dev, y.numpy(), ref.numpy()) >= 0.99
    y32 = m(x.to(dev)).cpu()
    assert (y32 - ref).abs().max().item() <= 1e-4
    img = synth.image_u8(250, 330, 3, 9)
    for fp16 in (True, False):
        assert np.array_equal(m.run_u8(img, fp16=fp16), U.tensor2np(m(U.np2tensor(img, dtype=torch.float16 if fp16 else torch.float32))))
    # un-tiled, a ragged size: reflect-padded inside the first conv, cropped by the shell (a chop tile of odd size cannot be blended: recompose refuses it, as the reference does)
    m2 = Model(path, arch="infer", device="cuda", chop=False)
    xs = torch.from_numpy(synth.uniform((1, 3, 131, 151), 43))
    ys = m2(xs.to(dev).half()).float().cpu()
    assert tuple(ys.shape) == (1, 3, 262, 302) and (ys - oracle_realesrgan(sd_old, xs, r, nb)).abs().max().item() < 1e-2
    imgs = synth.image_u8(131, 151, 3, 10)
    assert np.array_equal(m2.run_u8(imgs), U.tensor2np(m2(U.np2tensor(imgs, dtype=torch.float16))))


def test_scale4_basicsr_keys_equal_old_arch_keys(dev):
    """r = 1: a BasicSR-keyed 4x checkpoint (6 blocks, the anime model's count) runs the engine of today bit for bit -- fp16, fp32 mode and uint8."""
    from innfer_amd import synth
    from innfer_amd.run import Model
    nb = 6
    sd_old = _np_sd(synth.rrdbnet_shapes(nb=nb, scale=4), 31)
    a = Model(None, arch="infer", device="cuda", chop=False, state_dict={"params": _basicsr(sd_old, nb)})
    b = Model(None, arch="infer", device="cuda", chop=False, state_dict=dict(sd_old))
    assert (a.arch, a.scale, b.arch, b.scale) == ("realesrgan", 4, "esrgan", 4)
    x = torch.from_numpy(synth.uniform((1, 3, 40, 56), 32)).to(dev)
    assert torch.equal(a(x.half()), b(x.half())) and torch.equal(a(x), b(x))
    img = synth.image_u8(40, 56, 3, 3)
    assert np.array_equal(a.run_u8(img), b.run_u8(img))
