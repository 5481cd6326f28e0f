"""BasicSR SRVGGNetCompact on the GPU (needs an MI355X: `pytest -m gpu`): the PReLU conv epilogue alone, the shuffle-add tail alone, whole networks, the Model.

1. act 8 (innfer_conv3x3_f16_slope) against float64 conv + PReLU on the operands of tests/_conv_ref.py, within its derived bound (assert_within_fp16_rounding).
2. innfer_shuffle_add against F.pixel_shuffle + F.interpolate('nearest') in torch CPU half, bit for bit; its uint8 ends against innfer_u8hwc_to_nchw /
   innfer_nchw_to_u8hwc, bit for bit.
3. Networks against the float64 forward of tests/_compact_ref.py: max |err| <= 2 x the fp16 storage model's own error on the same case (the engine and the model make
   the same fp16 storage roundings and differ in the fp32 order of summation only), and >= 99 % of the uint8 codes within +-1.
   Measured on the MI355X, engine max |err| / storage model max |err| (100 % of the codes within +-1 in every case):
       num_conv 2 x4 32x32 1.022 | 2 x2 31x33 1.020 | 1 x3 17x9 1.000 | 0 x1 8x8 1.116 | 16 x4 40x56 0.980 | 32 x4 40x56 0.950 | nf 32 batch of two 1.000 |
       nf 24 1.000 | relu 1.000 | leakyrelu 1.000 | Model chop x2 250x330 1.000
   act 8 alone: worst err / bound 0.973 .. 0.996 (e32 5e-8 .. 6.4e-7), the figures of the other fp16 slab stores of tests/test_gpu_conv_forms.py.
4. Model(arch='infer', chop=True) from a .pth under params_ema against the helper run tile by tile; run_u8 and its options against their definitions, bit for bit.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _compact_ref as CR
import _conv_ref as R
from _conv_ref import Case

pytestmark = pytest.mark.gpu

FILL, FILL_U8, GUARD = -3.0, 171, 4096
S24 = [(1, 1, 1), (1, 24, 32), (1, 25, 33), (1, 50, 70), (3, 37, 45)]          # tiles of 24 x 32 (32 outputs)
S16 = [(1, 1, 1), (1, 16, 32), (1, 17, 33), (1, 50, 70), (3, 37, 45)]          # tiles of 16 x 32 (64 outputs)
MANY24, MANY16 = (1, 241, 833), (1, 273, 513)                                  # more tiles than the 256 workgroups: a second tile per workgroup


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


# ------------------------------------------------------------------------------------------------ 1. the PReLU epilogue alone
def _slopes(c):
    """K slopes in [-0.25, 0.75): negative, near-zero and positive ones."""
    from innfer_amd import synth
    return torch.from_numpy(synth.uniform((c.K,), 100 * c.seed + 30, -0.25, 0.75))


def _launch(dev, c, plane_rows=0, slope=True, expect=0, form="3x3", **fields):
    """One launch through innfer_conv3x3_f16_slope with act 8.  The output slab has one foreign group more than the conv writes and lies between guard bands: all of
    that must keep its fill, like everything a refused launch (expect != 0) was given.  Returns [N, K, H, W] fp16 (cpu)."""
    import innfer_amd.lib as L
    lib = L.lib
    x, w, b = R.data(c)
    N, Cc, H, W = x.shape
    xin = R.to_slab(x, Cc // 32 + 1).to(dev)
    wc = np.ascontiguousarray(w.numpy(), dtype=np.float32)
    if form == "1x1":
        packed = np.zeros(lib.innfer_conv1x1_packed_bytes(c.K, Cc), dtype=np.uint8)
        L.check(lib.innfer_pack_conv1x1(np.ascontiguousarray(wc[:, :, 1, 1]).ctypes.data, c.K, Cc, packed.ctypes.data))
    elif fields.get("split"):
        packed = np.zeros(3 * lib.innfer_conv3x3_packed_bytes(c.K, Cc), dtype=np.uint8)
        L.check(lib.innfer_pack_conv3x3_split(wc.ctypes.data, c.K, Cc, packed.ctypes.data))
    else:
        packed = np.zeros(lib.innfer_conv3x3_packed_bytes(c.K, Cc), dtype=np.uint8)
        L.check(lib.innfer_pack_conv3x3_rows(wc.ctypes.data, c.K, Cc, plane_rows, packed.ctypes.data))
    d_packed = torch.from_numpy(packed).to(dev)
    bias = torch.zeros(64); bias[:c.K] = b
    sl = torch.zeros(64); sl[:c.K] = _slopes(c)
    d_bias, d_slope = bias.to(dev), sl.to(dev)
    groups = c.K // 32 + 1
    G = N * H * W * 32
    numel = 2 * groups * G                                        # (room for the lo twin of a split launch, which is refused)
    buf = torch.full((numel + 2 * GUARD,), FILL, dtype=torch.float16, device=dev)
    a = L.ConvArgs()
    a.d_in, a.in_group_stride, a.C = xin.data_ptr(), G, Cc
    a.d_packed, a.d_bias = d_packed.data_ptr(), d_bias.data_ptr()
    a.d_out, a.out_group_stride, a.K = buf.data_ptr() + GUARD * 2, G, c.K
    a.N, a.H, a.W, a.act, a.plane_rows = N, H, W, 8, plane_rows
    a.conv1x1 = int(form == "1x1")
    for k, v in fields.items():
        assert hasattr(a, k), k
        setattr(a, k, v)
    rc = lib.innfer_conv3x3_f16_slope(C.byref(a), d_slope.data_ptr() if slope else None, None)
    torch.cuda.synchronize()
    raw = buf.cpu()
    if expect:
        assert rc == expect, (str(c), fields, rc, L.last_error())
        assert bool((raw == FILL).all()), f"{c}: a refused launch wrote to d_out"
        return None
    assert rc == 0, (str(c), L.last_error())
    assert bool((raw[:GUARD] == FILL).all()) and bool((raw[GUARD + groups * G:] == FILL).all()), f"{c}: wrote outside the output"
    got = R.from_slab(raw[GUARD:GUARD + groups * G].reshape(groups, N, H, W, 32))
    assert bool((got[:, c.K:] == FILL).all()), f"{c}: the foreign group of the slab was written"
    return got[:, :c.K]


def _check_prelu(dev, c, plane_rows, family):
    y64, e32 = R.pre(c)
    a = _slopes(c).double()[None, :, None, None]
    ref = torch.where(y64 >= 0, y64, a * y64)
    got = _launch(dev, c, plane_rows)
    return R.assert_within_fp16_rounding(got, ref, e32, what=f"{c} act 8 plane_rows {plane_rows}", family=family)


@pytest.mark.parametrize("plane_rows", [0, 1])
def test_prelu_epilogue_64_outputs(dev, plane_rows):
    """conv3x3_pc<2, 4, 4, OUT_SLAB, .., 0x10001FF / 0x14001FF>: 64 -> 64, both row orders; ragged edges, a batch, a workgroup's second tile (273 x 513)."""
    for i, (N, H, W) in enumerate(S16 + [MANY16]):
        _check_prelu(dev, Case("3x3", N, 64, 64, H, W, seed=40 + i), plane_rows, f"act 8, 64 outputs, plane_rows {plane_rows}")


def test_prelu_epilogue_32_outputs(dev):
    """conv3x3_pc<3, 2, 4, OUT_SLAB, .., 0x10001FF>: 64 -> 32 on 24 x 32 tiles, 241 x 833 for the second tile."""
    for i, (N, H, W) in enumerate(S24 + [MANY24]):
        _check_prelu(dev, Case("3x3", N, 64, 32, H, W, seed=50 + i), 0, "act 8, 32 outputs")


def test_prelu_epilogue_refusals(dev):
    """act 8 without slopes, or on a form that does not build it, launches nothing: the status, and d_out keeps its fill."""
    import innfer_amd.lib as L
    c = Case("3x3", 1, 64, 64, 17, 33, seed=60)
    _launch(dev, c, slope=False, expect=L.ERR_INVALID)
    _launch(dev, c, form="1x1", expect=L.ERR_UNSUPPORTED)
    _launch(dev, c, out_planar=1, expect=L.ERR_UNSUPPORTED)
    G = 17 * 33 * 32
    _launch(dev, c, split=1, in_lo=3 * G, out_lo=3 * G, expect=L.ERR_UNSUPPORTED)
    _launch(dev, Case("3x3", 1, 64, 16, 17, 33, seed=61), expect=L.ERR_UNSUPPORTED)
    # the plain entry point has no slope argument: act 8 is refused there too
    a = L.ConvArgs(d_in=0x1000, d_packed=0x1000, d_bias=0x1000, d_out=0x1000, C=64, K=64, N=1, H=4, W=4, in_group_stride=512, out_group_stride=512, act=8)
    assert L.lib.innfer_conv3x3_f16(C.byref(a), None) == L.ERR_INVALID and "slope" in L.last_error()


# ------------------------------------------------------------------------------------------------ 2. the tail alone
def _tail(dev, slab_nchw, base, s, Cc, out_dtype, normalize=False):
    """innfer_shuffle_add.  slab_nchw: [N, 32 | 64, H, W] fp16 (every channel random: those beyond Cc s^2 must not matter); base: [N, Cc, H, W] fp16 or
    [N, H, W, Cc] uint8.  Returns the result on the cpu; the output lies between guard bands."""
    import innfer_amd.lib as L
    N, _, H, W = slab_nchw.shape
    sl = R.to_slab(slab_nchw).to(dev)
    d_base = base.to(dev).contiguous()
    tdt = {L.F16: torch.float16, L.F32: torch.float32, L.U8: torch.uint8}[out_dtype]
    fill = FILL_U8 if out_dtype == L.U8 else FILL
    numel = N * Cc * H * s * W * s
    buf = torch.full((numel + 2 * GUARD,), fill, dtype=tdt, device=dev)
    L.check(L.lib.innfer_shuffle_add(sl.data_ptr(), N * H * W * 32, d_base.data_ptr(), L.U8 if base.dtype == torch.uint8 else L.F16, int(normalize),
                                     buf.data_ptr() + GUARD * buf.element_size(), out_dtype, N, Cc, H, W, s, None))
    torch.cuda.synchronize()
    raw = buf.cpu()
    assert bool((raw[:GUARD] == fill).all()) and bool((raw[GUARD + numel:] == fill).all()), "the tail wrote outside its output"
    core = raw[GUARD:GUARD + numel]
    return core.reshape(N, H * s, W * s, Cc) if out_dtype == L.U8 else core.reshape(N, Cc, H * s, W * s)


_TAIL_SHAPES = [(1, 1, 1), (1, 5, 7), (2, 17, 33), (1, 3, 130)]


def _tail_data(s, Cc, N, H, W):
    from innfer_amd import synth
    Kp = 32 if Cc * s * s <= 32 else 64
    seed = 1000 * s + 100 * Cc + H
    slab = torch.from_numpy(synth.uniform((N, Kp, H, W), seed, -1.5, 1.5)).half()
    base = torch.from_numpy(synth.uniform((N, Cc, H, W), seed + 1, -0.25, 1.25)).half()
    return slab, base


@pytest.mark.parametrize("s", [1, 2, 3, 4])
def test_tail_equals_torch_half(dev, s):
    """fp16 and fp32 outputs == F.pixel_shuffle(conv, s) + F.interpolate(x, scale_factor=s, mode='nearest') in torch CPU half, bit for bit."""
    import innfer_amd.lib as L
    for Cc in (1, 3, 4):
        for (N, H, W) in _TAIL_SHAPES:
            slab, base = _tail_data(s, Cc, N, H, W)
            want = F.pixel_shuffle(slab[:, :Cc * s * s], s) + F.interpolate(base, scale_factor=s, mode="nearest")
            assert want.dtype == torch.float16
            got16 = _tail(dev, slab, base, s, Cc, L.F16)
            assert torch.equal(got16.view(torch.int16), want.view(torch.int16)), (s, Cc, N, H, W)
            got32 = _tail(dev, slab, base, s, Cc, L.F32)
            assert torch.equal(got32, want.float()), (s, Cc, N, H, W)


@pytest.mark.parametrize("s", [1, 2, 3, 4])
def test_tail_uint8_ends(dev, s):
    """uint8 output == innfer_nchw_to_u8hwc (tensor2np) of the fp16 result, and a uint8 base == the fp16 base innfer_u8hwc_to_nchw (np2tensor) makes of it: bit for
    bit, both `normalize` settings."""
    import innfer_amd.lib as L
    from innfer_amd import synth
    for Cc in (1, 3, 4):
        for (N, H, W) in _TAIL_SHAPES:
            slab, base = _tail_data(s, Cc, N, H, W)
            img = torch.from_numpy(np.stack([synth.image_u8(H, W, Cc, 7 * n + s) for n in range(N)]))
            for normalize in (False, True):
                b16 = torch.empty((N, Cc, H, W), dtype=torch.float16, device=dev)
                for n in range(N):
                    L.check(L.lib.innfer_u8hwc_to_nchw(img[n].to(dev).contiguous().data_ptr(), H, W, Cc, int(normalize), b16[n].data_ptr(), L.F16, None))
                torch.cuda.synchronize()
                r16 = _tail(dev, slab, b16.cpu(), s, Cc, L.F16)
                assert torch.equal(_tail(dev, slab, img, s, Cc, L.F16, normalize).view(torch.int16), r16.view(torch.int16)), ("u8 base", s, Cc, N, H, W, normalize)
                want = torch.empty((N, H * s, W * s, Cc), dtype=torch.uint8, device=dev)
                d16 = r16.to(dev)
                for n in range(N):
                    L.check(L.lib.innfer_nchw_to_u8hwc(d16[n].data_ptr(), L.F16, H * s, W * s, Cc, int(normalize), want[n].data_ptr(), None))
                torch.cuda.synchronize()
                assert torch.equal(_tail(dev, slab, b16.cpu(), s, Cc, L.U8, normalize), want.cpu()), ("u8 out", s, Cc, N, H, W, normalize)
                assert torch.equal(_tail(dev, slab, img, s, Cc, L.U8, normalize), want.cpu()), ("u8 both", s, Cc, N, H, W, normalize)


def test_tail_refusals(dev):
    import innfer_amd.lib as L
    t = torch.zeros(4096, dtype=torch.float16, device=dev)
    for kw in (dict(C=5), dict(s=5), dict(s=0), dict(C=0)):
        a = dict(C=3, s=2); a.update(kw)
        assert L.lib.innfer_shuffle_add(t.data_ptr(), 32, t.data_ptr(), L.F16, 0, t.data_ptr(), L.F16, 1, a["C"], 1, 1, a["s"], None) == L.ERR_UNSUPPORTED
    assert L.lib.innfer_shuffle_add(t.data_ptr(), 31, t.data_ptr(), L.F16, 0, t.data_ptr(), L.F16, 1, 3, 1, 1, 2, None) == L.ERR_INVALID      # group stride < N H W 32
    assert L.lib.innfer_shuffle_add(t.data_ptr(), 32, t.data_ptr(), L.F32, 0, t.data_ptr(), L.F16, 1, 3, 1, 1, 2, None) == L.ERR_UNSUPPORTED  # fp32 base


# ------------------------------------------------------------------------------------------------ 3. networks
def _net(dev, sd, wrap=True):
    from innfer_amd.architectures import get_network
    from innfer_amd.run import infer_from_state_dict
    info = infer_from_state_dict({"params_ema": sd} if wrap else sd)
    net = get_network(info["net_params"])
    net.load_state_dict(info["state_dict"], strict=True)
    return net.to(dev).eval()


@functools.lru_cache(maxsize=None)
def _case(nf, num_conv, scale, shape, seed):
    """(state dict, input, float64 result, storage-model result) of a case, computed once."""
    from innfer_amd import synth
    sd = CR.fill(3, nf, num_conv, scale, seed=seed)
    x = torch.from_numpy(synth.uniform(shape, 7 + seed))
    return sd, x, CR.forward64(sd, x, num_conv, scale), CR.forward_storage(sd, x, num_conv, scale)


def _assert_like_storage_model(got, y64, ys, what):
    """max |engine - float64| <= 2 x max |storage model - float64| of the same case (computed here), and >= 99 % of the uint8 codes within +-1."""
    err, es = float((got.double() - y64).abs().max()), float((ys - y64).abs().max())
    share = CR.codes_within_one(got, y64)
    print(f"[compact] {what}: engine max|err| {err:.2e}, storage model {es:.2e}, ratio {err / es:.3f}; codes within +-1: {share:.5f}")
    assert got.shape == y64.shape and torch.isfinite(got).all()
    assert err <= 2 * es, (what, err, es)
    assert share >= 0.99, (what, share)


@pytest.mark.parametrize("num_conv,scale,hw", [(2, 4, (32, 32)), (2, 2, (31, 33)), (1, 3, (17, 9)), (0, 1, (8, 8))])
def test_network_vs_float64(dev, num_conv, scale, hw):
    from innfer_amd import synth
    from innfer_amd.utils import utils as U
    sd, x, y64, ys = _case(64, num_conv, scale, (1, 3) + hw, 10 + num_conv)
    net = _net(dev, sd)
    y = net(x.to(dev).half())
    assert y.dtype == torch.float16 and net._out_shape(1, hw[0], hw[1], dev) == tuple(y64.shape) == tuple(y.shape)
    _assert_like_storage_model(y.float().cpu(), y64, ys, f"num_conv {num_conv} x{scale} {hw[0]}x{hw[1]}")
    buf = torch.empty(y.shape, dtype=torch.float16, device=dev)
    assert net(x.to(dev).half(), out=buf) is buf and torch.equal(buf, y)
    img = torch.from_numpy(synth.image_u8(hw[0], hw[1], 3, scale)).to(dev)
    for normalize in (False, True):
        sep = U.tensor2np(net(U.np2tensor(img.cpu().numpy(), normalize=normalize, dtype=torch.float16)), denormalize=normalize)
        assert np.array_equal(net.forward_u8(img, normalize=normalize).cpu().numpy(), sep), normalize
    with pytest.raises(NotImplementedError, match="fp16 mode"):
        net(x.to(dev))
    with pytest.raises(NotImplementedError, match="fp16 mode"):
        net.forward_u8(img, fp16=False)
    assert net.flops(1, *hw) > 0 and net.tile_batch_bytes(2, 16) > 0


@pytest.mark.parametrize("num_conv", [16, 32])
def test_network_depth(dev, num_conv):
    sd, x, y64, ys = _case(64, num_conv, 4, (1, 3, 40, 56), 20 + num_conv)
    y = _net(dev, sd)(x.to(dev).half()).float().cpu()
    _assert_like_storage_model(y, y64, ys, f"num_conv {num_conv} x4 40x56")


def test_network_batch_nf32_and_padded_nf24(dev):
    """A batch of two on 32 features; a 24-feature net == the same weights zero-padded by the test to 32 features, bit for bit."""
    sd, x, y64, ys = _case(32, 2, 2, (2, 3, 21, 26), 31)
    y = _net(dev, sd)(x.to(dev).half()).float().cpu()
    _assert_like_storage_model(y, y64, ys, "nf 32, batch of two, x2 21x26")
    sd24, x, y64, ys = _case(24, 2, 4, (1, 3, 19, 23), 32)
    y24 = _net(dev, sd24)(x.to(dev).half())
    _assert_like_storage_model(y24.float().cpu(), y64, ys, "nf 24 x4 19x23")
    y32 = _net(dev, CR.pad_features(sd24, 2, 32))(x.to(dev).half())
    assert torch.equal(y24, y32)


@pytest.mark.parametrize("act", ["relu", "leakyrelu"])
def test_network_constant_slopes(dev, act):
    """ReLU and LeakyReLU(0.1) nets run the same code path with constant slopes (built by hand: their checkpoints cannot be inferred from the keys)."""
    from innfer_amd import synth
    from innfer_amd.architectures.SRVGG_arch import SRVGGNetCompact
    sd = CR.fill(3, 64, 2, 2, seed=41, act_type=act)
    x = torch.from_numpy(synth.uniform((1, 3, 20, 36), 42))
    net = SRVGGNetCompact(3, 3, 64, 2, 2, act)
    net.load_state_dict(sd, strict=True)
    y = net.to(dev).eval()(x.to(dev).half()).float().cpu()
    _assert_like_storage_model(y, CR.forward64(sd, x, 2, 2, act), CR.forward_storage(sd, x, 2, 2, act), f"{act} x2 20x36")


# ------------------------------------------------------------------------------------------------ 4. the Model
@pytest.fixture(scope="module")
def model(tmp_path_factory):
    from innfer_amd.run import Model
    sd = CR.fill(3, 64, 2, 2, seed=51)
    path = str(tmp_path_factory.mktemp("compact") / "compact_x2.pth")
    torch.save({"params_ema": sd}, path)
    m = Model(path, arch="infer", scale=None, device="cuda", chop=True, tile_batch=4)
    assert (m.arch, m.scale, m.in_nc, m.out_nc) == ("compact", 2, 3, 3)
    return m, sd


def test_model_chop(dev, model):
    """250 x 330 through the chop path against the helper run tile by tile (oracle.extract_patches_2d / recompose_tensor; the storage model's blend rounded to fp16 as
    the chop path's is); run_u8 == the separate conversions; a float32 tensor is refused."""
    import oracle
    from innfer_amd import synth
    from innfer_amd.utils import utils as U
    m, sd = model
    x = torch.from_numpy(synth.uniform((1, 3, 250, 330), 52))
    y = m(x.to(dev).half()).float().cpu()
    assert tuple(y.shape) == (1, 3, 500, 660)
    tiles = oracle.extract_patches_2d(x, (200, 200), [0.5, 0.5], batch_first=True).squeeze(0)
    h64 = torch.cat([CR.forward64(sd, tiles[i:i + 1], 2, 2) for i in range(tiles.shape[0])], 0)
    hs = torch.cat([CR.forward_storage(sd, tiles[i:i + 1], 2, 2) for i in range(tiles.shape[0])], 0)
    y64 = oracle.recompose_tensor(h64, 250, 330, step=0.5, scale=2).double()
    ys = oracle.recompose_tensor(hs, 250, 330, step=0.5, scale=2).half().double()
    _assert_like_storage_model(y, y64, ys, "Model chop x2 250x330")
    img = synth.image_u8(250, 330, 3, 9)
    assert np.array_equal(m.run_u8(img), U.tensor2np(m(U.np2tensor(img, dtype=torch.float16))))
    with pytest.raises(NotImplementedError, match="fp16 mode"):
        m(x.to(dev))


def test_model_run_u8_options(dev, model):
    """tta, seamless='tile', fit_channels on a BGRA image and outscale on a compact model: each equals the definition run_u8's docstring gives for it."""
    from innfer_amd import synth
    from innfer_amd.utils import utils as U
    m, _ = model
    h, w = 40, 56
    img = synth.image_u8(h, w, 3, 61)
    plain = m.run_u8(img)
    assert plain.shape == (2 * h, 2 * w, 3)
    got = m.run_u8(img, tta=True)
    assert np.array_equal(got, U.tensor2np(m.forward_tta(U.np2tensor(img, dtype=torch.float16))))
    got = m.run_u8(img, seamless="tile")
    want = U.tensor2np(m(U.np2tensor(U.seamless_pad_np(img, "tile"), dtype=torch.float16)))[32:-32, 32:-32]
    assert got.shape == plain.shape and np.array_equal(got, want)
    bgra = synth.image_u8(h, w, 4, 62)
    got = m.run_u8(bgra, fit_channels=True)
    assert got.shape == (2 * h, 2 * w, 4) and np.array_equal(got, U.fit_channels_forward(m, bgra, device=dev, dtype=torch.float16))
    got = m.run_u8(img, outscale=2.5)
    assert got.shape == (100, 140, 3) and np.array_equal(got, U.resample_np(plain, 100, 140))
