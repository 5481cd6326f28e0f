"""SPAN on the GPU (needs an MI355X: `pytest -m gpu`): the SiLU and gate conv epilogues alone, the first conv's input map, the PixelShuffle tail, whole networks, the Model.

1. act 9 / act 10 (innfer_conv3x3_f16) against float64 on the operands of tests/_conv_ref.py, within its derived bound (assert_within_fp16_rounding).  extra:
   act 9, f sigmoid(f): one hardware sigmoid (TRANS absolute) times |f|;  act 10, (f + res)(sigmoid(f) - 0.5) computed as (f + res) tanh(f / 2) / 2: the hardware tanh
   is TRANS absolute, halved, times |f + res| -- so |f + res| TRANS holds with room.  64 outputs in both row orders and 32 outputs; ragged tile edges, a batch, a
   workgroup's second tile; a row range with out_ch_off; guard bands and a foreign slab group that keep their fill; the refusals (status, nothing written).
2. The first conv's input map (innfer_first_conv_map) on fp16 and uint8 input against float64 on the mapped fp16 operand (border ring included: the padding is zero
   AFTER the map), within tests/_first_conv_ref.py's store bound; without a map the launch is innfer_first_conv's, bit for bit.
3. innfer_shuffle_add with a NULL base against F.pixel_shuffle in torch half, bit for bit, scales 1 .. 4; the uint8 end against innfer_nchw_to_u8hwc.
4. Networks against the float64 forward of tests/_span_ref.py: max |err| <= 2 x the fp16 storage model's own error on the same case and >= 99 % of the uint8 codes
   within +-1 (tests/test_span_host.py verifies the storage model alone on the CPU); <= 24 launches per forward.
   Measured on the MI355X, engine max |err| / storage model max |err| (100 % of the codes within +-1 in every case):
       f 48 x4 32x32 1.173 | f 48 x2 31x33 0.973 | f 52 x3 17x9 0.876 | f 32 x1 8x8 1.081 | batch of two 0.936 | norm=False 1.007 | deploy 0.973 |
       Model chop x4 250x330 0.960
   act 9 alone: worst err / bound 0.948 .. 0.993, act 10: 0.958 .. 0.987 (e32 3e-8 .. 6.5e-7); the first conv behind its map: 0.78 .. 0.84, the border ring no worse.
5. Model(arch='infer', chop=True) from a .pth under params_ema against the helper run tile by tile; run_u8 and its options against their definitions, bit for bit.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _conv_ref as R
import _first_conv_ref as FR
import _span_ref as SR
from _conv_ref import Case

pytestmark = pytest.mark.gpu

FILL, FILL_U8, GUARD = -3.0, 171, 4096
S16 = [(1, 1, 1), (1, 16, 32), (1, 17, 33), (1, 50, 70), (3, 37, 45)]          # the 16 x 32-tile edges (64 outputs)
MANY16 = (1, 273, 513)                                                         # more tiles than the 256 workgroups: a second tile per workgroup
S24 = [(1, 1, 1), (1, 24, 32), (1, 25, 33), (1, 50, 70), (3, 37, 45)]          # tiles of 24 x 32 (32 outputs)
MANY24 = (1, 241, 833)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


# ------------------------------------------------------------------------------------------------ 1. the two epilogues alone
def _launch(dev, c, act, plane_rows=0, res=True, expect=0, form="3x3", off=0, **fields):
    """One launch through innfer_conv3x3_f16 with act 9 / 10 (act 10: d_res1 = R.residual(c, 1) as a slab of its own).  The output slab has `off` channels in front of
    the conv's and one foreign group behind them and lies between guard bands: all of that must keep its fill, like everything a refused launch (expect != 0) was
    given.  Returns [N, K, H, W] fp16 (cpu) -- rows outside a row range still hold FILL."""
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
    d_bias = bias.to(dev)
    Kg = max(c.K, 32)
    r1 = torch.zeros((N, Kg, H, W), dtype=torch.float16)
    r1[:, :c.K] = R.residual(c, 1, (N, c.K, H, W))
    d_res = R.to_slab(r1).to(dev)
    groups = (off + c.K + 31) // 32 + 1
    G = N * H * W * 32
    numel = 2 * groups * G                                        # (room for the lo twin of a split launch, which is refused)
    buf = torch.full((numel + 2 * GUARD,), FILL, dtype=torch.float16, device=dev)
    keep = []
    a = L.ConvArgs()
    a.d_in, a.in_group_stride, a.C = xin.data_ptr(), G, Cc
    a.d_packed, a.d_bias = d_packed.data_ptr(), d_bias.data_ptr()
    a.d_out, a.out_group_stride, a.K, a.out_ch_off = buf.data_ptr() + GUARD * 2, G, c.K, off
    a.N, a.H, a.W, a.act, a.plane_rows = N, H, W, act, plane_rows
    a.conv1x1 = int(form == "1x1")
    if res:
        a.d_res1, a.res1_group_stride, a.res1_scale = d_res.data_ptr(), G, 1.0
    for k, v in fields.items():
        assert hasattr(a, k), k
        if k == "d_stats_part":
            n = N * lib.innfer_conv_stats_records(H, W, 1) * c.K * 3
            keep.append(torch.zeros(n, dtype=torch.float32, device=dev))
            a.d_stats_part, a.stats_part_floats = keep[-1].data_ptr(), n
        else:
            setattr(a, k, v)
    rc = lib.innfer_conv3x3_f16(C.byref(a), None)
    torch.cuda.synchronize()
    raw = buf.cpu()
    if expect:
        assert rc == expect, (str(c), act, fields, rc, L.last_error())
        assert bool((raw == FILL).all()), f"{c}: a refused launch wrote to d_out"
        return None
    assert rc == 0, (str(c), L.last_error())
    assert bool((raw[:GUARD] == FILL).all()) and bool((raw[GUARD + groups * G:] == FILL).all()), f"{c}: wrote outside the output"
    got = R.from_slab(raw[GUARD:GUARD + groups * G].reshape(groups, N, H, W, 32))
    assert bool((got[:, :off] == FILL).all()) and bool((got[:, off + c.K:] == FILL).all()), f"{c}: channels beside the conv's were written"
    return got[:, off:off + c.K]


def _ref(c, act):
    """(float64 reference, e32, extra) of the epilogue on the case's float64 conv + bias."""
    y64, e32 = R.pre(c)
    if act == 9:
        return y64 * torch.sigmoid(y64), e32, y64.abs() * R.TRANS
    r = R.residual(c, 1, y64.shape).double()
    return (y64 + r) * (torch.sigmoid(y64) - 0.5), e32, (y64 + r).abs() * R.TRANS


def _check(dev, c, act, plane_rows, family):
    ref, e32, extra = _ref(c, act)
    got = _launch(dev, c, act, plane_rows, res=act == 10)
    return R.assert_within_fp16_rounding(got, ref, e32, extra=extra, what=f"{c} act {act} plane_rows {plane_rows}", family=family)


@pytest.mark.parametrize("plane_rows", [0, 1])
@pytest.mark.parametrize("act", [9, 10])
def test_span_epilogues_64_outputs(dev, act, plane_rows):
    """conv3x3_pc<2, 4, 4, OUT_SLAB, .., TAPS_3X3 [| PC_ROWP] | PC_SPAN>: 64 -> 64, both row orders; ragged edges, a batch, a workgroup's second tile (273 x 513)."""
    for i, (N, H, W) in enumerate(S16 + [MANY16]):
        _check(dev, Case("3x3", N, 64, 64, H, W, seed=70 + i), act, plane_rows, f"act {act}, 64 outputs, plane_rows {plane_rows}")


@pytest.mark.parametrize("act", [9, 10])
def test_span_epilogues_32_outputs(dev, act):
    """conv3x3_pc<3, 2, 4, OUT_SLAB, .., TAPS_3X3 | PC_SPAN>: 64 -> 32 on 24 x 32 tiles, 241 x 833 for the second tile."""
    for i, (N, H, W) in enumerate(S24 + [MANY24]):
        _check(dev, Case("3x3", N, 64, 32, H, W, seed=80 + i), act, 0, f"act {act}, 32 outputs")


@pytest.mark.parametrize("act", [9, 10])
def test_span_epilogues_row_range_and_channel_offset(dev, act):
    """A batch of two, rows [5, 30) only, written at out_ch_off 32 (32 outputs) / 64 (64 outputs): the rows outside the range and the channels in front keep their fill."""
    for K, off in ((32, 32), (64, 64)):
        c = Case("3x3", 2, 64, K, 37, 45, seed=90 + K)
        ref, e32, extra = _ref(c, act)
        got = _launch(dev, c, act, int(K == 64), res=act == 10, off=off, row_begin=5, row_end=30)
        assert bool((got[:, :, :5] == FILL).all()) and bool((got[:, :, 30:] == FILL).all()), "rows outside the range were written"
        R.assert_within_fp16_rounding(got[:, :, 5:30], ref[:, :, 5:30], e32, extra=extra[:, :, 5:30], what=f"{c} act {act} rows 5..30 off {off}", family=f"act {act}, row range")


def test_span_epilogue_refusals(dev):
    """act 10 without d_res1 is INVALID; act 9 / 10 on a form that does not build them is UNSUPPORTED; nothing is launched: d_out keeps its fill."""
    import innfer_amd.lib as L
    c = Case("3x3", 1, 64, 64, 16, 32, seed=95)
    G = 16 * 32 * 32
    _launch(dev, c, 10, res=False, expect=L.ERR_INVALID)
    for act in (9, 10):
        r = act == 10
        _launch(dev, c, act, res=r, form="1x1", expect=L.ERR_UNSUPPORTED)
        _launch(dev, c, act, res=r, out_planar=1, expect=L.ERR_UNSUPPORTED)
        _launch(dev, c, act, res=r, split=1, in_lo=3 * G, out_lo=3 * G, res1_lo=3 * G, expect=L.ERR_UNSUPPORTED)
        _launch(dev, c, act, res=False, d_stats_part=1, expect=L.ERR_UNSUPPORTED)
        _launch(dev, c, act, res=False, stride2_k4=1, expect=L.ERR_UNSUPPORTED)
        _launch(dev, c, act, res=False, transposed2x=4, expect=L.ERR_UNSUPPORTED)
        _launch(dev, c, act, res=r, upsample2x=1, expect=L.ERR_UNSUPPORTED)
        _launch(dev, c, act, res=r, reflect_pad=1, expect=L.ERR_UNSUPPORTED)
        _launch(dev, Case("3x3", 1, 64, 32, 16, 32, seed=96), act, res=r, dilation=2, expect=L.ERR_UNSUPPORTED)
        _launch(dev, Case("3x3", 1, 64, 16, 16, 32, seed=97), act, res=r, expect=L.ERR_UNSUPPORTED)
    _launch(dev, c, 9, res=True, expect=L.ERR_UNSUPPORTED)          # SiLU takes no residual


# ------------------------------------------------------------------------------------------------ 2. the first conv's input map
def _first(dev, x, w, b, K, alpha, shift, u8=False, fp16_mode=1, mapped=True):
    """innfer_first_conv_map (mapped) / innfer_first_conv into a guarded slab; x: [N, C, H, W] fp16 or [N, H, W, C] uint8.  Returns [N, K, H, W] fp16 (cpu)."""
    import innfer_amd.lib as L
    N, Cc, H, W = (x.shape[0], x.shape[3], x.shape[1], x.shape[2]) if u8 else x.shape
    d_in = x.to(dev).contiguous()
    G = N * H * W * 32
    groups = K // 32 + 1
    buf = torch.full((groups * G + 2 * GUARD,), FILL, dtype=torch.float16, device=dev)
    wc, bc = np.ascontiguousarray(w, np.float32), np.ascontiguousarray(b, np.float32)
    if mapped:
        al = None if alpha is None else np.ascontiguousarray(alpha, np.float32)
        sh = None if shift is None else np.ascontiguousarray(shift, np.float32)
        L.check(L.lib.innfer_first_conv_map(d_in.data_ptr(), L.U8 if u8 else L.F16, 0, fp16_mode, N, Cc, H, W, wc.ctypes.data, bc.ctypes.data, K, 0,
                                            None if al is None else al.ctypes.data, None if sh is None else sh.ctypes.data, buf.data_ptr() + 2 * GUARD, G, None))
    else:
        L.check(L.lib.innfer_first_conv(d_in.data_ptr(), L.U8 if u8 else L.F16, 0, fp16_mode, N, Cc, H, W, wc.ctypes.data, bc.ctypes.data, K, 0, None,
                                        buf.data_ptr() + 2 * GUARD, G, 0, None, 0, 0, None))
    torch.cuda.synchronize()
    raw = buf.cpu()
    assert bool((raw[:GUARD] == FILL).all()) and bool((raw[GUARD + groups * G:] == FILL).all()), "the first conv wrote outside its output"
    got = R.from_slab(raw[GUARD:GUARD + groups * G].reshape(groups, N, H, W, 32))
    assert bool((got[:, K:] == FILL).all()), "the foreign group of the slab was written"
    return got[:, :K]


def _mapped_operand(v32, alpha, shift):
    """fp16(fma(alpha[c], v, shift[c])) as float32: the product of two float32 is exact in float64, the sum is rounded to float32 once (the fma), then to fp16."""
    a = np.asarray(alpha, np.float32).astype(np.float64)[None, :, None, None]
    s = np.asarray(shift, np.float32).astype(np.float64)[None, :, None, None]
    return (a * v32.astype(np.float64) + s).astype(np.float32).astype(np.float16).astype(np.float32)


@pytest.mark.parametrize("K", [64, 32])
@pytest.mark.parametrize("shape", [(1, 17, 33), (3, 20, 70)])
def test_first_conv_input_map(dev, K, shape):
    """SPAN's map (alpha 255, shift -255 mean) on an fp16 tensor and on a uint8 image (np2tensor's 1 / 255 in fp32: code - 255 mean in one rounding with fp16_mode 0;
    the network's own form, fp16_mode 1, rounds code / 255 to fp16 first like the tensor path) against float64 on the mapped operand."""
    from innfer_amd import synth
    N, H, W = shape
    w = synth.uniform((K, 3, 3, 3), 300 + K, -1, 1) / np.float32(np.sqrt(27.0) * 64)
    b = synth.uniform((K,), 301 + K, -1, 1)
    alpha = np.full(3, 255.0, np.float32)
    shift = (-np.asarray(SR.MEAN, np.float32) * np.float32(255.0)).astype(np.float32)
    x16 = synth.uniform((N, 3, H, W), 302 + H).astype(np.float16)
    img = FR.u8_images(N, H, W, 3, seed=5)
    cases = [("fp16", torch.from_numpy(x16), False, 1, x16.astype(np.float32))]
    for mode in (0, 1):
        cases.append((f"uint8 fp16_mode {mode}", torch.from_numpy(img), True, mode, FR.np2tensor_np(img, False, bool(mode))))
    for what, x, u8, mode, v32 in cases:
        op = _mapped_operand(v32, alpha, shift)
        if u8 and mode == 0:          # one rounding of code - 255 mean (the quotient's own fp32 rounding moves the fp16 result on a handful of ties at most)
            flip = img[..., ::-1].transpose(0, 3, 1, 2).astype(np.float64)
            direct = (flip + shift.astype(np.float64)[None, :, None, None]).astype(np.float16).astype(np.float32)
            assert float(np.mean(op != direct)) < 1e-3 and float(np.abs(op - direct).max()) <= float(FR.ulp16(np.abs(direct)).max())
        ref = FR.conv_ref(op, w, b, 0)
        e = FR.data_e(op, w, b, 0)
        got = _first(dev, x, w, b, K, alpha, shift, u8, mode).numpy().astype(np.float64)
        ratio = np.abs(got - ref) / FR.store_bound(ref, got, e)
        print(f"[span] first conv map K {K} {shape} {what}: e {e:.2e} worst err/bound {ratio.max():.3f} (ring {np.concatenate([ratio[:, :, 0].ravel(), ratio[:, :, -1].ravel(), ratio[:, :, :, 0].ravel(), ratio[:, :, :, -1].ravel()]).max():.3f})")
        assert ratio.max() <= 1.0, (what, K, shape, float(ratio.max()))
    # no map: innfer_first_conv's launch, bit for bit
    a = _first(dev, torch.from_numpy(x16), w, b, K, None, None)
    assert torch.equal(a.view(torch.int16), _first(dev, torch.from_numpy(x16), w, b, K, None, None, mapped=False).view(torch.int16))
    a = _first(dev, torch.from_numpy(img), w, b, K, None, None, u8=True)
    assert torch.equal(a.view(torch.int16), _first(dev, torch.from_numpy(img), w, b, K, None, None, u8=True, mapped=False).view(torch.int16))


# ------------------------------------------------------------------------------------------------ 3. the tail without a base
def _shuffle(dev, slab_nchw, s, Cc, out_dtype):
    import innfer_amd.lib as L
    N, _, H, W = slab_nchw.shape
    sl = R.to_slab(slab_nchw).to(dev)
    tdt = {L.F16: torch.float16, L.F32: torch.float32, L.U8: torch.uint8}[out_dtype]
    fill = FILL_U8 if out_dtype == L.U8 else FILL
    numel = N * Cc * H * s * W * s
    buf = torch.full((numel + 2 * GUARD,), fill, dtype=tdt, device=dev)
    L.check(L.lib.innfer_shuffle_add(sl.data_ptr(), N * H * W * 32, None, L.F16, 0, buf.data_ptr() + GUARD * buf.element_size(), out_dtype, N, Cc, H, W, s, None))
    torch.cuda.synchronize()
    raw = buf.cpu()
    assert bool((raw[:GUARD] == fill).all()) and bool((raw[GUARD + numel:] == fill).all()), "the tail wrote outside its output"
    core = raw[GUARD:GUARD + numel]
    return core.reshape(N, H * s, W * s, Cc) if out_dtype == L.U8 else core.reshape(N, Cc, H * s, W * s)


@pytest.mark.parametrize("s", [1, 2, 3, 4])
def test_shuffle_without_base(dev, s):
    """fp16 / fp32 outputs == F.pixel_shuffle in torch half, bit for bit; the uint8 output == innfer_nchw_to_u8hwc (tensor2np) of that."""
    import innfer_amd.lib as L
    from innfer_amd import synth
    for Cc in (1, 3, 4):
        for (N, H, W) in [(1, 1, 1), (1, 5, 7), (2, 17, 33), (1, 3, 130)]:
            Kp = 32 if Cc * s * s <= 32 else 64
            slab = torch.from_numpy(synth.uniform((N, Kp, H, W), 2000 * s + 100 * Cc + H, -0.5, 1.5)).half()
            want = F.pixel_shuffle(slab[:, :Cc * s * s], s)
            assert torch.equal(_shuffle(dev, slab, s, Cc, L.F16).view(torch.int16), want.view(torch.int16)), (s, Cc, N, H, W)
            assert torch.equal(_shuffle(dev, slab, s, Cc, L.F32), want.float()), (s, Cc, N, H, W)
            u8 = torch.empty((N, H * s, W * s, Cc), dtype=torch.uint8, device=dev)
            d16 = want.to(dev).contiguous()
            for n in range(N):
                L.check(L.lib.innfer_nchw_to_u8hwc(d16[n].data_ptr(), L.F16, H * s, W * s, Cc, 0, u8[n].data_ptr(), None))
            torch.cuda.synchronize()
            assert torch.equal(_shuffle(dev, slab, s, Cc, L.U8), u8.cpu()), ("u8", s, Cc, N, H, W)


# ------------------------------------------------------------------------------------------------ 4. networks
def _net(dev, sd, wrap=True):
    from innfer_amd.architectures import get_network
    from innfer_amd.run import infer_from_state_dict
    info = infer_from_state_dict({"params_ema": sd} if wrap else sd)
    net = get_network(info["net_params"])
    net.load_state_dict(info["state_dict"], strict=True)
    return net.to(dev).eval()


@functools.lru_cache(maxsize=None)
def _case(f, scale, shape, seed, norm=True, deploy=False):
    """(state dict, input, float64 result, storage-model result) of a case, computed once."""
    from innfer_amd import synth
    sd = SR.fill(3, f, scale, seed, norm, deploy)
    x = torch.from_numpy(synth.uniform(shape, 7 + seed))
    return sd, x, SR.forward64(sd, x, scale, norm), SR.forward_storage(sd, x, scale, norm)


def _assert_like_storage_model(got, y64, ys, what):
    """max |engine - float64| <= 2 x max |storage model - float64| of the same case (computed here), and >= 99 % of the uint8 codes within +-1."""
    err, es = float((got.double() - y64).abs().max()), float((ys - y64).abs().max())
    share = SR.codes_within_one(got, y64)
    print(f"[span] {what}: engine max|err| {err:.2e}, storage model {es:.2e}, ratio {err / es:.3f}; codes within +-1: {share:.5f}")
    assert got.shape == y64.shape and torch.isfinite(got).all()
    assert err <= 2 * es, (what, err, es)
    assert share >= 0.99, (what, share)


def _launches(net, x):
    """Launch count of one forward (innfer_net_forward_timed)."""
    import innfer_amd.lib as L
    N, _, H, W = x.shape
    s = L.lib.innfer_net_scale(net._handle)
    out = torch.empty((N, net.out_nc, H * s, W * s), dtype=torch.float16, device=x.device)
    ws = torch.empty(L.lib.innfer_net_workspace_bytes(net._handle, N, H, W), dtype=torch.uint8, device=x.device)
    n = C.c_int()
    ms = (C.c_float * 64)()
    L.check(L.lib.innfer_net_forward_timed(net._handle, x.data_ptr(), L.F16, out.data_ptr(), L.F16, N, H, W, ws.data_ptr(), ws.numel(), None, 64, ms, None, None, None, C.byref(n)))
    return n.value, out


@pytest.mark.parametrize("f,scale,hw,seed", [(48, 4, (32, 32), 1), (48, 2, (31, 33), 2), (52, 3, (17, 9), 3), (32, 1, (8, 8), 4)])
def test_network_vs_float64(dev, f, scale, hw, seed):
    from innfer_amd import synth
    from innfer_amd.utils import utils as U
    sd, x, y64, ys = _case(f, scale, (1, 3) + hw, seed)
    net = _net(dev, sd)
    xd = x.to(dev).half()
    y = net(xd)
    assert y.dtype == torch.float16 and net._out_shape(1, hw[0], hw[1], dev) == tuple(y64.shape) == tuple(y.shape)
    _assert_like_storage_model(y.float().cpu(), y64, ys, f"f {f} x{scale} {hw[0]}x{hw[1]}")
    buf = torch.empty(y.shape, dtype=torch.float16, device=dev)
    assert net(xd, out=buf) is buf and torch.equal(buf, y)
    n, yt = _launches(net, xd)
    assert n <= 24 and torch.equal(yt, y), n
    img = torch.from_numpy(synth.image_u8(hw[0], hw[1], 3, scale)).to(dev)
    sep = U.tensor2np(net(U.np2tensor(img.cpu().numpy(), dtype=torch.float16)))
    assert np.array_equal(net.forward_u8(img).cpu().numpy(), sep)
    with pytest.raises(NotImplementedError, match="fp16 mode"):
        net(x.to(dev))
    with pytest.raises(NotImplementedError, match="fp16 mode"):
        net.forward_u8(img, fp16=False)
    assert net.flops(1, *hw) > 0 and net.tile_batch_bytes(2, 16) > 0


def test_network_batch_of_two(dev):
    sd, x, y64, ys = _case(48, 2, (2, 3, 21, 26), 6)
    y = _net(dev, sd)(x.to(dev).half()).float().cpu()
    _assert_like_storage_model(y, y64, ys, "f 48, batch of two, x2 21x26")


def test_network_no_norm_and_deploy(dev):
    """norm=False (the `no_norm` buffer; conv_1 without an input map) and a `deploy` checkpoint (eval_conv.* used as given) == the full checkpoint it was collapsed from
    to the fp32 rounding of the collapse (the same case: the same bound)."""
    sd, x, y64, ys = _case(48, 2, (1, 3, 20, 24), 5, False)
    net = _net(dev, sd)
    assert not net.norm and "no_norm" in net.state_dict()
    _assert_like_storage_model(net(x.to(dev).half()).float().cpu(), y64, ys, "norm=False f 48 x2 20x24")
    sd, x, y64, ys = _case(48, 2, (1, 3, 31, 33), 2, True, True)
    net = _net(dev, sd)
    assert net.deploy and not any(".sk." in k for k in net.state_dict())
    _assert_like_storage_model(net(x.to(dev).half()).float().cpu(), y64, ys, "deploy f 48 x2 31x33")
    # the stored eval_conv.* of a full checkpoint is noise in the fixture: a result that used it would miss the reference altogether (covered by every case above)


# ------------------------------------------------------------------------------------------------ 5. the Model
@pytest.fixture(scope="module")
def model(tmp_path_factory):
    from innfer_amd.run import Model
    sd = SR.fill(3, 48, 4, seed=8)
    path = str(tmp_path_factory.mktemp("span") / "4x_span.pth")
    torch.save({"params_ema": sd}, path)
    m = Model(path, arch="infer", scale=None, device="cuda", chop=True, tile_batch=4)
    assert (m.arch, m.scale, m.in_nc, m.out_nc) == ("span", 4, 3, 3)
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
    assert tuple(y.shape) == (1, 3, 1000, 1320)
    tiles = oracle.extract_patches_2d(x, (200, 200), [0.5, 0.5], batch_first=True).squeeze(0)
    h64 = torch.cat([SR.forward64(sd, tiles[i:i + 1], 4) for i in range(tiles.shape[0])], 0)
    hs = torch.cat([SR.forward_storage(sd, tiles[i:i + 1], 4) for i in range(tiles.shape[0])], 0)
    y64 = oracle.recompose_tensor(h64, 250, 330, step=0.5, scale=4).double()
    ys = oracle.recompose_tensor(hs, 250, 330, step=0.5, scale=4).half().double()
    _assert_like_storage_model(y, y64, ys, "Model chop x4 250x330")
    img = synth.image_u8(250, 330, 3, 9)
    assert np.array_equal(m.run_u8(img), U.tensor2np(m(U.np2tensor(img, dtype=torch.float16))))
    with pytest.raises(NotImplementedError, match="fp16 mode"):
        m(x.to(dev))


def test_model_run_u8_options(dev, model):
    """plain, tile=, tta, seamless='tile' and run_u8_batch on a SPAN model: each equals the definition its docstring gives for it, bit for bit (images <= 96 px)."""
    from innfer_amd import synth
    from innfer_amd.run import Model
    from innfer_amd.utils import utils as U
    m, sd = model
    h, w = 40, 56
    img = synth.image_u8(h, w, 3, 61)
    plain = m.run_u8(img)
    assert plain.shape == (4 * h, 4 * w, 3) and np.array_equal(plain, U.tensor2np(m(U.np2tensor(img, dtype=torch.float16))))
    got = m.run_u8(img, tta=True)
    assert np.array_equal(got, U.tensor2np(m.forward_tta(U.np2tensor(img, dtype=torch.float16))))
    got = m.run_u8(img, seamless="tile")
    want = U.tensor2np(m(U.np2tensor(U.seamless_pad_np(img, "tile"), dtype=torch.float16)))[64:-64, 64:-64]
    assert got.shape == plain.shape and np.array_equal(got, want)
    imgs = [img, synth.image_u8(33, 96, 3, 62), synth.image_u8(64, 17, 3, 63)]
    for a, b in zip(m.run_u8_batch(imgs), [m.run_u8(i) for i in imgs]):
        assert np.array_equal(a, b)
    mt = Model(None, arch="infer", scale=None, device="cuda", chop=True, tile_batch=4, state_dict={"params_ema": sd}, tile=32, tile_pad=8)
    big = synth.image_u8(70, 96, 3, 64)
    assert np.array_equal(mt.run_u8(big), U.tensor2np(mt(U.np2tensor(big, dtype=torch.float16))))
