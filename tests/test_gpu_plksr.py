"""RealPLKSR on the GPU (needs an MI355X: `pytest -m gpu`): the partial large-kernel conv, the Mish epilogue and the GroupNorm + skip pass alone, whole networks, the Model.

1. innfer_plk_conv against float64 on the fp16 operands, within tests/_conv_ref.py's bound (assert_within_fp16_rounding) with e32 measured as _conv_ref defines it (float32
   F.conv2d on the CPU against float64, same operands) and extra = 0.  k 17 and k 13; 1x1, 8x8 (smaller than the radius), one whole tile, ragged edges, several tiles, a
   batch (a workgroup owns ONE tile: there is no second-tile path).  Channels 16 .. 31 bit for bit; guard bands and the neighbouring slab group keep their fill; an
   overlapping output is refused with nothing written.
2. act 11 (innfer_conv3x3_f16, 64 outputs, both row orders) against float64 Mish on the float64 conv, extra = |f| MISH_T.
   MISH_T -- derived as _conv_ref.TRANS is.  common.h fast_mish computes f * r, r = w / (w + 2), w = n (n + 2), n = e^min(f, 20):
     n:  v_exp_f32 is a 1-ulp instruction (2^-23 relative) and the argument scaling f log2(e), rounded to fp32, moves n by |f| 2^-24 relative:  dn <= |f| 2^-24 + 2^-23;
     w:  d ln w / d ln n = (2 n + 2) / (n + 2) <= 2, and two fp32 roundings (the sum, the product):                                         dw <= 2 dn + 2^-23;
     r:  d ln r / d ln w = 2 / (w + 2); the sum w + 2, v_rcp_f32 (1 ulp), the product w * rcp: 4 units of 2^-24;  f * r: one more.
   The absolute error of f r is therefore |f| r [2 / (w + 2)] dw + 5 |f| r 2^-24 <= |f| (g (|f| 2^-23 + 3 * 2^-23) + 5 * 2^-24) with g = 2 w / (w + 2)^2 <= 1/4 (w = 2) and
   |f| g <= 0.25 over the whole line (largest near f = -1.5; for large |f| either 2 / (w + 2) or r = w / (w + 2) ~ e^f kills it):  <= |f| (0.5 + 1.5 + 5) 2^-24 = |f| 7 * 2^-24.
   The cap of the exponent at 20 costs r = 1 instead of 1 - 2 e^-40.  MISH_T = 2^-21 holds with room.
   One case has biases of +-60: e^60 squared overflows fp32 -- the result must be finite (f itself above, -0 below).
   The refusals: status and nothing written.
3. innfer_group_norm_skip (statistics, merge, apply: the network's three launches) against float64 GroupNorm on the stored fp16 operands, PER SAMPLE, on batches whose
   samples differ in scale and offset.  The bound, per element, is one fp16 rounding plus GN_STATS (below): what fp32 statistics and the fp32 fma + add can cost.
     out = fp16(fma(alpha, u, shift) + skip), alpha = gamma rstd, shift = beta - mean alpha;  exact: y = gamma z + beta + skip, z = (u - mu) / sigma.
     mean:  a thread sums 128 values in order, then 4 butterfly steps and 3 adds over the waves: the summation bound gamma_135 ~ 135 * 2^-24 relative to sum |u| <= count A
            (A = max |u| of the sample); a Chan merge of two records costs <= 8 roundings on either moment, R = records per group:      |dmu| <= (135 + 8 R) 2^-24 A
     var:   the squared deviations from the segment's own (rounded) mean, summed the same way (the two-pass form: the mean's error enters squared):
                                                                                                                               dvar <= (140 + 8 R) 2^-24 relative
     rstd = 1 / sqrtf(var + eps): dvar / 2 and two operations of <= 2 ulp each; alpha = rstd gamma: one rounding:              dalpha <= ((140 + 8 R) / 2 + 9) 2^-24 relative
     out - y = (alpha^ - alpha)(u - mu) - alpha^ (mu^ - mu) + the roundings of shift (2), the fma (1) and the add (1), each relative to a term below
            |gamma| (A + |mu|) / sigma + |beta| + |skip|.
   GN_STATS = 2^-24 [ ((140 + 8 R) / 2 + 9) |gamma z| + (135 + 8 R) |gamma| A / sigma + 4 (|gamma| (A + |mu|) / sigma + |beta| + |skip|) ].
4. Networks against the float64 forward of tests/_plksr_ref.py: max |err| <= 2 x the fp16 storage model's own error on the same case and >= 99 % of the uint8 codes within
   +-1 (tests/test_plksr_host.py verifies the storage model alone on the CPU); <= 9 n_blocks + 3 launches per forward; forward_u8 == the separate conversions; a float32
   tensor is refused.
   Measured on the MI355X, engine max |err| / storage model max |err| (100 % of the codes within +-1 in every case):
       3 blocks x4 32x32 1.000 | 2 blocks x2 21x37 1.000 | 2 blocks x3 9x17 1.101 | 2 blocks x1 8x8 1.000 | S (k 13, no EA) x2 20x24 1.000 | batch of two 1.072 |
       28 blocks x4 24x24 1.062 | Model chop x2 250x330 1.000
   plk_conv alone: worst err / bound 0.875 .. 0.993 (e32 1.7e-8 .. 3.4e-6); act 11: 0.954 .. 0.995; GroupNorm + skip: 0.963 .. 0.982 (the fp16 rounding dominates).
5. Model(arch='infer', chop=True) from a .pth under params_ema against the helper run tile by tile (GroupNorm normalises per tile there, as in the reference run of the
   tiles); run_u8 and its options against their definitions, bit for bit.
"""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _conv_ref as R
import _plksr_ref as PR
from _conv_ref import Case

pytestmark = pytest.mark.gpu

FILL, GUARD = -3.0, 4096
MISH_T = 2.0 ** -21
S16 = [(1, 1, 1), (1, 16, 32), (1, 17, 33), (1, 50, 70), (3, 37, 45)]          # the 16 x 32-tile edges (64 outputs)
MANY16 = (1, 273, 513)                                                         # more tiles than the 256 workgroups: a second tile per workgroup
PLK_SHAPES = [(1, 1, 1), (1, 8, 8), (1, 16, 32), (1, 17, 33), (1, 50, 70), (3, 37, 45)]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


# ------------------------------------------------------------------------------------------------ 1. the partial large-kernel conv
def _plk_data(k, N, H, W, seed):
    from innfer_amd import synth
    x = torch.from_numpy(synth.uniform((N, 32, H, W), 9000 + seed, -1, 1)).half()
    w = torch.from_numpy(synth.uniform((16, 16, k, k), 9001 + seed, -1, 1) / np.float32(np.sqrt(16.0 * k * k)))
    b = torch.from_numpy(synth.uniform((16,), 9002 + seed, -1, 1))
    return x, w, b


def _plk_launch(dev, x, w, b, k, overlap=None):
    """innfer_plk_conv from a slab of its own into [guard | output group | neighbouring group | guard]; overlap: element offset of the output INSIDE the input's buffer
    instead (must be refused).  Returns the output group as [N, 32, H, W] fp16 (cpu)."""
    import innfer_amd.lib as L
    N, _, H, W = x.shape
    G = N * H * W * 32
    wc, bc = np.ascontiguousarray(w.numpy(), np.float32), np.ascontiguousarray(b.numpy(), np.float32)
    if overlap is not None:
        buf = torch.full((2 * G + 2 * GUARD,), FILL, dtype=torch.float16, device=dev)
        rc = L.lib.innfer_plk_conv(buf.data_ptr() + 2 * GUARD, buf.data_ptr() + 2 * (GUARD + overlap), N, H, W, k, wc.ctypes.data, bc.ctypes.data, None)
        torch.cuda.synchronize()
        assert rc == L.ERR_INVALID, (overlap, rc, L.last_error())
        assert bool((buf.cpu() == FILL).all()), "a refused launch wrote"
        return None
    xin = R.to_slab(x).to(dev)
    buf = torch.full((2 * G + 2 * GUARD,), FILL, dtype=torch.float16, device=dev)
    L.check(L.lib.innfer_plk_conv(xin.data_ptr(), buf.data_ptr() + 2 * GUARD, N, H, W, k, wc.ctypes.data, bc.ctypes.data, None))
    torch.cuda.synchronize()
    raw = buf.cpu()
    assert bool((raw[:GUARD] == FILL).all()) and bool((raw[GUARD + 2 * G:] == FILL).all()), "plk_conv wrote outside its output"
    assert bool((raw[GUARD + G:GUARD + 2 * G] == FILL).all()), "plk_conv wrote to the neighbouring slab group"
    assert torch.equal(xin.cpu(), R.to_slab(x)), "plk_conv wrote to its input"
    return R.from_slab(raw[GUARD:GUARD + G].reshape(1, N, H, W, 32))


@pytest.mark.parametrize("k", [17, 13])
def test_plk_conv(dev, k):
    for i, (N, H, W) in enumerate(PLK_SHAPES):
        x, w, b = _plk_data(k, N, H, W, 10 * k + i)
        w16 = w.half()
        ref = F.conv2d(x[:, :16].double(), w16.double(), b.double(), padding=k // 2)
        e32 = float((F.conv2d(x[:, :16].float(), w16.float(), b, padding=k // 2).double() - ref).abs().max())
        got = _plk_launch(dev, x, w, b, k)
        assert torch.equal(got[:, 16:].view(torch.int16), x[:, 16:].view(torch.int16)), f"k {k} {N}x{H}x{W}: channels 16 .. 31 are not the input's"
        R.assert_within_fp16_rounding(got[:, :16], ref, e32, what=f"plk k {k} {N}x{H}x{W}", family=f"plk_conv k {k}")


def test_plk_conv_refuses_overlap(dev):
    """The output on the input, or shifted by part of a group into it: INNFER_ERR_INVALID and nothing written (other workgroups still read the halo)."""
    import innfer_amd.lib as L
    x, w, b = _plk_data(17, 1, 16, 32, 5)
    G = 16 * 32 * 32
    for off in (0, 32, G - 32):
        _plk_launch(dev, x, w, b, 17, overlap=off)
    buf = torch.zeros(4 * G, dtype=torch.float16, device=dev)
    wc = np.ascontiguousarray(w.numpy(), np.float32)
    for kk in (16, 19, 1):
        assert L.lib.innfer_plk_conv(buf.data_ptr(), buf.data_ptr() + 4 * G, 1, 16, 32, kk, wc.ctypes.data, None, None) == L.ERR_UNSUPPORTED


# ------------------------------------------------------------------------------------------------ 2. the Mish epilogue
def _launch(dev, c, plane_rows=0, expect=0, form="3x3", bias=None, res=False, **fields):
    """One launch through innfer_conv3x3_f16 with act 11 into [guard | the conv's groups | a foreign group | guard]: everything beside the result must keep its fill, like
    everything a refused launch (expect != 0) was given.  Returns [N, K, H, W] fp16 (cpu)."""
    import innfer_amd.lib as L
    lib = L.lib
    x, w, b = R.data(c)
    if bias is not None:
        b = bias
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
    bb = torch.zeros(64); bb[:c.K] = b
    d_bias = bb.to(dev)
    groups = (c.K + 31) // 32 + 1
    G = N * H * W * 32
    buf = torch.full((2 * groups * G + 2 * GUARD,), FILL, dtype=torch.float16, device=dev)
    keep = []
    a = L.ConvArgs()
    a.d_in, a.in_group_stride, a.C = xin.data_ptr(), G, Cc
    a.d_packed, a.d_bias = d_packed.data_ptr(), d_bias.data_ptr()
    a.d_out, a.out_group_stride, a.K = buf.data_ptr() + GUARD * 2, G, c.K
    a.N, a.H, a.W, a.act, a.plane_rows = N, H, W, 11, plane_rows
    a.conv1x1 = int(form == "1x1")
    if res:
        keep.append(R.to_slab(torch.zeros((N, max(c.K, 32), H, W), dtype=torch.float16)).to(dev))
        a.d_res1, a.res1_group_stride, a.res1_scale = keep[-1].data_ptr(), G, 1.0
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
        assert rc == expect, (str(c), fields, rc, L.last_error())
        assert bool((raw == FILL).all()), f"{c}: a refused launch wrote to d_out"
        return None
    assert rc == 0, (str(c), L.last_error())
    assert bool((raw[:GUARD] == FILL).all()) and bool((raw[GUARD + groups * G:] == FILL).all()), f"{c}: wrote outside the output"
    got = R.from_slab(raw[GUARD:GUARD + groups * G].reshape(groups, N, H, W, 32))
    assert bool((got[:, c.K:] == FILL).all()), f"{c}: channels beside the conv's were written"
    return got[:, :c.K]


@pytest.mark.parametrize("plane_rows", [0, 1])
def test_mish_epilogue(dev, plane_rows):
    """conv3x3_pc<2, 4, 4, OUT_SLAB, .., TAPS_3X3 [| PC_ROWP] | PC_MISH>: 64 -> 64, both row orders; ragged edges, a batch, a workgroup's second tile (273 x 513)."""
    for i, (N, H, W) in enumerate(S16 + [MANY16]):
        c = Case("3x3", N, 64, 64, H, W, seed=170 + i, blo=-3.0)
        y64, e32 = R.pre(c)
        got = _launch(dev, c, plane_rows)
        R.assert_within_fp16_rounding(got, PR.mish(y64), e32, extra=y64.abs() * MISH_T, what=f"{c} act 11 plane_rows {plane_rows}", family=f"act 11, plane_rows {plane_rows}")


@pytest.mark.parametrize("plane_rows", [0, 1])
def test_mish_epilogue_large_arguments(dev, plane_rows):
    """Biases of +-60 (alternating by channel): n^2 = e^120 overflows fp32 -- the result stays finite: f itself above, (minus) zero below."""
    c = Case("3x3", 1, 64, 64, 17, 33, seed=181)
    bias = torch.tensor([60.0 if i % 2 == 0 else -60.0 for i in range(64)])
    x, w, _ = R.data(c)
    y64 = F.conv2d(x.double(), w.half().double(), bias.double(), padding=1)
    e32 = float((F.conv2d(x.float(), w.half().float(), bias, padding=1).double() - y64).abs().max())
    got = _launch(dev, c, plane_rows, bias=bias)
    assert torch.isfinite(got).all() and float(y64.abs().min()) > 55
    assert bool((got[:, 1::2] == 0).all()) and bool((got[:, 0::2] > 55).all())
    R.assert_within_fp16_rounding(got, PR.mish(y64), e32, extra=y64.abs() * MISH_T, what=f"{c} act 11, biases +-60, plane_rows {plane_rows}", family="act 11, large arguments")


def test_mish_epilogue_refusals(dev):
    """act 11 on a form that does not build it is UNSUPPORTED; nothing is launched: d_out keeps its fill."""
    import innfer_amd.lib as L
    c = Case("3x3", 1, 64, 64, 16, 32, seed=195)
    G = 16 * 32 * 32
    U = L.ERR_UNSUPPORTED
    _launch(dev, c, form="1x1", expect=U)
    _launch(dev, c, out_planar=1, expect=U)
    _launch(dev, c, split=1, in_lo=3 * G, out_lo=3 * G, expect=U)
    _launch(dev, c, d_stats_part=1, expect=U)
    _launch(dev, c, stride2_k4=1, expect=U)
    _launch(dev, c, transposed2x=4, expect=U)
    _launch(dev, c, upsample2x=1, expect=U)
    _launch(dev, c, reflect_pad=1, expect=U)
    _launch(dev, c, res=True, expect=U)
    _launch(dev, Case("3x3", 1, 64, 32, 16, 32, seed=196), dilation=2, expect=U)
    _launch(dev, Case("3x3", 1, 64, 32, 16, 32, seed=196), expect=U)          # the 32-output kernel has no Mish form
    _launch(dev, Case("3x3", 1, 64, 16, 16, 32, seed=197), expect=U)


# ------------------------------------------------------------------------------------------------ 3. GroupNorm + skip
def _gn_data(N, H, W, seed):
    from innfer_amd import synth
    u = synth.uniform((N, 64, H, W), 7000 + seed, -1, 1)
    for n in range(N):                                  # samples of different scale and offset: statistics shared across the batch would miss by far
        u[n] = u[n] * np.float32(1.0 + 1.5 * n) + np.float32(0.4 * n - 0.2)
    u = u * synth.uniform((1, 64, 1, 1), 7001 + seed, 0.5, 1.5) + synth.uniform((1, 64, 1, 1), 7002 + seed, -0.5, 0.5)      # channels of a group differ too
    skip = synth.uniform((N, 64, H, W), 7003 + seed, -1, 1)
    gamma, beta = synth.uniform((64,), 7004 + seed, 0.25, 0.75), synth.uniform((64,), 7005 + seed, -0.1, 0.1)
    return torch.from_numpy(u).half(), torch.from_numpy(skip).half(), torch.from_numpy(gamma), torch.from_numpy(beta)


def _gn_launch(dev, u, skip, gamma, beta, groups, in_place=False):
    import innfer_amd.lib as L
    N, _, H, W = u.shape
    G = N * H * W * 32
    du, ds = R.to_slab(u).to(dev), R.to_slab(skip).to(dev)
    nb = L.lib.innfer_group_norm_skip_work_bytes(N, H * W)
    work = torch.empty(nb, dtype=torch.uint8, device=dev)
    g, b = np.ascontiguousarray(gamma.numpy(), np.float32), np.ascontiguousarray(beta.numpy(), np.float32)
    if in_place:
        L.check(L.lib.innfer_group_norm_skip(du.data_ptr(), G, ds.data_ptr(), G, ds.data_ptr(), G, N, H * W, groups, g.ctypes.data, b.ctypes.data, 1e-5, work.data_ptr(), nb, None))
        torch.cuda.synchronize()
        return R.from_slab(ds.cpu())
    buf = torch.full((3 * G + 2 * GUARD,), FILL, dtype=torch.float16, device=dev)
    L.check(L.lib.innfer_group_norm_skip(du.data_ptr(), G, ds.data_ptr(), G, buf.data_ptr() + 2 * GUARD, G, N, H * W, groups, g.ctypes.data, b.ctypes.data, 1e-5, work.data_ptr(), nb, None))
    torch.cuda.synchronize()
    raw = buf.cpu()
    assert bool((raw[:GUARD] == FILL).all()) and bool((raw[GUARD + 2 * G:] == FILL).all()), "group_norm_skip wrote outside its output"
    assert torch.equal(du.cpu(), R.to_slab(u)) and torch.equal(ds.cpu(), R.to_slab(skip)), "group_norm_skip wrote to its inputs"
    return R.from_slab(raw[GUARD:GUARD + 2 * G].reshape(2, N, H, W, 32))


@pytest.mark.parametrize("groups", [4, 1, 8])
def test_group_norm_skip(dev, groups):
    for i, (N, H, W) in enumerate([(2, 9, 17), (2, 37, 45), (3, 40, 70)]):
        u, skip, gamma, beta = _gn_data(N, H, W, 10 * groups + i)
        u64, cpg = u.double(), 64 // groups
        ref = F.group_norm(u64, groups, gamma.double(), beta.double(), eps=1e-5) + skip.double()
        grp = u64.reshape(N, groups, cpg * H * W)
        mu = grp.mean(2).repeat_interleave(cpg, 1)[:, :, None, None]
        sigma = torch.sqrt(grp.var(2, unbiased=False) + 1e-5).repeat_interleave(cpg, 1)[:, :, None, None]
        A = u64.abs().amax((1, 2, 3), keepdim=True)
        Rn = ((H * W + 1023) // 1024) * (cpg // 8)                     # records per group
        ga, be = gamma.double().abs()[None, :, None, None], beta.double().abs()[None, :, None, None]
        z = (u64 - mu) / sigma
        gn_stats = 2.0 ** -24 * (((140 + 8 * Rn) / 2 + 9) * ga * z.abs() + (135 + 8 * Rn) * ga * A / sigma + 4 * (ga * (A + mu.abs()) / sigma + be + skip.double().abs()))
        got = _gn_launch(dev, u, skip, gamma, beta, groups)
        R.assert_within_fp16_rounding(got, ref, 0.0, extra=gn_stats, what=f"group norm + skip, {groups} groups, {N}x{H}x{W}", family=f"group norm, {groups} groups")
        # a batch is N independent samples: sample n alone gives the same bits
        one = _gn_launch(dev, u[N - 1:], skip[N - 1:], gamma, beta, groups)
        assert torch.equal(one.view(torch.int16), got[N - 1:].view(torch.int16))
        if i == 1:
            assert torch.equal(_gn_launch(dev, u, skip, gamma, beta, groups, in_place=True).view(torch.int16), got.view(torch.int16))


# ------------------------------------------------------------------------------------------------ 4. networks
def _net(dev, sd, wrap=True):
    from innfer_amd.architectures import get_network
    from innfer_amd.run import infer_from_state_dict
    info = infer_from_state_dict({"params_ema": sd} if wrap else sd)
    net = get_network(info["net_params"])
    net.load_state_dict(info["state_dict"], strict=True)
    return net.to(dev).eval()


def _assert_like_storage_model(got, y64, ys, what):
    """max |engine - float64| <= 2 x max |storage model - float64| of the same case (computed here), and >= 99 % of the uint8 codes within +-1."""
    err, es = float((got.double() - y64).abs().max()), float((ys - y64).abs().max())
    share = PR.codes_within_one(got, y64)
    print(f"[plksr] {what}: engine max|err| {err:.2e}, storage model {es:.2e}, ratio {err / es:.3f}; codes within +-1: {share:.5f}")
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
    ms = (C.c_float * 512)()
    L.check(L.lib.innfer_net_forward_timed(net._handle, x.data_ptr(), L.F16, out.data_ptr(), L.F16, N, H, W, ws.data_ptr(), ws.numel(), None, 512, ms, None, None, None, C.byref(n)))
    return n.value, out


@pytest.mark.parametrize("name", list(PR.FIXTURES))
def test_network_vs_float64(dev, name):
    from innfer_amd import synth
    from innfer_amd.utils import utils as U
    nb, scale, shape, k, ea, seed = PR.FIXTURES[name]
    sd, x, y64, ys = PR.case(name)
    net = _net(dev, sd)
    assert (net.n_blocks, net.kernel_size, net.use_ea) == (nb, k, ea)
    xd = x.to(dev).half()
    y = net(xd)
    assert y.dtype == torch.float16 and net._out_shape(shape[0], shape[2], shape[3], dev) == tuple(y64.shape) == tuple(y.shape)
    _assert_like_storage_model(y.float().cpu(), y64, ys, name)
    n, yt = _launches(net, xd)
    assert n <= 9 * nb + 3 and n == (9 if ea else 8) * nb + 3 and torch.equal(yt, y), n
    if nb > 3:
        return
    buf = torch.empty(y.shape, dtype=torch.float16, device=dev)
    assert net(xd, out=buf) is buf and torch.equal(buf, y)
    if shape[0] > 1:          # a batch is independent samples: GroupNorm's statistics are per sample
        assert torch.equal(net(xd[1:]), y[1:])
    img = torch.from_numpy(synth.image_u8(shape[2], shape[3], 3, scale)).to(dev)
    sep = U.tensor2np(net(U.np2tensor(img.cpu().numpy(), dtype=torch.float16)))
    assert np.array_equal(net.forward_u8(img).cpu().numpy(), sep)
    with pytest.raises(NotImplementedError, match="fp16 mode"):
        net(x.to(dev))
    with pytest.raises(NotImplementedError, match="fp16 mode"):
        net.forward_u8(img, fp16=False)
    assert net.flops(1, shape[2], shape[3]) > 0 and net.tile_batch_bytes(2, 16) > 0


# ------------------------------------------------------------------------------------------------ 5. the Model
@pytest.fixture(scope="module")
def model(tmp_path_factory):
    from innfer_amd.run import Model
    sd = PR.fill(3, 64, 1, 2, 17, True, seed=8)
    path = str(tmp_path_factory.mktemp("plksr") / "2x_realplksr.pth")
    torch.save({"params_ema": sd}, path)
    m = Model(path, arch="infer", scale=None, device="cuda", chop=True, tile_batch=4)
    assert (m.arch, m.scale, m.in_nc, m.out_nc) == ("realplksr", 2, 3, 3)
    return m, sd


def test_model_chop(dev, model):
    """250 x 330 through the chop path against the helper run tile by tile (oracle.extract_patches_2d / recompose_tensor; the storage model's blend rounded to fp16 as the
    chop path's is; every 200-px tile is normalised by its own statistics on both sides); run_u8 == the separate conversions; a float32 tensor is refused."""
    import oracle
    from innfer_amd import synth
    from innfer_amd.utils import utils as U
    m, sd = model
    x = torch.from_numpy(synth.uniform((1, 3, 250, 330), 52))
    y = m(x.to(dev).half()).float().cpu()
    assert tuple(y.shape) == (1, 3, 500, 660)
    tiles = oracle.extract_patches_2d(x, (200, 200), [0.5, 0.5], batch_first=True).squeeze(0)
    h64 = torch.cat([PR.forward64(sd, tiles[i:i + 1], 2) for i in range(tiles.shape[0])], 0)
    hs = torch.cat([PR.forward_storage(sd, tiles[i:i + 1], 2) for i in range(tiles.shape[0])], 0)
    y64 = oracle.recompose_tensor(h64, 250, 330, step=0.5, scale=2).double()
    ys = oracle.recompose_tensor(hs, 250, 330, step=0.5, scale=2).half().double()
    _assert_like_storage_model(y, y64, ys, "Model chop x2 250x330")
    img = synth.image_u8(250, 330, 3, 9)
    assert np.array_equal(m.run_u8(img), U.tensor2np(m(U.np2tensor(img, dtype=torch.float16))))
    with pytest.raises(NotImplementedError, match="fp16 mode"):
        m(x.to(dev))


def test_model_run_u8_options(dev, model):
    """plain, tile=, tta, seamless='tile' and run_u8_batch on a RealPLKSR model: each equals the definition its docstring gives for it, bit for bit (images <= 96 px)."""
    from innfer_amd import synth
    from innfer_amd.run import Model
    from innfer_amd.utils import utils as U
    m, sd = model
    h, w = 40, 56
    img = synth.image_u8(h, w, 3, 61)
    plain = m.run_u8(img)
    assert plain.shape == (2 * h, 2 * w, 3) and np.array_equal(plain, U.tensor2np(m(U.np2tensor(img, dtype=torch.float16))))
    got = m.run_u8(img, tta=True)
    assert np.array_equal(got, U.tensor2np(m.forward_tta(U.np2tensor(img, dtype=torch.float16))))
    got = m.run_u8(img, seamless="tile")
    want = U.tensor2np(m(U.np2tensor(U.seamless_pad_np(img, "tile"), dtype=torch.float16)))[32:-32, 32:-32]
    assert got.shape == plain.shape and np.array_equal(got, want)
    imgs = [img, synth.image_u8(33, 96, 3, 62), synth.image_u8(64, 17, 3, 63)]
    for a, b in zip(m.run_u8_batch(imgs), [m.run_u8(i) for i in imgs]):
        assert np.array_equal(a, b)
    mt = Model(None, arch="infer", scale=None, device="cuda", chop=True, tile_batch=4, state_dict={"params_ema": sd}, tile=32, tile_pad=8)
    big = synth.image_u8(70, 96, 3, 64)
    assert np.array_equal(mt.run_u8(big), U.tensor2np(mt(U.np2tensor(big, dtype=torch.float16))))
