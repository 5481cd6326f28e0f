"""Swin2SR on the GPU (needs an MI355X: `pytest -m gpu`): the cosine window attention and the LayerNorm + residual alone, whole networks, the Model.
Every launch writes between guard bands that must keep their fill; inputs must be unchanged.

1. innfer_window_attention_cos against float64 on the stored fp16 operands: padded sizes 8x8, 8x16, 16x24, 24x40, each with shift 0 and shift 4; (nH, d) = (6, 30),
   (6, 10), (2, 32), (8, 30); tau spread geometrically over 1 .. 100 across the heads; a batch of 3 whose samples differ, each bit-equal to its own N = 1 launch; one case
   where some tokens' q and some tokens' k are all zero (their scores are the bias alone: finite, inside the bound); one case with q scaled by 1 / 64 and k by 24 (a
   normalisation forgotten on either operand scales the scores by that factor).  The bound is tests/test_gpu_swinir.py's convention, ulp16 / 2 + 8 e_model:
   e_model = max |model - exact| of a torch model of the kernel's DECLARED roundings -- the raw product of the fp16 operands, the two norms, r = 1 / max(sqrt(.), 1e-12)
   and S = raw (rq tau) rk + B (+ M) in float32, float32 maximum, exponentials and sum, P rounded to fp16 as the operand of P v, float32 accumulation and division --
   computed on the CPU, never from the kernel.  Pad channels of the output are exactly zero.  The refusals return a status and write nothing.
2. innfer_layer_norm_add against float64 res + LayerNorm(x) on the stored fp16 operands: C = 60, 180, 240, 64 in slabs of 64 ceil(C / 64) channels whose pad channels
   hold junk in `in` (and in `res`); 1x1, 8x8, 17x33 pixels and a batch; out of place, out == res and out == in agree bit for bit.  The bound, per element, is one fp16
   rounding plus tests/test_gpu_swinir.py's LN_STATS (derived there: what the float32 statistics, the difference, the product and the fma can cost) plus the added
   operation: the kernel computes fp16(fl32(res + LN^)) where LN^ is the float32 fma's result.  LN^ is now a float32 INTERMEDIATE and not the operand of the fp16
   rounding: its own rounding is <= u |LN|, u = 2^-24; res is an fp16 number, exact in float32; the float32 sum rounds once: <= u |res + LN|.  So
     bound = ulp16 / 2 + LN_STATS + 2^-24 (|LN| + |res + LN|).
3. Networks against the float64 forward of tests/_swin2sr_ref.py: max |err| <= 2 x the fp16 storage model's own error on the same case and >= 99 % of the uint8 codes
   within +-1 (tests/test_swin2sr_host.py verifies the storage model alone on the CPU); the launch count equals SwinIR's formula; out= is
   honoured; a batch's sample equals its own forward bit for bit; forward_u8 == the separate conversions; a float32 tensor is refused; a side too short to pad is refused.
   Measured on the MI355X, engine max |err| / storage model max |err| (100 % of the codes within +-1 in every case):
       C60 [2,2] direct x2 16x24 1.008 | C60 direct x4 13x21 (padded) 1.000 | C180 pixelshuffle x4 16x16 0.855 | pixelshuffle x3 9x17 0.937 |
       C240 nH8 3conv nearest+conv x4 16x24 0.953 | C64 nH2 pixelshuffle x2 8x8 1.000 | batch of two pixelshuffle x2 19x26 0.985 | Model chop x2 250x330 1.000
   Measured worst err / bound of the single launches: cosine attention 0.200 .. 0.254 (e_model 1.3e-4 .. 3.1e-4; zero rows 0.219 .. 0.237, q / 64 with 24 k
   0.240 .. 0.250); layer norm + residual 0.993 .. 0.998 (the fp16 rounding dominates).
4. Model(arch='infer', chop=True) from a .pth under params (with the three buffers of a published checkpoint) against the helper run tile by tile; run_u8 plain, tta,
   seamless='tile', run_u8_batch and tile=32, tile_pad=8 against their definitions, bit for bit.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import _conv_ref as R
import _swin2sr_ref as S2
import _swinir_ref as SR

pytestmark = pytest.mark.gpu

FILL, GUARD = -3.0, 4096


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


# ------------------------------------------------------------------------------------------------ 1. the cosine window attention
def _tau(nH):
    return torch.from_numpy(np.geomspace(1.0, 100.0, nH).astype(np.float32)) if nH > 1 else torch.tensor([100.0])


def _attn_data(N, Hp, Wp, nH, d, seed, qgain=1.0, kgain=1.0, zeros=False):
    """q, k, v as fp16 [3, N, nH, d, Hp, Wp] (the values of the slab's real channels), the dense bias table [nH, 64, 64] float32 and tau [nH] float32; samples differ."""
    from innfer_amd import synth
    qkv = synth.uniform((3, N, nH, d, Hp, Wp), 6000 + seed, -1, 1)
    for n in range(N):
        qkv[:, n] *= np.float32(1.0 + 0.5 * n)
    qkv[0] *= np.float32(qgain)
    qkv[1] *= np.float32(kgain)
    if zeros:                                                  # all-zero q rows at some pixels, all-zero k rows at others (and both at one)
        qkv[0, :, :, :, 1::3, 2::5] = 0
        qkv[1, :, :, :, 2::4, 1::3] = 0
        qkv[0:2, :, :, :, 0, 0] = 0
    table = synth.uniform((nH, 64, 64), 6001 + seed, 0, 16)
    return torch.from_numpy(qkv).half(), torch.from_numpy(np.ascontiguousarray(table)), _tau(nH)


def _attn_ref(qkv, table, tau, shift, dt, model=False):
    """softmax((q^ k^^T) tau + B + M) v per window and head in dtype dt through the roll; model (dt float32): the declared roundings -- raw product, norms and the scaling
    S = raw (rq tau) rk + B in float32, P rounded to fp16 in front of P v, the sum over the unrounded values."""
    _, N, nH, d, Hp, Wp = qkv.shape
    x = qkv.to(dt).reshape(3 * N, nH * d, Hp, Wp)
    if shift:
        x = torch.roll(x, (-shift, -shift), (2, 3))
    w = SR._windows(x).reshape(3, N, -1, 64, nH, d).permute(0, 1, 2, 4, 3, 5)          # [3, N, nW, nH, 64, d]
    q, k, v = w[0], w[1], w[2]
    t = tau.to(dt)[:, None, None]
    if model:
        rq = t / torch.sqrt((q * q).sum(-1, keepdim=True)).clamp(min=1e-12)
        rk = 1.0 / torch.sqrt((k * k).sum(-1, keepdim=True)).clamp(min=1e-12)
        S = (q @ k.transpose(-1, -2)) * rq * rk.transpose(-1, -2) + table.to(dt)
    else:
        qn = q / q.norm(dim=-1, keepdim=True).clamp(min=1e-12)
        kn = k / k.norm(dim=-1, keepdim=True).clamp(min=1e-12)
        S = (qn @ kn.transpose(-1, -2)) * t + table.to(dt)
    if shift:
        S = S + SR.shift_mask(Hp, Wp).to(dt)[None, :, None]
    if model:
        e = torch.exp(S - S.amax(-1, keepdim=True))
        o = (e.half().to(dt) @ v) / e.sum(-1, keepdim=True)
    else:
        o = torch.softmax(S, -1) @ v
    o = SR._unwindows(o.permute(0, 1, 3, 2, 4).reshape(N, -1, 64, nH * d), Hp, Wp)
    if shift:
        o = torch.roll(o, (shift, shift), (2, 3))
    return o.reshape(N, nH, d, Hp, Wp)


def _attn_launch(dev, qkv, table, tau, shift):
    """innfer_window_attention_cos from a head-padded slab of its own into [guard | nH groups | a foreign group | guard].  Returns [N, nH, 32, Hp, Wp] fp16 (cpu)."""
    import innfer_amd.lib as L
    _, N, nH, d, Hp, Wp = qkv.shape
    G = N * Hp * Wp * 32
    pad = torch.zeros(3, N, nH, 32, Hp, Wp, dtype=torch.float16)
    pad[:, :, :, :d] = qkv
    slab = pad.permute(0, 2, 1, 4, 5, 3).contiguous()                                  # [3, nH, N, Hp, Wp, 32]: group which * nH + h
    xin = slab.to(dev)
    buf = torch.full(((nH + 1) * G + 2 * GUARD,), FILL, dtype=torch.float16, device=dev)
    tb, tt = np.ascontiguousarray(table.numpy(), np.float32), np.ascontiguousarray(tau.numpy(), np.float32)
    L.check(L.lib.innfer_window_attention_cos(xin.data_ptr(), G, buf.data_ptr() + 2 * GUARD, G, tb.ctypes.data, tt.ctypes.data, N, Hp, Wp, nH, d, shift, None))
    torch.cuda.synchronize()
    raw = buf.cpu()
    assert bool((raw[:GUARD] == FILL).all()) and bool((raw[GUARD + nH * G:] == FILL).all()), "cosine attention wrote outside its output"
    assert torch.equal(xin.cpu(), slab), "cosine attention wrote to its input"
    return raw[GUARD:GUARD + nH * G].reshape(nH, N, Hp, Wp, 32).permute(1, 0, 4, 2, 3)


def _attn_check(dev, N, Hp, Wp, nH, d, shift, seed, note="", **kw):
    qkv, table, tau = _attn_data(N, Hp, Wp, nH, d, seed, **kw)
    ref = _attn_ref(qkv, table, tau, shift, torch.float64)
    e_model = float((_attn_ref(qkv, table, tau, shift, torch.float32, model=True).double() - ref).abs().max())
    got = _attn_launch(dev, qkv, table, tau, shift)
    assert bool((got[:, :, d:] == 0).all()), "pad channels of the attention's result are not zero"
    R.assert_within_fp16_rounding(got[:, :, :d], ref, e_model, what=f"cosine attention {N}x{Hp}x{Wp} nH {nH} d {d} shift {shift}{note}", family=f"cosine attention, shift {shift}")
    return qkv, table, tau, got


@pytest.mark.parametrize("nH,d", [(6, 30), (6, 10), (2, 32), (8, 30)])
def test_cosine_attention(dev, nH, d):
    for i, (Hp, Wp) in enumerate([(8, 8), (8, 16), (16, 24), (24, 40)]):
        for shift in (0, 4):
            _attn_check(dev, 1, Hp, Wp, nH, d, shift, 100 * nH + 10 * i + shift)


def test_cosine_attention_batch_zero_rows_and_scaled_operands(dev):
    """A window of sample n reads only sample n: each sample of a batch of three equals its own launch bit for bit.  All-zero q / k rows give finite results inside the
    bound (their scores are the bias alone).  q / 64 and 24 k give results inside the same bound: both operands are normalised."""
    for shift in (0, 4):
        qkv, table, tau, got = _attn_check(dev, 3, 16, 24, 6, 30, shift, 900 + shift)
        for n in range(3):
            one = _attn_launch(dev, qkv[:, n:n + 1].contiguous(), table, tau, shift)
            assert torch.equal(one.view(torch.int16), got[n:n + 1].contiguous().view(torch.int16)), (shift, n)
        qkv, _, _, got = _attn_check(dev, 1, 16, 24, 6, 30, shift, 930 + shift, note=" (zero rows)", zeros=True)
        assert not qkv[0, 0, :, :, 0, 0].any() and not qkv[1, 0, :, :, 2, 1].any() and torch.isfinite(got).all()
        _attn_check(dev, 1, 16, 24, 2, 32, shift, 950 + shift, note=" (q / 64, 24 k)", qgain=1.0 / 64, kgain=24.0)
        _attn_check(dev, 1, 8, 16, 8, 30, shift, 960 + shift, note=" (q / 64, 24 k)", qgain=1.0 / 64, kgain=24.0)


def test_cosine_attention_refusals(dev):
    """A bad size, 9 heads, 33 channels, shift 2, a null tau: a status, and nothing written."""
    import innfer_amd.lib as L
    src = torch.zeros(64 * 64 * 32 * 8, dtype=torch.float16, device=dev)
    dst = torch.full((64 * 64 * 32 * 8,), FILL, dtype=torch.float16, device=dev)
    tb, tt = np.zeros((9, 64, 64), np.float32), np.ones(9, np.float32)
    G = 16 * 16 * 32
    call = lambda Hp, Wp, nH, d, shift, tau=tt.ctypes.data: L.lib.innfer_window_attention_cos(src.data_ptr(), G, dst.data_ptr(), G, tb.ctypes.data, tau, 1, Hp, Wp, nH, d, shift, None)
    assert call(16, 12, 2, 32, 0) == L.ERR_INVALID and call(16, 16, 9, 8, 0) == L.ERR_UNSUPPORTED and call(16, 16, 2, 33, 0) == L.ERR_UNSUPPORTED
    assert call(16, 16, 2, 32, 2) == L.ERR_UNSUPPORTED and call(16, 16, 2, 32, 0, None) == L.ERR_INVALID
    torch.cuda.synchronize()
    assert bool((dst == FILL).all()), "a refused launch wrote to its output"
    assert call(16, 16, 2, 32, 4) == 0


# ------------------------------------------------------------------------------------------------ 2. LayerNorm + residual
def _lna_launch(dev, x, res, Cc, gamma, beta, alias=None):
    """x, res: fp16 [N, c_pad, H, W] whose channels >= Cc hold junk.  alias: None (out of place, between guards), 'res' or 'in'.  Returns [N, c_pad, H, W] fp16 (cpu)."""
    import innfer_amd.lib as L
    N, cp, H, W = x.shape
    G, ng = N * H * W * 32, cp // 32
    xin, rin = R.to_slab(x).to(dev), R.to_slab(res).to(dev)
    g, b = np.ascontiguousarray(gamma.numpy(), np.float32), np.ascontiguousarray(beta.numpy(), np.float32)
    if alias:
        out = rin if alias == "res" else xin
        L.check(L.lib.innfer_layer_norm_add(xin.data_ptr(), G, rin.data_ptr(), G, out.data_ptr(), G, N * H * W, Cc, cp, g.ctypes.data, b.ctypes.data, 1e-5, None))
        torch.cuda.synchronize()
        other, kept = (xin, x) if alias == "res" else (rin, res)
        assert torch.equal(other.cpu(), R.to_slab(kept)), "layer norm + residual wrote to the operand it was not given as its output"
        return R.from_slab(out.cpu())
    buf = torch.full(((ng + 1) * G + 2 * GUARD,), FILL, dtype=torch.float16, device=dev)
    L.check(L.lib.innfer_layer_norm_add(xin.data_ptr(), G, rin.data_ptr(), G, buf.data_ptr() + 2 * GUARD, G, N * H * W, Cc, cp, g.ctypes.data, b.ctypes.data, 1e-5, None))
    torch.cuda.synchronize()
    raw = buf.cpu()
    assert bool((raw[:GUARD] == FILL).all()) and bool((raw[GUARD + ng * G:] == FILL).all()), "layer norm + residual wrote outside its output"
    assert torch.equal(xin.cpu(), R.to_slab(x)) and torch.equal(rin.cpu(), R.to_slab(res)), "layer norm + residual wrote to its inputs"
    return R.from_slab(raw[GUARD:GUARD + ng * G].reshape(ng, N, H, W, 32))


@pytest.mark.parametrize("Cc", [60, 180, 240, 64])
def test_layer_norm_add(dev, Cc):
    from innfer_amd import synth
    cp = -(-Cc // 64) * 64
    n_chain = cp // 4 + 2
    for i, (N, H, W) in enumerate([(1, 1, 1), (1, 8, 8), (1, 17, 33), (3, 17, 33)]):
        seed = 7500 + 10 * Cc + i
        x = synth.uniform((N, cp, H, W), seed, -1, 1)
        x = x * synth.uniform((N, 1, H, W), seed + 1, 0.25, 4.0) + synth.uniform((N, 1, H, W), seed + 2, -2.0, 2.0)          # pixels differ in scale and offset
        x[:, Cc:] = 7.0                                                                                                     # junk in the pad channels: ignored
        res = synth.uniform((N, cp, H, W), seed + 5, -4, 4)
        res[:, Cc:] = -5.0
        x, res = torch.from_numpy(np.ascontiguousarray(x, np.float32)).half(), torch.from_numpy(np.ascontiguousarray(res, np.float32)).half()
        gamma, beta = torch.from_numpy(synth.uniform((Cc,), seed + 3, 0.5, 1.5)), torch.from_numpy(synth.uniform((Cc,), seed + 4, -0.2, 0.2))
        x64 = x[:, :Cc].double()
        ln = SR.layer_norm(x64, gamma.double(), beta.double())
        ref = res[:, :Cc].double() + ln
        mu = x64.mean(1, keepdim=True)
        sigma = torch.sqrt(x64.var(1, unbiased=False, keepdim=True) + 1e-5)
        A = x64.abs().amax(1, keepdim=True)
        ga, be = gamma.double().abs()[None, :, None, None], beta.double().abs()[None, :, None, None]
        gz = ga * ((x64 - mu) / sigma).abs()
        ln_stats = 2.0 ** -24 * (((n_chain + 5) / 2 + 7) * gz + (n_chain + 2) * ga * A / sigma + gz + be)
        extra = ln_stats + 2.0 ** -24 * (ln.abs() + ref.abs())
        got = _lna_launch(dev, x, res, Cc, gamma, beta)
        assert bool((got[:, Cc:] == 0).all()), "pad channels of the result are not zero"
        R.assert_within_fp16_rounding(got[:, :Cc], ref, 0.0, extra=extra, what=f"layer norm + residual C {Cc} {N}x{H}x{W}", family=f"layer norm + residual, C {Cc}")
        for alias in ("res", "in"):
            assert torch.equal(_lna_launch(dev, x, res, Cc, gamma, beta, alias=alias).view(torch.int16), got.view(torch.int16)), f"out == {alias} differs from out of place"


def test_layer_norm_add_refusals(dev):
    import innfer_amd.lib as L
    src = torch.zeros(64 * 512, dtype=torch.float16, device=dev)
    dst = torch.full((64 * 512,), FILL, dtype=torch.float16, device=dev)
    g = np.ones(512, np.float32)
    call = lambda Cc, cp, res=src.data_ptr(), gs=64 * 32: L.lib.innfer_layer_norm_add(src.data_ptr(), 64 * 32, res, gs, dst.data_ptr(), 64 * 32, 64, Cc, cp, g.ctypes.data, g.ctypes.data, 1e-5, None)
    assert call(300, 320) == L.ERR_UNSUPPORTED and call(60, 48) == L.ERR_UNSUPPORTED and call(60, 32) == L.ERR_UNSUPPORTED
    assert call(60, 64, None) == L.ERR_INVALID and call(60, 64, gs=63 * 32) == L.ERR_INVALID
    torch.cuda.synchronize()
    assert bool((dst == FILL).all()), "a refused launch wrote to its output"
    assert call(60, 64) == 0


# ------------------------------------------------------------------------------------------------ 3. networks
def _net(dev, sd, wrap=True, with_buffers=False):
    from innfer_amd.architectures import get_network
    from innfer_amd.run import infer_from_state_dict
    if with_buffers:
        sd = dict(sd, **S2.buffers(sd))
    info = infer_from_state_dict({"params_ema": sd} if wrap else sd)
    assert info["arch"] == "swin2sr"
    net = get_network(info["net_params"])
    net.load_state_dict(info["state_dict"], strict=True)
    return net.to(dev).eval()


def _assert_like_storage_model(got, y64, ys, what):
    """max |engine - float64| <= 2 x max |storage model - float64| of the same case (computed here), and >= 99 % of the uint8 codes within +-1."""
    err, es = float((got.double() - y64).abs().max()), float((ys - y64).abs().max())
    share = S2.codes_within_one(got, y64)
    print(f"[swin2sr] {what}: engine max|err| {err:.2e}, storage model {es:.2e}, ratio {err / es:.3f}; codes within +-1: {share:.5f}")
    assert got.shape == y64.shape and torch.isfinite(got).all()
    assert err <= 2 * es, (what, err, es)
    assert share >= 0.99, (what, share)


def launch_formula(Cc, nH, hidden, depths, upsampler, s, resi, padded):
    """SwinIR's: S1 + 2 + B (3 + SQ + 2 S1 + SH) + (R + 1) SR + T + 2 [padded]."""
    S1, SQ, SH = -(-Cc // 64), -(-3 * nH // 2), -(-hidden // 64)
    SR_ = S1 if resi == "1conv" else 2 * -(-Cc // 256) + S1
    lg = {2: 1, 4: 2}.get(s, 0)
    T = {"pixelshuffledirect": 2, "pixelshuffle": 4 if s == 3 else 2 + lg, "nearest+conv": 3 + lg}[upsampler]
    return S1 + 2 + sum(depths) * (3 + SQ + 2 * S1 + SH) + (len(depths) + 1) * SR_ + T + (2 if padded else 0)


def _launches(net, x):
    """Launch count of one forward (innfer_net_forward_timed)."""
    import innfer_amd.lib as L
    N, _, H, W = x.shape
    s = L.lib.innfer_net_scale(net._handle)
    out = torch.empty((N, net.out_nc, H * s, W * s), dtype=torch.float16, device=x.device)
    ws = torch.empty(L.lib.innfer_net_workspace_bytes(net._handle, N, H, W), dtype=torch.uint8, device=x.device)
    n = C.c_int()
    ms = (C.c_float * 1024)()
    L.check(L.lib.innfer_net_forward_timed(net._handle, x.data_ptr(), L.F16, out.data_ptr(), L.F16, N, H, W, ws.data_ptr(), ws.numel(), None, 1024, ms, None, None, None, C.byref(n)))
    return n.value, out


@pytest.mark.parametrize("name", list(S2.FIXTURES))
def test_network_vs_float64(dev, name):
    from innfer_amd import synth
    from innfer_amd.utils import utils as U
    Cc, nH, depths, shape, ups, s, resi, cpb, seed = S2.FIXTURES[name]
    sd, x, y64, ys = S2.case(name)
    net = _net(dev, sd, with_buffers=seed % 2 == 1)
    assert (net.nf, net.num_heads, tuple(net.depths), net.upsampler, net.upscale, net.resi_connection, net.cpb_hidden) == (Cc, nH, tuple(depths), ups, s, resi, cpb)
    xd = x.to(dev).half()
    y = net(xd)
    assert y.dtype == torch.float16 and net._out_shape(shape[0], shape[2], shape[3], dev) == tuple(y64.shape) == tuple(y.shape)
    _assert_like_storage_model(y.float().cpu(), y64, ys, name)
    n, yt = _launches(net, xd)
    assert n == launch_formula(Cc, nH, 2 * Cc, depths, ups, s, resi, shape[2] % 8 != 0 or shape[3] % 8 != 0) and torch.equal(yt, y), n
    buf = torch.empty(y.shape, dtype=torch.float16, device=dev)
    assert net(xd, out=buf) is buf and torch.equal(buf, y)
    if shape[0] > 1:          # nothing in Swin2SR crosses samples
        assert torch.equal(net(xd[1:]), y[1:])
    img = torch.from_numpy(synth.image_u8(shape[2], shape[3], 3, s)).to(dev)
    sep = U.tensor2np(net(U.np2tensor(img.cpu().numpy(), dtype=torch.float16)))
    assert np.array_equal(net.forward_u8(img).cpu().numpy(), sep)
    with pytest.raises(NotImplementedError, match="fp16 mode"):
        net(x.to(dev))
    with pytest.raises(NotImplementedError, match="fp16 mode"):
        net.forward_u8(img, fp16=False)
    assert net.flops(1, shape[2], shape[3]) > 0 and net.tile_batch_bytes(2, 16) > 0


def test_network_refuses_sides_too_short_to_pad(dev):
    sd = S2.fixture_sd("C64 nH2 [2] pixelshuffle x2 8x8")
    net = _net(dev, sd)
    with pytest.raises(NotImplementedError, match="reflection"):
        net(torch.zeros(1, 3, 4, 16, dtype=torch.float16, device=dev))
    assert tuple(net(torch.zeros(1, 3, 5, 16, dtype=torch.float16, device=dev)).shape) == (1, 3, 10, 32)


# ------------------------------------------------------------------------------------------------ 4. the Model
@pytest.fixture(scope="module")
def model(tmp_path_factory):
    from innfer_amd.run import Model
    sd = S2.fill(3, 60, (2,), 6, 2.0, 2, "pixelshuffle", "1conv", 512, seed=8)
    path = str(tmp_path_factory.mktemp("swin2sr") / "2x_swin2sr.pth")
    torch.save({"params": dict(sd, **S2.buffers(sd))}, path)
    m = Model(path, arch="infer", scale=None, device="cuda", chop=True, tile_batch=4)
    assert (m.arch, m.scale, m.in_nc, m.out_nc) == ("swin2sr", 2, 3, 3)
    return m, sd


def test_model_chop(dev, model):
    """250 x 330 through the chop path against the helper run tile by tile (oracle.extract_patches_2d / recompose_tensor; the storage model's blend rounded to fp16 as the
    chop path's is); run_u8 == the separate conversions; a float32 tensor is refused."""
    import oracle
    from innfer_amd import synth
    from innfer_amd.utils import utils as U
    m, sd = model
    x = torch.from_numpy(synth.uniform((1, 3, 250, 330), 52))
    y = m(x.to(dev).half()).float().cpu()
    assert tuple(y.shape) == (1, 3, 500, 660)
    tiles = oracle.extract_patches_2d(x, (200, 200), [0.5, 0.5], batch_first=True).squeeze(0)
    h64 = torch.cat([S2.forward64(sd, tiles[i:i + 1], 2, "pixelshuffle") for i in range(tiles.shape[0])], 0)
    hs = torch.cat([S2.forward_storage(sd, tiles[i:i + 1], 2, "pixelshuffle") for i in range(tiles.shape[0])], 0)
    y64 = oracle.recompose_tensor(h64, 250, 330, step=0.5, scale=2).double()
    ys = oracle.recompose_tensor(hs, 250, 330, step=0.5, scale=2).half().double()
    _assert_like_storage_model(y, y64, ys, "Model chop x2 250x330")
    img = synth.image_u8(250, 330, 3, 9)
    assert np.array_equal(m.run_u8(img), U.tensor2np(m(U.np2tensor(img, dtype=torch.float16))))
    with pytest.raises(NotImplementedError, match="fp16 mode"):
        m(x.to(dev))


def test_model_run_u8_options(dev, model):
    """plain, tile=, tta, seamless='tile' and run_u8_batch on a Swin2SR model: each equals the definition its docstring gives for it, bit for bit (images <= 96 px)."""
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
    mt = Model(None, arch="infer", scale=None, device="cuda", chop=True, tile_batch=4, state_dict={"params": sd}, tile=32, tile_pad=8)
    big = synth.image_u8(70, 96, 3, 64)
    assert np.array_equal(mt.run_u8(big), U.tensor2np(mt(U.np2tensor(big, dtype=torch.float16))))
