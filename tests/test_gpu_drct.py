"""DRCT on the GPU (needs an MI355X: `pytest -m gpu`): the wide-head 16 x 16 window attention and the holed LayerNorm alone, whole networks, the Model.  Every launch writes
between guard bands that must keep their fill; inputs must be unchanged.

1. innfer_window_attention16_wide against float64 on the stored fp16 operands (tests/test_gpu_hat.py's harness): padded sizes 16x16 (the one window wraps onto itself under
   shift 8), 32x48 and 48x48 (one window without a border), shifts 0 and 8, (nH, d) = (4, 53), (2, 122), (4, 77), (6, 46), (1, 128), (2, 33), (3, 64), (1, 96) -- every
   G = ceil(d / 32), d at and just over each group boundary, odd d; a batch of 2 whose samples differ, each bit-equal to its own N = 1 launch; one case with scores of some
   +-250.  The bound is ulp16 / 2 + 8 e_model, e_model = max |model - exact| of a float32 torch model of the kernel's DECLARED arithmetic (float32 scores, the keys walked
   in blocks of 64 with a running maximum and sum, P rounded to fp16 as the operand of P v, float32 accumulation and division), computed on the CPU, never from the kernel.
   Pad channels of the output are exactly zero.  The refusals (d 32, d 129, Hp 24, shift 4): a status and nothing written.
2. innfer_layer_norm_holed against float64 LayerNorm over the REAL channels of the dense slab -- [0, C) and [32 ceil(C / 32), c_end): C 180 with 1 .. 4 extra groups, C 60
   (the hole 60 .. 63) with 1 and 4; the hole and the pads hold junk on input (NaN and Inf among it) and are written as zeros; in place == out of place bit for bit.  The
   bound is test_gpu_swinir.py's LN_STATS with n = c_pad / 4 + 2.  The existing entries are unchanged by the new template argument: innfer_layer_norm and
   innfer_layer_norm_wide give, bit for bit, what a float32 model of the kernel's order of operations gives (computed here: the lane's groups in order, the quad's
   butterfly, fma where the source says so) -- and the holed form with an empty hole gives the same bits.
3. Networks against the float64 forward of tests/_drct_ref.py: max |err| <= 2 x the fp16 storage model's own error on the same case and >= 99 % of the uint8 codes within
   +-1 (3.4m's criterion); the launch count equals the formula of DESIGN.md 3.4p; out= is honoured; a batch's sample equals its own forward bit for bit; forward_u8 ==
   the separate conversions; a float32 tensor is refused; a forward is bit-identical on a repeat and on a workspace pre-filled with NaN bit patterns (no group of the dense
   slab is read before it is written).
   Measured on the MI355X, engine max |err| / storage model max |err| (100 % of the codes within +-1 in every case):
       C60 R2 x2 13x21 (padded) 1.000 | C180 R1 x4 32x48 0.966 | C96 R1 x3 batch of two 19x26 1.088
   Measured worst err / bound of the single launches: the wide attention 0.20 .. 0.34 (scores beyond +-300 included), the holed LayerNorm 0.96 .. 0.99 (the fp16 rounding
   dominates).
4. Model(arch='infer', chop=True) from a .pth under params_ema (with the buffers) on a 250 x 330 image against the network run tile by tile and blended by the oracle's
   helper; run_u8_batch equals per-image runs; a side too short to pad is refused.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import _conv_ref as R
import _drct_ref as DR
import _hat_ref as HR

pytestmark = pytest.mark.gpu

FILL, GUARD = -3.0, 4096

@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


# ------------------------------------------------------------------------------------------------ 1. the wide window attention
def _attn_data(N, Hp, Wp, nH, d, seed, gain=1.0):
    """q, k, v as fp16 [3, N, nH, d, Hp, Wp] (the values of the slab's real channels; q and k shrink with sqrt(32 / d) so that scores keep the spread they have at d = 32)
    and the dense bias table [nH, 256, 256] float32; samples of a batch differ."""
    from innfer_amd import synth
    qkv = synth.uniform((3, N, nH, d, Hp, Wp), 6500 + seed, -1, 1)
    for n in range(N):
        qkv[:, n] *= np.float32(1.0 + 0.5 * n)
    qkv[:2] *= np.float32((32.0 / d) ** 0.25)
    qkv[0] *= np.float32(gain)
    table = synth.uniform((nH, 256, 256), 6501 + seed, -2, 2)
    return torch.from_numpy(qkv).half(), torch.from_numpy(np.ascontiguousarray(table))


def _attn_ref(qkv, table, shift, dt, model=False):
    """softmax(q k^T + B + M) v per window and head in dtype dt; model: the kernel's declared arithmetic (blocks of 64 keys, running maximum and sum, P rounded to fp16)."""
    _, N, nH, d, Hp, Wp = qkv.shape
    x = qkv.to(dt).reshape(3, N, nH * d, Hp, Wp)
    heads = lambda w: w.reshape(w.shape[0], w.shape[1], w.shape[2], nH, d).permute(0, 1, 3, 2, 4)          # [N, nW, T, C] -> [N, nW, nH, T, d]
    xs = torch.roll(x, (-shift, -shift), (3, 4)) if shift else x
    q, k, v = (heads(HR._windows(xs[i])) for i in range(3))
    S = q @ k.transpose(-1, -2) + table.to(dt)
    if shift:
        S = S + HR.shift_mask(Hp, Wp).to(dt)[None, :, None]
    if model:
        m = torch.full(S.shape[:-1] + (1,), -3.0e38, dtype=dt)
        l = torch.zeros_like(m)
        o = torch.zeros(S.shape[:-1] + (d,), dtype=dt)
        for b in range(0, 256, 64):
            sb = S[..., b:b + 64]
            mn = torch.maximum(m, sb.amax(-1, keepdim=True))
            alpha = torch.exp(m - mn)
            e = torch.exp(sb - mn)
            l = l * alpha + e.sum(-1, keepdim=True)
            o = o * alpha + e.half().to(dt) @ v[..., b:b + 64, :]
            m = mn
        o = o / l
    else:
        o = torch.softmax(S, -1) @ v
    o = HR._unwindows(o.permute(0, 1, 3, 2, 4).reshape(N, -1, 256, nH * d), Hp, Wp)
    if shift:
        o = torch.roll(o, (shift, shift), (2, 3))
    return o.reshape(N, nH, d, Hp, Wp), float(S.abs().max())


def _wide_slab(qkv):
    """[3, N, nH, d, Hp, Wp] -> the slab [3, nH, G, N, Hp, Wp, 32]: head h of q / k / v in G = ceil(d / 32) consecutive groups, d real channels, then zeros."""
    _, N, nH, d, Hp, Wp = qkv.shape
    Gh = -(-d // 32)
    pad = torch.zeros(3, N, nH, 32 * Gh, Hp, Wp, dtype=torch.float16)
    pad[:, :, :, :d] = qkv
    return pad.reshape(3, N, nH, Gh, 32, Hp, Wp).permute(0, 2, 3, 1, 5, 6, 4).contiguous()


def _attn_launch(dev, qkv, table, shift):
    """innfer_window_attention16_wide from a slab of its own into [guard | nH G groups | a foreign group | guard].  Returns [N, nH, 32 G, Hp, Wp] fp16 (cpu)."""
    import innfer_amd.lib as L
    _, N, nH, d, Hp, Wp = qkv.shape
    Gh, G = -(-d // 32), N * Hp * Wp * 32
    slab = _wide_slab(qkv)
    xin = slab.to(dev)
    buf = torch.full(((nH * Gh + 1) * G + 2 * GUARD,), FILL, dtype=torch.float16, device=dev)
    tb = np.ascontiguousarray(table.numpy(), np.float32)
    L.check(L.lib.innfer_window_attention16_wide(xin.data_ptr(), G, buf.data_ptr() + 2 * GUARD, G, tb.ctypes.data, N, Hp, Wp, nH, d, shift, None))
    torch.cuda.synchronize()
    raw = buf.cpu()
    assert bool((raw[:GUARD] == FILL).all()) and bool((raw[GUARD + nH * Gh * G:] == FILL).all()), "wide window attention wrote outside its output"
    assert torch.equal(xin.cpu(), slab), "wide window attention wrote to its input"
    return raw[GUARD:GUARD + nH * Gh * G].reshape(nH, Gh, N, Hp, Wp, 32).permute(2, 0, 1, 5, 3, 4).reshape(N, nH, 32 * Gh, Hp, Wp)


def _attn_check(dev, N, Hp, Wp, nH, d, shift, seed, gain=1.0, smin=0.0):
    qkv, table = _attn_data(N, Hp, Wp, nH, d, seed, gain)
    ref, smax = _attn_ref(qkv, table, shift, torch.float64)
    assert smax >= smin, (smax, smin)
    e_model = float((_attn_ref(qkv, table, shift, torch.float32, model=True)[0].double() - ref).abs().max())
    got = _attn_launch(dev, qkv, table, shift)
    assert bool((got[:, :, d:] == 0).all()), "pad channels of the attention's result are not zero"
    what = f"wide window attention {N}x{Hp}x{Wp} nH {nH} d {d} shift {shift} (|S| up to {smax:.0f})"
    R.assert_within_fp16_rounding(got[:, :, :d], ref, e_model, what=what, family=f"wide window attention 16, G {-(-d // 32)}, shift {shift}")
    return qkv, table, got


@pytest.mark.parametrize("nH,d", [(4, 53), (2, 122), (4, 77), (6, 46), (1, 128), (2, 33), (3, 64), (1, 96)])
def test_window_attention16_wide(dev, nH, d):
    for i, (Hp, Wp) in enumerate([(16, 16), (32, 48), (48, 48)]):
        for shift in (0, 8):
            _attn_check(dev, 1, Hp, Wp, nH, d, shift, 100 * nH + d + 10 * i + shift)


@pytest.mark.parametrize("nH,d", [(4, 53), (2, 122)])
def test_window_attention16_wide_batch_and_large_scores(dev, nH, d):
    """A window of sample n reads only sample n: each sample of a batch of two equals its own launch bit for bit; scores of some +-250 stay finite and inside the bound."""
    for shift in (0, 8):
        qkv, table, got = _attn_check(dev, 2, 16, 32, nH, d, shift, 900 + shift + d)
        for n in range(2):
            one = _attn_launch(dev, qkv[:, n:n + 1].contiguous(), table, shift)
            assert torch.equal(one.view(torch.int16), got[n:n + 1].contiguous().view(torch.int16)), (shift, n)
        _attn_check(dev, 1, 16, 32, nH, d, shift, 950 + shift + d, gain=24.0, smin=200.0)


def test_window_attention16_wide_refusals(dev):
    """Refused with nothing launched: the output keeps its fill."""
    import innfer_amd.lib as L
    G = 32 * 32 * 32
    qkv = torch.zeros(3 * 2 * 4 * G + 3 * 5 * G, dtype=torch.float16, device=dev)
    out = torch.full((10 * G,), FILL, dtype=torch.float16, device=dev)
    tb = np.zeros((2, 256, 256), np.float32)
    call = lambda Hp, Wp, nH, d, shift, gs=G, q=qkv.data_ptr(): L.lib.innfer_window_attention16_wide(q, gs, out.data_ptr(), G, tb.ctypes.data, 1, Hp, Wp, nH, d, shift, None)
    assert call(32, 32, 2, 32, 0) == L.ERR_UNSUPPORTED and call(32, 32, 2, 129, 0) == L.ERR_UNSUPPORTED
    assert call(24, 32, 2, 64, 0) == L.ERR_INVALID and call(32, 24, 2, 64, 0) == L.ERR_INVALID
    assert call(32, 32, 2, 64, 4) == L.ERR_UNSUPPORTED and call(32, 32, 9, 64, 0) == L.ERR_UNSUPPORTED
    assert call(32, 32, 2, 64, 0, gs=G - 32) == L.ERR_INVALID and call(32, 32, 2, 64, 0, q=None) == L.ERR_INVALID
    torch.cuda.synchronize()
    assert bool((out == FILL).all())
    assert call(32, 32, 2, 64, 8) == 0


# ------------------------------------------------------------------------------------------------ 2. the holed LayerNorm
def _hln_launch(dev, x, Cc, c_end, gamma, beta, in_place=False, entry="innfer_layer_norm_holed"):
    """x: fp16 [N, c_pad, H, W] in SLAB order whose hole and pads hold junk; gamma / beta: c_pad floats in slab order.  Returns [N, c_pad, H, W] fp16 (cpu)."""
    import innfer_amd.lib as L
    N, cp, H, W = x.shape
    G, ng = N * H * W * 32, cp // 32
    xin = R.to_slab(x).to(dev)
    g, b = np.ascontiguousarray(gamma.numpy(), np.float32), np.ascontiguousarray(beta.numpy(), np.float32)

    def go(dst):
        if entry == "innfer_layer_norm_holed":
            L.check(L.lib.innfer_layer_norm_holed(xin.data_ptr(), G, dst, G, N * H * W, Cc, c_end, cp, g.ctypes.data, b.ctypes.data, 1e-5, None))
        else:
            L.check(getattr(L.lib, entry)(xin.data_ptr(), G, dst, G, N * H * W, Cc, cp, g.ctypes.data, b.ctypes.data, 1e-5, None))
        torch.cuda.synchronize()
    if in_place:
        go(xin.data_ptr())
        return R.from_slab(xin.cpu())
    buf = torch.full(((ng + 1) * G + 2 * GUARD,), FILL, dtype=torch.float16, device=dev)
    go(buf.data_ptr() + 2 * GUARD)
    raw = buf.cpu()
    assert bool((raw[:GUARD] == FILL).all()) and bool((raw[GUARD + ng * G:] == FILL).all()), "layer norm wrote outside its output"
    assert torch.equal(xin.cpu().view(torch.int16), R.to_slab(x).view(torch.int16)), "layer norm wrote to its input"
    return R.from_slab(raw[GUARD:GUARD + ng * G].reshape(ng, N, H, W, 32))


def _ln_data(N, cp, H, W, seed):
    from innfer_amd import synth
    x = synth.uniform((N, cp, H, W), seed, -1, 1)
    x = x * synth.uniform((N, 1, H, W), seed + 1, 0.25, 4.0) + synth.uniform((N, 1, H, W), seed + 2, -2.0, 2.0)          # pixels differ in scale and offset
    g, b = synth.uniform((cp,), seed + 3, 0.5, 1.5), synth.uniform((cp,), seed + 4, -0.2, 0.2)
    return np.ascontiguousarray(x, np.float32), torch.from_numpy(g), torch.from_numpy(b)


@pytest.mark.parametrize("Cc,extra", [(180, 1), (180, 2), (180, 3), (180, 4), (60, 1), (60, 4)])
def test_layer_norm_holed(dev, Cc, extra):
    h1 = -(-Cc // 32) * 32
    c_end = h1 + 32 * extra
    cp = -(-c_end // 64) * 64
    real = torch.tensor([c < Cc or h1 <= c < c_end for c in range(cp)])
    n_chain = cp // 4 + 2
    for i, (N, H, W) in enumerate([(1, 1, 1), (1, 17, 33), (2, 9, 21)]):
        seed = 7300 + 10 * Cc + 100 * extra + i
        x, gamma, beta = _ln_data(N, cp, H, W, seed)
        junk = np.array([7.0, np.nan, np.inf, -np.inf, 65504.0, -3.0], np.float32)
        x[:, ~real.numpy()] = junk[np.arange(int((~real).sum())) % len(junk)][None, :, None, None]          # the hole and the pads: never in the statistics
        x = torch.from_numpy(x).half()
        x64 = x[:, real].double()
        ga, be = gamma[real].double(), beta[real].double()
        ref = HR.layer_norm(x64, ga, be)
        mu = x64.mean(1, keepdim=True)
        sigma = torch.sqrt(x64.var(1, unbiased=False, keepdim=True) + 1e-5)
        A = x64.abs().amax(1, keepdim=True)
        gab, beb = ga.abs()[None, :, None, None], be.abs()[None, :, None, None]
        gz = gab * ((x64 - mu) / sigma).abs()
        ln_stats = 2.0 ** -24 * (((n_chain + 5) / 2 + 7) * gz + (n_chain + 2) * gab * A / sigma + gz + beb)
        got = _hln_launch(dev, x, Cc, c_end, gamma, beta)
        assert bool((got[:, ~real] == 0).all()), "the hole and the pads of the layer norm's result are not zero"
        R.assert_within_fp16_rounding(got[:, real], ref, 0.0, extra=ln_stats, what=f"holed layer norm C {Cc} + {extra} groups {N}x{H}x{W}", family=f"holed layer norm, C {Cc}")
        assert torch.equal(_hln_launch(dev, x, Cc, c_end, gamma, beta, in_place=True).view(torch.int16), got.view(torch.int16)), "in place differs from out of place"


def _ln_model32(x, Cc, gamma, beta):
    """layer_norm_kernel's float32 arithmetic in its own order, as hipcc contracts it (-ffp-contract=fast, read off the gfx950 code), on the CPU: lane q of a pixel's quad
    owns channels 8 q .. 8 q + 7 of every group; s += x over its groups in order, then the butterfly (+ lane q ^ 1, then + lane q ^ 2); d = fma(-(1 / C), s, x) -- the mean
    is never rounded on its own --; s = fma(d, d, s) in the same order and the same butterfly; rstd = 1 / sqrtf(fma(s, 1 / C, eps)), division and root correctly rounded;
    out = fma(d * rstd, gamma, beta) with ONE rounding, from the exact fma straight to fp16 (v_fma_mixlo_f16).  fma(a, b, c) is float32(float64(a) float64(b) + float64(c)):
    the product of two float32 values is exact in float64."""
    f32 = np.float32
    N, cp, H, W = x.shape
    v = x.float().permute(0, 2, 3, 1).reshape(-1, cp // 32, 4, 8).numpy()                       # [pixel, group, lane, element]
    chan = (np.arange(cp // 32)[:, None, None] * 32 + np.arange(4)[None, :, None] * 8 + np.arange(8)[None, None, :])
    ok = chan < Cc
    fma = lambda a, b, c: (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(f32)

    def quad(s):                                                                               # s [pixel, lane]
        s = s + s[:, [1, 0, 3, 2]]
        return s + s[:, [2, 3, 0, 1]]
    s = np.zeros(v.shape[:1] + (4,), f32)
    for g in range(cp // 32):
        for e in range(8):
            s = np.where(ok[g, :, e][None, :], s + v[:, g, :, e], s)
    rc = f32(1.0) / f32(Cc)
    qs = quad(s)
    d = fma(-rc, qs[:, None, :, None], v)                                                      # x - mean, one rounding
    s = np.zeros_like(s)
    for g in range(cp // 32):
        for e in range(8):
            s = np.where(ok[g, :, e][None, :], fma(d[:, g, :, e], d[:, g, :, e], s), s)
    rstd = f32(1.0) / np.sqrt(fma(quad(s), rc, f32(1e-5)))
    gam = np.zeros(cp, f32); gam[:len(gamma)] = gamma.numpy()
    bet = np.zeros(cp, f32); bet[:len(beta)] = beta.numpy()
    z = (d * rstd[:, None, :, None]).astype(f32)
    y = (z.astype(np.float64) * gam[chan][None].astype(np.float64) + bet[chan][None].astype(np.float64)).astype(np.float16)
    y = np.where(ok[None], y, np.float16(0.0))
    return torch.from_numpy(np.ascontiguousarray(y)).reshape(N, H, W, cp).permute(0, 3, 1, 2).contiguous()


def test_existing_layer_norm_entries_keep_their_bits(dev):
    """The new template argument leaves the instantiations of the existing entries alone: on one shared case innfer_layer_norm and innfer_layer_norm_wide give what the
    float32 model of the kernel gives, bit for bit -- and so does the holed form when the hole is empty (C = 192: no hole, nothing behind it)."""
    for entry, Cc, cp in (("innfer_layer_norm", 180, 192), ("innfer_layer_norm_wide", 300, 320), ("innfer_layer_norm", 192, 192)):
        x, gamma, beta = _ln_data(2, cp, 9, 21, 7900 + Cc)
        x[:, Cc:] = 7.0
        x = torch.from_numpy(x).half()
        want = _ln_model32(x, Cc, gamma[:Cc], beta[:Cc])
        got = _hln_launch(dev, x, Cc, 0, gamma[:Cc], beta[:Cc], entry=entry)
        assert torch.equal(got.view(torch.int16), want.view(torch.int16)), (entry, Cc, int((got.view(torch.int16) != want.view(torch.int16)).sum()))
        if Cc == cp:
            holed = _hln_launch(dev, x, Cc, cp, gamma, beta)
            assert torch.equal(holed.view(torch.int16), want.view(torch.int16)), "the holed form with an empty hole differs from the plain one"


# ------------------------------------------------------------------------------------------------ 3. networks
def _net(dev, name):
    from innfer_amd.architectures import get_network
    from innfer_amd.run import infer_from_state_dict
    info = infer_from_state_dict({"params_ema": DR.fixture_sd(name)})
    net = get_network(dict(info["net_params"]))
    net.load_state_dict(info["state_dict"], strict=True)
    return net.to(dev).eval()


def _assert_like_storage_model(got, y64, ys, what):
    """max |engine - float64| <= 2 x max |storage model - float64| of the same case (computed here), and >= 99 % of the uint8 codes within +-1."""
    err, es = float((got.double() - y64).abs().max()), float((ys - y64).abs().max())
    share = DR.codes_within_one(got, y64)
    print(f"[drct] {what}: engine max|err| {err:.2e}, storage model {es:.2e}, ratio {err / es:.3f}; codes within +-1: {share:.5f}")
    assert got.shape == y64.shape and torch.isfinite(got).all()
    assert err <= 2 * es, (what, err, es)
    assert share >= 0.99, (what, share)


def launch_formula(Cc, heads, hidden, s, padded):
    """2 S1 + 2 + sum over blocks (3 + SQ + 2 S + SH + A) + T + 2 [padded]; S1 = C_pad / 64, per block k = 0 .. 4 of its group S = lp_k / 64 with
    lp_k = 32 (ceil(C / 32) + k) rounded up to 64, SQ = ceil(3 nH G / 2), SH = hidden_pad / 64, A = 1 (k < 4) | S1 (k = 4); T = 2 + log2(s) (4 for s = 3)."""
    S1, gx = -(-Cc // 64), -(-Cc // 32)
    n = 2 * S1 + 2 + (4 if s == 3 else 2 + {2: 1, 4: 2}[s]) + (2 if padded else 0)
    for blk, (nh, hid) in enumerate(zip(heads, hidden)):
        k = blk % 5
        G = -(-((Cc + 32 * k) // nh) // 32)
        n += 3 + -(-3 * nh * G // 2) + 2 * -(-(gx + k) // 2) + -(-hid // 64) + (1 if k < 4 else S1)
    return n


def _forward_raw(net, x, ws=None):
    """One innfer_net_forward_timed on a workspace of the caller's (None: a fresh one): (launch count, result)."""
    import innfer_amd.lib as L
    N, _, H, W = x.shape
    s = L.lib.innfer_net_scale(net._handle)
    out = torch.empty((N, net.out_nc, H * s, W * s), dtype=torch.float16, device=x.device)
    if ws is None:
        ws = torch.empty(L.lib.innfer_net_workspace_bytes(net._handle, N, H, W), dtype=torch.uint8, device=x.device)
    n = C.c_int()
    ms = (C.c_float * 2048)()
    L.check(L.lib.innfer_net_forward_timed(net._handle, x.data_ptr(), L.F16, out.data_ptr(), L.F16, N, H, W, ws.data_ptr(), ws.numel(), None, 2048, ms, None, None, None, C.byref(n)))
    return n.value, out


@pytest.mark.parametrize("name", list(DR.FIXTURES))
def test_network_vs_float64(dev, name):
    import innfer_amd.lib as L
    from innfer_amd import synth
    from innfer_amd.utils import utils as U
    Cc, nH, R, shape, s, stored, seed = DR.FIXTURES[name]
    sd, x, y64, ys, st = DR.case(name)
    net = _net(dev, name)
    heads = [DR.head_rule(Cc + 32 * k, nH) for _ in range(R) for k in range(5)]
    hidden = [2 * (Cc + 32 * k) for _ in range(R) for k in range(5)]
    assert (net.nf, net.n_groups, net.upscale, net.block_heads, net.block_hidden) == (Cc, R, s, heads, hidden)
    xd = x.to(dev).half()
    y = net(xd)
    assert y.dtype == torch.float16 and net._out_shape(shape[0], shape[2], shape[3], dev) == tuple(y64.shape) == tuple(y.shape)
    _assert_like_storage_model(y.float().cpu(), y64, ys, name)
    padded = shape[2] % 16 != 0 or shape[3] % 16 != 0
    n, yt = _forward_raw(net, xd)
    assert n == launch_formula(Cc, heads, hidden, s, padded) == net.launches(padded) and torch.equal(yt, y), n
    assert torch.equal(net(xd), y), "a forward is not bit-identical on a repeat"
    # no group of the dense slab (nor anything else in the workspace) is read before it is written: a workspace full of NaN bit patterns gives the same bits
    nb = L.lib.innfer_net_workspace_bytes(net._handle, shape[0], shape[2], shape[3])
    ws = torch.full((nb // 2 + 1,), float("nan"), dtype=torch.float16, device=dev).view(torch.uint8)
    assert torch.equal(_forward_raw(net, xd, ws)[1], y), "a workspace pre-filled with NaN changes the result"
    ws = torch.full((nb // 2 + 1,), -1, dtype=torch.int16, device=dev).view(torch.uint8)          # (0xffff: another NaN pattern)
    assert torch.equal(_forward_raw(net, xd, ws)[1], y)
    buf = torch.empty(y.shape, dtype=torch.float16, device=dev)
    assert net(xd, out=buf) is buf and torch.equal(buf, y)
    if shape[0] > 1:          # nothing in DRCT crosses samples
        assert torch.equal(net(xd[1:]), y[1:]) and torch.equal(net(xd[:1]), y[:1])
    img = torch.from_numpy(synth.image_u8(shape[2], shape[3], 3, s)).to(dev)
    sep = U.tensor2np(net(U.np2tensor(img.cpu().numpy(), dtype=torch.float16)))
    assert np.array_equal(net.forward_u8(img).cpu().numpy(), sep)
    with pytest.raises(NotImplementedError, match="fp16 mode"):
        net(x.to(dev))
    with pytest.raises(NotImplementedError, match="fp16 mode"):
        net.forward_u8(img, fp16=False)
    assert net.flops(1, shape[2], shape[3]) > 0 and net.tile_batch_bytes(2, 16) > 0


def test_network_refuses_sides_too_short_to_pad(dev):
    net = _net(dev, "C96 R1 x3 batch of two 19x26")
    with pytest.raises(NotImplementedError, match="reflection"):
        net(torch.zeros(1, 3, 8, 16, dtype=torch.float16, device=dev))
    assert tuple(net(torch.zeros(1, 3, 9, 16, dtype=torch.float16, device=dev)).shape) == (1, 3, 27, 48)


# ------------------------------------------------------------------------------------------------ 4. the Model
@pytest.fixture(scope="module")
def model(tmp_path_factory):
    from innfer_amd.run import Model
    sd = DR.fill(3, 60, 1, 6, 2.0, 2, seed=8)
    path = str(tmp_path_factory.mktemp("drct") / "2x_drct.pth")
    torch.save({"params_ema": dict(sd, **DR.buffers(sd))}, path)
    m = Model(path, arch="infer", scale=None, device="cuda", chop=True, tile_batch=4)
    assert (m.arch, m.scale, m.in_nc, m.out_nc) == ("drct", 2, 3, 3)
    return m


def test_model_chop(dev, model):
    """250 x 330 through the chop path (200-px tiles) against the network run tile by tile and the oracle's blend of those fp16 tiles, rounded to fp16 as the chop path's
    is: the two differ in the blend's arithmetic alone -- one fp16 rounding of a value below 2.  run_u8 == the separate conversions; a float32 tensor is refused."""
    import oracle
    from innfer_amd import synth
    from innfer_amd.utils import utils as U
    m = model
    x = torch.from_numpy(synth.uniform((1, 3, 250, 330), 52))
    y = m(x.to(dev).half()).float().cpu()
    assert tuple(y.shape) == (1, 3, 500, 660)
    tiles = oracle.extract_patches_2d(x, (200, 200), [0.5, 0.5], batch_first=True).squeeze(0)
    ht = torch.cat([m.model(tiles[i:i + 1].to(dev).half()).float().cpu() for i in range(tiles.shape[0])], 0)
    want = oracle.recompose_tensor(ht, 250, 330, step=0.5, scale=2).half().float()
    assert float((y - want).abs().max()) <= 2.0 ** -10, float((y - want).abs().max())
    img = synth.image_u8(250, 330, 3, 9)
    assert np.array_equal(m.run_u8(img), U.tensor2np(m(U.np2tensor(img, dtype=torch.float16))))
    with pytest.raises(NotImplementedError, match="fp16 mode"):
        m(x.to(dev))


def test_model_run_u8_batch_and_short_side(dev, model):
    from innfer_amd import synth
    m = model
    imgs = [synth.image_u8(40, 56, 3, 61), synth.image_u8(33, 96, 3, 62), synth.image_u8(64, 17, 3, 63)]
    for a, b in zip(m.run_u8_batch(imgs), [m.run_u8(i) for i in imgs]):
        assert np.array_equal(a, b)
    with pytest.raises(NotImplementedError, match="reflection"):
        m.run_u8(synth.image_u8(8, 40, 3, 64))
