"""HAT on the GPU (needs an MI355X: `pytest -m gpu`): the 16 x 16 window attention over both key windows, the channel attention's launches and the GELU epilogue of the 3x3
conv alone, whole networks, the Model.  Every launch writes between guard bands that must keep their fill; inputs must be unchanged.

1. innfer_window_attention16 against float64 on the stored fp16 operands, key window 16 (shift 0 and 8; at 16x16 the one window wraps onto itself) and 24 (zeros in k and v
   outside the grid, such keys inside the softmax): padded sizes 16x16, 32x48, and 48x48 (one window without a border); (nH, d) = (6, 30), (6, 24), (2, 32), (8, 10); a batch
   of 2 whose samples differ, each bit-equal to its own N = 1 launch; one case with scores of some +-250.  The bound is tests/test_gpu_swinir.py's, ulp16 / 2 + 8 e_model,
   re-derived for this kernel: e_model = max |model - exact| of a float32 torch model of the kernel's DECLARED arithmetic -- float32 scores (q k^T + B, then + M), the keys
   walked in blocks of 64 with a running maximum m and sum l (m' = max(m, block maximum); l and the accumulator times exp(m - m')), P = exp(s - m') rounded to fp16 as the
   operand of P v, float32 accumulation and division -- computed on the CPU, never from the kernel.  Pad channels of the output are exactly zero.
2. innfer_chan_attn_excite / innfer_chan_attn_scale_add against float64 on slabs whose pad channels hold junk: 5x7, 40x50 (two segments) and a batch of two 33x47 (more
   than one segment, a ragged last one).  The sums: |err| <= (n + 1) u sum |z| with u = 2^-24 and n = 16 + 4 + 3 + segments the longest chain of float32 additions (a
   thread's pixels, the butterfly, the waves, the merge).  y: 8 e_model + 2^-22, e_model that of a float32 torch model (the float32 exponential and division cost a few u
   of a value below 1).  The scale-add, given the y the GPU computed: one fp16 rounding + 8 e32.  Bit-identical on a repeat, and per sample in a batch.
3. act 13 (innfer_conv3x3_f16, the plain 3x3 form, 64 -> 64 and 192 -> 64) with act 12's bound (tests/test_gpu_swinir.py: extra = |f| GELU_T, GELU_T = 2^-20): ragged
   edges, a batch, a whole-group channel offset.  The refusals: status and nothing written.
4. Networks against the float64 forward of tests/_hat_ref.py: max |err| <= 2 x the fp16 storage model's own error on the same case and >= 99 % of the uint8 codes within
   +-1; the launch count equals the formula of DESIGN.md 3.4m; out= is honoured; a batch's sample equals its own forward bit for bit; forward_u8 == the separate
   conversions; a float32 tensor is refused.
   Measured on the MI355X, engine max |err| / storage model max |err| (100 % of the codes within +-1 in every case):
       C60 [2] x2 16x16 1.176 | C60 [1,1] x4 13x21 (padded) 1.051 | C180 [2] x3 32x48 0.937 | C144 [2] x2 batch of two 19x26 0.994 | C60 [2] x2 48x48 1.072
   Measured worst err / bound of the single launches: scale-add 0.997 .. 0.999, act 13 0.929 .. 0.989 (the fp16 rounding dominates); y |err| <= 5.4e-7.
5. Model(arch='infer', chop=True) from a .pth under params_ema (with the two index buffers) on a 250 x 330 image against the network run tile by tile and blended by the
   oracle's helper; run_u8_batch equals per-image runs; a side too short to pad is refused.
"""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _conv_ref as R
import _hat_ref as HR
from _conv_ref import Case

pytestmark = pytest.mark.gpu

FILL, GUARD = -3.0, 4096
GELU_T = 2.0 ** -20
S16 = [(1, 1, 1), (1, 16, 32), (1, 17, 33), (1, 50, 70), (3, 37, 45)]          # the 16 x 32-tile edges, and a batch


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


# ------------------------------------------------------------------------------------------------ 1. the window attention
def _attn_data(N, Hp, Wp, nH, d, kw, seed, gain=1.0):
    """q, k, v as fp16 [3, N, nH, d, Hp, Wp] (the values of the slab's real channels) and the dense bias table [nH, 256, kw^2] float32; samples of a batch differ."""
    from innfer_amd import synth
    qkv = synth.uniform((3, N, nH, d, Hp, Wp), 6000 + seed, -1, 1)
    for n in range(N):
        qkv[:, n] *= np.float32(1.0 + 0.5 * n)
    qkv[0] *= np.float32(gain)
    table = synth.uniform((nH, 256, kw * kw), 6001 + seed, -2, 2)
    return torch.from_numpy(qkv).half(), torch.from_numpy(np.ascontiguousarray(table))


def _attn_ref(qkv, table, shift, kw, dt, model=False):
    """softmax(q k^T + B + M) v per window and head in dtype dt; model: the kernel's declared arithmetic (blocks of 64 keys, running maximum and sum, P rounded to fp16)."""
    _, N, nH, d, Hp, Wp = qkv.shape
    x = qkv.to(dt).reshape(3, N, nH * d, Hp, Wp)
    heads = lambda w: w.reshape(w.shape[0], w.shape[1], w.shape[2], nH, d).permute(0, 1, 3, 2, 4)          # [N, nW, T, C] -> [N, nW, nH, T, d]
    if kw == 16:
        xs = torch.roll(x, (-shift, -shift), (3, 4)) if shift else x
        q, k, v = (heads(HR._windows(xs[i])) for i in range(3))
    else:
        q = heads(HR._windows(x[0]))
        k, v = (heads(HR.overlap_kv(x[i])[0]) for i in (1, 2))
    S = q @ k.transpose(-1, -2) + table.to(dt)
    if kw == 16 and shift:
        S = S + HR.shift_mask(Hp, Wp).to(dt)[None, :, None]
    if model:
        m = torch.full(S.shape[:-1] + (1,), -3.0e38, dtype=dt)
        l = torch.zeros_like(m)
        o = torch.zeros(S.shape[:-1] + (d,), dtype=dt)
        for b in range(0, kw * kw, 64):
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
    if kw == 16 and shift:
        o = torch.roll(o, (shift, shift), (2, 3))
    return o.reshape(N, nH, d, Hp, Wp), float(S.abs().max())


def _attn_launch(dev, qkv, table, shift, kw):
    """innfer_window_attention16 from a head-padded slab of its own into [guard | nH groups | a foreign group | guard].  Returns [N, nH, 32, Hp, Wp] fp16 (cpu)."""
    import innfer_amd.lib as L
    _, N, nH, d, Hp, Wp = qkv.shape
    G = N * Hp * Wp * 32
    pad = torch.zeros(3, N, nH, 32, Hp, Wp, dtype=torch.float16)
    pad[:, :, :, :d] = qkv
    slab = pad.permute(0, 2, 1, 4, 5, 3).contiguous()                                  # [3, nH, N, Hp, Wp, 32]: group which * nH + h
    xin = slab.to(dev)
    buf = torch.full(((nH + 1) * G + 2 * GUARD,), FILL, dtype=torch.float16, device=dev)
    tb = np.ascontiguousarray(table.numpy(), np.float32)
    L.check(L.lib.innfer_window_attention16(xin.data_ptr(), G, buf.data_ptr() + 2 * GUARD, G, tb.ctypes.data, N, Hp, Wp, nH, d, shift, kw, None))
    torch.cuda.synchronize()
    raw = buf.cpu()
    assert bool((raw[:GUARD] == FILL).all()) and bool((raw[GUARD + nH * G:] == FILL).all()), "window attention 16 wrote outside its output"
    assert torch.equal(xin.cpu(), slab), "window attention 16 wrote to its input"
    return raw[GUARD:GUARD + nH * G].reshape(nH, N, Hp, Wp, 32).permute(1, 0, 4, 2, 3)


def _attn_check(dev, N, Hp, Wp, nH, d, shift, kw, seed, gain=1.0, smin=0.0):
    qkv, table = _attn_data(N, Hp, Wp, nH, d, kw, seed, gain)
    ref, smax = _attn_ref(qkv, table, shift, kw, torch.float64)
    assert smax >= smin, (smax, smin)
    e_model = float((_attn_ref(qkv, table, shift, kw, torch.float32, model=True)[0].double() - ref).abs().max())
    got = _attn_launch(dev, qkv, table, shift, kw)
    assert bool((got[:, :, d:] == 0).all()), "pad channels of the attention's result are not zero"
    what = f"window attention 16 / {kw} {N}x{Hp}x{Wp} nH {nH} d {d} shift {shift}" + (f" (|S| up to {smax:.0f})" if smin else "")
    R.assert_within_fp16_rounding(got[:, :, :d], ref, e_model, what=what, family=f"window attention 16, keys {kw}, shift {shift}")
    return qkv, table, got


@pytest.mark.parametrize("kw", [16, 24])
@pytest.mark.parametrize("nH,d", [(6, 30), (6, 24), (2, 32), (8, 10)])
def test_window_attention16(dev, nH, d, kw):
    for i, (Hp, Wp) in enumerate([(16, 16), (32, 48)] + ([(48, 48)] if d == 24 else [])):
        for shift in ((0, 8) if kw == 16 else (0,)):
            _attn_check(dev, 1, Hp, Wp, nH, d, shift, kw, 100 * nH + 10 * i + shift + kw)


@pytest.mark.parametrize("kw", [16, 24])
def test_window_attention16_batch_and_large_scores(dev, kw):
    """A window of sample n reads only sample n: each sample of a batch of two equals its own launch bit for bit; scores of some +-250 stay finite and inside the bound."""
    for shift in ((0, 8) if kw == 16 else (0,)):
        qkv, table, got = _attn_check(dev, 2, 16, 32, 6, 30, shift, kw, 900 + shift + kw)
        for n in range(2):
            one = _attn_launch(dev, qkv[:, n:n + 1].contiguous(), table, shift, kw)
            assert torch.equal(one.view(torch.int16), got[n:n + 1].contiguous().view(torch.int16)), (kw, shift, n)
        _attn_check(dev, 1, 16, 32, 2, 32, shift, kw, 950 + shift + kw, gain=24.0, smin=200.0)


def test_window_attention16_refusals(dev):
    """Refused with nothing launched: the output keeps its fill."""
    import innfer_amd.lib as L
    G = 32 * 32 * 32
    qkv = torch.zeros(24 * G, dtype=torch.float16, device=dev)
    out = torch.full((8 * G,), FILL, dtype=torch.float16, device=dev)
    tb = np.zeros((8, 256, 576), np.float32)
    call = lambda Hp, Wp, nH, d, shift, kw, gs=G, q=qkv.data_ptr(): L.lib.innfer_window_attention16(q, gs, out.data_ptr(), G, tb.ctypes.data, 1, Hp, Wp, nH, d, shift, kw, None)
    assert call(32, 24, 2, 32, 0, 16) == L.ERR_INVALID and call(24, 32, 2, 32, 0, 24) == L.ERR_INVALID
    assert call(32, 32, 9, 8, 0, 16) == L.ERR_UNSUPPORTED and call(32, 32, 2, 33, 0, 16) == L.ERR_UNSUPPORTED
    assert call(32, 32, 2, 32, 4, 16) == L.ERR_UNSUPPORTED and call(32, 32, 2, 32, 8, 24) == L.ERR_UNSUPPORTED
    assert call(32, 32, 2, 32, 0, 8) == L.ERR_UNSUPPORTED and call(32, 32, 2, 32, 0, 32) == L.ERR_UNSUPPORTED
    assert call(32, 32, 2, 32, 0, 16, gs=G - 32) == L.ERR_INVALID and call(32, 32, 2, 32, 0, 16, q=None) == L.ERR_INVALID
    torch.cuda.synchronize()
    assert bool((out == FILL).all())
    assert call(32, 32, 2, 32, 8, 16) == 0


# ------------------------------------------------------------------------------------------------ 2. the channel attention
def _ca_data(N, Cc, cp, H, W, hid, seed):
    from innfer_amd import synth
    z = synth.uniform((N, cp, H, W), 8000 + seed, -1, 1) + synth.uniform((N, cp, 1, 1), 8001 + seed, -0.5, 0.5)          # channel means that differ, per sample
    t = synth.uniform((N, cp, H, W), 8002 + seed, -2, 2)
    z[:, Cc:] = 7.0                                                                                                      # junk in the pad channels of z
    t[:, Cc:] = 0.0
    w1 = synth.uniform((hid, Cc), 8003 + seed, -1, 1) * np.float32(6.0 / np.sqrt(Cc))
    w2 = synth.uniform((Cc, hid), 8004 + seed, -1, 1) * np.float32(6.0 / np.sqrt(hid))
    b1, b2 = synth.uniform((hid,), 8005 + seed, -0.1, 0.3), synth.uniform((Cc,), 8006 + seed, -0.5, 0.5)
    f = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32))
    return f(z).half(), f(t).half(), f(w1), f(b1), f(w2), f(b2)


def _ca_excite(dev, z, Cc, hid, w1, b1, w2, b2):
    """innfer_chan_attn_excite -> (sums [N, cp], y [N, cp]) float32 (cpu); the work buffer and both results sit between guards."""
    import innfer_amd.lib as L
    N, cp, H, W = z.shape
    G = N * H * W * 32
    zin = R.to_slab(z).to(dev)
    nb = L.lib.innfer_chan_attn_work_bytes(N, H * W, cp)
    assert nb == 4 * N * cp * -(-H * W // 1024)
    work = torch.full((nb // 4 + 2 * 64,), FILL, dtype=torch.float32, device=dev)
    res = torch.full((2 * N * cp + 3 * 64,), FILL, dtype=torch.float32, device=dev)
    a = [np.ascontiguousarray(v.numpy(), np.float32) for v in (w1, b1, w2, b2)]
    L.check(L.lib.innfer_chan_attn_excite(zin.data_ptr(), G, N, H * W, Cc, cp, hid, a[0].ctypes.data, a[1].ctypes.data, a[2].ctypes.data, a[3].ctypes.data,
                                          res.data_ptr() + 4 * 64, res.data_ptr() + 4 * (128 + N * cp), work.data_ptr() + 4 * 64, nb, None))
    torch.cuda.synchronize()
    r, wk = res.cpu(), work.cpu()
    assert bool((r[:64] == FILL).all()) and bool((r[64 + N * cp:128 + N * cp] == FILL).all()) and bool((r[128 + 2 * N * cp:] == FILL).all()), "excite wrote outside its results"
    assert bool((wk[:64] == FILL).all()) and bool((wk[64 + nb // 4:] == FILL).all()), "the pool wrote outside its work buffer"
    assert torch.equal(zin.cpu(), R.to_slab(z)), "the pool wrote to its input"
    return r[128 + N * cp:128 + 2 * N * cp].reshape(N, cp), r[64:64 + N * cp].reshape(N, cp)


def _ca_scale_add(dev, t, z, y, scale):
    import innfer_amd.lib as L
    N, cp, H, W = t.shape
    G, ng = N * H * W * 32, cp // 32
    zin, yd = R.to_slab(z).to(dev), y.contiguous().to(dev)
    buf = torch.full(((ng + 1) * G + 2 * GUARD,), FILL, dtype=torch.float16, device=dev)
    buf[GUARD:GUARD + ng * G] = R.to_slab(t).reshape(-1).to(dev)
    L.check(L.lib.innfer_chan_attn_scale_add(buf.data_ptr() + 2 * GUARD, G, zin.data_ptr(), G, yd.data_ptr(), scale, N, H * W, cp, None))
    torch.cuda.synchronize()
    raw = buf.cpu()
    assert bool((raw[:GUARD] == FILL).all()) and bool((raw[GUARD + ng * G:] == FILL).all()), "the scale-add wrote outside its tensor"
    assert torch.equal(zin.cpu(), R.to_slab(z)) and torch.equal(yd.cpu(), y), "the scale-add wrote to its inputs"
    return R.from_slab(raw[GUARD:GUARD + ng * G].reshape(ng, N, H, W, 32))


@pytest.mark.parametrize("Cc,hid", [(60, 2), (180, 6), (144, 6), (256, 64)])
def test_channel_attention(dev, Cc, hid):
    cp = -(-Cc // 64) * 64
    u = 2.0 ** -24
    for i, (N, H, W) in enumerate([(1, 5, 7), (1, 40, 50), (2, 33, 47)]):
        z, t, w1, b1, w2, b2 = _ca_data(N, Cc, cp, H, W, hid, 10 * Cc + i)
        sums, y = _ca_excite(dev, z, Cc, hid, w1, b1, w2, b2)
        z64 = z.double()
        s64 = z64.sum((2, 3))
        n_chain = 16 + 4 + 3 + -(-H * W // 1024)
        bound = (n_chain + 1) * u * z64.abs().sum((2, 3))
        assert bool(((sums.double() - s64).abs() <= bound).all()), (Cc, N, H, W, float(((sums.double() - s64).abs() / bound).max()))

        def excite(dt):
            mean = (z.to(dt).sum((2, 3)) / (H * W))[:, :Cc]
            return torch.sigmoid(F.relu(mean @ w1.to(dt).T + b1.to(dt)) @ w2.to(dt).T + b2.to(dt))
        y64 = excite(torch.float64)
        e_model = float((excite(torch.float32).double() - y64).abs().max())
        err = float((y[:, :Cc].double() - y64).abs().max())
        print(f"[hat] channel attention C {Cc} hid {hid} {N}x{H}x{W}: y in [{float(y64.min()):.3f}, {float(y64.max()):.3f}], |err| {err:.2e}, e_model {e_model:.2e}")
        assert bool((y[:, Cc:] == 0).all()) and float(y64.max() - y64.min()) > 0.3          # (the test data spreads y)
        assert err <= 8 * e_model + 2.0 ** -22, (Cc, N, H, W, err, e_model)
        sums2, y2 = _ca_excite(dev, z, Cc, hid, w1, b1, w2, b2)
        assert torch.equal(sums2.view(torch.int32), sums.view(torch.int32)) and torch.equal(y2.view(torch.int32), y.view(torch.int32)), "not bit-identical on a repeat"
        for scale in (1.0, 0.01):
            got = _ca_scale_add(dev, t, z, y, scale)
            yy = y.double()[:, :, None, None]
            ref = t.double() + scale * yy * z64
            e32 = float(((t.float() + (np.float32(scale) * y[:, :, None, None]) * z.float()).double() - ref).abs().max())
            assert torch.equal(got[:, Cc:], t[:, Cc:]), "pad channels moved"
            R.assert_within_fp16_rounding(got[:, :Cc], ref[:, :Cc], e32, what=f"scale-add C {Cc} {N}x{H}x{W} scale {scale}", family="channel attention scale-add")
        if N > 1:          # nothing crosses samples
            whole = _ca_scale_add(dev, t, z, y, 1.0)
            for n in range(N):
                s1, y1 = _ca_excite(dev, z[n:n + 1].contiguous(), Cc, hid, w1, b1, w2, b2)
                assert torch.equal(s1.view(torch.int32), sums[n:n + 1].contiguous().view(torch.int32)) and torch.equal(y1.view(torch.int32), y[n:n + 1].contiguous().view(torch.int32))
                g1 = _ca_scale_add(dev, t[n:n + 1].contiguous(), z[n:n + 1].contiguous(), y1, 1.0)
                assert torch.equal(g1.view(torch.int16), whole[n:n + 1].contiguous().view(torch.int16))


def test_channel_attention_refusals(dev):
    import innfer_amd.lib as L
    G = 64 * 32
    buf = torch.zeros(8 * G, dtype=torch.float16, device=dev)
    f = torch.zeros(4096, dtype=torch.float32, device=dev)
    w = np.zeros(256 * 64, np.float32)
    ex = lambda Cc, cp, hid, nb=4096 * 4: L.lib.innfer_chan_attn_excite(buf.data_ptr(), G, 1, 64, Cc, cp, hid, w.ctypes.data, w.ctypes.data, w.ctypes.data, w.ctypes.data,
                                                                       f.data_ptr(), None, f.data_ptr() + 4 * 1024, nb, None)
    assert ex(60, 32, 2) == L.ERR_UNSUPPORTED and ex(60, 320, 2) == L.ERR_UNSUPPORTED and ex(70, 64, 2) == L.ERR_UNSUPPORTED and ex(60, 64, 65) == L.ERR_UNSUPPORTED
    assert ex(60, 64, 2, nb=16) == L.ERR_WORKSPACE and ex(60, 64, 2) == 0
    sa = lambda cp, gs=G: L.lib.innfer_chan_attn_scale_add(buf.data_ptr(), gs, buf.data_ptr(), G, f.data_ptr(), 1.0, 1, 64, cp, None)
    assert sa(96) == L.ERR_UNSUPPORTED and sa(64, gs=G - 32) == L.ERR_INVALID and sa(64) == 0


# ------------------------------------------------------------------------------------------------ 3. the GELU epilogue of the 3x3 conv
def _launch(dev, c, expect=0, form="3x3", res=False, off=0, **fields):
    """One launch through innfer_conv3x3_f16 with act 13 into [guard | off / 32 groups | the conv's groups | a foreign group | guard]: everything beside the result must
    keep its fill, like everything a refused launch (expect != 0) was given.  Returns [N, K, H, W] fp16 (cpu)."""
    import innfer_amd.lib as L
    lib = L.lib
    x, w, b = R.data(c)
    N, Cc, H, W = x.shape
    xin = R.to_slab(x, Cc // 32 + 1).to(dev)
    wc = np.ascontiguousarray(w.numpy(), dtype=np.float32)
    if form == "1x1":
        packed = np.zeros(lib.innfer_conv1x1_packed_bytes(c.K, Cc), dtype=np.uint8)
        L.check(lib.innfer_pack_conv1x1(wc.ctypes.data, c.K, Cc, packed.ctypes.data))
    else:
        packed = np.zeros(lib.innfer_conv3x3_packed_bytes(c.K, Cc), dtype=np.uint8)
        L.check(lib.innfer_pack_conv3x3_rows(wc.ctypes.data, c.K, Cc, fields.get("plane_rows", 0), packed.ctypes.data))
    d_packed = torch.from_numpy(packed).to(dev)
    bb = torch.zeros(64); bb[:c.K] = b
    d_bias = bb.to(dev)
    groups = off // 32 + (c.K + 31) // 32 + 1
    G = N * H * W * 32
    buf = torch.full((2 * groups * G + 2 * GUARD,), FILL, dtype=torch.float16, device=dev)
    keep = []
    a = L.ConvArgs()
    a.d_in, a.in_group_stride, a.C = xin.data_ptr(), G, Cc
    a.d_packed, a.d_bias = d_packed.data_ptr(), d_bias.data_ptr()
    a.d_out, a.out_group_stride, a.K, a.out_ch_off = buf.data_ptr() + GUARD * 2, G, c.K, off
    a.N, a.H, a.W, a.act = N, H, W, 13
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
    assert torch.equal(xin.cpu(), R.to_slab(x, Cc // 32 + 1)), f"{c}: wrote to its input"
    got = R.from_slab(raw[GUARD:GUARD + groups * G].reshape(groups, N, H, W, 32))
    assert bool((got[:, :off] == FILL).all()) and bool((got[:, off + c.K:] == FILL).all()), f"{c}: channels beside the conv's were written"
    return got[:, off:off + c.K]


def _gelu64(y):
    return y * 0.5 * (1.0 + torch.erf(y / np.sqrt(2.0)))


@pytest.mark.parametrize("Cin", [64, 192])
def test_gelu_epilogue_3x3(dev, Cin):
    """conv3x3_pc<2, 4, 4, OUT_SLAB, .., TAPS_3X3 | PC_GELU>: ragged edges, a batch, a whole-group channel offset."""
    for i, (N, H, W) in enumerate(S16):
        c = Case("3x3", N, Cin, 64, H, W, seed=500 + Cin + i, blo=-3.0)
        y64, e32 = R.pre(c)
        got = _launch(dev, c, off=64 if i == 2 else 0)
        R.assert_within_fp16_rounding(got, _gelu64(y64), e32, extra=y64.abs() * GELU_T, what=f"{c} act 13", family=f"act 13, {Cin} -> 64")


def test_gelu_epilogue_3x3_refusals(dev):
    """act 13 on a form that does not build it is UNSUPPORTED; nothing is launched: d_out keeps its fill."""
    import innfer_amd.lib as L
    c = Case("3x3", 1, 64, 64, 16, 32, seed=595)
    c1 = Case("1x1", 1, 64, 64, 16, 32, seed=595)
    G = 16 * 32 * 32
    U = L.ERR_UNSUPPORTED
    _launch(dev, c1, form="1x1", expect=U)
    _launch(dev, c, plane_rows=1, expect=U)
    _launch(dev, c, out_planar=1, expect=U)
    _launch(dev, c, split=1, in_lo=3 * G, out_lo=3 * G, expect=U)
    _launch(dev, c, d_stats_part=1, expect=U)
    _launch(dev, c, upsample2x=1, expect=U)
    _launch(dev, c, reflect_pad=1, expect=U)
    _launch(dev, c, res=True, expect=U)
    _launch(dev, Case("3x3", 1, 64, 32, 16, 32, seed=596), expect=U)          # the 32-output kernel has no GELU form
    _launch(dev, Case("3x3", 1, 64, 16, 16, 32, seed=597), expect=U)


# ------------------------------------------------------------------------------------------------ 4. networks
def _net(dev, name):
    from innfer_amd.architectures import get_network
    from innfer_amd.run import infer_from_state_dict
    cs = HR.FIXTURES[name][7]
    info = infer_from_state_dict({"params_ema": HR.fixture_sd(name)})
    net = get_network(dict(info["net_params"], conv_scale=cs))
    net.load_state_dict(info["state_dict"], strict=True)
    return net.to(dev).eval()


def _assert_like_storage_model(got, y64, ys, what):
    """max |engine - float64| <= 2 x max |storage model - float64| of the same case (computed here), and >= 99 % of the uint8 codes within +-1."""
    err, es = float((got.double() - y64).abs().max()), float((ys - y64).abs().max())
    share = HR.codes_within_one(got, y64)
    print(f"[hat] {what}: engine max|err| {err:.2e}, storage model {es:.2e}, ratio {err / es:.3f}; codes within +-1: {share:.5f}")
    assert got.shape == y64.shape and torch.isfinite(got).all()
    assert err <= 2 * es, (what, err, es)
    assert share >= 0.99, (what, share)


def launch_formula(Cc, nH, hidden, depths, s, padded):
    """S1 + 2 + B (7 + SQ + 3 S1 + SH) + R (3 + SQ + 2 S1 + SH) + (R + 1) S1 + T + 2 [padded]."""
    S1, SQ, SH = -(-Cc // 64), -(-3 * nH // 2), -(-hidden // 64)
    T = 4 if s == 3 else 2 + {2: 1, 4: 2}[s]
    return S1 + 2 + sum(depths) * (7 + SQ + 3 * S1 + SH) + len(depths) * (3 + SQ + 2 * S1 + SH) + (len(depths) + 1) * S1 + T + (2 if padded else 0)


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


@pytest.mark.parametrize("name", list(HR.FIXTURES))
def test_network_vs_float64(dev, name):
    from innfer_amd import synth
    from innfer_amd.utils import utils as U
    Cc, nH, depths, shape, s, cr, sq, cs, stored, seed = HR.FIXTURES[name]
    sd, x, y64, ys = HR.case(name)
    net = _net(dev, name)
    assert (net.nf, net.num_heads, tuple(net.depths), net.upscale, net.compress_ch, net.squeeze_ch, net.conv_scale) == (Cc, nH, tuple(depths), s, Cc // cr, Cc // sq, cs)
    xd = x.to(dev).half()
    y = net(xd)
    assert y.dtype == torch.float16 and net._out_shape(shape[0], shape[2], shape[3], dev) == tuple(y64.shape) == tuple(y.shape)
    _assert_like_storage_model(y.float().cpu(), y64, ys, name)
    n, yt = _launches(net, xd)
    assert n == launch_formula(Cc, nH, 2 * Cc, depths, s, shape[2] % 16 != 0 or shape[3] % 16 != 0) and torch.equal(yt, y), n
    buf = torch.empty(y.shape, dtype=torch.float16, device=dev)
    assert net(xd, out=buf) is buf and torch.equal(buf, y)
    if shape[0] > 1:          # nothing in HAT crosses samples: the channel attention pools per sample
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
    net = _net(dev, "C60 [2] x2 16x16 cs1")
    with pytest.raises(NotImplementedError, match="reflection"):
        net(torch.zeros(1, 3, 8, 16, dtype=torch.float16, device=dev))
    assert tuple(net(torch.zeros(1, 3, 9, 16, dtype=torch.float16, device=dev)).shape) == (1, 3, 18, 32)


# ------------------------------------------------------------------------------------------------ 5. the Model
@pytest.fixture(scope="module")
def model(tmp_path_factory):
    from innfer_amd.run import Model
    sd = HR.fill(3, 60, (2,), 6, 2.0, 2, 3, 30, seed=8)
    path = str(tmp_path_factory.mktemp("hat") / "2x_hat.pth")
    torch.save({"params_ema": dict(sd, **HR.buffers())}, path)
    m = Model(path, arch="infer", scale=None, device="cuda", chop=True, tile_batch=4)
    assert (m.arch, m.scale, m.in_nc, m.out_nc) == ("hat", 2, 3, 3)
    return m


def test_model_chop(dev, model):
    """250 x 330 through the chop path (200-px tiles: the channel attention pools per tile) against the network run tile by tile and the oracle's blend of those fp16
    tiles, rounded to fp16 as the chop path's is: the two differ in the blend's arithmetic alone -- one fp16 rounding of a value below 2.  run_u8 == the separate
    conversions; a float32 tensor is refused."""
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
