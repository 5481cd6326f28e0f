"""DAT on the GPU (needs an MI355X: `pytest -m gpu`): the kernels of its block one launch at a time, whole networks, the Model.  The launches run against float64 on the stored fp16 operands (tests/_dat_ref.py).  Every
launch writes between guard bands that must keep their fill; inputs must be unchanged.  Bounds follow tests/test_gpu_hat.py / test_gpu_swinir.py: ulp16 / 2 + 8 e_model
through _conv_ref.assert_within_fp16_rounding, e_model the error of a float32 CPU model of the kernel's DECLARED arithmetic, computed here and never taken from the kernel.

1. innfer_window_attention_rect: splits [8, 32] and [8, 16], shifted and not; grids 5 x 7 (every window mostly pad), 32 x 32 (no pad; the shift wraps a window onto
   itself), 40 x 72 (padded to 64 x 96 / 48 x 80: interior windows, border windows, pad tokens as keys); (nH, d) = (6, 30), (2, 32), (4, 10); a batch of 2 whose samples
   differ, each bit-equal to its own N = 1 launch; one case with |scores| beyond 200.  Pad channels of the result are exactly zero.  The 40 x 72 shifted case is asserted
   to have mask entries of -100 and pad keys in both branches.  e_model: float32 scores, the keys walked in blocks of 64 with a running maximum and sum, P rounded to fp16
   in front of P v, float32 accumulation and division.
2. innfer_channel_attention_scores / _apply: grids 5 x 7, 40 x 50 (two segments), a batch of two 33 x 47 (a ragged second segment); (nH, d) = (6, 30), (2, 32); a negative
   temperature, an all-zero q column (its row of A is uniform), junk in the slab's pad channels.  G, sq, sk: |err| <= (n + 1) u sum |products|, u = 2^-24, n = min(HW, 1024)
   + segments the longest chain of float32 additions (a segment's pixels, then the merge).  A: 8 e_model + 2^-22, e_model that of a float32 numpy model with the kernel's
   chain order; the apply, from the float64 A: one fp16 rounding + 8 e_model.  Bit-identical on a repeat and per sample of a batch.
3. innfer_dwconv3x3, epilogues none / GELU / times a second slab: 1 x 1, 3 x 70, 33 x 47 and a batch; C 60 / 64, 180 / 192, 360 / 384 with junk in the pad channels.  The
   GELU form carries act 12's extra |f| GELU_T, GELU_T = 2^-20 (tests/test_gpu_swinir.py derives it for common.h fast_gelu).
4. innfer_chan_attn_excite_gelu (y against 8 e_model + 2^-22, as for HAT's excite) and innfer_aim_mix with both (X, Y) assignments, given the gate the GPU computed:
   one fp16 rounding + 8 e_model; in place on X and on Y equals out of place.
5. innfer_layer_norm_wide at C 360 / c_pad 384 and C 500 / c_pad 512 with test_gpu_swinir.py's LayerNorm bound (n = c_pad / 4 + 2).
6. Refusals: the status is returned and nothing is written.
7. Networks (innfer_dat_create through the DAT shell) against the float64 forward of tests/_dat_ref.py: max |err| <= 2 x the fp16 storage model's own error on the same
   case and >= 99 % of the uint8 codes within +-1 (tests/test_dat_host.py checks the storage model alone on the CPU); the launch count equals the formula of the header /
   DESIGN.md 3.4o; out= is honoured; a batch's sample equals its own forward bit for bit; forward_u8 == the separate conversions; a float32 tensor is refused.  Fixtures:
   C 60 / nH 6 / [8, 16] / depth [3, 2] / 3conv / pixelshuffledirect x2 at 20 x 44 (a pad, shifted blocks in both groups, both block forms); C 180 / [8, 32] / depth [2] / x4
   pixelshuffle at 40 x 72; C 64 / nH 2 (d 32) / [8, 16] / depth [4] / expansion 4 / x3 as a batch of two 19 x 26.
   Measured on the MI355X, engine max |err| / storage model max |err|: 
       C60 [3, 2] 3conv direct x2 20x44 1.331 | C180 [2] x4 40x72 1.290 | C64 nH2 [4] x3 batch of two 19x26 1.059 (100 % of the codes within +-1 in every case)
8. Model(arch='infer', chop=True) from a .pth under params_ema with every buffer (rpe_biases, relative_position_index, attn_mask_0 / _1) on a 250 x 330 image against the
   network run tile by tile and blended by the oracle's helper (<= 2^-10); run_u8_batch equals per-image runs, a 5 x 7 image included.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _conv_ref as R
import _dat_ref as DR

pytestmark = pytest.mark.gpu

FILL, GUARD = -3.0, 4096
GELU_T = 2.0 ** -20
U32 = 2.0 ** -24


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _f32(a):
    return np.ascontiguousarray(a.numpy() if torch.is_tensor(a) else a, np.float32)


def _qkv_slab(qkv):
    """[3, N, nH, d, H, W] fp16 -> the head-padded slab [3 nH, N, H, W, 32] (group which * nH + h), pad channels zero."""
    _, N, nH, d, H, W = qkv.shape
    pad = torch.zeros(3, N, nH, 32, H, W, dtype=torch.float16)
    pad[:, :, :, :d] = qkv
    return pad.permute(0, 2, 1, 4, 5, 3).reshape(3 * nH, N, H, W, 32).contiguous()


# ------------------------------------------------------------------------------------------------ 1. the rectangular window attention
def _attn_data(N, H, W, nH, d, T, seed, gain=1.0):
    from innfer_amd import synth
    qkv = synth.uniform((3, N, nH, d, H, W), 16000 + seed, -1, 1)
    for n in range(N):
        qkv[:, n] *= np.float32(1.0 + 0.5 * n)
    qkv[0] *= np.float32(gain)
    table = synth.uniform((nH, T, T), 16001 + seed, -2, 2)
    return torch.from_numpy(qkv).half(), torch.from_numpy(np.ascontiguousarray(table))


def _attn_launch(dev, qkv, table, s0, s1, shifted):
    """innfer_window_attention_rect into [guard | nH groups | a foreign group | guard].  Returns [N, nH, 32, H, W] fp16 (cpu)."""
    import innfer_amd.lib as L
    _, N, nH, d, H, W = qkv.shape
    G = N * H * W * 32
    slab = _qkv_slab(qkv)
    xin = slab.to(dev)
    buf = torch.full(((nH + 1) * G + 2 * GUARD,), FILL, dtype=torch.float16, device=dev)
    tb = _f32(table)
    L.check(L.lib.innfer_window_attention_rect(xin.data_ptr(), G, buf.data_ptr() + 2 * GUARD, G, tb.ctypes.data, N, H, W, nH, d, s0, s1, shifted, None))
    torch.cuda.synchronize()
    raw = buf.cpu()
    assert bool((raw[:GUARD] == FILL).all()) and bool((raw[GUARD + nH * G:] == FILL).all()), "rect attention wrote outside its output"
    assert torch.equal(xin.cpu(), slab), "rect attention wrote to its input"
    return raw[GUARD:GUARD + nH * G].reshape(nH, N, H, W, 32).permute(1, 0, 4, 2, 3)


def _attn_check(dev, N, H, W, nH, d, s1, shifted, seed, gain=1.0, smin=0.0):
    qkv, table = _attn_data(N, H, W, nH, d, 8 * s1, seed, gain)
    ref, smax = DR.rect_attention(qkv, table, 8, s1, shifted, torch.float64)
    assert smax >= smin, (smax, smin)
    e_model = float((DR.rect_attention(qkv, table, 8, s1, shifted, torch.float32, model=True)[0].double() - ref).abs().max())
    got = _attn_launch(dev, qkv, table, 8, s1, shifted)
    assert bool((got[:, :, d:] == 0).all()), "pad channels of the attention's result are not zero"
    what = f"rect attention [8, {s1}] {N}x{H}x{W} nH {nH} d {d} shifted {shifted}" + (f" (|S| up to {smax:.0f})" if smin else "")
    R.assert_within_fp16_rounding(got[:, :, :d], ref, e_model, what=what, family=f"rect attention [8, {s1}], shifted {shifted}")
    return qkv, table, got


def test_rect_attention_case_has_mask_and_pad_keys():
    """The 40 x 72 shifted case exercises what it is meant to: -100 entries and pad tokens as keys in both branches, for both splits; windows without a mask as well."""
    for s1 in (32, 16):
        Hp, Wp = DR.padded(40, 72, 8, s1)
        assert (Hp, Wp) == ((64, 96) if s1 == 32 else (48, 80))
        for br in (0, 1):
            wh, ww, shy, shx = DR.branch_geometry(br, 8, s1, 1)
            M = DR.shift_mask(Hp, Wp, wh, ww, shy, shx)
            pk = DR.pad_keys(40, 72, 8, s1, br, 1)
            assert float(M.min()) == -100.0 and bool((M.amin((1, 2)) == 0).any()), (s1, br)
            assert bool(pk.any()) and bool((pk.any(1) & (~pk).any(1)).any()), (s1, br)          # (windows that mix real and pad tokens)


@pytest.mark.parametrize("s1", [32, 16])
@pytest.mark.parametrize("nH,d", [(6, 30), (2, 32), (4, 10)])
def test_rect_attention(dev, nH, d, s1):
    for i, (H, W) in enumerate([(5, 7), (32, 32), (40, 72)]):
        for shifted in (0, 1):
            _attn_check(dev, 1, H, W, nH, d, s1, shifted, 100 * nH + 10 * i + shifted + s1)


@pytest.mark.parametrize("s1", [32, 16])
def test_rect_attention_batch_and_large_scores(dev, s1):
    """A window of sample n reads only sample n: each sample of a batch of two equals its own launch bit for bit; scores beyond +-200 stay finite and inside the bound."""
    for shifted in (0, 1):
        qkv, table, got = _attn_check(dev, 2, 19, 40, 6, 30, s1, shifted, 900 + shifted + s1)
        for n in range(2):
            one = _attn_launch(dev, qkv[:, n:n + 1].contiguous(), table, 8, s1, shifted)
            assert torch.equal(one.view(torch.int16), got[n:n + 1].contiguous().view(torch.int16)), (s1, shifted, n)
        _attn_check(dev, 1, 19, 40, 2, 32, s1, shifted, 950 + shifted + s1, gain=24.0, smin=200.0)


def test_rect_attention_refusals(dev):
    """Refused with nothing launched: the output keeps its fill."""
    import innfer_amd.lib as L
    G = 32 * 32 * 32
    qkv = torch.zeros(24 * G, dtype=torch.float16, device=dev)
    out = torch.full((8 * G,), FILL, dtype=torch.float16, device=dev)
    tb = np.zeros((8, 256, 256), np.float32)
    call = lambda nH, d, s0, s1, sh=0, gs=G, q=qkv.data_ptr(), H=32: L.lib.innfer_window_attention_rect(q, gs, out.data_ptr(), G, tb.ctypes.data, 1, H, 32, nH, d, s0, s1, sh, None)
    assert call(2, 32, 8, 8) == L.ERR_UNSUPPORTED and call(2, 32, 16, 16) == L.ERR_UNSUPPORTED and call(2, 32, 32, 8) == L.ERR_UNSUPPORTED and call(2, 32, 8, 64) == L.ERR_UNSUPPORTED
    assert call(3, 32, 8, 32) == L.ERR_UNSUPPORTED and call(10, 8, 8, 32) == L.ERR_UNSUPPORTED and call(2, 33, 8, 32) == L.ERR_UNSUPPORTED and call(2, 0, 8, 16) == L.ERR_UNSUPPORTED
    assert call(2, 32, 8, 32, sh=2) == L.ERR_INVALID and call(2, 32, 8, 32, gs=G - 32) == L.ERR_INVALID and call(2, 32, 8, 32, q=None) == L.ERR_INVALID
    assert call(2, 32, 8, 32, H=0) == L.ERR_INVALID
    torch.cuda.synchronize()
    assert bool((out == FILL).all())
    assert call(2, 32, 8, 32, sh=1) == 0


# ------------------------------------------------------------------------------------------------ 2. the attention across channels
def _csa_data(N, H, W, nH, d, seed):
    from innfer_amd import synth
    qkv = synth.uniform((3, N, nH, d, H, W), 17000 + seed, -1, 1) + synth.uniform((3, N, nH, d, 1, 1), 17001 + seed, -0.3, 0.3)
    for n in range(N):
        qkv[:, n] *= np.float32(1.0 + 0.5 * n)
    qkv[0, :, 0, 3] = 0.0                                                                  # an all-zero column of q: its row of A is uniform
    temp = synth.uniform((nH,), 17002 + seed, 0.5, 3.0)
    temp[-1] = -temp[-1]                                                                   # a negative temperature
    return torch.from_numpy(qkv).half(), torch.from_numpy(temp)


def _csa_slab(qkv):
    d = qkv.shape[3]
    slab = _qkv_slab(qkv)
    slab[..., d:] = 7.0                                                                    # junk in the pad channels of q, k and v
    return slab


def _csa_scores(dev, qkv, temp):
    """-> (A [N, nH, 32, 32], gram [N, nH, 1088]) float32 (cpu); the work buffer and both results sit between guards."""
    import innfer_amd.lib as L
    _, N, nH, d, H, W = qkv.shape
    G = N * H * W * 32
    slab = _csa_slab(qkv)
    xin = slab.to(dev)
    nb = L.lib.innfer_channel_attention_work_bytes(N, H * W, nH)
    assert nb == 4 * N * nH * 1088 * -(-H * W // 1024)
    nA, nG = N * nH * 1024, N * nH * 1088
    work = torch.full((nb // 4 + 128,), FILL, dtype=torch.float32, device=dev)
    res = torch.full((nA + nG + 192,), FILL, dtype=torch.float32, device=dev)
    t = _f32(temp)
    L.check(L.lib.innfer_channel_attention_scores(xin.data_ptr(), G, N, H * W, nH, d, t.ctypes.data, res.data_ptr() + 4 * 64, res.data_ptr() + 4 * (128 + nA),
                                                  work.data_ptr() + 4 * 64, nb, None))
    torch.cuda.synchronize()
    r, wk = res.cpu(), work.cpu()
    assert bool((r[:64] == FILL).all()) and bool((r[64 + nA:128 + nA] == FILL).all()) and bool((r[128 + nA + nG:] == FILL).all()), "the scores wrote outside their results"
    assert bool((wk[:64] == FILL).all()) and bool((wk[64 + nb // 4:] == FILL).all()), "the Gram pass wrote outside its work buffer"
    assert torch.equal(xin.cpu(), slab), "the scores wrote to their input"
    return r[64:64 + nA].reshape(N, nH, 32, 32).clone(), r[128 + nA:128 + nA + nG].reshape(N, nH, 1088).clone()


def _csa_apply(dev, qkv, A):
    import innfer_amd.lib as L
    _, N, nH, d, H, W = qkv.shape
    G = N * H * W * 32
    slab = _csa_slab(qkv)
    xin, Ad = slab.to(dev), A.contiguous().to(dev)
    buf = torch.full(((nH + 1) * G + 2 * GUARD,), FILL, dtype=torch.float16, device=dev)
    L.check(L.lib.innfer_channel_attention_apply(xin.data_ptr(), G, buf.data_ptr() + 2 * GUARD, G, Ad.data_ptr(), N, H * W, nH, d, None))
    torch.cuda.synchronize()
    raw = buf.cpu()
    assert bool((raw[:GUARD] == FILL).all()) and bool((raw[GUARD + nH * G:] == FILL).all()), "the apply wrote outside its output"
    assert torch.equal(xin.cpu(), slab) and torch.equal(Ad.cpu(), A), "the apply wrote to its inputs"
    return raw[GUARD:GUARD + nH * G].reshape(nH, N, H, W, 32).permute(1, 0, 4, 2, 3)


def _csa_model32(q, k, temp):
    """The kernel's declared arithmetic in float32 numpy: per segment of 1024 pixels a chain over the pixels in order, the segments merged in order, the scaling, the softmax."""
    N, nH, d = q.shape[:3]
    qf, kf = q.float().reshape(N, nH, d, -1).numpy(), k.float().reshape(N, nH, d, -1).numpy()
    HW = qf.shape[-1]
    G, sq, sk = (np.zeros(s, np.float32) for s in ((N, nH, d, d), (N, nH, d), (N, nH, d)))
    for p0 in range(0, HW, 1024):
        g, a, b = (np.zeros(s, np.float32) for s in ((N, nH, d, d), (N, nH, d), (N, nH, d)))
        for n in range(p0, min(p0 + 1024, HW)):
            g += qf[..., n, None] * kf[..., None, :, n]
            a += qf[..., n] * qf[..., n]
            b += kf[..., n] * kf[..., n]
        G, sq, sk = G + g, sq + a, sk + b
    rq, rk = np.float32(1) / np.maximum(np.sqrt(sq), np.float32(1e-12)), np.float32(1) / np.maximum(np.sqrt(sk), np.float32(1e-12))
    S = (G * (rq[..., :, None] * rk[..., None, :])) * temp.float().numpy()[None, :, None, None]
    e = np.exp(S - S.max(-1, keepdims=True))
    return torch.from_numpy(e / e.sum(-1, keepdims=True, dtype=np.float32))


@pytest.mark.parametrize("nH,d", [(6, 30), (2, 32)])
def test_channel_self_attention(dev, nH, d):
    for i, (N, H, W) in enumerate([(1, 5, 7), (1, 40, 50), (2, 33, 47)]):
        qkv, temp = _csa_data(N, H, W, nH, d, 10 * nH + i)
        A, gram = _csa_scores(dev, qkv, temp)
        q64, k64 = (qkv[j].double().reshape(N, nH, d, -1) for j in (0, 1))
        G64, sq64, sk64, A64 = DR.channel_scores(qkv[0], qkv[1], temp, torch.float64)
        n_chain = min(H * W, 1024) + -(-H * W // 1024)
        Gg = gram[:, :, :1024].reshape(N, nH, 32, 32)
        bG = (n_chain + 1) * U32 * (q64.abs() @ k64.abs().transpose(-1, -2))
        assert bool(((Gg[:, :, :d, :d].double() - G64).abs() <= bG).all()), ("G", nH, d, N, H, W)
        assert bool(((gram[:, :, 1024:1024 + d].double() - sq64).abs() <= (n_chain + 1) * U32 * sq64).all()), ("sq", nH, d, N, H, W)
        assert bool(((gram[:, :, 1056:1056 + d].double() - sk64).abs() <= (n_chain + 1) * U32 * sk64).all()), ("sk", nH, d, N, H, W)
        assert bool((Gg[:, :, d:] == 0).all()) and bool((Gg[:, :, :, d:] == 0).all()) and bool((gram[:, :, 1024 + d:1056] == 0).all()) and bool((gram[:, :, 1056 + d:] == 0).all())
        e_model = float((_csa_model32(qkv[0], qkv[1], temp).double() - A64).abs().max())
        err = float((A[:, :, :d, :d].double() - A64).abs().max())
        print(f"[dat] channel attention nH {nH} d {d} {N}x{H}x{W}: A in [{float(A64.min()):.4f}, {float(A64.max()):.4f}], |err| {err:.2e}, e_model {e_model:.2e}")
        assert err <= 8 * e_model + 2.0 ** -22, (nH, d, N, H, W, err, e_model)
        assert bool((A[:, :, d:] == 0).all()) and bool((A[:, :, :, d:] == 0).all()), "pad rows / columns of A are not zero"
        assert bool((A[:, 0, 3, :d] == np.float32(1) / np.float32(d)).all()), "the row of an all-zero q column is not uniform"
        assert float(A64[:, -1].max()) > 1.1 / d, "the temperatures do not spread A"
        A2, gram2 = _csa_scores(dev, qkv, temp)
        assert torch.equal(A2.view(torch.int32), A.view(torch.int32)) and torch.equal(gram2.view(torch.int32), gram.view(torch.int32)), "not bit-identical on a repeat"

        A64p = torch.zeros(N, nH, 32, 32, dtype=torch.float64)
        A64p[:, :, :d, :d] = A64
        got = _csa_apply(dev, qkv, A64p.float())                                           # from the float64 A rounded to float32 once
        ref = DR.channel_apply(A64p[:, :, :d, :d].float().double(), qkv[2].double())
        e32 = float((DR.channel_apply(A64p[:, :, :d, :d].float(), qkv[2].float()).double() - ref).abs().max())
        assert bool((got[:, :, d:] == 0).all()), "pad channels of the apply's result are not zero"
        R.assert_within_fp16_rounding(got[:, :, :d], ref, e32, what=f"channel attention apply nH {nH} d {d} {N}x{H}x{W}", family="channel attention apply")
        if N > 1:          # nothing crosses samples
            whole = _csa_apply(dev, qkv, A)
            for n in range(N):
                A1, g1 = _csa_scores(dev, qkv[:, n:n + 1].contiguous(), temp)
                assert torch.equal(A1.view(torch.int32), A[n:n + 1].contiguous().view(torch.int32)) and torch.equal(g1.view(torch.int32), gram[n:n + 1].contiguous().view(torch.int32))
                o1 = _csa_apply(dev, qkv[:, n:n + 1].contiguous(), A1)
                assert torch.equal(o1.view(torch.int16), whole[n:n + 1].contiguous().view(torch.int16))


def test_channel_self_attention_refusals(dev):
    import innfer_amd.lib as L
    G = 64 * 32
    buf = torch.zeros(24 * G, dtype=torch.float16, device=dev)
    f = torch.full((32768,), FILL, dtype=torch.float32, device=dev)
    t = np.ones(8, np.float32)
    sc = lambda nH, d, nb=4 * 8 * 1088, gs=G, HW=64: L.lib.innfer_channel_attention_scores(buf.data_ptr(), gs, 1, HW, nH, d, t.ctypes.data, f.data_ptr(), None,
                                                                                          f.data_ptr() + 4 * 8192, nb, None)
    assert sc(9, 8) == L.ERR_UNSUPPORTED and sc(2, 33) == L.ERR_UNSUPPORTED and sc(2, 0) == L.ERR_UNSUPPORTED
    assert sc(2, 32, nb=16) == L.ERR_WORKSPACE and sc(2, 32, gs=G - 32) == L.ERR_INVALID and sc(2, 32, HW=0) == L.ERR_INVALID
    out = torch.full((8 * G,), FILL, dtype=torch.float16, device=dev)
    ap = lambda nH, d, gs=G: L.lib.innfer_channel_attention_apply(buf.data_ptr(), gs, out.data_ptr(), G, f.data_ptr(), 1, 64, nH, d, None)
    assert ap(9, 8) == L.ERR_UNSUPPORTED and ap(2, 33) == L.ERR_UNSUPPORTED and ap(2, 32, gs=G - 32) == L.ERR_INVALID
    torch.cuda.synchronize()
    assert bool((f == FILL).all()) and bool((out == FILL).all())
    assert sc(2, 32) == 0


# ------------------------------------------------------------------------------------------------ 3. the depthwise conv
def _slab_out(dev, ng, G):
    return torch.full(((ng + 1) * G + 2 * GUARD,), FILL, dtype=torch.float16, device=dev)


def _slab_read(buf, ng, N, H, W, what):
    G = N * H * W * 32
    raw = buf.cpu()
    assert bool((raw[:GUARD] == FILL).all()) and bool((raw[GUARD + ng * G:] == FILL).all()), f"{what} wrote outside its output"
    return R.from_slab(raw[GUARD:GUARD + ng * G].reshape(ng, N, H, W, 32))


def _dw_launch(dev, x, mul, Cc, taps, bias, epi):
    import innfer_amd.lib as L
    N, cp, H, W = x.shape
    G, ng = N * H * W * 32, cp // 32
    xin = R.to_slab(x).to(dev)
    min_ = R.to_slab(mul).to(dev) if mul is not None else None
    buf = _slab_out(dev, ng, G)
    tp, bs = _f32(taps), _f32(bias)
    L.check(L.lib.innfer_dwconv3x3(xin.data_ptr(), G, min_.data_ptr() if mul is not None else None, G, buf.data_ptr() + 2 * GUARD, G, N, H, W, Cc, cp, tp.ctypes.data,
                                   bs.ctypes.data, epi, None))
    torch.cuda.synchronize()
    assert torch.equal(xin.cpu(), R.to_slab(x)) and (mul is None or torch.equal(min_.cpu(), R.to_slab(mul))), "the depthwise conv wrote to its inputs"
    return _slab_read(buf, ng, N, H, W, "the depthwise conv")


@pytest.mark.parametrize("Cc,cp", [(60, 64), (180, 192), (360, 384)])
def test_dwconv3x3(dev, Cc, cp):
    from innfer_amd import synth
    for i, (N, H, W) in enumerate([(1, 1, 1), (1, 3, 70), (1, 33, 47), (2, 33, 47)]):
        seed = 18000 + 10 * Cc + i
        x = synth.uniform((N, cp, H, W), seed, -2, 2)
        m = synth.uniform((N, cp, H, W), seed + 1, -2, 2)
        for n in range(N):
            x[n] *= np.float32(1.0 + 0.5 * n)
        x[:, Cc:], m[:, Cc:] = 7.0, 7.0                                                   # junk in the pad channels
        x, m = torch.from_numpy(x).half(), torch.from_numpy(m).half()
        taps = torch.from_numpy(synth.uniform((Cc, 3, 3), seed + 2, -1, 1))
        bias = torch.from_numpy(synth.uniform((Cc,), seed + 3, -1, 1))
        f64 = DR.dwconv(x[:, :Cc].double(), taps.double(), bias.double())
        e32 = float((DR.dwconv(x[:, :Cc].float(), taps, bias).double() - f64).abs().max())
        for epi in (0, 1, 2):
            got = _dw_launch(dev, x, m if epi == 2 else None, Cc, taps, bias, epi)
            assert bool((got[:, Cc:] == 0).all()), "pad channels of the depthwise conv's result are not zero"
            what = f"dwconv C {Cc} {N}x{H}x{W} epilogue {epi}"
            if epi == 0:
                R.assert_within_fp16_rounding(got[:, :Cc], f64, e32, what=what, family="dwconv")
            elif epi == 1:
                R.assert_within_fp16_rounding(got[:, :Cc], DR.gelu(f64), e32, extra=f64.abs() * GELU_T, what=what, family="dwconv + GELU")
            else:
                m64 = m[:, :Cc].double()
                R.assert_within_fp16_rounding(got[:, :Cc], f64 * m64, 0.0, extra=(8 * e32 + U32 * f64.abs()) * m64.abs(), what=what, family="dwconv x gate")
        if N > 1:
            one = _dw_launch(dev, x[1:2].contiguous(), None, Cc, taps, bias, 1)
            assert torch.equal(one.view(torch.int16), _dw_launch(dev, x, None, Cc, taps, bias, 1)[1:2].contiguous().view(torch.int16))


def test_dwconv3x3_refusals(dev):
    import innfer_amd.lib as L
    G = 64 * 32
    buf = torch.zeros(20 * G, dtype=torch.float16, device=dev)
    out = torch.full((20 * G,), FILL, dtype=torch.float16, device=dev)
    w = np.zeros(600 * 9, np.float32)
    call = lambda Cc, cp, epi=0, mul=None, o=out.data_ptr(), gs=G: L.lib.innfer_dwconv3x3(buf.data_ptr(), gs, mul, G, o, G, 1, 8, 8, Cc, cp, w.ctypes.data, w.ctypes.data, epi, None)
    assert call(60, 48) == L.ERR_UNSUPPORTED and call(70, 64) == L.ERR_UNSUPPORTED and call(520, 544) == L.ERR_UNSUPPORTED and call(60, 64, epi=3) == L.ERR_UNSUPPORTED
    assert call(60, 64, epi=2) == L.ERR_INVALID and call(60, 64, o=buf.data_ptr()) == L.ERR_INVALID and call(60, 64, gs=G - 32) == L.ERR_INVALID
    torch.cuda.synchronize()
    assert bool((out == FILL).all())
    assert call(60, 64, epi=2, mul=buf.data_ptr()) == 0


# ------------------------------------------------------------------------------------------------ 4. the GELU excite and the interaction mix
def _excite_gelu(dev, z, Cc, hid, w1, b1, w2, b2):
    import innfer_amd.lib as L
    N, cp, H, W = z.shape
    G = N * H * W * 32
    zin = R.to_slab(z).to(dev)
    nb = L.lib.innfer_chan_attn_work_bytes(N, H * W, cp)
    work = torch.full((nb // 4 + 128,), FILL, dtype=torch.float32, device=dev)
    res = torch.full((N * cp + 128,), FILL, dtype=torch.float32, device=dev)
    a = [_f32(v) for v in (w1, b1, w2, b2)]
    L.check(L.lib.innfer_chan_attn_excite_gelu(zin.data_ptr(), G, N, H * W, Cc, cp, hid, a[0].ctypes.data, a[1].ctypes.data, a[2].ctypes.data, a[3].ctypes.data,
                                               res.data_ptr() + 4 * 64, None, work.data_ptr() + 4 * 64, nb, None))
    torch.cuda.synchronize()
    r, wk = res.cpu(), work.cpu()
    assert bool((r[:64] == FILL).all()) and bool((r[64 + N * cp:] == FILL).all()) and bool((wk[:64] == FILL).all()) and bool((wk[64 + nb // 4:] == FILL).all())
    assert torch.equal(zin.cpu(), R.to_slab(z)), "the excite wrote to its input"
    return r[64:64 + N * cp].reshape(N, cp).clone()


def _mix(dev, x, y, gate, Cc, hid, w1, b1, w2, b2, in_place=None):
    import innfer_amd.lib as L
    N, cp, H, W = x.shape
    G, ng = N * H * W * 32, cp // 32
    xin, yin, gd = R.to_slab(x).to(dev), R.to_slab(y).to(dev), gate.contiguous().to(dev)
    a = [_f32(v) for v in (w1, b1, w2)]
    args = (gd.data_ptr(), N, H * W, Cc, cp, hid, a[0].ctypes.data, a[1].ctypes.data, a[2].ctypes.data, float(b2), None)
    if in_place is not None:
        dst = xin if in_place == "x" else yin
        L.check(L.lib.innfer_aim_mix(xin.data_ptr(), G, yin.data_ptr(), G, dst.data_ptr(), G, *args))
        torch.cuda.synchronize()
        return R.from_slab(dst.cpu())
    buf = _slab_out(dev, ng, G)
    L.check(L.lib.innfer_aim_mix(xin.data_ptr(), G, yin.data_ptr(), G, buf.data_ptr() + 2 * GUARD, G, *args))
    torch.cuda.synchronize()
    assert torch.equal(xin.cpu(), R.to_slab(x)) and torch.equal(yin.cpu(), R.to_slab(y)) and torch.equal(gd.cpu(), gate), "the mix wrote to its inputs"
    return _slab_read(buf, ng, N, H, W, "the mix")


@pytest.mark.parametrize("Cc", [60, 180, 64, 256])
def test_aim_mix(dev, Cc):
    from innfer_amd import synth
    cp, hc, hs = -(-Cc // 64) * 64, Cc // 8, Cc // 16
    f = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32))
    for i, (N, H, W) in enumerate([(1, 5, 7), (1, 40, 50), (2, 33, 47)]):
        seed = 19000 + 10 * Cc + i
        a = synth.uniform((N, cp, H, W), seed, -1, 1) + synth.uniform((N, cp, 1, 1), seed + 1, -0.5, 0.5)
        c = synth.uniform((N, cp, H, W), seed + 2, -2, 2) + synth.uniform((N, cp, 1, 1), seed + 3, -0.5, 0.5)
        a[:, Cc:], c[:, Cc:] = 7.0, 7.0                                                   # junk in the pad channels
        a, c = f(a).half(), f(c).half()
        cw1 = f(synth.uniform((hc, Cc), seed + 4, -1, 1) * np.float32(6.0 / np.sqrt(Cc)))
        cw2 = f(synth.uniform((Cc, hc), seed + 5, -1, 1) * np.float32(6.0 / np.sqrt(hc)))
        cb1, cb2 = f(synth.uniform((hc,), seed + 6, -0.3, 0.3)), f(synth.uniform((Cc,), seed + 7, -0.5, 0.5))
        sw1 = f(synth.uniform((hs, Cc), seed + 8, -1, 1) * np.float32(3.0 / np.sqrt(Cc)))
        sb1, sw2, sb2 = f(synth.uniform((hs,), seed + 9, -0.3, 0.3)), f(synth.uniform((hs,), seed + 10, -1, 1) * np.float32(6.0 / np.sqrt(hs))), 0.125
        for X, Y, name in ((a, c, "ASA"), (c, a, "ACA")):                                 # X gated per channel by the pool over Y, Y per pixel by the gate computed from X
            gate = _excite_gelu(dev, Y, Cc, hc, cw1, cb1, cw2, cb2)
            pooled = lambda dt: (Y.to(dt).sum((2, 3)) / (H * W))[:, :Cc]
            y64 = DR.excite_gelu(pooled(torch.float64), cw1, cb1, cw2, cb2)
            e_y = float((DR.excite_gelu(pooled(torch.float32), cw1, cb1, cw2, cb2).double() - y64).abs().max())
            err = float((gate[:, :Cc].double() - y64).abs().max())
            print(f"[dat] GELU excite C {Cc} hid {hc} {N}x{H}x{W} ({name}): y in [{float(y64.min()):.3f}, {float(y64.max()):.3f}], |err| {err:.2e}, e_model {e_y:.2e}")
            assert bool((gate[:, Cc:] == 0).all()) and float(y64.max() - y64.min()) > 0.3
            assert err <= 8 * e_y + 2.0 ** -22, (Cc, N, H, W, name, err, e_y)
            g = gate[:, :Cc]
            ref = DR.aim_mix(X[:, :Cc].double(), Y[:, :Cc].double(), g.double(), sw1, sb1, sw2, sb2)
            e32 = float((DR.aim_mix(X[:, :Cc].float(), Y[:, :Cc].float(), g, sw1, sb1, sw2, sb2).double() - ref).abs().max())
            s64 = DR.spatial_gate(X[:, :Cc].double(), sw1, sb1, sw2, sb2)
            assert float(s64.max() - s64.min()) > 0.3                                     # (the test data spreads the per-pixel gate)
            got = _mix(dev, X, Y, gate, Cc, hs, sw1, sb1, sw2, sb2)
            assert bool((got[:, Cc:] == 0).all()), "pad channels of the mix are not zero"
            R.assert_within_fp16_rounding(got[:, :Cc], ref, e32, what=f"mix C {Cc} {N}x{H}x{W} {name}", family="interaction mix")
            for where in ("x", "y"):
                assert torch.equal(_mix(dev, X, Y, gate, Cc, hs, sw1, sb1, sw2, sb2, in_place=where).view(torch.int16), got.view(torch.int16)), f"in place on {where} differs"
        if N > 1:
            gate = _excite_gelu(dev, c, Cc, hc, cw1, cb1, cw2, cb2)
            whole = _mix(dev, a, c, gate, Cc, hs, sw1, sb1, sw2, sb2)
            for n in range(N):
                g1 = _excite_gelu(dev, c[n:n + 1].contiguous(), Cc, hc, cw1, cb1, cw2, cb2)
                assert torch.equal(g1.view(torch.int32), gate[n:n + 1].contiguous().view(torch.int32))
                o1 = _mix(dev, a[n:n + 1].contiguous(), c[n:n + 1].contiguous(), g1, Cc, hs, sw1, sb1, sw2, sb2)
                assert torch.equal(o1.view(torch.int16), whole[n:n + 1].contiguous().view(torch.int16))


def test_aim_mix_refusals(dev):
    import innfer_amd.lib as L
    G = 64 * 32
    buf = torch.zeros(8 * G, dtype=torch.float16, device=dev)
    out = torch.full((8 * G,), FILL, dtype=torch.float16, device=dev)
    f = torch.zeros(4096, dtype=torch.float32, device=dev)
    w = np.zeros(256 * 64, np.float32)
    mix = lambda Cc, cp, hid, gs=G, g=f.data_ptr(): L.lib.innfer_aim_mix(buf.data_ptr(), gs, buf.data_ptr(), G, out.data_ptr(), G, g, 1, 64, Cc, cp, hid, w.ctypes.data,
                                                                        w.ctypes.data, w.ctypes.data, 0.0, None)
    assert mix(60, 32, 3) == L.ERR_UNSUPPORTED and mix(60, 320, 3) == L.ERR_UNSUPPORTED and mix(70, 64, 3) == L.ERR_UNSUPPORTED and mix(60, 64, 17) == L.ERR_UNSUPPORTED
    assert mix(60, 64, 0) == L.ERR_UNSUPPORTED and mix(60, 64, 3, gs=G - 32) == L.ERR_INVALID and mix(60, 64, 3, g=None) == L.ERR_INVALID
    ex = lambda Cc, cp, hid, nb=4096 * 4: L.lib.innfer_chan_attn_excite_gelu(buf.data_ptr(), G, 1, 64, Cc, cp, hid, w.ctypes.data, w.ctypes.data, w.ctypes.data, w.ctypes.data,
                                                                            f.data_ptr(), None, f.data_ptr() + 4 * 1024, nb, None)
    assert ex(60, 32, 2) == L.ERR_UNSUPPORTED and ex(70, 64, 2) == L.ERR_UNSUPPORTED and ex(60, 64, 65) == L.ERR_UNSUPPORTED and ex(60, 64, 2, nb=16) == L.ERR_WORKSPACE
    torch.cuda.synchronize()
    assert bool((out == FILL).all()) and bool((f == 0).all())
    assert mix(60, 64, 3) == 0 and ex(60, 64, 7) == 0


# ------------------------------------------------------------------------------------------------ 5. the wide LayerNorm
def _ln_launch(dev, x, Cc, gamma, beta, in_place=False):
    import innfer_amd.lib as L
    N, cp, H, W = x.shape
    G, ng = N * H * W * 32, cp // 32
    xin = R.to_slab(x).to(dev)
    g, b = _f32(gamma), _f32(beta)
    if in_place:
        L.check(L.lib.innfer_layer_norm_wide(xin.data_ptr(), G, xin.data_ptr(), G, N * H * W, Cc, cp, g.ctypes.data, b.ctypes.data, 1e-5, None))
        torch.cuda.synchronize()
        return R.from_slab(xin.cpu())
    buf = _slab_out(dev, ng, G)
    L.check(L.lib.innfer_layer_norm_wide(xin.data_ptr(), G, buf.data_ptr() + 2 * GUARD, G, N * H * W, Cc, cp, g.ctypes.data, b.ctypes.data, 1e-5, None))
    torch.cuda.synchronize()
    assert torch.equal(xin.cpu(), R.to_slab(x)), "layer norm wrote to its input"
    return _slab_read(buf, ng, N, H, W, "layer norm")


@pytest.mark.parametrize("Cc,cp", [(360, 384), (500, 512), (180, 192)])
def test_layer_norm_wide(dev, Cc, cp):
    from innfer_amd import synth
    n_chain = cp // 4 + 2
    for i, (N, H, W) in enumerate([(1, 1, 1), (1, 17, 33), (3, 17, 33)]):
        seed = 20000 + 10 * Cc + i
        x = synth.uniform((N, cp, H, W), seed, -1, 1)
        x = x * synth.uniform((N, 1, H, W), seed + 1, 0.25, 4.0) + synth.uniform((N, 1, H, W), seed + 2, -2.0, 2.0)          # pixels differ in scale and offset
        x[:, Cc:] = 7.0                                                                                                     # junk in the pad channels: ignored
        x = torch.from_numpy(np.ascontiguousarray(x, np.float32)).half()
        gamma, beta = torch.from_numpy(synth.uniform((Cc,), seed + 3, 0.5, 1.5)), torch.from_numpy(synth.uniform((Cc,), seed + 4, -0.2, 0.2))
        x64 = x[:, :Cc].double()
        ref = DR.layer_norm(x64, gamma.double(), beta.double())
        mu = x64.mean(1, keepdim=True)
        sigma = torch.sqrt(x64.var(1, unbiased=False, keepdim=True) + 1e-5)
        A = x64.abs().amax(1, keepdim=True)
        ga, be = gamma.double().abs()[None, :, None, None], beta.double().abs()[None, :, None, None]
        gz = ga * ((x64 - mu) / sigma).abs()
        ln_stats = U32 * (((n_chain + 5) / 2 + 7) * gz + (n_chain + 2) * ga * A / sigma + gz + be)          # tests/test_gpu_swinir.py derives it
        got = _ln_launch(dev, x, Cc, gamma, beta)
        assert bool((got[:, Cc:] == 0).all()), "pad channels of the layer norm's result are not zero"
        R.assert_within_fp16_rounding(got[:, :Cc], ref, 0.0, extra=ln_stats, what=f"wide layer norm C {Cc} {N}x{H}x{W}", family=f"wide layer norm, C {Cc}")
        assert torch.equal(_ln_launch(dev, x, Cc, gamma, beta, in_place=True).view(torch.int16), got.view(torch.int16)), "in place differs from out of place"


def test_layer_norm_wide_refusals(dev):
    import innfer_amd.lib as L
    buf = torch.full((64 * 640,), FILL, dtype=torch.float16, device=dev)
    g = np.ones(640, np.float32)
    call = lambda Cc, cp: L.lib.innfer_layer_norm_wide(buf.data_ptr(), 64 * 32, buf.data_ptr(), 64 * 32, 64, Cc, cp, g.ctypes.data, g.ctypes.data, 1e-5, None)
    assert call(520, 576) == L.ERR_UNSUPPORTED and call(300, 352) == L.ERR_UNSUPPORTED and call(400, 384) == L.ERR_UNSUPPORTED and call(0, 64) == L.ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert bool((buf == FILL).all())
    assert call(300, 320) == 0


# ------------------------------------------------------------------------------------------------ 7. networks
def _net(dev, name):
    from innfer_amd.architectures.DAT_arch import DAT
    Cc, nH, split, depths, ef, ups, resi, s, shape, seed = DR.FIXTURES[name]
    net = DAT(in_chans=shape[1], embed_dim=Cc, split_size=list(split), depth=list(depths), num_heads=[nH] * len(depths), expansion_factor=ef, upscale=s, upsampler=ups,
              resi_connection=resi)
    net.load_state_dict(DR.fixture_sd(name), strict=True)
    return net.to(dev).eval()


def _assert_like_storage_model(got, y64, ys, what):
    """max |engine - float64| <= 2 x max |storage model - float64| of the same case (computed here), and >= 99 % of the uint8 codes within +-1."""
    err, es = float((got.double() - y64).abs().max()), float((ys - y64).abs().max())
    share = DR.codes_within_one(got, y64)
    print(f"[dat] {what}: engine max|err| {err:.2e}, storage model {es:.2e}, ratio {err / es:.3f}; codes within +-1: {share:.5f}")
    assert got.shape == y64.shape and torch.isfinite(got).all()
    assert err <= 2 * es, (what, err, es)
    assert share >= 0.99, (what, share)


def launch_formula(Cc, nH, hidden, depths, s, direct, conv3):
    """include/innfer_amd.h, innfer_dat_create: S1 + 2 + B0 (9 + SQ + 2 S1 + SF) + B1 (11 + SQ + 2 S1 + SF) + (R + 1) SR + T."""
    S1, SQ, SF = -(-Cc // 64), 3 * nH // 2, 2 * -(-(hidden // 2) // 64)
    SR = 2 * -(-Cc // 256) + S1 if conv3 else S1
    T = 2 if direct else (4 if s == 3 else 2 + {2: 1, 4: 2}[s])
    B1 = sum(d // 2 for d in depths)
    B0 = sum(depths) - B1
    return S1 + 2 + B0 * (9 + SQ + 2 * S1 + SF) + B1 * (11 + SQ + 2 * S1 + SF) + (len(depths) + 1) * SR + T


def _launches(net, x):
    """Launch count of one forward (innfer_net_forward_timed)."""
    import ctypes as C
    import innfer_amd.lib as L
    N, _, H, W = x.shape
    s = L.lib.innfer_net_scale(net._handle)
    out = torch.empty((N, net.out_nc, H * s, W * s), dtype=torch.float16, device=x.device)
    ws = torch.empty(L.lib.innfer_net_workspace_bytes(net._handle, N, H, W), dtype=torch.uint8, device=x.device)
    n = C.c_int()
    ms = (C.c_float * 2048)()
    L.check(L.lib.innfer_net_forward_timed(net._handle, x.data_ptr(), L.F16, out.data_ptr(), L.F16, N, H, W, ws.data_ptr(), ws.numel(), None, 2048, ms, None, None, None, C.byref(n)))
    return n.value, out


@pytest.mark.parametrize("name", list(DR.FIXTURES))
def test_network_vs_float64(dev, name):
    from innfer_amd import synth
    from innfer_amd.utils import utils as U
    Cc, nH, split, depths, ef, ups, resi, s, shape, seed = DR.FIXTURES[name]
    sd, x, y64, ys = DR.case(name)
    net = _net(dev, name)
    xd = x.to(dev).half()
    y = net(xd)
    assert y.dtype == torch.float16 and tuple(y64.shape) == tuple(y.shape)
    _assert_like_storage_model(y.float().cpu(), y64, ys, name)
    n, yt = _launches(net, xd)
    assert n == launch_formula(Cc, nH, int(Cc * ef), depths, s, ups == "pixelshuffledirect", resi == "3conv") and torch.equal(yt, y), n
    buf = torch.empty(y.shape, dtype=torch.float16, device=dev)
    assert net(xd, out=buf) is buf and torch.equal(buf, y)
    if shape[0] > 1:          # nothing in DAT crosses samples: the pool and the channel attention run per sample
        assert torch.equal(net(xd[1:]), y[1:])
    img = torch.from_numpy(synth.image_u8(shape[2], shape[3], 3, s)).to(dev)
    sep = U.tensor2np(net(U.np2tensor(img.cpu().numpy(), dtype=torch.float16)))
    assert np.array_equal(net.forward_u8(img).cpu().numpy(), sep)
    with pytest.raises(NotImplementedError, match="fp16 mode"):
        net(x.to(dev))
    with pytest.raises(NotImplementedError, match="fp16 mode"):
        net.forward_u8(img, fp16=False)
    assert net.flops(1, shape[2], shape[3]) > 0 and net.tile_batch_bytes(2, 16) > 0


# ------------------------------------------------------------------------------------------------ 8. the Model
@pytest.fixture(scope="module")
def model(tmp_path_factory):
    from innfer_amd.architectures import DAT_arch as A
    from innfer_amd.run import Model
    depths, split = (3, 2), (8, 16)
    sd = DR.fill(3, 60, depths, 6, 2.0, 2, "pixelshuffledirect", "1conv", seed=8)
    bufs = {}
    for i, depth in enumerate(depths):          # every buffer a published checkpoint stores
        for j in range(0, depth, 2):
            for br, (wh, ww) in enumerate(((split[0], split[1]), (split[1], split[0]))):
                bufs[f"layers.{i}.blocks.{j}.attn.attns.{br}.rpe_biases"] = A.rpe_biases(wh, ww).float()
                bufs[f"layers.{i}.blocks.{j}.attn.attns.{br}.relative_position_index"] = A.relative_position_index(wh, ww)
            if (i, j) in A.shifted_blocks(depths):
                bufs[f"layers.{i}.blocks.{j}.attn.attn_mask_0"] = torch.zeros(2, 128, 128)
                bufs[f"layers.{i}.blocks.{j}.attn.attn_mask_1"] = torch.zeros(2, 128, 128)
    path = str(tmp_path_factory.mktemp("dat") / "2x_dat.pth")
    torch.save({"params_ema": dict(sd, **bufs)}, path)
    m = Model(path, arch="infer", scale=None, device="cuda", chop=True, tile_batch=4)
    assert (m.arch, m.scale, m.in_nc, m.out_nc) == ("dat", 2, 3, 3) and m.model.shift_blocks == [(0, 2), (1, 0)] and tuple(m.model.split) == split
    return m


def test_model_chop(dev, model):
    """250 x 330 through the chop path (200-px tiles: the pool and the channel attention run per tile) against the network run tile by tile and the oracle's blend of those
    fp16 tiles, rounded to fp16 as the chop path's is: one fp16 rounding of a value below 2.  run_u8 == the separate conversions; a float32 tensor is refused."""
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


def test_model_run_u8_batch(dev, model):
    from innfer_amd import synth
    m = model
    imgs = [synth.image_u8(40, 56, 3, 61), synth.image_u8(33, 96, 3, 62), synth.image_u8(64, 17, 3, 63), synth.image_u8(5, 7, 3, 64)]
    for a, b in zip(m.run_u8_batch(imgs), [m.run_u8(i) for i in imgs]):
        assert np.array_equal(a, b)
