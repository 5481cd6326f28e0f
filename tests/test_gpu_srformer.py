"""SRFormer on the GPU (needs an MI355X: `pytest -m gpu`): the two new launches against float64 on their stored fp16 operands (one fp16 rounding + 8 e_model, e_model
from a float32 CPU model of the declared arithmetic; the depthwise conv adds |f| 2^-20 for common.h fast_gelu, as tests/test_gpu_dat.py), every launch between guard bands;
whole networks by DESIGN.md 3.4m's criterion with the launch count of 3.4q; the Model's chop path and the command line from a .pth."""
import ctypes as C

import numpy as np
import pytest
import torch

import _conv_ref as R
import _srformer_ref as SF

pytestmark = pytest.mark.gpu

FILL, GUARD = -3.0, 4096
GELU_T = 2.0 ** -20


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


# ------------------------------------------------------------------------------------------------ 1. the permuted window attention
def _psa_data(N, Hp, Wp, Cc, nH, ws, seed, gain=1.0):
    from innfer_amd import synth
    q = synth.uniform((N, Cc, Hp, Wp), 7000 + seed, -1, 1) * np.float32(gain)
    kv = synth.uniform((2, N, Cc // 4, Hp, Wp), 7001 + seed, -1, 1)
    for n in range(N):
        q[n] *= np.float32(1.0 + 0.5 * n)
        kv[:, n] *= np.float32(1.0 - 0.25 * n)
    table = synth.uniform(((ws - 1) ** 2, nH), 7002 + seed, -2, 2)
    return torch.from_numpy(q).half(), torch.from_numpy(kv[0]).half(), torch.from_numpy(kv[1]).half(), torch.from_numpy(np.ascontiguousarray(table))


def _psa_launch(dev, q, k, v, table, ws, shift, expect=0, kv_gs=None):
    """From a head-padded q slab and a kv slab of their own into [guard | nH groups | a foreign group | guard].  Returns [N, nH, 32, Hp, Wp] fp16 (cpu)."""
    import innfer_amd.lib as L
    N, Cc, Hp, Wp = q.shape
    nH, d, c4 = table.shape[1], Cc // table.shape[1], Cc // 4
    kg, G = -(-c4 // 32), N * Hp * Wp * 32
    qs = torch.zeros(nH, N, Hp, Wp, 32, dtype=torch.float16)
    dd = min(d, 32)                      # (a refused shape may not fit the slab at all)
    qs[..., :dd] = q[:, :nH * d].reshape(N, nH, d, Hp, Wp).permute(1, 0, 3, 4, 2)[..., :dd]
    kvp = torch.zeros(2, N, kg * 32, Hp, Wp, dtype=torch.float16)
    kvp[0, :, :c4], kvp[1, :, :c4] = k, v
    kvs = kvp.reshape(2, N, kg, 32, Hp, Wp).permute(0, 2, 1, 4, 5, 3).contiguous()                  # [which, group, N, Hp, Wp, 32]
    dq, dkv = qs.to(dev), kvs.to(dev)
    buf = torch.full(((nH + 1) * G + 2 * GUARD,), FILL, dtype=torch.float16, device=dev)
    tb = np.ascontiguousarray(table.numpy().T, np.float32)
    rc = L.lib.innfer_window_attention_perm(dq.data_ptr(), G, dkv.data_ptr(), kv_gs or G, buf.data_ptr() + 2 * GUARD, G, tb.ctypes.data, N, Hp, Wp, Cc, nH, ws, shift, None)
    torch.cuda.synchronize()
    raw = buf.cpu()
    assert torch.equal(dq.cpu(), qs) and torch.equal(dkv.cpu(), kvs), "the attention wrote to its input"
    if expect:
        assert rc == expect and bool((raw == FILL).all()), (rc, "a refused launch wrote to d_out")
        return None
    L.check(rc)
    assert bool((raw[:GUARD] == FILL).all()) and bool((raw[GUARD + nH * G:] == FILL).all()), "the attention wrote outside its output"
    return raw[GUARD:GUARD + nH * G].reshape(nH, N, Hp, Wp, 32).permute(1, 0, 4, 2, 3)


def _psa_check(dev, N, Hp, Wp, Cc, nH, ws, shift, seed, gain=1.0, smin=0.0):
    q, k, v, table = _psa_data(N, Hp, Wp, Cc, nH, ws, seed, gain)
    d = Cc // nH
    ref, smax = SF.psa(q, k, v, table, ws, shift)
    assert smax >= smin, (smax, smin)
    e_model = float((SF.psa(q, k, v, table, ws, shift, torch.float32, model=True)[0].double() - ref).abs().max())
    got = _psa_launch(dev, q, k, v, table, ws, shift)
    assert bool((got[:, :, d:] == 0).all()), "pad channels of the attention's result are not zero"
    what = f"permuted attention ws {ws} {N}x{Hp}x{Wp} C {Cc} nH {nH} shift {shift}" + (f" (|q k^T| up to {smax:.0f})" if smin else "")
    R.assert_within_fp16_rounding(got[:, :, :d].reshape(N, Cc, Hp, Wp), ref, e_model, what=what, family=f"permuted attention ws {ws}")
    return (q, k, v, table), got


@pytest.mark.parametrize("ws", [16, 22, 24])
@pytest.mark.parametrize("Cc,nH", [(60, 6), (180, 6), (64, 2), (96, 4), (256, 8)])
def test_window_attention_perm(dev, ws, Cc, nH):
    for i, side in enumerate((ws, 3 * ws)):
        for shift in (0, ws // 2):
            _psa_check(dev, 1, side, side, Cc, nH, ws, shift, 1000 * ws + 10 * Cc + 2 * i + (shift > 0))


@pytest.mark.parametrize("ws", [16, 22, 24])
def test_window_attention_perm_batch_and_large_scores(dev, ws):
    (q, k, v, table), got = _psa_check(dev, 2, ws, 2 * ws, 60, 6, ws, ws // 2, 500 + ws)
    for n in range(2):
        one = _psa_launch(dev, q[n:n + 1], k[n:n + 1], v[n:n + 1], table, ws, ws // 2)
        assert torch.equal(one.view(torch.int16), got[n:n + 1].contiguous().view(torch.int16)), n
    _psa_check(dev, 1, ws, 2 * ws, 64, 2, ws, ws // 2, 600 + ws, gain=60.0, smin=250.0)


def test_window_attention_perm_refusals(dev):
    import innfer_amd.lib as L
    U, I = L.ERR_UNSUPPORTED, L.ERR_INVALID
    mk = lambda Hp, Wp, Cc, nH, ws: _psa_data(1, Hp, Wp, Cc, nH, ws, 1)
    _psa_launch(dev, *mk(32, 32, 64, 2, 16)[:3], torch.zeros(49, 2), 8, 0, expect=U)             # a window of 8
    _psa_launch(dev, *mk(40, 40, 64, 2, 20)[:3], torch.zeros(361, 2), 20, 0, expect=U)           # a window of 20
    _psa_launch(dev, *mk(16, 24, 64, 2, 16), 16, 0, expect=I)                                     # Wp no multiple of 16
    _psa_launch(dev, *mk(22, 32, 64, 2, 22), 22, 0, expect=I)                                     # Wp no multiple of 22
    _psa_launch(dev, *mk(44, 48, 64, 2, 24), 24, 0, expect=I)         # Hp no multiple of 24
    _psa_launch(dev, *mk(16, 16, 64, 2, 16), 16, 0, expect=I, kv_gs=16 * 16 * 32 - 32)           # a kv group stride below N Hp Wp 32
    _psa_launch(dev, *mk(16, 16, 62, 2, 16), 16, 0, expect=U)                                     # C % 4
    _psa_launch(dev, *mk(16, 16, 64, 3, 16)[:3], torch.zeros(225, 3), 16, 0, expect=U)           # C % nH
    _psa_launch(dev, *mk(16, 16, 64, 1, 16), 16, 0, expect=U)                                     # d 64
    _psa_launch(dev, *mk(16, 16, 72, 9, 16), 16, 0, expect=U)                                     # 9 heads
    _psa_launch(dev, *mk(16, 16, 288, 9, 16), 16, 0, expect=U)                                    # C 288
    _psa_launch(dev, *mk(16, 16, 64, 2, 16), 16, 4, expect=U)                                     # shift 4
    _psa_launch(dev, *mk(22, 22, 64, 2, 22), 22, 8, expect=U)                                     # shift 8 on 22


# ------------------------------------------------------------------------------------------------ 2. the depthwise 5 x 5 conv
@pytest.mark.parametrize("Cc", [40, 120, 360])
def test_dwconv5x5_gelu_add(dev, Cc):
    import innfer_amd.lib as L
    from innfer_amd import synth
    cp = -(-Cc // 64) * 64
    for i, (N, H, W) in enumerate([(2, 3, 5), (2, 17, 33)]):
        seed = 21000 + 10 * Cc + i
        x = torch.from_numpy(synth.uniform((N, cp, H, W), seed, -2, 2)).half()
        x[:, Cc:] = 9.0
        x[:, Cc::3] = float("nan")
        x[:, Cc + 1::3] = float("inf")
        taps = torch.from_numpy(synth.uniform((Cc, 1, 5, 5), seed + 1, -0.35, 0.35))
        bias = torch.from_numpy(synth.uniform((Cc,), seed + 2, -0.5, 0.5))
        xr = x[:, :Cc]
        f64 = torch.nn.functional.conv2d(xr.double(), taps.double(), bias.double(), padding=2, groups=Cc)
        ref = SF.dwconv5(xr, taps, bias)
        e32 = float((SF.dwconv5(xr, taps, bias, torch.float32).double() - ref).abs().max())
        G = N * H * W * 32
        xin = R.to_slab(x).to(dev)
        buf = torch.full(((cp // 32 + 1) * G + 2 * GUARD,), FILL, dtype=torch.float16, device=dev)
        tp, bs = np.ascontiguousarray(taps.numpy().reshape(Cc, 25)), np.ascontiguousarray(bias.numpy())
        L.check(L.lib.innfer_dwconv5x5_gelu_add(xin.data_ptr(), G, buf.data_ptr() + 2 * GUARD, G, N, H, W, Cc, cp, tp.ctypes.data, bs.ctypes.data, None))
        torch.cuda.synchronize()
        raw = buf.cpu()
        assert bool((raw[:GUARD] == FILL).all()) and bool((raw[GUARD + cp // 32 * G:] == FILL).all()), "the depthwise conv wrote outside its output"
        assert torch.equal(xin.cpu().view(torch.int16), R.to_slab(x).view(torch.int16)), "the depthwise conv wrote to its input"
        got = raw[GUARD:GUARD + cp // 32 * G].reshape(cp // 32, N, H, W, 32).permute(1, 0, 4, 2, 3).reshape(N, cp, H, W)
        assert bool((got[:, Cc:] == 0).all()), "pad channels of the depthwise conv's result are not zero"
        R.assert_within_fp16_rounding(got[:, :Cc], ref, e32, extra=f64.abs() * GELU_T, what=f"dwconv5 C {Cc} {N}x{H}x{W}", family="dwconv5 + GELU + input")
        assert L.lib.innfer_dwconv5x5_gelu_add(xin.data_ptr(), G, xin.data_ptr(), G, N, H, W, Cc, cp, tp.ctypes.data, bs.ctypes.data, None) == L.ERR_INVALID


# ------------------------------------------------------------------------------------------------ 3. networks
def launch_formula(Cc, nH, hidden, depths, upsampler, s, padded):
    """S1 + 2 + B (4 + SQ + SK + 2 S1 + SH) + (R + 1) S1 + T + 2 [padded]  ('1conv')."""
    S1, SQ, SK, SH = -(-Cc // 64), -(-nH // 2), -(-Cc // 128), -(-hidden // 64)
    lg = {2: 1, 4: 2}.get(s, 0)
    T = {"pixelshuffledirect": 2, "pixelshuffle": 4 if s == 3 else 2 + lg, "nearest+conv": 3 + lg}[upsampler]
    return S1 + 2 + sum(depths) * (4 + SQ + SK + 2 * S1 + SH) + (len(depths) + 1) * S1 + T + (2 if padded else 0)


def _raw_forward(net, x, pattern):
    """innfer_net_forward_timed on a workspace of the test's own: the first half filled with `pattern`, the second half a guard.  Returns (result, launches)."""
    import innfer_amd.lib as L
    N, _, H, W = x.shape
    s = L.lib.innfer_net_scale(net._handle)
    out = torch.empty((N, net.out_nc, H * s, W * s), dtype=torch.float16, device=x.device)
    need = L.lib.innfer_net_workspace_bytes(net._handle, N, H, W)
    ws = torch.full((2 * need,), 0xA5, dtype=torch.uint8, device=x.device)
    ws[:need] = pattern
    n = C.c_int()
    ms = (C.c_float * 1024)()
    L.check(L.lib.innfer_net_forward_timed(net._handle, x.data_ptr(), L.F16, out.data_ptr(), L.F16, N, H, W, ws.data_ptr(), need, None, 1024, ms, None, None, None, C.byref(n)))
    torch.cuda.synchronize()
    assert bool((ws[need:] == 0xA5).all()), "the forward wrote behind its workspace"
    return out, n.value


@pytest.mark.parametrize("name", list(SF.FIXTURES))
def test_network_vs_float64(dev, name):
    """Measured on the MI355X, engine / storage-model error: C60 ws16 direct x2 1.000 (8.86e-4), C180 ws22 pixelshuffle x4 1.000 (1.50e-3), C96 ws24 nearest+conv x4
    batch of two 1.043 (3.42e-3 / 3.27e-3); every code within +-1."""
    from innfer_amd import synth
    from innfer_amd.architectures import get_network
    from innfer_amd.run import infer_from_state_dict
    from innfer_amd.utils import utils as U
    Cc, nH, depths, ws, shape, ups, s, seed = SF.FIXTURES[name]
    sd, x, y64, ys, _ = SF.case(name)
    info = infer_from_state_dict({"params_ema": dict(sd, **SF.buffers(sd, ws))})
    net = get_network(info["net_params"])
    net.load_state_dict(info["state_dict"], strict=True)
    net = net.to(dev).eval()
    assert (info["arch"], net.nf, net.num_heads, tuple(net.depths), net.window_size, net.upsampler, net.upscale) == ("srformer", Cc, nH, tuple(depths), ws, ups, s)
    xd = x.to(dev).half()
    y = net(xd)
    got = y.float().cpu()
    err, es = float((got.double() - y64).abs().max()), float((ys - y64).abs().max())
    share = SF.SR.codes_within_one(got, y64)
    print(f"[srformer] {name}: engine max|err| {err:.2e}, storage model {es:.2e}, ratio {err / es:.3f}; codes within +-1: {share:.5f}")
    assert got.shape == y64.shape and torch.isfinite(got).all()
    assert err <= 2 * es, (name, err, es)
    assert share >= 0.99, (name, share)
    y0, n = _raw_forward(net, xd, 0x00)
    assert n == launch_formula(Cc, nH, 2 * Cc, depths, ups, s, shape[2] % ws != 0 or shape[3] % ws != 0), n
    assert torch.equal(y0, y) and torch.equal(_raw_forward(net, xd, 0xFF)[0], y), "the result depends on what the workspace held"
    buf = torch.empty(y.shape, dtype=torch.float16, device=dev)
    assert net(xd, out=buf) is buf and torch.equal(buf, y)
    if shape[0] > 1:
        assert torch.equal(net(xd[1:]), y[1:])
    img = torch.from_numpy(synth.image_u8(shape[2], shape[3], 3, s)).to(dev)
    sep = U.tensor2np(net(U.np2tensor(img.cpu().numpy(), dtype=torch.float16)))
    assert np.array_equal(net.forward_u8(img).cpu().numpy(), sep)
    with pytest.raises(NotImplementedError, match="fp16 mode"):
        net(x.to(dev))


# ------------------------------------------------------------------------------------------------ 4. the Model and the command line
def test_model_chop_and_command_line(dev, tmp_path):
    """A .pth under params_ema with the buffers; 250 x 330 through the chop path (200-px tiles, each padded to 220 inside the engine) against the network run tile by tile
    and the oracle's blend of those fp16 tiles, rounded to fp16 as the chop path's is: they differ in the blend's arithmetic alone, one fp16 rounding of a value below 2.
    `python run.py -m <that .pth>` writes the image run_u8 returns."""
    import os
    import subprocess
    import sys
    import oracle
    from innfer_amd import synth
    from innfer_amd.run import Model
    from innfer_amd.utils import utils as U
    sd = SF.fill(3, 60, (2,), 6, 2.0, 2, "pixelshuffle", "1conv", 22, seed=8)
    path = str(tmp_path / "2x_srformer.pth")
    torch.save({"params_ema": dict(sd, **SF.buffers(sd, 22))}, path)
    m = Model(path, arch="infer", scale=None, device="cuda", chop=True, tile_batch=4)
    assert (m.arch, m.scale, m.in_nc, m.out_nc) == ("srformer", 2, 3, 3)
    x = torch.from_numpy(synth.uniform((1, 3, 250, 330), 52))
    y = m(x.to(dev).half()).float().cpu()
    assert tuple(y.shape) == (1, 3, 500, 660)
    tiles = oracle.extract_patches_2d(x, (200, 200), [0.5, 0.5], batch_first=True).squeeze(0)
    ht = torch.cat([m.model(tiles[i:i + 1].to(dev).half()).float().cpu() for i in range(tiles.shape[0])], 0)
    want = oracle.recompose_tensor(ht, 250, 330, step=0.5, scale=2).half().float()
    assert float((y - want).abs().max()) <= 2.0 ** -10, float((y - want).abs().max())
    img = synth.image_u8(250, 330, 3, 9)
    got = m.run_u8(img)
    assert np.array_equal(got, U.tensor2np(m(U.np2tensor(img, dtype=torch.float16))))
    (tmp_path / "in").mkdir()
    U.save_img(img, str(tmp_path / "in" / "a.png"))
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    subprocess.run([sys.executable, os.path.join(root, "run.py"), "-m", path, "-i", str(tmp_path / "in"), "-o", str(tmp_path / "out")], check=True, cwd=str(tmp_path), timeout=120)
    assert np.array_equal(U.read_img(str(tmp_path / "out" / "a.png")), got)
