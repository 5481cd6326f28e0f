"""SAFMN on the GPU (needs an MI355X: `pytest -m gpu`): the feature modulation launch against float64 (one fp16 rounding + 8 e_model, e_model the storage model's own
error on the same case: _conv_ref.assert_within_fp16_rounding, the window-attention tests' form), between guard bands and over NaN pads; whole networks against the
storage model with the header's launch count; the command line from a .pth through the chop path."""
import ctypes as C

import numpy as np
import pytest
import torch

import _conv_ref as R
import _safmn_ref as SM

pytestmark = pytest.mark.gpu

GUARD = 4096


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _safm_case(dev, N, H, W, dim, fill, pad):
    """One launch from slabs of pad64(dim) channels whose pad channels hold `pad` into [guard | groups | a foreign group | guard] of `fill`.  u is negative throughout.
    Returns (result [N, c_pad, H, W], float64 reference, storage model's error)."""
    import innfer_amd.lib as L
    from innfer_amd import synth
    cp, seed = -(-dim // 64) * 64, dim + H
    ng, G = cp // 32, N * H * W * 32
    u = torch.from_numpy(synth.uniform((N, dim, H, W), 9200 + seed, -2.0, -0.05)).half()
    t = torch.from_numpy(synth.uniform((N, dim, H, W), 9201 + seed, -1, 1)).half()
    u[N - 1] *= 0.5
    sd = SM.fill(3, dim, 1, 2.0, 2, seed)
    mw, mb = torch.cat([sd[f'feats.0.safm.mfr.{i}.weight'] for i in range(4)]), torch.cat([sd[f'feats.0.safm.mfr.{i}.bias'] for i in range(4)])
    aw, ab = sd['feats.0.safm.aggr.weight'], sd['feats.0.safm.aggr.bias']
    ref = t.double() + SM.safm(u.double(), mw.double(), mb.double(), aw.double(), ab.double())
    e_model = float((t.double() + SM.safm(u.double(), mw.double(), mb.double(), aw.double(), ab.double(), model=True) - ref).abs().max())
    slab = lambda v: R.to_slab(torch.cat([v, torch.full((N, cp - dim, H, W), pad, dtype=torch.float16)], 1)).to(dev)
    du, dt = slab(u), slab(t)
    buf = torch.full(((ng + 1) * G + 2 * GUARD,), fill, dtype=torch.float16, device=dev)
    f32 = lambda v: np.ascontiguousarray(v.numpy().reshape(v.shape[0], -1), np.float32)
    a = [f32(aw), f32(ab), f32(mw), f32(mb)]
    L.check(L.lib.innfer_safm(du.data_ptr(), G, dt.data_ptr(), G, buf.data_ptr() + 2 * GUARD, G, N, H, W, dim, cp, *[v.ctypes.data for v in a], None))
    raw = buf.cpu()
    same = (lambda v: bool(torch.isnan(v).all())) if fill != fill else (lambda v: bool((v == fill).all()))
    assert same(raw[:GUARD]) and same(raw[GUARD + ng * G:]), "the launch wrote outside its output"
    assert torch.equal(du.cpu().view(torch.int16), slab(u).cpu().view(torch.int16)), "the launch wrote to u"
    return R.from_slab(raw[GUARD:GUARD + ng * G].reshape(ng, N, H, W, 32)), ref, e_model


@pytest.mark.parametrize("N,H,W,dim", [(1, 8, 8, 36), (1, 16, 24, 64), (1, 13, 27, 36), (1, 33, 50, 128), (2, 40, 72, 36), (1, 33, 50, 64), (1, 13, 27, 72), (1, 19, 21, 256)])
def test_safm_vs_float64(dev, N, H, W, dim):
    got, ref, e_model = _safm_case(dev, N, H, W, dim, -3.0, 0.0)
    assert bool((got[:, dim:] == 0).all()), "pad channels of the result are not zero"
    R.assert_within_fp16_rounding(got[:, :dim], ref, e_model, what=f"safm {N}x{H}x{W} dim {dim}", family="safm")


@pytest.mark.parametrize("N,H,W,dim", [(1, 13, 27, 36), (1, 17, 9, 72)])
def test_safm_nan_pads_and_output(dev, N, H, W, dim):
    got, ref, e_model = _safm_case(dev, N, H, W, dim, float("nan"), float("nan"))
    assert bool((got[:, dim:] == 0).all()), "pad channels of the result are not zero over NaN pads"
    R.assert_within_fp16_rounding(got[:, :dim], ref, e_model, what=f"safm over NaN {N}x{H}x{W} dim {dim}", family="safm")


def launch_formula(dim, hidden, n_blocks):
    S1, SH = -(-dim // 64), -(-hidden // 64)
    return S1 + n_blocks * (3 + SH + S1) + 3


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


@pytest.mark.parametrize("name", list(SM.FIXTURES))
def test_network_vs_float64(dev, name):
    from innfer_amd.architectures import get_network
    from innfer_amd.run import infer_from_state_dict
    in_ch, dim, nb, s, shape, _ = SM.FIXTURES[name]
    sd, x, y64, ys = SM.case(name)
    info = infer_from_state_dict({"params_ema": dict(sd)})
    net = get_network(info["net_params"])
    net.load_state_dict(info["state_dict"], strict=True)
    net = net.to(dev).eval()
    assert (info["arch"], net.nf, net.n_blocks, net.hidden, net.upscale, net.in_nc) == ("safmn", dim, nb, 2 * dim, s, in_ch)
    xd = x.to(dev)
    y = net(xd)
    got = y.float().cpu()
    err, es = float((got.double() - y64).abs().max()), float((ys - y64).abs().max())
    print(f"[safmn] {name}: engine max|err| {err:.2e}, storage model {es:.2e}, ratio {err / es:.3f}")
    assert got.shape == y64.shape and torch.isfinite(got).all()
    assert err <= 2 * es, (name, err, es)
    y0, n = _raw_forward(net, xd, 0x00)
    assert n == launch_formula(dim, 2 * dim, nb), n
    assert torch.equal(y0, y) and torch.equal(_raw_forward(net, xd, 0xFF)[0], y), "the result depends on what the workspace held"
    if shape[0] > 1:
        assert torch.equal(net(xd[1:]), y[1:])
    with pytest.raises(NotImplementedError, match="fp16 mode"):
        net(x.float().to(dev))


def test_command_line_from_pth_with_chop(dev, tmp_path):
    """A .pth saved from the float64 model's weights; a ragged 230 x 270 PNG through run.py's main and the default chop: the image Model.run_u8 returns."""
    from innfer_amd import run, synth
    from innfer_amd.utils import utils as U
    path = str(tmp_path / "2x_safmn.pth")
    torch.save({"params": SM.fill(3, 36, 2, 2.0, 2, 5)}, path)
    m = run.Model(path, arch="infer", scale=None, device="cuda", chop=True)
    assert (m.arch, m.scale, m.in_nc) == ("safmn", 2, 3)
    img = synth.image_u8(230, 270, 3, 11)
    want = m.run_u8(img)
    assert want.shape == (460, 540, 3)
    (tmp_path / "in").mkdir()
    U.save_img(img, str(tmp_path / "in" / "a.png"))
    run.main(["-m", path, "-i", str(tmp_path / "in"), "-o", str(tmp_path / "out")])
    assert np.array_equal(U.read_img(str(tmp_path / "out" / "a.png")), want)
