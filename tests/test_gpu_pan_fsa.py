"""PAN's self-attention block (FSA, csrc/pan.hip + csrc/f32ops.hip), one launch at a time, against float64 (needs an MI355X: `pytest -m gpu`).

The network tests do not hold this block: FSA.gamma of the synthetic weights is -0.003, their f . g scores span < 0.1 per row (a softmax uniform to three digits) and
the up-convs damp what is left by 100x -- deleting the block from the engine passed the whole suite, fp32 mode included (the table in tests/test_pan_fsa_cpu.py).
Here each launch runs alone through innfer_pan_attention / innfer_pan_maxpool / innfer_pan_fsa_combine, the launch functions the two forwards call.

Attention   every case of tests/_pan_attention_ref.py (13 key counts x 4 operand families) x form 0 (pan_attention), 1 (pan_attn_prep + pan_attention_mfma<false>),
            2 (<true>) against exact float64.  Bounds, per case, never taken from the kernel: form 0: 8 e32 (e32: torch float32 on the CPU against exact); form 1:
            8 e_model(split = False); form 2: 8 (e_model(split = True) + e32) -- e_model: the numpy model of the kernel's declared roundings against exact.
            tests/test_pan_fsa_cpu.py proves that five planted faults miss these bounds by >= 10x.  Columns 50 .. 63 of the fgh rows hold NaN, the workspace is 0xFF
            before each launch, the output buffer is one image longer than needed and its tail keeps the sentinel.  N = 3 at Np = 33 / 129 / 513: every image
            bit-equal to its own N = 1 launch.
Max-pool    against F.max_pool2d, equal as values; the slab form's pad channels zero; guards around the output.
Combine     against float64 gamma * F.interpolate(att, bicubic, align_corners = False) + inp: fp16 ulp16(max(|ref|, |got|)) / 2 + 8 e32, fp32 8 e32 (e32: the float32
            CPU evaluation against float64; the convention of tests/test_gpu_conv_forms.py); where W == 4 wp the strip and the one-pixel kernels agree bit for bit.
Wiring      one PAN per precision whose FSA weights are scaled until the block shows (f, g x 20, h x 6, gamma 2) against oracle.pan_forward at the networks' bounds.

Measured on the MI355X -- see docs/KERNELS.md section 3 (FSA block, launch by launch); test_report prints the table.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _pan_attention_ref as R
from _conv_ref import ulp16

pytestmark = pytest.mark.gpu

SENT = -3.0
GUARD = 4096
F16, F32 = 0, 1
OK, ERR_INVALID, ERR_WORKSPACE = 0, -1, -5
FP32_TOL = 1e-4
MEASURED = {}          # (kernel, form, family) -> [largest reference error (e32 / e_model), worst err / bound]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def record(key, eref, ratio):
    m = MEASURED.setdefault(key, [0.0, 0.0])
    m[0], m[1] = max(m[0], eref), max(m[1], ratio)


def stream():
    return torch.cuda.current_stream().cuda_stream


# ------------------------------------------------------------------------------------------------ attention
def launch_attention(dev, rows, bf, bg, bh, form):
    """One innfer_pan_attention of rows [N][Np][64] on cuda:0 -> fp32 [N][Np][40]; checks the tail of the output buffer and the bytes behind the workspace."""
    import innfer_amd.lib as L
    N, Np = rows.shape[0], rows.shape[1]
    d_fgh = torch.from_numpy(np.array(rows, order="C")).to(dev)
    d_b = [torch.from_numpy(np.array(b)).to(dev) for b in (bf, bg, bh)]
    need = L.lib.innfer_pan_attention_workspace_bytes(N, Np, form)
    assert (need == 0) == (form == 0)
    d_ws = torch.full((need + GUARD,), 0xFF, dtype=torch.uint8, device=dev)
    body = N * Np * R.C
    d_out = torch.full((body + Np * R.C,), SENT, dtype=torch.float32, device=dev)
    rc = L.lib.innfer_pan_attention(d_fgh.data_ptr(), d_b[0].data_ptr(), d_b[1].data_ptr(), d_b[2].data_ptr(), N, Np, form, d_out.data_ptr(),
                                    d_ws.data_ptr() if need else None, need, stream())
    torch.cuda.synchronize()
    assert rc == OK, (rc, L.last_error())
    out = d_out.cpu().numpy()
    assert (out[body:] == SENT).all(), f"Np {Np} form {form}: the launch wrote behind its {N} image(s)"
    assert (d_ws[need:] == 0xFF).all().item(), f"Np {Np} form {form}: the launch wrote behind its workspace"
    return out[:body].reshape(N, Np, R.C)


@pytest.mark.parametrize("c", R.cases(), ids=str)
def test_attention_vs_float64(dev, c):
    rows, bf, bg, bh, f, g, h = R.operands(c)
    ref, e32, em, ems = R.figures(c)
    for form in (0, 1, 2):
        got = launch_attention(dev, rows[None], bf, bg, bh, form)[0].astype(np.float64)
        assert np.isfinite(got).all(), f"{c} form {form}: non-finite values"
        e, b = float(np.abs(got - ref).max()), R.bound(c, form)
        ratio = e / b if b > 0 else (0.0 if e == 0 else float("inf"))
        print(f"[pan-fsa] attention {c} form {form}: e32 {e32:.2e} e_model {em:.2e} / split {ems:.2e}; err {e:.2e} bound {b:.2e} err/bound {ratio:.3f}")
        record(("attention", form, c.family), (e32, em, ems)[form], ratio)
        assert e <= b, f"{c} form {form}: |device - exact| {e:.3e} > {b:.3e}"


@pytest.mark.parametrize("Np", R.NP_BATCH)
def test_attention_batch_images_equal_their_own_launches(dev, Np):
    """N = 3 (three families' rows under the first one's biases): every image bit-equal to its own N = 1 launch, and the first within its case's bound."""
    cs = [c for c in R.cases() if c.Np == Np and c.family in ("peaked", "ramp", "negative")]
    rows = np.stack([R.operands(c)[0] for c in cs])
    _, bf, bg, bh = R.operands(cs[0])[:4]
    for form in (0, 1, 2):
        got = launch_attention(dev, rows, bf, bg, bh, form)
        for n in range(3):
            own = launch_attention(dev, rows[n:n + 1], bf, bg, bh, form)
            assert np.array_equal(got[n].view(np.uint32), own[0].view(np.uint32)), f"Np {Np} form {form}: image {n} of the batch differs from its own launch"
        assert np.abs(got[0].astype(np.float64) - R.figures(cs[0])[0]).max() <= R.bound(cs[0], form)


def test_attention_refusals(dev):
    import innfer_amd.lib as L
    c = R.Case("flat", 33, 1)
    rows, bf, bg, bh = R.operands(c)[:4]
    d_fgh = torch.from_numpy(np.array(rows)).to(dev)
    d_b = [torch.from_numpy(np.array(b)).to(dev) for b in (bf, bg, bh)]
    d_out = torch.full((33 * R.C,), SENT, dtype=torch.float32, device=dev)
    need = L.lib.innfer_pan_attention_workspace_bytes(1, 33, 2)
    assert need > L.lib.innfer_pan_attention_workspace_bytes(1, 33, 1) > 0
    assert L.lib.innfer_pan_attention_workspace_bytes(1, 0, 1) == 0
    d_ws = torch.zeros(need, dtype=torch.uint8, device=dev)
    call = lambda Np, form, ws, nbytes: L.lib.innfer_pan_attention(d_fgh.data_ptr(), d_b[0].data_ptr(), d_b[1].data_ptr(), d_b[2].data_ptr(), 1, Np, form,
                                                                   d_out.data_ptr(), ws, nbytes, stream())
    assert call(0, 1, d_ws.data_ptr(), need) == ERR_INVALID
    assert call(33, 3, d_ws.data_ptr(), need) == ERR_INVALID and call(33, -1, d_ws.data_ptr(), need) == ERR_INVALID
    assert call(33, 2, d_ws.data_ptr(), need - 1) == ERR_WORKSPACE and call(33, 1, None, need) == ERR_WORKSPACE
    torch.cuda.synchronize()
    assert (d_out == SENT).all().item(), "a refused launch wrote"
    assert call(33, 2, d_ws.data_ptr(), need) == OK
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ slabs
def to_slab(x, junk):
    """NCHW float -> blocked fp16 slab [ceil(C / 32)][N * H * W][32]; the pad channels hold `junk`."""
    N, Cc, H, W = x.shape
    G = (Cc + 31) // 32
    s = torch.full((N * H * W, G * 32), junk, dtype=torch.float16)
    s[:, :Cc] = x.permute(0, 2, 3, 1).reshape(N * H * W, Cc).half()
    return s.reshape(N * H * W, G, 32).permute(1, 0, 2).contiguous()


def from_slab(s, N, Cc, H, W):
    """-> (NCHW of the first Cc channels, the pad channels [N * H * W][32 G - Cc])"""
    G = s.shape[0]
    flat = s.permute(1, 0, 2).reshape(N * H * W, G * 32)
    return flat[:, :Cc].reshape(N, H, W, Cc).permute(0, 3, 1, 2).contiguous(), flat[:, Cc:]


def guarded(body, dev, dtype):
    return torch.full((body + 2 * GUARD,), SENT, dtype=dtype, device=dev)


def guards_kept(buf):
    return (buf[:GUARD] == SENT).all().item() and (buf[-GUARD:] == SENT).all().item()


# ------------------------------------------------------------------------------------------------ max-pool
POOL_SIZES = [(4, 4), (5, 7), (8, 9), (16, 64), (37, 21)]


@pytest.mark.parametrize("dtype,Cc", [(F16, 24), (F16, 40), (F16, 64), (F32, 40)])
@pytest.mark.parametrize("H,W", POOL_SIZES)
def test_maxpool_equals_torch(dev, H, W, dtype, Cc):
    import innfer_amd.lib as L
    N, hp, wp = 2, H // 4, W // 4
    x = torch.from_numpy(np.random.default_rng(100 * H + W + Cc).uniform(-1, 1, (N, Cc, H, W)).astype(np.float32))
    x[:, ::3] = -x[:, ::3].abs()                      # every third channel: all-negative windows (a maximum started from 0 would show)
    if dtype == F16:
        x = x.half().float()
    ref = F.max_pool2d(x, 4, 4)
    assert (ref < 0).any() and (ref > 0).any()
    if dtype == F16:
        G = (Cc + 31) // 32
        d_in = to_slab(x, 5.0).to(dev)
        body = G * N * hp * wp * 32
        d_out = guarded(body, dev, torch.float16)
        rc = L.lib.innfer_pan_maxpool(d_in.data_ptr(), F16, N, Cc, H, W, d_out.data_ptr() + 2 * GUARD, stream())
        torch.cuda.synchronize()
        assert rc == OK, L.last_error()
        assert guards_kept(d_out), "pan_maxpool wrote outside its output slab"
        got, padch = from_slab(d_out[GUARD:-GUARD].cpu().reshape(G, N * hp * wp, 32), N, Cc, hp, wp)
        assert (padch == 0).all(), "pad channels of the pooled slab are not zero"
        got = got.float()
    else:
        d_in = x.to(dev)
        d_out = guarded(N * Cc * hp * wp, dev, torch.float32)
        rc = L.lib.innfer_pan_maxpool(d_in.data_ptr(), F32, N, Cc, H, W, d_out.data_ptr() + 4 * GUARD, stream())
        torch.cuda.synchronize()
        assert rc == OK, L.last_error()
        assert guards_kept(d_out), "f32_maxpool4 wrote outside its output"
        got = d_out[GUARD:-GUARD].cpu().reshape(N, Cc, hp, wp)
    assert torch.equal(got, ref), f"{H}x{W} C {Cc} dtype {dtype}: {(got != ref).sum().item()} pooled values differ"
    record(("maxpool", "fp16 slab" if dtype == F16 else "fp32", "-"), 0.0, 0.0)


def test_maxpool_refuses_less_than_a_window(dev):
    import innfer_amd.lib as L
    d = torch.zeros(4096, dtype=torch.float32, device=dev)
    for H, W in ((3, 8), (8, 3)):
        for dtype in (F16, F32):
            assert L.lib.innfer_pan_maxpool(d.data_ptr(), dtype, 1, 8, H, W, d.data_ptr(), stream()) == ERR_INVALID
    assert L.lib.innfer_pan_maxpool(d.data_ptr(), 2, 1, 8, 8, 8, d.data_ptr(), stream()) == ERR_INVALID


# ------------------------------------------------------------------------------------------------ combine
COMBINE_SIZES = [(4, 4), (7, 5), (8, 8), (12, 8), (9, 8), (16, 64), (9, 33), (37, 45)]
GAMMAS = (1.5, -0.7, 0.0)


def combine_launch(dev, att, inp, gamma, dtype, form, H, W):
    """att [N][hp * wp][C] fp32, inp NCHW -> NCHW result of one innfer_pan_fsa_combine (fp16: through slabs with junk pad channels in inp)."""
    import innfer_amd.lib as L
    N, Cc = inp.shape[0], inp.shape[1]
    hp, wp = H // 4, W // 4
    d_att = att.to(dev)
    d_gamma = torch.tensor([gamma], dtype=torch.float32, device=dev)
    d_scr = guarded(N * Cc * hp * wp, dev, torch.float32)
    if dtype == F16:
        G = (Cc + 31) // 32
        d_in = to_slab(inp, 5.0).to(dev)
        d_out = guarded(G * N * H * W * 32, dev, torch.float16)
        rc = L.lib.innfer_pan_fsa_combine(d_att.data_ptr(), hp, wp, Cc, d_in.data_ptr(), F16, N, H, W, d_gamma.data_ptr(), form, d_out.data_ptr() + 2 * GUARD,
                                          None, stream())
        torch.cuda.synchronize()
        assert rc == OK, L.last_error()
        assert guards_kept(d_out), "the combine wrote outside its output slab"
        got, padch = from_slab(d_out[GUARD:-GUARD].cpu().reshape(G, N * H * W, 32), N, Cc, H, W)
        assert (padch == 0).all(), "pad channels of the combined slab are not zero"
        return got
    d_in = inp.to(dev)
    d_out = guarded(N * Cc * H * W, dev, torch.float32)
    rc = L.lib.innfer_pan_fsa_combine(d_att.data_ptr(), hp, wp, Cc, d_in.data_ptr(), F32, N, H, W, d_gamma.data_ptr(), form, d_out.data_ptr() + 4 * GUARD,
                                      d_scr.data_ptr() + 4 * GUARD, stream())
    torch.cuda.synchronize()
    assert rc == OK, L.last_error()
    assert guards_kept(d_out) and guards_kept(d_scr), "the combine wrote outside its output or its scratch"
    return d_out[GUARD:-GUARD].cpu().reshape(N, Cc, H, W)


@pytest.mark.parametrize("dtype", [F16, F32], ids=["fp16", "fp32"])
@pytest.mark.parametrize("H,W", COMBINE_SIZES)
def test_combine_vs_float64(dev, H, W, dtype):
    N, Cc, hp, wp = 2, 40, H // 4, W // 4
    r = np.random.default_rng(7000 + 100 * H + W)
    att = torch.from_numpy(r.uniform(-1, 1, (N, hp * wp, Cc)).astype(np.float32))
    inp = torch.from_numpy(r.uniform(-1, 1, (N, Cc, H, W)).astype(np.float32))
    if dtype == F16:
        inp = inp.half().float()
    a_nchw = att.reshape(N, hp, wp, Cc).permute(0, 3, 1, 2).contiguous()
    up64 = F.interpolate(a_nchw.double(), size=(H, W), mode="bicubic", align_corners=False)
    up32 = F.interpolate(a_nchw, size=(H, W), mode="bicubic", align_corners=False)
    strip = W == 4 * wp
    for gamma in GAMMAS:
        ref = gamma * up64 + inp.double()
        e32 = ((torch.tensor(gamma, dtype=torch.float32) * up32 + inp).double() - ref).abs().max().item()
        got = {form: combine_launch(dev, att, inp, gamma, dtype, form, H, W) for form in (0, 1)}
        for form in (0, 1):
            g = got[form].double()
            assert torch.isfinite(g).all()
            bound = 8.0 * e32 + (ulp16(torch.maximum(g.abs(), ref.abs())) / 2 if dtype == F16 else 0.0)
            d = (g - ref).abs()
            ok = d <= bound
            ratio = torch.where(d > 0, d / bound, torch.zeros_like(d)).max().item()          # (gamma 0 in fp32: bound 0, and nothing may differ)
            kernel = ("strip" if strip and form == 0 else "one-pixel")
            print(f"[pan-fsa] combine {'fp16' if dtype == F16 else 'fp32'} {H}x{W} gamma {gamma} {kernel}: e32 {e32:.2e} worst err/bound {ratio:.3f}")
            record(("combine " + ("fp16" if dtype == F16 else "fp32"), kernel, "-"), e32, ratio)
            assert ok.all(), f"{H}x{W} gamma {gamma} form {form}: {(~ok).sum().item()} values beyond the bound, worst err/bound {ratio:.3f}"
        if strip:
            assert torch.equal(got[0].view(torch.int16 if dtype == F16 else torch.int32), got[1].view(torch.int16 if dtype == F16 else torch.int32)), \
                f"{H}x{W} gamma {gamma}: the strip kernel and the one-pixel kernel differ in {(got[0] != got[1]).sum().item()} values"


# ------------------------------------------------------------------------------------------------ the wiring
@pytest.mark.parametrize("fp32", [False, True], ids=["fp16", "fp32"])
def test_network_with_a_visible_fsa_block(dev, fp32):
    """PAN nb = 4, seed 41, 50 x 70 (Np = 204: a ragged block), FSA.conv_f / conv_g x 20, conv_h x 6, gamma = 2: against the oracle at the networks' bounds.  With
    these weights the oracle itself says what a broken block costs: attention dropped 4.1e-2, uniform softmax 1.2e-2 (recomputed and asserted here), keys permuted
    1.8e-2, no rescale 3.0e-3, ragged tail dropped 6.1e-4."""
    import oracle
    from innfer_amd import synth
    from innfer_amd.architectures import get_network
    from innfer_amd.utils.defaults import get_network_G_config
    net = get_network(get_network_G_config({"type": "pan", "nb": 4}, 4))
    shapes = {k: tuple(v.shape) for k, v in net.state_dict().items()}
    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in synth.fill_state_dict(shapes, 41).items()}
    for k, s in (("FSA.conv_f", 20.0), ("FSA.conv_g", 20.0), ("FSA.conv_h", 6.0)):
        sd[k + ".weight"], sd[k + ".bias"] = sd[k + ".weight"] * s, sd[k + ".bias"] * s
    sd["FSA.gamma"] = torch.full_like(sd["FSA.gamma"], 2.0)
    x = torch.from_numpy(synth.uniform((1, 3, 50, 70), 304))
    dropped, uniform = dict(sd), dict(sd)
    dropped["FSA.gamma"] = torch.zeros_like(sd["FSA.gamma"])
    for k in ("FSA.conv_f.weight", "FSA.conv_f.bias", "FSA.conv_g.weight", "FSA.conv_g.bias"):
        uniform[k] = torch.zeros_like(sd[k])
    with torch.no_grad():
        ref = oracle.pan_forward(sd, x, nb=4, scale=4)
        e_drop = (oracle.pan_forward(dropped, x, nb=4, scale=4) - ref).abs().max().item()
        e_uni = (oracle.pan_forward(uniform, x, nb=4, scale=4) - ref).abs().max().item()
    lim = max(1.0, ref.abs().max().item())
    b32, b16 = FP32_TOL * lim, 1e-2 * lim
    print(f"[pan-fsa] wiring: oracle with the attention dropped {e_drop:.2e}, with a uniform softmax {e_uni:.2e}; bounds fp32 {b32:.2e} fp16 {b16:.2e}")
    assert e_drop > 10 * b32 and e_uni > 10 * b32 and e_drop > b16
    net.load_state_dict(sd, strict=True)
    net = net.to(dev).eval()
    if fp32:
        y = net(x.to(dev))
        assert y.dtype == torch.float32
        e = (y.cpu() - ref).abs().max().item()
        print(f"[pan-fsa] wiring fp32 mode: max {e:.2e} (bound {b32:.2e})")
        record(("network", "fp32 mode", "-"), 0.0, e / b32)
        assert e < b32, e
    else:
        y = net(x.to(dev).half())
        d = (y.float().cpu() - ref).abs()
        print(f"[pan-fsa] wiring fp16: max {d.max().item():.2e} mean {d.mean().item():.2e} (bounds {b16:.2e} / 1.5e-3)")
        record(("network", "fp16", "-"), 0.0, d.max().item() / b16)
        assert d.max().item() < b16 and d.mean().item() < 1.5e-3, (d.max().item(), d.mean().item())


def test_report():
    """The table of docs/KERNELS.md section 3: per kernel, form and family the largest reference error and the worst err / bound of this run."""
    print("\n[pan-fsa] kernel | form | family | largest e32 / e_model | worst err / bound")
    for (kernel, form, fam), (eref, ratio) in sorted(MEASURED.items(), key=lambda kv: tuple(map(str, kv[0]))):
        print(f"[pan-fsa] {kernel} | {form} | {fam} | {eref:.1e} | {ratio:.3f}")
