"""Parity of the HIP path (through the C ABI) against the oracle and the golden
vectors generated from the reference.  Needs an MI355X: `pytest -m gpu`.

Tolerances:
  fp16 HIP path vs fp32 oracle / golden .......... max-abs <= 1e-2 on O(1) outputs
  fp16 HIP path vs the reference's own fp16 mode . max-abs <= 4e-3 (golden G11)
  tiles, blend (fp32), uint8 pre/post, geometry .. bit-exact
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _sd(shapes, seed=0):
    from innfer_amd import synth
    return {k: torch.from_numpy(v) for k, v in synth.fill_state_dict(shapes, seed).items()}


# ------------------------------------------------------------------ single conv
def _run_conv(dev, x, w, b, K, act=0, up=False, res1=None, s1=1.0, res2=None, s2=1.0,
              in_extra=0, out_channels=None, out_off=0, rows=None, reflect=False, dilation=0, res1_is_input=False, res1_from_lds=False, plane_rows=None):
    """x [N,C,Hs,Ws] fp16 (cpu), w [K,C,3,3] fp32.  Runs the HIP conv on blocked-NHWC slabs
    ([C/32][N*H*W][32]) and returns (NCHW fp32 result, raw output slab [groups,N,H,W,32]) on the cpu.
    64-channel output groups exist in two row orders (innfer_conv_args.plane_rows): unless one is asked for, both run and must agree bit for bit."""
    import innfer_amd.lib as L
    if plane_rows is None and K % 64 == 0 and not dilation and out_off % 32 == 0:
        kw = dict(act=act, up=up, res1=res1, s1=s1, res2=res2, s2=s2, in_extra=in_extra, out_channels=out_channels, out_off=out_off, rows=rows, reflect=reflect,
                  dilation=dilation, res1_is_input=res1_is_input, res1_from_lds=res1_from_lds)
        r0, o0 = _run_conv(dev, x, w, b, K, plane_rows=0, **kw)
        r1, o1 = _run_conv(dev, x, w, b, K, plane_rows=1, **kw)
        assert torch.equal(r0, r1) and torch.equal(o0, o1), "plane row order != lane-contiguous row order"
        return r1, o1
    plane_rows = int(bool(plane_rows))
    N, Cc, Hs, Ws = x.shape
    H, W = (2 * Hs, 2 * Ws) if up else (Hs, Ws)
    in_groups = (Cc + in_extra) // 32
    g_in = N * Hs * Ws * 32
    slab = torch.full((in_groups, N, Hs, Ws, 32), 7.0, dtype=torch.float16, device=dev)   # junk in unused groups
    L.check(L.lib.innfer_nchw_to_slab(x.to(dev).contiguous().data_ptr(), L.F16, slab.data_ptr(), g_in, 0,
                                      N, Cc, Hs, Ws, None))
    nbytes = L.lib.innfer_conv3x3_packed_bytes(K, Cc)
    packed = np.zeros(nbytes, dtype=np.uint8)
    wc = np.ascontiguousarray(w.numpy())
    L.check(L.lib.innfer_pack_conv3x3_rows(wc.ctypes.data, K, Cc, plane_rows, packed.ctypes.data))
    d_packed = torch.from_numpy(packed).to(dev)
    d_bias = b.float().to(dev)
    out_channels = out_channels or max(K, 32)
    g_out = N * H * W * 32
    out = torch.full((out_channels // 32, N, H, W, 32), -3.0, dtype=torch.float16, device=dev)
    a = L.ConvArgs()
    a.d_in, a.in_group_stride, a.C = slab.data_ptr(), g_in, Cc
    a.d_packed, a.d_bias = d_packed.data_ptr(), d_bias.data_ptr()
    a.d_out, a.out_group_stride, a.out_ch_off, a.K = out.data_ptr(), g_out, out_off, K
    a.N, a.H, a.W, a.act, a.upsample2x = N, H, W, act, int(up)
    a.plane_rows = plane_rows
    keep = [slab, d_packed, d_bias]
    if res1_is_input:       # residual 1 = the first K channels of the conv's own input slab (x5 * 0.2 + x of an RDB)
        a.d_res1, a.res1_group_stride, a.res1_scale = slab.data_ptr(), g_in, s1
        a.res1_from_input = int(res1_from_lds)      # innfer_conv_args.res1_from_input: x from the conv's own staged LDS tiles (conv3x3_pc RLDS)
        res1 = None
    for name, r, sc in (("1", res1, s1), ("2", res2, s2)):
        if r is not None:
            rs = torch.empty((max(K, 32) // 32, N, H, W, 32), dtype=torch.float16, device=dev)
            L.check(L.lib.innfer_nchw_to_slab(r.to(dev).contiguous().data_ptr(), L.F16, rs.data_ptr(), g_out, 0, N, K, H, W, None))
            setattr(a, f"d_res{name}", rs.data_ptr()); setattr(a, f"res{name}_group_stride", g_out); setattr(a, f"res{name}_scale", sc)
            keep.append(rs)
    if rows:
        a.row_begin, a.row_end = rows
    a.reflect_pad = int(reflect)
    a.dilation = int(dilation)
    L.check(L.lib.innfer_conv3x3_f16(C.byref(a), None))
    torch.cuda.synchronize()
    res = torch.empty((N, K, H, W), dtype=torch.float32, device=dev)
    L.check(L.lib.innfer_slab_to_nchw(out.data_ptr(), g_out, out_off, res.data_ptr(), L.F32, N, K, H, W, None))
    torch.cuda.synchronize()
    return res.cpu(), out.cpu()


def _ref_conv(x, w, b, act=0, up=False, res1=None, s1=1.0, res2=None, s2=1.0):
    xx = x.float()
    if up:
        xx = F.interpolate(xx, scale_factor=2.0, mode="nearest")
    y = F.conv2d(xx, w.half().float(), b.float(), padding=1)
    if act == 1:
        y = F.leaky_relu(y, 0.2)
    elif act == 2:
        y = F.relu(y)
    if res1 is not None:
        y = y * s1 + res1.float()
    if res2 is not None:
        y = y * s2 + res2.float()
    return y


@pytest.mark.parametrize("Cc,K,H,W,N", [
    (64, 32, 16, 32, 1), (96, 32, 37, 45, 2), (128, 32, 8, 70, 1), (160, 32, 33, 33, 1),
    (192, 64, 21, 50, 2), (64, 64, 16, 16, 1), (64, 16, 19, 40, 1), (32, 32, 5, 3, 1), (64, 64, 1, 1, 1),
])
def test_conv_shapes(dev, Cc, K, H, W, N):
    from innfer_amd import synth
    x = torch.from_numpy(synth.uniform((N, Cc, H, W), 1, -1, 1)).half()
    w = torch.from_numpy(synth.uniform((K, Cc, 3, 3), 2, -1, 1)) / np.sqrt(9 * Cc)
    b = torch.from_numpy(synth.uniform((K,), 3, -1, 1))
    got, _ = _run_conv(dev, x, w, b, K, act=1, in_extra=32)
    ref = _ref_conv(x, w, b, act=1)
    assert (got - ref).abs().max().item() < 4e-3


def test_conv_random_shapes_fuzz(dev):
    """Seeded sweep over what the trunk kernels are parameterised on -- input / output channel counts, image sizes around the tile sizes (24 x 32,
    16 x 32), batches (N > 1 takes the image-canvas form when that saves tiles: cells, gutters, tiles that straddle images), activation, one
    or two residuals, nearest-2x input, reflection / replication padding, output channel offsets -- against F.conv2d on the same fp16 operands."""
    from innfer_amd import synth
    rng = np.random.RandomState(20260101)
    for case in range(48):
        K = int(rng.choice([16, 32, 64]))
        Cc = int(rng.choice([32, 64, 96, 128, 160, 192]))
        N = int(rng.choice([1, 1, 2, 3, 5]))
        H, W = int(rng.randint(1, 70)), int(rng.randint(1, 90))
        if case % 6 == 0:
            H, W = int(rng.choice([24, 48, 16, 32, 25, 47])), int(rng.choice([32, 64, 33, 63, 31]))      # whole tiles and one off
        act = int(rng.choice([0, 1, 2]))
        up = bool(rng.rand() < 0.15) and N == 1
        pad = 0 if (up or K < 32) else int(rng.choice([0, 0, 0, 1, 2]))      # reflection / replication padding: the 32- / 64-output slab kernels
        if pad == 1 and min(H, W) < 2:
            pad = 0
        use_r1 = K >= 32 and rng.rand() < 0.4
        use_r2 = use_r1 and rng.rand() < 0.5
        Hs, Ws = (H, W)
        Ho, Wo = (2 * H, 2 * W) if up else (H, W)
        x = torch.from_numpy(synth.uniform((N, Cc, Hs, Ws), 1000 + case, -1, 1)).half()
        w = torch.from_numpy(synth.uniform((K, Cc, 3, 3), 2000 + case, -1, 1)) / np.sqrt(9 * Cc)
        b = torch.from_numpy(synth.uniform((K,), 3000 + case, -1, 1))
        r1 = torch.from_numpy(synth.uniform((N, K, Ho, Wo), 4000 + case, -1, 1)).half() if use_r1 else None
        r2 = torch.from_numpy(synth.uniform((N, K, Ho, Wo), 5000 + case, -1, 1)).half() if use_r2 else None
        off = 0 if K == 64 else int(rng.choice([0, 16])) if K == 16 else 0
        got, _ = _run_conv(dev, x, w, b, K, act=act, up=up, res1=r1, s1=0.2, res2=r2, s2=0.2, in_extra=int(rng.choice([0, 32])),
                           out_channels=64, out_off=off, reflect=pad)
        xx = F.interpolate(x.float(), scale_factor=2.0, mode="nearest") if up else x.float()
        if pad:
            y = F.conv2d(F.pad(xx, (1, 1, 1, 1), mode="reflect" if pad == 1 else "replicate"), w.half().float(), b.float())
        else:
            y = F.conv2d(xx, w.half().float(), b.float(), padding=1)
        y = F.leaky_relu(y, 0.2) if act == 1 else F.relu(y) if act == 2 else y
        if use_r1:
            y = y * 0.2 + r1.float()
        if use_r2:
            y = y * 0.2 + r2.float()
        err = (got - y).abs().max().item()
        assert err < 4e-3, (case, N, Cc, K, H, W, act, up, pad, use_r1, use_r2, off, err)


def test_conv_epilogues_and_slab_offsets(dev):
    from innfer_amd import synth
    N, Cc, K, H, W = 1, 192, 64, 20, 36
    x = torch.from_numpy(synth.uniform((N, Cc, H, W), 4, -1, 1)).half()
    w = torch.from_numpy(synth.uniform((K, Cc, 3, 3), 5, -1, 1)) / np.sqrt(9 * Cc)
    b = torch.from_numpy(synth.uniform((K,), 6, -1, 1))
    r1 = torch.from_numpy(synth.uniform((N, K, H, W), 7, -1, 1)).half()
    r2 = torch.from_numpy(synth.uniform((N, K, H, W), 8, -1, 1)).half()
    got, raw = _run_conv(dev, x, w, b, K, act=0, res1=r1, s1=0.2, res2=r2, s2=0.2, out_channels=192, out_off=64)
    ref = _ref_conv(x, w, b, act=0, res1=r1, s1=0.2, res2=r2, s2=0.2)
    assert (got - ref).abs().max().item() < 4e-3
    # channel groups outside [64,128) of the output slab are untouched (dense concat = group offset)
    assert torch.all(raw[:2] == -3.0) and torch.all(raw[4:] == -3.0)
    got, _ = _run_conv(dev, x, w, b, K, act=2)
    assert (got - _ref_conv(x, w, b, act=2)).abs().max().item() < 4e-3


@pytest.mark.parametrize("N,H,W,with_res2", [(1, 37, 70, False), (1, 16, 32, True), (4, 40, 40, True), (3, 200, 200, False), (1, 1, 1, False)])
def test_conv_rdb_residual_aliasing_the_input_slab(dev, N, H, W, with_res2):
    """RRDBNet_arch.py:165 `x5 * 0.2 + x` exactly as the trunk issues it: residual 1 is channels 0..63 of the conv's OWN input slab (the pointer
    aliases the input) -- plain lattice, image canvas (N > 1) and the RRDB's second residual; same result as with the residual in its own buffer."""
    from innfer_amd import synth
    Cc, K = 192, 64
    x = torch.from_numpy(synth.uniform((N, Cc, H, W), 14, -1, 1)).half()
    w = torch.from_numpy(synth.uniform((K, Cc, 3, 3), 15, -1, 1)) / np.sqrt(9 * Cc)
    b = torch.from_numpy(synth.uniform((K,), 16, -1, 1))
    r2 = torch.from_numpy(synth.uniform((N, K, H, W), 17, -1, 1)).half() if with_res2 else None
    got, _ = _run_conv(dev, x, w, b, K, act=0, s1=0.2, res2=r2, s2=0.2, res1_is_input=True)
    ref = _ref_conv(x, w, b, act=0, res1=x[:, :K], s1=0.2, res2=r2, s2=0.2)
    assert (got - ref).abs().max().item() < 4e-3
    got2, _ = _run_conv(dev, x, w, b, K, act=0, res1=x[:, :K].contiguous(), s1=0.2, res2=r2, s2=0.2)
    assert torch.equal(got, got2)


@pytest.mark.parametrize("N,Cc,H,W,with_res2,rows", [(1, 192, 37, 70, False, None), (1, 192, 16, 32, True, None), (4, 192, 40, 40, True, None), (3, 192, 200, 200, False, None),
                                                     (1, 192, 1, 1, True, None), (1, 96, 33, 65, False, None), (2, 128, 17, 31, True, None), (1, 192, 64, 40, True, (16, 48))])
def test_conv_rdb_residual_from_lds(dev, N, Cc, H, W, with_res2, rows):
    """The same launch with the residual taken from the conv's own staged LDS tiles (innfer_conv_args.res1_from_input, conv3x3_pc<.., TMF | 0x40000>;
    innfer_net_set_residual_lds, the networks' default): chunk order 2, 3, .., 0, 1 and x / s1 added to the fp32 accumulators instead of fma(acc, s1, x) in
    the epilogue -- against F.conv2d (<= 4e-3) and against the epilogue-load form to the last fp16 rounding; plain lattice, image canvas, one and two residuals,
    a row range, 96 .. 192 input channels."""
    from innfer_amd import synth
    K = 64
    x = torch.from_numpy(synth.uniform((N, Cc, H, W), 14, -1, 1)).half()
    w = torch.from_numpy(synth.uniform((K, Cc, 3, 3), 15, -1, 1)) / np.sqrt(9 * Cc)
    b = torch.from_numpy(synth.uniform((K,), 16, -1, 1))
    r2 = torch.from_numpy(synth.uniform((N, K, H, W), 17, -1, 1)).half() if with_res2 else None
    got, raw = _run_conv(dev, x, w, b, K, act=0, s1=0.2, res2=r2, s2=0.2, res1_is_input=True, res1_from_lds=True, rows=rows)
    base, raw0 = _run_conv(dev, x, w, b, K, act=0, s1=0.2, res2=r2, s2=0.2, res1_is_input=True, rows=rows)
    ref = _ref_conv(x, w, b, act=0, res1=x[:, :K], s1=0.2, res2=r2, s2=0.2)
    sl = slice(*rows) if rows else slice(None)
    assert (got[:, :, sl] - ref[:, :, sl]).abs().max().item() < 4e-3
    _assert_same_to_the_last_rounding(got[:, :, sl], base[:, :, sl], "residual from LDS vs epilogue load")
    if rows:                                    # rows outside the range keep the buffer's fill value in both forms
        assert torch.equal(raw[:, :, :rows[0]], raw0[:, :, :rows[0]]) and torch.equal(raw[:, :, rows[1]:], raw0[:, :, rows[1]:])


def test_conv_pixel_attention_gate_epilogue(dev):
    """act 4 / 5: res1 * sigmoid(conv + bias) [+ LeakyReLU] -- PAN's PA / PAConv gate (PAN_arch.py) as a conv epilogue."""
    from innfer_amd import synth
    N, Cc, K, H, W = 2, 32, 32, 19, 41
    x = torch.from_numpy(synth.uniform((N, Cc, H, W), 31, -1, 1)).half()
    w = torch.from_numpy(synth.uniform((K, Cc, 3, 3), 32, -1, 1)) / np.sqrt(9 * Cc)
    b = torch.from_numpy(synth.uniform((K,), 33, -1, 1))
    v = torch.from_numpy(synth.uniform((N, K, H, W), 34, -2, 2)).half()
    gate = v.float() * torch.sigmoid(F.conv2d(x.float(), w.half().float(), b.float(), padding=1))
    got, _ = _run_conv(dev, x, w, b, K, act=5, res1=v)
    assert (got - gate).abs().max().item() < 4e-3
    got, _ = _run_conv(dev, x, w, b, K, act=4, res1=v)
    assert (got - F.leaky_relu(gate, 0.2)).abs().max().item() < 4e-3


@pytest.mark.parametrize("N,Cc,K,H,W", [(1, 64, 64, 25, 33), (2, 32, 32, 2, 2), (1, 64, 32, 48, 64), (1, 32, 64, 24, 32)])
def test_conv_reflection_padding(dev, N, Cc, K, H, W):
    """nn.ReflectionPad2d(1) + conv (ResNet_arch.py:103-140) in the halo-tile loader: ragged, tile-aligned and minimal sizes."""
    from innfer_amd import synth
    x = torch.from_numpy(synth.uniform((N, Cc, H, W), 61, -1, 1)).half()
    w = torch.from_numpy(synth.uniform((K, Cc, 3, 3), 62, -1, 1)) / np.sqrt(9 * Cc)
    b = torch.from_numpy(synth.uniform((K,), 63, -1, 1))
    got, _ = _run_conv(dev, x, w, b, K, act=0, reflect=True)
    ref = F.conv2d(F.pad(x.float(), (1, 1, 1, 1), mode="reflect"), w.half().float(), b.float())
    assert (got - ref).abs().max().item() < 4e-3


@pytest.mark.parametrize("d", [2, 3, 4, 5, 6, 7, 8])
def test_conv_dilated_polyphase(dev, d):
    """Dilated 3x3 conv, zero padding d (PPON_arch.py:83-91), as ordinary 3x3 convs on the d*d polyphase components of the image:
    ragged sizes (the components have different extents), a batch, sizes below the dilation."""
    from innfer_amd import synth
    for (N, H, W) in ((2, 37, 53), (1, 200, 200), (1, 5, 3)):
        x = torch.from_numpy(synth.uniform((N, 64, H, W), 71 + d, -1, 1)).half()
        w = torch.from_numpy(synth.uniform((32, 64, 3, 3), 72, -1, 1)) / np.sqrt(9 * 64)
        b = torch.from_numpy(synth.uniform((32,), 73, -1, 1))
        got, _ = _run_conv(dev, x, w, b, 32, act=0, dilation=d)
        ref = F.conv2d(x.float(), w.half().float(), b.float(), padding=d, dilation=d)
        assert (got - ref).abs().max().item() < 4e-3, (d, N, H, W)


def test_conv_dilation_groups_one_launch(dev):
    """PPON's eight dilated convs (64 -> 32 each, rates 1..8) as ONE launch: output channel group g = the conv of dilation g+1 with its
    own panel and tile grid.  Against eight F.conv2d calls on a ragged batch."""
    import innfer_amd.lib as L
    from innfer_amd import synth
    N, H, W, G = 2, 45, 70, 8
    x = torch.from_numpy(synth.uniform((N, 64, H, W), 81, -1, 1)).half()
    ws = [torch.from_numpy(synth.uniform((32, 64, 3, 3), 82 + g, -1, 1)) / 24 for g in range(G)]
    b = torch.from_numpy(synth.uniform((32 * G,), 90, -1, 1))
    g_in = N * H * W * 32
    slab = torch.empty((2, N, H, W, 32), dtype=torch.float16, device=dev)
    L.check(L.lib.innfer_nchw_to_slab(x.to(dev).contiguous().data_ptr(), L.F16, slab.data_ptr(), g_in, 0, N, 64, H, W, None))
    pb = L.lib.innfer_conv3x3_packed_bytes(32, 64)
    packed = np.zeros(G * pb, dtype=np.uint8)
    for g in range(G):
        wc = np.ascontiguousarray(ws[g].numpy())
        L.check(L.lib.innfer_pack_conv3x3(wc.ctypes.data, 32, 64, packed[g * pb:].ctypes.data))
    d_packed, d_bias = torch.from_numpy(packed).to(dev), b.float().to(dev)
    out = torch.full((G, N, H, W, 32), -3.0, dtype=torch.float16, device=dev)
    a = L.ConvArgs()
    a.d_in, a.in_group_stride, a.C = slab.data_ptr(), g_in, 64
    a.d_packed, a.d_bias = d_packed.data_ptr(), d_bias.data_ptr()
    a.d_out, a.out_group_stride, a.out_ch_off, a.K = out.data_ptr(), g_in, 0, 32 * G
    a.N, a.H, a.W, a.act, a.dilation_groups = N, H, W, 0, G
    L.check(L.lib.innfer_conv3x3_f16(C.byref(a), None))
    res = torch.empty((N, 32 * G, H, W), dtype=torch.float32, device=dev)
    L.check(L.lib.innfer_slab_to_nchw(out.data_ptr(), g_in, 0, res.data_ptr(), L.F32, N, 32 * G, H, W, None))
    torch.cuda.synchronize()
    ref = torch.cat([F.conv2d(x.float(), ws[g].half().float(), b[32 * g:32 * g + 32].float(), padding=g + 1, dilation=g + 1) for g in range(G)], 1)
    assert (res.cpu() - ref).abs().max().item() < 4e-3


def _run_shuffle_conv(dev, x, w, b, act, phase_major=None):
    """conv (K = w.shape[0], K % 64 == 0) with nn.PixelShuffle(2) folded into the store: returns the [N, K/4, 2H, 2W] result (fp32, cpu).
    phase_major: True = the phase-major plane-order panels of innfer_pack_conv3x3_shuffle2 (plane_rows 2: the producer / consumer kernel's store, K % 256 == 0),
    False = the plain panels (the two-workgroup kernel); None = BOTH where K % 256 == 0, and the two results must be the same bits."""
    import innfer_amd.lib as L
    N, Cc, H, W = x.shape
    K = w.shape[0]
    if phase_major is None:
        r0 = _run_shuffle_conv(dev, x, w, b, act, False)
        if K % 256 == 0:
            assert torch.equal(_run_shuffle_conv(dev, x, w, b, act, True), r0), "phase-major PixelShuffle store != the plain one"
        return r0
    g_in, g_out = N * H * W * 32, N * 4 * H * W * 32
    slab = torch.zeros((Cc // 32, N, H, W, 32), dtype=torch.float16, device=dev)
    L.check(L.lib.innfer_nchw_to_slab(x.to(dev).contiguous().data_ptr(), L.F16, slab.data_ptr(), g_in, 0, N, Cc, H, W, None))
    packed = np.zeros(L.lib.innfer_conv3x3_packed_bytes(K, Cc), dtype=np.uint8)
    wc = np.ascontiguousarray(w.numpy())
    bias = np.ascontiguousarray(b.float().numpy())
    if phase_major:
        bias_pm = np.zeros(K, dtype=np.float32)
        L.check(L.lib.innfer_pack_conv3x3_shuffle2(wc.ctypes.data, bias.ctypes.data, K, Cc, packed.ctypes.data, bias_pm.ctypes.data))
        assert np.array_equal(bias_pm.reshape(4, K // 4), bias.reshape(K // 4, 4).T)
        bias = bias_pm
    else:
        L.check(L.lib.innfer_pack_conv3x3(wc.ctypes.data, K, Cc, packed.ctypes.data))
    d_packed, d_bias = torch.from_numpy(packed).to(dev), torch.from_numpy(bias).to(dev)
    out = torch.full((max(K // 4, 32) // 32, N, 2 * H, 2 * W, 32), -3.0, dtype=torch.float16, device=dev)
    a = L.ConvArgs()
    a.d_in, a.in_group_stride, a.C = slab.data_ptr(), g_in, Cc
    a.d_packed, a.d_bias = d_packed.data_ptr(), d_bias.data_ptr()
    a.d_out, a.out_group_stride, a.out_ch_off, a.K = out.data_ptr(), g_out, 0, K
    a.N, a.H, a.W, a.act, a.pixel_shuffle2 = N, H, W, act, 1
    a.plane_rows = 2 if phase_major else 0
    L.check(L.lib.innfer_conv3x3_f16(C.byref(a), None))
    res = torch.empty((N, K // 4, 2 * H, 2 * W), dtype=torch.float32, device=dev)
    L.check(L.lib.innfer_slab_to_nchw(out.data_ptr(), g_out, 0, res.data_ptr(), L.F32, N, K // 4, 2 * H, 2 * W, None))
    torch.cuda.synchronize()
    return res.cpu()


def test_pixelshuffle_store_phase_major_vs_torch(dev):
    """The PixelShuffle(2) store of the producer / consumer kernel (innfer_pack_conv3x3_shuffle2, VERDICT r4 weak 6: SRResNet's up stages ran on the round-1 kernel) on
    real-valued data: == the plain-panel form bit for bit (same MFMAs, same order per value) and within 4e-3 of F.pixel_shuffle(act(F.conv2d)); whole tiles, ragged
    frames, a batch, 200 x 200 chop tiles."""
    from innfer_amd import synth
    for i, (N, H, W, act) in enumerate([(1, 16, 32, 2), (1, 37, 70, 2), (2, 33, 50, 1), (1, 200, 200, 2), (3, 20, 24, 0)]):
        x = torch.from_numpy(synth.uniform((N, 64, H, W), 60 + i, -1, 1)).half()
        w = torch.from_numpy(synth.uniform((256, 64, 3, 3), 70 + i, -1, 1)) / np.sqrt(9 * 64)
        b = torch.from_numpy(synth.uniform((256,), 80 + i, -1, 1))
        y = _run_shuffle_conv(dev, x, w, b, act)          # both forms, bit-compared
        ref = F.conv2d(x.float(), w.half().float(), b, padding=1)
        ref = F.leaky_relu(ref, 0.2) if act == 1 else (F.relu(ref) if act == 2 else ref)
        assert (y - F.pixel_shuffle(ref, 2)).abs().max().item() < 4e-3, (N, H, W, act)


def test_pixelshuffle_store_is_bit_exact(dev, golden):
    """nn.PixelShuffle(2) folded into the conv's store (pixelshuffle_block, block.py:333-346) is a pure index map and must be BIT-EXACT:
    (a) the reference's known answer (golden G6: ps_in = arange [1,8,3,5] -> ps_out [1,2,6,10]) through the HIP store, with a conv whose
        centre tap copies input channel k to conv channel k;
    (b) all 256 conv channels at ragged sizes and batches with small-integer inputs and weights in {-1,0,1}: every product and every
        partial sum is an integer below 2048, so the fp32 MFMA accumulation, the fp16 rounding and torch's fp32 conv are all exact and
        the HIP result must EQUAL F.pixel_shuffle(act(F.conv2d(...))) whatever the summation order."""
    g = golden("g6_srgan")
    ps_in, ps_out = torch.from_numpy(g["ps_in"]), torch.from_numpy(g["ps_out"])
    x = torch.zeros((1, 32, 3, 5))
    x[:, :8] = ps_in
    w = torch.zeros((64, 32, 3, 3))
    for k in range(8):
        w[k, k, 1, 1] = 1.0
    y = _run_shuffle_conv(dev, x.half(), w, torch.zeros(64), act=0)
    assert torch.equal(y[:, :2], ps_out) and not y[:, 2:].any()
    for (N, Cc, K, H, W, act, seed) in [(1, 64, 256, 24, 32, 2, 0), (2, 64, 256, 25, 33, 2, 1), (1, 32, 64, 7, 50, 0, 2), (3, 64, 128, 17, 16, 1, 3)]:
        rng = np.random.default_rng(seed)
        x = torch.from_numpy(rng.integers(-3, 4, (N, Cc, H, W)).astype(np.float32))
        w = torch.from_numpy(rng.integers(-1, 2, (K, Cc, 3, 3)).astype(np.float32))
        b = torch.from_numpy(rng.integers(-5, 6, (K,)).astype(np.float32))
        ref = F.conv2d(x, w, b, padding=1)
        assert ref.abs().max().item() < 2048
        if act == 1:
            ref = torch.where(ref > 0, ref, (ref * 0.2).half().float())      # the only inexact step: one fp16 rounding of 0.2*v, same on both sides
        elif act == 2:
            ref = F.relu(ref)
        ref = F.pixel_shuffle(ref, 2)
        y = _run_shuffle_conv(dev, x.half(), w, b, act)
        if act == 1:
            assert (y - ref).abs().max().item() <= 0.5 and torch.equal(y[ref > 0], ref[ref > 0])
        else:
            assert torch.equal(y, ref), (N, Cc, K, H, W)


def test_conv_nearest_upsample_fused(dev):
    from innfer_amd import synth
    N, Cc, K, Hs, Ws = 1, 64, 64, 13, 21
    x = torch.from_numpy(synth.uniform((N, Cc, Hs, Ws), 9, -1, 1)).half()
    w = torch.from_numpy(synth.uniform((K, Cc, 3, 3), 10, -1, 1)) / np.sqrt(9 * Cc)
    b = torch.from_numpy(synth.uniform((K,), 11, -1, 1))
    got, _ = _run_conv(dev, x, w, b, K, act=1, up=True)
    assert (got - _ref_conv(x, w, b, act=1, up=True)).abs().max().item() < 4e-3


def test_conv_row_range(dev):
    from innfer_amd import synth
    N, Cc, K, H, W = 1, 64, 32, 50, 40
    x = torch.from_numpy(synth.uniform((N, Cc, H, W), 12, -1, 1)).half()
    w = torch.from_numpy(synth.uniform((K, Cc, 3, 3), 13, -1, 1)) / np.sqrt(9 * Cc)
    b = torch.zeros(K)
    full, _ = _run_conv(dev, x, w, b, K)
    part, raw = _run_conv(dev, x, w, b, K, rows=(7, 29))
    assert torch.equal(part[:, :, 7:29], full[:, :, 7:29])
    assert torch.all(raw[:, :, :7] == -3.0) and torch.all(raw[:, :, 29:] == -3.0)


def test_conv_error_codes(dev):
    import innfer_amd.lib as L
    a = L.ConvArgs()
    assert L.lib.innfer_conv3x3_f16(C.byref(a), None) == L.ERR_INVALID
    with pytest.raises(ValueError):
        L.check(L.lib.innfer_conv3x3_f16(C.byref(a), None))
    assert L.lib.innfer_conv3x3_packed_bytes(32, 48) == 0


# -------------------------------------------------------------------- networks
def _rrdb(dev, nb, scale, seed=0):
    from innfer_amd import synth
    from innfer_amd.architectures.RRDBNet_arch import RRDBNet
    sd = _sd(synth.rrdbnet_shapes(nb=nb, scale=scale), seed)
    net = RRDBNet(3, 3, 64, nb, upscale=scale)
    net.load_state_dict(sd, strict=True)
    return net.to(dev).eval(), sd


def _codes_within_one(dev, y, ref):
    """fraction of the final uint8 codes (tensor2np: clip, *255, round half to even -- the HIP post kernel) within +-1 of the
    codes of the fp32 reference output.  y, ref: [1,C,H,W] float arrays."""
    from innfer_amd.utils import utils as U
    a = U.tensor2np(torch.as_tensor(np.ascontiguousarray(y), dtype=torch.float32).to(dev)).astype(np.int32)
    b = U.tensor2np(torch.as_tensor(np.ascontiguousarray(ref), dtype=torch.float32).to(dev)).astype(np.int32)
    return float((np.abs(a - b) <= 1).mean())


def test_rrdbnet23_x4_golden(dev, golden):
    from innfer_amd import synth
    g3, g11 = golden("g3_rrdbnet23_x4"), golden("g11_rrdbnet23_x4_fp16")
    net, _ = _rrdb(dev, 23, 4)
    for tag, shape, seed in (("out_32", (1, 3, 32, 32), 3), ("out_16", (1, 3, 16, 16), 4)):
        x = torch.from_numpy(synth.uniform(shape, seed)).to(dev)
        y = net(x.half()).float().cpu().numpy()
        assert np.isfinite(y).all()
        e32 = np.abs(y - g3[tag]).max()
        e16 = np.abs(y - g11[tag]).max()
        assert e32 < 1e-2, f"{tag}: vs fp32 reference {e32}"
        assert e16 < 4e-3, f"{tag}: vs the reference's fp16 mode {e16}"
        # and at least as close to the fp32 truth as the reference's own fp16 mode is (x1.5 slack)
        assert e32 <= 1.5 * np.abs(g11[tag] - g3[tag]).max() + 1e-4
        assert _codes_within_one(dev, y, g3[tag]) >= 0.99          # >= 99 % of the uint8 pixels within +-1 code
        y32 = net(x).float().cpu().numpy()          # fp32 I/O, fp16 internals
        assert np.abs(y32 - g3[tag]).max() < 1e-2


def test_rrdbnet_scales_golden(dev, golden):
    from innfer_amd import synth
    g = golden("g5_scales")
    x = torch.from_numpy(synth.uniform((1, 3, 16, 16), 5)).to(dev).half()
    for scale in (1, 2, 3, 8):
        net, _ = _rrdb(dev, 1, scale)
        y = net(x).float().cpu().numpy()
        assert y.shape == g[f"out_x{scale}"].shape
        assert np.abs(y - g[f"out_x{scale}"]).max() < 5e-3, scale
    from innfer_amd.architectures.RRDBNet_arch import RRDBNet
    from innfer_amd import synth as _s
    for fa in ("tanh", "sigmoid"):                       # finalact: activation in the last conv's epilogue
        net = RRDBNet(3, 3, 64, 1, upscale=4, finalact=fa)
        net.load_state_dict(_sd(_s.rrdbnet_shapes(nb=1, scale=4)), strict=True)
        y = net.to(dev).eval()(x).float().cpu().numpy()
        assert np.abs(y - g[f"out_x4_{fa}"]).max() < 5e-3, fa


def test_rrdbnet_constructor_variants_golden(dev, golden):
    """RRDBNet(nr=.., act_type='relu', mode='NAC', upsample_mode='pixelshuffle') (RRDBNet_arch.py:16-48) against the reference's outputs (G18)."""
    from innfer_amd import synth
    from innfer_amd.architectures.RRDBNet_arch import RRDBNet
    from test_oracle_golden import G18_CASES
    g = golden("g18_rrdb_variants")
    for i, (tag, (kw, shape, xseed)) in enumerate(G18_CASES.items()):
        ctor = dict(upscale=kw["scale"], nr=kw.get("nr", 3), upsample_mode=kw.get("upsample_mode", "upconv"), act_type=kw.get("act_type", "leakyrelu"),
                    mode="NAC" if tag == "nr2_relu_nac" else "CNA")
        net = RRDBNet(3, 3, 64, kw["nb"], **ctor)
        assert sorted(net.state_dict()) == list(g[tag + "_keys"])
        net.load_state_dict(_sd(synth.rrdbnet_shapes(nb=kw["nb"], scale=kw["scale"], nr=ctor["nr"], upsample_mode=ctor["upsample_mode"]), 180 + i), strict=True)
        x = torch.from_numpy(synth.uniform(shape, xseed)).to(dev).half()
        y = net.to(dev).eval()(x).float().cpu().numpy()
        assert y.shape == g[tag].shape and np.abs(y - g[tag]).max() < 5e-3, tag
    with pytest.raises(NotImplementedError):
        RRDBNet(3, 3, 64, 1, upsample_mode="deconv")
    # norm_type='batch': the eval-mode BatchNorm2d layers are folded into the convs when the weights are uploaded
    shapes = synth.rrdbnet_shapes(nb=2, scale=2, norm=True)
    net = RRDBNet(3, 3, 64, 2, upscale=2, norm_type="batch")
    assert sorted(net.state_dict()) == list(g["batchnorm_keys"])
    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in synth.fill_running_stats(synth.fill_state_dict(shapes, 184), 184).items()}
    net.load_state_dict(sd, strict=True)
    net = net.to(dev).eval()
    x = torch.from_numpy(synth.uniform((1, 3, 16, 16), 194)).to(dev).half()
    assert np.abs(net(x).float().cpu().numpy() - g["batchnorm"]).max() < 5e-3
    net.train()
    with pytest.raises(NotImplementedError):
        net(x)                                    # batch statistics: not what the engine folds
    with pytest.raises(NotImplementedError):
        RRDBNet(3, 3, 64, 1, norm_type="instance")


def test_srresnet_variants_and_outm_golden(dev, golden):
    """SRResNet(act_type='leakyrelu', res_scale, upsample_mode='upconv' / 'pixelshuffle') and forward(x, outm=...) of SRResNet / RRDBNet -- the
    range limiter runs in the last conv's epilogue -- against the reference (golden G18)."""
    from innfer_amd import synth
    from innfer_amd.architectures.RRDBNet_arch import RRDBNet
    from innfer_amd.architectures.SRResNet_arch import SRResNet
    from test_oracle_golden import G18_SR, OUTMS
    g = golden("g18_rrdb_variants")
    for j, (tag, kw) in enumerate(G18_SR.items()):
        net = SRResNet(3, 3, 64, 2, upscale=kw["scale"], norm_type=None, act_type=kw["act_type"], mode="CNA", res_scale=kw["res_scale"],
                       upsample_mode=kw["upsample_mode"])
        assert sorted(net.state_dict()) == list(g[tag + "_keys"])
        net.load_state_dict(_sd(synth.srresnet_shapes(nb=2, scale=kw["scale"], upsample_mode=kw["upsample_mode"]), 186 + j), strict=True)
        net = net.to(dev).eval()
        x = torch.from_numpy(synth.uniform((1, 3, 14, 18), 196 + j)).to(dev).half()
        for om in OUTMS:
            y = (net(x, outm=om) if om else net(x)).float().cpu().numpy()
            assert np.abs(y - g[tag + ("_" + om if om else "")]).max() < 5e-3, (tag, om)
        assert torch.equal(net(x, outm="no such limiter"), net(x))              # anything else means none, as in the reference
    net, _ = _rrdb(dev, 1, 2)
    x = torch.from_numpy(synth.uniform((1, 3, 12, 12), 198)).to(dev).half()
    for om in ("scaltanh", "clamp"):
        assert np.abs(net(x, outm=om).float().cpu().numpy() - g["rrdb_" + om]).max() < 5e-3, om
    plain = net(x)
    assert not torch.equal(plain, net(x, outm="clamp")) and torch.equal(net(x), plain)          # outm does not stick to the module


def test_srresnet_norm_and_mode_golden(dev, golden):
    """SRResNet(norm_type='batch', mode='NAC') -- the class's own defaults (SRResNet_arch.py:16-17) -- and the other norm / mode combinations in eval
    mode, upscale=3 with 'upconv': BatchNorm behind a conv is folded at upload, norm -> act in front of a conv whose input is the residual stream runs
    as the engine's input map (innfer_net_set_conv_input_map).  Against the reference (golden G26); parameter names in state-dict order."""
    from innfer_amd.architectures.SRResNet_arch import SRResNet
    from test_oracle_golden import G26_SR, g26_case
    g = golden("g26_srresnet_modes")
    for j, tag in enumerate(G26_SR):
        c, shapes, sd, x = g26_case(j, tag)
        net = SRResNet(3, 3, 64, 2, upscale=c["scale"], norm_type="batch" if c["norm"] else None, act_type=c["act_type"], mode=c["mode"],
                       res_scale=c["res_scale"], upsample_mode="upconv")
        assert list(net.state_dict()) == list(g[tag + "_keys"]), tag
        net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
        net = net.to(dev).eval()
        xt = torch.from_numpy(x).to(dev)
        y = net(xt.half()).float().cpu().numpy()
        assert y.shape == g[tag].shape, tag
        assert np.abs(y - g[tag]).max() < 1.5e-3, (tag, float(np.abs(y - g[tag]).max()))
        y32 = net(xt).cpu().numpy()                      # fp32 at the boundary, fp16 slabs inside
        assert np.abs(y32 - g[tag]).max() < 1.5e-3, tag
        if c["norm"]:
            with pytest.raises(NotImplementedError):
                net.train()(xt)
            net.eval()
    from innfer_amd import synth
    from innfer_amd.architectures.RRDBNet_arch import RRDBNet
    for j, mode in enumerate(("NAC", "CNAC")):              # RRDBNet(norm_type='batch', mode): LR_conv = norm, conv under 'NAC' (the input map), conv, norm else
        net = RRDBNet(3, 3, 64, 2, upscale=2, norm_type="batch", mode=mode)
        assert list(net.state_dict()) == list(g[f"rrdb_bn_{mode}_keys"])
        sd = synth.fill_running_stats(synth.fill_state_dict(synth.rrdbnet_shapes(nb=2, scale=2, norm=True, mode=mode), 320 + j), 320 + j)
        net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
        net = net.to(dev).eval()
        y = net(torch.from_numpy(synth.uniform((1, 3, 16, 16), 330 + j)).to(dev).half()).float().cpu().numpy()
        assert np.abs(y - g["rrdb_bn_" + mode]).max() < 5e-3, (mode, float(np.abs(y - g["rrdb_bn_" + mode]).max()))
    # PixelShuffle(3), PixelShuffle(2) on 32 features: conv to a slab, one gather pass (slab_pixel_shuffle)
    from test_oracle_golden import G26_PS
    nets = {"ps3_sr": lambda: SRResNet(3, 3, 64, 2, upscale=3, norm_type=None, mode="CNA", upsample_mode="pixelshuffle"),
            "ps2_sr_nf32": lambda: SRResNet(3, 3, 32, 2, upscale=4, norm_type=None, mode="CNA", upsample_mode="pixelshuffle"),
            "ps3_rrdb": lambda: RRDBNet(3, 3, 64, 1, upscale=3, upsample_mode="pixelshuffle")}
    for tag, (shapes, seed, _) in G26_PS.items():
        net = nets[tag]()
        assert list(net.state_dict()) == list(g[tag + "_keys"]), tag
        net.load_state_dict(_sd(shapes(), seed), strict=True)
        net = net.to(dev).eval()
        y = net(torch.from_numpy(synth.uniform((1, 3, 10, 12), seed + 10)).to(dev).half()).float().cpu().numpy()
        assert y.shape == g[tag].shape and np.abs(y - g[tag]).max() < 5e-3, (tag, float(np.abs(y - g[tag]).max()))
    with pytest.raises(NotImplementedError):
        SRResNet(3, 3, 64, 2, norm_type="instance")
    with pytest.raises(NotImplementedError):
        SRResNet(3, 3, 32, 2, upscale=3, upsample_mode="pixelshuffle", norm_type=None, mode="CNA")          # 9 * 32 output channels: not a multiple of 64


def test_esrgan_plus_golden(dev, golden):
    """ESRGAN+ residual paths (x2 += conv1x1(x), x4 += x2) against the reference (golden G5)."""
    from innfer_amd import synth
    from innfer_amd.architectures.RRDBNet_arch import RRDBNet
    g = golden("g5_scales")
    sd = _sd(synth.rrdbnet_shapes(nb=1, scale=4, plus=True))
    net = RRDBNet(3, 3, 64, 1, upscale=4, plus=True)
    net.load_state_dict(sd, strict=True)
    net = net.to(dev).eval()
    x = torch.from_numpy(synth.uniform((1, 3, 16, 16), 5)).to(dev).half()
    y = net(x).float().cpu().numpy()
    assert np.abs(y - g["out_x4_plus"]).max() < 5e-3


def test_mrrdbnet_golden_and_same_engine(dev, golden):
    """MRRDBNet built directly: golden G16 (reference MRRDBNet, nb 2), and bit-identical to the old-arch RRDBNet holding
    the same weights under mod2normal's names (one engine, two key layouts)."""
    from innfer_amd import synth
    from innfer_amd.architectures import get_network
    from innfer_amd.utils.defaults import get_network_G_config
    g = golden("g16_mrrdb")
    sd = {k: torch.from_numpy(v) for k, v in synth.fill_state_dict(synth.mrrdbnet_shapes(nb=2), 61).items()}
    net = get_network(get_network_G_config({"type": "mrrdb_net", "nb": 2}, 4))
    net.load_state_dict(sd, strict=True)
    net = net.to(dev).eval()
    x = torch.from_numpy(synth.uniform((2, 3, 16, 20), 62)).to(dev)
    y = net(x)
    err = np.abs(y.cpu().numpy() - g["out"])
    assert err.max() < 5e-3, err.max()                                   # fp32 in/out, fp16 storage inside; golden is fp32
    yh = net(x.half())
    assert np.abs(yh.float().cpu().numpy() - g["out"]).max() < 5e-3
    from innfer_amd.architectures.keys import mrrdb_key_of
    old = get_network(get_network_G_config({"type": "esrgan", "nb": 2}, 4))
    old.load_state_dict({k: sd[mrrdb_key_of(k.rsplit(".", 1)[0], 2) + "." + k.rsplit(".", 1)[1]] for k in old.state_dict()}, strict=True)
    assert torch.equal(old.to(dev).eval()(x.half()), yh)


def test_rrdbnet_batch_and_ragged_sizes(dev):
    import oracle
    from innfer_amd import synth
    net, sd = _rrdb(dev, 2, 4)
    x = torch.from_numpy(synth.uniform((3, 3, 37, 53), 21))
    y = net(x.to(dev).half()).float().cpu()
    with torch.no_grad():
        ref = oracle.rrdbnet_forward(sd, x, nb=2, scale=4)
    assert (y - ref).abs().max().item() < 1e-2
    y0 = net(x[1:2].to(dev).half()).float().cpu()
    assert torch.equal(y0, y[1:2])                 # batching does not change a tile's result


def test_rrdbnet_degenerate_sizes(dev):
    """Edge sizes: a single pixel, one-pixel-wide rows / columns, sizes below one MFMA tile, a chop of an image smaller
    than the patch.  (An empty batch is an argument error, as nn.Conv2d's 'non-zero batch' check is in the reference.)"""
    import oracle
    from innfer_amd import synth
    net, sd = _rrdb(dev, 1, 4)
    for i, (n, h, w) in enumerate([(1, 1, 1), (2, 1, 9), (1, 7, 1), (1, 2, 2), (1, 3, 33), (1, 25, 2)]):
        x = torch.from_numpy(synth.uniform((n, 3, h, w), 70 + i))
        y = net(x.to(dev).half()).float().cpu()
        with torch.no_grad():
            ref = oracle.rrdbnet_forward(sd, x, nb=1, scale=4)
        assert y.shape == ref.shape == (n, 3, 4 * h, 4 * w)
        assert (y - ref).abs().max().item() < 5e-3, (n, h, w)
    with pytest.raises((RuntimeError, ValueError)):
        net(torch.zeros(0, 3, 8, 8, device=dev, dtype=torch.float16))


def test_forward_does_not_depend_on_workspace_contents(dev):
    """Every byte the kernels read was written by an earlier launch of the same forward:
    poisoning the workspace (NaN patterns) must not change the result."""
    from innfer_amd import synth
    net, _ = _rrdb(dev, 1, 4)
    x = torch.from_numpy(synth.uniform((2, 3, 21, 45), 23)).to(dev).half()
    y = net(x)
    assert torch.isfinite(y).all()
    net._ws.fill_(0xFF)
    y2 = net(x)
    assert torch.equal(y, y2)


def test_rrdbnet_banded_schedule_is_identical(dev):
    from innfer_amd import synth
    net, _ = _rrdb(dev, 2, 2)
    x = torch.from_numpy(synth.uniform((1, 3, 150, 70), 22)).to(dev).half()
    y = net(x)
    for rows in (16, 37, 64):
        net.band_rows = rows
        assert torch.equal(net(x), y), rows
    net.band_rows = 0


def test_srresnet_golden(dev, golden):
    from innfer_amd import synth
    from innfer_amd.architectures.SRResNet_arch import SRResNet
    g = golden("g6_srgan")
    sd = _sd(synth.srresnet_shapes(nb=16, scale=4))
    net = SRResNet(3, 3, 64, 16, upscale=4, norm_type=None, act_type='relu', mode='CNA',
                   upsample_mode='pixelshuffle')
    net.load_state_dict(sd, strict=True)
    net = net.to(dev).eval()
    x = torch.from_numpy(synth.uniform((1, 3, 24, 24), 6)).to(dev).half()
    y = net(x).float().cpu().numpy()
    assert np.abs(y - g["out_24"]).max() < 1e-2
    # finalact='tanh' (SRResNet_arch.py:41-44): the same graph with tanh after the last conv
    nt = SRResNet(3, 3, 64, 16, upscale=4, norm_type=None, act_type='relu', mode='CNA', upsample_mode='pixelshuffle', finalact='tanh')
    nt.load_state_dict(sd, strict=True)
    yt = nt.to(dev).eval()(x).float().cpu().numpy()
    assert np.abs(yt - np.tanh(g["out_24"])).max() < 1e-2


def test_srresnet_chop_batch_beyond_the_pixelshuffle_store_bound(dev):
    """the phase-major PixelShuffle(2) store of the producer / consumer kernel is bounded at 2 GiB per output group (N * H * W * 256 bytes); the
    engine's own default chop batches (parallel.engine_tile_cap: up to 272 tiles of 200 x 200 for SRResNet = 10.9 M pixels, 2.8 GB at the first stage) exceed it and
    the forward raised.  Such launches take the two-workgroup kernel (64-bit indices).  220 tiles (2.25 GB at stage 1, 9 GB at stage 2): the first / a middle / the
    last tile == the engine's batch-1 forward of that tile bit for bit (tiles are independent; both PixelShuffle stores compute the same bits), last tile vs oracle."""
    import oracle
    from innfer_amd import synth
    from innfer_amd.architectures.SRResNet_arch import SRResNet
    sd = _sd(synth.srresnet_shapes(nb=16, scale=4))
    net = SRResNet(3, 3, 64, 16, upscale=4, norm_type=None, act_type='relu', mode='CNA', upsample_mode='pixelshuffle')
    net.load_state_dict(sd, strict=True)
    net = net.to(dev).eval()
    n = 220
    assert n * 200 * 200 * 256 >= 2 ** 31 - 1
    tiles = torch.from_numpy(synth.uniform((n, 3, 200, 200), 94)).half()
    y = net(tiles.to(dev))
    assert tuple(y.shape) == (n, 3, 800, 800)
    for i in (0, 111, n - 1):
        assert torch.equal(y[i:i + 1], net(tiles[i:i + 1].to(dev))), i
    with torch.no_grad():
        ref = oracle.srresnet_forward(sd, tiles[n - 1:n].float(), nb=16, scale=4)
    assert (y[n - 1:n].float().cpu() - ref).abs().max().item() < 1e-2
    del y
    net.release_workspace()
    torch.cuda.empty_cache()


def test_missing_weights_and_cpu_are_loud(dev):
    from innfer_amd.architectures.RRDBNet_arch import RRDBNet
    net = RRDBNet(3, 3, 64, 1, upscale=2)
    with pytest.raises(RuntimeError):
        net(torch.zeros(1, 3, 8, 8))               # CPU tensor: no fallback
    with pytest.raises(NotImplementedError):
        RRDBNet(3, 3, 64, 1, upscale=4, norm_type='instance')        # instance statistics cannot be folded into the convs: not built


def test_unet256_golden(dev, golden):
    """pix2pix UNet_256 (BASELINE config 5) with per-image train-mode BatchNorm against the reference
    (golden G7).  fp16 activations through 15 BatchNorms (down to 2x2 statistics): SURVEY 8c's 1e-2 on the
    tanh output, mean error an order of magnitude below, and no further from the fp32 truth than the reference's own fp16 mode."""
    import ast
    from innfer_amd import synth
    from innfer_amd.architectures import get_network
    from innfer_amd.utils.defaults import get_network_G_config
    g = golden("g7_unet256")
    shapes = {str(k): ast.literal_eval(str(s)) for k, s in zip(g["keys"], g["shapes"])}
    sd = _sd(shapes)
    net = get_network(get_network_G_config("p2p_256", 1))
    net.load_state_dict(sd, strict=True)
    net = net.to(dev)
    net.train()                                                     # meval=False (run.py:299-303)
    xa = torch.from_numpy(synth.uniform((1, 3, 256, 256), 7, -1.0, 1.0)).to(dev)
    ya = net(xa.half()).float().cpu().numpy()
    ref = g["out_a"].astype(np.float32)
    err = np.abs(ya - ref)
    assert np.isfinite(ya).all() and np.abs(ya).max() <= 1.0
    assert err.max() < 1e-2 and err.mean() < 1e-3, (err.max(), err.mean())          # SURVEY 8c (measured 4.3e-3 / 4.1e-4)
    assert np.abs(ya[0, :, ::4, ::4] - g["out_a_sub"]).max() < 1e-2
    # batch = independent batch-1 forwards (per-image statistics)
    xb = torch.from_numpy(synth.uniform((1, 3, 256, 256), 8, -1.0, 1.0)).to(dev)
    yab = net(torch.cat([xa, xb], 0).half()).float().cpu().numpy()
    assert np.array_equal(yab[0:1], ya)
    assert np.array_equal(yab[1:2], net(xb.half()).float().cpu().numpy())
    # What fp16 costs on THIS network: the reference's own fp16 mode (net.half(), run.py:383, on the CPU: golden G17) is 6.9e-3 max /
    # 6.7e-4 mean away from its fp32 output.  The HIP path (fp16 activations, fp32 accumulate and statistics; measured 4.3e-3 / 4.1e-4)
    # must be no further from the fp32 truth than that, and within twice that of the reference's fp16 output (two roundings apart).
    g17 = golden("g17_fp16_and_eval")
    ref_max, ref_mean = [float(v) for v in g17["unet_fp16_err_vs_fp32"]]
    print(f"unet256 train-mode BN: HIP vs fp32 golden max {err.max():.2e} mean {err.mean():.2e}; reference fp16 mode {ref_max:.2e} / {ref_mean:.2e}")
    assert err.max() <= 1.1 * ref_max and err.mean() <= 1.1 * ref_mean, (err.max(), err.mean(), ref_max, ref_mean)
    e16 = np.abs(ya - g17["unet_fp16_out_a"].astype(np.float32))
    print(f"unet256 train-mode BN: HIP vs the reference's fp16 mode max {e16.max():.2e} mean {e16.mean():.2e}")
    assert e16.max() <= 2.0 * ref_max + 1e-3 and e16.mean() <= 2.0 * ref_mean
    assert _codes_within_one(dev, (ya + 1) / 2, (ref + 1) / 2) >= 0.99          # SURVEY 8c on the denormalised image


def test_unet256_eval_mode_uses_running_statistics(dev, golden):
    """nn.Module.eval() is honoured: Model's default meval=True calls net.eval() (run.py:96-97), and the reference then normalises with
    the checkpoint's running statistics.  Golden G17: the reference UNet_256 in eval mode with non-trivial running_mean / running_var."""
    import ast
    from innfer_amd import synth
    from innfer_amd.architectures import get_network
    from innfer_amd.utils.defaults import get_network_G_config
    g, g17 = golden("g7_unet256"), golden("g17_fp16_and_eval")
    shapes = {str(k): ast.literal_eval(str(s)) for k, s in zip(g["keys"], g["shapes"])}
    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in synth.fill_running_stats(synth.fill_state_dict(shapes, 0), 17).items()}
    net = get_network(get_network_G_config("p2p_256", 1))
    net.load_state_dict(sd, strict=True)
    net = net.to(dev)
    xa = torch.from_numpy(synth.uniform((1, 3, 256, 256), 7, -1.0, 1.0)).to(dev)
    net.eval()
    y_ev = net(xa.half()).float().cpu().numpy()
    ref = g17["unet_eval_out_a"].astype(np.float32)
    err = np.abs(y_ev - ref)
    print(f"unet256 eval-mode BN: HIP vs fp32 golden max {err.max():.2e} mean {err.mean():.2e}")
    assert err.max() < 1e-2 and err.mean() < 1e-3, (err.max(), err.mean())
    assert np.abs(y_ev[0, :, ::4, ::4] - g17["unet_eval_out_a_sub"]).max() < 1e-2
    net.train()                                         # and back: the mode is read at every forward, not frozen at load time
    y_tr = net(xa.half()).float().cpu().numpy()
    assert np.abs(y_tr - g["out_a"].astype(np.float32)).max() < 1e-2
    assert np.abs(y_tr - y_ev).max() > 5e-2              # the two modes are different functions on this checkpoint
    net.eval()
    assert np.array_equal(net(xa.half()).float().cpu().numpy(), y_ev)
    xb = torch.from_numpy(synth.uniform((1, 3, 256, 256), 8, -1.0, 1.0)).to(dev)
    yab = net(torch.cat([xa, xb], 0).half()).float().cpu().numpy()
    assert np.array_equal(yab[0:1], y_ev)
    # running statistics are state: changing them changes the eval forward (they are re-uploaded like parameters)
    with torch.no_grad():
        for name, buf in net.named_buffers():
            if name.endswith("running_mean"):
                buf.add_(0.5)
    assert np.abs(net(xa.half()).float().cpu().numpy() - y_ev).max() > 1e-2


def test_unet_instance_norm_and_dropout_variants_golden(dev, golden):
    """UnetGenerator(norm_type='instance') in train and eval mode, (use_dropout=True) under eval() and upsample_mode='upconv' (UNet_arch.py:20-157) against the reference
    (golden G23): the reference's parameter names (biases instead of norm parameters for instance norm), outputs within the UNet tolerance."""
    from innfer_amd import synth
    from innfer_amd.architectures.UNet_arch import UnetGenerator
    from test_oracle_golden import G23_CASES, _g23_state
    g = golden("g23_unet_variants")
    for i, (tag, kw, ev) in enumerate(G23_CASES):
        net = UnetGenerator(3, 3, 5, ngf=32, **kw)
        assert list(net.state_dict()) == [str(k) for k in g[tag + "_keys"]]
        net.load_state_dict(_g23_state(g, tag, i), strict=True)
        net = net.to(dev)
        net = net.eval() if ev else net.train()
        x = torch.from_numpy(synth.uniform((1, 3, 64, 96), 240 + i, -1.0, 1.0)).to(dev)
        for xin in (x.half(),):          # (float32 tensors run the engine's fp32 mode: test_gpu_fp32_mode.py)
            err = np.abs(net(xin).float().cpu().numpy() - g[tag])
            assert err.max() < 1e-2 and err.mean() < 2e-3, (tag, err.max(), err.mean())
        if kw.get("use_dropout"):
            net.train()
            with pytest.raises(NotImplementedError):
                net(x)                               # use_dropout=True in train mode is random: refused
    with pytest.raises(NameError):
        UnetGenerator(3, 3, 5, norm_type="group")
    with pytest.raises(NotImplementedError):
        UnetGenerator(3, 3, 5, upsample_mode="pixelshuffle")   # documented by the reference, never built there either


def test_unet_variants_vs_oracle(dev):
    """Other UnetGenerator shapes through the same engine: unet_128 (7 levels) on a non-square image, and 1-channel input /
    5-channel output (the patch-slab first conv and the phase-combined last ConvTranspose are taken only for <= 4 channels)."""
    import oracle
    from innfer_amd import synth
    from innfer_amd.architectures.UNet_arch import UnetGenerator
    # (the 512 x 384 case puts four levels of either path on the halo-tile kernel -- stride-2 gather loader down, phase lattice up -- with ragged tile rows)
    for in_nc, out_nc, num_downs, h, w, seed in ((3, 3, 7, 128, 256, 40), (1, 5, 5, 64, 96, 41), (3, 3, 6, 512, 384, 42)):
        net = UnetGenerator(in_nc, out_nc, num_downs, ngf=64)
        shapes = {k: tuple(v.shape) for k, v in net.state_dict().items()}
        sd = _sd(shapes, seed)
        net.load_state_dict(sd, strict=True)
        net = net.to(dev)
        net.train()
        x = torch.from_numpy(synth.uniform((2, in_nc, h, w), seed + 1, -1.0, 1.0))
        y = net(x.to(dev).half()).float().cpu()
        with torch.no_grad():
            ref = torch.cat([oracle.unet_forward(sd, x[i:i + 1], num_downs=num_downs) for i in range(2)], 0)
        err = (y - ref).abs()
        assert y.shape == ref.shape == (2, out_nc, h, w)
        assert err.max().item() < 3e-2 and err.mean().item() < 3e-3, (in_nc, out_nc, num_downs, err.max().item(), err.mean().item())


def _run_stride2(dev, x, w, b, K, kind, k=4, act=0, plane_rows=0):
    """The stride-2 forms of the single-conv ABI: kind 'down' = Conv2d(4, 2, 1) (x [N,C,2H,2W] -> [N,K,H,W]), kind 'up' = ConvTranspose2d(k, 2, 1[, 1])
    (x [N,C,H,W] -> [N,K,2H,2W]).  Returns the NCHW fp32 result on the cpu."""
    import innfer_amd.lib as L
    N, Cc, Hi, Wi = x.shape
    Ho, Wo = (Hi // 2, Wi // 2) if kind == "down" else (2 * Hi, 2 * Wi)
    g_in, g_out = N * Hi * Wi * 32, N * Ho * Wo * 32
    slab = torch.full((Cc // 32, N, Hi, Wi, 32), 7.0, dtype=torch.float16, device=dev)
    L.check(L.lib.innfer_nchw_to_slab(x.to(dev).contiguous().data_ptr(), L.F16, slab.data_ptr(), g_in, 0, N, Cc, Hi, Wi, None))
    wc = np.ascontiguousarray(w.numpy())
    if kind == "down":
        packed = np.zeros(L.lib.innfer_conv4x4s2_packed_bytes(K, Cc), dtype=np.uint8)
        L.check(L.lib.innfer_pack_conv4x4s2(wc.ctypes.data, K, Cc, packed.ctypes.data))
        d_bias = b.float().to(dev)
    else:
        packed = np.zeros(L.lib.innfer_convt2x_packed_bytes(K, Cc), dtype=np.uint8)
        L.check(L.lib.innfer_pack_convt2x_rows(wc.ctypes.data, K, Cc, k, plane_rows, packed.ctypes.data))
        d_bias = b.float().repeat(4).to(dev)
    d_packed = torch.from_numpy(packed).to(dev)
    out = torch.full((K // 32, N, Ho, Wo, 32), -3.0, dtype=torch.float16, device=dev)
    a = L.ConvArgs()
    a.d_in, a.in_group_stride, a.C = slab.data_ptr(), g_in, Cc
    a.d_packed, a.d_bias = d_packed.data_ptr(), d_bias.data_ptr()
    a.d_out, a.out_group_stride, a.K = out.data_ptr(), g_out, K
    a.N, a.act = N, act
    if kind == "down":
        a.H, a.W, a.stride2_k4 = Ho, Wo, 1
    else:
        a.H, a.W, a.transposed2x = Hi, Wi, k
        a.plane_rows = plane_rows
    L.check(L.lib.innfer_conv3x3_f16(C.byref(a), None))
    res = torch.empty((N, K, Ho, Wo), dtype=torch.float32, device=dev)
    L.check(L.lib.innfer_slab_to_nchw(out.data_ptr(), g_out, 0, res.data_ptr(), L.F32, N, K, Ho, Wo, None))
    torch.cuda.synchronize()
    return res.cpu()


def test_stride2_conv_and_transposed_conv_vs_torch(dev):
    """Conv2d(4, 2, 1) on the stride-2 gather loader and ConvTranspose2d(4, 2, 1) / (3, 2, 1, output_padding 1) on the phase lattice (conv3x3_pc
    TMF 0x3B0 / 0x1B and their image-pair forms for grids at most 16 wide) against torch in fp32 on the fp16-rounded operands, over seeded shapes: ragged tile rows and
    columns, one- and two-tile-wide images, grids at most 16 wide (one 16-pixel segment), batches, 64 .. 192 output channels, activations.
    Tolerance: fp16 rounding of the stored result plus fp32 accumulation order (<= 4e-3 for unit-scale outputs, as for the 3x3 conv)."""
    import torch.nn.functional as F
    rng = np.random.RandomState(11)
    cases = [(1, 32, 64, 16, 32), (2, 64, 128, 24, 40), (1, 96, 64, 7, 9), (3, 32, 192, 16, 16), (1, 64, 64, 33, 65), (2, 32, 64, 5, 16), (1, 128, 128, 48, 17), (2, 64, 64, 50, 100)]
    for _ in range(6):
        cases.append((int(rng.randint(1, 4)), 32 * int(rng.randint(1, 5)), 64 * int(rng.randint(1, 4)), int(rng.randint(1, 50)), int(rng.randint(1, 70))))
    for i, (N, Cc, K, H, W) in enumerate(cases):
        act = i % 3
        post = (lambda t: t) if act == 0 else (lambda t: F.leaky_relu(t, 0.2)) if act == 1 else F.relu
        b = torch.from_numpy(rng.uniform(-0.5, 0.5, K).astype(np.float32))
        # down: output grid H x W from a 2H x 2W source
        x = torch.from_numpy(rng.uniform(-1, 1, (N, Cc, 2 * H, 2 * W)).astype(np.float32)).half()
        w = torch.from_numpy((rng.uniform(-1, 1, (K, Cc, 4, 4)) / np.sqrt(16 * Cc)).astype(np.float32)).half().float()
        ref = post(F.conv2d(x.float(), w, b, stride=2, padding=1))
        got = _run_stride2(dev, x, w, b, K, "down", act=act)
        assert got.shape == ref.shape and (got - ref).abs().max().item() < 4e-3, ("down", N, Cc, K, H, W, (got - ref).abs().max().item())
        # up: input grid H x W -> 2H x 2W
        for k in (4, 3):
            x = torch.from_numpy(rng.uniform(-1, 1, (N, Cc, H, W)).astype(np.float32)).half()
            w = torch.from_numpy((rng.uniform(-1, 1, (Cc, K, k, k)) / np.sqrt(k * k * Cc / 4)).astype(np.float32)).half().float()
            ref = post(F.conv_transpose2d(x.float(), w, b, stride=2, padding=1, output_padding=1 if k == 3 else 0))
            got = _run_stride2(dev, x, w, b, K, "up", k=k, act=act)
            assert got.shape == ref.shape and (got - ref).abs().max().item() < 4e-3, ("up", k, N, Cc, K, H, W, (got - ref).abs().max().item())
            if Cc == 64 and K == 64 and W > 16:      # plane-order panels: all four phases in one visit of a tile (conv3x3_pc UP4) -- the same MFMAs in the same order
                assert torch.equal(_run_stride2(dev, x, w, b, K, "up", k=k, act=act, plane_rows=1), got), ("up, one visit", k, N, H, W)


def test_small_grid_image_pairs_are_bit_identical_to_single_images(dev):
    """Grids at most 16 pixels wide: conv3x3_pc<.., TMF | 0x400> puts two images of the batch side by side in one tile row (LDS columns 0..17 / 18..35).
    Every output pixel must see the operands it saw in a tile of its own, in the same order: image i of an odd and of an even batch == the batch-1 run of
    image i, bit for bit, for both stride-2 forms; grids narrower than 16 and taller than one tile included."""
    rng = np.random.RandomState(23)
    for (N, Cc, K, H, W) in [(3, 64, 64, 16, 16), (4, 32, 128, 8, 8), (5, 32, 64, 40, 12), (2, 96, 64, 3, 16)]:
        b = torch.from_numpy(rng.uniform(-0.5, 0.5, K).astype(np.float32))
        x = torch.from_numpy(rng.uniform(-1, 1, (N, Cc, 2 * H, 2 * W)).astype(np.float32)).half()
        w = torch.from_numpy((rng.uniform(-1, 1, (K, Cc, 4, 4)) / np.sqrt(16 * Cc)).astype(np.float32)).half().float()
        got = _run_stride2(dev, x, w, b, K, "down", act=1)
        for i in range(N):
            one = _run_stride2(dev, x[i:i + 1], w, b, K, "down", act=1)
            assert torch.equal(got[i:i + 1], one), ("down", N, Cc, K, H, W, i)
        x = torch.from_numpy(rng.uniform(-1, 1, (N, Cc, H, W)).astype(np.float32)).half()
        w = torch.from_numpy((rng.uniform(-1, 1, (Cc, K, 4, 4)) / np.sqrt(4 * Cc)).astype(np.float32)).half().float()
        got = _run_stride2(dev, x, w, b, K, "up", k=4, act=2)
        for i in range(N):
            one = _run_stride2(dev, x[i:i + 1], w, b, K, "up", k=4, act=2)
            assert torch.equal(got[i:i + 1], one), ("up", N, Cc, K, H, W, i)


def test_pair_gate_epilogue_vs_torch(dev):
    """act 7 of the single-conv ABI: 64 rows -> 32 channels, out[8 q + r] = conv[16 q + r] * sigmoid(conv[16 q + 8 + r]) -- two independent 3x3 convs
    (value, gate) interleaved that way against torch; a batch of ragged images (the canvas form) and one image."""
    import torch.nn.functional as F
    rng = np.random.RandomState(9)
    for (N, Cc, H, W) in [(1, 32, 40, 56), (5, 64, 30, 38), (2, 32, 16, 32)]:
        x = torch.from_numpy(rng.uniform(-1, 1, (N, Cc, H, W)).astype(np.float32)).half()
        wv = torch.from_numpy((rng.uniform(-1, 1, (32, Cc, 3, 3)) / np.sqrt(9 * Cc)).astype(np.float32)).half().float()
        wg = torch.from_numpy((rng.uniform(-1, 1, (32, Cc, 3, 3)) / np.sqrt(9 * Cc) * 4).astype(np.float32)).half().float()
        bv, bg = [torch.from_numpy(rng.uniform(-0.5, 0.5, 32).astype(np.float32)) for _ in range(2)]
        w, b = torch.zeros(64, Cc, 3, 3), torch.zeros(64)
        for c in range(32):
            q, r = divmod(c, 8)
            w[16 * q + r], b[16 * q + r] = wv[c], bv[c]
            w[16 * q + 8 + r], b[16 * q + 8 + r] = wg[c], bg[c]
        ref = F.conv2d(x.float(), wv, bv, padding=1) * torch.sigmoid(F.conv2d(x.float(), wg, bg, padding=1))
        import innfer_amd.lib as L
        g = N * H * W * 32
        slab = torch.empty((Cc // 32, N, H, W, 32), dtype=torch.float16, device=dev)
        L.check(L.lib.innfer_nchw_to_slab(x.to(dev).contiguous().data_ptr(), L.F16, slab.data_ptr(), g, 0, N, Cc, H, W, None))
        packed = np.zeros(L.lib.innfer_conv3x3_packed_bytes(64, Cc), dtype=np.uint8)
        wc = np.ascontiguousarray(w.numpy())
        L.check(L.lib.innfer_pack_conv3x3(wc.ctypes.data, 64, Cc, packed.ctypes.data))
        d_packed, d_bias = torch.from_numpy(packed).to(dev), b.to(dev)
        out = torch.full((1, N, H, W, 32), -3.0, dtype=torch.float16, device=dev)
        a = L.ConvArgs()
        a.d_in, a.in_group_stride, a.C = slab.data_ptr(), g, Cc
        a.d_packed, a.d_bias = d_packed.data_ptr(), d_bias.data_ptr()
        a.d_out, a.out_group_stride, a.K = out.data_ptr(), g, 64
        a.N, a.H, a.W, a.act = N, H, W, 7
        L.check(L.lib.innfer_conv3x3_f16(C.byref(a), None))
        got = torch.empty((N, 32, H, W), dtype=torch.float32, device=dev)
        L.check(L.lib.innfer_slab_to_nchw(out.data_ptr(), g, 0, got.data_ptr(), L.F32, N, 32, H, W, None))
        torch.cuda.synchronize()
        err = (got.cpu() - ref).abs().max().item()
        assert err < 4e-3, (N, Cc, H, W, err)


def test_column7_conv_vs_torch(dev):
    """The 7 x 1 column conv of the single-conv ABI (three vertically displaced 3-tap blocks of the halo-tile kernel) against torch: zero-padded
    and reflected rows, 32 / 64 outputs, 32 / 64 input channels, ragged and sub-tile sizes, batches."""
    import torch.nn.functional as F
    import innfer_amd.lib as L
    rng = np.random.RandomState(5)
    for i, (N, Cc, K, H, W, reflect) in enumerate([(1, 32, 32, 32, 40, 0), (1, 32, 64, 32, 40, 1), (2, 32, 64, 64, 64, 1), (1, 64, 32, 19, 70, 0),
                                                   (2, 32, 32, 8, 33, 1), (1, 32, 64, 50, 50, 0), (1, 32, 64, 4, 9, 1)]):
        act = i % 3
        x = torch.from_numpy(rng.uniform(-1, 1, (N, Cc, H, W)).astype(np.float32)).half()
        w = torch.from_numpy((rng.uniform(-1, 1, (K, Cc, 7)) / np.sqrt(7 * Cc)).astype(np.float32)).half().float()
        b = torch.from_numpy(rng.uniform(-0.5, 0.5, K).astype(np.float32))
        xp = F.pad(x.float(), (0, 0, 3, 3), mode="reflect") if reflect else F.pad(x.float(), (0, 0, 3, 3))
        ref = F.conv2d(xp, w[:, :, :, None], b)
        ref = ref if act == 0 else F.leaky_relu(ref, 0.2) if act == 1 else F.relu(ref)
        g = N * H * W * 32
        slab = torch.full((Cc // 32, N, H, W, 32), 7.0, dtype=torch.float16, device=dev)
        L.check(L.lib.innfer_nchw_to_slab(x.to(dev).contiguous().data_ptr(), L.F16, slab.data_ptr(), g, 0, N, Cc, H, W, None))
        packed = np.zeros(L.lib.innfer_conv7x1_packed_bytes(K, Cc), dtype=np.uint8)
        wc = np.ascontiguousarray(w.numpy())
        L.check(L.lib.innfer_pack_conv7x1(wc.ctypes.data, K, Cc, packed.ctypes.data))
        d_packed, d_bias = torch.from_numpy(packed).to(dev), torch.cat([b, torch.zeros(64 - K)]).to(dev)
        out = torch.full((max(K, 32) // 32, N, H, W, 32), -3.0, dtype=torch.float16, device=dev)
        a = L.ConvArgs()
        a.d_in, a.in_group_stride, a.C = slab.data_ptr(), g, Cc
        a.d_packed, a.d_bias = d_packed.data_ptr(), d_bias.data_ptr()
        a.d_out, a.out_group_stride, a.K = out.data_ptr(), g, K
        a.N, a.H, a.W, a.act, a.column7, a.reflect_pad = N, H, W, act, 1, reflect
        L.check(L.lib.innfer_conv3x3_f16(C.byref(a), None))
        res = torch.empty((N, K, H, W), dtype=torch.float32, device=dev)
        L.check(L.lib.innfer_slab_to_nchw(out.data_ptr(), g, 0, res.data_ptr(), L.F32, N, K, H, W, None))
        torch.cuda.synchronize()
        err = (res.cpu() - ref).abs().max().item()
        assert err < 4e-3, (N, Cc, K, H, W, reflect, err)


def test_filter2d_golden(dev, golden):
    """filter2D against the reference's own function (golden G25): four border modes, 3x3 / 5x7 (normalised) / 4x4 (even: asymmetric padding) kernels, the box
    kernel of the guided filter; fp32 to 2e-6, fp16 input to fp16 rounding; the reference's errors."""
    from innfer_amd.utils import utils as U
    g = golden("g25_filter2d")
    x = torch.from_numpy(g["x"]).to(dev)
    for b in ("constant", "reflect", "replicate", "circular"):
        for name, kw in (("k33", {}), ("k57n", dict(normalized=True)), ("k44", {})):
            k = torch.from_numpy(g[name.rstrip("n")])
            y = U.filter2D(x, k, border_type=b, **kw)
            assert y.shape == x.shape and y.dtype == x.dtype
            assert np.abs(y.cpu().numpy() - g[f"{name}_{b}"]).max() < 2e-6, (name, b)
            yh = U.filter2D(x.half(), k, border_type=b, **kw)
            assert yh.dtype == torch.float16 and np.abs(yh.float().cpu().numpy() - g[f"{name}_{b}"]).max() < 6e-3, (name, b)
    assert np.abs(U.filter2D(x, U.get_box_kernel(5).unsqueeze(0)).cpu().numpy() - g["box5"]).max() < 2e-6
    with pytest.raises(ValueError):
        U.filter2D(x, torch.ones(1, 3, 3), border_type="wrap")
    with pytest.raises(RuntimeError):
        U.filter2D(x.cpu(), torch.ones(1, 3, 3))


def test_unet256_upconv_full_depth_vs_oracle(dev):
    """upsample_mode='upconv' at unet_256's full depth (8 levels, 1x1 bottleneck -> the 3x3 conv runs on 2x2 .. 256x256 upsampled grids
    with 512 .. 1024 input channels), batch 2, train-mode and eval-mode BatchNorm, against the oracle (itself pinned on the reference, G23)."""
    import oracle
    from innfer_amd import synth
    from innfer_amd.architectures.UNet_arch import UnetGenerator
    net = UnetGenerator(3, 3, 8, ngf=64, upsample_mode="upconv")
    shapes = {k: tuple(v.shape) for k, v in net.state_dict().items()}
    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in synth.fill_running_stats(synth.fill_state_dict(shapes, 77), 78).items()}
    net.load_state_dict(sd, strict=True)
    net = net.to(dev)
    x = torch.from_numpy(synth.uniform((2, 3, 256, 256), 79, -1.0, 1.0))
    for training in (True, False):
        net.train(training)
        y = net(x.to(dev).half()).float().cpu()
        with torch.no_grad():
            ref = torch.cat([oracle.unet_forward(sd, x[i:i + 1], num_downs=8, training=training, upsample_mode="upconv") for i in range(2)], 0)
        err = (y - ref).abs()
        assert err.max().item() < 3e-2 and err.mean().item() < 3e-3, (training, err.max().item(), err.mean().item())


def test_unet256_big_batch_uses_wide_tiles_and_stays_identical(dev):
    """A batch of 16 makes the mid layers take the 256 px x 128 channel GEMM tiles and keeps the deep
    layers on the split-K path; every image must still equal its own batch-1 forward bit for bit."""
    from innfer_amd import synth
    from innfer_amd.architectures import get_network
    from innfer_amd.utils.defaults import get_network_G_config
    net = get_network(get_network_G_config("p2p_256", 1))
    shapes = {k: tuple(v.shape) for k, v in net.state_dict().items()}
    net.load_state_dict(_sd(shapes, seed=5), strict=True)
    net = net.to(dev).train()
    x = torch.from_numpy(synth.uniform((16, 3, 256, 256), 41, -1.0, 1.0)).to(dev).half()
    y = net(x)
    assert torch.isfinite(y).all()
    for i in (0, 7, 15):
        assert torch.equal(y[i:i + 1], net(x[i:i + 1])), i
    # an odd batch: the last image of the 16-pixel-wide levels has no partner in its tile row (conv3x3_pc's image pairs), statistics per image
    y5 = net(x[:5])
    for i in range(5):
        assert torch.equal(y5[i:i + 1], y[i:i + 1]), i


def test_color_fix_vs_oracle(dev):
    """`-cf` colour fix.  The oracle restates OpenCV's published bicubic resize and 3x3
    Gaussian (parity with OpenCV itself is unpinned); the HIP kernels must agree with it to the uint8
    code: the final cast truncates, so float32 rounding noise (powf) may move a value across an integer
    boundary -- at most +-1 code, on at most 0.2 % of the values."""
    import oracle
    from oracle.colorfix import color_fix as ref_color_fix
    from innfer_amd import synth
    from innfer_amd.utils import utils as U
    for (hA, wA, scale, Cc) in [(25, 37, 4, 3), (64, 48, 2, 3), (30, 30, 1, 3), (17, 9, 4, 1)]:
        a = synth.image_u8(hA, wA, Cc, 3)
        # SR image = the LR image blown up and perturbed, like a real model output
        b = np.repeat(np.repeat(a, scale, 0), scale, 1).astype(np.int16) + (synth.image_u8(hA * scale, wA * scale, Cc, 4) % 25).astype(np.int16) - 12
        b = np.clip(b, 0, 255).astype(np.uint8)
        got = U.color_fix(a, b, device=dev)
        ref = ref_color_fix(a, b)
        assert got.shape == ref.shape and got.dtype == np.uint8
        d = np.abs(got.astype(np.int16) - ref.astype(np.int16))
        assert d.max() <= 1 and (d > 0).mean() <= 2e-3, (hA, wA, scale, d.max(), (d > 0).mean())
    with pytest.raises(ValueError):
        U.color_fix(synth.image_u8(20, 20, 3, 1), synth.image_u8(10, 10, 3, 2), device=dev)      # LR larger than SR


def test_command_line_image_loop(dev, tmp_path, monkeypatch, capsys):
    """`run.py -m <chain> -i in -o out [-cf] [-comp]` (run.py:318-445) end to end on the HIP engine: files in, files out.  Five images (one
    larger than a chop tile; more than the pipelined loop keeps in flight) and one file that is no image (reported and skipped, run.py:407-409),
    a 1x + 2x model chain found by partial name in ./models; the PNGs must hold exactly what the library calls
    return and lie within one uint8 code of the oracle's fp32 forward on >= 99 % of the values."""
    import oracle
    from innfer_amd import run as R, synth
    from innfer_amd.utils import utils as U
    (tmp_path / "models").mkdir(); (tmp_path / "in").mkdir()
    sds = {}
    for name, scale, seed in (("1x_clean.pth", 1, 31), ("2x_up.pth", 2, 32)):
        sds[name] = _sd(synth.rrdbnet_shapes(nb=1, scale=scale), seed)
        torch.save(sds[name], str(tmp_path / "models" / name))
    imgs = {"small": synth.image_u8(37, 52, 3, 41), "large": synth.image_u8(210, 230, 3, 42), "a": synth.image_u8(20, 31, 3, 43),
            "b": synth.image_u8(64, 17, 3, 44), "c": synth.image_u8(9, 9, 3, 45)}
    for k, im in imgs.items():
        U.save_img(im, str(tmp_path / "in" / f"{k}.png"))
    (tmp_path / "in" / "broken.png").write_bytes(b"this is not a PNG file")
    monkeypatch.chdir(tmp_path)
    assert R.main(["-m", "clean+2x_up", "-i", "in", "-o", "out"]) == 0
    assert "Error reading image" in capsys.readouterr().out and "broken.png" not in os.listdir(tmp_path / "out")
    assert sorted(os.listdir(tmp_path / "out")) == sorted(f"{k}.png" for k in imgs)
    assert R.main(["-m", "clean+2x_up", "-i", "in", "-o", "out_cf", "-cf", "-comp"]) == 0
    m1 = R.Model(str(tmp_path / "models" / "1x_clean.pth"), "infer", 1)
    m2 = R.Model(str(tmp_path / "models" / "2x_up.pth"), "infer", 2)
    for k, im in imgs.items():
        got = U.read_img(str(tmp_path / "out" / f"{k}.png"))
        want = U.tensor2np(m2(m1(U.np2tensor(im, dtype=torch.float16))))
        assert got.shape == (2 * im.shape[0], 2 * im.shape[1], 3) and np.array_equal(got, want), k
        comp = U.read_img(str(tmp_path / "out_cf" / f"{k}.png"))
        assert comp.shape == (2 * im.shape[0], 4 * im.shape[1], 3)
        assert np.array_equal(comp[:, 2 * im.shape[1]:], U.color_fix(im, want)), k
        if k == "small":                                   # below the tile size chop_forward is one tile: the plain forward
            x = oracle.np2tensor(im)
            with torch.no_grad():
                ref = oracle.tensor2np(oracle.rrdbnet_forward(sds["2x_up.pth"], oracle.rrdbnet_forward(sds["1x_clean.pth"], x, nb=1, scale=1), nb=1, scale=2))
            assert (np.abs(got.astype(np.int16) - ref.astype(np.int16)) <= 1).mean() >= 0.99
    # -no_fp16 (run.py:345,421-422): the same chain on the fp32-accurate engine -- exactly the float32 library calls, and the oracle's fp32
    # chop_forward chain to the uint8 code (<= 1e-4 before the rounding: a code can only differ where 255 x lies that close to a half)
    assert R.main(["-m", "clean+2x_up", "-i", "in", "-o", "out32", "-no_fp16"]) == 0
    f1 = lambda t: oracle.rrdbnet_forward(sds["1x_clean.pth"], t, nb=1, scale=1)
    f2 = lambda t: oracle.rrdbnet_forward(sds["2x_up.pth"], t, nb=1, scale=2)
    for k, im in imgs.items():
        got = U.read_img(str(tmp_path / "out32" / f"{k}.png"))
        assert np.array_equal(got, U.tensor2np(m2(m1(U.np2tensor(im, dtype=torch.float32))))), k
        with torch.no_grad():
            ref = oracle.tensor2np(oracle.chop_forward(f2, oracle.chop_forward(f1, oracle.np2tensor(im), 1), 2))
        d = np.abs(got.astype(np.int16) - ref.astype(np.int16))
        assert d.max() <= 1 and (d == 0).mean() >= 0.999, (k, d.max(), (d == 0).mean())
    # PAN has an fp32 mode since round 4: the flag runs it (float32 tensors through Model.__call__)
    from innfer_amd.architectures import get_network
    from innfer_amd.utils.defaults import get_network_G_config
    torch.save(get_network(get_network_G_config("pan", 4)).state_dict(), str(tmp_path / "models" / "4x_pan.pth"))
    assert R.main(["-m", "4x_pan", "-i", "in", "-o", "out_pan", "-no_fp16"]) == 0
    assert sorted(os.listdir(tmp_path / "out_pan")) == sorted(f"{k}.png" for k in imgs)
    # (every generator has an fp32 mode since round 4: test_gpu_fp32_mode.py::test_every_generator_answers_float32_tensors)


@pytest.mark.parametrize("chop", [True, False])
def test_image_in_image_out_equals_the_separate_passes(dev, tmp_path, chop):
    """Model.run_u8: np2tensor and tensor2np fused into the tile gather / blend (chop) or into the first / last conv (un-tiled) must return
    exactly tensor2np(model(np2tensor(img)[.half()])) -- fp16 and fp32 mode, with and without [-1,1] normalisation, images smaller and larger
    than a chop tile, gray models."""
    from innfer_amd import run as R, synth
    from innfer_amd.utils import utils as U
    for in_nc, name in ((3, "2x_rgb.pth"), (1, "2x_gray.pth")):
        torch.save(_sd(synth.rrdbnet_shapes(nb=1, scale=2, in_nc=in_nc, out_nc=in_nc), 60 + in_nc), str(tmp_path / name))
        m = R.Model(str(tmp_path / name), "infer", 2, in_nc=in_nc, out_nc=in_nc, chop=chop)
        for (h, w, seed) in [(37, 52, 61), (210, 230, 62), (200, 200, 63), (1, 1, 64)]:
            if chop and min(h, w) < 2:
                continue                      # a one-pixel patch has tile step 0: chop_forward raises, in the reference too
            img = synth.image_u8(h, w, in_nc, seed)
            for fp16 in (True, False):
                for normalize in (False, True):
                    want = U.tensor2np(m(U.np2tensor(img, normalize=normalize, dtype=torch.float16 if fp16 else torch.float32)), denormalize=normalize)
                    got = m.run_u8(img, normalize=normalize, fp16=fp16)
                    assert got.dtype == np.uint8 and got.shape == want.shape and np.array_equal(got, want), (in_nc, h, w, fp16, normalize)
            d = torch.from_numpy(img).to(dev)
            assert np.array_equal(m.run_u8(d).cpu().numpy(), m.run_u8(img))          # device image in, device image out
    net = m.model
    batch = torch.from_numpy(np.stack([synth.image_u8(20, 24, 1, 70 + i) for i in range(3)])).to(dev)
    got = net.forward_u8(batch)
    for i in range(3):
        assert torch.equal(got[i], net.forward_u8(batch[i]))


def test_guided_filter_windows_and_fast_mode_golden(dev, golden):
    """guided_filter(r=2), (ks=7) and mode='fast' with a 2x guidance image (utils.py:548-626) against the reference (golden G21)."""
    from innfer_amd.utils import utils as U
    from test_oracle_golden import _guided_cases
    g = golden("g21_guided")
    x, y, xh, cases = _guided_cases()
    x, y, xh = x.to(dev), y.to(dev), xh.to(dev)
    for tag, kw in cases.items():
        args = dict(ks=kw["ks"], eps=kw["eps"])
        if kw.get("hr"):
            args.update(x_HR=xh, mode="fast")
        got = U.guided_filter(x, y, **args).cpu().numpy()
        assert got.shape == g[tag].shape and np.abs(got - g[tag]).max() < 5e-5, (tag, np.abs(got - g[tag]).max())
    assert torch.equal(U.guided_filter(x, y, r=1, eps=5e-3), U.guided_filter(x, y, ks=3, eps=5e-3))
    # the forms that follow the reference's formula step by step on the HIP filter2D: a caller's conv_a, an even window, a precomputed kernel
    conv_a = torch.nn.Sequential(torch.nn.Conv2d(6, 3, 1)).to(dev)
    with torch.no_grad():
        conv_a[0].weight.copy_(torch.from_numpy(g["conv_w"])); conv_a[0].bias.copy_(torch.from_numpy(g["conv_b"]))
        got = U.guided_filter(x, y, x_HR=xh, r=1, mode="conv", conv_a=conv_a).cpu().numpy()
    assert got.shape == g["conv"].shape and np.abs(got - g["conv"]).max() < 5e-5
    assert np.abs(U.guided_filter(x, y, ks=4, eps=1e-2).cpu().numpy() - g["ks4"]).max() < 5e-5
    assert np.abs(U.guided_filter(x, y, box_kernel=torch.from_numpy(g["bk"]), eps=1e-2).cpu().numpy() - g["bk_out"]).max() < 5e-5
    # the stepwise form and the fused kernels agree where both apply
    assert (U._guided_filter_stepwise(x, y, None, U.get_box_kernel(5), 5e-3, "regular", None) - U.guided_filter(x, y, r=2, eps=5e-3)).abs().max().item() < 5e-5
    with pytest.raises(ValueError):
        U.guided_filter(x, y, r=1, mode="fast")
    with pytest.raises(ValueError):
        U.guided_filter(x, y, x_HR=xh, r=1, mode="conv")


def test_linear_resize_vs_oracle(dev):
    """linear_resize (utils.py:267-276, the pix2pix pre-step): srgb2linear -> bicubic to the next multiple of `st` -> linear2srgb against the
    oracle's restatement of OpenCV's INTER_CUBIC (unpinned against OpenCV itself, like color_fix); the truncating cast allows one code."""
    import oracle
    from oracle.colorfix import resize_cubic
    from innfer_amd import synth
    from innfer_amd.utils import utils as U
    for (h, w, st) in [(100, 130, 64), (250, 256, 256), (64, 64, 64), (31, 7, 16)]:
        img = synth.image_u8(h, w, 3, 51)
        got = U.linear_resize(img, st, device=dev)
        oh, ow = -(-h // st) * st, -(-w // st) * st
        if (oh, ow) == (h, w):
            assert got is img
            continue
        ref = oracle.linear2srgb(resize_cubic(oracle.srgb2linear(img).astype(np.float32), (ow, oh)))
        d = np.abs(got.astype(np.int16) - ref.astype(np.int16))
        assert got.shape == (oh, ow, 3) and d.max() <= 1 and (d > 0).mean() <= 2e-3, (h, w, st, d.max(), (d > 0).mean())


def test_frame_pipeline_equals_serial_loop(dev):
    """The overlapped image loop (uint8 over PCIe on side streams) must return exactly what the serial
    np2tensor -> model -> tensor2np loop returns, in order, with and without the colour fix."""
    from innfer_amd import synth
    from innfer_amd.pipeline import FramePipeline
    from innfer_amd.utils import utils as U
    net, _ = _rrdb(dev, 1, 2)
    frames = [synth.image_u8(40, 56, 3, 60 + i) for i in range(7)]
    serial = [U.tensor2np(net(U.np2tensor(f, device=dev).half())) for f in frames]
    got = [o.copy() for o in FramePipeline(net, scale=2, device=dev, depth=3)(frames)]
    assert len(got) == len(serial) and all(np.array_equal(a, b) for a, b in zip(got, serial))
    # a yielded view stays intact until the next frame has been yielded (a consumer may keep ONE previous frame without copying it)
    prev = None
    for i, o in enumerate(FramePipeline(net, scale=2, device=dev, depth=2)(frames)):
        if prev is not None:
            torch.cuda.synchronize()
            assert np.array_equal(prev, serial[i - 1])
        assert np.array_equal(o, serial[i])
        prev = o
    fixed = [o.copy() for o in FramePipeline(net, scale=2, device=dev, depth=2, color_fix=True)(frames[:3])]
    for f, sr, fx in zip(frames, serial, fixed):
        assert np.array_equal(fx, U.color_fix(f, sr, device=dev))
    # a consumer that abandons the stream mid-way (break) leaves a clean ring behind: the same pipeline object serves the next stream in full
    pipe = FramePipeline(net, scale=2, device=dev, depth=3)
    for i, o in enumerate(pipe(frames)):
        if i == 1:
            break
    again = [o.copy() for o in pipe(frames)]
    assert len(again) == len(serial) and all(np.array_equal(a, b) for a, b in zip(again, serial))


def test_ppon_scales_golden(dev, golden):
    """PPON with upscale 8 (three upconv stages), 3 (one nearest-3x stage) and 2 against the reference (golden G27), all three outputs."""
    import ast
    from innfer_amd import synth
    from innfer_amd.architectures.PPON_arch import PPON
    g = golden("g27_ppon_scales")
    for j, sc in enumerate((8, 3, 2)):
        shapes = {str(k): ast.literal_eval(str(s)) for k, s in zip(g[f"x{sc}_keys"], g[f"x{sc}_shapes"])}
        net = PPON(3, 64, 2, 3, upscale=sc)
        assert {k: tuple(v.shape) for k, v in net.state_dict().items()} == {k: tuple(v) for k, v in shapes.items()}
        net.load_state_dict(_sd(shapes, 340 + j), strict=True)
        net = net.to(dev).eval()
        x = torch.from_numpy(synth.uniform((1, 3, 10, 12), 350 + j)).to(dev)
        for xin in (x.half(),):          # (float32 tensors run the engine's fp32 mode: test_gpu_fp32_mode.py)
            outs = net(xin)
            for name, y in zip("csp", outs):
                ref = g[f"x{sc}_{name}"].astype(np.float32)
                assert tuple(y.shape) == ref.shape
                err = np.abs(y.float().cpu().numpy() - ref)
                assert err.max() < 1e-2 * max(1.0, np.abs(ref).max()), (sc, name, err.max())


def test_ppon_golden(dev, golden):
    """PPON 4x (24 + 4 residual-in-residual blocks of eight dilated convs, three heads)
    against the reference (golden G13), all three outputs.  fp16 slabs between the layers, fp32 sums:
    tolerance 1e-2 relative to the output range (|out| up to 5.5 with the synthetic weights)."""
    import ast
    from innfer_amd import synth
    from innfer_amd.architectures import get_network
    from innfer_amd.utils.defaults import get_network_G_config
    g = golden("g13_ppon")
    shapes = {str(k): ast.literal_eval(str(s)) for k, s in zip(g["keys"], g["shapes"])}
    net = get_network(get_network_G_config("ppon", 4))
    assert {k: tuple(v.shape) for k, v in net.state_dict().items()} == {k: tuple(v) for k, v in shapes.items()}
    net.load_state_dict(_sd(shapes), strict=True)
    net = net.to(dev).eval()
    for (h, w, seed) in [(24, 24, 13), (20, 28, 14)]:
        x = torch.from_numpy(synth.uniform((1, 3, h, w), seed)).to(dev)
        for xin in (x.half(),):          # (float32 tensors run the engine's fp32 mode: test_gpu_fp32_mode.py)
            outs = net(xin)
            assert len(outs) == 3
            for name, y in zip("csp", outs):
                ref = g[f"out_{name}_{h}x{w}"].astype(np.float32)
                err = np.abs(y.float().cpu().numpy() - ref)
                assert err.max() < 1e-2 * max(1.0, np.abs(ref).max()) and err.mean() < 2e-3 * max(1.0, np.abs(ref).max()), (name, h, w, err.max(), err.mean())
    xb = torch.from_numpy(synth.uniform((2, 3, 24, 24), 13)).to(dev)
    xb[1] = torch.from_numpy(synth.uniform((1, 3, 24, 24), 77)).to(dev)[0]
    xb = xb.half()
    yb = net(xb)[2]
    assert torch.equal(yb[0:1], net(xb[0:1])[2]) and torch.equal(yb[1:2], net(xb[1:2])[2])
    # Model keeps the perceptual output (run.py:191-192)
    from innfer_amd.run import Model
    m = Model(None, arch="infer", device=str(dev), chop=False, state_dict=_sd(shapes))
    assert m.arch == "ppon" and m.scale == 4
    assert torch.equal(m(xb[0:1].half()), net(xb[0:1].half())[2])


def test_cyclegan_resnet9_golden(dev, golden):
    """CycleGAN ResnetGenerator, 9 blocks against the reference (golden G14): reflection
    padding, stride-2 convs, instance norm over as few as 8x10 pixels, transposed convs, tanh.  fp16
    activations through 23 instance norms: SURVEY 8c's 1e-2 on the tanh output, and bounded by the reference's own fp16 mode (G17)."""
    import ast
    from innfer_amd import synth
    from innfer_amd.architectures import get_network
    from innfer_amd.utils.defaults import get_network_G_config
    g, g17 = golden("g14_resnet9"), golden("g17_fp16_and_eval")
    shapes = {str(k): ast.literal_eval(str(s)) for k, s in zip(g["keys"], g["shapes"])}
    net = get_network(get_network_G_config("resnet_9blocks", 1))
    assert {k: tuple(v.shape) for k, v in net.state_dict().items()} == {k: tuple(v) for k, v in shapes.items()}
    net.load_state_dict(_sd(shapes), strict=True)
    net = net.to(dev).eval()
    for (h, w, seed) in [(32, 40, 15), (64, 64, 16)]:
        x = torch.from_numpy(synth.uniform((1, 3, h, w), seed, -1.0, 1.0)).to(dev)
        ref = g[f"out_{h}x{w}"].astype(np.float32)
        for xin in (x.half(),):          # (float32 tensors run the engine's fp32 mode: test_gpu_fp32_mode.py)
            y = net(xin).float().cpu().numpy()
            err = np.abs(y - ref)
            assert np.isfinite(y).all() and np.abs(y).max() <= 1.0
            assert err.max() < 1e-2 and err.mean() < 1e-3, (h, w, err.max(), err.mean())          # SURVEY 8c (measured 3.4e-3 / 6.4e-4)
            # the reference's own fp16 mode on this input (golden G17) is 4.1e-3..4.2e-3 max / 7e-4..8e-4 mean away from its fp32 output:
            # the HIP path must be no further from the fp32 truth than that, and within twice that of the reference's fp16 output
            ref_max, ref_mean = [float(v) for v in g17[f"resnet_fp16_err_vs_fp32_{h}x{w}"]]
            e16 = np.abs(y - g17[f"resnet_fp16_out_{h}x{w}"])
            print(f"resnet9 {h}x{w} in={xin.dtype}: HIP vs fp32 max {err.max():.2e} mean {err.mean():.2e}; vs ref fp16 max {e16.max():.2e} mean {e16.mean():.2e}; "
                  f"reference fp16 mode vs fp32 {ref_max:.2e} / {ref_mean:.2e}")
            assert err.max() <= 1.1 * ref_max and err.mean() <= 1.1 * ref_mean, (h, w, err.max(), err.mean())
            assert e16.max() <= 2.0 * ref_max + 1e-3 and e16.mean() <= 2.0 * ref_mean
            assert _codes_within_one(dev, (y + 1) / 2, (ref + 1) / 2) >= 0.99
    xa = torch.from_numpy(synth.uniform((1, 3, 32, 40), 15, -1.0, 1.0)).to(dev).half()
    xb = torch.from_numpy(synth.uniform((1, 3, 32, 40), 91, -1.0, 1.0)).to(dev).half()
    yab = net(torch.cat([xa, xb], 0))
    assert torch.equal(yab[0:1], net(xa)) and torch.equal(yab[1:2], net(xb))
    with pytest.raises(ValueError):
        net(torch.zeros(1, 3, 30, 40, device=dev, dtype=torch.float16))                      # not a multiple of 4


def test_cyclegan_resnet_padding_and_dropout_variants_golden(dev, golden):
    """ResnetGenerator(padding_type='zero' / 'replicate', use_dropout=True) in eval mode (ResNet_arch.py:104-146) against the reference (G22):
    same parameter names (the conv indices inside `conv_block` move with the pad and dropout layers), outputs within the CycleGAN tolerance."""
    import ast
    from innfer_amd import synth
    from innfer_amd.architectures.ResNet_arch import ResnetGenerator
    from test_oracle_golden import G22_CASES, _g22_state
    g = golden("g22_resnet_variants")
    for i, (tag, kw) in enumerate(G22_CASES.items()):
        shapes = {str(k): ast.literal_eval(str(s)) for k, s in zip(g[tag + "_keys"], g[tag + "_shapes"])}
        kw = dict(kw)
        train = kw.pop("train", False)
        net = ResnetGenerator(3, 3, 64, n_blocks=2, **{"norm_type": "instance", **kw})
        assert list(net.state_dict()) == [str(k) for k in g[tag + "_keys"]]
        net.load_state_dict(_g22_state(shapes, kw, i), strict=True)
        net = net.to(dev)
        net = net.train() if train else net.eval()
        x = torch.from_numpy(synth.uniform((1, 3, 32, 40), 225 + i, -1.0, 1.0)).to(dev)
        for xin in (x.half(),):          # (float32 tensors run the engine's fp32 mode: test_gpu_fp32_mode.py)
            err = np.abs(net(xin).float().cpu().numpy() - g[tag])
            assert err.max() < 1e-2 and err.mean() < 2e-3, (tag, err.max(), err.mean())
    with pytest.raises(NotImplementedError):
        ResnetGenerator(3, 3, 64, norm_type="instance", padding_type="circular")
    with pytest.raises(NameError):
        ResnetGenerator(3, 3, 64, norm_type="group")              # the reference's own error
    assert ResnetGenerator(3, 3).batch_norm                        # the constructor's default is norm_type='batch' (ResNet_arch.py:19)
    drop = ResnetGenerator(3, 3, 64, norm_type="instance", n_blocks=1, use_dropout=True).to(dev).train()
    with pytest.raises(NotImplementedError):
        drop(x)                                  # use_dropout=True in train mode is random: refused


def test_cyclegan_resnet_chop_tile_shapes_vs_oracle(dev):
    """ResnetGenerator on 200 x 200 chop tiles and a 120 x 200 image (ragged tile rows and columns at every level): the transposed convs on the
    phase lattice of the halo-tile kernel and the last 7x7 conv in its nine-sub-block form over the reflection-padded slab, batch 2, against the
    oracle (pinned on the reference by G14 / G22); every image equals its batch-1 forward bit for bit."""
    import oracle
    from innfer_amd import synth
    from innfer_amd.architectures.ResNet_arch import ResnetGenerator
    net = ResnetGenerator(3, 3, 64, norm_type="instance", n_blocks=2)
    shapes = {k: tuple(v.shape) for k, v in net.state_dict().items()}
    sd = _sd(shapes, 333)
    net.load_state_dict(sd, strict=True)
    net = net.to(dev).eval()
    for (h, w, seed) in [(200, 200, 31), (120, 200, 32)]:
        x = torch.from_numpy(synth.uniform((2, 3, h, w), seed, -1.0, 1.0))
        y = net(x.to(dev).half())
        with torch.no_grad():
            ref = torch.cat([oracle.resnet_forward(sd, x[i:i + 1], n_blocks=2) for i in range(2)], 0)
        err = (y.float().cpu() - ref).abs()
        assert err.max().item() < 1e-2 and err.mean().item() < 1e-3, (h, w, err.max().item(), err.mean().item())
        assert torch.equal(y[1:2], net(x[1:2].to(dev).half()))


def test_wbcunet_and_guided_filter_golden(dev, golden):
    """White-box-Cartoonization UNet + the guided filter run.py applies to its output
    against the reference (golden G15).  No norm layers: fp16 slabs, tolerance 5e-3 on outputs of O(0.2)."""
    import ast
    from innfer_amd import synth
    from innfer_amd.architectures import get_network
    from innfer_amd.utils.defaults import get_network_G_config
    from innfer_amd.utils import utils as U
    g = golden("g15_wbcunet")
    shapes = {str(k): ast.literal_eval(str(s)) for k, s in zip(g["keys"], g["shapes"])}
    net = get_network(get_network_G_config("wbcunet", 1))
    assert {k: tuple(v.shape) for k, v in net.state_dict().items()} == {k: tuple(v) for k, v in shapes.items()}
    net.load_state_dict(_sd(shapes), strict=True)
    net = net.to(dev).eval()
    for (h, w, seed) in [(32, 40, 17), (64, 64, 18)]:
        x = torch.from_numpy(synth.uniform((1, 3, h, w), seed, -1.0, 1.0)).to(dev)
        ref, ref_gf = g[f"out_{h}x{w}"].astype(np.float32), g[f"gf_{h}x{w}"].astype(np.float32)
        for xin in (x.half(),):          # (float32 tensors run the engine's fp32 mode: test_gpu_fp32_mode.py)
            y = net(xin)
            err = np.abs(y.float().cpu().numpy() - ref)
            assert err.max() < 5e-3 and err.mean() < 5e-4, (h, w, err.max(), err.mean())
        # guided filter on the reference's own tensors (fp32): kernel vs reference
        gf = U.guided_filter(x, torch.from_numpy(ref).to(dev), r=1, eps=5e-3).cpu().numpy()
        assert np.abs(gf - ref_gf).max() < 2e-5
        # and the run.py sequence end to end in fp16
        y16 = net(x.half())
        gf16 = U.guided_filter(x.half(), y16, r=1, eps=5e-3).float().cpu().numpy()
        assert np.abs(gf16 - ref_gf).max() < 5e-3
    xa = torch.from_numpy(synth.uniform((2, 3, 32, 40), 17, -1.0, 1.0)).to(dev).half()
    yab = net(xa)
    assert torch.equal(yab[0:1], net(xa[0:1])) and torch.equal(yab[1:2], net(xa[1:2]))
    # the TensorFlow-converted variant: tf_same_padding in front of the stride-2 convs, tf_2xupsample_bilinear
    net_tf = get_network(get_network_G_config("wbcunet_tf", 1))
    net_tf.load_state_dict(_sd(shapes), strict=True)
    net_tf = net_tf.to(dev).eval()
    x = torch.from_numpy(synth.uniform((1, 3, 32, 40), 17, -1.0, 1.0)).to(dev)
    err = np.abs(net_tf(x.half()).float().cpu().numpy() - g["out_tf_32x40"])
    assert err.max() < 5e-3 and err.mean() < 5e-4, (err.max(), err.mean())


def test_pan_golden(dev, golden):
    """PAN 4x (nf 40, unf 24, 16 SCPA blocks, FSA self attention) against the
    reference (golden G8).  fp16 slabs between the GEMMs, fp32 accumulation / gates / softmax /
    bicubic: tolerance 1e-2 on outputs of O(1), mean error an order of magnitude below."""
    import ast
    from innfer_amd import synth
    from innfer_amd.architectures import get_network
    from innfer_amd.utils.defaults import get_network_G_config
    g = golden("g8_pan")
    shapes = {str(k): ast.literal_eval(str(s)) for k, s in zip(g["keys"], g["shapes"])}
    sd = _sd(shapes)
    net = get_network(get_network_G_config("pan", 4))
    net.load_state_dict(sd, strict=True)
    net = net.to(dev).eval()
    outs = {}
    for (h, w, seed) in [(48, 48, 8), (50, 70, 9)]:
        x = torch.from_numpy(synth.uniform((1, 3, h, w), seed)).to(dev)
        ref = g[f"out_{h}x{w}"].astype(np.float32)
        for xin in (x.half(),):          # (float32 tensors run the engine's fp32 mode: test_gpu_fp32_mode.py)
            y = net(xin).float().cpu().numpy()
            err = np.abs(y - ref)
            assert y.shape == ref.shape and np.isfinite(y).all()
            assert err.max() < 1e-2 * max(1.0, np.abs(ref).max()) and err.mean() < 1.5e-3, (h, w, err.max(), err.mean())
        outs[(h, w)] = net(x.half()).float().cpu().numpy()
    # a batch is independent images (attention and pooling are per image)
    xa = torch.from_numpy(synth.uniform((1, 3, 48, 48), 8)).to(dev).half()
    xb = torch.from_numpy(synth.uniform((1, 3, 48, 48), 21)).to(dev).half()
    yab = net(torch.cat([xa, xb], 0)).float().cpu().numpy()
    assert np.array_equal(yab[0:1], outs[(48, 48)])
    assert np.array_equal(yab[1:2], net(xb).float().cpu().numpy())


def test_pan_fused_scpa_vs_five_launches_and_oracle(dev):
    """An SCPA block as ONE launch (csrc/pan_scpa.hip, innfer_pan_set_fused_scpa, the default) against the five-launch schedule of rounds 1-3 and the oracle:
    frames smaller than a 16 x 32 tile, ragged frames with tiles on every border, whole tiles, batches (images are independent: bit-equal to their own
    forwards), a 200 x 200 chop tile.  Both schedules round the same intermediate tensors to fp16; the 3 x 3 convs add their taps in another order."""
    import oracle
    from innfer_amd import synth
    from innfer_amd.architectures import get_network
    from innfer_amd.utils.defaults import get_network_G_config
    net = get_network(get_network_G_config({"type": "pan", "nb": 4}, 4))
    shapes = {k: tuple(v.shape) for k, v in net.state_dict().items()}
    sd = _sd(shapes, 41)
    net.load_state_dict(sd, strict=True)
    net = net.to(dev).eval()
    for i, shape in enumerate([(1, 3, 5, 7), (1, 3, 16, 32), (1, 3, 33, 65), (3, 3, 21, 37), (1, 3, 50, 70), (2, 3, 64, 96), (1, 3, 200, 200)]):
        x = torch.from_numpy(synth.uniform(shape, 300 + i))
        with torch.no_grad():
            ref = oracle.pan_forward(sd, x, nb=4, scale=4)
        net.fused_scpa = True
        y1 = net(x.to(dev).half())
        assert torch.equal(y1, net(x.to(dev).half()))
        if shape[0] > 1:
            assert torch.equal(y1[-1:], net(x[-1:].to(dev).half()))
        net._ws.fill_(0xFF)                                             # every byte read was written by this forward
        assert torch.equal(y1, net(x.to(dev).half()))
        net.fused_scpa = False
        y0 = net(x.to(dev).half())
        net.fused_scpa = 2                                              # the fused blocks with the VALU attention: the two changes apart
        y2 = net(x.to(dev).half())
        net.fused_scpa = 3                                              # two-group slabs between the blocks instead of the compact channel plane (round 5): same bits
        assert torch.equal(net(x.to(dev).half()), y1), shape
        net.fused_scpa = True
        e1, e0 = (y1.float().cpu() - ref).abs(), (y0.float().cpu() - ref).abs()
        d = (y1.float() - y0.float()).abs().max().item()
        da = (y1.float() - y2.float()).abs().max().item()
        print(f"PAN fused SCPA {shape}: vs oracle max {e1.max().item():.2e} mean {e1.mean().item():.2e} (five launches: {e0.max().item():.2e} / {e0.mean().item():.2e}); "
              f"between the schedules {d:.2e}; MFMA attention vs VALU attention {da:.2e}")
        bound = 1e-2 * max(1.0, ref.abs().max().item())
        assert e1.max().item() < bound and e1.mean().item() < 1.5e-3 and e0.max().item() < bound and d < 4e-3 and da < 2e-3, (shape, e1.max().item(), e0.max().item(), d, da)


def test_pan_scpa_two_workgroup_form_is_bit_identical(dev):
    """The SCPA block kernel's two forms (round 6): one 8-wave workgroup per CU on 16 x 32 tiles (pan_scpa_fused; innfer_pan_set_fused_scpa(pan, 7))
    and two 4-wave workgroups per CU on 8 x 32 tiles with x loaded straight into MFMA fragments (pan_scpa_duo; 6) run the same MFMAs in the same order per value: the
    whole network's outputs are bit-identical -- one-tile, tile-plus-one-pixel, border-only and multi-tile frames, batches, 200 x 200 chop tiles -- and so is the
    default, which picks the form by the frame."""
    from innfer_amd import synth
    from innfer_amd.architectures import get_network
    from innfer_amd.utils.defaults import get_network_G_config
    net = get_network(get_network_G_config("pan", 4))
    net.load_state_dict({k: torch.from_numpy(v) for k, v in synth.fill_state_dict({k: tuple(v.shape) for k, v in net.state_dict().items()}, 3).items()}, strict=True)
    net = net.to(dev).eval()
    try:
        for shape in [(1, 3, 8, 32), (1, 3, 9, 33), (2, 3, 37, 45), (1, 3, 6, 40), (3, 3, 16, 64), (1, 3, 70, 130), (2, 3, 200, 200), (1, 3, 136, 260)]:
            x = torch.from_numpy(synth.uniform(shape, 90 + shape[3], 0, 1)).to(dev).half()
            y = {}
            for mode in (7, 6, 1):
                net.fused_scpa = mode
                y[mode] = net(x)
            assert torch.equal(y[7], y[6]) and torch.equal(y[7], y[1]), shape
    finally:
        net.fused_scpa = 1


def test_pan_bench_shapes_untiled_vs_oracle(dev):
    """the shapes the bench runs PAN on, un-tiled, against the oracle -- 264 x 392 (6 468 pooled keys, ragged in both tile
    directions) and the `pan540` workload itself, 540 x 960 = 32 400 pooled keys = 507 key blocks through the running-max softmax of
    pan_attention_mfma (csrc/pan.hip); the largest shape the other tests reach is 200 x 200 = 2 500 keys.  The default 16-block network."""
    import oracle
    from innfer_amd import synth
    from innfer_amd.architectures import get_network
    from innfer_amd.utils.defaults import get_network_G_config
    net = get_network(get_network_G_config("pan", 4))
    shapes = {k: tuple(v.shape) for k, v in net.state_dict().items()}
    sd = _sd(shapes, 43)
    net.load_state_dict(sd, strict=True)
    net = net.to(dev).eval()
    for i, shape in enumerate([(1, 3, 264, 392), (1, 3, 540, 960)]):
        x = torch.from_numpy(synth.uniform(shape, 330 + i))
        with torch.no_grad():
            ref = oracle.pan_forward(sd, x, nb=16, scale=4)
        y1 = net(x.to(dev).half())
        net._ws.fill_(0xFF)
        assert torch.equal(y1, net(x.to(dev).half()))
        net.fused_scpa = 2                                              # VALU attention: the MFMA attention's score / softmax path held to it at this key count
        y2 = net(x.to(dev).half())
        net.fused_scpa = True
        e1 = (y1.float().cpu() - ref).abs()
        da = (y1.float() - y2.float()).abs().max().item()
        print(f"PAN un-tiled {shape}: vs oracle max {e1.max().item():.2e} mean {e1.mean().item():.2e}; MFMA attention vs VALU attention {da:.2e}")
        assert y1.shape == ref.shape and torch.isfinite(y1).all()
        bound = 1e-2 * max(1.0, ref.abs().max().item())
        assert e1.max().item() < bound and e1.mean().item() < 1.5e-3 and da < 2e-3, (shape, e1.max().item(), e1.mean().item(), da)
        del ref, y1, y2


def test_pan_constructor_variants_golden(dev, golden):
    """PAN(self_attention=False), PAN(double_scpa=True) and both at 2x (PAN_arch.py:115-141,193-203) against the reference (G18): same
    parameter names in the same order, outputs within the PAN tolerance."""
    import ast
    from innfer_amd import synth
    from innfer_amd.architectures.PAN_arch import PAN
    from test_oracle_golden import G18_PAN
    g = golden("g18_pan_variants")
    for i, (tag, kw) in enumerate(G18_PAN.items()):
        shapes = {str(k): ast.literal_eval(str(s)) for k, s in zip(g[tag + "_keys"], g[tag + "_shapes"])}
        net = PAN(3, 3, 40, 24, 3, **kw)
        assert list(net.state_dict()) == [str(k) for k in g[tag + "_keys"]]
        net.load_state_dict(_sd(shapes, 185 + i), strict=True)
        net = net.to(dev).eval()
        x = torch.from_numpy(synth.uniform((1, 3, 20, 28), 195 + i)).to(dev)
        ref = g[tag].astype(np.float32)
        for xin in (x.half(),):          # (float32 tensors run the engine's fp32 mode: test_gpu_fp32_mode.py)
            y = net(xin).float().cpu().numpy()
            err = np.abs(y - ref)
            assert y.shape == ref.shape and err.max() < 1e-2 * max(1.0, np.abs(ref).max()) and err.mean() < 1.5e-3, (tag, err.max(), err.mean())
    with pytest.raises(NotImplementedError):
        PAN(ups_inter_mode='bicubic')


def test_pan_scales_vs_oracle(dev):
    """scale 2 and 1 (one / no up-block, unf = nf at scale 1), grayscale, ragged sizes, 3 blocks."""
    import oracle
    from innfer_amd import synth
    from innfer_amd.architectures import get_network
    from innfer_amd.utils.defaults import get_network_G_config
    for scale, in_nc, h, w in [(2, 3, 37, 21), (1, 1, 24, 33), (4, 1, 9, 5)]:
        net = get_network(get_network_G_config({"type": "pan", "nb": 3, "in_nc": in_nc, "out_nc": in_nc}, scale))
        shapes = {k: tuple(v.shape) for k, v in net.state_dict().items()}
        sd = _sd(shapes)
        net.load_state_dict(sd, strict=True)
        net = net.to(dev)
        x = torch.from_numpy(synth.uniform((2, in_nc, h, w), 30 + scale))
        with torch.no_grad():
            ref = oracle.pan_forward(sd, x, nb=3, scale=scale).numpy()
        y = net(x.to(dev).half()).float().cpu().numpy()
        err = np.abs(y - ref)
        assert y.shape == ref.shape
        assert err.max() < 1e-2 * max(1.0, np.abs(ref).max()) and err.mean() < 1.5e-3, (scale, err.max(), err.mean())
        net._ws.fill_(0xFF)                                             # every byte read was written by this forward: NaN-poisoned workspace
        assert torch.equal(net(x.to(dev).half()).float().cpu(), torch.from_numpy(y))
    with pytest.raises(ValueError):
        net(torch.zeros(1, 1, 3, 8, device=dev, dtype=torch.float16))                        # MaxPool2d(4) needs >= 4x4


def test_small_generators_shape_fuzz_and_poisoned_workspace(dev):
    """Seeded shapes for the pix2pix UNet, the CycleGAN ResNet and the WBC UNet against the oracle: every size decides anew which levels run on the
    halo-tile kernel's stride-2 / phase-lattice / column / sub-block forms (ragged tile rows and columns, grids at most 16 wide, batches) and which on the
    gather GEMM.  Each forward is repeated on a workspace filled with 0xFF bytes (NaN as fp16 / fp32): the result must not change, i.e. every byte a
    kernel reads -- padded rings, statistics partials, split-K segments -- was written by this forward."""
    import oracle
    from innfer_amd import synth
    from innfer_amd.architectures.UNet_arch import UnetGenerator
    from innfer_amd.architectures.ResNet_arch import ResnetGenerator
    from innfer_amd.architectures import get_network
    from innfer_amd.utils.defaults import get_network_G_config
    rng = np.random.RandomState(77)

    def check(net, x, ref, tol_max, tol_mean, tag):
        y = net(x.to(dev).half()).float().cpu()
        err = (y - ref).abs()
        assert y.shape == ref.shape and err.max().item() < tol_max and err.mean().item() < tol_mean, (tag, tuple(x.shape), err.max().item(), err.mean().item())
        net._ws.fill_(0xFF)
        assert torch.equal(net(x.to(dev).half()).float().cpu(), y), (tag, tuple(x.shape), "reads unwritten workspace")

    unet = UnetGenerator(3, 3, 5, ngf=64)
    sd_u = _sd({k: tuple(v.shape) for k, v in unet.state_dict().items()}, 401)
    unet.load_state_dict(sd_u, strict=True)
    unet = unet.to(dev).train()
    for _ in range(6):
        n, h, w = int(rng.randint(1, 3)), 32 * int(rng.randint(2, 9)), 32 * int(rng.randint(2, 9))
        x = torch.from_numpy(synth.uniform((n, 3, h, w), int(rng.randint(1 << 20)), -1.0, 1.0))
        with torch.no_grad():
            ref = torch.cat([oracle.unet_forward(sd_u, x[i:i + 1], num_downs=5) for i in range(n)], 0)
        check(unet, x, ref, 3e-2, 3e-3, "unet")
    res = ResnetGenerator(3, 3, 64, norm_type="instance", n_blocks=1)
    sd_r = _sd({k: tuple(v.shape) for k, v in res.state_dict().items()}, 402)
    res.load_state_dict(sd_r, strict=True)
    res = res.to(dev).eval()
    for _ in range(6):
        n, h, w = int(rng.randint(1, 3)), 4 * int(rng.randint(4, 60)), 4 * int(rng.randint(4, 60))
        x = torch.from_numpy(synth.uniform((n, 3, h, w), int(rng.randint(1 << 20)), -1.0, 1.0))
        with torch.no_grad():
            ref = torch.cat([oracle.resnet_forward(sd_r, x[i:i + 1], n_blocks=1) for i in range(n)], 0)
        check(res, x, ref, 1e-2, 1.5e-3, "resnet")
    pp = get_network(get_network_G_config({"type": "ppon", "nb": 2}, 4))          # two residual-in-residual blocks per module: the dilated-conv launch, the
    sd_p = _sd({k: tuple(v.shape) for k, v in pp.state_dict().items()}, 405)      # running-sum operand of c2 and the three heads on ragged sizes and batches
    pp.load_state_dict(sd_p, strict=True)
    pp = pp.to(dev).eval()
    for _ in range(4):
        n, h, w = int(rng.randint(1, 4)), int(rng.randint(9, 70)), int(rng.randint(9, 70))
        x = torch.from_numpy(synth.uniform((n, 3, h, w), int(rng.randint(1 << 20))))
        with torch.no_grad():
            refs = oracle.ppon_forward(sd_p, x, nb=2, scale=4)
        outs = pp(x.to(dev).half())
        for name, y, ref in zip("csp", outs, refs):
            err = (y.float().cpu() - ref).abs()
            lim = max(1.0, ref.abs().max().item())
            assert err.max().item() < 1e-2 * lim and err.mean().item() < 2e-3 * lim, ("ppon", name, n, h, w, err.max().item(), err.mean().item())
        keep = [o.clone() for o in outs]
        pp._ws.fill_(0xFF)
        assert all(torch.equal(a, b) for a, b in zip(pp(x.to(dev).half()), keep)), ("ppon", n, h, w, "reads unwritten workspace")
    for ngf in (32, 96, 128):                            # other widths than the presets' 64: some layers leave the 64-channel tile forms
        rw = ResnetGenerator(3, 3, ngf, norm_type="instance", n_blocks=1)
        sd_n = _sd({k: tuple(v.shape) for k, v in rw.state_dict().items()}, 404 + ngf)
        rw.load_state_dict(sd_n, strict=True)
        rw = rw.to(dev).eval()
        for (h, w) in ((64, 64), (72, 104)):
            x = torch.from_numpy(synth.uniform((2, 3, h, w), 500 + ngf + h, -1.0, 1.0))
            with torch.no_grad():
                ref = torch.cat([oracle.resnet_forward(sd_n, x[i:i + 1], n_blocks=1) for i in range(2)], 0)
            check(rw, x, ref, 1e-2, 1.5e-3, f"resnet ngf {ngf}")
    for mode in ("wbcunet", "wbcunet_tf"):
        wb = get_network(get_network_G_config(mode, 1))
        sd_w = _sd({k: tuple(v.shape) for k, v in wb.state_dict().items()}, 403)
        wb.load_state_dict(sd_w, strict=True)
        wb = wb.to(dev).eval()
        for _ in range(3):
            n, h, w = int(rng.randint(1, 3)), 4 * int(rng.randint(4, 50)), 4 * int(rng.randint(4, 50))
            x = torch.from_numpy(synth.uniform((n, 3, h, w), int(rng.randint(1 << 20)), -1.0, 1.0))
            with torch.no_grad():
                ref = oracle.wbcunet_forward(sd_w, x, mode="tf" if mode.endswith("tf") else "pt")
            check(wb, x, ref, 8e-3, 1e-3, mode)


def test_pan_fused_tail_vs_two_launches(dev):
    """Round 5: the last stage's HRconv carries conv_last in its epilogue (conv3x3_pc FUSE on the 32-channel kernel, 16-row tiles) wherever the full-resolution grid is whole
    16 x 32 tiles; `fused_scpa = 4` runs the two launches.  Same fp16 HR values, conv_last summed in another order: agreement to the last rounding of the fp16 output, batches
    and 2x / 4x; a ragged grid takes the two-launch form in both settings (bit-equal); the fused form is poison-proof (its rim buffer lives in the unwritten HR slab)."""
    from innfer_amd import synth
    from innfer_amd.architectures import get_network
    from innfer_amd.utils.defaults import get_network_G_config
    for scale, shapes in ((4, [(1, 3, 48, 48), (2, 3, 24, 40), (3, 3, 200, 200), (1, 3, 50, 70)]), (2, [(2, 3, 32, 48), (1, 3, 33, 48)])):
        net = get_network(get_network_G_config({"type": "pan", "nb": 2}, scale))
        net.load_state_dict(_sd({k: tuple(v.shape) for k, v in net.state_dict().items()}, 700 + scale), strict=True)
        net = net.to(dev).eval()
        for shape in shapes:
            x = torch.from_numpy(synth.uniform(shape, 710 + shape[2])).to(dev).half()
            net.fused_scpa = True
            yf = net(x)
            net._ws.fill_(0xFF)
            assert torch.equal(net(x), yf), (scale, shape, "the fused tail reads unwritten workspace")
            net.fused_scpa = 4
            y2 = net(x)
            net.fused_scpa = True
            whole = (shape[2] * scale) % 16 == 0 and (shape[3] * scale) % 32 == 0
            if whole:
                _assert_same_to_the_last_rounding(yf, y2, (scale, shape))
            else:
                assert torch.equal(yf, y2), (scale, shape)
            assert torch.isfinite(yf.float()).all()


def test_sr_network_options_shape_fuzz_and_poisoned_workspace(dev):
    """Seeded ragged shapes and batches for the SR shells' graph-changing options against the oracle: SRResNet's own defaults (BatchNorm, 'NAC': the
    input map in front of every block and of LR_conv), RRDBNet(norm_type='batch', mode='NAC'), the PixelShuffle(3) stage and PixelShuffle(2) on 32
    features (conv to a slab + gather pass), upscale 3 with 'upconv'.  Each forward is repeated on a workspace of 0xFF bytes: the result must not change."""
    import oracle
    from innfer_amd import synth
    from innfer_amd.architectures.RRDBNet_arch import RRDBNet
    from innfer_amd.architectures.SRResNet_arch import SRResNet
    rng = np.random.RandomState(91)

    def np_sd(shapes, seed, bn):
        sd = synth.fill_state_dict(shapes, seed)
        return {k: torch.from_numpy(np.asarray(v)) for k, v in (synth.fill_running_stats(sd, seed) if bn else sd).items()}

    cases = [
        ("sr nac bn", SRResNet(3, 3, 64, 3), True,
         lambda sd, x: oracle.srresnet_forward(sd, x, nb=3, scale=4, upsample_mode="upconv", norm_type="batch", mode="NAC")),
        ("sr nac lrelu x2", SRResNet(3, 3, 64, 2, upscale=2, norm_type=None, act_type="leakyrelu", res_scale=0.5), False,
         lambda sd, x: oracle.srresnet_forward(sd, x, nb=2, scale=2, act_type="leakyrelu", res_scale=0.5, upsample_mode="upconv", mode="NAC")),
        ("sr ps3", SRResNet(3, 3, 64, 2, upscale=3, norm_type=None, mode="CNA", upsample_mode="pixelshuffle"), False,
         lambda sd, x: oracle.srresnet_forward(sd, x, nb=2, scale=3, upsample_mode="pixelshuffle")),
        ("sr nf32 ps2", SRResNet(3, 3, 32, 2, upscale=2, norm_type=None, mode="CNA", upsample_mode="pixelshuffle"), False,
         lambda sd, x: oracle.srresnet_forward(sd, x, nb=2, scale=2, upsample_mode="pixelshuffle")),
        ("sr x3 upconv", SRResNet(3, 3, 64, 2, upscale=3, norm_type=None, mode="CNA"), False,
         lambda sd, x: oracle.srresnet_forward(sd, x, nb=2, scale=3, upsample_mode="upconv")),
        ("rrdb bn nac", RRDBNet(3, 3, 64, 1, upscale=2, norm_type="batch", mode="NAC"), True,
         lambda sd, x: oracle.rrdbnet_forward(sd, x, nb=1, scale=2)),
        ("rrdb ps3", RRDBNet(3, 3, 64, 1, upscale=3, upsample_mode="pixelshuffle"), False,
         lambda sd, x: oracle.rrdbnet_forward(sd, x, nb=1, scale=3, upsample_mode="pixelshuffle")),
    ]
    for j, (tag, net, bn, fwd) in enumerate(cases):
        sd = np_sd({k: tuple(v.shape) for k, v in net.state_dict().items()}, 600 + j, bn)
        net.load_state_dict(sd, strict=True)
        net = net.to(dev).eval()
        for _ in range(3):
            n, h, w = int(rng.randint(1, 4)), int(rng.randint(5, 75)), int(rng.randint(5, 75))
            x = torch.from_numpy(synth.uniform((n, 3, h, w), int(rng.randint(1 << 20))))
            with torch.no_grad():
                ref = fwd(sd, x)
            y = net(x.to(dev).half()).float().cpu()
            err = (y - ref).abs()
            lim = max(1.0, ref.abs().max().item())
            assert y.shape == ref.shape and err.max().item() < 5e-3 * lim, (tag, n, h, w, err.max().item())
            net._ws.fill_(0xFF)
            assert torch.equal(net(x.to(dev).half()).float().cpu(), y), (tag, n, h, w, "reads unwritten workspace")


# ---------------------------------------------------------- tiles / blend / io
def test_extract_and_blend_bit_exact(dev, golden):
    import oracle
    from innfer_amd import synth
    from innfer_amd.utils import utils as U
    g = golden("g2_blend")
    for scale in (1, 2, 4):
        h, w = 250, 330
        x = torch.from_numpy(synth.uniform((1, 3, h, w), 100 + scale))
        tiles = U.extract_patches_2d(x.to(dev), (200, 200), [0.5, 0.5], batch_first=True).squeeze(0)
        assert torch.equal(tiles.cpu(), oracle.extract_patches_2d(x, (200, 200), [0.5, 0.5], batch_first=True).squeeze(0))
        up = F.interpolate(tiles, scale_factor=float(scale), mode="nearest") if scale > 1 else tiles
        k = torch.arange(up.shape[0], dtype=torch.float32, device=dev)[:, None, None, None]
        r = U.recompose_tensor(up * (1.0 + k / 16.0), h, w, step=0.5, scale=scale).cpu()
        assert np.array_equal(r[0, :, ::7, ::5].numpy(), g[f"blend_s{scale}_sub"])
        assert r.double().sum().item() == g[f"blend_s{scale}_sum"]
    x = torch.from_numpy(synth.uniform((1, 3, 150, 250), 77))
    p = U.extract_patches_2d(x.to(dev), (150, 150), [0.5, 0.5], batch_first=True).squeeze(0)
    k = torch.arange(p.shape[0], dtype=torch.float32, device=dev)[:, None, None, None]
    r = U.recompose_tensor(p * (1.0 + k / 16.0), 150, 250, step=0.5, scale=1).cpu()
    assert np.array_equal(r[0].numpy(), g["blend_150x250"])
    # odd small patch: the reference raises (torch.ones(negative)); so do we
    with pytest.raises(ValueError):
        U.recompose_tensor(torch.zeros(2, 3, 151, 151, device=dev), 151, 250, step=0.5, scale=1)


def test_blend_identity_at_full_size(dev):
    """Size-independent property at the 8K-input tile count (3268 tiles of 200x200, scale 1):
    recompose(extract(x)) == x up to fp32 rounding: out = (sum_k w_k x) / (sum_k w_k) over the <= 4 tiles that cover a pixel -- one rounding per product, per
    addition of either sum and for the quotient: <= 8 half-ulps of a value below 1 = 8 * 2^-24 = 4.8e-7 (seeded input: with fresh random data the maximum over
    100 M values moved between 3.0e-7 and 3.6e-7 from run to run, around the old 3e-7 bound)."""
    from innfer_amd.utils import utils as U
    h, w = 4320, 7680
    x = torch.rand((1, 3, h, w), device=dev, generator=torch.Generator(device=dev).manual_seed(1234))
    tiles = U.extract_patches_2d(x, (200, 200), [0.5, 0.5], batch_first=True).squeeze(0)
    assert tiles.shape[0] == 3268
    r = U.recompose_tensor(tiles, h, w, step=0.5, scale=1)
    assert (r - x).abs().max().item() <= 4.8e-7


def test_pre_post_bit_exact(dev, golden):
    from innfer_amd import synth
    from innfer_amd.utils import utils as U
    g = golden("g9_convert")
    assert np.array_equal(U.np2tensor(g["ramp"]).cpu().numpy(), g["np2t"])
    assert np.array_equal(U.np2tensor(g["ramp"], normalize=True).cpu().numpy(), g["np2t_norm"])
    th = torch.from_numpy(g["t2np_in"]).to(dev)
    assert np.array_equal(U.tensor2np(th), g["t2np"])
    assert np.array_equal(U.tensor2np(th * 2 - 1, denormalize=True), g["t2np_denorm"])
    assert np.array_equal(U.tensor2np(torch.from_numpy(g["big_in"]).to(dev)), g["big_u8"])
    img = synth.image_u8(270, 481, 3, 5)
    assert np.array_equal(U.tensor2np(U.np2tensor(img)), img)               # exact uint8 round trip
    assert np.array_equal(U.tensor2np(U.np2tensor(img, dtype=torch.float16)), img)
    img4 = synth.image_u8(17, 9, 4, 6)
    t4 = U.np2tensor(img4).cpu().numpy()[0]
    assert np.array_equal(t4, (img4.astype(np.float32) / 255).transpose(2, 0, 1)[[2, 1, 0, 3]])


def test_pre_post_uint16_and_flags_bit_exact(dev, golden):
    """np2tensor / tensor2np with uint16 images (maxval 65535, utils.py:22-33) and the non-default flags (bgr2rgb / rgb2bgr off, add_batch
    off, change_range off, 3-D / 2-D tensors) against the reference (golden G19): bit-exact, like the uint8 defaults."""
    from innfer_amd.utils import utils as U
    from test_oracle_golden import _convert_flag_cases
    g = golden("g19_convert_flags")
    for name, got, want in _convert_flag_cases(g, U.np2tensor, U.tensor2np, to_t=lambda a: torch.from_numpy(a).to(dev)):
        got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
        assert got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want), name
    img16 = (np.arange(64 * 48 * 3, dtype=np.uint32) * 2654435761 % 65536).astype(np.uint16).reshape(64, 48, 3)
    assert np.array_equal(U.tensor2np(U.np2tensor(img16), data_range=65535, imtype=np.uint16), img16)      # exact uint16 round trip (fp32)
    with pytest.raises(NotImplementedError):
        U.np2tensor(img16.astype(np.float32))


def test_srgb_helpers(dev, golden):
    """colors.py srgb2linear / linear2srgb.  powf differs from numpy's by an ulp or so: float results
    within 2e-6; the truncating uint8 cast may flip one code exactly at a boundary."""
    from innfer_amd.utils import colors as Cc
    g = golden("g9_convert")
    lin = Cc.srgb2linear(np.arange(256, dtype=np.uint8))
    assert lin.dtype == np.float32 and np.abs(lin - g["srgb2linear"]).max() < 2e-6
    back = Cc.linear2srgb(np.linspace(-0.1, 1.1, 1001, dtype=np.float32))
    d = np.abs(back.astype(int) - g["linear2srgb"].astype(int))
    assert d.max() <= 1 and (d != 0).mean() < 0.005
    img = np.arange(256, dtype=np.uint8).reshape(16, 16)
    rt = Cc.linear2srgb(Cc.srgb2linear(img))
    assert np.abs(rt.astype(int) - img.astype(int)).max() <= 1


def test_esrgan_lite_and_gray_shapes(dev):
    """nf=32 (esrgan-lite, defaults.py:25-27) and 1-channel models run through the same kernels."""
    import oracle
    from innfer_amd import synth
    from innfer_amd.architectures.RRDBNet_arch import RRDBNet
    for (in_nc, out_nc, nf, nb, scale) in [(3, 3, 32, 2, 4), (1, 1, 64, 1, 2), (4, 4, 64, 1, 1)]:
        sd = _sd(synth.rrdbnet_shapes(in_nc=in_nc, out_nc=out_nc, nf=nf, nb=nb, scale=scale))
        net = RRDBNet(in_nc, out_nc, nf, nb, upscale=scale)
        net.load_state_dict(sd, strict=True)
        net = net.to(dev).eval()
        x = torch.from_numpy(synth.uniform((2, in_nc, 29, 41), 50 + nf))
        y = net(x.to(dev).half()).float().cpu()
        with torch.no_grad():
            ref = oracle.rrdbnet_forward(sd, x, nb=nb, scale=scale)
        assert (y - ref).abs().max().item() < 1e-2, (in_nc, nf, scale)


def test_first_conv_on_the_matrix_cores_all_widths(dev):
    """first_conv_mfma<NT, STEPS>: 1..8 input channels (one, two or three 32-deep k steps of 9 * in_nc taps), nf 32 / 64, fp16 and fp32 input,
    ragged and one-pixel images -- through a one-block RRDBNet against the oracle.  With fp32 input the split fp16 operands must keep the first
    conv at fp32 accuracy: fp32-in and fp16-in forwards of the same fp16-representable image agree bit for bit."""
    import oracle
    from innfer_amd import synth
    from innfer_amd.architectures.RRDBNet_arch import RRDBNet
    for in_nc in (1, 2, 3, 4, 5, 7, 8):
        for nf in (32, 64):
            sd = _sd(synth.rrdbnet_shapes(in_nc=in_nc, out_nc=3, nf=nf, nb=1, scale=1), 300 + in_nc)
            net = RRDBNet(in_nc, 3, nf, 1, upscale=1)
            net.load_state_dict(sd, strict=True)
            net = net.to(dev).eval()
            for shape in ((1, in_nc, 17, 23), (2, in_nc, 1, 1), (1, in_nc, 33, 16)):
                x = torch.from_numpy(synth.uniform(shape, 310 + in_nc)).half()
                with torch.no_grad():
                    ref = oracle.rrdbnet_forward(sd, x.float(), nb=1, scale=1)
                y16 = net(x.to(dev)).float().cpu()
                y32 = net(x.float().to(dev)).float().cpu()
                assert (y16 - ref).abs().max().item() < 5e-3, (in_nc, nf, shape)
                assert (y32 - ref).abs().max().item() < 1e-4, (in_nc, nf, shape)      # a float32 tensor runs the fp32-accurate engine (test_gpu_fp32_mode.py)


# ---------------------------------------------------------------- Model / chop
def test_forward_into_callers_tensor(dev):
    """forward(x, out=...): the last conv writes the caller's tensor -- same bits as a fresh result, for an engine of each base class and
    for a row range of a larger buffer (how chop batches land in the tile buffer); a wrong shape / dtype / a strided view is refused."""
    from innfer_amd import synth
    from innfer_amd.architectures import get_network
    from innfer_amd.architectures.RRDBNet_arch import RRDBNet
    from innfer_amd.utils.defaults import get_network_G_config
    net = RRDBNet(3, 3, 64, 1, upscale=2)
    net.load_state_dict(_sd(synth.rrdbnet_shapes(nb=1, scale=2), 7), strict=True)
    pan = get_network(get_network_G_config({"type": "pan", "nb": 2}, 4))
    pan.load_state_dict(_sd({k: tuple(v.shape) for k, v in pan.state_dict().items()}, 8), strict=True)
    for m, s in ((net.to(dev).eval(), 2), (pan.to(dev).eval(), 4)):
        x = torch.from_numpy(synth.uniform((3, 3, 40, 56), 9)).to(dev).half()
        ref = m(x)
        buf = torch.full((5, 3, 40 * s, 56 * s), float("nan"), dtype=torch.float16, device=dev)
        y = m(x, out=buf[1:4])
        assert y.data_ptr() == buf[1:4].data_ptr() and torch.equal(buf[1:4], ref)
        assert torch.isnan(buf[0]).all() and torch.isnan(buf[4]).all()                      # nothing outside the rows it was given
        for bad in (torch.empty((3, 3, 40 * s, 56 * s + 1), dtype=torch.float16, device=dev), torch.empty((3, 3, 40 * s, 56 * s), dtype=torch.float32, device=dev),
                    torch.empty((3, 3, 40 * s, 2 * 56 * s), dtype=torch.float16, device=dev)[..., ::2]):
            with pytest.raises(ValueError):
                m(x, out=bad)


def test_model_chop_golden(dev, golden, tmp_path):
    from innfer_amd import synth
    from innfer_amd.run import Model
    g = golden("g4_chop")
    for (nb, scale, h, w, tag) in [(2, 4, 250, 330, "x4_250x330"), (1, 2, 201, 640, "x2_201x640"),
                                   (1, 1, 150, 250, "x1_150x250")]:
        sd = _sd(synth.rrdbnet_shapes(nb=nb, scale=scale))
        path = str(tmp_path / f"{scale}x_{tag}.pth")
        torch.save(sd, path)
        m = Model(path, arch="infer", scale=None, device="cuda", chop=True, tile_batch=4)
        assert (m.arch, m.scale) == ("esrgan", scale)
        x = torch.from_numpy(synth.uniform((1, 3, h, w), 40 + scale)).to(dev).half()
        y = m(x).float().cpu()
        assert tuple(y.shape) == (1, 3, h * scale, w * scale)
        assert np.abs(y[0, :, ::8, ::8].numpy() - g[f"chop_{tag}_sub"]).max() < 1e-2
        assert np.abs(y[0, :, -32:, -32:].numpy() - g[f"chop_{tag}_crop_b"]).max() < 1e-2
        assert _codes_within_one(dev, y[:, :, ::8, ::8].numpy(), g[f"chop_{tag}_sub"][None]) >= 0.99
        assert _codes_within_one(dev, y[:, :, -32:, -32:].numpy(), g[f"chop_{tag}_crop_b"][None]) >= 0.99
        m2 = Model(path, arch="infer", device="cuda", chop=False)
        y2 = m2(x).float().cpu()
        assert np.abs(y2[0, :, ::8, ::8].numpy() - g[f"nochop_{tag}_sub"]).max() < 1e-2


def test_model_chop_16x_batches_follow_the_workspace(dev):
    """a 16x RRDBNet needs 2.9 GB of workspace per 200 x 200 tile (innfer_net_workspace_bytes: 770 GiB for 266 tiles), so the chop
    batches must follow the engine's workspace and the free memory instead of the 272-tile ceiling sized for 4x.  A 1000 x 1100 image (90 tiles)
    through Model(chop=True): the automatic batches fit, and the blend equals the one of batch-1 launches bit for bit."""
    from innfer_amd import synth
    from innfer_amd.parallel import MAX_TILE_BATCH, engine_tile_cap, free_device_bytes
    from innfer_amd.run import Model
    sd = _sd(synth.rrdbnet_shapes(nb=1, scale=16), 161)
    m = Model(None, arch="infer", device="cuda", chop=True, state_dict=dict(sd))
    assert (m.arch, m.scale) == ("esrgan", 16)
    cap = engine_tile_cap(m.model, 200, torch.float16, dev)
    need = m.model.tile_batch_bytes(cap, 200, torch.float16)
    assert 1 <= cap < MAX_TILE_BATCH and need <= 0.8 * free_device_bytes(dev) + 1, (cap, need)
    assert m.model.tile_batch_bytes(MAX_TILE_BATCH, 200, torch.float16) > 700 * 2 ** 30
    x = torch.from_numpy(synth.uniform((1, 3, 300, 500), 162)).to(dev).half()          # 2 x 4 tiles: 4800 x 8000 output
    y = m(x)
    assert tuple(y.shape) == (1, 3, 4800, 8000) and torch.isfinite(y).all()
    m1 = Model(None, arch="infer", device="cuda", chop=True, tile_batch=1, state_dict=dict(sd))
    assert torch.equal(m1(x), y)
    del y
    m.model.release_workspace(); m1.model.release_workspace()
    torch.cuda.empty_cache()
    # an allocator out-of-memory inside a launch halves the batch instead of ending the image: a budget-blind fixed batch of 90 tiles (260 GiB of
    # workspace) with only ~100 GiB left free by a ballast tensor -> 90 fails, 45 fails (130 GiB), 22 runs
    big = torch.from_numpy(synth.uniform((1, 3, 1000, 1100), 163)).to(dev).half()      # 9 x 10 = 90 tiles
    from innfer_amd.parallel import run_tile_batches
    from innfer_amd.utils import utils as U
    tiles = U.extract_patches_2d(big, (200, 200), [0.5, 0.5], batch_first=True).squeeze(0)
    seen, hr, ballast = [], None, None
    orig = m.model.forward
    def spy(t, *a, **k):
        seen.append(t.shape[0])
        return orig(t, *a, **k)
    m.model.forward = spy
    try:
        ballast = torch.empty(max(0, free_device_bytes(dev) - 100 * 2 ** 30), dtype=torch.uint8, device=dev)
        with torch.no_grad():
            hr = run_tile_batches(m.model, tiles, tile_batch=MAX_TILE_BATCH)
        assert seen[:2] == [90, 45] and sum(seen[2:]) == 90 and max(seen[2:]) <= 22, seen          # (the remaining tiles go in evenly sized launches)
        assert tuple(hr.shape) == (90, 3, 3200, 3200)
        m.model.forward = orig
        assert torch.equal(hr[89:90], m.model(tiles[89:90]))
    finally:
        m.model.forward = orig
        del hr, tiles, ballast
        m.model.release_workspace()
        torch.cuda.empty_cache()


def test_model_chop_pan_vs_oracle(dev, tmp_path):
    """A PAN checkpoint through Model.__call__(chop=True): loader inference (arch / scale from the keys), tile batches through the
    halo-tile convs, blend -- against the oracle's chop_forward of the oracle's PAN on a 210x250 image (4 tiles)."""
    import oracle
    from innfer_amd import synth
    from innfer_amd.architectures import get_network
    from innfer_amd.run import Model
    from innfer_amd.utils.defaults import get_network_G_config
    shapes = {k: tuple(v.shape) for k, v in get_network(get_network_G_config("pan", 4)).state_dict().items()}
    sd = _sd(shapes, 51)
    path = str(tmp_path / "4x_pan.pth")
    torch.save(sd, path)
    m = Model(path, arch="infer", scale=None, device="cuda", chop=True, tile_batch=3)
    assert (m.arch, m.scale) == ("pan", 4)
    x = torch.from_numpy(synth.uniform((1, 3, 210, 250), 52))
    y = m(x.to(dev).half()).float().cpu()
    with torch.no_grad():
        ref = oracle.chop_forward(lambda t: oracle.pan_forward(sd, t, nb=16, scale=4), x, 4)
    assert tuple(y.shape) == tuple(ref.shape) == (1, 3, 840, 1000)
    err = (y - ref).abs()
    assert err.max().item() < 1e-2 and err.mean().item() < 1.5e-3, (err.max().item(), err.mean().item())


def _assert_same_to_the_last_rounding(a, b, what=""):
    """Two fp16 results whose fp32 values were summed in a different order: equal up to one unit in the last place of the larger magnitude -- or, where
    the sum cancels to almost nothing, up to the fp32 noise of adding 576 products in another order (4e-6) -- and on all but a few per cent of the values
    bit for bit."""
    af, bf = a.float(), b.float()
    d = (af - bf).abs()
    mag = torch.maximum(af.abs(), bf.abs()).clamp_min(2.0 ** -14)
    ulp = torch.exp2(torch.floor(torch.log2(mag)) - 10).clamp_min(4e-6)
    assert bool((d <= ulp * 1.001).all()), (what, (d / ulp).max().item())
    assert (d > 0).float().mean().item() < 0.05, (what, (d > 0).float().mean().item())


def test_residual_from_lds_network_level(dev):
    """innfer_net_set_residual_lds (default on): the whole RRDBNet with the dense blocks' residual taken from LDS against the epilogue-load schedule and the
    oracle -- a single image, a batch on the image canvas, a ragged frame; both schedules inside the oracle bound (<= 1e-2), within 2e-3 of each other (the two
    sums differ in the last fp32 bit per block; 2 x 3 dense blocks and the up-convs carry that to a few fp16 ulps), and each schedule deterministic."""
    import oracle
    from innfer_amd import synth
    net, sd = _rrdb(dev, 2, 4, seed=5)
    for i, shape in enumerate([(1, 3, 40, 56), (3, 3, 33, 47), (1, 3, 16, 32)]):
        x = torch.from_numpy(synth.uniform(shape, 60 + i))
        with torch.no_grad():
            ref = oracle.rrdbnet_forward(sd, x, nb=2, scale=4)
        ys = {}
        for mode in (2, 1, 0):                  # every dense block / the RRDB-end blocks (the default) / epilogue loads
            net.residual_lds = mode
            ys[mode] = net(x.to(dev).half())
            assert torch.equal(ys[mode], net(x.to(dev).half()))
            if shape[0] > 1:                    # a batch equals its images' own forwards bit for bit (canvas form of the same kernel)
                assert torch.equal(ys[mode][1:2], net(x[1:2].to(dev).half()))
        net.residual_lds = 1
        e = {m: (y.float().cpu() - ref).abs().max().item() for m, y in ys.items()}
        d = max((ys[2].float() - ys[0].float()).abs().max().item(), (ys[1].float() - ys[0].float()).abs().max().item())
        print(f"residual from LDS {shape}: vs oracle {e[2]:.2e} / {e[1]:.2e} (epilogue loads: {e[0]:.2e}), between the schedules {d:.2e}")
        assert max(e.values()) < 1e-2 and d < 2e-3, (shape, e, d)


def test_fused_tail_vs_two_launches_and_oracle(dev):
    """HR_conv0 -> conv_last as one kernel (conv3x3_pc<.., TMF | 0x20000>, innfer_net_set_fused_tail, the default) against the two-launch schedule and the
    oracle: HR frames of 1 x 1 ... 4 x 3 tiles of 16 x 32 pixels (tiles with neighbours on every side, rims on the frame border), batches, a scale-2
    net, ReLU features, one grey output channel, the uint8 image form; frames that are NOT whole tiles take the two launches and must be bit-identical
    with the knob on or off."""
    import oracle
    from innfer_amd import synth
    from innfer_amd.architectures.RRDBNet_arch import RRDBNet
    cases = [(4, 3, "leakyrelu", (1, 3, 4, 8)), (4, 3, "leakyrelu", (1, 3, 12, 24)), (4, 3, "leakyrelu", (3, 3, 16, 24)), (2, 3, "leakyrelu", (2, 3, 24, 32)),
             (4, 3, "relu", (1, 3, 8, 16)), (4, 1, "leakyrelu", (2, 1, 12, 16)), (4, 3, "leakyrelu", (1, 3, 200, 200))]
    for i, (scale, nc, act, shape) in enumerate(cases):
        shapes = synth.rrdbnet_shapes(nb=1, scale=scale, in_nc=nc, out_nc=nc) if nc != 3 else synth.rrdbnet_shapes(nb=1, scale=scale)
        sd = _sd(shapes, 70 + i)
        net = RRDBNet(nc, nc, 64, 1, upscale=scale, act_type=act)
        net.load_state_dict(sd, strict=True)
        net = net.to(dev).eval()
        x = torch.from_numpy(synth.uniform(shape, 700 + i)).to(dev).half()
        yf = net(x)
        net.fused_tail = False
        y2 = net(x)
        _assert_same_to_the_last_rounding(yf, y2, ("fused vs two launches", scale, nc, act, shape))
        net.fused_tail = True
        if i in (1, 2, 5):
            with torch.no_grad():
                ref = oracle.rrdbnet_forward(sd, x.float().cpu(), nb=1, scale=scale) if act == "leakyrelu" and nc == 3 else None
            if ref is not None:
                e = (yf.float().cpu() - ref).abs()
                assert e.max().item() < 1e-2 and e.mean().item() < 1e-3, (shape, e.max().item(), e.mean().item())
    # the uint8 image form (forward_u8: np2tensor in the first conv, tensor2np as the fused tail's store): exactly tensor2np of the tensor forward with the
    # fused tail on both sides (same sums, the fp16 rounding emulated in front of the uint8 conversion), and within one code of the two-launch form
    from innfer_amd.utils import utils as U
    net, _ = _rrdb(dev, 1, 4)
    for normalize in (False, True):
        img = torch.from_numpy(synth.image_u8(16, 24, 3, 5)).to(dev)
        got = net.forward_u8(img, normalize=normalize)
        want = U.tensor2np(net(U.np2tensor(img.cpu().numpy(), normalize=normalize, dtype=torch.float16).to(dev)), denormalize=normalize)
        assert np.array_equal(got.cpu().numpy(), want), normalize
        net.fused_tail = False
        two = net.forward_u8(img, normalize=normalize)
        net.fused_tail = True
        dd = (got.int() - two.int()).abs()
        assert dd.max().item() <= 1 and (dd > 0).float().mean().item() < 0.005, (normalize, dd.max().item(), (dd > 0).float().mean().item())
    # through the C ABI: fp16 engine, fp16 input, FLOAT32 output tensor (the fused tail's planar fp32 store): the fp16 result is its rounding
    import innfer_amd.lib as L
    x = torch.from_numpy(synth.uniform((2, 3, 8, 16), 11)).to(dev).half()
    y16 = net(x)
    y32 = torch.empty(y16.shape, dtype=torch.float32, device=dev)
    L.check(L.lib.innfer_net_set_precision(net._handle, 0))
    L.check(L.lib.innfer_net_forward(net._handle, x.data_ptr(), L.F16, y32.data_ptr(), L.F32, 2, 8, 16, net._ws.data_ptr(), net._ws.numel(),
                                     torch.cuda.current_stream(dev).cuda_stream))
    torch.cuda.synchronize()
    assert torch.equal(y32.half(), y16)
    # not whole tiles (HR 40 x 72): the knob changes nothing
    net, _ = _rrdb(dev, 1, 4)
    x = torch.from_numpy(synth.uniform((2, 3, 10, 18), 9)).to(dev).half()
    ya = net(x)
    net.fused_tail = False
    assert torch.equal(ya, net(x))


def test_upconv_phases_vs_nine_taps_and_oracle(dev):
    """upconv_block (nearest 2x -> conv 3x3 -> act, block.py:348-361) as the four 2x2-tap phases of the equivalent transposed conv (innfer_net_set_upconv_phases,
    the default) against the nine-tap form through the upsampling loader and against the oracle: the same linear map, the summed taps rounded to fp16 once
    instead of tap by tap -- both within the fp16 bound of the oracle, and within 4e-3 of each other; scale 4 (two stages) and 2, batches, ragged sizes,
    grids at most 16 pixels wide (image pairs), ReLU features."""
    import oracle
    from innfer_amd import synth
    from innfer_amd.architectures.RRDBNet_arch import RRDBNet
    for i, (scale, act, shape) in enumerate([(4, "leakyrelu", (1, 3, 24, 40)), (4, "leakyrelu", (3, 3, 7, 13)), (2, "leakyrelu", (2, 3, 33, 65)), (4, "relu", (1, 3, 16, 16)), (4, "leakyrelu", (2, 3, 70, 100)),
                                              (4, "relu", (1, 3, 256, 384))]):       # (the last: 768 tiles in the second stage -- three per workgroup, every state of the slot rotation)
        sd = _sd(synth.rrdbnet_shapes(nb=1, scale=scale), 90 + i)
        net = RRDBNet(3, 3, 64, 1, upscale=scale, act_type=act)
        net.load_state_dict(sd, strict=True)
        net = net.to(dev).eval()
        x = torch.from_numpy(synth.uniform(shape, 950 + i)).to(dev).half()
        yp = net(x)
        net.upconv_phases = 2            # one phase per visit of a tile (round 3's form): the same MFMAs on the same operands in the same order
        assert torch.equal(net(x), yp), (scale, act, shape, "four phases in one visit != one phase per visit")
        net.upconv_phases = False
        y9 = net(x)
        net.upconv_phases = True
        assert yp.shape == y9.shape and (yp.float() - y9.float()).abs().max().item() < 4e-3, (scale, act, shape, (yp.float() - y9.float()).abs().max().item())
        if act == "leakyrelu":
            with torch.no_grad():
                ref = oracle.rrdbnet_forward(sd, x.float().cpu(), nb=1, scale=scale)
            for tag, y in (("phases", yp), ("nine taps", y9)):
                e = (y.float().cpu() - ref).abs()
                assert e.max().item() < 1e-2 and e.mean().item() < 1e-3, (tag, scale, shape, e.max().item(), e.mean().item())


def test_hr_chain_equals_the_launches_it_replaces(dev):
    """The last upconv_block -> HR_conv0 -> conv_last as ONE kernel chained through LDS (csrc/hr_chain.hip, innfer_net_set_hr_chain; RRDBNet_arch.py:31-42,
    block.py:348-361) against the two launches it replaces (one-visit up-conv + fused HR_conv0 / conv_last): every value sees the same fp16 operands in the same MFMA
    order, so the results must be EQUAL bit for bit -- frames of whole 16 x 32 HR tiles: all-border tiles, interior tiles, batches, a 200 x 200 chop tile, 2x and 4x
    networks, ReLU trunks, fp16 and uint8 boundaries; and against the oracle."""
    import oracle
    from innfer_amd import synth
    from innfer_amd.architectures.RRDBNet_arch import RRDBNet
    cases = [(4, 1, 8, 16, "leakyrelu"), (4, 1, 24, 40, "leakyrelu"), (4, 2, 28, 56, "leakyrelu"), (2, 1, 48, 80, "leakyrelu"), (2, 3, 24, 32, "relu"),
             (4, 1, 200, 200, "leakyrelu"), (4, 1, 36, 104, "relu"), (8, 1, 12, 24, "leakyrelu"), (4, 1, 272, 480, "leakyrelu"), (4, 5, 200, 200, "leakyrelu")]
    # (the last two: 4080 / 6250 tiles = 16 / 25 per persistent workgroup, both traversal directions: the LR-tile / weight-ring hand-over between tiles)
    for i, (scale, n, h, w, act) in enumerate(cases):
        sd = _sd(synth.rrdbnet_shapes(nb=1, scale=scale), 300 + i)
        net = RRDBNet(3, 3, 64, 1, upscale=scale, act_type=act)
        net.load_state_dict(sd, strict=True)
        net = net.to(dev).eval()
        x = torch.from_numpy(synth.uniform((n, 3, h, w), 310 + i)).to(dev).half()
        net.hr_chain = True
        y1 = net(x)
        net._ws.fill_(0xFF)                        # (poisoned workspace: the chained kernel must not read the HR slab it no longer writes)
        y1b = net(x)
        net.hr_chain = False
        y0 = net(x)
        assert torch.equal(y1, y0), (scale, n, h, w, act, (y1.float() - y0.float()).abs().max().item())
        assert torch.equal(y1, y1b), (scale, n, h, w, act, "poisoned workspace")
        if i in (1, 4):
            with torch.no_grad():
                ref = oracle.rrdbnet_forward(sd, x.float().cpu(), nb=1, scale=scale, act_type=act)
            assert (y1.float().cpu() - ref).abs().max().item() < 1e-2, (scale, n, h, w)
        if i in (1, 5):                            # uint8 in, uint8 out (np2tensor / tensor2np fused at both ends)
            img = torch.from_numpy((synth.uniform((h, w, 3), 320 + i) * 255).astype(np.uint8)).to(dev)
            net.hr_chain = True
            u1 = net.forward_u8(img)
            net.hr_chain = False
            assert torch.equal(u1, net.forward_u8(img)), (scale, n, h, w, "u8")


def test_full_frame_1080p_translation_property(dev):
    """BASELINE config 2 size (1x3x1080x1920 -> 1x3x4320x7680, RRDBNet-23 4x fp16): an
    interior window of the full-frame result equals the forward of a crop that
    contains the window plus the network's receptive radius (stride-1 convs are
    translation equivariant).  Also: banded schedule == plain schedule at full size."""
    from innfer_amd import synth
    net, sd = _rrdb(dev, 23, 4)
    x = torch.from_numpy(synth.uniform((1, 3, 1080, 1920), 31)).to(dev).half()
    yf = net(x)                       # HR_conv0 -> conv_last fused (the default; 4320 x 7680 is whole 16 x 32 tiles)
    net.fused_tail = False            # the bit-for-bit properties below belong to the two-launch schedule: the fused tail sums a rim pixel in another order
    y = net(x)
    _assert_same_to_the_last_rounding(yf, y, "fused tail vs two launches, 1080p frame")
    corners16 = {"top-left": yf[:, :, :128, :128].float().cpu(), "bottom-right": yf[:, :, -128:, -128:].float().cpu()}   # the DEFAULT path's values
    del yf
    assert tuple(y.shape) == (1, 3, 4320, 7680)
    assert torch.isfinite(y).all()
    R = 23 * 15 + 6                                   # 3x3 convs on the LR grid: 1 + 345 + 1 (+2 HR-side, <1 LR px each)
    cy, cx, hw = 540, 960, 16
    y0, y1, x0, x1 = cy - hw - R, cy + hw + R, cx - hw - R, cx + hw + R
    yc = net(x[:, :, y0:y1, x0:x1].contiguous())
    a = y[:, :, 4 * (cy - hw):4 * (cy + hw), 4 * (cx - hw):4 * (cx + hw)]
    b = yc[:, :, 4 * (cy - hw - y0):4 * (cy + hw - y0), 4 * (cx - hw - x0):4 * (cx + hw - x0)]
    assert torch.equal(a, b)
    net.band_rows = 128
    assert torch.equal(net(x), y)
    net.band_rows = 0
    net.fused_tail = True
    # ... and the VALUES of that window against the oracle (fp32, host CPU) run on the same 734 x 734 crop -- the crop holds the window's whole
    # receptive field, so the oracle's window IS the reference's value for the full frame (run.py:217-219, RRDBNet_arch.py:50-51).  SURVEY 8c:
    # fp16 engine <= 1e-2 and >= 99 % of the uint8 codes within +-1; fp32-accurate engine (a float32 frame: 24 GB of slab pairs) <= 1e-4.
    import oracle
    crop = x[:, :, y0:y1, x0:x1].float().cpu()
    with torch.no_grad():
        ref = oracle.rrdbnet_forward(sd, crop, nb=23, scale=4)[:, :, 4 * (cy - hw - y0):4 * (cy + hw - y0), 4 * (cx - hw - x0):4 * (cx + hw - x0)]
    e16 = (a.float().cpu() - ref).abs()
    print(f"1080p frame, 128x128 HR window vs oracle: fp16 engine max {e16.max().item():.2e} mean {e16.mean().item():.2e}")
    assert e16.max().item() < 1e-2, e16.max().item()
    assert _codes_within_one(dev, a.float().cpu().numpy(), ref.numpy()) >= 0.99
    del y, yc
    y32 = net(x.float())
    e32 = (y32[:, :, 4 * (cy - hw):4 * (cy + hw), 4 * (cx - hw):4 * (cx + hw)].cpu() - ref).abs()
    print(f"1080p frame, same window: fp32-accurate engine max {e32.max().item():.2e} mean {e32.mean().item():.2e}")
    assert e32.max().item() < 1e-4, e32.max().item()
    # ... and the frame's BORDERS against the oracle: the 128 x 128 HR windows in the top-left and bottom-right corners, where the
    # zero padding of every conv (block.py:163-166, 213-254) meets the tile lattice's first and last (partly filled) tiles.  The oracle runs on the
    # (32 + R)^2 LR crop anchored AT the corner: it shares the frame's two borders there, its other two sides lie beyond the window's receptive radius.
    for name, (rows, cols, win) in {"top-left": (slice(0, 32 + R), slice(0, 32 + R), (slice(0, 128), slice(0, 128))),
                                    "bottom-right": (slice(1080 - 32 - R, 1080), slice(1920 - 32 - R, 1920), (slice(-128, None), slice(-128, None)))}.items():
        with torch.no_grad():
            cref = oracle.rrdbnet_forward(sd, x[:, :, rows, cols].float().cpu(), nb=23, scale=4)[:, :, win[0], win[1]]
        c16 = (corners16[name] - cref).abs()
        c32 = (y32[:, :, win[0], win[1]].cpu() - cref).abs()
        print(f"1080p frame, {name} 128x128 HR corner vs oracle: fp16 engine max {c16.max().item():.2e} mean {c16.mean().item():.2e}; "
              f"fp32-accurate engine max {c32.max().item():.2e}")
        assert c16.max().item() < 1e-2, (name, c16.max().item())
        assert _codes_within_one(dev, corners16[name].numpy(), cref.numpy()) >= 0.99, name
        assert c32.max().item() < 1e-4, (name, c32.max().item())
    del y32
    net.release_workspace()
    torch.cuda.empty_cache()


def test_bench_shape_tile_batch_vs_oracle(dev):
    """The chop path at the bench's shape: ONE launch sequence over a canvas of 266 tiles of 200 x 200 (parallel.tile_batches: 798 = 3 x 266) through
    RRDBNet-23 4x.  Tiles at the canvas's first, an inner and its last cell against the oracle's fp32 forward of that tile alone (<= 1e-2, >= 99 %
    of the uint8 codes within +-1) and against the batch-1 forward of the engine (bit for bit: tiles are independent, run.py:186-197)."""
    import oracle
    from innfer_amd import synth
    from innfer_amd.parallel import tile_batches
    assert tile_batches(798, None)[0] == 266
    net, sd = _rrdb(dev, 23, 4)
    n = 266
    tiles = torch.from_numpy(synth.uniform((n, 3, 200, 200), 93)).half()
    y = net(tiles.to(dev))
    assert tuple(y.shape) == (n, 3, 800, 800)
    for i in (0, 137, 265):
        assert torch.equal(y[i:i + 1], net(tiles[i:i + 1].to(dev))), i
    for i in (137, 265):
        with torch.no_grad():
            ref = oracle.rrdbnet_forward(sd, tiles[i:i + 1].float(), nb=23, scale=4)
        err = (y[i:i + 1].float().cpu() - ref).abs()
        print(f"tile {i} of a 266-tile canvas vs oracle: max {err.max().item():.2e} mean {err.mean().item():.2e}")
        assert err.max().item() < 1e-2, (i, err.max().item())
        assert _codes_within_one(dev, y[i:i + 1].float().cpu().numpy(), ref.numpy()) >= 0.99
    del y
    net.release_workspace()
    torch.cuda.empty_cache()


def test_unet256_batch64_vs_oracle(dev, golden):
    """BASELINE config 5 at its stated size: pix2pix UNet_256 on 64 x 3 x 256 x 256 (train-mode BatchNorm per image, run.py:299-303,349-357).  Images
    0 and 63 of the batch against the engine's batch-1 forwards (bit for bit) and against the oracle's fp32 forward of that image (<= 1e-2
    on the tanh output... the network amplifies fp16 rounding through eight BatchNorms: bounded like golden G7 / G17)."""
    import ast
    import oracle
    from innfer_amd import synth
    from innfer_amd.architectures import get_network
    from innfer_amd.utils.defaults import get_network_G_config
    g = golden("g7_unet256")
    shapes = {str(k): ast.literal_eval(str(s)) for k, s in zip(g["keys"], g["shapes"])}
    sd = _sd(shapes)
    net = get_network(get_network_G_config("unet_256", 1))
    net.load_state_dict(sd, strict=True)
    net = net.to(dev).train()                              # run.py runs pix2pix with meval=False
    x = torch.from_numpy(synth.uniform((64, 3, 256, 256), 640, -1.0, 1.0)).half()
    y = net(x.to(dev))
    assert tuple(y.shape) == (64, 3, 256, 256) and torch.isfinite(y).all()
    for i in (0, 63):
        assert torch.equal(y[i:i + 1], net(x[i:i + 1].to(dev))), i
        with torch.no_grad():
            ref = oracle.unet_forward(sd, x[i:i + 1].float())
        err = (y[i:i + 1].float().cpu() - ref).abs()
        print(f"UNet_256 x64, image {i} vs oracle: max {err.max().item():.2e} mean {err.mean().item():.2e}")
        assert err.max().item() < 1e-2 and err.mean().item() < 1e-3, (i, err.max().item(), err.mean().item())


def test_4k_input_untiled_addresses_beyond_2gib(dev):
    """A 2160x3840 frame un-tiled through a 1-block 4x RRDBNet: the HR slabs are 17 GB each (132.7 M pixels x 64 channels), far beyond
    32-bit byte offsets.  A window at the bottom-right corner (the largest addresses) must equal the forward of a crop that
    contains the window plus the receptive radius, bit for bit (stride-1 convs are translation equivariant; the crop keeps
    the frame's bottom / right borders so the zero padding matches)."""
    from innfer_amd import synth
    net, _ = _rrdb(dev, 1, 4)
    H, W = 2160, 3840
    x = torch.from_numpy(synth.uniform((1, 3, H, W), 77)).to(dev).half()
    yf = net(x)                       # fused tail: 64 800 x 4 tiles, rim buffer and planar stores beyond 2 GiB as well
    net.fused_tail = False
    y = net(x)
    _assert_same_to_the_last_rounding(yf[:, :, -512:, -512:], y[:, :, -512:, -512:], "fused tail vs two launches, corner of the 4K frame")
    _assert_same_to_the_last_rounding(yf[:, :, :512, :512], y[:, :, :512, :512], "fused tail vs two launches, origin of the 4K frame")
    del yf
    assert tuple(y.shape) == (1, 3, 4 * H, 4 * W) and torch.isfinite(y[:, :, -64:, -64:]).all()
    R, hw = 1 * 15 + 6, 24
    y0, x0 = H - hw - R, W - hw - R
    yc = net(x[:, :, y0:, x0:].contiguous())
    assert torch.equal(y[:, :, 4 * (H - hw):, 4 * (W - hw):], yc[:, :, 4 * R:, 4 * R:])
    del y, yc
    net.release_workspace()
    torch.cuda.empty_cache()


@pytest.mark.parametrize("kind,scale,shape", [("p2p_256", 1, (2, 3, 256, 256)), ("resnet_9blocks", 1, (2, 3, 32, 48)), ("wbcunet", 1, (1, 3, 40, 56)),
                                              ("wbcunet_tf", 1, (1, 3, 40, 56)), ("ppon", 4, (2, 3, 24, 20)), ("pan", 4, (2, 3, 21, 37)),
                                              ("srgan", 4, (1, 3, 19, 33))])
def test_every_family_ignores_workspace_contents(dev, kind, scale, shape):
    """Every byte a forward reads from its workspace was written by an earlier launch of the SAME forward: filling the
    workspace with NaN patterns between two forwards must not change a single output bit (pad channels, halo rows, split-K
    partials, statistics scratch ...).  Nor must 0x7B bytes (fp16 0x7B7B = 6.1e4, fp32 1.3e36: finite and huge) -- a running
    maximum or a select drops a NaN it read and shows a huge finite value; NaN x 0 shows where a finite value x 0 does not."""
    from innfer_amd import synth
    from innfer_amd.architectures import get_network
    from innfer_amd.utils.defaults import get_network_G_config
    net = get_network(get_network_G_config(kind, scale))
    net.load_state_dict(_sd({k: tuple(v.shape) for k, v in net.state_dict().items()}, 5), strict=True)
    net = net.to(dev)
    if kind.startswith("p2p"):
        net.train()
    else:
        net.eval()
    x = torch.from_numpy(synth.uniform(shape, 6, -1.0, 1.0)).to(dev).half()
    out = lambda r: r[-1] if isinstance(r, (tuple, list)) else r
    y = out(net(x)).clone()
    assert torch.isfinite(y).all()
    net._ws.fill_(0xFF)
    assert torch.equal(out(net(x)), y), "0xFF (NaN) in the workspace changes the result"
    net._ws.fill_(0x7B)
    assert torch.equal(out(net(x)), y), "0x7B (huge, finite) in the workspace changes the result"


@pytest.mark.parametrize("kind", ["wbcunet", "resnet_9blocks"])
def test_7x7_last_conv_interior_and_edge_tiles_vs_oracle(dev, kind):
    """The last 7x7 conv of the WBC UNet (zero padding) and of the CycleGAN generator (ReflectionPad2d(3), tanh) runs as nine displaced
    3x3 convs; tiles at least 4 pixels away from every border take the tile-relative path, the others derive per-lane offsets from
    the image origin.  132x172 has both kinds (24x32 tiles) and ragged last tiles; compared with the oracle."""
    import oracle
    from innfer_amd import synth
    from innfer_amd.architectures import get_network
    from innfer_amd.utils.defaults import get_network_G_config
    net = get_network(get_network_G_config(kind, 1))
    sd = _sd({k: tuple(v.shape) for k, v in net.state_dict().items()}, 9)
    net.load_state_dict(sd, strict=True)
    net = net.to(dev).eval()
    x = torch.from_numpy(synth.uniform((1, 3, 132, 172), 10, -1.0, 1.0))
    y = net(x.to(dev).half()).float().cpu()
    with torch.no_grad():
        ref = oracle.wbcunet_forward(sd, x) if kind == "wbcunet" else oracle.resnet_forward(sd, x, n_blocks=9)
    err = (y - ref).abs()
    assert err.max().item() < 3e-2 and err.mean().item() < 3e-3, (kind, err.max().item(), err.mean().item())


def test_weight_upload_follows_rebound_buffers_and_parameters(dev):
    """nn.Module._apply (.to / .cuda / .half) REBINDS buffers, load_state_dict(assign=True) rebinds parameters; the engine's cached walk of the
    module tree must not keep comparing the old tensor objects -- an edit of a BatchNorm running mean, or new weights, after such a rebinding has to reach
    the next forward."""
    from innfer_amd import synth
    from innfer_amd.architectures.RRDBNet_arch import RRDBNet
    shapes = synth.rrdbnet_shapes(nb=1, scale=2, norm=True)
    net = RRDBNet(3, 3, 64, 1, upscale=2, norm_type="batch")
    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in synth.fill_running_stats(synth.fill_state_dict(shapes, 7), 7).items()}
    net.load_state_dict(sd, strict=True)
    net = net.to(dev).eval()
    x = torch.from_numpy(synth.uniform((1, 3, 16, 16), 8)).to(dev).half()
    y0 = net(x).clone()
    net._apply(lambda t: t.clone())                                   # what .to() does to buffers: new tensor objects behind the same names
    bn = [k for k in net.state_dict() if k.endswith("running_mean")][0]
    dict(net.named_buffers())[bn].add_(0.25)                          # in-place edit of the NEW object
    y1 = net(x).clone()
    assert not torch.equal(y1, y0), "the forward still used the statistics uploaded before the buffers were rebound"
    sd2 = {k: v.clone() for k, v in net.state_dict().items()}
    wkey = [k for k in sd2 if k.endswith("conv1.0.weight")][0]
    sd2[wkey] = sd2[wkey] * 0.5
    net.load_state_dict(sd2, strict=True, assign=True)                # parameters replaced by new objects
    y2 = net(x)
    assert not torch.equal(y2, y1), "the forward still used the weights uploaded before load_state_dict(assign=True)"
    # the same for the engines addressed by parameter key (UNet: BatchNorm buffers are part of its eval-mode forward)
    from innfer_amd.architectures import get_network
    from innfer_amd.utils.defaults import get_network_G_config
    un = get_network(get_network_G_config("unet_128", 1))
    un.load_state_dict(_sd({k: tuple(v.shape) for k, v in un.state_dict().items()}, 9), strict=True)
    un = un.to(dev).eval()
    xu = torch.from_numpy(synth.uniform((1, 3, 128, 128), 10, -1, 1)).to(dev).half()
    u0 = un(xu).clone()
    un._apply(lambda t: t.clone())
    rv = [k for k in dict(un.named_buffers()) if k.endswith("running_var")][0]
    dict(un.named_buffers())[rv].mul_(4.0)
    assert not torch.equal(un(xu), u0)
