"""DAT, what can be checked without a GPU: keys.dat_shapes loads strict=True into the shell and run._infer_dat round-trips the published configurations (with and
without the buffers, under params / params_ema); shift_blocks from stored masks; the dense bias, the BatchNorm folds and the fc1 / fc2 half layout taken apart again against
float64; every refusal; SwinIR, HAT and Swin2SR dictionaries keep their route; the fp16 storage model alone meets the 99 % criterion on the network fixtures.  And the kernels: the new entry points are declared, bound and built; the refusals that need no device; the mask the
rectangular window attention computes from coordinates against the mask built the published way; tests/_dat_ref.py against independent formulations of the same
definitions (so that the reference the GPU tests lean on is itself checked)."""
import ctypes as C
import os
import re

import numpy as np
import torch

import _dat_ref as DR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("innfer_window_attention_rect", "innfer_channel_attention_work_bytes", "innfer_channel_attention_scores", "innfer_channel_attention_apply", "innfer_dwconv3x3",
       "innfer_chan_attn_excite_gelu", "innfer_aim_mix", "innfer_layer_norm_wide", "innfer_dat_create", "innfer_dat_block_floats", "innfer_net_set_dat_block")


def test_new_symbols_are_declared_bound_and_built():
    """Declared in the header (additive under 123: the revision stays), bound in lib.py's SIGNATURES, exported by the library; the sources are part of the build."""
    import innfer_amd.lib as L
    hdr = open(os.path.join(ROOT, "include", "innfer_amd.h")).read()
    for sym in NEW:
        assert re.search(r"^(?:int|size_t) %s\(" % sym, hdr, re.M), sym
        assert sym in L.SIGNATURES and hasattr(L.lib, sym), sym
    assert re.search(r"^#define INNFER_ABI_VERSION 124$", hdr, re.M) and L.lib.innfer_version() == 124
    assert "innfer_window_attention_rect" in hdr.split("#define INNFER_ABI_VERSION")[0], "the revision note does not name the new entry points"
    mk = open(os.path.join(ROOT, "Makefile")).read()
    for src in ("win_attn_rect", "chan_self_attn", "dwconv", "aim_mix", "dat_launches"):
        assert f"csrc/{src}.hip" in mk, src


def test_refusals_without_a_device():
    """What the entries refuse before they touch the device: status and message."""
    import innfer_amd.lib as L
    lib = L.lib
    one = C.c_void_p(256)          # (never dereferenced: every call below returns before a launch)
    tb = np.zeros(4, np.float32)
    rect = lambda nH, s0, s1, q=one: lib.innfer_window_attention_rect(q, 0, one, 0, tb.ctypes.data, 1, 8, 8, nH, 8, s0, s1, 0, None)
    assert rect(2, 8, 32, q=None) == L.ERR_INVALID
    for s0, s1 in ((8, 8), (16, 16), (32, 8), (8, 64), (4, 32), (7, 7)):
        assert rect(2, s0, s1) == L.ERR_UNSUPPORTED and "[8, 32] and [8, 16]" in L.last_error(), (s0, s1)
    for nH in (1, 3, 5, 7, 9, 10, 0):
        assert rect(nH, 8, 16) == L.ERR_UNSUPPORTED, nH
    assert lib.innfer_channel_attention_work_bytes(1, 2000, 6) == 4 * 6 * 1088 * 2 and lib.innfer_channel_attention_work_bytes(2, 1024, 2) == 4 * 2 * 2 * 1088
    assert lib.innfer_channel_attention_work_bytes(0, 64, 2) == 0
    sc = lambda nH, d, nb=1 << 20, HW=64: lib.innfer_channel_attention_scores(one, 64 * 32, 1, HW, nH, d, tb.ctypes.data, one, None, one, nb, None)
    assert sc(9, 8) == L.ERR_UNSUPPORTED and sc(2, 33) == L.ERR_UNSUPPORTED and sc(2, 32, nb=16) == L.ERR_WORKSPACE and sc(2, 32, HW=0) == L.ERR_INVALID
    assert lib.innfer_dwconv3x3(one, 0, None, 0, one, 0, 1, 8, 8, 513, 576, tb.ctypes.data, tb.ctypes.data, 0, None) == L.ERR_UNSUPPORTED
    assert lib.innfer_aim_mix(one, 0, one, 0, one, 0, one, 1, 64, 60, 64, 17, tb.ctypes.data, tb.ctypes.data, tb.ctypes.data, 0.0, None) == L.ERR_UNSUPPORTED
    assert lib.innfer_aim_mix(one, 0, one, 0, one, 0, one, 1, 64, 257, 320, 3, tb.ctypes.data, tb.ctypes.data, tb.ctypes.data, 0.0, None) == L.ERR_UNSUPPORTED
    assert lib.innfer_layer_norm_wide(one, 0, one, 0, 64, 513, 576, tb.ctypes.data, tb.ctypes.data, 1e-5, None) == L.ERR_UNSUPPORTED
    assert lib.innfer_chan_attn_excite_gelu(one, 0, 1, 64, 60, 64, 65, *([tb.ctypes.data] * 4), one, None, one, 1 << 20, None) == L.ERR_UNSUPPORTED


def _band(r, n, win, sh):
    return 0 if r < n - win else (1 if r < n - sh else 2)


def test_mask_from_coordinates_is_the_published_mask():
    """The label 3 a(r) + b(c) of csrc/win_attn_rect.hip (a = 0 below Hp - wh, 1 below Hp - shy, else 2; b likewise), token by token, against the mask built from the
    label image, its window partition and the pairwise differences: both splits, both branches, frames of one window row / column and of several."""
    for s1 in (32, 16):
        for H, W in ((5, 7), (32, 32), (40, 72), (33, 100)):
            Hp, Wp = DR.padded(H, W, 8, s1)
            for br in (0, 1):
                wh, ww, shy, shx = DR.branch_geometry(br, 8, s1, 1)
                assert (wh, ww, shy, shx) == ((8, s1, 4, s1 // 2) if br == 0 else (s1, 8, s1 // 2, 4))
                M = DR.shift_mask(Hp, Wp, wh, ww, shy, shx)
                nwx = Wp // ww
                assert M.shape == (Hp * Wp // (8 * s1), 8 * s1, 8 * s1)
                for w in range(M.shape[0]):
                    wy, wx = divmod(w, nwx)
                    lab = torch.tensor([3 * _band(wy * wh + j // ww, Hp, wh, shy) + _band(wx * ww + j % ww, Wp, ww, shx) for j in range(wh * ww)])
                    mine = torch.where(lab[:, None] != lab[None, :], -100.0, 0.0)
                    assert torch.equal(mine, M[w]), (s1, H, W, br, w)
                    if wy < Hp // wh - 1 and wx < nwx - 1:
                        assert not M[w].any(), "a window off the last row / column carries a mask"


def test_rect_attention_reference_pads_behind_the_linear():
    """A pad token is a key with q = k = v = 0 that takes part in the softmax: on a 5 x 7 grid, per pixel and head, the reference equals the softmax over the window's
    real tokens PLUS the pad tokens' bias-only scores; leaving the pad keys out gives something else.  The blocked model agrees with the exact softmax."""
    torch.manual_seed(0)
    nH, d, s1, H, W = 2, 4, 16, 5, 7
    T = 8 * s1
    qkv = torch.randn(3, 1, nH, d, H, W, dtype=torch.float64)
    table = torch.randn(nH, T, T, dtype=torch.float64)
    ref, _ = DR.rect_attention(qkv, table, 8, s1, 0, torch.float64)
    for h in range(nH):
        wh, ww = (8, s1) if h < nH // 2 else (s1, 8)
        tok = lambda r, c: r * ww + c                                       # (the one window at the origin holds the whole 5 x 7 grid)
        real = [tok(r, c) for r in range(H) for c in range(W)]
        k = qkv[1, 0, h].reshape(d, -1).T
        v = qkv[2, 0, h].reshape(d, -1).T
        for (r, c) in ((0, 0), (4, 6), (2, 3)):
            q = qkv[0, 0, h, :, r, c]
            s = table[h, tok(r, c)].clone()                                 # every key's bias; the pad keys' scores are the bias alone
            s[real] += k @ q
            p = torch.softmax(s, 0)
            assert torch.allclose(ref[0, h, :, r, c], p[real] @ v, atol=1e-12), (h, r, c)
            p_wrong = torch.softmax(s[real], 0)
            assert not torch.allclose(ref[0, h, :, r, c], p_wrong @ v, atol=1e-3)
    mod, _ = DR.rect_attention(qkv.half(), table.float(), 8, s1, 1, torch.float32, model=True)
    ex, _ = DR.rect_attention(qkv.half(), table.float(), 8, s1, 1, torch.float64)
    assert float((mod.double() - ex).abs().max()) < 5e-3


def test_channel_attention_reference():
    """F.normalize over the pixels: scaling q or k leaves A alone; an all-zero q column gives a uniform row; the apply is A v per pixel."""
    torch.manual_seed(1)
    N, nH, d, H, W = 2, 2, 5, 6, 7
    q, k, v = (torch.randn(N, nH, d, H, W, dtype=torch.float64) for _ in range(3))
    temp = torch.tensor([1.5, -0.7], dtype=torch.float64)
    G, sq, sk, A = DR.channel_scores(q, k, temp, torch.float64)
    assert torch.allclose(DR.channel_scores(3.0 * q, 0.25 * k, temp, torch.float64)[3], A, atol=1e-13)
    qn = torch.nn.functional.normalize(q.reshape(N, nH, d, -1), dim=-1)
    kn = torch.nn.functional.normalize(k.reshape(N, nH, d, -1), dim=-1)
    assert torch.allclose(A, torch.softmax(qn @ kn.transpose(-1, -2) * temp[None, :, None, None], -1), atol=1e-13)
    assert torch.allclose(G, torch.einsum("nhxp,nhyp->nhxy", q.reshape(N, nH, d, -1), k.reshape(N, nH, d, -1)), atol=1e-12)
    q[:, 0, 3] = 0
    A0 = DR.channel_scores(q, k, temp, torch.float64)[3]
    assert torch.equal(A0[:, 0, 3], torch.full((N, d), 1.0 / d, dtype=torch.float64))
    a = DR.channel_apply(A0, v)
    assert torch.allclose(a[1, 1, :, 2, 3], A0[1, 1] @ v[1, 1, :, 2, 3], atol=1e-13)


def test_fold_bn_and_the_small_references():
    """BatchNorm (eval) behind a conv folds into its weight and bias; the depthwise reference is the nine-tap sum with zero padding; the mix is X y + Y s."""
    torch.manual_seed(2)
    Cc = 6
    x = torch.randn(2, Cc, 5, 4, dtype=torch.float64)
    taps, bias = torch.randn(Cc, 3, 3, dtype=torch.float64), torch.randn(Cc, dtype=torch.float64)
    bw, bb, mean, var = torch.rand(Cc) + 0.5, torch.randn(Cc), torch.randn(Cc), torch.rand(Cc) + 0.5
    bn = torch.nn.BatchNorm2d(Cc).double().eval()
    with torch.no_grad():
        bn.weight.copy_(bw); bn.bias.copy_(bb); bn.running_mean.copy_(mean); bn.running_var.copy_(var)
        want = bn(DR.dwconv(x, taps, bias))
    wf, bf = DR.fold_bn(taps, bias, bw, bb, mean, var)
    assert torch.allclose(DR.dwconv(x, wf, bf), want, atol=1e-12)
    xp = torch.nn.functional.pad(x, (1, 1, 1, 1))
    manual = sum(taps[None, :, ky, kx, None, None] * xp[:, :, ky:ky + 5, kx:kx + 4] for ky in range(3) for kx in range(3)) + bias[None, :, None, None]
    assert torch.allclose(DR.dwconv(x, taps, bias), manual, atol=1e-12)
    assert abs(float(DR.gelu(torch.tensor(0.7, dtype=torch.float64))) - float(torch.nn.functional.gelu(torch.tensor(0.7, dtype=torch.float64)))) < 1e-15
    y = torch.randn(2, Cc, 5, 4, dtype=torch.float64)
    gate = torch.rand(2, Cc, dtype=torch.float64)
    w1, b1, w2 = torch.randn(2, Cc, dtype=torch.float64), torch.randn(2, dtype=torch.float64), torch.randn(2, dtype=torch.float64)
    out = DR.aim_mix(x, y, gate, w1, b1, w2, 0.3)
    n, r, c = 1, 2, 3
    s = torch.sigmoid(w2 @ DR.gelu(w1 @ x[n, :, r, c] + b1) + 0.3)
    assert torch.allclose(out[n, :, r, c], x[n, :, r, c] * gate[n] + y[n, :, r, c] * s, atol=1e-13)
    g, b = torch.rand(Cc, dtype=torch.float64) + 0.5, torch.randn(Cc, dtype=torch.float64)
    assert torch.allclose(DR.layer_norm(x, g, b), torch.nn.functional.layer_norm(x.permute(0, 2, 3, 1), (Cc,), g, b, 1e-5).permute(0, 3, 1, 2), atol=1e-12)


# ------------------------------------------------------------------------------------------------ the shell and the loader
CONFIGS = {          # the four published configurations as recalled (C, nH, split, depths, expansion_factor, upsampler, scale)
    "DAT": (180, 6, (8, 32), (6,) * 6, 4.0, "pixelshuffle", 4),
    "DAT-S": (180, 6, (8, 16), (6,) * 6, 2.0, "pixelshuffle", 4),
    "DAT-2": (180, 6, (8, 32), (6,) * 6, 2.0, "pixelshuffle", 2),
    "DAT-light": (60, 6, (8, 32), (18,), 2.0, "pixelshuffledirect", 3),
}


def _buffers(sd, split, depths, masks=None):
    """What a published checkpoint stores beside its parameters: rpe_biases and relative_position_index per branch of every window block, attn_mask_0 / _1 on shifted ones."""
    from innfer_amd.architectures import DAT_arch as A
    out = {}
    for i, depth in enumerate(depths):
        for j in range(0, depth, 2):
            for br, (wh, ww) in enumerate(((split[0], split[1]), (split[1], split[0]))):
                out[f"layers.{i}.blocks.{j}.attn.attns.{br}.rpe_biases"] = A.rpe_biases(wh, ww).float()
                out[f"layers.{i}.blocks.{j}.attn.attns.{br}.relative_position_index"] = A.relative_position_index(wh, ww)
            if (i, j) in (A.shifted_blocks(depths) if masks is None else masks):
                out[f"layers.{i}.blocks.{j}.attn.attn_mask_0"] = torch.zeros(4, 8, 8)
                out[f"layers.{i}.blocks.{j}.attn.attn_mask_1"] = torch.zeros(4, 8, 8)
    return out


def test_shapes_load_strict_and_infer_round_trips():
    from innfer_amd.architectures import get_network
    from innfer_amd.architectures.keys import dat_shapes
    from innfer_amd.run import infer_from_state_dict
    for name, (Cc, nH, split, depths, ef, ups, s) in CONFIGS.items():
        small = depths if len(depths) == 1 and depths[0] <= 2 else ((3, 2) if len(depths) > 1 else (4,))          # (the key table per block does not depend on the depth)
        sd = DR.fill(3, Cc, small, nH, ef, s, ups, "1conv", seed=3)
        assert set(sd) == set(dat_shapes(3, Cc, small, nH, ef, s, ups, "1conv"))
        for wrap, bufs in ((None, True), ("params_ema", True), ("params", False)):
            full = dict(sd, **(_buffers(sd, split, small) if bufs else {}))
            info = infer_from_state_dict({wrap: full} if wrap else full)
            p = info["net_params"]
            assert info["arch"] == "dat" and info["scale"] == s and set(info["state_dict"]) == set(sd), name
            assert (p["embed_dim"], p["depth"], p["num_heads"], p["expansion_factor"], p["upscale"], p["upsampler"]) == (Cc, list(small), [nH] * len(small), ef, s, ups), (name, p)
            if bufs:
                from innfer_amd.architectures.DAT_arch import shifted_blocks
                assert p["split_size"] == list(split) and not p["split_assumed"] and p["shift_blocks"] == (shifted_blocks(small) or None) and p["rpe_biases"] is not None
            else:
                assert p["split_size"] == [8, 32] and p["split_assumed"] and p["shift_blocks"] is None and p["rpe_biases"] is None
            if bufs or split == (8, 32):
                net = get_network(dict(p))
                assert not net._has_fp32 and net.load_state_dict(info["state_dict"], strict=True)


def test_shift_blocks_come_from_the_stored_masks():
    from innfer_amd.architectures import get_network
    from innfer_amd.run import infer_from_state_dict
    sd = DR.fill(3, 60, (3, 2), 6, 2.0, 2, "pixelshuffledirect", "3conv", seed=4)
    info = infer_from_state_dict(dict(sd, **_buffers(sd, (8, 16), (3, 2), masks=[(0, 0), (1, 0)])))
    assert info["net_params"]["shift_blocks"] == [(0, 0), (1, 0)] and info["net_params"]["resi_connection"] == "3conv"
    assert get_network(dict(info["net_params"])).shift_blocks == [(0, 0), (1, 0)]
    info = infer_from_state_dict(dict(sd, **{k: v for k, v in _buffers(sd, (8, 16), (3, 2)).items() if "attn_mask" not in k}))
    assert info["net_params"]["shift_blocks"] is None and get_network(dict(info["net_params"])).shift_blocks == [(0, 2), (1, 0)]


def test_dense_bias_and_folds_against_float64():
    from innfer_amd.architectures import DAT_arch as A
    Cc, nH, split, ef = 60, 6, (8, 16), 2.0
    sd = DR.fill(3, Cc, (2,), nH, ef, 2, "pixelshuffledirect", "1conv", seed=5)
    tb = torch.from_numpy(A.dense_bias(sd, "layers.0.blocks.0.", *split)).double()
    ref = torch.cat([DR.pos_bias(sd, "layers.0.blocks.0.attn.attns.0.pos.", 8, 16), DR.pos_bias(sd, "layers.0.blocks.0.attn.attns.1.pos.", 16, 8)])
    assert tb.shape == (nH, 128, 128) and float((tb - ref).abs().max()) <= 2.0 ** -24 * float(ref.abs().max())
    net = A.DAT(embed_dim=Cc, split_size=[8, 16], depth=[2], num_heads=[nH], expansion_factor=ef, upscale=2, upsampler="pixelshuffledirect")
    net.load_state_dict(sd, strict=True)
    for j in (0, 1):          # the packed block parameters, taken apart again
        b = f"layers.0.blocks.{j}."
        prm = torch.from_numpy(net.block_params(net.state_dict(), 0, j)).double()
        chp, hc, hs, half, d = 32 * nH, Cc // 8, Cc // 16, int(Cc * ef) // 2, Cc // nH
        hp = A.head_pad_index(Cc, nH)
        at = 0
        def take(*shape):
            nonlocal at
            n = int(np.prod(shape)); v = prm[at:at + n].reshape(shape); at += n
            return v
        dw_t, dw_b = take(chp, 9), take(chp)
        w64, b64 = DR.fold_bn(sd[b + "attn.dwconv.0.weight"].reshape(Cc, 9), sd[b + "attn.dwconv.0.bias"], sd[b + "attn.dwconv.1.weight"], sd[b + "attn.dwconv.1.bias"],
                              sd[b + "attn.dwconv.1.running_mean"], sd[b + "attn.dwconv.1.running_var"])
        assert torch.allclose(dw_t[hp], w64, rtol=2e-7, atol=0) and torch.allclose(dw_b[hp], b64, rtol=2e-7, atol=1e-9)
        pad = torch.ones(chp, dtype=torch.bool); pad[hp] = False
        assert not dw_t[pad].any() and not dw_b[pad].any()
        ci_w1, ci_b1, ci_w2, ci_b2 = take(hc, chp), take(hc), take(chp, hc), take(chp)
        w64, b64 = DR.fold_bn(sd[b + "attn.channel_interaction.1.weight"].reshape(hc, Cc), sd[b + "attn.channel_interaction.1.bias"], sd[b + "attn.channel_interaction.2.weight"],
                              sd[b + "attn.channel_interaction.2.bias"], sd[b + "attn.channel_interaction.2.running_mean"], sd[b + "attn.channel_interaction.2.running_var"])
        assert torch.allclose(ci_w1[:, hp], w64, rtol=2e-7, atol=0) and torch.allclose(ci_b1, b64, rtol=2e-7, atol=1e-9) and not ci_w1[:, pad].any()
        assert torch.equal(ci_w2[hp].float(), sd[b + "attn.channel_interaction.4.weight"].reshape(Cc, hc)) and torch.equal(ci_b2[hp].float(), sd[b + "attn.channel_interaction.4.bias"])
        si_w1, si_b1, si_w2, si_b2 = take(hs, chp), take(hs), take(hs), take(1)
        w64, b64 = DR.fold_bn(sd[b + "attn.spatial_interaction.0.weight"].reshape(hs, Cc), sd[b + "attn.spatial_interaction.0.bias"], sd[b + "attn.spatial_interaction.1.weight"],
                              sd[b + "attn.spatial_interaction.1.bias"], sd[b + "attn.spatial_interaction.1.running_mean"], sd[b + "attn.spatial_interaction.1.running_var"])
        assert torch.allclose(si_w1[:, hp], w64, rtol=2e-7, atol=0) and torch.allclose(si_b1, b64, rtol=2e-7, atol=1e-9)
        assert torch.equal(si_w2.float(), sd[b + "attn.spatial_interaction.3.weight"].reshape(hs)) and torch.equal(si_b2.float(), sd[b + "attn.spatial_interaction.3.bias"])
        g, be, sg_t, sg_b, temp = take(half), take(half), take(half, 9), take(half), take(nH)
        assert torch.equal(g.float(), sd[b + "ffn.sg.norm.weight"]) and torch.equal(sg_t.float(), sd[b + "ffn.sg.conv.weight"].reshape(half, 9)) and at == prm.numel()
        assert torch.equal(temp.float(), sd[b + "attn.temperature"].reshape(nH)) if j else not temp.any()
        # fc1 / fc2 in halves; qkv of the channel block unscaled, of the window block with d^-0.5 in the q rows
        w1 = np.concatenate([net._conv_tensors(b + f"ffn.fc1#{p}", net.state_dict())[0] for p in range(2)])
        assert np.array_equal(w1[:half, :Cc, 0, 0], sd[b + "ffn.fc1.weight"][:half].numpy()) and np.array_equal(w1[64:64 + half, :Cc, 0, 0], sd[b + "ffn.fc1.weight"][half:].numpy())
        assert not w1[half:64].any() and not w1[64 + half:].any() and not w1[:, Cc:].any()
        w2 = net._conv_tensors(b + "ffn.fc2#0", net.state_dict())[0]
        assert w2.shape == (64, 64, 1, 1) and np.array_equal(w2[:Cc, :half, 0, 0], sd[b + "ffn.fc2.weight"].numpy()) and not w2[:, half:].any()
        wq = net._conv_tensors(b + "attn.qkv#0", net.state_dict())[0]
        want = sd[b + "attn.qkv.weight"][:d].numpy() * (np.float32(1) if j else np.float32(d ** -0.5))
        assert np.array_equal(wq[:d, :Cc, 0, 0], want) and not wq[d:32].any()


def test_refusals_of_the_shell_and_the_loader():
    import pytest
    from innfer_amd.architectures.DAT_arch import DAT
    from innfer_amd.run import infer_from_state_dict
    ok = dict(embed_dim=60, split_size=[8, 16], depth=[2], num_heads=[6], expansion_factor=2.0, upscale=2, upsampler="pixelshuffledirect")
    for bad, word in ((dict(split_size=[8, 8]), "split_size"), (dict(split_size=[16, 16]), "split_size"), (dict(num_heads=[5]), "num_heads"), (dict(embed_dim=66, num_heads=[2]), "num_heads"),
                      (dict(img_range=255.0), "img_range"), (dict(upsampler="nearest+conv"), "upsampler"), (dict(qkv_bias=False), "qkv_bias")):
        with pytest.raises(NotImplementedError, match=word):
            DAT(**dict(ok, **bad))
    with pytest.raises(NotImplementedError, match="split_size.*img_range"):
        DAT(**dict(ok, split_size=[4, 4], img_range=2.0))
    net = DAT(**ok)
    with pytest.raises(NotImplementedError, match="fp16 mode"):
        net(torch.zeros(1, 3, 8, 8))
    with pytest.raises(NotImplementedError, match="fp16 mode"):
        net.tile_batch_bytes(1, 16, torch.float32)
    sd = DR.fill(3, 60, (2,), 6, 2.0, 2, "pixelshuffledirect", "1conv", seed=6)
    bufs = _buffers(sd, (8, 16), (2,))
    k = "layers.0.blocks.0.attn.attns.1.relative_position_index"
    with pytest.raises(NotImplementedError, match="differs from the published formula"):
        infer_from_state_dict(dict(sd, **dict(bufs, **{k: bufs[k].T.contiguous()})))
    from innfer_amd.architectures import DAT_arch as A
    odd = {f"layers.0.blocks.0.attn.attns.{br}.rpe_biases": A.rpe_biases(*((4, 4))).float() for br in (0, 1)}
    with pytest.raises(NotImplementedError, match="split_size"):
        infer_from_state_dict(dict(sd, **odd))


def test_other_dictionaries_keep_their_route():
    """A SwinIR, a HAT and a Swin2SR dictionary are sniffed as before; a dictionary with before_RG.1 but an incomplete block 0 falls through to the old route."""
    import pytest
    import _hat_ref as HR
    import _swin2sr_ref as S2
    import _swinir_ref as SR
    from innfer_amd.run import infer_from_state_dict
    assert infer_from_state_dict(HR.fill(3, 60, (1,), 6, 2.0, 2, 3, 30, seed=1))["arch"] == "hat"
    assert infer_from_state_dict(SR.fill(3, 60, (1,), 6, 2.0, 2, "pixelshuffledirect", "1conv", seed=1))["arch"] == "swinir"
    assert infer_from_state_dict(S2.fill(3, 60, (1,), 6, 2.0, 2, "pixelshuffledirect", "1conv", seed=1))["arch"] == "swin2sr"
    sd = DR.fill(3, 60, (2,), 6, 2.0, 2, "pixelshuffledirect", "1conv", seed=7)
    del sd["layers.0.blocks.0.attn.dwconv.0.weight"]
    with pytest.raises(Exception) as e:
        infer_from_state_dict(sd)
    assert not isinstance(e.value, NotImplementedError) or "DAT" not in str(e.value)


def test_storage_model_alone_meets_the_criterion():
    """The fp16 storage model of every network fixture keeps >= 99 % of the uint8 codes within +-1 of the float64 forward: the GPU test's criterion can be met at all."""
    for name in DR.FIXTURES:
        sd, x, y64, ys = DR.case(name)
        assert DR.codes_within_one(ys, y64) >= 0.99 and float((ys - y64).abs().max()) > 0, name
