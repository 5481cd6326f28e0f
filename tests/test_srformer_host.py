"""SRFormer without a GPU: the sniffing and its refusals, the key table, the reference of tests/_srformer_ref.py against a module-style restatement, the shell's
load-time folds taken apart again, and the fixture conditions tests/test_gpu_srformer.py relies on (the storage model alone keeps >= 99 % of the uint8 codes within +-1;
max |q k^T| >= 4: the attention is far from uniform)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _srformer_ref as SF

B0 = "layers.0.residual_group.blocks.0."


def _zeros(**kw):
    from innfer_amd.architectures.keys import srformer_shapes
    return {k: torch.zeros(s) for k, s in srformer_shapes(**kw).items()}


@pytest.mark.parametrize("C,depths,nH,ws,ratio,ups,s", [(60, (6, 6, 6, 6), 6, 16, 2.0, "pixelshuffledirect", 2), (180, (6,) * 6, 6, 22, 2.0, "pixelshuffle", 4),
                                                         (180, (2, 3), 6, 24, 2.0, "nearest+conv", 4), (96, (2,), 4, 24, 3.0, "pixelshuffle", 3)])
def test_infer(C, depths, nH, ws, ratio, ups, s):
    from innfer_amd.run import infer_from_state_dict
    sd = _zeros(embed_dim=C, depths=depths, num_heads=nH, mlp_ratio=ratio, upscale=s, upsampler=ups, window_size=ws)
    for wrap in (lambda d: d, lambda d: {"params": d}, lambda d: {"params_ema": dict(d, **SF.buffers(d, ws))}):
        info = infer_from_state_dict(wrap(sd))
        p = info["net_params"]
        assert (info["arch"], info["scale"], p["embed_dim"], tuple(p["depths"]), p["num_heads"][0], p["window_size"], p["upsampler"]) == ("srformer", s, C, tuple(depths), nH, ws, ups)
        assert int(C * p["mlp_ratio"] + 1e-6) == int(C * ratio) and info["state_dict"].keys() == sd.keys()


def test_incomplete_key_set_is_sniffed_as_before():
    from innfer_amd.run import infer_from_state_dict
    for gone in ("attn.q.weight", "attn.kv.weight", "mlp.dwconv.depthwise_conv.0.weight"):
        sd = _zeros(embed_dim=60, depths=(2,), upsampler="pixelshuffledirect", upscale=2, window_size=16)
        del sd[B0 + gone]
        with pytest.raises(Exception, match="Could not infer model parameters"):
            infer_from_state_dict(sd)


def test_refusals_name_their_reason():
    from innfer_amd.architectures.SRFormer_arch import SRFormer
    from innfer_amd.run import infer_from_state_dict
    base = dict(embed_dim=60, depths=(2,), upsampler="pixelshuffle", upscale=2, window_size=16)

    def refused(match, edit):
        sd = _zeros(**base)
        edit(sd)
        with pytest.raises(NotImplementedError, match=match):
            infer_from_state_dict(sd)
    refused("window_size 14", lambda sd: sd.update({k: torch.zeros(169, 6) for k in list(sd) if k.endswith("bias_table")}))
    refused("absolute_pos_embed", lambda sd: sd.update(absolute_pos_embed=torch.zeros(1, 64, 60)))
    refused("upsampler ''", lambda sd: [sd.pop(k) for k in list(sd) if k.startswith(("conv_before_upsample", "upsample", "conv_last"))])
    refused("hidden <= 1024", lambda sd: sd.update({B0 + "mlp.fc1.weight": torch.zeros(1100, 60)}))
    refused("unequal channel counts", lambda sd: sd.update({"conv_last.weight": torch.zeros(1, 64, 3, 3)}))
    refused("differs from", lambda sd: sd.update({B0 + "attn.aligned_relative_position_index": SF.aligned_index(16).flip(0)}))
    with pytest.raises(NotImplementedError, match="img_range"):
        SRFormer(embed_dim=60, depths=(2,), num_heads=(6,), window_size=16, upscale=2, upsampler="pixelshuffle", img_range=255.)
    with pytest.raises(NotImplementedError, match="window_size=8"):
        SRFormer(embed_dim=60, depths=(2,), num_heads=(6,), window_size=8, upscale=2, upsampler="pixelshuffle")
    net = SRFormer(embed_dim=60, depths=(2,), num_heads=(6,), window_size=16, upscale=2, upsampler="pixelshuffle")
    with pytest.raises(NotImplementedError, match="fp16 mode"):
        net(torch.zeros(1, 3, 16, 16))


def _psa_restated(u, lin_q, lin_kv, table, ws, shift):
    """The attention as a module would write it: nn.Linear on tokens, torch.roll, space-to-depth for the keys, the mask from label images on both grids."""
    N, C, Hp, Wp = u.shape
    nH, pw, d = table.shape[1], ws // 2, C // table.shape[1]
    t = u.permute(0, 2, 3, 1)
    if shift:
        t = torch.roll(t, (-shift, -shift), (1, 2))
    q = lin_q(t) * d ** -0.5                                                                 # [N, Hp, Wp, C]
    kv = lin_kv(t).reshape(N, Hp // 2, 2, Wp // 2, 2, 2, C // 4)                            # (Y, a, X, b, k | v, cc)
    kv = kv.permute(5, 0, 1, 3, 2, 4, 6).reshape(2, N, Hp // 2, Wp // 2, C)                 # channel (2 a + b)(C / 4) + cc on the half-resolution grid
    lab = lambda H, W, win, sh: torch.bucketize(torch.arange(H), torch.tensor([H - win, H - sh]), right=True)[:, None] * 3 + \
        torch.bucketize(torch.arange(W), torch.tensor([W - win, W - sh]), right=True)[None, :]
    lq, lk = lab(Hp, Wp, ws, ws // 2), lab(Hp // 2, Wp // 2, pw, pw // 2)
    out = torch.zeros(N, Hp, Wp, C, dtype=u.dtype)
    idx = torch.tensor([[(r // 2 - py + pw - 1) * (2 * pw - 1) + (c // 2 - px + pw - 1) for py in range(pw) for px in range(pw)] for r in range(ws) for c in range(ws)])
    for wy in range(Hp // ws):
        for wx in range(Wp // ws):
            qs = q[:, wy * ws:(wy + 1) * ws, wx * ws:(wx + 1) * ws].reshape(N, ws * ws, nH, d).transpose(1, 2)
            ks, vs = (kv[i][:, wy * pw:(wy + 1) * pw, wx * pw:(wx + 1) * pw].reshape(N, pw * pw, nH, d).transpose(1, 2) for i in (0, 1))
            S = qs @ ks.transpose(-1, -2) + table[idx.reshape(-1)].reshape(ws * ws, pw * pw, nH).permute(2, 0, 1)
            if shift:
                a, b = lq[wy * ws:(wy + 1) * ws, wx * ws:(wx + 1) * ws].reshape(-1), lk[wy * pw:(wy + 1) * pw, wx * pw:(wx + 1) * pw].reshape(-1)
                S = S + torch.where(a[:, None] != b[None, :], -100.0, 0.0)
            out[:, wy * ws:(wy + 1) * ws, wx * ws:(wx + 1) * ws] = (torch.softmax(S, -1) @ vs).transpose(1, 2).reshape(N, ws, ws, C)
    if shift:
        out = torch.roll(out, (shift, shift), (1, 2))
    return out.permute(0, 3, 1, 2)


@pytest.mark.parametrize("ws,C,nH,shift", [(22, 60, 6, 11), (22, 60, 6, 0), (16, 64, 2, 8), (24, 96, 4, 12)])
def test_reference_equals_module_style_restatement(ws, C, nH, shift):
    torch.manual_seed(ws + shift)
    lin_q, lin_kv = torch.nn.Linear(C, C).double(), torch.nn.Linear(C, C // 2).double()
    u = torch.randn(2, C, 2 * ws, 3 * ws, dtype=torch.float64)
    table = torch.randn((ws - 1) ** 2, nH, dtype=torch.float64)
    with torch.no_grad():
        want = _psa_restated(u, lin_q, lin_kv, table, ws, shift)
        q = F.conv2d(u, lin_q.weight[:, :, None, None], lin_q.bias) * (C // nH) ** -0.5
        kv = F.conv2d(u, lin_kv.weight[:, :, None, None], lin_kv.bias)
        got, _ = SF.psa(q, kv[:, :C // 4], kv[:, C // 4:], table, ws, shift)
    assert float((got - want).abs().max()) <= 1e-12
    if ws == 22 and shift:          # key row 5 of a last-row window is label 1 although it covers query rows 10 and 11
        M = SF.shift_mask(44, 66, 22)[-1]
        assert M[10 * 22, 5 * 11] == 0 and M[11 * 22, 5 * 11] == -100 and M[11 * 22, 6 * 11] == 0


def test_shell_folds_taken_apart():
    """attn.q, attn.kv and the last conv as the shell hands them to the engine, put together again: the float64 definition to 5e-8."""
    from innfer_amd.architectures.SRFormer_arch import SRFormer
    for name in ("C60 nH6 [2] ws16 direct x2 13x21", "C180 nH6 [2] ws22 pixelshuffle x4 44x66"):
        Cc, nH, depths, ws, shape, ups, s, seed = SF.FIXTURES[name]
        sd = SF.fixture_sd(name)
        net = SRFormer(embed_dim=Cc, depths=depths, num_heads=[nH] * len(depths), window_size=ws, upscale=s, upsampler=ups)
        net.load_state_dict(sd, strict=True)
        d, c4 = Cc // nH, Cc // 4
        kg = -(-c4 // 32)
        f64 = lambda k: sd[k].double().numpy()
        wq, bq = net.relayout(B0 + "attn.q", f64(B0 + "attn.q.weight"), f64(B0 + "attn.q.bias"))
        assert wq.shape == (-(-nH // 2) * 64, -(-Cc // 64) * 64, 1, 1)
        back = np.concatenate([wq[32 * h:32 * h + d, :Cc, 0, 0] for h in range(nH)]).astype(np.float64)
        assert np.abs(back - f64(B0 + "attn.q.weight") * d ** -0.5).max() <= 5e-8 and np.count_nonzero(wq) == np.count_nonzero(back)
        assert np.abs(np.concatenate([bq[32 * h:32 * h + d] for h in range(nH)]) - f64(B0 + "attn.q.bias") * d ** -0.5).max() <= 5e-8
        wk, bk = net.relayout(B0 + "attn.kv", f64(B0 + "attn.kv.weight"), f64(B0 + "attn.kv.bias"))
        assert wk.shape == (kg * 64, -(-Cc // 64) * 64, 1, 1)
        back = np.concatenate([wk[:c4, :Cc, 0, 0], wk[32 * kg:32 * kg + c4, :Cc, 0, 0]])
        assert np.array_equal(back, sd[B0 + "attn.kv.weight"].numpy()) and np.count_nonzero(wk) == np.count_nonzero(back)
        assert np.array_equal(np.concatenate([bk[:c4], bk[32 * kg:32 * kg + c4]]), sd[B0 + "attn.kv.bias"].numpy())
        last = "upsample.0" if ups == "pixelshuffledirect" else "conv_last"
        wl, bl = net.relayout(last, f64(last + ".weight"), f64(last + ".bias"))
        mean = np.asarray(np.float32(SF.SR.MEAN), np.float64)
        assert np.abs(bl - (f64(last + ".bias") + (np.repeat(mean, s * s) if last == "upsample.0" else mean))).max() <= 5e-8
        assert np.array_equal(wl[:, :Cc] if last == "upsample.0" else wl, sd[last + ".weight"].numpy())
        norms, tables, taps, biases = net.engine_tables()
        assert len(norms) == 2 + 2 * sum(depths) and np.array_equal(tables[0], sd[B0 + "attn.relative_position_bias_table"].numpy().T)
        assert np.array_equal(taps[0].reshape(-1, 1, 5, 5), sd[B0 + "mlp.dwconv.depthwise_conv.0.weight"].numpy())


@pytest.mark.parametrize("name", list(SF.FIXTURES))
def test_fixture_conditions(name):
    sd, x, y64, ys, smax = SF.case(name)
    share = SF.SR.codes_within_one(ys, y64)
    print(f"[srformer] {name}: storage model max|err| {float((ys - y64).abs().max()):.2e}, codes within +-1 {share:.5f}, max |q k^T| {smax:.1f}")
    assert share >= 0.99 and smax >= 4.0
