"""Swin2SR: the host logic (no GPU) -- the key table, strict loading, checkpoint sniffing with and without the three buffers (a stored relative_coords_table is used), the
refusals, what the other families still sniff as, the shell's dense bias table and tau against the float64 definition, the new symbols, and the test data's own figures:
the storage model's error, the share of peaked softmax rows, and what each planted fault costs."""
import math
import os
import re

import numpy as np
import pytest
import torch

import _swin2sr_ref as S2
import _swinir_ref as SR
from innfer_amd import synth
from innfer_amd.run import infer_from_state_dict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (in_chans, C, depths, nH, mlp_ratio, s, upsampler, resi, cpb hidden)
VARIANTS = [(3, 180, (6,) * 6, 6, 2.0, 4, "pixelshuffle", "1conv", 512), (3, 60, (6,) * 4, 6, 2.0, 2, "pixelshuffledirect", "1conv", 512),
            (3, 180, (6,) * 6, 6, 2.0, 4, "nearest+conv", "1conv", 512), (3, 240, (6,) * 9, 8, 2.0, 4, "nearest+conv", "3conv", 512),
            (1, 64, (2, 1), 2, 4.0, 3, "pixelshuffle", "3conv", 1), (4, 96, (1, 2, 3), 4, 1.5, 3, "pixelshuffledirect", "1conv", 48),
            (3, 60, (2,), 6, 2.0, 2, "nearest+conv", "1conv", 512), (3, 60, (2,), 6, 2.0, 2, "pixelshuffle", "1conv", 512)]
FAULTS = ("no_qk_norm", "no_clamp", "pre_norm", "no_sigmoid", "k_bias", "coords_linear", "no_shift", "no_mask", "bias_T", "roll_sign", "ln_pad")
B0 = "layers.0.residual_group.blocks.0."


def _zeros(v):
    return {k: torch.zeros(s) for k, s in S2.shapes(*v).items()}


def _ids(v):
    return f"in{v[0]}-C{v[1]}-{len(v[2])}x-nH{v[3]}-r{v[4]}-x{v[5]}-{v[6]}-{v[7]}-cpb{v[8]}"


def _params(v, coords=False):
    cin, Cc, depths, nH, r, s, ups, resi, cpb = v
    return dict(type="swin2sr", in_chans=cin, embed_dim=Cc, depths=list(depths), num_heads=[nH] * len(depths), window_size=8, mlp_ratio=r, upscale=s, img_range=1.0,
                upsampler=ups, resi_connection=resi, cpb_hidden=cpb)


def _split(net_params):
    """net_params without the coords table (an array or None), and the table."""
    p = dict(net_params)
    return p, p.pop("coords_table")


def test_key_table_and_strict_loading():
    """swin2sr_shapes == the definition written out in _swin2sr_ref; the shell's state dict has exactly those keys (no buffers) and loads a filled one strictly."""
    from innfer_amd.architectures.Swin2SR_arch import Swin2SR
    for v in VARIANTS:
        cin, Cc, depths, nH, r, s, ups, resi, cpb = v
        want = S2.shapes(*v)
        assert synth.swin2sr_shapes(cin, Cc, depths, nH, r, s, ups, resi, 8, cpb) == want
        assert not any(k.endswith(("relative_position_bias_table", "attn.qkv.bias")) for k in want)
        if sum(depths) > 6:
            continue
        net = Swin2SR(in_chans=cin, embed_dim=Cc, depths=depths, num_heads=[nH] * len(depths), window_size=8, mlp_ratio=r, upscale=s, upsampler=ups, resi_connection=resi,
                      cpb_hidden=cpb)
        assert {k: tuple(t.shape) for k, t in net.state_dict().items()} == {k: tuple(sh) for k, sh in want.items()}
        net.load_state_dict(S2.fill(*v, seed=5), strict=True)
    with pytest.raises(RuntimeError):          # a Swin2SR shell refuses a SwinIR checkpoint, and a cpb_mlp of another width
        Swin2SR(embed_dim=60, depths=[1], num_heads=[6], window_size=8, upsampler="pixelshuffle", mlp_ratio=2.0).load_state_dict(SR.fill(3, 60, (1,), 6, 2.0, 2, "pixelshuffle", "1conv"), strict=True)
    with pytest.raises(RuntimeError):
        Swin2SR(embed_dim=60, depths=[1], num_heads=[6], window_size=8, upsampler="pixelshuffle", mlp_ratio=2.0).load_state_dict(S2.fill(3, 60, (1,), 6, 2.0, 2, "pixelshuffle", "1conv", 48), strict=True)


@pytest.mark.parametrize("v", VARIANTS, ids=_ids)
def test_swin2sr_checkpoints_are_inferred(v):
    """Everything from the shapes alone: bare and under params_ema / params, with and without the three buffers; the checkpoint handed back loads strictly.  A stored
    relative_coords_table is handed on whole -- also one that differs from the formula -- and without one the formula serves."""
    from innfer_amd.architectures import get_network
    cin, Cc, depths, nH, r, s, ups, resi, cpb = v
    sd = _zeros(v)
    full = dict(sd, **S2.buffers(sd, 48))
    assert len(full) > len(sd) and any(k.endswith("relative_coords_table") for k in full) and any(k.endswith("attn_mask") for k in full)
    other = S2.coords_table(linear=True)
    odd = dict(sd, **S2.buffers(sd, 48, coords=other))
    only_index = {k: t for k, t in full.items() if not k.endswith("relative_coords_table")}
    for wrapped, table in ((sd, None), ({"params_ema": sd}, None), ({"params": sd}, None), (full, S2.coords_table()), ({"params_ema": full}, S2.coords_table()),
                           ({"params": odd}, other), (only_index, None)):
        info = infer_from_state_dict(wrapped)
        assert (info["arch"], info["scale"], info["nf"], info["nb"], info["in_nc"], info["out_nc"]) == ("swin2sr", s, Cc, sum(depths), cin, cin)
        params, coords = _split(info["net_params"])
        assert params == _params(v)
        if table is None:
            assert coords is None
        else:
            assert np.asarray(coords).shape == (1, 15, 15, 2) and np.array_equal(np.asarray(coords, np.float64).reshape(225, 2), table.float().double().numpy())
        assert set(info["state_dict"]) == set(sd)
    if sum(depths) <= 6:
        net = get_network(dict(info["net_params"]))
        net.load_state_dict(info["state_dict"], strict=True)
        assert (net.nf, net.num_heads, net.hidden, net.upsampler, net.upscale, net.resi_connection, net.cpb_hidden) == (Cc, nH, int(Cc * r), ups, s, resi, cpb)
        assert np.allclose(net.coords, S2.coords_table().numpy(), rtol=0, atol=1e-15)          # the formula, where nothing was stored
        net = get_network(dict(infer_from_state_dict(odd)["net_params"]))
        assert np.array_equal(net.coords, other.float().double().numpy())                       # the stored table, where one was


def test_other_families_still_infer_as_before():
    """SwinIR, HAT, ESRGAN, Real-ESRGAN and compact dictionaries sniff as before; a SwinIR dictionary with one stray attn.logit_scale and a HAT dictionary with one still
    meet their refusals, word for word."""
    import _compact_ref as CR
    from innfer_amd.architectures import keys
    v = (3, 60, (2,), 6, 2.0, 2, "pixelshuffle", "1conv")
    swinir = {k: torch.zeros(s) for k, s in SR.shapes(*v).items()}
    assert infer_from_state_dict({"params_ema": swinir})["arch"] == "swinir"
    with pytest.raises(NotImplementedError, match=re.escape("Swin2SR checkpoint (attn.logit_scale: cosine attention, continuous position bias): not built on the HIP path")):
        infer_from_state_dict(dict(swinir, **{B0 + "attn.logit_scale": torch.zeros(6, 1, 1)}))
    hat = {k: torch.zeros(s) for k, s in keys.hat_shapes(3, 60, (1,), 6, 2.0, 2).items()}
    assert infer_from_state_dict(hat)["arch"] == "hat"
    with pytest.raises(NotImplementedError, match=re.escape("HAT-like checkpoint with attn.logit_scale (cosine attention): not built on the HIP path")):
        infer_from_state_dict(dict(hat, **{B0 + "attn.logit_scale": torch.zeros(6, 1, 1)}))
    new = infer_from_state_dict({k: torch.zeros(s) for k, s in keys.mrrdbnet_shapes(nb=23).items()})
    assert (new["arch"], new["scale"], new["nb"]) == ("esrgan", 4, 23) and "model.0.weight" in new["state_dict"]
    assert infer_from_state_dict({k: torch.zeros(s) for k, s in keys.realesrgan_shapes(num_block=2).items()})["arch"] == "realesrgan"
    assert infer_from_state_dict(CR.fill(3, 64, 2, 4, seed=2))["arch"] == "compact"
    # Hugging Face key names are not recognised at all
    with pytest.raises(Exception, match="Could not infer"):
        infer_from_state_dict({"swin2sr.encoder.stages.0.layers.0.attention.self.logit_scale": torch.zeros(6, 1, 1), "swin2sr.first_convolution.weight": torch.zeros(60, 3, 3, 3)})


def test_refusals():
    """Clear NotImplementedErrors that name the reason, raised by the sniffing or the shell's constructor: nothing touches the GPU."""
    from innfer_amd.architectures import get_network
    from innfer_amd.architectures.Swin2SR_arch import Swin2SR
    v = (3, 60, (2,), 6, 2.0, 2, "pixelshuffle", "1conv", 512)
    sd = _zeros(v)
    b1 = "layers.0.residual_group.blocks.1."

    def refused(changed, match):
        with pytest.raises(NotImplementedError, match=match):
            infer_from_state_dict({"params_ema": changed})
    refused(dict(sd, **{"conv_bicubic.weight": torch.zeros(60, 3, 3, 3), "conv_aux.weight": torch.zeros(3, 60, 3, 3), "conv_after_aux.0.weight": torch.zeros(60, 3, 3, 3)}), "pixelshuffle_aux")
    refused(dict(sd, **{"conv_first_hf.0.weight": torch.zeros(60, 64, 3, 3), "layers_hf.0.residual_group.blocks.0.norm1.weight": torch.zeros(60)}), "pixelshuffle_hf")
    refused({k: t for k, t in sd.items() if not k.startswith(("conv_before_upsample", "upsample", "conv_last"))}, "JPEG / denoising")
    refused(dict(sd, absolute_pos_embed=torch.zeros(1, 2304, 60)), "absolute_pos_embed")
    refused({k: t for k, t in sd.items() if not k.startswith("patch_embed.norm")}, "patch_embed.norm")
    refused({k: t for k, t in sd.items() if not k.endswith(("attn.q_bias", "attn.v_bias"))}, "q_bias / attn.v_bias")
    refused({k: t for k, t in sd.items() if not k.endswith("attn.v_bias")}, "q_bias / attn.v_bias")
    refused(dict(sd, **{B0 + "attn.relative_coords_table": torch.zeros(1, 13, 13, 2)}), "window_size 7")             # another window, read off the coords table ..
    refused(dict(sd, **{B0 + "attn.relative_position_index": torch.zeros(256, 256, dtype=torch.long)}), "window_size 16")          # .. or off the index
    refused(dict(sd, **{B0 + "attn.relative_coords_table": torch.zeros(15, 15, 2)}), "relative_coords_table has shape")
    refused(dict(sd, **{B0 + "attn.relative_coords_table": torch.zeros(1, 15, 15, 2), b1 + "attn.relative_coords_table": torch.zeros(1, 15, 15, 3)}), "relative_coords_table has shape")
    refused(dict(sd, **{B0 + "attn.relative_coords_table": torch.zeros(1, 15, 15, 2), b1 + "attn.relative_coords_table": torch.ones(1, 15, 15, 2)}), "differs from")
    bad = SR.position_index()
    bad[3, 5] += 1
    refused(dict(sd, **{b1 + "attn.relative_position_index": bad}), "relative_position_index differs")
    odd = _zeros((3, 60, (2,), 6, 2.0, 2, "pixelshuffledirect", "1conv", 512))          # 40 channels out of upsample.0 of a pixelshuffledirect tail: not 3 times a square
    odd["upsample.0.weight"], odd["upsample.0.bias"] = torch.zeros(40, 60, 3, 3), torch.zeros(40)
    refused(odd, "square")
    # sizes outside the built list: through the sniffing path (the constructor refuses) and directly
    for vv in ((3, 288, (1,), 8, 2.0, 2, "pixelshuffle", "1conv", 512), (3, 216, (1,), 6, 2.0, 2, "pixelshuffle", "1conv", 512), (3, 180, (1,), 10, 2.0, 2, "pixelshuffle", "1conv", 512),
               (3, 240, (1,), 8, 5.0, 2, "pixelshuffle", "1conv", 512), (5, 60, (1,), 6, 2.0, 2, "pixelshuffle", "1conv", 512),
               (3, 60, (1,), 6, 2.0, 8, "pixelshuffle", "1conv", 512)):
        info = infer_from_state_dict(_zeros(vv))
        assert info["arch"] == "swin2sr"
        with pytest.raises(NotImplementedError, match="not built on the HIP path"):
            get_network(dict(info["net_params"]))
    ok = dict(embed_dim=60, depths=[1], num_heads=[6], window_size=8, mlp_ratio=2.0, upscale=2, upsampler="pixelshuffle")
    for what, kw in (("window_size", dict(window_size=16)), ("upsampler", dict(upsampler="")), ("pixelshuffle_aux", dict(upsampler="pixelshuffle_aux")),
                     ("pixelshuffle_hf", dict(upsampler="pixelshuffle_hf")), ("upscale", dict(upsampler="nearest+conv", upscale=3)), ("upscale", dict(upscale=8)),
                     ("ape", dict(ape=True)), ("patch_norm", dict(patch_norm=False)), ("qkv_bias", dict(qkv_bias=False)), ("img_range", dict(img_range=255.0)),
                     ("in_chans", dict(in_chans=5)), ("num_heads", dict(depths=[1, 1], num_heads=[6, 3])), ("embed_dim", dict(embed_dim=64)), ("embed_dim", dict(embed_dim=264, num_heads=[8])),
                     ("embed_dim", dict(embed_dim=240, num_heads=[6])), ("mlp_ratio", dict(embed_dim=240, num_heads=[8], mlp_ratio=4.5)), ("patch_size", dict(patch_size=2)),
                     ("resi_connection", dict(resi_connection="5conv")), ("cpb_hidden", dict(cpb_hidden=0)), ("coords_table", dict(coords_table=np.zeros((1, 13, 13, 2))))):
        with pytest.raises(NotImplementedError, match=what):
            Swin2SR(**dict(ok, **kw))
    net = Swin2SR(**ok)
    assert Swin2SR._has_fp32 is False                       # -no_fp16 is refused by run.py's check of this flag
    with pytest.raises(NotImplementedError, match="Swin2SR is built for the fp16 mode only"):
        net.forward(torch.zeros(1, 3, 8, 8))
    with pytest.raises(NotImplementedError, match="fp16 mode only"):
        net.tile_batch_bytes(1, 16, torch.float32)
    for H, W in ((4, 16), (16, 3), (1, 1), (2, 9)):        # a reflect pad of 8 ceil(n / 8) - n >= n: refused before the device is touched
        with pytest.raises(NotImplementedError, match="reflection"):
            net.forward(torch.zeros(1, 3, H, W, dtype=torch.float16))


def test_new_symbols_are_declared_and_bound():
    """The new entry points: declared in the header as additive under 123, bound in lib.py's SIGNATURES; the ABI revision (now 124); the sources are part of the build."""
    hdr = open(os.path.join(ROOT, "include", "innfer_amd.h")).read()
    lib_py = open(os.path.join(ROOT, "innfer_amd", "lib.py")).read()
    for sym in ("innfer_swin2sr_create", "innfer_net_set_attn_scale", "innfer_window_attention_cos", "innfer_layer_norm_add"):
        assert re.search(r"/\* \(123, additive\)(?:(?!\*/).)*\*/\nint %s\(" % sym, hdr, re.S), sym
        assert '"%s"' % sym in lib_py, sym
    assert re.search(r"^#define INNFER_ABI_VERSION 124$", hdr, re.M)
    net = open(os.path.join(ROOT, "innfer_amd", "csrc", "net.hip")).read()
    assert "net->kind == 7" in net and "win_attn_cos_launch" in net and "layer_norm_add_launch" in net
    assert "Swin2SR is built for the fp16 mode only" in net
    mk = open(os.path.join(ROOT, "Makefile")).read()
    assert "csrc/win_attn.hip" in mk and "csrc/layer_norm.hip" in mk          # (the two new kernels are forms of these files' kernels)
    assert "template <bool COS>" in open(os.path.join(ROOT, "innfer_amd", "csrc", "win_attn.hip")).read()
    assert "bool ADD" in open(os.path.join(ROOT, "innfer_amd", "csrc", "layer_norm.hip")).read()


def test_shell_tables_against_the_definition():
    """What the shell hands the engine beside the convs, taken apart again: the dense bias [nH, 64, 64] equals 16 sigmoid(cpb_mlp(coords)) gathered by the position index and
    tau equals exp(min(logit_scale, ln 100)), both to float32 rounding of the float64 definition (_swin2sr_ref); with a stored coords table it is that table that is used.
    attn.qkv's rows are the checkpoint's, permuted and padded only (no d^-0.5), its bias cat(q_bias, 0, v_bias); everything else is SwinIR's relayout."""
    from innfer_amd.architectures.Swin2SR_arch import Swin2SR, pad64
    from innfer_amd.architectures.SwinIR_arch import relayout
    for name in ("C60 [2,2] direct x2 16x24", "C240 nH8 [2] 3conv nearest+conv x4 16x24", "C64 nH2 [2] pixelshuffle x2 8x8"):
        Cc, nH, depths, shape, ups, s, resi, cpb, seed = S2.FIXTURES[name]
        sd = S2.fixture_sd(name)
        d = Cc // nH
        for stored in (None, S2.coords_table(linear=True)):
            net = Swin2SR(in_chans=3, embed_dim=Cc, depths=list(depths), num_heads=[nH] * len(depths), window_size=8, mlp_ratio=2.0, upscale=s, upsampler=ups,
                          resi_connection=resi, cpb_hidden=cpb, coords_table=None if stored is None else stored.reshape(1, 15, 15, 2).numpy())
            net.load_state_dict(sd, strict=True)
            norms, tables, taus = net.engine_tables()
            blocks = [f"layers.{i}.residual_group.blocks.{j}." for i, dep in enumerate(depths) for j in range(dep)]
            assert norms == ["patch_embed.norm"] + [b + n for b in blocks for n in ("norm1", "norm2")] + ["norm"] and len(tables) == len(taus) == len(blocks)
            above = below = 0
            for b, t, tau in zip(blocks, tables, taus):
                want = S2.bias_table(sd, b, coords=stored).numpy()
                assert t.dtype == np.float32 and t.shape == (nH, 64, 64) and t.flags["C_CONTIGUOUS"]
                assert np.abs(t.astype(np.float64) - want).max() <= 2.0 ** -24 * 16 and float(want.max() - want.min()) > 4.0          # one float32 rounding of values <= 16
                if stored is not None:
                    assert np.abs(want - S2.bias_table(sd, b).numpy()).max() > 0.1                                              # (the stored table matters)
                wt = S2.tau_of(sd, b).numpy()
                assert tau.dtype == np.float32 and tau.shape == (nH,) and np.allclose(tau.astype(np.float64), wt, rtol=2.0 ** -23, atol=0) and float(tau.max()) <= 100.0
                ls = sd[b + "attn.logit_scale"].reshape(-1)
                above, below = above + int((ls > math.log(100.0)).sum()), below + int((ls < math.log(100.0)).sum())
            assert above >= 1 and below >= 1, "the fixture's logit_scale lies on one side of ln 100 only"
        # attn.qkv: index work only
        key = blocks[-1] + "attn.qkv"
        w, bq = net._conv_tensors(key, net.state_dict())
        w0, qb, vb = sd[key + ".weight"].numpy(), sd[blocks[-1] + "attn.q_bias"].numpy(), sd[blocks[-1] + "attn.v_bias"].numpy()
        b0 = np.concatenate([qb, np.zeros(Cc, np.float32), vb])
        assert w.shape == ((3 * nH + 1) // 2 * 64, pad64(Cc), 1, 1) and w.dtype == np.float32 and bq.dtype == np.float32
        real = np.zeros(w.shape[0], bool)
        for which in range(3):
            for h in range(nH):
                dst, src = slice((which * nH + h) * 32, (which * nH + h) * 32 + d), slice(which * Cc + h * d, which * Cc + (h + 1) * d)
                assert np.array_equal(w[dst, :Cc, 0, 0], w0[src]) and np.array_equal(bq[dst], b0[src])
                real[dst] = True
        assert not w[~real].any() and not bq[~real].any() and not w[:, Cc:].any()
        assert not bq[nH * 32:2 * nH * 32].any()                                                                                # k has no bias
        # a slice of a sliced conv, and a tensor that is SwinIR's
        ws, bs = net._conv_tensors(key + "#1", net.state_dict())
        assert np.array_equal(ws, w[64:128]) and np.array_equal(bs, bq[64:128])
        pk = blocks[0] + "attn.proj"
        wp, bp = net._conv_tensors(pk, net.state_dict())
        wr, br = relayout(pk, sd[pk + ".weight"].numpy(), sd[pk + ".bias"].numpy(), Cc, nH, 2 * Cc, 3, s, ups == "pixelshuffledirect")
        assert np.array_equal(wp, wr) and np.array_equal(bp, br)


@pytest.mark.parametrize("name", list(S2.FIXTURES))
def test_storage_model_is_what_the_gpu_tests_take_it_for(name):
    """Guards the test data of tests/test_gpu_swin2sr.py: on every network fixture the fp16 storage model alone has ALL its uint8 codes within +-1 of float64 (its max error
    is printed: the GPU tests allow the engine twice that), something IS rounded, and the attention matters: at least half of the softmax rows are peaked.
    Figures of this fill (max |err| of the storage model; share of rows with largest p > 0.5), 100 % of the codes within +-1 everywhere:
        C60 [2,2] direct x2 16x24 3.36e-3, 0.639 | C60 [2] direct x4 13x21 2.36e-3, 0.684 | C180 pixelshuffle x4 16x16 1.48e-3, 0.570 | C180 pixelshuffle x3 9x17 1.58e-3, 0.601 |
        C240 nH8 3conv nearest+conv x4 16x24 1.37e-3, 0.562 | C64 nH2 pixelshuffle x2 8x8 1.17e-3, 0.637 | C60 batch of two pixelshuffle x2 19x26 2.88e-3, 0.726
    (tau = 100 on unit vectors turns the fp16 rounding of q and k, 2^-11 relative, into 0.05 in a score: the narrow heads of C60, d = 10, feel it most)."""
    Cc, nH, depths, shape, ups, s, resi, cpb, seed = S2.FIXTURES[name]
    sd, x, y64, ys = S2.case(name)
    err = float((ys - y64).abs().max())
    share = S2.codes_within_one(ys, y64)
    peaked = S2.peaked_share(sd, x, s, ups)
    print(f"swin2sr {name} (seed {seed}): storage model max|err| {err:.2e}, codes within +-1 {share:.5f}, range [{float(y64.min()):.3f}, {float(y64.max()):.3f}]; "
          f"softmax rows with max p > 0.5: {peaked:.3f}")
    assert tuple(y64.shape) == (shape[0], 3, shape[2] * s, shape[3] * s) and torch.isfinite(y64).all()
    assert share == 1.0, (name, share)
    assert err >= 2.0 ** -13, (name, err)                   # fp16 storage costs something: the model is not float64 by accident
    assert peaked >= 0.5, (name, peaked)


def test_planted_faults_move_the_result():
    """Each mistake a Swin2SR engine can make -- the cosine's normalisation left out, tau not clamped, the norm in front of the branch, the bias without its sigmoid, a
    bias on k, linear coordinates, and SwinIR's five -- moves forward64 by at least 10 x the storage model's error on at least one fixture.  Worst fixture of each, in
    units of the storage model's error there: no_qk_norm 313, no_clamp 32, pre_norm 295, no_sigmoid 202, k_bias 95, coords_linear 166, no_shift 180, no_mask 162,
    bias_T 292, roll_sign 201, ln_pad 23 (roll_sign and ln_pad are 0 on C64 8x8: one window that wraps onto itself, no pad channels)."""
    worst = {f: 0.0 for f in FAULTS}
    for name in ("C60 [2] direct x4 13x21 (padded)", "C180 [2] pixelshuffle x3 9x17", "C64 nH2 [2] pixelshuffle x2 8x8"):
        Cc, nH, depths, shape, ups, s, resi, cpb, seed = S2.FIXTURES[name]
        sd, x, y64, ys = S2.case(name)
        es = float((ys - y64).abs().max())
        for f in FAULTS:
            r = float((S2.forward64(sd, x, s, ups, fault=f) - y64).abs().max()) / es
            print(f"swin2sr fault {f} on {name}: {r:.1f} x the storage model's error")
            worst[f] = max(worst[f], r)
    assert all(r >= 10.0 for r in worst.values()), worst
