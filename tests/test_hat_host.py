"""HAT: the host logic (no GPU) -- the key table, strict loading, checkpoint sniffing with and without the index buffers, the refusals, the new symbols, the engine's
tensors taken apart again, stored against formula indices, and the test data's own figures: the storage model's error, the share of peaked softmax rows, and what each
planted fault costs."""
import os
import re

import numpy as np
import pytest
import torch

import _hat_ref as HR
import _swinir_ref as SR
from innfer_amd import synth
from innfer_amd.run import infer_from_state_dict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (in_chans, C, depths, nH, mlp_ratio, s, compress_ratio, squeeze_factor): HAT, HAT-S, HAT-L's width, and small ones
VARIANTS = [(3, 180, (6,) * 6, 6, 2.0, 4, 3, 30), (3, 144, (6,) * 6, 6, 2.0, 4, 24, 24), (3, 180, (6,) * 12, 6, 2.0, 2, 3, 30), (1, 64, (2, 1), 2, 4.0, 3, 4, 16),
            (4, 96, (1, 2), 4, 1.5, 3, 3, 32), (3, 60, (2,), 6, 2.0, 2, 3, 30)]
FAULTS = ("no_shift", "no_mask", "sa_bias_T", "oca_bias_T", "oca_skip", "oca_origin", "roll_sign", "no_conv_scale", "pool_unpadded", "y_per_pixel", "ln_pad")


def _zeros(v):
    return {k: torch.zeros(s) for k, s in HR.shapes(*v).items()}


def _ids(v):
    return f"in{v[0]}-C{v[1]}-{len(v[2])}x-nH{v[3]}-r{v[4]}-x{v[5]}-c{v[6]}-s{v[7]}"


def test_key_table_and_strict_loading():
    """hat_shapes == the definition written out in _hat_ref; the shell's state dict has exactly those keys (no buffers) and loads a filled one strictly."""
    from innfer_amd.architectures.HAT_arch import HAT
    for v in VARIANTS:
        cin, Cc, depths, nH, r, s, cr, sq = v
        want = HR.shapes(*v)
        assert synth.hat_shapes(cin, Cc, depths, nH, r, s, cr, sq) == want
        if sum(depths) > 6:
            continue
        net = HAT(in_chans=cin, embed_dim=Cc, depths=depths, num_heads=[nH] * len(depths), window_size=16, compress_ratio=cr, squeeze_factor=sq, mlp_ratio=r, upscale=s,
                  upsampler="pixelshuffle")
        assert {k: tuple(t.shape) for k, t in net.state_dict().items()} == {k: tuple(sh) for k, sh in want.items()}
        net.load_state_dict(HR.fill(*v, seed=5), strict=True)


@pytest.mark.parametrize("v", VARIANTS, ids=_ids)
def test_hat_checkpoints_are_inferred(v):
    """Everything from the shapes alone: bare and under params_ema / params, with and without the two index buffers (dropped from the state dict handed back and passed on
    as rpi_sa / rpi_oca); conv_scale is 0.01; the checkpoint handed back loads strictly."""
    from innfer_amd.architectures import get_network
    cin, Cc, depths, nH, r, s, cr, sq = v
    sd = _zeros(v)
    full = dict(sd, **HR.buffers())
    for wrapped in (sd, {"params_ema": sd}, {"params": sd}, full, {"params_ema": full}):
        info = infer_from_state_dict(wrapped)
        assert (info["arch"], info["scale"], info["nf"], info["nb"], info["in_nc"], info["out_nc"]) == ("hat", s, Cc, sum(depths), cin, cin)
        p = dict(info["net_params"])
        stored = "relative_position_index_SA" in (wrapped.get("params_ema") or wrapped.get("params") or wrapped)
        sa, oca = p.pop("rpi_sa"), p.pop("rpi_oca")
        assert (sa is not None) == stored and (oca is not None) == stored
        if stored:
            assert np.array_equal(sa, HR.index_sa().numpy()) and np.array_equal(oca, HR.index_oca().numpy())
        assert Cc // p.pop("compress_ratio") == Cc // cr and Cc // p.pop("squeeze_factor") == Cc // sq
        assert p == dict(type="hat", in_chans=cin, embed_dim=Cc, depths=list(depths), num_heads=[nH] * len(depths), window_size=16, conv_scale=0.01, overlap_ratio=0.5,
                         mlp_ratio=r, upscale=s, img_range=1.0, upsampler="pixelshuffle", resi_connection="1conv")
        assert set(info["state_dict"]) == set(sd)
    if sum(depths) <= 6:
        net = get_network(dict(info["net_params"]))
        net.load_state_dict(info["state_dict"], strict=True)
        assert (net.nf, net.num_heads, net.hidden, net.upscale, net.compress_ch, net.squeeze_ch, net.conv_scale) == (Cc, nH, int(Cc * r), s, Cc // cr, Cc // sq, 0.01)
        other = get_network(dict(info["net_params"], conv_scale=1.0))          # net_params take another conv_scale
        assert other.conv_scale == 1.0


def test_other_families_still_infer_as_before():
    """An incomplete HAT key set falls through to the sniffing as it was: the two SwinIR-plus-one-stray-key dictionaries still raise "HAT / DRCT", a SwinIR is a SwinIR, and
    conv_first.weight alone is still a new-arch ESRGAN."""
    import _compact_ref as CR
    from innfer_amd.architectures import keys
    v = (3, 60, (2,), 6, 2.0, 2, "pixelshuffle", "1conv")
    sd = {k: torch.zeros(s) for k, s in SR.shapes(*v).items()}
    assert infer_from_state_dict({"params_ema": sd})["arch"] == "swinir"
    for stray in ({"layers.0.residual_group.overlap_attn.qkv.weight": torch.zeros(180, 60)}, {"layers.0.residual_group.blocks.0.conv_block.cab.0.weight": torch.zeros(20, 60, 3, 3)}):
        with pytest.raises(NotImplementedError, match="HAT / DRCT"):
            infer_from_state_dict({"params_ema": dict(sd, **stray)})
    hat = _zeros(VARIANTS[-1])
    for k in ("layers.0.residual_group.overlap_attn.relative_position_bias_table", "layers.0.residual_group.blocks.0.conv_block.cab.3.attention.3.weight"):
        with pytest.raises(NotImplementedError, match="HAT / DRCT"):          # a HAT without one key of the set is not taken for a HAT
            infer_from_state_dict({k2: t for k2, t in hat.items() if k2 != k})
    new = infer_from_state_dict({k: torch.zeros(s) for k, s in keys.mrrdbnet_shapes(nb=23).items()})
    assert (new["arch"], new["scale"], new["nb"]) == ("esrgan", 4, 23)
    assert infer_from_state_dict({k: torch.zeros(s) for k, s in keys.realesrgan_shapes(num_block=2).items()})["arch"] == "realesrgan"
    assert infer_from_state_dict(CR.fill(3, 64, 2, 4, seed=2))["arch"] == "compact"


def test_refusals():
    """Clear NotImplementedErrors, raised by the sniffing or the shell's constructor: nothing touches the GPU."""
    from innfer_amd.architectures import get_network
    from innfer_amd.architectures.HAT_arch import HAT
    v = (3, 60, (2,), 6, 2.0, 2, 3, 30)
    sd = _zeros(v)
    b0 = "layers.0.residual_group.blocks.0."

    def refused(changed, match):
        with pytest.raises(NotImplementedError, match=match):
            infer_from_state_dict({"params_ema": changed})
    refused(dict(sd, absolute_pos_embed=torch.zeros(1, 2304, 60)), "absolute_pos_embed")
    refused(dict(sd, **{"layers.0.swin_DRCT.x": torch.zeros(1)}), "DRCT")
    refused({k: t for k, t in sd.items() if not k.startswith("patch_embed.norm")}, "patch_embed.norm")
    refused({k: t for k, t in sd.items() if not k.endswith("qkv.bias")}, "qkv biases")
    refused({k: t for k, t in sd.items() if not k.startswith(("conv_before_upsample", "upsample", "conv_last"))}, "pixelshuffle tail")
    w8 = dict(sd)
    for k in sd:
        if k.endswith("attn.relative_position_bias_table"):
            w8[k] = torch.zeros(225, 6)
    refused(w8, "window_size 8")
    o20 = dict(sd)
    for k in sd:
        if k.endswith("overlap_attn.relative_position_bias_table"):
            o20[k] = torch.zeros(35 * 35, 6)
    refused(o20, "overlapping window of 20")
    refused(dict(sd, relative_position_index_OCA=torch.zeros(256, 400, dtype=torch.long)), "relative_position_index_OCA has shape")
    bad = HR.buffers()
    bad["relative_position_index_OCA"] = bad["relative_position_index_OCA"].clone()
    bad["relative_position_index_OCA"][3, 5] = 1521          # outside [-rows, rows): the constructor refuses
    info = infer_from_state_dict(dict(sd, **bad))
    with pytest.raises(NotImplementedError, match="does not address"):
        get_network(info["net_params"])
    bad["relative_position_index_OCA"][3, 5] = -1521          # the torch wrap rule reaches the first row: fine
    get_network(dict(infer_from_state_dict(dict(sd, **bad))["net_params"]))
    # sizes outside the built list: through the sniffing path (the constructor refuses) and directly
    for vv in ((3, 288, (1,), 8, 2.0, 2, 6, 30), (3, 216, (1,), 6, 2.0, 2, 4, 30), (3, 180, (1,), 10, 2.0, 2, 3, 30), (3, 240, (1,), 8, 5.0, 2, 4, 30), (5, 60, (1,), 6, 2.0, 2, 3, 30),
               (3, 60, (1,), 6, 2.0, 8, 3, 30)):
        info = infer_from_state_dict(_zeros(vv))
        assert info["arch"] == "hat"
        with pytest.raises(NotImplementedError, match="not built on the HIP path"):
            get_network(info["net_params"])
    refused(_zeros((3, 240, (1,), 8, 2.0, 2, 2, 30)), "conv block of 120 channels")          # C / compress_ratio > 64
    refused(_zeros((3, 240, (1,), 8, 2.0, 2, 4, 3)), "channel attention of 80")              # C / squeeze_factor > 64
    ok = dict(embed_dim=60, depths=[1], num_heads=[6], window_size=16, mlp_ratio=2.0, upscale=2, upsampler="pixelshuffle")
    for what, kw in (("window_size", dict(window_size=8)), ("overlap_ratio", dict(overlap_ratio=0.25)), ("upsampler", dict(upsampler="pixelshuffledirect")), ("upscale", dict(upscale=8)),
                     ("ape", dict(ape=True)), ("patch_norm", dict(patch_norm=False)), ("qkv_bias", dict(qkv_bias=False)), ("img_range", dict(img_range=255.0)),
                     ("in_chans", dict(in_chans=5)), ("num_heads", dict(depths=[1, 1], num_heads=[6, 3])), ("embed_dim", dict(embed_dim=264, num_heads=[8])),
                     ("mlp_ratio", dict(embed_dim=240, num_heads=[8], mlp_ratio=4.5)), ("patch_size", dict(patch_size=2)), ("resi_connection", dict(resi_connection="3conv")),
                     ("compress_ratio", dict(embed_dim=240, num_heads=[8], compress_ratio=3)), ("squeeze_factor", dict(embed_dim=240, num_heads=[8], compress_ratio=4, squeeze_factor=3))):
        with pytest.raises(NotImplementedError, match=what):
            HAT(**dict(ok, **kw))
    net = HAT(**ok)
    assert HAT._has_fp32 is False                          # -no_fp16 is refused by run.py's check of this flag
    with pytest.raises(NotImplementedError, match="HAT is built for the fp16 mode only"):
        net.forward(torch.zeros(1, 3, 16, 16))
    with pytest.raises(NotImplementedError, match="fp16 mode only"):
        net.tile_batch_bytes(1, 16, torch.float32)
    for H, W in ((8, 16), (16, 7), (1, 1), (2, 33)):       # a reflect pad of 16 ceil(n / 16) - n >= n: torch refuses it, so does the shell, before the device is touched
        with pytest.raises(NotImplementedError, match="reflection"):
            net.forward(torch.zeros(1, 3, H, W, dtype=torch.float16))
        with pytest.raises(RuntimeError):
            torch.nn.functional.pad(torch.zeros(1, 3, H, W), (0, -W % 16, 0, -H % 16), mode="reflect")


def test_new_symbols_are_declared_and_bound():
    """The new entry points: declared in the header as additive under 123, bound in lib.py's SIGNATURES; the ABI revision (now 124); the sources are part of the build;
    win_attn.hip is the SwinIR commit's, untouched."""
    hdr = open(os.path.join(ROOT, "include", "innfer_amd.h")).read()
    lib_py = open(os.path.join(ROOT, "innfer_amd", "lib.py")).read()
    for sym in ("innfer_hat_create", "innfer_net_set_chan_attn", "innfer_net_set_conv_scale", "innfer_window_attention16"):
        assert re.search(r"/\* \(123, additive\)(?:(?!\*/).)*\*/\nint %s\(" % sym, hdr, re.S), sym
        assert '"%s"' % sym in lib_py, sym
    for sym in ("innfer_chan_attn_work_bytes", "innfer_chan_attn_excite", "innfer_chan_attn_scale_add"):
        assert re.search(r"^(int|size_t) %s\(" % sym, hdr, re.M) and '"%s"' % sym in lib_py, sym
    assert re.search(r"^#define INNFER_ABI_VERSION 124$", hdr, re.M)
    assert "act = 13" in hdr
    net = open(os.path.join(ROOT, "innfer_amd", "csrc", "net.hip")).read()
    assert "net->kind == 6" in net and "win_attn16_launch" in net and "ca_scale_add_launch" in net
    mk = open(os.path.join(ROOT, "Makefile")).read()
    assert "csrc/win_attn16.hip" in mk and "csrc/chan_attn.hip" in mk and "csrc/win_attn.hip" in mk


def test_stored_and_formula_indices_give_the_same_tables():
    """The dense tables the attention reads: built from the stored buffers, from the shell's formulas and from the reference's, they are one and the same -- negative
    entries of the OCA index wrap to the end of the table, as torch indexing does."""
    from innfer_amd.architectures.HAT_arch import HAT, dense_bias_indexed, relative_position_index_oca
    from innfer_amd.architectures.SwinIR_arch import relative_position_index
    assert torch.equal(relative_position_index(16), HR.index_sa()) and torch.equal(relative_position_index_oca(), HR.index_oca())
    oca = HR.index_oca()
    assert int(oca.min()) == -22 * 39 - 22 and int(oca.max()) == 16 * 39 + 16 and int(HR.index_sa().min()) == 0 and int(HR.index_sa().max()) == 960
    t_sa, t_oca = torch.from_numpy(synth.uniform((961, 6), 1, -1, 1)), torch.from_numpy(synth.uniform((1521, 6), 2, -1, 1))
    want = t_oca[oca.reshape(-1)].reshape(256, 576, 6).permute(2, 0, 1)          # torch's own indexing, negative entries included
    assert np.array_equal(dense_bias_indexed(t_oca.numpy(), oca.numpy()), want.numpy())
    assert np.array_equal(dense_bias_indexed(t_oca.numpy(), (oca % 1521).numpy()), want.numpy())
    name = "C60 [2] x2 16x16 cs1"
    nets = []
    for with_buffers in (True, False):
        info = infer_from_state_dict(HR.fixture_sd(name, with_buffers))
        from innfer_amd.architectures import get_network
        net = get_network(dict(info["net_params"]))
        net.load_state_dict(info["state_dict"], strict=True)
        nets.append(net.engine_tables())
    for a, b in zip(nets[0][1], nets[1][1]):
        assert a.dtype == np.float32 and np.array_equal(a, b)
    assert [t.shape for t in nets[0][1]] == [(6, 256, 256), (6, 256, 256), (6, 256, 576)]
    sd = HR.fixture_sd(name, False)
    assert np.array_equal(nets[0][1][2], HR.dense_table(sd["layers.0.residual_group.overlap_attn.relative_position_bias_table"], oca).numpy())
    assert np.array_equal(nets[0][1][0], HR.dense_table(sd["layers.0.residual_group.blocks.0.attn.relative_position_bias_table"], HR.index_sa()).numpy())
    assert nets[0][0] == ["patch_embed.norm"] + [f"layers.0.residual_group.blocks.{j}.norm{k}" for j in (0, 1) for k in (1, 2)] + \
        ["layers.0.residual_group.overlap_attn.norm1", "layers.0.residual_group.overlap_attn.norm2", "norm"]


def test_engine_tensors_taken_apart_again():
    """What the shell hands the engine for every conv slot (the key order of innfer_hat_create), un-padded, un-permuted and un-folded, is the checkpoint: exactly where the
    re-layout is index work, within one float32 rounding where it folds (d^-0.5 into q, + mean into conv_last's bias); everything the padding adds is zero."""
    from innfer_amd.architectures import get_network
    from innfer_amd.architectures.HAT_arch import pad64
    from test_swinir_host import _undo
    for name in ("C60 [2] x2 16x16 cs1", "C144 [2] x2 batch of two 19x26 cs1 (formula indices)"):
        Cc, nH, depths, shape, s, cr, sq, cs, stored, seed = HR.FIXTURES[name]
        info = infer_from_state_dict(HR.fixture_sd(name))
        net = get_network(dict(info["net_params"], conv_scale=cs))
        net.load_state_dict(info["state_dict"], strict=True)
        sd = net.state_dict()
        d, hidden, Cp = Cc // nH, 2 * Cc, pad64(Cc)
        for key in sorted({k.rsplit(".", 1)[0] for k, t in sd.items() if t.dim() in (2, 4) and not k.endswith("bias_table") and ".attention." not in k}):
            w0, b0 = sd[key + ".weight"].numpy(), sd[key + ".bias"].numpy()
            w, b = net._conv_tensors(key, sd)
            assert w.dtype == np.float32 and b.dtype == np.float32 and w.ndim == 4 and w.shape[0] == b.shape[0]
            assert np.array_equal(net._conv_tensors(key + "#0", sd)[0], w[:64])
            un = _undo(key, w, b, Cc, nH, hidden, 3, s, False)
            if un is not None:
                wu, bu = un
                if key.endswith("qkv"):
                    assert w.shape == ((3 * nH + 1) // 2 * 64, Cp, 1, 1)
                    assert np.array_equal(wu[Cc:], w0[Cc:]) and np.array_equal(bu[Cc:], b0[Cc:])
                    assert np.allclose(wu[:Cc], w0[:Cc], rtol=2.0 ** -22, atol=0) and np.allclose(bu[:Cc], b0[:Cc], rtol=2.0 ** -22, atol=0)
                else:
                    assert np.array_equal(wu, w0.reshape(wu.shape)) and np.array_equal(bu, b0)
                assert np.count_nonzero(w) == np.count_nonzero(w0) and np.count_nonzero(b) == np.count_nonzero(b0)          # everything the padding adds is zero
            elif key == "conv_last":
                assert np.array_equal(w, w0) and np.allclose(b - np.float32(HR.MEAN), b0, rtol=0, atol=2.0 ** -24)
            else:
                assert np.array_equal(w[:w0.shape[0], :w0.shape[1]], w0) and np.array_equal(b[:b0.shape[0]], b0)
                assert np.count_nonzero(w) == np.count_nonzero(w0) and not b[b0.shape[0]:].any()
                if key.endswith("cab.0"):
                    assert w.shape == (64, Cp, 3, 3)
                if key.endswith("cab.2"):
                    assert w.shape == (Cp, 64, 3, 3)
        norms, tables, cas = net.engine_tables()
        assert len(cas) == sum(depths) and len(tables) == sum(depths) + len(depths) and len(norms) == 2 + 2 * (sum(depths) + len(depths))
        a = "layers.0.residual_group.blocks.1.conv_block.cab.3.attention."
        w1, b1, w2, b2 = cas[1]
        assert w1.shape == (Cc // sq, Cc) and w2.shape == (Cc, Cc // sq) and b1.size == Cc // sq and b2.size == Cc
        assert np.array_equal(w1, sd[a + "1.weight"].numpy()[:, :, 0, 0]) and np.array_equal(w2, sd[a + "3.weight"].numpy()[:, :, 0, 0])
        assert np.array_equal(b1.reshape(-1), sd[a + "1.bias"].numpy()) and np.array_equal(b2.reshape(-1), sd[a + "3.bias"].numpy())


@pytest.mark.parametrize("name", list(HR.FIXTURES))
def test_storage_model_is_what_the_gpu_tests_take_it_for(name):
    """Guards the test data of tests/test_gpu_hat.py: on every network fixture the fp16 storage model alone has >= 99 % of its uint8 codes within +-1 of float64 (its max
    error is printed: the GPU tests allow the engine twice that), something IS rounded, the result is an image that reaches both clips, and the attention matters."""
    Cc, nH, depths, shape, s, cr, sq, cs, stored, seed = HR.FIXTURES[name]
    sd, x, y64, ys = HR.case(name)
    err = float((ys - y64).abs().max())
    share = HR.codes_within_one(ys, y64)
    peaked = HR.peaked_share(sd, x, s, cs)
    print(f"hat {name} (seed {seed}): storage model max|err| {err:.2e}, codes within +-1 {share:.5f}, range [{float(y64.min()):.3f}, {float(y64.max()):.3f}]; "
          f"softmax rows with max p > 0.5: {peaked:.3f}")
    assert tuple(y64.shape) == (shape[0], 3, shape[2] * s, shape[3] * s) and torch.isfinite(y64).all()
    assert share >= 0.99, (name, share)
    assert err >= 2.0 ** -13, (name, err)                   # fp16 storage costs something: the model is not float64 by accident
    assert float(y64.min()) < 0.0 and float(y64.max()) > 0.8
    assert float(y64.min()) > -0.6 and float(y64.max()) < 1.6
    assert peaked > 0.5, (name, peaked)                     # a majority of the softmax rows is peaked
    assert float((HR.forward64(sd, x, s, cs, idx=(HR.index_sa() % 961, HR.index_oca() % 1521)) - y64).abs().max()) == 0.0          # the wrap rule


def test_planted_faults_move_the_result():
    """Each of the eleven mistakes moves forward64 by at least 10 x the storage model's error on at least one fixture: the network tests would see it."""
    worst = {f: 0.0 for f in FAULTS}
    for name in HR.FIXTURES:
        Cc, nH, depths, shape, s, cr, sq, cs, stored, seed = HR.FIXTURES[name]
        sd, x, y64, ys = HR.case(name)
        es = float((ys - y64).abs().max())
        for f in FAULTS:
            if worst[f] >= 10.0 and name != "C60 [2] x2 16x16 cs1":
                continue
            r = float((HR.forward64(sd, x, s, cs, fault=f) - y64).abs().max()) / es
            print(f"hat fault {f} on {name}: {r:.1f} x the storage model's error")
            worst[f] = max(worst[f], r)
    assert all(r >= 10.0 for r in worst.values()), worst
