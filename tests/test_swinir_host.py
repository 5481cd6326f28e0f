"""SwinIR: the host logic (no GPU) -- the key table, strict loading, checkpoint sniffing with and without the buffers, the refusals, the new symbols, the re-layout, and the
test data's own figures: the storage model's error, the share of peaked softmax rows, and what each planted fault costs."""
import os
import re

import numpy as np
import pytest
import torch

import _swinir_ref as SR
from innfer_amd import synth
from innfer_amd.run import infer_from_state_dict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (in_chans, C, depths, nH, mlp_ratio, s, upsampler, resi)
VARIANTS = [(3, 180, (6,) * 6, 6, 2.0, 4, "pixelshuffle", "1conv"), (3, 60, (6,) * 4, 6, 2.0, 2, "pixelshuffledirect", "1conv"), (3, 180, (6,) * 6, 6, 2.0, 4, "nearest+conv", "1conv"),
            (3, 240, (6,) * 9, 8, 2.0, 4, "nearest+conv", "3conv"), (1, 64, (2, 1), 2, 4.0, 3, "pixelshuffle", "3conv"), (4, 96, (1, 2, 3), 4, 1.5, 3, "pixelshuffledirect", "1conv"),
            (3, 60, (2,), 6, 2.0, 2, "nearest+conv", "1conv"), (3, 60, (2,), 6, 2.0, 2, "pixelshuffle", "1conv")]
FAULTS = ("no_shift", "no_mask", "no_bias", "bias_T", "roll_sign", "ln_pad")


def _zeros(v):
    return {k: torch.zeros(s) for k, s in SR.shapes(*v).items()}


def _ids(v):
    return f"in{v[0]}-C{v[1]}-{len(v[2])}x-nH{v[3]}-r{v[4]}-x{v[5]}-{v[6]}-{v[7]}"


def test_key_table_and_strict_loading():
    """swinir_shapes == the definition written out in _swinir_ref; the shell's state dict has exactly those keys (no buffers) and loads a filled one strictly."""
    from innfer_amd.architectures.SwinIR_arch import SwinIR
    for v in VARIANTS:
        cin, Cc, depths, nH, r, s, ups, resi = v
        want = SR.shapes(*v)
        assert synth.swinir_shapes(cin, Cc, depths, nH, r, s, ups, resi) == want
        if sum(depths) > 6:
            continue
        net = SwinIR(in_chans=cin, embed_dim=Cc, depths=depths, num_heads=[nH] * len(depths), window_size=8, mlp_ratio=r, upscale=s, upsampler=ups, resi_connection=resi)
        assert {k: tuple(t.shape) for k, t in net.state_dict().items()} == {k: tuple(sh) for k, sh in want.items()}
        net.load_state_dict(SR.fill(*v, seed=5), strict=True)
    with pytest.raises(RuntimeError):          # a '3conv' shell refuses a '1conv' checkpoint
        SwinIR(embed_dim=60, depths=[1], num_heads=[6], window_size=8, upsampler="pixelshuffle", resi_connection="3conv").load_state_dict(SR.fill(3, 60, (1,), 6, 4.0, 2, "pixelshuffle", "1conv"), strict=True)


@pytest.mark.parametrize("v", VARIANTS, ids=_ids)
def test_swinir_checkpoints_are_inferred(v):
    """Everything from the shapes alone: bare and under params_ema / params, with and without the two buffers; the checkpoint handed back loads strictly."""
    from innfer_amd.architectures import get_network
    cin, Cc, depths, nH, r, s, ups, resi = v
    sd = _zeros(v)
    full = dict(sd, **SR.buffers(sd, 48))
    assert len(full) > len(sd)
    for wrapped in (sd, {"params_ema": sd}, {"params": sd}, full, {"params_ema": full}):
        info = infer_from_state_dict(wrapped)
        assert (info["arch"], info["scale"], info["nf"], info["nb"], info["in_nc"], info["out_nc"]) == ("swinir", s, Cc, sum(depths), cin, cin)
        assert info["net_params"] == dict(type="swinir", in_chans=cin, embed_dim=Cc, depths=list(depths), num_heads=[nH] * len(depths), window_size=8, mlp_ratio=r,
                                          upscale=s, img_range=1.0, upsampler=ups, resi_connection=resi)
        assert set(info["state_dict"]) == set(sd)
    if sum(depths) <= 6:
        net = get_network(info["net_params"])
        net.load_state_dict(info["state_dict"], strict=True)
        assert (net.nf, net.num_heads, net.hidden, net.upsampler, net.upscale, net.resi_connection) == (Cc, nH, int(Cc * r), ups, s, resi)


def test_other_families_still_infer_as_before():
    """conv_first.weight alone is still a new-arch ESRGAN (or BasicSR's RRDBNet): the SwinIR probe sits ahead of it and needs the transformer's keys."""
    import _compact_ref as CR
    from innfer_amd.architectures import keys
    new = infer_from_state_dict({k: torch.zeros(v) for k, v in keys.mrrdbnet_shapes(nb=23).items()})          # (the reference's conversion is written for 23 blocks)
    assert (new["arch"], new["scale"], new["nb"]) == ("esrgan", 4, 23) and "model.0.weight" in new["state_dict"]
    assert infer_from_state_dict({k: torch.zeros(v) for k, v in keys.realesrgan_shapes(num_block=2).items()})["arch"] == "realesrgan"
    assert infer_from_state_dict(CR.fill(3, 64, 2, 4, seed=2))["arch"] == "compact"


def test_refusals():
    """Clear NotImplementedErrors, raised by the sniffing or the shell's constructor: nothing touches the GPU."""
    from innfer_amd.architectures import get_network
    from innfer_amd.architectures.SwinIR_arch import SwinIR
    v = (3, 60, (2,), 6, 2.0, 2, "pixelshuffle", "1conv")
    sd = _zeros(v)
    b0, b1 = "layers.0.residual_group.blocks.0.", "layers.0.residual_group.blocks.1."

    def refused(changed, match):
        with pytest.raises(NotImplementedError, match=match):
            infer_from_state_dict({"params_ema": changed})
    refused(dict(sd, **{b0 + "attn.logit_scale": torch.zeros(6, 1, 1)}), "Swin2SR")
    refused(dict(sd, **{"layers.0.residual_group.overlap_attn.qkv.weight": torch.zeros(180, 60)}), "HAT / DRCT")
    refused(dict(sd, **{b0 + "conv_block.cab.0.weight": torch.zeros(20, 60, 3, 3)}), "HAT / DRCT")
    refused(dict(sd, absolute_pos_embed=torch.zeros(1, 2304, 60)), "absolute_pos_embed")
    w7 = dict(sd)
    for k in sd:
        if k.endswith("relative_position_bias_table"):
            w7[k] = torch.zeros(169, 6)
    refused(w7, "window_size 7")
    refused({k: t for k, t in sd.items() if not k.startswith(("conv_before_upsample", "upsample", "conv_last"))}, "denoising / JPEG")
    refused({k: t for k, t in sd.items() if not k.startswith("patch_embed.norm")}, "patch_embed.norm")
    refused({k: t for k, t in sd.items() if not k.endswith("attn.qkv.bias")}, "qkv.bias")
    bad = SR.position_index()
    bad[3, 5] += 1
    refused(dict(sd, **{b1 + "attn.relative_position_index": bad}), "relative_position_index differs")
    odd = _zeros((3, 60, (2,), 6, 2.0, 2, "pixelshuffledirect", "1conv"))          # 40 channels out of upsample.0 of a pixelshuffledirect tail: not 3 times a square
    odd["upsample.0.weight"], odd["upsample.0.bias"] = torch.zeros(40, 60, 3, 3), torch.zeros(40)
    refused(odd, "square")
    # sizes outside the built list: through the sniffing path (the constructor refuses) and directly
    for vv in ((3, 288, (1,), 8, 2.0, 2, "pixelshuffle", "1conv"), (3, 216, (1,), 6, 2.0, 2, "pixelshuffle", "1conv"), (3, 180, (1,), 10, 2.0, 2, "pixelshuffle", "1conv"),
               (3, 240, (1,), 8, 5.0, 2, "pixelshuffle", "1conv"), (5, 60, (1,), 6, 2.0, 2, "pixelshuffle", "1conv"),
               (3, 60, (1,), 6, 2.0, 8, "pixelshuffle", "1conv")):
        info = infer_from_state_dict(_zeros(vv))
        assert info["arch"] == "swinir"
        with pytest.raises(NotImplementedError, match="not built on the HIP path"):
            get_network(info["net_params"])
    ok = dict(embed_dim=60, depths=[1], num_heads=[6], window_size=8, mlp_ratio=2.0, upscale=2, upsampler="pixelshuffle")
    for what, kw in (("window_size", dict(window_size=7)), ("upsampler", dict(upsampler="")), ("upscale", dict(upsampler="nearest+conv", upscale=3)), ("upscale", dict(upscale=8)),
                     ("ape", dict(ape=True)), ("patch_norm", dict(patch_norm=False)), ("qkv_bias", dict(qkv_bias=False)), ("img_range", dict(img_range=255.0)),
                     ("in_chans", dict(in_chans=5)), ("num_heads", dict(depths=[1, 1], num_heads=[6, 3])), ("embed_dim", dict(embed_dim=64)), ("embed_dim", dict(embed_dim=264, num_heads=[8])),
                     ("embed_dim", dict(embed_dim=240, num_heads=[6])), ("mlp_ratio", dict(embed_dim=240, num_heads=[8], mlp_ratio=4.5)), ("patch_size", dict(patch_size=2)),
                     ("resi_connection", dict(resi_connection="5conv"))):
        with pytest.raises(NotImplementedError, match=what):
            SwinIR(**dict(ok, **kw))
    net = SwinIR(**ok)
    assert SwinIR._has_fp32 is False                       # -no_fp16 is refused by run.py's check of this flag
    with pytest.raises(NotImplementedError, match="fp16 mode only"):
        net.forward(torch.zeros(1, 3, 8, 8))
    with pytest.raises(NotImplementedError, match="fp16 mode only"):
        net.tile_batch_bytes(1, 16, torch.float32)
    for H, W in ((4, 16), (16, 3), (1, 1), (2, 9)):        # a reflect pad of 8 ceil(n / 8) - n >= n: torch refuses it, so does the shell, before the device is touched
        with pytest.raises(NotImplementedError, match="reflection"):
            net.forward(torch.zeros(1, 3, H, W, dtype=torch.float16))
        with pytest.raises(RuntimeError):
            torch.nn.functional.pad(torch.zeros(1, 3, H, W), (0, -W % 8, 0, -H % 8), mode="reflect")


def test_new_symbols_are_declared_and_bound():
    """The new entry points: declared in the header as additive under 123, bound in lib.py's SIGNATURES; the ABI revision (now 124); the sources are part of the build."""
    hdr = open(os.path.join(ROOT, "include", "innfer_amd.h")).read()
    lib_py = open(os.path.join(ROOT, "innfer_amd", "lib.py")).read()
    for sym in ("innfer_swinir_create", "innfer_net_set_layer_norm", "innfer_net_set_attn_bias", "innfer_window_attention", "innfer_layer_norm"):
        assert re.search(r"/\* \(123, additive\)(?:(?!\*/).)*\*/\nint %s\(" % sym, hdr, re.S), sym
        assert '"%s"' % sym in lib_py, sym
    assert re.search(r"^#define INNFER_ABI_VERSION 124$", hdr, re.M)
    assert "act = 12 (GELU" in hdr
    net = open(os.path.join(ROOT, "innfer_amd", "csrc", "net.hip")).read()
    assert "swinir_forward" in net and "net->kind == 5" in net
    mk = open(os.path.join(ROOT, "Makefile")).read()
    assert "csrc/win_attn.hip" in mk and "csrc/layer_norm.hip" in mk
    modes = open(os.path.join(ROOT, "innfer_amd", "csrc", "conv3x3_modes.h")).read()
    assert "PC_GELU" in modes


def _undo(key, w, b, Cc, nH, hidden, cin, s, direct):
    """The inverse of SwinIR_arch.relayout on the engine's tensors: un-pad, un-permute, un-fold (in float64)."""
    from innfer_amd.architectures.SwinIR_arch import RGB_MEAN
    d = Cc // nH
    w, b = w.astype(np.float64), b.astype(np.float64)
    mean = np.asarray(RGB_MEAN if cin == 3 else (0.0,) * cin, np.float64)
    if key.endswith("attn.qkv"):
        wo, bo = np.zeros((3 * Cc, Cc)), np.zeros(3 * Cc)
        for which in range(3):
            for h in range(nH):
                src = slice((which * nH + h) * 32, (which * nH + h) * 32 + d)
                dst = slice(which * Cc + h * d, which * Cc + (h + 1) * d)
                sc = float(np.float32(d ** -0.5)) if which == 0 else 1.0
                wo[dst], bo[dst] = w[src, :Cc, 0, 0] / sc, b[src] / sc
        return wo, bo
    if key.endswith("attn.proj"):
        wo = np.concatenate([w[:Cc, 32 * h:32 * h + d, 0, 0] for h in range(nH)], 1)
        return wo, b[:Cc]
    if key.endswith("mlp.fc1"):
        return w[:hidden, :Cc, 0, 0], b[:hidden]
    if key.endswith("mlp.fc2"):
        return w[:Cc, :hidden, 0, 0], b[:Cc]
    return None


def test_relayout_applied_and_undone():
    """The engine's weights (head permutation, padding to multiples of 64, d^-0.5 and mean folds) taken apart again give the checkpoint back: exactly where the re-layout
    is index work, within one float32 rounding where it folds (q rows and biases, the last conv's bias); everything the padding adds is zero.  forward64 on the recovered
    checkpoint is forward64 on the original within 1e-6."""
    from innfer_amd.architectures.SwinIR_arch import relayout, pad64
    for name in ("C60 [2,2] direct x2 16x24", "C240 [2] 3conv nearest+conv x4 16x24"):
        Cc, nH, depths, shape, ups, s, resi, seed = SR.FIXTURES[name]
        sd, x, y64, _ = SR.case(name)
        d, hidden, direct = Cc // nH, 2 * Cc, ups == "pixelshuffledirect"
        back = dict(sd)
        for key in sorted({k.rsplit(".", 1)[0] for k, t in sd.items() if t.dim() in (2, 4) and not k.endswith("bias_table")}):
            w0, b0 = sd[key + ".weight"].numpy(), sd[key + ".bias"].numpy()
            w, b = relayout(key, w0, b0, Cc, nH, hidden, 3, s, direct)
            assert w.dtype == np.float32 and b.dtype == np.float32 and w.ndim == 4 and w.shape[0] == b.shape[0]
            un = _undo(key, w, b, Cc, nH, hidden, 3, s, direct)
            if un is not None:
                wu, bu = un
                if key.endswith("attn.qkv"):
                    assert w.shape == ((3 * nH + 1) // 2 * 64, pad64(Cc), 1, 1)
                    assert np.array_equal(wu[Cc:], w0[Cc:]) and np.array_equal(bu[Cc:], b0[Cc:])               # k and v: index work only
                    assert np.allclose(wu[:Cc], w0[:Cc], rtol=2.0 ** -22, atol=0) and np.allclose(bu[:Cc], b0[:Cc], rtol=2.0 ** -22, atol=0)
                    assert not w[:, Cc:].any()                                                                  # the padded columns are zero
                    real = np.zeros(w.shape[0], bool)
                    for g in range(3 * nH):
                        real[32 * g:32 * g + d] = True
                    assert not w[~real].any() and not b[~real].any()                                            # the padded rows are zero
                else:
                    assert np.array_equal(wu, w0.reshape(wu.shape)) and np.array_equal(bu, b0)
                    assert np.count_nonzero(w) == np.count_nonzero(wu) and np.count_nonzero(b) == np.count_nonzero(bu)          # everything the padding adds is zero
                back[key + ".weight"], back[key + ".bias"] = torch.from_numpy(wu.reshape(w0.shape).astype(np.float32)), torch.from_numpy(bu.astype(np.float32))
            elif key in ("conv_last", "upsample.0") and (key == "conv_last" or direct):
                rep = s * s if direct else 1
                assert np.array_equal(w[:w0.shape[0], :w0.shape[1]], w0) and np.allclose(b - np.repeat(np.float32(SR.MEAN), rep), b0, rtol=0, atol=2.0 ** -24)
            else:                                        # convs: zero padding only
                assert np.array_equal(w[:w0.shape[0], :w0.shape[1]], w0) and np.array_equal(b[:b0.shape[0]], b0)
                assert np.count_nonzero(w) == np.count_nonzero(w0) and not b[b0.shape[0]:].any()
                assert w.shape[0] % 64 == 0 or key in ("conv_last", "upsample.0", "upsample.2") or w.shape[0] in (256, 576)
        assert float((SR.forward64(back, x, s, ups) - y64).abs().max()) < 1e-6


@pytest.mark.parametrize("name", list(SR.FIXTURES))
def test_storage_model_is_what_the_gpu_tests_take_it_for(name):
    """Guards the test data of tests/test_gpu_swinir.py: on every network fixture the fp16 storage model alone has ALL its uint8 codes within +-1 of float64 (its max error
    is printed: the GPU tests allow the engine twice that), something IS rounded, the result is an image that reaches both clips, and the attention matters: a good share
    of the softmax rows is peaked."""
    Cc, nH, depths, shape, ups, s, resi, seed = SR.FIXTURES[name]
    sd, x, y64, ys = SR.case(name)
    err = float((ys - y64).abs().max())
    share = SR.codes_within_one(ys, y64)
    peaked = SR.peaked_share(sd, x, s, ups)
    print(f"swinir {name} (seed {seed}): storage model max|err| {err:.2e}, codes within +-1 {share:.5f}, range [{float(y64.min()):.3f}, {float(y64.max()):.3f}]; "
          f"softmax rows with max p > 0.5: {peaked:.3f}")
    assert tuple(y64.shape) == (shape[0], 3, shape[2] * s, shape[3] * s) and torch.isfinite(y64).all()
    assert share == 1.0, (name, share)
    assert err >= 2.0 ** -13, (name, err)                   # fp16 storage costs something: the model is not float64 by accident
    assert float(y64.min()) < 0.0 and float(y64.max()) > 0.8
    assert float(y64.min()) > -0.6 and float(y64.max()) < 1.6
    assert peaked > 0.3, (name, peaked)


def test_planted_faults_move_the_result():
    """Each mistake a window-attention engine can make -- no shift, no mask, no bias, the bias transposed, the roll back with the wrong sign, LayerNorm counting the pad
    channels -- moves forward64 by at least 10 x the storage model's error on at least one fixture (on most of them by 100 x): the network tests would see it."""
    worst = {f: 0.0 for f in FAULTS}
    for name in ("C60 [2,2] direct x2 16x24", "C180 [2] pixelshuffle x3 9x17", "C64 [2] nearest+conv x2 8x8"):
        Cc, nH, depths, shape, ups, s, resi, seed = SR.FIXTURES[name]
        sd, x, y64, ys = SR.case(name)
        es = float((ys - y64).abs().max())
        for f in FAULTS:
            r = float((SR.forward64(sd, x, s, ups, fault=f) - y64).abs().max()) / es
            print(f"swinir fault {f} on {name}: {r:.1f} x the storage model's error")
            worst[f] = max(worst[f], r)
    assert all(r >= 10.0 for r in worst.values()), worst
