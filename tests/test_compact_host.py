"""BasicSR SRVGGNetCompact: the host logic (no GPU) -- checkpoint sniffing, the key table, the refusals, and the test data's own figures."""
import numpy as np
import pytest
import torch

import _compact_ref as CR
from innfer_amd import synth
from innfer_amd.run import infer_from_state_dict


def _np_sd(shapes, seed):
    return {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in synth.fill_state_dict(shapes, seed).items()}


@pytest.mark.parametrize("num_conv,scale,nf,in_nc", [(16, 4, 64, 3), (32, 4, 64, 3), (2, 2, 32, 3), (0, 1, 64, 1), (8, 3, 24, 3), (1, 2, 48, 4)])
def test_compact_checkpoints_are_inferred(num_conv, scale, nf, in_nc):
    """(arch, scale, nf, num_conv, in_nc) from the keys alone, bare and under params_ema; the config builds BasicSR's constructor arguments."""
    sd = CR.fill(in_nc, nf, num_conv, scale, seed=1)
    for wrapped in (sd, {"params_ema": sd}, {"params": sd}):
        info = infer_from_state_dict(wrapped)
        assert (info["arch"], info["scale"], info["nf"], info["nb"], info["in_nc"], info["out_nc"]) == ("compact", scale, nf, num_conv, in_nc, in_nc)
        assert info["net_params"] == dict(type="compact_net", num_in_ch=in_nc, num_out_ch=in_nc, num_feat=nf, num_conv=num_conv, upscale=scale, act_type="prelu")
        assert set(info["state_dict"]) == set(sd)


def test_other_families_still_infer_as_before():
    """A BasicSR RRDBNet dict (its `body.<b>.rdb1..` keys share the prefix) stays 'realesrgan', an old-arch dict 'esrgan'."""
    from innfer_amd.architectures.keys import realesrgan_shapes
    assert infer_from_state_dict({"params_ema": _np_sd(realesrgan_shapes(num_block=2), 3)})["arch"] == "realesrgan"
    assert infer_from_state_dict(_np_sd(synth.rrdbnet_shapes(nb=1), 4))["arch"] == "esrgan"
    with pytest.raises(Exception, match="Could not infer"):
        infer_from_state_dict({"something.weight": torch.zeros(3)})


def test_refusals():
    sd = CR.fill(3, 64, 2, 4, seed=2)
    bad = dict(sd)                                         # 40 channels out of the last conv: not 3 times a square
    bad["body.6.weight"], bad["body.6.bias"] = torch.zeros(40, 64, 3, 3), torch.zeros(40)
    with pytest.raises(NotImplementedError, match="square"):
        infer_from_state_dict(bad)
    bad = dict(sd)                                         # 27 = 3 * 9 is fine, 4 * 3 = 12 out of a 3-channel net is scale 2; 3 in, 4 * 4 out: in_nc != out_nc
    bad["body.6.weight"], bad["body.6.bias"] = torch.zeros(16, 64, 3, 3), torch.zeros(16)
    with pytest.raises(NotImplementedError, match="num_out_ch"):
        infer_from_state_dict(bad)
    relu = {k: v for k, v in sd.items() if v.dim() != 1 or k.endswith(".bias")}          # no slopes: ReLU or LeakyReLU, undecidable
    with pytest.raises(NotImplementedError, match="ReLU"):
        infer_from_state_dict(relu)
    half = dict(sd); del half["body.3.weight"]             # one activation without its slopes
    with pytest.raises(NotImplementedError, match="PReLU"):
        infer_from_state_dict(half)
    from innfer_amd.architectures.SRVGG_arch import SRVGGNetCompact
    for kw in (dict(num_in_ch=3, num_out_ch=1), dict(num_feat=96), dict(upscale=8), dict(act_type="gelu"), dict(num_in_ch=5, num_out_ch=5)):
        with pytest.raises(NotImplementedError):
            SRVGGNetCompact(**kw)


@pytest.mark.parametrize("act", ["prelu", "relu", "leakyrelu"])
def test_key_table_equals_the_definition(act):
    from innfer_amd.architectures.SRVGG_arch import SRVGGNetCompact
    for nc, s, nf, cin in ((16, 4, 64, 3), (0, 1, 32, 1), (3, 3, 24, 4)):
        want = CR.shapes(cin, nf, nc, s, act)
        assert synth.compact_shapes(cin, cin, nf, nc, s, act) == want
        net = SRVGGNetCompact(cin, cin, nf, nc, s, act)
        assert {k: tuple(v.shape) for k, v in net.state_dict().items()} == {k: tuple(v) for k, v in want.items()}
        net.load_state_dict(CR.fill(cin, nf, nc, s, seed=5, act_type=act), strict=True)


def test_storage_model_is_what_the_gpu_tests_take_it_for():
    """Guards the test data: the fp16 storage model alone against float64 at nf 64, (num_conv, scale) = (2, 4), (16, 3), (32, 1), input synth.uniform((1, 3, 40, 56), 7).
    Outputs reach about 1.14, where fp16 is spaced 2^-10: the final rounding alone costs up to 2^-11 = 4.9e-4 and everything upstream at most as much again, so
    the model must lie in [2^-12, 2^-10] -- a smaller figure would mean nothing is rounded, a larger one that the filler lets the roundings grow with depth (the GPU
    tests hold the engine to twice this figure).  Measured: 7.9e-4, 8.5e-4, 8.4e-4; every uint8 code within +-1 of float64's (100 %); outputs in [-0.13, 1.15]."""
    x = torch.from_numpy(synth.uniform((1, 3, 40, 56), 7))
    for nc, s in ((2, 4), (16, 3), (32, 1)):
        sd = CR.fill(3, 64, nc, s, seed=nc)
        y64, ys = CR.forward64(sd, x, nc, s), CR.forward_storage(sd, x, nc, s)
        err = float((ys - y64).abs().max())
        print(f"compact storage model num_conv {nc} scale {s}: max|err| {err:.2e}, range [{float(y64.min()):.3f}, {float(y64.max()):.3f}]")
        assert 2.0 ** -12 <= err <= 2.0 ** -10, (nc, s, err)
        assert CR.codes_within_one(ys, y64) == 1.0
        assert -0.2 < float(y64.min()) and float(y64.max()) < 1.2
    # zero-padding the features is exact
    sd = CR.fill(3, 24, 2, 2, seed=9)
    assert torch.equal(CR.forward64(sd, x, 2, 2), CR.forward64(CR.pad_features(sd, 2, 32), x, 2, 2))
