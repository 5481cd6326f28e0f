"""SPAN: the host logic (no GPU) -- the Conv3XC collapse, the key table, strict loading, checkpoint sniffing, the refusals, the new symbols, and the test data's own figures."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _span_ref as SR
from innfer_amd import synth
from innfer_amd.run import infer_from_state_dict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _unit(ci, co, seed, gain=2):
    """A lone Conv3XC(ci, co) under the prefix `u`, every part O(1)."""
    shp = {"u.sk.weight": (co, ci, 1, 1), "u.sk.bias": (co,), "u.conv.0.weight": (ci * gain, ci, 1, 1), "u.conv.0.bias": (ci * gain,),
           "u.conv.1.weight": (co * gain, ci * gain, 3, 3), "u.conv.1.bias": (co * gain,), "u.conv.2.weight": (co, co * gain, 1, 1), "u.conv.2.bias": (co,)}
    return {k: torch.from_numpy(synth.uniform(s, synth.key_seed(k, seed), -0.5, 0.5)) for k, s in shp.items()}


@pytest.mark.parametrize("ci,co,shape", [(3, 48, (2, 7, 9)), (48, 48, (1, 5, 11)), (5, 7, (3, 1, 1)), (5, 7, (1, 2, 13))])
def test_collapse_equals_the_training_branch(ci, co, shape):
    """One 3x3 zero-pad-1 conv with the collapsed (W, b) == conv.2(conv.1(conv.0(F.pad(x, 1)))) + sk(x) in float64 on ragged sizes, border included (the padded
    ring carries conv.0.b, which is what b assumes); the shell's numpy collapse == the reference's to the fp32 rounding."""
    from innfer_amd.architectures.SPAN_arch import collapse_conv3xc
    sd = _unit(ci, co, ci + co)
    x = torch.from_numpy(synth.uniform((shape[0], ci) + shape[1:], 11)).double() * 4 - 2
    W, b = SR.collapse(sd, "u")
    got, want = F.conv2d(x, W, b, padding=1), SR.training_branch(sd, "u", x)
    err = float((got - want).abs().max())
    mag = float(want.abs().max())
    print(f"collapse {ci}->{co} {shape}: max |one conv - training branch| {err:.1e} at magnitude {mag:.1f}")
    # both sides are float64 sums of at most 9 * 96 * 96 * 48 products in different orders: a few thousand roundings of 1.1e-16 relative each, far below 1e-12
    assert err <= 1e-12 * max(1.0, mag)
    w, bb = collapse_conv3xc(sd, "u")
    assert w.dtype == np.float32 and np.abs(w - W.numpy()).max() <= 2.0 ** -23 * np.abs(W.numpy()).max() and np.abs(bb - b.numpy()).max() <= 2.0 ** -22 * max(1.0, np.abs(b.numpy()).max())


def test_key_table_and_strict_loading():
    """span_shapes == the definition written out in _span_ref; full, deploy and no_norm state dicts load strictly (no_norm is a buffer, registered exactly then)."""
    from innfer_amd.architectures.SPAN_arch import SPAN
    for cin, f, s in ((3, 48, 4), (3, 52, 2), (1, 32, 1), (4, 24, 3)):
        for norm in (True, False):
            for deploy in (False, True):
                want = SR.shapes(cin, f, s, norm, deploy)
                assert synth.span_shapes(cin, cin, f, s, norm, deploy) == want
                if norm and cin != 3:
                    continue
                net = SPAN(cin, cin, f, s, norm=norm, deploy=deploy)
                assert {k: tuple(v.shape) for k, v in net.state_dict().items()} == {k: tuple(v) for k, v in want.items()}
                assert ("no_norm" in dict(net.named_buffers())) == (not norm) and "no_norm" not in dict(net.named_parameters())
                net.load_state_dict(SR.fill(cin, f, s, 5, norm, deploy), strict=True)
    with pytest.raises(RuntimeError):          # a deploy shell refuses a full checkpoint, a norm shell a no_norm one
        SPAN(deploy=True).load_state_dict(SR.fill(3, 48, 4, 5), strict=True)
    with pytest.raises(RuntimeError):
        SPAN().load_state_dict(SR.fill(3, 48, 4, 5, norm=False), strict=True)


@pytest.mark.parametrize("f,scale", [(48, 4), (52, 2), (32, 1), (48, 3), (52, 4), (32, 2)])
def test_span_checkpoints_are_inferred(f, scale):
    """(arch, scale, f, in_nc, norm, deploy) from the keys alone, bare and under params_ema / params."""
    for norm, deploy in ((True, False), (False, False), (True, True)):
        sd = SR.fill(3, f, scale, 1, norm, deploy)
        for wrapped in (sd, {"params_ema": sd}, {"params": sd}):
            info = infer_from_state_dict(wrapped)
            assert (info["arch"], info["scale"], info["nf"], info["in_nc"], info["out_nc"]) == ("span", scale, f, 3, 3)
            assert info["net_params"] == dict(type="span_net", num_in_ch=3, num_out_ch=3, feature_channels=f, upscale=scale, norm=norm, deploy=deploy)
            assert set(info["state_dict"]) == set(sd)


def test_other_families_still_infer_as_before():
    from innfer_amd.architectures.keys import realesrgan_shapes
    import _compact_ref as CR
    np_sd = lambda shapes, seed: {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in synth.fill_state_dict(shapes, seed).items()}
    assert infer_from_state_dict({"params_ema": np_sd(realesrgan_shapes(num_block=2), 3)})["arch"] == "realesrgan"
    assert infer_from_state_dict(np_sd(synth.rrdbnet_shapes(nb=1), 4))["arch"] == "esrgan"
    assert infer_from_state_dict(CR.fill(3, 64, 2, 4, seed=2))["arch"] == "compact"
    with pytest.raises(Exception, match="Could not infer"):          # conv_1.sk without conv_cat is not a SPAN
        infer_from_state_dict({"conv_1.sk.weight": torch.zeros(48, 3, 1, 1)})


def test_refusals():
    from innfer_amd.architectures import get_network
    from innfer_amd.architectures.SPAN_arch import SPAN
    sd = SR.fill(3, 48, 4, 2)
    bad = dict(sd)                                         # 40 channels out of upsampler.0: not 3 times a square
    bad["upsampler.0.weight"], bad["upsampler.0.bias"] = torch.zeros(40, 48, 3, 3), torch.zeros(40)
    with pytest.raises(NotImplementedError, match="square"):
        infer_from_state_dict(bad)
    for what, kw in (("num_in_ch", dict(num_in_ch=1, num_out_ch=1)), ("feature_channels", dict(feature_channels=96)), ("upscale", dict(upscale=8)),
                     ("num_out_ch", dict(num_in_ch=3, num_out_ch=1)), ("bias", dict(bias=False))):
        with pytest.raises(NotImplementedError, match=what):
            SPAN(**kw)
    SPAN(num_in_ch=1, num_out_ch=1, norm=False)             # one channel is fine without the three-entry mean
    # the same refusals through the sniffing path: f 96, upscale 8, in_nc 1 with norm
    for kw in (dict(f=96, upscale=2), dict(f=48, upscale=8), dict(num_in_ch=1, f=48, upscale=2)):
        info = infer_from_state_dict({k: torch.zeros(v) for k, v in SR.shapes(**kw).items()})
        with pytest.raises(NotImplementedError, match="not built on the HIP path"):
            get_network(info["net_params"])
    assert SPAN._has_fp32 is False                          # -no_fp16 is refused by run.py's check of this flag


def test_new_symbols_are_declared_and_bound():
    """innfer_span_create / innfer_first_conv_map: declared in the header, bound in lib.py's SIGNATURES; the ABI revision (now 124)."""
    hdr = open(os.path.join(ROOT, "include", "innfer_amd.h")).read()
    lib_py = open(os.path.join(ROOT, "innfer_amd", "lib.py")).read()
    for sym in ("innfer_span_create", "innfer_first_conv_map"):
        assert re.search(r"^int %s\(" % sym, hdr, re.M), sym
        assert '"%s"' % sym in lib_py, sym
    assert re.search(r"^#define INNFER_ABI_VERSION 124$", hdr, re.M)
    assert "span_forward" in open(os.path.join(ROOT, "innfer_amd", "csrc", "net.hip")).read()


def test_storage_model_is_what_the_gpu_tests_take_it_for():
    """Guards the test data of tests/test_gpu_span.py: on every fixture the float64 forward shows the unsaturated AND the saturated gate (shares of |out3| < 2 and
    > 4 both above 10 %), the result is an image, and the fp16 storage model alone meets the 99 % uint8 rule with a max error between 2^-12 (something is rounded) and
    2^-9 (the roundings do not grow through six blocks; outputs lie below 1, where fp16 is spaced 2^-11: the last rounding alone costs up to 2^-12)."""
    for f, s, shape, seed, norm in ((48, 4, (1, 3, 32, 32), 1, True), (48, 2, (1, 3, 31, 33), 2, True), (52, 3, (1, 3, 17, 9), 3, True), (32, 1, (1, 3, 8, 8), 4, True),
                                    (48, 2, (2, 3, 21, 26), 6, True), (48, 2, (1, 3, 20, 24), 5, False)):
        sd = SR.fill(3, f, s, seed, norm)
        x = torch.from_numpy(synth.uniform(shape, 7 + seed))
        lo, hi = SR.gate_shares(sd, x, s, norm)
        y64, ys = SR.forward64(sd, x, s, norm), SR.forward_storage(sd, x, s, norm)
        err = float((ys - y64).abs().max())
        print(f"span f {f} x{s} {shape} seed {seed} norm {norm}: |out3| < 2: {lo:.2f}, > 4: {hi:.2f}; storage model max|err| {err:.2e}, range [{float(y64.min()):.3f}, {float(y64.max()):.3f}]")
        assert lo > 0.10 and hi > 0.10, (f, s, lo, hi)
        assert 2.0 ** -12 <= err <= 2.0 ** -9, (f, s, err)
        assert SR.codes_within_one(ys, y64) >= 0.99
        assert 0.0 < float(y64.min()) and float(y64.max()) < 1.0
        if seed == 2:          # a deploy dict is the same network: float64 on its fp32-rounded collapsed convs
            yd = SR.forward64(SR.fill(3, f, s, seed, norm, True), x, s, norm)
            assert float((yd - y64).abs().max()) < 1e-5
    # zero-padded features are exact: SiLU(0) = 0 and the gate of (0, 0) is (0 + 0) * 0
    z = torch.zeros(3, dtype=torch.float64)
    assert float((z * torch.sigmoid(z)).abs().max()) == 0.0 and float(((z + z) * (torch.sigmoid(z) - 0.5)).abs().max()) == 0.0
