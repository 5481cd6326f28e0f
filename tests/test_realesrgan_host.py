"""BasicSR RRDBNet / Real-ESRGAN checkpoints on the host: key sniffing, hyper-parameter inference, the key map, the module shell -- and the CPU oracle
composition (pixel_unshuffle in front of the old-arch 4x graph) pinned to the reference's own output (G28).  No GPU."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import oracle
from innfer_amd import synth
from innfer_amd.architectures import keys

CASES = [(23, 1), (6, 1), (2, 2), (2, 4)]          # (num_block, unshuffle factor r); the scale is 4 // r


def _basicsr_sd(nb, r, nf=64, gc=32, out_nc=3):
    shapes = keys.realesrgan_shapes(3, out_nc, 4 // r, nf, nb, gc)
    return {k: torch.zeros(v) for k, v in shapes.items()}


def oracle_realesrgan(sd_old, x, r, nb):
    """BasicSR RRDBNet(scale = 4 // r) on the CPU oracle: reflect pad bottom / right to a multiple of r, unshuffle, the 4x graph, crop."""
    H, W = x.shape[-2:]
    ph, pw = -H % r, -W % r
    xp = F.pad(x, (0, pw, 0, ph), mode="reflect") if ph or pw else x
    s = 4 // r
    return oracle.rrdbnet_forward(sd_old, F.pixel_unshuffle(xp, r) if r > 1 else xp, nb=nb, scale=4)[:, :, :s * H, :s * W]


@pytest.mark.parametrize("nb,r", CASES)
@pytest.mark.parametrize("wrap", [None, "params_ema", "params"])
def test_infer_basicsr_keys(nb, r, wrap):
    from innfer_amd.run import infer_from_state_dict
    sd = _basicsr_sd(nb, r)
    ck = sd if wrap is None else {wrap: sd}
    if wrap == "params":
        ck = {"params": sd, "iter": 5}                     # other entries beside the weights are ignored
    info = infer_from_state_dict(ck)
    assert (info["arch"], info["scale"], info["nb"], info["nf"], info["in_nc"], info["out_nc"]) == ("realesrgan", 4 // r, nb, 64, 3, 3)
    assert info["net_params"] == dict(type="realesrgan_net", num_in_ch=3, num_out_ch=3, scale=4 // r, num_feat=64, num_block=nb, num_grow_ch=32)
    assert set(info["state_dict"]) == set(sd)              # BasicSR's keys are kept: the shell registers its parameters under them


def test_infer_prefers_params_ema_and_other_widths():
    from innfer_amd.run import infer_from_state_dict
    ema, raw = _basicsr_sd(6, 1), _basicsr_sd(2, 1)
    assert infer_from_state_dict({"params": raw, "params_ema": ema})["nb"] == 6
    info = infer_from_state_dict(_basicsr_sd(3, 2, nf=32, out_nc=1))
    assert (info["nf"], info["out_nc"], info["scale"], info["nb"]) == (32, 1, 2, 3)


@pytest.mark.parametrize("nb,r", CASES)
def test_key_map_is_a_bijection_onto_old_arch(nb, r):
    m = keys.realesrgan_key_map(nb)
    old = keys.rrdbnet_shapes(in_nc=3 * r * r, nb=nb, scale=4)
    new = keys.realesrgan_shapes(3, 3, 4 // r, 64, nb, 32)
    mapped = {o + "." + p: new[n + "." + p] for n, o in m.items() for p in ("weight", "bias")}
    assert len(set(m.values())) == len(m) and mapped == old                 # one to one, onto, shapes agree
    for n, o in m.items():
        assert keys.realesrgan_key_of(o, nb) == n
    from innfer_amd.utils.utils import realesrgan2normal
    conv = realesrgan2normal({k: k for k in new})
    assert set(conv) == set(old) and all(m[v.rsplit(".", 1)[0]] == k.rsplit(".", 1)[0] for k, v in conv.items())


@pytest.mark.parametrize("nb,r", CASES)
def test_shell_has_exactly_the_basicsr_keys(nb, r):
    from innfer_amd.architectures import get_network
    from innfer_amd.run import infer_from_state_dict
    sd = {k: torch.from_numpy(v) for k, v in synth.fill_state_dict(keys.realesrgan_shapes(3, 3, 4 // r, 64, nb, 32), 1).items()}
    info = infer_from_state_dict({"params_ema": sd})
    net = get_network(info["net_params"])
    assert list(net.state_dict()) == list(sd)
    net.load_state_dict(info["state_dict"], strict=True)
    assert (net.upscale, net.unshuffle, net.in_nc, net.nb) == (4 // r, r, 3, nb)
    assert torch.equal(net.state_dict()["conv_first.weight"], sd["conv_first.weight"]) and tuple(sd["conv_first.weight"].shape) == (64, 3 * r * r, 3, 3)
    for (H, W) in [(200, 200), (31, 33), (7, 5)]:          # true scale; padded rows / columns of ragged sizes are cropped
        full, want = net._io_sizes(H, W, 4)
        assert want == (H * 4 // r, W * 4 // r) and full == (-(-H // r) * 4, -(-W // r) * 4) and full >= want


def test_grow_channels_other_than_32_are_refused():
    from innfer_amd.architectures.RRDBNet_arch import RealESRGANNet
    from innfer_amd.run import infer_from_state_dict
    with pytest.raises(NotImplementedError, match="num_grow_ch=16"):
        infer_from_state_dict({"params_ema": _basicsr_sd(2, 1, gc=16)})
    with pytest.raises(NotImplementedError, match="num_grow_ch=16"):
        RealESRGANNet(num_grow_ch=16)
    with pytest.raises(NotImplementedError, match="scale=3"):
        RealESRGANNet(scale=3)


def test_other_key_layouts_infer_as_before():
    """Old-arch, new-arch (RRDB_trunk) and SWA checkpoints do not meet the new probe or the unwrapping."""
    from innfer_amd.run import infer_from_state_dict
    old = {k: torch.zeros(v) for k, v in keys.rrdbnet_shapes(nb=5, scale=2).items()}
    info = infer_from_state_dict(dict(old))
    assert (info["arch"], info["scale"], info["nb"], info["nf"], info["in_nc"], info["out_nc"], info["plus"]) == ("esrgan", 2, 5, 64, 3, 3, False)
    assert info["net_params"]["type"] == "rrdb_net" and list(info["state_dict"]) == list(old)
    new = {k: torch.zeros(v) for k, v in keys.mrrdbnet_shapes(nb=23).items()}
    info = infer_from_state_dict(dict(new))
    assert (info["arch"], info["scale"], info["nb"], info["nf"]) == ("esrgan", 4, 23, 64)
    assert set(info["state_dict"]) == set(keys.rrdbnet_shapes(nb=23, scale=4))
    swa = {"n_averaged": torch.tensor(3)}
    swa.update({"module.module." + k: v for k, v in old.items()})
    info = infer_from_state_dict(swa)
    assert (info["arch"], info["scale"], info["nb"]) == ("esrgan", 2, 5) and list(info["state_dict"]) == list(old)
    srgan = {k: torch.zeros(v) for k, v in keys.srresnet_shapes(nb=4, scale=4).items()}
    assert infer_from_state_dict(srgan)["arch"] == "srgan"


def test_oracle_composition_vs_golden_g28(golden):
    """pixel_unshuffle + the oracle's old-arch 4x forward (the oracle of the GPU tests) against the reference's RRDBNet(in_nc = 3 r^2) on the same weights:
    the bound of test_oracle_golden.test_g3_rrdbnet23."""
    g = golden("g28_realesrgan")
    for r in (2, 4):
        sd = {k: torch.from_numpy(v) for k, v in synth.fill_state_dict(synth.rrdbnet_shapes(in_nc=3 * r * r, nb=2, scale=4), r).items()}
        for name, shape, seed in (("32x32", (1, 3, 32, 32), 280), ("31x33", (1, 3, 31, 33), 290)):
            x = torch.from_numpy(synth.uniform(shape, seed + r))
            with torch.no_grad():
                y = oracle_realesrgan(sd, x, r, 2)
            want = g[f"r{r}_{name}"]
            assert y.shape == want.shape == (1, 3, shape[2] * 4 // r, shape[3] * 4 // r)
            np.testing.assert_allclose(y.numpy(), want, atol=2e-6, rtol=0, err_msg=f"r{r}_{name}")
