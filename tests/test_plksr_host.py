"""RealPLKSR: the host logic (no GPU) -- the key table, strict loading, checkpoint sniffing, the "S" variant, the refusals, the new symbols, and the test data's own figures."""
import os
import re

import pytest
import torch

import _plksr_ref as PR
from innfer_amd import synth
from innfer_amd.run import infer_from_state_dict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VARIANTS = [dict(in_ch=3, n_blocks=28, scale=4, k=17, use_ea=True), dict(in_ch=3, n_blocks=12, scale=4, k=13, use_ea=False), dict(in_ch=1, n_blocks=2, scale=2, k=17, use_ea=True),
            dict(in_ch=4, n_blocks=3, scale=3, k=5, use_ea=False), dict(in_ch=3, n_blocks=1, scale=1, k=3, use_ea=True)]


def _zeros(**kw):
    return {k: torch.zeros(v) for k, v in PR.shapes(**kw).items()}


def test_key_table_and_strict_loading():
    """realplksr_shapes == the definition written out in _plksr_ref; the shell's state dict has exactly those keys and loads a filled one strictly."""
    from innfer_amd.architectures.PLKSR_arch import RealPLKSR
    for v in VARIANTS:
        want = PR.shapes(v["in_ch"], 64, v["n_blocks"], v["scale"], v["k"], v["use_ea"])
        assert synth.realplksr_shapes(v["in_ch"], v["in_ch"], 64, v["n_blocks"], v["scale"], v["k"], 0.25, v["use_ea"]) == want
        net = RealPLKSR(v["in_ch"], v["in_ch"], 64, v["n_blocks"], v["scale"], v["k"], 0.25, v["use_ea"])
        assert {k: tuple(t.shape) for k, t in net.state_dict().items()} == {k: tuple(s) for k, s in want.items()}
        if v["n_blocks"] <= 3:
            net.load_state_dict(PR.fill(v["in_ch"], 64, v["n_blocks"], v["scale"], v["k"], v["use_ea"], 5), strict=True)
    with pytest.raises(RuntimeError):          # an EA shell refuses a checkpoint without attn.f.0, and the other way round
        RealPLKSR(n_blocks=2).load_state_dict(PR.fill(3, 64, 2, 4, 17, False, 5), strict=True)
    with pytest.raises(RuntimeError):
        RealPLKSR(n_blocks=2, use_ea=False).load_state_dict(PR.fill(3, 64, 2, 4, 17, True, 5), strict=True)


@pytest.mark.parametrize("v", VARIANTS, ids=lambda v: f"in{v['in_ch']}-n{v['n_blocks']}-x{v['scale']}-k{v['k']}-ea{int(v['use_ea'])}")
def test_realplksr_checkpoints_are_inferred(v):
    """Everything but norm_groups from the shapes alone, bare and under params_ema / params; the checkpoint then loads strictly into the network the config builds."""
    from innfer_amd.architectures import get_network
    sd = _zeros(in_ch=v["in_ch"], n_blocks=v["n_blocks"], scale=v["scale"], k=v["k"], use_ea=v["use_ea"])
    for wrapped in (sd, {"params_ema": sd}, {"params": sd}):
        info = infer_from_state_dict(wrapped)
        assert (info["arch"], info["scale"], info["nf"], info["nb"], info["in_nc"], info["out_nc"]) == ("realplksr", v["scale"], 64, v["n_blocks"], v["in_ch"], v["in_ch"])
        assert info["net_params"] == dict(type="realplksr", in_ch=v["in_ch"], out_ch=v["in_ch"], dim=64, n_blocks=v["n_blocks"], upscaling_factor=v["scale"],
                                          kernel_size=v["k"], split_ratio=0.25, use_ea=v["use_ea"], norm_groups=4)
        assert set(info["state_dict"]) == set(sd)
    net = get_network(info["net_params"])
    net.load_state_dict(info["state_dict"], strict=True)
    assert (net.kernel_size, net.use_ea, net.n_blocks, net.norm_groups) == (v["k"], v["use_ea"], v["n_blocks"], 4)


def test_the_s_variant_loads():
    """RealPLKSR "S": n_blocks 12, kernel_size 13, use_ea False."""
    from innfer_amd.architectures import get_network
    sd = PR.fill(3, 64, 12, 4, 13, False, 3)
    info = infer_from_state_dict({"params_ema": sd})
    assert (info["net_params"]["n_blocks"], info["net_params"]["kernel_size"], info["net_params"]["use_ea"]) == (12, 13, False)
    net = get_network(info["net_params"])
    net.load_state_dict(info["state_dict"], strict=True)
    assert not any(".attn." in k for k in net.state_dict())


def test_other_families_still_infer_as_before():
    import _compact_ref as CR
    import _span_ref as SR
    assert infer_from_state_dict(CR.fill(3, 64, 2, 4, seed=2))["arch"] == "compact"
    assert infer_from_state_dict(SR.fill(3, 48, 2, 1))["arch"] == "span"
    with pytest.raises(Exception, match="Could not infer"):          # feats.0 without a PLK block is not a RealPLKSR
        infer_from_state_dict({"feats.0.weight": torch.zeros(64, 3, 3, 3)})


def test_refusals():
    """Clear NotImplementedErrors, raised by the shell's constructor or the sniffing: nothing touches the GPU."""
    from innfer_amd.architectures import get_network
    from innfer_amd.architectures.PLKSR_arch import RealPLKSR
    for what, kw in (("dim", dict(dim=48, split_ratio=1 / 3)), ("split_ratio", dict(split_ratio=0.5)), ("kernel_size", dict(kernel_size=16)), ("kernel_size", dict(kernel_size=19)),
                     ("out_ch", dict(in_ch=3, out_ch=1)), ("in_ch", dict(in_ch=5, out_ch=5)), ("in_ch", dict(in_ch=0, out_ch=0)), ("upscaling_factor", dict(upscaling_factor=8)),
                     ("upscaling_factor", dict(upscaling_factor=0)), ("dysample", dict(dysample=True))):
        with pytest.raises(NotImplementedError, match=what):
            RealPLKSR(n_blocks=1, **kw)
    # the same through the sniffing path: dim 32 (p 8), p 32, k 16, k 19, in_ch 5, scale 5
    for kw in (dict(dim=32, p=8), dict(p=32), dict(k=16), dict(k=19), dict(in_ch=5), dict(scale=5)):
        info = infer_from_state_dict(_zeros(n_blocks=1, **kw))
        assert info["arch"] == "realplksr"
        with pytest.raises(NotImplementedError, match="not built on the HIP path"):
            get_network(info["net_params"])
    sd = _zeros(n_blocks=1)
    bad = dict(sd)                                         # 40 channels out of the last conv: not 3 times a square (out_ch != in_ch)
    bad["feats.3.weight"], bad["feats.3.bias"] = torch.zeros(40, 64, 3, 3), torch.zeros(40)
    with pytest.raises(NotImplementedError, match="square"):
        infer_from_state_dict(bad)
    dys = dict(sd)                                         # the DySample upsampler
    dys["to_img.init_pos"], dys["to_img.offset.weight"] = torch.zeros(1, 32, 1, 1), torch.zeros(32, 48, 1, 1)
    with pytest.raises(NotImplementedError, match="DySample"):
        infer_from_state_dict({"params_ema": dys})
    plain = {k: v for k, v in sd.items() if ".norm." not in k}          # the original PLKSR has no GroupNorm
    with pytest.raises(NotImplementedError, match="original PLKSR"):
        infer_from_state_dict(plain)
    assert RealPLKSR._has_fp32 is False                     # -no_fp16 is refused by run.py's check of this flag
    with pytest.raises(NotImplementedError, match="fp16 mode only"):
        RealPLKSR(n_blocks=1).forward(torch.zeros(1, 3, 8, 8))
    with pytest.raises(NotImplementedError, match="fp16 mode only"):
        RealPLKSR(n_blocks=1).tile_batch_bytes(1, 16, torch.float32)


def test_new_symbols_are_declared_and_bound():
    """The new entry points: declared in the header, bound in lib.py's SIGNATURES; the ABI revision (now 124); the sources are part of the build."""
    hdr = open(os.path.join(ROOT, "include", "innfer_amd.h")).read()
    lib_py = open(os.path.join(ROOT, "innfer_amd", "lib.py")).read()
    for sym in ("innfer_plksr_create", "innfer_net_set_group_norm", "innfer_plk_conv", "innfer_group_norm_skip"):
        assert re.search(r"^int %s\(" % sym, hdr, re.M), sym
        assert '"%s"' % sym in lib_py, sym
    assert re.search(r"^size_t innfer_group_norm_skip_work_bytes\(", hdr, re.M) and '"innfer_group_norm_skip_work_bytes"' in lib_py
    assert re.search(r"^#define INNFER_ABI_VERSION 124$", hdr, re.M)
    assert "plksr_forward" in open(os.path.join(ROOT, "innfer_amd", "csrc", "net.hip")).read()
    mk = open(os.path.join(ROOT, "Makefile")).read()
    assert "csrc/plk_conv.hip" in mk and "csrc/group_norm.hip" in mk


@pytest.mark.parametrize("name", list(PR.FIXTURES))
def test_storage_model_is_what_the_gpu_tests_take_it_for(name):
    """Guards the test data of tests/test_gpu_plksr.py: on every network fixture the fp16 storage model alone has >= 99.5 % of its uint8 codes within +-1 of float64
    (its max error is printed: the GPU tests allow the engine twice that), something IS rounded, the result is an image that reaches both clips where the fixture is
    large enough, and the Mish and gate arguments cover both regimes."""
    nb, s, shape, k, ea, seed = PR.FIXTURES[name]
    sd, x, y64, ys = PR.case(name)
    err = float((ys - y64).abs().max())
    share = PR.codes_within_one(ys, y64)
    sh = PR.argument_shares(sd, x, s)
    gate = "-" if sh["gate"] is None else f"|g| < 2: {sh['gate'][0]:.2f}, > 4: {sh['gate'][1]:.3f}"
    print(f"plksr {name} (k {k}, EA {ea}, seed {seed}): storage model max|err| {err:.2e}, codes within +-1 {share:.5f}, range [{float(y64.min()):.3f}, {float(y64.max()):.3f}]; "
          f"Mish |f| < 1: {sh['mish'][0]:.2f}, f < -3: {sh['mish'][1]:.3f}; gate {gate}")
    assert tuple(y64.shape) == (shape[0], 3, shape[2] * s, shape[3] * s) and torch.isfinite(y64).all()
    assert share >= 0.995, (name, share)
    assert err >= 2.0 ** -13, (name, err)                   # fp16 storage costs something: the model is not float64 by accident
    assert float(y64.min()) < 0.05 and float(y64.max()) > 0.95
    assert 0.2 < sh["mish"][0] < 0.9
    if sh["gate"] is not None:
        assert sh["gate"][0] > 0.1                           # the unsaturated gate is exercised (the saturated one needs no share: sigmoid there is 0 or 1)
