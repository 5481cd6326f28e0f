"""SAFMN without a GPU: what run.infer_from_state_dict reads off a checkpoint, its refusals, strict loading, and the three entry points' declarations."""
import os
import re

import pytest
import torch

import _safmn_ref as SM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("wrap", [None, "params", "params_ema"])
def test_sniffing_reads_the_shapes(wrap):
    from innfer_amd.run import infer_from_state_dict
    sd = SM.fill(1, 48, 3, 1.5, 3, 0)
    info = infer_from_state_dict(sd if wrap is None else {wrap: sd})
    assert (info["arch"], info["scale"], info["in_nc"], info["nf"], info["nb"]) == ("safmn", 3, 1, 48, 3)
    p = info["net_params"]
    assert (p["dim"], p["n_blocks"], p["upscaling_factor"], p["in_chans"], int(p["dim"] * p["ffn_scale"] + 1e-6)) == (48, 3, 3, 1, 72)


def test_incomplete_block_0_is_not_sniffed():
    from innfer_amd.run import infer_from_state_dict
    sd = SM.fill(3, 36, 1, 2.0, 4, 0)
    del sd["feats.0.safm.aggr.bias"]
    with pytest.raises(Exception, match="Could not infer model parameters."):
        infer_from_state_dict(sd)


def _five_levels(sd):
    sd["feats.0.safm.mfr.4.weight"], sd["feats.0.safm.mfr.4.bias"] = sd["feats.0.safm.mfr.3.weight"], sd["feats.0.safm.mfr.3.bias"]


def _dim_38(sd):
    sd["to_feat.weight"] = torch.zeros(38, 3, 3, 3)


def _non_square(sd):
    sd["to_img.0.weight"] = torch.zeros(24, 36, 3, 3)


@pytest.mark.parametrize("edit,match", [(_five_levels, "5 feature-modulation levels"), (_dim_38, "dim 38"), (_non_square, "times a square")])
def test_refusals(edit, match):
    from innfer_amd.run import infer_from_state_dict
    sd = SM.fill(3, 36, 1, 2.0, 4, 0)
    edit(sd)
    with pytest.raises(NotImplementedError, match=match):
        infer_from_state_dict(sd)


def test_float32_tensor_and_strict_loading():
    from innfer_amd.architectures import get_network
    from innfer_amd.run import infer_from_state_dict
    net = get_network(infer_from_state_dict(SM.fill(3, 36, 2, 2.0, 4, 0))["net_params"])
    assert net._has_fp32 is False
    with pytest.raises(NotImplementedError, match="fp16 mode"):
        net(torch.zeros(1, 3, 16, 16))
    with pytest.raises(RuntimeError, match="size mismatch|Missing key"):
        net.load_state_dict(SM.fill(3, 128, 16, 2.0, 4, 0), strict=True)


def test_symbols_and_makefile():
    from innfer_amd.lib import SIGNATURES
    header = open(os.path.join(ROOT, "include", "innfer_amd.h")).read()
    for name in ("innfer_safmn_create", "innfer_net_set_safm", "innfer_safm"):
        assert re.search(r"\bint %s\(" % name, header) and name in SIGNATURES, name
    assert "innfer_amd/csrc/safm.hip" in open(os.path.join(ROOT, "Makefile")).read()
