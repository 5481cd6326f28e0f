"""The five generator engines keep their device memory in one owner each (csrc/engine_host.h DeviceBufs): a re-upload and a precision switch give the
same bits as the first forward, and a create / forward / destroy cycle gives every block back."""
import gc

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _unet():
    from innfer_amd.architectures.UNet_arch import UnetGenerator
    return UnetGenerator(3, 3, 5, ngf=64), (1, 3, 32, 32)


def _resnet():
    from innfer_amd.architectures.ResNet_arch import ResnetGenerator
    return ResnetGenerator(3, 3, ngf=64, norm_type="instance", n_blocks=9), (1, 3, 16, 16)


def _ppon():
    from innfer_amd.architectures.PPON_arch import PPON
    return PPON(), (1, 3, 16, 16)


def _pan():
    from innfer_amd.architectures.PAN_arch import PAN
    return PAN(nb=1), (1, 3, 16, 16)


def _wbc():
    from innfer_amd.architectures.WBCNet_arch import UnetGeneratorWBC
    return UnetGeneratorWBC(), (1, 3, 16, 16)


# (builder, assert the memory condition): the condition needs weights of at least 8 MiB so that allocator granularity cannot hide a leaked copy;
# PAN's and WBC's are far smaller, they assert the bit identity only
ENGINES = {"unet": (_unet, True), "resnet": (_resnet, True), "ppon": (_ppon, True), "pan": (_pan, False), "wbc": (_wbc, False)}


def _last(y):
    return y[-1] if isinstance(y, (list, tuple)) else y


@pytest.mark.parametrize("eng", sorted(ENGINES))
def test_reupload_precision_switch_and_destroy(dev, eng):
    """Per cycle: build, load seeded weights, y0 = forward(x); bump one parameter's version with identical values (the module re-sends every parameter, the
    engine frees and rebuilds every device block) -> the same bits; fp16 -> fp32 -> fp16 input (the fp32 panels are built beside the fp16 blocks) -> the
    third result is y0 again.  Five cycles; the device's free bytes after cycle 5 may lie below those after cycle 2 by less than ONE instance's packed
    weights, taken as 2 bytes x the parameter count -- a leak of one upload's blocks per cycle would be three times that, and every cycle uploads twice."""
    from innfer_amd import synth
    build, check_mem = ENGINES[eng]
    x = None
    free, n_params = {}, 0
    for cycle in range(1, 6):
        net, shape = build()
        sd = {k: torch.from_numpy(np.asarray(v)) for k, v in synth.fill_state_dict({k: tuple(t.shape) for k, t in net.state_dict().items()}, 3).items()}
        net.load_state_dict(sd, strict=True)
        net = net.to(dev).eval()
        n_params = sum(p.numel() for p in net.parameters())
        if x is None:
            x = torch.from_numpy(synth.uniform(shape, 11, -1.0, 1.0)).to(dev)
        y0 = _last(net(x.half())).clone()
        assert y0.dtype == torch.float16 and torch.isfinite(y0).all()
        with torch.no_grad():
            next(net.parameters()).add_(0)                     # same values, new version: _upload re-sends everything
        assert torch.equal(_last(net(x.half())), y0), (eng, cycle, "re-upload")
        y32 = _last(net(x))
        assert y32.dtype == torch.float32 and torch.isfinite(y32).all()
        assert torch.equal(_last(net(x.half())), y0), (eng, cycle, "fp16 after fp32")
        del net, y0, y32, sd
        gc.collect()
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        free[cycle] = torch.cuda.mem_get_info()[0]
    drop, weights = free[2] - free[5], 2 * n_params
    print(f"{eng}: free bytes after cycle 2 {free[2]}, after cycle 5 {free[5]}: drop {drop}; one instance's packed weights {weights}")
    if check_mem:
        assert weights >= 8 << 20, (eng, weights)
        assert drop < weights, (eng, drop, weights)
