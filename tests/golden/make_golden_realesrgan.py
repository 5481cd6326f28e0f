#!/usr/bin/env python3
"""Golden vectors G28: the BasicSR RRDBNet forms of scale 2 and 1 (Real-ESRGAN x2plus and kin) produced by the REFERENCE's own RRDBNet.

BasicSR's RRDBNet(scale = 2 | 1) is pixel_unshuffle(x, r = 2 | 4) in front of the ordinary 4x graph, whose first conv then takes 3 r^2 channels.  The
reference has that graph (RRDBNet(in_nc=3 r^2, upscale=4)); torch supplies the unshuffle.  Sizes that are not a multiple of r are reflect-padded bottom /
right and the result cropped, as BasicSR's inference tools do.

Runs only where the reference is mounted (INNFER_REFERENCE, default /root/reference), like make_golden.py:

    python tests/golden/make_golden_realesrgan.py      # writes tests/golden/g28_realesrgan.npz

The fixture holds OUTPUTS only; weights (synth.fill_state_dict(rrdbnet_shapes(in_nc=3 r^2, nb=2), seed r)) and inputs (synth.uniform, seeds below) are
regenerated from their seeds by the tests.
"""
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("INNFER_REFERENCE", "/root/reference")
sys.path.insert(0, REPO)
sys.path.insert(0, REF)
sys.modules.setdefault("cv2", types.ModuleType("cv2"))

from innfer_amd import synth  # noqa: E402
from utils.defaults import get_network_G_config  # noqa: E402
from architectures import get_network  # noqa: E402

NB = 2
CASES = {"32x32": ((1, 3, 32, 32), 280), "31x33": ((1, 3, 31, 33), 290)}      # name -> (input shape, seed base; the seed is base + r)


def main():
    torch.set_num_threads(8)
    out = {}
    for r in (2, 4):
        sd = synth.fill_state_dict(synth.rrdbnet_shapes(in_nc=3 * r * r, nb=NB, scale=4), r)
        net = get_network(get_network_G_config(dict(type="esrgan", in_nc=3 * r * r, nb=NB), 4))
        net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
        net.eval()
        s = 4 // r
        for name, (shape, seed) in CASES.items():
            x = torch.from_numpy(synth.uniform(shape, seed + r))
            H, W = shape[2:]
            ph, pw = -H % r, -W % r
            xp = F.pad(x, (0, pw, 0, ph), mode="reflect") if ph or pw else x
            with torch.no_grad():
                y = net(F.pixel_unshuffle(xp, r))[:, :, :s * H, :s * W]
            assert tuple(y.shape) == (1, 3, s * H, s * W)
            out[f"r{r}_{name}"] = y.contiguous().numpy()
    path = os.path.join(HERE, "g28_realesrgan.npz")
    np.savez_compressed(path, **out)
    print(f"g28_realesrgan.npz  {os.path.getsize(path) / 1024:.0f} KiB")


if __name__ == "__main__":
    main()
