"""SAFMN on the MI355X: the feature modulation launch next to the same operator composed from torch-ROCm ops, and ms per forward (measurement only; needs the GPU).

(a) innfer_safm at dim 36 and 128 on 16 tiles of 200 x 200 (the library's launch timer around the launch function the network calls) and, on the same values as NCHW
    fp16 tensors, t + gelu(conv1x1(cat(s_i))) * u composed from adaptive_max_pool2d / conv2d / interpolate / gelu (HIP events around the composed call), alternating
    launch by launch in ONE process, medians over the rounds.  The byte floor is u and t read once and the result written once (6 dim bytes a pixel) at HBM_PEAK.
(b) Forwards of SAFMN x4 (dim 36, 8 blocks) and SAFMN-L x4 (dim 128, 16 blocks), random weights (tests/_safmn_ref.fill), fp16 I/O, at 16 x 200 x 200: the host clock
    around the module's forward ending in a device synchronise.
The shader clock is read after each part.

    python scripts/time_safmn.py [--rounds 7] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))

import _conv_ref as R               # noqa: E402
import _safmn_ref as SM             # noqa: E402
import innfer_amd.lib as L          # noqa: E402
from innfer_amd import synth        # noqa: E402
from time_compact import shader_clock_mhz          # noqa: E402

N, H, W = 16, 200, 200
HBM_PEAK = 8.0e12                   # bytes / s, the MI355X's published HBM3E peak
MODELS = {"SAFMN_x4": (36, 8), "SAFMN-L_x4": (128, 16)}


def composed(u, t, mw, mb, aw, ab):
    chunk, s = u.shape[1] // 4, []
    for i in range(4):
        c = slice(i * chunk, (i + 1) * chunk)
        p = u[:, c] if i == 0 else F.adaptive_max_pool2d(u[:, c], (H >> i, W >> i))
        p = F.conv2d(p, mw[c], mb[c], padding=1, groups=chunk)
        s.append(p if i == 0 else F.interpolate(p, size=(H, W), mode="nearest"))
    return t + F.gelu(F.conv2d(torch.cat(s, 1), aw, ab)) * u


def launches(dev, rounds):
    cases = {}
    for dim in (36, 128):
        cp = -(-dim // 64) * 64
        G = N * H * W * 32
        u = (torch.rand((N, dim, H, W)) * 2 - 1).half()          # (random data: zeros would read fast)
        t = (torch.rand((N, dim, H, W)) * 2 - 1).half()
        sd = SM.fill(3, dim, 1, 2.0, 4, dim)
        mw, mb = torch.cat([sd[f"feats.0.safm.mfr.{i}.weight"] for i in range(4)]), torch.cat([sd[f"feats.0.safm.mfr.{i}.bias"] for i in range(4)])
        aw, ab = sd["feats.0.safm.aggr.weight"], sd["feats.0.safm.aggr.bias"]
        pad = lambda v: R.to_slab(torch.cat([v, torch.zeros((N, cp - dim, H, W), dtype=torch.float16)], 1)).to(dev)
        du, dt, do = pad(u), pad(t), torch.empty((cp // 32, G), dtype=torch.float16, device=dev)
        host = [np.ascontiguousarray(v.numpy().reshape(v.shape[0], -1), np.float32) for v in (aw, ab, mw, mb)]
        cases[f"safm dim {dim}"] = (dim, lambda du=du, dt=dt, do=do, G=G, dim=dim, cp=cp, host=host: L.timed_launches(lambda: L.check(
            L.lib.innfer_safm(du.data_ptr(), G, dt.data_ptr(), G, do.data_ptr(), G, N, H, W, dim, cp, *[v.ctypes.data for v in host], None)))[0][1])
        g = [v.to(dev).half() for v in (u, t, mw, mb, aw, ab)]

        def torch_ms(g=g):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            composed(*g)
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1)
        cases[f"torch composed dim {dim}"] = (dim, torch_ms)
    ms = {k: [] for k in cases}
    for r in range(rounds + 2):
        for k, (_, fn) in cases.items():
            v = fn()
            if r >= 2:
                ms[k].append(v)
    res = {}
    for k, (dim, _) in cases.items():
        med, floor = statistics.median(ms[k]), 6.0 * dim * N * H * W / HBM_PEAK * 1e3
        res[k] = dict(median_ms=round(med, 4), min_ms=round(min(ms[k]), 4), byte_floor_ms=round(floor, 4), time_over_byte_floor=round(med / floor, 2))
    return res


def forwards(dev, rounds):
    from innfer_amd.architectures.SAFMN_arch import SAFMN
    x = torch.from_numpy(synth.uniform((N, 3, H, W), 5)).half().to(dev)
    nets = {}
    for name, (dim, nb) in MODELS.items():
        net = SAFMN(dim=dim, n_blocks=nb, ffn_scale=2.0, upscaling_factor=4)
        net.load_state_dict(SM.fill(3, dim, nb, 2.0, 4, 9), strict=True)
        nets[name] = net.to(dev).eval()
        nets[name](x)
    ms = {k: [] for k in nets}
    for _ in range(rounds):
        for k, net in nets.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            net(x)
            torch.cuda.synchronize()
            ms[k].append((time.perf_counter() - t0) * 1e3)
    return {k: dict(median_ms=round(statistics.median(v), 3), min_ms=round(min(v), 3)) for k, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {"launches_16x200x200": launches(dev, a.rounds), "clock_after_launches_mhz": shader_clock_mhz()}
    res["forwards_16x200x200"] = forwards(dev, a.rounds)
    res["clock_after_forwards_mhz"] = shader_clock_mhz()
    print(json.dumps(res, indent=1))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
