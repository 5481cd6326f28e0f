"""Swin2SR on the MI355X next to SwinIR: ms per forward, the split by launch kind, and the two attention and the two LayerNorm launches alone (measurement only; needs the GPU).

Swin2SR with SwinIR-M's and SwinIR-L's shapes (random weights: tests/_swin2sr_ref.fill) and SwinIR itself (scripts/time_swinir.py's two models), fp16 I/O:
    M x4   embed_dim 180, depths [6] * 6, 6 heads, mlp_ratio 2, pixelshuffle, '1conv'
    L x4   embed_dim 240, depths [6] * 9, 8 heads, mlp_ratio 2, nearest+conv, '3conv'
each at 16 tiles of 200 x 200 and at 540 x 960 whole (padded to 544 x 960 inside the engine).
(a) The eight (family, model, shape) cases alternate in one process, round after round: the host clock around innfer_net_forward ending in a device synchronise, and
    innfer_net_forward_timed's device-event time per launch, summed by kind (as scripts/time_swinir.py; 8008 is LayerNorm + residual) for the median round.
(b) innfer_window_attention and innfer_window_attention_cos (6 heads of 30), innfer_layer_norm and innfer_layer_norm_add (C 180 in 192) alone on the 16 x 200 x 200 and
    544 x 960 grids, alternating, with the library's launch timer.
The shader clock is read after the runs.

    python scripts/time_swin2sr.py [--rounds 9] [--out FILE]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _swin2sr_ref as S2           # noqa: E402
import _swinir_ref as SR            # noqa: E402
import innfer_amd.lib as L          # noqa: E402
from innfer_amd import synth        # noqa: E402
from time_compact import shader_clock_mhz          # noqa: E402
from time_swinir import MODELS, SHAPES              # noqa: E402


def build(dev, family, name):
    Cc, depths, nH, ups, resi = MODELS[name]
    kw = dict(embed_dim=Cc, depths=depths, num_heads=[nH] * len(depths), window_size=8, mlp_ratio=2.0, upscale=4, upsampler=ups, resi_connection=resi)
    if family == "swinir":
        from innfer_amd.architectures.SwinIR_arch import SwinIR
        net = SwinIR(**kw)
        net.load_state_dict(SR.fill(3, Cc, depths, nH, 2.0, 4, ups, resi, seed=9), strict=True)
    else:
        from innfer_amd.architectures.Swin2SR_arch import Swin2SR
        net = Swin2SR(**kw)
        net.load_state_dict(S2.fill(3, Cc, depths, nH, 2.0, 4, ups, resi, 512, seed=9), strict=True)
    return net.to(dev).eval()


def forwards(dev, rounds):
    cases = []
    for m in MODELS:
        for family in ("swinir", "swin2sr"):
            net = build(dev, family, m)
            for sname, (N, H, W) in SHAPES.items():
                x = torch.from_numpy(synth.uniform((N, 3, H, W), 5)).half().to(dev)
                y = net(x)                                                       # warm-up of every shape; sizes the workspace
                ws = torch.empty(L.lib.innfer_net_workspace_bytes(net._handle, N, H, W), dtype=torch.uint8, device=dev)
                cases.append((f"{family} {m}", sname, net, x, y, ws))
    cap = 8192
    ms, fl, by, kind, n = (C.c_float * cap)(), (C.c_double * cap)(), (C.c_double * cap)(), (C.c_int * cap)(), C.c_int()
    stream = torch.cuda.current_stream(dev).cuda_stream
    wall = {(m, s): [] for m, s, *_ in cases}
    per = {(m, s): [] for m, s, *_ in cases}
    for r in range(rounds + 1):
        for m, s, net, x, y, ws in cases:
            N, _, H, W = x.shape
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            L.check(L.lib.innfer_net_forward(net._handle, x.data_ptr(), L.F16, y.data_ptr(), L.F16, N, H, W, ws.data_ptr(), ws.numel(), stream))
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            L.check(L.lib.innfer_net_forward_timed(net._handle, x.data_ptr(), L.F16, y.data_ptr(), L.F16, N, H, W, ws.data_ptr(), ws.numel(), stream, cap, ms, fl, by, kind, C.byref(n)))
            if r >= 1:
                wall[(m, s)].append((t1 - t0) * 1e3)
                per[(m, s)].append([(kind[i], ms[i], fl[i]) for i in range(n.value)])
    out = {}
    for m, s, net, x, y, ws in cases:
        sums = [sum(q[1] for q in p) for p in per[(m, s)]]
        med = per[(m, s)][sums.index(sorted(sums)[len(sums) // 2])]
        by_kind = {}
        for k, t, f in med:
            e = by_kind.setdefault(str(k), [0, 0.0, 0.0]); e[0] += 1; e[1] += t; e[2] += f
        out[f"{m} {s}"] = dict(launches=len(med), forward_wall_ms_median=statistics.median(wall[(m, s)]), forward_wall_ms_min=min(wall[(m, s)]),
                               kernel_sum_ms_median=sorted(sums)[len(sums) // 2], kernel_sum_ms_min=min(sums), workspace_bytes=int(ws.numel()),
                               algorithmic_tflops=net.flops(x.shape[0], x.shape[2], x.shape[3]) / 1e12,
                               by_kind={k: dict(launches=c, ms=round(t, 4), tflops_per_s=round(f / t / 1e9, 1) if t > 0 and f > 0 else None) for k, (c, t, f) in sorted(by_kind.items(), key=lambda kv: -kv[1][1])})
    return out


def launches_alone(dev, rounds):
    nH, d, Cc, cp = 6, 30, 180, 192
    table = np.ascontiguousarray(synth.uniform((nH, 64, 64), 3, 0, 16))
    tau = np.ascontiguousarray(np.geomspace(3.0, 100.0, nH).astype(np.float32))
    gamma, beta = np.ascontiguousarray(synth.uniform((Cc,), 4, 0.5, 1.5)), np.ascontiguousarray(synth.uniform((Cc,), 5, -0.2, 0.2))
    bufs = {}
    for sname, (N, Hp, Wp) in {"16x200x200": (16, 200, 200), "1x544x960": (1, 544, 960)}.items():
        G = N * Hp * Wp * 32
        qkv = (torch.rand((3 * nH, G), device=dev) * 2 - 1).half()          # (random data: zeros would read fast)
        qkv.view(3 * nH, -1, 32)[:, :, d:] = 0
        bufs[sname] = (N, Hp, Wp, G, qkv, torch.empty((nH, G), dtype=torch.float16, device=dev), (torch.rand((cp // 32, G), device=dev) * 2 - 1).half(),
                       (torch.rand((cp // 32, G), device=dev) * 2 - 1).half(), torch.empty((cp // 32, G), dtype=torch.float16, device=dev))
    run = {
        "window_attention": lambda b, shift: L.lib.innfer_window_attention(b[4].data_ptr(), b[3], b[5].data_ptr(), b[3], table.ctypes.data, b[0], b[1], b[2], nH, d, shift, None),
        "window_attention_cos": lambda b, shift: L.lib.innfer_window_attention_cos(b[4].data_ptr(), b[3], b[5].data_ptr(), b[3], table.ctypes.data, tau.ctypes.data, b[0], b[1], b[2],
                                                                                   nH, d, shift, None),
        "layer_norm": lambda b, shift: L.lib.innfer_layer_norm(b[6].data_ptr(), b[3], b[8].data_ptr(), b[3], b[0] * b[1] * b[2], Cc, cp, gamma.ctypes.data, beta.ctypes.data, 1e-5, None),
        "layer_norm_add": lambda b, shift: L.lib.innfer_layer_norm_add(b[6].data_ptr(), b[3], b[7].data_ptr(), b[3], b[8].data_ptr(), b[3], b[0] * b[1] * b[2], Cc, cp, gamma.ctypes.data,
                                                                       beta.ctypes.data, 1e-5, None),
    }
    keys = [(k, s, sh) for k in run for s in bufs for sh in ((0, 4) if k.startswith("window") else (0,))]
    ms = {k: [] for k in keys}
    for r in range(rounds + 2):
        for k, s, sh in keys:
            t = L.timed_launches(lambda: L.check(run[k](bufs[s], sh)))[0][1]
            if r >= 2:
                ms[(k, s, sh)].append(t)
    res = {}
    for (k, s, sh), v in ms.items():
        b = bufs[s]
        med = statistics.median(v)
        if k.startswith("window"):
            items = b[0] * nH * (b[1] // 8) * (b[2] // 8)
            res[f"{k} {s} shift {sh}"] = dict(median_ms=med, min_ms=min(v), windows_x_heads=items, gbytes_per_s=round(items * 64 * 32 * 2 * 4 / med / 1e6, 1),
                                              tflops_per_s=round(items * 4.0 * 64 * 64 * 32 / med / 1e9, 1))
        else:
            px = b[0] * b[1] * b[2]
            res[f"{k} {s}"] = dict(median_ms=med, min_ms=min(v), pixels=px, gbytes_per_s=round(px * cp * 2 * (3 if k.endswith("add") else 2) / med / 1e6, 1))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "forwards": forwards(dev, args.rounds)}
    res["sclk_mhz_after_forwards"] = shader_clock_mhz()
    res["launches_alone_nH6_d30_C180"] = launches_alone(dev, 2 * args.rounds)
    res["sclk_mhz_after_launches"] = shader_clock_mhz()
    txt = json.dumps(res, indent=1)
    print(txt)
    if args.out:
        with open(args.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
