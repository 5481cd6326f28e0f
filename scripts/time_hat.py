"""HAT on the MI355X: ms per forward, the split by launch kind, and the two attention launches alone (measurement only; needs the GPU).

Two published shapes with random weights (tests/_hat_ref.fill) and random input, fp16 I/O:
    HAT x4     embed_dim 180, depths [6] * 6, 6 heads, mlp_ratio 2, compress_ratio 3, squeeze_factor 30
    HAT-S x4   embed_dim 144, depths [6] * 6, 6 heads, mlp_ratio 2, compress_ratio 24, squeeze_factor 24
each at 16 tiles of 200 x 200 (what the chop path hands the engine; padded to 208 x 208 inside it) and at 540 x 960 whole (padded to 544 x 960).
(a) The four (model, shape) cases alternate in one process, round after round: the host clock around innfer_net_forward ending in a device synchronise, and
    innfer_net_forward_timed's device-event time per launch, summed by kind (0 the first conv, 16 NT + out_mode the convs -- 64 slab convs and Linears, 17 the planar last
    conv, 66 the PixelShuffle(2) store --, 8000 LayerNorm, 8001 the two window attentions, 8002 / 8003 pad / crop, 8005 / 8006 / 8007 the channel attention's sums,
    squeeze / excite and scale-add) for the median round.  Medians and minima over the rounds.
(b) The attention launch alone (innfer_window_attention16: the library's launch timer around win_attn16_launch) on HAT's 16 x 208 x 208 and 544 x 960 grids: key window
    16 with shift 0 and 8, key window 24, alternating.  Bytes per launch: q and the result once, k and v once per window (the gather), and the dense bias (256 x kw^2
    floats per window and head: table reads that mostly hit the cache, reported apart).
The shader clock is read after the runs.

    python scripts/time_hat.py [--rounds 7] [--out FILE]
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

import _hat_ref as HR               # noqa: E402
import innfer_amd.lib as L          # noqa: E402
from innfer_amd import synth        # noqa: E402
from time_compact import shader_clock_mhz          # noqa: E402

MODELS = {"HAT_x4": (180, (6,) * 6, 6, 3, 30), "HAT-S_x4": (144, (6,) * 6, 6, 24, 24)}
SHAPES = {"16x200x200": (16, 200, 200), "1x540x960": (1, 540, 960)}


def build(dev, name):
    from innfer_amd.architectures.HAT_arch import HAT
    Cc, depths, nH, cr, sq = MODELS[name]
    net = HAT(embed_dim=Cc, depths=depths, num_heads=[nH] * len(depths), window_size=16, compress_ratio=cr, squeeze_factor=sq, mlp_ratio=2.0, upscale=4, upsampler="pixelshuffle")
    net.load_state_dict(HR.fill(3, Cc, depths, nH, 2.0, 4, cr, sq, seed=9), strict=True)
    return net.to(dev).eval()


def forwards(dev, rounds):
    nets = {m: build(dev, m) for m in MODELS}
    cases = []
    for m, net in nets.items():
        for sname, (N, H, W) in SHAPES.items():
            x = torch.from_numpy(synth.uniform((N, 3, H, W), 5)).half().to(dev)
            y = net(x)                                                       # warm-up of every shape; sizes the workspace
            ws = torch.empty(L.lib.innfer_net_workspace_bytes(net._handle, N, H, W), dtype=torch.uint8, device=dev)
            cases.append((m, sname, net, x, y, ws))
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
                per[(m, s)].append([(kind[i], ms[i], fl[i], by[i]) for i in range(n.value)])
    out = {}
    for m, s, net, x, y, ws in cases:
        sums = [sum(q[1] for q in p) for p in per[(m, s)]]
        med = per[(m, s)][sums.index(sorted(sums)[len(sums) // 2])]
        by_kind = {}
        for k, t, f, b in med:
            e = by_kind.setdefault(str(k), [0, 0.0, 0.0, 0.0]); e[0] += 1; e[1] += t; e[2] += f; e[3] += b
        out[f"{m} {s}"] = dict(launches=len(med), forward_wall_ms_median=statistics.median(wall[(m, s)]), forward_wall_ms_min=min(wall[(m, s)]),
                               kernel_sum_ms_median=sorted(sums)[len(sums) // 2], kernel_sum_ms_min=min(sums), workspace_bytes=int(ws.numel()),
                               algorithmic_tflops=net.flops(x.shape[0], x.shape[2], x.shape[3]) / 1e12,
                               by_kind={k: dict(launches=c, ms=round(t, 4), tflops_per_s=round(f / t / 1e9, 1) if t > 0 and f > 0 else None,
                                                gbytes_per_s=round(b / t / 1e6, 1) if t > 0 and b > 0 else None) for k, (c, t, f, b) in sorted(by_kind.items(), key=lambda kv: -kv[1][1])})
    return out


def attention_alone(dev, rounds):
    nH, d = 6, 30
    tables = {kw: np.ascontiguousarray(synth.uniform((nH, 256, kw * kw), 3 + kw, -2, 2)) for kw in (16, 24)}
    bufs = {}
    for sname, (N, Hp, Wp) in {"16x208x208": (16, 208, 208), "1x544x960": (1, 544, 960)}.items():
        G = N * Hp * Wp * 32
        qkv = (torch.rand((3 * nH, G), device=dev) * 2 - 1).half()          # (random data: zeros would read fast)
        qkv.view(3 * nH, -1, 32)[:, :, d:] = 0
        bufs[sname] = (N, Hp, Wp, G, qkv, torch.empty((nH, G), dtype=torch.float16, device=dev))
    run = lambda b, kw, shift: L.check(L.lib.innfer_window_attention16(b[4].data_ptr(), b[3], b[5].data_ptr(), b[3], tables[kw].ctypes.data, b[0], b[1], b[2], nH, d, shift, kw, None))
    forms = ((16, 0), (16, 8), (24, 0))
    ms = {(s, f): [] for s in bufs for f in forms}
    for r in range(rounds + 2):
        for s, b in bufs.items():
            for kw, shift in forms:
                t = L.timed_launches(lambda: run(b, kw, shift))[0][1]
                if r >= 2:
                    ms[(s, (kw, shift))].append(t)
    res = {}
    for (s, (kw, shift)), v in ms.items():
        b = bufs[s]
        items = b[0] * nH * (b[1] // 16) * (b[2] // 16)
        med = statistics.median(v)
        res[f"{s} keys {kw} shift {shift}"] = dict(median_ms=med, min_ms=min(v), windows_x_heads=items,
                                                   slab_gbytes_per_s=round(items * (256 * 2 + kw * kw * 2) * 32 * 2 / med / 1e6, 1),
                                                   bias_read_gbytes_per_s=round(items * 256 * kw * kw * 4 / med / 1e6, 1),
                                                   tflops_per_s=round(items * 4.0 * 256 * kw * kw * 32 / med / 1e9, 1))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "forwards": forwards(dev, args.rounds)}
    res["sclk_mhz_after_forwards"] = shader_clock_mhz()
    res["window_attention16_alone_nH6_d30"] = attention_alone(dev, 2 * args.rounds)
    res["sclk_mhz_after_attention"] = shader_clock_mhz()
    txt = json.dumps(res, indent=1)
    print(txt)
    if args.out:
        with open(args.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
