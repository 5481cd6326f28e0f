"""DRCT on the MI355X: ms per forward, the split by launch kind, and the 16 x 16 attention launches alone -- the wide-head kernel next to win_attn16 as the yardstick
(measurement only; needs the GPU).

Two published shapes with random weights (tests/_drct_ref.fill) and random input, fp16 I/O:
    DRCT x4     embed_dim 180, 6 dense groups, num_heads 6 (per block 6, 4, 2, 6, 4 heads of 30, 53, 122, 46, 77 channels), mlp_ratio 2
    DRCT-L x4   the same with 12 dense groups
each at 16 tiles of 200 x 200 (what the chop path hands the engine; padded to 208 x 208 inside it) and at 540 x 960 whole (padded to 544 x 960).
(a) The attention launch alone, in ONE process, alternating launch by launch, medians over the rounds (the library's launch timer around the launch function the network
    calls): innfer_window_attention16 at (nH, d) = (6, 30), the yardstick, and innfer_window_attention16_wide at (4, 53), (2, 122), (6, 46), (4, 77), shift 0 and 8, on the
    16 x 208 x 208 and 544 x 960 grids.  TFLOP/s count the two products on the REAL d: 4 x 256 x 256 x d per window and head.
(b) The four (model, shape) forwards alternate, round after round: the host clock around innfer_net_forward ending in a device synchronise, and
    innfer_net_forward_timed's device-event time per launch, summed by kind (0 the first conv, 16 NT + out_mode the convs -- 64 slab convs and Linears, 17 the planar last
    conv, 66 the PixelShuffle(2) store --, 8000 LayerNorm, 8001 the window attentions, 8002 / 8003 pad / crop) for the median round.
The shader clock is read after each part.

    python scripts/time_drct.py [--rounds 7] [--out FILE] [--skip-forwards]
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

import _drct_ref as DR              # noqa: E402
import innfer_amd.lib as L          # noqa: E402
from innfer_amd import synth        # noqa: E402
from time_compact import shader_clock_mhz          # noqa: E402

MODELS = {"DRCT_x4": 6, "DRCT-L_x4": 12}
SHAPES = {"16x200x200": (16, 200, 200), "1x540x960": (1, 540, 960)}
HEADS = ((6, 30), (4, 53), (2, 122), (6, 46), (4, 77))          # (6, 30): win_attn16, the yardstick


def build(dev, name):
    from innfer_amd.architectures.DRCT_arch import DRCT
    R = MODELS[name]
    net = DRCT(embed_dim=180, depths=[6] * R, num_heads=[6] * R, window_size=16, mlp_ratio=2.0, upscale=4, upsampler="pixelshuffle")
    net.load_state_dict(DR.fill(3, 180, R, 6, 2.0, 4, seed=9), strict=True)
    return net.to(dev).eval()


def forwards(dev, rounds):
    cases = []
    for m in MODELS:
        net = build(dev, m)
        for sname, (N, H, W) in SHAPES.items():
            x = torch.from_numpy(synth.uniform((N, 3, H, W), 5)).half().to(dev)
            y = net(x)                                                       # warm-up of every shape; sizes the workspace
            net.release_workspace()
            ws = torch.empty(L.lib.innfer_net_workspace_bytes(net._handle, N, H, W), dtype=torch.uint8, device=dev)
            cases.append((m, sname, net, x, y, ws))
    cap = 16384
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
        padded = x.shape[2] % 16 != 0 or x.shape[3] % 16 != 0
        out[f"{m} {s}"] = dict(launches=len(med), launches_formula=net.launches(padded), forward_wall_ms_median=statistics.median(wall[(m, s)]),
                               forward_wall_ms_min=min(wall[(m, s)]), kernel_sum_ms_median=sorted(sums)[len(sums) // 2], kernel_sum_ms_min=min(sums),
                               workspace_bytes=int(ws.numel()), algorithmic_tflops=net.flops(x.shape[0], x.shape[2], x.shape[3]) / 1e12,
                               by_kind={k: dict(launches=c, ms=round(t, 4), tflops_per_s=round(f / t / 1e9, 1) if t > 0 and f > 0 else None,
                                                gbytes_per_s=round(b / t / 1e6, 1) if t > 0 and b > 0 else None) for k, (c, t, f, b) in sorted(by_kind.items(), key=lambda kv: -kv[1][1])})
    return out


def attention_alone(dev, rounds):
    table = np.ascontiguousarray(synth.uniform((8, 256, 256), 19, -2, 2))
    bufs = {}
    for sname, (N, Hp, Wp) in {"16x208x208": (16, 208, 208), "1x544x960": (1, 544, 960)}.items():
        G = N * Hp * Wp * 32
        for nH, d in HEADS:
            hg = nH * -(-d // 32)
            qkv = (torch.rand((3 * hg, G), device=dev) * 2 - 1).half()          # (random data: zeros would read fast)
            v = qkv.view(3, nH, -1, N * Hp * Wp, 32)                             # [which, head, group of the head, pixel, channel]
            for g in range(v.shape[2]):
                v[:, :, g, :, max(0, min(32, d - 32 * g)):] = 0
            bufs[(sname, nH, d)] = (N, Hp, Wp, G, qkv, torch.empty((hg, G), dtype=torch.float16, device=dev))

    def run(key, shift):
        N, Hp, Wp, G, qkv, out = bufs[key]
        nH, d = key[1], key[2]
        if d <= 32:
            L.check(L.lib.innfer_window_attention16(qkv.data_ptr(), G, out.data_ptr(), G, table.ctypes.data, N, Hp, Wp, nH, d, shift, 16, None))
        else:
            L.check(L.lib.innfer_window_attention16_wide(qkv.data_ptr(), G, out.data_ptr(), G, table.ctypes.data, N, Hp, Wp, nH, d, shift, None))
    ms = {(key, shift): [] for key in bufs for shift in (0, 8)}
    for r in range(rounds + 2):
        for key in bufs:                                                        # alternating launch by launch
            for shift in (0, 8):
                t = L.timed_launches(lambda: run(key, shift))[0][1]
                if r >= 2:
                    ms[(key, shift)].append(t)
    res = {}
    for (key, shift), v in ms.items():
        sname, nH, d = key
        N, Hp, Wp = bufs[key][:3]
        items = N * nH * (Hp // 16) * (Wp // 16)
        med = statistics.median(v)
        res[f"{sname} nH {nH} d {d} shift {shift}"] = dict(kernel="win_attn16" if d <= 32 else f"win_attn16_wide G {-(-d // 32)}", median_ms=round(med, 4), min_ms=round(min(v), 4),
                                                           windows_x_heads=items, tflops_per_s_real_d=round(items * 4.0 * 256 * 256 * d / med / 1e9, 1),
                                                           bias_read_gbytes_per_s=round(items * 65536 * 4 / med / 1e6, 1))
    for sname in ("16x208x208", "1x544x960"):
        for shift in (0, 8):
            y = res[f"{sname} nH 6 d 30 shift {shift}"]["tflops_per_s_real_d"]
            for nH, d in HEADS[1:]:
                e = res[f"{sname} nH {nH} d {d} shift {shift}"]
                e["share_of_yardstick"] = round(e["tflops_per_s_real_d"] / y, 3)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--skip-forwards", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0)}
    res["attention_alone"] = attention_alone(dev, args.rounds)
    res["sclk_mhz_after_attention"] = shader_clock_mhz()

    def dump():
        txt = json.dumps(res, indent=1)
        if args.out:
            with open(args.out, "w") as f:
                f.write(txt + "\n")
        return txt
    dump()
    if not args.skip_forwards:
        res["forwards"] = forwards(dev, args.rounds)
        res["sclk_mhz_after_forwards"] = shader_clock_mhz()
    print(dump())


if __name__ == "__main__":
    main()
