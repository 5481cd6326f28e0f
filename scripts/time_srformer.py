"""SRFormer on the MI355X: the permuted window attention next to win_attn16 as the yardstick, the depthwise 5 x 5 conv, and ms per forward with the split by launch kind
(measurement only; needs the GPU).

(a) Launches alone, in ONE process, alternating launch by launch, medians over the rounds (the library's launch timer around the launch function the network calls):
    innfer_window_attention_perm at C 180 / 6 heads of 30 on windows of 16, 22, 24 and innfer_window_attention16 at 6 x 30, shift 0 and ws / 2, on 16 tiles of 200 x 200
    and on 540 x 960 whole, each padded to its own window (208 / 220 / 216; 544 x 960 / 550 x 968 / 552 x 960).  TFLOP/s count the two products on the real d: 4 ws^2
    (ws / 2)^2 d per window and head (a quarter of win_attn16's keys).  What to read off: ms per PIXEL and head against the yardstick (the permuted form has a quarter of
    the matrix work, no dense bias stream, but an element-wise two-byte gather and one LDS read per score -- the first suspects where it does not come out ahead, window 16
    above all, where a workgroup has only 16 query tiles of 4 + 4 MFMAs behind its gather).  innfer_dwconv5x5_gelu_add at hidden 120 and 360 on the same two grids: GB/s
    over one read and one write of the slab.
(b) Forwards, alternating round after round: the light form (C 60, 4 x 6 blocks, window 16, pixelshuffledirect x4) and the classical one (C 180, 6 x 6, window 22 and 24,
    pixelshuffle x4), random weights (tests/_srformer_ref.fill), fp16 I/O, at 16 x 200 x 200 and 1 x 540 x 960: the host clock around innfer_net_forward ending in a device
    synchronise, and innfer_net_forward_timed's device-event time per launch summed by kind (8000 LayerNorm, 8001 the attention, 8013 the depthwise conv, 16 NT + out_mode
    the convs and Linears, 8002 / 8003 pad / crop) for the median round.
The shader clock is read after each part.

    python scripts/time_srformer.py [--rounds 7] [--out FILE] [--skip-forwards]
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

import _srformer_ref as SF          # noqa: E402
import innfer_amd.lib as L          # noqa: E402
from innfer_amd import synth        # noqa: E402
from time_compact import shader_clock_mhz          # noqa: E402

MODELS = {"light_x4_ws16": (60, (6,) * 4, 16, "pixelshuffledirect"), "classical_x4_ws22": (180, (6,) * 6, 22, "pixelshuffle"), "classical_x4_ws24": (180, (6,) * 6, 24, "pixelshuffle")}
SHAPES = {"16x200x200": (16, 200, 200), "1x540x960": (1, 540, 960)}
C_ATT, NH, D = 180, 6, 30


def pad_to(n, ws):
    return -(-n // ws) * ws


def launches_alone(dev, rounds):
    rnd = lambda *shape: (torch.rand(shape, device=dev) * 2 - 1).half()          # (random data: zeros would read fast)
    cases = {}
    for sname, (N, H, W) in SHAPES.items():
        Hp, Wp = pad_to(H, 16), pad_to(W, 16)
        G = N * Hp * Wp * 32
        qkv = rnd(3 * NH, G)
        qkv.view(3 * NH, -1, 32)[:, :, D:] = 0
        out = torch.empty((NH, G), dtype=torch.float16, device=dev)
        dense = np.ascontiguousarray(synth.uniform((NH, 256, 256), 19, -2, 2))
        for shift in (0, 8):
            cases[f"{sname} win_attn16 shift {shift}"] = ("attn", 16, 256, N * Hp * Wp, (lambda qkv=qkv, out=out, G=G, N=N, Hp=Hp, Wp=Wp, shift=shift: L.check(
                L.lib.innfer_window_attention16(qkv.data_ptr(), G, out.data_ptr(), G, dense.ctypes.data, N, Hp, Wp, NH, D, shift, 16, None))))
        for ws in (16, 22, 24):
            Hp, Wp = pad_to(H, ws), pad_to(W, ws)
            G = N * Hp * Wp * 32
            q, kv, o = rnd(NH, G), rnd(4, G), torch.empty((NH, G), dtype=torch.float16, device=dev)
            q.view(NH, -1, 32)[:, :, D:] = 0
            kv.view(2, 2, -1, 32)[:, 1, :, C_ATT // 4 - 32:] = 0
            table = np.ascontiguousarray(synth.uniform((NH, (ws - 1) ** 2), 20, -2, 2))
            for shift in (0, ws // 2):
                cases[f"{sname} win_attn_perm ws {ws} shift {shift}"] = ("attn", ws, ws * ws // 4, N * Hp * Wp, (lambda q=q, kv=kv, o=o, G=G, N=N, Hp=Hp, Wp=Wp, ws=ws, shift=shift, table=table: L.check(
                    L.lib.innfer_window_attention_perm(q.data_ptr(), G, kv.data_ptr(), G, o.data_ptr(), G, table.ctypes.data, N, Hp, Wp, C_ATT, NH, ws, shift, None))))
        Hp, Wp = pad_to(H, 16), pad_to(W, 16)
        G = N * Hp * Wp * 32
        for hid in (120, 360):
            cp = pad_to(hid, 64)
            x, y = rnd(cp // 32, G), torch.empty((cp // 32, G), dtype=torch.float16, device=dev)
            taps, bias = np.ascontiguousarray(synth.uniform((hid, 25), 21, -0.3, 0.3)), np.ascontiguousarray(synth.uniform((hid,), 22, -0.5, 0.5))
            cases[f"{sname} dwconv5 hidden {hid}"] = ("dw", cp, hid, N * Hp * Wp, (lambda x=x, y=y, G=G, N=N, Hp=Hp, Wp=Wp, hid=hid, cp=cp, taps=taps, bias=bias: L.check(
                L.lib.innfer_dwconv5x5_gelu_add(x.data_ptr(), G, y.data_ptr(), G, N, Hp, Wp, hid, cp, taps.ctypes.data, bias.ctypes.data, None))))
    ms = {k: [] for k in cases}
    for r in range(rounds + 2):
        for k, case in cases.items():                                            # alternating launch by launch
            t = L.timed_launches(case[4])[0][1]
            if r >= 2:
                ms[k].append(t)
    res = {}
    for k, (what, a, b, npx, _) in cases.items():
        med = statistics.median(ms[k])
        e = dict(median_ms=round(med, 4), min_ms=round(min(ms[k]), 4), pixels=npx, ns_per_pixel=round(med * 1e6 / npx, 4))
        if what == "attn":           # a: window, b: keys per window
            e["tflops_per_s_real_d"] = round(npx * NH * 4.0 * b * D / med / 1e9, 1)
        else:                        # a: c_pad, b: hidden
            e["gbytes_per_s"] = round(npx * a * 4.0 / med / 1e6, 1)
        res[k] = e
    for sname in SHAPES:
        for k, e in res.items():
            if k.startswith(sname + " win_attn_perm"):
                y = res[f"{sname} win_attn16 shift {0 if k.endswith(' 0') else 8}"]
                e["time_per_pixel_vs_win_attn16"] = round(e["ns_per_pixel"] / y["ns_per_pixel"], 3)
    return res


def build(dev, name):
    from innfer_amd.architectures.SRFormer_arch import SRFormer
    Cc, depths, ws, ups = MODELS[name]
    net = SRFormer(embed_dim=Cc, depths=list(depths), num_heads=[6] * len(depths), window_size=ws, mlp_ratio=2.0, upscale=4, upsampler=ups)
    net.load_state_dict(SF.fill(3, Cc, depths, 6, 2.0, 4, ups, "1conv", ws, seed=9), strict=True)
    return net.to(dev).eval()


def forwards(dev, rounds):
    cases = []
    for m in MODELS:
        net = build(dev, m)
        for sname, (N, H, W) in SHAPES.items():
            x = torch.from_numpy(synth.uniform((N, 3, H, W), 5)).half().to(dev)
            y = net(x)                                                       # warm-up of every shape
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
            full = y                                                         # (the engine pads and crops inside: it writes exactly the result)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            L.check(L.lib.innfer_net_forward(net._handle, x.data_ptr(), L.F16, full.data_ptr(), L.F16, N, H, W, ws.data_ptr(), ws.numel(), stream))
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            L.check(L.lib.innfer_net_forward_timed(net._handle, x.data_ptr(), L.F16, full.data_ptr(), L.F16, N, H, W, ws.data_ptr(), ws.numel(), stream, cap, ms, fl, by, kind, C.byref(n)))
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--skip-forwards", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0)}
    res["launches_alone"] = launches_alone(dev, args.rounds)
    res["sclk_mhz_after_launches"] = shader_clock_mhz()

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
