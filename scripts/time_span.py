"""SPAN on the MI355X: what the act-9 / act-10 epilogues cost a launch, and whole 1080p frames (measurement only; needs the GPU).

(a) one 64 -> 64 conv at 1 x 64 x 1080 x 1920 (plane-order panels, as the network runs it) with act 9 (SiLU) and with act 10 (the SPAB gate, d_res1 = a slab of the
    output's size) against the same launch with act 1 (LeakyReLU(0.2)), and with act 1 plus the same residual ("act1r", the 8 x 1 consumer form the new epilogues
    run on): the four alternate in one process, device-event time per launch (the library's launch
    timer), median and minimum of the rounds.
(b) innfer_net_forward_timed of whole 1080p -> 4x frames, feature_channels 48, fp16 and uint8 I/O: per-kernel times of the median frame, summed by kind (0 first
    conv, 64 the 3x3 slab convs and conv_cat, 6001 the SiLU pass, 6000 the PixelShuffle store), and the frame's host-clock time around a synchronised forward.

    python scripts/time_span.py [--rounds 30] [--out FILE]
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

import _span_ref as SR              # noqa: E402
import innfer_amd.lib as L          # noqa: E402
from innfer_amd import synth        # noqa: E402
from time_compact import shader_clock_mhz          # noqa: E402


def one_launch(dev, rounds):
    N, Cc, K, H, W = 1, 64, 64, 1080, 1920
    G = N * H * W * 32
    x = (torch.rand((2, G), device=dev) * 2 - 1).half()               # (random data: zeros would read fast)
    res = (torch.rand((2, G), device=dev) * 2 - 1).half()
    w = np.ascontiguousarray(synth.uniform((K, Cc, 3, 3), 2, -1, 1) / np.float32(np.sqrt(9 * Cc)))
    packed = np.zeros(L.lib.innfer_conv3x3_packed_bytes(K, Cc), np.uint8)
    L.check(L.lib.innfer_pack_conv3x3_rows(w.ctypes.data, K, Cc, 1, packed.ctypes.data))
    d_packed = torch.from_numpy(packed).to(dev)
    d_bias = torch.from_numpy(synth.uniform((64,), 3, -1, 1)).to(dev)
    out = torch.empty((2, G), dtype=torch.float16, device=dev)

    def run(act):
        # "1r": LeakyReLU with a memory residual on the 8 x 1 consumer form -- what the gate's residual load alone costs, without its transcendentals
        a = L.ConvArgs(d_in=x.data_ptr(), in_group_stride=G, C=Cc, d_packed=d_packed.data_ptr(), d_bias=d_bias.data_ptr(), d_out=out.data_ptr(), out_group_stride=G,
                       K=K, N=N, H=H, W=W, plane_rows=1, act=1 if act == "1r" else act)
        if act in (10, "1r"):
            a.d_res1, a.res1_group_stride, a.res1_scale = res.data_ptr(), G, 1.0
        if act == "1r":
            L.check(L.lib.innfer_conv3x3_f16_grid(C.byref(a), 0, None))
        else:
            L.check(L.lib.innfer_conv3x3_f16(C.byref(a), None))

    acts = (1, "1r", 9, 10)
    for _ in range(5):
        for act in acts:
            run(act)
    torch.cuda.synchronize()
    ms = {act: [] for act in acts}
    for _ in range(rounds):
        for act in acts:
            ms[act].append(L.timed_launches(lambda: run(act))[0][1])
    flops = 2.0 * 9 * K * Cc * N * H * W
    return {f"act{act}": dict(median_ms=statistics.median(v), min_ms=min(v), tflops_median=flops / statistics.median(v) / 1e9) for act, v in ms.items()}


def frames(dev, f, u8, rounds):
    from innfer_amd.architectures.SPAN_arch import SPAN
    net = SPAN(3, 3, f, 4)
    net.load_state_dict(SR.fill(3, f, 4, seed=f), strict=True)
    net = net.to(dev).eval()
    H, W = 1080, 1920
    if u8:
        x = torch.from_numpy(synth.image_u8(H, W, 3, 1)).to(dev)
        y = net.forward_u8(x)
        dt = L.U8
    else:
        x = torch.from_numpy(synth.uniform((1, 3, H, W), 5)).half().to(dev)
        y = net(x)
        dt = L.F16
    ws, stream = net._ws, torch.cuda.current_stream(dev).cuda_stream
    cap = 64
    ms, fl, by, kind, n = (C.c_float * cap)(), (C.c_double * cap)(), (C.c_double * cap)(), (C.c_int * cap)(), C.c_int()
    per, wall = [], []
    for r in range(rounds + 3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        L.check(L.lib.innfer_net_forward(net._handle, x.data_ptr(), dt, y.data_ptr(), dt, 1, H, W, ws.data_ptr(), ws.numel(), stream))
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        L.check(L.lib.innfer_net_forward_timed(net._handle, x.data_ptr(), dt, y.data_ptr(), dt, 1, H, W, ws.data_ptr(), ws.numel(), stream, cap, ms, fl, by, kind, C.byref(n)))
        if r >= 3:
            wall.append((t1 - t0) * 1e3)
            per.append([(kind[i], ms[i]) for i in range(n.value)])
    sums = sorted(sum(m for _, m in p) for p in per)
    med = per[[sum(m for _, m in p) for p in per].index(sums[len(sums) // 2])]
    by_kind = {}
    for k, m in med:
        e = by_kind.setdefault(str(k), [0, 0.0]); e[0] += 1; e[1] += m
    return dict(feature_channels=f, io="uint8" if u8 else "fp16", launches=len(med), kernel_sum_ms_median=sums[len(sums) // 2], kernel_sum_ms_min=sums[0],
                frame_wall_ms_median=statistics.median(wall), frame_wall_ms_min=min(wall), by_kind={k: dict(launches=c, ms=m) for k, (c, m) in by_kind.items()},
                ms_per_launch=[round(m, 4) for _, m in med])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "one_launch_1x64x1080x1920": one_launch(dev, args.rounds)}
    res["sclk_mhz_after_launches"] = shader_clock_mhz()
    res["frames_1080p_x4"] = [frames(dev, 48, u8, max(5, args.rounds // 3)) for u8 in (False, True)]
    res["sclk_mhz_after_frames"] = shader_clock_mhz()
    txt = json.dumps(res, indent=1)
    print(txt)
    if args.out:
        with open(args.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
