"""RealPLKSR on the MI355X: what the partial large-kernel conv costs against a trunk conv, and a whole 1080p frame (measurement only; needs the GPU).

(a) one plk_conv launch (k 17 and k 13) at 1 x 64 x 1080 x 1920 (one 32-channel group in, one out) against a 64 -> 64 3x3 launch with LeakyReLU (act 1), the same launch
    with Mish (act 11: half of channel_mixer.0) and the 128 -> 64 launch (channel_mixer.2), all with plane-order panels as the network runs them: the five alternate in one
    process, device-event time per launch (the library's launch timer), median and minimum of the rounds.
(b) innfer_net_forward_timed of a whole 1080p -> 4x frame, 28 blocks, k 17, EA, fp16 I/O: per-kernel times of the median frame, summed by kind (0 first conv, 64 the
    slab convs, 7000 plk_conv, 7001 / 7002 / 7003 GroupNorm statistics / merge / apply + skip, 6000 the shuffle-add tail), and the frame's host-clock time.

    python scripts/time_plksr.py [--rounds 30] [--out FILE]
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

import _plksr_ref as PR             # noqa: E402
import innfer_amd.lib as L          # noqa: E402
from innfer_amd import synth        # noqa: E402
from time_compact import shader_clock_mhz          # noqa: E402


def one_launch(dev, rounds):
    N, H, W = 1, 1080, 1920
    G = N * H * W * 32
    x = (torch.rand((4, G), device=dev) * 2 - 1).half()               # (random data: zeros would read fast)
    out = torch.empty((2, G), dtype=torch.float16, device=dev)
    d_bias = torch.from_numpy(synth.uniform((64,), 3, -1, 1)).to(dev)
    packed = {}
    for Cc in (64, 128):
        w = np.ascontiguousarray(synth.uniform((64, Cc, 3, 3), 2, -1, 1) / np.float32(np.sqrt(9 * Cc)))
        p = np.zeros(L.lib.innfer_conv3x3_packed_bytes(64, Cc), np.uint8)
        L.check(L.lib.innfer_pack_conv3x3_rows(w.ctypes.data, 64, Cc, 1, p.ctypes.data))
        packed[Cc] = torch.from_numpy(p).to(dev)
    wl = {k: np.ascontiguousarray(synth.uniform((16, 16, k, k), 4, -1, 1) / np.float32(np.sqrt(16.0 * k * k))) for k in (17, 13)}

    def run(what):
        if what in ("plk17", "plk13"):
            k = int(what[3:])
            L.check(L.lib.innfer_plk_conv(x.data_ptr(), out.data_ptr(), N, H, W, k, wl[k].ctypes.data, None, None))
            return
        Cc = 128 if what == "conv128_act0" else 64
        a = L.ConvArgs(d_in=x.data_ptr(), in_group_stride=G, C=Cc, d_packed=packed[Cc].data_ptr(), d_bias=d_bias.data_ptr(), d_out=out.data_ptr(), out_group_stride=G,
                       K=64, N=N, H=H, W=W, plane_rows=1, act={"conv64_act1": 1, "conv64_act11": 11, "conv128_act0": 0}[what])
        L.check(L.lib.innfer_conv3x3_f16(C.byref(a), None))

    kinds = ("conv64_act1", "conv64_act11", "conv128_act0", "plk17", "plk13")
    for _ in range(3):
        for what in kinds:
            run(what)
    torch.cuda.synchronize()
    ms = {what: [] for what in kinds}
    for _ in range(rounds):
        for what in kinds:
            ms[what].append(L.timed_launches(lambda: run(what))[0][1])
    return {what: dict(median_ms=statistics.median(v), min_ms=min(v)) for what, v in ms.items()}


def frame(dev, rounds, n_blocks=28):
    from innfer_amd.architectures.PLKSR_arch import RealPLKSR
    net = RealPLKSR(3, 3, 64, n_blocks, 4, 17)
    net.load_state_dict(PR.fill(3, 64, n_blocks, 4, 17, True, seed=9), strict=True)
    net = net.to(dev).eval()
    H, W = 1080, 1920
    x = torch.from_numpy(synth.uniform((1, 3, H, W), 5)).half().to(dev)
    y = net(x)
    ws, stream = net._ws, torch.cuda.current_stream(dev).cuda_stream
    cap = 9 * n_blocks + 8
    ms, fl, by, kind, n = (C.c_float * cap)(), (C.c_double * cap)(), (C.c_double * cap)(), (C.c_int * cap)(), C.c_int()
    per, wall = [], []
    for r in range(rounds + 2):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        L.check(L.lib.innfer_net_forward(net._handle, x.data_ptr(), L.F16, y.data_ptr(), L.F16, 1, H, W, ws.data_ptr(), ws.numel(), stream))
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        L.check(L.lib.innfer_net_forward_timed(net._handle, x.data_ptr(), L.F16, y.data_ptr(), L.F16, 1, H, W, ws.data_ptr(), ws.numel(), stream, cap, ms, fl, by, kind, C.byref(n)))
        if r >= 2:
            wall.append((t1 - t0) * 1e3)
            per.append([(kind[i], ms[i]) for i in range(n.value)])
    sums = sorted(sum(m for _, m in p) for p in per)
    med = per[[sum(m for _, m in p) for p in per].index(sums[len(sums) // 2])]
    by_kind = {}
    for k, m in med:
        e = by_kind.setdefault(str(k), [0, 0.0]); e[0] += 1; e[1] += m
    nb = 9                                             # the launches of block 14, in order
    return dict(n_blocks=n_blocks, launches=len(med), kernel_sum_ms_median=sums[len(sums) // 2], kernel_sum_ms_min=sums[0], frame_wall_ms_median=statistics.median(wall),
                frame_wall_ms_min=min(wall), by_kind={k: dict(launches=c, ms=m) for k, (c, m) in by_kind.items()},
                block_14_ms=[round(m, 4) for _, m in med[1 + 13 * nb:1 + 14 * nb]], workspace_bytes=int(ws.numel()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "one_launch_1x1080x1920": one_launch(dev, args.rounds)}
    res["sclk_mhz_after_launches"] = shader_clock_mhz()
    res["frame_1080p_x4"] = frame(dev, max(3, args.rounds // 6))
    res["sclk_mhz_after_frame"] = shader_clock_mhz()
    txt = json.dumps(res, indent=1)
    print(txt)
    if args.out:
        with open(args.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
